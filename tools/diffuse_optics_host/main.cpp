// Host build of sr_diffuse_tangent_kernel's optics instance (OPT: a direction in ssa, asym and the surface albedo) and of
// sr_diffuse_contract_kernel (spectrobot_amd/csrc/sr_diffuse_jac.inc, the file the library compiles, behind
// sr_diffuse_source.inc) with tools/host_sim/hip_on_host.hpp, the twin of tools/diffuse_jacobian_host: every buffer has
// exactly the size the entry gives it, so that AddressSanitizer sees an index beyond it -- the staged dopt
// [n_par][kDiffuseOpt] and the workspace included --; the outputs start as NaN (or, accumulating, as a known pattern), and
// the rows of jac that no parameter names must keep their bits.
// Against plain loops in long double that are independent of the kernel's tangent formulas and of the host plan's
// coefficient tangents: forward-mode differentiation (a value and its tangent through every statement) of the
// definition's sums from ssa, asym and f = max(asym, 0)^2 as dual numbers, of diffuse_layer's OWN closed forms and of the
// adding recurrences as sr_diffuse_source.inc states them from a dual albedo on, Cb carried.  Those forms lose digits near
// co's floor and under thick layers, so the cases here keep co = 0 exactly or >= 1e-3 and the column's optical depth below
// 3, and the tolerance is eps (n_gas + 128 n_layers + 16) of the column's largest |dJ|, of the direction or of its five
// parts' magnitudes added (the direction in the scattering sums, the absorption sum, the asymmetry sum, the albedo, the
// beam; times sum_l q for jac).  Cases: n_layers 1, 2, 3, 17, 80 x n_gas 1, 3, 8
// x n_pts 1, 63, 65, 257 with n_par 1, 2, 5, 9 and n_rays 1, 8, 9 dealt over them, empty layers, the three kinds of
// direction alone and mixed, an albedo-only parameter (an empty layer range) and one without dlnbeam; every instance
// (overwrite / accumulate, with and without q, with and without dj_out, dlnbeam null), a call in two point chunks
// (p_lo > 0) and a call in parameter tiles of one tile per launch, which must give the bits of the call in one.
// Built with AddressSanitizer and UBSan by tools/host_sim/run.sh diffuse_optics_host -- indexing, the workspace, the
// tiles and the sweeps on a machine without a GPU, not the compiled gfx950 code.
#include "hip_on_host.hpp"
#include "sr_solar_plan.hpp"
namespace sr {
#include "sr_diffuse_source.inc"
#include "sr_diffuse_jac.inc"
}
using namespace sr;

typedef long double LDb;
constexpr int NP = kDiffuseJacPars, NR = kDiffuseJacRays;

struct Case {
  int n_layers, n_gas, n_pts, n_par, n_rays, n_rows;
  std::vector<double> A, V, ssa, asym, beam, sun, dssa, dasym, dalb, dlnb, q;
  std::vector<int> slot;
  double mu0, albedo;
};

static Case make_case(int N, int n_gas, int n_pts, int n_par, int n_rays, unsigned seed) {
  std::mt19937_64 rng(seed);
  std::uniform_real_distribution<double> R(0.0, 1.0);
  Case c{N, n_gas, n_pts, n_par, n_rays, n_par + 2, {}, {}, {}, {}, {}, {}, {}, {}, {}, {}, {}, {}, -0.3 + 1.3 * R(rng), 0.0};
  const int pick = (int)(3 * R(rng));
  c.albedo = pick == 0 ? 0.0 : pick == 1 ? 1.0 : R(rng);
  const bool cons = R(rng) < 0.15;
  const int n_sca = n_gas == 1 ? 1 : 1 + (int)(R(rng) * std::min(n_gas, 3)) % std::min(n_gas, 3);
  c.ssa.assign(n_gas, 0.0);
  c.asym.assign(n_gas, 0.0);
  for (int g = 0; g < n_sca; ++g) c.ssa[g] = cons ? 1.0 : 0.3 + 0.7 * R(rng), c.asym[g] = -0.5 + 1.45 * R(rng);
  const double total = std::exp(std::log(1e-4) + R(rng) * std::log(3.0 / 1e-4));
  c.V.assign((size_t)n_gas * N, 0.0);
  std::vector<int> filled;
  for (int l = 0; l < N; ++l) {
    if (N > 1 && R(rng) < 0.1) continue; // an empty layer
    filled.push_back(l);
    const double share = total * (0.2 + R(rng)) / N;
    for (int g = 0; g < n_sca; ++g) c.V[(size_t)g * N + l] = share * (0.1 + R(rng)) / n_sca;
    if (!cons)
      for (int g = n_sca; g < n_gas; ++g) c.V[(size_t)g * N + l] = share * std::exp(std::log(1e-3) * R(rng));
  }
  if (!cons && n_sca == n_gas) // no absorber slot: the scatterers absorb, co >= 1e-3
    for (int g = 0; g < n_sca; ++g) c.ssa[g] = std::min(c.ssa[g], 0.998);
  c.A.resize((size_t)n_gas * N * n_pts);
  for (double &x : c.A) x = 0.15 + 1.35 * R(rng);
  const double depth = 10.0 * R(rng);
  c.beam.resize((size_t)(N + 1) * n_pts);
  for (int r = 0; r <= N; ++r)
    for (int j = 0; j < n_pts; ++j) c.beam[(size_t)r * n_pts + j] = std::exp(-depth * (r == N ? 1.0 : (N - 0.5 - r) / (N + 1.0))) * (0.9 + 0.1 * R(rng));
  c.sun.resize(n_pts);
  for (double &x : c.sun) x = 5.0 + 15.0 * R(rng);
  // directions: parameter p moves ssa of one gas (p % 3 == 0), asym of one gas (1) or the albedo alone (2: an empty layer
  // range); from the fourth on every third moves all three on every gas; parameter 2 has no dlnbeam
  c.dssa.assign((size_t)n_par * n_gas, 0.0);
  c.dasym.assign((size_t)n_par * n_gas, 0.0);
  c.dalb.assign((size_t)n_par, 0.0);
  c.dlnb.resize((size_t)n_par * (N + 1) * n_pts);
  for (double &x : c.dlnb) x = 2.0 * R(rng) - 1.0;
  auto size = [&] { return (R(rng) < 0.5 ? -1.0 : 1.0) * (0.2 + 0.8 * R(rng)); };
  for (int p = 0; p < n_par; ++p) {
    if (p == 2) std::fill(c.dlnb.begin() + (size_t)p * (N + 1) * n_pts, c.dlnb.begin() + (size_t)(p + 1) * (N + 1) * n_pts, 0.0);
    const int g = (int)(R(rng) * n_gas) % n_gas;
    if (p >= 3 && p % 3 == 0) {
      for (int h = 0; h < n_gas; ++h) c.dssa[(size_t)p * n_gas + h] = size(), c.dasym[(size_t)p * n_gas + h] = size();
      c.dalb[p] = size();
    } else if (p % 3 == 0) {
      c.dssa[(size_t)p * n_gas + g] = size();
    } else if (p % 3 == 1) {
      c.dasym[(size_t)p * n_gas + g] = size();
    } else {
      c.dalb[p] = size();
    }
  }
  c.q.resize((size_t)n_rays * N * n_pts);
  for (double &x : c.q) x = 0.1 + 0.9 * R(rng);
  c.slot.resize(n_par);
  for (int p = 0; p < n_par; ++p) c.slot[p] = n_par - p; // rows n_par .. 1: row 0 and the last stay unnamed
  return c;
}

struct Out { std::vector<double> jac, dJ; };
static double pattern(size_t at) { return 1e-3 * (1.0 + (double)(at % 17)); }

static Out fresh(const Case &c, bool acc) {
  Out o;
  o.jac.resize((size_t)c.n_rays * c.n_rows * c.n_pts);
  for (size_t at = 0; at < o.jac.size(); ++at) o.jac[at] = acc ? pattern(at) : (double)NAN;
  o.dJ.assign((size_t)c.n_par * c.n_layers * c.n_pts, NAN);
  return o;
}

// the entry's host side: the padded coefficients, the masks, the workspace, a tangent and a contraction launch per
// (chunk of `chunk` points, group of `tiles` parameter tiles)
static void run_entry(const Case &c, int chunk, int tiles, bool with_q, bool with_dj, bool acc, bool with_beam, Out &o) {
  double coef[3 * kDiffuseGases] = {0.0};
  for (int g = 0; g < c.n_gas; ++g) {
    const double f = c.asym[g] > 0.0 ? c.asym[g] * c.asym[g] : 0.0;
    coef[g] = c.ssa[g] * (1.0 - f), coef[kDiffuseGases + g] = 1.0 - c.ssa[g], coef[2 * kDiffuseGases + g] = c.ssa[g] * (c.asym[g] - f);
  }
  std::vector<int> mask;
  std::vector<double> dopt; // exactly [n_par][kDiffuseOpt], as the entry stages it
  if (!diffuse_optics_plan(c.V.data(), c.ssa.data(), c.asym.data(), c.dssa.data(), c.dasym.data(), c.dalb.data(), c.n_par, c.n_gas,
                           c.n_layers, dopt, mask))
    std::abort();
  for (int p = 0; p < c.n_par; ++p) { // an albedo-only parameter has an empty range, a gas's direction the layers of its column
    bool gas = false;
    for (int g = 0; g < c.n_gas; ++g) gas |= c.dssa[(size_t)p * c.n_gas + g] != 0.0 || c.dasym[(size_t)p * c.n_gas + g] != 0.0;
    if (!gas && mask[2 * p + 1] != 0) std::abort();
  }
  const int N = c.n_layers, n_tiles = (c.n_par + NP - 1) / NP;
  tiles = std::min(tiles, n_tiles);
  const int stride = (std::min(chunk, c.n_pts) + 255) / 256 * 256;
  const bool dj_ws = with_q && !with_dj;
  const size_t sweep = (size_t)tiles * (3 + 4 * NP) * N * stride;
  std::vector<double> ws(sweep + (dj_ws ? (size_t)tiles * NP * N * stride : 0), NAN);
  for (int p_lo = 0; p_lo < c.n_pts; p_lo += chunk) {
    const int p_hi = std::min(c.n_pts, p_lo + chunk), n_pb = (p_hi - p_lo + 255) / 256;
    for (int t0 = 0; t0 < n_tiles; t0 += tiles) {
      const int par_lo = t0 * NP, par_hi = std::min(c.n_par, (t0 + tiles) * NP), nt = (par_hi - par_lo + NP - 1) / NP;
      double *dj = dj_ws ? ws.data() + sweep : o.dJ.data();
      const int dj_stride = dj_ws ? stride : c.n_pts, dj_joff = dj_ws ? p_lo : 0, dj_par0 = dj_ws ? par_lo : 0;
      launch((unsigned)((n_pb + 7) / 8 * 8) * nt, 1, [&] {
        sr_diffuse_tangent_kernel<NP, true>(c.A.data(), c.n_gas, N, c.n_pts, p_lo, p_hi, par_lo, par_hi, c.V.data(), dopt.data(), coef, mask.data(),
                                      c.beam.data(), c.sun.data(), with_beam ? c.dlnb.data() : nullptr, c.mu0, c.albedo, ws.data(), stride, dj,
                                      dj_stride, dj_joff, dj_par0);
      });
      if (!with_q) continue;
      const unsigned items = (unsigned)nt * ((c.n_rays + NR - 1) / NR);
      launch((unsigned)((n_pb + 7) / 8 * 8) * items, 1, [&] {
        if (acc)
          sr_diffuse_contract_kernel<NR, NP, true>(c.q.data(), c.n_rays, N, c.n_pts, p_lo, p_hi, par_lo, par_hi, dj, dj_stride, dj_joff, dj_par0,
                                                   c.slot.data(), o.jac.data(), c.n_rows);
        else
          sr_diffuse_contract_kernel<NR, NP, false>(c.q.data(), c.n_rays, N, c.n_pts, p_lo, p_hi, par_lo, par_hi, dj, dj_stride, dj_joff, dj_par0,
                                                    c.slot.data(), o.jac.data(), c.n_rows);
      });
    }
  }
}

// a value and its tangent
struct Du {
  LDb v, d;
  Du(LDb v_ = 0, LDb d_ = 0) : v(v_), d(d_) {}
};
static Du operator+(Du a, Du b) { return {a.v + b.v, a.d + b.d}; }
static Du operator-(Du a, Du b) { return {a.v - b.v, a.d - b.d}; }
static Du operator-(Du a) { return {-a.v, -a.d}; }
static Du operator*(Du a, Du b) { return {a.v * b.v, a.d * b.v + a.v * b.d}; }
static Du operator/(Du a, Du b) { return {a.v / b.v, (a.d - a.v / b.v * b.d) / b.v}; }
static Du dsqrt(Du a) { const LDb s = std::sqrt(a.v); return {s, a.d / (2 * s)}; }
static Du dexp(Du a) { const LDb e = std::exp(a.v); return {e, e * a.d}; }
static Du dexpm1(Du a) { return {std::expm1(a.v), std::exp(a.v) * a.d}; }

// plain loops in long double, one point and one parameter: dJ [N].  part < 0: the direction; part 0 .. 4: one of its five
// parts alone -- the direction as it enters the scattering sums (sigma, sigma_f), the absorption sum, the asymmetry sum,
// the albedo, the beam -- whose tangents, added as magnitudes, are the scale of the tolerance: a gas's ssa moves
// scattering and absorption against each other (at ssa = 1 and asym <= 0 the whole direction is null: the floor holds co,
// dtau and g stand still), and the kernel rounds the three coefficients' tangents before it forms the sums
constexpr int kParts = 5;
static void plain(const Case &c, int p, int j, bool with_beam, int part, std::vector<LDb> &dJ) {
  const int N = c.n_layers;
  const LDb r3 = std::sqrt((LDb)3), mu0 = c.mu0, sun = c.sun[j];
  auto on = [&](int k) { return part < 0 || part == k; };
  auto lnb = [&](int row) { return with_beam && on(4) ? (LDb)c.dlnb[((size_t)p * (N + 1) + row) * c.n_pts + j] : (LDb)0; };
  std::vector<Du> tq(N), cq(N), rb(N), ub(N);
  const Du alb(c.albedo, on(3) ? (LDb)c.dalb[p] : (LDb)0);
  const LDb lit = std::max(mu0, (LDb)0) * (sun * c.beam[(size_t)N * c.n_pts + j]);
  Du Rb = alb, Cb = Du(1) - alb, Ub = alb * Du(lit, lit * lnb(N));
  for (int l = 0; l < N; ++l) {
    Du sig, al, sf, sg;
    for (int g = 0; g < c.n_gas; ++g) {
      const LDb a = c.A[((size_t)g * N + l) * c.n_pts + j];
      const LDb ds = c.dssa[(size_t)p * c.n_gas + g], da = c.dasym[(size_t)p * c.n_gas + g];
      auto ssa = [&](int k) { return Du(c.ssa[g], on(k) ? ds : (LDb)0); };
      auto as = [&](int k) { return Du(c.asym[g], on(k) ? da : (LDb)0); };
      const Du f = c.asym[g] > 0 ? as(0) * as(0) : Du(0), t((LDb)c.V[(size_t)g * N + l] * a);
      sig = sig + ssa(0) * t, al = al + (Du(1) - ssa(1)) * t, sf = sf + ssa(0) * f * t, sg = sg + ssa(2) * as(2) * t;
    }
    const Du sp = sig - sf, dtau = sp + al;
    Du R(0), T(1), Ep(0), Em(0), oneR(1), ab(0), q(1);
    if (dtau.v > 0) { // (an empty layer: no tangent whatever dv says)
      const LDb floor_ = std::ldexp((LDb)1, -52);
      Du co = al / dtau;
      if (!(co.v > floor_)) co = Du(floor_);
      const Du om = Du(1) - co, g = sp.v > 0 ? (sg - sf) / sp : Du(0);
      const Du d = Du(r3) * co, s = Du(r3) * (Du(1) - om * g), sd = dsqrt(d), ss = dsqrt(s), k = sd * ss, g1 = (s + d) / Du(2), g2 = Du(r3) * om * (Du(1) - g) / Du(2);
      const Du Gm = g2 / (g1 + k), u = sd * (sd + ss) / (g1 + k), e = dexp(-(k * dtau)), m = -dexpm1(-(k * dtau));
      const LDb Dv = sun * c.beam[(size_t)l * c.n_pts + j];
      const Du ge = Du(1) + Gm * e, den = (u + Gm * m) * ge, D(Dv, Dv * lnb(l));
      R = Gm * m * (Du(1) + e) / den, T = e * u * (Du(1) + Gm) / den, oneR = u * (Du(1) + Gm * e * e) / den, ab = m * u * (Du(1) - Gm * e) / den;
      const Du oneT = m * (u + Gm * ge) / den, es = om * D * (sd + ss) / (g1 + k) * (m / sd) / ge, ed = -(om * D * Du(r3 * mu0) * g) / s * (oneT + R);
      Ep = (es + ed) / Du(2), Em = (es - ed) / Du(2), q = Du(1) / (Cb + Rb * oneR);
    }
    tq[l] = T * q, cq[l] = (Em + R * Ub) * q, rb[l] = Rb, ub[l] = Ub;
    Ub = Ep + T * (Ub + Rb * Em) * q;
    Cb = (oneR * Cb + Rb * ab * (oneR + T)) * q;
    Rb = R + T * T * Rb * q;
  }
  dJ.assign(N, 0);
  const LDb kJ = r3 / (8 * std::acos((LDb)-1));
  Du fp = Ub, fm(0);
  for (int l = N - 1; l >= 0; --l) {
    const Du fm_l = tq[l] * fm + cq[l], fp_l = ub[l] + rb[l] * fm_l;
    dJ[l] = kJ * ((fp_l.d + fm_l.d) + (fp.d + fm.d));
    fp = fp_l, fm = fm_l;
  }
}

static int check(const Case &c, const Out &o, bool with_q, bool acc, bool with_beam) {
  const int N = c.n_layers;
  const LDb eps = std::ldexp((LDb)1, -53), fac = eps * (c.n_gas + 128 * N + 16);
  int bad = 0;
  std::vector<LDb> dJ, mag;
  std::vector<int> row_of(c.n_rows, -1);
  for (int p = 0; p < c.n_par; ++p) row_of[c.slot[p]] = p;
  for (int j = 0; j < c.n_pts; ++j)
    for (int p = 0; p < c.n_par; ++p) {
      plain(c, p, j, with_beam, -1, dJ);
      std::vector<LDb> scale(N, 0);
      for (int part = 0; part < kParts; ++part) {
        plain(c, p, j, with_beam, part, mag);
        for (int l = 0; l < N; ++l) scale[l] += std::fabs(mag[l]);
      }
      LDb top = 0;
      for (int l = 0; l < N; ++l) top = std::max(top, std::max(std::fabs(dJ[l]), scale[l]));
      for (int l = 0; l < N; ++l) {
        const double v = o.dJ[((size_t)p * N + l) * c.n_pts + j];
        if (!(std::fabs((LDb)v - dJ[l]) <= fac * top) && bad++ < 10) std::printf("dJ par %d layer %d point %d: %.17g, plain %.17Lg (largest %.3Lg)\n", p, l, j, v, dJ[l], top);
      }
      if (!with_q) continue;
      for (int y = 0; y < c.n_rays; ++y) {
        LDb sum = 0, qsum = 0;
        for (int l = 0; l < N; ++l) {
          const LDb qv = c.q[((size_t)y * N + l) * c.n_pts + j];
          sum += qv * dJ[l], qsum += qv;
        }
        const size_t at = ((size_t)y * c.n_rows + c.slot[p]) * c.n_pts + j;
        const LDb base = acc ? pattern(at) : 0;
        if (!(std::fabs((LDb)o.jac[at] - (base + sum)) <= fac * qsum * top + eps * std::fabs(base + sum)) && bad++ < 10)
          std::printf("jac ray %d par %d point %d: %.17g, plain %.17Lg\n", y, p, j, o.jac[at], base + sum);
      }
    }
  // rows no parameter names keep their bits
  for (int y = 0; y < c.n_rays && with_q; ++y)
    for (int r = 0; r < c.n_rows; ++r) {
      if (row_of[r] >= 0) continue;
      for (int j = 0; j < c.n_pts; ++j) {
        const size_t at = ((size_t)y * c.n_rows + r) * c.n_pts + j;
        const bool kept = acc ? o.jac[at] == pattern(at) : std::isnan(o.jac[at]);
        if (!kept && bad++ < 10) std::printf("jac ray %d row %d point %d was written\n", y, r, j);
      }
    }
  return bad;
}

static bool same(const std::vector<double> &a, const std::vector<double> &b) { return !std::memcmp(a.data(), b.data(), a.size() * sizeof(double)); }

int main() {
  const int layers[] = {1, 2, 3, 17, 80}, gases[] = {1, 3, 8}, pts[] = {1, 63, 65, 257}, pars[] = {1, 2, 5, 9}, rays[] = {1, 8, 9};
  unsigned seed = 20261023;
  int bad = 0, n = 0;
  for (int a = 0; a < 5; ++a)
    for (int b = 0; b < 3; ++b)
      for (int d = 0; d < 4; ++d) {
        const int n_par = pars[(a + b + d) % 4], n_rays = rays[(a + 2 * b + d) % 3];
        const Case c = make_case(layers[a], gases[b], pts[d], n_par, n_rays, seed++);
        const int all = 1 << 30;
        Out full = fresh(c, false);
        run_entry(c, all, all, true, true, false, true, full);
        int bc = check(c, full, true, false, true);
        { // without dj_out: dJ through the workspace, the same bits of jac and dJ untouched
          Out o = fresh(c, false);
          run_entry(c, all, all, true, false, false, true, o);
          bc += !same(o.jac, full.jac);
          for (double v : o.dJ) bc += !std::isnan(v);
        }
        { // dJ alone
          Out o = fresh(c, false);
          run_entry(c, all, all, false, true, false, true, o);
          bc += !same(o.dJ, full.dJ);
          for (double v : o.jac) bc += !std::isnan(v);
        }
        { // accumulate: base plus the overwrite call's value, one rounding
          Out o = fresh(c, true);
          run_entry(c, all, all, true, true, true, true, o);
          bc += check(c, o, true, true, true);
          for (int p = 0; p < c.n_par; ++p)
            for (int y = 0; y < c.n_rays; ++y)
              for (int j = 0; j < c.n_pts; ++j) {
                const size_t at = ((size_t)y * c.n_rows + c.slot[p]) * c.n_pts + j;
                bc += !(o.jac[at] == pattern(at) + full.jac[at]);
              }
        }
        if ((a + b + d) % 3 == 0) { // the beam held fixed
          Out o = fresh(c, false);
          run_entry(c, all, all, true, true, false, false, o);
          bc += check(c, o, true, false, false);
        }
        if (pts[d] == 257) { // two point chunks, the second from p_lo = 256 on: the same bits, with and without dj_out
          for (int with_dj = 0; with_dj < 2; ++with_dj) {
            Out o = fresh(c, false);
            run_entry(c, 256, all, true, with_dj != 0, false, true, o);
            bc += !same(o.jac, full.jac) + (with_dj && !same(o.dJ, full.dJ));
          }
        }
        if (n_par > NP) { // one parameter tile per launch: the same bits
          for (int with_dj = 0; with_dj < 2; ++with_dj) {
            Out o = fresh(c, false);
            run_entry(c, pts[d] == 257 ? 256 : all, 1, true, with_dj != 0, false, true, o);
            bc += !same(o.jac, full.jac) + (with_dj && !same(o.dJ, full.dJ));
          }
        }
        if (bc) std::printf("n_layers %d n_gas %d n_pts %d n_par %d n_rays %d: FAILED\n", layers[a], gases[b], pts[d], n_par, n_rays);
        bad += bc;
        ++n;
      }
  std::printf(bad ? "FAILED\n" : "all %d cases ok\n", n);
  return bad ? 1 : 0;
}
