// Host build of sr_diffuse_field_kernel's own text (spectrobot_amd/csrc/sr_diffuse_source.inc, the file the library
// compiles) behind tools/host_sim/hip_on_host.hpp: the kernel has no barrier, so a block's lanes run one after the other.
// Every buffer has exactly the size the entry gives it, so that AddressSanitizer sees an index beyond it -- the workspace
// included, [4][n_layers][points rounded up to 256], and temps [n_layers]; the night instances get NULL for beam and sun and
// the instances without the thermal source NULL for temps, so that a read of either is a fault --; the outputs start as
// NaN (or, accumulating, as a known pattern), so that the comparison sees a place that was not written.  Against plain
// loops in long double on two panels of n_layers 1, 2, 3, 17, 80 x n_gas 1, 3, 8 x n_pts 1, 63, 65, 257, with empty layers,
// conservative layers (co = 0; alpha == 0: no thermal source), a beam that falls by up to e^-30 and albedos 0, 1 and
// between:
//   the source panel of tests/test_gpu_diffuse_source.py, the sun alone, to the bound of tests/diffuse_source_reference.py,
//     b = eps (n_gas + 16 n_layers + 16) |ref|;
//   the thermal panel of tests/test_gpu_diffuse_thermal.py, thermal alone and with the sun, own_emission off and on,
//     temperatures of 70 .. 200 K, nu in 500 .. 3300 cm^-1, a surface that emits or not, to the bound of
//     tests/diffuse_thermal_reference.py, b = eps (n_gas + 16 n_layers + 24 + 2 x_max) |ref|.
// The instance with every output runs on the whole panel of its kind, the other seven of each kind on the panel's corners,
// which must give the same bits: twenty-four in all; a call in two point chunks (p_lo > 0) against the call in one; and on
// the thermal panel's corners with every ssa 1 (alpha exactly 0), no surface and own off, the instance with both sources
// against the sun's alone: the same bytes.  exp, expm1 and sqrt here are the host's (the device routines are pinned on the
// GPU).  Built with AddressSanitizer and UBSan by tools/host_sim/run.sh diffuse_source_host -- indexing, the workspace and
// the sweeps on a machine without a GPU, not the compiled gfx950 code.
#include "hip_on_host.hpp"
#include "sr_solar_plan.hpp"
namespace sr {
#include "sr_diffuse_source.inc"
}
using namespace sr;

typedef long double LDb;

struct Case {
  int n_layers, n_gas, n_pts, g_lo;
  std::vector<double> A, V, ssa, asym, beam, sun, temps; // temps empty: a case of the source panel
  double mu0, albedo, t_surface, w0, step;
};

// one generator for both panels; the thermal panel's draws (g_lo, the surface, the grid, the temperatures) stand where
// its cases have always made them
static Case make_case(int N, int n_gas, int n_pts, unsigned seed, bool thermal) {
  std::mt19937_64 rng(seed);
  std::uniform_real_distribution<double> R(0.0, 1.0);
  Case c{N, n_gas, n_pts, 0, {}, {}, {}, {}, {}, {}, {}, 0.0, 0.0, 0.0, 0.0, 0.01};
  if (thermal) c.g_lo = (int)(5000 * R(rng));
  c.mu0 = -0.3 + 1.3 * R(rng);
  const int pick = (int)(3 * R(rng));
  c.albedo = pick == 0 ? 0.0 : pick == 1 ? 1.0 : R(rng);
  if (thermal) {
    c.t_surface = R(rng) < 0.4 ? 0.0 : 70.0 + 130.0 * R(rng);
    c.w0 = std::floor(500.0 + R(rng) * (2800.0 - (c.g_lo + n_pts) * c.step));
    c.temps.resize(N);
  }
  const bool cons = R(rng) < 0.15;
  const int n_sca = n_gas == 1 ? 1 : 1 + (int)(R(rng) * std::min(n_gas, 3)) % std::min(n_gas, 3);
  c.ssa.assign(n_gas, 0.0);
  c.asym.assign(n_gas, 0.0);
  for (int g = 0; g < n_sca; ++g) c.ssa[g] = cons ? 1.0 : 0.3 + 0.7 * R(rng), c.asym[g] = -0.5 + 1.45 * R(rng);
  const double total = std::exp(std::log(1e-8) + R(rng) * std::log(80.0 / 1e-8));
  c.V.assign((size_t)n_gas * N, 0.0);
  for (int l = 0; l < N; ++l) {
    if (thermal) c.temps[l] = 70.0 + 130.0 * R(rng);
    if (R(rng) < 0.1) continue; // an empty layer
    const double share = total * (0.2 + R(rng)) / N;
    for (int g = 0; g < n_sca; ++g) c.V[(size_t)g * N + l] = share * (0.1 + R(rng)) / n_sca;
    if (!cons)
      for (int g = n_sca; g < n_gas; ++g) c.V[(size_t)g * N + l] = share * std::exp(std::log(1e-14) * R(rng));
  }
  c.A.resize((size_t)n_gas * N * n_pts);
  for (double &x : c.A) x = 0.15 + 1.35 * R(rng);
  const double depth = 30.0 * R(rng);
  c.beam.resize((size_t)(N + 1) * n_pts);
  for (int r = 0; r <= N; ++r)
    for (int j = 0; j < n_pts; ++j) c.beam[(size_t)r * n_pts + j] = std::exp(-depth * (r == N ? 1.0 : (N - 0.5 - r) / (N + 1.0))) * (0.9 + 0.1 * R(rng));
  c.sun.resize(n_pts);
  for (double &x : c.sun) x = 5.0 + 15.0 * R(rng);
  return c;
}

struct Out { std::vector<double> emi, J, F; };

// the entry's host side: the padded coefficients, the workspace, one launch per chunk of `chunk` points; what an instance
// must not read is NULL or NaN
template <bool SOLAR, bool THERMAL, bool ACC, bool WJ, bool WF> static void run_kernel(const Case &c, bool own, int chunk, Out &o) {
  std::vector<double> coef(3 * kDiffuseGases, 0.0); // (its own allocation: coef[kDiffuseGases + out_gas] is read too)
  for (int g = 0; g < c.n_gas; ++g) {
    const double f = c.asym[g] > 0.0 ? c.asym[g] * c.asym[g] : 0.0;
    coef[g] = c.ssa[g] * (1.0 - f), coef[kDiffuseGases + g] = 1.0 - c.ssa[g], coef[2 * kDiffuseGases + g] = c.ssa[g] * (c.asym[g] - f);
  }
  const int stride = (std::min(chunk, c.n_pts) + 255) / 256 * 256;
  std::vector<double> ws((size_t)4 * c.n_layers * stride, NAN);
  for (int p_lo = 0; p_lo < c.n_pts; p_lo += chunk) {
    const int p_hi = std::min(c.n_pts, p_lo + chunk), n_pb = (p_hi - p_lo + 255) / 256;
    launch((unsigned)((n_pb + 7) / 8 * 8), 1, [&] {
      sr_diffuse_field_kernel<SOLAR, THERMAL, ACC, WJ, WF>(
          c.A.data(), c.n_gas, c.n_layers, c.n_pts, p_lo, p_hi, c.V.data(), coef.data(), THERMAL ? c.temps.data() : nullptr,
          SOLAR ? c.beam.data() : nullptr, SOLAR ? c.sun.data() : nullptr, SOLAR ? c.mu0 : (double)NAN, c.albedo,
          THERMAL ? c.t_surface : (double)NAN, THERMAL ? c.w0 : (double)NAN, THERMAL ? c.step : (double)NAN, c.g_lo, (int)own, 0,
          ws.data(), stride, o.emi.data(), WJ ? o.J.data() : nullptr, WF ? o.F.data() : nullptr);
    });
  }
}

static double pattern(size_t at) { return 1e-3 * (1.0 + (double)(at % 17)); }

static Out fresh(const Case &c, bool acc) {
  Out o;
  o.emi.resize((size_t)c.n_layers * c.n_pts);
  for (size_t at = 0; at < o.emi.size(); ++at) o.emi[at] = acc ? pattern(at) : (double)NAN;
  o.J.assign((size_t)c.n_layers * c.n_pts, NAN);
  o.F.assign((size_t)2 * (c.n_layers + 1) * c.n_pts, NAN);
  return o;
}

static bool same(const Out &a, const Out &b) {
  return !std::memcmp(a.emi.data(), b.emi.data(), a.emi.size() * sizeof(double)) &&
         !std::memcmp(a.J.data(), b.J.data(), a.J.size() * sizeof(double)) && !std::memcmp(a.F.data(), b.F.data(), a.F.size() * sizeof(double));
}

static LDb planck(const Case &c, int j, double T) {
  const LDb nu = c.w0 + (double)(c.g_lo + j) * c.step; // (the double the kernel forms, taken as exact)
  return 2 * (LDb)kHcgs * ((LDb)kCcgs * kCcgs) * (nu * nu * nu) / (std::exp((LDb)kC2 * nu / T) - 1);
}

// plain loops in long double, point by point: F [2][N + 1], J [N], B [N] (0 without the thermal source)
static void plain(const Case &c, bool solar, bool thermal, int j, std::vector<LDb> &F, std::vector<LDb> &J, std::vector<LDb> &B) {
  const int N = c.n_layers;
  const LDb r3 = std::sqrt((LDb)3), pi = std::acos((LDb)-1), kth = 2 * pi / r3, mu0 = solar ? c.mu0 : 0, alb = c.albedo,
            sun = solar ? c.sun[j] : 0;
  std::vector<LDb> tq(N), cq(N), rb(N), ub(N);
  B.assign(N, 0);
  LDb Rb = alb, Cb = 1 - alb, Ub = solar ? alb * (std::max(mu0, (LDb)0) * (sun * c.beam[(size_t)N * c.n_pts + j])) : 0;
  if (thermal && c.t_surface > 0) Ub += (1 - alb) * kth * planck(c, j, c.t_surface);
  for (int l = 0; l < N; ++l) {
    if (thermal) B[l] = planck(c, j, c.temps[l]);
    LDb sig = 0, al = 0, sf = 0, sg = 0;
    for (int g = 0; g < c.n_gas; ++g) {
      const LDb t = (LDb)c.V[(size_t)g * N + l] * c.A[((size_t)g * N + l) * c.n_pts + j], as = c.asym[g], f = as > 0 ? as * as : 0;
      sig += c.ssa[g] * t, al += (1 - (LDb)c.ssa[g]) * t, sf += c.ssa[g] * f * t, sg += c.ssa[g] * as * t;
    }
    const LDb sp = sig - sf, dtau = sp + al;
    LDb R = 0, T = 1, Ep = 0, Em = 0, oneR = 1, ab = 0, q = 1;
    if (dtau > 0) {
      const LDb co = std::max(al / dtau, std::ldexp((LDb)1, -52)), om = 1 - co, g = sp > 0 ? (sg - sf) / sp : 0;
      const LDb d = r3 * co, s = r3 * (1 - om * g), sd = std::sqrt(d), ss = std::sqrt(s), k = sd * ss, g1 = (s + d) / 2, g2 = r3 * om * (1 - g) / 2;
      const LDb Gm = g2 / (g1 + k), u = sd * (sd + ss) / (g1 + k), e = std::exp(-k * dtau), m = -std::expm1(-k * dtau);
      const LDb ge = 1 + Gm * e, den = (u + Gm * m) * ge, D = solar ? sun * c.beam[(size_t)l * c.n_pts + j] : 0;
      R = Gm * m * (1 + e) / den, T = e * u * (1 + Gm) / den, oneR = u * (1 + Gm * e * e) / den, ab = m * u * (1 - Gm * e) / den;
      const LDb oneT = m * (u + Gm * ge) / den, es = om * D * (sd + ss) / (g1 + k) * (m / sd) / ge, ed = -(om * D * r3 * g * mu0) / s * (oneT + R);
      const LDb eth = al > 0 ? kth * B[l] * (m * u / ge) : 0; // 1 - R - T without the subtraction
      Ep = (es + ed) / 2 + eth, Em = (es - ed) / 2 + eth, q = 1 / (Cb + Rb * oneR);
    }
    tq[l] = T * q, cq[l] = (Em + R * Ub) * q, rb[l] = Rb, ub[l] = Ub;
    Ub = Ep + T * (Ub + Rb * Em) * q;
    Cb = (oneR * Cb + Rb * ab * (oneR + T)) * q;
    Rb = R + T * T * Rb * q;
  }
  F.assign(2 * (N + 1), 0);
  J.assign(N, 0);
  F[N] = Ub;
  const LDb kJ = r3 / (8 * pi);
  for (int l = N - 1; l >= 0; --l) {
    F[N + 1 + l] = tq[l] * F[N + 1 + l + 1] + cq[l];
    F[l] = ub[l] + rb[l] * F[N + 1 + l];
    J[l] = kJ * ((F[l] + F[N + 1 + l]) + (F[l + 1] + F[N + 1 + l + 1]));
  }
}

static int check_all_outputs(const Case &c, bool solar, bool thermal, bool own, const Out &o, bool acc) {
  const int N = c.n_layers;
  double tmin = c.t_surface > 0 ? c.t_surface : 1e9;
  for (double t : c.temps) tmin = std::min(tmin, t);
  const LDb eps = std::ldexp((LDb)1, -53);
  const LDb f0 = c.asym[0] > 0 ? (LDb)c.asym[0] * c.asym[0] : 0, w = c.ssa[0] * (1 - f0), wa = 1 - (LDb)c.ssa[0];
  int bad = 0;
  std::vector<LDb> F, J, B;
  for (int j = 0; j < c.n_pts; ++j) {
    const LDb xmax = (LDb)kC2 * (c.w0 + (double)(c.g_lo + j) * c.step) / tmin; // (the thermal panel's allowance for B)
    const LDb fac = eps * (thermal ? c.n_gas + 16 * N + 24 + 2 * xmax : c.n_gas + 16 * N + 16);
    plain(c, solar, thermal, j, F, J, B);
    for (int i = 0; i < 2 * (N + 1); ++i) {
      const double v = o.F[(size_t)i * c.n_pts + j];
      if (!(std::fabs((LDb)v - F[i]) <= fac * F[i]) || v < 0) {
        if (bad++ < 10) std::printf("flux %d point %d: %.17g, plain %.17Lg\n", i, j, v, F[i]);
      }
    }
    for (int l = 0; l < N; ++l) {
      const size_t at = (size_t)l * c.n_pts + j;
      const LDb e = own ? c.A[at] * (wa * B[l] + w * J[l]) : w * c.A[at] * J[l], base = acc ? pattern(at) : 0;
      const bool ok = std::fabs((LDb)o.J[at] - J[l]) <= fac * J[l] && std::fabs((LDb)o.emi[at] - (base + e)) <= fac * e + eps * (base + e);
      if (!ok && bad++ < 10) std::printf("layer %d point %d: J %.17g plain %.17Lg, emi %.17g plain %.17Lg\n", l, j, o.J[at], J[l], o.emi[at], base + e);
    }
  }
  return bad;
}

template <bool SOLAR, bool THERMAL, bool ACC, bool WJ, bool WF> static int same_bits(const Case &c, bool own, const Out &full) {
  Out o = fresh(c, ACC);
  run_kernel<SOLAR, THERMAL, ACC, WJ, WF>(c, own, 1 << 30, o);
  int bad = 0;
  if (!ACC && std::memcmp(o.emi.data(), full.emi.data(), o.emi.size() * sizeof(double))) ++bad;
  if (WJ && std::memcmp(o.J.data(), full.J.data(), o.J.size() * sizeof(double))) ++bad;
  if (WF && std::memcmp(o.F.data(), full.F.data(), o.F.size() * sizeof(double))) ++bad;
  for (size_t at = 0; at < o.J.size(); ++at) bad += (!WJ && !std::isnan(o.J[at]));   // an output that was not asked for stays untouched
  for (size_t at = 0; at < o.F.size(); ++at) bad += (!WF && !std::isnan(o.F[at]));
  if (ACC)
    for (size_t at = 0; at < o.emi.size(); ++at) bad += !(o.emi[at] == pattern(at) + full.emi[at]); // overwrite plus base, one rounding
  if (bad) std::printf("instance <%d, %d, %d, %d, %d> differs from the full instance\n", (int)SOLAR, (int)THERMAL, (int)ACC, (int)WJ, (int)WF);
  return bad;
}

template <bool SOLAR, bool THERMAL> static int run_kind(const Case &c, bool own, bool corner, bool chunks) {
  Out full = fresh(c, false);
  run_kernel<SOLAR, THERMAL, false, true, true>(c, own, 1 << 30, full);
  int bc = check_all_outputs(c, SOLAR, THERMAL, own, full, false);
  if (corner) {
    bc += same_bits<SOLAR, THERMAL, false, false, false>(c, own, full) + same_bits<SOLAR, THERMAL, false, true, false>(c, own, full) +
          same_bits<SOLAR, THERMAL, false, false, true>(c, own, full);
    bc += same_bits<SOLAR, THERMAL, true, false, false>(c, own, full) + same_bits<SOLAR, THERMAL, true, true, false>(c, own, full) +
          same_bits<SOLAR, THERMAL, true, false, true>(c, own, full);
    bc += same_bits<SOLAR, THERMAL, true, true, true>(c, own, full);
    Out acc = fresh(c, true);
    run_kernel<SOLAR, THERMAL, true, true, true>(c, own, 1 << 30, acc);
    bc += check_all_outputs(c, SOLAR, THERMAL, own, acc, true);
  }
  if (chunks) { // two point chunks, the second from p_lo = 256 on: the same bits
    Out two = fresh(c, false);
    run_kernel<SOLAR, THERMAL, false, true, true>(c, own, 256, two);
    if (!same(two, full)) {
      std::printf("two point chunks differ from one\n");
      ++bc;
    }
  }
  return bc;
}

// a thermal source of exactly 0 (alpha == 0 in every layer, no surface, own off): both sources give the sun's bytes
static int zero_thermal_is_solar(Case c) {
  std::fill(c.ssa.begin(), c.ssa.end(), 1.0);
  c.t_surface = 0.0;
  Out both = fresh(c, false), solar = fresh(c, false);
  run_kernel<true, true, false, true, true>(c, false, 1 << 30, both);
  run_kernel<true, false, false, true, true>(c, false, 1 << 30, solar);
  if (same(both, solar)) return 0;
  std::printf("<1, 1, 0, 1, 1> with a thermal source of 0 differs from <1, 0, 0, 1, 1>\n");
  return 1;
}

int main() {
  const int layers[] = {1, 2, 3, 17, 80}, gases[] = {1, 3, 8}, pts[] = {1, 63, 65, 257};
  int bad = 0, n = 0;
  for (int thermal = 0; thermal < 2; ++thermal) {
    unsigned seed = thermal ? 20261022 : 20261021;
    for (int a = 0; a < 5; ++a)
      for (int b = 0; b < 3; ++b)
        for (int d = 0; d < 4; ++d) {
          const Case c = make_case(layers[a], gases[b], pts[d], seed++, thermal != 0);
          const bool corner = ((a == 0 || a == 4) && (b == 0 || b == 2) && (d == 0 || d == 3)) || (a == 3 && b == 1 && d == 2);
          int bc = 0;
          if (!thermal) bc += run_kind<true, false>(c, false, corner, pts[d] == 257);
          for (int own = 0; thermal && own < 2; ++own)
            bc += run_kind<false, true>(c, own != 0, corner, pts[d] == 257) + run_kind<true, true>(c, own != 0, corner, pts[d] == 257);
          if (thermal && corner) bc += zero_thermal_is_solar(c);
          if (bc) std::printf("%s panel, n_layers %d n_gas %d n_pts %d: FAILED\n", thermal ? "thermal" : "source", layers[a], gases[b], pts[d]);
          bad += bc;
          ++n;
        }
  }
  std::printf(bad ? "FAILED\n" : "all %d cases ok\n", n);
  return bad ? 1 : 0;
}
