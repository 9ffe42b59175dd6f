// Host build of sr_diffuse_columns_kernel's own text (spectrobot_amd/csrc/sr_diffuse_columns.inc, the file the library
// compiles) and of its plan (diffuse_columns_plan, sr_solar_plan.hpp) behind tools/host_sim/hip_on_host.hpp: the kernel
// has no barrier, so a block's lanes run one after the other.  Every buffer has exactly the size the entry gives it, so
// that AddressSanitizer sees an index beyond it -- the workspace included, [2 + 2 NC][n_layers][points rounded up to 256],
// and the padded mu0 [NC] and col_w [n_rows][NC] --; the outputs start as NaN (or, accumulating, as a known pattern), so
// that the comparison sees a place that was not written.  Against plain loops in long double, column by column with the
// unfactored sources, to the bound of tests/diffuse_columns_reference.py, b = eps (n_gas + 16 n_layers + 16) |ref| for J
// and the fluxes and b + eps n_col |ref| for the rows: n_layers 1, 2, 3, 17, 80 x n_gas 1, 3, 8 x n_pts 1, 63, 65, 257 with
// n_col cycling through 1, 2, 3, 5, 8 (every instance; 3 and 5 padded), 2 n_layers + 3 rows in shuffled order (a layer
// without a row, one with several, a row of zero weights, a dense row, the rest two adjacent weights); accumulate against
// overwrite plus base with the zero row's bits kept; the instances without j_out / flux_out / emi_out give the same bits;
// a call in two point chunks (p_lo > 0) against the call in one; columns [a, b, c] against [c, a]: the same bits of a and
// c.  exp, expm1 and sqrt here are the host's.  Built with AddressSanitizer and UBSan by tools/host_sim/run.sh
// diffuse_columns_host -- indexing, the workspace, the plan and the sweeps on a machine without a GPU, not the compiled
// gfx950 code.
#include "hip_on_host.hpp"
#include "sr_solar_plan.hpp"
namespace sr {
#include "sr_diffuse_source.inc"
#include "sr_diffuse_columns.inc"
}
using namespace sr;

typedef long double LDb;

struct Case {
  int n_layers, n_gas, n_pts, n_col, n_rows, n_src;
  std::vector<double> A, V, ssa, asym, beam, sun, mu0, col_w, sca;
  std::vector<int> row_layer, src_row;
  double albedo;
};

static Case make_case(int N, int n_gas, int n_pts, int n_col, unsigned seed) {
  std::mt19937_64 rng(seed);
  std::uniform_real_distribution<double> R(0.0, 1.0);
  Case c{};
  c.n_layers = N, c.n_gas = n_gas, c.n_pts = n_pts, c.n_col = n_col, c.n_rows = 2 * N + 3, c.n_src = N + 1;
  const int pick = (int)(3 * R(rng));
  c.albedo = pick == 0 ? 0.0 : pick == 1 ? 1.0 : R(rng);
  const bool cons = R(rng) < 0.15;
  const int n_sca = n_gas == 1 ? 1 : 1 + (int)(R(rng) * std::min(n_gas, 3)) % std::min(n_gas, 3);
  c.ssa.assign(n_gas, 0.0);
  c.asym.assign(n_gas, 0.0);
  for (int g = 0; g < n_sca; ++g) c.ssa[g] = cons ? 1.0 : 0.3 + 0.7 * R(rng), c.asym[g] = -0.5 + 1.45 * R(rng);
  const double total = std::exp(std::log(1e-8) + R(rng) * std::log(80.0 / 1e-8));
  c.V.assign((size_t)n_gas * N, 0.0);
  for (int l = 0; l < N; ++l) {
    if (R(rng) < 0.1) continue; // an empty layer
    const double share = total * (0.2 + R(rng)) / N;
    for (int g = 0; g < n_sca; ++g) c.V[(size_t)g * N + l] = share * (0.1 + R(rng)) / n_sca;
    if (!cons)
      for (int g = n_sca; g < n_gas; ++g) c.V[(size_t)g * N + l] = share * std::exp(std::log(1e-14) * R(rng));
  }
  c.A.resize((size_t)n_gas * N * n_pts);
  for (double &x : c.A) x = 0.15 + 1.35 * R(rng);
  c.sca.resize((size_t)c.n_src * n_pts);
  for (double &x : c.sca) x = 0.15 + 1.35 * R(rng);
  const double depth = 30.0 * R(rng);
  c.beam.resize((size_t)n_col * (N + 1) * n_pts);
  for (int k = 0; k < n_col; ++k) {
    const double power = n_col == 1 ? 1.0 : 0.5 + 0.75 * k / (n_col - 1);
    c.mu0.push_back(n_col == 1 ? -0.2 + R(rng) : -0.2 + 1.0 * k / (n_col - 1));
    for (int r = 0; r <= N; ++r)
      for (int j = 0; j < n_pts; ++j)
        c.beam[((size_t)k * (N + 1) + r) * n_pts + j] = std::exp(-power * depth * (r == N ? 1.0 : (N - 0.5 - r) / (N + 1.0))) * (0.9 + 0.1 * R(rng));
  }
  c.sun.resize(n_pts);
  for (double &x : c.sun) x = 5.0 + 15.0 * R(rng);
  // the rows: every layer but `none` twice, `three` once more, four more elsewhere; then shuffled
  const int none = N > 1 ? (int)(R(rng) * N) % N : -1, three = N > 1 ? (none + 1 + (int)(R(rng) * (N - 1)) % (N - 1)) % N : 0;
  for (int l = 0; l < N; ++l)
    if (l != none) c.row_layer.push_back(l), c.row_layer.push_back(l);
  c.row_layer.push_back(three);
  while ((int)c.row_layer.size() < c.n_rows) {
    const int l = (int)(R(rng) * N) % N;
    c.row_layer.push_back(l == none ? three : l);
  }
  std::shuffle(c.row_layer.begin(), c.row_layer.end(), rng);
  c.col_w.assign((size_t)c.n_rows * n_col, 0.0);
  for (int r = 0; r < c.n_rows; ++r) {
    c.src_row.push_back((int)(R(rng) * c.n_src) % c.n_src);
    double *w = c.col_w.data() + (size_t)r * n_col;
    if (r == 1) continue; // every weight zero
    if (r == 0 || n_col == 1) {
      for (int k = 0; k < n_col; ++k) w[k] = 0.1 + 0.9 * R(rng);
    } else {
      const int k = (int)(R(rng) * (n_col - 1)) % (n_col - 1);
      const double t = R(rng);
      w[k] = 1.0 - t, w[k + 1] = t;
    }
  }
  return c;
}

struct Out { std::vector<double> emi, J, F; };

static double pattern(size_t at) { return (at % 5 == 0 ? -1.0 : 1.0) * 1e-3 * (double)(at % 17); } // (a -0.0 among them)

static Out fresh(const Case &c, bool acc) {
  Out o;
  o.emi.resize((size_t)c.n_rows * c.n_pts);
  for (size_t at = 0; at < o.emi.size(); ++at) o.emi[at] = acc ? pattern(at) : (double)NAN;
  o.J.assign((size_t)c.n_col * c.n_layers * c.n_pts, NAN);
  o.F.assign((size_t)c.n_col * 2 * (c.n_layers + 1) * c.n_pts, NAN);
  return o;
}

// the entry's host side: the padded coefficients, the plan, the workspace, one launch per chunk of `chunk` points
template <int NC, bool ACC> static void run_instance(const Case &c, int chunk, bool we, bool wj, bool wf, Out &o) {
  double coef[3 * kDiffuseGases] = {0.0};
  for (int g = 0; g < c.n_gas; ++g) {
    const double f = c.asym[g] > 0.0 ? c.asym[g] * c.asym[g] : 0.0;
    coef[g] = c.ssa[g] * (1.0 - f), coef[kDiffuseGases + g] = 1.0 - c.ssa[g], coef[2 * kDiffuseGases + g] = c.ssa[g] * (c.asym[g] - f);
  }
  std::vector<double> mu0p, wp;
  std::vector<int> row_off, row_ix;
  const int n_rows = we ? c.n_rows : 0;
  if (!diffuse_columns_plan(c.mu0.data(), c.col_w.data(), c.row_layer.data(), c.src_row.data(), c.n_col, n_rows, c.n_layers, c.n_src,
                            coef[0] == 0.0, ACC, mu0p, wp, row_off, row_ix) ||
      (int)mu0p.size() != NC) {
    std::printf("the plan refused a valid case\n");
    std::exit(1);
  }
  const int stride = (std::min(chunk, c.n_pts) + 255) / 256 * 256;
  std::vector<double> ws((size_t)(2 + 2 * NC) * c.n_layers * stride, NAN);
  for (int p_lo = 0; p_lo < c.n_pts; p_lo += chunk) {
    const int p_hi = std::min(c.n_pts, p_lo + chunk), n_pb = (p_hi - p_lo + 255) / 256;
    launch((unsigned)((n_pb + 7) / 8 * 8), 1, [&] {
      sr_diffuse_columns_kernel<NC, ACC>(c.A.data(), c.n_gas, c.n_layers, c.n_pts, p_lo, p_hi, c.V.data(), coef, c.beam.data(), c.n_col,
                                         c.sun.data(), mu0p.data(), c.albedo, coef[0], row_off.data(), row_ix.data(), c.src_row.data(),
                                         wp.data(), c.sca.data(), ws.data(), stride, we ? o.emi.data() : nullptr,
                                         wj ? o.J.data() : nullptr, wf ? o.F.data() : nullptr);
    });
  }
}

template <bool ACC> static void run_kernel(const Case &c, int chunk, bool we, bool wj, bool wf, Out &o) {
  switch (diffuse_columns_instance(c.n_col)) {
  case 1: run_instance<1, ACC>(c, chunk, we, wj, wf, o); break;
  case 2: run_instance<2, ACC>(c, chunk, we, wj, wf, o); break;
  case 4: run_instance<4, ACC>(c, chunk, we, wj, wf, o); break;
  default: run_instance<kDiffuseColumns, ACC>(c, chunk, we, wj, wf, o); break;
  }
}

// plain loops in long double for column k, point j: F [2][N + 1], J [N]; the sources unfactored
static void plain(const Case &c, int k, int j, std::vector<LDb> &F, std::vector<LDb> &J) {
  const int N = c.n_layers;
  const double *beam = c.beam.data() + (size_t)k * (N + 1) * c.n_pts;
  const LDb r3 = std::sqrt((LDb)3), mu0 = c.mu0[k], alb = c.albedo, sun = c.sun[j];
  std::vector<LDb> tq(N), cq(N), rb(N), ub(N);
  LDb Rb = alb, Cb = 1 - alb, Ub = alb * (std::max(mu0, (LDb)0) * (sun * beam[(size_t)N * c.n_pts + j]));
  for (int l = 0; l < N; ++l) {
    LDb sig = 0, al = 0, sf = 0, sg = 0;
    for (int g = 0; g < c.n_gas; ++g) {
      const LDb t = (LDb)c.V[(size_t)g * N + l] * c.A[((size_t)g * N + l) * c.n_pts + j], as = c.asym[g], f = as > 0 ? as * as : 0;
      sig += c.ssa[g] * t, al += (1 - (LDb)c.ssa[g]) * t, sf += c.ssa[g] * f * t, sg += c.ssa[g] * as * t;
    }
    const LDb sp = sig - sf, dtau = sp + al;
    LDb R = 0, T = 1, Ep = 0, Em = 0, oneR = 1, ab = 0, q = 1;
    if (dtau > 0) {
      const LDb co = std::max(al / dtau, std::ldexp((LDb)1, -52)), om = 1 - co, g = sp > 0 ? (sg - sf) / sp : 0;
      const LDb d = r3 * co, s = r3 * (1 - om * g), sd = std::sqrt(d), ss = std::sqrt(s), kk = sd * ss, g1 = (s + d) / 2, g2 = r3 * om * (1 - g) / 2;
      const LDb Gm = g2 / (g1 + kk), u = sd * (sd + ss) / (g1 + kk), e = std::exp(-kk * dtau), m = -std::expm1(-kk * dtau);
      const LDb ge = 1 + Gm * e, den = (u + Gm * m) * ge, D = sun * beam[(size_t)l * c.n_pts + j];
      R = Gm * m * (1 + e) / den, T = e * u * (1 + Gm) / den, oneR = u * (1 + Gm * e * e) / den, ab = m * u * (1 - Gm * e) / den;
      const LDb oneT = m * (u + Gm * ge) / den, es = om * D * (sd + ss) / (g1 + kk) * (m / sd) / ge, ed = -(om * D * r3 * g * mu0) / s * (oneT + R);
      Ep = (es + ed) / 2, Em = (es - ed) / 2, q = 1 / (Cb + Rb * oneR);
    }
    tq[l] = T * q, cq[l] = (Em + R * Ub) * q, rb[l] = Rb, ub[l] = Ub;
    Ub = Ep + T * (Ub + Rb * Em) * q;
    Cb = (oneR * Cb + Rb * ab * (oneR + T)) * q;
    Rb = R + T * T * Rb * q;
  }
  F.assign(2 * (N + 1), 0);
  J.assign(N, 0);
  F[N] = Ub;
  const LDb kJ = r3 / (8 * std::acos((LDb)-1));
  for (int l = N - 1; l >= 0; --l) {
    F[N + 1 + l] = tq[l] * F[N + 1 + l + 1] + cq[l];
    F[l] = ub[l] + rb[l] * F[N + 1 + l];
    J[l] = kJ * ((F[l] + F[N + 1 + l]) + (F[l + 1] + F[N + 1 + l + 1]));
  }
}

static int check_all_outputs(const Case &c, const Out &o, bool acc) {
  const int N = c.n_layers;
  const LDb eps = std::ldexp((LDb)1, -53), fac = eps * (c.n_gas + 16 * N + 16);
  const LDb f0 = c.asym[0] > 0 ? (LDb)c.asym[0] * c.asym[0] : 0, w = c.ssa[0] * (1 - f0);
  int bad = 0;
  std::vector<std::vector<LDb>> F(c.n_col), J(c.n_col);
  for (int j = 0; j < c.n_pts; ++j) {
    for (int k = 0; k < c.n_col; ++k) {
      plain(c, k, j, F[k], J[k]);
      for (int i = 0; i < 2 * (N + 1); ++i) {
        const double v = o.F[((size_t)k * 2 * (N + 1) + i) * c.n_pts + j];
        if ((!(std::fabs((LDb)v - F[k][i]) <= fac * F[k][i]) || v < 0) && bad++ < 10)
          std::printf("column %d flux %d point %d: %.17g, plain %.17Lg\n", k, i, j, v, F[k][i]);
      }
      for (int l = 0; l < N; ++l) {
        const double v = o.J[((size_t)k * N + l) * c.n_pts + j];
        if ((!(std::fabs((LDb)v - J[k][l]) <= fac * J[k][l]) || v < 0) && bad++ < 10)
          std::printf("column %d layer %d point %d: J %.17g plain %.17Lg\n", k, l, j, v, J[k][l]);
      }
    }
    for (int r = 0; r < c.n_rows; ++r) {
      const size_t at = (size_t)r * c.n_pts + j;
      LDb dot = 0;
      bool any = false;
      for (int k = 0; k < c.n_col; ++k) dot += (LDb)c.col_w[(size_t)r * c.n_col + k] * J[k][c.row_layer[r]], any |= c.col_w[(size_t)r * c.n_col + k] != 0.0;
      const LDb e = w * c.sca[(size_t)c.src_row[r] * c.n_pts + j] * dot, base = acc ? pattern(at) : 0;
      bool ok = std::fabs((LDb)o.emi[at] - (base + e)) <= (fac + eps * c.n_col) * e + eps * std::fabs(base + e);
      if (!any || w == 0) { // an exact zero; accumulating, the bits of the base (a -0.0 stays one)
        const double want = acc ? pattern(at) : 0.0;
        ok = std::memcmp(&o.emi[at], &want, sizeof(double)) == 0;
      }
      if (!ok && bad++ < 10) std::printf("row %d point %d: emi %.17g plain %.17Lg\n", r, j, o.emi[at], base + e);
    }
  }
  return bad;
}

template <bool ACC> static int same_bits(const Case &c, const Out &full, bool we, bool wj, bool wf) {
  Out o = fresh(c, ACC);
  run_kernel<ACC>(c, 1 << 30, we, wj, wf, o);
  int bad = 0;
  if (we && !ACC && std::memcmp(o.emi.data(), full.emi.data(), o.emi.size() * sizeof(double))) ++bad;
  if (wj && std::memcmp(o.J.data(), full.J.data(), o.J.size() * sizeof(double))) ++bad;
  if (wf && std::memcmp(o.F.data(), full.F.data(), o.F.size() * sizeof(double))) ++bad;
  for (size_t at = 0; at < o.J.size(); ++at) bad += (!wj && !std::isnan(o.J[at])); // an output that was not asked for stays untouched
  for (size_t at = 0; at < o.F.size(); ++at) bad += (!wf && !std::isnan(o.F[at]));
  if (!we)
    for (size_t at = 0; at < o.emi.size(); ++at) bad += !(ACC ? o.emi[at] == pattern(at) : std::isnan(o.emi[at]));
  if (we && ACC)
    for (size_t at = 0; at < o.emi.size(); ++at) bad += !(o.emi[at] == pattern(at) + full.emi[at]); // overwrite plus base, one rounding
  if (bad) std::printf("instance acc %d, outputs %d %d %d, differs from the full instance\n", (int)ACC, (int)we, (int)wj, (int)wf);
  return bad;
}

// columns [a, b, c] against [c, a]: a's and c's J and fluxes bit for bit (another instance, another order)
static int independent(const Case &c3) {
  Case c2 = c3;
  const int N = c3.n_layers;
  const size_t nb = (size_t)(N + 1) * c3.n_pts, nj = (size_t)N * c3.n_pts, nf = 2 * nb;
  c2.n_col = 2;
  c2.mu0 = {c3.mu0[2], c3.mu0[0]};
  c2.beam.assign(c3.beam.begin() + 2 * nb, c3.beam.begin() + 3 * nb);
  c2.beam.insert(c2.beam.end(), c3.beam.begin(), c3.beam.begin() + nb);
  c2.col_w.assign((size_t)c2.n_rows * 2, 0.5);
  Out a = fresh(c3, false), b = fresh(c2, false);
  run_kernel<false>(c3, 1 << 30, true, true, true, a);
  run_kernel<false>(c2, 1 << 30, true, true, true, b);
  int bad = 0;
  bad += std::memcmp(a.J.data(), b.J.data() + nj, nj * sizeof(double)) != 0;
  bad += std::memcmp(a.J.data() + 2 * nj, b.J.data(), nj * sizeof(double)) != 0;
  bad += std::memcmp(a.F.data(), b.F.data() + nf, nf * sizeof(double)) != 0;
  bad += std::memcmp(a.F.data() + 2 * nf, b.F.data(), nf * sizeof(double)) != 0;
  if (bad) std::printf("a column's bits depend on its neighbours\n");
  return bad;
}

int main() {
  const int layers[] = {1, 2, 3, 17, 80}, gases[] = {1, 3, 8}, pts[] = {1, 63, 65, 257}, cols[] = {1, 2, 3, 5, 8};
  unsigned seed = 20261021;
  int bad = 0, n = 0;
  for (int a = 0; a < 5; ++a)
    for (int b = 0; b < 3; ++b)
      for (int d = 0; d < 4; ++d) {
        const Case c = make_case(layers[a], gases[b], pts[d], cols[n % 5], seed++);
        Out full = fresh(c, false);
        run_kernel<false>(c, 1 << 30, true, true, true, full);
        int bc = check_all_outputs(c, full, false);
        const bool corner = (a == 0 || a == 4) && (b == 0 || b == 2) && (d == 0 || d == 3);
        if (corner || n % 7 == 3) {
          bc += same_bits<false>(c, full, true, false, false) + same_bits<false>(c, full, true, true, false) + same_bits<false>(c, full, true, false, true);
          bc += same_bits<false>(c, full, false, true, true) + same_bits<false>(c, full, false, true, false) + same_bits<false>(c, full, false, false, true);
          bc += same_bits<true>(c, full, true, false, false) + same_bits<true>(c, full, true, true, true);
          Out acc = fresh(c, true);
          run_kernel<true>(c, 1 << 30, true, true, true, acc);
          bc += check_all_outputs(c, acc, true);
        }
        if (pts[d] == 257) { // two point chunks, the second from p_lo = 256 on: the same bits
          Out two = fresh(c, false);
          run_kernel<false>(c, 256, true, true, true, two);
          if (std::memcmp(two.emi.data(), full.emi.data(), two.emi.size() * sizeof(double)) || std::memcmp(two.F.data(), full.F.data(), two.F.size() * sizeof(double)) ||
              std::memcmp(two.J.data(), full.J.data(), two.J.size() * sizeof(double))) {
            std::printf("two point chunks differ from one\n");
            ++bc;
          }
        }
        if (c.n_col == 3) bc += independent(c);
        if (bc) std::printf("n_layers %d n_gas %d n_pts %d n_col %d: FAILED\n", layers[a], gases[b], pts[d], c.n_col);
        bad += bc;
        ++n;
      }
  std::printf(bad ? "FAILED\n" : "all %d cases ok\n", n);
  return bad ? 1 : 0;
}
