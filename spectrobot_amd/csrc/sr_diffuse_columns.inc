// sr_diffuse_columns.inc -- sr_diffuse_columns_kernel.  Included by sr_solar_source.hip inside namespace sr, behind
// sr_diffuse_source.inc (whose diffuse_sums, diffuse_operators and diffuse_boundary it uses), and by the host build
// tools/diffuse_columns_host.  Nothing else includes it.

// The two-stream diffuse source of sr_diffuse_source.inc for NC columns of illumination -- (mu0_c, beam_c), c < NC -- over
// one atmosphere, in one walk of the layers, and the emission rows of LOS steps from its downward sweep (DESIGN.md 4.11e).
// Of a layer's operators R, T, 1 - R, 1 - R - T, the elimination q and the stack's Rb, Cb do not depend on the
// illumination; the two sources are linear in D_c = sun beam_c[l] with one factor each,
//   fs = omega (sd + ss) / (gamma1 + k) (m / sd) / (1 + Gamma e),   fd = -omega sqrt3 g / s ((1 - T) + R)
//   E+_c + E-_c = D_c fs,   E+_c - E-_c = (D_c mu0_c) fd
// so a column costs a handful of multiply-adds and two workspace doubles per layer:
//   Ub_c' = E+_c + T (Ub_c + Rb E-_c) q,   F-_c,l = T q F-_c,l+1 + (E-_c + R Ub_c) q,   F+_c,l = Ub_c + Rb F-_c,l
// and J_c,l as in sr_diffuse_source.inc.  No column's arithmetic reads another's: a column's bits do not depend on which
// columns share the call, nor on the instance.  Then, for the rows r the host lists under layer l,
//   emi[r][j] (+)= w_out sca_abs[src_row[r]][j] sum_c col_w[r][c] J_c,l        c ascending, from the first term
// a dense dot product (no register array is indexed by a runtime column).  A listed row with kZeroRow set stores an exact
// 0 (every weight is 0, or w_out is); under accumulate the host does not list such a row at all, so that it keeps its bits.
//
// One thread per grid point, 256 points per block, blocks dealt by limb_block(), as the sibling.  The workspace is
// ws [2 + 2 NC][N][ws_stride]: T q, Rb, then per column (E-_c + R Ub_c) q and Ub_c.  A layer's rows of A, the beams and the
// workspace are requested one layer ahead of the arithmetic that uses them, a row's sca_abs (and, accumulating, its old
// value) one row ahead.  mu0 [NC], col_w [n_rows][NC], src_row, row_off [N + 1] and row_ix are staged by the host and
// block-uniform (scalar loads): row_ix lists the rows in the order of the walk, top layer first, layer l's at
// row_off[N - 1 - l] .. row_off[N - l].  A column c >= n_col is padding: its beam is 0 without a load, mu0 and weights are
// the host's zeros, nothing of it is stored but its workspace.  A point beyond the call's last reads the last point and
// stores nothing.  One writer per element, no atomics: the same call gives the same bits.
// (kZeroRow, kDiffuseColumns and the host's plan diffuse_columns_plan: sr_solar_plan.hpp)
struct DiffuseShared { double R, T, oneR, absb, fs, fd; bool live; };

// the columns' source former: the operators every column shares (diffuse_operators) and the two factors, D left out
__device__ __forceinline__ DiffuseShared diffuse_layer_shared(double sp, double al, double sg) {
  const double kSqrt3 = 1.7320508075688772;
  if (!(sp + al > 0.0)) return DiffuseShared{0.0, 1.0, 1.0, 0.0, 0.0, 0.0, false};
  const DiffuseOps p = diffuse_operators(sp, al, sg);
  const double fs = p.om * (p.sd + p.ss) * p.rg * (p.m / p.sd) / p.ge;
  const double fd = -(p.om * (kSqrt3 * p.g)) / p.s * (p.oneT + p.R);
  return DiffuseShared{p.R, p.T, p.oneR, p.absb, fs, fd, true};
}

template <int NC, bool ACC>
__global__ __launch_bounds__(256) void sr_diffuse_columns_kernel(
    const double *__restrict__ tab_abs, int n_gas, int n_layers, int n_pts, int p_lo, int p_hi, const double *__restrict__ v,
    const double *__restrict__ coef, const double *__restrict__ beam, int n_col, const double *__restrict__ sun,
    const double *__restrict__ mu0, double albedo, double w_out, const int *__restrict__ row_off, const int *__restrict__ row_ix,
    const int *__restrict__ src_row, const double *__restrict__ col_w, const double *__restrict__ sca_abs, double *__restrict__ ws,
    int ws_stride, double *emi_out, double *__restrict__ j_out, double *__restrict__ flux_out) {
  int pb, item;
  if (!limb_block((p_hi - p_lo + 255) / 256, 1, pb, item)) return; // (block-uniform)
  const int col = pb * 256 + threadIdx.x, j = p_lo + col;
  const bool live = j < p_hi;
  const size_t np = (size_t)n_pts, jj = (size_t)min(j, p_hi - 1);
  const size_t wrow = (size_t)ws_stride, wq = (size_t)n_layers * wrow; // ws [2 + 2 NC][n_layers][ws_stride]
  const size_t brow = (size_t)(n_layers + 1) * np;                      // beam [n_col][n_layers + 1][n_pts]
  const double sj = sun[jj];

  // ---- bottom up ----
  double a_nx[kDiffuseGases], b_nx[NC];
  auto fetch = [&](int l) {
#pragma unroll
    for (int g = 0; g < kDiffuseGases; ++g) a_nx[g] = tab_abs[((size_t)(g < n_gas ? g : 0) * n_layers + l) * np + jj];
#pragma unroll
    for (int c = 0; c < NC; ++c) b_nx[c] = c < n_col ? beam[c * brow + (size_t)l * np + jj] : 0.0;
  };
  fetch(0);
  double Rb = 0.0, Cb = 0.0, Ub[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c)
    diffuse_boundary(albedo, mu0[c], sj, c < n_col ? beam[c * brow + (size_t)n_layers * np + jj] : 0.0, Rb, Cb, Ub[c]);
  for (int l = 0; l < n_layers; ++l) {
    double a[kDiffuseGases], bm[NC];
#pragma unroll
    for (int g = 0; g < kDiffuseGases; ++g) a[g] = a_nx[g];
#pragma unroll
    for (int c = 0; c < NC; ++c) bm[c] = b_nx[c];
    if (l + 1 < n_layers) fetch(l + 1); // the next layer's rows in flight under this layer's arithmetic
    const DiffuseSums s = diffuse_sums(v, coef, n_gas, n_layers, l, a);
    const DiffuseShared o = diffuse_layer_shared(s.sp, s.al, s.sg);
    const double q = o.live ? 1.0 / (Cb + Rb * o.oneR) : 1.0; // (an empty layer: every quantity keeps its bits)
    const size_t at = (size_t)l * wrow + col;
    ws[at] = o.T * q;
    ws[wq + at] = Rb;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const double D = sj * bm[c];
      const double es = D * o.fs, ed = (D * mu0[c]) * o.fd;
      const double Ep = 0.5 * (es + ed), Em = 0.5 * (es - ed);
      ws[(2 + 2 * c) * wq + at] = (Em + o.R * Ub[c]) * q;
      ws[(3 + 2 * c) * wq + at] = Ub[c];
      Ub[c] = Ep + o.T * (Ub[c] + Rb * Em) * q;
    }
    Cb = (o.oneR * Cb + Rb * o.absb * (o.oneR + o.T)) * q;
    Rb = o.R + o.T * o.T * Rb * q;
  }

  // ---- top down ----
  const double kJ = 1.7320508075688772 / (8.0 * 3.141592653589793);
  const size_t frow = (size_t)(n_layers + 1) * np, jrow = (size_t)n_layers * np; // flux_out [n_col][2][N + 1][n_pts], j_out [n_col][N][n_pts]
  const bool wj = j_out != nullptr, wf = flux_out != nullptr;                    // (block-uniform)
  double fp[NC], fm[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    fp[c] = Ub[c], fm[c] = 0.0;
    if (wf && live && c < n_col) {
      flux_out[2 * c * frow + (size_t)n_layers * np + j] = fp[c];
      flux_out[(2 * c + 1) * frow + (size_t)n_layers * np + j] = fm[c];
    }
  }
  const int n_listed = emi_out != nullptr ? row_off[n_layers] : 0; // (block-uniform)
  double w_nx[2 + 2 * NC], s_nx = 0.0, e_nx = 0.0;
  auto fetch_down = [&](int l) {
    const size_t at = (size_t)l * wrow + col;
#pragma unroll
    for (int c = 0; c < 2 + 2 * NC; ++c) w_nx[c] = ws[c * wq + at];
  };
  auto fetch_row = [&](int k) { // the row listed at k: its scatterer's row and, accumulating, the value it adds to
    const int r = row_ix[k] & (kZeroRow - 1);
    s_nx = sca_abs[(size_t)src_row[r] * np + jj];
    if (ACC && live) e_nx = emi_out[(size_t)r * np + j];
  };
  fetch_down(n_layers - 1);
  if (n_listed > 0) fetch_row(0);
  for (int l = n_layers - 1; l >= 0; --l) {
    double w[2 + 2 * NC];
#pragma unroll
    for (int c = 0; c < 2 + 2 * NC; ++c) w[c] = w_nx[c];
    if (l > 0) fetch_down(l - 1);
    const double tq = w[0], rb = w[1];
    double J[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const double fm_l = tq * fm[c] + w[2 + 2 * c], fp_l = w[3 + 2 * c] + rb * fm_l;
      J[c] = kJ * ((fp_l + fm_l) + (fp[c] + fm[c]));
      fp[c] = fp_l, fm[c] = fm_l;
      if (live && c < n_col) {
        const size_t at = (size_t)l * np + j;
        if (wf) {
          flux_out[2 * c * frow + at] = fp_l;
          flux_out[(2 * c + 1) * frow + at] = fm_l;
        }
        if (wj) j_out[c * jrow + at] = J[c];
      }
    }
    const int k_hi = n_listed > 0 ? row_off[n_layers - l] : 0;
    for (int k = row_off[n_layers - 1 - l]; k < k_hi; ++k) {
      const int entry = row_ix[k], r = entry & (kZeroRow - 1);
      const double sca = s_nx, old = e_nx;
      if (k + 1 < n_listed) fetch_row(k + 1);
      const double *__restrict__ cw = col_w + (size_t)r * NC;
      double dot = cw[0] * J[0];
#pragma unroll
      for (int c = 1; c < NC; ++c) dot += cw[c] * J[c];
      const double val = (entry & kZeroRow) ? 0.0 : (w_out * sca) * dot;
      if (live) emi_out[(size_t)r * np + j] = ACC ? old + val : val;
    }
  }
}
