// sr_absorber_table.inc -- sr_absorber_table_kernel.  Included by sr_ops.hip inside namespace sr, and by the host
// build tools/absorber_table_host.

// A tabulated absorber (cross-section, CIA or extinction table: sr_abs_table_create) put onto coefficient rows.  The
// build's own definition -- the reference has no counterpart:
//   nu_j = w0 + (double)(g_lo + j) gstep                      (limb_initial's wavenumber, unfused)
//   set k: t = (nu_j - v0_k) / dv_k (a true division: a point exactly on the last knot gives t == n_k - 1 exactly),
//          s_k(j) = a_k[i] + (a_k[i+1] - a_k[i]) (t - i), i = floor(t);  a_k[n_k - 1] at t == n_k - 1;  0 where the ROUNDED
//          t is < 0 or > n_k - 1
//   row r: abs = c_r (w_lo s_lo + w_hi s_hi),  emi = abs B(nu_j, T_r),  dabs = c_r (dw_lo s_lo + dw_hi s_hi),
//          demi = dabs B + abs dB/dT;   B = 2 h c^2 nu^3 / (exp(x) - 1), x = c2 nu / T, dB/dT = B (x / T) (e^x / (e^x - 1))
// (exp - 1 by subtraction, as limb_initial has it: no expm1).  x is formed WITHOUT its two roundings: the exponential's
// condition number is x (up to 50 in the thermal windows), and c2 nu / T rounded twice would spend the whole of the
// emission's error budget (eps (8 + 2 x), tests/absorber_table_reference.py).  x~ = (c2 nu) (1 / T) in double, its exact
// residual against the unrounded c2 nu / T from two fused multiply-adds, dx = (fma(-x~, T, p) + fma(c2, nu, -p)) / T with
// p = c2 nu rounded, and exp(x) = exp(x~) (1 + dx).
//
// A block takes 256 consecutive grid points, a lane one point, blockIdx.y a chunk of rows_per_block rows.  The launch's
// sets (at most kAbsTabSets: the host splits the rows into launches by the sets they use, slot2 numbers them inside the
// launch) are interpolated ONCE per lane into that lane's own column of LDS -- index arithmetic and table loads are per
// point, not per row; no lane reads another's column, so no barrier.  The rows are then walked with block-uniform plan
// words (temps, scale, slot2, w2, dw2: scalar loads) and written as coalesced rows: one exp per (row, point) serves B and
// dB/dT.  No atomics, one writer per element: the same call gives the same bits.  ACC: the outputs are read and added
// to; a point outside both of a row's sets is neither read nor written.
constexpr int kAbsTabSets = 16;

template <bool SOURCE, bool DERIV, bool ACC>
__global__ __launch_bounds__(256) void sr_absorber_table_kernel(
    int n_used, const double *__restrict__ set_v0, const double *__restrict__ set_dv, const long long *__restrict__ set_off,
    const int *__restrict__ set_n, const double *__restrict__ values, int row0, int row1, int rows_per_block,
    const double *__restrict__ temps, const double *__restrict__ scale, const int *__restrict__ slot2,
    const double *__restrict__ w2, const double *__restrict__ dw2, double w0, double gstep, int g_lo, int n_pts,
    double *__restrict__ abs_out, double *__restrict__ emi_out, double *__restrict__ dabs_out, double *__restrict__ demi_out) {
  __shared__ double s_val[kAbsTabSets * 256];
  const int lane = threadIdx.x, j = blockIdx.x * 256 + lane;
  const bool live = j < n_pts;
  const double nu = w0 + (double)(g_lo + j) * gstep;
  unsigned inside = 0; // bit k: the point lies in set k's range
  for (int k = 0; k < n_used; ++k) {
    const int last = set_n[k] - 1;
    const double t = (nu - set_v0[k]) / set_dv[k];
    double s = 0.0;
    if (live && t >= 0.0 && t <= (double)last) {
      const int i = (int)t, i1 = min(i + 1, last); // t == last: i1 == i, the last value itself
      const double *a = values + set_off[k];
      const double a0 = a[i], a1 = a[i1];
      s = a0 + (a1 - a0) * (t - (double)i);
      inside |= 1u << k;
    }
    s_val[k * 256 + lane] = s;
  }
  if (!live) return;
  [[maybe_unused]] const double c2nu = kC2 * nu, c2nu_lo = fma(kC2, nu, -c2nu), pnu = 2 * kHcgs * (kCcgs * kCcgs) * (nu * nu * nu);
  const int r_lo = row0 + blockIdx.y * rows_per_block, r_hi = min(r_lo + rows_per_block, row1);
  for (int r = r_lo; r < r_hi; ++r) {
    const int lo = slot2[2 * r], hi = slot2[2 * r + 1];
    if (ACC && !(((inside >> lo) | (inside >> hi)) & 1u)) continue;
    const double s_lo = s_val[lo * 256 + lane], s_hi = s_val[hi * 256 + lane];
    const double c = scale[r];
    const double a = c * (w2[2 * r] * s_lo + w2[2 * r + 1] * s_hi);
    double e = 0.0, da = 0.0, de = 0.0;
    if (DERIV) da = c * (dw2[2 * r] * s_lo + dw2[2 * r + 1] * s_hi);
    if (SOURCE) {
      const double T = temps[r], rT = 1.0 / T, x = c2nu * rT, dx = (fma(-x, T, c2nu) + c2nu_lo) * rT;
      const double ex0 = exp(x), ex = ex0 + ex0 * dx, rem1 = 1.0 / (ex - 1); // two divisions per (row, point): 1 / T, this one
      const double B = pnu * rem1;
      e = a * B;
      if (DERIV) de = da * B + a * (B * (x * rT) * (ex * rem1));
    }
    const size_t at = (size_t)r * n_pts + j;
    if (ACC) {
      abs_out[at] += a;
      if (SOURCE) emi_out[at] += e;
      if (DERIV) {
        dabs_out[at] += da;
        if (SOURCE) demi_out[at] += de;
      }
    } else {
      abs_out[at] = a;
      emi_out[at] = e;
      if (DERIV) {
        dabs_out[at] = da;
        if (SOURCE || demi_out) demi_out[at] = de; // (without a source the caller may leave demi_out out)
      }
    }
  }
}
