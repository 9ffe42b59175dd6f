// sr_ops.hip -- the small operators beside the coefficient op and the limb family, with their launchers.
//
//   shims                          humliv_bb / sum_all_lines / curgod_fort_N call shapes
//   sr_lut_kernel                  G-coefficient tables interpolated in (P, T), combined with the level population
//   sr_glevel_combine*_kernel      level tables combined with populations
//   sr_lowres_*_kernel             the instrument's band integrals (hires_to_lowres; sr_lowres_weights_tab.inc)
//   sr_absorber_table_kernel       tabulated absorbers on coefficient rows (sr_absorber_table.inc)
#include <climits>
#include <cstdlib>

#include "sr_device.hpp"
#include "sr_kernels.hpp"

namespace sr {

// ------------------------------------------------------------------------
// shims
// ------------------------------------------------------------------------
// lineshape.f:226-569, middle branch, on a caller-supplied x(i1..i2)
__global__ __launch_bounds__(256) void sr_humliv_kernel(const double *__restrict__ x, int i1, int n,
                                                        double x0, double lw, double dwp,
                                                        double *__restrict__ y) {
  ArrX xf{x + (i1 - 1)};
  const Bounds B = humliv_bounds(xf, n, x0, lw, dwp); // cheap; every thread recomputes
  FastRec r;
  r.xl = B.xl; r.xr = B.xr; r.xstep = B.xstep;
  r1_set(r, B.ry);
  r.wabs = r.wemi = 1.0; r.j1 = 0;
  r.ilir = (uint32_t)B.il | ((uint32_t)B.ir << 16);
  const ColdFull c = expand_cold(make_cold(B, dwp, x0, xf));
  for (int k = blockIdx.x * blockDim.x + threadIdx.x + 1; k <= n; k += gridDim.x * blockDim.x)
    y[i1 - 1 + k - 1] = humliv_point(k, r, c, xf);
}

// lineshape.f:272-442: x0 at or beyond an end of x(i1..i2).  These two branches advance rx and the
// region starts by running sums from the near end, so they are inherently sequential; no caller on
// the hot path reaches them, one thread walks the Fortran's loops as written.
__global__ void sr_humliv_outer_kernel(const double *__restrict__ x, int i1, int i2, double x0, double lw,
                                       double dw, double *__restrict__ y) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
#define SR_X(k) x[(k)-1]
#define SR_Y(k) y[(k)-1]
  const double ry = lw / dw, xstep = (SR_X(i1 + 1) - SR_X(i1)) / dw, ryf = (double)(float)ry;
  double q2[8], a1, b1, c1, d1;
  region2_coef(ry, q2);
  region1_coef(ry, a1, b1, c1, d1);
  auto r1 = [&](double xr) { const double x2 = xr * xr; return (a1 + x2 * b1) / (c1 + x2 * (d1 + 4. * x2)); };
  auto r2 = [&](double xr) {
    const double x2 = xr * xr;
    return (q2[0] + x2 * (q2[1] + x2 * (q2[2] + q2[3] * x2))) / (q2[4] + x2 * (q2[5] + x2 * (q2[6] + x2 * (q2[7] + x2))));
  };
  if (x0 <= SR_X(i1)) { // :272-357
    int j = i1;
    double rx = (SR_X(j) - x0) / dw;
    while ((rx + ry < 5.5) && (j <= i2)) {
      SR_Y(j) = core_point(rx, ry, ryf);
      j = j + 1;
      rx = rx + xstep;
    }
    if (j <= i2) {
      int l = max((int)round((15.0 - ry - rx) / xstep), 0) + j;
      l = min(l, i2);
      if (l > j) {
        double xrun = (SR_X(j) - x0) / dw;
        for (int k = j; k <= l; ++k) { SR_Y(k) = r2(xrun); xrun = xrun + xstep; }
        l = l + 1;
      }
      if (l < j) l = j;
      if (l < i2) {
        double xrun = (SR_X(l) - x0) / dw;
        for (int k = l; k <= i2; ++k) { SR_Y(k) = r1(xrun); xrun = xrun + xstep; }
      }
    }
  } else { // x0 >= x(i2), :358-442
    int j = i2;
    double rx = (x0 - SR_X(j)) / dw;
    while ((rx + ry < 5.5) && (j >= i1)) {
      SR_Y(j) = core_point(rx, ry, ryf);
      j = j - 1;
      rx = rx + xstep;
    }
    if (j >= i1) {
      int l = j - max((int)round((15.0 - ry - rx) / dw / xstep), 0); // sic, :404
      l = max(l, i1);
      if (l == i2) l = i2 + 1;
      if (l < j) {
        double xrun = (x0 - SR_X(l)) / dw;
        for (int k = l; k <= j; ++k) { SR_Y(k) = r2(xrun); xrun = xrun - xstep; }
      }
      if (l >= i1) {
        double xrun = (x0 - SR_X(i1)) / dw;
        for (int k = i1; k <= l - 1; ++k) { SR_Y(k) = r1(xrun); xrun = xrun - xstep; }
      }
    }
  }
#undef SR_X
#undef SR_Y
}

int launch_humliv(const double *x, int i1, int i2, double x0, double lw, double dwp, double *y, int outer,
                  hipStream_t st) {
  const int n = i2 - i1 + 1;
  if (outer)
    hipLaunchKernelGGL(sr_humliv_outer_kernel, dim3(1), dim3(64), 0, st, x, i1, i2, x0, lw, dwp, y);
  else
    hipLaunchKernelGGL(sr_humliv_kernel, dim3((n + 255) / 256), dim3(256), 0, st, x, i1, n, x0, lw, dwp, y);
  return (int)hipGetLastError();
}

// lineshape.f:15-23 as a gather: thread j adds the rows in line order, so the
// floating-point sum order is the Fortran's.
__global__ __launch_bounds__(256) void sr_sum_lines_kernel(double *__restrict__ spe, long n_spe,
                                                           const double *__restrict__ rows,
                                                           const int *__restrict__ init,
                                                           const int *__restrict__ fin, int n_lines,
                                                           int row_len) {
  __shared__ int s_init[256], s_fin[256];
  const long j = (long)blockIdx.x * blockDim.x + threadIdx.x + 1; // 1-based
  double acc = j <= n_spe ? spe[j - 1] : 0.0;
  for (int c = 0; c < n_lines; c += 256) {
    __syncthreads();
    if (c + (int)threadIdx.x < n_lines) {
      s_init[threadIdx.x] = init[c + threadIdx.x];
      s_fin[threadIdx.x] = fin[c + threadIdx.x];
    }
    __syncthreads();
    const int cnt = min(256, n_lines - c);
    for (int l = 0; l < cnt; ++l) {
      const int a = s_init[l], b = s_fin[l];
      if (j >= a && j <= b) acc = acc + rows[(size_t)(c + l) * row_len + (j - a)];
    }
  }
  if (j <= n_spe) spe[j - 1] = acc;
}

int launch_sum_lines(double *spe, long n_spe, const double *rows, const int *init, const int *fin,
                     int n_lines, int row_len, hipStream_t st) {
  if (n_spe <= 0) return 0;
  hipLaunchKernelGGL(sr_sum_lines_kernel, dim3((unsigned)((n_spe + 255) / 256)), dim3(256), 0, st, spe,
                     n_spe, rows, init, fin, n_lines, row_len);
  return (int)hipGetLastError();
}

// ------------------------------------------------------------------------
// A9: look-up-table route.  LutSet.calculate (spect_main_module.py:997-1066) interpolates the three G
// spectra of one level between tabulated (P, T) couples -- linear in P between the two nearest pressures
// at each of the two nearest temperatures, then linear in T (SpectralGcoeff.interpolate,
// spect_classes.py:1349-1375); below the lowest tabulated pressure in T only -- and
// make_abscoeff_isomolec / make_abscoeff_LUTS_fast combine them with the level population
// (spect_main_module.py:2073-2080, 2241-2249).  Thread = (grid point, LOS step); tab: [3][n_pt][n_pts].
// idx[s][4]: table rows (P1,T1), (P1,T2), (P2,T1), (P2,T2), or (P1,TA), (P1,TB), -1, -1 for the T-only case.
// COMBINE: abs += pop (Gabs - Gind), emi += pop Gsp; else the interpolated set itself, g_out[3][n_steps][n_pts].
// ------------------------------------------------------------------------
template <bool COMBINE>
__global__ __launch_bounds__(256) void sr_lut_kernel(const double *__restrict__ tab, int n_pt, int n_pts,
                                                     const int *__restrict__ idx, const double *__restrict__ wgt,
                                                     const double *__restrict__ pop, double *__restrict__ out_a,
                                                     double *__restrict__ out_e) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x, s = blockIdx.y, n_steps = gridDim.y;
  if (j >= n_pts) return;
  const int i1 = idx[4 * s + 0], i2 = idx[4 * s + 1], i3 = idx[4 * s + 2], i4 = idx[4 * s + 3];
  const double wp1 = wgt[4 * s + 0], wp2 = wgt[4 * s + 1], wt1 = wgt[4 * s + 2], wt2 = wgt[4 * s + 3];
  double v[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double *t = tab + (size_t)c * n_pt * n_pts + j;
    if (i3 >= 0) {
      const double c13 = wp1 * t[(size_t)i1 * n_pts] + wp2 * t[(size_t)i3 * n_pts];
      const double c24 = wp1 * t[(size_t)i2 * n_pts] + wp2 * t[(size_t)i4 * n_pts];
      v[c] = wt1 * c13 + wt2 * c24;
    } else {
      v[c] = wt1 * t[(size_t)i1 * n_pts] + wt2 * t[(size_t)i2 * n_pts];
    }
  }
  const size_t o = (size_t)s * n_pts + j;
  if (COMBINE) {
    const double p = pop[s];
    double a = out_a[o];
    a = a + v[2] * p; // spect_main_module.py:2078-2080, in this order
    a = a - v[1] * p;
    out_a[o] = a;
    out_e[o] = out_e[o] + v[0] * p;
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) out_a[(size_t)c * n_steps * n_pts + o] = v[c];
  }
}

int launch_lut(int combine, const double *tab, int n_pt, int n_pts, int n_steps, const int *idx, const double *wgt,
               const double *pop, double *out_a, double *out_e, hipStream_t st) {
  if (n_pts <= 0 || n_steps <= 0) return 0;
  const dim3 grid((n_pts + 255) / 256, n_steps);
  if (combine)
    hipLaunchKernelGGL(sr_lut_kernel<true>, grid, dim3(256), 0, st, tab, n_pt, n_pts, idx, wgt, pop, out_a, out_e);
  else
    hipLaunchKernelGGL(sr_lut_kernel<false>, grid, dim3(256), 0, st, tab, n_pt, n_pts, idx, wgt, pop, out_a, out_e);
  return (int)hipGetLastError();
}

// ------------------------------------------------------------------------
// Level-factored combine (spect_main_module.py:2036-2106 / 2200-2276 for all steps of a row at once): a block takes
// 256 points of ONE (P, T) row, holds the row's 2 NL pair spectra (and their T-differences) in registers and walks the
// row's steps; the populations of a step are wave-uniform (scalar loads).  HBM: the tables once + the outputs.
// ------------------------------------------------------------------------
template <int NL, bool DT>
__global__ __launch_bounds__(256) void sr_glevel_combine_kernel(
    const double *__restrict__ tab, const double *__restrict__ tab_dT, int n_levels, int n_rows, int n_pts,
    const int *__restrict__ rows_used, const int *__restrict__ row_off, const int *__restrict__ step_of,
    const double *__restrict__ pop, const double *__restrict__ dpop, double inv_dT, double *__restrict__ abs_out,
    double *__restrict__ emi_out, double *__restrict__ dabs_out, double *__restrict__ demi_out) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x, u = blockIdx.y;
  if (j >= n_pts) return;
  const int row = rows_used[u];
  const size_t plane = (size_t)n_rows * n_pts; // one (level, A | E) plane of the tables
  double A[NL], E[NL], DA[DT ? NL : 1], DE[DT ? NL : 1];
#pragma unroll
  for (int l = 0; l < NL; ++l) {
    const bool on = l < n_levels;
    const size_t o = (size_t)(2 * (on ? l : 0)) * plane + (size_t)row * n_pts + j;
    A[l] = on ? tab[o] : 0.0;
    E[l] = on ? tab[o + plane] : 0.0;
    if (DT) {
      DA[l] = on ? (tab_dT[o] - A[l]) * inv_dT : 0.0;
      DE[l] = on ? (tab_dT[o + plane] - E[l]) * inv_dT : 0.0;
    }
  }
  for (int q = row_off[u]; q < row_off[u + 1]; ++q) {
    const int s = step_of[q];
    const double *p = pop + (size_t)s * n_levels, *dp = DT ? dpop + (size_t)s * n_levels : nullptr;
    double a = 0., e = 0., da = 0., de = 0.;
#pragma unroll
    for (int l = 0; l < NL; ++l) {
      if (l < n_levels) { // wave-uniform
        const double pl = p[l];
        a = fma(pl, A[l], a);
        e = fma(pl, E[l], e);
        if (DT) {
          const double dl = dp[l];
          da = fma(pl, DA[l], fma(dl, A[l], da));
          de = fma(pl, DE[l], fma(dl, E[l], de));
        }
      }
    }
    const size_t o = (size_t)s * n_pts + j;
    abs_out[o] = a;
    emi_out[o] = e;
    if (DT) {
      dabs_out[o] = da;
      demi_out[o] = de;
    }
  }
}

// More than 16 levels (SR_MAX_LEVELS is 64): the pair spectra do not fit the registers; every step re-reads them
// (from L2: the steps of a row follow each other).
template <bool DT>
__global__ __launch_bounds__(256) void sr_glevel_combine_stream_kernel(
    const double *__restrict__ tab, const double *__restrict__ tab_dT, int n_levels, int n_rows, int n_pts,
    const int *__restrict__ rows_used, const int *__restrict__ row_off, const int *__restrict__ step_of,
    const double *__restrict__ pop, const double *__restrict__ dpop, double inv_dT, double *__restrict__ abs_out,
    double *__restrict__ emi_out, double *__restrict__ dabs_out, double *__restrict__ demi_out) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x, u = blockIdx.y;
  if (j >= n_pts) return;
  const int row = rows_used[u];
  const size_t plane = (size_t)n_rows * n_pts;
  for (int q = row_off[u]; q < row_off[u + 1]; ++q) {
    const int s = step_of[q];
    double a = 0., e = 0., da = 0., de = 0.;
    for (int l = 0; l < n_levels; ++l) {
      const size_t o = (size_t)(2 * l) * plane + (size_t)row * n_pts + j;
      const double pl = pop[(size_t)s * n_levels + l], Al = tab[o], El = tab[o + plane];
      a = fma(pl, Al, a);
      e = fma(pl, El, e);
      if (DT) {
        const double dl = dpop[(size_t)s * n_levels + l];
        da = fma(pl, (tab_dT[o] - Al) * inv_dT, fma(dl, Al, da));
        de = fma(pl, (tab_dT[o + plane] - El) * inv_dT, fma(dl, El, de));
      }
    }
    const size_t o = (size_t)s * n_pts + j;
    abs_out[o] = a;
    emi_out[o] = e;
    if (DT) {
      dabs_out[o] = da;
      demi_out[o] = de;
    }
  }
}

int launch_glevel_combine(const double *tab, const double *tab_dT, int n_levels, int n_rows, int n_pts, int n_used,
                          const int *rows_used, const int *row_off, const int *step_of, const double *pop,
                          const double *dpop, double inv_dT, double *abs_out, double *emi_out, double *dabs_out,
                          double *demi_out, hipStream_t st) {
  if (n_pts <= 0 || n_used <= 0) return 0;
  const dim3 grid((n_pts + 255) / 256, n_used);
#define SR_GLC(NL, DT)                                                                                               \
  hipLaunchKernelGGL((sr_glevel_combine_kernel<NL, DT>), grid, dim3(256), 0, st, tab, tab_dT, n_levels, n_rows, n_pts, \
                     rows_used, row_off, step_of, pop, dpop, inv_dT, abs_out, emi_out, dabs_out, demi_out)
#define SR_GLC2(NL) do { if (tab_dT) SR_GLC(NL, true); else SR_GLC(NL, false); } while (0)
  if (n_levels <= 1) SR_GLC2(1);
  else if (n_levels <= 4) SR_GLC2(4);
  else if (n_levels <= 8) SR_GLC2(8);
  else if (n_levels <= 12) SR_GLC2(12);
  else if (n_levels <= 16) SR_GLC2(16);
  else if (tab_dT)
    hipLaunchKernelGGL(sr_glevel_combine_stream_kernel<true>, grid, dim3(256), 0, st, tab, tab_dT, n_levels, n_rows, n_pts,
                       rows_used, row_off, step_of, pop, dpop, inv_dT, abs_out, emi_out, dabs_out, demi_out);
  else
    hipLaunchKernelGGL(sr_glevel_combine_stream_kernel<false>, grid, dim3(256), 0, st, tab, tab_dT, n_levels, n_rows, n_pts,
                       rows_used, row_off, step_of, pop, dpop, inv_dT, abs_out, emi_out, dabs_out, demi_out);
#undef SR_GLC2
#undef SR_GLC
  return (int)hipGetLastError();
}

// curgods.f:2-98, one thread per LOS segment
__global__ void sr_curgod_kernel(int which, const double *__restrict__ nd, const double *__restrict__ vmr,
                                 const double *__restrict__ f, const double *__restrict__ x,
                                 const int *__restrict__ off, int n_seg, double *__restrict__ res) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_seg) return;
  double acc = 0.0;
  for (int i = off[s]; i < off[s + 1] - 1; ++i) {
    const double dx = x[i + 1] - x[i];
    if (which == 1) {
      const double fu = nd[i + 1] / nd[i];
      const double D = log(fu) / dx;
      acc = acc + (nd[i + 1] - nd[i]) / D;
    } else if (which == 2) {
      const double A = nd[i] * vmr[i];
      const double B = nd[i] * (vmr[i + 1] - vmr[i]) / dx;
      const double fu = nd[i + 1] / nd[i];
      const double D = log(fu) / dx;
      acc = acc + (A * D * (fu - 1.) + B * fu * (D * dx - 1.) + B) / (D * D);
    } else if (which == 3) {
      const double A = nd[i] * vmr[i] * f[i];
      const double cc = (vmr[i + 1] - vmr[i]) / dx;
      const double bb = (f[i + 1] - f[i]) / dx;
      const double B = nd[i] * (vmr[i] * bb + f[i] * cc);
      const double C = nd[i] * bb * cc;
      const double fu = nd[i + 1] / nd[i];
      const double D = log(fu) / dx;
      acc = acc + (fu * (D * (A * D + B * (D * dx - 1.)) + C * (D * dx * (D * dx - 2.) + 2.)) +
                   D * (B - A * D) - 2 * C) / (D * D * D);
    } else {
      const double A = nd[i] * vmr[i] * f[i];
      const double cc = (vmr[i + 1] - vmr[i]) / dx;
      const double B = nd[i] * f[i] * cc;
      const double fu = nd[i + 1] * f[i + 1] / (nd[i] * f[i]);
      const double D = log(fu) / dx;
      acc = acc + (A * D * (fu - 1.) + B * fu * (D * dx - 1.) + B) / (D * D);
    }
  }
  res[s] = acc;
}

// ------------------------------------------------------------------------
// N2: SpectralIntensity.hires_to_lowres (spect_classes.py:1180-1191): cm-1 -> nm
// (grid and spectrum, spcl:404-407, 779-783), Gaussian ILS over +-n_sigma sigma
// by the trapezoid rule on the irregular nm grid (convolve_to_grid_from_irregular,
// spcl:883-918; gaussian, spcl:1926-1934; conv_single = np.trapz, spcl:1162-1164).
// One block per (band, ray); nm index i <-> cm-1 index n-1-i.
// ------------------------------------------------------------------------
// g_lo: grid index of rad's first point (a spectral shard's PARTIAL band integrals: the trapezoids between the
// shard's own points, grid values exactly those of the whole grid; the partial sums of the shards add up).
//
// Round 5: two kernels.  The trapezoid sum of a band, sum_i (x_(i+1) - x_i) (y_(i+1) + y_i) / 2 with y_i = s_i u_i, is
// sum_i s_i W_i with W_i = u_i c_i, c_i = (x_(i+1) - x_(i-1)) / 2 inside the window and the half interval at its two
// ends -- and W depends on the band and the grid alone, not on the spectrum.  A retrieval iteration degrades 144 spectra
// (18 LOS x (radiance + 7 derivatives)) with the same 14 bands: one block per (band, spectrum) re-evaluated the
// Gaussian, four IEEE divisions and two exp per trapezoid 144 times over (0.19 ms of a 1.26 ms configs[4] iteration).
// sr_lowres_weights_kernel makes W [n_bands][n_pts] (cm-1 index order) and the bands' point ranges once per call,
// sr_lowres_apply_kernel is the banded product: a block per (spectrum, chunk of 4096 points, group of 16 bands), the
// chunks' partial sums added in chunk order by sr_lowres_sum_kernel.
//
// INSTR = true: the two instrument derivatives of a band, the window's membership held fixed (it is piecewise constant in
// f and w; between its jumps, of relative size exp(-n_sigma^2 / 2), these are the exact derivatives of the sum):
//   centre f -> f + delta (nm):  d band / d delta = sum_i s_i W_i t_i / w
//   width  w -> w e^eta:         d band / d eta   = sum_i s_i W_i (t_i^2 - 1)
// (d u / d f = u t / w; d u / d ln w = u (t^2 - 1): the Gaussian's t^2 and the normalisation's -1; c_i does not move.)
// Linear functionals of the spectrum with weights that differ from W by a polynomial in t: the two tables are written
// beside W and Wt in the same pass -- the same window search, the same t -- as tables 1 and 2 of the scratch
// (lowres_layout, instr), each factor applied to the weight itself (moments sum s x W would cancel).  A window of fewer
// than two points is zero in all three.  INSTR = false: the kernel as it was.
template <bool INSTR>
__global__ __launch_bounds__(256) void sr_lowres_weights_kernel(int n_pts, int g_lo, double w0, double gstep,
                                                                const double *__restrict__ cen, const double *__restrict__ wid,
                                                                double n_sigma, int n_bands, double *__restrict__ W, // [n_bands][n_pts]
                                                                int *__restrict__ range,  // [n_bands][2]: j_lo, j_hi (exclusive)
                                                                double *__restrict__ Wt) { // [gridDim.y / 16][n_pts][16]
  const int b = blockIdx.y;
  if (b >= n_bands) { // the zero columns that fill the last tile of Wt
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n_pts) {
      const size_t at = ((size_t)(b >> 4) * n_pts + j) * 16 + (b & 15);
      Wt[at] = 0.0;
      if constexpr (INSTR) {
        const size_t tab_wt = (size_t)(gridDim.y >> 4) * n_pts * 16; // a table of Wt
        Wt[tab_wt + at] = Wt[2 * tab_wt + at] = 0.0;
      }
    }
    return;
  }
  const double f = cen[b], w = wid[b];
  const double lo = f - n_sigma * w, hi = f + n_sigma * w;
  const double fac = 1 / (w * sqrt(2. * kPi));
  auto gcm = [&](int i) { return w0 + (double)(g_lo + n_pts - 1 - i) * gstep; }; // nm index i <-> cm-1 index n-1-i
  auto xnm = [&](int i) { return 1.e7 / gcm(i); };
  // first i with x >= lo, first i with x > hi (x ascending in i): every thread the same two searches (17 steps)
  int i0, i1;
  {
    int a = 0, c = n_pts;
    while (a < c) { int m = (a + c) >> 1; if (xnm(m) < lo) a = m + 1; else c = m; }
    i0 = a;
    a = 0; c = n_pts;
    while (a < c) { int m = (a + c) >> 1; if (xnm(m) <= hi) a = m + 1; else c = m; }
    i1 = a; // selected: i0 .. i1-1; fewer than two points: no trapezoid
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const bool any = i1 - i0 >= 2;
    range[2 * b] = any ? n_pts - i1 : 0;       // cm-1 indices j = n_pts - 1 - i, i in [i0, i1)
    range[2 * b + 1] = any ? n_pts - i0 : 0;
  }
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_pts) return;
  const int i = n_pts - 1 - j;
  double wgt = 0.0;
  [[maybe_unused]] double wgt_f = 0.0, wgt_w = 0.0;
  if (i >= i0 && i < i1 && i1 - i0 >= 2) {
    const double g = gcm(i), x = 1.e7 / g, t = (x - f) / w;
    const double u = ((g * g) * 1.e-7) * (fac * exp(-0.5 * (t * t))); // y = s u (spcl:779-783 the cm-1 -> nm factor, :1926-1934 the Gaussian)
    const double xl = i > i0 ? xnm(i - 1) : x, xr = i + 1 < i1 ? xnm(i + 1) : x;
    wgt = u * ((xr - xl) / 2.0);
    if constexpr (INSTR) {
      wgt_f = wgt * (t / w);
      wgt_w = wgt * (t * t - 1.0);
    }
  }
  const size_t at = (size_t)b * n_pts + j, at_t = ((size_t)(b >> 4) * n_pts + j) * 16 + (b & 15);
  W[at] = wgt;
  Wt[at_t] = wgt;
  if constexpr (INSTR) {
    const size_t tab_w = (size_t)n_bands * n_pts, tab_wt = (size_t)(gridDim.y >> 4) * n_pts * 16; // a table of W, of Wt
    W[tab_w + at] = wgt_f;
    W[2 * tab_w + at] = wgt_w;
    Wt[tab_wt + at_t] = wgt_f;
    Wt[2 * tab_wt + at_t] = wgt_w;
  }
}

#include "sr_lowres_weights_tab.inc"

constexpr int kLowresBands = 16;   // bands per block of the apply kernel
#ifndef SR_LOWRES_CHUNK
#define SR_LOWRES_CHUNK 4096
#endif
constexpr int kLowresChunk = SR_LOWRES_CHUNK; // (2048 / 1024 measured 60 / 80 us against 56 for the 144 spectra of a configs[4] iteration) points per block: 144 spectra x 15 chunks fill the chip (a block per spectrum walked
                                   // its 60 000 points alone: 117 dependent rounds of 15 loads, 0.21 ms)
// N_TAB = 1: the weights alone, part [n_rays][n_chunks][n_bands].  N_TAB = 3 (sr_hires_to_lowres_instr_shard_dev): the three
// tables of an instr scratch applied in ONE read of the spectrum -- per band the value's accumulator takes the same
// operations in the same order (row 0 is the N_TAB = 1 result, bit for bit: one text), the two derivative accumulators
// beside it; part [n_rays][3][n_chunks][n_bands], i.e. row 3 ray + k of sr_lowres_sum_kernel's [rows][n_chunks][n_bands].
template <int N_TAB>
__global__ __launch_bounds__(256) void sr_lowres_apply_kernel(const double *__restrict__ rad, int n_pts,
                                                              const double *__restrict__ W, const int *__restrict__ range,
                                                              int n_bands, int n_chunks,
                                                              double *__restrict__ part) { // [n_rays][N_TAB][n_chunks][n_bands]
  const int ray = blockIdx.x, chunk = blockIdx.y, b0 = blockIdx.z * kLowresBands, nb = min(kLowresBands, n_bands - b0);
  const double *sp = rad + (size_t)ray * n_pts;
  [[maybe_unused]] const size_t tab = (size_t)n_bands * n_pts; // a table of W
  const int c_lo = chunk * kLowresChunk, c_hi = min(c_lo + kLowresChunk, n_pts);
  double acc[N_TAB][kLowresBands];
#pragma unroll
  for (int k = 0; k < N_TAB; ++k)
#pragma unroll
    for (int q = 0; q < kLowresBands; ++q) acc[k][q] = 0.0;
  // W is zero outside a band's window: no per-point range test, only whole bands that miss the chunk are skipped
  // (block-uniform); the loads of a point's bands are independent of each other
  bool use[kLowresBands];
  bool any_use = false;
#pragma unroll
  for (int q = 0; q < kLowresBands; ++q) {
    use[q] = q < nb && range[2 * (b0 + q)] < c_hi && range[2 * (b0 + q) + 1] > c_lo;
    any_use = any_use || use[q];
  }
  auto row = [&](int k) { return (((size_t)ray * N_TAB + k) * n_chunks + chunk) * n_bands + b0; };
  if (!any_use) { // none of this block's bands reaches the chunk (block-uniform): zeros, and the spectrum is not read
    if ((int)threadIdx.x < nb)
#pragma unroll
      for (int k = 0; k < N_TAB; ++k) part[row(k) + threadIdx.x] = 0.0;
    return;
  }
  for (int j = c_lo + (int)threadIdx.x; j < c_hi; j += (int)blockDim.x) {
    const double sv = sp[j];
#pragma unroll
    for (int q = 0; q < kLowresBands; ++q)
      if (use[q]) {
        const double *w = W + (size_t)(b0 + q) * n_pts + j;
#pragma unroll
        for (int k = 0; k < N_TAB; ++k) acc[k][q] = fma(sv, w[k * tab], acc[k][q]);
      }
  }
  __shared__ double red[N_TAB][kLowresBands][4];
#pragma unroll
  for (int k = 0; k < N_TAB; ++k)
#pragma unroll
    for (int q = 0; q < kLowresBands; ++q) {
      double v = acc[k][q];
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
      if ((threadIdx.x & 63) == 0) red[k][q][threadIdx.x >> 6] = v;
    }
  __syncthreads();
  if ((int)threadIdx.x < nb) {
    const int q = threadIdx.x;
#pragma unroll
    for (int k = 0; k < N_TAB; ++k) part[row(k) + q] = (red[k][q][0] + red[k][q][1]) + (red[k][q][2] + red[k][q][3]);
  }
}
__global__ void sr_lowres_sum_kernel(const double *__restrict__ part, int n_rays, int n_chunks, int n_bands, int out_units,
                                     double *__restrict__ out) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_rays * n_bands) return;
  const int ray = t / n_bands, b = t - ray * n_bands;
  double v = 0.0;
  for (int c = 0; c < n_chunks; ++c) v += part[((size_t)ray * n_chunks + c) * n_bands + b]; // in chunk order: deterministic
  v = v * 1.e-3;                    // 'ergscm2' -> 'Wm2', spcl:1215-1218
  if (out_units == 1) v = v * 1.e3; // -> 'ergscm2', spcl:1224-1228
  if (out_units == 2) v = v * 1.e5; // -> 'nWcm2',   spcl:1230-1234
  out[t] = v;
}

// ... of the partial sums sr_limb_fold_sens_lds_kernel<., true> leaves per 64-point slot (a wave's points): a block per
// (spectrum, band tile), thread = (band of the tile, one of 16 interleaved slices of the slots); a band's slots inside its
// window only; slice sums added in slice order: deterministic.
__global__ __launch_bounds__(256) void sr_lowres_sum_blocks_kernel(const double *__restrict__ part, const int *__restrict__ range,
                                                                   int n_blocks, int n_bands, int out_units, double *__restrict__ out) {
  __shared__ double red[16][16];
  const int row = blockIdx.x, tile = blockIdx.y, n_tiles = gridDim.y;
  const int col = threadIdx.x & 15, slice = threadIdx.x >> 4, b = 16 * tile + col;
  double v = 0.0;
  if (b < n_bands) {
    const int r0 = range[2 * b], r1 = range[2 * b + 1];
    if (r1 > r0)
      for (int c = (r0 >> 6) + slice; c <= (r1 - 1) >> 6; c += 16) v += part[(((size_t)row * n_blocks + c) * n_tiles + tile) * 16 + col];
  }
  red[slice][col] = v;
  __syncthreads();
  if (slice != 0 || b >= n_bands) return;
  v = 0.0;
#pragma unroll
  for (int sl = 0; sl < 16; ++sl) v += red[sl][col];
  v = v * 1.e-3;                    // as sr_lowres_sum_kernel
  if (out_units == 1) v = v * 1.e3;
  if (out_units == 2) v = v * 1.e5;
  out[(size_t)row * n_bands + b] = v;
}

static int lowres_chunks(int n_pts) { return (n_pts + kLowresChunk - 1) / kLowresChunk; }
// fused: the partial sums are per wave of the recursion (launch_fold_dense with the scratch).  n_rays: the rows of partial
// sums (spectra; with the instrument derivatives, instr, the caller counts their rows in).  The scratch grows by the two
// derivative tables with instr only.
size_t lowres_scratch_bytes(int n_pts, int n_bands, int n_rays, bool fused, bool instr) {
  const size_t tiles16 = (size_t)((n_bands + 15) / 16) * 16, n_tab = instr ? kLowresTables : 1;
  const size_t n_part = fused ? 4 * (size_t)((n_pts + 255) / 256) * tiles16 : (size_t)lowres_chunks(n_pts) * n_bands;
  return sizeof(double) * n_tab * ((size_t)n_bands + tiles16) * n_pts + sizeof(double) * (size_t)n_rays * n_part +
         sizeof(int) * (2 * (size_t)n_bands + 2);
}

int launch_lowres_weights(int n_pts, int g_lo, double w0, double gstep, const double *cen, const double *wid, int n_bands,
                          double n_sigma, void *scratch, hipStream_t st, bool instr) {
  if (n_bands <= 0) return 0;
  const LowresScratch L = lowres_layout(scratch, n_pts, n_bands, instr);
  const dim3 grid((n_pts + 255) / 256, (n_bands + 15) / 16 * 16);
  if (instr)
    hipLaunchKernelGGL(sr_lowres_weights_kernel<true>, grid, dim3(256), 0, st, n_pts, g_lo, w0, gstep, cen, wid, n_sigma, n_bands, L.W,
                       L.range, L.Wt);
  else
    hipLaunchKernelGGL(sr_lowres_weights_kernel<false>, grid, dim3(256), 0, st, n_pts, g_lo, w0, gstep, cen, wid, n_sigma, n_bands, L.W,
                       L.range, L.Wt);
  return (int)hipGetLastError();
}

int launch_lowres_weights_tab(int n_pts, int g_lo, double w0, double gstep, const double *cen, const double *wid, int n_bands,
                              const double *tab, int n_shapes, int n_tab, double t_lo, double t_hi, void *scratch, hipStream_t st,
                              bool instr) {
  if (n_bands <= 0) return 0;
  if (!tab || n_tab < 2 || (n_shapes != 1 && n_shapes != n_bands)) return (int)hipErrorInvalidValue; // (the kernel's indexing rests on it)
  const LowresScratch L = lowres_layout(scratch, n_pts, n_bands, instr);
  const dim3 grid((n_pts + 255) / 256, (n_bands + 15) / 16 * 16);
  if (instr)
    hipLaunchKernelGGL(sr_lowres_weights_tab_kernel<true>, grid, dim3(256), 0, st, n_pts, g_lo, w0, gstep, cen, wid, tab, n_shapes,
                       n_tab, t_lo, t_hi, n_bands, L.W, L.range, L.Wt);
  else
    hipLaunchKernelGGL(sr_lowres_weights_tab_kernel<false>, grid, dim3(256), 0, st, n_pts, g_lo, w0, gstep, cen, wid, tab, n_shapes,
                       n_tab, t_lo, t_hi, n_bands, L.W, L.range, L.Wt);
  return (int)hipGetLastError();
}

int launch_lowres_sum_blocks(int n_pts, int n_rows, int n_bands, int out_units, double *out, void *scratch, hipStream_t st,
                             bool instr) {
  if (n_bands <= 0 || n_rows <= 0) return 0;
  const LowresScratch L = lowres_layout(scratch, n_pts, n_bands, instr);
  hipLaunchKernelGGL(sr_lowres_sum_blocks_kernel, dim3(n_rows, (n_bands + 15) / 16), dim3(256), 0, st, L.part, L.range,
                     4 * ((n_pts + 255) / 256), n_bands, out_units, out);
  return (int)hipGetLastError();
}

int launch_lowres(const double *rad, int n_pts, int g_lo, int n_rays, double w0, double gstep, const double *cen,
                  const double *wid, int n_bands, double n_sigma, int out_units, double *out, void *scratch, hipStream_t st,
                  bool weights) {
  if (n_bands <= 0 || n_rays <= 0) return 0;
  const int n_chunks = lowres_chunks(n_pts);
  const LowresScratch L = lowres_layout(scratch, n_pts, n_bands);
  if (weights) launch_lowres_weights(n_pts, g_lo, w0, gstep, cen, wid, n_bands, n_sigma, scratch, st);
  hipLaunchKernelGGL(sr_lowres_apply_kernel<1>, dim3(n_rays, n_chunks, (n_bands + kLowresBands - 1) / kLowresBands), dim3(256), 0, st,
                     rad, n_pts, L.W, L.range, n_bands, n_chunks, L.part);
  hipLaunchKernelGGL(sr_lowres_sum_kernel, dim3((n_rays * n_bands + 255) / 256), dim3(256), 0, st, L.part, n_rays, n_chunks, n_bands,
                     out_units, out);
  return (int)hipGetLastError();
}

// ... with the instrument derivatives: the scratch of an instr call with its three tables in place (launch_lowres_weights,
// instr; sized for 3 n_rays rows); out [n_rays][3][n_bands]: the value, d / d centre, d / d ln width
int launch_lowres_instr(const double *rad, int n_pts, int n_rays, int n_bands, int out_units, double *out, void *scratch,
                        hipStream_t st) {
  if (n_bands <= 0 || n_rays <= 0) return 0;
  const int n_chunks = lowres_chunks(n_pts), n_rows = kLowresTables * n_rays;
  const LowresScratch L = lowres_layout(scratch, n_pts, n_bands, true);
  hipLaunchKernelGGL(sr_lowres_apply_kernel<kLowresTables>, dim3(n_rays, n_chunks, (n_bands + kLowresBands - 1) / kLowresBands), dim3(256), 0,
                     st, rad, n_pts, L.W, L.range, n_bands, n_chunks, L.part);
  hipLaunchKernelGGL(sr_lowres_sum_kernel, dim3((n_rows * n_bands + 255) / 256), dim3(256), 0, st, L.part, n_rows, n_chunks, n_bands,
                     out_units, out);
  return (int)hipGetLastError();
}

int launch_curgod(int which, const double *nd, const double *vmr, const double *f, const double *x,
                  const int *off, int n_seg, double *res, hipStream_t st) {
  if (n_seg <= 0) return 0;
  hipLaunchKernelGGL(sr_curgod_kernel, dim3((n_seg + 63) / 64), dim3(64), 0, st, which, nd, vmr, f, x, off,
                     n_seg, res);
  return (int)hipGetLastError();
}

#include "sr_absorber_table.inc"
static_assert(kAbsTabSets == kAbsTabMaxSets, "the host groups the rows by the kernel's set slots");

int launch_absorber_table(int n_used, const double *set_v0, const double *set_dv, const long long *set_off, const int *set_n,
                          const double *values, int row0, int row1, const double *temps, const double *scale, const int *slot2,
                          const double *w2, const double *dw2, double w0, double gstep, int g_lo, int n_pts, bool source,
                          bool accumulate, double *abs_out, double *emi_out, double *dabs_out, double *demi_out, hipStream_t st) {
  if (row1 <= row0 || n_pts <= 0) return 0;
  if (n_used <= 0 || n_used > kAbsTabSets) return (int)hipErrorInvalidValue; // (the kernel's LDS columns rest on it)
  // 16 rows per block: the sets are interpolated again per row chunk (a few loads and a division per set and point
  // against 16 rows of stores), and 80 rows x 1e5 points are 5 x 391 blocks for 256 CUs
  constexpr int kRows = 16;
  const dim3 grid((n_pts + 255) / 256, (row1 - row0 + kRows - 1) / kRows);
  const bool deriv = dabs_out != nullptr;
#define SR_ABT(S, D, A)                                                                                                      \
  hipLaunchKernelGGL((sr_absorber_table_kernel<S, D, A>), grid, dim3(256), 0, st, n_used, set_v0, set_dv, set_off, set_n, values, \
                     row0, row1, kRows, temps, scale, slot2, w2, dw2, w0, gstep, g_lo, n_pts, abs_out, emi_out, dabs_out, demi_out)
#define SR_ABT2(S, D) do { if (accumulate) SR_ABT(S, D, true); else SR_ABT(S, D, false); } while (0)
  if (source) { if (deriv) SR_ABT2(true, true); else SR_ABT2(true, false); }
  else { if (deriv) SR_ABT2(false, true); else SR_ABT2(false, false); }
#undef SR_ABT2
#undef SR_ABT
  return (int)hipGetLastError();
}

} // namespace sr
