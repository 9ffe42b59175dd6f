// sr_limb.hip -- the limb family: the radiance recursion along rays and its Jacobians, with every launcher.
//
//   sr_radiance_kernel / sr_radiance_jac*_kernel   the recursion on host-built columns
//   sr_los_columns*_kernel, sr_los_vmr_from_params_kernel, sr_jac_rows_sum_kernel   Curtis-Godson columns of a ray batch
//   sr_limb_kernel / sr_limb_split_kernel          path-order radiances (sr_limb_forward.inc), one to four gases
//   sr_limb_jac_kernel / sr_limb_jac_layer_kernel  forward-sensitivity Jacobians
//   sr_limb_parts_kernel                           the radiance budget
//   sr_limb_adjoint*_kernel, sr_limb_fold_*_kernel the one-pass, layer-synchronous and folded formulations, their packs
//   launch_limb_jac_state                          the prelude of the state kernel's launch; its instances are units of
//                                                  their own (sr_limb_state_unit.hpp), and so are the radiance kernels of
//                                                  five to eight gases (sr_limb_many.hip)
#include <climits>
#include <cstdlib>

#include "sr_device.hpp"
#include "sr_kernels.hpp"
#include "sr_limb_dispatch.hpp"

namespace sr {

// ------------------------------------------------------------------------
// radiance recursion (build's own definition, see include/spectrobot_hip.h)
// ------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sr_radiance_kernel(const double *__restrict__ abs_c,
                                                          const double *__restrict__ emi_c,
                                                          int n_pts, int /*n_rays: gridDim.y*/,
                                                          const int *__restrict__ seg_off,
                                                          const int *__restrict__ seg_layer,
                                                          const double *__restrict__ seg_col,
                                                          int init_from_rad, double *__restrict__ rad) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  const int ray = blockIdx.y;
  if (j >= n_pts) return;
  double I = init_from_rad ? rad[(size_t)ray * n_pts + j] : 0.0;
  const int s0 = seg_off[ray], s1 = seg_off[ray + 1];
  // The recursion is sequential in the segments and a 1-ray launch has only ~1.5 waves per SIMD,
  // so the coefficient loads of kB segments are issued together ahead of their use (one memory
  // latency per kB segments instead of one per segment: 147 -> ~40 us for 160 segments x 1e5 points)
  constexpr int kB = 8;
  for (int sb = s0; sb < s1; sb += kB) {
    double a[kB], e[kB], u[kB];
#pragma unroll
    for (int t = 0; t < kB; ++t) {
      const int s = min(sb + t, s1 - 1);
      const size_t o = (size_t)seg_layer[s] * n_pts + j;
      a[t] = abs_c[o];
      e[t] = emi_c[o];
      u[t] = seg_col[s];
    }
#pragma unroll
    for (int t = 0; t < kB; ++t) {
      if (sb + t < s1) {
        const Atten A = attenuation(a[t] * u[t]);
        I = I * A.t + (e[t] * u[t]) * A.f;
      }
    }
  }
  rad[(size_t)ray * n_pts + j] = I;
}

// Radiance and its derivatives with respect to NP retrieval parameters the absorber columns
// depend on linearly (VMR profile parameters, spect_main_module.py:319-375: col_s = sum_p
// dcol[s][p] * x_p).  Forward sensitivity of the same recursion:
//   d/dcol [I e^-tau + emi col (1 - e^-tau)/tau] = e^-tau (emi - abs I)
//   J_p <- J_p e^-tau + e^-tau (emi - abs I_prev) dcol[s][p];   I <- I e^-tau + src
// (thin segments, |tau| <= 1e-12: the source term by the thin rule's f = 1, f' = -1/2, as everywhere else)
// Thread = (point, ray, chunk of NP parameters).
template <int NP>
__global__ __launch_bounds__(256) void sr_radiance_jac_kernel(const double *__restrict__ abs_c,
                                                              const double *__restrict__ emi_c, int n_pts,
                                                              int /*n_rays: gridDim.y*/, const int *__restrict__ seg_off,
                                                              const int *__restrict__ seg_layer,
                                                              const double *__restrict__ seg_col,
                                                              const double *__restrict__ dcol, int n_par,
                                                              double *__restrict__ rad, double *__restrict__ jac) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  const int ray = blockIdx.y, p0 = blockIdx.z * NP;
  if (j >= n_pts) return;
  double I = 0.0, J[NP];
#pragma unroll
  for (int q = 0; q < NP; ++q) J[q] = 0.0;
  const int s0 = seg_off[ray], s1 = seg_off[ray + 1];
  constexpr int kB = 8; // coefficient loads of kB segments ahead of the recursion, as in sr_radiance_kernel
  for (int sb = s0; sb < s1; sb += kB) {
    double av[kB], ev[kB];
#pragma unroll
    for (int t = 0; t < kB; ++t) {
      const size_t o = (size_t)seg_layer[min(sb + t, s1 - 1)] * n_pts + j;
      av[t] = abs_c[o];
      ev[t] = emi_c[o];
    }
#pragma unroll
    for (int k = 0; k < kB; ++k) {
      const int s = sb + k;
      if (s < s1) {
        const double u = seg_col[s], a = av[k], e = ev[k];
        const double tau = a * u;
        const Atten A = attenuation(tau);
        const double t = A.t, src = (e * u) * A.f;
        // f + tau f' = t for the functions themselves; under the thin rule (f = 1, f' = -1/2) it is 1 - tau / 2, and
        // the source term of every other Jacobian kernel (dE f + E f' dtau) carries that
        double g = t * (e - a * I);
        if (A.thin) g = fma(0.5 * tau, e, g);
#pragma unroll
        for (int q = 0; q < NP; ++q) {
          const double d = (p0 + q < n_par) ? dcol[(size_t)s * n_par + p0 + q] : 0.0;
          J[q] = fma(J[q], t, g * d);
        }
        I = I * t + src;
      }
    }
  }
  if (blockIdx.z == 0) rad[(size_t)ray * n_pts + j] = I;
#pragma unroll
  for (int q = 0; q < NP; ++q)
    if (p0 + q < n_par) jac[((size_t)ray * n_par + p0 + q) * n_pts + j] = J[q];
}

// Radiance derivatives with respect to ONE scalar per layer (its temperature, ...) through the
// layer's own coefficients: dabs[k][j], demi[k][j] = d(abs, emi of layer k)/d(parameter of layer k).
// Forward sensitivity of the recursion I <- I t + src, t = e^-tau, src = emi u f(tau), f = (1 - e^-tau)/tau:
//   dt = -u t dabs,  dsrc = u f demi + emi u^2 f'(tau) dabs,  f' = (tau e^-tau - (1 - e^-tau))/tau^2
//   J_k <- J_k t + [seg_layer == k] (I_prev dt + dsrc).
// Thread = (point, ray, chunk of NP layers); build's definition like the recursion itself.
template <int NP>
__global__ __launch_bounds__(256) void sr_radiance_jac_layer_kernel(
    const double *__restrict__ abs_c, const double *__restrict__ emi_c, const double *__restrict__ dabs,
    const double *__restrict__ demi, int n_pts, int n_layers, const int *__restrict__ seg_off,
    const int *__restrict__ seg_layer, const double *__restrict__ seg_col, double *__restrict__ jac) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  const int ray = blockIdx.y, p0 = blockIdx.z * NP;
  if (j >= n_pts) return;
  double I = 0.0, J[NP];
#pragma unroll
  for (int q = 0; q < NP; ++q) J[q] = 0.0;
  const int s0 = seg_off[ray], s1 = seg_off[ray + 1];
  for (int s = s0; s < s1; ++s) {
    const int k = seg_layer[s];
    const size_t o = (size_t)k * n_pts + j;
    const double u = seg_col[s], a = abs_c[o], e = emi_c[o];
    const double tau = a * u;
    const Atten A = attenuation(tau);
    const double t = A.t, f = A.f;
    const double src = (e * u) * f;
    if (k >= p0 && k < p0 + NP) { // this segment's layer is one of this thread's parameters
      const double fp = atten_fprime(A, tau);
      const double da = dabs[o], de = demi[o];
      const double d = I * (-u * t * da) + u * f * de + e * u * u * fp * da;
#pragma unroll
      for (int q = 0; q < NP; ++q) J[q] = fma(J[q], t, (k == p0 + q) ? d : 0.0);
    } else {
#pragma unroll
      for (int q = 0; q < NP; ++q) J[q] *= t;
    }
    I = I * t + src;
  }
#pragma unroll
  for (int q = 0; q < NP; ++q)
    if (p0 + q < n_layers) jac[((size_t)ray * n_layers + p0 + q) * n_pts + j] = J[q];
}

// ------------------------------------------------------------------------
// Device LOS pipeline (the build's own definition standing in for the absent sbm
// LineOfSight.calc_radtran_steps / radtran_fast, call sites spect_main_module.py:2746-2767, 2834-2845).
//   sr_los_columns_kernel   Curtis-Godson columns of every (gas | profile parameter, segment):
//                           curgod_fort_2 (curgods.f:24-45) over the segment's LOS sample points
//   sr_limb_kernel          recursion of a ray batch over n_gas gases with the call-site options
//                           solo_absorption / initial_intensity (Planck) (radtran_3D_ch4.py:297-315)
//   sr_limb_jac_kernel      + derivatives w.r.t. VMR-profile parameters (columns linear in them)
//   sr_limb_jac_layer_kernel  + derivatives w.r.t. one scalar per layer acting through the coefficients
//   sr_limb_jac_state_kernel  + derivatives w.r.t. level populations / vibrational temperatures of a level-factored gas,
//                             alone or with column parameters in the accumulators of the same pass
//   (all three: forward sensitivities, NP parameters per thread; many parameters / layers: sr_limb_adjoint_kernel below)
//   sr_limb_parts_kernel    the radiance split into the parts single gases / single levels emit, and the background
// Per segment s of a ray, layer k = seg_layer[s], columns u_g = col[g][s]:
//   tau = sum_g abs_g[k] u_g,  E = sum_g emi_g[k] u_g,  t = e^-tau,  f = (1 - t)/tau
//   I <- I t + E f          (E f dropped with solo_absorption)
// ------------------------------------------------------------------------
__global__ void sr_los_columns_kernel(const double *__restrict__ nd, const double *__restrict__ x,
                                      const double *__restrict__ prof, // [n_prof][n_pt]: vmr per gas, then weights per parameter
                                      const double *__restrict__ scale, // [n_prof]
                                      const int *__restrict__ pt_off, int n_seg, int n_pt,
                                      double *__restrict__ col) {      // [n_prof][n_seg]
  const int s = blockIdx.x * blockDim.x + threadIdx.x, q = blockIdx.y;
  if (s >= n_seg) return;
  const double *vmr = prof + (size_t)q * n_pt;
  double acc = 0.0;
  for (int i = pt_off[s]; i < pt_off[s + 1] - 1; ++i) { // curgods.f:33-43
    const double dx = x[i + 1] - x[i];
    const double A = nd[i] * vmr[i];
    const double B = nd[i] * (vmr[i + 1] - vmr[i]) / dx;
    const double fu = nd[i + 1] / nd[i];
    const double D = log(fu) / dx;
    acc = acc + (A * D * (fu - 1.) + B * fu * (D * dx - 1.) + B) / (D * D);
  }
  col[(size_t)q * n_seg + s] = scale[q] * acc;
}

// The VMRs of the retrieved gases at a resident batch's sample points from the parameter vector of a retrieval:
// prof[g][i] = sum over the parameters p of gas g of x_p w_p[i], w_p = prof[n_gas + p] the parameter's mask at the
// sample points.  (A profile that is sum_p mask_p x_p on the altitude levels, interpolated linearly to the sample
// points, is the same sum of the interpolated masks: spect_main_module.py LinearProfile_1D.profile.)  Gases without
// parameters keep their row.
// The parameter vector travels as a kernel argument (up to kVmrParArg values: no staging copy in front of a retrieval
// iteration's first kernel); longer ones in blocks of kVmrParArg, each block adding to the row the first one started.
struct ParVec { double x[kVmrParArg]; };
__global__ void sr_los_vmr_from_params_kernel(double *__restrict__ prof, int n_gas, int n_par, int n_pt,
                                              const int *__restrict__ par_gas, ParVec xv, int p0) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x, g = blockIdx.y;
  if (i >= n_pt) return;
  bool any = false;
  for (int p = 0; p < p0; ++p) any = any || par_gas[p] == g; // (an earlier block started the row)
  double v = any ? prof[(size_t)g * n_pt + i] : 0.0;
  for (int p = p0; p < min(n_par, p0 + kVmrParArg); ++p)
    if (par_gas[p] == g) {
      v = v + xv.x[p - p0] * prof[(size_t)(n_gas + p) * n_pt + i];
      any = true;
    }
  if (any) prof[(size_t)g * n_pt + i] = v;
}
int launch_los_vmr_from_params(double *prof, int n_gas, int n_par, int n_pt, const int *par_gas, const double *x_host, hipStream_t st) {
  if (n_pt <= 0 || n_gas <= 0 || n_par <= 0) return 0;
  for (int p0 = 0; p0 < n_par; p0 += kVmrParArg) {
    ParVec xv;
    for (int p = 0; p < kVmrParArg; ++p) xv.x[p] = p0 + p < n_par ? x_host[p0 + p] : 0.0;
    hipLaunchKernelGGL(sr_los_vmr_from_params_kernel, dim3((n_pt + 255) / 256, n_gas), dim3(256), 0, st, prof, n_gas, n_par, n_pt,
                       par_gas, xv, p0);
  }
  return (int)hipGetLastError();
}

int launch_los_columns(const double *nd, const double *x, const double *prof, const double *scale, const int *pt_off,
                       int n_seg, int n_pt, int n_prof, double *col, hipStream_t st) {
  if (n_seg <= 0 || n_prof <= 0) return 0;
  hipLaunchKernelGGL(sr_los_columns_kernel, dim3((n_seg + 63) / 64, n_prof), dim3(64), 0, st, nd, x, prof, scale, pt_off,
                     n_seg, n_pt, col);
  return (int)hipGetLastError();
}

// d col_g[s] / d z_t of limb rays, the crossed shells held fixed (sr_los_columns_dz): the forward-mode derivative of
// sr_los_columns_kernel's term.  Inside a segment ln nd and the VMR are linear in altitude (geometry.limb_los), their
// slopes taken from the segment's first and last sample point (zero where the two altitudes coincide), so with
// dx_dz = d x_i / d z_t [cm / km] and dalt_dz = d alt_i / d z_t of the path:
//   d nd_i = nd_i slope_ln_nd dalt_dz[i],   d vmr_i = slope_vmr dalt_dz[i].
// One thread per (segment, gas); row g of dcol, [n_gas][n_seg].  Zero path derivatives give an exact 0.0.
__global__ void sr_los_columns_dz_kernel(const double *__restrict__ nd, const double *__restrict__ x,
                                         const double *__restrict__ prof, // [.][n_pt]: the gases' VMRs first
                                         const double *__restrict__ scale, const int *__restrict__ pt_off,
                                         const double *__restrict__ alt, const double *__restrict__ dx_dz,
                                         const double *__restrict__ dalt_dz, int n_seg, int n_pt,
                                         double *__restrict__ dcol) {     // [n_gas][n_seg]
  const int s = blockIdx.x * blockDim.x + threadIdx.x, g = blockIdx.y;
  if (s >= n_seg) return;
  const double *vmr = prof + (size_t)g * n_pt;
  const int i0 = pt_off[s], i1 = pt_off[s + 1] - 1;
  const double dal = alt[i1] - alt[i0];
  const double sl_nd = dal != 0.0 ? log(nd[i1] / nd[i0]) / dal : 0.0;
  const double sl_v = dal != 0.0 ? (vmr[i1] - vmr[i0]) / dal : 0.0;
  double acc = 0.0;
  for (int i = i0; i < i1; ++i) {
    const double dx = x[i + 1] - x[i], ddx = dx_dz[i + 1] - dx_dz[i];
    const double n0 = nd[i], n1 = nd[i + 1], v0 = vmr[i], v1 = vmr[i + 1];
    const double dn0 = n0 * sl_nd * dalt_dz[i], dn1 = n1 * sl_nd * dalt_dz[i + 1];
    const double dv0 = sl_v * dalt_dz[i], dv1 = sl_v * dalt_dz[i + 1];
    const double A = n0 * v0, dA = dn0 * v0 + n0 * dv0;
    const double B = n0 * (v1 - v0) / dx;
    const double dB = (dn0 * (v1 - v0) + n0 * (dv1 - dv0)) / dx - B * ddx / dx;
    const double fu = n1 / n0, dfu = (dn1 - fu * dn0) / n0;
    const double L = log(fu), dL = dfu / fu; // L = D dx
    const double D = L / dx, dD = (dL - D * ddx) / dx;
    const double N = A * D * (fu - 1.) + B * fu * (L - 1.) + B;
    const double dN = dA * D * (fu - 1.) + A * dD * (fu - 1.) + A * D * dfu + dB * fu * (L - 1.) + B * dfu * (L - 1.) +
                      B * fu * dL + dB;
    const double T = N / (D * D);
    acc = acc + (dN - 2. * T * D * dD) / (D * D);
  }
  dcol[(size_t)g * n_seg + s] = scale[g] * acc;
}

int launch_los_columns_dz(const double *nd, const double *x, const double *prof, const double *scale, const int *pt_off,
                          const double *alt, const double *dx_dz, const double *dalt_dz, int n_seg, int n_pt, int n_gas,
                          double *dcol, hipStream_t st) {
  if (n_seg <= 0 || n_gas <= 0) return 0;
  hipLaunchKernelGGL(sr_los_columns_dz_kernel, dim3((n_seg + 63) / 64, n_gas), dim3(64), 0, st, nd, x, prof, scale, pt_off,
                     alt, dx_dz, dalt_dz, n_seg, n_pt, dcol);
  return (int)hipGetLastError();
}

// jac[ray][n_state][j] = sum over the n_hid rows behind it, in row order (the pointing row of
// sr_limb_rays_jac_state_path_dev from its per-gas rows); rows of n_row_tot = n_state + n_hid.
__global__ void sr_jac_rows_sum_kernel(double *__restrict__ jac, int n_rays, int n_state, int n_hid, int n_pts) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_pts) return;
  for (int ray = blockIdx.y; ray < n_rays; ray += gridDim.y) {
    double *row = jac + ((size_t)ray * (n_state + n_hid) + n_state) * n_pts + j;
    double v = row[0];
    for (int g = 1; g < n_hid; ++g) v = v + row[(size_t)g * n_pts];
    row[0] = v;
  }
}

int launch_jac_rows_sum(double *jac, int n_rays, int n_state, int n_hid, int n_pts, hipStream_t st) {
  if (n_rays <= 0 || n_pts <= 0 || n_hid <= 1) return 0;
  hipLaunchKernelGGL(sr_jac_rows_sum_kernel, dim3((n_pts + 255) / 256, n_rays < 65535 ? n_rays : 65535), dim3(256), 0, st, jac, n_rays, n_state,
                     n_hid,
                     n_pts);
  return (int)hipGetLastError();
}

#include "sr_limb_forward.inc"

// Derivatives w.r.t. NP parameters per thread; parameter p belongs to gas par_gas[p] and moves its columns
// linearly, d u_g[s] / d x_p = dcol[p][s] (profile parameters of RetParam / LinearProfile, smm:319-375):
//   d tau = a_g D,  d(E f) = e_g D f + E f'(tau) a_g D,  f' = (tau t - (1 - t))/tau^2
//   J_p <- J_p t + (-I t a_g + e_g f + E f' a_g) D      (single gas: t (e - a I) D)
template <int NG, int NP>
__global__ __launch_bounds__(256) void sr_limb_jac_kernel(
    const double *__restrict__ abs_c, const double *__restrict__ emi_c, int n_pts, int n_layers,
    const int *__restrict__ seg_off, const int *__restrict__ seg_layer, const double *__restrict__ col,
    const double *__restrict__ dcol, const int *__restrict__ par_gas, int n_par, LimbOpts o,
    double *__restrict__ rad, double *__restrict__ jac) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x, ray = blockIdx.y, p0 = blockIdx.z * NP;
  if (j >= n_pts) return;
  double I = limb_initial(o, rad, (size_t)ray * n_pts + j, j), J[NP];
  int pg[NP];
#pragma unroll
  for (int q = 0; q < NP; ++q) {
    J[q] = 0.0;
    pg[q] = p0 + q < n_par ? par_gas[p0 + q] : 0;
  }
  const int s0 = seg_off[ray], s1 = seg_off[ray + 1];
  const size_t gstride = (size_t)n_layers * n_pts;
  for (int s = s0; s < s1; ++s) {
    const size_t ofs = (size_t)seg_layer[s] * n_pts + j;
    double a[NG], e[NG];
    double tau = 0.0, E = 0.0;
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      a[g] = abs_c[g * gstride + ofs];
      e[g] = emi_c[g * gstride + ofs];
      const double u = col[(size_t)g * o.n_seg_total + s];
      tau = g == 0 ? a[g] * u : tau + a[g] * u;
      E = g == 0 ? e[g] * u : E + e[g] * u;
    }
    const Atten A = attenuation(tau);
    const double t = A.t, f = A.f;
    const double fp = atten_fprime(A, tau);
    const double src = o.solo_absorption ? 0.0 : E * f;
#pragma unroll
    for (int q = 0; q < NP; ++q) {
      double ag = a[0], eg = e[0];
#pragma unroll
      for (int g = 1; g < NG; ++g) {
        ag = pg[q] == g ? a[g] : ag;
        eg = pg[q] == g ? e[g] : eg;
      }
      const double D = p0 + q < n_par ? dcol[(size_t)(p0 + q) * o.n_seg_total + s] : 0.0;
      const double dsrc = o.solo_absorption ? 0.0 : fma(E * fp, ag, eg * f);
      J[q] = fma(J[q], t, (dsrc - I * t * ag) * D);
    }
    I = I * t + src;
  }
  if (blockIdx.z == 0) rad[(size_t)ray * n_pts + j] = I;
#pragma unroll
  for (int q = 0; q < NP; ++q)
    if (p0 + q < n_par) jac[((size_t)ray * n_par + p0 + q) * n_pts + j] = J[q];
}

// Derivatives w.r.t. ONE scalar per layer acting through the layer's coefficients (temperature, ...):
// dabs / demi: [NG][n_layers][n_pts].  See sr_radiance_jac_layer_kernel for the recursion.
template <int NG, int NP>
__global__ __launch_bounds__(256) void sr_limb_jac_layer_kernel(
    const double *__restrict__ abs_c, const double *__restrict__ emi_c, const double *__restrict__ dabs,
    const double *__restrict__ demi, int n_pts, int n_layers, const int *__restrict__ seg_off,
    const int *__restrict__ seg_layer, const double *__restrict__ col, LimbOpts o, double *__restrict__ jac) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x, ray = blockIdx.y, p0 = blockIdx.z * NP;
  if (j >= n_pts) return;
  double I = limb_initial(o, jac, 0, j), J[NP]; // init_mode 1 is refused by the host for this kernel
#pragma unroll
  for (int q = 0; q < NP; ++q) J[q] = 0.0;
  const int s0 = seg_off[ray], s1 = seg_off[ray + 1];
  const size_t gstride = (size_t)n_layers * n_pts;
  for (int s = s0; s < s1; ++s) {
    const int k = seg_layer[s];
    const size_t ofs = (size_t)k * n_pts + j;
    const bool mine = k >= p0 && k < p0 + NP;
    double tau = 0.0, E = 0.0, dtau = 0.0, dE = 0.0;
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      const double u = col[(size_t)g * o.n_seg_total + s];
      const double av = abs_c[g * gstride + ofs], ev = emi_c[g * gstride + ofs];
      tau = g == 0 ? av * u : tau + av * u;
      E = g == 0 ? ev * u : E + ev * u;
      if (mine) {
        dtau = fma(dabs[g * gstride + ofs], u, dtau);
        dE = fma(demi[g * gstride + ofs], u, dE);
      }
    }
    const Atten A = attenuation(tau);
    const double t = A.t, f = A.f;
    const double src = o.solo_absorption ? 0.0 : E * f;
    if (mine) {
      const double fp = atten_fprime(A, tau);
      const double d = -I * t * dtau + (o.solo_absorption ? 0.0 : dE * f + E * fp * dtau);
#pragma unroll
      for (int q = 0; q < NP; ++q) J[q] = fma(J[q], t, (k == p0 + q) ? d : 0.0);
    } else {
#pragma unroll
      for (int q = 0; q < NP; ++q) J[q] *= t;
    }
    I = I * t + src;
  }
#pragma unroll
  for (int q = 0; q < NP; ++q)
    if (p0 + q < n_layers) jac[((size_t)ray * n_layers + p0 + q) * n_pts + j] = J[q];
}

// The radiance budget of a ray batch (sr_limb_rays_parts_dev): the recursion is linear in the emission, so the share
// e_k[r] of one gas's emission -- a whole gas, or c[k][r] E_L[row[r]] of one level of the level-factored gas (plane 1 of
// the pair tables of sr_glevel_pairs_dev) -- reaches the observer as
//   C_k <- C_k t + e_k[r] u_g(k) f      (C_k starts at 0; t, f of the TOTAL absorption)
//   B   <- B t                          (B starts at the initial intensity: the background part)
// and the gas parts and B add up to I.  One segment of one part (limb_parts_segment) and the kernel around it:
// NP accumulators per thread, blocks of NP parts on blockIdx.z (the host sorts the parts by level, gas parts first, the
// background last: slot_level >= 0 the row of the tables at which a level's E plane begins, (2 L + 1) n_tab_rows -- a
// 32-bit row number, the 64-bit offset is formed per load --, -1 - g the gas part of gas g, kPartNoSource B or an unused
// slot); per (part
// block, coefficient row) one word, bit q: slot q has a source on this row (c != 0), bit 16 + q: its table value has
// to be loaded (clear for a gas part and where the slot before it holds the same level and is active: that value is
// passed on), and NP coefficients c (for a gas part: the gas's index in the low word).  A block works on one ray, so words and levels are wave-uniform -- scalar loads,
// scalar branches, the accumulators indexed statically -- and a segment none of the block's parts touches costs NP
// multiplications.  The NP coefficients of a row are loaded by lanes 0 .. NP - 1 (one vector load, two registers
// instead of 2 NP scalar ones) and read from there when a slot is worked on (lane_value).  The table values and coefficients of segment s + 1 are loaded before segment s
// is worked on (two register sets that swap roles: the loop is unrolled by two).  Rays and point blocks by
// limb_block(): the rays of a point block share one XCD's L2 for the table rows.
template <int NG, int NP>
__device__ __forceinline__ void limb_parts_segment(
    int s, int s1, size_t j, const double *__restrict__ abs_c, const double *__restrict__ emi_c, int n_pts, size_t gstride,
    const int *__restrict__ seg_layer, const double *__restrict__ col, const LimbOpts &o, int gas,
    const double *__restrict__ tab, const int *__restrict__ coef_row, const unsigned *__restrict__ words,
    const double *__restrict__ cc, const int (&lv)[NP], double (&an)[NG], double (&en)[NG], unsigned &m,
    const double (&cur)[NP], double (&nxt)[NP], double ccur, double &cnxt, double &I, double (&J)[NP]) {
  const int r = seg_layer[s];
  double tau = 0.0, E = 0.0, ug = 0.0, Eg[NG];
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    const double u = col[(size_t)g * o.n_seg_total + s];
    tau = g == 0 ? an[g] * u : tau + an[g] * u;
    Eg[g] = en[g] * u;
    E = g == 0 ? Eg[g] : E + Eg[g];
    ug = g == gas ? u : ug;
  }
  // what segment s + 1 needs: its coefficients and the table values its word asks for
  const int rn = seg_layer[min(s + 1, s1 - 1)];
  const unsigned mn = s + 1 < s1 && !o.solo_absorption ? words[rn] : 0u;
  {
    limb_load_coef<NG>(abs_c, emi_c, gstride, (size_t)rn * n_pts + j, an, en);
    if (NG > 1 && mn) cnxt = cc[(size_t)rn * NP];
    if (mn >> 16) {
      if (NG == 1) cnxt = cc[(size_t)rn * NP];
      const double *tr = tab + j;
      const int row = coef_row[rn];
#pragma unroll
      for (int q = 0; q < NP; ++q)
        if (mn >> (16 + q) & 1u) nxt[q] = tr[(size_t)(lv[q] + row) * n_pts];
    }
  }
  const Atten A = attenuation(tau);
  const double t = A.t, f = A.f;
#pragma unroll
  for (int q = 0; q < NP; ++q) J[q] *= t;
  if (m & 0xffffu) {
    double last = 0.0;
#pragma unroll
    for (int q = 0; q < NP; ++q)
      if (m >> q & 1u) {
        double e;
        if (lv[q] < 0) {
          e = Eg[0];
          if constexpr (NG > 1) { // (which gas: read with the row's coefficients, not compared slot by slot with lv --
            // NP (NG - 1) loop-invariant conditions would each be kept in a scalar register pair)
            const int gi = __builtin_amdgcn_readlane(__double2loint(ccur), q);
#pragma unroll
            for (int g = 1; g < NG; ++g) e = gi == g ? Eg[g] : e;
          }
        } else {
          last = m >> (16 + q) & 1u ? cur[q] : last;
          e = lane_value(ccur, q) * last * ug;
        }
        J[q] += e * f;
      }
  }
  I = I * t + (o.solo_absorption ? 0.0 : E * f);
  m = mn;
}

template <int NG, int NP>
__global__ __launch_bounds__(256) void sr_limb_parts_kernel(
    const double *__restrict__ abs_c, const double *__restrict__ emi_c, int n_pts, int n_layers,
    const int *__restrict__ seg_off, const int *__restrict__ seg_layer, const double *__restrict__ col, LimbOpts o,
    int n_rays, int gas, const double *__restrict__ tab, const int *__restrict__ coef_row,
    const unsigned *__restrict__ words, const double *__restrict__ cc, const int *__restrict__ slot_level,
    const int *__restrict__ slot_part, int n_part, double *__restrict__ rad, double *__restrict__ parts) {
  static_assert(NP <= 16, "a row's word has 16 bits per kind");
  int pb, ray;
  if (!limb_block((n_pts + 255) / 256, n_rays, pb, ray)) return;
  const int j0 = pb * 256 + threadIdx.x;
  if (j0 - (int)(threadIdx.x & 63) >= n_pts) return; // the whole wave lies beyond the grid
  // (a wave that straddles the end keeps all its lanes: the coefficients of a row sit in lanes 0 .. NP - 1 and are
  // read from there, lane_value; the lanes beyond the grid work on its last point and store nothing)
  const bool live = j0 < n_pts;
  const int j = min(j0, n_pts - 1);
  const double I0 = limb_initial(o, parts, 0, j); // init_mode 1 is refused by the host for this kernel
  double I = I0, J[NP], ta[NP], tb[NP], ca = 0.0, cb = 0.0;
  int lv[NP];
#pragma unroll
  for (int q = 0; q < NP; ++q) {
    lv[q] = slot_level[blockIdx.z * NP + q];
    J[q] = slot_part[blockIdx.z * NP + q] == n_part ? I0 : 0.0;
    ta[q] = tb[q] = 0.0;
  }
  words += (size_t)blockIdx.z * n_layers;
  cc += (size_t)blockIdx.z * n_layers * NP + (threadIdx.x & (NP - 1)); // lane q holds the coefficient of slot q
  const int s0 = seg_off[ray], s1 = seg_off[ray + 1];
  const size_t gstride = (size_t)n_layers * n_pts;
  double an[NG], en[NG];
  unsigned m = 0u;
  if (s0 < s1) {
    const int r = seg_layer[s0];
    limb_load_coef<NG>(abs_c, emi_c, gstride, (size_t)r * n_pts + j, an, en);
    m = o.solo_absorption ? 0u : words[r];
    if (NG > 1 && m) ca = cc[(size_t)r * NP];
    if (m >> 16) {
      if (NG == 1) ca = cc[(size_t)r * NP];
      const double *tr = tab + j;
      const int row = coef_row[r];
#pragma unroll
      for (int q = 0; q < NP; ++q)
        if (m >> (16 + q) & 1u) ta[q] = tr[(size_t)(lv[q] + row) * n_pts];
    }
  }
#define SR_SEG(S, CUR, NXT, CCUR, CNXT) limb_parts_segment<NG, NP>(S, s1, (size_t)j, abs_c, emi_c, n_pts, gstride, seg_layer, col, o, gas, \
                                                       tab, coef_row, words, cc, lv, an, en, m, CUR, NXT, CCUR, CNXT, I, J)
  for (int s = s0; s < s1; s += 2) {
    SR_SEG(s, ta, tb, ca, cb);
    if (s + 1 < s1) SR_SEG(s + 1, tb, ta, cb, ca);
  }
#undef SR_SEG
  if (!live) return;
  if (blockIdx.z == 0 && rad) rad[(size_t)ray * n_pts + j] = I;
#pragma unroll
  for (int q = 0; q < NP; ++q) {
    const int p = slot_part[blockIdx.z * NP + q];
    if (p >= 0) parts[((size_t)ray * (n_part + 1) + p) * n_pts + j] = J[q];
  }
}

// ------------------------------------------------------------------------
// Radiances and BOTH kinds of Jacobian of a ray batch in ONE pass over each ray (round 3).
//
// I_final = sum_s src_s T(s+1 .. end) + I_0 T(all), so the derivative with respect to anything that acts through
// segment s alone is that segment's own sensitivity times the transmission of everything behind it:
//   w_tau = (-I_prev t + E f') T_after,   w_E = f T_after          (d I_final / d tau_s,  / d E_s)
//   per-layer scalar (temperature):   J_k += w_tau dtau_k u + w_E dE_k u            over the segments in layer k
//   column parameter p of gas g:      J_p += (w_tau a_g + w_E e_g) dcol[p][s]       over the segments p touches
// T_after = exp(-(tau_total - tau(0..s))): a first sweep adds up tau_total (no exp; error-free two-sums, see the
// kernel), the second runs the recursion.
// The forward-sensitivity kernels carry NP accumulators through the whole recursion and repeat it per block of NP
// parameters: 80 per-layer VMR parameters cost five recursions of 160 x (60 + 16 x 4) instructions; here one of
// 160 x ~100.  What remains is the traffic of the Jacobian rows (configs[3]: 2 x 1 GB per set of 8 rays), so the
// host plans the accumulation per ray (SegProg):
//   * a layer's (parameter's) FIRST touch in the ray stores, later ones add: no memset, no read of zeros;
//     rows the ray never touches are zero-filled by the kernel;
//   * a parameter touched by consecutive segments (a level's VMR acts on the shells above and below it) is
//     carried in one of four registers across them and written once per run: a limb path touches a level on its
//     way down and again on its way up -- one store, one read-add-store instead of four accesses.
// Everything in a SegProg is wave-uniform (a block works on one ray): scalar loads and scalar branches.
// ------------------------------------------------------------------------
struct __attribute__((aligned(16))) SegProg {
  int layer;            // row of the coefficient tables
  int flags;            // bit 0: first touch of the per-layer Jacobian row in this ray (store), else add
  int n_ent;
  int jrow;             // row of the per-layer Jacobian (= layer, or the altitude layer of a 3-D path's step)
  int ent_p[kAdjEnt];   // parameter
  int ent_gf[kAdjEnt];  // gas | slot << 8 | flags << 16: bit 0 run starts here (no carry in), bit 1 run ends here
                        // (write), bit 2 first write of the parameter in this ray (store)
  double u[4];          // column of every gas
  double dc[kAdjEnt];   // d col / d x_p of the entries
};
static_assert(sizeof(SegProg) == 112, "SegProg layout");

// The host's plan (layer, flags, entries) + the columns the device computed -> one record per segment.
__global__ void sr_adj_pack_kernel(const int *__restrict__ plan, // [n_seg][4 + 2 kAdjEnt] ints: layer, flags, n_ent, 0, ent_p, ent_gf
                                   const double *__restrict__ col, int n_gas, int n_seg, SegProg *__restrict__ out) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_seg) return;
  const int *pl = plan + (size_t)s * (4 + 2 * kAdjEnt);
  SegProg r;
  r.layer = pl[0]; r.flags = pl[1]; r.n_ent = pl[2]; r.jrow = pl[3];
#pragma unroll
  for (int i = 0; i < kAdjEnt; ++i) {
    r.ent_p[i] = pl[4 + i];
    r.ent_gf[i] = pl[4 + kAdjEnt + i];
    r.dc[i] = i < r.n_ent ? col[(size_t)(n_gas + r.ent_p[i]) * n_seg + s] : 0.0;
  }
#pragma unroll
  for (int g = 0; g < 4; ++g) r.u[g] = g < n_gas ? col[(size_t)g * n_seg + s] : 0.0;
  out[s] = r;
}

template <int NG, bool LAYER, bool PAR>
__global__ __launch_bounds__(256) void sr_limb_adjoint_kernel(
    const double *__restrict__ abs_c, const double *__restrict__ emi_c, const double *__restrict__ dabs,
    const double *__restrict__ demi, int n_pts, int n_layers, int n_jrows, const int *__restrict__ seg_off,
    const SegProg *__restrict__ prog, const int *__restrict__ zero_off, const int *__restrict__ zero_row, int n_par,
    LimbOpts o, double *__restrict__ rad, double *__restrict__ jac_layer, double *__restrict__ jac_par) {
  // (rays on the slow grid axis: this kernel is bound by its Jacobian writes; with the limb_block order of the
  // radiance kernels -- all rays of a point block on one XCD -- it measured 2.21 instead of 2.11 ms on configs[3])
  const int j = blockIdx.x * blockDim.x + threadIdx.x, ray = blockIdx.y;
  if (j >= n_pts) return;
  const int s0 = seg_off[ray], s1 = seg_off[ray + 1];
  const size_t gstride = (size_t)n_layers * n_pts;
  // rows this ray never touches: row < n_jrows: per-layer Jacobian row, else parameter row - n_jrows
  for (int q = zero_off[ray]; q < zero_off[ray + 1]; ++q) {
    const int row = zero_row[q];
    if (row < n_jrows) {
      if (LAYER) jac_layer[((size_t)ray * n_jrows + row) * n_pts + j] = 0.0;
    } else if (PAR) {
      jac_par[((size_t)ray * n_par + (row - n_jrows)) * n_pts + j] = 0.0;
    }
  }
  // Optical depth of the segments not yet passed, as an unevaluated sum rem + rem_lo (two-sum: every addition's
  // rounding error is kept).  The first sweep adds the segments' tau up, the recursion takes the SAME values off again
  // one by one: at a line centre the path's total can be 1e9 while the last segments' own depth is 0.1 -- carried in
  // one double the difference would be good to 1e-7 only, and with it the transmission behind the near-side layers.
  double rem = 0.0, rem_lo = 0.0;
  for (int s = s0; s < s1; ++s) {
    const SegProg &P = prog[s];
    const size_t ofs = (size_t)P.layer * n_pts + j;
    double tau = 0.0;
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      const double ag = abs_c[g * gstride + ofs];
      tau = g == 0 ? ag * P.u[g] : tau + ag * P.u[g];   // as the recursion below forms it
    }
    const double sm = rem + tau, bb = sm - rem;
    rem_lo += (rem - (sm - bb)) + (tau - bb);
    rem = sm;
  }
  double I = limb_initial(o, rad, (size_t)ray * n_pts + j, j);
  double slot[4] = {0., 0., 0., 0.};
  constexpr int kB = NG == 1 ? 4 : 2; // segments whose coefficient loads are issued together
  for (int sb = s0; sb < s1; sb += kB) {
    double a[kB][NG], e[kB][NG], da[kB][NG], de[kB][NG];
#pragma unroll
    for (int t = 0; t < kB; ++t) {
      const int s = min(sb + t, s1 - 1);
      const size_t ofs = (size_t)prog[s].layer * n_pts + j;
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        a[t][g] = abs_c[g * gstride + ofs];
        e[t][g] = emi_c[g * gstride + ofs];
        if (LAYER) {
          da[t][g] = dabs[g * gstride + ofs];
          de[t][g] = demi[g * gstride + ofs];
        }
      }
    }
#pragma unroll
    for (int t = 0; t < kB; ++t) {
      const int s = sb + t;
      if (s >= s1) break;
      const SegProg &P = prog[s];
      double tau = 0.0, E = 0.0, dtau = 0.0, dE = 0.0;
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        const double u = P.u[g];
        tau = g == 0 ? a[t][g] * u : tau + a[t][g] * u;
        E = g == 0 ? e[t][g] * u : E + e[t][g] * u;
        if (LAYER) {
          dtau = fma(da[t][g], u, dtau);
          dE = fma(de[t][g], u, dE);
        }
      }
      const Atten A = attenuation(tau);
      const double fp = atten_fprime(A, tau);
      {
        const double sm = rem - tau, bb = sm - rem;
        rem_lo += (rem - (sm - bb)) + (-tau - bb);
        rem = sm;
      }
      const double Ta = exp_bounded(fmin(fmax(-(rem + rem_lo), -700.0), 700.0)); // transmission of everything behind this segment
      const double w_tau = (o.solo_absorption ? -I * A.t : fma(E, fp, -I * A.t)) * Ta;
      const double w_E = o.solo_absorption ? 0.0 : A.f * Ta;
      if (LAYER) {
        const double d = fma(w_tau, dtau, w_E * dE);
        double *out = jac_layer + ((size_t)ray * n_jrows + P.jrow) * n_pts + j;
        if (P.flags & 1) *out = d; else *out += d;
      }
      if (PAR) {
        for (int i = 0; i < P.n_ent; ++i) {
          const int gf = P.ent_gf[i], g = gf & 0xff, sl = (gf >> 8) & 0xff, fl = gf >> 16;
          double ag = a[t][0], eg = e[t][0];
#pragma unroll
          for (int q = 1; q < NG; ++q) {
            ag = g == q ? a[t][q] : ag;
            eg = g == q ? e[t][q] : eg;
          }
          double v = fma(w_tau, ag, w_E * eg) * P.dc[i];
          if (!(fl & 1)) v += sl == 0 ? slot[0] : (sl == 1 ? slot[1] : (sl == 2 ? slot[2] : slot[3]));
          if (fl & 2) {
            double *out = jac_par + ((size_t)ray * n_par + P.ent_p[i]) * n_pts + j;
            if (fl & 4) *out = v; else *out += v;
          } else {
            if (sl == 0) slot[0] = v; else if (sl == 1) slot[1] = v; else if (sl == 2) slot[2] = v; else slot[3] = v;
          }
        }
      }
      I = I * A.t + (o.solo_absorption ? 0.0 : E * A.f);
    }
  }
  if (rad) rad[(size_t)ray * n_pts + j] = I;
}

// ------------------------------------------------------------------------
// The same recursion, LAYER-SYNCHRONOUS over a batch of NR rays (round 4).  sr_limb_adjoint_kernel gives every ray
// its own threads, and every ray streams the four coefficient tables from HBM again, twice (the optical-depth sweep
// and the recursion): configs[3], 8 rays: 8.4 GB fetched + 3.5 GB written per set for 2.6 GB of algorithmic bytes, the
// kernel bound by that (profiles/r03_config3_pmc_limb_kernels.txt).  In a 1-D atmosphere all rays walk the SAME
// coefficient rows, down to their tangent shells and up again: a thread here owns one grid point for NR rays, the host
// lists the shells in that order (`sched`: per visit the layer and every ray's segment there, -1 = the ray is not in
// this shell on this side), the shell's coefficients are loaded ONCE per visit and every ray that crosses it takes its
// step -- per ray exactly the operations of sr_limb_adjoint_kernel in exactly its order, so the results are bit for
// bit the same.  State per ray: I, the two-sum of the remaining optical depth, four carry slots.
// ------------------------------------------------------------------------
template <int NG, bool LAYER, bool PAR, int NR>
__global__ __launch_bounds__(256) void sr_limb_adjoint_sync_kernel(
    const double *__restrict__ abs_c, const double *__restrict__ emi_c, const double *__restrict__ dabs,
    const double *__restrict__ demi, int n_pts, int n_layers, int n_jrows, const SegProg *__restrict__ prog,
    const int *__restrict__ zero_off, const int *__restrict__ zero_row, int n_par, LimbOpts o,
    const int *__restrict__ sched, // [n_batches][n_visits][1 + NR]: layer, segment of each ray of the batch (or -1)
    int n_visits, int n_rays, double *__restrict__ rad, double *__restrict__ jac_layer, double *__restrict__ jac_par) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x, batch = blockIdx.y;
  if (j >= n_pts) return;
  const int ray0 = batch * NR;
  const int *sc = sched + (size_t)batch * n_visits * (1 + NR);
  const size_t gstride = (size_t)n_layers * n_pts;
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    const int ray = ray0 + r;
    if (ray >= n_rays) continue;
    for (int q = zero_off[ray]; q < zero_off[ray + 1]; ++q) { // rows this ray never touches
      const int row = zero_row[q];
      if (row < n_jrows) {
        if (LAYER) jac_layer[((size_t)ray * n_jrows + row) * n_pts + j] = 0.0;
      } else if (PAR) {
        jac_par[((size_t)ray * n_par + (row - n_jrows)) * n_pts + j] = 0.0;
      }
    }
  }
  double rem[NR], rem_lo[NR], I[NR], slot[NR][4];
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    rem[r] = rem_lo[r] = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) slot[r][q] = 0.0;
  }
  // sweep 1: the optical depth of every ray's path, two-sums (see sr_limb_adjoint_kernel)
  for (int v = 0; v < n_visits; ++v) {
    const int *sv = sc + (size_t)v * (1 + NR);
    const size_t ofs = (size_t)sv[0] * n_pts + j;
    double a[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) a[g] = abs_c[g * gstride + ofs];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const int sg = sv[1 + r];
      if (sg < 0) continue; // wave-uniform
      const SegProg &P = prog[sg];
      double tau = 0.0;
#pragma unroll
      for (int g = 0; g < NG; ++g) tau = g == 0 ? a[g] * P.u[g] : tau + a[g] * P.u[g];
      const double sm = rem[r] + tau, bb = sm - rem[r];
      rem_lo[r] += (rem[r] - (sm - bb)) + (tau - bb);
      rem[r] = sm;
    }
  }
#pragma unroll
  for (int r = 0; r < NR; ++r) I[r] = ray0 + r < n_rays ? limb_initial(o, rad, (size_t)(ray0 + r) * n_pts + j, j) : 0.0;
  // sweep 2: the recursion, shell by shell
  for (int v = 0; v < n_visits; ++v) {
    const int *sv = sc + (size_t)v * (1 + NR);
    const size_t ofs = (size_t)sv[0] * n_pts + j;
    double a[NG], e[NG], da[NG], de[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      a[g] = abs_c[g * gstride + ofs];
      e[g] = emi_c[g * gstride + ofs];
      if (LAYER) {
        da[g] = dabs[g * gstride + ofs];
        de[g] = demi[g * gstride + ofs];
      }
    }
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const int sg = sv[1 + r];
      if (sg < 0) continue;
      const int ray = ray0 + r;
      const SegProg &P = prog[sg];
      double tau = 0.0, E = 0.0, dtau = 0.0, dE = 0.0;
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        const double u = P.u[g];
        tau = g == 0 ? a[g] * u : tau + a[g] * u;
        E = g == 0 ? e[g] * u : E + e[g] * u;
        if (LAYER) {
          dtau = fma(da[g], u, dtau);
          dE = fma(de[g], u, dE);
        }
      }
      const Atten A = attenuation(tau);
      const double fp = atten_fprime(A, tau);
      {
        const double sm = rem[r] - tau, bb = sm - rem[r];
        rem_lo[r] += (rem[r] - (sm - bb)) + (-tau - bb);
        rem[r] = sm;
      }
      const double Ta = exp_bounded(fmin(fmax(-(rem[r] + rem_lo[r]), -700.0), 700.0));
      const double w_tau = (o.solo_absorption ? -I[r] * A.t : fma(E, fp, -I[r] * A.t)) * Ta;
      const double w_E = o.solo_absorption ? 0.0 : A.f * Ta;
      if (LAYER) {
        const double d = fma(w_tau, dtau, w_E * dE);
        double *out = jac_layer + ((size_t)ray * n_jrows + P.jrow) * n_pts + j;
        if (P.flags & 1) *out = d; else *out += d;
      }
      if (PAR) {
        for (int i = 0; i < P.n_ent; ++i) {
          const int gf = P.ent_gf[i], g = gf & 0xff, sl = (gf >> 8) & 0xff, fl = gf >> 16;
          double ag = a[0], eg = e[0];
#pragma unroll
          for (int q = 1; q < NG; ++q) {
            ag = g == q ? a[q] : ag;
            eg = g == q ? e[q] : eg;
          }
          double val = fma(w_tau, ag, w_E * eg) * P.dc[i];
          if (!(fl & 1)) val += sl == 0 ? slot[r][0] : (sl == 1 ? slot[r][1] : (sl == 2 ? slot[r][2] : slot[r][3]));
          if (fl & 2) {
            double *out = jac_par + ((size_t)ray * n_par + P.ent_p[i]) * n_pts + j;
            if (fl & 4) *out = val; else *out += val;
          } else {
            if (sl == 0) slot[r][0] = val; else if (sl == 1) slot[r][1] = val; else if (sl == 2) slot[r][2] = val; else slot[r][3] = val;
          }
        }
      }
      I[r] = I[r] * A.t + (o.solo_absorption ? 0.0 : E * A.f);
    }
  }
  if (rad) {
#pragma unroll
    for (int r = 0; r < NR; ++r)
      if (ray0 + r < n_rays) rad[(size_t)(ray0 + r) * n_pts + j] = I[r];
  }
}

int launch_limb_adjoint_sync(const double *abs_c, const double *emi_c, const double *dabs, const double *demi, int n_pts,
                             int n_layers, int n_jrows, int n_rays, const SegProg *prog, const int *zero_off,
                             const int *zero_row, int n_par, const LimbOpts &o, const int *sched, int n_visits, double *rad,
                             double *jac_layer, double *jac_par, hipStream_t st) {
  bool found = false; // (an instance for o.n_gas exists and was launched)
  if (n_pts <= 0 || n_rays <= 0 || n_visits <= 0) return 0;
  const dim3 grid((n_pts + 255) / 256, (n_rays + kAdjSyncRays - 1) / kAdjSyncRays);
  found = by_ngas(o.n_gas, [&](auto ng) {
    by_jac_kinds(jac_layer, jac_par, [&](auto lay, auto par) {
      hipLaunchKernelGGL((sr_limb_adjoint_sync_kernel<decltype(ng)::value, decltype(lay)::value, decltype(par)::value, kAdjSyncRays>),
                         grid, dim3(256), 0, st, abs_c, emi_c, dabs, demi, n_pts, n_layers, n_jrows, prog, zero_off, zero_row, n_par,
                         o, sched, n_visits, n_rays, rad, jac_layer, jac_par);
    });
  });
  return found ? (int)hipGetLastError() : (int)hipErrorInvalidValue;
}

// ------------------------------------------------------------------------
// The FOLDED one-pass kernel (round 4): a limb ray crosses every shell above its tangent point twice, and both one-pass
// kernels above touch the shell's Jacobian row twice -- a store on the far side, a read-add-store on the near side --
// and stream the coefficient tables along the path, 2 x 80 visits per sweep.  Here a thread walks the SHELLS once per
// sweep, from the outermost inwards, and takes a ray's far-side and near-side segment of a shell TOGETHER:
//   far side, in path order:   I_f <- I_f t + E f  (the recursion itself), the transmission behind the segment from
//                              the two-sum of the remaining optical depth (as sr_limb_adjoint_kernel);
//   near side, from the observer inwards:  Tn = prod t of the near-side segments outside this one (the transmission
//                              behind it, no subtraction), cs = sum of E f Tn over them (what they contribute to the
//                              observed radiance), and what ENTERS the segment, seen at the observer, is the rest:
//                              I_in t Tn = I_obs - cs(including this segment) -- I_obs from sweep 1,
//                              I_obs = I_f(tangent) Tn(all) + cs(all).
// The weights are those of sr_limb_adjoint_kernel, w_tau = (E f' - I_in t) Ta, w_E = f Ta, the two segments' values
// of a row are added in registers and stored ONCE; a column parameter's touches on both sides fall into the same run
// of shells and are carried in one register.  Per set of configs[3]: 80 visits x (2 + 4) table rows per ray batch
// instead of 160 x (1 + 4), 1 access per Jacobian value instead of 1.7.  I_obs and cs are carried as error-free sums
// of two doubles, so that the difference keeps the relative accuracy of what is still to come (see sweep 2).
// Segments of one shell with the same columns (a 1-D limb path is symmetric) share one attenuation().
// ------------------------------------------------------------------------
#ifndef SR_FOLD_WAVES
#define SR_FOLD_WAVES 4 // waves per SIMD the register allocation of the folded kernel aims at
#endif
struct __attribute__((aligned(16))) FoldRec { // one ray in one shell
  int layer;            // row of the coefficient tables (1-D atmospheres: of both segments; 3-D paths: of the far-side one)
  int has;              // bit 0: far-side segment, bit 1: near-side segment, bit 2: both, with the same columns (and rows)
  int n_ent;
  int layer_n;          // row of the near-side segment's coefficients (3-D paths: every LOS step has its own; else = layer)
  int jrow, pad[3];     // row of the per-layer Jacobian (the shell)
  int ent_p[kAdjEnt], ent_gf[kAdjEnt]; // as SegProg
  double u_f[4], u_n[4];               // columns of the two segments
  double dc_f[kAdjEnt], dc_n[kAdjEnt]; // d col / d x_p of the entries, per side (0: that side does not touch it)
};
static_assert(sizeof(FoldRec) == 192, "FoldRec layout");

// plan: [n_rec][kFoldPlanInts] ints: layer, far segment, near segment (-1: none), n_ent, ent_p, ent_gf, layer_n, jrow
__global__ void sr_fold_pack_kernel(const int *__restrict__ plan, const double *__restrict__ col, int n_gas, int n_seg, int n_rec,
                                    FoldRec *__restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_rec) return;
  const int *pl = plan + (size_t)i * kFoldPlanInts;
  const int sf = pl[1], sn = pl[2];
  FoldRec r;
  r.layer = pl[0]; r.n_ent = pl[3]; r.layer_n = pl[12]; r.jrow = pl[13]; r.pad[0] = r.pad[1] = r.pad[2] = 0;
  bool same = sf >= 0 && sn >= 0 && r.layer == r.layer_n;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    r.u_f[g] = g < n_gas && sf >= 0 ? col[(size_t)g * n_seg + sf] : 0.0;
    r.u_n[g] = g < n_gas && sn >= 0 ? col[(size_t)g * n_seg + sn] : 0.0;
    same = same && fabs(r.u_f[g] - r.u_n[g]) <= 2e-15 * fabs(r.u_f[g]);
  }
  // The two segments of a shell on a symmetric path have the same column; the column integration leaves them a few
  // ulp apart in half of the cases (<= 4.4e-16 relative on the configs[3] rays): within 2e-15 they are taken as ONE
  // value, and the segments share their attenuation.
  if (same)
#pragma unroll
    for (int g = 0; g < 4; ++g) r.u_n[g] = r.u_f[g];
#pragma unroll
  for (int e = 0; e < kAdjEnt; ++e) {
    r.ent_p[e] = pl[4 + e];
    r.ent_gf[e] = pl[4 + kAdjEnt + e];
    r.dc_f[e] = e < r.n_ent && sf >= 0 ? col[(size_t)(n_gas + r.ent_p[e]) * n_seg + sf] : 0.0;
    r.dc_n[e] = e < r.n_ent && sn >= 0 ? col[(size_t)(n_gas + r.ent_p[e]) * n_seg + sn] : 0.0;
  }
  r.has = (sf >= 0 ? 1 : 0) | (sn >= 0 ? 2 : 0) | (same ? 4 : 0);
  out[i] = r;
}

// Rays per thread, NR: 1 as built (1.28-1.39 ms per configs[3] set; 2: 1.45-1.53, 4: 2.3 (spills); path order: 2.1, tools/adjoint_probe.py).
// TWO: the two segments of a shell read different coefficient rows (3-D paths: a row per LOS step; one ray per thread)
template <int NG, bool LAYER, bool PAR, int NR, bool TWO>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(SR_FOLD_WAVES, SR_FOLD_WAVES))) void sr_limb_adjoint_fold_kernel(
    const double *__restrict__ abs_c, const double *__restrict__ emi_c, const double *__restrict__ dabs,
    const double *__restrict__ demi, int n_pts, int n_layers, int n_jrows, const FoldRec *__restrict__ rec, // [n_batches][n_visits][NR]
    const int *__restrict__ zero_off, const int *__restrict__ zero_row, int n_par, LimbOpts o, int n_visits, int n_rays,
    double *__restrict__ rad, double *__restrict__ jac_layer, double *__restrict__ jac_par) {
  static_assert(!TWO || NR == 1, "rows per ray: one ray per thread");
  int pb, batch; // all batches of a point block on one XCD, one after the other (limb_block): 1.22 vs 1.28 ms per configs[3] set
  if (!limb_block((n_pts + 255) / 256, (n_rays + NR - 1) / NR, pb, batch)) return;
  const int j = pb * 256 + threadIdx.x;
  if (j >= n_pts) return;
  const int ray0 = batch * NR;
  const FoldRec *rc = rec + (size_t)batch * n_visits * NR;
  const size_t gstride = (size_t)n_layers * n_pts;
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    const int ray = ray0 + r;
    if (ray >= n_rays) continue;
    for (int q = zero_off[ray]; q < zero_off[ray + 1]; ++q) { // rows this ray never touches
      const int row = zero_row[q];
      if (row < n_jrows) {
        if (LAYER) jac_layer[((size_t)ray * n_jrows + row) * n_pts + j] = 0.0;
      } else if (PAR) {
        jac_par[((size_t)ray * n_par + (row - n_jrows)) * n_pts + j] = 0.0;
      }
    }
  }
  double If[NR], rem[NR], rem_lo[NR], Tn[NR], cs[NR], cs_lo[NR], Iobs[NR], Iobs_lo[NR];
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    If[r] = ray0 + r < n_rays ? limb_initial(o, rad, (size_t)(ray0 + r) * n_pts + j, j) : 0.0;
    rem[r] = rem_lo[r] = cs[r] = cs_lo[r] = 0.0;
    Tn[r] = 1.0;
  }
  auto two_sum_add = [](double &hi, double &lo, double x) {
    const double sm = hi + x, bb = sm - hi;
    lo += (hi - (sm - bb)) + (x - bb);
    hi = sm;
  };
  // sweep 1: the observed radiance and the path's optical depth
  for (int v = 0; v < n_visits; ++v) {
    const FoldRec *rv = rc + (size_t)v * NR;
    const size_t ofs = (size_t)rv[0].layer * n_pts + j;
    double a[NG], e[NG], a2[NG], e2[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      a[g] = abs_c[g * gstride + ofs];
      e[g] = emi_c[g * gstride + ofs];
      if (TWO) {
        const size_t ofs2 = (size_t)rv[0].layer_n * n_pts + j;
        a2[g] = abs_c[g * gstride + ofs2];
        e2[g] = emi_c[g * gstride + ofs2];
      } else {
        a2[g] = a[g];
        e2[g] = e[g];
      }
    }
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const FoldRec &R = rv[r];
      if (!R.has) continue; // wave-uniform
      Atten A;
      if (R.has & 1) {
        double tau = 0.0, E = 0.0;
#pragma unroll
        for (int g = 0; g < NG; ++g) {
          tau = g == 0 ? a[g] * R.u_f[g] : tau + a[g] * R.u_f[g];
          E = g == 0 ? e[g] * R.u_f[g] : E + e[g] * R.u_f[g];
        }
        two_sum_add(rem[r], rem_lo[r], tau);
        A = attenuation(tau);
        If[r] = If[r] * A.t + (o.solo_absorption ? 0.0 : E * A.f);
      }
      if (R.has & 2) {
        double tau = 0.0, E = 0.0;
#pragma unroll
        for (int g = 0; g < NG; ++g) {
          tau = g == 0 ? a2[g] * R.u_n[g] : tau + a2[g] * R.u_n[g];
          E = g == 0 ? e2[g] * R.u_n[g] : E + e2[g] * R.u_n[g];
        }
        two_sum_add(rem[r], rem_lo[r], tau);
        if (!(R.has & 4)) A = attenuation(tau);
        two_sum_add(cs[r], cs_lo[r], (o.solo_absorption ? 0.0 : E * Tn[r]) * A.f);
        Tn[r] *= A.t;
      }
    }
  }
  double slot[NR][4];
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    // I_obs = I_f Tn + cs as an unevaluated sum of two doubles (exact product, two-sums): see sweep 2
    const double p_hi = If[r] * Tn[r], p_lo = fma(If[r], Tn[r], -p_hi);
    Iobs[r] = cs[r];
    Iobs_lo[r] = cs_lo[r] + p_lo;
    two_sum_add(Iobs[r], Iobs_lo[r], p_hi);
    If[r] = ray0 + r < n_rays ? limb_initial(o, rad, (size_t)(ray0 + r) * n_pts + j, j) : 0.0; // (rad is written at the very end)
    cs[r] = cs_lo[r] = 0.0;
    Tn[r] = 1.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) slot[r][q] = 0.0;
  }
  // sweep 2: the weights, shell by shell
  for (int v = 0; v < n_visits; ++v) {
    const FoldRec *rv = rc + (size_t)v * NR;
    const size_t ofs = (size_t)rv[0].layer * n_pts + j;
    double a[NG], e[NG], da[NG], de[NG], a2[NG], e2[NG], da2[NG], de2[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      a[g] = abs_c[g * gstride + ofs];
      e[g] = emi_c[g * gstride + ofs];
      if (LAYER) {
        da[g] = dabs[g * gstride + ofs];
        de[g] = demi[g * gstride + ofs];
      }
      if (TWO) {
        const size_t ofs2 = (size_t)rv[0].layer_n * n_pts + j;
        a2[g] = abs_c[g * gstride + ofs2];
        e2[g] = emi_c[g * gstride + ofs2];
        if (LAYER) {
          da2[g] = dabs[g * gstride + ofs2];
          de2[g] = demi[g * gstride + ofs2];
        }
      } else {
        a2[g] = a[g];
        e2[g] = e[g];
        if (LAYER) {
          da2[g] = da[g];
          de2[g] = de[g];
        }
      }
    }
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const FoldRec &R = rv[r];
      if (!R.has) continue;
      const int ray = ray0 + r;
      Atten A;
      double fp = 0.0, d = 0.0, wt_f = 0.0, we_f = 0.0, wt_n = 0.0, we_n = 0.0;
      if (R.has & 1) {
        double tau = 0.0, E = 0.0, dtau = 0.0, dE = 0.0;
#pragma unroll
        for (int g = 0; g < NG; ++g) {
          const double u = R.u_f[g];
          tau = g == 0 ? a[g] * u : tau + a[g] * u;
          E = g == 0 ? e[g] * u : E + e[g] * u;
          if (LAYER) {
            dtau = fma(da[g], u, dtau);
            dE = fma(de[g], u, dE);
          }
        }
        A = attenuation(tau);
        fp = atten_fprime(A, tau);
        two_sum_add(rem[r], rem_lo[r], -tau);
        const double Ta = exp_bounded(fmin(fmax(-(rem[r] + rem_lo[r]), -700.0), 700.0)); // everything behind: the inner far side and the near side
        wt_f = (o.solo_absorption ? -If[r] * A.t : fma(E, fp, -If[r] * A.t)) * Ta;
        we_f = o.solo_absorption ? 0.0 : A.f * Ta;
        if (LAYER) d = fma(wt_f, dtau, we_f * dE);
        If[r] = If[r] * A.t + (o.solo_absorption ? 0.0 : E * A.f);
      }
      if (R.has & 2) {
        double tau = 0.0, E = 0.0, dtau = 0.0, dE = 0.0;
#pragma unroll
        for (int g = 0; g < NG; ++g) {
          const double u = R.u_n[g];
          tau = g == 0 ? a2[g] * u : tau + a2[g] * u;
          E = g == 0 ? e2[g] * u : E + e2[g] * u;
          if (LAYER) {
            dtau = fma(da2[g], u, dtau);
            dE = fma(de2[g], u, dE);
          }
        }
        if (!(R.has & 4)) {
          A = attenuation(tau);
          fp = atten_fprime(A, tau);
        }
        const double ETn = o.solo_absorption ? 0.0 : E * Tn[r];
        // I_in t Tn = I_obs - cs.  Both are carried as error-free sums (two doubles) of the SAME rounded terms -- the
        // operations of sweep 1, bit for bit -- so the difference is the sum of the terms still to come, I_f Tn(all) and
        // the inner segments' E f Tn, to THEIR relative accuracy: in one double it was good to eps x I_obs only, which
        // at a point whose tangent shells are hidden behind tau ~ 25 left 4e-22 on a value of 1e-25 (configs[3]: 1e-9
        // of a row's largest value)
        two_sum_add(cs[r], cs_lo[r], ETn * A.f);
        const double X = (Iobs[r] - cs[r]) + (Iobs_lo[r] - cs_lo[r]);
        wt_n = fma(ETn, fp, -X); // E f' Tn - I_in t Tn
        we_n = o.solo_absorption ? 0.0 : A.f * Tn[r];
        if (LAYER) d += fma(wt_n, dtau, we_n * dE);
        Tn[r] *= A.t;
      }
      if (LAYER) jac_layer[((size_t)ray * n_jrows + R.jrow) * n_pts + j] = d;
      if (PAR) {
        for (int i = 0; i < R.n_ent; ++i) {
          const int gf = R.ent_gf[i], g = gf & 0xff, sl = (gf >> 8) & 0xff, fl = gf >> 16;
          double ag = a[0], eg = e[0], ag2 = a2[0], eg2 = e2[0];
#pragma unroll
          for (int q = 1; q < NG; ++q) {
            ag = g == q ? a[q] : ag;
            eg = g == q ? e[q] : eg;
            ag2 = g == q ? a2[q] : ag2;
            eg2 = g == q ? e2[q] : eg2;
          }
          double val = fma(fma(wt_f, ag, we_f * eg), R.dc_f[i], fma(wt_n, ag2, we_n * eg2) * R.dc_n[i]);
          if (!(fl & 1)) val += sl == 0 ? slot[r][0] : (sl == 1 ? slot[r][1] : (sl == 2 ? slot[r][2] : slot[r][3]));
          if (fl & 2) {
            double *out = jac_par + ((size_t)ray * n_par + R.ent_p[i]) * n_pts + j;
            if (fl & 4) *out = val; else *out += val;
          } else {
            if (sl == 0) slot[r][0] = val; else if (sl == 1) slot[r][1] = val; else if (sl == 2) slot[r][2] = val; else slot[r][3] = val;
          }
        }
      }
    }
  }
  if (rad) {
#pragma unroll
    for (int r = 0; r < NR; ++r)
      if (ray0 + r < n_rays) rad[(size_t)(ray0 + r) * n_pts + j] = Iobs[r] + Iobs_lo[r];
  }
}

// ------------------------------------------------------------------------
// The folded recursion for FEW, BROAD column parameters (the retrieval loop of configs[4]: 7 profile parameters whose
// masks cover the whole path): the path-order forward-sensitivity kernel carries four derivatives through the recursion
// and repeats it per block of four, segment by segment; here a shell's coefficients are loaded once for its two
// segments and every parameter (up to kFoldDensePar) is carried along in ONE sweep: sr_limb_fold_sens_lds_kernel below.
// ------------------------------------------------------------------------
struct __attribute__((aligned(16))) FoldDense { // one ray in one shell
  int layer, has, pad0, pad1;                // has: as FoldRec
  double u_f[4], u_n[4];
  double dc_f[kFoldDensePar], dc_n[kFoldDensePar]; // d col / d x_p of the two segments
};
static_assert(sizeof(FoldDense) == 16 + 64 + 16 * kFoldDensePar, "FoldDense layout");
struct ParGas { int g[kFoldDensePar]; };

// plan: [n_rec][4] ints: layer, far segment, near segment (-1: none), 0
__global__ void sr_fold_dense_pack_kernel(const int *__restrict__ plan, const double *__restrict__ col, int n_gas, int n_par,
                                          int n_seg, int n_rec, FoldDense *__restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_rec) return;
  const int *pl = plan + (size_t)i * 4;
  const int sf = pl[1], sn = pl[2];
  FoldDense r;
  r.layer = pl[0]; r.pad0 = r.pad1 = 0;
  bool same = sf >= 0 && sn >= 0;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    r.u_f[g] = g < n_gas && sf >= 0 ? col[(size_t)g * n_seg + sf] : 0.0;
    r.u_n[g] = g < n_gas && sn >= 0 ? col[(size_t)g * n_seg + sn] : 0.0;
    same = same && fabs(r.u_f[g] - r.u_n[g]) <= 2e-15 * fabs(r.u_f[g]);
  }
  // The two segments of a shell on a symmetric path have the same column; the column integration leaves them a few
  // ulp apart in half of the cases (<= 4.4e-16 relative on the configs[3] rays): within 2e-15 they are taken as ONE
  // value, and the segments share their attenuation.
  if (same)
#pragma unroll
    for (int g = 0; g < 4; ++g) r.u_n[g] = r.u_f[g];
#pragma unroll
  for (int p = 0; p < kFoldDensePar; ++p) {
    r.dc_f[p] = p < n_par && sf >= 0 ? col[(size_t)(n_gas + p) * n_seg + sf] : 0.0;
    r.dc_n[p] = p < n_par && sn >= 0 ? col[(size_t)(n_gas + p) * n_seg + sn] : 0.0;
  }
  r.has = (sf >= 0 ? 1 : 0) | (sn >= 0 ? 2 : 0) | (same ? 4 : 0);
  out[i] = r;
}

// ONE sweep (round 5): forward sensitivities in fold order.  The far side carries dI_f / dx_p through the recursion
// (dI_f' = dI_f t + (w_tau a_g + w_E e_g) dc_far,p); the near side is visited from the observer inwards, so the
// transmission T_n between a segment and the observer is known when the segment is reached, and its logarithmic
// derivative D_p = sum a_g dc_near,p over the segments already passed is carried beside it:
//   d cs_p += T_n (f e_g + E f' a_g) dc_near,p - E f T_n D_p,   D_p += a_g dc_near,p,
//   d I_obs / d x_p = T_n (dI_f,p - I_f D_p) + d cs_p           (I_obs = I_f T_n + cs).
// Round 4's kernel ran two sweeps with one accumulator per parameter (sr_limb_adjoint_fold_kernel's quantities: 10 023
// VALU instructions per wave on configs[4] -- an attenuation() per shell and sweep, the exponential of the remaining
// optical depth, four error-free sums); here three accumulators per parameter, 4 300-5 000 instructions, and no
// difference of nearly equal sums anywhere: every term is a product of the quantities the radiance itself is made of.
// A parameter's gas is wave-uniform: the choice between the gases' weights is a scalar branch (the asm statements keep
// the compiler from turning it into per-lane selects, two v_cndmask per double).  profiles/r05_fold_sens_ab.txt.

// attenuation() with the polynomial's coefficients in SGPRs (the same operations, bit for bit): for a kernel whose
// registers are its accumulators (20 VGPRs of constants otherwise)
__device__ inline Atten attenuation_sc(double tau) {
  const double x = -tau;
  const double n = rint(x * 0x1.71547652b82fep+0);
  double r = fma(-n, 0x1.62e42fefa39efp-1, x);
  r = fma(-n, 0x1.abc9e3b39803fp-56, r);
  double p = fma3vs(r, 0x1.ade156a5dcb37p-26, 0x1.28af3fca7ab0cp-22);
  p = fma3s(r, p, 0x1.71dee623fde64p-19);
  p = fma3s(r, p, 0x1.a01997c89e6b0p-16);
  p = fma3s(r, p, 0x1.a01a014761f6ep-13);
  p = fma3s(r, p, 0x1.6c16c1852b7b0p-10);
  p = fma3s(r, p, 0x1.1111111122322p-7);
  p = fma3s(r, p, 0x1.55555555502a1p-5);
  p = fma3s(r, p, 0x1.5555555555511p-3);
  p = fma3s(r, p, 0x1.000000000000bp-1);
  const double pm1 = r * fma(r, p, 1.0);
  const double s = ldexp(1.0, (int)fmin(fmax(n, -1100.0), 1100.0));
  Atten A;
  A.t = fma(s, pm1, s);
  A.em1 = fma(-s, pm1, 1.0 - s);
  A.thin = !(fabs(tau) > 1e-12);
  A.rtau = fast_rcp<2>(tau);
  A.f = A.thin ? 1.0 : A.em1 * A.rtau;
  A.n0 = n == 0.0;
  A.fp0 = fma(fabs(r) < 0x1p-4 ? p - 0x1.6p-50 : p, 1.0 - r, -1.0);
  return A;
}

// The one-sweep kernel with the ray's records in LDS.  With the records read by scalar loads (the first one-sweep version)
// a wave waits for its 208-byte record (the scalar cache holds 16 KB, the rays resident on a CU stream 50 KB through
// it), THEN for the coefficients whose address the record gives, then computes: 46 % issue-busy at four waves per SIMD.
// Here a block copies its ray's records to LDS in chunks of kSensChunk shells; headers are read one shell ahead, so
// the next shell's coefficients are in flight during this shell's arithmetic, and the column derivatives arrive
// as LDS broadcasts under the attenuation.
constexpr int kSensChunk = 64;
constexpr int kSensRecD = 26; // doubles per FoldDense
static_assert(sizeof(FoldDense) == kSensRecD * 8, "FoldDense in doubles");
// BANDS (round 6): the instrument bands in the epilogue.  A retrieval iteration wants the band integrals of the block's
// eight or nine spectra (radiance + derivatives), not the spectra: S[q][b] = sum_j val_q(j) W_b(j) over the block's 256
// points is a [9 x 256] x [256 x n_bands] product -- a wave's values go through LDS and it multiplies its own 64 points
// with v_mfma_f64_16x16x4 (A = the values, rows padded to 16; B = a 16-band tile of the band-minor weight table) and
// stores ONE partial sum per (spectrum, band) and wave -- the 69 MB of spectra a configs[4] iteration wrote and
// sr_lowres_apply_kernel read again (57 us of a 350 us iteration) never exist.  (First version: per band a product per
// value and a lane reduction, 26 ds_bpermute each; configs[4]'s 14 bands all cover its whole grid: +27 us on the kernel's
// 260.)  part: [n_rays (1 + n_par)][64-point slots][band tiles][16], rows as sr_retrieval_forward_dev orders them;
// sr_lowres_sum_blocks_kernel adds a band's slots.
// (FoldBands and kBandRow: sr_limb_common.hpp -- sr_limb_jac_state_kernel's BANDS instances use them too)
constexpr int kBandVals = kFoldDensePar + 1;  // spectra per ray: the radiance and its derivatives
template <int NG, bool BANDS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(NG <= 2 ? 4 : 3, NG <= 2 ? 4 : 3))) void sr_limb_fold_sens_lds_kernel(
    const double *__restrict__ abs_c, const double *__restrict__ emi_c, int n_pts, int n_layers,
    const FoldDense *__restrict__ rec, // [n_rays][n_visits]
    int n_par, ParGas pg, LimbOpts o, int n_visits, int n_rays, double *__restrict__ rad, double *__restrict__ jac_par,
    FoldBands bd) {
  // the ray's records + a row of zeros; BANDS: + every wave's tile of values
  constexpr int kRecDoubles = kSensChunk * kSensRecD + kFoldDensePar;
  __shared__ double lrec[kRecDoubles + (BANDS ? 4 * kBandVals * kBandRow : 0)];
  int pb, ray; // all rays of a point block on one XCD, one after the other
  if (!limb_block((n_pts + 255) / 256, n_rays, pb, ray)) return; // (block-uniform)
  const int j0 = pb * 256 + threadIdx.x;
  const bool live = j0 < n_pts;
  const int j = live ? j0 : n_pts - 1; // (the block's barriers need every thread)
  const double *src = reinterpret_cast<const double *>(rec + (size_t)ray * n_visits);
  const size_t gstride = (size_t)n_layers * n_pts;
  double If = limb_initial(o, rad, (size_t)ray * n_pts + j, j), Tn = 1.0, cs = 0.0;
  double dIf[kFoldDensePar], dcs[kFoldDensePar], Dn[kFoldDensePar];
  int gmask = 0;
#pragma unroll
  for (int p = 0; p < kFoldDensePar; ++p) {
    dIf[p] = dcs[p] = Dn[p] = 0.0;
    gmask |= (pg.g[p] & 3) << (2 * p);
  }
  const bool solo = o.solo_absorption != 0;
  for (int v0 = 0; v0 < n_visits; v0 += kSensChunk) {
    const int nv = min(kSensChunk, n_visits - v0);
    __syncthreads(); // (the previous chunk has been consumed)
    for (int i = threadIdx.x; i < nv * kSensRecD; i += 256) lrec[i] = src[(size_t)v0 * kSensRecD + i];
    if (threadIdx.x < kFoldDensePar) lrec[kSensChunk * kSensRecD + threadIdx.x] = 0.0;
    __syncthreads();
    double an[NG], en[NG];
    int has_n;
    auto fetch = [&](int v) { // header of shell v of the chunk; its coefficients requested
      has_n = 0;
      if (v < nv) {
        const int2 hd = *reinterpret_cast<const int2 *>(lrec + v * kSensRecD);
        has_n = __builtin_amdgcn_readfirstlane(hd.y);
        const int layer = __builtin_amdgcn_readfirstlane(hd.x);
        if (has_n) {
          const size_t ofs = (size_t)layer * n_pts + j;
#pragma unroll
          for (int g = 0; g < NG; ++g) {
            an[g] = abs_c[g * gstride + ofs];
            en[g] = emi_c[g * gstride + ofs];
          }
        }
      }
    };
    fetch(0);
    for (int v = 0; v < nv; ++v) {
      const int has = has_n;
      double a[NG], e[NG];
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        a[g] = an[g];
        e[g] = en[g];
      }
      fetch(v + 1);
      if (!has) continue;
      const double *lr = lrec + v * kSensRecD;
      // one pass for a shell whose two segments have the same columns (has & 4: every shell of a 1-D limb path) or one
      // segment; otherwise the far segment, then the near one
      const int n_pass = (has & 7) == 3 ? 2 : 1;
      for (int k = 0; k < n_pass; ++k) {
        const bool far = (has & 1) && k == 0, near = (has & 2) && (k == 1 || n_pass == 1);
        const double *u = lr + (far ? 2 : 6);
        const double *lcf = lr + 10, *lcn = near ? lr + 18 : lrec + kSensChunk * kSensRecD; // (no near segment: zeros)
        // (LDS broadcasts: the first half of the parameters in flight under the attenuation, the second half under the
        // first half's steps -- all sixteen doubles at the top were 140 VGPRs, three waves per SIMD)
        constexpr int kH = kFoldDensePar / 2;
        double cf[kFoldDensePar], cn[kFoldDensePar];
#pragma unroll
        for (int p = 0; p < kH; ++p) {
          cf[p] = lcf[p];
          cn[p] = lcn[p];
        }
        double tau = a[0] * u[0], E = e[0] * u[0];
#pragma unroll
        for (int g = 1; g < NG; ++g) {
          tau = tau + a[g] * u[g];
          E = E + e[g] * u[g];
        }
        if (solo) E = 0.0;
        const Atten A = attenuation_sc(tau);
        const double fp = atten_fprime(A, tau);
        const double Ef = E * A.f, we = solo ? 0.0 : A.f;
        double t_f = 1.0, nEfTn = 0.0, bf[NG], wn[NG];
#pragma unroll
        for (int g = 0; g < NG; ++g) bf[g] = wn[g] = 0.0;
        if (far) {
          const double wt = fma(E, fp, -If * A.t);
#pragma unroll
          for (int g = 0; g < NG; ++g) bf[g] = fma(wt, a[g], we * e[g]);
          If = If * A.t + Ef;
          t_f = A.t;
        }
        if (near) {
          const double wtn = (E * Tn) * fp, wen = we * Tn;
#pragma unroll
          for (int g = 0; g < NG; ++g) wn[g] = fma(wtn, a[g], wen * e[g]);
          cs = fma(E * Tn, A.f, cs); // (sr_limb_fold_fwd_kernel's operations: the two kernels' radiances are the same doubles)
          nEfTn = -(Ef * Tn);
          Tn *= A.t;
        }
        // The parameters' gases as a bit field, made opaque per pass (hoisted out of the loop as 16 compare results they
        // cost 32 SGPRs and spill), and gas by gas, so that every (gas, parameter) step is its own block behind a scalar
        // branch (one chain over the gases per parameter was tail-merged into moves of the chosen weights)
        int gm = gmask, np = n_par;
        asm volatile("" : "+s"(gm), "+s"(np) : : "memory");
#pragma unroll
        for (int p = kH; p < kFoldDensePar; ++p) {
          cf[p] = lcf[p];
          cn[p] = lcn[p];
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
#pragma unroll
          for (int q = 0; q < NG; ++q) {
#pragma unroll
            for (int p = h * kH; p < (h + 1) * kH; ++p) {
              // (Round 6: a two-instruction step for the parameters whose column derivatives are both zero in a shell -- a
              // bit mask in the record header, a scalar branch per parameter -- was built: the second code path per
              // parameter cost 44 VGPR spills at this kernel's 128 registers, 0.26 -> 0.81 ms.  Not kept.)
              if (p < np && (NG == 1 || ((gm >> (2 * p)) & 3) == q)) {
                asm volatile("");
                dIf[p] = fma3(dIf[p], t_f, bf[q] * cf[p]);
                dcs[p] = fma(wn[q], cn[p], dcs[p]);
                dcs[p] = fma(nEfTn, Dn[p], dcs[p]);
                Dn[p] = fma(a[q], cn[p], Dn[p]);
              }
            }
          }
        }
      }
    }
  }
  if constexpr (BANDS) {
    // Wave by wave, no block barrier: a wave's values go through ITS rows of the tile, its 9 x 16 sums to its own slot of
    // `part`.  configs[4] (variant builds that leave parts out): main loop 259 us, + 23 here -- the sixteen MFMAs 9 (their
    // flops at the fp64 rate: rows and bands padded to 16), the stores 5, LDS 3; the weight loads nothing.
    constexpr int kV = kBandVals;
    const int c_lo = pb * 256, n_slots = 4 * ((n_pts + 255) / 256);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lo = lane & 15, kq = lane >> 4;
    const int n_tiles = (bd.n_bands + 15) >> 4;
    double *vt = lrec + kRecDoubles + wave * (kV * kBandRow);
    vt[lane] = live ? fma(If, Tn, cs) : 0.0;
#pragma unroll
    for (int p = 0; p < kFoldDensePar; ++p)
      vt[(1 + p) * kBandRow + lane] = live && p < n_par ? fma(Tn, fma(-If, Dn[p], dIf[p]), dcs[p]) : 0.0;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // A[row = lane & 15][k = lane >> 4], B[k][col = lane & 15], D[row = (lane >> 4) + 4 r][col]
    const double *va = vt + min(lo, kV - 1) * kBandRow + kq;
    double A[16];
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) A[ks] = lo < kV ? va[4 * ks] : 0.0;
    for (int tile = 0; tile < n_tiles; ++tile) {
      const double *wt = bd.Wt + (size_t)tile * n_pts * 16 + lo;
      double Bv[16]; // a tile's sixteen B operands requested together
#pragma unroll
      for (int ks = 0; ks < 16; ++ks) Bv[ks] = wt[(size_t)min(c_lo + 64 * wave + 4 * ks + kq, n_pts - 1) * 16]; // (beyond the grid A is zero)
      v4d acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int ks = 0; ks < 16; ++ks) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(A[ks], Bv[ks], acc, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int q = kq + 4 * r;
        if (q <= n_par) {
          const size_t row = q == 0 ? (size_t)ray : (size_t)n_rays + (size_t)ray * n_par + (q - 1);
          bd.part[((row * n_slots + 4 * pb + wave) * n_tiles + tile) * 16 + lo] = acc[r];
        }
      }
    }
    return;
  }
  if (!live) return;
#pragma unroll
  for (int p = 0; p < kFoldDensePar; ++p)
    if (p < n_par) jac_par[((size_t)ray * n_par + p) * n_pts + j] = fma(Tn, fma(-If, Dn[p], dIf[p]), dcs[p]);
  rad[(size_t)ray * n_pts + j] = fma(If, Tn, cs);
}

// The radiances alone, folded (ray batches; BASELINE configs[2]: 64 rays): one sweep over the shells, a shell's coefficients
// loaded once for the ray's two segments and -- the path being symmetric -- ONE attenuation() for both:
// I_obs = I_f(tangent) Tn(all) + sum E f Tn over the near side (sr_limb_adjoint_fold_kernel's sweep 1).
template <int NG>
__global__ __launch_bounds__(256) void sr_limb_fold_fwd_kernel(const double *__restrict__ abs_c, const double *__restrict__ emi_c,
                                                               int n_pts, int n_layers, const FoldDense *__restrict__ rec,
                                                               LimbOpts o, int n_visits, int n_rays, double *__restrict__ rad) {
  int pb, ray;
  if (!limb_block((n_pts + 255) / 256, n_rays, pb, ray)) return;
  const int j = pb * 256 + threadIdx.x;
  if (j >= n_pts) return;
  const FoldDense *rc = rec + (size_t)ray * n_visits;
  const size_t gstride = (size_t)n_layers * n_pts;
  double If = limb_initial(o, rad, (size_t)ray * n_pts + j, j), Tn = 1.0, cs = 0.0;
  constexpr int kB = NG == 1 ? 4 : 2; // visits whose loads are issued together
  for (int vb = 0; vb < n_visits; vb += kB) {
    double a[kB][NG], e[kB][NG];
#pragma unroll
    for (int t = 0; t < kB; ++t) {
      const FoldDense &Rl = rc[min(vb + t, n_visits - 1)];
      const bool on = Rl.has != 0; // wave-uniform: a shell this ray does not cross costs no loads
      const size_t ofs = (size_t)Rl.layer * n_pts + j;
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        a[t][g] = on ? abs_c[g * gstride + ofs] : 0.0;
        e[t][g] = on ? emi_c[g * gstride + ofs] : 0.0;
      }
    }
#pragma unroll
    for (int t = 0; t < kB; ++t) {
      if (vb + t >= n_visits) break;
      const FoldDense &R = rc[vb + t];
      if (!R.has) continue; // wave-uniform
      Atten A;
      if (R.has & 1) {
        double tau = a[t][0] * R.u_f[0], E = e[t][0] * R.u_f[0];
#pragma unroll
        for (int g = 1; g < NG; ++g) {
          tau = tau + a[t][g] * R.u_f[g];
          E = E + e[t][g] * R.u_f[g];
        }
        A = attenuation(tau);
        If = If * A.t + (o.solo_absorption ? 0.0 : E * A.f);
        if (R.has & 4) { // the near-side segment: same columns, same tau and E
          cs = fma(o.solo_absorption ? 0.0 : E * Tn, A.f, cs);
          Tn *= A.t;
        }
      }
      if ((R.has & 6) == 2) {
        double tau = a[t][0] * R.u_n[0], E = e[t][0] * R.u_n[0];
#pragma unroll
        for (int g = 1; g < NG; ++g) {
          tau = tau + a[t][g] * R.u_n[g];
          E = E + e[t][g] * R.u_n[g];
        }
        A = attenuation(tau);
        cs = fma(o.solo_absorption ? 0.0 : E * Tn, A.f, cs);
        Tn *= A.t;
      }
    }
  }
  rad[(size_t)ray * n_pts + j] = fma(If, Tn, cs);
}

int launch_fold_fwd(const int *plan, const double *col, int n_seg, int n_rec, FoldDense *rec, const double *abs_c,
                    const double *emi_c, int n_pts, int n_layers, int n_rays, int n_visits, const LimbOpts &o, double *rad,
                    hipStream_t st, bool pack) {
  bool found = false; // (an instance for o.n_gas exists and was launched)
  if (n_rec <= 0 || n_rays <= 0) return 0;
  if (pack)
    hipLaunchKernelGGL(sr_fold_dense_pack_kernel, dim3((n_rec + 63) / 64), dim3(64), 0, st, plan, col, o.n_gas, 0, n_seg, n_rec, rec);
  if (n_pts <= 0) return (int)hipGetLastError(); // (packing only)
  const dim3 grid(limb_grid((n_pts + 255) / 256, n_rays));
  found = by_ngas(o.n_gas, [&](auto ng) {
    hipLaunchKernelGGL(sr_limb_fold_fwd_kernel<decltype(ng)::value>, grid, dim3(256), 0, st, abs_c, emi_c, n_pts, n_layers, rec, o,
                       n_visits, n_rays, rad);
  });
  return found ? (int)hipGetLastError() : (int)hipErrorInvalidValue;
}

size_t fold_dense_bytes(int n_rec) { return sizeof(FoldDense) * (size_t)n_rec; }

int launch_fold_dense(const int *plan, const double *col, const int *par_gas_host, int n_par, int n_seg, int n_rec, FoldDense *rec,
                      const double *abs_c, const double *emi_c, int n_pts, int n_layers, int n_rays, int n_visits,
                      const LimbOpts &o, double *rad, double *jac_par, hipStream_t st, const void *lowres_scratch, int n_bands) {
  bool found = false; // (an instance for o.n_gas exists and was launched)
  if (n_rec <= 0 || n_pts <= 0 || n_rays <= 0 || n_par <= 0 || n_par > kFoldDensePar) return 0;
  hipLaunchKernelGGL(sr_fold_dense_pack_kernel, dim3((n_rec + 63) / 64), dim3(64), 0, st, plan, col, o.n_gas, n_par, n_seg, n_rec, rec);
  ParGas pg;
  for (int p = 0; p < kFoldDensePar; ++p) pg.g[p] = p < n_par ? par_gas_host[p] : 0;
  const dim3 grid(limb_grid((n_pts + 255) / 256, n_rays));
  FoldBands bd{nullptr, nullptr, nullptr, 0};
  if (lowres_scratch) {
    const LowresScratch L = lowres_layout(const_cast<void *>(lowres_scratch), n_pts, n_bands);
    bd = FoldBands{L.Wt, L.range, L.part, n_bands};
  }
  found = by_ngas(o.n_gas, [&](auto ng) {
    auto launch = [&](auto bands) {
      hipLaunchKernelGGL((sr_limb_fold_sens_lds_kernel<decltype(ng)::value, decltype(bands)::value>), grid, dim3(256), 0, st, abs_c,
                         emi_c, n_pts, n_layers, rec, n_par, pg, o, n_visits, n_rays, rad, jac_par, bd);
    };
    if (lowres_scratch) launch(std::true_type{});
    else launch(std::false_type{});
  });
  return found ? (int)hipGetLastError() : (int)hipErrorInvalidValue;
}

size_t fold_rec_bytes(int n_rec) { return sizeof(FoldRec) * (size_t)n_rec; }

int launch_fold_pack(const int *plan, const double *col, int n_gas, int n_seg, int n_rec, FoldRec *out, hipStream_t st) {
  if (n_rec <= 0) return 0;
  hipLaunchKernelGGL(sr_fold_pack_kernel, dim3((n_rec + 63) / 64), dim3(64), 0, st, plan, col, n_gas, n_seg, n_rec, out);
  return (int)hipGetLastError();
}

int launch_limb_adjoint_fold(const double *abs_c, const double *emi_c, const double *dabs, const double *demi, int n_pts,
                             int n_layers, int n_jrows, int two_rows, int n_rays, const FoldRec *rec, const int *zero_off,
                             const int *zero_row, int n_par, const LimbOpts &o, int n_visits, double *rad, double *jac_layer,
                             double *jac_par, hipStream_t st) {
  bool found = false; // (an instance for o.n_gas exists and was launched)
  if (n_pts <= 0 || n_rays <= 0 || n_visits <= 0) return 0;
  const dim3 grid(limb_grid((n_pts + 255) / 256, n_rays));
  found = by_ngas(o.n_gas, [&](auto ng) {
    by_jac_kinds(jac_layer, jac_par, [&](auto lay, auto par) {
      auto launch = [&](auto two) { // two_rows: a coefficient row per segment
        hipLaunchKernelGGL((sr_limb_adjoint_fold_kernel<decltype(ng)::value, decltype(lay)::value, decltype(par)::value, 1, decltype(two)::value>),
                           grid, dim3(256), 0, st, abs_c, emi_c, dabs, demi, n_pts, n_layers, n_jrows, rec, zero_off, zero_row, n_par,
                           o, n_visits, n_rays, rad, jac_layer, jac_par);
      };
      if (two_rows) launch(std::true_type{});
      else launch(std::false_type{});
    });
  });
  return found ? (int)hipGetLastError() : (int)hipErrorInvalidValue;
}

size_t adj_prog_bytes(int n_seg) { return sizeof(SegProg) * (size_t)n_seg; }

int launch_adj_pack(const int *plan, const double *col, int n_gas, int n_seg, SegProg *out, hipStream_t st) {
  if (n_seg <= 0) return 0;
  hipLaunchKernelGGL(sr_adj_pack_kernel, dim3((n_seg + 63) / 64), dim3(64), 0, st, plan, col, n_gas, n_seg, out);
  return (int)hipGetLastError();
}

int launch_limb_adjoint(const double *abs_c, const double *emi_c, const double *dabs, const double *demi, int n_pts,
                        int n_layers, int n_jrows, int n_rays, const int *seg_off, const SegProg *prog, const int *zero_off,
                        const int *zero_row, int n_par, const LimbOpts &o, double *rad, double *jac_layer,
                        double *jac_par, hipStream_t st) {
  bool found = false; // (an instance for o.n_gas exists and was launched)
  if (n_pts <= 0 || n_rays <= 0) return 0;
  const dim3 grid((n_pts + 255) / 256, n_rays);
  found = by_ngas(o.n_gas, [&](auto ng) {
    by_jac_kinds(jac_layer, jac_par, [&](auto lay, auto par) {
      hipLaunchKernelGGL((sr_limb_adjoint_kernel<decltype(ng)::value, decltype(lay)::value, decltype(par)::value>), grid, dim3(256), 0,
                         st, abs_c, emi_c, dabs, demi, n_pts, n_layers, n_jrows, seg_off, prog, zero_off, zero_row, n_par, o, rad,
                         jac_layer, jac_par);
    });
  });
  return found ? (int)hipGetLastError() : (int)hipErrorInvalidValue;
}

int launch_limb(const double *abs_c, const double *emi_c, int n_pts, int n_layers, int n_rays, const int *seg_off,
                const int *seg_layer, const double *col, const LimbOpts &o, double *rad, hipStream_t st) {
  bool found = false; // (an instance for o.n_gas exists and was launched)
  if (n_pts <= 0 || n_rays <= 0) return 0;
  if (o.n_gas > kFoldGasMax) return launch_limb_many(abs_c, emi_c, n_pts, n_layers, n_rays, seg_off, seg_layer, col, o, rad, st);
  // fewer than two waves per SIMD: the latency-bound variant (a function of the launch shape only)
  if (limb_launch_is_small(n_pts, n_rays)) {
    const dim3 gs(limb_grid((n_pts + 63) / 64, n_rays));
    found = by_ngas(o.n_gas, [&](auto ng) {
      hipLaunchKernelGGL(sr_limb_split_kernel<decltype(ng)::value>, gs, dim3(64 * kLimbParts), 0, st, abs_c, emi_c, n_pts, n_layers,
                         seg_off, seg_layer, col, o, n_rays, rad);
    });
    return found ? (int)hipGetLastError() : (int)hipErrorInvalidValue;
  }
  const dim3 grid(limb_grid((n_pts + 255) / 256, n_rays));
  found = by_ngas(o.n_gas, [&](auto ng) {
    hipLaunchKernelGGL(sr_limb_kernel<decltype(ng)::value>, grid, dim3(256), 0, st, abs_c, emi_c, n_pts, n_layers, seg_off, seg_layer,
                       col, o, n_rays, rad);
  });
  return found ? (int)hipGetLastError() : (int)hipErrorInvalidValue;
}

int launch_limb_jac(const double *abs_c, const double *emi_c, int n_pts, int n_layers, int n_rays, const int *seg_off,
                    const int *seg_layer, const double *col, const double *dcol, const int *par_gas, int n_par,
                    const LimbOpts &o, double *rad, double *jac, hipStream_t st) {
  bool found = false; // (an instance for o.n_gas exists and was launched)
  if (n_pts <= 0 || n_rays <= 0 || n_par <= 0) return 0;
  // Every block of NP parameters repeats the recursion (exp, expm1, the coefficient loads): with many parameters
  // (configs[3]: one per layer) 16 per thread instead of 4 cut the kernel's instructions 3.4x (160 segments x
  // (60 + NP) per block of NP).
  auto launch = [&](auto np) {
    found = by_ngas(o.n_gas, [&](auto ng) {
      constexpr int NP = decltype(np)::value;
      hipLaunchKernelGGL((sr_limb_jac_kernel<decltype(ng)::value, NP>), dim3((n_pts + 255) / 256, n_rays, (n_par + NP - 1) / NP),
                         dim3(256), 0, st, abs_c, emi_c, n_pts, n_layers, seg_off, seg_layer, col, dcol, par_gas, n_par, o, rad, jac);
    });
  };
  if (n_par > 8) launch(std::integral_constant<int, 16>{});
  else launch(std::integral_constant<int, 4>{});
  return found ? (int)hipGetLastError() : (int)hipErrorInvalidValue;
}

int launch_limb_jac_layer(const double *abs_c, const double *emi_c, const double *dabs, const double *demi, int n_pts,
                          int n_layers, int n_rays, const int *seg_off, const int *seg_layer, const double *col,
                          const LimbOpts &o, double *jac, hipStream_t st) {
  bool found = false; // (an instance for o.n_gas exists and was launched)
  if (n_pts <= 0 || n_rays <= 0 || n_layers <= 0) return 0;
  auto launch = [&](auto np) { // (the one-pass formulation is sr_limb_adjoint_kernel, launch_limb_adjoint)
    found = by_ngas(o.n_gas, [&](auto ng) {
      constexpr int NP = decltype(np)::value;
      hipLaunchKernelGGL((sr_limb_jac_layer_kernel<decltype(ng)::value, NP>), dim3((n_pts + 255) / 256, n_rays, (n_layers + NP - 1) / NP),
                         dim3(256), 0, st, abs_c, emi_c, dabs, demi, n_pts, n_layers, seg_off, seg_layer, col, o, jac);
    });
  };
  if (n_layers > 8) launch(std::integral_constant<int, 16>{});
  else launch(std::integral_constant<int, 4>{});
  return found ? (int)hipGetLastError() : (int)hipErrorInvalidValue;
}

// Which state unit holds the instances of a batch of n_gas gases with np slots per block (the one place that knows):
// a pair of gas counts and an NP each; above four gases the plan has 8 slots whatever its parameter count.
// nullptr: no unit, and so no instance -- the launcher answers hipErrorInvalidValue.
using StateUnit = int (*)(const StateLaunch &, const FoldBands &, int, hipStream_t);
static StateUnit state_unit(int n_gas, int np) {
  if (n_gas < 1 || n_gas > kLimbGasMax || (np != kLevelJacNPSmall && np != kLevelJacNPLarge)) return nullptr;
  const bool small = np == kLevelJacNPSmall;
  if (n_gas > kFoldGasMax) return small ? launch_limb_jac_state_many : nullptr;
  if (n_gas <= 2) return small ? launch_limb_jac_state_12_np8 : launch_limb_jac_state_12_np16;
  return small ? launch_limb_jac_state_34_np8 : launch_limb_jac_state_34_np16;
}

int launch_limb_jac_state(const StateLaunch &L, hipStream_t st) {
  const bool bands = L.lowres_scratch != nullptr;
  if (L.instr && !bands) return 0;
  if (L.n_pts <= 0 || L.n_rays <= 0 || L.n_par < (L.instr ? 0 : 1) || L.n_blocks <= 0) return 0;
  if (bands && L.n_bands <= 0) return 0;
  if ((L.lgas && L.o.n_gas < 2) || L.o.n_gas > kLimbGasMax) return (int)hipErrorInvalidValue; // (no such instance)
  FoldBands bd{};
  if (bands) {
    const LowresScratch S = lowres_layout(const_cast<void *>(L.lowres_scratch), L.n_pts, L.n_bands, L.instr);
    bd = FoldBands{S.Wt, S.range, S.part, L.n_bands};
  }
  const int n_row_par = L.n_par + (L.instr ? kLowresTables - 1 : 0); // the parameter rows of a ray in `part`
  // blocks per ray: a ray's blocks write the rows of the parameters that touch it, the others read as exact zeros --
  // cleared here, on the stream, ahead of the launch (the radiance rows of `part`, rows 0 .. n_rays - 1, are block 0's)
  const bool per_ray = L.ray_blk_off != nullptr;
  if (per_ray && (L.np != kLevelJacNPSmall && L.np != kLevelJacNPLarge)) return (int)hipErrorInvalidValue;
  if (per_ray && n_row_par > 0) {
    const size_t row = bands ? 4 * (size_t)((L.n_pts + 255) / 256) * ((L.n_bands + 15) / 16) * 16 : (size_t)L.n_pts;
    double *const rows = bands ? bd.part + (size_t)L.n_rays * row : L.jac;
    const hipError_t e = hipMemsetAsync(rows, 0, sizeof(double) * (size_t)L.n_rays * n_row_par * row, st);
    if (e != hipSuccess) return (int)e;
  }
  // the kernel's instances are other translation units'; the launch itself is one body (sr_limb_state_launch.inc).
  // The dense plan's slots per block: level_jac_np of the parameter count, which is 8 whatever the count above four
  // gases (state_gas_bits is 3 there) -- what the plan's builder (level_jac_plan) used.
  const StateUnit unit = state_unit(L.o.n_gas, per_ray ? L.np : level_jac_np(L.n_par, state_gas_bits(L.o.n_gas)));
  return unit ? unit(L, bd, n_row_par, st) : (int)hipErrorInvalidValue;
}

int launch_limb_parts(const double *abs_c, const double *emi_c, int n_pts, int n_layers, int n_rays, const int *seg_off,
                      const int *seg_layer, const double *col, const LimbOpts &o, int gas, const double *tab,
                      const int *coef_row, int n_blocks, const unsigned *words, const double *cc, const int *slot_level,
                      const int *slot_part, int n_part, double *rad, double *parts, hipStream_t st) {
  bool found = false; // (an instance for o.n_gas exists and was launched)
  if (n_pts <= 0 || n_rays <= 0 || n_part <= 0 || n_blocks <= 0) return 0;
  const dim3 grid(limb_grid((n_pts + 255) / 256, n_rays), 1, n_blocks);
  by_level_np(limb_parts_np(n_part), [&](auto np) {
    found = by_ngas(o.n_gas, [&](auto ng) {
      hipLaunchKernelGGL((sr_limb_parts_kernel<decltype(ng)::value, decltype(np)::value>), grid, dim3(256), 0, st, abs_c, emi_c, n_pts,
                         n_layers, seg_off, seg_layer, col, o, n_rays, gas, tab, coef_row, words, cc, slot_level, slot_part, n_part,
                         rad, parts);
    });
  });
  return found ? (int)hipGetLastError() : (int)hipErrorInvalidValue;
}

int launch_radiance_jac_layer(const double *abs_c, const double *emi_c, const double *dabs, const double *demi,
                              int n_pts, int n_layers, int n_rays, const int *seg_off, const int *seg_layer,
                              const double *seg_col, double *jac, hipStream_t st) {
  if (n_pts <= 0 || n_rays <= 0 || n_layers <= 0) return 0;
  constexpr int NP = 4;
  dim3 grid((n_pts + 255) / 256, n_rays, (n_layers + NP - 1) / NP);
  hipLaunchKernelGGL(sr_radiance_jac_layer_kernel<NP>, grid, dim3(256), 0, st, abs_c, emi_c, dabs, demi, n_pts,
                     n_layers, seg_off, seg_layer, seg_col, jac);
  return (int)hipGetLastError();
}

int launch_radiance_jac(const double *abs_c, const double *emi_c, int n_pts, int n_rays, const int *seg_off,
                        const int *seg_layer, const double *seg_col, const double *dcol, int n_par, double *rad,
                        double *jac, hipStream_t st) {
  if (n_pts <= 0 || n_rays <= 0 || n_par <= 0) return 0;
  constexpr int NP = 4;
  dim3 grid((n_pts + 255) / 256, n_rays, (n_par + NP - 1) / NP);
  hipLaunchKernelGGL(sr_radiance_jac_kernel<NP>, grid, dim3(256), 0, st, abs_c, emi_c, n_pts, n_rays, seg_off,
                     seg_layer, seg_col, dcol, n_par, rad, jac);
  return (int)hipGetLastError();
}

int launch_radiance(const double *abs_c, const double *emi_c, int n_pts, int n_rays, const int *seg_off,
                    const int *seg_layer, const double *seg_col, int init_from_rad, double *rad,
                    hipStream_t st) {
  if (n_pts <= 0 || n_rays <= 0) return 0;
  dim3 grid((n_pts + 255) / 256, n_rays);
  hipLaunchKernelGGL(sr_radiance_kernel, grid, dim3(256), 0, st, abs_c, emi_c, n_pts, n_rays, seg_off,
                     seg_layer, seg_col, init_from_rad, rad);
  return (int)hipGetLastError();
}

} // namespace sr
