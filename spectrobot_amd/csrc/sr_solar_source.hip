// sr_solar_source.hip -- the solar subject's unit: the single-scattering solar source of coefficient rows
// (sr_solar_source_rows_dev: sr_solar_source.inc) and the solar attenuation in the Jacobians (sr_solar_jacobian_rows_dev:
// sr_solar_jac.inc), both on the tile product of sr_solar_tile.inc, and the two-stream diffuse field under the sun, from
// thermal emission or both (sr_diffuse_source_rows_dev, sr_diffuse_thermal_rows_dev: sr_diffuse_source.inc), its tangent in
// the Jacobians (sr_diffuse_jacobian_rows_dev: sr_diffuse_jac.inc) and the solar field for several columns of illumination
// with the rows of LOS steps (sr_diffuse_source_columns_dev: sr_diffuse_columns.inc), each kernel's text and its launcher.
// A translation unit of its own, compiled beside the others: no other unit includes the kernels' text, and this one
// instantiates no other kernel.
//
//   sr_solar_source_kernel<ACC, TRANS>   four instances: overwrite / accumulate, with and without the transmission
//   sr_solar_jac_kernel<NR, ACC>         two instances: overwrite / accumulate, NR = kSolarJacRays rays per block
//   sr_diffuse_field_kernel<SOLAR, THERMAL, ACC, WJ, WF> twenty-four instances: the sun alone, thermal emission alone or
//                                         both (never neither), each overwrite / accumulate, with and without j_out / flux_out
//   sr_diffuse_tangent_kernel<NP, OPT>    two instances: NP = kDiffuseJacPars parameters per block; along column parameters,
//                                         and (OPT) along a direction in ssa, asym and the surface albedo
//   sr_diffuse_contract_kernel<NR, NP, ACC> two instances: overwrite / accumulate, kDiffuseJacRays x kDiffuseJacPars per thread
//   sr_diffuse_columns_kernel<NC, ACC>    eight instances: NC = 1, 2, 4, 8 columns, overwrite / accumulate
#include "sr_device.hpp"
#include "sr_kernels.hpp"
#include "sr_limb_dispatch.hpp"
#include "sr_solar_plan.hpp"

namespace sr {

#include "sr_solar_tile.inc"
#include "sr_solar_source.inc"
#include "sr_solar_jac.inc"
#include "sr_diffuse_source.inc"
#include "sr_diffuse_jac.inc"
#include "sr_diffuse_columns.inc"

int launch_solar_source(const double *tab_abs, int n_k, int n_pts, const double *u, const double *w, const int *src_row,
                        int n_rows, const int *tile_off, const int *chunks, const double *sca_abs, const double *sun,
                        bool accumulate, double *emi_out, double *trans_out, hipStream_t st) {
  if (n_rows <= 0 || n_pts <= 0) return 0;
  const dim3 grid(limb_grid((n_pts + 255) / 256, (n_rows + kSolarRows - 1) / kSolarRows));
  by_flag(accumulate, [&](auto acc) {
    by_flag(trans_out != nullptr, [&](auto trans) {
      hipLaunchKernelGGL((sr_solar_source_kernel<decltype(acc)::value, decltype(trans)::value>), grid, dim3(256), 0, st, tab_abs,
                         n_k, n_pts, u, w, src_row, n_rows, tile_off, chunks, sca_abs, sun, emi_out, trans_out);
    });
  });
  return (int)hipGetLastError();
}

int launch_solar_jac(const double *tab_abs, int n_k, int n_pts, const double *du, int n_par, int n_rows, const int *tile_off,
                     const int *chunks, const double *q, int n_rays, const int *par_slot, bool accumulate, double *jac,
                     int n_jac_rows, hipStream_t st) {
  if (n_par <= 0 || n_rows <= 0 || n_pts <= 0 || n_rays <= 0) return 0;
  const dim3 grid(limb_grid((n_pts + 255) / 256, n_par * ((n_rays + kSolarJacRays - 1) / kSolarJacRays)));
  by_flag(accumulate, [&](auto acc) {
    hipLaunchKernelGGL((sr_solar_jac_kernel<kSolarJacRays, decltype(acc)::value>), grid, dim3(256), 0, st, tab_abs, n_k, n_pts, du,
                       n_par, n_rows, tile_off, chunks, q, n_rays, par_slot, jac, n_jac_rows);
  });
  return (int)hipGetLastError();
}

int launch_diffuse_field(const double *tab_abs, int n_gas, int n_layers, int n_pts, int p_lo, int p_hi, const double *v,
                         const double *coef, const double *temps, const double *beam, const double *sun, double mu0,
                         double albedo, double t_surface, double w0, double step, int g_lo, bool own, int out_gas, double *ws,
                         int ws_stride, bool accumulate, double *emi_out, double *j_out, double *flux_out, hipStream_t st) {
  if (!beam && !temps) return (int)hipErrorInvalidValue; // a field without a source: <false, false> is not instantiated
  if (n_layers <= 0 || p_hi <= p_lo) return 0;
  const dim3 grid(limb_grid((p_hi - p_lo + 255) / 256, 1));
  auto go = [&](auto solar, auto thermal) {
    by_flag(accumulate && emi_out, [&](auto acc) {
      by_flag(j_out != nullptr, [&](auto wj) {
        by_flag(flux_out != nullptr, [&](auto wf) {
          hipLaunchKernelGGL((sr_diffuse_field_kernel<decltype(solar)::value, decltype(thermal)::value, decltype(acc)::value,
                                                      decltype(wj)::value, decltype(wf)::value>),
                             grid, dim3(256), 0, st, tab_abs, n_gas, n_layers, n_pts, p_lo, p_hi, v, coef, temps, beam, sun, mu0,
                             albedo, t_surface, w0, step, g_lo, (int)own, out_gas, ws, ws_stride, emi_out, j_out, flux_out);
        });
      });
    });
  };
  if (!temps) go(std::true_type{}, std::false_type{});
  else if (!beam) go(std::false_type{}, std::true_type{});
  else go(std::true_type{}, std::true_type{});
  return (int)hipGetLastError();
}

int launch_diffuse_tangent(const double *tab_abs, int n_gas, int n_layers, int n_pts, int p_lo, int p_hi, int par_lo, int par_hi,
                           const double *v, const double *dv, const double *coef, const int *mask, const double *beam,
                           const double *sun, const double *dlnbeam, double mu0, double albedo, double *ws, int ws_stride,
                           double *dj, int dj_stride, int dj_joff, int dj_par0, hipStream_t st) {
  if (n_layers <= 0 || p_hi <= p_lo || par_hi <= par_lo) return 0;
  const dim3 grid(limb_grid((p_hi - p_lo + 255) / 256, (par_hi - par_lo + kDiffuseJacPars - 1) / kDiffuseJacPars));
  hipLaunchKernelGGL((sr_diffuse_tangent_kernel<kDiffuseJacPars>), grid, dim3(256), 0, st, tab_abs, n_gas, n_layers, n_pts, p_lo,
                     p_hi, par_lo, par_hi, v, dv, coef, mask, beam, sun, dlnbeam, mu0, albedo, ws, ws_stride, dj, dj_stride, dj_joff,
                     dj_par0);
  return (int)hipGetLastError();
}

int launch_diffuse_optics_tangent(const double *tab_abs, int n_gas, int n_layers, int n_pts, int p_lo, int p_hi, int par_lo,
                                  int par_hi, const double *v, const double *dopt, const double *coef, const int *mask,
                                  const double *beam, const double *sun, const double *dlnbeam, double mu0, double albedo,
                                  double *ws, int ws_stride, double *dj, int dj_stride, int dj_joff, int dj_par0, hipStream_t st) {
  if (n_layers <= 0 || p_hi <= p_lo || par_hi <= par_lo) return 0;
  const dim3 grid(limb_grid((p_hi - p_lo + 255) / 256, (par_hi - par_lo + kDiffuseJacPars - 1) / kDiffuseJacPars));
  hipLaunchKernelGGL((sr_diffuse_tangent_kernel<kDiffuseJacPars, true>), grid, dim3(256), 0, st, tab_abs, n_gas, n_layers, n_pts, p_lo,
                     p_hi, par_lo, par_hi, v, dopt, coef, mask, beam, sun, dlnbeam, mu0, albedo, ws, ws_stride, dj, dj_stride, dj_joff,
                     dj_par0);
  return (int)hipGetLastError();
}

int launch_diffuse_contract(const double *q, int n_rays, int n_layers, int n_pts, int p_lo, int p_hi, int par_lo, int par_hi,
                            const double *dj, int dj_stride, int dj_joff, int dj_par0, const int *par_slot, bool accumulate,
                            double *jac, int n_jac_rows, hipStream_t st) {
  if (n_layers <= 0 || p_hi <= p_lo || par_hi <= par_lo || n_rays <= 0) return 0;
  const dim3 grid(limb_grid((p_hi - p_lo + 255) / 256, ((par_hi - par_lo + kDiffuseJacPars - 1) / kDiffuseJacPars) *
                                                           ((n_rays + kDiffuseJacRays - 1) / kDiffuseJacRays)));
  by_flag(accumulate, [&](auto acc) {
    hipLaunchKernelGGL((sr_diffuse_contract_kernel<kDiffuseJacRays, kDiffuseJacPars, decltype(acc)::value>), grid, dim3(256), 0, st,
                       q, n_rays, n_layers, n_pts, p_lo, p_hi, par_lo, par_hi, dj, dj_stride, dj_joff, dj_par0, par_slot, jac,
                       n_jac_rows);
  });
  return (int)hipGetLastError();
}

int launch_diffuse_columns(const double *tab_abs, int n_gas, int n_layers, int n_pts, int p_lo, int p_hi, const double *v,
                           const double *coef, const double *beam, int n_col, const double *sun, const double *mu0, double albedo,
                           double w_out, const int *row_off, const int *row_ix, const int *src_row, const double *col_w,
                           const double *sca_abs, double *ws, int ws_stride, bool accumulate, double *emi_out, double *j_out,
                           double *flux_out, hipStream_t st) {
  if (n_layers <= 0 || p_hi <= p_lo) return 0;
  const dim3 grid(limb_grid((p_hi - p_lo + 255) / 256, 1));
  auto go = [&](auto nc) {
    by_flag(accumulate && emi_out, [&](auto acc) {
      hipLaunchKernelGGL((sr_diffuse_columns_kernel<decltype(nc)::value, decltype(acc)::value>), grid, dim3(256), 0, st, tab_abs,
                         n_gas, n_layers, n_pts, p_lo, p_hi, v, coef, beam, n_col, sun, mu0, albedo, w_out, row_off, row_ix, src_row,
                         col_w, sca_abs, ws, ws_stride, emi_out, j_out, flux_out);
    });
  };
  switch (diffuse_columns_instance(n_col)) { // (mu0 and col_w are padded to the instance by diffuse_columns_plan)
  case 1: go(std::integral_constant<int, 1>()); break;
  case 2: go(std::integral_constant<int, 2>()); break;
  case 4: go(std::integral_constant<int, 4>()); break;
  default: go(std::integral_constant<int, kDiffuseColumns>()); break;
  }
  return (int)hipGetLastError();
}

} // namespace sr
