// sr_solar_source.hip -- the solar subject's unit: the single-scattering solar source of coefficient rows
// (sr_solar_source_rows_dev: sr_solar_source.inc) and the solar attenuation in the Jacobians (sr_solar_jacobian_rows_dev:
// sr_solar_jac.inc), each kernel's text and its launcher.  A translation unit of its own, compiled beside the others: no
// other unit includes the kernels' text, and this one instantiates no other kernel.
//
//   sr_solar_source_kernel<ACC, TRANS>   four instances: overwrite / accumulate, with and without the transmission
//   sr_solar_jac_kernel<NR, ACC>         two instances: overwrite / accumulate, NR = kSolarJacRays rays per block
#include "sr_device.hpp"
#include "sr_kernels.hpp"
#include "sr_solar_plan.hpp"

namespace sr {

#include "sr_solar_source.inc"
#include "sr_solar_jac.inc"

int launch_solar_source(const double *tab_abs, int n_k, int n_pts, const double *u, const double *w, const int *src_row,
                        int n_rows, const int *tile_off, const int *chunks, const double *sca_abs, const double *sun,
                        bool accumulate, double *emi_out, double *trans_out, hipStream_t st) {
  if (n_rows <= 0 || n_pts <= 0) return 0;
  const dim3 grid(limb_grid((n_pts + 255) / 256, (n_rows + kSolarRows - 1) / kSolarRows));
  auto go = [&](auto acc, auto trans) {
    hipLaunchKernelGGL((sr_solar_source_kernel<decltype(acc)::value, decltype(trans)::value>), grid, dim3(256), 0, st, tab_abs, n_k,
                       n_pts, u, w, src_row, n_rows, tile_off, chunks, sca_abs, sun, emi_out, trans_out);
  };
  if (accumulate) {
    if (trans_out) go(std::true_type{}, std::true_type{});
    else go(std::true_type{}, std::false_type{});
  } else {
    if (trans_out) go(std::false_type{}, std::true_type{});
    else go(std::false_type{}, std::false_type{});
  }
  return (int)hipGetLastError();
}

int launch_solar_jac(const double *tab_abs, int n_k, int n_pts, const double *du, int n_par, int n_rows, const int *tile_off,
                     const int *chunks, const double *q, int n_rays, const int *par_slot, bool accumulate, double *jac,
                     int n_jac_rows, hipStream_t st) {
  if (n_par <= 0 || n_rows <= 0 || n_pts <= 0 || n_rays <= 0) return 0;
  const dim3 grid(limb_grid((n_pts + 255) / 256, n_par * ((n_rays + kSolarJacRays - 1) / kSolarJacRays)));
  if (accumulate)
    hipLaunchKernelGGL((sr_solar_jac_kernel<kSolarJacRays, true>), grid, dim3(256), 0, st, tab_abs, n_k, n_pts, du, n_par, n_rows,
                       tile_off, chunks, q, n_rays, par_slot, jac, n_jac_rows);
  else
    hipLaunchKernelGGL((sr_solar_jac_kernel<kSolarJacRays, false>), grid, dim3(256), 0, st, tab_abs, n_k, n_pts, du, n_par, n_rows,
                       tile_off, chunks, q, n_rays, par_slot, jac, n_jac_rows);
  return (int)hipGetLastError();
}

} // namespace sr
