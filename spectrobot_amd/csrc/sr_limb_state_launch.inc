// sr_limb_state_launch.inc -- the one launch of sr_limb_jac_state_kernel from a StateLaunch: every combination of the
// kernel's compile-time parameters a call can reach, behind the dispatchers of the including translation unit.  Included
// inside namespace sr behind sr_limb_state.inc and by_flag (sr_limb_dispatch.hpp) by sr_limb_state_unit.hpp, and through
// it by every state unit -- sr_limb_state_{12,34}_np{8,16}.hip (NG = 1..4, NP = 8 or 16) and sr_limb_many.hip (NG = 6 or
// 8, NP = 8): one body, so the rules for gas / tab / rad and the order of the parameter pack cannot drift apart between
// them.
//   NP: the unit's slots per block (launch_limb_jac_state picks the unit by the plan's);
//   by_ng(f): f(integral_constant<int, NG>) for the batch's gas count among the unit's, false when it is none of them.
// bd: the band scratch's layout (BANDS), n_row_par: the parameter rows of a ray in `part`; the caller has made the checks
// of the record and cleared the rows of a launch with blocks per ray.  Returns the launch's status; a gas count without
// an instance is hipErrorInvalidValue, never a skipped launch.
template <int NP, class ByNG>
inline int launch_state_instances(const StateLaunch &L, const FoldBands &bd, int n_row_par, hipStream_t st, ByNG &&by_ng) {
  const bool bands = L.lowres_scratch != nullptr, rows = L.dabs && L.demi, per_ray = L.ray_blk_off != nullptr;
  const dim3 grid(limb_grid((L.n_pts + 255) / 256, L.n_rays), 1, L.n_blocks);
  // (gas, tab and n_tab_rows belong to the one-gas instances, rad to those that write spectra)
  const int gas = L.lgas ? -1 : L.gas, n_tab_rows = L.lgas ? 0 : L.n_tab_rows;
  const double *const tab = L.lgas ? nullptr : L.tab;
  double *const rad = bands ? nullptr : L.rad;
  const StateRayBlocks rbk{L.ray_blk_off, L.col_row};
  bool found = false;
  by_flag(L.blk != nullptr, [&](auto cols) { // no blk: the instances without column slots
    found = by_ng([&](auto ng) {
      by_flag(rows, [&](auto rw) {
        by_flag(bands, [&](auto bn) {
          by_flag(L.instr, [&](auto ins) {
            by_flag(L.lgas != nullptr, [&](auto several) {
              by_flag(per_ray, [&](auto rayblk) {
                constexpr int NG = decltype(ng)::value;
                constexpr bool COLS = decltype(cols)::value, ROWS = decltype(rw)::value, BANDS = decltype(bn)::value;
                constexpr bool INSTR = decltype(ins)::value, SEVERAL = decltype(several)::value, RAYBLK = decltype(rayblk)::value;
                // the instrument rows are band integrals; several level gases are several gases of the batch
                if constexpr ((BANDS || !INSTR) && (NG >= 2 || !SEVERAL)) {
                  auto launch_pack = [&](auto... pack) {
                    std::conditional_t<BANDS, FoldBands, double *> out;
                    if constexpr (BANDS) out = bd;
                    else out = L.jac;
                    hipLaunchKernelGGL((sr_limb_jac_state_kernel<NG, NP, COLS, ROWS, BANDS, INSTR, decltype(pack)...>), grid, dim3(256), 0,
                                       st, L.abs_c, L.emi_c, L.n_pts, L.n_layers, L.seg_off, L.seg_layer, L.col, L.dcol, L.o, L.n_rays, gas,
                                       tab, n_tab_rows, L.coef_row, L.blk, L.ent_off, L.ent, L.slot_par, n_row_par, rad, out, pack...);
                    g_last_state_instance = StateInstance{NG, NP, COLS, ROWS, BANDS, INSTR, SEVERAL, RAYBLK}; // the census
                  };
                  auto launch = [&](auto... pack) { // the ray blocks last
                    if constexpr (RAYBLK) launch_pack(pack..., rbk);
                    else launch_pack(pack...);
                  };
                  if constexpr (ROWS && SEVERAL) launch(L.dabs, L.demi, *L.lgas);
                  else if constexpr (ROWS) launch(L.dabs, L.demi);
                  else if constexpr (SEVERAL) launch(*L.lgas);
                  else launch();
                }
              });
            });
          });
        });
      });
    });
  });
  return found ? (int)hipGetLastError() : (int)hipErrorInvalidValue;
}
