// sr_limb_state.inc -- sr_limb_jac_state_kernel and what only it uses.  Included inside namespace sr by
// sr_limb_state_unit.hpp (the library's state units: sr_limb_state_*.hip and sr_limb_many.hip), and by the host builds
// under tools/ (tools/host_sim/hip_on_host.hpp) behind sr_limb_plan.hpp and sr_limb_common.hpp (FoldBands, kLowresTables,
// kBandRow).
// SR_PIN_SCALARS(a, b): the includer's -- pins two wave-uniform ints to scalar registers, or nothing on a host.

// the buffer limb_initial() reads with init_mode 1 (which the host refuses for the state kernel): none with BANDS
__device__ inline const double *limb_state_init_src(const double *jac) { return jac; }
__device__ inline const double *limb_state_init_src(const FoldBands &) { return nullptr; }

// the state kernel's trailing parameter pack: dabs and demi (ROWS), then the LevelGasTabs of a call with several level gases
template <class... T>
inline constexpr bool kStateSeveralGases = (std::is_same_v<T, LevelGasTabs> || ...);
template <class... R>
__device__ __forceinline__ const double *state_row_spectrum(int which, const double *dabs, const double *demi, const R &...) {
  return which == 0 ? dabs : demi;
}
template <class... R>
__device__ __forceinline__ const LevelGasTabs &state_level_gases(const LevelGasTabs &g, const R &...) { return g; }
template <class T, class... R>
__device__ __forceinline__ const LevelGasTabs &state_level_gases(const T &, const R &...r) { return state_level_gases(r...); }
// ... and last of all the StateRayBlocks of a launch with the parameter blocks PER RAY (RAYBLK below)
struct StateRayBlocks {
  const int *ray_blk_off; // [n_rays + 1]
  const int *col_row;     // [ray blocks][NP]
};
template <class... T>
inline constexpr bool kStateRayBlocks = (std::is_same_v<T, StateRayBlocks> || ...);
__device__ __forceinline__ const StateRayBlocks &state_ray_blocks(const StateRayBlocks &b) { return b; }
template <class T, class... R>
__device__ __forceinline__ const StateRayBlocks &state_ray_blocks(const T &, const R &...r) { return state_ray_blocks(r...); }

// Derivatives w.r.t. LEVEL parameters of one level-factored gas (sr_limb_rays_jac_level_dev, COLS = false) or w.r.t. a
// MIXED state vector of column and level parameters in one pass (sr_limb_rays_jac_state_dev, COLS = true).  The gas's
// coefficients are abs[r] = sum_L pop[r][L] A_L[row[r]], emi[r] likewise with E_L (the pair tables of
// sr_glevel_pairs_dev), and level parameter p moves the population of level lev[p] on coefficient row r by c[p][r].
// Both kinds feed the same recursion,
//   J_p <- J_p t + (-I t dtau_p + dE_p f + E f' dtau_p),
// and differ only in where dtau_p and dE_p come from:
//   column parameter of gas g (as sr_limb_jac_kernel):  dtau = a_g D,  dE = e_g D,  D = dcol[p][s]
//   level parameter of level L:  dtau = c u A_L[row[r]],  dE = c u E_L[row[r]]   (u the column of `gas`, c = c[p][r];
//                                the per-layer recursion above with dabs / demi replaced by table spectra times c)
// so a ray is walked once per block of NP parameters whatever their kinds: NP accumulators per thread, blocks of NP
// parameters on blockIdx.z.  The host lists the column parameters first (caller's order), then the level parameters in
// level order, and cuts the list into blocks of NP: in a block the column slots are slots 0 .. nc - 1 and stand for the
// consecutive parameters blockIdx.z NP + q (their dcol rows need no index table), the level slots follow in level order.
// blk [n_blocks][2] = nc, and the column slots' gases, two bits each.  Per (parameter block, coefficient row) the host
// lists the entries (slot, level, c) with c != 0 in level order (LevelEnt): one d = -I t dtau_L + dE_L f + E f' dtau_L
// per level touched, J_slot += c d per entry.  A block works on one ray, so nc, the gases, the D and the entry lists are
// wave-uniform: scalar loads, scalar branches, the accumulators indexed statically.  A column slot costs its D (a scalar
// load, all of a segment's issued together ahead of the exponential), a multiplication and an FMA on top of one
// (dsrc - I t a_g) per gas; a segment none of the block's level slots touches costs them J *= t.
// COLS = false compiles every column-slot line out: dcol and blk are never read and may be null, all slots are level
// slots.  The level slots' arithmetic is the same in both instances, operation for operation.
// Coefficients of segment s + 1 are loaded while s is worked on (a ray's segments are a dependent chain); rays and
// point blocks by limb_block(): all rays of a point block on one XCD, so that the table rows they share are read from
// HBM once.
// ROWS = true adds a third kind (sr_limb_rays_jac_state_rows_dev): a ROW parameter p acts through the coefficients of
// every gas, with a weight w[p][r] per coefficient row (kinetic-temperature nodes: dabs / demi = d abs / dT, d emi / dT,
// [NG][n_layers][n_pts], the columns held fixed),
//   row parameter:  dtau = w sum_g u_g dabs_g[r],  dE = w sum_g u_g demi_g[r]
// sr_limb_jac_layer_kernel's expression contracted with the weights inside the recursion.  The row slots ride on the entry
// lists: behind a row's level entries the host appends one entry per row slot with w != 0, its level kLevelEntRows and
// c = w, so the sums are formed once per segment (2 NG loads at (g, r, j); the columns u_g are read again there, scalar
// loads that hit the scalar cache, rather than kept in scalar registers over the exponential) and every row slot costs
// its one multiply-add; a row no row slot weights costs nothing.  dabs and demi are the kernel's last two arguments and
// exist with ROWS = true only (row_spectra, empty otherwise): the ROWS = false instances keep their argument block and
// with it their machine code, instruction for instruction.
// BANDS = true (sr_limb_rays_state_bands_dev): the instrument bands in the epilogue, as sr_limb_fold_sens_lds_kernel<., true>
// integrates them.  The recursion is the same, operation for operation; at its end a wave's values -- its NP accumulators,
// and in parameter block 0 the radiance -- go through the wave's own tile in LDS (row q = slot q, row NP = the radiance) and
// are multiplied with the 16-band tiles of Wt by v_mfma_f64_16x16x4: ONE partial sum per (spectrum, band, wave) in `part`
// [(row n_slots + 4 pb + wave) n_tiles + tile][16], rows as sr_retrieval_forward_dev orders them (row ray = the radiance,
// row n_rays + ray n_par + p = parameter p), which sr_lowres_sum_blocks_kernel adds.  A block writes the rows of its own
// slots (slot_par >= 0), block 0 the radiance row too.  NP = 16 and the radiance are 17 rows, one more than an MFMA tile:
// block 0 alone runs a SECOND row tile that holds the radiance (NP = 8: nine rows, one tile).  No lane leaves early: a
// wave needs its 64 lanes for the product, so lanes beyond the grid work on its last point (`live` false) and put exact
// zeros into the tile; waves that lie wholly beyond the grid leave (the sum kernel reads only slots inside a band's point
// range).  An accumulator no segment of the ray touches is an exact 0 and so is every one of its sums.  `jac` is the
// FoldBands of the call in these instances and rad is not used; the BANDS = false instances keep their argument block,
// their early exit and their stores: the same machine code as before the parameter existed.
// SEVERAL level-factored gases (sr_limb_rays_jac_state_gases_dev, sr_limb_rays_state_bands_gases_dev): the parameter pack
// ends in a LevelGasTabs -- the tables, their row counts and the batch gases of up to four level gases, by value in the
// argument block -- and an entry's `level` is level | level gas << kLevelEntGasShift (the host sorts the level slots by
// level gas, then level, so "two loads and one d per distinct level" holds as it stands: the comparison of the packed
// words is the comparison of (level gas, level)).  A level slot of level gas k then reads
//   dtau = c u_{gas[k]} A^k_L[row_k[r]],  dE = c u_{gas[k]} E^k_L[row_k[r]],  row_k = coef_row + k n_layers,
// the table pointer, the row count and the gas index by scalar loads from the argument block where the level changes, the
// column u by a scalar load that hits the scalar cache (as the ROWS branch reads its columns: nothing of this is kept
// in scalar registers over the exponential; the COLS instances sit at the scalar-register limit).  The recursion term,
// the row slots, the kLevelEntRows sentinel and the band epilogue are untouched; gas, tab and n_tab_rows are not read.
// The instances without a LevelGasTabs keep their argument block and their machine code.
// INSTR = true (sr_limb_rays_state_bands_instr_dev, BANDS instances only): the two instrument derivatives of the radiance's
// bands, d / d centre and d / d ln width (sr_lowres_weights_kernel).  They are band integrals of the radiance alone with
// other weights, and those weights lie in Wt as further band tiles (table k at tile k n_tiles + tile, k = 1, 2): in
// parameter block 0 the tile loop of the row tile that holds the radiance runs over them too -- the same A operands, the
// same MFMA chain -- and stores that ONE row, to the rows of parameters n_par - 2 and n_par - 1 (the host counts the two
// instrument rows into n_par: they are the last two "parameters" of every ray, so the rows of `part`, the sum kernel and
// the field of view take them as they are).  slot_par never names them.  The recursion, every other row and the
// INSTR = false instances are untouched: same argument block, same machine code.
// RAYBLK (sr_set_state_ray_blocks: the parameter pack ends in a StateRayBlocks): parameter blocks PER RAY.  The dense plan
// cuts the batch's parameter list, so every ray is walked gridDim.z times whatever it touches; here every ray has its own
// list -- the parameters that touch it (ray_jac_plan) -- cut into its own blocks, and the tables blk, ent_off and slot_par
// are indexed by ray_blk_off[ray] + blockIdx.z.  gridDim.z is the largest block count of a ray; a workgroup beyond its
// ray's count leaves at once (wave-uniform, two scalar loads).  A ray's column slots are not consecutive parameters:
// col_row [ray blocks][NP] names the row of dcol behind each, read by scalar loads.  The indices are loop-invariant and
// left to the compiler, which keeps them over the segment loop: re-read per segment (through SR_PIN_SCALARS, so that
// they are dead over the exponential) every D load waits for its index load, two dependent scalar loads per segment,
// and the call was 13 % slower (DESIGN 4.7h); the instances spill fewer scalars than the dense ones either way.  The
// recursion, the entry loop, the row slots, the level-gas lookup and the band epilogue are the same operations; `first`
// is still blockIdx.z == 0, the radiance's block of every ray.  Rows of jac / part that no block of a ray writes are
// cleared by the host on the stream ahead of the launch.  The instances without a StateRayBlocks keep their argument block
// and their machine code.
// MORE THAN FOUR GASES (NG > kFoldGasMax, NP = 8; instantiated by sr_limb_many.hip): blk's gas word holds three bits per
// column slot, gas of slot q = gws >> 3 q & 7 (state_gas_bits; the host's plans pack them so), and an instance may have
// more gas slots than the batch has gases -- o.n_gas of them are live, the launcher takes the next instance up.  A
// padding slot reads gas 0's coefficient rows (limb_load_coef_padded: every load is valid) and column 0 (state_column),
// and its column counts as an exact 0: tau + a 0, E + e 0 and the row sums' fma(., 0, .) return their other operand for
// finite a and e, no column slot names the padding gas, so no result depends on it.  The recursion, the entry loop, the
// row slots, the level-gas lookup and the band epilogue are the same operations; every line of it stands behind a
// constexpr of NG, and the instances of at most four gases keep their machine code.
template <bool PAD>
__device__ __forceinline__ double state_column(const double *__restrict__ col, int g, int n_live, int n_seg_total, int s) {
  if constexpr (PAD) {
    const bool on = g < n_live;
    const double u = col[(size_t)(on ? g : 0) * n_seg_total + s];
    return on ? u : 0.0;
  } else {
    return col[(size_t)g * n_seg_total + s];
  }
}
template <int NG, int NP, bool COLS, bool ROWS, bool BANDS, bool INSTR, class... RowSpectra>
__global__ __launch_bounds__(256) void sr_limb_jac_state_kernel(
    const double *__restrict__ abs_c, const double *__restrict__ emi_c, int n_pts, int n_layers,
    const int *__restrict__ seg_off, const int *__restrict__ seg_layer, const double *__restrict__ col,
    const double *__restrict__ dcol, LimbOpts o, int n_rays, int gas, const double *__restrict__ tab, int n_tab_rows,
    const int *__restrict__ coef_row, const int *__restrict__ blk, const int *__restrict__ ent_off,
    const LevelEnt *__restrict__ ent, const int *__restrict__ slot_par, int n_par, double *__restrict__ rad,
    std::conditional_t<BANDS, FoldBands, double *__restrict__> jac, RowSpectra... row_spectra) {
  static_assert(NG <= kFoldGasMax ? NP <= 16 : (NG <= kLimbGasMax && NP <= kLevelJacNPSmall),
                "blk packs the gases of a block's column slots: 16 slots of two bits (up to four gases) or 8 of three (up to eight)");
  constexpr bool PAD = NG > kFoldGasMax; // (the instances that may have more gas slots than the batch has gases)
  constexpr int kGasBits = PAD ? 3 : 2;
  constexpr unsigned kGasMask = (1u << kGasBits) - 1u;
  static_assert(BANDS || !INSTR, "the instrument rows are band integrals");
  constexpr bool GASES = kStateSeveralGases<RowSpectra...>, RAYBLK = kStateRayBlocks<RowSpectra...>;
  static_assert(sizeof...(RowSpectra) == (ROWS ? 2 : 0) + (GASES ? 1 : 0) + (RAYBLK ? 1 : 0),
                "dabs and demi with ROWS, then the level gases' tables, if several, then the ray blocks, if per ray");
  int pb, ray;
  if (!limb_block((n_pts + 255) / 256, n_rays, pb, ray)) return;
  unsigned rb = blockIdx.z; // the block's row in blk, ent_off and slot_par
  if constexpr (RAYBLK) {
    const int *const off = state_ray_blocks(row_spectra...).ray_blk_off;
    const int b0 = off[ray];
    if ((int)blockIdx.z >= off[ray + 1] - b0) return; // (the ray has fewer blocks than the longest list)
    rb = (unsigned)b0 + blockIdx.z;
  }
  const int jt = pb * 256 + threadIdx.x;
  if (BANDS ? jt - (int)(threadIdx.x & 63) >= n_pts : jt >= n_pts) return; // BANDS: only whole waves beyond the grid leave
  [[maybe_unused]] const bool live = jt < n_pts;
  const int j = BANDS ? min(jt, n_pts - 1) : jt;
  double I = limb_initial(o, limb_state_init_src(jac), 0, j), J[NP]; // init_mode 1 is refused by the host for this kernel
#pragma unroll
  for (int q = 0; q < NP; ++q) J[q] = 0.0;
  const int nc = COLS ? blk[2 * rb] : 0;
  const unsigned gw = COLS ? (unsigned)blk[2 * rb + 1] : 0u;
  const double *dc = dcol + (RAYBLK ? (size_t)0 : (size_t)rb * NP * o.n_seg_total); // (read with nc > 0 only)
  const int *eo = ent_off + (size_t)rb * (n_layers + 1);
  const int s0 = seg_off[ray], s1 = seg_off[ray + 1];
  const size_t gstride = (size_t)n_layers * n_pts, plane = (size_t)n_tab_rows * n_pts;
  double an[NG], en[NG];
  if (s0 < s1) {
    if constexpr (PAD) limb_load_coef_padded<NG>(abs_c, emi_c, gstride, (size_t)seg_layer[s0] * n_pts + j, o.n_gas, an, en);
    else limb_load_coef<NG>(abs_c, emi_c, gstride, (size_t)seg_layer[s0] * n_pts + j, an, en);
  }
  for (int s = s0; s < s1; ++s) {
    const int r = seg_layer[s];
    double a[NG], e[NG], D[NP];
    double tau = 0.0, E = 0.0, ug = 0.0;
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      a[g] = an[g];
      e[g] = en[g];
      const double u = state_column<PAD>(col, g, o.n_gas, o.n_seg_total, s);
      tau = g == 0 ? a[g] * u : tau + a[g] * u;
      E = g == 0 ? e[g] * u : E + e[g] * u;
      ug = g == gas ? u : ug;
    }
    if (nc > 0) {
      if constexpr (RAYBLK) { // the slots' rows of dcol through col_row (loop-invariant: the compiler keeps the indices)
        const int *cr = state_ray_blocks(row_spectra...).col_row + (size_t)rb * NP;
#pragma unroll
        for (int q = 0; q < NP; ++q) D[q] = dc[(size_t)cr[min(q, nc - 1)] * o.n_seg_total + s];
      } else {
#pragma unroll
        for (int q = 0; q < NP; ++q) D[q] = dc[(size_t)min(q, nc - 1) * o.n_seg_total + s];
      }
    }
    if constexpr (PAD) limb_load_coef_padded<NG>(abs_c, emi_c, gstride, (size_t)seg_layer[min(s + 1, s1 - 1)] * n_pts + j, o.n_gas, an, en);
    else limb_load_coef<NG>(abs_c, emi_c, gstride, (size_t)seg_layer[min(s + 1, s1 - 1)] * n_pts + j, an, en);
    const Atten A = attenuation(tau);
    const double t = A.t, em1 = A.em1, f = A.f;
    const bool thin = A.thin;
    const double src = o.solo_absorption ? 0.0 : E * f;
    const int e0 = eo[r], e1 = eo[r + 1];
    double fp = 0.0, W[NG];
    if (nc > 0 || e0 < e1) fp = atten_fprime(A, tau);
    if (nc > 0) { // what a column slot of gas g adds per unit of its D: sr_limb_jac_kernel's (dsrc - I t a_g), once per gas
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        const double dsrc = o.solo_absorption ? 0.0 : fma(E * fp, a[g], e[g] * f);
        W[g] = dsrc - I * t * a[g];
      }
    }
    // (nc and the gases are loop-invariant: left to itself the compiler keeps every slot's comparisons in scalar
    // register pairs over the whole loop, NP NG of them, and spills; re-read through an empty asm they are formed
    // where they are used)
    int ncs = nc;
    unsigned gws = gw;
    if constexpr (COLS) SR_PIN_SCALARS(ncs, gws);
#pragma unroll
    for (int q = 0; q < NP; ++q) {
      if (COLS && q < ncs) { // a column slot: sr_limb_jac_kernel's update
        if constexpr (NG == 1) {
          J[q] = fma(J[q], t, W[0] * D[q]);
        } else { // the gas is chosen on the scalar side: D or 0 per gas, the products with 0 add nothing
          const unsigned gq = gws >> (kGasBits * q) & kGasMask;
          double x = W[0] * (gq == 0u ? D[q] : 0.0);
#pragma unroll
          for (int g = 1; g < NG; ++g) x = fma(W[g], gq == (unsigned)g ? D[q] : 0.0, x);
          J[q] = fma(J[q], t, x);
        }
      } else {
        J[q] *= t;
      }
    }
    if (e0 < e1) { // the level slots
      [[maybe_unused]] const double *tr = nullptr;
      if constexpr (!GASES) tr = tab + (size_t)coef_row[r] * n_pts + j;
      int lev = -1;
      double d = 0.0;
      for (int i = e0; i < e1; ++i) {
        const int slot = ent[i].slot, lv = ent[i].level;
        if (lv != lev) { // (entries in level order: two loads and one d per distinct level)
          lev = lv;
          bool rows = false;
          if constexpr (ROWS) rows = lv == kLevelEntRows;
          if (rows) { // the row slots: one d for all of them (sr_limb_jac_layer_kernel's sums)
            if constexpr (ROWS) {
              const double *const rs[] = {state_row_spectrum(0, row_spectra...), state_row_spectrum(1, row_spectra...)};
              const size_t ofs = (size_t)r * n_pts + j;
              double dtau = 0.0, dE = 0.0;
#pragma unroll
              for (int g = 0; g < NG; ++g) {
                if constexpr (PAD) { // (a padding slot: gas 0's rows, an exact zero for its column)
                  const double u = state_column<true>(col, g, o.n_gas, o.n_seg_total, s);
                  const size_t go = (g < o.n_gas ? (size_t)g : (size_t)0) * gstride + ofs;
                  dtau = fma(rs[0][go], u, dtau);
                  dE = fma(rs[1][go], u, dE);
                } else {
                  const double u = col[(size_t)g * o.n_seg_total + s];
                  dtau = fma(rs[0][g * gstride + ofs], u, dtau);
                  dE = fma(rs[1][g * gstride + ofs], u, dE);
                }
              }
              d = -I * t * dtau + (o.solo_absorption ? 0.0 : dE * f + E * fp * dtau);
            }
          } else if constexpr (GASES) { // a level of level gas k: its table, its row map, its gas's column
            const LevelGasTabs &lg = state_level_gases(row_spectra...);
            const int k = lv >> kLevelEntGasShift, L = lv & kLevelEntLevelMask;
            const size_t pl = (size_t)lg.n_tab_rows[k] * n_pts;
            const double *tl = lg.tab[k] + (size_t)coef_row[(size_t)k * n_layers + r] * n_pts + j + (size_t)L * 2 * pl;
            const double u = col[(size_t)lg.gas[k] * o.n_seg_total + s];
            const double dtau = u * tl[0], dE = u * tl[pl];
            d = -I * t * dtau + (o.solo_absorption ? 0.0 : dE * f + E * fp * dtau);
          } else {
            const double *tl = tr + (size_t)lv * 2 * plane;
            const double dtau = ug * tl[0], dE = ug * tl[plane];
            d = -I * t * dtau + (o.solo_absorption ? 0.0 : dE * f + E * fp * dtau);
          }
        }
        const double v = ent[i].c * d;
#pragma unroll
        for (int q = 0; q < NP; ++q) J[q] += q == slot ? v : 0.0;
      }
    }
    I = I * t + src;
  }
  if constexpr (BANDS) {
    // Wave by wave, no block barrier (sr_limb_fold_sens_lds_kernel's epilogue): a wave's values go through ITS tile, its
    // sums to its own slot of `part`.
    constexpr int kV = NP + 1; // rows of a wave's tile: the slots, then the radiance
    __shared__ double tiles[4 * kV * kBandRow];
    const FoldBands &bd = jac;
    const int c_lo = pb * 256, n_slots = 4 * ((n_pts + 255) / 256);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lo = lane & 15, kq = lane >> 4;
    const int n_tiles = (bd.n_bands + 15) >> 4;
    const bool first = blockIdx.z == 0;
    const int n_val = first ? kV : NP; // (the radiance is block 0's)
    double *vt = tiles + wave * (kV * kBandRow);
#pragma unroll
    for (int q = 0; q < NP; ++q) vt[q * kBandRow + lane] = live ? J[q] : 0.0;
    vt[NP * kBandRow + lane] = live && first ? I : 0.0;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // A[row = lane & 15][k = lane >> 4], B[k][col = lane & 15], D[row = (lane >> 4) + 4 r][col]; row tile rt holds the
    // values 16 rt .. 16 rt + 15 (a second one with NP = 16 in block 0 only: the radiance)
    for (int rt = 0; 16 * rt < n_val; ++rt) {
      const int vr = 16 * rt + lo;
      const double *va = vt + min(vr, kV - 1) * kBandRow + kq;
      double A[16];
#pragma unroll
      for (int ks = 0; ks < 16; ++ks) A[ks] = vr < n_val ? va[4 * ks] : 0.0;
      long long orow[4]; // the rows of `part` this lane's four sums belong to, or -1
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int q = 16 * rt + kq + 4 * r;
        const int p = slot_par[rb * NP + min(q, NP - 1)];
        orow[r] = q < NP ? (p >= 0 ? (long long)n_rays + (long long)ray * n_par + p : -1) : (q == NP && first ? (long long)ray : -1);
      }
      // INSTR: in block 0 the row tile that holds the radiance (value NP: row NP & 15 of row tile NP / 16, held by the lanes
      // kq == (NP & 3) in acc[(NP & 15) >> 2]) goes on over the tiles of the two derivative tables -- the same loop, the
      // same operands -- and stores that one row (a second loop of its own cost 36 VGPRs and a wave per SIMD)
      int n_tl = n_tiles;
      if constexpr (INSTR) n_tl = first && rt == NP / 16 ? kLowresTables * n_tiles : n_tiles;
      for (int tile = 0; tile < n_tl; ++tile) {
        const double *wt = bd.Wt + (size_t)tile * n_pts * 16 + lo;
        double Bv[16]; // a tile's sixteen B operands requested together
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) Bv[ks] = wt[(size_t)min(c_lo + 64 * wave + 4 * ks + kq, n_pts - 1) * 16]; // (beyond the grid A is zero)
        v4d acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(A[ks], Bv[ks], acc, 0, 0, 0);
        if constexpr (INSTR) {
          if (tile >= n_tiles) { // (wave-uniform) table k = 1, 2, its band tile bt: the instrument row n_par - 3 + k of the ray
            const int k = tile >= 2 * n_tiles ? 2 : 1, bt = tile - k * n_tiles;
            const size_t row = (size_t)n_rays + (size_t)ray * n_par + (n_par - kLowresTables + k);
            if (kq == (NP & 3)) bd.part[((row * n_slots + 4 * pb + wave) * n_tiles + bt) * 16 + lo] = acc[(NP & 15) >> 2];
            continue;
          }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (orow[r] >= 0) bd.part[(((size_t)orow[r] * n_slots + 4 * pb + wave) * n_tiles + tile) * 16 + lo] = acc[r];
      }
    }
  } else {
    if (blockIdx.z == 0 && rad) rad[(size_t)ray * n_pts + j] = I;
#pragma unroll
    for (int q = 0; q < NP; ++q) {
      const int p = slot_par[rb * NP + q];
      if (p >= 0) jac[((size_t)ray * n_par + p) * n_pts + j] = J[q];
    }
  }
}
