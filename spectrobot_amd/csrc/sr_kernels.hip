// sr_kernels.hip -- the coefficient op's HIP kernels for gfx950 (MI355X): prep, near field, far field and the
// multi-channel pass, with their launchers.  The limb kernels are sr_limb.hip's (the state kernel's instances:
// sr_limb_state_*.hip, sr_limb_many.hip), the small operators sr_ops.hip's, the solar source sr_solar_source.hip's.
//
//   sr_prep_kernel      one thread per (line, layer): widths, G coefficients,
//                       level-population weights, Humlicek region boundaries
//                       -> FastRec / ColdRec tables in HBM.
//   coefficient spectra, gather formulation (no global atomics, no [n_lines x 13010]
//   matrix, coalesced fp64 stores; fp64 VALU bound):
//     default  far region-1 wings as per-box Taylor sums (local expansions), built from box pairs:
//                sr_s2m_kernel / sr_m2m_kernel   multipole moments of the lines of each source box, all levels
//                sr_m2l_kernel                   moments -> local coefficients (fp64 MFMA: the one matrix product here)
//                sr_farfield_kernel<., true>     per-line expansions of the (line, box) pairs no box pair covers
//              (sr_set_far_field(1): sr_farfield_kernel<., false>, one expansion per (line, box) at every level)
//              sr_abscoeff_near_wings_kernel  exact region 1 of the near lines + one polynomial per level and point
//              sr_abscoeff_near_zones_kernel  regions 2/3/4 through an LDS image of the group
//     exact    sr_abscoeff_wings_kernel / sr_abscoeff_cores_kernel: every evaluation
#include <climits>
#include <cstdlib>

#include "sr_device.hpp"
#include "sr_kernels.hpp"

namespace sr {

// ------------------------------------------------------------------------
// prep: spect_classes.py:174-206 (MakeShapeLine), 312-343 (Calc_Gcoeffs),
//       spect_main_module.py:2049-2080 (population weights), lineshape.f:443-490
// ------------------------------------------------------------------------
// The three G coefficients of line ln at temperature Tw (spect_classes.py:326-337, 1806-1853): 0 where A, g_up or g_lo
// is 0 (:332-341).  lin: linearised about Tw and continued by dTl (sr_lineset_set_linear_weights, see line_physics).
struct LineG {
  double sp, in, ab;
};
__device__ __forceinline__ LineG line_gcoeffs(const LinesDev &L, int ln, double Tw, bool lin, double dTl) {
  auto ex = [](double u) { return exp_bounded(fmin(fmax(u, -700.0), 700.0)); };
  LineG G{0., 0., 0.};
  const double x0 = L.freq[ln];
  const double a_co = L.a_coeff[ln], gu = L.g_up[ln], gl = L.g_lo[ln];
  if (a_co != 0.0 && gl != 0.0 && gu != 0.0) {
    const double four_pi = 4 * kPi;
    const double el = L.e_lower[ln];
    const double eps_up = el + x0 - L.evib_up[ln], eps_lo = el - L.evib_lo[ln];
    // (one division by Tw, one by 4 pi and, in line_physics, one by fac per record, multiplications after that: an IEEE
    // fp64 division is ~13 instructions and this kernel had nine per record; the weights move by an ulp or two.  The
    // widths keep their divisions: dw' places the region boundaries by index.)
    const double inv_Tw = 1.0 / Tw;
    double rot_up = gu * ex(-kC2 * eps_up * inv_Tw);
    double rot_lo = gl * ex(-kC2 * eps_lo * inv_Tw);
    if (lin) { // d ln(exp(-c2 eps / T) / sqrt(T)) / d T = c2 eps / T^2 - 1 / (2 T)   (fac ~ dw ~ sqrt(T))
      rot_up *= fma(dTl, fma(kC2 * eps_up, 1.0 / (Tw * Tw), -0.5 / Tw), 1.0);
      rot_lo *= fma(dTl, fma(kC2 * eps_lo, 1.0 / (Tw * Tw), -0.5 / Tw), 1.0);
    }
    const double hcf = L.hcf[ln];
    const double inv_four_pi = 1.0 / four_pi; // (a compile-time constant)
    G.sp = hcf * rot_up * a_co * inv_four_pi;
    G.in = hcf * rot_up * L.b21[ln] * inv_four_pi;
    G.ab = hcf * rot_lo * L.b12[ln] * inv_four_pi;
  }
  return G;
}

// CalcStrength_from_Strength (spect_classes.py:256-289) of one line: S(T) of CalcStrength_at_T (:1713-1733) from the
// intensity s_ref at t_ref, with qrat = Q(t_ref) / Q(T); s_ab = S alpha_nlte(nu, T, r_lo, r_up) (:1485-1488),
// s_em = S r_up BB_erg(T, nu) with BB_erg's own constants (:2097-2107: rc1 = 1.1904e-5, rhck = 1.4388 -- not c1 = 2 h c^2
// and c2, which puts s_em 0.05-0.2 % below the Einstein source's, as in the reference).
struct LineS {
  double ab, em;
};
__device__ inline LineS hitran_strength(double s_ref, double nu, double e_low, double T, double t_ref, double qrat,
                                        double r_lo, double r_up) {
  auto ex = [](double u) { return exp_bounded(fmin(fmax(u, -700.0), 700.0)); };
  const double gm = ex(-kC2 * nu / T); // Boltz_ratio_nodeg(Freq, Temp)
  const double S = s_ref * qrat * (ex(-kC2 * e_low / T) / ex(-kC2 * e_low / t_ref)) * ((1.0 - gm) / (1.0 - ex(-kC2 * nu / t_ref)));
  const double alpha = r_lo * (1.0 - gm * r_up / r_lo) / (1.0 - gm);
  const double bb = 1.1904e-5 * (nu * nu * nu) / (ex(nu * 1.4388 / T) - 1.0);
  return LineS{S * alpha, S * r_up * bb};
}

// Widths, normalisation and the two output weights of line ln in layer k.
//   lw, dw' (= dw / sqrt(ln2)), fac        spect_classes.py:1972, 1984, 1997-1999
//   G coefficients                         spect_classes.py:326-337, 1806-1853
//   weights by W.mode (sr_kernels.hpp: WeightMode), already divided by fac (shape = y / fac, :2003)
struct LinePhys {
  double lw, dwp, wabs, wemi;
  double w3; // kWeightChannels only: the third weight (0 otherwise)
};
// sr_lineset_set_line_shape (include/spectrobot_hip.h): what multiplies (296/T)^n in the Lorentz width of line ln in
// layer k, gamma_air (P - Ps) + gamma_self Ps (spcl:1972 with its Self_broad / Self_pres_atm passed), and the centre
// that positions the shape, x0' = Freq + P_shift P (spcl:187).  Unset data: the expressions as they always were.
__device__ __forceinline__ double line_gamma_p(const LinesDev &L, const LayersDev &A, int ln, int k) {
  if (L.self_broad) {
    const double ps = A.ps_atm[k];
    return L.air_broad[ln] * (A.p_atm[k] - ps) + L.self_broad[ln] * ps;
  }
  return L.air_broad[ln] * A.p_atm[k];
}
__device__ __forceinline__ double line_centre(const LinesDev &L, const LayersDev &A, int ln, int k) {
  const double x0 = L.freq[ln];
  return L.p_shift ? x0 + L.p_shift[ln] * A.p_atm[k] : x0;
}
__device__ inline LinePhys line_physics(const LinesDev &L, const LayersDev &A, const WeightMode W, int ln, int k) {
  LinePhys P;
  const double T = A.temps[k];
  const double x0 = L.freq[ln];
  // exp_bounded: the library routine without its special cases (|argument| clamped to 700: e^-700 = 1e-304 is as good
  // as the 0 the reference's exp underflows to much later); three of them were 12 % of this kernel's instructions
  auto ex = [](double u) { return exp_bounded(fmin(fmax(u, -700.0), 700.0)); };
  P.lw = ex(L.t_dep[ln] * A.ltrat[k]) * line_gamma_p(L, A, ln, k); // (296/T)^n gamma P  (spcl:1972)
  const double dw = x0 / kCcgs * A.sqk[k];
  P.dwp = dw / A.sqrt_ln2;
  // Linearised weights (sr_lineset_set_linear_weights, with frozen boundaries): the G coefficients and the
  // normalisation are taken at the BOUNDARY temperature Tb and continued to the call's T by their first-order Taylor
  // term, w(Tb) (1 + (T - Tb) d ln w / d T): a difference quotient (c_lin(Tb + dT) - c(Tb)) / dT then carries no
  // curvature of the Boltzmann factors (c2 eps / T^2 ~ 0.1 / K: the truncation that held its step to 0.002 K, where the
  // reference's single-precision staircase is 1e-7 |c| / dT) and the step can be 25 times larger.  Widths and
  // running x above follow the call's own T as always.
  const bool lin = A.frozen && A.linear_w;
  const double Tw = lin ? A.temps_b[k] : T;
  const double fac = (lin ? x0 / kCcgs * A.sqk_b[k] : dw) * A.sqrt_pi_ln2;
  const double dTl = T - Tw;
  const LineG G = line_gcoeffs(L, ln, Tw, lin, dTl);
  const double g_sp = G.sp, g_in = G.in, g_ab = G.ab;
  const int lu = L.lev_up[ln], ll = L.lev_lo[ln];
  const double *pop = A.pop + (size_t)k * A.n_pop;
  double wabs, wemi;
  P.w3 = 0.0;
  if (W.mode == kWeightFolded) { // spect_main_module.py:2073-2080 folded per line
    const double pu = pop[lu], pl = pop[ll];
    wabs = pl * g_ab - pu * g_in;
    wemi = pu * g_sp;
  } else if (W.mode == kWeightGabsGsp) { // BuildCoeff of level W.level: absorption | sp_emission (spcl:1304-1313)
    wabs = (W.level < 0 || ll == W.level) ? g_ab : 0.0; // level < 0: every line (the 'all' LutSet of an LTE table)
    wemi = (W.level < 0 || lu == W.level) ? g_sp : 0.0;
  } else if (W.mode == kWeightGind) {    // ... ind_emission | nothing
    wabs = (W.level < 0 || lu == W.level) ? g_in : 0.0;
    wemi = 0.0;
  } else if (W.mode == kWeightChannels) { // the multi-channel pass: the line's three G coefficients, each to its own channel
    wabs = g_ab;                           // -> the absorption spectrum of the line's LOWER level
    wemi = g_sp;                           // -> the sp_emission spectrum of its UPPER level
    P.w3 = (W.level == 0 ? -g_in : g_in) / fac; // -> ind_emission of its UPPER level (level 0: subtracted from that level's absorption spectrum, smm:2078)
  } else if (W.mode == kWeightLevelPair) { // what pop_level multiplies in the combine loop (smm:2078-2080)
    const bool all = W.level < 0;          // no level table: the 'all' set (smm:2052-2057)
    wabs = ((all || ll == W.level) ? g_ab : 0.0) - ((all || lu == W.level) ? g_in : 0.0);
    wemi = (all || lu == W.level) ? g_sp : 0.0;
  } else if (W.mode == kWeightStrength) { // the HITRAN intensities' s_ab, s_em per molecule of the isotopologue
    const double *rv = A.rvib + (size_t)k * A.n_pop;
    const LineS S = hitran_strength(L.s_ref[ln], x0, L.e_lower[ln], T, W.t_ref, A.qrat[k], rv[ll], rv[lu]);
    wabs = S.ab * W.inv_iso_ab;
    wemi = S.em * W.inv_iso_ab;
  } else {                               // kWeightTracked: one level's share of abs / emi (smm:2083-2087)
    const double pu = pop[lu], pl = pop[ll];
    wabs = (ll == W.level ? pl * g_ab : 0.0) - (lu == W.level ? pu * g_in : 0.0);
    wemi = lu == W.level ? pu * g_sp : 0.0;
  }
  const double inv_fac = 1.0 / fac;
  P.wabs = wabs * inv_fac;
  P.wemi = wemi * inv_fac;
  return P;
}

constexpr int kPrepBlock = 64; // one wave per block: a four-wave block with 20 KB of LDS never found room beside the zones
                               // kernel (16 one-wave blocks of 10 KB fill a CU's LDS; a retiring wave frees ONE slot)
                               // or the wings kernel, and the next call's preparation ran after them instead of beside
// (the body apart from its kernel: sr_prep_batch_kernel runs it for every sparse far-only pass of a multi-channel
// table build in one launch; bx, k: the block's line chunk and layer)
__device__ __forceinline__ void prep_body(const LinesDev &L, const LayersDev &A, const GridParams &gp, const WeightMode W,
                                          int line_lo, int n_sub, int cold_lo, int cold_hi, FastRec *__restrict__ fast,
                                          ColdRec *__restrict__ cold, const int bx, const int k) {
  // records leave through LDS: stored from the registers, a lane's 80 / 128 B record goes out in 16-byte pieces at
  // a 80 / 128 B stride across the lanes; the wave's 64 records are contiguous in the table, so they are transposed
  // and stored 1 KB of consecutive bytes per instruction instead (the kernel writes its 1.63 GB at 5.2 TB/s).
  __shared__ uint4 s_rec[kPrepBlock / 64][64 * sizeof(FastRec) / 16]; // per wave: 64 fast records, then its 64 cold records
  static_assert(sizeof(ColdRec) <= sizeof(FastRec), "the cold records share the fast records' staging buffer");
  const int i0 = bx * blockDim.x + threadIdx.x;
  // (k = blockIdx.y; layers on the fast grid axis instead -- the line arrays then stay in L2 -- measured slower: 0.32 vs 0.29 ms, the record rows of consecutive blocks lie 8 MB apart)
  const int wave_first = i0 - (threadIdx.x & 63);
  if (wave_first >= n_sub) return; // whole wave out of range
  const bool valid = i0 < n_sub;
  const int i = valid ? i0 : n_sub - 1;
  const int ln = line_lo + i;
  const double freq = L.freq[ln];
  const double x0 = line_centre(L, A, ln, k); // positions the shape; the Doppler width and the weights keep Freq
  const LinePhys ph = line_physics(L, A, W, ln, k);
  const double lw = ph.lw, dwp = ph.dwp;

  const int ic = L.ic[ln];
  WinX xf{gp.lin_start, gp.lin_delta, grid_at(gp, ic)};
  Bounds B = humliv_bounds(xf, kImxsig, x0, lw, dwp), B0 = B;
  double dwp0 = dwp;
  if (A.frozen) {
    // sr_lineset_set_bounds_temps: the region boundaries (indices) as at the layer's boundary temperature, every
    // width and running x at the call's own -- c(T + dT) and c(T) then share their seams
    const double lw_b = exp_bounded(fmin(fmax(L.t_dep[ln] * A.ltrat_b[k], -700.0), 700.0)) * line_gamma_p(L, A, ln, k);
    dwp0 = freq / kCcgs * A.sqk_b[k] / A.sqrt_ln2;
    B0 = humliv_bounds(xf, kImxsig, x0, lw_b, dwp0);
    B.il = B0.il; B.ir = B0.ir; B.il2 = B0.il2; B.ir2 = B0.ir2;
    B.xr = div_with(xf(B.ir) - x0, dwp, B.inv_dwp); // lineshape.f:471 at the frozen ir
  }

  FastRec r;
  r.xl = B.xl;
  r.xr = B.xr;
  r.xstep = B.xstep;
  r1_set(r, B.ry);
  r.w3 = ph.w3;
  r.wabs = ph.wabs;
  r.wemi = ph.wemi;
  r.j1 = ic - kHalf;
  r.ilir = (uint32_t)B.il | ((uint32_t)B.ir << 16);
  {
    const int lane = threadIdx.x & 63, n_valid = min(64, n_sub - wave_first);
    uint4 *buf = s_rec[threadIdx.x >> 6];
    const size_t o = (size_t)k * n_sub + wave_first;
    constexpr int NF = sizeof(FastRec) / 16, NC = sizeof(ColdRec) / 16;
    const uint4 *rp = reinterpret_cast<const uint4 *>(&r);
#pragma unroll
    for (int q = 0; q < NF; ++q) buf[lane * NF + q] = rp[q];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    uint4 *gf = reinterpret_cast<uint4 *>(fast + o);
#pragma unroll
    for (int q = 0; q < NF; ++q)
      if (q * 64 + lane < n_valid * NF) gf[q * 64 + lane] = buf[q * 64 + lane];
    __builtin_amdgcn_wave_barrier();
    // The cold record (regions 2-4) is read only for lines whose zone meets [cold_lo, cold_hi]: in
    // far-field mode that is the shard, so the halo lines of a multi-GPU shard (half of its lines
    // at 8 GPUs) skip its computation and its 48 B; exact mode reads it for window ends too and
    // passes the whole index range.
    const int zl = r.j1 + B.il - 1, zh = r.j1 + B.ir - 1;
    if (__any(valid && zl <= cold_hi && zh >= cold_lo)) {
      ColdRec c = make_cold(B0, dwp0, x0, xf); // il2 | ir2 and the region-3 interval (at the boundary temperature)
      if (A.frozen) {
        c.ry = B.ry;
        c.dwp = dwp;
        c.xs2l = div_with(x0 - xf(B.il), dwp, B.inv_dwp);  // lineshape.f:504
        c.xs2r = div_with(xf(B.ir2) - x0, dwp, B.inv_dwp); // :514
      }
      const uint4 *cp = reinterpret_cast<const uint4 *>(&c);
      uint4 *gc = reinterpret_cast<uint4 *>(cold + o);
      // staged like the fast records: 64 x 48 bytes, consecutive in the table, 1 KB per store instruction
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int q = 0; q < NC; ++q) buf[lane * NC + q] = cp[q];
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int q = 0; q < NC; ++q)
        if (q * 64 + lane < n_valid * NC) gc[q * 64 + lane] = buf[q * 64 + lane];
    }
  }
  // (The widest zone of the layer, which the other kernels use to bound their candidate ranges, comes from the host
  // as a bound -- (lw_max + 15 dw'_max) / step: the wave maxima + one atomicMax per wave on the layer's single counter
  // serialised in L2 and WERE this kernel's 0.8 ms: it took as long with its stores or its arithmetic compiled out.)
}
__global__ __launch_bounds__(kPrepBlock) void sr_prep_kernel(LinesDev L, LayersDev A, GridParams gp, WeightMode W,
                                                      int line_lo, int n_sub, int cold_lo, int cold_hi,
                                                      FastRec *__restrict__ fast,
                                                      ColdRec *__restrict__ cold) {
  prep_body(L, A, gp, W, line_lo, n_sub, cold_lo, cold_hi, fast, cold, (int)blockIdx.x, (int)blockIdx.y);
}
// The tables of ALL sparse far-only passes of a table build (FarBatchItem) in one launch: grid (line chunks of the
// largest item, layers, items); fast records only (an empty cold range).
__global__ __launch_bounds__(kPrepBlock) void sr_prep_batch_kernel(const FarBatchItem *__restrict__ items, LayersDev A, GridParams gp) {
  const FarBatchItem it = items[blockIdx.z];
  prep_body(it.L, A, gp, it.W, it.line_lo, it.n_sub, INT_MAX / 2, INT_MIN / 2, it.fast, nullptr, (int)blockIdx.x, (int)blockIdx.y);
}

// ------------------------------------------------------------------------
// Lines whose centre lies outside their own 13010-point window (farther than ~3.25 cm-1 from the
// grid): closest_grid puts their window on the first / last grid point (spect_classes.py:1941) and
// humliv_bb takes one of its two sequential outer branches; the part of the window inside the grid
// is added to the spectrum like any other line (spect_classes.py:1113-1120).  They are few: one
// thread per (line, layer) walks the Fortran's control flow for the segment bounds, then one thread
// per (grid point, layer) adds the lines in list order (gather: deterministic, no atomics).
// ------------------------------------------------------------------------
__global__ __launch_bounds__(64) void sr_outer_prep_kernel(LinesDev L, int n_out, LayersDev A, GridParams gp,
                                                           WeightMode W, OuterRec *__restrict__ recs) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x, k = blockIdx.y;
  if (i >= n_out) return;
  const LinePhys ph = line_physics(L, A, W, i, k);
  const double x0 = line_centre(L, A, i, k), dw = ph.dwp;
  const int ic = L.ic[i], n = kImxsig;
  const WinX xf{gp.lin_start, gp.lin_delta, grid_at(gp, ic)};
  OuterRec r;
  r.ry = ph.lw / dw;                        // lineshape.f:261
  r.ryf = (double)(float)r.ry;
  r.xstep = (xf(2) - xf(1)) / dw;           // :265-266
  region1_coef(r.ry, r.a, r.b, r.c, r.d);
  region2_coef(r.ry, r.q2);
  r.wabs = ph.wabs;
  r.wemi = ph.wemi;
  r.j1 = ic - kHalf;
  r.c_lo = r.r2_lo = r.r1_lo = 1;
  r.c_hi = r.r2_hi = r.r1_hi = 0;
  r.c_ref = 1;
  r.x_core = r.x_r2 = r.x_r1 = 0.0;
  const double ry = r.ry, xstep = r.xstep;
  if (x0 <= xf(1)) {                        // :272-357
    r.dir = 1;
    int j = 1;
    double rx = (xf(j) - x0) / dw;
    r.x_core = rx;
    while ((rx + ry < 5.5) && (j <= n)) { j = j + 1; rx = rx + xstep; }
    r.c_lo = 1; r.c_hi = j - 1; r.c_ref = 1;
    if (j <= n) {
      int l = max((int)round((15.0 - ry - rx) / xstep), 0) + j;
      l = min(l, n);
      if (l > j) {
        r.r2_lo = j; r.r2_hi = l;
        r.x_r2 = (xf(j) - x0) / dw;
        l = l + 1;
      }
      if (l < j) l = j;
      if (l < n) {
        r.r1_lo = l; r.r1_hi = n;
        r.x_r1 = (xf(l) - x0) / dw;
      }
    }
  } else {                                  // x0 >= x(i2), :358-442
    r.dir = -1;
    int j = n;
    double rx = (x0 - xf(j)) / dw;
    r.x_core = rx;
    while ((rx + ry < 5.5) && (j >= 1)) { j = j - 1; rx = rx + xstep; }
    r.c_lo = j + 1; r.c_hi = n; r.c_ref = n;
    if (j >= 1) {
      int l = j - max((int)round((15.0 - ry - rx) / dw / xstep), 0); // sic, :404
      l = max(l, 1);
      if (l == n) l = n + 1;
      if (l < j) {
        r.r2_lo = l; r.r2_hi = j;
        r.x_r2 = (x0 - xf(l)) / dw;
      }
      if (l >= 1) {
        r.r1_lo = 1; r.r1_hi = l - 1;
        r.x_r1 = (x0 - xf(1)) / dw;
      }
    }
  }
  recs[(size_t)k * n_out + i] = r;
}

__global__ __launch_bounds__(256) void sr_outer_add_kernel(const OuterRec *__restrict__ recs, int n_out, int p_lo,
                                                           int p_hi, int g_lo, int g_hi,
                                                           double *__restrict__ abs_out,
                                                           double *__restrict__ emi_out) {
  const int j = p_lo + blockIdx.x * blockDim.x + threadIdx.x, layer = blockIdx.y;
  if (j >= p_hi) return;
  const OuterRec *row = recs + (size_t)layer * n_out;
  double acc_a = 0., acc_e = 0.;
  for (int i = 0; i < n_out; ++i) {
    const OuterRec &r = row[i]; // wave-uniform address
    const int k = j - r.j1 + 1;
    if (k < 1 || k > kImxsig) continue;
    const double s = (double)r.dir;
    double y;
    // the Fortran writes core, region 2, region 1 in this order over disjoint index ranges
    if (k >= r.c_lo && k <= r.c_hi) {
      y = core_point(fma(s * (double)(k - r.c_ref), r.xstep, r.x_core), r.ry, r.ryf);
    } else if (k >= r.r2_lo && k <= r.r2_hi) {
      y = region2_val(r.q2, fma(s * (double)(k - r.r2_lo), r.xstep, r.x_r2));
    } else if (k >= r.r1_lo && k <= r.r1_hi) {
      const double x = fma(s * (double)(k - r.r1_lo), r.xstep, r.x_r1);
      const double x2 = x * x;
      y = fma(x2, r.b, r.a) * fast_rcp<2>(fma(x2, fma(x2, 4.0, r.d), r.c));
    } else {
      continue;
    }
    acc_a = fma(r.wabs, y, acc_a);
    acc_e = fma(r.wemi, y, acc_e);
  }
  const size_t o = (size_t)layer * (size_t)(g_hi - g_lo) + (size_t)(j - g_lo);
  abs_out[o] += acc_a;
  emi_out[o] += acc_e;
}

int launch_outer(const LinesDev &Lo, int n_out, const LayersDev &A, const GridParams &gp, const WeightMode &W,
                 OuterRec *recs, int g_lo, int g_hi, double *abs_out, double *emi_out, hipStream_t st) {
  if (n_out <= 0 || A.n_layers <= 0 || g_hi <= g_lo) return 0;
  // their windows sit on the first / last grid point: only points within half a window of a grid end
  const int ranges[2][2] = {{max(g_lo, 0), min(g_hi, kHalf)}, {max(g_lo, max(gp.n_grid - 1 - kHalf, kHalf)), g_hi}};
  if (ranges[0][0] >= ranges[0][1] && ranges[1][0] >= ranges[1][1]) return 0;
  hipLaunchKernelGGL(sr_outer_prep_kernel, dim3((n_out + 63) / 64, A.n_layers), dim3(64), 0, st, Lo, n_out, A, gp, W,
                     recs);
  for (int q = 0; q < 2; ++q) {
    const int lo = ranges[q][0], hi = ranges[q][1];
    if (lo >= hi) continue;
    hipLaunchKernelGGL(sr_outer_add_kernel, dim3((hi - lo + 255) / 256, A.n_layers), dim3(256), 0, st, recs, n_out,
                       lo, hi, g_lo, g_hi, abs_out, emi_out);
  }
  return (int)hipGetLastError();
}

// ------------------------------------------------------------------------
// Line strengths (sr_line_strengths_dev): one thread per (input line, layer), stored in input order -- consecutive
// threads, consecutive outputs.  inpos[i]: main-list position p >= 0, outer-list position -2 - p, or -1 for a line the
// lineset's filter dropped (0).
//   source 0: CalcStrength_from_Einstein (spect_classes.py:219-254) times iso_ab, from the G coefficients and the
//             populations b(E_L, Tvib_L) / Q(T) the coefficient op uses
//   source 1: CalcStrength_from_Strength (:256-289), hitran_strength
// ------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sr_line_strengths_kernel(LinesDev L, LinesDev Lo, const int *__restrict__ inpos,
                                                                int n_in, LayersDev A, int source, double iso_ab,
                                                                double t_ref, double *__restrict__ s_ab,
                                                                double *__restrict__ s_em) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x, k = blockIdx.y;
  if (i >= n_in) return;
  const int p = inpos[i];
  double ab = 0.0, em = 0.0;
  if (p != -1) {
    const LinesDev &M = p >= 0 ? L : Lo;
    const int ln = p >= 0 ? p : -2 - p;
    const int lu = M.lev_up[ln], ll = M.lev_lo[ln];
    const double T = A.temps[k];
    if (source == 0) {
      const double *pop = A.pop + (size_t)k * A.n_pop;
      const LineG G = line_gcoeffs(M, ln, T, false, 0.0);
      ab = iso_ab * (pop[ll] * G.ab - pop[lu] * G.in);
      em = iso_ab * (pop[lu] * G.sp);
    } else {
      const double *rv = A.rvib + (size_t)k * A.n_pop;
      const LineS S = hitran_strength(M.s_ref[ln], M.freq[ln], M.e_lower[ln], T, t_ref, A.qrat[k], rv[ll], rv[lu]);
      ab = S.ab;
      em = S.em;
    }
  }
  const size_t o = (size_t)k * (size_t)n_in + (size_t)i;
  s_ab[o] = ab;
  if (s_em) s_em[o] = em;
}

int launch_line_strengths(const LinesDev &L, const LinesDev &Lo, const int *inpos, int n_in, const LayersDev &A,
                          int source, double iso_ab, double t_ref, double *s_ab, double *s_em, hipStream_t st) {
  if (n_in <= 0 || A.n_layers <= 0) return 0;
  hipLaunchKernelGGL(sr_line_strengths_kernel, dim3((n_in + 255) / 256, A.n_layers), dim3(256), 0, st, L, Lo, inpos,
                     n_in, A, source, iso_ab, t_ref, s_ab, s_em);
  return (int)hipGetLastError();
}

// ------------------------------------------------------------------------
// coefficient kernels (gather formulation)
//
// One wavefront owns WP = 64*P consecutive grid points of one layer ("wave
// tile") and walks the nu-sorted lines whose 13010-point windows touch it.
// Everything per line is wave-uniform and lives in SGPRs (records are read with
// scalar loads); every lane accumulates abs/emi for its own P points (stride
// 64, so each slot p is 64 consecutive points and stores are coalesced).
//
//   sr_abscoeff_wings_kernel  (line, group of 256 points) pairs for which the
//       WHOLE group lies in one region-1 wing and inside the window (98 % of all
//       evaluations): x = x_b + lane_p*xstep, (a + x^2 b)/(c + x^2 (d + 4 x^2)),
//       one reciprocal shared by the group's four slots, no branches in the body.
//   sr_abscoeff_cores_kernel  the remaining (line, group) pairs -- group meets
//       the line's region-2/3/4 zone or a window end -- evaluated slot by slot
//       with the general, region-by-index code; adds into the wings' output.
// Both apply the same classify() to the same groups, so every (line, point) is
// counted exactly once.
// ------------------------------------------------------------------------
// first line (index into the shard's record table) whose window centre is >= v
__device__ inline int lower_bound_ic(const IcIndex &ix, int v) {
  const int g = ix.first[min(max(v - ix.x0, 0), ix.n_tab - 1)];
  return min(max(g - ix.line_lo, 0), ix.n_sub);
}

// XCD-aware bijective remap (8 XCDs, blocks dealt round-robin): blocks that
// share an XCD get consecutive work ids, so neighbouring tiles of one layer --
// which read almost the same records -- hit the same L2.
__device__ inline int xcd_remap(int b, int nb) {
  const int q = nb >> 3, r = nb & 7, x = b & 7, i = b >> 3;
  return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + i;
}

// ... for kernels whose work ids differ in COST along the id axis (the per-line far-field kernels: widest level first,
// a top-level box holds ten times the candidates of a level-0 box): xcd_remap hands every XCD one contiguous eighth of
// the ids -- the first XCD all the wide boxes -- and the others wait for it (CUs idle 29 % of the sparse passes' kernel:
// SQ_BUSY_CU_CYCLES).  Here the ids are dealt in groups of G consecutive ones, round-robin over the XCDs: neighbours
// still share an L2, every XCD gets every level.  Bijective on [0, nb).
__device__ inline int xcd_remap_groups(int b, int nb, int G) {
  const int full = nb / (8 * G) * (8 * G);
  if (b >= full) return b;
  const int x = b & 7, i = b >> 3;
  return ((i / G) * 8 + x) * G + i % G;
}

// Executed-work counters (counting instantiations only): sum a per-lane count over the wave, one
// atomic per wave and counter.
__device__ inline void count_add(unsigned long long *cnt, int which, unsigned per_lane, int lane) {
  unsigned v = per_lane;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  if (lane == 0 && v) atomicAdd(&cnt[which], (unsigned long long)v);
}

// 1: every point of [lo, hi] is strictly left of il (region 1, running x from
// k = 1) and inside the window; 2: strictly right of ir; 0: anything else.
__device__ inline int classify(int j1, int il, int ir, int lo, int hi) {
  if (lo >= j1 && hi < j1 + il - 1) return 1;
  if (lo > j1 + ir - 1 && hi <= j1 + (kImxsig - 1)) return 2;
  return 0;
}
// -x (left) or x (right) at grid index `at`: only x^2 is used.
__device__ inline double wing_x_at(const FastRec &r, int cls, int j1, int at) {
  return cls == 1 ? fma((double)(at - j1), r.xstep, -r.xl)
                  : fma((double)(at - (j1 + r.ir() - 1)), r.xstep, r.xr);
}

// Region 1 at four points per lane (x = xb + fl[i]*xs) with ONE reciprocal:
// 1/(d0 d1 d2 d3) by v_rcp_f64 (2^-24) + one Newton step (2e-15), unfolded by
// multiplications.  den >= 4*15^4 and <= ~1e19 here, so the product of four
// cannot leave the fp64 range.
__device__ inline void wing_eval4(const double xb, const double xs, const double a, const double b,
                                  const double c, const double d, const double wa, const double we,
                                  const double *fl, double *acc_a, double *acc_e) {
  double num[4], den[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const double x = fma(fl[i], xs, xb);
    const double x2 = x * x;
    num[i] = fma(x2, b, a);
    den[i] = fma(x2, fma(x2, 4.0, d), c);
  }
  const double d01 = den[0] * den[1], d23 = den[2] * den[3];
  const double r = fast_rcp<1>(d01 * d23);
  const double r01 = r * d23, r23 = r * d01;
  const double q0 = (num[0] * den[1]) * r01, q1 = (num[1] * den[0]) * r01;
  const double q2 = (num[2] * den[3]) * r23, q3 = (num[3] * den[2]) * r23;
  acc_a[0] = fma(wa, q0, acc_a[0]); acc_e[0] = fma(we, q0, acc_e[0]);
  acc_a[1] = fma(wa, q1, acc_a[1]); acc_e[1] = fma(we, q1, acc_e[1]);
  acc_a[2] = fma(wa, q2, acc_a[2]); acc_e[2] = fma(we, q2, acc_e[2]);
  acc_a[3] = fma(wa, q3, acc_a[3]); acc_e[3] = fma(we, q3, acc_e[3]);
}

constexpr int kGroup = 256; // points per ownership group: 4 slots of 64 (one shared reciprocal)

template <int P>
__global__ __launch_bounds__(64) void sr_abscoeff_wings_kernel(
    const FastRec *__restrict__ fast,
    IcIndex ix, // index into the sorted window centres of the prepped lines
    int n_sub, int n_tiles, int g_lo, int g_hi, double *__restrict__ abs_out,
    double *__restrict__ emi_out) {
  static_assert(P % 4 == 0, "P must be a multiple of 4");
  constexpr int WP = 64 * P, NG = P / 4;
  const int wg = xcd_remap(blockIdx.x, gridDim.x);
  const int layer = wg / n_tiles, tile = wg - layer * n_tiles;
  const int wlo = g_lo + tile * WP;
  const int whi = min(wlo + WP, g_hi) - 1;
  const int lane = threadIdx.x;

  // lines whose window [ic-6505, ic+6504] meets [wlo, whi]
  const int l0 = lower_bound_ic(ix, wlo - (kHalf - 1));
  const int l1 = lower_bound_ic(ix, whi + kHalf + 1);

  double acc_a[P], acc_e[P], fl[4];
#pragma unroll
  for (int p = 0; p < P; ++p) acc_a[p] = acc_e[p] = 0.;
#pragma unroll
  for (int i = 0; i < 4; ++i) fl[i] = (double)(lane + 64 * i);
  const FastRec *frow = fast + (size_t)layer * n_sub;
  FastRec nxt = frow[l0 < l1 ? l0 : 0];
  for (int l = l0; l < l1; ++l) {
    // wave-uniform address: two scalar loads; the next record is fetched while this
    // one is evaluated (the table has one record of slack behind its end)
    const FastRec r = nxt;
    nxt = frow[l + 1];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      const int glo = wlo + kGroup * g, ghi = min(glo + kGroup - 1, whi);
      const int cls = glo <= whi ? classify(r.j1, r.il(), r.ir(), glo, ghi) : 0;
      if (cls == 0) continue; // left to sr_abscoeff_cores_kernel (or outside the window)
      const double xb = wing_x_at(r, cls, r.j1, glo);
      const R1Coef rq = r1_of(r);
      wing_eval4(xb, r.xstep, rq.a, rq.b, rq.c, rq.d, r.wabs, r.wemi, fl, acc_a + 4 * g, acc_e + 4 * g);
    }
  }
  const size_t row = (size_t)layer * (size_t)(g_hi - g_lo);
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const int j = wlo + lane + 64 * p;
    if (j <= whi) {
      abs_out[row + (j - g_lo)] = acc_a[p];
      emi_out[row + (j - g_lo)] = acc_e[p];
    }
  }
}

// One wave per group of 256 points: the (line, group) pairs the wings kernel skips.
__global__ __launch_bounds__(64) void sr_abscoeff_cores_kernel(
    const FastRec *__restrict__ fast, const ColdRec *__restrict__ cold,
    IcIndex ix, const int *__restrict__ zmax, // [n_layers] max zone half-width
    int n_sub, int n_groups, int g_lo, int g_hi, GridParams gp, double *__restrict__ abs_out,
    double *__restrict__ emi_out) {
  const int wg = xcd_remap(blockIdx.x, gridDim.x);
  const int layer = wg / n_groups, grp = wg - layer * n_groups;
  const int wlo = g_lo + grp * kGroup;
  const int whi = min(wlo + kGroup, g_hi) - 1;
  const int lane = threadIdx.x;
  const int zm = min(zmax[layer], kHalf - 1);

  // candidates (as ranges of the sorted centre list), C <= A <= B by start:
  //  C: window END inside the group      ic+6504 in [wlo, whi)
  //  A: region-2/3/4 zone may meet it    ic in [wlo-zm, whi+zm]
  //  B: window START inside the group    ic-6505 in (wlo, whi]
  const int c0 = lower_bound_ic(ix, wlo - (kHalf - 1));
  const int c1 = lower_bound_ic(ix, whi - (kHalf - 1));
  const int a0 = lower_bound_ic(ix, wlo - zm);
  const int a1 = lower_bound_ic(ix, whi + zm + 1);
  const int b0 = lower_bound_ic(ix, wlo + kHalf + 1);
  const int b1 = lower_bound_ic(ix, whi + kHalf + 1);
  int rs[3], re[3];
  rs[0] = c0; re[0] = max(c1, c0);
  rs[1] = max(a0, re[0]); re[1] = max(a1, rs[1]);
  rs[2] = max(b0, re[1]); re[2] = max(b1, rs[2]);

  double acc_a[4], acc_e[4], fl[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    acc_a[p] = 0.;
    acc_e[p] = 0.;
    fl[p] = (double)(lane + 64 * p);
  }
  const FastRec *frow = fast + (size_t)layer * n_sub;
  const ColdRec *crow = cold + (size_t)layer * n_sub;
  for (int rg = 0; rg < 3; ++rg) {
    if (rs[rg] >= re[rg]) continue;
    FastRec nxt = frow[rs[rg]];
    ColdRec cnxt = crow[rs[rg]];
    for (int l = rs[rg]; l < re[rg]; ++l) {
      const FastRec r = nxt;
      const ColdFull cr = expand_cold(cnxt);
      nxt = frow[l + 1]; // one record of slack behind both tables
      cnxt = crow[l + 1];
      const int j1 = r.j1, jN = j1 + (kImxsig - 1);
      if (jN < wlo || j1 > whi) continue;
      if (classify(j1, r.il(), r.ir(), wlo, whi) != 0) continue; // done by the wings kernel
      const WinX xf{gp.lin_start, gp.lin_delta, grid_at(gp, j1 + kHalf)};
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const int slo = wlo + 64 * p, shi = min(slo + 63, whi);
        if (slo > whi || jN < slo || j1 > shi) continue;
        const int scls = classify(j1, r.il(), r.ir(), slo, shi);
        double y;
        if (scls != 0) { // the whole slot in one wing
          const double x = fma(fl[p], r.xstep, wing_x_at(r, scls, j1, wlo));
          const double x2 = x * x;
          const R1Coef rq = r1_of(r);
          y = fma(x2, rq.b, rq.a) * fast_rcp<1>(fma(x2, fma(x2, 4.0, rq.d), rq.c));
        } else {
          const int k = slo + lane - j1 + 1; // 1-based window index
          y = (k >= 1 && k <= kImxsig && slo + lane <= shi) ? humliv_point(k, r, cr, xf) : 0.0;
        }
        acc_a[p] = fma(r.wabs, y, acc_a[p]);
        acc_e[p] = fma(r.wemi, y, acc_e[p]);
      }
    }
  }
  const size_t row = (size_t)layer * (size_t)(g_hi - g_lo);
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int j = wlo + lane + 64 * p;
    if (j <= whi) {
      abs_out[row + (j - g_lo)] += acc_a[p];
      emi_out[row + (j - g_lo)] += acc_e[p];
    }
  }
}

// ------------------------------------------------------------------------
// far field by local (Taylor) expansions
//
// Where a whole box of target points lies in one region-1 wing of a line, inside
// its window and at least kTheta box half-widths from its centre, the line's
// contribution w*(a + x^2 b)/(c + x^2(d + 4x^2)), x affine in the grid index, is
// analytic over the box with convergence ratio <= 1/kTheta: its Taylor
// coefficients in t = (j - centre)/half_width come from a 4-term linear
// recurrence (power-series division of a quadratic by a quartic), the
// coefficients of all such lines are summed per box (lanes = lines), and each
// point evaluates ONE polynomial per level instead of one rational per line.
// Truncation at degree kFD = 19 (kTheta = 4) is <= 18 x 4^-20 = 1.6e-11 of the line's own contribution
// (worst case: nearest admissible line, the box edge AWAY from it; the admissible distance that holds it is
// ff_thr2, sr_kernels.hpp, with its derivation; -DSR_KFD=22: 2.6e-13).  Boxes are nested (width
// 64 << level); a (line, slot) pair is owned by the highest admissible level
// (admissibility is monotone down the hierarchy) or, if none, by the exact
// near-field kernel.  All ownership tests are integer and shared by the kernels.
// ------------------------------------------------------------------------
__device__ inline bool ff_admissible(int j1, int il, int ir, int blo, int bhi, int thr2) {
  if (classify(j1, il, ir, blo, bhi) == 0) return false;
  const int d2 = blo + bhi - 2 * (j1 + kHalf); // twice (box centre - line centre)
  return (d2 < 0 ? -d2 : d2) >= thr2;
}

// Box-pair mode (FarParams::m2l).  Source box s and target box t of level l, both counted in boxes of 64 << l
// points from g_lo, o = t - s: the pair is VALID when every line centred in s sees all of t in one region-1 wing
// inside its window, far enough for the multipole / local pair of expansions: gap between the boxes >= the widest
// zone of the layer (zreq) and >= 2 box widths, more where the poles
// of the layer's lines (pms grid points from their centres) are not small against the box (m2l_separated).
// Validity is monotone down the hierarchy (children of a valid pair are valid), so a pair is TRANSLATED at level
// l iff it is valid there and its parent pair is not, and a level-0 pair is covered by some level iff it is valid
// at level 0.  Valid pairs are admissible for every line of s (ff_admissible at level 0), so the near kernels
// need not know about box pairs at all.
// The separation ratio rho = (h + pole) / (distance of the centres - h), h = W / 2, in hundredths.  What it bounds is the
// MULTIPOLE series, which stops at order kFD: a singularity h + pole from the source centre, seen from the nearest target
// point on the other side of that centre, is sum_m (m + 1) (-rho)^m with the terms m <= kFD - 2 kept; what is dropped is
// (kFD + (kFD - 1) rho) rho^(kFD-1) of the line's own value there -- 1.44e-11 at rho = 0.21 and degree 19 (1.6e-13 at 22),
// to which the local expansion of the target box adds (kFD + 2 + (kFD + 1) r) r^(kFD+1), r = h / (distance of the
// centres - h - pole) <= rho: 7e-13.  (Until the far field was held to one line's own contribution the ratio was 0.27,
// set when the degree was 22 by 0.27^(kFD+1): at degree 19 a Doppler line on the last point of its source box measured
// 1.9e-11 at the nearest point of the first valid target box, tests/test_gpu_farfield_lines.py; 0.21: 6.4e-12, and the
// first valid offset of level 0 is 4 where it was 3 -- headline step 5.055 -> 5.090 ms, +0.7 %, same box, interleaved.)
constexpr int kM2LRatioPct = 21;
constexpr long double m2l_dropped_over_bound() {
  const long double rho = kM2LRatioPct / 100.0L;
  long double mp = 1.0L, lc = 1.0L, bound = 18.0L;
  for (int n = 0; n < kFD - 1; ++n) mp *= rho;
  for (int n = 0; n <= kFD; ++n) { lc *= rho; bound /= kTheta; }
  return ((kFD + (kFD - 1) * rho) * mp + (kFD + 2 + (kFD + 1) * rho) * lc) / bound;
}
static_assert(m2l_dropped_over_bound() <= 1.0L, "the box pairs' separation ratio does not hold the truncation bound at this degree");
__device__ inline bool m2l_separated(int level, int a, int zreq, int pms) { // a = |o|
  const int W = 64 << level;
  // gap >= zone and >= two boxes; (h + pole) <= 0.21 (distance of the centres - h)
  return a >= 3 && (a - 1) * W >= zreq && 100 * (W + 2 * pms) <= kM2LRatioPct * (2 * a - 1) * W;
}
__device__ inline bool m2l_valid(int level, int o, int zreq, int pms) {
  const int W = 64 << level, a = o < 0 ? -o : o;
  if (!m2l_separated(level, a, zreq, pms)) return false;
  // window [ic - kHalf, ic + kHalf - 1] of every centre ic of s holds all of t
  return (a + 1) * W <= (o > 0 ? kHalf : kHalf + 1);
}
// smallest separated |o| of the level (capped: beyond the window nothing is valid anyway)
__device__ inline int m2l_first_offset(int level, int zreq, int pms) {
  int a = 3;
  while (a < 128 && !m2l_separated(level, a, zreq, pms)) ++a;
  return a;
}

// Sum N per-lane values over the 64 lanes: at step M the pairs (i, i + N/2) are split
// between the lanes with bit M clear / set, an unpaired last value takes a plain butterfly.
// Afterwards v[0] of each lane is the total of value lane_reduce_index(lane) (several lanes
// can hold the same one: `primary` picks one of them).
template <int N, int M>
__device__ inline void lane_reduce(double *v, int lane) {
  if constexpr (M >= 1) {
    constexpr int half = N / 2;
    const bool up = (lane & M) != 0;
#pragma unroll
    for (int i = 0; i < half; ++i) {
      const double keep = up ? v[i + half] : v[i];
      const double send = up ? v[i] : v[i + half];
      v[i] = keep + __shfl_xor(send, M);
    }
    if constexpr (N & 1) v[half] = v[2 * half] + __shfl_xor(v[2 * half], M);
    lane_reduce<half + (N & 1), M / 2>(v, lane);
  }
}
template <int N, int M>
__device__ inline int lane_reduce_index(int lane, bool &primary) {
  if constexpr (M == 0) {
    return 0;
  } else {
    constexpr int half = N / 2;
    const int s = lane_reduce_index<half + (N & 1), M / 2>(lane, primary); // slot after this step
    const bool up = (lane & M) != 0;
    if (s < half) return s + (up ? half : 0);
    if (up) primary = false;
    return 2 * half;
  }
}

// COUNT: the instantiation sr_set_counting(1) selects; it adds the number of (line, box) expansions
// this launch performs to cnt[kCntExpansions] (bench.py's executed-work accounting).  The timed
// instantiation carries no counting code.
// (Occupancy unconstrained, 140 VGPRs.  Built for 4 waves per SIMD, with S2M, to fit beside the zones kernel: 48 B of scratch, far-field group 1.07 -> 1.66 ms, step 6.07 vs 5.61 ms.)
template <bool COUNT, bool M2L>
__global__ __launch_bounds__(64) void sr_farfield_kernel(const FastRec *__restrict__ fast,
                                                         IcIndex ix,
                                                         const int *__restrict__ zmax, int n_sub, int g_lo,
                                                         int /*g_hi*/, FarParams fp,
                                                         unsigned long long *__restrict__ cnt) {
  // block -> (layer, level, box).  Layers are taken in groups of ceil(n_layers / 8); xcd_remap
  // gives each XCD a contiguous run of work ids, i.e. (about) one group.  Inside a group: first
  // the two widest levels of ALL its layers (a 1024-point box runs ~100 us; left to the end of
  // the last layer, as in a plain layer-major order, those were the tail of the kernel: 0.36 vs
  // 0.27 ms expected on a 1/8 shard), then layer by layer the narrower levels, widest first, so
  // that the blocks resident on an XCD share one stretch of one layer's record row, which its
  // L2 holds.  On the full grid that locality is worth more than the tail (2.14 ms against 2.66 with
  // the wide levels first, 2.76 fully level-major), so the host asks for it on small shards only.
  const int wid = xcd_remap(blockIdx.x, gridDim.x);
  const int lg = (fp.n_layers + 7) / 8;                       // layers per group
  const int grp = wid / (lg * fp.n_boxes_total);
  const int l_first = grp * lg, l_cnt = min(lg, fp.n_layers - l_first);
  int idx = wid - grp * lg * fp.n_boxes_total;                // within the group
  const int n_top = fp.top_first ? min(2, fp.n_levels - 1) : 0; // levels taken first (small shards only)
  int level = fp.n_levels - 1, layer = -1;
  if (M2L) { // box-pair mode: level 0 only (grid = box_count[0] * n_layers), layer-major
    layer = wid / fp.box_count[0];
    idx = wid - layer * fp.box_count[0];
    level = 0;
  }
  for (int t = 0; t < n_top && layer < 0; ++t, --level) {
    const int cnt = l_cnt * fp.box_count[level];
    if (idx < cnt) {
      layer = l_first + idx / fp.box_count[level];
      idx -= (layer - l_first) * fp.box_count[level];
      ++level; // undo the loop's decrement
    } else {
      idx -= cnt;
    }
  }
  if (layer < 0) { // the narrower levels, layer-major
    int per_layer = 0;
    for (int lv = 0; lv <= level; ++lv) per_layer += fp.box_count[lv];
    layer = l_first + idx / per_layer;
    idx -= (layer - l_first) * per_layer;
    if (fp.top_first) {
      while (level > 0 && idx >= fp.box_count[level]) {
        idx -= fp.box_count[level];
        --level;
      }
    } else {
      // Full grids: inside a layer the boxes of ALL levels are taken super-tile by super-tile (kFarSuper
      // points = 16 top-level boxes).  A level-major sweep over the whole grid touches the layer's whole
      // record row (8 MB for 1e5 lines) once per level -- more than an XCD's 4 MB L2 holds, so every level
      // re-read it from HBM (4.7 GB per step); the records of one super-tile and its window halo
      // ((16384 + 13010) lines x 80 B = 2.3 MB) stay in L2 across the five levels.
      const int top_lv = fp.n_levels - 1;
      const int per_super = (kFarSuper >> 6) * 2 - (kFarSuper >> (6 + top_lv)); // sum over levels of kFarSuper / W
      const int n_full = fp.box_count[top_lv] > 0 ? (fp.box_count[0] * 64) / kFarSuper : 0; // complete super-tiles
      int st = idx / per_super;
      if (st >= n_full) st = n_full; // the last, partial super-tile holds the rest
      idx -= st * per_super;
      level = top_lv;
      for (;;) {
        const int per = kFarSuper >> (6 + level);                  // boxes of this level per super-tile
        const int first = st * per;
        const int cnt = min(per, max(fp.box_count[level] - first, 0));
        if (idx < cnt || level == 0) {
          idx += first;
          break;
        }
        idx -= cnt;
        --level;
      }
    }
  }
  const int b = idx;
  const int lane = threadIdx.x;
  const int W = 64 << level, h = W >> 1;
  const int blo = g_lo + b * W, bhi = blo + W - 1;
  const int pm = fp.pm[layer];
  const int zm = min(zmax[layer], kHalf - 1);
  const int thr2 = ff_thr2(level, pm);
  const bool top = level == fp.n_levels - 1 && !M2L;
  const int W2 = 2 * W, plo = g_lo + (b >> 1) * W2, phi = plo + W2 - 1, thr2p = ff_thr2(level + 1, pm);
  const int zreq = zm + 2, pms = M2L ? fp.pm_src[layer] : 0; // box-pair mode: see m2l_valid

  // candidate centre intervals [lo, hi] (inclusive), see DESIGN.md
  int clo[4], chi[4], nr, n_extra = 0;
  const int mid = blo + h, near_in = thr2 / 2; // candidates: no closer than the admissible distance, rounded down
  if (M2L) {
    // the (line, box) pairs no box pair covers: source boxes closer than the first valid offset, and the two
    // source boxes on either side whose lines' windows end inside or just beyond this box (|o| = 101, 102)
    const int a_min = m2l_first_offset(0, zreq, pms);
    // (of those only the lines whose window holds the whole box: centre in [bhi - kHalf + 1, blo + kHalf])
    clo[0] = bhi - kHalf; chi[0] = blo - 100 * 64;
    clo[1] = blo - (a_min - 1) * 64 - 1; chi[1] = mid - near_in + 1;
    clo[2] = mid + near_in - 2; chi[2] = bhi + (a_min - 1) * 64 + 1;
    clo[3] = blo + 101 * 64 - 1; chi[3] = blo + kHalf + 1;
    nr = 4;
    n_extra = 2; // + the lines beyond the grid ends (FarParams::disp_lo_end)
  } else if (top) {
    clo[0] = blo - kHalf - 1; chi[0] = mid - near_in + 1;
    clo[1] = mid + near_in - 2; chi[1] = bhi + kHalf + 1;
    nr = 2;
  } else {
    // beyond bn a line is the parent's: the parent's centre is h from this box's, its admissible distance thr2p / 2
    const int bn = max((thr2p + 1) / 2 + h, zm + 3 * h) + 2;
    clo[0] = plo - kHalf; chi[0] = phi - (kHalf - 1) + 1;       // window end inside the parent
    clo[1] = mid - bn - 1; chi[1] = mid - near_in + 1;           // left near band
    clo[2] = mid + near_in - 2; chi[2] = mid + bn + 1;           // right near band
    clo[3] = plo + kHalf - 1; chi[3] = phi + kHalf + 1;          // window start inside the parent
    nr = 4;
  }
  int rs[6], re[6];
  for (int i = 0; i < nr; ++i) {
    rs[i] = lower_bound_ic(ix, clo[i]);
    re[i] = lower_bound_ic(ix, chi[i] + 1);
  }
  if (n_extra) {
    rs[nr] = 0; re[nr] = fp.disp_lo_end;
    rs[nr + 1] = fp.disp_hi_begin; re[nr + 1] = n_sub;
    nr += 2;
  }
  for (int i = 1; i < nr; ++i) // sort by start
    for (int k = i; k > 0 && rs[k] < rs[k - 1]; --k) {
      int t0 = rs[k]; rs[k] = rs[k - 1]; rs[k - 1] = t0;
      t0 = re[k]; re[k] = re[k - 1]; re[k - 1] = t0;
    }
  int done = 0; // make disjoint
  for (int i = 0; i < nr; ++i) {
    rs[i] = max(rs[i], done);
    re[i] = max(re[i], rs[i]);
    done = re[i];
  }

  double v[2 * kFC]; // [0, kFC): abs coefficients, [kFC, 2 kFC): emi
#pragma unroll
  for (int n = 0; n < 2 * kFC; ++n) v[n] = 0.;
  const FastRec *frow = fast + (size_t)layer * n_sub;
  const double hw = (double)h;
  unsigned n_exp = 0;
  // The candidate ranges as ONE list (they are disjoint and sorted): chunks of 64 across the range ends.  Taken range by
  // range, every range ended in a partly filled chunk, and a chunk costs its ~230 (8-term series: ~110) instructions
  // whatever its lanes hold: 5.2 chunk bodies per box on config 2 for 168 expansions.
  int off[7];
  off[0] = 0;
  for (int i = 0; i < 6; ++i) off[i + 1] = off[i] + (i < nr ? re[i] - rs[i] : 0);
  const int total = off[6];
  {
    for (int base = 0; base < total; base += 64) {
      const int g = base + lane;
      if (g >= total) continue;
      int l = rs[0] + g;
#pragma unroll
      for (int i = 1; i < 6; ++i)
        if (i < nr && g >= off[i]) l = rs[i] + (g - off[i]);
      const FastRec r = frow[l];
      const int j1 = r.j1, il = r.il(), ir = r.ir();
      if (!ff_admissible(j1, il, ir, blo, bhi, thr2)) continue;
      if (M2L) {
        const bool displaced = l < fp.disp_lo_end || l >= fp.disp_hi_begin;
        if (!displaced && m2l_valid(0, b - ((j1 + kHalf - g_lo) >> 6), zreq, pms)) continue; // covered by a box pair
      } else if (!top && ff_admissible(j1, il, ir, plo, phi, thr2p)) {
        continue; // owned by a wider box
      }
      const int cls = classify(j1, il, ir, blo, bhi);
      if (COUNT) ++n_exp;
      // x (or -x) at the box centre blo + h - 1/2, and the half-width in x units
      const double xc = cls == 1 ? fma(0.5 * (double)(2 * (blo - j1) + W - 1), r.xstep, -r.xl)
                                 : fma(0.5 * (double)(2 * (blo - (j1 + ir - 1)) + W - 1), r.xstep, r.xr);
      const double e = hw * r.xstep;
      const double u0 = xc * xc, u1 = 2. * xc * e, u2 = e * e;
      const R1Coef rq = r1_of(r);
      const double n0 = fma(rq.b, u0, rq.a), n1 = rq.b * u1, n2 = rq.b * u2;
      const double d0 = fma(u0, fma(4., u0, rq.d), rq.c);
      const double d1 = u1 * fma(8., u0, rq.d);
      const double d2 = fma(u2, rq.d, 4. * fma(u1, u1, 2. * u0 * u2));
      const double d3 = 8. * u1 * u2, d4 = 4. * u2 * u2;
      const double r0 = fast_rcp<2>(d0);
      const double D1 = d1 * r0, D2 = d2 * r0, D3 = d3 * r0, D4 = d4 * r0;
      // series coefficients f_n, accumulated as they are produced (a window of four is live)
      double f0 = n0 * r0;
      double f1 = fma(-D1, f0, n1 * r0);
      double f2 = fma(-D1, f1, fma(-D2, f0, n2 * r0));
      double f3 = -fma(D1, f2, fma(D2, f1, D3 * f0));
      v[0] = fma(r.wabs, f0, v[0]); v[kFC + 0] = fma(r.wemi, f0, v[kFC + 0]);
      v[1] = fma(r.wabs, f1, v[1]); v[kFC + 1] = fma(r.wemi, f1, v[kFC + 1]);
      v[2] = fma(r.wabs, f2, v[2]); v[kFC + 2] = fma(r.wemi, f2, v[kFC + 2]);
      v[3] = fma(r.wabs, f3, v[3]); v[kFC + 3] = fma(r.wemi, f3, v[kFC + 3]);
      // Box-pair mode: the lines of the window bands are > 6000 points away -- the series converges like
      // (32/6000)^n, eight terms carry it to 1e-18 of the leading one.  The bands are disjoint runs of the sorted
      // list, so whole chunks take the short path.
      constexpr int kShort = kFC < 8 ? kFC : 8;
      const int d_abs = blo - (j1 + kHalf);
      if (M2L && __all((d_abs < 0 ? -d_abs : d_abs) > 4096)) {
#pragma unroll
        for (int n = 4; n < kShort; ++n) {
          const double fn = -fma(D1, f3, fma(D2, f2, fma(D3, f1, D4 * f0)));
          v[n] = fma(r.wabs, fn, v[n]);
          v[kFC + n] = fma(r.wemi, fn, v[kFC + n]);
          f0 = f1; f1 = f2; f2 = f3; f3 = fn;
        }
        continue;
      }
#pragma unroll
      for (int n = 4; n < kFC; ++n) {
        const double fn = -fma(D1, f3, fma(D2, f2, fma(D3, f1, D4 * f0)));
        v[n] = fma(r.wabs, fn, v[n]);
        v[kFC + n] = fma(r.wemi, fn, v[kFC + n]);
        f0 = f1; f1 = f2; f2 = f3; f3 = fn;
      }
    }
  }
  // Sum the 2*kFC coefficient sets over the lanes.  A butterfly per value would cost
  // 6 exchanges each (480 ds_bpermute per box); exchanging HALF of the values at every
  // step instead (the lanes with bit m set keep the upper half) needs 2*kFC - 1 in all
  // and leaves one finished sum per lane.
  lane_reduce<2 * kFC, 32>(v, lane);
  bool primary = true;
  const int n_out = lane_reduce_index<2 * kFC, 32>(lane, primary);
  if (primary)
    fp.coef[((size_t)layer * fp.n_boxes_total + fp.box_off[level] + b) * (2 * kFC) + n_out] = v[0];
  if (COUNT) count_add(cnt, kCntExpansions, n_exp, lane);
}

// The per-line scheme for SPARSE line sets (the per-level passes of the pair tables: 0.09-0.16 lines per grid point):
// sr_farfield_kernel gives a (box, level, layer) a wave whatever the box holds -- five or six lines in one chunk body
// of ~230 instructions at a tenth of its lanes, behind ~450 of range searches, reduction and indexing: 0.34 of the pass's
// 0.53 ms were that.  Here a wave takes a box for kFarRows LAYERS: lane = (line of the chunk, layer), kFarLines lines x
// kFarRows layers per chunk body (8 x 8 when this was written, 4 x 16 as built now); the candidate ranges are the union over the wave's layers (the exact admissibility tests
// run per lane with its layer's margins), the 2 kFC sums are reduced over the kFarLines lanes of a layer (log2 of them exchange
// steps instead of six).  Same expansions, same owner of every (line, box): the coefficients differ from
// sr_farfield_kernel<., false>'s by the summation order.
#ifndef SR_FAR_ROWS
#define SR_FAR_ROWS 16 // layers per wave x 64 / that many lines.  8 x 8 through round 6 (degree 22: 16 x 4 and 4 x 16 lost);
                       // at degree 19 a table build of 12 levels: 16 x 4 11.94 / 23.92 ms (1e5 / 2e5 lines), 8 x 8 12.27 / 24.42, 4 x 16 13.45 / 26.74
#endif
constexpr int kFarRows = SR_FAR_ROWS, kFarLines = 64 / kFarRows; // lanes: kFarRows layers x kFarLines lines of a chunk
static_assert(kFarRows == 4 || kFarRows == 8 || kFarRows == 16, "SR_FAR_ROWS");
template <int N, int M>
__device__ inline void lane_reduce_slots(int lane, int *idx) { // which of the N values v[i] holds after lane_reduce<N, M>
  if constexpr (M >= 1) {
    constexpr int half = N / 2;
    const bool up = (lane & M) != 0;
#pragma unroll
    for (int i = 0; i < half; ++i) idx[i] = up ? idx[i + half] : idx[i];
    if constexpr (N & 1) idx[half] = idx[2 * half];
    lane_reduce_slots<half + (N & 1), M / 2>(lane, idx);
  }
}
template <int N, int M>
constexpr int lane_reduce_left() { // values per lane after lane_reduce<N, M>
  if constexpr (M >= 1) return lane_reduce_left<N / 2 + (N & 1), M / 2>(); else return N;
}
// NW waves per workgroup, each with a box of its own (wid: the wave's work id, < n_boxes_total x layer groups)
template <bool COUNT, int NW>
__device__ __forceinline__ void farfield_rows_body(const FastRec *__restrict__ fast, const IcIndex ix,
                                                   const int *__restrict__ zmax, int n_sub, int g_lo, const FarParams &fp,
                                                   unsigned long long *__restrict__ cnt, const int wid) {
  const int grp = wid / fp.n_boxes_total; // group of kFarRows layers
  int idx = wid - grp * fp.n_boxes_total, level = fp.n_levels - 1;
  while (level > 0 && idx >= fp.box_count[level]) { // widest level first
    idx -= fp.box_count[level];
    --level;
  }
  const int b = idx;
  const int lane = threadIdx.x & 63, sub = lane % kFarLines, layer = grp * kFarRows + lane / kFarLines;
  const bool live = layer < fp.n_layers;
  const int lc = min(layer, fp.n_layers - 1);
  const int W = 64 << level, h = W >> 1;
  const int blo = g_lo + b * W, bhi = blo + W - 1;
  const int pm = fp.pm[lc];
  const int zm = min(zmax[lc], kHalf - 1);
  const int thr2 = ff_thr2(level, pm);
  const bool top = level == fp.n_levels - 1;
  const int W2 = 2 * W, plo = g_lo + (b >> 1) * W2, phi = plo + W2 - 1, thr2p = ff_thr2(level + 1, pm);
  // margins of the wave's layers: the candidate ranges must hold every layer's candidates
  int pm_min = pm, pm_max = pm, zm_max = zm;
#pragma unroll
  for (int m = kFarLines; m < 64; m <<= 1) {
    pm_min = min(pm_min, __shfl_xor(pm_min, m));
    pm_max = max(pm_max, __shfl_xor(pm_max, m));
    zm_max = max(zm_max, __shfl_xor(zm_max, m));
  }
  pm_min = __builtin_amdgcn_readfirstlane(pm_min);
  pm_max = __builtin_amdgcn_readfirstlane(pm_max);
  zm_max = __builtin_amdgcn_readfirstlane(zm_max);
  // (the ranges live in LDS: as local arrays their dynamic indices put them in scratch memory -- 32 bytes per lane, and
  // a wave that owns scratch is dispatched through the scratch ring)
  __shared__ int rs_all[NW][4], re_all[NW][4];
  int *rs = rs_all[threadIdx.x >> 6], *re = re_all[threadIdx.x >> 6];
  int nr;
  const int mid = blo + h, near_in = ff_thr2(level, pm_min) / 2;
  if (top) {
    const int a0 = lower_bound_ic(ix, blo - kHalf - 1), b0 = lower_bound_ic(ix, mid - near_in + 1 + 1);
    const int a1 = lower_bound_ic(ix, mid + near_in - 2), b1 = lower_bound_ic(ix, bhi + kHalf + 1 + 1);
    rs[0] = a0; re[0] = b0; rs[1] = a1; re[1] = b1;
    nr = 2;
  } else {
    const int bn = max((ff_thr2(level + 1, pm_max) + 1) / 2 + h, zm_max + 3 * h) + 2; // (the parent's margin: see sr_farfield_kernel)
    const int a0 = lower_bound_ic(ix, plo - kHalf), b0 = lower_bound_ic(ix, phi - (kHalf - 1) + 1 + 1); // window end inside the parent
    const int a1 = lower_bound_ic(ix, mid - bn - 1), b1 = lower_bound_ic(ix, mid - near_in + 1 + 1);   // left near band
    const int a2 = lower_bound_ic(ix, mid + near_in - 2), b2 = lower_bound_ic(ix, mid + bn + 1 + 1);   // right near band
    const int a3 = lower_bound_ic(ix, plo + kHalf - 1), b3 = lower_bound_ic(ix, phi + kHalf + 1 + 1);  // window start inside the parent
    rs[0] = a0; re[0] = b0; rs[1] = a1; re[1] = b1; rs[2] = a2; re[2] = b2; rs[3] = a3; re[3] = b3;
    nr = 4;
  }
  for (int i = 1; i < nr; ++i) // sort by start
    for (int k = i; k > 0 && rs[k] < rs[k - 1]; --k) {
      int t0 = rs[k]; rs[k] = rs[k - 1]; rs[k - 1] = t0;
      t0 = re[k]; re[k] = re[k - 1]; re[k - 1] = t0;
    }
  int done = 0; // make disjoint
  for (int i = 0; i < nr; ++i) {
    rs[i] = max(rs[i], done);
    re[i] = max(re[i], rs[i]);
    done = re[i];
  }
  // Adjacent ranges merge; the chunks are aligned on multiples of eight LINE INDICES, lane sub takes the lines with
  // l = sub (mod 8) in increasing order: which lane adds which line, and in which order, then depends on the layer's
  // own admissible lines alone -- not on the other layers of the wave, whose margins widen the ranges -- and a layer
  // stack processed in batches (sr_set_table_budget) gives the bits of the unbatched call.
  int nm = 0;
  for (int i = 0; i < nr; ++i) {
    if (re[i] <= rs[i]) continue;
    if (nm > 0 && rs[i] <= ((re[nm - 1] + kFarLines - 1) & ~(kFarLines - 1))) {
      re[nm - 1] = re[i]; // (the lines between the two ranges are no candidates of any layer: the exact tests reject them)
    } else {
      rs[nm] = rs[i]; re[nm] = re[i]; ++nm;
    }
  }

  // (Round 6 tried two phases -- the admissibility tests over all candidates first, every layer row queueing its
  // admissible lines in LDS, then eight queued lines of a row at a time: 333 -> 1109 us per sparse pass; the candidates
  // of a box are mostly its own already, the queue's round trip and the second record fetch were pure cost.
  // And two chunks at a time -- both records requested first, the two chains of 4 x kFC dependent fma interleaved, chunks
  // without an admissible lane skipped as here; the same doubles -- : 168 VGPRs, still three waves per SIMD, a table build
  // 13.0 -> 13.6 ms (1e5 x 1e5 x 80) and 25.2 -> 26.4 (2e5), same box: the chain's latency is not what the kernel waits for.)
  double v[2 * kFC];
#pragma unroll
  for (int n = 0; n < 2 * kFC; ++n) v[n] = 0.;
  const FastRec *frow = fast + (size_t)lc * n_sub;
  const double hw = (double)h;
  unsigned n_exp = 0;
  for (int i = 0; i < nm; ++i) {
  const int rsi = __builtin_amdgcn_readfirstlane(rs[i]), rei = __builtin_amdgcn_readfirstlane(re[i]);
  for (int l0 = rsi & ~(kFarLines - 1); l0 < rei; l0 += kFarLines) {
    const int l = l0 + sub;
    if (l < rsi || l >= rei || !live) continue;
    const FastRec r = frow[l];
    const int j1 = r.j1, il = r.il(), ir = r.ir();
    if (!ff_admissible(j1, il, ir, blo, bhi, thr2)) continue;
    if (!top && ff_admissible(j1, il, ir, plo, phi, thr2p)) continue; // owned by a wider box
    const int cls = classify(j1, il, ir, blo, bhi);
    if (COUNT) ++n_exp;
    const double xc = cls == 1 ? fma(0.5 * (double)(2 * (blo - j1) + W - 1), r.xstep, -r.xl)
                               : fma(0.5 * (double)(2 * (blo - (j1 + ir - 1)) + W - 1), r.xstep, r.xr);
    const double e = hw * r.xstep;
    const double u0 = xc * xc, u1 = 2. * xc * e, u2 = e * e;
    const R1Coef rq = r1_of(r);
    const double n0 = fma(rq.b, u0, rq.a), n1 = rq.b * u1, n2 = rq.b * u2;
    const double d0 = fma(u0, fma(4., u0, rq.d), rq.c);
    const double d1 = u1 * fma(8., u0, rq.d);
    const double d2 = fma(u2, rq.d, 4. * fma(u1, u1, 2. * u0 * u2));
    const double d3 = 8. * u1 * u2, d4 = 4. * u2 * u2;
    const double r0 = fast_rcp<2>(d0);
    const double D1 = d1 * r0, D2 = d2 * r0, D3 = d3 * r0, D4 = d4 * r0;
    double f0 = n0 * r0;
    double f1 = fma(-D1, f0, n1 * r0);
    double f2 = fma(-D1, f1, fma(-D2, f0, n2 * r0));
    double f3 = -fma(D1, f2, fma(D2, f1, D3 * f0));
    v[0] = fma(r.wabs, f0, v[0]); v[kFC + 0] = fma(r.wemi, f0, v[kFC + 0]);
    v[1] = fma(r.wabs, f1, v[1]); v[kFC + 1] = fma(r.wemi, f1, v[kFC + 1]);
    v[2] = fma(r.wabs, f2, v[2]); v[kFC + 2] = fma(r.wemi, f2, v[kFC + 2]);
    v[3] = fma(r.wabs, f3, v[3]); v[kFC + 3] = fma(r.wemi, f3, v[kFC + 3]);
#pragma unroll
    for (int n = 4; n < kFC; ++n) {
      const double fn = -fma(D1, f3, fma(D2, f2, fma(D3, f1, D4 * f0)));
      v[n] = fma(r.wabs, fn, v[n]);
      v[kFC + n] = fma(r.wemi, fn, v[kFC + n]);
      f0 = f1; f1 = f2; f2 = f3; f3 = fn;
    }
  }
  }
  // sums over the eight lanes of a layer (lane bits 4, 2, 1); every lane is left with kLeft finished values
  lane_reduce<2 * kFC, kFarLines / 2>(v, lane);
  constexpr int kLeft = lane_reduce_left<2 * kFC, kFarLines / 2>();
  int slot[2 * kFC];
#pragma unroll
  for (int n = 0; n < 2 * kFC; ++n) slot[n] = n;
  lane_reduce_slots<2 * kFC, kFarLines / 2>(lane, slot);
  if (live) {
    double *out = fp.coef + ((size_t)layer * fp.n_boxes_total + fp.box_off[level] + b) * (2 * kFC);
#pragma unroll
    for (int n = 0; n < kLeft; ++n) out[slot[n]] = v[n]; // (an unpaired value is held by two lanes: the same sum twice)
  }
  if (COUNT) count_add(cnt, kCntExpansions, n_exp, lane);
}
// (The sparse sets' kernels: occupancy unconstrained, 138 VGPRs = 3 waves per SIMD; built for 4: 128 VGPRs + 48 B of scratch in the batch kernel, a table build 13.4 -> 15.1 ms.)
template <bool COUNT>
__global__ __launch_bounds__(64) void sr_farfield_rows_kernel(const FastRec *__restrict__ fast, IcIndex ix,
                                                              const int *__restrict__ zmax, int n_sub, int g_lo, FarParams fp,
                                                              unsigned long long *__restrict__ cnt) {
  farfield_rows_body<COUNT, 1>(fast, ix, zmax, n_sub, g_lo, fp, cnt, xcd_remap_groups((int)blockIdx.x, (int)gridDim.x, 16));
}
// ... of every sparse far-only pass of a table build in one launch (grid.y = item): one at a time these launches --
// eleven of 0.3 ms, latency-bound, each behind ~0.3 ms of host calls -- were 6 ms of a 13 ms build
#ifndef SR_ROWS_BATCH_WAVES
#define SR_ROWS_BATCH_WAVES 4
#endif
constexpr int kRowsBatchWaves = SR_ROWS_BATCH_WAVES; // waves (boxes) per workgroup of the batch kernel
__global__ __launch_bounds__(64 * kRowsBatchWaves) void sr_farfield_rows_batch_kernel(const FarBatchItem *__restrict__ items, const int *__restrict__ zmax,
                                                                    int g_lo, FarParams fp, int n_work) {
  const FarBatchItem it = items[blockIdx.y];
  fp.coef = it.coef;
  const int wid = xcd_remap_groups((int)blockIdx.x, (int)gridDim.x, 16 / kRowsBatchWaves) * kRowsBatchWaves + (int)(threadIdx.x >> 6);
  if (wid >= n_work) return; // (wave-uniform; the kernel has no block barrier)
  farfield_rows_body<false, kRowsBatchWaves>(it.fast, IcIndex{it.first, it.first_x0, it.first_n, it.line_lo, it.n_sub}, zmax, it.n_sub, g_lo, fp,
                                             nullptr, wid);
}

// ------------------------------------------------------------------------
// Box-pair far field (FarParams::m2l): multipole moments, upward pass, translations.
//
// Region 1 of a line is w g(x), g(x) = (a + b x^2)/(c + d x^2 + 4 x^4), x = xstep (j - j0) with j0 the (real)
// grid position where the reference's running x of that wing passes through zero.  At infinity
// g = sum_n e_(n-1) x^(-2n), e_0 = b/4, e_1 = (a - d e_0)/4, e_k = -(d e_(k-1) + c e_(k-2))/4, and about the
// centre C of a source box of half-width h (delta = j0 - C, J = j - C):
//   (J - delta)^(-2n) = sum_m binom(2n + m - 1, m) delta^m J^(-2n-m)
//   =>  g = sum_q M_q J^(-q),  M_q / (h^q (q-1)!) = sum_(2n+m=q) [e_(n-1) (xstep h)^(-2n)/(2n-1)!] [(delta/h)^m/m!]
// -- a convolution of two short series per line, summed over the lines of the box with lanes = lines.  The
// scaled moments mh_q of a parent box follow from its children (centres -+ h/2 from its own) by
//   mh_q = 2^-q sum_(m=0..q-2) (mhL_(q-m) (-1)^m + mhR_(q-m))/m!
// and the local coefficients (in t = (j - centre)/h, the polynomial each point evaluates) of a target box
// o boxes away by  L_n = sum_q T_o[n][q] mh_q,  T_o[n][q] = (-1)^n (q+n-1)!/n! (1/2o)^(q+n)  (host table).
// The two wings of a line use different anchors (xl from x(1), xr from x(ir): lineshape.f:462, 471; they differ
// by the rounding of the grid, ~1e-9 points), hence two sets of moments: side 0 serves targets right of the
// source box, side 1 targets left of it.
// ------------------------------------------------------------------------
__device__ constexpr double inv_factorial(int n) {
  double f = 1.0;
  for (int i = 2; i <= n; ++i) f *= (double)i;
  return 1.0 / f;
}
// One wave per (source box, layer); lane = (line % 32, side): the lower half-wave builds the right-going moments
// of 32 lines at a time, the upper half the left-going ones of the same lines, and each half sums its 2 kMQ values
// over its own 32 lanes.  (A box holds 64 +- 8 lines on config 2: with 64 lines per step and one wave per side the
// second step of most boxes ran nearly empty.)
// (Occupancy unconstrained, 154 VGPRs; built for 4 waves per SIMD like sr_farfield_kernel: 104 B of scratch.)
// (one convolution per line about the MEAN of its two anchors + first-order corrections; round 3's one-per-side
// variant is in the history: S2M 0.375 vs 0.31 ms)
// Round 4: one moment set per line instead of one per side.  The two wings of a line use different anchors (the zero of
// the reference's running x: xl from x(1), xr from x(ir): lineshape.f:462, 471), eps ~ 1e-9 grid points apart (the
// rounding of the grid).  The moments are analytic in the anchor: M_q(delta +- eps / 2) = M_q(delta) +- (eps / 2) d M_q /
// d delta + O(eps^2 ~ 1e-18), and d m_q / d delta = m_(q-1) / h for the scaled per-line moments (the delta-series
// D_m = (delta / h)^m / m! shifts by one index).  So: ONE convolution per line about the mean anchor (lane = line, 64
// lines per step instead of 32 per side: a box holds 64 +- 8 lines -- 1.5 steps on average instead of 2.5), the sums
// v_q, and correction sums c_q = sum_i w_i (eps_i / 2 h) m_(q-1, i) for q = 3..6 only -- the correction of order q
// reaches a target J >= 192 points away with (h / J)^(q - 2) of a term that is 1e-11 of the pair's contribution to begin
// with: beyond q = 6 that is < 1e-15.  Written out: side 0 (right-going) = v + c, side 1 (left-going) = v - c: M2M and
// M2L read what they always read.
constexpr int kS2MCorr = 4; // corrected orders q = 3 .. 2 + kS2MCorr
template <bool COUNT>
__global__ __launch_bounds__(64) void sr_s2m_kernel(const FastRec *__restrict__ fast, IcIndex ix, int n_sub, int g_lo,
                                                    FarParams fp, unsigned long long *__restrict__ cnt) {
  const int wid = xcd_remap(blockIdx.x, gridDim.x);
  const int layer = wid / fp.n_src[0], sb = wid - layer * fp.n_src[0];
  const int lane = threadIdx.x;
  const int s_lo = g_lo + (sb - kSrcPad) * 64; // first centre position of the box
  // A box wholly LEFT of the shard only ever serves targets to its right (side 0), one wholly right of it targets to
  // its left (side 1) -- and so do all its ancestors: the side nobody reads is written as zeros (sr_m2m_kernel skips it).
  const int only = s_lo + 64 <= g_lo ? 0 : (s_lo >= g_lo + fp.box_count[0] * 64 ? 1 : -1);
  const int l0 = lower_bound_ic(ix, s_lo), l1 = lower_bound_ic(ix, s_lo + 64);
  constexpr int NE = kFD / 2; // terms of the Laurent series
  double v[2 * kMQ];          // [0, kMQ): abs, [kMQ, 2 kMQ): emi -- about the mean anchor
  double c[2 * kS2MCorr];     // first-order anchor corrections of orders 3 .. 2 + kS2MCorr: abs, emi
#pragma unroll
  for (int n = 0; n < 2 * kMQ; ++n) v[n] = 0.;
#pragma unroll
  for (int n = 0; n < 2 * kS2MCorr; ++n) c[n] = 0.;
  const FastRec *frow = fast + (size_t)layer * n_sub;
  unsigned n_lines = 0;
  for (int base = l0; base < l1; base += 64) {
    const int l = base + lane;
    if (l >= l1 || l < fp.disp_lo_end || l >= fp.disp_hi_begin) continue;
    const FastRec r = frow[l];
    if (COUNT) n_lines += 2; // (line, side) pairs served
    constexpr double h = 32.0;
    const double sh = r.xstep * h;
    const double V = fast_rcp<2>(sh * sh);
    double E[NE]; // e_(n-1) (xstep h)^(-2n) / (2n-1)!
    {
      const R1Coef rq = r1_of(r);
      const double dV = 0.25 * rq.d * V, cV = 0.25 * rq.c * (V * V);
      E[0] = 0.25 * rq.b * V;
      E[1] = fma(0.25 * rq.a * V, V, -dV * E[0]);
#pragma unroll
      for (int k = 2; k < NE; ++k) E[k] = -fma(dV, E[k - 1], cV * E[k - 2]);
#pragma unroll
      for (int k = 1; k < NE; ++k) E[k] *= inv_factorial(2 * k + 1);
    }
    // zeros of the two running x, relative to the box centre s_lo + 31.5 (grid points)
    const double inv_xs = fast_rcp<2>(r.xstep);
    const double off_r = (double)(r.j1 + r.ir() - 1 - s_lo - 32) + (0.5 - r.xr * inv_xs);
    const double off_l = (double)(r.j1 - s_lo - 32) + (0.5 + r.xl * inv_xs);
    const double dt = (0.5 / h) * (off_r + off_l);   // mean anchor / h
    const double eh = (0.5 / h) * (off_r - off_l);   // eps / 2 h: side 0 sits at dt + eh, side 1 at dt - eh
    double D[kMQ]; // (delta/h)^m / m!, m = 0..kFD-2
    D[0] = 1.0;
#pragma unroll
    for (int m = 1; m < kMQ; ++m) D[m] = D[m - 1] * (dt * (1.0 / (double)m));
    const double wa_e = r.wabs * eh, we_e = r.wemi * eh;
#pragma unroll
    for (int q = 2; q <= kFD; ++q) {
      double mq = 0.;
#pragma unroll
      for (int n = 1; 2 * n <= q; ++n) mq = fma(E[n - 1], D[q - 2 * n], mq);
      v[q - 2] = fma(r.wabs, mq, v[q - 2]);
      v[kMQ + q - 2] = fma(r.wemi, mq, v[kMQ + q - 2]);
      if (q - 2 < kS2MCorr) { // d m_(q+1) / d delta = m_q / h
        c[q - 2] = fma(wa_e, mq, c[q - 2]);
        c[kS2MCorr + q - 2] = fma(we_e, mq, c[kS2MCorr + q - 2]);
      }
    }
  }
  // sums over the 64 lanes: the moments by halving exchanges (one finished value per lane), the few corrections by butterflies
  lane_reduce<kMQ, 32>(v, lane);
  lane_reduce<kMQ, 32>(v + kMQ, lane);
#pragma unroll
  for (int n = 0; n < 2 * kS2MCorr; ++n)
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) c[n] += __shfl_xor(c[n], m);
  bool primary = true;
  const int n_out = lane_reduce_index<kMQ, 32>(lane, primary); // this lane holds order q = n_out + 2
  if (primary) {
    double ca = 0., ce = 0.; // correction of order q = n_out + 2: c index q - 3
#pragma unroll
    for (int i = 0; i < kS2MCorr; ++i) {
      ca = n_out == i + 1 ? c[i] : ca;
      ce = n_out == i + 1 ? c[kS2MCorr + i] : ce;
    }
    double *mo = fp.mom + ((size_t)(fp.src_off[0] + sb) * fp.n_layers + layer) * kMomPerBox + n_out;
    const bool z0 = only == 1, z1 = only == 0; // the side a halo box never serves
    mo[0] = z0 ? 0.0 : v[0] + ca;                       // side 0 (right-going), abs
    mo[kMQ] = z0 ? 0.0 : v[kMQ] + ce;                   //                       emi
    mo[2 * kMQ] = z1 ? 0.0 : v[0] - ca;                 // side 1 (left-going), abs
    mo[3 * kMQ] = z1 ? 0.0 : v[kMQ] - ce;
  }
  if (COUNT) count_add(cnt, kCntS2M, n_lines, lane);
}

// One thread per (parent box of level l, layer, side, weight); one launch per level, narrow to wide (round 3: one
// thread per widest-level subtree walked all its 15 boxes in sequence -- 500 waves with 15 dependent rounds of loads:
// 70 us alone on config 2, 130-210 us in the step's traces, where this kernel runs on an otherwise idle chip).
__global__ __launch_bounds__(64) void sr_m2m_kernel(FarParams fp, int l) {
  const int tid = blockIdx.x * blockDim.x + threadIdx.x;
  if (tid >= fp.n_src[l] * fp.n_layers * 4) return;
  const int sw = tid & 3, rest = tid >> 2;
  const int layer = rest % fp.n_layers, p = rest / fp.n_layers;
  // halo boxes: the side nobody reads is not built (see sr_s2m_kernel); sw = side * 2 + weight
  if ((sw >> 1) == 1 ? ((p + 1) << l) <= kSrcPad : (p << l) - kSrcPad >= fp.box_count[0]) return;
  const double *cl = fp.mom + ((size_t)(fp.src_off[l - 1] + 2 * p) * fp.n_layers + layer) * kMomPerBox + sw * kMQ;
  const double *cr = cl + (size_t)fp.n_layers * kMomPerBox;
  double *par = fp.mom + ((size_t)(fp.src_off[l] + p) * fp.n_layers + layer) * kMomPerBox + sw * kMQ;
  double a[kMQ], b[kMQ];
#pragma unroll
  for (int q = 0; q < kMQ; ++q) {
    a[q] = cl[q];
    b[q] = cr[q];
  }
  double scale = 0.25; // 2^-q
#pragma unroll
  for (int q = 2; q <= kFD; ++q) {
    double s = 0.;
#pragma unroll
    for (int m = 0; m <= q - 2; ++m) {
      const double pair = (m & 1) ? b[q - m - 2] - a[q - m - 2] : b[q - m - 2] + a[q - m - 2];
      s = fma(pair, inv_factorial(m), s);
    }
    par[q - 2] = s * scale;
    scale *= 0.5;
  }
}

// Translations: L[pair][n] += sum_q mh[pair][q] T_o[q][n] is a small dense product per box offset o, the one
// place of this path with the shape of a matrix multiplication: v_mfma_f64_16x16x4_f64 with A = the moments of 16
// (target box, layer) pairs (rows) and B = the operator (16 of the kFC columns).  The matrix unit is no faster than
// the vector unit in fp64, but one lane-load of A and of B feeds 2 x 256 fma: the vector formulations were bound by
// their loads (lanes = pairs, operator by scalar loads: 0.9-1.6 ms on config 2; lane = (pair, n) with two
// accumulators: 63 loads per 42 fma, 1.0 ms).  Layout (cdna_hip_programming.md): A[row = lane & 15][k = lane >> 4],
// B[k = lane >> 4][col = lane & 15], D[row = (lane >> 4) + 4 r][col = lane & 15], r = 0..3.
// A pair that does not take part in an offset (its own validity, or it lies outside the level) enters with zeros.
// Stores the local coefficients of levels >= 1, adds to those the level-0 pass of sr_farfield_kernel stored.
constexpr int kM2LSlices = kM2LRow / 16; // column tiles: all in one wave (the A loads are the cost, shared by them)
template <bool COUNT>
__global__ __launch_bounds__(64) void sr_m2l_kernel(const int *__restrict__ zmax, FarParams fp,
                                                    unsigned long long *__restrict__ cnt) {
  int chunk = blockIdx.x, level = 0;
  for (;;) {
    const int c = (fp.box_count[level] * fp.n_layers + 15) >> 4;
    if (chunk < c || level + 1 >= fp.n_levels) break;
    chunk -= c;
    ++level;
  }
  const int lane = threadIdx.x, lo = lane & 15, kq = lane >> 4;
  const int n_pairs = fp.box_count[level] * fp.n_layers;
  // the pair of this lane's A row
  const int idx = chunk * 16 + lo;
  const bool live = idx < n_pairs;
  const int t = live ? idx / fp.n_layers : 0, layer = live ? idx - t * fp.n_layers : 0;
  const int zreq = min(zmax[layer], kHalf - 1) + 2, pms = fp.pm_src[layer];
  const int W = 64 << level;
  const bool has_parent = level + 1 < fp.n_levels;
  const int a_max = (kHalf + 1) / W - 1;
  // offsets whose parent pair can be invalid: close ones (parent closer than its first valid offset, taken over
  // the wave's layers) and the ones at the window ends
  int near_hi = a_max, win_lo = a_max + 1;
  if (has_parent) {
    const int W2 = 2 * W;
    int a_min_p = m2l_first_offset(level + 1, zreq, pms);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) a_min_p = max(a_min_p, __shfl_xor(a_min_p, m));
    near_hi = __builtin_amdgcn_readfirstlane(min(a_max, 2 * a_min_p + 1));
    win_lo = max(near_hi + 1, 2 * (kHalf / W2 - 1));
  }
  unsigned n_pairs_on = 0; // COUNT: translations of this lane's pair (counted once per pair: kq == 0)
  v4d acc_a[kM2LSlices], acc_e[kM2LSlices];
#pragma unroll
  for (int sl = 0; sl < kM2LSlices; ++sl) acc_a[sl] = acc_e[sl] = v4d{0., 0., 0., 0.};
  const int pad = kSrcPad >> level;
  for (int a = 3; a <= a_max; a = (a == near_hi ? win_lo : a + 1)) {
    for (int sg = 0; sg < 2; ++sg) {
      const int o = sg ? -a : a, s = t - o;
      const int sidx = s + pad;
      const bool on = live && sidx >= 0 && sidx < fp.n_src[level] && m2l_valid(level, o, zreq, pms) &&
                      !(has_parent && m2l_valid(level + 1, (t >> 1) - (s >> 1), zreq, pms));
      if (!__any(on)) continue;
      if (COUNT) n_pairs_on += on && kq == 0;
      const double *m = fp.mom + ((size_t)(fp.src_off[level] + (on ? sidx : 0)) * fp.n_layers + layer) * kMomPerBox + sg * (2 * kMQ);
      const double *T = fp.tab + ((size_t)sg * kM2LOffsets + a) * (kM2LQ * kM2LRow) + lo;
#pragma unroll
      for (int ks = 0; ks < kM2LQ / 4; ++ks) {
        const int q = 4 * ks + kq;
        const bool use = on && q < kMQ;
        const double A_a = use ? m[q] : 0.0;
        const double A_e = use ? m[kMQ + q] : 0.0;
#pragma unroll
        for (int sl = 0; sl < kM2LSlices; ++sl) {
          const double B = T[q * kM2LRow + 16 * sl];
          acc_a[sl] = __builtin_amdgcn_mfma_f64_16x16x4f64(A_a, B, acc_a[sl], 0, 0, 0);
          acc_e[sl] = __builtin_amdgcn_mfma_f64_16x16x4f64(A_e, B, acc_e[sl], 0, 0, 0);
        }
      }
    }
  }
  if (COUNT) count_add(cnt, kCntM2L, n_pairs_on, lane);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int io = chunk * 16 + kq + 4 * r; // the pair of D's row
    if (io >= n_pairs) continue;
    const int to = io / fp.n_layers, lyo = io - to * fp.n_layers;
    double *c = fp.coef + ((size_t)lyo * fp.n_boxes_total + fp.box_off[level] + to) * (2 * kFC);
#pragma unroll
    for (int sl = 0; sl < kM2LSlices; ++sl) {
      const int n = 16 * sl + lo; // this lane's column of D
      if (n < kFC) {
        if (level == 0) {
          c[n] += acc_a[sl][r];
          c[kFC + n] += acc_e[sl][r];
        } else {
          c[n] = acc_a[sl][r];
          c[kFC + n] = acc_e[sl][r];
        }
      }
    }
  }
}

// Exact near field + evaluation of the far-field polynomials.  The scalar unit is shared by
// the CU's four SIMDs, so ownership tests and interval arithmetic run on the VALU, 64 candidate
// lines at a time (lane = line); ballots mark the lines with work; those are walked in ROWS: the
// wave's 64 lanes as 8 rows of 8, a row takes one line (its record by per-lane loads) and steps
// through that line's points 8 at a time.
//
// sr_abscoeff_near_wings_kernel (one 64-point slot per wave): every REGION-1 point of the
//   lines that no far-field level owns for the slot, in rows; the slots holding a window end or
//   start by per-line expansions and a lane scan (window_end_sum) -- plus one far-field
//   polynomial per level; writes abs/emi (or adds, when the zones kernel stored first).
// sr_abscoeff_near_zones_kernel (one 512-point LDS image per wave; stores or adds to abs/emi):
//   region 3 (~15 points per line) with lanes = lines in the chunk phase; regions 2 and 4 in
//   rows, sums by return-less LDS adds (one wave per image, program order: deterministic).
// ------------------------------------------------------------------------
__device__ inline void near_ranges(const IcIndex &ix, int wlo, int width, int zm,
                                   int rs[3], int re[3]) {
  // candidates as ranges of the sorted centre list, C <= A <= B by start; NOMINAL tile end
  // (the far-field kernel tests nominal boxes, which may reach past g_hi):
  //  C: window END inside the tile      ic+6504 in [wlo, whn]
  //  A: within zm of the tile           ic in [wlo-zm, whn+zm]
  //  B: window START inside the tile    ic-6505 in (wlo, whn]
  const int whn = wlo + width - 1;
  const int c0 = lower_bound_ic(ix, wlo - (kHalf - 1));
  const int c1 = lower_bound_ic(ix, whn - (kHalf - 1) + 1);
  const int a0 = lower_bound_ic(ix, wlo - zm);
  const int a1 = lower_bound_ic(ix, whn + zm + 1);
  const int b0 = lower_bound_ic(ix, wlo + kHalf + 1);
  const int b1 = lower_bound_ic(ix, whn + kHalf + 1);
  rs[0] = c0; re[0] = max(c1, c0);
  rs[1] = max(a0, re[0]); re[1] = max(a1, rs[1]);
  rs[2] = max(b0, re[1]); re[2] = max(b1, rs[2]);
}

// ------------------------------------------------------------------------
// Window ends.  Every line has two, and in the slot holding one it contributes region-1 values to the
// points up to (from) its last (first) window point only -- nothing beyond, exactly as the
// reference's 13010-point window.  Walked line by line these partial slots were half of the near
// wings kernel (64 ends + 64 starts per slot at one line per point).  They are 6441+ points from
// the line centre, where the wing is so smooth over 64 points (Taylor ratio 32/6441) that degree 5
// is exact to 2e-14 of the term; so: lanes = lines, each lane expands its own line about the slot
// centre, a suffix (ends) / prefix (starts) sum over the lanes -- the lines are sorted by window
// position -- gives for every cut-off position the polynomial of all lines still (already) inside
// their window, and each point evaluates the one for its own position.
// (the sums over the lanes: dpp_move and lane_value, sr_device.hpp)
// ------------------------------------------------------------------------
constexpr int kWE = 6; // series coefficients of the window-end expansions
__device__ inline void wing_series6(double xc, double e, const FastRec &r, double f[kWE]) {
  const double u0 = xc * xc, u1 = 2. * xc * e, u2 = e * e;
  const R1Coef rq = r1_of(r);
  const double n0 = fma(rq.b, u0, rq.a), n1 = rq.b * u1, n2 = rq.b * u2;
  const double d0 = fma(u0, fma(4., u0, rq.d), rq.c);
  const double d1 = u1 * fma(8., u0, rq.d);
  const double d2 = fma(u2, rq.d, 4. * fma(u1, u1, 2. * u0 * u2));
  const double d3 = 8. * u1 * u2, d4 = 4. * u2 * u2;
  const double r0 = fast_rcp<2>(d0);
  const double D1 = d1 * r0, D2 = d2 * r0, D3 = d3 * r0, D4 = d4 * r0;
  f[0] = n0 * r0;
  f[1] = fma(-D1, f[0], n1 * r0);
  f[2] = fma(-D1, f[1], fma(-D2, f[0], n2 * r0));
  f[3] = -fma(D1, f[2], fma(D2, f[1], D3 * f[0]));
#pragma unroll
  for (int n = 4; n < kWE; ++n) f[n] = -fma(D1, f[n - 1], fma(D2, f[n - 2], fma(D3, f[n - 3], D4 * f[n - 4])));
}
// Sum over the lanes' lines of (value at this lane's point, 0 outside the line's window) for one chunk
// of 64 lines.  ends: line of lane i is valid at points p <= pos_i; starts: at p >= pos_i; pos is
// non-decreasing over the lanes (lines sorted by window centre); lanes without such a line carry
// zero coefficients.  c: [0, kWE) abs, [kWE, 2 kWE) emi series coefficients of the lane's line.
__device__ inline void window_end_sum(bool ends, int pos, double c[2 * kWE], int lane, double &out_a, double &out_e) {
  // inclusive suffix (ends) or prefix (starts) sums over the lanes: inside each row of 16 lanes by DPP
  // row shifts (plain VALU moves, zero shifted in at the row end), then the totals of the other rows
  const int row = lane >> 4;
#pragma unroll
  for (int n = 0; n < 2 * kWE; ++n) {
    double v = c[n];
    if (ends) {
      v += dpp_move<0x101>(v); // row_shl:1  lane i <- lane i + 1
      v += dpp_move<0x102>(v);
      v += dpp_move<0x104>(v);
      v += dpp_move<0x108>(v);
      const double t1 = lane_value(v, 16), t2 = lane_value(v, 32), t3 = lane_value(v, 48); // row totals
      const double t23 = t2 + t3;
      v += row == 0 ? t1 + t23 : (row == 1 ? t23 : (row == 2 ? t3 : 0.0));
    } else {
      v += dpp_move<0x111>(v); // row_shr:1  lane i <- lane i - 1
      v += dpp_move<0x112>(v);
      v += dpp_move<0x114>(v);
      v += dpp_move<0x118>(v);
      const double t0 = lane_value(v, 15), t1 = lane_value(v, 31), t2 = lane_value(v, 47);
      const double t01 = t0 + t1;
      v += row == 3 ? t01 + t2 : (row == 2 ? t01 : (row == 1 ? t0 : 0.0));
    }
    c[n] = v;
  }
  // this lane as a POINT p = lane: ends: first line with pos >= p; starts: last line with pos <= p
  int lo = 0, hi = 64; // 65 possible answers: 7 halvings
#pragma unroll
  for (int it = 0; it < 7; ++it) {
    const int mid = min((lo + hi) >> 1, 63);
    const int v = __shfl(pos, mid);
    const bool right = lo < hi && (ends ? v < lane : v <= lane);
    const bool left = lo < hi && !right;
    lo = right ? mid + 1 : lo;
    hi = left ? mid : hi;
  }
  const int src = ends ? lo : lo - 1; // lo = number of lines with pos < p (ends) / pos <= p (starts)
  const bool any = ends ? src < 64 : src >= 0;
  const double t = (double)(2 * lane - 63) * (1.0 / 64);
  double pa = 0., pe = 0.;
#pragma unroll
  for (int n = kWE - 1; n >= 0; --n) {
    const double ca = __shfl(c[n], src & 63), ce = __shfl(c[kWE + n], src & 63);
    pa = fma(pa, t, any ? ca : 0.0);
    pe = fma(pe, t, any ? ce : 0.0);
  }
  out_a += pa;
  out_e += pe;
}

// One 64-point slot per wave (4 or 2 slots per wave measured slower: 2.53 / 2.31 ms on config 2 at the time).
// Per chunk of 64 candidate lines (lane = line): which lines have region-1 points in the slot that no far-field
// level owns; window ends / starts by expansion and scan; the rest in ROWS: eight lines at a time, each row of 8
// lanes evaluates ONE line at 8 points per step (8 steps cover the slot), the line's record in the row's registers
// by per-lane loads.  Before, every such line cost a scalar record fetch, a ballot walk and four specialised masked
// loops: the walk took 0.87 of the kernel's 1.34 ms for 0.27 ms worth of vector work.
template <bool COUNT>
__global__ __launch_bounds__(64) void sr_abscoeff_near_wings_kernel(
    const FastRec *__restrict__ fast, IcIndex ix, const int *__restrict__ zmax, int n_sub,
    int n_tiles, int g_lo, int g_hi, FarParams fp, int add, const double *__restrict__ z_abs,
    const double *__restrict__ z_emi, double *__restrict__ abs_out, double *__restrict__ emi_out,
    unsigned long long *__restrict__ cnt) {
  const int wg = xcd_remap(blockIdx.x, gridDim.x);
  const int layer = wg / n_tiles, tile = wg - layer * n_tiles;
  const int wlo = g_lo + tile * 64;
  const int whi = min(wlo + 64, g_hi) - 1;
  const int lane = threadIdx.x;
  const int pm = fp.pm[layer];
  const int thr0 = ff_thr2(0, pm);
  int rs[3], re[3];
  near_ranges(ix, wlo, 64, min(max(zmax[layer], kTheta * 32 + pm + 1), kHalf - 1), rs, re);

  constexpr int kRowLanes = 8, kRows = 8;
  const int row = lane / kRowLanes, col = lane % kRowLanes;
  double sum_a = 0., sum_e = 0.; // this lane's point wlo + lane: window ends, polynomials, and the rows' total
  double ra[kRows], rb[kRows];    // rows: partial sums (abs, emi) of point wlo + col + 8 s over the lines of this lane's row
#pragma unroll
  for (int q = 0; q < kRows; ++q) ra[q] = rb[q] = 0.;
  const FastRec *frow = fast + (size_t)layer * n_sub;
  unsigned n_r1 = 0, n_we = 0; // COUNT: region-1 evaluations of this lane, window-end expansions
#ifdef SR_DIAG_WINGS
  unsigned n_diag = 0;
#endif
  for (int rg = 0; rg < 3; ++rg) {
    for (int base = rs[rg]; base < re[rg]; base += 64) {
      const int lv = base + lane;
      // lane = line: does the line have region-1 points in this slot that no far-field level owns, and are they
      // cut by the window end / start only (then it can join the expansion + scan below)
      bool need = false, fastl = false;
      bool has_l = false, has_r = false; // region-1 points of the lane's line in this slot: left wing (k < il), right wing (k > ir)
      int pos = 64; // lanes without a line: never selected by the scan
      if (lv < re[rg]) {
        const int j1 = frow[lv].j1;
        const unsigned ilir = frow[lv].ilir;
        const int il = (int)(ilir & 0xffffu), ir = (int)(ilir >> 16), jN = j1 + (kImxsig - 1);
        // cut-off position of the scan: every line of the range takes part in it (the positions are
        // non-decreasing over the lanes), lines handled elsewhere with zero coefficients
        pos = rg == 0 ? min(max(jN - wlo, -1), 64) : min(max(j1 - wlo, 0), 64);
        if (jN >= wlo && j1 <= whi && !ff_admissible(j1, il, ir, wlo, wlo + 63, thr0)) {
          has_l = max(wlo, j1) <= min(whi, j1 + il - 2); // points with 1 <= k < il
          has_r = max(wlo, j1 + ir) <= min(whi, jN);     // points with ir < k <= 13010
          need = has_l || has_r;
          if (rg != 1 && classify(j1, il, ir, wlo, whi) == 0)
            fastl = rg == 0 ? (has_r && !has_l && j1 + ir <= wlo) : (has_l && !has_r && j1 + il - 2 >= wlo + 63);
        }
      }
      if (__ballot(need) == 0) continue;
      // window ends (range 0) / starts (range 2) of this slot, when there are enough of them
      if (rg != 1) {
        const bool ends = rg == 0;
        const unsigned long long fm = __ballot(fastl);
        if (__builtin_popcountll(fm) >= 12) {
          double c[2 * kWE];
#pragma unroll
          for (int n = 0; n < 2 * kWE; ++n) c[n] = 0.;
          if (fastl) {
            const FastRec r = frow[lv];
            // -x (starts: left wing) or x (ends: right wing) at the slot centre wlo + 31.5
            const double xc = ends ? fma(0.5 * (double)(2 * (wlo - (r.j1 + r.ir() - 1)) + 63), r.xstep, r.xr)
                                   : fma(0.5 * (double)(2 * (wlo - r.j1) + 63), r.xstep, -r.xl);
            double f[kWE];
            wing_series6(xc, 32.0 * r.xstep, r, f);
            if (COUNT) ++n_we;
#pragma unroll
            for (int n = 0; n < kWE; ++n) {
              c[n] = r.wabs * f[n];
              c[kWE + n] = r.wemi * f[n];
            }
            need = false; // done here
          }
          window_end_sum(ends, pos, c, lane, sum_a, sum_e);
          if (__ballot(need) == 0) continue;
        }
      }
      // rows: region 1 is k < il (running x from k = 1: x = (k - 1) xstep - xl, i.e. -x) or k > ir
      // (x = (k - ir) xstep + xr), inside the window and the grid (lineshape.f:461-477, last writer wins).
      // A row takes one (line, wing) ITEM: the wing's points in the slot are one run of window indices
      // [k_a, k_b], so a step's lane mask is one add + one compare and x one fma from the row's x at step 0.
      // (Round 2 walked lines, with the wing chosen per point and step: 6 instructions of tests for each of the
      // 8 steps, executed or not, 17 per executed step, 27 to deal the lines to the rows and 16 unconditional
      // accumulations: 183 per round of which 80 evaluated something -- tools/diag_counts.py: 2.2e6 rounds,
      // 4.7 executed steps per round, 48 of 64 lanes on in an executed step on config 2.)
      unsigned long long m_l = __ballot(need && has_l), m_r = __ballot(need && has_r);
      while (m_l | m_r) {
        int code = -1; // this row's item: line (index into the chunk) | wing << 6; -1: none left
#pragma unroll
        for (int q = 0; q < kRows; ++q) {
          int c_ = -1; // wave-uniform
          if (m_l) {
            c_ = __builtin_ctzll(m_l);
            asm("s_bitset0_b64 %0, %1" : "+s"(m_l) : "s"(c_)); // m_l &= m_l - 1 in one scalar instruction instead of three
          } else if (m_r) {
            const int cr = __builtin_ctzll(m_r);
            asm("s_bitset0_b64 %0, %1" : "+s"(m_r) : "s"(cr));
            c_ = cr | 64;
          }
          code = row == q ? c_ : code;
        }
#ifdef SR_DIAG_WINGS // diagnostic builds only: rounds of the row walk (in the window-end counter)
        if (COUNT) n_we += 1; // summed over the 64 lanes
#endif
        const bool live = code >= 0, rw = live && (code & 64);
        const FastRec &r = frow[base + (live ? (code & 63) : 0)];
        const R1Coef rq = r1_of(r);
        const double xstep = r.xstep, a = rq.a, b = rq.b, c = rq.c, d = rq.d, wa = r.wabs, we = r.wemi;
        const int j1 = r.j1, il = r.il(), ir = r.ir();
        const int kb0 = wlo - j1 + 1 + col;              // window index of this lane's point at step 0
        const int k_last = min(kImxsig, whi - j1 + 1);  // last window index inside the slot, the grid and the window
        const int k_a = rw ? ir + 1 : 1, k_b = rw ? k_last : min(il - 1, k_last);
        const unsigned n_on = live ? (unsigned)max(k_b - k_a + 1, 0) : 0u;
        const int t0 = kb0 - k_a;                        // step q is on for this lane: (unsigned)(t0 + 8 q) < n_on
        const double x0 = fma((double)(kb0 - (rw ? ir : 1)), xstep, rw ? r.xr : -r.xl);
#pragma unroll
        for (int q = 0; q < kRows; ++q) {
          // a branch per step: steps no lane of the wave needs are skipped
          if ((unsigned)(t0 + kRowLanes * q) < n_on) {
            double x = x0;
            if (q > 0) asm("v_fma_f64 %0, %1, %2, %3" : "=v"(x) : "s"((double)(kRowLanes * q)), "v"(xstep), "v"(x0)); // one instruction
            const double x2 = x * x;
            const double y = fma(x2, b, a) * fast_rcp<1>(fma(x2, fma(x2, 4.0, d), c));
            if (COUNT) ++n_r1;
#ifdef SR_DIAG_WINGS // executed steps (in the polynomial counter)
            if (COUNT) n_diag |= 1u << q;
#endif
            ra[q] = fma(wa, y, ra[q]);
            rb[q] = fma(we, y, rb[q]);
          }
        }
#ifdef SR_DIAG_WINGS
        if (COUNT) {
          unsigned any_ = n_diag & 0xffu;
#pragma unroll
          for (int m = 32; m >= 1; m >>= 1) any_ |= (unsigned)__shfl_xor((int)any_, m);
          n_diag = (n_diag & ~0xffu) + ((unsigned)__builtin_popcount(any_) << 8);
        }
#endif
      }
    }
  }
  // totals of the rows: point wlo + lane is (col, step) = (lane % 8, lane / 8): sum over the eight rows of that step
#pragma unroll
  for (int q = 0; q < kRows; ++q) {
    double ta = ra[q], te = rb[q];
#pragma unroll
    for (int m = kRowLanes; m < 64; m <<= 1) {
      ta += __shfl_xor(ta, m);
      te += __shfl_xor(te, m);
    }
    if (row == q) {
      sum_a += ta;
      sum_e += te;
    }
  }
  if (COUNT) {
    count_add(cnt, kCntRegion1, n_r1, lane);
    count_add(cnt, kCntWindowEnds, n_we, lane);
#ifdef SR_DIAG_WINGS
    count_add(cnt, kCntPolyPoints, lane == 0 ? n_diag >> 8 : 0u, lane);
#else
    count_add(cnt, kCntPolyPoints, (wlo + lane <= whi) ? (unsigned)(fp.folded0 ? 1 : fp.n_levels) : 0u, lane);
#endif
  }
  // far field: one polynomial per level, or level 0 alone where sr_l2l_kernel has folded the wider levels into it
  const double *cl = fp.coef + (size_t)layer * fp.n_boxes_total * (2 * kFC);
  const int n_lv = fp.folded0 ? 1 : fp.n_levels;
  for (int lv = 0; lv < n_lv; ++lv) {
    const int W = 64 << lv;
    const int b = (wlo - g_lo) >> (6 + lv);
    const int blo = g_lo + b * W;
    const double t = (double)(2 * (wlo + lane - blo) - (W - 1)) * (1.0 / 64 / (double)(1 << lv)); // exact: W = 2^(6+lv)
    const double *c = cl + (size_t)(fp.box_off[lv] + b) * (2 * kFC);
    double pa = c[kFC - 1], pe = c[2 * kFC - 1];
#pragma unroll
    for (int n = kFC - 2; n >= 0; --n) {
      pa = fma3s(pa, t, c[n]);
      pe = fma3s(pe, t, c[kFC + n]);
    }
    sum_a += pa;
    sum_e += pe;
  }
  const size_t orow = (size_t)layer * (size_t)(g_hi - g_lo);
  const int j = wlo + lane;
  if (j <= whi) {
    if (z_abs) { // the zones kernel's sums sit in a buffer of their own (it runs decoupled from the caller's stream)
      abs_out[orow + (j - g_lo)] = z_abs[orow + (j - g_lo)] + sum_a;
      emi_out[orow + (j - g_lo)] = z_emi[orow + (j - g_lo)] + sum_e;
    } else if (add) { // the zones kernel ran first (overlapped with the far-field kernel) and stored its sums
      abs_out[orow + (j - g_lo)] += sum_a;
      emi_out[orow + (j - g_lo)] += sum_e;
    } else {
      abs_out[orow + (j - g_lo)] = sum_a;
      emi_out[orow + (j - g_lo)] = sum_e;
    }
  }
}

// ------------------------------------------------------------------------
// The zones walk: regions 2, 3 and 4 of the lines whose zone meets a group of grid points, summed into an LDS image
// of the group.  sr_abscoeff_near_zones_kernel and sr_zones_mc_kernel run the SAME walk, one 64-line chunk at a time
// (zones_chunk); they differ in the SINK, which says where a line's value goes:
//   kWords            words per entry of the item lists: lane, two run words and, if 4, the sink's own word
//   Chans             the planes of a line; channels(lv) reads them, pack() / unpack() are the item's fourth word
//   Line              line(r, ch, ibase): the line's weights and planes; add(k, y) adds weight * y at element
//                     k + ibase of each plane, add_at_byte(ab, y) at byte ab (ibase = 0).  Several lines can hit the
//                     same grid point in one step, hence LDS atomics
//   count(region, on) the executed-work counters
// Everything is inlined into the two kernels: nothing of it lives in memory that a kernel would hold in registers.
// ------------------------------------------------------------------------
#ifndef SR_ZONES_ROW
#define SR_ZONES_ROW 8 // lanes per row of the region-2 / region-4 walk: eight lines at a time (16: 4.35, 8: 4.1, 4: 4.87, 32: 5.09 ms)
#endif
// Largest of a value that is uniform within each row of 8 lanes, as a scalar: eight v_readlane + scalar max.  The
// row loops then run on a scalar step counter; "while any lane has a step left" costs three VALU instructions per
// step however it is written (the ballot's mask goes through v_cndmask + v_cmp_ne).
__device__ inline int rows_max(int v) {
  int m = __builtin_amdgcn_readlane(v, 0);
#pragma unroll
  for (int r = 8; r < 64; r += 8) m = max(m, __builtin_amdgcn_readlane(v, r));
  return m;
}
// What a wave's walk needs of its group: the layer's records, the group's first and last grid point, and the wave's
// item lists [2 regions][kWords][64]: per region (2, 4) the chunk's lines with work there, compacted in lane order --
// lane id, the two run words, the sink's word -- written by the lanes = lines phase, read by the rows (dealing the
// lines to the rows with ballots and selects cost 27 VALU instructions per round of eight lines, two bpermutes
// fetched the run words)
struct ZoneWalk {
  const FastRec *frow;
  const ColdRec *crow;
  const GridParams &gp;
  int *items;
  int wlo, whi, lane;
  double p6_vgpr; // see core_region4_m
};
// does the zone (inside the window) of the lane's line meet the group: from the FastRec alone
__device__ __forceinline__ bool zone_meets_group(const FastRec &r, bool in_list, int wlo, int whi) {
  const int j1 = r.j1, il = r.il(), ir = r.ir();
  const int zl = max(j1 + il - 1, j1), zh = min(j1 + ir - 1, j1 + (kImxsig - 1));
  return in_list && zl <= whi && zh >= wlo;
}
// runs of the lane's line inside this group, start | count << 16 (window indices <= 13010): region 2 left / right
// (lineshape.f:503-522), region 4 left / right of the region-3 interval; region 3 = n3 points from e0
struct ZoneRuns {
  unsigned run2l, run2r, run4l, run4r;
  int e0, n3;
  bool w2, w4; // the line has region-2 / region-4 work here
};
__device__ __forceinline__ ZoneRuns zone_runs(const FastRec &r, const ColdRec &z, bool act, int wlo, int whi) {
  ZoneRuns o;
  const int j1 = r.j1, il = r.il(), ir = r.ir();
  const int k3lo = z.k3lo(), k3hi = z.k3hi();
  const int il2 = z.il2(), ir2 = z.ir2();
  const int k_lo = max(wlo - j1 + 1, 1), k_hi = min(whi - j1 + 1, kImxsig); // group & window, as k
  {
    const int a0 = max(il, k_lo), a1 = il < il2 ? min(il2, k_hi) : a0 - 1;
    const int b0 = max(ir2, k_lo), b1 = ir2 < ir ? min(ir, k_hi) : b0 - 1;
    o.run2l = (unsigned)a0 | ((unsigned)max(a1 - a0 + 1, 0) << 16);
    o.run2r = (unsigned)b0 | ((unsigned)max(b1 - b0 + 1, 0) << 16);
  }
  // the core (il2a, ir2a), lineshape.f:524-562: region 3 = [k3lo, k3hi], region 4 on both sides
  const int c_lo = max(((il2 == il) ? il - 1 : il2) + 1, k_lo), c_hi = min(((ir2 == ir) ? ir + 1 : ir2) - 1, k_hi);
  const bool has3 = k3lo <= k3hi;
  {
    const int a0 = c_lo, a1 = has3 ? min(k3lo - 1, c_hi) : c_hi;
    const int b0 = has3 ? max(k3hi + 1, c_lo) : c_hi + 1, b1 = c_hi;
    o.run4l = (unsigned)a0 | ((unsigned)max(a1 - a0 + 1, 0) << 16);
    o.run4r = (unsigned)b0 | ((unsigned)max(b1 - b0 + 1, 0) << 16);
  }
  o.e0 = max(k3lo, c_lo);
  const int e1 = min(k3hi, c_hi);
  o.n3 = (act && has3) ? max(e1 - o.e0 + 1, 0) : 0;
  o.w2 = act && ((o.run2l >> 16) + (o.run2r >> 16)) > 0;
  o.w4 = act && ((o.run4l >> 16) + (o.run4r >> 16)) > 0;
  return o;
}
// the cosine's argument range over the line's region-4 runs (cos_tiered), for bits 30-31 of run4l (a count is
// < 2^14): |Im c1| = 2 ry rx is largest at the outer ends of the two runs
__device__ __forceinline__ unsigned zone_cos_tier(const WinX &xf, unsigned run4l, unsigned run4r, double x0, double inv_dwp,
                                                  double ryf) {
  const double rx_max = fmax(fabs(xf((int)(run4l & 0xffffu)) - x0),
                             fabs(xf((int)(run4r & 0xffffu) + (int)(run4r >> 16) - 1) - x0)) * inv_dwp * 1.001;
  const double ui_max = (ryf + ryf) * rx_max;
  return ui_max < 6.5e-3 ? 2u : (ui_max < 0.78 ? 1u : 0u);
}
// REGION 3 (lineshape.f:554-560), the ~15 points around the centre, lane = line: all lanes step through their own
// interval together (the intervals of neighbouring lines are equally long), the line's data sit in the lane's
// registers and die before the rows; sums by ds_add_f64.  Walked line by line with lanes = points these few points
// cost a whole 64-lane chunk per line (1.1 of 6.6 ms).  Leaves the cosine's tier in run4l.
template <class Sink>
__device__ __forceinline__ void zone_region3(const ZoneWalk &W, Sink &sink, const FastRec &r, const ColdRec &z, ZoneRuns &zr,
                                             const typename Sink::Chans &ch) {
  const int j1 = r.j1;
  const WinX xf{W.gp.lin_start, W.gp.lin_delta, grid_at(W.gp, j1 + kHalf)};
  const double x0 = z.x0, dwp = z.dwp, inv_dwp = cold_inv_dwp(z.dwp), ryf = cold_ryf(z.ry);
  const typename Sink::Line to = sink.line(r, ch, j1 - W.wlo); // element = point + 1
  zr.run4l |= zone_cos_tier(xf, zr.run4l, zr.run4r, x0, inv_dwp, ryf) << 30;
  const int e0 = zr.e0, n3 = zr.n3;
  for (int t = 0; __any(t < n3); ++t) {
    if (t < n3) {
      const int k = e0 + t;
      const double d = fabs(xf(k) - x0);
      double rx = d * inv_dwp; // |x(k)-x0|/dw correctly rounded: one residual correction
      rx = fma(fma(-dwp, rx, d), inv_dwp, rx);
      const double y = core_region3(ryf, (double)(float)(-rx));
      sink.count(3, true);
      to.add(k, y);
    }
  }
}
// the lines with work in a region (0: region 2, 1: region 4), compacted in lane order; returns their number
template <class Sink>
__device__ __forceinline__ int zone_compact(const ZoneWalk &W, int region, bool w, unsigned run_l, unsigned run_r, int word) {
  const unsigned long long m = __ballot(w);
  if (w) {
    const int at = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
    int *const it = W.items + region * Sink::kWords * 64 + at;
    it[0] = W.lane;
    it[64] = (int)run_l;
    it[128] = (int)run_r;
    if (Sink::kWords > 3) it[192] = word;
  }
  return __builtin_popcountll(m);
}
// ---- regions 2 and 4, kZoneRows lines at a time: each row of kZoneRowLanes lanes walks the points of ONE line,
// kZoneRowLanes per step, with the line's data in its own registers (per-lane loads of the record fields: the four
// rows read four records).  History: one line at a time with 64 points per step left the last chunk of each
// run mostly empty (a line has ~150 region-2 and ~72 region-4 points: 64 + 64 + 22 lanes, 71-78 % lane use)
// and cost a scalar record fetch + ~40 scalar / vector instructions per line; packing region-4 points of
// consecutive lines into full chunks fixed its lane use but not the per-line walk.  Rows: lane use 90-94 %, no
// scalar walk, no pending state: sr_abscoeff_near_zones_kernel 4.9 -> 4.2 ms on config 2.
constexpr int kZoneRowLanes = SR_ZONES_ROW, kZoneRows = 64 / kZoneRowLanes;
// the item of this lane's row in round g of a region's list (the last item again, not live, where the list ends)
struct ZoneItem {
  bool live;
  int line; // lane of the line in the chunk
  unsigned ul, ur;
  int word;
};
template <class Sink>
__device__ __forceinline__ ZoneItem zone_item(const ZoneWalk &W, int region, int g, int n_items) {
  const int row = W.lane / kZoneRowLanes;
  const int *const it = W.items + region * Sink::kWords * 64 + min(g + row, n_items - 1);
  return {g + row < n_items, it[0], (unsigned)it[64], (unsigned)it[128], Sink::kWords > 3 ? it[192] : 0};
}
// region 2 (lineshape.f:503-522): item t of a line: left k = a0 + t, x = xs2l - (k - il) xstep; right
// k = b0 + (t - na), x = xs2r + (k - ir2) xstep.  Only x^2 enters, so both are t xstep + c with a per-line c.
template <class Sink>
__device__ __forceinline__ void zone_rows2(const ZoneWalk &W, Sink &sink, int base, int n_items) {
  const int col = W.lane % kZoneRowLanes;
  for (int g = 0; g < n_items; g += kZoneRows) {
    const ZoneItem I = zone_item<Sink>(W, 0, g, n_items);
    const FastRec &r = W.frow[base + I.line];
    const ColdRec &z = W.crow[base + I.line];
    const int a0 = (int)(I.ul & 0xffffu), na = (int)(I.ul >> 16), b0 = (int)(I.ur & 0xffffu), nb = (int)(I.ur >> 16);
    const double xstep = r.xstep;
    const typename Sink::Line to = sink.line(r, Sink::Chans::unpack(I.word), 0);
    double q2[8];
    region2_coef_fma(z.ry, q2); // rebuilt per line (ColdRec): 25 flops against ~20 steps of 21 instructions
    const int base_idx = r.j1 - W.wlo; // element = point + 1
    // the two runs one after the other, t counted from each run's first point (one loop over both with the
    // side chosen per point cost a compare and three selects per point: 25 -> 21 VALU instructions per point
    // for ~5 % more steps)
    auto run = [&](const int n, const int n_max, const double c, const int i0) {
      const int n_steps = (n_max + kZoneRowLanes - 1) / kZoneRowLanes; // wave-uniform: a scalar loop counter
      // x of the lane's point by a running sum, eight steps of xstep at a time (one add instead of a conversion
      // and an fma per point; <= 20 steps of a run: <= 20 ulp of x, 1e-14 of the value at most): 5.38 vs 5.42 ms
      // per headline step
      double xt = fma((double)col, xstep, c);
      const double xs8 = (double)kZoneRowLanes * xstep;
      // ... and ONE counter per lane: the byte offset of its point in the image, which is the loop's predicate too
      int ab = (col + i0) * 8;
      const int ab_end = (n + i0) * 8;
      for (int st = 0; st < n_steps; ++st, ab += 8 * kZoneRowLanes) {
        if (ab < ab_end) {
          const double y = region2_val(q2, xt);
          xt += xs8;
          sink.count(2, true);
          to.add_at_byte(ab, y); // return-less LDS adds: no wait for a read, runs of different lines overlap
        }
      }
    };
    // (step counts by rows_max() per round; from per-round maxima that the lanes = lines phase wrote to LDS: 3.51 vs 3.50 ms, 128-129 VGPRs)
    run(I.live ? na : 0, rows_max(I.live ? na : 0), fma((double)(a0 - r.il()), xstep, -z.xs2l), a0 + base_idx);
    run(I.live ? nb : 0, rows_max(I.live ? nb : 0), fma((double)(b0 - z.ir2()), xstep, z.xs2r), b0 + base_idx);
  }
}
// region 4 (lineshape.f:530-546), on both sides of the region-3 interval
template <class Sink>
__device__ __forceinline__ void zone_rows4(const ZoneWalk &W, Sink &sink, int base, int n_items) {
  const int col = W.lane % kZoneRowLanes;
  for (int g = 0; g < n_items; g += kZoneRows) {
    const ZoneItem I = zone_item<Sink>(W, 1, g, n_items);
    const FastRec &r = W.frow[base + I.line];
    const ColdRec &z = W.crow[base + I.line];
    const unsigned ul = I.ul, ur = I.ur;
    const int a0 = (int)(ul & 0xffffu), na = (int)((ul >> 16) & 0x3fffu), b0 = (int)(ur & 0xffffu), nb = (int)(ur >> 16);
    const int n = I.live ? na + nb : 0;
    const int j1 = r.j1;
    const double gc = grid_at(W.gp, j1 + kHalf), x0 = z.x0, dwp = z.dwp, inv_dwp = cold_inv_dwp(z.dwp);
    const double ryf = cold_ryf(z.ry), ryf2 = ryf * ryf, two_ryf = ryf + ryf;
    const typename Sink::Line to = sink.line(r, Sink::Chans::unpack(I.word), j1 - W.wlo); // element = point + 1
    // the cosine's tier of this round: the smallest of its lines' (from the lanes = lines phase; cos_tiered)
    const int tier_ = I.live ? (int)(ul >> 30) : 2;
    const int cos_tier = __all(tier_ == 2) ? 2 : (__all(tier_ >= 1) ? 1 : 0);
    const int n_steps = (rows_max(n) + kZoneRowLanes - 1) / kZoneRowLanes;
    const WinX xf{W.gp.lin_start, W.gp.lin_delta, gc};
    for (int st = 0; st < n_steps; ++st) {
      const int t = col + kZoneRowLanes * st;
      const int k = t < na ? a0 + t : b0 + (t - na);
      sink.count(4, t < n);
      if (t < n) {
        const double d = fabs(xf(k) - x0);
        double rx = d * inv_dwp; // |x(k)-x0|/dw correctly rounded: one residual correction
        rx = fma(fma(-dwp, rx, d), inv_dwp, rx);
        const double y = core_region4_m(ryf, ryf2, two_ryf, (double)(float)rx, cos_tier, W.p6_vgpr);
        to.add(k, y);
      }
    }
  }
}
// One 64-line chunk from record `base` of a list that ends before l1: lane = line for the interval arithmetic of
// every line (the rows read it back from the item lists: done there it was ~70 scalar instructions per line) and
// region 3, then the rows.
template <class Sink>
__device__ __forceinline__ void zones_chunk(const ZoneWalk &W, Sink &sink, int base, int l1) {
  const int lv = min(base + W.lane, l1 - 1);
  const FastRec &r = W.frow[lv];
  const bool act = zone_meets_group(r, base + W.lane < l1, W.wlo, W.whi);
  if (__ballot(act) == 0) return; // before the first ColdRec load
  const ColdRec &z = W.crow[lv];
  ZoneRuns zr = zone_runs(r, z, act, W.wlo, W.whi);
  const typename Sink::Chans ch = sink.channels(lv);
  if (__any(zr.n3 > 0 || zr.w4)) zone_region3(W, sink, r, z, zr, ch);
  const int n_items2 = zone_compact<Sink>(W, 0, zr.w2, zr.run2l, zr.run2r, ch.pack());
  const int n_items4 = zone_compact<Sink>(W, 1, zr.w4, zr.run4l, zr.run4r, ch.pack());
  zone_rows2(W, sink, base, n_items2);
  zone_rows4(W, sink, base, n_items4);
}

// The folded op's sink: two sums, wabs and wemi, into the wave's private image (one wave per image, program order:
// the sums stay deterministic), and the COUNT counters.
template <bool COUNT>
struct FoldedSink {
  static constexpr int kWords = 3;
  double *s_a, *s_e;
  unsigned n_r[3]; // COUNT: evaluations of this lane in regions 2, 3, 4
  struct Chans {
    __device__ __forceinline__ int pack() const { return 0; }
    static __device__ __forceinline__ Chans unpack(int) { return {}; }
  };
  struct Line {
    double *s_a, *s_e;
    double wa, we;
    int ibase;
    __device__ __forceinline__ void add(int k, double y) const {
      atomicAdd(&s_a[k + ibase], wa * y);
      atomicAdd(&s_e[k + ibase], we * y);
    }
    __device__ __forceinline__ void add_at_byte(int ab, double y) const {
      atomicAdd(reinterpret_cast<double *>(reinterpret_cast<char *>(s_a) + ab), wa * y);
      atomicAdd(reinterpret_cast<double *>(reinterpret_cast<char *>(s_e) + ab), we * y);
    }
  };
  __device__ __forceinline__ Chans channels(int) const { return {}; }
  __device__ __forceinline__ Line line(const FastRec &r, Chans, int ibase) const { return {s_a, s_e, r.wabs, r.wemi, ibase}; }
  __device__ __forceinline__ void count(int region, bool on) {
    if (COUNT) n_r[region - 2] += on;
  }
};
// WT points per wave (a multiple of 64): the wider the image, the fewer zones are cut in two by
// its ends (a zone is ~280 points), i.e. the fewer partially filled lane runs.
// At least four waves per SIMD (<= 128 VGPRs): the kernel sits at 118-127; with 129 (one more feature in the rows)
// the 8-wave blocks of a small shard went from two per CU to one and the shard's kernel from 0.50 to 0.63 ms.
template <int WT, int NW, bool COUNT>
__global__ __launch_bounds__(64 * NW) __attribute__((amdgpu_waves_per_eu(4))) void sr_abscoeff_near_zones_kernel(
    const FastRec *__restrict__ fast, const ColdRec *__restrict__ cold, IcIndex ix,
    const int *__restrict__ zmax, int n_sub, int n_groups, int g_lo, int g_hi, GridParams gp, int add,
    double *__restrict__ abs_out, double *__restrict__ emi_out, unsigned long long *__restrict__ cnt, int layer0) {
  // one private image per wave: abs, emi.  Point p of the group (window index k of a line: p = k + j1 - 1 - wlo) lives at
  // element p + 1, i.e. element k + (j1 - wlo): the hot loops' address arithmetic carries no "- 1" (it cost a v_add per
  // region-2 point: the offset field of ds_add cannot be negative)
  __shared__ double s_img[NW][2][WT + 2];
  __shared__ int s_item[NW][2][3][64]; // the waves' item lists (ZoneWalk)
  const int wg = xcd_remap(blockIdx.x, gridDim.x);
  const int layer = layer0 + wg / n_groups, grp = wg - (layer - layer0) * n_groups; // layer0: the launch's first layer (layer chunks)
  const int wlo = g_lo + grp * WT;
  const int whi = min(wlo + WT, g_hi) - 1;
  // NW waves work on the same group and take its 64-line chunks in turn, each into its own image
  // (added up in wave order at the end: the result does not depend on timing).  For small shards,
  // where one wave per 512-point image leaves wave slots empty and 256-point images cut more zones.
  const int lane = NW == 1 ? threadIdx.x : threadIdx.x & 63, wave = NW == 1 ? 0 : threadIdx.x >> 6;
  double *const s_a = s_img[wave][0], *const s_e = s_img[wave][1];
  const int zm = min(zmax[layer], kHalf - 1);
#pragma unroll
  for (int p = 0; p < WT / 64; ++p) s_a[1 + lane + 64 * p] = s_e[1 + lane + 64 * p] = 0.;
  FoldedSink<COUNT> sink{s_a, s_e, {0, 0, 0}};
  const double p6_vgpr = vgpr_constant(SR_F32(.56419)); // see core_region4_m
  // lines whose zone [ic - zm, ic + zm] can meet the group
  const int l0 = lower_bound_ic(ix, wlo - zm), l1 = lower_bound_ic(ix, whi + zm + 1);
  const FastRec *frow = fast + (size_t)layer * n_sub;
  const ColdRec *crow = cold + (size_t)layer * n_sub;
  // Serpentine sweep: even groups take their 64-line chunks left to right, odd groups right to left.  Neighbouring
  // groups (consecutive work ids, same XCD, started together) share the lines within the zone width of their common
  // edge -- 45 % more record bytes than the tables hold; swept in opposite directions both reach the shared lines at
  // the same time (start or end of their sweep) and the second one finds them in L2 instead of HBM.
  const int n_chunks = (l1 - l0 + 63) >> 6;
  const ZoneWalk W{frow, crow, gp, &s_item[wave][0][0][0], wlo, whi, lane, p6_vgpr};
  for (int ci = wave; ci < n_chunks; ci += NW) zones_chunk(W, sink, l0 + 64 * ((grp & 1) ? n_chunks - 1 - ci : ci), l1);
  if (COUNT) {
    count_add(cnt, kCntRegion2, sink.n_r[0], lane);
    count_add(cnt, kCntRegion3, sink.n_r[1], lane);
    count_add(cnt, kCntRegion4, sink.n_r[2], lane);
  }
  if (NW > 1) __syncthreads();
  const size_t row = (size_t)layer * (size_t)(g_hi - g_lo);
  for (int p = threadIdx.x; p < WT; p += 64 * NW) {
    const int j = wlo + p;
    if (j <= whi) {
      double ta = s_img[0][0][p + 1], te = s_img[0][1][p + 1];
#pragma unroll
      for (int w = 1; w < NW; ++w) {
        ta += s_img[w][0][p + 1];
        te += s_img[w][1][p + 1];
      }
      if (add) {
        abs_out[row + (j - g_lo)] += ta;
        emi_out[row + (j - g_lo)] += te;
      } else {
        abs_out[row + (j - g_lo)] = ta;
        emi_out[row + (j - g_lo)] = te;
      }
    }
  }
}


// ------------------------------------------------------------------------
// The multi-channel pass (level pair tables, G-coefficient tables): every line ONCE, each of its three weighted
// contributions to the spectrum of the level it belongs to.
//
// The per-level route evaluates every line twice (in its upper level's pass and in its lower level's) and pays the
// fixed cost of a (slot, layer) wave twelve times -- a 9 %-of-the-lines pass cost 1.08 ms where its lines' share of a
// full pass is 0.48 (3.1-3.4 coefficient-op equivalents for twelve levels).  Here the near-field
// kernels walk the FULL sorted list once, exactly as the folded op does, and the accumulation goes to an LDS image
// with one plane per output spectrum: wabs -> plane (lev_lo, o_lo), wemi -> (lev_up, o_up_e), w3 -> (lev_up, o_up_a)
// (McChannels).  An image of n_ch x 256 points is shared by the NW waves of a workgroup (return-less ds_add_f64 from
// all of them: the sums' order of addition depends on timing at the 1e-16 level, unlike the one-wave images of the folded op).
// The far field stays per level (its translations and polynomials are linear per output spectrum anyway): far-only
// passes of the level sub-linesets leave their coefficients for sr_wings_mc_kernel's polynomial stage.
// ------------------------------------------------------------------------
// ------------------------------------------------------------------------
// Local-to-local translation (the downward pass of the hierarchy).  A box's local expansion IS a polynomial of degree
// kFD over the box, so its restriction to a child box is the same polynomial re-centred: with t_parent = s/2 + t_child/2
// (s = -1 left, +1 right child)  child_n += sum_{m >= n} 2^-m C(m, n) s^(m-n) parent_m  -- exact algebra, no truncation,
// operator entries exact in fp64 (an integer below 2^53 times a power of two).  After it the level-0 coefficients hold
// every level's far field and a point evaluates ONE polynomial per output instead of one per hierarchy level.  For the
// multi-channel pass (n_far x 2 outputs per point: 5 x 12 x 2 Horner chains of 22 fma per point were 2.3 of
// sr_wings_mc_kernel's 5.2 ms) and for the folded op in the box-pair mode (FarParams::folded0: 152 fma and four batches of
// scalar coefficient loads less per wave of the near-wings kernel, -6 % of its instructions; this kernel runs behind M2L,
// beside the zones kernel).  The per-line mode of sparse sets keeps one polynomial per level.
// One wave per (layer, widest box) of a far pass: the box's tree of 31 coefficient sets in LDS, levels top down.
// ------------------------------------------------------------------------
__global__ __launch_bounds__(64) void sr_l2l_kernel(double *__restrict__ coef_one, const FarBatchItem *__restrict__ items, FarParams fp,
                                                    const double *__restrict__ tab) {
  double *const coef = items ? items[blockIdx.z].coef : coef_one; // one pass, or item blockIdx.z of a batch
  constexpr int kBlk = 2 * kFC, kTop = kMaxFarLevels - 1;
  constexpr int kTree = (2 << kTop) - 1; // boxes of the tree under one widest box: 1 + 2 + ... + 2^kTop
  __shared__ double s_c[kTree * kBlk];
  const int layer = blockIdx.y, top = blockIdx.x, lane = threadIdx.x;
  double *cl = coef + (size_t)layer * fp.n_boxes_total * kBlk;
  const int lq = min(lane, kBlk - 1), ch = lq / kFC, n = lq - ch * kFC; // lanes 0 .. 2 kFC - 1: (output, coefficient)
  // this lane's two operator rows in registers (zeros left of the diagonal: the inner loop needs no bounds); in LDS the
  // 8.5 KB table held a CU to eight of these waves (first build: 2.2 ms for 0.3 ms of work)
  double T0[kFC], T1[kFC];
#pragma unroll
  for (int m = 0; m < kFC; ++m) {
    T0[m] = tab[(size_t)n * kFC + m];
    T1[m] = tab[((size_t)kFC + n) * kFC + m];
  }
  // tree slot of box j (0-based within this top box) of level lv: the levels stored widest first
  auto slot = [&](int lv, int j) { return ((1 << (kTop - lv)) - 1) + j; };
  for (int lv = kTop; lv >= 0; --lv) {
    const int nb = 1 << (kTop - lv);
    for (int j = 0; j < nb; ++j) {
      const int b = top * nb + j;
      if (lane < kBlk) s_c[slot(lv, j) * kBlk + lane] = b < fp.box_count[lv] ? cl[(size_t)(fp.box_off[lv] + b) * kBlk + lane] : 0.0;
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  for (int lv = kTop; lv >= 1; --lv) {
    const int nb = 1 << (kTop - lv);
    for (int j = 0; j < nb; ++j) {
      const double *par = s_c + slot(lv, j) * kBlk + ch * kFC;
      double *c0 = s_c + slot(lv - 1, 2 * j) * kBlk + lq, *c1 = c0 + kBlk;
      double a0 = *c0, a1 = *c1;
#pragma unroll
      for (int m = 0; m < kFC; ++m) {
        const double pm = par[m];
        a0 = fma(T0[m], pm, a0);
        a1 = fma(T1[m], pm, a1);
      }
      if (lane < kBlk) {
        *c0 = a0;
        *c1 = a1;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
  const int nb0 = 1 << kTop;
  for (int j = 0; j < nb0; ++j) {
    const int b = top * nb0 + j;
    if (lane < kBlk && b < fp.box_count[0]) cl[(size_t)(fp.box_off[0] + b) * kBlk + lane] = s_c[slot(0, j) * kBlk + lane];
  }
}
void l2l_table_host(double *tab) { // [2: left, right child][n][m]
  for (int sg = 0; sg < 2; ++sg)
    for (int n = 0; n < kFC; ++n)
      for (int m = 0; m < kFC; ++m) {
        long double v = 0.0L;
        if (m >= n) {
          v = 1.0L;
          for (int k = 1; k <= n; ++k) v = v * (long double)(m - n + k) / (long double)k; // C(m, n)
          for (int k = 0; k < m; ++k) v *= 0.5L;
          if (sg == 0 && ((m - n) & 1)) v = -v;
        }
        tab[((size_t)sg * kFC + n) * kFC + m] = (double)v;
      }
}
int launch_l2l(double *coef, int n_layers, const FarParams &fp, const double *tab, hipStream_t st) {
  if (n_layers <= 0) return 0;
  hipLaunchKernelGGL(sr_l2l_kernel, dim3((unsigned)fp.box_count[kMaxFarLevels - 1], (unsigned)n_layers), dim3(64), 0, st, coef,
                     (const FarBatchItem *)nullptr, fp, tab);
  return (int)hipGetLastError();
}
// tables, per-line expansions at every level and the downward pass of n_items sparse far-only passes, three launches
int launch_far_batch(const FarBatchItem *items, int n_items, int max_n_sub, const LayersDev &A, const GridParams &gp, const int *zmax,
                     int g_lo, const FarParams &fp, const double *l2l_tab, hipStream_t st) {
  if (n_items <= 0 || A.n_layers <= 0 || max_n_sub <= 0) return 0;
  hipLaunchKernelGGL(sr_prep_batch_kernel, dim3((unsigned)((max_n_sub + kPrepBlock - 1) / kPrepBlock), (unsigned)A.n_layers, (unsigned)n_items),
                     dim3(kPrepBlock), 0, st, items, A, gp);
  const unsigned gx = (unsigned)(fp.n_boxes_total * ((A.n_layers + kFarRows - 1) / kFarRows));
  hipLaunchKernelGGL(sr_farfield_rows_batch_kernel, dim3((gx + kRowsBatchWaves - 1) / kRowsBatchWaves, (unsigned)n_items), dim3(64 * kRowsBatchWaves), 0,
                     st, items, zmax, g_lo, fp, (int)gx);
  hipLaunchKernelGGL(sr_l2l_kernel, dim3((unsigned)fp.box_count[kMaxFarLevels - 1], (unsigned)A.n_layers, (unsigned)n_items), dim3(64), 0, st,
                     (double *)nullptr, items, fp, l2l_tab);
  return (int)hipGetLastError();
}

__device__ inline int mc_base(const McChannels &mc, int level, int off, int plane) { return (mc.stride * level + off) * plane; }

// The two stages of a 64-point slot's near wings (sr_wings_mc_kernel):
// img = plane 0 at the slot's first point, `plane` doubles between planes; the slot's n_waves waves (this one: `wave`) take
// its candidate chunks and far passes in turn.
__device__ __forceinline__ void wings_mc_rows(const FastRec *__restrict__ frow, const int *__restrict__ lev_up,
                                              const int *__restrict__ lev_lo, const IcIndex &ix, const int zm_near, const int wlo,
                                              const int whi, const int thr0, const McChannels &mc, double *const img,
                                              const int plane, const int lane, const int wave, const int n_waves) {
  int rs[3], re[3];
  near_ranges(ix, wlo, 64, zm_near, rs, re);
  constexpr int kRowLanes = 8, kRows = 8;
  const int row = lane / kRowLanes, col = lane % kRowLanes;
  int turn = 0; // chunks of all three ranges dealt to the waves in turn
  for (int rg = 0; rg < 3; ++rg) {
    for (int base = rs[rg]; base < re[rg]; base += 64) {
      if ((turn++) % n_waves != wave) continue;
      const int lv = base + lane;
      bool has_l = false, has_r = false; // region-1 points of the lane's line in this slot that no far-field level owns
      if (lv < re[rg]) {
        const int j1 = frow[lv].j1;
        const unsigned ilir = frow[lv].ilir;
        const int il = (int)(ilir & 0xffffu), ir = (int)(ilir >> 16), jN = j1 + (kImxsig - 1);
        if (jN >= wlo && j1 <= whi && !ff_admissible(j1, il, ir, wlo, wlo + 63, thr0)) {
          has_l = max(wlo, j1) <= min(whi, j1 + il - 2); // points with 1 <= k < il
          has_r = max(wlo, j1 + ir) <= min(whi, jN);     // points with ir < k <= 13010
        }
      }
      unsigned long long m_l = __ballot(has_l), m_r = __ballot(has_r);
      while (m_l | m_r) {
        int code = -1; // this row's item: line (index into the chunk) | wing << 6; -1: none left
#pragma unroll
        for (int q = 0; q < kRows; ++q) {
          int c_ = -1; // wave-uniform
          if (m_l) {
            c_ = __builtin_ctzll(m_l);
            asm("s_bitset0_b64 %0, %1" : "+s"(m_l) : "s"(c_));
          } else if (m_r) {
            const int cr = __builtin_ctzll(m_r);
            asm("s_bitset0_b64 %0, %1" : "+s"(m_r) : "s"(cr));
            c_ = cr | 64;
          }
          code = row == q ? c_ : code;
        }
        const bool live = code >= 0, rw = live && (code & 64);
        const int li = base + (live ? (code & 63) : 0);
        const FastRec &r = frow[li];
        const R1Coef rq = r1_of(r);
        const double xstep = r.xstep, a = rq.a, b = rq.b, c = rq.c, d = rq.d, wa = r.wabs, we = r.wemi, w3 = r.w3;
        const int j1 = r.j1, il = r.il(), ir = r.ir();
        const int lu = lev_up[li], ll = lev_lo[li];
        double *const p_lo = img + (mc.stride * ll + mc.o_lo) * plane + col, *const p_ue = img + (mc.stride * lu + mc.o_up_e) * plane + col,
                     *const p_ua = img + (mc.stride * lu + mc.o_up_a) * plane + col;
        const int kb0 = wlo - j1 + 1 + col;              // window index of this lane's point at step 0
        const int k_last = min(kImxsig, whi - j1 + 1);  // last window index inside the slot, the grid and the window
        const int k_a = rw ? ir + 1 : 1, k_b = rw ? k_last : min(il - 1, k_last);
        const unsigned n_on = live ? (unsigned)max(k_b - k_a + 1, 0) : 0u;
        const int t0 = kb0 - k_a;                        // step q is on for this lane: (unsigned)(t0 + 8 q) < n_on
        const double x0 = fma((double)(kb0 - (rw ? ir : 1)), xstep, rw ? r.xr : -r.xl);
        // (The rows take the slot's eight 8-point groups in lockstep -- row r and row r' add to the same eight doubles of a
        // plane when their lines share a level, as most do with the ground state.  Taking them in ROTATED order, row r at
        // group (q + r) mod 8, removes that same-address conflict: built -- a table build 13.02 (lockstep) vs 13.17 ms (rotated), three
        // alternating runs: the three more integer instructions per step cost more than the conflicts.)
#pragma unroll
        for (int q = 0; q < kRows; ++q) {
          if ((unsigned)(t0 + kRowLanes * q) < n_on) {
            double x = x0;
            if (q > 0) asm("v_fma_f64 %0, %1, %2, %3" : "=v"(x) : "s"((double)(kRowLanes * q)), "v"(xstep), "v"(x0));
            const double x2 = x * x;
            const double y = fma(x2, b, a) * fast_rcp<1>(fma(x2, fma(x2, 4.0, d), c));
            atomicAdd(&p_lo[kRowLanes * q], wa * y); // return-less LDS adds: rows of different lines may hit the same point
            atomicAdd(&p_ue[kRowLanes * q], we * y);
            atomicAdd(&p_ua[kRowLanes * q], w3 * y);
          }
        }
      }
    }
  }
  // far field: one polynomial per (far pass, hierarchy level), added to the pass's two planes at this lane's point.
  // The coefficients of a pass -- kMaxFarLevels x 2 kFC doubles, one block per hierarchy level -- come in by four
  // coalesced vector loads (lane = coefficient), go through an LDS staging row and are read back as broadcasts; the next
  // pass's loads are in flight while this one is evaluated.  (Round 6, first build: wave-uniform scalar loads, one
  // (pass, level) block of 92 SGPRs at a time, each waited for before its 44 fma -- 60 dependent round trips per wave
  // and most of the kernel's 4.9 ms.)
}
__device__ __forceinline__ void wings_mc_polys(const McFarPass *__restrict__ far, const int n_far, const FarParams &fp, const int layer,
                                               const int g_lo, const int wlo, double *const img, const int plane,
                                               double *const s_cf, const int lane, const int wave, const int n_waves) {
  {
    constexpr int kEvalLevels = 1; // sr_l2l_kernel has folded the wider levels into level 0
    constexpr int kBlk = 2 * kFC, kTot = kEvalLevels * kBlk;
    constexpr int kLoads = (kTot + 63) / 64; // loads per lane that cover a pass
    // s_cf: [64 kLoads] staging row of this wave
    double tt[kMaxFarLevels];
    int cidx[kLoads]; // element of the pass's coefficient table this lane fetches in load j (-1: none)
#pragma unroll
    for (int lv = 0; lv < kMaxFarLevels; ++lv) {
      const int W = 64 << lv;
      const int blo = g_lo + ((wlo - g_lo) >> (6 + lv)) * W;
      tt[lv] = (double)(2 * (wlo + lane - blo) - (W - 1)) * (1.0 / 64 / (double)(1 << lv)); // exact: W = 2^(6+lv)
    }
#pragma unroll
    for (int q = 0; q < kLoads; ++q) {
      const int e = lane + 64 * q, lv = e / kBlk;
      cidx[q] = e < kTot ? (fp.box_off[min(lv, kMaxFarLevels - 1)] + ((wlo - g_lo) >> (6 + lv))) * kBlk + (e - lv * kBlk) : -1;
    }
    const size_t lrow = (size_t)layer * fp.n_boxes_total * kBlk;
    auto next_pass = [&](int f) { // first pass >= f of this wave (passes f = wave, wave + kMcWingWaves, ...) with coefficients
      while (f < n_far && !far[f].coef) f += n_waves;
      return f;
    };
    double reg[kLoads];
    auto fetch = [&](int f) {
      const double *cl = far[f].coef + lrow;
#pragma unroll
      for (int q = 0; q < kLoads; ++q) reg[q] = cidx[q] >= 0 ? cl[cidx[q]] : 0.0;
    };
    int f = next_pass(wave);
    if (f < n_far) fetch(f);
    while (f < n_far) {
      __builtin_amdgcn_wave_barrier(); // (the previous pass's broadcast reads are done: LDS is in order per wave)
#pragma unroll
      for (int q = 0; q < kLoads; ++q) s_cf[lane + 64 * q] = reg[q];
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      const int ch_a = far[f].ch_a, ch_e = far[f].ch_e;
      const int fn = next_pass(f + n_waves);
      if (fn < n_far) fetch(fn);
      // one Horner chain (kFC broadcast reads, then kFC - 1 fma) at a time: unrolled over levels and outputs the
      // compiler hoisted all 230 reads of a pass (256 VGPRs, or 171 spills at 128)
      double sa = 0., se = 0.;
#pragma unroll 1
      for (int h = 0; h < 2 * kEvalLevels; ++h) {
        const int lv = h >> 1;
        const double *c = s_cf + h * kFC; // block lv: [abs kFC | emi kFC]
        double t = tt[0];
#pragma unroll
        for (int q = 1; q < kMaxFarLevels; ++q) t = lv == q ? tt[q] : t;
        double cv[kFC];
#pragma unroll
        for (int n = 0; n < kFC; ++n) cv[n] = c[n];
        double pv = cv[kFC - 1];
#pragma unroll
        for (int n = kFC - 2; n >= 0; --n) pv = fma(pv, t, cv[n]);
        if (h & 1) se += pv; else sa += pv;
      }
      if (ch_a >= 0) img[ch_a * plane + lane] += sa;
      if (ch_e >= 0) img[ch_e * plane + lane] += se;
      f = fn;
    }
  }
}

// (Round 6 also built this kernel FUSED with the near wings and the polynomials -- wings_mc_rows / wings_mc_polys on the
// same image, two waves per 64-point slot, the tables stored once instead of stored, read and stored again: 13.5 vs 13.1
// ms per build of the pair tables, 24.0 vs 21.5 for the three ctypes.  The wings stages ran at this kernel's 16 waves per
// CU instead of their own 24, behind barriers, and the zones part no longer ran beside the far passes.  Removed.)
// The multi-channel sink: three sums, wabs, wemi and w3, into the planes of the line's levels (McChannels) in an image
// [n_ch][kPlane] that the workgroup's waves share; the planes' indices travel in the item's fourth word, 3 x 10 bits.
template <int kPlane>
struct McSink {
  static constexpr int kWords = 4;
  double *s_img;
  const int *lev_up, *lev_lo;
  const McChannels &mc;
  struct Chans {
    int lo, ue, ua;
    __device__ __forceinline__ int pack() const { return lo | (ue << 10) | (ua << 20); }
    static __device__ __forceinline__ Chans unpack(int w) { return {w & 0x3ff, (w >> 10) & 0x3ff, w >> 20}; }
  };
  struct Line {
    double *s_img;
    Chans ch;
    double wa, we, w3;
    int ibase;
    __device__ __forceinline__ void add(int k, double y) const {
      double *const p_lo = s_img + ch.lo * kPlane + ibase, *const p_ue = s_img + ch.ue * kPlane + ibase,
                   *const p_ua = s_img + ch.ua * kPlane + ibase;
      atomicAdd(&p_lo[k], wa * y);
      atomicAdd(&p_ue[k], we * y);
      atomicAdd(&p_ua[k], w3 * y);
    }
    __device__ __forceinline__ void add_at_byte(int ab, double y) const {
      // byte offsets of the line's second and third plane relative to its first
      const int d_ue = (ch.ue - ch.lo) * (kPlane * 8), d_ua = (ch.ua - ch.lo) * (kPlane * 8);
      char *const plane0 = reinterpret_cast<char *>(s_img + ch.lo * kPlane);
      atomicAdd(reinterpret_cast<double *>(plane0 + ab), wa * y);
      atomicAdd(reinterpret_cast<double *>(plane0 + ab + d_ue), we * y);
      atomicAdd(reinterpret_cast<double *>(plane0 + ab + d_ua), w3 * y);
    }
  };
  __device__ __forceinline__ Chans channels(int lv) const {
    const int lu = lev_up[lv], ll = lev_lo[lv];
    return {mc.stride * ll + mc.o_lo, mc.stride * lu + mc.o_up_e, mc.stride * lu + mc.o_up_a};
  }
  __device__ __forceinline__ Line line(const FastRec &r, const Chans &ch, int ibase) const {
    return {s_img, ch, r.wabs, r.wemi, r.w3, ibase};
  }
  __device__ __forceinline__ void count(int, bool) {}
};
template <int WT, int NW>
__global__ __launch_bounds__(64 * NW) __attribute__((amdgpu_waves_per_eu(4))) void sr_zones_mc_kernel(
    const FastRec *__restrict__ fast, const ColdRec *__restrict__ cold, const int *__restrict__ lev_up,
    const int *__restrict__ lev_lo, IcIndex ix, const int *__restrict__ zmax, int n_sub, int n_groups, int g_lo, int g_hi,
    GridParams gp, McChannels mc, double *__restrict__ out, int n_rows_total, int row0) {
  extern __shared__ double s_dyn[];
  constexpr int kPlane = WT + 2;             // point p of the group lives at element p + 1 of its plane
  double *const s_img = s_dyn;               // [n_ch][kPlane]
  int *const s_item_all = reinterpret_cast<int *>(s_dyn + (size_t)mc.n_ch * kPlane); // [NW][2][4][64]: the waves' item lists (ZoneWalk)
  const int wg = xcd_remap(blockIdx.x, gridDim.x);
  const int layer = wg / n_groups, grp = wg - layer * n_groups;
  const int wlo = g_lo + grp * WT;
  const int whi = min(wlo + WT, g_hi) - 1;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int zm = min(zmax[layer], kHalf - 1);
  for (int e = threadIdx.x; e < mc.n_ch * kPlane; e += 64 * NW) s_img[e] = 0.;
  __syncthreads();
  const double p6_vgpr = vgpr_constant(SR_F32(.56419)); // see core_region4_m
  const int l0 = lower_bound_ic(ix, wlo - zm), l1 = lower_bound_ic(ix, whi + zm + 1);
  const FastRec *frow = fast + (size_t)layer * n_sub;
  const ColdRec *crow = cold + (size_t)layer * n_sub;
  const int n_chunks = (l1 - l0 + 63) >> 6;
  McSink<kPlane> sink{s_img, lev_up, lev_lo, mc};
  const ZoneWalk W{frow, crow, gp, s_item_all + wave * (2 * 4 * 64), wlo, whi, lane, p6_vgpr};
  // the serpentine sweep of sr_abscoeff_near_zones_kernel
  for (int ci = wave; ci < n_chunks; ci += NW) zones_chunk(W, sink, l0 + 64 * ((grp & 1) ? n_chunks - 1 - ci : ci), l1);
  __syncthreads();
  // the image's planes to their spectra: out [n_ch][n_rows_total][n_pts], stores (sr_wings_mc_kernel adds)
  const size_t n_pts = (size_t)(g_hi - g_lo);
  const int n_here = whi - wlo + 1;
  for (int c = wave; c < mc.n_ch; c += NW) {
    double *o = out + ((size_t)c * n_rows_total + (size_t)(row0 + layer)) * n_pts + (size_t)(wlo - g_lo);
    for (int p = lane; p < n_here; p += 64) o[p] = s_img[c * kPlane + p + 1];
  }
}

// wave-uniform loads of far-field coefficients through the constant address space: scalar loads whatever LDS traffic
// precedes them (profiles/r05_wings_experiments.md: behind any LDS store the compiler turned these loads, through a flat
// pointer, into 24 vector loads per level)
typedef const double __attribute__((address_space(4))) *kconst_ptr;
__device__ inline kconst_ptr as_kconst(const double *p) { return (kconst_ptr)(uintptr_t)p; }

// sr_wings_mc_kernel (one 64-point slot per wave, as sr_abscoeff_near_wings_kernel): every region-1 point of the lines
// that no far-field level owns for the slot -- window ends and starts included: the per-channel suffix sums of the
// folded kernel's window-end scan would be n_ch scans -- in rows, summed into the wave's LDS image [n_ch][64]; then one
// far-field polynomial per (far pass, hierarchy level) from the coefficients the level sub-linesets' far-only passes
// left; ADDS to out (sr_zones_mc_kernel stored).
__global__ __launch_bounds__(64 * kMcWingWaves) void sr_wings_mc_kernel(
    const FastRec *__restrict__ fast, const int *__restrict__ lev_up, const int *__restrict__ lev_lo, IcIndex ix,
    const int *__restrict__ zmax, int n_sub, int n_tiles, int g_lo, int g_hi, FarParams fp, McChannels mc,
    const McFarPass *__restrict__ far, int n_far, double *__restrict__ out, int n_rows_total, int row0) {
  extern __shared__ double s_dyn[];
  double *const s_img = s_dyn; // [n_ch][64]
  const int wg = xcd_remap(blockIdx.x, gridDim.x);
  const int layer = wg / n_tiles, tile = wg - layer * n_tiles;
  const int wlo = g_lo + tile * 64;
  const int whi = min(wlo + 64, g_hi) - 1;
  // kMcWingWaves waves share the slot's image and take its candidate chunks, far passes and output planes in turn: one
  // wave per slot with its 12 KB image kept a CU to 11 of these latency-bound waves (24 of the folded kernel's fit)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int pm = fp.pm[layer];
  for (int c = wave; c < mc.n_ch; c += kMcWingWaves) s_img[c * 64 + lane] = 0.;
  __syncthreads();
  wings_mc_rows(fast + (size_t)layer * n_sub, lev_up, lev_lo, ix, min(max(zmax[layer], kTheta * 32 + pm + 1), kHalf - 1), wlo, whi,
                ff_thr2(0, pm), mc, s_img, 64, lane, wave, kMcWingWaves);
  __syncthreads(); // the rows' sums of every wave are in the image
  wings_mc_polys(far, n_far, fp, layer, g_lo, wlo, s_img, 64, s_img + mc.n_ch * 64 + wave * 64, lane, wave, kMcWingWaves);
  __syncthreads(); // (a pass's two planes are its wave's alone, but the output planes below are dealt by index)
  const int j = wlo + lane;
  if (j <= whi) {
    const size_t n_pts = (size_t)(g_hi - g_lo);
    double *o = out + (size_t)(row0 + layer) * n_pts + (size_t)(j - g_lo);
    const size_t cstride = (size_t)n_rows_total * n_pts;
    for (int c = wave; c < mc.n_ch; c += kMcWingWaves) o[c * cstride] += s_img[c * 64 + lane];
  }
}

// Image width by what fits: two workgroups of kMcImage points per CU when their planes allow (24 planes x 258 doubles =
// 49.5 KB), else 128-point images (36 planes -- the three ctypes of twelve levels -- are 74 KB at 256 points: ONE workgroup,
// eight waves per CU; at 128 points 37 KB: two).  Up to 31 planes at 256 points and up to 141 at 128 (64 levels' pair
// tables are 128 planes, the three ctypes of 47 levels 141; more planes: 0, one coefficient op per level).
size_t zones_mc_lds(int n_ch, int wt) { return sizeof(double) * (size_t)n_ch * (wt + 2) + sizeof(int) * (size_t)kMcWaves * 2 * 4 * 64; }
int zones_mc_image(int n_ch) {
  if (2 * zones_mc_lds(n_ch, kMcImage) <= (size_t)160 * 1024) return kMcImage;
  return zones_mc_lds(n_ch, 128) <= (size_t)160 * 1024 ? 128 : 0;
}
template <int WT>
static int launch_zones_mc_wt(const ShardTables &t, const int *lev_up, const int *lev_lo, const GridParams &gp, const McChannels &mc,
                              double *out, int n_rows_total, int row0, hipStream_t st) {
  constexpr int NW = kMcWaves;
  const int n_t = (t.g_hi - t.g_lo + WT - 1) / WT;
  // (more than 64 KB of dynamic LDS needs the attribute once per kernel and DEVICE: a process that moves to another
  // device sets it there too)
  static unsigned long long attr_set = 0;
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (!(attr_set >> (dev & 63) & 1ull)) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&sr_zones_mc_kernel<WT, NW>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    attr_set |= 1ull << (dev & 63);
  }
  hipLaunchKernelGGL((sr_zones_mc_kernel<WT, NW>), dim3((unsigned)(n_t * t.n_layers)), dim3(64 * NW), zones_mc_lds(mc.n_ch, WT), st, t.fast, t.cold,
                     lev_up, lev_lo, t.ix, t.zmax, t.ix.n_sub, n_t, t.g_lo, t.g_hi, gp, mc, out, n_rows_total, row0);
  return (int)hipGetLastError();
}
int launch_zones_mc(const ShardTables &t, const int *lev_up, const int *lev_lo, const GridParams &gp, const McChannels &mc,
                    double *out, int n_rows_total, int row0, hipStream_t st) {
  if (t.g_hi <= t.g_lo || t.n_layers <= 0) return 0;
  const int wt = zones_mc_image(mc.n_ch);
  if (wt == kMcImage) return launch_zones_mc_wt<kMcImage>(t, lev_up, lev_lo, gp, mc, out, n_rows_total, row0, st);
  if (wt == 128) return launch_zones_mc_wt<128>(t, lev_up, lev_lo, gp, mc, out, n_rows_total, row0, st);
  return (int)hipErrorInvalidValue;
}

size_t wings_mc_lds(int n_ch) { return sizeof(double) * ((size_t)n_ch * 64 + 64 * kMcWingWaves); }
int launch_wings_mc(const ShardTables &t, const int *lev_up, const int *lev_lo, const FarParams &fp, const McChannels &mc,
                    const McFarPass *far, int n_far, double *out, int n_rows_total, int row0, hipStream_t st) {
  if (t.g_hi <= t.g_lo || t.n_layers <= 0) return 0;
  const int n_g1 = (t.g_hi - t.g_lo + 63) / 64;
  const size_t lds = wings_mc_lds(mc.n_ch); // the image + the polynomial stage's staging rows
  if (lds > 160 * 1024) return (int)hipErrorInvalidValue;
  static unsigned long long attr_set = 0; // (per kernel and device, see launch_zones_mc_wt)
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (!(attr_set >> (dev & 63) & 1ull)) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&sr_wings_mc_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    attr_set |= 1ull << (dev & 63);
  }
  hipLaunchKernelGGL(sr_wings_mc_kernel, dim3((unsigned)(n_g1 * t.n_layers)), dim3(64 * kMcWingWaves), lds, st, t.fast, lev_up, lev_lo, t.ix, t.zmax,
                     t.ix.n_sub, n_g1, t.g_lo, t.g_hi, fp, mc, far, n_far, out, n_rows_total, row0);
  return (int)hipGetLastError();
}

int launch_farfield(const ShardTables &t, const FarParams &fp, unsigned long long *cnt, hipStream_t st) {
  const IcIndex &ix = t.ix;
  const int n_sub = ix.n_sub, n_layers = t.n_layers, g_lo = t.g_lo, g_hi = t.g_hi;
  if (g_hi <= g_lo || n_layers <= 0) return 0;
  if (!fp.m2l && fp.rows) { // sparse line set: a box for kFarRows layers per wave
    const dim3 gr((unsigned)(fp.n_boxes_total * ((n_layers + kFarRows - 1) / kFarRows)));
    if (cnt)
      hipLaunchKernelGGL(sr_farfield_rows_kernel<true>, gr, dim3(64), 0, st, t.fast, ix, t.zmax, n_sub, g_lo, fp, cnt);
    else
      hipLaunchKernelGGL(sr_farfield_rows_kernel<false>, gr, dim3(64), 0, st, t.fast, ix, t.zmax, n_sub, g_lo, fp, cnt);
    return (int)hipGetLastError();
  }
  const dim3 grid((unsigned)((fp.m2l ? fp.box_count[0] : fp.n_boxes_total) * n_layers));
#define SR_FAR(C, M) hipLaunchKernelGGL((sr_farfield_kernel<C, M>), grid, dim3(64), 0, st, t.fast, ix, t.zmax, n_sub, g_lo, g_hi, fp, cnt)
  if (fp.m2l) {
    if (cnt) SR_FAR(true, true); else SR_FAR(false, true);
  } else {
    if (cnt) SR_FAR(true, false); else SR_FAR(false, false);
  }
#undef SR_FAR
  return (int)hipGetLastError();
}

int launch_m2l(const ShardTables &t, const FarParams &fp, unsigned long long *cnt, hipStream_t st, int which) {
  const IcIndex &ix = t.ix;
  const int n_sub = ix.n_sub, n_layers = t.n_layers, g_lo = t.g_lo, g_hi = t.g_hi;
  if (g_hi <= g_lo || n_layers <= 0) return 0;
  if (which & 1) {
  const dim3 g1((unsigned)(fp.n_src[0] * n_layers));
  if (cnt)
    hipLaunchKernelGGL(sr_s2m_kernel<true>, g1, dim3(64), 0, st, t.fast, ix, n_sub, g_lo, fp, cnt);
  else
    hipLaunchKernelGGL(sr_s2m_kernel<false>, g1, dim3(64), 0, st, t.fast, ix, n_sub, g_lo, fp, cnt);
  for (int l = 1; l < fp.n_levels; ++l) { // upward pass, level by level
    const int n2 = fp.n_src[l] * n_layers * 4;
    hipLaunchKernelGGL(sr_m2m_kernel, dim3((unsigned)((n2 + 63) / 64)), dim3(64), 0, st, fp, l);
  }
  }
  if (!(which & 2)) return (int)hipGetLastError();
  int chunks = 0;
  for (int lv = 0; lv < fp.n_levels; ++lv) chunks += (fp.box_count[lv] * n_layers + 15) / 16;
  if (cnt)
    hipLaunchKernelGGL(sr_m2l_kernel<true>, dim3((unsigned)chunks), dim3(64), 0, st, t.zmax, fp, cnt);
  else
    hipLaunchKernelGGL(sr_m2l_kernel<false>, dim3((unsigned)chunks), dim3(64), 0, st, t.zmax, fp, cnt);
  return (int)hipGetLastError();
}

// Translation operator of the box-pair far field, [o > 0 | o < 0][|o|][q - 2 < kM2LQ][n < kM2LRow]:
// (-1)^n (q + n - 1)!/n! r^(q+n), r = 1/(2o) (see sr_m2l_kernel); long double, rounded once.
void m2l_table_host(double *tab) {
  for (size_t i = 0; i < (size_t)2 * kM2LOffsets * kM2LQ * kM2LRow; ++i) tab[i] = 0.0; // padding rows / columns
  for (int sg = 0; sg < 2; ++sg)
    for (int a = 0; a < kM2LOffsets; ++a)
      for (int q = 2; q <= kFD; ++q) {
        double *row = tab + (((size_t)sg * kM2LOffsets + a) * kM2LQ + (q - 2)) * kM2LRow;
        if (a == 0) continue;
        const long double r = (sg ? -1.0L : 1.0L) / (2.0L * a);
        long double v = 1.0L;
        for (int k = 2; k < q; ++k) v *= k;        // (q-1)!
        for (int k = 0; k < q; ++k) v *= r;        // r^q
        row[0] = (double)v;
        for (int n = 1; n < kFC; ++n) {
          v *= -r * (long double)(q + n - 1) / (long double)n;
          row[n] = (double)v;
        }
      }
}

#ifndef SR_ZONES_WT
#define SR_ZONES_WT 512
#endif
constexpr int kZoneImage = SR_ZONES_WT; // grid points per LDS image of sr_abscoeff_near_zones_kernel (a multiple of 64)
template <int NW, bool COUNT>
static void launch_zones(dim3 gz, const FastRec *fast, const ColdRec *cold, const IcIndex &ix, const int *zmax,
                         int n_sub, int n_t, int g_lo, int g_hi, const GridParams &gp, int add, double *abs_out,
                         double *emi_out, unsigned long long *cnt, hipStream_t st) {
  // (layer chunks, one launch each, were measured and lost: profiles/r04_timeline_zones_chunks8.txt)
  hipLaunchKernelGGL((sr_abscoeff_near_zones_kernel<kZoneImage, NW, COUNT>), gz, dim3(64 * NW), 0, st, fast, cold, ix, zmax, n_sub,
                     n_t, g_lo, g_hi, gp, add, abs_out, emi_out, cnt, 0);
}

int launch_near(int part, int add, const ShardTables &t, const GridParams &gp, const FarParams &fp, double *abs_out,
                double *emi_out, unsigned long long *cnt, hipStream_t st, const double *z_abs, const double *z_emi) {
  const IcIndex &ix = t.ix;
  const int n_sub = ix.n_sub, n_layers = t.n_layers, g_lo = t.g_lo, g_hi = t.g_hi;
  if (g_hi <= g_lo || n_layers <= 0) return 0;
  const int n_groups = (g_hi - g_lo + kGroup - 1) / kGroup;
  const dim3 grid((unsigned)(n_groups * n_layers));
  if (part == 1) {
    // slots per wave: 4 (256-point groups) measured 2.53 ms on config 2, 2: 2.31 ms, 1: see DESIGN.md
    const int n_g1 = (g_hi - g_lo + 63) / 64;
    if (cnt)
      hipLaunchKernelGGL(sr_abscoeff_near_wings_kernel<true>, dim3((unsigned)(n_g1 * n_layers)), dim3(64), 0, st,
                         t.fast, ix, t.zmax, n_sub, n_g1, g_lo, g_hi, fp, add, z_abs, z_emi, abs_out, emi_out, cnt);
    else
      hipLaunchKernelGGL(sr_abscoeff_near_wings_kernel<false>, dim3((unsigned)(n_g1 * n_layers)), dim3(64), 0, st,
                         t.fast, ix, t.zmax, n_sub, n_g1, g_lo, g_hi, fp, add, z_abs, z_emi, abs_out, emi_out, cnt);
  } else {
    // Image width: wider images cut fewer zones in two (fewer (line, group) pairs: 7.1 -> 6.7 ms on
    // 1e5 points x 80 layers with 512 instead of 256) as long as the waves still fill the chip
    // several times over (1024: 9.3 ms, too few waves and 16 KB LDS each).
    const long waves512 = (long)((g_hi - g_lo + kZoneImage - 1) / kZoneImage) * n_layers;
    const int n_t = (g_hi - g_lo + kZoneImage - 1) / kZoneImage;
    const dim3 gz((unsigned)(n_t * n_layers));
#define SR_ZONES(NW)                                                                                         \
  (cnt ? launch_zones<NW, true>(gz, t.fast, t.cold, ix, t.zmax, n_sub, n_t, g_lo, g_hi, gp, add, abs_out, emi_out, cnt, st) \
       : launch_zones<NW, false>(gz, t.fast, t.cold, ix, t.zmax, n_sub, n_t, g_lo, g_hi, gp, add, abs_out, emi_out, cnt, st))
    if (waves512 >= 3 * 4096)
      SR_ZONES(1);
    else if (waves512 >= 3 * 2048)
      SR_ZONES(2);
    else if (waves512 >= 3 * 512)
      // Judged by the PIPELINED step (zones beside the far-field and wings kernels), not by the kernel alone: on
      // config 2 (round 3) 1/8 shard, 2000 images: NW = 1 / 2 / 4 / 8 -> 1.065 / 0.928 / 0.870 / 0.923 ms per step
      // (alone: 0.765 / 0.550 / 0.520 / 0.518) -- round 2 took 8 below 3072 images; 1/4 shard, 3920 images:
      // 1.554 / 1.588 / 1.589 / 1.602; 1/2 shard: 2.848 / 2.881 / 2.841 / 2.900; whole grid, 15680: 5.49 / 5.52
      // (alone 3.53 / 3.34: two waves per image have the shorter tail, but beside the other kernels the tail is
      // filled anyway).  One wave from 3072 images up looked as good on config 2 but left a sparse 20000-point
      // shard (0.3 lines per point, 3300 images) at 2.8 instead of 1.5 ms: it is the WAVES that must fill the chip.
      // 5, 6 and 7 waves (14 chunks per image = 2 x 7) measured 0.68 / 0.81 / 0.59 ms alone on the 1/8 shard.
      SR_ZONES(4);
    else
      SR_ZONES(8);
#undef SR_ZONES
  }
  return (int)hipGetLastError();
}

int launch_prep(const LinesDev &L, const LayersDev &A, const GridParams &gp, const WeightMode &W, int line_lo,
                int n_sub, int cold_lo, int cold_hi, FastRec *fast, ColdRec *cold, hipStream_t st) {
  if (n_sub <= 0 || A.n_layers <= 0) return 0;
  dim3 grid((n_sub + kPrepBlock - 1) / kPrepBlock, A.n_layers);
  hipLaunchKernelGGL(sr_prep_kernel, grid, dim3(kPrepBlock), 0, st, L, A, gp, W, line_lo, n_sub, cold_lo, cold_hi, fast,
                     cold);
  return (int)hipGetLastError();
}

int abscoeff_tile_points(int variant) { return 64 * (variant == 4 ? 4 : 8); }

int launch_abscoeff(int variant, int which, const ShardTables &t, const GridParams &gp, double *abs_out, double *emi_out,
                    hipStream_t st) {
  const IcIndex &ix = t.ix;
  const int n_sub = ix.n_sub, n_layers = t.n_layers, g_lo = t.g_lo, g_hi = t.g_hi;
  if (g_hi <= g_lo || n_layers <= 0) return 0;
  if (which == 0) {
    const int tp = abscoeff_tile_points(variant);
    const int n_tiles = (g_hi - g_lo + tp - 1) / tp;
    dim3 grid((unsigned)(n_tiles * n_layers));
    if (variant == 4)
      hipLaunchKernelGGL((sr_abscoeff_wings_kernel<4>), grid, dim3(64), 0, st, t.fast, ix, n_sub, n_tiles,
                         g_lo, g_hi, abs_out, emi_out);
    else
      hipLaunchKernelGGL((sr_abscoeff_wings_kernel<8>), grid, dim3(64), 0, st, t.fast, ix, n_sub, n_tiles,
                         g_lo, g_hi, abs_out, emi_out);
  } else {
    const int n_groups = (g_hi - g_lo + kGroup - 1) / kGroup;
    dim3 grid((unsigned)(n_groups * n_layers));
    hipLaunchKernelGGL(sr_abscoeff_cores_kernel, grid, dim3(64), 0, st, t.fast, t.cold, ix, t.zmax, n_sub, n_groups,
                       g_lo, g_hi, gp, abs_out, emi_out);
  }
  return (int)hipGetLastError();
}

} // namespace sr
