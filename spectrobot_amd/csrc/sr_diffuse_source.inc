// sr_diffuse_source.inc -- sr_diffuse_field_kernel and the layer operators of the diffuse family.  Included by
// sr_solar_source.hip inside namespace sr, and by the host builds tools/diffuse_*_host.  Nothing else includes it.

// The diffuse (multiply scattered) field of coefficient rows, under the sun, from thermal emission, or both: a
// plane-parallel two-stream solve per grid point with delta scaling and a Lambertian lower boundary, under the direct beam
// the caller made in spherical geometry.  The build's own definition -- the reference has no counterpart (DESIGN.md 4.11b,
// 4.11f).  Layers l = 0 .. N-1 bottom to top, interfaces i = 0 .. N; per layer and point, with t_g = V[g][l] A[g N + l][j]
// and every sum one of non-negative addends (1 - omega' is never formed by subtraction):
//   sp = sum ssa_g (1 - f_g) t_g,  al = sum (1 - ssa_g) t_g,  sg = sum ssa_g (asym_g - f_g) t_g,   f_g = max(asym_g, 0)^2
//   dtau = sp + al,  co = max(al / dtau, 2^-52),  omega = 1 - co,  g = sg / sp (0 where sp == 0)
// and the quadrature two-stream scheme of Meador & Weaver (1980) with the source of the layer's middle,
// D = sun[j] beam[l][j]:
//   d = sqrt3 co, s = sqrt3 (1 - omega g), sd = sqrt d, ss = sqrt s, k = sd ss, gamma1 = (s + d) / 2,
//   gamma2 = sqrt3 omega (1 - g) / 2, Gamma = gamma2 / (gamma1 + k), e = exp(-k dtau), m = -expm1(-k dtau),
//   u = sd (sd + ss) / (gamma1 + k) [= 1 - Gamma], den = (u + Gamma m)(1 + Gamma e)
//   R = Gamma m (1 + e) / den,  T = e u (1 + Gamma) / den,  1 - T = m (u + Gamma (1 + Gamma e)) / den,
//   1 - R = u (1 + Gamma e^2) / den,  1 - R - T = m u (1 - Gamma e) / den
//   E+ + E- = omega D (sd + ss) / (gamma1 + k) (m / sd) / (1 + Gamma e)
//   E+ - E- = -omega D sqrt3 g mu0 / s ((1 - T) + R)
// A layer with dtau == 0 passes light through: R = 0, T = 1, E = 0, q = 1 (nothing below or above changes a bit).  Adding, bottom up -- Rb the reflection of everything
// below interface l, Ub the upwelling it sends with nothing coming down, Cb = 1 - Rb carried beside Rb so that
// 1 - Rb R = Cb + Rb (1 - R) is a sum too:
//   Rb_0 = albedo, Cb_0 = 1 - albedo, Ub_0 = albedo max(mu0, 0) sun beam[N]
//   q = 1 / (Cb + Rb (1 - R)),  Rb' = R + T^2 Rb q,  Cb' = ((1 - R) Cb + Rb (1 - R - T)((1 - R) + T)) q
//   Ub' = E+ + T (Ub + Rb E-) q
// then top down: F-_N = 0, F+_N = Ub_N, F-_l = T q F-_{l+1} + (E- + R Ub_l) q, F+_l = Ub_l + Rb_l F-_l, and
//   J_l = sqrt3 (F+_l + F-_l + F+_{l+1} + F-_{l+1}) / (8 pi),   emi[l][j] (+)= w_out A[G N + l][j] J_l,
// w_out = ssa_G (1 - f_G).
//
// Thermal emission (THERMAL) is a source of the same field, alone (the night side, SOLAR = false) or together with the
// sun's: the two-stream equations are linear in their sources, so the thermal terms are added to the same E+- and Ub_0.
// The source of layer l is isotropic and constant over the layer, at the layer's own temperature, S+ = S- = 2 pi co B_l:
// the particular solution is F+ = F- = 2 pi B_l / sqrt3 (co cancels), and with nothing coming in the layer sends out
//   E+_th = E-_th = (2 pi / sqrt3) B_l (1 - R - T)                                            -- Kirchhoff's law
// with 1 - R - T = m u / (1 + Gamma e) (absq below: absb's closed form with u + Gamma m = 1 - Gamma e cancelled against
// den; as co -> 0 in a thin layer the subtraction 1 - Gamma e would lose sqrt(co) of the SOURCE's digits),
//   B_l = 2 h c^2 nu^3 / (exp(x) - 1), x = c2 nu / T_l, nu = w0 + (double)(g_lo + j) step       (the point's wavenumber)
// A layer with alpha == 0 at a point has a thermal source of exactly 0: the floor co >= 2^-52 invents no emission.  The
// lower boundary, a Lambertian surface of emissivity 1 - albedo at t_surface (0: none), adds
//   Ub_0 += (1 - albedo) (2 pi / sqrt3) B(nu, t_surface)
// -- the two-stream value, not pi B: a surface, an atmosphere and incident light at one temperature then leave
// F+- = 2 pi B / sqrt3 and J = B exactly.  F-(top) = 0 stays.  The rows:
//   own == 0:  emi[l][j] (+)= w_out A[G N + l][j] J_l                         w_out = ssa_G (1 - f_G)
//   own != 0:  emi[l][j] (+)= A[G N + l][j] (w_abs B_l + w_out J_l)           w_abs = 1 - ssa_G: the complete thermal row
// x is formed as sr_absorber_table_kernel forms it (sr_absorber_table.inc): x~ = (c2 nu)(1 / T) with its exact residual dx
// from two fused multiply-adds, exp(x) = exp(x~)(1 + dx), exp - 1 by subtraction; c2 nu, its residual and 2 h c^2 nu^3
// once per thread.  x >= 700 (exp would overflow) is B = 0.  The downward sweep forms B_l again for the own rows: the
// workspace stays four doubles per (layer, point).
//
// One thread per grid point, 256 points per block, blocks dealt by limb_block().  Every load and store is one row at
// consecutive points.  The upward sweep leaves four doubles per (layer, point) in the workspace ws [4][N][ws_stride] --
// T q, (E- + R Ub) q, Rb, Ub -- which the downward sweep reads back: no per-thread array is indexed by layer.  A layer's
// rows of A and beam are requested one layer ahead of the arithmetic that uses them.  V, temps [N] and the per-gas
// coefficients are block-uniform (scalar loads), staged together; the gas loop has kDiffuseGases slots, a slot beyond
// n_gas reads gas 0's row with coefficients of zero (coef is padded by the host): every load valid, 0 . finite contributes
// nothing.  A point beyond the call's last reads the last point and stores nothing (its workspace column is its own).
// SOLAR = false reads neither beam nor sun (both may be null), mu0 is not used and the solar sources are not formed;
// THERMAL = false reads no temps (it may be null) and holds no thermal statement.  No LDS, one writer per element, no
// atomics: the same call gives the same bits.
// (kDiffuseGases: sr_solar_plan.hpp)

// What the illumination does not touch, of a layer with dtau = sp + al > 0 -- R, T, 1 - R, 1 - R - T (absb; absq: the
// same once more, as m u / (1 + Gamma e), nothing subtracted: the thermal source) -- and the intermediates the two source
// formers read, diffuse_layer below and diffuse_layer_shared (sr_diffuse_columns.inc).  The empty layer is the formers':
// R = 0, T = 1, 1 - R = 1, every source 0, live = false.
struct DiffuseOps { double R, T, oneR, absb, absq, om, g, s, sd, ss, rg, m, ge, oneT; };

__device__ __forceinline__ DiffuseOps diffuse_operators(double sp, double al, double sg) {
  const double kSqrt3 = 1.7320508075688772;
  DiffuseOps o;
  const double dtau = sp + al;
  const double co = fmax(al / dtau, 0x1p-52);
  o.om = 1.0 - co;
  o.g = sp > 0.0 ? sg / sp : 0.0;
  const double d = kSqrt3 * co;
  o.s = kSqrt3 * (1.0 - o.om * o.g);
  o.sd = sqrt(d), o.ss = sqrt(o.s);
  const double k = o.sd * o.ss, g1 = 0.5 * (o.s + d);
  const double g2 = 0.5 * (kSqrt3 * o.om * (1.0 - o.g));
  o.rg = 1.0 / (g1 + k);
  const double Gm = g2 * o.rg, u = o.sd * (o.sd + o.ss) * o.rg;
  const double x = k * dtau, e = exp(-x);
  o.m = -expm1(-x);
  o.ge = 1.0 + Gm * e;
  const double rden = 1.0 / ((u + Gm * o.m) * o.ge);
  o.R = Gm * o.m * (1.0 + e) * rden;
  o.T = e * u * (1.0 + Gm) * rden;
  o.oneR = u * (1.0 + Gm * e * e) * rden;
  o.absb = o.m * u * (1.0 - Gm * e) * rden;
  o.absq = o.m * u / o.ge;
  o.oneT = o.m * (u + Gm * o.ge) * rden;
  return o;
}

// The source former of one column of illumination: the operators and E+- under the source D of the layer's middle,
// omega D first.  (The columns' former factors D out instead: another order of roundings.)
struct DiffuseLayer { double R, T, Ep, Em, oneR, absb, absq; bool live; };

__device__ __forceinline__ DiffuseLayer diffuse_layer(double sp, double al, double sg, double D, double mu0) {
  const double kSqrt3 = 1.7320508075688772;
  if (!(sp + al > 0.0)) return DiffuseLayer{0.0, 1.0, 0.0, 0.0, 1.0, 0.0, 0.0, false};
  const DiffuseOps p = diffuse_operators(sp, al, sg);
  const double src = p.om * D;
  const double es = src * (p.sd + p.ss) * p.rg * (p.m / p.sd) / p.ge;
  const double ed = -(src * (kSqrt3 * p.g * mu0)) / p.s * (p.oneT + p.R);
  return DiffuseLayer{p.R, p.T, 0.5 * (es + ed), 0.5 * (es - ed), p.oneR, p.absb, p.absq, true};
}

// The adding's start at the lower boundary, for sr_diffuse_tangent_kernel (sr_diffuse_jac.inc) too: Rb_0 = albedo,
// Cb_0 = 1 - albedo, Ub_0 = albedo max(mu0, 0) sun beam[N].
__device__ __forceinline__ void diffuse_boundary(double albedo, double mu0, double sj, double beam_below, double &Rb, double &Cb,
                                                 double &Ub) {
  Rb = albedo, Cb = 1.0 - albedo;
  Ub = albedo * (fmax(mu0, 0.0) * (sj * beam_below));
}

// The three sums of layer l from its rows a[g] of A, for every kernel of the family: gas by gas in the slots' order, a slot
// beyond n_gas with gas 0's column and coefficients of zero.  coef [3][kDiffuseGases]: ssa (1 - f), 1 - ssa, ssa (asym - f).
struct DiffuseSums { double sp, al, sg; };
__device__ __forceinline__ DiffuseSums diffuse_sums(const double *__restrict__ v, const double *__restrict__ coef, int n_gas,
                                                    int n_layers, int l, const double (&a)[kDiffuseGases]) {
  const double *cs = coef, *ca = coef + kDiffuseGases, *cg = coef + 2 * kDiffuseGases;
  double sp = 0.0, al = 0.0, sg = 0.0;
#pragma unroll
  for (int g = 0; g < kDiffuseGases; ++g) {
    const double t = v[(g < n_gas ? g : 0) * n_layers + l] * a[g];
    sp += cs[g] * t;
    al += ca[g] * t;
    sg += cg[g] * t;
  }
  return DiffuseSums{sp, al, sg};
}

// The Planck function at a point of the grid: what depends on nu alone, once per thread
struct ThermalPoint { double c2nu, c2nu_lo, pnu; };

__device__ __forceinline__ ThermalPoint thermal_point(double w0, double step, int g) {
  const double nu = w0 + (double)g * step;
  const double c2nu = kC2 * nu;
  return ThermalPoint{c2nu, fma(kC2, nu, -c2nu), 2 * kHcgs * (kCcgs * kCcgs) * (nu * nu * nu)};
}

__device__ __forceinline__ double thermal_planck(const ThermalPoint &p, double T) {
  const double rT = 1.0 / T, x = p.c2nu * rT, dx = (fma(-x, T, p.c2nu) + p.c2nu_lo) * rT;
  const double ex0 = exp(x), ex = ex0 + ex0 * dx;
  return x > 0.0 && x < 700.0 ? p.pnu * (1.0 / (ex - 1)) : 0.0;
}

template <bool SOLAR, bool THERMAL, bool ACC, bool WJ, bool WF>
__global__ __launch_bounds__(256) void sr_diffuse_field_kernel(
    const double *__restrict__ tab_abs, int n_gas, int n_layers, int n_pts, int p_lo, int p_hi, const double *__restrict__ v,
    const double *__restrict__ coef, const double *__restrict__ temps, const double *__restrict__ beam,
    const double *__restrict__ sun, double mu0, double albedo, double t_surface, double w0, double step, int g_lo, int own,
    int out_gas, double *__restrict__ ws, int ws_stride, double *__restrict__ emi_out,
    double *__restrict__ j_out, double *__restrict__ flux_out) {
  static_assert(SOLAR || THERMAL, "a field without a source");
  int pb, item;
  if (!limb_block((p_hi - p_lo + 255) / 256, 1, pb, item)) return; // (block-uniform)
  const int col = pb * 256 + threadIdx.x, j = p_lo + col;
  const bool live = j < p_hi;
  const size_t np = (size_t)n_pts, jj = (size_t)min(j, p_hi - 1);
  const size_t wrow = (size_t)ws_stride, wq = (size_t)n_layers * wrow; // ws [4][n_layers][ws_stride]
  const double kTh = 2.0 * 3.141592653589793 / 1.7320508075688772;    // 2 pi / sqrt3
  ThermalPoint tp = {};
  if (THERMAL) tp = thermal_point(w0, step, g_lo + (int)jj);
  double sj = 0.0;
  if (SOLAR) sj = sun[jj];

  // G's row weight of the instances without the thermal source, read ahead of the upward sweep: read behind it, as the
  // thermal instances read theirs, it cost these twenty scalar moves more per layer than a kernel argument did
  // (profiles/diffuse_field_kernel_resources.txt)
  const double w_sun = !THERMAL && emi_out != nullptr ? coef[out_gas] : 0.0;

  // ---- bottom up ----
  double a_nx[kDiffuseGases], b_nx = 0.0;
  auto fetch = [&](int l) {
#pragma unroll
    for (int g = 0; g < kDiffuseGases; ++g) a_nx[g] = tab_abs[((size_t)(g < n_gas ? g : 0) * n_layers + l) * np + jj];
    if (SOLAR) b_nx = beam[(size_t)l * np + jj];
  };
  fetch(0);
  double Rb, Cb, Ub;
  if (SOLAR) {
    diffuse_boundary(albedo, mu0, sj, beam[(size_t)n_layers * np + jj], Rb, Cb, Ub);
  } else {
    Rb = albedo, Cb = 1.0 - albedo, Ub = 0.0;
  }
  if (THERMAL && t_surface > 0.0) Ub += Cb * (kTh * thermal_planck(tp, t_surface)); // (block-uniform)
  for (int l = 0; l < n_layers; ++l) {
    double a[kDiffuseGases];
#pragma unroll
    for (int g = 0; g < kDiffuseGases; ++g) a[g] = a_nx[g];
    const double bm = b_nx;
    if (l + 1 < n_layers) fetch(l + 1); // the next layer's rows in flight under this layer's arithmetic
    const DiffuseSums s = diffuse_sums(v, coef, n_gas, n_layers, l, a);
    const DiffuseLayer o = diffuse_layer(s.sp, s.al, s.sg, SOLAR ? sj * bm : 0.0, SOLAR ? mu0 : 0.0);
    double Ep = o.Ep, Em = o.Em;
    if (THERMAL) {
      const double eth = s.al > 0.0 ? (kTh * thermal_planck(tp, temps[l])) * o.absq : 0.0; // no absorber: an exact 0
      Ep = SOLAR ? o.Ep + eth : eth, Em = SOLAR ? o.Em + eth : eth; // (night: the solar sources are never formed)
    }
    const double q = o.live ? 1.0 / (Cb + Rb * o.oneR) : 1.0; // (an empty layer: every quantity keeps its bits)
    const size_t at = (size_t)l * wrow + col;
    ws[at] = o.T * q;
    ws[wq + at] = (Em + o.R * Ub) * q;
    ws[2 * wq + at] = Rb;
    ws[3 * wq + at] = Ub;
    Ub = Ep + o.T * (Ub + Rb * Em) * q;
    Cb = (o.oneR * Cb + Rb * o.absb * (o.oneR + o.T)) * q;
    Rb = o.R + o.T * o.T * Rb * q;
  }

  // ---- top down ----
  const double kJ = 1.7320508075688772 / (8.0 * 3.141592653589793);
  const size_t frow = (size_t)(n_layers + 1) * np; // flux_out [2][n_layers + 1][n_pts]
  double fp = Ub, fm = 0.0;
  if (WF && live) {
    flux_out[(size_t)n_layers * np + j] = fp;
    flux_out[frow + (size_t)n_layers * np + j] = fm;
  }
  const bool emit = emi_out != nullptr; // (block-uniform)
  const double w_out = THERMAL ? (emit ? coef[out_gas] : 0.0) : w_sun;          // ssa (1 - f) of G
  const double w_abs = THERMAL && emit ? coef[kDiffuseGases + out_gas] : 0.0; // 1 - ssa of G
  double w_nx[4], s_nx = 0.0;
  auto fetch_down = [&](int l) {
    const size_t at = (size_t)l * wrow + col;
#pragma unroll
    for (int c = 0; c < 4; ++c) w_nx[c] = ws[c * wq + at];
    if (emit) s_nx = tab_abs[((size_t)out_gas * n_layers + l) * np + jj];
  };
  fetch_down(n_layers - 1);
  for (int l = n_layers - 1; l >= 0; --l) {
    const double tq = w_nx[0], cq = w_nx[1], rb = w_nx[2], ub = w_nx[3], sca = s_nx;
    if (l > 0) fetch_down(l - 1);
    const double fm_l = tq * fm + cq, fp_l = ub + rb * fm_l;
    const double J = kJ * ((fp_l + fm_l) + (fp + fm));
    fp = fp_l, fm = fm_l;
    if (!live) continue;
    const size_t at = (size_t)l * np + j;
    if (WF) {
      flux_out[at] = fp;
      flux_out[frow + at] = fm;
    }
    if (WJ) j_out[at] = J;
    if (emit) {
      const double val = THERMAL && own ? sca * (w_abs * thermal_planck(tp, temps[l]) + w_out * J) : (w_out * sca) * J;
      emi_out[at] = ACC ? emi_out[at] + val : val;
    }
  }
}
