// sr_diffuse_thermal.inc -- sr_diffuse_thermal_kernel.  Included by sr_solar_source.hip inside namespace sr after
// sr_diffuse_source.inc, whose diffuse_sums, diffuse_layer and diffuse_boundary it uses, and by the host build
// tools/diffuse_thermal_host.  Nothing else includes it.

// Thermal emission as a source of the two-stream diffuse field, alone (the night side) or together with the sun's.  The
// build's own definition -- the reference has no counterpart (DESIGN.md 4.11f).  Notation, layer operators, adding and
// sweeps are sr_diffuse_source_kernel's (sr_diffuse_source.inc); the two-stream equations are linear in their sources, so
// the thermal terms are added to the same E+- and Ub_0.  The source of layer l is isotropic and constant over the layer,
// at the layer's own temperature, S+ = S- = 2 pi co B_l: the particular solution is F+ = F- = 2 pi B_l / sqrt3 (co
// cancels), and with nothing coming in the layer sends out
//   E+_th = E-_th = (2 pi / sqrt3) B_l (1 - R - T)                                            -- Kirchhoff's law
// with 1 - R - T = m u / (1 + Gamma e) (absq of diffuse_layer(): absb's closed form with u + Gamma m = 1 - Gamma e cancelled
// against den; as co -> 0 in a thin layer the subtraction 1 - Gamma e would lose sqrt(co) of the SOURCE's digits),
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
// Laid out as its sibling: one thread per grid point, 256 per block, limb_block(), the next layer's rows in flight, ws
// [4][N][ws_stride].  temps [N] is block-uniform (scalar loads), staged with v.  SOLAR = false is the night instance: it
// reads neither beam nor sun (both may be null), mu0 is not used and the solar sources are not formed.  No LDS, no
// atomics, one writer per element: the same call gives the same bits.
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

template <bool SOLAR, bool ACC, bool WJ, bool WF>
__global__ __launch_bounds__(256) void sr_diffuse_thermal_kernel(
    const double *__restrict__ tab_abs, int n_gas, int n_layers, int n_pts, int p_lo, int p_hi, const double *__restrict__ v,
    const double *__restrict__ coef, const double *__restrict__ temps, const double *__restrict__ beam,
    const double *__restrict__ sun, double mu0, double albedo, double t_surface, double w0, double step, int g_lo, int own,
    int out_gas, double *__restrict__ ws, int ws_stride, double *__restrict__ emi_out,
    double *__restrict__ j_out, double *__restrict__ flux_out) {
  int pb, item;
  if (!limb_block((p_hi - p_lo + 255) / 256, 1, pb, item)) return; // (block-uniform)
  const int col = pb * 256 + threadIdx.x, j = p_lo + col;
  const bool live = j < p_hi;
  const size_t np = (size_t)n_pts, jj = (size_t)min(j, p_hi - 1);
  const size_t wrow = (size_t)ws_stride, wq = (size_t)n_layers * wrow; // ws [4][n_layers][ws_stride]
  const double kTh = 2.0 * 3.141592653589793 / 1.7320508075688772;    // 2 pi / sqrt3
  const ThermalPoint tp = thermal_point(w0, step, g_lo + (int)jj);
  double sj = 0.0;
  if (SOLAR) sj = sun[jj];

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
  if (t_surface > 0.0) Ub += Cb * (kTh * thermal_planck(tp, t_surface)); // (block-uniform)
  for (int l = 0; l < n_layers; ++l) {
    double a[kDiffuseGases];
#pragma unroll
    for (int g = 0; g < kDiffuseGases; ++g) a[g] = a_nx[g];
    const double bm = b_nx;
    if (l + 1 < n_layers) fetch(l + 1); // the next layer's rows in flight under this layer's arithmetic
    const DiffuseSums s = diffuse_sums(v, coef, n_gas, n_layers, l, a);
    const DiffuseLayer o = diffuse_layer(s.sp, s.al, s.sg, SOLAR ? sj * bm : 0.0, SOLAR ? mu0 : 0.0);
    const double eth = s.al > 0.0 ? (kTh * thermal_planck(tp, temps[l])) * o.absq : 0.0; // no absorber: an exact 0
    const double Ep = SOLAR ? o.Ep + eth : eth, Em = SOLAR ? o.Em + eth : eth; // (night: the solar sources are never formed)
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
  const double w_out = emit ? coef[out_gas] : 0.0, w_abs = emit ? coef[kDiffuseGases + out_gas] : 0.0; // ssa (1 - f), 1 - ssa of G
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
      const double val = own ? sca * (w_abs * thermal_planck(tp, temps[l]) + w_out * J) : (w_out * sca) * J;
      emi_out[at] = ACC ? emi_out[at] + val : val;
    }
  }
}
