// sr_diffuse_source.inc -- sr_diffuse_source_kernel.  Included by sr_solar_source.hip inside namespace sr, and by the host
// build tools/diffuse_source_host.  Nothing else includes it.

// The diffuse (multiply scattered) solar source of coefficient rows: a plane-parallel two-stream solve per grid point with
// delta scaling and a Lambertian lower boundary, under the direct beam the caller made in spherical geometry.  The build's
// own definition -- the reference has no counterpart (DESIGN.md 4.11b).  Layers l = 0 .. N-1 bottom to top, interfaces
// i = 0 .. N; per layer and point, with t_g = V[g][l] A[g N + l][j] and every sum one of non-negative addends
// (1 - omega' is never formed by subtraction):
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
// One thread per grid point, 256 points per block, blocks dealt by limb_block().  Every load and store is one row at
// consecutive points.  The upward sweep leaves four doubles per (layer, point) in the workspace ws [4][N][ws_stride] --
// T q, (E- + R Ub) q, Rb, Ub -- which the downward sweep reads back: no per-thread array is indexed by layer.  A layer's
// rows of A and beam are requested one layer ahead of the arithmetic that uses them.  V and the per-gas coefficients are
// block-uniform (scalar loads); the gas loop has kDiffuseGases slots, a slot beyond n_gas reads gas 0's row with
// coefficients of zero (coef is padded by the host): every load valid, 0 . finite contributes nothing.  A point beyond the
// call's last reads the last point and stores nothing (its workspace column is its own).  One writer per element, no
// atomics: the same call gives the same bits.
// (kDiffuseGases: sr_solar_plan.hpp)
struct DiffuseLayer { double R, T, Ep, Em, oneR, absb, absq; bool live; }; // absq: 1 - R - T once more, as m u / (1 + Gamma e) --
// u + Gamma m = 1 - Gamma e cancelled against den, nothing subtracted -- for sr_diffuse_thermal_kernel, whose source it is

// the layer operators from the three sums and the source D of the layer's middle
__device__ __forceinline__ DiffuseLayer diffuse_layer(double sp, double al, double sg, double D, double mu0) {
  const double kSqrt3 = 1.7320508075688772;
  DiffuseLayer o;
  const double dtau = sp + al;
  if (!(dtau > 0.0)) {
    o.R = 0.0, o.T = 1.0, o.Ep = 0.0, o.Em = 0.0, o.oneR = 1.0, o.absb = 0.0, o.absq = 0.0, o.live = false;
    return o;
  }
  o.live = true;
  const double co = fmax(al / dtau, 0x1p-52), om = 1.0 - co;
  const double g = sp > 0.0 ? sg / sp : 0.0;
  const double d = kSqrt3 * co, s = kSqrt3 * (1.0 - om * g);
  const double sd = sqrt(d), ss = sqrt(s), k = sd * ss, g1 = 0.5 * (s + d);
  const double g2 = 0.5 * (kSqrt3 * om * (1.0 - g));
  const double rg = 1.0 / (g1 + k);
  const double Gm = g2 * rg, u = sd * (sd + ss) * rg;
  const double x = k * dtau, e = exp(-x), m = -expm1(-x);
  const double ge = 1.0 + Gm * e;
  const double rden = 1.0 / ((u + Gm * m) * ge);
  o.R = Gm * m * (1.0 + e) * rden;
  o.T = e * u * (1.0 + Gm) * rden;
  o.oneR = u * (1.0 + Gm * e * e) * rden;
  o.absb = m * u * (1.0 - Gm * e) * rden;
  o.absq = m * u / ge;
  const double oneT = m * (u + Gm * ge) * rden;
  const double src = om * D;
  const double es = src * (sd + ss) * rg * (m / sd) / ge;
  const double ed = -(src * (kSqrt3 * g * mu0)) / s * (oneT + o.R);
  o.Ep = 0.5 * (es + ed);
  o.Em = 0.5 * (es - ed);
  return o;
}

// The adding's start at the lower boundary, for sr_diffuse_tangent_kernel (sr_diffuse_jac.inc) too: Rb_0 = albedo,
// Cb_0 = 1 - albedo, Ub_0 = albedo max(mu0, 0) sun beam[N].
__device__ __forceinline__ void diffuse_boundary(double albedo, double mu0, double sj, double beam_below, double &Rb, double &Cb,
                                                 double &Ub) {
  Rb = albedo, Cb = 1.0 - albedo;
  Ub = albedo * (fmax(mu0, 0.0) * (sj * beam_below));
}

// The three sums of layer l from its rows a[g] of A, for both kernels: gas by gas in the slots' order, a slot beyond n_gas
// with gas 0's column and coefficients of zero.  coef [3][kDiffuseGases]: ssa (1 - f), 1 - ssa, ssa (asym - f).
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

template <bool ACC, bool WJ, bool WF>
__global__ __launch_bounds__(256) void sr_diffuse_source_kernel(const double *__restrict__ tab_abs, int n_gas, int n_layers, int n_pts,
                                                                int p_lo, int p_hi, const double *__restrict__ v,
                                                                const double *__restrict__ coef, const double *__restrict__ beam,
                                                                const double *__restrict__ sun, double mu0, double albedo, int out_gas,
                                                                double w_out, double *__restrict__ ws, int ws_stride,
                                                                double *__restrict__ emi_out, double *__restrict__ j_out,
                                                                double *__restrict__ flux_out) {
  int pb, item;
  if (!limb_block((p_hi - p_lo + 255) / 256, 1, pb, item)) return; // (block-uniform)
  const int col = pb * 256 + threadIdx.x, j = p_lo + col;
  const bool live = j < p_hi;
  const size_t np = (size_t)n_pts, jj = (size_t)min(j, p_hi - 1);
  const size_t wrow = (size_t)ws_stride, wq = (size_t)n_layers * wrow; // ws [4][n_layers][ws_stride]
  const double sj = sun[jj];

  // ---- bottom up ----
  double a_nx[kDiffuseGases], b_nx;
  auto fetch = [&](int l) {
#pragma unroll
    for (int g = 0; g < kDiffuseGases; ++g) a_nx[g] = tab_abs[((size_t)(g < n_gas ? g : 0) * n_layers + l) * np + jj];
    b_nx = beam[(size_t)l * np + jj];
  };
  fetch(0);
  double Rb, Cb, Ub;
  diffuse_boundary(albedo, mu0, sj, beam[(size_t)n_layers * np + jj], Rb, Cb, Ub);
  for (int l = 0; l < n_layers; ++l) {
    double a[kDiffuseGases];
#pragma unroll
    for (int g = 0; g < kDiffuseGases; ++g) a[g] = a_nx[g];
    const double bm = b_nx;
    if (l + 1 < n_layers) fetch(l + 1); // the next layer's rows in flight under this layer's arithmetic
    const DiffuseSums s = diffuse_sums(v, coef, n_gas, n_layers, l, a);
    const DiffuseLayer o = diffuse_layer(s.sp, s.al, s.sg, sj * bm, mu0);
    const double q = o.live ? 1.0 / (Cb + Rb * o.oneR) : 1.0; // (an empty layer: every quantity keeps its bits)
    const size_t at = (size_t)l * wrow + col;
    ws[at] = o.T * q;
    ws[wq + at] = (o.Em + o.R * Ub) * q;
    ws[2 * wq + at] = Rb;
    ws[3 * wq + at] = Ub;
    Ub = o.Ep + o.T * (Ub + Rb * o.Em) * q;
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
      const double val = (w_out * sca) * J;
      emi_out[at] = ACC ? emi_out[at] + val : val;
    }
  }
}
