// sr_diffuse_jac.inc -- sr_diffuse_tangent_kernel and sr_diffuse_contract_kernel.  Included by sr_solar_source.hip inside
// namespace sr, behind sr_diffuse_source.inc (DiffuseLayer, diffuse_layer, diffuse_boundary, diffuse_sums), and by the
// host build tools/diffuse_jacobian_host.  Nothing else includes it.

// The diffuse rows in the Jacobians: the tangent of sr_diffuse_field_kernel's solar J along column parameters, and its product
// with the radiances' derivative to J.  The build's own definition -- the reference has no counterpart (DESIGN.md 4.11c).
// In the notation of sr_diffuse_source.inc a parameter x_p moves a layer's three sums and its source through
//   d t_g[l] = dv[p][g][l] A[g N + l][j],   d D_l = D_l dlnbeam[p][l][j],   d Ub_0 = Ub_0 dlnbeam[p][N][j]
// (dlnbeam null: the beam is held fixed) and dJ[p][l][j] is the tangent of J_l of the function AS BUILT, statement by
// statement, every quantity of diffuse_layer and of the two sweeps with its tangent beside it:
//   co = max(al / dtau, 2^-52)   has tangent 0 where the floor holds (al / dtau <= 2^-52)
//   g = 0 where sp == 0          has tangent 0 there
//   a layer with dtau == 0 passes light through whatever dv says: every operator tangent is 0, q = 1 has tangent 0
// with the operators' tangents taken of their even forms in k (diffuse_layer_tangent, below).
// Then   jac[ray][slot[p]][j] (+)= sum_l q[ray][l][j] dJ[p][l][j],   l ascending from 0.0, one product and one addition
// per layer, the base added last (ACC).
//
// sr_diffuse_tangent_kernel<NP, OPT> (OPT, a direction in ssa, asym and the surface albedo where the text below says dv:
// at the kernel; tools/diffuse_optics_host is its host build): one thread per grid point, 256 points per block, a block
// takes a point block and a tile of NP parameters (limb_block deals them; the tiles of a point block follow each other on
// one XCD and read the same rows).
// The base quantities of a layer are made once per block (diffuse_layer, unchanged) and held in registers; per parameter
// of the tile the layer's operator tangents come from
//   outside the parameter's layer range [mask[2 p], mask[2 p + 1]): d t_g = 0 for every gas, so dR = dT = d(1 - R) =
//     d(1 - R - T) = 0 and dE+- = E+- dlnbeam (E+- is linear in D): two products, no sqrt / exp / expm1 / division;
//   inside it: diffuse_layer_tangent, the closed forms differentiated term by term (block-uniform branch);
// and the adding recurrences carry dRb and dUb upward (dCb = -dRb; the forms: at the step itself).  The upward sweep leaves in the workspace, per tile,
// ws [3 + 4 NP][N][ws_stride]: T q, (E- + R Ub) q, Rb and per parameter the tangents of these and of Ub; the downward sweep reads
// them back and carries dF+, dF- and writes dJ rows: dj[(p - dj_par0) N + l][j - dj_joff] with row pitch dj_stride
// (the caller's dj_out, or a workspace for the contraction).  A parameter slot beyond par_hi repeats the tile's last
// parameter and stores no dJ; a point beyond p_hi reads the last point and stores no dJ (its workspace column is its own).
//
// sr_diffuse_contract_kernel<NR, NP, ACC>: one thread per grid point, a block takes 256 points, NR rays and NP parameters:
// an NR x NP register tile, the layer sum in fixed order.  q is read once per parameter tile, dJ once per ray tile.
// One writer per element, no atomics: the same call gives the same bits, and a parameter's rows do not depend on the
// tile it stands in nor a point's on its chunk.
struct DiffuseTan { double R, T, Ep, Em, absb; }; // (d(1 - R) = -dR is not kept)

// cosh and sinh of x = sqrt(y) as the even functions the layer operators are made of, each times e = exp(-x), for y < 4:
//   Sh = e sinh(x) / x, Ch = e cosh(x), c2 = e (cosh(x) - 1) / y, W = e (cosh(x) - sinh(x) / x) / y = 2 e d(sinh(x) / x) / dy,
//   c2p = e d((cosh(x) - 1) / y) / dy
// by their power series in y (fourteen terms of non-negative addends: the next is below 1e-20 of the sum).
struct DiffuseEven { double e, Sh, Ch, c2, W, c2p; };
__device__ __forceinline__ DiffuseEven diffuse_even(double y) {
  DiffuseEven o;
  o.e = exp(-sqrt(y));
  double a = 1.0, S = 0.0, c2 = 0.0, W = 0.0, c2p = 0.0; // a = y^n / (2 n + 1)!
#pragma unroll
  for (int n = 0; n < 14; ++n) {
    S += a;
    c2 += a * (1.0 / (2 * n + 2));
    W += a * (1.0 / (2 * n + 3));
    c2p += a * (1.0 / (2.0 * (2 * n + 3) * (2 * n + 4)));
    a *= y * (1.0 / ((2.0 * n + 2) * (2 * n + 3)));
  }
  o.Sh = o.e * S, o.c2 = o.e * c2, o.W = o.e * W, o.c2p = o.e * c2p;
  o.Ch = o.e * (1.0 + y * c2);
  return o;
}

// The tangent of diffuse_layer's results along (dsp, dal, dsg, dD).  The closed forms of diffuse_layer are built on
// sqrt(co), whose tangent d co / (2 sqrt(co)) is as large as 1e7 d co near co's floor while R, T and E+- are smooth in co:
// differentiated term by term they would cancel to eps 1e7.  The same operators are even functions of k, so the tangent
// is taken of their even forms, with y = k^2 dtau^2, x = sqrt(y), Delta = cosh x + gamma1 dtau sinh(x) / x:
//   T = 1 / Delta,  R = gamma2 dtau (sinh(x) / x) / Delta,  1 - R - T = d dtau An
//   E+ + E- = omega D (1 - R - T) / d  = D (omega dtau) An,   An = (s dtau (cosh x - 1) / y + sinh(x) / x) / Delta
//   E+ - E- = -omega D sqrt3 g mu0 (1 - T + R) / s = -sqrt3 mu0 D (omega g dtau) Bn,   Bn = (d dtau (cosh x - 1) / y + sinh(x) / x) / Delta
// (the particular solution of a uniform source, (S+ + S-) / d and (S+ - S-) / s, less what the layer reflects and transmits
// of it): sums of non-negative terms, every quantity times exp(-x) so that a thick layer does not overflow.  And every
// coefficient enters as its product with dtau, which above the floor is one of the layer's own sums -- co dtau = al,
// omega dtau = sp, omega g dtau = sg -- so that its tangent is that sum's (an absorber's column moves co by dal / dtau,
// many times its share of the light; the products stand still).  Under the floor co is the constant 2^-52.
__device__ __forceinline__ DiffuseTan diffuse_layer_tangent(double sp, double al, double sg, double D, double mu0, double dsp,
                                                            double dal, double dsg, double dD) {
  const double kSqrt3 = 1.7320508075688772;
  DiffuseTan t;
  t.R = 0.0, t.T = 0.0, t.Ep = 0.0, t.Em = 0.0, t.absb = 0.0;
  const double dtau = sp + al;
  if (!(dtau > 0.0)) return t;
  const double ddtau = dsp + dal;
  const bool fl = !(al / dtau > 0x1p-52); // the floor holds
  const double om = 1.0 - 0x1p-52;        // (under the floor)
  const double cd = fl ? 0x1p-52 * dtau : al, dcd = fl ? 0x1p-52 * ddtau : dal; // co dtau
  const double od = fl ? om * dtau : sp, dod = fl ? om * ddtau : dsp;           // omega dtau
  const bool sc = sp > 0.0;
  const double g = sc ? sg / sp : 0.0, dg = sc ? (dsg - g * dsp) / sp : 0.0;
  const double go = fl ? g * od : (sc ? sg : 0.0), dgo = fl ? dg * od + g * dod : (sc ? dsg : 0.0); // omega g dtau
  const double bd = kSqrt3 * cd, dbd = kSqrt3 * dcd;                     // d dtau
  const double bs = kSqrt3 * (dtau - go), dbs = kSqrt3 * (ddtau - dgo);  // s dtau
  const double y = bd * bs, dy = dbd * bs + bd * dbs;
  const double a1 = 0.5 * (bs + bd), da1 = 0.5 * (dbs + dbd);                              // gamma1 dtau
  const double a2 = 0.5 * (kSqrt3 * (od - go)), da2 = 0.5 * (kSqrt3 * (dod - dgo));        // gamma2 dtau
  double An, Bn, dAn, dBn;
  if (y < 4.0) { // the series; tangents of the functions themselves, each times e (the factor e^x is common to all)
    const DiffuseEven v = diffuse_even(y);
    const double rD = 1.0 / (v.Ch + a1 * v.Sh);                     // 1 / (e Delta)
    const double dSh = 0.5 * (v.W * dy);                            // e d(sinh(x) / x)
    const double dDh = 0.5 * (v.Sh * dy) + (da1 * v.Sh + a1 * dSh); // e d Delta
    const double T = v.e * rD, R = a2 * v.Sh * rD;
    t.T = -(T * dDh * rD);
    t.R = ((da2 * v.Sh + a2 * dSh) - R * dDh) * rD;
    const double c2y = v.c2p * dy;
    An = (bs * v.c2 + v.Sh) * rD, Bn = (bd * v.c2 + v.Sh) * rD;
    dAn = (((dbs * v.c2 + bs * c2y) + dSh) - An * dDh) * rD;
    dBn = (((dbd * v.c2 + bd * c2y) + dSh) - Bn * dDh) * rD;
  } else { // a thick layer: e d(f) grows as x f d ln(dtau) in numerator and denominator alike and would cancel to eps x;
           // here the tangents are those of the SCALED functions e f, in which dtau is left in e^-x and e^-2x alone
    const double x = sqrt(y), dx = 0.5 * dy / x, e = exp(-x), e2 = e * e;
    const double Ch = 0.5 * (1.0 + e2), dCh = -(e2 * dx);
    const double Sh = 0.5 * (1.0 - e2) / x, dSh = (e2 * dx - Sh * dx) / x;
    const double c2 = (Ch - e) / y, dc2 = ((dCh + e * dx) - c2 * dy) / y;
    const double rD = 1.0 / (Ch + a1 * Sh), dDh = dCh + (da1 * Sh + a1 * dSh);
    const double T = e * rD, R = a2 * Sh * rD;
    t.T = -((e * dx + T * dDh) * rD);
    t.R = ((da2 * Sh + a2 * dSh) - R * dDh) * rD;
    An = (bs * c2 + Sh) * rD, Bn = (bd * c2 + Sh) * rD;
    dAn = (((dbs * c2 + bs * dc2) + dSh) - An * dDh) * rD;
    dBn = (((dbd * c2 + bd * dc2) + dSh) - Bn * dDh) * rD;
  }
  t.absb = dbd * An + bd * dAn;
  const double des = (dD * od + D * dod) * An + D * od * dAn;
  const double c = kSqrt3 * mu0;
  const double ded = -(c * ((dD * go + D * dgo) * Bn + D * go * dBn));
  t.Ep = 0.5 * (des + ded);
  t.Em = 0.5 * (des - ded);
  return t;
}

// OPT false: a direction in the columns, dv [n_par][n_gas][n_layers].  OPT true: a direction in the optics (DESIGN.md
// 4.11d) -- in dv's place dopt [n_par][kDiffuseOpt]: the per-gas coefficients' tangents [3][kDiffuseGases] (d(ssa (1 - f)),
// d(1 - ssa), d(ssa (asym - f)), zeros beyond n_gas) and then the albedo's, block-uniform (scalar loads); inside a
// parameter's layer range the three sums move with the coefficients' tangents on the products t_g = v a that diffuse_sums
// forms, and the boundary starts with dRb_0 = dalb, dUb_0 = Ub_0 dlnbeam + dalb max(mu0, 0) sun beam[N].
template <int NP, bool OPT = false>
__global__ __launch_bounds__(256) void sr_diffuse_tangent_kernel(const double *__restrict__ tab_abs, int n_gas, int n_layers, int n_pts,
                                                                 int p_lo, int p_hi, int par_lo, int par_hi,
                                                                 const double *__restrict__ v, const double *__restrict__ dv,
                                                                 const double *__restrict__ coef, const int *__restrict__ mask,
                                                                 const double *__restrict__ beam, const double *__restrict__ sun,
                                                                 const double *__restrict__ dlnbeam, double mu0, double albedo,
                                                                 double *__restrict__ ws, int ws_stride, double *__restrict__ dj,
                                                                 int dj_stride, int dj_joff, int dj_par0) {
  int pb, tile;
  if (!limb_block((p_hi - p_lo + 255) / 256, (par_hi - par_lo + NP - 1) / NP, pb, tile)) return; // (block-uniform)
  const int col = pb * 256 + threadIdx.x, j = p_lo + col;
  const bool live = j < p_hi;
  const size_t np = (size_t)n_pts, jj = (size_t)min(j, p_hi - 1);
  const size_t wrow = (size_t)ws_stride, wq = (size_t)n_layers * wrow; // ws [tile][3 + 4 NP][n_layers][ws_stride]
  double *w0 = ws + (size_t)tile * (3 + 4 * NP) * wq;
  const double *cs = coef, *ca = coef + kDiffuseGases, *cg = coef + 2 * kDiffuseGases;
  const double sj = sun[jj];
  const size_t brow = (size_t)(n_layers + 1) * np; // dlnbeam [n_par][n_layers + 1][n_pts]
  int par[NP], m_lo[NP], m_hi[NP];
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    par[i] = min(par_lo + tile * NP + i, par_hi - 1);
    m_lo[i] = mask[2 * par[i]], m_hi[i] = mask[2 * par[i] + 1];
  }

  // ---- bottom up ----
  double Rb, Cb, Ub;
  diffuse_boundary(albedo, mu0, sj, beam[(size_t)n_layers * np + jj], Rb, Cb, Ub);
  double dRb[NP], dUb[NP]; // (Cb = 1 - Rb: its tangent is -dRb and is not carried)
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    dRb[i] = 0.0;
    dUb[i] = dlnbeam ? Ub * dlnbeam[(size_t)par[i] * brow + (size_t)n_layers * np + jj] : 0.0;
    if (OPT) { // the albedo's direction: Rb_0 = albedo, Ub_0 = albedo max(mu0, 0) sun beam[N] (diffuse_boundary)
      const double dalb = dv[(size_t)par[i] * kDiffuseOpt + 3 * kDiffuseGases];
      dRb[i] = dalb;
      dUb[i] += dalb * (fmax(mu0, 0.0) * (sj * beam[(size_t)n_layers * np + jj]));
    }
  }
  for (int l = 0; l < n_layers; ++l) {
    double a[kDiffuseGases];
#pragma unroll
    for (int g = 0; g < kDiffuseGases; ++g) a[g] = tab_abs[((size_t)(g < n_gas ? g : 0) * n_layers + l) * np + jj];
    const double bm = beam[(size_t)l * np + jj];
    const DiffuseSums s = diffuse_sums(v, coef, n_gas, n_layers, l, a);
    const double sp = s.sp, al = s.al, sg = s.sg;
    double tg[kDiffuseGases]; // (OPT) diffuse_sums' own products
    if (OPT) {
#pragma unroll
      for (int g = 0; g < kDiffuseGases; ++g) tg[g] = v[(g < n_gas ? g : 0) * n_layers + l] * a[g];
    }
    const double D = sj * bm;
    const DiffuseLayer o = diffuse_layer(sp, al, sg, D, mu0);
    const double den = Cb + Rb * o.oneR;
    const double q = o.live ? 1.0 / den : 1.0;
    const size_t at = (size_t)l * wrow + col;
    const double tq = o.T * q, cn = o.Em + o.R * Ub, wv = Ub + Rb * o.Em;
    const double cn2 = o.oneR * Cb + Rb * o.absb * (o.oneR + o.T);
    const double z = (Cb + Rb * o.absb) * q;
    w0[at] = tq;
    w0[wq + at] = cn * q;
    w0[2 * wq + at] = Rb;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const double dlb = dlnbeam ? dlnbeam[(size_t)par[i] * brow + (size_t)l * np + jj] : 0.0;
      DiffuseTan t;
      if (l >= m_lo[i] && l < m_hi[i]) { // (block-uniform) inside the parameter's layers: the closed forms' tangent
        double dsp = 0.0, dal = 0.0, dsg = 0.0;
        if (OPT) {
          const double *dc = dv + (size_t)par[i] * kDiffuseOpt;
#pragma unroll
          for (int g = 0; g < kDiffuseGases; ++g) {
            dsp += dc[g] * tg[g];
            dal += dc[kDiffuseGases + g] * tg[g];
            dsg += dc[2 * kDiffuseGases + g] * tg[g];
          }
        } else {
          const double *dvp = dv + (size_t)par[i] * n_gas * n_layers;
#pragma unroll
          for (int g = 0; g < kDiffuseGases; ++g) {
            const double dt = (g < n_gas ? dvp[g * n_layers + l] : 0.0) * a[g];
            dsp += cs[g] * dt;
            dal += ca[g] * dt;
            dsg += cg[g] * dt;
          }
        }
        t = diffuse_layer_tangent(sp, al, sg, D, mu0, dsp, dal, dsg, D * dlb);
      } else { // outside: the operators stand still, the sources follow the beam
        t.R = 0.0, t.T = 0.0, t.absb = 0.0;
        t.Ep = o.Ep * dlb, t.Em = o.Em * dlb;
      }
      // The adding step's tangents, in the forms that stay sums of small terms both under a thick layer (T -> 0) and in
      // a lossless column (1 - R - T -> 0, Rb -> 1).  With z = 1 - T q Rb = (Cb + Rb (1 - R - T)) q and dCb = -dRb:
      //   dq      = q^2 (dRb R + Rb dR)
      //   d(T q)  = q (dT + T q (dRb R + Rb dR))  =  q (T q R dRb - dR z - d(1 - R - T)):  the one whose addends are smaller
      //   dUb'    = dE+ + T dw q + w d(T q),   w = Ub + Rb E-
      //   dRb'    = T Rb d(T q) + (dR z - T Rb q d(1 - R - T)) + T^2 q dRb
      const double dq = o.live ? (q * q) * (dRb[i] * o.R + Rb * t.R) : 0.0;
      const double bA = t.T + tq * (dRb[i] * o.R + Rb * t.R), mA = fabs(t.T) + tq * (fabs(dRb[i]) * o.R + Rb * fabs(t.R));
      const double bB = (tq * o.R * dRb[i] - t.R * z) - t.absb, mB = (tq * o.R * fabs(dRb[i]) + fabs(t.R) * z) + fabs(t.absb);
      const double dtq = q * (mA <= mB ? bA : bB);
      double *wi = w0 + (size_t)(3 + 4 * i) * wq;
      wi[at] = dtq;
      wi[wq + at] = (t.Em + (t.R * Ub + o.R * dUb[i])) * q + cn * dq;
      wi[2 * wq + at] = dRb[i];
      wi[3 * wq + at] = dUb[i];
      const double dwv = dUb[i] + (dRb[i] * o.Em + Rb * t.Em);
      dUb[i] = t.Ep + (o.T * dwv * q + wv * dtq);
      dRb[i] = o.T * Rb * dtq + ((t.R * z - o.T * Rb * q * t.absb) + o.T * o.T * q * dRb[i]);
    }
    Ub = o.Ep + o.T * wv * q;
    Cb = cn2 * q;
    Rb = o.R + o.T * o.T * Rb * q;
  }

  // ---- top down ----
  const double kJ = 1.7320508075688772 / (8.0 * 3.141592653589793);
  double fm = 0.0, dfp[NP], dfm[NP];
#pragma unroll
  for (int i = 0; i < NP; ++i) dfp[i] = dUb[i], dfm[i] = 0.0;
  for (int l = n_layers - 1; l >= 0; --l) {
    const size_t at = (size_t)l * wrow + col;
    const double tq = w0[at], cq = w0[wq + at], rb = w0[2 * wq + at];
    const double fm_l = tq * fm + cq;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const double *wi = w0 + (size_t)(3 + 4 * i) * wq;
      const double dtq = wi[at], dcq = wi[wq + at], drb = wi[2 * wq + at], dub = wi[3 * wq + at];
      const double dfm_l = (dtq * fm + tq * dfm[i]) + dcq;
      const double dfp_l = dub + (drb * fm_l + rb * dfm_l);
      const double dJ = kJ * ((dfp_l + dfm_l) + (dfp[i] + dfm[i]));
      dfp[i] = dfp_l, dfm[i] = dfm_l;
      const int p = par_lo + tile * NP + i;
      if (live && p < par_hi) dj[((size_t)(p - dj_par0) * n_layers + l) * (size_t)dj_stride + (size_t)(j - dj_joff)] = dJ;
    }
    fm = fm_l;
  }
}

template <int NR, int NP, bool ACC>
__global__ __launch_bounds__(256) void sr_diffuse_contract_kernel(const double *__restrict__ q, int n_rays, int n_layers, int n_pts,
                                                                  int p_lo, int p_hi, int par_lo, int par_hi,
                                                                  const double *__restrict__ dj, int dj_stride, int dj_joff,
                                                                  int dj_par0, const int *__restrict__ par_slot,
                                                                  double *__restrict__ jac, int n_jac_rows) {
  const int n_pt = (par_hi - par_lo + NP - 1) / NP, n_rt = (n_rays + NR - 1) / NR;
  int pb, item; // the parameter tiles of a ray tile follow each other and read the same rows of q
  if (!limb_block((p_hi - p_lo + 255) / 256, n_pt * n_rt, pb, item)) return; // (block-uniform)
  const int j = p_lo + pb * 256 + threadIdx.x;
  const bool live = j < p_hi;
  const size_t np = (size_t)n_pts, jj = (size_t)min(j, p_hi - 1);
  const int par0 = par_lo + (item % n_pt) * NP, ray0 = (item / n_pt) * NR;
  int par[NP], ray[NR];
#pragma unroll
  for (int i = 0; i < NP; ++i) par[i] = min(par0 + i, par_hi - 1);
#pragma unroll
  for (int y = 0; y < NR; ++y) ray[y] = min(ray0 + y, n_rays - 1);
  double sum[NR][NP];
#pragma unroll
  for (int y = 0; y < NR; ++y)
#pragma unroll
    for (int i = 0; i < NP; ++i) sum[y][i] = 0.0;
  for (int l = 0; l < n_layers; ++l) {
    double d[NP], qv[NR];
#pragma unroll
    for (int i = 0; i < NP; ++i) d[i] = dj[((size_t)(par[i] - dj_par0) * n_layers + l) * (size_t)dj_stride + (jj - (size_t)dj_joff)];
#pragma unroll
    for (int y = 0; y < NR; ++y) qv[y] = q[((size_t)ray[y] * n_layers + l) * np + jj];
#pragma unroll
    for (int y = 0; y < NR; ++y)
#pragma unroll
      for (int i = 0; i < NP; ++i) sum[y][i] += qv[y] * d[i];
  }
  if (!live) return;
#pragma unroll
  for (int y = 0; y < NR; ++y) {
    if (ray0 + y >= n_rays) continue; // (block-uniform)
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      if (par0 + i >= par_hi) continue; // (block-uniform)
      double *out = jac + ((size_t)ray[y] * n_jac_rows + par_slot[par[i]]) * np + j;
      *out = ACC ? *out + sum[y][i] : sum[y][i];
    }
  }
}
