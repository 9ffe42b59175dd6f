// sr_lowres_weights_tab.inc -- sr_lowres_weights_tab_kernel.  Included by sr_ops.hip inside namespace sr, and by the host
// build tools/ils_host.

// The weights of a TABULATED instrument line shape (sr_set_ils): sr_lowres_weights_kernel with the Gaussian replaced by
// the cubic Hermite interpolant phi^ of n_tab knots at the reduced offsets t_lo + k h, zero outside [t_lo, t_hi].  The same
// grid, block, searches, writes (W, Wt with the zero columns of its last tile, range, the three tables with INSTR) and
// layouts: everything downstream reads the tables as it reads the Gaussian's.
//   window of band b: f + t_lo w <= x_i <= f + t_hi w on the fp64 nm values (n_sigma plays no part)
//   p_i = g_i^2 1e-7 c_i:   W_i = p_i phi^(t_i) / w,   W^f_i = -p_i phi^'(t_i) / w^2,   W^w_i = -p_i (phi^ + t_i phi^') / w
// (d / d centre per nm and d / d ln width of phi^((x - f) / w) / w, the window's membership held fixed; the derivative
// tables on their own, not W times a factor: phi^ may vanish where phi^' does not).
// tab [n_shapes][n_tab][2]: the knot phi_k and its slope PER KNOT INTERVAL d_k = h m_k ((phi_(k+1) - phi_(k-1)) / 2 inside,
// the one-sided difference at the two ends; formed once on the host, sr_set_ils) -- a few KB read with plain loads, resident
// in L2; n_shapes = 1: every band the same table, else table b for band b.  On interval k, s = (t - t_lo) / h - k:
//   phi^  = (1 + 2 s)(1 - s)^2 phi_k + s (1 - s)^2 d_k + s^2 (3 - 2 s) phi_(k+1) + s^2 (s - 1) d_(k+1)
//   phi^' = (6 s (s - 1) (phi_k - phi_(k+1)) + (3 s - 1)(s - 1) d_k + s (3 s - 2) d_(k+1)) / h
// k is clamped to [0, n_tab - 2]: a point of the window whose rounded t falls a rounding outside the table, and t = t_hi
// itself (the last knot, s = 1), stay on the table's end intervals.
template <bool INSTR>
__global__ __launch_bounds__(256) void sr_lowres_weights_tab_kernel(int n_pts, int g_lo, double w0, double gstep,
                                                                    const double *__restrict__ cen, const double *__restrict__ wid,
                                                                    const double *__restrict__ tab, int n_shapes, int n_tab,
                                                                    double t_lo, double t_hi, int n_bands,
                                                                    double *__restrict__ W,    // [n_bands][n_pts]
                                                                    int *__restrict__ range,   // [n_bands][2]: j_lo, j_hi (exclusive)
                                                                    double *__restrict__ Wt) { // [gridDim.y / 16][n_pts][16]
  const int b = blockIdx.y;
  if (b >= n_bands) { // the zero columns that fill the last tile of Wt
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n_pts) {
      const size_t at = ((size_t)(b >> 4) * n_pts + j) * 16 + (b & 15);
      Wt[at] = 0.0;
      if constexpr (INSTR) {
        const size_t tab_wt = (size_t)(gridDim.y >> 4) * n_pts * 16; // a table of Wt
        Wt[tab_wt + at] = Wt[2 * tab_wt + at] = 0.0;
      }
    }
    return;
  }
  const double f = cen[b], w = wid[b];
  const double lo = f + t_lo * w, hi = f + t_hi * w;
  const double h = (t_hi - t_lo) / (double)(n_tab - 1);
  const double *shape = tab + (n_shapes > 1 ? (size_t)b * n_tab * 2 : 0);
  auto gcm = [&](int i) { return w0 + (double)(g_lo + n_pts - 1 - i) * gstep; }; // nm index i <-> cm-1 index n-1-i
  auto xnm = [&](int i) { return 1.e7 / gcm(i); };
  // first i with x >= lo, first i with x > hi (x ascending in i): the two searches of sr_lowres_weights_kernel
  int i0, i1;
  {
    int a = 0, c = n_pts;
    while (a < c) { int m = (a + c) >> 1; if (xnm(m) < lo) a = m + 1; else c = m; }
    i0 = a;
    a = 0; c = n_pts;
    while (a < c) { int m = (a + c) >> 1; if (xnm(m) <= hi) a = m + 1; else c = m; }
    i1 = a; // selected: i0 .. i1-1; fewer than two points: no trapezoid
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const bool any = i1 - i0 >= 2;
    range[2 * b] = any ? n_pts - i1 : 0;       // cm-1 indices j = n_pts - 1 - i, i in [i0, i1)
    range[2 * b + 1] = any ? n_pts - i0 : 0;
  }
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_pts) return;
  const int i = n_pts - 1 - j;
  double wgt = 0.0;
  [[maybe_unused]] double wgt_f = 0.0, wgt_w = 0.0;
  if (i >= i0 && i < i1 && i1 - i0 >= 2) {
    const double g = gcm(i), x = 1.e7 / g, t = (x - f) / w;
    const double q = (t - t_lo) / h;
    const int k = min(max((int)floor(q), 0), n_tab - 2); // the clamp: see above
    const double s = q - (double)k;
    const double p0 = shape[2 * k], d0 = shape[2 * k + 1], p1 = shape[2 * k + 2], d1 = shape[2 * k + 3];
    const double r = 1.0 - s;
    const double phi = ((1.0 + 2.0 * s) * (r * r)) * p0 + (s * (r * r)) * d0 + ((s * s) * (3.0 - 2.0 * s)) * p1 - ((s * s) * r) * d1;
    const double xl = i > i0 ? xnm(i - 1) : x, xr = i + 1 < i1 ? xnm(i + 1) : x;
    const double p = ((g * g) * 1.e-7) * ((xr - xl) / 2.0);
    wgt = p * phi / w;
    if constexpr (INSTR) {
      const double dphi = ((6.0 * s * r) * (p1 - p0) - ((3.0 * s - 1.0) * r) * d0 + (s * (3.0 * s - 2.0)) * d1) / h;
      wgt_f = -(p * dphi) / (w * w);
      wgt_w = -(p * (phi + t * dphi)) / w;
    }
  }
  const size_t at = (size_t)b * n_pts + j, at_t = ((size_t)(b >> 4) * n_pts + j) * 16 + (b & 15);
  W[at] = wgt;
  Wt[at_t] = wgt;
  if constexpr (INSTR) {
    const size_t tab_w = (size_t)n_bands * n_pts, tab_wt = (size_t)(gridDim.y >> 4) * n_pts * 16; // a table of W, of Wt
    W[tab_w + at] = wgt_f;
    W[2 * tab_w + at] = wgt_w;
    Wt[tab_wt + at_t] = wgt_f;
    Wt[2 * tab_wt + at_t] = wgt_w;
  }
}
