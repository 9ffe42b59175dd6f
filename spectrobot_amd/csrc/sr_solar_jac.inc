// sr_solar_jac.inc -- sr_solar_jac_kernel.  Included by sr_solar_source.hip inside namespace sr, behind
// sr_solar_tile.inc (the tile product and its lane mapping), and by the host build tools/solar_jacobian_host.  Nothing
// else includes it.

// The solar attenuation in the Jacobians: the derivative of limb radiances to a column parameter THROUGH the optical depth
// of the solar source (sr_solar_source.inc).  The build's own definition -- the reference has no counterpart:
//   dtau[p][r][j] = sum_{k < n_k} du[p][r][k] A[k][j]           (du = d U / d x_p: any finite sign, mostly zeros)
//   jac[ray][slot[p]][j] (+)= - sum_{r < n_rows} q[ray][r][j] dtau[p][r][j]
// with q[ray][r] = d rad[ray] / d eps_r for emi[r] -> emi[r] + eps_r (solar rows of r), so that q dtau is the radiance's
// change through exp(-tau).  The first contraction is sr_solar_source_kernel's product, tile for tile
// (solar_tile_product<LIT = false> of sr_solar_tile.inc: no weights, every row counts), the k axis walked through host
// chunk lists per (parameter, row tile) (solar_jac_chunk_lists).
//
// A block takes 256 points, ONE parameter and a group of NR rays, and loops over the row tiles; a tile whose list is empty
// is skipped whole (block-uniform): it would have added exact zeros (q finite).  After a tile's MFMAs a lane holds rows
// kq + 4 r4 x its four consecutive points of dtau and multiplies them with q[ray][row][4 points] (32-byte loads, sixteen
// lanes 512 consecutive bytes of a row) into NR x 4 partial sums.  After the last tile the four lane groups of a column
// are added once, through LDS in the fixed order ((kq 0 + 1) + (2 + 3)), four rays per pass: lane group g adds and stores
// ray g of the pass, 0 - sum or base - sum (ACC), four consecutive points.  One writer per element, no atomics: the same
// call gives the same bits.  Padding as in sr_solar_source.inc: every load valid; a padded k or row carries du = 0 (a
// padded row's q is not read), a point beyond n_pts reads the last point and stores nothing, a ray beyond n_rays is
// neither read nor stored.  With ACC a parameter without any listed chunk leaves its row as it is, unread.
// Summation order of an element: per row the listed k ascending in the MFMA's own order, per lane group rows ascending,
// then the four groups: a K-term and an R-term sum with one product each between them.
template <int NR, bool ACC>
__global__ __launch_bounds__(256) void sr_solar_jac_kernel(const double *__restrict__ tab_abs, int n_k, int n_pts,
                                                           const double *__restrict__ du, int n_par, int n_rows,
                                                           const int *__restrict__ tile_off, const int *__restrict__ chunks,
                                                           const double *__restrict__ q, int n_rays, const int *__restrict__ par_slot,
                                                           double *__restrict__ jac, int n_jac_rows) {
  static_assert(NR % 4 == 0 && NR * 1024 <= 4 * kSolarBatch * 64, "the last reduction takes four rays per pass through s_u");
  __shared__ double s_u[kSolarBatch * 64];
  const int n_tiles = (n_rows + kSolarRows - 1) / kSolarRows, n_groups = (n_rays + NR - 1) / NR;
  int pb, item; // the (parameter, ray group) items of a point block on one XCD, one after the other: the parameters of a
                // ray group follow each other and read the same rows of q
  if (!limb_block((n_pts + 255) / 256, n_par * n_groups, pb, item)) return; // (block-uniform)
  const int par = item % n_par, ray0 = (item / n_par) * NR;
  const int t_lo = par * n_tiles;
  if (ACC && tile_off[t_lo] == tile_off[t_lo + n_tiles]) return; // no column at all: the row is left as it is
  const SolarLane ln(pb, n_pts);
  const double *u = du + (size_t)par * n_rows * n_k;
  double sum[NR][4];
#pragma unroll
  for (int y = 0; y < NR; ++y)
#pragma unroll
    for (int t = 0; t < 4; ++t) sum[y][t] = 0.0;

  for (int tile = 0; tile < n_tiles; ++tile) {
    const int c_lo = tile_off[t_lo + tile], c_hi = tile_off[t_lo + tile + 1];
    if (c_lo == c_hi) continue; // (block-uniform)
    const int row0 = tile * kSolarRows;
    v4d acc[4];
    solar_tile_product<false>(tab_abs, n_k, n_pts, u, nullptr, n_rows, row0, chunks, c_lo, c_hi, ln, s_u, acc);
    // register r4 of a lane is row kq + 4 r4 of the tile, its four column tiles four consecutive points
#pragma unroll
    for (int r4 = 0; r4 < 4; ++r4) {
      const int r = row0 + ln.kq + 4 * r4;
      if (r >= n_rows) continue; // (a padded row: its product is 0, its q does not exist)
#pragma unroll
      for (int y = 0; y < NR; ++y) {
        if (ray0 + y >= n_rays) continue; // (block-uniform)
        const SolarQuad qv = solar_load_quad(q + ((size_t)(ray0 + y) * n_rows + r) * n_pts, ln);
#pragma unroll
        for (int t = 0; t < 4; ++t) sum[y][t] += qv[t] * acc[t][r4];
      }
    }
  }

  // the four lane groups of a column, once: four rays per pass through s_u, lane group g adds and stores ray g of the pass
  const int slot = par_slot[par];
#pragma unroll
  for (int y0 = 0; y0 < NR; y0 += 4) {
    if (ray0 + y0 >= n_rays) break; // (block-uniform)
    __syncthreads();                // (the last batch, or the previous pass, has been consumed)
#pragma unroll
    for (int y = 0; y < 4; ++y)
#pragma unroll
      for (int t = 0; t < 4; ++t) s_u[(y * 256 + threadIdx.x) * 4 + t] = sum[y0 + y][t];
    __syncthreads();
    const int ray = ray0 + y0 + ln.kq;
    if (ray >= n_rays) continue; // (after the pass's last barrier)
    const double *part = s_u + ((size_t)ln.kq * 256 + ln.wave * 64 + ln.lo) * 4; // + 64 g: lane group g's partial sums of this ray
    double *out = jac + ((size_t)ray * n_jac_rows + slot) * n_pts + ln.p0;
    SolarQuad res;
#pragma unroll
    for (int t = 0; t < 4; ++t) res[t] = (part[t] + part[64 + t]) + (part[128 + t] + part[192 + t]);
    if (ln.whole) { // 32-byte stores: sixteen lanes write 512 consecutive bytes of the row
      SolarQuad base = SolarQuad{0.0, 0.0, 0.0, 0.0};
      if (ACC) base = solar_quad(out);
#pragma unroll
      for (int t = 0; t < 4; ++t) res[t] = base[t] - res[t];
      solar_quad(out, res);
    } else {
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        if (ln.p0 + t >= n_pts) continue;
        out[t] = (ACC ? out[t] : 0.0) - res[t];
      }
    }
  }
}
