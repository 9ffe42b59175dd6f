// sr_solar_source.inc -- sr_solar_source_kernel.  Included by sr_solar_source.hip inside namespace sr, and by the host
// build tools/solar_source_host.  Nothing else includes it.

// The single-scattering solar source of coefficient rows.  The build's own definition -- the reference has no counterpart:
//   tau[r][j] = sum_{k < n_k} U[r][k] A[k][j]                  (U >= 0: slant columns towards the sun, A: absorption rows)
//   T[r][j]   = exp(-tau[r][j])                                exactly 0 where w[r] == 0 or tau >= 700
//   emi[r][j] (+)= sca[src_row[r]][j] (w[r] sun[j] T[r][j])
// a matrix product [n_rows x n_k] . [n_k x n_pts] in fp64 with an exponential epilogue.
//
// A block takes a tile of kSolarRows = 16 rows and 256 consecutive grid points; a wave 64 of them as FOUR column tiles of
// v_mfma_f64_16x16x4: column c of column tile t is the point p0 + 4 c + t, so that a lane's four B operands of a chunk
// are four consecutive doubles of one row of A and the sixteen lanes of a k read 512 consecutive bytes of it -- and, in the
// epilogue, a lane writes four consecutive points of a row, sixteen lanes 512 bytes.  Operand layout: A[i][k] in lane
// 16 k + i, B[k][c] in lane 16 k + c, D[i][c] in lane 16 (i % 4) + c, register i / 4.
//
// The k axis is walked in chunks of four (one MFMA).  Per row tile the host lists the chunks in which any lit row of the
// tile has a column (tile_off, chunks: block-uniform, scalar loads); a chunk not listed would have added exact zeros to
// every accumulator, so the result does not depend on the lists.  The tile of U of the listed chunks goes through LDS
// once per block, kSolarBatch chunks at a time, in operand order (a conflict-free 8-byte read per lane and chunk).  Padding
// by sr_absorber_table's rule -- every load valid, 0 . finite contributes nothing: a k beyond n_k and a row beyond n_rows
// (or in shadow, w == 0: its optical depth is not evaluated) carry U = 0, a padded k reads row 0 of A, a point beyond
// n_pts the last point.  The blocks are dealt by limb_block(): the row tiles of a point block follow each other on one
// XCD, and the strip of A they share (n_k x 2 KB) is read from HBM once and by the other row tiles from that XCD's L2.
// One writer per element, no atomics: the same call gives the same bits.
// (kSolarRows, kSolarChunk and the lists: sr_solar_plan.hpp)
typedef double SolarQuad __attribute__((ext_vector_type(4), aligned(8))); // four consecutive doubles of a row: 8-byte aligned only
constexpr int kSolarBatch = 64; // chunks of four k whose U tile is in LDS at a time (32 KB)
static_assert(kSolarRows == 16 && kSolarChunk == 4, "the tile is one v_mfma_f64_16x16x4");

template <bool ACC, bool TRANS>
__global__ __launch_bounds__(256) void sr_solar_source_kernel(const double *__restrict__ tab_abs, int n_k, int n_pts,
                                                              const double *__restrict__ u, const double *__restrict__ w,
                                                              const int *__restrict__ src_row, int n_rows,
                                                              const int *__restrict__ tile_off, const int *__restrict__ chunks,
                                                              const double *__restrict__ sca_abs, const double *__restrict__ sun,
                                                              double *__restrict__ emi_out, double *__restrict__ trans_out) {
  __shared__ double s_u[kSolarBatch * 64];
  int pb, tile; // all row tiles of a point block on one XCD, one after the other
  if (!limb_block((n_pts + 255) / 256, (n_rows + kSolarRows - 1) / kSolarRows, pb, tile)) return; // (block-uniform)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lo = lane & 15, kq = lane >> 4;
  const int row0 = tile * kSolarRows, p0 = pb * 256 + wave * 64 + 4 * lo; // the lane's four points: p0 + t
  const bool whole = p0 + 3 < n_pts; // (false in the grid's last points only)
  int pj[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) pj[t] = min(p0 + t, n_pts - 1);
  const int c_lo = tile_off[tile], c_hi = tile_off[tile + 1];
  v4d acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = v4d{0.0, 0.0, 0.0, 0.0};
  for (int c0 = c_lo; c0 < c_hi; c0 += kSolarBatch) {
    const int nb = min(kSolarBatch, c_hi - c0), nb2 = (nb + 1) & ~1; // (walked in pairs: an odd batch ends on a chunk of zeros)
    __syncthreads();                                                 // (the previous batch has been consumed)
    for (int e = threadIdx.x; e < nb2 * 64; e += 256) {
      const int cl = e >> 6, i = (e >> 2) & 15, kk = e & 3; // four lanes read 32 consecutive bytes of a row of U
      double v = 0.0;
      if (cl < nb) {
        const int k = 4 * chunks[c0 + cl] + kk, r = row0 + i;
        if (k < n_k && r < n_rows && w[r] != 0.0) v = u[(size_t)r * n_k + k];
      }
      s_u[cl * 64 + kk * 16 + i] = v;
    }
    __syncthreads();
    double bn[2][4];
    auto fetch = [&](int cl) { // the B operands of the pair of chunks at cl, requested together
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int k = cl + h < nb ? 4 * chunks[c0 + cl + h] + kq : 0;
        const double *arow = tab_abs + (size_t)(k < n_k ? k : 0) * n_pts;
        if (whole) { // one 32-byte load: sixteen lanes read 512 consecutive bytes of the row
          const SolarQuad q = *reinterpret_cast<const SolarQuad *>(arow + p0);
#pragma unroll
          for (int t = 0; t < 4; ++t) bn[h][t] = q[t];
        } else {
#pragma unroll
          for (int t = 0; t < 4; ++t) bn[h][t] = arow[pj[t]];
        }
      }
    };
    fetch(0);
    for (int cl = 0; cl < nb2; cl += 2) {
      double b[2][4];
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int t = 0; t < 4; ++t) b[h][t] = bn[h][t];
      const double a0 = s_u[cl * 64 + lane], a1 = s_u[(cl + 1) * 64 + lane];
      if (cl + 2 < nb2) fetch(cl + 2); // the next pair in flight under this pair's products
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b[0][t], acc[t], 0, 0, 0);
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b[1][t], acc[t], 0, 0, 0);
    }
  }
  // epilogue: register r4 of a lane is row kq + 4 r4 of the tile, its four column tiles four consecutive points
#pragma unroll
  for (int r4 = 0; r4 < 4; ++r4) {
    const int r = row0 + kq + 4 * r4;
    if (r >= n_rows) continue;
    const double wr = w[r];
    if (wr == 0.0 && ACC && !TRANS) continue; // in shadow: the row is left as it is
    const double *sca = sca_abs + (size_t)src_row[r] * n_pts;
    const size_t at0 = (size_t)r * n_pts + p0;
    SolarQuad tr, e;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const double tau = acc[t][r4];
      tr[t] = (wr != 0.0 && tau < 700.0) ? exp_bounded(-tau) : 0.0;
      e[t] = wr != 0.0 ? sca[pj[t]] * ((wr * sun[pj[t]]) * tr[t]) : 0.0;
    }
    if (whole) { // 32-byte stores: sixteen lanes write 512 consecutive bytes of the row
      if (TRANS) *reinterpret_cast<SolarQuad *>(trans_out + at0) = tr;
      if (wr == 0.0 && ACC) continue;
      SolarQuad *out = reinterpret_cast<SolarQuad *>(emi_out + at0);
      if (ACC) {
        const SolarQuad base = *out;
#pragma unroll
        for (int t = 0; t < 4; ++t) e[t] = base[t] + e[t];
      }
      *out = e;
    } else {
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        if (p0 + t >= n_pts) continue;
        if (TRANS) trans_out[at0 + t] = tr[t];
        if (wr == 0.0 && ACC) continue;
        if (ACC) emi_out[at0 + t] += e[t];
        else emi_out[at0 + t] = e[t];
      }
    }
  }
}
