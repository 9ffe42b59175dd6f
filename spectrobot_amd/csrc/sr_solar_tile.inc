// sr_solar_tile.inc -- what the two MFMA kernels of the solar unit share: sr_solar_source_kernel (sr_solar_source.inc) and
// sr_solar_jac_kernel (sr_solar_jac.inc).  Included by sr_solar_source.hip inside namespace sr ahead of both, and by the
// host builds tools/solar_source_host and tools/solar_jacobian_host.  Nothing else includes it.
//
// The tile product: acc = X[row0 .. row0 + 15][k] . A[k][256 points] in fp64 over the listed chunks of k.  A block takes
// kSolarRows = 16 rows and 256 consecutive grid points; a wave 64 of them as FOUR column tiles of v_mfma_f64_16x16x4:
// column c of column tile t is the point p0 + 4 c + t, so that a lane's four B operands of a chunk are four consecutive
// doubles of one row of A and the sixteen lanes of a k read 512 consecutive bytes of it -- and, in an epilogue, a lane
// holds four consecutive points of a row.  Operand layout: A[i][k] in lane 16 k + i, B[k][c] in lane 16 k + c, D[i][c]
// in lane 16 (i % 4) + c, register i / 4: register r4 of a lane is row kq + 4 r4 of the tile.
// (kSolarRows, kSolarChunk and the lists: sr_solar_plan.hpp)
typedef double SolarQuad __attribute__((ext_vector_type(4), aligned(8))); // four consecutive doubles of a row: 8-byte aligned only
constexpr int kSolarBatch = 64; // chunks of four k whose X tile is in LDS at a time (32 KB)
static_assert(kSolarRows == 16 && kSolarChunk == 4, "the tile is one v_mfma_f64_16x16x4");

// A thread's place in its block's 256 points: the lane's four points are p0 + t.
struct SolarLane {
  int lane, wave, lo, kq, p0;
  bool whole; // all four points exist (false in the grid's last points only)
  int pj[4];  // the points clamped to the grid: every load valid
  __device__ __forceinline__ SolarLane(int pb, int n_pts) {
    lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lo = lane & 15, kq = lane >> 4;
    p0 = pb * 256 + wave * 64 + 4 * lo;
    whole = p0 + 3 < n_pts;
#pragma unroll
    for (int t = 0; t < 4; ++t) pj[t] = min(p0 + t, n_pts - 1);
  }
};

// Four consecutive doubles of a row as one 32-byte access (sixteen lanes: 512 consecutive bytes of the row).
__device__ __forceinline__ SolarQuad solar_quad(const double *at) { return *reinterpret_cast<const SolarQuad *>(at); }
__device__ __forceinline__ void solar_quad(double *at, const SolarQuad &v) { *reinterpret_cast<SolarQuad *>(at) = v; }

// The lane's four points of a row of an input: one 32-byte load if they all exist, else four loads at the clamped points.
// (The stores are the kernels' own: where a lane's points do not all exist they go point by point, inside the grid only,
// and each kernel has its own rule for what it leaves as it is.)
__device__ __forceinline__ SolarQuad solar_load_quad(const double *__restrict__ row, const SolarLane &ln) {
  if (ln.whole) return solar_quad(row + ln.p0);
  SolarQuad v;
#pragma unroll
  for (int t = 0; t < 4; ++t) v[t] = row[ln.pj[t]];
  return v;
}

// acc[t][r4] = sum over the chunks c_lo .. c_hi - 1 of the lists (block-uniform) of x[row0 + kq + 4 r4][k] A[k][p0 + t].
// The k axis is walked in chunks of four (one MFMA); a chunk not listed would have added exact zeros to every
// accumulator.  The tile of x of the listed chunks goes through LDS (s_u [kSolarBatch * 64]) once per block, kSolarBatch
// chunks at a time, in operand order (a conflict-free 8-byte read per lane and chunk).  Padding by sr_absorber_table's
// rule -- every load valid, 0 . finite contributes nothing: a k beyond n_k and a row beyond n_rows carry x = 0, a padded k
// reads row 0 of A, a point beyond n_pts the last point.  LIT: a row with w == 0 (in shadow) carries x = 0 too; without
// it w is never read.  Every thread of the block calls it (barriers); after it s_u is the caller's behind one more barrier.
template <bool LIT>
__device__ __forceinline__ void solar_tile_product(const double *__restrict__ tab_abs, int n_k, int n_pts,
                                                   const double *__restrict__ x, const double *__restrict__ w, int n_rows, int row0,
                                                   const int *__restrict__ chunks, int c_lo, int c_hi, const SolarLane &ln,
                                                   double *s_u, v4d (&acc)[4]) {
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = v4d{0.0, 0.0, 0.0, 0.0};
  for (int c0 = c_lo; c0 < c_hi; c0 += kSolarBatch) {
    const int nb = min(kSolarBatch, c_hi - c0), nb2 = (nb + 1) & ~1; // (walked in pairs: an odd batch ends on a chunk of zeros)
    __syncthreads();                                                 // (the previous batch has been consumed)
    for (int e = threadIdx.x; e < nb2 * 64; e += 256) {
      const int cl = e >> 6, i = (e >> 2) & 15, kk = e & 3; // four lanes read 32 consecutive bytes of a row of x
      double v = 0.0;
      if (cl < nb) {
        const int k = 4 * chunks[c0 + cl] + kk, r = row0 + i;
        if (k < n_k && r < n_rows && (!LIT || w[r] != 0.0)) v = x[(size_t)r * n_k + k];
      }
      s_u[cl * 64 + kk * 16 + i] = v;
    }
    __syncthreads();
    double bn[2][4];
    auto fetch = [&](int cl) { // the B operands of the pair of chunks at cl, requested together
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int k = cl + h < nb ? 4 * chunks[c0 + cl + h] + ln.kq : 0;
        const SolarQuad q = solar_load_quad(tab_abs + (size_t)(k < n_k ? k : 0) * n_pts, ln);
#pragma unroll
        for (int t = 0; t < 4; ++t) bn[h][t] = q[t];
      }
    };
    fetch(0);
    for (int cl = 0; cl < nb2; cl += 2) {
      double b[2][4];
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int t = 0; t < 4; ++t) b[h][t] = bn[h][t];
      const double a0 = s_u[cl * 64 + ln.lane], a1 = s_u[(cl + 1) * 64 + ln.lane];
      if (cl + 2 < nb2) fetch(cl + 2); // the next pair in flight under this pair's products
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b[0][t], acc[t], 0, 0, 0);
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b[1][t], acc[t], 0, 0, 0);
    }
  }
}
