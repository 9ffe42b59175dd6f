// sr_solar_source.inc -- sr_solar_source_kernel.  Included by sr_solar_source.hip inside namespace sr, and by the host
// build tools/solar_source_host.  Nothing else includes it.

// The single-scattering solar source of coefficient rows.  The build's own definition -- the reference has no counterpart:
//   tau[r][j] = sum_{k < n_k} U[r][k] A[k][j]                  (U >= 0: slant columns towards the sun, A: absorption rows)
//   T[r][j]   = exp(-tau[r][j])                                exactly 0 where w[r] == 0 or tau >= 700
//   emi[r][j] (+)= sca[src_row[r]][j] (w[r] sun[j] T[r][j])
// a matrix product [n_rows x n_k] . [n_k x n_pts] in fp64 with an exponential epilogue.
//
// The product is sr_solar_tile.inc's (solar_tile_product<LIT = true>: tile, operand and point layout, LDS staging, padding);
// in the epilogue a lane writes four consecutive points of a row, sixteen lanes 512 bytes.  Per row tile the host lists
// the chunks in which any lit row of the tile has a column (tile_off, chunks: block-uniform, scalar loads); a chunk not
// listed would have added exact zeros to every accumulator, so the result does not depend on the lists.  A row in shadow
// (w == 0) carries U = 0: its optical depth is not evaluated.  The blocks are dealt by limb_block(): the row tiles of a
// point block follow each other on one XCD, and the strip of A they share (n_k x 2 KB) is read from HBM once and by the
// other row tiles from that XCD's L2.  One writer per element, no atomics: the same call gives the same bits.
// (kSolarRows, kSolarChunk and the lists: sr_solar_plan.hpp)
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
  const SolarLane ln(pb, n_pts);
  const int row0 = tile * kSolarRows;
  v4d acc[4];
  solar_tile_product<true>(tab_abs, n_k, n_pts, u, w, n_rows, row0, chunks, tile_off[tile], tile_off[tile + 1], ln, s_u, acc);
  // epilogue: register r4 of a lane is row kq + 4 r4 of the tile, its four column tiles four consecutive points
#pragma unroll
  for (int r4 = 0; r4 < 4; ++r4) {
    const int r = row0 + ln.kq + 4 * r4;
    if (r >= n_rows) continue;
    const double wr = w[r];
    if (wr == 0.0 && ACC && !TRANS) continue; // in shadow: the row is left as it is
    const double *sca = sca_abs + (size_t)src_row[r] * n_pts;
    SolarQuad tr, e;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const double tau = acc[t][r4];
      tr[t] = (wr != 0.0 && tau < 700.0) ? exp_bounded(-tau) : 0.0;
      e[t] = wr != 0.0 ? sca[ln.pj[t]] * ((wr * sun[ln.pj[t]]) * tr[t]) : 0.0;
    }
    const size_t at0 = (size_t)r * n_pts + ln.p0;
    if (ln.whole) { // 32-byte stores: sixteen lanes write 512 consecutive bytes of the row
      if (TRANS) solar_quad(trans_out + at0, tr);
      if (wr == 0.0 && ACC) continue;
      if (ACC) {
        const SolarQuad base = solar_quad(emi_out + at0);
#pragma unroll
        for (int t = 0; t < 4; ++t) e[t] = base[t] + e[t];
      }
      solar_quad(emi_out + at0, e);
    } else {
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        if (ln.p0 + t >= n_pts) continue;
        if (TRANS) trans_out[at0 + t] = tr[t];
        if (wr == 0.0 && ACC) continue;
        if (ACC) emi_out[at0 + t] += e[t];
        else emi_out[at0 + t] = e[t];
      }
    }
  }
}
