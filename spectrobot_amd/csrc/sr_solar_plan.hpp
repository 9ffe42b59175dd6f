// sr_solar_plan.hpp -- the host plan of sr_solar_source_kernel (sr_solar_source.inc) as a plain function: per tile of
// kSolarRows rows the chunks of kSolarChunk consecutive k in which any LIT row of the tile (w != 0) has a non-zero
// column, in ascending order.  Included by sr_api.hip and by the host build tools/solar_source_host; no HIP header.
// U is read as it is: nothing is sorted, nothing is changed.  full: every chunk of every tile is listed (the check
// that the result does not depend on the lists: a chunk that is not listed would only have added exact zeros).
// The plan of sr_solar_jac_kernel (sr_solar_jac.inc; tools/solar_jacobian_host) is the same walk per parameter.
#pragma once
#include <cstddef>
#include <vector>

namespace sr {

constexpr int kSolarRows = 16; // rows of a tile: the MFMA's M
constexpr int kSolarChunk = 4; // k per chunk: the MFMA's K
constexpr int kSolarJacRays = 8; // NR: rays per block of sr_solar_jac_kernel (profiles/solar_jac_kernel_resources.txt)
constexpr int kDiffuseGases = 8; // gas slots of the diffuse kernels' loop (sr_diffuse_source.inc): n_gas above is refused
constexpr int kDiffuseJacPars = 4; // NP: parameters per block of sr_diffuse_tangent_kernel and per thread of the contraction
constexpr int kDiffuseOpt = 3 * kDiffuseGases + 1; // doubles per parameter of an optics direction: the coefficients' tangents, the albedo's
constexpr int kDiffuseJacRays = 8; // NR: rays per thread of sr_diffuse_contract_kernel (profiles/diffuse_jacobian_kernel_resources.txt)
constexpr int kDiffuseColumns = 8; // columns of sr_diffuse_columns_kernel's largest instance (SR_MAX_DIFFUSE_COLUMNS): n_col above is refused
constexpr int kZeroRow = 1 << 30;  // row_ix flag of sr_diffuse_columns_kernel: the row is an exact 0 (row numbers stay below 2^17)

// The one walk behind both plans: x [n_groups][n_rows][n_k], per (group, row tile) the chunks in which a row of the tile
// that counts (w == nullptr: every row; else the rows with w[r] != 0) has a non-zero element, ascending; tile_off
// [n_groups n_tiles + 1] into chunks, the tiles of group p at p n_tiles ..: a tile never straddles a group.  n_tiles =
// ceil(n_rows / kSolarRows), chunk c covers k = 4 c .. 4 c + 3 (< n_k).  Returns false if an element of x is not finite
// or, with NONNEG, negative (the entry's check, in the same walk: x is the one large array of a call and is read once);
// the lists are then unspecified.  A whole chunk is checked and marked without a branch per element.
template <bool NONNEG>
inline bool solar_walk_chunk_lists(const double *x, const double *w, int n_groups, int n_rows, int n_k, bool full,
                                   std::vector<int> &tile_off, std::vector<int> &chunks) {
  const int n_tiles = (n_rows + kSolarRows - 1) / kSolarRows, n_chunks = (n_k + kSolarChunk - 1) / kSolarChunk;
  const int n_whole = n_k / kSolarChunk; // chunks with all four k
  constexpr double kMax = 1.7976931348623157e308, kMin = NONNEG ? 0.0 : -kMax;
  tile_off.assign(1, 0);
  chunks.clear();
  std::vector<char> hit((size_t)n_chunks);
  bool ok = true;
  for (int p = 0; p < n_groups; ++p)
    for (int t = 0; t < n_tiles; ++t) {
      hit.assign((size_t)n_chunks, full ? 1 : 0);
      const int r1 = n_rows < (t + 1) * kSolarRows ? n_rows : (t + 1) * kSolarRows;
      for (int r = t * kSolarRows; r < r1; ++r) {
        const char lit = !w || w[r] != 0.0; // in shadow: the row's optical depth is not evaluated, its columns list nothing
        const double *xr = x + ((size_t)p * n_rows + r) * n_k;
        for (int c = 0; c < n_whole; ++c) {
          const double *v = xr + kSolarChunk * c;
          // (a NaN fails v >= min, an infinity one of the two)
          ok &= (v[0] >= kMin) & (v[1] >= kMin) & (v[2] >= kMin) & (v[3] >= kMin) & (v[0] <= kMax) & (v[1] <= kMax) &
                (v[2] <= kMax) & (v[3] <= kMax);
          hit[(size_t)c] |= lit & (char)((v[0] != 0.0) | (v[1] != 0.0) | (v[2] != 0.0) | (v[3] != 0.0));
        }
        for (int k = kSolarChunk * n_whole; k < n_k; ++k) {
          ok &= (xr[k] >= kMin) & (xr[k] <= kMax);
          hit[(size_t)n_whole] |= lit & (char)(xr[k] != 0.0);
        }
      }
      for (int c = 0; c < n_chunks; ++c)
        if (hit[(size_t)c]) chunks.push_back(c);
      tile_off.push_back((int)chunks.size());
    }
  return ok;
}

// The plan of sr_solar_source_kernel: u [n_rows][n_k] >= 0, the lit rows of w.  Returns false if an element of u is
// negative or not finite.
inline bool solar_chunk_lists(const double *u, const double *w, int n_rows, int n_k, bool full, std::vector<int> &tile_off,
                              std::vector<int> &chunks) {
  return solar_walk_chunk_lists<true>(u, w, 1, n_rows, n_k, full, tile_off, chunks);
}

// The plan of sr_solar_jac_kernel (sr_solar_jac.inc): the same lists per (parameter, row tile) of du [n_par][n_rows][n_k],
// the derivative of the columns to a parameter -- any finite sign, no weights.  Returns false if an element is not finite.
inline bool solar_jac_chunk_lists(const double *du, int n_par, int n_rows, int n_k, bool full, std::vector<int> &tile_off,
                                  std::vector<int> &chunks) {
  return solar_walk_chunk_lists<false>(du, nullptr, n_par, n_rows, n_k, full, tile_off, chunks);
}

// The plan of sr_diffuse_tangent_kernel (sr_diffuse_jac.inc; tools/diffuse_jacobian_host): per parameter the layer range
// mask[2 p] .. mask[2 p + 1] - 1 that holds every layer with a non-zero dv[p][.][l] (lo = hi = 0: none) of
// dv [n_par][n_gas][n_layers]; outside it the layer operators have no tangent.  A layer without any column (every
// v[g][l] == 0) has dtau == 0 at every point and no tangent whatever dv says: it widens no range.  Returns false if an
// element of dv is not finite.
inline bool diffuse_jac_masks(const double *v, const double *dv, int n_par, int n_gas, int n_layers, std::vector<int> &mask) {
  mask.assign((size_t)2 * n_par, 0);
  bool ok = true;
  std::vector<char> filled((size_t)n_layers, 0);
  for (int g = 0; g < n_gas; ++g)
    for (int l = 0; l < n_layers; ++l) filled[(size_t)l] |= (char)(v[(size_t)g * n_layers + l] != 0.0);
  for (int p = 0; p < n_par; ++p) {
    int lo = n_layers, hi = 0;
    for (int g = 0; g < n_gas; ++g) {
      const double *row = dv + ((size_t)p * n_gas + g) * n_layers;
      for (int l = 0; l < n_layers; ++l) {
        ok &= (row[l] >= -1.7976931348623157e308) & (row[l] <= 1.7976931348623157e308); // (a NaN fails both)
        if (row[l] != 0.0 && filled[(size_t)l]) {
          lo = l < lo ? l : lo;
          hi = l + 1 > hi ? l + 1 : hi;
        }
      }
    }
    if (hi > lo) mask[(size_t)2 * p] = lo, mask[(size_t)2 * p + 1] = hi;
  }
  return ok;
}

// The plan of sr_diffuse_tangent_kernel's optics instance (sr_diffuse_jac.inc; tools/diffuse_optics_host): per parameter
// dopt [n_par][kDiffuseOpt] -- the tangents of the per-gas coefficients as built, [3][kDiffuseGases] (zeros beyond n_gas),
// along dssa and dasym [n_par][n_gas], with f = max(asym, 0)^2, df = 2 max(asym, 0) dasym:
//   d(ssa (1 - f)) = dssa (1 - f) - ssa df,  d(1 - ssa) = -dssa,  d(ssa (asym - f)) = dssa (asym - f) + ssa (dasym - df)
// and then dalb[p] -- and the layer range mask[2 p] .. mask[2 p + 1] - 1 that holds every layer in which a gas with a
// non-zero coefficient tangent has a column (lo = hi = 0: none -- a direction in the albedo alone).  dssa, dasym and dalb
// may each be null: zeros.  Returns false if an element of them, or a tangent made of them, is not finite.
inline bool diffuse_optics_plan(const double *v, const double *ssa, const double *asym, const double *dssa, const double *dasym,
                                const double *dalb, int n_par, int n_gas, int n_layers, std::vector<double> &dopt,
                                std::vector<int> &mask) {
  dopt.assign((size_t)n_par * kDiffuseOpt, 0.0);
  mask.assign((size_t)2 * n_par, 0);
  bool ok = true;
  for (int p = 0; p < n_par; ++p) {
    double *dc = dopt.data() + (size_t)p * kDiffuseOpt;
    int lo = n_layers, hi = 0;
    const double db = dalb ? dalb[p] : 0.0;
    ok &= (db >= -1.7976931348623157e308) & (db <= 1.7976931348623157e308);
    dc[3 * kDiffuseGases] = db;
    for (int g = 0; g < n_gas; ++g) {
      const double ds = dssa ? dssa[(size_t)p * n_gas + g] : 0.0, da = dasym ? dasym[(size_t)p * n_gas + g] : 0.0;
      ok &= (ds >= -1.7976931348623157e308) & (ds <= 1.7976931348623157e308) & (da >= -1.7976931348623157e308) &
            (da <= 1.7976931348623157e308); // (a NaN fails both)
      const double as = asym[g], f = as > 0.0 ? as * as : 0.0, df = as > 0.0 ? 2.0 * as * da : 0.0;
      dc[g] = ds * (1.0 - f) - ssa[g] * df;
      dc[kDiffuseGases + g] = -ds;
      dc[2 * kDiffuseGases + g] = ds * (as - f) + ssa[g] * (da - df);
      for (int c = 0; c < 3; ++c) // (a direction so large that a coefficient's tangent overflows is refused too)
        ok &= (dc[c * kDiffuseGases + g] >= -1.7976931348623157e308) & (dc[c * kDiffuseGases + g] <= 1.7976931348623157e308);
      if (dc[g] == 0.0 && dc[kDiffuseGases + g] == 0.0 && dc[2 * kDiffuseGases + g] == 0.0) continue;
      for (int l = 0; l < n_layers; ++l)
        if (v[(size_t)g * n_layers + l] != 0.0) {
          lo = l < lo ? l : lo;
          hi = l + 1 > hi ? l + 1 : hi;
        }
    }
    if (hi > lo) mask[(size_t)2 * p] = lo, mask[(size_t)2 * p + 1] = hi;
  }
  return ok;
}

// The plan of sr_diffuse_columns_kernel (sr_diffuse_columns.inc; tools/diffuse_columns_host).  nc: the instance a call of
// n_col columns runs, the next of 1, 2, 4, 8.  mu0p [nc] and wp [n_rows][nc]: mu0 and col_w padded with zeros.  row_ix: the
// rows in the order of the kernel's downward walk -- layer n_layers - 1 first, a layer's rows ascending --, layer l's at
// row_off[n_layers - 1 - l] .. row_off[n_layers - l]; a row that is an exact 0 (`dark`: the gas scatters nothing; or
// every weight is 0) carries kZeroRow, or, accumulating, is not listed at all: its row of the output keeps its bits.
// Returns false for a mu0 outside [-1, 1], a weight that is negative or not finite, or a row_layer or src_row outside
// its range; the arrays are then unspecified.
inline int diffuse_columns_instance(int n_col) { return n_col <= 1 ? 1 : n_col <= 2 ? 2 : n_col <= 4 ? 4 : kDiffuseColumns; }
inline bool diffuse_columns_plan(const double *mu0, const double *col_w, const int *row_layer, const int *src_row, int n_col,
                                 int n_rows, int n_layers, int n_src, bool dark, bool accumulate, std::vector<double> &mu0p,
                                 std::vector<double> &wp, std::vector<int> &row_off, std::vector<int> &row_ix) {
  const int nc = diffuse_columns_instance(n_col);
  mu0p.assign((size_t)nc, 0.0);
  wp.assign((size_t)n_rows * nc, 0.0);
  row_off.assign((size_t)n_layers + 1, 0);
  row_ix.clear();
  bool ok = true;
  for (int c = 0; c < n_col; ++c) {
    ok &= (mu0[c] >= -1.0) & (mu0[c] <= 1.0); // (a NaN fails both)
    mu0p[(size_t)c] = mu0[c];
  }
  std::vector<char> zero((size_t)n_rows, 1);
  std::vector<int> count((size_t)n_layers, 0);
  for (int r = 0; r < n_rows; ++r) {
    for (int c = 0; c < n_col; ++c) {
      const double w = col_w[(size_t)r * n_col + c];
      ok &= (w >= 0.0) & (w <= 1.7976931348623157e308);
      wp[(size_t)r * nc + c] = w;
      if (w != 0.0 && !dark) zero[(size_t)r] = 0;
    }
    if (row_layer[r] < 0 || row_layer[r] >= n_layers || src_row[r] < 0 || src_row[r] >= n_src) return false;
    if (!(zero[(size_t)r] && accumulate)) ++count[(size_t)row_layer[r]];
  }
  if (!ok) return false;
  for (int l = n_layers - 1; l >= 0; --l) row_off[(size_t)(n_layers - l)] = row_off[(size_t)(n_layers - 1 - l)] + count[(size_t)l];
  row_ix.resize((size_t)row_off[(size_t)n_layers]);
  std::vector<int> at(row_off.begin(), row_off.end() - 1);
  for (int r = 0; r < n_rows; ++r)
    if (!(zero[(size_t)r] && accumulate)) row_ix[(size_t)at[(size_t)(n_layers - 1 - row_layer[r])]++] = r | (zero[(size_t)r] ? kZeroRow : 0);
  return true;
}

} // namespace sr
