// sr_limb_forward.inc -- the path-order radiance kernels of a ray batch, sr_limb_kernel and sr_limb_split_kernel.
// Included inside namespace sr by sr_limb.hip (NG = 1..4), by sr_limb_many.hip (NG = 5..8) and by the host builds under
// tools/ (tools/host_sim/hip_on_host.hpp) behind sr_limb_common.hpp.
template <int NG>
__global__ __launch_bounds__(256) void sr_limb_kernel(const double *__restrict__ abs_c, const double *__restrict__ emi_c,
                                                      int n_pts, int n_layers, const int *__restrict__ seg_off,
                                                      const int *__restrict__ seg_layer, const double *__restrict__ col,
                                                      LimbOpts o, int n_rays, double *__restrict__ rad) {
  int pb, ray;
  if (!limb_block((n_pts + 255) / 256, n_rays, pb, ray)) return;
  const int j = pb * 256 + threadIdx.x;
  if (j >= n_pts) return;
  double I = limb_initial(o, rad, (size_t)ray * n_pts + j, j);
  const int s0 = seg_off[ray], s1 = seg_off[ray + 1];
  // NG = 5..8 keep kB = 2: 4 NG vector loads of 8 bytes (20 .. 32) in flight per thread, which is what kB = 8 gives one
  // gas and kB = 4 two; kB = 1 would leave one segment's loads (2 NG) exposed per step of the dependent chain, and a
  // larger kB only costs registers (4 kB NG VGPRs of coefficients).
  constexpr int kB = NG == 1 ? 8 : (NG == 2 ? 4 : 2); // segments whose loads are issued together (see sr_radiance_kernel)
  const size_t gstride = (size_t)n_layers * n_pts;
  for (int sb = s0; sb < s1; sb += kB) {
    double a[kB][NG], e[kB][NG], u[kB][NG];
#pragma unroll
    for (int t = 0; t < kB; ++t) {
      const int s = min(sb + t, s1 - 1);
      const size_t ofs = (size_t)seg_layer[s] * n_pts + j;
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        a[t][g] = abs_c[g * gstride + ofs];
        e[t][g] = emi_c[g * gstride + ofs];
        u[t][g] = col[(size_t)g * o.n_seg_total + s];
      }
    }
#pragma unroll
    for (int t = 0; t < kB; ++t) {
      if (sb + t < s1) {
        double tau = a[t][0] * u[t][0], E = e[t][0] * u[t][0];
#pragma unroll
        for (int g = 1; g < NG; ++g) {
          tau = tau + a[t][g] * u[t][g];
          E = E + e[t][g] * u[t][g];
        }
        const Atten A = attenuation(tau);
        I = I * A.t + (o.solo_absorption ? 0.0 : E * A.f);
      }
    }
  }
  rad[(size_t)ray * n_pts + j] = I;
}

// The same recursion for SMALL launches (one ray on a 1/8 spectral shard: 49 blocks on 256 CUs), where the run time
// is the latency of one thread's chain of 160 dependent segments: the segments of a ray are cut into kLimbParts
// consecutive stretches, one wave per stretch and 64 points; a stretch is the affine map I -> I T + S (T = product of
// its transmissions, S its own emission attenuated by what follows inside the stretch), and maps compose in order.
constexpr int kLimbParts = 4;
template <int NG>
__global__ __launch_bounds__(64 * kLimbParts) void sr_limb_split_kernel(
    const double *__restrict__ abs_c, const double *__restrict__ emi_c, int n_pts, int n_layers,
    const int *__restrict__ seg_off, const int *__restrict__ seg_layer, const double *__restrict__ col, LimbOpts o,
    int n_rays, double *__restrict__ rad) {
  __shared__ double s_T[kLimbParts][64], s_S[kLimbParts][64];
  const int lane = threadIdx.x & 63, part = threadIdx.x >> 6;
  int pb, ray;
  if (!limb_block((n_pts + 63) / 64, n_rays, pb, ray)) return; // block-uniform: no thread reaches the barrier
  const int j = pb * 64 + lane;
  const int jj = min(j, n_pts - 1);
  const int r0 = seg_off[ray], r1 = seg_off[ray + 1], n = r1 - r0;
  const int s0 = r0 + (int)(((long)n * part) / kLimbParts), s1 = r0 + (int)(((long)n * (part + 1)) / kLimbParts);
  constexpr int kB = NG == 1 ? 8 : (NG == 2 ? 4 : 2);
  const size_t gstride = (size_t)n_layers * n_pts;
  double T = 1.0, S = 0.0;
  for (int sb = s0; sb < s1; sb += kB) {
    double a[kB][NG], e[kB][NG], u[kB][NG];
#pragma unroll
    for (int t = 0; t < kB; ++t) {
      const int s = min(sb + t, s1 - 1);
      const size_t ofs = (size_t)seg_layer[s] * n_pts + jj;
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        a[t][g] = abs_c[g * gstride + ofs];
        e[t][g] = emi_c[g * gstride + ofs];
        u[t][g] = col[(size_t)g * o.n_seg_total + s];
      }
    }
#pragma unroll
    for (int t = 0; t < kB; ++t) {
      if (sb + t < s1) {
        double tau = a[t][0] * u[t][0], E = e[t][0] * u[t][0];
#pragma unroll
        for (int g = 1; g < NG; ++g) {
          tau = tau + a[t][g] * u[t][g];
          E = E + e[t][g] * u[t][g];
        }
        const Atten A = attenuation(tau);
        T = T * A.t;
        S = S * A.t + (o.solo_absorption ? 0.0 : E * A.f);
      }
    }
  }
  s_T[part][lane] = T;
  s_S[part][lane] = S;
  __syncthreads();
  if (part == 0 && j < n_pts) {
    double I = limb_initial(o, rad, (size_t)ray * n_pts + j, j);
#pragma unroll
    for (int p = 0; p < kLimbParts; ++p) I = I * s_T[p][lane] + s_S[p][lane];
    rad[(size_t)ray * n_pts + j] = I;
  }
}
