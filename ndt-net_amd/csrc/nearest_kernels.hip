// nearest_kernels.hip -- the PointNet-on-FPS baseline's device steps on gfx950
// (include/ndnet_nearest.h).
//
//   k_nearest     one workgroup of 256 threads per tile of kTile points of one
//                 cloud; thread i owns the points tile0 + i, + 256, + 512, + 768
//                 (coordinates and the running (best, row) in registers).  The
//                 cloud's samples pass through LDS in chunks of kChunk, one
//                 float4 each; in the inner loop every lane reads the same
//                 sample (one ds_read_b128 broadcast for four points' work).
//                 Samples are visited in ascending t and taken only on a
//                 strictly smaller distance, so ties keep the smaller t and the
//                 result does not depend on the tiling.  A tile wholly past the
//                 cloud's count writes its -1s and leaves.
//   k_transform3  one thread per point: y = t1[b] p, then the reference's
//                 nan_to_num.
//
// Built with -ffp-contract=off: every operation of d = (dx*dx + dy*dy) + dz*dz
// and of the transform's sums is rounded on its own (the header's definitions).
#include <hip/hip_runtime.h>
#include <float.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/ndnet_amd.h"
#include "../../include/ndnet_nearest.h"

namespace {

#define NN_HIPCHK(x)                                                          \
  do {                                                                        \
    hipError_t e_ = (x);                                                      \
    if (e_ != hipSuccess) {                                                   \
      fprintf(stderr, "ndnet_amd: %s: %s\n", #x, hipGetErrorString(e_));      \
      return NDNET_ERR_HIP;                                                   \
    }                                                                         \
  } while (0)

constexpr int kT = 256;
constexpr int kTile = NDNET_NN_TILE_POINTS, kChunk = NDNET_NN_CHUNK_SAMPLES;
constexpr int kPer = kTile / kT;  // points per thread
static_assert(kTile % kT == 0 && kChunk % kT == 0, "");

__device__ __forceinline__ uint32_t clamp_count(const int32_t* counts, uint64_t b, uint32_t hi) {
  if (!counts) return hi;
  const int32_t c = counts[b];
  return c < 0 ? 0u : (uint32_t)c > hi ? hi : (uint32_t)c;
}

__global__ void __launch_bounds__(kT) k_nearest(const float* __restrict__ points, uint32_t n,
                                                const int32_t* __restrict__ counts,
                                                const float* __restrict__ samples, uint32_t S,
                                                const int32_t* __restrict__ sample_counts,
                                                int32_t* __restrict__ rows, float* __restrict__ dist) {
  __shared__ float4 s_s[kChunk];
  const uint32_t tid = threadIdx.x;
  const uint64_t b = blockIdx.y;
  const uint32_t tile0 = blockIdx.x * (uint32_t)kTile;  // < n < 2^31
  const uint32_t m = clamp_count(counts, b, n);
  int32_t* __restrict__ out = rows + b * n;

  if (tile0 >= m) {  // the whole tile is padding (uniform: no barrier is skipped by part of a workgroup)
#pragma unroll
    for (int k = 0; k < kPer; k++) {
      const uint32_t i = tile0 + tid + k * kT;
      if (i < n) out[i] = -1;
    }
    return;
  }
  const uint32_t ms = clamp_count(sample_counts, b, S);
  const float* __restrict__ p = points + b * n * 3;
  const float* __restrict__ s = samples + b * S * 3;

  float px[kPer], py[kPer], pz[kPer], best[kPer];
  int32_t row[kPer];
#pragma unroll
  for (int k = 0; k < kPer; k++) {
    const uint32_t i = tile0 + tid + k * kT;
    const bool has = i < m;  // (a point past the count is never read; its slot's work is discarded)
    px[k] = has ? p[(uint64_t)i * 3 + 0] : 0.0f;
    py[k] = has ? p[(uint64_t)i * 3 + 1] : 0.0f;
    pz[k] = has ? p[(uint64_t)i * 3 + 2] : 0.0f;
    best[k] = __builtin_inff();
    row[k] = -1;
  }

  for (uint32_t c0 = 0; c0 < ms; c0 += kChunk) {
    const uint32_t len = ms - c0 < (uint32_t)kChunk ? ms - c0 : (uint32_t)kChunk;
    __syncthreads();  // the chunk before this one has been read by every wave
    for (uint32_t j = tid; j < len; j += kT) {
      const uint64_t t = (uint64_t)(c0 + j) * 3;
      s_s[j] = make_float4(s[t + 0], s[t + 1], s[t + 2], 0.0f);
    }
    __syncthreads();
#pragma unroll 4
    for (uint32_t j = 0; j < len; j++) {
      const float4 v = s_s[j];
      const int32_t t = (int32_t)(c0 + j);
#pragma unroll
      for (int k = 0; k < kPer; k++) {
        const float dx = px[k] - v.x, dy = py[k] - v.y, dz = pz[k] - v.z;
        const float d = (dx * dx + dy * dy) + dz * dz;
        if (d < best[k]) {
          best[k] = d;
          row[k] = t;
        }
      }
    }
  }

#pragma unroll
  for (int k = 0; k < kPer; k++) {
    const uint32_t i = tile0 + tid + k * kT;
    if (i < m) {
      out[i] = row[k];
      if (dist) dist[b * n + i] = best[k];
    } else if (i < n) {
      out[i] = -1;
    }
  }
}

__global__ void __launch_bounds__(kT) k_transform3(const float* __restrict__ points, int64_t p_ld,
                                                   const float* __restrict__ t1, float* __restrict__ outp,
                                                   int64_t o_ld, uint32_t n) {
  const uint32_t i = blockIdx.x * (uint32_t)kT + threadIdx.x;
  const uint64_t b = blockIdx.y;
  if (i >= n) return;
  const float* __restrict__ t = t1 + b * 9;
  const float* __restrict__ p = points + (b * n + i) * p_ld;
  float* __restrict__ o = outp + (b * n + i) * o_ld;
  const float x = p[0], y = p[1], z = p[2];
#pragma unroll
  for (int a = 0; a < 3; a++) {
    float v = (t[3 * a + 0] * x + t[3 * a + 1] * y) + t[3 * a + 2] * z;
    if (v != v) v = 0.0f;
    else if (v > FLT_MAX) v = FLT_MAX;
    else if (v < -FLT_MAX) v = -FLT_MAX;
    o[a] = v;
  }
}

}  // namespace

extern "C" {

int ndnet_nearest_sample_run(const float* d_points, int B, uint64_t n, const int32_t* d_counts,
                             const float* d_samples, uint64_t S, const int32_t* d_sample_counts, int32_t* d_rows,
                             float* d_dist, void* stream) {
  if (!d_points || !d_samples || !d_rows || B < 1 || n < 1 || S < 1 || n >= (1ull << 31) || S >= (1ull << 31))
    return NDNET_ERR_ARG;
  if (B > 65535) return NDNET_ERR_ARG;  // (the grid's y extent)
  const dim3 grid((uint32_t)((n + kTile - 1) / kTile), (uint32_t)B);
  k_nearest<<<grid, kT, 0, (hipStream_t)stream>>>(d_points, (uint32_t)n, d_counts, d_samples, (uint32_t)S,
                                                  d_sample_counts, d_rows, d_dist);
  NN_HIPCHK(hipGetLastError());
  return NDNET_OK;
}

int ndnet_pn_transform3_run(const float* d_points, int64_t p_ld, const float* d_t1, float* d_out, int64_t o_ld, int B,
                            uint64_t n, void* stream) {
  if (!d_points || !d_t1 || !d_out || B < 1 || B > 65535 || n < 1 || n >= (1ull << 31) || p_ld < 3 || o_ld < 3)
    return NDNET_ERR_ARG;
  const dim3 grid((uint32_t)((n + kT - 1) / kT), (uint32_t)B);
  k_transform3<<<grid, kT, 0, (hipStream_t)stream>>>(d_points, p_ld, d_t1, d_out, o_ld, (uint32_t)n);
  NN_HIPCHK(hipGetLastError());
  return NDNET_OK;
}

}  // extern "C"
