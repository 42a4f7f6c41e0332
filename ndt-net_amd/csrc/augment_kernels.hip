// augment_kernels.hip -- train-time augmentation on gfx950 (include/ndnet_augment.h).
//
//   k_aug_params  one workgroup: reads the step, leaves step + 1, and writes the
//                 step's snapshot and every cloud's matrix, translation and drop
//                 threshold into the work buffer (cos / sin once per cloud, in
//                 double).
//   k_aug_count   drop_max > 0 only: the kept points of every tile of
//                 NDNET_AUG_TILE points.  Reads no point data: Philox and the
//                 cloud's threshold.
//   k_aug_apply   one workgroup per tile: the points arrive as the flat coalesced
//                 float stream (as k_point_rows reads them) into LDS, thread t
//                 owns the points t, t + 256, ... of the tile (LDS stride 3:
//                 conflict-free), transforms them, ranks the kept ones in input
//                 order (a ballot per slab of 256, the 16 wave counts through
//                 LDS), writes them to LDS at their rank and the workgroup
//                 stores the compacted tile as one flat coalesced stream at the
//                 cloud's offset -- the sum of the preceding tiles' counts,
//                 which the workgroup adds up itself.  Without dropout the rank
//                 is the index and the offset the tile's start.
//
// Three dependent launches; no workgroup waits on another.  Built with
// -ffp-contract=off: the header defines the result operation by operation.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/ndnet_amd.h"
#include "../../include/ndnet_augment.h"

namespace {

#define AUG_HIPCHK(x)                                                         \
  do {                                                                        \
    hipError_t e_ = (x);                                                      \
    if (e_ != hipSuccess) {                                                   \
      fprintf(stderr, "ndnet_amd: %s: %s\n", #x, hipGetErrorString(e_));      \
      return NDNET_ERR_HIP;                                                   \
    }                                                                         \
  } while (0)

constexpr int kT = 256;                       // threads of every workgroup here
constexpr int kWaves = kT / 64;
constexpr int kPPT = NDNET_AUG_TILE / kT;     // a thread's points per tile
constexpr int kSlabs = kPPT * kWaves;         // (slab of 256 points, wave) pairs of a tile, in input order
static_assert(NDNET_AUG_TILE % kT == 0 && kPPT >= 1, "");

constexpr uint32_t kPurposeCloud = 0, kPurposeJitter = 1, kPurposeKeep = 2;

// the work buffer: AugHead | xform [B][12] float | T [B] uint32 | tile counts [B][tiles] uint32
struct AugHead {
  uint64_t step;  // the call's step, snapshotted by k_aug_params
  uint64_t pad;
};
constexpr size_t kXformBytes = 12 * sizeof(float);

__host__ __device__ inline uint32_t aug_tiles(uint32_t n) { return (n + NDNET_AUG_TILE - 1) / NDNET_AUG_TILE; }
__host__ __device__ inline float* work_xform(void* w) { return (float*)((char*)w + sizeof(AugHead)); }
__host__ __device__ inline uint32_t* work_thr(void* w, int B) {
  return (uint32_t*)((char*)w + sizeof(AugHead) + kXformBytes * (size_t)B);
}
__host__ __device__ inline uint32_t* work_tiles(void* w, int B) { return work_thr(w, B) + B; }

struct U4 {
  uint32_t w[4];
};

__device__ __forceinline__ U4 philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
  constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;
#pragma unroll
  for (int r = 0; r < 10; r++) {
    const uint64_t p0 = (uint64_t)M0 * c0, p1 = (uint64_t)M1 * c2;  // (one 32 x 32 -> 64 multiply each)
    const uint32_t h0 = (uint32_t)(p0 >> 32), l0 = (uint32_t)p0, h1 = (uint32_t)(p1 >> 32), l1 = (uint32_t)p1;
    const uint32_t n0 = h1 ^ c1 ^ k0, n2 = h0 ^ c3 ^ k1;
    c0 = n0;
    c1 = l1;
    c2 = n2;
    c3 = l0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return U4{{c0, c1, c2, c3}};
}

__device__ __forceinline__ double u24(uint32_t w) { return (double)(w >> 8) * 0x1p-24; }

__device__ __forceinline__ uint32_t cloud_len(const int32_t* counts, int b, uint32_t n) {
  if (!counts) return n;
  const int32_t c = counts[b];
  return c < 1 ? 1u : (uint32_t)c > n ? n : (uint32_t)c;
}

__global__ void __launch_bounds__(kT) k_aug_params(ndnet_aug_config cfg, int B, uint64_t* __restrict__ d_step,
                                                   void* __restrict__ work, float* __restrict__ d_xform) {
  const uint64_t step = *d_step;  // every thread reads it before thread 0 replaces it
  __syncthreads();
  if (threadIdx.x == 0) {
    ((AugHead*)work)->step = step;
    *d_step = step + 1;
  }
  const uint32_t c2 = (uint32_t)step, c3 = ((uint32_t)(step >> 32) << 2) | kPurposeCloud;
  float* wx = work_xform(work);
  uint32_t* wt = work_thr(work, B);
  for (int b = threadIdx.x; b < B; b += kT) {
    const U4 P = philox(0u, (uint32_t)b, c2, c3, cfg.seed, cfg.stream);
    const U4 Q = philox(1u, (uint32_t)b, c2, c3, cfg.seed, cfg.stream);
    const double theta = (2.0 * u24(P.w[0]) - 1.0) * cfg.yaw_max;
    const double s = cfg.scale_lo + u24(P.w[1]) * (cfg.scale_hi - cfg.scale_lo);
    const double fx = (P.w[2] & 0xffffu) < cfg.flip_x_16 ? -1.0 : 1.0;
    const double fy = (P.w[2] >> 16) < cfg.flip_y_16 ? -1.0 : 1.0;
    const uint32_t T = (uint32_t)floor(u24(P.w[3]) * cfg.drop_max * 0x1p32);
    const double c = cos(theta), z = sin(theta);
    const double sc = s * c, sz = s * z;
    float m[12];
    m[0] = (float)(fx * sc);
    m[1] = (float)(fx * -sz);
    m[2] = 0.0f;
    m[3] = (float)((2.0 * u24(Q.w[0]) - 1.0) * cfg.shift_max[0]);
    m[4] = (float)(fy * sz);
    m[5] = (float)(fy * sc);
    m[6] = 0.0f;
    m[7] = (float)((2.0 * u24(Q.w[1]) - 1.0) * cfg.shift_max[1]);
    m[8] = 0.0f;
    m[9] = 0.0f;
    m[10] = (float)s;
    m[11] = (float)((2.0 * u24(Q.w[2]) - 1.0) * cfg.shift_max[2]);
#pragma unroll
    for (int j = 0; j < 12; j++) {
      wx[12 * b + j] = m[j];
      if (d_xform) d_xform[12 * b + j] = m[j];
    }
    wt[b] = T;
  }
}

// keep of point i: point 0 always, else word 6 (the third of the purpose-2 draw) against the threshold
__device__ __forceinline__ bool aug_keep(uint32_t i, uint32_t b, uint32_t c2, uint32_t c3hi, uint32_t k0, uint32_t k1,
                                         uint32_t T) {
  const U4 W = philox(i, b, c2, c3hi | kPurposeKeep, k0, k1);
  return i == 0 || W.w[2] >= T;
}

// the 16 (slab, wave) counts of a tile through LDS: every thread leaves with the kept points before
// its own in input order and the tile's total.  s_cnt must not be in use (one barrier inside).
__device__ __forceinline__ void tile_ranks(const bool (&keep)[kPPT], uint32_t* s_cnt, uint32_t (&rank)[kPPT],
                                           uint32_t& total) {
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t below[kPPT];
#pragma unroll
  for (int q = 0; q < kPPT; q++) {
    const unsigned long long mask = __ballot(keep[q]);
    below[q] = (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
    if (lane == 0) s_cnt[q * kWaves + wave] = (uint32_t)__popcll(mask);
  }
  __syncthreads();
  uint32_t run = 0;
#pragma unroll
  for (int q = 0; q < kPPT; q++) {
#pragma unroll
    for (int w = 0; w < kWaves; w++) {
      if ((uint32_t)w == wave) rank[q] = run + below[q];
      run += s_cnt[q * kWaves + w];
    }
  }
  total = run;
}

__global__ void __launch_bounds__(kT) k_aug_count(uint32_t k0, uint32_t k1, const int32_t* __restrict__ counts,
                                                  uint32_t n, int B, void* __restrict__ work) {
  __shared__ uint32_t s_cnt[kWaves];
  const uint32_t b = blockIdx.y, tile = blockIdx.x, t = threadIdx.x;
  const uint32_t tiles = aug_tiles(n);
  uint32_t* out = work_tiles(work, B) + (uint64_t)b * tiles + tile;
  const uint32_t m = cloud_len(counts, (int)b, n);
  const uint32_t start = tile * NDNET_AUG_TILE;
  if (start >= m) {  // a tile of padding
    if (t == 0) *out = 0;
    return;
  }
  const uint64_t step = ((const AugHead*)work)->step;
  const uint32_t c2 = (uint32_t)step, c3hi = (uint32_t)(step >> 32) << 2;
  const uint32_t T = work_thr(work, B)[b];
  uint32_t kept = 0;
#pragma unroll
  for (int q = 0; q < kPPT; q++) {
    const uint32_t i = start + t + kT * q;  // (< 2^31 + 1024)
    kept += i < m && aug_keep(i, b, c2, c3hi, k0, k1, T) ? 1u : 0u;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) kept += __shfl_xor(kept, d, 64);
  if ((t & 63) == 0) s_cnt[t >> 6] = kept;
  __syncthreads();
  if (t == 0) {
    uint32_t sum = 0;
#pragma unroll
    for (int w = 0; w < kWaves; w++) sum += s_cnt[w];
    *out = sum;
  }
}

template <bool kDrop, bool kLabels>
// (pts / out_pts and labels / out_labels may be the same arrays without dropout: no __restrict__)
__global__ void __launch_bounds__(kT) k_aug_apply(uint32_t k0, uint32_t k1, float sigma, const float* pts,
                                                  const int32_t* labels, const int32_t* __restrict__ counts,
                                                  uint32_t n, int B, const void* work_c, float* out_pts,
                                                  int32_t* out_labels, int32_t* out_counts) {
  __shared__ float sp[3 * NDNET_AUG_TILE];
  __shared__ int32_t s_lab[kLabels ? NDNET_AUG_TILE : 1];
  __shared__ uint32_t s_cnt[kSlabs];
  __shared__ uint32_t s_base[kWaves];
  void* work = const_cast<void*>(work_c);
  const uint32_t b = blockIdx.y, tile = blockIdx.x, t = threadIdx.x;
  const uint32_t m = cloud_len(counts, (int)b, n);
  const uint32_t start = tile * NDNET_AUG_TILE;
  if (start >= m) return;  // a tile of padding: nothing read, nothing written
  const uint32_t cnt = m - start < (uint32_t)NDNET_AUG_TILE ? m - start : (uint32_t)NDNET_AUG_TILE;
  const bool last = start + cnt == m;
  const uint64_t row0 = (uint64_t)b * n;  // the cloud's first row

  // the tile's points as a flat float stream, every load issued before the first use
  {
    const float* p = pts + (row0 + start) * 3;
    float v[3 * kPPT];
#pragma unroll
    for (int j = 0; j < 3 * kPPT; j++) {
      const uint32_t f = t + kT * j;
      v[j] = f < 3 * cnt ? p[f] : 0.0f;
    }
#pragma unroll
    for (int j = 0; j < 3 * kPPT; j++) sp[t + kT * j] = v[j];
  }
  int32_t lab[kPPT];
  if (kLabels) {
#pragma unroll
    for (int q = 0; q < kPPT; q++) {
      const uint32_t il = t + kT * q;
      lab[q] = il < cnt ? labels[row0 + start + il] : 0;
    }
  }
  // the cloud's rows before this tile: the kept points of the preceding tiles
  uint32_t base = start;
  if (kDrop) {
    const uint32_t* tc = work_tiles(work, B) + (uint64_t)b * aug_tiles(n);
    uint32_t sum = 0;
    for (uint32_t j = t; j < tile; j += kT) sum += tc[j];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, 64);
    if ((t & 63) == 0) s_base[t >> 6] = sum;
  }
  __syncthreads();
  if (kDrop) {
    base = 0;
#pragma unroll
    for (int w = 0; w < kWaves; w++) base += s_base[w];
  }

  const uint64_t step = ((const AugHead*)work)->step;
  const uint32_t c2 = (uint32_t)step, c3hi = (uint32_t)(step >> 32) << 2;
  const float* M = work_xform(work) + 12 * b;
  const float m00 = M[0], m01 = M[1], m02 = M[2], tx = M[3], m10 = M[4], m11 = M[5], m12 = M[6], ty = M[7],
              m20 = M[8], m21 = M[9], m22 = M[10], tz = M[11];
  const uint32_t T = kDrop ? work_thr(work, B)[b] : 0u;
  const float K = (float)(1.7320508075688772 / 65536.0);  // float32(sqrt(3.0) / 65536.0)

  float ox[kPPT], oy[kPPT], oz[kPPT];
  bool keep[kPPT];
#pragma unroll
  for (int q = 0; q < kPPT; q++) {
    const uint32_t il = t + kT * q, i = start + il;
    const float x = sp[3 * il], y = sp[3 * il + 1], z = sp[3 * il + 2];
    const U4 W = philox(i, b, c2, c3hi | kPurposeJitter, k0, k1);  // words 0 .. 3
    const U4 V = philox(i, b, c2, c3hi | kPurposeKeep, k0, k1);    // words 4 .. 7
    const int32_t sx = (int32_t)((W.w[0] & 0xffffu) + (W.w[0] >> 16) + (W.w[1] & 0xffffu) + (W.w[1] >> 16));
    const int32_t sy = (int32_t)((W.w[2] & 0xffffu) + (W.w[2] >> 16) + (W.w[3] & 0xffffu) + (W.w[3] >> 16));
    const int32_t sz = (int32_t)((V.w[0] & 0xffffu) + (V.w[0] >> 16) + (V.w[1] & 0xffffu) + (V.w[1] >> 16));
    keep[q] = il < cnt && (!kDrop || i == 0 || V.w[2] >= T);
    const float jx = sigma * ((float)(sx - 131070) * K);
    const float jy = sigma * ((float)(sy - 131070) * K);
    const float jz = sigma * ((float)(sz - 131070) * K);
    ox[q] = (((m00 * x + m01 * y) + m02 * z) + tx) + jx;
    oy[q] = (((m10 * x + m11 * y) + m12 * z) + ty) + jy;
    oz[q] = (((m20 * x + m21 * y) + m22 * z) + tz) + jz;
  }

  uint32_t rank[kPPT], total = cnt;
  if (kDrop) {
    tile_ranks(keep, s_cnt, rank, total);  // (its barrier: every thread has read its points)
  } else {
#pragma unroll
    for (int q = 0; q < kPPT; q++) rank[q] = t + kT * q;
    __syncthreads();
  }
#pragma unroll
  for (int q = 0; q < kPPT; q++) {
    if (keep[q]) {
      sp[3 * rank[q]] = ox[q];
      sp[3 * rank[q] + 1] = oy[q];
      sp[3 * rank[q] + 2] = oz[q];
      if (kLabels) s_lab[rank[q]] = lab[q];
    }
  }
  __syncthreads();
  // base + total <= m <= n: the stores stay inside the cloud's rows
  float* o = out_pts + (row0 + base) * 3;
  for (uint32_t f = t; f < 3 * total; f += kT) o[f] = sp[f];
  if (kLabels) {
    int32_t* ol = out_labels + row0 + base;
    for (uint32_t f = t; f < total; f += kT) ol[f] = s_lab[f];
  }
  if (last && t == 0) out_counts[b] = (int32_t)(base + total);
}

bool amplitude_ok(double v) { return v >= 0.0; }  // (false for NaN)

}  // namespace

extern "C" {

size_t ndnet_aug_work_bytes(int B, uint64_t n) {
  if (B < 1 || n < 1 || n >= (1ull << 31)) return 0;
  return sizeof(AugHead) + (kXformBytes + sizeof(uint32_t)) * (size_t)B +
         sizeof(uint32_t) * (size_t)B * aug_tiles((uint32_t)n);
}

int ndnet_aug_run(const ndnet_aug_config* cfg, const float* d_points, const int32_t* d_labels, const int32_t* d_counts,
                  int B, uint64_t n, uint64_t* d_step, void* d_work, float* d_out_points, int32_t* d_out_labels,
                  int32_t* d_out_counts, float* d_xform, void* stream) {
  if (!cfg || !d_points || !d_step || !d_work || !d_out_points || !d_out_counts) return NDNET_ERR_ARG;
  if ((d_labels != nullptr) != (d_out_labels != nullptr)) return NDNET_ERR_ARG;
  if (B < 1 || B > 65535 || n < 1 || n >= (1ull << 31)) return NDNET_ERR_ARG;
  if (!(cfg->scale_lo > 0.0) || !(cfg->scale_lo <= cfg->scale_hi)) return NDNET_ERR_ARG;
  if (!(cfg->drop_max >= 0.0 && cfg->drop_max <= 1.0)) return NDNET_ERR_ARG;
  if (!amplitude_ok(cfg->yaw_max) || !amplitude_ok(cfg->shift_max[0]) || !amplitude_ok(cfg->shift_max[1]) ||
      !amplitude_ok(cfg->shift_max[2]) || !amplitude_ok(cfg->jitter_sigma))
    return NDNET_ERR_ARG;
  if (cfg->flip_x_16 > 65536u || cfg->flip_y_16 > 65536u) return NDNET_ERR_ARG;
  const bool drop = cfg->drop_max > 0.0;
  if (drop && (d_out_points == d_points || (d_labels && d_out_labels == d_labels))) return NDNET_ERR_ARG;

  hipStream_t st = (hipStream_t)stream;
  const uint32_t n32 = (uint32_t)n;
  const dim3 grid(aug_tiles(n32), (uint32_t)B);
  const float sigma = (float)cfg->jitter_sigma;
  k_aug_params<<<1, kT, 0, st>>>(*cfg, B, d_step, d_work, d_xform);
  AUG_HIPCHK(hipGetLastError());
  if (drop) {
    k_aug_count<<<grid, kT, 0, st>>>(cfg->seed, cfg->stream, d_counts, n32, B, d_work);
    AUG_HIPCHK(hipGetLastError());
  }
#define AUG_APPLY(D, L)                                                                                          \
  k_aug_apply<D, L><<<grid, kT, 0, st>>>(cfg->seed, cfg->stream, sigma, d_points, d_labels, d_counts, n32, B, \
                                         d_work, d_out_points, d_out_labels, d_out_counts)
  if (drop) {
    if (d_labels) AUG_APPLY(true, true); else AUG_APPLY(true, false);
  } else {
    if (d_labels) AUG_APPLY(false, true); else AUG_APPLY(false, false);
  }
#undef AUG_APPLY
  AUG_HIPCHK(hipGetLastError());
  return NDNET_OK;
}

}  // extern "C"
