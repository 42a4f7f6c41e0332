// segment_kernels.hip -- per-point segmentation labels on gfx950
// (include/ndnet_segment.h): the class of every ND row, gathered to the points
// through the rows ndnet_ndt_point_rows wrote, and the point-level confusion
// matrix.
//
//   k_seg_nd_argmax     a wave per ND row: lanes stride the row's columns
//                       (coalesced), the wave reduces to the first maximum
//   k_seg_point_labels  a thread per point: one coalesced int32 load and store,
//                       the ND labels (4 k bytes per cloud) from cache
//   k_seg_point_labels_u8  the same as bytes, four points per thread: a 16-byte
//                       row load and a 4-byte label store (scalar head and tail)
//   k_seg_confusion     grid-stride over the points; a per-workgroup LDS
//                       histogram flushed with 64-bit global atomics, or one
//                       64-bit global atomic per point for wide matrices
//   k_seg_row_hist      a thread per point: the class histogram of every ND row
//                       (the point-level training loss), one return-less
//                       32-bit global atomic per counted point
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/ndnet_amd.h"
#include "../../include/ndnet_segment.h"

namespace {

#define SEG_HIPCHK(x)                                                         \
  do {                                                                        \
    hipError_t e_ = (x);                                                      \
    if (e_ != hipSuccess) {                                                   \
      fprintf(stderr, "ndnet_amd: %s: %s\n", #x, hipGetErrorString(e_));      \
      return NDNET_ERR_HIP;                                                   \
    }                                                                         \
  } while (0)

constexpr int kSegThreads = 256;

// (v, i) beats (w, j) as the row's argmax: a NaN beats every number, a larger
// number a smaller one, the lower index an equal value (torch.argmax)
__device__ __forceinline__ bool seg_beats(float v, int i, float w, int j) {
  const bool vn = v != v, wn = w != w;
  if (vn || wn) return vn && (!wn || i < j);
  return v > w || (v == w && i < j);
}

__global__ void __launch_bounds__(kSegThreads) k_seg_nd_argmax(const float* __restrict__ scores, uint64_t rows,
                                                             int cols, int32_t* __restrict__ nd_labels) {
  const uint64_t r = (uint64_t)blockIdx.x * (kSegThreads / 64) + (threadIdx.x >> 6);
  if (r >= rows) return;  // (wave-uniform)
  const int lane = threadIdx.x & 63;
  const float* row = scores + r * (uint64_t)cols;
  float bv = -__builtin_inff();
  int bi = 0x7fffffff;  // a lane without a column loses to every column
  for (int j = lane; j < cols; j += 64) {
    const float v = row[j];
    if (seg_beats(v, j, bv, bi)) {
      bv = v;
      bi = j;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (seg_beats(ov, oi, bv, bi)) {
      bv = ov;
      bi = oi;
    }
  }
  if (lane == 0) nd_labels[r] = bi;
}

__global__ void __launch_bounds__(kSegThreads) k_seg_point_labels(const int32_t* __restrict__ point_rows,
                                                                const int32_t* __restrict__ nd_labels, uint64_t n,
                                                                uint64_t k, int32_t unassigned,
                                                                int32_t* __restrict__ point_labels) {
  const uint64_t i = (uint64_t)blockIdx.x * kSegThreads + threadIdx.x;
  if (i >= n) return;
  const uint64_t b = blockIdx.y;
  const int32_t row = point_rows[b * n + i];
  point_labels[b * n + i] = row >= 0 && (uint64_t)row < k ? nd_labels[b * k + (uint64_t)row] : unassigned;
}

// The labels as bytes, kSegU8Width points per thread: cloud b (grid y) is cut
// into a head of 0..3 points that brings its output to a 4-byte boundary
// (thread 0, byte stores), groups of four points -- one 16-byte row load where
// the rows of the first group are 16-byte aligned (then every group's are),
// four 4-byte loads where not, and one 4-byte store of the four labels -- and a
// tail of n' % 4 points (the thread after the last whole group, byte stores).
// The cut is per cloud, so no group spans two clouds whatever b * n is; both
// branches are uniform over the cloud.  A label is < cols <= 255: one byte.
constexpr int kSegU8Width = 4;

__global__ void __launch_bounds__(kSegThreads) k_seg_point_labels_u8(const int32_t* __restrict__ point_rows,
                                                                   const int32_t* __restrict__ nd_labels, uint64_t n,
                                                                   uint64_t k, uint32_t unassigned,
                                                                   uint8_t* __restrict__ point_labels) {
  const uint64_t b = blockIdx.y;
  const int32_t* rows = point_rows + b * n;
  const int32_t* nd = nd_labels + b * k;
  uint8_t* out = point_labels + b * n;
  uint64_t head = (uint64_t)(0 - (uintptr_t)out) & (kSegU8Width - 1);
  if (head > n) head = n;
  auto label = [&](int32_t row) -> uint32_t {
    return row >= 0 && (uint64_t)row < k ? (uint32_t)nd[(uint64_t)row] & 0xffu : unassigned;
  };
  const uint64_t t = (uint64_t)blockIdx.x * kSegThreads + threadIdx.x;
  if (t == 0) {
    for (uint64_t i = 0; i < head; i++) out[i] = (uint8_t)label(rows[i]);
    return;
  }
  const uint64_t i0 = head + (t - 1) * kSegU8Width;
  if (i0 >= n) return;
  if (i0 + kSegU8Width > n) {
    for (uint64_t i = i0; i < n; i++) out[i] = (uint8_t)label(rows[i]);
    return;
  }
  int32_t r0, r1, r2, r3;
  if ((((uintptr_t)(rows + head)) & 15) == 0) {
    const int4 v = *reinterpret_cast<const int4*>(rows + i0);
    r0 = v.x, r1 = v.y, r2 = v.z, r3 = v.w;
  } else {
    r0 = rows[i0], r1 = rows[i0 + 1], r2 = rows[i0 + 2], r3 = rows[i0 + 3];
  }
  // (little-endian: point i0 is the word's lowest byte)
  *reinterpret_cast<uint32_t*>(out + i0) = label(r0) | label(r1) << 8 | label(r2) << 16 | label(r3) << 24;
}

constexpr int kConfPPT = 8;        // points per thread per grid-stride round
constexpr int kConfMaxBlocks = 1024;
constexpr int kConfLdsCols = NDNET_SEG_CONF_LDS_MAX_COLS;
constexpr int kConfLdsBins = kConfLdsCols * kConfLdsCols + 1;

template <bool kLds>
__global__ void __launch_bounds__(kSegThreads) k_seg_confusion(const int32_t* __restrict__ pred,
                                                             const int32_t* __restrict__ gt, uint64_t count, int cols,
                                                             unsigned long long* __restrict__ conf) {
  __shared__ uint32_t hist[kLds ? kConfLdsBins : 1];
  const uint32_t bins = (uint32_t)cols * (uint32_t)cols + 1u;
  if constexpr (kLds) {
    for (uint32_t j = threadIdx.x; j < bins; j += kSegThreads) hist[j] = 0;
    __syncthreads();
  }
  // (32-bit LDS counters: a workgroup's share of the points, count / gridDim.x, stays far below 2^32)
  const uint64_t stride = (uint64_t)gridDim.x * kSegThreads * kConfPPT;
  for (uint64_t base = (uint64_t)blockIdx.x * kSegThreads * kConfPPT; base < count; base += stride) {
    int32_t p[kConfPPT], g[kConfPPT];
#pragma unroll
    for (int q = 0; q < kConfPPT; q++) {
      const uint64_t i = base + threadIdx.x + (uint64_t)kSegThreads * q;
      p[q] = i < count ? pred[i] : 0;
      g[q] = i < count ? gt[i] : 0;
    }
#pragma unroll
    for (int q = 0; q < kConfPPT; q++) {
      const uint64_t i = base + threadIdx.x + (uint64_t)kSegThreads * q;
      if (i >= count) continue;
      const bool in = p[q] >= 0 && p[q] < cols && g[q] >= 0 && g[q] < cols;
      const uint32_t bin = in ? (uint32_t)g[q] * (uint32_t)cols + (uint32_t)p[q] : bins - 1u;
      if constexpr (kLds) atomicAdd(&hist[bin], 1u);
      else atomicAdd(&conf[bin], 1ull);
    }
  }
  if constexpr (kLds) {
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < bins; j += kSegThreads) {
      const uint32_t c = hist[j];
      if (c) atomicAdd(&conf[j], (unsigned long long)c);
    }
  }
}

// hist[b][row][label] += 1 for every point of cloud b (grid y) with a row in
// 0..k-1 and a label in 0..cols-1 other than `ignore`: a thread per point, two
// coalesced int32 loads and one return-less 32-bit global atomic.  Integer
// counts: any arrival order gives the same table.
__global__ void __launch_bounds__(kSegThreads) k_seg_row_hist(const int32_t* __restrict__ point_rows,
                                                            const int32_t* __restrict__ point_labels, uint64_t n,
                                                            uint64_t k, int cols, int32_t ignore,
                                                            int32_t* __restrict__ hist) {
  const uint64_t i = (uint64_t)blockIdx.x * kSegThreads + threadIdx.x;
  if (i >= n) return;
  const uint64_t b = blockIdx.y;
  const int32_t row = point_rows[b * n + i], lb = point_labels[b * n + i];
  if (row < 0 || (uint64_t)row >= k || lb < 0 || lb >= cols || lb == ignore) return;
  int32_t* cell = hist + (b * k + (uint64_t)row) * (uint64_t)cols + (uint64_t)lb;
  (void)__hip_atomic_fetch_add(cell, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace

extern "C" {

int ndnet_seg_point_labels(const float* d_scores, const int32_t* d_point_rows, int B, uint64_t n, uint64_t k, int cols,
                           int32_t unassigned, int32_t* d_nd_labels, int32_t* d_point_labels, void* stream) {
  if (!d_scores || !d_point_rows || !d_nd_labels || !d_point_labels || B < 1 || n < 1 || k < 1 || cols < 1)
    return NDNET_ERR_ARG;
  const uint64_t rows = (uint64_t)B * k, pblocks = (n + kSegThreads - 1) / kSegThreads;
  const uint64_t rblocks = (rows + kSegThreads / 64 - 1) / (kSegThreads / 64);
  if (rblocks > 0x7fffffffull || pblocks > 0x7fffffffull || B > 65535) return NDNET_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  k_seg_nd_argmax<<<(uint32_t)rblocks, kSegThreads, 0, st>>>(d_scores, rows, cols, d_nd_labels);
  k_seg_point_labels<<<dim3((uint32_t)pblocks, (uint32_t)B), kSegThreads, 0, st>>>(d_point_rows, d_nd_labels, n, k,
                                                                                  unassigned, d_point_labels);
  SEG_HIPCHK(hipGetLastError());
  return NDNET_OK;
}

int ndnet_seg_point_labels_u8(const float* d_scores, const int32_t* d_point_rows, int B, uint64_t n, uint64_t k, int cols,
                              uint8_t unassigned, int32_t* d_nd_labels, uint8_t* d_point_labels, void* stream) {
  if (!d_scores || !d_point_rows || !d_nd_labels || !d_point_labels || B < 1 || n < 1 || k < 1 || cols < 1)
    return NDNET_ERR_ARG;
  if (cols > 255 || (int)unassigned < cols) return NDNET_ERR_ARG;  // a class is a byte; the marker is no class
  // thread 0 of a cloud takes its head, the next ceil(n / 4) its groups and tail
  const uint64_t rows = (uint64_t)B * k, threads = 1 + (n + kSegU8Width - 1) / kSegU8Width;
  const uint64_t pblocks = (threads + kSegThreads - 1) / kSegThreads;
  const uint64_t rblocks = (rows + kSegThreads / 64 - 1) / (kSegThreads / 64);
  if (rblocks > 0x7fffffffull || pblocks > 0x7fffffffull || B > 65535) return NDNET_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  k_seg_nd_argmax<<<(uint32_t)rblocks, kSegThreads, 0, st>>>(d_scores, rows, cols, d_nd_labels);
  k_seg_point_labels_u8<<<dim3((uint32_t)pblocks, (uint32_t)B), kSegThreads, 0, st>>>(
      d_point_rows, d_nd_labels, n, k, (uint32_t)unassigned, d_point_labels);
  SEG_HIPCHK(hipGetLastError());
  return NDNET_OK;
}

int ndnet_seg_confusion(const int32_t* d_pred, const int32_t* d_gt, uint64_t count, int cols,
                        unsigned long long* d_conf, void* stream) {
  if (!d_pred || !d_gt || !d_conf || count == 0 || cols < 1 || cols > 46340) return NDNET_ERR_ARG;  // cols^2 + 1 in 32 bits
  const uint64_t per = (uint64_t)kSegThreads * kConfPPT;
  uint64_t blocks = (count + per - 1) / per;
  if (blocks > (uint64_t)kConfMaxBlocks) blocks = kConfMaxBlocks;
  hipStream_t st = (hipStream_t)stream;
  if (cols <= kConfLdsCols) k_seg_confusion<true><<<(uint32_t)blocks, kSegThreads, 0, st>>>(d_pred, d_gt, count, cols, d_conf);
  else k_seg_confusion<false><<<(uint32_t)blocks, kSegThreads, 0, st>>>(d_pred, d_gt, count, cols, d_conf);
  SEG_HIPCHK(hipGetLastError());
  return NDNET_OK;
}

int ndnet_seg_row_hist(const int32_t* d_point_rows, const int32_t* d_point_labels, int B, uint64_t n, uint64_t k,
                       int cols, int32_t ignore_label, int32_t* d_hist, void* stream) {
  if (!d_point_rows || !d_point_labels || !d_hist || B < 1 || n < 1 || k < 1 || cols < 1) return NDNET_ERR_ARG;
  const uint64_t pblocks = (n + kSegThreads - 1) / kSegThreads;
  // (rows are int32, so k above 2^31 holds no more of them; the table's bytes stay in 64 bits)
  if (pblocks > 0x7fffffffull || B > 65535 || k > 0x80000000ull) return NDNET_ERR_ARG;
  if ((uint64_t)B * k > (1ull << 60) / (uint64_t)cols) return NDNET_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  SEG_HIPCHK(hipMemsetAsync(d_hist, 0, (uint64_t)B * k * (uint64_t)cols * sizeof(int32_t), st));
  k_seg_row_hist<<<dim3((uint32_t)pblocks, (uint32_t)B), kSegThreads, 0, st>>>(d_point_rows, d_point_labels, n, k, cols,
                                                                              ignore_label, d_hist);
  SEG_HIPCHK(hipGetLastError());
  return NDNET_OK;
}

}  // extern "C"
