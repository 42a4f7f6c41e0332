// fps_kernels.hip -- farthest point sampling on gfx950 (include/ndnet_fps.h).
//
//   k_fps<T>  one workgroup of 512 threads (8 waves, two per SIMD) per cloud,
//             thread i owns the points i, i + 512, ... ("slab" q holds the
//             points 512 q .. 512 q + 511).  The running squared distances of
//             the first kRegSlabs slabs live in registers (196 of the 256 a
//             wave has at two waves per SIMD), those of later slabs in
//             d_min_dist; the coordinates of the first kLdsSlabs slabs in LDS
//             (x, y and z rows of 512, lane-linear: conflict-free), the others
//             stream from L2 in chunks of kChunk slabs whose loads are issued
//             together.  Per sample: every thread folds its points into a
//             (value, index) maximum, the wave reduces it across lanes (DPP
//             for the steps inside a row of 16, ds_bpermute for 16 and 32),
//             lane 0 of every wave leaves it in LDS, one barrier, and every
//             thread reduces the eight pairs itself.  The pairs' slots
//             alternate between two sets by the sample's parity, so the one
//             barrier per sample also keeps a fast wave from overwriting what
//             a slow one still reads.  The loop runs min(n_samples, m) trips
//             and waits on nothing outside the workgroup.
//
// Built with -ffp-contract=off: d = (dx*dx + dy*dy) + dz*dz rounds every
// operation in T (the definition in the header).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <utility>

#include "../../include/ndnet_amd.h"
#include "../../include/ndnet_fps.h"

namespace {

#define FPS_HIPCHK(x)                                                         \
  do {                                                                        \
    hipError_t e_ = (x);                                                      \
    if (e_ != hipSuccess) {                                                   \
      fprintf(stderr, "ndnet_amd: %s: %s\n", #x, hipGetErrorString(e_));      \
      return NDNET_ERR_HIP;                                                   \
    }                                                                         \
  } while (0)

constexpr int kT = NDNET_FPS_THREADS;
constexpr int kWaves = kT / 64;

template <typename T> struct FpsCfg;
template <> struct FpsCfg<float> {
  static constexpr int kRegSlabs = NDNET_FPS_REG_POINTS_F32 / kT, kLdsSlabs = NDNET_FPS_LDS_POINTS_F32 / kT;
  static constexpr int kChunk = NDNET_FPS_CHUNK_SLABS_F32;  // slabs whose coordinate loads are in flight together (21 registers)
};
template <> struct FpsCfg<double> {
  static constexpr int kRegSlabs = NDNET_FPS_REG_POINTS_F64 / kT, kLdsSlabs = NDNET_FPS_LDS_POINTS_F64 / kT;
  static constexpr int kChunk = NDNET_FPS_CHUNK_SLABS_F64;  // (24 registers)
};
static_assert(NDNET_FPS_REG_POINTS_F32 % (kT * FpsCfg<float>::kChunk) == 0, "");
static_assert(NDNET_FPS_REG_POINTS_F64 % (kT * FpsCfg<double>::kChunk) == 0, "");
static_assert(NDNET_FPS_LDS_POINTS_F32 % kT == 0 && NDNET_FPS_LDS_POINTS_F64 % kT == 0, "");

// every 32-bit word of v from another lane of the row (DPP control kCtrl)
template <int kCtrl, typename V> __device__ __forceinline__ V fps_dpp(V v) {
  static_assert(sizeof(V) % 4 == 0, "");
  int w[sizeof(V) / 4];
  __builtin_memcpy(w, &v, sizeof(V));
#pragma unroll
  for (unsigned i = 0; i < sizeof(V) / 4; i++) w[i] = __builtin_amdgcn_update_dpp(w[i], w[i], kCtrl, 0xf, 0xf, false);
  __builtin_memcpy(&v, w, sizeof(V));
  return v;
}

// (v, i) becomes the greater of (v, i) and (ov, oi): greater value, or equal value and smaller
// index -- a total order, so the result does not depend on how points are dealt to lanes
template <typename T> __device__ __forceinline__ void fps_take(T& v, uint32_t& i, T ov, uint32_t oi) {
  if (ov > v || (ov == v && oi < i)) {
    v = ov;
    i = oi;
  }
}

// all 64 lanes end with the wave's maximum.  Lanes ^1 and ^2 (quad permutes), then the mirrored
// half row and the mirrored row: each step's groups are uniform by then, so a mirror is as good
// as an xor; 16 and 32 cross rows and go through ds_bpermute.
template <typename T> __device__ __forceinline__ void fps_wave_max(T& v, uint32_t& i) {
  fps_take(v, i, fps_dpp<0xB1>(v), fps_dpp<0xB1>(i));    // quad_perm [1,0,3,2]
  fps_take(v, i, fps_dpp<0x4E>(v), fps_dpp<0x4E>(i));    // quad_perm [2,3,0,1]
  fps_take(v, i, fps_dpp<0x141>(v), fps_dpp<0x141>(i));  // row_half_mirror
  fps_take(v, i, fps_dpp<0x140>(v), fps_dpp<0x140>(i));  // row_mirror
  fps_take(v, i, __shfl_xor(v, 16, 64), __shfl_xor(i, 16, 64));
  fps_take(v, i, __shfl_xor(v, 32, 64), __shfl_xor(i, 32, 64));
}

template <typename T> struct FpsPoint {
  T x, y, z;
};

// One chunk of kChunk register slabs from slab kQ0 on: the coordinate loads first, all in flight
// together, then the arithmetic.  kTail is the chunk that holds the cloud's end: its slabs past
// the end cost their arithmetic and change nothing (kAbsent), and its loads are clamped to the
// last point; a full chunk's loads are the scalar base pq plus one lane offset.  The best slab is
// kept as its number, and the picked point found by tid == cur - 512 q, so that nothing per slab
// is invariant over the samples (the compiler would keep 196 of it in registers).
template <typename T, int kQ0, bool kTail>
__device__ __forceinline__ void fps_chunk(T (&mind)[FpsCfg<T>::kRegSlabs], const T* s_xyz,
                                          const FpsPoint<T>* __restrict__ p,
                                          uint32_t tid, uint32_t last, uint32_t cur, T cx, T cy, T cz, T& best,
                                          uint32_t& bq) {
  constexpr int QL = FpsCfg<T>::kLdsSlabs, kChunk = FpsCfg<T>::kChunk;
  T x[kChunk], y[kChunk], z[kChunk];
#pragma unroll
  for (int c = 0; c < kChunk; c++) {
    const int q = kQ0 + c;
    if (q < QL) {
      x[c] = s_xyz[(q * 3 + 0) * kT + tid];
      y[c] = s_xyz[(q * 3 + 1) * kT + tid];
      z[c] = s_xyz[(q * 3 + 2) * kT + tid];
    } else {
      // (a register slab: its indices are far below 2^32 / 3)
      const uint32_t j = (uint32_t)q * kT + tid;
      const FpsPoint<T> v = kTail ? p[j < last ? j : last] : (p + (uint32_t)q * kT)[tid];
      x[c] = v.x;
      y[c] = v.y;
      z[c] = v.z;
    }
  }
#pragma unroll
  for (int c = 0; c < kChunk; c++) {
    const int q = kQ0 + c;
    const T dx = x[c] - cx, dy = y[c] - cy, dz = z[c] - cz;
    const T d = (dx * dx + dy * dy) + dz * dz;
    T md = tid == cur - (uint32_t)q * kT ? (T)-1 : mind[q];
    if (d < md) md = d;
    mind[q] = md;
    if (md > best) {  // (a thread's indices grow with q: a later equal value does not displace an earlier one)
      best = md;
      bq = (uint32_t)q;
    }
  }
}

// the chunks in order, up to the one that holds the cloud's end (the fold's && is the loop's break;
// written as a fold so that every mind[] index is a constant and the array stays in registers)
template <typename T, int... kC>
__device__ __forceinline__ void fps_chunks(std::integer_sequence<int, kC...>, T (&mind)[FpsCfg<T>::kRegSlabs],
                                           const T* s_xyz, const FpsPoint<T>* __restrict__ p, uint32_t tid, uint32_t m,
                                           uint32_t cur, T cx, T cy, T cz, T& best, uint32_t& bq) {
  constexpr int kChunk = FpsCfg<T>::kChunk;
  (void)(((uint32_t)(kC * kChunk) * kT < m &&
          ((uint32_t)((kC + 1) * kChunk) * kT <= m
               ? fps_chunk<T, kC * kChunk, false>(mind, s_xyz, p, tid, m - 1, cur, cx, cy, cz, best, bq)
               : fps_chunk<T, kC * kChunk, true>(mind, s_xyz, p, tid, m - 1, cur, cx, cy, cz, best, bq),
           true)) &&
         ...);
}

template <typename T>
__global__ void __launch_bounds__(kT) k_fps(const T* __restrict__ points, uint32_t n, uint32_t n_samples,
                                            const int32_t* __restrict__ counts, const int32_t* __restrict__ start,
                                            T* __restrict__ min_dist, int32_t* __restrict__ indices) {
  constexpr int R = FpsCfg<T>::kRegSlabs, QL = FpsCfg<T>::kLdsSlabs;
  constexpr uint32_t kRegPoints = (uint32_t)R * kT, kLdsPoints = (uint32_t)QL * kT;
  __shared__ T s_xyz[QL * 3 * kT];  // [slab][x, y, z][thread]
  __shared__ T s_val[2][kWaves];
  __shared__ uint32_t s_idx[2][kWaves];

  const uint32_t tid = threadIdx.x;
  const uint64_t b = blockIdx.x;
  const T* __restrict__ p = points + b * n * 3;
  T* __restrict__ gmind = min_dist + b * n;
  int32_t* __restrict__ out = indices + b * n_samples;

  uint32_t m = n;
  if (counts) {
    const int32_t c = counts[b];
    m = c < 1 ? 1u : (uint32_t)c > n ? n : (uint32_t)c;
  }
  uint32_t cur = 0;
  if (start) {
    const int32_t s = start[b];
    cur = s < 0 ? 0u : (uint32_t)s >= m ? m - 1 : (uint32_t)s;
  }
  const uint32_t trips = n_samples < m ? n_samples : m;
  const uint32_t last = m - 1;
  const T kInf = (T)__builtin_inff();
  const T kAbsent = (T)-2;  // a lane's slot past the cloud's end: below every real value, and no d is less

  for (int q = 0; q < QL; q++) {
    if ((uint32_t)q * kT >= m) break;
    const uint32_t j = (uint32_t)q * kT + tid;
    const uint64_t jj = j < last ? j : last;
    s_xyz[(q * 3 + 0) * kT + tid] = p[jj * 3 + 0];
    s_xyz[(q * 3 + 1) * kT + tid] = p[jj * 3 + 1];
    s_xyz[(q * 3 + 2) * kT + tid] = p[jj * 3 + 2];
  }
  T mind[R];
#pragma unroll
  for (int q = 0; q < R; q++) mind[q] = (uint32_t)q * kT + tid < m ? kInf : kAbsent;
  for (uint64_t j = (uint64_t)kRegPoints + tid; j < m; j += kT) gmind[j] = kInf;
  __syncthreads();

  for (uint32_t t = 0; t < trips; t++) {
    cur = (uint32_t)__builtin_amdgcn_readfirstlane((int)cur);  // (uniform already: lets the loads below be scalar)
    T cx, cy, cz;
    if (cur < kLdsPoints) {
      const uint32_t q = cur / kT, l = cur % kT;
      cx = s_xyz[(q * 3 + 0) * kT + l];
      cy = s_xyz[(q * 3 + 1) * kT + l];
      cz = s_xyz[(q * 3 + 2) * kT + l];
    } else {
      cx = p[(uint64_t)cur * 3 + 0];
      cy = p[(uint64_t)cur * 3 + 1];
      cz = p[(uint64_t)cur * 3 + 2];
    }
    if (tid == 0) out[t] = (int32_t)cur;

    T best = kAbsent;
    uint32_t bq = 0x7fffffu;  // no slab: 512 bq + tid is past every index
    // (what a slab derives from these is made anew on every sample; derived from tid, m and p
    // themselves it would be kept in registers across the samples, 196 times over)
    uint32_t tl = tid, ml = m, zero = 0;
    asm volatile("" : "+s"(zero), "+v"(tl), "+s"(ml));
    tl &= kT - 1;  // (known to be small again: a lane's byte offset fits 32 bits)
    const FpsPoint<T>* __restrict__ pt = (const FpsPoint<T>*)p + zero;
    fps_chunks<T>(std::make_integer_sequence<int, R / FpsCfg<T>::kChunk>{}, mind, s_xyz, pt, tl, ml, cur, cx, cy, cz, best, bq);
    uint32_t bi = bq * kT + tid;
#pragma unroll 4
    for (uint32_t j0 = kRegPoints; j0 < m; j0 += kT) {
      const uint32_t j = j0 + tid;
      if (j < m) {
        const uint64_t jj = j;
        const T dx = p[jj * 3 + 0] - cx, dy = p[jj * 3 + 1] - cy, dz = p[jj * 3 + 2] - cz;
        const T d = (dx * dx + dy * dy) + dz * dz;
        T md = j == cur ? (T)-1 : gmind[j];
        if (d < md) md = d;
        gmind[j] = md;
        if (md > best) {
          best = md;
          bi = j;
        }
      }
    }

    fps_wave_max(best, bi);
    const int par = t & 1;
    if ((tid & 63) == 0) {
      s_val[par][tid >> 6] = best;
      s_idx[par][tid >> 6] = bi;
    }
    __syncthreads();
    best = s_val[par][0];
    bi = s_idx[par][0];
#pragma unroll
    for (int w = 1; w < kWaves; w++) fps_take(best, bi, s_val[par][w], s_idx[par][w]);
    cur = bi;
  }

  for (uint32_t t = trips + tid; t < n_samples; t += kT) out[t] = -1;
  uint32_t te = tid, me = m;
  asm volatile("" : "+v"(te), "+s"(me));  // (as in the loop: the stores' indices and masks are made here)
#pragma unroll
  for (int q = 0; q < R; q++) {
    const uint32_t j = (uint32_t)q * kT + te;
    if (j < me) gmind[j] = mind[q];
  }
}

template <typename T>
int fps_run(const T* d_points, int B, uint64_t n, uint64_t n_samples, const int32_t* d_counts, const int32_t* d_start,
            void* d_min_dist, int32_t* d_indices, void* stream) {
  if (!d_points || !d_min_dist || !d_indices || B < 1 || n < 1 || n_samples < 1 || n_samples > n || n >= (1ull << 31))
    return NDNET_ERR_ARG;
  k_fps<T><<<(uint32_t)B, kT, 0, (hipStream_t)stream>>>(d_points, (uint32_t)n, (uint32_t)n_samples, d_counts, d_start,
                                                       (T*)d_min_dist, d_indices);
  FPS_HIPCHK(hipGetLastError());
  return NDNET_OK;
}

}  // namespace

extern "C" {

int ndnet_fps_run(const float* d_points, int B, uint64_t n, uint64_t n_samples, const int32_t* d_counts,
                  const int32_t* d_start, void* d_min_dist, int32_t* d_indices, void* stream) {
  return fps_run<float>(d_points, B, n, n_samples, d_counts, d_start, d_min_dist, d_indices, stream);
}

int ndnet_fps_run_f64(const double* d_points, int B, uint64_t n, uint64_t n_samples, const int32_t* d_counts,
                      const int32_t* d_start, void* d_min_dist, int32_t* d_indices, void* stream) {
  return fps_run<double>(d_points, B, n, n_samples, d_counts, d_start, d_min_dist, d_indices, stream);
}

}  // extern "C"
