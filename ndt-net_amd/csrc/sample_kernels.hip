// sample_kernels.hip -- the exact-size random subsample on gfx950 (include/ndnet_sample.h).
//
//   k_smp_init    one workgroup per cloud clears the cloud's histogram; the first
//                 one reads the step, snapshots it into the work buffer and leaves
//                 step + 1 when the call advances.
//   k_smp_keys    one workgroup per tile of NDNET_SAMPLE_TILE points: Philox, the
//                 keys into the work buffer, the histogram of their top 8 bits
//                 through LDS atomics and from there the non-empty bins to the
//                 cloud's histogram with vector atomics.  Reads no point data.
//   k_smp_select  one workgroup of 1024 threads per cloud: the bin that holds the
//                 S-th smallest key by a scan of the 256 counts, then 8 more bits
//                 per pass -- over the bin's keys in LDS when they are at most
//                 NDNET_SAMPLE_LIST (about n / 256 of them at 32 bits: one read of
//                 the cloud's keys, four 16-byte loads in flight per thread),
//                 else over the cloud's keys again.  Publishes tau and the tie
//                 quota.
//   k_smp_count   per tile: the keys below tau and the keys equal to it.
//   k_smp_apply   per tile: sums its cloud's preceding tile counts itself, ranks
//                 the tile's ties and then its chosen points in input order (a
//                 ballot per slab of 256, the wave counts through LDS) and writes
//                 index, point and label at the row.  A cloud with m <= S is
//                 copied whole and the tiles fill the rows m .. S - 1 they cover.
//   k_smp_gather  ndnet_sample_gather_run: one row per thread; the first workgroup
//                 of a cloud also counts the cloud's valid rows.
//
// A cloud with m <= S skips the keys, the threshold and the counts.  Five
// dependent launches; ordering comes from the kernel boundaries alone, no
// workgroup waits on another.  Integer only: nothing here rounds.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/ndnet_amd.h"
#include "../../include/ndnet_sample.h"

namespace {

#define SMP_HIPCHK(x)                                                         \
  do {                                                                        \
    hipError_t e_ = (x);                                                      \
    if (e_ != hipSuccess) {                                                   \
      fprintf(stderr, "ndnet_amd: %s: %s\n", #x, hipGetErrorString(e_));      \
      return NDNET_ERR_HIP;                                                   \
    }                                                                         \
  } while (0)

constexpr int kT = 256;                        // threads of every workgroup here
constexpr int kWaves = kT / 64;
constexpr int kPPT = NDNET_SAMPLE_TILE / kT;   // a thread's points per tile
constexpr int kSlabs = kPPT * kWaves;          // (slab of 256 points, wave) pairs of a tile, in input order
constexpr int kBins = 256;                     // 8 bits per radix pass: one bin per thread
constexpr int kSelT = 1024;                    // threads of k_smp_select
constexpr int kSelWaves = kSelT / 64;
static_assert(NDNET_SAMPLE_TILE % kT == 0 && kPPT >= 1 && kBins == kT && kBins <= kSelT, "");

constexpr uint32_t kPurposeSample = 3;  // the purpose ndnet_augment.h leaves unused

// the work buffer: SmpHead | tau [B] | quota [B] | hist [B][256] | tile counts [B][tiles][2] | keys [B][stride],
// the keys 16-byte aligned and a cloud's stride n rounded up to 4 (k_smp_select loads four keys at a time)
struct SmpHead {
  uint64_t step;  // the call's step, snapshotted by k_smp_init
  uint64_t pad;
};

__host__ __device__ inline uint32_t smp_tiles(uint32_t n) { return (n + NDNET_SAMPLE_TILE - 1) / NDNET_SAMPLE_TILE; }
__host__ __device__ inline uint32_t* work_tau(void* w) { return (uint32_t*)((char*)w + sizeof(SmpHead)); }
__host__ __device__ inline uint32_t* work_quota(void* w, int B) { return work_tau(w) + B; }
__host__ __device__ inline uint32_t* work_hist(void* w, int B) { return work_quota(w, B) + B; }
__host__ __device__ inline uint32_t* work_tiles(void* w, int B) { return work_hist(w, B) + (size_t)kBins * B; }
__host__ __device__ inline uint32_t key_stride(uint32_t n) { return (n + 3u) & ~3u; }
__host__ __device__ inline size_t keys_offset(int B, uint32_t n) {  // in words from the head's end, a multiple of 4
  return (((size_t)B * (2 + (size_t)kBins + 2 * (size_t)smp_tiles(n))) + 3) & ~(size_t)3;
}
__host__ __device__ inline uint32_t* work_keys(void* w, int B, uint32_t n) { return work_tau(w) + keys_offset(B, n); }

// Philox4x32-10 as ndnet_augment.h defines it; word 0
__device__ __forceinline__ uint32_t philox_w0(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                              uint32_t k1) {
  constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;
#pragma unroll
  for (int r = 0; r < 10; r++) {
    const uint64_t p0 = (uint64_t)M0 * c0, p1 = (uint64_t)M1 * c2;
    const uint32_t h0 = (uint32_t)(p0 >> 32), l0 = (uint32_t)p0, h1 = (uint32_t)(p1 >> 32), l1 = (uint32_t)p1;
    const uint32_t n0 = h1 ^ c1 ^ k0, n2 = h0 ^ c3 ^ k1;
    c0 = n0;
    c1 = l1;
    c2 = n2;
    c3 = l0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c0;
}

__device__ __forceinline__ uint32_t cloud_len(const int32_t* counts, int b, uint32_t n) {
  if (!counts) return n;
  const int32_t c = counts[b];
  return c < 1 ? 1u : (uint32_t)c > n ? n : (uint32_t)c;
}

__global__ void __launch_bounds__(kT) k_smp_init(int B, int advance, uint64_t* __restrict__ d_step,
                                                 void* __restrict__ work) {
  work_hist(work, B)[(size_t)blockIdx.x * kBins + threadIdx.x] = 0;
  if (blockIdx.x == 0 && threadIdx.x == 0) {  // the one reader and writer of the counter
    const uint64_t step = *d_step;
    ((SmpHead*)work)->step = step;
    if (advance) *d_step = step + 1;
  }
}

__global__ void __launch_bounds__(kT) k_smp_keys(uint32_t k0, uint32_t k1, int key_bits,
                                                 const int32_t* __restrict__ counts, uint32_t n, uint32_t S, int B,
                                                 void* __restrict__ work) {
  __shared__ uint32_t s_hist[kBins];
  const uint32_t b = blockIdx.y, tile = blockIdx.x, t = threadIdx.x;
  const uint32_t m = cloud_len(counts, (int)b, n);
  const uint32_t start = tile * NDNET_SAMPLE_TILE;
  if (m <= S || start >= m) return;  // the whole cloud is taken, or a tile of padding
  s_hist[t] = 0;
  __syncthreads();
  const uint64_t step = ((const SmpHead*)work)->step;
  const uint32_t c2 = (uint32_t)step, c3 = ((uint32_t)(step >> 32) << 2) | kPurposeSample;
  const int top = key_bits > 8 ? key_bits - 8 : 0;  // the first pass reads the bits above `top`
  uint32_t* keys = work_keys(work, B, n) + (uint64_t)b * key_stride(n);
#pragma unroll
  for (int q = 0; q < kPPT; q++) {
    const uint32_t i = start + t + kT * q;  // (< 2^31 + 1024)
    if (i < m) {
      const uint32_t key = philox_w0(i, b, c2, c3, k0, k1) >> (32 - key_bits);
      keys[i] = key;
      atomicAdd(&s_hist[key >> top], 1u);  // (key >> top < 256)
    }
  }
  __syncthreads();
  const uint32_t h = s_hist[t];
  if (h) atomicAdd(&work_hist(work, B)[(size_t)b * kBins + t], h);
}

// The bin of the r-th entry (1 <= r <= the sum) of a 256-bin histogram, one count per thread (0 in the
// threads past the bins): every thread leaves with the bin, the entries below it and its count.
__device__ __forceinline__ void pick_bin(uint32_t h, uint32_t r, uint32_t* s_wave, uint32_t* s_pick, uint32_t& bin,
                                         uint32_t& below, uint32_t& cnt) {
  const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6;
  uint32_t inc = h;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t v = __shfl_up(inc, d, 64);
    if (lane >= (uint32_t)d) inc += v;
  }
  if (lane == 63) s_wave[wave] = inc;
  __syncthreads();
  uint32_t excl = inc - h;
#pragma unroll
  for (int w = 0; w < kSelWaves; w++)
    if ((uint32_t)w < wave) excl += s_wave[w];
  if (excl < r && r <= excl + h) {  // exactly one thread
    s_pick[0] = t;
    s_pick[1] = excl;
    s_pick[2] = h;
  }
  __syncthreads();
  bin = s_pick[0];
  below = s_pick[1];
  cnt = s_pick[2];
  __syncthreads();  // s_wave and s_pick are free again
}

// f(key) for every key of a cloud, the workgroup's threads striding over groups of four keys with four
// 16-byte loads issued before the first use (the keys' rows are 16-byte aligned and padded to 4)
template <class F>
__device__ __forceinline__ void for_each_key(const uint32_t* __restrict__ keys, uint32_t m, F f) {
  const uint4* k4 = (const uint4*)keys;
  const uint32_t groups = (m + 3) / 4;
  for (uint32_t j0 = threadIdx.x; j0 < groups; j0 += 4 * kSelT) {
    uint4 v[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const uint32_t j = j0 + u * kSelT;
      v[u] = j < groups ? k4[j] : uint4{0, 0, 0, 0};
    }
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const uint32_t i = 4 * (j0 + u * kSelT);  // (>= m past the last group)
      if (i < m) f(v[u].x);
      if (i + 1 < m) f(v[u].y);
      if (i + 2 < m) f(v[u].z);
      if (i + 3 < m) f(v[u].w);
    }
  }
}

__global__ void __launch_bounds__(kSelT) k_smp_select(int key_bits, const int32_t* __restrict__ counts, uint32_t n,
                                                   uint32_t S, int B, void* __restrict__ work) {
  __shared__ uint32_t s_hist[kBins];
  __shared__ uint32_t s_list[NDNET_SAMPLE_LIST];
  __shared__ uint32_t s_wave[kSelWaves];
  __shared__ uint32_t s_pick[3];
  __shared__ uint32_t s_n;
  const uint32_t b = blockIdx.x, t = threadIdx.x;
  const uint32_t m = cloud_len(counts, (int)b, n);
  if (m <= S) return;  // the whole cloud is taken: no threshold
  if (t < 3) s_pick[t] = 0;
  if (t == 0) s_n = 0;
  __syncthreads();
  const uint32_t* keys = work_keys(work, B, n) + (uint64_t)b * key_stride(n);
  int shift = key_bits > 8 ? key_bits - 8 : 0;  // the bits still open below the prefix
  uint32_t r = S;                               // the rank wanted among the keys that share the prefix
  uint32_t prefix, below, cnt;
  pick_bin(t < (uint32_t)kBins ? work_hist(work, B)[(size_t)b * kBins + t] : 0u, r, s_wave, s_pick, prefix, below,
           cnt);
  r -= below;
  bool listed = false;
  while (shift > 0) {
    const int d = shift > 8 ? 8 : shift, low = shift - d;
    if (!listed && cnt <= (uint32_t)NDNET_SAMPLE_LIST) {  // (uniform) the bin's keys into LDS, in any order
      for_each_key(keys, m, [&](uint32_t key) {
        if ((key >> shift) == prefix) {
          const uint32_t j = atomicAdd(&s_n, 1u);
          if (j < (uint32_t)NDNET_SAMPLE_LIST) s_list[j] = key;
        }
      });
      listed = true;
    }
    if (t < (uint32_t)kBins) s_hist[t] = 0;
    __syncthreads();
    const uint32_t mask = (1u << d) - 1u;
    if (listed) {
      const uint32_t len = s_n < (uint32_t)NDNET_SAMPLE_LIST ? s_n : (uint32_t)NDNET_SAMPLE_LIST;
      for (uint32_t j = t; j < len; j += kSelT) {
        const uint32_t key = s_list[j];
        if ((key >> shift) == prefix) atomicAdd(&s_hist[(key >> low) & mask], 1u);
      }
    } else {
      for_each_key(keys, m, [&](uint32_t key) {
        if ((key >> shift) == prefix) atomicAdd(&s_hist[(key >> low) & mask], 1u);
      });
    }
    __syncthreads();
    uint32_t bin;
    pick_bin(t < (uint32_t)kBins ? s_hist[t] : 0u, r, s_wave, s_pick, bin, below, cnt);
    prefix = (prefix << d) | bin;
    r -= below;
    shift = low;
  }
  if (t == 0) {
    work_tau(work)[b] = prefix;     // the S-th smallest key
    work_quota(work, B)[b] = r;     // S - #{key < tau}: the ties taken, lowest indices first
  }
}

__global__ void __launch_bounds__(kT) k_smp_count(const int32_t* __restrict__ counts, uint32_t n, uint32_t S, int B,
                                                  void* __restrict__ work) {
  __shared__ uint32_t s_lt[kWaves], s_eq[kWaves];
  const uint32_t b = blockIdx.y, tile = blockIdx.x, t = threadIdx.x;
  const uint32_t m = cloud_len(counts, (int)b, n);
  if (m <= S) return;  // (the apply pass reads no counts of such a cloud)
  uint32_t* out = work_tiles(work, B) + 2 * ((uint64_t)b * smp_tiles(n) + tile);
  const uint32_t start = tile * NDNET_SAMPLE_TILE;
  if (start >= m) {  // a tile of padding
    if (t < 2) out[t] = 0;
    return;
  }
  const uint32_t tau = work_tau(work)[b];
  const uint32_t* keys = work_keys(work, B, n) + (uint64_t)b * key_stride(n);
  uint32_t lt = 0, eq = 0;
#pragma unroll
  for (int q = 0; q < kPPT; q++) {
    const uint32_t i = start + t + kT * q;
    if (i < m) {
      const uint32_t key = keys[i];
      lt += key < tau ? 1u : 0u;
      eq += key == tau ? 1u : 0u;
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    lt += __shfl_xor(lt, d, 64);
    eq += __shfl_xor(eq, d, 64);
  }
  if ((t & 63) == 0) {
    s_lt[t >> 6] = lt;
    s_eq[t >> 6] = eq;
  }
  __syncthreads();
  if (t == 0) {
    uint32_t a = 0, e = 0;
#pragma unroll
    for (int w = 0; w < kWaves; w++) {
      a += s_lt[w];
      e += s_eq[w];
    }
    out[0] = a;
    out[1] = e;
  }
}

// the 16 (slab, wave) counts of a tile through LDS: every thread leaves with the flagged points
// before its own in input order.  s_cnt must not be in use (one barrier inside).
__device__ __forceinline__ void tile_ranks(const bool (&flag)[kPPT], uint32_t* s_cnt, uint32_t (&rank)[kPPT]) {
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t below[kPPT];
#pragma unroll
  for (int q = 0; q < kPPT; q++) {
    const unsigned long long mask = __ballot(flag[q]);
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
}

__device__ __forceinline__ void put_row(uint64_t row, int32_t index, const float* __restrict__ src,
                                        int32_t label, float* __restrict__ out_pts, int32_t* __restrict__ out_labels,
                                        int32_t* __restrict__ out_indices) {
  const float x = src[0], y = src[1], z = src[2];
  out_pts[3 * row] = x;
  out_pts[3 * row + 1] = y;
  out_pts[3 * row + 2] = z;
  if (out_labels) out_labels[row] = label;
  if (out_indices) out_indices[row] = index;
}

__global__ void __launch_bounds__(kT) k_smp_apply(const float* __restrict__ pts, const int32_t* __restrict__ labels,
                                                  const int32_t* __restrict__ counts, uint32_t n, uint32_t S, int B,
                                                  int32_t fill_label, const void* work_c,
                                                  float* __restrict__ out_pts, int32_t* __restrict__ out_labels,
                                                  int32_t* __restrict__ out_indices,
                                                  int32_t* __restrict__ out_counts) {
  __shared__ uint32_t s_eq[kSlabs], s_take[kSlabs];
  __shared__ uint32_t s_base[2 * kWaves];
  void* work = const_cast<void*>(work_c);
  const uint32_t b = blockIdx.y, tile = blockIdx.x, t = threadIdx.x;
  const uint32_t m = cloud_len(counts, (int)b, n);
  const uint32_t start = tile * NDNET_SAMPLE_TILE;
  const float* p = pts + (uint64_t)b * n * 3;             // the cloud's points
  const int32_t* lab = labels ? labels + (uint64_t)b * n : nullptr;
  const uint64_t out0 = (uint64_t)b * S;                  // the cloud's first output row
  if (tile == 0 && t == 0) out_counts[b] = (int32_t)(m < S ? m : S);

  if (m <= S) {  // the whole cloud, row = index; this tile's share of the filler rows m .. S - 1
#pragma unroll
    for (int q = 0; q < kPPT; q++) {
      const uint32_t i = start + t + kT * q;
      if (i < m) put_row(out0 + i, (int32_t)i, p + 3 * (uint64_t)i, lab ? lab[i] : 0, out_pts, out_labels, out_indices);
      else if (i < S) put_row(out0 + i, -1, p, fill_label, out_pts, out_labels, out_indices);
    }
    return;
  }
  if (start >= m) return;  // a tile of padding: nothing read, nothing written

  // the cloud's keys below and at the threshold before this tile
  {
    const uint32_t* tc = work_tiles(work, B) + 2 * (uint64_t)b * smp_tiles(n);
    uint32_t a = 0, e = 0;
    for (uint32_t j = t; j < tile; j += kT) {
      a += tc[2 * j];
      e += tc[2 * j + 1];
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      a += __shfl_xor(a, d, 64);
      e += __shfl_xor(e, d, 64);
    }
    if ((t & 63) == 0) {
      s_base[t >> 6] = a;
      s_base[kWaves + (t >> 6)] = e;
    }
  }
  __syncthreads();
  uint32_t base_lt = 0, base_eq = 0;
#pragma unroll
  for (int w = 0; w < kWaves; w++) {
    base_lt += s_base[w];
    base_eq += s_base[kWaves + w];
  }
  const uint32_t tau = work_tau(work)[b], quota = work_quota(work, B)[b];
  const uint32_t* keys = work_keys(work, B, n) + (uint64_t)b * key_stride(n);
  bool lt[kPPT], eq[kPPT];
#pragma unroll
  for (int q = 0; q < kPPT; q++) {
    const uint32_t i = start + t + kT * q;
    const uint32_t key = i < m ? keys[i] : 0u;
    lt[q] = i < m && key < tau;
    eq[q] = i < m && key == tau;
  }
  uint32_t rank_eq[kPPT], rank[kPPT];
  tile_ranks(eq, s_eq, rank_eq);
  bool take[kPPT];
#pragma unroll
  for (int q = 0; q < kPPT; q++) take[q] = lt[q] || (eq[q] && base_eq + rank_eq[q] < quota);
  tile_ranks(take, s_take, rank);
  // the rows before this tile: every smaller key and the ties already taken
  const uint32_t row0 = base_lt + (base_eq < quota ? base_eq : quota);
#pragma unroll
  for (int q = 0; q < kPPT; q++) {
    const uint32_t i = start + t + kT * q, row = row0 + rank[q];
    if (take[q] && row < S)  // (row < S by the definition of tau and the quota)
      put_row(out0 + row, (int32_t)i, p + 3 * (uint64_t)i, lab ? lab[i] : 0, out_pts, out_labels, out_indices);
  }
}

__global__ void __launch_bounds__(kT) k_smp_gather(const float* __restrict__ pts, const int32_t* __restrict__ labels,
                                                   const int32_t* __restrict__ indices, uint32_t n, uint32_t S,
                                                   int32_t fill_label, float* __restrict__ out_pts,
                                                   int32_t* __restrict__ out_labels,
                                                   int32_t* __restrict__ out_counts) {
  __shared__ uint32_t s_cnt[kWaves];
  const uint32_t b = blockIdx.y, t = threadIdx.x;
  const uint32_t row = blockIdx.x * kT + t;
  const float* p = pts + (uint64_t)b * n * 3;
  const int32_t* idx = indices + (uint64_t)b * S;
  if (row < S) {
    const int32_t i = idx[row];
    const bool ok = i >= 0 && (uint32_t)i < n;
    put_row((uint64_t)b * S + row, 0, ok ? p + 3 * (uint64_t)i : p, ok && labels ? labels[(uint64_t)b * n + i] : fill_label,
            out_pts, out_labels, nullptr);
  }
  if (blockIdx.x != 0) return;
  uint32_t valid = 0;  // the first workgroup counts the cloud's valid rows
  for (uint32_t j = t; j < S; j += kT) {
    const int32_t i = idx[j];
    valid += i >= 0 && (uint32_t)i < n ? 1u : 0u;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) valid += __shfl_xor(valid, d, 64);
  if ((t & 63) == 0) s_cnt[t >> 6] = valid;
  __syncthreads();
  if (t == 0) {
    uint32_t sum = 0;
#pragma unroll
    for (int w = 0; w < kWaves; w++) sum += s_cnt[w];
    out_counts[b] = (int32_t)sum;
  }
}

// two byte ranges share a byte (a NULL range shares none)
bool overlap(const void* a, uint64_t na, const void* b, uint64_t nb) {
  if (!a || !b) return false;
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + nb && y < x + na;
}

// any of the `no` outputs shares a byte with an input or with another output
bool any_overlap(const void* const* out, const uint64_t* out_bytes, int no, const void* const* in,
                 const uint64_t* in_bytes, int ni) {
  for (int o = 0; o < no; o++) {
    for (int i = 0; i < ni; i++)
      if (overlap(out[o], out_bytes[o], in[i], in_bytes[i])) return true;
    for (int p = o + 1; p < no; p++)
      if (overlap(out[o], out_bytes[o], out[p], out_bytes[p])) return true;
  }
  return false;
}

}  // namespace

extern "C" {

size_t ndnet_sample_work_bytes(int B, uint64_t n) {
  if (B < 1 || n < 1 || n >= (1ull << 31)) return 0;
  return sizeof(SmpHead) + sizeof(uint32_t) * (keys_offset(B, (uint32_t)n) + (size_t)B * key_stride((uint32_t)n));
}

int ndnet_sample_random_run(const ndnet_sample_config* cfg, const float* d_points, const int32_t* d_labels,
                            const int32_t* d_counts, int B, uint64_t n, uint64_t S, int32_t fill_label, int advance,
                            uint64_t* d_step, void* d_work, float* d_out_points, int32_t* d_out_labels,
                            int32_t* d_out_counts, int32_t* d_out_indices, void* stream) {
  if (!cfg || !d_points || !d_step || !d_work || !d_out_points || !d_out_counts) return NDNET_ERR_ARG;
  if ((d_labels != nullptr) != (d_out_labels != nullptr)) return NDNET_ERR_ARG;
  if (B < 1 || B > 65535 || n < 1 || n >= (1ull << 31) || S < 1 || S > n) return NDNET_ERR_ARG;
  if (cfg->key_bits < 1 || cfg->key_bits > 32) return NDNET_ERR_ARG;
  {
    const uint64_t rows_in = (uint64_t)B * n, rows_out = (uint64_t)B * S;
    const void* const out[4] = {d_out_points, d_out_labels, d_out_counts, d_out_indices};
    const uint64_t out_bytes[4] = {12 * rows_out, 4 * rows_out, 4 * (uint64_t)B, 4 * rows_out};
    // (the scratch among the inputs: no output, and neither the counter nor an input, may lie in it)
    const void* const in[5] = {d_points, d_labels, d_counts, d_step, d_work};
    const uint64_t in_bytes[5] = {12 * rows_in, 4 * rows_in, 4 * (uint64_t)B, 8, ndnet_sample_work_bytes(B, n)};
    if (any_overlap(out, out_bytes, 4, in, in_bytes, 5)) return NDNET_ERR_ARG;
    if (any_overlap(&in[4], &in_bytes[4], 1, in, in_bytes, 4)) return NDNET_ERR_ARG;
  }

  hipStream_t st = (hipStream_t)stream;
  const uint32_t n32 = (uint32_t)n, S32 = (uint32_t)S;
  const dim3 grid(smp_tiles(n32), (uint32_t)B);
  k_smp_init<<<B, kT, 0, st>>>(B, advance, d_step, d_work);
  SMP_HIPCHK(hipGetLastError());
  if (S32 < n32) {  // (with S == n every cloud is taken whole)
    k_smp_keys<<<grid, kT, 0, st>>>(cfg->seed, cfg->stream, cfg->key_bits, d_counts, n32, S32, B, d_work);
    SMP_HIPCHK(hipGetLastError());
    k_smp_select<<<B, kSelT, 0, st>>>(cfg->key_bits, d_counts, n32, S32, B, d_work);
    SMP_HIPCHK(hipGetLastError());
    k_smp_count<<<grid, kT, 0, st>>>(d_counts, n32, S32, B, d_work);
    SMP_HIPCHK(hipGetLastError());
  }
  k_smp_apply<<<grid, kT, 0, st>>>(d_points, d_labels, d_counts, n32, S32, B, fill_label, d_work, d_out_points,
                                   d_out_labels, d_out_indices, d_out_counts);
  SMP_HIPCHK(hipGetLastError());
  return NDNET_OK;
}

int ndnet_sample_gather_run(const float* d_points, const int32_t* d_labels, const int32_t* d_indices, int B,
                            uint64_t n, uint64_t S, int32_t fill_label, float* d_out_points, int32_t* d_out_labels,
                            int32_t* d_out_counts, void* stream) {
  if (!d_points || !d_indices || !d_out_points || !d_out_counts) return NDNET_ERR_ARG;
  if ((d_labels != nullptr) != (d_out_labels != nullptr)) return NDNET_ERR_ARG;
  if (B < 1 || B > 65535 || n < 1 || n >= (1ull << 31) || S < 1 || S >= (1ull << 31)) return NDNET_ERR_ARG;
  {
    const uint64_t rows_in = (uint64_t)B * n, rows_out = (uint64_t)B * S;
    const void* const out[3] = {d_out_points, d_out_labels, d_out_counts};
    const uint64_t out_bytes[3] = {12 * rows_out, 4 * rows_out, 4 * (uint64_t)B};
    const void* const in[3] = {d_points, d_labels, d_indices};
    const uint64_t in_bytes[3] = {12 * rows_in, 4 * rows_in, 4 * rows_out};
    if (any_overlap(out, out_bytes, 3, in, in_bytes, 3)) return NDNET_ERR_ARG;
  }
  const uint32_t n32 = (uint32_t)n, S32 = (uint32_t)S;
  const dim3 grid((S32 + kT - 1) / kT, (uint32_t)B);
  k_smp_gather<<<grid, kT, 0, (hipStream_t)stream>>>(d_points, d_labels, d_indices, n32, S32, fill_label, d_out_points,
                                                     d_out_labels, d_out_counts);
  SMP_HIPCHK(hipGetLastError());
  return NDNET_OK;
}

}  // extern "C"
