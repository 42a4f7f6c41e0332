// ndt_block.h -- what every stage shares on the device: point loads, the wave
// and block scans with their Add* / Min* functors, and grid_from (the voxel
// grid of a voxel size, voxel.c:61-81).
//
// Included by ndt_kernels.hip inside its anonymous namespace, after
// ndt_plan.h (CloudCtl).
#pragma once

__device__ inline uint32_t hash32(uint32_t k) { return (k * 2654435761u) >> (32 - 11); }

template <typename T>
__device__ inline void load_point(const T* pts, uint64_t i, double* x) {
  x[0] = (double)pts[3 * i + 0];
  x[1] = (double)pts[3 * i + 1];
  x[2] = (double)pts[3 * i + 2];
}

// Inclusive wave scan (64 lanes) with op; returns inclusive value.
template <typename T, typename Op>
__device__ inline T wave_incl_scan(T x, Op op) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    T y = __shfl_up(x, o, 64);
    if (lane >= o) x = op(y, x);
  }
  return x;
}

// Exclusive block scan of one value per thread.  `scratch` holds >= 16 T.
template <typename T, typename Op>
__device__ inline T block_excl_scan(T v, T identity, Op op, T* scratch, T& total) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
  T incl = wave_incl_scan(v, op);
  T excl_w = __shfl_up(incl, 1, 64);
  if (lane == 0) excl_w = identity;
  if (lane == 63) scratch[wid] = incl;
  __syncthreads();
  if (wid == 0) {
    T s = lane < nw ? scratch[lane] : identity;
    s = wave_incl_scan(s, op);
    if (lane < nw) scratch[lane] = s;
  }
  __syncthreads();
  T pre = wid > 0 ? scratch[wid - 1] : identity;
  total = scratch[nw - 1];
  __syncthreads();
  return op(pre, excl_w);
}

// Exclusive block scan over ITEMS consecutive elements per thread (one
// barrier round for blockDim * ITEMS elements).  v[j] becomes the exclusive
// prefix of element j within the round; total is the round's reduction.
template <int ITEMS, typename T, typename Op>
__device__ inline void block_scan_items(T (&v)[ITEMS], T identity, Op op, T* scratch, T& total) {
  T local = identity;
#pragma unroll
  for (int j = 0; j < ITEMS; j++) {
    const T x = v[j];
    v[j] = local;
    local = op(local, x);
  }
  const T ex = block_excl_scan(local, identity, op, scratch, total);
#pragma unroll
  for (int j = 0; j < ITEMS; j++) v[j] = op(ex, v[j]);
}

struct AddU64 {
  __device__ unsigned long long operator()(unsigned long long a, unsigned long long b) const { return a + b; }
};

struct AddU32 {
  __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return a + b; }
};
struct MinF64 {
  __device__ double operator()(double a, double b) const { return b < a ? b : a; }
};

__device__ inline void grid_from(const CloudCtl& c, double vs, uint32_t* len, double* off, uint64_t* V) {
  // voxel.c:61-81: len = (int)ceil(dim / vs), offset = min
  uint64_t v = 1;
  for (int a = 0; a < 3; a++) {
    const double d = c.lim[a] - c.lim[3 + a];
    const double q = ceil(d / vs);
    int li;
    if (q >= -2147483648.0 && q < 2147483648.0) li = (int)q;
    else li = (int)0x80000000;  // x86 cvttsd2si overflow value
    len[a] = (uint32_t)li;
    off[a] = c.lim[3 + a];
    v *= (uint64_t)len[a];
  }
  *V = v;
}
