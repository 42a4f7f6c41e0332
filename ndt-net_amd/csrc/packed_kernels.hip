// packed_kernels.hip -- packed int16 point input on gfx950
// (include/ndnet_packed.h): the decode at the head of the NDT stage.
//
//   k_pts_unpack_i16  a stream, 6 bytes in and 12 out per point.  Cloud b (grid
//                     y) is a flat run of 3 m elements (the axis of element e
//                     is e % 3), cut into a head of 0..7 elements that brings
//                     its q to a 16-byte boundary (thread 0), groups of eight
//                     -- one 16-byte load; two 16-byte stores where the
//                     output is 16-byte aligned there, eight 4-byte stores
//                     where not -- and a tail of < 8 elements (the thread
//                     after the last whole group).  The cut is per cloud, so
//                     no group spans two clouds whatever 6 n b is, and every
//                     branch but the tail's is uniform over the cloud.
//
// Built with -ffp-contract=off, and the decode is written __fmul_rn then
// __fadd_rn: the header defines it as two roundings, never an fma.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/ndnet_amd.h"
#include "../../include/ndnet_packed.h"

namespace {

#define PK_HIPCHK(x)                                                          \
  do {                                                                        \
    hipError_t e_ = (x);                                                      \
    if (e_ != hipSuccess) {                                                   \
      fprintf(stderr, "ndnet_amd: %s: %s\n", #x, hipGetErrorString(e_));      \
      return NDNET_ERR_HIP;                                                   \
    }                                                                         \
  } while (0)

constexpr int kPkThreads = 256;
constexpr int kPkWidth = 8;  // elements per thread: 16 bytes of q, 32 of output

typedef short pk_short8 __attribute__((ext_vector_type(8)));

__global__ void __launch_bounds__(kPkThreads) k_pts_unpack_i16(const int16_t* __restrict__ q_all,
                                                             const float* __restrict__ qparams, uint64_t n,
                                                             const int32_t* __restrict__ counts,
                                                             float* __restrict__ points) {
  const uint64_t b = blockIdx.y;
  uint64_t m = n;
  if (counts) {
    const int32_t c = counts[b];
    m = c < 0 ? 0 : ((uint64_t)c > n ? n : (uint64_t)c);
  }
  const uint64_t E = 3 * m;  // (n < 2^31: no overflow)
  const int16_t* q = q_all + 3 * n * b;
  float* out = points + 3 * n * b;
  const float o0 = qparams[4 * b], o1 = qparams[4 * b + 1], o2 = qparams[4 * b + 2], step = qparams[4 * b + 3];
  auto decode = [&](int16_t v, float o) -> float { return __fadd_rn(__fmul_rn((float)v, step), o); };
  uint64_t head = ((uint64_t)(0 - (uintptr_t)q) & 15) / sizeof(int16_t);
  if (head > E) head = E;
  const uint64_t t = (uint64_t)blockIdx.x * kPkThreads + threadIdx.x;
  // this thread's first element and the origins of its axis and the two after it
  // (selects on registers: an origin table indexed by e % 3 would live in scratch)
  const uint64_t e0 = t == 0 ? 0 : head + (t - 1) * kPkWidth;
  if (e0 >= E) return;
  const uint32_t axis = (uint32_t)(e0 % 3);
  float oa = axis == 0 ? o0 : (axis == 1 ? o1 : o2);
  float ob = axis == 0 ? o1 : (axis == 1 ? o2 : o0);
  float oc = axis == 0 ? o2 : (axis == 1 ? o0 : o1);
  const uint64_t e1 = t == 0 ? head : E;  // thread 0: the head; a thread short of a whole group: the tail
  if (t == 0 || e0 + kPkWidth > E) {
    for (uint64_t e = e0; e < e1; e++) {
      out[e] = decode(q[e], oa);
      const float r = oa;
      oa = ob, ob = oc, oc = r;
    }
    return;
  }
  const pk_short8 v = *reinterpret_cast<const pk_short8*>(q + e0);  // (q + head is 16-byte aligned, e0 - head a multiple of 8)
  const float x[kPkWidth] = {decode(v[0], oa), decode(v[1], ob), decode(v[2], oc), decode(v[3], oa),
                             decode(v[4], ob), decode(v[5], oc), decode(v[6], oa), decode(v[7], ob)};
  if ((((uintptr_t)(out + head)) & 15) == 0) {
    float4* o = reinterpret_cast<float4*>(out + e0);
    o[0] = make_float4(x[0], x[1], x[2], x[3]);
    o[1] = make_float4(x[4], x[5], x[6], x[7]);
  } else {
#pragma unroll
    for (int j = 0; j < kPkWidth; j++) out[e0 + j] = x[j];
  }
}

}  // namespace

extern "C" {

int ndnet_pts_unpack_i16(const int16_t* d_q, const float* d_qparams, int B, uint64_t n, const int32_t* d_counts,
                         float* d_points, void* stream) {
  if (!d_q || !d_qparams || !d_points || B < 1 || B > 65535 || n < 1 || n >= (1ull << 31)) return NDNET_ERR_ARG;
  // thread 0 of a cloud takes its head, the next ceil(3 n / 8) its groups and tail
  const uint64_t threads = 1 + (3 * n + kPkWidth - 1) / kPkWidth;
  const uint64_t blocks = (threads + kPkThreads - 1) / kPkThreads;  // (< 2^22)
  k_pts_unpack_i16<<<dim3((uint32_t)blocks, (uint32_t)B), kPkThreads, 0, (hipStream_t)stream>>>(d_q, d_qparams, n,
                                                                                               d_counts, d_points);
  PK_HIPCHK(hipGetLastError());
  return NDNET_OK;
}

}  // extern "C"
