// pointnet_kernels.hip -- NDTNetSegmentation forward (eval) on gfx950.
//
// The reference runs NDTNet as a chain of torch Conv1d(k=1)/BatchNorm1d/ReLU
// ops (ndnet/models/ndtnet.py:45-60, 148-161, 233-241), each a GEMM over
// (points x channels) whose activations round-trip through HBM -- e.g. the
// TNet conv3 output is [B*N x 1024] fp32, 65 MB per batch, written and read
// back only to be max-pooled.  Here one workgroup carries a tile of 64 points
// through a whole per-point MLP chain: activations stay in LDS, each layer is
// an FP32 MFMA GEMM (v_mfma_f32_16x16x4_f32: exact fp32 products and sums, as
// torch's fp32 GEMM), BatchNorm is folded into the weights, and the chain
// ends either in a max-pool over points (fused into the last GEMM's
// epilogue: a column max over the tile, then one float atomic max per
// channel) or in log-softmax.
//
// Tile geometry: 64 points = four 16-row MFMA blocks per workgroup, 16 waves
// (4 per SIMD, so a wave waiting on its weight loads leaves three to keep the
// MFMA pipe busy).  A layer's waves split the tile as (row groups x column
// groups): for N a multiple of 256 each wave takes all four row blocks of one
// 16-column block (16 x 1), so every weight fragment is loaded once per
// workgroup; 2 x 8 for N = 128, 4 x 4 for N = 64 / 32.  Weights are stored
// fragment-major (include/ndnet_pointnet.h) and stream from L2 straight into
// registers, two k-groups ahead; the activations stay in LDS.  Barriers only
// separate layers (and the chunks of a fused pair).
// B=16 clouds x 1000 points is 256 tiles: one workgroup per CU, one round.
//
// A layer flagged fuse_next (the seg head's 64 -> 512) is produced 64 columns
// at a time into a small LDS buffer and consumed at once by the next layer
// (512 -> 256), whose accumulators persist across the chunks, so the 512-wide
// activation never needs LDS of its own.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../include/ndnet_pointnet.h"

namespace {

// Tile size: 64 points (16 waves), or 32 points (8 waves) in the second build
// of this file (-DNDNET_PN_TILE=32: pointnet_chain_t32.o, entry point
// ndnet_pn_chain_run_t32) for batches whose 64-point tiles would leave CUs
// idle (C5's 500-point level: 128 workgroups on 256 CUs).  Same wave-per-row-
// block ratios, so every layer split below has the same shape per wave.
#ifndef NDNET_PN_TILE
#define NDNET_PN_TILE 64
#endif
constexpr int kP = NDNET_PN_TILE;  // points per workgroup
#ifndef NDNET_PN_WAVES
#define NDNET_PN_WAVES (NDNET_PN_TILE / 4)
#endif
constexpr int kWaves = NDNET_PN_WAVES;
constexpr int kThreads = 64 * kWaves;
constexpr int kRowBlocks = kP / 16;  // 4 (2 for 32-point tiles)
static_assert(kP == 64 || kP == 32, "64- or 32-point tiles");
constexpr int kFuseNC = 64;     // columns per chunk of a fused layer
// LDS row pitch padding.  An A-fragment read (ds_read_b128, 16 B per lane at
// row l & 15, column offset 16 B * (l >> 4)) is conflict-free when the row
// pitch is 32 B mod 256 B (two 4-bank slots per row: the 16 lanes of each
// ds_read_b128 lane group land on 16 distinct slots); a pitch of 16 B mod
// 256 B (one slot per row) puts two lanes of every group on one slot and
// doubles the read.  Activation widths are multiples of 64 (or 16 / 32 / 64
// for the input tile), so width + kPadF floats / width + kPadB bf16 give it.
constexpr int kPadF = 8;        // fp32 regions: pitch = width + 8 floats
constexpr int kPadB = 16;       // bf16 planes: pitch = width + 16 bf16
// bf16 planes, round 6: the epilogues store a lane's 4 channels of one point
// as one ds_write_b64 per plane, and a write's 16-lane group (one kq, points
// cl = 0..15) lands on 16 rows of the same columns.  Writes bank on (a/4) mod
// 32 (MI355X_MICROARCH.md §LDS): with these pitches (32 B + a multiple of
// 128 B: 8 dwords mod 32) rows r and r + 4 share banks -- 4-way, the chain
// D conflicts (25.7% of its LDS cycles, profiles/r05_pmc_summary.txt).  So the
// 16-byte slots of row r are XOR-swizzled by bit 2 of r (slot s at s ^
// ((r >> 2) & 1)): the writes become 2-way, the least 16 rows x 8 bytes at
// 16-byte granularity allow (8 distinct slots mod 128 B), and the
// ds_read_b128 A-fragment reads stay conflict-free (every lane group on 16
// distinct 16-byte slots; checked exhaustively for the pitches used).  A read
// keeps its 16 bytes whole: only which slot of its row it reads moves.
#ifndef NDNET_PN_PLANE_SWZ
#define NDNET_PN_PLANE_SWZ 1
#endif
// the bf16 column where element (row, col) of a plane is stored (bit 3 of the
// column, slot bit 0, flipped on rows 4..7 mod 8)
__device__ inline int plane_col(int row, int col) {
  return NDNET_PN_PLANE_SWZ ? col ^ (((row >> 2) & 1) << 3) : col;
}
#ifndef NDNET_PN_DEPTH
#define NDNET_PN_DEPTH 2
#endif
constexpr int kDepth = NDNET_PN_DEPTH;  // weight k-groups in flight per wave
#ifndef NDNET_PN_DEPTH6
#define NDNET_PN_DEPTH6 1
#endif
constexpr int kDepth6 = NDNET_PN_DEPTH6;  // the same for split-bf16 layers (3 fragment planes each)
// chain D's fused pair computes chunk f + 1's P before chunk f's Q (same
// products, same order): 43.4 -> 42.9 us per chain D (gpurun_out/r05w_v)
#ifndef NDNET_PN_PAIR_PFIRST
#define NDNET_PN_PAIR_PFIRST 1
#endif
#ifndef NDNET_PN_CHUNK_ROT
#define NDNET_PN_CHUNK_ROT 1
#endif
constexpr bool kChunkRot = NDNET_PN_CHUNK_ROT;  // per-workgroup chunk order (run_tiles_x6 rot)
static_assert(kWaves % kRowBlocks == 0, "every row group has whole column groups");

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

__device__ inline void atomic_max_f32(float* addr, float v) {
  v = v + 0.0f;  // -0 -> +0 so the integer orderings below agree
  if (v >= 0.0f) atomicMax(reinterpret_cast<int*>(addr), __float_as_int(v));
  else atomicMin(reinterpret_cast<unsigned int*>(addr), __float_as_uint(v));
}

// Output orientation of the MFMA tiles.  With the weights as the A operand
// and the activations as B (NDNET_PN_SWAP = 1, default) a 16 x 16 tile comes
// out transposed: lane (kq, cl) holds point cl, channels 4 kq .. 4 kq + 3 --
// four consecutive channels of one point, which the epilogue stores as one
// ds_write_b128 (fp32) or one ds_write_b64 per bf16 plane instead of 4 / 12
// scalar stores, and max-pools over the 16 points of a lane row with DPP.
// The operands' lane data are the same either way (the fragment layouts are
// symmetric), so only the MFMA argument order and the epilogues change.
// NDNET_PN_SWAP = 0: activations as A, lane (kq, cl) holds points 4 kq + r of
// channel cl.
#ifndef NDNET_PN_SWAP
#define NDNET_PN_SWAP 1
#endif

// v of lane (lane ^ S) within a 16-lane row, through DPP (no LDS)
template <int S>
__device__ inline float xor_row(float v) {
  const int x = __float_as_int(v);
  if constexpr (S == 1) {
    return __int_as_float(__builtin_amdgcn_mov_dpp(x, 0xB1, 0xF, 0xF, false));  // quad_perm [1,0,3,2]
  } else if constexpr (S == 2) {
    return __int_as_float(__builtin_amdgcn_mov_dpp(x, 0x4E, 0xF, 0xF, false));  // quad_perm [2,3,0,1]
  } else if constexpr (S == 4) {
    const int h = __builtin_amdgcn_mov_dpp(x, 0x141, 0xF, 0xF, false);          // row_half_mirror: i ^ 7
    return __int_as_float(__builtin_amdgcn_mov_dpp(h, 0x1B, 0xF, 0xF, false));  // quad_perm [3,2,1,0]: ^ 3
  } else {
    const int h = __builtin_amdgcn_mov_dpp(x, 0x140, 0xF, 0xF, false);           // row_mirror: i ^ 15
    return __int_as_float(__builtin_amdgcn_mov_dpp(h, 0x141, 0xF, 0xF, false));  // row_half_mirror: ^ 7
  }
}

// dynamic LDS of k_pn_chain: the two activation regions and the fused pair's
// double buffer, addressed by float offsets so every access is a ds_* op
extern __shared__ __attribute__((aligned(16))) float g_smem[];
#ifndef NDNET_PN_TID_FRESH
#define NDNET_PN_TID_FRESH 1
#endif
// threadIdx.x as a value the compiler cannot see through: a layer's lane /
// wave / row / column offsets are derived from it where the layer runs
// instead of being hoisted to the kernel's start and kept live through every
// layer (they took ~48 of the 128 VGPRs the 16-wave build has, so the x6
// loops could neither keep a plane's four A fragments nor the next weight
// step in registers)
__device__ inline int pn_tid() {
  int t = (int)threadIdx.x;
#if NDNET_PN_TID_FRESH
  asm volatile("" : "+v"(t));
#endif
  return t;
}


// Timing build only (-DNDNET_PN_STAMPS, tools/pn_stamps.py): s_memrealtime
// (100 MHz) of every workgroup at its start (0), after chain B's head
// prologue or chain C's t2 fold (1), after the input tile (2), after each layer's closing barrier
// (3 + layer) and at its end (15), read back by ndnet_pn_debug_stamps.  The
// product build compiles none of it.
#ifdef NDNET_PN_STAMPS
constexpr int kStampWgs = 1024;
__device__ unsigned long long g_pn_stamps[kStampWgs][16];
#define PN_STAMP(i)                                                                           \
  do {                                                                                        \
    const int w_ = blockIdx.y * gridDim.x + blockIdx.x;                                       \
    if (threadIdx.x == 0 && w_ < kStampWgs) g_pn_stamps[w_][(i)] = __builtin_amdgcn_s_memrealtime(); \
  } while (0)
#else
#define PN_STAMP(i) \
  do {              \
  } while (0)
#endif

// Weights are fragment-major (include/ndnet_pointnet.h): the 16 x 16 block
// (k-group kg, column block cb) of W^T is 64 lanes x float4, lane kq * 16 + cl
// holding W^T[16 kg + 4 kq + s][16 cb + cl] for s = 0..3 -- the B operands of
// four consecutive 16x16x4 MFMAs, one coalesced 1 KB global_load_dwordx4 per
// wave.  The A operand uses the same K permutation: lane (kq, cl) reads
// activation row cl, columns 16 kg + 4 kq .. + 3 with one ds_read_b128.  So
// the weights stream from L2 straight into registers (no LDS staging, no
// barrier inside a layer) and only the activations live in LDS.
struct LayerCtx {
  const f32x4* __restrict__ w;     // this cloud's fragments, offset by the lane (prec 0)
  const bf16x8* __restrict__ w6;   // split-bf16 fragments, offset by the lane (prec 1..3)
  const float* __restrict__ bias;
  int KG, N, relu, prec;           // KG: 16-row k-groups (prec 0) or 32-row (prec 1..3)
  float sc;                        // the fp16 form (T = 2): what undoes the operands' scales, 2^-4 2^-s (1 for prec 0)
};

// bias: the layer's (this cloud's) bias, staged in LDS by the kernel's prologue
// The first weight step of a layer, loaded by each wave before the barrier
// that closes the previous layer (its latency hides behind the barrier wait;
// 16-wave 64-point build, where every layer's wave tile is one column block):
// r0..r2 = the bf16x8 planes the mode reads for prec 1..3, r0 for prec 0.
struct Pre {
  bool on;
  f32x4 r0, r1, r2;  // prec 1..3: bf16x8 planes h, m, l (bit_cast); prec 0: r0
};

template <int T>
__device__ inline LayerCtx layer_ctx(const ndnet_pn_chain& A, const ndnet_pn_f16* X, int l, int b, const float* bias) {
  const ndnet_pn_layer& L = A.L[l];
  LayerCtx C;
  C.w = reinterpret_cast<const f32x4*>(L.w + (int64_t)b * L.w_cloud_stride) + (pn_tid() & 63);
  C.w6 = reinterpret_cast<const bf16x8*>(L.w + (int64_t)b * L.w_cloud_stride) + (pn_tid() & 63);
  C.sc = 1.0f;
  if constexpr (T == 2) {  // the fp16 planes (shared weights: no per-cloud copies) and the layer's scale
    if (L.prec) {
      C.w6 = reinterpret_cast<const bf16x8*>(X->w16[l]) + (pn_tid() & 63);
      C.sc = 0.0625f * *X->scale[l];
    }
  }
  C.bias = bias;
  C.prec = L.prec;
  C.KG = L.prec ? L.K / 32 : L.K / 16;  // split-bf16: 32-row k-groups
  C.N = L.N;
  C.relu = L.relu;
  return C;
}

template <int RB, int NB>
__device__ __attribute__((always_inline)) inline void zero_acc(f32x4 (&acc)[RB][NB]) {
#pragma unroll
  for (int rb = 0; rb < RB; rb++)
#pragma unroll
    for (int j = 0; j < NB; j++) acc[rb][j] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// acc[rb][j] += A(row block rb, one k-group) . W(k-group, column block j)
template <int RB, int NB>
__device__ __attribute__((always_inline)) inline void mma_kgroup(f32x4 (&acc)[RB][NB], const f32x4 (&a)[RB],
                                                                 const f32x4 (&bw)[NB]) {
#pragma unroll
  for (int s = 0; s < 4; s++)
#pragma unroll
    for (int rb = 0; rb < RB; rb++)
#pragma unroll
      for (int j = 0; j < NB; j++)
#if NDNET_PN_SWAP
        acc[rb][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(bw[j][s], a[rb][s], acc[rb][j], 0, 0, 0);
#else
        acc[rb][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[rb][s], bw[j][s], acc[rb][j], 0, 0, 0);
#endif
}

// T = nchunk * nkg k-group steps.  Step t is k-group kg0 + t % nkg of column
// chunk c = t / nkg, whose column blocks for this wave are cb0 + c * cbs + j;
// its A fragment sits at abase + 16 (t % nkg) (+ 16 rb rows).  epi(acc, c)
// runs at each chunk end.  The weight fragments are prefetched kDepth steps
// ahead in a ring of register sets; past the last step the loads repeat it.
template <int RB, int NB, class Epi>
__device__ __attribute__((always_inline)) inline void run_tiles(f32x4 (&acc)[RB][NB], const f32x4* __restrict__ w,
                                                                int KG, int kg0, int nkg, int cb0, int cbs,
                                                                int nchunk, const float* abase, int pin, Epi epi,
                                                                Pre pre = {}) {
  const int T = nchunk * nkg;
  const int64_t jstride = (int64_t)KG * 64;
  const int64_t chunk_jump = ((int64_t)cbs * KG - (nkg - 1)) * 64;
  const f32x4* lp = w + ((int64_t)cb0 * KG + kg0) * 64;  // the next load's step
  int lkk = 0, lleft = T;
  auto advance = [&]() {
    if (lleft > 1) {
      lleft--;
      if (++lkk == nkg) {
        lkk = 0;
        lp += chunk_jump;
      } else {
        lp += 64;
      }
    }
  };
  auto load = [&](f32x4 (&bw)[NB]) {
#pragma unroll
    for (int j = 0; j < NB; j++) bw[j] = lp[j * jstride];
    advance();
  };
  // A fragments are software-pipelined one step ahead too (the A region is
  // read-only during the layer, so the prefetch may run into the next chunk)
  int kk = 0, c = 0, akk = 0;
  f32x4 a[RB];
  auto load_a = [&]() {
#pragma unroll
    for (int rb = 0; rb < RB; rb++) a[rb] = *reinterpret_cast<const f32x4*>(abase + rb * 16 * pin + 16 * akk);
    akk = akk + 1 == nkg ? 0 : akk + 1;
  };
  auto step = [&](const f32x4 (&bw)[NB]) {
    f32x4 cur[RB];
#pragma unroll
    for (int rb = 0; rb < RB; rb++) cur[rb] = a[rb];
    load_a();
    mma_kgroup<RB, NB>(acc, cur, bw);
    if (++kk == nkg) {
      epi(acc, c);
      kk = 0;
      c++;
    }
  };
  load_a();
  f32x4 bq[kDepth][NB];
#pragma unroll
  for (int i = 0; i < kDepth; i++) {
    if (NB == 1 && i == 0 && pre.on) {  // the first step, prefetched by the caller
      bq[0][0] = pre.r0;
      advance();
    } else {
      load(bq[i]);
    }
  }
  for (int t = 0; t < T; t += kDepth) {
#pragma unroll
    for (int i = 0; i < kDepth; i++) {
      if (t + i < T) {
        step(bq[i]);
        load(bq[i]);
      }
    }
  }
}

// Bias + ReLU of this wave's tile (rows row0.., bias columns col0 + 16 j + cl)
// into an LDS activation region at columns oc0 + 16 j + cl.
// T = 2 (the fp16 form): the accumulators carry the operands' scales, undone by sc in the bias add.
template <int RB, int NB, int T = 6>
__device__ __attribute__((always_inline)) inline void store_cols(const f32x4 (&acc)[RB][NB],
                                                                 const float* __restrict__ bias, int col0, int relu,
                                                                 int row0, int out, int pout, int oc0, float sc = 1.0f) {
  static_assert(T != 2 || NDNET_PN_SWAP, "the fp16 form is written for the swapped orientation");
  const int lane = pn_tid() & 63;
  const int kq = lane >> 4, cl = lane & 15;
#if NDNET_PN_SWAP
#pragma unroll
  for (int j = 0; j < NB; j++) {
    float bv[4];
#pragma unroll
    for (int r = 0; r < 4; r++) bv[r] = bias[col0 + 16 * j + 4 * kq + r];
#pragma unroll
    for (int rb = 0; rb < RB; rb++) {
      f32x4 v;
#pragma unroll
      for (int r = 0; r < 4; r++) {
        if constexpr (T == 2) v[r] = fmaf(acc[rb][j][r], sc, bv[r]);
        else v[r] = acc[rb][j][r] + bv[r];
        if (relu) v[r] = fmaxf(v[r], 0.0f);
      }
      *reinterpret_cast<f32x4*>(g_smem + out + (row0 + 16 * rb + cl) * pout + oc0 + 16 * j + 4 * kq) = v;
    }
  }
#else
#pragma unroll
  for (int j = 0; j < NB; j++) {
    const float bv = bias[col0 + 16 * j + cl];
#pragma unroll
    for (int rb = 0; rb < RB; rb++)
#pragma unroll
      for (int r = 0; r < 4; r++) {
        float v = acc[rb][j][r] + bv;
        if (relu) v = fmaxf(v, 0.0f);
        g_smem[out + (row0 + 16 * rb + 4 * kq + r) * pout + oc0 + 16 * j + cl] = v;
      }
  }
#endif
}

// Bias + ReLU + max over this wave's valid rows, one float atomic max per
// column and wave into gmax (the workgroup's row groups meet in the atomics).
// T = 2: the maximum is taken over the scaled accumulators and sc (a positive power of two) undone in
// the bias add -- fma(a, sc, b) is monotonic in a too.
template <int RB, int NB, int T = 6>
__device__ __attribute__((always_inline)) inline void pool_cols(const f32x4 (&acc)[RB][NB],
                                                                const float* __restrict__ bias, int col0, int relu,
                                                                int row0, int rows_valid, float* gmax, float sc = 1.0f) {
  const int lane = pn_tid() & 63;
  const int kq = lane >> 4, cl = lane & 15;
#if NDNET_PN_SWAP
  // lane (kq, cl): point cl of each row block, channels 4 kq + r; the max over
  // the tile's valid points first (RB values in the lane, then the 16 lanes of
  // a lane row by DPP), then bias + ReLU once on the maximum -- exact, as
  // fl(a + b) and ReLU are monotonic in a -- and lane cl < 4 of the row takes
  // channel 4 kq + cl's atomic
  const bool full = row0 + 16 * RB <= rows_valid;  // wave-uniform: every row of the wave's tile is a point
#pragma unroll
  for (int j = 0; j < NB; j++) {
    float m[4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
      if (full) {
        m[r] = acc[0][j][r];
#pragma unroll
        for (int rb = 1; rb < RB; rb++) m[r] = fmaxf(m[r], acc[rb][j][r]);
      } else {
        m[r] = -INFINITY;
#pragma unroll
        for (int rb = 0; rb < RB; rb++)
          if (row0 + 16 * rb + cl < rows_valid) m[r] = fmaxf(m[r], acc[rb][j][r]);
      }
      m[r] = fmaxf(m[r], xor_row<1>(m[r]));
      m[r] = fmaxf(m[r], xor_row<2>(m[r]));
      m[r] = fmaxf(m[r], xor_row<4>(m[r]));
      m[r] = fmaxf(m[r], xor_row<8>(m[r]));
    }
    const float mm = cl == 0 ? m[0] : cl == 1 ? m[1] : cl == 2 ? m[2] : m[3];
    if (cl < 4 && mm > -INFINITY) {
      float v;
      if constexpr (T == 2) v = fmaf(mm, sc, bias[col0 + 16 * j + 4 * kq + cl]);
      else v = mm + bias[col0 + 16 * j + 4 * kq + cl];
      if (relu) v = fmaxf(v, 0.0f);
      atomic_max_f32(gmax + col0 + 16 * j + 4 * kq + cl, v);
    }
  }
#else
#pragma unroll
  for (int j = 0; j < NB; j++) {
    const float bv = bias[col0 + 16 * j + cl];
    float m = -INFINITY;
#pragma unroll
    for (int rb = 0; rb < RB; rb++)
#pragma unroll
      for (int r = 0; r < 4; r++) {
        float v = acc[rb][j][r] + bv;
        if (relu) v = fmaxf(v, 0.0f);
        if (row0 + 16 * rb + 4 * kq + r < rows_valid) m = fmaxf(m, v);
      }
    m = fmaxf(m, __shfl_xor(m, 16, 64));
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    if (lane < 16 && m > -INFINITY) atomic_max_f32(gmax + col0 + 16 * j + cl, m);
  }
#endif
}

// ---------------------------------------------------------------------------
// Split-bf16 layers (ndnet_pn_layer.prec = 1): fp32-accurate GEMMs on the
// bf16 matrix cores.  Every operand x is split x = h + m + l into three bf16
// (8 + 8 + 8 significant bits = fp32's 24; h = bf16(x), m = bf16(x - h),
// l = bf16(x - h - m), each residual exact in fp32).  A product keeps the six
// terms of weight >= 2^-16 (mm, mh, lh, hl, hm, hh in that order) -- each
// an exact bf16 x bf16 product accumulated in fp32 by v_mfma_f32_16x16x32_bf16;
// the dropped ml, lm, ll are below 3 * 2^-24 |x y|, the size of fp32's own
// rounding.  Six 16-cycle MFMAs per 16x16x32 block against eight 32-cycle
// v_mfma_f32_16x16x4_f32 for the same FLOPs: 2.7x less matrix-core time.
//
// The layer's input activations are stored by the producing layer's epilogue
// as three bf16 planes of the LDS region (plane p at p * kP * pitch, element
// (row, k) at row * pitch + k, pitch = width + kPadB bf16); lane l of a 16x16x32
// A fragment reads row l & 15, k = 32 kg + 8 (l >> 4) .. + 7 with one
// ds_read_b128 per plane.  The weights are fragment-major per 32-row k-group:
// [column block][k-group][plane][lane][8 bf16], lane l holding
// W^T[32 kg + 8 (l >> 4) + j][16 cb + (l & 15)] (include/ndnet_pointnet.h).

__device__ inline void split3(float v, __bf16& h, __bf16& m, __bf16& l) {
  h = (__bf16)v;
  const float r = v - (float)h;
  m = (__bf16)r;
  l = (__bf16)(r - (float)m);
}

// The reduced modes (ndnet_pn_layer.prec 2 / 3) keep fewer of those products,
// on the same planes and the same weight layout.  T is the number of terms,
// a compile-time parameter of everything below and of the whole kernel (all
// split layers of a chain share one mode, so T = 6 compiles to the code it
// was before the modes existed):
//   T = 6 (prec 1)  mm, mh, lh, hl, hm, hh   planes h, m, l
//   T = 3 (prec 2)  mh, hm, hh               planes h, m: 16 significant bits
//                   per operand, dropped terms <= 3.02 * 2^-18 |x y|
//   T = 1 (prec 3)  hh                       plane h: plain bf16 operands,
//                   dropped terms <= (2^-8 + 2^-18) |x y|
// A plane a mode does not read is neither computed, stored, loaded from LDS
// or global memory, nor prefetched; the LDS layout (plane p at p * kP * pitch)
// and the weight layout (three planes per k-group) are the same in all modes.
//
// T = 2 is the fp16 two-slice form of the same layers (ndnet_pn_f16, include/ndnet_pointnet.h): operands
// x = h + l in two fp16 (11 + 11 significant bits and the residual's sign), three products l*h, h*l, h*h
// on v_mfma_f32_16x16x32_f16 -- T = 3's instruction shape with T = 6's accuracy class.  fp16's 5 exponent
// bits make it conditional: activations are stored as split(16 v), weights as split(w 2^s) (two planes
// per k-group, a layout of their own), the epilogue undoes both scales, and a tile whose activations
// leave the window runs T = 6 instead (k_pn_chain_f16).  The planes are moved as bf16x8 / bf16x4 bit
// patterns; only the conversions and the MFMA know the element type.
template <int T>
constexpr int kPlanes = T == 6 ? 3 : T == 1 ? 1 : 2;
// planes stored per k-group of the weights a mode reads
template <int T>
constexpr int kWPlanes = T == 2 ? 2 : 3;

// the row maximum of a lane row of 16 (DPP), on bit patterns: NaN and infinity order above every finite |v|
__device__ inline unsigned umax_row16(unsigned x) {
  int v = (int)x;
  v = max(v, __builtin_amdgcn_mov_dpp(v, 0xB1, 0xF, 0xF, false));   // quad_perm [1,0,3,2]
  v = max(v, __builtin_amdgcn_mov_dpp(v, 0x4E, 0xF, 0xF, false));   // quad_perm [2,3,0,1]
  v = max(v, __builtin_amdgcn_mov_dpp(v, 0x141, 0xF, 0xF, false));  // row_half_mirror
  v = max(v, __builtin_amdgcn_mov_dpp(v, 0x140, 0xF, 0xF, false));  // row_mirror
  return (unsigned)v;
}

// T = 2: |v|'s bits (sign cleared, so they order as the values do) of everything a lane stored into a
// split layer's input, folded into that tensor's window word: one LDS max per lane row
__device__ inline void window_note(int flag, unsigned mx) {
  mx = umax_row16(mx);
  if ((pn_tid() & 15) == 0) atomicMax(reinterpret_cast<unsigned*>(g_smem) + flag, mx);
}

// split(16 v) into two fp16, both conversions to nearest even (v_cvt_f16_f32)
__device__ inline void split_f16(float v, _Float16& h, _Float16& l) {
  const float s = 16.0f * v;
  h = (_Float16)s;
  l = (_Float16)(s - (float)h);
}

// v's first kPlanes<T> bf16 planes (l, or m and l, left alone when unused)
template <int T>
__device__ inline void split_t(float v, __bf16& h, __bf16& m, __bf16& l) {
  static_assert(T == 6 || T == 3 || T == 2 || T == 1, "6, 3 or 1 terms (2: the fp16 form, which has split_f16)");
  if constexpr (T == 2) {
    __builtin_unreachable();  // its callers return before they get here
  } else if constexpr (T == 6) {
    split3(v, h, m, l);
  } else if constexpr (T == 3) {
    h = (__bf16)v;
    m = (__bf16)(v - (float)h);
  } else {
    h = (__bf16)v;
  }
}

// Bias + ReLU of this wave's tile into the bf16 planes of a region that the
// consumer's mode reads (`out` in floats; pitch in bf16).
template <int RB, int NB, int T>
__device__ __attribute__((always_inline)) inline void store_cols_planes(const f32x4 (&acc)[RB][NB],
                                                                        const float* __restrict__ bias, int col0,
                                                                        int relu, int row0, int out, int pitchb,
                                                                        int oc0, float sc = 1.0f, int flag = 0) {
  const int lane = pn_tid() & 63;
  const int kq = lane >> 4, cl = lane & 15;
  __bf16* const base = reinterpret_cast<__bf16*>(g_smem + out);
  const int plane = kP * pitchb;
#if NDNET_PN_SWAP
  typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
  if constexpr (T == 2) {  // two fp16 planes of split(16 v), v = fma(acc, sc, bias); the window word takes max |v|
    unsigned mx = 0;
#pragma unroll
    for (int j = 0; j < NB; j++) {
      float bv[4];
#pragma unroll
      for (int r = 0; r < 4; r++) bv[r] = bias[col0 + 16 * j + 4 * kq + r];
#pragma unroll
      for (int rb = 0; rb < RB; rb++) {
        f16x4 h4, l4;
#pragma unroll
        for (int r = 0; r < 4; r++) {
          float v = fmaf(acc[rb][j][r], sc, bv[r]);
          if (relu) v = fmaxf(v, 0.0f);
          mx = max(mx, __float_as_uint(v) & 0x7fffffffu);
          _Float16 h, l;
          split_f16(v, h, l);
          h4[r] = h;
          l4[r] = l;
        }
        const int row = row0 + 16 * rb + cl;
        const int e = row * pitchb + plane_col(row, oc0 + 16 * j + 4 * kq);
        *reinterpret_cast<f16x4*>(base + e) = h4;
        *reinterpret_cast<f16x4*>(base + plane + e) = l4;
      }
    }
    window_note(flag, mx);
    return;
  }
#pragma unroll
  for (int j = 0; j < NB; j++) {
    float bv[4];
#pragma unroll
    for (int r = 0; r < 4; r++) bv[r] = bias[col0 + 16 * j + 4 * kq + r];
#pragma unroll
    for (int rb = 0; rb < RB; rb++) {
      bf16x4 h4, m4, l4;
#pragma unroll
      for (int r = 0; r < 4; r++) {
        float v = acc[rb][j][r] + bv[r];
        if (relu) v = fmaxf(v, 0.0f);
        __bf16 h, m, l;
        split_t<T>(v, h, m, l);
        h4[r] = h;
        if constexpr (T >= 3) m4[r] = m;
        if constexpr (T == 6) l4[r] = l;
      }
      const int row = row0 + 16 * rb + cl;
      const int e = row * pitchb + plane_col(row, oc0 + 16 * j + 4 * kq);  // 4 channels: 8 bytes
      *reinterpret_cast<bf16x4*>(base + e) = h4;
      if constexpr (T >= 3) *reinterpret_cast<bf16x4*>(base + plane + e) = m4;
      if constexpr (T == 6) *reinterpret_cast<bf16x4*>(base + 2 * plane + e) = l4;
    }
  }
#else
#pragma unroll
  for (int j = 0; j < NB; j++) {
    const float bv = bias[col0 + 16 * j + cl];
#pragma unroll
    for (int rb = 0; rb < RB; rb++)
#pragma unroll
      for (int r = 0; r < 4; r++) {
        float v = acc[rb][j][r] + bv;
        if (relu) v = fmaxf(v, 0.0f);
        __bf16 h, m, l;
        split_t<T>(v, h, m, l);
        const int row = row0 + 16 * rb + 4 * kq + r;
        const int e = row * pitchb + plane_col(row, oc0 + 16 * j + cl);
        base[e] = h;
        if constexpr (T >= 3) base[plane + e] = m;
        if constexpr (T == 6) base[2 * plane + e] = l;
      }
  }
#endif
}

// One 32-row k-group: the A planes are read one at a time (m, l, h) so only
// one plane's fragments are live; per plane the B planes its terms need.
// T terms, smallest first: 6 as listed above, 3 = m*h, h*m, h*h, 1 = h*h.
template <int RB, int NB, int T>
__device__ __attribute__((always_inline)) inline void mma_kgroup_x6(f32x4 (&acc)[RB][NB], const __bf16* a0, int plane,
                                                                    int rstride, const bf16x8 (&bw)[NB][kPlanes<T>]) {
  bf16x8 a[RB];
  auto ld = [&](int p) {
#pragma unroll
    for (int rb = 0; rb < RB; rb++) a[rb] = *reinterpret_cast<const bf16x8*>(a0 + p * plane + rb * rstride);
  };
  auto mm = [&](int pb) {
#pragma unroll
    for (int rb = 0; rb < RB; rb++)
#pragma unroll
      for (int j = 0; j < NB; j++)
#if NDNET_PN_SWAP
        if constexpr (T == 2)
          acc[rb][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, bw[j][pb]),
                                                              __builtin_bit_cast(f16x8, a[rb]), acc[rb][j], 0, 0, 0);
        else
          acc[rb][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bw[j][pb], a[rb], acc[rb][j], 0, 0, 0);
#else
        acc[rb][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[rb], bw[j][pb], acc[rb][j], 0, 0, 0);
#endif
  };
  if constexpr (T == 6) {
    ld(1);  // m: m*m, m*h
    mm(1);
    mm(0);
    ld(2);  // l: l*h
    mm(0);
    ld(0);  // h: h*l, h*m, h*h
    mm(2);
    mm(1);
    mm(0);
  } else if constexpr (T == 3 || T == 2) {
    ld(1);  // m: m*h  (T = 2: the fp16 l plane, l*h)
    mm(0);
    ld(0);  // h: h*m, h*h
    mm(1);
    mm(0);
  } else {
    ld(0);  // h: h*h
    mm(0);
  }
}

// run_tiles for split-bf16 layers: 32-row k-groups; A from the mode's planes
// (abase: this lane's row / k offset in plane 0, in bf16), B the mode's 1 KB
// fragment pieces (of the three stored) per column block, prefetched kDepth6
// steps ahead.
template <int T, int RB, int NB, class Epi, int kD = kDepth6>
__device__ __attribute__((always_inline)) inline void run_tiles_x6(f32x4 (&acc)[RB][NB],
                                                                   const bf16x8* __restrict__ w, int KG, int kg0,
                                                                   int nkg, int cb0, int cbs, int nchunk,
                                                                   const __bf16* abase, int pitchb, Epi epi,
                                                                   Pre pre = {}, int rot = 0) {
  // rot: the chunks run in the order rot, rot + 1, .. (mod nchunk), so that
  // workgroups in lockstep do not all stream the same weight fragments at
  // once (different chunks hit different L2 lines); each chunk's columns and
  // sums are unchanged
  const int NT = nchunk * nkg;  // k-group steps
  const int plane = kP * pitchb;
  constexpr int WPL = kWPlanes<T>;  // planes stored per k-group (3; the fp16 form's 2)
  const int64_t jstride = (int64_t)KG * WPL * 64;
  const int64_t chunk_jump = ((int64_t)cbs * KG - (nkg - 1)) * WPL * 64;
  const int64_t wrap = (int64_t)nchunk * cbs * KG * WPL * 64;
  const bf16x8* lp = w + ((int64_t)(cb0 + rot * cbs) * KG + kg0) * WPL * 64;
  int lkk = 0, lleft = NT, lc = rot;
  auto advance = [&]() {
    if (lleft > 1) {
      lleft--;
      if (++lkk == nkg) {
        lkk = 0;
        lp += chunk_jump;
        if (++lc == nchunk) {
          lc = 0;
          lp -= wrap;
        }
      } else {
        lp += WPL * 64;
      }
    }
  };
  constexpr int NPL = kPlanes<T>;
  auto load = [&](bf16x8 (&bw)[NB][NPL]) {
#pragma unroll
    for (int j = 0; j < NB; j++)
#pragma unroll
      for (int p = 0; p < NPL; p++) bw[j][p] = lp[j * jstride + p * 64];
    advance();
  };
  int kk = 0, c = rot;
  auto step = [&](const bf16x8 (&bw)[NB][NPL]) {
    mma_kgroup_x6<RB, NB, T>(acc, abase + 32 * kk, plane, 16 * pitchb, bw);
    if (++kk == nkg) {
      epi(acc, c);
      kk = 0;
      if (++c == nchunk) c = 0;
    }
  };
  bf16x8 bq[kD][NB][NPL];
#pragma unroll
  for (int i = 0; i < kD; i++) {
    if (NB == 1 && i == 0 && pre.on) {  // the first step, prefetched by the caller
      bq[0][0][0] = __builtin_bit_cast(bf16x8, pre.r0);
      if constexpr (NPL >= 2) bq[0][0][1] = __builtin_bit_cast(bf16x8, pre.r1);
      if constexpr (NPL == 3) bq[0][0][2] = __builtin_bit_cast(bf16x8, pre.r2);
      advance();
    } else {
      load(bq[i]);
    }
  }
  for (int t = 0; t < NT; t += kD) {
#pragma unroll
    for (int i = 0; i < kD; i++) {
      if (t + i < NT) {
        step(bq[i]);
        if (t + i + kD < NT) load(bq[i]);  // no reload past the last step
      }
    }
  }
}

// One layer: RB row blocks x NB column blocks per wave; 4 / RB row groups x
// 4 RB column groups of waves; N in chunks of (column groups x NB x 16).
template <int RB, int NB, int T>
__device__ __attribute__((always_inline)) inline void plain_layer(const LayerCtx& C, int in, int pin, int out, int pout, float* gmax, int rows_valid,
                            bool out_planes, Pre pre = {}, int oflag = 0) {
  constexpr int WR = kRowBlocks / RB, WC = kWaves / WR, CB = WC * NB;
  const int lane = pn_tid() & 63, wave = pn_tid() >> 6;
  const int wr = wave / WC, wc = wave % WC;
  const int kq = lane >> 4, cl = lane & 15;
  const int row0 = wr * RB * 16;
  // N is a multiple of the chunk width, or narrower than one chunk (then the
  // waves past column N / 16 idle; there is no barrier inside a layer)
  if (C.N < CB * 16 && wc * NB * 16 >= C.N) return;
  f32x4 acc[RB][NB];
  zero_acc(acc);
  auto epi = [&](f32x4 (&a)[RB][NB], int c) {
    const int col0 = (c * CB + wc * NB) * 16;
    if (gmax) pool_cols<RB, NB, T>(a, C.bias, col0, C.relu, row0, rows_valid, gmax, C.sc);
    else if (out_planes) store_cols_planes<RB, NB, T>(a, C.bias, col0, C.relu, row0, out, C.N + kPadB, col0, C.sc, oflag);
    else store_cols<RB, NB, T>(a, C.bias, col0, C.relu, row0, out, pout, col0, C.sc);
    zero_acc(a);
  };
  const int nchunk = C.N < CB * 16 ? 1 : C.N / (CB * 16);
  if (C.prec) {  // input: three bf16 planes of pitch K + kPadB (the producer's N + kPadB)
    const int pb = 32 * C.KG + kPadB;
    const __bf16* abase6 = reinterpret_cast<const __bf16*>(g_smem + in) + (row0 + cl) * pb + plane_col(cl, 8 * kq);
#ifndef NDNET_PN_SHORT_D2
#define NDNET_PN_SHORT_D2 1
#endif
    // a layer of two k-group steps (K = 64, one chunk: the narrow 64 -> 64 /
    // 64 -> 128 layers) loads both up front, so only one L2 latency is exposed
    if (NDNET_PN_SHORT_D2 && nchunk * C.KG == 2)
      run_tiles_x6<T, RB, NB, decltype(epi), 2>(acc, C.w6, C.KG, 0, C.KG, wc * NB, CB, nchunk, abase6, pb, epi, pre, 0);
    else
      run_tiles_x6<T, RB, NB>(acc, C.w6, C.KG, 0, C.KG, wc * NB, CB, nchunk, abase6, pb, epi, pre,
                           kChunkRot ? (int)((blockIdx.x + blockIdx.y) % nchunk) : 0);
  } else {
    const float* abase = g_smem + in + (row0 + cl) * pin + 4 * kq;
    run_tiles<RB, NB>(acc, C.w, C.KG, 0, C.KG, wc * NB, CB, nchunk, abase, pin, epi, pre);
  }
}

// Floats of the fused pair's double buffer: two 64-column chunks, fp32 or
// (split-bf16 consumer) three bf16 planes of pitch 72.
__host__ __device__ inline int fbuf_floats(int qprec) {
  return qprec ? 2 * 3 * kP * (kFuseNC + kPadB) / 2 : 2 * kP * (kFuseNC + kPadF);
}

// A fused pair: layer P (K -> N1) produced 64 columns at a time into a
// double-buffered LDS chunk (waves 4 x 4, one 16 x 16 tile each), each chunk
// consumed at once as 4 k-groups of layer Q (N1 -> N2 = one chunk of Q's
// (RB, NB) split), whose accumulators persist across the chunks: the N1-wide
// activation never needs LDS of its own.  One barrier per chunk.
template <int RB, int NB, int T>
__device__ __attribute__((always_inline)) inline void fused_pair(const LayerCtx& P, const LayerCtx& Q, int in, int pin, int fbuf, int out, int pout,
                           float* gmax, int rows_valid, bool out_planes, Pre pre = {}, int qflag = 0, int oflag = 0) {
  constexpr int kFP = kFuseNC + kPadF;
  constexpr int WR = kRowBlocks / RB, WC = kWaves / WR;
  const int lane = pn_tid() & 63, wave = pn_tid() >> 6;
  const int kq = lane >> 4, cl = lane & 15;
  // P: row block wave / PWC, PNB column blocks from 4 f + PNB (wave % PWC)
  constexpr int PWC = kWaves / kRowBlocks, PNB = 4 / PWC;
  const int prow0 = (wave / PWC) * 16, pwc = (wave % PWC) * PNB;
  const float* ain = g_smem + in + (prow0 + cl) * pin + 4 * kq;
  const __bf16* ain6 = reinterpret_cast<const __bf16*>(g_smem + in) + (prow0 + cl) * (32 * P.KG + kPadB) +
                       plane_col(cl, 8 * kq);
  // Q: row group wave / WC, column group wave % WC
  const int qrow0 = (wave / WC) * RB * 16, qwc = wave % WC;
  const bool qidle = qwc * NB * 16 >= Q.N;
  const int nf = P.N / kFuseNC;
  // a split-bf16 Q reads its chunks as three bf16 planes (pitch 72)
  const int fbsz = Q.prec ? fbuf_floats(1) / 2 : kP * kFP;
  auto p_chunk = [&](int f) {
    f32x4 acc1[1][PNB];
    zero_acc(acc1);
    const int fb = fbuf + (f & 1) * fbsz;
    auto epi = [&](f32x4 (&a)[1][PNB], int) {
      if (Q.prec) store_cols_planes<1, PNB, T>(a, P.bias, 64 * f + 16 * pwc, P.relu, prow0, fb, kFuseNC + kPadB, 16 * pwc, P.sc, qflag);
      else store_cols<1, PNB, T>(a, P.bias, 64 * f + 16 * pwc, P.relu, prow0, fb, kFP, 16 * pwc, P.sc);
    };
    Pre pf = pre;
    if (f != 0) pf.on = false;
    if (P.prec) run_tiles_x6<T, 1, PNB>(acc1, P.w6, P.KG, 0, P.KG, 4 * f + pwc, 0, 1, ain6, 32 * P.KG + kPadB, epi, pf);
    else run_tiles<1, PNB>(acc1, P.w, P.KG, 0, P.KG, 4 * f + pwc, 0, 1, ain, pin, epi, pf);
  };
  f32x4 acc2[RB][NB];
  zero_acc(acc2);
  p_chunk(0);
  __syncthreads();
  for (int f = 0; f < nf; f++) {
    if (!qidle) {
      if (Q.prec) {
        const __bf16* af6 = reinterpret_cast<const __bf16*>(g_smem + fbuf + (f & 1) * fbsz) +
                            (qrow0 + cl) * (kFuseNC + kPadB) + plane_col(cl, 8 * kq);
        run_tiles_x6<T, RB, NB>(acc2, Q.w6, Q.KG, 2 * f, 2, qwc * NB, 0, 1, af6, kFuseNC + kPadB,
                             [](f32x4 (&)[RB][NB], int) {});
      } else {
        const float* af = g_smem + fbuf + (f & 1) * fbsz + (qrow0 + cl) * kFP + 4 * kq;
        run_tiles<RB, NB>(acc2, Q.w, Q.KG, 4 * f, 4, qwc * NB, 0, 1, af, kFP, [](f32x4 (&)[RB][NB], int) {});
      }
    }
    if (f + 1 < nf) p_chunk(f + 1);
    __syncthreads();
  }
  if (qidle) return;
  if (gmax) pool_cols<RB, NB, T>(acc2, Q.bias, 16 * qwc * NB, Q.relu, qrow0, rows_valid, gmax, Q.sc);
  else if (out_planes) store_cols_planes<RB, NB, T>(acc2, Q.bias, 16 * qwc * NB, Q.relu, qrow0, out, Q.N + kPadB, 16 * qwc * NB, Q.sc, oflag);
  else store_cols<RB, NB, T>(acc2, Q.bias, 16 * qwc * NB, Q.relu, qrow0, out, pout, 16 * qwc * NB, Q.sc);
}

// The fused pair with both layers split-bf16 and P's K = 64 (the seg head's
// 64 -> 512 -> 256, ndtnet.py:233-234), software-pipelined across chunks.
// fused_pair loads each chunk's weights at the start of the chunk's GEMM, so
// every chunk exposes the L2 latency of P's and Q's first steps -- with all 16
// waves in lockstep between the chunk barriers, nothing covers it (chain D's
// pair ran at ~0.42 of the issued peak against ~0.55 for the plain x6 layers,
// profiles/r04_chain_vgpr_ab.txt).  Here a chunk's weights (P: 2 k-groups, Q:
// 2 k-groups, 3 planes each: 48 VGPRs) are loaded one chunk ahead, right after
// the previous chunk's MFMAs consumed the registers, so each load has a whole
// phase and a barrier to arrive.  Same products, same accumulation order.
//
// PF32: P is a prec-0 layer with K = 16 at the head of the chain (the seg head's conv1 with conv1, t1 and
// t2 folded in per cloud: 12 -> 512).  Its A operand is this lane's piece of its input row (xa: row
// prow0 + cl, columns 4 kq .. 4 kq + 3, loaded once by the kernel's prologue and kept for all chunks),
// its weights per chunk one fp32 fragment (1 KB per wave, loaded one chunk ahead as wp is): four
// v_mfma_f32_16x16x4_f32 where the split-bf16 P issues twelve bf16 MFMAs and six LDS fragment reads.
// There is no LDS input tile and no layer-0 phase in front of it.  Q's side is the same code.
template <int RB, int T, bool PF32 = false>
__device__ __attribute__((always_inline)) inline void fused_pair_x6p(const LayerCtx& P, const LayerCtx& Q, int in,
                                                                     int fbuf, int out, int pout, float* gmax,
                                                                     int rows_valid, bool out_planes,
                                                                     f32x4 xa = {0.f, 0.f, 0.f, 0.f}, int qflag = 0,
                                                                     int oflag = 0) {
  constexpr int WR = kRowBlocks / RB, WC = kWaves / WR;  // Q: NB = 1
  constexpr int PWC = kWaves / kRowBlocks;                // P: 4 column groups of one block
  static_assert(PWC == 4 && kFuseNC == 64, "16 waves, 64-column chunks");
  const int lane = pn_tid() & 63, wave = pn_tid() >> 6;
  const int kq = lane >> 4, cl = lane & 15;
  const int prow0 = (wave / PWC) * 16, pwc = wave % PWC;
  const int pinb = 32 * P.KG + kPadB;  // P.KG == 2
  const __bf16* ain6 = reinterpret_cast<const __bf16*>(g_smem + in) + (prow0 + cl) * pinb + plane_col(cl, 8 * kq);
  const int qrow0 = (wave / WC) * RB * 16, qwc = wave % WC;
  const int nf = P.N / kFuseNC;
  const int fbsz = fbuf_floats(1) / 2;
  constexpr int fpb = kFuseNC + kPadB;
  // chunk f's weights: P column block 4 f + pwc, k-groups 0, 1; Q column block qwc, k-groups 2 f, 2 f + 1
  constexpr int NPL = kPlanes<T>;  // of the three planes stored per k-group (the fp16 form: both of its two)
  constexpr int WPL = kWPlanes<T>;
  bf16x8 wp[2][1][NPL], wq[2][1][NPL];
  f32x4 wpf[1];  // PF32: chunk f's fragment of P (one k-group)
  auto load_p = [&](int f) {
    if constexpr (PF32) {
      wpf[0] = P.w[(int64_t)(4 * f + pwc) * 64];
      return;
    }
    const bf16x8* s = P.w6 + ((int64_t)(4 * f + pwc) * P.KG) * WPL * 64;
#pragma unroll
    for (int k = 0; k < 2; k++)
#pragma unroll
      for (int p = 0; p < NPL; p++) wp[k][0][p] = s[(k * WPL + p) * 64];
  };
  auto load_q = [&](int f) {
    const bf16x8* s = Q.w6 + ((int64_t)qwc * Q.KG + 2 * f) * WPL * 64;
#pragma unroll
    for (int k = 0; k < 2; k++)
#pragma unroll
      for (int p = 0; p < NPL; p++) wq[k][0][p] = s[(k * WPL + p) * 64];
  };
  auto p_chunk = [&](int f) {
    f32x4 acc1[1][1];
    zero_acc(acc1);
    if constexpr (PF32) {
      const f32x4 a1[1] = {xa};
      mma_kgroup<1, 1>(acc1, a1, wpf);
    } else {
#pragma unroll
      for (int k = 0; k < 2; k++) mma_kgroup_x6<1, 1, T>(acc1, ain6 + 32 * k, kP * pinb, 16 * pinb, wp[k]);
    }
    store_cols_planes<1, 1, T>(acc1, P.bias, 64 * f + 16 * pwc, P.relu, prow0, fbuf + (f & 1) * fbsz, fpb, 16 * pwc, P.sc,
                               qflag);
  };
  f32x4 acc2[RB][1];
  zero_acc(acc2);
  load_p(0);
  load_q(0);
  p_chunk(0);
  if (nf > 1) load_p(1);
  __syncthreads();
  for (int f = 0; f < nf; f++) {
    const __bf16* af6 =
        reinterpret_cast<const __bf16*>(g_smem + fbuf + (f & 1) * fbsz) + (qrow0 + cl) * fpb + plane_col(cl, 8 * kq);
#if NDNET_PN_PAIR_PFIRST
    // A/B: chunk f + 1's P (into the other buffer, free since the last
    // barrier) before chunk f's Q, so its epilogue overlaps other waves' Q
    // MFMAs and the barrier follows the uniform Q phase
    if (f + 1 < nf) {
      p_chunk(f + 1);
      if (f + 2 < nf) load_p(f + 2);
    }
#pragma unroll
    for (int k = 0; k < 2; k++) mma_kgroup_x6<RB, 1, T>(acc2, af6 + 32 * k, kP * fpb, 16 * fpb, wq[k]);
    if (f + 1 < nf) load_q(f + 1);
#else
#pragma unroll
    for (int k = 0; k < 2; k++) mma_kgroup_x6<RB, 1, T>(acc2, af6 + 32 * k, kP * fpb, 16 * fpb, wq[k]);
    if (f + 1 < nf) {
      load_q(f + 1);
      p_chunk(f + 1);
      if (f + 2 < nf) load_p(f + 2);
    }
#endif
    __syncthreads();
  }
  if (gmax) pool_cols<RB, 1, T>(acc2, Q.bias, 16 * qwc, Q.relu, qrow0, rows_valid, gmax, Q.sc);
  else if (out_planes) store_cols_planes<RB, 1, T>(acc2, Q.bias, 16 * qwc, Q.relu, qrow0, out, Q.N + kPadB, 16 * qwc, Q.sc, oflag);
  else store_cols<RB, 1, T>(acc2, Q.bias, 16 * qwc, Q.relu, qrow0, out, pout, 16 * qwc, Q.sc);
}

// Loads the first weight step this wave runs in layer l (the 16-wave 64-point
// build; others leave pre off): the column block plain_layer<RB, 1> /
// fused_pair's first chunk gives the wave, at k-group 0 -- the address
// run_tiles* would load first.
template <int T>
__device__ inline void prefetch_first(const ndnet_pn_chain& A, int l, int b, Pre& pre) {
  pre.on = false;
  if constexpr (T == 2) return;  // (the experiment below addresses three planes per k-group)
#ifndef NDNET_PN_PREFETCH  // off by default: measured 1-2 us slower per chain (profiles/r03e_stamps_ab.txt)
  return;
#endif
  if constexpr (kP == 64 && kWaves == 16) {
    const ndnet_pn_layer& L = A.L[l];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int cb0;
    if (L.fuse_next) {
      cb0 = wave % 4;  // fused_pair: PWC = 4 column groups of PNB = 1, chunk 0
    } else {
      const int WC = L.N % 256 == 0 ? 16 : L.N % 128 == 0 ? 8 : 4;  // plain_layer<4 | 2 | 1, 1>
      cb0 = wave % WC;
      if (L.N < WC * 16 && cb0 * 16 >= L.N) return;  // an idle wave of a narrow layer
    }
    const int KG = L.prec ? L.K / 32 : L.K / 16;
    const float* wb = L.w + (int64_t)b * L.w_cloud_stride;
    if (L.prec) {  // the planes the mode reads
      const bf16x8* q = reinterpret_cast<const bf16x8*>(wb) + lane + (int64_t)cb0 * KG * 3 * 64;
      pre.r0 = __builtin_bit_cast(f32x4, q[0]);
      if constexpr (T >= 3) pre.r1 = __builtin_bit_cast(f32x4, q[64]);
      if constexpr (T == 6) pre.r2 = __builtin_bit_cast(f32x4, q[128]);
    } else {
      pre.r0 = (reinterpret_cast<const f32x4*>(wb) + lane + (int64_t)cb0 * KG * 64)[0];
    }
    pre.on = true;
  }
}

// The barrier between layers: LDS traffic retired, then s_barrier, with no
// vmcnt drain (__syncthreads' fence waits for every vector-memory op, the
// next layer's prefetched weights included; nothing between layers is a
// global store -- the max-pool atomics come only in the last layer, which
// closes with __syncthreads).
__device__ inline void layer_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// Floats of LDS region r: fp32 activations (pitch width + kPadF) or, when it ever
// holds a split-bf16 layer's input (planes bit r), three bf16 planes.
__host__ __device__ inline int region_floats(int width, int planes) {
  const int f32 = kP * (width + kPadF), b16 = 3 * kP * (width + kPadB) / 2;
  return planes && b16 > f32 ? b16 : f32;
}

// Layer 0 of the chains (conv1 of ndtnet.py:47 / :148, K = 3 or 12 inputs
// padded to 16, N = 64) runs on the VALU straight from the input rows: each
// thread computes 4 channels of one point from the point's 12 input floats
// (three dwordx4 loads) and W0^T staged in LDS row-major ([16][64]) -- no
// input tile, no MFMA fragment loads, one memory round trip for x, W0, every
// layer's bias and (chain B) the TNet(3) tail.  The products are fp32 FMAs
// (k ascending); the MFMA path computed the same sums in another order.
__host__ __device__ inline bool valu_layer0(const ndnet_pn_chain& A) {
  return A.num_layers > 1 && A.L[0].K == 16 && A.L[0].N == 64 && A.L[0].prec == 0 && !A.L[0].fuse_next &&
         A.in_cols <= 12 && A.x_ld % 4 == 0;
}

// 1: the 16-wave 64-point build runs a fused pair into a 256-wide split-bf16 Q software-pipelined
// (fused_pair_x6p); 0 (a build switch for comparisons): every pair takes the generic fused_pair.
#ifndef NDNET_PN_FUSED_PIPE
#define NDNET_PN_FUSED_PIPE 1
#endif

// The chain opens with a fused pair whose P (prec 0, K = 16) the 16-wave 64-point build runs straight
// from the input rows (fused_pair_x6p<.., PF32>): no input tile is staged and none is sized.
__host__ __device__ inline bool pair0_direct(const ndnet_pn_chain& A) {
  return kP == 64 && kWaves == 16 && NDNET_PN_FUSED_PIPE && A.num_layers >= 2 && A.L[0].fuse_next &&
         A.L[0].prec == 0 && A.L[0].K == 16 && A.L[1].prec != 0 && A.L[1].N == 256 && A.x_ld % 4 == 0 &&
         (uintptr_t)A.x % 16 == 0 && !A.head_h2;
}

// LDS floats of the VALU layer-0 prologue scratch (W0^T [16][64] + bias [64]),
// overlaid on activation region 0, which layer 0 neither reads nor writes.
constexpr int kValu0Floats = 16 * 64 + 64;

// Floats of activation region 0 (kernel and launcher): room for the layer-0
// prologue's scratch (+ chain B's t1) when layer 0 runs on the VALU.
__host__ __device__ inline int region0_floats(const ndnet_pn_chain& A, int planes) {
  const int r = region_floats(A.max_width, planes & 1);
  return valu_layer0(A) && r < kValu0Floats + 16 ? kValu0Floats + 16 : r;
}

// The kernel's body, one tile from its first load to its stores.  T = 2 is the fp16 form (X: its planes
// and scales; flag_base: NDNET_PN_MAX_LAYERS LDS words, word l the maximum |v| of split layer l's input
// tile, gathered by the epilogue that stores it): it tests each split layer's input after the barrier
// that closes its producer and returns false -- the whole workgroup, before the chain's first global
// store or atomic other than the head prologue's -- when one lies outside the window; the caller then
// runs the tile through T = 6.  Every other T returns true.
template <int T>
__device__ __attribute__((always_inline)) inline bool pn_chain_body(const ndnet_pn_chain& A, const ndnet_pn_f16* X,
                                                                    int planes, int fbuf, int bias_base,
                                                                    int flag_base) {
#define PN_BODY_FAIL return false
#include "pointnet_chain_body.inc"
#undef PN_BODY_FAIL
  return true;
}

// One instantiation per mode of the chain's split-bf16 layers (T terms):
// k_pn_chain<6> serves prec 1 and chains with no split layer -- the kernel as
// it was before the modes, register for register -- <3> prec 2, <1> prec 3.
template <int T>
__global__ void __launch_bounds__(kThreads) k_pn_chain(ndnet_pn_chain A, int planes, int fbuf, int bias_base) {
  static_assert(T != 2, "the fp16 form is k_pn_chain_f16");
  constexpr const ndnet_pn_f16* X = nullptr;
  constexpr int flag_base = 0;
#define PN_BODY_FAIL return
#include "pointnet_chain_body.inc"
#undef PN_BODY_FAIL
}

// The fp16 form with its fallback: a tile whose activations leave fp16's window (pn_chain_body<2> returns
// false, the whole workgroup at one point, nothing of the tile stored yet) runs k_pn_chain<6>'s body from
// the start, on the same LDS layout -- the fp16 planes are the first two of the three bf16 ones -- and is
// counted.
__global__ void __launch_bounds__(kThreads) k_pn_chain_f16(ndnet_pn_chain A, ndnet_pn_f16 X, int planes, int fbuf,
                                                           int bias_base, int flag_base) {
  if (pn_chain_body<2>(A, &X, planes, fbuf, bias_base, flag_base)) return;
  __syncthreads();  // every wave has left the fp16 body: its LDS is free
  if (threadIdx.x == 0) atomicAdd(X.fallbacks, 1u);
  pn_chain_body<6>(A, nullptr, planes, fbuf, bias_base, 0);
}

// ---------------------------------------------------------------------------
// Per-cloud steps between the chains (the TNet FC heads, ndtnet.py:53-60, and
// the weight folds), on the same stream.  The batch is small (B clouds, a
// 16-row GEMM at B = 16), so these are weight-streaming GEMVs, not MFMA tiles.

// out[b][n] = act(bias[n] + sum_k in[b][k] * W[n][k]), b < B <= 16.
// One wave per output channel (4 per workgroup): its 64 lanes split K in
// 16-byte pieces and keep one partial sum per cloud, so the weight row is read
// once for all clouds; the partials meet in a wave reduction.
__global__ void __launch_bounds__(256) k_pn_fc(const float* __restrict__ in, int ld_in, const float* __restrict__ W,
                                               const float* __restrict__ bias, float* __restrict__ out, int ld_out,
                                               int B, int K, int N, int relu) {
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;
  const int kv = K / 4;
  const f32x4* w = reinterpret_cast<const f32x4*>(W + (int64_t)n * K);
  float acc[16];
#pragma unroll
  for (int b = 0; b < 16; b++) acc[b] = 0.0f;
  for (int f = lane; f < kv; f += 64) {
    const f32x4 wv = w[f];
    f32x4 xv[16];
#pragma unroll
    for (int b = 0; b < 16; b++) xv[b] = reinterpret_cast<const f32x4*>(in + (int64_t)(b < B ? b : 0) * ld_in)[f];
#pragma unroll
    for (int b = 0; b < 16; b++) {
      const f32x4 pr = xv[b] * wv;
      acc[b] += (pr[0] + pr[1]) + (pr[2] + pr[3]);
    }
  }
#pragma unroll
  for (int b = 0; b < 16; b++)
    for (int o = 32; o > 0; o >>= 1) acc[b] += __shfl_xor(acc[b], o, 64);
  if (lane < B) {
    float v = 0.0f;
#pragma unroll
    for (int b = 0; b < 16; b++) v = lane == b ? acc[b] : v;
    v += bias[n];
    if (relu) v = fmaxf(v, 0.0f);
    out[(int64_t)lane * ld_out + n] = v;
  }
}

// The same FC layer on the fp32 matrix cores: a 16-row GEMM (row = cloud,
// b < B <= 16) with W^T fragment-major (the chain layout, [cb][kg][lane][4]).
// One workgroup per 16-column block; its kFcWaves waves (8: measured best in the
// pipelined step, 16 slowed it) split the K-groups,
// each wave's weight fragments (1 KB each) and input pieces (a float4 of 4
// consecutive k per lane) loaded up front -- one memory round trip per
// launch -- then 4 MFMAs per k-group; the waves' 16 x 16 partial tiles are
// summed in LDS in wave order (deterministic) and wave 0 adds the bias.
// Products are exact and sums fp32, as torch's fp32 GEMM (another order).
#ifndef NDNET_PN_FC_WAVES
#define NDNET_PN_FC_WAVES 8
#endif
constexpr int kFcWaves = NDNET_PN_FC_WAVES, kFcMaxG = 64 / kFcWaves;  // K <= 16 * kFcWaves * kFcMaxG = 1024
// CBW column blocks per workgroup (round 6): a wide, shallow layer (TNet(64)'s
// fc3, 256 -> 4096: 256 one-block workgroups, ~5 us each, the whole chip for
// its duration in the pipelined step) runs as 64 four-block workgroups, each
// wave holding CBW x ng weight fragments (ng * CBW <= kFcMaxG registers'
// worth, the host checks) -- the same per-column sums in the same order, so
// the output is bit-identical for every CBW; only the CU-time shrinks.
template <int CBW>
__global__ void __launch_bounds__(kFcWaves * 64) k_pn_fc_mfma(const float* __restrict__ in, int ld_in,
                                                              const f32x4* __restrict__ wf,
                                                              const float* __restrict__ bias, int bias_ld,
                                                              float* __restrict__ out, int ld_out, int B, int KG,
                                                              int relu) {
  constexpr int kG = kFcMaxG / CBW;
  static_assert(CBW <= kFcWaves && kG >= 1, "one reducing wave per column block");
  __shared__ f32x4 part[kFcWaves][CBW][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int kq = lane >> 4, cl = lane & 15;
  const int cb0 = blockIdx.x * CBW;
  const int kg0 = KG * wave / kFcWaves, ng = KG * (wave + 1) / kFcWaves - kg0;
  const float* xr = in + (int64_t)(cl < B ? cl : 0) * ld_in + 16 * kg0 + 4 * kq;  // rows past B: discarded
  // the reducing waves' bias values (clouds 4 kq + r of column 16 (cb0 + wave) + cl; rows past B: the last
  // row's, discarded), loaded with the first loads; bias_ld 0: one bias row for every cloud
  float bv[4] = {0.f, 0.f, 0.f, 0.f};
  if (wave < CBW) {
#pragma unroll
    for (int r = 0; r < 4; r++) bv[r] = bias[(int64_t)min(4 * kq + r, B - 1) * bias_ld + 16 * (cb0 + wave) + cl];
  }
  f32x4 wv[CBW][kG], xv[kG];
#pragma unroll
  for (int i = 0; i < kG; i++) {
    if (i < ng) {
      xv[i] = *reinterpret_cast<const f32x4*>(xr + 16 * i);
#pragma unroll
      for (int j = 0; j < CBW; j++) wv[j][i] = wf[((int64_t)(cb0 + j) * KG + kg0 + i) * 64 + lane];
    }
  }
#pragma unroll
  for (int j = 0; j < CBW; j++) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < kG; i++)
      if (i < ng)
#pragma unroll
        for (int s = 0; s < 4; s++) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[i][s], wv[j][i][s], acc, 0, 0, 0);
    part[wave][j][lane] = acc;
  }
  __syncthreads();
  if (wave >= CBW) return;
  const int j = wave;  // wave j reduces column block cb0 + j over the waves in order
  f32x4 t = part[0][j][lane];
#pragma unroll
  for (int w = 1; w < kFcWaves; w++) t += part[w][j][lane];
  // lane (kq, cl): clouds 4 kq + r of column 16 (cb0 + j) + cl
  const int n = 16 * (cb0 + j) + cl;
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const int b = 4 * kq + r;
    if (b < B) {
      float v = t[r] + bv[r];
      if (relu) v = fmaxf(v, 0.0f);
      out[(int64_t)b * ld_out + n] = v;
    }
  }
}

#if NDNET_PN_TILE == 64
// The classification head's last layer and its softmax (ndtnet.py:188-194) in
// one launch: probs[b] = softmax(in[b] @ W^T + bias) over the first out_cols
// of N padded columns.  One workgroup per chunk of 16 clouds (one 16-row tile
// of the fp32 MFMA); no workgroup talks to another.  Every wave keeps the
// chunk's 16 x K input fragment in registers (K <= 256: 16 float4) and
// streams the weight fragments of its column blocks (wave, wave + 8, ...),
// the next block's loads issued ahead of the current one's MFMAs (as compiled
// they are waited for before the chain; a straight-line variant that keeps
// them in flight across it measured slower, 24.4 against 19.6 us at N = 512);
// one wave forms a column's whole K-sum, k-group by k-group, so the result
// does not depend on scheduling.  The 16 x N logits (+ bias) go to LDS (<= 64 KB) and
// never to memory unless `logits` asks for them; then one wave per row takes
// the maximum of the first out_cols columns (padded columns take no part),
// exp(x - max) with the accurate expf, the sum (64 strided partial sums, then a
// butterfly) and a true division.  Rows at or past `batch` read the chunk's
// first row and are discarded.  `clear` is filled with -inf, the workgroups
// sharing the range: the kernel does not read it.
constexpr int kClsWaves = 8, kClsMaxG = 16;  // K <= 16 * kClsMaxG = 256
__global__ void __launch_bounds__(kClsWaves * 64) k_pn_cls_head(const float* __restrict__ in, int ld_in,
                                                                const f32x4* __restrict__ wf,
                                                                const float* __restrict__ bias, float* __restrict__ probs,
                                                                int ld_probs, float* __restrict__ logits, int ld_logits,
                                                                int batch, int KG, int N, int out_cols,
                                                                float* __restrict__ clear, int64_t clear_count) {
  extern __shared__ float cls_lg[];  // [16][N]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int kq = lane >> 4, cl = lane & 15;
  for (int64_t i = (int64_t)blockIdx.x * (kClsWaves * 64) + threadIdx.x; i < clear_count;
       i += (int64_t)gridDim.x * (kClsWaves * 64))
    clear[i] = -INFINITY;
  const int b0 = blockIdx.x * 16;
  const int B = batch - b0 < 16 ? batch - b0 : 16;
  const float* xr = in + (int64_t)(b0 + (cl < B ? cl : 0)) * ld_in + 4 * kq;
  f32x4 xv[kClsMaxG], cur[kClsMaxG], nxt[kClsMaxG];
#pragma unroll
  for (int i = 0; i < kClsMaxG; i++)
    if (i < KG) xv[i] = *reinterpret_cast<const f32x4*>(xr + 16 * i);
  const int nb = N >> 4;
  if (wave < nb) {
#pragma unroll
    for (int i = 0; i < kClsMaxG; i++)
      if (i < KG) cur[i] = wf[((int64_t)wave * KG + i) * 64 + lane];
  }
  for (int cb = wave; cb < nb; cb += kClsWaves) {
    if (cb + kClsWaves < nb) {
#pragma unroll
      for (int i = 0; i < kClsMaxG; i++)
        if (i < KG) nxt[i] = wf[((int64_t)(cb + kClsWaves) * KG + i) * 64 + lane];
    }
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < kClsMaxG; i++)
      if (i < KG)
#pragma unroll
        for (int s = 0; s < 4; s++) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[i][s], cur[i][s], acc, 0, 0, 0);
    // lane (kq, cl): clouds 4 kq + r of column 16 cb + cl
    const int n = 16 * cb + cl;
    const float bv = bias[n];
#pragma unroll
    for (int r = 0; r < 4; r++) cls_lg[(4 * kq + r) * N + n] = acc[r] + bv;
#pragma unroll
    for (int i = 0; i < kClsMaxG; i++) cur[i] = nxt[i];
  }
  __syncthreads();
  for (int r = wave; r < B; r += kClsWaves) {  // one wave per cloud; a lane rereads only what it wrote
    float* row = cls_lg + r * N;
    float m = -INFINITY;
    for (int c = lane; c < out_cols; c += 64) m = fmaxf(m, row[c]);
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    float sum = 0.0f;
    for (int c = lane; c < out_cols; c += 64) {
      const float x = row[c];
      if (logits) logits[(int64_t)(b0 + r) * ld_logits + c] = x;
      const float e = expf(x - m);
      row[c] = e;
      sum += e;
    }
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    float* pr = probs + (int64_t)(b0 + r) * ld_probs;
    for (int c = lane; c < out_cols; c += 64) pr[c] = row[c] / sum;
  }
}
#endif

// Index of W^T element (k, n) in the fragment-major layout (KG k-groups).
__device__ inline int64_t frag_index(int k, int n, int KG) {
  return ((int64_t)((n >> 4) * KG + (k >> 4)) * 64 + ((k >> 2) & 3) * 16 + (n & 15)) * 4 + (k & 3);
}

// The same GEMV with K split across the lanes of WPO waves (K = 256 WPO,
// WPO = 2 or 4; at K = 256 the one-wave kernel above measured faster): every thread loads ONE float4 of the weight row and the
// matching float4 of all B inputs up front -- a single memory round trip
// per launch instead of one per K-chunk of 64 lanes -- then the partial sums
// of the 16 clouds are reduced across the wave (shuffles) and the WPO waves
// (LDS).  4 / WPO output channels per 256-thread workgroup.
template <int WPO>
__global__ void __launch_bounds__(256) k_pn_fc_split(const float* __restrict__ in, int ld_in,
                                                     const float* __restrict__ W, const float* __restrict__ bias,
                                                     float* __restrict__ out, int ld_out, int B, int N, int relu) {
  constexpr int K = 256 * WPO, OPW = 4 / WPO;
  __shared__ float s_part[4][16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int o = wave / WPO, wq = wave % WPO;  // output within the workgroup, K quarter of that output
  const int n = blockIdx.x * OPW + o;
  const int nn = n < N ? n : N - 1;
  const int c4 = wq * 64 + lane;  // this thread's float4 of the row
  const f32x4 wv = reinterpret_cast<const f32x4*>(W + (int64_t)nn * K)[c4];
  f32x4 xv[16];
#pragma unroll
  for (int b = 0; b < 16; b++) xv[b] = reinterpret_cast<const f32x4*>(in + (int64_t)(b < B ? b : 0) * ld_in)[c4];
  float acc[16];
#pragma unroll
  for (int b = 0; b < 16; b++) {
    const f32x4 pr = xv[b] * wv;
    acc[b] = (pr[0] + pr[1]) + (pr[2] + pr[3]);
  }
#pragma unroll
  for (int b = 0; b < 16; b++)
    for (int off = 32; off > 0; off >>= 1) acc[b] += __shfl_xor(acc[b], off, 64);
  if (WPO > 1) {
    if (lane < 16) {
      float v = 0.0f;
#pragma unroll
      for (int b = 0; b < 16; b++) v = lane == b ? acc[b] : v;
      s_part[wave][lane] = v;
    }
    __syncthreads();
    if (wq != 0) return;
    if (lane < 16) {
      float v = 0.0f;
#pragma unroll
      for (int q = 0; q < WPO; q++) v += s_part[wave + q][lane];
      acc[0] = v;
    }
  } else if (lane < 16) {
    float v = 0.0f;
#pragma unroll
    for (int b = 0; b < 16; b++) v = lane == b ? acc[b] : v;
    acc[0] = v;
  }
  if (lane < B && n < N) {
    float v = acc[0] + bias[n];
    if (relu) v = fmaxf(v, 0.0f);
    out[(int64_t)lane * ld_out + n] = v;
  }
}

// TNet(64)'s transform through conv1 for chains C and D (ndtnet.py:152-155,
// x_t2 = t2^T (W1' x + b1)): W1''[b] = W1'[b]^T t2[b] (12 x 64) and b1''[b] =
// b1^T t2[b], once per cloud, written as chains C / D read their layer 0
// (fragment-major, K padded to 16, rows 12..15 left as they are: zero) and
// the per-cloud bias.  fp32 FMAs in i order.  (Before round 5 every chain-C
// workgroup computed it in its prologue on the fp32 MFMA: 16 workgroups per
// cloud doing the same 16 x 64 x 64 product, ~2 us of each one's time.)
__global__ void __launch_bounds__(1024) k_pn_fold_t2(const float* __restrict__ w1f, int w1_stride,
                                                     const float* __restrict__ b1, const float* __restrict__ t2,
                                                     int t2_ld, float* __restrict__ outf, float* __restrict__ outb) {
  const int b = blockIdx.x, e = threadIdx.x;
  __shared__ float s_w[13 * 64];  // rows 0..11 W1'^T (row-major [k][n]), row 12 the bias
  __shared__ float s_t[64 * 64];
  {
    const float* wb = w1f + (int64_t)b * w1_stride;
    if (e < 16 * 64) {  // fragment-major element e -> (k, n)
      const int cb = e >> 8, ln = (e >> 2) & 63, k = 4 * (ln >> 4) + (e & 3), n = 16 * cb + (ln & 15);
      const float v = wb[e];
      if (k < 12) s_w[k * 64 + n] = v;
    }
    if (e < 64) s_w[12 * 64 + e] = b1[e];
    const f32x4* tb = reinterpret_cast<const f32x4*>(t2 + (int64_t)b * t2_ld);
    reinterpret_cast<f32x4*>(s_t)[e] = tb[e];  // 1024 threads x 4 = the 64 x 64 matrix
  }
  __syncthreads();
  if (e < 13 * 64) {
    const int r = e >> 6, n = e & 63;
    float acc = 0.0f;
#pragma unroll 16
    for (int i = 0; i < 64; i++) acc = fmaf(s_w[r * 64 + i], s_t[i * 64 + n], acc);
    if (r < 12) outf[(int64_t)b * 1024 + ((((n >> 4) * 64 + ((r >> 2) & 3) * 16 + (n & 15)) << 2) + (r & 3))] = acc;
    else outb[(int64_t)b * 64 + n] = acc;
  }
}

// k_pn_fold_t2's work and, from the values it has just formed, the seg head's conv1 collapsed into the same
// per-cloud layer (ndnet_pn_fold_seg_run): no ReLU separates x_t2 = x W1''[b] + b1''[b] from conv1's
// x_t2 s1a^T (+ the per-cloud global-feature bias), so chain D's first layer is 12 -> N2,
//   wd[b] = W1''[b] s1a^T (12 x N2, fragment-major K = 16, rows 12..15 untouched),  bd[b] = b1''[b] s1a^T + s1b.
// One workgroup per 64 columns of one cloud.  Each repeats the 13 x 64 fold (the same fp32 FMAs in the
// same order as k_pn_fold_t2: the cloud's first workgroup stores outf / outb, bit for bit that kernel's),
// then forms its 13 x 64 slice from those fp32 values, one output per thread: double FMAs, i ascending,
// rounded once, both operands converted to double once when they are staged in LDS.  On the VALU, not the
// f64 MFMA: this launch runs in the forward's serial chain beside other forwards' chain kernels, which
// keep the matrix pipe busy (a 256-column form on v_mfma_f64_16x16x4_f64 measured 12 us in the pipelined
// step where k_pn_fold_t2 takes 5.4).  Nothing is kept between launches.
__global__ void __launch_bounds__(1024) k_pn_fold_seg(const float* __restrict__ w1f, int w1_stride,
                                                      const float* __restrict__ b1, const float* __restrict__ t2,
                                                      int t2_ld, float* __restrict__ outf, float* __restrict__ outb,
                                                      const float* __restrict__ s1aT, const float* __restrict__ s1b,
                                                      int N2, float* __restrict__ wd, int64_t wd_stride,
                                                      float* __restrict__ bd, int64_t bd_stride) {
  const int b = blockIdx.y, c0 = 64 * blockIdx.x, e = threadIdx.x;
  __shared__ float s_w[13 * 64];   // rows 0..11 W1'^T (row-major [k][n]), row 12 the bias
  __shared__ float s_t[64 * 64];
  __shared__ double s_s[64 * 64];  // s1a^T[i][c0 + c]
  __shared__ double s_o[13 * 64];  // [W1''; b1''] as stored (fp32 values)
  const int r = e >> 6, n = e & 63;
  const float sb = e < 13 * 64 ? s1b[c0 + n] : 0.0f;
  {
    const float* wb = w1f + (int64_t)b * w1_stride;
    {  // fragment-major element e -> (k, n)
      const int cb = e >> 8, ln = (e >> 2) & 63, k = 4 * (ln >> 4) + (e & 3), nn = 16 * cb + (ln & 15);
      const float v = wb[e];
      if (k < 12) s_w[k * 64 + nn] = v;
    }
    if (e < 64) s_w[12 * 64 + e] = b1[e];
    reinterpret_cast<f32x4*>(s_t)[e] = reinterpret_cast<const f32x4*>(t2 + (int64_t)b * t2_ld)[e];
    const f32x4 sv = *reinterpret_cast<const f32x4*>(s1aT + (int64_t)(e >> 4) * N2 + c0 + 4 * (e & 15));
#pragma unroll
    for (int j = 0; j < 4; j++) s_s[4 * e + j] = (double)sv[j];
  }
  __syncthreads();
  if (e < 13 * 64) {
    float acc = 0.0f;
#pragma unroll 16
    for (int i = 0; i < 64; i++) acc = fmaf(s_w[r * 64 + i], s_t[i * 64 + n], acc);
    s_o[e] = (double)acc;
    if (blockIdx.x == 0) {
      if (r < 12) outf[(int64_t)b * 1024 + ((((n >> 4) * 64 + ((r >> 2) & 3) * 16 + (n & 15)) << 2) + (r & 3))] = acc;
      else outb[(int64_t)b * 64 + n] = acc;
    }
  }
  __syncthreads();
  if (e < 13 * 64) {
    double acc = 0.0;
#pragma unroll 16
    for (int i = 0; i < 64; i++) acc = fma(s_o[r * 64 + i], s_s[i * 64 + n], acc);
    const int col = c0 + n;
    if (r < 12) wd[(int64_t)b * wd_stride + ((((col >> 4) * 64 + ((r >> 2) & 3) * 16 + (col & 15)) << 2) + (r & 3))] = (float)acc;
    else bd[(int64_t)b * bd_stride + col] = (float)(acc + (double)sb);
  }
}

#if NDNET_PN_TILE == 64
// ---- chain C as one per-cloud 12 -> F layer (ndnet_pn_pool12_run) ----
// NDTNet's conv1 (with t1, t2 folded), conv2 and conv3 have no ReLU between
// them (ndtnet.py:149-161), so the pooled feature is
//   g3[b][f] = max_n (sum_k x[b][n][k] Wc[b][k][f]) + bc[b][f],
//   [Wc[b]; bc[b]] = [W0''[b]; b0''[b]] W2'^T W3'^T  (+ b2' W3'^T + b3' on the bias row)
// -- 12 multiply-adds per point and column where the layered chain does 64
// into 128 and 128 into F.  One workgroup per 64 columns of one cloud:
//   phase 1  its 13 x 64 slice of [Wc; bc], the bias carried as row 12 (as
//            k_pn_fold_t2 does), on the f64 MFMA from the live folded tensors
//            (they are re-folded in place after a weight update: no product
//            of them is kept anywhere), rounded once to fp32;
//   phase 2  the cloud's rows in 16-point tiles dealt to the 16 waves, a tile
//            times the slice as three v_mfma_f32_16x16x4_f32 per 16 columns
//            (fp32 FMAs, k ascending), a running fmaxf per lane from -inf,
//            one reduction over the lane rows (DPP) and the waves (LDS), the
//            bias added to the maximum (fl(a + b) is monotonic in a, as
//            pool_cols relies on), one plain store per column.
// A row with a NaN or an infinity takes no part in the maximum: chain C's
// split-bf16 layers turn an infinite layer-0 output into NaN planes, and
// fmaxf drops the NaNs.  The rows past the cloud's last point enter as NaN
// rows, dropped the same way.
typedef double f64x4 __attribute__((ext_vector_type(4)));
constexpr int kP12Waves = 16;
constexpr int kP12Pre = 4;     // tiles per wave whose rows are loaded ahead of phase 1 (all of them up to 1024 points)
constexpr int kP12Pitch = 130; // doubles per row of the 13 x 128 intermediate: phase 1's column reads spread over the banks

// this lane's part of tile `tile`: point 16 tile + cl, columns 4 s + kq.  Loads only (no branch, nothing
// that waits for them): a lane past the cloud's last point reads the last row, which p12_clean drops
__device__ inline void p12_rows(const float* __restrict__ xb, int x_ld, int n, int tile, int kq, int cl, float (&v)[3]) {
  const int p = min(16 * tile + cl, n - 1);
  const float* r = xb + (int64_t)p * x_ld + kq;
#pragma unroll
  for (int s = 0; s < 3; s++) v[s] = r[4 * s];
}

// ... and what enters the products: NaN for a lane past the cloud and for a NaN or an infinity
__device__ inline void p12_clean(int n, int tile, int cl, float (&v)[3]) {
  const bool in = 16 * tile + cl < n;
#pragma unroll
  for (int s = 0; s < 3; s++) v[s] = (in & (fabsf(v[s]) < INFINITY)) ? v[s] : NAN;  // & : one select, no branch
}

// kTail: phase 1 from the composed tail (ndnet_pn_pool12_tail_run) -- w23 = W2'^T W3'^T (64 x Fp doubles) and
// its bias row b23 = b2' W3'^T + b3', both outputs of the fold's job table, so the slice is the one product
// [W0''; b0''] (13 x 64) w23[:, c0 .. c0 + 64): waves 0..3, one on each SIMD, 16 columns and 16 MFMAs each on
// four independent accumulators.  That is a quarter of the layered product's MFMAs per SIMD, and neither the
// 13 x 128 intermediate nor its barrier.  w_mid, b_mid, w_tail, b_tail are then not read.
template <bool kTail>
__global__ void __launch_bounds__(kP12Waves * 64) k_pn_pool12(
    const float* __restrict__ x, int x_ld, int n, const float* __restrict__ w0f, int64_t w0_stride,
    const float* __restrict__ b0, int64_t b0_stride, const float* __restrict__ w_mid,
    const float* __restrict__ b_mid, const float* __restrict__ w_tail, const float* __restrict__ b_tail,
    const double* __restrict__ w23, const double* __restrict__ b23, int Fp, float* __restrict__ gmax, int gmax_ld) {
  __shared__ double s_m[kTail ? 1 : 13 * kP12Pitch];  // [W0''; b0''] W2'^T (+ b2' on row 12)
  __shared__ float s_wc[13 * 64];            // this workgroup's columns of [Wc; bc]
  __shared__ float s_red[kP12Waves * 64];
  const int b = blockIdx.y, c0 = 64 * blockIdx.x;
  const int lane = threadIdx.x & 63, kq = lane >> 4, cl = lane & 15;
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int tiles = (n + 15) >> 4;
  const float* xb = x + (int64_t)b * n * x_ld;

  // the first tiles' rows and phase 1's operands: every load of the kernel's first half in flight at once
  float xp[kP12Pre][3];
#pragma unroll
  for (int i = 0; i < kP12Pre; i++) p12_rows(xb, x_ld, n, wave + kP12Waves * i, kq, cl, xp[i]);
  float tw[32];  // waves 8..11 (phase 1b): W3'^T[4 ks + kq][c0 + 16 (wave - 8) + cl]

  if constexpr (kTail) {
    // phase 1, waves 0..3: A = [W0''; b0''] (row cl of 16, 13 used) as phase 1a reads it, B = w23's column
    // c0 + 16 wave + cl; v_mfma_f64_16x16x4_f64 leaves row kq + 4 q, column cl in element q
    if (wave < 4) {
      const float* wb = w0f + (int64_t)b * w0_stride;
      const float* bb = b0 + (int64_t)b * b0_stride;
      const int tc = min(c0 + 16 * wave + cl, Fp - 1);  // Fp = 32: the upper half's columns are never stored
      float a[16];
      double bw[16];
#pragma unroll
      for (int ks = 0; ks < 16; ks++) {
        const int i = 4 * ks + kq;
        const float* src = cl < 12 ? wb + ((((i >> 4) * 64 + ((cl >> 2) & 3) * 16 + (i & 15)) << 2) + (cl & 3)) : bb + i;
        a[ks] = *src;  // rows 13..15 read the bias too and are zeroed below: one load, no branch
        bw[ks] = w23[(int64_t)i * Fp + tc];
      }
      const double brow = b23[tc];
#pragma unroll
      for (int ks = 0; ks < 16; ks++) a[ks] = cl < 13 ? a[ks] : 0.0f;
      f64x4 acc[4];
#pragma unroll
      for (int j = 0; j < 4; j++) acc[j] = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int ks = 0; ks < 16; ks++)
        acc[ks & 3] = __builtin_amdgcn_mfma_f64_16x16x4f64((double)a[ks], bw[ks], acc[ks & 3], 0, 0, 0);
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int row = kq + 4 * q, col = 16 * wave + cl;
        double v = (acc[0][q] + acc[1][q]) + (acc[2][q] + acc[3][q]);
        if (row == 12) v += brow;
        if (row < 13) s_wc[row * 64 + col] = (float)v;
      }
    }
  } else {
  // phase 1a, waves 0..7, 16 columns of the intermediate each: A = [W0''; b0''] (row cl of 16, 13 used),
  // B = W2'^T; v_mfma_f64_16x16x4_f64 leaves row kq + 4 q, column cl in element q
  if (wave < 8) {
    const float* wb = w0f + (int64_t)b * w0_stride;
    const float* bb = b0 + (int64_t)b * b0_stride;
    float a[16], bw[16];
#pragma unroll
    for (int ks = 0; ks < 16; ks++) {
      const int i = 4 * ks + kq;  // conv1's output channel: W0'' is fragment-major with K = 16 (k_pn_fold_t2)
      const float* src = cl < 12 ? wb + ((((i >> 4) * 64 + ((cl >> 2) & 3) * 16 + (i & 15)) << 2) + (cl & 3)) : bb + i;
      a[ks] = *src;  // rows 13..15 read the bias too and are zeroed below: one load, no branch
      bw[ks] = w_mid[i * 128 + 16 * wave + cl];
    }
#pragma unroll
    for (int ks = 0; ks < 16; ks++) a[ks] = cl < 13 ? a[ks] : 0.0f;
    f64x4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int ks = 0; ks < 16; ks += 2) {
      acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64((double)a[ks], (double)bw[ks], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64((double)a[ks + 1], (double)bw[ks + 1], acc1, 0, 0, 0);
    }
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int row = kq + 4 * q, col = 16 * wave + cl;
      double v = acc0[q] + acc1[q];
      if (row == 12) v += (double)b_mid[col];
      if (row < 13) s_m[row * kP12Pitch + col] = v;
    }
  } else if (wave < 12) {
    const int tc = min(c0 + 16 * (wave - 8) + cl, Fp - 1);  // Fp = 32: the upper half's columns are never stored
#pragma unroll
    for (int ks = 0; ks < 32; ks++) tw[ks] = w_tail[(int64_t)(4 * ks + kq) * Fp + tc];
  }
  __syncthreads();
  // phase 1b, waves 8..11 (idle in 1a, so their operands are already here), 16 of the workgroup's columns
  // each: A = the intermediate, B = W3'^T
  if (wave >= 8 && wave < 12) {
    f64x4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int ks = 0; ks < 32; ks += 2) {
      const double a0 = s_m[min(cl, 12) * kP12Pitch + 4 * ks + kq], a1 = s_m[min(cl, 12) * kP12Pitch + 4 * ks + 4 + kq];
      acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(cl < 13 ? a0 : 0.0, (double)tw[ks], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(cl < 13 ? a1 : 0.0, (double)tw[ks + 1], acc1, 0, 0, 0);
    }
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int row = kq + 4 * q, col = 16 * (wave - 8) + cl;
      double v = acc0[q] + acc1[q];
      if (row == 12) v += (double)b_tail[min(c0 + col, Fp - 1)];
      if (row < 13) s_wc[row * 64 + col] = (float)v;
    }
  }
  }  // !kTail
  __syncthreads();

  // phase 2: A = the slice (lane (kq, cl): row 4 s + kq, column 16 cb + cl), B = the tile's rows;
  // lane (kq, cl) gets point cl, columns 16 cb + 4 kq + r
  float wc[4][3];
#pragma unroll
  for (int cb = 0; cb < 4; cb++)
#pragma unroll
    for (int s = 0; s < 3; s++) wc[cb][s] = s_wc[(4 * s + kq) * 64 + 16 * cb + cl];
  float m[4][4];
#pragma unroll
  for (int cb = 0; cb < 4; cb++)
#pragma unroll
    for (int r = 0; r < 4; r++) m[cb][r] = -INFINITY;
  auto tile = [&](int t, float (&xv)[3]) {
    p12_clean(n, t, cl, xv);
    f32x4 acc[4];
#pragma unroll
    for (int cb = 0; cb < 4; cb++) acc[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < 3; s++)  // four independent accumulators per k step
#pragma unroll
      for (int cb = 0; cb < 4; cb++) acc[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(wc[cb][s], xv[s], acc[cb], 0, 0, 0);
#pragma unroll
    for (int cb = 0; cb < 4; cb++)
#pragma unroll
      for (int r = 0; r < 4; r++) m[cb][r] = fmaxf(m[cb][r], acc[cb][r]);
  };
#pragma unroll
  for (int i = 0; i < kP12Pre; i++)
    if (wave + kP12Waves * i < tiles) tile(wave + kP12Waves * i, xp[i]);
  for (int t = wave + kP12Waves * kP12Pre; t < tiles; t += kP12Waves) {
    float xv[3];
    p12_rows(xb, x_ld, n, t, kq, cl, xv);
    tile(t, xv);
  }
  // the maximum over the 16 points of a lane row (DPP), halving the values a lane carries at every step:
  // after xor 8, 4, 2, 1 lane cl is left with value 4 cb + r = cl of the 16, i.e. column 16 (cl >> 2) + 4 kq + (cl & 3)
  float* mv = &m[0][0];
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const bool hi = cl & 8;
    mv[i] = fmaxf(hi ? mv[i + 8] : mv[i], xor_row<8>(hi ? mv[i] : mv[i + 8]));
  }
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const bool hi = cl & 4;
    mv[i] = fmaxf(hi ? mv[i + 4] : mv[i], xor_row<4>(hi ? mv[i] : mv[i + 4]));
  }
#pragma unroll
  for (int i = 0; i < 2; i++) {
    const bool hi = cl & 2;
    mv[i] = fmaxf(hi ? mv[i + 2] : mv[i], xor_row<2>(hi ? mv[i] : mv[i + 2]));
  }
  {
    const bool hi = cl & 1;
    mv[0] = fmaxf(hi ? mv[1] : mv[0], xor_row<1>(hi ? mv[0] : mv[1]));
  }
  s_red[wave * 64 + 16 * (cl >> 2) + 4 * kq + (cl & 3)] = mv[0];
  __syncthreads();
  if (threadIdx.x < 64) {
    const int c = threadIdx.x;
    float mm = s_red[c];
#pragma unroll
    for (int w = 1; w < kP12Waves; w++) mm = fmaxf(mm, s_red[w * 64 + c]);
    // as pool_cols + atomic_max_f32: a column no row reached stays -inf, -0 becomes +0
    if (c0 + c < Fp) gmax[(int64_t)b * gmax_ld + c0 + c] = mm > -INFINITY ? (mm + s_wc[12 * 64 + c]) + 0.0f : -INFINITY;
  }
}
#endif

// TNet(3) tail: t1[b] = fc3(h2[b]) (+ I, folded into the bias) and the t1
// fold of conv1, W1'^T[b] = t1[b] (1 x 9) @ basis (9 x kin*nout), written
// fragment-major with K padded to 16 (rows kin..15 zero).  One workgroup per cloud.
__global__ void __launch_bounds__(256) k_pn_head3(const float* __restrict__ h2, int ld_h, const float* __restrict__ W3,
                                                  const float* __restrict__ b3, const float* __restrict__ basis,
                                                  float* __restrict__ t1_out, float* __restrict__ w1f, int K, int kin,
                                                  int nout) {
  __shared__ float s_t[9];
  const int b = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* h = h2 + (int64_t)b * ld_h;
  for (int o = wave; o < 9; o += 4) {  // one wave per output, lanes split K
    float acc = 0.0f;
    for (int k = lane; k < K; k += 64) acc += h[k] * W3[(int64_t)o * K + k];
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if (lane == 0) {
      s_t[o] = acc + b3[o];
      t1_out[b * 9 + o] = acc + b3[o];
    }
  }
  const int M = kin * nout, total = 16 * nout;  // one k-group
  // fragment-major position e -> (k, n); the first kE positions of every
  // thread have their basis values loaded before the barrier, behind fc3
  auto kn = [&](int e, int& k, int& n) {
    const int cb = e >> 8, ln = (e >> 2) & 63;
    k = 4 * (ln >> 4) + (e & 3);
    n = 16 * cb + (ln & 15);
  };
  constexpr int kE = 4;
  float bas[kE][9];
#pragma unroll
  for (int i = 0; i < kE; i++) {
    const int e = threadIdx.x + i * blockDim.x;
    int k, n;
    kn(e, k, n);
#pragma unroll
    for (int a = 0; a < 9; a++) bas[i][a] = (e < total && k < kin) ? basis[a * M + k * nout + n] : 0.0f;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < kE; i++) {
    const int e = threadIdx.x + i * blockDim.x;
    if (e < total) {
      float acc = 0.0f;
#pragma unroll
      for (int a = 0; a < 9; a++) acc += s_t[a] * bas[i][a];
      w1f[(int64_t)b * total + e] = acc;
    }
  }
  for (int e = threadIdx.x + kE * blockDim.x; e < total; e += blockDim.x) {
    int k, n;
    kn(e, k, n);
    float acc = 0.0f;
    if (k < kin) {
#pragma unroll
      for (int a = 0; a < 9; a++) acc += s_t[a] * basis[a * M + k * nout + n];
    }
    w1f[(int64_t)b * total + e] = acc;
  }
}

#if NDNET_PN_TILE == 64
// ---- the BatchNorm fold, in place (ndnet_pn_fold_run, include/ndnet_pointnet.h) ----
// HBM-bound copy work (~14 MB read, ~40 MB written for the F = 1024 model):
// each thread writes one unit (4 fp32 of a fragment, 8 bf16 of each split
// plane, else one float), so every output row is written with full-width,
// contiguous stores; the strided weight reads hit L2.
constexpr int kFoldThreads = 256;

__device__ inline uint16_t fold_bf16(float x) {  // torch's float -> bfloat16: round to nearest even
  uint32_t u = __float_as_uint(x);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);
  return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

template <class Job>
__device__ inline float fold_w(const Job& J, int n, int k) {
#pragma clang fp contract(off)
  if (n >= J.N || k >= J.K) return 0.0f;
  const float w = J.w[(int64_t)n * J.ld + J.k0 + k];
  if (!J.gamma) return w;
  return w * (J.gamma[n] / sqrtf(J.var[n] + J.eps));  // pointnet_hip._bn_fold, operation by operation
}

__host__ __device__ inline int64_t fold_units(const ndnet_pn_fold_job& J) {
  switch (J.kind) {
    case NDNET_FOLD_WT: return (int64_t)J.Kp * J.Np;
    case NDNET_FOLD_FRAG: return (int64_t)J.Kp * J.Np / 4;
    case NDNET_FOLD_FRAG6: return (int64_t)J.Kp * J.Np / 8;
    case NDNET_FOLD_ROWS: return (int64_t)J.N * J.K;
    case NDNET_FOLD_BASIS: return (int64_t)9 * J.K * J.N;
    case NDNET_FOLD_PROD: return (int64_t)J.N * J.Np;
    default: return J.Np;
  }
}

// block_base: the launch's first block of the list.  The product jobs read other jobs' outputs, so they are
// the list's last blocks and run as a second launch behind the first (ndnet_pn_fold_run).
__global__ void __launch_bounds__(kFoldThreads) k_pn_fold(const ndnet_pn_fold_job* __restrict__ jobs, int num_jobs,
                                                          int64_t block_base) {
#pragma clang fp contract(off)
  const int64_t blk = block_base + blockIdx.x;
  int j = 0;  // this workgroup's job: the last one starting at or before it (block0 ascends)
  for (int i = 1; i < num_jobs; i++)
    if (jobs[i].block0 <= blk) j = i;
  const ndnet_pn_fold_job J = jobs[j];
  const int64_t u = (blk - J.block0) * kFoldThreads + threadIdx.x;
  if (u >= fold_units(J)) return;
  switch (J.kind) {
    case NDNET_FOLD_WT: {
      const int n = (int)(u % J.Np), k = (int)(u / J.Np);
      static_cast<float*>(J.out)[u] = fold_w(J, n, k);
      break;
    }
    case NDNET_FOLD_FRAG: {  // [cb][kg][kq][cl][s]: k = 16 kg + 4 kq + s, n = 16 cb + cl
      const int kgs = J.Kp / 16;
      const int cl = (int)(u % 16), kq = (int)(u / 16 % 4), kg = (int)(u / 64 % kgs), cb = (int)(u / (64 * kgs));
      const int k = 16 * kg + 4 * kq, n = 16 * cb + cl;
      f32x4 v = {fold_w(J, n, k), fold_w(J, n, k + 1), fold_w(J, n, k + 2), fold_w(J, n, k + 3)};
      reinterpret_cast<f32x4*>(J.out)[u] = v;
      break;
    }
    case NDNET_FOLD_FRAG6: {  // [cb][kg][plane][kq][cl][j]: k = 32 kg + 8 kq + j, n = 16 cb + cl
      const int kgs = J.Kp / 32;
      const int cl = (int)(u % 16), kq = (int)(u / 16 % 4), kg = (int)(u / 64 % kgs), cb = (int)(u / (64 * kgs));
      const int k = 32 * kg + 8 * kq, n = 16 * cb + cl;
      uint32_t p[3][4];
#pragma unroll
      for (int t = 0; t < 8; t += 2) {
        uint16_t hv[2], mv[2], lv[2];
#pragma unroll
        for (int e = 0; e < 2; e++) {
          const float w = fold_w(J, n, k + t + e);
          hv[e] = fold_bf16(w);
          const float r = w - __uint_as_float((uint32_t)hv[e] << 16);
          mv[e] = fold_bf16(r);
          lv[e] = fold_bf16(r - __uint_as_float((uint32_t)mv[e] << 16));
        }
        p[0][t / 2] = hv[0] | ((uint32_t)hv[1] << 16);
        p[1][t / 2] = mv[0] | ((uint32_t)mv[1] << 16);
        p[2][t / 2] = lv[0] | ((uint32_t)lv[1] << 16);
      }
      const int64_t unit = u % 64 + (u / 64) * 192;  // 64 units per (cb, kg), three planes of them
      uint4* o = reinterpret_cast<uint4*>(J.out);
#pragma unroll
      for (int pl = 0; pl < 3; pl++) o[unit + 64 * pl] = make_uint4(p[pl][0], p[pl][1], p[pl][2], p[pl][3]);
      break;
    }
    case NDNET_FOLD_ROWS: {
      const int n = (int)(u / J.K), k = (int)(u % J.K);
      static_cast<float*>(J.out)[u] = fold_w(J, n, k);
      break;
    }
    case NDNET_FOLD_BASIS: {  // out[3a + c][r][n]: r < 3 the point (t1 p), else the covariance rows (t1 C)
      const int n = (int)(u % J.N), r = (int)(u / J.N % J.K), ac = (int)(u / ((int64_t)J.N * J.K));
      const int a = ac / 3, c = ac % 3;
      float v = 0.0f;
      if (r < 3) {
        if (r == c) v = fold_w(J, n, a);
      } else if ((r - 3) / 3 == c) {
        v = fold_w(J, n, 3 + 3 * a + (r - 3) % 3);
      }
      static_cast<float*>(J.out)[u] = v;
      break;
    }
    case NDNET_FOLD_PROD: {  // out[r][n] = sum_k w[r][k] rhs[k][n] (+ bias[n]): double, k ascending, rounded at the store
      const int n = (int)(u % J.Np), r = (int)(u / J.Np);
      const float* a = J.w + (int64_t)r * J.ld + J.k0;
      double acc = 0.0;
      for (int k = 0; k < J.K; k++) acc += (double)a[k] * (double)J.rhs[(int64_t)k * J.Np + n];  // the product is exact
      if (J.bias) acc += (double)J.bias[n];
      if (J.out_f64) static_cast<double*>(J.out)[u] = acc;
      else static_cast<float*>(J.out)[u] = (float)acc;
      break;
    }
    default: {  // NDNET_FOLD_BIAS
      const int n = (int)u;
      float v = 0.0f;
      if (n < J.N) {
        v = J.bias[n];
        if (J.gamma) v = (v - J.mean[n]) * (J.gamma[n] / sqrtf(J.var[n] + J.eps)) + J.beta[n];
        if (J.eye > 0) v = v + (n / J.eye == n % J.eye ? 1.0f : 0.0f);
      }
      static_cast<float*>(J.out)[u] = v;
    }
  }
}

// ---- the fp16 planes of a split layer (ndnet_pn_fold16_run, include/ndnet_pointnet.h) ----
// Launch 1: the maximum of |fw| over part blockIdx.x of kFold16Parts interleaved parts of job blockIdx.y's
// layer (fmaxf: a NaN weight takes no part), one float each -- no atomics, so nothing to zero between folds.
constexpr int kFold16Parts = 16;

__global__ void __launch_bounds__(kFoldThreads) k_pn_fold16_max(const ndnet_pn_fold16_job* __restrict__ jobs) {
#pragma clang fp contract(off)
  __shared__ float s_m[kFoldThreads];
  const ndnet_pn_fold16_job J = jobs[blockIdx.y];
  const int64_t total = (int64_t)J.N * J.K;
  float m = 0.0f;
  for (int64_t e = (int64_t)blockIdx.x * kFoldThreads + threadIdx.x; e < total; e += (int64_t)kFold16Parts * kFoldThreads)
    m = fmaxf(m, fabsf(fold_w(J, (int)(e / J.K), (int)(e % J.K))));
  s_m[threadIdx.x] = m;
  __syncthreads();
  for (int o = kFoldThreads / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) s_m[threadIdx.x] = fmaxf(s_m[threadIdx.x], s_m[threadIdx.x + o]);
    __syncthreads();
  }
  if (threadIdx.x == 0) J.partial[blockIdx.x] = s_m[0];
}

// The layer's exponent s from its maximum: max 2^s in [2^13, 2^14); 0 for a zero or non-finite maximum.  Any
// finite maximum has s >= -114, which 2^s and 2^-s both hold; s stops at 100 (a maximum below 2^-87 then
// lands under 2^13: fewer bits of weights that small, never an overflow).
__device__ inline int fold16_exp(float m) {
  if (!(m > 0.0f) || !(m < INFINITY)) return 0;
  const int s = 13 - ilogbf(m);
  return s > 100 ? 100 : s;
}

// Launch 2: one thread per 8 consecutive k of one column -- 16 bytes of each plane, as NDNET_FOLD_FRAG6's
// units, [cb][kg][plane][kq][cl][j] with two planes; the job's first thread stores 2^-s.
__global__ void __launch_bounds__(kFoldThreads) k_pn_fold16_frag(const ndnet_pn_fold16_job* __restrict__ jobs) {
#pragma clang fp contract(off)
  const ndnet_pn_fold16_job J = jobs[blockIdx.y];
  const int64_t u = (int64_t)blockIdx.x * kFoldThreads + threadIdx.x;
  if (u >= (int64_t)J.Kp * J.Np / 8) return;
  float m = 0.0f;
#pragma unroll
  for (int i = 0; i < kFold16Parts; i++) m = fmaxf(m, J.partial[i]);
  const int s = fold16_exp(m);
  const float up = ldexpf(1.0f, s);
  if (u == 0) *J.scale = ldexpf(1.0f, -s);
  const int kgs = J.Kp / 32;
  const int cl = (int)(u % 16), kq = (int)(u / 16 % 4), kg = (int)(u / 64 % kgs), cb = (int)(u / (64 * kgs));
  const int k = 32 * kg + 8 * kq, n = 16 * cb + cl;
  f16x8 h8, l8;
#pragma unroll
  for (int t = 0; t < 8; t++) {
    const float x = fold_w(J, n, k + t) * up;  // exact but for an underflow far below the layer's maximum
    const _Float16 h = (_Float16)x;            // round to nearest even, as the activations' split
    h8[t] = h;
    l8[t] = (_Float16)(x - (float)h);
  }
  const int64_t unit = u % 64 + (u / 64) * 128;  // 64 units per (cb, kg), two planes of them
  f16x8* o = reinterpret_cast<f16x8*>(J.out);
  o[unit] = h8;
  o[unit + 64] = l8;
}
#endif

#if NDNET_PN_TILE == 64
int fc_mfma_cbw(int nb, int ngmax) {
  static const int cap = [] {
    const char* e = getenv("NDNET_PN_FC_CBW");
    return e ? atoi(e) : 4;
  }();
  for (int c = cap >= 4 ? 4 : cap >= 2 ? 2 : 1; c > 1; c >>= 1)
    if (nb % c == 0 && nb / c >= 32 && ngmax * c <= kFcMaxG) return c;
  return 1;
}
#endif

}  // namespace

extern "C" {

#if NDNET_PN_TILE == 64  // the 32-point build exports only its chain entry point (below)
int ndnet_pn_fc_mfma_bias_run(const float* in, int ld_in, const float* Wf, const float* bias, int bias_ld, float* out,
                              int ld_out, int batch, int K, int N, int relu, void* stream) {
  if (!in || !Wf || !bias || !out || batch <= 0 || batch > 16 || K <= 0 || K % 16 || K > 16 * kFcWaves * kFcMaxG ||
      N <= 0 || N % 16 || ld_in % 4 || ld_in < K || ld_out < N || ((uintptr_t)in | (uintptr_t)Wf) % 16 ||
      (bias_ld != 0 && bias_ld < N))
    return -20;
  const int KG = K / 16, nb = N / 16, ngmax = (KG + kFcWaves - 1) / kFcWaves;
  // column blocks per workgroup: 4 while that keeps >= 32 workgroups and the
  // fragments fit (fc_mfma_cbw; NDNET_PN_FC_CBW=1 restores one block each)
  const int cbw = fc_mfma_cbw(nb, ngmax);
  const f32x4* wf = reinterpret_cast<const f32x4*>(Wf);
  hipStream_t st = (hipStream_t)stream;
  if (cbw == 4)
    k_pn_fc_mfma<4><<<nb / 4, kFcWaves * 64, 0, st>>>(in, ld_in, wf, bias, bias_ld, out, ld_out, batch, KG, relu);
  else if (cbw == 2)
    k_pn_fc_mfma<2><<<nb / 2, kFcWaves * 64, 0, st>>>(in, ld_in, wf, bias, bias_ld, out, ld_out, batch, KG, relu);
  else
    k_pn_fc_mfma<1><<<nb, kFcWaves * 64, 0, st>>>(in, ld_in, wf, bias, bias_ld, out, ld_out, batch, KG, relu);
  return hipGetLastError() == hipSuccess ? 0 : -21;
}

int ndnet_pn_fc_mfma_run(const float* in, int ld_in, const float* Wf, const float* bias, float* out, int ld_out,
                         int batch, int K, int N, int relu, void* stream) {
  return ndnet_pn_fc_mfma_bias_run(in, ld_in, Wf, bias, 0, out, ld_out, batch, K, N, relu, stream);
}

int ndnet_pn_cls_head_run(const float* in, int ld_in, const float* Wf, const float* bias, float* probs, int ld_probs,
                          float* logits, int ld_logits, int batch, int K, int N, int out_cols, float* clear,
                          int64_t clear_count, void* stream) {
  if (!in || !Wf || !bias || !probs || batch <= 0 || K <= 0 || K % 16 || K > 16 * kClsMaxG || N <= 0 || N % 16 ||
      N > 1024 || out_cols < 1 || out_cols > N || ld_in % 4 || ld_in < K || ld_probs < out_cols ||
      (logits && ld_logits < out_cols) || ((uintptr_t)in | (uintptr_t)Wf) % 16 || clear_count < 0 ||
      (!clear && clear_count))
    return -20;
  k_pn_cls_head<<<(batch + 15) / 16, kClsWaves * 64, (size_t)16 * N * sizeof(float), (hipStream_t)stream>>>(
      in, ld_in, reinterpret_cast<const f32x4*>(Wf), bias, probs, ld_probs, logits, ld_logits, batch, K / 16, N,
      out_cols, clear, clear_count);
  return hipGetLastError() == hipSuccess ? 0 : -21;
}

int ndnet_pn_fc_run(const float* in, int ld_in, const float* W, const float* bias, float* out, int ld_out, int batch,
                    int K, int N, int relu, void* stream) {
  if (!in || !W || !bias || !out || batch <= 0 || batch > 16 || K <= 0 || K % 4 || N <= 0 || ld_in % 4 ||
      ld_in < K || ld_out < N || ((uintptr_t)in | (uintptr_t)W) % 16)
    return -20;
  hipStream_t st = (hipStream_t)stream;
  switch (K % 256 == 0 && K <= 1024 ? K / 256 : 0) {
    case 2: k_pn_fc_split<2><<<(N + 1) / 2, 256, 0, st>>>(in, ld_in, W, bias, out, ld_out, batch, N, relu); break;
    case 4: k_pn_fc_split<4><<<N, 256, 0, st>>>(in, ld_in, W, bias, out, ld_out, batch, N, relu); break;
    default: k_pn_fc<<<(N + 3) / 4, 256, 0, st>>>(in, ld_in, W, bias, out, ld_out, batch, K, N, relu);
  }
  return hipGetLastError() == hipSuccess ? 0 : -21;
}

int ndnet_pn_head3_run(const float* h2, int ld_h, const float* W3, const float* b3, const float* basis, float* t1,
                       float* w1f, int batch, int K, int kin, int nout, void* stream) {
  if (!h2 || !W3 || !b3 || !basis || !t1 || !w1f || batch <= 0 || K <= 0 || ld_h < K || kin <= 0 || kin > 16 ||
      nout <= 0 || nout % 16)
    return -20;
  k_pn_head3<<<batch, 256, 0, (hipStream_t)stream>>>(h2, ld_h, W3, b3, basis, t1, w1f, K, kin, nout);
  return hipGetLastError() == hipSuccess ? 0 : -21;
}

int ndnet_pn_fold_t2_run(const float* w1f, int w1_stride, const float* b1, const float* t2, int t2_ld, float* outf,
                         float* outb, int batch, void* stream) {
  if (!w1f || !b1 || !t2 || !outf || !outb || batch <= 0 || w1_stride < 1024 || t2_ld < 4096 || t2_ld % 4 ||
      (uintptr_t)t2 % 16)
    return -20;
  k_pn_fold_t2<<<batch, 1024, 0, (hipStream_t)stream>>>(w1f, w1_stride, b1, t2, t2_ld, outf, outb);
  return hipGetLastError() == hipSuccess ? 0 : -21;
}

int ndnet_pn_fold_seg_run(const float* w1f, int w1_stride, const float* b1, const float* t2, int t2_ld, float* outf,
                          float* outb, const float* s1aT, const float* s1b, int N2, float* wd, int64_t wd_stride,
                          float* bd, int64_t bd_stride, int batch, void* stream) {
  if (!w1f || !b1 || !t2 || !outf || !outb || !s1aT || !s1b || !wd || !bd || batch <= 0 || batch > 65535 ||
      w1_stride < 1024 || t2_ld < 4096 || t2_ld % 4 || (uintptr_t)t2 % 16 || N2 <= 0 || N2 % 64 ||
      (uintptr_t)s1aT % 16 || wd_stride < 16 * (int64_t)N2 || bd_stride < N2)
    return -20;
  k_pn_fold_seg<<<dim3(N2 / 64, batch), 1024, 0, (hipStream_t)stream>>>(w1f, w1_stride, b1, t2, t2_ld, outf, outb, s1aT,
                                                                        s1b, N2, wd, wd_stride, bd, bd_stride);
  return hipGetLastError() == hipSuccess ? 0 : -21;
}

int ndnet_pn_pool12_run(const float* x, int x_ld, int num_points, const float* w0f, int64_t w0_stride, const float* b0,
                        int64_t b0_stride, const float* w_mid, const float* b_mid, const float* w_tail,
                        const float* b_tail, int F, int Fp, float* gmax, int gmax_ld, int batch, void* stream) {
  if (!x || !w0f || !b0 || !w_mid || !b_mid || !w_tail || !b_tail || !gmax || batch <= 0 || batch > 65535 ||
      num_points <= 0 || x_ld < 12 || x_ld % 4 || w0_stride < 1024 || b0_stride < 64 || F <= 0 || F > Fp ||
      (Fp != 32 && Fp % 64) || gmax_ld < Fp)
    return -20;
  k_pn_pool12<false><<<dim3((Fp + 63) / 64, batch), kP12Waves * 64, 0, (hipStream_t)stream>>>(
      x, x_ld, num_points, w0f, w0_stride, b0, b0_stride, w_mid, b_mid, w_tail, b_tail, nullptr, nullptr, Fp, gmax,
      gmax_ld);
  return hipGetLastError() == hipSuccess ? 0 : -21;
}

int ndnet_pn_pool12_tail_run(const float* x, int x_ld, int num_points, const float* w0f, int64_t w0_stride,
                             const float* b0, int64_t b0_stride, const double* w23, const double* b23, int Fp,
                             float* gmax, int gmax_ld, int batch, void* stream) {
  if (!x || !w0f || !b0 || !w23 || !b23 || !gmax || batch <= 0 || batch > 65535 || num_points <= 0 || x_ld < 12 ||
      x_ld % 4 || w0_stride < 1024 || b0_stride < 64 || Fp <= 0 || (Fp != 32 && Fp % 64) || gmax_ld < Fp ||
      ((uintptr_t)w23 | (uintptr_t)b23) % 8)
    return -20;
  k_pn_pool12<true><<<dim3((Fp + 63) / 64, batch), kP12Waves * 64, 0, (hipStream_t)stream>>>(
      x, x_ld, num_points, w0f, w0_stride, b0, b0_stride, nullptr, nullptr, nullptr, nullptr, w23, b23, Fp, gmax,
      gmax_ld);
  return hipGetLastError() == hipSuccess ? 0 : -21;
}

int ndnet_pn_fold_prepare(ndnet_pn_fold_job* jobs, int num_jobs, int64_t* num_blocks) {
  if (!jobs || num_jobs <= 0 || !num_blocks) return -20;
  int64_t blocks = 0, prod0 = -1;  // prod0: the first block of the product jobs, which close the list
  for (int i = 0; i < num_jobs; i++) {
    ndnet_pn_fold_job& J = jobs[i];
    const bool bn = J.gamma != nullptr;
    if (J.kind == NDNET_FOLD_PROD) {
      if (bn || !J.rhs || J.Np <= 0 || (J.out_f64 != 0 && J.out_f64 != 1)) return -20;
      if (prod0 < 0) prod0 = blocks;
    } else if (prod0 >= 0) {
      return -20;
    }
    if (!J.out || (uintptr_t)J.out % 16 || J.kind < NDNET_FOLD_WT || J.kind > NDNET_FOLD_PROD || J.N <= 0 ||
        (bn && (!J.beta || !J.mean || !J.var || !(J.eps >= 0.0f))) || (!bn && (J.beta || J.mean || J.var)))
      return -20;
    if (J.kind == NDNET_FOLD_BIAS) {
      if (!J.bias || J.Np < J.N || J.eye < 0 || (J.eye > 0 && J.eye * J.eye != J.N)) return -20;
    } else {
      if (!J.w || J.K <= 0 || J.k0 < 0 || J.ld < J.k0 + J.K) return -20;
      if (J.kind == NDNET_FOLD_WT && (J.Kp < J.K || J.Np < J.N)) return -20;
      if (J.kind == NDNET_FOLD_FRAG && (J.Kp < J.K || J.Np < J.N || J.Kp % 16 || J.Np % 16)) return -20;
      if (J.kind == NDNET_FOLD_FRAG6 && (J.Kp < J.K || J.Np < J.N || J.Kp % 32 || J.Np % 16)) return -20;
      if (J.kind == NDNET_FOLD_BASIS && J.K != 12) return -20;
    }
    J.block0 = blocks;
    blocks += (fold_units(J) + kFoldThreads - 1) / kFoldThreads;
  }
  if (blocks <= 0 || blocks > 0x7fffffff) return -20;
  *num_blocks = blocks | ((prod0 < 0 ? 0 : blocks - prod0) << 32);  // the product jobs' blocks in the upper half
  return 0;
}

int ndnet_pn_fold_run(const ndnet_pn_fold_job* jobs, int num_jobs, int64_t num_blocks, void* stream) {
  const int64_t blocks = num_blocks & 0xffffffff, prod = num_blocks >> 32;
  if (!jobs || num_jobs <= 0 || blocks <= 0 || blocks > 0x7fffffff || prod < 0 || prod > blocks) return -20;
  if (blocks > prod) k_pn_fold<<<(unsigned)(blocks - prod), kFoldThreads, 0, (hipStream_t)stream>>>(jobs, num_jobs, 0);
  // the products of what the first launch has just written, behind it in stream order
  if (prod) k_pn_fold<<<(unsigned)prod, kFoldThreads, 0, (hipStream_t)stream>>>(jobs, num_jobs, blocks - prod);
  return hipGetLastError() == hipSuccess ? 0 : -21;
}

int ndnet_pn_fold16_check(const ndnet_pn_fold16_job* jobs, int num_jobs, int64_t* max_units) {
  if (!jobs || num_jobs <= 0 || num_jobs > 65535 || !max_units) return -20;
  int64_t mu = 0;
  for (int i = 0; i < num_jobs; i++) {
    const ndnet_pn_fold16_job& J = jobs[i];
    if (!J.w || !J.out || !J.partial || !J.scale || (uintptr_t)J.out % 16 || J.N <= 0 || J.K <= 0 || J.k0 < 0 ||
        J.ld < J.k0 + J.K || J.Kp < J.K || J.Np < J.N || J.Kp % 32 || J.Np % 16 || (J.gamma == nullptr) != (J.var == nullptr) ||
        (J.gamma && !(J.eps >= 0.0f)))
      return -20;
    const int64_t units = (int64_t)J.Kp * J.Np / 8;
    if (units > mu) mu = units;
  }
  if ((mu + kFoldThreads - 1) / kFoldThreads > 0x7fffffff) return -20;
  *max_units = mu;
  return 0;
}

int ndnet_pn_fold16_run(const ndnet_pn_fold16_job* jobs, int num_jobs, int64_t max_units, void* stream) {
  const int64_t blocks = (max_units + kFoldThreads - 1) / kFoldThreads;
  if (!jobs || num_jobs <= 0 || num_jobs > 65535 || max_units <= 0 || blocks > 0x7fffffff) return -20;
  k_pn_fold16_max<<<dim3(kFold16Parts, num_jobs), kFoldThreads, 0, (hipStream_t)stream>>>(jobs);
  // the planes, scaled by what the first launch has just found, behind it in stream order
  k_pn_fold16_frag<<<dim3((unsigned)blocks, num_jobs), kFoldThreads, 0, (hipStream_t)stream>>>(jobs);
  return hipGetLastError() == hipSuccess ? 0 : -21;
}

// One fused point-MLP chain over `batch` clouds on `stream` (see pointnet.h).

// Timing builds: zeroes the stamp array (before a launch whose stamps are read)
int ndnet_pn_debug_stamps_clear(void) {
#ifdef NDNET_PN_STAMPS
  static unsigned long long zeros[kStampWgs][16];
  return hipMemcpyToSymbol(HIP_SYMBOL(g_pn_stamps), zeros, sizeof(zeros)) == hipSuccess ? 0 : -21;
#else
  return -20;
#endif
}

// Timing builds (-DNDNET_PN_STAMPS): copies the stamps of the last chain
// launch, [wgs][16] u64, to host memory; the product build returns -20.
int ndnet_pn_debug_stamps(unsigned long long* host, int wgs) {
#ifdef NDNET_PN_STAMPS
  if (!host || wgs <= 0 || wgs > kStampWgs) return -20;
  if (hipDeviceSynchronize() != hipSuccess) return -21;
  return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_pn_stamps), (size_t)wgs * 16 * sizeof(unsigned long long)) ==
                 hipSuccess ? 0 : -21;
#else
  (void)host; (void)wgs;
  return -20;
#endif
}
#endif

// an inconsistent argument block: NDNET_ERR_ARG, with the failing check's line on stderr
#define PN_ARG_FAIL()                                                                          \
  do {                                                                                         \
    fprintf(stderr, "ndnet_amd: chain launch: invalid argument (pointnet_kernels.hip:%d)\n", __LINE__); \
    return -20;                                                                                \
  } while (0)

}  // extern "C"

namespace {

// ext: the fp16 form's block (ndnet_pn_chain_f16_run), or NULL
int chain_launch(const ndnet_pn_chain* args, const ndnet_pn_f16* ext, int batch, void* stream) {
  if (!args || batch <= 0 || args->num_layers < 1 || args->num_layers > NDNET_PN_MAX_LAYERS || args->num_points <= 0 ||
      args->in_cols < 1 || args->in_cols > args->L[0].K || args->in_cols > args->x_ld)
    PN_ARG_FAIL();
  // activation regions: layer l reads region l & 1 (or the fused-chunk buffer
  // after a fused layer) and writes region (l + 1) & 1
  int w[2] = {args->L[0].K, 0};
  int pw1 = 0;  // widest split-bf16 input held in region 1 (three planes of pitch K + kPadB)
  bool has_fuse = false;
  int planes = 0, qprec = 0;
  int smode = 0;  // the one prec (1, 2 or 3) of the chain's split-bf16 layers; 0: it has none
  for (int l = 0; l < args->num_layers; l++) {
    const ndnet_pn_layer& L = args->L[l];
    if (!L.w || !L.bias || L.K <= 0 || L.K % 16 || L.N <= 0 || L.N % 32 || (L.N > 32 && L.N % 64) ||
        ((uintptr_t)L.w % 16) ||
        L.w_cloud_stride % 4)
      PN_ARG_FAIL();
    const bool fed = l > 0 && args->L[l - 1].fuse_next;
    if (L.prec < 0 || L.prec > 3) PN_ARG_FAIL();
    if (L.prec) {  // split-bf16: reads planes its producer writes (into a region, or the fused chunks)
      if (l == 0 || L.K % 32 || args->L[l - 1].N != L.K) PN_ARG_FAIL();
      if (smode && L.prec != smode) PN_ARG_FAIL();  // one mode per chain: the kernel is instantiated per mode
      smode = L.prec;
      if (fed) qprec = 1;
      else planes |= 1 << (l & 1);
      if (!fed && (l & 1) && L.K > pw1) pw1 = L.K;
    }
    if (fed) {
      if (L.K != args->L[l - 1].N || (L.N != 64 && L.N != 128 && L.N != 256) || L.fuse_next) PN_ARG_FAIL();
    } else if (l > 0 && L.K > w[l & 1]) {
      PN_ARG_FAIL();
    }
    if (L.fuse_next) {
      if (l + 1 >= args->num_layers || L.N % kFuseNC) PN_ARG_FAIL();
      has_fuse = true;
      continue;  // not stored in a region
    }
    const bool stored = l + 1 < args->num_layers || args->mode == 1;
    if (stored && L.N > w[(l + 1) & 1]) w[(l + 1) & 1] = L.N;
  }
  if (args->max_width < w[0] || args->max_width2 < w[1] || args->max_width % 8 || args->max_width2 % 8) PN_ARG_FAIL();
  if (args->mode == 1 && (!args->out || args->out_cols <= 0 || args->out_cols > args->L[args->num_layers - 1].N))
    PN_ARG_FAIL();
  if (args->mode == 0 && !args->gmax) PN_ARG_FAIL();
  // LDS: region 0 | region 1, then the fused pair's chunks.  Q writes the
  // region P reads, after its last chunk, so the chunks may start right after
  // P's input inside that region (and run past its end when it is region 1)
  const int r0f = region0_floats(*args, planes);
  // region 1 is sized here only (the kernel addresses it from region 0's end): its fp32 rows at the
  // pitch of max_width2, its bf16 planes at their consumer's K -- a wide fp32 last layer (mode 1,
  // N > 256) beside 256-wide planes then fits the 64-point build
  const int r1f32 = region_floats(args->max_width2, 0), r1b16 = pw1 ? region_floats(pw1, 1) : 0;
  const int r1f = r1b16 > r1f32 ? r1b16 : r1f32;
  int fbuf_off = r0f + r1f;
  size_t total = (size_t)r0f + r1f;
  if (has_fuse) {
    int lf = 0;
    while (!args->L[lf].fuse_next) lf++;
    const int r = lf & 1, fb = fbuf_floats(qprec);
    const int p_in = pair0_direct(*args) ? 0                                    // P reads the input rows: no tile
                     : args->L[lf].prec ? 3 * kP * (args->L[lf].K + kPadB) / 2  // P's input: bf16 planes, pitch K + kPadB
                                        : kP * ((r ? args->max_width2 : args->max_width) + kPadF);  // or fp32, region pitch
    const int inside = (r ? r0f : 0) + p_in;
    if (r == 1 || inside + fb <= r0f) fbuf_off = inside;
    total = fbuf_off + (size_t)fb > total ? fbuf_off + (size_t)fb : total;
  }
  if (args->head_h2) {  // the TNet(3) tail in the prologue: it writes layer 0's per-cloud weights (one k-group)
    const ndnet_pn_layer& L0 = args->L[0];
    if (!args->head_w3 || !args->head_b3 || !args->head_basis || !args->head_t1) PN_ARG_FAIL();
    if (args->head_K < 1 || args->head_ld < args->head_K || args->head_kin < 1 || args->head_kin > 16) PN_ARG_FAIL();
    // head_nout != L0.N would write the [16][64] LDS copy (VALU layer 0) out of its shape; a shorter
    // stride would make the clouds overwrite each other's weights
    if (L0.K != 16 || args->head_nout != L0.N || L0.w_cloud_stride < 16 * (int64_t)args->head_nout) PN_ARG_FAIL();
    // head_K == 256 reads h2's row and W3's rows as one float4 per lane
    if (args->head_K == 256 &&
        (((uintptr_t)args->head_h2 | (uintptr_t)args->head_w3) % 16 || args->head_ld % 4))
      PN_ARG_FAIL();
  }
  if ((args->fold_out_w || args->fold_out_b) && (!args->fold_t2 || !args->fold_out_w || !args->fold_out_b))
    PN_ARG_FAIL();
  if (args->fold_bias && !args->fold_t2) PN_ARG_FAIL();
  if (args->x_nonfinite_nan != 0 && args->x_nonfinite_nan != 1) PN_ARG_FAIL();
  if (args->fold_t2) {  // the t2 fold runs in layer 0's VALU prologue (after the head prologue, if any), t2 staged at region 1
    // fold_ld 0: one matrix for every cloud
    if (!valu_layer0(*args) || (args->fold_ld != 0 && args->fold_ld < 4096) || args->fold_ld % 4 ||
        (uintptr_t)args->fold_t2 % 16)
      PN_ARG_FAIL();
    if (total < (size_t)r0f + 4096) total = (size_t)r0f + 4096;
  }
  // every layer's bias after the other regions (layer 0's too: the prologue
  // reads it there when layer 0 runs on the MFMA path)
  const int bias_base = (int)((total + 3) & ~(size_t)3);
  int nbias = 0;
  for (int l = 0; l < args->num_layers; l++) {
    if (args->L[l].N > 2 * kThreads) PN_ARG_FAIL();  // the prologue stages <= 2 bias values per thread and layer
    nbias += args->L[l].N;
  }
  total = (size_t)bias_base + nbias;
  int flag_base = 0;
  if (ext) {
    // the fp16 form: prec 1 layers only (its fallback is k_pn_chain<6>'s body), each with its planes and
    // scale; a pooled last layer fed by a fused one would max-pool before its input's window is known
    if (smode != 1 || !ext->fallbacks) PN_ARG_FAIL();
    for (int l = 0; l < args->num_layers; l++) {
      if (!args->L[l].prec) continue;
      if (!ext->w16[l] || !ext->scale[l] || (uintptr_t)ext->w16[l] % 16 || args->L[l].w_cloud_stride) PN_ARG_FAIL();
      // a split layer produced in chunks into the next (the layered seg head's 64 -> 512) has no caller in
      // this form -- the forward takes it only with chain D collapsed, whose fused P is fp32 -- and no test
      if (args->L[l].fuse_next) PN_ARG_FAIL();
    }
    const int nl = args->num_layers;
    if (args->mode == 0 && nl >= 2 && args->L[nl - 2].fuse_next) PN_ARG_FAIL();
    flag_base = (int)total;  // the window words, one per layer, behind the biases
    total += NDNET_PN_MAX_LAYERS;
  }
  const size_t lds = sizeof(float) * total;
  const int ki = ext ? 3 : smode > 1 ? smode - 1 : 0;  // k_pn_chain<6>, <3>, <1>, k_pn_chain_f16
  const void* const kernel = ki == 0   ? (const void*)k_pn_chain<6>
                             : ki == 1 ? (const void*)k_pn_chain<3>
                             : ki == 2 ? (const void*)k_pn_chain<1>
                                       : (const void*)k_pn_chain_f16;
  static bool attr_set[4] = {false, false, false, false};
  if (!attr_set[ki]) {
    if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess) return -21;
    attr_set[ki] = true;
  }
  if (lds > 160 * 1024) PN_ARG_FAIL();
  dim3 grid((args->num_points + kP - 1) / kP, batch);
  hipStream_t st = (hipStream_t)stream;
  if (ki == 0) k_pn_chain<6><<<grid, kThreads, lds, st>>>(*args, planes, fbuf_off, bias_base);
  else if (ki == 1) k_pn_chain<3><<<grid, kThreads, lds, st>>>(*args, planes, fbuf_off, bias_base);
  else if (ki == 2) k_pn_chain<1><<<grid, kThreads, lds, st>>>(*args, planes, fbuf_off, bias_base);
  else k_pn_chain_f16<<<grid, kThreads, lds, st>>>(*args, *ext, planes, fbuf_off, bias_base, flag_base);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    fprintf(stderr, "ndnet_amd: k_pn_chain launch failed: %s\n", hipGetErrorString(e));
    return -21;
  }
  return 0;
}

}  // namespace

extern "C" {

#if NDNET_PN_TILE == 64
int ndnet_pn_chain_run(const ndnet_pn_chain* args, int batch, void* stream) {
  return chain_launch(args, nullptr, batch, stream);
}

int ndnet_pn_chain_f16_run(const ndnet_pn_chain* args, const ndnet_pn_f16* ext, int batch, void* stream) {
  if (!ext) PN_ARG_FAIL();
  return chain_launch(args, ext, batch, stream);
}

int ndnet_pn_take_f16_fallbacks(uint32_t* device_counter, void* stream) {
  if (!device_counter) return -20;
  hipStream_t st = (hipStream_t)stream;
  uint32_t v = 0;
  if (hipMemcpyAsync(&v, device_counter, sizeof v, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipMemsetAsync(device_counter, 0, sizeof v, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
    return -21;
  return v > 0x7fffffffu ? 0x7fffffff : (int)v;
}
#else
int ndnet_pn_chain_run_t32(const ndnet_pn_chain* args, int batch, void* stream) {
  return chain_launch(args, nullptr, batch, stream);
}

int ndnet_pn_chain_f16_run_t32(const ndnet_pn_chain* args, const ndnet_pn_f16* ext, int batch, void* stream) {
  if (!ext) PN_ARG_FAIL();
  return chain_launch(args, ext, batch, stream);
}
#endif

}  // extern "C"
