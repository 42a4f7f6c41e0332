// pointnet_chain_body.inc -- the body of the chain kernels of pointnet_kernels.hip: one tile from its first
// load to its stores.  Included as text, once into k_pn_chain<T> itself (the compiler then sees the
// kernel it always saw: a call through a function, even an inlined one, changed k_pn_chain<6>'s register
// allocation) and once into pn_chain_body<T>, which k_pn_chain_f16 calls twice.  The including scope
// provides T, A, X, planes, fbuf, bias_base, flag_base and PN_BODY_FAIL (what leaves the body when a
// T = 2 tile is outside fp16's window; never reached for another T).
  const int b = blockIdx.y;
  const int p0 = blockIdx.x * kP;
  PN_STAMP(0);
  // LDS: activation region 0 | region 1 | [fused-chunk double buffer] | biases of layers 1..
  const int pitch0 = A.max_width + kPadF, pitch1 = A.max_width2 + kPadF;
  const int reg[2] = {0, region0_floats(A, planes)};
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // every layer's bias (this cloud's) -> LDS at boff[l] (layer 0's into the
  // prologue scratch when it runs on the VALU); the loads are issued together
  // with the prologue's, so the epilogues never wait on a global bias read
  int boff[NDNET_PN_MAX_LAYERS];
  {
    int o = bias_base;
#pragma unroll
    for (int l = 0; l < NDNET_PN_MAX_LAYERS; l++) {
      boff[l] = o;
      if (l < A.num_layers) o += A.L[l].N;
    }
    float bv[NDNET_PN_MAX_LAYERS][2];
#pragma unroll
    for (int l = 0; l < NDNET_PN_MAX_LAYERS; l++)
#pragma unroll
      for (int i = 0; i < 2; i++) {
        const int e = threadIdx.x + i * kThreads;
        bv[l][i] = (l < A.num_layers && e < A.L[l].N) ? A.L[l].bias[(int64_t)b * A.L[l].bias_cloud_stride + e] : 0.0f;
      }
#pragma unroll
    for (int l = 0; l < NDNET_PN_MAX_LAYERS; l++)
#pragma unroll
      for (int i = 0; i < 2; i++) {
        const int e = threadIdx.x + i * kThreads;
        if (l < A.num_layers && e < A.L[l].N) g_smem[boff[l] + e] = bv[l][i];
      }
  }
  if constexpr (T == 2) {  // the window words: zero (|v| >= 0) ahead of the prologue's barriers
    if (threadIdx.x < NDNET_PN_MAX_LAYERS) reinterpret_cast<unsigned*>(g_smem)[flag_base + threadIdx.x] = 0u;
  }
  // T = 2: whether split layer l's input tile lies in fp16's window -- its maximum |v| in [2^-4, 2^11), or
  // all zero; a NaN or an infinity fails the upper test.  Read after the barrier behind the tile's stores.
  auto in_window = [&](int l) {
    const float m = g_smem[flag_base + l];
    return m == 0.0f || (m >= 0.0625f && m < 2048.0f);
  };
  const bool v0 = valu_layer0(A);
  Pre pre;  // the next layer's first weight step (prefetched before each layer barrier)
  prefetch_first<T>(A, v0 ? 1 : 0, b, pre);
  float* const s_w0 = g_smem;  // v0: W0^T [16][64] row-major, in region 0
  // v0: this thread's point rows (t / 16 + pass * kThreads / 16) and 4 output
  // channels (4 (t % 16) ..)
  constexpr int kV0Pass = kP * 16 / kThreads;
  static_assert(kV0Pass >= 1 && kV0Pass * kThreads == kP * 16, "whole layer-0 passes");
  const int vq = threadIdx.x & 15;
  f32x4 xin[kV0Pass][3] = {};
  // both prologues (chain B collapsed): the fold matrix is no product of this launch's head, so waves
  // 0..3, which run the fold, load their B operands of its 16 MFMA steps here with the kernel's first
  // loads -- M[4 st + fk][16 wave + fr], no LDS staging -- and they land under the head prologue's two
  // round trips
  const bool fold_early = A.head_h2 && A.fold_t2;
  constexpr int kFoldPitch = 68;  // floats per row of the head's W1f copy the fold reads: 16 rows x 4 k on 64 distinct banks
  float fmr[16] = {};
  if (fold_early && wave < 4) {
    const float* mb = A.fold_t2 + (int64_t)b * A.fold_ld + (lane >> 4) * 64 + 16 * wave + (lane & 15);
#pragma unroll
    for (int st = 0; st < 16; st++) fmr[st] = mb[st * 256];
  }
  // ... and the folded layer's own bias (TNet(64) conv1's), joined to b0' by waves 0..3: column 16 wave + (lane & 15)
  const float fb = A.fold_bias ? A.fold_bias[(16 * wave + (lane & 15)) & 63] : 0.0f;
  // a chain that opens with the direct fused pair: this lane's piece of its input row, P's A operand for
  // every chunk (row (wave / 4) * 16 + cl, columns 4 kq ..; zero past in_cols and past the cloud)
  const bool direct0 = pair0_direct(A);
  f32x4 xa = {0.f, 0.f, 0.f, 0.f};
  if (direct0) {
    const int kq = lane >> 4, p = p0 + (wave / 4) * 16 + (lane & 15);
    if (p < A.num_points && 4 * kq < A.in_cols) {
      xa = *reinterpret_cast<const f32x4*>(A.x + ((int64_t)b * A.num_points + p) * A.x_ld + 4 * kq);
#pragma unroll
      for (int s = 0; s < 4; s++) {
        if (4 * kq + s >= A.in_cols) xa[s] = 0.0f;
        else if (A.x_nonfinite_nan && !(fabsf(xa[s]) < INFINITY)) xa[s] = NAN;
      }
    }
  }
  if (v0) {
#pragma unroll
    for (int ps = 0; ps < kV0Pass; ps++) {
      const int vr = (threadIdx.x >> 4) + ps * (kThreads / 16);
      const int p = p0 + vr;
      if (p < A.num_points) {
        const f32x4* xr = reinterpret_cast<const f32x4*>(A.x + ((int64_t)b * A.num_points + p) * A.x_ld);
#pragma unroll
        for (int i = 0; i < 3; i++)
          if (4 * i < A.in_cols) xin[ps][i] = xr[i];
      }
    }
    if (!A.head_h2 && threadIdx.x < 256) {  // W0^T fragment-major [cb][kq][cl][s] -> row-major [k][n]
      const f32x4 wv = reinterpret_cast<const f32x4*>(A.L[0].w + (int64_t)b * A.L[0].w_cloud_stride)[threadIdx.x];
      const int cb = threadIdx.x >> 6, kq = (threadIdx.x >> 4) & 3, cl = threadIdx.x & 15;
#pragma unroll
      for (int s = 0; s < 4; s++) s_w0[(4 * kq + s) * 64 + 16 * cb + cl] = wv[s];
    }
  }
  if (A.head_h2) {
    // TNet(3)'s tail for this cloud (ndnet_pn_head3_run's work, ndtnet.py:57-60):
    // t1 = h2 @ W3^T + b3, then conv1 with t1 folded into layer 0's weights
    float* const s_t1 = g_smem + (v0 ? kValu0Floats : 0);  // [9] (v0: past the scratch; region 0 is free until layer 1)
    const int M = A.head_kin * A.head_nout, total = 16 * A.head_nout;  // one k-group, K padded to 16
    // this thread's fold element(s): basis values loaded ahead of the fc3 reduction
    const int e0 = threadIdx.x;
    const int cb0 = e0 >> 8, ln0 = (e0 >> 2) & 63, k0 = 4 * (ln0 >> 4) + (e0 & 3), n0 = 16 * cb0 + (ln0 & 15);
    float bas[9];
#pragma unroll
    for (int a = 0; a < 9; a++) bas[a] = (e0 < total && k0 < A.head_kin) ? A.head_basis[a * M + k0 * A.head_nout + n0] : 0.0f;
    const float* h = A.head_h2 + (int64_t)b * A.head_ld;
    for (int o = wave; o < 9; o += kWaves) {  // one wave per output, lanes split K
      float acc = 0.0f;
      const float* wr = A.head_w3 + (int64_t)o * A.head_K;
      if (A.head_K == 256) {  // one float4 of h and of the row per lane: one load round trip
        const f32x4 hv = reinterpret_cast<const f32x4*>(h)[lane];
        const f32x4 wv = reinterpret_cast<const f32x4*>(wr)[lane];
        acc = (hv[0] * wv[0] + hv[1] * wv[1]) + (hv[2] * wv[2] + hv[3] * wv[3]);
      } else {
        for (int k = lane; k < A.head_K; k += 64) acc += h[k] * wr[k];
      }
      for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
      if (lane == 0) {
        s_t1[o] = acc + A.head_b3[o];
        if (blockIdx.x == 0) A.head_t1[b * 9 + o] = acc + A.head_b3[o];
      }
    }
    __syncthreads();
    float* w1 = const_cast<float*>(A.L[0].w) + (int64_t)b * A.L[0].w_cloud_stride;
    // v0: only the cloud's first workgroup publishes the fragment-major W0^T
    // (chains C and D read it in later launches); every workgroup keeps its own
    // copy in LDS.  Otherwise every workgroup stores it and its layer 0 reads it.
    const bool publish = !v0 || blockIdx.x == 0;
    for (int e = e0; e < total; e += kThreads) {
      const int cb = e >> 8, ln = (e >> 2) & 63, k = 4 * (ln >> 4) + (e & 3), n = 16 * cb + (ln & 15);
      float acc = 0.0f;
      if (e == e0) {
#pragma unroll
        for (int a = 0; a < 9; a++) acc += s_t1[a] * bas[a];
      } else if (k < A.head_kin) {
#pragma unroll
        for (int a = 0; a < 9; a++) acc += s_t1[a] * A.head_basis[a * M + k * A.head_nout + n];
      }
      if (publish) w1[e] = acc;
      // the fold prologue follows: its A operand [W1f; b1; 0] goes to region 1 at a pitch its reads do
      // not conflict on, and s_w0 is left to its output (no barrier between its MFMAs and its stores)
      if (fold_early) g_smem[reg[1] + k * kFoldPitch + n] = k == 12 ? g_smem[boff[0] + n] : acc;
      else if (v0) s_w0[k * 64 + n] = acc;
    }
    // !v0: layer 0 reads these weights back: __syncthreads' workgroup-scope release
    // / acquire orders this workgroup's stores before its loads (same CU; no
    // lines of them are cached here yet).  Every workgroup of the cloud stores
    // the same bits.  (A device-scope __threadfence here writes back the L2:
    // measured +60 us per launch.)
    PN_STAMP(1);
  }
  if (A.fold_t2) {
    // TNet(64)'s transform through layer 0 (chains C, D; v0 only, checked on
    // the host): x_t2 = t2^T (W0 x + b0) = (W0^T t2)^T x + t2^T b0, so layer 0
    // runs on W0' = W0^T t2 (its 12 used rows) and b0' = b0^T t2: a 16 x 64 x 64
    // GEMM (rows 0..11 W0^T, row 12 the bias, 13..15 zero) on the fp32 MFMA,
    // waves 0..3 one 16-column block each, t2 staged in region 1 (layer 0 has
    // not written it yet; the launcher keeps the biases past it)
    // After the head prologue (chain B collapsed: a shared matrix, hot in L2) the same product takes
    // its B operand from registers (fmr) and its A operand from the head's copy in region 1, so the
    // fold costs one barrier and 16 MFMAs of four waves.
    float* const s_t2 = g_smem + reg[1];
    f32x4 fo = {0.f, 0.f, 0.f, 0.f};
    const int fr = lane & 15, fk = lane >> 4;  // operand row / k within a 4-step
    if (fold_early) {
      __syncthreads();  // [W1f; b1; 0] at s_t2, pitch kFoldPitch
      if (wave < 4) {
#pragma unroll
        for (int st = 0; st < 16; st++)
          fo = __builtin_amdgcn_mfma_f32_16x16x4f32(s_t2[fr * kFoldPitch + 4 * st + fk], fmr[st], fo, 0, 0, 0);
      }
    } else {
      const f32x4* t2b = reinterpret_cast<const f32x4*>(A.fold_t2 + (int64_t)b * A.fold_ld);
      for (int e = threadIdx.x; e < 1024; e += kThreads) reinterpret_cast<f32x4*>(s_t2)[e] = t2b[e];
      __syncthreads();  // + s_w0 (W0^T row-major) and layer 0's bias at boff[0]
      if (wave < 4) {
#pragma unroll
        for (int st = 0; st < 16; st++) {
          const int i = 4 * st + fk;
          const float av = fr < 12 ? s_w0[fr * 64 + i] : fr == 12 ? g_smem[boff[0] + i] : 0.0f;
          const float bv = s_t2[i * 64 + 16 * wave + fr];
          fo = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, fo, 0, 0, 0);
        }
      }
      __syncthreads();
    }
    if (wave < 4) {  // lane (fk, fr): rows 4 fk + r, column 16 wave + fr
      const int n = 16 * wave + fr;
      if (A.fold_bias && fk == 3) fo[0] += fb;  // row 12: b0' = b0^T M + the folded layer's bias
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int row = 4 * fk + r;
        if (row < 12) s_w0[row * 64 + n] = fo[r];
        else if (row == 12) g_smem[boff[0] + n] = fo[r];
      }
      // the cloud's first workgroup publishes W0' (fragment-major, K = 16, rows
      // 12..15 left zero) and b0' for a later chain's plain layer 0 (chain D)
      if (A.fold_out_w && blockIdx.x == 0) {
        float* ow = A.fold_out_w + (int64_t)b * 1024;
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const int row = 4 * fk + r;
          if (row < 12) ow[(((n >> 4) * 64 + ((row >> 2) & 3) * 16 + (n & 15)) << 2) + (row & 3)] = fo[r];
          else if (row == 12) A.fold_out_b[(int64_t)b * 64 + n] = fo[r];
        }
      }
    }
    PN_STAMP(1);  // (timing builds) chains C / D: t2 staged and folded into layer 0
  }
  __syncthreads();
  if (v0) {
    // layer 0: out = act(x W0^T + b0) for 4 channels of one point, into region 1
    // as the next layer reads it (three bf16 planes, or fp32)
#pragma unroll
    for (int ps = 0; ps < kV0Pass; ps++) {
      const int vr = (threadIdx.x >> 4) + ps * (kThreads / 16);
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      float xs[12] = {xin[ps][0][0], xin[ps][0][1], xin[ps][0][2], xin[ps][0][3], xin[ps][1][0], xin[ps][1][1],
                      xin[ps][1][2], xin[ps][1][3], xin[ps][2][0], xin[ps][2][1], xin[ps][2][2], xin[ps][2][3]};
      if (A.x_nonfinite_nan) {  // a collapsed first layer: the row leaves its ReLU as zeros, as the layered pair's does
#pragma unroll
        for (int k = 0; k < 12; k++) xs[k] = fabsf(xs[k]) < INFINITY ? xs[k] : NAN;
      }
#pragma unroll
      for (int k = 0; k < 12; k++) {
        if (k < A.in_cols) {
          const f32x4 w = *reinterpret_cast<const f32x4*>(s_w0 + k * 64 + 4 * vq);
#pragma unroll
          for (int j = 0; j < 4; j++) acc[j] = fmaf(xs[k], w[j], acc[j]);
        }
      }
      const f32x4 bb = *reinterpret_cast<const f32x4*>(g_smem + boff[0] + 4 * vq);
#pragma unroll
      for (int j = 0; j < 4; j++) {
        acc[j] += bb[j];
        if (A.L[0].relu) acc[j] = fmaxf(acc[j], 0.0f);
      }
      const int out = reg[1];
      if (A.L[1].prec) {  // the mode's bf16 planes, pitch 64 + kPadB
        typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
        const int pb = 64 + kPadB;
        __bf16* const base = reinterpret_cast<__bf16*>(g_smem + out) + vr * pb + plane_col(vr, 4 * vq);
        if constexpr (T == 2) {  // two fp16 planes of split(16 v), and the tile's maximum |v| for layer 1's window
          f16x4 h4, l4;
          unsigned mx = 0;
#pragma unroll
          for (int j = 0; j < 4; j++) {
            mx = max(mx, __float_as_uint(acc[j]) & 0x7fffffffu);
            _Float16 hh, ll;
            split_f16(acc[j], hh, ll);
            h4[j] = hh;
            l4[j] = ll;
          }
          *reinterpret_cast<f16x4*>(base) = h4;
          *reinterpret_cast<f16x4*>(base + kP * pb) = l4;
          window_note(flag_base + 1, mx);
        } else {
          bf16x4 h4, m4, l4;
#pragma unroll
          for (int j = 0; j < 4; j++) {
            __bf16 hh, mm, ll;
            split_t<T>(acc[j], hh, mm, ll);
            h4[j] = hh;
            if constexpr (T >= 3) m4[j] = mm;
            if constexpr (T == 6) l4[j] = ll;
          }
          *reinterpret_cast<bf16x4*>(base) = h4;
          if constexpr (T >= 3) *reinterpret_cast<bf16x4*>(base + kP * pb) = m4;
          if constexpr (T == 6) *reinterpret_cast<bf16x4*>(base + 2 * kP * pb) = l4;
        }
      } else {
        *reinterpret_cast<f32x4*>(g_smem + out + vr * pitch1 + 4 * vq) = acc;
      }
    }
  } else if (!direct0) {
    const int K0 = A.L[0].K;
    for (int e = threadIdx.x; e < kP * K0; e += kThreads) {
      const int r = e / K0, c = e % K0;
      const int p = p0 + r;
      float v = 0.0f;
      if (p < A.num_points && c < A.in_cols) v = A.x[((int64_t)b * A.num_points + p) * A.x_ld + c];
      if (A.x_nonfinite_nan && !(fabsf(v) < INFINITY)) v = NAN;
      g_smem[r * pitch0 + c] = v;
    }
  }
  __syncthreads();
  PN_STAMP(2);
  const int rows_valid = A.num_points - p0;
  float* const gmax_b = A.mode == 0 ? A.gmax + (int64_t)b * A.gmax_ld : nullptr;
  int lfirst = v0 ? 1 : 0;
  if constexpr (kP == 64 && kWaves == 16) {
    if (direct0) {  // layers 0 and 1 as the direct fused pair, ahead of the loop: xa is live up to here only
      const LayerCtx P = layer_ctx<T>(A, X, 0, b, g_smem + boff[0]), Q = layer_ctx<T>(A, X, 1, b, g_smem + boff[1]);
      const bool last = A.num_layers == 2;
      fused_pair_x6p<4, T, true>(P, Q, reg[0], fbuf, reg[0], pitch0, (last && gmax_b) ? gmax_b : nullptr, rows_valid,
                                 !last && A.L[2].prec, xa, flag_base + 1, flag_base + 2);
      __syncthreads();
      PN_STAMP(3 + 1);
      if constexpr (T == 2) {  // Q's input, chunk by chunk (the launcher keeps such a Q from being a pooled last layer)
        if (!in_window(1)) PN_BODY_FAIL;
      }
      lfirst = 2;
    }
  }
  for (int l = lfirst; l < A.num_layers; l++) {
    const int in = reg[l & 1], pin = (l & 1) ? pitch1 : pitch0;
    if constexpr (T == 2) {  // this layer's input tile, complete since the last barrier
      if (A.L[l].prec && !in_window(l)) PN_BODY_FAIL;
    }
    const int qflag = flag_base + l + 1, oflag = flag_base + l + (A.L[l].fuse_next ? 2 : 1);  // T = 2: window words
    if (A.L[l].fuse_next) {  // layers l and l + 1 together; l + 1 writes region (l + 2) & 1
      const LayerCtx P = layer_ctx<T>(A, X, l, b, g_smem + boff[l]), Q = layer_ctx<T>(A, X, l + 1, b, g_smem + boff[l + 1]);
      const bool last = l + 2 == A.num_layers;
      const int out = reg[(l + 2) & 1], pout = ((l + 2) & 1) ? pitch1 : pitch0;
      float* gm = (last && gmax_b) ? gmax_b : nullptr;
      // Q is one chunk of its (RB, NB) split: NB = N2 / (16 * column groups)
      constexpr int kQ = 16 / kWaves > 0 ? 16 / kWaves : 1;
      const bool op = !last && A.L[l + 2].prec;  // the layer after Q reads bf16 planes
      if constexpr (kP == 32) {  // two row blocks: each Q split with half the row groups
        if (Q.N == 256) fused_pair<2, kQ, T>(P, Q, in, pin, fbuf, out, pout, gm, rows_valid, op, {}, qflag, oflag);
        else fused_pair<1, kQ, T>(P, Q, in, pin, fbuf, out, pout, gm, rows_valid, op, {}, qflag, oflag);
      } else {
        bool piped = false;
        if constexpr (kWaves == 16) {
          if (NDNET_PN_FUSED_PIPE && Q.N == 256 && P.prec && Q.prec && P.KG == 2) {
            fused_pair_x6p<4, T>(P, Q, in, fbuf, out, pout, gm, rows_valid, op, f32x4{0.f, 0.f, 0.f, 0.f}, qflag, oflag);
            piped = true;
          }
        }
        if (piped) {
        } else if (Q.N == 256) fused_pair<4, kQ, T>(P, Q, in, pin, fbuf, out, pout, gm, rows_valid, op, pre, qflag, oflag);
        else if (Q.N > 64) fused_pair<2, kQ, T>(P, Q, in, pin, fbuf, out, pout, gm, rows_valid, op, pre, qflag, oflag);
        else fused_pair<1, kQ, T>(P, Q, in, pin, fbuf, out, pout, gm, rows_valid, op, pre, qflag, oflag);
      }
      l++;
    } else {
      const LayerCtx C = layer_ctx<T>(A, X, l, b, g_smem + boff[l]);
      const bool last = l + 1 == A.num_layers;
      const int out = reg[(l + 1) & 1], pout = ((l + 1) & 1) ? pitch1 : pitch0;
      float* gm = (last && gmax_b) ? gmax_b : nullptr;
      const bool op = !last && A.L[l + 1].prec;  // the next layer reads bf16 planes
      if constexpr (kP == 32) {
        // 32-point tiles, 8 waves: two row blocks, columns per wave as the
        // 64-point form's (one row group, all waves across the columns)
        if (C.N % 256 == 0) plain_layer<2, 2, T>(C, in, pin, out, pout, gm, rows_valid, op, {}, oflag);
        else if (C.N % 128 == 0) plain_layer<2, 1, T>(C, in, pin, out, pout, gm, rows_valid, op, {}, oflag);
        else plain_layer<1, 1, T>(C, in, pin, out, pout, gm, rows_valid, op, {}, oflag);  // N % 64 == 0, or N = 32 (half idle)
      } else if constexpr (kWaves == 8) {
        // 8 waves (2 per SIMD, up to 256 registers each): a wave takes up to
        // four column blocks, so each A fragment feeds NB MFMAs per plane
        // (tools/ubench/mfma_bf16_peak.hip b9 / b13 vs b3)
#ifndef NDNET_PN_W8_NB4
#define NDNET_PN_W8_NB4 1
#endif
        if (NDNET_PN_W8_NB4 && C.N % 512 == 0) plain_layer<4, 4, T>(C, in, pin, out, pout, gm, rows_valid, op, {}, oflag);
        else if (C.N % 256 == 0) plain_layer<4, 2, T>(C, in, pin, out, pout, gm, rows_valid, op, {}, oflag);
        else if (C.N % 128 == 0) plain_layer<4, 1, T>(C, in, pin, out, pout, gm, rows_valid, op, {}, oflag);
        else if (C.N % 64 == 0) plain_layer<2, 1, T>(C, in, pin, out, pout, gm, rows_valid, op, {}, oflag);
        else plain_layer<1, 1, T>(C, in, pin, out, pout, gm, rows_valid, op, {}, oflag);  // N = 32
      } else {
#ifndef NDNET_PN_NB2  // two column blocks per wave on the 1024-wide x6 layers (-5% per layer, r03q)
#define NDNET_PN_NB2 1
#endif
        if (NDNET_PN_NB2 && C.N % 512 == 0 && C.prec) plain_layer<4, 2, T>(C, in, pin, out, pout, gm, rows_valid, op, pre, oflag);
        else if (C.N % 256 == 0) plain_layer<4, 1, T>(C, in, pin, out, pout, gm, rows_valid, op, pre, oflag);
        else if (C.N % 128 == 0) plain_layer<2, 1, T>(C, in, pin, out, pout, gm, rows_valid, op, pre, oflag);
        else plain_layer<1, 1, T>(C, in, pin, out, pout, gm, rows_valid, op, pre, oflag);  // N % 64 == 0, or N = 32 (half idle)
      }
    }
#ifdef NDNET_PN_PREFETCH
    if (l + 1 < A.num_layers) {
      prefetch_first<T>(A, l + 1, b, pre);
      layer_barrier();
    } else {
      __syncthreads();
    }
#else
    __syncthreads();
#endif
    PN_STAMP(3 + l);
    if constexpr (T == 2) {  // a fused pair just closed: its Q's input, which came chunk by chunk
      if (l > 0 && A.L[l].prec && A.L[l - 1].fuse_next && !in_window(l)) PN_BODY_FAIL;
    }
  }
  if (A.clear && blockIdx.x == 0 && blockIdx.y == 0)
    for (int64_t i = threadIdx.x; i < A.clear_count; i += kThreads) A.clear[i] = -INFINITY;
  if (A.mode == 1) {  // log_softmax over channels (ndtnet.py:239), [B][N][C+1] layout
    const int lg = reg[A.num_layers & 1];
    const int pl = (A.num_layers & 1) ? pitch1 : pitch0;
    // 16 lanes per point (a quarter wave): columns q, q + 16, ...; the max
    // and the sum of exponentials meet in xor shuffles within the group
    constexpr int kLpr = 16, kRpp = kThreads / kLpr;  // lanes per row, rows per pass
    const int q = threadIdx.x % kLpr;
    for (int r0 = 0; r0 < kP; r0 += kRpp) {
      const int r = r0 + threadIdx.x / kLpr;
      const int p = p0 + r;
      const bool live = r < kP && p < A.num_points;  // uniform per 16-lane group
      const float* row = g_smem + lg + (r < kP ? r : 0) * pl;
      float m = -INFINITY;
      for (int c = q; c < A.out_cols; c += kLpr) m = fmaxf(m, row[c]);
#pragma unroll
      for (int o = kLpr / 2; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
      float sum = 0.0f;
      for (int c = q; c < A.out_cols; c += kLpr) sum += expf(row[c] - m);
#pragma unroll
      for (int o = kLpr / 2; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
      const float ls = logf(sum);
      if (live) {
        float* out = A.out + ((int64_t)b * A.num_points + p) * A.out_cols;
        for (int c = q; c < A.out_cols; c += kLpr) out[c] = (row[c] - m) - ls;
      }
    }
  }
  PN_STAMP(15);
