/*
 * ndnet_pointnet.h -- C ABI of the fused point-MLP kernel of libndnet_amd.so
 * (ndt-net_amd/csrc/pointnet_kernels.hip), the NDTNetSegmentation eval forward
 * on gfx950.
 *
 * It replaces the per-point Conv1d(k=1) + BatchNorm1d + ReLU chains of
 * ndnet/models/ndtnet.py:45-60 (TNet convs), :148-161 (NDTNet convs) and
 * :233-241 (segmentation head), each of which the reference runs as separate
 * torch ops with activations round-tripping through memory.  Host side:
 * ndt-net_amd/ndnet/models/pointnet_hip.py (BatchNorm folding, per-cloud
 * steps, the four chains A-D).  NDTNetClassification's eval forward shares
 * chains A-C and ends in its own head (ndnet_pn_cls_head_run below).
 *
 * Layer weights are W^T (K input channels x N output channels) with BatchNorm
 * folded in, K padded to a multiple of 16 and N to 32 (N <= 32) or 64, stored FRAGMENT-MAJOR
 * for the 16x16x4 fp32 MFMA: element (k, n) at
 *   ((n / 16) * (K / 16) + k / 16) * 256 + (((k / 4) % 4) * 16 + n % 16) * 4 + k % 4
 * i.e. [column block][k-group][lane = 16 ((k/4)%4) + n%16][k%4] -- one 1 KB
 * (k-group, column block) piece is what one wave loads per k-group, lane l
 * holding the B operands of four consecutive MFMAs.  Padding is zero.
 */
#ifndef NDNET_POINTNET_H_
#define NDNET_POINTNET_H_
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NDNET_PN_MAX_LAYERS 5

typedef struct ndnet_pn_layer {
  const float* w;         // fragment-major W^T, K * N floats (+ cloud * w_cloud_stride), 16-byte aligned
  int64_t w_cloud_stride; // 0 for shared weights, else the per-cloud stride (floats) of folded weights
  const float* bias;      // [N] (+ cloud * bias_cloud_stride)
  int64_t bias_cloud_stride;
  int32_t K, N;           // padded sizes: K % 16 == 0; N == 32 or N % 64 == 0
  int32_t relu;
  int32_t prec;           // 0: fp32 MFMA (v_mfma_f32_16x16x4_f32) on fp32 fragment-major weights;
                          // 1: split-bf16 "x6" (fp32-accurate, v_mfma_f32_16x16x32_bf16): K % 32 == 0,
                          //    `w` = bf16 [N/16][K/32][3 planes][64 lanes][8] with W^T = h + m + l and
                          //    lane l's 8 values W^T[32 kg + 8 (l/16) + j][16 cb + l%16]; the layer's
                          //    producer must be the previous, unfused layer (it stores bf16 planes).
                          //    Per operand pair x = h + m + l, y = h' + m' + l' it keeps the six products
                          //    mm', mh', lh', hl', hm', hh' (dropped: < 3 * 2^-24 |x y|, fp32's own rounding)
                          // 2: split-bf16 "x3": the products mh', hm', hh' of the same planes (16 significant
                          //    bits per operand); dropped terms <= 3.02 * 2^-18 |x y| per product
                          // 3: split-bf16 "x1": hh' only -- plain bf16 operands, fp32 accumulation; dropped
                          //    terms <= (2^-8 + 2^-18) |x y| per product
                          //    (from |x - h| <= 2^-9 |x|, |x - h - m| <= 2^-18 |x|, round to nearest even)
                          //    2 and 3 read the prec 1 weights as they are (NDNET_FOLD_FRAG6: one fold
                          //    serves the three modes; the planes a mode does not use are never loaded)
                          //    under the constraints of prec 1.  All layers of a chain with prec != 0 carry
                          //    the same prec (each mode is an instantiation of the whole kernel; prec 1's is
                          //    the code it was without the others); prec 0 layers mix freely with them
  int32_t fuse_next;     // 1: this layer's output (N % 64 == 0) is produced in 64-column chunks, each
                          // consumed at once by the next layer (whose N is 64, 128 or 256) -- the
                          // activation never occupies LDS whole
} ndnet_pn_layer;

// mode: 0 = max-pool the last layer over points into gmax[cloud][N]
//       1 = log-softmax over the first `out_cols` channels of the last layer,
//           written to out[cloud][point][out_cols]
typedef struct ndnet_pn_chain {
  const float* x;         // [B][num_points][x_ld] input rows
  int32_t x_ld;           // floats per input row (12)
  int32_t in_cols;        // columns of x the first layer reads (3 or 12); the rest of K is zero
  int32_t num_points;
  int32_t num_layers;
  ndnet_pn_layer L[NDNET_PN_MAX_LAYERS];
  int32_t mode;
  int32_t out_cols;
  float* gmax;            // mode 0: [B][gmax_ld], pre-set to -inf
  int32_t gmax_ld;
  int32_t max_width;      // widest activation of LDS region 0 (the input, layers 1, 3, ... outputs), % 8 == 0
  int32_t max_width2;     // widest activation of LDS region 1 (layers 0, 2, ... outputs), % 8 == 0; a fused
                          // layer's output is not stored in either region
  float* out;             // mode 1
  float* clear;           // optional: set clear[0 .. clear_count) to -inf once the chain no longer
  int64_t clear_count;    // reads it (re-arms a max-pool buffer for the next forward), or NULL
  // optional prologue (head_h2 != NULL; chain B): the TNet(3) tail of ndnet_pn_head3_run computed by
  // every workgroup of a cloud before layer 0, which reads its result -- t1[b] = h2[b] @ W3^T + b3 (9
  // outputs, the identity folded into b3) and conv1 with t1 folded, written fragment-major (K padded to
  // 16) to L[0].w + b * L[0].w_cloud_stride (every workgroup writes the same bits); t1 to head_t1[b].
  // With head_h2 set, NDNET_ERR_ARG unless: head_w3, head_b3, head_basis and head_t1 are non-NULL;
  // head_K >= 1 and head_ld >= head_K; 1 <= head_kin <= 16; L[0].K == 16 (the fold writes one k-group);
  // head_nout == L[0].N; L[0].w_cloud_stride >= 16 * head_nout (each cloud its own weights); and, with
  // head_K == 256 (h2's row and W3's rows are read as one float4 per lane), head_h2 and head_w3
  // 16-byte aligned and head_ld % 4 == 0
  const float* head_h2;   // [B][head_ld], head_ld >= head_K
  int32_t head_ld, head_K;
  const float* head_w3;   // [9][head_K]
  const float* head_b3;   // [9]
  const float* head_basis;  // [9][head_kin * head_nout]
  int32_t head_kin, head_nout;  // 1 <= head_kin <= 16; head_nout == L[0].N
  float* head_t1;         // [B][9]
  // optional prologue (fold_t2 != NULL; chains C and D, layer 0 on the VALU): TNet(64)'s feature
  // transform applied through layer 0 -- x_t2 = t2[b]^T (W0 x + b0) (ndtnet.py:150-157: bmm of the
  // bn1(conv1) rows with t2, no ReLU between) -- as the per-cloud layer W0' = W0^T t2[b], b0' = b0^T t2[b],
  // computed by every workgroup in LDS before layer 0; t2[b] = fold_t2 + b * fold_ld, 64 x 64 row-major
  // (row = the input channel of conv1's output).  Layer 0 must be 64 wide; its relu flag is applied after.
  const float* fold_t2;
  int32_t fold_ld;
  // optional with fold_t2: the cloud's first workgroup also writes W0' fragment-major (K = 16, rows
  // 12..15 untouched: zero-initialise them) to fold_out_w + b * 1024 and b0' to fold_out_b + b * 64,
  // so a later chain runs the same transformed layer 0 as a plain per-cloud layer (chain D)
  float* fold_out_w;
  float* fold_out_b;
  // Fields added after the first release of this struct; zero means the behaviour above.
  //
  // head_h2 and fold_t2 may both be set (chain B with TNet(64)'s first layer collapsed into conv1): the
  // head prologue runs first and leaves W1f[b] (conv1 with t1 folded) as layer 0's weights, then the fold
  // prologue replaces them by W1f[b] fold_t2[b] -- so with no ReLU between conv1 and the folded layer,
  // layer 0 IS the pair, relu(x (W1f[b] M) + (b1 M + bM)) with L[0].relu = 1.  What the head prologue
  // publishes to L[0].w is still the plain W1f[b] (ndnet_pn_fold_t2_run and ndnet_pn_pool12_run read it),
  // bit for bit what it publishes alone.  The matrix is then loaded with the kernel's first loads, behind
  // the head prologue's round trips.
  // fold_ld == 0: one matrix shared by all clouds (else fold_ld >= 4096, one per cloud).
  // fold_bias: optional (NULL: none), [64], shared: the folded layer's own bias, added to b0' = b0^T M
  // (and to what fold_out_b receives).  NDNET_ERR_ARG with fold_bias set and fold_t2 NULL.
  // Nothing of the product is kept between launches: it is formed from the tensors as they are at the
  // launch, so an in-place re-fold of either factor is followed.
  const float* fold_bias;
  // 1: a NaN or an infinity among an input row's in_cols values enters layer 0 as NaN, whichever way
  // layer 0 runs (on the VALU, from the staged input tile, as the direct fused pair below);
  // NDNET_ERR_ARG for any value but 0 and 1.  With L[0].relu the row then
  // leaves layer 0 as zeros -- what the layered pair gives for it: conv1 (no ReLU) hands an infinity or
  // a NaN to the split-bf16 layer behind it, whose plane split (inf - inf) makes every output of that
  // row NaN, and its ReLU's maximum drops the NaN.  A collapsed first layer sets this flag to keep
  // that.  (Finite rows whose 64-wide conv1 output overflows fp32 although the composed layer's does
  // not are out of scope: there the two forms differ.)
  int32_t x_nonfinite_nan;
  int32_t reserved0;
  // A chain may open with a fused pair whose P is a prec-0 layer with K = 16 (chain D with the seg
  // head's conv1 collapsed into its first layer: P = 12 -> 512 per cloud, ReLU, fuse_next, into
  // Q = 512 -> 256 split-bf16).  The 16-wave 64-point build runs it without an input tile when
  // Q.N == 256, Q.prec != 0, x_ld % 4 == 0, x is 16-byte aligned and head_h2 is NULL: every wave keeps
  // its 16 rows' input pieces in registers as P's operand for all chunks, and P's weights stream one
  // 1 KB fp32 fragment per wave and chunk.  Every other such block, and ndnet_pn_chain_run_t32, stage
  // the tile and run the generic fused pair.
} ndnet_pn_chain;

/* Runs one chain over `batch` clouds on `stream` (a hipStream_t; NULL = default
 * stream).  Returns 0, NDNET_ERR_ARG (-20) for an inconsistent argument block
 * (layer sizes, LDS region widths, a prec above 3, split layers of different
 * prec in one chain) or NDNET_ERR_HIP (-21) on a launch failure.
 * No allocation, no synchronisation: graph-capturable. */
int ndnet_pn_chain_run(const ndnet_pn_chain *args, int batch, void *stream);
/* The same chain on 32-point tiles (8 waves per workgroup; same arguments,
 * results within fp32 summation order): for batches whose 64-point tiles
 * would leave CUs idle, e.g. 16 clouds of 500 points. */
int ndnet_pn_chain_run_t32(const ndnet_pn_chain *args, int batch, void *stream);

/* The fp16 two-slice form of a chain's prec 1 layers ("x6" accuracy class on half the matrix
 * instructions).  ndnet_pn_chain and ndnet_pn_layer are released structs of fixed size, so what the form
 * adds travels in a block of its own beside them:
 *   w16[l]      layer l's weights as two fp16 planes, [N/16][K/32][2 planes][64 lanes][8] -- the prec 1
 *               layout with two planes per k-group -- holding h = fp16(W^T 2^s), l = fp16(W^T 2^s - h),
 *               round to nearest even, with the layer-wide power of two 2^s that puts max |W^T| 2^s in
 *               [2^13, 2^14) (s = 0 for an all-zero layer; s <= 100, see ndnet_pn_fold16_run); 16-byte
 *               aligned.  NULL for a prec 0 layer.
 *   scale[l]    DEVICE pointer to one float, 2^-s, written with w16[l] by ndnet_pn_fold16_run (the kernel
 *               reads it at every launch: an in-place re-fold is followed with no host read)
 *   fallbacks   DEVICE counter, incremented once per tile that ran the bf16 form instead (below)
 * A producing epilogue stores split(16 v) as two fp16 planes (the layout, swizzle and pitch of the prec 2
 * mode's h and m planes); the consuming epilogue undoes both scales with one exact multiply folded into
 * the bias add, v = fma(acc, 2^-4 2^-s, bias), so pooled maxima and logits are true values.  Three
 * products per operand pair (h h', h l', l h').  With 11 significant bits per slice and signed
 * residuals, |x - h| <= 2^-11 |x| and |x - h - l| <= 2^-23 |x| (one bit short of fp32's 24 in the
 * worst case, exact in half of them), so the dropped l l' is at most 2^-22 |x y|.
 * fp16 has 5 exponent bits, so a tile (64 or 32 rows) takes this form only while every split layer's
 * input lies in the window: the maximum |v| over the whole input tile in [2^-4, 2^11), or the tile all
 * zero (then each element's representation error is at most max(2^-23 |v|, 2^-25 tile max); this relies
 * on the f16 MFMA keeping subnormal inputs, which the default MODE.denorm does).  The maximum is gathered
 * by the producing epilogue and tested, NaN and infinity counting as outside, after the layer barrier
 * and before the chain's first global store or atomic; a tile outside it for any split layer is run
 * again from the start by the unchanged bf16 three-slice code on L[l].w, so its result is bit for bit
 * ndnet_pn_chain_run's.  Chain B's head prologue then publishes the same bits twice.
 * ndnet_pn_chain_f16_run takes the chain block of ndnet_pn_chain_run (every split layer prec 1, its
 * bf16 `w` valid) and this block.  NDNET_ERR_ARG (-20) before any launch, beyond ndnet_pn_chain_run's
 * cases: ext or fallbacks NULL, a split layer of prec 2 or 3, a prec 1 layer whose w16 or scale is NULL
 * or whose w16 is not 16-byte aligned or whose weights are per cloud, a split layer with fuse_next (a
 * fused pair's first layer must be prec 0 here), a chain with no split layer, or a max-pooled chain
 * whose last layer is fed by a fused one (its atomics would precede the test of its input). */
typedef struct ndnet_pn_f16 {
  const void *w16[NDNET_PN_MAX_LAYERS];
  const float *scale[NDNET_PN_MAX_LAYERS];
  uint32_t *fallbacks;
} ndnet_pn_f16;
int ndnet_pn_chain_f16_run(const ndnet_pn_chain *args, const ndnet_pn_f16 *ext, int batch, void *stream);
int ndnet_pn_chain_f16_run_t32(const ndnet_pn_chain *args, const ndnet_pn_f16 *ext, int batch, void *stream);
/* Reads a fallback counter and sets it to zero, after the work queued on `stream` so far (it waits for
 * it: not graph-capturable).  Returns the count (clamped to INT32_MAX), -20 for NULL, -21 on a HIP error. */
int ndnet_pn_take_f16_fallbacks(uint32_t *device_counter, void *stream);

/* The fold of those fp16 planes, on the device from the live weights (re-run in place after a weight
 * update, like ndnet_pn_fold_run; graph-capturable, no host read).  One job per layer, with the
 * fields of ndnet_pn_fold_job's NDNET_FOLD_FRAG6 (fw(n, k), Kp % 32 == 0, Np % 16 == 0) and
 *   out      the two fp16 planes (Kp * Np * 2 halves), 16-byte aligned
 *   partial  16 floats of scratch: the launch's first kernel leaves the maxima of |fw| over 16
 *            interleaved parts of the layer here (a pass of its own: the scale needs the whole layer)
 *   scale    one float: 2^-s, s = min(13 - floor(log2(max |fw|)), 100): every finite maximum lands below
 *            2^14 (s >= -114, which fp32 holds), one below 2^-87 stays under 2^13; s = 0 for a maximum
 *            that is zero or not finite
 * Two launches in stream order: the maxima, then the planes and the scale.  ndnet_pn_fold16_check
 * validates a HOST copy of the list (NDNET_ERR_ARG for a NULL pointer, sizes that are not positive,
 * ld < k0 + K, Kp < K, Np < N, Kp % 32, Np % 16, a misaligned out, BatchNorm pointers given in part)
 * and returns the widest job's 8-element units in *max_units for ndnet_pn_fold16_run. */
typedef struct ndnet_pn_fold16_job {
  const float *w;
  const float *gamma, *var;  /* BatchNorm1d weight and running variance; both NULL: none */
  void *out;
  float *partial;
  float *scale;
  int32_t N, K;
  int32_t ld, k0;
  int32_t Kp, Np;
  float eps;
  int32_t reserved;
} ndnet_pn_fold16_job;
int ndnet_pn_fold16_check(const ndnet_pn_fold16_job *host_jobs, int num_jobs, int64_t *max_units);
int ndnet_pn_fold16_run(const ndnet_pn_fold16_job *device_jobs, int num_jobs, int64_t max_units, void *stream);

/* Timing builds only (-DNDNET_PN_STAMPS, tools/pn_stamps.py): the
 * s_memrealtime stamps (100 MHz) of every workgroup of the last chain
 * launch, [wgs][16] (0 start, 1 head prologue, 2 input tile, 3 + l after
 * layer l, 15 end), copied to host memory.  The product build returns -20. */
int ndnet_pn_debug_stamps(unsigned long long *host, int wgs);
int ndnet_pn_debug_stamps_clear(void);  /* zeroes them (timing builds; else -20) */

/* The per-cloud steps between the chains (TNet FC heads ndtnet.py:53-60 and
 * the t1 weight fold of pointnet_hip.py), for batch <= 16 clouds:
 *   ndnet_pn_fc_run:     out[b][n] = act(bias[n] + sum_k in[b][k] W[n][k]),
 *                        W row-major [N][K], K % 4 == 0, act = ReLU if relu
 *                        (Linear + folded BatchNorm1d + ReLU, ndtnet.py:55-56)
 *   ndnet_pn_head3_run:  t1[b] = h2[b] @ W3^T + b3 (9 outputs; the TNet
 *                        identity folded into b3, ndtnet.py:57-60) and
 *                        w1f[b] = t1[b] @ basis ([9][kin * nout] row-major) --
 *                        conv1 with t1 folded, written fragment-major with K
 *                        padded to 16 (16 * nout floats per cloud)
 * NDNET_ERR_ARG (-20) before any launch: ndnet_pn_fc_run for a NULL pointer,
 * batch outside 1..16, K < 1 or K % 4, N < 1, ld_in % 4, ld_in < K,
 * ld_out < N, or `in` / W not 16-byte aligned; ndnet_pn_head3_run (h2
 * [batch][ld_h], W3 [9][K]) for a NULL pointer, batch < 1, K < 1, ld_h < K,
 * kin outside 1..16, nout < 1 or nout % 16.
 * Same return codes as ndnet_pn_chain_run; graph-capturable. */
int ndnet_pn_fc_run(const float *in, int ld_in, const float *W, const float *bias, float *out, int ld_out,
                    int batch, int K, int N, int relu, void *stream);
/* The same FC layer on the fp32 MFMA (the default): Wf = W^T in the chain's
 * fragment-major layout ([N/16][K/16][64 lanes][4], as ndnet_pn_layer.w with
 * prec 0), K % 16 == 0, K <= 1024, N % 16 == 0; one launch of N / 16
 * workgroups, each summing its waves' K-slices in a fixed order. */
int ndnet_pn_fc_mfma_run(const float *in, int ld_in, const float *Wf, const float *bias, float *out, int ld_out,
                         int batch, int K, int N, int relu, void *stream);
/* The same with a bias row per cloud: out[b][n] = act(bias[b * bias_ld + n] + ...), bias_ld >= N, or
 * bias_ld == 0 for one shared row -- then it is ndnet_pn_fc_mfma_run, bit for bit (that entry forwards
 * here).  The seg head's per-cloud bias with conv1 collapsed into chain D's first layer:
 * cvec[b] = g3[b] s1g^T + bd[b] (ndnet_pn_fold_seg_run).  NDNET_ERR_ARG (-20) as ndnet_pn_fc_mfma_run,
 * and for 0 < bias_ld < N. */
int ndnet_pn_fc_mfma_bias_run(const float *in, int ld_in, const float *Wf, const float *bias, int bias_ld, float *out,
                              int ld_out, int batch, int K, int N, int relu, void *stream);
/* The classification head's last layer and softmax (ndtnet.py:188-194: conv3
 * then softmax over the classes; no BatchNorm) in one launch, for any batch:
 *   probs[b][c] = softmax_c(bias[c] + sum_k in[b][k] W^T[k][c]),  c < out_cols
 * Wf = W^T fragment-major as for ndnet_pn_fc_mfma_run (K x N, prec-0 layout),
 * K % 16 == 0, K <= 256, N % 16 == 0, N <= 1024, 1 <= out_cols <= N (columns
 * at or past out_cols are padding: computed, never part of the maximum or the
 * sum, never written), batch >= 1; in and Wf 16-byte aligned, ld_in % 4 == 0,
 * ld_in >= K, ld_probs >= out_cols (and ld_logits >= out_cols with logits).
 * One workgroup per 16 clouds, ceil(batch / 16) of them, none waiting for
 * another; the 16 x N logits stay in LDS, a column's K-sum is formed by one
 * wave in a fixed order (bit-identical from run to run), the exponential is
 * the accurate expf of x - max and the division a true one.
 *   logits  optional (NULL: not written): the pre-softmax values, [batch][ld_logits]
 *   clear   optional (NULL with clear_count 0): clear[0 .. clear_count) is set
 *           to -inf, the workgroups sharing the range -- re-arms the max-pool
 *           buffer for the next forward.  The kernel reads nothing of it, so
 *           it must not overlap in, Wf or bias; its last reader must be
 *           earlier in stream order.
 * Same return codes as ndnet_pn_chain_run (-20 before any launch, -21 on a
 * launch failure); no allocation, no synchronisation: graph-capturable. */
int ndnet_pn_cls_head_run(const float *in, int ld_in, const float *Wf, const float *bias, float *probs,
                          int ld_probs, float *logits, int ld_logits, int batch, int K, int N, int out_cols,
                          float *clear, int64_t clear_count, void *stream);
/* BatchNorm fold of the eval forward's weights, re-run in place after a
 * weight update (the host-side first fold: pointnet_hip._Folded; the folds
 * it restates: ndtnet.py's Conv1d / Linear + BatchNorm1d pairs, :45-60,
 * :148-161, :218-241, with running statistics).  One job writes one output
 * tensor from one layer's parameters; the folded weight of layer row n and
 * input column k is
 *   fw(n, k) = w[n * ld + k0 + k] * (gamma[n] / sqrt(var[n] + eps))
 * (no BatchNorm: gamma == NULL, fw = w), every operation a separately
 * rounded fp32 operation as torch computes the fold.  Kinds:
 *   NDNET_FOLD_WT     out[k][n] (Kp x Np floats) = fw(n, k), zero padded
 *   NDNET_FOLD_FRAG   the same W^T fragment-major (ndnet_pn_layer.w, prec 0)
 *   NDNET_FOLD_FRAG6  the same W^T split-bf16 (ndnet_pn_layer.w, prec 1, 2 and 3;
 *                     bf16 rounding to nearest even, residuals exact)
 *   NDNET_FOLD_ROWS   out[n][k] (N x K floats) = fw(n, k)
 *   NDNET_FOLD_BASIS  TNet(3)'s t1 basis of conv1 (K == 12):
 *                     out[3a + c][r][n] = E_ac^T fw^T with E_ac the 0/1
 *                     matrix of p -> t1 p, C -> t1 C (pointnet_hip._Folded)
 *   NDNET_FOLD_BIAS   out[n] (Np floats) = (bias[n] - mean[n]) * s[n] + beta[n]
 *                     (no BatchNorm: bias[n]), + 1 on the diagonal of an
 *                     eye x eye matrix when eye > 0, zero padded
 *   NDNET_FOLD_PROD   a product of two tensors that other jobs of the list write
 *                     (or of any fp32 tensors), for the forward's weight-only products:
 *                       out[r][n] = sum_k w[r * ld + k0 + k] * rhs[k * Np + n]  (+ bias[n]),
 *                     r < N, k < K, n < Np; `w` is the left factor as it is (no BatchNorm:
 *                     gamma must be NULL), rhs the right one, K x Np row-major, bias an
 *                     optional row added to every output row.  Each fp32 x fp32 product is
 *                     exact in double; the sum runs in double with k ascending (bias last)
 *                     and is rounded once at the store.  out_f64 = 1 stores the doubles
 *                     themselves: `out` is then N x Np DOUBLES -- the one output type of
 *                     the table that is neither fp32 nor bf16 (ndnet_pn_pool12_tail_run's
 *                     w23 and b23) -- else N x Np floats.
 *                     PROD jobs read what the other kinds write, so they must be the
 *                     list's last jobs; ndnet_pn_fold_run runs them as a second launch
 *                     behind the first, in stream order.
 * ndnet_pn_fold_prepare validates a host copy of the job list and fills each
 * job's block0 (its first workgroup), returning the grid size in
 * *num_blocks (the list's workgroups in the lower 32 bits, those of its PROD
 * jobs in the upper: pass it on as it is); ndnet_pn_fold_run then runs the
 * list from DEVICE memory in one launch, two with PROD jobs
 * (graph-capturable, no allocation).  NDNET_ERR_ARG (-20) on an invalid job
 * or a PROD job followed by one of another kind. */
#define NDNET_FOLD_WT 0
#define NDNET_FOLD_FRAG 1
#define NDNET_FOLD_FRAG6 2
#define NDNET_FOLD_ROWS 3
#define NDNET_FOLD_BASIS 4
#define NDNET_FOLD_BIAS 5
#define NDNET_FOLD_PROD 6
typedef struct ndnet_pn_fold_job {
  const float *w;                          /* layer weight, rows of ld floats (not read by BIAS) */
  const float *bias;                       /* layer bias [N] (BIAS only) */
  const float *gamma, *beta, *mean, *var;  /* BatchNorm1d weight, bias, running mean / var; NULL: none */
  void *out;                               /* the output tensor (bf16 for FRAG6, double for PROD with out_f64,
                                              else fp32), 16-byte aligned */
  int32_t kind;
  int32_t N, K;                            /* layer rows (outputs) and the input columns used */
  int32_t ld, k0;                          /* row stride of w and the first column used */
  int32_t Kp, Np;                          /* padded sizes (WT / FRAG / FRAG6: Kp x Np; BIAS: Np) */
  int32_t eye;
  float eps;
  int32_t reserved;
  int64_t block0;                          /* filled by ndnet_pn_fold_prepare */
  /* Fields added after the first release of this struct (PROD only; zero otherwise). */
  const float *rhs;                        /* the right factor, K x Np floats row-major */
  int32_t out_f64;                         /* 1: `out` is N x Np doubles; 0: floats */
  int32_t reserved1;
} ndnet_pn_fold_job;
int ndnet_pn_fold_prepare(ndnet_pn_fold_job *host_jobs, int num_jobs, int64_t *num_blocks);
int ndnet_pn_fold_run(const ndnet_pn_fold_job *device_jobs, int num_jobs, int64_t num_blocks, void *stream);

int ndnet_pn_head3_run(const float *h2, int ld_h, const float *W3, const float *b3, const float *basis,
                       float *t1, float *w1f, int batch, int K, int kin, int nout, void *stream);

/* TNet(64)'s transform through conv1 (ndtnet.py:152-155), once per cloud, for
 * chains C and D's layer 0 (round 5; chain C's fold_t2 prologue did it per
 * workgroup): outf[b] = (w1f[b] as W1'^T, 12 of its 16 rows) @ t2[b] in the
 * fragment-major K = 16 layout (rows 12..15 untouched), outb[b] = b1^T t2[b].
 * w1f [batch][w1_stride >= 1024], b1 [64], t2 [batch][t2_ld >= 4096] (16-byte
 * aligned), outf [batch][1024], outb [batch][64]. */
int ndnet_pn_fold_t2_run(const float *w1f, int w1_stride, const float *b1, const float *t2, int t2_ld, float *outf,
                         float *outb, int batch, void *stream);

/* ndnet_pn_fold_t2_run and, in the same launch, the seg head's conv1 collapsed into chain D's first
 * layer.  x_t2 = x W1''[b] + b1''[b] (outf, outb) feeds the seg head's conv1[:, :64] with no ReLU between
 * (ndtnet.py:152-157, :227-233), so the two are one per-cloud 12 -> N2 layer:
 *   wd[b] = W1''[b] s1aT      (12 x N2) in the fragment-major K = 16 layout, 16 * N2 floats per cloud;
 *                             rows 12..15 are left untouched: zero-initialise them
 *   bd[b] = b1''[b] s1aT + s1b   (N2 floats; the per-cloud global-feature term is added by
 *                             ndnet_pn_fc_mfma_bias_run)
 * from the fp32 values of W1''[b], b1''[b] just written, the products accumulated in double (i
 * ascending) and rounded once to fp32.  outf and outb are written exactly as ndnet_pn_fold_t2_run
 * writes them, bit for bit (ndnet_pn_pool12_run reads them).  Nothing is cached: every launch reads
 * the tensors as they are, so an in-place re-fold is followed.
 *   w1f, w1_stride, b1, t2, t2_ld, outf, outb   as ndnet_pn_fold_t2_run
 *   s1aT   [64][N2] row-major (the seg head's conv1[:, :64]^T, BatchNorm folded), 16-byte aligned
 *   s1b    [N2];  N2 a multiple of 64
 *   wd     [batch][wd_stride >= 16 * N2];  bd [batch][bd_stride >= N2]
 * One launch of (N2 / 64, batch) workgroups for any batch in 1..65535; bit-identical from run to run.
 * NDNET_ERR_ARG (-20) before any launch for a NULL pointer, batch outside 1..65535, a stride below
 * its minimum, t2_ld % 4, N2 < 1 or N2 % 64, or t2 / s1aT not 16-byte aligned; -21 on a launch
 * failure.  No allocation, no synchronisation: graph-capturable. */
int ndnet_pn_fold_seg_run(const float *w1f, int w1_stride, const float *b1, const float *t2, int t2_ld, float *outf,
                          float *outb, const float *s1aT, const float *s1b, int N2, float *wd, int64_t wd_stride,
                          float *bd, int64_t bd_stride, int batch, void *stream);

/* Chain C (conv1 with t1 and t2 folded, conv2, conv3, max over points) as one
 * per-cloud 12 -> F layer: no ReLU separates the three (ndtnet.py:149-161),
 * so with y0 = x W0[b] + b0[b], y1 = y0 w_mid + b_mid, y2 = y1 w_tail + b_tail
 *   gmax[b][f] = max_n (sum_k x[b][n][k] Wc[b][k][f]) + bc[b][f],   f < Fp,
 *   Wc[b] = W0[b] w_mid w_tail,  bc[b] = (b0[b] w_mid + b_mid) w_tail + b_tail.
 * Fp is 32 or a multiple of 64, as a chain layer's N.  One launch of
 * (ceil(Fp / 64), batch) workgroups.  Each forms its 64 columns of
 * [Wc; bc] from the tensors as they are at the launch (products in double,
 * rounded once to fp32; nothing is cached, so an in-place re-fold is picked
 * up), then streams the cloud's rows: 12 fp32 multiply-adds per point and
 * column with k ascending (v_mfma_f32_16x16x4_f32, fp32 products and sums),
 * the maximum over the points, the bias added to the maximum, one plain
 * store per column.  No atomics: gmax needs no -inf before the
 * launch and is written only in columns 0 .. Fp - 1 of its rows.
 *   x       [batch][num_points][x_ld], columns 0..11 read; x_ld >= 12, x_ld % 4 == 0
 *   w0f     [batch][w0_stride >= 1024]: W0[b] (12 x 64) in the fragment-major K = 16
 *           layout ndnet_pn_fold_t2_run writes (rows 12..15 are not read)
 *   b0      [batch][b0_stride >= 64]
 *   w_mid   W2'^T [64][128] row-major, b_mid [128]
 *   w_tail  W3'^T [128][Fp] row-major, b_tail [Fp]; columns F .. Fp - 1 of both are zero
 *           padding, which leaves those columns of gmax at exactly 0
 *   gmax    [batch][gmax_ld >= Fp]
 * As the chain's pooled epilogue: a NaN never wins the maximum, -0 is stored
 * as +0, and a column no row reached is stored as -inf.  A row holding a NaN
 * or an infinity takes no part (the layered chain's split-bf16 layers turn an
 * infinite activation into NaNs, which the maximum drops).  Bit-identical
 * from run to run.  NDNET_ERR_ARG (-20) before any launch for a NULL pointer,
 * batch outside 1..65535, num_points < 1, a stride below its minimum,
 * x_ld % 4, F outside 1..Fp, Fp neither 32 nor a multiple of 64, or
 * gmax_ld < Fp; -21 on a launch
 * failure.  No allocation, no synchronisation: graph-capturable. */
int ndnet_pn_pool12_run(const float *x, int x_ld, int num_points, const float *w0f, int64_t w0_stride,
                        const float *b0, int64_t b0_stride, const float *w_mid, const float *b_mid,
                        const float *w_tail, const float *b_tail, int F, int Fp, float *gmax, int gmax_ld,
                        int batch, void *stream);

/* The same launch from the composed tail: w_mid w_tail and its bias row do not
 * depend on the cloud, so the fold forms them once (two NDNET_FOLD_PROD jobs
 * with out_f64 = 1, re-run by every in-place re-fold) and each workgroup's
 * slice is the one product
 *   [Wc[b]; bc[b]] = [W0[b]; b0[b]] w23  (+ b23 on the bias row),
 *   w23 = w_mid w_tail (64 x Fp doubles, row-major),  b23 = b_mid w_tail + b_tail (Fp doubles),
 * on the f64 MFMA, rounded once to fp32 -- a quarter of ndnet_pn_pool12_run's
 * matrix work per workgroup and no intermediate.  The value differs from that
 * entry's only in the order of the double sums (W0 (w_mid w_tail) for
 * (W0 w_mid) w_tail).  Everything after it -- the rows, the NaN and infinity
 * rule, the maximum, the store, the grid -- is ndnet_pn_pool12_run's, and so
 * are the other arguments and the return codes; w23 and b23 must be 8-byte
 * aligned.  Nothing is cached: w23 and b23 are read at every launch. */
int ndnet_pn_pool12_tail_run(const float *x, int x_ld, int num_points, const float *w0f, int64_t w0_stride,
                             const float *b0, int64_t b0_stride, const double *w23, const double *b23, int Fp,
                             float *gmax, int gmax_ld, int batch, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* NDNET_POINTNET_H_ */
