/*
 * ndnet_augment.h -- train-time augmentation of a point-cloud batch on gfx950
 * (libndnet_amd.so): a random yaw, scale, flip and shift per cloud, jitter per
 * point and random point dropout as a stable compaction that writes the new
 * per-cloud counts.  Device pointers, stream ordered, no allocation and no
 * synchronisation (capturable); the random state is a step counter in device
 * memory that every call advances, so a replayed graph draws anew each time.
 * Return codes as ndnet_amd.h: NDNET_OK, NDNET_ERR_ARG (checked before any
 * launch), NDNET_ERR_HIP.
 *
 * Random numbers: Philox4x32-10 (multipliers 0xD2511F53 / 0xCD9E8D57, key
 * increments 0x9E3779B9 / 0xBB67AE85, the key bumped after each round):
 *
 *   round:   c' = (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0))
 *   key:     (seed, stream)
 *   counter: (i, b, uint32(step), (uint32(step >> 32) << 2) | purpose),  step < 2^62
 *
 * step is read from *d_step at the start of the call, which leaves step + 1.
 *
 * Per cloud b (purpose 0): P = philox(i = 0), Q = philox(i = 1),
 * u(w) = double(w >> 8) * 2^-24.  In double, every operation rounded, nothing
 * fused (cos and sin are the device library's):
 *
 *   theta = (2 u(P0) - 1) * yaw_max
 *   s     = scale_lo + u(P1) * (scale_hi - scale_lo)
 *   fx    = (P2 & 0xffff) < flip_x_16 ? -1 : 1,   fy = (P2 >> 16) < flip_y_16 ? -1 : 1
 *   T     = uint32(floor(u(P3) * drop_max * 2^32))
 *   t[a]  = (2 u(Q[a]) - 1) * shift_max[a]
 *   c = cos(theta), z = sin(theta), sc = s * c, sz = s * z
 *   M = s diag(fx, fy, 1) Rz(theta):  m00 = fx * sc   m01 = fx * -sz   m02 = 0
 *                                     m10 = fy * sz   m11 = fy * sc    m12 = 0
 *                                     m20 = 0         m21 = 0          m22 = s
 *
 * Each of the 12 entries of [M | t] is rounded once to float32; a cloud's row
 * of d_xform is  m00 m01 m02 tx  m10 m11 m12 ty  m20 m21 m22 tz.
 *
 * Per point i < m (m = d_counts ? clamp(d_counts[b], 1, n) : n; padding is
 * never read): W0..W3 = philox(purpose 1), W4..W7 = philox(purpose 2).
 *
 *   keep  = i == 0 || W6 >= T                       (point 0 always survives)
 *   S[a]  = lo16(W[2a]) + hi16(W[2a]) + lo16(W[2a+1]) + hi16(W[2a+1])       (integers)
 *   j[a]  = float(jitter_sigma) * (float(S[a] - 131070) * K),  K = float(sqrt(3.0) / 65536.0)
 *   x'    = (((m00 x + m01 y) + m02 z) + tx) + j[0],  y' and z' likewise     (float32, each rounded)
 *
 * j is a sum of four uniforms scaled to unit variance, within 3.47 sigma.  W7
 * is reserved.  The kept points of cloud b go, in input order, to the rows
 * 0 .. m' - 1 of d_out_points[b], their labels to d_out_labels[b], and
 * d_out_counts[b] = m'; rows >= m' are not written.
 */
#ifndef NDNET_AUGMENT_H_
#define NDNET_AUGMENT_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Points per workgroup of the keep-count and the apply pass. */
#define NDNET_AUG_TILE 1024

typedef struct ndnet_aug_config {
  uint32_t seed, stream;   /* the Philox key; stream: the rank under data parallelism */
  double yaw_max;          /* radians, >= 0 */
  double scale_lo, scale_hi; /* 0 < scale_lo <= scale_hi */
  double shift_max[3];     /* >= 0 */
  double drop_max;         /* in [0, 1]: a cloud's drop probability is uniform in [0, drop_max) */
  double jitter_sigma;     /* >= 0; used rounded to float32 */
  uint32_t flip_x_16, flip_y_16; /* flip probability in 1 / 65536, <= 65536 */
} ndnet_aug_config;

/* Bytes of d_work for a [B][n][3] batch: the step's snapshot, the clouds'
 * matrices and thresholds and one count per tile of NDNET_AUG_TILE points.
 * 0 for B < 1, n < 1 or n >= 2^31.  After a call the buffer holds
 *   uint64 step (the call's), 8 bytes unused, float xform[B][12], uint32 T[B],
 *   uint32 kept[B][ceil(n / NDNET_AUG_TILE)] (written with drop_max > 0 only). */
size_t ndnet_aug_work_bytes(int B, uint64_t n);

/* d_points [B][n][3] float32; d_labels NULL or [B][n] int32; d_counts NULL or [B] int32;
 * d_step one uint64 on the device; d_work ndnet_aug_work_bytes(B, n) bytes, 16-byte aligned,
 * the caller's, private to the call until it has run; d_out_points [B][n][3];
 * d_out_labels [B][n] exactly when d_labels is given; d_out_counts [B] int32; d_xform NULL or
 * [B][12] float32.  With drop_max == 0 the call may run in place (d_out_points == d_points,
 * d_out_labels == d_labels); with drop_max > 0 the outputs must not overlap the inputs.
 * Launches: the parameters (one workgroup), with drop_max > 0 the keep counts per tile, and
 * the apply pass, which sums its cloud's preceding tile counts itself (one load per thread up
 * to 256 tiles); no workgroup waits on another.
 * NDNET_ERR_ARG for a NULL cfg, d_points, d_step, d_work, d_out_points or d_out_counts,
 * labels in without labels out or the reverse, B < 1, B > 65535, n < 1, n >= 2^31,
 * d_out_points == d_points or d_out_labels == d_labels while drop_max > 0, scale_lo <= 0,
 * scale_lo > scale_hi, drop_max outside [0, 1], a negative or NaN yaw_max, shift_max or
 * jitter_sigma, or a flip threshold above 65536. */
int ndnet_aug_run(const ndnet_aug_config *cfg, const float *d_points, const int32_t *d_labels,
                  const int32_t *d_counts, int B, uint64_t n, uint64_t *d_step, void *d_work,
                  float *d_out_points, int32_t *d_out_labels, int32_t *d_out_counts, float *d_xform,
                  void *stream);

#ifdef __cplusplus
}
#endif

#endif /* NDNET_AUGMENT_H_ */
