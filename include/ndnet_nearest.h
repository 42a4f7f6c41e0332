/*
 * ndnet_nearest.h -- the PointNet-on-FPS baseline's device steps on gfx950
 * (libndnet_amd.so, ndt-net_amd/csrc/nearest_kernels.hip).
 *
 * ndnet_nearest_sample_run: for every point of a [B][n][3] batch, the index of
 * the nearest of its cloud's samples ([B][S][3], e.g. the farthest-point
 * samples a PointNet labelled) -- the baseline's counterpart of
 * ndnet_ndt_point_rows.  The rows go unchanged into ndnet_seg_point_labels,
 * ndnet_seg_confusion and ndnet_seg_row_hist.  Device pointers, stream ordered,
 * no allocation and no synchronisation (capturable).  Return codes as
 * ndnet_amd.h: NDNET_OK, NDNET_ERR_ARG (checked before any launch),
 * NDNET_ERR_HIP.
 *
 * Per cloud b, in float32, every operation rounded and nothing fused (the
 * distance expression of ndnet_fps.h):
 *
 *   m  = d_counts ? clamp(d_counts[b], 0, n) : n
 *   ms = d_sample_counts ? clamp(d_sample_counts[b], 0, S) : S
 *   for i < m:  best = +inf; row = -1
 *               for t in 0 .. ms:  dx = p[i].x - s[t].x, dy, dz likewise
 *                                  d = (dx*dx + dy*dy) + dz*dz
 *                                  if (d < best) { best = d; row = t }    (false for NaN; ties keep the smaller t)
 *               d_rows[b][i] = row;  d_dist[b][i] = best
 *   for m <= i < n:  d_rows[b][i] = -1   (d_dist not written)
 *
 * So: a point with a non-finite coordinate gets -1 (every d is NaN or +inf,
 * and neither is less than +inf); a non-finite sample is never chosen (for the
 * same reason); a point that is itself a sample gets the smallest t at
 * distance 0.  Points past d_counts[b] and samples past d_sample_counts[b] are
 * never read.  The search is exhaustive: no grid, no atomics, no state shared
 * between workgroups.
 *
 * ndnet_pn_transform3_run: the baseline's input transform with the reference's
 * nan_to_num (models/pointnet.py:114-117), one launch between TNet(3)'s head
 * and the shared conv1 (nan_to_num is not linear, so t1 cannot be folded into
 * conv1's weights as the NDT model's chain B does):
 *
 *   out[b][i][a] = fix(((t[b][a][0]*x + t[b][a][1]*y) + t[b][a][2]*z))   a = 0, 1, 2; every operation rounded
 *   fix: NaN -> 0, +inf -> FLT_MAX, -inf -> -FLT_MAX
 */
#ifndef NDNET_NEAREST_H_
#define NDNET_NEAREST_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* A workgroup owns a tile of this many points of one cloud (256 threads, four
 * points each, coordinates and the running (best, row) in registers) ... */
#define NDNET_NN_TILE_POINTS 1024
/* ... and walks the cloud's samples in chunks of this many, staged in LDS
 * (16 bytes a sample; every lane reads the same one at a time: a broadcast). */
#define NDNET_NN_CHUNK_SAMPLES 1024

/* d_points [B][n][3]; d_counts NULL or [B] int32; d_samples [B][S][3]; d_sample_counts NULL or
 * [B] int32; d_rows [B][n] int32; d_dist NULL (not written) or [B][n] float.
 * NDNET_ERR_ARG for a NULL d_points, d_samples or d_rows, B < 1, n < 1, S < 1, n >= 2^31 or
 * S >= 2^31 (and for B > 65535, the grid's second extent). */
int ndnet_nearest_sample_run(const float *d_points, int B, uint64_t n, const int32_t *d_counts,
                             const float *d_samples, uint64_t S, const int32_t *d_sample_counts,
                             int32_t *d_rows, float *d_dist, void *stream);

/* d_points [B][n] rows of p_ld floats (the first three are read); d_t1 [B][9] row-major; d_out
 * [B][n] rows of o_ld floats (the first three are written).  NDNET_ERR_ARG for a NULL pointer,
 * B < 1, B > 65535, n < 1, n >= 2^31, p_ld < 3 or o_ld < 3. */
int ndnet_pn_transform3_run(const float *d_points, int64_t p_ld, const float *d_t1, float *d_out, int64_t o_ld,
                            int B, uint64_t n, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* NDNET_NEAREST_H_ */
