/*
 * ndnet_fps.h -- farthest point sampling on gfx950 (libndnet_amd.so).
 *
 * Picks n_samples of the points of every cloud of a [B][n][3] batch, each the
 * point farthest from the ones picked before it; with d_counts the clouds may
 * have different lengths (a ragged batch padded to n).  Device pointers,
 * stream ordered, no allocation and no synchronisation (capturable).  Return
 * codes as ndnet_amd.h: NDNET_OK, NDNET_ERR_ARG (checked before any launch),
 * NDNET_ERR_HIP.
 *
 * Per cloud b, in the point type T (float or double, every operation rounded
 * in T, nothing fused):
 *
 *   m = d_counts ? d_counts[b] : n;  cur = d_start ? d_start[b] : 0   (cur clamped into [0, m))
 *   mind[0..m) = +inf
 *   for t in 0 .. min(n_samples, m):
 *       indices[t] = cur;  mind[cur] = -1
 *       for every j < m:  dx = p[j].x - p[cur].x, dy, dz likewise
 *                         d = (dx*dx + dy*dy) + dz*dz
 *                         if (d < mind[j]) mind[j] = d          (false for NaN: mind keeps its value)
 *       cur = the smallest j with mind[j] == max over j of mind[j]
 *   indices[t] = -1 for t >= m
 *
 * The indices of a cloud are distinct even among duplicate points; a point
 * with a non-finite coordinate keeps +inf, so it is picked early and once.
 */
#ifndef NDNET_FPS_H_
#define NDNET_FPS_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* One workgroup of this many threads per cloud; thread i owns the points i, i + THREADS, ... */
#define NDNET_FPS_THREADS 512
/* The coordinates of a cloud's first LDS_POINTS points stay in LDS (144 KiB of
 * it); those of the others stream from L2 on every sample. */
#define NDNET_FPS_LDS_POINTS_F32 12288
#define NDNET_FPS_LDS_POINTS_F64 6144
/* The running distances of a cloud's first REG_POINTS points stay in registers
 * (196 floats or 96 doubles per thread); those of the others are kept in
 * d_min_dist and make a round trip through L2 on every sample. */
#define NDNET_FPS_REG_POINTS_F32 100352
#define NDNET_FPS_REG_POINTS_F64 49152
/* The register tier is walked in chunks of this many slabs whose loads are in flight together. */
#define NDNET_FPS_CHUNK_SLABS_F32 7
/* The same for double (24 registers of coordinates, against float's 21). */
#define NDNET_FPS_CHUNK_SLABS_F64 4

/* d_points [B][n][3]; d_counts NULL or [B] int32 with 1 <= d_counts[b] <= n (only the first
 * d_counts[b] points of cloud b exist, the others are never read; a value outside the range
 * is clamped into it); d_start NULL (index 0) or [B] int32; d_min_dist [B][n] of the point
 * type, caller scratch and an output: the final squared distance of every existing point to
 * the picked set, -1 for a picked point (entries past d_counts[b] are not written);
 * d_indices [B][n_samples] int32.
 * NDNET_ERR_ARG for a NULL d_points, d_min_dist or d_indices, B < 1, n < 1, n_samples < 1,
 * n_samples > n or n >= 2^31. */
int ndnet_fps_run(const float *d_points, int B, uint64_t n, uint64_t n_samples, const int32_t *d_counts,
                  const int32_t *d_start, void *d_min_dist, int32_t *d_indices, void *stream);
int ndnet_fps_run_f64(const double *d_points, int B, uint64_t n, uint64_t n_samples, const int32_t *d_counts,
                      const int32_t *d_start, void *d_min_dist, int32_t *d_indices, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* NDNET_FPS_H_ */
