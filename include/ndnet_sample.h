/*
 * ndnet_sample.h -- an exact-size random subsample of every cloud of a ragged
 * batch on gfx950 (libndnet_amd.so), and the gather of points and labels by
 * given indices.  Device pointers, stream ordered, no allocation and no
 * synchronisation (capturable); the random state is a step counter in device
 * memory, as ndnet_augment.h has it, so a replayed graph draws anew each time.
 * Return codes as ndnet_amd.h: NDNET_OK, NDNET_ERR_ARG (checked before any
 * launch), NDNET_ERR_HIP.
 *
 * The definition is integer only.  Philox4x32-10, its key and its counter are
 * those of ndnet_augment.h; the purpose field is 3, the one value the
 * augmentation leaves unused, so a sampler and an augmentation that share a
 * seed draw independently.
 *
 *   cfg: seed, stream (the Philox key, as ndnet_aug_config), key_bits in 1..32
 *   step = *d_step at the start of the call; the call leaves step + 1 if advance != 0, else step
 *   per cloud b:  m = d_counts ? clamp(d_counts[b], 1, n) : n
 *     key[i] = philox(counter = (i, b, uint32(step), (uint32(step >> 32) << 2) | 3), key = (seed, stream)).word0
 *              >> (32 - key_bits)                                   for i < m   (padding is never read)
 *     m' = min(m, S)
 *     chosen = every i < m if m <= S, else the S points smallest in (key[i], i), compared lexicographically
 *     the chosen points in ascending i are rows t = 0 .. m'-1:
 *         out_indices[b][t] = i, out_points[b][t] = p[b][i], out_labels[b][t] = labels[b][i]
 *     rows m' <= t < S:  out_indices = -1, out_points = p[b][0], out_labels = fill_label
 *     out_counts[b] = m'
 *
 * With tau the S-th smallest key, the chosen set is {key < tau} and the first
 * S - #{key < tau} indices among {key == tau}.  key_bits is 32 in every
 * product path; fewer bits force ties (at 1 bit the tie rule decides most of
 * the set), which is what tests use it for.
 */
#ifndef NDNET_SAMPLE_H_
#define NDNET_SAMPLE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Points per workgroup of the key, the count and the apply pass. */
#define NDNET_SAMPLE_TILE 1024
/* The most keys of one radix bin the threshold search keeps in LDS; a larger
 * bin is re-read from the keys in d_work once per further 8 bits. */
#define NDNET_SAMPLE_LIST 1024

typedef struct ndnet_sample_config {
  uint32_t seed, stream; /* the Philox key; stream: the rank under data parallelism */
  int32_t key_bits;      /* 1 .. 32: the bits of word 0 that make the sort key */
} ndnet_sample_config;

/* Bytes of d_work for a [B][n][3] batch; 0 for B < 1, n < 1 or n >= 2^31.
 * After a call the buffer holds
 *   uint64 step (the call's), 8 bytes unused, uint32 tau[B], uint32 quota[B]
 *   (clouds with m > S only), uint32 hist[B][256] (the keys' top 8 bits),
 *   uint32 below_equal[B][ceil(n / NDNET_SAMPLE_TILE)][2], padding to 16 bytes,
 *   uint32 key[B][n rounded up to 4]. */
size_t ndnet_sample_work_bytes(int B, uint64_t n);

/* d_points [B][n][3] float32; d_labels NULL or [B][n] int32; d_counts NULL or [B] int32;
 * d_step one uint64 on the device; d_work ndnet_sample_work_bytes(B, n) bytes, 16-byte
 * aligned, the caller's, private to the call until it has run and written anew by every
 * call; d_out_points [B][S][3]; d_out_labels [B][S] exactly when d_labels is given;
 * d_out_counts [B] int32; d_out_indices NULL or [B][S] int32.
 * Launches: the step and the cleared histograms (one workgroup per cloud); the keys and
 * the histogram of their top 8 bits per tile; the threshold (one workgroup of 1024 threads
 * per cloud: 8 bits per pass, on the bin's keys in LDS when they are at most
 * NDNET_SAMPLE_LIST); the tiles' counts below and at the threshold; the apply pass, which
 * sums its cloud's preceding tile counts itself and writes the rows.  No workgroup waits on
 * another.
 * NDNET_ERR_ARG for a NULL cfg, d_points, d_step, d_work, d_out_points or d_out_counts,
 * labels in without labels out or the reverse, B < 1, B > 65535, n < 1, n >= 2^31,
 * S < 1, S > n, key_bits outside 1 .. 32, an output that overlaps d_points, d_labels,
 * d_counts, d_step, d_work or another output, or d_work overlapping one of those inputs. */
int ndnet_sample_random_run(const ndnet_sample_config *cfg, const float *d_points, const int32_t *d_labels,
                            const int32_t *d_counts, int B, uint64_t n, uint64_t S, int32_t fill_label,
                            int advance, uint64_t *d_step, void *d_work, float *d_out_points,
                            int32_t *d_out_labels, int32_t *d_out_counts, int32_t *d_out_indices, void *stream);

/* The apply pass alone, for indices from elsewhere (farthest point sampling): d_indices
 * [B][S] int32; a row with 0 <= d_indices[b][t] < n takes that point and label, any other
 * p[b][0] and fill_label; d_out_counts[b] = the number of such rows of cloud b.  One launch.
 * NDNET_ERR_ARG for a NULL d_points, d_indices, d_out_points or d_out_counts, labels in
 * without labels out or the reverse, B < 1, B > 65535, n < 1, n >= 2^31, S < 1, S >= 2^31,
 * or an output that overlaps an input or another output. */
int ndnet_sample_gather_run(const float *d_points, const int32_t *d_labels, const int32_t *d_indices, int B,
                            uint64_t n, uint64_t S, int32_t fill_label, float *d_out_points,
                            int32_t *d_out_labels, int32_t *d_out_counts, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* NDNET_SAMPLE_H_ */
