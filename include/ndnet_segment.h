/*
 * ndnet_segment.h -- per-point segmentation labels on gfx950 (libndnet_amd.so).
 *
 * NDTNetSegmentation scores NDs ([B][k][C + 1] log-probs, one row per ND);
 * ndnet_ndt_point_rows (ndnet_amd.h) gives the row every input point was
 * folded into.  These plan-free entry points turn the two into a class per
 * point and count a point-level confusion matrix.  Device pointers, stream
 * ordered, no allocation and no synchronisation (capturable).  Return codes
 * as ndnet_amd.h: NDNET_OK, NDNET_ERR_ARG (checked before any launch),
 * NDNET_ERR_HIP.
 */
#ifndef NDNET_SEGMENT_H_
#define NDNET_SEGMENT_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* d_nd_labels[b][r] = first argmax of d_scores[b][r][0..cols) (NaN counts as a maximum, as
 * ndnet_row_argmax / torch.argmax); d_point_labels[b][i] = d_nd_labels[b][row] or `unassigned`
 * where d_point_rows[b][i] < 0 (or >= k).  d_nd_labels is caller scratch and an output.
 * d_scores [B][k][cols] float32, d_point_rows and d_point_labels [B][n] int32, d_nd_labels [B][k] int32.
 * NDNET_ERR_ARG for a NULL pointer or B, n, k or cols < 1. */
int ndnet_seg_point_labels(const float *d_scores, const int32_t *d_point_rows, int B, uint64_t n, uint64_t k,
                           int cols, int32_t unassigned, int32_t *d_nd_labels, int32_t *d_point_labels, void *stream);

/* The same with one byte per point -- what a serving loop copies back to the host: d_point_labels
 * [B][n] uint8, any byte alignment; d_nd_labels stays int32.  Same argmax (the same kernel), same
 * gather, `unassigned` where the row is < 0 or >= k.  The gather takes four consecutive points per
 * thread (a 16-byte row load, a 4-byte label store) wherever a cloud's rows and labels are so
 * aligned, and single points at a cloud's misaligned head and its tail.
 * NDNET_ERR_ARG for a NULL pointer, B, n, k or cols < 1, cols > 255 (a class must fit a byte) or
 * unassigned < cols (the marker must not be a class). */
int ndnet_seg_point_labels_u8(const float *d_scores, const int32_t *d_point_rows, int B, uint64_t n, uint64_t k,
                              int cols, uint8_t unassigned, int32_t *d_nd_labels, uint8_t *d_point_labels, void *stream);

/* Confusion matrices up to this many classes are counted in a per-workgroup
 * LDS histogram (cols * cols + 1 counters of 32 bits: 15.5 KB at 63) flushed
 * with one 64-bit global atomic per non-zero counter; wider ones take a 64-bit
 * global atomic per point. */
#define NDNET_SEG_CONF_LDS_MAX_COLS 63

/* d_conf[gt * cols + pred] += 1 over `count` points with 0 <= pred, gt < cols; every other point
 * adds 1 to d_conf[cols * cols].  uint64 counters, the caller zeroes them.
 * NDNET_ERR_ARG for a NULL pointer, count == 0 or cols < 1. */
int ndnet_seg_confusion(const int32_t *d_pred, const int32_t *d_gt, uint64_t count, int cols,
                        unsigned long long *d_conf, void *stream);

/* The class histogram of every ND row, the target of the point-level training loss
 * (ndnet_tr_nll_hist, ndnet_train.h): d_hist[b][r][c] = the number of points i of cloud b with
 * d_point_rows[b][i] == r and d_point_labels[b][i] == c.  A point is skipped when its row lies
 * outside 0..k-1, its label outside 0..cols-1, or its label equals ignore_label (-1: none).
 * d_point_rows and d_point_labels [B][n] int32, d_hist [B][k][cols] int32.  The call clears d_hist
 * itself, in stream order, then adds one 32-bit global atomic per counted point: integer counts,
 * so the table is the same bits whatever the order.
 * NDNET_ERR_ARG for a NULL pointer or B, n, k or cols < 1. */
int ndnet_seg_row_hist(const int32_t *d_point_rows, const int32_t *d_point_labels, int B, uint64_t n, uint64_t k,
                       int cols, int32_t ignore_label, int32_t *d_hist, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* NDNET_SEGMENT_H_ */
