/*
 * ndnet_packed.h -- packed int16 point input on gfx950 (libndnet_amd.so).
 *
 * A scan that arrives over PCIe does not need 32 bits per coordinate: a packed
 * batch is q [B][n][3] int16 and qparams [B][4] float32, (ox, oy, oz, step)
 * per cloud -- 6 bytes per point where float32 takes 12.  The cloud itself is,
 * by definition, the decoded float32 cloud
 *
 *     x[b][i][a] = RN( RN( float(q[b][i][a]) * step[b] ) + o[b][a] )
 *
 * element-wise in float32 with two roundings, never a fused multiply-add (in
 * numpy: q.astype(np.float32) * step + origin on float32 arrays).  Everything
 * downstream runs on that cloud as on any other.  The packer is host code
 * (ndnet.packed.pack_points).
 *
 * Plan-free: device pointers, stream ordered, no allocation and no
 * synchronisation (capturable).  Return codes as ndnet_amd.h: NDNET_OK,
 * NDNET_ERR_ARG (checked before any launch), NDNET_ERR_HIP.
 */
#ifndef NDNET_PACKED_H_
#define NDNET_PACKED_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* d_points[b][i][a] = the decoded q[b][i][a] for every point i < m_b of every cloud b, where m_b is
 * n (d_counts NULL) or d_counts[b] clamped into 0..n ([B] int32, read on the device; the NDT run
 * that follows reports a count outside 1..n, as it does today).  Points past m_b are neither read
 * nor written: d_points keeps whatever it held there.
 * d_q [B][n][3] int16 (2-byte aligned), d_qparams [B][4] float32, d_points [B][n][3] float32
 * (4-byte aligned); d_q and d_points must not overlap.  A cloud is decoded as a flat run of 3 m_b
 * elements, eight per thread -- one 16-byte load, two 16-byte stores -- from the first element
 * whose q is 16-byte aligned, wherever the output is 16-byte aligned there too (it always is when
 * d_q and d_points both are); the 0..7 elements before it, the tail and an output that is not so
 * aligned take single elements.
 * NDNET_ERR_ARG for a NULL d_q, d_qparams or d_points, B < 1 or > 65535, n < 1 or n >= 2^31. */
int ndnet_pts_unpack_i16(const int16_t *d_q, const float *d_qparams, int B, uint64_t n, const int32_t *d_counts,
                         float *d_points, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* NDNET_PACKED_H_ */
