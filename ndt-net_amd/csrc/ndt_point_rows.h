// ndt_point_rows.h -- k_point_rows: the output row every input point was
// folded into (ndnet_ndt_point_rows).
//
// Included by ndt_kernels.hip inside its anonymous namespace, after ndt_plan.h
// (CloudCtl), ndt_block.h (block_excl_scan) and the path-1 kernels of
// ndt_kernels.hip (voxel_key, voxel_key_f32).
#pragma once

// k_point_rows: the output row every input point was folded into, after a run
// (or a further prune level) of the plan.  A point contributed to an ND iff its
// cloud has rc 0, it lies below the n % 8 tail and its worker's cut-off
// (first_bad), and its key at the accepted grid -- voxel_key_f32 with
// voxel_key as the fallback, from the constants k_front derives -- is in grid;
// the ND is the dense id d with vox[d] == key (vox ascends: a binary search in
// LDS), the row the number of alive NDs below d, where that is below
// min(num_out, num_desired).  Every other point gets -1 or, with fill nearest,
// the row whose fp32 mean is nearest (dx dx + dy dy + dz dz in fp32, the lowest
// row on a tie); a point with a non-finite coordinate always gets -1.
//
// One workgroup per kPrPts points of a cloud: the points arrive as the flat
// coalesced float stream (every load issued before the first use), vox and the
// row table (a block scan of alive) are staged in LDS, the rows leave as
// coalesced int32 stores.  The nearest phase gathers the workgroup's
// unassigned points into an LDS list and searches them densely: a group of
// L = 256 / (list length) lanes (a power of two, at most a wave) per point,
// the rows dealt round-robin to the group's lanes, tiles of kPrTile row means
// in LDS (over the vox / row-table region, dead by then).  Reads the plan's
// state only.
constexpr int kPrThreads = 256;
constexpr int kPrPPT = 4;      // 1024 points per workgroup: 8 at 2048 measured 21.4 / 30.7 us (none / nearest, U)
                               // against 18.2 / 21.5, 2 at 512 18.5 / 19.4 (profiles/point_labels.json's shape)
constexpr int kPrPts = kPrThreads * kPrPPT;
constexpr int kPrTile = 1024;  // row means per LDS tile of the nearest phase (12 KB)
constexpr uint16_t kPrNoRow = 0xffffu;

__host__ __device__ inline uint32_t pr_region_words(uint32_t ndcap, int fill) {
  const uint32_t a = ndcap + (ndcap + 1) / 2, t = fill ? 3u * kPrTile : 0u;  // vox u32 + row table u16
  return a > t ? a : t;
}
static size_t pr_lds_bytes(uint32_t ndcap, int fill) {
  // points | vox + row table (nearest: row-mean tile) | nearest: rows, list
  return sizeof(float) * 3 * kPrPts + 4 * (size_t)pr_region_words(ndcap, fill) +
         (fill ? (sizeof(int32_t) + sizeof(uint16_t)) * kPrPts : 0);
}

__global__ void __launch_bounds__(kPrThreads) k_point_rows(const float* __restrict__ pts, const CloudCtl* ctl,
                                                          const uint32_t* __restrict__ vox_all,
                                                          const uint8_t* __restrict__ alive_all,
                                                          const float* __restrict__ rows_block, int32_t* __restrict__ out,
                                                          uint64_t n, uint32_t ndcap, uint64_t kdes, int fill,
                                                          const int32_t* __restrict__ counts) {
  extern __shared__ __attribute__((aligned(16))) uint32_t pr_smem[];
  __shared__ uint32_t scratch[16];
  __shared__ uint32_t s_cut[kWorkers];
  __shared__ uint32_t s_nun;
  const int b = blockIdx.y;
  const uint32_t t = threadIdx.x;
  const CloudCtl& c = ctl[b];
  const uint64_t start = (uint64_t)blockIdx.x * kPrPts;
  const uint32_t cnt = (uint32_t)(n - start < (uint64_t)kPrPts ? n - start : (uint64_t)kPrPts);
  int32_t* o = out + (uint64_t)b * n + start;
  const uint32_t nout = c.num_out < kdes ? c.num_out : (uint32_t)kdes;  // rows of the level last run
  if (c.state != kAccepted || c.rc != 0 || nout == 0 || c.num_nds == 0) {  // a cloud without rows
#pragma unroll
    for (int q = 0; q < kPrPPT; q++) {
      const uint32_t il = t + kPrThreads * q;
      if (il < cnt) o[il] = -1;
    }
    return;
  }
  float* sp = (float*)pr_smem;                        // [3 * kPrPts]
  uint32_t* s_vox = pr_smem + 3 * kPrPts;             // [nd]
  uint16_t* s_row = (uint16_t*)(s_vox + ndcap);       // [nd] row of dense id (< k <= 13653), or kPrNoRow
  float* s_mean = (float*)s_vox;                      // nearest: [3 * kPrTile]
  int32_t* s_prow = (int32_t*)(pr_smem + 3 * kPrPts + pr_region_words(ndcap, fill));  // nearest: [kPrPts]
  uint16_t* s_un = (uint16_t*)(s_prow + kPrPts);      // nearest: [kPrPts] unassigned local ids
  const uint32_t nd = c.num_nds < ndcap ? c.num_nds : ndcap;
  {
    const float* p = pts + ((uint64_t)b * n + start) * 3;
    float v[3 * kPrPPT];
#pragma unroll
    for (int j = 0; j < 3 * kPrPPT; j++) {
      const uint32_t f = t + kPrThreads * j;
      v[j] = f < 3 * cnt ? p[f] : 0.0f;
    }
    const uint32_t* vox = vox_all + (uint64_t)b * ndcap;
    const uint8_t* alive = alive_all + (uint64_t)b * ndcap;
    uint8_t* s_alive = (uint8_t*)s_row;  // [nd], consumed before the row table takes its place
#pragma unroll 4
    for (uint32_t d = t; d < nd; d += kPrThreads) {  // (no barrier inside: the loads stay in flight together)
      s_vox[d] = vox[d];
      s_alive[d] = alive[d];
    }
    if (t < (uint32_t)kWorkers) s_cut[t] = c.first_bad[t];
    if (t == 0) s_nun = 0;
#pragma unroll
    for (int j = 0; j < 3 * kPrPPT; j++) sp[t + kPrThreads * j] = v[j];
  }
  __syncthreads();
  {
    // row of dense id: thread t owns `per` consecutive NDs (<= 64: ndcap <= 16384), its alive
    // flags in a register mask, one block scan of the counts
    const uint32_t per = (nd + kPrThreads - 1) / kPrThreads, d0 = t * per;
    const uint8_t* s_alive = (const uint8_t*)s_row;
    unsigned long long live = 0;
    for (uint32_t j = 0; j < per; j++)
      if (d0 + j < nd && s_alive[d0 + j]) live |= 1ull << j;
    uint32_t tot;
    uint32_t rw = block_excl_scan((uint32_t)__popcll(live), 0u, AddU32(), scratch, tot);  // (barriers: the flags are read)
    for (uint32_t j = 0; j < per; j++) {
      if (d0 + j >= nd) break;
      const uint32_t l = (uint32_t)(live >> j) & 1u;
      s_row[d0 + j] = l && rw < nout ? (uint16_t)rw : kPrNoRow;
      rw += l;
    }
  }
  __syncthreads();
  // the key constants as k_front's search passes (ndt_front.h) and
  // k_debug_voxel_keys (ndt_kernels.hip, the tested copy) derive them: keep
  // the three sites the same
  const double vs = c.vs, inv_vs = 1.0 / vs;
  const double off[3] = {c.off[0], c.off[1], c.off[2]};
  const uint32_t len[3] = {c.len[0], c.len[1], c.len[2]};
  const float off32[3] = {(float)off[0], (float)off[1], (float)off[2]};
  const float inv32 = (float)inv_vs;
  const float lenf[3] = {(float)len[0], (float)len[1], (float)len[2]};
  const float lmax = fmaxf(lenf[0], fmaxf(lenf[1], lenf[2]));
  const float half_tol = 0.5f - lmax * 0x1p-19f;
  const bool fast32 = (double)off32[0] == off[0] && (double)off32[1] == off[1] && (double)off32[2] == off[2];
  // ragged batches: the cloud's own count for the tail and the workers (a
  // cloud with rows has a valid count); a point at or past it is padding --
  // whatever it holds, it gets -1 and never joins the nearest list
  const uint64_t nc = cloud_points(counts, b, n);
  const uint64_t chunk = nc / kWorkers, n8 = chunk * kWorkers;
#pragma unroll
  for (int q = 0; q < kPrPPT; q++) {
    const uint32_t il = t + kPrThreads * q;
    const uint64_t i = start + il;
    const float x = sp[3 * il], y = sp[3 * il + 1], z = sp[3 * il + 2];
    const bool finite = i < nc && isfinite(x) && isfinite(y) && isfinite(z);
    // a point of the run is never below the grid offset (the cloud's minimum); one that is
    // (a caller's other points) takes the double path, which finds it out of grid
    const bool below = x < off32[0] || y < off32[1] || z < off32[2];
    uint32_t key = kKeyRedo;
    if (fast32 && !below) key = voxel_key_f32(x, y, z, off32, inv32, half_tol, lenf, len);
    if (__any(key == kKeyRedo)) {  // (voxel_key votes across the wave: every lane enters)
      const uint32_t k64 = voxel_key((double)x, (double)y, (double)z, off, len, vs, inv_vs);
      if (key == kKeyRedo) key = k64;
    }
    int32_t row = -1;
    const uint32_t w = i < n8 ? (uint32_t)(i / chunk) : 0u;  // (i < n8: chunk > 0 and w < 8)
    if (il < cnt && finite && i < n8 && i < s_cut[w] && key != kInvalid) {
      uint32_t lo = 0, hi = nd;  // first d with vox[d] >= key
      while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (s_vox[mid] < key) lo = mid + 1;
        else hi = mid;
      }
      if (lo < nd && s_vox[lo] == key && s_row[lo] != kPrNoRow) row = (int32_t)s_row[lo];
    }
    if (!fill) {
      if (il < cnt) o[il] = row;
    } else {
      s_prow[il] = row;
      if (il < cnt && row < 0 && finite) s_un[atomicAdd(&s_nun, 1u)] = (uint16_t)il;
    }
  }
  if (!fill) return;
  __syncthreads();
  const uint32_t nun = s_nun;  // (block-uniform; vox and the row table are dead from here)
  if (nun) {
    uint32_t L = 1;
    while (L < 64 && 2 * L * nun <= (uint32_t)kPrThreads) L <<= 1;
    const uint32_t per = kPrThreads / L, grp = t / L, gl = t & (L - 1);
    const float* rb = rows_block + (uint64_t)b * kdes * 12;
    const uint32_t ntile = (nout + kPrTile - 1) / kPrTile;
    for (uint32_t u0 = 0; u0 < nun; u0 += per) {
      const uint32_t u = u0 + grp;
      const uint32_t il = u < nun ? s_un[u] : 0u;
      const float x = sp[3 * il], y = sp[3 * il + 1], z = sp[3 * il + 2];
      float bd = __builtin_inff();
      uint32_t br = 0x7fffffffu;
      for (uint32_t tl = 0; tl < ntile; tl++) {
        const uint32_t r0 = tl * kPrTile;
        const uint32_t nr = nout - r0 < (uint32_t)kPrTile ? nout - r0 : (uint32_t)kPrTile;
        if (ntile > 1 || u0 == 0) {  // one tile: staged once
          if (ntile > 1) __syncthreads();
          for (uint32_t f = t; f < 3 * nr; f += kPrThreads) s_mean[f] = rb[(uint64_t)(r0 + f / 3) * 12 + f % 3];
          __syncthreads();
        }
#pragma unroll 4
        for (uint32_t r = gl; r < nr; r += L) {  // ascending rows: the strict < keeps the lowest on a tie
          const float dx = x - s_mean[3 * r], dy = y - s_mean[3 * r + 1], dz = z - s_mean[3 * r + 2];
          float d = dx * dx;
          d = d + dy * dy;
          d = d + dz * dz;
          if (d < bd) {
            bd = d;
            br = r0 + r;
          }
        }
      }
      for (uint32_t m = 1; m < L; m <<= 1) {  // the group's minimum, the lowest row on a tie
        const float od = __shfl_xor(bd, (int)m, 64);
        const uint32_t orow = __shfl_xor(br, (int)m, 64);
        if (od < bd || (od == bd && orow < br)) {
          bd = od;
          br = orow;
        }
      }
      // every distance +inf (coordinates near FLT_MAX): row 0, the lowest of the tie
      if (gl == 0 && u < nun) s_prow[il] = br == 0x7fffffffu ? 0 : (int32_t)br;
    }
    __syncthreads();
  }
#pragma unroll
  for (int q = 0; q < kPrPPT; q++) {
    const uint32_t il = t + kPrThreads * q;
    if (il < cnt) o[il] = s_prow[il];
  }
}
