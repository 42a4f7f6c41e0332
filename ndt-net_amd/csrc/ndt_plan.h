// ndt_plan.h -- the tunable constants of the NDT path, the per-cloud control
// block (CloudCtl) and the plan (Plan: geometry, options, every device buffer).
//
// Included by ndt_kernels.hip inside its anonymous namespace, first of the
// stage headers.  Needs <hip/hip_runtime.h>, ndt_device.h (kWorkers) and
// ../../include/ndnet_amd.h (ndnet_ndt_stats).
#pragma once

constexpr int kPassThreads = 256;    // threads per search workgroup
constexpr int kPassPPT = 4;          // points per thread per search workgroup
constexpr int kPassPts = kPassThreads * kPassPPT;
constexpr int kHashSlots = 2048;     // LDS dedup table of a search workgroup (>= kBitsWords)
constexpr int kBitsCap = 32768;      // grids up to this many voxels count through bitmaps
constexpr int kBitsWords = kBitsCap / 32;
constexpr int kKLThreads = 1024;
constexpr int kChunk = 256;          // slots per chunk of the chip-wide event sort
constexpr int kKLMarks = 32;  // phase stamps per cloud of the KL kernels (timing level 2)
constexpr int kMergeLdsChunks = 34;  // k_kl_merge stages score + NaN keys in LDS up to this many chunks (136 KB)
constexpr int kMergeScoreChunks = 72; // ... and the score runs alone up to this many (144 KB; k <= 2440)
constexpr int kMaxChunks = 6 * 16384 / kChunk;  // ndcap <= 16384
// NDs with at least this many samples get a whole wave each in k_welford_q
// (wq_heavy): k_front / k_bin_offsets list them per cloud.  The plan's
// default (ndnet_ndt_set_heavy_threshold).
#ifndef NDNET_WQ_HEAVY
#define NDNET_WQ_HEAVY 256
#endif
constexpr uint32_t kWqHeavy = NDNET_WQ_HEAVY;

enum State : uint32_t { kSearching = 0, kAccepted = 1, kFailed = 2 };

struct CloudCtl {
  unsigned long long limkey[6];  // order keys: max x,y,z then min x,y,z
  double lim[6];
  double guess, lo, hi;
  double vs;
  double off[3];
  uint32_t len[3];
  uint32_t state;
  int32_t rc;
  uint32_t iter;
  uint32_t epoch;
  uint32_t stamp;
  uint32_t accepted_stamp;
  uint32_t acc_mode;     // occupancy of the accepted pass: 0/1 bitmap buffer, 2 stamps
  uint32_t count;
  uint32_t arrive;
  uint32_t nbad;
  uint32_t first_bad[kWorkers];
  uint64_t V;
  uint32_t num_nds;
  double guesses[16];
  uint32_t counts[16];
  // list state kept for further prune levels (ndt_legacy.py:173-240)
  uint32_t num_valid;
  uint32_t num_kl;       // live list length
  uint32_t num_phys;     // entries ever written (the rest is poison)
  uint32_t num_events;
  int32_t prune_rc;
  uint32_t num_out;
  uint32_t last_k;
  uint32_t clear_stamps; // the epoch wrapped this run: k_limits zeroes the cloud's stamps
  uint32_t kl_deferred;  // the retained list was not built by the run (lazy list, num_nds <= k)
  uint32_t flag_count;   // events of a deferred cloud, counted by k_kl_rank_chunks (zeroed per run)
  uint32_t list_off;     // physical index of the retained list's first entry (the prunes' pending
                         // left shifts, ndt.c:69-72; always 0 on the global-memory prune path)
  uint32_t heavy_n;      // NDs of the accepted grid with >= kWqHeavy samples, listed in Plan::heavy
                         // (written by the binning of every run that accepts a grid)
  uint32_t heavy_t;      // the threshold that list was built with: k_welford_q's light items skip
                         // exactly the NDs it holds, whatever the plan's threshold is by then
  uint32_t kl_arrive;    // k_kl_merge<.., kTail> workgroups of the cloud done (re-armed by the last)
};

struct Plan {
  int B;
  uint64_t n;
  uint64_t k;
  int ncls;            // num_classes (histograms have ncls+1 bins)
  uint64_t vcap;       // voxels per cloud the stamp / dense tables hold
  uint32_t ndcap;      // max accepted NDs per cloud = floor(1.2 k) + 1
  uint32_t ecap;       // 6 * ndcap
  uint32_t nbins;      // 1024-point binning chunks per cloud
  uint32_t G;          // search workgroups per cloud
  int in_f64;          // input element type of the last run
  uint64_t calls;      // runs issued from the host (graph replays not counted)
  int timing;          // 0 off, 1 stage events, 2 + k_kl phase marks
  int ev_created;
  hipEvent_t ev[8];
  unsigned long long* kl_marks;  // [B][kKLMarks] s_memrealtime stamps (timing level 2)
  unsigned long long* wq_marks;  // [wq_items][kWqMarkW] k_welford_q per-item stamps (timing level 2)
  // device buffers
  CloudCtl* ctl;
  uint32_t* stamps;    // [B][vcap]
  uint32_t* dense_of;  // [B][vcap]
  uint32_t* vox;       // [B][ndcap] linear index of dense id
  uint32_t* gbits;     // [B][2][kBitsWords] occupancy bitmaps of small-grid passes
  uint32_t* pkeys;     // [B][n] voxel key of every point in the latest pass
  uint32_t* did;       // [B][n] dense id of every point in the accepted pass
  uint32_t* bin_cnt;   // [B][nbins][ndcap] per-chunk histograms -> offsets
  uint32_t* nd_base;   // [B][ndcap]
  void* nd_pts;        // [B][n][3] points grouped by ND (input element type)
  uint16_t* nd_lbl;    // [B][n]
  uint32_t* nd_n;      // [B][ndcap]
  double* nd_mean;     // [B][ndcap][3]
  double* nd_cov;      // [B][ndcap][9] pre-KL
  double* nd_cov_post; // [B][ndcap][9]
  uint16_t* nd_cls;    // [B][ndcap]
  uint32_t* hist;      // [B][ndcap][ncls+1]
  int32_t* nb;         // [B][ndcap][6]
  uint32_t* keys;      // [B][ndcap][12]
  uint32_t* nkeys;     // [B][ndcap]
  double* chain;       // [B][ndcap][12][9]
  uint32_t* chain_ps;  // [B][ndcap][12] perm | (signum < 0) << 8
  uint32_t* chain_ok;  // [B][ndcap] bit t: LU state t has det != 0 and sgndet != 0 (lazy clouds only)
  double* slot_val;    // [B][ecap]
  uint32_t* slot_flag; // [B][ecap]
  double* ev_val;      // [B][ecap]
  uint32_t* ev_p;      // [B][ecap]
  uint32_t* ev_q;      // [B][ecap]
  double* ev_min;      // [B][ecap] exclusive prefix min (NaN-skipping)
  unsigned long long* sort_key;  // [B][sortcap]
  uint32_t* sort_idx;  // [B][sortcap]
  uint32_t* nan_list;  // [B][ecap] NaN slots per chunk (chunk * kChunk + j)
  unsigned long long* nan_key;  // [B][ecap] NaN keys, contiguous in slot order
  uint32_t* nan_slot;  // [B][ecap] their slots
  uint32_t* chunk_nanbase;  // [B][nchunk] NaN events in earlier chunks
  double* ord_val;     // [B][ecap] the retained list (physical array)
  uint32_t* ord_p;     // [B][ecap]
  uint32_t* ord_q;     // [B][ecap]
  uint32_t* first_occ; // [B][ndcap]
  uint32_t* tmp_u32;   // [B][ecap] scratch
  uint8_t* alive;      // [B][ndcap]
  uint32_t sortcap;    // chunked sort arrays per cloud: roundup(ecap, kChunk)
  uint32_t nchunk;     // kChunk-slot chunks per cloud (max)
  uint32_t* chunk_cnt; // [B][nchunk] (non-NaN count << 16) | NaN count
  double* chunk_min;   // [B][nchunk] min non-NaN value of the chunk (+inf if none)
  ndnet_ndt_stats* d_stats;  // [B] device copy of the stats
  // k_front (ndt_front.h): the fused front of the pipeline
  int front;                 // 1: k_front path, 0: the multi-kernel path
  int front_ok;              // the plan's shape admits k_front
  uint32_t fG, fbpw, frbs;   // workgroups per cloud, 1024-point bins per workgroup, points per rank bin
  size_t flds;               // dynamic LDS bytes of k_front
  unsigned long long* flims; // [B][fG][6]
  uint32_t* frec;            // [B][kFrontPhases][fG][kRecWords]
  uint32_t* fwgcnt;          // [B][fG][ndcap]
  uint32_t* fbar;            // [B][kBarStride]
  unsigned long long* fmarks; // [B][kFrontMarkStride]: k_front phase stamps of WG 0 + start/end of every WG (timing level 2)
  int exact_counts;           // k_front counts every bisection grid (ndnet_ndt_set_exact_counts)
  int wq_l64;                 // k_welford_q light form: 1 light64 (one ND per lane), 0 lane quads
  int wq_form;                // 0 auto (quads at CU share 1, light64 above), 1 light64, 2 quads
  uint32_t wq_grid;           // k_welford_q workgroups: one per CU (of the plan's CU share)
  int cus;                    // the device's CUs
  int cu_share;               // k_front / k_welford_q use CUs / cu_share (ndnet_ndt_set_cu_share)
  uint32_t* wq_ctr;           // [8][16] k_welford_q dynamic item counters, one per XCD (re-armed by k_kl_rank_chunks)
  int eager_list;             // build every cloud's retained list in the run (ndnet_ndt_set_lazy_list(plan, 0))
  int kl_fuse;                // the run's prune rides on the merge launch (kl_fusable; NDNET_KL_FUSE=0: k_kl)
  int list_sort;              // 2 (auto): k_kl_sort at a CU share > 1 where the list fits (sort_fits); 1: wherever it fits;
                              // 3: as 1 in k_kl_rank_sort's one launch; 0: k_kl_merge (NDNET_KL_SORT)
  uint64_t front_sync_ticks;  // k_front's cloud-barrier timeout (ndnet_ndt_debug_set_sync_timeout)
  int lists_built;            // the deferred lists of the last run are built (no further build launches)
  int front_staged;           // k_front's scatter through LDS records (ndnet_ndt_set_front_staged; default 1)
  int run_part;               // ndnet_ndt_set_run_part: 0 whole run, 1 front only, 2 from k_welford_q on
  int lane_rec;               // this run's k_front still to be recorded on its lanes (front_lanes_finish)
  int lane_g;                 // this plan's share of FrontLaneSet::gsum (G - 1)
  uint32_t* heavy;            // [B][ndcap] the heavy NDs of each cloud (CloudCtl::heavy_n of them)
  double* rtab;               // [n + 1][2] (rc, rl) per count for wq_heavy's divisions
  uint32_t* lu_done;          // [B][ceil(ndcap / 64)] k_welford_q's per-group completion counters (re-armed to 0)
  uint32_t heavy_t;           // NDs with >= heavy_t samples take wq_heavy (ndnet_ndt_set_heavy_threshold)
  // k_front admission (front_gate): the device's front lanes this plan's
  // k_front occupies, and the barrier-timeout flag k_front raises in host memory
  int dev;                    // the device the plan lives on
  int lane0, nlanes;          // lanes [lane0, lane0 + nlanes) mod kFrontLanes
  hipEvent_t front_ev;        // records this plan's k_front launches (the lanes' admission)
  uint32_t* sync_fail_h;      // pinned host word (mapped): nonzero after a k_front barrier timeout
  uint32_t* sync_fail_d;      // its device address
};
