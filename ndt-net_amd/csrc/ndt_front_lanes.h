// ndt_front_lanes.h -- k_front admission on the host: the device's front
// lanes (FrontLaneSet), their assignment to a plan, and front_launch /
// front_lanes_finish around every k_front launch.
//
// Included by ndt_kernels.hip inside its anonymous namespace, after ndt_plan.h
// (Plan), ndt_front.h (k_front, FrontArgs) and two host helpers of that file: HIPCHK,
// and g_lane_mu, which plan_free shares.
#pragma once

// k_front's workgroups of a cloud meet at cloud barriers, so all of them must
// be resident at once.  Two k_front grids that together want more workgroups
// than the chip holds can each get part of their workgroups resident and then
// wait on each other until the barrier timeout fails their clouds (measured:
// 640 ms per step, profiles/r04_ndt_streams_guard.txt).  The library rules that
// out itself, for any number of plans and streams, eager or captured in HIP
// graphs: the chip is split into kFrontLanes lanes of CUs / kFrontLanes; a
// plan's k_front occupies ceil(kFrontLanes * workgroups / CUs) of them (all four
// at CU share 1, two at share 2); before its launch the stream waits for the
// last k_front launched on each of its lanes, and after it the launch is
// recorded in the plan's own event, which becomes those lanes' last launch
// (explicit event graph nodes when the stream is being captured, so a replayed
// graph waits for the k_front launches before it, whatever stream they ran
// on).  A wait is left out when stream order already gives it (the lane's last
// launch came from the same stream in the same capture, or both eager), and
// lanes whose last launch shares an event are waited on once (round-5 r05e:
// four waits + four records per run cost 19 us of k_front stage).  So the
// k_front launches in flight at any time never want more workgroups than
// there are CUs, and grids on disjoint lanes (two share-2 plans: the
// pipeline's NDT streams) still run concurrently.  The other kernels never
// wait on anything, so they drain.
//
// Round 6: the admission is engaged only where it is needed.  k_front deals a
// launch's clouds cloud-major within each XCD (ndt_front.h), so a launch
// leaves at most G - 1 workgroups of one partially resident cloud waiting on
// an XCD.  While the live path-2 plans of the device together have
// sum (G - 1) < CUs per XCD (32), every XCD always keeps a CU free or a cloud
// completing, whatever the plans' launches overlap: no barrier can wait on a
// workgroup that never starts, and no admission is needed.  That covers one or
// two share-1 plans (15 + 15), and up to four share-2 plans (7 each).  Past
// the bound the lanes order the launches as above.  The bound matters: an
// event node in a replayed graph costs ~6 us (C2 alone: 151k clouds/s with
// the lanes' record and wait nodes, 171k without: profiles/r06d_lanes_ab.txt).
constexpr int kFrontLanes = 4;
constexpr int kMaxDevices = 64;
struct FrontLaneSet {
  int next;                          // the lane the next plan's lanes start at (round robin)
  int plans;                         // live plans holding a lane event on this device
  int gsum;                          // sum over them of (G - 1): their partial workgroups per XCD at most
  hipEvent_t ev[kFrontLanes];        // the event of the lane's last k_front launch (null: none yet)
  hipStream_t st[kFrontLanes];       // the stream it was launched on
  unsigned long long cap[kFrontLanes];  // the capture it was launched in (0: eager)
  std::vector<hipEvent_t> pool;      // events of freed plans, reused by later plans
};
static FrontLaneSet g_lanes[kMaxDevices];

// Drops a freed plan's event from the lanes (caller holds g_lane_mu; the
// event has completed, so nothing left to wait for).  The event itself is
// kept in the device's pool and handed to the next plan: a graph captured
// while this plan held a lane may still hold a wait node on it,
// and waiting on a pooled event only ever waits for a completed or a later
// k_front launch.
static void front_lanes_forget(Plan* P) {
  if (P->dev < 0 || P->dev >= kMaxDevices || !P->front_ev) return;
  FrontLaneSet& L = g_lanes[P->dev];
  for (int i = 0; i < kFrontLanes; i++)
    if (L.ev[i] == P->front_ev) L.ev[i] = nullptr;
  L.pool.push_back(P->front_ev);
  L.plans--;
  L.gsum -= P->lane_g;
  P->lane_g = 0;
  P->front_ev = nullptr;
}

// Assigns the plan's lanes for its current k_front geometry (caller holds g_lane_mu).
static hipError_t front_lanes_assign(Plan* P) {
  if (P->dev < 0 || P->dev >= kMaxDevices) return hipErrorInvalidDevice;
  FrontLaneSet& L = g_lanes[P->dev];
  if (!P->front_ev) {
    if (!L.pool.empty()) {
      P->front_ev = L.pool.back();
      L.pool.pop_back();
    } else {
      const hipError_t e = hipEventCreateWithFlags(&P->front_ev, hipEventDisableTiming);
      if (e != hipSuccess) return e;
    }
    L.plans++;
  }
  L.gsum -= P->lane_g;
  P->lane_g = P->fG > 1 ? (int)P->fG - 1 : 0;
  L.gsum += P->lane_g;
  const uint64_t wgs = (uint64_t)P->fG * (uint64_t)P->B;
  const int cus = P->cus > 0 ? P->cus : 1;
  int nl = (int)((wgs * kFrontLanes + (uint64_t)cus - 1) / (uint64_t)cus);
  nl = nl < 1 ? 1 : nl > kFrontLanes ? kFrontLanes : nl;
  P->nlanes = nl;
  P->lane0 = L.next;
  L.next = (L.next + nl) % kFrontLanes;
  return hipSuccess;
}

// Whether the device's live plans need the admission (the bound above);
// NDNET_FRONT_ADMIT=1 (A/B, tests) engages it always.  A launch made while
// the bound held records nothing; when more plans make it fail, their
// launches and the earlier ones' last runs may overlap once: the earlier plans
// alone were within the bound, and the lanes order everything after.
static bool admit_always() {
  static const bool v = [] {
    const char* e = getenv("NDNET_FRONT_ADMIT");
    return e && e[0] == '1';
  }();
  return v;
}
static bool admission_needed(const Plan* P, const FrontLaneSet& L) {
  const int per_xcd = P->cus >= 8 ? P->cus / 8 : 1;
  return admit_always() || L.gsum >= per_xcd;
}

// Adds an event node (wait or record) after the capture's current
// dependencies and makes it the capture's only dependency.
static hipError_t capture_event_node(hipStream_t st, hipEvent_t ev, bool wait) {
  hipStreamCaptureStatus cs;
  unsigned long long id = 0;
  hipGraph_t g = nullptr;
  const hipGraphNode_t* deps = nullptr;
  size_t nd = 0;
  hipError_t e = hipStreamGetCaptureInfo_v2(st, &cs, &id, &g, &deps, &nd);
  if (e != hipSuccess) return e;
  std::vector<hipGraphNode_t> dv(deps, deps + nd);
  hipGraphNode_t node;
  e = wait ? hipGraphAddEventWaitNode(&node, g, dv.data(), dv.size(), ev)
           : hipGraphAddEventRecordNode(&node, g, dv.data(), dv.size(), ev);
  if (e != hipSuccess) return e;
  return hipStreamUpdateCaptureDependencies(st, &node, 1, hipStreamSetCaptureDependencies);
}

// Records the plan's last k_front launch on its lanes (caller holds
// g_lane_mu).  The record is made at the end of the plan's run
// (front_lanes_finish), not right after k_front: a record node between
// k_front and k_welford_q held the next launch back -- the isolated C2 k_front
// stage 51 -> 55 us, profiles/r05_lanes_ab.txt; at the run's end it follows
// the last KL launch, where the pipeline records its own stage event anyway
// (profiles/r06c_two_process_and_lane_record.txt).  A later k_front on those
// lanes then waits for the whole run instead of its k_front only: stricter,
// and still one chip's worth at a time.
static int front_lanes_record(Plan* P, hipStream_t st) {
  FrontLaneSet& L = g_lanes[P->dev];
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  unsigned long long cap_id = 0;
  HIPCHK(hipStreamGetCaptureInfo(st, &cs, &cap_id));
  const bool cap = cs == hipStreamCaptureStatusActive;
  if (!cap) cap_id = 0;
  if (!cap) HIPCHK(hipEventRecord(P->front_ev, st));
  else HIPCHK(capture_event_node(st, P->front_ev, false));
  for (int i = 0; i < P->nlanes; i++) {
    const int l = (P->lane0 + i) % kFrontLanes;
    L.ev[l] = P->front_ev;
    L.st[l] = st;
    L.cap[l] = cap_id;
  }
  return NDNET_OK;
}

// The record a run deferred to its end: after its last launch.
static int front_lanes_finish(Plan* P, hipStream_t st) {
  if (!P->lane_rec) return NDNET_OK;
  P->lane_rec = 0;
  std::lock_guard<std::mutex> lk(g_lane_mu);
  return front_lanes_record(P, st);
}

template <typename T>
static void front_kernel(Plan* P, hipStream_t st, const T* pts, const FrontArgs& F) {
  // grid, workgroups per cloud and LDS are the plan's, with or without counts
  if (F.counts) k_front<T, true><<<P->fG * P->B, kFrontThreads, P->flds, st>>>(pts, F);
  else k_front<T, false><<<P->fG * P->B, kFrontThreads, P->flds, st>>>(pts, F);
}

// Launches k_front after the lane waits (front_lanes_assign); the run's end
// records it (front_lanes_finish).  A stream being captured is admitted with
// explicit graph nodes (hipGraphAddEventWaitNode / hipGraphAddEventRecordNode
// on the capture's graph, then the capture's dependencies moved past them).
// The capture forms hipStreamWaitEvent(hipEventWaitExternal) and
// hipEventRecordWithFlags(hipEventRecordExternal) abort inside HIP on ROCm 7.2
// (std::bad_alloc; error -21: profiles/r05_capture_lane_probe.txt) and are not
// used.
template <typename T>
static int front_launch(Plan* P, hipStream_t st, const T* pts, const FrontArgs& F) {
  P->lane_rec = 0;
  std::lock_guard<std::mutex> lk(g_lane_mu);  // waits and launch in one host order
  FrontLaneSet& L = g_lanes[P->dev];
  if (!admission_needed(P, L)) {
    front_kernel<T>(P, st, pts, F);
    HIPCHK(hipGetLastError());
    return NDNET_OK;
  }
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  unsigned long long cap_id = 0;
  HIPCHK(hipStreamGetCaptureInfo(st, &cs, &cap_id));
  const bool cap = cs == hipStreamCaptureStatusActive;
  if (!cap) cap_id = 0;
  hipEvent_t waited[kFrontLanes];
  int nw = 0;
  for (int i = 0; i < P->nlanes; i++) {
    const int l = (P->lane0 + i) % kFrontLanes;
    hipEvent_t ev = L.ev[l];
    if (!ev || (L.st[l] == st && L.cap[l] == cap_id)) continue;  // nothing yet / stream order covers it
    bool dup = false;
    for (int j = 0; j < nw; j++) dup |= waited[j] == ev;
    if (dup) continue;
    waited[nw++] = ev;
    if (!cap) HIPCHK(hipStreamWaitEvent(st, ev, 0));
    else HIPCHK(capture_event_node(st, ev, true));
  }
  front_kernel<T>(P, st, pts, F);
  HIPCHK(hipGetLastError());
  P->lane_rec = 1;
  return NDNET_OK;
}
