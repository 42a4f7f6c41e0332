// ndt_prune.h -- the KL kernels launched after a run, on request: k_prune, a
// further prune level on the retained list (ndt.c:28-73), and k_kl_chains, the
// LU chain states of a cloud whose list a lazy run deferred.
//
// Included by ndt_kernels.hip inside its anonymous namespace, after ndt_plan.h
// (CloudCtl, kKLThreads) and the KL stage of ndt_kernels.hip (KLArgs,
// prune_and_emit, the output helpers), and after the list sort: the kernels
// keep the order of definition they have always had in the unit.
#pragma once

__global__ void __launch_bounds__(kKLThreads) k_prune(KLArgs A) {
  const int b = blockIdx.x;
  CloudCtl& c = A.ctl[b];
  __shared__ uint32_t s_u32[16];
  if (c.state != kAccepted) {
    zero_outputs(A, b, A.k);
    pad_class_rows(A, b, A.k, 0);
    if (threadIdx.x == 0) write_stats(A, b);
    return;
  }
  const uint32_t nout = A.kl_lds ? prune_and_emit<true>(A, b, A.k, s_u32, s_u32)
                                 : prune_and_emit<false>(A, b, A.k, s_u32, s_u32);
  fill_tail(A, b, A.k, nout < A.k ? nout : (uint32_t)A.k);
  __syncthreads();
  if (threadIdx.x == 0) write_stats(A, b);
}

// The LU chain states of a deferred cloud (k_welford_q stored only their
// determinant bits): from the pre-KL covariance and the chain mask, the same
// in-place lu3 sequence as k_welford_q's epilogue, one thread per ND.
__global__ void __launch_bounds__(256) k_kl_chains(KLArgs A) {
  const int b = blockIdx.y;
  const CloudCtl& c = A.ctl[b];
  if (c.state != kAccepted || !c.kl_deferred) return;
  const uint32_t u = blockIdx.x * 256 + threadIdx.x;
  if (u >= c.num_nds) return;
  const uint64_t ob = (uint64_t)b * A.ndcap;
  double S[9];
#pragma unroll
  for (int q = 0; q < 9; q++) S[q] = A.nd_cov[9 * (ob + u) + q];
  const int nT = __popc(A.nkeys_all[ob + u]);
  double* chain = A.chain_all + ob * 108 + u;
  uint32_t* ps = A.chain_ps_all + ob * 12 + u;
  for (int t = 0; t < nT; t++) {
    uint32_t perm;
    int sg;
    lu3(S, perm, sg);
#pragma unroll
    for (int q = 0; q < 9; q++) chain[(uint64_t)(9 * t + q) * A.ndcap] = S[q];
    ps[(uint64_t)t * A.ndcap] = perm | (sg < 0 ? 0x100u : 0u);
  }
}
