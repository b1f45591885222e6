// sg_runs.h -- the first stage of the entry points that start from the raw KCOV
// buffers of whole executions (sg_triage_runs.hip, sg_minimize_pred.hip): mark
// the one call of each execution that counts, and truncate the PCs.  Not
// installed.
#pragma once

#include "sg_internal.h"

namespace sg {
namespace {

constexpr uint32_t kNoCall = 0xFFFFFFFFu;

// Execution e owns calls prog_off[e] .. prog_off[e + 1]; the call that counts is
// call[e / nruns] (nruns executions per entry of call).  sel[c] = 1 for that
// call, on top of what sel holds, and selcall[e] = c; an execution with fewer
// calls is len(info) == 0: selcall[e] = kNoCall.
__global__ void k_tr_select(const uint64_t* __restrict__ prog_off, const uint32_t* __restrict__ call, uint64_t nexec,
                            uint32_t nruns, uint64_t ncalls, uint32_t* __restrict__ selcall, uint8_t* __restrict__ sel) {
  const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= nexec) return;
  uint64_t c0, c1;
  sgd::csr_range(prog_off, e, ncalls, c0, c1);
  const uint64_t want = call[e / nruns];
  if (c1 - c0 > want) {  // fuzzer.go:547 / :558 / :580: info[call] exists
    selcall[e] = (uint32_t)(c0 + want);
    sel[c0 + want] = 1;
  } else {
    selcall[e] = kNoCall;
  }
}

// executor.h:394 (uint32_t)cover_data[i]
__global__ void k_tr_trunc(const uint64_t* __restrict__ pcs, uint64_t n, uint32_t* __restrict__ out) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = (uint32_t)pcs[i];
}

}  // namespace
}  // namespace sg
