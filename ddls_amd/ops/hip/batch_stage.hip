// Minibatch stage kernel for the cached-models PPO step (gfx950).
//
// The rollout batch stays in device memory in a fixed-address store
// (rl/graph_step.py::DeviceBatchStore).  cs_stage_kernel gathers ONE
// minibatch from it into the staged-input buffers cached_step.hip reads
// (the stepper's d-buffers), so a captured replay needs no host staging and
// no H2D copy: row i of the minibatch is store row perm[cursor, i].
//
// One 256-thread workgroup: a minibatch is B <= 1024 rows of 34 floats plus
// five per-row scalars (~25 KB at B=128), far below what one CU moves in a
// microsecond, and a single workgroup lets the cursor advance without a
// second kernel or a grid-wide barrier.
//
// Cursor protocol.  Every thread reads the cursor, the block barriers, and
// only after that barrier may thread 0 store cursor + 1, so no thread of the
// launch can observe the advanced value.  The row counts (n_rows, n_mb) are
// device scalars: a captured graph survives a change of batch size within
// the store's capacity.
//
// Guards.  cursor outside [0, n_mb) or [0, cap_mb), or any index of the
// selected perm row outside [0, n_rows) or [0, cap_n): the store is NOT read
// at that position, err is set (it is never cleared here), the destination
// buffers stay untouched and the cursor does not advance.  cursor ==
// CS_STAGE_BYPASS (-1) is the host-staged mode: the caller filled the
// destination buffers itself, the kernel leaves everything alone.
#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>
#include <vector>

// StagePtrs / StageDims, the kernel body and the host-side argument checks:
// shared with cached_step.hip, whose first forward launch can run the same
// role in its block 0 (cached_step_fwd_staged)
#include "cs_stage.h"

__global__ __launch_bounds__(CS_STAGE_THREADS) void cs_stage_kernel(
    StagePtrs P, StageDims D) {
  cs_stage_body(P, D);
}

// ===========================================================================
// host binding
// ===========================================================================

// store = [gfull, model_ids, actions, old_logp, adv, vtarg]
// dst   = [gf, mask, model_ids, actions, old_logp, adv, vtarg]
// dims  = [n_rows, n_mb] device scalars
void cached_stage(std::vector<torch::Tensor> store,
                  std::vector<torch::Tensor> dst, torch::Tensor perm,
                  torch::Tensor cursor, torch::Tensor err,
                  std::vector<torch::Tensor> dims) {
  StagePtrs P;
  StageDims D;
  cs_stage_args(P, D, "cached_stage", store, dst, perm, cursor, err, dims);
  hipStream_t stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(cs_stage_kernel, dim3(1), dim3(CS_STAGE_THREADS), 0,
                     stream, P, D);
}
