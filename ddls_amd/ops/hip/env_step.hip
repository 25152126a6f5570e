// Batched RAMP env step for gfx950: one workgroup per env, the whole
// steady-state PAC-ML env step in ONE kernel launch over B vectorised envs
// (reference hot loop ramp_cluster_environment.py:894-1044
// + the first-fit block placement search agents/placers/utils.py:532).
//
// This kernel is a LINE-FOR-LINE translation of the CPU mirror
// (ddls_amd/cluster/vec_engine.py::cpu_step_env) and must stay in lockstep
// with it: the GPU parity test asserts BITWISE f64 equality of state and
// f32 equality of observations over whole episodes.
//
// Memo probes go through an open-addressing hash table in HBM keyed
// (model_id << 20 | degree) — the device-side analogue of the reference's
// job_model_to_max_num_partitions_to_lookahead dict
// (ramp_cluster_environment.py:269-277).  A probe miss aborts the env's
// step WITHOUT mutating state (status = ST_MISS); the host services the
// miss (runs the lookahead, inserts) and relaunches for the missed envs.
#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>
#include <vector>

#include "env_step_body.h"

// ---- the step kernel: one workgroup per env, thread 0 runs the body ----
__global__ void __launch_bounds__(64)
env_step_kernel(EnvPtrs P, EnvDims D) {
  const int b = blockIdx.x;
  if (b >= D.B) return;
  if (P.status[b] != ST_STEP) return;
  if (threadIdx.x != 0) return;   // sequential control flow per env (v1)

  extern __shared__ char smem[];
  env_step_body(P, D, b, smem, nullptr);
}

// ---------------------------------------------------------------------------
// host binding
// ---------------------------------------------------------------------------

void env_step_batch(std::vector<torch::Tensor> T,
                    std::vector<double> fscal,
                    std::vector<int64_t> iscal) {
  EnvPtrs P;
  EnvDims D;
  env_unpack(T, fscal, iscal, P, D);
  hipStream_t stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(env_step_kernel, dim3(D.B), dim3(64),
                     env_step_scratch_bytes(D), stream, P, D);
}
