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

#define CS_STAGE_THREADS 256
#define CS_STAGE_MAX_B 1024
#define CS_STAGE_BYPASS (-1)
#define CS_STAGE_ERR_CURSOR 1
#define CS_STAGE_ERR_INDEX 2

struct StagePtrs {
  // store
  const float* s_gfull;
  const long* s_model_ids;
  const long* s_actions;
  const float* s_old_logp;
  const float* s_adv;
  const float* s_vtarg;
  const int* perm;
  const int* n_rows;
  const int* n_mb;
  int* cursor;
  int* err;
  // staged inputs of cached_step_fwd
  float* gf;
  float* mask;
  long* model_ids;
  long* actions;
  float* old_logp;
  float* adv;
  float* vtarg;
};

struct StageDims {
  int B, Fg, A, cap_n, cap_mb;
};

__global__ __launch_bounds__(CS_STAGE_THREADS) void cs_stage_kernel(
    StagePtrs P, StageDims D) {
  __shared__ int s_idx[CS_STAGE_MAX_B];
  __shared__ int s_bad;
  const int tid = threadIdx.x;
  const int cur = *P.cursor;
  const int n_rows = *P.n_rows;
  const int n_mb = *P.n_mb;
  if (tid == 0) s_bad = 0;
  __syncthreads();   // every thread holds the cursor; s_bad initialised
  if (cur == CS_STAGE_BYPASS) return;
  if (cur < 0 || cur >= n_mb || cur >= D.cap_mb) {
    if (tid == 0) *P.err = CS_STAGE_ERR_CURSOR;
    return;
  }
  const int row_hi = n_rows < D.cap_n ? n_rows : D.cap_n;
  const int* prow = P.perm + (long)cur * D.B;
  for (int i = tid; i < D.B; i += CS_STAGE_THREADS) {
    const int r = prow[i];
    s_idx[i] = r;
    if (r < 0 || r >= row_hi) s_bad = 1;   // same value from every writer
  }
  __syncthreads();
  if (s_bad) {
    if (tid == 0) *P.err = CS_STAGE_ERR_INDEX;
    return;
  }
  // gf rows: consecutive lanes take consecutive floats of a row (136 B rows,
  // dense stores); the trailing A columns are the action mask
  const int total = D.B * D.Fg;
  const int m0 = D.Fg - D.A;
  for (int e = tid; e < total; e += CS_STAGE_THREADS) {
    const int i = e / D.Fg;
    const int c = e - i * D.Fg;
    const float v = P.s_gfull[(long)s_idx[i] * D.Fg + c];
    P.gf[e] = v;
    if (c >= m0) P.mask[i * D.A + (c - m0)] = v;
  }
  for (int i = tid; i < D.B; i += CS_STAGE_THREADS) {
    const long r = s_idx[i];
    P.model_ids[i] = P.s_model_ids[r];
    P.actions[i] = P.s_actions[r];
    P.old_logp[i] = P.s_old_logp[r];
    P.adv[i] = P.s_adv[r];
    P.vtarg[i] = P.s_vtarg[r];
  }
  if (tid == 0) *P.cursor = cur + 1;
}

// ===========================================================================
// host binding
// ===========================================================================

static void check_t(const torch::Tensor& t, c10::ScalarType dt,
                    const torch::Tensor& like, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.device() == like.device(),
              "cached_stage: ", name, " not on the store's device");
  TORCH_CHECK(t.scalar_type() == dt, "cached_stage: ", name, " dtype");
  TORCH_CHECK(t.is_contiguous(), "cached_stage: ", name, " not contiguous");
}

// store = [gfull, model_ids, actions, old_logp, adv, vtarg]
// dst   = [gf, mask, model_ids, actions, old_logp, adv, vtarg]
// dims  = [n_rows, n_mb] device scalars
void cached_stage(std::vector<torch::Tensor> store,
                  std::vector<torch::Tensor> dst, torch::Tensor perm,
                  torch::Tensor cursor, torch::Tensor err,
                  std::vector<torch::Tensor> dims) {
  TORCH_CHECK(store.size() == 6 && dst.size() == 7 && dims.size() == 2,
              "cached_stage: expected 6 store, 7 dst and 2 dims tensors");
  const torch::Tensor& g = store[0];
  TORCH_CHECK(g.is_cuda() && g.dim() == 2, "cached_stage: gfull [cap_n, Fg]");
  StageDims D;
  D.cap_n = (int)g.size(0);
  D.Fg = (int)g.size(1);
  D.B = (int)dst[0].size(0);
  D.A = (int)dst[1].size(1);
  D.cap_mb = (int)perm.size(0);
  TORCH_CHECK(D.B >= 1 && D.B <= CS_STAGE_MAX_B,
              "cached_stage: minibatch size ", D.B, " outside [1, ",
              CS_STAGE_MAX_B, "]");
  TORCH_CHECK(D.A >= 1 && D.A <= D.Fg, "cached_stage: A outside [1, Fg]");
  TORCH_CHECK(g.size(0) >= 1 && g.size(0) < (1L << 31) / D.Fg,
              "cached_stage: store too large for 32-bit row indices");
  const auto f32 = torch::kFloat32;
  const auto i64 = torch::kInt64;
  const auto i32 = torch::kInt32;
  const c10::ScalarType sdt[6] = {f32, i64, i64, f32, f32, f32};
  const char* sname[6] = {"store.gfull", "store.model_ids", "store.actions",
                          "store.old_logp", "store.adv", "store.vtarg"};
  for (int k = 0; k < 6; ++k) {
    check_t(store[k], sdt[k], g, sname[k]);
    TORCH_CHECK(store[k].size(0) == D.cap_n && (k == 0 || store[k].dim() == 1),
                "cached_stage: ", sname[k], " shape");
  }
  const c10::ScalarType ddt[7] = {f32, f32, i64, i64, f32, f32, f32};
  const char* dname[7] = {"gf", "mask", "model_ids", "actions", "old_logp",
                          "adv", "vtarg"};
  for (int k = 0; k < 7; ++k) {
    check_t(dst[k], ddt[k], g, dname[k]);
    TORCH_CHECK(dst[k].size(0) == D.B && (k < 2 || dst[k].dim() == 1),
                "cached_stage: ", dname[k], " shape");
  }
  TORCH_CHECK(dst[0].dim() == 2 && dst[0].size(1) == D.Fg
              && dst[1].dim() == 2, "cached_stage: gf/mask shape");
  check_t(perm, i32, g, "perm");
  TORCH_CHECK(perm.dim() == 2 && perm.size(1) == D.B,
              "cached_stage: perm [cap_mb, B]");
  check_t(cursor, i32, g, "cursor");
  check_t(err, i32, g, "err");
  check_t(dims[0], i32, g, "n_rows");
  check_t(dims[1], i32, g, "n_mb");
  TORCH_CHECK(cursor.numel() == 1 && err.numel() == 1
              && dims[0].numel() == 1 && dims[1].numel() == 1,
              "cached_stage: cursor/err/n_rows/n_mb are [1] tensors");

  StagePtrs P;
  P.s_gfull = store[0].data_ptr<float>();
  P.s_model_ids = store[1].data_ptr<long>();
  P.s_actions = store[2].data_ptr<long>();
  P.s_old_logp = store[3].data_ptr<float>();
  P.s_adv = store[4].data_ptr<float>();
  P.s_vtarg = store[5].data_ptr<float>();
  P.perm = perm.data_ptr<int>();
  P.n_rows = dims[0].data_ptr<int>();
  P.n_mb = dims[1].data_ptr<int>();
  P.cursor = cursor.data_ptr<int>();
  P.err = err.data_ptr<int>();
  P.gf = dst[0].data_ptr<float>();
  P.mask = dst[1].data_ptr<float>();
  P.model_ids = dst[2].data_ptr<long>();
  P.actions = dst[3].data_ptr<long>();
  P.old_logp = dst[4].data_ptr<float>();
  P.adv = dst[5].data_ptr<float>();
  P.vtarg = dst[6].data_ptr<float>();
  hipStream_t stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(cs_stage_kernel, dim3(1), dim3(CS_STAGE_THREADS), 0,
                     stream, P, D);
}
