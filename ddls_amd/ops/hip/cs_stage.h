// Minibatch stage role shared by batch_stage.hip (cs_stage_kernel, one launch
// of its own) and cached_step.hip (block 0 of the step's first forward
// launch).  The protocol, the guards and the error codes are described at the
// top of batch_stage.hip; both users run this body as ONE 256-thread
// workgroup.
#pragma once
#include <hip/hip_runtime.h>
#include <torch/extension.h>
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

// Called by every thread of one CS_STAGE_THREADS-wide workgroup (barriers
// inside; the early returns are block-uniform).  Takes 4 KB + 4 B of LDS.
__device__ __forceinline__ void cs_stage_body(StagePtrs P, StageDims D) {
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
// host side: argument checks and pointer table
// ===========================================================================

static inline void cs_stage_check_t(const torch::Tensor& t,
                                    c10::ScalarType dt,
                                    const torch::Tensor& like,
                                    const char* who, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.device() == like.device(),
              who, ": ", name, " not on the store's device");
  TORCH_CHECK(t.scalar_type() == dt, who, ": ", name, " dtype");
  TORCH_CHECK(t.is_contiguous(), who, ": ", name, " not contiguous");
}

// store = [gfull, model_ids, actions, old_logp, adv, vtarg]
// dst   = [gf, mask, model_ids, actions, old_logp, adv, vtarg]
// dims  = [n_rows, n_mb] device scalars
// `who` names the binding in the error messages.
static inline void cs_stage_args(StagePtrs& P, StageDims& D, const char* who,
                                 const std::vector<torch::Tensor>& store,
                                 const std::vector<torch::Tensor>& dst,
                                 const torch::Tensor& perm,
                                 const torch::Tensor& cursor,
                                 const torch::Tensor& err,
                                 const std::vector<torch::Tensor>& dims) {
  TORCH_CHECK(store.size() == 6 && dst.size() == 7 && dims.size() == 2,
              who, ": expected 6 store, 7 dst and 2 dims tensors");
  const torch::Tensor& g = store[0];
  TORCH_CHECK(g.is_cuda() && g.dim() == 2, who, ": gfull [cap_n, Fg]");
  D.cap_n = (int)g.size(0);
  D.Fg = (int)g.size(1);
  D.B = (int)dst[0].size(0);
  D.A = (int)dst[1].size(1);
  D.cap_mb = (int)perm.size(0);
  TORCH_CHECK(D.B >= 1 && D.B <= CS_STAGE_MAX_B,
              who, ": minibatch size ", D.B, " outside [1, ",
              CS_STAGE_MAX_B, "]");
  TORCH_CHECK(D.A >= 1 && D.A <= D.Fg, who, ": A outside [1, Fg]");
  TORCH_CHECK(g.size(0) >= 1 && g.size(0) < (1L << 31) / D.Fg,
              who, ": store too large for 32-bit row indices");
  const auto f32 = torch::kFloat32;
  const auto i64 = torch::kInt64;
  const auto i32 = torch::kInt32;
  const c10::ScalarType sdt[6] = {f32, i64, i64, f32, f32, f32};
  const char* sname[6] = {"store.gfull", "store.model_ids", "store.actions",
                          "store.old_logp", "store.adv", "store.vtarg"};
  for (int k = 0; k < 6; ++k) {
    cs_stage_check_t(store[k], sdt[k], g, who, sname[k]);
    TORCH_CHECK(store[k].size(0) == D.cap_n && (k == 0 || store[k].dim() == 1),
                who, ": ", sname[k], " shape");
  }
  const c10::ScalarType ddt[7] = {f32, f32, i64, i64, f32, f32, f32};
  const char* dname[7] = {"gf", "mask", "model_ids", "actions", "old_logp",
                          "adv", "vtarg"};
  for (int k = 0; k < 7; ++k) {
    cs_stage_check_t(dst[k], ddt[k], g, who, dname[k]);
    TORCH_CHECK(dst[k].size(0) == D.B && (k < 2 || dst[k].dim() == 1),
                who, ": ", dname[k], " shape");
  }
  TORCH_CHECK(dst[0].dim() == 2 && dst[0].size(1) == D.Fg
              && dst[1].dim() == 2, who, ": gf/mask shape");
  cs_stage_check_t(perm, i32, g, who, "perm");
  TORCH_CHECK(perm.dim() == 2 && perm.size(1) == D.B,
              who, ": perm [cap_mb, B]");
  cs_stage_check_t(cursor, i32, g, who, "cursor");
  cs_stage_check_t(err, i32, g, who, "err");
  cs_stage_check_t(dims[0], i32, g, who, "n_rows");
  cs_stage_check_t(dims[1], i32, g, who, "n_mb");
  TORCH_CHECK(cursor.numel() == 1 && err.numel() == 1
              && dims[0].numel() == 1 && dims[1].numel() == 1,
              who, ": cursor/err/n_rows/n_mb are [1] tensors");

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
}
