// Fused rollout for the env engine on gfx950: ONE launch carries every env
// through up to T steps of  actor row -> env step -> stores of row t.
//
// The per-step path (actor_batch + env_step_batch + a status read-back per
// step) is bound by launches and host syncs, not by arithmetic.  The envs are
// independent, so one wave can keep an env for many steps and stop only where
// the host is really needed: an episode end (the host drains the next
// schedule) or a memo miss (the host inserts into the hash table).
//
// Work split: one wave per env, WPB envs per workgroup (WPB <= 4, picked by
// the binding from the LDS budget).  Lane l owns column l of the actor row as
// in actor.hip; lane 0 runs the sequential env step (env_step_body.h).
//
// LDS (dynamic, carved below):
//   per workgroup, policy modes only, staged ONCE per launch:
//     W1p, W1v [2][256][24+1]   Wg [8][64+1]   W2p [A][256+1]
//     ln_w ln_b bg b1p b2p b1v W2v b2v         model_emb [M][16] if it fits
//   per wave:
//     hand [68]: the observation the env step hands to the next actor row
//                (gf 17, mask A, then model id and schedule slot as ints)
//     yln [68], emb [28], h1 [256]             (policy modes)
//     the env step's placement scratch         (env_step_scratch_bytes)
// The heuristic instantiation stages nothing.
//
// Arithmetic is actor_row.h and env_step_body.h, the bodies actor_kernel and
// env_step_kernel run, with the Philox counter (b, step0 + t, 0): the result
// is bit-equal to T alternations of those two kernels.
//
// Stop protocol (no inter-block waiting anywhere): a wave leaves its loop
// when t == T (WHY_T), when the step set done (WHY_DONE, stop_t = t + 1),
// when the step missed the memo (WHY_MISS, stop_t = t, state untouched, row t
// is rewritten with identical values on resume) or on ST_ERR (WHY_ERR).
#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>
#include <vector>

#include "actor_row.h"
#include "env_step_body.h"

#define MAX_WPB 4
#define MAX_STEPS 4096
#define HAND 68          // floats per wave: 17 + 32 obs, 2 ints at [64], [65]
#define YLN 68
#define EMBW 28
#define W2P_LD (H1 + 1)
#define VEC_FLOATS (64 + 64 + 8 + H1 + 32 + H1 + H1 + 8)

enum { WHY_T = 0, WHY_DONE = 1, WHY_MISS = 2, WHY_ERR = 3 };
enum { R_GFULL = 0, R_LP_ALL, R_LOGP, R_VALUE, R_U, R_ACTIONS, R_MODEL,
       R_REWARDS, R_DONES, R_RET, R_NLIVE, R_COUNT };

struct RolloutArgs {
  // actor
  const float* model_emb;   // [M,16] (policy modes)
  const float* head[12];    // head_fwd's parameter order (policy modes)
  int M, mode, sip_ml_cap;
  unsigned seed_lo, seed_hi;
  unsigned long long step0;
  // rows [T,B,...]; null = not written
  float *gfull, *lp_all, *logp, *value, *u, *rewards;
  long *actions, *model;
  uint8_t* dones;
  double* ret;              // [B] += reward in step order
  long* nlive;              // [B] += 1 per step taken
  // control
  const int* t0;            // [B] first step of env b; outside [0,T) = skip
  int* stop;                // [4,B]: stop_t, why, miss model, miss action
  int* eng_actions;         // the engine's own actions tensor [B]
  int T, emb_in_lds, wave_bytes;
};

template <bool POLICY>
__global__ void __launch_bounds__(WAVE * MAX_WPB)
env_rollout_kernel(EnvPtrs P, EnvDims D, RolloutArgs R) {
  extern __shared__ __align__(16) char lds[];
  const int A = D.A, B = D.B, Fg = NGF + A, M = R.M;
  const int nthr = blockDim.x, wpb = blockDim.x / WAVE;
  float* f = (float*)lds;
  const float (*w1s)[H1][EMB + 1] = nullptr;
  const float (*wgs)[64 + 1] = nullptr;
  ActorHead W = {};
  const float* embt = R.model_emb;
  if constexpr (POLICY) {
    float (*w1)[H1][EMB + 1] = (float (*)[H1][EMB + 1])f;
    f += 2 * H1 * (EMB + 1);
    float (*wg)[64 + 1] = (float (*)[64 + 1])f;
    f += GEMB * (64 + 1);
    float* w2p = f;  f += A * W2P_LD;
    float* ln_w = f; f += 64;
    float* ln_b = f; f += 64;
    float* bg = f;   f += 8;
    float* b1p = f;  f += H1;
    float* b2p = f;  f += 32;
    float* b1v = f;  f += H1;
    float* w2v = f;  f += H1;
    float* b2v = f;  f += 8;
    for (int i = threadIdx.x; i < H1 * EMB; i += nthr) {
      w1[0][i / EMB][i % EMB] = R.head[4][i];
      w1[1][i / EMB][i % EMB] = R.head[8][i];
    }
    for (int i = threadIdx.x; i < GEMB * Fg; i += nthr)
      wg[i / Fg][i % Fg] = R.head[2][i];
    for (int i = threadIdx.x; i < A * H1; i += nthr)
      w2p[(i / H1) * W2P_LD + i % H1] = R.head[6][i];
    for (int i = threadIdx.x; i < H1; i += nthr) {
      b1p[i] = R.head[5][i];
      b1v[i] = R.head[9][i];
      w2v[i] = R.head[10][i];
    }
    for (int i = threadIdx.x; i < Fg; i += nthr) {
      ln_w[i] = R.head[0][i];
      ln_b[i] = R.head[1][i];
    }
    if (threadIdx.x < GEMB) bg[threadIdx.x] = R.head[3][threadIdx.x];
    if (threadIdx.x < A) b2p[threadIdx.x] = R.head[7][threadIdx.x];
    if (threadIdx.x == 0) b2v[0] = R.head[11][0];
    if (R.emb_in_lds) {
      for (int i = threadIdx.x; i < M * 16; i += nthr) f[i] = R.model_emb[i];
      embt = f;
      f += M * 16;
    }
    // the waves' regions hold f64 scratch: keep them 8-byte aligned
    f = (float*)lds + (((f - (float*)lds) + 1) & ~1L);
    w1s = w1;
    wgs = wg;
    W = {ln_w, ln_b, bg, b1p, w2p, b2p, b1v, w2v, b2v, W2P_LD};
    __syncthreads();
  }

  const int wave = threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  const int b = blockIdx.x * wpb + wave;
  if (b >= B) return;                       // no block barrier below
  char* mine = (char*)f + (long)wave * R.wave_bytes;
  float* hand = (float*)mine;
  float* yln = hand + HAND;
  float* embw = yln + (POLICY ? YLN : 0);
  float* h1 = embw + (POLICY ? EMBW : 0);
  char* step_lds = (char*)(h1 + (POLICY ? H1 : 0));

  int* stop_t = R.stop + b;
  int* stop_why = R.stop + B + b;
  int t = R.t0[b];
  if (t < 0 || t >= R.T) {                  // nothing to do for this env
    if (lane == 0) { *stop_t = R.T; *stop_why = WHY_T; }
    return;
  }
  if (P.done[b] != 0) {                     // the host resets, or leaves it
    if (lane == 0) { *stop_t = t; *stop_why = WHY_DONE; }
    return;
  }
  // the first row's observation comes from the engine's tensors; every later
  // one is handed over in LDS by the env step of the same wave
  if (lane < NGF) hand[lane] = P.obs_gf[(long)b * NGF + lane];
  else if (lane < Fg) hand[lane] = P.obs_mask[(long)b * A + (lane - NGF)];
  if (lane == 0) {
    ((int*)hand)[64] = P.obs_model[b];
    ((int*)hand)[65] = P.obs_sched[b];
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();

  int why = WHY_T;
  for (; t < R.T; ++t) {
    const long tb = (long)t * B + b;
    const int mid = ((const int*)hand)[64];
    const int ksch = ((const int*)hand)[65];
    int act = 0;
    if (mid >= 0 && mid < M) {              // else actor.hip's done rule
      const unsigned long long step = R.step0 + (unsigned long long)t;
      double seq = 0.0;
      if (!POLICY && R.mode == ACCEPTABLE_JCT) seq = P.model_seq[mid];
      const ActorRowOut out = {
          POLICY ? R.gfull + tb * Fg : nullptr,
          POLICY ? R.lp_all + tb * A : nullptr,
          POLICY ? R.logp + tb : nullptr, POLICY ? R.value + tb : nullptr,
          R.u != nullptr ? R.u + tb : nullptr};
      act = actor_row<POLICY>(
          lane, (unsigned)b, hand, hand + NGF,
          POLICY ? embt + (long)mid * 16 : nullptr, ksch, seq,
          P.sch_acc + (long)b * D.SCH, D.SCH, w1s, wgs, yln, embw, h1, W, out,
          A, R.mode, R.sip_ml_cap, R.seed_lo, R.seed_hi,
          (unsigned)(step & 0xffffffffull), (unsigned)(step >> 32));
    }
    __builtin_amdgcn_wave_barrier();
    int st = ST_ERR, dn = 0;
    if (lane == 0) {
      R.eng_actions[b] = act;
      if (R.actions != nullptr) R.actions[tb] = act;
      if (R.model != nullptr) R.model[tb] = mid;
      P.status[b] = ST_STEP;
      env_step_body(P, D, b, step_lds, hand);
      st = P.status[b];
      if (st == ST_OK) {
        const double r = P.reward[b];
        dn = P.step_done[b];
        if (R.rewards != nullptr) R.rewards[tb] = (float)r;
        if (R.dones != nullptr) R.dones[tb] = (uint8_t)dn;
        if (R.ret != nullptr) R.ret[b] += r;
        if (R.nlive != nullptr) R.nlive[b] += 1;
      } else if (st == ST_MISS) {
        R.stop[2 * B + b] = mid;
        R.stop[3 * B + b] = act;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    st = __shfl(st, 0, WAVE);
    dn = __shfl(dn, 0, WAVE);
    if (st == ST_MISS) { why = WHY_MISS; break; }
    if (st != ST_OK) { why = WHY_ERR; break; }
    if (dn != 0) { why = WHY_DONE; ++t; break; }
  }
  if (lane == 0) { *stop_t = t; *stop_why = why; }
}

// ---------------------------------------------------------------------------
// host binding
// ---------------------------------------------------------------------------
template <typename scalar>
static scalar* row_ptr(const torch::Tensor& t, torch::ScalarType dt,
                       int64_t numel, const char* what) {
  if (t.numel() == 0) return nullptr;
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == dt && t.is_contiguous() &&
              t.numel() == numel, "env_rollout_batch: ", what,
              " must be a contiguous device tensor of ", numel,
              " elements of its dtype");
  return t.data_ptr<scalar>();
}

// Returns {envs per workgroup, LDS bytes per workgroup, 1 if the embedding
// table was staged in LDS}.
std::vector<int64_t> env_rollout_batch(
    std::vector<torch::Tensor> T, std::vector<double> fscal,
    std::vector<int64_t> iscal, torch::Tensor model_emb,
    std::vector<torch::Tensor> head, int64_t mode, int64_t sip_ml_cap,
    uint64_t seed, uint64_t step0, int64_t steps, torch::Tensor t0,
    torch::Tensor stop, std::vector<torch::Tensor> rows) {
  EnvPtrs P;
  EnvDims D;
  env_unpack(T, fscal, iscal, P, D);
  const int64_t B = D.B, A = D.A, Fg = NGF + A;
  TORCH_CHECK(mode >= POLICY_GREEDY && mode <= ACCEPTABLE_JCT,
              "env_rollout_batch: unknown mode ", mode);
  TORCH_CHECK(A >= 1 && A <= 32 && Fg <= 64,
              "env_rollout_batch: needs 1 <= A <= 32 and 17 + A <= 64");
  TORCH_CHECK(steps >= 1 && steps <= MAX_STEPS, "env_rollout_batch: steps "
              "must be in [1, ", MAX_STEPS, "] per launch; chunk above it");
  TORCH_CHECK((int64_t)rows.size() == R_COUNT,
              "env_rollout_batch: rows takes ", (int)R_COUNT, " tensors");
  for (int k : {T_OBS_GF, T_OBS_MASK, T_OBS_MODEL, T_OBS_SCHED, T_DONE,
                T_STATUS, T_REWARD, T_STEP_DONE, T_ACTIONS})
    TORCH_CHECK(T[k].is_cuda() && T[k].is_contiguous() && T[k].size(0) == B,
                "env_rollout_batch: engine tensor ", k, " is not [B, ...]");
  TORCH_CHECK(T[T_OBS_MASK].numel() == B * A && T[T_OBS_GF].numel() == B * NGF,
              "env_rollout_batch: obs_gf / obs_mask shape");
  TORCH_CHECK(T[T_SCH_ACC].numel() == B * (int64_t)D.SCH,
              "env_rollout_batch: sch_acc must be [B,SCH]");
  auto i32 = [&](const torch::Tensor& t, int64_t n, const char* what) {
    TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kInt32 &&
                t.is_contiguous() && t.numel() == n,
                "env_rollout_batch: ", what, " must be a contiguous i32 "
                "device tensor of ", n, " elements");
    return t.data_ptr<int>();
  };

  RolloutArgs R = {};
  R.t0 = i32(t0, B, "t0");
  R.stop = i32(stop, 4 * B, "stop");
  R.eng_actions = T[T_ACTIONS].data_ptr<int>();
  R.T = (int)steps;
  R.mode = (int)mode;
  R.sip_ml_cap = (int)sip_ml_cap;
  R.seed_lo = (unsigned)(seed & 0xffffffffu);
  R.seed_hi = (unsigned)(seed >> 32);
  R.step0 = step0;
  const bool policy = mode == POLICY_GREEDY || mode == POLICY_SAMPLE;
  const int64_t TB = steps * B;
  R.u = row_ptr<float>(rows[R_U], torch::kFloat32, TB, "u");
  R.rewards = row_ptr<float>(rows[R_REWARDS], torch::kFloat32, TB, "rewards");
  R.actions = (long*)row_ptr<int64_t>(rows[R_ACTIONS], torch::kInt64, TB,
                                      "actions");
  R.model = (long*)row_ptr<int64_t>(rows[R_MODEL], torch::kInt64, TB, "model");
  R.dones = row_ptr<uint8_t>(rows[R_DONES], torch::kUInt8, TB, "dones");
  R.ret = row_ptr<double>(rows[R_RET], torch::kFloat64, B, "ret");
  R.nlive = (long*)row_ptr<int64_t>(rows[R_NLIVE], torch::kInt64, B, "nlive");

  size_t shared_bytes = 0, wave_bytes = HAND * sizeof(float);
  if (policy) {
    TORCH_CHECK(model_emb.is_cuda() && model_emb.dim() == 2 &&
                model_emb.size(1) == 16 &&
                model_emb.scalar_type() == torch::kFloat32 &&
                model_emb.is_contiguous(),
                "env_rollout_batch: model_emb must be a contiguous f32 "
                "[M,16] device tensor");
    R.M = (int)model_emb.size(0);
    R.model_emb = model_emb.data_ptr<float>();
    TORCH_CHECK(head.size() == 12, "env_rollout_batch: the policy modes take "
                "head_fwd's 12 parameter tensors");
    const int64_t want[12] = {Fg, Fg, GEMB * Fg, GEMB, H1 * EMB, H1,
                              A * H1, A, H1 * EMB, H1, H1, 1};
    for (int i = 0; i < 12; ++i) {
      TORCH_CHECK(head[i].is_cuda() &&
                  head[i].scalar_type() == torch::kFloat32 &&
                  head[i].is_contiguous() && head[i].numel() == want[i],
                  "env_rollout_batch: head[", i, "] must be a contiguous f32 "
                  "device tensor of ", want[i], " elements");
      R.head[i] = head[i].data_ptr<float>();
    }
    for (int k : {R_GFULL, R_LP_ALL, R_LOGP, R_VALUE})
      TORCH_CHECK(rows[k].numel() > 0, "env_rollout_batch: the policy modes "
                  "fill gfull, lp_all, logp and value");
    R.gfull = row_ptr<float>(rows[R_GFULL], torch::kFloat32, TB * Fg, "gfull");
    R.lp_all = row_ptr<float>(rows[R_LP_ALL], torch::kFloat32, TB * A,
                              "lp_all");
    R.logp = row_ptr<float>(rows[R_LOGP], torch::kFloat32, TB, "logp");
    R.value = row_ptr<float>(rows[R_VALUE], torch::kFloat32, TB, "value");
    shared_bytes = (2 * H1 * (EMB + 1) + GEMB * (64 + 1) + A * W2P_LD +
                    VEC_FLOATS) * sizeof(float);
    // alignment pad in front of the waves' regions (they hold f64 scratch)
    shared_bytes = (shared_bytes + 8 + 7) & ~(size_t)7;
    wave_bytes += (YLN + EMBW + H1) * sizeof(float);
  } else {
    // M only bounds the model id: heuristics index model_seq alone
    R.M = (int)T[T_MODEL_SEQ].numel();
  }
  wave_bytes = (wave_bytes + env_step_scratch_bytes(D) + 7) & ~(size_t)7;
  if (B == 0) return {0, 0, 0};

  // envs per workgroup and the embedding table from the LDS budget
  int dev = 0, budget = 0;
  TORCH_CHECK(hipGetDevice(&dev) == hipSuccess &&
              hipDeviceGetAttribute(&budget,
                  hipDeviceAttributeMaxSharedMemoryPerBlock, dev) == hipSuccess,
              "env_rollout_batch: cannot read the LDS size");
  int wpb = MAX_WPB;
  while (wpb > 1 && shared_bytes + wpb * wave_bytes > (size_t)budget) --wpb;
  TORCH_CHECK(shared_bytes + wpb * wave_bytes <= (size_t)budget,
              "env_rollout_batch: one env needs ", shared_bytes + wave_bytes,
              " bytes of LDS, the device has ", budget);
  const size_t emb_bytes = (size_t)R.M * 16 * sizeof(float);
  R.emb_in_lds = policy &&
      shared_bytes + emb_bytes + wpb * wave_bytes <= (size_t)budget;
  if (R.emb_in_lds) shared_bytes += emb_bytes;
  R.wave_bytes = (int)wave_bytes;
  const size_t lds_bytes = shared_bytes + wpb * wave_bytes;

  hipStream_t stream = at::cuda::getCurrentCUDAStream();
  const dim3 grid((unsigned)((B + wpb - 1) / wpb)), block(WAVE * wpb);
  auto launch = [&](auto kernel) {
    if (lds_bytes > 64 * 1024)
      TORCH_CHECK(hipFuncSetAttribute(
                      reinterpret_cast<const void*>(kernel),
                      hipFuncAttributeMaxDynamicSharedMemorySize,
                      (int)lds_bytes) == hipSuccess,
                  "env_rollout_batch: cannot raise the dynamic LDS limit to ",
                  lds_bytes);
    hipLaunchKernelGGL(kernel, grid, block, lds_bytes, stream, P, D, R);
  };
  if (policy) launch(env_rollout_kernel<true>);
  else launch(env_rollout_kernel<false>);
  TORCH_CHECK(hipGetLastError() == hipSuccess,
              "env_rollout_batch: launch failed");
  return {wpb, (int64_t)lds_bytes, R.emb_in_lds};
}
