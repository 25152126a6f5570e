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
// Population variant (env_rollout_pop_kernel, for rl/es_population.py): the
// grid is (ceil(E / WPB), P) and every wave of a workgroup serves member
// m = blockIdx.y.  The workgroup stages member m's head from row m of the
// [P, n] population matrix (pop + m * n + head_offs[i], 4-byte loads: rows
// are not 16-byte aligned) and model_emb_pop[m]; wave `e` owns engine row
// b = m * E + e and draws with the Philox index e, not b (common random
// numbers: every member sees the uniforms of a batch of E rows).  Staging,
// the LDS carve-up, the step loop and the stop protocol are the functions
// below, shared by both kernels; the variant keeps no [T, B, ...] rows but
// the optional actions row.
//
// Stop protocol (no inter-block waiting anywhere): a wave leaves its loop
// when t == T (WHY_T), when the step set done (WHY_DONE, stop_t = t + 1),
// when the step missed the memo (WHY_MISS, stop_t = t, state untouched, row t
// is rewritten with identical values on resume) or on ST_ERR (WHY_ERR).
#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>
#include <utility>
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

// the staged head of a workgroup and where the waves' regions start
struct HeadLds {
  const float (*w1s)[H1][EMB + 1];
  const float (*wgs)[64 + 1];
  ActorHead W;
  const float* embt;        // [M,16]: LDS when it fits, else global
  float* waves;
};

// Stages the 12 head tensors (head_fwd's order; 4-byte loads, no alignment
// assumed) and, with `emb_in_lds`, the embedding table into LDS.  The whole
// workgroup calls this; it ends in the kernel's ONE block barrier.
__device__ __forceinline__ HeadLds stage_head(
    float* f, const float* const* head, const float* model_emb, int M,
    int emb_in_lds, int A) {
  const int Fg = NGF + A, nthr = blockDim.x;
  float* const lds0 = f;
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
    w1[0][i / EMB][i % EMB] = head[4][i];
    w1[1][i / EMB][i % EMB] = head[8][i];
  }
  for (int i = threadIdx.x; i < GEMB * Fg; i += nthr)
    wg[i / Fg][i % Fg] = head[2][i];
  for (int i = threadIdx.x; i < A * H1; i += nthr)
    w2p[(i / H1) * W2P_LD + i % H1] = head[6][i];
  for (int i = threadIdx.x; i < H1; i += nthr) {
    b1p[i] = head[5][i];
    b1v[i] = head[9][i];
    w2v[i] = head[10][i];
  }
  for (int i = threadIdx.x; i < Fg; i += nthr) {
    ln_w[i] = head[0][i];
    ln_b[i] = head[1][i];
  }
  if (threadIdx.x < GEMB) bg[threadIdx.x] = head[3][threadIdx.x];
  if (threadIdx.x < A) b2p[threadIdx.x] = head[7][threadIdx.x];
  if (threadIdx.x == 0) b2v[0] = head[11][0];
  const float* embt = model_emb;
  if (emb_in_lds) {
    for (int i = threadIdx.x; i < M * 16; i += nthr) f[i] = model_emb[i];
    embt = f;
    f += M * 16;
  }
  // the waves' regions hold f64 scratch: keep them 8-byte aligned
  f = lds0 + (((f - lds0) + 1) & ~1L);
  __syncthreads();
  return {w1, wg, {ln_w, ln_b, bg, b1p, w2p, b2p, b1v, w2v, b2v, W2P_LD},
          embt, f};
}

// One wave carries env row `b` from step t0[b] to its stop.  `ctr0` is word 0
// of the Philox counter (the row for one policy, e = b % E for a population);
// `mine` is the wave's own LDS region of R.wave_bytes.  No block barrier.
template <bool POLICY>
__device__ __forceinline__ void rollout_wave(
    const EnvPtrs& P, const EnvDims& D, const RolloutArgs& R, int b,
    unsigned ctr0, int lane, char* mine, const HeadLds& H) {
  const int A = D.A, B = D.B, Fg = NGF + A, M = R.M;
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
          R.gfull != nullptr ? R.gfull + tb * Fg : nullptr,
          R.lp_all != nullptr ? R.lp_all + tb * A : nullptr,
          R.logp != nullptr ? R.logp + tb : nullptr,
          R.value != nullptr ? R.value + tb : nullptr,
          R.u != nullptr ? R.u + tb : nullptr};
      act = actor_row<POLICY>(
          lane, ctr0, hand, hand + NGF,
          POLICY ? H.embt + (long)mid * 16 : nullptr, ksch, seq,
          P.sch_acc + (long)b * D.SCH, D.SCH, H.w1s, H.wgs, yln, embw, h1,
          H.W, out, A, R.mode, R.sip_ml_cap, R.seed_lo, R.seed_hi,
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

template <bool POLICY>
__global__ void __launch_bounds__(WAVE * MAX_WPB)
env_rollout_kernel(EnvPtrs P, EnvDims D, RolloutArgs R) {
  extern __shared__ __align__(16) char lds[];
  HeadLds H = {};
  H.embt = R.model_emb;
  H.waves = (float*)lds;
  if constexpr (POLICY)
    H = stage_head((float*)lds, R.head, R.model_emb, R.M, R.emb_in_lds, D.A);
  const int wave = threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  const int b = blockIdx.x * (blockDim.x / WAVE) + wave;
  if (b >= D.B) return;                     // no block barrier below
  rollout_wave<POLICY>(P, D, R, b, (unsigned)b, lane,
                       (char*)H.waves + (long)wave * R.wave_bytes, H);
}

// where member m's head and embedding table are
struct PopArgs {
  const float* pop;         // [P,n]
  long n;
  long off[12];             // head_fwd's parameter order, inside a pop row
  int E;
};

// R.model_emb is model_emb_pop [P,M,16]; R.head is not used
__global__ void __launch_bounds__(WAVE * MAX_WPB)
env_rollout_pop_kernel(EnvPtrs P, EnvDims D, RolloutArgs R, PopArgs Q) {
  extern __shared__ __align__(16) char lds[];
  const int m = blockIdx.y;
  const float* th = Q.pop + (long)m * Q.n;
  const float* head[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) head[i] = th + Q.off[i];
  const HeadLds H = stage_head((float*)lds, head,
                               R.model_emb + (long)m * R.M * 16, R.M,
                               R.emb_in_lds, D.A);
  const int wave = threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  const int e = blockIdx.x * (blockDim.x / WAVE) + wave;
  if (e >= Q.E) return;                     // no block barrier below
  rollout_wave<true>(P, D, R, m * Q.E + e, (unsigned)e, lane,
                     (char*)H.waves + (long)wave * R.wave_bytes, H);
}

// ---------------------------------------------------------------------------
// host bindings
// ---------------------------------------------------------------------------
template <typename scalar>
static scalar* row_ptr(const char* op, const torch::Tensor& t,
                       torch::ScalarType dt, int64_t numel, const char* what) {
  if (t.numel() == 0) return nullptr;
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == dt && t.is_contiguous() &&
              t.numel() == numel, op, ": ", what,
              " must be a contiguous device tensor of ", numel,
              " elements of its dtype");
  return t.data_ptr<scalar>();
}

// What both bindings share: the engine's tensors and scalars, the control
// arrays and the actor's scalars.
static void rollout_setup(
    const char* op, const std::vector<torch::Tensor>& T,
    const std::vector<double>& fscal, const std::vector<int64_t>& iscal,
    int64_t mode, int64_t sip_ml_cap, uint64_t seed, uint64_t step0,
    int64_t steps, const torch::Tensor& t0, const torch::Tensor& stop,
    EnvPtrs& P, EnvDims& D, RolloutArgs& R) {
  env_unpack(T, fscal, iscal, P, D);
  const int64_t B = D.B, A = D.A, Fg = NGF + A;
  TORCH_CHECK(A >= 1 && A <= 32 && Fg <= 64,
              op, ": needs 1 <= A <= 32 and 17 + A <= 64");
  TORCH_CHECK(steps >= 1 && steps <= MAX_STEPS, op, ": steps "
              "must be in [1, ", MAX_STEPS, "] per launch; chunk above it");
  for (int k : {T_OBS_GF, T_OBS_MASK, T_OBS_MODEL, T_OBS_SCHED, T_DONE,
                T_STATUS, T_REWARD, T_STEP_DONE, T_ACTIONS})
    TORCH_CHECK(T[k].is_cuda() && T[k].is_contiguous() && T[k].size(0) == B,
                op, ": engine tensor ", k, " is not [B, ...]");
  TORCH_CHECK(T[T_OBS_MASK].numel() == B * A && T[T_OBS_GF].numel() == B * NGF,
              op, ": obs_gf / obs_mask shape");
  TORCH_CHECK(T[T_SCH_ACC].numel() == B * (int64_t)D.SCH,
              op, ": sch_acc must be [B,SCH]");
  auto i32 = [&](const torch::Tensor& t, int64_t n, const char* what) {
    TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kInt32 &&
                t.is_contiguous() && t.numel() == n,
                op, ": ", what, " must be a contiguous i32 "
                "device tensor of ", n, " elements");
    return t.data_ptr<int>();
  };
  R.t0 = i32(t0, B, "t0");
  R.stop = i32(stop, 4 * B, "stop");
  R.eng_actions = T[T_ACTIONS].data_ptr<int>();
  R.T = (int)steps;
  R.mode = (int)mode;
  R.sip_ml_cap = (int)sip_ml_cap;
  R.seed_lo = (unsigned)(seed & 0xffffffffu);
  R.seed_hi = (unsigned)(seed >> 32);
  R.step0 = step0;
}

// Envs per workgroup (at most `max_wpb`) and whether the embedding table is
// staged, from the device's LDS budget; fills R.emb_in_lds / R.wave_bytes.
// Returns {wpb, LDS bytes per workgroup}.
static std::pair<int, size_t> rollout_lds_plan(
    const char* op, bool policy, const EnvDims& D, RolloutArgs& R,
    int max_wpb) {
  size_t shared_bytes = 0, wave_bytes = HAND * sizeof(float);
  if (policy) {
    shared_bytes = (2 * H1 * (EMB + 1) + GEMB * (64 + 1) + D.A * W2P_LD +
                    VEC_FLOATS) * sizeof(float);
    // alignment pad in front of the waves' regions (they hold f64 scratch)
    shared_bytes = (shared_bytes + 8 + 7) & ~(size_t)7;
    wave_bytes += (YLN + EMBW + H1) * sizeof(float);
  }
  wave_bytes = (wave_bytes + env_step_scratch_bytes(D) + 7) & ~(size_t)7;
  int dev = 0, budget = 0;
  TORCH_CHECK(hipGetDevice(&dev) == hipSuccess &&
              hipDeviceGetAttribute(&budget,
                  hipDeviceAttributeMaxSharedMemoryPerBlock, dev) == hipSuccess,
              op, ": cannot read the LDS size");
  int wpb = max_wpb;
  while (wpb > 1 && shared_bytes + wpb * wave_bytes > (size_t)budget) --wpb;
  TORCH_CHECK(shared_bytes + wpb * wave_bytes <= (size_t)budget,
              op, ": one env needs ", shared_bytes + wave_bytes,
              " bytes of LDS, the device has ", budget);
  const size_t emb_bytes = (size_t)R.M * 16 * sizeof(float);
  R.emb_in_lds = policy &&
      shared_bytes + emb_bytes + wpb * wave_bytes <= (size_t)budget;
  if (R.emb_in_lds) shared_bytes += emb_bytes;
  R.wave_bytes = (int)wave_bytes;
  return {wpb, shared_bytes + wpb * wave_bytes};
}

template <typename Kernel, typename... Args>
static void rollout_launch(const char* op, Kernel kernel, dim3 grid, int wpb,
                           size_t lds_bytes, Args... args) {
  if (lds_bytes > 64 * 1024)
    TORCH_CHECK(hipFuncSetAttribute(
                    reinterpret_cast<const void*>(kernel),
                    hipFuncAttributeMaxDynamicSharedMemorySize,
                    (int)lds_bytes) == hipSuccess,
                op, ": cannot raise the dynamic LDS limit to ", lds_bytes);
  hipStream_t stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(kernel, grid, dim3(WAVE * wpb), lds_bytes, stream,
                     args...);
  TORCH_CHECK(hipGetLastError() == hipSuccess, op, ": launch failed");
}

// Returns {envs per workgroup, LDS bytes per workgroup, 1 if the embedding
// table was staged in LDS}.
std::vector<int64_t> env_rollout_batch(
    std::vector<torch::Tensor> T, std::vector<double> fscal,
    std::vector<int64_t> iscal, torch::Tensor model_emb,
    std::vector<torch::Tensor> head, int64_t mode, int64_t sip_ml_cap,
    uint64_t seed, uint64_t step0, int64_t steps, torch::Tensor t0,
    torch::Tensor stop, std::vector<torch::Tensor> rows) {
  const char* op = "env_rollout_batch";
  EnvPtrs P;
  EnvDims D;
  RolloutArgs R = {};
  TORCH_CHECK(mode >= POLICY_GREEDY && mode <= ACCEPTABLE_JCT,
              op, ": unknown mode ", mode);
  TORCH_CHECK((int64_t)rows.size() == R_COUNT,
              op, ": rows takes ", (int)R_COUNT, " tensors");
  rollout_setup(op, T, fscal, iscal, mode, sip_ml_cap, seed, step0, steps, t0,
                stop, P, D, R);
  const int64_t B = D.B, A = D.A, Fg = NGF + A;
  const bool policy = mode == POLICY_GREEDY || mode == POLICY_SAMPLE;
  const int64_t TB = steps * B;
  R.u = row_ptr<float>(op, rows[R_U], torch::kFloat32, TB, "u");
  R.rewards = row_ptr<float>(op, rows[R_REWARDS], torch::kFloat32, TB,
                             "rewards");
  R.actions = (long*)row_ptr<int64_t>(op, rows[R_ACTIONS], torch::kInt64, TB,
                                      "actions");
  R.model = (long*)row_ptr<int64_t>(op, rows[R_MODEL], torch::kInt64, TB,
                                    "model");
  R.dones = row_ptr<uint8_t>(op, rows[R_DONES], torch::kUInt8, TB, "dones");
  R.ret = row_ptr<double>(op, rows[R_RET], torch::kFloat64, B, "ret");
  R.nlive = (long*)row_ptr<int64_t>(op, rows[R_NLIVE], torch::kInt64, B,
                                    "nlive");
  if (policy) {
    TORCH_CHECK(model_emb.is_cuda() && model_emb.dim() == 2 &&
                model_emb.size(1) == 16 &&
                model_emb.scalar_type() == torch::kFloat32 &&
                model_emb.is_contiguous(),
                op, ": model_emb must be a contiguous f32 "
                "[M,16] device tensor");
    R.M = (int)model_emb.size(0);
    R.model_emb = model_emb.data_ptr<float>();
    TORCH_CHECK(head.size() == 12, op, ": the policy modes take "
                "head_fwd's 12 parameter tensors");
    const int64_t want[12] = {Fg, Fg, GEMB * Fg, GEMB, H1 * EMB, H1,
                              A * H1, A, H1 * EMB, H1, H1, 1};
    for (int i = 0; i < 12; ++i) {
      TORCH_CHECK(head[i].is_cuda() &&
                  head[i].scalar_type() == torch::kFloat32 &&
                  head[i].is_contiguous() && head[i].numel() == want[i],
                  op, ": head[", i, "] must be a contiguous f32 "
                  "device tensor of ", want[i], " elements");
      R.head[i] = head[i].data_ptr<float>();
    }
    for (int k : {R_GFULL, R_LP_ALL, R_LOGP, R_VALUE})
      TORCH_CHECK(rows[k].numel() > 0, op, ": the policy modes "
                  "fill gfull, lp_all, logp and value");
    R.gfull = row_ptr<float>(op, rows[R_GFULL], torch::kFloat32, TB * Fg,
                             "gfull");
    R.lp_all = row_ptr<float>(op, rows[R_LP_ALL], torch::kFloat32, TB * A,
                              "lp_all");
    R.logp = row_ptr<float>(op, rows[R_LOGP], torch::kFloat32, TB, "logp");
    R.value = row_ptr<float>(op, rows[R_VALUE], torch::kFloat32, TB, "value");
  } else {
    // M only bounds the model id: heuristics index model_seq alone
    R.M = (int)T[T_MODEL_SEQ].numel();
  }
  if (B == 0) return {0, 0, 0};

  const auto [wpb, lds_bytes] = rollout_lds_plan(op, policy, D, R, MAX_WPB);
  const dim3 grid((unsigned)((B + wpb - 1) / wpb));
  if (policy)
    rollout_launch(op, env_rollout_kernel<true>, grid, wpb, lds_bytes, P, D, R);
  else
    rollout_launch(op, env_rollout_kernel<false>, grid, wpb, lds_bytes, P, D,
                   R);
  return {wpb, (int64_t)lds_bytes, R.emb_in_lds};
}

// The population variant: member m = b / E of `pop` [P,n] plays engine rows
// [mE, (m+1)E) with its own head (at `head_offs` inside its row) and its own
// embedding table `model_emb_pop[m]`; the Philox index is e = b % E.  Keeps
// `ret` / `nlive` [B] and, when given, the [steps,B] `actions` row.
// `max_wpb` caps the envs per workgroup (the LDS budget may lower it).
// Returns what env_rollout_batch returns.
std::vector<int64_t> env_rollout_population(
    std::vector<torch::Tensor> T, std::vector<double> fscal,
    std::vector<int64_t> iscal, torch::Tensor pop,
    torch::Tensor model_emb_pop, std::vector<int64_t> head_offs, int64_t E,
    int64_t mode, uint64_t seed, uint64_t step0, int64_t steps,
    torch::Tensor t0, torch::Tensor stop, torch::Tensor ret,
    torch::Tensor nlive, torch::Tensor actions, int64_t max_wpb) {
  const char* op = "env_rollout_population";
  EnvPtrs P;
  EnvDims D;
  RolloutArgs R = {};
  PopArgs Q = {};
  TORCH_CHECK(mode == POLICY_GREEDY || mode == POLICY_SAMPLE,
              op, ": mode must be 0 (greedy) or 1 (sample), not ", mode);
  TORCH_CHECK(max_wpb >= 1 && max_wpb <= MAX_WPB,
              op, ": max_wpb must be in [1, ", MAX_WPB, "]");
  rollout_setup(op, T, fscal, iscal, mode, -1, seed, step0, steps, t0, stop,
                P, D, R);
  const int64_t B = D.B, A = D.A, Fg = NGF + A;
  TORCH_CHECK(pop.dim() == 2 && pop.is_cuda() && pop.is_contiguous() &&
              pop.scalar_type() == torch::kFloat32,
              op, ": pop must be a contiguous f32 [P,n] device tensor");
  const int64_t NP = pop.size(0), n = pop.size(1);
  TORCH_CHECK(E >= 1 && NP >= 1 && NP <= 65535 && B == NP * E,
              op, ": needs B == P * E with 1 <= P <= 65535 and E >= 1, got "
              "B = ", B, ", P = ", NP, ", E = ", E);
  TORCH_CHECK(model_emb_pop.is_cuda() && model_emb_pop.dim() == 3 &&
              model_emb_pop.size(0) == NP && model_emb_pop.size(2) == 16 &&
              model_emb_pop.scalar_type() == torch::kFloat32 &&
              model_emb_pop.is_contiguous(),
              op, ": model_emb_pop must be a contiguous f32 [P,M,16] device "
              "tensor");
  TORCH_CHECK(head_offs.size() == 12,
              op, ": head_offs holds head_fwd's 12 row offsets");
  const int64_t want[12] = {Fg, Fg, GEMB * Fg, GEMB, H1 * EMB, H1,
                            A * H1, A, H1 * EMB, H1, H1, 1};
  for (int i = 0; i < 12; ++i) {
    TORCH_CHECK(head_offs[i] >= 0 && head_offs[i] + want[i] <= n,
                op, ": head_offs[", i, "] = ", head_offs[i], " with ",
                want[i], " elements leaves a pop row of ", n);
    Q.off[i] = (long)head_offs[i];
  }
  Q.pop = pop.data_ptr<float>();
  Q.n = (long)n;
  Q.E = (int)E;
  R.M = (int)model_emb_pop.size(1);
  R.model_emb = model_emb_pop.data_ptr<float>();
  TORCH_CHECK(ret.numel() == B && nlive.numel() == B,
              op, ": ret and nlive are [B] accumulators");
  R.ret = row_ptr<double>(op, ret, torch::kFloat64, B, "ret");
  R.nlive = (long*)row_ptr<int64_t>(op, nlive, torch::kInt64, B, "nlive");
  R.actions = (long*)row_ptr<int64_t>(op, actions, torch::kInt64, steps * B,
                                      "actions");

  const auto [wpb, lds_bytes] =
      rollout_lds_plan(op, true, D, R, (int)max_wpb);
  const dim3 grid((unsigned)((E + wpb - 1) / wpb), (unsigned)NP);
  rollout_launch(op, env_rollout_pop_kernel, grid, wpb, lds_bytes, P, D, R, Q);
  return {wpb, (int64_t)lds_bytes, R.emb_in_lds};
}
