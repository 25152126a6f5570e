// n-step replay ingest and fused dueling double-DQN TD loss forward +
// analytic backward for gfx950.
//
// The torch learner (rl/dqn.py) turns a rollout fragment into n-step
// transitions with a Python triple loop over T x N x n_step, keeps them as
// Python tuples, re-stacks every minibatch on the host and evaluates the loss
// as ~20 small torch ops plus their autograd chain.  Here:
//   dqn_nstep_ingest_kernel  one wave per transition: lane 0 walks the (at
//                            most n_step) rewards, the 64 lanes copy the
//                            state row and the next-state row into the ring
//   dqn_row_kernel           one wave per minibatch row, one lane per action:
//                            dueling recombination of Q(s,.), Q_online(s',.)
//                            and Q_target(s',.), double-Q argmax, clamped
//                            target, TD error, Huber term
//   dqn_reduce_kernel        one block: 256 per-thread partials in f64, added
//                            in a fixed order (no float atomics), then the
//                            means
//   dqn_loss_bwd_kernel      closed-form d loss/d logits_s, d loss/d values_s;
//                            everything on the target side is a constant, as
//                            in the torch learner's no_grad block
//
// Ring layout.  Transition k of a fragment (k = t*N + b, t-major, for
// t < T - n_step) has its state in fragment row k and its next state in row
// k + steps*N, and goes to slot (written + k) % C.  A fragment that yields
// K > C transitions would send two waves to one slot, so only its last C
// (k >= K - C) are written: that is what a list that overwrites its oldest
// entry holds afterwards.  A transition whose return was cut by a done has
// has_next = 0 and carries a copy of its own state as next state, so every
// ring row is a valid network input.
//
// Bit contract (ingest).  ret and disc equal
// rl/dqn.py::nstep_transitions_reference bit for bit: R is an f32, the
// running discount an f64 that is rounded to f32 for each multiply, each
// f32 multiply and add is rounded singly (no FMA contraction), and disc is
// the f64 rounded once.
//
// Precision (loss).  A row's arithmetic is carried in f64 and rounded to f32
// once per output, so the loss, the stats and the gradients are the f64
// values of the same f32 inputs to half an ulp; the f32 torch chain rounds
// at every op.
#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>
#include <cmath>
#include <vector>

#define WAVE 64
#define WAVES 4
#define BLOCK (WAVE * WAVES)

// butterfly sum: every lane ends with the same total, added in a fixed order
__device__ __forceinline__ double dqn_wave_sum_all(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        v += __shfl_xor(v, off, WAVE);
    return v;
}

__device__ __forceinline__ double dqn_wave_sum_d(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        v += __shfl_down(v, off, WAVE);
    return v;   // valid on lane 0
}

// butterfly argmax: the largest value, on an exact tie the lowest index;
// every lane ends with the same (val, idx)
__device__ __forceinline__ void dqn_wave_argmax(double& val, int& idx) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_xor(val, off, WAVE);
        const int oi = __shfl_xor(idx, off, WAVE);
        if (ov > val || (ov == val && oi < idx)) {
            val = ov;
            idx = oi;
        }
    }
}

// Q of this lane's action, as DQNTrainer._q_values has it: valid lanes get
// (v + logit) - mean of the valid logits, masked lanes (logit <= -1e30, i.e.
// finfo.min) keep the raw logit.  Called by all 64 lanes.
__device__ __forceinline__ double dqn_q_lane(float x, float v, bool in_row,
                                             bool dueling, int& nvalid) {
    const bool valid = in_row && x > -1e30f;
    nvalid = __popcll(__ballot(valid));
    if (!dueling) return (double)x;
    const double s = dqn_wave_sum_all(valid ? (double)x : 0.0);
    const double mean_adv = s / (double)(nvalid > 1 ? nvalid : 1);
    return valid ? ((double)v + (double)x) - mean_adv : (double)x;
}

__global__ void __launch_bounds__(BLOCK)
dqn_nstep_ingest_kernel(const float* __restrict__ gfull,     // [T*N, F]
                        const long* __restrict__ model_ids,  // [T*N]
                        const long* __restrict__ actions,    // [T*N]
                        const float* __restrict__ rewards,   // [T*N]
                        const float* __restrict__ dones,     // [T*N]
                        float* __restrict__ s_gfull,         // [C, F]
                        long* __restrict__ s_model,          // [C]
                        long* __restrict__ action,           // [C]
                        float* __restrict__ ret,             // [C]
                        float* __restrict__ disc,            // [C]
                        float* __restrict__ has_next,        // [C]
                        float* __restrict__ n_gfull,         // [C, F]
                        long* __restrict__ n_model,          // [C]
                        long k0, long K, int N, int F, long C, long written,
                        int n_step, double gamma) {
#pragma clang fp contract(off)
    const int wave = threadIdx.x / WAVE;
    const int lane = threadIdx.x % WAVE;
    for (long k = k0 + (long)blockIdx.x * WAVES + wave; k < K;
         k += (long)gridDim.x * WAVES) {
        float R = 0.0f;
        double discount = 1.0;
        int steps = 0, cut = 0;
        if (lane == 0) {
            for (int i = 0; i < n_step; ++i) {
                const long row = k + (long)i * N;
                const float term = (float)discount * rewards[row];
                R = R + term;
                discount = discount * gamma;
                steps = i + 1;
                if (dones[row] != 0.0f) {
                    cut = 1;
                    break;
                }
            }
        }
        steps = __shfl(steps, 0, WAVE);
        cut = __shfl(cut, 0, WAVE);
        const long slot = (written + k) % C;
        const long nrow = cut ? k : k + (long)steps * N;
        for (int j = lane; j < F; j += WAVE) {
            s_gfull[slot * F + j] = gfull[k * F + j];
            n_gfull[slot * F + j] = gfull[nrow * F + j];
        }
        if (lane == 0) {
            s_model[slot] = model_ids[k];
            n_model[slot] = model_ids[nrow];
            action[slot] = actions[k];
            ret[slot] = R;
            disc[slot] = (float)discount;
            has_next[slot] = cut ? 0.0f : 1.0f;
        }
    }
}

// one wave per row (A <= 64).  rows_out[b] = {huber, q_a, |td|, target};
// dq_out[b] = clamp(td, -1, 1), the Huber derivative.  With importance
// weights (prioritized replay; `weights` is null otherwise) the Huber term
// and dq are multiplied by w[b], so the reduction gives mean(w * huber) and
// the backward kernel is the same; q_a, |td| and target stay unweighted, and
// |td| also goes to td_abs_out, the new priorities' input.
__global__ void __launch_bounds__(BLOCK)
dqn_row_kernel(const float* __restrict__ logits_s,    // [B, A] online, s
               const float* __restrict__ values_s,    // [B]
               const float* __restrict__ logits_no,   // [B, A] online, s'
               const float* __restrict__ values_no,   // [B]
               const float* __restrict__ logits_nt,   // [B, A] target, s'
               const float* __restrict__ values_nt,   // [B]
               const long* __restrict__ actions,      // [B]
               const float* __restrict__ ret,         // [B]
               const float* __restrict__ disc,        // [B]
               const float* __restrict__ has_next,    // [B]
               const float* __restrict__ weights,     // [B] or null
               double* __restrict__ rows_out,         // [B, 4]
               double* __restrict__ dq_out,           // [B]
               double* __restrict__ td_abs_out,       // [B] or null
               int B, int A, double v_min, double v_max, bool dueling,
               bool double_q) {
    const int wave = threadIdx.x / WAVE;
    const int lane = threadIdx.x % WAVE;
    const bool in_row = lane < A;
    for (int b = blockIdx.x * WAVES + wave; b < B; b += gridDim.x * WAVES) {
        const long at = (long)b * A + lane;
        int nv;
        const float xs = in_row ? logits_s[at] : 0.0f;
        const double qs = dqn_q_lane(xs, values_s[b], in_row, dueling, nv);
        const int a = (int)actions[b];
        const double q_a = __shfl(qs, a, WAVE);

        const float xt = in_row ? logits_nt[at] : 0.0f;
        const double qt = dqn_q_lane(xt, values_nt[b], in_row, dueling, nv);
        double val;
        if (double_q) {
            const float xo = in_row ? logits_no[at] : 0.0f;
            const double qo = dqn_q_lane(xo, values_no[b], in_row, dueling,
                                         nv);
            double best = in_row ? qo : -HUGE_VAL;
            int a_star = lane;
            dqn_wave_argmax(best, a_star);
            val = __shfl(qt, a_star, WAVE);
        } else {
            val = in_row ? qt : -HUGE_VAL;
            int at_max = lane;
            dqn_wave_argmax(val, at_max);
        }
        // a select: a cut transition's next state may be all finfo.min
        const double boot = (has_next[b] != 0.0f) ? val : 0.0;
        double target = (double)ret[b] + (double)disc[b] * boot;
        target = fmin(fmax(target, v_min), v_max);
        const double td = q_a - target;
        const double ad = fabs(td);
        const double huber = (ad < 1.0) ? 0.5 * td * td : ad - 0.5;
        if (lane == 0) {
            const double dq = fmin(fmax(td, -1.0), 1.0);
            if (weights != nullptr) {
                const double w = (double)weights[b];
                rows_out[(long)b * 4 + 0] = w * huber;
                dq_out[b] = w * dq;
            } else {
                rows_out[(long)b * 4 + 0] = huber;
                dq_out[b] = dq;
            }
            rows_out[(long)b * 4 + 1] = q_a;
            rows_out[(long)b * 4 + 2] = ad;
            rows_out[(long)b * 4 + 3] = target;
            if (td_abs_out != nullptr) td_abs_out[b] = ad;
        }
    }
}

// One block.  Thread j sums rows j, j+BLOCK, ... (a fixed 256 partials), the
// partials are added by a fixed shuffle tree and then in wave order, so two
// calls on the same inputs give the same bits.
// stats = {total_loss, q_mean, td_abs_mean, target_mean}
__global__ void __launch_bounds__(BLOCK)
dqn_reduce_kernel(const double* __restrict__ rows,   // [B, 4]
                  float* __restrict__ loss_out,      // [1]
                  float* __restrict__ stats_out,     // [4]
                  int B) {
    __shared__ double part[WAVES][4];
    const int wave = threadIdx.x / WAVE;
    const int lane = threadIdx.x % WAVE;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < B; i += BLOCK)
        for (int q = 0; q < 4; ++q) s[q] += rows[(long)i * 4 + q];
    for (int q = 0; q < 4; ++q) s[q] = dqn_wave_sum_d(s[q]);
    if (lane == 0)
        for (int q = 0; q < 4; ++q) part[wave][q] = s[q];
    __syncthreads();
    if (threadIdx.x == 0) {
        double t[4] = {0.0, 0.0, 0.0, 0.0};
        for (int w = 0; w < WAVES; ++w)
            for (int q = 0; q < 4; ++q) t[q] += part[w][q];
        for (int q = 0; q < 4; ++q) stats_out[q] = (float)(t[q] / B);
        loss_out[0] = (float)(t[0] / B);
    }
}

// one wave per row.  d loss/d q_a = g * dq / B; with dueling
// d q_a/d logit_j = [j == a] - 1/nvalid on valid lanes and d q_a/d value = 1,
// without it d q_a/d logit_j = [j == a] and the value takes no gradient.
__global__ void __launch_bounds__(BLOCK)
dqn_loss_bwd_kernel(const float* __restrict__ logits_s,   // [B, A]
                    const long* __restrict__ actions,     // [B]
                    const double* __restrict__ dq,        // [B]
                    const float* __restrict__ gl,         // [1] upstream
                    float* __restrict__ glogits,          // [B, A]
                    float* __restrict__ gvalues,          // [B]
                    int B, int A, bool dueling) {
    const int wave = threadIdx.x / WAVE;
    const int lane = threadIdx.x % WAVE;
    const bool in_row = lane < A;
    const double g = (double)gl[0];
    for (int b = blockIdx.x * WAVES + wave; b < B; b += gridDim.x * WAVES) {
        const long at = (long)b * A + lane;
        const float x = in_row ? logits_s[at] : 0.0f;
        const bool valid = in_row && x > -1e30f;
        const int nvalid = __popcll(__ballot(valid));
        const int a = (int)actions[b];
        const double c = g * dq[b] / (double)B;
        const double delta = (lane == a) ? 1.0 : 0.0;
        if (in_row) {
            float gj;
            if (dueling)
                gj = valid ? (float)(c * (delta - 1.0 / (double)nvalid))
                           : 0.0f;
            else
                gj = (lane == a) ? (float)c : 0.0f;
            glogits[at] = gj;
        }
        if (lane == 0) gvalues[b] = dueling ? (float)c : 0.0f;
    }
}

static void check_f32(const torch::Tensor& t, int64_t numel,
                      const char* name) {
    TORCH_CHECK(t.is_cuda() && t.dtype() == torch::kFloat32
                && t.is_contiguous() && t.numel() == numel,
                name, ": expected a contiguous f32 CUDA tensor of ", numel,
                " elements");
}

static void check_i64(const torch::Tensor& t, int64_t numel,
                      const char* name) {
    TORCH_CHECK(t.is_cuda() && t.dtype() == torch::kInt64
                && t.is_contiguous() && t.numel() == numel,
                name, ": expected a contiguous int64 CUDA tensor of ", numel,
                " elements");
}

static void check_f64(const torch::Tensor& t, int64_t numel,
                      const char* name) {
    TORCH_CHECK(t.is_cuda() && t.dtype() == torch::kFloat64
                && t.is_contiguous() && t.numel() == numel,
                name, ": expected a contiguous f64 CUDA tensor of ", numel,
                " elements");
}

static int row_blocks(int64_t R) {
    int64_t blocks = (R + WAVES - 1) / WAVES;
    return (int)(blocks > 1024 ? 1024 : blocks);
}

// ring = {s_gfull, s_model, action, ret, disc, has_next, n_gfull, n_model};
// returns the number of transitions the fragment yields, (T - n_step) * N or
// 0, which the caller adds to `written` (also when fewer were stored)
int64_t dqn_nstep_ingest(
    torch::Tensor gfull, torch::Tensor model_ids, torch::Tensor actions,
    torch::Tensor rewards, torch::Tensor dones,
    std::vector<torch::Tensor> ring, int64_t T, int64_t N, int64_t capacity,
    int64_t written, int64_t n_step, double gamma) {
    TORCH_CHECK(gfull.dim() == 2, "dqn_nstep_ingest: gfull must be [T*N, F]");
    TORCH_CHECK(T >= 1 && N >= 1 && T * N < (1LL << 31),
                "dqn_nstep_ingest: T*N out of range");
    TORCH_CHECK(n_step >= 1, "dqn_nstep_ingest: n_step must be >= 1");
    TORCH_CHECK(capacity >= 1 && written >= 0,
                "dqn_nstep_ingest: capacity / written out of range");
    TORCH_CHECK(ring.size() == 8, "dqn_nstep_ingest: ring must hold 8 tensors");
    const int64_t R = T * N, F = gfull.size(1), C = capacity;
    TORCH_CHECK(F >= 1 && F < (1LL << 31),
                "dqn_nstep_ingest: feature width out of range");
    check_f32(gfull, R * F, "dqn_nstep_ingest gfull");
    check_i64(model_ids, R, "dqn_nstep_ingest model_ids");
    check_i64(actions, R, "dqn_nstep_ingest actions");
    check_f32(rewards, R, "dqn_nstep_ingest rewards");
    check_f32(dones, R, "dqn_nstep_ingest dones");
    check_f32(ring[0], C * F, "dqn_nstep_ingest ring s_gfull");
    check_i64(ring[1], C, "dqn_nstep_ingest ring s_model");
    check_i64(ring[2], C, "dqn_nstep_ingest ring action");
    check_f32(ring[3], C, "dqn_nstep_ingest ring ret");
    check_f32(ring[4], C, "dqn_nstep_ingest ring disc");
    check_f32(ring[5], C, "dqn_nstep_ingest ring has_next");
    check_f32(ring[6], C * F, "dqn_nstep_ingest ring n_gfull");
    check_i64(ring[7], C, "dqn_nstep_ingest ring n_model");
    const int64_t K = (T - n_step) * N;
    if (K <= 0) return 0;
    // rows read: k + i*N with k < K, i <= n_step, so at most T*N - 1
    const int64_t k0 = K > C ? K - C : 0;
    hipStream_t stream = at::cuda::getCurrentCUDAStream();
    hipLaunchKernelGGL(dqn_nstep_ingest_kernel, dim3(row_blocks(K - k0)),
                       dim3(BLOCK), 0, stream, gfull.data_ptr<float>(),
                       model_ids.data_ptr<long>(), actions.data_ptr<long>(),
                       rewards.data_ptr<float>(), dones.data_ptr<float>(),
                       ring[0].data_ptr<float>(), ring[1].data_ptr<long>(),
                       ring[2].data_ptr<long>(), ring[3].data_ptr<float>(),
                       ring[4].data_ptr<float>(), ring[5].data_ptr<float>(),
                       ring[6].data_ptr<float>(), ring[7].data_ptr<long>(),
                       (long)k0, (long)K, (int)N, (int)F, (long)C,
                       (long)written, (int)n_step, gamma);
    return K;
}

// weights: null for the plain loss.  Returns {loss[1], stats[4], dq[B] (f64)}
// and, with weights, td_abs[B] (f64)
static std::vector<torch::Tensor> dqn_loss_fwd_impl(
    const char* name, torch::Tensor logits_s, torch::Tensor values_s,
    torch::Tensor logits_no, torch::Tensor values_no, torch::Tensor logits_nt,
    torch::Tensor values_nt, torch::Tensor actions, torch::Tensor ret,
    torch::Tensor disc, torch::Tensor has_next, double v_min, double v_max,
    bool dueling, bool double_q, const torch::Tensor* weights) {
    TORCH_CHECK(logits_s.dim() == 2, name, ": logits_s must be [B, A]");
    const int64_t B = logits_s.size(0), A = logits_s.size(1);
    TORCH_CHECK(B >= 1 && B < (1LL << 31), name, ": B out of range");
    TORCH_CHECK(A >= 1 && A <= 64, name,
                " needs A <= 64 (one wave per row)");
    check_f32(logits_s, B * A, "dqn_loss_fwd logits_s");
    check_f32(values_s, B, "dqn_loss_fwd values_s");
    check_f32(logits_no, B * A, "dqn_loss_fwd logits_no");
    check_f32(values_no, B, "dqn_loss_fwd values_no");
    check_f32(logits_nt, B * A, "dqn_loss_fwd logits_nt");
    check_f32(values_nt, B, "dqn_loss_fwd values_nt");
    check_i64(actions, B, "dqn_loss_fwd actions");
    check_f32(ret, B, "dqn_loss_fwd ret");
    check_f32(disc, B, "dqn_loss_fwd disc");
    check_f32(has_next, B, "dqn_loss_fwd has_next");
    if (weights != nullptr)
        check_f32(*weights, B, "dqn_loss_fwd_weighted weights");
    auto opt = logits_s.options();
    auto opt64 = opt.dtype(torch::kFloat64);
    auto rows = torch::empty({B, 4}, opt64);
    auto dq = torch::empty({B}, opt64);
    auto loss = torch::empty({1}, opt);
    auto stats = torch::empty({4}, opt);
    torch::Tensor td_abs;
    if (weights != nullptr) td_abs = torch::empty({B}, opt64);
    hipStream_t stream = at::cuda::getCurrentCUDAStream();
    hipLaunchKernelGGL(dqn_row_kernel, dim3(row_blocks(B)), dim3(BLOCK), 0,
                       stream, logits_s.data_ptr<float>(),
                       values_s.data_ptr<float>(),
                       logits_no.data_ptr<float>(),
                       values_no.data_ptr<float>(),
                       logits_nt.data_ptr<float>(),
                       values_nt.data_ptr<float>(), actions.data_ptr<long>(),
                       ret.data_ptr<float>(), disc.data_ptr<float>(),
                       has_next.data_ptr<float>(),
                       weights != nullptr ? weights->data_ptr<float>()
                                          : (const float*)nullptr,
                       rows.data_ptr<double>(), dq.data_ptr<double>(),
                       weights != nullptr ? td_abs.data_ptr<double>()
                                          : (double*)nullptr,
                       (int)B, (int)A, v_min, v_max, dueling, double_q);
    hipLaunchKernelGGL(dqn_reduce_kernel, dim3(1), dim3(BLOCK), 0, stream,
                       rows.data_ptr<double>(), loss.data_ptr<float>(),
                       stats.data_ptr<float>(), (int)B);
    if (weights != nullptr) return {loss, stats, dq, td_abs};
    return {loss, stats, dq};
}

// returns {loss[1], stats[4], dq[B] (f64)}; dq (with logits_s and actions)
// is what dqn_loss_bwd needs
std::vector<torch::Tensor> dqn_loss_fwd(
    torch::Tensor logits_s, torch::Tensor values_s, torch::Tensor logits_no,
    torch::Tensor values_no, torch::Tensor logits_nt, torch::Tensor values_nt,
    torch::Tensor actions, torch::Tensor ret, torch::Tensor disc,
    torch::Tensor has_next, double v_min, double v_max, bool dueling,
    bool double_q) {
    return dqn_loss_fwd_impl("dqn_loss_fwd", logits_s, values_s, logits_no,
                             values_no, logits_nt, values_nt, actions, ret,
                             disc, has_next, v_min, v_max, dueling, double_q,
                             nullptr);
}

// the importance-weighted loss of prioritized replay: loss = mean(w * huber),
// dq = w * clamp(td, -1, 1).  Returns {loss[1], stats[4], dq[B], td_abs[B]}
// (the last two f64); td_abs is the unweighted |td| that per_update reads
std::vector<torch::Tensor> dqn_loss_fwd_weighted(
    torch::Tensor logits_s, torch::Tensor values_s, torch::Tensor logits_no,
    torch::Tensor values_no, torch::Tensor logits_nt, torch::Tensor values_nt,
    torch::Tensor actions, torch::Tensor ret, torch::Tensor disc,
    torch::Tensor has_next, double v_min, double v_max, bool dueling,
    bool double_q, torch::Tensor weights) {
    return dqn_loss_fwd_impl("dqn_loss_fwd_weighted", logits_s, values_s,
                             logits_no, values_no, logits_nt, values_nt,
                             actions, ret, disc, has_next, v_min, v_max,
                             dueling, double_q, &weights);
}

std::vector<torch::Tensor> dqn_loss_bwd(
    torch::Tensor logits_s, torch::Tensor actions, torch::Tensor dq,
    torch::Tensor gl, bool dueling) {
    TORCH_CHECK(logits_s.dim() == 2, "dqn_loss_bwd: logits_s must be [B, A]");
    const int64_t B = logits_s.size(0), A = logits_s.size(1);
    TORCH_CHECK(B >= 1 && B < (1LL << 31), "dqn_loss_bwd: B out of range");
    TORCH_CHECK(A >= 1 && A <= 64, "dqn_loss_bwd needs A <= 64");
    check_f32(logits_s, B * A, "dqn_loss_bwd logits_s");
    check_i64(actions, B, "dqn_loss_bwd actions");
    check_f64(dq, B, "dqn_loss_bwd dq");
    check_f32(gl, 1, "dqn_loss_bwd gl");
    auto glogits = torch::empty({B, A}, logits_s.options());
    auto gvalues = torch::empty({B}, logits_s.options());
    hipStream_t stream = at::cuda::getCurrentCUDAStream();
    hipLaunchKernelGGL(dqn_loss_bwd_kernel, dim3(row_blocks(B)), dim3(BLOCK),
                       0, stream, logits_s.data_ptr<float>(),
                       actions.data_ptr<long>(), dq.data_ptr<double>(),
                       gl.data_ptr<float>(), glogits.data_ptr<float>(),
                       gvalues.data_ptr<float>(), (int)B, (int)A, dueling);
    return {glogits, gvalues};
}
