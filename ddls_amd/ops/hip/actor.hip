// Device-side actors for the env engine on gfx950: ONE launch turns the
// engine's observation tensors (obs_gf / obs_mask / obs_model / obs_sched)
// into its `actions` tensor, for the GNN policy head (greedy or sampled) and
// for the six paper baselines of envs/actors.py.
//
// Layout (same as head_fwd_kernel in policy_head.hip): one wave per env row,
// WPB rows per block, grid-stride over rows.  Lane l of a row's wave owns
// column l of everything that is at most 64 wide: feature l of gf++mask for
// the LayerNorm, action l (l < A <= 32) for the mask / logit / log-prob.  The
// policy instantiation stages both first-layer weight matrices in LDS once
// per block; the heuristic instantiation stages nothing and never touches a
// head parameter.  No private arrays: per-action values live one per lane
// and are read across lanes with __shfl / __ballot.
//
// Done rule: a row with done != 0 (or a model id outside [0, M)) gets action
// 0 and none of its output rows are written.
//
// RNG contract: Philox4x32-10, key (seed_lo, seed_hi), counter
// (b, step_lo, step_hi, 0); u = (word0 >> 8) * 2^-24, so u is in [0, 1).
#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>
#include <vector>

#include "actor_row.h"

#define WPB 4
#define BLOCK (WAVE * WPB)

template <bool POLICY>
__global__ void __launch_bounds__(BLOCK)
actor_kernel(const float* __restrict__ obs_gf,      // [B,17]
             const float* __restrict__ obs_mask,    // [B,A]
             const int* __restrict__ obs_model,     // [B]
             const int* __restrict__ obs_sched,     // [B]
             const unsigned char* __restrict__ done,  // [B]
             const float* __restrict__ model_emb,   // [M,16]
             const float* __restrict__ ln_w, const float* __restrict__ ln_b,
             const float* __restrict__ Wg, const float* __restrict__ bg,
             const float* __restrict__ W1p, const float* __restrict__ b1p,
             const float* __restrict__ W2p, const float* __restrict__ b2p,
             const float* __restrict__ W1v, const float* __restrict__ b1v,
             const float* __restrict__ W2v, const float* __restrict__ b2v,
             const double* __restrict__ model_seq,  // [M]
             const double* __restrict__ sch_acc,    // [B,SCH]
             int* __restrict__ actions,             // [B]
             float* __restrict__ gfull,             // [B,17+A]
             float* __restrict__ lp_all,            // [B,A]
             float* __restrict__ logp,              // [B]
             float* __restrict__ value,             // [B]
             float* __restrict__ u_out,             // [B] (may be null)
             int B, int A, int M, int SCH, int mode, int sip_ml_cap,
             unsigned seed_lo, unsigned seed_hi,
             unsigned step_lo, unsigned step_hi) {
    // the heuristic instantiation keeps 1-element placeholders: no LDS
    __shared__ float w1s[POLICY ? 2 : 1][POLICY ? H1 : 1][EMB + 1];
    __shared__ float wgs[POLICY ? GEMB : 1][64 + 1];
    __shared__ float ylns[POLICY ? WPB : 1][64 + 1];
    __shared__ float embs[POLICY ? WPB : 1][EMB + 1];
    __shared__ float h1s[POLICY ? WPB : 1][POLICY ? H1 : 1];
    const int Fg = NGF + A;
    if (POLICY) {
        for (int i = threadIdx.x; i < H1 * EMB; i += BLOCK) {
            w1s[0][i / EMB][i % EMB] = W1p[i];
            w1s[1][i / EMB][i % EMB] = W1v[i];
        }
        for (int i = threadIdx.x; i < GEMB * Fg; i += BLOCK)
            wgs[i / Fg][i % Fg] = Wg[i];
        __syncthreads();
    }

    const int wave = threadIdx.x / WAVE;
    const int lane = threadIdx.x % WAVE;
    const ActorHead W = {ln_w, ln_b, bg, b1p, W2p, b2p, b1v, W2v, b2v, H1};
    for (int r = blockIdx.x * WPB + wave; r < B; r += gridDim.x * WPB) {
        const int mid = obs_model[r];
        if (done[r] != 0 || mid < 0 || mid >= M) {   // wave uniform
            if (lane == 0) actions[r] = 0;
            continue;
        }
        double seq = 0.0;
        if (!POLICY && mode == ACCEPTABLE_JCT) seq = model_seq[mid];
        const ActorRowOut out = {
            POLICY ? gfull + (long)r * Fg : nullptr,
            POLICY ? lp_all + (long)r * A : nullptr,
            POLICY ? logp + r : nullptr, POLICY ? value + r : nullptr,
            u_out != nullptr ? u_out + r : nullptr};
        const int act = actor_row<POLICY>(
            lane, (unsigned)r, obs_gf + (long)r * NGF, obs_mask + (long)r * A,
            POLICY ? model_emb + (long)mid * 16 : nullptr, obs_sched[r], seq,
            sch_acc + (long)r * SCH, SCH,
            (const float (*)[H1][EMB + 1])w1s, wgs, ylns[wave], embs[wave],
            h1s[wave], W, out, A, mode, sip_ml_cap, seed_lo, seed_hi,
            step_lo, step_hi);
        if (lane == 0) actions[r] = act;
    }
}

// ---------------------------------------------------------------------------
static const float* fptr(const torch::Tensor& t) {
    return t.numel() ? t.data_ptr<float>() : nullptr;
}

static void check_f32(const torch::Tensor& t, int64_t numel, const char* what) {
    TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kFloat32 &&
                t.is_contiguous() && t.numel() == numel,
                "actor_batch: ", what, " must be a contiguous f32 device "
                "tensor of ", numel, " elements");
}

void actor_batch(torch::Tensor obs_gf, torch::Tensor obs_mask,
                 torch::Tensor obs_model, torch::Tensor obs_sched,
                 torch::Tensor done, torch::Tensor model_emb,
                 std::vector<torch::Tensor> head, torch::Tensor model_seq,
                 torch::Tensor sch_acc, int64_t mode, int64_t sip_ml_cap,
                 uint64_t seed, uint64_t step, torch::Tensor actions,
                 torch::Tensor gfull, torch::Tensor lp_all,
                 torch::Tensor logp, torch::Tensor value, torch::Tensor u) {
    TORCH_CHECK(obs_mask.dim() == 2, "actor_batch: obs_mask must be [B,A]");
    const int64_t B = obs_mask.size(0), A = obs_mask.size(1);
    const int64_t Fg = NGF + A;
    TORCH_CHECK(mode >= POLICY_GREEDY && mode <= ACCEPTABLE_JCT,
                "actor_batch: unknown mode ", mode);
    TORCH_CHECK(A >= 1 && A <= 32 && Fg <= 64,
                "actor_batch: needs 1 <= A <= 32 and 17 + A <= 64");
    check_f32(obs_gf, B * NGF, "obs_gf");
    check_f32(obs_mask, B * A, "obs_mask");
    auto check_i32 = [&](const torch::Tensor& t, const char* what) {
        TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kInt32 &&
                    t.is_contiguous() && t.numel() == B,
                    "actor_batch: ", what, " must be a contiguous i32 [B] "
                    "device tensor");
    };
    check_i32(obs_model, "obs_model");
    check_i32(obs_sched, "obs_sched");
    check_i32(actions, "actions");
    TORCH_CHECK(done.is_cuda() && done.scalar_type() == torch::kUInt8 &&
                done.is_contiguous() && done.numel() == B,
                "actor_batch: done must be a contiguous u8 [B] device tensor");
    const bool policy = mode == POLICY_GREEDY || mode == POLICY_SAMPLE;
    int64_t M = 0, SCH = 0;
    if (policy) {
        TORCH_CHECK(model_emb.dim() == 2 && model_emb.size(1) == 16,
                    "actor_batch: model_emb must be [M,16]");
        M = model_emb.size(0);
        check_f32(model_emb, M * 16, "model_emb");
        TORCH_CHECK(head.size() == 12, "actor_batch: the policy modes take "
                    "head_fwd's 12 parameter tensors");
        const int64_t want[12] = {Fg, Fg, GEMB * Fg, GEMB, H1 * EMB, H1,
                                  A * H1, A, H1 * EMB, H1, H1, 1};
        for (int i = 0; i < 12; ++i) check_f32(head[i], want[i], "head[i]");
        check_f32(gfull, B * Fg, "gfull");
        check_f32(lp_all, B * A, "lp_all");
        check_f32(logp, B, "logp");
        check_f32(value, B, "value");
    } else {
        // M only bounds the model id: heuristics index model_seq alone
        TORCH_CHECK(model_seq.is_cuda() &&
                    model_seq.scalar_type() == torch::kFloat64 &&
                    model_seq.is_contiguous() && model_seq.dim() == 1,
                    "actor_batch: model_seq must be a contiguous f64 [M] "
                    "device tensor");
        M = model_seq.size(0);
        if (mode == ACCEPTABLE_JCT) {
            TORCH_CHECK(sch_acc.is_cuda() &&
                        sch_acc.scalar_type() == torch::kFloat64 &&
                        sch_acc.is_contiguous() && sch_acc.dim() == 2 &&
                        sch_acc.size(0) == B,
                        "actor_batch: sch_acc must be a contiguous f64 "
                        "[B,SCH] device tensor");
            SCH = sch_acc.size(1);
        }
    }
    if (u.numel()) check_f32(u, B, "u");
    if (B == 0) return;

    hipStream_t stream = at::cuda::getCurrentCUDAStream();
    int blocks = (int)((B + WPB - 1) / WPB);
    if (blocks > 2048) blocks = 2048;
    const unsigned seed_lo = (unsigned)(seed & 0xffffffffu);
    const unsigned seed_hi = (unsigned)(seed >> 32);
    const unsigned step_lo = (unsigned)(step & 0xffffffffu);
    const unsigned step_hi = (unsigned)(step >> 32);
    float* u_ptr = u.numel() ? u.data_ptr<float>() : nullptr;
    if (policy) {
        hipLaunchKernelGGL(
            actor_kernel<true>, dim3(blocks), dim3(BLOCK), 0, stream,
            obs_gf.data_ptr<float>(), obs_mask.data_ptr<float>(),
            obs_model.data_ptr<int>(), obs_sched.data_ptr<int>(),
            done.data_ptr<unsigned char>(), model_emb.data_ptr<float>(),
            fptr(head[0]), fptr(head[1]), fptr(head[2]), fptr(head[3]),
            fptr(head[4]), fptr(head[5]), fptr(head[6]), fptr(head[7]),
            fptr(head[8]), fptr(head[9]), fptr(head[10]), fptr(head[11]),
            (const double*)nullptr, (const double*)nullptr,
            actions.data_ptr<int>(), gfull.data_ptr<float>(),
            lp_all.data_ptr<float>(), logp.data_ptr<float>(),
            value.data_ptr<float>(), u_ptr,
            (int)B, (int)A, (int)M, 0, (int)mode, (int)sip_ml_cap,
            seed_lo, seed_hi, step_lo, step_hi);
    } else {
        const float* nf = nullptr;
        hipLaunchKernelGGL(
            actor_kernel<false>, dim3(blocks), dim3(BLOCK), 0, stream,
            obs_gf.data_ptr<float>(), obs_mask.data_ptr<float>(),
            obs_model.data_ptr<int>(), obs_sched.data_ptr<int>(),
            done.data_ptr<unsigned char>(), nf,
            nf, nf, nf, nf, nf, nf, nf, nf, nf, nf, nf, nf,
            model_seq.data_ptr<double>(),
            SCH ? sch_acc.data_ptr<double>() : (const double*)nullptr,
            actions.data_ptr<int>(), (float*)nullptr, (float*)nullptr,
            (float*)nullptr, (float*)nullptr, u_ptr,
            (int)B, (int)A, (int)M, (int)SCH, (int)mode, (int)sip_ml_cap,
            seed_lo, seed_hi, step_lo, step_hi);
    }
}
