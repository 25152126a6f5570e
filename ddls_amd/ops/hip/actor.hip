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

#define WAVE 64
#define WPB 4
#define BLOCK (WAVE * WPB)
#define LN_EPS 1e-5f
#define EMB 24
#define H1 256
#define GEMB 8
#define NGF 17
#define MASK_MIN (-3.4028234663852886e+38f)

enum ActorMode {
    POLICY_GREEDY = 0, POLICY_SAMPLE = 1, RANDOM = 2, NO_PARALLELISM = 3,
    MIN_PARALLELISM = 4, MAX_PARALLELISM = 5, SIP_ML = 6, ACCEPTABLE_JCT = 7
};

__device__ __forceinline__ float awave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        v += __shfl_down(v, off, WAVE);
    return __shfl(v, 0, WAVE);
}

__device__ __forceinline__ float awave_max(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        v = fmaxf(v, __shfl_xor(v, off, WAVE));
    return v;
}

// first output word of Philox4x32-10
__device__ __forceinline__ unsigned philox_word0(unsigned c0, unsigned c1,
                                                 unsigned c2, unsigned c3,
                                                 unsigned k0, unsigned k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0);
        const unsigned lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2);
        const unsigned lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c0;
}

__device__ __forceinline__ int lowest_bit(unsigned v) { return __ffs(v) - 1; }
__device__ __forceinline__ int highest_bit(unsigned v) { return 31 - __clz(v); }

// the baselines of envs/actors.py on the bit set of valid actions (wave
// uniform: every lane computes the same answer)
__device__ __forceinline__ int heuristic_action(
        int mode, unsigned vb, int A, float u, int sip_ml_cap,
        double seq, double acc) {
    const int n = __popc(vb);
    // len(valid) <= 1: the count-based actors answer 0, the others valid[0]
    if (n == 0 || mode == NO_PARALLELISM || mode == MIN_PARALLELISM) {
        if (n <= 1) return 0;
    }
    if (n == 1) return lowest_bit(vb);
    const int last = highest_bit(vb);
    switch (mode) {
    case NO_PARALLELISM:
        return 1;
    case MIN_PARALLELISM:
        return (n > 2) ? 2 : 1;
    case MAX_PARALLELISM:
        return last;
    case SIP_ML:
        return (sip_ml_cap >= 0) ? min(sip_ml_cap, last) : last;
    case ACCEPTABLE_JCT: {
        const double want = ceil(seq / acc);
        if (!(want <= (double)A)) return last;   // also NaN / +inf
        const int w = (want > 0.0) ? (int)want : 0;
        const unsigned ge = (w >= 32) ? 0u : (vb & ~((1u << w) - 1u));
        return ge ? lowest_bit(ge) : last;
    }
    case RANDOM: {
        // valid[1:][min(n-2, floor(u*(n-1)))]
        int idx = (int)floorf(u * (float)(n - 1));
        idx = min(idx, n - 2);
        unsigned rest = vb & (vb - 1u);          // drop valid[0]
        for (int i = 0; i < idx; ++i) rest &= rest - 1u;
        return lowest_bit(rest);
    }
    default:
        return 0;
    }
}

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
    for (int r = blockIdx.x * WPB + wave; r < B; r += gridDim.x * WPB) {
        const int mid = obs_model[r];
        if (done[r] != 0 || mid < 0 || mid >= M) {   // wave uniform
            if (lane == 0) actions[r] = 0;
            continue;
        }
        const float mk = (lane < A) ? obs_mask[(long)r * A + lane] : 0.0f;
        const unsigned vb = (unsigned)__ballot(lane < A && mk > 0.0f);
        const unsigned x = philox_word0((unsigned)r, step_lo, step_hi, 0u,
                                        seed_lo, seed_hi);
        const float u = (float)(x >> 8) * 5.9604644775390625e-08f;  // 2^-24

        if constexpr (!POLICY) {
            double seq = 0.0, acc = 0.0;
            if (mode == ACCEPTABLE_JCT) {
                const int k = obs_sched[r];
                seq = model_seq[mid];
                // an out-of-range schedule slot reads as "never reached"
                acc = (k >= 0 && k < SCH) ? sch_acc[(long)r * SCH + k] : 0.0;
            }
            const int a = heuristic_action(mode, vb, A, u, sip_ml_cap, seq,
                                           acc);
            if (lane == 0) {
                actions[r] = a;
                if (mode == RANDOM && u_out != nullptr) u_out[r] = u;
            }
            continue;
        }
        if constexpr (POLICY) {
        // ---- policy head: LN(gf ++ mask) -> graph Linear -> concat ----
        float v = 0.0f;
        if (lane < NGF) v = obs_gf[(long)r * NGF + lane];
        else if (lane < Fg) v = obs_mask[(long)r * A + (lane - NGF)];
        if (lane < Fg) gfull[(long)r * Fg + lane] = v;
        const float mean = awave_sum(v) / Fg;
        const float d = (lane < Fg) ? v - mean : 0.0f;
        const float var = awave_sum(d * d) / Fg;
        const float inv_sigma = rsqrtf(var + LN_EPS);
        if (lane < Fg)
            ylns[wave][lane] = d * inv_sigma * ln_w[lane] + ln_b[lane];
        __builtin_amdgcn_wave_barrier();
        if (lane < GEMB) {
            float ge = bg[lane];
            for (int k = 0; k < Fg; ++k)
                ge = fmaf(wgs[lane][k], ylns[wave][k], ge);
            embs[wave][16 + lane] = ge;
        }
        if (lane < 16) embs[wave][lane] = model_emb[(long)mid * 16 + lane];
        __builtin_amdgcn_wave_barrier();

        // policy branch
#pragma unroll
        for (int i = 0; i < H1 / WAVE; ++i) {
            const int j = lane + WAVE * i;
            float a1 = b1p[j];
#pragma unroll
            for (int k = 0; k < EMB; ++k)
                a1 = fmaf(w1s[0][j][k], embs[wave][k], a1);
            h1s[wave][j] = fmaxf(a1, 0.0f);
        }
        __builtin_amdgcn_wave_barrier();
        float lg = -INFINITY;
        if (lane < A) {
            lg = b2p[lane];
            const float* w2row = W2p + (long)lane * H1;
            for (int j = 0; j < H1; ++j)
                lg = fmaf(w2row[j], h1s[wave][j], lg);
            // torch: logits + clamp(log(mask), min=float32_min)
            lg += (mk > 0.0f) ? logf(mk) : MASK_MIN;
        }
        __builtin_amdgcn_wave_barrier();
        // value branch
#pragma unroll
        for (int i = 0; i < H1 / WAVE; ++i) {
            const int j = lane + WAVE * i;
            float a1 = b1v[j];
#pragma unroll
            for (int k = 0; k < EMB; ++k)
                a1 = fmaf(w1s[1][j][k], embs[wave][k], a1);
            h1s[wave][j] = fmaxf(a1, 0.0f);
        }
        __builtin_amdgcn_wave_barrier();
        float vp = 0.0f;
#pragma unroll
        for (int i = 0; i < H1 / WAVE; ++i) {
            const int j = lane + WAVE * i;
            vp = fmaf(W2v[j], h1s[wave][j], vp);
        }
        vp = awave_sum(vp) + b2v[0];

        // max-subtracted log-softmax over the A lanes
        const float mx = awave_max(lg);
        const float ex = (lane < A) ? expf(lg - mx) : 0.0f;
        const float lse = logf(awave_sum(ex));
        const float lp = (lane < A) ? lg - mx - lse : -INFINITY;
        if (lane < A) lp_all[(long)r * A + lane] = lp;

        int act;
        if (mode == POLICY_GREEDY) {
            // argmax of the masked logits, ties to the lowest index
            const unsigned long long top = __ballot(lane < A && lg == mx);
            act = __ffsll((long long)top) - 1;
            if (act < 0) act = 0;                // all-NaN logits
        } else {
            // inverse CDF: first valid a with u < cum, else the last valid
            const float p = (lane < A) ? expf(lp) : 0.0f;
            float cum = 0.0f;
            act = -1;
            for (int a = 0; a < A; ++a) {
                cum += __shfl(p, a, WAVE);
                if (act < 0 && ((vb >> a) & 1u) && u < cum) act = a;
            }
            if (act < 0) act = vb ? highest_bit(vb) : 0;
        }
        const float lpa = __shfl(lp, act, WAVE);
        if (lane == 0) {
            actions[r] = act;
            logp[r] = lpa;
            value[r] = vp;
            if (u_out != nullptr) u_out[r] = u;
        }
        __builtin_amdgcn_wave_barrier();
        }  // POLICY
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
