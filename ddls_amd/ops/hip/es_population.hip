// Population evaluation for Evolution Strategies on gfx950: the three
// launches of a generation that are not the env step.
//
//   es_perturb        eps [K,n] and pop [2K,n] from theta [n] in one launch
//   actor_population  actor_kernel<true>'s row contract (actor.hip) with the
//                     head weights and the embedding table of row b taken
//                     from member b / E
//   es_update         theta' = (theta + scale * sum_k w[k] eps[k]) - decay theta
//
// Conventions: K perturbation pairs, P = 2K members, member m = 2k + s with
// s = 0 for +eps_k and s = 1 for -eps_k, E envs per member, engine row
// b = m * E + e, n = numel(theta) (no alignment assumed: scalar accesses).
//
// Noise contract: Philox4x32-10, key (seed_lo, seed_hi), counter
// (j, k, gen_lo, gen_hi) with j = i / 4.  Words (w0, w1) give elements 4j and
// 4j+1, (w2, w3) give 4j+2 and 4j+3, by Box-Muller:
//   u1 = ((w >> 8) + 1) * 2^-24  in (0, 1],  u2 = (w' >> 8) * 2^-24 in [0, 1)
//   r = sqrtf(-2 logf(u1)),  a = 6.2831855f * u2
//   z_even = r cosf(a),  z_odd = r sinf(a)
//
// Sampling contract of actor_population: counter (e, step_lo, step_hi, 0)
// with e = b % E, so every member draws the uniforms actor_kernel draws for a
// batch of E rows.
//
// Every rounding below is written out: contraction is off and a fused
// multiply-add appears only as fmaf.
#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>
#include <vector>

#pragma clang fp contract(off)

#define WAVE 64
#define WPB 4
#define BLOCK (WAVE * WPB)
#define LN_EPS 1e-5f
#define EMB 24
#define H1 256
#define GEMB 8
#define NGF 17
#define MASK_MIN (-3.4028234663852886e+38f)
#define TWO_M24 5.9604644775390625e-08f
#define TWO_PI_F 6.2831855f

enum { POP_GREEDY = 0, POP_SAMPLE = 1 };

struct HeadOffs { long o[12]; };

__device__ __forceinline__ float pwave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        v += __shfl_down(v, off, WAVE);
    return __shfl(v, 0, WAVE);
}

// pwave_sum(d * d) as actor.hip's build evaluates it: the compiler contracts
// the first step of the reduction into fma(d, d, shfl(d * d)); with
// contraction off here that step is spelled out, so both kernels round alike
__device__ __forceinline__ float pwave_sum_sq(float d) {
    const float dd = d * d;
    float v = fmaf(d, d, __shfl_down(dd, 32, WAVE));
#pragma unroll
    for (int off = 16; off > 0; off >>= 1)
        v += __shfl_down(v, off, WAVE);
    return __shfl(v, 0, WAVE);
}

__device__ __forceinline__ float pwave_max(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        v = fmaxf(v, __shfl_xor(v, off, WAVE));
    return v;
}

// Philox4x32-10: the rounds of actor.hip's philox_word0, all four words
__device__ __forceinline__ uint4 philox4(unsigned c0, unsigned c1,
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
    return make_uint4(c0, c1, c2, c3);
}

__device__ __forceinline__ void box_muller(unsigned wa, unsigned wb,
                                           float* z_even, float* z_odd) {
    const float u1 = (float)((wa >> 8) + 1u) * TWO_M24;
    const float u2 = (float)(wb >> 8) * TWO_M24;
    const float r = sqrtf(-2.0f * logf(u1));
    const float a = TWO_PI_F * u2;
    float s, c;
    sincosf(a, &s, &c);
    *z_even = r * c;
    *z_odd = r * s;
}

// ---------------------------------------------------------------------------
// es_perturb: thread (j, k) owns elements 4j .. 4j+3 of pair k
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(BLOCK)
es_perturb_kernel(const float* __restrict__ theta,   // [n]
                  float* __restrict__ eps,           // [K,n]
                  float* __restrict__ pop,           // [2K,n]
                  long n, float sigma,
                  unsigned seed_lo, unsigned seed_hi,
                  unsigned gen_lo, unsigned gen_hi) {
    const long nq = (n + 3) / 4;
    const long j = (long)blockIdx.x * BLOCK + threadIdx.x;
    const int k = blockIdx.y;
    if (j >= nq) return;
    const uint4 w = philox4((unsigned)j, (unsigned)k, gen_lo, gen_hi,
                            seed_lo, seed_hi);
    float z[4];
    box_muller(w.x, w.y, &z[0], &z[1]);
    box_muller(w.z, w.w, &z[2], &z[3]);
    float* eps_k = eps + (long)k * n;
    float* pop_p = pop + (long)(2 * k) * n;
    float* pop_m = pop_p + n;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const long i = 4 * j + q;
        if (i < n) {
            const float t = sigma * z[q];
            const float th = theta[i];
            eps_k[i] = z[q];
            pop_p[i] = th + t;
            pop_m[i] = th - t;
        }
    }
}

// ---------------------------------------------------------------------------
// es_update: thread i owns element i
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(BLOCK)
es_update_kernel(const float* __restrict__ theta,   // [n]
                 const float* __restrict__ eps,     // [K,n]
                 const float* __restrict__ w,       // [K]
                 float* __restrict__ out,           // [n]
                 long n, int K, float scale, float decay) {
    const long i = (long)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    float acc = 0.0f;
    for (int k = 0; k < K; ++k) {
        const float prod = w[k] * eps[(long)k * n + i];
        acc = acc + prod;
    }
    const float th = theta[i];
    const float step = scale * acc;
    const float shrink = decay * th;
    out[i] = (th + step) - shrink;
}

// ---------------------------------------------------------------------------
// actor_population: block (c, m) stages member m's first-layer matrices once;
// its WPB waves serve rows e = c * WPB + wave of that member.  Lane layout,
// fmaf chains, done rule and sampling rule are actor_kernel<true>'s.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(BLOCK)
actor_population_kernel(const float* __restrict__ obs_gf,      // [B,17]
                        const float* __restrict__ obs_mask,    // [B,A]
                        const int* __restrict__ obs_model,     // [B]
                        const unsigned char* __restrict__ done,  // [B]
                        const float* __restrict__ pop,         // [P,n]
                        const float* __restrict__ model_emb_pop,  // [P,M,16]
                        HeadOffs ho,
                        int* __restrict__ actions,             // [B]
                        float* __restrict__ lp_all,            // [B,A] / null
                        float* __restrict__ logp,              // [B] / null
                        float* __restrict__ value,             // [B] / null
                        float* __restrict__ u_out,             // [B] / null
                        int E, int A, int M, long n, int mode,
                        unsigned seed_lo, unsigned seed_hi,
                        unsigned step_lo, unsigned step_hi) {
    __shared__ float w1s[2][H1][EMB + 1];
    __shared__ float wgs[GEMB][64 + 1];
    __shared__ float ylns[WPB][64 + 1];
    __shared__ float embs[WPB][EMB + 1];
    __shared__ float h1s[WPB][H1];
    const int Fg = NGF + A;
    const int m = blockIdx.y;
    const float* th = pop + (long)m * n;
    const float* ln_w = th + ho.o[0];
    const float* ln_b = th + ho.o[1];
    const float* Wg = th + ho.o[2];
    const float* bg = th + ho.o[3];
    const float* W1p = th + ho.o[4];
    const float* b1p = th + ho.o[5];
    const float* W2p = th + ho.o[6];
    const float* b2p = th + ho.o[7];
    const float* W1v = th + ho.o[8];
    const float* b1v = th + ho.o[9];
    const float* W2v = th + ho.o[10];
    const float* b2v = th + ho.o[11];
    const float* model_emb = model_emb_pop + (long)m * M * 16;

    for (int i = threadIdx.x; i < H1 * EMB; i += BLOCK) {
        w1s[0][i / EMB][i % EMB] = W1p[i];
        w1s[1][i / EMB][i % EMB] = W1v[i];
    }
    for (int i = threadIdx.x; i < GEMB * Fg; i += BLOCK)
        wgs[i / Fg][i % Fg] = Wg[i];
    __syncthreads();
    // the only block barrier is behind us: from here on waves leave on their
    // own and synchronise with wave barriers alone

    const int wave = threadIdx.x / WAVE;
    const int lane = threadIdx.x % WAVE;
    const int e = blockIdx.x * WPB + wave;
    if (e >= E) return;                              // wave uniform
    const long r = (long)m * E + e;
    const int mid = obs_model[r];
    if (done[r] != 0 || mid < 0 || mid >= M) {       // wave uniform
        if (lane == 0) actions[r] = 0;
        return;
    }
    const float mk = (lane < A) ? obs_mask[r * A + lane] : 0.0f;
    const unsigned vb = (unsigned)__ballot(lane < A && mk > 0.0f);
    const uint4 x = philox4((unsigned)e, step_lo, step_hi, 0u,
                            seed_lo, seed_hi);
    const float u = (float)(x.x >> 8) * TWO_M24;

    // ---- LN(gf ++ mask) -> graph Linear -> concat ----
    float v = 0.0f;
    if (lane < NGF) v = obs_gf[r * NGF + lane];
    else if (lane < Fg) v = obs_mask[r * A + (lane - NGF)];
    const float mean = pwave_sum(v) / Fg;
    const float d = (lane < Fg) ? v - mean : 0.0f;
    const float var = pwave_sum_sq(d) / Fg;
    const float inv_sigma = rsqrtf(var + LN_EPS);
    if (lane < Fg)
        ylns[wave][lane] = fmaf(d * inv_sigma, ln_w[lane], ln_b[lane]);
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
    vp = pwave_sum(vp) + b2v[0];

    // max-subtracted log-softmax over the A lanes
    const float mx = pwave_max(lg);
    const float ex = (lane < A) ? expf(lg - mx) : 0.0f;
    const float lse = logf(pwave_sum(ex));
    const float lp = (lane < A) ? lg - mx - lse : -INFINITY;
    if (lp_all != nullptr && lane < A) lp_all[r * A + lane] = lp;

    int act;
    if (mode == POP_GREEDY) {
        // argmax of the masked logits, ties to the lowest index
        const unsigned long long top = __ballot(lane < A && lg == mx);
        act = __ffsll((long long)top) - 1;
        if (act < 0) act = 0;                        // all-NaN logits
    } else {
        // inverse CDF: first valid a with u < cum, else the last valid
        const float p = (lane < A) ? expf(lp) : 0.0f;
        float cum = 0.0f;
        act = -1;
        for (int a = 0; a < A; ++a) {
            cum += __shfl(p, a, WAVE);
            if (act < 0 && ((vb >> a) & 1u) && u < cum) act = a;
        }
        if (act < 0) act = vb ? (31 - __clz(vb)) : 0;
    }
    const float lpa = __shfl(lp, act, WAVE);
    if (lane == 0) {
        actions[r] = act;
        if (logp != nullptr) logp[r] = lpa;
        if (value != nullptr) value[r] = vp;
        if (u_out != nullptr) u_out[r] = u;
    }
}

// ---------------------------------------------------------------------------
static void pop_check_f32(const torch::Tensor& t, int64_t numel,
                          const char* op, const char* what) {
    TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kFloat32 &&
                t.is_contiguous() && t.numel() == numel,
                op, ": ", what, " must be a contiguous f32 device tensor of ",
                numel, " elements");
}

static float* pop_optional(const torch::Tensor& t, int64_t numel,
                           const char* what) {
    if (t.numel() == 0) return nullptr;
    pop_check_f32(t, numel, "actor_population", what);
    return t.data_ptr<float>();
}

void es_perturb(torch::Tensor theta, double sigma, uint64_t seed,
                uint64_t generation, torch::Tensor eps, torch::Tensor pop) {
    TORCH_CHECK(theta.dim() == 1, "es_perturb: theta must be [n]");
    TORCH_CHECK(eps.dim() == 2 && pop.dim() == 2,
                "es_perturb: eps must be [K,n] and pop [2K,n]");
    const int64_t n = theta.numel(), K = eps.size(0);
    TORCH_CHECK(K >= 1 && K <= 32767, "es_perturb: needs 1 <= K <= 32767");
    TORCH_CHECK(pop.size(0) == 2 * K, "es_perturb: pop must have 2K rows");
    TORCH_CHECK((n + 3) / 4 <= 0x7fffffffLL * BLOCK,
                "es_perturb: n is beyond the grid");
    pop_check_f32(theta, n, "es_perturb", "theta");
    pop_check_f32(eps, K * n, "es_perturb", "eps");
    pop_check_f32(pop, 2 * K * n, "es_perturb", "pop");
    if (n == 0) return;
    hipStream_t stream = at::cuda::getCurrentCUDAStream();
    const int64_t nq = (n + 3) / 4;
    const dim3 grid((unsigned)((nq + BLOCK - 1) / BLOCK), (unsigned)K);
    hipLaunchKernelGGL(
        es_perturb_kernel, grid, dim3(BLOCK), 0, stream,
        theta.data_ptr<float>(), eps.data_ptr<float>(), pop.data_ptr<float>(),
        (long)n, (float)sigma,
        (unsigned)(seed & 0xffffffffu), (unsigned)(seed >> 32),
        (unsigned)(generation & 0xffffffffu), (unsigned)(generation >> 32));
}

void es_update(torch::Tensor theta, torch::Tensor eps, torch::Tensor w,
               double scale, double decay, torch::Tensor out) {
    TORCH_CHECK(theta.dim() == 1 && eps.dim() == 2,
                "es_update: theta must be [n] and eps [K,n]");
    const int64_t n = theta.numel(), K = eps.size(0);
    TORCH_CHECK(K >= 1 && K <= 0x7fffffff, "es_update: needs K >= 1");
    TORCH_CHECK((n + BLOCK - 1) / BLOCK <= 0x7fffffffLL,
                "es_update: n is beyond the grid");
    pop_check_f32(theta, n, "es_update", "theta");
    pop_check_f32(eps, K * n, "es_update", "eps");
    pop_check_f32(w, K, "es_update", "w");
    pop_check_f32(out, n, "es_update", "out");
    if (n == 0) return;
    hipStream_t stream = at::cuda::getCurrentCUDAStream();
    hipLaunchKernelGGL(
        es_update_kernel, dim3((unsigned)((n + BLOCK - 1) / BLOCK)),
        dim3(BLOCK), 0, stream,
        theta.data_ptr<float>(), eps.data_ptr<float>(), w.data_ptr<float>(),
        out.data_ptr<float>(), (long)n, (int)K, (float)scale, (float)decay);
}

void actor_population(torch::Tensor obs_gf, torch::Tensor obs_mask,
                      torch::Tensor obs_model, torch::Tensor done,
                      torch::Tensor pop, torch::Tensor model_emb_pop,
                      std::vector<int64_t> head_offs, int64_t E, int64_t mode,
                      uint64_t seed, uint64_t step, torch::Tensor actions,
                      torch::Tensor lp_all, torch::Tensor logp,
                      torch::Tensor value, torch::Tensor u) {
    const char* op = "actor_population";
    TORCH_CHECK(obs_mask.dim() == 2, op, ": obs_mask must be [B,A]");
    TORCH_CHECK(pop.dim() == 2, op, ": pop must be [P,n]");
    const int64_t B = obs_mask.size(0), A = obs_mask.size(1);
    const int64_t P = pop.size(0), n = pop.size(1);
    const int64_t Fg = NGF + A;
    TORCH_CHECK(mode == POP_GREEDY || mode == POP_SAMPLE,
                op, ": mode must be 0 (greedy) or 1 (sample), not ", mode);
    TORCH_CHECK(A >= 1 && A <= 32 && Fg <= 64,
                op, ": needs 1 <= A <= 32 and 17 + A <= 64");
    TORCH_CHECK(E >= 1 && P >= 1 && P <= 65535 && B == P * E &&
                B <= 0x7fffffff,
                op, ": needs B == P * E with 1 <= P <= 65535 and E >= 1");
    pop_check_f32(obs_gf, B * NGF, op, "obs_gf");
    pop_check_f32(obs_mask, B * A, op, "obs_mask");
    pop_check_f32(pop, P * n, op, "pop");
    auto check_i32 = [&](const torch::Tensor& t, const char* what) {
        TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kInt32 &&
                    t.is_contiguous() && t.numel() == B,
                    op, ": ", what, " must be a contiguous i32 [B] device "
                    "tensor");
    };
    check_i32(obs_model, "obs_model");
    check_i32(actions, "actions");
    TORCH_CHECK(done.is_cuda() && done.scalar_type() == torch::kUInt8 &&
                done.is_contiguous() && done.numel() == B,
                op, ": done must be a contiguous u8 [B] device tensor");
    TORCH_CHECK(model_emb_pop.dim() == 3 && model_emb_pop.size(0) == P &&
                model_emb_pop.size(2) == 16,
                op, ": model_emb_pop must be [P,M,16]");
    const int64_t M = model_emb_pop.size(1);
    pop_check_f32(model_emb_pop, P * M * 16, op, "model_emb_pop");
    TORCH_CHECK(head_offs.size() == 12,
                op, ": head_offs holds head_fwd's 12 row offsets");
    const int64_t want[12] = {Fg, Fg, GEMB * Fg, GEMB, H1 * EMB, H1,
                              A * H1, A, H1 * EMB, H1, H1, 1};
    HeadOffs ho;
    for (int i = 0; i < 12; ++i) {
        TORCH_CHECK(head_offs[i] >= 0 && head_offs[i] + want[i] <= n,
                    op, ": head_offs[", i, "] = ", head_offs[i], " with ",
                    want[i], " elements leaves a pop row of ", n);
        ho.o[i] = (long)head_offs[i];
    }
    float* lp_ptr = pop_optional(lp_all, B * A, "lp_all");
    float* logp_ptr = pop_optional(logp, B, "logp");
    float* value_ptr = pop_optional(value, B, "value");
    float* u_ptr = pop_optional(u, B, "u");

    hipStream_t stream = at::cuda::getCurrentCUDAStream();
    const int64_t chunks = (E + WPB - 1) / WPB;
    TORCH_CHECK(chunks <= 0x7fffffff, op, ": E is beyond the grid");
    hipLaunchKernelGGL(
        actor_population_kernel, dim3((unsigned)chunks, (unsigned)P),
        dim3(BLOCK), 0, stream,
        obs_gf.data_ptr<float>(), obs_mask.data_ptr<float>(),
        obs_model.data_ptr<int>(), done.data_ptr<unsigned char>(),
        pop.data_ptr<float>(), model_emb_pop.data_ptr<float>(), ho,
        actions.data_ptr<int>(), lp_ptr, logp_ptr, value_ptr, u_ptr,
        (int)E, (int)A, (int)M, (long)n, (int)mode,
        (unsigned)(seed & 0xffffffffu), (unsigned)(seed >> 32),
        (unsigned)(step & 0xffffffffu), (unsigned)(step >> 32));
}
