// The optimiser tail of the device DQN / IMPALA learners for gfx950: global
// grad norm, clip, torch's Adam update and the per-minibatch stats
// accumulation over a LIST of ordinary parameter tensors, in one launch for
// the tuned policy (about 22k floats in 36 tensors) and two for larger ones.
//
// Tensor table.  The learners keep plain nn.Parameters whose .grad tensors are
// new allocations every minibatch, so nothing here is a view into a flat
// buffer.  The 4 * L base pointers (param, grad, exp_avg, exp_avg_sq) and the
// L + 1 element offsets of the concatenated index space travel BY VALUE in the
// kernel argument (LtTable, 2.3 KB at the fixed capacity of 64 tensors): a
// changed grad pointer costs nothing, there is no table upload to order
// against the launch.  Every block copies the table into LDS once, because
// lanes index it divergently.
//
// Work unit.  A "quad" is four consecutive elements of ONE tensor starting at
// a multiple of four inside that tensor; tensor k owns ceil(n_k / 4) quads and
// the quads of all tensors are numbered consecutively (qoff, a prefix sum one
// thread builds in LDS from the element offsets).  A full quad of a tensor whose
// four base pointers are 16-byte aligned moves as one float4 per array; the
// last quad of a tensor whose size is no multiple of four, and every quad of
// a misaligned tensor, takes the scalar path.  Numbering the quads per tensor
// keeps the vector path alive after an odd-sized tensor (the 17-wide logits
// bias, the 1-wide value bias), which element-space groups of four would not.
// A thread maps a quad number to (tensor, local quad) by walking qoff
// forward; its quad numbers only grow, so the walk never restarts.
//
//   lt_fused_kernel     total <= LT_ONE_LAUNCH_MAX elements.  Grid 1, 1024
//                       threads.  Phase 1: thread t squares the grads of quads
//                       t, t + 1024, ... in f64 (element order inside a quad,
//                       then quad order).  lt_block_sum folds the lanes of a
//                       wave by shuffles at distances 32, 16, ..., 1, parks
//                       the 16 wave sums in LDS and, after the one barrier
//                       between the phases, every thread adds them from wave
//                       0 up.  Phase 2: norm, clip, Adam over the same quads.
//   lt_partials_kernel  the larger totals: block b owns quads [b * QPB,
//   lt_update_kernel    (b + 1) * QPB), QPB = LT_QUADS_PER_BLOCK; the first
//                       stores one f64 partial per block and advances step_t,
//                       the second has every block add the partials (thread t
//                       takes t, t + 1024, ..., then lt_block_sum) and update
//                       its own range.
//
// Both paths call the same lt_locate / lt_quad_sumsq / lt_quad_update.
//
// Determinism.  No atomics and no arrival counters; every sum has one fixed
// order, so two calls on equal inputs give equal bits.
//
// Arithmetic.  clip_grad_norm_ then torch.optim.Adam (foreach, no amsgrad, no
// weight decay) in torch's operation order, every rounding written out:
//   g'  = g * clip                      clip = min(1, max_norm / (norm + 1e-6))
//   m   = m + (1 - b1) * (g' - m)       lerp
//   v   = v * b2 + (1 - b2) * (g' * g') mul, addcmul
//   d   = sqrt(v) / sqrt(bc2) + eps
//   p   = p + (-lr / bc1) * (m / d)     addcdiv
// bc1 = 1 - b1^step and bc2 = 1 - b2^step are formed in f64 from the advanced
// step counter and the three derived scalars rounded to f32 once, as torch
// forms them on the host.  max_norm <= 0 disables the clip: phase 1 is
// skipped, norm is reported as 0 and clip as 1.
#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>
#include <cmath>
#include <cstdint>
#include <vector>

// per-lane f32 ops only: no packed f32 instructions in this file's kernels
#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif
#pragma clang fp contract(off)

#define LT_WAVE 64
#define LT_BLOCK 1024
#define LT_WAVES (LT_BLOCK / LT_WAVE)
#define LT_MAX_TENSORS 64
#define LT_ONE_LAUNCH_MAX 65536      // elements served by lt_fused_kernel
#define LT_QUADS_PER_BLOCK 2048      // two-launch path: two quads per thread
#define LT_MAX_STATS 8

struct LtTable {
    float* p[LT_MAX_TENSORS];
    float* g[LT_MAX_TENSORS];
    float* m[LT_MAX_TENSORS];
    float* v[LT_MAX_TENSORS];
    int off[LT_MAX_TENSORS + 1];     // element offsets, off[n] = total
    int n;
};

struct LtHyper {
    double lr, b1, b2;
    float w1;          // (float)(1 - b1), the lerp weight
    float b2f;         // (float)b2
    float w2;          // (float)(1 - b2)
    float eps;
    float max_norm;    // <= 0: no clip
    int zero_grads;
};

// The block's LDS: the table, the quad prefix, the reduction slots and the
// step's scalars.
struct LtShared {
    float* p[LT_MAX_TENSORS];
    float* g[LT_MAX_TENSORS];
    float* m[LT_MAX_TENSORS];
    float* v[LT_MAX_TENSORS];
    int qoff[LT_MAX_TENSORS + 1];    // first quad of tensor k; qoff[n] = all
    int numel[LT_MAX_TENSORS];
    int vec[LT_MAX_TENSORS];         // all four bases 16-byte aligned
    double part[LT_WAVES];
    float bc2_sqrt, step_size;
};

// Copy the by-value table into LDS (one tensor per thread) and build the quad
// prefix.  The caller's next barrier publishes it.
__device__ __forceinline__ void lt_stage(const LtTable& T, LtShared& S) {
    const int t = threadIdx.x;
    if (t < T.n) {
        S.p[t] = T.p[t];
        S.g[t] = T.g[t];
        S.m[t] = T.m[t];
        S.v[t] = T.v[t];
        S.numel[t] = T.off[t + 1] - T.off[t];
        const uintptr_t bits = (uintptr_t)T.p[t] | (uintptr_t)T.g[t]
                               | (uintptr_t)T.m[t] | (uintptr_t)T.v[t];
        S.vec[t] = (bits & 15) == 0;
    }
    if (t == LT_BLOCK - 1) {
        int q = 0;
        for (int k = 0; k < T.n; ++k) {
            S.qoff[k] = q;
            q += (T.off[k + 1] - T.off[k] + 3) >> 2;
        }
        S.qoff[T.n] = q;
    }
}

// Advance k to the tensor that owns quad q (q < qoff[n]; k only grows).
__device__ __forceinline__ int lt_locate(const LtShared& S, int q, int k) {
    while (q >= S.qoff[k + 1]) ++k;
    return k;
}

// Sum of squares of quad q's grads in f64; x * x is exact there.
__device__ __forceinline__ double lt_quad_sumsq(const LtShared& S, int k,
                                                int q) {
    const int e0 = (q - S.qoff[k]) << 2;
    const int cnt = min(4, S.numel[k] - e0);
    const float* g = S.g[k] + e0;
    double s = 0.0;
    if (cnt == 4 && S.vec[k]) {
        const float4 x = *reinterpret_cast<const float4*>(g);
        s += (double)x.x * (double)x.x;
        s += (double)x.y * (double)x.y;
        s += (double)x.z * (double)x.z;
        s += (double)x.w * (double)x.w;
    } else {
        for (int c = 0; c < cnt; ++c) s += (double)g[c] * (double)g[c];
    }
    return s;
}

// One element of clip + Adam, in torch's operation order.
__device__ __forceinline__ void lt_element(float& p, float g, float& m,
                                           float& v, float clip,
                                           const LtHyper& H, float bc2_sqrt,
                                           float step_size) {
    const float gc = g * clip;
    const float diff = gc - m;
    // at::lerp: the form that is exact at the near end
    m = H.w1 < 0.5f ? m + H.w1 * diff : gc - diff * (1.0f - H.w1);
    const float gg = gc * gc;
    v = v * H.b2f;
    v = v + H.w2 * gg;
    const float d = sqrtf(v) / bc2_sqrt + H.eps;
    p = p + step_size * (m / d);
}

__device__ __forceinline__ void lt_quad_update(const LtShared& S, int k, int q,
                                               float clip, const LtHyper& H) {
    const int e0 = (q - S.qoff[k]) << 2;
    const int cnt = min(4, S.numel[k] - e0);
    float* p = S.p[k] + e0;
    float* g = S.g[k] + e0;
    float* m = S.m[k] + e0;
    float* v = S.v[k] + e0;
    const float bc2_sqrt = S.bc2_sqrt, step_size = S.step_size;
    if (cnt == 4 && S.vec[k]) {
        float4 pp = *reinterpret_cast<float4*>(p);
        const float4 gg = *reinterpret_cast<const float4*>(g);
        float4 mm = *reinterpret_cast<float4*>(m);
        float4 vv = *reinterpret_cast<float4*>(v);
        lt_element(pp.x, gg.x, mm.x, vv.x, clip, H, bc2_sqrt, step_size);
        lt_element(pp.y, gg.y, mm.y, vv.y, clip, H, bc2_sqrt, step_size);
        lt_element(pp.z, gg.z, mm.z, vv.z, clip, H, bc2_sqrt, step_size);
        lt_element(pp.w, gg.w, mm.w, vv.w, clip, H, bc2_sqrt, step_size);
        *reinterpret_cast<float4*>(p) = pp;
        *reinterpret_cast<float4*>(m) = mm;
        *reinterpret_cast<float4*>(v) = vv;
        if (H.zero_grads)
            *reinterpret_cast<float4*>(g) = make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
        for (int c = 0; c < cnt; ++c) {
            float pc = p[c], mc = m[c], vc = v[c];
            lt_element(pc, g[c], mc, vc, clip, H, bc2_sqrt, step_size);
            p[c] = pc;
            m[c] = mc;
            v[c] = vc;
            if (H.zero_grads) g[c] = 0.0f;
        }
    }
}

// Block sum in a fixed order: lanes by shuffles at 32, 16, ..., 1, then the
// wave sums from wave 0 up, added by every thread after the barrier (which
// also publishes whatever the caller wrote to LDS before the call).
__device__ __forceinline__ double lt_block_sum(double s, LtShared& S) {
#pragma unroll
    for (int off = LT_WAVE / 2; off > 0; off >>= 1)
        s += __shfl_down(s, off, LT_WAVE);
    if (threadIdx.x % LT_WAVE == 0) S.part[threadIdx.x / LT_WAVE] = s;
    __syncthreads();
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < LT_WAVES; ++w) t += S.part[w];
    return t;
}

// The step's scalars from the advanced step count, as torch's Adam forms them
// in Python floats: f64, rounded to f32 once.
__device__ __forceinline__ void lt_step_scalars(double step, const LtHyper& H,
                                                LtShared& S) {
    const double bc1 = 1.0 - pow(H.b1, step);
    const double bc2 = 1.0 - pow(H.b2, step);
    S.step_size = (float)(-(H.lr / bc1));
    S.bc2_sqrt = (float)sqrt(bc2);
}

__device__ __forceinline__ float lt_clip(double sumsq, const LtHyper& H,
                                         float& norm) {
    if (!(H.max_norm > 0.0f)) {
        norm = 0.0f;
        return 1.0f;
    }
    norm = (float)sqrt(sumsq);
    return fminf(H.max_norm / (norm + 1e-6f), 1.0f);
}

// Thread 0 reports norm and clip; threads i < nstats do acc[i] += stats_in[i].
__device__ __forceinline__ void lt_report(float norm, float clip,
                                          float* stats_out, float* acc,
                                          const float* stats_in, int nstats) {
    if (threadIdx.x == 0) {
        stats_out[0] = norm;
        stats_out[1] = clip;
    }
    if ((int)threadIdx.x < nstats) acc[threadIdx.x] += stats_in[threadIdx.x];
}

__global__ void __launch_bounds__(LT_BLOCK)
lt_fused_kernel(LtTable T, LtHyper H, float* __restrict__ step_t,
                float* __restrict__ stats_out, float* acc,
                const float* stats_in, int nstats) {
    __shared__ LtShared S;
    lt_stage(T, S);
    __syncthreads();
    if (threadIdx.x == 0) {
        const float step = step_t[0] + 1.0f;
        step_t[0] = step;
        lt_step_scalars((double)step, H, S);
    }
    const int nq = S.qoff[T.n];
    double s = 0.0;
    if (H.max_norm > 0.0f) {
        int k = 0;
        for (int q = threadIdx.x; q < nq; q += LT_BLOCK) {
            k = lt_locate(S, q, k);
            s += lt_quad_sumsq(S, k, q);
        }
    }
    const double sumsq = lt_block_sum(s, S);
    float norm;
    const float clip = lt_clip(sumsq, H, norm);
    int k = 0;
    for (int q = threadIdx.x; q < nq; q += LT_BLOCK) {
        k = lt_locate(S, q, k);
        lt_quad_update(S, k, q, clip, H);
    }
    lt_report(norm, clip, stats_out, acc, stats_in, nstats);
}

// nparts blocks (one when the clip is off: then it only advances step_t).
__global__ void __launch_bounds__(LT_BLOCK)
lt_partials_kernel(LtTable T, LtHyper H, float* __restrict__ step_t,
                   double* __restrict__ partials) {
    __shared__ LtShared S;
    if (blockIdx.x == 0 && threadIdx.x == 0) step_t[0] += 1.0f;
    if (!(H.max_norm > 0.0f)) return;
    lt_stage(T, S);
    __syncthreads();
    const int q0 = blockIdx.x * LT_QUADS_PER_BLOCK;
    const int q1 = min(q0 + LT_QUADS_PER_BLOCK, S.qoff[T.n]);
    double s = 0.0;
    int k = 0;
    for (int q = q0 + threadIdx.x; q < q1; q += LT_BLOCK) {
        k = lt_locate(S, q, k);
        s += lt_quad_sumsq(S, k, q);
    }
    const double t = lt_block_sum(s, S);
    if (threadIdx.x == 0) partials[blockIdx.x] = t;
}

__global__ void __launch_bounds__(LT_BLOCK)
lt_update_kernel(LtTable T, LtHyper H, const float* __restrict__ step_t,
                 const double* __restrict__ partials, int nparts,
                 float* __restrict__ stats_out, float* acc,
                 const float* stats_in, int nstats) {
    __shared__ LtShared S;
    lt_stage(T, S);
    __syncthreads();
    if (threadIdx.x == 0) lt_step_scalars((double)step_t[0], H, S);
    double s = 0.0;
    for (int b = threadIdx.x; b < nparts; b += LT_BLOCK) s += partials[b];
    const double sumsq = lt_block_sum(s, S);
    float norm;
    const float clip = lt_clip(sumsq, H, norm);
    const int q0 = blockIdx.x * LT_QUADS_PER_BLOCK;
    const int q1 = min(q0 + LT_QUADS_PER_BLOCK, S.qoff[T.n]);
    int k = 0;
    for (int q = q0 + threadIdx.x; q < q1; q += LT_BLOCK) {
        k = lt_locate(S, q, k);
        lt_quad_update(S, k, q, clip, H);
    }
    if (blockIdx.x == 0)
        lt_report(norm, clip, stats_out, acc, stats_in, nstats);
}

#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute pop
#endif

static void lt_check(const torch::Tensor& t, const torch::Tensor& like,
                     const char* what, size_t k) {
    TORCH_CHECK(t.is_cuda() && t.device() == like.device()
                && t.scalar_type() == torch::kFloat32 && t.is_contiguous()
                && t.numel() == like.numel(),
                "learner_tail: ", what, "[", k, "] must be a contiguous f32 "
                "tensor on the parameters' device with its parameter's size");
}

// {tensor capacity, largest one-launch total, elements per two-launch block}
std::vector<int64_t> learner_tail_limits() {
    return {LT_MAX_TENSORS, LT_ONE_LAUNCH_MAX, 4 * LT_QUADS_PER_BLOCK};
}

void learner_tail(std::vector<torch::Tensor> params,
                  std::vector<torch::Tensor> grads,
                  std::vector<torch::Tensor> exp_avg,
                  std::vector<torch::Tensor> exp_avg_sq, torch::Tensor step_t,
                  torch::Tensor stats_out, c10::optional<torch::Tensor> acc,
                  c10::optional<torch::Tensor> stats_in, double lr,
                  double beta1, double beta2, double eps, double max_norm,
                  bool zero_grads) {
    const size_t L = params.size();
    TORCH_CHECK(L >= 1 && L <= LT_MAX_TENSORS, "learner_tail: ", L,
                " tensors; the table holds 1 to ", LT_MAX_TENSORS);
    TORCH_CHECK(grads.size() == L && exp_avg.size() == L
                && exp_avg_sq.size() == L,
                "learner_tail: the four lists must have one length");
    LtTable T = {};
    int64_t total = 0;
    for (size_t k = 0; k < L; ++k) {
        TORCH_CHECK(params[k].device() == params[0].device(),
                    "learner_tail: the parameters live on several devices");
        lt_check(params[k], params[k], "params", k);
        lt_check(grads[k], params[k], "grads", k);
        lt_check(exp_avg[k], params[k], "exp_avg", k);
        lt_check(exp_avg_sq[k], params[k], "exp_avg_sq", k);
        T.p[k] = params[k].data_ptr<float>();
        T.g[k] = grads[k].data_ptr<float>();
        T.m[k] = exp_avg[k].data_ptr<float>();
        T.v[k] = exp_avg_sq[k].data_ptr<float>();
        T.off[k] = (int)total;
        total += params[k].numel();
        // with room for the quads' rounding up
        TORCH_CHECK(total < (int64_t)1 << 30,
                    "learner_tail: more than 2^30 elements");
    }
    T.off[L] = (int)total;
    T.n = (int)L;
    TORCH_CHECK(total > 0, "learner_tail: the tensors are empty");
    const torch::Tensor& dev = params[0];
    auto scalar_ok = [&](const torch::Tensor& t, int64_t n) {
        return t.is_cuda() && t.device() == dev.device()
               && t.scalar_type() == torch::kFloat32 && t.is_contiguous()
               && t.numel() >= n;
    };
    TORCH_CHECK(scalar_ok(step_t, 1) && step_t.numel() == 1,
                "learner_tail: step_t must be one f32 on the device");
    TORCH_CHECK(scalar_ok(stats_out, 2),
                "learner_tail: stats_out must hold two f32 on the device");
    TORCH_CHECK(acc.has_value() == stats_in.has_value(),
                "learner_tail: acc and stats_in come together");
    float* acc_p = nullptr;
    const float* in_p = nullptr;
    int nstats = 0;
    if (acc.has_value()) {
        nstats = (int)stats_in->numel();
        TORCH_CHECK(nstats <= LT_MAX_STATS && scalar_ok(*acc, nstats)
                    && scalar_ok(*stats_in, nstats)
                    && acc->numel() == nstats,
                    "learner_tail: acc and stats_in must be f32 device "
                    "tensors of one length, at most ", LT_MAX_STATS);
        acc_p = acc->data_ptr<float>();
        in_p = stats_in->data_ptr<float>();
    }
    TORCH_CHECK(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0,
                "learner_tail: betas must lie in [0, 1)");
    LtHyper H;
    H.lr = lr;
    H.b1 = beta1;
    H.b2 = beta2;
    H.w1 = (float)(1.0 - beta1);
    H.b2f = (float)beta2;
    H.w2 = (float)(1.0 - beta2);
    H.eps = (float)eps;
    H.max_norm = (float)max_norm;
    H.zero_grads = zero_grads ? 1 : 0;

    hipStream_t stream = at::cuda::getCurrentCUDAStream();
    if (total <= LT_ONE_LAUNCH_MAX) {
        hipLaunchKernelGGL(lt_fused_kernel, dim3(1), dim3(LT_BLOCK), 0, stream,
                           T, H, step_t.data_ptr<float>(),
                           stats_out.data_ptr<float>(), acc_p, in_p, nstats);
        return;
    }
    int64_t nq = 0;
    for (size_t k = 0; k < L; ++k) nq += (params[k].numel() + 3) / 4;
    const int nblocks =
        (int)((nq + LT_QUADS_PER_BLOCK - 1) / LT_QUADS_PER_BLOCK);
    const int nparts = max_norm > 0.0 ? nblocks : 0;
    auto partials = torch::empty(
        {nblocks}, torch::dtype(torch::kFloat64).device(dev.device()));
    hipLaunchKernelGGL(lt_partials_kernel, dim3(nparts > 0 ? nparts : 1),
                       dim3(LT_BLOCK), 0, stream, T, H,
                       step_t.data_ptr<float>(), partials.data_ptr<double>());
    hipLaunchKernelGGL(lt_update_kernel, dim3(nblocks), dim3(LT_BLOCK), 0,
                       stream, T, H, step_t.data_ptr<float>(),
                       partials.data_ptr<double>(), nparts,
                       stats_out.data_ptr<float>(), acc_p, in_p, nstats);
}
