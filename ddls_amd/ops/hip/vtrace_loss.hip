// V-trace recurrence and fused IMPALA loss forward + analytic backward for
// gfx950.
//
// The torch learner (rl/impala.py) evaluates the V-trace recurrence as a
// Python loop of T reversed steps with several tiny elementwise launches
// each, then a ~100-node autograd loss chain whose five stats are read back
// one .item() at a time.  Here the recurrence is one kernel (one lane per
// env column), and the whole loss is three launches forward, one backward:
//   K1 impala_row_kernel     one wave per sample row: log-softmax, p, lp,
//                            row entropy, logp_a, ratio = pi/mu
//   K2 impala_scan_kernel    the recurrence with rho = min(ratio, rho_clip),
//                            c = min(ratio, c_clip); pg_adv *= pg_rho
//   K3 impala_reduce_kernel  one block: 256 per-thread partials in f64,
//                            added in a fixed order (no float atomics), then
//                            the means, the total loss and the stats
//   impala_loss_bwd_kernel   closed-form d loss/d logits, d loss/d values;
//                            vs and pg_adv are constants, as in the torch
//                            learner's no_grad block
//
// Layout is [T, N] row-major (sample row i = t*N + n), the order
// EngineVectorEnv.rollout returns.
//
// Bit contract: vtrace_step() below performs each f32 add/sub/mul singly and
// in exactly the order rl/impala.py::vtrace_targets evaluates them (no FMA
// contraction), so vtrace_scan equals vtrace_targets bit for bit.
#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>
#include <vector>

#define WAVE 64
#define WAVES 4
#define BLOCK (WAVE * WAVES)

__device__ __forceinline__ float wave_max_v(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        v = fmaxf(v, __shfl_down(v, off, WAVE));
    return __shfl(v, 0, WAVE);
}

__device__ __forceinline__ float wave_sum_v(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        v += __shfl_down(v, off, WAVE);
    return __shfl(v, 0, WAVE);
}

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        v += __shfl_down(v, off, WAVE);
    return v;   // valid on lane 0
}

// One timestep of the recurrence for one env column.  v_next / vs_next are
// V(x_{t+1}) / vs_{t+1}, with the bootstrap value standing in at t = T-1.
// acc carries vs_{t+1} - V(x_{t+1}) in and vs_t - V(x_t) out.
__device__ __forceinline__ void vtrace_step(float r, float done, float v,
                                            float v_next, float vs_next,
                                            float rho, float c, float gamma,
                                            float& acc, float& vs_out,
                                            float& pg_out) {
#pragma clang fp contract(off)
    const float nonterminal = 1.0f - done;
    const float vtp1 = v_next * nonterminal;
    const float gv = gamma * vtp1;
    const float rgv = r + gv;
    const float td = rgv - v;
    const float delta = rho * td;
    const float gc = gamma * c;
    const float gcn = gc * nonterminal;
    const float carry = gcn * acc;
    acc = delta + carry;
    vs_out = v + acc;
    const float vsn = vs_next * nonterminal;
    const float gvs = gamma * vsn;
    const float rgvs = r + gvs;
    pg_out = rgvs - v;
}

// one lane per env column, t = T-1 .. 0; row t is read coalesced across lanes
__global__ void __launch_bounds__(BLOCK)
vtrace_scan_kernel(const float* __restrict__ rewards,
                   const float* __restrict__ dones,
                   const float* __restrict__ values,
                   const float* __restrict__ bootstrap,
                   const float* __restrict__ rho,
                   const float* __restrict__ c,
                   float* __restrict__ vs_out,
                   float* __restrict__ pg_out, int T, int N, float gamma) {
    const int n = blockIdx.x * BLOCK + threadIdx.x;
    if (n >= N) return;
    float acc = 0.0f;
    float v_next = bootstrap[n];
    float vs_next = v_next;
    for (int t = T - 1; t >= 0; --t) {
        const long i = (long)t * N + n;
        const float v = values[i];
        float vs, pg;
        vtrace_step(rewards[i], dones[i], v, v_next, vs_next, rho[i], c[i],
                    gamma, acc, vs, pg);
        vs_out[i] = vs;
        pg_out[i] = pg;
        v_next = v;
        vs_next = vs;
    }
}

// K1: one wave per row (A <= 64).  Masked logits arrive as finfo.min: their
// exp underflows to an exact 0 and p*lp is taken as 0, never 0*inf.
__global__ void __launch_bounds__(BLOCK)
impala_row_kernel(const float* __restrict__ logits,
                  const long* __restrict__ actions,
                  const float* __restrict__ behaviour_logp,
                  float* __restrict__ p_out,       // [R, A]
                  float* __restrict__ lp_out,      // [R, A]
                  float* __restrict__ h_out,       // [R] row entropy
                  float* __restrict__ logp_a_out,  // [R]
                  float* __restrict__ ratio_out,   // [R] pi/mu, unclipped
                  int R, int A) {
    const int wave = threadIdx.x / WAVE;
    const int lane = threadIdx.x % WAVE;
    for (int b = blockIdx.x * WAVES + wave; b < R; b += gridDim.x * WAVES) {
        const float x = (lane < A) ? logits[(long)b * A + lane] : -3.0e38f;
        const float mx = wave_max_v(x);
        const float ex = (lane < A) ? expf(x - mx) : 0.0f;
        const float Z = wave_sum_v(ex);
        const float lse = mx + logf(Z);
        const float lp = x - lse;
        const float p = ex / Z;
        if (lane < A) {
            p_out[(long)b * A + lane] = p;
            lp_out[(long)b * A + lane] = lp;
        }
        const float ent =
            -wave_sum_v((lane < A && p > 0.0f) ? p * lp : 0.0f);
        const int a = (int)actions[b];
        const float logp_a = __shfl(lp, a, WAVE);
        if (lane == 0) {
            h_out[b] = ent;
            logp_a_out[b] = logp_a;
            ratio_out[b] = expf(logp_a - behaviour_logp[b]);
        }
    }
}

// K2: the recurrence over the clipped ratios; shares vtrace_step with
// vtrace_scan_kernel.  pg_adv leaves multiplied by min(ratio, pg_rho_clip).
__global__ void __launch_bounds__(BLOCK)
impala_scan_kernel(const float* __restrict__ rewards,
                   const float* __restrict__ dones,
                   const float* __restrict__ values,
                   const float* __restrict__ bootstrap,
                   const float* __restrict__ ratio,
                   float* __restrict__ vs_out,
                   float* __restrict__ pg_out, int T, int N, float gamma,
                   float rho_clip, float pg_rho_clip, float c_clip) {
    const int n = blockIdx.x * BLOCK + threadIdx.x;
    if (n >= N) return;
    float acc = 0.0f;
    float v_next = bootstrap[n];
    float vs_next = v_next;
    for (int t = T - 1; t >= 0; --t) {
        const long i = (long)t * N + n;
        const float v = values[i];
        const float rt = ratio[i];
        float vs, pg;
        vtrace_step(rewards[i], dones[i], v, v_next, vs_next,
                    fminf(rt, rho_clip), fminf(rt, c_clip), gamma, acc, vs,
                    pg);
        vs_out[i] = vs;
        pg_out[i] = fminf(rt, pg_rho_clip) * pg;
        v_next = v;
        vs_next = vs;
    }
}

// K3: one block.  Thread j sums rows j, j+BLOCK, ... in f64 (a fixed 256
// partials), the partials are added by a fixed shuffle tree and then in wave
// order, so two calls on the same inputs give the same bits.
// stats = {policy_loss, vf_loss, entropy, total_loss, mean_rho}
__global__ void __launch_bounds__(BLOCK)
impala_reduce_kernel(const float* __restrict__ values,
                     const float* __restrict__ vs,
                     const float* __restrict__ pg_adv,
                     const float* __restrict__ logp_a,
                     const float* __restrict__ h,
                     const float* __restrict__ ratio,
                     float* __restrict__ loss_out,   // [1]
                     float* __restrict__ stats_out,  // [5]
                     int R, int K, float rho_clip, float vf_coeff,
                     float ent_coeff) {
    __shared__ double part[WAVES][4];
    const int wave = threadIdx.x / WAVE;
    const int lane = threadIdx.x % WAVE;
    double s_pg = 0.0, s_vf = 0.0, s_ent = 0.0, s_rho = 0.0;
    for (int i = threadIdx.x; i < R; i += BLOCK) {
        s_rho += (double)fminf(ratio[i], rho_clip);
        if (i < K) {   // kept rows are the first K (whole timesteps)
            const float d = vs[i] - values[i];
            s_pg += (double)(pg_adv[i] * logp_a[i]);
            s_vf += (double)(d * d);
            s_ent += (double)h[i];
        }
    }
    s_pg = wave_sum_d(s_pg);
    s_vf = wave_sum_d(s_vf);
    s_ent = wave_sum_d(s_ent);
    s_rho = wave_sum_d(s_rho);
    if (lane == 0) {
        part[wave][0] = s_pg;
        part[wave][1] = s_vf;
        part[wave][2] = s_ent;
        part[wave][3] = s_rho;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t[4] = {0.0, 0.0, 0.0, 0.0};
        for (int w = 0; w < WAVES; ++w)
            for (int q = 0; q < 4; ++q) t[q] += part[w][q];
        const float pl = (float)(-t[0] / K);
        const float vf = (float)(0.5 * t[1] / K);
        const float ent = (float)(t[2] / K);
        const float loss = pl + vf_coeff * vf - ent_coeff * ent;
        stats_out[0] = pl;
        stats_out[1] = vf;
        stats_out[2] = ent;
        stats_out[3] = loss;
        stats_out[4] = (float)(t[3] / R);
        loss_out[0] = loss;
    }
}

// one wave per row; rows at or past K (the dropped last timestep) get zeros
__global__ void __launch_bounds__(BLOCK)
impala_loss_bwd_kernel(const float* __restrict__ p,
                       const float* __restrict__ lp,
                       const float* __restrict__ h,
                       const long* __restrict__ actions,
                       const float* __restrict__ values,
                       const float* __restrict__ vs,
                       const float* __restrict__ pg_adv,
                       const float* __restrict__ gl,   // [1] upstream dloss
                       float* __restrict__ glogits,    // [R, A]
                       float* __restrict__ gvalues,    // [R]
                       int R, int A, int K, float vf_coeff,
                       float ent_coeff) {
    const int wave = threadIdx.x / WAVE;
    const int lane = threadIdx.x % WAVE;
    const float g = gl[0];
    for (int b = blockIdx.x * WAVES + wave; b < R; b += gridDim.x * WAVES) {
        if (b >= K) {
            if (lane < A) glogits[(long)b * A + lane] = 0.0f;
            if (lane == 0) gvalues[b] = 0.0f;
            continue;
        }
        const int a = (int)actions[b];
        const float coef = -pg_adv[b] / K;   // d loss/d logp_a
        const float hb = h[b];
        if (lane < A) {
            const float pj = p[(long)b * A + lane];
            const float lpj = lp[(long)b * A + lane];
            const float delta = (lane == a) ? 1.0f : 0.0f;
            // d[-ec*H]/dlogits = ec/K * p*(lp + H); p == 0 on masked lanes
            const float ent_g =
                (pj > 0.0f) ? (ent_coeff / K) * pj * (lpj + hb) : 0.0f;
            glogits[(long)b * A + lane] = g * (coef * (delta - pj) + ent_g);
        }
        if (lane == 0)
            gvalues[b] = g * vf_coeff * (values[b] - vs[b]) / K;
    }
}

static void check_f32(const torch::Tensor& t, int64_t numel,
                      const char* name) {
    TORCH_CHECK(t.is_cuda() && t.dtype() == torch::kFloat32
                && t.is_contiguous() && t.numel() == numel,
                name, ": expected a contiguous f32 CUDA tensor of ", numel,
                " elements");
}

static int scan_blocks(int N) { return (N + BLOCK - 1) / BLOCK; }

static int row_blocks(int R) {
    int blocks = (R + WAVES - 1) / WAVES;
    return blocks > 1024 ? 1024 : blocks;
}

std::vector<torch::Tensor> vtrace_scan(
    torch::Tensor rewards, torch::Tensor dones, torch::Tensor values,
    torch::Tensor bootstrap, torch::Tensor rho, torch::Tensor c,
    double gamma) {
    TORCH_CHECK(rewards.dim() == 2, "vtrace_scan: rewards must be [T, N]");
    const int64_t T = rewards.size(0), N = rewards.size(1);
    TORCH_CHECK(T >= 1 && N >= 1 && T * N < (1LL << 31),
                "vtrace_scan: T*N out of range");
    check_f32(rewards, T * N, "vtrace_scan rewards");
    check_f32(dones, T * N, "vtrace_scan dones");
    check_f32(values, T * N, "vtrace_scan values");
    check_f32(bootstrap, N, "vtrace_scan bootstrap");
    check_f32(rho, T * N, "vtrace_scan rho");
    check_f32(c, T * N, "vtrace_scan c");
    auto vs = torch::empty({T, N}, rewards.options());
    auto pg = torch::empty({T, N}, rewards.options());
    hipStream_t stream = at::cuda::getCurrentCUDAStream();
    hipLaunchKernelGGL(vtrace_scan_kernel, dim3(scan_blocks((int)N)),
                       dim3(BLOCK), 0, stream, rewards.data_ptr<float>(),
                       dones.data_ptr<float>(), values.data_ptr<float>(),
                       bootstrap.data_ptr<float>(), rho.data_ptr<float>(),
                       c.data_ptr<float>(), vs.data_ptr<float>(),
                       pg.data_ptr<float>(), (int)T, (int)N, (float)gamma);
    return {vs, pg};
}

// returns {loss[1], stats[5], p, lp, h, vs, pg_adv}; the last five (with
// actions and values) are what impala_loss_bwd needs
std::vector<torch::Tensor> impala_loss_fwd(
    torch::Tensor logits, torch::Tensor values, torch::Tensor actions,
    torch::Tensor behaviour_logp, torch::Tensor rewards, torch::Tensor dones,
    torch::Tensor bootstrap, int64_t T, int64_t N, double gamma,
    double rho_clip, double pg_rho_clip, double c_clip, double vf_coeff,
    double ent_coeff, bool drop_last) {
    TORCH_CHECK(logits.dim() == 2, "impala_loss_fwd: logits must be [T*N, A]");
    TORCH_CHECK(T >= 1 && N >= 1 && T * N < (1LL << 31),
                "impala_loss_fwd: T*N out of range");
    const int64_t R = T * N, A = logits.size(1);
    TORCH_CHECK(A >= 1 && A <= 64,
                "impala_loss_fwd needs A <= 64 (one wave per row)");
    check_f32(logits, R * A, "impala_loss_fwd logits");
    check_f32(values, R, "impala_loss_fwd values");
    check_f32(behaviour_logp, R, "impala_loss_fwd behaviour_logp");
    check_f32(rewards, R, "impala_loss_fwd rewards");
    check_f32(dones, R, "impala_loss_fwd dones");
    check_f32(bootstrap, N, "impala_loss_fwd bootstrap");
    TORCH_CHECK(actions.is_cuda() && actions.dtype() == torch::kInt64
                && actions.is_contiguous() && actions.numel() == R,
                "impala_loss_fwd actions: expected contiguous int64 [T*N]");
    const int64_t K = (drop_last && T > 1) ? (T - 1) * N : R;
    auto opt = logits.options();
    auto p = torch::empty({R, A}, opt);
    auto lp = torch::empty({R, A}, opt);
    auto h = torch::empty({R}, opt);
    auto logp_a = torch::empty({R}, opt);
    auto ratio = torch::empty({R}, opt);
    auto vs = torch::empty({R}, opt);
    auto pg = torch::empty({R}, opt);
    auto loss = torch::empty({1}, opt);
    auto stats = torch::empty({5}, opt);
    hipStream_t stream = at::cuda::getCurrentCUDAStream();
    hipLaunchKernelGGL(impala_row_kernel, dim3(row_blocks((int)R)),
                       dim3(BLOCK), 0, stream, logits.data_ptr<float>(),
                       actions.data_ptr<long>(),
                       behaviour_logp.data_ptr<float>(), p.data_ptr<float>(),
                       lp.data_ptr<float>(), h.data_ptr<float>(),
                       logp_a.data_ptr<float>(), ratio.data_ptr<float>(),
                       (int)R, (int)A);
    hipLaunchKernelGGL(impala_scan_kernel, dim3(scan_blocks((int)N)),
                       dim3(BLOCK), 0, stream, rewards.data_ptr<float>(),
                       dones.data_ptr<float>(), values.data_ptr<float>(),
                       bootstrap.data_ptr<float>(), ratio.data_ptr<float>(),
                       vs.data_ptr<float>(), pg.data_ptr<float>(), (int)T,
                       (int)N, (float)gamma, (float)rho_clip,
                       (float)pg_rho_clip, (float)c_clip);
    hipLaunchKernelGGL(impala_reduce_kernel, dim3(1), dim3(BLOCK), 0, stream,
                       values.data_ptr<float>(), vs.data_ptr<float>(),
                       pg.data_ptr<float>(), logp_a.data_ptr<float>(),
                       h.data_ptr<float>(), ratio.data_ptr<float>(),
                       loss.data_ptr<float>(), stats.data_ptr<float>(),
                       (int)R, (int)K, (float)rho_clip, (float)vf_coeff,
                       (float)ent_coeff);
    return {loss, stats, p, lp, h, vs, pg};
}

std::vector<torch::Tensor> impala_loss_bwd(
    torch::Tensor p, torch::Tensor lp, torch::Tensor h,
    torch::Tensor actions, torch::Tensor values, torch::Tensor vs,
    torch::Tensor pg_adv, torch::Tensor gl, int64_t T, int64_t N,
    double vf_coeff, double ent_coeff, bool drop_last) {
    TORCH_CHECK(p.dim() == 2 && p.size(0) == T * N,
                "impala_loss_bwd: p must be [T*N, A]");
    const int64_t R = T * N, A = p.size(1);
    TORCH_CHECK(A >= 1 && A <= 64, "impala_loss_bwd needs A <= 64");
    check_f32(p, R * A, "impala_loss_bwd p");
    check_f32(lp, R * A, "impala_loss_bwd lp");
    check_f32(h, R, "impala_loss_bwd h");
    check_f32(values, R, "impala_loss_bwd values");
    check_f32(vs, R, "impala_loss_bwd vs");
    check_f32(pg_adv, R, "impala_loss_bwd pg_adv");
    check_f32(gl, 1, "impala_loss_bwd gl");
    TORCH_CHECK(actions.is_cuda() && actions.dtype() == torch::kInt64
                && actions.is_contiguous() && actions.numel() == R,
                "impala_loss_bwd actions: expected contiguous int64 [T*N]");
    const int64_t K = (drop_last && T > 1) ? (T - 1) * N : R;
    auto glogits = torch::empty({R, A}, p.options());
    auto gvalues = torch::empty({R}, p.options());
    hipStream_t stream = at::cuda::getCurrentCUDAStream();
    hipLaunchKernelGGL(impala_loss_bwd_kernel, dim3(row_blocks((int)R)),
                       dim3(BLOCK), 0, stream, p.data_ptr<float>(),
                       lp.data_ptr<float>(), h.data_ptr<float>(),
                       actions.data_ptr<long>(), values.data_ptr<float>(),
                       vs.data_ptr<float>(), pg_adv.data_ptr<float>(),
                       gl.data_ptr<float>(), glogits.data_ptr<float>(),
                       gvalues.data_ptr<float>(), (int)R, (int)A, (int)K,
                       (float)vf_coeff, (float)ent_coeff);
    return {glogits, gvalues};
}
