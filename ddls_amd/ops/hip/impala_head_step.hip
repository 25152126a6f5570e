// Fused actor-critic head step of the IMPALA device learner for gfx950: the
// head forward over the whole [T, N] batch, the V-trace loss and the analytic
// backward into the 12 head tensors (head_params order) and the per-model
// embeddings, reading the flat tensors of rollout(device_resident=True).
//
// Built for R = T*N in the thousands: a block stages the head in LDS once and
// serves IH_ROWS = 64 rows, one 16-row MFMA tile per wave.
//
// Forward, two launches:
//   ihs_fwd_kernel          per 16-row tile: LN of gfull -> Linear(F,8) ->
//                           gather + concat -> final [16, 24]; then the
//                           TRANSPOSED products on v_mfma_f32_16x16x4_f32:
//                             h1^T [512 x 16] = W1 [512 x 24] . final^T
//                             out^T [A x 16]  = W2p [A x 256] . h1p^T
//                           The D fragment of the first product (lane (g, j)
//                           holds hidden units 16t + 4g + reg of row j) is the
//                           B operand of the second as it stands: MFMA step
//                           `reg` of hidden tile t contracts k = 16t + 4g +
//                           reg, a permuted k order inside the 16-block that
//                           the A operand (W2p from LDS) follows.  No LDS
//                           round trip between the layers.  The value output
//                           (one row of W2v) is 4 f64 FMAs per tile on the
//                           same fragment.  Row epilogue in the same launch:
//                           clamp(log(mask)), log-softmax, p, lp, entropy,
//                           logp_a, ratio = pi/mu (impala_row_kernel's job).
//   ihs_scan_reduce_kernel  one block: the V-trace recurrence (vtrace_step of
//                           vtrace_step.h, one thread per env column) and, in
//                           the same pass, the f64 sums of the loss terms;
//                           a fixed shuffle tree and wave order give loss,
//                           stats[5] and the OR of the rows' validation flags
// Backward, two launches:
//   ihs_bwd_rows_kernel     per 16-row tile: closed-form d loss / d logits
//                           and d value (rows at or past K give zeros), then
//                           gz^T = W2^T . gl^T (masked by h1 > 0) and
//                           dfinal^T = W1^T . gz^T, chained through the D
//                           fragments the same way; d LN-output from dfinal
//   ihs_bwd_wgrad_kernel    every sum over rows.  One block (8 waves) per
//                           16x16 output tile of the weight grads, k = row
//                           index on MFMA; one block for the LN grads; one
//                           block per model for g_model_emb.
//
// Fragment map of 16x16x4 (dqn_head_step.hip): A[i = lane&15][k = lane>>4],
// B[k = lane>>4][j = lane&15], D: col = lane&15, row = (lane>>4)*4 + reg.
// Below m = lane & 15 and g = lane >> 4.
//
// Row sums.  Rows are split into chunks of IW_CHUNK = 128 (a compile-time
// constant); in a round wave w of the block takes chunk round*8 + w, sums it
// 32 rows at a time in the f32 MFMA accumulator and folds those into the
// chunk's own f64 partial; wave 0 then adds the 8 partials in chunk order.
// No float atomics, no arrival counters: two calls give the same bits.
//
// Precision.  The first layer accumulates its 24 terms on top of the bias in
// the f32 MFMA accumulator.  The 256-deep second layer and the 512-deep
// dfinal fold a 16-term f32 MFMA partial into f64 per hidden tile.  The row
// epilogue and the closed-form gradients are f64, rounded once per stored
// value.  h1 [R, 512] is SAVED by the forward (the weight grads contract over
// it), not recomputed.
//
// Validation.  A model id outside [0, M) or an action outside [0, A) never
// indexes memory: the row reads model / action 0 and raises the device flag
// `err` (dqn_head_step_fwd's err / validate convention).
#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>
#include <cfloat>
#include <cmath>
#include <vector>

#include "vtrace_step.h"

// per-lane f32 ops only: no packed f32 instructions in this file's kernels
#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

#define WAVE 64
#define IH_WAVES 4
#define IH_BLOCK (WAVE * IH_WAVES)
#define IH_TILE 16                    // rows per wave: one MFMA tile
#define IH_ROWS (IH_TILE * IH_WAVES)  // rows per block
#define IH_HID 256
#define IH_EMB 24        // 16 node + 8 graph
#define IH_NODE 16
#define IH_GR 8
#define IH_AMAX 32
#define IH_FMAX 64
#define IH_GF 17         // graph features in front of the action mask
#define IH_W1S 25        // LDS row stride of W1 (24 + 1: conflict-free in i)
#define IH_W2S 260       // LDS row stride of W2p (256 + 4, keeps 16 B aligned)
#define IH_LDH 528       // saved h1: h1p | h1v | ones column tile
#define IH_LDF 32        // saved final: 24 | one | zeros
#define IH_LDY 80        // saved LN output: 64 | ones column tile
#define IH_LDG 48        // d logits: 32 | d value | zeros
#define IH_LN_EPS 1e-5
#define IW_WAVES 8
#define IW_BLOCK (WAVE * IW_WAVES)
#define IW_SUB 32        // rows per f32 MFMA partial
#define IW_CHUNK 128     // rows per chunk (one wave, one f64 partial)

typedef float ih_f4 __attribute__((ext_vector_type(4)));

struct IhHead {          // head_params(policy) order
    const float *ln_w, *ln_b, *Wg, *bg, *W1p, *b1p, *W2p, *b2p, *W1v, *b1v,
        *W2v, *b2v;
};

struct IhGrads {
    float *ln_w, *ln_b, *Wg, *bg, *W1p, *b1p, *W2p, *b2p, *W1v, *b1v, *W2v,
        *b2v, *emb;
};

// the head (about 88 KB) plus each wave's tile scratch (8 KB): about 121 KB
struct IhLds {
    float W1[2 * IH_HID * IH_W1S];    // rows 0..255 policy, 256..511 value
    float W2p[IH_AMAX * IH_W2S];      // rows at or past A are zero
    float W2v[IH_HID];
    float b1[2 * IH_HID];
    float b2p[IH_AMAX];
    float Wg[IH_GR * IH_FMAX];
    float bg[IH_GR];
    float lnw[IH_FMAX];
    float lnb[IH_FMAX];
    float b2v;
    float y[IH_WAVES][IH_TILE][IH_FMAX];     // LN output
    float fin[IH_WAVES][IH_TILE][IH_LDF];    // final (bwd: d final)
    float lm[IH_WAVES][IH_TILE][IH_AMAX];    // clamp(log(mask))
};

__device__ __forceinline__ double ih_wave_sum_all(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        v += __shfl_xor(v, off, WAVE);
    return v;
}

__device__ __forceinline__ double ih_wave_sum_d(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        v += __shfl_down(v, off, WAVE);
    return v;   // valid on lane 0
}

// sum over the four lanes (g = 0..3) that share a row j; every lane gets it
__device__ __forceinline__ double ih_row_sum(double v) {
    v += __shfl_xor(v, 16, WAVE);
    v += __shfl_xor(v, 32, WAVE);
    return v;
}

__device__ __forceinline__ void ih_stage(IhLds& L, const IhHead& w, int A,
                                         int F) {
    const int tid = threadIdx.x;
    for (int e = tid; e < IH_HID * IH_EMB; e += IH_BLOCK) {
        const int j = e / IH_EMB, i = e % IH_EMB;
        L.W1[j * IH_W1S + i] = w.W1p[e];
        L.W1[(IH_HID + j) * IH_W1S + i] = w.W1v[e];
    }
    for (int e = tid; e < IH_AMAX * IH_HID; e += IH_BLOCK) {
        const int o = e / IH_HID, u = e % IH_HID;
        L.W2p[o * IH_W2S + u] = o < A ? w.W2p[e] : 0.0f;
    }
    for (int e = tid; e < IH_GR * IH_FMAX; e += IH_BLOCK) {
        const int k = e / IH_FMAX, f = e % IH_FMAX;
        L.Wg[e] = f < F ? w.Wg[k * F + f] : 0.0f;
    }
    L.W2v[tid] = w.W2v[tid];
    L.b1[tid] = w.b1p[tid];
    L.b1[IH_HID + tid] = w.b1v[tid];
    if (tid < IH_AMAX) L.b2p[tid] = tid < A ? w.b2p[tid] : 0.0f;
    if (tid < IH_GR) L.bg[tid] = w.bg[tid];
    if (tid < IH_FMAX) {
        L.lnw[tid] = tid < F ? w.ln_w[tid] : 0.0f;
        L.lnb[tid] = tid < F ? w.ln_b[tid] : 0.0f;
    }
    if (tid == 0) L.b2v = w.b2v[0];
    __syncthreads();
}

// Every per-row array has Rpad = gridDim.x * IH_ROWS rows, so a tile stores
// all its rows unguarded; rows at or past R are stored as zeros (they pad the
// weight grads' k) and read row R - 1 of the inputs.
__global__ void __launch_bounds__(IH_BLOCK)
ihs_fwd_kernel(const float* __restrict__ gfull,      // [R, F]
               const long* __restrict__ model_ids,   // [R]
               const long* __restrict__ actions,     // [R]
               const float* __restrict__ mu_logp,    // [R]
               const float* __restrict__ emb,        // [M, 16]
               IhHead head,
               float* __restrict__ p_out,            // [Rpad, 32]
               float* __restrict__ lp_out,           // [Rpad, 32]
               float* __restrict__ h_out,            // [Rpad] row entropy
               float* __restrict__ logp_a_out,       // [Rpad]
               float* __restrict__ ratio_out,        // [Rpad] pi/mu
               float* __restrict__ values_out,       // [Rpad]
               float* __restrict__ sv_y,             // [Rpad, IH_LDY]
               float* __restrict__ sv_xhat,          // [Rpad, 64]
               float* __restrict__ sv_fin,           // [Rpad, IH_LDF]
               float* __restrict__ sv_h1,            // [Rpad, IH_LDH]
               int* __restrict__ sv_mid,             // [Rpad]
               int* __restrict__ sv_act,             // [Rpad]
               int* __restrict__ rowerr,             // [Rpad]
               long R, int A, int F, int M) {
    __shared__ IhLds L;
    ih_stage(L, head, A, F);
    const int tid = threadIdx.x;
    const int wave = tid / WAVE, lane = tid % WAVE;
    const int m = lane & 15, g = lane >> 4;
    const long row0 = (long)blockIdx.x * IH_ROWS + wave * IH_TILE;

    // LN, clamp(log(mask)), the embedding gather, validation
    for (int r = 0; r < IH_TILE; ++r) {
        const long row = row0 + r;
        const bool live = row < R;
        const long rr = live ? row : R - 1;
        const bool in = lane < F;
        const float xv = in ? gfull[rr * F + lane] : 0.0f;
        const double mean = ih_wave_sum_all(in ? (double)xv : 0.0) / F;
        const double d = in ? (double)xv - mean : 0.0;
        const double var = ih_wave_sum_all(d * d) / F;
        const double xh = d / sqrt(var + IH_LN_EPS);
        const float y = in ? (float)(xh * (double)L.lnw[lane]
                                     + (double)L.lnb[lane]) : 0.0f;
        L.y[wave][r][lane] = y;
        if (lane >= IH_GF && lane < IH_GF + IH_AMAX)
            L.lm[wave][r][lane - IH_GF] =
                in ? (float)fmax(log((double)xv), -(double)FLT_MAX) : 0.0f;
        sv_y[row * IH_LDY + lane] = live ? y : 0.0f;
        if (lane < 16)
            sv_y[row * IH_LDY + IH_FMAX + lane] =
                (live && lane == 0) ? 1.0f : 0.0f;
        sv_xhat[row * IH_FMAX + lane] = live ? (float)xh : 0.0f;
        long mid = model_ids[rr];
        int bad = mid < 0 || mid >= M;
        if (bad) mid = 0;
        long a = actions[rr];
        if (a < 0 || a >= A) { bad = 1; a = 0; }
        if (lane < IH_NODE) L.fin[wave][r][lane] = emb[mid * IH_NODE + lane];
        if (lane == 0) {
            sv_mid[row] = live ? (int)mid : -1;
            sv_act[row] = (int)a;
            rowerr[row] = live ? bad : 0;
        }
    }
    __syncthreads();
    // graph embedding: 8 lanes per output, then a 3-step butterfly
    for (int r = 0; r < IH_TILE; ++r) {
        const int k = lane >> 3, part = lane & 7;
        double acc = 0.0;
        for (int f = part; f < F; f += 8)
            acc = fma((double)L.Wg[k * IH_FMAX + f], (double)L.y[wave][r][f],
                      acc);
        acc += __shfl_xor(acc, 1, WAVE);
        acc += __shfl_xor(acc, 2, WAVE);
        acc += __shfl_xor(acc, 4, WAVE);
        if (part == 0)
            L.fin[wave][r][IH_NODE + k] = (float)(acc + (double)L.bg[k]);
    }
    __syncthreads();
    for (int r = 0; r < IH_TILE; ++r) {
        const long row = row0 + r;
        if (lane < IH_LDF) {
            const float v = lane < IH_EMB ? L.fin[wave][r][lane]
                                          : (lane == IH_EMB ? 1.0f : 0.0f);
            sv_fin[row * IH_LDF + lane] = row < R ? v : 0.0f;
        }
    }

    // the two layers on the transposed tiles; this lane's row is j = m
    const long rowj = row0 + m;
    const bool livej = rowj < R;
    const long rrj = livej ? rowj : R - 1;
    float bf[IH_EMB / 4];
#pragma unroll
    for (int s = 0; s < IH_EMB / 4; ++s) bf[s] = L.fin[wave][m][4 * s + g];
    const int n_ot = A > 16 ? 2 : 1;
    double out[2][4] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}};
    double vacc = 0.0;
    for (int t = 0; t < 2 * IH_HID / 16; ++t) {
        const int u0 = 16 * t + 4 * g;      // this lane's 4 hidden units
        ih_f4 acc = {L.b1[u0], L.b1[u0 + 1], L.b1[u0 + 2], L.b1[u0 + 3]};
        const float* w1 = &L.W1[(16 * t + m) * IH_W1S + g];
#pragma unroll
        for (int s = 0; s < IH_EMB / 4; ++s)
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w1[4 * s], bf[s], acc,
                                                       0, 0, 0);
        ih_f4 h;
#pragma unroll
        for (int q = 0; q < 4; ++q) h[q] = fmaxf(acc[q], 0.0f);
        ih_f4 hs = {0.0f, 0.0f, 0.0f, 0.0f};
        if (livej) hs = h;
        *reinterpret_cast<ih_f4*>(&sv_h1[rowj * IH_LDH + u0]) = hs;
        if (t < IH_HID / 16) {
            for (int ot = 0; ot < n_ot; ++ot) {
                const float* w2 = &L.W2p[(16 * ot + m) * IH_W2S + u0];
                ih_f4 a2 = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    a2 = __builtin_amdgcn_mfma_f32_16x16x4f32(w2[q], h[q], a2,
                                                              0, 0, 0);
#pragma unroll
                for (int q = 0; q < 4; ++q) out[ot][q] += (double)a2[q];
            }
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                vacc = fma((double)L.W2v[u0 - IH_HID + q], (double)h[q], vacc);
        }
    }
    {   // ones column tile of the saved h1
        ih_f4 one = {0.0f, 0.0f, 0.0f, 0.0f};
        if (g == 0 && livej) one[0] = 1.0f;
        *reinterpret_cast<ih_f4*>(&sv_h1[rowj * IH_LDH + 2 * IH_HID + 4 * g]) =
            one;
    }
    vacc = ih_row_sum(vacc);
    const float value = (float)(vacc + (double)L.b2v);

    // row epilogue: lane (g, m) holds actions 16 ot + 4 g + q of row m
    double x[2][4];
    bool valid[2][4];
    double mx = -HUGE_VAL;
#pragma unroll
    for (int ot = 0; ot < 2; ++ot)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int o = 16 * ot + 4 * g + q;
            valid[ot][q] = o < A;
            const float xf = (float)((out[ot][q] + (double)L.b2p[o])
                                     + (double)L.lm[wave][m][o]);
            x[ot][q] = valid[ot][q] ? (double)xf : -HUGE_VAL;
            mx = fmax(mx, x[ot][q]);
        }
    mx = fmax(mx, __shfl_xor(mx, 16, WAVE));
    mx = fmax(mx, __shfl_xor(mx, 32, WAVE));
    double ex[2][4];
    double Z = 0.0;
#pragma unroll
    for (int ot = 0; ot < 2; ++ot)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            ex[ot][q] = valid[ot][q] ? exp(x[ot][q] - mx) : 0.0;
            Z += ex[ot][q];
        }
    Z = ih_row_sum(Z);
    const double lse = mx + log(Z);
    long a = actions[rrj];
    if (a < 0 || a >= A) a = 0;
    double ent = 0.0, lpa = 0.0;
    ih_f4 pv[2], lpv[2];
#pragma unroll
    for (int ot = 0; ot < 2; ++ot)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int o = 16 * ot + 4 * g + q;
            const double lp = valid[ot][q] ? x[ot][q] - lse : 0.0;
            const double p = ex[ot][q] / Z;
            // a masked lane's p * lp is taken as 0, never 0 * inf
            if (valid[ot][q] && p > 0.0) ent += p * lp;
            if (o == (int)a) lpa = lp;
            pv[ot][q] = livej ? (float)p : 0.0f;
            lpv[ot][q] = livej ? (float)lp : 0.0f;
        }
    ent = -ih_row_sum(ent);
    lpa = ih_row_sum(lpa);
#pragma unroll
    for (int ot = 0; ot < 2; ++ot) {
        *reinterpret_cast<ih_f4*>(&p_out[rowj * IH_AMAX + 16 * ot + 4 * g]) =
            pv[ot];
        *reinterpret_cast<ih_f4*>(&lp_out[rowj * IH_AMAX + 16 * ot + 4 * g]) =
            lpv[ot];
    }
    if (g == 0) {
        const float lpa_f = (float)lpa;
        h_out[rowj] = livej ? (float)ent : 0.0f;
        logp_a_out[rowj] = livej ? lpa_f : 0.0f;
        ratio_out[rowj] =
            livej ? (float)exp((double)lpa_f - (double)mu_logp[rrj]) : 0.0f;
        values_out[rowj] = livej ? value : 0.0f;
    }
}

// One block.  Thread j owns env columns j, j + 256, ...: the recurrence of
// impala_scan_kernel (vs and pg_adv * min(ratio, pg_rho_clip) are stored for
// the backward) and, in the same pass, f64 partials of the loss terms, which
// are then added by a fixed shuffle tree and in wave order.
// stats = {policy_loss, vf_loss, entropy, total_loss, mean_rho}
__global__ void __launch_bounds__(IH_BLOCK)
ihs_scan_reduce_kernel(const float* __restrict__ rewards,
                       const float* __restrict__ dones,
                       const float* __restrict__ values,
                       const float* __restrict__ bootstrap,
                       const float* __restrict__ ratio,
                       const float* __restrict__ logp_a,
                       const float* __restrict__ h,
                       const int* __restrict__ rowerr,
                       float* __restrict__ vs_out,
                       float* __restrict__ pg_out,
                       float* __restrict__ loss_out,   // [1]
                       float* __restrict__ stats_out,  // [5]
                       int* __restrict__ err_out,      // [1]
                       int* __restrict__ err_acc,      // [1] or null
                       int T, int N, long K, float gamma, float rho_clip,
                       float pg_rho_clip, float c_clip, float vf_coeff,
                       float ent_coeff) {
    __shared__ double part[IH_WAVES][4];
    __shared__ int bad[IH_WAVES];
    const int wave = threadIdx.x / WAVE;
    const int lane = threadIdx.x % WAVE;
    double s_pg = 0.0, s_vf = 0.0, s_ent = 0.0, s_rho = 0.0;
    int e = 0;
    for (int n = threadIdx.x; n < N; n += IH_BLOCK) {
        float acc = 0.0f;
        float v_next = bootstrap[n];
        float vs_next = v_next;
        for (int t = T - 1; t >= 0; --t) {
            const long i = (long)t * N + n;
            const float v = values[i];
            const float rt = ratio[i];
            float vs, pg;
            vtrace_step(rewards[i], dones[i], v, v_next, vs_next,
                        fminf(rt, rho_clip), fminf(rt, c_clip), gamma, acc,
                        vs, pg);
            const float pgc = fminf(rt, pg_rho_clip) * pg;
            vs_out[i] = vs;
            pg_out[i] = pgc;
            v_next = v;
            vs_next = vs;
            s_rho += (double)fminf(rt, rho_clip);
            if (i < K) {   // kept rows are the first K (whole timesteps)
                const double d = (double)vs - (double)v;
                s_pg += (double)pgc * (double)logp_a[i];
                s_vf += d * d;
                s_ent += (double)h[i];
            }
            e |= rowerr[i];
        }
    }
    s_pg = ih_wave_sum_d(s_pg);
    s_vf = ih_wave_sum_d(s_vf);
    s_ent = ih_wave_sum_d(s_ent);
    s_rho = ih_wave_sum_d(s_rho);
    const int any = __ballot(e != 0) != 0;
    if (lane == 0) {
        part[wave][0] = s_pg;
        part[wave][1] = s_vf;
        part[wave][2] = s_ent;
        part[wave][3] = s_rho;
        bad[wave] = any;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t[4] = {0.0, 0.0, 0.0, 0.0};
        int eb = 0;
        for (int w = 0; w < IH_WAVES; ++w) {
            for (int q = 0; q < 4; ++q) t[q] += part[w][q];
            eb |= bad[w];
        }
        const double R = (double)T * (double)N;
        const double pl = -t[0] / (double)K;
        const double vf = 0.5 * t[1] / (double)K;
        const double ent = t[2] / (double)K;
        // combined in f64, rounded once
        const float loss = (float)((pl + (double)vf_coeff * vf)
                                   - (double)ent_coeff * ent);
        stats_out[0] = (float)pl;
        stats_out[1] = (float)vf;
        stats_out[2] = (float)ent;
        stats_out[3] = loss;
        stats_out[4] = (float)(t[3] / R);
        loss_out[0] = loss;
        err_out[0] = eb;
        if (err_acc != nullptr) err_acc[0] |= eb;
    }
}

// Per 16-row tile: d loss / d logits and d value (impala_loss_bwd_kernel's
// closed form), gz = (gl . W2) masked by h1 > 0, d final = gz . W1, and the
// gradient of the LN output through Wg.
__global__ void __launch_bounds__(IH_BLOCK)
ihs_bwd_rows_kernel(const float* __restrict__ p,        // [Rpad, 32]
                    const float* __restrict__ lp,       // [Rpad, 32]
                    const float* __restrict__ h,        // [Rpad]
                    const float* __restrict__ values,   // [Rpad]
                    const float* __restrict__ vs,       // [Rpad]
                    const float* __restrict__ pg_adv,   // [Rpad]
                    const int* __restrict__ sv_act,     // [Rpad]
                    const float* __restrict__ sv_h1,    // [Rpad, IH_LDH]
                    const float* __restrict__ gl,       // [1] upstream
                    IhHead head,
                    float* __restrict__ glx,            // [Rpad, IH_LDG]
                    float* __restrict__ gz,             // [Rpad, 512]
                    float* __restrict__ gfin,           // [Rpad, IH_LDF]
                    float* __restrict__ gy,             // [Rpad, 64]
                    long K, int A, int F, float vf_coeff, float ent_coeff) {
    __shared__ IhLds L;
    ih_stage(L, head, A, F);
    const int tid = threadIdx.x;
    const int wave = tid / WAVE, lane = tid % WAVE;
    const int m = lane & 15, g = lane >> 4;
    const long row0 = (long)blockIdx.x * IH_ROWS + wave * IH_TILE;
    const long rowj = row0 + m;
    const bool live = rowj < K;
    const double gup = (double)gl[0];
    const double dK = (double)K;
    const int n_ot = A > 16 ? 2 : 1;

    const int a = sv_act[rowj];
    const double coef = live ? -(double)pg_adv[rowj] / dK : 0.0;
    const double hb = (double)h[rowj];
    ih_f4 gj[2];
#pragma unroll
    for (int ot = 0; ot < 2; ++ot) {
        const ih_f4 pj = *reinterpret_cast<const ih_f4*>(
            &p[rowj * IH_AMAX + 16 * ot + 4 * g]);
        const ih_f4 lpj = *reinterpret_cast<const ih_f4*>(
            &lp[rowj * IH_AMAX + 16 * ot + 4 * g]);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int o = 16 * ot + 4 * g + q;
            const double pd = (double)pj[q];
            const double delta = (o == a) ? 1.0 : 0.0;
            // d[-ec*H]/dlogits = ec/K * p*(lp + H); p == 0 on masked lanes
            const double ent_g = pj[q] > 0.0f
                ? ((double)ent_coeff / dK) * pd * ((double)lpj[q] + hb) : 0.0;
            gj[ot][q] = (live && o < A)
                ? (float)(gup * (coef * (delta - pd) + ent_g)) : 0.0f;
        }
        *reinterpret_cast<ih_f4*>(&glx[rowj * IH_LDG + 16 * ot + 4 * g]) =
            gj[ot];
    }
    const float gv = live
        ? (float)(gup * (double)vf_coeff
                  * ((double)values[rowj] - (double)vs[rowj]) / dK) : 0.0f;
    {
        ih_f4 t4 = {0.0f, 0.0f, 0.0f, 0.0f};
        if (g == 0) t4[0] = gv;
        *reinterpret_cast<ih_f4*>(&glx[rowj * IH_LDG + IH_AMAX + 4 * g]) = t4;
    }

    double df[2][4] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}};
    for (int t = 0; t < 2 * IH_HID / 16; ++t) {
        const int u0 = 16 * t + 4 * g;      // this lane's 4 hidden units
        ih_f4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
        if (t < IH_HID / 16) {
            // gzp^T [16 hidden x 16 rows] = W2p^T . gl^T, k = 16 ot + 4 g + q
            for (int ot = 0; ot < n_ot; ++ot) {
                const float* w2 =
                    &L.W2p[(16 * ot + 4 * g) * IH_W2S + 16 * t + m];
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(
                        w2[q * IH_W2S], gj[ot][q], acc, 0, 0, 0);
            }
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                acc[q] = gv * L.W2v[u0 - IH_HID + q];
        }
        const ih_f4 h1 = *reinterpret_cast<const ih_f4*>(
            &sv_h1[rowj * IH_LDH + u0]);
        ih_f4 z;
#pragma unroll
        for (int q = 0; q < 4; ++q) z[q] = h1[q] > 0.0f ? acc[q] : 0.0f;
        *reinterpret_cast<ih_f4*>(&gz[rowj * 2 * IH_HID + u0]) = z;
        // d final^T [24 x 16 rows] += W1^T . gz^T, k = 16 t + 4 g + q
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int i = 16 * it + m;
            ih_f4 d = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float w1 =
                    i < IH_EMB ? L.W1[(u0 + q) * IH_W1S + i] : 0.0f;
                d = __builtin_amdgcn_mfma_f32_16x16x4f32(w1, z[q], d, 0, 0,
                                                         0);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) df[it][q] += (double)d[q];
        }
    }
    // lane (g, m) holds d final[row m][16 it + 4 g + q]
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        ih_f4 o4;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            o4[q] = (float)df[it][q];
            L.fin[wave][m][16 * it + 4 * g + q] = o4[q];
        }
        *reinterpret_cast<ih_f4*>(&gfin[rowj * IH_LDF + 16 * it + 4 * g]) =
            o4;
    }
    __syncthreads();
    for (int r = 0; r < IH_TILE; ++r) {
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < IH_GR; ++k)
            acc = fma((double)L.fin[wave][r][IH_NODE + k],
                      (double)L.Wg[k * IH_FMAX + lane], acc);
        gy[(row0 + r) * IH_FMAX + lane] = lane < F ? (float)acc : 0.0f;
    }
}

// Wave `wave` of the block sums its chunk of each round; wave 0 folds the
// rounds' IW_WAVES partials in chunk order into `total` (valid on wave 0).
// D[16x16] = sum over rows k of P[k][pcol0 + i] * Q[k][qcol0 + j]; out[reg]
// is D's row (lane>>4)*4 + reg, column lane&15.  Rk = rows padded to 4.
__device__ __forceinline__ void iw_mfma_tile(
    const float* __restrict__ P, int ldp, int pcol0,
    const float* __restrict__ Q, int ldq, int qcol0, long Rk, int wave,
    int lane, double (*part)[WAVE][4], double total[4]) {
    const int m = lane & 15, kp = lane >> 4;
    const float* p = P + (long)kp * ldp + pcol0 + m;
    const float* q = Q + (long)kp * ldq + qcol0 + m;
    total[0] = total[1] = total[2] = total[3] = 0.0;
    for (long base = 0; base < Rk; base += (long)IW_WAVES * IW_CHUNK) {
        const long c0 = base + (long)wave * IW_CHUNK;
        double ch[4] = {0.0, 0.0, 0.0, 0.0};
        for (int sub = 0; sub < IW_CHUNK; sub += IW_SUB) {
            const long k0 = c0 + sub;
            if (k0 >= Rk) break;
            ih_f4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
            if (k0 + IW_SUB <= Rk) {
#pragma unroll
                for (int s = 0; s < IW_SUB; s += 4)
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(
                        p[(k0 + s) * ldp], q[(k0 + s) * ldq], acc, 0, 0, 0);
            } else {
                for (long k = k0; k < Rk; k += 4)
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(
                        p[k * ldp], q[k * ldq], acc, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) ch[r] += (double)acc[r];
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) part[wave][lane][r] = ch[r];
        __syncthreads();
        if (wave == 0) {
            for (int w = 0; w < IW_WAVES; ++w)
#pragma unroll
                for (int r = 0; r < 4; ++r) total[r] += part[w][lane][r];
        }
        __syncthreads();
    }
}

#define IW_T_W1 64       // gz^T [512 x k] . final_ext [k x 32]
#define IW_T_W2 51       // glx^T [48 x k] . h1_ext [k x 17 tiles]
#define IW_T_WG 5        // d graph_emb^T [8(16) x k] . y_ext [k x 80]
#define IW_TILES (IW_T_W1 + IW_T_W2 + IW_T_WG)

__global__ void __launch_bounds__(IW_BLOCK)
ihs_bwd_wgrad_kernel(const float* __restrict__ glx,     // [Rpad, IH_LDG]
                     const float* __restrict__ gz,      // [Rpad, 512]
                     const float* __restrict__ gfin,    // [Rpad, IH_LDF]
                     const float* __restrict__ gy,      // [Rpad, 64]
                     const float* __restrict__ sv_y,    // [Rpad, IH_LDY]
                     const float* __restrict__ sv_xhat, // [Rpad, 64]
                     const float* __restrict__ sv_fin,  // [Rpad, IH_LDF]
                     const float* __restrict__ sv_h1,   // [Rpad, IH_LDH]
                     const int* __restrict__ sv_mid,    // [Rpad]
                     IhGrads G, long R, int A, int F, int M) {
    __shared__ double part[IW_WAVES][WAVE][4];
    const int tid = threadIdx.x;
    const int wave = tid / WAVE, lane = tid % WAVE;
    const long Rk = (R + 3) / 4 * 4;    // rows R..Rk-1 are zero rows
    if (blockIdx.x < IW_TILES) {
        int t = blockIdx.x;
        const int col = lane & 15, row0 = (lane >> 4) * 4;
        double d[4];
        if (t < IW_T_W1) {
            const int jt = t >> 1, it = t & 1;
            iw_mfma_tile(gz, 2 * IH_HID, jt * 16, sv_fin, IH_LDF, it * 16, Rk,
                         wave, lane, part, d);
            if (wave != 0) return;
            const int i = it * 16 + col;
            float* gW = jt < 16 ? G.W1p : G.W1v;
            float* gb = jt < 16 ? G.b1p : G.b1v;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int j = (jt & 15) * 16 + row0 + r;
                if (i < IH_EMB) gW[j * IH_EMB + i] = (float)d[r];
                else if (i == IH_EMB) gb[j] = (float)d[r];
            }
            return;
        }
        t -= IW_T_W1;
        if (t < IW_T_W2) {
            const int at = t / 17, jt = t % 17;
            const int qcol0 = jt == 16 ? 2 * IH_HID
                                       : (at < 2 ? 0 : IH_HID) + jt * 16;
            iw_mfma_tile(glx, IH_LDG, at * 16, sv_h1, IH_LDH, qcol0, Rk, wave,
                         lane, part, d);
            if (wave != 0) return;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int a = at * 16 + row0 + r;
                if (a < A) {
                    if (jt < 16)
                        G.W2p[a * IH_HID + jt * 16 + col] = (float)d[r];
                    else if (col == 0) G.b2p[a] = (float)d[r];
                } else if (a == IH_AMAX) {
                    if (jt < 16) G.W2v[jt * 16 + col] = (float)d[r];
                    else if (col == 0) G.b2v[0] = (float)d[r];
                }
            }
            return;
        }
        t -= IW_T_W2;
        iw_mfma_tile(gfin, IH_LDF, IH_NODE, sv_y, IH_LDY, t * 16, Rk, wave,
                     lane, part, d);
        if (wave != 0) return;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int k = row0 + r;
            if (k < IH_GR) {
                const int f = t * 16 + col;
                if (t < 4) {
                    if (f < F) G.Wg[k * F + f] = (float)d[r];
                } else if (col == 0) {
                    G.bg[k] = (float)d[r];
                }
            }
        }
        return;
    }
    if (blockIdx.x == IW_TILES) {
        // LN grads: lane = feature, wave = chunk of the round, rows in order
        double tw = 0.0, tb = 0.0;
        for (long base = 0; base < R; base += (long)IW_WAVES * IW_CHUNK) {
            const long c0 = base + (long)wave * IW_CHUNK;
            const long c1 = c0 + IW_CHUNK < R ? c0 + IW_CHUNK : R;
            double aw = 0.0, ab = 0.0;
#pragma unroll 8
            for (long b = c0; b < c1; ++b) {
                const double gyv = (double)gy[b * IH_FMAX + lane];
                aw = fma(gyv, (double)sv_xhat[b * IH_FMAX + lane], aw);
                ab += gyv;
            }
            part[wave][lane][0] = aw;
            part[wave][lane][1] = ab;
            __syncthreads();
            if (wave == 0)
                for (int w = 0; w < IW_WAVES; ++w) {
                    tw += part[w][lane][0];
                    tb += part[w][lane][1];
                }
            __syncthreads();
        }
        if (wave == 0 && lane < F) {
            G.ln_w[lane] = (float)tw;
            G.ln_b[lane] = (float)tb;
        }
        return;
    }
    // g_model_emb of model mm: lane = (row phase q, component i)
    const int mm = blockIdx.x - IW_TILES - 1;
    const int i = lane & 15, q = lane >> 4;
    double tot = 0.0;
    for (long base = 0; base < R; base += (long)IW_WAVES * IW_CHUNK) {
        const long c0 = base + (long)wave * IW_CHUNK;
        const long c1 = c0 + IW_CHUNK < R ? c0 + IW_CHUNK : R;
        double acc = 0.0;
        for (long b = c0 + q; b < c1; b += 4)
            acc += sv_mid[b] == mm ? (double)gfin[b * IH_LDF + i] : 0.0;
        acc = ih_row_sum(acc);
        part[wave][lane][0] = acc;
        __syncthreads();
        if (wave == 0)
            for (int w = 0; w < IW_WAVES; ++w) tot += part[w][lane][0];
        __syncthreads();
    }
    if (wave == 0 && lane < IH_NODE) G.emb[mm * IH_NODE + lane] = (float)tot;
}

#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute pop
#endif

// ---------------------------------------------------------------------------
static void ih_check(const torch::Tensor& t, c10::ScalarType dt,
                     std::vector<int64_t> shape, const char* name) {
    TORCH_CHECK(t.is_cuda() && t.scalar_type() == dt && t.is_contiguous()
                && t.sizes() == c10::IntArrayRef(shape),
                "impala_head_step ", name, ": expected a contiguous CUDA ",
                c10::toString(dt), " tensor of shape ",
                c10::IntArrayRef(shape));
}

// flat [R] or [T, N]: only the element count is fixed
static void ih_check_flat(const torch::Tensor& t, c10::ScalarType dt,
                          int64_t numel, const char* name) {
    TORCH_CHECK(t.is_cuda() && t.scalar_type() == dt && t.is_contiguous()
                && t.numel() == numel,
                "impala_head_step ", name, ": expected a contiguous CUDA ",
                c10::toString(dt), " tensor of ", numel, " elements");
}

static IhHead ih_check_head(const std::vector<torch::Tensor>& h, int64_t A,
                            int64_t F) {
    TORCH_CHECK(h.size() == 12, "impala_head_step head: expected the 12 "
                "tensors of head_params(policy)");
    const auto f32 = torch::kFloat32;
    ih_check(h[0], f32, {F}, "head");
    ih_check(h[1], f32, {F}, "head");
    ih_check(h[2], f32, {IH_GR, F}, "head");
    ih_check(h[3], f32, {IH_GR}, "head");
    ih_check(h[4], f32, {IH_HID, IH_EMB}, "head");
    ih_check(h[5], f32, {IH_HID}, "head");
    ih_check(h[6], f32, {A, IH_HID}, "head");
    ih_check(h[7], f32, {A}, "head");
    ih_check(h[8], f32, {IH_HID, IH_EMB}, "head");
    ih_check(h[9], f32, {IH_HID}, "head");
    ih_check(h[10], f32, {1, IH_HID}, "head");
    ih_check(h[11], f32, {1}, "head");
    IhHead w;
    const float** p = &w.ln_w;
    for (int i = 0; i < 12; ++i) p[i] = h[i].data_ptr<float>();
    return w;
}

// Returns {loss[1], stats[5], err[1] (int32), saved...}; saved = {p, lp, h,
// values, vs, pg_adv, sv_y, sv_xhat, sv_fin, sv_h1, sv_mid, sv_act} is what
// impala_head_step_bwd takes.  With `validate` the call reads err back and
// raises on a bad model id or action; without it (no host sync) the flag is
// OR-ed into `err_acc` for the caller to read later.
std::vector<torch::Tensor> impala_head_step_fwd(
    torch::Tensor gfull, torch::Tensor model_ids, torch::Tensor actions,
    torch::Tensor behaviour_logp, torch::Tensor rewards, torch::Tensor dones,
    torch::Tensor bootstrap, torch::Tensor model_emb,
    std::vector<torch::Tensor> head, int64_t T, int64_t N, double gamma,
    double rho_clip, double pg_rho_clip, double c_clip, double vf_coeff,
    double ent_coeff, bool drop_last, c10::optional<torch::Tensor> err_acc,
    bool validate) {
    TORCH_CHECK(T >= 1 && N >= 1 && T * N < (1LL << 31),
                "impala_head_step: T*N out of range");
    TORCH_CHECK(gfull.dim() == 2, "impala_head_step: gfull must be [T*N, F]");
    const int64_t R = T * N, F = gfull.size(1), A = F - IH_GF;
    TORCH_CHECK(A >= 1 && A <= IH_AMAX, "impala_head_step needs 1 <= A <= 32,"
                " got A = ", A, " (F = 17 + A)");
    TORCH_CHECK(model_emb.dim() == 2 && model_emb.size(0) >= 1
                && model_emb.size(0) < (1LL << 24),
                "impala_head_step: model_emb must be [M, 16]");
    const int64_t M = model_emb.size(0);
    const auto f32 = torch::kFloat32, i64 = torch::kInt64;
    ih_check(gfull, f32, {R, F}, "gfull");
    ih_check_flat(model_ids, i64, R, "model_ids");
    ih_check_flat(actions, i64, R, "actions");
    ih_check_flat(behaviour_logp, f32, R, "behaviour_logp");
    ih_check_flat(rewards, f32, R, "rewards");
    ih_check_flat(dones, f32, R, "dones");
    ih_check_flat(bootstrap, f32, N, "bootstrap");
    ih_check(model_emb, f32, {M, IH_NODE}, "model_emb");
    const IhHead w = ih_check_head(head, A, F);
    int* eptr = nullptr;
    if (err_acc.has_value()) {
        ih_check(*err_acc, torch::kInt32, {1}, "err_acc");
        eptr = err_acc->data_ptr<int>();
    }
    const int64_t K = (drop_last && T > 1) ? (T - 1) * N : R;
    const int64_t tiles = (R + IH_ROWS - 1) / IH_ROWS, Rpad = tiles * IH_ROWS;
    auto opt = model_emb.options();
    auto opti = opt.dtype(torch::kInt32);
    auto p = torch::empty({Rpad, IH_AMAX}, opt);
    auto lp = torch::empty({Rpad, IH_AMAX}, opt);
    auto h = torch::empty({Rpad}, opt);
    auto logp_a = torch::empty({Rpad}, opt);
    auto ratio = torch::empty({Rpad}, opt);
    auto values = torch::empty({Rpad}, opt);
    auto vs = torch::empty({Rpad}, opt);
    auto pg = torch::empty({Rpad}, opt);
    auto sv_y = torch::empty({Rpad, IH_LDY}, opt);
    auto sv_xhat = torch::empty({Rpad, IH_FMAX}, opt);
    auto sv_fin = torch::empty({Rpad, IH_LDF}, opt);
    auto sv_h1 = torch::empty({Rpad, IH_LDH}, opt);
    auto sv_mid = torch::empty({Rpad}, opti);
    auto sv_act = torch::empty({Rpad}, opti);
    auto rowerr = torch::empty({Rpad}, opti);
    auto err = torch::empty({1}, opti);
    auto loss = torch::empty({1}, opt);
    auto stats = torch::empty({5}, opt);
    hipStream_t stream = at::cuda::getCurrentCUDAStream();
    hipLaunchKernelGGL(ihs_fwd_kernel, dim3((unsigned)tiles), dim3(IH_BLOCK),
                       0, stream, gfull.data_ptr<float>(),
                       model_ids.data_ptr<long>(), actions.data_ptr<long>(),
                       behaviour_logp.data_ptr<float>(),
                       model_emb.data_ptr<float>(), w, p.data_ptr<float>(),
                       lp.data_ptr<float>(), h.data_ptr<float>(),
                       logp_a.data_ptr<float>(), ratio.data_ptr<float>(),
                       values.data_ptr<float>(), sv_y.data_ptr<float>(),
                       sv_xhat.data_ptr<float>(), sv_fin.data_ptr<float>(),
                       sv_h1.data_ptr<float>(), sv_mid.data_ptr<int>(),
                       sv_act.data_ptr<int>(), rowerr.data_ptr<int>(),
                       (long)R, (int)A, (int)F, (int)M);
    hipLaunchKernelGGL(ihs_scan_reduce_kernel, dim3(1), dim3(IH_BLOCK), 0,
                       stream, rewards.data_ptr<float>(),
                       dones.data_ptr<float>(), values.data_ptr<float>(),
                       bootstrap.data_ptr<float>(), ratio.data_ptr<float>(),
                       logp_a.data_ptr<float>(), h.data_ptr<float>(),
                       rowerr.data_ptr<int>(), vs.data_ptr<float>(),
                       pg.data_ptr<float>(), loss.data_ptr<float>(),
                       stats.data_ptr<float>(), err.data_ptr<int>(), eptr,
                       (int)T, (int)N, (long)K, (float)gamma, (float)rho_clip,
                       (float)pg_rho_clip, (float)c_clip, (float)vf_coeff,
                       (float)ent_coeff);
    if (validate)
        TORCH_CHECK(err.item<int>() == 0, "impala_head_step: a model id is "
                    "outside [0, M) or an action outside [0, A)");
    return {loss, stats, err, p, lp, h, values, vs, pg, sv_y, sv_xhat, sv_fin,
            sv_h1, sv_mid, sv_act};
}

// saved = impala_head_step_fwd's {p, lp, h, values, vs, pg_adv, sv_y,
// sv_xhat, sv_fin, sv_h1, sv_mid, sv_act}.  Returns the gradients of
// gl * loss: the 12 head tensors in head_params order, then model_emb [M, 16].
std::vector<torch::Tensor> impala_head_step_bwd(
    std::vector<torch::Tensor> saved, std::vector<torch::Tensor> head,
    torch::Tensor gl, int64_t T, int64_t N, int64_t M, double vf_coeff,
    double ent_coeff, bool drop_last) {
    TORCH_CHECK(saved.size() == 12, "impala_head_step_bwd: saved must hold "
                "the 12 tensors impala_head_step_fwd returned");
    TORCH_CHECK(head.size() == 12 && head[0].dim() == 1,
                "impala_head_step_bwd: expected head_params(policy)");
    TORCH_CHECK(T >= 1 && N >= 1 && T * N < (1LL << 31),
                "impala_head_step_bwd: T*N out of range");
    const int64_t R = T * N, F = head[0].size(0), A = F - IH_GF;
    TORCH_CHECK(A >= 1 && A <= IH_AMAX, "impala_head_step_bwd needs A <= 32");
    TORCH_CHECK(M >= 1 && M < (1LL << 24),
                "impala_head_step_bwd: M out of range");
    const IhHead w = ih_check_head(head, A, F);
    const int64_t K = (drop_last && T > 1) ? (T - 1) * N : R;
    const int64_t tiles = (R + IH_ROWS - 1) / IH_ROWS, Rpad = tiles * IH_ROWS;
    const auto f32 = torch::kFloat32, i32 = torch::kInt32;
    ih_check(saved[0], f32, {Rpad, IH_AMAX}, "saved p");
    ih_check(saved[1], f32, {Rpad, IH_AMAX}, "saved lp");
    ih_check(saved[2], f32, {Rpad}, "saved h");
    ih_check(saved[3], f32, {Rpad}, "saved values");
    ih_check(saved[4], f32, {Rpad}, "saved vs");
    ih_check(saved[5], f32, {Rpad}, "saved pg_adv");
    ih_check(saved[6], f32, {Rpad, IH_LDY}, "saved y");
    ih_check(saved[7], f32, {Rpad, IH_FMAX}, "saved xhat");
    ih_check(saved[8], f32, {Rpad, IH_LDF}, "saved final");
    ih_check(saved[9], f32, {Rpad, IH_LDH}, "saved h1");
    ih_check(saved[10], i32, {Rpad}, "saved model ids");
    ih_check(saved[11], i32, {Rpad}, "saved actions");
    ih_check(gl, f32, {1}, "gl");
    auto opt = gl.options();
    auto glx = torch::empty({Rpad, IH_LDG}, opt);
    auto gz = torch::empty({Rpad, 2 * IH_HID}, opt);
    auto gfin = torch::empty({Rpad, IH_LDF}, opt);
    auto gy = torch::empty({Rpad, IH_FMAX}, opt);
    std::vector<torch::Tensor> grads;
    for (const auto& t : head) grads.push_back(torch::empty_like(t));
    grads.push_back(torch::empty({M, IH_NODE}, opt));
    IhGrads G;
    float** gp = &G.ln_w;
    for (int i = 0; i < 13; ++i) gp[i] = grads[i].data_ptr<float>();
    hipStream_t stream = at::cuda::getCurrentCUDAStream();
    hipLaunchKernelGGL(ihs_bwd_rows_kernel, dim3((unsigned)tiles),
                       dim3(IH_BLOCK), 0, stream, saved[0].data_ptr<float>(),
                       saved[1].data_ptr<float>(), saved[2].data_ptr<float>(),
                       saved[3].data_ptr<float>(), saved[4].data_ptr<float>(),
                       saved[5].data_ptr<float>(), saved[11].data_ptr<int>(),
                       saved[9].data_ptr<float>(), gl.data_ptr<float>(), w,
                       glx.data_ptr<float>(), gz.data_ptr<float>(),
                       gfin.data_ptr<float>(), gy.data_ptr<float>(), (long)K,
                       (int)A, (int)F, (float)vf_coeff, (float)ent_coeff);
    hipLaunchKernelGGL(ihs_bwd_wgrad_kernel,
                       dim3((unsigned)(IW_TILES + 1 + M)), dim3(IW_BLOCK), 0,
                       stream, glx.data_ptr<float>(), gz.data_ptr<float>(),
                       gfin.data_ptr<float>(), gy.data_ptr<float>(),
                       saved[6].data_ptr<float>(), saved[7].data_ptr<float>(),
                       saved[8].data_ptr<float>(), saved[9].data_ptr<float>(),
                       saved[10].data_ptr<int>(), G, (long)R, (int)A, (int)F,
                       (int)M);
    return grads;
}
