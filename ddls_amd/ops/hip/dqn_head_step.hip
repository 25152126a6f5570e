// Fused Q-head minibatch step of the DQN device learner for gfx950: the three
// head passes (online on s, online on s', target on s'), the dueling
// double-Q TD loss and the analytic backward into the 12 online head tensors
// and the per-model embeddings, reading the replay ring through `idx`.
//
// Forward, three launches:
//   dqn_hs_fwd_kernel     grid (row tiles, 2 roles), 256 threads.  Role 0
//                         stages the ONLINE head in LDS once and runs the s
//                         and the s' pass of its HS_ROWS rows; role 1 stages
//                         the TARGET head and runs the s' pass.  A pass is
//                         LN -> Linear(F,8) -> concat -> two Linear(24,256)+
//                         ReLU (thread j owns hidden unit j) -> A+1 dots of
//                         length 256 (one wave per output, lanes stride the
//                         hidden units, butterfly sum).  Role 0 also saves
//                         what the backward needs and validates the row.
//   dqn_hs_row_kernel     one wave per row, one lane per action: the row
//                         loss of dqn_row_kernel on the three passes' outputs
//   dqn_hs_reduce_kernel  one block: ordered f64 sums -> loss, stats, and
//                         the OR of the rows' validation flags
// Backward, two launches:
//   dqn_hs_bwd_rows_kernel   online head staged in LDS; per row d loss /
//                            d logits, back through both branches to the
//                            pre-activations gz [B,512], d final [B,24] and
//                            d LN-output [B,F]
//   dqn_hs_bwd_wgrad_kernel  every cross-row sum.  The weight grads are
//                            contractions over the minibatch rows and run as
//                            v_mfma_f32_16x16x4_f32 tiles, one wave per
//                            16x16 output tile, k = row index padded with
//                            zero rows to a multiple of 4; a ones column in
//                            the saved activations makes the bias grads one
//                            more column of the same tiles.  LN grads and the
//                            per-model embedding grads are one thread per
//                            output walking the rows in order.
//
// Fragment map of 16x16x4 (as meanpool_mfma.hip): A[i = lane&15][k = lane>>4],
// B[k = lane>>4][j = lane&15], D: col = lane&15, row = (lane>>4)*4 + reg.
//
// Determinism.  No atomics and no arrival counters: every sum over rows has
// one owner that adds in row order, so two calls give the same bits.
//
// Precision.  Dots accumulate in f64 from the f32 operands and are rounded
// to f32 once per stored activation; a row's loss arithmetic is f64 as in
// dqn_row_kernel.  An MFMA tile accumulates 8 k-steps (32 rows) in f32 and
// folds that partial into an f64 accumulator.
//
// Validation.  A slot outside [0, C), a model id outside [0, M) or an action
// outside [0, A) never indexes memory: the row reads slot / model 0 instead
// and raises the device flag `err`, which the host turns into an error (at
// once with validate = true, else wherever the caller reads it).
#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>
#include <cfloat>
#include <cmath>
#include <vector>

// per-lane f32 ops only: no packed f32 instructions in this file's kernels
#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

#define WAVE 64
#define WAVES 4
#define BLOCK (WAVE * WAVES)
#define HS_ROWS 4        // minibatch rows per block (forward and backward)
#define HS_HID 256
#define HS_EMB 24        // 16 node + 8 graph
#define HS_NODE 16
#define HS_GR 8
#define HS_AMAX 32
#define HS_FMAX 64
#define HS_GF 17         // graph features in front of the action mask
#define HS_HQ 40         // row stride of the head outputs: logits 0..A-1, value at 32
#define HS_LDH 528       // saved h1: h1p | h1v | ones column tile
#define HS_LDF 32        // saved final: 24 | one | zeros
#define HS_LDY 80        // saved LN output: 64 | ones column tile
#define HS_LDG 48        // d logits: 32 | d value | zeros
#define HS_LN_EPS 1e-5

typedef float f32x4_t __attribute__((ext_vector_type(4)));

struct HsHead {          // head_params(policy) order
    const float *ln_w, *ln_b, *Wg, *bg, *W1p, *b1p, *W2p, *b2p, *W1v, *b1v,
        *W2v, *b2v;
};

struct HsGrads {
    float *ln_w, *ln_b, *Wg, *bg, *W1p, *b1p, *W2p, *b2p, *W1v, *b1v, *W2v,
        *b2v, *emb;
};

// one net's head (about 88 KB at the maximal shape) plus a row's scratch
struct HsLds {
    float W1pT[HS_EMB * HS_HID];   // transposed: [i][j], lanes stride j
    float W1vT[HS_EMB * HS_HID];
    float W2p[HS_AMAX * HS_HID];
    float W2v[HS_HID];
    float Wg[HS_GR * HS_FMAX];
    float b1p[HS_HID];
    float b1v[HS_HID];
    float b2p[HS_AMAX];
    float bg[HS_GR];
    float lnw[HS_FMAX];
    float lnb[HS_FMAX];
    float b2v;
    // row scratch
    float y[HS_FMAX];              // LN output (bwd: d LN output unused)
    float lm[HS_AMAX];             // clamp(log(mask))
    float fin[HS_LDF];             // final embedding (bwd: d final)
    float h1[2 * HS_HID];          // h1p | h1v (bwd: gz)
    float gl[HS_LDG];              // bwd: d logits | d value
};

__device__ __forceinline__ double hs_wave_sum_all(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        v += __shfl_xor(v, off, WAVE);
    return v;
}

__device__ __forceinline__ double hs_wave_sum_d(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        v += __shfl_down(v, off, WAVE);
    return v;   // valid on lane 0
}

// largest value, lowest index on an exact tie; every lane gets the result
__device__ __forceinline__ void hs_wave_argmax(double& val, int& idx) {
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

// dqn_q_lane of dqn_loss.hip
__device__ __forceinline__ double hs_q_lane(float x, float v, bool in_row,
                                            bool dueling, int& nvalid) {
    const bool valid = in_row && x > -1e30f;
    nvalid = __popcll(__ballot(valid));
    if (!dueling) return (double)x;
    const double s = hs_wave_sum_all(valid ? (double)x : 0.0);
    const double mean_adv = s / (double)(nvalid > 1 ? nvalid : 1);
    return valid ? ((double)v + (double)x) - mean_adv : (double)x;
}

__device__ __forceinline__ void hs_stage(HsLds& L, const HsHead& w, int A,
                                         int F) {
    const int tid = threadIdx.x;
    for (int e = tid; e < HS_HID * HS_EMB; e += BLOCK) {
        const int j = e / HS_EMB, i = e % HS_EMB;
        L.W1pT[i * HS_HID + j] = w.W1p[e];
        L.W1vT[i * HS_HID + j] = w.W1v[e];
    }
    for (int e = tid; e < A * HS_HID; e += BLOCK) L.W2p[e] = w.W2p[e];
    for (int e = tid; e < HS_GR * F; e += BLOCK)
        L.Wg[(e / F) * HS_FMAX + e % F] = w.Wg[e];
    L.W2v[tid] = w.W2v[tid];
    L.b1p[tid] = w.b1p[tid];
    L.b1v[tid] = w.b1v[tid];
    if (tid < A) L.b2p[tid] = w.b2p[tid];
    if (tid < HS_GR) L.bg[tid] = w.bg[tid];
    if (tid < F) {
        L.lnw[tid] = w.ln_w[tid];
        L.lnb[tid] = w.ln_b[tid];
    }
    if (tid == 0) L.b2v = w.b2v[0];
    __syncthreads();
}

// One head pass of one row with the staged net.  `x` is the row's gfull [F],
// `emb` its model's embedding [16], `hq` its output row [HS_HQ].  With
// `save` the activations the backward needs go to row b of the sv_* arrays.
__device__ __forceinline__ void hs_pass(
    HsLds& L, const float* __restrict__ x, const float* __restrict__ emb,
    int A, int F, float* __restrict__ hq, bool save, long b,
    float* __restrict__ sv_y, float* __restrict__ sv_xhat,
    float* __restrict__ sv_fin, float* __restrict__ sv_h1) {
    const int tid = threadIdx.x;
    const int wave = tid / WAVE, lane = tid % WAVE;
    if (wave == 0) {
        const bool in = lane < F;
        const float xv = in ? x[lane] : 0.0f;
        const double mean = hs_wave_sum_all(in ? (double)xv : 0.0) / F;
        const double d = in ? (double)xv - mean : 0.0;
        const double var = hs_wave_sum_all(d * d) / F;
        const double xh = d / sqrt(var + HS_LN_EPS);
        const float y = in ? (float)(xh * (double)L.lnw[lane]
                                     + (double)L.lnb[lane]) : 0.0f;
        L.y[lane] = y;
        if (lane >= HS_GF && in)
            L.lm[lane - HS_GF] =
                (float)fmax(log((double)xv), -(double)FLT_MAX);
        if (save) {
            sv_y[b * HS_LDY + lane] = y;
            if (lane < 16)
                sv_y[b * HS_LDY + HS_FMAX + lane] = lane == 0 ? 1.0f : 0.0f;
            sv_xhat[b * HS_FMAX + lane] = (float)xh;
        }
    } else if (wave == 1 && lane < HS_NODE) {
        L.fin[lane] = emb[lane];
    }
    __syncthreads();
    if (wave == 0) {
        // graph embedding: 8 lanes per output, then a 3-step butterfly
        const int k = lane >> 3, part = lane & 7;
        double acc = 0.0;
        for (int f = part; f < F; f += 8)
            acc = fma((double)L.Wg[k * HS_FMAX + f], (double)L.y[f], acc);
        acc += __shfl_xor(acc, 1, WAVE);
        acc += __shfl_xor(acc, 2, WAVE);
        acc += __shfl_xor(acc, 4, WAVE);
        if (part == 0) L.fin[HS_NODE + k] = (float)(acc + (double)L.bg[k]);
    }
    __syncthreads();
    {
        double accp = (double)L.b1p[tid], accv = (double)L.b1v[tid];
#pragma unroll
        for (int i = 0; i < HS_EMB; ++i) {
            const double f = (double)L.fin[i];
            accp = fma((double)L.W1pT[i * HS_HID + tid], f, accp);
            accv = fma((double)L.W1vT[i * HS_HID + tid], f, accv);
        }
        const float hp = fmaxf((float)accp, 0.0f);
        const float hv = fmaxf((float)accv, 0.0f);
        L.h1[tid] = hp;
        L.h1[HS_HID + tid] = hv;
        if (save) {
            sv_h1[b * HS_LDH + tid] = hp;
            sv_h1[b * HS_LDH + HS_HID + tid] = hv;
            if (tid < 16)
                sv_h1[b * HS_LDH + 2 * HS_HID + tid] =
                    tid == 0 ? 1.0f : 0.0f;
            if (tid < HS_LDF)
                sv_fin[b * HS_LDF + tid] =
                    tid < HS_EMB ? L.fin[tid] : (tid == HS_EMB ? 1.0f : 0.0f);
        }
    }
    __syncthreads();
    for (int o = wave; o < A + 1; o += WAVES) {
        const float* w = o < A ? &L.W2p[o * HS_HID] : L.W2v;
        const float* h = o < A ? L.h1 : L.h1 + HS_HID;
        double acc = 0.0;
#pragma unroll
        for (int q = 0; q < HS_HID / WAVE; ++q)
            acc = fma((double)w[lane + q * WAVE], (double)h[lane + q * WAVE],
                      acc);
        acc = hs_wave_sum_d(acc);
        if (lane == 0) {
            if (o < A)
                hq[o] = (float)((acc + (double)L.b2p[o]) + (double)L.lm[o]);
            else
                hq[HS_AMAX] = (float)(acc + (double)L.b2v);
        }
    }
    __syncthreads();
}

__global__ void __launch_bounds__(BLOCK)
dqn_hs_fwd_kernel(const float* __restrict__ s_gfull,    // [C, F]
                  const long* __restrict__ s_model,     // [C]
                  const long* __restrict__ action,      // [C]
                  const float* __restrict__ n_gfull,    // [C, F]
                  const long* __restrict__ n_model,     // [C]
                  const long* __restrict__ idx,         // [B]
                  const float* __restrict__ emb_o,      // [M, 16]
                  const float* __restrict__ emb_t,      // [M, 16]
                  HsHead online, HsHead target,
                  float* __restrict__ hq,               // [3, B, HS_HQ]
                  float* __restrict__ sv_y,             // [Bpad, HS_LDY]
                  float* __restrict__ sv_xhat,          // [B, 64]
                  float* __restrict__ sv_fin,           // [Bpad, HS_LDF]
                  float* __restrict__ sv_h1,            // [Bpad, HS_LDH]
                  int* __restrict__ sv_mid,             // [B]
                  int* __restrict__ sv_act,             // [B]
                  int* __restrict__ rowerr,             // [B]
                  int B, int Bpad, int A, int F, long C, int M) {
    __shared__ HsLds L;
    const int role = blockIdx.y;
    const int tid = threadIdx.x;
    hs_stage(L, role == 0 ? online : target, A, F);
    for (int r = 0; r < HS_ROWS; ++r) {
        const long b = (long)blockIdx.x * HS_ROWS + r;
        if (b >= Bpad) break;
        if (b >= B) {
            // zero rows that pad the contractions' k to a multiple of 4
            if (role == 0) {
                for (int e = tid; e < HS_LDH; e += BLOCK)
                    sv_h1[b * HS_LDH + e] = 0.0f;
                if (tid < HS_LDY) sv_y[b * HS_LDY + tid] = 0.0f;
                if (tid < HS_LDF) sv_fin[b * HS_LDF + tid] = 0.0f;
            }
            continue;
        }
        long slot = idx[b];
        int bad = slot < 0 || slot >= C;
        if (bad) slot = 0;
        long ms = s_model[slot], mn = n_model[slot];
        if (ms < 0 || ms >= M) { bad = 1; ms = 0; }
        if (mn < 0 || mn >= M) { bad = 1; mn = 0; }
        if (role == 0) {
            long a = action[slot];
            if (a < 0 || a >= A) { bad = 1; a = 0; }
            if (tid == 0) {
                sv_mid[b] = (int)ms;
                sv_act[b] = (int)a;
                rowerr[b] = bad;
            }
            hs_pass(L, s_gfull + slot * F, emb_o + ms * HS_NODE, A, F,
                    hq + b * HS_HQ, true, b, sv_y, sv_xhat, sv_fin, sv_h1);
            hs_pass(L, n_gfull + slot * F, emb_o + mn * HS_NODE, A, F,
                    hq + ((long)B + b) * HS_HQ, false, b, sv_y, sv_xhat,
                    sv_fin, sv_h1);
        } else {
            hs_pass(L, n_gfull + slot * F, emb_t + mn * HS_NODE, A, F,
                    hq + (2 * (long)B + b) * HS_HQ, false, b, sv_y, sv_xhat,
                    sv_fin, sv_h1);
        }
    }
}

// dqn_row_kernel on the head outputs; ret / disc / has_next come from the
// ring through idx.  rows_out[b] = {huber, q_a, |td|, target}, dq_out[b] =
// clamp(td, -1, 1), both times w[b] where weights are given.
__global__ void __launch_bounds__(BLOCK)
dqn_hs_row_kernel(const float* __restrict__ hq,         // [3, B, HS_HQ]
                  const int* __restrict__ sv_act,       // [B]
                  const long* __restrict__ idx,         // [B]
                  const float* __restrict__ ret,        // [C]
                  const float* __restrict__ disc,       // [C]
                  const float* __restrict__ has_next,   // [C]
                  const float* __restrict__ weights,    // [B] or null
                  double* __restrict__ rows_out,        // [B, 4]
                  double* __restrict__ dq_out,          // [B]
                  double* __restrict__ td_abs_out,      // [B] or null
                  int B, int A, long C, double v_min, double v_max,
                  bool dueling, bool double_q) {
    const int wave = threadIdx.x / WAVE;
    const int lane = threadIdx.x % WAVE;
    const bool in_row = lane < A;
    for (int b = blockIdx.x * WAVES + wave; b < B; b += gridDim.x * WAVES) {
        long slot = idx[b];
        if (slot < 0 || slot >= C) slot = 0;
        const float* qs_row = hq + (long)b * HS_HQ;
        const float* qo_row = hq + ((long)B + b) * HS_HQ;
        const float* qt_row = hq + (2 * (long)B + b) * HS_HQ;
        int nv;
        const float xs = in_row ? qs_row[lane] : 0.0f;
        const double qs = hs_q_lane(xs, qs_row[HS_AMAX], in_row, dueling, nv);
        const double q_a = __shfl(qs, sv_act[b], WAVE);

        const float xt = in_row ? qt_row[lane] : 0.0f;
        const double qt = hs_q_lane(xt, qt_row[HS_AMAX], in_row, dueling, nv);
        double val;
        if (double_q) {
            const float xo = in_row ? qo_row[lane] : 0.0f;
            const double qo = hs_q_lane(xo, qo_row[HS_AMAX], in_row, dueling,
                                        nv);
            double best = in_row ? qo : -HUGE_VAL;
            int a_star = lane;
            hs_wave_argmax(best, a_star);
            val = __shfl(qt, a_star, WAVE);
        } else {
            val = in_row ? qt : -HUGE_VAL;
            int at_max = lane;
            hs_wave_argmax(val, at_max);
        }
        // a select: a cut transition's next state may be all finfo.min
        const double boot = (has_next[slot] != 0.0f) ? val : 0.0;
        double target = (double)ret[slot] + (double)disc[slot] * boot;
        target = fmin(fmax(target, v_min), v_max);
        const double td = q_a - target;
        const double ad = fabs(td);
        const double huber = (ad < 1.0) ? 0.5 * td * td : ad - 0.5;
        if (lane == 0) {
            const double dq = fmin(fmax(td, -1.0), 1.0);
            const double w = weights != nullptr ? (double)weights[b] : 1.0;
            rows_out[(long)b * 4 + 0] = weights != nullptr ? w * huber : huber;
            dq_out[b] = weights != nullptr ? w * dq : dq;
            rows_out[(long)b * 4 + 1] = q_a;
            rows_out[(long)b * 4 + 2] = ad;
            rows_out[(long)b * 4 + 3] = target;
            if (td_abs_out != nullptr) td_abs_out[b] = ad;
        }
    }
}

// dqn_reduce_kernel plus the OR of the rows' validation flags, which is
// also OR-ed into err_acc (a caller's flag over several steps) when given
__global__ void __launch_bounds__(BLOCK)
dqn_hs_reduce_kernel(const double* __restrict__ rows,   // [B, 4]
                     const int* __restrict__ rowerr,    // [B]
                     float* __restrict__ loss_out,      // [1]
                     float* __restrict__ stats_out,     // [4]
                     int* __restrict__ err_out,         // [1]
                     int* __restrict__ err_acc,         // [1] or null
                     int B) {
    __shared__ double part[WAVES][4];
    __shared__ int bad[WAVES];
    const int wave = threadIdx.x / WAVE;
    const int lane = threadIdx.x % WAVE;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    int e = 0;
    for (int i = threadIdx.x; i < B; i += BLOCK) {
        for (int q = 0; q < 4; ++q) s[q] += rows[(long)i * 4 + q];
        e |= rowerr[i];
    }
    for (int q = 0; q < 4; ++q) s[q] = hs_wave_sum_d(s[q]);
    const int any = __ballot(e != 0) != 0;
    if (lane == 0) {
        for (int q = 0; q < 4; ++q) part[wave][q] = s[q];
        bad[wave] = any;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t[4] = {0.0, 0.0, 0.0, 0.0};
        int eb = 0;
        for (int w = 0; w < WAVES; ++w) {
            for (int q = 0; q < 4; ++q) t[q] += part[w][q];
            eb |= bad[w];
        }
        for (int q = 0; q < 4; ++q) stats_out[q] = (float)(t[q] / B);
        loss_out[0] = (float)(t[0] / B);
        err_out[0] = eb;
        if (err_acc != nullptr) err_acc[0] |= eb;
    }
}

// Per row: d loss/d logits (dqn_loss_bwd_kernel's closed form), then back
// through W2 and the ReLUs to gz, through W1 to d final, through Wg to the
// gradient of the LN output.
__global__ void __launch_bounds__(BLOCK)
dqn_hs_bwd_rows_kernel(const float* __restrict__ hq,       // pass s rows
                       const int* __restrict__ sv_act,     // [B]
                       const double* __restrict__ dq,      // [B]
                       const float* __restrict__ gl,       // [1] upstream
                       const float* __restrict__ sv_h1,    // [Bpad, HS_LDH]
                       HsHead online,
                       float* __restrict__ glx,            // [Bpad, HS_LDG]
                       float* __restrict__ gz,             // [Bpad, 512]
                       float* __restrict__ gfin,           // [Bpad, HS_LDF]
                       float* __restrict__ gy,             // [B, 64]
                       int B, int Bpad, int A, int F, bool dueling) {
    __shared__ HsLds L;
    const int tid = threadIdx.x;
    const int wave = tid / WAVE, lane = tid % WAVE;
    hs_stage(L, online, A, F);
    const double g = (double)gl[0];
    for (int r = 0; r < HS_ROWS; ++r) {
        const long b = (long)blockIdx.x * HS_ROWS + r;
        if (b >= Bpad) break;
        if (b >= B) {
            for (int e = tid; e < 2 * HS_HID; e += BLOCK)
                gz[b * 2 * HS_HID + e] = 0.0f;
            if (tid < HS_LDG) glx[b * HS_LDG + tid] = 0.0f;
            if (tid < HS_LDF) gfin[b * HS_LDF + tid] = 0.0f;
            continue;
        }
        if (wave == 0) {
            const bool in_row = lane < A;
            const float x = in_row ? hq[b * HS_HQ + lane] : 0.0f;
            const bool valid = in_row && x > -1e30f;
            const int nvalid = __popcll(__ballot(valid));
            const int a = sv_act[b];
            const double c = g * dq[b] / (double)B;
            const double delta = (lane == a) ? 1.0 : 0.0;
            float gj = 0.0f;
            if (in_row) {
                if (dueling)
                    gj = valid ? (float)(c * (delta - 1.0 / (double)nvalid))
                               : 0.0f;
                else
                    gj = (lane == a) ? (float)c : 0.0f;
            }
            if (lane == HS_AMAX) gj = dueling ? (float)c : 0.0f;
            if (lane < HS_LDG) {
                L.gl[lane] = gj;
                glx[b * HS_LDG + lane] = gj;
            }
        }
        __syncthreads();
        {
            double acc = 0.0;
            for (int a = 0; a < A; ++a)
                acc = fma((double)L.gl[a], (double)L.W2p[a * HS_HID + tid],
                          acc);
            const float zp = sv_h1[b * HS_LDH + tid] > 0.0f
                ? (float)acc : 0.0f;
            const float zv = sv_h1[b * HS_LDH + HS_HID + tid] > 0.0f
                ? L.gl[HS_AMAX] * L.W2v[tid] : 0.0f;
            L.h1[tid] = zp;
            L.h1[HS_HID + tid] = zv;
            gz[b * 2 * HS_HID + tid] = zp;
            gz[b * 2 * HS_HID + HS_HID + tid] = zv;
        }
        __syncthreads();
        for (int o = wave; o < HS_EMB; o += WAVES) {
            double acc = 0.0;
#pragma unroll
            for (int q = 0; q < HS_HID / WAVE; ++q) {
                const int j = lane + q * WAVE;
                acc = fma((double)L.h1[j], (double)L.W1pT[o * HS_HID + j],
                          acc);
                acc = fma((double)L.h1[HS_HID + j],
                          (double)L.W1vT[o * HS_HID + j], acc);
            }
            acc = hs_wave_sum_d(acc);
            if (lane == 0) {
                L.fin[o] = (float)acc;
                gfin[b * HS_LDF + o] = (float)acc;
            }
        }
        if (tid >= HS_EMB && tid < HS_LDF) gfin[b * HS_LDF + tid] = 0.0f;
        __syncthreads();
        if (tid < HS_FMAX) {
            double acc = 0.0;
            if (tid < F) {
#pragma unroll
                for (int k = 0; k < HS_GR; ++k)
                    acc = fma((double)L.fin[HS_NODE + k],
                              (double)L.Wg[k * HS_FMAX + tid], acc);
            }
            gy[b * HS_FMAX + tid] = (float)acc;
        }
        __syncthreads();
    }
}

// D[16x16] = sum over rows k of P[k][pcol0 + i] * Q[k][qcol0 + j]: 8 k-steps
// in the f32 MFMA accumulator, then folded into f64.  out[reg] is D's row
// (lane>>4)*4 + reg, column lane&15.
__device__ __forceinline__ void hs_mfma_tile(
    const float* __restrict__ P, int ldp, int pcol0,
    const float* __restrict__ Q, int ldq, int qcol0, int Bpad, int lane,
    double out[4]) {
    const int m = lane & 15, kp = lane >> 4;
    const float* p = P + (long)kp * ldp + pcol0 + m;
    const float* q = Q + (long)kp * ldq + qcol0 + m;
    out[0] = out[1] = out[2] = out[3] = 0.0;
    int k = 0;
    for (; k + 32 <= Bpad; k += 32) {
        f32x4_t acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int s = 0; s < 32; s += 4)
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(
                p[(long)(k + s) * ldp], q[(long)(k + s) * ldq], acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) out[r] += (double)acc[r];
    }
    if (k < Bpad) {
        f32x4_t acc = {0.0f, 0.0f, 0.0f, 0.0f};
        for (; k < Bpad; k += 4)
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(
                p[(long)k * ldp], q[(long)k * ldq], acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) out[r] += (double)acc[r];
    }
}

#define HS_T_W1 64       // gz^T [512 x k] . final_ext [k x 32]
#define HS_T_W2 51       // glx^T [48 x k] . h1_ext [k x 17 tiles]
#define HS_T_WG 5        // d graph_emb^T [8(16) x k] . y_ext [k x 80]
#define HS_TILES (HS_T_W1 + HS_T_W2 + HS_T_WG)
#define HS_MFMA_BLOCKS (HS_TILES / WAVES)

__global__ void __launch_bounds__(BLOCK)
dqn_hs_bwd_wgrad_kernel(const float* __restrict__ glx,     // [Bpad, HS_LDG]
                        const float* __restrict__ gz,      // [Bpad, 512]
                        const float* __restrict__ gfin,    // [Bpad, HS_LDF]
                        const float* __restrict__ gy,      // [B, 64]
                        const float* __restrict__ sv_y,    // [Bpad, HS_LDY]
                        const float* __restrict__ sv_xhat, // [B, 64]
                        const float* __restrict__ sv_fin,  // [Bpad, HS_LDF]
                        const float* __restrict__ sv_h1,   // [Bpad, HS_LDH]
                        const int* __restrict__ sv_mid,    // [B]
                        HsGrads G, int B, int Bpad, int A, int F, int M) {
    const int tid = threadIdx.x;
    const int wave = tid / WAVE, lane = tid % WAVE;
    if (blockIdx.x < HS_MFMA_BLOCKS) {
        int t = blockIdx.x * WAVES + wave;
        const int col = lane & 15, row0 = (lane >> 4) * 4;
        double d[4];
        if (t < HS_T_W1) {
            const int jt = t >> 1, it = t & 1;
            hs_mfma_tile(gz, 2 * HS_HID, jt * 16, sv_fin, HS_LDF, it * 16,
                         Bpad, lane, d);
            const int i = it * 16 + col;
            float* gW = jt < 16 ? G.W1p : G.W1v;
            float* gb = jt < 16 ? G.b1p : G.b1v;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int j = (jt & 15) * 16 + row0 + r;
                if (i < HS_EMB) gW[j * HS_EMB + i] = (float)d[r];
                else if (i == HS_EMB) gb[j] = (float)d[r];
            }
            return;
        }
        t -= HS_T_W1;
        if (t < HS_T_W2) {
            const int at = t / 17, jt = t % 17;
            const int qcol0 = jt == 16 ? 2 * HS_HID
                                       : (at < 2 ? 0 : HS_HID) + jt * 16;
            hs_mfma_tile(glx, HS_LDG, at * 16, sv_h1, HS_LDH, qcol0, Bpad,
                         lane, d);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int a = at * 16 + row0 + r;
                if (a < A) {
                    if (jt < 16) G.W2p[a * HS_HID + jt * 16 + col] = (float)d[r];
                    else if (col == 0) G.b2p[a] = (float)d[r];
                } else if (a == HS_AMAX) {
                    if (jt < 16) G.W2v[jt * 16 + col] = (float)d[r];
                    else if (col == 0) G.b2v[0] = (float)d[r];
                }
            }
            return;
        }
        t -= HS_T_W2;
        hs_mfma_tile(gfin, HS_LDF, HS_NODE, sv_y, HS_LDY, t * 16, Bpad, lane,
                     d);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int k = row0 + r;
            if (k < HS_GR) {
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
    // one thread per output, rows in order
    const int v = (blockIdx.x - HS_MFMA_BLOCKS) * BLOCK + tid;
    if (v < 2 * HS_FMAX) {
        const int f = v & (HS_FMAX - 1);
        if (f >= F) return;
        double acc = 0.0;
        if (v < HS_FMAX) {
#pragma unroll 8
            for (int b = 0; b < B; ++b)
                acc = fma((double)gy[(long)b * HS_FMAX + f],
                          (double)sv_xhat[(long)b * HS_FMAX + f], acc);
            G.ln_w[f] = (float)acc;
        } else {
#pragma unroll 8
            for (int b = 0; b < B; ++b) acc += (double)gy[(long)b * HS_FMAX + f];
            G.ln_b[f] = (float)acc;
        }
        return;
    }
    const int e = v - 2 * HS_FMAX;
    if (e < M * HS_NODE) {
        const int m = e / HS_NODE, i = e % HS_NODE;
        double acc = 0.0;
#pragma unroll 8
        for (int b = 0; b < B; ++b)
            acc += sv_mid[b] == m ? (double)gfin[(long)b * HS_LDF + i] : 0.0;
        G.emb[e] = (float)acc;
    }
}

#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute pop
#endif

// ---------------------------------------------------------------------------
static void hs_check(const torch::Tensor& t, c10::ScalarType dt,
                     std::vector<int64_t> shape, const char* name) {
    TORCH_CHECK(t.is_cuda() && t.scalar_type() == dt && t.is_contiguous()
                && t.sizes() == c10::IntArrayRef(shape),
                "dqn_head_step ", name, ": expected a contiguous CUDA ",
                c10::toString(dt), " tensor of shape ",
                c10::IntArrayRef(shape));
}

static HsHead hs_check_head(const std::vector<torch::Tensor>& h, int64_t A,
                            int64_t F, const char* name) {
    TORCH_CHECK(h.size() == 12, "dqn_head_step ", name,
                ": expected the 12 tensors of head_params(policy)");
    const auto f32 = torch::kFloat32;
    hs_check(h[0], f32, {F}, name);
    hs_check(h[1], f32, {F}, name);
    hs_check(h[2], f32, {HS_GR, F}, name);
    hs_check(h[3], f32, {HS_GR}, name);
    hs_check(h[4], f32, {HS_HID, HS_EMB}, name);
    hs_check(h[5], f32, {HS_HID}, name);
    hs_check(h[6], f32, {A, HS_HID}, name);
    hs_check(h[7], f32, {A}, name);
    hs_check(h[8], f32, {HS_HID, HS_EMB}, name);
    hs_check(h[9], f32, {HS_HID}, name);
    hs_check(h[10], f32, {1, HS_HID}, name);
    hs_check(h[11], f32, {1}, name);
    HsHead w;
    const float** p = &w.ln_w;
    for (int i = 0; i < 12; ++i) p[i] = h[i].data_ptr<float>();
    return w;
}

static int hs_row_blocks(int64_t R) {
    int64_t blocks = (R + WAVES - 1) / WAVES;
    return (int)(blocks > 1024 ? 1024 : blocks);
}

// ring = {s_gfull, s_model, action, ret, disc, has_next, n_gfull, n_model}.
// Returns {loss[1], stats[4], err[1] (int32), saved...} and, with weights,
// td_abs[B] (f64) at the end.  saved = {hq, dq, sv_y, sv_xhat, sv_fin,
// sv_h1, sv_mid, sv_act} is what dqn_head_step_bwd takes.  With `validate`
// the call reads err back and raises on a bad slot, model id or action;
// without it (no host sync) the flag is OR-ed into `err_acc` for the caller
// to read later.
std::vector<torch::Tensor> dqn_head_step_fwd(
    std::vector<torch::Tensor> ring, torch::Tensor idx,
    torch::Tensor model_emb, torch::Tensor target_emb,
    std::vector<torch::Tensor> online, std::vector<torch::Tensor> target,
    double v_min, double v_max, bool dueling, bool double_q,
    c10::optional<torch::Tensor> weights,
    c10::optional<torch::Tensor> err_acc, bool validate) {
    TORCH_CHECK(ring.size() == 8, "dqn_head_step: ring must hold 8 tensors");
    TORCH_CHECK(ring[0].dim() == 2, "dqn_head_step: s_gfull must be [C, F]");
    const int64_t C = ring[0].size(0), F = ring[0].size(1), A = F - HS_GF;
    TORCH_CHECK(A >= 1 && A <= HS_AMAX, "dqn_head_step needs 1 <= A <= 32, "
                "got A = ", A, " (F = 17 + A)");
    TORCH_CHECK(C >= 1, "dqn_head_step: empty ring");
    TORCH_CHECK(idx.dim() == 1 && idx.size(0) >= 1
                && idx.size(0) < (1LL << 24),
                "dqn_head_step: idx must be [B] with 1 <= B < 2^24");
    const int64_t B = idx.size(0), Bpad = (B + 3) / 4 * 4;
    TORCH_CHECK(model_emb.dim() == 2 && model_emb.size(0) >= 1
                && model_emb.size(0) < (1LL << 24),
                "dqn_head_step: model_emb must be [M, 16]");
    const int64_t M = model_emb.size(0);
    const auto f32 = torch::kFloat32, i64 = torch::kInt64;
    hs_check(ring[0], f32, {C, F}, "s_gfull");
    hs_check(ring[1], i64, {C}, "s_model");
    hs_check(ring[2], i64, {C}, "action");
    hs_check(ring[3], f32, {C}, "ret");
    hs_check(ring[4], f32, {C}, "disc");
    hs_check(ring[5], f32, {C}, "has_next");
    hs_check(ring[6], f32, {C, F}, "n_gfull");
    hs_check(ring[7], i64, {C}, "n_model");
    hs_check(idx, i64, {B}, "idx");
    hs_check(model_emb, f32, {M, HS_NODE}, "model_emb");
    hs_check(target_emb, f32, {M, HS_NODE}, "target_emb");
    const HsHead wo = hs_check_head(online, A, F, "online head");
    const HsHead wt = hs_check_head(target, A, F, "target head");
    const float* wptr = nullptr;
    if (weights.has_value()) {
        hs_check(*weights, f32, {B}, "weights");
        wptr = weights->data_ptr<float>();
    }
    int* eptr = nullptr;
    if (err_acc.has_value()) {
        hs_check(*err_acc, torch::kInt32, {1}, "err_acc");
        eptr = err_acc->data_ptr<int>();
    }
    auto opt = model_emb.options();
    auto opt64 = opt.dtype(torch::kFloat64);
    auto opti = opt.dtype(torch::kInt32);
    auto hq = torch::empty({3, B, HS_HQ}, opt);
    auto sv_y = torch::empty({Bpad, HS_LDY}, opt);
    auto sv_xhat = torch::empty({B, HS_FMAX}, opt);
    auto sv_fin = torch::empty({Bpad, HS_LDF}, opt);
    auto sv_h1 = torch::empty({Bpad, HS_LDH}, opt);
    auto sv_mid = torch::empty({B}, opti);
    auto sv_act = torch::empty({B}, opti);
    auto rowerr = torch::empty({B}, opti);
    auto err = torch::empty({1}, opti);
    auto rows = torch::empty({B, 4}, opt64);
    auto dq = torch::empty({B}, opt64);
    auto loss = torch::empty({1}, opt);
    auto stats = torch::empty({4}, opt);
    torch::Tensor td_abs;
    if (wptr != nullptr) td_abs = torch::empty({B}, opt64);
    hipStream_t stream = at::cuda::getCurrentCUDAStream();
    const int tiles = (int)((Bpad + HS_ROWS - 1) / HS_ROWS);
    hipLaunchKernelGGL(dqn_hs_fwd_kernel, dim3(tiles, 2), dim3(BLOCK), 0,
                       stream, ring[0].data_ptr<float>(),
                       ring[1].data_ptr<long>(), ring[2].data_ptr<long>(),
                       ring[6].data_ptr<float>(), ring[7].data_ptr<long>(),
                       idx.data_ptr<long>(), model_emb.data_ptr<float>(),
                       target_emb.data_ptr<float>(), wo, wt,
                       hq.data_ptr<float>(), sv_y.data_ptr<float>(),
                       sv_xhat.data_ptr<float>(), sv_fin.data_ptr<float>(),
                       sv_h1.data_ptr<float>(), sv_mid.data_ptr<int>(),
                       sv_act.data_ptr<int>(), rowerr.data_ptr<int>(),
                       (int)B, (int)Bpad, (int)A, (int)F, (long)C, (int)M);
    hipLaunchKernelGGL(dqn_hs_row_kernel, dim3(hs_row_blocks(B)), dim3(BLOCK),
                       0, stream, hq.data_ptr<float>(),
                       sv_act.data_ptr<int>(), idx.data_ptr<long>(),
                       ring[3].data_ptr<float>(), ring[4].data_ptr<float>(),
                       ring[5].data_ptr<float>(), wptr,
                       rows.data_ptr<double>(), dq.data_ptr<double>(),
                       wptr != nullptr ? td_abs.data_ptr<double>()
                                       : (double*)nullptr,
                       (int)B, (int)A, (long)C, v_min, v_max, dueling,
                       double_q);
    hipLaunchKernelGGL(dqn_hs_reduce_kernel, dim3(1), dim3(BLOCK), 0, stream,
                       rows.data_ptr<double>(), rowerr.data_ptr<int>(),
                       loss.data_ptr<float>(), stats.data_ptr<float>(),
                       err.data_ptr<int>(), eptr, (int)B);
    if (validate)
        TORCH_CHECK(err.item<int>() == 0, "dqn_head_step: an idx entry is "
                    "outside [0, C), a model id outside [0, M) or an action "
                    "outside [0, A)");
    std::vector<torch::Tensor> out = {loss, stats, err, hq, dq, sv_y, sv_xhat,
                                      sv_fin, sv_h1, sv_mid, sv_act};
    if (wptr != nullptr) out.push_back(td_abs);
    return out;
}

// saved = dqn_head_step_fwd's {hq, dq, sv_y, sv_xhat, sv_fin, sv_h1, sv_mid,
// sv_act}.  Returns the gradients of gl * loss: the 12 online head tensors in
// head_params order, then model_emb [M, 16].
std::vector<torch::Tensor> dqn_head_step_bwd(
    std::vector<torch::Tensor> saved, std::vector<torch::Tensor> online,
    torch::Tensor gl, int64_t M, bool dueling) {
    TORCH_CHECK(saved.size() == 8, "dqn_head_step_bwd: saved must hold the 8 "
                "tensors dqn_head_step_fwd returned");
    TORCH_CHECK(online.size() == 12 && online[0].dim() == 1,
                "dqn_head_step_bwd: expected head_params(policy)");
    TORCH_CHECK(saved[1].dim() == 1 && saved[1].size(0) >= 1,
                "dqn_head_step_bwd: dq must be [B]");
    const int64_t F = online[0].size(0), A = F - HS_GF, B = saved[1].size(0);
    const int64_t Bpad = (B + 3) / 4 * 4;
    TORCH_CHECK(A >= 1 && A <= HS_AMAX, "dqn_head_step_bwd needs A <= 32");
    TORCH_CHECK(M >= 1 && M < (1LL << 24), "dqn_head_step_bwd: M out of range");
    const HsHead wo = hs_check_head(online, A, F, "online head");
    const auto f32 = torch::kFloat32, i32 = torch::kInt32;
    hs_check(saved[0], f32, {3, B, HS_HQ}, "saved hq");
    hs_check(saved[1], torch::kFloat64, {B}, "saved dq");
    hs_check(saved[2], f32, {Bpad, HS_LDY}, "saved y");
    hs_check(saved[3], f32, {B, HS_FMAX}, "saved xhat");
    hs_check(saved[4], f32, {Bpad, HS_LDF}, "saved final");
    hs_check(saved[5], f32, {Bpad, HS_LDH}, "saved h1");
    hs_check(saved[6], i32, {B}, "saved model ids");
    hs_check(saved[7], i32, {B}, "saved actions");
    hs_check(gl, f32, {1}, "gl");
    auto opt = gl.options();
    auto glx = torch::empty({Bpad, HS_LDG}, opt);
    auto gz = torch::empty({Bpad, 2 * HS_HID}, opt);
    auto gfin = torch::empty({Bpad, HS_LDF}, opt);
    auto gy = torch::empty({B, HS_FMAX}, opt);
    std::vector<torch::Tensor> grads;
    for (const auto& t : online) grads.push_back(torch::empty_like(t));
    grads.push_back(torch::empty({M, HS_NODE}, opt));
    HsGrads G;
    float** p = &G.ln_w;
    for (int i = 0; i < 13; ++i) p[i] = grads[i].data_ptr<float>();
    hipStream_t stream = at::cuda::getCurrentCUDAStream();
    const int tiles = (int)((Bpad + HS_ROWS - 1) / HS_ROWS);
    hipLaunchKernelGGL(dqn_hs_bwd_rows_kernel, dim3(tiles), dim3(BLOCK), 0,
                       stream, saved[0].data_ptr<float>(),
                       saved[7].data_ptr<int>(), saved[1].data_ptr<double>(),
                       gl.data_ptr<float>(), saved[5].data_ptr<float>(), wo,
                       glx.data_ptr<float>(), gz.data_ptr<float>(),
                       gfin.data_ptr<float>(), gy.data_ptr<float>(), (int)B,
                       (int)Bpad, (int)A, (int)F, dueling);
    const int valu = (int)((2 * HS_FMAX + M * HS_NODE + BLOCK - 1) / BLOCK);
    hipLaunchKernelGGL(dqn_hs_bwd_wgrad_kernel, dim3(HS_MFMA_BLOCKS + valu),
                       dim3(BLOCK), 0, stream, glx.data_ptr<float>(),
                       gz.data_ptr<float>(), gfin.data_ptr<float>(),
                       gy.data_ptr<float>(), saved[2].data_ptr<float>(),
                       saved[3].data_ptr<float>(), saved[4].data_ptr<float>(),
                       saved[5].data_ptr<float>(), saved[6].data_ptr<int>(),
                       G, (int)B, (int)Bpad, (int)A, (int)F, (int)M);
    return grads;
}
