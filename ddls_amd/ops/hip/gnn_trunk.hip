// The GNN trunk of the tuned PAC-ML policy for gfx950, forward and analytic
// backward without autograd: MeanPoolLayer.forward twice, then graph_mean
// (models/gnn.py), on a flat batch of G graphs.  Built for the device DQN
// learner, whose models batch is a handful of small static graphs: the cost
// there is the launch count, so the trunk is three launches per minibatch.
//
// The tuned shape only, every dim a compile-time constant: two rounds,
// module_depth 1, ReLU, node features 5, edge features 2, message 32
// (16 + 16), hidden 64, node output 16.
//
//   gt_fwd_kernel        grid = G, one workgroup per graph (every dependency
//                        between rows stays inside one graph).  The block
//                        stages all 24 parameter tensors in LDS once, the W
//                        matrices transposed ([k][j], so consecutive lanes =
//                        consecutive outputs j read consecutive banks), then
//                        walks the phases with block barriers only:
//                          1 LayerNorm of the node rows and the edge rows
//                          2 node / edge Linear + ReLU            -> hn, he
//                          3 gather hn[src] || he, LayerNorm over 32
//                          4 reduce Linear + ReLU per message     -> r
//                          5 segment mean per destination node    -> z
//                        for round 1 (5 -> 16, 32 -> 64) and round 2
//                        (64 -> 16, 32 -> 16), then the graph mean.
//   gt_bwd_rows_kernel   grid = G, weights staged untransposed ([j][k]: the
//                        backward contracts over the outputs j and lanes run
//                        along k).  From g_model_emb[g] down the same phases;
//                        stores the pre-activation gradients gz of all six
//                        modules and the gradients gy of their LayerNorm
//                        outputs.  The hn[src] scatter is a gather over a
//                        CSR-by-src list in a fixed order.
//   gt_bwd_wgrad_kernel  every cross-row sum.  The three K >= 32 weight grads
//                        (both reduce modules, the round-2 node module) are
//                        v_mfma_f32_16x16x4_f32 tiles, one wave per 16x16
//                        output tile, k = row index, a ones column for the
//                        bias; the K = 5 / K = 2 modules and the twelve
//                        LayerNorm grads are one thread per output walking
//                        the rows in order in f64.
//
// Row order.  Edges are addressed by their position p in the CSR-by-dst order
// (plan `eo[p]` is the edge id): a graph's positions and a node's in-edges
// are then contiguous ranges.  Message row m is p for an edge message and
// E + v for node v's self message.
//
// Activations live in a global workspace (returned to the caller, read again
// by the backward), so a graph's size is not bounded by LDS; rows are walked
// with block-stride loops, and a block re-reads only rows of its own graph
// after a barrier.
//
// Fragment map of 16x16x4 (as meanpool_mfma.hip): A[i = lane&15][k = lane>>4],
// B[k = lane>>4][j = lane&15], D: col = lane&15, row = (lane>>4)*4 + reg.
//
// Determinism.  No atomics, no arrival counters: every sum has one owner that
// adds in a fixed order, so two calls give the same bits.
//
// Precision.  Row dots and LayerNorm statistics accumulate in f64 from the
// f32 operands and round to f32 once per stored activation.  An MFMA tile
// accumulates 8 k-steps (32 rows) in f32 and folds that partial into f64.
#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>
#include <algorithm>
#include <cmath>
#include <vector>

// per-lane f32 ops only: no packed f32 instructions in this file's kernels
#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

#define GT_WAVE 64
#define GT_BLOCK 512          // forward and backward-rows workgroup
#define GT_WG_BLOCK 256       // wgrad workgroup: 4 waves, one tile each
#define GT_HALF 16
#define GT_MSG 32
#define GT_FE 2
#define GT_LN_EPS 1e-5

typedef float f32x4_t __attribute__((ext_vector_type(4)));

// Offsets of one MeanPool layer's 12 tensors in gnn.parameters() order.
template <int FN_, int OUT_, int BASE>
struct GtLay {
    static constexpr int FN = FN_, OUT = OUT_;
    static constexpr int n_lnw = BASE, n_lnb = n_lnw + FN, n_W = n_lnb + FN,
                         n_b = n_W + GT_HALF * FN, e_lnw = n_b + GT_HALF,
                         e_lnb = e_lnw + GT_FE, e_W = e_lnb + GT_FE,
                         e_b = e_W + GT_HALF * GT_FE, r_lnw = e_b + GT_HALF,
                         r_lnb = r_lnw + GT_MSG, r_W = r_lnb + GT_MSG,
                         r_b = r_W + OUT * GT_MSG, end = r_b + OUT;
};
typedef GtLay<5, 64, 0> GtL1;
typedef GtLay<64, 16, GtL1::end> GtL2;
#define GT_NP (GtL2::end)     // 4146 floats
static_assert(GtL1::end == 2334 && GT_NP == 4146, "tuned GNN shape");

struct GtParams { const float* p[24]; };

// int32 index plan of the static batch (GraphBatch.trunk_plan)
struct GtPlan {
    const int* eo;        // [E] edge id at CSR-by-dst position p
    const int* srcp;      // [E] source node of position p
    const int* dstp;      // [E] destination node of position p
    const int* indptr;    // [N+1] positions of a node's in-edges
    const int* sptr;      // [N+1] CSR by source ...
    const int* slist;     // [E]   ... of positions, ascending per node
    const int* node_ptr;  // [G+1]
};

// forward workspace: what the backward reads again
struct GtWs {
    float *xn1, *xe1, *hn1, *he1, *mh1, *rs1, *r1, *z1;
    float *xn2, *rsn2, *xe2, *hn2, *he2, *mh2, *rs2, *r2, *z2;
};

// backward scratch: gz / gy of the six modules (read by the wgrad kernel)
struct GtBs {
    float *gup2, *gzr2, *gyr2, *gm2, *gzn2, *gze2, *gyn2, *gye2;
    float *gup1, *gzr1, *gyr1, *gm1, *gzn1, *gze1, *gyn1, *gye1;
};

// ---------------------------------------------------------------------------
// staging: all 24 tensors into one flat LDS array at their GtLay offsets
__device__ __forceinline__ void gt_copy(float* dst, const float* __restrict__ src,
                                        int n) {
    for (int i = threadIdx.x; i < n; i += blockDim.x) dst[i] = src[i];
}

// W is torch-layout [rows][cols]; transposed it lands as [cols][rows]
template <bool TRANSPOSE>
__device__ __forceinline__ void gt_copy_w(float* dst,
                                          const float* __restrict__ src,
                                          int rows, int cols) {
    for (int i = threadIdx.x; i < rows * cols; i += blockDim.x) {
        if (TRANSPOSE) dst[(i % cols) * rows + i / cols] = src[i];
        else dst[i] = src[i];
    }
}

template <class L, bool TRANSPOSE>
__device__ __forceinline__ void gt_stage_layer(float* P, const GtParams& w,
                                               int t0) {
    gt_copy(P + L::n_lnw, w.p[t0 + 0], L::FN);
    gt_copy(P + L::n_lnb, w.p[t0 + 1], L::FN);
    gt_copy_w<TRANSPOSE>(P + L::n_W, w.p[t0 + 2], GT_HALF, L::FN);
    gt_copy(P + L::n_b, w.p[t0 + 3], GT_HALF);
    gt_copy(P + L::e_lnw, w.p[t0 + 4], GT_FE);
    gt_copy(P + L::e_lnb, w.p[t0 + 5], GT_FE);
    gt_copy_w<TRANSPOSE>(P + L::e_W, w.p[t0 + 6], GT_HALF, GT_FE);
    gt_copy(P + L::e_b, w.p[t0 + 7], GT_HALF);
    gt_copy(P + L::r_lnw, w.p[t0 + 8], GT_MSG);
    gt_copy(P + L::r_lnb, w.p[t0 + 9], GT_MSG);
    gt_copy_w<TRANSPOSE>(P + L::r_W, w.p[t0 + 10], L::OUT, GT_MSG);
    gt_copy(P + L::r_b, w.p[t0 + 11], L::OUT);
}

// ---------------------------------------------------------------------------
// forward pieces
//
// LayerNorm statistics of one row, one thread: xh = (x - mean) * rstd.
template <int K>
__device__ __forceinline__ void gt_ln_row(const float* x, float* xh,
                                          float* rs) {
    double s = 0.0;
#pragma unroll 8
    for (int k = 0; k < K; ++k) s += (double)x[k];
    const double mean = s / K;
    double v = 0.0;
#pragma unroll 8
    for (int k = 0; k < K; ++k) {
        const double d = (double)x[k] - mean;
        v = fma(d, d, v);
    }
    const double rstd = 1.0 / sqrt(v / K + GT_LN_EPS);
#pragma unroll 8
    for (int k = 0; k < K; ++k) xh[k] = (float)(((double)x[k] - mean) * rstd);
    if (rs != nullptr) rs[0] = (float)rstd;
}

// relu(sum_k (xh[k] * lnw[k] + lnb[k]) * WT[k][j] + b[j]), WT in LDS
template <int K>
__device__ __forceinline__ float gt_lin_relu(const float* xh, const float* lnw,
                                             const float* lnb, const float* WT,
                                             int ldw, int j, float bias) {
    double acc = (double)bias;
#pragma unroll 8
    for (int k = 0; k < K; ++k) {
        const double y = fma((double)xh[k], (double)lnw[k], (double)lnb[k]);
        acc = fma((double)WT[k * ldw + j], y, acc);
    }
    return fmaxf((float)acc, 0.0f);
}

// One MeanPool round of graph rows [n0, n1) / positions [e0, e1).  `x` is the
// round's node input [N, FN] (batch.z, or z1 in the workspace).
template <class L>
__device__ __forceinline__ void gt_round_fwd(
    const float* P, const float* x, const float* __restrict__ e,
    const GtPlan& pl, int n0, int n1, int e0, int e1, int E, float* xn,
    float* rsn, float* xe, float* hn, float* he, float* mh, float* rs,
    float* r, float* z) {
    constexpr int FN = L::FN, OUT = L::OUT;
    const int tid = threadIdx.x;
    const int Ng = n1 - n0, Eg = e1 - e0, Mg = Ng + Eg;
    // 1: LayerNorm statistics, one thread per node row / edge row
    for (int t = tid; t < Mg; t += GT_BLOCK) {
        if (t < Ng) {
            const long v = n0 + t;
            gt_ln_row<FN>(x + v * FN, xn + v * FN,
                          rsn != nullptr ? rsn + v : nullptr);
        } else {
            const long p = e0 + (t - Ng);
            gt_ln_row<GT_FE>(e + (long)pl.eo[p] * GT_FE, xe + p * GT_FE,
                             nullptr);
        }
    }
    __syncthreads();
    // 2: node and edge Linear + ReLU, one thread per (row, output)
    for (int t = tid; t < Mg * GT_HALF; t += GT_BLOCK) {
        const int row = t / GT_HALF, j = t % GT_HALF;
        if (row < Ng) {
            const long v = n0 + row;
            hn[v * GT_HALF + j] = gt_lin_relu<FN>(
                xn + v * FN, P + L::n_lnw, P + L::n_lnb, P + L::n_W, GT_HALF,
                j, P[L::n_b + j]);
        } else {
            const long p = e0 + (row - Ng);
            he[p * GT_HALF + j] = gt_lin_relu<GT_FE>(
                xe + p * GT_FE, P + L::e_lnw, P + L::e_lnb, P + L::e_W,
                GT_HALF, j, P[L::e_b + j]);
        }
    }
    __syncthreads();
    // 3: message rows hn[src] || he (self: hn[v] || 0), LayerNorm over 32
    for (int t = tid; t < Mg; t += GT_BLOCK) {
        const bool is_edge = t < Eg;
        const long p = e0 + t;                         // edge rows only
        const long node = is_edge ? pl.srcp[p] : n0 + (t - Eg);
        const long m = is_edge ? p : (long)E + node;
        const float* a = hn + node * GT_HALF;
        const float* b = he + (is_edge ? p : 0) * GT_HALF;
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < GT_HALF; ++k) {
            s += (double)a[k];
            if (is_edge) s += (double)b[k];
        }
        const double mean = s / GT_MSG;
        double var = 0.0;
#pragma unroll
        for (int k = 0; k < GT_HALF; ++k) {
            const double da = (double)a[k] - mean;
            const double db = (is_edge ? (double)b[k] : 0.0) - mean;
            var = fma(da, da, var);
            var = fma(db, db, var);
        }
        const double rstd = 1.0 / sqrt(var / GT_MSG + GT_LN_EPS);
#pragma unroll
        for (int k = 0; k < GT_HALF; ++k) {
            mh[m * GT_MSG + k] = (float)(((double)a[k] - mean) * rstd);
            mh[m * GT_MSG + GT_HALF + k] =
                (float)(((is_edge ? (double)b[k] : 0.0) - mean) * rstd);
        }
        rs[m] = (float)rstd;
    }
    __syncthreads();
    // 4: reduce Linear + ReLU, one thread per (message, output)
    for (int t = tid; t < Mg * OUT; t += GT_BLOCK) {
        const int row = t / OUT, j = t % OUT;
        const long m = row < Eg ? (long)e0 + row : (long)E + n0 + (row - Eg);
        r[m * OUT + j] = gt_lin_relu<GT_MSG>(
            mh + m * GT_MSG, P + L::r_lnw, P + L::r_lnb, P + L::r_W, OUT, j,
            P[L::r_b + j]);
    }
    __syncthreads();
    // 5: mean over a node's mail and its self message; no mail -> zeros
    for (int t = tid; t < Ng * OUT; t += GT_BLOCK) {
        const long v = n0 + t / OUT;
        const int j = t % OUT;
        const int pb = pl.indptr[v], pe = pl.indptr[v + 1];
        float out = 0.0f;
        if (pe > pb) {
            double acc = (double)r[((long)E + v) * OUT + j];
            for (long p = pb; p < pe; ++p) acc += (double)r[p * OUT + j];
            out = (float)(acc / (double)(pe - pb + 1));
        }
        z[v * OUT + j] = out;
    }
    __syncthreads();
}

__global__ void __launch_bounds__(GT_BLOCK)
gt_fwd_kernel(const float* __restrict__ z0,      // [N, 5]
              const float* __restrict__ e,       // [E, 2]
              GtPlan pl, GtParams w, GtWs ws,
              float* __restrict__ emb,           // [G, 16]
              int E) {
    __shared__ float P[GT_NP];
    __shared__ double part[GT_BLOCK / GT_HALF][GT_HALF];
    gt_stage_layer<GtL1, true>(P, w, 0);
    gt_stage_layer<GtL2, true>(P, w, 12);
    __syncthreads();
    const int g = blockIdx.x;
    const int n0 = pl.node_ptr[g], n1 = pl.node_ptr[g + 1];
    const int e0 = pl.indptr[n0], e1 = pl.indptr[n1];
    gt_round_fwd<GtL1>(P, z0, e, pl, n0, n1, e0, e1, E, ws.xn1, nullptr,
                       ws.xe1, ws.hn1, ws.he1, ws.mh1, ws.rs1, ws.r1, ws.z1);
    gt_round_fwd<GtL2>(P, ws.z1, e, pl, n0, n1, e0, e1, E, ws.xn2, ws.rsn2,
                       ws.xe2, ws.hn2, ws.he2, ws.mh2, ws.rs2, ws.r2, ws.z2);
    // graph mean: 32 row groups x 16 features, partials summed in order
    const int j = threadIdx.x % GT_HALF, grp = threadIdx.x / GT_HALF;
    double acc = 0.0;
    for (long v = n0 + grp; v < n1; v += GT_BLOCK / GT_HALF)
        acc += (double)ws.z2[v * GT_HALF + j];
    part[grp][j] = acc;
    __syncthreads();
    if (threadIdx.x < GT_HALF) {
        double s = 0.0;
#pragma unroll
        for (int q = 0; q < GT_BLOCK / GT_HALF; ++q) s += part[q][threadIdx.x];
        emb[g * GT_HALF + threadIdx.x] =
            n1 > n0 ? (float)(s / (double)(n1 - n0)) : 0.0f;
    }
}

// ---------------------------------------------------------------------------
// backward pieces
//
// LayerNorm backward of one row, one thread: gy is the gradient of the LN
// output; out(k, value) receives d/dx[k].  Two passes, nothing kept per k.
template <int K, class Out>
__device__ __forceinline__ void gt_ln_bwd_row(const float* gy, const float* xh,
                                              const float* lnw, double rstd,
                                              Out out) {
    double s1 = 0.0, s2 = 0.0;
#pragma unroll 8
    for (int k = 0; k < K; ++k) {
        const double g = (double)gy[k] * (double)lnw[k];
        s1 += g;
        s2 = fma(g, (double)xh[k], s2);
    }
    const double m1 = s1 / K, m2 = s2 / K;
#pragma unroll 8
    for (int k = 0; k < K; ++k) {
        const double g = (double)gy[k] * (double)lnw[k];
        out(k, (float)(rstd * (g - m1 - (double)xh[k] * m2)));
    }
}

// One MeanPool round backwards.  gup [N, OUT] is the gradient of the round's
// output rows; with INGRAD the gradient of its node input goes to gin.
template <class L, bool INGRAD>
__device__ __forceinline__ void gt_round_bwd(
    const float* P, const GtPlan& pl, int n0, int n1, int e0, int e1, int E,
    const float* gup, const float* xn, const float* rsn, const float* hn,
    const float* he, const float* mh, const float* rs, const float* r,
    float* gzr, float* gyr, float* gm, float* gzn, float* gze, float* gyn,
    float* gye, float* gin) {
    constexpr int FN = L::FN, OUT = L::OUT;
    const int tid = threadIdx.x;
    const int Ng = n1 - n0, Eg = e1 - e0, Mg = Ng + Eg;
    // segment mean and the ReLU gate of the reduce module
    for (int t = tid; t < Mg * OUT; t += GT_BLOCK) {
        const int row = t / OUT, j = t % OUT;
        const bool is_edge = row < Eg;
        const long p = e0 + row;
        const long d = is_edge ? pl.dstp[p] : n0 + (row - Eg);
        const long m = is_edge ? p : (long)E + d;
        const int deg = pl.indptr[d + 1] - pl.indptr[d];
        float val = 0.0f;
        if (deg > 0 && r[m * OUT + j] > 0.0f)
            val = (float)((double)gup[d * OUT + j] / (double)(deg + 1));
        gzr[m * OUT + j] = val;
    }
    __syncthreads();
    // gradient of the reduce module's LN output: gz . W, W natural in LDS
    for (int t = tid; t < Mg * GT_MSG; t += GT_BLOCK) {
        const int row = t / GT_MSG, k = t % GT_MSG;
        const long m = row < Eg ? (long)e0 + row : (long)E + n0 + (row - Eg);
        double acc = 0.0;
#pragma unroll 8
        for (int j = 0; j < OUT; ++j)
            acc = fma((double)gzr[m * OUT + j],
                      (double)P[L::r_W + j * GT_MSG + k], acc);
        gyr[m * GT_MSG + k] = (float)acc;
    }
    __syncthreads();
    // LN backward per message; split: the first 16 wait for the gather by
    // source (gm), the last 16 are the edge module's output gradient, gated
    for (int t = tid; t < Mg; t += GT_BLOCK) {
        const bool is_edge = t < Eg;
        const long p = e0 + t;
        const long m = is_edge ? p : (long)E + n0 + (t - Eg);
        gt_ln_bwd_row<GT_MSG>(
            gyr + m * GT_MSG, mh + m * GT_MSG, P + L::r_lnw, (double)rs[m],
            [&](int k, float g) {
                if (k < GT_HALF) {
                    gm[m * GT_HALF + k] = g;
                } else if (is_edge) {
                    const long o = p * GT_HALF + (k - GT_HALF);
                    gze[o] = he[o] > 0.0f ? g : 0.0f;
                }
            });
    }
    __syncthreads();
    // node module output gradient: self message plus the messages the node
    // sent, in CSR-by-src order; and the edge module's LN-output gradient
    for (int t = tid; t < Ng * GT_HALF + Eg * GT_FE; t += GT_BLOCK) {
        if (t < Ng * GT_HALF) {
            const long v = n0 + t / GT_HALF;
            const int j = t % GT_HALF;
            double acc = (double)gm[((long)E + v) * GT_HALF + j];
            const int qb = pl.sptr[v], qe = pl.sptr[v + 1];
            for (int q = qb; q < qe; ++q)
                acc += (double)gm[(long)pl.slist[q] * GT_HALF + j];
            gzn[v * GT_HALF + j] =
                hn[v * GT_HALF + j] > 0.0f ? (float)acc : 0.0f;
        } else {
            const int u = t - Ng * GT_HALF;
            const long p = e0 + u / GT_FE;
            const int k = u % GT_FE;
            double acc = 0.0;
#pragma unroll
            for (int j = 0; j < GT_HALF; ++j)
                acc = fma((double)gze[p * GT_HALF + j],
                          (double)P[L::e_W + j * GT_FE + k], acc);
            gye[p * GT_FE + k] = (float)acc;
        }
    }
    __syncthreads();
    // node module's LN-output gradient
    for (int t = tid; t < Ng * FN; t += GT_BLOCK) {
        const long v = n0 + t / FN;
        const int k = t % FN;
        double acc = 0.0;
#pragma unroll
        for (int j = 0; j < GT_HALF; ++j)
            acc = fma((double)gzn[v * GT_HALF + j],
                      (double)P[L::n_W + j * FN + k], acc);
        gyn[v * FN + k] = (float)acc;
    }
    __syncthreads();
    if (INGRAD) {
        for (int t = tid; t < Ng; t += GT_BLOCK) {
            const long v = n0 + t;
            gt_ln_bwd_row<FN>(gyn + v * FN, xn + v * FN, P + L::n_lnw,
                              (double)rsn[v],
                              [&](int k, float g) { gin[v * FN + k] = g; });
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(GT_BLOCK)
gt_bwd_rows_kernel(const float* __restrict__ gemb,   // [G, 16]
                   GtPlan pl, GtParams w, GtWs ws, GtBs bs, int E) {
    __shared__ float P[GT_NP];
    gt_stage_layer<GtL1, false>(P, w, 0);
    gt_stage_layer<GtL2, false>(P, w, 12);
    const int g = blockIdx.x;
    const int n0 = pl.node_ptr[g], n1 = pl.node_ptr[g + 1];
    const int e0 = pl.indptr[n0], e1 = pl.indptr[n1];
    // graph mean
    for (int t = threadIdx.x; t < (n1 - n0) * GT_HALF; t += GT_BLOCK)
        bs.gup2[(long)n0 * GT_HALF + t] =
            (float)((double)gemb[g * GT_HALF + t % GT_HALF]
                    / (double)(n1 - n0));
    __syncthreads();
    gt_round_bwd<GtL2, true>(P, pl, n0, n1, e0, e1, E, bs.gup2, ws.xn2,
                             ws.rsn2, ws.hn2, ws.he2, ws.mh2, ws.rs2, ws.r2,
                             bs.gzr2, bs.gyr2, bs.gm2, bs.gzn2, bs.gze2,
                             bs.gyn2, bs.gye2, bs.gup1);
    gt_round_bwd<GtL1, false>(P, pl, n0, n1, e0, e1, E, bs.gup1, ws.xn1,
                              nullptr, ws.hn1, ws.he1, ws.mh1, ws.rs1, ws.r1,
                              bs.gzr1, bs.gyr1, bs.gm1, bs.gzn1, bs.gze1,
                              bs.gyn1, bs.gye1, nullptr);
}

// ---------------------------------------------------------------------------
// weight gradients
//
// D[16x16] = sum over rows k < R of gz[k][i0 + i] * y[k][j0 + j], with
// y = xh * lnw + lnb (the module's LN output, rounded to f32 as an MFMA
// operand), or with `ones` y[k][0] = 1 and the other columns 0 (the bias).
// Rows past R contribute zeros and are never read.  8 k-steps in the f32
// MFMA accumulator, then folded into f64.  out[reg] is D's row
// (lane>>4)*4 + reg, column lane&15.
__device__ __forceinline__ void gt_mfma_tile(
    const float* __restrict__ gz, int ldg, int i0,
    const float* __restrict__ xh, int ldx, int j0,
    const float* __restrict__ lnw, const float* __restrict__ lnb, bool ones,
    long R, int lane, double out[4]) {
    const int m = lane & 15, kp = lane >> 4;
    const double lw = ones ? 0.0 : (double)lnw[j0 + m];
    const double lb = ones ? (m == 0 ? 1.0 : 0.0) : (double)lnb[j0 + m];
    out[0] = out[1] = out[2] = out[3] = 0.0;
    for (long k0 = 0; k0 < R; k0 += 32) {
        f32x4_t acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int s = 0; s < 32; s += 4) {
            const long row = k0 + s + kp;
            const bool in = row < R;
            const long rr = in ? row : 0;
            const float a = in ? gz[rr * ldg + i0 + m] : 0.0f;
            const float x = (in && !ones) ? xh[rr * ldx + j0 + m] : 0.0f;
            const float b = in ? (float)fma((double)x, lw, lb) : 0.0f;
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) out[q] += (double)acc[q];
    }
}

// one thread per output of a K = 5 / K = 2 module: u < 16 * (K + 1)
template <int K>
__device__ __forceinline__ void gt_small_wgrad(
    const float* __restrict__ gz, const float* __restrict__ xh,
    const float* __restrict__ lnw, const float* __restrict__ lnb, long R,
    int u, float* __restrict__ gW, float* __restrict__ gb) {
    const int i = u / (K + 1), c = u % (K + 1);
    double acc = 0.0;
    if (c < K) {
        const double lw = (double)lnw[c], lb = (double)lnb[c];
#pragma unroll 8
        for (long r = 0; r < R; ++r)
            acc = fma((double)gz[r * GT_HALF + i],
                      fma((double)xh[r * K + c], lw, lb), acc);
        gW[i * K + c] = (float)acc;
    } else {
#pragma unroll 8
        for (long r = 0; r < R; ++r) acc += (double)gz[r * GT_HALF + i];
        gb[i] = (float)acc;
    }
}

// one thread per LayerNorm gradient: u < K is ln_w[u], else ln_b[u - K]
__device__ __forceinline__ void gt_ln_wgrad(const float* __restrict__ gy,
                                            const float* __restrict__ xh,
                                            int K, long R, int u,
                                            float* __restrict__ glnw,
                                            float* __restrict__ glnb) {
    double acc = 0.0;
    if (u < K) {
#pragma unroll 8
        for (long r = 0; r < R; ++r)
            acc = fma((double)gy[r * K + u], (double)xh[r * K + u], acc);
        glnw[u] = (float)acc;
    } else {
        const int k = u - K;
#pragma unroll 8
        for (long r = 0; r < R; ++r) acc += (double)gy[r * K + k];
        glnb[k] = (float)acc;
    }
}

#define GT_T_WR1 12      // gzr1^T [64 x k] . (y1 | ones) [k x 3 tiles]
#define GT_T_WR2 3       // gzr2^T [16 x k] . (y2 | ones)
#define GT_T_WN2 5       // gzn2^T [16 x k] . (yn2 | ones) [k x 5 tiles]
#define GT_TILES (GT_T_WR1 + GT_T_WR2 + GT_T_WN2)
#define GT_MFMA_BLOCKS (GT_TILES / 4)
#define GT_SMALL (16 * 6 + 16 * 3 + 16 * 3)
#define GT_LNG (2 * (5 + GT_FE + GT_MSG + 64 + GT_FE + GT_MSG))
#define GT_VALU_BLOCKS ((GT_SMALL + GT_LNG + GT_WG_BLOCK - 1) / GT_WG_BLOCK)
static_assert(GT_TILES % 4 == 0, "one wave per tile, four waves per block");

__global__ void __launch_bounds__(GT_WG_BLOCK)
gt_bwd_wgrad_kernel(GtParams w, GtWs ws, GtBs bs,
                    float* __restrict__ G,          // [GT_NP] flat grads
                    int N, int E) {
    const int tid = threadIdx.x;
    const int wave = tid / GT_WAVE, lane = tid % GT_WAVE;
    const long M = (long)N + E;
    if (blockIdx.x < GT_MFMA_BLOCKS) {
        int t = blockIdx.x * 4 + wave;
        const int col = lane & 15, row0 = (lane >> 4) * 4;
        double d[4];
        if (t < GT_T_WR1) {
            const int it = t / 3, jt = t % 3;
            gt_mfma_tile(bs.gzr1, 64, it * 16, ws.mh1, GT_MSG,
                         jt < 2 ? jt * 16 : 0, w.p[8], w.p[9], jt == 2, M,
                         lane, d);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int i = it * 16 + row0 + q;
                if (jt < 2) G[GtL1::r_W + i * GT_MSG + jt * 16 + col] = (float)d[q];
                else if (col == 0) G[GtL1::r_b + i] = (float)d[q];
            }
            return;
        }
        t -= GT_T_WR1;
        if (t < GT_T_WR2) {
            gt_mfma_tile(bs.gzr2, 16, 0, ws.mh2, GT_MSG, t < 2 ? t * 16 : 0,
                         w.p[20], w.p[21], t == 2, M, lane, d);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int i = row0 + q;
                if (t < 2) G[GtL2::r_W + i * GT_MSG + t * 16 + col] = (float)d[q];
                else if (col == 0) G[GtL2::r_b + i] = (float)d[q];
            }
            return;
        }
        t -= GT_T_WR2;
        gt_mfma_tile(bs.gzn2, GT_HALF, 0, ws.xn2, 64, t < 4 ? t * 16 : 0,
                     w.p[12], w.p[13], t == 4, N, lane, d);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = row0 + q;
            if (t < 4) G[GtL2::n_W + i * 64 + t * 16 + col] = (float)d[q];
            else if (col == 0) G[GtL2::n_b + i] = (float)d[q];
        }
        return;
    }
    // one thread per output, rows in order
    int u = (blockIdx.x - GT_MFMA_BLOCKS) * GT_WG_BLOCK + tid;
    if (u < 96) {
        gt_small_wgrad<5>(bs.gzn1, ws.xn1, w.p[0], w.p[1], N, u,
                          G + GtL1::n_W, G + GtL1::n_b);
        return;
    }
    u -= 96;
    if (u < 48) {
        gt_small_wgrad<GT_FE>(bs.gze1, ws.xe1, w.p[4], w.p[5], E, u,
                              G + GtL1::e_W, G + GtL1::e_b);
        return;
    }
    u -= 48;
    if (u < 48) {
        gt_small_wgrad<GT_FE>(bs.gze2, ws.xe2, w.p[16], w.p[17], E, u,
                              G + GtL2::e_W, G + GtL2::e_b);
        return;
    }
    u -= 48;
    if (u < 10) {
        gt_ln_wgrad(bs.gyn1, ws.xn1, 5, N, u, G + GtL1::n_lnw, G + GtL1::n_lnb);
        return;
    }
    u -= 10;
    if (u < 4) {
        gt_ln_wgrad(bs.gye1, ws.xe1, GT_FE, E, u, G + GtL1::e_lnw,
                    G + GtL1::e_lnb);
        return;
    }
    u -= 4;
    if (u < 64) {
        gt_ln_wgrad(bs.gyr1, ws.mh1, GT_MSG, M, u, G + GtL1::r_lnw,
                    G + GtL1::r_lnb);
        return;
    }
    u -= 64;
    if (u < 128) {
        gt_ln_wgrad(bs.gyn2, ws.xn2, 64, N, u, G + GtL2::n_lnw,
                    G + GtL2::n_lnb);
        return;
    }
    u -= 128;
    if (u < 4) {
        gt_ln_wgrad(bs.gye2, ws.xe2, GT_FE, E, u, G + GtL2::e_lnw,
                    G + GtL2::e_lnb);
        return;
    }
    u -= 4;
    if (u < 64)
        gt_ln_wgrad(bs.gyr2, ws.mh2, GT_MSG, M, u, G + GtL2::r_lnw,
                    G + GtL2::r_lnb);
}

// ---------------------------------------------------------------------------
// population forward (ES): P members x G graphs in one launch, forward only
//
//   gt_pop_fwd_kernel    grid = (G, P), one workgroup per (graph, member).
//                        Member m's 4146 trunk weights are the contiguous
//                        range pop[m, off : off + 4146], already in GtLay
//                        order: one pass stages them into LDS, the six W
//                        matrices transposed as gt_stage_layer<L, true> does
//                        (scalar loads: a row of pop is not 16-byte aligned).
//                        A round is two phases instead of five:
//                          A  per node / edge row, one 16-lane group:
//                             LayerNorm -> Linear -> ReLU      -> hn, he
//                          B  per destination node, OUT lanes: self message,
//                             then in-edges ascending; gather, LayerNorm over
//                             32, reduce Linear + ReLU, running sum -> z
//                        xn / xe / mh / rs / r never reach memory.  The rows
//                        between the phases (hn, he, z1; z2 takes z1's place)
//                        are Ng * 80 + Eg * 16 floats: in LDS when that fits
//                        GT_POP_ROWS, else in the (member, graph) slab of a
//                        global scratch tensor.
//
// The arithmetic is gt_fwd_kernel's, operation for operation: the same f64
// sums in the same order, rounded to f32 where gt_fwd_kernel stores (xh, hn /
// he, mh, r, z), so member m's output equals gnn_trunk_fwd on member m's
// tensors bit for bit.
#define GT_POP_ROWS 8192      // floats; 16.6 KB weights + 4 KB partials +
                              // 32 KB rows < 160 KB / 3: LDS allows the 3
                              // workgroups per CU that 80 VGPRs allow
#define GT_POP_NODE (GT_HALF + 64)   // hn row + z1 row, floats per node

// where element i of the flat GtLay range lands in LDS
template <class L>
__device__ __forceinline__ int gt_pop_dst(int i) {
    if (i >= L::n_W && i < L::n_b) {
        const int u = i - L::n_W;
        return L::n_W + (u % L::FN) * GT_HALF + u / L::FN;
    }
    if (i >= L::e_W && i < L::e_b) {
        const int u = i - L::e_W;
        return L::e_W + (u % GT_FE) * GT_HALF + u / GT_FE;
    }
    if (i >= L::r_W && i < L::r_b) {
        const int u = i - L::r_W;
        return L::r_W + (u % GT_MSG) * L::OUT + u / GT_MSG;
    }
    return i;
}

// Phase A of one row by the 16 lanes of a group (all 16 active): lane j holds
// x[j], x[16 + j], ...; every lane walks k = 0 .. K-1 over lane shuffles in
// gt_ln_row's order, so the 16 lanes hold the same statistics; lane j then
// owns xh[j], xh[16 + j], ... and output j (gt_lin_relu's sum).
template <int K>
__device__ __forceinline__ float gt_pop_row(const float* x, const float* lnw,
                                            const float* lnb, const float* WT,
                                            int j, float bias) {
    constexpr int NV = (K + GT_HALF - 1) / GT_HALF;
    float xr[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int k = i * GT_HALF + j;
        xr[i] = k < K ? x[k] : 0.0f;
    }
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        constexpr int KK = K < GT_HALF ? K : GT_HALF;
#pragma unroll 8
        for (int kk = 0; kk < KK; ++kk)
            s += (double)__shfl(xr[i], kk, GT_HALF);
    }
    const double mean = s / K;
    double v = 0.0;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        constexpr int KK = K < GT_HALF ? K : GT_HALF;
#pragma unroll 8
        for (int kk = 0; kk < KK; ++kk) {
            const double d = (double)__shfl(xr[i], kk, GT_HALF) - mean;
            v = fma(d, d, v);
        }
    }
    const double rstd = 1.0 / sqrt(v / K + GT_LN_EPS);
#pragma unroll
    for (int i = 0; i < NV; ++i)
        xr[i] = (float)(((double)xr[i] - mean) * rstd);
    double acc = (double)bias;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        constexpr int KK = K < GT_HALF ? K : GT_HALF;
#pragma unroll 8
        for (int kk = 0; kk < KK; ++kk) {
            const int k = i * GT_HALF + kk;
            const float xh = __shfl(xr[i], kk, GT_HALF);
            const double y = fma((double)xh, (double)lnw[k], (double)lnb[k]);
            acc = fma((double)WT[k * GT_HALF + j], y, acc);
        }
    }
    return fmaxf((float)acc, 0.0f);
}

// One message through the reduce module, output j: a = hn[src], b = he[p]
// for an edge message; the self message has zeros in b's place.  Phases 3 and
// 4 of gt_round_fwd with nothing stored: the row is read three times (LDS, or
// L1 on the scratch path) so that no loop needs it in registers.
template <class L, bool EDGE>
__device__ __forceinline__ float gt_pop_msg(const float* P, const float* a,
                                            const float* b, int j) {
    double s = 0.0;
#pragma unroll 4
    for (int k = 0; k < GT_HALF; ++k) {
        s += (double)a[k];
        if (EDGE) s += (double)b[k];
    }
    const double mean = s / GT_MSG;
    double var = 0.0;
#pragma unroll 4
    for (int k = 0; k < GT_HALF; ++k) {
        const double da = (double)a[k] - mean;
        const double db = (EDGE ? (double)b[k] : 0.0) - mean;
        var = fma(da, da, var);
        var = fma(db, db, var);
    }
    const double rstd = 1.0 / sqrt(var / GT_MSG + GT_LN_EPS);
    // mh[k] is rounded to f32 as gt_round_fwd stores it, then gt_lin_relu's
    // sum over k = 0 .. 31: the hn half, then the he half
    double acc = (double)P[L::r_b + j];
#pragma unroll 4
    for (int k = 0; k < GT_HALF; ++k) {
        const float mh = (float)(((double)a[k] - mean) * rstd);
        const double y = fma((double)mh, (double)P[L::r_lnw + k],
                             (double)P[L::r_lnb + k]);
        acc = fma((double)P[L::r_W + k * L::OUT + j], y, acc);
    }
#pragma unroll 4
    for (int k = 0; k < GT_HALF; ++k) {
        const float mh = (float)(((EDGE ? (double)b[k] : 0.0) - mean) * rstd);
        const double y = fma((double)mh, (double)P[L::r_lnw + GT_HALF + k],
                             (double)P[L::r_lnb + GT_HALF + k]);
        acc = fma((double)P[L::r_W + (GT_HALF + k) * L::OUT + j], y, acc);
    }
    return fmaxf((float)acc, 0.0f);
}

// One MeanPool round of graph rows [n0, n1) / positions [e0, e1) over row
// pointers (LDS or global alike).  x is the round's node input, row v at
// x + (v - xbase) * FN; hn [Ng, 16], he [Eg, 16] and z [Ng, OUT] are indexed
// from the graph's first node / position.
template <class L>
__device__ __forceinline__ void gt_pop_round(
    const float* P, const float* x, int xbase, const float* __restrict__ e,
    const GtPlan& pl, int n0, int n1, int e0, int e1, float* hn, float* he,
    float* z) {
    constexpr int FN = L::FN, OUT = L::OUT;
    const int tid = threadIdx.x;
    const int Ng = n1 - n0, Eg = e1 - e0;
    // A: one 16-lane group per node row / edge row
    {
        const int j = tid % GT_HALF;
        for (int row = tid / GT_HALF; row < Ng + Eg;
             row += GT_BLOCK / GT_HALF) {
            if (row < Ng) {
                hn[row * GT_HALF + j] = gt_pop_row<FN>(
                    x + (long)(n0 + row - xbase) * FN, P + L::n_lnw,
                    P + L::n_lnb, P + L::n_W, j, P[L::n_b + j]);
            } else {
                const int q = row - Ng;
                he[q * GT_HALF + j] = gt_pop_row<GT_FE>(
                    e + (long)pl.eo[e0 + q] * GT_FE, P + L::e_lnw,
                    P + L::e_lnb, P + L::e_W, j, P[L::e_b + j]);
            }
        }
    }
    __syncthreads();
    // B: OUT lanes per destination node, lane j owns output j
    {
        const int j = tid % OUT;
        for (int t = tid / OUT; t < Ng; t += GT_BLOCK / OUT) {
            const int v = n0 + t;
            const int pb = pl.indptr[v], pe = pl.indptr[v + 1];
            float out = 0.0f;
            if (pe > pb) {
                double acc = (double)gt_pop_msg<L, false>(
                    P, hn + t * GT_HALF, nullptr, j);
                for (int p = pb; p < pe; ++p)
                    acc += (double)gt_pop_msg<L, true>(
                        P, hn + (pl.srcp[p] - n0) * GT_HALF,
                        he + (p - e0) * GT_HALF, j);
                out = (float)(acc / (double)(pe - pb + 1));
            }
            z[t * OUT + j] = out;
        }
    }
    __syncthreads();
}

// both rounds over one set of row pointers; z2 takes z1's place (round 2
// reads z1 in phase A only, and a barrier ends that phase)
__device__ __forceinline__ const float* gt_pop_rounds(
    const float* P, const float* __restrict__ z0, const float* __restrict__ e,
    const GtPlan& pl, int n0, int n1, int e0, int e1, float* rows) {
    float* hn = rows;
    float* he = hn + (long)(n1 - n0) * GT_HALF;
    float* zz = he + (long)(e1 - e0) * GT_HALF;
    gt_pop_round<GtL1>(P, z0, 0, e, pl, n0, n1, e0, e1, hn, he, zz);
    gt_pop_round<GtL2>(P, zz, n0, e, pl, n0, n1, e0, e1, hn, he, zz);
    return zz;
}

__global__ void __launch_bounds__(GT_BLOCK)
gt_pop_fwd_kernel(const float* __restrict__ z0,      // [N, 5]
                  const float* __restrict__ e,       // [E, 2]
                  GtPlan pl,
                  const float* __restrict__ pop,     // [P, n], trunk at off
                  long n, long off,
                  float* __restrict__ scratch,       // [P, slab] or null
                  long slab,                         // N * 80 + E * 16
                  float* __restrict__ emb) {         // [P, G, 16]
    __shared__ float P[GT_NP];
    __shared__ __attribute__((aligned(16))) float R[GT_POP_ROWS];
    __shared__ double part[GT_BLOCK / GT_HALF][GT_HALF];
    const int g = blockIdx.x, m = blockIdx.y;
    const float* w = pop + (long)m * n + off;
    for (int i = threadIdx.x; i < GT_NP; i += GT_BLOCK)
        P[i < GtL1::end ? gt_pop_dst<GtL1>(i) : gt_pop_dst<GtL2>(i)] = w[i];
    __syncthreads();
    const int n0 = pl.node_ptr[g], n1 = pl.node_ptr[g + 1];
    const int e0 = pl.indptr[n0], e1 = pl.indptr[n1];
    const long need = (long)(n1 - n0) * GT_POP_NODE + (long)(e1 - e0) * GT_HALF;
    // one branch per address space, so each copy of the rounds is compiled
    // for LDS or for global rows
    const float* z2;
    if (need <= GT_POP_ROWS)
        z2 = gt_pop_rounds(P, z0, e, pl, n0, n1, e0, e1, R);
    else
        z2 = gt_pop_rounds(P, z0, e, pl, n0, n1, e0, e1,
                           scratch + (long)m * slab + (long)n0 * GT_POP_NODE
                               + (long)e0 * GT_HALF);
    // graph mean: 32 row groups x 16 features, partials summed in order
    const int j = threadIdx.x % GT_HALF, grp = threadIdx.x / GT_HALF;
    double acc = 0.0;
    for (int t = grp; t < n1 - n0; t += GT_BLOCK / GT_HALF)
        acc += (double)z2[t * GT_HALF + j];
    part[grp][j] = acc;
    __syncthreads();
    if (threadIdx.x < GT_HALF) {
        double s = 0.0;
#pragma unroll
        for (int q = 0; q < GT_BLOCK / GT_HALF; ++q) s += part[q][threadIdx.x];
        emb[((long)m * gridDim.x + g) * GT_HALF + threadIdx.x] =
            n1 > n0 ? (float)(s / (double)(n1 - n0)) : 0.0f;
    }
}

#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute pop
#endif

// ---------------------------------------------------------------------------
static void gt_check(const torch::Tensor& t, c10::ScalarType dt,
                     std::vector<int64_t> shape, const char* name) {
    TORCH_CHECK(t.is_cuda() && t.scalar_type() == dt && t.is_contiguous()
                && t.sizes() == c10::IntArrayRef(shape),
                "gnn_trunk ", name, ": expected a contiguous CUDA ",
                c10::toString(dt), " tensor of shape ",
                c10::IntArrayRef(shape), ", got ", t.sizes(),
                " (the kernels serve the tuned GNN shape only: two rounds, "
                "node 5, edge 2, message 32, hidden 64, output 16)");
}

static GtParams gt_check_params(const std::vector<torch::Tensor>& p) {
    TORCH_CHECK(p.size() == 24, "gnn_trunk: expected the 24 tensors of "
                "gnn.parameters() (two MeanPool rounds, module_depth 1), got ",
                p.size());
    const auto f32 = torch::kFloat32;
    GtParams w;
    for (int l = 0; l < 2; ++l) {
        const int64_t FN = l == 0 ? 5 : 64, OUT = l == 0 ? 64 : 16;
        const int t = 12 * l;
        gt_check(p[t + 0], f32, {FN}, "node ln weight");
        gt_check(p[t + 1], f32, {FN}, "node ln bias");
        gt_check(p[t + 2], f32, {GT_HALF, FN}, "node W");
        gt_check(p[t + 3], f32, {GT_HALF}, "node b");
        gt_check(p[t + 4], f32, {GT_FE}, "edge ln weight");
        gt_check(p[t + 5], f32, {GT_FE}, "edge ln bias");
        gt_check(p[t + 6], f32, {GT_HALF, GT_FE}, "edge W");
        gt_check(p[t + 7], f32, {GT_HALF}, "edge b");
        gt_check(p[t + 8], f32, {GT_MSG}, "reduce ln weight");
        gt_check(p[t + 9], f32, {GT_MSG}, "reduce ln bias");
        gt_check(p[t + 10], f32, {OUT, GT_MSG}, "reduce W");
        gt_check(p[t + 11], f32, {OUT}, "reduce b");
    }
    for (int i = 0; i < 24; ++i) w.p[i] = p[i].data_ptr<float>();
    return w;
}

// plan = {eo, srcp, dstp, indptr, sptr, slist, node_ptr}, int32, as
// GraphBatch.trunk_plan() builds and validates it on the host
static GtPlan gt_check_plan(const std::vector<torch::Tensor>& plan, int64_t N,
                            int64_t E, int64_t* G) {
    TORCH_CHECK(plan.size() == 7, "gnn_trunk: plan must hold 7 tensors");
    TORCH_CHECK(plan[6].dim() == 1 && plan[6].size(0) >= 2,
                "gnn_trunk: node_ptr must be [G + 1] with G >= 1");
    *G = plan[6].size(0) - 1;
    const auto i32 = torch::kInt32;
    gt_check(plan[0], i32, {E}, "plan eo");
    gt_check(plan[1], i32, {E}, "plan srcp");
    gt_check(plan[2], i32, {E}, "plan dstp");
    gt_check(plan[3], i32, {N + 1}, "plan indptr");
    gt_check(plan[4], i32, {N + 1}, "plan sptr");
    gt_check(plan[5], i32, {E}, "plan slist");
    gt_check(plan[6], i32, {*G + 1}, "plan node_ptr");
    GtPlan pl;
    pl.eo = plan[0].data_ptr<int>();
    pl.srcp = plan[1].data_ptr<int>();
    pl.dstp = plan[2].data_ptr<int>();
    pl.indptr = plan[3].data_ptr<int>();
    pl.sptr = plan[4].data_ptr<int>();
    pl.slist = plan[5].data_ptr<int>();
    pl.node_ptr = plan[6].data_ptr<int>();
    return pl;
}

// Workspace layout: consecutive row-major arrays in GtWs order.  Returns the
// float count; fills `ws` when base is given.
static int64_t gt_ws_layout(float* base, int64_t N, int64_t E, GtWs* ws) {
    const int64_t M = N + E;
    const int64_t sizes[17] = {N * 5, E * 2, N * 16, E * 16, M * 32, M, M * 64,
                               N * 64, N * 64, N, E * 2, N * 16, E * 16,
                               M * 32, M, M * 16, N * 16};
    float** f = &ws->xn1;
    int64_t off = 0;
    for (int i = 0; i < 17; ++i) {
        if (base != nullptr) f[i] = base + off;
        off += sizes[i];
    }
    return off;
}

static int64_t gt_bs_layout(float* base, int64_t N, int64_t E, GtBs* bs) {
    const int64_t M = N + E;
    const int64_t sizes[16] = {N * 16, M * 16, M * 32, M * 16, N * 16, E * 16,
                               N * 64, E * 2, N * 64, M * 64, M * 32, M * 16,
                               N * 16, E * 16, N * 5, E * 2};
    float** f = &bs->gup2;
    int64_t off = 0;
    for (int i = 0; i < 16; ++i) {
        if (base != nullptr) f[i] = base + off;
        off += sizes[i];
    }
    return off;
}

static void gt_check_batch(const torch::Tensor& z, const torch::Tensor& e,
                           int64_t* N, int64_t* E) {
    TORCH_CHECK(z.dim() == 2 && e.dim() == 2,
                "gnn_trunk: z must be [N, 5] and e [E, 2]");
    *N = z.size(0);
    *E = e.size(0);
    TORCH_CHECK(*N >= 1 && *N + *E < (1LL << 24),
                "gnn_trunk: needs N >= 1 nodes and N + E < 2^24 rows");
    gt_check(z, torch::kFloat32, {*N, 5}, "z");
    gt_check(e, torch::kFloat32, {*E, GT_FE}, "e");
}

// Returns {model_emb [G, 16], workspace}: the workspace is what gnn_trunk_bwd
// reads again.
std::vector<torch::Tensor> gnn_trunk_fwd(torch::Tensor z, torch::Tensor e,
                                         std::vector<torch::Tensor> plan,
                                         std::vector<torch::Tensor> params) {
    int64_t N, E, G;
    gt_check_batch(z, e, &N, &E);
    const GtPlan pl = gt_check_plan(plan, N, E, &G);
    const GtParams w = gt_check_params(params);
    GtWs ws;
    auto wst = torch::empty({gt_ws_layout(nullptr, N, E, &ws)}, z.options());
    gt_ws_layout(wst.data_ptr<float>(), N, E, &ws);
    auto emb = torch::empty({G, GT_HALF}, z.options());
    hipStream_t stream = at::cuda::getCurrentCUDAStream();
    hipLaunchKernelGGL(gt_fwd_kernel, dim3((unsigned)G), dim3(GT_BLOCK), 0,
                       stream, z.data_ptr<float>(), e.data_ptr<float>(), pl,
                       w, ws, emb.data_ptr<float>(), (int)E);
    return {emb, wst};
}

// Gradients of sum(gemb * model_emb) in gnn.parameters() order (24 tensors,
// views of one flat buffer).  batch.z and batch.e are constants.
std::vector<torch::Tensor> gnn_trunk_bwd(torch::Tensor gemb,
                                         torch::Tensor workspace,
                                         std::vector<torch::Tensor> plan,
                                         std::vector<torch::Tensor> params) {
    TORCH_CHECK(plan.size() == 7 && plan[3].dim() == 1 && plan[0].dim() == 1,
                "gnn_trunk_bwd: plan must hold 7 tensors");
    const int64_t N = plan[3].size(0) - 1, E = plan[0].size(0);
    TORCH_CHECK(N >= 1 && N + E < (1LL << 24),
                "gnn_trunk_bwd: needs N >= 1 nodes and N + E < 2^24 rows");
    int64_t G;
    const GtPlan pl = gt_check_plan(plan, N, E, &G);
    const GtParams w = gt_check_params(params);
    GtWs ws;
    GtBs bs;
    gt_check(workspace, torch::kFloat32, {gt_ws_layout(nullptr, N, E, &ws)},
             "workspace");
    gt_check(gemb, torch::kFloat32, {G, GT_HALF}, "g_model_emb");
    gt_ws_layout(workspace.data_ptr<float>(), N, E, &ws);
    auto bst = torch::empty({gt_bs_layout(nullptr, N, E, &bs)},
                            gemb.options());
    gt_bs_layout(bst.data_ptr<float>(), N, E, &bs);
    auto flat = torch::empty({GT_NP}, gemb.options());
    hipStream_t stream = at::cuda::getCurrentCUDAStream();
    hipLaunchKernelGGL(gt_bwd_rows_kernel, dim3((unsigned)G), dim3(GT_BLOCK),
                       0, stream, gemb.data_ptr<float>(), pl, w, ws, bs,
                       (int)E);
    hipLaunchKernelGGL(gt_bwd_wgrad_kernel,
                       dim3(GT_MFMA_BLOCKS + GT_VALU_BLOCKS),
                       dim3(GT_WG_BLOCK), 0, stream, w, ws, bs,
                       flat.data_ptr<float>(), (int)N, (int)E);
    std::vector<torch::Tensor> grads;
    int64_t off = 0;
    for (const auto& p : params) {
        grads.push_back(flat.narrow(0, off, p.numel()).view(p.sizes()));
        off += p.numel();
    }
    return grads;
}

// model_emb [P, G, 16] of P population members in one launch: member m's
// trunk is pop[m, off : off + 4146] (gnn.parameters() order).  Forward only,
// no workspace.  Scratch is allocated only when some graph's rows exceed
// GT_POP_ROWS; finding that out reads node_ptr / indptr back (one sync), and
// only when the whole batch is larger than the budget.
torch::Tensor gnn_trunk_population_fwd(torch::Tensor z, torch::Tensor e,
                                       std::vector<torch::Tensor> plan,
                                       torch::Tensor pop, int64_t off) {
    int64_t N, E, G;
    gt_check_batch(z, e, &N, &E);
    const GtPlan pl = gt_check_plan(plan, N, E, &G);
    TORCH_CHECK(pop.is_cuda() && pop.device() == z.device()
                && pop.scalar_type() == torch::kFloat32 && pop.dim() == 2
                && pop.is_contiguous(),
                "gnn_trunk population: pop must be a contiguous float32 "
                "[P, n] tensor on the batch's device");
    const int64_t P = pop.size(0), n = pop.size(1);
    TORCH_CHECK(P >= 1 && P <= 65535 && G <= 0x7fffffff,
                "gnn_trunk population: needs 1 <= P <= 65535 members, got ",
                P);
    TORCH_CHECK(off >= 0 && off + GT_NP <= n,
                "gnn_trunk population: the trunk's ", (int)GT_NP,
                " parameters at offset ", off, " do not fit a row of ", n,
                " (the kernels serve the tuned GNN shape only)");
    const int64_t slab = N * GT_POP_NODE + E * GT_HALF;
    torch::Tensor scratch;
    if (slab > GT_POP_ROWS) {
        const auto np = plan[6].cpu(), ip = plan[3].cpu();
        const int* npp = np.data_ptr<int>();
        const int* ipp = ip.data_ptr<int>();
        int64_t worst = 0;
        for (int64_t g = 0; g < G; ++g) {
            TORCH_CHECK(npp[g] >= 0 && npp[g] <= npp[g + 1]
                        && npp[g + 1] <= N,
                        "gnn_trunk population: node_ptr is not a prefix "
                        "over [0, N]");
            worst = std::max<int64_t>(
                worst, (int64_t)(npp[g + 1] - npp[g]) * GT_POP_NODE
                           + (int64_t)(ipp[npp[g + 1]] - ipp[npp[g]])
                                 * GT_HALF);
        }
        if (worst > GT_POP_ROWS) scratch = torch::empty({P * slab}, z.options());
    }
    auto emb = torch::empty({P, G, GT_HALF}, z.options());
    hipStream_t stream = at::cuda::getCurrentCUDAStream();
    hipLaunchKernelGGL(gt_pop_fwd_kernel, dim3((unsigned)G, (unsigned)P),
                       dim3(GT_BLOCK), 0, stream, z.data_ptr<float>(),
                       e.data_ptr<float>(), pl, pop.data_ptr<float>(),
                       (long)n, (long)off,
                       scratch.defined() ? scratch.data_ptr<float>() : nullptr,
                       (long)slab, emb.data_ptr<float>());
    return emb;
}
