// Fully-fused PPO minibatch step for the cached-models SGD mode (gfx950).
//
// The tuned PAC-ML policy is ~35k params and a minibatch is 128 samples over
// M <= 16 distinct workload-model graphs (~200 nodes total): the whole
// fwd+bwd is ~10 MFLOP.  Run as torch autograd it is ~146 dispatches per
// replay (42% zero-fill / grad-accumulate glue — profiles/
// kernel_stats_r02_cachedsgd.csv); here it is SIX kernels (3 fwd + 3 bwd)
// sized to the work's parallelism, with every weight gradient computed as a
// deterministic LDS-tiled A^T.B contraction (no atomics, replay-stable):
//
//   fwd:  cs_fwd_gnn   (1 WG)   GNN rounds + pooling + per-sample `final`
//         cs_fwd_head  (many)   FC branches over B x FC units
//         cs_fwd_loss  (1 WG)   softmax/surrogate rows + device stats
//   bwd:  cs_bwd_head  (many)   per-sample chain: glogits -> gh1 -> gfinal
//         cs_bwd_gnn   (1 WG)   pool grads + both MeanPool rounds' data bwd
//         cs_bwd_w     (many)   ALL weight/bias/LN grads into flat_g
//
// That was the first cut.  The step is now 13 launches (16 per replay with
// the stage kernel and the two-launch optimiser tail), in this order:
//
//   fwd:  cs_fwd_mlp_lanes<1>        round-1 node / edge modules
//         cs_fwd_reduce_lanes<1>     round-1 reduce module (edge + self rows)
//         cs_fwd_comb1_mlp2_lanes    h1 = CSR mean, then the round-2 modules
//         cs_fwd_reduce_lanes<2>     round-2 reduce module
//         cs_fwd_comb2_pool          h2 = CSR mean + per-model means
//         cs_head                    per SAMPLE: final row, FC branches,
//                                    logits/value, loss row, and the whole
//                                    head backward down to gfinal / gu34
//   bwd:  cs_bwd_pool                pool grads -> gh2
//         cs_bwd_reduce_lanes<2>     round-2 reduce module backward
//         cs_bwd_scat2_mlp2_lanes    scatter to ghn2/ghe2 + round-2 modules
//         cs_bwd_reduce_lanes<1>     round-1 reduce module backward
//         cs_bwd_scat1_gu1           scatter to ghn1/ghe1 + module-1 gu rows
//                                    (+ one block for the C_STATS sums)
//         cs_bwd_w, cs_bwd_w_reduce  all weight grads into flat_g
//
// By default two of those carry work that waits for nothing ahead of it in
// the chain (section "work off the serial chain" below): the first forward
// launch is cs_fwd_stage_mlp1_lanes (block 0 gathers the minibatch, so the
// stage kernel's own launch goes away: 15 per replay), and cs_bwd_pool is
// cs_bwd_pool_wfc, one pool block per model beside the 17 B-row weight-grad
// blocks that cs_bwd_w then no longer launches.  DDLS_AMD_STEP_OVERLAP=off
// launches the sequence above.
//
// By default three pairs of those are merged along row-local dependencies
// (DDLS_AMD_STEP_MERGE, sections "cs_stage + round-1 node / edge modules +
// round-1 reduce module" and "cs_bwd_scat1_gu1 + the row jobs of cs_bwd_w"
// below): the first two forward launches are one, cs_bwd_scat1_gu1 and
// cs_bwd_w are one, and cs_bwd_w_reduce's sums are formed by the first
// kernel of the optimiser tail when the caller defers them: 12 per replay.
//
// By default the two longest of those twelve run with shorter chains
// (DDLS_AMD_STEP_HEAD, sections "cs_head with a shorter chain" and
// "cs_bwd_pool_wfc with shorter roles" below): cs_head2 in place of cs_head
// and cs_bwd_pool_wfc2 in place of cs_bwd_pool_wfc, the same launches with
// the same outputs in the same bits.  DDLS_AMD_STEP_HEAD=off launches the
// two kernels they replace.
//
// DDLS_AMD_STEP_FUSION=off launches the previous 20 separate kernels and
// DDLS_AMD_ROW_KERNELS=thread the thread-per-row ones before them; both
// sets stay in this file unchanged as oracles for bitwise comparison.
//
// Exact-by-linearity gradient aggregation: per-sample dL/d emb reaches the
// (shared) per-model GNN summed over the minibatch — the same contraction
// index_select's backward performs, done here in one deterministic pass.
//
// Layer semantics mirror models/gnn.py (MeanPoolLayer / GNNPolicy): each
// module is LayerNorm -> Linear -> ReLU (module_depth=1), message =
// concat(hn[src], he), self-message = concat(hn[v], 0), out =
// (sum msgs + self) / (deg+1), zero for nodes with no in-edges; the
// graph_module is LN -> Linear (no activation); branches Linear-ReLU-Linear;
// mask added as clamp(log(mask)).  Loss matches ppo_loss.hip.  LayerNorm
// eps = 1e-5 (torch default), biased variance.
#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>
#include <cstdlib>
#include <cstring>
#include <vector>

// the minibatch stage role (shared with batch_stage.hip)
#include "cs_stage.h"

#define LN_EPS 1e-5f

// Gradients from this file are compared bitwise from one revision to the
// next.  Whether the compiler contracts a*b+c into one fused multiply-add or
// rounds the product first depends on its unrolling and packing choices, so
// kernels that were restructured after such a comparison was first taken
// spell out the rounding their predecessor had: FMA() is one rounding,
// x + mul_rn(a, b) is two.
#define FMA(a, b, c) __builtin_fmaf((a), (b), (c))
__device__ __forceinline__ float mul_rn(float a, float b) {
  float p = a * b;
  asm("" : "+v"(p));   // opaque to the optimiser: stays a rounded product
  return p;
}

// Compile-time dims of the tuned PAC-ML policy (model/gnn.yaml values).
// fill_ptrs TORCH_CHECKs the runtime tensors against these; the Python side
// (graph_step._FusedCachedEngine.eligible) refuses other shapes.  Constant
// bounds let hipcc fully unroll the row loops so per-thread scratch arrays
// live in registers instead of spilled scratch memory.
#define KF0 5
#define KFE 2
#define KH 16
#define KMSG 32
#define KHID 64
#define KOUT 16
#define KGF 34
#define KGE 8
#define KFIN 24
#define KFC 256
#define KA 17

// ---- tensor-list indices (mirror rl/graph_step.py fused mode) ----
enum {
  // static graph
  C_Z0 = 0, C_E, C_SRC, C_DST, C_ORDER, C_INDPTR, C_SRC_ORDER, C_SRC_INDPTR,
  C_NODE_MODEL, C_MODEL_NPTR,
  // staged inputs
  C_MODEL_IDS, C_GF, C_MASK, C_ACTIONS, C_OLD_LOGP, C_ADV, C_VTARG, C_KL,
  // weights
  C_FLAT_P, C_FLAT_G, C_OFFS,
  // fwd activation scratch
  C_HN1, C_HE1, C_RE1, C_RS1, C_H1,
  C_HN2, C_HE2, C_RE2, C_RS2, C_H2, C_POOLED,
  C_XH_Z1, C_XH_E1, C_XH_M1E, C_XH_M1S, C_RST_Z1, C_RST_E1, C_RST_M1E,
  C_RST_M1S,
  C_XH_H2, C_XH_E2, C_XH_M2E, C_XH_M2S, C_RST_H2, C_RST_E2, C_RST_M2E,
  C_RST_M2S,
  C_XH34, C_FINAL, C_H1P, C_H1V, C_VALUES, C_P, C_LP, C_COEF, C_HENT,
  C_STATS,
  // bwd scratch
  C_GLOGITS, C_GVALUE, C_GH1P, C_GH1V, C_GFINAL, C_GU34,
  C_GPOOL, C_GH2, C_GME2, C_GMS2, C_GHN2, C_GHE2, C_GH1B,
  C_GME1, C_GMS1, C_GHN1, C_GHE1,
  C_GPN2, C_GPE2, C_GPN1, C_GPE1,
  C_GPRE1E, C_GPRE1S,
  // LN-out grad rows (gu = W^T gpre), stored by the data-bwd kernels for
  // the LN gamma/beta reductions in cs_bwd_w
  C_GU_M2E, C_GU_M2S, C_GU_H2, C_GU_E2, C_GU_M1E, C_GU_M1S, C_GU_Z1,
  C_GU_E1,
  // row-split wgrad partial sums: [6 jobs][WSPLIT][WG_JSTRIDE]
  C_WG_SCRATCH,
  C_NT
};

// The six row-heavy wgrad jobs (module weight grads over N/E rows) are
// row-split WSPLIT ways — a single workgroup per job leaves one CU
// streaming ~4 MB from HBM while the other 255 idle (measured 85 us, 22%
// of the fused step).  Partials land in wg_scratch in a FIXED layout and
// a 6-block reduce kernel sums them in fixed split order: deterministic,
// no atomics.  WG_JSTRIDE = max(Din*Dout) + max(Dout) + 2*max(Din).
#define WSPLIT 16
#define WG_JSTRIDE (KMSG * KHID + KHID + KHID + KHID)

// weight slots within OFFS (order fixed; mirror _fused_offsets in Python)
enum {
  W_LN_N1_W = 0, W_LN_N1_B, W_N1_W, W_N1_B,
  W_LN_E1_W, W_LN_E1_B, W_E1_W, W_E1_B,
  W_LN_R1_W, W_LN_R1_B, W_R1_W, W_R1_B,
  W_LN_N2_W, W_LN_N2_B, W_N2_W, W_N2_B,
  W_LN_E2_W, W_LN_E2_B, W_E2_W, W_E2_B,
  W_LN_R2_W, W_LN_R2_B, W_R2_W, W_R2_B,
  W_LN_G_W, W_LN_G_B, W_G_W, W_G_B,
  W_P1_W, W_P1_B, W_P2_W, W_P2_B,
  W_V1_W, W_V1_B, W_V2_W, W_V2_B,
  W_COUNT
};

struct CachedDims {
  int N, E, M, B, A;
  int F0, FE, H, MSG, HID, OUT, GFin, GEMB, FIN, FC;
  int wgrad_mfma;   // DDLS_AMD_WGRAD_MFMA=1: matrix-core weight grads.
                    // Default VALU: measured A/B at the tuned tile sizes
                    // (gW <= 64x64, ds_read-latency-bound) has the tiled
                    // VALU contraction ~3% faster end-to-end (6.68k vs
                    // 6.50k env-steps/s) — MFMA's 16x16x4 chains leave the
                    // wave latency-exposed at 1-2 accumulators.
  float clip, vf_clip, vf_coef, ent_coef;
};

struct CachedPtrs {
  const float *z0, *e, *gf, *mask, *old_logp, *adv, *vtarg, *kl;
  const long *src, *dst, *order, *indptr, *src_order, *src_indptr;
  const long *node_model, *model_nptr, *model_ids, *actions;
  const float *flat_p;
  float *flat_g;
  const long *offs;
  float *hn1, *he1, *re1, *rs1, *h1;
  float *hn2, *he2, *re2, *rs2, *h2, *pooled;
  float *xh_z1, *xh_e1, *xh_m1e, *xh_m1s, *rst_z1, *rst_e1, *rst_m1e,
        *rst_m1s;
  float *xh_h2, *xh_e2, *xh_m2e, *xh_m2s, *rst_h2, *rst_e2, *rst_m2e,
        *rst_m2s;
  float *xh34, *fin, *h1p, *h1v, *values, *p, *lp, *coef, *hent, *stats;
  float *glogits, *gvalue, *gh1p, *gh1v, *gfinal, *gu34;
  float *gpool, *gh2, *gme2, *gms2, *ghn2, *ghe2, *gh1b;
  float *gme1, *gms1, *ghn1, *ghe1;
  float *gpn2, *gpe2, *gpn1, *gpe1;
  float *gpre1_e, *gpre1_s;
  float *gu_m2e, *gu_m2s, *gu_h2, *gu_e2, *gu_m1e, *gu_m1s, *gu_z1, *gu_e1;
  float *wg_scratch;
};

#define WP(slot) (P.flat_p + P.offs[slot])
#define WG_(slot) (P.flat_g + P.offs[slot])

// LayerNorm into a REGISTER xhat array (fully unrolled: constant Dd), also
// spilled to the global xhat row for the backward.  One thread per row.
template <int Dd>
__device__ __forceinline__ float ln_row_reg(const float* __restrict__ x,
                                            float* __restrict__ xhat_reg,
                                            float* __restrict__ xhat_out) {
  float mu = 0.f;
#pragma unroll
  for (int i = 0; i < Dd; ++i) mu += x[i];
  mu /= Dd;
  float var = 0.f;
#pragma unroll
  for (int i = 0; i < Dd; ++i) { float d = x[i] - mu; var += d * d; }
  var /= Dd;
  float rstd = rsqrtf(var + LN_EPS);
#pragma unroll
  for (int i = 0; i < Dd; ++i) {
    xhat_reg[i] = (x[i] - mu) * rstd;
    xhat_out[i] = xhat_reg[i];
  }
  return rstd;
}

// one MeanPool "row MLP": out = relu(Lin(LNaffine(x))); weights from LDS
template <int Din, int Dout>
__device__ __forceinline__ void row_mlp_fwd_t(
    const float* __restrict__ x, const float* __restrict__ gam,
    const float* __restrict__ bet, const float* __restrict__ W,
    const float* __restrict__ b, float* __restrict__ xhat_out,
    float* __restrict__ rstd_out, float* __restrict__ out) {
  float xh[Din];
  *rstd_out = ln_row_reg<Din>(x, xh, xhat_out);
  float u[Din];
#pragma unroll
  for (int i = 0; i < Din; ++i) u[i] = xh[i] * gam[i] + bet[i];
#pragma unroll 2
  for (int o = 0; o < Dout; ++o) {
    float acc = b[o];
#pragma unroll
    for (int i = 0; i < Din; ++i) acc += W[o * Din + i] * u[i];
    out[o] = acc > 0.f ? acc : 0.f;
  }
}

// cooperative LDS stage of one module's (gam, bet, W, b)
template <int Din, int Dout>
__device__ __forceinline__ void stage_module(const CachedPtrs& P, int w_slot,
                                             int tid, int NT, float* sGam,
                                             float* sBet, float* sW,
                                             float* sB) {
  for (int i = tid; i < Din; i += NT) {
    sGam[i] = WP(w_slot)[i];
    sBet[i] = WP(w_slot + 1)[i];
  }
  for (int x = tid; x < Din * Dout; x += NT) sW[x] = WP(w_slot + 2)[x];
  for (int o = tid; o < Dout; o += NT) sB[o] = WP(w_slot + 3)[o];
}

// backward of one row-MLP row: gpre = gout*(out>0) stored; gu = W^T gpre
// stored; optional input grad via the LN backward.
template <int Din, int Dout>
__device__ __forceinline__ void row_mlp_bwd_row_t(
    const float* __restrict__ gout,
    const float* __restrict__ out, const float* __restrict__ xhat,
    float rstd, const float* __restrict__ gam,
    const float* __restrict__ W, float* __restrict__ gpre_store,
    float* __restrict__ gu_store, float* __restrict__ gin /*or null*/) {
  float gpre[Dout];
#pragma unroll
  for (int o = 0; o < Dout; ++o) {
    gpre[o] = out[o] > 0.f ? gout[o] : 0.f;
    gpre_store[o] = gpre[o];
  }
  float gu[Din];
#pragma unroll 2
  for (int i = 0; i < Din; ++i) {
    float acc = 0.f;
#pragma unroll
    for (int o = 0; o < Dout; ++o) acc += W[o * Din + i] * gpre[o];
    gu[i] = acc;
    gu_store[i] = acc;
  }
  if (gin != nullptr) {
    float xh[Din];
#pragma unroll
    for (int i = 0; i < Din; ++i) xh[i] = xhat[i];
    float m1 = 0.f, m2 = 0.f;
#pragma unroll
    for (int i = 0; i < Din; ++i) {
      float gh = gu[i] * gam[i];
      m1 += gh;
      m2 += gh * xh[i];
    }
    m1 /= Din;
    m2 /= Din;
#pragma unroll
    for (int i = 0; i < Din; ++i) {
      float gh = gu[i] * gam[i];
      gin[i] = rstd * (gh - m1 - xh[i] * m2);
    }
  }
}

// ===========================================================================
// forward
// ===========================================================================

#define GSTRIDE for (long u = (long)blockIdx.x * blockDim.x + threadIdx.x; \
                            u < total; u += (long)gridDim.x * blockDim.x)

// round MLPs: rows 0..N-1 are node rows, N..N+E-1 are edge rows
template <int ROUND>
__global__ void __launch_bounds__(256)
cs_fwd_mlp_kernel(CachedPtrs P, CachedDims D) {
  constexpr int DN = (ROUND == 1) ? KF0 : KHID;
  __shared__ float sGamN[DN], sBetN[DN], sWN[KH * DN], sBN[KH];
  __shared__ float sGamE[KFE], sBetE[KFE], sWE[KH * KFE], sBE[KH];
  const int tid = threadIdx.x, NT = blockDim.x;
  stage_module<DN, KH>(P, (ROUND == 1) ? W_LN_N1_W : W_LN_N2_W, tid, NT,
                       sGamN, sBetN, sWN, sBN);
  stage_module<KFE, KH>(P, (ROUND == 1) ? W_LN_E1_W : W_LN_E2_W, tid, NT,
                        sGamE, sBetE, sWE, sBE);
  __syncthreads();
  const long total = D.N + D.E;
  GSTRIDE {
    if (u < D.N) {
      const long v = u;
      if (ROUND == 1)
        row_mlp_fwd_t<KF0, KH>(P.z0 + v * KF0, sGamN, sBetN, sWN, sBN,
                               P.xh_z1 + v * KF0, P.rst_z1 + v,
                               P.hn1 + v * KH);
      else
        row_mlp_fwd_t<KHID, KH>(P.h1 + v * KHID, sGamN, sBetN, sWN, sBN,
                                P.xh_h2 + v * KHID, P.rst_h2 + v,
                                P.hn2 + v * KH);
    } else {
      const long k = u - D.N;
      if (ROUND == 1)
        row_mlp_fwd_t<KFE, KH>(P.e + k * KFE, sGamE, sBetE, sWE, sBE,
                               P.xh_e1 + k * KFE, P.rst_e1 + k,
                               P.he1 + k * KH);
      else
        row_mlp_fwd_t<KFE, KH>(P.e + k * KFE, sGamE, sBetE, sWE, sBE,
                               P.xh_e2 + k * KFE, P.rst_e2 + k,
                               P.he2 + k * KH);
    }
  }
}

template <int ROUND>
__global__ void __launch_bounds__(256)
cs_fwd_reduce_kernel(CachedPtrs P, CachedDims D) {
  constexpr int DO = (ROUND == 1) ? KHID : KOUT;
  __shared__ float sGam[KMSG], sBet[KMSG], sW[DO * KMSG], sB[DO];
  const int tid = threadIdx.x, NT = blockDim.x;
  stage_module<KMSG, DO>(P, (ROUND == 1) ? W_LN_R1_W : W_LN_R2_W, tid, NT,
                         sGam, sBet, sW, sB);
  __syncthreads();
  const float* hn = (ROUND == 1) ? P.hn1 : P.hn2;
  const float* he = (ROUND == 1) ? P.he1 : P.he2;
  const long total = D.E + D.N;
  GSTRIDE {
    float msg[KMSG];
    if (u < D.E) {
      const long k = u;
      const long sv = P.src[k];
#pragma unroll
      for (int i = 0; i < KH; ++i) msg[i] = hn[sv * KH + i];
#pragma unroll
      for (int i = 0; i < KH; ++i) msg[KH + i] = he[k * KH + i];
      if (ROUND == 1)
        row_mlp_fwd_t<KMSG, KHID>(msg, sGam, sBet, sW, sB,
                                  P.xh_m1e + k * KMSG,
                                  P.rst_m1e + k, P.re1 + k * KHID);
      else
        row_mlp_fwd_t<KMSG, KOUT>(msg, sGam, sBet, sW, sB,
                                  P.xh_m2e + k * KMSG,
                                  P.rst_m2e + k, P.re2 + k * KOUT);
    } else {
      const long v = u - D.E;
#pragma unroll
      for (int i = 0; i < KH; ++i) msg[i] = hn[v * KH + i];
#pragma unroll
      for (int i = 0; i < KH; ++i) msg[KH + i] = 0.f;
      if (ROUND == 1)
        row_mlp_fwd_t<KMSG, KHID>(msg, sGam, sBet, sW, sB,
                                  P.xh_m1s + v * KMSG,
                                  P.rst_m1s + v, P.rs1 + v * KHID);
      else
        row_mlp_fwd_t<KMSG, KOUT>(msg, sGam, sBet, sW, sB,
                                  P.xh_m2s + v * KMSG,
                                  P.rst_m2s + v, P.rs2 + v * KOUT);
    }
  }
}

template <int ROUND>
__global__ void __launch_bounds__(256)
cs_fwd_combine_kernel(CachedPtrs P, CachedDims D) {
  const int DO = (ROUND == 1) ? KHID : KOUT;
  const float* re = (ROUND == 1) ? P.re1 : P.re2;
  const float* rs = (ROUND == 1) ? P.rs1 : P.rs2;
  float* h = (ROUND == 1) ? P.h1 : P.h2;
  const long total = (long)D.N * DO;
  GSTRIDE {
    int v = (int)(u / DO), i = (int)(u % DO);
    long lo = P.indptr[v], hi = P.indptr[v + 1];
    float out = 0.f;
    if (hi > lo) {
      float acc = rs[(long)v * DO + i];
      for (long q = lo; q < hi; ++q)
        acc += re[P.order[q] * DO + i];
      out = acc / (float)(hi - lo + 1);
    }
    h[(long)v * DO + i] = out;
  }
}

// pool (M x OUT) then per-sample `final` (one WG: final depends on pooled)
__global__ void __launch_bounds__(512)
cs_fwd_pool_kernel(CachedPtrs P, CachedDims D) {
  const int tid = threadIdx.x;
  const int NT = blockDim.x;
  constexpr int PT = 256;   // node rows of h2 staged per tile
  __shared__ float sH2[PT * KOUT];
  __shared__ float sGam[KGF], sBet[KGF], sWg[KGE * KGF], sBg[KGE];
  for (int i = tid; i < KGF; i += NT) {
    sGam[i] = WP(W_LN_G_W)[i];
    sBet[i] = WP(W_LN_G_B)[i];
  }
  for (int x = tid; x < KGE * KGF; x += NT) sWg[x] = WP(W_G_W)[x];
  for (int o = tid; o < KGE; o += NT) sBg[o] = WP(W_G_B)[o];
  // per-model means: h2 goes through LDS tile by tile; each (m, i) unit
  // adds its model's nodes in node order, as a chain out of LDS
  const int units = D.M * KOUT;
  for (int ub = 0; ub < units; ub += NT) {
    const int u = ub + tid;
    const int m = u / KOUT, i = u % KOUT;
    long lo = 0, hi = 0;
    if (u < units) { lo = P.model_nptr[m]; hi = P.model_nptr[m + 1]; }
    float acc = 0.f;
    for (long v0 = 0; v0 < D.N; v0 += PT) {
      const long v1 = min((long)D.N, v0 + PT);
      __syncthreads();
      for (long x = tid; x < (v1 - v0) * KOUT; x += NT)
        sH2[x] = P.h2[v0 * KOUT + x];
      __syncthreads();
      const long a = max(lo, v0), e = min(hi, v1);
      for (long v = a; v < e; ++v) acc += sH2[(v - v0) * KOUT + i];
    }
    if (u < units) P.pooled[(long)m * KOUT + i] = acc / (float)(hi - lo);
  }
  __syncthreads();
  for (int b = tid; b < D.B; b += NT) {
    const long mid = P.model_ids[b];
    float* fin = P.fin + (long)b * KFIN;
#pragma unroll
    for (int i = 0; i < KOUT; ++i) fin[i] = P.pooled[mid * KOUT + i];
    float xh[KGF];
    ln_row_reg<KGF>(P.gf + (long)b * KGF, xh, P.xh34 + (long)b * KGF);
    const float* __restrict__ gam = sGam;
    const float* __restrict__ bet = sBet;
    const float* __restrict__ Wg = sWg;
    const float* __restrict__ bg = sBg;
    float uu[KGF];
#pragma unroll
    for (int i = 0; i < KGF; ++i) uu[i] = xh[i] * gam[i] + bet[i];
    // not unrolled over o: with the weights in LDS a full unroll hoists all
    // KGE*KGF reads and spills
#pragma unroll 1
    for (int o = 0; o < KGE; ++o) {
      float acc = bg[o];
#pragma unroll
      for (int i = 0; i < KGF; ++i) acc += Wg[o * KGF + i] * uu[i];
      fin[KOUT + o] = acc;               // graph_module has NO activation
    }
  }
}

// FC branches: one thread per (b, hidden j) unit; W1p/W1v rows via L1/L2
__global__ void __launch_bounds__(256)
cs_fwd_head_kernel(CachedPtrs P, CachedDims D) {
  const long total = (long)D.B * KFC;
  for (long u = blockIdx.x * blockDim.x + threadIdx.x; u < total;
       u += (long)gridDim.x * blockDim.x) {
    int b = (int)(u / KFC), j = (int)(u % KFC);
    const float* fin = P.fin + (long)b * KFIN;
    const float* W1p = WP(W_P1_W);
    const float* W1v = WP(W_V1_W);
    float ap = WP(W_P1_B)[j], av = WP(W_V1_B)[j];
#pragma unroll 4
    for (int i = 0; i < KFIN; ++i) {
      ap += W1p[j * KFIN + i] * fin[i];
      av += W1v[j * KFIN + i] * fin[i];
    }
    P.h1p[u] = ap > 0.f ? ap : 0.f;
    P.h1v[u] = av > 0.f ? av : 0.f;
  }
}

// logits+value rows + loss (1 WG so the stats reduction stays in-block)
// final logit/value projection, one block per SAMPLE: the previous
// 32-samples-per-block layout ran the whole [B,17]x[17,256] contraction on
// 4 workgroups (one serial 256-wide loop per sample-thread, 39 us); here
// 128 blocks tile (action x 16-chunk) over 272 threads with an LDS
// partial-sum reduce — fixed order, deterministic
__global__ void __launch_bounds__(512)
cs_fwd_logits_kernel(CachedPtrs P, CachedDims D) {
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  __shared__ float shp[KFC], shv[KFC];
  __shared__ float part[KA][16];
  __shared__ float vred[256];
  const float* __restrict__ hp = P.h1p + (long)b * KFC;
  const float* __restrict__ hv = P.h1v + (long)b * KFC;
  for (int x = tid; x < KFC; x += 512) {
    shp[x] = hp[x];
    shv[x] = hv[x];
  }
  __syncthreads();
  if (tid < KA * 16) {
    const int a = tid / 16, c = tid % 16;
    const float* __restrict__ w = WP(W_P2_W) + (long)a * KFC + c * 16;
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) s += w[i] * shp[c * 16 + i];
    part[a][c] = s;
  }
  if (tid < 256) vred[tid] = WP(W_V2_W)[tid] * shv[tid];
  __syncthreads();
  for (int sft = 128; sft > 0; sft >>= 1) {
    if (tid < sft) vred[tid] += vred[tid + sft];
    __syncthreads();
  }
  if (tid < KA) {
    float acc = WP(W_P2_B)[tid];
#pragma unroll
    for (int c = 0; c < 16; ++c) acc += part[tid][c];
    const float fmin = -3.402823466e+38f;
    float lm = logf(P.mask[(long)b * KA + tid]);
    if (!(lm > fmin)) lm = fmin;
    P.p[(long)b * KA + tid] = acc + lm;   // raw masked logits
  }
  if (tid == 0) P.values[b] = vred[0] + WP(W_V2_B)[0];
}

__global__ void __launch_bounds__(256)
cs_fwd_loss_kernel(CachedPtrs P, CachedDims D) {
  const int tid = threadIdx.x;
  const int NT = blockDim.x;
  const int b_lo = blockIdx.x * 32;
  const int b_hi = min(D.B, b_lo + 32);
  __shared__ float acc_s[4];
  if (tid < 4) acc_s[tid] = 0.f;
  __syncthreads();
  for (int b = b_lo + tid; b < b_hi; b += NT) {
    float* row = P.p + (long)b * KA;
    float mx = -3.0e38f;
    for (int a = 0; a < KA; ++a) mx = fmaxf(mx, row[a]);
    float Z = 0.f;
    for (int a = 0; a < KA; ++a) Z += __expf(row[a] - mx);
    float lse = mx + __logf(Z);
    float ent = 0.f;
    for (int a = 0; a < KA; ++a) {
      float lp = row[a] - lse;
      P.lp[(long)b * KA + a] = lp;
      ent -= __expf(lp) * lp;
    }
    for (int a = 0; a < KA; ++a)
      row[a] = __expf(P.lp[(long)b * KA + a]);
    const long a = P.actions[b];
    const float logp_a = P.lp[(long)b * KA + a];
    const float ratio = __expf(logp_a - P.old_logp[b]);
    const float A_b = P.adv[b];
    const float r_cl = fminf(fmaxf(ratio, 1.f - D.clip), 1.f + D.clip);
    const float surr1 = ratio * A_b, surr2 = r_cl * A_b;
    const float surr = fminf(surr1, surr2);
    float ds = ratio * A_b;
    if (surr2 < surr1 && (ratio < 1.f - D.clip || ratio > 1.f + D.clip))
      ds = 0.f;
    const float kl_b = P.old_logp[b] - logp_a;
    const float verr = P.values[b] - P.vtarg[b];
    const float vf_b = fminf(verr * verr, D.vf_clip);
    P.hent[b] = ent;
    P.coef[b] = -ds - P.kl[0];
    atomicAdd(&acc_s[0], -surr);
    atomicAdd(&acc_s[1], vf_b);
    atomicAdd(&acc_s[2], kl_b);
    atomicAdd(&acc_s[3], ent);
  }
  __syncthreads();
  if (tid == 0) {
    // cross-block accumulation: float atomics (stats are logging-only; the
    // gradient path is deterministic elsewhere)
    const float inv = 1.f / D.B;
    const float pl = acc_s[0] * inv;
    const float vf = acc_s[1] * inv;
    const float kl = acc_s[2] * inv;
    const float ent = acc_s[3] * inv;
    atomicAdd(&P.stats[0], pl);
    atomicAdd(&P.stats[1], vf);
    atomicAdd(&P.stats[2], kl);
    atomicAdd(&P.stats[3], ent);
    atomicAdd(&P.stats[4],
              pl + P.kl[0] * kl + D.vf_coef * vf - D.ent_coef * ent);
  }
}

// ===========================================================================
// backward
// ===========================================================================

// per-SAMPLE chain: each block owns a contiguous sample range, so every
// cross-unit dependency (glogits row -> gh1 row -> gfinal row) stays inside
// the block.  256 threads cooperate FC-wise within each sample.
__global__ void __launch_bounds__(256)
cs_bwd_head_kernel(CachedPtrs P, CachedDims D) {
  __shared__ float sW2p[KA * KFC], sW2v[KFC];
  __shared__ float sW1p[KFC * KFIN], sW1v[KFC * KFIN], sWg[KGE * KGF];
  constexpr int HS = 4;   // samples in flight per block
  // per-sample rows; +1 keeps the HS rows of one column on distinct banks
  __shared__ float sGL[HS][KA], sGV[HS], sGF[HS][KFIN];
  __shared__ float sGHp[HS][KFC + 1], sGHv[HS][KFC + 1];
  const int tid = threadIdx.x;
  const int NT = blockDim.x;
  for (int x = tid; x < KA * KFC; x += NT) sW2p[x] = WP(W_P2_W)[x];
  for (int x = tid; x < KFC; x += NT) sW2v[x] = WP(W_V2_W)[x];
  for (int x = tid; x < KFC * KFIN; x += NT) {
    sW1p[x] = WP(W_P1_W)[x];
    sW1v[x] = WP(W_V1_W)[x];
  }
  for (int x = tid; x < KGE * KGF; x += NT) sWg[x] = WP(W_G_W)[x];
  __syncthreads();
  const int per = (D.B + gridDim.x - 1) / gridDim.x;
  const int b0 = blockIdx.x * per;
  const int b1 = min(D.B, b0 + per);
  // HS samples go through the phases side by side; each sample's rows stay
  // in LDS between phases (they are also written out for cs_bwd_w), so no
  // phase waits on a global store -> load round trip.
  for (int c0 = b0; c0 < b1; c0 += HS) {
    const int ns = min(HS, b1 - c0);
    // loss backward rows (upstream grad = 1)
    for (int x = tid; x < ns * KA; x += NT) {
      const int s = x / KA, a = x % KA;
      const int b = c0 + s;
      const long u = (long)b * KA + a;
      const long act = P.actions[b];
      const float c = P.coef[b] / D.B;
      const float pj = P.p[u];
      const float lpj = P.lp[u];
      const float delta = (a == (int)act) ? 1.f : 0.f;
      const float gl = mul_rn(c, delta - pj)
                       + mul_rn(mul_rn(D.ent_coef / D.B, pj),
                                lpj + P.hent[b]);
      P.glogits[u] = gl;
      sGL[s][a] = gl;
    }
    if (tid >= 128 && tid < 128 + ns) {
      const int s = tid - 128;
      const int b = c0 + s;
      const float verr = P.values[b] - P.vtarg[b];
      const float mk = (verr * verr <= D.vf_clip) ? 1.f : 0.f;
      const float gv = D.vf_coef * 2.f * verr * mk / D.B;
      P.gvalue[b] = gv;
      sGV[s] = gv;
    }
    __syncthreads();
    // hidden grads
    for (int x = tid; x < ns * KFC; x += NT) {
      const int s = x / KFC, j = x % KFC;
      const long u = (long)(c0 + s) * KFC + j;
      float acc = 0.f;
#pragma unroll
      for (int a = 0; a < KA; ++a) {
        // the first five terms are fused, the rest rounded products
        if (a < 5) acc = FMA(sW2p[a * KFC + j], sGL[s][a], acc);
        else acc = acc + mul_rn(sW2p[a * KFC + j], sGL[s][a]);
      }
      const float gp = P.h1p[u] > 0.f ? acc : 0.f;
      const float av = sW2v[j] * sGV[s];
      const float gv = P.h1v[u] > 0.f ? av : 0.f;
      P.gh1p[u] = gp;
      P.gh1v[u] = gv;
      sGHp[s][j] = gp;
      sGHv[s][j] = gv;
    }
    __syncthreads();
    // gfinal: one thread per (sample, i), j = 0..FC-1 in order
    for (int x = tid; x < ns * KFIN; x += NT) {
      const int s = x / KFIN, i = x % KFIN;
      float acc = 0.f;
#pragma unroll 8
      for (int j = 0; j < KFC; ++j) {
        acc = FMA(sW1p[j * KFIN + i], sGHp[s][j], acc);
        acc = FMA(sW1v[j * KFIN + i], sGHv[s][j], acc);
      }
      P.gfinal[(long)(c0 + s) * KFIN + i] = acc;
      sGF[s][i] = acc;
    }
    __syncthreads();
    // graph-module LN-out grads
    for (int x = tid; x < ns * KGF; x += NT) {
      const int s = x / KGF, i = x % KGF;
      float acc = 0.f;
#pragma unroll
      for (int o = 0; o < KGE; ++o)
        acc = acc + mul_rn(sWg[o * KGF + i], sGF[s][KOUT + o]);
      P.gu34[(long)(c0 + s) * KGF + i] = acc;
    }
    // no barrier here: every row buffer's next write is at least one
    // barrier after its last read above
  }
}

// pool grads -> gh2 (1 WG: gh2 depends on gpool; both tiny)
__global__ void __launch_bounds__(512)
cs_bwd_pool_kernel(CachedPtrs P, CachedDims D) {
  const int tid = threadIdx.x;
  const int NT = blockDim.x;
  __shared__ int smid[1024];
  for (int b = tid; b < D.B; b += NT) smid[b] = (int)P.model_ids[b];
  __syncthreads();
  // gfinal[:, :KOUT] goes through LDS in tiles of BT samples; each (m, i)
  // unit still adds b = 0..B-1 in order
  constexpr int BT = 128;
  __shared__ float sG[BT][KOUT];
  const int units = D.M * KOUT;
  for (int ub = 0; ub < units; ub += NT) {
    const int u = ub + tid;
    const int m = u / KOUT, i = u % KOUT;
    float acc = 0.f;
    for (int t0 = 0; t0 < D.B; t0 += BT) {
      const int bt = min(BT, D.B - t0);
      __syncthreads();
      for (int x = tid; x < bt * KOUT; x += NT)
        sG[x / KOUT][x % KOUT] = P.gfinal[(long)(t0 + x / KOUT) * KFIN
                                          + x % KOUT];
      __syncthreads();
      if (bt == BT) {
#pragma unroll 8
        for (int b = 0; b < BT; ++b)
          acc += (smid[t0 + b] == m) ? sG[b][i] : 0.f;
      } else {
        for (int b = 0; b < bt; ++b)
          acc += (smid[t0 + b] == m) ? sG[b][i] : 0.f;
      }
    }
    if (u < units) P.gpool[u] = acc;
  }
  __syncthreads();
  for (long u = tid; u < (long)D.N * KOUT; u += NT) {
    int v = (int)(u / KOUT), i = (int)(u % KOUT);
    const long m = P.node_model[v];
    const float nn = (float)(P.model_nptr[m + 1] - P.model_nptr[m]);
    P.gh2[u] = P.gpool[m * KOUT + i] / nn;
  }
}

// reduce-module backward rows (edge rows then self rows)
template <int ROUND>
__global__ void __launch_bounds__(256)
cs_bwd_reduce_kernel(CachedPtrs P, CachedDims D) {
  constexpr int DO = (ROUND == 1) ? KHID : KOUT;
  constexpr int SLOT = (ROUND == 1) ? W_LN_R1_W : W_LN_R2_W;
  __shared__ float sGam[KMSG], sW[DO * KMSG];
  const int tid = threadIdx.x, NT = blockDim.x;
  for (int i = tid; i < KMSG; i += NT) sGam[i] = WP(SLOT)[i];
  for (int x = tid; x < DO * KMSG; x += NT) sW[x] = WP(SLOT + 2)[x];
  __syncthreads();
  const long total = D.E + D.N;
  GSTRIDE {
    if (ROUND == 2) {
      float gr[KOUT];
      if (u < D.E) {
        const long k = u;
        const int v = (int)P.dst[k];
        const long deg = P.indptr[v + 1] - P.indptr[v];
        const float f = 1.f / (float)(deg + 1);
#pragma unroll
        for (int i = 0; i < KOUT; ++i)
          gr[i] = P.gh2[(long)v * KOUT + i] * f;
        row_mlp_bwd_row_t<KMSG, KOUT>(gr, P.re2 + k * KOUT,
                                      P.xh_m2e + k * KMSG, P.rst_m2e[k],
                                      sGam, sW, P.gpe2 + k * KOUT,
                                      P.gu_m2e + k * KMSG,
                                      P.gme2 + k * KMSG);
      } else {
        const long v = u - D.E;
        const long deg = P.indptr[v + 1] - P.indptr[v];
        const float f = (deg > 0) ? 1.f / (float)(deg + 1) : 0.f;
#pragma unroll
        for (int i = 0; i < KOUT; ++i)
          gr[i] = P.gh2[v * KOUT + i] * f;
        row_mlp_bwd_row_t<KMSG, KOUT>(gr, P.rs2 + v * KOUT,
                                      P.xh_m2s + v * KMSG, P.rst_m2s[v],
                                      sGam, sW, P.gpn2 + v * KOUT,
                                      P.gu_m2s + v * KMSG,
                                      P.gms2 + v * KMSG);
      }
    } else {
      float gr[KHID];
      if (u < D.E) {
        const long k = u;
        const int v = (int)P.dst[k];
        const long deg = P.indptr[v + 1] - P.indptr[v];
        const float f = 1.f / (float)(deg + 1);
#pragma unroll
        for (int i = 0; i < KHID; ++i)
          gr[i] = P.gh1b[(long)v * KHID + i] * f;
        row_mlp_bwd_row_t<KMSG, KHID>(gr, P.re1 + k * KHID,
                                      P.xh_m1e + k * KMSG, P.rst_m1e[k],
                                      sGam, sW, P.gpre1_e + k * KHID,
                                      P.gu_m1e + k * KMSG,
                                      P.gme1 + k * KMSG);
      } else {
        const long v = u - D.E;
        const long deg = P.indptr[v + 1] - P.indptr[v];
        const float f = (deg > 0) ? 1.f / (float)(deg + 1) : 0.f;
#pragma unroll
        for (int i = 0; i < KHID; ++i)
          gr[i] = P.gh1b[v * KHID + i] * f;
        row_mlp_bwd_row_t<KMSG, KHID>(gr, P.rs1 + v * KHID,
                                      P.xh_m1s + v * KMSG, P.rst_m1s[v],
                                      sGam, sW, P.gpre1_s + v * KHID,
                                      P.gu_m1s + v * KMSG,
                                      P.gms1 + v * KMSG);
      }
    }
  }
}

// scatter message grads back to hn/he (ROUND 2 plain; ROUND 1 also applies
// the relu mask in place, producing the module-1 gpre rows)
template <int ROUND>
__global__ void __launch_bounds__(256)
cs_bwd_scatter_kernel(CachedPtrs P, CachedDims D) {
  const float* gme = (ROUND == 1) ? P.gme1 : P.gme2;
  const float* gms = (ROUND == 1) ? P.gms1 : P.gms2;
  const long total = (long)(D.N + D.E) * KH;
  GSTRIDE {
    if (u < (long)D.N * KH) {
      int v = (int)(u / KH), i = (int)(u % KH);
      long lo = P.src_indptr[v], hi = P.src_indptr[v + 1];
      float acc = gms[(long)v * KMSG + i];
      for (long q = lo; q < hi; ++q)
        acc += gme[P.src_order[q] * KMSG + i];
      if (ROUND == 1)
        P.ghn1[u] = P.hn1[u] > 0.f ? acc : 0.f;
      else
        P.ghn2[u] = acc;
    } else {
      const long x = u - (long)D.N * KH;
      int k = (int)(x / KH), i = (int)(x % KH);
      float g = gme[(long)k * KMSG + KH + i];
      if (ROUND == 1)
        P.ghe1[x] = P.he1[x] > 0.f ? g : 0.f;
      else
        P.ghe2[x] = g;
    }
  }
}

// round-2 node/edge module data backward (node rows produce gh1)
__global__ void __launch_bounds__(256)
cs_bwd_mlp2_kernel(CachedPtrs P, CachedDims D) {
  __shared__ float sGamN[KHID], sWN[KH * KHID];
  __shared__ float sGamE[KFE], sWE[KH * KFE];
  const int tid = threadIdx.x, NT = blockDim.x;
  for (int i = tid; i < KHID; i += NT) sGamN[i] = WP(W_LN_N2_W)[i];
  for (int x = tid; x < KH * KHID; x += NT) sWN[x] = WP(W_N2_W)[x];
  for (int i = tid; i < KFE; i += NT) sGamE[i] = WP(W_LN_E2_W)[i];
  for (int x = tid; x < KH * KFE; x += NT) sWE[x] = WP(W_E2_W)[x];
  __syncthreads();
  const long total = D.N + D.E;
  GSTRIDE {
    if (u < D.N) {
      const long v = u;
      row_mlp_bwd_row_t<KHID, KH>(P.ghn2 + v * KH, P.hn2 + v * KH,
                                  P.xh_h2 + v * KHID, P.rst_h2[v],
                                  sGamN, sWN, P.gpn1 + v * KH,
                                  P.gu_h2 + v * KHID, P.gh1b + v * KHID);
    } else {
      const long k = u - D.N;
      row_mlp_bwd_row_t<KFE, KH>(P.ghe2 + k * KH, P.he2 + k * KH,
                                 P.xh_e2 + k * KFE, P.rst_e2[k],
                                 sGamE, sWE, P.gpe1 + k * KH,
                                 P.gu_e2 + k * KFE, nullptr);
    }
  }
}

// module-1 LN-out grad rows (gu = W^T gpre; inputs static, no input grads)
__global__ void __launch_bounds__(256)
cs_bwd_gu1_kernel(CachedPtrs P, CachedDims D) {
  __shared__ float sWN[KH * KF0], sWE[KH * KFE];
  const int tid = threadIdx.x, NT = blockDim.x;
  for (int x = tid; x < KH * KF0; x += NT) sWN[x] = WP(W_N1_W)[x];
  for (int x = tid; x < KH * KFE; x += NT) sWE[x] = WP(W_E1_W)[x];
  __syncthreads();
  const long total = D.N + D.E;
  GSTRIDE {
    if (u < D.N) {
      const long v = u;
      const float* __restrict__ W = sWN;
      float g[KH];
#pragma unroll
      for (int o = 0; o < KH; ++o) g[o] = P.ghn1[v * KH + o];
#pragma unroll
      for (int i = 0; i < KF0; ++i) {
        float acc = 0.f;
#pragma unroll
        for (int o = 0; o < KH; ++o) acc += W[o * KF0 + i] * g[o];
        P.gu_z1[v * KF0 + i] = acc;
      }
    } else {
      const long k = u - D.N;
      const float* __restrict__ W = sWE;
      float g[KH];
#pragma unroll
      for (int o = 0; o < KH; ++o) g[o] = P.ghe1[k * KH + o];
#pragma unroll
      for (int i = 0; i < KFE; ++i) {
        float acc = 0.f;
#pragma unroll
        for (int o = 0; o < KH; ++o) acc += W[o * KFE + i] * g[o];
        P.gu_e1[k * KFE + i] = acc;
      }
    }
  }
}

// ---------------------------------------------------------------------------
// weight gradients: one block per weight-matrix job, LDS-tiled over rows.
// Each job: gW[Dout,Din] = sum_r gpre[r,:] (x) u[r,:]  with u = xh*gam+bet,
// rows drawn from one or two sources (edge rows ++ self rows); bias grads
// accumulated from the same tiles; LN gamma/beta grads from stored gu rows.
// Deterministic: fixed tile order, no atomics.
// ---------------------------------------------------------------------------

#define TILE_K 32

template <int Din, int Dout>
__device__ __forceinline__ void wgrad_tiled(
    const CachedPtrs& P, int tid, int NT, int rows0, int rows1,
    const float* __restrict__ gpre0, const float* __restrict__ gpre1,
    const float* __restrict__ xh0, const float* __restrict__ xh1,
    const float* __restrict__ gu0, const float* __restrict__ gu1,
    int w_slot, float (*tG)[65], float (*tU)[65], float (*tGU)[65],
    float (*tXH)[65], int split = 0, int nsplit = 1,
    float* __restrict__ pout = nullptr) {
  const float* __restrict__ gam = WP(w_slot);
  const float* __restrict__ bet = WP(w_slot + 1);
  constexpr int UNITS = Din * Dout;
  constexpr int MYU = (UNITS + 255) / 256;
  float acc[MYU];
#pragma unroll
  for (int q = 0; q < MYU; ++q) acc[q] = 0.f;
  float bacc = 0.f, lacc_w = 0.f, lacc_b = 0.f;
  const int rows = rows0 + rows1;
  for (int r0 = split * TILE_K; r0 < rows; r0 += nsplit * TILE_K) {
    const int rt = min(TILE_K, rows - r0);
    for (int x = tid; x < rt * Dout; x += NT) {
      int t = x / Dout, o = x % Dout;
      int r = r0 + t;
      tG[t][o] = (r < rows0) ? gpre0[(long)r * Dout + o]
                             : gpre1[(long)(r - rows0) * Dout + o];
    }
    for (int x = tid; x < rt * Din; x += NT) {
      int t = x / Din, i = x % Din;
      int r = r0 + t;
      float xh = (r < rows0) ? xh0[(long)r * Din + i]
                             : xh1[(long)(r - rows0) * Din + i];
      tU[t][i] = xh * gam[i] + bet[i];
      tXH[t][i] = xh;
      tGU[t][i] = (r < rows0) ? gu0[(long)r * Din + i]
                              : gu1[(long)(r - rows0) * Din + i];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < MYU; ++q) {
      int u = tid + q * 256;
      if (u < UNITS) {
        int o = u / Din, i = u % Din;
        float a = acc[q];
        if (rt == TILE_K) {
#pragma unroll
          for (int t = 0; t < TILE_K; ++t) a += tG[t][o] * tU[t][i];
        } else {
          for (int t = 0; t < rt; ++t) a += tG[t][o] * tU[t][i];
        }
        acc[q] = a;
      }
    }
    if (tid < Dout)
      for (int t = 0; t < rt; ++t) bacc += tG[t][tid];
    if (tid < Din)
      for (int t = 0; t < rt; ++t) {
        lacc_w += tGU[t][tid] * tXH[t][tid];
        lacc_b += tGU[t][tid];
      }
    __syncthreads();
  }
  if (pout != nullptr) {
    // partial layout: [w UNITS][b Dout][ln_w Din][ln_b Din]
#pragma unroll
    for (int q = 0; q < MYU; ++q) {
      int u = tid + q * 256;
      if (u < UNITS) pout[u] = acc[q];
    }
    if (tid < Dout) pout[UNITS + tid] = bacc;
    if (tid < Din) {
      pout[UNITS + Dout + tid] = lacc_w;
      pout[UNITS + Dout + Din + tid] = lacc_b;
    }
    return;
  }
#pragma unroll
  for (int q = 0; q < MYU; ++q) {
    int u = tid + q * 256;
    if (u < UNITS) WG_(w_slot + 2)[u] = acc[q];
  }
  if (tid < Dout) WG_(w_slot + 3)[tid] = bacc;
  if (tid < Din) {
    WG_(w_slot)[tid] = lacc_w;
    WG_(w_slot + 1)[tid] = lacc_b;
  }
}

// ---------------------------------------------------------------------------
// MFMA weight-grad contraction: gW[Dout,Din] = sum_r gpre[r,:] (x) u[r,:]
// on v_mfma_f32_16x16x4_f32 tiles (exact f32: the result is a k-ordered fmaf
// chain).  A[m][k=r] = gpre[r][m], B[k=r][i] = u[r][i]; per-lane fragments
// A[l&15][l>>4], B[l>>4][l&15]; D col = l&15, row = (l>>4)*4 + reg.
// Rows stream through zero-padded LDS tiles; each WAVE owns a set of 16x16
// C tiles and accumulates across row tiles.  LN gamma/beta + bias grads ride
// along as VALU reductions on the same tiles.
// ---------------------------------------------------------------------------
typedef float f32x4 __attribute__((ext_vector_type(4)));

template <int Din, int Dout, int DinP, int DoutP>
__device__ __forceinline__ void wgrad_tiled_mfma(
    const CachedPtrs& P, int tid, int NT, int rows0, int rows1,
    const float* __restrict__ gpre0, const float* __restrict__ gpre1,
    const float* __restrict__ xh0, const float* __restrict__ xh1,
    const float* __restrict__ gu0, const float* __restrict__ gu1,
    int w_slot, float* ldsG, float* ldsU, float* ldsGU, float* ldsXH) {
  // lds row stride = padded dim (+1 would break MFMA b128 patterns; plain)
  const float* __restrict__ gam = WP(w_slot);
  const float* __restrict__ bet = WP(w_slot + 1);
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int n_waves = NT >> 6;
  constexpr int MT = DoutP / 16;
  constexpr int NTL = DinP / 16;
  constexpr int CT = MT * NTL;                 // 16x16 C tiles
  constexpr int MY_CT = (CT + 3) / 4;          // per wave (4 waves)
  f32x4 acc[MY_CT];
#pragma unroll
  for (int q = 0; q < MY_CT; ++q) acc[q] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float bacc = 0.f, lacc_w = 0.f, lacc_b = 0.f;
  const int rows = rows0 + rows1;
  for (int r0 = 0; r0 < rows; r0 += TILE_K) {
    const int rt = min(TILE_K, rows - r0);
    // zero-fill then stage (padding rows/cols contribute 0 to the MFMA)
    for (int x = tid; x < TILE_K * DoutP; x += NT) ldsG[x] = 0.f;
    for (int x = tid; x < TILE_K * DinP; x += NT) ldsU[x] = 0.f;
    __syncthreads();
    for (int x = tid; x < rt * Dout; x += NT) {
      int t = x / Dout, o = x % Dout;
      int r = r0 + t;
      ldsG[t * DoutP + o] = (r < rows0)
          ? gpre0[(long)r * Dout + o]
          : gpre1[(long)(r - rows0) * Dout + o];
    }
    for (int x = tid; x < rt * Din; x += NT) {
      int t = x / Din, i = x % Din;
      int r = r0 + t;
      float xh = (r < rows0) ? xh0[(long)r * Din + i]
                             : xh1[(long)(r - rows0) * Din + i];
      ldsU[t * DinP + i] = xh * gam[i] + bet[i];
      ldsXH[t * DinP + i] = xh;
      ldsGU[t * DinP + i] = (r < rows0)
          ? gu0[(long)r * Din + i]
          : gu1[(long)(r - rows0) * Din + i];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < MY_CT; ++q) {
      const int ct = wave + q * n_waves;
      if (ct < CT) {
        const int m0 = (ct / NTL) * 16;
        const int n0 = (ct % NTL) * 16;
        f32x4 a = acc[q];
#pragma unroll
        for (int kk = 0; kk < TILE_K; kk += 4) {
          const float af = ldsG[(kk + (lane >> 4)) * DoutP + m0 + (lane & 15)];
          const float bf = ldsU[(kk + (lane >> 4)) * DinP + n0 + (lane & 15)];
          a = __builtin_amdgcn_mfma_f32_16x16x4f32(af, bf, a, 0, 0, 0);
        }
        acc[q] = a;
      }
    }
    // bias + LN grads (VALU, from the same tiles)
    if (tid < Dout)
      for (int t = 0; t < rt; ++t) bacc += ldsG[t * DoutP + tid];
    if (tid < Din)
      for (int t = 0; t < rt; ++t) {
        lacc_w += ldsGU[t * DinP + tid] * ldsXH[t * DinP + tid];
        lacc_b += ldsGU[t * DinP + tid];
      }
    __syncthreads();
  }
  // write C tiles (skip padded rows/cols)
#pragma unroll
  for (int q = 0; q < MY_CT; ++q) {
    const int ct = wave + q * n_waves;
    if (ct >= CT) continue;
    const int m0 = (ct / NTL) * 16;
    const int n0 = (ct % NTL) * 16;
    const int col = n0 + (lane & 15);
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int row = m0 + (lane >> 4) * 4 + reg;
      if (row < Dout && col < Din)
        WG_(w_slot + 2)[(long)row * Din + col] = acc[q][reg];
    }
  }
  if (tid < Dout) WG_(w_slot + 3)[tid] = bacc;
  if (tid < Din) {
    WG_(w_slot)[tid] = lacc_w;
    WG_(w_slot + 1)[tid] = lacc_b;
  }
}

struct WJob {
  const float *gpre0, *xh0;   // source 0 rows
  const float *gpre1, *xh1;   // source 1 rows (or null)
  const float *gu0, *gu1;     // LN-out grad rows (for gamma/beta)
  int rows0, rows1, Din, Dout;
  int w_slot;                 // base slot (LN w, LN b, W, b)
  int has_affine_u;           // u = xh*gam+bet (always true here)
};

__global__ void __launch_bounds__(256)
cs_bwd_w_kernel(CachedPtrs P, CachedDims D) {
  const int tid = threadIdx.x;
  const int NT = blockDim.x;
  __shared__ float tG[TILE_K][65];
  __shared__ float tU[TILE_K][65];
  __shared__ float tGU[TILE_K][65];
  __shared__ float tXH[TILE_K][65];
  __shared__ float ldsG[TILE_K * 64], ldsU[TILE_K * 64];
  __shared__ float ldsGU[TILE_K * 64], ldsXH[TILE_K * 64];

  // jobs 0..5 are row-split nsplit ways (one WG per (job, split)); the
  // MFMA variants (env opt-in) keep single-WG jobs
  const int nsplit = D.wgrad_mfma ? 1 : WSPLIT;
  const int jobs_end = 6 * nsplit;
  if ((int)blockIdx.x < jobs_end) {
    const int job = blockIdx.x / nsplit;
    const int sp = blockIdx.x % nsplit;
    float* pout = (nsplit > 1)
        ? P.wg_scratch + ((long)job * WSPLIT + sp) * WG_JSTRIDE : nullptr;
    switch (job) {
      case 0:  // node module 1
        wgrad_tiled<KF0, KH>(P, tid, NT, D.N, 0, P.ghn1, nullptr, P.xh_z1,
                             nullptr, P.gu_z1, nullptr, W_LN_N1_W, tG, tU,
                             tGU, tXH, sp, nsplit, pout);
        return;
      case 1:  // edge module 1
        wgrad_tiled<KFE, KH>(P, tid, NT, D.E, 0, P.ghe1, nullptr, P.xh_e1,
                             nullptr, P.gu_e1, nullptr, W_LN_E1_W, tG, tU,
                             tGU, tXH, sp, nsplit, pout);
        return;
      case 2:  // reduce module 1 (edge ++ self rows)
        if (D.wgrad_mfma)
          wgrad_tiled_mfma<KMSG, KHID, KMSG, KHID>(
              P, tid, NT, D.E, D.N, P.gpre1_e, P.gpre1_s,
              P.xh_m1e, P.xh_m1s, P.gu_m1e, P.gu_m1s,
              W_LN_R1_W, ldsG, ldsU, ldsGU, ldsXH);
        else
          wgrad_tiled<KMSG, KHID>(P, tid, NT, D.E, D.N, P.gpre1_e,
                                  P.gpre1_s, P.xh_m1e, P.xh_m1s, P.gu_m1e,
                                  P.gu_m1s, W_LN_R1_W, tG, tU, tGU, tXH,
                                  sp, nsplit, pout);
        return;
      case 3:  // node module 2
        if (D.wgrad_mfma)
          wgrad_tiled_mfma<KHID, KH, KHID, 16>(
              P, tid, NT, D.N, 0, P.gpn1, nullptr, P.xh_h2,
              nullptr, P.gu_h2, nullptr, W_LN_N2_W, ldsG, ldsU, ldsGU,
              ldsXH);
        else
          wgrad_tiled<KHID, KH>(P, tid, NT, D.N, 0, P.gpn1, nullptr,
                                P.xh_h2, nullptr, P.gu_h2, nullptr,
                                W_LN_N2_W, tG, tU, tGU, tXH, sp, nsplit,
                                pout);
        return;
      case 4:  // edge module 2
        wgrad_tiled<KFE, KH>(P, tid, NT, D.E, 0, P.gpe1, nullptr, P.xh_e2,
                             nullptr, P.gu_e2, nullptr, W_LN_E2_W, tG, tU,
                             tGU, tXH, sp, nsplit, pout);
        return;
      default:  // 5: reduce module 2
        if (D.wgrad_mfma)
          wgrad_tiled_mfma<KMSG, KOUT, KMSG, 16>(
              P, tid, NT, D.E, D.N, P.gpe2, P.gpn2,
              P.xh_m2e, P.xh_m2s, P.gu_m2e, P.gu_m2s,
              W_LN_R2_W, ldsG, ldsU, ldsGU, ldsXH);
        else
          wgrad_tiled<KMSG, KOUT>(P, tid, NT, D.E, D.N, P.gpe2, P.gpn2,
                                  P.xh_m2e, P.xh_m2s, P.gu_m2e, P.gu_m2s,
                                  W_LN_R2_W, tG, tU, tGU, tXH, sp, nsplit,
                                  pout);
        return;
    }
  }

  // ---- special jobs over the B sample rows ----
  // Rule for all of them: operands are staged into LDS tile by tile with
  // coalesced cooperative loads, then every output element is reduced in
  // the original b = 0..B-1 order (tile by tile, t within the tile) — a
  // serial chain out of LDS, never a chain of dependent global loads.
  if ((int)blockIdx.x == jobs_end) {
    // graph module: Wg[GEMB,GFin], bg; LN gamma/beta from gu34 + xh34.
    // gpre rows are gfinal[:, KOUT:KOUT+KGE] (row stride KFIN).
    const float* __restrict__ gam = WP(W_LN_G_W);
    const float* __restrict__ bet = WP(W_LN_G_B);
    constexpr int UNITS = KGE * KGF;
    constexpr int MYU = (UNITS + 255) / 256;
    float acc[MYU];
#pragma unroll
    for (int q = 0; q < MYU; ++q) acc[q] = 0.f;
    // tid in [64, 64+KGE): bias sums; tid in [128, 128+KGF): LN gamma/beta
    float bacc = 0.f, lacc_w = 0.f, lacc_b = 0.f;
    for (int r0 = 0; r0 < D.B; r0 += TILE_K) {
      const int rt = min(TILE_K, D.B - r0);
      for (int x = tid; x < rt * KGE; x += NT) {
        int t = x / KGE, o = x % KGE;
        tG[t][o] = P.gfinal[(long)(r0 + t) * KFIN + KOUT + o];
      }
      for (int x = tid; x < rt * KGF; x += NT) {
        int t = x / KGF, i = x % KGF;
        const float xh = P.xh34[(long)r0 * KGF + x];
        tU[t][i] = FMA(xh, gam[i], bet[i]);
        tXH[t][i] = xh;
        tGU[t][i] = P.gu34[(long)r0 * KGF + x];
      }
      __syncthreads();
#pragma unroll
      for (int q = 0; q < MYU; ++q) {
        int u = tid + q * 256;
        if (u < UNITS) {
          int o = u / KGF, i = u % KGF;
          float a = acc[q];
          for (int t = 0; t < rt; ++t) a = FMA(tG[t][o], tU[t][i], a);
          acc[q] = a;
        }
      }
      if (tid >= 64 && tid < 64 + KGE)
        for (int t = 0; t < rt; ++t) bacc += tG[t][tid - 64];
      if (tid >= 128 && tid < 128 + KGF)
        for (int t = 0; t < rt; ++t) {
          lacc_w = lacc_w + mul_rn(tGU[t][tid - 128], tXH[t][tid - 128]);
          lacc_b += tGU[t][tid - 128];
        }
      __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < MYU; ++q) {
      int u = tid + q * 256;
      if (u < UNITS) WG_(W_G_W)[u] = acc[q];
    }
    if (tid >= 64 && tid < 64 + KGE) WG_(W_G_B)[tid - 64] = bacc;
    if (tid >= 128 && tid < 128 + KGF) {
      WG_(W_LN_G_W)[tid - 128] = lacc_w;
      WG_(W_LN_G_B)[tid - 128] = lacc_b;
    }
    return;
  }
  // remaining blocks split the FC columns: block jb owns columns [j0, j1)
  // of W1p/W1v [FC,FIN] (+ b1p/b1v) AND of W2p [A,FC] / W2v [FC]; block 0
  // also sums b2p and b2v.
  {
    const int nb = gridDim.x - jobs_end - 1;
    const int jb = blockIdx.x - jobs_end - 1;
    const int per = (KFC + nb - 1) / nb;
    const int j0 = jb * per, j1 = min(KFC, j0 + per);
    const int JW = j1 - j0;
    __shared__ float tF[TILE_K][KFIN];
    __shared__ float tGp[TILE_K][16], tGv[TILE_K][16];
    __shared__ float tHp[TILE_K][16], tHv[TILE_K][16];
    __shared__ float tGL[TILE_K][KA], tGV[TILE_K];
    constexpr int MYU = (16 * KFIN + 255) / 256;   // JW <= 16
    constexpr int MYU2 = (16 * KA + 255) / 256;
    float accp[MYU], accv[MYU], acc2[MYU2];
#pragma unroll
    for (int q = 0; q < MYU; ++q) { accp[q] = 0.f; accv[q] = 0.f; }
#pragma unroll
    for (int q = 0; q < MYU2; ++q) acc2[q] = 0.f;
    // tid < JW: column sums b1p/b1v and the W2v column; jb == 0 only:
    // tid in [64, 64+KA) sums b2p, tid == 128 sums b2v
    float bp = 0.f, bv = 0.f, w2v = 0.f, b2 = 0.f;
    for (int r0 = 0; r0 < D.B; r0 += TILE_K) {
      const int rt = min(TILE_K, D.B - r0);
      for (int x = tid; x < rt * KFIN; x += NT) {
        int t = x / KFIN, i = x % KFIN;
        tF[t][i] = P.fin[(long)(r0 + t) * KFIN + i];
      }
      for (int x = tid; x < rt * JW; x += NT) {
        int t = x / JW, j = x % JW;
        const long g = (long)(r0 + t) * KFC + j0 + j;
        tGp[t][j] = P.gh1p[g];
        tGv[t][j] = P.gh1v[g];
        tHp[t][j] = P.h1p[g];
        tHv[t][j] = P.h1v[g];
      }
      for (int x = tid; x < rt * KA; x += NT)
        tGL[x / KA][x % KA] = P.glogits[(long)r0 * KA + x];
      for (int t = tid; t < rt; t += NT) tGV[t] = P.gvalue[r0 + t];
      __syncthreads();
#pragma unroll
      for (int q = 0; q < MYU; ++q) {
        int u = tid + q * NT;
        if (u < JW * KFIN) {
          int j = u / KFIN, i = u % KFIN;
          float ap = accp[q], av = accv[q];
          if (rt == TILE_K) {
#pragma unroll
            for (int t = 0; t < TILE_K; ++t) {
              ap = FMA(tGp[t][j], tF[t][i], ap);
              av = FMA(tGv[t][j], tF[t][i], av);
            }
          } else {
            for (int t = 0; t < rt; ++t) {
              ap = FMA(tGp[t][j], tF[t][i], ap);
              av = FMA(tGv[t][j], tF[t][i], av);
            }
          }
          accp[q] = ap;
          accv[q] = av;
        }
      }
#pragma unroll
      for (int q = 0; q < MYU2; ++q) {
        int u = tid + q * NT;
        if (u < KA * JW) {
          int a = u / JW, j = u % JW;
          float s = acc2[q];
          if (rt == TILE_K) {
#pragma unroll
            for (int t = 0; t < TILE_K; ++t) {
              // a full tile's first 20 terms are fused, the last 12 are
              // rounded products; a partial tile is fused throughout
              if (t < 20) s = FMA(tGL[t][a], tHp[t][j], s);
              else s = s + mul_rn(tGL[t][a], tHp[t][j]);
            }
          } else {
            for (int t = 0; t < rt; ++t) s = FMA(tGL[t][a], tHp[t][j], s);
          }
          acc2[q] = s;
        }
      }
      if (tid < JW) {
        for (int t = 0; t < rt; ++t) {
          bp += tGp[t][tid];
          bv += tGv[t][tid];
          w2v = FMA(tGV[t], tHv[t][tid], w2v);
        }
      }
      if (jb == 0) {
        if (tid >= 64 && tid < 64 + KA)
          for (int t = 0; t < rt; ++t) b2 += tGL[t][tid - 64];
        if (tid == 128)
          for (int t = 0; t < rt; ++t) b2 += tGV[t];
      }
      __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < MYU; ++q) {
      int u = tid + q * NT;
      if (u < JW * KFIN) {
        int j = u / KFIN, i = u % KFIN;
        WG_(W_P1_W)[(long)(j0 + j) * KFIN + i] = accp[q];
        WG_(W_V1_W)[(long)(j0 + j) * KFIN + i] = accv[q];
      }
    }
#pragma unroll
    for (int q = 0; q < MYU2; ++q) {
      int u = tid + q * NT;
      if (u < KA * JW) {
        int a = u / JW, j = u % JW;
        WG_(W_P2_W)[(long)a * KFC + j0 + j] = acc2[q];
      }
    }
    if (tid < JW) {
      WG_(W_P1_B)[j0 + tid] = bp;
      WG_(W_V1_B)[j0 + tid] = bv;
      WG_(W_V2_W)[j0 + tid] = w2v;
    }
    if (jb == 0) {
      if (tid >= 64 && tid < 64 + KA) WG_(W_P2_B)[tid - 64] = b2;
      if (tid == 128) WG_(W_V2_B)[0] = b2;
    }
  }
}

// sum the row-split partials (fixed split order: deterministic) into the
// flat gradient; one block per job
__global__ void __launch_bounds__(256)
cs_bwd_w_reduce_kernel(CachedPtrs P, CachedDims D) {
  int Din, Dout, slot;
  switch (blockIdx.x) {
    case 0: Din = KF0;  Dout = KH;   slot = W_LN_N1_W; break;
    case 1: Din = KFE;  Dout = KH;   slot = W_LN_E1_W; break;
    case 2: Din = KMSG; Dout = KHID; slot = W_LN_R1_W; break;
    case 3: Din = KHID; Dout = KH;   slot = W_LN_N2_W; break;
    case 4: Din = KFE;  Dout = KH;   slot = W_LN_E2_W; break;
    default: Din = KMSG; Dout = KOUT; slot = W_LN_R2_W; break;
  }
  const float* __restrict__ base =
      P.wg_scratch + (long)blockIdx.x * WSPLIT * WG_JSTRIDE;
  const int tid = threadIdx.x, NT = blockDim.x;
  const int units = Din * Dout;
  for (int u = tid; u < units; u += NT) {
    float a = 0.f;
    for (int s = 0; s < WSPLIT; ++s) a += base[(long)s * WG_JSTRIDE + u];
    WG_(slot + 2)[u] = a;
  }
  for (int o = tid; o < Dout; o += NT) {
    float a = 0.f;
    for (int s = 0; s < WSPLIT; ++s)
      a += base[(long)s * WG_JSTRIDE + units + o];
    WG_(slot + 3)[o] = a;
  }
  for (int i = tid; i < Din; i += NT) {
    float aw = 0.f, ab = 0.f;
    for (int s = 0; s < WSPLIT; ++s) {
      aw += base[(long)s * WG_JSTRIDE + units + Dout + i];
      ab += base[(long)s * WG_JSTRIDE + units + Dout + Din + i];
    }
    WG_(slot)[i] = aw;
    WG_(slot + 1)[i] = ab;
  }
}

// ===========================================================================
// lane-parallel row kernels
// ===========================================================================
//
// The thread-per-row kernels above (cs_fwd_mlp, cs_fwd_reduce, cs_bwd_reduce,
// cs_bwd_mlp2, cs_bwd_gu1) put the N+E graph rows on two workgroups and run
// each row's LayerNorm and Din x Dout GEMV as one thread's serial chain.  The
// kernels below give each row a group of L lanes and a block 256/L rows, so
// the same work spreads over (N+E)*L/256 workgroups.  They are the default;
// DDLS_AMD_ROW_KERNELS=thread launches the thread-per-row kernels instead,
// which stay in the file unchanged as the oracle for bitwise comparison.
//
// No sum is re-associated: every output element is still accumulated by one
// lane in the order the thread-per-row code uses (i ascending for a forward
// output and the LN sums, o ascending for a gu element); lanes only divide
// the OUTPUTS among themselves.  The rows of a block are staged in LDS once
// (row stride +1 so the groups of a wave sit on different banks; the forward
// weights too, because the lanes of a group read different W rows at one i).
//
// Contraction is switched off from here to the end of the file and every
// rounding is written out, FMA() = one rounding, a + b * c = two.  The
// pattern per instantiation is the one the thread-per-row build has (read
// off its gfx950 ISA; docs/KERNELS.md "Round 5" lists it):
//   LN variance    d0*d0 rounded, then d_i*d_i added as rounded products,
//                  except the LAST term of a 5-wide row and the 16 zero-half
//                  terms of a self row, which are fused
//   var/Din + eps  one FMA when Din is a power of two, divide-then-add for 5
//   u = xh*gam+bet one FMA; every forward GEMV term fused
//   gu = W^T gpre  all 16 terms fused (Dout 16, node/edge modules), the first
//                  4 of 16 (reduce module 2) or the first 52 of 64 (reduce
//                  module 1) fused and the last 12 rounded products
//   LN backward    gh = gu*gam rounded inside m1 and m2, gh*xh rounded;
//                  gin = rstd * FMA(-xh, m2, FMA(gu, gam, -m1)), except the
//                  last two elements of a 32-wide row, which take the rounded
//                  gh: FMA(m1sum, -1/32, gh)
#pragma clang fp contract(off)

#define ROW_NT 256   // block size of every lane-parallel row kernel

// forward of the block's rows [r0, r0 + 256/L) of one row class.  NF = the
// number of trailing variance terms that are fused.  Called by all threads
// of the block (barriers inside).
template <int Din, int Dout, int NF, int L, typename LoadX>
__device__ __forceinline__ void rows_fwd_lanes(
    const CachedPtrs& P, int w_slot, long r0, long nrows, LoadX loadx,
    float* __restrict__ xhat_out, float* __restrict__ rstd_out,
    float* __restrict__ out) {
  constexpr int RPB = ROW_NT / L;
  constexpr int XS = Din + 1;
  __shared__ float sGam[Din], sBet[Din], sW[Dout * XS], sB[Dout];
  __shared__ float sX[RPB * XS], sU[RPB * XS];
  const int tid = threadIdx.x;
  for (int i = tid; i < Din; i += ROW_NT) {
    sGam[i] = WP(w_slot)[i];
    sBet[i] = WP(w_slot + 1)[i];
  }
  for (int x = tid; x < Din * Dout; x += ROW_NT)
    sW[(x / Din) * XS + x % Din] = WP(w_slot + 2)[x];
  for (int o = tid; o < Dout; o += ROW_NT) sB[o] = WP(w_slot + 3)[o];
  for (int x = tid; x < RPB * Din; x += ROW_NT) {
    const int r = x / Din, i = x % Din;
    sX[r * XS + i] = (r0 + r < nrows) ? loadx(r0 + r, i) : 0.f;
  }
  __syncthreads();
  const int g = tid / L, l = tid % L;
  const long row = r0 + g;
  const bool live = row < nrows;
  // LN statistics: every lane of the group walks the whole row in order
  const float* __restrict__ x = sX + g * XS;
  float s = 0.f;
#pragma unroll 8
  for (int i = 0; i < Din; ++i) s = s + x[i];
  const float mu = s / Din;
  float var;
  {
    const float d0 = x[0] - mu;
    var = d0 * d0;
  }
#pragma unroll 8
  for (int i = 1; i < Din; ++i) {
    const float d = x[i] - mu;
    if (i >= Din - NF) var = FMA(d, d, var);
    else var = var + d * d;
  }
  float rstd;
  if ((Din & (Din - 1)) == 0) rstd = rsqrtf(FMA(var, 1.f / Din, LN_EPS));
  else rstd = rsqrtf(var / Din + LN_EPS);
  for (int i = l; i < Din; i += L) {
    const float xh = (x[i] - mu) * rstd;
    if (live) xhat_out[row * Din + i] = xh;
    sU[g * XS + i] = FMA(xh, sGam[i], sBet[i]);
  }
  if (live && l == 0) rstd_out[row] = rstd;
  __syncthreads();
  const float* __restrict__ u = sU + g * XS;
  for (int o = l; o < Dout; o += L) {
    const float* __restrict__ w = sW + o * XS;
    float acc = sB[o];
#pragma unroll 8
    for (int i = 0; i < Din; ++i) acc = FMA(u[i], w[i], acc);
    if (live) out[row * Dout + o] = acc > 0.f ? acc : 0.f;
  }
}

// backward of the block's rows of one row class: gpre = gout*(out>0) and
// gu = W^T gpre stored; with GIN the input grad through the LN backward.
// NFU = leading fused terms of a gu chain, NTAIL = trailing gin elements
// that take the rounded gh.
template <int Din, int Dout, int NFU, int NTAIL, int L, bool GIN,
          typename LoadG>
__device__ __forceinline__ void rows_bwd_lanes(
    const CachedPtrs& P, int w_slot, long r0, long nrows, LoadG loadg,
    const float* __restrict__ out, const float* __restrict__ xhat,
    const float* __restrict__ rst, float* __restrict__ gpre_store,
    float* __restrict__ gu_store, float* __restrict__ gin) {
  constexpr int RPB = ROW_NT / L;
  constexpr int XS = Din + 1;
  constexpr int GS = Dout + 1;
  __shared__ float sGam[Din], sW[Dout * Din];
  __shared__ float sG[RPB * GS], sGU[RPB * XS], sXH[GIN ? RPB * XS : 1];
  const int tid = threadIdx.x;
  for (int i = tid; i < Din; i += ROW_NT) sGam[i] = WP(w_slot)[i];
  for (int x = tid; x < Dout * Din; x += ROW_NT) sW[x] = WP(w_slot + 2)[x];
  for (int x = tid; x < RPB * Dout; x += ROW_NT) {
    const int r = x / Dout, o = x % Dout;
    const long row = r0 + r;
    float gp = 0.f;
    if (row < nrows) {
      const float go = loadg(row, o);
      gp = out[row * Dout + o] > 0.f ? go : 0.f;
      gpre_store[row * Dout + o] = gp;
    }
    sG[r * GS + o] = gp;
  }
  if (GIN) {
    for (int x = tid; x < RPB * Din; x += ROW_NT) {
      const int r = x / Din, i = x % Din;
      sXH[r * XS + i] = (r0 + r < nrows) ? xhat[(r0 + r) * Din + i] : 0.f;
    }
  }
  __syncthreads();
  const int g = tid / L, l = tid % L;
  const long row = r0 + g;
  const bool live = row < nrows;
  const float* __restrict__ gp = sG + g * GS;
  for (int i = l; i < Din; i += L) {
    float acc = 0.f;
#pragma unroll 8
    for (int o = 0; o < Dout; ++o) {
      if (o < NFU) acc = FMA(sW[o * Din + i], gp[o], acc);
      else acc = acc + sW[o * Din + i] * gp[o];
    }
    if (live) gu_store[row * Din + i] = acc;
    sGU[g * XS + i] = acc;
  }
  if (GIN) {
    __syncthreads();
    const float* __restrict__ gu = sGU + g * XS;
    const float* __restrict__ xh = sXH + g * XS;
    float m1 = 0.f, m2 = 0.f;
#pragma unroll 8
    for (int i = 0; i < Din; ++i) {
      const float gh = gu[i] * sGam[i];
      m1 = m1 + gh;
      m2 = m2 + gh * xh[i];
    }
    const float m1d = m1 / Din;
    const float m2d = m2 / Din;
    const float rstd = live ? rst[row] : 0.f;
    for (int i = l; i < Din; i += L) {
      float a;
      if (i < Din - NTAIL) a = FMA(gu[i], sGam[i], -m1d);
      else a = FMA(m1, -1.f / Din, gu[i] * sGam[i]);
      if (live) gin[row * Din + i] = rstd * FMA(-xh[i], m2d, a);
    }
  }
}

// Row classes never share a block: blocks [0, nb0) take the first class,
// the rest the second, so a block runs one instantiation and its barriers
// are block-uniform.
template <int ROUND, int L>
__global__ void __launch_bounds__(ROW_NT)
cs_fwd_mlp_lanes_kernel(CachedPtrs P, CachedDims D) {
  constexpr int RPB = ROW_NT / L;
  const int nbN = (D.N + RPB - 1) / RPB;
  if ((int)blockIdx.x < nbN) {
    const long r0 = (long)blockIdx.x * RPB;
    if (ROUND == 1)
      rows_fwd_lanes<KF0, KH, 1, L>(
          P, W_LN_N1_W, r0, D.N,
          [&](long v, int i) { return P.z0[v * KF0 + i]; },
          P.xh_z1, P.rst_z1, P.hn1);
    else
      rows_fwd_lanes<KHID, KH, 0, L>(
          P, W_LN_N2_W, r0, D.N,
          [&](long v, int i) { return P.h1[v * KHID + i]; },
          P.xh_h2, P.rst_h2, P.hn2);
  } else {
    const long r0 = (long)(blockIdx.x - nbN) * RPB;
    auto ld = [&](long k, int i) { return P.e[k * KFE + i]; };
    if (ROUND == 1)
      rows_fwd_lanes<KFE, KH, 0, L>(P, W_LN_E1_W, r0, D.E, ld, P.xh_e1,
                                    P.rst_e1, P.he1);
    else
      rows_fwd_lanes<KFE, KH, 0, L>(P, W_LN_E2_W, r0, D.E, ld, P.xh_e2,
                                    P.rst_e2, P.he2);
  }
}

template <int ROUND, int L>
__global__ void __launch_bounds__(ROW_NT)
cs_fwd_reduce_lanes_kernel(CachedPtrs P, CachedDims D) {
  constexpr int RPB = ROW_NT / L;
  constexpr int DO = (ROUND == 1) ? KHID : KOUT;
  constexpr int SLOT = (ROUND == 1) ? W_LN_R1_W : W_LN_R2_W;
  const float* __restrict__ hn = (ROUND == 1) ? P.hn1 : P.hn2;
  const float* __restrict__ he = (ROUND == 1) ? P.he1 : P.he2;
  const int nbE = (D.E + RPB - 1) / RPB;
  if ((int)blockIdx.x < nbE) {
    const long r0 = (long)blockIdx.x * RPB;
    rows_fwd_lanes<KMSG, DO, 0, L>(
        P, SLOT, r0, D.E,
        [&](long k, int i) {
          return i < KH ? hn[P.src[k] * KH + i] : he[k * KH + (i - KH)];
        },
        (ROUND == 1) ? P.xh_m1e : P.xh_m2e,
        (ROUND == 1) ? P.rst_m1e : P.rst_m2e,
        (ROUND == 1) ? P.re1 : P.re2);
  } else {
    // self message = concat(hn[v], 0): the zero half's variance terms are
    // the fused ones
    const long r0 = (long)(blockIdx.x - nbE) * RPB;
    rows_fwd_lanes<KMSG, DO, KH, L>(
        P, SLOT, r0, D.N,
        [&](long v, int i) { return i < KH ? hn[v * KH + i] : 0.f; },
        (ROUND == 1) ? P.xh_m1s : P.xh_m2s,
        (ROUND == 1) ? P.rst_m1s : P.rst_m2s,
        (ROUND == 1) ? P.rs1 : P.rs2);
  }
}

template <int ROUND, int L>
__global__ void __launch_bounds__(ROW_NT)
cs_bwd_reduce_lanes_kernel(CachedPtrs P, CachedDims D) {
  constexpr int RPB = ROW_NT / L;
  constexpr int DO = (ROUND == 1) ? KHID : KOUT;
  constexpr int SLOT = (ROUND == 1) ? W_LN_R1_W : W_LN_R2_W;
  constexpr int NFU = DO - 12;
  const float* __restrict__ gh = (ROUND == 1) ? P.gh1b : P.gh2;
  const int nbE = (D.E + RPB - 1) / RPB;
  if ((int)blockIdx.x < nbE) {
    const long r0 = (long)blockIdx.x * RPB;
    rows_bwd_lanes<KMSG, DO, NFU, 2, L, true>(
        P, SLOT, r0, D.E,
        [&](long k, int o) {
          const int v = (int)P.dst[k];
          const long deg = P.indptr[v + 1] - P.indptr[v];
          const float f = 1.f / (float)(deg + 1);
          return gh[(long)v * DO + o] * f;
        },
        (ROUND == 1) ? P.re1 : P.re2,
        (ROUND == 1) ? P.xh_m1e : P.xh_m2e,
        (ROUND == 1) ? P.rst_m1e : P.rst_m2e,
        (ROUND == 1) ? P.gpre1_e : P.gpe2,
        (ROUND == 1) ? P.gu_m1e : P.gu_m2e,
        (ROUND == 1) ? P.gme1 : P.gme2);
  } else {
    const long r0 = (long)(blockIdx.x - nbE) * RPB;
    rows_bwd_lanes<KMSG, DO, NFU, 2, L, true>(
        P, SLOT, r0, D.N,
        [&](long v, int o) {
          const long deg = P.indptr[v + 1] - P.indptr[v];
          const float f = (deg > 0) ? 1.f / (float)(deg + 1) : 0.f;
          return gh[v * DO + o] * f;
        },
        (ROUND == 1) ? P.rs1 : P.rs2,
        (ROUND == 1) ? P.xh_m1s : P.xh_m2s,
        (ROUND == 1) ? P.rst_m1s : P.rst_m2s,
        (ROUND == 1) ? P.gpre1_s : P.gpn2,
        (ROUND == 1) ? P.gu_m1s : P.gu_m2s,
        (ROUND == 1) ? P.gms1 : P.gms2);
  }
}

template <int L>
__global__ void __launch_bounds__(ROW_NT)
cs_bwd_mlp2_lanes_kernel(CachedPtrs P, CachedDims D) {
  constexpr int RPB = ROW_NT / L;
  const int nbN = (D.N + RPB - 1) / RPB;
  if ((int)blockIdx.x < nbN) {
    const long r0 = (long)blockIdx.x * RPB;
    rows_bwd_lanes<KHID, KH, KH, 0, L, true>(
        P, W_LN_N2_W, r0, D.N,
        [&](long v, int o) { return P.ghn2[v * KH + o]; },
        P.hn2, P.xh_h2, P.rst_h2, P.gpn1, P.gu_h2, P.gh1b);
  } else {
    const long r0 = (long)(blockIdx.x - nbN) * RPB;
    rows_bwd_lanes<KFE, KH, KH, 0, L, false>(
        P, W_LN_E2_W, r0, D.E,
        [&](long k, int o) { return P.ghe2[k * KH + o]; },
        P.he2, nullptr, nullptr, P.gpe1, P.gu_e2, nullptr);
  }
}

// module-1 LN-out grad rows: one thread per gu element (all 16 terms fused)
__global__ void __launch_bounds__(ROW_NT)
cs_bwd_gu1_lanes_kernel(CachedPtrs P, CachedDims D) {
  __shared__ float sWN[KH * KF0], sWE[KH * KFE];
  const int tid = threadIdx.x;
  for (int x = tid; x < KH * KF0; x += ROW_NT) sWN[x] = WP(W_N1_W)[x];
  for (int x = tid; x < KH * KFE; x += ROW_NT) sWE[x] = WP(W_E1_W)[x];
  __syncthreads();
  const long nU = (long)D.N * KF0;
  const long total = nU + (long)D.E * KFE;
  const long u = (long)blockIdx.x * ROW_NT + tid;
  if (u >= total) return;
  if (u < nU) {
    const long v = u / KF0;
    const int i = (int)(u % KF0);
    float acc = 0.f;
#pragma unroll
    for (int o = 0; o < KH; ++o)
      acc = FMA(sWN[o * KF0 + i], P.ghn1[v * KH + o], acc);
    P.gu_z1[u] = acc;
  } else {
    const long x = u - nU;
    const long k = x / KFE;
    const int i = (int)(x % KFE);
    float acc = 0.f;
#pragma unroll
    for (int o = 0; o < KH; ++o)
      acc = FMA(sWE[o * KFE + i], P.ghe1[k * KH + o], acc);
    P.gu_e1[x] = acc;
  }
}

// ===========================================================================
// fused launches
// ===========================================================================
//
// Neighbouring kernels whose dependencies are row-local or sample-local, run
// as one launch each (a replay is a serial chain of launches, each near the
// dispatch floor).  Default; DDLS_AMD_STEP_FUSION=off launches the separate
// kernels above, which stay in the file unchanged as the oracle.  Every
// tensor the separate kernels wrote is still written, in the same bits: the
// summation orders are theirs, and the roundings are the ones their gfx950
// ISA has (docs/KERNELS.md "Round 6"):
//   fwd_head       bias first, i = 0..23, every term fused
//   fwd_logits     16-term chunk partial: terms 0-3 fused onto 0, 4-15 rounded
//                  products; logit = bias + partials c = 0..15, plain adds;
//                  value = W2v*h1v rounded, 256-wide halving tree, + bias
//   fwd_loss       plain adds for Z; entropy terms fused: fma(-lp, exp(lp), .)
//   combine        plain adds in CSR order, IEEE division by deg+1
//   scatter        plain adds in src-CSR order

// ---- per-sample chain: fwd_head + fwd_logits + fwd_loss + bwd_head ----
#define HD_HS 4                    // samples in flight per block
#define HD_CS 20                   // LDS stride of a 16-float chunk: lanes
                                   // that read one chunk each (b128) spread
                                   // over all banks
#define HD_ROW (16 * HD_CS)        // a KFC-wide row stored as 16 chunks
__device__ __forceinline__ int hd_pad(int j) {
  return (j >> 4) * HD_CS + (j & 15);
}

// Blocks and sample ranges are cs_bwd_head_kernel's: min(B, 32) blocks, each
// walking its contiguous range HD_HS samples at a time.  Thread j owns hidden
// unit j of both branches through the forward AND the backward (its W1p/W1v
// rows sit in registers for the forward; h1p/h1v stay in registers as the
// relu masks); rows that another thread needs go through LDS, and every row
// the separate kernels stored is stored for cs_bwd_w and the tests.
__global__ void __launch_bounds__(256)
cs_head_kernel(CachedPtrs P, CachedDims D) {
  constexpr int HS = HD_HS;
  __shared__ float sW2p[KA * HD_ROW];
  __shared__ float sW1p[KFC * KFIN], sW1v[KFC * KFIN], sWg[KGE * KGF];
  __shared__ float sB2p[KA];
  // backward rows; +1 keeps the HS rows of one column on distinct banks
  __shared__ float sGL[HS][KA], sGV[HS], sGF[HS][KFIN];
  __shared__ float sGHp[HS][KFC + 1], sGHv[HS][KFC + 1];
  // forward rows
  __shared__ float sFin[HS][KFIN], sHp[HS][HD_ROW], sVred[HS][KFC];
  __shared__ float sGf[HS][KGF], sU34[HS][KGF];
  __shared__ float sGamG[KGF], sBetG[KGF], sBg[KGE];
  __shared__ float sPart[HS][KA][16 + 1];
  __shared__ float sRow[HS][KA], sPp[HS][KA], sLp[HS][KA];
  __shared__ float sVal[HS], sCoef[HS], sHent[HS];
  const int tid = threadIdx.x;
  constexpr int NT = 256;
  for (int x = tid; x < KA * KFC; x += NT)
    sW2p[(x / KFC) * HD_ROW + hd_pad(x % KFC)] = WP(W_P2_W)[x];
  for (int x = tid; x < KGE * KGF; x += NT) sWg[x] = WP(W_G_W)[x];
  if (tid < KA) sB2p[tid] = WP(W_P2_B)[tid];
  if (tid < KGF) {
    sGamG[tid] = WP(W_LN_G_W)[tid];
    sBetG[tid] = WP(W_LN_G_B)[tid];
  }
  if (tid < KGE) sBg[tid] = WP(W_G_B)[tid];
  float w1p[KFIN], w1v[KFIN];
#pragma unroll
  for (int i = 0; i < KFIN; ++i) {
    w1p[i] = WP(W_P1_W)[tid * KFIN + i];
    w1v[i] = WP(W_V1_W)[tid * KFIN + i];
  }
  // the backward's LDS copy of W1p / W1v comes out of the same registers:
  // the block's threads hold exactly the two matrices, one row each
#pragma unroll
  for (int i = 0; i < KFIN; ++i) {
    sW1p[tid * KFIN + i] = w1p[i];
    sW1v[tid * KFIN + i] = w1v[i];
  }
  const float b1p = WP(W_P1_B)[tid], b1v = WP(W_V1_B)[tid];
  const float w2v = WP(W_V2_W)[tid];
  const float b2v = WP(W_V2_B)[0];
  const float klc = P.kl[0];
  const int wv = tid >> 6, ln = tid & 63;
  const int per = (D.B + gridDim.x - 1) / gridDim.x;
  const int b0 = blockIdx.x * per;
  const int b1 = min(D.B, b0 + per);
  for (int c0 = b0; c0 < b1; c0 += HS) {
    const int ns = min(HS, b1 - c0);
    // final = concat(pooled[model], graph_module(LN(gf))): the per-sample
    // half of cs_fwd_pool_kernel.  The lanes of a sample walk its gf row
    // redundantly for the LN sums (same bits in every lane).
    for (int x = tid; x < ns * KGF; x += NT)
      sGf[x / KGF][x % KGF] = P.gf[(long)c0 * KGF + x];
    for (int x = tid; x < ns * KOUT; x += NT) {
      const int s = x / KOUT, i = x % KOUT;
      const long mid = P.model_ids[c0 + s];
      const float pv = P.pooled[mid * KOUT + i];
      sFin[s][i] = pv;
      P.fin[(long)(c0 + s) * KFIN + i] = pv;
    }
    __syncthreads();
    for (int x = tid; x < ns * KGF; x += NT) {
      const int s = x / KGF, i = x % KGF;
      const float* __restrict__ xr = sGf[s];
      float sum = 0.f;
#pragma unroll
      for (int k = 0; k < KGF; ++k) sum = sum + xr[k];
      const float mu = sum / KGF;
      float var;
      {
        const float d0 = xr[0] - mu;
        var = d0 * d0;
      }
#pragma unroll
      for (int k = 1; k < KGF; ++k) {
        const float d = xr[k] - mu;
        var = var + d * d;
      }
      const float rstd = rsqrtf(var / KGF + LN_EPS);
      const float xh = (xr[i] - mu) * rstd;
      P.xh34[(long)(c0 + s) * KGF + i] = xh;
      sU34[s][i] = FMA(xh, sGamG[i], sBetG[i]);
    }
    __syncthreads();
    for (int x = tid; x < ns * KGE; x += NT) {
      const int s = x / KGE, o = x % KGE;
      float acc = sBg[o];
#pragma unroll
      for (int i = 0; i < KGF; ++i)
        acc = FMA(sWg[o * KGF + i], sU34[s][i], acc);
      sFin[s][KOUT + o] = acc;               // graph_module has NO activation
      P.fin[(long)(c0 + s) * KFIN + KOUT + o] = acc;
    }
    __syncthreads();
    // FC hidden layers: bias first, i ascending
    float hp[HS], hv[HS];
#pragma unroll
    for (int s = 0; s < HS; ++s) {
      hp[s] = 0.f;
      hv[s] = 0.f;
      if (s < ns) {
        float ap = b1p, av = b1v;
#pragma unroll
        for (int i = 0; i < KFIN; ++i) {
          ap = FMA(w1p[i], sFin[s][i], ap);
          av = FMA(w1v[i], sFin[s][i], av);
        }
        ap = ap > 0.f ? ap : 0.f;
        av = av > 0.f ? av : 0.f;
        const long u = (long)(c0 + s) * KFC + tid;
        P.h1p[u] = ap;
        P.h1v[u] = av;
        hp[s] = ap;
        hv[s] = av;
        sHp[s][hd_pad(tid)] = ap;
        sVred[s][tid] = w2v * av;
      }
    }
    __syncthreads();
    // logit partials over the 16 chunks of the hidden row
    for (int x = tid; x < ns * KA * 16; x += NT) {
      const int s = x / (KA * 16), r = x % (KA * 16);
      const int a = r / 16, c = r % 16;
      const float* __restrict__ w = sW2p + a * HD_ROW + c * HD_CS;
      const float* __restrict__ h = sHp[s] + c * HD_CS;
      float acc = FMA(w[0], h[0], 0.f);
#pragma unroll
      for (int i = 1; i < 16; ++i) {
        if (i < 4) acc = FMA(w[i], h[i], acc);
        else acc = acc + w[i] * h[i];
      }
      sPart[s][a][c] = acc;
    }
    // value: wave s folds sample s's 256 products in the halving tree's
    // pairing (t with t + 128, 64, ... 1)
    if (wv < ns) {
      const float* __restrict__ vr = sVred[wv];
      float a0 = vr[ln] + vr[ln + 128];
      const float a1 = vr[ln + 64] + vr[ln + 192];
      a0 = a0 + a1;
#pragma unroll
      for (int off = 32; off > 0; off >>= 1)
        a0 = a0 + __shfl_down(a0, off, 64);
      if (ln == 0) {
        const float val = a0 + b2v;
        sVal[wv] = val;
        P.values[c0 + wv] = val;
      }
    }
    __syncthreads();
    // raw masked logits
    for (int x = tid; x < ns * KA; x += NT) {
      const int s = x / KA, a = x % KA;
      float acc = sB2p[a];
#pragma unroll
      for (int c = 0; c < 16; ++c) acc = acc + sPart[s][a][c];
      const float fmin = -3.402823466e+38f;
      float lm = logf(P.mask[(long)c0 * KA + x]);
      if (!(lm > fmin)) lm = fmin;
      sRow[s][a] = acc + lm;
    }
    __syncthreads();
    // softmax / surrogate row of sample s: lane 0 of wave s
    if (wv < ns && ln == 0) {
      const int s = wv;
      const int b = c0 + s;
      const float* __restrict__ row = sRow[s];
      float mx = -3.0e38f;
#pragma unroll
      for (int a = 0; a < KA; ++a) mx = fmaxf(mx, row[a]);
      float Z = 0.f;
#pragma unroll
      for (int a = 0; a < KA; ++a) Z = Z + __expf(row[a] - mx);
      const float lse = mx + __logf(Z);
      float ent = 0.f;
#pragma unroll
      for (int a = 0; a < KA; ++a) {
        const float lp = row[a] - lse;
        const float e = __expf(lp);
        sLp[s][a] = lp;
        sPp[s][a] = e;
        ent = FMA(-lp, e, ent);
      }
      const long act = P.actions[b];
      const float logp_a = sLp[s][act];
      const float old_lp = P.old_logp[b];
      const float ratio = __expf(logp_a - old_lp);
      const float A_b = P.adv[b];
      const float r_cl = fminf(fmaxf(ratio, 1.f - D.clip), 1.f + D.clip);
      const float surr1 = ratio * A_b, surr2 = r_cl * A_b;
      float ds = ratio * A_b;
      if (surr2 < surr1 && (ratio < 1.f - D.clip || ratio > 1.f + D.clip))
        ds = 0.f;
      const float coef = -ds - klc;
      P.hent[b] = ent;
      P.coef[b] = coef;
      sHent[s] = ent;
      sCoef[s] = coef;
    }
    __syncthreads();
    // loss backward rows (upstream grad = 1); p and lp go out here
    for (int x = tid; x < ns * KA; x += NT) {
      const int s = x / KA, a = x % KA;
      const int b = c0 + s;
      const long u = (long)b * KA + a;
      const long act = P.actions[b];
      const float c = sCoef[s] / D.B;
      const float pj = sPp[s][a];
      const float lpj = sLp[s][a];
      P.p[u] = pj;
      P.lp[u] = lpj;
      const float delta = (a == (int)act) ? 1.f : 0.f;
      const float gl = mul_rn(c, delta - pj)
                       + mul_rn(mul_rn(D.ent_coef / D.B, pj),
                                lpj + sHent[s]);
      P.glogits[u] = gl;
      sGL[s][a] = gl;
    }
    if (tid >= 128 && tid < 128 + ns) {
      const int s = tid - 128;
      const int b = c0 + s;
      const float verr = sVal[s] - P.vtarg[b];
      const float mk = (verr * verr <= D.vf_clip) ? 1.f : 0.f;
      const float gv = D.vf_coef * 2.f * verr * mk / D.B;
      P.gvalue[b] = gv;
      sGV[s] = gv;
    }
    __syncthreads();
    // hidden grads
#pragma unroll
    for (int s = 0; s < HS; ++s) {
      if (s < ns) {
        const int j = tid;
        const long u = (long)(c0 + s) * KFC + j;
        float acc = 0.f;
#pragma unroll
        for (int a = 0; a < KA; ++a) {
          // the first five terms are fused, the rest rounded products
          const float w = sW2p[a * HD_ROW + hd_pad(j)];
          if (a < 5) acc = FMA(w, sGL[s][a], acc);
          else acc = acc + mul_rn(w, sGL[s][a]);
        }
        const float gp = hp[s] > 0.f ? acc : 0.f;
        const float av = w2v * sGV[s];
        const float gv = hv[s] > 0.f ? av : 0.f;
        P.gh1p[u] = gp;
        P.gh1v[u] = gv;
        sGHp[s][j] = gp;
        sGHv[s][j] = gv;
      }
    }
    __syncthreads();
    // gfinal: one thread per (sample, i), j = 0..FC-1 in order
    for (int x = tid; x < ns * KFIN; x += NT) {
      const int s = x / KFIN, i = x % KFIN;
      float acc = 0.f;
#pragma unroll 8
      for (int j = 0; j < KFC; ++j) {
        acc = FMA(sW1p[j * KFIN + i], sGHp[s][j], acc);
        acc = FMA(sW1v[j * KFIN + i], sGHv[s][j], acc);
      }
      P.gfinal[(long)(c0 + s) * KFIN + i] = acc;
      sGF[s][i] = acc;
    }
    __syncthreads();
    // graph-module LN-out grads
    for (int x = tid; x < ns * KGF; x += NT) {
      const int s = x / KGF, i = x % KGF;
      float acc = 0.f;
#pragma unroll
      for (int o = 0; o < KGE; ++o)
        acc = acc + mul_rn(sWg[o * KGF + i], sGF[s][KOUT + o]);
      P.gu34[(long)(c0 + s) * KGF + i] = acc;
    }
    // no barrier here: every row buffer's next write is at least one
    // barrier after its last read above
  }
  // the logging-only C_STATS sums are taken from the stored rows by the
  // statistics blocks of cs_bwd_scat1_gu1_kernel
}

// ---- cs_head with a shorter chain (DDLS_AMD_STEP_HEAD, default on) ----
// cs_head_kernel's phases, arithmetic and stores, term for term; the kernel
// above stays unchanged as the oracle.  What changes is what sits on the
// block's serial chain:
//  * every per-sample input of a chunk (mask, actions, old_logp, adv, vtarg)
//    is loaded at the chunk's top, in the round trip of gf / model_ids, not
//    in the middle of the chain (logf(mask) is taken there too);
//  * the gfinal phase reads its W1p / W1v copies i-major ([i][j], row stride
//    HD2_WS) and the hidden-grad rows with 16-byte LDS reads: 4 reads per
//    four j instead of 16.  The chain order stays j = 0..255, policy term
//    then value term, all fused.  Thread j writes column j of the copies, so
//    the writes are conflict-free;
//  * one sample a block on min(B, HD2_MAXB) blocks instead of four on
//    min(B, 32): the FC-hidden, logit-partial and hidden-grad phases are as
//    many times as long per thread as a block has samples in flight, and the
//    other CUs idle anyway.  The chunk loop and the [HS] row buffers are the
//    oracle's, with HS = 1; traces of 4, 2 and 1 samples a block at B = 128
//    are in docs/KERNELS.md, "Round 9".
#define HD2_WS (KFC + 4)           // 16-byte aligned, rows 4 banks apart
#define HD2_MAXB 128
#define LDS4(p) (*reinterpret_cast<const float4*>(p))   // 16-byte LDS read
__global__ void __launch_bounds__(256)
cs_head2_kernel(CachedPtrs P, CachedDims D) {
  constexpr int HS = 1;              // samples in flight per block
  __shared__ float sW2p[KA * HD_ROW];
  __shared__ __align__(16) float sW1p[KFIN * HD2_WS], sW1v[KFIN * HD2_WS];
  __shared__ float sWg[KGE * KGF];
  __shared__ float sB2p[KA];
  __shared__ float sGL[HS][KA], sGV[HS], sGF[HS][KFIN];
  __shared__ __align__(16) float sGHp[HS][HD2_WS], sGHv[HS][HD2_WS];
  // forward rows
  __shared__ float sFin[HS][KFIN], sHp[HS][HD_ROW], sVred[HS][KFC];
  __shared__ float sGf[HS][KGF], sU34[HS][KGF];
  __shared__ float sGamG[KGF], sBetG[KGF], sBg[KGE];
  __shared__ float sPart[HS][KA][16 + 1];
  __shared__ float sRow[HS][KA], sPp[HS][KA], sLp[HS][KA];
  __shared__ float sVal[HS], sCoef[HS], sHent[HS];
  const int tid = threadIdx.x;
  constexpr int NT = 256;
  for (int x = tid; x < KA * KFC; x += NT)
    sW2p[(x / KFC) * HD_ROW + hd_pad(x % KFC)] = WP(W_P2_W)[x];
  for (int x = tid; x < KGE * KGF; x += NT) sWg[x] = WP(W_G_W)[x];
  if (tid < KA) sB2p[tid] = WP(W_P2_B)[tid];
  if (tid < KGF) {
    sGamG[tid] = WP(W_LN_G_W)[tid];
    sBetG[tid] = WP(W_LN_G_B)[tid];
  }
  if (tid < KGE) sBg[tid] = WP(W_G_B)[tid];
  float w1p[KFIN], w1v[KFIN];
#pragma unroll
  for (int i = 0; i < KFIN; ++i) {
    w1p[i] = WP(W_P1_W)[tid * KFIN + i];
    w1v[i] = WP(W_V1_W)[tid * KFIN + i];
  }
  // the backward's LDS copy of W1p / W1v, i-major: thread j writes column j
#pragma unroll
  for (int i = 0; i < KFIN; ++i) {
    sW1p[i * HD2_WS + tid] = w1p[i];
    sW1v[i * HD2_WS + tid] = w1v[i];
  }
  const float b1p = WP(W_P1_B)[tid], b1v = WP(W_V1_B)[tid];
  const float w2v = WP(W_V2_W)[tid];
  const float b2v = WP(W_V2_B)[0];
  const float klc = P.kl[0];
  const int wv = tid >> 6, ln = tid & 63;
  const int per = (D.B + gridDim.x - 1) / gridDim.x;
  const int b0 = blockIdx.x * per;
  const int b1 = min(D.B, b0 + per);
  for (int c0 = b0; c0 < b1; c0 += HS) {
    const int ns = min(HS, b1 - c0);
    // per-sample inputs of the chunk, clamped instead of branched on: row
    // thread x = (s, a) its mask entry and its sample's action; lane 0 of
    // wave s the loss row's scalars; thread 128 + s the value target
    const int xr_ = min(tid, ns * KA - 1);
    const float r_mask = P.mask[(long)c0 * KA + xr_];
    const long r_act = P.actions[c0 + xr_ / KA];
    const int bw_ = c0 + min(wv, ns - 1);
    const long w_act = P.actions[bw_];
    const float w_old_lp = P.old_logp[bw_];
    const float w_adv = P.adv[bw_];
    const float r_vtarg = P.vtarg[c0 + min(max(tid - 128, 0), ns - 1)];
    for (int x = tid; x < ns * KGF; x += NT)
      sGf[x / KGF][x % KGF] = P.gf[(long)c0 * KGF + x];
    for (int x = tid; x < ns * KOUT; x += NT) {
      const int s = x / KOUT, i = x % KOUT;
      const long mid = P.model_ids[c0 + s];
      const float pv = P.pooled[mid * KOUT + i];
      sFin[s][i] = pv;
      P.fin[(long)(c0 + s) * KFIN + i] = pv;
    }
    const float fmin = -3.402823466e+38f;
    float r_lm = logf(r_mask);
    if (!(r_lm > fmin)) r_lm = fmin;
    __syncthreads();
    for (int x = tid; x < ns * KGF; x += NT) {
      const int s = x / KGF, i = x % KGF;
      const float* __restrict__ xr = sGf[s];
      float sum = 0.f;
#pragma unroll
      for (int k = 0; k < KGF; ++k) sum = sum + xr[k];
      const float mu = sum / KGF;
      float var;
      {
        const float d0 = xr[0] - mu;
        var = d0 * d0;
      }
#pragma unroll
      for (int k = 1; k < KGF; ++k) {
        const float d = xr[k] - mu;
        var = var + d * d;
      }
      const float rstd = rsqrtf(var / KGF + LN_EPS);
      const float xh = (xr[i] - mu) * rstd;
      P.xh34[(long)(c0 + s) * KGF + i] = xh;
      sU34[s][i] = FMA(xh, sGamG[i], sBetG[i]);
    }
    __syncthreads();
    for (int x = tid; x < ns * KGE; x += NT) {
      const int s = x / KGE, o = x % KGE;
      float acc = sBg[o];
#pragma unroll
      for (int i = 0; i < KGF; ++i)
        acc = FMA(sWg[o * KGF + i], sU34[s][i], acc);
      sFin[s][KOUT + o] = acc;               // graph_module has NO activation
      P.fin[(long)(c0 + s) * KFIN + KOUT + o] = acc;
    }
    __syncthreads();
    // FC hidden layers: bias first, i ascending
    float hp[HS], hv[HS];
#pragma unroll
    for (int s = 0; s < HS; ++s) {
      hp[s] = 0.f;
      hv[s] = 0.f;
      if (s < ns) {
        float ap = b1p, av = b1v;
#pragma unroll
        for (int i = 0; i < KFIN; ++i) {
          ap = FMA(w1p[i], sFin[s][i], ap);
          av = FMA(w1v[i], sFin[s][i], av);
        }
        ap = ap > 0.f ? ap : 0.f;
        av = av > 0.f ? av : 0.f;
        const long u = (long)(c0 + s) * KFC + tid;
        P.h1p[u] = ap;
        P.h1v[u] = av;
        hp[s] = ap;
        hv[s] = av;
        sHp[s][hd_pad(tid)] = ap;
        sVred[s][tid] = w2v * av;
      }
    }
    __syncthreads();
    // logit partials over the 16 chunks of the hidden row
    for (int x = tid; x < ns * KA * 16; x += NT) {
      const int s = x / (KA * 16), r = x % (KA * 16);
      const int a = r / 16, c = r % 16;
      const float* __restrict__ w = sW2p + a * HD_ROW + c * HD_CS;
      const float* __restrict__ h = sHp[s] + c * HD_CS;
      float acc = FMA(w[0], h[0], 0.f);
#pragma unroll
      for (int i = 1; i < 16; ++i) {
        if (i < 4) acc = FMA(w[i], h[i], acc);
        else acc = acc + w[i] * h[i];
      }
      sPart[s][a][c] = acc;
    }
    // value: wave s folds sample s's 256 products in the halving tree's
    // pairing (t with t + 128, 64, ... 1)
    if (wv < ns) {
      const float* __restrict__ vr = sVred[wv];
      float a0 = vr[ln] + vr[ln + 128];
      const float a1 = vr[ln + 64] + vr[ln + 192];
      a0 = a0 + a1;
#pragma unroll
      for (int off = 32; off > 0; off >>= 1)
        a0 = a0 + __shfl_down(a0, off, 64);
      if (ln == 0) {
        const float val = a0 + b2v;
        sVal[wv] = val;
        P.values[c0 + wv] = val;
      }
    }
    __syncthreads();
    // raw masked logits
    if (tid < ns * KA) {
      const int s = tid / KA, a = tid % KA;
      float acc = sB2p[a];
#pragma unroll
      for (int c = 0; c < 16; ++c) acc = acc + sPart[s][a][c];
      sRow[s][a] = acc + r_lm;
    }
    __syncthreads();
    // softmax / surrogate row of sample s: lane 0 of wave s
    if (wv < ns && ln == 0) {
      const int s = wv;
      const int b = c0 + s;
      const float* __restrict__ row = sRow[s];
      float mx = -3.0e38f;
#pragma unroll
      for (int a = 0; a < KA; ++a) mx = fmaxf(mx, row[a]);
      float Z = 0.f;
#pragma unroll
      for (int a = 0; a < KA; ++a) Z = Z + __expf(row[a] - mx);
      const float lse = mx + __logf(Z);
      float ent = 0.f;
#pragma unroll
      for (int a = 0; a < KA; ++a) {
        const float lp = row[a] - lse;
        const float e = __expf(lp);
        sLp[s][a] = lp;
        sPp[s][a] = e;
        ent = FMA(-lp, e, ent);
      }
      const float logp_a = sLp[s][w_act];
      const float ratio = __expf(logp_a - w_old_lp);
      const float A_b = w_adv;
      const float r_cl = fminf(fmaxf(ratio, 1.f - D.clip), 1.f + D.clip);
      const float surr1 = ratio * A_b, surr2 = r_cl * A_b;
      float ds = ratio * A_b;
      if (surr2 < surr1 && (ratio < 1.f - D.clip || ratio > 1.f + D.clip))
        ds = 0.f;
      const float coef = -ds - klc;
      P.hent[b] = ent;
      P.coef[b] = coef;
      sHent[s] = ent;
      sCoef[s] = coef;
    }
    __syncthreads();
    // loss backward rows (upstream grad = 1); p and lp go out here
    if (tid < ns * KA) {
      const int s = tid / KA, a = tid % KA;
      const int b = c0 + s;
      const long u = (long)b * KA + a;
      const float c = sCoef[s] / D.B;
      const float pj = sPp[s][a];
      const float lpj = sLp[s][a];
      P.p[u] = pj;
      P.lp[u] = lpj;
      const float delta = (a == (int)r_act) ? 1.f : 0.f;
      const float gl = mul_rn(c, delta - pj)
                       + mul_rn(mul_rn(D.ent_coef / D.B, pj),
                                lpj + sHent[s]);
      P.glogits[u] = gl;
      sGL[s][a] = gl;
    }
    if (tid >= 128 && tid < 128 + ns) {
      const int s = tid - 128;
      const int b = c0 + s;
      const float verr = sVal[s] - r_vtarg;
      const float mk = (verr * verr <= D.vf_clip) ? 1.f : 0.f;
      const float gv = D.vf_coef * 2.f * verr * mk / D.B;
      P.gvalue[b] = gv;
      sGV[s] = gv;
    }
    __syncthreads();
    // hidden grads
#pragma unroll
    for (int s = 0; s < HS; ++s) {
      if (s < ns) {
        const int j = tid;
        const long u = (long)(c0 + s) * KFC + j;
        float acc = 0.f;
#pragma unroll
        for (int a = 0; a < KA; ++a) {
          // the first five terms are fused, the rest rounded products
          const float w = sW2p[a * HD_ROW + hd_pad(j)];
          if (a < 5) acc = FMA(w, sGL[s][a], acc);
          else acc = acc + mul_rn(w, sGL[s][a]);
        }
        const float gp = hp[s] > 0.f ? acc : 0.f;
        const float av = w2v * sGV[s];
        const float gv = hv[s] > 0.f ? av : 0.f;
        P.gh1p[u] = gp;
        P.gh1v[u] = gv;
        sGHp[s][j] = gp;
        sGHv[s][j] = gv;
      }
    }
    __syncthreads();
    // gfinal: one thread per (sample, i), j = 0..FC-1 in order, four j a read
    if (tid < ns * KFIN) {
      const int s = tid / KFIN, i = tid % KFIN;
      const float* __restrict__ wp = sW1p + i * HD2_WS;
      const float* __restrict__ wvv = sW1v + i * HD2_WS;
      const float* __restrict__ gp = sGHp[s];
      const float* __restrict__ gv = sGHv[s];
      float acc = 0.f;
#pragma unroll 4
      for (int j = 0; j < KFC; j += 4) {
        const float4 a = LDS4(wp + j), b = LDS4(wvv + j);
        const float4 g = LDS4(gp + j), h = LDS4(gv + j);
        acc = FMA(a.x, g.x, acc);
        acc = FMA(b.x, h.x, acc);
        acc = FMA(a.y, g.y, acc);
        acc = FMA(b.y, h.y, acc);
        acc = FMA(a.z, g.z, acc);
        acc = FMA(b.z, h.z, acc);
        acc = FMA(a.w, g.w, acc);
        acc = FMA(b.w, h.w, acc);
      }
      P.gfinal[(long)(c0 + s) * KFIN + i] = acc;
      sGF[s][i] = acc;
    }
    __syncthreads();
    // graph-module LN-out grads
    for (int x = tid; x < ns * KGF; x += NT) {
      const int s = x / KGF, i = x % KGF;
      float acc = 0.f;
#pragma unroll
      for (int o = 0; o < KGE; ++o)
        acc = acc + mul_rn(sWg[o * KGF + i], sGF[s][KOUT + o]);
      P.gu34[(long)(c0 + s) * KGF + i] = acc;
    }
    // The next chunk's first barrier separates these reads from the next
    // writes of the row buffers, as in cs_head_kernel.
  }
}

// ---- cs_fwd_combine<2> + the per-model means of cs_fwd_pool ----
// One block per model: its nodes' h2 rows are computed into the LDS tile
// (and written out), then unit i adds them in node order, as a chain out of
// LDS.  The per-sample half of cs_fwd_pool_kernel is in cs_head_kernel.
__global__ void __launch_bounds__(256)
cs_fwd_comb2_pool_kernel(CachedPtrs P, CachedDims D) {
  constexpr int PT = 256;   // node rows of h2 per tile
  __shared__ float sH2[PT * KOUT];
  const int tid = threadIdx.x;
  const int m = blockIdx.x;
  const long lo = P.model_nptr[m], hi = P.model_nptr[m + 1];
  float acc = 0.f;
  for (long v0 = lo; v0 < hi; v0 += PT) {
    const long v1 = min(hi, v0 + PT);
    __syncthreads();
    for (long x = tid; x < (v1 - v0) * KOUT; x += 256) {
      const long v = v0 + x / KOUT;
      const int i = (int)(x % KOUT);
      const long qlo = P.indptr[v], qhi = P.indptr[v + 1];
      float out = 0.f;
      if (qhi > qlo) {
        float a = P.rs2[v * KOUT + i];
        for (long q = qlo; q < qhi; ++q)
          a = a + P.re2[P.order[q] * KOUT + i];
        out = a / (float)(qhi - qlo + 1);
      }
      P.h2[v * KOUT + i] = out;
      sH2[x] = out;
    }
    __syncthreads();
    if (tid < KOUT)
      for (long v = v0; v < v1; ++v) acc = acc + sH2[(v - v0) * KOUT + tid];
  }
  if (tid < KOUT) P.pooled[(long)m * KOUT + tid] = acc / (float)(hi - lo);
}

// ---- cs_fwd_combine<1> inside cs_fwd_mlp_lanes<2>'s staging loop ----
// The node rows of the block are h1 rows: each staged element is computed
// here, (rs1[v] + sum over the in-edges in CSR order of re1) / (deg + 1),
// 0 without in-edges, and written to h1 for the backward.
template <int L>
__global__ void __launch_bounds__(ROW_NT)
cs_fwd_comb1_mlp2_lanes_kernel(CachedPtrs P, CachedDims D) {
  constexpr int RPB = ROW_NT / L;
  const int nbN = (D.N + RPB - 1) / RPB;
  if ((int)blockIdx.x < nbN) {
    const long r0 = (long)blockIdx.x * RPB;
    rows_fwd_lanes<KHID, KH, 0, L>(
        P, W_LN_N2_W, r0, D.N,
        [&](long v, int i) {
          const long lo = P.indptr[v], hi = P.indptr[v + 1];
          float out = 0.f;
          if (hi > lo) {
            float acc = P.rs1[v * KHID + i];
            for (long q = lo; q < hi; ++q)
              acc = acc + P.re1[P.order[q] * KHID + i];
            out = acc / (float)(hi - lo + 1);
          }
          P.h1[v * KHID + i] = out;
          return out;
        },
        P.xh_h2, P.rst_h2, P.hn2);
  } else {
    const long r0 = (long)(blockIdx.x - nbN) * RPB;
    rows_fwd_lanes<KFE, KH, 0, L>(
        P, W_LN_E2_W, r0, D.E,
        [&](long k, int i) { return P.e[k * KFE + i]; },
        P.xh_e2, P.rst_e2, P.he2);
  }
}

// ---- cs_bwd_scatter<2> inside cs_bwd_mlp2_lanes's staging loop ----
// ghn2[v] = gms2[v][:KH] + sum over the out-edges in src-CSR order of
// gme2[.][:KH]; ghe2[k] = gme2[k][KH:].  Both are still written out.
template <int L>
__global__ void __launch_bounds__(ROW_NT)
cs_bwd_scat2_mlp2_lanes_kernel(CachedPtrs P, CachedDims D) {
  constexpr int RPB = ROW_NT / L;
  const int nbN = (D.N + RPB - 1) / RPB;
  if ((int)blockIdx.x < nbN) {
    const long r0 = (long)blockIdx.x * RPB;
    rows_bwd_lanes<KHID, KH, KH, 0, L, true>(
        P, W_LN_N2_W, r0, D.N,
        [&](long v, int o) {
          const long lo = P.src_indptr[v], hi = P.src_indptr[v + 1];
          float acc = P.gms2[v * KMSG + o];
          for (long q = lo; q < hi; ++q)
            acc = acc + P.gme2[P.src_order[q] * KMSG + o];
          P.ghn2[v * KH + o] = acc;
          return acc;
        },
        P.hn2, P.xh_h2, P.rst_h2, P.gpn1, P.gu_h2, P.gh1b);
  } else {
    const long r0 = (long)(blockIdx.x - nbN) * RPB;
    rows_bwd_lanes<KFE, KH, KH, 0, L, false>(
        P, W_LN_E2_W, r0, D.E,
        [&](long k, int o) {
          const float g = P.gme2[k * KMSG + KH + o];
          P.ghe2[k * KH + o] = g;
          return g;
        },
        P.he2, nullptr, nullptr, P.gpe1, P.gu_e2, nullptr);
  }
}

// ---- cs_bwd_scatter<1> + cs_bwd_gu1 ----
// A block owns SG_RPB rows of one class (node blocks first, then edge
// blocks): thread (r, i) scatters element i of row r with the relu mask,
// the row stays in LDS, then one thread per gu element runs the 16-term
// chain (all fused, from 0, o ascending).
//
// The grid's last block takes the C_STATS sums (logging only), which
// cs_head_kernel leaves out.  It recomputes cs_fwd_loss_kernel's four terms
// per sample from the stored rows (lp, values, hent: the same single
// operations, so the same bits), sums them per group of 32 samples in sample
// order, as that kernel's blocks do in LDS, and one thread adds the group
// partials to C_STATS with float atomics in group order: the result
// cs_fwd_loss_kernel gives when its blocks' atomics arrive in block order,
// and the same bits on every run.
#define SG_RPB (ROW_NT / KH)
#define SG_SPB 32     // samples per statistics group
#define SG_MAXB 1024  // cached_step_bwd refuses larger minibatches
__global__ void __launch_bounds__(ROW_NT)
cs_bwd_scat1_gu1_kernel(CachedPtrs P, CachedDims D) {
  __shared__ float sWN[KH * KF0], sWE[KH * KFE];
  __shared__ float sG[SG_RPB][KH + 1];
  const int tid = threadIdx.x;
  for (int x = tid; x < KH * KF0; x += ROW_NT) sWN[x] = WP(W_N1_W)[x];
  for (int x = tid; x < KH * KFE; x += ROW_NT) sWE[x] = WP(W_E1_W)[x];
  const int nbN = (D.N + SG_RPB - 1) / SG_RPB;
  const int nbE = (D.E + SG_RPB - 1) / SG_RPB;
  const int r = tid / KH, i = tid % KH;
  if ((int)blockIdx.x >= nbN + nbE) {
    __shared__ float sT[SG_MAXB][4];
    __shared__ float sAcc[SG_MAXB / SG_SPB][4];
    for (int b = tid; b < D.B; b += ROW_NT) {
      const float logp_a = P.lp[(long)b * KA + P.actions[b]];
      const float old_lp = P.old_logp[b];
      const float ratio = __expf(logp_a - old_lp);
      const float A_b = P.adv[b];
      const float r_cl = fminf(fmaxf(ratio, 1.f - D.clip), 1.f + D.clip);
      const float surr1 = ratio * A_b, surr2 = r_cl * A_b;
      const float verr = P.values[b] - P.vtarg[b];
      sT[b][0] = -fminf(surr1, surr2);
      sT[b][1] = fminf(verr * verr, D.vf_clip);
      sT[b][2] = old_lp - logp_a;
      sT[b][3] = P.hent[b];
    }
    __syncthreads();
    const int ng = (D.B + SG_SPB - 1) / SG_SPB;
    // thread (g, k): statistic k of group g, samples in order
    for (int x = tid; x < ng * 4; x += ROW_NT) {
      const int g = x / 4, k = x % 4;
      const int b_lo = g * SG_SPB;
      const int nb = min(D.B - b_lo, SG_SPB);
      float acc = sT[b_lo][k];
      for (int t = 1; t < nb; ++t) acc = acc + sT[b_lo + t][k];
      sAcc[g][k] = acc;
    }
    __syncthreads();
    if (tid == 0) {
      const float inv = 1.f / D.B;
      const float klc = P.kl[0];
      for (int g = 0; g < ng; ++g) {
        const float pl = sAcc[g][0] * inv;
        const float vf = sAcc[g][1] * inv;
        const float kl = sAcc[g][2] * inv;
        const float ent = sAcc[g][3] * inv;
        atomicAdd(&P.stats[0], pl);
        atomicAdd(&P.stats[1], vf);
        atomicAdd(&P.stats[2], kl);
        atomicAdd(&P.stats[3], ent);
        atomicAdd(&P.stats[4],
                  FMA(-D.ent_coef, ent, FMA(D.vf_coef, vf, FMA(kl, klc, pl))));
      }
    }
  } else if ((int)blockIdx.x < nbN) {
    const long r0 = (long)blockIdx.x * SG_RPB;
    const long v = r0 + r;
    float g = 0.f;
    if (v < D.N) {
      const long lo = P.src_indptr[v], hi = P.src_indptr[v + 1];
      float acc = P.gms1[v * KMSG + i];
      for (long q = lo; q < hi; ++q)
        acc = acc + P.gme1[P.src_order[q] * KMSG + i];
      g = P.hn1[v * KH + i] > 0.f ? acc : 0.f;
      P.ghn1[v * KH + i] = g;
    }
    sG[r][i] = g;
    __syncthreads();
    for (int x = tid; x < SG_RPB * KF0; x += ROW_NT) {
      const int rr = x / KF0, ii = x % KF0;
      if (r0 + rr < D.N) {
        float acc = 0.f;
#pragma unroll
        for (int o = 0; o < KH; ++o)
          acc = FMA(sWN[o * KF0 + ii], sG[rr][o], acc);
        P.gu_z1[(r0 + rr) * KF0 + ii] = acc;
      }
    }
  } else {
    const long r0 = (long)(blockIdx.x - nbN) * SG_RPB;
    const long k = r0 + r;
    float g = 0.f;
    if (k < D.E) {
      const float ge = P.gme1[k * KMSG + KH + i];
      g = P.he1[k * KH + i] > 0.f ? ge : 0.f;
      P.ghe1[k * KH + i] = g;
    }
    sG[r][i] = g;
    __syncthreads();
    for (int x = tid; x < SG_RPB * KFE; x += ROW_NT) {
      const int rr = x / KFE, ii = x % KFE;
      if (r0 + rr < D.E) {
        float acc = 0.f;
#pragma unroll
        for (int o = 0; o < KH; ++o)
          acc = FMA(sWE[o * KFE + ii], sG[rr][o], acc);
        P.gu_e1[(r0 + rr) * KFE + ii] = acc;
      }
    }
  }
}

// ===========================================================================
// work off the serial chain (DDLS_AMD_STEP_OVERLAP, default on)
// ===========================================================================
//
// A replay is one serial chain of launches.  Two pieces of work sat on it
// although nothing ahead of them in the chain produces their inputs; each now
// rides as extra blocks of a launch that exists anyway (different roles per
// block index, like the statistics block of cs_bwd_scat1_gu1_kernel), so the
// chain stays serial and every output element keeps its summation order.

// ---- cs_bwd_pool + the B-row ("special") blocks of cs_bwd_w ----
// Blocks [0, M): pool role, one block per model.  Block M: the graph-module
// weight-grad job.  Blocks M+1 .. M+16: the FC-column jobs.  The special jobs
// read only what cs_head_kernel wrote, so they run here, five launches
// earlier than in cs_bwd_w_kernel, which is then launched with its row-job
// blocks only.  Arithmetic is that of cs_bwd_pool_kernel and of
// cs_bwd_w_kernel's special blocks, term for term; what changes is the
// staging: a super-tile of up to WFC_ST sample rows per global round trip
// instead of TILE_K, walked in TILE_K-row tiles so a chain sees the same
// full / partial tiles as before.
#define WFC_ST 128        // sample rows per super-tile (a multiple of TILE_K)
#define WFC_NFC 16        // FC-column blocks
// LDS floats per role; the kernel's buffer is their maximum (a union)
#define WFC_LDS_POOL (1024 + WFC_ST * KOUT + KOUT)
#define WFC_LDS_G (WFC_ST * (KGE + 3 * KGF))
#define WFC_LDS_FC (WFC_ST * (KFIN + 4 * 16 + KA + 1))
#define WFC_LDS (WFC_LDS_G > WFC_LDS_FC ? WFC_LDS_G : WFC_LDS_FC)
static_assert(WFC_LDS >= WFC_LDS_POOL, "pool role LDS");
static_assert(WFC_LDS * 4 <= 64 * 1024, "cs_bwd_pool_wfc: LDS over 64 KB");
static_assert(WFC_ST % TILE_K == 0, "super-tile of whole tiles");
static_assert(KFC / WFC_NFC == 16 && KFC % WFC_NFC == 0, "16 columns a block");

__global__ void __launch_bounds__(256)
cs_bwd_pool_wfc_kernel(CachedPtrs P, CachedDims D) {
  __shared__ float lds[WFC_LDS];
  const int tid = threadIdx.x;
  constexpr int NT = 256;
  const int bid = blockIdx.x;

  if (bid < D.M) {
    // ---- pool role: gpool[m] and this model's gh2 rows ----
    const int m = bid;
    int* smid = reinterpret_cast<int*>(lds);            // [1024]
    float (*sG)[KOUT] = reinterpret_cast<float (*)[KOUT]>(lds + 1024);
    float* sP = lds + 1024 + WFC_ST * KOUT;             // [KOUT]
    // read ahead of the chain; used after it
    const long lo = P.model_nptr[m], hi = P.model_nptr[m + 1];
    for (int b = tid; b < D.B; b += NT) smid[b] = (int)P.model_ids[b];
    float acc = 0.f;
    for (int t0 = 0; t0 < D.B; t0 += WFC_ST) {
      const int bt = min(WFC_ST, D.B - t0);
      float rG[WFC_ST * KOUT / NT];
#pragma unroll
      for (int k = 0; k < WFC_ST * KOUT / NT; ++k) {
        const int x = min(tid + k * NT, bt * KOUT - 1);
        rG[k] = P.gfinal[(long)(t0 + x / KOUT) * KFIN + x % KOUT];
      }
      __syncthreads();
#pragma unroll
      for (int k = 0; k < WFC_ST * KOUT / NT; ++k) {
        const int x = tid + k * NT;
        if (x < bt * KOUT) sG[x / KOUT][x % KOUT] = rG[k];
      }
      __syncthreads();
      if (tid < KOUT) {
        if (bt == WFC_ST) {
#pragma unroll 8
          for (int b = 0; b < WFC_ST; ++b)
            acc += (smid[t0 + b] == m) ? sG[b][tid] : 0.f;
        } else {
          for (int b = 0; b < bt; ++b)
            acc += (smid[t0 + b] == m) ? sG[b][tid] : 0.f;
        }
      }
    }
    if (tid < KOUT) {
      P.gpool[(long)m * KOUT + tid] = acc;
      sP[tid] = acc;
    }
    __syncthreads();
    const float nn = (float)(hi - lo);
    for (long u = lo * KOUT + tid; u < hi * KOUT; u += NT)
      P.gh2[u] = sP[u % KOUT] / nn;
    return;
  }

  if (bid == D.M) {
    // ---- graph module: Wg[GEMB,GFin], bg; LN gamma/beta from gu34 + xh34.
    // gpre rows are gfinal[:, KOUT:KOUT+KGE] (row stride KFIN).
    float (*tG)[KGE] = reinterpret_cast<float (*)[KGE]>(lds);
    float (*tU)[KGF] = reinterpret_cast<float (*)[KGF]>(lds + WFC_ST * KGE);
    float (*tXH)[KGF] =
        reinterpret_cast<float (*)[KGF]>(lds + WFC_ST * (KGE + KGF));
    float (*tGU)[KGF] =
        reinterpret_cast<float (*)[KGF]>(lds + WFC_ST * (KGE + 2 * KGF));
    const float* __restrict__ gam = WP(W_LN_G_W);
    const float* __restrict__ bet = WP(W_LN_G_B);
    constexpr int UNITS = KGE * KGF;
    constexpr int MYU = (UNITS + 255) / 256;
    float acc[MYU];
#pragma unroll
    for (int q = 0; q < MYU; ++q) acc[q] = 0.f;
    // tid in [64, 64+KGE): bias sums; tid in [128, 128+KGF): LN gamma/beta
    float bacc = 0.f, lacc_w = 0.f, lacc_b = 0.f;
    for (int r0 = 0; r0 < D.B; r0 += WFC_ST) {
      const int rt = min(WFC_ST, D.B - r0);
      // Every global load of the super-tile is issued before the first LDS
      // store: constant trip counts, indices clamped instead of branched on
      // so the loads share a basic block.  One round trip per super-tile.
      {
        constexpr int CG = WFC_ST * KGE / NT, CX = WFC_ST * KGF / NT;
        static_assert(CG * NT == WFC_ST * KGE && CX * NT == WFC_ST * KGF,
                      "whole trips");
        float rG[CG], rXH[CX], rGU[CX], rGam[CX], rBet[CX];
#pragma unroll
        for (int k = 0; k < CG; ++k) {
          const int x = min(tid + k * NT, rt * KGE - 1);
          rG[k] = P.gfinal[(long)(r0 + x / KGE) * KFIN + KOUT + x % KGE];
        }
#pragma unroll
        for (int k = 0; k < CX; ++k) {
          const int x = min(tid + k * NT, rt * KGF - 1);
          rXH[k] = P.xh34[(long)r0 * KGF + x];
          rGU[k] = P.gu34[(long)r0 * KGF + x];
          rGam[k] = gam[x % KGF];
          rBet[k] = bet[x % KGF];
        }
#pragma unroll
        for (int k = 0; k < CG; ++k) {
          const int x = tid + k * NT;
          if (x < rt * KGE) tG[x / KGE][x % KGE] = rG[k];
        }
#pragma unroll
        for (int k = 0; k < CX; ++k) {
          const int x = tid + k * NT;
          if (x < rt * KGF) {
            const int t = x / KGF, i = x % KGF;
            tU[t][i] = FMA(rXH[k], rGam[k], rBet[k]);
            tXH[t][i] = rXH[k];
            tGU[t][i] = rGU[k];
          }
        }
      }
      __syncthreads();
      // a full super-tile has constant trip counts: the LDS reads of a chain
      // run ahead of its adds
#pragma unroll
      for (int q = 0; q < MYU; ++q) {
        int u = tid + q * 256;
        if (u < UNITS) {
          int o = u / KGF, i = u % KGF;
          float a = acc[q];
          if (rt == WFC_ST) {
#pragma unroll 16
            for (int t = 0; t < WFC_ST; ++t) a = FMA(tG[t][o], tU[t][i], a);
          } else {
            for (int t = 0; t < rt; ++t) a = FMA(tG[t][o], tU[t][i], a);
          }
          acc[q] = a;
        }
      }
      if (tid >= 64 && tid < 64 + KGE) {
        if (rt == WFC_ST) {
#pragma unroll 16
          for (int t = 0; t < WFC_ST; ++t) bacc = bacc + tG[t][tid - 64];
        } else {
          for (int t = 0; t < rt; ++t) bacc = bacc + tG[t][tid - 64];
        }
      }
      if (tid >= 128 && tid < 128 + KGF) {
        if (rt == WFC_ST) {
#pragma unroll 16
          for (int t = 0; t < WFC_ST; ++t) {
            lacc_w = lacc_w + mul_rn(tGU[t][tid - 128], tXH[t][tid - 128]);
            lacc_b = lacc_b + tGU[t][tid - 128];
          }
        } else {
          for (int t = 0; t < rt; ++t) {
            lacc_w = lacc_w + mul_rn(tGU[t][tid - 128], tXH[t][tid - 128]);
            lacc_b = lacc_b + tGU[t][tid - 128];
          }
        }
      }
      __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < MYU; ++q) {
      int u = tid + q * 256;
      if (u < UNITS) WG_(W_G_W)[u] = acc[q];
    }
    if (tid >= 64 && tid < 64 + KGE) WG_(W_G_B)[tid - 64] = bacc;
    if (tid >= 128 && tid < 128 + KGF) {
      WG_(W_LN_G_W)[tid - 128] = lacc_w;
      WG_(W_LN_G_B)[tid - 128] = lacc_b;
    }
    return;
  }

  // ---- FC-column jobs: block jb owns columns [j0, j0 + 16) of W1p/W1v
  // [FC,FIN] (+ b1p/b1v) AND of W2p [A,FC] / W2v [FC]; block 0 also sums b2p
  // and b2v.
  {
    constexpr int JW = KFC / WFC_NFC;   // 16
    const int jb = bid - D.M - 1;
    if (jb >= WFC_NFC) return;
    const int j0 = jb * JW;
    float* q_ = lds;
    float (*tF)[KFIN] = reinterpret_cast<float (*)[KFIN]>(q_);
    q_ += WFC_ST * KFIN;
    float (*tGp)[16] = reinterpret_cast<float (*)[16]>(q_);
    q_ += WFC_ST * 16;
    float (*tGv)[16] = reinterpret_cast<float (*)[16]>(q_);
    q_ += WFC_ST * 16;
    float (*tHp)[16] = reinterpret_cast<float (*)[16]>(q_);
    q_ += WFC_ST * 16;
    float (*tHv)[16] = reinterpret_cast<float (*)[16]>(q_);
    q_ += WFC_ST * 16;
    float (*tGL)[KA] = reinterpret_cast<float (*)[KA]>(q_);
    q_ += WFC_ST * KA;
    float* tGV = q_;                                    // [WFC_ST]
    constexpr int MYU = (16 * KFIN + 255) / 256;
    constexpr int MYU2 = (16 * KA + 255) / 256;
    float accp[MYU], accv[MYU], acc2[MYU2];
#pragma unroll
    for (int q = 0; q < MYU; ++q) { accp[q] = 0.f; accv[q] = 0.f; }
#pragma unroll
    for (int q = 0; q < MYU2; ++q) acc2[q] = 0.f;
    // The single-chain sums sit in the waves with the fewest weight units
    // (units fill tid 0.. upwards).  tid in [192, 192+JW): column sums
    // b1p/b1v and the W2v column; jb == 0 only: tid in [128, 128+KA) sums
    // b2p, tid == 128+KA sums b2v
    const int cj = tid - 192;
    float bp = 0.f, bv = 0.f, w2v = 0.f, b2 = 0.f;
    for (int s0 = 0; s0 < D.B; s0 += WFC_ST) {
      const int st = min(WFC_ST, D.B - s0);
      // as in the graph-module role: all global loads of the super-tile
      // first (clamped indices, one basic block), then the LDS stores
      {
        constexpr int CF = WFC_ST * KFIN / NT, CJ = WFC_ST * JW / NT;
        constexpr int CL = (WFC_ST * KA + NT - 1) / NT;
        static_assert(CF * NT == WFC_ST * KFIN && CJ * NT == WFC_ST * JW
                      && WFC_ST <= NT, "whole trips");
        float rF[CF], rGp[CJ], rGv[CJ], rHp[CJ], rHv[CJ], rGL[CL];
#pragma unroll
        for (int k = 0; k < CF; ++k) {
          const int x = min(tid + k * NT, st * KFIN - 1);
          rF[k] = P.fin[(long)s0 * KFIN + x];
        }
#pragma unroll
        for (int k = 0; k < CJ; ++k) {
          const int x = min(tid + k * NT, st * JW - 1);
          const long g = (long)(s0 + x / JW) * KFC + j0 + x % JW;
          rGp[k] = P.gh1p[g];
          rGv[k] = P.gh1v[g];
          rHp[k] = P.h1p[g];
          rHv[k] = P.h1v[g];
        }
#pragma unroll
        for (int k = 0; k < CL; ++k) {
          const int x = min(tid + k * NT, st * KA - 1);
          rGL[k] = P.glogits[(long)s0 * KA + x];
        }
        const float rGV = P.gvalue[s0 + min(tid, st - 1)];
#pragma unroll
        for (int k = 0; k < CF; ++k) {
          const int x = tid + k * NT;
          if (x < st * KFIN) tF[x / KFIN][x % KFIN] = rF[k];
        }
#pragma unroll
        for (int k = 0; k < CJ; ++k) {
          const int x = tid + k * NT;
          if (x < st * JW) {
            const int t = x / JW, j = x % JW;
            tGp[t][j] = rGp[k];
            tGv[t][j] = rGv[k];
            tHp[t][j] = rHp[k];
            tHv[t][j] = rHv[k];
          }
        }
#pragma unroll
        for (int k = 0; k < CL; ++k) {
          const int x = tid + k * NT;
          if (x < st * KA) tGL[x / KA][x % KA] = rGL[k];
        }
        if (tid < st) tGV[tid] = rGV;
      }
      __syncthreads();
      // the super-tile in TILE_K-row tiles: each chain sees the full and
      // partial tiles cs_bwd_w_kernel's special blocks saw
      for (int r0 = 0; r0 < st; r0 += TILE_K) {
        const int rt = min(TILE_K, st - r0);
#pragma unroll
        for (int q = 0; q < MYU; ++q) {
          int u = tid + q * NT;
          if (u < JW * KFIN) {
            int j = u / KFIN, i = u % KFIN;
            float ap = accp[q], av = accv[q];
            if (rt == TILE_K) {
#pragma unroll
              for (int t = 0; t < TILE_K; ++t) {
                ap = FMA(tGp[r0 + t][j], tF[r0 + t][i], ap);
                av = FMA(tGv[r0 + t][j], tF[r0 + t][i], av);
              }
            } else {
              for (int t = 0; t < rt; ++t) {
                ap = FMA(tGp[r0 + t][j], tF[r0 + t][i], ap);
                av = FMA(tGv[r0 + t][j], tF[r0 + t][i], av);
              }
            }
            accp[q] = ap;
            accv[q] = av;
          }
        }
#pragma unroll
        for (int q = 0; q < MYU2; ++q) {
          int u = tid + q * NT;
          if (u < KA * JW) {
            int a = u / JW, j = u % JW;
            float s = acc2[q];
            if (rt == TILE_K) {
#pragma unroll
              for (int t = 0; t < TILE_K; ++t) {
                // a full tile's first 20 terms are fused, the last 12 are
                // rounded products; a partial tile is fused throughout
                if (t < 20) s = FMA(tGL[r0 + t][a], tHp[r0 + t][j], s);
                else s = s + mul_rn(tGL[r0 + t][a], tHp[r0 + t][j]);
              }
            } else {
              for (int t = 0; t < rt; ++t)
                s = FMA(tGL[r0 + t][a], tHp[r0 + t][j], s);
            }
            acc2[q] = s;
          }
        }
      }
      if (cj >= 0 && cj < JW) {
        if (st == WFC_ST) {
#pragma unroll 16
          for (int t = 0; t < WFC_ST; ++t) {
            bp = bp + tGp[t][cj];
            bv = bv + tGv[t][cj];
            w2v = FMA(tGV[t], tHv[t][cj], w2v);
          }
        } else {
          for (int t = 0; t < st; ++t) {
            bp = bp + tGp[t][cj];
            bv = bv + tGv[t][cj];
            w2v = FMA(tGV[t], tHv[t][cj], w2v);
          }
        }
      }
      if (jb == 0) {
        if (tid >= 128 && tid < 128 + KA) {
          if (st == WFC_ST) {
#pragma unroll 16
            for (int t = 0; t < WFC_ST; ++t) b2 = b2 + tGL[t][tid - 128];
          } else {
            for (int t = 0; t < st; ++t) b2 = b2 + tGL[t][tid - 128];
          }
        }
        if (tid == 128 + KA) {
          if (st == WFC_ST) {
#pragma unroll 16
            for (int t = 0; t < WFC_ST; ++t) b2 = b2 + tGV[t];
          } else {
            for (int t = 0; t < st; ++t) b2 = b2 + tGV[t];
          }
        }
      }
      __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < MYU; ++q) {
      int u = tid + q * NT;
      if (u < JW * KFIN) {
        int j = u / KFIN, i = u % KFIN;
        WG_(W_P1_W)[(long)(j0 + j) * KFIN + i] = accp[q];
        WG_(W_V1_W)[(long)(j0 + j) * KFIN + i] = accv[q];
      }
    }
#pragma unroll
    for (int q = 0; q < MYU2; ++q) {
      int u = tid + q * NT;
      if (u < KA * JW) {
        int a = u / JW, j = u % JW;
        WG_(W_P2_W)[(long)a * KFC + j0 + j] = acc2[q];
      }
    }
    if (cj >= 0 && cj < JW) {
      WG_(W_P1_B)[j0 + cj] = bp;
      WG_(W_V1_B)[j0 + cj] = bv;
      WG_(W_V2_W)[j0 + cj] = w2v;
    }
    if (jb == 0) {
      if (tid >= 128 && tid < 128 + KA) WG_(W_P2_B)[tid - 128] = b2;
      if (tid == 128 + KA) WG_(W_V2_B)[0] = b2;
    }
  }
}

// ---- cs_bwd_pool_wfc with shorter roles (DDLS_AMD_STEP_HEAD, default on) ----
// Same launch, same outputs, same bits as cs_bwd_pool_wfc_kernel above, which
// stays unchanged as the oracle (DDLS_AMD_STEP_HEAD=off launches it).  The
// launch lasts as long as its slowest block, and every role's time is issue
// slots of one wave: LDS reads and dependent FMAs.  What changes:
//
//  * FC-column role: WFC2_JW columns a block instead of 16 (KFC / WFC2_JW
//    blocks instead of 16), so no thread carries more than one weight unit,
//    and the weight units, the W2p units and the single-chain sums sit in
//    different waves where the block has room.  Columns are independent
//    outputs: no partial sums, no reduce, every chain keeps its term order.
//  * Sample-major tiles are stored transposed ([column][sample], row stride
//    WFC2_TS), so a chain reads four consecutive samples of an operand with
//    one 16-byte LDS read: 3 reads + 8 FMAs per four terms of a W1p/W1v unit
//    instead of 12 + 8.  The terms are still consumed in sample order.
//  * Graph-module role: the same transposed layout and 16-byte reads.
//  * Pool role: wave 0 lists the model's samples once, in sample order, and
//    the chain then adds only those.  The oracle adds +0 for every other
//    sample.  Its accumulator starts at +0, and a round-to-nearest sum is -0
//    only when both addends are -0, so the accumulator is never -0 and adding
//    +0 to it never changes it: leaving those terms out gives the same bits.
//  * The weight slot offsets are loaded once at the top of a block, in the
//    same round trip as the first tile, not in front of the final stores.
//
// Tile pattern of the W2p units as in the oracle: the super-tile is walked in
// TILE_K-row tiles; a full tile's terms 0-19 are fused and 20-31 are rounded
// products, a partial tile is fused throughout.
#define WFC2_JW 4                       // FC columns per block
#define WFC2_NFC (KFC / WFC2_JW)        // FC-column blocks
#define WFC2_TS (WFC_ST + 4)            // transposed row stride (16 B aligned)
#define WFC2_LDS_POOL (2 * 1024 + WFC_ST * KOUT + KOUT + 16)
#define WFC2_LDS_G (WFC2_TS * (KGE + 3 * KGF))
#define WFC2_LDS_FC (WFC2_TS * (KFIN + 4 * WFC2_JW + KA + 1))
#define WFC2_LDS (WFC2_LDS_G > WFC2_LDS_FC ? WFC2_LDS_G : WFC2_LDS_FC)
static_assert(WFC2_LDS >= WFC2_LDS_POOL, "pool role LDS");
static_assert(WFC2_LDS * 4 <= 64 * 1024, "cs_bwd_pool_wfc2: LDS over 64 KB");
static_assert(WFC2_JW % 4 == 0 && KFC % WFC2_JW == 0, "whole float4 columns");
static_assert(WFC2_JW * KFIN <= 256, "one weight unit a thread");
static_assert(WFC_ST % 64 == 0 && SG_MAXB % WFC_ST == 0, "tiles of whole waves");
static_assert(TILE_K == 32, "20 fused + 12 rounded terms a full tile");

__global__ void __launch_bounds__(256)
cs_bwd_pool_wfc2_kernel(CachedPtrs P, CachedDims D) {
  __shared__ __align__(16) float lds[WFC2_LDS];
  const int tid = threadIdx.x;
  constexpr int NT = 256;
  constexpr int TS = WFC2_TS;
  const int bid = blockIdx.x;

  if (bid < D.M) {
    // ---- pool role: gpool[m] and this model's gh2 rows ----
    const int m = bid;
    int* smid = reinterpret_cast<int*>(lds);            // [1024]
    int* slist = smid + 1024;                           // [1024] members
    float (*sG)[KOUT] = reinterpret_cast<float (*)[KOUT]>(lds + 2048);
    float* sP = lds + 2048 + WFC_ST * KOUT;             // [KOUT]
    int* send = reinterpret_cast<int*>(sP + KOUT);      // [SG_MAXB / WFC_ST]
    const long lo = P.model_nptr[m], hi = P.model_nptr[m + 1];
    for (int b = tid; b < D.B; b += NT) smid[b] = (int)P.model_ids[b];
    float acc = 0.f;
    int k = 0;
    for (int t0 = 0; t0 < D.B; t0 += WFC_ST) {
      const int bt = min(WFC_ST, D.B - t0);
      float rG[WFC_ST * KOUT / NT];
#pragma unroll
      for (int q = 0; q < WFC_ST * KOUT / NT; ++q) {
        const int x = min(tid + q * NT, bt * KOUT - 1);
        rG[q] = P.gfinal[(long)(t0 + x / KOUT) * KFIN + x % KOUT];
      }
      __syncthreads();
      if (t0 == 0 && tid < 64) {
        // the model's samples in sample order; send[t]: how many of them lie
        // in super-tiles 0..t
        int cnt = 0;
        for (int b0 = 0; b0 < D.B; b0 += 64) {
          const int b = b0 + tid;
          const bool mine = b < D.B && smid[min(b, D.B - 1)] == m;
          const unsigned long long bal = __ballot(mine);
          if (mine) slist[cnt + __popcll(bal & ((1ull << tid) - 1ull))] = b;
          cnt += __popcll(bal);
          if (tid == 0 && ((b0 + 64) % WFC_ST == 0 || b0 + 64 >= D.B))
            send[b0 / WFC_ST] = cnt;
        }
      }
#pragma unroll
      for (int q = 0; q < WFC_ST * KOUT / NT; ++q) {
        const int x = tid + q * NT;
        if (x < bt * KOUT) sG[x / KOUT][x % KOUT] = rG[q];
      }
      __syncthreads();
      if (tid < KOUT) {
        const int k1 = send[t0 / WFC_ST];
#pragma unroll 4
        for (; k < k1; ++k) acc += sG[slist[k] - t0][tid];
      }
    }
    if (tid < KOUT) {
      P.gpool[(long)m * KOUT + tid] = acc;
      sP[tid] = acc;
    }
    __syncthreads();
    const float nn = (float)(hi - lo);
    for (long u = lo * KOUT + tid; u < hi * KOUT; u += NT)
      P.gh2[u] = sP[u % KOUT] / nn;
    return;
  }

  if (bid == D.M) {
    // ---- graph module: Wg[GEMB,GFin], bg; LN gamma/beta from gu34 + xh34.
    // gpre rows are gfinal[:, KOUT:KOUT+KGE] (row stride KFIN).
    float* tG = lds;                                    // [KGE][TS]
    float* tU = tG + KGE * TS;                          // [KGF][TS]
    float* tXH = tU + KGF * TS;                         // [KGF][TS]
    float* tGU = tXH + KGF * TS;                        // [KGF][TS]
    const long o_gam = P.offs[W_LN_G_W], o_bet = P.offs[W_LN_G_B];
    const long o_w = P.offs[W_G_W], o_b = P.offs[W_G_B];
    const float* __restrict__ gam = P.flat_p + o_gam;
    const float* __restrict__ bet = P.flat_p + o_bet;
    constexpr int UNITS = KGE * KGF;
    constexpr int MYU = (UNITS + 255) / 256;
    float acc[MYU];
#pragma unroll
    for (int q = 0; q < MYU; ++q) acc[q] = 0.f;
    // tid in [64, 64+KGE): bias sums; tid in [128, 128+KGF): LN gamma;
    // tid in [192, 192+KGF): LN beta
    float bacc = 0.f, lacc = 0.f;
    for (int r0 = 0; r0 < D.B; r0 += WFC_ST) {
      const int rt = min(WFC_ST, D.B - r0);
      {
        constexpr int CX = WFC_ST * KGF / NT;
        static_assert(WFC_ST * KGE / 4 == NT && CX * NT == WFC_ST * KGF,
                      "whole trips");
        float rXH[CX], rGU[CX], rGam[CX], rBet[CX];
        // one 16-byte load a thread: row tid / 2, half tid % 2 of gpre
        const int gx = min(tid, rt * (KGE / 4) - 1);
        const float4 rG = *reinterpret_cast<const float4*>(
            P.gfinal + (long)(r0 + gx / (KGE / 4)) * KFIN + KOUT
            + 4 * (gx % (KGE / 4)));
#pragma unroll
        for (int k = 0; k < CX; ++k) {
          const int x = min(tid + k * NT, rt * KGF - 1);
          rXH[k] = P.xh34[(long)r0 * KGF + x];
          rGU[k] = P.gu34[(long)r0 * KGF + x];
          rGam[k] = gam[x % KGF];
          rBet[k] = bet[x % KGF];
        }
        if (tid < rt * (KGE / 4)) {
          const int t = tid / (KGE / 4), c = 4 * (tid % (KGE / 4));
          tG[(c + 0) * TS + t] = rG.x;
          tG[(c + 1) * TS + t] = rG.y;
          tG[(c + 2) * TS + t] = rG.z;
          tG[(c + 3) * TS + t] = rG.w;
        }
#pragma unroll
        for (int k = 0; k < CX; ++k) {
          const int x = tid + k * NT;
          if (x < rt * KGF) {
            const int t = x / KGF, i = x % KGF;
            tU[i * TS + t] = FMA(rXH[k], rGam[k], rBet[k]);
            tXH[i * TS + t] = rXH[k];
            tGU[i * TS + t] = rGU[k];
          }
        }
      }
      __syncthreads();
      const int rt4 = rt & ~3;
#pragma unroll
      for (int q = 0; q < MYU; ++q) {
        int u = tid + q * 256;
        if (u < UNITS) {
          const float* go = tG + (u / KGF) * TS;
          const float* ui = tU + (u % KGF) * TS;
          float a = acc[q];
          if (rt == WFC_ST) {
#pragma unroll 8
            for (int t = 0; t < WFC_ST; t += 4) {
              const float4 g = LDS4(go + t), v = LDS4(ui + t);
              a = FMA(g.x, v.x, a);
              a = FMA(g.y, v.y, a);
              a = FMA(g.z, v.z, a);
              a = FMA(g.w, v.w, a);
            }
          } else {
            for (int t = 0; t < rt4; t += 4) {
              const float4 g = LDS4(go + t), v = LDS4(ui + t);
              a = FMA(g.x, v.x, a);
              a = FMA(g.y, v.y, a);
              a = FMA(g.z, v.z, a);
              a = FMA(g.w, v.w, a);
            }
            for (int t = rt4; t < rt; ++t) a = FMA(go[t], ui[t], a);
          }
          acc[q] = a;
        }
      }
      if (tid >= 64 && tid < 64 + KGE) {
        const float* go = tG + (tid - 64) * TS;
        for (int t = 0; t < rt4; t += 4) {
          const float4 g = LDS4(go + t);
          bacc = bacc + g.x;
          bacc = bacc + g.y;
          bacc = bacc + g.z;
          bacc = bacc + g.w;
        }
        for (int t = rt4; t < rt; ++t) bacc = bacc + go[t];
      }
      if (tid >= 128 && tid < 128 + KGF) {
        const float* gu = tGU + (tid - 128) * TS;
        const float* xh = tXH + (tid - 128) * TS;
        for (int t = 0; t < rt4; t += 4) {
          const float4 g = LDS4(gu + t), x = LDS4(xh + t);
          lacc = lacc + mul_rn(g.x, x.x);
          lacc = lacc + mul_rn(g.y, x.y);
          lacc = lacc + mul_rn(g.z, x.z);
          lacc = lacc + mul_rn(g.w, x.w);
        }
        for (int t = rt4; t < rt; ++t) lacc = lacc + mul_rn(gu[t], xh[t]);
      }
      if (tid >= 192 && tid < 192 + KGF) {
        const float* gu = tGU + (tid - 192) * TS;
        for (int t = 0; t < rt4; t += 4) {
          const float4 g = LDS4(gu + t);
          lacc = lacc + g.x;
          lacc = lacc + g.y;
          lacc = lacc + g.z;
          lacc = lacc + g.w;
        }
        for (int t = rt4; t < rt; ++t) lacc = lacc + gu[t];
      }
      __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < MYU; ++q) {
      int u = tid + q * 256;
      if (u < UNITS) P.flat_g[o_w + u] = acc[q];
    }
    if (tid >= 64 && tid < 64 + KGE) P.flat_g[o_b + tid - 64] = bacc;
    if (tid >= 128 && tid < 128 + KGF) P.flat_g[o_gam + tid - 128] = lacc;
    if (tid >= 192 && tid < 192 + KGF) P.flat_g[o_bet + tid - 192] = lacc;
    return;
  }

  // ---- FC-column jobs: block jb owns columns [j0, j0 + JW) of W1p/W1v
  // [FC,FIN] (+ b1p/b1v) AND of W2p [A,FC] / W2v [FC]; block 0 also sums b2p
  // and b2v.
  {
    constexpr int JW = WFC2_JW;
    constexpr int PV = JW * KFIN;       // W1p/W1v units: tid in [0, PV)
    constexpr int A2 = KA * JW;         // W2p units: tid in [A2_T0, A2_T0+A2)
    constexpr int A2_T0 = PV <= 128 ? 128 : NT - A2;
    constexpr int CS_N = 2 * JW;        // b1p, b1v column sums: tid < CS_N
    constexpr int W2V_T0 = PV;          // W2v columns: tid in [PV, PV+JW)
    constexpr int B2_T0 = NT - 32;      // jb == 0: b2p rows, then b2v
    static_assert(A2_T0 >= 0 && A2_T0 + A2 <= NT && W2V_T0 + JW <= NT
                  && KA + 1 <= 32, "roles fit the block");
    const int jb = bid - D.M - 1;
    if (jb >= WFC2_NFC) return;
    const int j0 = jb * JW;
    float* tF = lds;                                    // [KFIN][TS]
    float* tGp = tF + KFIN * TS;                        // [JW][TS]
    float* tGv = tGp + JW * TS;                         // [JW][TS], after tGp
    float* tHp = tGv + JW * TS;                         // [JW][TS]
    float* tHv = tHp + JW * TS;                         // [JW][TS]
    float* tGL = tHv + JW * TS;                         // [KA + 1][TS]; row KA
                                                        // is gvalue
    const long o_p1w = P.offs[W_P1_W], o_v1w = P.offs[W_V1_W];
    const long o_p2w = P.offs[W_P2_W], o_p1b = P.offs[W_P1_B];
    const long o_v1b = P.offs[W_V1_B], o_v2w = P.offs[W_V2_W];
    const long o_p2b = P.offs[W_P2_B], o_v2b = P.offs[W_V2_B];
    float ap = 0.f, av = 0.f, s2 = 0.f, cs = 0.f, w2v = 0.f, b2 = 0.f;
    const bool is_pv = tid < PV;
    const bool is_a2 = tid >= A2_T0 && tid < A2_T0 + A2;
    const bool is_cs = tid < CS_N;
    const bool is_w2v = tid >= W2V_T0 && tid < W2V_T0 + JW;
    const bool is_b2 = jb == 0 && tid >= B2_T0 && tid < B2_T0 + KA + 1;
    const int pj = tid / KFIN, pi = tid % KFIN;
    const int aa = (tid - A2_T0) / JW, aj = (tid - A2_T0) % JW;
    for (int s0 = 0; s0 < D.B; s0 += WFC_ST) {
      const int st = min(WFC_ST, D.B - s0);
      // all global loads of the super-tile first (clamped indices, one basic
      // block), then the transposed LDS stores
      {
        constexpr int CF = WFC_ST * KFIN / 4 / NT;      // float4 a thread
        constexpr int CL = (WFC_ST * KA + NT - 1) / NT;
        constexpr int Q = JW / 4;                       // float4 a column row
        static_assert(CF * NT * 4 == WFC_ST * KFIN && WFC_ST * Q <= NT
                      && WFC_ST <= NT, "whole trips");
        float4 rF[CF];
        float rGL[CL];
#pragma unroll
        for (int k = 0; k < CF; ++k) {
          const int x = min(tid + k * NT, st * (KFIN / 4) - 1);
          rF[k] = *reinterpret_cast<const float4*>(
              P.fin + (long)s0 * KFIN + 4 * x);
        }
        const int cx = min(tid, st * Q - 1);
        const long cg = (long)(s0 + cx / Q) * KFC + j0 + 4 * (cx % Q);
        const float4 rGp = *reinterpret_cast<const float4*>(P.gh1p + cg);
        const float4 rGv = *reinterpret_cast<const float4*>(P.gh1v + cg);
        const float4 rHp = *reinterpret_cast<const float4*>(P.h1p + cg);
        const float4 rHv = *reinterpret_cast<const float4*>(P.h1v + cg);
#pragma unroll
        for (int k = 0; k < CL; ++k) {
          const int x = min(tid + k * NT, st * KA - 1);
          rGL[k] = P.glogits[(long)s0 * KA + x];
        }
        const float rGV = P.gvalue[s0 + min(tid, st - 1)];
#pragma unroll
        for (int k = 0; k < CF; ++k) {
          const int x = tid + k * NT;
          if (x < st * (KFIN / 4)) {
            const int t = x / (KFIN / 4), c = 4 * (x % (KFIN / 4));
            tF[(c + 0) * TS + t] = rF[k].x;
            tF[(c + 1) * TS + t] = rF[k].y;
            tF[(c + 2) * TS + t] = rF[k].z;
            tF[(c + 3) * TS + t] = rF[k].w;
          }
        }
        if (tid < st * Q) {
          const int t = tid / Q, c = 4 * (tid % Q);
          tGp[(c + 0) * TS + t] = rGp.x;
          tGp[(c + 1) * TS + t] = rGp.y;
          tGp[(c + 2) * TS + t] = rGp.z;
          tGp[(c + 3) * TS + t] = rGp.w;
          tGv[(c + 0) * TS + t] = rGv.x;
          tGv[(c + 1) * TS + t] = rGv.y;
          tGv[(c + 2) * TS + t] = rGv.z;
          tGv[(c + 3) * TS + t] = rGv.w;
          tHp[(c + 0) * TS + t] = rHp.x;
          tHp[(c + 1) * TS + t] = rHp.y;
          tHp[(c + 2) * TS + t] = rHp.z;
          tHp[(c + 3) * TS + t] = rHp.w;
          tHv[(c + 0) * TS + t] = rHv.x;
          tHv[(c + 1) * TS + t] = rHv.y;
          tHv[(c + 2) * TS + t] = rHv.z;
          tHv[(c + 3) * TS + t] = rHv.w;
        }
#pragma unroll
        for (int k = 0; k < CL; ++k) {
          const int x = tid + k * NT;
          if (x < st * KA) tGL[(x % KA) * TS + x / KA] = rGL[k];
        }
        if (tid < st) tGL[KA * TS + tid] = rGV;
      }
      __syncthreads();
      const int st4 = st & ~3;
      if (is_pv) {
        // W1p / W1v unit (pj, pi): sample order, fused throughout
        const float* fr = tF + pi * TS;
        const float* gp = tGp + pj * TS;
        const float* gv = tGv + pj * TS;
        if (st == WFC_ST) {
#pragma unroll 8
          for (int t = 0; t < WFC_ST; t += 4) {
            const float4 f = LDS4(fr + t), a = LDS4(gp + t), b = LDS4(gv + t);
            ap = FMA(a.x, f.x, ap);
            av = FMA(b.x, f.x, av);
            ap = FMA(a.y, f.y, ap);
            av = FMA(b.y, f.y, av);
            ap = FMA(a.z, f.z, ap);
            av = FMA(b.z, f.z, av);
            ap = FMA(a.w, f.w, ap);
            av = FMA(b.w, f.w, av);
          }
        } else {
          for (int t = 0; t < st4; t += 4) {
            const float4 f = LDS4(fr + t), a = LDS4(gp + t), b = LDS4(gv + t);
            ap = FMA(a.x, f.x, ap);
            av = FMA(b.x, f.x, av);
            ap = FMA(a.y, f.y, ap);
            av = FMA(b.y, f.y, av);
            ap = FMA(a.z, f.z, ap);
            av = FMA(b.z, f.z, av);
            ap = FMA(a.w, f.w, ap);
            av = FMA(b.w, f.w, av);
          }
          for (int t = st4; t < st; ++t) {
            ap = FMA(gp[t], fr[t], ap);
            av = FMA(gv[t], fr[t], av);
          }
        }
      }
      if (is_a2) {
        // W2p unit (aa, aj), tile by tile as the oracle's chain saw them
        const float* gl = tGL + aa * TS;
        const float* hp = tHp + aj * TS;
        for (int r0 = 0; r0 < st; r0 += TILE_K) {
          const int rt = min(TILE_K, st - r0);
          if (rt == TILE_K) {
#pragma unroll
            for (int t = 0; t < TILE_K; t += 4) {
              const float4 g = LDS4(gl + r0 + t), h = LDS4(hp + r0 + t);
              if (t < 20) {
                s2 = FMA(g.x, h.x, s2);
                s2 = FMA(g.y, h.y, s2);
                s2 = FMA(g.z, h.z, s2);
                s2 = FMA(g.w, h.w, s2);
              } else {
                s2 = s2 + mul_rn(g.x, h.x);
                s2 = s2 + mul_rn(g.y, h.y);
                s2 = s2 + mul_rn(g.z, h.z);
                s2 = s2 + mul_rn(g.w, h.w);
              }
            }
          } else {
            for (int t = 0; t < rt; ++t)
              s2 = FMA(gl[r0 + t], hp[r0 + t], s2);
          }
        }
      }
      if (is_cs) {
        // b1p (tid < JW) and b1v column sums: rows of tGp, then of tGv
        const float* g = tGp + tid * TS;
        for (int t = 0; t < st4; t += 4) {
          const float4 v = LDS4(g + t);
          cs = cs + v.x;
          cs = cs + v.y;
          cs = cs + v.z;
          cs = cs + v.w;
        }
        for (int t = st4; t < st; ++t) cs = cs + g[t];
      }
      if (is_w2v) {
        const float* gvl = tGL + KA * TS;
        const float* hv = tHv + (tid - W2V_T0) * TS;
        for (int t = 0; t < st4; t += 4) {
          const float4 g = LDS4(gvl + t), h = LDS4(hv + t);
          w2v = FMA(g.x, h.x, w2v);
          w2v = FMA(g.y, h.y, w2v);
          w2v = FMA(g.z, h.z, w2v);
          w2v = FMA(g.w, h.w, w2v);
        }
        for (int t = st4; t < st; ++t) w2v = FMA(gvl[t], hv[t], w2v);
      }
      if (is_b2) {
        // b2p rows 0..KA-1 of glogits, b2v row KA (gvalue)
        const float* g = tGL + (tid - B2_T0) * TS;
        for (int t = 0; t < st4; t += 4) {
          const float4 v = LDS4(g + t);
          b2 = b2 + v.x;
          b2 = b2 + v.y;
          b2 = b2 + v.z;
          b2 = b2 + v.w;
        }
        for (int t = st4; t < st; ++t) b2 = b2 + g[t];
      }
      __syncthreads();
    }
    if (is_pv) {
      P.flat_g[o_p1w + (long)(j0 + pj) * KFIN + pi] = ap;
      P.flat_g[o_v1w + (long)(j0 + pj) * KFIN + pi] = av;
    }
    if (is_a2) P.flat_g[o_p2w + (long)aa * KFC + j0 + aj] = s2;
    if (is_cs) {
      if (tid < JW) P.flat_g[o_p1b + j0 + tid] = cs;
      else P.flat_g[o_v1b + j0 + tid - JW] = cs;
    }
    if (is_w2v) P.flat_g[o_v2w + j0 + tid - W2V_T0] = w2v;
    if (is_b2) {
      if (tid - B2_T0 < KA) P.flat_g[o_p2b + tid - B2_T0] = b2;
      else P.flat_g[o_v2b] = b2;
    }
  }
}

// ---- cs_stage + cs_fwd_mlp_lanes<1> ----
// Block 0 gathers the minibatch from the device batch store (the body of
// cs_stage_kernel, one workgroup, same cursor protocol and guards); blocks
// 1.. are cs_fwd_mlp_lanes_kernel<1, L>'s blocks 0.. .  No GNN forward kernel
// reads a staged buffer (cs_head_kernel is their first reader), so the two
// roles are independent and one launch of the chain goes away.
static_assert(CS_STAGE_THREADS == ROW_NT, "stage role runs a ROW_NT block");

template <int L>
__global__ void __launch_bounds__(ROW_NT)
cs_fwd_stage_mlp1_lanes_kernel(CachedPtrs P, CachedDims D, StagePtrs SP,
                               StageDims SD) {
  if (blockIdx.x == 0) {
    cs_stage_body(SP, SD);
    return;
  }
  constexpr int RPB = ROW_NT / L;
  const int blk = (int)blockIdx.x - 1;
  const int nbN = (D.N + RPB - 1) / RPB;
  if (blk < nbN) {
    const long r0 = (long)blk * RPB;
    rows_fwd_lanes<KF0, KH, 1, L>(
        P, W_LN_N1_W, r0, D.N,
        [&](long v, int i) { return P.z0[v * KF0 + i]; },
        P.xh_z1, P.rst_z1, P.hn1);
  } else {
    const long r0 = (long)(blk - nbN) * RPB;
    rows_fwd_lanes<KFE, KH, 0, L>(
        P, W_LN_E1_W, r0, D.E,
        [&](long k, int i) { return P.e[k * KFE + i]; },
        P.xh_e1, P.rst_e1, P.he1);
  }
}

// ---- cs_stage + round-1 node / edge modules + round-1 reduce module ----
// The round-1 modules are 5 -> 16 and 2 -> 16: a reduce-module block can
// compute hn1[src[k]] and he1[k] for its own message rows from z0 / e while
// it stages them, which is cheaper than a launch of its own and a
// src -> hn1 gather through memory.  Block 0 (with a device batch store) is
// the stage role; then cs_fwd_reduce_lanes_kernel<1, L>'s edge-row and
// self-row blocks.  Every tensor the two launches stored is still stored,
// once: he1 / xh_e1 / rst_e1 by the edge block that owns the edge, hn1 /
// xh_z1 / rst_z1 by the self-row block that owns the node (an edge block
// recomputes hn1[src] and does not store it).  DDLS_AMD_STEP_MERGE=off
// launches the two kernels above.

// one output element of a round-1 module row: rows_fwd_lanes<Din, KH, NF, .>'s
// operation sequence on the Din inputs at x; *xh_c is xhat[c]
template <int Din, int NF>
__device__ __forceinline__ float mod1_elem(
    const float* __restrict__ x, const float* __restrict__ gam,
    const float* __restrict__ bet, const float* __restrict__ w, float b,
    int c, float* __restrict__ xh_c, float* __restrict__ rstd_out) {
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < Din; ++i) s = s + x[i];
  const float mu = s / Din;
  float var;
  {
    const float d0 = x[0] - mu;
    var = d0 * d0;
  }
#pragma unroll
  for (int i = 1; i < Din; ++i) {
    const float d = x[i] - mu;
    if (i >= Din - NF) var = FMA(d, d, var);
    else var = var + d * d;
  }
  float rstd;
  if ((Din & (Din - 1)) == 0) rstd = rsqrtf(FMA(var, 1.f / Din, LN_EPS));
  else rstd = rsqrtf(var / Din + LN_EPS);
  *rstd_out = rstd;
  *xh_c = (x[c] - mu) * rstd;
  float acc = b;
#pragma unroll
  for (int i = 0; i < Din; ++i) {
    const float xh = (x[i] - mu) * rstd;
    acc = FMA(FMA(xh, gam[i], bet[i]), w[i], acc);
  }
  return acc > 0.f ? acc : 0.f;
}

template <int L, bool EDGE>
__device__ __forceinline__ void mlp1_red1_rows(const CachedPtrs& P, long r0,
                                               long nrows) {
  constexpr int RPB = ROW_NT / L;
  constexpr int XS = KMSG + 1;
  constexpr int RW = EDGE ? KF0 + KFE : KF0;     // staged inputs per row
  constexpr int NSM = 2 * KMSG + KHID + (2 * KF0 + KH * KF0 + KH)
                      + (EDGE ? 2 * KFE + KH * KFE + KH : 0);
  constexpr int WQ = KMSG * KHID / ROW_NT;
  static_assert(RPB * RW <= ROW_NT && NSM <= 2 * ROW_NT
                && KMSG * KHID % ROW_NT == 0, "one staging pass");
  __shared__ float sGam[KMSG], sBet[KMSG], sW[KHID * XS], sB[KHID];
  __shared__ float sX[RPB * XS], sU[RPB * XS];
  // gam | bet | W | b of the node module, then of the edge module
  __shared__ float sM1[2 * KF0 + KH * KF0 + KH + 2 * KFE + KH * KFE + KH];
  __shared__ float sIn[RPB * (KF0 + KFE)];
  float* const sGamN = sM1;
  float* const sBetN = sGamN + KF0;
  float* const sWN = sBetN + KF0;
  float* const sBN = sWN + KH * KF0;
  float* const sGamE = sBN + KH;
  float* const sBetE = sGamE + KFE;
  float* const sWE = sBetE + KFE;
  float* const sBE = sWE + KH * KFE;
  const int tid = threadIdx.x;
  // the small parameter vectors as one index space: global source and LDS
  // destination of element x
  auto small = [&](int x, const float*& src, float*& dst) {
    const int seg[12] = {KMSG, KMSG, KHID, KF0, KF0, KH * KF0, KH,
                         KFE, KFE, KH * KFE, KH, 0};
    const int slot[11] = {W_LN_R1_W, W_LN_R1_B, W_R1_B,
                          W_LN_N1_W, W_LN_N1_B, W_N1_W, W_N1_B,
                          W_LN_E1_W, W_LN_E1_B, W_E1_W, W_E1_B};
    float* const lds[11] = {sGam, sBet, sB, sGamN, sBetN, sWN, sBN,
                            sGamE, sBetE, sWE, sBE};
    src = nullptr;
    dst = nullptr;
#pragma unroll
    for (int q = 0; q < 11; ++q) {
      if (x >= 0 && x < seg[q]) {
        src = WP(slot[q]) + x;
        dst = lds[q] + x;
      }
      x -= seg[q];
    }
  };
  // every global load of the thread before its first LDS store
  float wr[WQ];
  {
    const float* __restrict__ gW = WP(W_R1_W);
#pragma unroll
    for (int q = 0; q < WQ; ++q) wr[q] = gW[tid + q * ROW_NT];
  }
  const float* sm_src[2];
  float* sm_dst[2];
  float sm_val[2];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int x = tid + q * ROW_NT;
    small(x < NSM ? x : -1, sm_src[q], sm_dst[q]);
    sm_val[q] = sm_src[q] != nullptr ? *sm_src[q] : 0.f;
  }
  float in_val = 0.f;
  if (tid < RPB * RW) {
    const int r = tid / RW, c = tid % RW;
    const long row = r0 + r;
    if (row < nrows) {
      if (EDGE)
        in_val = c < KF0 ? P.z0[P.src[row] * KF0 + c]
                         : P.e[row * KFE + (c - KF0)];
      else
        in_val = P.z0[row * KF0 + c];
    }
  }
#pragma unroll
  for (int q = 0; q < WQ; ++q) {
    const int x = tid + q * ROW_NT;
    sW[(x / KMSG) * XS + x % KMSG] = wr[q];
  }
#pragma unroll
  for (int q = 0; q < 2; ++q)
    if (sm_dst[q] != nullptr) *sm_dst[q] = sm_val[q];
  if (tid < RPB * RW)
    sIn[(tid / RW) * (KF0 + KFE) + tid % RW] = in_val;
  __syncthreads();
  // the message rows: one thread per element, node-module elements first so
  // that a wave runs one module
  constexpr int NEL = RPB * KH;
  for (int x = tid; x < (EDGE ? 2 : 1) * NEL; x += ROW_NT) {
    const bool node = x < NEL;
    const int y = node ? x : x - NEL;
    const int r = y / KH, j = y % KH;
    const long row = r0 + r;
    const bool live = row < nrows;
    const float* __restrict__ in = sIn + r * (KF0 + KFE);
    float val, xh, rstd;
    if (node) {
      const int c = j < KF0 ? j : 0;
      val = mod1_elem<KF0, 1>(in, sGamN, sBetN, sWN + j * KF0, sBN[j], c, &xh,
                              &rstd);
      if (!EDGE && live) {
        P.hn1[row * KH + j] = val;
        if (j < KF0) P.xh_z1[row * KF0 + j] = xh;
        if (j == 0) P.rst_z1[row] = rstd;
      }
      sX[r * XS + j] = live ? val : 0.f;
      if (!EDGE) sX[r * XS + KH + j] = 0.f;
    } else {
      const int c = j < KFE ? j : 0;
      val = mod1_elem<KFE, 0>(in + KF0, sGamE, sBetE, sWE + j * KFE, sBE[j],
                              c, &xh, &rstd);
      if (live) {
        P.he1[row * KH + j] = val;
        if (j < KFE) P.xh_e1[row * KFE + j] = xh;
        if (j == 0) P.rst_e1[row] = rstd;
      }
      sX[r * XS + KH + j] = live ? val : 0.f;
    }
  }
  __syncthreads();
  // from here rows_fwd_lanes<KMSG, KHID, EDGE ? 0 : KH, L>'s body
  constexpr int NF = EDGE ? 0 : KH;
  float* __restrict__ xhat_out = EDGE ? P.xh_m1e : P.xh_m1s;
  float* __restrict__ rstd_out = EDGE ? P.rst_m1e : P.rst_m1s;
  float* __restrict__ out = EDGE ? P.re1 : P.rs1;
  const int g = tid / L, l = tid % L;
  const long row = r0 + g;
  const bool live = row < nrows;
  const float* __restrict__ x = sX + g * XS;
  float s = 0.f;
#pragma unroll 8
  for (int i = 0; i < KMSG; ++i) s = s + x[i];
  const float mu = s / KMSG;
  float var;
  {
    const float d0 = x[0] - mu;
    var = d0 * d0;
  }
#pragma unroll 8
  for (int i = 1; i < KMSG; ++i) {
    const float d = x[i] - mu;
    if (i >= KMSG - NF) var = FMA(d, d, var);
    else var = var + d * d;
  }
  const float rstd = rsqrtf(FMA(var, 1.f / KMSG, LN_EPS));
  for (int i = l; i < KMSG; i += L) {
    const float xh = (x[i] - mu) * rstd;
    if (live) xhat_out[row * KMSG + i] = xh;
    sU[g * XS + i] = FMA(xh, sGam[i], sBet[i]);
  }
  if (live && l == 0) rstd_out[row] = rstd;
  __syncthreads();
  const float* __restrict__ u = sU + g * XS;
  for (int o = l; o < KHID; o += L) {
    const float* __restrict__ w = sW + o * XS;
    float acc = sB[o];
#pragma unroll 8
    for (int i = 0; i < KMSG; ++i) acc = FMA(u[i], w[i], acc);
    if (live) out[row * KHID + o] = acc > 0.f ? acc : 0.f;
  }
}

template <int L>
__global__ void __launch_bounds__(ROW_NT)
cs_fwd_stage_mlp1_red1_lanes_kernel(CachedPtrs P, CachedDims D, StagePtrs SP,
                                    StageDims SD, int stage) {
  if (stage && blockIdx.x == 0) {
    cs_stage_body(SP, SD);
    return;
  }
  constexpr int RPB = ROW_NT / L;
  const int blk = (int)blockIdx.x - stage;
  const int nbE = (D.E + RPB - 1) / RPB;
  if (blk < nbE)
    mlp1_red1_rows<L, true>(P, (long)blk * RPB, D.E);
  else
    mlp1_red1_rows<L, false>(P, (long)(blk - nbE) * RPB, D.N);
}

// ---- cs_bwd_scat1_gu1 + the row jobs of cs_bwd_w ----
// ghn1 / ghe1 / gu_z1 / gu_e1 are row-local functions of gms1 / gme1, which
// cs_bwd_reduce_lanes<1> wrote one launch earlier, and only the N1 and E1
// weight-grad jobs read them: those jobs recompute them per 32-row tile while
// staging it, so the scatter launch and the weight-grad launch need no
// grid-wide dependency between them and run as one.  Blocks [0, sg_b) are
// cs_bwd_scat1_gu1_kernel's (they keep storing the four tensors and C_STATS),
// then the 6 x WSPLIT row-job blocks; R1, R2, N2 and E2 run wgrad_tiled's
// loops with the roundings written out (wgrad_tiled_x).
//
// wgrad_tiled sits above the contraction pragma; its roundings in
// cs_bwd_w_kernel's gfx950 ISA (docs/KERNELS.md "Round 8") are the same in
// all six row jobs:
//   tU = xh*gam+bet   one FMA
//   unit chain        full 32-row tile: terms 0-19 fused, 20-31 rounded
//                     products; partial tile: every term fused; the
//                     accumulator runs on through a split's tiles
//   bias sum          plain adds
//   LN gamma sum      gu*xh rounded, then added; LN beta sum plain adds
template <int Din, int Dout>
__device__ __forceinline__ void wgrad_tiled_x(
    const CachedPtrs& P, int tid, int rows0, int rows1,
    const float* __restrict__ gpre0, const float* __restrict__ gpre1,
    const float* __restrict__ xh0, const float* __restrict__ xh1,
    const float* __restrict__ gu0, const float* __restrict__ gu1,
    int w_slot, float (*tG)[65], float (*tU)[65], float (*tGU)[65],
    float (*tXH)[65], int split, float* __restrict__ pout) {
  const float* __restrict__ gam = WP(w_slot);
  const float* __restrict__ bet = WP(w_slot + 1);
  constexpr int UNITS = Din * Dout;
  constexpr int MYU = (UNITS + ROW_NT - 1) / ROW_NT;
  float acc[MYU];
#pragma unroll
  for (int q = 0; q < MYU; ++q) acc[q] = 0.f;
  float bacc = 0.f, lacc_w = 0.f, lacc_b = 0.f;
  const int rows = rows0 + rows1;
  for (int r0 = split * TILE_K; r0 < rows; r0 += WSPLIT * TILE_K) {
    const int rt = min(TILE_K, rows - r0);
    for (int x = tid; x < rt * Dout; x += ROW_NT) {
      const int t = x / Dout, o = x % Dout;
      const int r = r0 + t;
      tG[t][o] = (r < rows0) ? gpre0[(long)r * Dout + o]
                             : gpre1[(long)(r - rows0) * Dout + o];
    }
    for (int x = tid; x < rt * Din; x += ROW_NT) {
      const int t = x / Din, i = x % Din;
      const int r = r0 + t;
      const float xh = (r < rows0) ? xh0[(long)r * Din + i]
                                   : xh1[(long)(r - rows0) * Din + i];
      tU[t][i] = FMA(xh, gam[i], bet[i]);
      tXH[t][i] = xh;
      tGU[t][i] = (r < rows0) ? gu0[(long)r * Din + i]
                              : gu1[(long)(r - rows0) * Din + i];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < MYU; ++q) {
      const int u = tid + q * ROW_NT;
      if (u < UNITS) {
        const int o = u / Din, i = u % Din;
        float a = acc[q];
        if (rt == TILE_K) {
#pragma unroll
          for (int t = 0; t < 20; ++t) a = FMA(tG[t][o], tU[t][i], a);
#pragma unroll
          for (int t = 20; t < TILE_K; ++t) a = a + tG[t][o] * tU[t][i];
        } else {
          for (int t = 0; t < rt; ++t) a = FMA(tG[t][o], tU[t][i], a);
        }
        acc[q] = a;
      }
    }
    if (tid < Dout)
      for (int t = 0; t < rt; ++t) bacc = bacc + tG[t][tid];
    if (tid < Din)
      for (int t = 0; t < rt; ++t) {
        lacc_w = lacc_w + tGU[t][tid] * tXH[t][tid];
        lacc_b = lacc_b + tGU[t][tid];
      }
    __syncthreads();
  }
  // partial layout: [w UNITS][b Dout][ln_w Din][ln_b Din]
#pragma unroll
  for (int q = 0; q < MYU; ++q) {
    const int u = tid + q * ROW_NT;
    if (u < UNITS) pout[u] = acc[q];
  }
  if (tid < Dout) pout[UNITS + tid] = bacc;
  if (tid < Din) {
    pout[UNITS + Dout + tid] = lacc_w;
    pout[UNITS + Dout + Din + tid] = lacc_b;
  }
}

// the N1 / E1 jobs: wgrad_tiled_x with tG and tGU recomputed from gms1 / gme1
template <int Din, bool NODE>
__device__ __forceinline__ void wgrad_m1_tiled(
    const CachedPtrs& P, int tid, int rows, int w_slot, float (*tG)[65],
    float (*tU)[65], float (*tGU)[65], float (*tXH)[65], int split,
    float* __restrict__ pout) {
  constexpr int Dout = KH;
  constexpr int UNITS = Din * Dout;
  static_assert(UNITS <= ROW_NT, "one unit per thread");
  __shared__ float sWm[KH * Din];
  const float* __restrict__ gam = WP(w_slot);
  const float* __restrict__ bet = WP(w_slot + 1);
  const float* __restrict__ xhp = NODE ? P.xh_z1 : P.xh_e1;
  for (int x = tid; x < KH * Din; x += ROW_NT) sWm[x] = WP(w_slot + 2)[x];
  float acc = 0.f, bacc = 0.f, lacc_w = 0.f, lacc_b = 0.f;
  for (int r0 = split * TILE_K; r0 < rows; r0 += WSPLIT * TILE_K) {
    const int rt = min(TILE_K, rows - r0);
    // tG: cs_bwd_scat1_gu1_kernel's scatter of the tile's rows
    for (int x = tid; x < rt * Dout; x += ROW_NT) {
      const int t = x / Dout, o = x % Dout;
      const long r = r0 + t;
      float g;
      if (NODE) {
        const long lo = P.src_indptr[r], hi = P.src_indptr[r + 1];
        float a = P.gms1[r * KMSG + o];
        for (long q = lo; q < hi; ++q)
          a = a + P.gme1[P.src_order[q] * KMSG + o];
        g = P.hn1[r * KH + o] > 0.f ? a : 0.f;
      } else {
        const float ge = P.gme1[r * KMSG + KH + o];
        g = P.he1[r * KH + o] > 0.f ? ge : 0.f;
      }
      tG[t][o] = g;
    }
    for (int x = tid; x < rt * Din; x += ROW_NT) {
      const int t = x / Din, i = x % Din;
      const float xh = xhp[(long)(r0 + t) * Din + i];
      tU[t][i] = FMA(xh, gam[i], bet[i]);
      tXH[t][i] = xh;
    }
    __syncthreads();
    // tGU: the 16-term chain from 0, all fused
    for (int x = tid; x < rt * Din; x += ROW_NT) {
      const int t = x / Din, i = x % Din;
      float a = 0.f;
#pragma unroll
      for (int o = 0; o < KH; ++o) a = FMA(sWm[o * Din + i], tG[t][o], a);
      tGU[t][i] = a;
    }
    __syncthreads();
    if (tid < UNITS) {
      const int o = tid / Din, i = tid % Din;
      float a = acc;
      if (rt == TILE_K) {
#pragma unroll
        for (int t = 0; t < 20; ++t) a = FMA(tG[t][o], tU[t][i], a);
#pragma unroll
        for (int t = 20; t < TILE_K; ++t) a = a + tG[t][o] * tU[t][i];
      } else {
        for (int t = 0; t < rt; ++t) a = FMA(tG[t][o], tU[t][i], a);
      }
      acc = a;
    }
    if (tid < Dout)
      for (int t = 0; t < rt; ++t) bacc = bacc + tG[t][tid];
    if (tid < Din)
      for (int t = 0; t < rt; ++t) {
        lacc_w = lacc_w + tGU[t][tid] * tXH[t][tid];
        lacc_b = lacc_b + tGU[t][tid];
      }
    __syncthreads();
  }
  // partial layout: [w UNITS][b Dout][ln_w Din][ln_b Din]
  if (tid < UNITS) pout[tid] = acc;
  if (tid < Dout) pout[UNITS + tid] = bacc;
  if (tid < Din) {
    pout[UNITS + Dout + tid] = lacc_w;
    pout[UNITS + Dout + Din + tid] = lacc_b;
  }
}

__global__ void __launch_bounds__(ROW_NT)
cs_bwd_scat1_gu1_w_kernel(CachedPtrs P, CachedDims D) {
  const int tid = threadIdx.x;
  const int nbN = (D.N + SG_RPB - 1) / SG_RPB;
  const int nbE = (D.E + SG_RPB - 1) / SG_RPB;
  const int sg_b = nbN + nbE + 1;
  if ((int)blockIdx.x >= sg_b) {
    __shared__ float tG[TILE_K][65];
    __shared__ float tU[TILE_K][65];
    __shared__ float tGU[TILE_K][65];
    __shared__ float tXH[TILE_K][65];
    const int blk = (int)blockIdx.x - sg_b;
    const int job = blk / WSPLIT;
    const int sp = blk % WSPLIT;
    float* pout = P.wg_scratch + ((long)job * WSPLIT + sp) * WG_JSTRIDE;
    switch (job) {
      case 0:  // node module 1
        wgrad_m1_tiled<KF0, true>(P, tid, D.N, W_LN_N1_W, tG, tU, tGU, tXH,
                                  sp, pout);
        return;
      case 1:  // edge module 1
        wgrad_m1_tiled<KFE, false>(P, tid, D.E, W_LN_E1_W, tG, tU, tGU, tXH,
                                   sp, pout);
        return;
      case 2:  // reduce module 1 (edge ++ self rows)
        wgrad_tiled_x<KMSG, KHID>(P, tid, D.E, D.N, P.gpre1_e, P.gpre1_s,
                                  P.xh_m1e, P.xh_m1s, P.gu_m1e, P.gu_m1s,
                                  W_LN_R1_W, tG, tU, tGU, tXH, sp, pout);
        return;
      case 3:  // node module 2
        wgrad_tiled_x<KHID, KH>(P, tid, D.N, 0, P.gpn1, nullptr, P.xh_h2,
                                nullptr, P.gu_h2, nullptr, W_LN_N2_W, tG, tU,
                                tGU, tXH, sp, pout);
        return;
      case 4:  // edge module 2
        wgrad_tiled_x<KFE, KH>(P, tid, D.E, 0, P.gpe1, nullptr, P.xh_e2,
                               nullptr, P.gu_e2, nullptr, W_LN_E2_W, tG, tU,
                               tGU, tXH, sp, pout);
        return;
      default:  // 5: reduce module 2
        wgrad_tiled_x<KMSG, KOUT>(P, tid, D.E, D.N, P.gpe2, P.gpn2,
                                  P.xh_m2e, P.xh_m2s, P.gu_m2e, P.gu_m2s,
                                  W_LN_R2_W, tG, tU, tGU, tXH, sp, pout);
        return;
    }
  }
  // cs_bwd_scat1_gu1_kernel's blocks, unchanged
  __shared__ float sWN[KH * KF0], sWE[KH * KFE];
  __shared__ float sG[SG_RPB][KH + 1];
  for (int x = tid; x < KH * KF0; x += ROW_NT) sWN[x] = WP(W_N1_W)[x];
  for (int x = tid; x < KH * KFE; x += ROW_NT) sWE[x] = WP(W_E1_W)[x];
  const int r = tid / KH, i = tid % KH;
  if ((int)blockIdx.x >= nbN + nbE) {
    __shared__ float sT[SG_MAXB][4];
    __shared__ float sAcc[SG_MAXB / SG_SPB][4];
    for (int b = tid; b < D.B; b += ROW_NT) {
      const float logp_a = P.lp[(long)b * KA + P.actions[b]];
      const float old_lp = P.old_logp[b];
      const float ratio = __expf(logp_a - old_lp);
      const float A_b = P.adv[b];
      const float r_cl = fminf(fmaxf(ratio, 1.f - D.clip), 1.f + D.clip);
      const float surr1 = ratio * A_b, surr2 = r_cl * A_b;
      const float verr = P.values[b] - P.vtarg[b];
      sT[b][0] = -fminf(surr1, surr2);
      sT[b][1] = fminf(verr * verr, D.vf_clip);
      sT[b][2] = old_lp - logp_a;
      sT[b][3] = P.hent[b];
    }
    __syncthreads();
    const int ng = (D.B + SG_SPB - 1) / SG_SPB;
    for (int x = tid; x < ng * 4; x += ROW_NT) {
      const int g = x / 4, k = x % 4;
      const int b_lo = g * SG_SPB;
      const int nb = min(D.B - b_lo, SG_SPB);
      float acc = sT[b_lo][k];
      for (int t = 1; t < nb; ++t) acc = acc + sT[b_lo + t][k];
      sAcc[g][k] = acc;
    }
    __syncthreads();
    if (tid == 0) {
      const float inv = 1.f / D.B;
      const float klc = P.kl[0];
      for (int g = 0; g < ng; ++g) {
        const float pl = sAcc[g][0] * inv;
        const float vf = sAcc[g][1] * inv;
        const float kl = sAcc[g][2] * inv;
        const float ent = sAcc[g][3] * inv;
        atomicAdd(&P.stats[0], pl);
        atomicAdd(&P.stats[1], vf);
        atomicAdd(&P.stats[2], kl);
        atomicAdd(&P.stats[3], ent);
        atomicAdd(&P.stats[4],
                  FMA(-D.ent_coef, ent, FMA(D.vf_coef, vf, FMA(kl, klc, pl))));
      }
    }
  } else if ((int)blockIdx.x < nbN) {
    const long r0 = (long)blockIdx.x * SG_RPB;
    const long v = r0 + r;
    float g = 0.f;
    if (v < D.N) {
      const long lo = P.src_indptr[v], hi = P.src_indptr[v + 1];
      float acc = P.gms1[v * KMSG + i];
      for (long q = lo; q < hi; ++q)
        acc = acc + P.gme1[P.src_order[q] * KMSG + i];
      g = P.hn1[v * KH + i] > 0.f ? acc : 0.f;
      P.ghn1[v * KH + i] = g;
    }
    sG[r][i] = g;
    __syncthreads();
    for (int x = tid; x < SG_RPB * KF0; x += ROW_NT) {
      const int rr = x / KF0, ii = x % KF0;
      if (r0 + rr < D.N) {
        float acc = 0.f;
#pragma unroll
        for (int o = 0; o < KH; ++o)
          acc = FMA(sWN[o * KF0 + ii], sG[rr][o], acc);
        P.gu_z1[(r0 + rr) * KF0 + ii] = acc;
      }
    }
  } else {
    const long r0 = (long)(blockIdx.x - nbN) * SG_RPB;
    const long k = r0 + r;
    float g = 0.f;
    if (k < D.E) {
      const float ge = P.gme1[k * KMSG + KH + i];
      g = P.he1[k * KH + i] > 0.f ? ge : 0.f;
      P.ghe1[k * KH + i] = g;
    }
    sG[r][i] = g;
    __syncthreads();
    for (int x = tid; x < SG_RPB * KFE; x += ROW_NT) {
      const int rr = x / KFE, ii = x % KFE;
      if (r0 + rr < D.E) {
        float acc = 0.f;
#pragma unroll
        for (int o = 0; o < KH; ++o)
          acc = FMA(sWE[o * KFE + ii], sG[rr][o], acc);
        P.gu_e1[(r0 + rr) * KFE + ii] = acc;
      }
    }
  }
}

// ===========================================================================
// host bindings
// ===========================================================================

// Row-kernel selection, read per call like DDLS_AMD_WGRAD_MFMA:
//   DDLS_AMD_ROW_KERNELS=thread  the thread-per-row kernels (oracle / A/B)
//   DDLS_AMD_ROW_LANES=8|16|32   lanes per row for ALL lane-parallel kernels
//                                (measurement switch).  Unset: each launch's
//                                own default, the best of the three as
//                                measured on MI355X at the benchmark's 417
//                                rows (docs/KERNELS.md "Round 5"): 32 for the
//                                two 32x64 reduce-module-1 kernels, else 16.
//   DDLS_AMD_STEP_FUSION=off     the separate kernels of every fused launch
//                                (oracle / A/B); 'thread' above implies it
//   DDLS_AMD_STEP_OVERLAP=off    cs_stage, cs_bwd_pool and the B-row blocks
//                                of cs_bwd_w as launches / blocks of their
//                                own (oracle / A/B); STEP_FUSION=off and
//                                'thread' imply it
//   DDLS_AMD_STEP_MERGE=off      cs_fwd_stage_mlp1_lanes + cs_fwd_reduce_lanes<1>
//                                and cs_bwd_scat1_gu1 + cs_bwd_w as two
//                                launches each, and cs_bwd_w_reduce always
//                                launched by cached_step_bwd (oracle / A/B);
//                                STEP_OVERLAP=off, STEP_FUSION=off and
//                                'thread' imply it
//   DDLS_AMD_STEP_HEAD=off       cs_head and cs_bwd_pool_wfc in place of
//                                cs_head2 and cs_bwd_pool_wfc2 (oracle /
//                                A/B); STEP_MERGE=off and whatever implies it
//                                imply this too.  The new kernels do not
//                                depend on DDLS_AMD_WGRAD_MFMA and stay the
//                                default with it.
struct RowCfg {
  bool thread;
  int lanes;   // 0: per-kernel default
  bool fused;  // the fused launches (needs the lane-parallel row kernels)
  bool overlap;  // independent work rides in launches that exist anyway
                 // (needs the fused launches)
  bool merge;    // launches merged along row-local dependencies (needs
                 // overlap)
  bool head;     // cs_head2 / cs_bwd_pool_wfc2 (needs merge)
};

static RowCfg row_cfg() {
  RowCfg c;
  const char* rk = getenv("DDLS_AMD_ROW_KERNELS");
  c.thread = (rk != nullptr && strcmp(rk, "thread") == 0);
  TORCH_CHECK(rk == nullptr || rk[0] == '\0' || c.thread
              || strcmp(rk, "lanes") == 0,
              "cached_step: DDLS_AMD_ROW_KERNELS must be 'thread' or "
              "'lanes', got '", rk, "'");
  c.lanes = 0;
  const char* rl = getenv("DDLS_AMD_ROW_LANES");
  if (rl != nullptr && rl[0] != '\0') {
    c.lanes = atoi(rl);
    TORCH_CHECK(c.lanes == 8 || c.lanes == 16 || c.lanes == 32,
                "cached_step: DDLS_AMD_ROW_LANES must be 8, 16 or 32, got '",
                rl, "'");
  }
  const char* sf = getenv("DDLS_AMD_STEP_FUSION");
  const bool off = (sf != nullptr && strcmp(sf, "off") == 0);
  TORCH_CHECK(sf == nullptr || sf[0] == '\0' || off || strcmp(sf, "on") == 0,
              "cached_step: DDLS_AMD_STEP_FUSION must be 'on' or 'off', got '",
              sf, "'");
  c.fused = !off && !c.thread;
  const char* so = getenv("DDLS_AMD_STEP_OVERLAP");
  const bool ooff = (so != nullptr && strcmp(so, "off") == 0);
  TORCH_CHECK(so == nullptr || so[0] == '\0' || ooff || strcmp(so, "on") == 0,
              "cached_step: DDLS_AMD_STEP_OVERLAP must be 'on' or 'off', got '",
              so, "'");
  c.overlap = !ooff && c.fused;
  const char* sm = getenv("DDLS_AMD_STEP_MERGE");
  const bool moff = (sm != nullptr && strcmp(sm, "off") == 0);
  TORCH_CHECK(sm == nullptr || sm[0] == '\0' || moff || strcmp(sm, "on") == 0,
              "cached_step: DDLS_AMD_STEP_MERGE must be 'on' or 'off', got '",
              sm, "'");
  c.merge = !moff && c.overlap;
  const char* sh = getenv("DDLS_AMD_STEP_HEAD");
  const bool hoff = (sh != nullptr && strcmp(sh, "off") == 0);
  TORCH_CHECK(sh == nullptr || sh[0] == '\0' || hoff || strcmp(sh, "on") == 0,
              "cached_step: DDLS_AMD_STEP_HEAD must be 'on' or 'off', got '",
              sh, "'");
  c.head = !hoff && c.merge;
  return c;
}

// launch KERNEL<..., L> for the configured group size (DEFL when not
// configured) over the two row classes' blocks
#define LAUNCH_ROWS(KERNEL_L, DEFL, rows0, rows1)                            \
  do {                                                                       \
    const int L_ = R.lanes ? R.lanes : (DEFL);                               \
    const int rpb_ = ROW_NT / L_;                                            \
    const int nb_ = ((rows0) + rpb_ - 1) / rpb_ + ((rows1) + rpb_ - 1) / rpb_; \
    if (nb_ > 0) {                                                           \
      if (L_ == 8)                                                           \
        hipLaunchKernelGGL(KERNEL_L(8), dim3(nb_), dim3(ROW_NT), 0, stream,  \
                           P, D);                                            \
      else if (L_ == 16)                                                     \
        hipLaunchKernelGGL(KERNEL_L(16), dim3(nb_), dim3(ROW_NT), 0, stream, \
                           P, D);                                            \
      else                                                                   \
        hipLaunchKernelGGL(KERNEL_L(32), dim3(nb_), dim3(ROW_NT), 0, stream, \
                           P, D);                                            \
    }                                                                        \
  } while (0)
#define K_FWD_MLP1(L) (cs_fwd_mlp_lanes_kernel<1, L>)
#define K_FWD_MLP2(L) (cs_fwd_mlp_lanes_kernel<2, L>)
#define K_FWD_RED1(L) (cs_fwd_reduce_lanes_kernel<1, L>)
#define K_FWD_RED2(L) (cs_fwd_reduce_lanes_kernel<2, L>)
#define K_BWD_RED1(L) (cs_bwd_reduce_lanes_kernel<1, L>)
#define K_BWD_RED2(L) (cs_bwd_reduce_lanes_kernel<2, L>)
#define K_BWD_MLP2(L) (cs_bwd_mlp2_lanes_kernel<L>)
#define K_FWD_COMB1_MLP2(L) (cs_fwd_comb1_mlp2_lanes_kernel<L>)
#define K_BWD_SCAT2_MLP2(L) (cs_bwd_scat2_mlp2_lanes_kernel<L>)

static void fill_ptrs(CachedPtrs& P, CachedDims& D, RowCfg& R,
                      std::vector<torch::Tensor>& T,
                      std::vector<double>& fs) {
  TORCH_CHECK((int)T.size() == C_NT, "cached_step: tensor list size ",
              T.size(), " != ", (int)C_NT);
  D.N = (int)T[C_Z0].size(0);
  D.F0 = (int)T[C_Z0].size(1);
  D.E = (int)T[C_E].size(0);
  D.FE = (int)T[C_E].size(1);
  D.M = (int)T[C_MODEL_NPTR].size(0) - 1;
  D.B = (int)T[C_GF].size(0);
  D.GFin = (int)T[C_GF].size(1);
  D.A = (int)T[C_MASK].size(1);
  D.H = (int)T[C_HN1].size(1);
  D.MSG = 2 * D.H;
  D.HID = (int)T[C_H1].size(1);
  D.OUT = (int)T[C_H2].size(1);
  D.GEMB = (int)T[C_FINAL].size(1) - D.OUT;
  D.FIN = (int)T[C_FINAL].size(1);
  D.FC = (int)T[C_H1P].size(1);
  const char* wm = getenv("DDLS_AMD_WGRAD_MFMA");
  D.wgrad_mfma = (wm != nullptr && wm[0] == '1') ? 1 : 0;
  R = row_cfg();
  D.clip = (float)fs[0];
  D.vf_clip = (float)fs[1];
  D.vf_coef = (float)fs[2];
  D.ent_coef = (float)fs[3];
  TORCH_CHECK(D.F0 == KF0 && D.FE == KFE && D.H == KH && D.MSG == KMSG
              && D.HID == KHID && D.OUT == KOUT && D.GFin == KGF
              && D.GEMB == KGE && D.FIN == KFIN && D.FC == KFC && D.A == KA,
              "cached_step: compiled for the tuned PAC-ML dims only");
  P.z0 = T[C_Z0].data_ptr<float>();
  P.e = T[C_E].data_ptr<float>();
  P.src = T[C_SRC].data_ptr<long>();
  P.dst = T[C_DST].data_ptr<long>();
  P.order = T[C_ORDER].data_ptr<long>();
  P.indptr = T[C_INDPTR].data_ptr<long>();
  P.src_order = T[C_SRC_ORDER].data_ptr<long>();
  P.src_indptr = T[C_SRC_INDPTR].data_ptr<long>();
  P.node_model = T[C_NODE_MODEL].data_ptr<long>();
  P.model_nptr = T[C_MODEL_NPTR].data_ptr<long>();
  P.model_ids = T[C_MODEL_IDS].data_ptr<long>();
  P.gf = T[C_GF].data_ptr<float>();
  P.mask = T[C_MASK].data_ptr<float>();
  P.actions = T[C_ACTIONS].data_ptr<long>();
  P.old_logp = T[C_OLD_LOGP].data_ptr<float>();
  P.adv = T[C_ADV].data_ptr<float>();
  P.vtarg = T[C_VTARG].data_ptr<float>();
  P.kl = T[C_KL].data_ptr<float>();
  P.flat_p = T[C_FLAT_P].data_ptr<float>();
  P.flat_g = T[C_FLAT_G].data_ptr<float>();
  P.offs = T[C_OFFS].data_ptr<long>();
  P.hn1 = T[C_HN1].data_ptr<float>();
  P.he1 = T[C_HE1].data_ptr<float>();
  P.re1 = T[C_RE1].data_ptr<float>();
  P.rs1 = T[C_RS1].data_ptr<float>();
  P.h1 = T[C_H1].data_ptr<float>();
  P.hn2 = T[C_HN2].data_ptr<float>();
  P.he2 = T[C_HE2].data_ptr<float>();
  P.re2 = T[C_RE2].data_ptr<float>();
  P.rs2 = T[C_RS2].data_ptr<float>();
  P.h2 = T[C_H2].data_ptr<float>();
  P.pooled = T[C_POOLED].data_ptr<float>();
  P.xh_z1 = T[C_XH_Z1].data_ptr<float>();
  P.xh_e1 = T[C_XH_E1].data_ptr<float>();
  P.xh_m1e = T[C_XH_M1E].data_ptr<float>();
  P.xh_m1s = T[C_XH_M1S].data_ptr<float>();
  P.rst_z1 = T[C_RST_Z1].data_ptr<float>();
  P.rst_e1 = T[C_RST_E1].data_ptr<float>();
  P.rst_m1e = T[C_RST_M1E].data_ptr<float>();
  P.rst_m1s = T[C_RST_M1S].data_ptr<float>();
  P.xh_h2 = T[C_XH_H2].data_ptr<float>();
  P.xh_e2 = T[C_XH_E2].data_ptr<float>();
  P.xh_m2e = T[C_XH_M2E].data_ptr<float>();
  P.xh_m2s = T[C_XH_M2S].data_ptr<float>();
  P.rst_h2 = T[C_RST_H2].data_ptr<float>();
  P.rst_e2 = T[C_RST_E2].data_ptr<float>();
  P.rst_m2e = T[C_RST_M2E].data_ptr<float>();
  P.rst_m2s = T[C_RST_M2S].data_ptr<float>();
  P.xh34 = T[C_XH34].data_ptr<float>();
  P.fin = T[C_FINAL].data_ptr<float>();
  P.h1p = T[C_H1P].data_ptr<float>();
  P.h1v = T[C_H1V].data_ptr<float>();
  P.values = T[C_VALUES].data_ptr<float>();
  P.p = T[C_P].data_ptr<float>();
  P.lp = T[C_LP].data_ptr<float>();
  P.coef = T[C_COEF].data_ptr<float>();
  P.hent = T[C_HENT].data_ptr<float>();
  P.stats = T[C_STATS].data_ptr<float>();
  P.glogits = T[C_GLOGITS].data_ptr<float>();
  P.gvalue = T[C_GVALUE].data_ptr<float>();
  P.gh1p = T[C_GH1P].data_ptr<float>();
  P.gh1v = T[C_GH1V].data_ptr<float>();
  P.gfinal = T[C_GFINAL].data_ptr<float>();
  P.gu34 = T[C_GU34].data_ptr<float>();
  P.gpool = T[C_GPOOL].data_ptr<float>();
  P.gh2 = T[C_GH2].data_ptr<float>();
  P.gme2 = T[C_GME2].data_ptr<float>();
  P.gms2 = T[C_GMS2].data_ptr<float>();
  P.ghn2 = T[C_GHN2].data_ptr<float>();
  P.ghe2 = T[C_GHE2].data_ptr<float>();
  P.gh1b = T[C_GH1B].data_ptr<float>();
  P.gme1 = T[C_GME1].data_ptr<float>();
  P.gms1 = T[C_GMS1].data_ptr<float>();
  P.ghn1 = T[C_GHN1].data_ptr<float>();
  P.ghe1 = T[C_GHE1].data_ptr<float>();
  P.gpn2 = T[C_GPN2].data_ptr<float>();
  P.gpe2 = T[C_GPE2].data_ptr<float>();
  P.gpn1 = T[C_GPN1].data_ptr<float>();
  P.gpe1 = T[C_GPE1].data_ptr<float>();
  P.gpre1_e = T[C_GPRE1E].data_ptr<float>();
  P.gpre1_s = T[C_GPRE1S].data_ptr<float>();
  P.gu_m2e = T[C_GU_M2E].data_ptr<float>();
  P.gu_m2s = T[C_GU_M2S].data_ptr<float>();
  P.gu_h2 = T[C_GU_H2].data_ptr<float>();
  P.gu_e2 = T[C_GU_E2].data_ptr<float>();
  P.gu_m1e = T[C_GU_M1E].data_ptr<float>();
  P.gu_m1s = T[C_GU_M1S].data_ptr<float>();
  P.gu_z1 = T[C_GU_Z1].data_ptr<float>();
  P.gu_e1 = T[C_GU_E1].data_ptr<float>();
  P.wg_scratch = T[C_WG_SCRATCH].data_ptr<float>();
  TORCH_CHECK(T[C_WG_SCRATCH].numel() >= (long)6 * WSPLIT * WG_JSTRIDE,
              "cached_step: wg_scratch too small");
}

// the forward launches; with SP/SD (cached_step_fwd_staged, overlap mode) the
// first one carries the stage role in its block 0
static void step_fwd_launches(const CachedPtrs& P, const CachedDims& D,
                              const RowCfg& R, const StagePtrs* SP,
                              const StageDims* SD) {
  hipStream_t stream = at::cuda::getCurrentCUDAStream();
  const int rows_b = (D.N + D.E + 255) / 256;
  const int comb1_b = ((long)D.N * D.HID + 255) / 256;
  const int comb2_b = ((long)D.N * D.OUT + 255) / 256;
  if (R.thread) {
    hipLaunchKernelGGL(cs_fwd_mlp_kernel<1>, dim3(rows_b), dim3(256), 0,
                       stream, P, D);
    hipLaunchKernelGGL(cs_fwd_reduce_kernel<1>, dim3(rows_b), dim3(256), 0,
                       stream, P, D);
  } else if (R.merge) {
    // stage role (with a store) + round-1 modules + round-1 reduce module
    const int L_ = R.lanes ? R.lanes : 32;
    const int rpb_ = ROW_NT / L_;
    const int stage = SP != nullptr ? 1 : 0;
    const dim3 grid(stage + (D.E + rpb_ - 1) / rpb_ + (D.N + rpb_ - 1) / rpb_);
    StagePtrs sp0;
    StageDims sd0;
    memset(&sp0, 0, sizeof(sp0));
    memset(&sd0, 0, sizeof(sd0));
    const StagePtrs& sp = stage ? *SP : sp0;
    const StageDims& sd = stage ? *SD : sd0;
    if (grid.x > 0) {
      if (L_ == 8)
        hipLaunchKernelGGL(cs_fwd_stage_mlp1_red1_lanes_kernel<8>, grid,
                           dim3(ROW_NT), 0, stream, P, D, sp, sd, stage);
      else if (L_ == 16)
        hipLaunchKernelGGL(cs_fwd_stage_mlp1_red1_lanes_kernel<16>, grid,
                           dim3(ROW_NT), 0, stream, P, D, sp, sd, stage);
      else
        hipLaunchKernelGGL(cs_fwd_stage_mlp1_red1_lanes_kernel<32>, grid,
                           dim3(ROW_NT), 0, stream, P, D, sp, sd, stage);
    }
  } else {
    if (SP != nullptr) {
      const int L_ = R.lanes ? R.lanes : 16;
      const int rpb_ = ROW_NT / L_;
      const dim3 grid(1 + (D.N + rpb_ - 1) / rpb_ + (D.E + rpb_ - 1) / rpb_);
      if (L_ == 8)
        hipLaunchKernelGGL(cs_fwd_stage_mlp1_lanes_kernel<8>, grid,
                           dim3(ROW_NT), 0, stream, P, D, *SP, *SD);
      else if (L_ == 16)
        hipLaunchKernelGGL(cs_fwd_stage_mlp1_lanes_kernel<16>, grid,
                           dim3(ROW_NT), 0, stream, P, D, *SP, *SD);
      else
        hipLaunchKernelGGL(cs_fwd_stage_mlp1_lanes_kernel<32>, grid,
                           dim3(ROW_NT), 0, stream, P, D, *SP, *SD);
    } else {
      LAUNCH_ROWS(K_FWD_MLP1, 16, D.N, D.E);
    }
    LAUNCH_ROWS(K_FWD_RED1, 32, D.E, D.N);
  }
  if (!R.fused)
    hipLaunchKernelGGL(cs_fwd_combine_kernel<1>, dim3(comb1_b), dim3(256), 0,
                       stream, P, D);
  if (R.thread) {
    hipLaunchKernelGGL(cs_fwd_mlp_kernel<2>, dim3(rows_b), dim3(256), 0,
                       stream, P, D);
    hipLaunchKernelGGL(cs_fwd_reduce_kernel<2>, dim3(rows_b), dim3(256), 0,
                       stream, P, D);
  } else {
    if (R.fused)
      LAUNCH_ROWS(K_FWD_COMB1_MLP2, 16, D.N, D.E);
    else
      LAUNCH_ROWS(K_FWD_MLP2, 16, D.N, D.E);
    LAUNCH_ROWS(K_FWD_RED2, 16, D.E, D.N);
  }
  if (R.fused) {
    // h2 and the per-model means, one block per model; then the whole
    // per-sample chain (final rows, head, loss, head backward) in one
    // launch: cached_step_bwd starts at cs_bwd_pool
    if (D.M > 0)
      hipLaunchKernelGGL(cs_fwd_comb2_pool_kernel, dim3(D.M), dim3(256), 0,
                         stream, P, D);
    // one sample a block (cs_head2) or four (cs_head, the oracle)
    const int hb = R.head ? (D.B < HD2_MAXB ? D.B : HD2_MAXB)
                          : (D.B < 32 ? D.B : 32);
    if (hb > 0) {
      if (R.head)
        hipLaunchKernelGGL(cs_head2_kernel, dim3(hb), dim3(256), 0, stream,
                           P, D);
      else
        hipLaunchKernelGGL(cs_head_kernel, dim3(hb), dim3(256), 0, stream,
                           P, D);
    }
    return;
  }
  hipLaunchKernelGGL(cs_fwd_combine_kernel<2>, dim3(comb2_b), dim3(256), 0,
                     stream, P, D);
  hipLaunchKernelGGL(cs_fwd_pool_kernel, dim3(1), dim3(512), 0, stream,
                     P, D);
  int head_blocks = ((long)D.B * D.FC + 255) / 256;
  if (head_blocks > 128) head_blocks = 128;
  hipLaunchKernelGGL(cs_fwd_head_kernel, dim3(head_blocks), dim3(256), 0,
                     stream, P, D);
  hipLaunchKernelGGL(cs_fwd_logits_kernel, dim3(D.B), dim3(512), 0,
                     stream, P, D);
  hipLaunchKernelGGL(cs_fwd_loss_kernel, dim3((D.B + 31) / 32), dim3(256),
                     0, stream, P, D);
}

void cached_step_fwd(std::vector<torch::Tensor> T, std::vector<double> fs) {
  CachedPtrs P;
  CachedDims D;
  RowCfg R;
  fill_ptrs(P, D, R, T, fs);
  step_fwd_launches(P, D, R, nullptr, nullptr);
}

// cached_step_fwd with the minibatch gathered from the device batch store by
// block 0 of the first launch (overlap mode only: the caller launches
// cached_stage itself otherwise).  store / perm / cursor / err / dims are
// cached_stage's arguments; the destinations are T's own staged inputs.
void cached_step_fwd_staged(std::vector<torch::Tensor> T,
                            std::vector<double> fs,
                            std::vector<torch::Tensor> store,
                            torch::Tensor perm, torch::Tensor cursor,
                            torch::Tensor err,
                            std::vector<torch::Tensor> dims) {
  CachedPtrs P;
  CachedDims D;
  RowCfg R;
  fill_ptrs(P, D, R, T, fs);
  TORCH_CHECK(R.overlap, "cached_step_fwd_staged: needs the lane-parallel "
              "fused launches with DDLS_AMD_STEP_OVERLAP on");
  StagePtrs SP;
  StageDims SD;
  cs_stage_args(SP, SD, "cached_step_fwd_staged", store,
                {T[C_GF], T[C_MASK], T[C_MODEL_IDS], T[C_ACTIONS],
                 T[C_OLD_LOGP], T[C_ADV], T[C_VTARG]},
                perm, cursor, err, dims);
  step_fwd_launches(P, D, R, &SP, &SD);
}

// defer_reduce: leave the row jobs' partial sums in wg_scratch for the folded
// optimiser tail (flat_sumsq_adam_folded), which then forms flat_g's row-job
// segments itself.  Ignored unless the merge switch is on and the row jobs
// are split (not with DDLS_AMD_WGRAD_MFMA=1); cached_step_reduce_deferred()
// tells the caller.  Default: flat_g is complete when this returns.
bool cached_step_reduce_deferred(bool defer_reduce) {
  const char* wm = getenv("DDLS_AMD_WGRAD_MFMA");
  const bool mfma = (wm != nullptr && wm[0] == '1');
  return defer_reduce && row_cfg().merge && !mfma;
}

// The row jobs' gradient segments for the folded tail: for each of the 24
// (job, tensor) pairs the flat start, the length and the offset of split 0's
// partial in wg_scratch (cs_bwd_w_reduce_kernel's layout: W, b, LN gamma, LN
// beta), then WSPLIT and WG_JSTRIDE.  offs is the host copy of C_OFFS.
std::vector<int64_t> cached_step_fold_segments(std::vector<int64_t> offs) {
  TORCH_CHECK((int)offs.size() == W_COUNT, "cached_step_fold_segments: ",
              (int)W_COUNT, " slot offsets expected, got ", offs.size());
  const int din[6] = {KF0, KFE, KMSG, KHID, KFE, KMSG};
  const int dout[6] = {KH, KH, KHID, KH, KH, KOUT};
  const int slot[6] = {W_LN_N1_W, W_LN_E1_W, W_LN_R1_W,
                       W_LN_N2_W, W_LN_E2_W, W_LN_R2_W};
  std::vector<int64_t> segs;
  for (int j = 0; j < 6; ++j) {
    const int64_t base = (int64_t)j * WSPLIT * WG_JSTRIDE;
    const int64_t units = (int64_t)din[j] * dout[j];
    const int64_t quad[4][3] = {
        {offs[slot[j] + 2], units, base},
        {offs[slot[j] + 3], dout[j], base + units},
        {offs[slot[j]], din[j], base + units + dout[j]},
        {offs[slot[j] + 1], din[j], base + units + dout[j] + din[j]}};
    for (int q = 0; q < 4; ++q)
      for (int c = 0; c < 3; ++c) segs.push_back(quad[q][c]);
  }
  segs.push_back(WSPLIT);
  segs.push_back(WG_JSTRIDE);
  return segs;
}

void cached_step_bwd(std::vector<torch::Tensor> T, std::vector<double> fs,
                     bool defer_reduce) {
  CachedPtrs P;
  CachedDims D;
  RowCfg R;
  fill_ptrs(P, D, R, T, fs);
  hipStream_t stream = at::cuda::getCurrentCUDAStream();
  // cs_bwd_pool keeps the minibatch's model ids in a fixed LDS array
  TORCH_CHECK(D.B <= 1024 && D.B <= SG_MAXB,
              "cached_step: minibatch larger than 1024");
  int hb = D.B < 32 ? D.B : 32;
  const int rows_b = (D.N + D.E + 255) / 256;
  const int scat_b = ((long)(D.N + D.E) * D.H + 255) / 256;
  if (!R.fused)
    hipLaunchKernelGGL(cs_bwd_head_kernel, dim3(hb), dim3(256), 0, stream,
                       P, D);
  if (R.head) {
    // the same roles in shorter blocks; its 16-byte loads need these rows
    // aligned (every scratch tensor is an allocation of its own)
    for (const float* q : {(const float*)P.fin, (const float*)P.gfinal,
                           (const float*)P.gh1p, (const float*)P.gh1v,
                           (const float*)P.h1p, (const float*)P.h1v})
      TORCH_CHECK(reinterpret_cast<uintptr_t>(q) % 16 == 0,
                  "cached_step: head scratch tensors must be 16-byte aligned");
    hipLaunchKernelGGL(cs_bwd_pool_wfc2_kernel, dim3(D.M + 1 + WFC2_NFC),
                       dim3(256), 0, stream, P, D);
  } else if (R.overlap)
    // one pool block per model + the graph-module block + the FC-column
    // blocks, which cs_bwd_w below then does not launch
    hipLaunchKernelGGL(cs_bwd_pool_wfc_kernel, dim3(D.M + 1 + WFC_NFC),
                       dim3(256), 0, stream, P, D);
  else
    hipLaunchKernelGGL(cs_bwd_pool_kernel, dim3(1), dim3(512), 0, stream,
                       P, D);
  if (R.thread)
    hipLaunchKernelGGL(cs_bwd_reduce_kernel<2>, dim3(rows_b), dim3(256), 0,
                       stream, P, D);
  else
    LAUNCH_ROWS(K_BWD_RED2, 16, D.E, D.N);
  if (!R.fused)
    hipLaunchKernelGGL(cs_bwd_scatter_kernel<2>, dim3(scat_b), dim3(256), 0,
                       stream, P, D);
  if (R.thread) {
    hipLaunchKernelGGL(cs_bwd_mlp2_kernel, dim3(rows_b), dim3(256), 0,
                       stream, P, D);
    hipLaunchKernelGGL(cs_bwd_reduce_kernel<1>, dim3(rows_b), dim3(256), 0,
                       stream, P, D);
  } else {
    if (R.fused)
      LAUNCH_ROWS(K_BWD_SCAT2_MLP2, 16, D.N, D.E);
    else
      LAUNCH_ROWS(K_BWD_MLP2, 16, D.N, D.E);
    LAUNCH_ROWS(K_BWD_RED1, 32, D.E, D.N);
  }
  const int nsplit = D.wgrad_mfma ? 1 : WSPLIT;
  if (R.merge && nsplit > 1 && D.B > 0) {
    // the scatter's row blocks and statistics block, then the 6 x WSPLIT
    // row-job blocks, in one launch
    const int sg_b = (D.N + SG_RPB - 1) / SG_RPB + (D.E + SG_RPB - 1) / SG_RPB
                     + 1;
    hipLaunchKernelGGL(cs_bwd_scat1_gu1_w_kernel, dim3(sg_b + 6 * WSPLIT),
                       dim3(ROW_NT), 0, stream, P, D);
    if (!defer_reduce)
      hipLaunchKernelGGL(cs_bwd_w_reduce_kernel, dim3(6), dim3(256), 0,
                         stream, P, D);
    return;
  }
  if (R.fused) {
    // row blocks, then the loss-statistics block
    const int sg_b = (D.N + SG_RPB - 1) / SG_RPB + (D.E + SG_RPB - 1) / SG_RPB
                     + 1;
    if (D.B > 0)
      hipLaunchKernelGGL(cs_bwd_scat1_gu1_kernel, dim3(sg_b), dim3(ROW_NT),
                         0, stream, P, D);
  } else {
    hipLaunchKernelGGL(cs_bwd_scatter_kernel<1>, dim3(scat_b), dim3(256), 0,
                       stream, P, D);
  }
  if (R.fused) {
    // gu_z1 / gu_e1 came out of the scatter launch above
  } else if (R.thread) {
    hipLaunchKernelGGL(cs_bwd_gu1_kernel, dim3(rows_b), dim3(256), 0, stream,
                       P, D);
  } else {
    const int gu1_b =
        (int)(((long)D.N * KF0 + (long)D.E * KFE + ROW_NT - 1) / ROW_NT);
    if (gu1_b > 0)
      hipLaunchKernelGGL(cs_bwd_gu1_lanes_kernel, dim3(gu1_b), dim3(ROW_NT),
                         0, stream, P, D);
  }
  // 6 row jobs x nsplit, the graph-module block, 16 FC-column blocks; in
  // overlap mode the 17 B-row blocks ran in cs_bwd_pool_wfc above, and with
  // the row-job grid their paths are never entered
  hipLaunchKernelGGL(cs_bwd_w_kernel,
                     dim3(6 * nsplit + (R.overlap ? 0 : 1 + 16)), dim3(256),
                     0, stream, P, D);
  if (nsplit > 1 && !(defer_reduce && R.merge))
    hipLaunchKernelGGL(cs_bwd_w_reduce_kernel, dim3(6), dim3(256), 0,
                       stream, P, D);
}
