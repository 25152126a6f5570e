// MFMA (matrix-core) forward kernels for the MeanPool GNN on gfx950.
//
// The row/message MLPs are GEMM-shaped (R x F @ F^T x H with R ~ 1e4..4e4,
// F <= 64, H in {16, 64}), so the matrix units do the contraction:
// v_mfma_f32_16x16x4_f32 tiles (f32-in/f32-acc — exact fmaf-chain numerics,
// same data as the VALU path) with the LayerNorm fused in front via lane
// shuffles and an LDS-staged normalised tile.  Replaces the wave-per-row GEMV
// of meanpool.hip on the training path; the segment mean over dst-CSR is a
// separate light kernel (segment_combine) since backward needs the
// per-message activations materialised anyway.
//
// Fragment maps for 16x16x4 (cdna_hip_programming.md "FP32-input MFMA"):
//   A[i = lane&15][k = lane>>4], B[k = lane>>4][j = lane&15],
//   C/D: col = lane&15, row = (lane>>4)*4 + reg.
#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>
#include <cstring>
#include <vector>

#define WAVE 64
#define WAVES_PER_BLOCK 4
#define BLOCK (WAVE * WAVES_PER_BLOCK)
#define LN_EPS 1e-5f

typedef float f32x4_t __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------
// y[r, :] = relu(LN(x[r, :]) @ W^T + b), W torch-layout [H, F].
// One 16-row tile per wave; K staged through LDS zero-padded to F_pad.
// Requires H % 16 == 0, H <= 64, F <= 64.
__global__ void __launch_bounds__(BLOCK)
row_mlp_mfma_kernel(const float* __restrict__ x,
                    const float* __restrict__ ln_g,
                    const float* __restrict__ ln_b,
                    const float* __restrict__ W,
                    const float* __restrict__ b,
                    float* __restrict__ y,
                    int R, int F, int H) {
    const int F_pad = (F + 3) & ~3;
    const int Q = F_pad / 4;            // elements per lane in phase A
    __shared__ float xs[WAVES_PER_BLOCK][16][64 + 4];
    __shared__ float ws[64][64 + 4];    // W zero-padded to [H][F_pad]
    for (int i = threadIdx.x; i < H * F_pad; i += BLOCK) {
        const int j = i / F_pad, k = i % F_pad;
        ws[j][k] = (k < F) ? W[(long)j * F + k] : 0.0f;
    }
    __syncthreads();

    const int wave = threadIdx.x / WAVE;
    const int lane = threadIdx.x % WAVE;
    const int mrow = lane & 15;         // M index within the tile
    const int kpart = lane >> 4;        // 0..3
    const int tiles = (R + 16 * WAVES_PER_BLOCK - 1) / (16 * WAVES_PER_BLOCK);
    for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int rbase = (t * WAVES_PER_BLOCK + wave) * 16;
        const int r = rbase + mrow;
        // phase A: LayerNorm 16 rows, 4 lanes per row
        float vals[16];
        float s = 0.0f;
        for (int i = 0; i < Q; ++i) {
            const int k = kpart * Q + i;
            const float v = (r < R && k < F) ? x[(long)r * F + k] : 0.0f;
            vals[i] = v;
            s += v;
        }
        s += __shfl_xor(s, 16, WAVE);
        s += __shfl_xor(s, 32, WAVE);
        const float mean = s / F;
        float d2 = 0.0f;
        for (int i = 0; i < Q; ++i) {
            const int k = kpart * Q + i;
            const float d = (k < F) ? vals[i] - mean : 0.0f;
            vals[i] = d;
            d2 += d * d;
        }
        d2 += __shfl_xor(d2, 16, WAVE);
        d2 += __shfl_xor(d2, 32, WAVE);
        const float inv_sigma = rsqrtf(d2 / F + LN_EPS);
        for (int i = 0; i < Q; ++i) {
            const int k = kpart * Q + i;
            if (k < F_pad)
                xs[wave][mrow][k] =
                    (k < F) ? vals[i] * inv_sigma * ln_g[k] + ln_b[k] : 0.0f;
        }
        __builtin_amdgcn_wave_barrier();
        // phase B: 16x16 output tiles on the matrix core
        for (int jt = 0; jt < H; jt += 16) {
            f32x4_t acc = {0.0f, 0.0f, 0.0f, 0.0f};
            for (int kk = 0; kk < F_pad; kk += 4) {
                const float a = xs[wave][mrow][kk + kpart];
                const float bb = ws[jt + mrow][kk + kpart];
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bb, acc, 0, 0, 0);
            }
            const int col = jt + mrow;
            const float bias = b[col];
            for (int reg = 0; reg < 4; ++reg) {
                const int row = rbase + kpart * 4 + reg;
                if (row < R)
                    y[(long)row * H + col] = fmaxf(acc[reg] + bias, 0.0f);
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// ---------------------------------------------------------------------------
// Per-message reduce-MLP on the matrix core: messages 0..E-1 are edge
// messages [hn[src[m]] || he[m]], messages E..E+N-1 are self messages
// [hn[v] || 0].  r = relu(LN(msg) @ Wr^T + br) -> r_edge [E][OUT] (edge-id
// indexed) and r_self [N][OUT].  Requires half == 16 (MSG = 32),
// OUT % 16 == 0, OUT <= 64.
__global__ void __launch_bounds__(BLOCK)
message_mlp_mfma_kernel(const float* __restrict__ hn,
                        const float* __restrict__ he,
                        const long* __restrict__ src,
                        const float* __restrict__ ln_g,
                        const float* __restrict__ ln_b,
                        const float* __restrict__ Wr,
                        const float* __restrict__ br,
                        float* __restrict__ r_edge,
                        float* __restrict__ r_self,
                        long E, int N, int OUT) {
    const int MSG = 32, Q = 8;
    __shared__ float ms[WAVES_PER_BLOCK][16][MSG + 4];
    __shared__ float ws[64][MSG + 4];
    for (int i = threadIdx.x; i < OUT * MSG; i += BLOCK)
        ws[i / MSG][i % MSG] = Wr[i];
    __syncthreads();

    const int wave = threadIdx.x / WAVE;
    const int lane = threadIdx.x % WAVE;
    const int mrow = lane & 15;
    const int kpart = lane >> 4;
    const long M = E + N;
    const long tiles = (M + 16 * WAVES_PER_BLOCK - 1) / (16 * WAVES_PER_BLOCK);
    for (long t = blockIdx.x; t < tiles; t += gridDim.x) {
        const long mbase = (t * WAVES_PER_BLOCK + wave) * 16;
        const long m = mbase + mrow;
        float vals[Q];
        float s = 0.0f;
        if (m < M) {
            const bool is_edge = m < E;
            const long node = is_edge ? src[m] : (m - E);
            for (int i = 0; i < Q; ++i) {
                const int k = kpart * Q + i;
                float v;
                if (k < 16)
                    v = hn[node * 16 + k];
                else if (is_edge)
                    v = he[m * 16 + (k - 16)];
                else
                    v = 0.0f;  // self message upper half is zero
                vals[i] = v;
                s += v;
            }
        } else {
            for (int i = 0; i < Q; ++i) vals[i] = 0.0f;
        }
        s += __shfl_xor(s, 16, WAVE);
        s += __shfl_xor(s, 32, WAVE);
        const float mean = s / MSG;
        float d2 = 0.0f;
        for (int i = 0; i < Q; ++i) {
            const float d = (m < M) ? vals[i] - mean : 0.0f;
            vals[i] = d;
            d2 += d * d;
        }
        d2 += __shfl_xor(d2, 16, WAVE);
        d2 += __shfl_xor(d2, 32, WAVE);
        const float inv_sigma = rsqrtf(d2 / MSG + LN_EPS);
        for (int i = 0; i < Q; ++i) {
            const int k = kpart * Q + i;
            ms[wave][mrow][k] = vals[i] * inv_sigma * ln_g[k] + ln_b[k];
        }
        __builtin_amdgcn_wave_barrier();
        for (int jt = 0; jt < OUT; jt += 16) {
            f32x4_t acc = {0.0f, 0.0f, 0.0f, 0.0f};
            for (int kk = 0; kk < MSG; kk += 4) {
                const float a = ms[wave][mrow][kk + kpart];
                const float bb = ws[jt + mrow][kk + kpart];
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bb, acc, 0, 0, 0);
            }
            const int col = jt + mrow;
            const float bias = br[col];
            for (int reg = 0; reg < 4; ++reg) {
                const long row = mbase + kpart * 4 + reg;
                if (row < M) {
                    const float r = fmaxf(acc[reg] + bias, 0.0f);
                    if (row < E)
                        r_edge[row * OUT + col] = r;
                    else
                        r_self[(row - E) * OUT + col] = r;
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// ---------------------------------------------------------------------------
// out[v] = indeg(v) > 0 ? (r_self[v] + sum_csr r_edge[edge_order[e]])
//                         / (indeg+1)
//                       : 0   (DGL zero-fill), summed in the same order as
// the fused message_reduce (self first, then CSR order).
__global__ void __launch_bounds__(BLOCK)
segment_combine_kernel(const float* __restrict__ r_edge,
                       const float* __restrict__ r_self,
                       const long* __restrict__ edge_order,
                       const long* __restrict__ indptr,
                       float* __restrict__ out,
                       int N, int OUT) {
    const int wave = threadIdx.x / WAVE;
    const int lane = threadIdx.x % WAVE;
    const int v0 = blockIdx.x * WAVES_PER_BLOCK + wave;
    const int stride = gridDim.x * WAVES_PER_BLOCK;
    for (int v = v0; v < N; v += stride) {
        const long e_begin = indptr[v];
        const long e_end = indptr[v + 1];
        const int indeg = (int)(e_end - e_begin);
        if (lane < OUT) {
            if (indeg > 0) {
                float acc = r_self[(long)v * OUT + lane];
                for (long e = e_begin; e < e_end; ++e)
                    acc += r_edge[edge_order[e] * OUT + lane];
                out[(long)v * OUT + lane] = acc / (indeg + 1);
            } else {
                out[(long)v * OUT + lane] = 0.0f;
            }
        }
    }
}

// ---------------------------------------------------------------------------
static int grid_for_tiles(long rows) {
    long blocks = (rows + 16L * WAVES_PER_BLOCK - 1) / (16L * WAVES_PER_BLOCK);
    if (blocks > 4096) blocks = 4096;
    if (blocks < 1) blocks = 1;
    return (int)blocks;
}

torch::Tensor row_mlp_mfma(torch::Tensor x, torch::Tensor ln_g,
                           torch::Tensor ln_b, torch::Tensor W,
                           torch::Tensor b) {
    TORCH_CHECK(x.is_cuda() && x.dtype() == torch::kFloat32);
    const int R = (int)x.size(0), F = (int)x.size(1), H = (int)W.size(0);
    TORCH_CHECK(F <= 64 && H <= 64 && H % 16 == 0,
                "row_mlp_mfma needs F<=64, H multiple of 16");
    auto y = torch::empty({R, H}, x.options());
    if (R == 0) return y;
    hipStream_t stream = at::cuda::getCurrentCUDAStream();
    hipLaunchKernelGGL(row_mlp_mfma_kernel, dim3(grid_for_tiles(R)),
                       dim3(BLOCK), 0, stream,
                       x.data_ptr<float>(), ln_g.data_ptr<float>(),
                       ln_b.data_ptr<float>(), W.data_ptr<float>(),
                       b.data_ptr<float>(), y.data_ptr<float>(), R, F, H);
    return y;
}

std::vector<torch::Tensor> message_mlp_mfma(
    torch::Tensor hn, torch::Tensor he, torch::Tensor src, torch::Tensor ln_g,
    torch::Tensor ln_b, torch::Tensor Wr, torch::Tensor br) {
    TORCH_CHECK(hn.is_cuda() && hn.dtype() == torch::kFloat32);
    const long E = src.size(0);
    const int N = (int)hn.size(0), half = (int)hn.size(1);
    const int OUT = (int)Wr.size(0);
    TORCH_CHECK(half == 16 && (int)Wr.size(1) == 32,
                "message_mlp_mfma needs half==16 (MSG=32)");
    TORCH_CHECK(OUT <= 64 && OUT % 16 == 0);
    auto r_edge = torch::empty({E, OUT}, hn.options());
    auto r_self = torch::empty({N, OUT}, hn.options());
    hipStream_t stream = at::cuda::getCurrentCUDAStream();
    hipLaunchKernelGGL(message_mlp_mfma_kernel,
                       dim3(grid_for_tiles(E + N)), dim3(BLOCK), 0, stream,
                       hn.data_ptr<float>(), he.data_ptr<float>(),
                       src.data_ptr<long>(), ln_g.data_ptr<float>(),
                       ln_b.data_ptr<float>(), Wr.data_ptr<float>(),
                       br.data_ptr<float>(), r_edge.data_ptr<float>(),
                       r_self.data_ptr<float>(), E, N, OUT);
    return {r_edge, r_self};
}

torch::Tensor segment_combine(torch::Tensor r_edge, torch::Tensor r_self,
                              torch::Tensor edge_order, torch::Tensor indptr) {
    const int N = (int)r_self.size(0), OUT = (int)r_self.size(1);
    auto out = torch::empty({N, OUT}, r_self.options());
    if (N == 0) return out;
    hipStream_t stream = at::cuda::getCurrentCUDAStream();
    int blocks = (N + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(segment_combine_kernel, dim3(blocks), dim3(BLOCK), 0,
                       stream, r_edge.data_ptr<float>(),
                       r_self.data_ptr<float>(), edge_order.data_ptr<long>(),
                       indptr.data_ptr<long>(), out.data_ptr<float>(), N, OUT);
    return out;
}

// ---------------------------------------------------------------------------
// segment_mean backward: gx[n] = gout[g]/count(g) for n in graph g.
__global__ void __launch_bounds__(BLOCK)
segment_mean_bwd_kernel(const float* __restrict__ gout,
                        const long* __restrict__ node_ptr,
                        float* __restrict__ gx,
                        int G, int F) {
    // one block per graph, node-parallel broadcast (F <= 16)
    const int feat = threadIdx.x & 15;
    const int nsub = threadIdx.x >> 4;
    for (int g = blockIdx.x; g < G; g += gridDim.x) {
        const long n_begin = node_ptr[g];
        const long n_end = node_ptr[g + 1];
        const long cnt = n_end - n_begin;
        if (feat < F && cnt > 0) {
            const float val = gout[(long)g * F + feat] / cnt;
            for (long n = n_begin + nsub; n < n_end; n += 16)
                gx[n * F + feat] = val;
        }
    }
}

torch::Tensor segment_mean_bwd(torch::Tensor gout, torch::Tensor node_ptr,
                               int64_t N) {
    const int G = (int)gout.size(0), F = (int)gout.size(1);
    TORCH_CHECK(F <= 16, "segment_mean_bwd kernel is tiled for F <= 16");
    // node_ptr spans every row (the flat batch is graph-contiguous and, in
    // the captured path, the dummy graph owns all padding), so plain empty +
    // full overwrite is safe
    auto gx = torch::empty({N, F}, gout.options());
    if (G == 0) return gx.zero_();
    hipStream_t stream = at::cuda::getCurrentCUDAStream();
    int blocks = G > 2048 ? 2048 : G;
    hipLaunchKernelGGL(segment_mean_bwd_kernel, dim3(blocks), dim3(BLOCK), 0,
                       stream, gout.data_ptr<float>(),
                       node_ptr.data_ptr<long>(), gx.data_ptr<float>(), G, F);
    return gx;
}

// ---------------------------------------------------------------------------
// Fused flat Adam + grad clip: one kernel over the flat param/grad/m/v
// buffers (the captured step keeps every param and grad a VIEW into these).
// scale = min(1, clip / (sqrt(normsq) + 1e-6)) matches
// torch.nn.utils.clip_grad_norm_; the update matches torch Adam exactly
// (step_size = lr/bias1, denom = sqrt(v)/sqrt(bias2) + eps).  Grads are
// zeroed after consumption so the next backward accumulates from zero.
__global__ void flat_adam_kernel(float* __restrict__ p,
                                 float* __restrict__ g,
                                 float* __restrict__ m,
                                 float* __restrict__ v,
                                 const float* __restrict__ step_t,  // [1]
                                 const float* __restrict__ normsq,  // [1]
                                 long numel, float clip, float lr, float b1,
                                 float b2, float eps) {
    const float t = step_t[0];
    float scale = 1.0f;
    if (clip > 0.0f) {
        const float norm = sqrtf(normsq[0]);
        const float c = clip / (norm + 1e-6f);
        scale = fminf(c, 1.0f);
    }
    const float bias1 = 1.0f - powf(b1, t);
    const float bias2 = 1.0f - powf(b2, t);
    const float step_size = lr / bias1;
    const float inv_sqrt_bias2 = rsqrtf(bias2);
    const long i0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long stride = (long)gridDim.x * blockDim.x;
    for (long i = i0; i < numel; i += stride) {
        const float gi = g[i] * scale;
        const float mi = b1 * m[i] + (1.0f - b1) * gi;
        const float vi = b2 * v[i] + (1.0f - b2) * gi * gi;
        m[i] = mi;
        v[i] = vi;
        p[i] -= step_size * mi / (sqrtf(vi) * inv_sqrt_bias2 + eps);
        g[i] = 0.0f;
    }
}

__global__ void step_inc_kernel(float* step_t) { step_t[0] += 1.0f; }

void flat_adam(torch::Tensor p, torch::Tensor g, torch::Tensor m,
               torch::Tensor v, torch::Tensor step_t, torch::Tensor normsq,
               double clip, double lr, double b1, double b2, double eps) {
    const long numel = p.numel();
    hipStream_t stream = at::cuda::getCurrentCUDAStream();
    hipLaunchKernelGGL(step_inc_kernel, dim3(1), dim3(1), 0, stream,
                       step_t.data_ptr<float>());
    long blocks = (numel + BLOCK - 1) / BLOCK;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(flat_adam_kernel, dim3((int)blocks), dim3(BLOCK), 0,
                       stream, p.data_ptr<float>(), g.data_ptr<float>(),
                       m.data_ptr<float>(), v.data_ptr<float>(),
                       step_t.data_ptr<float>(), normsq.data_ptr<float>(),
                       numel, (float)clip, (float)lr, (float)b1, (float)b2,
                       (float)eps);
}

// ===========================================================================
// MFMA backward for the message reduce-MLP (replaces the wave-per-message
// meanpool_bwd kernel for the tuned shape half=16/MSG=32).  Three stages:
//   K1 msg_bwd_ga:   gA[m,j] = relu'(r[m,j]) * gout[node(m),j] / (deg+1)
//   K2 msg_bwd_data: gXln = gA @ Wr (MFMA) -> LayerNorm backward ->
//                    scatter ghn (atomic) / ghe; accumulates gln_g/gln_b via
//                    LDS block partials + atomics
//   K3 msg_bwd_wr:   gWr = gA^T @ xln (MFMA over message chunks, xln
//                    recomputed as mhat*g+b) + gbr column sums, atomics
// Message order: 0..E-1 edge messages, E..E+N-1 self messages (as forward).
// ALL reductions live in these kernels: torch's multi-pass .sum() proved
// unstable under hipGraph replay (outputs drift after ~100 replays), so no
// torch reduction may run inside the captured region.
// ===========================================================================

__global__ void __launch_bounds__(BLOCK)
msg_bwd_ga_kernel(const float* __restrict__ r_edge,
                  const float* __restrict__ r_self,
                  const long* __restrict__ dst,
                  const long* __restrict__ indptr,
                  const float* __restrict__ gout,
                  float* __restrict__ gA,
                  long E, int N, int OUT) {
    const int wave = threadIdx.x / WAVE;
    const int lane = threadIdx.x % WAVE;
    const long M = E + (long)N;
    const long m0 = (long)blockIdx.x * WAVES_PER_BLOCK + wave;
    const long stride = (long)gridDim.x * WAVES_PER_BLOCK;
    for (long m = m0; m < M; m += stride) {
        const long node = (m < E) ? dst[m] : (m - E);
        const long deg = indptr[node + 1] - indptr[node];
        if (lane < OUT) {
            float v = 0.0f;
            if (deg > 0) {
                const float r = (m < E) ? r_edge[m * OUT + lane]
                                        : r_self[(m - E) * OUT + lane];
                if (r > 0.0f)
                    v = gout[node * OUT + lane] / (float)(deg + 1);
            }
            gA[m * OUT + lane] = v;
        }
    }
}

__global__ void __launch_bounds__(BLOCK)
msg_bwd_data_kernel(const float* __restrict__ hn,
                    const float* __restrict__ he,
                    const long* __restrict__ src,
                    const float* __restrict__ ln_g,
                    const float* __restrict__ Wr,
                    const float* __restrict__ gA,
                    float* __restrict__ ghn,     // [N,16] pre-zeroed
                    float* __restrict__ ghe,     // [E,16]
                    float* __restrict__ mhat_out,  // [M,32]
                    float* __restrict__ gln_g_out,  // [32] pre-zeroed
                    float* __restrict__ gln_b_out,  // [32] pre-zeroed
                    long E, int N, int OUT) {
    const int MSG = 32, Q = 8;
    __shared__ float ws[64][MSG + 4];          // Wr [OUT][MSG]
    __shared__ float gx[WAVES_PER_BLOCK][16][MSG + 4];
    __shared__ float lng_acc[MSG], lnb_acc[MSG];
    for (int i = threadIdx.x; i < OUT * MSG; i += BLOCK)
        ws[i / MSG][i % MSG] = Wr[i];
    if (threadIdx.x < MSG) {
        lng_acc[threadIdx.x] = 0.0f;
        lnb_acc[threadIdx.x] = 0.0f;
    }
    __syncthreads();

    const int wave = threadIdx.x / WAVE;
    const int lane = threadIdx.x % WAVE;
    const int mrow = lane & 15;
    const int kpart = lane >> 4;
    const long M = E + (long)N;
    const long tiles = (M + 16 * WAVES_PER_BLOCK - 1) / (16 * WAVES_PER_BLOCK);
    for (long t = blockIdx.x; t < tiles; t += gridDim.x) {
        const long mbase = (t * WAVES_PER_BLOCK + wave) * 16;
        // gXln tile = gA_tile @ Wr on the matrix core
        for (int jt = 0; jt < MSG; jt += 16) {
            f32x4_t acc = {0.0f, 0.0f, 0.0f, 0.0f};
            for (int kk = 0; kk < OUT; kk += 4) {
                const long m = mbase + mrow;
                const float a = (m < M)
                    ? gA[m * OUT + kk + kpart] : 0.0f;
                const float bb = ws[kk + kpart][jt + mrow];
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bb, acc, 0, 0, 0);
            }
            for (int reg = 0; reg < 4; ++reg)
                gx[wave][kpart * 4 + reg][jt + mrow] = acc[reg];
        }
        __builtin_amdgcn_wave_barrier();

        // per-message LayerNorm backward + scatter (fwd lane layout)
        const long m = mbase + mrow;
        float vals[Q];
        float s = 0.0f;
        const bool live = (m < M);
        const bool is_edge = live && (m < E);
        const long node = !live ? 0 : (is_edge ? src[m] : (m - E));
        for (int i = 0; i < Q; ++i) {
            const int k = kpart * Q + i;
            float v = 0.0f;
            if (live) {
                if (k < 16) v = hn[node * 16 + k];
                else if (is_edge) v = he[m * 16 + (k - 16)];
            }
            vals[i] = v;
            s += v;
        }
        s += __shfl_xor(s, 16, WAVE);
        s += __shfl_xor(s, 32, WAVE);
        const float mean = s / MSG;
        float d2 = 0.0f;
        for (int i = 0; i < Q; ++i) {
            const float d = live ? vals[i] - mean : 0.0f;
            vals[i] = d;
            d2 += d * d;
        }
        d2 += __shfl_xor(d2, 16, WAVE);
        d2 += __shfl_xor(d2, 32, WAVE);
        const float inv_sigma = rsqrtf(d2 / MSG + LN_EPS);
        float gyg[Q], mh[Q];
        float s1 = 0.0f, s2 = 0.0f;
        for (int i = 0; i < Q; ++i) {
            const int k = kpart * Q + i;
            mh[i] = vals[i] * inv_sigma;
            const float gy = gx[wave][mrow][k];
            gyg[i] = gy * ln_g[k];
            s1 += gyg[i];
            s2 += gyg[i] * mh[i];
        }
        s1 += __shfl_xor(s1, 16, WAVE);
        s1 += __shfl_xor(s1, 32, WAVE);
        s2 += __shfl_xor(s2, 16, WAVE);
        s2 += __shfl_xor(s2, 32, WAVE);
        const float m1 = s1 / MSG, m2 = s2 / MSG;
        if (live) {
            for (int i = 0; i < Q; ++i) {
                const int k = kpart * Q + i;
                mhat_out[m * MSG + k] = mh[i];
                const float gy = gx[wave][mrow][k];
                atomicAdd(&lnb_acc[k], gy);
                atomicAdd(&lng_acc[k], gy * mh[i]);
                const float gmsg = inv_sigma * (gyg[i] - m1 - mh[i] * m2);
                if (k < 16)
                    atomicAdd(&ghn[node * 16 + k], gmsg);
                else if (is_edge)
                    ghe[m * 16 + (k - 16)] = gmsg;
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    if (threadIdx.x < MSG) {
        atomicAdd(&gln_g_out[threadIdx.x], lng_acc[threadIdx.x]);
        atomicAdd(&gln_b_out[threadIdx.x], lnb_acc[threadIdx.x]);
    }
}

// small chunks: the chip needs >>256 workgroups to fill (8 XCDs x 32 CU);
// 1024-message chunks left only ~21 blocks in flight
#define K3_CHUNK 128

__global__ void __launch_bounds__(BLOCK)
msg_bwd_wr_kernel(const float* __restrict__ gA,
                  const float* __restrict__ mhat,
                  const float* __restrict__ ln_g,
                  const float* __restrict__ ln_b,
                  float* __restrict__ gWr,   // [OUT,32] pre-zeroed
                  float* __restrict__ gbr,   // [OUT] pre-zeroed
                  long M, int OUT) {
    const int MSG = 32;
    const int wave = threadIdx.x / WAVE;
    const int lane = threadIdx.x % WAVE;
    const int mrow = lane & 15;
    const int kpart = lane >> 4;
    const int T = (OUT / 16) * 2;          // (jt, kt) tiles
    const long chunks = (M + K3_CHUNK - 1) / K3_CHUNK;
    for (long c = blockIdx.x; c < chunks; c += gridDim.x) {
        const long c0 = c * K3_CHUNK;
        for (int t = wave; t < T; t += WAVES_PER_BLOCK) {
            const int jt = (t >> 1) * 16;   // OUT tile base
            const int kt = (t & 1) * 16;    // msg-dim tile base
            f32x4_t acc = {0.0f, 0.0f, 0.0f, 0.0f};
            float sba = 0.0f;               // gbr partial (kt==0 tiles only)
            for (int kk = 0; kk < K3_CHUNK; kk += 4) {
                const long m = c0 + kk + kpart;
                float a = 0.0f, bb = 0.0f;
                if (m < M) {
                    a = gA[m * OUT + jt + mrow];
                    const int k = kt + mrow;
                    bb = mhat[m * MSG + k] * ln_g[k] + ln_b[k];
                }
                if (kt == 0) sba += a;
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bb, acc, 0, 0, 0);
            }
            for (int reg = 0; reg < 4; ++reg)
                atomicAdd(&gWr[(long)(jt + kpart * 4 + reg) * MSG + kt + mrow],
                          acc[reg]);
            if (kt == 0) {
                sba += __shfl_xor(sba, 16, WAVE);
                sba += __shfl_xor(sba, 32, WAVE);
                if (kpart == 0) atomicAdd(&gbr[jt + mrow], sba);
            }
        }
    }
}

std::vector<torch::Tensor> message_reduce_bwd_mfma(
    torch::Tensor hn, torch::Tensor he, torch::Tensor src, torch::Tensor dst,
    torch::Tensor indptr, torch::Tensor ln_g, torch::Tensor ln_b,
    torch::Tensor Wr, torch::Tensor r_edge, torch::Tensor r_self,
    torch::Tensor gout) {
    const long E = src.size(0);
    const int N = (int)hn.size(0), OUT = (int)Wr.size(0);
    TORCH_CHECK((int)hn.size(1) == 16 && (int)Wr.size(1) == 32);
    TORCH_CHECK(OUT % 16 == 0 && OUT <= 64);
    const long M = E + N;
    auto opt = hn.options();
    auto gA = torch::empty({M, (long)OUT}, opt);
    auto mhat = torch::empty({M, 32L}, opt);
    auto ghn = torch::zeros({(long)N, 16L}, opt);
    auto ghe = torch::zeros({E, 16L}, opt);
    auto gWr = torch::zeros({(long)OUT, 32L}, opt);
    auto gbr = torch::zeros({(long)OUT}, opt);
    auto gln_g = torch::zeros({32L}, opt);
    auto gln_b = torch::zeros({32L}, opt);
    hipStream_t stream = at::cuda::getCurrentCUDAStream();
    {
        long blocks = (M + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK;
        if (blocks > 4096) blocks = 4096;
        hipLaunchKernelGGL(msg_bwd_ga_kernel, dim3((int)blocks), dim3(BLOCK),
                           0, stream, r_edge.data_ptr<float>(),
                           r_self.data_ptr<float>(), dst.data_ptr<long>(),
                           indptr.data_ptr<long>(), gout.data_ptr<float>(),
                           gA.data_ptr<float>(), E, N, OUT);
    }
    {
        long blocks = grid_for_tiles(M);
        if (blocks > 1024) blocks = 1024;
        hipLaunchKernelGGL(msg_bwd_data_kernel, dim3((int)blocks),
                           dim3(BLOCK), 0, stream, hn.data_ptr<float>(),
                           he.data_ptr<float>(), src.data_ptr<long>(),
                           ln_g.data_ptr<float>(), Wr.data_ptr<float>(),
                           gA.data_ptr<float>(), ghn.data_ptr<float>(),
                           ghe.data_ptr<float>(), mhat.data_ptr<float>(),
                           gln_g.data_ptr<float>(), gln_b.data_ptr<float>(),
                           E, N, OUT);
    }
    {
        long blocks = (M + K3_CHUNK - 1) / K3_CHUNK;
        if (blocks > 2048) blocks = 2048;
        hipLaunchKernelGGL(msg_bwd_wr_kernel, dim3((int)blocks), dim3(BLOCK),
                           0, stream, gA.data_ptr<float>(),
                           mhat.data_ptr<float>(), ln_g.data_ptr<float>(),
                           ln_b.data_ptr<float>(), gWr.data_ptr<float>(),
                           gbr.data_ptr<float>(), M, OUT);
    }
    return {ghn, ghe, gWr, gbr, gln_g, gln_b};
}

// ---------------------------------------------------------------------------
// capture-safe sum of squares (torch multi-pass reductions proved unstable
// under hipGraph replay); out is zeroed by the leading 1-thread kernel.
__global__ void zero1_kernel(float* out) { out[0] = 0.0f; }

__global__ void __launch_bounds__(BLOCK)
sumsq_kernel(const float* __restrict__ x, float* __restrict__ out, long n) {
    __shared__ float part[WAVES_PER_BLOCK];
    const int wave = threadIdx.x / WAVE;
    const int lane = threadIdx.x % WAVE;
    float s = 0.0f;
    for (long i = (long)blockIdx.x * BLOCK + threadIdx.x; i < n;
         i += (long)gridDim.x * BLOCK)
        s += x[i] * x[i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        s += __shfl_down(s, off, WAVE);
    if (lane == 0) part[wave] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.0f;
        for (int w = 0; w < WAVES_PER_BLOCK; ++w) t += part[w];
        atomicAdd(out, t);
    }
}

void flat_sumsq(torch::Tensor x, torch::Tensor out) {
    const long n = x.numel();
    hipStream_t stream = at::cuda::getCurrentCUDAStream();
    hipLaunchKernelGGL(zero1_kernel, dim3(1), dim3(1), 0, stream,
                       out.data_ptr<float>());
    long blocks = (n + BLOCK - 1) / BLOCK;
    if (blocks > 512) blocks = 512;
    hipLaunchKernelGGL(sumsq_kernel, dim3((int)blocks), dim3(BLOCK), 0,
                       stream, x.data_ptr<float>(), out.data_ptr<float>(), n);
}

// ---------------------------------------------------------------------------
// Two-launch optimiser tail of the captured step (flat_sumsq + flat_adam are
// four: zero1, sumsq, step_inc, flat_adam).
//   K1 sumsq_partials: sumsq_kernel's grid and per-block reduction, but each
//      block STORES its partial (no atomic, so nothing to zero first); block
//      0 also advances step_t (the former step_inc).
//   K2 flat_adam_partials: every block adds the partials from 0 in block
//      order — one of the orders the float atomics of sumsq_kernel can
//      produce, and the same one on every run — and then runs
//      flat_adam_kernel's loop.  Block 0 publishes the sum in normsq[0].
#define SUMSQ_MAX_BLOCKS 512

__global__ void __launch_bounds__(BLOCK)
sumsq_partials_kernel(const float* __restrict__ x,
                      float* __restrict__ partials, float* step_t, long n) {
    __shared__ float part[WAVES_PER_BLOCK];
    const int wave = threadIdx.x / WAVE;
    const int lane = threadIdx.x % WAVE;
    float s = 0.0f;
    for (long i = (long)blockIdx.x * BLOCK + threadIdx.x; i < n;
         i += (long)gridDim.x * BLOCK)
        s += x[i] * x[i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        s += __shfl_down(s, off, WAVE);
    if (lane == 0) part[wave] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.0f;
        for (int w = 0; w < WAVES_PER_BLOCK; ++w) t += part[w];
        partials[blockIdx.x] = t;
        if (blockIdx.x == 0) step_t[0] += 1.0f;
    }
}

__global__ void __launch_bounds__(BLOCK)
flat_adam_partials_kernel(float* __restrict__ p, float* __restrict__ g,
                          float* __restrict__ m, float* __restrict__ v,
                          const float* __restrict__ step_t,    // [1]
                          const float* __restrict__ partials,  // [nparts]
                          float* __restrict__ normsq,          // [1]
                          int nparts, long numel, float clip, float lr,
                          float b1, float b2, float eps) {
    __shared__ float sp[SUMSQ_MAX_BLOCKS];
    __shared__ float ssum;
    for (int k = threadIdx.x; k < nparts; k += BLOCK) sp[k] = partials[k];
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.0f;
#pragma unroll 8
        for (int k = 0; k < nparts; ++k) t += sp[k];
        ssum = t;
        if (blockIdx.x == 0) normsq[0] = t;
    }
    __syncthreads();
    const float t = step_t[0];
    float scale = 1.0f;
    if (clip > 0.0f) {
        const float norm = sqrtf(ssum);
        const float c = clip / (norm + 1e-6f);
        scale = fminf(c, 1.0f);
    }
    const float bias1 = 1.0f - powf(b1, t);
    const float bias2 = 1.0f - powf(b2, t);
    const float step_size = lr / bias1;
    const float inv_sqrt_bias2 = rsqrtf(bias2);
    const long i0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long stride = (long)gridDim.x * blockDim.x;
    for (long i = i0; i < numel; i += stride) {
        const float gi = g[i] * scale;
        const float mi = b1 * m[i] + (1.0f - b1) * gi;
        const float vi = b2 * v[i] + (1.0f - b2) * gi * gi;
        m[i] = mi;
        v[i] = vi;
        p[i] -= step_size * mi / (sqrtf(vi) * inv_sqrt_bias2 + eps);
        g[i] = 0.0f;
    }
}

void flat_sumsq_adam(torch::Tensor p, torch::Tensor g, torch::Tensor m,
                     torch::Tensor v, torch::Tensor step_t,
                     torch::Tensor normsq, torch::Tensor partials,
                     double clip, double lr, double b1, double b2,
                     double eps) {
    const long numel = p.numel();
    TORCH_CHECK(g.numel() == numel && m.numel() == numel
                && v.numel() == numel, "flat_sumsq_adam: size mismatch");
    long sblocks = (numel + BLOCK - 1) / BLOCK;
    if (sblocks > SUMSQ_MAX_BLOCKS) sblocks = SUMSQ_MAX_BLOCKS;
    TORCH_CHECK(partials.numel() >= sblocks,
                "flat_sumsq_adam: partials buffer holds ", partials.numel(),
                " floats, needs ", sblocks);
    if (numel == 0) return;
    hipStream_t stream = at::cuda::getCurrentCUDAStream();
    hipLaunchKernelGGL(sumsq_partials_kernel, dim3((int)sblocks), dim3(BLOCK),
                       0, stream, g.data_ptr<float>(),
                       partials.data_ptr<float>(), step_t.data_ptr<float>(),
                       numel);
    long blocks = (numel + BLOCK - 1) / BLOCK;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(flat_adam_partials_kernel, dim3((int)blocks),
                       dim3(BLOCK), 0, stream, p.data_ptr<float>(),
                       g.data_ptr<float>(), m.data_ptr<float>(),
                       v.data_ptr<float>(), step_t.data_ptr<float>(),
                       partials.data_ptr<float>(), normsq.data_ptr<float>(),
                       (int)sblocks, numel, (float)clip, (float)lr, (float)b1,
                       (float)b2, (float)eps);
}

// number of partials flat_sumsq_adam writes for a buffer of numel floats
int64_t flat_sumsq_blocks(int64_t numel) {
    long sblocks = (numel + BLOCK - 1) / BLOCK;
    return sblocks > SUMSQ_MAX_BLOCKS ? SUMSQ_MAX_BLOCKS : sblocks;
}

// ---------------------------------------------------------------------------
// The optimiser tail with the row-split weight-grad reduce folded in.
// cached_step_bwd can leave the six row jobs' partial sums in wg_scratch
// (cs_bwd_w_reduce's launch goes away); K1 below then forms each of those
// gradient elements itself: thread i of sumsq_partials' grid looks flat index
// i up in the segment table (passed by value), and if it lies in a row-job
// segment adds the nsplit partials from 0 in split order — the sequence
// cs_bwd_w_reduce_kernel runs — stores flat_g[i] and squares it in
// sumsq_partials' own chain.  K2 is flat_adam_partials, unchanged.
//
// Contraction is off from here on and the roundings are written out as the
// gfx950 ISA of the two kernels this one replaces has them: the reduce is
// plain adds (it has no products), and sumsq's per-thread chain is one fused
// multiply-add per element, s = fma(x, x, s); the wave and block sums are
// plain adds.
#pragma clang fp contract(off)

#define FOLD_MAX_SEGS 24
#define FOLD_NSPLIT 16

struct FoldSegs {
    int nseg;
    int stride;                  // floats between two splits of one job
    int start[FOLD_MAX_SEGS];    // first flat index of the segment
    int len[FOLD_MAX_SEGS];
    int soff[FOLD_MAX_SEGS];     // split 0's offset of the segment in scratch
};

__global__ void __launch_bounds__(BLOCK)
sumsq_partials_folded_kernel(float* __restrict__ g,
                             const float* __restrict__ scratch, FoldSegs S,
                             float* __restrict__ partials, float* step_t,
                             long n) {
    __shared__ float part[WAVES_PER_BLOCK];
    const int wave = threadIdx.x / WAVE;
    const int lane = threadIdx.x % WAVE;
    float s = 0.0f;
    for (long i = (long)blockIdx.x * BLOCK + threadIdx.x; i < n;
         i += (long)gridDim.x * BLOCK) {
        long so = -1;
        for (int q = 0; q < S.nseg; ++q) {
            const long d = i - S.start[q];
            if (d >= 0 && d < S.len[q]) so = S.soff[q] + d;
        }
        float x;
        if (so >= 0) {
            float pv[FOLD_NSPLIT];
#pragma unroll
            for (int k = 0; k < FOLD_NSPLIT; ++k)
                pv[k] = scratch[so + (long)k * S.stride];
            float a = 0.0f;
#pragma unroll
            for (int k = 0; k < FOLD_NSPLIT; ++k) a = a + pv[k];
            g[i] = a;
            x = a;
        } else {
            x = g[i];
        }
        s = __builtin_fmaf(x, x, s);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        s = s + __shfl_down(s, off, WAVE);
    if (lane == 0) part[wave] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.0f;
        for (int w = 0; w < WAVES_PER_BLOCK; ++w) t = t + part[w];
        partials[blockIdx.x] = t;
        if (blockIdx.x == 0) step_t[0] = step_t[0] + 1.0f;
    }
}

// segs = nseg x (flat start, length, scratch offset of split 0), as
// cached_step_fold_segments() returns them; host data, so nothing is read
// from the device while a graph is being captured
void flat_sumsq_adam_folded(torch::Tensor p, torch::Tensor g, torch::Tensor m,
                            torch::Tensor v, torch::Tensor step_t,
                            torch::Tensor normsq, torch::Tensor partials,
                            torch::Tensor scratch, std::vector<int64_t> segs,
                            int64_t nsplit, int64_t stride, double clip,
                            double lr, double b1, double b2, double eps) {
    const long numel = p.numel();
    TORCH_CHECK(g.numel() == numel && m.numel() == numel
                && v.numel() == numel,
                "flat_sumsq_adam_folded: size mismatch");
    TORCH_CHECK(scratch.is_cuda() && scratch.is_contiguous()
                && scratch.scalar_type() == torch::kFloat32
                && scratch.device() == g.device(),
                "flat_sumsq_adam_folded: scratch must be a contiguous f32 "
                "tensor on the gradient's device");
    TORCH_CHECK(nsplit == FOLD_NSPLIT, "flat_sumsq_adam_folded: compiled for ",
                FOLD_NSPLIT, " splits, got ", nsplit);
    TORCH_CHECK(segs.size() % 3 == 0
                && segs.size() / 3 <= (size_t)FOLD_MAX_SEGS,
                "flat_sumsq_adam_folded: at most ", FOLD_MAX_SEGS,
                " (start, len, offset) segments");
    TORCH_CHECK(stride > 0 && stride < (1L << 30) && numel < (1L << 31),
                "flat_sumsq_adam_folded: stride / numel out of range");
    FoldSegs S;
    memset(&S, 0, sizeof(S));
    S.nseg = (int)(segs.size() / 3);
    S.stride = (int)stride;
    for (int q = 0; q < S.nseg; ++q) {
        const int64_t st = segs[3 * q], ln = segs[3 * q + 1],
                      so = segs[3 * q + 2];
        TORCH_CHECK(st >= 0 && ln >= 0 && st + ln <= numel,
                    "flat_sumsq_adam_folded: segment ", q,
                    " outside the flat buffer");
        TORCH_CHECK(so >= 0
                    && so + (nsplit - 1) * stride + ln <= scratch.numel(),
                    "flat_sumsq_adam_folded: segment ", q,
                    " outside the scratch buffer");
        S.start[q] = (int)st;
        S.len[q] = (int)ln;
        S.soff[q] = (int)so;
    }
    long sblocks = (numel + BLOCK - 1) / BLOCK;
    if (sblocks > SUMSQ_MAX_BLOCKS) sblocks = SUMSQ_MAX_BLOCKS;
    TORCH_CHECK(partials.numel() >= sblocks,
                "flat_sumsq_adam_folded: partials buffer holds ",
                partials.numel(), " floats, needs ", sblocks);
    if (numel == 0) return;
    hipStream_t stream = at::cuda::getCurrentCUDAStream();
    hipLaunchKernelGGL(sumsq_partials_folded_kernel, dim3((int)sblocks),
                       dim3(BLOCK), 0, stream, g.data_ptr<float>(),
                       scratch.data_ptr<float>(), S,
                       partials.data_ptr<float>(), step_t.data_ptr<float>(),
                       numel);
    long blocks = (numel + BLOCK - 1) / BLOCK;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(flat_adam_partials_kernel, dim3((int)blocks),
                       dim3(BLOCK), 0, stream, p.data_ptr<float>(),
                       g.data_ptr<float>(), m.data_ptr<float>(),
                       v.data_ptr<float>(), step_t.data_ptr<float>(),
                       partials.data_ptr<float>(), normsq.data_ptr<float>(),
                       (int)sblocks, numel, (float)clip, (float)lr, (float)b1,
                       (float)b2, (float)eps);
}
