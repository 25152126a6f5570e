// Prioritized replay on the device ring: a sum tree and a min tree over the
// ring's slots, for gfx950.
//
// State (owned by rl/device_replay.py::DeviceReplay, all in HBM).  P is the
// smallest power of two >= capacity C.  tree_sum and tree_min are f64 [2P];
// the leaf of slot s is node P + s, node i holds tree_sum[2i] + tree_sum[2i+1]
// (tree_min: fmin of the two), node 1 is the root and node 0 is unused.
// Empty and padding leaves hold 0 in the sum tree and +inf in the min tree.
// max_prio is f64 [1], the largest priority |td| + eps seen so far (1.0 at
// the start).
//
//   per_ingest_kernel  one block: the slots a fragment just wrote get
//                      pow(max_prio, alpha) in both trees, then their
//                      ancestors are recomputed level by level
//   per_sample_kernel  multi-block, read-only, one thread per draw: descent
//                      from the root by prefix mass, importance weight
//   per_update_kernel  one block: new leaves pow(|td| + eps, alpha) for a
//                      minibatch's slots (last occurrence of a slot wins),
//                      ancestors level by level, max_prio folded by a block
//                      reduction
//
// Bit contract.  Every internal node is the singly rounded f64 sum (the
// fmin) of its two children, so the tree is a pure function of its leaves
// and numpy rebuilds it bit for bit (SumTreeReference).  All arithmetic on
// tree values is f64 with FMA contraction off.  Both trees are written only
// by the two single-block kernels, on the current stream: levels are
// separated by __syncthreads() and nothing is handed from one workgroup to
// another inside a launch.  No float atomics.
//
// Descent guard.  From node 1: go left if mass < left || right == 0.0, else
// mass -= left and go right.  Without the right == 0 test, u = 1 - 2^-53 or
// the rounding of the subtractions can leave mass >= left at a node whose
// right subtree is padding.  With it every visited node has a positive sum,
// so the leaf reached is a filled slot.
#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>
#include <cmath>
#include <vector>

#define PER_WAVE 64
#define PER_BLOCK 256
#define PER_WAVES (PER_BLOCK / PER_WAVE)
#define PER_MAX_BATCH 4096

// node i of both trees from its two children
__device__ __forceinline__ void per_refresh_node(double* tree_sum,
                                                 double* tree_min, long i) {
#pragma clang fp contract(off)
    tree_sum[i] = tree_sum[2 * i] + tree_sum[2 * i + 1];
    tree_min[i] = fmin(tree_min[2 * i], tree_min[2 * i + 1]);
}

// Slots [start, start + count) mod C, count <= C.  Range 0 is
// [lo0, hi0], range 1 is [lo1, hi1] (empty when the range does not wrap);
// at level l the touched nodes are (P + lo) >> l .. (P + hi) >> l of each.
__global__ void __launch_bounds__(PER_BLOCK)
per_ingest_kernel(double* tree_sum,                     // [2P]
                  double* tree_min,                     // [2P]
                  const double* __restrict__ max_prio,  // [1]
                  long P, long C, long start, long count, double alpha) {
#pragma clang fp contract(off)
    long lo0, hi0, lo1 = 0, hi1 = -1;
    if (count >= C) {
        lo0 = 0;
        hi0 = C - 1;
    } else if (start + count <= C) {
        lo0 = start;
        hi0 = start + count - 1;
    } else {
        lo0 = start;
        hi0 = C - 1;
        hi1 = start + count - C - 1;
    }
    const double leaf = pow(max_prio[0], alpha);
    for (long s = lo0 + threadIdx.x; s <= hi0; s += PER_BLOCK) {
        tree_sum[P + s] = leaf;
        tree_min[P + s] = leaf;
    }
    for (long s = lo1 + threadIdx.x; s <= hi1; s += PER_BLOCK) {
        tree_sum[P + s] = leaf;
        tree_min[P + s] = leaf;
    }
    long a0 = P + lo0, b0 = P + hi0, a1 = P + lo1, b1 = P + hi1;
    const bool two = hi1 >= lo1;
    for (long width = P; width > 1; width >>= 1) {
        a0 >>= 1;
        b0 >>= 1;
        a1 >>= 1;
        b1 >>= 1;
        __syncthreads();
        for (long i = a0 + threadIdx.x; i <= b0; i += PER_BLOCK)
            per_refresh_node(tree_sum, tree_min, i);
        if (two)
            for (long i = a1 + threadIdx.x; i <= b1; i += PER_BLOCK)
                per_refresh_node(tree_sum, tree_min, i);
    }
}

__global__ void __launch_bounds__(PER_BLOCK)
per_sample_kernel(const double* __restrict__ tree_sum,  // [2P]
                  const double* __restrict__ tree_min,  // [2P]
                  const double* __restrict__ u,         // [n] in [0, 1)
                  long* __restrict__ idx_out,           // [n]
                  float* __restrict__ weight_out,       // [n]
                  long n, long P, double beta) {
#pragma clang fp contract(off)
    const long i = (long)blockIdx.x * PER_BLOCK + threadIdx.x;
    if (i >= n) return;
    double mass = u[i] * tree_sum[1];
    long node = 1;
    while (node < P) {
        const double left = tree_sum[2 * node];
        const double right = tree_sum[2 * node + 1];
        if (mass < left || right == 0.0) {
            node = 2 * node;
        } else {
            mass = mass - left;
            node = 2 * node + 1;
        }
    }
    idx_out[i] = node - P;
    weight_out[i] = (float)pow(tree_min[1] / tree_sum[node], beta);
}

// B <= PER_MAX_BATCH.  A slot outside [0, C) is skipped: it writes nothing
// and takes no part in max_prio.
__global__ void __launch_bounds__(PER_BLOCK)
per_update_kernel(double* tree_sum,                   // [2P]
                  double* tree_min,                   // [2P]
                  double* max_prio,                   // [1]
                  const long* __restrict__ idx,       // [B]
                  const double* __restrict__ td_abs,  // [B]
                  int B, long P, long C, double alpha, double eps) {
#pragma clang fp contract(off)
    __shared__ long slot[PER_MAX_BATCH];
    __shared__ double wave_max[PER_WAVES];
    for (int i = threadIdx.x; i < B; i += PER_BLOCK) {
        const long s = idx[i];
        slot[i] = (s >= 0 && s < C) ? s : -1;
    }
    __syncthreads();
    double pmax = 0.0;
    for (int i = threadIdx.x; i < B; i += PER_BLOCK) {
        const long s = slot[i];
        if (s < 0) continue;
        const double p = td_abs[i] + eps;
        pmax = fmax(pmax, p);
        bool last = true;
        for (int j = i + 1; j < B; ++j)
            if (slot[j] == s) {
                last = false;
                break;
            }
        if (last) {
            const double leaf = pow(p, alpha);
            tree_sum[P + s] = leaf;
            tree_min[P + s] = leaf;
        }
    }
    // a max is the same in any order
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        pmax = fmax(pmax, __shfl_xor(pmax, off, PER_WAVE));
    if (threadIdx.x % PER_WAVE == 0) wave_max[threadIdx.x / PER_WAVE] = pmax;
    for (long width = P, shift = 1; width > 1; width >>= 1, ++shift) {
        __syncthreads();
        for (int i = threadIdx.x; i < B; i += PER_BLOCK) {
            const long s = slot[i];
            if (s >= 0)
                per_refresh_node(tree_sum, tree_min, (P + s) >> shift);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double m = max_prio[0];
        for (int w = 0; w < PER_WAVES; ++w) m = fmax(m, wave_max[w]);
        max_prio[0] = m;
    }
}

static int64_t per_check_state(const torch::Tensor& tree_sum,
                               const torch::Tensor& tree_min,
                               int64_t capacity, const char* name) {
    TORCH_CHECK(capacity >= 1 && capacity <= (1LL << 30), name,
                ": capacity out of range");
    int64_t P = 1;
    while (P < capacity) P *= 2;
    TORCH_CHECK(tree_sum.is_cuda() && tree_sum.dtype() == torch::kFloat64
                && tree_sum.is_contiguous() && tree_sum.numel() == 2 * P,
                name, ": tree_sum must be a contiguous f64 CUDA tensor of ",
                2 * P, " elements");
    TORCH_CHECK(tree_min.is_cuda() && tree_min.dtype() == torch::kFloat64
                && tree_min.is_contiguous() && tree_min.numel() == 2 * P,
                name, ": tree_min must be a contiguous f64 CUDA tensor of ",
                2 * P, " elements");
    return P;
}

static void per_check_f64(const torch::Tensor& t, int64_t numel,
                          const char* name) {
    TORCH_CHECK(t.is_cuda() && t.dtype() == torch::kFloat64
                && t.is_contiguous() && t.numel() == numel,
                name, ": expected a contiguous f64 CUDA tensor of ", numel,
                " elements");
}

// slots [start, start + count) mod capacity enter at pow(max_prio, alpha)
void per_ingest(torch::Tensor tree_sum, torch::Tensor tree_min,
                torch::Tensor max_prio, int64_t start, int64_t count,
                int64_t capacity, double alpha) {
    const int64_t P = per_check_state(tree_sum, tree_min, capacity,
                                      "per_ingest");
    per_check_f64(max_prio, 1, "per_ingest max_prio");
    TORCH_CHECK(start >= 0 && start < capacity,
                "per_ingest: start out of range");
    TORCH_CHECK(count >= 0 && count <= capacity,
                "per_ingest: count out of range");
    TORCH_CHECK(alpha >= 0.0, "per_ingest: alpha must be >= 0");
    if (count == 0) return;
    hipStream_t stream = at::cuda::getCurrentCUDAStream();
    hipLaunchKernelGGL(per_ingest_kernel, dim3(1), dim3(PER_BLOCK), 0, stream,
                       tree_sum.data_ptr<double>(),
                       tree_min.data_ptr<double>(),
                       max_prio.data_ptr<double>(), (long)P, (long)capacity,
                       (long)start, (long)count, alpha);
}

// u f64 [n] in [0, 1) -> {idx int64 [n], weight f32 [n]}
std::vector<torch::Tensor> per_sample(
    torch::Tensor tree_sum, torch::Tensor tree_min, torch::Tensor u,
    int64_t capacity, double beta) {
    const int64_t P = per_check_state(tree_sum, tree_min, capacity,
                                      "per_sample");
    TORCH_CHECK(u.dim() == 1, "per_sample: u must be [n]");
    const int64_t n = u.numel();
    TORCH_CHECK(n >= 1 && n < (1LL << 31), "per_sample: n out of range");
    per_check_f64(u, n, "per_sample u");
    TORCH_CHECK(beta >= 0.0, "per_sample: beta must be >= 0");
    auto idx = torch::empty({n}, u.options().dtype(torch::kInt64));
    auto weight = torch::empty({n}, u.options().dtype(torch::kFloat32));
    hipStream_t stream = at::cuda::getCurrentCUDAStream();
    const int blocks = (int)((n + PER_BLOCK - 1) / PER_BLOCK);
    hipLaunchKernelGGL(per_sample_kernel, dim3(blocks), dim3(PER_BLOCK), 0,
                       stream, tree_sum.data_ptr<double>(),
                       tree_min.data_ptr<double>(), u.data_ptr<double>(),
                       idx.data_ptr<long>(), weight.data_ptr<float>(),
                       (long)n, (long)P, beta);
    return {idx, weight};
}

// leaves of slots idx become pow(td_abs + eps, alpha); max_prio is folded
void per_update(torch::Tensor tree_sum, torch::Tensor tree_min,
                torch::Tensor max_prio, torch::Tensor idx,
                torch::Tensor td_abs, int64_t capacity, double alpha,
                double eps) {
    const int64_t P = per_check_state(tree_sum, tree_min, capacity,
                                      "per_update");
    per_check_f64(max_prio, 1, "per_update max_prio");
    TORCH_CHECK(idx.dim() == 1, "per_update: idx must be [B]");
    const int64_t B = idx.numel();
    TORCH_CHECK(B >= 1 && B <= PER_MAX_BATCH,
                "per_update needs 1 <= B <= 4096 (one workgroup)");
    TORCH_CHECK(idx.is_cuda() && idx.dtype() == torch::kInt64
                && idx.is_contiguous(),
                "per_update idx: expected a contiguous int64 CUDA tensor");
    per_check_f64(td_abs, B, "per_update td_abs");
    TORCH_CHECK(alpha >= 0.0 && eps > 0.0,
                "per_update: alpha must be >= 0 and eps > 0");
    hipStream_t stream = at::cuda::getCurrentCUDAStream();
    hipLaunchKernelGGL(per_update_kernel, dim3(1), dim3(PER_BLOCK), 0, stream,
                       tree_sum.data_ptr<double>(),
                       tree_min.data_ptr<double>(),
                       max_prio.data_ptr<double>(), idx.data_ptr<long>(),
                       td_abs.data_ptr<double>(), (int)B, (long)P,
                       (long)capacity, alpha, eps);
}
