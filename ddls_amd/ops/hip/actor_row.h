// One row of the device-side actors (actor.hip's contract: lane ownership,
// fmaf chains and orders, Philox counter), as a __device__ function shared by
// actor.hip (one launch per step) and env_rollout.hip (actor + env step, T
// times in one launch, for one policy or for a population of them).  Both callers run the SAME arithmetic, so their rows
// are bit-equal.  The row reads its weights through plain pointers: actor.hip
// passes LDS for the first-layer matrices and global memory for the rest,
// env_rollout.hip passes LDS for all of them.
#pragma once
#include <hip/hip_runtime.h>

#define WAVE 64
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

// what a row reads besides the first-layer matrices; `w2p_ld` is the row
// stride of W2p (H1 in global memory, padded in LDS)
struct ActorHead {
    const float *ln_w, *ln_b, *bg, *b1p, *W2p, *b2p, *b1v, *W2v, *b2v;
    int w2p_ld;
};

// where a row's results go; a null pointer leaves that result unwritten (the
// population rollout keeps none of them)
struct ActorRowOut {
    float *gfull, *lp_all, *logp, *value, *u;
};

// The action of one live row, wave uniform.  The whole wave calls this with
// the same arguments.  `gf` / `mask` are the row's 17 graph features and A
// mask values, `emb` the 16 floats of model_emb[mid]; `w1s` / `wgs` are the
// staged first-layer matrices and `yln` [64+1], `embw` [EMB+1], `h1` [H1] the
// wave's own LDS rows.  `ctr0` is word 0 of the Philox counter (the env row).
template <bool POLICY>
__device__ __forceinline__ int actor_row(
        int lane, unsigned ctr0, const float* gf, const float* mask,
        const float* emb, int k_sched, double seq,
        const double* sch_acc_row, int SCH,
        const float (*w1s)[H1][EMB + 1], const float (*wgs)[64 + 1],
        float* yln, float* embw, float* h1, const ActorHead& W,
        const ActorRowOut& out, int A, int mode, int sip_ml_cap,
        unsigned seed_lo, unsigned seed_hi,
        unsigned step_lo, unsigned step_hi) {
    const int Fg = NGF + A;
    const float mk = (lane < A) ? mask[lane] : 0.0f;
    const unsigned vb = (unsigned)__ballot(lane < A && mk > 0.0f);
    const unsigned x = philox_word0(ctr0, step_lo, step_hi, 0u,
                                    seed_lo, seed_hi);
    const float u = (float)(x >> 8) * 5.9604644775390625e-08f;  // 2^-24

    if constexpr (!POLICY) {
        double acc = 0.0;
        if (mode == ACCEPTABLE_JCT) {
            // an out-of-range schedule slot reads as "never reached"
            acc = (k_sched >= 0 && k_sched < SCH) ? sch_acc_row[k_sched] : 0.0;
        }
        const int a = heuristic_action(mode, vb, A, u, sip_ml_cap, seq, acc);
        if (lane == 0 && mode == RANDOM && out.u != nullptr) out.u[0] = u;
        return a;
    } else {
        // ---- policy head: LN(gf ++ mask) -> graph Linear -> concat ----
        float v = 0.0f;
        if (lane < NGF) v = gf[lane];
        else if (lane < Fg) v = mask[lane - NGF];
        if (out.gfull != nullptr && lane < Fg) out.gfull[lane] = v;
        const float mean = awave_sum(v) / Fg;
        const float d = (lane < Fg) ? v - mean : 0.0f;
        const float var = awave_sum(d * d) / Fg;
        const float inv_sigma = rsqrtf(var + LN_EPS);
        if (lane < Fg)
            yln[lane] = d * inv_sigma * W.ln_w[lane] + W.ln_b[lane];
        __builtin_amdgcn_wave_barrier();
        if (lane < GEMB) {
            float ge = W.bg[lane];
            for (int k = 0; k < Fg; ++k)
                ge = fmaf(wgs[lane][k], yln[k], ge);
            embw[16 + lane] = ge;
        }
        if (lane < 16) embw[lane] = emb[lane];
        __builtin_amdgcn_wave_barrier();

        // policy branch
#pragma unroll
        for (int i = 0; i < H1 / WAVE; ++i) {
            const int j = lane + WAVE * i;
            float a1 = W.b1p[j];
#pragma unroll
            for (int k = 0; k < EMB; ++k)
                a1 = fmaf(w1s[0][j][k], embw[k], a1);
            h1[j] = fmaxf(a1, 0.0f);
        }
        __builtin_amdgcn_wave_barrier();
        float lg = -INFINITY;
        if (lane < A) {
            lg = W.b2p[lane];
            const float* w2row = W.W2p + (long)lane * W.w2p_ld;
            for (int j = 0; j < H1; ++j)
                lg = fmaf(w2row[j], h1[j], lg);
            // torch: logits + clamp(log(mask), min=float32_min)
            lg += (mk > 0.0f) ? logf(mk) : MASK_MIN;
        }
        __builtin_amdgcn_wave_barrier();
        // value branch
#pragma unroll
        for (int i = 0; i < H1 / WAVE; ++i) {
            const int j = lane + WAVE * i;
            float a1 = W.b1v[j];
#pragma unroll
            for (int k = 0; k < EMB; ++k)
                a1 = fmaf(w1s[1][j][k], embw[k], a1);
            h1[j] = fmaxf(a1, 0.0f);
        }
        __builtin_amdgcn_wave_barrier();
        float vp = 0.0f;
#pragma unroll
        for (int i = 0; i < H1 / WAVE; ++i) {
            const int j = lane + WAVE * i;
            vp = fmaf(W.W2v[j], h1[j], vp);
        }
        vp = awave_sum(vp) + W.b2v[0];

        // max-subtracted log-softmax over the A lanes
        const float mx = awave_max(lg);
        const float ex = (lane < A) ? expf(lg - mx) : 0.0f;
        const float lse = logf(awave_sum(ex));
        const float lp = (lane < A) ? lg - mx - lse : -INFINITY;
        if (out.lp_all != nullptr && lane < A) out.lp_all[lane] = lp;

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
            if (out.logp != nullptr) out.logp[0] = lpa;
            if (out.value != nullptr) out.value[0] = vp;
            if (out.u != nullptr) out.u[0] = u;
        }
        __builtin_amdgcn_wave_barrier();
        return act;
    }
}
