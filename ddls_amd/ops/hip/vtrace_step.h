// One timestep of the V-trace recurrence, shared by vtrace_loss.hip and
// impala_head_step.hip.
//
// Bit contract: each f32 add/sub/mul is performed singly and in exactly the
// order rl/impala.py::vtrace_targets evaluates them (no FMA contraction), so
// a scan built on vtrace_step() equals vtrace_targets bit for bit.
#pragma once
#include <hip/hip_runtime.h>

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
