"""The fused launches of the cached PPO step (ops/hip/cached_step.hip
``cs_head_kernel``, ``cs_fwd_comb1_mlp2_lanes``, ``cs_bwd_scat2_mlp2_lanes``,
``cs_bwd_scat1_gu1``) and the two-launch optimiser tail
(``flat_sumsq_adam``) against the separate kernels they replace, which
``DDLS_AMD_STEP_FUSION=off`` launches.

Step: ``fused.run()`` once per mode on the same staged minibatch in one
process; EVERY tensor of ``fused.scratch`` is compared bit for bit in the
order of the C_* enum (pipeline order), so the first difference names the
kernel that produced it.  ``C_STATS`` alone is summed with float atomics and
keeps the 1e-4 tolerance of test_cached_step_shapes.py.

``cs_head_kernel`` runs min(B, 32) blocks, each walking a contiguous sample
range 4 samples at a time:
  B = 5    one sample per block
  B = 33   17 blocks of 2, the last one short (1 sample); 15 idle blocks
  B = 128  32 blocks of one full chunk of 4
  B = 130  blocks of 5: a chunk of 4 followed by a chunk of 1
The row folds depend on N and E (model sets of test_row_kernels_lanes.py);
all sets but ``bench`` contain nodes without in-edges, the ``deg == 0``
branch of the combine fold.

Tail: the new binding against ``flat_sumsq`` + ``flat_adam`` on synthetic
flat buffers: one block, the policy's size (138 blocks, a partial last one),
and a size past the 512-block cap where the grid-stride loops take a second
trip.
"""
import os

import numpy as np
import pytest
import torch

from tests.test_cached_step_shapes import _stage
from tests.test_row_kernels_lanes import (_assert_same, _engine, _enum_names,
                                          _run, rollouts)  # noqa: F401

_ENV_F = "DDLS_AMD_STEP_FUSION"
_CASES = [("three_models", 5), ("three_models", 33), ("three_models", 130),
          ("one_model", 5), ("tail_one", 33), ("straddle", 33),
          ("bench", 128)]


def _run_fusion(st, fused, fusion, lanes=None):
    """One step under DDLS_AMD_STEP_FUSION=fusion (None: the default)."""
    old = os.environ.pop(_ENV_F, None)
    try:
        if fusion is not None:
            os.environ[_ENV_F] = fusion
        return _run(st, fused, None, lanes)
    finally:
        os.environ.pop(_ENV_F, None)
        if old is not None:
            os.environ[_ENV_F] = old


def _idx(ro, B, start=0):
    """B sample indices; a rollout shorter than B wraps around."""
    n = len(ro["data"]["obs"])
    return (start + np.arange(B)) % n


@pytest.mark.gpu
@pytest.mark.parametrize("set_name,B", _CASES,
                         ids=[f"{s}-B{b}" for s, b in _CASES])
def test_fused_matches_separate_kernels_bitwise(rollouts, set_name, B):
    ro = rollouts(set_name)
    if set_name != "bench":
        _, indptr = ro["venv"]._models_batch.csr_by_dst()
        assert ((indptr[1:] - indptr[:-1]) == 0).any(), \
            "no node without in-edges"
    st, fused = _engine(ro, B)
    _stage(st, ro["data"], _idx(ro, B), 0)
    ref = _run_fusion(st, fused, "off")
    assert float(ref[_enum_names().index("C_FLAT_G")].abs().max()) > 0
    got = _run_fusion(st, fused, None)
    _assert_same(got, ref, f"{set_name} B={B} fused vs off")
    _assert_same(_run_fusion(st, fused, "on"), ref,
                 f"{set_name} B={B} 'on' vs off")


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [8, 32])
def test_fused_matches_at_other_group_sizes(rollouts, lanes):
    ro = rollouts("three_models")
    st, fused = _engine(ro, 33)
    _stage(st, ro["data"], _idx(ro, 33), 0)
    ref = _run_fusion(st, fused, "off")
    _assert_same(_run_fusion(st, fused, None, lanes), ref,
                 f"three_models B=33 fused at {lanes} lanes vs off")


@pytest.mark.gpu
def test_fused_no_stale_state_between_minibatches(rollouts):
    """X, a different Y, X again: the sample rows a block keeps in LDS and
    registers across its chunks must not leak from Y into X."""
    B = 130
    ro = rollouts("three_models")
    st, fused = _engine(ro, B)
    i_g = _enum_names().index("C_FLAT_G")
    _stage(st, ro["data"], _idx(ro, B), 0)
    x1 = _run_fusion(st, fused, None)
    _stage(st, ro["data"], _idx(ro, B, 37), 1)
    y = _run_fusion(st, fused, None)
    assert not torch.equal(x1[i_g], y[i_g]), "Y must be a different minibatch"
    _stage(st, ro["data"], _idx(ro, B), 0)
    _assert_same(_run_fusion(st, fused, None), x1, "X after Y vs X")


@pytest.mark.gpu
def test_fusion_switch_rejects_unknown_value(rollouts):
    ro = rollouts("one_model")
    st, fused = _engine(ro, 5)
    _stage(st, ro["data"], np.arange(5), 0)
    with pytest.raises(RuntimeError, match=_ENV_F):
        _run_fusion(st, fused, "none")


def test_tail_switch_follows_the_step_switch(monkeypatch):
    from ddls_amd.rl.graph_step import step_fusion_enabled
    monkeypatch.delenv(_ENV_F, raising=False)
    monkeypatch.delenv("DDLS_AMD_ROW_KERNELS", raising=False)
    assert step_fusion_enabled()
    monkeypatch.setenv(_ENV_F, "on")
    assert step_fusion_enabled()
    monkeypatch.setenv(_ENV_F, "off")
    assert not step_fusion_enabled()
    monkeypatch.setenv(_ENV_F, "none")
    with pytest.raises(RuntimeError, match=_ENV_F):
        step_fusion_enabled()
    monkeypatch.delenv(_ENV_F)
    monkeypatch.setenv("DDLS_AMD_ROW_KERNELS", "thread")
    assert not step_fusion_enabled()


# ---------------------------------------------------------------------------
# optimiser tail
# ---------------------------------------------------------------------------
_HYPER = (0.5, 3e-4, 0.9, 0.999, 1e-8)     # clip, lr, b1, b2, eps


def _tail_state(numel, dev, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    p = torch.randn(numel, generator=g).to(dev)
    # three steps' gradients, norm ~0.1: well under the 0.5 clip
    grads = [(torch.randn(numel, generator=g) * (0.1 / numel ** 0.5)).to(dev)
             for _ in range(3)]
    return p, grads


def _tail_run(ext, numel, dev, new):
    p, grads = _tail_state(numel, dev, 5)
    m = torch.zeros(numel, device=dev)
    v = torch.zeros(numel, device=dev)
    g = torch.zeros(numel, device=dev)
    step_t = torch.zeros(1, device=dev)
    normsq = torch.full((1,), -1.0, device=dev)
    nparts = int(ext.flat_sumsq_blocks(numel))
    # stale partials must not matter: nothing is zeroed between steps
    partials = torch.full((nparts,), 7.0, device=dev)
    norms = []
    for gk in grads:
        g.copy_(gk)
        if new:
            ext.flat_sumsq_adam(p, g, m, v, step_t, normsq, partials, *_HYPER)
        else:
            ext.flat_sumsq(g, normsq)
            ext.flat_adam(p, g, m, v, step_t, normsq, *_HYPER)
        torch.cuda.synchronize()
        norms.append(normsq.clone())
        assert float(normsq.item()) < 0.9 * _HYPER[0] ** 2, \
            "case precondition: the grad clip must stay inactive"
        assert not bool(g.any()), "flat_g must be zero after the step"
    return {"p": p, "m": m, "v": v, "step_t": step_t, "norms": norms,
            "nparts": nparts}


@pytest.mark.gpu
@pytest.mark.parametrize("numel", [100, 35201, 140003])
def test_tail_matches_old_pair(numel):
    from ddls_amd import ops as hip_ops
    ext = hip_ops.get_extension(required=True)
    dev = torch.device("cuda:0")
    old = _tail_run(ext, numel, dev, new=False)
    new = _tail_run(ext, numel, dev, new=True)
    again = _tail_run(ext, numel, dev, new=True)
    assert new["nparts"] == min(512, (numel + 255) // 256)
    for name in ("p", "m", "v", "step_t"):
        assert torch.equal(new[name].view(torch.int32),
                           old[name].view(torch.int32)), name
    assert float(new["step_t"].item()) == 3.0
    assert not torch.equal(new["p"], _tail_state(numel, dev, 5)[0])
    bound = new["nparts"] * 2.0 ** -23
    for k in range(3):
        a, b, o = (float(r["norms"][k].item()) for r in (new, again, old))
        print(f"numel {numel} step {k}: normsq new {a!r} old {o!r} "
              f"rel diff {abs(a - o) / o:.3e} (bound {bound:.3e})")
        assert torch.equal(new["norms"][k].view(torch.int32),
                           again["norms"][k].view(torch.int32)), \
            "normsq must be the same bits on two runs"
        assert o > 0 and abs(a - o) <= bound * o
