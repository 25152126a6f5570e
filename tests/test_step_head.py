"""The two longest launches of the cached PPO step with shorter chains
(ops/hip/cached_step.hip, ``DDLS_AMD_STEP_HEAD``, default on) against the
kernels they replace, which ``DDLS_AMD_STEP_HEAD=off`` launches:

  ``cs_head2_kernel``          the per-sample chain with one sample a block
                               on min(B, 128) blocks, every per-sample input
                               loaded at the top of a chunk and the gfinal
                               phase fed by 16-byte LDS reads, in place of
                               ``cs_head_kernel`` (4 samples a block on
                               min(B, 32) blocks)
  ``cs_bwd_pool_wfc2_kernel``  one pool block per model (sums only the
                               model's own samples, in sample order), the
                               graph-module block and 64 FC-column blocks of
                               4 columns, all reading transposed LDS tiles
                               16 bytes at a time, in place of
                               ``cs_bwd_pool_wfc_kernel`` (16 FC-column
                               blocks of 16 columns)

As in test_step_overlap.py and test_step_merge.py, one ``fused.run()`` per
mode on the same staged minibatch and EVERY tensor of ``fused.scratch``
compared bit for bit in the order of the C_* enum; ``C_STATS`` alone keeps
its 1e-4 tolerance.

The weight-grad kernel stages 128 sample rows at a time and walks them in
32-row tiles and groups of four samples; the pool role lists a model's samples
64 at a time.  B = 1, 3, 4, 5 (less than a group, a group, a group plus one),
33 (a tile plus one row), 127, 128, 130 (a super-tile less one row, exactly
one, one plus two rows) and 257 (two super-tiles plus one row) cross each of
those boundaries.  For the head kernel B <= 128 is one sample a block (fewer
samples than the 128-block cap), B = 130 two samples in the first blocks and
empty last blocks, B = 257 three in a block and a short last block.
"""
import os

import numpy as np
import pytest
import torch

from tests.test_cached_step_shapes import _stage
from tests.test_row_kernels_lanes import (_assert_same, _engine, _enum_names,
                                          _run, rollouts)  # noqa: F401
from tests.test_step_merge import _replay_three
from tests.test_step_overlap import _idx, _t

_ENV_H = "DDLS_AMD_STEP_HEAD"
_ENV_M = "DDLS_AMD_STEP_MERGE"
_CASES = ([("three_models", b) for b in (1, 3, 4, 5, 33, 127, 128, 130, 257)]
          + [("one_model", 5), ("one_model", 33), ("bench", 128)])
_LANE_CASES = [("three_models", 33), ("three_models", 130), ("bench", 128)]


def _run_env(st, fused, head=None, merge=None, lanes=None):
    """One step under the switches (None: unset, the default)."""
    want = {_ENV_H: head, _ENV_M: merge}
    old = {k: os.environ.pop(k, None) for k in want}
    try:
        for k, v in want.items():
            if v is not None:
                os.environ[k] = v
        return _run(st, fused, None, lanes)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


@pytest.mark.gpu
@pytest.mark.parametrize("set_name,B", _CASES,
                         ids=[f"{s}-B{b}" for s, b in _CASES])
def test_head_matches_parent_launch_bitwise(rollouts, set_name, B):
    ro = rollouts(set_name)
    st, fused = _engine(ro, B)
    _stage(st, ro["data"], _idx(ro, B), 0)
    ref = _run_env(st, fused, head="off")
    assert float(_t(ref, "C_FLAT_G").abs().max()) > 0
    assert float(_t(ref, "C_GH2").abs().max()) > 0
    _assert_same(_run_env(st, fused), ref, f"{set_name} B={B} default vs off")
    _assert_same(_run_env(st, fused, head="on"), ref,
                 f"{set_name} B={B} 'on' vs off")
    # whatever turns the merged launches off turns this off too
    _assert_same(_run_env(st, fused, merge="off"), ref,
                 f"{set_name} B={B} STEP_MERGE=off vs STEP_HEAD=off")


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [8, 32])
@pytest.mark.parametrize("set_name,B", _LANE_CASES,
                         ids=[f"{s}-B{b}" for s, b in _LANE_CASES])
def test_head_matches_at_8_and_32_lanes(rollouts, set_name, B, lanes):
    ro = rollouts(set_name)
    st, fused = _engine(ro, B)
    _stage(st, ro["data"], _idx(ro, B), 0)
    _assert_same(_run_env(st, fused, lanes=lanes),
                 _run_env(st, fused, head="off", lanes=lanes),
                 f"{set_name} B={B} {lanes} lanes, default vs off")


@pytest.mark.gpu
@pytest.mark.parametrize("B", [33, 130])
def test_head_model_without_a_sample(rollouts, B):
    """One model of three has no sample in the minibatch: its pool block's
    member list is empty, and its gpool row and gh2 rows are the oracle's
    zeros."""
    ro = rollouts("three_models")
    obs = ro["data"]["obs"]
    mids = np.array([obs[i].model_id for i in range(len(obs))])
    absent = int(mids[0])
    keep = np.nonzero(mids != absent)[0]
    assert len(keep) > 0
    st, fused = _engine(ro, B)
    _stage(st, ro["data"], keep[np.arange(B) % len(keep)], 0)
    staged = st.d["model_ids"].cpu().numpy()
    assert (staged != absent).all()
    ref = _run_env(st, fused, head="off")
    got = _run_env(st, fused)
    _assert_same(got, ref, "absent model, default vs off")
    nptr = _t(got, "C_MODEL_NPTR").cpu().numpy()
    assert nptr[absent + 1] > nptr[absent]
    assert not bool(_t(got, "C_GPOOL")[absent].any())
    assert not bool(_t(got, "C_GH2")[nptr[absent]:nptr[absent + 1]].any())
    assert bool(_t(got, "C_GPOOL").any()) and bool(_t(got, "C_GH2").any())


@pytest.mark.gpu
def test_head_with_matrix_core_wgrads(rollouts, monkeypatch):
    """DDLS_AMD_WGRAD_MFMA=1 changes the row jobs only: the new head-wgrad
    launch is still the default and still gives the parent's bits."""
    B = 33
    ro = rollouts("three_models")
    st, fused = _engine(ro, B)
    _stage(st, ro["data"], _idx(ro, B), 0)
    monkeypatch.setenv("DDLS_AMD_WGRAD_MFMA", "1")
    ref = _run_env(st, fused, head="off")
    assert float(_t(ref, "C_FLAT_G").abs().max()) > 0
    _assert_same(_run_env(st, fused), ref, "MFMA wgrads, default vs off")


@pytest.mark.gpu
def test_head_data_dependent_branches(rollouts):
    """Both sides of every data-dependent branch of the per-sample chain whose
    outputs this launch reduces: a zero mask entry, a clipped and an unclipped
    sample, a value error above and below the clip, actions 0 and 16."""
    B = 33
    ro = rollouts("three_models")
    st, fused = _engine(ro, B)
    _stage(st, ro["data"], _idx(ro, B), 0)
    first = _run_env(st, fused, head="off")
    lp = _t(first, "C_LP").cpu().numpy()
    values = _t(first, "C_VALUES").cpu().numpy()
    clip, vf_clip = float(fused.fscal[0]), float(fused.fscal[1])
    actions = st.d["actions"].cpu().numpy().copy()
    old_logp = st.d["old_logp"].cpu().numpy().copy()
    adv = st.d["adv"].cpu().numpy().copy()
    vtarg = st.d["vtarg"].cpu().numpy().copy()
    actions[2], actions[3] = 0, 16
    old_logp[:] = lp[np.arange(B), actions]          # ratio 1: unclipped
    old_logp[0] -= 1.0                               # ratio e, adv > 0: clipped
    adv[0] = 1.0
    vtarg[0] = values[0] + 2.0 * np.sqrt(vf_clip) + 1.0
    vtarg[1] = values[1]
    for k, v in (("actions", actions), ("old_logp", old_logp), ("adv", adv),
                 ("vtarg", vtarg)):
        st.d[k].copy_(torch.as_tensor(v))
    ref = _run_env(st, fused, head="off")
    mask = _t(ref, "C_MASK").cpu().numpy()
    a = _t(ref, "C_ACTIONS").cpu().numpy()
    lp_a = _t(ref, "C_LP").cpu().numpy()[np.arange(B), a]
    ratio = np.exp(lp_a - _t(ref, "C_OLD_LOGP").cpu().numpy())
    adv_r = _t(ref, "C_ADV").cpu().numpy()
    clipped = np.clip(ratio, 1 - clip, 1 + clip) * adv_r < ratio * adv_r
    verr2 = (_t(ref, "C_VALUES").cpu().numpy()
             - _t(ref, "C_VTARG").cpu().numpy()) ** 2
    assert (mask == 0).any() and (mask > 0).any()
    assert clipped.any() and (~clipped).any(), ratio
    assert (verr2 > vf_clip).any() and (verr2 < vf_clip).any(), verr2
    assert (a == 0).any() and (a == 16).any()
    assert np.isfinite(_t(ref, "C_FLAT_G").cpu().numpy()).all()
    _assert_same(_run_env(st, fused), ref, "branches, default vs off")


@pytest.mark.gpu
def test_head_no_stale_state_between_minibatches(rollouts):
    """X, a different Y, X again: nothing a block keeps in LDS or registers
    across its super-tiles leaks from Y into X."""
    B = 130
    ro = rollouts("three_models")
    st, fused = _engine(ro, B)
    _stage(st, ro["data"], _idx(ro, B), 0)
    x1 = _run_env(st, fused)
    _stage(st, ro["data"], _idx(ro, B, 37), 1)
    y = _run_env(st, fused)
    assert not torch.equal(_t(x1, "C_FLAT_G"), _t(y, "C_FLAT_G")), \
        "Y must be a different minibatch"
    _stage(st, ro["data"], _idx(ro, B), 0)
    _assert_same(_run_env(st, fused), x1, "X after Y vs X")


@pytest.mark.gpu
def test_captured_step_head_on_and_off(rollouts):
    B = 33
    ro = rollouts("three_models")
    on = _replay_three(ro, B, {_ENV_H: None})
    off = _replay_three(ro, B, {_ENV_H: "off"})
    for st in (on, off):
        assert not st.broken and st.capture_count == 1
        assert float(st.step_t.item()) == 3.0
    assert float(on.flat_m.abs().max()) > 0
    for name in ("flat_p", "flat_m", "flat_v", "step_t"):
        assert torch.equal(getattr(on, name), getattr(off, name)), name


@pytest.mark.gpu
def test_head_switch_rejects_unknown_value(rollouts):
    ro = rollouts("one_model")
    st, fused = _engine(ro, 5)
    _stage(st, ro["data"], np.arange(5), 0)
    with pytest.raises(RuntimeError, match=_ENV_H):
        _run_env(st, fused, head="none")
