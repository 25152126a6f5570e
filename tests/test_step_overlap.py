"""Work taken off the serial chain of the cached PPO step
(ops/hip/cached_step.hip, ``DDLS_AMD_STEP_OVERLAP``, default on) against the
launch sequence it replaces, which ``DDLS_AMD_STEP_OVERLAP=off`` launches:

  ``cs_bwd_pool_wfc_kernel``          one pool block per model + the
                                      graph-module block + the 16 FC-column
                                      blocks, in place of ``cs_bwd_pool`` and
                                      the 17 B-row blocks of ``cs_bwd_w``
  ``cs_fwd_stage_mlp1_lanes_kernel``  the stage role in block 0 of the first
                                      forward launch (``run(store)``), in
                                      place of ``cs_stage_kernel``'s launch

As in test_step_fusion.py, one ``fused.run()`` per mode on the same staged
minibatch and EVERY tensor of ``fused.scratch`` compared bit for bit in the
order of the C_* enum; ``C_STATS`` alone keeps its 1e-4 tolerance.

The B-row blocks stage the minibatch in super-tiles of 128 rows and walk a
super-tile in 32-row tiles:
  B = 5    one partial tile
  B = 33   a full tile plus a 1-row tile
  B = 128  exactly one super-tile
  B = 130  a super-tile plus a 2-row tail
  B = 160  a super-tile plus one full tile
  B = 257  two super-tiles plus one row
"""
import os

import numpy as np
import pytest
import torch

from tests.test_cached_step_shapes import _stage
from tests.test_row_kernels_lanes import (_assert_same, _engine, _enum_names,
                                          _run, rollouts)  # noqa: F401

_ENV_O = "DDLS_AMD_STEP_OVERLAP"
_ENV_F = "DDLS_AMD_STEP_FUSION"
_CASES = [("three_models", 5), ("three_models", 33), ("three_models", 128),
          ("three_models", 130), ("three_models", 160), ("three_models", 257),
          ("one_model", 33), ("bench", 128)]
_STAGED = ("C_MODEL_IDS", "C_GF", "C_MASK", "C_ACTIONS", "C_OLD_LOGP",
           "C_ADV", "C_VTARG")


class _WithStore:
    """``fused`` whose run() gathers its minibatch from ``store``."""

    def __init__(self, fused, store):
        self._fused, self._store = fused, store
        self.scratch = fused.scratch

    def run(self):
        self._fused.run(self._store)


def _run_env(st, fused, overlap=None, fusion=None, lanes=None):
    """One step under the two switches (None: unset, the default)."""
    want = {_ENV_O: overlap, _ENV_F: fusion}
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


def _idx(ro, B, start=0):
    """B sample indices; a rollout shorter than B wraps around."""
    n = len(ro["data"]["obs"])
    return (start + np.arange(B)) % n


def _t(res, name):
    return res[_enum_names().index(name)]


@pytest.mark.gpu
@pytest.mark.parametrize("set_name,B", _CASES,
                         ids=[f"{s}-B{b}" for s, b in _CASES])
def test_overlap_matches_serial_launches_bitwise(rollouts, set_name, B):
    ro = rollouts(set_name)
    st, fused = _engine(ro, B)
    _stage(st, ro["data"], _idx(ro, B), 0)
    ref = _run_env(st, fused, overlap="off")
    assert float(_t(ref, "C_FLAT_G").abs().max()) > 0
    _assert_same(_run_env(st, fused), ref, f"{set_name} B={B} default vs off")
    _assert_same(_run_env(st, fused, overlap="on"), ref,
                 f"{set_name} B={B} 'on' vs off")
    _assert_same(_run_env(st, fused), _run_env(st, fused, fusion="off"),
                 f"{set_name} B={B} default vs STEP_FUSION=off")


@pytest.mark.gpu
def test_model_without_a_sample(rollouts):
    """One model of three has no sample in the minibatch: its pool block sums
    nothing, and its gpool row and gh2 rows are the oracle's zeros."""
    B = 33
    ro = rollouts("three_models")
    obs = ro["data"]["obs"]
    mids = np.array([obs[i].model_id for i in range(len(obs))])
    absent = int(mids[0])
    keep = np.nonzero(mids != absent)[0]
    assert len(keep) > 0
    st, fused = _engine(ro, B)
    _stage(st, ro["data"], keep[np.arange(B) % len(keep)], 0)
    staged = st.d["model_ids"].cpu().numpy()
    assert (staged != absent).all() and len(np.unique(staged)) >= 1
    ref = _run_env(st, fused, overlap="off")
    got = _run_env(st, fused)
    _assert_same(got, ref, "absent model, default vs off")
    nptr = _t(got, "C_MODEL_NPTR").cpu().numpy()
    assert nptr[absent + 1] > nptr[absent]
    for res in (got, ref):
        assert not bool(_t(res, "C_GPOOL")[absent].any())
        assert not bool(_t(res, "C_GH2")[nptr[absent]:nptr[absent + 1]].any())
    assert bool(_t(got, "C_GPOOL").any()) and bool(_t(got, "C_GH2").any())


@pytest.mark.gpu
def test_overlap_with_matrix_core_wgrads(rollouts, monkeypatch):
    """DDLS_AMD_WGRAD_MFMA=1 runs the six row jobs as one block each, so
    cs_bwd_w is launched with six blocks and no reduce launch follows."""
    B = 33
    ro = rollouts("three_models")
    st, fused = _engine(ro, B)
    _stage(st, ro["data"], _idx(ro, B), 0)
    monkeypatch.setenv("DDLS_AMD_WGRAD_MFMA", "1")
    ref = _run_env(st, fused, overlap="off")
    assert float(_t(ref, "C_FLAT_G").abs().max()) > 0
    _assert_same(_run_env(st, fused), ref, "MFMA wgrads, default vs off")


@pytest.mark.gpu
def test_overlap_no_stale_state_between_minibatches(rollouts):
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


# ---------------------------------------------------------------------------
# stage role of the first forward launch
# ---------------------------------------------------------------------------
def _store(ro, B, starts=(0, 37, 0)):
    """A bound store over the whole rollout; minibatch k is the wrapped index
    run starting at starts[k] (X, a different Y, X again)."""
    from ddls_amd.rl.graph_step import DeviceBatchStore
    data = ro["data"]
    n = len(data["obs"])
    obs = [data["obs"][i] for i in range(n)]
    rng = np.random.RandomState(B)
    gfull = np.stack([o.graph_features for o in obs]).astype(np.float32)
    store = DeviceBatchStore(cap_n=n + 8, cap_mb=len(starts) + 2, B=B,
                             Fg=gfull.shape[1], A=17, device=ro["dev"])
    store.bind(gfull,
               np.array([o.model_id for o in obs], dtype=np.int64),
               data["actions"].reshape(-1).astype(np.int64),
               data["logp"].reshape(-1).astype(np.float32),
               rng.randn(n).astype(np.float32),
               rng.randn(n).astype(np.float32),
               np.stack([_idx(ro, B, s) for s in starts]))
    return store, n


def _ctl(store):
    torch.cuda.synchronize()
    return int(store.cursor.item()), int(store.err.item())


def _staged(res):
    return [_t(res, name).clone() for name in _STAGED]


def _assert_staged_equal(res, before, what):
    for name, b in zip(_STAGED, before):
        assert torch.equal(_t(res, name), b), (what, name)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [5, 33])
def test_stage_role_matches_stage_kernel(rollouts, B):
    ro = rollouts("three_models")
    st, fused = _engine(ro, B)
    store, _n = _store(ro, B)
    staged = _WithStore(fused, store)
    refs = []
    for k in range(3):              # cs_stage_kernel's launch, then the step
        refs.append(_run_env(st, staged, overlap="off"))
        assert _ctl(store) == (k + 1, 0)
    assert not torch.equal(_t(refs[0], "C_GF"), _t(refs[1], "C_GF")), \
        "Y must be a different minibatch"
    store.reset()
    for k in range(3):              # the stage role of the first launch
        got = _run_env(st, staged)
        assert _ctl(store) == (k + 1, 0)
        _assert_same(got, refs[k], f"B={B} minibatch {k} staged in-launch")
    store.check_err()


@pytest.mark.gpu
@pytest.mark.parametrize("B", [5, 33])
def test_stage_role_guards(rollouts, B):
    ro = rollouts("three_models")
    st, fused = _engine(ro, B)
    store, n = _store(ro, B)
    staged = _WithStore(fused, store)
    before = _staged(_run_env(st, staged))          # minibatch 0 staged
    assert _ctl(store) == (1, 0)

    # bypass cursor: nothing is read or written
    store.set_bypass()
    res = _run_env(st, staged)
    assert _ctl(store) == (store.BYPASS, 0)
    _assert_staged_equal(res, before, "bypass")

    # cursor past the table (n_mb = 3 of cap_mb = 5; row 3 holds valid rows)
    store.reset()
    store.perm[3].copy_(store.perm[1])
    store.cursor.fill_(3)
    res = _run_env(st, staged)
    assert _ctl(store) == (3, 1)
    _assert_staged_equal(res, before, "cursor past the table")

    # an index equal to n_rows (< cap_n) in the selected row
    store.reset()
    store.cursor.fill_(1)
    store.perm[1, B - 1] = n
    res = _run_env(st, staged)
    assert _ctl(store) == (1, 2)
    _assert_staged_equal(res, before, "index == n_rows")


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [8, 32])
def test_overlap_matches_at_other_group_sizes(rollouts, lanes):
    """The first forward launch is templated on the lanes per row."""
    B = 33
    ro = rollouts("three_models")
    st, fused = _engine(ro, B)
    store, _n = _store(ro, B)
    staged = _WithStore(fused, store)
    ref = _run_env(st, staged, fusion="off")
    store.reset()
    _assert_same(_run_env(st, staged, lanes=lanes), ref,
                 f"three_models B={B} overlap at {lanes} lanes vs off")
    assert _ctl(store) == (1, 0)


# ---------------------------------------------------------------------------
# switch
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_overlap_switch_rejects_unknown_value(rollouts):
    ro = rollouts("one_model")
    st, fused = _engine(ro, 5)
    _stage(st, ro["data"], np.arange(5), 0)
    with pytest.raises(RuntimeError, match=_ENV_O):
        _run_env(st, fused, overlap="none")


def test_python_mirror_follows_the_three_switches(monkeypatch):
    from ddls_amd.rl.graph_step import step_overlap_enabled
    for k in (_ENV_O, _ENV_F, "DDLS_AMD_ROW_KERNELS"):
        monkeypatch.delenv(k, raising=False)
    assert step_overlap_enabled()
    monkeypatch.setenv(_ENV_O, "on")
    assert step_overlap_enabled()
    monkeypatch.setenv(_ENV_O, "off")
    assert not step_overlap_enabled()
    monkeypatch.setenv(_ENV_O, "none")
    with pytest.raises(RuntimeError, match=_ENV_O):
        step_overlap_enabled()
    monkeypatch.setenv(_ENV_O, "on")
    monkeypatch.setenv(_ENV_F, "off")
    assert not step_overlap_enabled()
    monkeypatch.setenv(_ENV_F, "none")
    with pytest.raises(RuntimeError, match=_ENV_F):
        step_overlap_enabled()
    monkeypatch.delenv(_ENV_F)
    monkeypatch.delenv(_ENV_O)
    monkeypatch.setenv("DDLS_AMD_ROW_KERNELS", "thread")
    assert not step_overlap_enabled()
    monkeypatch.setenv("DDLS_AMD_ROW_KERNELS", "lanes")
    assert step_overlap_enabled()
