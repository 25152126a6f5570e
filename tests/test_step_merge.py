"""Launches of the cached PPO step merged along row-local dependencies
(ops/hip/cached_step.hip and meanpool_mfma.hip, ``DDLS_AMD_STEP_MERGE``,
default on) against the launch sequence they replace, which
``DDLS_AMD_STEP_MERGE=off`` launches:

  ``cs_fwd_stage_mlp1_red1_lanes_kernel``  the stage role, the round-1 node /
                                           edge modules and the round-1
                                           reduce module in one launch, in
                                           place of ``cs_fwd_stage_mlp1_lanes``
                                           + ``cs_fwd_reduce_lanes<1>``
  ``cs_bwd_scat1_gu1_w_kernel``            the round-1 scatter blocks and the
                                           six row-split weight-grad jobs in
                                           one launch (the N1 / E1 jobs
                                           recompute their gradient rows per
                                           32-row tile), in place of
                                           ``cs_bwd_scat1_gu1`` + ``cs_bwd_w``
  ``sumsq_partials_folded_kernel``         the row-split weight-grad reduce
                                           inside the optimiser tail's first
                                           launch, in place of
                                           ``cs_bwd_w_reduce`` +
                                           ``sumsq_partials``

As in test_step_overlap.py, one ``fused.run()`` per mode on the same staged
minibatch and EVERY tensor of ``fused.scratch`` compared bit for bit in the
order of the C_* enum; ``C_STATS`` alone keeps its 1e-4 tolerance.

A merged first-launch block holds 256/L rows of one class (edge rows, then
self rows), L = 32 by default; every case also runs at 8 and 16 lanes per
row, because the merged staging depends on the rows per block.
"""
import os

import numpy as np
import pytest
import torch

from tests.test_cached_step_shapes import _stage
from tests.test_row_kernels_lanes import (_assert_same, _engine, _enum_names,
                                          _run, rollouts)  # noqa: F401
from tests.test_step_overlap import (_WithStore, _assert_staged_equal, _ctl,
                                     _idx, _staged, _store, _t)
from tests.test_vec_engine import make_env

_ENV_M = "DDLS_AMD_STEP_MERGE"
_ENV_O = "DDLS_AMD_STEP_OVERLAP"
_ENV_F = "DDLS_AMD_STEP_FUSION"
_CASES = [("three_models", 5), ("three_models", 33), ("three_models", 130),
          ("one_model", 33), ("tail_one", 33), ("bench", 128)]
_LANES = (8, 16, 32)


def _run_env(st, fused, merge=None, overlap=None, lanes=None):
    """One step under the switches (None: unset, the default)."""
    want = {_ENV_M: merge, _ENV_O: overlap}
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


def _graph_facts(res):
    """Host-side facts about the staged graph set of one run."""
    N = _t(res, "C_Z0").shape[0]
    E = _t(res, "C_E").shape[0]
    src = _t(res, "C_SRC").cpu().numpy()
    dst = _t(res, "C_DST").cpu().numpy()
    nptr = _t(res, "C_MODEL_NPTR").cpu().numpy()
    return {"N": N, "E": E,
            "no_in": bool((np.bincount(dst, minlength=N) == 0).any()),
            "no_out": bool((np.bincount(src, minlength=N) == 0).any()),
            "min_model_n": int((nptr[1:] - nptr[:-1]).min())}


@pytest.mark.gpu
@pytest.mark.parametrize("set_name,B", _CASES,
                         ids=[f"{s}-B{b}" for s, b in _CASES])
def test_merge_matches_separate_launches_bitwise(rollouts, set_name, B):
    ro = rollouts(set_name)
    st, fused = _engine(ro, B)
    _stage(st, ro["data"], _idx(ro, B), 0)
    ref = _run_env(st, fused, merge="off")
    assert float(_t(ref, "C_FLAT_G").abs().max()) > 0
    assert float(_t(ref, "C_WG_SCRATCH").abs().max()) > 0
    facts = _graph_facts(ref)
    print(set_name, facts)
    if set_name == "three_models":
        # a node without in-edges (f = 0 self row), a node without out-edges
        # (it is no edge block's src), and a model smaller than a block's
        # rows at 8 lanes per row
        assert facts["no_in"] and facts["no_out"], facts
        assert facts["min_model_n"] < 256 // 8, facts
    if set_name == "tail_one":
        # partial last blocks of both classes at every group size
        assert facts["N"] % 8 != 0 and facts["E"] % 8 != 0, facts
    _assert_same(_run_env(st, fused), ref, f"{set_name} B={B} default vs off")
    _assert_same(_run_env(st, fused, merge="on"), ref,
                 f"{set_name} B={B} 'on' vs off")
    for lanes in _LANES:
        _assert_same(_run_env(st, fused, lanes=lanes),
                     _run_env(st, fused, merge="off", lanes=lanes),
                     f"{set_name} B={B} {lanes} lanes, default vs off")
    # whatever turns the overlap launches off turns the merge off too
    _assert_same(_run_env(st, fused, overlap="off"), ref,
                 f"{set_name} B={B} STEP_OVERLAP=off vs STEP_MERGE=off")


@pytest.fixture(scope="module")
def medium_rollout(tmp_path_factory):
    """data/medium_graphs plus the two smallest graphs of data/small_graphs:
    more than 512 edge rows but not more than 512 node rows, so a split of
    the edge-row weight-grad jobs walks two 32-row tiles while the node-row
    jobs walk one, and the merged first launch has 60+ blocks per class."""
    import shutil
    from ddls_amd.models.gnn import GNNPolicy
    from ddls_amd.rl.engine_env import EngineVectorEnv
    here = os.path.dirname(os.path.abspath(__file__))
    data = os.path.join(here, "..", "data")
    d = tmp_path_factory.mktemp("jobs_medium")
    for sub, name in (("medium_graphs", "synth_bert.txt"),
                      ("medium_graphs", "synth_resnet152.txt"),
                      ("medium_graphs", "synth_wideresnet.txt"),
                      ("small_graphs", "synth_alexnet.txt"),
                      ("small_graphs", "synth_squeezenet.txt")):
        shutil.copy(os.path.join(data, sub, name), str(d / name))
    dev = torch.device("cuda:0")
    torch.manual_seed(4)
    policy = GNNPolicy(num_actions=17).to(dev)
    venv = EngineVectorEnv(
        lambda: make_env(str(d), "remove_and_repeat", 2, 4000, 20),
        num_envs=8, device=dev, base_seed=31)
    data = venv.rollout(policy, steps=5)
    return {"policy": policy, "venv": venv, "data": data, "dev": dev}


@pytest.mark.gpu
def test_merge_matches_with_more_than_512_edges(medium_rollout):
    B = 33
    ro = medium_rollout
    st, fused = _engine(ro, B)
    _stage(st, ro["data"], _idx(ro, B), 0)
    ref = _run_env(st, fused, merge="off")
    facts = _graph_facts(ref)
    print("medium", facts)
    assert facts["N"] <= 512 < facts["E"], facts
    assert float(_t(ref, "C_FLAT_G").abs().max()) > 0
    _assert_same(_run_env(st, fused), ref, "medium graphs, default vs off")
    _assert_same(_run_env(st, fused, lanes=8),
                 _run_env(st, fused, merge="off", lanes=8),
                 "medium graphs, 8 lanes, default vs off")


@pytest.mark.gpu
def test_merge_with_matrix_core_wgrads(rollouts, monkeypatch):
    """DDLS_AMD_WGRAD_MFMA=1 has no row-split partials: the first launch is
    still the merged one, and no reduce can be deferred."""
    B = 33
    ro = rollouts("three_models")
    st, fused = _engine(ro, B)
    _stage(st, ro["data"], _idx(ro, B), 0)
    assert st._ext.cached_step_reduce_deferred(True)
    monkeypatch.setenv("DDLS_AMD_WGRAD_MFMA", "1")
    assert not st._ext.cached_step_reduce_deferred(True)
    ref = _run_env(st, fused, merge="off")
    assert float(_t(ref, "C_FLAT_G").abs().max()) > 0
    _assert_same(_run_env(st, fused), ref, "MFMA wgrads, default vs off")


@pytest.mark.gpu
def test_merge_no_stale_state_between_minibatches(rollouts):
    B = 33
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
# stage role of the merged first launch
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("B", [5, 33])
def test_stage_role_of_merged_launch_matches_stage_kernel(rollouts, B):
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
    for k in range(3):              # block 0 of the merged launch
        got = _run_env(st, staged)
        assert _ctl(store) == (k + 1, 0)
        _assert_same(got, refs[k], f"B={B} minibatch {k} staged in-launch")
    store.reset()
    for k in range(3):              # block 0 of the round-7 first launch
        got = _run_env(st, staged, merge="off")
        assert _ctl(store) == (k + 1, 0)
        _assert_same(got, refs[k], f"B={B} minibatch {k}, STEP_MERGE=off")
    store.check_err()


@pytest.mark.gpu
def test_stage_role_of_merged_launch_guards(rollouts):
    B = 33
    ro = rollouts("three_models")
    st, fused = _engine(ro, B)
    store, n = _store(ro, B)
    staged = _WithStore(fused, store)
    before = _staged(_run_env(st, staged))          # minibatch 0 staged
    assert _ctl(store) == (1, 0)

    store.set_bypass()
    res = _run_env(st, staged)
    assert _ctl(store) == (store.BYPASS, 0)
    _assert_staged_equal(res, before, "bypass")

    store.reset()
    store.perm[3].copy_(store.perm[1])
    store.cursor.fill_(3)
    res = _run_env(st, staged)
    assert _ctl(store) == (3, 1)
    _assert_staged_equal(res, before, "cursor past the table")

    store.reset()
    store.cursor.fill_(1)
    store.perm[1, B - 1] = n
    res = _run_env(st, staged)
    assert _ctl(store) == (1, 2)
    _assert_staged_equal(res, before, "index == n_rows")


# ---------------------------------------------------------------------------
# the reduce folded into the optimiser tail
# ---------------------------------------------------------------------------
def _tail_state(st):
    return {k: getattr(st, k).detach().clone()
            for k in ("flat_p", "flat_m", "flat_v", "flat_g", "step_t",
                      "normsq", "normsq_partials")}


@pytest.mark.gpu
@pytest.mark.parametrize("clip_rel", [0.5, 2.0], ids=["clipped", "unclipped"])
def test_folded_tail_matches_reduce_then_tail(rollouts, clip_rel):
    """cs_bwd_w_reduce + flat_sumsq_adam against the deferred reduce + the
    folded tail, from the same parameters and Adam state.  flat_m and the
    block partials pin every gradient element."""
    B = 33
    ro = rollouts("three_models")
    st, fused = _engine(ro, B)
    ext = st._ext
    _stage(st, ro["data"], _idx(ro, B), 0)
    g = torch.Generator(device="cpu").manual_seed(5)
    st.flat_m.copy_(torch.randn(st.flat_m.shape, generator=g) * 1e-3)
    st.flat_v.copy_(torch.rand(st.flat_v.shape, generator=g) * 1e-4)
    st.step_t.fill_(3.0)
    start = _tail_state(st)

    def restore():
        for k in ("flat_p", "flat_m", "flat_v", "step_t"):
            getattr(st, k).copy_(start[k])
        st.flat_g.zero_()
        st.normsq.zero_()
        st.normsq_partials.fill_(-1.0)

    restore()
    fused.run()
    torch.cuda.synchronize()
    g_ref = st.flat_g.detach().clone()
    norm = float(g_ref.double().pow(2).sum().sqrt())
    assert norm > 0
    clip = clip_rel * norm
    hyper = (clip, 1e-3, 0.9, 0.999, 1e-8)
    ext.flat_sumsq_adam(st.flat_p, st.flat_g, st.flat_m, st.flat_v,
                        st.step_t, st.normsq, st.normsq_partials, *hyper)
    torch.cuda.synchronize()
    ref = _tail_state(st)
    assert not torch.equal(ref["flat_p"], start["flat_p"])
    assert (float(ref["normsq"]) > clip * clip) == (clip_rel < 1.0)

    restore()
    fused.run(defer_reduce=True)
    torch.cuda.synchronize()
    segs, nsplit, stride = fused.fold_segments()
    assert len(segs) == 3 * 24
    seg_elems = sum(segs[1::3])
    # the deferred step left the row jobs' segments of flat_g untouched
    idx = torch.cat([torch.arange(s, s + n) for s, n in
                     zip(segs[0::3], segs[1::3])]).to(st.flat_g.device)
    assert idx.numel() == seg_elems and idx.unique().numel() == seg_elems
    assert not bool(st.flat_g[idx].any())
    assert bool(g_ref[idx].any())
    ext.flat_sumsq_adam_folded(st.flat_p, st.flat_g, st.flat_m, st.flat_v,
                               st.step_t, st.normsq, st.normsq_partials,
                               fused.scratch[-1], segs, nsplit, stride,
                               *hyper)
    torch.cuda.synchronize()
    got = _tail_state(st)
    for k in ref:
        assert torch.equal(got[k].view(torch.int32),
                           ref[k].view(torch.int32)), k
    assert not bool(got["flat_g"].any())
    assert float(got["step_t"]) == 4.0


@pytest.mark.gpu
def test_bwd_without_defer_argument_leaves_complete_flat_g(rollouts):
    """The distributed path's contract: in merge mode cached_step_bwd called
    as before (no defer argument) ends with cs_bwd_w_reduce."""
    B = 33
    ro = rollouts("three_models")
    st, fused = _engine(ro, B)
    _stage(st, ro["data"], _idx(ro, B), 0)
    ref = _run_env(st, fused, merge="off")
    st.flat_g.zero_()
    st.reset_stats()
    st._ext.cached_step_fwd(fused.scratch, fused.fscal)
    st._ext.cached_step_bwd(fused.scratch, fused.fscal)
    torch.cuda.synchronize()
    assert torch.equal(st.flat_g, _t(ref, "C_FLAT_G"))
    segs, _nsplit, _stride = fused.fold_segments()
    assert all(bool(st.flat_g[s:s + n].any())
               for s, n in zip(segs[0::3], segs[1::3]) if n > 2)


# ---------------------------------------------------------------------------
# captured stepper with a device batch store
# ---------------------------------------------------------------------------
def _replay_three(ro, B, env):
    """A CapturedSGDStep over a bound device store: capture, three replays."""
    from ddls_amd.rl.graph_step import CapturedSGDStep
    from ddls_amd.rl.ppo import PPOConfig
    old = {k: os.environ.pop(k, None) for k in env}
    try:
        for k, v in env.items():
            if v is not None:
                os.environ[k] = v
        torch.manual_seed(4)
        from ddls_amd.models.gnn import GNNPolicy
        policy = GNNPolicy(num_actions=17).to(ro["dev"])
        cfg = PPOConfig(sgd_minibatch_size=B, num_sgd_iter=1, grad_clip=None)
        opt = torch.optim.Adam(policy.parameters(), lr=cfg.lr)
        store, _n = _store(ro, B)
        st = CapturedSGDStep(policy, opt, cfg, ro["dev"],
                             models_batch=ro["venv"]._models_batch,
                             device_store=store)
        st.set_kl_coeff(cfg.kl_coeff)
        assert st.ensure_capacity(0, 0), st.last_error
        assert st._fused_cached is not None
        st.reset_stats()
        for _ in range(3):
            st.replay_next()
        st.read_stats()
        torch.cuda.synchronize()
        assert _ctl(store) == (3, 0)
        return st
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


@pytest.mark.gpu
def test_captured_step_with_store_merge_on_and_off(rollouts):
    B = 33
    ro = rollouts("three_models")
    on = _replay_three(ro, B, {_ENV_M: None, "DDLS_AMD_WGRAD_MFMA": None})
    off = _replay_three(ro, B, {_ENV_M: "off", "DDLS_AMD_WGRAD_MFMA": None})
    mfma = _replay_three(ro, B, {_ENV_M: None, "DDLS_AMD_WGRAD_MFMA": "1"})
    assert on._fold_tail and not off._fold_tail
    assert not mfma._fold_tail, "no deferred reduce without row-split partials"
    for st in (on, off, mfma):
        assert not st.broken and st.capture_count == 1
        assert float(st.step_t.item()) == 3.0
    assert float(on.flat_m.abs().max()) > 0
    for name in ("flat_p", "flat_m", "flat_v", "step_t"):
        assert torch.equal(getattr(on, name), getattr(off, name)), name


# ---------------------------------------------------------------------------
# switch
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_merge_switch_rejects_unknown_value(rollouts):
    ro = rollouts("one_model")
    st, fused = _engine(ro, 5)
    _stage(st, ro["data"], np.arange(5), 0)
    with pytest.raises(RuntimeError, match=_ENV_M):
        _run_env(st, fused, merge="none")


def test_python_mirror_follows_the_four_switches(monkeypatch):
    from ddls_amd.rl.graph_step import step_merge_enabled
    for k in (_ENV_M, _ENV_O, _ENV_F, "DDLS_AMD_ROW_KERNELS"):
        monkeypatch.delenv(k, raising=False)
    assert step_merge_enabled()
    monkeypatch.setenv(_ENV_M, "on")
    assert step_merge_enabled()
    monkeypatch.setenv(_ENV_M, "off")
    assert not step_merge_enabled()
    monkeypatch.setenv(_ENV_M, "none")
    with pytest.raises(RuntimeError, match=_ENV_M):
        step_merge_enabled()
    monkeypatch.setenv(_ENV_M, "on")
    monkeypatch.setenv(_ENV_O, "off")
    assert not step_merge_enabled()
    monkeypatch.delenv(_ENV_O)
    monkeypatch.setenv(_ENV_F, "off")
    assert not step_merge_enabled()
    monkeypatch.delenv(_ENV_F)
    monkeypatch.setenv("DDLS_AMD_ROW_KERNELS", "thread")
    assert not step_merge_enabled()
    monkeypatch.setenv("DDLS_AMD_ROW_KERNELS", "lanes")
    assert step_merge_enabled()
