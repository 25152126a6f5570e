"""The two launch sequences of the fused cached PPO step
(ops/hip/cached_step.hip), selected with ``DDLS_AMD_STEP_PATH``:

  production  (default) the lane-parallel, merged launches:
              ``cs_fwd_stage_mlp1_red1_lanes``, ``cs_fwd_comb1_mlp2_lanes``,
              ``cs_fwd_reduce_lanes<2>``, ``cs_fwd_comb2_pool``, ``cs_head2``,
              ``cs_bwd_pool_wfc2``, ``cs_bwd_reduce_lanes<2>``,
              ``cs_bwd_scat2_mlp2_lanes``, ``cs_bwd_reduce_lanes<1>``,
              ``cs_bwd_scat1_gu1_w`` and ``cs_bwd_w_reduce`` (or the folded
              optimiser tail)
  reference   the thread-per-row and separate kernels that
              test_cached_step_shapes.py pins to torch autograd

Step: ``fused.run()`` once per path on the same staged minibatch in one
process; EVERY tensor of ``fused.scratch`` is compared bit for bit in the
order of the C_* enum (which is pipeline order: forward activations, backward
rows, flat gradient partials), so the first difference names the kernel that
produced it.  ``C_STATS`` alone is summed with float atomics and keeps the
1e-4 tolerance of test_cached_step_shapes.py.

Rows.  The row kernels depend on the row counts N and E, not on B.  A
production block holds 256/L rows of one class (node / edge / self rows); L
is 16 lanes per row by default and 32 in the two reduce-module-1 launches,
and DDLS_AMD_ROW_LANES sets it for all of them: every case also runs at 8, 16
and 32 (the reference path has no lanes and is computed once per case).  At
16 rows per block:
  three_models  N=48 E=53   several blocks per class, a partial last block;
                            a node without in-edges (f = 0 self row), a node
                            without out-edges, a model smaller than a block
  one_model     N=16 E=19   exactly one full node block
  tail_one      N=18 E=17   N no multiple of 16; the edge class ends in a
                            block with a single row and 15 idle lane groups
  straddle      N=24 E=25   (N+E) mod 16 == 1, N no multiple of 16
  bench         the benchmark's own model set (data/small_graphs), B=128
  medium        data/medium_graphs + two small graphs: N <= 512 < E
All but ``bench`` contain nodes without in-edges, the ``deg == 0`` branch of
the combine fold.

Samples.  ``cs_head2`` runs one sample a block on min(B, 128) blocks;
``cs_bwd_pool_wfc2`` stages 128 sample rows at a time and walks them in 32-row
tiles and groups of four samples, and its pool role lists a model's samples
64 at a time.  B = 1, 3, 4, 5 (less than a group, a group, a group plus one),
33 (a tile plus one row), 127, 128, 130 (a super-tile less one row, exactly
one, one plus two rows), 160 (a super-tile plus a full tile) and 257 (two
super-tiles plus one row) cross each of those boundaries; for the head kernel
B = 130 is two samples in the first blocks and empty last blocks, B = 257
three in a block and a short last block.

Spellings.  ``DDLS_AMD_ROW_KERNELS=thread`` and ``=off`` in
``DDLS_AMD_STEP_FUSION`` / ``_OVERLAP`` / ``_MERGE`` / ``_HEAD`` used to bring
back the launch sequence one generation older.  Those sequences are gone and
the names are deprecated spellings of ``DDLS_AMD_STEP_PATH=reference``.
test_row_kernels_lanes.py, test_step_fusion.py, test_step_overlap.py,
test_step_merge.py and test_step_head.py still set them; every case and
assertion of theirs about the production path is in this file, in the new
spelling, so they can go without loss when the names do.

Tail: ``flat_sumsq_adam`` against ``flat_sumsq`` + ``flat_adam`` on synthetic
flat buffers (one block, the policy's size with a partial last block, and a
size past the 512-block cap), and the folded tail
(``sumsq_partials_folded_kernel``) against ``cs_bwd_w_reduce`` +
``flat_sumsq_adam``.
"""
import contextlib
import os
import re

import numpy as np
import pytest
import torch

from tests.test_cached_step_shapes import _MODELS, _stage
from tests.test_vec_engine import make_env

_GEN = dict(_MODELS, g_tail=(9, 0, 1.0, 21), g_straddle=(12, 1, 1.0, 22))
_SETS = {"three_models": ("m_small", "m_mid", "m_big"),
         "one_model": ("m_mid",),
         "tail_one": ("g_tail",),
         "straddle": ("g_straddle",),
         "bench": None}
_CASES = ([("three_models", b)
           for b in (1, 3, 4, 5, 33, 127, 128, 130, 160, 257)]
          + [("one_model", 5), ("one_model", 33), ("tail_one", 33),
             ("straddle", 33), ("bench", 128)])
_LANES = (8, 16, 32)
_RPB = 16          # rows per block at 16 lanes per row
_ENV = "DDLS_AMD_STEP_PATH"
_ENV_L = "DDLS_AMD_ROW_LANES"
# (name, production value, reference value): the switch and its deprecated
# spellings, the switches of the launch sequences that were removed
_SPELLINGS = ((_ENV, "production", "reference"),
              ("DDLS_AMD_ROW_KERNELS", "lanes", "thread"),
              ("DDLS_AMD_STEP_FUSION", "on", "off"),
              ("DDLS_AMD_STEP_OVERLAP", "on", "off"),
              ("DDLS_AMD_STEP_MERGE", "on", "off"),
              ("DDLS_AMD_STEP_HEAD", "on", "off"))
_ALL = tuple(n for n, _p, _r in _SPELLINGS)
_STAGED = ("C_MODEL_IDS", "C_GF", "C_MASK", "C_ACTIONS", "C_OLD_LOGP",
           "C_ADV", "C_VTARG")


def _enum_names():
    """The C_* tensor-list enum of cached_step.hip, in order."""
    here = os.path.dirname(os.path.abspath(__file__))
    src = open(os.path.join(here, "..", "ddls_amd", "ops", "hip",
                            "cached_step.hip")).read()
    body = src[src.index("C_Z0 = 0"):src.index("C_NT")]
    body = re.sub(r"//[^\n]*", "", body)
    return [n for n in re.findall(r"C_[A-Z0-9_]+", body)]


@pytest.fixture(scope="module")
def rollouts(tmp_path_factory):
    """One engine rollout per model set, made on first use and shared."""
    from ddls_amd.models.gnn import GNNPolicy
    from ddls_amd.rl.engine_env import EngineVectorEnv
    from ddls_amd.workloads import generate_model, write_pipedream_txt
    cache = {}

    def get(name):
        if name in cache:
            return cache[name]
        if _SETS[name] is None:
            from bench import build_env_fn
            env_fn, num_envs, steps = build_env_fn(), 16, 8
        else:
            d = tmp_path_factory.mktemp("jobs_" + name)
            for m in _SETS[name]:
                nn, sk, sc, seed = _GEN[m]
                nodes, edges = generate_model(m, nn, sk, sc, seed)
                write_pipedream_txt(str(d / f"{m}.txt"), nodes, edges)
            jobs, num_envs, steps = str(d), 16, 5
            env_fn = lambda: make_env(jobs, "remove_and_repeat", 2, 4000, 20)
        dev = torch.device("cuda:0")
        torch.manual_seed(4)
        policy = GNNPolicy(num_actions=17).to(dev)
        venv = EngineVectorEnv(env_fn, num_envs=num_envs, device=dev,
                               base_seed=31)
        data = venv.rollout(policy, steps=steps)
        mb = venv._models_batch
        N, E = mb.z.shape[0], mb.src.shape[0]
        if name == "tail_one":
            assert N % _RPB != 0 and E % _RPB == 1, (N, E)
        if name == "straddle":
            assert N % _RPB != 0 and (N + E) % _RPB == 1, (N, E)
        if name == "bench":
            assert N + E == 417, (N, E)
        else:
            _, indptr = mb.csr_by_dst()
            assert ((indptr[1:] - indptr[:-1]) == 0).any(), \
                "no node without in-edges"
        cache[name] = {"policy": policy, "venv": venv, "data": data,
                       "dev": dev}
        return cache[name]

    return get


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


def _engine(ro, B):
    from ddls_amd.rl.graph_step import CapturedSGDStep, _FusedCachedEngine
    from ddls_amd.rl.ppo import PPOConfig
    policy, venv, dev = ro["policy"], ro["venv"], ro["dev"]
    cfg = PPOConfig(sgd_minibatch_size=B, num_sgd_iter=1)
    opt = torch.optim.Adam(policy.parameters(), lr=cfg.lr)
    st = CapturedSGDStep(policy, opt, cfg, dev,
                         models_batch=venv._models_batch)
    assert _FusedCachedEngine.eligible(policy, st._ext)
    st._alloc(0, 0)
    st._flatten_params()
    st.set_kl_coeff(cfg.kl_coeff)
    return st, _FusedCachedEngine(st, venv._models_batch)


@contextlib.contextmanager
def _environ(want):
    """os.environ with ``want`` applied (None: unset), restored on exit."""
    old = {k: os.environ.pop(k, None) for k in want}
    try:
        for k, v in want.items():
            if v is not None:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _run(st, fused, path=None, lanes=None, env=None):
    """One fused step under DDLS_AMD_STEP_PATH=path (None: the default) and
    DDLS_AMD_ROW_LANES=lanes; returns a copy of every scratch tensor."""
    want = {_ENV: path, _ENV_L: None if lanes is None else str(lanes)}
    want.update(env or {})
    with _environ(want):
        st.reset_stats()
        fused.run()
        torch.cuda.synchronize()
    return [t.detach().clone() for t in fused.scratch]


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _assert_same(a, b, what):
    names = _enum_names()
    assert len(names) == len(a) == len(b)
    i_stats = names.index("C_STATS")
    for i, (x, y) in enumerate(zip(a, b)):
        if i == i_stats:
            np.testing.assert_allclose(x.cpu().numpy(), y.cpu().numpy(),
                                       rtol=1e-4, atol=1e-5,
                                       err_msg=f"{what}: loss stats")
            continue
        if not torch.equal(_bits(x), _bits(y)):
            nbad = int((_bits(x) != _bits(y)).sum())
            diff = (x.double() - y.double()).abs().max().item()
            raise AssertionError(
                f"{what}: first differing tensor is #{i} {names[i]} "
                f"(shape {tuple(x.shape)}, {nbad} elements differ, "
                f"max abs diff {diff:.3e})")


def _idx(ro, B, start=0):
    """B sample indices; a rollout shorter than B wraps around."""
    n = len(ro["data"]["obs"])
    return (start + np.arange(B)) % n


def _t(res, name):
    return res[_enum_names().index(name)]


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


# ---------------------------------------------------------------------------
# whole step, production against reference
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("set_name,B", _CASES,
                         ids=[f"{s}-B{b}" for s, b in _CASES])
def test_production_matches_reference_bitwise(rollouts, set_name, B):
    ro = rollouts(set_name)
    st, fused = _engine(ro, B)
    _stage(st, ro["data"], _idx(ro, B), 0)
    ref = _run(st, fused, "reference")
    assert float(_t(ref, "C_FLAT_G").abs().max()) > 0
    assert float(_t(ref, "C_WG_SCRATCH").abs().max()) > 0
    assert float(_t(ref, "C_GH2").abs().max()) > 0
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
    _assert_same(_run(st, fused), ref, f"{set_name} B={B} default vs reference")
    # and the explicit spelling of the default
    _assert_same(_run(st, fused, "production"), ref,
                 f"{set_name} B={B} 'production' vs reference")
    # 32 / 16 / 8 rows per block; the reference path has no lanes
    for lanes in _LANES:
        _assert_same(_run(st, fused, None, lanes), ref,
                     f"{set_name} B={B} {lanes} lanes vs reference")
    _assert_same(_run(st, fused, "reference", 8), ref,
                 f"{set_name} B={B} reference ignores the lanes")


@pytest.mark.gpu
def test_matches_with_more_than_512_edges(medium_rollout):
    B = 33
    ro = medium_rollout
    st, fused = _engine(ro, B)
    _stage(st, ro["data"], _idx(ro, B), 0)
    ref = _run(st, fused, "reference")
    facts = _graph_facts(ref)
    print("medium", facts)
    assert facts["N"] <= 512 < facts["E"], facts
    assert float(_t(ref, "C_FLAT_G").abs().max()) > 0
    _assert_same(_run(st, fused), ref, "medium graphs, default vs reference")
    _assert_same(_run(st, fused, None, 8), ref,
                 "medium graphs, 8 lanes vs reference")


@pytest.mark.gpu
@pytest.mark.parametrize("B", [33, 130])
def test_model_without_a_sample(rollouts, B):
    """One model of three has no sample in the minibatch: its pool block's
    member list is empty, and its gpool row and gh2 rows are the reference's
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
    assert (staged != absent).all() and len(np.unique(staged)) >= 1
    ref = _run(st, fused, "reference")
    got = _run(st, fused)
    _assert_same(got, ref, "absent model, default vs reference")
    nptr = _t(got, "C_MODEL_NPTR").cpu().numpy()
    assert nptr[absent + 1] > nptr[absent]
    for res in (got, ref):
        assert not bool(_t(res, "C_GPOOL")[absent].any())
        assert not bool(_t(res, "C_GH2")[nptr[absent]:nptr[absent + 1]].any())
    assert bool(_t(got, "C_GPOOL").any()) and bool(_t(got, "C_GH2").any())


@pytest.mark.gpu
def test_head_data_dependent_branches(rollouts):
    """Both sides of every data-dependent branch of the per-sample chain whose
    outputs this launch reduces: a zero mask entry, a clipped and an unclipped
    sample, a value error above and below the clip, actions 0 and 16."""
    B = 33
    ro = rollouts("three_models")
    st, fused = _engine(ro, B)
    _stage(st, ro["data"], _idx(ro, B), 0)
    first = _run(st, fused, "reference")
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
    ref = _run(st, fused, "reference")
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
    _assert_same(_run(st, fused), ref, "branches, default vs reference")


@pytest.mark.gpu
@pytest.mark.parametrize("set_name,B", [("three_models", 33),
                                        ("tail_one", 33),
                                        ("three_models", 130)])
def test_no_stale_state_between_minibatches(rollouts, set_name, B):
    """X, a different Y, X again on the production path: staged LDS rows, idle
    lane groups, the sample rows a block keeps in LDS and registers across
    its chunks and super-tiles, or scratch rows left over from Y must not
    reach X."""
    ro = rollouts(set_name)
    st, fused = _engine(ro, B)
    _stage(st, ro["data"], _idx(ro, B), 0)
    x1 = _run(st, fused)
    _stage(st, ro["data"], _idx(ro, B, 37), 1)
    y = _run(st, fused)
    assert not torch.equal(_t(x1, "C_FLAT_G"), _t(y, "C_FLAT_G")), \
        "Y must be a different minibatch"
    _stage(st, ro["data"], _idx(ro, B), 0)
    _assert_same(_run(st, fused), x1, f"{set_name} B={B} X after Y vs X")


@pytest.mark.gpu
def test_matrix_core_wgrads(rollouts, monkeypatch):
    """DDLS_AMD_WGRAD_MFMA=1 has no row-split partials: the production path
    launches cs_bwd_scat1_gu1 and a six-block cs_bwd_w of their own, no reduce
    can be deferred, and both paths end in the same cs_bwd_w_kernel."""
    B = 33
    ro = rollouts("three_models")
    st, fused = _engine(ro, B)
    _stage(st, ro["data"], _idx(ro, B), 0)
    assert st._ext.cached_step_reduce_deferred(True)
    assert not st._ext.cached_step_reduce_deferred(False)
    with _environ({_ENV: "reference"}):
        assert not st._ext.cached_step_reduce_deferred(True)
    monkeypatch.setenv("DDLS_AMD_WGRAD_MFMA", "1")
    assert not st._ext.cached_step_reduce_deferred(True)
    ref = _run(st, fused, "reference")
    assert float(_t(ref, "C_FLAT_G").abs().max()) > 0
    _assert_same(_run(st, fused), ref, "MFMA wgrads, default vs reference")


# ---------------------------------------------------------------------------
# stage role of the first forward launch
# ---------------------------------------------------------------------------
class _WithStore:
    """``fused`` whose run() gathers its minibatch from ``store``."""

    def __init__(self, fused, store):
        self._fused, self._store = fused, store
        self.scratch = fused.scratch

    def run(self):
        self._fused.run(self._store)


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
        refs.append(_run(st, staged, "reference"))
        assert _ctl(store) == (k + 1, 0)
    assert not torch.equal(_t(refs[0], "C_GF"), _t(refs[1], "C_GF")), \
        "Y must be a different minibatch"
    store.reset()
    for k in range(3):              # block 0 of the first forward launch
        got = _run(st, staged)
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
    before = _staged(_run(st, staged))              # minibatch 0 staged
    assert _ctl(store) == (1, 0)

    # bypass cursor: nothing is read or written
    store.set_bypass()
    res = _run(st, staged)
    assert _ctl(store) == (store.BYPASS, 0)
    _assert_staged_equal(res, before, "bypass")

    # cursor past the table (n_mb = 3 of cap_mb = 5; row 3 holds valid rows)
    store.reset()
    store.perm[3].copy_(store.perm[1])
    store.cursor.fill_(3)
    res = _run(st, staged)
    assert _ctl(store) == (3, 1)
    _assert_staged_equal(res, before, "cursor past the table")

    # an index equal to n_rows (< cap_n) in the selected row
    store.reset()
    store.cursor.fill_(1)
    store.perm[1, B - 1] = n
    res = _run(st, staged)
    assert _ctl(store) == (1, 2)
    _assert_staged_equal(res, before, "index == n_rows")


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [8, 16])
def test_stage_role_at_other_group_sizes(rollouts, lanes):
    """The first forward launch is templated on the lanes per row (32 by
    default)."""
    B = 33
    ro = rollouts("three_models")
    st, fused = _engine(ro, B)
    store, _n = _store(ro, B)
    staged = _WithStore(fused, store)
    ref = _run(st, staged, "reference")
    store.reset()
    _assert_same(_run(st, staged, None, lanes), ref,
                 f"three_models B={B} staged at {lanes} lanes vs reference")
    assert _ctl(store) == (1, 0)


@pytest.mark.gpu
def test_staged_forward_is_production_only(rollouts):
    B = 5
    ro = rollouts("one_model")
    st, fused = _engine(ro, B)
    store, _n = _store(ro, B)
    with _environ({_ENV: "reference"}):
        with pytest.raises(RuntimeError, match="production path only"):
            st._ext.cached_step_fwd_staged(
                fused.scratch, fused.fscal, store.tensors(), store.perm,
                store.cursor, store.err, [store.n_rows, store.n_mb])
    assert _ctl(store) == (0, 0)


# ---------------------------------------------------------------------------
# the reduce folded into the optimiser tail
# ---------------------------------------------------------------------------
def _tail_state_of(st):
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
    start = _tail_state_of(st)

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
    ref = _tail_state_of(st)
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
    got = _tail_state_of(st)
    for k in ref:
        assert torch.equal(got[k].view(torch.int32),
                           ref[k].view(torch.int32)), k
    assert not bool(got["flat_g"].any())
    assert float(got["step_t"]) == 4.0


@pytest.mark.gpu
def test_bwd_without_defer_argument_leaves_complete_flat_g(rollouts):
    """The distributed path's contract: cached_step_bwd called without the
    defer argument ends with cs_bwd_w_reduce on the production path too."""
    B = 33
    ro = rollouts("three_models")
    st, fused = _engine(ro, B)
    _stage(st, ro["data"], _idx(ro, B), 0)
    ref = _run(st, fused, "reference")
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


# ---------------------------------------------------------------------------
# captured stepper with a device batch store
# ---------------------------------------------------------------------------
def _replay_three(ro, B, env):
    """A CapturedSGDStep over a bound device store: capture, three replays."""
    from ddls_amd.rl.graph_step import CapturedSGDStep
    from ddls_amd.rl.ppo import PPOConfig
    with _environ(env):
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


@pytest.mark.gpu
def test_captured_step_with_store_on_both_paths(rollouts):
    B = 33
    ro = rollouts("three_models")
    prod = _replay_three(ro, B, {_ENV: None, "DDLS_AMD_WGRAD_MFMA": None})
    ref = _replay_three(ro, B, {_ENV: "reference",
                                "DDLS_AMD_WGRAD_MFMA": None})
    mfma = _replay_three(ro, B, {_ENV: None, "DDLS_AMD_WGRAD_MFMA": "1"})
    assert prod._fold_tail and not ref._fold_tail
    assert not mfma._fold_tail, "no deferred reduce without row-split partials"
    for st in (prod, ref, mfma):
        assert not st.broken and st.capture_count == 1
        assert float(st.step_t.item()) == 3.0
    assert float(prod.flat_m.abs().max()) > 0
    for name in ("flat_p", "flat_m", "flat_v", "step_t"):
        assert torch.equal(getattr(prod, name), getattr(ref, name)), name


# ---------------------------------------------------------------------------
# switch
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_path_switch_rejects_unknown_value(rollouts):
    ro = rollouts("one_model")
    st, fused = _engine(ro, 5)
    _stage(st, ro["data"], np.arange(5), 0)
    with pytest.raises(RuntimeError, match=_ENV):
        _run(st, fused, "oracle")


@pytest.mark.gpu
def test_every_spelling_selects_the_same_two_paths(rollouts):
    """The paths write the same bits, so the scratch tensors cannot tell which
    one ran; cached_step_reduce_deferred(True) can: false on the reference
    path."""
    ro = rollouts("one_model")
    st, _fused = _engine(ro, 5)
    ext = st._ext
    clear = {k: None for k in _ALL}
    for name, prod, ref in _SPELLINGS:
        for value, deferred in ((prod, True), ("", True), (ref, False)):
            with _environ(dict(clear, **{name: value})):
                assert ext.cached_step_reduce_deferred(True) is deferred, \
                    (name, value)
        # 'reference' from any one of them wins
        with _environ(dict(clear, **{_ENV: "production", name: ref})):
            assert not ext.cached_step_reduce_deferred(True), (name, ref)
        with _environ(dict(clear, **{name: "oracle"})):
            with pytest.raises(RuntimeError, match=name):
                ext.cached_step_reduce_deferred(True)


def test_python_mirror_of_the_path_switch(monkeypatch):
    from ddls_amd.rl.graph_step import (step_fusion_enabled,
                                        step_merge_enabled,
                                        step_overlap_enabled,
                                        step_reference_path)
    for k in _ALL:
        monkeypatch.delenv(k, raising=False)
    assert step_reference_path() is False
    for name, prod, ref in _SPELLINGS:
        for value, want in (("", False), (prod, False), (ref, True)):
            monkeypatch.setenv(name, value)
            assert step_reference_path() is want, (name, value)
            for old in (step_fusion_enabled, step_overlap_enabled,
                        step_merge_enabled):
                assert old() is (not want), (name, value)
        monkeypatch.setenv(name, "oracle")
        with pytest.raises(RuntimeError, match=name):
            step_reference_path()
        monkeypatch.delenv(name)
    monkeypatch.setenv(_ENV, "production")
    monkeypatch.setenv("DDLS_AMD_STEP_HEAD", "off")
    assert step_reference_path() is True
