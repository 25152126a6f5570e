"""GPU tests: the lane-parallel GNN row kernels of the fused cached step
(ops/hip/cached_step.hip, ``cs_*_lanes_kernel``) against the thread-per-row
kernels they replace, selected with ``DDLS_AMD_ROW_KERNELS=thread``.

Each case runs ``fused.run()`` once per mode on the same staged minibatch in
one process and compares EVERY tensor of ``fused.scratch`` bit for bit, in
the order of the C_* enum (which is pipeline order: forward activations,
backward rows, flat gradient partials), so the first difference names the
kernel that produced it.  ``C_STATS`` alone is summed with float atomics and
is compared with the tolerance of test_cached_step_shapes.py.

The row kernels depend on the row counts N and E, not on B.  A block holds
256/L rows of one class (node / edge / self rows); L is 16 lanes per row by
default and 32 in the two reduce-module-1 kernels, and DDLS_AMD_ROW_LANES
sets it for all of them (every case below also runs at 8, 16 and 32).  At
16 rows per block:
  three_models  N=48 E=53   several blocks per class, a partial last block
  one_model     N=16 E=19   exactly one full node block
  tail_one      N=18 E=17   N no multiple of 16; the edge class ends in a
                            block with a single row and 15 idle lane groups
  straddle      N=24 E=25   (N+E) mod 16 == 1, N no multiple of 16
  bench         the benchmark's own model set (data/small_graphs), B=128
All but the last contain source nodes without in-edges (f = 0 self rows).
"""
import os
import re

import numpy as np
import pytest
import torch

from tests.test_cached_step_shapes import _MODELS, _stage
from tests.test_vec_engine import make_env

pytestmark = pytest.mark.gpu

_GEN = dict(_MODELS, g_tail=(9, 0, 1.0, 21), g_straddle=(12, 1, 1.0, 22))
_SETS = {"three_models": ("m_small", "m_mid", "m_big"),
         "one_model": ("m_mid",),
         "tail_one": ("g_tail",),
         "straddle": ("g_straddle",),
         "bench": None}
_CASES = [("three_models", 5), ("three_models", 33),
          ("one_model", 5), ("one_model", 33),
          ("tail_one", 33), ("straddle", 33), ("bench", 128)]
_RPB = 16          # rows per block at 16 lanes per row
_ENV = "DDLS_AMD_ROW_KERNELS"
_ENV_L = "DDLS_AMD_ROW_LANES"


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
            assert ((indptr[1:] - indptr[:-1]) == 0).any()
        cache[name] = {"policy": policy, "venv": venv, "data": data,
                       "dev": dev}
        return cache[name]

    return get


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


def _run(st, fused, mode, lanes=None):
    """One fused step under DDLS_AMD_ROW_KERNELS=mode (None: the default)
    and DDLS_AMD_ROW_LANES=lanes; returns a copy of every scratch tensor."""
    want = {_ENV: mode, _ENV_L: None if lanes is None else str(lanes)}
    old = {k: os.environ.pop(k, None) for k in want}
    try:
        for k, v in want.items():
            if v is not None:
                os.environ[k] = v
        st.reset_stats()
        fused.run()
        torch.cuda.synchronize()
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
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


@pytest.mark.parametrize("set_name,B", _CASES,
                         ids=[f"{s}-B{b}" for s, b in _CASES])
def test_lanes_match_thread_per_row_bitwise(rollouts, set_name, B):
    ro = rollouts(set_name)
    st, fused = _engine(ro, B)
    _stage(st, ro["data"], np.arange(B), 0)
    ref = _run(st, fused, "thread")
    assert float(ref[_enum_names().index("C_FLAT_G")].abs().max()) > 0
    got = _run(st, fused, None)
    _assert_same(got, ref, f"{set_name} B={B} lanes vs thread")
    # and the explicit spelling of the default
    _assert_same(_run(st, fused, "lanes"), ref,
                 f"{set_name} B={B} 'lanes' vs thread")


@pytest.mark.parametrize("lanes", [8, 16, 32])
@pytest.mark.parametrize("set_name,B", [("three_models", 33),
                                        ("tail_one", 33), ("straddle", 33),
                                        ("bench", 128)])
def test_every_group_size_matches_bitwise(rollouts, set_name, B, lanes):
    """DDLS_AMD_ROW_LANES=8 / 16 / 32 in every kernel (32 / 16 / 8 rows per
    block; tail_one's 17 edge rows end in a single-row block at each)."""
    ro = rollouts(set_name)
    st, fused = _engine(ro, B)
    _stage(st, ro["data"], np.arange(B), 0)
    ref = _run(st, fused, "thread")
    _assert_same(_run(st, fused, None, lanes), ref,
                 f"{set_name} B={B} {lanes} lanes vs thread")


@pytest.mark.parametrize("set_name", ["three_models", "tail_one"])
def test_lanes_no_stale_state_between_minibatches(rollouts, set_name):
    """X, a different Y, X again on the lane path: staged LDS rows, idle
    lane groups or scratch rows left over from Y must not reach X."""
    B = 33
    ro = rollouts(set_name)
    st, fused = _engine(ro, B)
    i_g = _enum_names().index("C_FLAT_G")
    _stage(st, ro["data"], np.arange(B), 0)
    x1 = _run(st, fused, None)
    _stage(st, ro["data"], np.arange(B, 2 * B), 1)
    y = _run(st, fused, None)
    assert not torch.equal(x1[i_g], y[i_g]), "Y must be a different minibatch"
    _stage(st, ro["data"], np.arange(B), 0)
    x3 = _run(st, fused, None)
    _assert_same(x3, x1, f"{set_name} X after Y vs X")


def test_row_kernel_switch_rejects_unknown_value(rollouts):
    ro = rollouts("one_model")
    st, fused = _engine(ro, 5)
    _stage(st, ro["data"], np.arange(5), 0)
    with pytest.raises(RuntimeError, match="DDLS_AMD_ROW_KERNELS"):
        _run(st, fused, "threads")
