"""GPU tests for the fused cached step (ops/hip/cached_step.hip) at the
minibatch sizes and model sets where its tiling can go wrong.

The kernels stage operands through LDS in 32-row tiles, walk the head
backward a few samples per block, and map each GNN row onto a group of
lanes, so the cases are: B=5 (less than one tile, fewer samples than
head-backward blocks), B=33 (one full tile plus a one-row tail) and B=128
(the benchmark's tile count), on a three-model batch and a single-model
batch whose row counts are no multiple of the rows per block.  Both
contain source nodes without in-edges (zero-filled combine rows).

Reference: the stepper's own torch-autograd cached branch on the same
staged minibatch; tolerances as in
test_engine_rollout.py::test_fused_cached_step_grads_match_autograd.
"""
import numpy as np
import pytest
import torch

from tests.test_vec_engine import make_env

pytestmark = pytest.mark.gpu

# the models of tests/test_vec_engine.py::multi_model_files
_MODELS = {"m_small": (5, 0, 0.5, 11),
           "m_mid": (8, 2, 1.0, 12),
           "m_big": (11, 3, 1.6, 13)}
_SETS = {"three_models": ("m_small", "m_mid", "m_big"),
         "one_model": ("m_mid",)}
_BATCHES = (5, 33, 128)
_NUM_ENVS, _STEPS = 16, 16          # 256 samples: two disjoint B=128 draws


@pytest.fixture(scope="module", params=sorted(_SETS))
def rollout(request, tmp_path_factory):
    """One engine rollout per model set, shared by every minibatch size."""
    from ddls_amd.models.gnn import GNNPolicy
    from ddls_amd.rl.engine_env import EngineVectorEnv
    from ddls_amd.workloads import generate_model, write_pipedream_txt

    d = tmp_path_factory.mktemp("jobs_" + request.param)
    for name in _SETS[request.param]:
        nn, sk, sc, seed = _MODELS[name]
        nodes, edges = generate_model(name, nn, sk, sc, seed)
        write_pipedream_txt(str(d / f"{name}.txt"), nodes, edges)
    dev = torch.device("cuda:0")
    torch.manual_seed(4)
    policy = GNNPolicy(num_actions=17).to(dev)
    venv = EngineVectorEnv(
        lambda: make_env(str(d), "remove_and_repeat", 2, 4000, 20),
        num_envs=_NUM_ENVS, device=dev, base_seed=31)
    data = venv.rollout(policy, steps=_STEPS)
    mb = venv._models_batch
    assert mb.num_graphs == len(_SETS[request.param])
    _, indptr = mb.csr_by_dst()
    deg = (indptr[1:] - indptr[:-1]).cpu().numpy()
    assert (deg == 0).any(), "no source node without in-edges"
    return {"policy": policy, "venv": venv, "data": data, "dev": dev}


def _stage(st, data, idx, seed):
    obs = data["obs"]
    mb = [obs[i] for i in idx]
    rng = np.random.RandomState(seed)
    n = len(idx)
    st.d["model_ids"].copy_(torch.as_tensor([o.model_id for o in mb],
                                            dtype=torch.int64))
    st.d["gf"].copy_(torch.as_tensor(np.stack([o.graph_features
                                               for o in mb])))
    st.d["mask"].copy_(torch.as_tensor(np.stack([o.action_mask
                                                 for o in mb])))
    st.d["actions"].copy_(torch.as_tensor(data["actions"].reshape(-1)[idx]))
    st.d["old_logp"].copy_(torch.as_tensor(
        data["logp"].reshape(-1)[idx].astype(np.float32)))
    st.d["adv"].copy_(torch.as_tensor(rng.randn(n).astype(np.float32)))
    st.d["vtarg"].copy_(torch.as_tensor(rng.randn(n).astype(np.float32)))


@pytest.fixture(scope="module", params=_BATCHES)
def case(request, rollout):
    """Stage X, run twice, stage Y, run, stage X again, run; then the
    autograd reference on X.  The tests below only compare the results."""
    from ddls_amd.rl.graph_step import CapturedSGDStep, _FusedCachedEngine
    from ddls_amd.rl.ppo import PPOConfig

    B = request.param
    policy, venv, data, dev = (rollout[k] for k in
                               ("policy", "venv", "data", "dev"))
    cfg = PPOConfig(sgd_minibatch_size=B, num_sgd_iter=1)
    opt = torch.optim.Adam(policy.parameters(), lr=cfg.lr)
    st = CapturedSGDStep(policy, opt, cfg, dev,
                         models_batch=venv._models_batch)
    assert _FusedCachedEngine.eligible(policy, st._ext)
    st._alloc(0, 0)
    st._flatten_params()
    st.set_kl_coeff(cfg.kl_coeff)
    fused = _FusedCachedEngine(st, venv._models_batch)
    idx_x = np.arange(B)
    idx_y = np.arange(B, 2 * B)

    def run():
        st.reset_stats()
        fused.run()
        torch.cuda.synchronize()
        return st.flat_g.detach().clone(), st.stats_acc.detach().clone()

    out = {"B": B}
    _stage(st, data, idx_x, 0)
    out["g_x1"], out["stats_x1"] = run()
    out["g_x2"], _ = run()
    _stage(st, data, idx_y, 1)
    out["g_y"], _ = run()
    _stage(st, data, idx_x, 0)
    out["g_x3"], _ = run()

    st._fused_cached = None
    st.flat_g.zero_()
    st.reset_stats()
    st._body_fwd_bwd()
    torch.cuda.synchronize()
    out["g_ref"] = st.flat_g.detach().clone()
    out["stats_ref"] = st.stats_acc.detach().clone()
    return out


def test_grads_match_autograd(case):
    np.testing.assert_allclose(case["stats_x1"].cpu().numpy(),
                               case["stats_ref"].cpu().numpy(), rtol=1e-4,
                               atol=1e-5, err_msg="loss stats")
    g, g_ref = case["g_x1"].cpu().numpy(), case["g_ref"].cpu().numpy()
    assert np.abs(g_ref).max() > 0
    scale = np.abs(g_ref).max()
    np.testing.assert_allclose(g, g_ref, rtol=0,
                               atol=max(scale, 1.0) * 2e-5,
                               err_msg="flat gradients")


def test_rerun_is_bitwise_deterministic(case):
    assert torch.equal(case["g_x1"], case["g_x2"])


def test_no_stale_state_between_minibatches(case):
    """X, then a different Y, then X again: partial tiles or scratch rows
    left over from Y must not reach X's gradients."""
    assert not torch.equal(case["g_x1"], case["g_y"]), \
        "Y must be a different minibatch"
    assert torch.equal(case["g_x1"], case["g_x3"])
