"""Fused actor-critic head step of the IMPALA device learner
(ops/hip/impala_head_step.hip, rl/impala.py ``head_step="fused"``) against
``impala_head_step_reference`` in float64."""
import functools
import os

import numpy as np
import pytest
import torch

from tests.test_dqn_head_step import HEAD_NAMES, _hold_to_float64_bound
from tests.test_impala_device import _loss_cfg
from tests.test_vec_engine import make_env, multi_model_files  # noqa: F401

SHAPES = [(1, 1, 2, 1), (2, 3, 17, 2), (5, 13, 17, 5), (9, 29, 32, 3)]
CLIPS = [(1.0, 1.0, 1.0), (0.9, 1.3, 1.1)]
GRADS = ("g_model_emb",) + tuple("g_" + n for n in HEAD_NAMES)


@functools.lru_cache(maxsize=None)
def _case(T, N, A, M, seed):
    """CPU inputs of one step: (gfull, model_ids, actions, behaviour_logp,
    rewards, dones, bootstrap, model_emb, head).  About 20% of the mask is
    zero, never the taken action; action A - 1 is masked in every row and
    never taken (A > 2); no row names model M - 2 (M > 3).  pi/mu of the
    float64 reference spreads evenly over [0.5, 1.63]."""
    from ddls_amd.models.gnn import GNNPolicy
    from ddls_amd.rl.device_actor import head_params
    from ddls_amd.rl.dqn import _heads_functional
    g = torch.Generator(device="cpu").manual_seed(seed)
    R, free = T * N, (A - 1 if A > 2 else A)
    actions = torch.randint(0, free, (R,), generator=g)
    mask = (torch.rand(R, A, generator=g) >= 0.2).float()
    mask[torch.arange(R), actions] = 1.0
    mask[:, free:] = 0.0
    gfull = torch.cat([torch.randn(R, 17, generator=g), mask], dim=1)
    mids = torch.randint(0, M, (R,), generator=g)
    if M > 3:
        mids = torch.where(mids == M - 2, torch.zeros_like(mids), mids)
    emb = torch.randn(M, 16, generator=g) * 2
    torch.manual_seed(seed)
    policy = GNNPolicy(num_actions=A)
    assert policy._fused_head_ok
    head = head_params(policy)
    with torch.no_grad():
        logits, _ = _heads_functional([p.double() for p in head],
                                      emb.double(), gfull.double(), mids)
        logp_a = torch.log_softmax(logits, -1)[torch.arange(R), actions]
    ratio = torch.linspace(0.5, 1.63, R)[torch.randperm(R, generator=g)]
    return (gfull, mids, actions, (logp_a - torch.log(ratio.double())).float(),
            torch.randn(R, generator=g),
            (torch.rand(R, generator=g) < 0.15).float(),
            torch.randn(N, generator=g) * 5, emb, head)


def _evaluate(case, T, N, cfg, dtype, fused=False):
    """{quantity: tensor} of one step: the reference in ``dtype`` or the
    kernels.  A gradient autograd leaves None is reported as zeros."""
    from ddls_amd.rl.impala import (_ImpalaHeadStepFn,
                                    impala_head_step_reference)
    dev = torch.device("cuda:0")
    cast = lambda t: (t.to(dtype) if t.is_floating_point() else t).to(dev)
    data = [cast(t) for t in case[:7]]
    leaves = [cast(t).clone().requires_grad_(True)
              for t in [case[7]] + list(case[8])]
    if fused:
        loss, stats = _ImpalaHeadStepFn.apply(
            *data, leaves[0], T, N, cfg.gamma, cfg.rho_clip, cfg.pg_rho_clip,
            cfg.c_clip, cfg.vf_loss_coeff, cfg.entropy_coeff,
            cfg.vtrace_drop_last_ts, None, *leaves[1:])
    else:
        loss, stats = impala_head_step_reference(*data, leaves[0],
                                                 leaves[1:], T, N, cfg)
    loss.backward()
    res = {"loss": loss.detach(), "stats": stats}
    for name, t in zip(GRADS, leaves):
        res[name] = t.grad if t.grad is not None else torch.zeros_like(t)
    return {k: v.detach().double().cpu() for k, v in res.items()}


def _compare(case, T, N, cfg):
    truth = _evaluate(case, T, N, cfg, torch.float64)
    ref32 = _evaluate(case, T, N, cfg, torch.float32)
    fused = _evaluate(case, T, N, cfg, torch.float32, fused=True)
    assert all(torch.isfinite(v).all() for v in fused.values())
    _hold_to_float64_bound(truth, ref32, fused)
    return fused


def _trainer(jobs_dir, dev, num_envs, seed, **switches):
    from ddls_amd.models.gnn import GNNPolicy
    from ddls_amd.rl.engine_env import EngineVectorEnv
    from ddls_amd.rl.impala import ImpalaConfig, ImpalaTrainer
    torch.manual_seed(4)
    policy = GNNPolicy(num_actions=17)
    venv = EngineVectorEnv(
        lambda: make_env(jobs_dir, "remove_and_repeat", 2, 3000, 15),
        num_envs=num_envs, device=dev, base_seed=seed)
    cfg = ImpalaConfig(train_batch_size=num_envs * 8, learner="device",
                       **switches)
    return ImpalaTrainer(venv, policy, cfg, device=dev)


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
def test_switches_are_checked_and_configured():
    import yaml
    from ddls_amd.rl.impala import ImpalaConfig
    cfg = ImpalaConfig()
    assert cfg.head_step == "torch" and cfg.trunk_step == "torch"
    for key in ("head_step", "trunk_step"):
        with pytest.raises(ValueError):
            ImpalaConfig(**{key: "bogus"})
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "configs", "algo", "impala.yaml")) as f:
        algo = yaml.safe_load(f)
    assert algo["head_step"] == "torch" and algo["trunk_step"] == "torch"


def test_fused_switches_on_cpu_are_the_torch_chain(multi_model_files):
    params = []
    for head_step, trunk_step in (("fused", "fused"), ("fused", "torch"),
                                  ("torch", "torch")):
        tr = _trainer(multi_model_files, torch.device("cpu"), 4, 19,
                      head_step=head_step, trunk_step=trunk_step)
        torch.manual_seed(8)
        st = tr.update(tr.collect_rollout(6))
        assert st["learner"] == 1 and st["head_step"] == 0
        params.append([p.detach().clone() for p in tr.policy.parameters()])
    for other in params[:2]:
        assert all(torch.equal(a, b) for a, b in zip(other, params[2]))


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("clips", CLIPS)
@pytest.mark.parametrize("drop_last", [True, False])
@pytest.mark.parametrize("T,N,A,M", SHAPES)
def test_head_step_matches_float64_reference(T, N, A, M, drop_last, clips):
    fused = _compare(_case(T, N, A, M, 11 * T * N + A), T, N,
                     _loss_cfg(clips=clips, drop_last=drop_last))
    if M > 3:       # the model no row names
        assert torch.count_nonzero(fused["g_model_emb"][M - 2]) == 0
        assert torch.count_nonzero(fused["g_model_emb"]) > 0
    if A > 2:       # the action masked in every row
        assert torch.count_nonzero(fused["g_W2p"][A - 1]) == 0
        assert fused["g_b2p"][A - 1] == 0
        assert torch.count_nonzero(fused["g_W2p"]) > 0


@pytest.mark.gpu
def test_head_step_is_reproducible():
    case, cfg = _case(9, 29, 32, 3, 11 * 261 + 32), _loss_cfg((0.9, 1.3, 1.1))
    a = _evaluate(case, 9, 29, cfg, torch.float32, fused=True)
    b = _evaluate(case, 9, 29, cfg, torch.float32, fused=True)
    assert all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["A=33", "model id=M", "float actions"])
def test_head_step_rejects(what):
    case = list(_case(2, 3, 17, 2, 50))
    if what == "A=33":
        case[0] = torch.cat([case[0], case[0][:, :16]], dim=1).contiguous()
    elif what == "model id=M":
        case[1] = case[1].clone()
        case[1][1] = 2
    else:
        case[2] = case[2].float()
    with pytest.raises(RuntimeError, match="impala_head_step"):
        _evaluate(tuple(case), 2, 3, _loss_cfg(), torch.float32, fused=True)


@pytest.mark.gpu
def test_head_step_on_engine_env_batch(multi_model_files):
    """One device-resident rollout at the environment's reward scale, where
    the loss is of order 1e5."""
    from ddls_amd.rl.device_actor import head_params
    tr = _trainer(multi_model_files, torch.device("cuda:0"), 16, 23)
    data = tr.collect_rollout(8)
    with torch.no_grad():
        emb = tr._policy_model_emb()
    keys = ("gfull_dev", "model_ids_dev", "actions_dev", "logp_dev",
            "rewards_dev", "dones_dev", "bootstrap_dev")
    case = tuple(data[k].cpu() for k in keys) + (
        emb.cpu(), [p.cpu() for p in head_params(tr.policy)])
    _compare(case, 8, 16, tr.config)


@pytest.mark.gpu
def test_trainer_with_fused_head_and_trunk_step(multi_model_files):
    tr = _trainer(multi_model_files, torch.device("cuda:0"), 16, 23,
                  head_step="fused", trunk_step="fused")
    before = [p.detach().clone() for p in tr.policy.parameters()]
    for _ in range(2):
        st = tr.train(num_steps=8)
        assert st["learner"] == st["head_step"] == st["trunk_step"] == 1
        assert all(np.isfinite(v) for v in st.values())
    assert any(not torch.equal(a, b)
               for a, b in zip(before, tr.policy.parameters()))
