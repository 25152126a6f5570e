"""The device learners' one-launch optimiser tail (ops/hip/learner_tail.hip,
rl/learner_tail.py, ``optimizer_step="fused"``) against
``learner_tail_reference`` in float64 under the project's bound; the f32
reference is ``clip_grad_norm_`` + ``torch.optim.Adam``."""
import functools
import os

import numpy as np
import pytest
import torch

from tests.test_dqn_head_step import _hold_to_float64_bound
from tests.test_impala_head_step import _trainer as _impala_trainer
from tests.test_vec_engine import make_env, multi_model_files  # noqa: F401

LR, BETAS, EPS = 1e-2, (0.9, 0.999), 1e-8
LIMIT = 65536           # learner_tail_limits()[1], the one-launch total
STEPS = 3
SIZES = {
    "one": [1],
    "boundaries": [3, 1, 64, 65, 1023, 1025],
    "policy": None,     # the tuned GNNPolicy's 36 tensors
    "64x7": [7] * 64,
    "limit": [40000, 25535, 1],
    "limit+1": [40000, 25535, 2],
    # 49004 quads: 23 full blocks of the two-launch path and one of 1900
    "3xlimit": [100003, 96001, 7],
}
CLIP_MODES = ("active", "inactive", "disabled")


@functools.lru_cache(maxsize=None)
def _case(name):
    """(p0, grads of each step, stats of each step) as f32 CPU tensors, and
    the float64 grad norm of each step."""
    sizes = SIZES[name]
    if sizes is None:
        from ddls_amd.models.gnn import GNNPolicy
        sizes = [p.numel() for p in GNNPolicy(num_actions=17).parameters()]
        assert len(sizes) == 36
    g = torch.Generator(device="cpu").manual_seed(len(sizes) + sum(sizes))
    rand = lambda: [torch.randn(n, generator=g) for n in sizes]
    p0, grads = rand(), [rand() for _ in range(STEPS)]
    stats = [torch.randn(4, generator=g) for _ in range(STEPS)]
    norms = [torch.cat(gs).double().norm().item() for gs in grads]
    return p0, grads, stats, norms


def _max_norm(case, mode):
    norms = case[3]
    return {"active": 0.5 * min(norms), "inactive": 2.0 * max(norms),
            "disabled": 0.0}[mode]


def _run(case, max_norm, zero_grads, dtype, dev, impl):
    """{quantity: f64 CPU tensor} after STEPS steps of ``impl``: "kernel",
    "reference" (learner_tail_reference) or "torch" (clip_grad_norm_ +
    Adam)."""
    from ddls_amd.rl.learner_tail import learner_tail_reference
    p0, grads, stats, _ = case
    put = lambda t: t.to(dtype).to(dev).clone()     # the case stays as it is
    ps = [put(t) for t in p0]
    acc = torch.zeros(4, dtype=dtype, device=dev)
    reports = []
    if impl == "torch":
        ps = [torch.nn.Parameter(p) for p in ps]
        opt = torch.optim.Adam(ps, lr=LR, betas=BETAS, eps=EPS, foreach=True)
        for gs, st in zip(grads, stats):
            for p, g in zip(ps, gs):
                p.grad = put(g)
            norm, clip = torch.zeros((), device=dev), torch.ones((), device=dev)
            if max_norm > 0:
                norm = torch.nn.utils.clip_grad_norm_(ps, max_norm)
                clip = torch.clamp(max_norm / (norm + 1e-6), max=1.0)
            opt.step()
            acc += put(st)
            reports.append(torch.stack([norm, clip]))
        ms = [opt.state[p]["exp_avg"] for p in ps]
        vs = [opt.state[p]["exp_avg_sq"] for p in ps]
    else:
        from ddls_amd import ops as hip_ops
        fn = (hip_ops.get_extension(required=True).learner_tail
              if impl == "kernel" else learner_tail_reference)
        ms, vs = ([torch.zeros_like(p) for p in ps] for _ in range(2))
        step_t = torch.zeros(1, dtype=dtype, device=dev)
        stats_out = torch.zeros(2, dtype=dtype, device=dev)
        for gs, st in zip(grads, stats):
            gs_d = [put(g) for g in gs]
            fn(ps, gs_d, ms, vs, step_t, stats_out, acc, put(st), LR, *BETAS,
               EPS, max_norm, zero_grads)
            reports.append(stats_out.clone())
            want = [put(torch.zeros_like(g) if zero_grads else g) for g in gs]
            assert all(torch.equal(a, b) for a, b in zip(gs_d, want))
        assert step_t.item() == STEPS
    reports = torch.stack(reports)
    res = {"p": torch.cat([p.detach() for p in ps]), "exp_avg": torch.cat(ms),
           "exp_avg_sq": torch.cat(vs), "norm": reports[:, 0],
           "clip": reports[:, 1], "acc": acc}
    return {k: v.double().cpu() for k, v in res.items()}


def _dqn_trainer(jobs_dir, optimizer_step, prioritized):
    from ddls_amd.models.gnn import GNNPolicy
    from ddls_amd.rl.dqn import DQNConfig, DQNTrainer
    from ddls_amd.rl.engine_env import EngineVectorEnv
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    venv = EngineVectorEnv(
        lambda: make_env(jobs_dir, "remove_and_repeat", 2, 3000, 15),
        num_envs=16, device=dev, base_seed=23)
    cfg = DQNConfig(learning_starts=50, sgd_minibatch_size=32, num_sgd_iter=2,
                    lr=1e-4, learner="device", head_step="fused",
                    trunk_step="fused", prioritized_replay=prioritized,
                    optimizer_step=optimizer_step)
    return DQNTrainer(venv, GNNPolicy(num_actions=17).to(dev), cfg,
                      device=dev)


def test_optimizer_step_is_checked_and_configured():
    import yaml
    from ddls_amd.rl.dqn import DQNConfig
    from ddls_amd.rl.impala import ImpalaConfig
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for cls, name in ((DQNConfig, "apex_dqn"), (ImpalaConfig, "impala")):
        assert cls().optimizer_step == "torch"
        assert cls(optimizer_step="fused").optimizer_step == "fused"
        with pytest.raises(ValueError):
            cls(optimizer_step="bogus")
        with open(os.path.join(root, "configs", "algo", name + ".yaml")) as f:
            assert yaml.safe_load(f)["optimizer_step"] == "torch"


@pytest.mark.parametrize("mode", CLIP_MODES)
def test_reference_on_cpu_is_clip_and_adam(mode):
    case, dev = _case("boundaries"), torch.device("cpu")
    run = functools.partial(_run, case, _max_norm(case, mode), False, dev=dev)
    _hold_to_float64_bound(run(torch.float64, impl="reference"),
                           run(torch.float32, impl="torch"),
                           run(torch.float32, impl="reference"))


@pytest.mark.parametrize("first", ["fused", "torch"])
def test_state_dict_continues_under_the_other_setting(first):
    """Two steps under one setting, a state dict, one step under the other,
    against an Adam that made all three steps itself (CPU tensors, so "fused"
    is learner_tail_reference)."""
    from ddls_amd.rl.learner_tail import LearnerTail
    p0, grads, _, norms = _case("boundaries")
    max_norm = 0.5 * min(norms)

    def make(ps, fused):
        opt = torch.optim.Adam(ps, lr=LR, betas=BETAS, eps=EPS, foreach=True)
        return ps, opt, LearnerTail(opt, ps, max_norm) if fused else None

    def step(ps, opt, tail, gs):
        for p, g in zip(ps, gs):
            p.grad = g.clone()
        if tail is not None:
            return tail.step()
        torch.nn.utils.clip_grad_norm_(ps, max_norm)
        opt.step()

    fresh = lambda: [torch.nn.Parameter(p.clone()) for p in p0]
    alone, a = make(fresh(), False), make(fresh(), first == "fused")
    for gs in grads[:2]:
        step(*alone, gs)
        step(*a, gs)
    b = make(a[0], first == "torch")    # the same parameters, a new optimizer
    if a[2] is not None:
        a[2].sync_steps()
    b[1].load_state_dict(a[1].state_dict())
    if b[2] is not None:
        b[2].load_steps()
    step(*alone, grads[2])
    step(*b, grads[2])
    if b[2] is not None:
        b[2].sync_steps()
    assert all(b[1].state[p]["step"].item() == 3 for p in b[0])
    truth = {"p": torch.cat([p.detach() for p in alone[0]]).double()}
    _hold_to_float64_bound(
        truth, truth, {"p": torch.cat([p.detach() for p in b[0]]).double()})


@pytest.mark.gpu
@pytest.mark.parametrize("zero_grads", [False, True])
@pytest.mark.parametrize("mode", CLIP_MODES)
@pytest.mark.parametrize("name", list(SIZES))
def test_kernel_matches_float64_reference(name, mode, zero_grads):
    from ddls_amd import ops as hip_ops
    assert hip_ops.get_extension(required=True).learner_tail_limits()[:2] \
        == [64, LIMIT]
    case, dev = _case(name), torch.device("cuda:0")
    run = functools.partial(_run, case, _max_norm(case, mode), zero_grads,
                            dev=dev)
    fused = run(torch.float32, impl="kernel")
    assert all(torch.isfinite(v).all() for v in fused.values())
    _hold_to_float64_bound(run(torch.float64, impl="reference"),
                           run(torch.float32, impl="torch"), fused)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["policy", "3xlimit"])
def test_kernel_is_reproducible(name):
    case, dev = _case(name), torch.device("cuda:0")
    a, b = (_run(case, _max_norm(case, "active"), True, torch.float32, dev,
                 "kernel") for _ in range(2))
    assert all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.gpu
def test_kernel_rejects_65_tensors():
    from ddls_amd import ops as hip_ops
    ext = hip_ops.get_extension(required=True)
    dev = torch.device("cuda:0")
    lists = [[torch.zeros(7, device=dev) for _ in range(65)] for _ in range(4)]
    with pytest.raises(RuntimeError, match="learner_tail"):
        ext.learner_tail(*lists, torch.zeros(1, device=dev),
                         torch.zeros(2, device=dev), None, None, LR, *BETAS,
                         EPS, 1.0, False)


@pytest.mark.gpu
@pytest.mark.parametrize("algo", ["dqn", "dqn_prioritized", "impala"])
def test_learner_with_fused_optimizer_step(multi_model_files, algo):
    """One device update from the same weights and rollout under either
    setting.  All parameters together are one quantity, as "p" above, held to
    the bound with the "torch" setting as both truth and reference:
    4 * eps_f32 * max|p|."""
    flat = lambda tr: torch.cat([p.detach().flatten() for p in
                                 tr.policy.parameters()]).double().cpu()
    params = {}
    for setting in ("torch", "fused"):
        if algo == "impala":
            tr = _impala_trainer(
                multi_model_files, torch.device("cuda:0"), 16, 23,
                head_step="fused", trunk_step="fused", optimizer_step=setting)
        else:
            tr = _dqn_trainer(multi_model_files, setting,
                              algo == "dqn_prioritized")
        before = flat(tr)
        torch.manual_seed(8)
        st = tr.train(num_steps=8)
        assert st["learner"] == 1 and st["total_loss"] != 0
        assert st["optimizer_step"] == int(setting == "fused")
        assert all(np.isfinite(v) for v in st.values())
        params[setting] = flat(tr)
        assert not torch.equal(before, params[setting])
    truth = {"p": params["torch"]}
    _hold_to_float64_bound(truth, truth, {"p": params["fused"]})
