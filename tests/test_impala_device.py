"""Device IMPALA learner (rl/impala.py ``learner="device"``) and the fused
V-trace loss kernels (ops/hip/vtrace_loss.hip)."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.test_vec_engine import make_env, multi_model_files  # noqa: F401

EPS32 = float(np.finfo(np.float32).eps)


def vtrace_reference(rewards, dones, values, bootstrap, rho, c, gamma):
    """Slow literal recursion of Espeholt et al. (2018), eqns 1-2."""
    T, N = rewards.shape
    nonterminal = 1.0 - dones
    vp1 = np.concatenate([values[1:], bootstrap[None]], axis=0) * nonterminal
    delta = rho * (rewards + gamma * vp1 - values)
    vs = np.zeros_like(values)
    for t in reversed(range(T)):
        nxt = (vs[t + 1] - values[t + 1]) if t + 1 < T else 0.0
        vs[t] = values[t] + delta[t] + gamma * c[t] * nonterminal[t] * nxt
    vsp1 = np.concatenate([vs[1:], bootstrap[None]], axis=0) * nonterminal
    pg_adv = rewards + gamma * vsp1 - values
    return vs, pg_adv


def _loss_cfg(clips=(1.0, 1.0, 1.0), drop_last=True, gamma=0.997,
              vf_coeff=0.5, ent_coeff=0.01):
    return SimpleNamespace(rho_clip=clips[0], pg_rho_clip=clips[1],
                           c_clip=clips[2], gamma=gamma,
                           vf_loss_coeff=vf_coeff, entropy_coeff=ent_coeff,
                           vtrace_drop_last_ts=drop_last)


def _loss_inputs(T, N, A, seed, dev):
    """Inputs at the scales of test_fused_ppo_loss_matches_torch: logits*2
    with 20% masked to finfo.min (never the taken action), values*5.  The
    behaviour log-probs place pi/mu evenly over [0.5, 1.63], so ratios fall
    on both sides of every clip in {0.9, 1.0, 1.1, 1.3}."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    R = T * N
    logits = torch.randn(R, A, generator=g) * 2
    masked = torch.rand(R, A, generator=g) < 0.2
    actions = torch.randint(0, A, (R,), generator=g)
    masked[torch.arange(R), actions] = False
    logits[masked] = torch.finfo(torch.float32).min
    values = torch.randn(R, generator=g) * 5
    rewards = torch.randn(T, N, generator=g)
    dones = (torch.rand(T, N, generator=g) < 0.15).float()
    bootstrap = torch.randn(N, generator=g) * 5
    ratio = torch.linspace(0.5, 1.63, R)[torch.randperm(R, generator=g)]
    logp_a = torch.log_softmax(logits, -1)[torch.arange(R), actions]
    behaviour_logp = logp_a - torch.log(ratio)
    for clip in (0.9, 1.0, 1.1, 1.3):
        assert (ratio < clip - 1e-3).any() and (ratio > clip + 1e-3).any()
        assert ((ratio - clip).abs() > 1e-3).all()
    out = dict(logits=logits, values=values, actions=actions,
               behaviour_logp=behaviour_logp, rewards=rewards, dones=dones,
               bootstrap=bootstrap)
    return {k: v.to(dev) for k, v in out.items()}


def _reference(inp, cfg, dtype=torch.float32):
    """impala_loss_reference + autograd -> (loss, stats[5], glogits,
    gvalues), all in ``dtype``."""
    from ddls_amd.rl.impala import STAT_KEYS, impala_loss_reference
    cast = lambda t: t.to(dtype) if t.is_floating_point() else t
    x = {k: cast(v) for k, v in inp.items()}
    lt = x["logits"].clone().requires_grad_(True)
    vt = x["values"].clone().requires_grad_(True)
    loss, st = impala_loss_reference(
        lt, vt, x["actions"], x["behaviour_logp"], x["rewards"], x["dones"],
        x["bootstrap"], cfg)
    loss.backward()
    return (loss.detach(), torch.stack([st[k] for k in STAT_KEYS]),
            lt.grad, vt.grad)


def _fused(inp, cfg):
    from ddls_amd.rl.impala import _ImpalaLossFn
    T, N = inp["rewards"].shape
    lf = inp["logits"].clone().requires_grad_(True)
    vf = inp["values"].clone().requires_grad_(True)
    loss, stats = _ImpalaLossFn.apply(
        lf, vf, inp["actions"], inp["behaviour_logp"].reshape(-1),
        inp["rewards"].reshape(-1), inp["dones"].reshape(-1),
        inp["bootstrap"], T, N, cfg.gamma, cfg.rho_clip, cfg.pg_rho_clip,
        cfg.c_clip, cfg.vf_loss_coeff, cfg.entropy_coeff,
        cfg.vtrace_drop_last_ts)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach(), stats, lf.grad, vf.grad


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
def test_learner_value_is_checked(multi_model_files):
    from ddls_amd.models.gnn import GNNPolicy
    from ddls_amd.rl.impala import ImpalaConfig, ImpalaTrainer
    from ddls_amd.rl.rollout import VectorEnv

    assert ImpalaConfig().learner == "torch"
    venv = VectorEnv([lambda: make_env(multi_model_files,
                                       "remove_and_repeat", 2, 3000, 30)],
                     base_seed=3)
    with pytest.raises(ValueError):
        ImpalaTrainer(venv, GNNPolicy(num_actions=17),
                      ImpalaConfig(learner="bogus"),
                      device=torch.device("cpu"))


def test_config_group_carries_learner():
    import yaml
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "configs", "algo", "impala.yaml")) as f:
        assert yaml.safe_load(f)["learner"] == "torch"


def test_device_learner_falls_back_on_host_env(multi_model_files, capsys):
    """An env without supports_device_resident: one warning, torch path."""
    from ddls_amd.models.gnn import GNNPolicy
    from ddls_amd.rl.impala import ImpalaConfig, ImpalaTrainer
    from ddls_amd.rl.rollout import VectorEnv

    torch.manual_seed(0)
    venv = VectorEnv([lambda i=i: make_env(multi_model_files,
                                           "remove_and_repeat", 2, 3000, 30)
                      for i in range(2)], base_seed=3)
    policy = GNNPolicy(num_actions=17)
    before = {k: v.clone() for k, v in policy.state_dict().items()}
    tr = ImpalaTrainer(venv, policy,
                       ImpalaConfig(train_batch_size=2 * 4, learner="device"),
                       device=torch.device("cpu"))
    for _ in range(2):
        st = tr.train(num_steps=4)
        assert np.isfinite(st["total_loss"]) and st["learner"] == 0
    assert capsys.readouterr().err.count("learner='device'") == 1
    assert any(not torch.equal(before[k], v)
               for k, v in policy.state_dict().items())


def _cpu_engine_trainer(jobs_dir, learner):
    from ddls_amd.models.gnn import GNNPolicy
    from ddls_amd.rl.engine_env import EngineVectorEnv
    from ddls_amd.rl.impala import ImpalaConfig, ImpalaTrainer

    dev = torch.device("cpu")
    torch.manual_seed(4)
    policy = GNNPolicy(num_actions=17)
    venv = EngineVectorEnv(
        lambda: make_env(jobs_dir, "remove_and_repeat", 2, 3000, 15),
        num_envs=4, device=dev, base_seed=19)
    return ImpalaTrainer(venv, policy,
                         ImpalaConfig(train_batch_size=4 * 6,
                                      learner=learner), device=dev)


def test_device_learner_equals_torch_learner_on_cpu_engine(multi_model_files):
    """Same seed, same initial weights: after two iterations every parameter
    of the device learner is torch.equal to the torch learner's — on CPU
    tensors both evaluate the same torch expressions on the same values."""
    runs = {}
    for learner in ("torch", "device"):
        tr = _cpu_engine_trainer(multi_model_files, learner)
        torch.manual_seed(8)
        stats = []
        for _ in range(2):
            data = tr.collect_rollout(6)
            st = tr.update(data)
            stats.append(st)
            if learner == "device":
                assert st["learner"] == 1
                assert data["obs"]._items is None
                assert data["rewards_dev"].shape == (24,)
                assert data["dones_dev"].dtype == torch.float32
                assert data["bootstrap_dev"].shape == (4,)
                assert np.array_equal(data["rewards_dev"].numpy(),
                                      data["rewards"].reshape(-1))
                assert np.array_equal(data["dones_dev"].numpy() != 0,
                                      data["dones"].reshape(-1))
            else:
                assert st["learner"] == 0
        runs[learner] = (tr.policy.state_dict(), stats)
    sd_t, st_t = runs["torch"]
    sd_d, st_d = runs["device"]
    for k in sd_t:
        assert torch.equal(sd_t[k], sd_d[k]), k
    for a, b in zip(st_t, st_d):
        for k in ("policy_loss", "vf_loss", "entropy", "total_loss",
                  "mean_rho"):
            assert a[k] == b[k], k


@pytest.mark.parametrize("drop_last", [True, False])
def test_loss_reference_matches_numpy_recursion(drop_last):
    """impala_loss_reference in float64 against the loss written out in
    numpy over the literal recursion vtrace_reference."""
    from ddls_amd.rl.impala import impala_loss_reference
    T, N, A = 6, 4, 5
    cfg = _loss_cfg(clips=(0.9, 1.3, 1.1), drop_last=drop_last, gamma=0.99)
    inp = _loss_inputs(T, N, A, seed=2, dev="cpu")
    x = {k: (v.double() if v.is_floating_point() else v)
         for k, v in inp.items()}
    loss, st = impala_loss_reference(
        x["logits"], x["values"], x["actions"], x["behaviour_logp"],
        x["rewards"], x["dones"], x["bootstrap"], cfg)

    lg = x["logits"].numpy()
    lp = lg - lg.max(-1, keepdims=True)
    lp = lp - np.log(np.exp(lp).sum(-1, keepdims=True))
    p = np.exp(lp)
    ent = -np.where(p > 0, p * lp, 0.0).sum(-1).reshape(T, N)
    logp_a = lp[np.arange(T * N), x["actions"].numpy()].reshape(T, N)
    ratio = np.exp(logp_a - x["behaviour_logp"].numpy().reshape(T, N))
    values = x["values"].numpy().reshape(T, N)
    vs, pg = vtrace_reference(
        x["rewards"].numpy(), x["dones"].numpy(), values,
        x["bootstrap"].numpy(), np.minimum(ratio, cfg.rho_clip),
        np.minimum(ratio, cfg.c_clip), cfg.gamma)
    pg = np.minimum(ratio, cfg.pg_rho_clip) * pg
    k = slice(0, T - 1) if drop_last else slice(0, T)
    want = {"policy_loss": -(pg[k] * logp_a[k]).mean(),
            "vf_loss": 0.5 * ((vs[k] - values[k]) ** 2).mean(),
            "entropy": ent[k].mean(),
            "mean_rho": np.minimum(ratio, cfg.rho_clip).mean()}
    want["total_loss"] = (want["policy_loss"] + 0.5 * want["vf_loss"]
                          - 0.01 * want["entropy"])
    for key, w in want.items():
        assert st[key].item() == pytest.approx(w, rel=1e-10, abs=1e-12), key
    assert loss.item() == pytest.approx(want["total_loss"], rel=1e-10)


def test_pg_on_cpu_engine_unchanged(multi_model_files):
    """PGTrainer inherits collect_rollout and holds a PGConfig, which has no
    learner switch.  The values are the ones the trainer produced before the
    device learner existed (seed 5, one iteration)."""
    from ddls_amd.models.gnn import GNNPolicy
    from ddls_amd.rl.engine_env import EngineVectorEnv
    from ddls_amd.rl.pg import PGConfig, PGTrainer

    dev = torch.device("cpu")
    torch.manual_seed(5)
    policy = GNNPolicy(num_actions=17)
    venv = EngineVectorEnv(
        lambda: make_env(multi_model_files, "remove_and_repeat", 2, 3000, 15),
        num_envs=4, device=dev, base_seed=29)
    tr = PGTrainer(venv, policy, PGConfig(train_batch_size=4 * 6), device=dev)
    st = tr.train(num_steps=6)
    recorded = {"policy_loss": -98.8288345336914,
                "total_loss": -98.8288345336914,
                "entropy": 1.9434407949447632,
                "mean_return": -50.94508743286133,
                "mean_reward": -12.932952880859375}
    for k, want in recorded.items():
        assert st[k] == pytest.approx(want, rel=1e-5), k
    assert "learner" not in st


# ---------------------------------------------------------------------------
# GPU: kernels
# ---------------------------------------------------------------------------
def _ext():
    from ddls_amd import ops as hip_ops
    ext = hip_ops.get_extension(required=True)
    assert hasattr(ext, "vtrace_scan") and hasattr(ext, "impala_loss_fwd")
    return ext


@pytest.mark.gpu
@pytest.mark.parametrize("T,N", [(1, 1), (2, 3), (13, 5), (9, 70), (5, 300)])
def test_vtrace_scan_bits(T, N):
    """vtrace_scan equals vtrace_targets bit for bit on the same CUDA
    tensors: dones with p=0.15, a column that is all done, a done on the
    first and on the last row, c != rho, a gamma that is not an f32."""
    from ddls_amd.rl.impala import vtrace_targets
    ext = _ext()
    dev = "cuda:0"
    g = torch.Generator(device="cpu").manual_seed(100 * T + N)
    rewards = torch.randn(T, N, generator=g) * 3
    values = torch.randn(T, N, generator=g) * 5
    bootstrap = torch.randn(N, generator=g) * 5
    dones = (torch.rand(T, N, generator=g) < 0.15).float()
    dones[:, 0] = 1.0
    dones[0, 1 % N] = 1.0
    dones[T - 1, 2 % N] = 1.0
    ratio = torch.exp(torch.randn(T, N, generator=g) * 0.3)
    rho = torch.clamp(ratio, max=1.0)
    c = torch.clamp(ratio, max=0.8)
    assert not torch.equal(rho, c)
    args = [t.to(dev) for t in (rewards, dones, values, bootstrap, rho, c)]
    vs, pg = ext.vtrace_scan(*args, 0.997)
    vs_ref, pg_ref = vtrace_targets(*args, 0.997)
    torch.cuda.synchronize()
    assert vs.shape == (T, N) and pg.shape == (T, N)
    assert torch.equal(vs, vs_ref), (vs - vs_ref).abs().max().item()
    assert torch.equal(pg, pg_ref), (pg - pg_ref).abs().max().item()


@pytest.mark.gpu
@pytest.mark.parametrize("clips", [(1.0, 1.0, 1.0), (0.9, 1.3, 1.1)])
@pytest.mark.parametrize("drop_last", [True, False])
@pytest.mark.parametrize("T,N,A", [(7, 13, 17), (1, 5, 3), (4, 3, 64)])
def test_fused_impala_loss_matches_torch(T, N, A, drop_last, clips):
    """impala_loss_fwd / impala_loss_bwd against torch autograd over
    impala_loss_reference, held to test_fused_ppo_loss_matches_torch's
    figures for the sister kernel."""
    _ext()
    cfg = _loss_cfg(clips=clips, drop_last=drop_last)
    inp = _loss_inputs(T, N, A, seed=7 * T + A, dev="cuda:0")
    loss_r, stats_r, gl_r, gv_r = _reference(inp, cfg)
    loss_f, stats_f, gl_f, gv_f = _fused(inp, cfg)
    print(f"loss {loss_f.item():.6f} vs {loss_r.item():.6f}; stats err "
          f"{(stats_f - stats_r).abs().tolist()}; glogits err "
          f"{(gl_f - gl_r).abs().max().item():.3e}; gvalues err "
          f"{(gv_f - gv_r).abs().max().item():.3e}")
    assert torch.isfinite(gl_f).all() and torch.isfinite(gv_f).all()
    assert loss_f.item() == pytest.approx(loss_r.item(), abs=2e-4)
    for got, want in zip(stats_f.tolist(), stats_r.tolist()):
        assert got == pytest.approx(want, abs=2e-4)
    assert torch.allclose(gl_f, gl_r, atol=1e-5), \
        (gl_f - gl_r).abs().max().item()
    assert torch.allclose(gv_f, gv_r, atol=1e-6), \
        (gv_f - gv_r).abs().max().item()
    if drop_last and T > 1:
        K = (T - 1) * N
        assert torch.count_nonzero(gl_f[K:]) == 0
        assert torch.count_nonzero(gv_f[K:]) == 0
        assert torch.count_nonzero(gl_f[:K]) > 0
    # masked logits: p = 0 and a zero gradient, never NaN
    masked = inp["logits"] == torch.finfo(torch.float32).min
    assert torch.count_nonzero(gl_f[masked]) == 0


@pytest.mark.gpu
def test_fused_impala_loss_is_reproducible():
    """No float atomics: two calls on the same inputs give the same bits."""
    _ext()
    cfg = _loss_cfg(clips=(0.9, 1.3, 1.1))
    inp = _loss_inputs(7, 13, 17, seed=3, dev="cuda:0")
    a = _fused(inp, cfg)
    b = _fused(inp, cfg)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.gpu
def test_fused_impala_loss_rejects_wide_rows():
    ext = _ext()
    inp = _loss_inputs(2, 3, 65, seed=1, dev="cuda:0")
    with pytest.raises(RuntimeError, match="A <= 64"):
        ext.impala_loss_fwd(
            inp["logits"], inp["values"], inp["actions"],
            inp["behaviour_logp"], inp["rewards"].reshape(-1),
            inp["dones"].reshape(-1), inp["bootstrap"], 2, 3, 0.99, 1.0, 1.0,
            1.0, 0.5, 0.01, True)


# ---------------------------------------------------------------------------
# GPU: trainer
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_device_learner_on_engine_env(multi_model_files):
    """Two device-learner iterations on the GPU engine, then the kernels
    against a float64 truth at the environment's reward scale: their error
    may be at most 4x the float32 torch reference's own error plus
    4*eps_f32*max|truth| (the 4 covers a different exp/log and a different
    summation order)."""
    from ddls_amd.models.gnn import GNNPolicy
    from ddls_amd.rl.engine_env import EngineVectorEnv
    from ddls_amd.rl.impala import STAT_KEYS, ImpalaConfig, ImpalaTrainer

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    policy = GNNPolicy(num_actions=17).to(dev)
    venv = EngineVectorEnv(
        lambda: make_env(multi_model_files, "remove_and_repeat", 2, 3000, 15),
        num_envs=16, device=dev, base_seed=17)
    cfg = ImpalaConfig(train_batch_size=16 * 8, learner="device")
    tr = ImpalaTrainer(venv, policy, cfg, device=dev)
    for _ in range(2):
        data = tr.collect_rollout(8)
        st = tr.update(data)
        assert st["learner"] == 1
        assert all(np.isfinite(st[k]) for k in STAT_KEYS)
        assert data["obs"]._items is None

    with torch.no_grad():
        logits, values = tr._forward_device(data)
    assert data["obs"]._items is None
    inp = dict(logits=logits, values=values, actions=data["actions_dev"],
               behaviour_logp=data["logp_dev"],
               rewards=data["rewards_dev"].reshape(8, 16),
               dones=data["dones_dev"], bootstrap=data["bootstrap_dev"])
    truth = _reference(inp, cfg, torch.float64)
    ref32 = _reference(inp, cfg, torch.float32)
    fused = _fused(inp, cfg)
    names = ["loss"] + ["stat " + k for k in STAT_KEYS] \
        + ["glogits", "gvalues"]

    def split(r):
        return [r[0]] + list(r[1]) + [r[2], r[3]]

    failures = []
    for name, t, r, f in zip(names, split(truth), split(ref32), split(fused)):
        e_ref = (r.double() - t).abs().max().item()
        e_fused = (f.double() - t).abs().max().item()
        bound = 4 * e_ref + 4 * EPS32 * t.abs().max().item()
        print(f"{name}: max|truth| {t.abs().max().item():.6g} fused err "
              f"{e_fused:.3e} torch f32 err {e_ref:.3e} bound {bound:.3e} "
              f"ratio {e_fused / max(e_ref, 1e-300):.2f}")
        if not e_fused <= bound:
            failures.append(name)
    assert not failures, failures
