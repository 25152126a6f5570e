"""The population rollout kernel (``env_rollout_population``) against the
per-step kernels it fuses (``actor_population`` + ``env_step_batch``), bit for
bit, and the public paths built on it: ``PopulationEvaluator(rollout="fused")``
and ``ESConfig.population_rollout``.

Episodes are 150 s of simulated time at one arrival per 15 s, so every env
ends its episode after ten steps; the memo hash table of the kernel test
starts cold, so the first placed job of every (model, degree) is a memo miss.
"""
import os

import pytest
import torch

from ddls_amd.cluster.vec_engine import compile_engine_spec
from ddls_amd.rl.engine_env import EngineVectorEnv
from ddls_amd.rl.es import ESConfig, ESTrainer
from ddls_amd.rl.es_population import PopulationEvaluator
from tests.test_engine_eval import jobs_dir, make_env  # noqa: F401
from tests.test_es_population import _flat, _policy

REWARDS = ("lookahead_job_completion_time", "mean_cluster_throughput")
SEED = 7
# members of the seed-4 policy perturbed with sigma 0.1 take different actions
# on these episodes (checked on a CpuEngine with act_population_reference:
# 6 to 50 (step, schedule) pairs differ per case, in both modes)
POLICY_SEED, SIGMA, K = 4, 0.1, 2


@pytest.fixture(scope="module")
def short(jobs_dir):  # noqa: F811
    """reward -> (compiled spec, proto env) of the 150 s episode."""
    out = {}
    for reward in REWARDS:
        proto = make_env(jobs_dir, reward)
        proto.max_simulation_run_time = 150
        proto.reset(seed=987654321)
        out[reward] = (compile_engine_spec(proto, lookahead_device=None),
                       proto)
    return out


def _evaluator(short, reward, device, E, **kw):
    spec, proto = short[reward]
    venv = EngineVectorEnv(None, num_envs=E, device=device, base_seed=SEED,
                           spec=spec, proto_env=proto)
    policy = _policy(17, seed=POLICY_SEED).to(device)
    ev = PopulationEvaluator(venv, policy, perturbation_pairs=K,
                             envs_per_member=E, **kw)
    return ev, ev.perturb(_flat(policy), SIGMA, 0)[1]


def _play(short, reward, greedy, E, fused, total=16, chunk=4, **kw):
    """A cold-memo engine of 2K * E envs, reset as ``PopulationEvaluator.reset``
    does and played until every env is done: per step (``actor_population`` +
    ``eng.step``) or in ``rollout_population`` launches of ``chunk`` steps."""
    from ddls_amd.cluster.gpu_engine import GpuEngine
    dev = torch.device("cuda:0")
    ev, pop = _evaluator(short, reward, dev, E, deterministic=greedy)
    scheds = ev.schedules(0)
    ev._cap = max(s.n for s in scheds) + 8
    eng = ev.eng = GpuEngine(ev.spec, B=ev.B, device=dev, preload_memo=False,
                             n_jobs_cap=ev._cap)
    ev.reset(scheds)
    emb = ev.embeddings(pop)
    ret = torch.zeros(ev.B, dtype=torch.float64, device=dev)
    nlive = torch.zeros(ev.B, dtype=torch.int64, device=dev)
    actions = torch.full((total, ev.B), -7, dtype=torch.int64, device=dev)
    t = 0
    while t < total and bool((eng.T["done"] == 0).any()):
        if fused:
            eng.rollout_population(pop, emb, ev.head_offs, E, ev.mode, SEED,
                                   100 + t, chunk, ret, nlive,
                                   actions=actions[t:t + chunk], **kw)
            t += chunk
            continue
        live = eng.T["done"] == 0
        acts = ev.act(pop, emb, 100 + t)
        actions[t] = torch.where(live, acts.long(), actions[t])
        eng.step(acts)
        ret = torch.where(live, ret + eng.T["reward"], ret)
        nlive += live.long()
        t += 1
    out = {k: eng.T[k] for k in eng._env_keys}
    out.update(ret=ret.view(torch.int64), nlive=nlive, actions_rows=actions)
    return out, len(eng._hash_slots)


@pytest.mark.gpu
@pytest.mark.parametrize("reward", REWARDS)
@pytest.mark.parametrize("E", [1, 5])
@pytest.mark.parametrize("greedy", [False, True])
def test_kernel_equals_per_step_kernels(short, greedy, E, reward):
    want, inserts = _play(short, reward, greedy, E, fused=False)
    assert inserts >= 1 and bool(want["done"].any())
    rows = want["actions_rows"].view(-1, 2 * K, E)
    assert bool(((rows != rows[:, :1]) & (rows >= 0)
                 & (rows[:, :1] >= 0)).any())    # members act differently
    # the default envs per workgroup, and 4 (E = 5: a ragged last workgroup)
    for kw in ({}, {"max_wpb": 4}):
        got, _ = _play(short, reward, greedy, E, fused=True, **kw)
        for k in want:
            assert torch.equal(got[k], want[k]), (kw, k)


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [6, 40])     # truncates / above the episode
def test_evaluator_fused_equals_steps(short, cap):
    res = {}
    for rollout in ("steps", "fused"):
        ev, pop = _evaluator(short, REWARDS[0], torch.device("cuda:0"), 3,
                             eval_max_steps=cap, rollout=rollout,
                             fused_steps=4)
        assert ev.fused_rollout == (rollout == "fused")
        res[rollout] = ev.evaluate(pop, generation=1)
    a, b = res["fused"], res["steps"]
    assert a["returns"].tobytes() == b["returns"].tobytes()
    for k in ("live_steps", "eval_steps", "truncated_envs"):
        assert a[k] == b[k], k
    assert (b["truncated_envs"] > 0) == (cap == 6)
    assert b["eval_steps"] == min(cap, 10)


@pytest.mark.parametrize("device", [
    "cpu", pytest.param("cuda:0", marks=pytest.mark.gpu)])
def test_trainer_fused_equals_steps(short, device):
    """Also on a CpuEngine, where "fused" is the step path."""
    spec, proto = short[REWARDS[0]]
    ends = {}
    for rollout in ("steps", "fused"):
        venv = EngineVectorEnv(None, num_envs=2, device=device,
                               base_seed=SEED, spec=spec, proto_env=proto)
        tr = ESTrainer(venv, _policy(17, seed=POLICY_SEED), ESConfig(
            evaluator="population", perturbation_pairs=K, envs_per_member=2,
            eval_max_steps=12, noise_seed=3, noise_stdev=SIGMA,
            population_rollout=rollout), device=torch.device(device))
        for _ in range(2):
            st = tr.train()
        assert st["population_rollout"] == int(
            rollout == "fused" and device != "cpu")
        assert st["eval_steps"] == 10
        ends[rollout] = tr._get_flat().cpu().numpy().tobytes()
    assert ends["fused"] == ends["steps"]


def test_config_takes_population_rollout(short, jobs_dir):  # noqa: F811
    import yaml

    from ddls_amd.runtime.config import build_trainer_from_config, load_config
    assert ESConfig().population_rollout == "steps"
    with pytest.raises(ValueError):
        ESConfig(population_rollout="graph")
    with pytest.raises(ValueError):
        _evaluator(short, REWARDS[0], torch.device("cpu"), 2, rollout="graph")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = load_config(os.path.join(root, "configs", "train_config.yaml"))
    with open(os.path.join(root, "configs", "algo", "es.yaml")) as f:
        cfg["algo"] = yaml.safe_load(f)
    assert cfg["algo"]["population_rollout"] == "steps"
    cfg["algo"].update(evaluator="population", population_rollout="fused")
    cfg["env_config"]["jobs_config"]["path_to_files"] = jobs_dir
    cfg["epoch_loop"].update(num_envs=2, num_env_workers=1,
                             precompute_lookaheads=False,
                             env_backend="engine")
    tr = build_trainer_from_config(cfg, device=torch.device("cpu"))
    assert tr.config.population_rollout == "fused"
    tr.env.close()
