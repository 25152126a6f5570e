"""The fused rollout kernel (``env_rollout_batch``) against the per-step
kernels it fuses (``actor_batch`` + ``env_step_batch``), bit for bit, and the
public paths built on it: ``rollout(sampler="fused")`` and
``EngineEvalLoop(fused_steps=...)``.

Episodes are 150 s of simulated time at one arrival per 15 s, so an env ends
an episode every ten steps; the memo hash table starts cold, so the first
placed job of every (model, degree) is a memo miss.
"""
import numpy as np
import pytest
import torch

from ddls_amd.cluster.vec_engine import (compile_engine_spec,
                                         drain_episode_schedule)
from ddls_amd.models.gnn import graph_mean
from ddls_amd.rl.device_actor import ROW_KEYS, DeviceActor
from ddls_amd.rl.engine_env import EngineVectorEnv, build_models_batch
from ddls_amd.runtime.loops import EngineEvalLoop
from tests.test_engine_eval import _policy, jobs_dir, make_env  # noqa: F401

REWARDS = ("lookahead_job_completion_time", "mean_cluster_throughput")
SEED = 7
B = 5          # not a multiple of the 4 envs per workgroup


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


def _play(spec, proto, mode, T, fused, splits=None):
    """A cold-memo GpuEngine of B envs played for T steps with resets, as
    ``rollout`` does: per step (``actor.act`` + ``eng.step``) or, ``fused``,
    with ``actor.rollout``.  ``splits`` is a list of (T, t0) calls to make
    instead of one (T, None).  Returns (every row buffer and every state
    tensor but the hash table by name, episodes ended, memo inserts)."""
    from ddls_amd.cluster.gpu_engine import GpuEngine
    dev = torch.device("cuda:0")
    gen = proto.cluster.jobs_generator
    sched = lambda b, ep: drain_episode_schedule(
        gen, spec, seed=SEED + 1000 * b + ep)
    first = [sched(b, 0) for b in range(B)]
    eng = GpuEngine(spec, B=B, device=dev, preload_memo=False,
                    n_jobs_cap=max(s.n for s in first) + 8)
    for b in range(B):
        eng.reset_env(b, first[b])
    if mode in ("policy_sample", "policy_greedy"):
        policy = _policy().to(dev)
        actor = DeviceActor.policy(policy, mode == "policy_greedy", seed=SEED)
        batch = build_models_batch(spec, dev)
        actor.prepare(None, model_emb=graph_mean(policy.gnn(batch), batch))
    else:
        actor = DeviceActor.heuristic(mode, seed=SEED)
    A = spec.A
    fill = lambda *s, dt=torch.float32: torch.full(s, -7, dtype=dt, device=dev)
    rows = {"gfull": fill(T, B, 17 + A), "lp_all": fill(T, B, A),
            "logp": fill(T, B), "value": fill(T, B), "u": fill(T, B),
            "actions": fill(T, B, dt=torch.int64),
            "model": fill(T, B, dt=torch.int64), "rewards": fill(T, B),
            "dones": fill(T, B, dt=torch.uint8)}
    episodes = [0] * B

    def result():
        state = {k: v for k, v in eng.T.items() if torch.is_tensor(v)
                 and k not in ("hash_keys", "hash_vals")}
        return {**rows, **state}, sum(episodes), len(eng._hash_slots)

    def reset(b):
        episodes[b] += 1
        eng.reset_env(b, sched(b, episodes[b]))

    if fused:
        for n, t0 in splits or [(T, None)]:
            part = {k: v[:n] for k, v in rows.items()}
            while t0 is None or (np.asarray(t0) < n).any():
                t0, done = actor.rollout(eng, 100, n, part, t0=t0)
                for b, _ in done:
                    reset(b)
        return result()
    for t in range(T):
        rows["model"][t] = eng.T["obs_model"]
        acts = actor.act(eng, 100 + t, rows={k: rows[k][t] for k in ROW_KEYS})
        rows["actions"][t] = acts
        eng.step(acts)
        rows["rewards"][t] = eng.T["reward"].float()
        rows["dones"][t] = eng.T["done"]
        for b in torch.nonzero(eng.T["done"]).flatten().tolist():
            reset(b)
    return result()


@pytest.mark.gpu
@pytest.mark.parametrize("reward", REWARDS)
@pytest.mark.parametrize("mode", ["policy_sample", "policy_greedy", "random",
                                  "acceptable_jct"])
def test_kernel_equals_per_step_kernels(short, mode, reward):
    spec, proto = short[reward]
    want, episodes, inserts = _play(spec, proto, mode, 12, fused=False)
    assert episodes >= 1 and inserts >= 1    # an episode end and a memo miss
    got, _, _ = _play(spec, proto, mode, 12, fused=True)
    for k in want:
        assert torch.equal(got[k], want[k]), k


@pytest.mark.gpu
def test_resume_and_nonuniform_t0(short):
    spec, proto = short[REWARDS[0]]
    whole, _, inserts = _play(spec, proto, "policy_sample", 7, fused=True)
    assert inserts >= 1
    # [1]: steps 0-1 for all, step 2 for envs 1 and 3 only, then the rest
    for splits in ([(3, None), (7, [3] * B)],
                   [(2, None), (3, [3, 2, 3, 2, 3]), (7, [2, 3, 2, 3, 2])]):
        got, _, _ = _play(spec, proto, "policy_sample", 7, fused=True,
                          splits=splits)
        for k in whole:
            assert torch.equal(got[k], whole[k]), (splits, k)


@pytest.mark.parametrize("device_resident", [False, True])
@pytest.mark.parametrize("device", [
    "cpu", pytest.param("cuda:0", marks=pytest.mark.gpu)])
def test_rollout_fused_equals_device(short, device, device_resident):
    """Also on a CpuEngine, where "fused" is the "device" path."""
    spec, proto = short[REWARDS[0]]
    policy = _policy().to(device)
    envs = [EngineVectorEnv(None, num_envs=B, device=device, base_seed=SEED,
                            spec=spec, proto_env=proto) for _ in range(2)]
    a, b = (env.rollout(policy, 12, device_resident=device_resident,
                        sampler=sampler)
            for env, sampler in zip(envs, ("fused", "device")))
    assert set(a) == set(b)
    for k in b:
        if k == "obs":
            for x, y in zip(a[k], b[k]):
                assert x.model_id == y.model_id
                np.testing.assert_array_equal(x.graph_features,
                                              y.graph_features)
        elif torch.is_tensor(b[k]):
            assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k
        else:
            assert a[k].dtype == b[k].dtype, k
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    assert envs[0]._sampler_step == envs[1]._sampler_step == 12
    stats = [env.completed_episode_stats for env in envs]
    assert len(stats[0]) == len(stats[1]) >= B
    for x, y in zip(*stats):
        assert x.keys() == y.keys()
        for k in y:
            np.testing.assert_array_equal(x[k], y[k], err_msg=k)


@pytest.mark.gpu
def test_eval_loop_fused_steps(short):
    spec, proto = short[REWARDS[0]]
    seeds = [3, 1799, 5]
    for actor in (DeviceActor.heuristic("acceptable_jct"),
                  DeviceActor.policy(_policy().to("cuda:0"))):
        want = EngineEvalLoop(actor, None, "cuda:0", spec=spec,
                              proto_env=proto).run(seeds)
        got = EngineEvalLoop(actor, None, "cuda:0", spec=spec,
                             proto_env=proto, fused_steps=8).run(seeds)
        for g, w in zip(got, want):
            assert w["num_actor_steps"] > 8      # more than one chunk
            for k in ("seed", "num_actor_steps", "episode_return"):
                assert g[k] == w[k], k
            assert g["episode_stats"].keys() == w["episode_stats"].keys()
            for k, v in w["episode_stats"].items():
                np.testing.assert_array_equal(g["episode_stats"][k], v,
                                              err_msg=k)


def test_configs_take_fused_and_reject_unknown():
    from ddls_amd.rl.dqn import DQNConfig
    from ddls_amd.rl.impala import ImpalaConfig
    from ddls_amd.rl.ppo import PPOConfig
    for cls in (ImpalaConfig, DQNConfig, PPOConfig):
        assert cls().rollout_sampler == "torch"
        assert cls(rollout_sampler="fused").rollout_sampler == "fused"
        with pytest.raises(ValueError):
            cls(rollout_sampler="numpy")
