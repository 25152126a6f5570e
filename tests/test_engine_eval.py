"""Batched evaluation and device-sampled rollouts on the env engine.

``EngineEvalLoop`` is pinned exactly against ``EvalLoop`` on the real env
(CPU), and the GpuEngine + ``actor_batch`` path against the CpuEngine +
``act_reference`` path (GPU).  ``rollout(sampler="device")`` keeps the
trainer-facing dict and is reproducible from ``base_seed``.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from ddls_amd.envs import RampJobPartitioningEnvironment
from ddls_amd.envs.actors import ACTORS
from ddls_amd.rl.device_actor import DeviceActor, policy_head_reference
from ddls_amd.rl.engine_env import EngineVectorEnv
from ddls_amd.runtime.loops import EngineEvalLoop, EvalLoop

DETERMINISTIC = ("no_parallelism", "min_parallelism", "max_parallelism",
                 "sip_ml", "acceptable_jct")
SIP_CAP = 8
EXACT_KEYS = ("blocking_rate", "acceptance_rate")
EXACT_STATS = ("num_jobs_arrived", "num_jobs_completed", "num_jobs_blocked")
GREEDY_POLICY_SEED = 0     # min top-two gap >= 1e-3 on the CPU trajectory
ROLLOUT_BASE_SEED = 7      # every u >= 1e-4 from a CDF boundary on the CPU


def make_env(jobs_dir, reward="lookahead_job_completion_time",
             reward_kwargs=None):
    """The congested three-model recipe: remove_and_repeat pool, replication
    2, 3000 s of simulated time, one arrival every 15 s."""
    return RampJobPartitioningEnvironment(
        topology_config={"type": "ramp", "kwargs": {
            "num_communication_groups": 4,
            "num_racks_per_communication_group": 4,
            "num_servers_per_rack": 2,
            "num_channels": 1,
            "total_node_bandwidth": 1.6e12,
            "intra_gpu_propagation_latency": 50e-9,
            "worker_io_latency": 100e-9}},
        node_config={"type_1": {"num_nodes": 32, "workers_config": [
            {"num_workers": 1, "worker": "ddls_amd.devices.A100"}]}},
        jobs_config={"path_to_files": jobs_dir,
                     "replication_factor": 2,
                     "job_sampling_mode": "remove_and_repeat",
                     "job_interarrival_time_dist": {
                         "_target_": "ddls_amd.distributions.Fixed",
                         "val": 15},
                     "max_acceptable_job_completion_time_frac_dist": {
                         "_target_": "ddls_amd.distributions.Uniform",
                         "min_val": 0.1, "max_val": 1, "decimals": 2},
                     "num_training_steps": 10},
        max_partitions_per_op=16,
        min_op_run_time_quantum=0.01,
        pad_obs_kwargs=None,
        reward_function=reward,
        reward_function_kwargs=reward_kwargs,
        max_simulation_run_time=3000)


@pytest.fixture(scope="module")
def jobs_dir(tmp_path_factory):
    """Three small models with different sizes/costs."""
    from ddls_amd.workloads import generate_model, write_pipedream_txt
    d = tmp_path_factory.mktemp("jobs")
    for name, (nn, sk, sc, seed) in {
            "m_small": (5, 0, 0.5, 11),
            "m_mid": (8, 2, 1.0, 12),
            "m_big": (11, 3, 1.6, 13)}.items():
        nodes, edges = generate_model(name, nn, sk, sc, seed)
        write_pipedream_txt(str(d / f"{name}.txt"), nodes, edges)
    return str(d)


@pytest.fixture(scope="module")
def cpu_loop(jobs_dir):
    """One spec compile shared by the CPU-side runs of this module."""
    return EngineEvalLoop(None, lambda: make_env(jobs_dir), "cpu")


def _heuristic(name):
    kwargs = {"max_partitions_per_op": SIP_CAP} if name == "sip_ml" else {}
    return DeviceActor.heuristic(name, **kwargs)


def _memo_preload_for_env(spec):
    return {(spec.models[mid].name, deg): (jct, comm, comp,
                                           {"active_time_sum": act_sum})
            for (mid, deg), (jct, comm, comp, act_sum) in spec.memo.items()}


def _assert_same_episode(got, want, return_rtol=None):
    for k in EXACT_KEYS + ("num_actor_steps",):
        assert got[k] == want[k], k
    for k in EXACT_STATS:
        assert got["episode_stats"][k] == want["episode_stats"][k], k
    # the real env has no list at all when every job was blocked
    assert list(got["episode_stats"].get("job_completion_time", [])) == \
        list(want["episode_stats"].get("job_completion_time", []))
    if return_rtol is None:
        assert got["episode_return"] == want["episode_return"]
    else:
        np.testing.assert_allclose(got["episode_return"],
                                   want["episode_return"], rtol=return_rtol)


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", DETERMINISTIC)
def test_engine_eval_loop_matches_eval_loop(jobs_dir, cpu_loop, name):
    seeds = [3, 1799]
    cpu_loop.actor = _heuristic(name)
    got = cpu_loop.run(seeds)
    assert [r["seed"] for r in got] == seeds
    preload = _memo_preload_for_env(cpu_loop.spec)
    for r in got:
        kwargs = {"max_partitions_per_op": SIP_CAP} if name == "sip_ml" else {}
        env = make_env(jobs_dir)
        env.lookahead_memo_preload = preload
        want = EvalLoop(ACTORS[name](**kwargs), env).run(seed=r["seed"])
        assert want["num_actor_steps"] == 200
        _assert_same_episode(r, want, return_rtol=1e-12)
        for k in ("mean_job_completion_time",
                  "mean_job_completion_time_speedup"):
            assert r[k] == want[k], k
        assert set(want) <= set(r)


@pytest.mark.parametrize("reward,kwargs", [
    ("lookahead_job_completion_time", None),
    ("lookahead_job_completion_time",
     {"normaliser": "job_sequential_completion_time_times_fail_reward_factor",
      "fail_reward_factor": 2.0, "transform_with_log": True}),
    ("multi_objective_jct_blocking", None)])
def test_last_step_reward_matches_env(jobs_dir, reward, kwargs):
    """Seed 1799 ends with a job placed on the last step and still running
    at max_simulation_run_time: the env blocks it at finalisation before it
    extracts the reward, so that step pays the fail reward.  Every step's
    engine reward (the last one included) equals the env's."""
    env_fn = lambda: make_env(jobs_dir, reward, kwargs)
    loop = EngineEvalLoop(_heuristic("min_parallelism"), env_fn, "cpu")
    got = loop.run([1799])[0]
    env = env_fn()
    env.lookahead_memo_preload = _memo_preload_for_env(loop.spec)
    obs = env.reset(seed=1799)
    actor, rewards, done = ACTORS["min_parallelism"](), [], False
    while not done:
        obs, r, done, _ = env.step(actor.compute_action(obs))
        rewards.append(r)
    assert len(rewards) == got["num_actor_steps"] == 200
    es = got["episode_stats"]
    ret = 0.0
    for r in rewards:
        ret += r
    assert got["episode_return"] == ret
    assert es["episode_return"] == ret      # the engine's own ep_return too


def test_engine_eval_loop_waves_and_random(cpu_loop):
    """More seeds than envs run in waves with the same per-seed results; the
    random actor only ever plays valid actions (the engine accepts them)."""
    cpu_loop.actor = _heuristic("acceptable_jct")
    one = cpu_loop.run([3, 1799, 5])
    cpu_loop.num_envs = 2
    try:
        waves = cpu_loop.run([3, 1799, 5])
    finally:
        cpu_loop.num_envs = None
    for a, b in zip(one, waves):
        _assert_same_episode(a, b)
    cpu_loop.actor = DeviceActor.heuristic("random", seed=9)
    r1 = cpu_loop.run([3])
    r2 = cpu_loop.run([3])
    _assert_same_episode(r1[0], r2[0])
    assert r1[0]["num_actor_steps"] == 200


def _policy(num_actions=17, seed=GREEDY_POLICY_SEED):
    from ddls_amd.models.gnn import GNNPolicy
    torch.manual_seed(seed)
    return GNNPolicy(num_actions=num_actions)


def _venv(jobs_dir, device, base_seed=ROLLOUT_BASE_SEED, num_envs=8,
          like=None):
    """``like``: an env whose compiled spec (and proto env) to share."""
    return EngineVectorEnv(lambda: make_env(jobs_dir), num_envs=num_envs,
                           device=device, base_seed=base_seed,
                           spec=like.spec if like else None,
                           proto_env=like.proto_env if like else None)


def test_rollout_device_sampler_cpu_backend(jobs_dir):
    policy = _policy()
    ref = _venv(jobs_dir, "cpu", num_envs=4).rollout(policy, 5)
    a = _venv(jobs_dir, "cpu", num_envs=4).rollout(policy, 5,
                                                   sampler="device")
    b = _venv(jobs_dir, "cpu", num_envs=4).rollout(policy, 5,
                                                   sampler="device")
    assert set(a) == set(ref)
    for k in ref:
        if k == "obs":
            assert len(a[k]) == len(ref[k])
            continue
        assert a[k].shape == ref[k].shape and a[k].dtype == ref[k].dtype, k
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    T, B = a["actions"].shape
    masks = np.stack([o.action_mask for o in a["obs"]]).reshape(T, B, -1)
    t_idx, b_idx = np.meshgrid(np.arange(T), np.arange(B), indexing="ij")
    assert (masks[t_idx, b_idx, a["actions"]] > 0).all()
    np.testing.assert_array_equal(
        a["logp"], a["lp_all"][t_idx, b_idx, a["actions"]])
    for o, o2 in zip(a["obs"], b["obs"]):
        np.testing.assert_array_equal(o.graph_features, o2.graph_features)
    # a second rollout on the same env draws fresh uniforms
    env = _venv(jobs_dir, "cpu", num_envs=4)
    env.rollout(policy, 5, sampler="device")
    assert env._sampler_step == 5
    with pytest.raises(ValueError):
        env.rollout(policy, 1, sampler="numpy")

    dr = _venv(jobs_dir, "cpu", num_envs=4).rollout(
        policy, 5, device_resident=True, sampler="device")
    ref_dr = _venv(jobs_dir, "cpu", num_envs=4).rollout(
        policy, 5, device_resident=True)
    assert set(dr) == set(ref_dr)
    for k in ref_dr:
        if k == "obs":
            continue
        assert dr[k].shape == ref_dr[k].shape and dr[k].dtype == ref_dr[k].dtype, k
    np.testing.assert_array_equal(dr["actions"], a["actions"])
    np.testing.assert_array_equal(dr["actions_dev"].numpy(),
                                  a["actions"].reshape(-1))
    np.testing.assert_array_equal(dr["logp_dev"].numpy(),
                                  a["logp"].reshape(-1))


def test_ppo_config_forwards_rollout_sampler(jobs_dir):
    from ddls_amd.rl.ppo import PPOConfig, PPOTrainer
    assert PPOConfig().rollout_sampler == "torch"
    env = _venv(jobs_dir, "cpu", num_envs=4)
    trainer = PPOTrainer(env, _policy(), PPOConfig(
        train_batch_size=8, sgd_minibatch_size=8, num_sgd_iter=1,
        rollout_sampler="device"), device=torch.device("cpu"))
    trainer.collect_rollout(2)
    assert env._sampler_step == 2


def test_eval_heuristic_cli_engine_backend(tmp_path):
    from ddls_amd.workloads import generate_model, write_pipedream_txt
    d = tmp_path / "jobs"
    d.mkdir()
    nodes, edges = generate_model("m_a", 6, 1, 0.8, 61)
    write_pipedream_txt(str(d / "m_a.txt"), nodes, edges)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def run(*extra):
        out = subprocess.run(
            [sys.executable, "scripts/eval_heuristic.py", *extra,
             f"env_config.jobs_config.path_to_files={d}",
             "env_config.jobs_config.replication_factor=8",
             "actors=[sip_ml]"],
            cwd=root, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        rows = {}
        for line in out.stdout.splitlines():
            if ": {" in line:
                name, _, payload = line.partition(": ")
                rows[name] = json.loads(payload)
        return rows

    env_rows = run()
    eng_rows = run("--backend", "engine")
    assert set(env_rows) == {"sip_ml"}
    assert set(eng_rows) == {"sip_ml[1799]", "sip_ml[mean]"}
    assert set(eng_rows["sip_ml[1799]"]) == set(env_rows["sip_ml"])
    for k in ("blocking_rate", "mean_job_completion_time"):
        assert eng_rows["sip_ml[1799]"][k] == env_rows["sip_ml"][k], k
        assert eng_rows["sip_ml[mean]"][k] == env_rows["sip_ml"][k], k


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
def _greedy_min_gap(loop, actor, seeds):
    """Run ``loop`` with ``actor`` and return (results, min top-two gap of
    the masked logits over every live env-step with a choice to make)."""
    gaps = []
    real_act = actor.act

    def act(eng, step, rows=None):
        T = eng.T
        live = (T["done"] == 0) & (T["obs_mask"].sum(1) > 1)
        gfull = torch.cat([T["obs_gf"], T["obs_mask"]], dim=1)
        logits, _ = policy_head_reference(
            actor.policy_net, actor.model_emb, T["obs_model"].long(), gfull,
            T["obs_mask"])
        top = torch.topk(logits, 2, dim=1).values
        gaps.extend((top[:, 0] - top[:, 1])[live].tolist())
        return real_act(eng, step, rows)

    actor.act = act
    try:
        loop.actor = actor
        results = loop.run(seeds)
    finally:
        del actor.act
    return results, min(gaps)


def test_greedy_policy_reference_gap(cpu_loop):
    """Precondition of the GPU greedy comparison, checkable on the CPU."""
    actor = DeviceActor.policy(_policy(), deterministic=True)
    results, gap = _greedy_min_gap(cpu_loop, actor, [3, 1799, 5])
    assert gap >= 1e-3, gap
    assert all(r["num_actor_steps"] == 200 for r in results)


@pytest.mark.gpu
def test_engine_eval_loop_gpu_matches_cpu(jobs_dir, cpu_loop):
    seeds = [3, 1799, 5]
    # same compiled spec on both sides: this test is about the actors and
    # the engines, not about the two lookahead backends
    gpu_loop = EngineEvalLoop(None, None, "cuda:0", spec=cpu_loop.spec,
                              proto_env=cpu_loop.proto_env)
    for name in DETERMINISTIC:
        cpu_loop.actor = _heuristic(name)
        gpu_loop.actor = _heuristic(name)
        for got, want in zip(gpu_loop.run(seeds), cpu_loop.run(seeds)):
            _assert_same_episode(got, want)
    cpu_actor = DeviceActor.policy(_policy(), deterministic=True)
    want, gap = _greedy_min_gap(cpu_loop, cpu_actor, seeds)
    assert gap >= 1e-3, gap
    gpu_loop.actor = DeviceActor.policy(_policy().to("cuda:0"),
                                        deterministic=True)
    for g, w in zip(gpu_loop.run(seeds), want):
        _assert_same_episode(g, w)


def _cdf_margin(data):
    """Smallest distance of a rollout's uniforms from a CDF boundary."""
    cum = np.cumsum(np.exp(data["lp_all"].astype(np.float64)), axis=-1)
    return np.abs(cum - data["u"][..., None]).min()


def _rollout_with_u(env, policy, steps):
    """rollout(sampler="device") that also returns the uniforms it drew."""
    from ddls_amd.rl.device_actor import philox_uniform
    step0 = env._sampler_step
    data = env.rollout(policy, steps, sampler="device")
    data["u"] = np.stack([philox_uniform(env.base_seed, step0 + t,
                                         env.num_envs)
                          for t in range(steps)])
    return data


def test_rollout_device_sampler_reference_margin(jobs_dir):
    """Precondition of the GPU rollout comparison, checkable on the CPU."""
    data = _rollout_with_u(_venv(jobs_dir, "cpu"), _policy(), 6)
    assert _cdf_margin(data) >= 1e-4


@pytest.mark.gpu
def test_rollout_device_sampler_gpu_matches_cpu(jobs_dir):
    cpu_env = _venv(jobs_dir, "cpu")
    want = _rollout_with_u(cpu_env, _policy(), 6)
    assert _cdf_margin(want) >= 1e-4
    got = _venv(jobs_dir, "cuda:0", like=cpu_env).rollout(
        _policy().to("cuda:0"), 6, sampler="device")
    assert got["actions"].shape == (6, 8)
    for k in ("actions", "rewards", "dones"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    masks = np.stack([o.action_mask for o in want["obs"]]).reshape(6, 8, -1)
    np.testing.assert_allclose(got["logp"], want["logp"], atol=1e-4, rtol=0)
    np.testing.assert_allclose(got["values"], want["values"], atol=1e-4,
                               rtol=0)
    np.testing.assert_allclose(got["lp_all"][masks > 0],
                               want["lp_all"][masks > 0], atol=1e-4, rtol=0)
    for o, o2 in zip(got["obs"], want["obs"]):
        np.testing.assert_array_equal(o.graph_features, o2.graph_features)
