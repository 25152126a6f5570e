#!/usr/bin/env python3
"""ES generations on the GPU env engine: the population evaluator (one
batched rollout of all 2K members, rl/es_population.py) against the
sequential evaluator (2K rollouts one after the other) on the env_mi355x
config, both at B = 2K * E envs, alternating in one process.

Prints one JSON object: per evaluator ms per generation, env steps per
generation and env steps / s; for the population path the split of a
generation into perturb, the P GNN forwards, reset + replicate, the step loop
and the update; and the step loop against ``EngineVectorEnv.rollout(
sampler="device")`` — the single-policy path — at the same B and step count
(the difference is what per-member weights cost).

The timer is a host clock around a generation that ends in
``torch.cuda.synchronize()``.  GPU only.

Usage: python scripts/es_population_bench.py [--pairs 16]
           [--envs-per-member 8] [--eval-max-steps 64] [--generations 3]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=16)
    ap.add_argument("--envs-per-member", type=int, default=8)
    ap.add_argument("--eval-max-steps", type=int, default=64,
                    help="cap of the population rollout (episodes of this "
                         "config run for ~1000 steps)")
    ap.add_argument("--fragment-steps", type=int, default=16)
    ap.add_argument("--generations", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("es_population_bench.py needs a GPU")
    dev = torch.device("cuda:0")

    from ddls_amd.cluster.vec_engine import compile_engine_spec
    from ddls_amd.models.gnn import GNNPolicy
    from ddls_amd.rl.engine_env import EngineVectorEnv
    from ddls_amd.rl.es import (ESConfig, ESTrainer, centered_ranks_ties)
    from ddls_amd.rl.es_population import (es_pair_weights,
                                           es_update_scalars)
    from ddls_amd.runtime.config import build_env_from_config, load_config

    K, E = args.pairs, args.envs_per_member
    B = 2 * K * E
    cfg = load_config(os.path.join(ROOT, "configs", "heuristic_config.yaml"),
                      overrides=["env_config=env_mi355x"])

    def env_fn():
        env = build_env_from_config(cfg)
        env.reuse_jobs_generator = True
        return env

    # the config is built and compiled once; both envs share spec and proto
    proto = env_fn()
    proto.reset(seed=987654321)
    spec = compile_engine_spec(proto, lookahead_device=dev)
    num_actions = cfg["env_config"].get("max_partitions_per_op", 16) + 1

    def trainer(evaluator):
        venv = EngineVectorEnv(env_fn, num_envs=B, device=dev, base_seed=0,
                               spec=spec, proto_env=proto)
        torch.manual_seed(0)
        policy = GNNPolicy(num_actions=num_actions).to(dev)
        return ESTrainer(venv, policy, ESConfig(
            perturbation_pairs=K, fragment_steps=args.fragment_steps,
            evaluator=evaluator, envs_per_member=E,
            eval_max_steps=args.eval_max_steps), device=dev)

    trainers = {"sequential": trainer("sequential"),
                "population": trainer("population")}

    def generation(name):
        tr = trainers[name]
        before = tr.total_env_steps
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tr.train()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, tr.total_env_steps - before

    for _ in range(args.warmup):
        for name in trainers:
            generation(name)
    times = {name: [] for name in trainers}
    steps = {name: [] for name in trainers}
    for _ in range(args.generations):
        for name in trainers:
            dt, n = generation(name)
            times[name].append(dt)
            steps[name].append(n)
    out = {"pairs": K, "envs_per_member": E, "B": B,
           "eval_max_steps": args.eval_max_steps,
           "fragment_steps": args.fragment_steps,
           "generations": args.generations}
    for name in trainers:
        t, n = float(np.median(times[name])), float(np.median(steps[name]))
        out[name] = {"ms_per_generation": t * 1e3,
                     "ms_per_generation_all": [x * 1e3 for x in times[name]],
                     "env_steps_per_generation": n,
                     "env_steps_per_sec": n / t}

    # one more population generation, piece by piece
    tr = trainers["population"]
    ev = tr._population_evaluator()
    c = tr.config
    sync = torch.cuda.synchronize
    theta = tr._get_flat()
    sync()
    t0 = time.perf_counter()
    eps, pop = ev.perturb(theta, c.noise_stdev, tr.iteration)
    sync()
    t1 = time.perf_counter()
    res = ev.evaluate(pop, tr.iteration)
    sync()
    t2 = time.perf_counter()
    w = es_pair_weights(centered_ranks_ties(res["fitness"]))
    scale, decay = es_update_scalars(K, c.noise_stdev, c.stepsize, c.l2_coeff)
    ev.update(theta, eps, w, scale, decay)
    sync()
    t3 = time.perf_counter()
    split = {"perturb_ms": (t1 - t0) * 1e3,
             "gnn_forwards_ms": ev.timings["gnn_s"] * 1e3,
             "reset_replicate_ms": ev.timings["reset_s"] * 1e3,
             "step_loop_ms": ev.timings["steps_s"] * 1e3,
             "update_ms": (t3 - t2) * 1e3,
             "eval_steps": res["eval_steps"],
             "truncated_envs": res["truncated_envs"]}
    split["gnn_share"] = split["gnn_forwards_ms"] / ((t3 - t0) * 1e3)
    out["population_split"] = split

    # the single-policy path at the same B and step count
    venv = trainers["sequential"].env
    policy = trainers["sequential"].policy
    n_steps = max(res["eval_steps"], 1)
    with torch.no_grad():
        venv.rollout(policy, n_steps, device_resident=True, sampler="device")
        sync()
        t0 = time.perf_counter()
        venv.rollout(policy, n_steps, device_resident=True, sampler="device")
        sync()
        single_ms = (time.perf_counter() - t0) * 1e3
    out["step_loop_vs_single_policy"] = {
        "steps": n_steps,
        "population_step_loop_ms": split["step_loop_ms"],
        "single_policy_rollout_ms": single_ms,
        "ratio": split["step_loop_ms"] / single_ms}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
