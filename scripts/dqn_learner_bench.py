#!/usr/bin/env python3
"""DQN iterations on the GPU env engine: the device learner (device replay
ring + fused TD-loss kernels, rl/dqn.py ``learner="device"``) against the
torch learner (host list replay + autograd loss) on the env_mi355x config at
the operating point of configs/algo/apex_dqn.yaml, alternating in one
process.

Prints one JSON object: per learner the mean, median, standard deviation,
minimum and maximum of ``update_time_s`` and ``rollout_time_s`` over the
timed iterations (warm-up iterations excluded), every sample, and the ratio
of the two mean update times.  Both learners start from the same weights and
draw the same minibatch indices; their rollouts differ only in what they
return (flat device tensors against T*N host observations), which is what
``rollout_time_s`` shows.

The timer is a host clock around each phase, and each phase ends in
``torch.cuda.synchronize()``.  ``--count-launches`` also runs one device
update under the torch profiler and reports the number of kernels it
launched.  GPU only.

``--prioritized`` runs both learners with ``prioritized_replay`` on (the
yaml's alpha, beta and eps): the device learner with the sum-tree kernels of
ops/hip/per_replay.hip, the torch learner with the host numpy tree.  The
launch count then also reports the ``per_`` kernels, expected to be
1 + 2 * num_sgd_iter per update (one ``per_ingest_kernel``, and per minibatch
one ``per_sample_kernel`` and one ``per_update_kernel``): 9 at the yaml's
num_sgd_iter = 4.

Usage: python scripts/dqn_learner_bench.py [--envs 256] [--iters 10]
           [--warmup 2] [--prioritized] [--count-launches] [--out FILE]
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
import yaml


def summary(xs):
    a = np.asarray(xs, dtype=np.float64)
    return {"mean": float(a.mean()), "median": float(np.median(a)),
            "std": float(a.std(ddof=1)) if len(a) > 1 else 0.0,
            "min": float(a.min()), "max": float(a.max()),
            "all": [float(x) for x in a]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--iters", type=int, default=10,
                    help="timed iterations per learner")
    ap.add_argument("--warmup", type=int, default=2,
                    help="untimed iterations per learner")
    ap.add_argument("--prioritized", action="store_true",
                    help="prioritized replay in both learners")
    ap.add_argument("--count-launches", action="store_true")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("dqn_learner_bench.py needs a GPU")
    dev = torch.device("cuda:0")

    from ddls_amd.cluster.vec_engine import compile_engine_spec
    from ddls_amd.models.gnn import GNNPolicy
    from ddls_amd.rl.dqn import DQNConfig, DQNTrainer
    from ddls_amd.rl.engine_env import EngineVectorEnv
    from ddls_amd.runtime.config import build_env_from_config, load_config

    cfg = load_config(os.path.join(ROOT, "configs", "heuristic_config.yaml"),
                      overrides=["env_config=env_mi355x"])
    with open(os.path.join(ROOT, "configs", "algo", "apex_dqn.yaml")) as f:
        algo = yaml.safe_load(f)

    def env_fn():
        env = build_env_from_config(cfg)
        env.reuse_jobs_generator = True
        return env

    # the config is built and compiled once; both envs share spec and proto
    proto = env_fn()
    proto.reset(seed=987654321)
    spec = compile_engine_spec(proto, lookahead_device=dev)
    num_actions = cfg["env_config"].get("max_partitions_per_op", 16) + 1
    steps = max(1, algo["train_batch_size"] // args.envs)

    def trainer(learner):
        venv = EngineVectorEnv(env_fn, num_envs=args.envs, device=dev,
                               base_seed=0, spec=spec, proto_env=proto)
        torch.manual_seed(0)
        policy = GNNPolicy(num_actions=num_actions).to(dev)
        return DQNTrainer(venv, policy, DQNConfig(
            gamma=algo["gamma"], lr=algo["lr"], n_step=algo["n_step"],
            double_q=algo["double_q"], dueling=algo["dueling"],
            target_network_update_freq=algo["target_network_update_freq"],
            v_min=algo["v_min"], v_max=algo["v_max"],
            train_batch_size=algo["train_batch_size"],
            sgd_minibatch_size=algo["sgd_minibatch_size"],
            num_sgd_iter=algo["num_sgd_iter"], learner=learner,
            prioritized_replay=args.prioritized,
            prioritized_replay_alpha=algo["prioritized_replay_alpha"],
            prioritized_replay_beta=algo["prioritized_replay_beta"],
            prioritized_replay_eps=algo["prioritized_replay_eps"]),
            device=dev)

    trainers = {"torch": trainer("torch"), "device": trainer("device")}
    sync = torch.cuda.synchronize

    def iteration(name):
        tr = trainers[name]
        sync()
        t0 = time.perf_counter()
        data = tr.collect_rollout(steps)
        sync()
        t1 = time.perf_counter()
        st = tr.update(data)
        sync()
        t2 = time.perf_counter()
        tr.iteration += 1
        return t1 - t0, t2 - t1, st

    for _ in range(args.warmup):
        for name in trainers:
            iteration(name)
    rollout = {name: [] for name in trainers}
    update = {name: [] for name in trainers}
    last = {}
    for _ in range(args.iters):
        for name in trainers:
            r, u, st = iteration(name)
            rollout[name].append(r)
            update[name].append(u)
            last[name] = st
    out = {"envs": args.envs, "steps_per_iteration": steps,
           "sgd_minibatch_size": algo["sgd_minibatch_size"],
           "num_sgd_iter": algo["num_sgd_iter"], "n_step": algo["n_step"],
           "iters": args.iters, "warmup": args.warmup,
           "prioritized": args.prioritized}
    for name in trainers:
        assert last[name]["learner"] == (1 if name == "device" else 0)
        assert last[name]["total_loss"] > 0, "the timed updates must train"
        out[name] = {"update_time_s": summary(update[name]),
                     "rollout_time_s": summary(rollout[name]),
                     "replay": last[name]["replay"],
                     "total_loss": last[name]["total_loss"]}
        if args.prioritized:
            out[name]["is_weight_mean"] = last[name]["is_weight_mean"]
            out[name]["max_priority"] = last[name]["max_priority"]
    out["update_time_ratio_torch_over_device"] = (
        out["torch"]["update_time_s"]["mean"]
        / out["device"]["update_time_s"]["mean"])
    out["rollout_time_ratio_torch_over_device"] = (
        out["torch"]["rollout_time_s"]["mean"]
        / out["device"]["rollout_time_s"]["mean"])

    def emit():
        line = json.dumps(out)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)),
                        exist_ok=True)
            with open(args.out, "w") as f:
                f.write(line + "\n")

    if not args.count_launches:
        emit()
        return
    if args.out:
        emit()   # keep the timings whatever the profiler does

    # kernels launched by one device update(), the ingest included
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    tr = trainers["device"]
    data = tr.collect_rollout(steps)
    sync()
    with profile(activities=[ProfilerActivity.CPU,
                             ProfilerActivity.CUDA]) as prof:
        tr.update(data)
        sync()
    tr.iteration += 1
    names = [e.name for e in prof.events()
             if e.device_type == DeviceType.CUDA
             and not e.name.lower().startswith(("memcpy", "memset"))]
    out["device_update_launches"] = {
        "kernels": len(names),
        "dqn_kernels": sum(n.startswith("dqn_") for n in names),
        # less the ingest (and, prioritized, the per_ingest) launch
        "per_minibatch": (len(names) - (2 if args.prioritized else 1))
        / algo["num_sgd_iter"]}
    if args.prioritized:
        out["device_update_launches"]["per_kernels"] = sum(
            n.startswith("per_") for n in names)
        out["device_update_launches"]["per_kernels_expected"] = \
            1 + 2 * algo["num_sgd_iter"]
    emit()


if __name__ == "__main__":
    main()
