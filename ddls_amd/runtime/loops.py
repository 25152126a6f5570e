"""Training/eval loops + launcher.

Reference: ``ddls/loops/rllib_epoch_loop.py:34`` (epoch = one trainer.train()),
``rllib_eval_loop.py:11`` (checkpoint rollout eval), ``eval_loop.py:14``
(heuristic actor eval), ``ddls/launchers/launcher.py:17`` (run-until loop with
checkpoint/log cadence and best-checkpoint tracking).
"""
from __future__ import annotations

import time
from collections import defaultdict
from typing import Callable, Dict, List, Optional

import numpy as np

from .checkpointer import Checkpointer
from .logger import Logger


class EpochLoop:
    """One epoch = one PPO iteration (rollout + SGD update)."""

    def __init__(self, trainer):
        self.trainer = trainer
        self.best_eval_reward = -float("inf")
        self.best_checkpoint_paths: List[str] = []

    def run(self) -> Dict:
        t0 = time.perf_counter()
        stats = self.trainer.train()
        stats["epoch_time_s"] = time.perf_counter() - t0
        return stats

    def state_dict(self):
        return self.trainer.state_dict()


class EvalLoop:
    """Roll a heuristic actor (or a policy actor) through full episodes and
    harvest the cluster's episode stats (reference ``eval_loop.py:26-129``)."""

    def __init__(self, actor, env, max_steps: int = 100000):
        self.actor = actor
        self.env = env
        self.max_steps = max_steps

    def run(self, seed: Optional[int] = None, verbose: bool = False) -> Dict:
        obs = self.env.reset(seed=seed)
        done, steps = False, 0
        rewards = []
        t0 = time.perf_counter()
        while not done and steps < self.max_steps:
            job_to_place = next(iter(self.env.cluster.job_queue.jobs.values()))
            action = self.actor.compute_action(obs, job_to_place=job_to_place)
            obs, reward, done, info = self.env.step(int(action))
            rewards.append(reward)
            steps += 1
        results = {
            "episode_stats": dict(self.env.cluster.episode_stats),
            "num_actor_steps": steps,
            "episode_return": float(np.sum(rewards)),
            "mean_reward": float(np.mean(rewards)) if rewards else 0.0,
            "run_time": time.perf_counter() - t0,
        }
        es = results["episode_stats"]
        for key in ("job_completion_time", "job_completion_time_speedup"):
            vals = es.get(key, [])
            results[f"mean_{key}"] = float(np.mean(vals)) if len(vals) else None
        results["blocking_rate"] = es.get("blocking_rate", None)
        results["acceptance_rate"] = es.get("acceptance_rate", None)
        return results


class EngineEvalLoop:
    """``EvalLoop`` over many seeds at once on the vectorised env engine.

    One env per seed: env b plays ``drain_episode_schedule(gen, spec,
    seed=seeds[b])``, the episode ``env.reset(seed=seeds[b])`` plays, with a
    ``rl.device_actor.DeviceActor`` acting for the whole batch per step (one
    launch on a ``GpuEngine``).  Nothing is reset: finished envs stay done
    and the engine skips them.  More seeds than ``num_envs`` run in waves.

    ``run(seeds)`` returns one dict per seed with ``EvalLoop.run``'s keys
    plus ``seed``.  ``episode_return`` is the f64 sum of ``T["reward"]`` in
    step order over the steps the env was live for (a skipped env keeps a
    stale reward) — not the engine's own ``ep_return``.
    """

    def __init__(self, actor, env_fn, device, num_envs: Optional[int] = None,
                 max_steps: int = 100000, spec=None, proto_env=None):
        import torch
        from ..cluster.vec_engine import compile_engine_spec
        from ..rl.engine_env import build_models_batch
        self.actor = actor
        self.device = torch.device(device)
        self.num_envs = num_envs
        self.max_steps = max_steps
        if proto_env is None:
            proto_env = env_fn()
            proto_env.reset(seed=987654321)
        self.proto_env = proto_env
        if spec is None:
            # raises the engine's ValueError for configs it does not support
            spec = compile_engine_spec(
                proto_env, lookahead_device=self.device
                if self.device.type == "cuda" else None)
        self.spec = spec
        self.gen = proto_env.cluster.jobs_generator
        self._models_batch = build_models_batch(self.spec, self.device)

    def _make_engine(self, scheds):
        cap = max(s.n for s in scheds) + 8
        if self.device.type == "cuda":
            from ..cluster.gpu_engine import GpuEngine
            eng = GpuEngine(self.spec, B=len(scheds), device=self.device,
                            n_jobs_cap=cap)
        else:
            from ..cluster.vec_engine import CpuEngine
            eng = CpuEngine(self.spec, B=len(scheds), n_jobs_cap=cap)
        for b, sched in enumerate(scheds):
            eng.reset_env(b, sched)
        return eng

    def _run_wave(self, seeds: List[int]) -> List[Dict]:
        import torch
        from ..cluster.vec_engine import drain_episode_schedule
        t0 = time.perf_counter()
        scheds = [drain_episode_schedule(self.gen, self.spec, seed=int(s))
                  for s in seeds]
        eng = self._make_engine(scheds)
        B = len(seeds)
        dev = eng.T["reward"].device
        ret = torch.zeros(B, dtype=torch.float64, device=dev)
        nsteps = torch.zeros(B, dtype=torch.int64, device=dev)
        step = 0
        while step < self.max_steps:
            live = eng.T["done"] == 0
            if not bool(live.any()):
                break
            actions = self.actor.act(eng, step)
            eng.step(actions)
            # only envs that were live before the step earned this reward
            ret = torch.where(live, ret + eng.T["reward"], ret)
            nsteps += live.to(torch.int64)
            step += 1
        ret = ret.cpu().numpy()
        nsteps = nsteps.cpu().numpy()
        run_time = time.perf_counter() - t0
        out = []
        for b, seed in enumerate(seeds):
            es = eng.episode_stats(b)
            n = int(nsteps[b])
            r = {
                "seed": int(seed),
                "episode_stats": es,
                "num_actor_steps": n,
                "episode_return": float(ret[b]),
                "mean_reward": float(ret[b] / n) if n else 0.0,
                # the wave's wall time, shared by its envs
                "run_time": run_time,
            }
            for key in ("job_completion_time", "job_completion_time_speedup"):
                vals = es.get(key, [])
                r[f"mean_{key}"] = float(np.mean(vals)) if len(vals) else None
            r["blocking_rate"] = es.get("blocking_rate", None)
            r["acceptance_rate"] = es.get("acceptance_rate", None)
            out.append(r)
        return out

    def run(self, seeds) -> List[Dict]:
        seeds = [int(s) for s in seeds]
        self.actor.prepare(self)
        width = self.num_envs or max(len(seeds), 1)
        results: List[Dict] = []
        for i in range(0, len(seeds), width):
            results.extend(self._run_wave(seeds[i:i + width]))
        return results


class PolicyActor:
    """Greedy/stochastic actor wrapping a trained GNNPolicy for EvalLoop."""

    def __init__(self, policy, device=None, deterministic: bool = True,
                 name: str = "gnn_policy"):
        import torch
        self.torch = torch
        self.policy = policy
        self.device = device or torch.device("cpu")
        self.policy.to(self.device)
        self.deterministic = deterministic
        self.name = name

    def compute_action(self, obs, *args, **kwargs):
        import torch
        from ..rl.rollout import CompactObs, collate
        with torch.no_grad():
            inputs = collate([CompactObs.from_obs(obs)], self.device)
            logits, _ = self.policy.forward_flat(
                inputs["batch"], inputs["graph_features"], inputs["action_mask"])
            if self.deterministic:
                return int(torch.argmax(logits, dim=-1).item())
            return int(torch.distributions.Categorical(logits=logits)
                       .sample().item())

    @classmethod
    def from_checkpoint(cls, checkpoint_path: str, num_actions: int = 17,
                        config: Optional[dict] = None, **kwargs):
        from ..models.gnn import GNNPolicy
        state = Checkpointer.read(checkpoint_path)
        state = state.get("trainer", state)   # launcher full-state layout
        policy = GNNPolicy(num_actions=num_actions, config=config)
        policy.load_state_dict(state["policy"])
        return cls(policy, **kwargs)


class Launcher:
    """Run epochs until a budget is hit; checkpoint + log on a cadence and
    track the best checkpoint by eval episode return
    (reference ``launcher.py:97-184``, ``rllib_epoch_loop.py:144-230``)."""

    def __init__(self,
                 epoch_loop: EpochLoop,
                 num_epochs: Optional[int] = None,
                 max_actor_steps: Optional[int] = None,
                 evaluation_interval: int = 10,
                 eval_fn: Optional[Callable[[], Dict]] = None,
                 path_to_save: Optional[str] = None,
                 use_sqlite_database: bool = False,
                 external_logger=None,
                 verbose: bool = True):
        self.epoch_loop = epoch_loop
        self.num_epochs = num_epochs
        self.max_actor_steps = max_actor_steps
        self.evaluation_interval = evaluation_interval
        self.eval_fn = eval_fn
        self.logger = (Logger(path_to_save, use_sqlite_database=use_sqlite_database)
                       if path_to_save else None)
        self.checkpointer = Checkpointer(path_to_save) if path_to_save else None
        self.external_logger = external_logger   # runtime.logger.ExternalLogger
        self.verbose = verbose
        self.results_log = defaultdict(list)
        self.best_eval_return = -float("inf")
        self.best_checkpoint: Optional[str] = None
        self.epoch = 0

    # ------------------------------------------------------------------
    # full-state resume (reference launcher.py:97-184
    # restarts from the RLlib checkpoint — here the launcher's own
    # bookkeeping rides along in the same checkpoint file)
    def _full_state(self) -> Dict:
        return {
            "trainer": self.epoch_loop.state_dict(),
            "launcher": {
                "epoch": self.epoch,
                "results_log": {k: list(v)
                                for k, v in self.results_log.items()},
                "best_eval_return": self.best_eval_return,
                "best_checkpoint": self.best_checkpoint,
            },
        }

    def _write_checkpoint(self, index: int) -> Optional[str]:
        if self.checkpointer is None:
            return None
        return self.checkpointer.write(self._full_state(), index=index)

    def resume(self, checkpoint_path: Optional[str] = None) -> bool:
        """Restore trainer + launcher bookkeeping from a checkpoint (the
        latest one by default).  Returns True if a checkpoint was loaded."""
        if checkpoint_path is None:
            if self.checkpointer is None:
                return False
            checkpoint_path = self.checkpointer.latest()
            if checkpoint_path is None:
                return False
        state = Checkpointer.read(checkpoint_path)
        trainer_state = state.get("trainer", state)   # old flat layout too
        self.epoch_loop.trainer.load_state_dict(trainer_state)
        ls = state.get("launcher")
        if ls is not None:
            self.epoch = int(ls.get("epoch", 0))
            self.results_log = defaultdict(list)
            for k, v in ls.get("results_log", {}).items():
                self.results_log[k] = list(v)
            self.best_eval_return = ls.get("best_eval_return", -float("inf"))
            self.best_checkpoint = ls.get("best_checkpoint")
        return True

    def _should_stop(self, epoch: int, total_steps: int) -> bool:
        if self.num_epochs is not None and epoch >= self.num_epochs:
            return True
        if self.max_actor_steps is not None and total_steps >= self.max_actor_steps:
            return True
        return False

    def run(self) -> Dict:
        epoch = self.epoch
        if self.checkpointer is not None and epoch == 0:
            self._write_checkpoint(index=0)
        while not self._should_stop(epoch, getattr(self.epoch_loop.trainer,
                                                   "total_env_steps", 0)):
            stats = self.epoch_loop.run()
            epoch += 1
            self.epoch = epoch
            for k, v in stats.items():
                if isinstance(v, (int, float, np.floating, np.integer)):
                    self.results_log[k].append(float(v))
            self.results_log["epoch_counter"].append(epoch)
            if self.external_logger is not None:
                self.external_logger.log(stats, step=epoch)

            if epoch % self.evaluation_interval == 0 or self._should_stop(
                    epoch, getattr(self.epoch_loop.trainer, "total_env_steps", 0)):
                if self.eval_fn is not None:
                    eval_results = self.eval_fn()
                    ret = eval_results.get("episode_return", None)
                    self.results_log["eval_episode_return"].append(ret)
                    if ret is not None and ret > self.best_eval_return:
                        self.best_eval_return = ret
                        self.best_checkpoint = self._write_checkpoint(epoch)
                    else:
                        self._write_checkpoint(epoch)
                else:
                    self._write_checkpoint(epoch)
                if self.logger is not None:
                    self.logger.write({"train_log": dict(self.results_log)})
            if self.verbose:
                msg = (f"epoch {epoch}: loss={stats.get('total_loss', 0):.4f} "
                       f"kl={stats.get('kl', 0):.5f} "
                       f"reward={stats.get('mean_reward', 0):.3f}")
                if "episode_reward_mean" in stats:
                    msg += f" ep_ret={stats['episode_reward_mean']:.2f}"
                print(msg, flush=True)
        if self.logger is not None:
            self.logger.write({"train_log": dict(self.results_log)}, block=True)
        return dict(self.results_log)
