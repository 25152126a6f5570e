"""Evolution Strategies — the reference's fifth algorithm config group
(``scripts/.../algo/es.yaml`` -> ray.rllib.agents.es.ESTrainer, OpenAI-ES:
antithetic Gaussian perturbations, centered-rank fitness shaping, l2 decay;
reference hparams noise_stdev 0.02, stepsize 0.01, l2_coeff 0.005).

Synchronous variant: perturbation pairs are evaluated sequentially on the
(shared) vectorised env as fixed-length fragments whose mean per-step reward
is the fitness (the engine makes fragment evaluation cheap); RLlib's
distributed noise table + full-episode returns are replaced accordingly —
an honest simplification of APEX-style actor fan-out, not of the ES math.

``ESConfig.evaluator = "population"`` (opt-in, engine envs only) replaces the
member loop with ``rl/es_population.py``: all 2 * pairs members play whole
episodes at once on one engine of 2 * pairs * envs_per_member envs, every
member on the same schedules and the same sampling uniforms (common random
numbers), with Philox noise keyed by ``(noise_seed, iteration)`` and tie-safe
ranks.  The sequential evaluator is the default and is unchanged.
"""
from __future__ import annotations

import sys
import time
from dataclasses import dataclass
from typing import Dict, Optional

import numpy as np
import torch


@dataclass
class ESConfig:
    # reference algo/es.yaml values
    noise_stdev: float = 0.02
    stepsize: float = 0.01
    l2_coeff: float = 0.005
    perturbation_pairs: int = 16
    fragment_steps: int = 16
    # "sequential": the members play fragment_steps rollouts one after the
    # other on the trainer's env.  "population" (opt-in): all 2 * pairs
    # members play whole episodes at once on an engine of 2 * pairs *
    # envs_per_member envs with common random numbers (rl/es_population.py)
    evaluator: str = "sequential"
    envs_per_member: int = 8
    eval_max_steps: int = 100000
    noise_seed: int = 0
    deterministic_eval: bool = False


EVALUATORS = ("sequential", "population")


def centered_ranks(x: np.ndarray) -> np.ndarray:
    """RLlib es_utils.compute_centered_ranks: ranks scaled to [-0.5, 0.5]."""
    ranks = np.empty(len(x), dtype=np.float64)
    ranks[x.argsort()] = np.arange(len(x))
    return ranks / (len(x) - 1) - 0.5


def centered_ranks_ties(x: np.ndarray) -> np.ndarray:
    """``centered_ranks`` with equal values sharing their average rank: the
    same numbers when all values are distinct, and a tied antithetic pair
    gets weight exactly 0 instead of argsort's arbitrary order."""
    x = np.asarray(x)
    order = x.argsort(kind="stable")
    xs = x[order]
    ranks = np.empty(len(x), dtype=np.float64)
    i = 0
    while i < len(x):
        j = i
        while j + 1 < len(x) and xs[j + 1] == xs[i]:
            j += 1
        ranks[order[i:j + 1]] = 0.5 * (i + j)
        i = j + 1
    return ranks / (len(x) - 1) - 0.5


def count_tied_pairs(fitness: np.ndarray) -> int:
    """Antithetic pairs ``(2k, 2k + 1)`` with exactly equal fitness."""
    fitness = np.asarray(fitness)
    return int(np.sum(fitness[0::2] == fitness[1::2]))


class ESTrainer:
    """Same trainer-facing interface as the gradient trainers."""

    def __init__(self, vector_env, policy, config: Optional[ESConfig] = None,
                 device: Optional[torch.device] = None):
        self.env = vector_env
        self.config = config or ESConfig()
        self.device = device or torch.device(
            "cuda" if torch.cuda.is_available() else "cpu")
        self.policy = policy.to(self.device)
        self.obs = self.env.reset()
        self.total_env_steps = 0
        self.iteration = 0
        self._params = [p for p in self.policy.parameters()]
        self._numel = sum(p.numel() for p in self._params)
        if self.config.evaluator not in EVALUATORS:
            raise ValueError(f"ESConfig.evaluator must be one of {EVALUATORS}"
                             f", not {self.config.evaluator!r}")
        self._population = None
        self._warned_population = False

    def _population_evaluator(self):
        """The PopulationEvaluator when the config asks for it and the env
        can serve it; None (after one warning) otherwise."""
        if self.config.evaluator != "population":
            return None
        if not getattr(self.env, "supports_population_eval", False):
            if not self._warned_population:
                self._warned_population = True
                print("[es] evaluator='population' needs an EngineVectorEnv; "
                      f"{type(self.env).__name__} has no population "
                      "evaluation: running the sequential evaluator",
                      file=sys.stderr)
            return None
        if self._population is None:
            from .es_population import PopulationEvaluator
            cfg = self.config
            self._population = PopulationEvaluator(
                self.env, self.policy, cfg.perturbation_pairs,
                cfg.envs_per_member, eval_max_steps=cfg.eval_max_steps,
                noise_seed=cfg.noise_seed,
                deterministic=cfg.deterministic_eval)
        return self._population

    def _get_flat(self) -> torch.Tensor:
        return torch.cat([p.detach().reshape(-1) for p in self._params])

    @torch.no_grad()
    def _set_flat(self, flat: torch.Tensor):
        off = 0
        for p in self._params:
            n = p.numel()
            p.copy_(flat[off:off + n].view(p.shape))
            off += n

    @torch.no_grad()
    def _fitness(self, steps: int) -> float:
        data = self.env.rollout(self.policy, steps) \
            if hasattr(self.env, "rollout") else self._inline_rollout(steps)
        self.total_env_steps += int(np.prod(np.asarray(
            data["rewards"]).shape))
        return float(np.mean(data["rewards"]))

    def _inline_rollout(self, steps: int):
        from .rollout import collate
        rews = []
        for _ in range(steps):
            inputs = collate(self.obs, self.device)
            logits, _ = self.policy.forward_flat(
                inputs["batch"], inputs["graph_features"],
                inputs["action_mask"])
            actions = torch.distributions.Categorical(
                logits=logits).sample().cpu().numpy()
            self.obs, r, _dones = self.env.step(actions)
            rews.append(r)
        return {"rewards": np.stack(rews)}

    def _train_population(self, ev) -> Dict[str, float]:
        """One generation with the population evaluator: noise, population
        and update run where the engine lives; ranks stay on the host."""
        from .es_population import es_pair_weights, es_update_scalars
        cfg = self.config
        t0 = time.perf_counter()
        gen = self.iteration
        theta = self._get_flat().to(ev.device)
        eps, pop = ev.perturb(theta, cfg.noise_stdev, gen)
        res = ev.evaluate(pop, gen)
        fitness = res["fitness"]
        w = es_pair_weights(centered_ranks_ties(fitness))
        scale, decay = es_update_scalars(cfg.perturbation_pairs,
                                         cfg.noise_stdev, cfg.stepsize,
                                         cfg.l2_coeff)
        self._set_flat(ev.update(theta, eps, w, scale, decay))
        self.iteration += 1
        self.total_env_steps += res["live_steps"]
        return {
            "iteration": self.iteration,
            "fitness_mean": float(np.mean(fitness)),
            "fitness_max": float(np.max(fitness)),
            "total_loss": -float(np.mean(fitness)),   # for generic loops
            "mean_reward": float(np.mean(fitness)),
            "total_env_steps": self.total_env_steps,
            "update_time_s": time.perf_counter() - t0,
            "evaluator": 1,
            "eval_steps": res["eval_steps"],
            "truncated_envs": res["truncated_envs"],
            "tied_pairs": count_tied_pairs(fitness),
            "episode_reward_mean": float(np.mean(res["returns"])),
        }

    def train(self, num_steps: Optional[int] = None) -> Dict[str, float]:
        cfg = self.config
        ev = self._population_evaluator()
        if ev is not None:
            return self._train_population(ev)
        steps = num_steps or cfg.fragment_steps
        t0 = time.perf_counter()
        theta = self._get_flat()
        rng = np.random.RandomState(self.iteration)
        eps = []
        fitness = []
        for _k in range(cfg.perturbation_pairs):
            e = torch.as_tensor(
                rng.randn(self._numel).astype(np.float32),
                device=theta.device)
            eps.append(e)
            for sign in (1.0, -1.0):
                self._set_flat(theta + sign * cfg.noise_stdev * e)
                fitness.append(self._fitness(steps))
        ranks = centered_ranks(np.asarray(fitness))
        grad = torch.zeros_like(theta)
        for k, e in enumerate(eps):
            grad += float(ranks[2 * k] - ranks[2 * k + 1]) * e
        grad /= (2 * cfg.perturbation_pairs * cfg.noise_stdev)
        theta = theta + cfg.stepsize * grad - cfg.stepsize * cfg.l2_coeff * theta
        self._set_flat(theta)
        self.iteration += 1
        stats = {
            "iteration": self.iteration,
            "fitness_mean": float(np.mean(fitness)),
            "fitness_max": float(np.max(fitness)),
            "total_loss": -float(np.mean(fitness)),   # for generic loops
            "mean_reward": float(np.mean(fitness)),
            "total_env_steps": self.total_env_steps,
            "update_time_s": time.perf_counter() - t0,
            "evaluator": 0,
        }
        episode_stats = getattr(self.env, "drain_episode_stats", lambda: [])()
        if episode_stats:
            stats["episode_reward_mean"] = float(np.mean(
                [s["episode_return"] for s in episode_stats]))
        return stats

    def state_dict(self) -> Dict:
        return {"policy": self.policy.state_dict(),
                "iteration": self.iteration,
                "total_env_steps": self.total_env_steps, "algo": "es"}

    def load_state_dict(self, state: Dict):
        self.policy.load_state_dict(state["policy"])
        self.iteration = state.get("iteration", 0)
        self.total_env_steps = state.get("total_env_steps", 0)
