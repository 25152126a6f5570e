"""Population evaluation for Evolution Strategies on the env engine.

One engine of ``B = P * E`` envs plays all ``P = 2K`` members of a generation
at once: member ``m = 2k + s`` (``s = 0`` is ``+eps_k``, ``s = 1`` is
``-eps_k``) owns engine rows ``[m * E, (m + 1) * E)``, every member plays the
same ``E`` episode schedules, and in sample mode every member draws the same
uniforms — common random numbers, so a fitness difference is the effect of
the perturbation alone.

On a ``GpuEngine`` a generation is ``es_perturb`` (noise + population, one
launch), ``P`` GNN forwards for the per-member embedding tables, one
``actor_population`` launch + one env step per step of the rollout, and
``es_update`` (``ops/hip/es_population.hip``).  On a ``CpuEngine`` the
reference functions below do the same work in numpy / torch.  Each backend is
deterministic on its own; the two are not bit-equal to each other (``logf`` /
``sincosf`` differ in the last bits).

Noise contract (both backends): Philox4x32-10, key ``(seed_lo, seed_hi)`` of
``noise_seed``, counter ``(j, k, gen_lo, gen_hi)`` with ``j = i // 4``; words
``(w0, w1)`` give elements ``4j`` and ``4j + 1``, ``(w2, w3)`` give ``4j + 2``
and ``4j + 3`` by Box-Muller: ``u1 = ((w >> 8) + 1) * 2**-24`` in (0, 1],
``u2 = (w' >> 8) * 2**-24`` in [0, 1), ``r = sqrt(-2 log u1)``,
``a = 6.2831855f * u2``, ``z_even = r cos a``, ``z_odd = r sin a``.
"""
from __future__ import annotations

import copy
import time
from typing import Dict, List

import numpy as np
import torch

from .device_actor import (MODES, POLICY_MODES, act_reference, head_params,
                           philox4x32_10)

_U32 = 0xFFFFFFFF
_U64 = 0xFFFFFFFFFFFFFFFF
_TWO_PI_F32 = float(np.float32(6.2831855))


# ---------------------------------------------------------------------------
# references (numpy / torch): the CpuEngine backend and the GPU tests' oracle
# ---------------------------------------------------------------------------
def es_noise_reference(seed: int, generation: int, K: int,
                       n: int) -> np.ndarray:
    """The noise contract in float64 from the same Philox words, cast to
    float32: ``eps`` [K, n]."""
    seed = int(seed) & _U64
    generation = int(generation) & _U64
    nq = (n + 3) // 4
    ctr = np.zeros((K, nq, 4), dtype=np.uint64)
    ctr[:, :, 0] = np.arange(nq, dtype=np.uint64)[None, :]
    ctr[:, :, 1] = np.arange(K, dtype=np.uint64)[:, None]
    ctr[:, :, 2] = generation & _U32
    ctr[:, :, 3] = generation >> 32
    key = np.array([seed & _U32, seed >> 32], dtype=np.uint64)
    w = philox4x32_10(ctr, np.broadcast_to(key, (K, nq, 2)))
    z = np.empty((K, nq, 4), dtype=np.float64)
    for half in (0, 1):
        wa = w[..., 2 * half].astype(np.uint64)
        wb = w[..., 2 * half + 1].astype(np.uint64)
        u1 = ((wa >> np.uint64(8)) + np.uint64(1)).astype(np.float64) \
            * 2.0 ** -24
        u2 = (wb >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
        r = np.sqrt(-2.0 * np.log(u1))
        a = _TWO_PI_F32 * u2
        z[..., 2 * half] = r * np.cos(a)
        z[..., 2 * half + 1] = r * np.sin(a)
    return z.reshape(K, nq * 4)[:, :n].astype(np.float32)


def es_population_reference(theta: np.ndarray, eps: np.ndarray,
                            sigma: float) -> np.ndarray:
    """``pop`` [2K, n] in numpy f32: ``t = sigma * eps`` is one rounded
    product, ``pop[2k] = theta + t`` and ``pop[2k + 1] = theta - t``."""
    theta = np.asarray(theta, dtype=np.float32)
    eps = np.asarray(eps, dtype=np.float32)
    t = np.float32(sigma) * eps
    pop = np.empty((2 * eps.shape[0], eps.shape[1]), dtype=np.float32)
    pop[0::2] = theta[None, :] + t
    pop[1::2] = theta[None, :] - t
    return pop


def es_update_scalars(K: int, sigma: float, stepsize: float, l2_coeff: float):
    """(scale, decay) of the update: f64 expressions cast to f32."""
    scale = np.float32(float(stepsize) / (2.0 * K * float(sigma)))
    decay = np.float32(float(stepsize) * float(l2_coeff))
    return scale, decay


def es_pair_weights(ranks: np.ndarray) -> np.ndarray:
    """``w[k] = r[2k] - r[2k + 1]`` in f64, cast to f32."""
    r = np.asarray(ranks, dtype=np.float64)
    return (r[0::2] - r[1::2]).astype(np.float32)


def es_update_reference(theta: np.ndarray, eps: np.ndarray, w: np.ndarray,
                        scale, decay) -> np.ndarray:
    """``es_update`` in numpy f32: ``acc = acc + w[k] * eps[k]`` for ``k``
    ascending (product and sum each rounded), then ``(theta + scale * acc) -
    decay * theta`` left to right."""
    theta = np.asarray(theta, dtype=np.float32)
    eps = np.asarray(eps, dtype=np.float32)
    w = np.asarray(w, dtype=np.float32)
    scale, decay = np.float32(scale), np.float32(decay)
    acc = np.zeros_like(theta)
    for k in range(eps.shape[0]):
        acc = acc + w[k] * eps[k]
    return (theta + scale * acc) - decay * theta


def head_offsets(policy) -> List[int]:
    """Offsets of ``head_params(policy)``'s 12 tensors inside the flat
    parameter vector (``policy.parameters()`` order): the last 12 parameters
    are exactly the head's, in ``head_fwd``'s order."""
    params = list(policy.parameters())
    head = head_params(policy)
    tail = params[-len(head):]
    assert len(tail) == len(head) and all(
        p.data_ptr() == h.data_ptr() and p.shape == h.shape
        for p, h in zip(tail, head)), \
        "head_params(policy) is not the tail of policy.parameters()"
    off = sum(p.numel() for p in params[:-len(head)])
    offs = []
    for p in tail:
        offs.append(off)
        off += p.numel()
    return offs


@torch.no_grad()
def load_flat(policy, flat: torch.Tensor):
    """Copy a flat parameter vector (``policy.parameters()`` order) into
    ``policy``."""
    off = 0
    for p in policy.parameters():
        k = p.numel()
        p.copy_(flat[off:off + k].view(p.shape))
        off += k
    assert off == flat.numel(), "flat vector does not match the policy"


@torch.no_grad()
def act_population_reference(mode: int, obs_gf, obs_mask, obs_model,
                             obs_sched, done, policy, pop, model_emb_pop,
                             E: int, seed: int = 0, step: int = 0
                             ) -> Dict[str, torch.Tensor]:
    """The ``actor_population`` contract in torch + numpy: member ``m``'s
    weights are loaded into ``policy`` (a scratch copy — it is overwritten)
    and ``act_reference`` runs on rows ``[mE, (m+1)E)``.  A slice call has
    ``B = E``, so its Philox index is ``e``."""
    if mode not in POLICY_MODES:
        raise ValueError("act_population_reference serves the policy modes "
                         f"only, not mode {mode}")
    P = pop.shape[0]
    B = obs_mask.shape[0]
    if B != P * E:
        raise ValueError(f"B = {B} is not P * E = {P} * {E}")
    outs = []
    for m in range(P):
        sl = slice(m * E, (m + 1) * E)
        load_flat(policy, pop[m])
        outs.append(act_reference(
            mode, obs_gf[sl], obs_mask[sl], obs_model[sl], obs_sched[sl],
            done[sl], policy=policy, model_emb=model_emb_pop[m], seed=seed,
            step=step))
    return {k: torch.cat([o[k] for o in outs], dim=0) for k in outs[0]}


# ---------------------------------------------------------------------------
class PopulationEvaluator:
    """Evaluates a whole ES population in one batched engine rollout.

    Built from an ``EngineVectorEnv`` (``supports_population_eval``): reuses
    its ``spec``, ``gen``, ``_models_batch``, ``device`` and ``base_seed`` and
    owns a separate engine of ``B = P * E`` envs, allocated once and rebuilt
    only when a schedule outgrows it.  The caller's env is never stepped.
    """

    def __init__(self, vec_env, policy, perturbation_pairs: int,
                 envs_per_member: int, eval_max_steps: int = 100000,
                 noise_seed: int = 0, deterministic: bool = False):
        if not getattr(vec_env, "supports_population_eval", False):
            raise TypeError("PopulationEvaluator needs an env with "
                            "supports_population_eval (EngineVectorEnv)")
        self.env = vec_env
        self.spec = vec_env.spec
        self.gen = vec_env.gen
        self.device = torch.device(vec_env.device)
        self.base_seed = int(vec_env.base_seed)
        self.K = int(perturbation_pairs)
        self.P = 2 * self.K
        self.E = int(envs_per_member)
        self.B = self.P * self.E
        if self.K < 1 or self.E < 1:
            raise ValueError("perturbation_pairs and envs_per_member must be "
                             "at least 1")
        self.eval_max_steps = int(eval_max_steps)
        self.noise_seed = int(noise_seed) & _U64
        self.mode = MODES["policy_greedy" if deterministic
                          else "policy_sample"]
        self.on_gpu = self.device.type == "cuda"
        if self.on_gpu and not getattr(policy, "_fused_head_ok", False):
            raise ValueError("actor_population is built for the default head "
                             "shapes only (policy._fused_head_ok)")
        # member weights are loaded into this copy, never into the trainer's
        self.scratch = copy.deepcopy(policy).to(self.device)
        self.head_offs = head_offsets(self.scratch)
        self.numel = sum(p.numel() for p in self.scratch.parameters())
        self.eng = None
        self._cap = 0
        self._ext = None
        if self.on_gpu:
            from .. import ops as hip_ops
            self._ext = hip_ops.get_extension(required=True)
            self._empty = torch.empty(0, device=self.device)
        self.timings: Dict[str, float] = {}

    # ------------------------------------------------------------------
    def _sync(self):
        if self.on_gpu:
            torch.cuda.synchronize(self.device)

    def perturb(self, theta: torch.Tensor, sigma: float, generation: int):
        """(``eps`` [K, n], ``pop`` [2K, n]) for this generation."""
        n = theta.numel()
        sigma32 = float(np.float32(sigma))
        if self.on_gpu:
            theta = theta.detach().float().contiguous()
            eps = torch.empty((self.K, n), device=self.device)
            pop = torch.empty((self.P, n), device=self.device)
            self._ext.es_perturb(theta, sigma32, self.noise_seed,
                                 int(generation) & _U64, eps, pop)
            return eps, pop
        eps = es_noise_reference(self.noise_seed, generation, self.K, n)
        pop = es_population_reference(theta.detach().cpu().numpy(), eps,
                                      sigma32)
        return torch.from_numpy(eps), torch.from_numpy(pop)

    def update(self, theta: torch.Tensor, eps: torch.Tensor, w: np.ndarray,
               scale, decay) -> torch.Tensor:
        """``theta'`` of the ES step (see ``es_update_reference``)."""
        if self.on_gpu:
            theta = theta.detach().float().contiguous()
            out = torch.empty_like(theta)
            w_dev = torch.as_tensor(np.asarray(w, dtype=np.float32),
                                    device=self.device)
            self._ext.es_update(theta, eps, w_dev, float(np.float32(scale)),
                                float(np.float32(decay)), out)
            return out
        return torch.from_numpy(es_update_reference(
            theta.detach().cpu().numpy(), eps.numpy(), w, scale, decay))

    # ------------------------------------------------------------------
    def schedules(self, generation: int):
        """Schedule ``e`` of generation ``g``: ``_drain``'s seed formula with
        ``g`` as the episode counter; shared by all members."""
        from ..cluster.vec_engine import drain_episode_schedule
        return [drain_episode_schedule(
            self.gen, self.spec,
            seed=self.base_seed + 1000 * e + int(generation))
            for e in range(self.E)]

    def _make_engine(self, cap: int):
        if self.on_gpu:
            from ..cluster.gpu_engine import GpuEngine
            self.eng = GpuEngine(self.spec, B=self.B, device=self.device,
                                 n_jobs_cap=cap)
        else:
            from ..cluster.vec_engine import CpuEngine
            self.eng = CpuEngine(self.spec, B=self.B, n_jobs_cap=cap)
        self._cap = cap

    def reset(self, scheds):
        """Every member starts from the same ``E`` freshly reset envs."""
        need = max(s.n for s in scheds)
        if self.eng is None or need + 1 > self._cap:
            self._make_engine(need + 8)
        eng, E = self.eng, self.E
        if self.on_gpu:
            for e in range(E):
                eng.reset_env(e, scheds[e])
            if self.P > 1:
                eng.replicate_envs(list(range(E)) * (self.P - 1),
                                   list(range(E, self.B)))
        else:
            for b in range(self.B):
                eng.reset_env(b, scheds[b % E])

    @torch.no_grad()
    def embeddings(self, pop: torch.Tensor) -> torch.Tensor:
        """``model_emb_pop`` [P, M, 16]: one GNN forward per member."""
        from ..models.gnn import graph_mean
        mb = self.env._models_batch
        out = []
        for m in range(self.P):
            load_flat(self.scratch, pop[m])
            out.append(graph_mean(self.scratch.gnn(mb), mb).float())
        return torch.stack(out).contiguous()

    def act(self, pop, model_emb_pop, step: int) -> torch.Tensor:
        """Actions [B] for the engine's current observations (ES needs
        nothing else: the kernel's optional outputs are left out)."""
        T = self.eng.T
        if self.on_gpu:
            empty = self._empty
            self._ext.actor_population(
                T["obs_gf"], T["obs_mask"], T["obs_model"], T["done"], pop,
                model_emb_pop, self.head_offs, self.E, self.mode,
                self.base_seed & _U64, int(step) & _U64, T["actions"],
                empty, empty, empty, empty)
            return T["actions"]
        return act_population_reference(
            self.mode, T["obs_gf"], T["obs_mask"], T["obs_model"],
            T["obs_sched"], T["done"], self.scratch, pop, model_emb_pop,
            self.E, seed=self.base_seed, step=step)["actions"]

    def rollout(self, pop, model_emb_pop, generation: int):
        """``EngineEvalLoop._run_wave``'s loop: while any env is live and the
        cap is not reached, actor -> step -> ``ret += reward where live``
        (f64 on the engine's device).  The Philox step counter is
        ``generation * eval_max_steps + t``: a function of the generation
        alone, so a resumed run replays it."""
        eng = self.eng
        dev = eng.T["reward"].device
        ret = torch.zeros(self.B, dtype=torch.float64, device=dev)
        nsteps = torch.zeros(self.B, dtype=torch.int64, device=dev)
        step0 = int(generation) * self.eval_max_steps
        t = 0
        while t < self.eval_max_steps:
            live = eng.T["done"] == 0
            if not bool(live.any()):
                break
            actions = self.act(pop, model_emb_pop, step0 + t)
            eng.step(actions)
            ret = torch.where(live, ret + eng.T["reward"], ret)
            nsteps += live.to(torch.int64)
            t += 1
        return ret, nsteps, t

    def evaluate(self, pop: torch.Tensor, generation: int) -> Dict:
        """One generation's evaluation: ``fitness`` [P] (f64 mean over the
        member's ``E`` returns), ``returns`` [P, E], ``live_steps`` (env steps
        played), ``eval_steps`` (length of the step loop) and
        ``truncated_envs`` (envs still live at the cap; they count with their
        return so far)."""
        tm = self.timings = {}
        self._sync()
        t0 = time.perf_counter()
        self.reset(self.schedules(generation))
        self._sync()
        t1 = time.perf_counter()
        model_emb_pop = self.embeddings(pop)
        self._sync()
        t2 = time.perf_counter()
        ret, nsteps, eval_steps = self.rollout(pop, model_emb_pop, generation)
        still_live = self.eng.T["done"] == 0
        # one D2H copy of the returns and the live-step counts
        packed = torch.stack([ret, nsteps.to(torch.float64),
                              still_live.to(torch.float64)]).cpu().numpy()
        t3 = time.perf_counter()
        tm["reset_s"] = t1 - t0
        tm["gnn_s"] = t2 - t1
        tm["steps_s"] = t3 - t2
        returns = packed[0].reshape(self.P, self.E)
        return {
            "fitness": returns.mean(axis=1),
            "returns": returns,
            "live_steps": int(packed[1].sum()),
            "eval_steps": int(eval_steps),
            "truncated_envs": int(packed[2].sum()),
        }
