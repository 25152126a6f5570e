"""DQN-family trainer: dueling double-DQN with n-step targets and a replay
buffer — the reference's APEX-DQN config group
(``scripts/.../algo/apex_dqn.yaml``: gamma 0.999, lr 4.121e-7, dueling,
double_q, n_step 3, target_network_update_freq 100000, hiddens [256]).

Mapping onto this stack:
- The GNNPolicy already has the dueling decomposition: Q(s, a) =
  V(s) + A(s, a) - mean_a A(s, a), with A = policy_branch logits and
  V = value_branch (both fed by the shared GNN embedding; RLlib's dueling
  head has the same structure over ``hiddens: [256]``).
- Exploration is Boltzmann over Q (Categorical(logits=Q)) so collection
  reuses the SAME rollout machinery as PPO/IMPALA (engine or subprocess
  workers); APEX's epsilon-greedy-per-worker and its distributed
  replay shards are replaced by one in-memory buffer — divergences from
  APEX, not from DQN.
- The buffer samples uniformly by default.  ``prioritized_replay=True``
  turns on proportional prioritization with the reference's tuned
  ``prioritized_replay_alpha`` 0.9, ``_beta`` 0.1 and ``_eps`` 1e-6: slots
  are drawn in proportion to ``(|td| + eps) ** alpha`` from a sum tree, the
  loss is ``mean(w * huber)`` with ``w = (p_i n) ** -beta / max_weight``,
  and every minibatch's ``|td|`` becomes its slots' new priorities
  (rl/device_replay.py; on a GPU the kernels of ops/hip/per_replay.hip).
  Divergences that remain: new transitions enter at ``max_prio ** alpha``
  (standard PER) where the reference's ``worker_side_prioritization``
  computes an initial TD error; beta is constant; the tail of a fragment
  (its last ``n_step`` rows) is still dropped.
- Unlike the reference (which DISABLES action masking for DQN as a
  workaround for an RLlib crash, apex_dqn.yaml "TEMP HACK"), masking works
  here: invalid actions carry -inf Q and are never selected.

Two learners (``DQNConfig.learner``).  ``"torch"`` keeps the replay buffer as
a Python list of transitions and evaluates the loss as a torch autograd
chain.  ``"device"`` trains from the flat device tensors of
``rollout(device_resident=True)``: the n-step transitions go straight into a
``DeviceReplay`` ring, the forward is head-only and never touches
``data["obs"]``, and on a GPU the loss is the fused kernels of
``ops/hip/dqn_loss.hip`` with one D2H per update for the stats.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional

import numpy as np
import torch
import torch.nn.functional as F

from ..parallel import all_reduce_gradients
from .device_replay import DeviceReplay, SumTreeReference
from .impala import LEARNERS, ImpalaTrainer
from .rollout import CompactObs


@dataclass
class DQNConfig:
    # reference algo/apex_dqn.yaml tuned values
    gamma: float = 0.999
    lr: float = 4.121e-7
    n_step: int = 3
    double_q: bool = True
    dueling: bool = True
    target_network_update_freq: int = 100000   # env steps between syncs
    v_min: float = -1000.0
    v_max: float = 1000.0
    train_batch_size: int = 4096               # transitions per update
    sgd_minibatch_size: int = 256
    num_sgd_iter: int = 4
    replay_capacity: int = 200_000
    learning_starts: int = 2_000
    grad_clip: Optional[float] = 40.0
    # "torch": host list replay + autograd loss.  "device": device replay
    # ring + fused TD-loss kernels (needs an env with
    # supports_device_resident, else falls back to "torch" with a warning)
    learner: str = "torch"
    # proportional prioritized replay (both learners); the three values are
    # the reference's tuned ones
    prioritized_replay: bool = False
    prioritized_replay_alpha: float = 0.9
    prioritized_replay_beta: float = 0.1
    prioritized_replay_eps: float = 1e-6

    def __post_init__(self):
        if self.prioritized_replay_alpha < 0:
            raise ValueError("prioritized_replay_alpha must be >= 0")
        if self.prioritized_replay_beta < 0:
            raise ValueError("prioritized_replay_beta must be >= 0")
        if not self.prioritized_replay_eps > 0:
            raise ValueError("prioritized_replay_eps must be > 0")


def nstep_transitions_reference(rewards, dones, n_step: int, gamma: float):
    """The n-step numerics of ``DQNTrainer._ingest`` on f32 rewards, written
    with explicit casts: the return ``R`` is accumulated in f32, the running
    discount is an f64 rounded to f32 for each multiply, and ``disc`` is that
    f64 rounded to f32 once.  The return stops at the first done.

    ``rewards`` / ``dones`` are [T, N].  Returns, each [max(T - n_step, 0),
    N]: ``ret`` f32, ``disc`` f32 (gamma ** steps), ``has_next`` bool (False
    where a done cut the return) and ``steps`` int64 (rewards accumulated,
    so the next state of transition (t, b) is row ``(t + steps) * N + b``)."""
    r = np.asarray(rewards, dtype=np.float32)
    d = np.asarray(dones) != 0
    T, N = r.shape
    M = max(T - int(n_step), 0)
    ret = np.zeros((M, N), dtype=np.float32)
    disc = np.ones((M, N), dtype=np.float64)
    steps = np.zeros((M, N), dtype=np.int64)
    alive = np.ones((M, N), dtype=bool)
    discount = np.float64(1.0)
    if M > 0:
        for i in range(int(n_step)):
            term = np.float32(discount) * r[i:i + M]
            ret = np.where(alive, ret + term, ret).astype(np.float32)
            discount = np.float64(discount * np.float64(gamma))
            disc = np.where(alive, discount, disc)
            steps = steps + alive
            alive = alive & ~d[i:i + M]
    return ret, disc.astype(np.float32), alive, steps


def dueling_q(logits, values, dueling: bool):
    """Q(s, .) from the policy head's outputs, as ``DQNTrainer._q_values``
    recombines them: masked actions (logit at f32-min) are left out of the
    advantage mean and keep their raw logit."""
    if not dueling:
        return logits
    valid = logits > -1e30
    adv = torch.where(valid, logits, torch.zeros_like(logits))
    mean_adv = adv.sum(-1) / valid.sum(-1).clamp(min=1)
    q = values.unsqueeze(-1) + logits - mean_adv.unsqueeze(-1)
    return torch.where(valid, q, logits)


STAT_KEYS = ("total_loss", "q_mean", "td_abs_mean", "target_mean")
# what a prioritized update reports on top: the mean importance weight of the
# update's minibatches and the largest priority |td| + eps seen so far
PER_STAT_KEYS = ("is_weight_mean", "max_priority")


def dqn_loss_reference(logits_s, values_s, logits_no, values_no, logits_nt,
                       values_nt, actions, ret, disc, has_next, v_min, v_max,
                       dueling: bool, double_q: bool, weights=None):
    """The loss of ``DQNTrainer.update()`` as a torch autograd chain over
    whole-minibatch tensors.  ``logits_s`` [B, A] / ``values_s`` [B] are the
    online net on s and carry the graph; ``*_no`` / ``*_nt`` are the online
    and the target net on s' and are constants; ``has_next`` [B] is 0 where
    the n-step return was cut, and such a row bootstraps from 0 whatever its
    s' rows hold.  Returns (loss, dict of 0-d stat tensors in STAT_KEYS).

    With ``weights`` [B] (prioritized replay's importance weights) the loss
    is ``mean(weights * huber)``, the other stats stay unweighted, and the
    dict also carries ``td_abs`` [B], the rows' ``|q_a - target|``."""
    with torch.no_grad():
        q_next_t = dueling_q(logits_nt, values_nt, dueling)
        if double_q:
            a_star = dueling_q(logits_no, values_no, dueling).argmax(-1)
            vals = q_next_t.gather(1, a_star.unsqueeze(1)).squeeze(1)
        else:
            vals = q_next_t.max(-1).values
        boot = torch.where(has_next > 0, vals, torch.zeros_like(vals))
        target = torch.clamp(ret + disc * boot, v_min, v_max)
    q = dueling_q(logits_s, values_s, dueling)
    q_a = q.gather(1, actions.unsqueeze(1)).squeeze(1)
    if weights is None:
        loss = F.smooth_l1_loss(q_a, target)
    else:
        loss = (weights * F.smooth_l1_loss(q_a, target,
                                           reduction="none")).mean()
    stats = {"total_loss": loss.detach(),
             "q_mean": q_a.detach().mean(),
             "td_abs_mean": (q_a.detach() - target).abs().mean(),
             "target_mean": target.mean()}
    if weights is not None:
        stats["td_abs"] = (q_a.detach() - target).abs()
    return loss, stats


class _DQNLossFn(torch.autograd.Function):
    """Fused DQN TD loss (ops/hip/dqn_loss.hip): two launches forward (row
    kernel, ordered reduction), one analytic backward.  Only ``logits_s`` and
    ``values_s`` take a gradient.  Returns (loss, stats[4] in STAT_KEYS
    order)."""

    @staticmethod
    def forward(ctx, logits_s, values_s, logits_no, values_no, logits_nt,
                values_nt, actions, ret, disc, has_next, v_min, v_max,
                dueling, double_q):
        from .. import ops as hip_ops
        ext = hip_ops.get_extension(required=True)
        logits_s = logits_s.contiguous()
        loss, stats, dq = ext.dqn_loss_fwd(
            logits_s, values_s.contiguous(), logits_no.contiguous(),
            values_no.contiguous(), logits_nt.contiguous(),
            values_nt.contiguous(), actions, ret, disc, has_next,
            float(v_min), float(v_max), bool(dueling), bool(double_q))
        ctx.save_for_backward(logits_s, actions, dq)
        ctx.dueling = bool(dueling)
        ctx.mark_non_differentiable(stats)
        return loss.reshape(()), stats

    @staticmethod
    def backward(ctx, gl, _gstats):
        from .. import ops as hip_ops
        ext = hip_ops.get_extension(required=True)
        logits_s, actions, dq = ctx.saved_tensors
        glogits, gvalues = ext.dqn_loss_bwd(
            logits_s, actions, dq, gl.reshape(1).contiguous(), ctx.dueling)
        return (glogits, gvalues) + (None,) * 12


class _DQNWeightedLossFn(torch.autograd.Function):
    """``_DQNLossFn`` with importance weights (``dqn_loss_fwd_weighted``):
    loss = mean(w * huber) and the saved dq carries w, so the backward kernel
    is the same one.  Returns (loss, stats[4], td_abs[B] f64 unweighted)."""

    @staticmethod
    def forward(ctx, logits_s, values_s, logits_no, values_no, logits_nt,
                values_nt, actions, ret, disc, has_next, v_min, v_max,
                dueling, double_q, weights):
        from .. import ops as hip_ops
        ext = hip_ops.get_extension(required=True)
        logits_s = logits_s.contiguous()
        loss, stats, dq, td_abs = ext.dqn_loss_fwd_weighted(
            logits_s, values_s.contiguous(), logits_no.contiguous(),
            values_no.contiguous(), logits_nt.contiguous(),
            values_nt.contiguous(), actions, ret, disc, has_next,
            float(v_min), float(v_max), bool(dueling), bool(double_q),
            weights.contiguous())
        ctx.save_for_backward(logits_s, actions, dq)
        ctx.dueling = bool(dueling)
        ctx.mark_non_differentiable(stats, td_abs)
        return loss.reshape(()), stats, td_abs

    @staticmethod
    def backward(ctx, gl, _gstats, _gtd):
        return _DQNLossFn.backward(ctx, gl, _gstats) + (None,)


class DQNTrainer(ImpalaTrainer):
    """Same trainer-facing interface as PPOTrainer/ImpalaTrainer."""

    def __init__(self, vector_env, policy, config: Optional[DQNConfig] = None,
                 device: Optional[torch.device] = None):
        cfg = config or DQNConfig()
        if cfg.learner not in LEARNERS:
            raise ValueError("DQNConfig.learner must be 'torch' or "
                             f"'device', not {cfg.learner!r}")
        super().__init__(vector_env, policy, None, device=device)
        self.config = cfg
        self.optimizer = torch.optim.Adam(self.policy.parameters(),
                                          lr=cfg.lr, foreach=True)
        import copy
        self.target = copy.deepcopy(self.policy).to(self.device)
        self.target.eval()
        self._steps_since_sync = 0
        # list-based ring buffer (deque indexing is O(n))
        self.replay: List = []
        self._replay_ptr = 0
        # the device learner's ring, made on the first device-resident batch
        self.replay_dev: Optional[DeviceReplay] = None
        # the torch learner's priorities when prioritized_replay is on: a
        # host sum tree over the list's slots (slot k % capacity, as the list
        # fills and then overwrites)
        self._per_host: Optional[SumTreeReference] = None
        self._replay_written = 0

    # Q(s, .) with the dueling recombination over masked actions
    def _q_values(self, obs: List[CompactObs], net):
        logits, values = self._forward_batch_with(obs, net)
        if self.config.dueling:
            # masked actions carry clamp(log(0)) = f32-min in `logits`
            # (forward_flat); exclude them from the advantage mean and keep
            # them at f32-min in Q so argmax/gather never select them
            valid = logits > -1e30
            adv = torch.where(valid, logits, torch.zeros_like(logits))
            mean_adv = adv.sum(-1) / valid.sum(-1).clamp(min=1)
            q = values.unsqueeze(-1) + logits - mean_adv.unsqueeze(-1)
            q = torch.where(valid, q, logits)
            return q
        return logits

    def _forward_batch_with(self, obs, net):
        policy = self.policy
        try:
            self.policy = net
            return self._forward_batch(obs)
        finally:
            self.policy = policy

    # ------------------------------------------------------------------
    def _ingest(self, data: Dict):
        """Turn a [T, N] rollout fragment into n-step transitions."""
        cfg = self.config
        T, N = data["rewards"].shape
        obs = data["obs"]               # t-major flat list [T*N]
        rewards = data["rewards"]
        dones = data["dones"]
        n = cfg.n_step
        for t in range(T - n):
            for b in range(N):
                R, discount, cut = 0.0, 1.0, False
                for i in range(n):
                    R += discount * rewards[t + i][b]
                    discount *= cfg.gamma
                    if dones[t + i][b]:
                        cut = True
                        break
                item = (obs[t * N + b], int(data["actions"][t][b]),
                        float(R),
                        obs[(t + i + 1) * N + b] if not cut else None,
                        float(discount))
                if len(self.replay) < cfg.replay_capacity:
                    self.replay.append(item)
                else:
                    self.replay[self._replay_ptr] = item
                    self._replay_ptr = (self._replay_ptr + 1) \
                        % cfg.replay_capacity

    # ------------------------------------------------------------------
    def _heads(self, net, model_emb, gfull, model_ids):
        """(logits, values) of ``net``'s heads over flat state rows, given
        ``net``'s per-model GNN embeddings (ImpalaTrainer._forward_device)."""
        graph_emb = net.graph_module(gfull)
        final = torch.cat([model_emb[model_ids], graph_emb], dim=-1)
        logits = net.policy_branch(final)
        values = net.value_branch(final).squeeze(-1)
        if net.config["apply_action_mask"]:
            logits = logits + torch.clamp(
                torch.log(gfull[:, 17:]), min=torch.finfo(torch.float32).min)
        return logits, values

    def _loss_device(self, mb: Dict, target_emb, weights=None):
        """(loss, stats[4] tensor in STAT_KEYS order) of one ring minibatch:
        the fused kernels on a GPU, the torch chain on CPU tensors (the
        CpuEngine backend).  With importance ``weights`` the loss is weighted
        and a third value is the rows' unweighted |td| in f64."""
        from ..models.gnn import graph_mean
        cfg = self.config
        mb_static = self.env._models_batch
        model_emb = graph_mean(self.policy.gnn(mb_static), mb_static)
        logits_s, values_s = self._heads(self.policy, model_emb,
                                         mb["s_gfull"], mb["s_model"])
        with torch.no_grad():
            # same weights as the pass above, so its embeddings serve s'
            logits_no, values_no = self._heads(
                self.policy, model_emb.detach(), mb["n_gfull"], mb["n_model"])
            logits_nt, values_nt = self._heads(
                self.target, target_emb, mb["n_gfull"], mb["n_model"])
        args = (logits_s, values_s, logits_no, values_no, logits_nt,
                values_nt, mb["action"], mb["ret"], mb["disc"],
                mb["has_next"], cfg.v_min, cfg.v_max, cfg.dueling,
                cfg.double_q)
        if weights is None:
            if logits_s.is_cuda:
                return _DQNLossFn.apply(*args)
            loss, st = dqn_loss_reference(*args)
            return loss, torch.stack([st[k] for k in STAT_KEYS])
        if logits_s.is_cuda:
            return _DQNWeightedLossFn.apply(*args, weights)
        loss, st = dqn_loss_reference(*args, weights=weights)
        return (loss, torch.stack([st[k] for k in STAT_KEYS]),
                st["td_abs"].double())

    def _update_device(self, data: Dict) -> Dict[str, float]:
        from ..models.gnn import graph_mean
        cfg = self.config
        if self.replay_dev is None:
            self.replay_dev = DeviceReplay(
                cfg.replay_capacity, data["gfull_dev"].shape[1],
                data["gfull_dev"].device,
                prioritized=cfg.prioritized_replay,
                alpha=cfg.prioritized_replay_alpha,
                beta=cfg.prioritized_replay_beta,
                eps=cfg.prioritized_replay_eps)
        replay = self.replay_dev
        replay.ingest(data, cfg.n_step, cfg.gamma)
        if cfg.prioritized_replay:
            return self._update_device_prioritized(data)
        stats = {k: 0.0 for k in STAT_KEYS}
        if len(replay) >= cfg.learning_starts and cfg.num_sgd_iter > 0:
            rng = np.random.RandomState(self.iteration)
            # the torch learner's draws, uploaded once
            idx = torch.as_tensor(
                np.stack([rng.randint(0, len(replay),
                                      size=cfg.sgd_minibatch_size)
                          for _ in range(cfg.num_sgd_iter)]),
                device=replay.device)
            with torch.no_grad():
                mb_static = self.env._models_batch
                target_emb = graph_mean(self.target.gnn(mb_static), mb_static)
            acc = torch.zeros(len(STAT_KEYS), device=replay.device)
            for k in range(cfg.num_sgd_iter):
                loss, stats_t = self._loss_device(replay.gather(idx[k]),
                                                  target_emb)
                self.optimizer.zero_grad(set_to_none=True)
                loss.backward()
                all_reduce_gradients(self.policy.parameters())
                if cfg.grad_clip is not None:
                    torch.nn.utils.clip_grad_norm_(self.policy.parameters(),
                                                   cfg.grad_clip)
                self.optimizer.step()
                acc += stats_t.detach()
            # one D2H for all stats of all minibatches
            stats = dict(zip(STAT_KEYS, (acc / cfg.num_sgd_iter).tolist()))
        stats["replay"] = len(replay)
        stats["learner"] = 1
        self._sync_target(data)
        return stats

    def _update_device_prioritized(self, data: Dict) -> Dict[str, float]:
        """``_update_device`` after the ingest, with prioritized sampling:
        per minibatch sample -> gather -> weighted loss -> step ->
        update_priorities, all on the ring's device, and still one D2H per
        update."""
        from ..models.gnn import graph_mean
        cfg = self.config
        replay = self.replay_dev
        keys = STAT_KEYS + PER_STAT_KEYS
        stats = {k: 0.0 for k in keys}
        if len(replay) >= cfg.learning_starts and cfg.num_sgd_iter > 0:
            rng = np.random.RandomState(self.iteration)
            # the torch learner's uniforms, uploaded once
            u = torch.as_tensor(
                rng.random_sample((cfg.num_sgd_iter, cfg.sgd_minibatch_size)),
                device=replay.device)
            with torch.no_grad():
                mb_static = self.env._models_batch
                target_emb = graph_mean(self.target.gnn(mb_static), mb_static)
            acc = torch.zeros(len(STAT_KEYS) + 1, device=replay.device)
            for k in range(cfg.num_sgd_iter):
                idx, weight = replay.sample(u[k])
                loss, stats_t, td_abs = self._loss_device(
                    replay.gather(idx), target_emb, weights=weight)
                self.optimizer.zero_grad(set_to_none=True)
                loss.backward()
                all_reduce_gradients(self.policy.parameters())
                if cfg.grad_clip is not None:
                    torch.nn.utils.clip_grad_norm_(self.policy.parameters(),
                                                   cfg.grad_clip)
                self.optimizer.step()
                replay.update_priorities(idx, td_abs)
                acc[:len(STAT_KEYS)] += stats_t.detach()
                acc[len(STAT_KEYS)] += weight.mean()
            # one D2H for all stats of all minibatches and max_prio
            out = torch.cat([acc.double() / cfg.num_sgd_iter,
                             replay.max_prio])
            stats = dict(zip(keys, out.tolist()))
        stats["replay"] = len(replay)
        stats["learner"] = 1
        self._sync_target(data)
        return stats

    def _ingest_priorities(self, data: Dict):
        """The torch learner's tree after ``_ingest(data)``: the list slots
        the fragment wrote enter at ``max_prio ** alpha``."""
        cfg = self.config
        C = cfg.replay_capacity
        if self._per_host is None:
            self._per_host = SumTreeReference(
                C, cfg.prioritized_replay_alpha, cfg.prioritized_replay_beta,
                cfg.prioritized_replay_eps)
        T, N = data["rewards"].shape
        K = max(T - cfg.n_step, 0) * N
        if K > 0:
            self._per_host.ingest(
                (self._replay_written + max(K - C, 0)) % C, min(K, C))
        self._replay_written += K

    def _sync_target(self, data: Dict):
        # target sync on an env-step cadence (reference: 100k tuned)
        self._steps_since_sync += int(np.prod(data["rewards"].shape))
        if self._steps_since_sync >= self.config.target_network_update_freq:
            self.target.load_state_dict(self.policy.state_dict())
            self._steps_since_sync = 0

    def update(self, data: Dict) -> Dict[str, float]:
        cfg = self.config
        if self._device_learner() and "gfull_dev" in data:
            return self._update_device(data)
        self._ingest(data)
        per = None
        if cfg.prioritized_replay:
            self._ingest_priorities(data)
            per = self._per_host
        if len(self.replay) < cfg.learning_starts:
            return {"total_loss": 0.0, "q_mean": 0.0,
                    "replay": len(self.replay), "learner": 0}
        rng = np.random.RandomState(self.iteration)
        stats = {"total_loss": 0.0, "q_mean": 0.0}
        if per is not None:
            stats["is_weight_mean"] = 0.0
            # the device learner's uniforms
            u = rng.random_sample((cfg.num_sgd_iter, cfg.sgd_minibatch_size))
        n_updates = 0
        for it in range(cfg.num_sgd_iter):
            if per is None:
                idx = rng.randint(0, len(self.replay),
                                  size=cfg.sgd_minibatch_size)
            else:
                idx, weight = per.sample(u[it])
            batch = [self.replay[i] for i in idx]
            s = [b[0] for b in batch]
            a = torch.as_tensor([b[1] for b in batch], device=self.device)
            r = torch.as_tensor([b[2] for b in batch], device=self.device,
                                dtype=torch.float32)
            disc = torch.as_tensor([b[4] for b in batch], device=self.device,
                                   dtype=torch.float32)
            has_next = [b[3] is not None for b in batch]
            sp = [b[3] for b in batch if b[3] is not None]

            with torch.no_grad():
                boot = torch.zeros(len(batch), device=self.device)
                if sp:
                    q_next_t = self._q_values(sp, self.target)
                    if cfg.double_q:
                        q_next_o = self._q_values(sp, self.policy)
                        a_star = q_next_o.argmax(-1)
                        vals = q_next_t.gather(
                            1, a_star.unsqueeze(1)).squeeze(1)
                    else:
                        vals = q_next_t.max(-1).values
                    boot[torch.as_tensor(has_next,
                                         device=self.device)] = vals
                target = torch.clamp(r + disc * boot, cfg.v_min, cfg.v_max)
            q = self._q_values(s, self.policy)
            q_a = q.gather(1, a.unsqueeze(1)).squeeze(1)
            if per is None:
                loss = F.smooth_l1_loss(q_a, target)
            else:
                w = torch.as_tensor(weight, device=self.device)
                loss = (w * F.smooth_l1_loss(q_a, target,
                                             reduction="none")).mean()
            self.optimizer.zero_grad(set_to_none=True)
            loss.backward()
            all_reduce_gradients(self.policy.parameters())
            if cfg.grad_clip is not None:
                torch.nn.utils.clip_grad_norm_(self.policy.parameters(),
                                               cfg.grad_clip)
            self.optimizer.step()
            if per is not None:
                per.update(idx, (q_a.detach() - target).abs().double()
                           .cpu().numpy())
                stats["is_weight_mean"] += float(weight.mean())
            stats["total_loss"] += float(loss.item())
            stats["q_mean"] += float(q_a.mean().item())
            n_updates += 1
        for k in ("total_loss", "q_mean"):
            stats[k] /= max(n_updates, 1)
        if per is not None:
            stats["is_weight_mean"] /= max(n_updates, 1)
            stats["max_priority"] = float(per.max_prio[0])
        stats["replay"] = len(self.replay)
        stats["learner"] = 0
        self._sync_target(data)
        return stats

    # ------------------------------------------------------------------
    def state_dict(self) -> Dict:
        out = super().state_dict()
        out["target"] = self.target.state_dict()
        out["algo"] = "dqn"
        return out

    def load_state_dict(self, state: Dict):
        super().load_state_dict(state)
        if "target" in state:
            self.target.load_state_dict(state["target"])
