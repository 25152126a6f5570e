"""Device-side actors for the env engine.

``DeviceActor`` turns the engine's observation tensors (``obs_gf``,
``obs_mask``, ``obs_model``, ``obs_sched``) into its ``actions`` tensor for B
envs at once: the GNN policy (greedy or sampled) and the six paper baselines
of ``envs/actors.py``.  On a ``GpuEngine`` that is ONE ``actor_batch`` launch
(``ops/hip/actor.hip``); ``act_reference`` is the same contract in pure
torch + numpy on any device — the backend for ``CpuEngine`` and for head
shapes the kernel is not built for, and the oracle of the GPU tests.

RNG contract (both backends): Philox4x32-10 with key ``(seed_lo, seed_hi)``
and counter ``(b, step_lo, step_hi, 0)``; ``u = (word0 >> 8) * 2**-24`` is in
``[0, 1)``.  The ``random`` actor picks ``valid[1:][min(n - 2, floor(u * (n -
1)))]`` from that ``u`` — the same distribution as ``envs.actors.Random``
(uniform over ``valid[1:]``) but NOT numpy's global stream, so a ``random``
episode here is not the episode ``EvalLoop`` plays with ``np.random``.

Done rule: an env with ``done != 0`` gets action 0 and its output rows are
left untouched.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

MODES = {
    "policy_greedy": 0,
    "policy_sample": 1,
    "random": 2,
    "no_parallelism": 3,
    "min_parallelism": 4,
    "max_parallelism": 5,
    "sip_ml": 6,
    "acceptable_jct": 7,
}
POLICY_MODES = (MODES["policy_greedy"], MODES["policy_sample"])
ROW_KEYS = ("gfull", "lp_all", "logp", "value", "u")

_M0, _M1 = 0xD2511F53, 0xCD9E8D57
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_U32 = 0xFFFFFFFF


# ---------------------------------------------------------------------------
# Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2,
# 3", SC'11), written from the algorithm; vectorised over leading dims
# ---------------------------------------------------------------------------
def philox4x32_10(counter, key) -> np.ndarray:
    """``counter`` [..., 4] and ``key`` [..., 2] of 32-bit words -> the four
    output words [..., 4] as uint32."""
    c = np.asarray(counter, dtype=np.uint64) & _U32
    k = np.asarray(key, dtype=np.uint64) & _U32
    c0, c1, c2, c3 = (c[..., i].copy() for i in range(4))
    k0, k1 = k[..., 0].copy(), k[..., 1].copy()
    for _ in range(10):
        p0 = _M0 * c0           # 32x32 -> 64-bit products, exact in uint64
        p1 = _M1 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0, p1 & _U32,
                          (p0 >> 32) ^ c3 ^ k1, p0 & _U32)
        k0 = (k0 + _W0) & _U32
        k1 = (k1 + _W1) & _U32
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def philox_uniform(seed: int, step: int, B: int) -> np.ndarray:
    """The per-env uniform of the RNG contract: float32 [B] in [0, 1)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    step = int(step) & 0xFFFFFFFFFFFFFFFF
    ctr = np.zeros((B, 4), dtype=np.uint64)
    ctr[:, 0] = np.arange(B, dtype=np.uint64)
    ctr[:, 1] = step & _U32
    ctr[:, 2] = step >> 32
    key = np.array([seed & _U32, seed >> 32], dtype=np.uint64)
    x = philox4x32_10(ctr, np.broadcast_to(key, (B, 2)))[:, 0]
    # a 24-bit integer times 2^-24: exact in float32, never 1
    return (x >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


# ---------------------------------------------------------------------------
# heuristics on one mask row (the arithmetic of envs/actors.py)
# ---------------------------------------------------------------------------
def _heuristic_row(mode: int, mask_row: np.ndarray, u: float,
                   sip_ml_cap: Optional[int], seq: float, acc: float) -> int:
    A = len(mask_row)
    valid = np.flatnonzero(mask_row > 0)
    n = len(valid)
    if mode == MODES["no_parallelism"]:
        return 1 if n > 1 else 0
    if mode == MODES["min_parallelism"]:
        return 2 if n > 2 else (1 if n == 2 else 0)
    if n == 0:
        return 0
    if n == 1:
        return int(valid[0])
    last = int(valid[-1])
    if mode == MODES["max_parallelism"]:
        return last
    if mode == MODES["sip_ml"]:
        return last if sip_ml_cap is None or sip_ml_cap < 0 \
            else min(int(sip_ml_cap), last)
    if mode == MODES["acceptable_jct"]:
        with np.errstate(divide="ignore", invalid="ignore"):
            want = np.ceil(np.float64(seq) / np.float64(acc))
        if not want <= A:         # above A (or inf / nan): none reaches it
            return last
        for a in valid:
            if a >= want:
                return int(a)
        return last
    if mode == MODES["random"]:
        idx = int(np.floor(np.float32(u) * np.float32(n - 1)))
        return int(valid[1:][min(n - 2, idx)])
    raise ValueError(f"unknown heuristic mode {mode}")


def _gather_acc(sch_acc, obs_sched: np.ndarray) -> np.ndarray:
    """max-acceptable JCT of each env's queued job.  ``sch_acc`` is a
    ``[B, SCH]`` tensor/array or a per-env list of 1-D arrays (ragged: the
    ``max_acceptable`` of ``EpisodeSchedule``); a slot outside the row reads
    as 0 (``want`` = inf: no action reaches it)."""
    B = len(obs_sched)
    out = np.zeros(B, dtype=np.float64)
    for b in range(B):
        row = sch_acc[b]
        if row is None:
            continue
        if torch.is_tensor(row):
            row = row.detach().cpu().numpy()
        k = int(obs_sched[b])
        if 0 <= k < len(row):
            out[b] = float(row[k])
    return out


@torch.no_grad()
def policy_head_reference(policy, model_emb, obs_model, gfull, mask):
    """``GNNPolicy.forward_flat`` with the GNN replaced by the per-model
    embedding table: (masked logits [B,A], value [B])."""
    graph_emb = policy.graph_module(gfull)
    final = torch.cat([model_emb[obs_model], graph_emb], dim=-1)
    logits = policy.policy_branch(final)
    value = policy.value_branch(final).squeeze(-1)
    if policy.config["apply_action_mask"]:
        logits = logits + torch.clamp(torch.log(mask),
                                      min=torch.finfo(torch.float32).min)
    return logits, value


@torch.no_grad()
def act_reference(mode: int, obs_gf, obs_mask, obs_model, obs_sched, done,
                  policy=None, model_emb=None, model_seq=None, sch_acc=None,
                  sip_ml_cap: Optional[int] = None, seed: int = 0,
                  step: int = 0, actions=None,
                  rows: Optional[Dict[str, torch.Tensor]] = None
                  ) -> Dict[str, torch.Tensor]:
    """The ``actor_batch`` contract in torch + numpy, on the tensors' device.

    Returns ``{"actions": int32 [B]}`` plus, for the policy modes, the rows
    ``gfull`` / ``lp_all`` / ``logp`` / ``value`` / ``u`` (and ``logits``,
    the masked pre-softmax scores, for tests).  ``actions`` and ``rows``, when
    given, are written in place: only live envs' rows are touched.
    """
    dev = obs_mask.device
    B, A = obs_mask.shape
    mask_np = obs_mask.detach().cpu().numpy()
    live = (done.detach().cpu().numpy() == 0)
    mid_np = obs_model.detach().cpu().numpy().astype(np.int64)
    u = philox_uniform(seed, step, B)
    acts = np.zeros(B, dtype=np.int32)
    out: Dict[str, torch.Tensor] = {}

    if mode in POLICY_MODES:
        M = model_emb.shape[0]
        live &= (mid_np >= 0) & (mid_np < M)
        gfull = torch.cat([obs_gf, obs_mask], dim=1)
        mids = torch.as_tensor(np.where(live, mid_np, 0), device=dev)
        logits, value = policy_head_reference(policy, model_emb, mids, gfull,
                                              obs_mask)
        lp = torch.log_softmax(logits, dim=-1)
        lp_np = lp.cpu().numpy()
        if mode == MODES["policy_greedy"]:
            pick = np.argmax(logits.cpu().numpy(), axis=1)   # first maximum
        else:
            # sequential float32 inverse CDF over the A actions
            cum = np.cumsum(np.exp(lp_np), axis=1, dtype=np.float32)
            hit = (mask_np > 0) & (u[:, None] < cum)
            pick = np.zeros(B, dtype=np.int64)
            for b in range(B):
                valid = np.flatnonzero(mask_np[b] > 0)
                h = np.flatnonzero(hit[b])
                pick[b] = h[0] if len(h) else (valid[-1] if len(valid) else 0)
        acts[live] = pick[live]
        logp = lp.gather(1, torch.as_tensor(pick, device=dev).view(-1, 1)
                         ).squeeze(1)
        fresh = {"gfull": gfull, "lp_all": lp, "logp": logp, "value": value,
                 "u": torch.as_tensor(u, device=dev)}
        live_t = torch.as_tensor(live, device=dev)
        for k in ROW_KEYS:
            dst = rows.get(k) if rows is not None else None
            if dst is None:
                dst = torch.zeros_like(fresh[k])
            sel = live_t.view(-1, *([1] * (fresh[k].dim() - 1)))
            dst.copy_(torch.where(sel, fresh[k], dst))
            out[k] = dst
        out["logits"] = logits
    else:
        seq = np.zeros(B)
        acc = np.zeros(B)
        if model_seq is not None:
            ms = (model_seq.detach().cpu().numpy() if torch.is_tensor(model_seq)
                  else np.asarray(model_seq, dtype=np.float64))
            live &= (mid_np >= 0) & (mid_np < len(ms))
            seq = ms[np.where(live, mid_np, 0)]
        if mode == MODES["acceptable_jct"]:
            acc = _gather_acc(sch_acc, obs_sched.detach().cpu().numpy())
        for b in np.flatnonzero(live):
            acts[b] = _heuristic_row(mode, mask_np[b], float(u[b]),
                                     sip_ml_cap, float(seq[b]), float(acc[b]))
        if mode == MODES["random"]:
            dst = rows.get("u") if rows is not None else None
            fresh_u = torch.as_tensor(u, device=dev)
            if dst is None:
                dst = torch.zeros_like(fresh_u)
            dst.copy_(torch.where(torch.as_tensor(live, device=dev), fresh_u,
                                  dst))
            out["u"] = dst

    acts_t = torch.as_tensor(acts, device=dev)
    if actions is not None:
        actions.copy_(acts_t)
        acts_t = actions
    out["actions"] = acts_t
    return out


# ---------------------------------------------------------------------------
def head_params(policy):
    """The head's parameter tensors in ``head_fwd``'s order."""
    ln, lin_g = policy.graph_module[0], policy.graph_module[1]
    pb, vb = policy.policy_branch, policy.value_branch
    return [p.detach().contiguous() for p in (
        ln.weight, ln.bias, lin_g.weight, lin_g.bias,
        pb[0].weight, pb[0].bias, pb[2].weight, pb[2].bias,
        vb[0].weight, vb[0].bias, vb[2].weight, vb[2].bias)]


class DeviceActor:
    """Batched actor over an engine's tensors (see the module docstring)."""

    def __init__(self, mode: int, policy=None, seed: int = 0,
                 sip_ml_cap: Optional[int] = None, name: str = "actor"):
        self.mode = int(mode)
        self.policy_net = policy
        self.seed = int(seed)
        self.sip_ml_cap = sip_ml_cap
        self.name = name
        self.model_emb: Optional[torch.Tensor] = None
        self._head = None
        self._scratch: Dict[tuple, Dict[str, torch.Tensor]] = {}
        self._empty: Dict[torch.device, torch.Tensor] = {}

    @classmethod
    def policy(cls, policy, deterministic: bool = True, seed: int = 0):
        mode = MODES["policy_greedy" if deterministic else "policy_sample"]
        return cls(mode, policy=policy, seed=seed, name="gnn_policy")

    @classmethod
    def heuristic(cls, name: str, **kwargs):
        """``name`` is a key of ``envs.actors.ACTORS``; ``sip_ml`` takes
        ``max_partitions_per_op`` like ``envs.actors.SiPML``, ``random`` a
        ``seed`` for the Philox key."""
        from ..envs.actors import ACTORS
        if name not in ACTORS:
            raise ValueError(f"unknown heuristic actor {name!r}; "
                             f"one of {sorted(ACTORS)}")
        return cls(MODES[name], seed=kwargs.get("seed", 0),
                   sip_ml_cap=kwargs.get("max_partitions_per_op"), name=name)

    @property
    def is_policy(self) -> bool:
        return self.mode in POLICY_MODES

    # ------------------------------------------------------------------
    @torch.no_grad()
    def prepare(self, vec_env, model_emb: Optional[torch.Tensor] = None):
        """Compute the per-model embedding table once (the policy's weights
        are fixed while the actor is in use): ``policy.gnn`` over the env's
        ``_models_batch`` plus ``graph_mean``.  Heuristics need nothing."""
        if not self.is_policy:
            return self
        if model_emb is None:
            from ..models.gnn import graph_mean
            batch = vec_env._models_batch
            self.policy_net.to(batch.z.device)
            model_emb = graph_mean(self.policy_net.gnn(batch), batch)
        self.model_emb = model_emb.detach().float().contiguous()
        self._head = None
        return self

    def _kernel_serves(self, eng) -> bool:
        if not eng.T["obs_mask"].is_cuda:
            return False
        if self.is_policy:
            return bool(getattr(self.policy_net, "_fused_head_ok", False))
        A = eng.T["obs_mask"].shape[1]
        return A <= 32

    def _rows_for(self, eng) -> Dict[str, torch.Tensor]:
        mask = eng.T["obs_mask"]
        B, A = mask.shape
        key = (mask.device, B, A)
        if key not in self._scratch:
            z = lambda *s: torch.zeros(s, device=mask.device)
            self._scratch[key] = {"gfull": z(B, 17 + A), "lp_all": z(B, A),
                                  "logp": z(B), "value": z(B), "u": z(B)}
        return self._scratch[key]

    @torch.no_grad()
    def act(self, eng, step: int,
            rows: Optional[Dict[str, torch.Tensor]] = None) -> torch.Tensor:
        """Actions ``[B]`` (int32, the engine's own ``T["actions"]`` where it
        has one) for the engine's current observations.  ``rows`` maps
        ``gfull`` / ``lp_all`` / ``logp`` / ``value`` / ``u`` to the row
        tensors the policy modes fill (e.g. slice ``t`` of rollout buffers)."""
        T = eng.T
        if self.is_policy and self.model_emb is None:
            raise RuntimeError("DeviceActor.prepare(vec_env) must run before "
                               "a policy actor acts")
        actions = T.get("actions")
        if self._kernel_serves(eng):
            return self._act_kernel(eng, step, rows, actions)
        sch_acc = T.get("sch_acc")
        if sch_acc is None:
            sch_acc = [None if s is None else s.max_acceptable
                       for s in eng.schedules]
        model_seq = T.get("model_seq")
        if model_seq is None:
            model_seq = np.array([ms.seq_total for ms in eng.spec.models])
        out = act_reference(
            self.mode, T["obs_gf"], T["obs_mask"], T["obs_model"],
            T["obs_sched"], T["done"], policy=self.policy_net,
            model_emb=self.model_emb, model_seq=model_seq, sch_acc=sch_acc,
            sip_ml_cap=self.sip_ml_cap, seed=self.seed, step=step,
            actions=actions, rows=rows)
        return out["actions"]

    def _act_kernel(self, eng, step, rows, actions):
        from .. import ops as hip_ops
        ext = hip_ops.get_extension(required=True)
        T = eng.T
        dev = T["obs_mask"].device
        B = T["obs_mask"].shape[0]
        if actions is None:
            actions = torch.zeros(B, dtype=torch.int32, device=dev)
        empty = self._empty.get(dev)
        if empty is None:
            empty = self._empty[dev] = torch.empty(0, device=dev)
        if self.is_policy:
            if self._head is None:
                self._head = head_params(self.policy_net)
            r = self._rows_for(eng) if rows is None else rows
            missing = [k for k in ROW_KEYS[:4] if k not in r]
            if missing:
                raise ValueError(f"DeviceActor.act: rows lacks {missing}")
            ext.actor_batch(
                T["obs_gf"], T["obs_mask"], T["obs_model"], T["obs_sched"],
                T["done"], self.model_emb, self._head, T["model_seq"],
                T["sch_acc"], self.mode, -1, self.seed & (2 ** 64 - 1),
                int(step) & (2 ** 64 - 1), actions, r["gfull"], r["lp_all"],
                r["logp"], r["value"], r.get("u", empty))
        else:
            cap = -1 if self.sip_ml_cap is None else int(self.sip_ml_cap)
            u = rows.get("u", empty) if rows is not None else empty
            ext.actor_batch(
                T["obs_gf"], T["obs_mask"], T["obs_model"], T["obs_sched"],
                T["done"], empty, [], T["model_seq"], T["sch_acc"],
                self.mode, cap, self.seed & (2 ** 64 - 1),
                int(step) & (2 ** 64 - 1), actions, empty, empty, empty,
                empty, u)
        return actions
