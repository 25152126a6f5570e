"""Replay ring of n-step transitions that lives on the rollout's device.

The DQN device learner (rl/dqn.py ``learner="device"``) keeps its replay
buffer as eight flat tensors instead of a Python list of tuples.  A
device-resident rollout fragment is turned into n-step transitions and
written into the ring in one launch (``dqn_nstep_ingest`` of
ops/hip/dqn_loss.hip); on CPU tensors (the CpuEngine backend) the same
transitions come from ``rl.dqn.nstep_transitions_reference`` and index
copies.

Slot rule: the k-th transition ever produced goes to slot ``k % capacity``,
which is what a list that appends until it is full and then overwrites from
index 0 holds.  A fragment that yields more than ``capacity`` transitions
stores only its last ``capacity``.  A transition whose return was cut by a
done has ``has_next = 0`` and carries a copy of its own state as next state,
so every row is a valid network input and a minibatch never has to be
compacted.

Prioritized replay (``prioritized=True``).  The ring also owns a sum tree and
a min tree over its slots and the largest priority seen so far.  With ``P``
the smallest power of two ``>= capacity``, ``tree_sum`` and ``tree_min`` are
f64 ``[2P]``: the leaf of slot ``s`` is node ``P + s``, node ``i`` holds
``tree_sum[2i] + tree_sum[2i+1]`` (``fmin`` for the min tree), empty and
padding leaves hold 0 / +inf, and ``max_prio`` (f64 ``[1]``) starts at 1.
Every internal node is the singly rounded f64 sum of its two children, so the
tree is a pure function of its leaves.  New transitions enter at
``max_prio ** alpha``; ``sample(u)`` walks down from the root by prefix mass
and returns the slots with their importance weights
``(min_leaf / leaf) ** beta`` (RLlib's ``(p_i n) ** -beta / max_weight`` with
the common factors cancelled); ``update_priorities`` sets
``(|td| + eps) ** alpha``.  On a GPU these are the three kernels of
ops/hip/per_replay.hip; on CPU tensors they are ``SumTreeReference`` below,
which is also the kernels' oracle.
"""
from __future__ import annotations

from typing import Dict

import numpy as np
import torch

RING_KEYS = ("s_gfull", "s_model", "action", "ret", "disc", "has_next",
             "n_gfull", "n_model")


def tree_leaves(capacity: int) -> int:
    """``P``: the smallest power of two ``>= capacity``."""
    P = 1
    while P < capacity:
        P *= 2
    return P


def rebuild_tree(tree_sum: np.ndarray, tree_min: np.ndarray):
    """Both f64 ``[2P]`` trees rebuilt from their own leaves, level by level:
    what any sequence of ingests and updates must leave, bit for bit."""
    ts = np.array(tree_sum, dtype=np.float64)
    tm = np.array(tree_min, dtype=np.float64)
    width = len(ts) // 4
    while width >= 1:
        i = np.arange(width, 2 * width)
        ts[i] = ts[2 * i] + ts[2 * i + 1]
        tm[i] = np.fmin(tm[2 * i], tm[2 * i + 1])
        width //= 2
    return ts, tm


class SumTreeReference:
    """Plain-numpy mirror of ops/hip/per_replay.hip with the kernels' exact
    semantics.  ``tree_sum`` / ``tree_min`` / ``max_prio`` may be handed in
    (arrays downloaded from the device, say); they are used in place."""

    def __init__(self, capacity: int, alpha: float = 0.9, beta: float = 0.1,
                 eps: float = 1e-6, tree_sum=None, tree_min=None,
                 max_prio=None):
        if capacity < 1:
            raise ValueError("SumTreeReference capacity must be >= 1")
        if alpha < 0 or beta < 0 or not eps > 0:
            raise ValueError("prioritized replay needs alpha >= 0, "
                             "beta >= 0 and eps > 0")
        self.capacity = int(capacity)
        self.alpha, self.beta, self.eps = float(alpha), float(beta), float(eps)
        P = self.P = tree_leaves(self.capacity)
        self.tree_sum = (np.zeros(2 * P, dtype=np.float64)
                         if tree_sum is None else tree_sum)
        self.tree_min = (np.full(2 * P, np.inf, dtype=np.float64)
                         if tree_min is None else tree_min)
        self.max_prio = (np.ones(1, dtype=np.float64)
                         if max_prio is None else max_prio)
        for a, n in ((self.tree_sum, 2 * P), (self.tree_min, 2 * P),
                     (self.max_prio, 1)):
            assert a.dtype == np.float64 and a.shape == (n,)

    def _refresh(self, nodes: np.ndarray):
        """Recompute the ancestors of leaf nodes ``nodes``, level by level."""
        ts, tm = self.tree_sum, self.tree_min
        while len(nodes) and nodes[0] > 1:
            nodes = np.unique(nodes >> 1)
            ts[nodes] = ts[2 * nodes] + ts[2 * nodes + 1]
            tm[nodes] = np.fmin(tm[2 * nodes], tm[2 * nodes + 1])

    def ingest(self, start: int, count: int):
        """Slots ``[start, start + count)`` mod capacity (``count <=
        capacity``) enter at ``max_prio ** alpha``."""
        C = self.capacity
        assert 0 <= start < C and 0 <= count <= C
        if count == 0:
            return
        slots = np.unique((start + np.arange(count, dtype=np.int64)) % C)
        leaf = np.power(self.max_prio[0], np.float64(self.alpha))
        self.tree_sum[self.P + slots] = leaf
        self.tree_min[self.P + slots] = leaf
        self._refresh(self.P + slots)

    def sample(self, u):
        """``u`` f64 in [0, 1) -> (slots int64, importance weights f32).
        From node 1: left if ``mass < left or right == 0``, else
        ``mass -= left`` and right; the guard keeps the walk on nodes with a
        positive sum, so it ends on a filled slot."""
        ts = self.tree_sum
        u = np.asarray(u, dtype=np.float64).reshape(-1)
        mass = u * ts[1]
        node = np.ones(len(u), dtype=np.int64)
        width = 1
        while width < self.P:
            left, right = ts[2 * node], ts[2 * node + 1]
            go_left = (mass < left) | (right == 0.0)
            mass = np.where(go_left, mass, mass - left)
            node = np.where(go_left, 2 * node, 2 * node + 1)
            width *= 2
        with np.errstate(divide="ignore", invalid="ignore"):
            weight = np.power(self.tree_min[1] / ts[node],
                              np.float64(self.beta))
        return node - self.P, weight.astype(np.float32)

    def update(self, idx, td_abs):
        """Leaves of ``idx`` become ``(td_abs + eps) ** alpha``; where a slot
        occurs more than once its last occurrence wins.  ``max_prio`` takes
        every ``td_abs + eps``, the overwritten ones included."""
        idx = np.asarray(idx, dtype=np.int64).reshape(-1)
        p = np.asarray(td_abs, dtype=np.float64).reshape(-1) + self.eps
        assert len(idx) == len(p)
        ok = (idx >= 0) & (idx < self.capacity)
        idx, p = idx[ok], p[ok]
        if not len(idx):
            return
        self.max_prio[0] = max(self.max_prio[0], p.max())
        # first occurrence in the reversed batch = last occurrence
        slots, rev = np.unique(idx[::-1], return_index=True)
        leaf = np.power(p[::-1][rev], np.float64(self.alpha))
        self.tree_sum[self.P + slots] = leaf
        self.tree_min[self.P + slots] = leaf
        self._refresh(self.P + slots)


class DeviceReplay:
    """``capacity`` n-step transitions over ``feat_dim``-wide state rows
    (``17 + A``: graph features then the action mask)."""

    def __init__(self, capacity: int, feat_dim: int, device, *,
                 prioritized: bool = False, alpha: float = 0.9,
                 beta: float = 0.1, eps: float = 1e-6):
        if capacity < 1:
            raise ValueError("DeviceReplay capacity must be >= 1")
        self.capacity = int(capacity)
        self.feat_dim = int(feat_dim)
        self.device = torch.device(device)
        C, F, dev = self.capacity, self.feat_dim, self.device
        f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)
        i64 = lambda *s: torch.zeros(s, dtype=torch.int64, device=dev)
        self.s_gfull = f32(C, F)
        self.s_model = i64(C)
        self.action = i64(C)
        self.ret = f32(C)
        self.disc = f32(C)
        self.has_next = f32(C)
        self.n_gfull = f32(C, F)
        self.n_model = i64(C)
        # transitions produced so far (stored or not)
        self.written = 0
        self.prioritized = bool(prioritized)
        self.alpha, self.beta, self.eps = float(alpha), float(beta), float(eps)
        if self.prioritized:
            # the mirror validates alpha / beta / eps; on CPU tensors it is
            # also the implementation, and the tensors share its memory
            ref = SumTreeReference(C, alpha, beta, eps)
            if dev.type == "cuda":
                self._tree = None
                self.tree_sum = torch.from_numpy(ref.tree_sum).to(dev)
                self.tree_min = torch.from_numpy(ref.tree_min).to(dev)
                self.max_prio = torch.from_numpy(ref.max_prio).to(dev)
            else:
                self._tree = ref
                self.tree_sum = torch.from_numpy(ref.tree_sum)
                self.tree_min = torch.from_numpy(ref.tree_min)
                self.max_prio = torch.from_numpy(ref.max_prio)

    def __len__(self):
        return min(self.written, self.capacity)

    def ring(self):
        return [getattr(self, k) for k in RING_KEYS]

    def ingest(self, data: Dict, n_step: int, gamma: float) -> int:
        """Write the n-step transitions of a device-resident [T, N] fragment
        (``EngineVectorEnv.rollout(device_resident=True)``) into the ring;
        returns how many the fragment yields."""
        T, N = data["rewards"].shape
        gfull = data["gfull_dev"]
        if gfull.is_cuda:
            from .. import ops as hip_ops
            ext = hip_ops.get_extension(required=True)
            K = ext.dqn_nstep_ingest(
                gfull, data["model_ids_dev"], data["actions_dev"],
                data["rewards_dev"], data["dones_dev"], self.ring(), int(T),
                int(N), self.capacity, self.written, int(n_step),
                float(gamma))
        else:
            K = self._ingest_cpu(data, T, N, n_step, gamma)
        if self.prioritized and K > 0:
            # the slots just written: the last min(K, C) transitions
            C = self.capacity
            start = (self.written + max(int(K) - C, 0)) % C
            count = min(int(K), C)
            if self._tree is None:
                ext.per_ingest(self.tree_sum, self.tree_min, self.max_prio,
                               start, count, C, self.alpha)
            else:
                self._tree.ingest(start, count)
        self.written += int(K)
        return int(K)

    def _ingest_cpu(self, data, T, N, n_step, gamma) -> int:
        K = (T - n_step) * N
        if K <= 0:
            return 0
        from .dqn import nstep_transitions_reference
        ret, disc, has_next, steps = nstep_transitions_reference(
            data["rewards_dev"].reshape(T, N).numpy(),
            data["dones_dev"].reshape(T, N).numpy(), n_step, gamma)
        k = np.arange(max(K - self.capacity, 0), K)
        slots = torch.from_numpy((self.written + k) % self.capacity)
        has_next = has_next.reshape(-1)[k]
        nrow = np.where(has_next, k + steps.reshape(-1)[k] * N, k)
        k_t, nrow_t = torch.from_numpy(k), torch.from_numpy(nrow)
        gfull, mids = data["gfull_dev"], data["model_ids_dev"]
        self.s_gfull[slots] = gfull[k_t]
        self.s_model[slots] = mids[k_t]
        self.action[slots] = data["actions_dev"][k_t]
        self.ret[slots] = torch.from_numpy(ret.reshape(-1)[k])
        self.disc[slots] = torch.from_numpy(disc.reshape(-1)[k])
        self.has_next[slots] = torch.from_numpy(
            has_next.astype(np.float32))
        self.n_gfull[slots] = gfull[nrow_t]
        self.n_model[slots] = mids[nrow_t]
        return K

    def gather(self, idx: torch.Tensor) -> Dict[str, torch.Tensor]:
        """The minibatch at ring slots ``idx`` (int64, on the ring's
        device)."""
        return {k: getattr(self, k).index_select(0, idx) for k in RING_KEYS}

    def _need_prioritized(self):
        if not self.prioritized:
            raise RuntimeError("this DeviceReplay was made with "
                               "prioritized=False")

    def sample(self, u: torch.Tensor):
        """Slots drawn in proportion to their priorities, one per uniform in
        ``u`` (f64 in [0, 1), on the ring's device), and their importance
        weights: ``(idx int64, weight f32)``."""
        self._need_prioritized()
        if len(self) == 0:
            raise RuntimeError("cannot sample from an empty replay")
        if self._tree is None:
            from .. import ops as hip_ops
            ext = hip_ops.get_extension(required=True)
            idx, weight = ext.per_sample(self.tree_sum, self.tree_min,
                                         u.reshape(-1), self.capacity,
                                         self.beta)
            return idx, weight
        idx, weight = self._tree.sample(u.numpy())
        return torch.from_numpy(idx), torch.from_numpy(weight)

    def update_priorities(self, idx: torch.Tensor, td_abs: torch.Tensor):
        """New priorities ``(td_abs + eps) ** alpha`` for the slots ``idx``
        (``td_abs`` f64, one per slot; on a repeated slot the last wins)."""
        self._need_prioritized()
        if self._tree is None:
            from .. import ops as hip_ops
            ext = hip_ops.get_extension(required=True)
            ext.per_update(self.tree_sum, self.tree_min, self.max_prio, idx,
                           td_abs, self.capacity, self.alpha, self.eps)
        else:
            self._tree.update(idx.numpy(), td_abs.detach().numpy())
