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
"""
from __future__ import annotations

from typing import Dict

import numpy as np
import torch

RING_KEYS = ("s_gfull", "s_model", "action", "ret", "disc", "has_next",
             "n_gfull", "n_model")


class DeviceReplay:
    """``capacity`` n-step transitions over ``feat_dim``-wide state rows
    (``17 + A``: graph features then the action mask)."""

    def __init__(self, capacity: int, feat_dim: int, device):
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
