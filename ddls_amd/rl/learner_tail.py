"""The device learners' optimiser tail as one kernel launch
(``ops/hip/learner_tail.hip``): global grad norm, ``clip_grad_norm_``'s clip,
``torch.optim.Adam``'s update, the step count and the per-minibatch
``acc += stats`` over the parameters' ordinary ``.grad`` tensors.

``DQNConfig.optimizer_step`` / ``ImpalaConfig.optimizer_step`` = ``"fused"``
(device learner only) routes the minibatch loop through ``LearnerTail.step``
in place of ``clip_grad_norm_`` + ``optimizer.step()`` + ``acc += stats_t``.
The moments are the wrapped optimizer's own state tensors, so a checkpoint
saved under either setting continues under the other; the one thing that
differs is where the step count lives (a device f32 here, a host tensor per
parameter in torch), and ``sync_steps`` / ``load_steps`` carry it across.
"""
from __future__ import annotations

from typing import Iterable, Optional

import torch


def learner_tail_reference(params, grads, exp_avg, exp_avg_sq, step_t,
                           stats_out, acc, stats_in, lr, beta1, beta2, eps,
                           max_norm, zero_grads):
    """``ext.learner_tail`` as plain torch, in place and in the dtype of its
    inputs: the float64 oracle of the kernels and the path for CPU tensors.
    ``clip_grad_norm_(max_norm)`` then one Adam step (no amsgrad, no weight
    decay) in torch's operation order, except that the grads themselves are
    left unscaled (zeroed with ``zero_grads``).  ``max_norm <= 0``: no clip,
    norm reported as 0.  ``stats_out[0:2]`` = (norm, clip); with ``acc`` and
    ``stats_in``, ``acc += stats_in``."""
    with torch.no_grad():
        step_t += 1
        step = float(step_t)
        if max_norm > 0:
            norm = torch.linalg.vector_norm(torch.stack(
                [torch.linalg.vector_norm(g) for g in grads]))
            clip = torch.clamp(max_norm / (norm + 1e-6), max=1.0)
        else:
            norm = torch.zeros((), dtype=step_t.dtype, device=step_t.device)
            clip = torch.ones_like(norm)
        bc1 = 1 - beta1 ** step
        bc2_sqrt = (1 - beta2 ** step) ** 0.5
        for p, g, m, v in zip(params, grads, exp_avg, exp_avg_sq):
            gc = g * clip.to(g.dtype) if max_norm > 0 else g
            m.lerp_(gc, 1 - beta1)
            v.mul_(beta2).addcmul_(gc, gc, value=1 - beta2)
            p.addcdiv_(m, (v.sqrt() / bc2_sqrt).add_(eps), value=-(lr / bc1))
            if zero_grads:
                g.zero_()
        stats_out[0] = norm
        stats_out[1] = clip
        if acc is not None:
            acc += stats_in


class LearnerTail:
    """One-launch clip + Adam step over ``params`` with the state of
    ``optimizer`` (a single-group ``torch.optim.Adam`` without amsgrad, weight
    decay or maximize).  Owns ``step_t`` (device f32 [1], the step count of
    every parameter) and ``stats_out`` (device f32 [2]: the last step's grad
    norm and clip factor).  ``max_norm`` None or <= 0 disables the clip."""

    def __init__(self, optimizer: torch.optim.Adam, params: Iterable,
                 max_norm: Optional[float]):
        if not isinstance(optimizer, torch.optim.Adam) \
                or len(optimizer.param_groups) != 1:
            raise ValueError("LearnerTail wraps a single-group "
                             "torch.optim.Adam")
        group = optimizer.param_groups[0]
        if group["amsgrad"] or group["weight_decay"] != 0 \
                or group["maximize"] or torch.is_tensor(group["lr"]):
            raise ValueError("LearnerTail serves plain Adam only: no amsgrad,"
                             " weight decay, maximize or tensor lr")
        self.optimizer = optimizer
        self.params = list(params)
        self.max_norm = float(max_norm) if max_norm else 0.0
        device = self.params[0].device
        self.step_t = torch.zeros(1, dtype=torch.float32, device=device)
        self.stats_out = torch.zeros(2, dtype=torch.float32, device=device)
        # whether step_t is ahead of state[p]["step"]
        self._stepped = False
        for p in self.params:
            self._state(p)
        self.load_steps()

    def _state(self, p):
        """``optimizer.state[p]``, created as Adam's lazy init creates it."""
        state = self.optimizer.state[p]
        if len(state) == 0:
            state["step"] = torch.tensor(0.0, dtype=torch.float32)
            state["exp_avg"] = torch.zeros_like(
                p, memory_format=torch.preserve_format)
            state["exp_avg_sq"] = torch.zeros_like(
                p, memory_format=torch.preserve_format)
        return state

    def step(self, stats_t=None, acc=None) -> bool:
        """Clip and step every parameter that has a grad; with ``stats_t`` and
        ``acc`` (f32, at most 8 values) also ``acc += stats_t``.  True when
        the kernel ran, False when CPU tensors took
        ``learner_tail_reference``."""
        group = self.optimizer.param_groups[0]
        ps = [p for p in self.params if p.grad is not None]
        states = [self._state(p) for p in ps]
        args = (ps, [p.grad.contiguous() for p in ps],
                [s["exp_avg"] for s in states],
                [s["exp_avg_sq"] for s in states], self.step_t,
                self.stats_out, acc,
                None if stats_t is None else stats_t.detach(),
                float(group["lr"]), float(group["betas"][0]),
                float(group["betas"][1]), float(group["eps"]), self.max_norm,
                False)
        self._stepped = True
        if not self.step_t.is_cuda:
            learner_tail_reference(*args)
            return False
        from .. import ops as hip_ops
        hip_ops.get_extension(required=True).learner_tail(*args)
        return True

    def sync_steps(self):
        """Write ``step_t`` into every ``state[p]["step"]`` (one D2H); call
        before ``optimizer.state_dict()``."""
        if not self._stepped:
            return
        step = float(self.step_t.item())
        for p in self.params:
            self._state(p)["step"].fill_(step)
        self._stepped = False

    def load_steps(self):
        """Read ``step_t`` back from the optimizer's state; call after
        ``optimizer.load_state_dict()``."""
        steps = [float(self._state(p)["step"]) for p in self.params]
        self.step_t.fill_(max(steps))
        self._stepped = False
