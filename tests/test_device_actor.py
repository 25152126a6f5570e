"""Device-side actors (rl/device_actor.py + ops/hip/actor.hip).

CPU: ``act_reference`` against the ``envs/actors.py`` classes, the numpy
Philox against the Random123 known answer.  GPU: the ``actor_batch`` kernel
against ``act_reference`` — heuristics exactly, the policy head within the
tolerance ``head_fwd`` is held to, the sampler's ``u`` bitwise.
"""
import math

import numpy as np
import pytest
import torch

from ddls_amd.envs.actors import ACTORS
from ddls_amd.rl.device_actor import (MODES, act_reference, head_params,
                                      philox4x32_10, philox_uniform)

A = 17
MODEL_SEQ = np.array([12.0, 37.5, 90.0])       # M = 3
SIP_CAP = 8
DETERMINISTIC = ("no_parallelism", "min_parallelism", "max_parallelism",
                 "sip_ml", "acceptable_jct")
GPU_BATCHES = (1, 3, 4, 5, 67)   # < block, one block, block + 1, ragged grid
POLICY_SEED = 0                  # test_policy_reference_gap_share pins it


def _cases():
    """~500 random masks with mask[0] = 1 plus the edge cases, a model id
    per row and a max-acceptable JCT per row whose ratio seq/acc covers
    exact integers, non-integers and values above A."""
    rng = np.random.RandomState(0)
    masks = (rng.rand(500, A) < rng.rand(500, 1)).astype(np.float32)
    masks[:, 0] = 1.0
    edge = np.zeros((5, A), dtype=np.float32)
    edge[0, [0]] = 1
    edge[1, [0, 1]] = 1
    edge[2, [0, 1, 2]] = 1
    edge[3, :] = 1
    edge[4, [0, 1, 2, 4, 8, 16]] = 1
    masks = np.concatenate([edge, masks])
    # every edge mask meets every ratio class once more
    masks = np.concatenate([masks, np.tile(edge, (6, 1))])
    n = len(masks)
    mids = (np.arange(n) % 3).astype(np.int32)
    seq = MODEL_SEQ[mids]
    ratio = rng.uniform(0.3, 20.0, size=n)         # some above A = 17
    ratio[::4] = rng.randint(1, 18, size=len(ratio[::4]))   # exact integers
    ratio[-30:] = np.repeat([1.0, 2.0, 4.0, 16.0, 17.0, 40.0], 5)
    acc = seq / ratio
    return masks, mids, acc


class _Job:
    def __init__(self, seq, acc):
        self.details = {
            "job_sequential_completion_time": {"A100": seq},
            "max_acceptable_job_completion_time": {"A100": acc}}


def _reference_inputs(masks, mids, acc, done=None):
    n = len(masks)
    t = torch.as_tensor
    return dict(
        obs_gf=torch.zeros(n, 17), obs_mask=t(masks), obs_model=t(mids),
        obs_sched=torch.zeros(n, dtype=torch.int32),
        done=torch.zeros(n, dtype=torch.uint8) if done is None else t(done),
        model_seq=t(MODEL_SEQ), sch_acc=t(acc.reshape(n, 1)))


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
def test_reference_heuristics_match_actor_classes():
    masks, mids, acc = _cases()
    ratios = MODEL_SEQ[mids] / acc
    assert (ratios == np.round(ratios)).sum() > 50      # exact integers
    assert (ratios > A).sum() > 10                      # above A
    inp = _reference_inputs(masks, mids, acc)
    for name in DETERMINISTIC:
        kwargs = {"max_partitions_per_op": SIP_CAP} if name == "sip_ml" else {}
        actor = ACTORS[name](**kwargs)
        got = act_reference(MODES[name], sip_ml_cap=SIP_CAP, **inp)["actions"]
        want = [actor.compute_action(
            {"action_set": np.arange(A), "action_mask": masks[i]},
            job_to_place=_Job(float(MODEL_SEQ[mids[i]]), float(acc[i])))
            for i in range(len(masks))]
        np.testing.assert_array_equal(got.numpy(), np.array(want), err_msg=name)
    # SiP-ML without a cap is max_allowed
    got = act_reference(MODES["sip_ml"], sip_ml_cap=None, **inp)["actions"]
    want = [ACTORS["sip_ml"]().compute_action(
        {"action_set": np.arange(A), "action_mask": m}) for m in masks]
    np.testing.assert_array_equal(got.numpy(), np.array(want))


def test_reference_random_follows_documented_formula():
    masks, mids, acc = _cases()
    inp = _reference_inputs(masks, mids, acc)
    seen = set()
    for step in range(4):
        out = act_reference(MODES["random"], seed=5, step=step, **inp)
        u = philox_uniform(5, step, len(masks))
        np.testing.assert_array_equal(out["u"].numpy(), u)
        for i, m in enumerate(masks):
            valid = np.flatnonzero(m)
            a = int(out["actions"][i])
            if len(valid) == 1:
                assert a == valid[0]
                continue
            assert a in valid[1:]
            n = len(valid)
            idx = min(n - 2, int(math.floor(np.float32(u[i])
                                            * np.float32(n - 1))))
            assert a == valid[1:][idx]
            seen.add(idx)
    assert len(seen) > 8      # the draw really moves across valid[1:]


def test_reference_done_envs_get_action_zero():
    masks, mids, acc = _cases()
    done = np.zeros(len(masks), dtype=np.uint8)
    done[::3] = 1
    inp = _reference_inputs(masks, mids, acc, done)
    got = act_reference(MODES["max_parallelism"], **inp)["actions"].numpy()
    assert (got[::3] == 0).all()
    assert (got[1::3] > 0).any()


def test_philox_known_answer_and_uniform_range():
    # Random123 kat_vectors: philox4x32-10, counter 0, key 0
    out = philox4x32_10(np.zeros(4, dtype=np.uint32),
                        np.zeros(2, dtype=np.uint32))
    assert [f"{int(x):08x}" for x in out] == [
        "6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8"]
    # ... and all-ones counter and key
    ones = np.full(4, 0xFFFFFFFF, dtype=np.uint32)
    out = philox4x32_10(ones, ones[:2])
    assert [f"{int(x):08x}" for x in out] == [
        "408f276d", "41c83b0e", "a20bc7c6", "6d5451fd"]
    u = np.concatenate([philox_uniform(seed, step, 512)
                        for seed in (0, 7, 2 ** 63 + 5)
                        for step in (0, 1, 2 ** 40)])
    assert u.dtype == np.float32
    assert (u >= 0).all() and (u < 1).all()
    assert len(np.unique(u)) > 0.99 * len(u)
    assert 0.45 < u.mean() < 0.55
    # the largest word still maps below 1
    top = np.float32(0xFFFFFFFF >> 8) * np.float32(2.0 ** -24)
    assert top < 1.0


def _policy_case(num_actions, B, seed=POLICY_SEED):
    """A random-init policy, a random embedding table and B observations."""
    from ddls_amd.models.gnn import GNNPolicy
    torch.manual_seed(seed)
    policy = GNNPolicy(num_actions=num_actions)
    assert policy._fused_head_ok
    g = torch.Generator().manual_seed(1000 * seed + B)
    model_emb = torch.randn(3, 16, generator=g)
    obs_gf = torch.randn(B, 17, generator=g)
    mask = (torch.rand(B, num_actions, generator=g)
            < torch.rand(B, 1, generator=g)).float()
    mask[:, 0] = 1.0
    if B >= 4:
        mask[3, :] = 1.0
    obs_model = torch.randint(0, 3, (B,), generator=g).int()
    done = torch.zeros(B, dtype=torch.uint8)
    if B >= 5:
        done[1] = 1
    return policy, dict(obs_gf=obs_gf, obs_mask=mask, obs_model=obs_model,
                        obs_sched=torch.zeros(B, dtype=torch.int32),
                        done=done, model_emb=model_emb)


POLICY_CASES = [(17, B) for B in GPU_BATCHES] + [(5, 67)]


def _top_two_gap(logits):
    top = torch.topk(logits, 2, dim=1).values
    return (top[:, 0] - top[:, 1]).numpy()


def test_policy_reference_gap_share():
    """The GPU greedy test skips rows whose reference top-two gap is within
    2e-4; with POLICY_SEED that is at most 5% of the rows (CPU-checkable)."""
    gaps = []
    for num_actions, B in POLICY_CASES:
        policy, inp = _policy_case(num_actions, B)
        out = act_reference(MODES["policy_greedy"], policy=policy, **inp)
        assert out["lp_all"].shape == (B, num_actions)
        assert out["gfull"].shape == (B, 17 + num_actions)
        live = inp["done"].numpy() == 0
        multi = inp["obs_mask"].sum(1).numpy() > 1
        gaps.append(_top_two_gap(out["logits"])[live & multi])
        acts = out["actions"].long()
        assert (inp["obs_mask"].gather(1, acts.view(-1, 1)) > 0).all()
    gaps = np.concatenate(gaps)
    assert (gaps <= 2e-4).mean() <= 0.05


def test_reference_sampler_never_returns_masked_action():
    policy, inp = _policy_case(17, 67)
    for step in range(8):
        out = act_reference(MODES["policy_sample"], policy=policy, seed=3,
                            step=step, **inp)
        acts = out["actions"].long()
        live = inp["done"] == 0
        assert (inp["obs_mask"].gather(1, acts.view(-1, 1)) > 0).all()
        np.testing.assert_array_equal(
            out["logp"][live].numpy(),
            out["lp_all"].gather(1, acts.view(-1, 1)).squeeze(1)[live].numpy())


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
def _ext():
    from ddls_amd import ops
    return ops.get_extension(required=True)


def _kernel(mode, inp, head=(), sip_ml_cap=-1, seed=0, step=0, sentinel=-7.0):
    """Launch actor_batch on cuda copies of ``inp``; rows pre-filled with a
    sentinel so untouched rows are visible."""
    dev = torch.device("cuda:0")
    B, num_actions = inp["obs_mask"].shape
    c = lambda k: inp[k].to(dev).contiguous()
    empty = torch.empty(0, device=dev)
    f = lambda *s: torch.full(s, sentinel, device=dev)
    rows = {"gfull": f(B, 17 + num_actions), "lp_all": f(B, num_actions),
            "logp": f(B), "value": f(B), "u": f(B)}
    actions = torch.full((B,), -1, dtype=torch.int32, device=dev)
    policy_mode = mode in (MODES["policy_greedy"], MODES["policy_sample"])
    _ext().actor_batch(
        c("obs_gf"), c("obs_mask"), c("obs_model"), c("obs_sched"), c("done"),
        c("model_emb") if policy_mode else empty,
        [p.to(dev) for p in head],
        c("model_seq") if "model_seq" in inp else empty.double(),
        c("sch_acc") if "sch_acc" in inp else empty.double(),
        mode, sip_ml_cap, seed, step, actions,
        rows["gfull"] if policy_mode else empty,
        rows["lp_all"] if policy_mode else empty,
        rows["logp"] if policy_mode else empty,
        rows["value"] if policy_mode else empty, rows["u"])
    torch.cuda.synchronize()
    out = {k: v.cpu() for k, v in rows.items()}
    out["actions"] = actions.cpu()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("B", GPU_BATCHES + (535,))
def test_kernel_heuristics_equal_reference(B):
    masks, mids, acc = _cases()
    assert len(masks) == 535
    done = np.zeros(B, dtype=np.uint8)
    done[1::4] = 1
    inp = _reference_inputs(masks[:B], mids[:B], acc[:B], done)
    for name in DETERMINISTIC + ("random",):
        for step in (0, 3):
            ref = act_reference(MODES[name], sip_ml_cap=SIP_CAP, seed=11,
                                step=step, **inp)
            got = _kernel(MODES[name], inp, sip_ml_cap=SIP_CAP, seed=11,
                          step=step)
            np.testing.assert_array_equal(got["actions"].numpy(),
                                          ref["actions"].numpy(), err_msg=name)
            assert (got["actions"][1::4] == 0).all()
            live = torch.as_tensor(done == 0)
            if name == "random":
                np.testing.assert_array_equal(got["u"][live].numpy(),
                                              ref["u"][live].numpy())
            else:
                assert (got["u"] == -7.0).all()
            assert (got["u"][~live] == -7.0).all()
            for k in ("gfull", "lp_all", "logp", "value"):
                assert (got[k] == -7.0).all(), (name, k)


@pytest.mark.gpu
def test_kernel_policy_head_matches_reference():
    excluded = total = 0
    for num_actions, B in POLICY_CASES:
        policy, inp = _policy_case(num_actions, B)
        head = head_params(policy)
        ref = act_reference(MODES["policy_greedy"], policy=policy, **inp)
        got = _kernel(MODES["policy_greedy"], inp, head=head)
        live = inp["done"] == 0
        valid = (inp["obs_mask"] > 0) & live.view(-1, 1)
        np.testing.assert_array_equal(got["gfull"][live].numpy(),
                                      ref["gfull"][live].numpy())
        np.testing.assert_allclose(got["value"][live].numpy(),
                                   ref["value"][live].numpy(), atol=1e-4,
                                   rtol=0)
        np.testing.assert_allclose(got["lp_all"][valid].numpy(),
                                   ref["lp_all"][valid].numpy(), atol=1e-4,
                                   rtol=0)
        acts = got["actions"].long()
        np.testing.assert_array_equal(
            got["logp"][live].numpy(),
            got["lp_all"].gather(1, acts.view(-1, 1)).squeeze(1)[live].numpy())
        # done rows: action 0, every row keeps its sentinel
        assert (got["actions"][~live] == 0).all()
        for k in ("gfull", "lp_all", "logp", "value", "u"):
            assert (got[k][~live] == -7.0).all(), k
        multi = inp["obs_mask"].sum(1) > 1
        sure = torch.as_tensor(_top_two_gap(ref["logits"]) > 2e-4) | ~multi
        sel = live & sure
        np.testing.assert_array_equal(got["actions"][sel].numpy(),
                                      ref["actions"][sel].numpy())
        excluded += int((live & ~sure).sum())
        total += int(live.sum())
    assert excluded <= 0.05 * total, (excluded, total)


@pytest.mark.gpu
def test_kernel_sampler_4096_draws():
    B, steps, seed = 64, 64, 2 ** 40 + 17
    policy, inp = _policy_case(17, B)
    inp["done"] = torch.zeros(B, dtype=torch.uint8)
    head = head_params(policy)
    mask = inp["obs_mask"].numpy()
    near = draws = 0
    for step in range(steps):
        got = _kernel(MODES["policy_sample"], inp, head=head, seed=seed,
                      step=step)
        u = got["u"].numpy()
        assert u.tobytes() == philox_uniform(seed, step, B).tobytes()
        acts = got["actions"].numpy()
        assert (mask[np.arange(B), acts] > 0).all()     # never masked
        # host inverse CDF in f64 from the kernel's own lp_all
        cum = np.cumsum(np.exp(got["lp_all"].numpy().astype(np.float64)),
                        axis=1)
        for b in range(B):
            draws += 1
            if np.abs(cum[b] - float(u[b])).min() < 1e-5:
                near += 1
                continue
            hit = np.flatnonzero((mask[b] > 0) & (float(u[b]) < cum[b]))
            want = hit[0] if len(hit) else np.flatnonzero(mask[b])[-1]
            assert acts[b] == want, (step, b)
    assert draws == 4096 and near <= 0.01 * draws, near
