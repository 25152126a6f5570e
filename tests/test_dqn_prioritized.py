"""Prioritized replay on the DQN replay ring: the numpy sum tree
(rl/device_replay.py ``SumTreeReference``), the sum-tree kernels
(ops/hip/per_replay.hip), the importance-weighted TD loss
(``dqn_loss_fwd_weighted``) and both learners with
``DQNConfig.prioritized_replay``."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.test_dqn_device import (  # noqa: F401
    COMBOS, EPS32, GAMMA, ORDER, _fragment, _hold_to_float64_bound,
    _host_ingester, _leaves, _loss_inputs, _reference, _to, make_env,
    multi_model_files)

ALPHA, BETA, EPS = 0.9, 0.1, 1e-6
U_EDGES = [0.0, 1.0 - 2.0 ** -53, 0.5]
CAPACITIES = [1, 2, 5, 37, 1000]


# ---------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------
def _tree(C, **kw):
    from ddls_amd.rl.device_replay import SumTreeReference
    return SumTreeReference(C, kw.pop("alpha", ALPHA), kw.pop("beta", BETA),
                            kw.pop("eps", EPS), **kw)


def _assert_is_rebuild(tree_sum, tree_min, C):
    """Internal nodes of both trees against a straight numpy rebuild from
    the leaves, bit for bit; padding leaves untouched."""
    from ddls_amd.rl.device_replay import rebuild_tree, tree_leaves
    P = tree_leaves(C)
    assert tree_sum.shape == tree_min.shape == (2 * P,)
    want_sum, want_min = rebuild_tree(tree_sum, tree_min)
    assert np.array_equal(tree_sum[1:], want_sum[1:])
    assert np.array_equal(tree_min[1:], want_min[1:])
    # an independent spelling of the same rule for the sum tree
    node = tree_sum[P:].copy()
    while len(node) > 1:
        node = node[0::2] + node[1::2]
        assert np.array_equal(tree_sum[len(node):2 * len(node)], node)
    assert np.all(tree_sum[P + C:] == 0.0)
    assert np.all(np.isposinf(tree_min[P + C:]))


def _filled_tree(C, seed):
    """Priorities log-uniform over [1e-7, 2000] raised to alpha; from C = 5
    up two slots stay empty.  Returns (tree, filled mask)."""
    rng = np.random.RandomState(seed)
    t = _tree(C)
    prio = np.exp(rng.uniform(np.log(1e-7), np.log(2000.0), size=C))
    filled = np.ones(C, dtype=bool)
    if C >= 5:
        filled[rng.choice(C, size=2, replace=False)] = False
    slots = np.nonzero(filled)[0]
    # |td| = prio - eps, so the leaf is prio ** alpha
    t.update(slots, prio[slots] - EPS)
    return t, filled


# ---------------------------------------------------------------------------
# CPU: the mirror
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("C", CAPACITIES)
def test_mirror_tree_is_a_rebuild_and_draws_filled_slots(C):
    t, filled = _filled_tree(C, seed=C)
    _assert_is_rebuild(t.tree_sum, t.tree_min, C)
    leaves = t.tree_sum[t.P:t.P + C]
    assert np.all(leaves[filled] > 0) and np.all(leaves[~filled] == 0)
    assert np.array_equal(t.tree_min[t.P:t.P + C][filled], leaves[filled])
    u = np.concatenate([U_EDGES, np.random.RandomState(C + 1)
                        .random_sample(20000)])
    idx, w = t.sample(u)
    assert idx.dtype == np.int64 and w.dtype == np.float32
    assert idx.min() >= 0 and idx.max() < C
    assert filled[idx].all() and np.all(leaves[idx] > 0)
    assert np.all(np.isfinite(w)) and np.all(w > 0) and np.all(w <= 1)


def test_mirror_draws_in_proportion_to_the_leaves():
    """Leaves 1..37 (P = 64), 200000 draws: every slot's count is within
    5 sigma of n * leaf / sum."""
    C, n = 37, 200000
    t = _tree(C, alpha=1.0)
    t.update(np.arange(C), np.arange(1, C + 1) - EPS)
    leaves = t.tree_sum[t.P:t.P + C]
    assert np.allclose(leaves, np.arange(1, C + 1), rtol=1e-12)
    idx, _ = t.sample(np.random.RandomState(1).random_sample(n))
    p = leaves / leaves.sum()
    z = (np.bincount(idx, minlength=C) - n * p) / np.sqrt(n * p * (1 - p))
    print("max |z|", np.abs(z).max())
    assert np.abs(z).max() < 5


def test_mirror_weights():
    t, filled = _filled_tree(37, seed=3)
    leaves = t.tree_sum[t.P:t.P + 37]
    u = np.random.RandomState(4).random_sample(5000)
    idx, w = t.sample(u)
    min_leaf = leaves[filled].min()
    assert t.tree_min[1] == min_leaf
    want = (min_leaf / leaves[idx]) ** BETA
    assert np.array_equal(w, want.astype(np.float32))
    assert w.max() <= 1.0
    # the slot with the smallest priority carries the largest weight, 1:
    # aim a draw at the middle of its mass interval
    rare = int(np.argmin(np.where(filled, leaves, np.inf)))
    mid = (leaves[:rare].sum() + 0.5 * leaves[rare]) / leaves.sum()
    i1, w1 = t.sample(np.array([mid]))
    assert i1[0] == rare and w1[0] == 1.0
    t0 = _tree(37, beta=0.0, tree_sum=t.tree_sum, tree_min=t.tree_min,
               max_prio=t.max_prio)
    i0, w0 = t0.sample(u)
    assert np.array_equal(i0, idx) and np.all(w0 == 1.0)


def test_mirror_update_last_wins_and_max_prio_is_monotone():
    C = 5
    t = _tree(C)
    t.ingest(0, C)
    assert np.all(t.tree_sum[t.P:t.P + C] == 1.0) and t.max_prio[0] == 1.0
    # slot 3 three times, slot 1 twice; the largest value (7) is overwritten
    idx = np.array([3, 1, 3, 0, 1, 3])
    td = np.array([7.0, 0.5, 2.0, 0.25, 3.0, 0.125])
    t.update(idx, td)
    leaves = t.tree_sum[t.P:t.P + C]
    assert leaves[3] == np.power(0.125 + EPS, ALPHA)
    assert leaves[1] == np.power(3.0 + EPS, ALPHA)
    assert leaves[0] == np.power(0.25 + EPS, ALPHA)
    assert leaves[2] == 1.0 and leaves[4] == 1.0
    assert t.max_prio[0] == 7.0 + EPS
    _assert_is_rebuild(t.tree_sum, t.tree_min, C)
    # a smaller batch leaves max_prio alone; a larger value raises it
    t.update(np.array([2]), np.array([0.5]))
    assert t.max_prio[0] == 7.0 + EPS
    t.update(np.array([2, 2]), np.array([9.0, 0.5]))
    assert t.max_prio[0] == 9.0 + EPS
    assert t.tree_sum[t.P + 2] == np.power(0.5 + EPS, ALPHA)
    _assert_is_rebuild(t.tree_sum, t.tree_min, C)
    # out-of-range slots are skipped
    before = t.tree_sum.copy()
    t.update(np.array([-1, C]), np.array([100.0, 100.0]))
    assert np.array_equal(t.tree_sum, before) and t.max_prio[0] == 9.0 + EPS


def _prioritized_replay(C, device="cpu", A=17):
    from ddls_amd.rl.device_replay import DeviceReplay
    return DeviceReplay(C, 17 + A, device, prioritized=True, alpha=ALPHA,
                        beta=BETA, eps=EPS)


def test_ingest_resets_exactly_the_overwritten_slots():
    """C = 37 and the three fragments of
    test_device_replay_wraps_inside_a_fragment (27, 18, 18 transitions):
    after each ingest the slots it wrote, and only those, hold
    max_prio ** alpha."""
    A, n, C = 17, 3, 37
    replay = _prioritized_replay(C)
    assert torch.all(replay.tree_sum == 0) and replay.max_prio.item() == 1.0
    written, wrapped = 0, []
    for i, (T, N) in enumerate([(12, 3), (9, 3), (9, 3)]):
        # give every filled slot its own priority, raising max_prio
        if len(replay):
            idx = torch.arange(len(replay))
            replay.update_priorities(
                idx, torch.linspace(0.1, 2.0 + i, len(replay)).double())
        before = replay.tree_sum.clone()
        K = replay.ingest(_fragment(T, N, n, A=A, seed=60 + i), n, GAMMA)
        slots = (written + np.arange(K)) % C
        written += K
        fresh = np.power(replay.max_prio.item(), ALPHA)
        assert fresh > 1.0 or i == 0
        P = replay._tree.P
        touched = np.zeros(C, dtype=bool)
        touched[slots] = True
        leaves = replay.tree_sum[P:P + C].numpy()
        assert np.all(leaves[touched] == fresh)
        assert np.array_equal(leaves[~touched], before[P:P + C].numpy()
                              [~touched])
        assert np.array_equal(replay.tree_min[P:P + C].numpy()[touched],
                              leaves[touched])
        _assert_is_rebuild(replay.tree_sum.numpy(), replay.tree_min.numpy(),
                           C)
        wrapped.append(bool(touched[0] and touched[36]
                            and touched.sum() == 18))
    assert replay.written == 63 and wrapped == [False, True, False]


def test_ingest_longer_than_the_ring_resets_every_slot():
    A, n, C = 17, 3, 5
    replay = _prioritized_replay(C)
    replay.ingest(_fragment(9, 3, n, A=A, seed=1), n, GAMMA)
    replay.update_priorities(torch.arange(C),
                             torch.tensor([3.0, 0.1, 0.2, 0.3, 0.4]).double())
    assert replay.ingest(_fragment(9, 3, n, A=A, seed=2), n, GAMMA) == 18 > C
    P = replay._tree.P
    assert np.all(replay.tree_sum[P:P + C].numpy()
                  == np.power(3.0 + EPS, ALPHA))
    _assert_is_rebuild(replay.tree_sum.numpy(), replay.tree_min.numpy(), C)
    idx, w = replay.sample(torch.tensor(U_EDGES, dtype=torch.float64))
    assert idx.dtype == torch.int64 and w.dtype == torch.float32
    assert idx.tolist() == [0, 4, 2] and torch.all(w == 1.0)


def test_uniform_replay_has_no_priorities():
    from ddls_amd.rl.device_replay import DeviceReplay
    replay = DeviceReplay(5, 34, "cpu")
    assert not replay.prioritized and not hasattr(replay, "tree_sum")
    with pytest.raises(RuntimeError):
        replay.sample(torch.zeros(1, dtype=torch.float64))
    with pytest.raises(ValueError):
        DeviceReplay(5, 34, "cpu", prioritized=True, alpha=-0.1)


@pytest.mark.parametrize("dueling,double_q", COMBOS)
def test_loss_reference_with_weights(dueling, double_q):
    """Float64, against the literal mean(w * smooth_l1(reduction='none'));
    weights=None gives today's bits."""
    from ddls_amd.rl.dqn import STAT_KEYS, dqn_loss_reference, dueling_q
    inp = _loss_inputs(40, 17, seed=5)
    x = {k: (v.double() if v.is_floating_point() else v)
         for k, v in inp.items()}
    g = torch.Generator(device="cpu").manual_seed(9)
    w = torch.rand(41, generator=g, dtype=torch.float64) * 0.9 + 0.1
    args = [x[k] for k in ORDER] + [-4.0, 4.0, dueling, double_q]
    loss, st = dqn_loss_reference(*args, weights=w)
    plain, st_plain = dqn_loss_reference(*args)
    none, st_none = dqn_loss_reference(*args, weights=None)
    assert torch.equal(plain, none) and set(st_plain) == set(STAT_KEYS)
    q_a = dueling_q(x["logits_s"], x["values_s"], dueling).gather(
        1, x["actions"].unsqueeze(1)).squeeze(1)
    target = _target(x, dueling, double_q)
    # today's expression, today's bits
    assert torch.equal(plain, F.smooth_l1_loss(q_a, target))
    want = (w * F.smooth_l1_loss(q_a, target, reduction="none")).mean()
    assert loss.item() == pytest.approx(want.item(), rel=1e-12)
    assert torch.equal(st["td_abs"], (q_a - target).abs())
    for k in STAT_KEYS[1:]:
        assert torch.equal(st[k], st_plain[k]), k
    ones, _ = dqn_loss_reference(*args, weights=torch.ones_like(w))
    assert ones.item() == pytest.approx(plain.item(), rel=1e-14)


def _target(x, dueling, double_q, v_min=-4.0, v_max=4.0):
    from ddls_amd.rl.dqn import dueling_q
    qt = dueling_q(x["logits_nt"], x["values_nt"], dueling)
    if double_q:
        a = dueling_q(x["logits_no"], x["values_no"], dueling).argmax(-1)
        vals = qt.gather(1, a.unsqueeze(1)).squeeze(1)
    else:
        vals = qt.max(-1).values
    boot = torch.where(x["has_next"] > 0, vals, torch.zeros_like(vals))
    return torch.clamp(x["ret"] + x["disc"] * boot, v_min, v_max)


def test_config_validates_and_yaml_carries_the_keys():
    import yaml
    from ddls_amd.rl.dqn import DQNConfig
    cfg = DQNConfig()
    assert cfg.prioritized_replay is False
    assert (cfg.prioritized_replay_alpha, cfg.prioritized_replay_beta,
            cfg.prioritized_replay_eps) == (0.9, 0.1, 1e-6)
    DQNConfig(prioritized_replay_alpha=0.0, prioritized_replay_beta=0.0)
    for bad in ({"prioritized_replay_alpha": -0.1},
                {"prioritized_replay_beta": -1.0},
                {"prioritized_replay_eps": 0.0},
                {"prioritized_replay_eps": -1e-6}):
        with pytest.raises(ValueError):
            DQNConfig(**bad)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "configs", "algo", "apex_dqn.yaml")) as f:
        algo = yaml.safe_load(f)
    assert algo["prioritized_replay"] is False and algo["learner"] == "torch"
    assert algo["prioritized_replay_alpha"] == 0.9
    assert algo["prioritized_replay_beta"] == 0.1
    assert algo["prioritized_replay_eps"] == 1e-6


# ---------------------------------------------------------------------------
# CPU: trainer on the CpuEngine backend
# ---------------------------------------------------------------------------
def _cpu_engine_trainer(jobs_dir, learner):
    """tests.test_dqn_device._cpu_engine_trainer with prioritization on."""
    from ddls_amd.models.gnn import GNNPolicy
    from ddls_amd.rl.dqn import DQNConfig, DQNTrainer
    from ddls_amd.rl.engine_env import EngineVectorEnv

    dev = torch.device("cpu")
    torch.manual_seed(4)
    policy = GNNPolicy(num_actions=17)
    venv = EngineVectorEnv(
        lambda: make_env(jobs_dir, "remove_and_repeat", 2, 3000, 15),
        num_envs=4, device=dev, base_seed=19)
    cfg = DQNConfig(learning_starts=10, sgd_minibatch_size=8, lr=1e-4,
                    learner=learner, prioritized_replay=True)
    return DQNTrainer(venv, policy, cfg, device=dev)


def test_prioritized_device_learner_on_cpu_engine(multi_model_files):
    from ddls_amd.rl.dqn import PER_STAT_KEYS, STAT_KEYS
    tr = _cpu_engine_trainer(multi_model_files, "device")
    torch.manual_seed(8)
    for it in range(2):
        st = tr.update(tr.collect_rollout(8))
        tr.iteration += 1
        assert st["learner"] == 1
        assert all(np.isfinite(st[k]) for k in STAT_KEYS + PER_STAT_KEYS)
        assert st["total_loss"] > 0
        assert 0 < st["is_weight_mean"] <= 1
        assert st["max_priority"] >= 1
        assert st["replay"] == len(tr.replay_dev) == (it + 1) * 5 * 4
    replay = tr.replay_dev
    assert replay.prioritized and not tr.replay
    P, n = replay._tree.P, len(replay)
    leaves = replay.tree_sum[P:P + n].numpy()
    assert np.all(leaves > 0)
    assert np.count_nonzero(leaves != 1.0) > 0     # priorities were updated
    assert torch.all(replay.tree_sum[P + n:] == 0)
    _assert_is_rebuild(replay.tree_sum.numpy(), replay.tree_min.numpy(),
                       replay.capacity)


def test_prioritized_first_update_agrees_between_learners(multi_model_files):
    """Same seed, same fragment, same uniforms and the same slot rule: the
    first update's mean loss and mean Q agree to the bound of
    test_device_learner_first_update_agrees_with_torch_learner."""
    out = {}
    for learner in ("torch", "device"):
        tr = _cpu_engine_trainer(multi_model_files, learner)
        torch.manual_seed(8)
        out[learner] = tr.update(tr.collect_rollout(8))
    assert out["torch"]["learner"] == 0 and out["device"]["learner"] == 1
    assert out["torch"]["replay"] == out["device"]["replay"] == 20
    for k in ("total_loss", "q_mean", "is_weight_mean", "max_priority"):
        print(k, out["torch"][k], out["device"][k])
        assert out["device"][k] == pytest.approx(out["torch"][k], rel=1e-4), k


def test_prioritized_torch_learner_on_host_env(multi_model_files):
    """learner='device' on an env without device-resident rollouts falls
    back to the torch learner, which still prioritizes."""
    from ddls_amd.models.gnn import GNNPolicy
    from ddls_amd.rl.dqn import DQNConfig, DQNTrainer
    from ddls_amd.rl.rollout import VectorEnv

    torch.manual_seed(0)
    venv = VectorEnv([lambda i=i: make_env(multi_model_files,
                                           "remove_and_repeat", 2, 3000, 30)
                      for i in range(4)], base_seed=3)
    tr = DQNTrainer(venv, GNNPolicy(num_actions=17),
                    DQNConfig(learning_starts=10, sgd_minibatch_size=8,
                              lr=1e-4, learner="device", replay_capacity=30,
                              prioritized_replay=True),
                    device=torch.device("cpu"))
    for _ in range(2):
        st = tr.train(num_steps=8)
        assert st["learner"] == 0 and np.isfinite(st["total_loss"])
        assert 0 < st["is_weight_mean"] <= 1 and st["max_priority"] >= 1
    # 40 transitions through a 30-slot list: the tree covers exactly it
    t = tr._per_host
    assert len(tr.replay) == 30 and tr._replay_written == 40
    assert np.all(t.tree_sum[t.P:t.P + 30] > 0)
    _assert_is_rebuild(t.tree_sum, t.tree_min, 30)


# ---------------------------------------------------------------------------
# GPU: sum-tree kernels
# ---------------------------------------------------------------------------
def _ext():
    from ddls_amd import ops as hip_ops
    ext = hip_ops.get_extension(required=True)
    for name in ("per_ingest", "per_sample", "per_update",
                 "dqn_loss_fwd_weighted"):
        assert hasattr(ext, name), name
    return ext


def _download(replay):
    torch.cuda.synchronize()
    return (replay.tree_sum.cpu().numpy(), replay.tree_min.cpu().numpy(),
            replay.max_prio.cpu().numpy())


def _ulp_distance_f32(a, b):
    a = np.asarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    b = np.asarray(b, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.abs(a - b)


def _check_sample(replay, mirror_of, u):
    """per_sample against the mirror's descent on the downloaded tree."""
    ts, tm, mp = _download(replay)
    idx, w = replay.sample(torch.as_tensor(u, device=replay.device))
    torch.cuda.synchronize()
    want_idx, want_w = mirror_of(ts, tm, mp).sample(u)
    assert idx.dtype == torch.int64 and w.dtype == torch.float32
    assert torch.equal(idx.cpu(), torch.from_numpy(want_idx))
    assert int(idx.max()) < len(replay) and int(idx.min()) >= 0
    ulps = _ulp_distance_f32(w.cpu().numpy(), want_w)
    assert ulps.max() <= 1, ulps.max()
    assert float(w.max()) <= 1.0 and float(w.min()) > 0
    return idx, w


def _ingest_update_sequence(C, B, seed):
    """Device ring and mirror through the same ingests and updates.  The
    fills: a partial one (for C >= 5), one that wraps, one of count == C.
    After every call the device trees are a rebuild of their own leaves,
    max_prio equals the mirror's bits and the leaves agree to 1e-12.
    Returns (replay, worst relative leaf difference, sampled (idx, w))."""
    from ddls_amd.rl.device_replay import tree_leaves
    ext = _ext()
    dev = "cuda:0"
    replay = _prioritized_replay(C, dev)
    mirror = _tree(C)
    P = tree_leaves(C)
    rng = np.random.RandomState(seed)
    worst = 0.0
    samples = []

    def mirror_of(ts, tm, mp):
        return _tree(C, tree_sum=ts, tree_min=tm, max_prio=mp)

    def check():
        nonlocal worst
        ts, tm, mp = _download(replay)
        _assert_is_rebuild(ts, tm, C)
        assert np.array_equal(mp, mirror.max_prio), (mp, mirror.max_prio)
        got, want = ts[P:P + C], mirror.tree_sum[P:P + C]
        assert np.array_equal(got == 0, want == 0)
        assert np.array_equal(tm[P:P + C][got > 0], got[got > 0])
        assert np.all(np.isposinf(tm[P:P + C][got == 0]))
        nz = want > 0
        if nz.any():
            rel = np.abs(got[nz] - want[nz]) / want[nz]
            worst = max(worst, float(rel.max()))
            assert rel.max() <= 1e-12, rel.max()

    def ingest(start, count):
        ext.per_ingest(replay.tree_sum, replay.tree_min, replay.max_prio,
                       start, count, C, ALPHA)
        mirror.ingest(start, count)
        replay.written += count
        check()

    def update():
        n = len(replay)
        idx = rng.randint(0, n, size=B)
        td = np.exp(rng.uniform(np.log(1e-7), np.log(2000.0), size=B))
        replay.update_priorities(torch.as_tensor(idx, device=dev),
                                 torch.as_tensor(td, device=dev))
        mirror.update(idx, td)
        check()
        # a repeated slot holds its last occurrence's value
        ts = replay.tree_sum.cpu().numpy()
        last = {int(s): i for i, s in enumerate(idx)}
        if len(last) < B:
            dup = [s for s in last if (idx == s).sum() > 1]
            assert dup
            for s in dup[:8]:
                want = np.power(td[last[s]] + EPS, ALPHA)
                assert abs(ts[P + s] - want) <= 1e-12 * want
                others = [np.power(td[i] + EPS, ALPHA)
                          for i in np.nonzero(idx == s)[0][:-1]]
                assert all(abs(ts[P + s] - o) > 1e-9 * o for o in others)

    def sample():
        u = np.concatenate([U_EDGES, rng.random_sample(1000)])
        idx, w = _check_sample(replay, mirror_of, u)
        samples.append((idx.cpu(), w.cpu()))

    if C >= 5:
        ingest(0, C - 2)              # a ring that is only partly filled
        update()
        sample()
        ingest(C - 2, 2)
    else:
        ingest(0, C)
    update()
    ingest(C // 2, C - C // 2 + C // 3)   # wraps (C >= 3); count < C or == 1
    update()
    sample()
    ingest(C // 3, C)                 # count == C from a start inside
    update()
    sample()
    return replay, worst, samples


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 64, 300])
@pytest.mark.parametrize("C", CAPACITIES)
def test_per_kernels_against_the_mirror(C, B):
    """per_ingest / per_update / per_sample.  B = 300 is past one block
    pass; (C, B) = (5, 64) forces duplicate slots with different td_abs."""
    replay, worst, samples = _ingest_update_sequence(C, B, seed=100 * C + B)
    print(f"C={C} B={B}: worst relative leaf difference {worst:.3e}")
    assert len(replay) == C and len(samples) >= 2


@pytest.mark.gpu
def test_per_sequence_is_reproducible():
    """The same ingest -> sample -> update sequence twice: trees, indices
    and weights have the same bits."""
    a, _, sa = _ingest_update_sequence(37, 300, seed=11)
    b, _, sb = _ingest_update_sequence(37, 300, seed=11)
    torch.cuda.synchronize()
    assert torch.equal(a.tree_sum, b.tree_sum)
    assert torch.equal(a.tree_min, b.tree_min)
    assert torch.equal(a.max_prio, b.max_prio)
    for (ia, wa), (ib, wb) in zip(sa, sb):
        assert torch.equal(ia, ib) and torch.equal(wa, wb)


@pytest.mark.gpu
def test_per_bindings_check_their_arguments():
    ext = _ext()
    r = _prioritized_replay(5, "cuda:0")
    args = (r.tree_sum, r.tree_min, r.max_prio)
    with pytest.raises(RuntimeError, match="B <= 4096"):
        ext.per_update(*args, torch.zeros(4097, dtype=torch.int64,
                                          device="cuda:0"),
                       torch.zeros(4097, dtype=torch.float64,
                                   device="cuda:0"), 5, ALPHA, EPS)
    with pytest.raises(RuntimeError, match="tree_sum"):
        ext.per_ingest(*args, 0, 5, 9, ALPHA)      # P would be 16
    with pytest.raises(RuntimeError, match="count"):
        ext.per_ingest(*args, 0, 6, 5, ALPHA)
    with pytest.raises(RuntimeError, match="f64"):
        ext.per_sample(r.tree_sum, r.tree_min,
                       torch.zeros(3, device="cuda:0"), 5, BETA)


# ---------------------------------------------------------------------------
# GPU: weighted loss
# ---------------------------------------------------------------------------
def _weights(R, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.rand(R, generator=g) * 0.95 + 0.05    # (0, 1]


def _reference_weighted(inp, w, v_min, v_max, dueling, double_q, dtype):
    from ddls_amd.rl.dqn import STAT_KEYS, dqn_loss_reference
    x = _leaves(inp, dtype)
    loss, st = dqn_loss_reference(*x, v_min, v_max, dueling, double_q,
                                  weights=w.to(dtype))
    loss.backward()
    return (loss.detach(), torch.stack([st[k] for k in STAT_KEYS]),
            [t.grad for t in x[:6]]), st["td_abs"]


def _fused_weighted(inp, w, v_min, v_max, dueling, double_q):
    from ddls_amd.rl.dqn import _DQNWeightedLossFn
    x = _leaves(inp, torch.float32)
    loss, stats, td_abs = _DQNWeightedLossFn.apply(
        *x, v_min, v_max, dueling, double_q, w)
    loss.backward()
    torch.cuda.synchronize()
    return (loss.detach(), stats, [t.grad for t in x[:6]]), td_abs


@pytest.mark.gpu
@pytest.mark.parametrize("dueling,double_q", COMBOS)
@pytest.mark.parametrize("B,A", [(1, 3), (70, 17), (300, 64)])
def test_weighted_loss_matches_reference(B, A, dueling, double_q):
    from tests.test_dqn_device import _fused
    _ext()
    v_min, v_max = -4.0, 4.0
    inp = _to(_loss_inputs(B, A, seed=7 * B + A), "cuda:0")
    w = _weights(B + 1, seed=B).to("cuda:0")
    truth, td_truth = _reference_weighted(inp, w, v_min, v_max, dueling,
                                          double_q, torch.float64)
    ref32, _ = _reference_weighted(inp, w, v_min, v_max, dueling, double_q,
                                   torch.float32)
    fused, td_abs = _fused_weighted(inp, w, v_min, v_max, dueling, double_q)
    assert torch.isfinite(fused[0]) and torch.isfinite(fused[1]).all()
    _hold_to_float64_bound(truth, ref32, fused)
    assert td_abs.dtype == torch.float64 and td_abs.shape == (B + 1,)
    err = (td_abs - td_truth).abs().max().item()
    bound = 4 * EPS32 * td_truth.abs().max().item()
    print(f"td_abs: max|truth| {td_truth.abs().max().item():.6g} err "
          f"{err:.3e} bound {bound:.3e}")
    assert err <= bound
    # all-ones weights: the unweighted kernel's bits
    plain = _fused(inp, v_min, v_max, dueling, double_q)
    ones, td_ones = _fused_weighted(inp, torch.ones_like(w), v_min, v_max,
                                    dueling, double_q)
    assert torch.equal(ones[0], plain[0]) and torch.equal(ones[1], plain[1])
    assert torch.equal(ones[2][0], plain[2][0])
    assert torch.equal(ones[2][1], plain[2][1])
    assert torch.equal(td_ones, td_abs)


# ---------------------------------------------------------------------------
# GPU: trainer
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_prioritized_device_learner_on_engine_env(multi_model_files):
    from ddls_amd.models.gnn import GNNPolicy
    from ddls_amd.rl.device_replay import tree_leaves
    from ddls_amd.rl.dqn import (PER_STAT_KEYS, STAT_KEYS, DQNConfig,
                                 DQNTrainer)
    from ddls_amd.rl.engine_env import EngineVectorEnv
    from tests.test_dqn_device import _host_columns

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    venv = EngineVectorEnv(
        lambda: make_env(multi_model_files, "remove_and_repeat", 2, 3000, 15),
        num_envs=16, device=dev, base_seed=23)
    cfg = DQNConfig(learning_starts=50, sgd_minibatch_size=32,
                    num_sgd_iter=2, lr=1e-4, learner="device",
                    prioritized_replay=True)
    tr = DQNTrainer(venv, GNNPolicy(num_actions=17).to(dev), cfg, device=dev)
    host = _host_ingester(n_step=cfg.n_step, gamma=cfg.gamma)
    for _ in range(2):
        data = tr.collect_rollout(8)
        st = tr.update(data)
        tr.iteration += 1
        assert st["learner"] == 1
        assert all(np.isfinite(st[k]) for k in STAT_KEYS + PER_STAT_KEYS)
        assert 0 < st["is_weight_mean"] <= 1 and st["max_priority"] >= 1
        host._ingest({"obs": list(range(8 * 16)), "rewards": data["rewards"],
                      "dones": data["dones"], "actions": data["actions"]})
    replay = tr.replay_dev
    n = len(replay)
    assert replay.written == n == 160 and st["total_loss"] > 0
    ts, tm, mp = _download(replay)
    assert mp[0] == st["max_priority"]
    _assert_is_rebuild(ts, tm, cfg.replay_capacity)
    P = tree_leaves(cfg.replay_capacity)
    assert np.all(ts[P:P + n] > 0) and np.all(ts[P + n:] == 0)
    assert np.count_nonzero(ts[P:P + n] != 1.0) > 0
    ret, disc, has_next = _host_columns(host.replay)
    assert np.array_equal(replay.ret[:n].cpu().numpy(), ret)
    assert np.array_equal(replay.disc[:n].cpu().numpy(), disc)
    assert np.array_equal(replay.has_next[:n].cpu().numpy() != 0, has_next)
    assert torch.equal(replay.action[:n].cpu(),
                       torch.as_tensor([b[1] for b in host.replay]))
