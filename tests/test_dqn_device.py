"""Device DQN learner (rl/dqn.py ``learner="device"``), the device replay
ring (rl/device_replay.py) and the n-step ingest / fused TD-loss kernels
(ops/hip/dqn_loss.hip)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.test_vec_engine import make_env, multi_model_files  # noqa: F401

EPS32 = float(np.finfo(np.float32).eps)
FMIN = torch.finfo(torch.float32).min
GAMMA = 0.999
COMBOS = [(True, True), (True, False), (False, True), (False, False)]


# ---------------------------------------------------------------------------
# helpers: fragments and the host list buffer
# ---------------------------------------------------------------------------
def _host_ingester(capacity=200_000, n_step=3, gamma=GAMMA):
    """A DQNTrainer shell that can only run the host ``_ingest``: that method
    reads the config and the list buffer and nothing else, so no env or
    policy is built for it."""
    from ddls_amd.rl.dqn import DQNConfig, DQNTrainer
    tr = object.__new__(DQNTrainer)
    tr.config = DQNConfig(n_step=n_step, gamma=gamma,
                          replay_capacity=capacity)
    tr.replay = []
    tr._replay_ptr = 0
    return tr


def _fragment(T, N, n, A=17, seed=0, row0=0):
    """A [T, N] rollout fragment in both forms: the flat ``*_dev`` tensors
    (CPU) the device learner reads and the host arrays ``_ingest`` reads.
    ``obs`` holds global row numbers starting at ``row0`` instead of
    CompactObs, so a host buffer entry names the rows it came from.  Dones
    fall with p = 0.15, plus one in the first row, one in row T-n-1 (the last
    row that starts a transition) and a column that is all done."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    R = T * N
    gfull = torch.randn(R, 17 + A, generator=g)
    rewards = torch.randn(T, N, generator=g) * 3
    dones = torch.rand(T, N, generator=g) < 0.15
    dones[0, 1 % N] = True
    if T - n - 1 >= 0:
        dones[T - n - 1, 2 % N] = True
    if N > 3:
        dones[:, 3] = True
    actions = torch.randint(0, A, (T, N), generator=g)
    return {
        "gfull_dev": gfull,
        "model_ids_dev": torch.randint(0, 3, (R,), generator=g),
        "actions_dev": actions.reshape(R).clone(),
        "rewards_dev": rewards.reshape(R).clone(),
        "dones_dev": dones.reshape(R).float(),
        "rewards": rewards.numpy(),
        "dones": dones.numpy(),
        "actions": actions.numpy(),
        "obs": list(range(row0, row0 + R)),
    }


def _to(data, dev):
    return {k: (v.to(dev) if torch.is_tensor(v) else v)
            for k, v in data.items()}


def _host_columns(buf):
    """(ret, disc, has_next) of a host buffer after update()'s cast to f32."""
    ret = np.array([b[2] for b in buf], dtype=np.float32)
    disc = np.array([b[4] for b in buf], dtype=np.float32)
    has_next = np.array([b[3] is not None for b in buf])
    return ret, disc, has_next


def _assert_ring_is_host_buffer(replay, host, gfull_all):
    """Every slot of the ring against the host list's entry at that index."""
    buf = host.replay
    assert len(replay) == len(buf)
    n = len(buf)
    ret, disc, has_next = _host_columns(buf)
    s_rows = torch.as_tensor([b[0] for b in buf])
    assert torch.equal(replay.action[:n],
                       torch.as_tensor([b[1] for b in buf]))
    assert np.array_equal(replay.ret[:n].numpy(), ret)
    assert np.array_equal(replay.disc[:n].numpy(), disc)
    assert np.array_equal(replay.has_next[:n].numpy() != 0, has_next)
    assert torch.equal(replay.s_gfull[:n], gfull_all[s_rows])
    n_rows = torch.as_tensor([b[3] if b[3] is not None else b[0]
                              for b in buf])
    hn = torch.as_tensor(has_next)
    assert torch.equal(replay.n_gfull[:n][hn], gfull_all[n_rows][hn])
    # a cut transition carries a copy of its own state
    assert torch.equal(replay.n_gfull[:n][~hn], gfull_all[s_rows][~hn])


# ---------------------------------------------------------------------------
# helpers: loss inputs and the three evaluations
# ---------------------------------------------------------------------------
def _top_two_gap(logits_no, values_no):
    """Gap between the best and the second-best online next-state Q, in
    float64.  A constant per-row shift does not change it, so the dueling Q
    serves both settings."""
    from ddls_amd.rl.dqn import dueling_q
    q = dueling_q(logits_no.double(), values_no.double(), True)
    if q.shape[1] == 1:
        return torch.full((q.shape[0],), float("inf"), dtype=torch.float64)
    top = q.topk(2, dim=-1).values
    return top[:, 0] - top[:, 1]


def _loss_inputs(B, A, seed):
    """B rows at the scales the issue sets, plus one extra row with
    has_next = 0 whose next state is entirely masked (B + 1 rows).  The
    double-Q argmax is discontinuous, so every regular row whose top-two gap
    of the online next-state Q is below 1e-3 has its top valid logit raised
    by 0.01, which widens the gap by exactly that; the extra row's argmax is
    never used."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    R = B + 1
    actions = torch.randint(0, A, (R,), generator=g)
    rows = torch.arange(R)

    def logits(mask):
        x = torch.randn(R, A, generator=g) * 2
        x[mask] = FMIN
        return x

    mask_s = torch.rand(R, A, generator=g) < 0.2
    mask_s[rows, actions] = False
    mask_n = torch.rand(R, A, generator=g) < 0.2
    mask_n[rows, torch.randint(0, A, (R,), generator=g)] = False
    logits_s, logits_no, logits_nt = (logits(mask_s), logits(mask_n),
                                      logits(mask_n))
    values_s, values_no, values_nt = (torch.randn(R, generator=g) * 5
                                      for _ in range(3))
    ret = torch.randn(R, generator=g) * 3
    disc = torch.tensor([GAMMA, GAMMA ** 2, GAMMA ** 3])[
        torch.randint(0, 3, (R,), generator=g)]
    has_next = (torch.rand(R, generator=g) >= 0.2).float()
    # the extra row
    logits_no[B] = FMIN
    logits_nt[B] = FMIN
    has_next[B] = 0.0

    gap = _top_two_gap(logits_no[:B], values_no[:B])
    close = torch.nonzero(gap < 1e-3).flatten()
    if len(close):
        q = torch.where(mask_n[close], torch.full((), float("-inf")),
                        logits_no[close])
        logits_no[close, q.argmax(-1)] += 0.01
    gap = _top_two_gap(logits_no[:B], values_no[:B])
    assert (gap > 1e-3).all(), gap.min().item()
    return dict(logits_s=logits_s, values_s=values_s, logits_no=logits_no,
                values_no=values_no, logits_nt=logits_nt,
                values_nt=values_nt, actions=actions, ret=ret, disc=disc,
                has_next=has_next)


ORDER = ("logits_s", "values_s", "logits_no", "values_no", "logits_nt",
         "values_nt", "actions", "ret", "disc", "has_next")
GRAD_IN = ORDER[:6]


def _leaves(inp, dtype):
    out = []
    for k in ORDER:
        v = inp[k]
        if v.is_floating_point():
            v = v.to(dtype)
        if k in GRAD_IN:
            v = v.clone().requires_grad_(True)
        out.append(v)
    return out


def _reference(inp, v_min, v_max, dueling, double_q, dtype=torch.float32):
    """dqn_loss_reference + autograd -> (loss, stats[4], grads of the six
    network outputs, None where there is none), all in ``dtype``."""
    from ddls_amd.rl.dqn import STAT_KEYS, dqn_loss_reference
    x = _leaves(inp, dtype)
    loss, st = dqn_loss_reference(*x, v_min, v_max, dueling, double_q)
    loss.backward()
    return (loss.detach(), torch.stack([st[k] for k in STAT_KEYS]),
            [t.grad for t in x[:6]])


def _fused(inp, v_min, v_max, dueling, double_q):
    from ddls_amd.rl.dqn import _DQNLossFn
    x = _leaves(inp, torch.float32)
    loss, stats = _DQNLossFn.apply(*x, v_min, v_max, dueling, double_q)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach(), stats, [t.grad for t in x[:6]]


def _hold_to_float64_bound(truth, ref32, fused):
    """The project's bound (test_device_learner_on_engine_env): the fused
    error against the float64 truth may be at most 4x the float32 torch
    reference's own error plus 4 * eps_f32 * max|truth|."""
    from ddls_amd.rl.dqn import STAT_KEYS
    names = ["loss"] + ["stat " + k for k in STAT_KEYS] \
        + ["glogits_s", "gvalues_s"]

    def split(r):
        return [r[0]] + list(r[1]) + [r[2][0], r[2][1]]

    failures = []
    for name, t, r, f in zip(names, split(truth), split(ref32), split(fused)):
        if t is None:
            # no dueling: the value head takes no gradient
            assert r is None
            assert f is None or torch.count_nonzero(f) == 0, name
            continue
        t = t.cpu()
        e_ref = (r.double().cpu() - t).abs().max().item()
        e_fused = (f.double().cpu() - t).abs().max().item()
        bound = 4 * e_ref + 4 * EPS32 * t.abs().max().item()
        print(f"{name}: max|truth| {t.abs().max().item():.6g} fused err "
              f"{e_fused:.3e} torch f32 err {e_ref:.3e} bound {bound:.3e} "
              f"ratio {e_fused / max(e_ref, 1e-300):.2f}")
        if not e_fused <= bound:
            failures.append(name)
    assert not failures, failures


def _branches(inp, v_min, v_max, dueling, double_q):
    """Which clamps and Huber branches the float64 truth takes."""
    from ddls_amd.rl.dqn import dueling_q
    x = {k: (v.double() if v.is_floating_point() else v)
         for k, v in inp.items()}
    qt = dueling_q(x["logits_nt"], x["values_nt"], dueling)
    if double_q:
        a = dueling_q(x["logits_no"], x["values_no"], dueling).argmax(-1)
        vals = qt.gather(1, a.unsqueeze(1)).squeeze(1)
    else:
        vals = qt.max(-1).values
    raw = x["ret"] + x["disc"] * torch.where(x["has_next"] > 0, vals,
                                             torch.zeros_like(vals))
    q_a = dueling_q(x["logits_s"], x["values_s"], dueling).gather(
        1, x["actions"].unsqueeze(1)).squeeze(1)
    td = q_a - raw.clamp(v_min, v_max)
    return {"clamp_lo": bool((raw < v_min).any()),
            "clamp_hi": bool((raw > v_max).any()),
            "huber_quadratic": bool((td.abs() < 1).any()),
            "huber_linear": bool((td.abs() > 1).any())}


LOSS_SHAPES = [(1, 3), (5, 17), (70, 17), (300, 64), (4100, 17)]


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
def test_learner_value_is_checked(multi_model_files):
    from ddls_amd.models.gnn import GNNPolicy
    from ddls_amd.rl.dqn import DQNConfig, DQNTrainer
    from ddls_amd.rl.rollout import VectorEnv

    assert DQNConfig().learner == "torch"
    venv = VectorEnv([lambda: make_env(multi_model_files,
                                       "remove_and_repeat", 2, 3000, 30)],
                     base_seed=3)
    with pytest.raises(ValueError):
        DQNTrainer(venv, GNNPolicy(num_actions=17),
                   DQNConfig(learner="bogus"), device=torch.device("cpu"))


def test_config_group_carries_learner():
    import yaml
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "configs", "algo", "apex_dqn.yaml")) as f:
        assert yaml.safe_load(f)["learner"] == "torch"


def test_nstep_reference_on_the_transition_cut_case():
    """The case of test_dqn_nstep_transition_cuts."""
    from ddls_amd.rl.dqn import nstep_transitions_reference
    T, N = 7, 1
    rewards = np.ones((T, N))
    dones = np.zeros((T, N), dtype=bool)
    dones[2][0] = True
    host = _host_ingester(n_step=3, gamma=0.5)
    host._ingest({"obs": list(range(T * N)), "rewards": rewards,
                  "dones": dones, "actions": np.zeros((T, N), np.int64)})
    ret, disc, has_next, steps = nstep_transitions_reference(
        rewards, dones, 3, 0.5)
    h_ret, h_disc, h_next = _host_columns(host.replay)
    assert ret.dtype == np.float32 and disc.dtype == np.float32
    assert np.array_equal(ret.reshape(-1), h_ret)
    assert np.array_equal(disc.reshape(-1), h_disc)
    assert np.array_equal(has_next.reshape(-1), h_next)
    assert ret[0, 0] == 1.75 and not has_next[0, 0]
    assert ret[3, 0] == 1.75 and has_next[3, 0] and disc[3, 0] == 0.125
    assert steps.reshape(-1).tolist() == [3, 2, 1, 3]


@pytest.mark.parametrize("T,N,n", [(9, 3, 3), (13, 5, 1), (6, 30, 5),
                                   (12, 7, 4)])
def test_nstep_reference_equals_host_ingest(T, N, n):
    """Random f32 rewards, gamma = 0.999 (not an f32): the explicit-cast
    reference equals the host loop's stored values bit for bit.  The host
    loop multiplies a Python float by an np.float32, which is an f32 product
    under NEP 50 (numpy >= 2); the reference spells the casts out."""
    from ddls_amd.rl.dqn import nstep_transitions_reference
    data = _fragment(T, N, n, seed=10 * T + N)
    assert data["rewards"].dtype == np.float32
    assert data["dones"][0].any() and data["dones"][T - n - 1].any()
    assert N <= 3 or data["dones"][:, 3].all()
    host = _host_ingester(n_step=n)
    host._ingest(data)
    ret, disc, has_next, steps = nstep_transitions_reference(
        data["rewards"], data["dones"], n, GAMMA)
    h_ret, h_disc, h_next = _host_columns(host.replay)
    assert len(h_ret) == (T - n) * N
    assert np.array_equal(ret.reshape(-1), h_ret)
    assert np.array_equal(disc.reshape(-1), h_disc)
    assert np.array_equal(has_next.reshape(-1), h_next)
    # the next state the host stored is row (t + steps) * N + b
    k = np.arange((T - n) * N)
    want = [b[3] for b in host.replay]
    got = k + steps.reshape(-1) * N
    assert all(w is None or w == g_ for w, g_ in zip(want, got))
    assert h_next.any() and not h_next.all()


def test_nstep_reference_short_fragment_is_empty():
    from ddls_amd.rl.dqn import nstep_transitions_reference
    out = nstep_transitions_reference(np.ones((3, 2), np.float32),
                                      np.zeros((3, 2), bool), 3, GAMMA)
    assert all(o.shape == (0, 2) for o in out)


@pytest.mark.parametrize("C,fragments", [(37, 2), (37, 3), (5, 1), (5, 2)])
def test_device_replay_on_cpu_is_the_host_list(C, fragments):
    """(9, 3, 3) fragments of 18 transitions each.  C = 37 holds two of them
    and wraps inside the third; C = 5 holds less than one fragment yields.
    After every fragment each slot equals the host list's entry."""
    from ddls_amd.rl.device_replay import DeviceReplay
    T, N, n, A = 9, 3, 3, 17
    replay = DeviceReplay(C, 17 + A, "cpu")
    host = _host_ingester(capacity=C, n_step=n)
    gfull_all = []
    for i in range(fragments):
        data = _fragment(T, N, n, A=A, seed=40 + i, row0=i * T * N)
        gfull_all.append(data["gfull_dev"])
        assert replay.ingest(data, n, GAMMA) == (T - n) * N
        host._ingest(data)
        assert replay.written == (i + 1) * (T - n) * N
        assert len(replay) == min(replay.written, C)
        _assert_ring_is_host_buffer(replay, host, torch.cat(gfull_all))
    mb = replay.gather(torch.tensor([0, len(replay) - 1, 0]))
    assert mb["s_gfull"].shape == (3, 17 + A)
    assert torch.equal(mb["ret"], replay.ret[[0, len(replay) - 1, 0]])


def test_device_replay_wraps_inside_a_fragment():
    """C = 37 and two (9, 3, 3) fragments after one of 27 transitions: the
    first (9, 3, 3) fragment starts at slot 27 and crosses slot 36 -> 0."""
    from ddls_amd.rl.device_replay import DeviceReplay
    A, n, C = 17, 3, 37
    replay = DeviceReplay(C, 17 + A, "cpu")
    host = _host_ingester(capacity=C, n_step=n)
    gfull_all, row0 = [], 0
    for i, (T, N) in enumerate([(12, 3), (9, 3), (9, 3)]):
        data = _fragment(T, N, n, A=A, seed=60 + i, row0=row0)
        row0 += T * N
        gfull_all.append(data["gfull_dev"])
        replay.ingest(data, n, GAMMA)
        host._ingest(data)
        _assert_ring_is_host_buffer(replay, host, torch.cat(gfull_all))
    assert replay.written == 27 + 18 + 18 and len(replay) == C


@pytest.mark.parametrize("dueling,double_q", COMBOS)
def test_loss_reference_matches_update_expressions(dueling, double_q):
    """dqn_loss_reference in float64 against DQNTrainer.update()'s own
    expressions (compacted has_next rows, boot scattered back)."""
    from ddls_amd.rl.dqn import dqn_loss_reference
    inp = _loss_inputs(40, 17, seed=5)
    x = {k: (v.double() if v.is_floating_point() else v)
         for k, v in inp.items()}
    v_min, v_max = -4.0, 4.0

    def q_values(logits, values):
        if dueling:
            valid = logits > -1e30
            adv = torch.where(valid, logits, torch.zeros_like(logits))
            mean_adv = adv.sum(-1) / valid.sum(-1).clamp(min=1)
            q = values.unsqueeze(-1) + logits - mean_adv.unsqueeze(-1)
            return torch.where(valid, q, logits)
        return logits

    has_next = x["has_next"] > 0
    boot = torch.zeros(len(has_next), dtype=torch.float64)
    q_next_t = q_values(x["logits_nt"][has_next], x["values_nt"][has_next])
    if double_q:
        q_next_o = q_values(x["logits_no"][has_next],
                            x["values_no"][has_next])
        a_star = q_next_o.argmax(-1)
        vals = q_next_t.gather(1, a_star.unsqueeze(1)).squeeze(1)
    else:
        vals = q_next_t.max(-1).values
    boot[has_next] = vals
    target = torch.clamp(x["ret"] + x["disc"] * boot, v_min, v_max)
    q = q_values(x["logits_s"], x["values_s"])
    q_a = q.gather(1, x["actions"].unsqueeze(1)).squeeze(1)
    want = {"total_loss": F.smooth_l1_loss(q_a, target).item(),
            "q_mean": q_a.mean().item(),
            "td_abs_mean": (q_a - target).abs().mean().item(),
            "target_mean": target.mean().item()}

    loss, st = dqn_loss_reference(*[x[k] for k in ORDER], v_min, v_max,
                                  dueling, double_q)
    assert loss.item() == pytest.approx(want["total_loss"], rel=1e-10)
    for key, w in want.items():
        assert st[key].item() == pytest.approx(w, rel=1e-10), key


@pytest.mark.parametrize("B,A", LOSS_SHAPES)
def test_loss_inputs_are_unambiguous_and_cover_the_branches(B, A):
    """The seeds the GPU test uses: the argmax condition holds (asserted in
    the builder), and from 70 rows up both clamps and both Huber branches
    occur for every (dueling, double_q)."""
    inp = _loss_inputs(B, A, seed=7 * B + A)
    assert inp["logits_s"].shape == (B + 1, A)
    masked = inp["logits_s"] == FMIN
    assert not masked[torch.arange(B + 1), inp["actions"]].any()
    assert not (inp["logits_no"][:B] == FMIN).all(-1).any()
    assert (inp["logits_no"][B] == FMIN).all() and inp["has_next"][B] == 0
    for dueling, double_q in COMBOS:
        br = _branches(inp, -4.0, 4.0, dueling, double_q)
        if B >= 70:
            assert all(br.values()), (dueling, double_q, br)


def _cpu_engine_trainer(jobs_dir, learner):
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
                    learner=learner)
    return DQNTrainer(venv, policy, cfg, device=dev)


def test_device_learner_on_cpu_engine(multi_model_files):
    tr = _cpu_engine_trainer(multi_model_files, "device")
    before = {k: v.clone() for k, v in tr.policy.state_dict().items()}
    torch.manual_seed(8)
    for it in range(2):
        data = tr.collect_rollout(8)
        st = tr.update(data)
        tr.iteration += 1
        assert st["learner"] == 1
        assert all(np.isfinite(st[k]) for k in
                   ("total_loss", "q_mean", "td_abs_mean", "target_mean"))
        assert st["total_loss"] > 0
        assert data["obs"]._items is None
        assert st["replay"] == len(tr.replay_dev) == (it + 1) * 5 * 4
    assert not tr.replay          # the host list was never filled
    assert any(not torch.equal(before[k], v)
               for k, v in tr.policy.state_dict().items())


def test_device_learner_first_update_agrees_with_torch_learner(
        multi_model_files):
    """Same seed: both learners collect the same fragment, build the same
    transitions and draw the same minibatches, so the first update's mean
    loss and mean Q agree to float32 rounding (1e-4 relative leaves three
    decimal digits over eps for the different batching of the forwards)."""
    out = {}
    for learner in ("torch", "device"):
        tr = _cpu_engine_trainer(multi_model_files, learner)
        torch.manual_seed(8)
        data = tr.collect_rollout(8)
        out[learner] = tr.update(data)
    assert out["torch"]["learner"] == 0 and out["device"]["learner"] == 1
    assert out["torch"]["replay"] == out["device"]["replay"] == 20
    for k in ("total_loss", "q_mean"):
        assert out["device"][k] == pytest.approx(out["torch"][k], rel=1e-4), k


def test_device_learner_falls_back_on_host_env(multi_model_files, capsys):
    """An env without supports_device_resident: one warning, torch path."""
    from ddls_amd.models.gnn import GNNPolicy
    from ddls_amd.rl.dqn import DQNConfig, DQNTrainer
    from ddls_amd.rl.rollout import VectorEnv

    torch.manual_seed(0)
    venv = VectorEnv([lambda i=i: make_env(multi_model_files,
                                           "remove_and_repeat", 2, 3000, 30)
                      for i in range(4)], base_seed=3)
    tr = DQNTrainer(venv, GNNPolicy(num_actions=17),
                    DQNConfig(learning_starts=10, sgd_minibatch_size=8,
                              lr=1e-4, learner="device"),
                    device=torch.device("cpu"))
    for _ in range(2):
        st = tr.train(num_steps=8)
        assert np.isfinite(st["total_loss"]) and st["learner"] == 0
    assert capsys.readouterr().err.count("learner='device'") == 1
    assert tr.replay_dev is None and len(tr.replay) == 40


# ---------------------------------------------------------------------------
# GPU: kernels
# ---------------------------------------------------------------------------
def _ext():
    from ddls_amd import ops as hip_ops
    ext = hip_ops.get_extension(required=True)
    assert hasattr(ext, "dqn_nstep_ingest") and hasattr(ext, "dqn_loss_fwd")
    return ext


@pytest.mark.gpu
@pytest.mark.parametrize("ring", ["large", "wrap37", "small"])
@pytest.mark.parametrize("T,N,n", [(4, 1, 3), (3, 2, 3), (7, 1, 3),
                                   (13, 5, 1), (9, 70, 3), (6, 300, 5)])
def test_nstep_ingest_bits(T, N, n, ring):
    """dqn_nstep_ingest against the CPU DeviceReplay fed the same two
    fragments: all eight ring tensors are torch.equal.  ``wrap37`` wraps a
    C = 37 ring, ``small`` holds less than one fragment yields."""
    from ddls_amd.rl.device_replay import RING_KEYS, DeviceReplay
    _ext()
    A = 17
    K = max((T - n) * N, 0)
    C = {"large": 4096, "wrap37": 37, "small": max(1, K // 3)}[ring]
    cpu = DeviceReplay(C, 17 + A, "cpu")
    gpu = DeviceReplay(C, 17 + A, "cuda:0")
    for i in range(2):
        data = _fragment(T, N, n, A=A, seed=1000 * i + 10 * T + N)
        assert cpu.ingest(data, n, GAMMA) == K
        assert gpu.ingest(_to(data, "cuda:0"), n, GAMMA) == K
        torch.cuda.synchronize()
        assert gpu.written == cpu.written == (i + 1) * K
        assert len(gpu) == min(gpu.written, C)
        for key in RING_KEYS:
            assert torch.equal(getattr(gpu, key).cpu(), getattr(cpu, key)), \
                (key, i)
    if K == 0:
        # nothing launched, nothing touched
        assert all(torch.count_nonzero(getattr(gpu, k)) == 0
                   for k in RING_KEYS)


@pytest.mark.gpu
@pytest.mark.parametrize("dueling,double_q", COMBOS)
@pytest.mark.parametrize("B,A", LOSS_SHAPES)
def test_fused_dqn_loss_matches_reference(B, A, dueling, double_q):
    """dqn_loss_fwd / dqn_loss_bwd against the float64 dqn_loss_reference,
    held to the float32 reference's own error; (4100, 17) is past the
    1024-block grid cap, so the grid-stride loop runs."""
    _ext()
    v_min, v_max = -4.0, 4.0
    cpu = _loss_inputs(B, A, seed=7 * B + A)
    if B >= 70:
        assert all(_branches(cpu, v_min, v_max, dueling, double_q).values())
    inp = _to(cpu, "cuda:0")
    truth = _reference(inp, v_min, v_max, dueling, double_q, torch.float64)
    ref32 = _reference(inp, v_min, v_max, dueling, double_q, torch.float32)
    fused = _fused(inp, v_min, v_max, dueling, double_q)
    assert torch.isfinite(fused[0]) and torch.isfinite(fused[1]).all()
    gl, gv = fused[2][0], fused[2][1]
    assert torch.isfinite(gl).all() and torch.isfinite(gv).all()
    _hold_to_float64_bound(truth, ref32, fused)
    # masked lanes and every next-state input: exactly zero or None
    assert torch.count_nonzero(gl[inp["logits_s"] == FMIN]) == 0
    assert torch.count_nonzero(gl) > 0
    for g in fused[2][2:]:
        assert g is None or torch.count_nonzero(g) == 0
    # the extra row (has_next = 0, next state all masked) stays finite
    assert torch.isfinite(gl[B]).all() and torch.isfinite(gv[B])


@pytest.mark.gpu
def test_fused_dqn_loss_is_reproducible():
    """No float atomics: two calls on the same inputs give the same bits."""
    _ext()
    inp = _to(_loss_inputs(300, 17, seed=3), "cuda:0")
    a = _fused(inp, -4.0, 4.0, True, True)
    b = _fused(inp, -4.0, 4.0, True, True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(a[2][0], b[2][0]) and torch.equal(a[2][1], b[2][1])


@pytest.mark.gpu
def test_fused_dqn_loss_rejects_wide_rows():
    ext = _ext()
    inp = _to(_loss_inputs(5, 65, seed=1), "cuda:0")
    with pytest.raises(RuntimeError, match="A <= 64"):
        ext.dqn_loss_fwd(*[inp[k] for k in ORDER], -4.0, 4.0, True, True)


# ---------------------------------------------------------------------------
# GPU: trainer
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_device_learner_on_engine_env(multi_model_files):
    """Two device-learner iterations on the GPU engine: the ring against the
    host _ingest fed the same rewards / dones, then the kernels against a
    float64 truth on one ring minibatch at the environment's reward scale."""
    from ddls_amd.models.gnn import GNNPolicy, graph_mean
    from ddls_amd.rl.dqn import STAT_KEYS, DQNConfig, DQNTrainer
    from ddls_amd.rl.engine_env import EngineVectorEnv

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    venv = EngineVectorEnv(
        lambda: make_env(multi_model_files, "remove_and_repeat", 2, 3000, 15),
        num_envs=16, device=dev, base_seed=23)
    cfg = DQNConfig(learning_starts=50, sgd_minibatch_size=32,
                    num_sgd_iter=2, lr=1e-4, learner="device")
    tr = DQNTrainer(venv, GNNPolicy(num_actions=17).to(dev), cfg, device=dev)
    host = _host_ingester(n_step=cfg.n_step, gamma=cfg.gamma)
    for _ in range(2):
        data = tr.collect_rollout(8)
        st = tr.update(data)
        tr.iteration += 1
        assert st["learner"] == 1
        assert all(np.isfinite(st[k]) for k in STAT_KEYS)
        assert data["obs"]._items is None
        host._ingest({"obs": list(range(8 * 16)), "rewards": data["rewards"],
                      "dones": data["dones"], "actions": data["actions"]})
    replay = tr.replay_dev
    assert replay.written == 2 * 5 * 16
    assert len(replay) == min(replay.written, cfg.replay_capacity) == 160
    assert st["replay"] == 160 and st["total_loss"] > 0
    n = len(replay)
    ret, disc, has_next = _host_columns(host.replay)
    assert np.array_equal(replay.ret[:n].cpu().numpy(), ret)
    assert np.array_equal(replay.disc[:n].cpu().numpy(), disc)
    assert np.array_equal(replay.has_next[:n].cpu().numpy() != 0, has_next)
    assert torch.equal(replay.action[:n].cpu(),
                       torch.as_tensor([b[1] for b in host.replay]))

    g = torch.Generator(device="cpu").manual_seed(1)
    mb = replay.gather(torch.randint(0, n, (32,), generator=g).to(dev))
    with torch.no_grad():
        static = venv._models_batch
        emb_o = graph_mean(tr.policy.gnn(static), static)
        emb_t = graph_mean(tr.target.gnn(static), static)
        logits_s, values_s = tr._heads(tr.policy, emb_o, mb["s_gfull"],
                                       mb["s_model"])
        logits_no, values_no = tr._heads(tr.policy, emb_o, mb["n_gfull"],
                                         mb["n_model"])
        logits_nt, values_nt = tr._heads(tr.target, emb_t, mb["n_gfull"],
                                         mb["n_model"])
    inp = dict(logits_s=logits_s, values_s=values_s, logits_no=logits_no,
               values_no=values_no, logits_nt=logits_nt, values_nt=values_nt,
               actions=mb["action"], ret=mb["ret"], disc=mb["disc"],
               has_next=mb["has_next"])
    args = (cfg.v_min, cfg.v_max, cfg.dueling, cfg.double_q)
    truth = _reference(inp, *args, torch.float64)
    ref32 = _reference(inp, *args, torch.float32)
    fused = _fused(inp, *args)
    _hold_to_float64_bound(truth, ref32, fused)
