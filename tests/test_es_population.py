"""ES population evaluation (rl/es_population.py + ops/hip/es_population.hip).

CPU: the noise / update / actor references, tie-safe ranks, common random
numbers and the trainer on a ``CpuEngine``.  GPU: ``es_perturb``,
``actor_population`` and ``es_update`` against those references,
``actor_population`` bitwise against ``actor_batch``, ``replicate_envs``, the
evaluator in lockstep with the reference, and the trainer end to end.
"""
import copy
import functools

import numpy as np
import pytest
import torch

from ddls_amd.rl.device_actor import (MODES, act_reference, head_params,
                                      philox_uniform)
from ddls_amd.rl.es import (ESConfig, ESTrainer, centered_ranks,
                            centered_ranks_ties, count_tied_pairs)
from ddls_amd.rl.es_population import (PopulationEvaluator,
                                       act_population_reference,
                                       es_noise_reference, es_pair_weights,
                                       es_population_reference,
                                       es_update_reference,
                                       es_update_scalars, head_offsets,
                                       load_flat)
from tests.test_device_actor import (POLICY_SEED, _kernel as _actor_batch,
                                     _top_two_gap)
from tests.test_vec_engine import make_env, multi_model_files  # noqa: F401

GREEDY, SAMPLE = MODES["policy_greedy"], MODES["policy_sample"]
# (num_actions, P, E): E below one block of 4 rows, one more than a block,
# many blocks; the last case has the narrow head
POP_CASES = ((17, 4, 3), (17, 6, 5), (17, 2, 67), (5, 4, 5))
SENTINEL = -7.0


def _flat(policy):
    return torch.cat([p.detach().reshape(-1) for p in policy.parameters()])


def _policy(num_actions, seed=POLICY_SEED):
    from ddls_amd.models.gnn import GNNPolicy
    torch.manual_seed(seed)
    policy = GNNPolicy(num_actions=num_actions)
    assert policy._fused_head_ok
    return policy


@functools.lru_cache(maxsize=None)
def _pop_case(num_actions, P, E, sigma=0.1):
    """POLICY_SEED policy perturbed into P members (reference noise), a
    random embedding table per member and B = P * E observations; rows 1 of
    members 0 and 2 are done.  Cached: treat as read-only."""
    policy = _policy(num_actions)
    theta = _flat(policy).numpy()
    eps = es_noise_reference(3, 0, P // 2, theta.size)
    pop = torch.from_numpy(es_population_reference(theta, eps, sigma))
    B = P * E
    g = torch.Generator().manual_seed(7000 + 100 * P + E + num_actions)
    model_emb_pop = torch.randn(P, 3, 16, generator=g)
    obs_gf = torch.randn(B, 17, generator=g)
    mask = (torch.rand(B, num_actions, generator=g)
            < torch.rand(B, 1, generator=g)).float()
    mask[:, 0] = 1.0
    mask[2, :] = 1.0
    obs_model = torch.randint(0, 3, (B,), generator=g).int()
    done = torch.zeros(B, dtype=torch.uint8)
    for m in (0, 2):
        if m < P:
            done[m * E + 1] = 1
    inp = dict(obs_gf=obs_gf, obs_mask=mask, obs_model=obs_model,
               obs_sched=torch.zeros(B, dtype=torch.int32), done=done)
    return policy, inp, pop, model_emb_pop


@functools.lru_cache(maxsize=None)
def _pop_reference(num_actions, P, E, mode, seed=0, step=0, sigma=0.1):
    policy, inp, pop, emb = _pop_case(num_actions, P, E, sigma)
    return act_population_reference(mode, policy=copy.deepcopy(policy),
                                    pop=pop, model_emb_pop=emb, E=E,
                                    seed=seed, step=step, **inp)


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
def test_noise_reference():
    z = es_noise_reference(0, 0, 4, 2 ** 18)
    assert z.dtype == np.float32 and z.shape == (4, 2 ** 18)
    assert abs(float(z.mean(dtype=np.float64))) <= 0.01
    assert abs(float(z.var(dtype=np.float64)) - 1.0) <= 0.01
    assert np.isfinite(z).all()
    a = es_noise_reference(5, 2, 3, 64)
    assert not np.array_equal(a[0], a[1]) and not np.array_equal(a[1], a[2])
    assert not np.array_equal(a, es_noise_reference(5, 3, 3, 64))
    assert not np.array_equal(a, es_noise_reference(6, 2, 3, 64))
    # the 64-bit generation index reaches the counter's high word
    assert not np.array_equal(a, es_noise_reference(5, 2 + 2 ** 32, 3, 64))
    assert a.tobytes() == es_noise_reference(5, 2, 3, 64).tobytes()
    # n is not rounded up to the 4 elements of a Philox call
    assert es_noise_reference(5, 2, 3, 10).tobytes() == \
        np.ascontiguousarray(es_noise_reference(5, 2, 3, 12)[:, :10]).tobytes()


def test_ranks_ties():
    rng = np.random.RandomState(0)
    x = rng.permutation(32).astype(np.float64) * 0.37
    np.testing.assert_array_equal(centered_ranks_ties(x), centered_ranks(x))
    r = centered_ranks_ties(np.array([1.0, 1.0, 3.0, 2.0]))
    w = es_pair_weights(r)
    assert w.dtype == np.float32
    assert w[0] == 0.0
    np.testing.assert_allclose(r, [-1 / 3, -1 / 3, 0.5, 1 / 6])
    assert w[1] == np.float32(0.5 - 1 / 6)
    np.testing.assert_array_equal(centered_ranks_ties(np.full(6, 2.5)),
                                  np.zeros(6))
    assert count_tied_pairs(np.array([1.0, 1.0, 3.0, 2.0])) == 1


def test_update_reference_matches_trainer_formula():
    """The numpy f32 reference against the torch formula of
    ``ESTrainer.train`` (same eps, same ranks): they differ by f32
    reassociation of a 16-term sum."""
    K, n = 16, 1000
    sigma, stepsize, l2 = 0.02, 0.01, 0.005
    rng = np.random.RandomState(1)
    theta = rng.randn(n).astype(np.float32)
    eps = es_noise_reference(9, 4, K, n)
    fitness = rng.randn(2 * K)
    ranks = centered_ranks(fitness)
    np.testing.assert_array_equal(ranks, centered_ranks_ties(fitness))
    scale, decay = es_update_scalars(K, sigma, stepsize, l2)
    got = es_update_reference(theta, eps, es_pair_weights(ranks), scale, decay)
    assert got.dtype == np.float32
    # ESTrainer.train, verbatim
    th = torch.from_numpy(theta)
    grad = torch.zeros_like(th)
    for k in range(K):
        grad += float(ranks[2 * k] - ranks[2 * k + 1]) * torch.from_numpy(eps[k])
    grad /= (2 * K * sigma)
    want = th + stepsize * grad - stepsize * l2 * th
    np.testing.assert_allclose(got, want.numpy(), rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize("num_actions", [17, 5])
def test_head_offsets(num_actions):
    policy = _policy(num_actions)
    n = _flat(policy).numel()
    assert (n == 21920) or num_actions != 17
    offs = head_offsets(policy)
    assert len(offs) == 12
    g = torch.Generator().manual_seed(2)
    pop = torch.randn(3, n, generator=g)
    for m in range(3):
        scratch = copy.deepcopy(policy)
        load_flat(scratch, pop[m])
        assert torch.equal(_flat(scratch), pop[m])
        for off, p in zip(offs, head_params(scratch)):
            assert torch.equal(pop[m, off:off + p.numel()].view(p.shape), p)
    # a policy whose head is not the tail of parameters() is refused
    policy.extra = torch.nn.Linear(2, 2)
    with pytest.raises(AssertionError):
        head_offsets(policy)


def test_reference_actor_and_near_tie_cap():
    gaps = []
    for num_actions, P, E in POP_CASES:
        policy, inp, pop, emb = _pop_case(num_actions, P, E)
        out = _pop_reference(num_actions, P, E, GREEDY)
        B = P * E
        assert out["lp_all"].shape == (B, num_actions)
        assert out["actions"].shape == (B,)
        live = inp["done"].numpy() == 0
        assert (~live).sum() == (2 if P > 2 else 1)
        multi = inp["obs_mask"].sum(1).numpy() > 1
        gaps.append(_top_two_gap(out["logits"])[live & multi])
        acts = out["actions"].long()
        assert (inp["obs_mask"].gather(1, acts.view(-1, 1)) > 0).all()
        assert (out["actions"].numpy()[~live] == 0).all()
        # members differ by far more than the kernel's tolerance: with any
        # other member's weights and table, a member's own rows read > 1e-2
        # away (so a kernel that used member 0 for everyone cannot pass)
        scratch = copy.deepcopy(policy)
        for m in range(P):
            sl = slice(m * E, (m + 1) * E)
            rows = {k: v[sl] for k, v in inp.items()}
            valid = (rows["obs_mask"] > 0) & (rows["done"] == 0).view(-1, 1)
            for m2 in range(P):
                if m2 == m:
                    continue
                load_flat(scratch, pop[m2])
                other = act_reference(GREEDY, policy=scratch,
                                      model_emb=emb[m2], **rows)
                diff = (other["lp_all"] - out["lp_all"][sl]).abs()[valid]
                assert float(diff.max()) > 1e-2, (num_actions, P, E, m, m2)
    gaps = np.concatenate(gaps)
    assert len(gaps) > 100
    assert (gaps <= 2e-4).mean() <= 0.05
    # sample mode: every member draws the uniforms of a batch of E rows
    for num_actions, P, E in POP_CASES:
        _, inp, _, _ = _pop_case(num_actions, P, E)
        out = _pop_reference(num_actions, P, E, SAMPLE, seed=11, step=5)
        u = philox_uniform(11, 5, E)
        live = (inp["done"].numpy() == 0).reshape(P, E)
        got = out["u"].numpy().reshape(P, E)
        for m in range(P):
            np.testing.assert_array_equal(got[m][live[m]], u[live[m]])
        acts = out["actions"].long()
        assert (inp["obs_mask"].gather(1, acts.view(-1, 1)) > 0).all()


@pytest.mark.parametrize("sigma", [0.02, 0.3])
def test_reference_near_tie_share_other_sigmas(sigma):
    gaps = []
    for num_actions, P, E in POP_CASES[:3]:
        _, inp, _, _ = _pop_case(num_actions, P, E, sigma)
        out = _pop_reference(num_actions, P, E, GREEDY, sigma=sigma)
        live = inp["done"].numpy() == 0
        multi = inp["obs_mask"].sum(1).numpy() > 1
        gaps.append(_top_two_gap(out["logits"])[live & multi])
    assert (np.concatenate(gaps) <= 2e-4).mean() <= 0.05


def _cpu_venv(jobs_dir, num_envs=2, base_seed=19):
    from ddls_amd.rl.engine_env import EngineVectorEnv
    return EngineVectorEnv(
        lambda: make_env(jobs_dir, "remove_and_repeat", 2, 3000, 15),
        num_envs=num_envs, device=torch.device("cpu"), base_seed=base_seed)


def test_common_random_numbers(multi_model_files):
    """Four identical members in sample mode: same schedules, same uniforms,
    so bit-identical fitness and two tied pairs."""
    venv = _cpu_venv(multi_model_files)
    assert venv.supports_population_eval
    policy = _policy(17, seed=4)
    ev = PopulationEvaluator(venv, policy, perturbation_pairs=2,
                             envs_per_member=2, eval_max_steps=8,
                             deterministic=False)
    theta = _flat(policy)
    pop = theta.repeat(4, 1).contiguous()
    res = ev.evaluate(pop, generation=0)
    fit = res["fitness"]
    assert fit.dtype == np.float64 and fit.shape == (4,)
    assert np.isfinite(fit).all()
    assert all(fit[m].tobytes() == fit[0].tobytes() for m in range(4))
    assert count_tied_pairs(fit) == 2
    np.testing.assert_array_equal(es_pair_weights(centered_ranks_ties(fit)),
                                  np.zeros(2, dtype=np.float32))
    assert res["returns"].shape == (4, 2)
    assert res["eval_steps"] == 8
    assert 8 * res["truncated_envs"] <= res["live_steps"] <= 8 * 4 * 2
    # the caller's policy was not touched, and its env was not stepped
    assert torch.equal(_flat(policy), theta)
    # perturbed members do differ
    eps, pop2 = ev.perturb(theta, 0.1, 0)
    assert eps.shape == (2, theta.numel()) and pop2.shape == (4, theta.numel())
    np.testing.assert_array_equal(
        pop2.numpy(), es_population_reference(theta.numpy(), eps.numpy(), 0.1))


def _es_trainer(venv, device, seed=4, **cfg):
    policy = _policy(17, seed=seed)
    return ESTrainer(venv, policy, ESConfig(**cfg), device=device)


POP_CFG = dict(evaluator="population", perturbation_pairs=2,
               envs_per_member=2, eval_max_steps=6, noise_seed=3)


def test_trainer_population_on_cpu(multi_model_files, capsys):
    dev = torch.device("cpu")
    runs = []
    for _ in range(2):
        tr = _es_trainer(_cpu_venv(multi_model_files), dev, **POP_CFG)
        before = tr._get_flat().clone()
        stats = [tr.train() for _ in range(2)]
        for st in stats:
            assert np.isfinite(st["fitness_mean"])
            assert np.isfinite(st["fitness_max"])
            assert np.isfinite(st["episode_reward_mean"])
            assert st["evaluator"] == 1
            assert st["eval_steps"] == 6
            assert st["truncated_envs"] > 0
            assert 0 <= st["tied_pairs"] <= 2
        assert stats[1]["total_env_steps"] > stats[0]["total_env_steps"] > 0
        assert stats[1]["iteration"] == 2
        assert not torch.equal(before, tr._get_flat())
        runs.append(tr._get_flat().numpy().tobytes())
    assert runs[0] == runs[1]

    # resume: the noise and the uniforms depend on the iteration alone
    a = _es_trainer(_cpu_venv(multi_model_files), dev, **POP_CFG)
    a.train()
    state = copy.deepcopy(a.state_dict())
    assert set(state) == {"policy", "iteration", "total_env_steps", "algo"}
    b = _es_trainer(_cpu_venv(multi_model_files), dev, seed=99, **POP_CFG)
    b.load_state_dict(state)
    b.train()
    assert b._get_flat().numpy().tobytes() == runs[0]
    assert b.total_env_steps == stats[1]["total_env_steps"]
    assert capsys.readouterr().err.count("evaluator='population'") == 0


def test_trainer_population_falls_back_and_validates(multi_model_files,
                                                     capsys):
    from ddls_amd.rl.rollout import VectorEnv
    dev = torch.device("cpu")
    ends = {}
    for evaluator in ("population", "sequential"):
        venv = VectorEnv([lambda: make_env(multi_model_files,
                                           "remove_and_repeat", 2, 3000, 30)],
                         base_seed=21)
        tr = _es_trainer(venv, dev, evaluator=evaluator, perturbation_pairs=2,
                         fragment_steps=3)
        torch.manual_seed(6)
        np.random.seed(6)
        for _ in range(2):
            st = tr.train()
            assert st["evaluator"] == 0
        ends[evaluator] = tr._get_flat().numpy().tobytes()
        n_warn = capsys.readouterr().err.count("evaluator='population'")
        assert n_warn == (1 if evaluator == "population" else 0)
    assert ends["population"] == ends["sequential"]
    with pytest.raises(ValueError):
        _es_trainer(_cpu_venv(multi_model_files), dev, evaluator="bogus")


def test_config_passes_population_fields(multi_model_files):
    import os

    import yaml

    from ddls_amd.runtime.config import build_trainer_from_config, load_config
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = load_config(os.path.join(root, "configs", "train_config.yaml"))
    with open(os.path.join(root, "configs", "algo", "es.yaml")) as f:
        cfg["algo"] = yaml.safe_load(f)
    assert cfg["algo"]["evaluator"] == "sequential"
    cfg["algo"].update(evaluator="population", envs_per_member=2,
                       perturbation_pairs=2, eval_max_steps=4, noise_seed=5,
                       deterministic_eval=True)
    cfg["env_config"]["jobs_config"]["path_to_files"] = multi_model_files
    cfg["env_config"]["jobs_config"]["replication_factor"] = 2
    cfg["epoch_loop"]["num_envs"] = 2
    cfg["epoch_loop"]["num_env_workers"] = 1
    cfg["epoch_loop"]["precompute_lookaheads"] = False
    cfg["epoch_loop"]["env_backend"] = "engine"
    tr = build_trainer_from_config(cfg, device=torch.device("cpu"))
    assert isinstance(tr, ESTrainer)
    c = tr.config
    assert (c.evaluator, c.envs_per_member, c.perturbation_pairs,
            c.eval_max_steps, c.noise_seed, c.deterministic_eval) == \
        ("population", 2, 2, 4, 5, True)
    st = tr.train()
    assert st["evaluator"] == 1 and st["eval_steps"] == 4
    assert np.isfinite(st["fitness_mean"])
    tr.env.close()


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
def _ext():
    from ddls_amd import ops
    return ops.get_extension(required=True)


def _ulp(x):
    x = np.abs(np.asarray(x, dtype=np.float32))
    return (np.nextafter(x, np.float32(np.inf)) - x).astype(np.float64)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 5, 4096 + 3])
def test_kernel_es_perturb(n):
    dev = torch.device("cuda:0")
    K, seed = 3, 2 ** 40 + 17
    rng = np.random.RandomState(n)
    # policy-sized weights, and weights whose binade holds theta +- t (t is
    # at most 0.02 * 5.77): there each row is off by at most half an ulp of
    # theta, so the exact sum of a pair is within one ulp of 2 * theta
    sigma = 0.02
    thetas = [(False, (rng.randn(n) * 0.1).astype(np.float32)),
              (True, (rng.choice([-1.0, 1.0], n)
                      * rng.uniform(1.0, 1.5, n)).astype(np.float32))]
    worst = 0.0
    for generation in (0, 2 ** 33 + 1):
        ref = es_noise_reference(seed, generation, K, n)
        for same_binade, theta in thetas:
            eps = torch.full((K, n), SENTINEL, device=dev)
            pop = torch.full((2 * K, n), SENTINEL, device=dev)
            _ext().es_perturb(torch.from_numpy(theta).to(dev),
                              float(np.float32(sigma)), seed, generation, eps,
                              pop)
            torch.cuda.synchronize()
            eps, pop = eps.cpu().numpy(), pop.cpu().numpy()
            err = float(np.abs(eps.astype(np.float64) - ref).max())
            worst = max(worst, err)
            print(f"es_perturb n={n} gen={generation}: max |eps - ref| = "
                  f"{err:.3e}")
            np.testing.assert_allclose(eps, ref, atol=1e-5, rtol=0)
            assert pop.tobytes() == es_population_reference(
                theta, eps, sigma).tobytes()
            if same_binade:
                pair = pop[0::2].astype(np.float64) + pop[1::2]
                assert (np.abs(pair - 2.0 * theta.astype(np.float64))
                        <= _ulp(theta)).all()
    assert worst <= 1e-5


def _population_kernel(mode, inp, pop, emb, offs, E, seed=0, step=0,
                       optional=True):
    dev = torch.device("cuda:0")
    B, num_actions = inp["obs_mask"].shape
    c = lambda t: t.to(dev).contiguous()
    f = lambda *s: torch.full(s, SENTINEL, device=dev)
    empty = torch.empty(0, device=dev)
    rows = {"lp_all": f(B, num_actions), "logp": f(B), "value": f(B),
            "u": f(B)}
    actions = torch.full((B,), -1, dtype=torch.int32, device=dev)
    args = [rows[k] if optional else empty
            for k in ("lp_all", "logp", "value", "u")]
    _ext().actor_population(
        c(inp["obs_gf"]), c(inp["obs_mask"]), c(inp["obs_model"]),
        c(inp["done"]), c(pop), c(emb), offs, E, mode, seed, step, actions,
        *args)
    torch.cuda.synchronize()
    out = {k: v.cpu() for k, v in rows.items()}
    out["actions"] = actions.cpu()
    return out


@pytest.mark.gpu
def test_kernel_actor_population_matches_reference():
    excluded = total = 0
    for num_actions, P, E in POP_CASES:
        policy, inp, pop, emb = _pop_case(num_actions, P, E)
        ref = _pop_reference(num_actions, P, E, GREEDY)
        offs = head_offsets(policy)
        got = _population_kernel(GREEDY, inp, pop, emb, offs, E)
        live = inp["done"] == 0
        valid = (inp["obs_mask"] > 0) & live.view(-1, 1)
        np.testing.assert_allclose(got["value"][live].numpy(),
                                   ref["value"][live].numpy(), atol=1e-4,
                                   rtol=0)
        np.testing.assert_allclose(got["lp_all"][valid].numpy(),
                                   ref["lp_all"][valid].numpy(), atol=1e-4,
                                   rtol=0)
        acts = got["actions"].long()
        assert (acts >= 0).all()
        np.testing.assert_array_equal(
            got["logp"][live].numpy(),
            got["lp_all"].gather(1, acts.view(-1, 1)).squeeze(1)[live].numpy())
        assert (got["actions"][~live] == 0).all()
        for k in ("lp_all", "logp", "value", "u"):
            assert (got[k][~live] == SENTINEL).all(), k
        multi = inp["obs_mask"].sum(1) > 1
        sure = torch.as_tensor(_top_two_gap(ref["logits"]) > 2e-4) | ~multi
        sel = live & sure
        np.testing.assert_array_equal(got["actions"][sel].numpy(),
                                      ref["actions"][sel].numpy())
        excluded += int((live & ~sure).sum())
        total += int(live.sum())
        # production passes no optional output: only actions are written
        bare = _population_kernel(GREEDY, inp, pop, emb, offs, E,
                                  optional=False)
        assert torch.equal(bare["actions"], got["actions"])
        for k in ("lp_all", "logp", "value", "u"):
            assert (bare[k] == SENTINEL).all(), k
    assert excluded <= 0.05 * total, (excluded, total)


@pytest.mark.gpu
@pytest.mark.parametrize("num_actions", [17, 5])
@pytest.mark.parametrize("E", [3, 4, 5, 67])
def test_kernel_actor_population_equals_actor_batch(num_actions, E):
    """Equal members: each member's slice is byte for byte what actor_batch
    gives for that slice's E rows (row arithmetic, block-to-member mapping,
    the e-indexed Philox counter)."""
    P = 4
    policy = _policy(num_actions)
    head = head_params(policy)
    offs = head_offsets(policy)
    theta = _flat(policy)
    pop = theta.repeat(P, 1).contiguous()
    B = P * E
    g = torch.Generator().manual_seed(31 * E + num_actions)
    table = torch.randn(3, 16, generator=g)
    emb = table.repeat(P, 1, 1).contiguous()
    mask = (torch.rand(B, num_actions, generator=g)
            < torch.rand(B, 1, generator=g)).float()
    mask[:, 0] = 1.0
    mask[1, :] = 1.0
    done = torch.zeros(B, dtype=torch.uint8)
    done[2] = 1
    done[B - 1] = 1
    inp = dict(obs_gf=torch.randn(B, 17, generator=g), obs_mask=mask,
               obs_model=torch.randint(0, 3, (B,), generator=g).int(),
               obs_sched=torch.zeros(B, dtype=torch.int32), done=done)
    inp["obs_model"][E] = 7          # a model id outside the table
    seed, step = 2 ** 40 + 17, 2 ** 33 + 5
    for mode in (GREEDY, SAMPLE):
        got = _population_kernel(mode, inp, pop, emb, offs, E, seed=seed,
                                 step=step)
        for m in range(P):
            sl = slice(m * E, (m + 1) * E)
            rows = {k: v[sl] for k, v in inp.items()}
            rows["model_emb"] = table
            want = _actor_batch(mode, rows, head=head, seed=seed, step=step,
                                sentinel=SENTINEL)
            for k in ("actions", "lp_all", "logp", "value", "u"):
                assert got[k][sl].numpy().tobytes() == \
                    want[k].numpy().tobytes(), (mode, m, k)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 16])
@pytest.mark.parametrize("n", [1, 5, 4096 + 3])
def test_kernel_es_update(K, n):
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(100 * K + n)
    theta = (rng.randn(n) * 0.1).astype(np.float32)
    eps = es_noise_reference(1, 2, K, n)
    scale, decay = es_update_scalars(K, 0.02, 0.01, 0.005)
    ranks = centered_ranks_ties(rng.randn(2 * K).round(1))
    for w in (es_pair_weights(ranks), np.zeros(K, dtype=np.float32)):
        out = torch.full((n,), SENTINEL, device=dev)
        _ext().es_update(torch.from_numpy(theta).to(dev),
                         torch.from_numpy(eps).to(dev),
                         torch.from_numpy(w).to(dev), float(scale),
                         float(decay), out)
        torch.cuda.synchronize()
        want = es_update_reference(theta, eps, w, scale, decay)
        assert out.cpu().numpy().tobytes() == want.tobytes()
        if not w.any():
            assert want.tobytes() == (theta - decay * theta).tobytes()


def _gpu_venv(jobs_dir, num_envs=3, base_seed=23):
    from ddls_amd.rl.engine_env import EngineVectorEnv
    return EngineVectorEnv(
        lambda: make_env(jobs_dir, "remove_and_repeat", 2, 3000, 15),
        num_envs=num_envs, device=torch.device("cuda:0"), base_seed=base_seed)


@pytest.mark.gpu
def test_replicate_envs(multi_model_files):
    from ddls_amd.cluster.gpu_engine import GpuEngine
    from ddls_amd.cluster.vec_engine import drain_episode_schedule
    venv = _gpu_venv(multi_model_files)
    dev = venv.device
    scheds = [drain_episode_schedule(venv.gen, venv.spec, seed=500 + e)
              for e in range(3)]
    cap = max(s.n for s in scheds) + 8
    a = GpuEngine(venv.spec, B=12, device=dev, n_jobs_cap=cap)
    b = GpuEngine(venv.spec, B=12, device=dev, n_jobs_cap=cap)
    for e in range(3):
        a.reset_env(e, scheds[e])
    a.replicate_envs([0, 1, 2] * 3, list(range(3, 12)))
    for r in range(12):
        b.reset_env(r, scheds[r % 3])
    assert len(a._env_keys) > 30
    for k in a._env_keys:
        assert a.T[k].shape[0] == 12
        assert a.T[k].cpu().numpy().tobytes() == \
            b.T[k].cpu().numpy().tobytes(), k
    assert all(a.schedules[r] is scheds[r % 3] for r in range(12))
    for _ in range(3):
        mask = a.T["obs_mask"][:3]
        # the highest valid action of each schedule's env, for every member
        acts = (mask * torch.arange(mask.shape[1], device=dev)).argmax(1)
        a.step(acts.to(torch.int32).repeat(4))
        for k in a._env_keys:
            t = a.T[k].view(4, 3, *a.T[k].shape[1:])
            assert all(torch.equal(t[m], t[0]) for m in range(1, 4)), k
    assert int(a.T["ep_len"].min()) == 3
    with pytest.raises(ValueError):
        a.replicate_envs([0, 1], [1, 2])


@pytest.mark.gpu
def test_population_evaluator_lockstep(multi_model_files):
    venv = _gpu_venv(multi_model_files)
    policy = _policy(17, seed=4).to(venv.device)
    K, E, steps = 2, 3, 12
    ev = PopulationEvaluator(venv, policy, perturbation_pairs=K,
                             envs_per_member=E, eval_max_steps=steps,
                             deterministic=True)
    theta = _flat(policy)
    eps, pop = ev.perturb(theta, 0.1, 0)
    pop_cpu = pop.cpu()
    scratch = _policy(17, seed=4)
    ev.reset(ev.schedules(0))
    emb = ev.embeddings(pop)
    emb_cpu = emb.cpu()
    assert emb.shape[0] == 2 * K and emb.shape[2] == 16
    T = ev.eng.T
    want_ret = np.zeros(ev.B)
    excluded = total = 0
    for t in range(steps):
        live = (T["done"] == 0).cpu()
        obs = {k: T[k].cpu().clone() for k in
               ("obs_gf", "obs_mask", "obs_model", "obs_sched", "done")}
        ref = act_population_reference(GREEDY, policy=scratch, pop=pop_cpu,
                                       model_emb_pop=emb_cpu, E=E, **obs)
        actions = ev.act(pop, emb, t)
        multi = obs["obs_mask"].sum(1) > 1
        sure = torch.as_tensor(_top_two_gap(ref["logits"]) > 2e-4) | ~multi
        sel = live & sure
        np.testing.assert_array_equal(actions.cpu()[sel].numpy(),
                                      ref["actions"][sel].numpy())
        excluded += int((live & ~sure).sum())
        total += int(live.sum())
        ev.eng.step(actions)
        reward = T["reward"].cpu().numpy()
        want_ret = np.where(live.numpy(), want_ret + reward, want_ret)
    assert total > 0 and excluded <= 0.05 * total, (excluded, total)
    # the evaluator's own loop replays the same episode
    ev.reset(ev.schedules(0))
    ret, nsteps, played = ev.rollout(pop, emb, 0)
    assert played <= steps
    assert ret.dtype == torch.float64
    assert ret.cpu().numpy().tobytes() == want_ret.tobytes()


@pytest.mark.gpu
def test_trainer_population_on_gpu(multi_model_files):
    dev = torch.device("cuda:0")
    ends = []
    for _ in range(2):
        tr = _es_trainer(_gpu_venv(multi_model_files), dev,
                         evaluator="population", perturbation_pairs=2,
                         envs_per_member=3, eval_max_steps=12, noise_seed=3)
        before = tr._get_flat().clone()
        for _g in range(2):
            st = tr.train()
            assert np.isfinite(st["fitness_mean"])
            assert np.isfinite(st["episode_reward_mean"])
            assert st["evaluator"] == 1 and 0 < st["eval_steps"] <= 12
        assert st["total_env_steps"] > 0
        assert not torch.equal(before, tr._get_flat())
        assert torch.isfinite(tr._get_flat()).all()
        ends.append(tr._get_flat().cpu().numpy().tobytes())
    assert ends[0] == ends[1]
