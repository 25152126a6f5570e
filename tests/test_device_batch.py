"""Device-resident PPO batch: the minibatch stage kernel
(ops/hip/batch_stage.hip), the DeviceBatchStore / CapturedSGDStep.replay_next
path (rl/graph_step.py), EngineVectorEnv.rollout(device_resident=True) and
PPOConfig.device_batch.

The staged values are the same f32/i64 bits on the host-staged and on the
device path and the fused step has no atomics on the gradient path, so
parameters and Adam state are compared BITWISE; only the five loss sums
(float atomics) get the tolerance test_cached_step_shapes.py uses for them.

Three-model file set of tests/test_vec_engine.py, 16 envs x 16 steps = 256
samples, Fg = 34, A = 17.
"""
import numpy as np
import pytest
import torch

from tests.test_vec_engine import make_env

gpu = pytest.mark.gpu

_MODELS = {"m_small": (5, 0, 0.5, 11),
           "m_mid": (8, 2, 1.0, 12),
           "m_big": (11, 3, 1.6, 13)}
_NUM_ENVS, _STEPS = 16, 16
_N = _NUM_ENVS * _STEPS
_FG, _A = 34, 17
_DST_KEYS = ("gf", "mask", "model_ids", "actions", "old_logp", "adv",
             "vtarg")


@pytest.fixture(scope="module")
def jobs_dir(tmp_path_factory):
    from ddls_amd.workloads import generate_model, write_pipedream_txt
    d = tmp_path_factory.mktemp("jobs_device_batch")
    for name, (nn, sk, sc, seed) in _MODELS.items():
        nodes, edges = generate_model(name, nn, sk, sc, seed)
        write_pipedream_txt(str(d / f"{name}.txt"), nodes, edges)
    return str(d)


def _venv(jobs_dir, dev, base_seed=31):
    from ddls_amd.rl.engine_env import EngineVectorEnv
    return EngineVectorEnv(
        lambda: make_env(jobs_dir, "remove_and_repeat", 2, 4000, 20),
        num_envs=_NUM_ENVS, device=dev, base_seed=base_seed)


def _policy(dev, seed=4):
    from ddls_amd.models.gnn import GNNPolicy
    torch.manual_seed(seed)
    return GNNPolicy(num_actions=_A).to(dev)


def _params(policy):
    return torch.cat([p.detach().reshape(-1).cpu()
                      for p in policy.parameters()])


# ---------------------------------------------------------------------------
# CPU tests
# ---------------------------------------------------------------------------

def test_device_resident_rollout_matches_host_rollout_cpu(jobs_dir):
    """CPU engine backend: same sampling and RNG stream, same arrays; obs is
    a lazy sequence equal to the host list entry by entry."""
    dev = torch.device("cpu")
    outs = []
    for resident in (False, True):
        venv = _venv(jobs_dir, dev)
        policy = _policy(dev)
        torch.manual_seed(9)
        if resident:
            outs.append(venv.rollout(policy, _STEPS, device_resident=True))
        else:
            outs.append(venv.rollout(policy, _STEPS))
    host, res = outs
    assert isinstance(host["obs"], list)
    for k in ("actions", "logp", "values", "rewards", "dones",
              "bootstrap_values", "lp_all"):
        a, b = np.asarray(host[k]), np.asarray(res[k])
        assert a.dtype == b.dtype and a.shape == b.shape, k
        assert a.tobytes() == b.tobytes(), k
    assert not isinstance(res["obs"], list)
    assert len(res["obs"]) == _N == len(host["obs"])
    for i in (0, 17, 255):
        h, r = host["obs"][i], res["obs"][i]
        assert r.model_id == h.model_id
        for f in ("node_features", "edge_features", "edges_src",
                  "edges_dst", "graph_features", "action_mask"):
            np.testing.assert_array_equal(getattr(r, f), getattr(h, f), f)
        assert r.graph_features.shape == (_FG,)
        np.testing.assert_array_equal(r.action_mask, r.graph_features[17:])
    # the flat tensors under the new keys are the same samples
    assert tuple(res["gfull_dev"].shape) == (_N, _FG)
    np.testing.assert_array_equal(res["gfull_dev"][17].numpy(),
                                  host["obs"][17].graph_features)
    assert int(res["model_ids_dev"][255]) == host["obs"][255].model_id
    np.testing.assert_array_equal(res["actions_dev"].numpy(),
                                  host["actions"].reshape(-1))
    np.testing.assert_array_equal(res["logp_dev"].numpy(),
                                  host["logp"].reshape(-1))
    np.testing.assert_array_equal(res["lp_all_dev"].numpy(),
                                  host["lp_all"].reshape(_N, _A))


def test_stage_reference_hand_built_rows():
    """stage_reference against rows written out by hand, B=5: the perm row
    holds index 0, index n-1 and a repeated index."""
    from ddls_amd.rl.graph_step import DeviceBatchStore, stage_reference
    n, B = 6, 5
    store = DeviceBatchStore(cap_n=8, cap_mb=3, B=B, Fg=_FG, A=_A,
                             device="cpu")
    rows = np.arange(n)
    gfull = (rows[:, None] * 100 + np.arange(_FG)[None, :]).astype(np.float32)
    table = np.array([[1, 2, 3, 4, 5],
                      [0, n - 1, 2, 2, 3]], dtype=np.int32)
    store.bind(gfull, (rows % 3).astype(np.int64),
               (rows + 10).astype(np.int64),
               (-rows - 0.5).astype(np.float32),
               (rows * 0.25).astype(np.float32),
               (rows * 2.0).astype(np.float32), table)
    assert store.n == n and store.num_mb == 2
    assert store.h2d_copies == 0          # CPU store: nothing to upload
    out = stage_reference(store, store.perm, 1)
    picks = [0, n - 1, 2, 2, 3]
    for i, r in enumerate(picks):
        for c in range(_FG):
            assert float(out["gf"][i, c]) == r * 100 + c
        for a in range(_A):
            assert float(out["mask"][i, a]) == r * 100 + 17 + a
        assert int(out["model_ids"][i]) == r % 3
        assert int(out["actions"][i]) == r + 10
        assert float(out["old_logp"][i]) == -r - 0.5
        assert float(out["adv"][i]) == r * 0.25
        assert float(out["vtarg"][i]) == r * 2.0
    assert out["gf"].dtype == torch.float32
    assert out["model_ids"].dtype == torch.int64
    assert out["actions"].dtype == torch.int64
    # the table is checked on the way in
    bad = table.copy()
    bad[0, 0] = n
    with pytest.raises(ValueError):
        store.bind(gfull, rows % 3, rows + 10, -rows - 0.5, rows * 0.25,
                   rows * 2.0, bad)


def test_ppo_device_batch_on_falls_back_on_cpu(jobs_dir):
    """No cuda: device_batch='on' takes the host path and loses nothing —
    bit-identical parameters to 'off'."""
    from ddls_amd.rl.ppo import PPOConfig, PPOTrainer
    dev = torch.device("cpu")
    got = {}
    for mode in ("on", "off"):
        venv = _venv(jobs_dir, dev, base_seed=11)
        policy = _policy(dev)
        cfg = PPOConfig(train_batch_size=_N, sgd_minibatch_size=32,
                        num_sgd_iter=2, device_batch=mode)
        trainer = PPOTrainer(venv, policy, cfg, device=dev)
        torch.manual_seed(3)
        stats = trainer.train(num_steps=_STEPS)
        assert stats["device_batch"] == 0
        assert stats["env_steps_this_iter"] == _N
        got[mode] = _params(policy)
    assert torch.equal(got["on"], got["off"])
    with pytest.raises(ValueError):
        PPOTrainer(_venv(jobs_dir, dev), _policy(dev),
                   PPOConfig(device_batch="sometimes"), device=dev)


# ---------------------------------------------------------------------------
# GPU tests
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gpu_rollout(jobs_dir):
    """One device-resident engine rollout shared by the GPU tests, as the
    trainer collects it: flat per-sample arrays, GAE advantages and value
    targets on the host, the ``*_dev`` tensors on the device."""
    from ddls_amd.rl.ppo import PPOConfig, PPOTrainer
    dev = torch.device("cuda:0")
    venv = _venv(jobs_dir, dev)
    trainer = PPOTrainer(venv, _policy(dev),
                         PPOConfig(train_batch_size=_N, device_batch="on"),
                         device=dev)
    data = trainer.collect_rollout(_STEPS)
    assert not isinstance(data["obs"], list) and len(data["obs"]) == _N
    return {"venv": venv, "data": data, "dev": dev}


def _alloc_stepper(gpu_rollout, B, store=None, seed=4):
    from ddls_amd.rl.graph_step import CapturedSGDStep
    from ddls_amd.rl.ppo import PPOConfig
    dev = gpu_rollout["dev"]
    policy = _policy(dev, seed)
    cfg = PPOConfig(sgd_minibatch_size=B, num_sgd_iter=1)
    opt = torch.optim.Adam(policy.parameters(), lr=cfg.lr)
    st = CapturedSGDStep(policy, opt, cfg, dev,
                         models_batch=gpu_rollout["venv"]._models_batch,
                         device_store=store)
    return st, cfg


def _random_store(B, cap_mb, dev, seed):
    """n_rows = 256 random rows in a cap_n = 384 store; the rows past
    n_rows hold a sentinel a broken guard would copy out."""
    from ddls_amd.rl.graph_step import DeviceBatchStore
    rng = np.random.RandomState(seed)
    store = DeviceBatchStore(cap_n=384, cap_mb=cap_mb, B=B, Fg=_FG, A=_A,
                             device=dev)
    store.gfull.fill_(-7.0)
    store.model_ids.fill_(2)
    store.actions.fill_(16)
    store.old_logp.fill_(-7.0)
    store.adv.fill_(-7.0)
    store.vtarg.fill_(-7.0)
    host = (rng.randn(_N, _FG).astype(np.float32),
            rng.randint(0, 3, _N).astype(np.int64),
            rng.randint(0, _A, _N).astype(np.int64),
            rng.randn(_N).astype(np.float32),
            rng.randn(_N).astype(np.float32),
            rng.randn(_N).astype(np.float32))
    x = rng.randint(1, _N - 1, B)
    x[0], x[1], x[3] = 0, _N - 1, x[2]           # first, last, a duplicate
    y = rng.randint(0, _N, B)
    return store, host, x, y


def _dst_clone(d):
    return {k: d[k].detach().clone() for k in _DST_KEYS}


def _assert_dst_equal(d, ref, what):
    for k in _DST_KEYS:
        assert d[k].dtype == ref[k].dtype, (what, k)
        assert torch.equal(d[k], ref[k]), (what, k)


@gpu
@pytest.mark.parametrize("B", [5, 33, 128])
def test_stage_kernel_matches_reference(gpu_rollout, B):
    """Eager launches over minibatches X, Y, X: every destination buffer
    equals stage_reference bitwise, the cursor reads 1, 2, 3, the third
    launch equals the first (no stale rows from Y) and err stays 0."""
    from ddls_amd.rl.graph_step import stage_reference
    dev = gpu_rollout["dev"]
    store, host, x, y = _random_store(B, cap_mb=4, dev=dev, seed=B)
    store.bind(*host, np.stack([x, y, x]))
    assert store.h2d_copies == 7        # all-host inputs: one copy per field
    st, _cfg = _alloc_stepper(gpu_rollout, B)
    st._alloc(0, 0)
    ext = st._ext
    assert hasattr(ext, "cached_stage")
    outs = []
    for k in range(3):
        ref = stage_reference(store, store.perm, k)
        store.stage_into(ext, st.d)
        torch.cuda.synchronize()
        assert int(store.cursor.item()) == k + 1
        _assert_dst_equal(st.d, ref, f"launch {k}")
        outs.append(_dst_clone(st.d))
    assert not torch.equal(outs[0]["gf"], outs[1]["gf"]), \
        "Y must be a different minibatch"
    _assert_dst_equal(outs[2], outs[0], "X again after Y")
    assert torch.equal(outs[0]["mask"], outs[0]["gf"][:, _FG - _A:])
    assert int(store.err.item()) == 0
    store.check_err()


@gpu
def test_stage_kernel_guards(gpu_rollout):
    """Past the end of the table, and an index equal to n_rows: err is set,
    the destination buffers keep their bits and the cursor stays inside the
    table.  Every out-of-range position lies inside the allocation."""
    dev = gpu_rollout["dev"]
    B = 33
    store, host, x, y = _random_store(B, cap_mb=5, dev=dev, seed=77)
    store.bind(*host, np.stack([x, y, x]))          # n_mb = 3 of cap_mb = 5
    # row 3 is beyond n_mb but holds valid, different rows
    store.perm[3].copy_(torch.as_tensor((y[::-1] % _N).astype(np.int32)))
    st, _cfg = _alloc_stepper(gpu_rollout, B)
    st._alloc(0, 0)
    ext = st._ext
    for _ in range(3):
        store.stage_into(ext, st.d)
    torch.cuda.synchronize()
    assert int(store.err.item()) == 0 and int(store.cursor.item()) == 3
    before = _dst_clone(st.d)
    store.stage_into(ext, st.d)                     # fourth launch
    torch.cuda.synchronize()
    assert int(store.err.item()) != 0
    assert int(store.cursor.item()) == 3
    _assert_dst_equal(st.d, before, "launch past the table")
    with pytest.raises(RuntimeError, match="error code"):
        store.check_err()

    # an index equal to n_rows (< cap_n): sentinel rows must not be copied
    store.reset()
    assert int(store.err.item()) == 0 and int(store.cursor.item()) == 0
    store.perm[0, B - 1] = _N
    store.stage_into(ext, st.d)
    torch.cuda.synchronize()
    assert int(store.err.item()) != 0
    assert int(store.cursor.item()) == 0
    _assert_dst_equal(st.d, before, "index == n_rows")

    # cursor == BYPASS: the host-staged mode, nothing happens and no error
    store.reset()
    store.set_bypass()
    store.stage_into(ext, st.d)
    torch.cuda.synchronize()
    assert int(store.err.item()) == 0
    assert int(store.cursor.item()) == store.BYPASS
    _assert_dst_equal(st.d, before, "bypass")


@gpu
def test_replay_next_matches_host_staged(gpu_rollout):
    """Stepper A replays from a device store, stepper B is host-staged with
    prepare/commit on the same index lists (two epochs of three B=32
    minibatches from the trainer's permutation stream): bit-identical
    parameters and Adam state, one capture, no per-minibatch H2D copy.

    The inputs are the rollout's own standardised GAE advantages and value
    targets.  Bitwise equality of the parameters presupposes that the
    global-norm clip stays inactive: ``flat_sumsq`` adds its block partials
    with float atomics, so an active clip factor carries the norm's
    last-bit run-to-run spread into the parameters of ANY two steppers, two
    host-staged ones included (measured on an MI355X with N(0,1) advantages
    and targets, clip active from the second step: max |dp| 1.5e-8 between
    two host-staged steppers and the same between store and host).  The
    test therefore checks after every step that the norm is under the clip.
    """
    from ddls_amd.rl.graph_step import DeviceBatchStore, _FusedCachedEngine
    data, dev = gpu_rollout["data"], gpu_rollout["dev"]
    B, n = 32, 96
    rng = np.random.RandomState(0)                 # iteration 0, rank 0
    idx_lists = []
    for _ in range(2):
        perm = rng.permutation(n)
        for s in range(0, n, B):
            idx_lists.append(perm[s:s + B])
    assert len(idx_lists) == 6
    adv = data["advantages"]
    adv = ((adv - adv.mean()) / max(adv.std(), 1e-4)).astype(np.float32)[:n]
    vtarg = np.asarray(data["value_targets"], dtype=np.float32)[:n]
    actions = np.asarray(data["actions"]).reshape(-1)[:n]
    logp = np.asarray(data["logp"]).reshape(-1)[:n].astype(np.float32)

    store = DeviceBatchStore(cap_n=128, cap_mb=7, B=B, Fg=_FG, A=_A,
                             device=dev)
    st_a, cfg = _alloc_stepper(gpu_rollout, B, store=store)
    st_b, _ = _alloc_stepper(gpu_rollout, B)
    assert _FusedCachedEngine.eligible(st_a.policy, st_a._ext)
    for st in (st_a, st_b):
        st.set_kl_coeff(cfg.kl_coeff)

    store.bind(data["gfull_dev"][:n], data["model_ids_dev"][:n],
               data["actions_dev"][:n], data["logp_dev"][:n], adv, vtarg,
               np.stack(idx_lists))
    assert store.h2d_copies == 3                   # adv, vtarg, perm
    assert st_a.ensure_capacity(0, 0), st_a.last_error
    assert st_a._fused_cached is not None
    assert int(store.cursor.item()) == 0 and int(store.err.item()) == 0
    st_a.reset_stats()
    clip_sq = float(cfg.grad_clip) ** 2

    def unclipped(st, k):
        normsq = float(st.normsq.item())
        print(f"step {k}: grad norm^2 {normsq:.6g} (clip^2 {clip_sq:.6g})")
        assert normsq < 0.9 * clip_sq, \
            "case precondition: the grad clip must stay inactive"

    for k in range(len(idx_lists)):
        st_a.replay_next()
        unclipped(st_a, k)
    stats_a = st_a.read_stats()
    assert int(store.cursor.item()) == 6
    assert st_a.capture_count == 1
    assert st_a.h2d_copies == 3                    # nothing per minibatch

    assert st_b.ensure_capacity(0, 0), st_b.last_error
    st_b.reset_stats()
    obs = data["obs"]
    for k, idx in enumerate(idx_lists):
        st_b.commit(st_b.prepare([obs[i] for i in idx], actions[idx],
                                 logp[idx], adv[idx], vtarg[idx]))
        unclipped(st_b, k)
    stats_b = st_b.read_stats()
    assert st_b.h2d_copies == 2 * len(idx_lists)

    for name in ("flat_p", "flat_m", "flat_v", "step_t"):
        assert torch.equal(getattr(st_a, name), getattr(st_b, name)), name
    assert float(st_a.step_t.item()) == 6.0
    np.testing.assert_allclose(stats_a, stats_b, rtol=1e-4, atol=1e-5)

    # the host-staged API keeps working on the stepper that has a store
    st_a.reset_stats()
    st_b.reset_stats()
    idx = idx_lists[0]
    args = ([obs[i] for i in idx], actions[idx], logp[idx], adv[idx],
            vtarg[idx])
    assert st_a.step(*args) and st_b.step(*args)
    unclipped(st_a, 6)
    unclipped(st_b, 6)
    st_a.read_stats()
    assert torch.equal(st_a.flat_p, st_b.flat_p)
    assert st_a.capture_count == 1
    with pytest.raises(RuntimeError):
        st_a.replay_next()                         # store is bypassed now


@pytest.fixture(scope="module")
def e2e(jobs_dir):
    """Two train() iterations per trainer: 'off', 'on', and 'on' with twice
    the SGD epochs.

    grad_clip is set far above any gradient norm, so the clip runs but its
    factor is exactly 1.  With the default 1.5 the clip is active in most of
    these 16 steps (norm^2 up to 13.6 against 2.25), and its factor carries
    the last-bit spread of ``flat_sumsq``'s float atomics into the
    parameters: measured on an MI355X, two 'off' trainers then differ from
    EACH OTHER by 1.5e-8 after either iteration, 'on' from 'off' by 1.5e-8
    and 1.2e-7, with identical per-step norms to four digits; with the clip
    inactive all three are bit-identical, kl_analytic included.  Bitwise
    parity of the two paths is only defined where the host path is bitwise
    reproducible itself."""
    from ddls_amd.rl.ppo import PPOConfig, PPOTrainer
    dev = torch.device("cuda:0")
    out = {}
    for key, mode, iters in (("off", "off", 2), ("on", "on", 2),
                             ("on4", "on", 4)):
        venv = _venv(jobs_dir, dev, base_seed=21)
        policy = _policy(dev)
        cfg = PPOConfig(train_batch_size=_N, sgd_minibatch_size=64,
                        num_sgd_iter=iters, device_batch=mode, grad_clip=1e6)
        trainer = PPOTrainer(venv, policy, cfg, device=dev)
        torch.manual_seed(13)
        runs = []
        for _ in range(2):
            stats = trainer.train(num_steps=_STEPS)
            stats["last_grad_normsq"] = float(trainer._stepper.normsq.item())
            runs.append((stats, _params(policy)))
        out[key] = runs
    return out


@gpu
def test_trainer_device_batch_matches_host_path(e2e):
    """PPOTrainer.train() twice, 'on' against 'off': bit-identical
    parameters after each iteration (the second rebinds the store), with
    the grad clip inactive (see the e2e fixture)."""
    for it in range(2):
        s_off, p_off = e2e["off"][it]
        s_on, p_on = e2e["on"][it]
        print(f"iteration {it}: last grad norm^2 on "
              f"{s_on['last_grad_normsq']:.6g} off "
              f"{s_off['last_grad_normsq']:.6g}; max |dp| "
              f"{(p_on - p_off).abs().max().item():.3g}")
        assert s_off["device_batch"] == 0 and s_on["device_batch"] == 1
        assert torch.equal(p_on, p_off), f"iteration {it}"
        assert s_on["kl_analytic"] == s_off["kl_analytic"]
        assert s_on["kl_coeff"] == s_off["kl_coeff"]
        assert s_on["hipgraph_minibatches"] == 8
        assert s_off["hipgraph_minibatches"] == 8
        assert s_on["hipgraph_captures"] == 1
        assert s_off["hipgraph_captures"] == 1
        np.testing.assert_allclose(
            [s_on[k] for k in ("policy_loss", "vf_loss", "kl", "entropy",
                               "total_loss")],
            [s_off[k] for k in ("policy_loss", "vf_loss", "kl", "entropy",
                                "total_loss")], rtol=1e-4, atol=1e-5)


@gpu
def test_trainer_h2d_copies_do_not_grow_with_epochs(e2e):
    for it in range(2):
        assert e2e["off"][it][0]["staged_h2d_copies"] == 2 * 8
        const = e2e["on"][it][0]["staged_h2d_copies"]
        assert 0 < const <= 3
        s4 = e2e["on4"][it][0]
        assert s4["device_batch"] == 1
        assert s4["hipgraph_minibatches"] == 16
        assert s4["staged_h2d_copies"] == const
