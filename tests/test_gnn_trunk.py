"""Fused GNN trunk (ops/hip/gnn_trunk.hip, models/gnn.py ``gnn_trunk``,
rl/dqn.py ``trunk_step="fused"``) against the plain torch chain
``MeanPoolLayer.forward`` x 2 + ``graph_mean`` in float64 on the CPU.

Largest error / bound seen on an MI355X over the cases below: see the
precision table of docs/KERNELS.md, "gnn_trunk.hip"."""
import copy
import functools

import numpy as np
import pytest
import torch

from tests.test_dqn_head_step import _hold_to_float64_bound
from tests.test_vec_engine import make_env, multi_model_files  # noqa: F401

# name: (nodes per graph, edges per graph, seed)
CASES = {
    "one_node": ((1,), (0,), 1),
    "two_nodes": ((2,), (1,), 1),
    "three_graphs": ((1, 17, 33), (0, 40, 70), 1),
    "five_graphs": ((3, 16, 64, 65, 130), (2, 31, 200, 129, 300), 1),
    "one_large": ((300,), (700,), 5),
}


def _gnn(seed):
    """The tuned GNN with LayerNorm weights and biases moved off 1 and 0."""
    from ddls_amd.models.gnn import DEFAULT_GNN_CONFIG, GNN
    torch.manual_seed(seed)
    gnn = GNN(dict(DEFAULT_GNN_CONFIG))
    assert gnn._trunk_ok and len(list(gnn.parameters())) == 24
    with torch.no_grad():
        for name, p in gnn.named_parameters():
            if p.dim() == 1 and ".0." in name:       # the LayerNorms
                p.add_(0.1 * torch.randn(p.shape))
    return gnn


def _batch(nodes, edges, seed):
    """Seeded CPU batch: src / dst drawn inside each graph, z / e randn."""
    from ddls_amd.models.gnn import GraphBatch
    g = torch.Generator(device="cpu").manual_seed(seed)
    off = np.concatenate([[0], np.cumsum(nodes)])
    src = torch.cat([torch.randint(int(off[i]), int(off[i + 1]), (m,),
                                   generator=g) for i, m in enumerate(edges)])
    dst = torch.cat([torch.randint(int(off[i]), int(off[i + 1]), (m,),
                                   generator=g) for i, m in enumerate(edges)])
    return GraphBatch(
        z=torch.randn(int(off[-1]), 5, generator=g),
        e=torch.randn(sum(edges), 2, generator=g), src=src, dst=dst,
        graph_of_node=torch.repeat_interleave(torch.arange(len(nodes)),
                                              torch.as_tensor(nodes)),
        num_graphs=len(nodes))


def _preactivations(gnn, batch):
    """Float64 pre-activations (LN -> Linear) of the six modules."""
    net = copy.deepcopy(gnn).double()
    z, e, out = batch.z.double(), batch.e.double(), []
    with torch.no_grad():
        for layer in net.layers:
            hn = layer.node_module(z)
            msg = torch.cat([torch.cat([hn[batch.src],
                                        layer.edge_module(e)], -1),
                             torch.cat([hn, torch.zeros_like(hn)], -1)])
            out += [layer.node_module[:2](z), layer.edge_module[:2](e),
                    layer.reduce_module[:2](msg)]
            z = layer.forward(z, e, batch.src, batch.dst)
    return out


@functools.lru_cache(maxsize=None)
def _case(name):
    """(gnn, batch, upstream gradient) of a case.  No ReLU may sit within
    float32 rounding of its kink: every pre-activation is exactly zero or at
    least 1e-5 away from it, with no row excluded."""
    nodes, edges, seed = CASES[name]
    batch = _batch(nodes, edges, seed)
    if name == "two_nodes":                  # node 0 gets no mail
        batch.src[0], batch.dst[0] = 0, 1
    if name == "three_graphs":
        # in the last graph (nodes 18..50): in-degree 17 at node 18, edges 57
        # and 58 the same, a self loop at node 20, nothing leaves node 19
        batch.dst[40:57] = 18
        batch.src[58], batch.dst[58] = batch.src[57], batch.dst[57]
        batch.src[59] = batch.dst[59] = 20
        batch.src[batch.src == 19] = 21
        assert torch.bincount(batch.dst, minlength=51)[18] >= 17
    gnn = _gnn(seed)
    for pre in _preactivations(gnn, batch):
        assert bool(((pre.abs() >= 1e-5) | (pre == 0)).all()), name
    g = torch.Generator(device="cpu").manual_seed(seed + 100)
    return gnn, batch, torch.randn(len(nodes), 16, generator=g)


def _evaluate(gnn, batch, gout, dtype=torch.float32, dev="cpu", fused=False):
    """{quantity: float64 CPU tensor}: model_emb and the 24 gradients, from
    the kernels or from the plain chain in ``dtype``."""
    from ddls_amd.models.gnn import GraphBatch, _GNNTrunkFn, graph_mean
    net = copy.deepcopy(gnn).to(dev, dtype)
    b = GraphBatch(z=batch.z.to(dev, dtype), e=batch.e.to(dev, dtype),
                   src=batch.src.to(dev), dst=batch.dst.to(dev),
                   graph_of_node=batch.graph_of_node.to(dev),
                   num_graphs=batch.num_graphs)
    if fused:
        emb = _GNNTrunkFn.apply(b, *net.parameters())
    else:
        z = b.z
        for layer in net.layers:
            z = layer.forward(z, b.e, b.src, b.dst)
        emb = graph_mean(z, b)
    emb.backward(gout.to(dev, dtype))
    res = {"model_emb": emb}
    res.update({"g_" + n: p.grad for n, p in net.named_parameters()})
    return {k: v.detach().double().cpu() for k, v in res.items()}


@functools.lru_cache(maxsize=None)
def _references(name):
    case = _case(name)
    return _evaluate(*case, dtype=torch.float64), _evaluate(*case)


def _compare(truth, ref32, fused):
    assert len(fused) == 25
    assert all(torch.isfinite(v).all() for v in fused.values())
    _hold_to_float64_bound(truth, ref32, fused)
    for k, t in truth.items():       # exact zeros stay exact zeros
        both = (t == 0) & (ref32[k] == 0)
        assert torch.count_nonzero(fused[k][both]) == 0, k


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
def test_trunk_step_value_is_checked():
    from ddls_amd.rl.dqn import DQNConfig
    assert DQNConfig().trunk_step == "torch"
    with pytest.raises(ValueError):
        DQNConfig(trunk_step="bogus")


@pytest.mark.parametrize("name", list(CASES))
def test_case_seeds_keep_relus_off_their_kink(name):
    """The builder asserts it; the plan agrees with the batch."""
    _, batch, _ = _case(name)
    eo, srcp, dstp, indptr, sptr, slist, node_ptr = (
        t.long() for t in batch.trunk_plan())
    assert torch.equal(eo, batch.csr_by_dst()[0])
    assert torch.equal(srcp, batch.src[eo]) and torch.equal(dstp,
                                                            batch.dst[eo])
    assert torch.equal(torch.diff(node_ptr), torch.as_tensor(CASES[name][0]))
    assert torch.equal(torch.diff(sptr), torch.bincount(
        batch.src, minlength=batch.z.shape[0]))
    assert torch.equal(srcp[slist], torch.sort(batch.src).values)
    assert int(indptr[-1]) == len(eo)


def test_gnn_trunk_on_cpu_is_the_torch_chain():
    from ddls_amd.models.gnn import gnn_trunk, graph_mean
    gnn, batch, _ = _case("three_graphs")
    assert torch.equal(gnn_trunk(gnn, batch), graph_mean(gnn(batch), batch))


def test_fused_trunk_step_on_cpu_is_the_torch_chain(multi_model_files):
    from ddls_amd.models.gnn import GNNPolicy
    from ddls_amd.rl.dqn import DQNConfig, DQNTrainer
    from ddls_amd.rl.engine_env import EngineVectorEnv
    dev, params = torch.device("cpu"), {}
    for trunk_step in ("torch", "fused"):
        torch.manual_seed(4)
        policy = GNNPolicy(num_actions=17)
        venv = EngineVectorEnv(
            lambda: make_env(multi_model_files, "remove_and_repeat", 2, 3000,
                             15), num_envs=4, device=dev, base_seed=19)
        tr = DQNTrainer(venv, policy, DQNConfig(
            learning_starts=10, sgd_minibatch_size=8, lr=1e-4,
            learner="device", trunk_step=trunk_step), device=dev)
        torch.manual_seed(8)
        st = tr.update(tr.collect_rollout(8))
        assert st["learner"] == 1 and st["total_loss"] > 0
        assert st["trunk_step"] == 0
        params[trunk_step] = [p.detach().clone()
                              for p in tr.policy.parameters()]
    assert all(torch.equal(a, b)
               for a, b in zip(params["torch"], params["fused"]))


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_trunk_matches_float64_reference(name):
    truth, ref32 = _references(name)
    fused = _evaluate(*_case(name), dev="cuda:0", fused=True)
    _compare(truth, ref32, fused)
    if name == "one_node":           # no mail anywhere
        assert all(torch.count_nonzero(v) == 0 for v in fused.values())
    else:
        assert torch.count_nonzero(fused["model_emb"]) > 0


@pytest.mark.gpu
def test_trunk_on_engine_models_batch(multi_model_files):
    """The env's own static models batch, at its feature scales."""
    from ddls_amd.models.gnn import GraphBatch
    from ddls_amd.rl.engine_env import EngineVectorEnv
    venv = EngineVectorEnv(
        lambda: make_env(multi_model_files, "remove_and_repeat", 2, 3000, 15),
        num_envs=4, device=torch.device("cuda:0"), base_seed=23)
    mb = venv._models_batch
    batch = GraphBatch(z=mb.z.cpu(), e=mb.e.cpu(), src=mb.src.cpu(),
                       dst=mb.dst.cpu(), graph_of_node=mb.graph_of_node.cpu(),
                       num_graphs=mb.num_graphs)
    g = torch.Generator(device="cpu").manual_seed(7)
    case = (_gnn(7), batch, torch.randn(mb.num_graphs, 16, generator=g))
    _compare(_evaluate(*case, dtype=torch.float64), _evaluate(*case),
             _evaluate(*case, dev="cuda:0", fused=True))


@pytest.mark.gpu
def test_trunk_is_reproducible():
    case = _case("five_graphs")
    a = _evaluate(*case, dev="cuda:0", fused=True)
    b = _evaluate(*case, dev="cuda:0", fused=True)
    assert len(a) == 25 and all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.gpu
def test_trunk_rejects_another_shape():
    from ddls_amd.models.gnn import DEFAULT_GNN_CONFIG, GNN, _GNNTrunkFn
    gnn = GNN(dict(DEFAULT_GNN_CONFIG, out_features_hidden=32)).to("cuda:0")
    assert not gnn._trunk_ok
    _, batch, _ = _case("two_nodes")
    b = copy.copy(batch)
    b.z, b.e, b._trunk = batch.z.cuda(), batch.e.cuda(), None
    with pytest.raises(RuntimeError, match="gnn_trunk"):
        _GNNTrunkFn.apply(b, *gnn.parameters())


@pytest.mark.gpu
@pytest.mark.parametrize("head_step", ["torch", "fused"])
def test_trainer_with_fused_trunk_step(multi_model_files, head_step):
    from ddls_amd.models.gnn import GNNPolicy
    from ddls_amd.rl.dqn import DQNConfig, DQNTrainer
    from ddls_amd.rl.engine_env import EngineVectorEnv
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    venv = EngineVectorEnv(
        lambda: make_env(multi_model_files, "remove_and_repeat", 2, 3000, 15),
        num_envs=16, device=dev, base_seed=23)
    cfg = DQNConfig(learning_starts=50, sgd_minibatch_size=32, num_sgd_iter=2,
                    lr=1e-4, learner="device", head_step=head_step,
                    trunk_step="fused")
    tr = DQNTrainer(venv, GNNPolicy(num_actions=17).to(dev), cfg, device=dev)
    before = [p.detach().clone() for p in tr.policy.gnn.parameters()]
    for _ in range(2):
        st = tr.train(num_steps=8)
        assert st["learner"] == 1 and st["trunk_step"] == 1
        assert st["head_step"] == int(head_step == "fused")
        assert all(np.isfinite(v) for v in st.values())
    assert st["total_loss"] > 0
    assert any(not torch.equal(a, b)
               for a, b in zip(before, tr.policy.gnn.parameters()))
