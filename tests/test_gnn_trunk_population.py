"""Population GNN trunk (ops/hip/gnn_trunk.hip ``gt_pop_fwd_kernel``,
models/gnn.py ``gnn_trunk_population``, rl/es_population.py
``trunk="fused"``): every member against the plain torch chain
``MeanPoolLayer.forward`` x 2 + ``graph_mean`` in float64 on the CPU with that
member's weights, and bit for bit against ``gnn_trunk_fwd``.

Row ``m`` of ``pop`` is ``_gnn(seed + m)`` flattened plus 37 random floats:
n = 4183 is odd, so rows are unaligned and the stride is not the trunk's."""
import copy
import functools

import pytest
import torch

from tests.test_dqn_head_step import _hold_to_float64_bound
from tests.test_gnn_trunk import CASES, _case, _gnn
from tests.test_vec_engine import make_env, multi_model_files  # noqa: F401

TAIL = 37


def _flat(module):
    return torch.cat([p.detach().reshape(-1) for p in module.parameters()])


@functools.lru_cache(maxsize=None)
def _members(name, P):
    """(the P GNNs, pop [P, 4183]) of a case.  Read-only."""
    seed = CASES[name][2]
    gnns = [_gnn(seed + m) for m in range(P)]
    g = torch.Generator(device="cpu").manual_seed(seed)
    pop = torch.stack([torch.cat([_flat(n), torch.randn(TAIL, generator=g)])
                       for n in gnns])
    return gnns, pop


def _gnn_of(flat):
    """The tuned GNN holding the first 4146 values of ``flat``."""
    gnn, off = _gnn(0), 0
    with torch.no_grad():
        for p in gnn.parameters():
            p.copy_(flat[off:off + p.numel()].view(p.shape))
            off += p.numel()
    return gnn


def _chain(gnns, batch, dtype):
    """Stacked plain chain in ``dtype`` on the CPU, as float64 [P, G, 16]."""
    from ddls_amd.models.gnn import graph_mean
    b = copy.copy(batch)
    b.z, b.e = batch.z.to(dtype), batch.e.to(dtype)
    out = []
    with torch.no_grad():
        for gnn in gnns:
            z = b.z
            for layer in copy.deepcopy(gnn).to(dtype).layers:
                z = layer.forward(z, b.e, b.src, b.dst)
            out.append(graph_mean(z, b).double())
    return torch.stack(out)


def _on(batch, dev):
    from ddls_amd.models.gnn import GraphBatch
    return GraphBatch(*(t.to(dev) for t in (batch.z, batch.e, batch.src,
                                            batch.dst, batch.graph_of_node)),
                      num_graphs=batch.num_graphs)


def _es_trainer(venv, dev, trunk):
    from ddls_amd.models.gnn import GNNPolicy
    from ddls_amd.rl.es import ESConfig, ESTrainer
    torch.manual_seed(4)
    return ESTrainer(venv, GNNPolicy(num_actions=17), ESConfig(
        evaluator="population", perturbation_pairs=2, envs_per_member=2,
        eval_max_steps=6, noise_seed=3, population_trunk=trunk), device=dev)


def _venv(jobs_dir, dev, base_seed):
    from ddls_amd.rl.engine_env import EngineVectorEnv
    return EngineVectorEnv(
        lambda: make_env(jobs_dir, "remove_and_repeat", 2, 3000, 15),
        num_envs=2, device=torch.device(dev), base_seed=base_seed)


def test_population_on_cpu_is_the_stacked_torch_chain():
    from ddls_amd.models.gnn import gnn_trunk_population, graph_mean
    batch = _case("three_graphs")[1]
    gnns, pop = _members("three_graphs", 3)
    with torch.no_grad():
        want = torch.stack([graph_mean(n(batch), batch) for n in gnns])
    assert torch.equal(gnn_trunk_population(pop, batch), want)
    shifted = torch.cat([pop[:, -5:], pop], dim=1)
    assert torch.equal(gnn_trunk_population(shifted, batch, offset=5), want)
    with pytest.raises(ValueError, match="gnn_trunk_population"):
        gnn_trunk_population(pop[:, :4000], batch)


def test_population_trunk_value_is_checked():
    from ddls_amd.rl.es import ESConfig
    assert ESConfig().population_trunk == "torch"
    with pytest.raises(ValueError):
        ESConfig(population_trunk="bogus")


def test_fused_population_trunk_on_cpu_is_the_torch_loop(multi_model_files):
    ends = {}
    for trunk in ("torch", "fused"):
        tr = _es_trainer(_venv(multi_model_files, "cpu", 19),
                         torch.device("cpu"), trunk)
        for _ in range(2):
            st = tr.train()
            assert st["evaluator"] == 1 and st["population_trunk"] == 0
        ends[trunk] = tr._get_flat().numpy().tobytes()
    assert ends["torch"] == ends["fused"]


@pytest.mark.gpu
@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("name", list(CASES))
def test_population_matches_float64_reference(name, P):
    from ddls_amd.models.gnn import _GNNTrunkFn, gnn_trunk_population
    batch = _case(name)[1]
    gnns, pop = _members(name, P)
    b = _on(batch, "cuda:0")
    emb = gnn_trunk_population(pop.cuda(), b)
    assert emb.shape == (P, batch.num_graphs, 16) and emb.dtype == torch.float32
    _hold_to_float64_bound({"model_emb": _chain(gnns, batch, torch.float64)},
                           {"model_emb": _chain(gnns, batch, torch.float32)},
                           {"model_emb": emb.double().cpu()})
    for m, gnn in enumerate(gnns):
        one = _GNNTrunkFn.apply(b, *[p.detach().cuda()
                                     for p in gnn.parameters()])
        assert torch.equal(emb[m], one), m
        if name == "one_node":           # no mail anywhere
            assert torch.count_nonzero(emb[m]) == 0
        else:
            assert torch.count_nonzero(emb[m]) > 0


@pytest.mark.gpu
def test_evaluator_embeddings_with_fused_trunk(multi_model_files):
    from ddls_amd.models.gnn import GNNPolicy
    from ddls_amd.rl.es_population import PopulationEvaluator
    venv = _venv(multi_model_files, "cuda:0", 23)
    torch.manual_seed(4)
    policy = GNNPolicy(num_actions=17).to(venv.device)
    ev = PopulationEvaluator(venv, policy, perturbation_pairs=2,
                             envs_per_member=2, eval_max_steps=6,
                             trunk="fused")
    assert ev.fused_trunk
    _, pop = ev.perturb(_flat(policy), 0.1, 0)
    emb = ev.embeddings(pop)
    assert emb.shape[0] == 4 and emb.is_contiguous()
    assert torch.equal(emb, ev.embeddings(pop))
    batch = _on(venv._models_batch, "cpu")
    gnns = [_gnn_of(row) for row in pop.cpu()]
    _hold_to_float64_bound({"model_emb": _chain(gnns, batch, torch.float64)},
                           {"model_emb": _chain(gnns, batch, torch.float32)},
                           {"model_emb": emb.double().cpu()})


@pytest.mark.gpu
def test_trainer_with_fused_population_trunk(multi_model_files):
    dev, ends = torch.device("cuda:0"), []
    for _ in range(2):
        tr = _es_trainer(_venv(multi_model_files, dev, 23), dev, "fused")
        before = tr._get_flat().clone()
        for _g in range(2):
            st = tr.train()
            assert st["evaluator"] == 1 and st["population_trunk"] == 1
        assert not torch.equal(before, tr._get_flat())
        ends.append(tr._get_flat().cpu().numpy().tobytes())
    assert ends[0] == ends[1]
