"""PAC-ML GNN policy, batched.

Reference: ``ddls/ml_models/models/mean_pool.py:5`` (MeanPool),
``models/gnn.py:5`` (GNN stack), ``policies/gnn_policy.py:53`` (GNNPolicy).

The reference builds one DGL graph per sample in a Python loop
(``gnn_policy.py:226-253``) — the training hot spot.  This
rebuild batches the whole minibatch into one flat edge list (global node
indices + per-node graph ids) and runs message passing with gather/segment
ops, a layout chosen so the fused HIP/MFMA kernel (ddls_amd.ops) can replace
the inner loop 1:1.

Semantics parity notes:
- message = concat(node_mlp(z_src), edge_mlp(e)); the receiving node adds a
  self-message concat(node_mlp(z_v), zeros).
- every message goes through reduce_mlp (LayerNorm -> Linear -> act) BEFORE
  the mean (mean of MLP, not MLP of mean).
- DGL's update_all zero-fills nodes with no in-edges (the self-message is only
  added for nodes that receive mail); replicated here.
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Dict, List, Optional

import numpy as np
import torch
import torch.nn as nn

ACTIVATIONS = {
    "relu": nn.ReLU,
    "leaky_relu": nn.LeakyReLU,
    "tanh": nn.Tanh,
    "elu": nn.ELU,
    "sigmoid": nn.Sigmoid,
}

DEFAULT_GNN_CONFIG = {
    # tuned values from the reference (scripts/.../model/gnn.yaml:16-35)
    "in_features_node": 5,
    "in_features_edge": 2,
    "in_features_graph": 17,
    "out_features_msg": 32,
    "out_features_hidden": 64,
    "out_features_node": 16,
    "out_features_graph": 8,
    "num_rounds": 2,
    "aggregator_activation": "relu",
    "module_depth": 1,
    "fcnet_hiddens": [256],
    "fcnet_activation": "relu",
    "apply_action_mask": True,
}


@dataclass
class GraphBatch:
    """Flat batch of variable-size graphs."""
    z: torch.Tensor            # [N_total, F_node]
    e: torch.Tensor            # [E_total, F_edge]
    src: torch.Tensor          # [E_total] global node indices
    dst: torch.Tensor          # [E_total]
    graph_of_node: torch.Tensor  # [N_total] graph id per node
    num_graphs: int
    _csr: Optional[tuple] = None
    _node_ptr: Optional[torch.Tensor] = None
    _trunk: Optional[tuple] = None

    def csr_by_dst(self):
        """(edge_order, indptr) with edges sorted by destination node —
        the segment layout the HIP message_reduce kernel consumes."""
        if self._csr is None:
            n = self.z.shape[0]
            order = torch.argsort(self.dst, stable=True)
            counts = torch.bincount(self.dst, minlength=n)
            indptr = torch.zeros(n + 1, dtype=torch.int64, device=self.z.device)
            torch.cumsum(counts, 0, out=indptr[1:])
            self._csr = (order, indptr)
        return self._csr

    def node_ptr(self):
        """[G+1] prefix over nodes grouped by graph id (nodes are stored
        graph-contiguously by construction)."""
        if self._node_ptr is None:
            counts = torch.bincount(self.graph_of_node,
                                    minlength=self.num_graphs)
            ptr = torch.zeros(self.num_graphs + 1, dtype=torch.int64,
                              device=self.z.device)
            torch.cumsum(counts, 0, out=ptr[1:])
            self._node_ptr = ptr
        return self._node_ptr

    def trunk_plan(self):
        """The int32 index plan of the gnn_trunk kernels, built and validated
        on the host once (one sync; the batch is static): ``(eo, srcp, dstp,
        indptr, sptr, slist, node_ptr)``.  ``eo`` is the stable CSR-by-dst
        edge order of ``csr_by_dst()`` and ``indptr`` its row pointer;
        ``srcp`` / ``dstp`` are ``src`` / ``dst`` in that order; ``sptr`` /
        ``slist`` are a CSR by source over the positions of that order."""
        if self._trunk is None:
            n, E, G = self.z.shape[0], self.src.shape[0], self.num_graphs
            src = self.src.detach().cpu().numpy().astype(np.int64)
            dst = self.dst.detach().cpu().numpy().astype(np.int64)
            gon = self.graph_of_node.detach().cpu().numpy().astype(np.int64)
            if n < 1 or G < 1 or gon.shape[0] != n or self.e.shape[0] != E:
                raise ValueError("gnn_trunk: the batch needs nodes, graphs "
                                 "and one feature row per node and edge")
            if gon.min() < 0 or gon.max() >= G or np.any(np.diff(gon) < 0):
                raise ValueError("gnn_trunk: nodes must be stored "
                                 "graph-contiguously with ids in [0, G)")
            if E and (min(src.min(), dst.min()) < 0
                      or max(src.max(), dst.max()) >= n):
                raise ValueError("gnn_trunk: an edge names a node outside "
                                 "[0, N)")
            if np.any(gon[src] != gon[dst]):
                raise ValueError("gnn_trunk: an edge joins two graphs")
            eo = np.argsort(dst, kind="stable")
            srcp, dstp = src[eo], dst[eo]
            slist = np.argsort(srcp, kind="stable")

            def ptr(ids, size):
                out = np.zeros(size + 1, dtype=np.int64)
                np.cumsum(np.bincount(ids, minlength=size), out=out[1:])
                return out
            plan = (eo, srcp, dstp, ptr(dst, n), ptr(src, n), slist,
                    ptr(gon, G))
            self._trunk = tuple(
                torch.as_tensor(a.astype(np.int32), device=self.z.device)
                for a in plan)
        return self._trunk

    @staticmethod
    def from_padded(node_features: torch.Tensor,
                    edge_features: torch.Tensor,
                    edges_src: torch.Tensor,
                    edges_dst: torch.Tensor,
                    node_split: torch.Tensor,
                    edge_split: torch.Tensor) -> "GraphBatch":
        """Strip zero-padding and concatenate into one flat graph.

        All tensors batched [B, ...]; node_split/edge_split give the true
        counts per sample (reference obs fields of the same names).
        """
        B, Nmax = node_features.shape[0], node_features.shape[1]
        Emax = edge_features.shape[1]
        device = node_features.device
        ns = node_split.reshape(B).long()
        es = edge_split.reshape(B).long()
        node_mask = torch.arange(Nmax, device=device)[None, :] < ns[:, None]
        edge_mask = torch.arange(Emax, device=device)[None, :] < es[:, None]
        z = node_features[node_mask]
        e = edge_features[edge_mask]
        offsets = torch.cumsum(ns, 0) - ns
        src = (edges_src.long() + offsets[:, None])[edge_mask]
        dst = (edges_dst.long() + offsets[:, None])[edge_mask]
        graph_of_node = torch.repeat_interleave(
            torch.arange(B, device=device), ns)
        return GraphBatch(z=z, e=e, src=src, dst=dst,
                          graph_of_node=graph_of_node, num_graphs=B)


class _FusedMeanPoolFn(torch.autograd.Function):
    """Fused HIP forward+backward of one MeanPool layer (training path on
    MI355X; kernels in ddls_amd/ops/hip/meanpool.hip + meanpool_bwd.hip)."""

    @staticmethod
    def forward(ctx, z, e, src, dst, edge_order, indptr,
                ln_n_w, ln_n_b, W_n, b_n,
                ln_e_w, ln_e_b, W_e, b_e,
                ln_r_w, ln_r_b, W_r, b_r):
        from .. import ops as hip_ops
        ext = hip_ops.get_extension(required=True)
        zc, ec = z.contiguous(), e.contiguous()
        Wn, We, Wr = W_n.contiguous(), W_e.contiguous(), W_r.contiguous()
        half, out_dim = W_n.shape[0], W_r.shape[0]
        use_mfma = (half == 16 and W_r.shape[1] == 32 and out_dim % 16 == 0
                    and out_dim <= 64 and zc.shape[1] <= 64
                    and ec.shape[1] <= 64
                    and os.environ.get("DDLS_AMD_DISABLE_MFMA", "0") != "1")
        if use_mfma:
            # matrix-core forward: the MLP contractions on
            # v_mfma_f32_16x16x4_f32 tiles, then a light CSR combine
            hn = ext.row_mlp_mfma(zc, ln_n_w, ln_n_b, Wn, b_n)
            he = ext.row_mlp_mfma(ec, ln_e_w, ln_e_b, We, b_e)
            r_edge, r_self = ext.message_mlp_mfma(
                hn, he, src, ln_r_w, ln_r_b, Wr, b_r)
            out = ext.segment_combine(r_edge, r_self, edge_order, indptr)
        else:
            hn = ext.row_mlp(zc, ln_n_w, ln_n_b, Wn, b_n)
            he = ext.row_mlp(ec, ln_e_w, ln_e_b, We, b_e)
            out, r_edge, r_self = ext.message_reduce_train(
                hn, he, src, edge_order, indptr, ln_r_w, ln_r_b, Wr, b_r)
        ctx.save_for_backward(zc, ec, src, dst, indptr, hn, he, r_edge, r_self,
                              ln_n_w, ln_n_b, Wn, ln_e_w, ln_e_b, We,
                              ln_r_w, ln_r_b, Wr)
        ctx.use_mfma = use_mfma
        return out

    @staticmethod
    def backward(ctx, gout):
        from .. import ops as hip_ops
        ext = hip_ops.get_extension(required=True)
        (z, e, src, dst, indptr, hn, he, r_edge, r_self,
         ln_n_w, ln_n_b, W_n, ln_e_w, ln_e_b, W_e,
         ln_r_w, ln_r_b, W_r) = ctx.saved_tensors
        if (ctx.use_mfma and hasattr(ext, "message_reduce_bwd_mfma")
                and os.environ.get("DDLS_AMD_DISABLE_MFMA_BWD", "0") != "1"):
            ghn, ghe, gWr, gbr, glnr_g, glnr_b = ext.message_reduce_bwd_mfma(
                hn, he, src, dst, indptr, ln_r_w, ln_r_b, W_r, r_edge, r_self,
                gout.contiguous())
        else:
            ghn, ghe, gWr, gbr, glnr_g, glnr_b = ext.message_reduce_bwd(
                hn, he, src, dst, indptr, ln_r_w, ln_r_b, W_r, r_edge, r_self,
                gout.contiguous())
        gz, gWn, gbn, glnn_g, glnn_b = ext.row_mlp_bwd(
            z, hn, ghn, ln_n_w, ln_n_b, W_n)
        ge, gWe, gbe, glne_g, glne_b = ext.row_mlp_bwd(
            e, he, ghe, ln_e_w, ln_e_b, W_e)
        return (gz, ge, None, None, None, None,
                glnn_g, glnn_b, gWn, gbn,
                glne_g, glne_b, gWe, gbe,
                glnr_g, glnr_b, gWr, gbr)


def _mlp(in_dim: int, out_dim: int, act, depth: int,
         input_act: bool = True) -> nn.Sequential:
    layers: List[nn.Module] = [nn.LayerNorm(in_dim), nn.Linear(in_dim, out_dim)]
    if input_act:
        layers.append(act())
    for _ in range(depth - 1):
        layers.extend([nn.Linear(out_dim, out_dim), act()])
    return nn.Sequential(*layers)


class MeanPoolLayer(nn.Module):
    """One message-passing round (reference ``mean_pool.py:5-150``)."""

    def __init__(self, in_features_node: int, in_features_edge: int,
                 out_features_msg: int, out_features_reduce: int,
                 aggregator_activation: str = "leaky_relu",
                 module_depth: int = 1):
        super().__init__()
        if module_depth < 1:
            raise ValueError("module_depth must be >= 1")
        act = ACTIVATIONS[aggregator_activation]
        half = out_features_msg // 2
        self.node_module = _mlp(in_features_node, half, act, module_depth)
        self.edge_module = _mlp(in_features_edge, half, act, module_depth)
        self.reduce_module = _mlp(out_features_msg, out_features_reduce, act,
                                  module_depth)
        self.out_features_msg = out_features_msg
        self.out_features_reduce = out_features_reduce
        # the fused HIP kernels implement the tuned LN->Linear->ReLU depth-1
        # structure; other configs take the torch path
        self._hip_eligible = (module_depth == 1
                              and aggregator_activation == "relu")

    def forward_batch(self, z: torch.Tensor, batch: "GraphBatch") -> torch.Tensor:
        from .. import ops as hip_ops
        if self._hip_eligible and hip_ops.hip_ops_enabled_for(z):
            return self._forward_hip(z, batch)
        if (self._hip_eligible and z.is_cuda and torch.is_grad_enabled()
                and hip_ops.get_extension() is not None
                and os.environ.get("DDLS_AMD_DISABLE_HIP", "0") != "1"):
            # fused HIP forward+backward training path
            order, indptr = batch.csr_by_dst()
            ln_n, lin_n = self.node_module[0], self.node_module[1]
            ln_e, lin_e = self.edge_module[0], self.edge_module[1]
            ln_r, lin_r = self.reduce_module[0], self.reduce_module[1]
            return _FusedMeanPoolFn.apply(
                z, batch.e, batch.src, batch.dst, order, indptr,
                ln_n.weight, ln_n.bias, lin_n.weight, lin_n.bias,
                ln_e.weight, ln_e.bias, lin_e.weight, lin_e.bias,
                ln_r.weight, ln_r.bias, lin_r.weight, lin_r.bias)
        return self.forward(z, batch.e, batch.src, batch.dst)

    def _forward_hip(self, z: torch.Tensor, batch: "GraphBatch") -> torch.Tensor:
        from .. import ops as hip_ops
        ext = hip_ops.get_extension(required=True)
        ln_n, lin_n = self.node_module[0], self.node_module[1]
        ln_e, lin_e = self.edge_module[0], self.edge_module[1]
        ln_r, lin_r = self.reduce_module[0], self.reduce_module[1]
        zc, ec = z.contiguous(), batch.e.contiguous()
        Wn = lin_n.weight.contiguous()
        We = lin_e.weight.contiguous()
        Wr = lin_r.weight.contiguous()
        order, indptr = batch.csr_by_dst()
        half, out_dim = Wn.shape[0], Wr.shape[0]
        if (half == 16 and Wr.shape[1] == 32 and out_dim % 16 == 0
                and out_dim <= 64 and zc.shape[1] <= 64 and ec.shape[1] <= 64
                and os.environ.get("DDLS_AMD_DISABLE_MFMA", "0") != "1"):
            # matrix-core inference path (v_mfma_f32_16x16x4_f32 tiles) —
            # the rollout embedding cache runs through here every iteration
            hn = ext.row_mlp_mfma(zc, ln_n.weight, ln_n.bias, Wn, lin_n.bias)
            he = ext.row_mlp_mfma(ec, ln_e.weight, ln_e.bias, We, lin_e.bias)
            r_edge, r_self = ext.message_mlp_mfma(
                hn, he, batch.src, ln_r.weight, ln_r.bias, Wr, lin_r.bias)
            return ext.segment_combine(r_edge, r_self, order, indptr)
        hn = ext.row_mlp(zc, ln_n.weight, ln_n.bias, Wn, lin_n.bias)
        he = ext.row_mlp(ec, ln_e.weight, ln_e.bias, We, lin_e.bias)
        return ext.message_reduce(hn, he, batch.src, order, indptr,
                                  ln_r.weight, ln_r.bias, Wr, lin_r.bias)

    def forward(self, z: torch.Tensor, e: torch.Tensor, src: torch.Tensor,
                dst: torch.Tensor) -> torch.Tensor:
        N = z.shape[0]
        hn = self.node_module(z)                       # [N, msg/2]
        he = self.edge_module(e)                       # [E, msg/2]
        msg_edge = torch.cat([hn[src], he], dim=-1)    # [E, msg]
        msg_self = torch.cat([hn, torch.zeros_like(hn)], dim=-1)  # [N, msg]
        r_edge = self.reduce_module(msg_edge)          # [E, out]
        r_self = self.reduce_module(msg_self)          # [N, out]
        out = torch.zeros(N, r_self.shape[-1], dtype=r_edge.dtype,
                          device=z.device)
        out.index_add_(0, dst, r_edge)
        in_deg = torch.zeros(N, dtype=z.dtype, device=z.device)
        in_deg.index_add_(0, dst, torch.ones_like(dst, dtype=z.dtype))
        has_mail = in_deg > 0
        total = out + r_self
        count = (in_deg + 1).unsqueeze(-1)
        mean = total / count
        # DGL zero-fills nodes with no incoming messages
        return torch.where(has_mail.unsqueeze(-1), mean,
                           torch.zeros_like(mean))


class GNN(nn.Module):
    """Stack of >= 2 MeanPool rounds (reference ``models/gnn.py:5-89``)."""

    def __init__(self, config: Dict):
        super().__init__()
        if config["num_rounds"] < 2:
            raise ValueError("num_rounds must be >= 2")
        layers = [MeanPoolLayer(config["in_features_node"],
                                config["in_features_edge"],
                                config["out_features_msg"],
                                config["out_features_hidden"],
                                config["aggregator_activation"],
                                config["module_depth"])]
        for _ in range(config["num_rounds"] - 2):
            layers.append(MeanPoolLayer(config["out_features_hidden"],
                                        config["in_features_edge"],
                                        config["out_features_msg"],
                                        config["out_features_hidden"],
                                        config["aggregator_activation"],
                                        config["module_depth"]))
        layers.append(MeanPoolLayer(config["out_features_hidden"],
                                    config["in_features_edge"],
                                    config["out_features_msg"],
                                    config["out_features_node"],
                                    config["aggregator_activation"],
                                    config["module_depth"]))
        self.layers = nn.ModuleList(layers)

        # gnn_trunk eligibility (ops/hip/gnn_trunk.hip is built for the tuned
        # PAC-ML GNN shape)
        self._trunk_ok = (
            config["num_rounds"] == 2 and config["module_depth"] == 1
            and config["aggregator_activation"] == "relu"
            and config["in_features_node"] == 5
            and config["in_features_edge"] == 2
            and config["out_features_msg"] == 32
            and config["out_features_hidden"] == 64
            and config["out_features_node"] == 16)

    def forward(self, batch: GraphBatch) -> torch.Tensor:
        z = batch.z
        for layer in self.layers:
            z = layer.forward_batch(z, batch)
        return z


class _FusedHeadFn(torch.autograd.Function):
    """Fused policy/value head (ops/hip/policy_head.hip): LN(graph feats) ->
    graph MLP -> concat(pooled node emb) -> both FC branches + action mask,
    one kernel each way — replaces ~8 rocBLAS GEMMs and ~30 elementwise
    kernels per captured replay.  graph_features and mask need no grad."""

    @staticmethod
    def forward(ctx, gm, gf, mask, ln_w, ln_b, Wg, bg,
                W1p, b1p, W2p, b2p, W1v, b1v, W2v, b2v):
        from .. import ops as hip_ops
        ext = hip_ops.get_extension(required=True)
        logits, value, emb, h1p, h1v = ext.head_fwd(
            gm.contiguous(), gf.contiguous(), mask.contiguous(),
            ln_w, ln_b, Wg.contiguous(), bg, W1p.contiguous(), b1p,
            W2p.contiguous(), b2p, W1v.contiguous(), b1v,
            W2v.contiguous(), b2v)
        ctx.save_for_backward(gf, emb, h1p, h1v, ln_w, ln_b, Wg,
                              W1p, W2p, W1v, W2v)
        return logits, value

    @staticmethod
    def backward(ctx, glogits, gvalue):
        from .. import ops as hip_ops
        ext = hip_ops.get_extension(required=True)
        (gf, emb, h1p, h1v, ln_w, ln_b, Wg, W1p, W2p, W1v, W2v) = \
            ctx.saved_tensors
        (ggm, gln_w, gln_b, gWg, gbg, gW1p, gb1p, gW2p, gb2p,
         gW1v, gb1v, gW2v, gb2v) = ext.head_bwd(
            gf, emb, h1p, h1v, glogits.contiguous(), gvalue.contiguous(),
            ln_w, ln_b, Wg.contiguous(), W1p.contiguous(), W2p.contiguous(),
            W1v.contiguous(), W2v.contiguous())
        return (ggm, None, None, gln_w, gln_b, gWg, gbg,
                gW1p, gb1p, gW2p, gb2p, gW1v, gb1v, gW2v, gb2v)


class _SegmentMeanFn(torch.autograd.Function):
    """HIP per-graph mean with a broadcast/scale backward (replaces the
    torch index_add path, which costs ~100us per minibatch on MI355X)."""

    @staticmethod
    def forward(ctx, x, node_ptr, G):
        from .. import ops as hip_ops
        ext = hip_ops.get_extension(required=True)
        out = ext.segment_mean(x.contiguous(), node_ptr, G)
        ctx.save_for_backward(node_ptr)
        ctx.N = x.shape[0]
        return out

    @staticmethod
    def backward(ctx, gout):
        from .. import ops as hip_ops
        ext = hip_ops.get_extension(required=True)
        (node_ptr,) = ctx.saved_tensors
        return ext.segment_mean_bwd(gout.contiguous(), node_ptr,
                                    ctx.N), None, None


def graph_mean(node_emb: torch.Tensor, batch: GraphBatch) -> torch.Tensor:
    """Per-graph mean of node embeddings (HIP segment kernel on GPU)."""
    from .. import ops as hip_ops
    if (node_emb.is_cuda and torch.is_grad_enabled()
            and node_emb.requires_grad
            and hip_ops.get_extension() is not None
            and hasattr(hip_ops.get_extension(), "segment_mean_bwd")
            and os.environ.get("DDLS_AMD_DISABLE_HIP", "0") != "1"):
        return _SegmentMeanFn.apply(node_emb, batch.node_ptr(),
                                    batch.num_graphs)
    if hip_ops.hip_ops_enabled_for(node_emb):
        ext = hip_ops.get_extension(required=True)
        return ext.segment_mean(node_emb.contiguous(), batch.node_ptr(),
                                batch.num_graphs)
    B = batch.num_graphs
    sums = torch.zeros(B, node_emb.shape[-1], dtype=node_emb.dtype,
                       device=node_emb.device)
    sums.index_add_(0, batch.graph_of_node, node_emb)
    counts = torch.zeros(B, dtype=node_emb.dtype, device=node_emb.device)
    counts.index_add_(0, batch.graph_of_node,
                      torch.ones_like(batch.graph_of_node, dtype=node_emb.dtype))
    return sums / counts.clamp(min=1).unsqueeze(-1)


class _GNNTrunkFn(torch.autograd.Function):
    """The whole GNN trunk, ``graph_mean(gnn(batch), batch)``, as the kernels
    of ops/hip/gnn_trunk.hip: one launch forward, two backward.  Inputs are
    the batch (a constant: ``z`` and ``e`` get no gradient) and the 24
    tensors of ``gnn.parameters()``; the output is ``[G, 16]``."""

    @staticmethod
    def forward(ctx, batch, *params):
        from .. import ops as hip_ops
        ext = hip_ops.get_extension(required=True)
        plan = list(batch.trunk_plan())
        params_c = [p.detach().contiguous() for p in params]
        emb, workspace = ext.gnn_trunk_fwd(
            batch.z.detach().contiguous(), batch.e.detach().contiguous(),
            plan, params_c)
        ctx.save_for_backward(workspace, *plan, *params_c)
        return emb

    @staticmethod
    def backward(ctx, gemb):
        from .. import ops as hip_ops
        ext = hip_ops.get_extension(required=True)
        saved = ctx.saved_tensors
        grads = ext.gnn_trunk_bwd(gemb.contiguous(), saved[0],
                                  list(saved[1:8]), list(saved[8:]))
        return (None,) + tuple(grads)


def gnn_trunk(gnn: GNN, batch: GraphBatch) -> torch.Tensor:
    """Per-graph mean node embedding ``[G, out_node]`` of ``gnn`` on
    ``batch``.  An eligible GNN (``gnn._trunk_ok``) on a GPU runs the fused
    trunk kernels, forward and backward; anything else is the torch chain
    ``graph_mean(gnn(batch), batch)``, which is also the kernels' oracle."""
    if (getattr(gnn, "_trunk_ok", False) and batch.z.is_cuda
            and os.environ.get("DDLS_AMD_DISABLE_HIP", "0") != "1"):
        return _GNNTrunkFn.apply(batch, *gnn.parameters())
    return graph_mean(gnn(batch), batch)


class GNNPolicy(nn.Module):
    """GNN -> per-graph mean node embedding ++ graph-feature embedding ->
    policy logits + value (reference ``gnn_policy.py:53-276``; the FC head
    mirrors RLlib's FullyConnectedNetwork with a separate value branch)."""

    def __init__(self, num_actions: int, config: Optional[Dict] = None):
        super().__init__()
        cfg = dict(DEFAULT_GNN_CONFIG)
        if config:
            cfg.update(config)
        self.config = cfg
        self.num_actions = num_actions
        self.gnn = GNN(cfg)

        act = ACTIVATIONS[cfg["aggregator_activation"]]
        # graph module input = graph feats + action mask (appended by the obs fn)
        in_graph = cfg["in_features_graph"] + num_actions
        graph_layers: List[nn.Module] = [nn.LayerNorm(in_graph),
                                         nn.Linear(in_graph, cfg["out_features_graph"])]
        for _ in range(cfg["module_depth"] - 1):
            graph_layers.extend([nn.Linear(cfg["out_features_graph"],
                                           cfg["out_features_graph"]), act()])
        self.graph_module = nn.Sequential(*graph_layers)

        emb_dim = cfg["out_features_graph"] + cfg["out_features_node"]
        fc_act = ACTIVATIONS[cfg["fcnet_activation"]]
        hiddens = cfg["fcnet_hiddens"]

        def branch(out_dim):
            layers, d = [], emb_dim
            for h in hiddens:
                layers.extend([nn.Linear(d, h), fc_act()])
                d = h
            layers.append(nn.Linear(d, out_dim))
            return nn.Sequential(*layers)

        self.policy_branch = branch(num_actions)
        self.value_branch = branch(1)
        # fused-head eligibility (policy_head.hip is built for the tuned
        # PAC-ML head shape)
        self._fused_head_ok = (
            cfg["module_depth"] == 1 and hiddens == [256]
            and cfg["fcnet_activation"] == "relu"
            and cfg["apply_action_mask"]
            and cfg["out_features_graph"] == 8
            and cfg["out_features_node"] == 16
            and num_actions <= 32 and in_graph <= 64)

    def forward_flat(self, batch: GraphBatch, graph_features: torch.Tensor,
                     action_mask: torch.Tensor):
        """Forward on a pre-collated flat batch (the rollout/SGD hot path)."""
        node_emb = self.gnn(batch)                      # [N_total, out_node]
        graph_node_emb = graph_mean(node_emb, batch)    # [B, out_node]
        # opt-in: measured slightly SLOWER than the rocBLAS GEMM path at the
        # tuned head shape (A/B on one box: update 57 ms vs 49 ms per iter) —
        # kept for larger heads / kernel-count-sensitive deployments
        if (self._fused_head_ok and graph_node_emb.is_cuda
                and torch.is_grad_enabled() and graph_node_emb.requires_grad
                and os.environ.get("DDLS_AMD_ENABLE_FUSED_HEAD", "0") == "1"):
            from .. import ops as hip_ops
            ext = hip_ops.get_extension()
            if ext is not None and hasattr(ext, "head_fwd"):
                ln, lin_g = self.graph_module[0], self.graph_module[1]
                pb, vb = self.policy_branch, self.value_branch
                return _FusedHeadFn.apply(
                    graph_node_emb, graph_features, action_mask,
                    ln.weight, ln.bias, lin_g.weight, lin_g.bias,
                    pb[0].weight, pb[0].bias, pb[2].weight, pb[2].bias,
                    vb[0].weight, vb[0].bias, vb[2].weight, vb[2].bias)
        graph_emb = self.graph_module(graph_features)
        final_emb = torch.cat([graph_node_emb, graph_emb], dim=-1)
        logits = self.policy_branch(final_emb)
        value = self.value_branch(final_emb).squeeze(-1)
        if self.config["apply_action_mask"]:
            inf_mask = torch.clamp(torch.log(action_mask.to(logits.dtype)),
                                   min=torch.finfo(torch.float32).min)
            logits = logits + inf_mask
        return logits, value

    def forward(self, obs: Dict[str, torch.Tensor]):
        """obs: batched padded observation dict (torch tensors, [B, ...])."""
        batch = GraphBatch.from_padded(
            obs["node_features"], obs["edge_features"], obs["edges_src"],
            obs["edges_dst"], obs["node_split"], obs["edge_split"])
        return self.forward_flat(batch, obs["graph_features"],
                                 obs["action_mask"])


TRUNK_NUMEL = 4146      # parameters of the tuned GNN (gnn_trunk.hip, GT_NP)


@torch.no_grad()
def gnn_trunk_population(pop: torch.Tensor, batch: GraphBatch,
                         offset: int = 0) -> torch.Tensor:
    """Per-graph mean node embeddings ``[P, G, 16]`` of ``P`` tuned GNNs on
    one ``batch``: member ``m``'s trunk is ``pop[m, offset : offset + 4146]``
    in ``gnn.parameters()`` order (``offset = 0`` for a flat ``GNNPolicy``).
    On a GPU this is one launch of ``gt_pop_fwd_kernel``
    (ops/hip/gnn_trunk.hip); anything else is the plain chain, member by
    member, which is also the kernel's oracle.  No gradient."""
    if pop.dim() != 2 or pop.shape[0] < 1 or offset < 0 \
            or offset + TRUNK_NUMEL > pop.shape[1]:
        raise ValueError(
            "gnn_trunk_population: pop must be [P >= 1, n] with the tuned "
            f"trunk's {TRUNK_NUMEL} parameters at [offset, offset + "
            f"{TRUNK_NUMEL}); got {tuple(pop.shape)}, offset {offset}")
    if (batch.z.is_cuda
            and os.environ.get("DDLS_AMD_DISABLE_HIP", "0") != "1"):
        from .. import ops as hip_ops
        ext = hip_ops.get_extension(required=True)
        return ext.gnn_trunk_population_fwd(
            batch.z.detach().float().contiguous(),
            batch.e.detach().float().contiguous(), list(batch.trunk_plan()),
            pop.detach().float().contiguous(), int(offset))
    gnn = GNN(dict(DEFAULT_GNN_CONFIG)).to(batch.z.device, batch.z.dtype)
    params = list(gnn.parameters())
    assert sum(p.numel() for p in params) == TRUNK_NUMEL
    out = []
    for m in range(pop.shape[0]):
        off = offset
        for p in params:
            p.copy_(pop[m, off:off + p.numel()].view(p.shape))
            off += p.numel()
        out.append(graph_mean(gnn(batch), batch))
    return torch.stack(out).contiguous()
