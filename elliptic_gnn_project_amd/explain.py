"""GNNExplainer on the GPU (src/analysis/explain.py, the ``gnn`` sub-command): node-feature and edge
masks for many flagged nodes at once, each on its own computation subgraph, with the per-epoch mask
update in one HIP launch per mask (libgnnmp K16, csrc/explain.hip).

The algorithm is PyG 2.5.3 ``GNNExplainer`` as the reference configures it (node_mask_type
"attributes", edge_mask_type "object", explanation_type "model", binary classification on the raw
logit z = logits[:, 1] - logits[:, 0] of its ProbModel wrapper).  For a target node v of a model in
eval() mode:

    y  = (z_unmasked[v] > 0)
    M [N, F] ~ N(0, 0.1^2),   m [E] ~ N(0, std^2),  std = sqrt(2) * sqrt(2 / (2 N)),  N the FULL graph's
    epoch i: h = x * sigmoid(M); forward under set_masks(model, m, edge_index, apply_sigmoid=True);
             loss = BCE_with_logits(z[v], y)
                    + [i >= 1]  0.005 * sum(s_m) + 1.0 * mean(ent(s_m))        over the hard edges
                    + [i >= 1]  1.0 * mean(s_M) + 0.1 * mean(ent(s_M))         over the hard features
             ent(s) = -s log(s + 1e-15) - (1 - s) log(1 - s + 1e-15);   one torch.optim.Adam step (lr)
             after epoch 0's backward: hard_M = (dM != 0), hard_m = (dm != 0)
    result: sigmoid(M) * hard_M, sigmoid(m) * hard_m

Deviations, both stated in the issue that introduced this module:
* The initial logits come from the seeded counter-hash Gaussian of robustness.add_noise on zeros
  (host mirror: robustness.host_noise), keyed by GLOBAL node row / edge id: M from the noise seed
  ``node_seed(seed) = 2 * seed`` over [N, F], m from ``edge_seed(seed) = 2 * seed + 1`` over [E, 1]
  (both mod 2^64).  A subgraph run therefore starts from exactly the values a full-graph run has.
* A block without hard edges (features) gets no edge (feature) regulariser, where PyG's mean over
  an empty tensor would turn every mask into NaN.

A node's logits depend only on its L-hop in-neighbourhood (L conv layers), and PyG zeroes every mask
entry outside it, so each target is explained on the subgraph the neighbour sampler extracts with
fanout -1, and B targets run side by side as one block-diagonal graph: the prediction loss is the
sum of the targets' BCE terms and every regulariser mean is taken per block, so one batched run
equals B separate ones.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import math
import time
from dataclasses import dataclass
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib
from .conv import clear_masks, set_masks
from .dataset_elliptic import GraphData
from .robustness import _M64, _touch, add_noise, host_noise

EPS = 1e-15  # PyG GNNExplainer's EPS
COEFFS = dict(edge_size=0.005, edge_ent=1.0, node_feat_size=1.0, node_feat_ent=0.1)  # GNNExplainer.coeffs
BETAS, ADAM_EPS = (0.9, 0.999), 1e-8  # torch.optim.Adam defaults
NODE_INIT_STD = 0.1


def node_seed(seed: int) -> int:
    return (2 * int(seed)) & _M64


def edge_seed(seed: int) -> int:
    return (2 * int(seed) + 1) & _M64


def edge_init_std(num_nodes: int) -> float:
    """PyG's edge-mask init: calculate_gain('relu') * sqrt(2 / (2 N))."""
    return math.sqrt(2.0) * math.sqrt(2.0 / (2.0 * max(int(num_nodes), 1)))


def host_init_masks(num_nodes: int, num_feats: int, num_edges: int, seed: int) -> Tuple[np.ndarray, np.ndarray]:
    """The float64 host mirror of the initial logits (M [N, F], m [E])."""
    M = NODE_INIT_STD * host_noise(num_nodes, num_feats, node_seed(seed))
    m = edge_init_std(num_nodes) * host_noise(num_edges, 1, edge_seed(seed))[:, 0]
    return M, m


def init_masks(num_nodes: int, num_feats: int, num_edges: int, seed: int, device) -> Tuple[torch.Tensor, torch.Tensor]:
    """The initial logits of the full graph on ``device`` (K15 on zeros)."""
    M = add_noise(torch.zeros((num_nodes, num_feats), dtype=torch.float32, device=device), NODE_INIT_STD,
                  node_seed(seed))
    m = add_noise(torch.zeros((num_edges, 1), dtype=torch.float32, device=device), edge_init_std(num_nodes),
                  edge_seed(seed))
    return M, m.reshape(-1)


# ----------------------------------------------------------------------------- the mask step: mirror and K16
def host_mask_step(mask, exp_avg, exp_avg_sq, block_of, t: int, grad=None, dh=None, x=None, hard=None,
                   size_scale=None, ent_scale=None, lr: float = 0.01, betas=BETAS, eps: float = ADAM_EPS,
                   num_blocks: Optional[int] = None) -> Dict[str, np.ndarray]:
    """One gnn_explain_mask_step_f32 call restated in numpy float64.  Plain form: ``grad`` [n]; gate
    form: ``dh`` and ``x`` [n, F] with ``block_of`` [n] per row.  ``hard`` None is epoch 0.  Returns
    mask, exp_avg, exp_avg_sq, hard_out (epoch 0), h (gate form) and skipped (bad block ids)."""
    mk = np.array(mask, dtype=np.float64)
    m1 = np.array(exp_avg, dtype=np.float64)
    m2 = np.array(exp_avg_sq, dtype=np.float64)
    blk = np.asarray(block_of).astype(np.int64)
    gate = x is not None
    B = int(num_blocks) if num_blocks is not None else (len(size_scale) if size_scale is not None else int(blk.max(initial=0)) + 1)
    valid = (blk >= 0) & (blk < B)
    b = np.where(valid, blk, 0)
    if gate:
        xv = np.asarray(x, dtype=np.float64)
        valid, b = valid[:, None], b[:, None]
    out = {"skipped": ~np.broadcast_to(valid, mk.shape)}
    if t > 0:
        s = 1.0 / (1.0 + np.exp(-mk))
        sm = 1.0 / (1.0 + np.exp(mk))  # 1 - s
        g = np.asarray(dh, dtype=np.float64) * xv * (s * sm) if gate else np.array(grad, dtype=np.float64)
        if hard is None:
            out["hard_out"] = (g != 0) & valid
        else:
            ss = np.asarray(size_scale, dtype=np.float64)[b]
            es = np.asarray(ent_scale, dtype=np.float64)[b]
            dent = -np.log(s + EPS) - s / (s + EPS) + np.log(sm + EPS) + sm / (sm + EPS)
            g = g + (np.asarray(hard) != 0) * (s * sm) * (ss + es * dent)
        n1 = betas[0] * m1 + (1.0 - betas[0]) * g
        n2 = betas[1] * m2 + (1.0 - betas[1]) * g * g
        step = lr / (1.0 - betas[0] ** t)
        new = mk - step * n1 / (np.sqrt(n2) / math.sqrt(1.0 - betas[1] ** t) + eps)
        mk, m1, m2 = np.where(valid, new, mk), np.where(valid, n1, m1), np.where(valid, n2, m2)
    out.update(mask=mk, exp_avg=m1, exp_avg_sq=m2)
    if gate:
        out["h"] = xv / (1.0 + np.exp(-mk))
    return out


def _ld(t: torch.Tensor) -> int:
    return int(t.stride(0)) if t.size(0) > 1 else max(int(t.stride(0)), int(t.size(1)))


def mask_step(mask: torch.Tensor, exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor, block_of: torch.Tensor,
              num_blocks: int, t: int, status: torch.Tensor, grad=None, dh=None, x=None, h=None, hard=None,
              hard_out=None, size_scale=None, ent_scale=None, lr: float = 0.01, betas=BETAS,
              eps: float = ADAM_EPS) -> None:
    """K16 on CUDA tensors, in place (see gnnmp.h gnn_explain_step_params).  f32 masks, moments,
    gradients and scales, uint8 hard masks, int32 ``block_of`` and ``status`` [1]; 2-D operands of the
    gate form need unit column stride.  Nothing is synchronised: the caller reads ``status``."""
    gate = x is not None
    p = _lib.GnnExplainStepParams()
    f32 = [mask, exp_avg, exp_avg_sq, grad, dh, x, h, size_scale, ent_scale]
    if any(v is not None and v.dtype != torch.float32 for v in f32):
        raise TypeError("mask_step: float32 operands")
    if any(v is not None and v.dtype != torch.uint8 for v in (hard, hard_out)):
        raise TypeError("mask_step: uint8 hard masks")
    if block_of.dtype != torch.int32 or status.dtype != torch.int32:
        raise TypeError("mask_step: int32 block_of and status")
    if gate:
        mats = [v for v in (mask, exp_avg, exp_avg_sq, dh, x, h, hard, hard_out) if v is not None]
        if any(v.dim() != 2 or v.shape != mask.shape or (v.size(1) > 0 and v.stride(1) != 1) for v in mats):
            raise ValueError("mask_step: the gate form takes [rows, F] operands of one shape with unit column stride")
        if exp_avg_sq.stride(0) != exp_avg.stride(0) or (hard is not None and hard_out is not None
                                                         and hard.stride(0) != hard_out.stride(0)):
            raise ValueError("mask_step: the moments (and the hard masks) share one leading dimension")
        p.n, p.F = int(mask.size(0)), int(mask.size(1))
        p.ld_mask, p.ld_x, p.ld_state = _ld(mask), _ld(x), _ld(exp_avg)
        p.ld_dh = _ld(dh) if dh is not None else 0
        p.ld_h = _ld(h) if h is not None else 0
        hm = hard if hard is not None else hard_out
        p.ld_hard = _ld(hm) if hm is not None else 0
    else:
        vecs = [v for v in (mask, exp_avg, exp_avg_sq, grad, hard, hard_out) if v is not None]
        if any(v.dim() != 1 or v.numel() != mask.numel() or not v.is_contiguous() for v in vecs):
            raise ValueError("mask_step: the plain form takes contiguous [n] operands")
        p.n, p.F = int(mask.numel()), 1
    if block_of.numel() != p.n or not block_of.is_contiguous():
        raise ValueError("mask_step: block_of must be a contiguous [n]")
    for sc in (size_scale, ent_scale):
        if sc is not None and (sc.numel() != num_blocks or not sc.is_contiguous()):
            raise ValueError("mask_step: the scales are contiguous [num_blocks]")
    p.mask, p.grad, p.dh, p.x, p.h = _lib.ptr(mask), _lib.ptr(grad), _lib.ptr(dh), _lib.ptr(x), _lib.ptr(h)
    p.exp_avg, p.exp_avg_sq = _lib.ptr(exp_avg), _lib.ptr(exp_avg_sq)
    p.hard, p.hard_out = _lib.ptr(hard), _lib.ptr(hard_out)
    p.block_of, p.num_blocks, p.t = _lib.ptr(block_of), int(num_blocks), int(t)
    p.size_scale, p.ent_scale = _lib.ptr(size_scale), _lib.ptr(ent_scale)
    p.lr, p.beta1, p.beta2, p.eps = float(lr), float(betas[0]), float(betas[1]), float(eps)
    p.status = _lib.ptr(status)
    with torch.cuda.device(mask.device):
        _lib.call("gnn_explain_mask_step_f32", ctypes.byref(p), _lib.stream_handle(mask.device))
    if h is not None:
        _touch(h)  # written through its raw pointer: caches keyed on (data_ptr, _version) see an edit


def _block_scales(hard: torch.Tensor, block_of: torch.Tensor, num_blocks: int, size_coeff: float, ent_coeff: float,
                  size_is_mean: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per-block coefficients of sum(s) and sum(ent(s)) over a block's hard entries, so that the sums
    are the block's regularisers (``size_is_mean``: a mean, else PyG's plain sum); 0 for an empty block."""
    per = hard.reshape(hard.size(0), -1).sum(dim=1, dtype=torch.float32)
    cnt = torch.zeros(num_blocks, dtype=torch.float32, device=hard.device).index_add_(0, block_of.long(), per)
    inv = torch.where(cnt > 0, 1.0 / cnt.clamp_min(1.0), torch.zeros_like(cnt))
    size = size_coeff * inv if size_is_mean else torch.where(cnt > 0, torch.full_like(cnt, size_coeff),
                                                             torch.zeros_like(cnt))
    return size.contiguous(), (ent_coeff * inv).contiguous()


def _reg_term(logit: torch.Tensor, hard: torch.Tensor, size_scale: torch.Tensor, ent_scale: torch.Tensor,
              block_of: torch.Tensor) -> torch.Tensor:
    """The regularisers of one mask as PyG writes them (torch autograd), summed over the blocks."""
    s = logit.sigmoid()
    ent = -s * torch.log(s + EPS) - (1.0 - s) * torch.log(1.0 - s + EPS)
    ss, es = size_scale[block_of.long()], ent_scale[block_of.long()]
    if logit.dim() == 2:
        ss, es = ss.unsqueeze(1), es.unsqueeze(1)
    return ((ss * s + es * ent) * hard.to(s.dtype)).sum()


# ----------------------------------------------------------------------------- the search loop
@dataclass
class _Problem:
    """One block-diagonal run: B blocks over ``x`` [rows, F] / ``edge_index`` [2, edges] (local ids)."""
    x: torch.Tensor
    edge_index: torch.Tensor
    t_idx: Optional[torch.Tensor]
    target_rows: torch.Tensor  # [B] row of each block's target
    row_block: torch.Tensor    # [rows] int32
    edge_block: torch.Tensor   # [edges] int32
    num_blocks: int
    M: torch.Tensor            # [rows, F] initial logits (updated in place)
    m: torch.Tensor            # [edges]


def _search(model, pr: _Problem, epochs: int, lr: float, fused_step: bool, stats: Optional[Dict] = None):
    """The epoch loop over one problem.  Returns (node_mask, edge_mask, hard_M, hard_m, y, prob)."""
    if epochs < 1:
        raise ValueError("epochs must be >= 1")
    dev = pr.x.device
    B = pr.num_blocks
    x = pr.x.detach().contiguous()
    ei, t_idx, tgt = pr.edge_index, pr.t_idx, pr.target_rows
    M, m = pr.M.detach().contiguous(), pr.m.detach().contiguous()
    with torch.no_grad():
        logits = model(x, ei, t_idx).float()
        y = (logits[tgt, 1] - logits[tgt, 0] > 0).to(torch.float32)
        prob = torch.softmax(logits[tgt], dim=1)[:, 1]

    def loss_of(h):
        out = model(h, ei, t_idx).float()
        return F.binary_cross_entropy_with_logits(out[tgt, 1] - out[tgt, 0], y, reduction="sum")

    hard_M = torch.zeros(M.shape, dtype=torch.uint8, device=dev)
    hard_m = torch.zeros(m.shape, dtype=torch.uint8, device=dev)
    scales = None
    set_masks(model, m, ei, apply_sigmoid=True)
    try:
        if stats is not None:
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
        if fused_step:
            status = torch.zeros(1, dtype=torch.int32, device=dev)
            mom = [torch.zeros_like(M), torch.zeros_like(M), torch.zeros_like(m), torch.zeros_like(m)]
            h = torch.empty_like(x)
            mask_step(M, mom[0], mom[1], pr.row_block, B, 0, status, x=x, h=h)  # the first gate
            h.requires_grad_(True)
            m.requires_grad_(True)
            for i in range(epochs):
                with torch.enable_grad():
                    dh, dm = torch.autograd.grad(loss_of(h), [h, m])
                first = i == 0
                mask_step(M, mom[0], mom[1], pr.row_block, B, i + 1, status, dh=dh.contiguous(), x=x, h=h.detach(),
                          hard=None if first else hard_M, hard_out=hard_M if first else None,
                          size_scale=None if first else scales[0], ent_scale=None if first else scales[1], lr=lr)
                mask_step(m.detach(), mom[2], mom[3], pr.edge_block, B, i + 1, status, grad=dm.contiguous(),
                          hard=None if first else hard_m, hard_out=hard_m if first else None,
                          size_scale=None if first else scales[2], ent_scale=None if first else scales[3], lr=lr)
                _touch(h)
                _touch(m)
                if first:
                    scales = (_block_scales(hard_M, pr.row_block, B, COEFFS["node_feat_size"], COEFFS["node_feat_ent"], True)
                              + _block_scales(hard_m, pr.edge_block, B, COEFFS["edge_size"], COEFFS["edge_ent"], False))
            m = m.detach()
        else:
            M.requires_grad_(True)
            m.requires_grad_(True)
            opt = torch.optim.Adam([M, m], lr=lr)
            for i in range(epochs):
                with torch.enable_grad():
                    loss = loss_of(x * M.sigmoid())
                    if i > 0:
                        loss = loss + _reg_term(m, hard_m, scales[2], scales[3], pr.edge_block) \
                            + _reg_term(M, hard_M, scales[0], scales[1], pr.row_block)
                    M.grad, m.grad = torch.autograd.grad(loss, [M, m])
                if i == 0:
                    hard_M, hard_m = (M.grad != 0).to(torch.uint8), (m.grad != 0).to(torch.uint8)
                    scales = (_block_scales(hard_M, pr.row_block, B, COEFFS["node_feat_size"], COEFFS["node_feat_ent"], True)
                              + _block_scales(hard_m, pr.edge_block, B, COEFFS["edge_size"], COEFFS["edge_ent"], False))
                opt.step()
            M, m = M.detach(), m.detach()
    finally:
        clear_masks(model)  # also on an exception: the model never stays in explain mode
    if stats is not None:
        torch.cuda.synchronize(dev)
        stats.setdefault("runs", []).append(dict(rows=int(x.size(0)), edges=int(ei.size(1)), blocks=B, epochs=epochs,
                                                 ms_per_epoch=(time.perf_counter() - t0) * 1e3 / epochs))
    if fused_step and int(status.item()) != 0:
        raise IndexError("explain: a block id outside [0, num_blocks) reached the mask step")
    hard_M, hard_m = hard_M.bool(), hard_m.bool()
    return M.sigmoid() * hard_M, m.sigmoid() * hard_m, hard_M, hard_m, y, prob


# ----------------------------------------------------------------------------- subgraphs and batching
@dataclass
class NodeExplanation:
    """The masks of one target over its computation subgraph (local row 0 is the target)."""
    node_id: int
    n_id: torch.Tensor        # [rows] global node ids
    e_id: torch.Tensor        # [edges] global PyG edge ids
    node_mask: torch.Tensor   # [rows, F] sigmoid(M) * hard
    edge_mask: torch.Tensor   # [edges]   sigmoid(m) * hard
    node_hard: torch.Tensor   # [rows, F] bool
    edge_hard: torch.Tensor   # [edges] bool
    target: int               # the explained class: z_unmasked > 0
    probability_illicit: float  # unmasked softmax(logits)[1] of the target

    def to_full(self, num_nodes: int, num_edges: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """The masks in the reference's shapes: [N, F] and [E], zero outside the subgraph."""
        nm = self.node_mask.new_zeros((int(num_nodes), self.node_mask.size(1)))
        nm.index_copy_(0, self.n_id, self.node_mask)
        em = self.edge_mask.new_zeros(int(num_edges))
        em.index_copy_(0, self.e_id, self.edge_mask)
        return nm, em


def num_hops(model) -> int:
    """Hops of the computation subgraph: the number of conv layers L, and L + 1 for GCNNet — gcn_norm
    reads the in-degree of every sender, so the senders at distance L need their own in-edges for the
    L-hop messages to carry the full graph's weights (with L hops their degrees come out too small)."""
    from .gnn import GCNNet

    L = len(model.convs)
    return L + 1 if isinstance(model, GCNNet) else L


def _explanations(targets, subs, res, offs_n, offs_e) -> List[NodeExplanation]:
    nm, em, hM, hm, y, prob = res
    y, prob = y.cpu().tolist(), prob.cpu().tolist()
    out = []
    for b, (v, sub) in enumerate(zip(targets, subs)):
        rn, re = slice(offs_n[b], offs_n[b + 1]), slice(offs_e[b], offs_e[b + 1])
        out.append(NodeExplanation(int(v), sub.n_id, sub.e_id, nm[rn], em[re], hM[rn], hm[re], int(y[b]), float(prob[b])))
    return out


def _run_blocks(model, x, t_idx, M0, m0, targets, subs, epochs, lr, fused_step, stats) -> List[NodeExplanation]:
    dev = x.device
    B = len(subs)
    offs_n = np.concatenate([[0], np.cumsum([int(s.n_id.numel()) for s in subs])]).tolist()
    offs_e = np.concatenate([[0], np.cumsum([int(s.e_id.numel()) for s in subs])]).tolist()
    n_id = torch.cat([s.n_id for s in subs])
    e_id = torch.cat([s.e_id for s in subs])
    ei = torch.cat([s.edge_index + o for s, o in zip(subs, offs_n)], dim=1)
    i32 = dict(dtype=torch.int32, device=dev)
    row_block = torch.repeat_interleave(torch.arange(B, **i32), torch.tensor(np.diff(offs_n), device=dev))
    edge_block = torch.repeat_interleave(torch.arange(B, **i32), torch.tensor(np.diff(offs_e), device=dev))
    xs, ts = x.index_select(0, n_id), (t_idx.index_select(0, n_id) if t_idx is not None else None)
    M, m = M0.index_select(0, n_id), m0.index_select(0, e_id)
    nb = B
    if ei.size(1) == 0:
        # a run of isolated targets only: the explain-mode aggregations take no empty edge list, so it
        # gets a phantom block of two zero rows joined by one edge.  Nothing in it has a gradient, so
        # it is never hard, shares no block with a target, and is cut off the result below.
        rows = xs.size(0)
        xs = torch.cat([xs, xs.new_zeros((2, xs.size(1)))])
        ts = torch.cat([ts, ts[:1].expand(2)]) if ts is not None else None
        M, m = torch.cat([M, M.new_zeros((2, M.size(1)))]), m.new_zeros(1)
        ei = torch.tensor([[rows], [rows + 1]], dtype=torch.int64, device=dev)
        row_block = torch.cat([row_block, torch.full((2,), B, **i32)])
        edge_block = torch.full((1,), B, **i32)
        nb = B + 1
    pr = _Problem(xs, ei.contiguous(), ts, torch.tensor(offs_n[:-1], dtype=torch.int64, device=dev), row_block,
                  edge_block, nb, M, m)
    res = _search(model, pr, epochs, lr, fused_step, stats)
    return _explanations(targets, subs, res, offs_n, offs_e)


def _check_model(model, x: torch.Tensor) -> None:
    if not x.is_cuda or x.dtype != torch.float32 or x.dim() != 2:
        raise RuntimeError("explain: the convs run on the MI355X (HIP) device only; x must be a CUDA float32 [N, F]")
    if model.training:
        raise ValueError("explain: the model must be in eval() mode")


def explain_nodes(model, data, nodes: Sequence[int], epochs: int = 200, lr: float = 0.01, seed: int = 0,
                  t_idx: Optional[torch.Tensor] = None, fused_step: bool = True, max_rows: int = 1 << 18,
                  stats: Optional[Dict] = None) -> List[NodeExplanation]:
    """GNNExplainer masks of every node in ``nodes`` (global ids) for ``model`` (eval mode) on
    ``data`` (x [N, F] f32 and edge_index [2, E] on the GPU).  Each node is explained on its own
    computation subgraph; as many as fit ``max_rows`` concatenated rows run as one block-diagonal
    batch, further ones in further runs.  ``t_idx``: the timesteps of a model with a time embedding.
    ``fused_step=False`` runs the same loop with autograd regularisers and torch.optim.Adam (the A/B of
    K16).  ``stats`` (a dict) receives rows / edges / ms per epoch of every run.  The model leaves
    explain mode on return and on an exception."""
    from .loader import NeighborLoader

    x, ei = data.x, data.edge_index
    _check_model(model, x)
    N, E = int(x.size(0)), int(ei.size(1))
    nodes = [int(v) for v in nodes]
    if any(v < 0 or v >= N for v in nodes):
        raise IndexError(f"explain_nodes: node outside [0, {N})")
    if not nodes:
        return []
    # fanout -1: nothing is drawn, the sampler's seed is unused; x without columns: only ids are wanted
    loader = NeighborLoader(GraphData(edge_index=ei, x=x[:, :0]), [-1] * num_hops(model), batch_size=1)
    subs = [loader.sample(torch.tensor([v], device=x.device), seed=0) for v in nodes]
    M0, m0 = init_masks(N, int(x.size(1)), E, seed, x.device)
    out: List[NodeExplanation] = []
    lo = 0
    while lo < len(nodes):
        hi, rows = lo + 1, int(subs[lo].n_id.numel())
        while hi < len(nodes) and rows + int(subs[hi].n_id.numel()) <= max_rows:
            rows += int(subs[hi].n_id.numel())
            hi += 1
        out += _run_blocks(model, x, t_idx, M0, m0, nodes[lo:hi], subs[lo:hi], epochs, lr, fused_step, stats)
        lo = hi
    return out


def explain_full_graph(model, data, node: int, epochs: int = 200, lr: float = 0.01, seed: int = 0,
                       t_idx: Optional[torch.Tensor] = None, fused_step: bool = False,
                       stats: Optional[Dict] = None) -> NodeExplanation:
    """The reference's own form: one node, the loop over the whole graph with [N, F] and [E] masks
    (n_id and e_id are the identity).  What ``explain_nodes`` is tested against."""
    x, ei = data.x, data.edge_index
    _check_model(model, x)
    N, E = int(x.size(0)), int(ei.size(1))
    dev = x.device
    M0, m0 = init_masks(N, int(x.size(1)), E, seed, dev)
    i32 = dict(dtype=torch.int32, device=dev)
    pr = _Problem(x, ei, t_idx, torch.tensor([int(node)], device=dev), torch.zeros(N, **i32), torch.zeros(E, **i32),
                  1, M0, m0)
    nm, em, hM, hm, y, prob = _search(model, pr, epochs, lr, fused_step, stats)
    return NodeExplanation(int(node), torch.arange(N, device=dev), torch.arange(E, device=dev), nm, em, hM, hm,
                           int(y.item()), float(prob.item()))


def time_epochs(model, data, nodes: Sequence[int], epochs: int = 20, warmup: int = 3, fused_step: bool = True,
                t_idx: Optional[torch.Tensor] = None) -> Dict:
    """Milliseconds per epoch of one explain_nodes batch (after a ``warmup``-epoch run), with its
    concatenated row and edge counts — the measurement of DESIGN.md §4 "Explainer"."""
    explain_nodes(model, data, nodes, epochs=warmup, t_idx=t_idx, fused_step=fused_step)
    stats: Dict = {}
    explain_nodes(model, data, nodes, epochs=epochs, t_idx=t_idx, fused_step=fused_step, stats=stats)
    runs = stats["runs"]
    return dict(targets=len(nodes), fused_step=bool(fused_step), epochs=epochs, runs=len(runs),
                rows=sum(r["rows"] for r in runs), edges=sum(r["edges"] for r in runs),
                ms_per_epoch=sum(r["ms_per_epoch"] for r in runs))


# ----------------------------------------------------------------------------- node picker, export, CLI
def _load_scores(run_dir: Path):
    paths = [run_dir / n for n in ("scores_test.npy", "y_test.npy", "node_idx_test.npy")]
    if not all(p.exists() for p in paths):
        raise FileNotFoundError(f"{run_dir} lacks scores_test.npy, y_test.npy or node_idx_test.npy (train_gnn.main writes them)")
    scores, labels, node_ids = (np.load(p) for p in paths)
    thr = 0.5
    if (run_dir / "metrics.json").exists():
        with open(run_dir / "metrics.json", encoding="utf-8") as f:
            thr = float(json.load(f).get("threshold", thr))
    return scores, labels, node_ids, thr


def _info(kind: str, scores, labels, i: int) -> Dict:
    return {"selection": kind, "score": float(scores[i]), "label": int(labels[i])}


def pick_nodes(run_dir, nodes: Optional[Sequence[int]] = None, top: Optional[int] = None) -> List[Tuple[int, Dict]]:
    """[(node id, selection record)] as pick_node_to_explain (src/analysis/explain.py:370-429) chooses:
    the requested test nodes ("user"); else, by descending test score, the first true positive at the
    run's threshold, else the first false positive, else the highest score.  ``top`` = K: the K
    highest-scored predicted positives in that order ("top_k"; the auto pick when there is none)."""
    run_dir = Path(run_dir)
    scores, labels, node_ids, thr = _load_scores(run_dir)
    if nodes:
        out = []
        for v in nodes:
            hit = np.where(node_ids == int(v))[0]
            if hit.size == 0:
                raise ValueError(f"node {int(v)} is not one of the run's test nodes")
            out.append((int(v), _info("user", scores, labels, int(hit[0]))))
        return out
    order = np.argsort(scores)[::-1]
    pos = [int(i) for i in order if scores[i] >= thr]
    if top is not None:
        if int(top) < 1:
            raise ValueError("--top needs K >= 1")
        if pos:
            return [(int(node_ids[i]), _info("top_k", scores, labels, i)) for i in pos[:int(top)]]
    for kind, want in (("auto_true_positive", 1), ("auto_false_positive", 0)):
        cand = [i for i in pos if labels[i] == want]
        if cand:
            return [(int(node_ids[cand[0]]), _info(kind, scores, labels, cand[0]))]
    i = int(order[0])
    return [(int(node_ids[i]), _info("auto_high_score", scores, labels, i))]


def feature_names(num_feats: int, cfg: Dict) -> List[str]:
    names = [f"f{i}" for i in range(num_feats)]
    if names and cfg.get("use_time_scalar", False) and int(cfg.get("time_embed_dim", 0)) == 0:
        names[-1] = "time_scalar"  # the appended normalised timestep
    return names


def importance_record(ex: NodeExplanation, edge_index: torch.Tensor, num_nodes: int, cfg: Dict, selection: Dict,
                      probability: Optional[float] = None) -> Dict:
    """The reference's gnn_explainer_importance.json record (:673-731): feature importance = the column
    means of |node_mask| over the FULL graph's N rows, top min(20, F); edge importance = the top
    min(20, hard edges) in global ids.  Ties go to the lower feature index / edge id."""
    feat = ex.node_mask.abs().sum(dim=0, dtype=torch.float64).cpu().numpy() / float(num_nodes)
    names = feature_names(feat.shape[0], cfg)
    f_order = np.lexsort((np.arange(feat.shape[0]), -feat))[:min(20, feat.shape[0])]
    em = ex.edge_mask.detach().cpu().numpy().astype(np.float64)
    e_id = ex.e_id.cpu().numpy()
    n_hard = int(ex.edge_hard.sum().item())
    e_order = np.lexsort((e_id, -em))[:min(20, n_hard)]
    ends = edge_index.index_select(1, ex.e_id[torch.as_tensor(e_order, device=ex.e_id.device, dtype=torch.long)]).cpu().numpy() \
        if len(e_order) else np.zeros((2, 0), dtype=np.int64)
    return {
        "node_id": int(ex.node_id),
        "selection": selection,
        "probability_illicit": float(ex.probability_illicit if probability is None else probability),
        "feature_importance": [{"feature": names[int(i)], "importance": float(feat[int(i)])} for i in f_order],
        "edge_importance": [{"source": int(ends[0, k]), "target": int(ends[1, k]), "importance": float(em[int(i)])}
                            for k, i in enumerate(e_order)],
    }


def run_gnn(run_dir, node: Optional[int] = None, nodes: Optional[Sequence[int]] = None, top: Optional[int] = None,
            epochs: int = 200, seed: int = 0, processed_dir=None, fused_step: bool = True):
    """The ``gnn`` sub-command: explain the picked node(s) of a trained run and write
    gnn_explainer_importance.json (one node) or gnn_explainer_importance_batch.json (several)."""
    from .robustness import Run

    run_dir = Path(run_dir)
    want = list(nodes) if nodes else ([int(node)] if node is not None else None)
    picked = pick_nodes(run_dir, want, top)
    r = Run(run_dir, processed_dir)
    exs = explain_nodes(r.model, r.data, [v for v, _ in picked], epochs=epochs, seed=seed, t_idx=r.t_idx,
                        fused_step=fused_step)
    with torch.no_grad():  # the report's probability comes from the plain full-graph forward, as the reference's
        probs = torch.softmax(r.model(r.data.x, r.data.edge_index, r.t_idx).float(), dim=-1)[:, 1]
    recs = [importance_record(ex, r.data.edge_index, r.data.num_nodes, r.cfg, sel, float(probs[ex.node_id]))
            for ex, (_, sel) in zip(exs, picked)]
    single = len(recs) == 1 and top is None and not (nodes and len(nodes) > 1)
    out = recs[0] if single else recs
    name = "gnn_explainer_importance.json" if single else "gnn_explainer_importance_batch.json"
    with open(run_dir / name, "w", encoding="utf-8") as f:
        json.dump(out, f, indent=2)
    return out


def main(argv=None) -> None:
    ap = argparse.ArgumentParser(description="Explanations of a trained run's predictions")
    sub = ap.add_subparsers(dest="mode", required=True)
    g = sub.add_parser("gnn", help="GNNExplainer masks for test nodes of a GNN run")
    g.add_argument("--run_dir", type=Path, required=True, help="the trained run's directory")
    sel = g.add_mutually_exclusive_group()
    sel.add_argument("--node", type=int, default=None, help="one node id (default: picked from the test scores)")
    sel.add_argument("--nodes", type=int, nargs="+", default=None, help="Several node indices, explained as one batch")
    sel.add_argument("--top", type=int, default=None, help="Explain the K highest-scored predicted positives")
    g.add_argument("--epochs", type=int, default=200, help="GNNExplainer epochs")
    g.add_argument("--seed", type=int, default=0, help="Seed of the initial masks")
    g.add_argument("--processed_dir", type=Path, default=None,
                   help="processed graph directory (default: the run's config)")
    args = ap.parse_args(argv)
    out = run_gnn(args.run_dir, args.node, args.nodes, args.top, args.epochs, args.seed, args.processed_dir)
    recs = out if isinstance(out, list) else [out]
    print(json.dumps([{k: r[k] for k in ("node_id", "selection", "probability_illicit")} for r in recs], indent=2))


if __name__ == "__main__":
    main()
