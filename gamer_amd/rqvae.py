"""RQ-VAE item tokenizer on the HIP path (ref:SeqRec/models/tokenizer/RQVAE/*): the first stage of the pipeline, which turns item
embeddings into the semantic IDs every other model here consumes.

  encoder / decoder   act(x W^T + b) layers on the Linear + bias_act kernels ("f32" matmul mode), ``LinearActFn``
  quantiser           one autograd function (``RVQFn``) over gamer_rvq_fwd / gamer_rvq_bwd (csrc/rqvae.hip): all levels in one
                      launch; a Sinkhorn level costs one distance-only launch, the fp64 Sinkhorn in torch, and one launch that
                      takes the index it chose
  Sinkhorn            ``center_distance_for_constraint`` + ``sinkhorn_algorithm``: device torch ops in fp64, in the reference's
                      order of operations (they also run on the CPU)
  diversity term      positives drawn on the host with Python's ``random.choice`` in the reference's call order (one device-to-host
                      copy of the indices per step), the loss as vectorised device torch ops
  clustering          ``constrained_km`` behind ``--cluster_backend``: the reference's KMeansConstrained when installed, plain
                      sklearn KMeans as a documented deviation, or none

Parameters carry the reference's state-dict names (``encoder.mlp_layers.{1,4,..}``, ``rq.vq_layers.{i}.embedding.weight``,
``decoder...``), so its checkpoints load here and the ones written here load there.  BatchNorm and dropout are not built.
"""
from __future__ import annotations

import random
import warnings
from argparse import Namespace

import numpy as np
import torch
from torch import nn
from torch.nn import functional as F

from . import ops, rec_common

MU = 0.25                                   # the commitment weight of every level (VectorQuantizer's default, never overridden)
CLUSTER_BACKENDS = ("k_means_constrained", "sklearn", "none")


# ---- Sinkhorn (fp64 torch, the reference's order of operations) -------------------------------------------------------------------
def center_distance_for_constraint(distances: torch.Tensor) -> torch.Tensor:
    max_distance = distances.max()
    min_distance = distances.min()
    middle = (max_distance + min_distance) / 2
    amplitude = max_distance - middle + 1e-5
    assert amplitude > 0
    return (distances - middle) / amplitude


@torch.no_grad()
def sinkhorn_algorithm(distances: torch.Tensor, epsilon: float, sinkhorn_iterations: int) -> torch.Tensor:
    Q = torch.exp(-distances / epsilon)
    B, K = Q.shape
    Q /= Q.sum(-1, keepdim=True).sum(-2, keepdim=True)
    for _ in range(sinkhorn_iterations):
        Q /= torch.sum(Q, dim=1, keepdim=True)
        Q /= B
        Q /= torch.sum(Q, dim=0, keepdim=True)
        Q /= K
    Q *= B
    return Q


def sinkhorn_indices(d: torch.Tensor, epsilon: float, iters: int) -> torch.Tensor:
    """argmax of the Sinkhorn plan of a [B, K] fp32 distance matrix"""
    Q = sinkhorn_algorithm(center_distance_for_constraint(d).double(), epsilon, iters)
    if torch.isnan(Q).any() or torch.isinf(Q).any():
        warnings.warn("Sinkhorn Algorithm returns nan/inf values.")
    return torch.argmax(Q, dim=-1)


# ---- clustering -------------------------------------------------------------------------------------------------------------------
def constrained_km(data: np.ndarray, n_clusters: int = 10, init: bool = False, backend: str = "k_means_constrained"):
    """(centres [n_clusters, D] tensor, labels list) of the codes / latents in ``data``.  ``k_means_constrained`` is the
    reference's KMeansConstrained with its parameters; ``sklearn`` is plain KMeans(n_init=10, max_iter=10) - a deviation, it has
    no size bounds -, after which a cluster of fewer than two members is merged into the nearest other centre, so that every
    code has a positive to draw."""
    if backend == "k_means_constrained":
        try:
            from k_means_constrained import KMeansConstrained
        except ImportError as e:
            raise ImportError("the k_means_constrained package is not installed: install it, or choose --cluster_backend sklearn "
                              "(plain KMeans, no size bounds) or --cluster_backend none (needs beta == 0 and no kmeans_init)") from e
        size_min = min(len(data) // (n_clusters * 2), 50 if init else 10)
        clf = KMeansConstrained(n_clusters=n_clusters, size_min=size_min, size_max=size_min * 4 if init else n_clusters * 6,
                                max_iter=10, n_init=10, n_jobs=10, verbose=False)
        clf.fit(data)
        return torch.from_numpy(clf.cluster_centers_), torch.from_numpy(clf.labels_).tolist()
    if backend == "sklearn":
        from sklearn.cluster import KMeans
        clf = KMeans(n_clusters=min(n_clusters, len(data)), n_init=10, max_iter=10).fit(data)
        centers, labels = clf.cluster_centers_, clf.labels_.copy()
        if not init:
            counts = np.bincount(labels, minlength=len(centers))
            for c in np.nonzero(counts == 1)[0]:
                big = np.nonzero(counts >= 2)[0]
                if len(big) == 0:
                    break
                to = big[np.argmin(((centers[big] - centers[c]) ** 2).sum(-1))]
                labels[labels == c] = to
                counts[to] += 1
                counts[c] = 0
        return torch.from_numpy(centers), labels.tolist()
    raise ValueError(f"cluster backend {backend!r}: one of {CLUSTER_BACKENDS} ('none' does no clustering at all)")


def sample_positives(indices, labels, level: int = 0, rng=random):
    """The positives of one level as the reference draws them: per row, ``random.choice`` among the codes of the chosen code's
    cluster until another code comes up.  ``indices``: the level's chosen codes (a host sequence), ``labels``: the cluster of
    every code.  A cluster that holds no other code would spin forever in the reference: ValueError."""
    members: dict[int, list[int]] = {}
    for code, c in enumerate(labels):
        members.setdefault(c, []).append(code)
    out = []
    for row, code in enumerate(indices):
        code = int(code)
        pos = members[labels[code]]
        if all(p == code for p in pos):
            raise ValueError(f"diversity loss: at level {level} cluster {labels[code]} holds no code other than {code} (row {row}): "
                             "there is no positive to draw")
        choice = rng.choice(pos)
        while choice == code:
            choice = rng.choice(pos)
        out.append(choice)
    return out


# ---- layers -----------------------------------------------------------------------------------------------------------------------
class LinearActFn(torch.autograd.Function):
    """act(x w^T + b) for x [M, K], ``act`` a code of ops.ACTIVATIONS"""

    @staticmethod
    @ops.scoped_f32_matmul(lambda *a: "f32")
    def forward(ctx, x, w, b, act):
        x = x.contiguous()
        M, K = x.shape
        N = w.shape[0]
        pre = torch.empty(M, N, dtype=torch.float32, device=x.device)
        ops.linear_fwd(x, K, w, K, pre, N, M, N, K)
        out = pre if act == 0 else torch.empty_like(pre)
        ops.bias_act_fwd(pre, b, act, None if act == 0 else out)
        ctx.save_for_backward(x, w, None if act == 0 else pre)
        ctx.act = act
        return out

    @staticmethod
    @ops.scoped_f32_matmul(lambda *a: "f32")
    def backward(ctx, dout):
        x, w, pre = ctx.saved_tensors
        dx, dw, db = rec_common.linear_act_bwd(dout.contiguous().float().clone(), pre, x, w, ctx.act)
        return dx, dw, db, None


class MLPLayers(nn.Module):
    """Dropout(0), Linear, ReLU (none after the last) as the reference lays them out, so the Linears are ``mlp_layers.{1,4,..}``."""

    def __init__(self, layers: list[int]):
        super().__init__()
        self.layers = layers
        mods = []
        for i, (n_in, n_out) in enumerate(zip(layers[:-1], layers[1:])):
            mods.append(nn.Dropout(p=0.0))
            mods.append(nn.Linear(n_in, n_out))
            if i != len(layers) - 2:
                mods.append(nn.ReLU())
        self.mlp_layers = nn.Sequential(*mods)
        for m in self.mlp_layers:
            if isinstance(m, nn.Linear):
                nn.init.xavier_normal_(m.weight.data)
                m.bias.data.fill_(0.0)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if not x.is_cuda:
            raise RuntimeError("gamer_amd.rqvae runs on the HIP device only (no CPU fallback)")
        linears = [m for m in self.mlp_layers if isinstance(m, nn.Linear)]
        x = x.float()
        for i, m in enumerate(linears):
            act = ops.ACTIVATIONS["relu"] if i != len(linears) - 1 else ops.ACTIVATIONS["none"]
            x = LinearActFn.apply(x, m.weight, m.bias, act)
        return x


class VectorQuantizer(nn.Module):
    """Parameter holder of one level: ``embedding.weight`` [n_e, e_dim], and the level's Sinkhorn settings."""

    def __init__(self, n_e: int, e_dim: int, kmeans_init: bool, sk_epsilon: float, sk_iters: int):
        super().__init__()
        self.n_e, self.e_dim, self.sk_epsilon, self.sk_iters = n_e, e_dim, sk_epsilon, sk_iters
        self.embedding = nn.Embedding(n_e, e_dim)
        if not kmeans_init:
            self.initted = True
            self.embedding.weight.data.uniform_(-1.0 / n_e, 1.0 / n_e)
        else:
            self.initted = False
            self.embedding.weight.data.zero_()

    def init_emb(self, data: torch.Tensor, backend: str):
        centers, _ = constrained_km(data.detach().cpu().numpy(), 256, init=True, backend=backend)   # (256: the reference's constant)
        self.embedding.weight.data.copy_(centers)
        self.initted = True


def _run_levels(src, E, off, sk_eps, sk_iters, l0, l1, idx, xq, res, r_levels, sums):
    """Levels [l0, l1) on src [B, D]: the argmin levels between two Sinkhorn levels go in one launch each; returns the residual
    after level l1 - 1 (one of the two buffers ``res``)."""
    L = len(off) - 1
    modes = [0] * L
    cur = 0
    lvl = l0
    while lvl < l1:
        s = next((j for j in range(lvl, l1) if sk_eps[j] > 0), None)
        if s is None:
            ops.rvq_fwd(src, E, off, modes, lvl, l1, idx, xq, res[cur], r_levels, None, sums)
            return res[cur]
        d = torch.empty(src.shape[0], off[s + 1] - off[s], dtype=torch.float32, device=src.device)
        ops.rvq_fwd(src, E, off, modes, lvl, s + 1, idx, xq, res[cur], r_levels, d, sums)
        idx[:, s] = sinkhorn_indices(d, sk_eps[s], sk_iters).to(torch.int32)
        given = list(modes)
        given[s] = 1
        ops.rvq_fwd(res[cur], E, off, given, s, s + 1, idx, xq, res[1 - cur], r_levels, None, sums)
        src, lvl = res[1 - cur], s + 1              # (the next launch reads res[1 - cur] and writes res[cur])
    return src


class RVQFn(torch.autograd.Function):
    """(x_q [B, D], level_mse [L], indices int64 [B, L]) of the residual quantiser on z [B, D] with the packed codebooks E
    [sum K, D]; level_mse[l] = mse(e, sg r) + MU mse(sg e, r) of level l.  ``sk_eps[l] > 0``: level l takes its index from Sinkhorn."""

    @staticmethod
    def forward(ctx, z, E, off, sk_eps, sk_iters):
        z, E = z.contiguous().float(), E.contiguous()
        B, D = z.shape
        L = len(off) - 1
        dev = z.device
        f32 = dict(dtype=torch.float32, device=dev)
        idx = torch.empty(B, L, dtype=torch.int32, device=dev)
        xq = torch.empty(B, D, **f32)
        res = (torch.empty(B, D, **f32), torch.empty(B, D, **f32))
        keep = any(ctx.needs_input_grad[:2])
        r_levels = torch.empty(L, B, D, **f32) if keep else None
        sums = torch.zeros(L, **f32)
        _run_levels(z, E, off, sk_eps, sk_iters, 0, L, idx, xq, res, r_levels, sums)
        m = sums / float(B * D)
        if keep:
            ctx.save_for_backward(idx, r_levels, E)
            ctx.off = off
        idx64 = idx.long()
        ctx.mark_non_differentiable(idx64)
        return xq, m + MU * m, idx64

    @staticmethod
    def backward(ctx, g_xq, g_level, _g_idx):
        idx, r_levels, E = ctx.saved_tensors
        L, B, D = r_levels.shape
        g_level = torch.zeros(L, dtype=torch.float32, device=E.device) if g_level is None else g_level.contiguous().float()
        g_xq = None if g_xq is None else g_xq.contiguous().float()
        dz = torch.empty(B, D, dtype=torch.float32, device=E.device)
        dE = torch.empty_like(E)
        ops.rvq_bwd(idx, r_levels, E, ctx.off, g_xq, g_level, MU, dz, dE)
        return dz, dE, None, None, None


class ResidualVectorQuantizer(nn.Module):
    def __init__(self, n_e_list, e_dim, sk_epsilons, beta, kmeans_init, kmeans_iters, sk_iters, cluster_backend):
        super().__init__()
        self.n_e_list, self.e_dim, self.num_quantizers = n_e_list, e_dim, len(n_e_list)
        self.beta, self.kmeans_init, self.kmeans_iters, self.sk_epsilons, self.sk_iters = beta, kmeans_init, kmeans_iters, sk_epsilons, sk_iters
        self.cluster_backend = cluster_backend
        self.vq_layers = nn.ModuleList([VectorQuantizer(n_e, e_dim, kmeans_init, eps, sk_iters)
                                        for n_e, eps in zip(n_e_list, sk_epsilons)])
        self.last_positives = None

    def get_codebook(self) -> torch.Tensor:
        return torch.stack([q.embedding.weight for q in self.vq_layers])

    def _offsets(self):
        off = [0]
        for q in self.vq_layers:
            off.append(off[-1] + q.n_e)
        return off

    def _sk(self, use_sk: bool):
        return [float(q.sk_epsilon) if use_sk and q.sk_epsilon > 0 else 0.0 for q in self.vq_layers]

    @torch.no_grad()
    def vq_ini(self, x: torch.Tensor, use_sk: bool = True):
        """The reference's vq_ini: level by level, k-means initialisation of a level that is not initialised yet on the residual that
        reaches it, then that level's quantisation."""
        x = x.contiguous().float()
        B, D = x.shape
        off, sk = self._offsets(), self._sk(use_sk)
        L = self.num_quantizers
        f32 = dict(dtype=torch.float32, device=x.device)
        idx = torch.empty(B, L, dtype=torch.int32, device=x.device)
        xq, res = torch.empty(B, D, **f32), (torch.empty(B, D, **f32), torch.empty(B, D, **f32))
        src = x
        for l, q in enumerate(self.vq_layers):
            if not q.initted:
                q.init_emb(src, self.cluster_backend)
            E = torch.cat([v.embedding.weight.detach() for v in self.vq_layers])
            out = _run_levels(src, E, off, sk, self.sk_iters, l, l + 1, idx, xq, res, None, None)
            # (the next level must not write the buffer it reads: hand it the other one first)
            res = (res[1], res[0]) if out is res[0] else res
            src = out

    def diversity_loss(self, level: int, indices: torch.Tensor, y_true: torch.Tensor) -> torch.Tensor:
        """cross_entropy(e_idx . E^T with the own column at -1e12, y_true); gradients reach E through both factors"""
        emb = self.vq_layers[level].embedding.weight
        sim = torch.matmul(emb[indices], emb.t())
        sim = sim - torch.zeros_like(sim).scatter_(1, indices[:, None], 1e12)
        return F.cross_entropy(sim, y_true)

    def forward(self, x, labels, use_sk: bool = True, positives=None, with_loss: bool = True):
        """``with_loss=False`` (get_indices): the positives are still drawn, as the reference draws them there too - a seeded run
        keeps its stream of random numbers -, but no diversity loss is computed."""
        if self.training and any(not q.initted for q in self.vq_layers):
            self.vq_ini(x.detach(), use_sk=use_sk)
        E = torch.cat([q.embedding.weight for q in self.vq_layers])
        x_q, level_mse, indices = RVQFn.apply(x, E, self._offsets(), self._sk(use_sk), self.sk_iters)
        losses = [level_mse[l] for l in range(self.num_quantizers)]
        if self.beta > 0:
            if positives is None:
                host = indices.cpu().tolist()                                   # one copy for all levels
                positives = torch.tensor([sample_positives([row[l] for row in host], labels[str(l)], l)
                                          for l in range(self.num_quantizers)], device=x.device).t()
            positives = torch.as_tensor(positives, device=x.device).long()
            self.last_positives = positives
            for l in range(self.num_quantizers if with_loss else 0):
                losses[l] = losses[l] + self.beta * self.diversity_loss(l, indices[:, l], positives[:, l])
        return x_q, torch.stack(losses).mean(), indices


class RQVAE(nn.Module):
    def __init__(self, in_dim: int = 768, num_emb_list: list[int] = [256, 256, 256, 256], e_dim: int = 64,
                 layers: list[int] = [2048, 1024, 512, 256, 128, 64], dropout_prob: float = 0.0, bn: bool = False,
                 loss_type: str = "mse", quant_loss_weight: float = 1.0, kmeans_init: bool = False, kmeans_iters: int = 100,
                 sk_epsilons: list[float] = [0.0, 0.0, 0.0, 0.003], sk_iters: int = 50, alpha: float = 1.0, beta: float = 0.001,
                 n_clusters: int = 10, sample_strategy: str = "all", cf_embedding=0, cluster_backend: str = "k_means_constrained"):
        super().__init__()
        if bn:
            raise NotImplementedError("RQVAE on the HIP path: bn=True (BatchNorm1d in the MLPs) is not built")
        if dropout_prob > 0:
            raise NotImplementedError("RQVAE on the HIP path: dropout_prob > 0 is not built")
        ops.rvq_check_limits(num_emb_list, e_dim)
        if len(sk_epsilons) != len(num_emb_list):
            raise ValueError(f"sk_epsilons needs one value per level ({len(num_emb_list)}), got {len(sk_epsilons)}")
        if cluster_backend not in CLUSTER_BACKENDS:
            raise ValueError(f"cluster backend {cluster_backend!r}: one of {CLUSTER_BACKENDS}")
        if cluster_backend == "none" and (beta > 0 or kmeans_init):
            raise ValueError("cluster backend 'none' requires beta == 0 and kmeans_init=False")
        self.in_dim, self.num_emb_list, self.e_dim, self.layers = in_dim, num_emb_list, e_dim, layers
        self.dropout_prob, self.bn, self.loss_type, self.quant_loss_weight = dropout_prob, bn, loss_type, quant_loss_weight
        self.kmeans_init, self.kmeans_iters, self.sk_epsilons, self.sk_iters = kmeans_init, kmeans_iters, sk_epsilons, sk_iters
        self.cf_embedding, self.alpha, self.beta, self.n_clusters = cf_embedding, alpha, beta, n_clusters
        self.sample_strategy, self.cluster_backend = sample_strategy, cluster_backend

        self.encode_layer_dims = [in_dim] + list(layers) + [e_dim]
        self.encoder = MLPLayers(self.encode_layer_dims)
        self.rq = ResidualVectorQuantizer(num_emb_list, e_dim, sk_epsilons, beta, kmeans_init, kmeans_iters, sk_iters, cluster_backend)
        self.decode_layer_dims = self.encode_layer_dims[::-1]
        self.decoder = MLPLayers(self.decode_layer_dims)

    @property
    def args(self) -> Namespace:
        return Namespace(in_dim=self.in_dim, num_emb_list=self.num_emb_list, e_dim=self.e_dim, layers=self.layers,
                         dropout_prob=self.dropout_prob, bn=self.bn, loss_type=self.loss_type,
                         quant_loss_weight=self.quant_loss_weight, kmeans_init=self.kmeans_init, kmeans_iters=self.kmeans_iters,
                         sk_epsilons=self.sk_epsilons, sk_iters=self.sk_iters, alpha=self.alpha, beta=self.beta,
                         n_clusters=self.n_clusters, sample_strategy=self.sample_strategy)

    def forward(self, x, labels, use_sk: bool = True, positives=None):
        z = self.encoder(x)
        x_q, rq_loss, indices = self.rq(z, labels, use_sk=use_sk, positives=positives)
        return self.decoder(x_q), rq_loss, indices, x_q

    def CF_loss(self, quantized_rep: torch.Tensor, encoded_rep: torch.Tensor) -> torch.Tensor:
        labels = torch.arange(quantized_rep.size(0), dtype=torch.long, device=quantized_rep.device)
        return F.cross_entropy(torch.matmul(quantized_rep, encoded_rep.transpose(0, 1)), labels)

    @torch.no_grad()
    def vq_initialization(self, x: torch.Tensor, use_sk: bool = True):
        self.rq.vq_ini(self.encoder(x))

    @torch.no_grad()
    def get_indices(self, xs: torch.Tensor, labels=None, use_sk: bool = False) -> torch.Tensor:
        return self.rq(self.encoder(xs), labels, use_sk=use_sk, with_loss=False)[2]

    def compute_loss(self, out, quant_loss, emb_idx, dense_out, xs):
        if self.loss_type == "mse":
            loss_recon = F.mse_loss(out, xs, reduction="mean")
        elif self.loss_type == "l1":
            loss_recon = F.l1_loss(out, xs, reduction="mean")
        else:
            raise ValueError("incompatible loss type")
        rqvae_n_diversity_loss = loss_recon + self.quant_loss_weight * quant_loss
        if self.alpha > 0:
            rows = emb_idx.cpu().numpy() if torch.is_tensor(emb_idx) else np.asarray(emb_idx)
            cf = torch.from_numpy(np.asarray(self.cf_embedding)[rows]).to(dense_out.device)
            cf_loss = self.CF_loss(dense_out, cf)
        else:
            cf_loss = torch.tensor(0.0, device=dense_out.device)
        return rqvae_n_diversity_loss + self.alpha * cf_loss, cf_loss, loss_recon, quant_loss
