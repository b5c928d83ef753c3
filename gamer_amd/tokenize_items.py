"""``python -m gamer_amd.tokenize_items``: turn an RQ-VAE checkpoint into ``{dataset}.index.epoch{E}.alpha{a}-beta{b}.json``, item
number -> list of ``<a_i>`` .. ``<h_i>`` strings (the RQ-VAE branch of the reference's ``tokenize`` task, ref:SeqRec/tasks/tokenize.py).

A first pass over all items in batches of 1024 with ``use_sk=False``; then the reference's collision loop: at most 20 rounds, per
group of items that share an ID ``get_indices(..., use_sk=True)`` with the Sinkhorn epsilon 0 on all levels but the last and 0.003
on the last when it was 0.  Exact duplicates among the items keep colliding, as in the reference.  The checkpoint is the one
``python -m gamer_amd.train_rqvae`` or the reference's trainer wrote: its ``args`` may carry ``num_emb_list`` (what the trainers
write) or ``num_code_list`` (what the reference's tokenize task reads), and state-dict keys may carry DDP's ``module.`` prefix.
The RQ-KMeans, chunked-ID and random-ID branches of the task are not built.
"""
from __future__ import annotations

import argparse
import collections
import json
import os
import random
import sys
from collections import OrderedDict

import numpy as np
import torch

from .rqvae import CLUSTER_BACKENDS, RQVAE, constrained_km
from .train_rqvae import EmbDataset

PREFIX = ["<a_{}>", "<b_{}>", "<c_{}>", "<d_{}>", "<e_{}>", "<f_{}>", "<g_{}>", "<h_{}>"]
MAX_ROUNDS = 20


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="python -m gamer_amd.tokenize_items", description="Item tokenization with a trained RQ-VAE.")
    p.add_argument("--dataset", type=str, default="Instruments", help="Dataset name")
    p.add_argument("--data_path", type=str, required=True, help="Semantic embeddings path")
    p.add_argument("--output_dir", type=str, default="./data/", help="Output directory for tokenized data")
    p.add_argument("--root_path", type=str, default="./checkpoint/RQ-VAE", help="Root path to the RQ-VAE checkpoint")
    p.add_argument("--device", type=str, default="cuda:0", help="the HIP device")
    p.add_argument("--alpha", type=str, default="0.2", help="CF loss weight")
    p.add_argument("--beta", type=str, default="0.0001", help="Divergence loss weight")
    p.add_argument("--epoch", type=int, default=20000, help="The number of training epochs")
    p.add_argument("--checkpoint", type=str, default="best_collision_model.pth", help="The checkpoint file name")
    p.add_argument("--ckpt_path", type=str, default=None,
                   help="the checkpoint file itself, instead of root_path/dataset/alpha{a}-beta{b}/checkpoint")
    p.add_argument("--cluster_backend", type=str, default="k_means_constrained", choices=CLUSTER_BACKENDS,
                   help="the code labels the reference computes before tokenising (they only feed draws that are thrown away): "
                        "'none' skips them")
    return p


def load_model(ckpt_path: str, in_dim: int, device, cluster_backend: str = "none") -> tuple[RQVAE, argparse.Namespace]:
    ckpt = torch.load(ckpt_path, map_location=torch.device("cpu"), weights_only=False)
    ckpt_args, state_dict = ckpt["args"], ckpt["state_dict"]
    if all(k.startswith("module.") for k in state_dict.keys()):
        state_dict = OrderedDict((k[7:], v) for k, v in state_dict.items())
    num_emb_list = getattr(ckpt_args, "num_emb_list", None)
    if num_emb_list is None:
        num_emb_list = ckpt_args.num_code_list
    # (alpha and beta are not handed over, as in the reference: the model keeps its defaults; without labels there is nothing to draw)
    model = RQVAE(in_dim=in_dim, num_emb_list=list(num_emb_list), e_dim=ckpt_args.e_dim, layers=list(ckpt_args.layers),
                  dropout_prob=ckpt_args.dropout_prob, bn=ckpt_args.bn, loss_type=ckpt_args.loss_type,
                  quant_loss_weight=ckpt_args.quant_loss_weight, kmeans_init=False,         # (the codebooks come from the checkpoint)
                  kmeans_iters=ckpt_args.kmeans_iters, sk_epsilons=list(ckpt_args.sk_epsilons), sk_iters=ckpt_args.sk_iters,
                  cluster_backend=cluster_backend, **(dict(beta=0.0) if cluster_backend == "none" else {}))
    model.load_state_dict(state_dict, strict=False)
    return model.to(device).eval(), ckpt_args


def codes_of(indices: np.ndarray) -> list[list[str]]:
    return [[PREFIX[i].format(int(v)) for i, v in enumerate(row)] for row in indices]


def collision_groups(all_str: list[str]) -> list[list[int]]:
    where: dict[str, list[int]] = {}
    for i, s in enumerate(all_str):
        where.setdefault(s, []).append(i)
    return [g for g in where.values() if len(g) > 1]


def tokenize(model: RQVAE, embeddings: np.ndarray, labels, device, batch_size: int = 1024):
    """(codes: one list of strings per item, first-pass indices [N, L], rounds of the collision loop)"""
    x = torch.from_numpy(np.ascontiguousarray(embeddings, dtype=np.float32)).to(device)
    first = np.concatenate([model.get_indices(x[s:s + batch_size], labels, use_sk=False).cpu().numpy()
                            for s in range(0, len(x), batch_size)])
    all_codes = codes_of(first)
    all_str = [str(c) for c in all_codes]
    for q in model.rq.vq_layers[:-1]:
        q.sk_epsilon = 0.0
    if model.rq.vq_layers[-1].sk_epsilon == 0.0:
        model.rq.vq_layers[-1].sk_epsilon = 0.003
    rounds = 0
    while rounds < MAX_ROUNDS and len(set(all_str)) != len(all_str):
        groups = collision_groups(all_str)
        print(f"[tokenize_items] round {rounds}: {len(groups)} collision groups")
        for items in groups:
            idx = model.get_indices(x[torch.as_tensor(items, device=device)], labels, use_sk=True).cpu().numpy()
            for item, code in zip(items, codes_of(idx)):
                all_codes[item], all_str[item] = code, str(code)
        rounds += 1
    return all_codes, first, rounds


def run(a) -> str:
    random.seed(42), np.random.seed(42), torch.manual_seed(42)
    device = torch.device(a.device)
    if device.type != "cuda":
        raise RuntimeError("tokenize_items runs on the HIP device only (no CPU fallback)")
    data = EmbDataset(a.data_path)
    ckpt_path = a.ckpt_path or os.path.join(a.root_path, a.dataset, f"alpha{a.alpha}-beta{a.beta}", a.checkpoint)
    model, _ = load_model(ckpt_path, data.dim, device, a.cluster_backend)
    labels = None
    if a.cluster_backend != "none":
        labels = {str(i): constrained_km(q.embedding.weight.detach().cpu().numpy(), backend=a.cluster_backend)[1]
                  for i, q in enumerate(model.rq.vq_layers)}
    all_codes, _, rounds = tokenize(model, data.embeddings, labels, device)
    counts = collections.Counter(str(c) for c in all_codes)
    print(f"[tokenize_items] {len(all_codes)} items, {rounds} rounds, collision rate {1 - len(counts) / len(all_codes):.6f}, "
          f"largest group {max(counts.values())}")
    os.makedirs(a.output_dir, exist_ok=True)
    out = os.path.join(a.output_dir, f"{a.dataset}.index.epoch{a.epoch}.alpha{a.alpha}-beta{a.beta}.json")
    with open(out, "w") as fp:
        json.dump({i: c for i, c in enumerate(all_codes)}, fp)
    print(f"[tokenize_items] wrote {out}")
    return out


def main(argv=None) -> str:
    return run(build_parser().parse_args(argv))


if __name__ == "__main__":
    main(sys.argv[1:])
