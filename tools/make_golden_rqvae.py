#!/usr/bin/env python3
"""Golden fixture of the RQ-VAE item tokenizer, generated from the REAL reference classes.

Builds ``SeqRec.models.tokenizer.RQVAE.RQVAE`` (ref:SeqRec/models/tokenizer/RQVAE/model.py) on the CPU at in_dim 24, layers
[32, 16], e_dim 8, num_emb_list [20, 24, 20, 32], B = 37, with the codebooks re-drawn N(0, 0.05) so that every level matters, in
two configurations:
  a/   sk_epsilons all 0, alpha = beta = 0
  b/   the shipped form: sk_epsilons [0, 0, 0, 0.003], sk_iters 50, alpha 0.2, beta 1e-4, labels j % 10, a fixed ``random.seed``,
       a random cf_embedding
and records for each: the state dict (and its key list), the input, the labels, the positives the reference drew, ``out``, ``x_q``,
``indices``, the four loss values, every parameter gradient, ``get_indices`` with use_sk False and with use_sk True on a 5-row
group; for b/ also the [B, K] distance matrix and the Sinkhorn ``Q`` of the last level.  The same model in fp64 gives the
reference's own fp32 error for every compared quantity (``meta_json``: what a test bar may be derived from).

It asserts, and stores, in fp64: per row and argmin level the relative gap between the best and the second-best distance
(>= 1e-4, so a test may demand the indices exactly; the fp32 and fp64 argmin agree), and per row the relative gap between the best
and second-best ``Q`` entry of the Sinkhorn level (>= 1e-2: an fp32 rounding of the distances, 1e-6 of a centred distance, moves a
``Q`` entry by exp(1e-6 / 0.003) - 1 = 3e-4).  The 5-row group has fewer rows than codes, so a row owns several columns outright and
their entries differ only by leakage: there the gap must be >= 1e-9 (fp64 noise is 1e-15), and for both the argmax must survive 20
draws of relative noise 1e-6 on the distance matrix.  Seeds are tried from the given one until every assertion holds.

Usage:  python tools/make_golden_rqvae.py [seed]      (needs the reference checkout; CPU only)
"""
import importlib.machinery
import json
import os
import random
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import _ref_loader  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "rqvae_small.npz")
IN_DIM, LAYERS, E_DIM, NUM_EMB, B = 24, [32, 16], 8, [20, 24, 20, 32], 37
GROUP = [3, 11, 12, 20, 36]
PY_SEED = 1234
CONFIGS = {
    "a": dict(sk_epsilons=[0.0, 0.0, 0.0, 0.0], sk_iters=50, alpha=0.0, beta=0.0),
    "b": dict(sk_epsilons=[0.0, 0.0, 0.0, 0.003], sk_iters=50, alpha=0.2, beta=1e-4),
}


def reference_rqvae():
    _ref_loader._install_shims()
    ref = _ref_loader.REF_ROOT
    for parent in ("SeqRec", "SeqRec.models", "SeqRec.models.tokenizer", "SeqRec.utils"):
        if parent not in sys.modules:
            pkg = types.ModuleType(parent)
            pkg.__path__ = [os.path.join(ref, *parent.split("."))]
            pkg.__spec__ = importlib.machinery.ModuleSpec(parent, None, is_package=True)
            pkg.__spec__.submodule_search_locations = pkg.__path__
            sys.modules[parent] = pkg
    from SeqRec.models.tokenizer.RQVAE import vector_quantizer as vqm
    from SeqRec.models.tokenizer.RQVAE.model import RQVAE
    return RQVAE, vqm


def task_defaults():
    import argparse
    ref = _ref_loader.REF_ROOT
    for parent in ("SeqRec.tasks", "SeqRec.datasets"):
        if parent not in sys.modules:
            pkg = types.ModuleType(parent)
            pkg.__path__ = [os.path.join(ref, *parent.split("."))]
            pkg.__spec__ = importlib.machinery.ModuleSpec(parent, None, is_package=True)
            pkg.__spec__.submodule_search_locations = pkg.__path__
            sys.modules[parent] = pkg
    from SeqRec.tasks.RQVAE import TrainRQVAE
    parser = argparse.ArgumentParser()
    TrainRQVAE.add_sub_parsers(parser.add_subparsers())
    return vars(parser.parse_args(["RQVAE"]))


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-300))


def sinkhorn_argmax_is_stable(vqm_real, d, eps, iters, trials=20):
    """whether the argmax of the Sinkhorn plan survives an fp32 rounding of the distances: relative noise of 1e-6 on d.  (With
    fewer rows than codes a row owns several columns outright - entries of 1 / K up to a leakage of 1e-9 and less -, and the
    relative gap between two such entries says little: what decides is whether their order survives the perturbation.)"""
    center, sk = vqm_real
    ref = sk(center(d).double(), eps, iters).argmax(-1)
    g = torch.Generator().manual_seed(99)
    for _ in range(trials):
        dn = d * (1 + 1e-6 * torch.randn(d.shape, generator=g))
        if not torch.equal(sk(center(dn).double(), eps, iters).argmax(-1), ref):
            return False
    return True


def build(RQVAE, cfg, seed, cf):
    torch.manual_seed(seed)
    model = RQVAE(in_dim=IN_DIM, num_emb_list=NUM_EMB, e_dim=E_DIM, layers=LAYERS, kmeans_init=False, cf_embedding=cf, **cfg)
    for q in model.rq.vq_layers:
        q.embedding.weight.data.normal_(0.0, 0.05)
    return model


def run(model, x, labels, emb_idx):
    model.train()
    model.zero_grad()
    random.seed(PY_SEED)
    out, rq_loss, indices, x_q = model(x, labels)
    total, cf_loss, recon, quant = model.compute_loss(out, rq_loss, emb_idx, x_q, xs=x)
    total.backward()
    grads = {k: p.grad.detach().clone() for k, p in model.named_parameters()}
    return dict(out=out.detach(), x_q=x_q.detach(), indices=indices.detach(),
                losses=torch.stack([total.detach(), cf_loss.detach(), recon.detach(), quant.detach()])), grads


def main():
    first = int(sys.argv[1]) if len(sys.argv) > 1 else 0
    RQVAE, vqm = reference_rqvae()
    real = (vqm.center_distance_for_constraint, vqm.sinkhorn_algorithm, vqm.VectorQuantizer.diversity_loss)
    for seed in range(first, first + 200):
        try:
            return generate(RQVAE, vqm, real, seed)
        except AssertionError as e:
            print(f"seed {seed}: {e}")
    raise SystemExit("no seed passed")


def generate(RQVAE, vqm, real, seed):
    rec = {}
    meta = dict(in_dim=IN_DIM, layers=LAYERS, e_dim=E_DIM, num_emb_list=NUM_EMB, B=B, seed=seed, py_seed=PY_SEED, group=GROUP,
                configs=CONFIGS, mu=0.25, loss_order=["total", "cf", "recon", "quant"])
    g = torch.Generator().manual_seed(seed + 100)
    x = torch.randn(B, IN_DIM, generator=g)
    cf = torch.randn(B, E_DIM, generator=g).numpy()
    emb_idx = torch.arange(B)
    labels = {str(l): [j % 10 for j in range(k)] for l, k in enumerate(NUM_EMB)}
    rec["x"], rec["cf_embedding"] = x.numpy(), cf
    rec["labels_json"] = np.array(json.dumps(labels))

    # what the real classes hand to / get from Sinkhorn, and what random.choice returned to the diversity loss
    seen = {}
    real_center, real_sk, real_div = real

    def center(d):
        seen["d"] = d.detach().clone()
        return real_center(d)

    def sk(d, eps, it):
        seen["Q"] = real_sk(d, eps, it).clone()
        return seen["Q"].clone()

    def div(self, x_q, indices, indices_cluster, indices_list):
        state = random.getstate()
        loss = real_div(self, x_q, indices, indices_cluster, indices_list)
        random.setstate(state)                                  # draw again, this time keeping the values
        pos = []
        for i, c in enumerate(indices_cluster):
            e = random.choice(indices_list[c])
            while e == indices[i]:
                e = random.choice(indices_list[c])
            pos.append(e)
        seen.setdefault("positives", []).append(pos)
        return loss

    vqm.center_distance_for_constraint, vqm.sinkhorn_algorithm, vqm.VectorQuantizer.diversity_loss = center, sk, div

    for name, cfg in CONFIGS.items():
        seen.clear()
        model = build(RQVAE, cfg, seed, cf)
        sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
        res, grads = run(model, x, labels, emb_idx)
        L = len(NUM_EMB)
        if cfg["beta"] > 0:
            rec[f"{name}/positives"] = np.array(seen["positives"][:L], dtype=np.int64).T            # [B, L]
        else:
            assert "positives" not in seen
        if cfg["sk_epsilons"][-1] > 0:
            rec[f"{name}/dist_last"], rec[f"{name}/Q_last"] = seen["d"].numpy(), seen["Q"].numpy()
            top = torch.topk(seen["Q"], 2, dim=-1).values
            qgap = ((top[:, 0] - top[:, 1]) / top[:, 0]).numpy()
            assert qgap.min() >= 1e-2, f"Q gap {qgap.min():.3e} < 1e-2: pick another seed"
            assert sinkhorn_argmax_is_stable((real_center, real_sk), seen["d"], cfg["sk_epsilons"][-1], cfg["sk_iters"])
            assert torch.equal(seen["Q"].argmax(-1), res["indices"][:, -1])
            rec[f"{name}/q_gap"] = qgap
            meta[f"{name}_min_q_gap"] = float(qgap.min())

        # fp64 chain along the reference's indices: the gaps, and the agreement of the fp32 and fp64 argmin
        m64 = build(RQVAE, cfg, seed, cf.astype(np.float64)).double()
        r = m64.encoder(x.double()).detach()
        gaps = np.full((B, L), np.inf)
        for l, q in enumerate(m64.rq.vq_layers):
            E = q.embedding.weight.detach()
            d = (r ** 2).sum(1, keepdim=True) + (E ** 2).sum(1)[None] - 2 * r @ E.t()
            if cfg["sk_epsilons"][l] == 0:
                two = torch.topk(d, 2, dim=-1, largest=False).values
                gaps[:, l] = ((two[:, 1] - two[:, 0]) / two[:, 0]).numpy()
                assert torch.equal(d.argmin(-1), res["indices"][:, l]), f"fp32 and fp64 argmin differ at level {l}"
            r = r - E[res["indices"][:, l]]
        assert gaps.min() >= 1e-4, f"distance gap {gaps.min():.3e} < 1e-4: pick another seed"
        rec[f"{name}/dist_gap"] = gaps
        meta[f"{name}_min_dist_gap"] = float(gaps.min())

        # the reference's own fp32 error: the same model and step in fp64
        seen.clear()
        res64, grads64 = run(m64, x.double(), labels, emb_idx)
        assert torch.equal(res64["indices"], res["indices"])
        meta[f"{name}_ref_err"] = dict(out=rel(res["out"], res64["out"]), x_q=rel(res["x_q"], res64["x_q"]),
                                       losses=[abs(float(a) - float(b)) / max(abs(float(b)), 1e-300)
                                               for a, b in zip(res["losses"], res64["losses"])],
                                       grads={k: rel(grads[k], grads64[k]) for k in grads})
        rec[f"{name}/losses64"] = res64["losses"].numpy()

        model.eval()
        seen.clear()
        rec[f"{name}/get_indices"] = model.get_indices(x, labels, use_sk=False).numpy()
        # the collision loop's call: sk_epsilon 0 on all levels but the last, 0.003 there when it was 0
        for q in model.rq.vq_layers[:-1]:
            q.sk_epsilon = 0.0
        if model.rq.vq_layers[-1].sk_epsilon == 0.0:
            model.rq.vq_layers[-1].sk_epsilon = 0.003
        rec[f"{name}/get_indices_sk_group"] = model.get_indices(x[GROUP], labels, use_sk=True).numpy()
        gtop = torch.topk(seen["Q"], 2, dim=-1).values
        rec[f"{name}/group_q_gap"] = ((gtop[:, 0] - gtop[:, 1]) / gtop[:, 0]).numpy()
        meta[f"{name}_group_min_q_gap"] = float(rec[f"{name}/group_q_gap"].min())
        assert meta[f"{name}_group_min_q_gap"] >= 1e-9, f"Q gap of the 5-row group {meta[name + '_group_min_q_gap']:.3e} < 1e-9"
        assert sinkhorn_argmax_is_stable((real_center, real_sk), seen["d"], 0.003, cfg["sk_iters"]), "the 5-row group's argmax moves"

        for k, v in sd.items():
            rec[f"{name}/sd/{k}"] = v.numpy()
        for k, v in grads.items():
            rec[f"{name}/grad/{k}"] = v.numpy()
        for k, v in res.items():
            rec[f"{name}/{k}"] = v.numpy()
        meta[f"{name}_keys"] = list(sd.keys())
        meta[f"{name}_shapes"] = {k: list(v.shape) for k, v in sd.items()}
        print(f"[{name}] min distance gap {gaps.min():.3e}; losses {res['losses'].tolist()}; "
              f"reference fp32 error: out {meta[f'{name}_ref_err']['out']:.2e}, worst grad "
              f"{max(meta[f'{name}_ref_err']['grads'].values()):.2e}")

    # the defaults of the real task's parser (settings only: the tests compare the command's parser against them)
    meta["task_defaults"] = task_defaults()
    rec["meta_json"] = np.array(json.dumps(meta))
    np.savez_compressed(OUT, **rec)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
