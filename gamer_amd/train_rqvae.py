"""``python -m gamer_amd.train_rqvae``: train the RQ-VAE item tokenizer on item embeddings (the reference's task ``RQVAE``,
ref:SeqRec/tasks/RQVAE.py + SeqRec/trainers/RQVAE.py).

The flags and their defaults are the reference task's; ``--cluster_backend`` is new (see ``gamer_amd.rqvae.constrained_km``), and
``--bn`` / ``--kmeans_init`` read "false" / "0" / "no" as False (the reference's ``type=bool`` reads every non-empty string as
True).  The loop is the reference's: the k-means initialisation on the whole set, shuffled, as one batch when ``--kmeans_init`` is
set; per epoch new cluster labels of every codebook, then the batches; the collision rate over the whole set on epoch 0 and every
``eval_step`` epochs; checkpoints with the reference's keys and file names under ``ckpt_dir/<local time>/``, which
``python -m gamer_amd.tokenize_items`` and the reference's ``tokenize`` task both read.  Single GPU; no wandb.
"""
from __future__ import annotations

import argparse
import datetime
import os
import random
import sys
import time

import numpy as np
import torch
from torch import optim

from .rqvae import CLUSTER_BACKENDS, RQVAE, constrained_km


def _bool(s: str) -> bool:
    return str(s).strip().lower() not in ("", "0", "false", "no", "off")


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="python -m gamer_amd.train_rqvae", description="Train an RQ-VAE item tokenizer on the HIP engine.")
    p.add_argument("--seed", type=int, default=42, help="Random seed")
    p.add_argument("--lr", type=float, default=1e-3, help="learning rate")
    p.add_argument("--epochs", type=int, default=20000, help="number of epochs")
    p.add_argument("--batch_size", type=int, default=1024, help="batch size")
    p.add_argument("--num_workers", type=int, default=4, help="kept for the checkpoint's args; the data lives on the device")
    p.add_argument("--eval_step", type=int, default=2000, help="eval step")
    p.add_argument("--learner", type=str, default="AdamW", help="adam, adamw, sgd, adagrad or rmsprop (anything else: Adam)")
    p.add_argument("--data_path", type=str, default="data", help="Input data path (.npy of item embeddings).")
    p.add_argument("--weight_decay", type=float, default=1e-4, help="l2 regularization weight")
    p.add_argument("--dropout_prob", type=float, default=0.0, help="dropout ratio (only 0 is built)")
    p.add_argument("--bn", type=_bool, default=False, help="use batch norm or not (only False is built)")
    p.add_argument("--loss_type", type=str, default="mse", help="loss type: mse or l1")
    p.add_argument("--kmeans_init", type=_bool, default=True, help="use kmeans_init or not")
    p.add_argument("--kmeans_iters", type=int, default=100, help="max kmeans iters")
    p.add_argument("--sk_epsilons", type=float, nargs="+", default=[0.0, 0.0, 0.0, 0.003], help="sinkhorn epsilons")
    p.add_argument("--sk_iters", type=int, default=50, help="max sinkhorn iters")
    p.add_argument("--device", type=str, default="cuda:0", help="the HIP device")
    p.add_argument("--num_emb_list", type=int, nargs="+", default=[256, 256, 256, 256], help="emb num of every vq")
    p.add_argument("--e_dim", type=int, default=32, help="vq codebook embedding size")
    p.add_argument("--quant_loss_weight", type=float, default=1.0, help="vq quantion loss weight")
    p.add_argument("--alpha", type=float, default=0.2, help="cf loss weight")
    p.add_argument("--beta", type=float, default=0.0001, help="diversity loss weight")
    p.add_argument("--n_clusters", type=int, default=10, help="n_clusters")
    p.add_argument("--sample_strategy", type=str, default="all", help="sample strategy")
    p.add_argument("--cf_emb", type=str, default="./pretrained_ckpt/cf-embs/Instruments-32d-sasrec.pt", help="cf emb")
    p.add_argument("--layers", type=int, nargs="+", default=[2048, 1024, 512, 256, 128, 64], help="hidden sizes of every layer")
    p.add_argument("--ckpt_dir", type=str, default="./checkpoint/RQ-VAE", help="output directory for model")
    p.add_argument("--cluster_backend", type=str, default="k_means_constrained", choices=CLUSTER_BACKENDS,
                   help="constrained k-means of the code labels and of kmeans_init: the reference's package, plain sklearn KMeans "
                        "(no size bounds), or none (needs --beta 0 --kmeans_init False)")
    return p


class EmbDataset:
    """The item embeddings of a .npy file; a set whose standard deviation is below 0.2 is divided by it (the reference's rule)."""

    def __init__(self, data_path: str):
        self.data_path = data_path
        self.embeddings: np.ndarray = np.load(data_path)
        std = self.embeddings.std()
        if std < 0.2:
            print(f"[train_rqvae] standard deviation of the embeddings is low ({std:.4f}): dividing by it")
            self.embeddings /= std
        self.dim: int = self.embeddings.shape[-1]

    def __getitem__(self, index):
        return torch.FloatTensor(self.embeddings[index]), index

    def __len__(self):
        return len(self.embeddings)


def get_local_time() -> str:
    return datetime.datetime.now().strftime("%b-%d-%Y_%H-%M-%S")


def build_optimizer(model, learner: str, lr: float, weight_decay: float) -> optim.Optimizer:
    params, name = model.parameters(), learner.lower()
    if name == "adam":
        return optim.Adam(params, lr=lr, weight_decay=weight_decay)
    if name == "sgd":
        return optim.SGD(params, lr=lr, weight_decay=weight_decay)
    if name == "adagrad":
        return optim.Adagrad(params, lr=lr, weight_decay=weight_decay)
    if name == "rmsprop":
        return optim.RMSprop(params, lr=lr, weight_decay=weight_decay)
    if name == "adamw":
        return optim.AdamW(params, lr=lr, weight_decay=weight_decay)
    print("[train_rqvae] unrecognized optimizer, using Adam")
    return optim.Adam(params, lr=lr)


def collision_rate(codes: np.ndarray) -> float:
    """(rows - distinct rows) / rows of an [N, L] array of indices"""
    return (len(codes) - len({"-".join(str(int(v)) for v in row) for row in codes})) / len(codes)


class Trainer:
    def __init__(self, model: RQVAE, a, data: EmbDataset, device):
        self.model, self.a, self.device = model, a, device
        self.epochs, self.eval_step, self.batch_size = a.epochs, min(a.eval_step, a.epochs), a.batch_size
        self.ckpt_dir = os.path.join(a.ckpt_dir, get_local_time())
        os.makedirs(self.ckpt_dir, exist_ok=True)
        self.x = torch.from_numpy(np.ascontiguousarray(data.embeddings, dtype=np.float32)).to(device)
        self.labels = {str(i): [] for i in range(6)}
        self.best_loss = self.best_collision_rate = np.inf
        self.best_collision_ckpt = "best_collision_model.pth"
        self.optimizer = build_optimizer(model, a.learner, a.lr, a.weight_decay)
        self.saved = []

    def relabel(self):
        if self.model.cluster_backend == "none":
            return
        for i, q in enumerate(self.model.rq.vq_layers):
            _, self.labels[str(i)] = constrained_km(q.embedding.weight.detach().cpu().numpy(), backend=self.model.cluster_backend)

    def vq_init(self):
        self.model.eval()
        perm = torch.randperm(len(self.x), device=self.device)
        self.model.vq_initialization(self.x[perm])

    def train_step(self, rows: torch.Tensor):
        data = self.x[rows]
        self.optimizer.zero_grad()
        out, rq_loss, _, dense_out = self.model(data, self.labels)
        loss, cf_loss, recon, quant = self.model.compute_loss(out, rq_loss, rows.cpu(), dense_out, xs=data)
        if torch.isnan(loss):
            raise ValueError("Training loss is nan")
        loss.backward()
        self.optimizer.step()
        return loss.item(), recon.item(), cf_loss.item(), quant.item()

    def train_epoch(self):
        self.model.train()
        self.relabel()
        totals = np.zeros(4)
        perm = torch.randperm(len(self.x), device=self.device)
        for s in range(0, len(perm), self.batch_size):
            totals += self.train_step(perm[s:s + self.batch_size])
        return totals

    @torch.no_grad()
    def valid_epoch(self) -> float:
        self.model.eval()
        self.relabel()
        codes = [self.model.get_indices(self.x[s:s + self.batch_size], self.labels).cpu().numpy()
                 for s in range(0, len(self.x), self.batch_size)]
        return collision_rate(np.concatenate(codes))

    @property
    def args(self) -> argparse.Namespace:
        args = self.model.args
        a = self.a
        args.lr, args.epochs, args.num_workers, args.eval_step = a.lr, self.epochs, a.num_workers, self.eval_step
        args.learner, args.data_path, args.weight_decay, args.ckpt_dir = a.learner, a.data_path, a.weight_decay, self.ckpt_dir
        return args

    def save_checkpoint(self, epoch: int, rate: float = 1, ckpt_file: str | None = None) -> str:
        path = os.path.join(self.ckpt_dir, ckpt_file or f"epoch_{epoch}_collision_{rate:.4f}_model.pth")
        state = {"args": self.args, "epoch": epoch, "best_loss": self.best_loss, "best_collision_rate": self.best_collision_rate,
                 "state_dict": self.model.state_dict(), "optimizer": self.optimizer.state_dict()}
        torch.save(state, path, pickle_protocol=4)
        self.saved.append(path)
        print(f"[train_rqvae] saved {path}")
        return path

    def fit(self):
        if self.model.kmeans_init:
            self.vq_init()
        for epoch in range(self.epochs):
            loss, recon, cf, quant = self.train_epoch()
            self.last_losses = (loss, recon, cf, quant)
            self.best_loss = min(self.best_loss, loss)
            if (epoch + 1) % self.eval_step == 0 or epoch == 0:
                t0 = time.time()
                rate = self.valid_epoch()
                if rate < self.best_collision_rate:
                    self.best_collision_rate = rate
                    self.save_checkpoint(epoch, rate, self.best_collision_ckpt)
                print(f"[train_rqvae] epoch {epoch}: loss {loss:.6f} recon {recon:.6f} cf {cf:.6f} quant {quant:.6f}; "
                      f"collision_rate {rate:.4f} ({time.time() - t0:.2f}s)")
                self.last_collision_rate = rate
                self.save_checkpoint(epoch, rate)
        return self.best_loss, self.best_collision_rate


def run(a) -> Trainer:
    random.seed(a.seed), np.random.seed(a.seed), torch.manual_seed(a.seed)
    device = torch.device(a.device)
    if device.type != "cuda":
        raise RuntimeError("train_rqvae runs on the HIP device only (no CPU fallback)")
    data = EmbDataset(a.data_path)
    if os.path.exists(a.cf_emb):
        cf = torch.load(a.cf_emb, map_location="cpu").squeeze().detach().numpy()
    else:
        cf = np.zeros((len(data), a.e_dim), dtype=np.float32)
    model = RQVAE(in_dim=data.dim, num_emb_list=a.num_emb_list, e_dim=a.e_dim, layers=a.layers, dropout_prob=a.dropout_prob,
                  bn=a.bn, loss_type=a.loss_type, quant_loss_weight=a.quant_loss_weight, kmeans_init=a.kmeans_init,
                  kmeans_iters=a.kmeans_iters, sk_epsilons=a.sk_epsilons, sk_iters=a.sk_iters, alpha=a.alpha, beta=a.beta,
                  n_clusters=a.n_clusters, sample_strategy=a.sample_strategy, cf_embedding=cf,
                  cluster_backend=a.cluster_backend).to(device)
    trainer = Trainer(model, a, data, device)
    best_loss, best_rate = trainer.fit()
    print(f"[train_rqvae] best loss {best_loss}, best collision rate {best_rate}")
    return trainer


def main(argv=None) -> Trainer:
    return run(build_parser().parse_args(argv))


if __name__ == "__main__":
    main(sys.argv[1:])
