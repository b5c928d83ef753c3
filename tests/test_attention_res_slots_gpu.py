"""Resident-K/V attention kernels (csrc/attention_res.hip): every slot of the resident images and of their metadata arrays, one at a time.

The key / query-tile loops of these kernels read their LDS images through per-lane pointers that move one tile per trip, with the image,
the half of the block and the row group of a read in the instruction's immediate.  A wrong base, step or immediate reads another tile's
(or another image's) slot - but in a run over causal data most of such a mix-up still lands on keys the row may see, and shows as a
rounding-sized error.  Here the levels are built so that, for t = 0..9, ONLY the keys of key tile t are allowed, for the queries
behind them: every other key is blocked by its level and the queries in front of the tile are "empty" rows.  The whole result then
sits in the slots of tile t, once, and a read that goes anywhere else is an error of order one.

S = 300: two key blocks of 256 (tiles 0-7 both 64 KB halves of the forward's block, tiles 8-9 the second pass with the carried
softmax state), three query blocks of 128 slots in the dK / dV kernel, a ragged last tile of 12 keys.  Reference: a dense fp64 attention
with the kernels' dropout mask, at the bars of tests/test_attention_res_gpu.py."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

from gamer_amd import ops  # noqa: E402

B, S, NQ, NKV, SCALE, SEED = 2, 300, 6, 3, 0.125, (7 << 32) | 4242
DEV = "cuda"
_inputs = {}


def _mix32(x):
    x = x.astype(np.uint64) & 0xffffffff
    x ^= x >> 16
    x = (x * 0x7feb352d) & 0xffffffff
    x ^= x >> 15
    x = (x * 0x846ca68b) & 0xffffffff
    x ^= x >> 16
    return x


def _keep_mult(p, seed):
    """AttnDropout of csrc/common.h: 0 or 1 / (1 - p) per (b, head, query, key), keep = low32(row word * key word) >= p 2^32"""
    one = lambda v: _mix32(np.array([v & 0xffffffff], dtype=np.uint64))[0]
    k0 = one((seed & 0xffffffff) ^ 0x9e3779b9) ^ one((seed >> 32) + 0x7f4a7c15)
    k1 = one(int(k0) + 0x632be5ab)
    thr = np.uint64(int(np.float32(p) * np.float32(4294967296.0)))
    rows = np.arange(B * NQ * S, dtype=np.uint64)
    a = (_mix32((rows * np.uint64(0x9e3779b1) + k0) & np.uint64(0xffffffff)) & np.uint64(0xffffff)) | np.uint64(0x800001)
    keys = np.arange(S, dtype=np.uint64)
    w = _mix32((keys * np.uint64(0x85ebca6b) + k1) & np.uint64(0xffffffff)) & np.uint64(0xffffff)
    keep = ((a[:, None] * w[None, :]) & np.uint64(0xffffffff)) >= thr
    scale = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
    return torch.from_numpy(np.where(keep, scale, 0.0)).reshape(B, NQ, S, S)


def _tensors():
    """q, k, v, dO of every case (and their copies on the device): made once"""
    if not _inputs:
        g = torch.Generator().manual_seed(300)
        for name, h in (("q", NQ), ("k", NKV), ("v", NKV), ("d_o", NQ)):
            _inputs[name] = torch.randn(B, S, h, 64, generator=g)
        T = B * S
        qkv = torch.zeros(T, (NQ + 2 * NKV) * 64, device=DEV)          # v lives inside a q|k|v buffer, as in the model
        qkv[:, (NQ + NKV) * 64:] = _inputs["v"].reshape(T, -1).to(DEV)
        _inputs["dev"] = dict(q=_inputs["q"].reshape(T, -1).to(DEV), k=_inputs["k"].reshape(T, -1).to(DEV), qkv=qkv,
                              d_o=_inputs["d_o"].reshape(T, -1).to(DEV))
    return _inputs


@pytest.mark.parametrize("p_drop", [0.0, 0.25])
@pytest.mark.parametrize("t", range(10))
def test_only_the_keys_of_one_tile_are_allowed(t, p_drop):
    import test_ops_gpu as H
    x = _tensors()
    d = x["dev"]
    T = B * S
    pos = torch.arange(S)
    in_tile = (pos >= 32 * t) & (pos < 32 * t + 32)
    kl = torch.where(in_tile, 0, 1).int().expand(B, S).contiguous()               # a key of another tile: level 1, not below any query's
    ql = torch.ones(B, S, dtype=torch.int32)
    ok = ((pos[None, :] <= pos[:, None]) & in_tile[None, :]).expand(B, S, S)      # [b, query, key]
    row_empty = (~ok.any(-1)).int().contiguous()                                   # the queries in front of the tile
    n_t = (S + 31) // 32
    pad = torch.zeros(B, n_t * 32, dtype=torch.int32)
    pad[:, :S] = row_empty
    tile_empty = pad.view(B, n_t, 32).amax(-1).int().contiguous()

    leaves = [x[n].double().requires_grad_(True) for n in ("q", "k", "v")]
    mult = _keep_mult(p_drop, SEED) if p_drop > 0 else None
    o_ref, _, _ = H._attn_ref(*leaves, ok, NQ, NKV, SCALE, mult=None if mult is None else mult)
    (o_ref * x["d_o"].double()).sum().backward()

    ldv = d["qkv"].shape[1]
    v = d["qkv"][:, (NQ + NKV) * 64:]
    nan = float("nan")
    o, lse = torch.full((T, NQ * 64), nan, device=DEV), torch.full((B, NQ, S), nan, device=DEV)
    delta = torch.zeros(B, NQ, S, device=DEV)
    dq, dk = torch.full((T, NQ * 64), nan, device=DEV), torch.full((T, NKV * 64), nan, device=DEV)
    dqkv = torch.zeros(T, ldv, device=DEV)
    dv = dqkv[:, (NQ + NKV) * 64:]
    kl_d, ql_d, re_d, te_d = (a.to(DEV) for a in (kl, ql, row_empty, tile_empty))
    with ops.env_switches(GAMER_ATTN_RES=1, GAMER_ATTN_RES_GRID=3, GAMER_ATTN_RES_SPLIT=0):
        ops.attn_fwd_split(d["q"], NQ * 64, d["k"], NKV * 64, v, ldv, kl_d, ql_d, re_d, B, S, NQ, NKV, SCALE, p_drop, SEED, o, lse, h2=True)
        ops.attn_bwd_split(d["q"], NQ * 64, d["k"], NKV * 64, v, ldv, o, d["d_o"], lse, kl_d, ql_d, re_d, te_d, B, S, NQ, NKV, SCALE,
                           p_drop, SEED, delta, dq, NQ * 64, dk, NKV * 64, dv, ldv, h2=True)
        torch.cuda.synchronize()
    e = dict(o=H._rel(o, o_ref.reshape(T, -1)), dq=H._rel(dq, leaves[0].grad.reshape(T, -1)),
             dk=H._rel(dk, leaves[1].grad.reshape(T, -1)), dv=H._rel(dv, leaves[2].grad.reshape(T, -1)))
    print(f"tile {t} p_drop {p_drop}: " + " ".join(f"{k_} {v_:.2e}" for k_, v_ in e.items()))
    assert e["o"] < 2e-5
    assert e["dq"] < 5e-5
    assert e["dk"] < 5e-5
    assert e["dv"] < 5e-5
