"""MBHT's kernels and model on the GPU: the linear attention, the sequence-axis Linear and one multi-scale layer against fp64 torch
restatements of the reference's formulas written here, and the model against the real reference class
(tests/golden/mbht_small.npz, tools/make_golden_mbht.py).

Bars: the ones of this project's MBSTR tests, which pin the same kind of kernels (fp32 FMA chains of at most a few hundred terms):
2e-5 of the largest magnitude for outputs, 2e-4 for gradients, 1e-5 for the loss.  Every kernel test also prints the error of the
same mathematics as fp32 torch ops against the same fp64 values."""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import mbht_weights as mw  # noqa: E402

from gamer_amd import mbht, ops  # noqa: E402

pytestmark = pytest.mark.gpu
FX = os.path.join(os.path.dirname(__file__), "golden", "mbht_small.npz")
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("needs the GPU")
    from gamer_amd import build
    build.build()


def _rel(got, ref):
    got, ref = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(ref).detach().double().cpu()
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def _mix32(x):
    x = x.astype(np.uint64) & 0xffffffff
    x ^= x >> 16
    x = (x * 0x7feb352d) & 0xffffffff
    x ^= x >> 15
    x = (x * 0x846ca68b) & 0xffffffff
    x ^= x >> 16
    return x


def _keep_mask(p, seed, n):
    """DropoutRng::mult of csrc/common.h for the counters 0 .. n - 1: 0 or 1 / (1 - p)"""
    k0 = _mix32(np.array([(seed & 0xffffffff) ^ 0x9e3779b9]))[0]
    k1 = _mix32(np.array([((seed >> 32) + 0x85ebca6b) & 0xffffffff]))[0]
    thr = np.uint64(int(np.float32(p) * np.float32(4294967296.0)))
    idx = np.arange(n, dtype=np.uint64)
    hsh = _mix32((idx & 0xffffffff) ^ k0)
    hsh = _mix32((hsh + (idx >> np.uint64(32)) * 0x9e3779b1 + k1) & 0xffffffff)
    scale = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
    return torch.from_numpy(np.where(hsh >= thr, scale, 0.0))


# ---- the linear attention -------------------------------------------------------------------------------------------------------
def _linear_attention(q, k, v, keep, Ew, Eb, Fw, Fb, mult=None):
    """LinearAttention.forward's core in the dtype of its inputs: q, k, v [B, h, L, d]; keep [B, L] 0 / 1; mult [B, h, L, c]"""
    m = keep.to(q.dtype)[:, None, :, None]
    k, v = k * m, v * m
    vp = (v.transpose(2, 3) @ Ew.t() + Eb).transpose(2, 3)                       # E(value^T)^T: [B, h, c, d]
    kp = (k.transpose(2, 3) @ Fw.t() + Fb).transpose(2, 3)
    p = torch.softmax(q @ kp.transpose(-2, -1) * math.sqrt(1.0 / q.shape[-1]), dim=-1)
    if mult is not None:
        p = p * mult.to(q.dtype)
    return p @ vp


def _msa_case(L, d, c, B, p=0.0, seed=0, h=2, n_partial=None, poison=False):
    g = torch.Generator().manual_seed(1000 * L + 10 * d + c + B)
    H = h * d
    qkv = torch.randn(B * L, 3 * H, generator=g)
    lens = ([L, 0] + [int(torch.randint(1, L + 1, (1,), generator=g)) for _ in range(B)])[:B]     # no padding; fully padded
    if B == 1:
        lens = [max(1, L - 3)]
    keep = torch.zeros(B, L, dtype=torch.int32)
    for b, n in enumerate(lens):
        keep[b, :n] = 1
    Ew, Fw = 0.4 * torch.randn(c, L, generator=g), 0.4 * torch.randn(c, L, generator=g)
    Eb, Fb = 0.3 * torch.randn(c, generator=g), 0.3 * torch.randn(c, generator=g)
    d_o = torch.randn(B * L, H, generator=g)
    mult = _keep_mask(p, seed, B * h * L * c).reshape(B, h, L, c) if p > 0 else None
    # fp64 (and fp32 torch) restatement
    res = {}
    for dt in (torch.float64, torch.float32):
        t = [x.to(dt).requires_grad_(True) for x in (qkv, Ew, Eb, Fw, Fb)]
        heads = lambda x: x.view(B, L, h, d).permute(0, 2, 1, 3)
        o = _linear_attention(heads(t[0][:, :H]), heads(t[0][:, H:2 * H]), heads(t[0][:, 2 * H:]), keep, t[1], t[2], t[3], t[4], mult)
        o = o.permute(0, 2, 1, 3).reshape(B * L, H)
        o.backward(d_o.to(dt))
        res[dt] = dict(o=o.detach(), dqkv=t[0].grad, dEw=t[1].grad, dEb=t[2].grad, dFw=t[3].grad, dFb=t[4].grad)
    # the kernel; q / k / v are column slices of one [T, 3 H] buffer, followed by poisoned memory
    f32 = dict(dtype=torch.float32, device=DEV)
    tail = 4096 if poison else 0
    buf = torch.full((B * L * 3 * H + tail,), float("nan"), **f32)
    qkv_d = buf[:B * L * 3 * H].view(B * L, 3 * H)
    qkv_d.copy_(qkv)
    dev = [x.to(DEV) for x in (keep, Ew, Eb, Fw, Fb)]
    o, lse = torch.empty(B * L, H, **f32), torch.empty(B, h, L, **f32)
    scale = math.sqrt(1.0 / d)
    ops.msa_linear_fwd(qkv_d[:, :H], qkv_d[:, H:2 * H], qkv_d[:, 2 * H:], *dev, B, L, h, d, scale, p, seed, o, lse)
    n = ops.msa_n_partial(B, h) if n_partial is None else n_partial
    part = torch.zeros(n, 2 * c * L + 2 * c, **f32)
    dqkv = torch.full((B * L, 3 * H), float("nan"), **f32)
    ops.msa_linear_bwd(qkv_d[:, :H], qkv_d[:, H:2 * H], qkv_d[:, 2 * H:], *dev, B, L, h, d, scale, p, seed, d_o.to(DEV), lse,
                       dqkv[:, :H], dqkv[:, H:2 * H], dqkv[:, 2 * H:], part)
    s = mbht.colsum(part)
    got = dict(o=o, dqkv=dqkv, dEw=s[:c * L].view(c, L), dFw=s[c * L:2 * c * L].view(c, L), dEb=s[2 * c * L:2 * c * L + c],
               dFb=s[2 * c * L + c:])
    return got, res[torch.float64], res[torch.float32], keep


def _check(tag, got, ref, ref32):
    # a tensor that is zero in exact arithmetic (the key-side gradients when c = 1: a softmax over one column) is compared on the
    # scale of the largest tensor of the case
    top = max(float(v.abs().max()) for v in ref.values())
    rel = lambda a, k: _rel(a, ref[k]) if float(ref[k].abs().max()) > 0 else float(a.detach().double().abs().max().cpu()) / top
    errs = {k: rel(got[k], k) for k in ref}
    e32 = {k: rel(ref32[k], k) for k in ref}
    print(f"{tag}: " + " ".join(f"{k} {errs[k]:.2e} (torch fp32 {e32[k]:.2e})" for k in ref))
    for k, v in errs.items():
        assert v < (2e-5 if k in ("o", "y") else 2e-4), (k, v)
        assert math.isfinite(v)


@pytest.mark.parametrize("L", [8, 16, 40, 128])
@pytest.mark.parametrize("d", [16, 32, 64])
@pytest.mark.parametrize("c", [1, 5, 16])
def test_linear_attention_against_fp64(L, d, c):
    for B in (1, 3, 37):
        got, ref, ref32, keep = _msa_case(L, d, c, B, poison=True)
        _check(f"msa L={L} d={d} c={c} B={B}", got, ref, ref32)
        # padding keys and values get exact zeros
        H = 2 * d
        pad = (keep == 0).flatten().to(DEV)
        assert float(got["dqkv"][pad][:, H:].abs().max() if bool(pad.any()) else 0.0) == 0.0


@pytest.mark.parametrize("L,d,c", [(8, 16, 1), (40, 32, 5), (128, 64, 16)])
def test_linear_attention_with_dropout_on_the_kernels_own_mask(L, d, c):
    seed = (5 << 32) | 0x1234
    got, ref, ref32, _ = _msa_case(L, d, c, 3, p=0.3, seed=seed)
    kept = float((_keep_mask(0.3, seed, 3 * 2 * L * c) != 0).double().mean())
    assert 0.6 < kept < 0.8 or L * c < 200
    _check(f"msa dropout L={L} d={d} c={c}", got, ref, ref32)


def test_linear_attention_repeats_bit_for_bit_and_rows_are_independent():
    L, d, c = 40, 32, 5
    a, _, _, _ = _msa_case(L, d, c, 37, p=0.3, seed=77)
    b, _, _, _ = _msa_case(L, d, c, 37, p=0.3, seed=77)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    few, _, _, _ = _msa_case(L, d, c, 37, p=0.3, seed=77, n_partial=3)
    for k in ("o", "dqkv"):
        assert torch.equal(a[k], few[k]), k                                       # (a row's outputs do not depend on the slab count)
    for k in ("dEw", "dFw", "dEb", "dFb"):
        assert _rel(few[k], a[k]) < 1e-5


# ---- out_fc along the sequence axis -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Lout,Lin,H", [(8, 14, 32), (40, 53, 64), (128, 147, 100), (40, 52, 256)])
def test_seq_mix_against_fp64(Lout, Lin, H):
    B = 5
    g = torch.Generator().manual_seed(Lout + Lin)
    L0 = Lout
    L1 = (Lin - L0) // 3 * 2
    L2 = Lin - L0 - L1
    xs = [torch.randn(B, n, H, generator=g) for n in (L0, L1, L2)]
    W, bias, dy = 0.3 * torch.randn(Lout, Lin, generator=g), torch.randn(Lout, generator=g), torch.randn(B, Lout, H, generator=g)
    res = {}
    for dt in (torch.float64, torch.float32):
        t = [x.to(dt).requires_grad_(True) for x in xs + [W, bias]]
        y = (torch.cat(t[:3], 1).transpose(1, 2) @ t[3].t() + t[4]).transpose(1, 2)      # out_fc as the reference applies it
        y.backward(dy.to(dt))
        res[dt] = dict(y=y.detach(), dx0=t[0].grad, dx1=t[1].grad, dx2=t[2].grad, dW=t[3].grad, db=t[4].grad)
    f32 = dict(dtype=torch.float32, device=DEV)
    xd = [x.to(DEV) for x in xs]
    y = torch.full((B, Lout, H), float("nan"), **f32)
    ops.seq_mix_fwd(xd, W.to(DEV), bias.to(DEV), y)
    outs = []
    for n in (ops.seq_mix_n_partial(B, Lout, Lin), 2):
        dxs = [torch.full_like(x, float("nan")) for x in xd]
        part = torch.zeros(n, Lout * Lin + Lout, **f32)
        ops.seq_mix_bwd(xd, W.to(DEV), dy.to(DEV), dxs, part)
        s = mbht.colsum(part)
        outs.append(dict(y=y, dx0=dxs[0], dx1=dxs[1], dx2=dxs[2], dW=s[:Lout * Lin].view(Lout, Lin), db=s[Lout * Lin:]))
    _check(f"seq_mix {Lout}x{Lin} H={H}", outs[0], res[torch.float64], res[torch.float32])
    _check(f"seq_mix {Lout}x{Lin} H={H} two slabs", outs[1], res[torch.float64], res[torch.float32])
    # one source only (no second and third pointer)
    y1 = torch.empty(B, Lout, H, **f32)
    ops.seq_mix_fwd(xd[:1], W[:, :L0].contiguous().to(DEV), bias.to(DEV), y1)
    ref1 = (xs[0].double().transpose(1, 2) @ W[:, :L0].double().t() + bias.double()).transpose(1, 2)
    assert _rel(y1, ref1) < 2e-5


# ---- the model against the fixture -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fx():
    z = np.load(FX)
    return z, json.loads(str(z["meta_json"]))


def _model(fx, prefix):
    z, meta = fx
    m = meta[prefix]
    model = mbht.MBHT(mbht.MBHTConfig(**m["config"]), m["n_items"], m["max_his_len"], m["target_behavior_id"], m["n_behaviors"])
    shapes = {k: tuple(s) for k, s in zip(m["keys"], m["shapes"])}
    assert list(model.state_dict()) == m["keys"]
    sd = mw.init_state_dict(shapes, m["weight_seed"])
    assert np.allclose(mw.checksums(sd), z[prefix + "weight_checksums"], rtol=1e-12, atol=0)
    model.load_state_dict(sd)
    if hasattr(model, "hgnn_layer"):
        model.hgnn_layer.dropout = 0.0
    return model.to(DEV).train(), z, m


def _t(z, key):
    return torch.from_numpy(z[key]).to(DEV)


@pytest.mark.parametrize("prefix", ["a/", "b/"])
def test_model_output_loss_and_gradients_match_the_reference(fx, prefix):
    model, z, m = _model(fx, prefix)
    P = prefix
    masked = tuple(_t(z, P + k) for k in ("masked", "pos_items", "masked_index", "types"))
    with torch.no_grad():
        out = model.forward(masked[0], masked[3], (masked[2], torch.count_nonzero(masked[1], dim=1)))
    e_out = _rel(out, z[P + "out"])
    inter = dict(inputs=_t(z, P + "inputs"), behaviors=_t(z, P + "behaviors"), target=_t(z, P + "target"), behavior=_t(z, P + "behavior"))
    model.zero_grad()
    loss = model.calculate_loss(inter, masked=masked)
    loss.backward()
    e_loss = abs(float(loss.detach()) - float(z[P + "loss"])) / abs(float(z[P + "loss"]))
    print(f"[{P}] out {e_out:.2e} loss {e_loss:.2e} ({model.last_masked_count} slots)")
    assert e_out < 2e-5 and e_loss < 1e-5
    named = dict(model.named_parameters())
    assert list(named) == m["parameter_names"]
    mags = [float(np.abs(z[P + "grad/" + k]).max()) for k in named if k not in m["no_grad"]]
    typical = float(np.median(mags))
    worst = {}
    for k, p in named.items():
        if k in m["no_grad"]:
            # never used: no gradient, or exact zeros
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
            continue
        ref = torch.from_numpy(z[P + "grad/" + k])
        assert p.grad is not None, k
        if float(ref.abs().max()) < 1e-6 * typical:
            # attention2's key bias shifts every score of a softmax row by the same amount: its gradient is zero in exact
            # arithmetic and the reference's value is rounding noise, so it is compared on the scale of the other gradients
            worst[k] = float((p.grad.cpu().double() - ref.double()).abs().max()) / typical
        else:
            worst[k] = _rel(p.grad, ref)
    for k, v in sorted(worst.items(), key=lambda kv: -kv[1])[:5]:
        print(f"    {v:.2e}  {k}")
    assert sorted(m["no_grad"]) == sorted(k for k in named if not model._in_graph(k))
    assert max(worst.values()) < 2e-4, max(worst.items(), key=lambda kv: kv[1])


@pytest.mark.parametrize("prefix", ["a/", "b/"])
def test_model_scores_and_top10_match_the_reference(fx, prefix):
    model, z, m = _model(fx, prefix)
    model.eval()
    inter = dict(inputs=_t(z, prefix + "eval_inputs"), behaviors=_t(z, prefix + "eval_behaviors"))
    scores = model.full_sort_predict(inter)
    assert scores.shape == (6, m["n_items"] + 1)
    e = _rel(scores, z[prefix + "scores"])
    print(f"[{prefix}] scores {e:.2e}")
    assert e < 2e-5
    idx, val = model.full_sort_topk(inter, 10)
    ref = torch.from_numpy(z[prefix + "scores"])
    top = torch.from_numpy(z[prefix + "top10"])
    # the reference's ranking, unless two of its scores are closer than the bar allows to tell apart
    gaps = (ref.gather(1, top)[:, :-1] - ref.gather(1, top)[:, 1:]).min()
    if float(gaps) > 4e-5 * float(ref.abs().max()):
        assert torch.equal(idx.cpu(), top)
    assert _rel(val, ref.gather(1, idx.cpu())) < 2e-5


# ---- the hypergraph: selection, G and its backward ---------------------------------------------------------------------------------
MASK = 61


def _graph_ref(xm, seq, sel, drop_duplicates=False):
    """G [n, n] of one row in the dtype of xm, along the selection ``sel`` [L, K]: the reference's construction restated with the
    same indexed assignments, so that autograd differentiates it the same way (every duplicate index receives the full gradient)."""
    n = int((seq != 0).sum())
    s = seq[:n]
    u = torch.nn.functional.normalize(xm, dim=0)[:n]          # F.normalize(x_m) of [B, l, H] runs along l: per hidden column
    sim = u @ u.t()
    sim = torch.where(sim < 0, torch.full_like(sim, 0.01), sim)
    uniq, counts = torch.unique(s, return_counts=True)
    multi = uniq[(counts > 1) & (uniq != MASK)]
    col = {int(t): c for c, t in enumerate(uniq)}
    Hm = torch.zeros(n, len(uniq) + len(multi), dtype=xm.dtype)
    rows, cols, pi, pj, ones = [], [], [], [], []
    for i in range(n):
        if int(s[i]) == MASK:
            continue
        seen = set()
        for j in sel[i].tolist():
            if j < 0:
                continue
            tok = int(s[j])
            if tok == MASK:
                ones.append((i, col[int(s[i])]))
                continue
            if drop_duplicates and tok in seen:
                continue
            seen.add(tok)
            rows.append(i), cols.append(col[tok]), pi.append(i), pj.append(j)
    if rows:
        Hm[rows, cols] = sim[pi, pj]
    for i, c in ones:
        Hm[i, c] = 1.0
    Hm[torch.arange(n), [col[int(t)] for t in s]] = 1.0                           # self-loops overwrite
    for m_, t in enumerate(multi):
        Hm[s == t, len(uniq) + m_] = 1.0
    return (Hm / Hm.sum(1, keepdim=True)) @ (Hm / Hm.sum(0, keepdim=True)).t(), sim


GRAPH_ROWS = {
    "n=1": [[7]],
    "n<hyper_len": [[3, MASK, 9]],
    "n=L": [list(range(1, 12)) + [MASK]],
    "all items equal": [[5] * 7],
    "repeated items": [[4, 8, 4, 15, 8, 4, 23, MASK, 30, 8]],
    "several masked": [[MASK, 2, MASK, MASK, 6, 2, 11, MASK]],
    "batch": [[7], [3, MASK, 9], list(range(1, 12)) + [MASK], [5] * 7, [4, 8, 4, 15, 8, 4, 23, MASK, 30, 8],
              [MASK, 2, MASK, MASK, 6, 2, 11, MASK], [12, 13, 14, 15, 16, 17, MASK]],
}


def _graph_case(rows, H, K, clamped=False, L=12):
    g = torch.Generator().manual_seed(len(rows) * 100 + H + K)
    table = torch.randn(MASK + 1, H, generator=g)
    if not clamped:
        table = table * 0.3 + 0.5                                                   # one orthant: no negative similarity
    items = torch.zeros(len(rows), L, dtype=torch.long)
    for b, r in enumerate(rows):
        items[b, :len(r)] = torch.tensor(r)
    xm = table[items]                                                               # a function of the item alone, as in the model
    B = len(rows)
    f32 = dict(dtype=torch.float32, device=DEV)
    G = torch.full((B, L, L), float("nan"), **f32)
    sel = torch.full((B, L, K), -7, dtype=torch.int32, device=DEV)
    xd, idd = xm.to(DEV).contiguous(), items.to(torch.int32).to(DEV)
    ops.hg_build_fwd(xd, idd, MASK, K, G, sel)
    return items, xm, xd, idd, G, sel


@pytest.mark.parametrize("name", list(GRAPH_ROWS) + ["clamped"])
@pytest.mark.parametrize("H,K", [(32, 4), (100, 8)])
def test_graph_selection_G_and_gradient(name, H, K):
    clamped = name == "clamped"
    items, xm, xd, idd, G, sel = _graph_case(GRAPH_ROWS["batch" if clamped else name], H, K, clamped)
    B, L = items.shape
    selc, Gc = sel.cpu().long(), G.cpu()
    g = torch.Generator().manual_seed(3)
    dG = torch.randn(B, L, L, generator=g)
    dxm = torch.full((B, L, H), float("nan"), dtype=torch.float32, device=DEV)
    ops.hg_build_bwd(xd, idd, sel, G, dG.to(DEV), MASK, dxm)
    again = torch.empty_like(dxm)
    ops.hg_build_bwd(xd, idd, sel, G, dG.to(DEV), MASK, again)
    assert torch.equal(dxm, again)
    worst = dict(G=0.0, dxm=0.0, G32=0.0, dxm32=0.0)
    n_ties = 0
    for b in range(B):
        seq = items[b]
        n = int((seq != 0).sum())
        k = min(K, n)
        # -- the selection is valid
        x64 = xm[b].double().requires_grad_(True)
        Gref, sim = _graph_ref(x64, seq, selc[b])
        u = torch.nn.functional.normalize(xm[b].double(), dim=0)[:n]
        raw = u @ u.t()
        for i in range(L):
            row = selc[b, i].tolist()
            if i >= n or int(seq[i]) == MASK:
                assert row == [-1] * K, (b, i, row)
                continue
            chosen = row[:k]
            assert row[k:] == [-1] * (K - k) and len(set(chosen)) == k and all(0 <= j < n for j in chosen), (b, i, row)
            rest = [j for j in range(n) if j not in chosen]
            if rest:
                assert float(sim[i, chosen].min()) >= float(sim[i, rest].max()) - 1e-6, (b, i, row)
            for j in chosen:
                for j2 in rest:
                    if j2 < j:
                        tie = int(seq[j]) == int(seq[j2]) or (float(raw[i, j]) < -1e-6 and float(raw[i, j2]) < -1e-6)
                        assert not tie, (b, i, j, j2)                               # the lower position wins an exact tie
            n_ties += sum(1 for j in chosen if float(raw[i, j]) < -1e-6)
        # -- G along that selection
        worst["G"] = max(worst["G"], _rel(Gc[b, :n, :n], Gref))
        assert float(Gc[b, n:].abs().max() if n < L else 0.0) == 0.0 and float(Gc[b, :, n:].abs().max() if n < L else 0.0) == 0.0
        assert float((Gc[b, :n].sum(1) - 1).abs().max()) < 1e-5
        # -- dx_m against fp64 autograd
        (Gref * dG[b, :n, :n].double()).sum().backward()
        scale = float(x64.grad.abs().max())
        if scale > 0:
            worst["dxm"] = max(worst["dxm"], float((dxm[b].cpu().double() - x64.grad).abs().max()) / scale)
        else:
            assert float(dxm[b].abs().max()) == 0.0
        x32 = xm[b].clone().requires_grad_(True)
        G32, _ = _graph_ref(x32, seq, selc[b])
        (G32 * dG[b, :n, :n]).sum().backward()
        worst["G32"] = max(worst["G32"], _rel(G32, Gref))
        if scale > 0:
            worst["dxm32"] = max(worst["dxm32"], float((x32.grad.double() - x64.grad).abs().max()) / scale)
    print(f"graph {name} H={H} K={K}: G {worst['G']:.2e} (torch fp32 {worst['G32']:.2e}) dxm {worst['dxm']:.2e} "
          f"(torch fp32 {worst['dxm32']:.2e}); clamped selections {n_ties}")
    assert worst["G"] < 2e-5 and worst["dxm"] < 2e-4
    if clamped:
        assert n_ties > 0


def test_graph_gradient_doubles_for_a_repeated_item():
    rows = [[4, 8, 4, 15, 8, 4, 23, MASK, 30, 8]]
    items, xm, xd, idd, G, sel = _graph_case(rows, 32, 8, L=12)
    selc = sel.cpu().long()
    seq = items[0]
    n = 10
    # some row selects two positions of one item that is not its own
    dup = [i for i in range(n) if int(seq[i]) != MASK and
           len([j for j in selc[0, i].tolist() if j >= 0 and int(seq[j]) not in (MASK, int(seq[i]))]) >
           len({int(seq[j]) for j in selc[0, i].tolist() if j >= 0 and int(seq[j]) not in (MASK, int(seq[i]))})]
    assert dup
    dG = torch.randn(1, 12, 12, generator=torch.Generator().manual_seed(9))
    dxm = torch.empty(1, 12, 32, dtype=torch.float32, device=DEV)
    ops.hg_build_bwd(xd, idd, sel, G, dG.to(DEV), MASK, dxm)
    grads = []
    for drop in (False, True):
        x64 = xm[0].double().requires_grad_(True)
        Gref, _ = _graph_ref(x64, seq, selc[0], drop_duplicates=drop)
        (Gref * dG[0, :n, :n].double()).sum().backward()
        grads.append(x64.grad)
    scale = float(grads[0].abs().max())
    e_full = float((dxm[0].cpu().double() - grads[0]).abs().max()) / scale
    e_single = float((dxm[0].cpu().double() - grads[1]).abs().max()) / scale
    print(f"duplicate gradient: against the full assignment {e_full:.2e}, with one duplicate dropped {e_single:.2e}")
    assert e_full < 2e-4 and e_single > 1e-2


# ---- graph convolution, readout, fusion ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,L,H", [(3, 12, 32), (2, 40, 100), (2, 128, 256)])
def test_graph_convolution_against_fp64(B, L, H):
    g = torch.Generator().manual_seed(B + L)
    G, x, dy = torch.rand(B, L, L, generator=g), torch.randn(B, L, H, generator=g), torch.randn(B, L, H, generator=g)
    res = {}
    for dt in (torch.float64, torch.float32):
        Gt, xt = G.to(dt).requires_grad_(True), x.to(dt).requires_grad_(True)
        y = Gt @ xt
        y.backward(dy.to(dt))
        res[dt] = dict(y=y.detach(), dx=xt.grad, dG=Gt.grad)
    f32 = dict(dtype=torch.float32, device=DEV)
    y, dx, dG = (torch.full(s, float("nan"), **f32) for s in ((B, L, H), (B, L, H), (B, L, L)))
    ops.hg_conv_fwd(G.to(DEV), x.to(DEV), y)
    ops.hg_conv_bwd(G.to(DEV), x.to(DEV), dy.to(DEV), dx, dG)
    _check(f"hg_conv B={B} L={L} H={H}", dict(y=y, dx=dx, dG=dG), res[torch.float64], res[torch.float32])


def _readout_ref(x, pos, n, evaluation, before=10, follow=6):
    rows = list(x)
    for p in pos:
        if p >= len(rows) or (not evaluation and p <= 0):
            continue
        lo = max(p - before, 0)
        hi = p + 1 if evaluation else (p + follow if p + follow < n else n - 1)
        win = rows[lo:p] + rows[p + 1:max(hi, p + 1)]
        rows[p] = torch.stack(win).mean(0) if win else torch.full_like(rows[p], float("nan"))
    return torch.stack(rows)


def test_readout_against_fp64_training_and_evaluation_forms():
    L, H = 24, 40
    g = torch.Generator().manual_seed(4)
    # adjacent masked positions, pos = 0 (skipped), windows clipped at the start, at n - 1 and by both, a row with one item
    cases = [([0, 3, 4, 5], 12), ([0, 1, 2, 23], 24), ([0, 0, 11, 17], 18), ([0, 0, 0, 1], 2), ([0, 0, 0, 0], 1), ([13, 14, 19, 20], 21)]
    B = len(cases)
    x, dout = torch.randn(B, L, H, generator=g), torch.randn(B, L, H, generator=g)
    pos = torch.tensor([c[0] for c in cases], dtype=torch.int32)
    n = torch.tensor([c[1] for c in cases], dtype=torch.int32)
    f32 = dict(dtype=torch.float32, device=DEV)
    for evaluation, P in ((False, pos), (True, torch.tensor([[3], [10], [17], [1], [23], [12]], dtype=torch.int32))):
        res = {}
        for dt in (torch.float64, torch.float32):
            xt = x.clone().to(dt).requires_grad_(True)
            out = torch.stack([_readout_ref(xt[b], P[b].tolist(), int(n[b]), evaluation) for b in range(B)])
            out.backward(dout.to(dt))
            res[dt] = dict(y=out.detach(), dx=xt.grad)
        out, dx = torch.full((B, L, H), float("nan"), **f32), torch.full((B, L, H), float("nan"), **f32)
        ops.hg_readout_fwd(x.to(DEV), P.to(DEV), n.to(DEV), out, evaluation=evaluation)
        ops.hg_readout_bwd(dout.to(DEV), P.to(DEV), n.to(DEV), dx, evaluation=evaluation)
        _check(f"readout evaluation={evaluation}", dict(y=out, dx=dx), res[torch.float64], res[torch.float32])
    # evaluation at position 0: the mean of no rows, NaN as in the reference
    out = torch.empty(1, L, H, **f32)
    ops.hg_readout_fwd(x[:1].to(DEV), torch.zeros(1, 1, dtype=torch.int32, device=DEV), n[:1].to(DEV), out, evaluation=True)
    assert bool(torch.isnan(out[0, 0]).all()) and bool(torch.equal(out[0, 1:].cpu(), x[0, 1:]))


@pytest.mark.parametrize("T,H", [(5, 32), (1000, 100), (2000, 256)])
def test_fusion_against_fp64(T, H):
    g = torch.Generator().manual_seed(T)
    x0, x1, A, a, dout = (torch.randn(*s, generator=g) for s in ((T, H), (T, H), (H, H), (1, H), (T, H)))
    A = A * 0.2
    res = {}
    for dt in (torch.float64, torch.float32):
        t0, t1, w = x0.to(dt).requires_grad_(True), x1.to(dt).requires_grad_(True), (A.to(dt) @ a.to(dt).t()).reshape(H).requires_grad_(True)
        mixed = torch.stack((t0, t1))
        score = torch.softmax((mixed * w).sum(-1), dim=0).unsqueeze(-1)
        out = (mixed * score).sum(0)
        out.backward(dout.to(dt))
        res[dt] = dict(y=out.detach(), dx0=t0.grad, dx1=t1.grad, dw=w.grad)
    f32 = dict(dtype=torch.float32, device=DEV)
    w = (A @ a.t()).reshape(H).to(DEV)
    out, p0, dx0, dx1 = torch.empty(T, H, **f32), torch.empty(T, **f32), torch.empty(T, H, **f32), torch.empty(T, H, **f32)
    ops.hg_fuse_fwd(x0.to(DEV), x1.to(DEV), w, out, p0)
    part = torch.full((min(256, (T + 3) // 4), H), float("nan"), **f32)
    ops.hg_fuse_bwd(x0.to(DEV), x1.to(DEV), w, p0, dout.to(DEV), dx0, dx1, part)
    _check(f"fuse T={T} H={H}", dict(y=out, dx0=dx0, dx1=dx1, dw=mbht.colsum(part)), res[torch.float64], res[torch.float32])


# ---- the plain layer, the mask draw, memory, training -------------------------------------------------------------------------------
def test_enable_ms_false_is_the_plain_encoder_fed_the_same_weights():
    from gamer_amd import modules
    cfg = mbht.MBHTConfig(n_layers=2, n_heads=2, hidden_size=32, inner_size=64, dropout_prob=0.0, enable_hg=False, enable_ms=False)
    torch.manual_seed(1)
    model = mbht.MBHT(cfg, 60, 7, 3, 3).to(DEV).train()
    layer = modules.TransformerEncoderLayer(32, 2, 64, 0.0, "gelu", 1e-12)
    enc = modules.TransformerEncoder(layer, 2).to(DEV)
    enc.load_state_dict(model.trm_encoder.state_dict())
    items = torch.tensor([[5, 9, 2, 61, 0, 0, 0, 0], [1, 2, 3, 4, 5, 6, 7, 61]], device=DEV)
    types = torch.tensor([[1, 2, 3, 0, 0, 0, 0, 0], [1, 1, 2, 2, 3, 3, 1, 0]], device=DEV)
    out = model.forward(items, types)
    x = torch.nn.functional.layer_norm(model.item_embedding(items) + model.position_embedding.weight[None] + model.type_embedding(types),
                                       (32,), model.LayerNorm.weight, model.LayerNorm.bias, 1e-12)
    mask = ((items <= 0).float() * torch.finfo(torch.float32).min)[:, None, None, :]
    ref = enc(x.detach(), mask)
    assert _rel(out, ref) < 2e-5
    inter = dict(inputs=items[:, :7] * (items[:, :7] != 61), behaviors=types[:, :7], target=torch.tensor([3, 4], device=DEV),
                 behavior=torch.tensor([3, 3], device=DEV))
    loss = model.calculate_loss(inter)
    loss.backward()
    assert math.isfinite(float(loss)) and model.trm_encoder.layer[0].multi_head_attention.query.weight.grad is not None


def test_default_mask_draw():
    cfg = mbht.MBHTConfig(n_layers=1, n_heads=2, hidden_size=32, inner_size=32, scales=[5, 4, 20], enable_hg=False)
    model = mbht.MBHT(cfg, 500, 39, 1, 3).to(DEV)
    B = 4096
    g = torch.Generator().manual_seed(0)
    lens = torch.randint(1, 40, (B,), generator=g)
    items = torch.randint(1, 501, (B, 39), generator=g) * (torch.arange(39)[None] < lens[:, None])
    types = torch.randint(1, 4, (B, 39), generator=g) * (items != 0)
    target, ttype = torch.randint(1, 501, (B,), generator=g), torch.full((B,), 2)
    masked, pos_items, masked_index, mtypes = (t.cpu() for t in model.reconstruct_train_data(items.to(DEV), types.to(DEV), target.to(DEV),
                                                                                             ttype.to(DEV), seed=123))
    again = model.reconstruct_train_data(items.to(DEV), types.to(DEV), target.to(DEV), ttype.to(DEV), seed=123)
    assert torch.equal(masked, again[0].cpu()) and torch.equal(masked_index, again[2].cpu())
    ar = torch.arange(B)
    assert masked.shape == (B, 40) and pos_items.shape == (B, 7) == masked_index.shape
    assert bool((masked[ar, lens] == 501).all())                                    # the appended position is always masked
    m = masked == 501
    assert bool((mtypes[m] == 0).all()) and bool((mtypes[ar, lens] == 0).all())
    full = torch.zeros(B, 40, dtype=torch.long)
    full[:, :39] = items
    full[ar, lens] = target
    assert bool((masked[~m] == full[~m]).all()) and bool((masked[:, 1:][(full == 0)[:, 1:]] == 0).all())
    ft = torch.zeros(B, 40, dtype=torch.long)
    ft[:, :39] = types
    ft[ar, lens] = ttype
    assert bool((mtypes[~m] == ft[~m]).all())
    # left-padded with 0, the LAST 7 masked positions in ascending order, with their items
    for b in range(0, B, 97):
        where = m[b].nonzero()[:, 0].tolist()[-7:]
        assert masked_index[b].tolist() == [0] * (7 - len(where)) + where
        assert pos_items[b].tolist() == [0] * (7 - len(where)) + full[b, where].tolist()
    # the rate of the earlier positions: a binomial of sum(lens) draws at 0.2, within five standard deviations
    draws = int(lens.sum())
    hits = int(m.sum()) - B
    assert abs(hits - 0.2 * draws) < 5 * math.sqrt(draws * 0.2 * 0.8), (hits, draws)


def test_hypergraph_branch_peak_memory_stays_far_below_the_block_diagonal_matrix():
    cfg = mbht.MBHTConfig(n_layers=1, n_heads=2, hidden_size=64, inner_size=64, scales=[5, 4, 20], enable_hg=True, hyper_len=6)
    model = mbht.MBHT(cfg, 1000, 39, 1, 3).to(DEV).train()
    B, L, H = 1024, 40, 64
    g = torch.Generator().manual_seed(0)
    lens = torch.randint(20, 40, (B,), generator=g)
    items = (torch.randint(1, 1001, (B, L), generator=g) * (torch.arange(L)[None] < lens[:, None])).to(DEV)
    items[torch.arange(B), lens.to(DEV)] = 1001
    n_obj = torch.count_nonzero(items, dim=1)
    trm = torch.randn(B, L, H, device=DEV, requires_grad=True)
    e = model.item_embedding(items).detach().requires_grad_(True)
    pos = torch.zeros(B, 7, dtype=torch.int32, device=DEV)
    pos[:, -1] = lens.to(DEV)
    meta = dict(hyper_len=6, mask_token=1001, evaluation=False, dropout=0.2, training=True, before=10, follow=6)
    hc1, hc2 = model.hgnn_layer.hgc1, model.hgnn_layer.hgc2
    dout = torch.randn(B, L, H, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = mbht._HGFn.apply(trm, e, items.to(torch.int32), pos, n_obj.to(torch.int32), meta, model.gating_weight, model.gating_bias,
                           model.metric_w1, model.metric_w2, hc1.weight, hc1.bias, hc2.weight, hc2.bias, model.attn_weights, model.attn)
    out.backward(dout)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    block_diag = int(n_obj.sum()) ** 2 * 4
    print(f"hypergraph branch at {B} x {L}: peak {peak / 2**20:.1f} MiB beyond its inputs; the block-diagonal matrix alone "
          f"would be {block_diag / 2**20:.1f} MiB")
    assert peak < block_diag / 10
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(e.grad).all())


def test_dropout_training_is_finite_and_repeatable(fx):
    from gamer_amd import modules, rec_common
    model, z, m = _model(fx, "a/")
    model.dropout_prob = 0.5
    for layer in model.trm_encoder.layer:
        layer.dropout_p = 0.5
    model.hgnn_layer.dropout = 0.2
    inter = dict(inputs=_t(z, "a/inputs"), behaviors=_t(z, "a/behaviors"), target=_t(z, "a/target"), behavior=_t(z, "a/behavior"))
    res = []
    for _ in range(2):
        rec_common._Seeds.value = 77
        modules._SeedCounter.value = 99
        model.zero_grad()
        loss = model.calculate_loss(inter)
        loss.backward()
        res.append([loss.detach().clone()] + [p.grad.clone() for p in model.parameters() if p.grad is not None])
    assert torch.isfinite(res[0][0]) and model.last_masked_count > 0 and len(res[0]) > 60
    assert all(bool(torch.isfinite(t).all()) for t in res[0])
    for a, b in zip(res[0], res[1]):
        assert torch.equal(a, b)


def test_train_mbht_two_epochs_and_only_test(tmp_path):
    import subprocess
    from gamer_amd import synthetic
    synthetic.write_smb_dataset(str(tmp_path), "syn", n_users=60, n_items=40, seed=5, min_sessions=3, max_sessions=9)
    cfg = tmp_path / "cfg"
    cfg.mkdir()
    (cfg / "config.json").write_text(json.dumps(dict(hidden_size=64, inner_size=128, dropout_prob=0.1, scales=[3, 2, 4], hyper_len=4)))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    common = ["--base_model", str(cfg), "--data_path", str(tmp_path), "--dataset", "syn", "--tasks", "smb_dis_diff",
              "--test_task", "smb_dis_diff", "--max_his_len", "7", "--batch_size", "64", "--learning_rate", "3e-3",
              "--output_dir", str(tmp_path / "out"), "--result_dir", str(tmp_path / "res"), "--seed", "1"]
    run = lambda extra: subprocess.run([sys.executable, "-m", "gamer_amd.train_mbht", *common, *extra], cwd=root,
                                       capture_output=True, text=True, timeout=300)
    r = run(["--epochs", "2"])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    losses = [float(l.split(" loss ")[1].split()[0]) for l in r.stdout.splitlines() if l.startswith("[train_mbht] epoch")]
    assert len(losses) == 2 and all(math.isfinite(x) for x in losses), r.stdout
    sd = torch.load(tmp_path / "out" / "best_model.pth", map_location="cpu")
    assert sd["trm_encoder.layer.1.multi_head_attention.out_fc.weight"].shape == (8, 14)
    assert sd["hgnn_layer.hgc2.weight"].shape == (64, 64) and sd["position_embedding.weight"].shape == (8, 64)
    res = json.load(open(tmp_path / "res" / "result-smb_dis_diff.json"))
    metrics = "hit@1,hit@5,hit@10,recall@1,recall@5,recall@10,ndcg@5,ndcg@10".split(",")
    assert [e["eval_type"] for e in res] == ["Behavior buy", "Merged Behavior"]            # the target behaviour only
    assert all(all(k in e and math.isfinite(e[k]) for k in metrics) for e in res)
    assert all(res[0][k] == res[1][k] for k in metrics)
    r2 = run(["--only_test"])
    assert r2.returncode == 0, r2.stdout[-2000:] + r2.stderr[-2000:]
    assert json.load(open(tmp_path / "res" / "result-smb_dis_diff.json")) == res
