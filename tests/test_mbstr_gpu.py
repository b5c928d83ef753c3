"""MBSTR's kernels and model on the GPU: the behaviour attention, the mix kernels, one encoder layer and the CGC head against fp64
torch restatements of the reference's formulas written here (the reference hard-codes .float(), so it cannot run in fp64), and
the model against the real reference class (tests/golden/mbstr_small.npz, tools/make_golden_mbstr.py).

Bars of the fp64 comparisons: the project's fp32 bars for these models (test_bert4rec_forward_loss_and_grads_match_reference),
2e-5 of the largest magnitude for outputs and 2e-4 for gradients.  Every quantity here is a chain of at most five fp32
reductions of at most d d = 4096 or B L terms; with eps = 6e-8 a reduction of n random-sign terms errs by about sqrt(n) eps =
4e-6 of its operands' product, so both bars leave a factor of a few for the cancellation between the terms."""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import mbstr_weights as mw  # noqa: E402

pytestmark = pytest.mark.gpu
FX = os.path.join(os.path.dirname(__file__), "golden", "mbstr_small.npz")
DEV = "cuda:0"
FMIN = float(torch.finfo(torch.float32).min)


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("needs the GPU")
    from gamer_amd import build
    build.build()


def _rel(got, ref):
    got, ref = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(ref).detach().double().cpu()
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


# ---- the formulas of MBSMultiHeadAttention.forward, in the dtype of their inputs ----------------------------------------------------
def _pair(types, b):
    t = types.long()
    return ((t[:, :, None] * t[:, None, :]) != 0).long() * ((t[:, :, None] - 1) * b + t[:, None, :])          # [B, L, L]


def _mix(W, alpha):
    return torch.einsum("bhmn,Cbh->Chmn", W, torch.softmax(alpha, dim=1))


def _attention(q, k, v, types, W1, alpha1, W2, alpha2, rel, bucket, keep=None):
    """q, k, v [B, h, L, d]; rel [C, nb, h] or None; bucket long [2 L - 1]; keep [B, h, L, L] dropout multipliers or None"""
    B, h, L, d = q.shape
    b = W1.shape[0]
    pair = _pair(types, b)
    W1m, W2m = _mix(W1, alpha1), _mix(W2, alpha2)
    score = torch.zeros(B, h, L, L, dtype=q.dtype)
    for c in range(b * b + 1):
        sc = torch.einsum("BhQn,BhKn->BhQK", torch.einsum("BhQm,hmn->BhQn", q, W1m[c]), k)
        score = torch.where((pair == c)[:, None], sc, score)
    score = score * math.sqrt(1.0 / d)
    if rel is not None:
        bk = bucket[torch.arange(L)[None, :] - torch.arange(L)[:, None] + L - 1]                             # [L, L]
        score = score + rel[pair, bk[None].expand(B, -1, -1)].permute(0, 3, 1, 2)
    score = score + (types == 0)[:, None, None, :].to(q.dtype) * FMIN
    p = torch.softmax(score, dim=-1)
    if keep is not None:
        p = p * keep
    ctx = torch.zeros_like(q)
    for c in range(b * b + 1):
        u = torch.einsum("BhQK,BhKn->BhQn", p * (pair == c)[:, None].to(q.dtype), v)
        ctx = ctx + torch.einsum("BhQn,hnm->BhQm", u, W2m[c])
    return ctx


def _mix32(x):
    x = x.astype(np.uint64) & 0xffffffff
    x ^= x >> 16
    x = (x * 0x7feb352d) & 0xffffffff
    x ^= x >> 15
    x = (x * 0x846ca68b) & 0xffffffff
    x ^= x >> 16
    return x


def _keep_mask(p, seed, B, h, L):
    """DropoutRng::mult of csrc/common.h for element ((b h + head) L + q) L + k: 0 or 1 / (1 - p)"""
    k0 = _mix32(np.array([(seed & 0xffffffff) ^ 0x9e3779b9]))[0]
    k1 = _mix32(np.array([((seed >> 32) + 0x85ebca6b) & 0xffffffff]))[0]
    thr = np.uint64(int(np.float32(p) * np.float32(4294967296.0)))
    idx = np.arange(B * h * L * L, dtype=np.uint64)
    hsh = _mix32((idx & 0xffffffff) ^ k0)
    hsh = _mix32((hsh + (idx >> np.uint64(32)) * 0x9e3779b1 + k1) & 0xffffffff)
    scale = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
    return torch.from_numpy(np.where(hsh >= thr, scale, 0.0)).reshape(B, h, L, L)


def _types(B, L, b, g, absent=None):
    """row 0 full, row 1 one item, the others ragged; every type present in row 0 when it is long enough"""
    lens = [L, 1] + [int(torch.randint(1, L + 1, (1,), generator=g)) for _ in range(B - 2)]
    t = torch.zeros(B, L, dtype=torch.long)
    for r, n in enumerate(lens[:B]):
        t[r, :n] = torch.randint(1, b + 1, (n,), generator=g)
    t[0, :min(L, b)] = torch.arange(1, b + 1)[:L]
    if absent is not None:
        t[t == absent] = 1 if absent != 1 else 2
    return t


def _attn_case(L, d, b, bias, p=0.0, seed=0, B=3, h=2, rows=None, n_partial=None):
    from gamer_amd import ops
    from gamer_amd.mbstr import relative_position_buckets
    g = torch.Generator().manual_seed(1000 * L + 10 * d + b + (7 if bias else 0))
    H, C = h * d, b * b + 1
    types = _types(B, L, b, g)
    qkv = torch.randn(B * L, 3 * H, generator=g, dtype=torch.float64) * 0.5
    W1, W2 = (torch.randn(b, h, d, d, generator=g, dtype=torch.float64) * 0.7 / math.sqrt(d) for _ in range(2))
    a1, a2 = (torch.randn(C, b, h, generator=g, dtype=torch.float64) for _ in range(2))
    nb = 32
    rel = torch.randn(C, nb, h, generator=g, dtype=torch.float64) * 0.5 if bias else None
    bucket = relative_position_buckets(L, nb, 40)
    d_o = torch.randn(B * L, H, generator=g, dtype=torch.float64)
    if rows is not None:                                       # a sub-batch of the same rows: row independence
        sel = torch.tensor(rows)
        types = types[sel]
        qkv = qkv.view(B, L, -1)[sel].reshape(-1, 3 * H)
        d_o = d_o.view(B, L, -1)[sel].reshape(-1, H)
        B = len(rows)
    f = lambda t: None if t is None else t.float().to(DEV).contiguous()
    qd, t32 = f(qkv), types.to(torch.int32).to(DEV)
    W1d, W2d, a1d, a2d, reld, bd = f(W1), f(W2), f(a1), f(a2), f(rel), bucket.to(DEV)
    w1m, w2m = torch.empty(C, h, d, d, device=DEV), torch.empty(C, h, d, d, device=DEV)
    ops.mbs_mix_fwd(W1d, a1d, w1m)
    ops.mbs_mix_fwd(W2d, a2d, w2m)
    o, lse = torch.full((B * L, H), 7.0, device=DEV), torch.empty(B, h, L, device=DEV)
    scale = math.sqrt(1.0 / d)
    q_, k_, v_ = qd[:, :H], qd[:, H:2 * H], qd[:, 2 * H:]
    ops.mbs_attn_fwd(q_, k_, v_, t32, w1m, w2m, reld, bd, B, L, h, d, b, scale, p, seed, o, lse)
    n = n_partial or ops.mbs_n_partial(B, h, d, b)            # (slabs: workgroup s walks the rows s, s + n, ...)
    dqkv = torch.zeros(B * L, 3 * H, device=DEV)
    p1, p2 = torch.zeros(n, C, h, d, d, device=DEV), torch.zeros(n, C, h, d, d, device=DEV)
    pr = torch.zeros(n, C, 2 * L - 1, h, device=DEV) if bias else None
    ops.mbs_attn_bwd(q_, k_, v_, t32, w1m, w2m, reld, bd, B, L, h, d, b, scale, p, seed, o, f(d_o), lse, dqkv[:, :H],
                     dqkv[:, H:2 * H], dqkv[:, 2 * H:], p1, p2, pr)
    col = lambda part: (lambda out: (ops.colsum_reduce(part.view(n, -1), out), out)[1])(torch.empty(part[0].numel(), device=DEV))
    dw1m, dw2m = col(p1).view(C, h, d, d), col(p2).view(C, h, d, d)
    dW1, dW2, da1, da2 = torch.empty_like(W1d), torch.empty_like(W2d), torch.empty_like(a1d), torch.empty_like(a2d)
    ops.mbs_mix_bwd(W1d, a1d, dw1m, dW1, da1)
    ops.mbs_mix_bwd(W2d, a2d, dw2m, dW2, da2)
    drel = None
    if bias:
        drel = torch.empty_like(reld)
        ops.mbs_bias_fold(col(pr).view(C, 2 * L - 1, h), bd, drel)
    torch.cuda.synchronize()
    got = dict(o=o, dqkv=dqkv, dW1=dW1, dW2=dW2, da1=da1, da2=da2, drel=drel, lse=lse, w1m=w1m)
    # fp64 truth from the fp32 inputs
    leaf = lambda t: None if t is None else t.double().cpu().requires_grad_(True)
    q64, W1r, W2r, a1r, a2r, relr = leaf(qd), leaf(W1d), leaf(W2d), leaf(a1d), leaf(a2d), leaf(reld)
    heads = lambda x: x.view(B, L, h, d).permute(0, 2, 1, 3)
    keep = _keep_mask(p, seed, B, h, L) if p > 0 else None
    ctx = _attention(heads(q64[:, :H]), heads(q64[:, H:2 * H]), heads(q64[:, 2 * H:]), types, W1r, a1r, W2r, a2r, relr,
                     bucket.long(), keep)
    ref_o = ctx.permute(0, 2, 1, 3).reshape(B * L, H)
    (ref_o * d_o.view(B * L, H)).sum().backward()
    ref = dict(o=ref_o, dqkv=q64.grad, dW1=W1r.grad, dW2=W2r.grad, da1=a1r.grad, da2=a2r.grad,
               drel=None if relr is None else relr.grad, w1m=_mix(W1r, a1r))
    return got, ref


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("b", [2, 4, 5])
@pytest.mark.parametrize("d", [16, 32, 64])
@pytest.mark.parametrize("L", [1, 7, 50, 128])
def test_attention_against_fp64(L, d, b, bias):
    got, ref = _attn_case(L, d, b, bias)
    errs = {k: _rel(got[k], ref[k]) for k in ref if ref[k] is not None}
    print(f"L={L} d={d} b={b} bias={bias}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert bool(torch.isfinite(got["lse"]).all())
    assert errs["o"] < 2e-5 and errs["w1m"] < 2e-5
    keys = ("dqkv", "dW1", "dW2", "da1", "da2") + (("drel",) if bias else ())
    gmax = max(float(ref[k].abs().max()) for k in keys)
    for k in keys:
        if float(ref[k].abs().max()) < 1e-12 * gmax:
            # L = 1: a softmax over one key, so the scores do not reach the output and dW1, dalpha1 and the bias table's gradient
            # are zero in exact arithmetic.  The kernel's dS = p (dp - delta) is then the difference of two fp32 evaluations of
            # the same number, dO . ctx: rounding residue, held to the gradient bar against the case's largest gradient (all
            # operands are of order 1)
            assert L == 1 and float(got[k].abs().max()) < 2e-4 * gmax, (k, float(got[k].abs().max()), gmax)
        else:
            assert errs[k] < 2e-4, (k, errs[k])


@pytest.mark.parametrize("L,d,b", [(7, 16, 2), (50, 32, 4), (128, 64, 5)])
def test_attention_with_dropout_against_fp64_with_the_kernels_own_mask(L, d, b):
    got, ref = _attn_case(L, d, b, True, p=0.3, seed=(5 << 32) | 0x1234)
    keep = _keep_mask(0.3, (5 << 32) | 0x1234, 3, 2, L)
    assert 0.6 < float((keep != 0).double().mean()) < 0.8 or L < 50
    errs = {k: _rel(got[k], ref[k]) for k in ref if ref[k] is not None}
    print(f"dropout L={L} d={d} b={b}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert errs["o"] < 2e-5
    for k in ("dqkv", "dW1", "dW2", "da1", "da2", "drel"):
        assert errs[k] < 2e-4, (k, errs[k])


@pytest.mark.parametrize("B,n_partial", [(3, 1), (3, 2), (7, 3), (300, None)])
@pytest.mark.parametrize("L,d,b,p", [(7, 16, 2, 0.0), (50, 32, 4, 0.3), (128, 64, 5, 0.0)])
def test_attention_backward_walks_several_rows_per_workgroup(L, d, b, p, B, n_partial):
    """fewer slabs than rows (every real batch: n <= 256 / h): a workgroup re-stages its tiles and type lists for each of its rows
    and adds to its slab across them; at B = 300 the default n = 128 gives two or three rows per workgroup.  Same bars."""
    if B == 300 and L == 128:
        B = 130                                                 # (keeps the fp64 truth on the host short)
    from gamer_amd import ops
    assert (n_partial or ops.mbs_n_partial(B, 2, d, b)) < B
    got, ref = _attn_case(L, d, b, True, p=p, seed=(3 << 32) | 77, B=B, n_partial=n_partial)
    errs = {k: _rel(got[k], ref[k]) for k in ref if ref[k] is not None}
    print(f"multi-row L={L} d={d} b={b} p={p} B={B} n={n_partial}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert errs["o"] < 2e-5
    for k in ("dqkv", "dW1", "dW2", "da1", "da2", "drel"):
        assert errs[k] < 2e-4, (k, errs[k])
    again, _ = _attn_case(L, d, b, True, p=p, seed=(3 << 32) | 77, B=B, n_partial=n_partial)
    for k in got:
        assert torch.equal(got[k], again[k]), k


@pytest.mark.parametrize("b,h,d", [(2, 1, 16), (4, 2, 32), (5, 3, 64), (8, 2, 8)])
def test_mix_kernels_and_their_backward_against_fp64(b, h, d):
    from gamer_amd import ops
    g = torch.Generator().manual_seed(100 * b + d)
    C = b * b + 1
    W, alpha = torch.randn(b, h, d, d, generator=g), torch.randn(C, b, h, generator=g) * 2.0
    dWm = torch.randn(C, h, d, d, generator=g)
    Wd, ad, gd = W.to(DEV), alpha.to(DEV), dWm.to(DEV)
    Wm, dW, da = torch.empty(C, h, d, d, device=DEV), torch.full_like(Wd, 7.0), torch.full_like(ad, 7.0)
    ops.mbs_mix_fwd(Wd, ad, Wm)
    ops.mbs_mix_bwd(Wd, ad, gd, dW, da)
    W64, a64 = W.double().requires_grad_(True), alpha.double().requires_grad_(True)
    ref = _mix(W64, a64)
    (ref * dWm.double()).sum().backward()
    errs = (_rel(Wm, ref), _rel(dW, W64.grad), _rel(da, a64.grad))
    print(f"mix b={b} h={h} d={d}: Wm {errs[0]:.2e} dW {errs[1]:.2e} dalpha {errs[2]:.2e}")
    assert errs[0] < 2e-5 and errs[1] < 2e-4 and errs[2] < 2e-4
    dW2, da2 = torch.empty_like(Wd), torch.empty_like(ad)
    ops.mbs_mix_bwd(Wd, ad, gd, dW2, da2)
    assert torch.equal(dW, dW2) and torch.equal(da, da2)


def test_attention_two_calls_bit_identical_and_rows_independent():
    a, _ = _attn_case(50, 32, 4, True, p=0.0)
    b, _ = _attn_case(50, 32, 4, True, p=0.0)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    # a row's result does not depend on the other rows of the batch
    one, _ = _attn_case(50, 32, 4, True, rows=[2])
    L = 50
    assert torch.equal(one["o"], a["o"][2 * L:3 * L]) and torch.equal(one["dqkv"], a["dqkv"][2 * L:3 * L])
    assert torch.equal(one["lse"][0], a["lse"][2])


def test_attention_wrapper_limits():
    from gamer_amd import ops
    for L, H, d, b in ((129, 64, 32, 4), (50, 130, 65, 4), (50, 512, 64, 4), (50, 64, 32, 9)):
        with pytest.raises(NotImplementedError, match="MBSTR on the HIP path"):
            ops.mbs_check_limits(L, H, d, b)
    ops.mbs_check_limits(128, 256, 64, 8)


# ---- one encoder layer: grouped projections, attention, grouped FFN --------------------------------------------------------------
def _layer_ref(x, types, sd, b, h, act, eps, bucket):
    """MBSTransformerEncoderLayer.forward in x's dtype: per-type loops for the projections and the experts"""
    B, L, H = x.shape
    d = H // h
    A = "multi_head_attention."
    t = types
    proj = {}
    for name in ("query", "key", "value"):
        W = sd[A + name]
        out = torch.zeros(B, L, h, d, dtype=x.dtype)
        for ty in range(b + 1):
            out = out + (t == ty)[:, :, None, None].to(x.dtype) * torch.einsum("BLH,Hhd->BLhd", x, W[ty])
        proj[name] = out.permute(0, 2, 1, 3)
    rel = None
    if A + "relative_position_bias.0.relative_attention_bias.weight" in sd:
        rel = torch.stack([sd[A + f"relative_position_bias.{c}.relative_attention_bias.weight"] for c in range(b * b + 1)])
    ctx = _attention(proj["query"], proj["key"], proj["value"], t, sd[A + "W1"], sd[A + "alpha1"], sd[A + "W2"], sd[A + "alpha2"],
                     rel, bucket)
    ctx = ctx.permute(0, 2, 1, 3).reshape(B, L, H)
    y1 = torch.nn.functional.layer_norm(ctx + x, (H,), sd[A + "LayerNorm.weight"], sd[A + "LayerNorm.bias"], eps)
    F_ = "feed_forward."
    f = torch.zeros_like(y1)
    for i in range(b):
        e = torch.nn.functional.linear(act(torch.nn.functional.linear(y1, sd[F_ + f"FFN.{i}.dense_1.weight"],
                                                                       sd[F_ + f"FFN.{i}.dense_1.bias"])),
                                       sd[F_ + f"FFN.{i}.dense_2.weight"], sd[F_ + f"FFN.{i}.dense_2.bias"])
        f = f + (t == i + 1)[:, :, None].to(x.dtype) * e
    return torch.nn.functional.layer_norm(f + y1, (H,), sd[F_ + "LayerNorm.weight"], sd[F_ + "LayerNorm.bias"], eps)


@pytest.mark.parametrize("bias,act", [(True, "relu"), (False, "gelu")])
def test_layer_against_per_type_loops_with_an_absent_type(bias, act):
    from gamer_amd.mbstr import MBSTransformerEncoderLayer, _TypeLists, relative_position_buckets
    B, L, H, h, b, dff = 5, 12, 64, 2, 4, 96
    g = torch.Generator().manual_seed(3)
    torch.manual_seed(0)
    layer = MBSTransformerEncoderLayer(H, h, b, dff, 0.0, act, 1e-12, 32, 40, bias)
    with torch.no_grad():
        for n, p in layer.named_parameters():
            p.copy_(torch.randn(p.shape, generator=g) * (0.15 if p.dim() > 1 else 0.05) + (1.0 if n.endswith("LayerNorm.weight") else 0.0))
    layer = layer.to(DEV).train()
    types = _types(B, L, b, g, absent=3)                       # no row of type 3: an empty group in every grouped GEMM
    assert not bool((types == 3).any()) and bool((types == 0).any())
    x = (torch.randn(B, L, H, generator=g) * 0.5)
    dy = torch.randn(B, L, H, generator=g)
    bucket = relative_position_buckets(L, 32, 40)
    xd = x.to(DEV).requires_grad_(True)
    out = layer(xd, None, type_seq=_TypeLists(types.to(torch.int32).to(DEV), b), bucket=bucket.to(DEV) if bias else None)
    out.backward(dy.to(DEV))
    torch.cuda.synchronize()
    sd = {k: v.detach().double().cpu().requires_grad_(True) for k, v in layer.named_parameters()}
    x64 = x.double().requires_grad_(True)
    fn = dict(relu=torch.relu, gelu=torch.nn.functional.gelu)[act]
    ref = _layer_ref(x64, types, sd, b, h, fn, 1e-12, bucket.long())
    (ref * dy.double()).sum().backward()
    live = (types != 0)[:, :, None]
    assert _rel(out.detach().cpu() * live, ref.detach() * live) < 2e-5
    assert _rel(xd.grad, x64.grad) < 2e-4
    for k, p in layer.named_parameters():
        if ".FFN." in k and ".LayerNorm." in k:
            assert p.grad is None and sd[k].grad is None, k
            continue
        r = sd[k].grad
        if float(r.abs().max()) == 0:
            assert float(p.grad.abs().max()) == 0, k            # the absent type's expert, pair index 0's table
        else:
            assert _rel(p.grad, r) < 2e-4, (k, _rel(p.grad, r))
    assert float(layer.feed_forward.FFN[2].dense_1.weight.grad.abs().max()) == 0
    assert float(layer.multi_head_attention.query.grad[3].abs().max()) == 0


# ---- the CGC head -------------------------------------------------------------------------------------------------------------------
def test_cgc_head_against_the_formulas_with_a_padding_row():
    from gamer_amd.mbstr import CGCDotProductPredictionHead, _CGCHeadFn
    H, b, ns, nsp, T = 64, 4, 3, 2, 40
    g = torch.Generator().manual_seed(9)
    head = CGCDotProductPredictionHead(H, 10, torch.nn.Embedding(12, H), 1e-12, b, ns, nsp)
    with torch.no_grad():
        for n, p in head.named_parameters():
            p.copy_(torch.randn(p.shape, generator=g) * (0.2 if p.dim() > 1 else 0.05) + (1.0 if n == "ln.weight" else 0.0))
    head = head.to(DEV)
    x = torch.randn(T, H, generator=g)
    rows = torch.randperm(T, generator=g)[:17].sort().values
    types = torch.randint(1, b + 1, (17,), generator=g)
    types[4] = 0                                               # y = x + ln.bias there
    types[types == 2] = 1                                      # and a type with no row
    dy = torch.randn(17, H, generator=g)
    experts = []
    for e in list(head.shared_experts) + list(head.specific_experts):
        experts += [e[0].weight, e[0].bias]
    xd = x.to(DEV).requires_grad_(True)
    meta = dict(b=b, ns=ns, nsp=nsp, eps=1e-12)
    y = _CGCHeadFn.apply(xd, rows.to(DEV), types.to(torch.int32).to(DEV), meta, head.w_gates, head.ln.weight, head.ln.bias, *experts)
    y.backward(dy.to(DEV))
    torch.cuda.synchronize()
    # CGCDotProductPredictionHead.mmoe_process in fp64
    sd = {k: v.detach().double().cpu().requires_grad_(True) for k, v in head.named_parameters()}
    x64 = x.double().requires_grad_(True)
    hs = x64[rows]
    lin = lambda k: torch.nn.functional.linear(hs, sd[k + ".0.weight"], sd[k + ".0.bias"])
    shared = [lin(f"shared_experts.{i}") for i in range(ns)]
    spec = [lin(f"specific_experts.{i}") for i in range(b * nsp)]
    gates = torch.softmax(torch.einsum("BH,bHE->bBE", hs, sd["w_gates"]), -1)
    outs = torch.stack([torch.stack(shared + spec[i * nsp:(i + 1) * nsp]) for i in range(b)])
    output = torch.einsum("bEBH,bBE->bBH", outs, gates)
    outputs = torch.cat([torch.zeros_like(hs)[None], output])
    mix = torch.einsum("bBH,Bb->BH", outputs, torch.nn.functional.one_hot(types, b + 1).double())
    ref = hs + torch.nn.functional.layer_norm(mix, (H,), sd["ln.weight"], sd["ln.bias"], 1e-12)
    (ref * dy.double()).sum().backward()
    assert _rel(y, ref) < 2e-5
    assert torch.allclose(y[4].detach().cpu(), (x[rows[4]] + head.ln.bias.detach().cpu()), atol=1e-6)
    assert _rel(xd.grad, x64.grad) < 2e-4
    for k, p in head.named_parameters():
        if k.startswith("token_embeddings"):
            continue
        r = sd[k].grad
        if float(r.abs().max()) == 0:
            assert float(p.grad.abs().max()) == 0, k
        else:
            assert _rel(p.grad, r) < 2e-4, (k, _rel(p.grad, r))
    assert float(head.specific_experts[nsp].__getitem__(0).weight.grad.abs().max()) == 0       # type 2 has no row


# ---- the model against the real reference class ------------------------------------------------------------------------------------
def _model(second=False):
    from gamer_amd.mbstr import MBSTR, MBSTRConfig
    z = np.load(FX)
    m = json.loads(str(z["meta_json"]))
    m = m["second"] if second else m
    model = MBSTR(MBSTRConfig(**m["config"]), m["n_items"], m["max_his_len"], m["n_behaviors"])
    sd = mw.init_state_dict({k: tuple(s) for k, s in zip(m["keys"], m["shapes"])}, m["weight_seed"])
    model.load_state_dict(sd, strict=True)
    P = "b/" if second else ""
    return model.to(DEV), (lambda k: z[P + k]), m, [f[len(P):] for f in z.files if f.startswith(P + "grad/")]


@pytest.mark.parametrize("second", [False, True])
def test_mbstr_forward_loss_and_grads_match_reference(second):
    """the bars of test_bert4rec_forward_loss_and_grads_match_reference: 2e-5 outputs, 1e-5 loss, 2e-4 gradients"""
    model, z, m, grad_keys = _model(second)
    masked, labels = torch.from_numpy(z("masked")).to(DEV), torch.from_numpy(z("labels")).to(DEV)
    beh = torch.from_numpy(z("behaviors")).to(DEV)
    model.train()                                          # (dropout_prob 0 in the fixture's config)
    logits, valid_labels = model(masked, beh, labels)
    assert torch.equal(valid_labels.cpu(), torch.from_numpy(z("valid_labels")))
    assert logits.shape == (valid_labels.numel(), m["n_items"] + 1)
    cols = torch.from_numpy(z("cols"))
    e_logits = _rel(logits.cpu()[:, cols], z("logits_cols"))
    model.zero_grad()
    loss = model.calculate_loss(dict(inputs=torch.from_numpy(z("inputs")).to(DEV), behaviors=beh), masked_labels=(masked, labels))
    loss.backward()
    e_loss = abs(float(loss.detach()) - float(z("loss"))) / abs(float(z("loss")))
    print(f"second={second}: logits {e_logits:.2e} loss {e_loss:.2e}")
    assert e_logits < 2e-5
    assert model.last_masked_count == valid_labels.numel() == m["M"]
    assert e_loss <= 1e-5
    seen, worst = 0, ("", 0.0)
    for k, p in model.named_parameters():
        if k in m["no_grad"]:
            assert p.grad is None, k
        elif k in m["zero_grad"]:
            assert p.grad is not None and float(p.grad.abs().max()) == 0, k
        elif "grad/" + k in grad_keys:
            e = _rel(p.grad, z("grad/" + k))
            worst = max(worst, (k, e), key=lambda t: t[1])
            assert p.grad is not None and p.grad.shape == p.shape and e < 2e-4, (k, e)
            seen += 1
            if k in m["zero_index0"]:
                assert float(p.grad[0].abs().max()) == 0, k
    print(f"second={second}: {seen} gradient tensors, worst {worst[0]} {worst[1]:.2e}")
    assert seen >= 40 and len(m["zero_index0"]) == 6 and len(m["zero_grad"]) == (0 if second else 2)
    gi = model.item_embedding.weight.grad
    rows = torch.from_numpy(z("rows"))
    assert m["n_items"] + 1 in rows.tolist() and 0 in rows.tolist()
    assert _rel(gi.cpu()[rows], z("grad_item_rows")) < 2e-4
    ck = mw.checksums({"g": gi.cpu()})[0]
    ref = z("grad_item_checksum")
    assert abs(ck[0] - ref[0]) < 2e-4 * np.sqrt(ref[1]) * 10 and abs(ck[1] - ref[1]) < 1e-3 * ref[1]


@pytest.mark.parametrize("second", [False, True])
def test_mbstr_full_sort_matches_reference(second):
    model, z, m, _ = _model(second)
    model.eval()
    inter = dict(inputs=torch.from_numpy(z("eval_inputs")).to(DEV), behaviors=torch.from_numpy(z("eval_behaviors")).to(DEV),
                 seq_len=torch.from_numpy(z("eval_seq_len")).to(DEV))
    scores = model.full_sort_predict(dict(inter))
    assert scores.shape == (inter["inputs"].shape[0], m["n_items"] + 1)
    cols = torch.from_numpy(z("cols"))
    assert _rel(scores.cpu()[:, cols], z("scores_cols")) < 2e-5
    idx, sc = model.full_sort_topk(dict(inter), 10)
    assert int(idx.max()) <= m["n_items"] and int(idx.min()) >= 0               # <MASK> is never returned
    ref_top = torch.from_numpy(z("top10"))
    full = scores.cpu()
    for b in range(idx.shape[0]):
        for q in range(10):
            a, r = int(idx[b, q]), int(ref_top[b, q])
            # identical ranks unless two neighbours' scores lie within fp32 noise of each other
            assert a == r or abs(float(full[b, a]) - float(full[b, r])) < 1e-5, (b, q, a, r)
    assert _rel(sc, torch.gather(full, 1, idx.cpu())) < 1e-5


def test_mbstr_reference_behaviours():
    model, z, m, _ = _model()
    model.train()
    inputs, beh = torch.from_numpy(z("inputs")).to(DEV), torch.from_numpy(z("behaviors")).to(DEV)
    masked, labels = model.reconstruct_train_data(inputs, seed=3)
    again = model.reconstruct_train_data(inputs, seed=3)
    assert torch.equal(masked, again[0]) and torch.equal(labels, again[1])
    assert bool(((masked == inputs) | (masked == m["n_items"] + 1)).all()) and torch.equal(labels, inputs * (masked != inputs))
    assert bool((labels[inputs == 0] == 0).all())
    # a type outside [0, b]: the reference raises RuntimeError (recorded), and so does this, on the host
    assert m["type_error"].startswith("RuntimeError")
    bad = beh.clone()
    bad[0, 0] = m["n_behaviors"] + 1
    with pytest.raises(RuntimeError, match="behaviors outside"):
        model.calculate_loss(dict(inputs=inputs, behaviors=bad))
    with pytest.raises(RuntimeError, match="behaviors outside"):
        model.full_sort_topk(dict(inputs=inputs, behaviors=-beh, seq_len=(inputs != 0).sum(1)), 5)
    # over-limit shapes
    with pytest.raises(ValueError, match="max_his_len"):
        model.calculate_loss(dict(inputs=torch.ones(2, 9, dtype=torch.long, device=DEV), behaviors=torch.ones(2, 9, dtype=torch.long, device=DEV)))
    model.max_seq_length = 200
    with pytest.raises(NotImplementedError, match="L <= 128"):
        model.calculate_loss(dict(inputs=torch.ones(2, 129, dtype=torch.long, device=DEV), behaviors=torch.ones(2, 129, dtype=torch.long, device=DEV)))
    model.max_seq_length = m["max_his_len"]
    # M = 0, as recorded from the reference: NaN loss, backward() works, every gradient exactly zero, none NaN
    assert m["m0_loss_is_nan"] and m["m0_grads_all_zero"]
    model.mask_ratio = 0.0
    model.zero_grad()
    loss = model.calculate_loss(dict(inputs=inputs, behaviors=beh))
    assert model.last_masked_count == 0 and bool(torch.isnan(loss))
    loss.backward()
    assert [k for k, p in model.named_parameters() if p.grad is None] == m["m0_no_grad"]
    assert all(bool((p.grad == 0).all()) for p in model.parameters() if p.grad is not None)


def test_state_dict_round_trip_with_the_fixture_keys():
    model, z, m, _ = _model()
    sd = model.state_dict()
    assert list(sd) == m["keys"]
    from gamer_amd.mbstr import MBSTR, MBSTRConfig
    other = MBSTR(MBSTRConfig(**m["config"]), m["n_items"], m["max_his_len"], m["n_behaviors"])
    other.load_state_dict({k: v.cpu() for k, v in sd.items()}, strict=True)


# ---- memory ----------------------------------------------------------------------------------------------------------------------
def test_attention_op_keeps_nothing_quadratic_in_memory():
    """B 4096, L 50, h 2, b 4 (d 32): the peak beyond the op's inputs, outputs and gradients stays below ONE fp32 [B, h, L, L]
    tensor (82 MB); the reference holds two [B, h, L, L, 17] tensors of 1.4 GB each."""
    from gamer_amd import ops
    from gamer_amd.mbstr import relative_position_buckets
    B, L, h, d, b = 4096, 50, 2, 32, 4
    H, C = h * d, b * b + 1
    g = torch.Generator().manual_seed(2)
    qkv = (torch.randn(B * L, 3 * H, generator=g) * 0.5).to(DEV)
    types = torch.randint(0, b + 1, (B, L), generator=g).to(torch.int32).to(DEV)
    w1m, w2m = (torch.randn(C, h, d, d, generator=g) * 0.1).to(DEV), (torch.randn(C, h, d, d, generator=g) * 0.1).to(DEV)
    rel, bucket = torch.randn(C, 32, h, generator=g).to(DEV), relative_position_buckets(L, 32, 40).to(DEV)
    d_o = torch.randn(B * L, H, generator=g).to(DEV)
    o, lse, dqkv = torch.empty(B * L, H, device=DEV), torch.empty(B, h, L, device=DEV), torch.zeros(B * L, 3 * H, device=DEV)
    dw1m, dw2m, drel = torch.empty(C * h * d * d, device=DEV), torch.empty(C * h * d * d, device=DEV), torch.empty(C, 32, h, device=DEV)
    q_, k_, v_ = qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:]
    scale = math.sqrt(1.0 / d)

    def run():
        ops.mbs_attn_fwd(q_, k_, v_, types, w1m, w2m, rel, bucket, B, L, h, d, b, scale, 0.2, 11, o, lse)
        n = ops.mbs_n_partial(B, h, d, b)
        p1, p2 = torch.zeros(n, C, h, d, d, device=DEV), torch.zeros(n, C, h, d, d, device=DEV)
        pr = torch.zeros(n, C, 2 * L - 1, h, device=DEV)
        ops.mbs_attn_bwd(q_, k_, v_, types, w1m, w2m, rel, bucket, B, L, h, d, b, scale, 0.2, 11, o, d_o, lse, dqkv[:, :H],
                         dqkv[:, H:2 * H], dqkv[:, 2 * H:], p1, p2, pr)
        ops.colsum_reduce(p1.view(n, -1), dw1m)
        ops.colsum_reduce(p2.view(n, -1), dw2m)
        tmp = torch.empty(C * (2 * L - 1) * h, device=DEV)
        ops.colsum_reduce(pr.view(n, -1), tmp)
        ops.mbs_bias_fold(tmp.view(C, 2 * L - 1, h), bucket, drel)
    run()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    dqkv.zero_()
    run()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    limit = B * h * L * L * 4
    print(f"attention op peak beyond its tensors {peak / 2 ** 20:.1f} MiB, one [B, h, L, L] {limit / 2 ** 20:.1f} MiB")
    assert bool(torch.isfinite(o).all()) and bool(torch.isfinite(dqkv).all()) and bool(torch.isfinite(dw1m).all())
    assert peak < limit, (peak, limit)


def test_training_step_does_not_materialise_logits():
    from gamer_amd.mbstr import MBSTR, MBSTRConfig
    B, V, S, b = 4096, 200_000, 20, 4
    torch.manual_seed(0)
    model = MBSTR(MBSTRConfig(dropout_prob=0.0, n_layers=1, hidden_size=64, inner_size=128), V - 1, S, b).to(DEV)
    g = torch.Generator().manual_seed(1)
    inter = dict(inputs=torch.randint(1, V, (B, S), generator=g).to(DEV), behaviors=torch.randint(1, b + 1, (B, S), generator=g).to(DEV))
    model.train()

    def step():
        model.zero_grad(set_to_none=True)
        loss = model.calculate_loss(inter)
        loss.backward()
        assert torch.isfinite(loss)
    step()                                                # warm the cached workspaces
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    step()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    M = model.last_masked_count
    assert M > B
    limit = M * V * 4                                     # one [M, V] fp32 logits tensor
    print(f"M {M} peak {peak / 2 ** 20:.0f} MiB, [M, V] {limit / 2 ** 20:.0f} MiB")
    assert peak < 0.3 * limit, (peak, limit)              # the whole step, encoder activations included (SASRec's assertion)


# ---- training ----------------------------------------------------------------------------------------------------------------------
def test_mbstr_dropout_training_is_finite_and_repeatable():
    from gamer_amd import modules, rec_common
    model, z, m, _ = _model()
    model.dropout_prob = 0.5
    for layer in model.trm_encoder.layer:
        layer.dropout_p = 0.5
    model.train()
    inter = dict(inputs=torch.from_numpy(z("inputs")).to(DEV), behaviors=torch.from_numpy(z("behaviors")).to(DEV))
    res = []
    for _ in range(2):
        rec_common._Seeds.value = 77                       # (the cloze masks and the input dropout draw from this counter)
        modules._SeedCounter.value = 99
        model.zero_grad()
        loss = model.calculate_loss(inter)
        loss.backward()
        res.append([loss.detach().clone()] + [p.grad.clone() for p in model.parameters() if p.grad is not None])
    assert torch.isfinite(res[0][0]) and model.last_masked_count > 0 and len(res[0]) > 60
    assert all(bool(torch.isfinite(t).all()) for t in res[0])
    for a, b in zip(res[0], res[1]):
        assert torch.equal(a, b)


def test_train_mbstr_two_epochs_and_only_test(tmp_path):
    import subprocess
    from gamer_amd import synthetic
    synthetic.write_smb_dataset(str(tmp_path), "syn", n_users=60, n_items=40, seed=5, min_sessions=3, max_sessions=9)
    cfg = tmp_path / "cfg"
    cfg.mkdir()
    (cfg / "config.json").write_text(json.dumps(dict(hidden_size=64, inner_size=128, dropout_prob=0.1)))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    common = ["--base_model", str(cfg), "--data_path", str(tmp_path), "--dataset", "syn", "--tasks", "smb_dis_diff_decoder",
              "--test_task", "smb_dis_target_diff", "--max_his_len", "8", "--batch_size", "64", "--learning_rate", "3e-3",
              "--output_dir", str(tmp_path / "out"), "--result_dir", str(tmp_path / "res"), "--seed", "1"]
    run = lambda extra: subprocess.run([sys.executable, "-m", "gamer_amd.train_mbstr", *common, *extra], cwd=root,
                                       capture_output=True, text=True, timeout=300)
    r = run(["--epochs", "2"])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    losses = [float(l.split(" loss ")[1].split()[0]) for l in r.stdout.splitlines() if l.startswith("[train_mbstr] epoch")]
    assert len(losses) == 2 and all(math.isfinite(x) for x in losses), r.stdout
    sd = torch.load(tmp_path / "out" / "best_model.pth", map_location="cpu")
    assert "trm_encoder.layer.1.multi_head_attention.relative_position_bias.9.relative_attention_bias.weight" in sd
    assert sd["trm_encoder.layer.0.multi_head_attention.query"].shape == (4, 64, 2, 32)       # three behaviours + padding
    assert torch.equal(sd["item_embedding.weight"], sd["head.token_embeddings.weight"])
    res = json.load(open(tmp_path / "res" / "result-smb_dis_target_diff.json"))
    metrics = "hit@1,hit@5,hit@10,recall@1,recall@5,recall@10,ndcg@5,ndcg@10".split(",")
    assert [e["eval_type"] for e in res] == ["Behavior click", "Behavior cart", "Behavior buy", "Merged Behavior"]
    assert all(all(k in e and math.isfinite(e[k]) for k in metrics) for e in res)
    r2 = run(["--only_test"])
    assert r2.returncode == 0, r2.stdout[-2000:] + r2.stderr[-2000:]
    assert json.load(open(tmp_path / "res" / "result-smb_dis_target_diff.json")) == res
