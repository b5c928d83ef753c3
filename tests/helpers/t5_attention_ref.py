"""Reference code shared by the tests of the key-streaming T5 attention (tests/test_tiger_long_gpu.py): T5Attention's formulas in
the dtype of their inputs, the host rebuild of the kernels' dropout mask, the key masks, one case of the kernel grid against the
fp64 truth and the fp32 torch restatement, and the whole model restated in fp32 torch.  The formulas are those of
tests/test_tiger_gpu.py, restated here so that that file stays as it is."""
from collections import OrderedDict

import numpy as np
import torch

import tiger_weights as tw

DEV = "cuda:0"
NB, MAXD = 32, 128
QUANTITIES = ("o", "lse", "dq", "dk", "dv", "drel", "dtable")
MASKS = ("none", "right", "left", "holes", "empty")


def rel_err(got, ref):
    """largest absolute difference over the largest reference magnitude; inf when the finite patterns differ"""
    got, ref = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(ref).detach().double().cpu()
    fin = torch.isfinite(ref)
    if not bool(torch.equal(torch.isfinite(got), fin)):
        return float("inf")
    if not bool(fin.any()):
        return 0.0
    return float((got[fin] - ref[fin]).abs().max() / ref[fin].abs().max().clamp_min(1e-30))


def attention(q, k, v, rel, keep, causal, mult):
    """q [B, h, Sq, d], k / v [B, h, Sk, d], rel [h, Sq + Sk - 1] or None, keep bool [B, Sk] or None, mult [B, h, Sq, Sk] or None
    -> (context, log-sum-exp); a row with no allowed key: zeros, -inf"""
    Sq, Sk = q.shape[2], k.shape[2]
    s = q @ k.transpose(-1, -2)
    i, j = torch.arange(Sq, device=q.device)[:, None], torch.arange(Sk, device=q.device)[None, :]
    if rel is not None:
        s = s + rel[:, j - i + Sq - 1][None]
    ok = torch.ones(q.shape[0], 1, Sq, Sk, dtype=torch.bool, device=q.device)
    if keep is not None:
        ok = ok & keep[:, None, None, :]
    if causal:
        ok = ok & (j <= i)[None, None]
    s = s.masked_fill(~ok, float("-inf"))
    mx = s.amax(-1, keepdim=True).detach()
    mx = torch.where(torch.isinf(mx), torch.zeros_like(mx), mx)
    e = torch.exp(s - mx)
    tot = e.sum(-1, keepdim=True)
    p = e / tot.clamp_min(1e-300 if q.dtype == torch.float64 else 1e-37)
    lse = (mx + torch.log(tot))[..., 0]
    if mult is not None:
        p = p * mult
    return p @ v, lse


def _mix32(x):
    x = x.astype(np.uint64) & 0xffffffff
    x ^= x >> 16
    x = (x * 0x7feb352d) & 0xffffffff
    x ^= x >> 15
    x = (x * 0x846ca68b) & 0xffffffff
    x ^= x >> 16
    return x


def keep_mask(p, seed, B, h, Sq, Sk):
    """DropoutRng::mult of csrc/common.h for element ((b h + head) Sq + i) Sk + j: 0 or 1 / (1 - p)"""
    k0 = _mix32(np.array([(seed & 0xffffffff) ^ 0x9e3779b9]))[0]
    k1 = _mix32(np.array([((seed >> 32) + 0x85ebca6b) & 0xffffffff]))[0]
    thr = np.uint64(int(np.float32(p) * np.float32(4294967296.0)))
    idx = np.arange(B * h * Sq * Sk, dtype=np.uint64)
    hsh = _mix32((idx & 0xffffffff) ^ k0)
    hsh = _mix32((hsh + (idx >> np.uint64(32)) * 0x9e3779b1 + k1) & 0xffffffff)
    scale = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
    return torch.from_numpy(np.where(hsh >= thr, scale, 0.0)).reshape(B, h, Sq, Sk)


def key_mask(kind, B, Sk, g):
    if kind == "none":
        return None
    keep = torch.ones(B, Sk, dtype=torch.bool)
    for b in range(B):
        n = int(torch.randint(1, Sk + 1, (1,), generator=g))
        if kind == "right":
            keep[b, n:] = False
        elif kind == "left":
            keep[b, :Sk - n] = False
        elif kind in ("holes", "empty"):
            keep[b] = torch.rand(Sk, generator=g) < 0.6
            keep[b, int(torch.randint(0, Sk, (1,), generator=g))] = True
    if kind == "empty":
        keep[B - 1] = False                                            # one row with no kept key
    return keep


def case(Sq, Sk, h, d, B, bias, causal, mask, p, seed=(7 << 32) | 0x51, rows=None, n_slab=None, torch32=True, truth=True):
    """runs the key-streaming kernels and the fp64 truth (and the fp32 torch restatement) for one case -> (got, ref, t32) dicts;
    every output is filled with NaN before the launch"""
    from gamer_amd import ops
    from gamer_amd.tiger import bucket_vector
    g = torch.Generator().manual_seed(100003 * Sq + 1009 * Sk + 101 * h + 7 * d + B + (3 if bias else 0) + (5 if causal else 0))
    I, R = h * d, Sq + Sk - 1
    # scores of O(10): T5 does not scale them
    q = torch.randn(B, Sq, I, generator=g) * (10.0 / d) ** 0.5
    k = torch.randn(B, Sk, I, generator=g)
    v = torch.randn(B, Sk, I, generator=g)
    d_o = torch.randn(B, Sq, I, generator=g)
    table = torch.randn(NB, h, generator=g) if bias else None
    keep = key_mask(mask, B, Sk, g)
    if rows is not None:
        sel = torch.tensor(rows)
        q, k, v, d_o, keep, B = q[sel], k[sel], v[sel], d_o[sel], (None if keep is None else keep[sel]), len(rows)
    bucket = bucket_vector(max(Sq, Sk), not causal, NB, MAXD)
    bucket = bucket[max(Sq, Sk) - Sq:max(Sq, Sk) - Sq + R].contiguous()           # offsets -(Sq - 1) .. Sk - 1
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)
    if Sq == Sk:                                                     # column blocks of one q|k|v buffer, as the model has them
        buf = torch.cat([q, k, v], 2).reshape(B * Sq, 3 * I).to(DEV)
        qd, kd, vd = buf[:, :I], buf[:, I:2 * I], buf[:, 2 * I:]
        dbuf = nan(B * Sq, 3 * I)
        dq, dk, dv = dbuf[:, :I], dbuf[:, I:2 * I], dbuf[:, 2 * I:]
    else:
        qd = q.reshape(B * Sq, I).to(DEV)
        kvb = torch.cat([k, v], 2).reshape(B * Sk, 2 * I).to(DEV)
        kd, vd = kvb[:, :I], kvb[:, I:]
        dq, dkv = nan(B * Sq, I), nan(B * Sk, 2 * I)
        dk, dv = dkv[:, :I], dkv[:, I:]
    bd = bucket.to(DEV)
    rel = None
    if bias:
        rel = nan(h, R)
        ops.t5_bias_expand(table.to(DEV), bd, rel)
    keepd = None if keep is None else keep.to(torch.uint8).to(DEV)
    o, lse = nan(B * Sq, I), nan(B, h, Sq)
    ops.t5_attn_long_fwd(qd, kd, vd, rel, keepd, B, Sq, Sk, h, d, causal, p, seed, o, lse)
    n = n_slab or ops.t5_n_slab(B, h)
    slabs = nan(1, n, h, R) if bias else None
    ops.t5_attn_long_bwd(qd, kd, vd, rel, keepd, B, Sq, Sk, h, d, causal, p, seed, d_o.reshape(B * Sq, I).to(DEV), lse, dq, dk, dv,
                         None if slabs is None else slabs[0])
    got = dict(o=o, lse=lse, dq=dq, dk=dk, dv=dv)
    if bias:
        dtable = nan(NB, h)
        ops.t5_bias_fold(slabs, bd, dtable)
        got.update(drel=slabs[0].sum(0), dtable=dtable, slabs=slabs)
    torch.cuda.synchronize()
    if not truth:
        return got, None, None
    mult = keep_mask(p, seed, B, h, Sq, Sk) if p > 0 else None

    def restate(dtype, dev):
        leaf = lambda t: None if t is None else t.to(dev).to(dtype).requires_grad_(True)
        heads = lambda x, S: x.view(B, S, h, d).permute(0, 2, 1, 3)
        ql, kl, vl, tl = leaf(q), leaf(k), leaf(v), leaf(table)
        r = None
        if bias:
            r = tl[bucket.long().to(dev)].t()
            r.retain_grad()
        ctx, l = attention(heads(ql, Sq), heads(kl, Sk), heads(vl, Sk), r, None if keep is None else keep.to(dev), causal,
                           None if mult is None else mult.to(dev).to(dtype))
        out = ctx.permute(0, 2, 1, 3).reshape(B * Sq, I)
        (out * d_o.reshape(B * Sq, I).to(dev).to(dtype)).sum().backward()
        res = dict(o=out, lse=l, dq=ql.grad.reshape(B * Sq, I), dk=kl.grad.reshape(B * Sk, I), dv=vl.grad.reshape(B * Sk, I))
        if bias:
            res.update(drel=r.grad, dtable=tl.grad)
        return {k_: t.detach() for k_, t in res.items()}
    ref = restate(torch.float64, "cpu")
    t32 = restate(torch.float32, DEV) if torch32 else None
    return got, ref, t32


def grid_errors(cases):
    """{quantity: [(case, kernel error, fp32 torch error, reference magnitude, kernel magnitude, largest input gradient)]}; asserts
    that no NaN of the pre-filled outputs survives"""
    errs = {k: [] for k in QUANTITIES}
    for c in cases:
        got, ref, t32 = case(*c)
        gmax = max(float(ref[k].abs().max()) for k in ("dq", "dk", "dv"))
        for k in ref:
            fin = torch.isfinite(ref[k])
            errs[k].append((c, rel_err(got[k], ref[k]), rel_err(t32[k], ref[k]), float(ref[k][fin].abs().max()) if bool(fin.any()) else 0.0,
                            float(got[k][torch.isfinite(got[k])].abs().max()) if bool(torch.isfinite(got[k]).any()) else 0.0, gmax))
        for k, t in got.items():
            assert not bool(torch.isnan(t).any()), (c, k)                  # (every output was poisoned with NaN before the launch)
    return errs


# ---- the model ------------------------------------------------------------------------------------------------------------------------
def load_model(z, meta, name, dropout=0.0):
    """gamer_amd.tiger.TIGER of the fixture's config `name` with its seeded weights, on the device -> (model, state dict)"""
    from gamer_amd.tiger import TIGER, TigerConfig
    cfg = TigerConfig(**dict(meta["configs"][name], dropout_rate=dropout))
    torch.manual_seed(0)
    m = TIGER(cfg)
    shapes = OrderedDict(zip(meta[name]["keys"], [tuple(s) for s in meta[name]["shapes"]]))
    sd = tw.init_state_dict(shapes, meta[name]["weight_seed"])
    assert np.allclose(tw.checksums(sd), z[f"{name}/weight_checksums"], rtol=1e-12, atol=1e-9)
    m.load_state_dict(sd, strict=True)
    m.set_hyper(meta["temperature"])
    return m.to(DEV), sd


def restated_model(sd, cfg, ids, am, labels, temperature):
    """T5ForConditionalGeneration's forward as plain fp32 torch ops on the GPU: (loss, logits, {name: grad})"""
    from gamer_amd.tiger import bucket_vector
    P = {k: v.to(DEV).clone().requires_grad_(True) for k, v in sd.items() if k not in tw.TIED[1:]}
    h, d, eps, D = cfg["num_heads"], cfg["d_kv"], cfg["layer_norm_epsilon"], cfg["d_model"]
    E = P["shared.weight"]
    rms = lambda x, w: w * (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps))
    heads = lambda x: x.view(x.shape[0], x.shape[1], h, d).permute(0, 2, 1, 3)

    def attn(pre, xq, xkv, rel, keep, causal):
        q, k, v = xq @ P[pre + "q.weight"].t(), xkv @ P[pre + "k.weight"].t(), xkv @ P[pre + "v.weight"].t()
        ctx, _ = attention(heads(q), heads(k), heads(v), rel, keep, causal, None)
        return ctx.permute(0, 2, 1, 3).reshape(xq.shape[0], xq.shape[1], h * d) @ P[pre + "o.weight"].t()

    def stack(name, x, n_layers, causal, keep, enc=None):
        S = x.shape[1]
        bucket = bucket_vector(S, not causal, cfg["relative_attention_num_buckets"], cfg["relative_attention_max_distance"]).long().to(DEV)
        rel = P[f"{name}.block.0.layer.0.SelfAttention.relative_attention_bias.weight"][bucket].t()
        for l in range(n_layers):
            b = f"{name}.block.{l}.layer."
            x = x + attn(b + "0.SelfAttention.", rms(x, P[b + "0.layer_norm.weight"]), rms(x, P[b + "0.layer_norm.weight"]), rel,
                         None if causal else keep, causal)
            if enc is not None:
                x = x + attn(b + "1.EncDecAttention.", rms(x, P[b + "1.layer_norm.weight"]), enc, None, keep, False)
            f = b + ("2." if enc is not None else "1.")
            x = x + torch.relu(rms(x, P[f + "layer_norm.weight"]) @ P[f + "DenseReluDense.wi.weight"].t()) @ P[f + "DenseReluDense.wo.weight"].t()
        return rms(x, P[f"{name}.final_layer_norm.weight"])
    keep = am.to(DEV) != 0
    enc = stack("encoder", E[ids.to(DEV)], cfg["num_layers"], False, keep)
    dec_in = torch.zeros_like(labels)
    dec_in[:, 1:] = labels[:, :-1]
    dec_in[dec_in == -100] = 0
    out = stack("decoder", E[dec_in.to(DEV)], cfg["num_decoder_layers"], True, keep, enc) * D ** -0.5
    logits = out @ E.t()
    loss = torch.nn.functional.cross_entropy((logits / temperature).view(-1, logits.shape[-1]), labels.to(DEV).view(-1), ignore_index=-100)
    loss.backward()
    return loss.detach(), logits.detach(), {k: v.grad for k, v in P.items()}
