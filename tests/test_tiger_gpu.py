"""TIGER on the GPU: the T5 attention kernels against an fp64 torch restatement on the fp32-rounded inputs, their invariants, the
model against the real reference class (tests/golden/tiger_small.npz, tools/make_golden_tiger.py), beam search against HF's
``generate``, memory, dropout and the train command.

Bars.  Attention: every case of the grid also runs the restatement as fp32 torch ops on the GPU; per quantity the kernel may
err by at most twice the restatement's worst relative error over the grid (only the order of the sums differs), and never by
more than 1e-4.  Model: per config, twice the worst error of an fp32 torch restatement of the whole model (run on the GPU) against
the fixture, never above 1e-3, the project's logits bar.  Relative error = largest absolute difference over the largest
reference magnitude of the tensor."""
import json
import os
import sys
from collections import OrderedDict

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import tiger_weights as tw  # noqa: E402

pytestmark = pytest.mark.gpu
FX = os.path.join(os.path.dirname(__file__), "golden", "tiger_small.npz")
DEV = "cuda:0"
NB, MAXD = 32, 128


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("needs the GPU")
    from gamer_amd import build
    build.build()


@pytest.fixture(scope="module")
def fx():
    z = np.load(FX)
    return z, json.loads(str(z["meta_json"]))


def _rel(got, ref):
    got, ref = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(ref).detach().double().cpu()
    fin = torch.isfinite(ref)
    if not bool(torch.equal(torch.isfinite(got), fin)):
        return float("inf")
    if not bool(fin.any()):
        return 0.0
    return float((got[fin] - ref[fin]).abs().max() / ref[fin].abs().max().clamp_min(1e-30))


# ---- T5Attention's formulas in the dtype of their inputs ------------------------------------------------------------------------------
def _attention(q, k, v, rel, keep, causal, mult):
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


def _keep_mask(p, seed, B, h, Sq, Sk):
    """DropoutRng::mult of csrc/common.h for element ((b h + head) Sq + i) Sk + j: 0 or 1 / (1 - p)"""
    k0 = _mix32(np.array([(seed & 0xffffffff) ^ 0x9e3779b9]))[0]
    k1 = _mix32(np.array([((seed >> 32) + 0x85ebca6b) & 0xffffffff]))[0]
    thr = np.uint64(int(np.float32(p) * np.float32(4294967296.0)))
    idx = np.arange(B * h * Sq * Sk, dtype=np.uint64)
    hsh = _mix32((idx & 0xffffffff) ^ k0)
    hsh = _mix32((hsh + (idx >> np.uint64(32)) * 0x9e3779b1 + k1) & 0xffffffff)
    scale = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
    return torch.from_numpy(np.where(hsh >= thr, scale, 0.0)).reshape(B, h, Sq, Sk)


def _key_mask(kind, B, Sk, g):
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


def _case(Sq, Sk, h, d, B, bias, causal, mask, p, seed=(7 << 32) | 0x51, rows=None, n_slab=None, torch32=True):
    """runs the kernels and the fp64 truth (and the fp32 torch restatement) for one case -> (got, ref, t32) dicts"""
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
    keep = _key_mask(mask, B, Sk, g)
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
    ops.t5_attn_fwd(qd, kd, vd, rel, keepd, B, Sq, Sk, h, d, causal, p, seed, o, lse)
    n = n_slab or ops.t5_n_slab(B, h)
    slabs = nan(1, n, h, R) if bias else None
    ops.t5_attn_bwd(qd, kd, vd, rel, keepd, B, Sq, Sk, h, d, causal, p, seed, d_o.reshape(B * Sq, I).to(DEV), lse, dq, dk, dv,
                    None if slabs is None else slabs[0])
    got = dict(o=o, lse=lse, dq=dq, dk=dk, dv=dv)
    if bias:
        dtable = nan(NB, h)
        ops.t5_bias_fold(slabs, bd, dtable)
        got.update(drel=slabs[0].sum(0), dtable=dtable, slabs=slabs)
    torch.cuda.synchronize()
    mult = _keep_mask(p, seed, B, h, Sq, Sk) if p > 0 else None

    def restate(dtype, dev):
        leaf = lambda t: None if t is None else t.to(dev).to(dtype).requires_grad_(True)
        heads = lambda x, S: x.view(B, S, h, d).permute(0, 2, 1, 3)
        ql, kl, vl, tl = leaf(q), leaf(k), leaf(v), leaf(table)
        r = None
        if bias:
            r = tl[bucket.long().to(dev)].t()
            r.retain_grad()
        ctx, l = _attention(heads(ql, Sq), heads(kl, Sk), heads(vl, Sk), r, None if keep is None else keep.to(dev), causal,
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


SHAPES = [(1, 1, False), (7, 7, False), (8, 8, True), (5, 128, False), (8, 101, False), (101, 101, False), (128, 128, False)]
QUANTITIES = ("o", "lse", "dq", "dk", "dv", "drel", "dtable")


def _grid():
    """every shape with h in {1, 6}, d in {32, 64}, B in {1, 3}; bias, causality, the key masks and dropout rotate through the
    combinations so that each value of each meets every shape (causal needs Sq == Sk; (8, 8) is always causal: the decoder)"""
    masks = ("none", "right", "left", "holes", "empty")
    cases, n = [], 0
    for Sq, Sk, always_causal in SHAPES:
        for h in (1, 6):
            for d in (32, 64):
                for B in (1, 3):
                    for bias in (True, False):
                        causal = always_causal or (Sq == Sk and n % 3 == 0)
                        mask = masks[n % 5]
                        if mask == "empty" and B == 1:
                            mask = "holes"
                        cases.append((Sq, Sk, h, d, B, bias, causal, mask, 0.1 if n % 2 else 0.0))
                        n += 1
    return cases


@pytest.fixture(scope="module")
def grid():
    """{quantity: [(case, kernel error, fp32 torch error)]} over the grid, computed once"""
    errs = {k: [] for k in QUANTITIES}
    for case in _grid():
        got, ref, t32 = _case(*case)
        gmax = max(float(ref[k].abs().max()) for k in ("dq", "dk", "dv"))
        for k in ref:
            fin = torch.isfinite(ref[k])
            errs[k].append((case, _rel(got[k], ref[k]), _rel(t32[k], ref[k]), float(ref[k][fin].abs().max()) if bool(fin.any()) else 0.0,
                            float(got[k][torch.isfinite(got[k])].abs().max()) if bool(torch.isfinite(got[k]).any()) else 0.0, gmax))
        for k, t in got.items():
            assert not bool(torch.isnan(t).any()), (case, k)               # (every output was poisoned with NaN before the launch)
    return errs


@pytest.mark.parametrize("quantity", QUANTITIES)
def test_attention_against_fp64_within_twice_the_fp32_torch_error(grid, quantity):
    rows = grid[quantity]
    assert len(rows) >= 50
    # a quantity that is zero in exact arithmetic (one allowed key in every row: the scores do not reach the output) is rounding
    # residue, the difference of two fp32 evaluations of dO . ctx: held to the 1e-4 bar against the case's largest input gradient
    # instead, as test_mbstr_gpu does
    live = [r for r in rows if r[3] > 1e-12 * max(r[5], 1e-30)]
    worst_kernel, worst_torch = max(r[1] for r in live), max(r[2] for r in live)
    print(f"{quantity}: kernel {worst_kernel:.3e}  fp32 torch {worst_torch:.3e}  ({len(live)} of {len(rows)} cases)")
    for case, ek, et, mag, gotmag, gmax in rows:
        if mag > 1e-12 * max(gmax, 1e-30):
            assert ek <= 2.0 * worst_torch and ek <= 1e-4, (quantity, case, ek, worst_torch)
        else:
            assert gotmag <= 1e-4 * gmax, (quantity, case, gotmag, gmax)


def test_masks_cover_the_grid():
    cases = _grid()
    for Sq, Sk, _ in SHAPES:
        mine = [c for c in cases if c[:2] == (Sq, Sk)]
        assert {c[2] for c in mine} == {1, 6} and {c[3] for c in mine} == {32, 64} and {c[4] for c in mine} == {1, 3}
        assert {c[5] for c in mine} == {True, False} and {c[8] for c in mine} == {0.0, 0.1}
        assert {"none", "right", "left", "holes", "empty"} <= {c[7] for c in mine}
    assert {c[6] for c in cases if c[0] == c[1] and c[0] != 8} == {True, False}


def test_a_row_with_no_kept_key_gives_zeros_and_zero_gradients():
    got, ref, _ = _case(7, 7, 2, 32, 3, True, False, "empty", 0.0, torch32=False)
    o, dq, lse = got["o"].view(3, 7, -1), got["dq"].view(3, 7, -1), got["lse"]
    assert float(o[2].abs().max()) == 0.0 and float(dq[2].abs().max()) == 0.0
    assert float(got["dk"].view(3, 7, -1)[2].abs().max()) == 0.0 and float(got["dv"].view(3, 7, -1)[2].abs().max()) == 0.0
    assert bool(torch.isinf(lse[2]).all()) and bool((lse[2] < 0).all()) and bool(torch.isfinite(lse[:2]).all())
    for k in ref:
        assert _rel(got[k], ref[k]) < 1e-4, k


@pytest.mark.parametrize("case", [(8, 8, 6, 64, 3, True, True, "none", 0.1), (101, 101, 6, 64, 3, True, False, "right", 0.1),
                                  (5, 128, 2, 32, 3, False, False, "holes", 0.0)])
def test_two_calls_bit_identical(case):
    a, _, _ = _case(*case, torch32=False)
    b, _, _ = _case(*case, torch32=False)
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("Sq,Sk,h,d,causal", [(8, 8, 6, 64, True), (101, 101, 2, 32, False), (5, 128, 6, 64, False)])
def test_rows_are_independent(Sq, Sk, h, d, causal):
    full, _, _ = _case(Sq, Sk, h, d, 3, True, causal, "right", 0.0, torch32=False)
    one, _, _ = _case(Sq, Sk, h, d, 3, True, causal, "right", 0.0, rows=[2], torch32=False)
    for k, S in (("o", Sq), ("dq", Sq), ("dk", Sk), ("dv", Sk)):
        assert torch.equal(one[k], full[k][2 * S:3 * S]), k
    assert torch.equal(one["lse"][0], full["lse"][2])


@pytest.mark.parametrize("B,n_slab", [(7, 3), (7, 1), (5, 5)])
def test_backward_walks_several_rows_per_workgroup(B, n_slab):
    """fewer slabs than rows: a workgroup re-stages its tiles for each of its rows and adds to its own slab across them"""
    got, ref, _ = _case(23, 23, 2, 64, B, True, False, "left", 0.1, n_slab=n_slab, torch32=False)
    assert got["slabs"].shape[1] == n_slab and not bool(torch.isnan(got["slabs"]).any())
    for k in ref:
        assert _rel(got[k], ref[k]) < 1e-4, (k, _rel(got[k], ref[k]))


def test_slab_count_and_limits():
    from gamer_amd import _lib, ops
    for B, h in ((1, 1), (3, 6), (256, 6), (1024, 6), (5, 16)):
        n = ops.t5_n_slab(B, h)
        assert 1 <= n <= B and n * h <= max(512, h)
    t = torch.zeros(256, 64, device=DEV)
    lse = torch.zeros(1, 1, 128, device=DEV)
    for Sq, Sk, h, d in ((129, 8, 1, 64), (8, 129, 1, 64), (8, 8, 17, 64), (8, 8, 1, 16), (8, 8, 1, 48)):
        with pytest.raises(NotImplementedError):
            ops.t5_check_limits(Sq, Sk, h, d)
        # the C entry point refuses the same shapes before any launch
        with pytest.raises(RuntimeError, match="bad shape"):
            _lib.call("gamer_t5_attn_fwd", t.data_ptr(), 64, t.data_ptr(), 64, t.data_ptr(), 64, None, None, None, 1, Sq, Sk, h, d, 0, 0.0,
                      0, t.data_ptr(), 64, lse.data_ptr(), ops.stream_ptr())
    with pytest.raises(RuntimeError, match="n_slab"):
        _lib.call("gamer_t5_attn_bwd", t.data_ptr(), 64, t.data_ptr(), 64, t.data_ptr(), 64, None, None, 2, 8, 8, 1, 64, 0, 0.0, 0,
                  t.data_ptr(), 64, lse.data_ptr(), t.data_ptr(), 64, t.data_ptr(), 64, t.data_ptr(), 64, None, 3,
                  ops.stream_ptr())
    torch.cuda.synchronize()
    assert float(t.abs().max()) == 0.0


def test_a_stacks_table_gradient_is_the_sum_of_its_layers_folds_in_layer_order():
    from gamer_amd import ops
    layers = []
    for l in range(3):
        got, _, _ = _case(23, 23, 6, 64, 3, True, False, "right", 0.0, seed=l, torch32=False)
        layers.append(got["slabs"][0] * (1.0 + l))
    slabs = torch.stack(layers).contiguous()
    from gamer_amd.tiger import bucket_vector
    bd = bucket_vector(23, True, NB, MAXD).to(DEV)
    whole = torch.empty(NB, 6, device=DEV)
    ops.t5_bias_fold(slabs, bd, whole)
    acc = None
    for l in range(3):
        one = torch.empty(NB, 6, device=DEV)
        ops.t5_bias_fold(slabs[l:l + 1].contiguous(), bd, one)
        acc = one if acc is None else acc + one
    assert torch.equal(whole, acc)


# ---- the model against the real class -------------------------------------------------------------------------------------------------
def _model(fx, name, dropout=0.0):
    from gamer_amd.tiger import TIGER, TigerConfig
    z, meta = fx
    cfg = TigerConfig(**dict(meta["configs"][name], dropout_rate=dropout))
    torch.manual_seed(0)
    m = TIGER(cfg)
    shapes = OrderedDict(zip(meta[name]["keys"], [tuple(s) for s in meta[name]["shapes"]]))
    sd = tw.init_state_dict(shapes, meta[name]["weight_seed"])
    assert np.allclose(tw.checksums(sd), z[f"{name}/weight_checksums"], rtol=1e-12, atol=1e-9)
    m.load_state_dict(sd, strict=True)                              # a reference-shaped state dict
    m.set_hyper(meta["temperature"])
    return m.to(DEV), sd


def _restated_model(sd, cfg, ids, am, labels, temperature):
    """T5ForConditionalGeneration's forward as plain fp32 torch ops on the GPU: (loss, logits, {name: grad})"""
    from gamer_amd.tiger import bucket_vector
    P = {k: v.to(DEV).clone().requires_grad_(True) for k, v in sd.items() if k not in tw.TIED[1:]}
    h, d, eps, D = cfg["num_heads"], cfg["d_kv"], cfg["layer_norm_epsilon"], cfg["d_model"]
    E = P["shared.weight"]
    rms = lambda x, w: w * (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps))
    heads = lambda x: x.view(x.shape[0], x.shape[1], h, d).permute(0, 2, 1, 3)

    def attn(pre, xq, xkv, rel, keep, causal):
        q, k, v = xq @ P[pre + "q.weight"].t(), xkv @ P[pre + "k.weight"].t(), xkv @ P[pre + "v.weight"].t()
        ctx, _ = _attention(heads(q), heads(k), heads(v), rel, keep, causal, None)
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


@pytest.mark.parametrize("name", ["a", "b"])
def test_model_logits_loss_and_every_gradient_match_the_reference(fx, name):
    z, meta = fx
    m, sd = _model(fx, name)
    ids, am, labels = (torch.from_numpy(z[f"{name}/{k}"]) for k in ("input_ids", "attention_mask", "labels"))
    m.train()                                                       # (dropout_rate 0: the training path, CatalogCEFn and all)
    loss, logits = m(ids.to(DEV), am.to(DEV), labels=labels.to(DEV), want_logits=True)
    loss.backward()
    r_loss, r_logits, r_grads = _restated_model(sd, meta["configs"][name], ids, am, labels, meta["temperature"])
    params = dict(m.named_parameters())
    assert set(params) == set(meta[name]["param_keys"]) and meta[name]["no_grad"] == []
    kernel, torch32 = {}, {}
    kernel["logits"], torch32["logits"] = _rel(logits, z[f"{name}/logits"]), _rel(r_logits, z[f"{name}/logits"])
    ref_loss = float(z[f"{name}/loss"])
    kernel["loss"], torch32["loss"] = abs(float(loss.detach()) - ref_loss) / abs(ref_loss), abs(float(r_loss) - ref_loss) / abs(ref_loss)
    for k, p in params.items():
        ref = torch.from_numpy(z[f"{name}/grad/{k}"])
        rows = tw.sample_rows(p.shape)
        assert p.grad is not None, k
        kernel[k], torch32[k] = _rel(p.grad[rows.to(DEV)], ref), _rel(r_grads[k][rows.to(DEV)], ref)
        # the rows the fixture does not hold: the whole tensor's sum of squares, whose relative error is twice the values'
        want = float(z[f"{name}/grad_checksum/{k}"][1])
        kernel["sumsq/" + k] = 0.5 * abs(float(tw.checksums({k: p.grad.cpu()})[0][1]) - want) / want
        torch32["sumsq/" + k] = 0.5 * abs(float(tw.checksums({k: r_grads[k].cpu()})[0][1]) - want) / want
    bar = min(2.0 * max(torch32.values()), 1e-3)
    worst = max(kernel, key=kernel.get)
    print(f"config {name}: kernel worst {kernel[worst]:.3e} ({worst}), logits {kernel['logits']:.3e}, loss {kernel['loss']:.3e}; "
          f"fp32 torch worst {max(torch32.values()):.3e}, logits {torch32['logits']:.3e}; bar {bar:.3e}")
    for k, e in kernel.items():
        assert e <= bar, (k, e, bar)


def test_forward_without_labels_gives_the_logits(fx):
    z, meta = fx
    m, _ = _model(fx, "a")
    m.eval()
    ids, am, labels = (torch.from_numpy(z[f"a/{k}"]).to(DEV) for k in ("input_ids", "attention_mask", "labels"))
    with torch.no_grad():
        loss, logits = m(ids, am, decoder_input_ids=m._shift_right(labels))
        loss2, logits2 = m(ids, am, labels=labels)
    assert loss is None and _rel(logits, z["a/logits"]) < 1e-3
    assert torch.equal(logits, logits2) and abs(float(loss2) - float(z["a/loss"])) < 1e-3 * float(z["a/loss"])
    with pytest.raises(RuntimeError, match="HIP device only"):
        m(ids.cpu(), am.cpu(), labels=labels.cpu())


# ---- beam search ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", [4, 20])
@pytest.mark.parametrize("tag", ["plain", "prefix"])
def test_beam_search_finds_generates_beams(fx, tag, nb):
    from gamer_amd import tiger
    from gamer_amd.decode import ItemTrie
    z, meta = fx
    m, _ = _model(fx, "a")
    ids, am = torch.from_numpy(z["a/input_ids"][:3]).to(DEV), torch.from_numpy(z["a/attention_mask"][:3]).to(DEV)
    trie = ItemTrie(z[f"a/trie_{tag}"].tolist(), device=DEV, pad_token_id=0)
    prefix = torch.from_numpy(z[f"a/prefix_{tag}"])
    steps = z[f"a/beams_{tag}_{nb}"].shape[1] - prefix.shape[1]
    seqs, scores = tiger.beam_search(m, ids, am, trie, nb, steps, decoder_prefix=None if tag == "plain" else prefix)
    ref_s = torch.from_numpy(z[f"a/scores_{tag}_{nb}"])
    assert torch.equal(seqs.cpu(), torch.from_numpy(z[f"a/beams_{tag}_{nb}"]))
    assert _rel(scores, ref_s) < 1e-3
    # one user alone: the same beams as that user's rows of the batch
    one_s, one_sc = tiger.beam_search(m, ids[1:2], am[1:2], trie, nb, steps, decoder_prefix=None if tag == "plain" else prefix[1:2])
    assert torch.equal(one_s, seqs[nb:2 * nb]) and torch.allclose(one_sc, scores[nb:2 * nb], rtol=1e-5, atol=1e-6)


# ---- memory -------------------------------------------------------------------------------------------------------------------------------
def test_attention_needs_no_score_sized_memory():
    from gamer_amd import ops
    B, S, h, d = 1024, 101, 6, 64
    I = h * d
    qkv = torch.randn(B * S, 3 * I, device=DEV) * 0.3
    dqkv, o, d_o = torch.empty_like(qkv), torch.empty(B * S, I, device=DEV), torch.randn(B * S, I, device=DEV)
    lse, rel = torch.empty(B, h, S, device=DEV), torch.randn(h, 2 * S - 1, device=DEV)
    slabs = torch.empty(ops.t5_n_slab(B, h), h, 2 * S - 1, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ops.t5_attn_fwd(qkv[:, :I], qkv[:, I:2 * I], qkv[:, 2 * I:], rel, None, B, S, S, h, d, False, 0.1, 3, o, lse)
    ops.t5_attn_bwd(qkv[:, :I], qkv[:, I:2 * I], qkv[:, 2 * I:], rel, None, B, S, S, h, d, False, 0.1, 3, d_o, lse, dqkv[:, :I],
                    dqkv[:, I:2 * I], dqkv[:, 2 * I:], slabs)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base
    assert extra < B * h * S * S * 4, extra                                   # one [B, h, S, S] fp32 tensor: 250 MB
    assert bool(torch.isfinite(dqkv).all()) and bool(torch.isfinite(slabs).all())


def test_a_training_step_forms_no_logits(fx, monkeypatch):
    from gamer_amd import ops
    z, meta = fx
    m, _ = _model(fx, "b")
    m.train()
    V = meta["configs"]["b"]["vocab_size"]
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(2, V, (256, 101), generator=g)
    labels = torch.randint(2, V, (256, 5), generator=g)
    seen = []
    real = ops.linear_fwd
    monkeypatch.setattr(ops, "linear_fwd", lambda x, ldx, W, ldw, y, ldy, M, N, K, **kw: (seen.append(N), real(x, ldx, W, ldw, y, ldy, M, N, K, **kw))[1])
    monkeypatch.setattr(m, "logits", lambda *a: (_ for _ in ()).throw(AssertionError("the logits were formed")))
    loss, logits = m(ids.to(DEV), torch.ones_like(ids).to(DEV), labels=labels.to(DEV))
    loss.backward()
    assert logits is None and V not in seen and bool(torch.isfinite(loss))
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.parameters())


# ---- dropout, end to end ----------------------------------------------------------------------------------------------------------------
def test_dropout_is_repeatable_from_the_seed_counters(fx):
    from gamer_amd import modules, rec_common
    z, meta = fx
    m, _ = _model(fx, "a", dropout=0.1)
    m.train()
    ids, am, labels = (torch.from_numpy(z[f"a/{k}"]).to(DEV) for k in ("input_ids", "attention_mask", "labels"))

    def run(seed):
        modules._SeedCounter.value, rec_common._Seeds.value = 1000 + seed, 2000 + seed
        for p in m.parameters():
            p.grad = None
        loss, _ = m(ids, am, labels=labels)
        loss.backward()
        return loss.detach().clone(), [p.grad.clone() for p in m.parameters()]
    l1, g1 = run(0)
    l2, g2 = run(0)
    l3, _ = run(1)
    assert torch.equal(l1, l2) and all(torch.equal(a, b) for a, b in zip(g1, g2))
    assert not torch.equal(l1, l3) and abs(float(l1) - float(z["a/loss"])) > 1e-4
    assert all(bool(torch.isfinite(g).all()) for g in g1)


def test_train_tiger_end_to_end(tmp_path, capsys):
    from gamer_amd import synthetic, train_tiger
    root = tmp_path / "data"
    synthetic.write_seqrec_dataset(str(root), "Toy", n_users=40, n_items=60, codebook=8, seed=1)
    base = tmp_path / "base"
    base.mkdir()
    (base / "config.json").write_text(json.dumps(dict(d_model=64, d_kv=32, d_ff=128, num_layers=2, num_decoder_layers=2, num_heads=2,
                                                      dropout_rate=0.1, vocab_size=32128, task_specific_params={"x": 1})))
    out = tmp_path / "ckpt"
    common = ["--base_model", str(base), "--data_path", str(root), "--dataset", "Toy", "--max_his_len", "10", "--output_dir", str(out),
              "--per_device_batch_size", "64", "--test_batch_size", "16", "--num_beams", "10", "--metrics", "hit@1,hit@5,ndcg@5",
              "--results_file", str(tmp_path / "res.json")]
    res = train_tiger.main(common + ["--epochs", "2", "--learning_rate", "3e-3", "--warmup_ratio", "0.0"])
    log = capsys.readouterr().out
    losses = [float(l.split(" loss ")[1].split()[0]) for l in log.splitlines() if " loss " in l and "epoch" in l]
    assert len(losses) == 2 and losses[1] < losses[0], log
    assert (out / "best_model.pth").exists()
    sd = torch.load(out / "best_model.pth", map_location="cpu")
    assert "shared.weight" in sd and "lm_head.weight" in sd
    first = json.loads((tmp_path / "res.json").read_text())
    again = train_tiger.main(common + ["--only_test"])
    assert again == res and json.loads((tmp_path / "res.json").read_text()) == first
    assert set(res) >= {"hit@1", "hit@5", "ndcg@5"} and all(0.0 <= res[k] <= 1.0 for k in ("hit@1", "hit@5", "ndcg@5"))
