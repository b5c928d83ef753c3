"""PBAT's kernels and model on the GPU: the fused Wasserstein attention and the head's pieces against fp64 torch restatements of
the reference's formulas written here in their PAIRWISE form ([B, h, L, L, d] fused tensors, never the compact S[i, t_j] form the
kernel uses), and the model against the real reference class (tests/golden/pbat_small.npz, tools/make_golden_pbat.py).

Bars: the project's fp32 bars for these models, 2e-5 of the largest magnitude for outputs, loss and scores and 2e-4 for gradients
(``_rel``).  The Wasserstein forms cancel (|a|^2 + |b|^2 - 2 a.b), so every comparison also evaluates the same restatement in fp32
torch and prints its error beside the kernel's; where that error exceeds half the bar, the case's bar is twice the restatement's
error (``_bar``).  Worst pairs measured on MI355X are in the README's PBAT row.

Measured on MI355X (kernel / fp32 torch restatement, worst over the 36 attention shapes): see README (f)15."""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import pbat_weights as pw  # noqa: E402

pytestmark = pytest.mark.gpu
FX = os.path.join(os.path.dirname(__file__), "golden", "pbat_small.npz")
DEV = "cuda:0"
FMIN = float(torch.finfo(torch.float32).min)
EPS = 1e-24
OUT_BAR, GRAD_BAR = 2e-5, 2e-4


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("needs the GPU")
    from gamer_amd import build
    build.build()


def _rel(got, ref):
    got, ref = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(ref).detach().double().cpu()
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def _bar(base, e32):
    """the case's bar: ``base``, or twice the fp32 torch restatement's own error where that exceeds half of it"""
    return 2 * e32 if math.isfinite(e32) and e32 > base / 2 else base


# ---- the formulas of FBAMultiHeadAttention.forward, pair by pair, in the dtype of their inputs -------------------------------------
def _tri(m1, m2, m3, c1, c2, c3):
    c1, c2, c3 = c1.clamp(min=EPS), c2.clamp(min=EPS), c3.clamp(min=EPS)
    cov = 1.0 / (1.0 / c1 + 1.0 / c2 + 1.0 / c3)
    return cov * (m1 / c1 + m2 / c2 + m3 / c3), cov


def _wass(m1, c1, m2, c2):
    """the distance of Gaussian pairs along the last axis, in the reference's expanded form"""
    mean = (m1 ** 2).sum(-1) + (m2 ** 2).sum(-1) - 2 * (m1 * m2).sum(-1)
    cov = c1.sum(-1) + c2.sum(-1) - 2 * (torch.sqrt(c1.clamp(min=EPS)) * torch.sqrt(c2.clamp(min=EPS))).sum(-1)
    return mean + cov


def _attention(t, types, keep, drop=None):
    """t: q1 .. v2 [B, h, L, d], Rm / Rc [B, h, b + 1, b + 1, d], pm / pc [h, L, d], wq1 .. bk2; types long [B, L]; keep bool
    [B, L]; drop [B, h, L, L] dropout multipliers or None.  Forms every [B, h, L, L, d] tensor of the reference."""
    B, h, L, d = t["q1"].shape
    lin = lambda x, n: x @ t["w" + n].t() + t["b" + n]
    bi = torch.arange(B, device=types.device)[:, None, None]
    Rm = t["Rm"][bi, :, types[:, :, None], types[:, None, :]].permute(0, 3, 1, 2, 4)            # [B, h, L, L, d]: R[t_i, t_j]
    Rc = t["Rc"][bi, :, types[:, :, None], types[:, None, :]].permute(0, 3, 1, 2, 4)
    pm, pc = t["pm"][None, :, :, None, :], t["pc"][None, :, :, None, :]
    # (as the reference: the KEY projection sits on the query axis too)
    fQm, fQc = _tri(t["q1"][:, :, :, None, :], lin(Rm, "q1"), lin(t["pm"], "q2")[None, :, :, None, :], t["q2"][:, :, :, None, :], Rc, pc)
    fKm, fKc = _tri(t["k1"][:, :, :, None, :], lin(Rm, "k1"), lin(t["pm"], "k2")[None, :, :, None, :], t["k2"][:, :, :, None, :], Rc, pc)
    assert fQm.shape == (B, h, L, L, d) and pm.shape[-1] == d
    score = -_wass(fQm, fQc, fKm, fKc) * math.sqrt(1.0 / d)
    score = score + (~keep)[:, None, None, :].to(score.dtype) * FMIN
    p = torch.softmax(score, dim=-1)
    pd = p if drop is None else p * drop
    return pd @ t["v1"], pd @ t["v2"], p


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


def _rows(B, L, b, g):
    """(types, keep): row 0 full with every type that fits, row 1 as short as can be, row 2 with type 2 absent and padding behind
    it (when L allows), further rows ragged"""
    types, keep = torch.zeros(B, L, dtype=torch.long), torch.zeros(B, L, dtype=torch.bool)
    lens = [L, 1, max(1, L - max(1, L // 3))] + [int(torch.randint(1, L + 1, (1,), generator=g)) for _ in range(B - 3)]
    for r, n in enumerate(lens[:B]):
        types[r, :n] = torch.randint(1, b + 1, (n,), generator=g)
        keep[r, :n] = True
    types[0, :min(L, b)] = torch.arange(1, b + 1)[:L]
    if B > 2:
        types[2][types[2] == 2] = 1
    return types, keep


NAMES = ("q1", "q2", "k1", "k2", "v1", "v2")
WNAMES = ("wq1", "bq1", "wq2", "bq2", "wk1", "bk1", "wk2", "bk2")


def _inputs(B, h, L, d, b, g, clamp_case=False):
    cov = lambda *s: F.elu(torch.randn(*s, generator=g, dtype=torch.float64)) + 1
    t = dict(q1=torch.randn(B, h, L, d, generator=g, dtype=torch.float64), q2=cov(B, h, L, d),
             k1=torch.randn(B, h, L, d, generator=g, dtype=torch.float64), k2=cov(B, h, L, d),
             v1=torch.randn(B, h, L, d, generator=g, dtype=torch.float64), v2=cov(B, h, L, d),
             Rm=0.5 * torch.randn(B, h, b + 1, b + 1, d, generator=g, dtype=torch.float64), Rc=cov(B, h, b + 1, b + 1, d),
             pm=0.5 * torch.randn(h, L, d, generator=g, dtype=torch.float64), pc=cov(h, L, d))
    for n in ("q1", "q2", "k1", "k2"):
        t["w" + n] = torch.randn(d, d, generator=g, dtype=torch.float64) / math.sqrt(d)
        t["b" + n] = 0.1 * torch.randn(d, generator=g, dtype=torch.float64)
    if clamp_case:
        for n, (lo, hi) in (("q2", (0, 3)), ("k2", (2, 5)), ("Rc", (1, 2)), ("pc", (4, 6))):
            flat = t[n].view(-1, d)
            flat[::3, lo:hi:2] = 0.0                      # both clamp branches: exactly zero, and positive below 1e-24
            flat[1::3, lo + 1:hi:2] = 1e-30
    return t


def _flat(x):
    """[B, h, L, d] -> [B L, h d] fp32 on the device"""
    B, h, L, d = x.shape
    return x.permute(0, 2, 1, 3).reshape(B * L, h * d).float().contiguous().to(DEV)


def _kernel(t, types, keep, g1, g2, p=0.0, seed=0, n_partial=None, poison=False):
    """forward + backward of the op on fp32 copies; returns tensors in the layout of ``_attention``'s inputs"""
    from gamer_amd import ops
    B, h, L, d = t["q1"].shape
    b = t["Rm"].shape[2] - 1
    H, NP = h * d, (b + 1) ** 2
    pm_all = torch.cat([_flat(t[n]) for n in ("q1", "k1", "v1")], 1)
    pc_all = torch.cat([_flat(t[n]) for n in ("q2", "k2", "v2")], 1)
    proj = (pm_all[:, :H], pc_all[:, :H], pm_all[:, H:2 * H], pc_all[:, H:2 * H], pm_all[:, 2 * H:], pc_all[:, 2 * H:])
    rel = lambda x: x.permute(0, 2, 3, 1, 4).reshape(B, NP, H).float().contiguous().to(DEV)
    pos = lambda x: x.permute(1, 0, 2).reshape(L, H).float().contiguous().to(DEV)
    W = tuple(t[n].float().contiguous().to(DEV) for n in WNAMES)
    ty, kp = types.to(torch.int32).to(DEV), keep.to(torch.int32).to(DEV)
    fill = float("nan") if poison else 0.0
    new = lambda *s: torch.full(s, fill, dtype=torch.float32, device=DEV)
    o = new(2, B * L, H)
    S, lse = new(B, h, L, b + 1), new(B, h, L)
    scale = math.sqrt(1.0 / d)
    args = (proj, rel(t["Rm"]), rel(t["Rc"]), pos(t["pm"]), pos(t["pc"]), W, ty, kp, B, L, h, d, b, scale, p, seed)
    ops.pbat_attn_fwd(*args, o[0], o[1], S, lse)
    dpm, dpc = new(B * L, 3 * H), new(B * L, 3 * H)
    dproj = (dpm[:, :H], dpc[:, :H], dpm[:, H:2 * H], dpc[:, H:2 * H], dpm[:, 2 * H:], dpc[:, 2 * H:])
    drm, drc = new(B, NP, H), new(B, NP, H)
    n = ops.pbat_n_partial(B, h) if n_partial is None else n_partial
    wpart, ppart = torch.zeros(n, h, 4 * (d * d + d), device=DEV), torch.zeros(n, h, 4, L, d, device=DEV)
    ops.pbat_attn_bwd(*args, S, lse, _flat(g1), _flat(g2), dproj, drm, drc, wpart, ppart)
    dw = wpart.double().sum((0, 1)).view(4, d * d + d).cpu()
    dpos = ppart.double().sum(0).cpu()                                            # [h, 4, L, d]
    unflat = lambda x: x.view(B, L, h, d).permute(0, 2, 1, 3).cpu()
    unrel = lambda x: x.view(B, b + 1, b + 1, h, d).permute(0, 3, 1, 2, 4).cpu()
    out = dict(o1=unflat(o[0]), o2=unflat(o[1]), S=S.cpu(), lse=lse.cpu(), Rm=unrel(drm), Rc=unrel(drc), pm=dpos[:, 0], pc=dpos[:, 1],
               wq1=dw[0, :d * d].view(d, d), bq1=dw[0, d * d:], wk1=dw[1, :d * d].view(d, d), bk1=dw[1, d * d:],
               wq2=dw[2, :d * d].view(d, d), bq2=dw[2, d * d:], wk2=dw[3, :d * d].view(d, d), bk2=dw[3, d * d:],
               raw=(o.clone(), dpm.clone(), dpc.clone(), drm.clone(), drc.clone(), wpart.clone(), ppart.clone()))
    for i, nm in enumerate(NAMES):
        out[nm] = unflat(dproj[i])
    return out


def _reference(t, types, keep, g1, g2, drop, dtype):
    """(o1, o2, gradients by name) of the pairwise restatement in ``dtype`` on the device"""
    tt = {k: v.to(dtype).to(DEV).requires_grad_(True) for k, v in t.items()}
    o1, o2, _ = _attention(tt, types.to(DEV), keep.to(DEV), None if drop is None else drop.to(dtype).to(DEV))
    ((o1 * g1.to(dtype).to(DEV)).sum() + (o2 * g2.to(dtype).to(DEV)).sum()).backward()
    return dict(o1=o1.detach().cpu(), o2=o2.detach().cpu(), **{k: v.grad.cpu() for k, v in tt.items()})


def _compare(name, got, ref64, ref32):
    worst = {}
    for k in ref64:
        base = OUT_BAR if k in ("o1", "o2") else GRAD_BAR
        if float(ref64[k].abs().max()) == 0:               # (L = 1: one key, no score gradient) exactly zero here too
            assert float(got[k].abs().max()) == 0, (name, k)
        e, e32 = _rel(got[k], ref64[k]), _rel(ref32[k], ref64[k])
        bar = _bar(base, e32)
        print(f"  {name} {k:4s} kernel {e:.2e}  torch-fp32 {e32:.2e}  bar {bar:.1e}" + ("  (bar from the restatement)" if bar != base else ""))
        worst[k] = (e, e32, bar)
    bad = {k: v for k, v in worst.items() if not v[0] < v[2]}
    assert not bad, (name, bad)
    return worst


def _case(L, d, b, B=3, h=2, p=0.0, seed=0, clamp_case=False, tag=""):
    g = torch.Generator().manual_seed(1000 * L + 10 * d + b)
    t = _inputs(B, h, L, d, b, g, clamp_case)
    types, keep = _rows(B, L, b, g)
    g1 = torch.randn(B, h, L, d, generator=g, dtype=torch.float64)
    g2 = torch.randn(B, h, L, d, generator=g, dtype=torch.float64)
    drop = _keep_mask(p, seed, B, h, L) if p > 0 else None
    got = _kernel(t, types, keep, g1, g2, p, seed)
    ref64 = _reference(t, types, keep, g1, g2, drop, torch.float64)
    ref32 = _reference(t, types, keep, g1, g2, drop, torch.float32)
    return _compare(f"L{L} d{d} b{b}{tag}", got, ref64, ref32), drop


@pytest.mark.parametrize("b", [2, 4, 8])
@pytest.mark.parametrize("d", [16, 32, 64])
@pytest.mark.parametrize("L", [1, 7, 50, 128])
def test_attention_against_the_fp64_pairwise_restatement(L, d, b):
    _case(L, d, b)


def test_attention_with_clamped_covariances():
    """covariances of 0 and 1e-30 among q2, k2, R_c and pos_c: both clamp branches and their zero gradients"""
    worst, _ = _case(7, 16, 4, clamp_case=True, tag=" clamp")
    g = torch.Generator().manual_seed(1000 * 7 + 160 + 4)
    t = _inputs(3, 2, 7, 16, 4, g, True)
    assert bool((t["q2"] == 0).any()) and bool((t["q2"] == 1e-30).any()) and bool((t["Rc"] == 0).any())


def test_attention_with_dropout_on_the_kernels_own_mask():
    p = 0.3
    _, drop = _case(50, 32, 4, p=p, seed=0x1234567, tag=" p0.3")
    n = drop.numel()
    kept = float((drop != 0).double().mean())
    sd = math.sqrt(0.7 * 0.3 / n)
    print(f"  kept share {kept:.5f} of {n} (0.7 +- {5 * sd:.5f})")
    assert abs(kept - 0.7) < 5 * sd
    assert set(drop.unique().tolist()) == {0.0, float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))}


def test_equal_types_get_bit_equal_probabilities():
    """v1 = the identity: o1[i] is row i of the probabilities.  Two keys of one type hold the same bits; the restatement's rows
    agree with them"""
    B, h, L, d, b = 3, 2, 32, 32, 4
    g = torch.Generator().manual_seed(5)
    t = _inputs(B, h, L, d, b, g)
    t["v1"] = torch.eye(L, dtype=torch.float64).expand(B, h, L, d).clone()
    types, keep = _rows(B, L, b, g)
    z = torch.zeros(B, h, L, d, dtype=torch.float64)
    got = _kernel(t, types, keep, z, z)
    P = got["o1"]                                                                   # [B, h, L(i), L(j)]
    pairs = 0
    for r in range(B):
        for a in range(1, b + 1):
            js = [j for j in range(L) if keep[r, j] and int(types[r, j]) == a]
            for j in js[1:]:
                assert torch.equal(P[r, :, :, j], P[r, :, :, js[0]])
                pairs += 1
        assert float(P[r][:, :, ~keep[r]].abs().max()) == 0 if bool((~keep[r]).any()) else True
    assert pairs > 20
    with torch.no_grad():
        _, _, p64 = _attention({k: v.to(DEV) for k, v in t.items()}, types.to(DEV), keep.to(DEV))
    assert _rel(P, p64) < OUT_BAR
    assert _rel(P.sum(-1), torch.ones(B, h, L)) < 1e-5


def test_repeats_rows_poison_and_slab_counts():
    B, h, L, d, b = 5, 2, 50, 32, 4
    g = torch.Generator().manual_seed(9)
    t = _inputs(B, h, L, d, b, g)
    types, keep = _rows(B, L, b, g)
    g1, g2 = torch.randn(B, h, L, d, generator=g, dtype=torch.float64), torch.randn(B, h, L, d, generator=g, dtype=torch.float64)
    a = _kernel(t, types, keep, g1, g2, 0.2, 7)
    again = _kernel(t, types, keep, g1, g2, 0.2, 7, poison=True)                     # outputs pre-filled with NaN
    for x, y in zip(a["raw"], again["raw"]):
        assert bool(torch.isfinite(y).all()) and torch.equal(x, y)
    # a row alone equals the row in the batch (dropout off: the mask's index holds the batch row)
    full = _kernel(t, types, keep, g1, g2)
    for r in (0, 1, 2):
        one = {k: (v[r:r + 1] if v.shape[0] == B and k not in ("pm", "pc") and not k.startswith(("w", "b")) else v) for k, v in t.items()}
        alone = _kernel(one, types[r:r + 1], keep[r:r + 1], g1[r:r + 1], g2[r:r + 1])
        for k in ("o1", "o2", "Rm", "Rc") + NAMES:
            assert torch.equal(alone[k][0], full[k][r]), (r, k)
    # slab counts 1 and several: the same sums
    for n in (1, 2, 5):
        few = _kernel(t, types, keep, g1, g2, 0.2, 7, n_partial=n)
        for k in WNAMES + ("pm", "pc"):
            assert _rel(few[k], a[k]) < 1e-6, (n, k)
        for k in ("o1", "o2", "Rm", "Rc") + NAMES:
            assert torch.equal(few[k], a[k]), (n, k)


def test_attention_wrapper_limits():
    from gamer_amd import ops
    for L, H, d, b in ((129, 64, 32, 4), (50, 136, 68, 4), (50, 60, 30, 4), (50, 64, 32, 9)):
        with pytest.raises(NotImplementedError, match="PBAT on the HIP path"):
            ops.pbat_check_limits(L, H, d, b)


# ---- the head's pieces ---------------------------------------------------------------------------------------------------------------
def _head_ref(hm, hc, Em, Ec, V, target, dtype):
    hm, hc, Em, Ec = (x.to(dtype).to(DEV).requires_grad_(True) for x in (hm, hc, Em, Ec))
    em, ec = Em[:V], F.elu(Ec[:V]) + 1
    dist = _wass(hm[:, None, :], hc[:, None, :], em[None], ec[None])                # [R, V], the reference's expanded form
    loss = F.cross_entropy(dist, target.to(DEV))
    loss.backward()
    return dict(dist=dist.detach().cpu(), loss=loss.detach().cpu(), hm=hm.grad.cpu(), hc=hc.grad.cpu(), Em=Em.grad[:V].cpu(), Ec=Ec.grad[:V].cpu())


@pytest.mark.parametrize("H", [16, 64, 128])
@pytest.mark.parametrize("R", [1, 37, 130])
def test_head_pieces_loss_and_topk_against_fp64(R, H):
    from gamer_amd import ops
    V = 300
    g = torch.Generator().manual_seed(R * 1000 + H)
    hm, hc = torch.randn(R, H, generator=g, dtype=torch.float64), torch.randn(R, H, generator=g, dtype=torch.float64)
    assert bool((hc < 0).any())
    Em, Ec = 0.5 * torch.randn(V + 1, H, generator=g, dtype=torch.float64), torch.randn(V + 1, H, generator=g, dtype=torch.float64)
    target = torch.randint(0, V, (R,), generator=g)
    ref64, ref32 = _head_ref(hm, hc, Em, Ec, V, target, torch.float64), _head_ref(hm, hc, Em, Ec, V, target, torch.float32)
    f = lambda x: x.float().contiguous().to(DEV)
    hm_, hc_, Em_, Ec_ = f(hm), f(hc), f(Em), f(Ec)
    Em_[V], Ec_[V] = float("nan"), float("nan")                                   # the <MASK> row is never read
    new = lambda *s: torch.full(s, float("nan"), device=DEV)
    x, a, E2, c = new(R, 2 * H), new(R), new(V, 2 * H), new(V)
    ops.wass_rows_fwd(hm_, hc_, x, a)
    ops.wass_table_fwd(Em_, Ec_, V, E2, c)
    # the pieces against their formulas in fp64
    ec64 = F.elu(Ec[:V]) + 1
    assert _rel(x, torch.cat([-2 * hm, -2 * torch.sqrt(hc.clamp(min=EPS))], 1)) < 1e-6
    assert _rel(a, (hm ** 2).sum(1) + hc.sum(1)) < 1e-5
    assert _rel(E2, torch.cat([Em[:V], torch.sqrt(ec64)], 1)) < 1e-6 and _rel(c, (Em[:V] ** 2).sum(1) + ec64.sum(1)) < 1e-5
    dist = a.double()[:, None] + c.double()[None, :] + x.double() @ E2.double().t()
    e, e32 = _rel(dist, ref64["dist"]), _rel(ref32["dist"], ref64["dist"])
    print(f"  R{R} H{H} distances kernel {e:.2e} torch-fp32 {e32:.2e}")
    assert e < _bar(OUT_BAR, e32)
    # the composed loss and its gradients
    lse, loss, bad = new(R), torch.empty((), device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    tgt = target.to(DEV)
    ops.catalog_ce_bias_fwd(x, None, E2, c, tgt, lse, loss, bad, V)
    assert int(bad) == 0
    dE2, dx, dc = torch.zeros(V, 2 * H, device=DEV), new(R, 2 * H), new(V)
    ops.catalog_ce_bias_bwd(x, None, E2, c, tgt, lse, torch.ones((), device=DEV), 1.0 / R, dE=dE2, dh=dx, dbias=dc, V=V)
    dhm, dhc, dEm, dEc = new(R, H), new(R, H), torch.zeros(V + 1, H, device=DEV), torch.zeros(V + 1, H, device=DEV)
    ops.wass_rows_bwd(hm_, hc_, dx, None, dhm, dhc)
    ops.wass_table_bwd(Em_, Ec_, V, dE2, dc, dEm, dEc)
    assert float(dEm[V].abs().max()) == 0 and float(dEc[V].abs().max()) == 0
    # (a_r shifts every logit of a row alike: the cross entropy does not see it, but fp32 softmax of the restatement does)
    el = abs(float(loss) - float(ref64["loss"])) / abs(float(ref64["loss"]))
    el32 = abs(float(ref32["loss"]) - float(ref64["loss"])) / abs(float(ref64["loss"]))
    print(f"  R{R} H{H} loss kernel {el:.2e} torch-fp32 {el32:.2e}")
    assert el < _bar(OUT_BAR, el32)
    for k, got in (("hm", dhm), ("hc", dhc), ("Em", dEm[:V]), ("Ec", dEc[:V])):
        e, e32 = _rel(got, ref64[k]), _rel(ref32[k], ref64[k])
        print(f"  R{R} H{H} d{k} kernel {e:.2e} torch-fp32 {e32:.2e}")
        assert e < _bar(GRAD_BAR, e32), k
    # the rows' and the table's backward halves with da / dc given, against fp64 autograd
    hm2, hc2 = hm.clone().requires_grad_(True), hc.clone().requires_grad_(True)
    wx, wa = torch.randn(R, 2 * H, generator=g, dtype=torch.float64), torch.randn(R, generator=g, dtype=torch.float64)
    ((torch.cat([-2 * hm2, -2 * torch.sqrt(hc2.clamp(min=EPS))], 1) * wx).sum() + (((hm2 ** 2).sum(1) + hc2.sum(1)) * wa).sum()).backward()
    ops.wass_rows_bwd(hm_, hc_, f(wx), f(wa), dhm, dhc)
    assert _rel(dhm, hm2.grad) < 1e-5 and _rel(dhc, hc2.grad) < 1e-5
    assert float(dhc[hc_ < 0].double().sub(wa.to(DEV)[:, None].expand(R, H)[hc_ < 0]).abs().max()) < 1e-6      # clamped: only a's share
    # top-10 against the stable argsort of the materialised fp64 distances
    idx, sc = ops.catalog_topk_bias(x, E2, c, 10, 0, V, V=V)
    sc = sc + a[:, None]
    ref_top = torch.argsort(-ref64["dist"], dim=1, stable=True)[:, :10]
    tol = OUT_BAR * float(ref64["dist"].abs().max())
    assert int(idx.max()) < V
    for r in range(R):
        for q in range(10):
            i, j = int(idx[r, q]), int(ref_top[r, q])
            assert i == j or abs(float(ref64["dist"][r, i]) - float(ref64["dist"][r, j])) < tol, (r, q, i, j)
    assert _rel(sc, torch.gather(ref64["dist"], 1, idx.cpu())) < _bar(OUT_BAR, e32)


# ---- the model against the real class --------------------------------------------------------------------------------------------------
def _model(second=False):
    from gamer_amd.pbat import PBAT, PBATConfig
    z = np.load(FX)
    m = json.loads(str(z["meta_json"]))
    m = m["second"] if second else m
    model = PBAT(PBATConfig(**m["config"]), m["n_items"], m["n_users"], m["max_his_len"], m["n_behaviors"])
    sd = pw.init_state_dict({k: tuple(s) for k, s in zip(m["keys"], m["shapes"])}, m["weight_seed"])
    model.load_state_dict(sd, strict=True)
    P = "b/" if second else ""
    return model.to(DEV), (lambda k: z[P + k]), m, [f[len(P):] for f in z.files if f.startswith(P + "grad/")]


def _dev(z, k):
    return torch.from_numpy(z(k)).to(DEV)


@pytest.mark.parametrize("second", [False, True])
def test_pbat_forward_loss_and_grads_match_reference(second):
    model, z, m, grad_keys = _model(second)
    masked, labels, beh, uid = _dev(z, "masked"), _dev(z, "labels"), _dev(z, "behaviors"), _dev(z, "uid")
    model.train()                                          # (dropout_prob 0 in the fixture's config)
    logits, valid_labels = model(masked, beh, uid, labels)
    assert torch.equal(valid_labels.cpu(), torch.from_numpy(z("valid_labels")))
    assert logits.shape == (valid_labels.numel(), m["n_items"] + 1)
    cols = torch.from_numpy(z("cols"))
    e_logits = _rel(logits.cpu()[:, cols], z("logits_cols"))
    model.zero_grad()
    loss = model.calculate_loss(dict(inputs=_dev(z, "inputs"), behaviors=beh, uid=uid), masked_labels=(masked, labels))
    loss.backward()
    e_loss = abs(float(loss.detach()) - float(z("loss"))) / abs(float(z("loss")))
    print(f"second={second}: logits {e_logits:.2e} loss {e_loss:.2e}")
    assert e_logits < OUT_BAR and e_loss < OUT_BAR
    assert model.last_masked_count == valid_labels.numel() == m["M"]
    seen, worst = 0, ("", 0.0)
    for k, p in model.named_parameters():
        if k in m["no_grad"]:
            assert p.grad is None, k
        elif "grad/" + k in grad_keys:
            e = _rel(p.grad, z("grad/" + k))
            worst = max(worst, (k, e), key=lambda t: t[1])
            assert p.grad is not None and p.grad.shape == p.shape and e < GRAD_BAR, (k, e)
            seen += 1
    print(f"second={second}: {seen} gradient tensors, worst {worst[0]} {worst[1]:.2e}")
    named = dict(model.named_parameters())
    assert seen == len(grad_keys) == len(named) - len(m["no_grad"]) - 2 and m["zero_grad"] == []
    rows = torch.from_numpy(z("rows"))
    assert m["n_items"] + 1 in rows.tolist() and 0 in rows.tolist()
    for k in pw.ALIASES.values():
        gi = named[k].grad
        assert _rel(gi.cpu()[rows], z("grad_rows/" + k)) < GRAD_BAR, k
        ck, ref = pw.checksums({"g": gi.cpu()})[0], z("grad_checksum/" + k)
        assert abs(ck[0] - ref[0]) < 2e-4 * np.sqrt(ref[1]) * 10 and abs(ck[1] - ref[1]) < 1e-3 * ref[1], k
    # M = 1: the reference's head returns 1-D logits, which its loss accepts; the same loss here
    model.zero_grad()
    l1 = model.calculate_loss(dict(inputs=_dev(z, "inputs"), behaviors=beh, uid=uid), masked_labels=(_dev(z, "m1_masked"), _dev(z, "m1_labels")))
    assert model.last_masked_count == 1 and abs(float(l1) - float(z("m1_loss"))) < OUT_BAR * abs(float(z("m1_loss")))


@pytest.mark.parametrize("second", [False, True])
def test_pbat_full_sort_matches_reference(second):
    model, z, m, _ = _model(second)
    model.eval()
    inter = dict(inputs=_dev(z, "eval_inputs"), behaviors=_dev(z, "eval_behaviors"), uid=_dev(z, "uid"), seq_len=_dev(z, "eval_seq_len"))
    scores = model.full_sort_predict(dict(inter))
    assert scores.shape == (inter["inputs"].shape[0], m["n_items"] + 1)
    cols = torch.from_numpy(z("cols"))
    assert _rel(scores.cpu()[:, cols], z("scores_cols")) < OUT_BAR
    idx, sc = model.full_sort_topk(dict(inter), 10)
    assert int(idx.max()) <= m["n_items"] and int(idx.min()) >= 0               # <MASK> is never returned
    ref_top = torch.from_numpy(z("top10"))
    full = scores.cpu()
    tol = OUT_BAR * float(full.abs().max())
    for b in range(idx.shape[0]):
        for q in range(10):
            a, r = int(idx[b, q]), int(ref_top[b, q])
            # identical ranks unless two distances lie closer than the output bar can tell apart
            assert a == r or abs(float(full[b, a]) - float(full[b, r])) < tol, (b, q, a, r)
    assert _rel(sc, torch.gather(full, 1, idx.cpu())) < OUT_BAR
    assert _rel(sc, z("top10_scores")[:, :10]) < OUT_BAR                          # the LARGEST distances come first, as the reference ranks


def test_pbat_reference_behaviours_and_deviations():
    model, z, m, _ = _model()
    model.train()
    inputs, beh, uid = _dev(z, "inputs"), _dev(z, "behaviors"), _dev(z, "uid")
    masked, labels = model.reconstruct_train_data(inputs, seed=3)
    again = model.reconstruct_train_data(inputs, seed=3)
    assert torch.equal(masked, again[0]) and torch.equal(labels, again[1])
    assert bool(((masked == inputs) | (masked == m["n_items"] + 1)).all()) and torch.equal(labels, inputs * (masked != inputs))
    assert bool((labels[inputs == 0] == 0).all())
    # a type or a user outside its table: the reference's embedding raises IndexError (recorded), and so does this, on the host
    assert m["type_error"].startswith("IndexError")
    bad = beh.clone()
    bad[0, 0] = m["n_behaviors"] + 1
    with pytest.raises(IndexError, match="behaviors outside"):
        model.calculate_loss(dict(inputs=inputs, behaviors=bad, uid=uid))
    with pytest.raises(IndexError, match="uid outside"):
        model.calculate_loss(dict(inputs=inputs, behaviors=beh, uid=uid + m["n_users"]))
    with pytest.raises(IndexError, match="behaviors outside"):
        model.full_sort_topk(dict(inputs=inputs, behaviors=-beh, uid=uid, seq_len=(inputs != 0).sum(1)), 5)
    # over-limit shapes
    long = torch.ones(2, 9, dtype=torch.long, device=DEV)
    with pytest.raises(ValueError, match="max_his_len"):
        model.calculate_loss(dict(inputs=long, behaviors=long, uid=uid[:2]))
    model.max_seq_length = 200
    long = torch.ones(2, 129, dtype=torch.long, device=DEV)
    with pytest.raises(NotImplementedError, match="L <= 128"):
        model.calculate_loss(dict(inputs=long, behaviors=long, uid=uid[:2]))
    model.max_seq_length = m["max_his_len"]
    # B = 1: IndexError in the reference (recorded); here it runs and equals the row in the batch
    assert m["b1_error"].startswith("IndexError")
    model.eval()
    ev = dict(inputs=_dev(z, "eval_inputs"), behaviors=_dev(z, "eval_behaviors"), uid=uid, seq_len=_dev(z, "eval_seq_len"))
    full = model.full_sort_predict(dict(ev))
    one = model.full_sort_predict({k: v[3:4] for k, v in ev.items()})
    assert one.shape == (1, m["n_items"] + 1) and _rel(one[0], full[3]) < 1e-6
    model.train()
    l1 = model.calculate_loss(dict(inputs=inputs[:1], behaviors=beh[:1], uid=uid[:1]), masked_labels=(_dev(z, "masked")[:1], _dev(z, "labels")[:1]))
    l1.backward()
    assert bool(torch.isfinite(l1)) and model.last_masked_count == int((z("labels")[0] != 0).sum()) > 0
    # M = 0, as recorded from the reference: NaN loss, backward() works, every gradient exactly zero, none NaN
    assert m["m0_loss_is_nan"] and m["m0_grads_all_zero"]
    model.mask_ratio = 0.0
    model.zero_grad()
    loss = model.calculate_loss(dict(inputs=inputs, behaviors=beh, uid=uid))
    assert model.last_masked_count == 0 and bool(torch.isnan(loss))
    loss.backward()
    assert [k for k, p in model.named_parameters() if p.grad is None] == m["m0_no_grad"]
    assert all(bool((p.grad == 0).all()) for p in model.parameters() if p.grad is not None)


def test_one_head_runs_here():
    """the reference cannot run with one head (recorded: its .squeeze() drops the head axis); this does"""
    from gamer_amd.pbat import PBAT, PBATConfig
    assert json.loads(str(np.load(FX)["meta_json"]))["h1_error"].startswith("RuntimeError")
    torch.manual_seed(0)
    model = PBAT(PBATConfig(hidden_size=32, n_heads=1, inner_size=64, dropout_prob=0.0), 50, 6, 8, 2).to(DEV)
    g = torch.Generator().manual_seed(1)
    inter = dict(inputs=torch.randint(1, 51, (4, 8), generator=g).to(DEV), behaviors=torch.randint(1, 3, (4, 8), generator=g).to(DEV),
                 uid=torch.randint(1, 7, (4,), generator=g).to(DEV))
    model.train()
    model.mask_ratio = 0.5
    loss = model.calculate_loss(inter)
    loss.backward()
    assert bool(torch.isfinite(loss)) and all(bool(torch.isfinite(p.grad).all()) for p in model.parameters() if p.grad is not None)


def test_state_dict_round_trip_with_the_fixture_keys():
    from gamer_amd.pbat import PBAT, PBATConfig
    model, z, m, _ = _model()
    sd = model.state_dict()
    assert list(sd) == m["keys"]
    other = PBAT(PBATConfig(**m["config"]), m["n_items"], m["n_users"], m["max_his_len"], m["n_behaviors"])
    other.load_state_dict({k: v.cpu() for k, v in sd.items()}, strict=True)


# ---- memory ----------------------------------------------------------------------------------------------------------------------
def test_attention_op_keeps_nothing_quadratic_in_memory():
    """B 1024, L 50, 2 heads of 32, 4 behaviours: the peak beyond the op's inputs, outputs and gradients stays below a tenth of ONE
    fp32 [B, h, L, L, d] tensor (655 MB; the reference holds six of them).  What is kept is [B, h, L, b + 1] plus the slabs."""
    from gamer_amd import ops
    B, L, h, d, b = 1024, 50, 2, 32, 4
    H, NP = h * d, (b + 1) ** 2
    g = torch.Generator().manual_seed(2)
    rnd = lambda *s: (torch.randn(*s, generator=g) * 0.5).to(DEV)
    pm_all, pc_all = rnd(B * L, 3 * H), (F.elu(torch.randn(B * L, 3 * H, generator=g)) + 1).to(DEV)
    proj = (pm_all[:, :H], pc_all[:, :H], pm_all[:, H:2 * H], pc_all[:, H:2 * H], pm_all[:, 2 * H:], pc_all[:, 2 * H:])
    rel_m, rel_c = rnd(B, NP, H), (F.elu(torch.randn(B, NP, H, generator=g)) + 1).to(DEV)
    pos_m, pos_c = rnd(L, H), (F.elu(torch.randn(L, H, generator=g)) + 1).to(DEV)
    W = tuple(rnd(d) if i % 2 else rnd(d, d) / 4 for i in range(8))
    types = torch.randint(0, b + 1, (B, L), generator=g).to(torch.int32).to(DEV)
    keep = (types != 0).to(torch.int32)
    o, do = torch.empty(2, B * L, H, device=DEV), rnd(2, B * L, H)
    S, lse = torch.empty(B, h, L, b + 1, device=DEV), torch.empty(B, h, L, device=DEV)
    dpm, dpc = torch.empty(B * L, 3 * H, device=DEV), torch.empty(B * L, 3 * H, device=DEV)
    dproj = (dpm[:, :H], dpc[:, :H], dpm[:, H:2 * H], dpc[:, H:2 * H], dpm[:, 2 * H:], dpc[:, 2 * H:])
    drm, drc = torch.empty(B, NP, H, device=DEV), torch.empty(B, NP, H, device=DEV)
    dw, dpos = torch.empty(4 * (d * d + d), device=DEV), torch.empty(h * 4 * L * d, device=DEV)
    scale = math.sqrt(1.0 / d)
    args = (proj, rel_m, rel_c, pos_m, pos_c, W, types, keep, B, L, h, d, b, scale, 0.2, 11)

    def run():
        ops.pbat_attn_fwd(*args, o[0], o[1], S, lse)
        n = ops.pbat_n_partial(B, h)
        wpart, ppart = torch.zeros(n, h, 4 * (d * d + d), device=DEV), torch.zeros(n, h, 4, L, d, device=DEV)
        ops.pbat_attn_bwd(*args, S, lse, do[0], do[1], dproj, drm, drc, wpart, ppart)
        ops.colsum_reduce(wpart.view(n * h, -1), dw)
        ops.colsum_reduce(ppart.view(n, -1), dpos)
    run()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    run()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    limit = B * h * L * L * d * 4 // 10
    print(f"attention op peak beyond its tensors {peak / 2 ** 20:.1f} MiB, a tenth of one [B, h, L, L, d] {limit / 2 ** 20:.1f} MiB")
    assert all(bool(torch.isfinite(x).all()) for x in (o, dpm, dpc, drm, drc, dw, dpos))
    assert S.numel() == B * h * L * (b + 1) and peak < limit, (peak, limit)


def test_training_step_does_not_materialise_distances():
    from gamer_amd.pbat import PBAT, PBATConfig
    B, V, S, b = 4096, 200_000, 20, 4
    torch.manual_seed(0)
    model = PBAT(PBATConfig(dropout_prob=0.0, n_layers=1, hidden_size=64, inner_size=128), V - 1, 100, S, b).to(DEV)
    g = torch.Generator().manual_seed(1)
    inter = dict(inputs=torch.randint(1, V, (B, S), generator=g).to(DEV), behaviors=torch.randint(1, b + 1, (B, S), generator=g).to(DEV),
                 uid=torch.randint(1, 101, (B,), generator=g).to(DEV))
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
    limit = M * V * 4                                     # one [M, V] fp32 distance tensor
    print(f"M {M} peak {peak / 2 ** 20:.0f} MiB, [M, V] {limit / 2 ** 20:.0f} MiB")
    assert peak < limit, (peak, limit)


# ---- training ----------------------------------------------------------------------------------------------------------------------
def test_pbat_dropout_training_is_finite_and_repeatable():
    from gamer_amd import modules, rec_common
    model, z, m, _ = _model()
    for mod in model.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.5
    model.dropout_prob = 0.5
    for layer in model.trm_encoder.layer:
        layer.dropout_p = 0.5
    model.train()
    inter = dict(inputs=_dev(z, "inputs"), behaviors=_dev(z, "behaviors"), uid=_dev(z, "uid"))
    res = []
    for _ in range(2):
        rec_common._Seeds.value = 77                       # (the cloze masks and the embeddings' dropout draw from this counter)
        modules._SeedCounter.value = 99
        model.zero_grad()
        loss = model.calculate_loss(inter)
        loss.backward()
        res.append([loss.detach().clone()] + [p.grad.clone() for p in model.parameters() if p.grad is not None])
    assert torch.isfinite(res[0][0]) and model.last_masked_count > 0 and len(res[0]) > 100
    assert all(bool(torch.isfinite(t).all()) for t in res[0])
    for a, b in zip(res[0], res[1]):
        assert torch.equal(a, b)
    model.eval()
    rec_common._Seeds.value = 77
    evl = model.calculate_loss(inter)
    assert not torch.equal(evl, res[0][0])                 # dropout was on


def test_train_pbat_two_epochs_and_only_test(tmp_path):
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
    run = lambda extra: subprocess.run([sys.executable, "-m", "gamer_amd.train_pbat", *common, *extra], cwd=root,
                                       capture_output=True, text=True, timeout=300)
    r = run(["--epochs", "2"])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    losses = [float(l.split(" loss ")[1].split()[0]) for l in r.stdout.splitlines() if l.startswith("[train_pbat] epoch")]
    assert len(losses) == 2 and all(math.isfinite(x) for x in losses), r.stdout
    sd = torch.load(tmp_path / "out" / "best_model.pth", map_location="cpu")
    assert sd["user_embedding_m.embedding.weight"].shape == (61, 64)                       # 60 users + padding
    assert sd["type_relation_embedding_c.embedding.weight"].shape == (10, 64)              # three behaviours
    assert torch.equal(sd["item_embedding_c.embedding.weight"], sd["head.token_embeddings_c.weight"])
    res = json.load(open(tmp_path / "res" / "result-smb_dis_target_diff.json"))
    metrics = "hit@1,hit@5,hit@10,recall@1,recall@5,recall@10,ndcg@5,ndcg@10".split(",")
    assert [e["eval_type"] for e in res] == ["Behavior click", "Behavior cart", "Behavior buy", "Merged Behavior"]
    assert all(all(k in e and math.isfinite(e[k]) for k in metrics) for e in res)
    r2 = run(["--only_test"])
    assert r2.returncode == 0, r2.stdout[-2000:] + r2.stderr[-2000:]
    assert json.load(open(tmp_path / "res" / "result-smb_dis_target_diff.json")) == res
