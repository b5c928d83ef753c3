"""Every dispatch path of the kernels each model's training step ends in - temperature cross entropy, RMSNorm, column sums,
sumsq + AdamW - against fp64 torch on the CPU, through the C ABI (gamer_amd.ops), at the sizes where the path changes.

Cross entropy: which path (forward/backward) a (dtype, V, layout) takes.  Layouts: (a) ldl = V; (b) ldl = V rounded up to 16
plus 16, base aligned; (c) as (b) with the base moved one element into a larger buffer (good ldl, unaligned base).
  vec    the row in registers as 16-byte groups (ldl % (16 / sizeof) == 0, base aligned, V <= 1280 fp32 / 1536 bf16)
  reg    forward only: the row in registers one value at a time (V <= 1280 without that alignment)
  stream forward only: two passes over memory (everything else)
  scalar backward only: the plain column loop (everything that is not vec)

             fp32 (a)       fp32 (b)       fp32 (c)       bf16 (a)       bf16 (b)       bf16 (c)
      V=1    reg/scalar     vec/vec        reg/scalar     reg/scalar     vec/vec        reg/scalar
        3    reg/scalar     vec/vec        reg/scalar     reg/scalar     vec/vec        reg/scalar
        4    vec/vec        vec/vec        reg/scalar     reg/scalar     vec/vec        reg/scalar
        5    reg/scalar     vec/vec        reg/scalar     reg/scalar     vec/vec        reg/scalar
        8    vec/vec        vec/vec        reg/scalar     vec/vec        vec/vec        reg/scalar
        9    reg/scalar     vec/vec        reg/scalar     reg/scalar     vec/vec        reg/scalar
       64    vec/vec        vec/vec        reg/scalar     vec/vec        vec/vec        reg/scalar
      255    reg/scalar     vec/vec        reg/scalar     reg/scalar     vec/vec        reg/scalar
      256    vec/vec        vec/vec        reg/scalar     vec/vec        vec/vec        reg/scalar
      257    reg/scalar     vec/vec        reg/scalar     reg/scalar     vec/vec        reg/scalar
     1041    reg/scalar     vec/vec        reg/scalar     reg/scalar     vec/vec        reg/scalar
     1279    reg/scalar     vec/vec        reg/scalar     reg/scalar     vec/vec        reg/scalar
     1280    vec/vec        vec/vec        reg/scalar     vec/vec        vec/vec        reg/scalar
     1281    stream/scalar  stream/scalar  stream/scalar  stream/scalar  vec/vec        stream/scalar
     1535    stream/scalar  stream/scalar  stream/scalar  stream/scalar  vec/vec        stream/scalar
     1536    stream/scalar  stream/scalar  stream/scalar  vec/vec        vec/vec        stream/scalar
     1537    stream/scalar  stream/scalar  stream/scalar  stream/scalar  stream/scalar  stream/scalar
     4099    stream/scalar  stream/scalar  stream/scalar  stream/scalar  stream/scalar  stream/scalar
  vec: below / at / above its limit at 1279 / 1280 / 1281 (fp32, b) and 1535 / 1536 / 1537 (bf16, b); reg: 1279 / 1280 / 1281
  (a or c); stream and scalar begin where those end.  (test_path_table_is_the_one_written_here keeps the table honest.)
  Loops: T = 8200 (the reduce kernel's eight-loads loop needs T > 7168) and T = 32800 (more rows than the 32768 waves of
  the capped grid), both at V = 5 in all three layouts.

RMSNorm: H <= 256 takes the one-chunk instantiation (4, 8, 100, 252 partly filled; 256 full), H <= 1024 the four-chunk one
(260: one lane of the second chunk; 512, 772, 1020 partly filled; 1024 full), forward and backward; T = 1, 5, 333 and a
forward with 32800 rows (row grid-stride).  Column sums: rows < 97 only the tail loop, rows >= 128 the four-way loop in every
row group (127, 128, 129 around it), cols around the 32-column workgroup.  AdamW: n < 4 tail only; 1023 / 1024 / 1025 around a
workgroup's 256 float4s; 4 * 4096 * 256 + 1029 more float4s than the 4096-workgroup cap covers in one pass, with a tail of 1.

Tolerances.  Existing bars where a quantity has one (_rel, the maximum error over the largest reference magnitude: 1e-5 CE
gradient fp32, 2^-8 bf16, 2e-6 norm forward, 1e-5 norm backward, 1e-6 AdamW; 1e-4 relative on the loss sum).  The new
elementwise metrics have bars of four times the worst value that a plain fp32 torch restatement of the same formulas, in the
kernels' operation order, reaches against the fp64 reference over every case listed here (tests/helpers/rowwise_ref.py, run
as a script, prints them), and never above the existing bar:
                                                                   fp32 torch, worst     bar
  CE lse and row loss, fp32   |err| / (|lse| + |lse - max| + 1)         1.07e-7          4.27e-7
  CE lse and row loss, bf16                                             1.33e-7          5.32e-7
  CE gradient, fp32    |err| / (|ref| + max_row |ref| + |gs| onehot)    1.36e-6          5.45e-6
  CE gradient, bf16    (one rounding to bf16: 2^-9)                     1.93e-3          2^-8 (4 x is 7.7e-3: capped)
  AdamW p              |err| / (|p (1 - lr wd)| + lr / bc1 * sm / denom)  3.40e-7        1e-6 (4 x is 1.36e-6: capped)
  AdamW m              |err| / sm, sm = |b1 m| + |(1 - b1) g|           1.53e-7          6.1e-7
  AdamW v              |err| / |v|                                      1.90e-7          7.6e-7
The factor of four is for the device's expf / logf / rsqrtf (a few ulp where libm has about one) and the wave-tree summation
order.  Two terms above are not in the plain form |err| <= r |ref| + r max_row |ref|, each for a cancellation: at the target
column the gradient is (p - 1) gs, and in a row whose peak IS its target p - 1 is some 1e-8 with every other entry smaller
still, so the 2^-24 rounding of expf's result is an error of |gs| 2^-24 whatever the row's largest entry (hence |gs| onehot);
and AdamW's update inherits the cancellation of b1 m + (1 - b1) g (hence sm in p's scale).  A lost or doubled column still
cannot hide: in the planted rows it moves lse by log 2 or more and the gradient by order one.
The GPU's worst values per family go into the per-kernel tests' report (test_ops_gpu._record, keys rowwise_*).
"""
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

import rowwise_ref as rr  # noqa: E402
from gamer_amd import ops  # noqa: E402
from oracle import qwen3multi_oracle as orc  # noqa: E402

DEV = "cuda"
F32, BF = torch.float32, torch.bfloat16
IGN = rr.IGN
NAN = float("nan")
NAME = {F32: "f32", BF: "bf16"}

LSE_BAR = {F32: 4.27e-7, BF: 5.32e-7}
GRAD_BAR = {F32: 5.45e-6, BF: 2.0 ** -8}
ADAMW_BAR = {"p": 1e-6, "m": 6.1e-7, "v": 7.6e-7}

WORST = {}


def _note(name, value):
    """worst value per family, into the report of the per-kernel tests (their _record, so both modules' entries are kept)"""
    if value <= WORST.get(name, -1.0):
        return
    WORST[name] = value
    import test_ops_gpu
    test_ops_gpu._record("rowwise_" + name, value)


def _rel(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def _bits(t):
    return t.view(torch.int32 if t.dtype == F32 else torch.int16)


def _same_bits(a, b):
    return torch.equal(_bits(a.cpu()), _bits(b.cpu()))


def dev(t):
    return None if t is None else t.to(DEV).contiguous()


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    torch.manual_seed(0)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. cross entropy
# ---------------------------------------------------------------------------------------------------------------------------
def test_path_table_is_the_one_written_here():
    """The table in the module docstring, line by line, from the dispatch rule restated in rowwise_ref.ce_paths; every path of both
    kernels and both dtypes just below, at and above its limit."""
    for V in rr.CE_VS:
        cells = ["/".join(rr.ce_paths(dt, V, lay)) for dt in (F32, BF) for lay in rr.CE_LAYOUTS]
        line = next(ln for ln in __doc__.splitlines() if ln.split() and ln.split()[0] in (str(V), f"V={V}"))
        assert line.split()[1:] == cells, (V, line, cells)
    for dt, lim in ((F32, 1280), (BF, 1536)):
        assert [rr.ce_paths(dt, V, "b") for V in (lim - 1, lim, lim + 1)] == [("vec", "vec")] * 2 + [("stream", "scalar")]
        assert [rr.ce_paths(dt, V, "c")[0] for V in (1279, 1280, 1281)] == ["reg", "reg", "stream"]


def _check_ce(case, temp, where):
    dtype, V, T, ldl = case.dtype, case.V, case.T, case.ldl
    flat0 = case.flat()
    d = flat0.to(DEV)
    labels = case.labels.to(DEV)
    lse, rl, ls, cnt = (torch.full((n,), NAN, device=DEV) for n in (T, T, 1, 1))
    ops.ce_fwd(case.rows(d), ldl, labels, V, temp, IGN, lse, rl, ls, cnt)
    # the scaled logits bit for bit (at temperature 1: unchanged), every other element of the allocation untouched
    z = case.scaled(temp)
    want = flat0.clone()
    case.rows(want)[:, :V] = z
    assert _same_bits(d, want), where
    lse_ref, mx, rl_ref, G, onehot = rr.ce_ref(z, case)
    lse_c, rl_c = lse.cpu(), rl.cpu()
    e_lse = max(rr.ce_lse_metric(lse_c, lse_ref, lse_ref, mx), rr.ce_lse_metric(rl_c, rl_ref, lse_ref, mx))
    _note("ce_lse_" + NAME[dtype], e_lse)
    assert e_lse < LSE_BAR[dtype], (where, e_lse)
    assert bool((rl_c[~case.valid] == 0).all()), where                  # ignored, out-of-range and last-of-sequence rows
    assert float(cnt) == float(case.count), (where, float(cnt), case.count)
    ref_sum = float(rl_ref.sum())
    assert abs(float(ls) - ref_sum) <= 1e-4 * ref_sum, (where, float(ls), ref_sum)
    own = rl_c.double()
    assert abs(float(ls) - float(own.sum())) <= (math.ceil(T / 1024) + 10) * 2.0 ** -24 * float(own.abs().sum()), where
    for name, use_count, denom_host, dloss, dloss_dev in rr.CE_BWD_VARIANTS:
        w = f"{where} bwd={name}"
        db = d.clone()
        ops.ce_bwd(case.rows(db), ldl, labels, V, temp, IGN, lse, cnt if use_count else None, denom_host, dloss,
                   None if dloss_dev is None else torch.tensor([dloss_dev], device=DEV))
        gb = db.cpu()
        got = case.rows(gb)[:, :V].clone()
        keep = want.clone()
        case.rows(keep)[:, :V] = got
        assert _same_bits(gb, keep), w                                   # padding columns and the allocation around the rows
        got = got.float()
        assert not bool(torch.isnan(got).any()), w
        assert bool((got[~case.valid] == 0).all()), w
        denom = float(case.count) if use_count else denom_host
        if case.count == 0:
            continue                                                    # (count = 0: exact zeros over [0, V), just asserted)
        gs = rr.ce_gs(temp, denom, dloss, dloss_dev)
        ref = G * gs
        if float(ref.abs().max()) > 0:
            e = _rel(got, ref)
            _note("ce_grad_rel_" + NAME[dtype], e)
            if dtype == F32:
                assert e < 1e-5, (w, e)
            else:
                assert float((got.double() - ref).abs().max()) <= 2.0 ** -8 * float(ref.abs().max()) + 1e-9, (w, e)
        e = rr.ce_grad_metric(got, G, onehot, gs)                       # (V = 1: the reference is zero, this is |got| / |gs|)
        _note("ce_grad_elem_" + NAME[dtype], e)
        assert e < GRAD_BAR[dtype], (w, e)


@pytest.mark.parametrize("V", rr.CE_VS)
@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
def test_cross_entropy_on_every_path(dtype, V):
    """Three layouts x (2, 3), (5, 7), (1, 1), (6, 7) x temperatures 0.7, 1, 2, and an all-ignored batch: planted rows (a peak 20
    above the rest, the target at every group boundary, peak and target together and apart), an all-equal row, a +-3e4 row, a
    -inf, labels -100 / -1 / V / V + 5, NaN in every padding column.  Forward: scaled logits bit-equal to x * float32(1 / temp)
    rounded once, lse / row loss per row, exact count, loss sum against fp64 and against the kernel's own row losses; backward
    with count_dev, denom_host, dloss != 1 and dloss_dev: elementwise and max-normalised, exact zeros for rows without a target
    and for count = 0."""
    for case, temp in rr.ce_cases(dtype, V):
        _check_ce(case, temp, f"{NAME[dtype]} V={V} layout={case.layout} BxS={case.B}x{case.S} temp={temp} "
                              f"paths={rr.ce_paths(dtype, V, case.layout)}")


@pytest.mark.parametrize("B,S", rr.CE_LOOP_SHAPES)
@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
def test_cross_entropy_row_and_reduce_loops(dtype, B, S):
    for layout in rr.CE_LAYOUTS:
        case = rr.ce_case(dtype, 5, layout, B, S, seed=7 + B, plain=True)
        _check_ce(case, 0.7, f"{NAME[dtype]} V=5 layout={layout} BxS={B}x{S}")


@pytest.mark.parametrize("layout", ["b", "c"])
def test_cross_entropy_backward_maxima_sink(layout):
    """With the maxima sink armed the slot holds max |gradient| over the V valid columns (NaN padding does not count): the
    16-byte-group path (b) and the column loop (c)."""
    case = rr.ce_case(F32, 1041, layout, 5, 7, seed=5)
    T, V, ldl = case.T, case.V, case.ldl
    assert rr.ce_paths(F32, V, layout)[1] == {"b": "vec", "c": "scalar"}[layout]
    with ops.f32_matmul("split3"), ops.amax_reuse(everything=True) as cache:
        d = case.flat().to(DEV)
        lg, labels = case.rows(d), case.labels.to(DEV)
        lse, rl, ls, cnt = (torch.zeros(n, device=DEV) for n in (T, T, 1, 1))
        ops.ce_fwd(lg, ldl, labels, V, 0.7, IGN, lse, rl, ls, cnt)
        ops.ce_bwd(lg, ldl, labels, V, 0.7, IGN, lse, cnt, 0.0, 1.0)
        key = cache._key(lg.data_ptr(), (1, 0, T, V, ldl))
        assert key in cache.pending, "the producer did not open a slot"
        slot = cache.pending[key]
        pool = next(p for p in cache.pools if p.data_ptr() <= slot < p.data_ptr() + p.numel() * 4)
        off = (slot - pool.data_ptr()) // 4
        value = float(pool[off:off + ops.AMAX_WORDS].cpu().view(F32).max())
        assert value == float(lg[:, :V].abs().max()) and value > 0


def test_cross_entropy_refusals():
    T, V = 6, 8
    lg, labels = torch.zeros(T, 16, device=DEV), torch.zeros(2, 3, dtype=torch.int64, device=DEV)
    lse, rl, ls, cnt = (torch.zeros(n, device=DEV) for n in (T, T, 1, 1))
    for ldl, temp in ((V - 1, 0.7), (16, 0.0), (16, -1.0)):
        with pytest.raises(RuntimeError):
            ops.ce_fwd(lg, ldl, labels, V, temp, IGN, lse, rl, ls, cnt)
        with pytest.raises(RuntimeError):
            ops.ce_bwd(lg, ldl, labels, V, temp, IGN, lse, cnt, 0.0, 1.0)
    assert not bool(lg.any())


@pytest.mark.parametrize("n", [1, 2047, 2048, 2049, 3_000_000])
def test_check_labels_counts_what_the_kernels_skip(n):
    """bad_label += the number of labels outside [0, V) that are not the ignore index (n = 3e6: more than the capped grid
    covers in one pass)."""
    V = 11
    g = torch.Generator().manual_seed(n)
    labels = torch.randint(-3, V + 4, (n,), generator=g)
    labels[torch.randint(0, 5, (n,), generator=g) == 0] = IGN
    host = int(((labels != IGN) & ((labels < 0) | (labels >= V))).sum())
    bad = torch.full((1,), 7, dtype=torch.int32, device=DEV)
    ops.check_labels(labels.to(DEV), V, IGN, bad)
    assert int(bad) == 7 + host
    ops.check_labels(torch.full((n,), IGN, device=DEV), V, IGN, bad)    # the ignore index alone adds nothing
    assert int(bad) == 7 + host
    if n == 1:
        for lab, add in ((0, 0), (V - 1, 0), (-1, 1), (V, 1)):
            bad.fill_(0)
            ops.check_labels(torch.tensor([lab], device=DEV), V, IGN, bad)
            assert int(bad) == add


# ---------------------------------------------------------------------------------------------------------------------------
# 2. RMSNorm
# ---------------------------------------------------------------------------------------------------------------------------
RMS_HS = (4, 8, 100, 252, 256, 260, 512, 772, 1020, 1024)


def _rms_inputs(H, T):
    g = torch.Generator().manual_seed(1000 * H + T)
    x = torch.randn(T, H, generator=g) * 2
    if T >= 5:
        x[2] = 0                                     # rstd = 1 / sqrt(eps), y = 0, dx = rstd * w * dy
    w = 1 + 0.1 * torch.randn(H, generator=g)
    dy = torch.randn(T, H, generator=g).to(BF).float()          # bf16-representable: the bf16 entry point sees the same values
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    yr = orc.rmsnorm(xr, wr, 1e-6)
    yr.backward(dy.double())
    return g, x, w, dy, yr.detach(), xr.grad, wr.grad


@pytest.mark.parametrize("T", [1, 5, 333])
@pytest.mark.parametrize("H", RMS_HS)
def test_rmsnorm_on_both_instantiations(H, T):
    """Forward (fp32 and bf16 output) and backward (fp32 and bf16 dy) with the rows permuted and in place, ldy = H and H + 64 (NaN
    padding stays), 1 and 64 partial-sum workgroups (those without a row write zeros), dx accumulated and overwritten (over NaN),
    one all-zero input row (compared on its own: its dx is 1000 times the others')."""
    g, x, w, dy, yr, dx_ref, dw_ref = _rms_inputs(H, T)
    xd, wd = dev(x), dev(w)
    zero = torch.zeros(T, dtype=torch.bool)
    if T >= 5:
        zero[2] = True
    worst_f, worst_b = 0.0, 0.0
    for perm in (False, True):
        rows = torch.randperm(T, generator=g).int() if perm else None
        idx = rows.long() if perm else torch.arange(T)
        for ld in (H, H + 64):
            where = f"H={H} T={T} perm={perm} ld={ld}"
            y32 = torch.full((T, ld), NAN, device=DEV)
            y16 = torch.full((T, ld), NAN, dtype=BF, device=DEV)
            ops.rmsnorm_fwd(xd, wd, 1e-6, y32, ld, dev(rows))
            ops.rmsnorm_fwd(xd, wd, 1e-6, y16, ld, dev(rows))
            yc = y32.cpu()
            assert _same_bits(yc[:, H:], torch.full((T, ld - H), NAN)), where
            assert _same_bits(y16[:, H:], torch.full((T, ld - H), NAN, dtype=BF)), where
            got = yc[idx, :H]
            e = _rel(got, yr)
            worst_f = max(worst_f, e)
            assert e < 2e-6, (where, e)
            assert bool((got[zero] == 0).all()), where
            assert torch.equal(y16[:, :H], y32[:, :H].to(BF)), where
            dyb = torch.full((T, ld), NAN)
            dyb[idx, :H] = dy
            dy32, dy16 = dev(dyb), dev(dyb.to(BF))
            for npart in (1, 64):
                for acc in (True, False):
                    w2 = f"{where} n_partial={npart} accumulate={acc}"
                    dx0 = torch.randn(T, H, generator=g) if acc else torch.full((T, H), NAN)
                    dx32, dx16 = dev(dx0), dev(dx0)
                    pa32, pa16 = torch.full((npart, H), NAN, device=DEV), torch.full((npart, H), NAN, device=DEV)
                    ops.rmsnorm_bwd(xd, wd, dy32, ld, 1e-6, dx32, pa32, acc, dev(rows))
                    ops.rmsnorm_bwd(xd, wd, dy16, ld, 1e-6, dx16, pa16, acc, dev(rows))
                    assert torch.equal(dx16, dx32) and torch.equal(pa16, pa32), w2
                    dw = torch.full((H,), NAN, device=DEV)
                    ops.colsum_reduce(pa32, dw)
                    dxg = dx32.cpu().double() - (dx0.double() if acc else 0.0)
                    e1, e2 = _rel(dxg[~zero], dx_ref[~zero]), _rel(dw, dw_ref)
                    if bool(zero.any()):
                        e1 = max(e1, _rel(dxg[zero], dx_ref[zero]))
                    worst_b = max(worst_b, e1, e2)
                    assert e1 < 1e-5 and e2 < 1e-5, (w2, e1, e2)
                    empty = (T + 3) // 4                         # four waves = four rows per workgroup and pass
                    assert bool((pa32[empty:] == 0).all()), w2
                    assert _same_bits(dy32, dyb), w2
    _note("rmsnorm_fwd", worst_f)
    _note("rmsnorm_bwd", worst_b)


@pytest.mark.parametrize("H", [252, 772])
def test_rmsnorm_bwd_mask_out_equals_residual_dropout_bwd(H):
    """The fused branch gradient at a partly filled chunk of each instantiation: the same bits as rmsnorm_bwd followed by
    residual_dropout_bwd with the same seed, rows in place and scattered."""
    T = 333
    g, x, w, dy, _, _, _ = _rms_inputs(H, T)
    dx0 = torch.randn(T, H, generator=g)
    partial = torch.empty(64, H, device=DEV)
    for rows in (None, dev(torch.randperm(T, generator=g).int())):
        dxa, dxb = dev(dx0), dev(dx0)
        ma, mb = torch.zeros(T, H, device=DEV), torch.zeros(T, H, device=DEV)
        ops.rmsnorm_bwd(dev(x), dev(w), dev(dy), H, 1e-6, dxa, partial, True, None, mask_out=ma, mask_rows=rows, p=0.2, seed=123)
        ops.rmsnorm_bwd(dev(x), dev(w), dev(dy), H, 1e-6, dxb, partial, True, None)
        ops.residual_dropout_bwd(dxb, 0.2, 123, mb, rows)
        assert torch.equal(dxa, dxb) and torch.equal(ma, mb)
        assert 0.15 < float((ma == 0).float().mean()) < 0.25


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
def test_rmsnorm_fwd_row_grid_stride(dtype):
    H, T = 4, 32800                                  # more rows than the 32768 waves of the capped grid
    g = torch.Generator().manual_seed(4)
    x, w = torch.randn(T, H, generator=g) * 2, 1 + 0.1 * torch.randn(H, generator=g)
    rows = torch.randperm(T, generator=g).int()
    y = torch.full((T, H), NAN, dtype=dtype, device=DEV)
    ops.rmsnorm_fwd(dev(x), dev(w), 1e-6, y, H, dev(rows))
    y32 = y
    if dtype == BF:
        y32 = torch.full((T, H), NAN, device=DEV)
        ops.rmsnorm_fwd(dev(x), dev(w), 1e-6, y32, H, dev(rows))
        assert torch.equal(y, y32.to(BF))
    assert _rel(y32.cpu()[rows.long()], orc.rmsnorm(x.double(), w.double(), 1e-6)) < 2e-6


def test_rmsnorm_refusals():
    T = 3

    def run(H, ld, shift=0):
        xbuf = torch.zeros(T * H + 4, device=DEV)
        x = xbuf[shift:shift + T * H].view(T, H)
        w, y = torch.ones(H, device=DEV), torch.zeros(T, ld, device=DEV)
        with pytest.raises(RuntimeError):
            ops.rmsnorm_fwd(x, w, 1e-6, y, ld)
        with pytest.raises(RuntimeError):
            ops.rmsnorm_bwd(x, w, y, ld, 1e-6, torch.zeros(T, H, device=DEV), torch.zeros(1, H, device=DEV), False)
    run(6, 6)
    run(1028, 1028)
    run(8, 10)
    run(8, 8, shift=1)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. column sums
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", [1, 31, 32, 33, 100])
@pytest.mark.parametrize("rows", [1, 31, 32, 33, 127, 128, 129, 300])
def test_colsum_reduce_exact_on_integers(rows, cols):
    """Small integers: every partial sum is exact in fp32, so the sums equal the int64 column sums bit for bit - single and
    batched (three tables further apart than rows * cols, each with its own output), written and accumulated; nothing past
    `cols` is touched."""
    g = torch.Generator().manual_seed(100 * rows + cols)
    n, stride = 3, rows * cols + 40
    buf = torch.full((n * stride + 8,), 1e6)
    tabs = torch.randint(-8, 9, (n, rows, cols), generator=g)
    for i in range(n):
        buf[i * stride:i * stride + rows * cols] = tabs[i].reshape(-1).float()
    bufd = dev(buf)
    init = torch.randint(-8, 9, (n, cols), generator=g)
    for acc in (False, True):
        want = tabs.sum(1) + (init if acc else 0)
        outs = [dev(torch.cat([init[i].float(), torch.full((8,), 77.0)])) for i in range(n)]
        ops.colsum_reduce(bufd[:rows * cols].view(rows, cols), outs[0][:cols], accumulate=acc)
        assert torch.equal(outs[0].cpu()[:cols].long(), want[0]) and bool((outs[0][cols:] == 77.0).all()), acc
        outs = [dev(torch.cat([init[i].float(), torch.full((8,), 77.0)])) for i in range(n)]
        table = torch.tensor([o.data_ptr() for o in outs], dtype=torch.int64, device=DEV)
        ops.call("gamer_colsum_reduce_batched", ops.ptr(bufd), stride, rows, cols, n, ops.ptr(table), 1 if acc else 0, ops.stream_ptr())
        for i in range(n):
            assert torch.equal(outs[i].cpu()[:cols].long(), want[i]) and bool((outs[i][cols:] == 77.0).all()), (acc, i)
    assert torch.equal(bufd.cpu(), buf)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. sumsq + AdamW
# ---------------------------------------------------------------------------------------------------------------------------
SENT = 12345.0


def _padded(t):
    """the flat buffer as a caller holds it: n values, then the pad to a multiple of four and four more, all sentinel"""
    return dev(torch.cat([t, torch.full((4 + (-t.numel()) % 4,), SENT)]))


@pytest.mark.parametrize("n", rr.ADAMW_NS)
def test_sumsq_exact_on_integers_and_the_norm(n):
    """g in [-2, 2]: every sum of squares stays below 2^24, so the partials add up to the exact integer for every number of
    partials (also more partials than elements), and norm_out is sqrt of it times grad_scale to one fp32 ulp; the sentinel
    behind n would show in the sum if it were read."""
    g = torch.randint(-2, 3, (n,), generator=torch.Generator().manual_seed(n)).float()
    exact = int((g.long() ** 2).sum())
    Gd = _padded(g)
    P, M, V = (torch.zeros(n + 8, device=DEV) for _ in range(3))
    for npart in rr.ADAMW_NPARTIAL:
        partial = torch.full((npart,), NAN, device=DEV)
        ops.sumsq(Gd[:n], partial)
        assert float(partial.double().sum()) == float(exact), npart
        for gscale in (1.0, 0.125):
            norm = torch.full((1,), NAN, device=DEV)
            ops.adamw(P[:n], Gd[:n], M[:n], V[:n], n, 0.1, 0.9, 0.999, 1e-8, 0.5, 1, 1.0, gscale, partial, norm)
            ref = math.sqrt(exact) * gscale
            assert abs(float(norm) - ref) <= float(np.spacing(np.float32(ref))), (npart, gscale, float(norm), ref)


@pytest.mark.parametrize("n", rr.ADAMW_NS)
def test_adamw_update_elementwise(n):
    """p, m, v element by element against the fp64 clip_grad_norm_ + AdamW, with lr = 0.1 and weight_decay = 0.5 and |p| >= 1
    around n_decay (a boundary off by one is 5 % of that element): n_decay in {0, 1, 2, 5, n - 1, n}, step 1 / 2 / 1000, clipping
    active, inactive and off (max_norm = 0), grad_scale = 0.125, a zero gradient; 1 to 4096 partials.  Nothing behind n is
    written."""
    p0, m0, v0, gr, big = rr.adamw_inputs(n)
    Md0, Vd0, Gd = _padded(m0), _padded(v0), {}
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    for n_decay, (name, step, max_norm, gscale, gmag), npart in rr.adamw_cases(n):
        where = f"n={n} n_decay={n_decay} {name} n_partial={npart}"
        p, g = rr.adamw_p0(p0, big, n_decay), gr * gmag
        if gmag not in Gd:
            Gd[gmag] = _padded(g)
        Pd, Md, Vd = _padded(p), Md0.clone(), Vd0.clone()
        partial, norm = torch.full((npart,), NAN, device=DEV), torch.full((1,), NAN, device=DEV)
        ops.sumsq(Gd[gmag][:n], partial)
        ops.adamw(Pd[:n], Gd[gmag][:n], Md[:n], Vd[:n], n_decay, step=step, max_norm=max_norm, grad_scale=gscale, partial=partial,
                  norm_out=norm, **rr.ADAMW_HYPER)
        total, pr, mr, vr, sp, sm, sv = rr.adamw_ref(p, g, m0, v0, n_decay, step, max_norm, gscale, **rr.ADAMW_HYPER)
        assert abs(float(norm) - total) <= 1e-4 * total, (where, float(norm), total)
        for key, buf, ref, scale in (("p", Pd, pr, sp), ("m", Md, mr, sm), ("v", Vd, vr, sv)):
            got = buf.cpu()
            assert bool((got[n:] == SENT).all()), (where, key)
            e = rr.scaled_err(got[:n], ref, scale)
            worst[key] = max(worst[key], e)
            assert e < ADAMW_BAR[key], (where, key, e)
            assert _rel(got[:n], ref) < 1e-6, (where, key)
    for gmag, buf in Gd.items():
        assert torch.equal(buf.cpu()[:n], gr * gmag) and bool((buf[n:] == SENT).all())
    for key, e in worst.items():
        _note("adamw_" + key, e)
