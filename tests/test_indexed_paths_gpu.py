"""Every dispatch path of the indexed kernels of csrc/qknorm_rope.hip - per-head q/k RMSNorm + RoPE (+ behaviour bias) - and of
csrc/elementwise.hip - behaviour-table rows, embedding - against fp64 torch on the CPU, through the C ABI (gamer_amd.ops), at the smallest
shapes that reach each regime.  tests/helpers/qknorm_ref.py holds the cases, the references and a restatement of the host
dispatch; every case asserts with it that it runs the kernel, the iteration count and the reduce loop its name claims.

q/k norm + RoPE paths (rows per wave iteration: 4 fp32, 8 bf16; NH = nq + nkv (+ nkv cross); nqk = nq + nkv):
  forward   token-major (default): qknorm_rope_fwd_tok_kernel<float> / <bf16_t>, heads in groups of three - nqk = 2, 3, 4, 5, 8, 9
            fill the last group with 2, 3, 1, 2, 2, 3 heads; row-major (GAMER_QKNORM_ROW_MAJOR): qknorm_rope_fwd_row_kernel<float> /
            <bf16_t>, bit-identical outputs; grid capped at 32768 waves: T = 131075 (fp32) / 262150 (bf16) take two passes
  backward  self, token-major  qknorm_rope_bwd_tok_kernel<float> / <bf16_t>: n_waves = min(ceil(T / rows), 8192, scratch / 128)
              T = 301: one iteration per wave; scratch 3 * 128 (or 9 * 64 with (6, 3) heads: 4 waves), T = 101: 9 / 5 iterations,
              the last one partly filled; n_waves = 384 / 385 / 386 / 700: qknorm_partial_reduce_kernel's four-way loop (needs
              more than 384 items) off / on for one row group / on / on with a tail everywhere; T = 32773 / 65541: 4096 waves x 3
              iterations with ops' default scratch, 8192 waves x 2 iterations (the cap) with 8192 * 128 floats
            self, smallest accepted scratch (NH * 64 floats): still token-major, ONE wave; anything smaller is refused, so the
              head-major fallback of a self call is reached through the row-major switch only
            self, head-major (row-major switch): qknorm_rope_bwd_head_kernel<float, 8> / <bf16_t, 4> with cross = 0, waves_per_head =
              min(8192 / NH, ceil(T / rows), scratch / (NH * 64))
            cross, head-major  qknorm_rope_bwd_head_kernel<float, 8>, <bf16_t, 4> (nb1 <= 4), <bf16_t, 8> (nb1 5 .. 8): nb1 = 1, 4, 5, 8;
              (6, 3) heads at T = 2737 / 5467: 682 waves per head (the natural cap 8192 / 12) x 2 iterations, 4092 / 2046 / 682
              items per reduce column; scratch for waves_per_head = 1 and 2 at T = 101
Every case: T no multiple of the rows per wave; 8 sentinel rows behind q_rot, k_rot, dqkv (and 64 sentinel floats behind the
scratch); one all-zero q row and one all-zero k row (T >= 4; with one token and (1, 1) heads nothing else would be left);
weights 1 + 0.1 randn; a RoPE table of S + 5 rows; pos_ids absent, or random with repeats and rows >= S; cross: one bias row
without a token (nb1 > 1), whose gradient must keep its bits; dwq, dwk, dbias_* pre-filled (the kernels add to them); the v
columns of dqkv hold dV; every backward runs twice and must give the same bits.

Bars (`rel` = largest error over the largest reference magnitude, the existing tests' _rel).  Existing bars where a quantity has
one; four times the worst value of a plain fp32 torch restatement in the kernels' operation order against fp64 over every case
here where that is tighter (python tests/helpers/qknorm_ref.py prints this table):
  metric                  fp32 torch, worst         x4   existing        bar
  f32 dbias                       1.082e-06  4.330e-06  2.000e-05  4.330e-06
  f32 dbias_v                     1.097e-06  4.388e-06  2.000e-05  4.388e-06
  f32 dqkv                        2.065e-07  8.260e-07  2.000e-05  8.260e-07
  f32 dqkv_planted                2.196e-07  8.783e-07  2.000e-05  8.783e-07
  f32 dw                          1.666e-06  6.664e-06  2.000e-05  6.664e-06
  f32 fwd                         2.253e-07  9.011e-07  3.000e-06  9.011e-07
  f32 v                           5.850e-08  2.340e-07  3.000e-06  2.340e-07
  bf16 dbias                      1.969e-06  7.875e-06  1.000e-03  7.875e-06
  bf16 dbias_v                    6.361e-08  2.545e-07  1.000e-03  2.545e-07
  bf16 dqkv                       3.434e-03  1.374e-02  7.812e-03  7.812e-03
  bf16 dqkv_planted               3.136e-03  1.254e-02  7.812e-03  7.812e-03
  bf16 dw                         5.252e-04  2.101e-03  1.000e-03  1.000e-03
  bf16 fwd                        5.080e-03  2.032e-02  5.859e-03  5.859e-03
  bf16 v                          0.000e+00  0.000e+00  5.859e-03  0.000e+00
dqkv_planted: the cells of the all-zero rows of a self case, where rstd = 1000 - judged apart, they would set the scale of `rel`
for everything else.  v (and the q | k write-back of the fp32 cross forward) is one IEEE addition and one rounding per element:
the restatement has it exactly, and the tests ask for the bits.  Behaviour-table rows and embedding: 1e-5 under `rel`,
torch.equal where the operation is a copy.  The GPU's worst values go into the per-kernel report (test_ops_gpu._record, keys
indexed_*).
"""
import contextlib
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

import qknorm_ref as qr  # noqa: E402
from gamer_amd import ops  # noqa: E402

DEV = "cuda"
F32, BF = torch.float32, torch.bfloat16
NAME = qr.NAME
SENT = -7.0                                      # sentinel (a bf16 value)
GUARD = qr.GUARD

BAR = {F32: dict(dbias=4.330e-6, dbias_v=4.388e-6, dqkv=8.260e-7, dqkv_planted=8.783e-7, dw=6.664e-6, fwd=9.011e-7, v=2.340e-7),
       BF: dict(dbias=7.875e-6, dbias_v=2.545e-7, dqkv=7.812e-3, dqkv_planted=7.812e-3, dw=1.000e-3, fwd=5.859e-3, v=0.0)}
TABLE_BAR = 1e-5

WORST = {}


def _note(name, value):
    if value <= WORST.get(name, -1.0):
        return
    WORST[name] = value
    import test_ops_gpu
    test_ops_gpu._record("indexed_" + name, value)


def _bits(t):
    return t.view({4: torch.int32, 2: torch.int16, 8: torch.int64}[t.element_size()])


def _same_bits(a, b):
    return a.dtype == b.dtype and torch.equal(_bits(a.cpu().contiguous()), _bits(b.cpu().contiguous()))


def dev(t):
    return None if t is None else t.to(DEV).contiguous()


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    torch.manual_seed(0)


def _switch(row_major):
    return ops.env_switches(GAMER_QKNORM_ROW_MAJOR=1) if row_major else contextlib.nullcontext()


def _judge(c, m, where):
    for k, v in m.items():
        _note(f"qknorm_{k}_{NAME[c.dtype]}", v)
    bad = {k: (v, BAR[c.dtype][k]) for k, v in m.items() if not v <= BAR[c.dtype][k]}
    assert not bad, (where, bad)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. q/k RMSNorm + RoPE: the dispatch restatement and the tables above
# ---------------------------------------------------------------------------------------------------------------------------
def test_bar_table_is_the_one_written_here():
    for dt in (F32, BF):
        for k, v in BAR[dt].items():
            line = next(ln.split() for ln in __doc__.splitlines() if ln.split()[:2] == [NAME[dt], k])
            worst, x4, existing, bar = map(float, line[2:])
            assert existing == pytest.approx(qr.EXISTING[dt][k], rel=1e-3) and bar == v == pytest.approx(qr.bar(dt, k, worst), rel=2e-3)


def test_every_case_is_in_the_regime_its_name_claims():
    kinds = {}
    for c in qr.BWD_CASES:
        d = c.check_regime()
        kinds.setdefault(d["kernel"], []).append(d)
    # all five backward kernels, each with one and with several iterations per wave
    assert set(kinds) == {"qknorm_rope_bwd_tok_kernel<float>", "qknorm_rope_bwd_tok_kernel<bf16_t>", "qknorm_rope_bwd_head_kernel<float, 8>",
                          "qknorm_rope_bwd_head_kernel<bf16_t, 4>", "qknorm_rope_bwd_head_kernel<bf16_t, 8>"}
    for name, ds in kinds.items():
        assert min(d["iters"] for d in ds) == 1 and max(d["iters"] for d in ds) >= 2, name
        assert any(qr.reduce_four_way(max(d["items"].values())) for d in ds), name
    for dt, rows in ((F32, 4), (BF, 8)):
        assert [qr.bwd_dispatch(dt, False, 0, T, 2, 1)["waves"] for T, _ in qr.TOK_REDUCE_T[dt]] == [384, 385, 386, 700]
        assert [qr.reduce_four_way(n) for n in (384, 385)] == [False, True]
        d = qr.fwd_dispatch(dt, False, qr.GRID_CAP_T[dt], 1, 1)
        assert d["waves"] == 32768 and d["iters"] == 2 and qr.GRID_CAP_T[dt] % rows != 0
        assert qr.fwd_dispatch(dt, False, 32768 * rows, 1, 1)["iters"] == 1
        for T in qr.FWD_TS + (101, qr.TOK_CAP_T[dt], qr.HM_CAP_T[dt]):
            assert T % rows != 0
        # a self call cannot reach the head-major kernel through its scratch: below one token-major row it is refused
        assert qr.bwd_dispatch(dt, False, 0, 101, 1, 1, scratch=127) is None
        assert qr.bwd_dispatch(dt, False, 0, 101, 1, 1, scratch=128)["kernel"] == qr.TOK[dt]
    assert [qr.emb_chunk(T) for T in EMB_BWD_TS] == [128, 128, 128, 256, 512, 1024]


# ---------------------------------------------------------------------------------------------------------------------------
# 2. q/k RMSNorm + RoPE forward
# ---------------------------------------------------------------------------------------------------------------------------
def _cross_kw(c, inp, with_v):
    if not c.cross:
        return {}
    kw = dict(bias_q=dev(inp["bq"]), bias_k=dev(inp["bk"]), act_idx=dev(inp["act"]))
    if with_v:
        kw["bias_v"] = dev(inp["bv"])
    return kw


def _run_fwd(c, inp, row_major=False):
    T, nq, nkv, dt = c.T, c.nq, c.nkv, c.dtype
    qkv = dev(inp["qkv"].to(dt))
    q_rot = torch.full((T + GUARD, nq * 64), SENT, dtype=dt, device=DEV)
    k_rot = torch.full((T + GUARD, nkv * 64), SENT, dtype=dt, device=DEV)
    with _switch(row_major):
        ops.qknorm_rope_fwd(qkv, c.S, nq, nkv, dev(inp["wq"]), dev(inp["wk"]), qr.EPS, dev(inp["cos"]), dev(inp["sin"]), q_rot, k_rot,
                            pos_ids=dev(inp["pos"]), **_cross_kw(c, inp, True))
    return dict(q_rot=q_rot.cpu(), k_rot=k_rot.cpu(), qkv=qkv.cpu())


def _check_fwd_layout(c, inp, out):
    """sentinel rows, finite outputs (the all-zero rows included), and the write-back rule of q | k | v bit for bit: self -
    unchanged; cross fp32 - all three biased; cross bf16 - q | k unchanged, v + bias_v rounded"""
    T = c.T
    for k in ("q_rot", "k_rot"):
        assert bool((out[k][T:] == SENT).all()), (c.id, k, "guard rows")
        assert bool(torch.isfinite(out[k][:T].float()).all()), (c.id, k)
    assert _same_bits(out["qkv"], qr.writeback(c, inp).to(c.dtype)), (c.id, "q|k|v after the forward")


@pytest.mark.parametrize("nq,nkv", qr.HEADS)
@pytest.mark.parametrize("cross", [False, True], ids=["self", "cross"])
@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
def test_qknorm_rope_fwd_every_head_count(dtype, cross, nq, nkv):
    for c in qr.fwd_cases(dtype, cross, nq, nkv):
        d = qr.fwd_dispatch(dtype, cross, c.T, nq, nkv)
        assert d["kernel"].startswith("qknorm_rope_fwd_tok_kernel<") and d["iters"] == 1, (c.id, d)
        inp = qr.make_inputs(c, backward=False)
        out = _run_fwd(c, inp)
        _check_fwd_layout(c, inp, out)
        got = dict(q=out["q_rot"][:c.T], k=out["k_rot"][:c.T], v=out["qkv"][:, (nq + nkv) * 64:])
        _judge(c, qr.metrics(c, got, qr.ref64_fwd(c, inp), backward=False), c.id)


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
def test_qknorm_rope_fwd_grid_stride(dtype):
    """more tokens than the capped grid's 32768 waves take in one pass, with a partly filled last wave: every row checked"""
    c = qr.Case("fwd_grid_cap", dtype, False, 1, 1, 0, qr.GRID_CAP_T[dtype], False)
    assert qr.fwd_dispatch(dtype, False, c.T, 1, 1) == dict(kernel=qr.fwd_dispatch(dtype, False, 5, 1, 1)["kernel"], waves=32768, iters=2)
    inp = qr.make_inputs(c, backward=False)
    out = _run_fwd(c, inp)
    _check_fwd_layout(c, inp, out)
    worst = {}
    for lo in range(0, c.T, qr.CHUNK):
        hi = min(c.T, lo + qr.CHUNK)
        m = qr.metrics(c, dict(q=out["q_rot"][lo:hi], k=out["k_rot"][lo:hi]), qr.ref64_fwd(c, inp, lo, hi), backward=False)
        worst = {k: max(v, worst.get(k, 0.0)) for k, v in m.items()}
    _judge(c, worst, c.id)


@pytest.mark.parametrize("pos", [False, True], ids=["seq", "pos"])
@pytest.mark.parametrize("cross", [False, True], ids=["self", "cross"])
@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
def test_qknorm_rope_fwd_row_major_has_the_same_bits(dtype, cross, pos):
    """the kernel header's claim: the row-major forms (GAMER_QKNORM_ROW_MAJOR) give bit-identical outputs"""
    for (nq, nkv), nb1, T in (((6, 3), 5, 301), ((2, 1), 4, 5), ((4, 1), 8, 301)):
        c = qr.Case("fwd_row_major", dtype, cross, nq, nkv, nb1, T, pos)
        a, b = qr.fwd_dispatch(dtype, cross, T, nq, nkv), qr.fwd_dispatch(dtype, cross, T, nq, nkv, row_major=True)
        assert a["kernel"] != b["kernel"] and "_tok_" not in b["kernel"], (a, b)
        inp = qr.make_inputs(c, backward=False)
        tok, row = _run_fwd(c, inp), _run_fwd(c, inp, row_major=True)
        _check_fwd_layout(c, inp, row)
        for k in ("q_rot", "k_rot", "qkv"):
            assert _same_bits(tok[k], row[k]), (c.id, k)
        got = dict(q=row["q_rot"][:T], k=row["k_rot"][:T], v=row["qkv"][:, (nq + nkv) * 64:])
        _judge(c, qr.metrics(c, got, qr.ref64_fwd(c, inp), backward=False), c.id)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. q/k RMSNorm + RoPE backward
# ---------------------------------------------------------------------------------------------------------------------------
GRADS = ("dwq", "dwk", "dbq", "dbk", "dbv")


def _run_bwd(c, inp, row_major=None):
    """one backward call: dqkv with sentinel rows (and sentinels where the kernel must write), dV in its v columns, the weight and
    bias gradients pre-filled; the input q | k | v is what the forward leaves (fp32 cross: biased)"""
    T, nq, nkv, dt = c.T, c.nq, c.nkv, c.dtype
    nqk = (nq + nkv) * 64
    row_major = c.row_major if row_major is None else row_major
    dqkv = torch.full((T + GUARD, nqk + nkv * 64), SENT, dtype=dt, device=DEV)
    dqkv[:T, nqk:] = dev(inp["dv"].to(dt))
    acc = {k: dev(v.clone()) for k, v in inp["base"].items()}
    n = c.scratch if c.scratch is not None else qr.default_scratch(c.nb1)
    scratch = torch.full((n + 64,), SENT, device=DEV)
    kw = _cross_kw(c, inp, False)
    if c.cross:
        kw.update(nb1=c.nb1, dbias_q=acc["dbq"], dbias_k=acc["dbk"], dbias_v=acc["dbv"])
    with _switch(row_major):
        ops.qknorm_rope_bwd(dev(qr.writeback(c, inp).to(dt)), dev(inp["dq"].to(dt)), dev(inp["dk"].to(dt)), c.S, nq, nkv, dev(inp["wq"]),
                            dev(inp["wk"]), qr.EPS, dev(inp["cos"]), dev(inp["sin"]), dqkv, acc["dwq"], acc["dwk"], pos_ids=dev(inp["pos"]),
                            partial=scratch[:n], **kw)
    assert bool((scratch[n:] == SENT).all()), (c.id, "wrote past the scratch")
    out = {k: v.cpu() for k, v in acc.items()}
    out["dqkv"] = dqkv.cpu()
    return out


def _check_bwd(c, inp, out, ref, where):
    T, nqk = c.T, (c.nq + c.nkv) * 64
    assert bool((out["dqkv"][T:] == SENT).all()), (where, "guard rows")
    assert _same_bits(out["dqkv"][:T, nqk:], inp["dv"].to(c.dtype)), (where, "the v columns of dqkv hold dV and stay")
    assert bool(torch.isfinite(out["dqkv"][:T].float()).all()), where
    got = dict(q=ref["q"], k=ref["k"], v=ref["v"], dqkv=out["dqkv"][:T, :nqk])
    for k, base in inp["base"].items():
        got[k] = out[k].double() - base.double()              # the kernels add to what the buffers hold
        u = qr.unused_row(c.nb1)
        if k.startswith("db") and u >= 0:
            assert _same_bits(out[k][u], base[u]), (where, k, "a bias row without a token keeps its bits")
    m = qr.metrics(c, got, ref)
    del m["fwd"]
    m.pop("v", None)
    _judge(c, m, where)


@pytest.mark.parametrize("c", qr.BWD_CASES, ids=[c.id for c in qr.BWD_CASES])
def test_qknorm_rope_bwd_every_path(c):
    c.check_regime()
    inp = qr.make_inputs(c)
    ref = qr.ref64(c, inp)
    first, second = _run_bwd(c, inp), _run_bwd(c, inp)
    for k in first:
        assert _same_bits(first[k], second[k]), (c.id, k, "two calls, different bits")
    _check_bwd(c, inp, first, ref, c.id)


@pytest.mark.parametrize("pos", [False, True], ids=["seq", "pos"])
@pytest.mark.parametrize("nq,nkv", [(2, 1), (4, 1), (6, 3)])
@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
def test_qknorm_rope_bwd_row_major_against_token_major(dtype, nq, nkv, pos):
    """self: the head-major kernels (row-major switch) write the same dqkv bits as the token-major ones; dwq / dwk are summed in
    another order and meet the bar each"""
    c = qr.Case("bwd_row_major", dtype, False, nq, nkv, 0, 301, pos)
    assert qr.bwd_dispatch(dtype, False, 0, c.T, nq, nkv)["kernel"] == qr.TOK[dtype]
    assert qr.bwd_dispatch(dtype, False, 0, c.T, nq, nkv, row_major=True)["kernel"] == qr.head_major(dtype, False, 0)
    inp = qr.make_inputs(c)
    ref = qr.ref64(c, inp)
    tok, row = _run_bwd(c, inp, row_major=False), _run_bwd(c, inp, row_major=True)
    assert _same_bits(tok["dqkv"], row["dqkv"]), c.id
    _check_bwd(c, inp, tok, ref, c.id + " token-major")
    _check_bwd(c, inp, row, ref, c.id + " row-major")


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
def test_self_scratch_below_one_wave_is_refused(dtype):
    """127 floats hold neither a token-major row (128) nor a head-major one (NH * 64 = 128): an error, not a silent fallback"""
    c = qr.Case("refused", dtype, False, 1, 1, 0, 101, False, scratch=127)
    assert c.dispatch() is None
    inp = qr.make_inputs(c)
    with pytest.raises(RuntimeError):
        _run_bwd(c, inp)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. behaviour-table rows
# ---------------------------------------------------------------------------------------------------------------------------
def _rowtable_T_big(E):
    """a T above the 1024-workgroup cap of rowtable_bwd (256 / (E / 4) token rows per workgroup)"""
    return 40000 if E >= 64 else 1024 * (256 // (E // 4)) + 56


def _rowtable_inputs(E, T, rows, ld):
    g = torch.Generator().manual_seed(1000 * E + 10 * T + rows)
    used = torch.tensor([r for r in range(rows) if r != qr.unused_row(rows)])
    idx = used[torch.randint(0, len(used), (T,), generator=g)].int()
    dy = torch.randn(T, ld, generator=g).to(BF).float()
    perm = torch.randperm(T, generator=g).int()
    return idx, dy, perm, torch.randn(rows, E, generator=g), 0.5 * torch.randn(rows, E, generator=g)


@pytest.mark.parametrize("E", [4, 64, 96, 1024])
@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
def test_rowtable_every_width(dtype, E):
    """E = 96: 256 % (E / 4) != 0, sixteen idle threads per workgroup; E = 1024: one token row per workgroup.  Forward: a copy into
    columns [col0, col0 + E) of permuted rows, everything else untouched.  Backward: atomic and ordered form against fp64, += onto
    what dtable holds, a table row without a token keeps its bits; ordered: same bits twice, also with one workgroup only."""
    col0 = 8
    ld = col0 + E + 12
    for T in (1, 501, _rowtable_T_big(E)):
        for rows in ((1, 4, 8) if T <= 501 else (8,)):
            where = f"E={E} T={T} rows={rows} {NAME[dtype]}"
            idx, dy, perm, table, base = _rowtable_inputs(E, T, rows, ld)
            # forward
            y = torch.full((T + GUARD, ld), SENT, dtype=dtype, device=DEV)
            ops.rowtable_fwd(dev(table), dev(idx), y, ld, col0, dev(perm))
            want = torch.full((T + GUARD, ld), SENT, dtype=dtype)
            want[perm.long(), col0:col0 + E] = table[idx.long()].to(dtype)
            assert _same_bits(y, want), where
            # backward: dtable[idx[t]] += dy[dy_rows[t]][col0 : col0 + E]
            ref = base.double().index_put((idx.long(),), dy[perm.long(), col0:col0 + E].double(), accumulate=True)
            blocks = min(1024, qr.cdiv(T, 256 // (E // 4)))
            assert (blocks == 1024) == (T > 501), where
            d_dy, d_idx, d_perm, u = dev(dy.to(dtype)), dev(idx), dev(perm), qr.unused_row(rows)
            for form, scratch in (("atomic", None), ("ordered", blocks * rows * E), ("ordered_one_workgroup", rows * E)):
                outs = []
                for rep in range(1 if scratch is None else 2):
                    dt_ = dev(base.clone())
                    part = None if scratch is None else torch.full((scratch + 64,), SENT, device=DEV)
                    ops.rowtable_bwd(d_dy, ld, col0, d_idx, dt_, d_perm, partial=None if part is None else part[:scratch])
                    assert part is None or bool((part[scratch:] == SENT).all()), (where, form, "wrote past the scratch")
                    outs.append(dt_.cpu())
                e = qr.rel(outs[0], ref)
                _note(f"rowtable_bwd_{NAME[dtype]}", e)
                assert e < TABLE_BAR, (where, form, e)
                if u >= 0:
                    assert _same_bits(outs[0][u], base[u]), (where, form, "a table row without a token keeps its bits")
                if len(outs) == 2:
                    assert _same_bits(outs[0], outs[1]), (where, form, "two calls, different bits")


# ---------------------------------------------------------------------------------------------------------------------------
# 5. embedding
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,T", [(4, 1), (4, 32800), (128, 300), (128, 32800), (1028, 300)])
def test_embedding_fwd_widths_and_token_stride(H, T):
    """H / 4 = 257: a second trip of the lane loop for one lane; T = 32800: more tokens than the capped grid has waves (32768), so
    the token loop strides; ids out of range on either side give zero rows"""
    V = 61
    assert (qr.cdiv(T, 4) > qr.FWD_MAX_BLOCKS) == (T > 32768)
    g = torch.Generator().manual_seed(H + T)
    W = torch.randn(V, H, generator=g)
    ids = torch.randint(0, V, (T,), generator=g)
    bad = torch.zeros(T, dtype=torch.bool)
    if T > 1:
        ids[1], ids[T // 2], ids[T - 1] = -1, V, V + 7
        ids[T // 3] = -2 ** 40
        bad[[1, T // 2, T - 1, T // 3]] = True
    x = torch.full((T + GUARD, H), SENT, device=DEV)
    ops.embedding_fwd(dev(ids), dev(W), x)
    want = torch.full((T + GUARD, H), SENT)
    want[:T] = torch.where(bad[:, None], torch.zeros(1), W[ids.clamp(0, V - 1)])
    assert _same_bits(x, want), (H, T)


EMB_BWD_TS = (1, 129, 70000, 140000, 300000, 524300)           # chunks of 128, 128, 128, 256, 512, 1024 tokens per workgroup


@pytest.mark.parametrize("H,T", [(8, T) for T in EMB_BWD_TS] + [(128, 129), (128, 70000), (1024, 129), (1024, 2000)])
def test_embedding_bwd_chunk_ladder_and_cache(H, T):
    """gamer_embedding_bwd, the atomic form: every chunk size of the ladder; the first 64 tokens of most chunks hold more than
    EMB_CACHE = 8 distinct ids (so some rows of a chunk go through the LDS cache and others straight to global atomics); chunk 1
    holds only padding and out-of-range ids; the hot id opens the even chunks (cached there) and shows up in the odd ones only
    behind their first 64 tokens (not cached there); H = 1024 is the limit"""
    V, pad, hot = 300, 4, 17
    chunk = qr.emb_chunk(T)
    g = torch.Generator().manual_seed(H + T)
    ids = torch.randint(0, V, (T,), generator=g)
    ids[ids == hot] = hot + 1
    for c0 in range(0, T, chunk):
        if (c0 // chunk) % 2 == 0:
            ids[c0] = hot
        elif c0 + 70 < T:
            ids[c0 + 70] = hot
            assert len(set(ids[c0:c0 + 64].tolist()) - {pad}) > 8
    if T > 2 * chunk:
        ids[chunk:2 * chunk] = torch.tensor([pad, -1, V, V + 3])[torch.randint(0, 4, (chunk,), generator=g)]
    if T > 8:
        ids[5], ids[6], ids[7] = pad, -3, V
    dx = torch.randn(T, H, generator=g)
    base = torch.randn(V, H, generator=g)
    dW = dev(base.clone())
    ops.embedding_bwd(dev(ids), dev(dx), pad, dW)
    ok = (ids != pad) & (ids >= 0) & (ids < V)
    ref = base.double().index_put((ids[ok],), dx[ok].double(), accumulate=True)
    e = qr.rel(dW, ref)
    _note("embedding_bwd", e)
    assert e < TABLE_BAR, (H, T, e)
    untouched = torch.ones(V, dtype=torch.bool)
    untouched[ids[ok]] = False
    untouched[pad] = True
    assert _same_bits(dW.cpu()[untouched], base[untouched]), (H, T, "rows without a token, the padding row")
