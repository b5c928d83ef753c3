"""CPU side of tests/test_indexed_paths_gpu.py: the case lists of the q/k RMSNorm + RoPE kernels, their inputs, an fp64
reference (forward and backward, self and cross, pos_ids, the bf16 arithmetic of the kernel header), a plain fp32 torch
restatement of the same formulas in the kernels' operation order, and a restatement of the host dispatch of
gamer_qknorm_rope_fwd / _bwd and gamer_embedding_bwd.

Nothing here touches the GPU or imports gamer_amd.  `python tests/helpers/qknorm_ref.py` runs the fp32 restatement over every
listed case against the fp64 reference and prints the worst value of every metric with the bar that follows from it: the table
in the docstring of the test module.
"""
import zlib

import torch

F32, F64, BF = torch.float32, torch.float64, torch.bfloat16
NAME = {F32: "f32", BF: "bf16"}
EPS = 1e-6
HEADS = ((1, 1), (2, 1), (2, 2), (4, 1), (6, 2), (6, 3))         # nqk = 2, 3, 4, 5, 8, 9: every filling of the three-head groups
NB1S = (1, 4, 5, 8)
GUARD = 8                                                        # sentinel rows behind every output buffer

# ---------------------------------------------------------------------------------------------------------------------------
# host dispatch, restated (csrc/common.h: grid_for_waves; csrc/qknorm_rope.hip: qknorm_rope_fwd_impl, qknorm_rope_bwd_impl;
# csrc/elementwise.hip: gamer_embedding_bwd)
# ---------------------------------------------------------------------------------------------------------------------------
EW_WAVES = 4                     # waves per workgroup
FWD_MAX_BLOCKS = 8192            # grid_for_waves' cap: 32768 waves
BWD_MAX_WAVES = 8192
QKR_RG = 128                     # row groups of qknorm_partial_reduce_kernel: its four-way loop needs more than 3 * QKR_RG items
TOK = {F32: "qknorm_rope_bwd_tok_kernel<float>", BF: "qknorm_rope_bwd_tok_kernel<bf16_t>"}


def rpw(dtype):
    """token rows per wave iteration"""
    return 4 if dtype == F32 else 8


def cdiv(a, b):
    return (a + b - 1) // b


def n_heads(cross, nq, nkv):
    return nq + nkv + (nkv if cross else 0)


def default_scratch(nb1=0):
    return 8192 * (1 + nb1) * 64


def min_scratch(cross, nb1, nq, nkv):
    """the smallest `partial` the backward accepts: one wave per head"""
    return n_heads(cross, nq, nkv) * (1 + (nb1 if cross else 0)) * 64


def head_major(dtype, cross, nb1):
    if dtype == F32:
        return "qknorm_rope_bwd_head_kernel<float, 8>"
    return "qknorm_rope_bwd_head_kernel<bf16_t, 4>" if (not cross or nb1 <= 4) else "qknorm_rope_bwd_head_kernel<bf16_t, 8>"


def fwd_dispatch(dtype, cross, T, nq, nkv, row_major=False):
    r, NH = rpw(dtype), n_heads(cross, nq, nkv)
    rows = T * NH if row_major else T                    # row-major: one group of lanes per (token, head); else per token
    waves = EW_WAVES * min(max(cdiv(cdiv(rows, r), EW_WAVES), 1), FWD_MAX_BLOCKS)
    kernel = f"qknorm_rope_fwd_{'row' if row_major else 'tok'}_kernel<{'float' if dtype == F32 else 'bf16_t'}>"
    return dict(kernel=kernel, waves=waves, iters=cdiv(rows, waves * r))


def bwd_dispatch(dtype, cross, nb1, T, nq, nkv, scratch=None, row_major=False):
    """kernel name, its wave count (n_waves of the token-major kernels, waves_per_head of the head-major ones), the iterations
    of the longest-running wave, and the (row, head) items qknorm_partial_reduce_kernel adds up per output column; None where
    the entry point refuses the scratch"""
    if scratch is None:
        scratch = default_scratch(nb1 if cross else 0)
    r, NH, SL = rpw(dtype), n_heads(cross, nq, nkv), 1 + (nb1 if cross else 0)
    wph = min(BWD_MAX_WAVES // NH, cdiv(T, r), scratch // (NH * SL * 64))
    if wph < 1:
        return None
    n_tok = min(cdiv(T, r), BWD_MAX_WAVES, scratch // 128)
    if not cross and not row_major and n_tok >= 1:
        return dict(kernel=TOK[dtype], waves=n_tok, iters=cdiv(T, n_tok * r), items=dict(dwq=n_tok, dwk=n_tok))
    items = dict(dwq=wph * nq, dwk=wph * nkv)
    if cross:
        items["dbias"] = wph
    return dict(kernel=head_major(dtype, cross, nb1), waves=wph, iters=cdiv(T, wph * r), items=items)


def reduce_four_way(items):
    """does some row group of the reduce kernel run its unrolled loop?"""
    return items > 3 * QKR_RG


def emb_chunk(T):
    """tokens per workgroup of embedding_bwd_kernel"""
    chunk = 1024
    while chunk > 128 and cdiv(T, chunk) < 512:
        chunk >>= 1
    return chunk


# ---------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------
def seq_len(T, limit=512):
    """S with T % S == 0 (the entry points require it): the largest divisor of T up to `limit`"""
    return max(s for s in range(1, min(T, limit) + 1) if T % s == 0)


class Case:
    def __init__(self, kind, dtype, cross, nq, nkv, nb1, T, pos, scratch=None, row_major=False, **expect):
        self.kind, self.dtype, self.cross, self.nq, self.nkv, self.nb1 = kind, dtype, cross, nq, nkv, (nb1 if cross else 0)
        self.T, self.S, self.pos, self.scratch, self.row_major, self.expect = T, seq_len(T), pos, scratch, row_major, expect
        assert T < 5 or self.S >= 5, (T, self.S)        # (a T whose only small divisors are 1 .. 4 would hardly move t % S)
        self.id = (f"{kind}-{NAME[dtype]}-{'cross' if cross else 'self'}-h{nq}x{nkv}-nb{self.nb1}-T{T}-{'pos' if pos else 'seq'}"
                   f"-s{'dflt' if scratch is None else scratch}{'-rowmajor' if row_major else ''}")

    def dispatch(self):
        return bwd_dispatch(self.dtype, self.cross, self.nb1, self.T, self.nq, self.nkv, self.scratch, self.row_major)

    def check_regime(self):
        """the case is in the regime its name claims - or it fails, instead of passing on another path"""
        d, e = self.dispatch(), self.expect
        assert d is not None, self.id
        assert d["kernel"] == e["kernel"], (self.id, d)
        if "waves" in e:
            assert d["waves"] == e["waves"], (self.id, d)
        if "iters" in e:
            assert d["iters"] == e["iters"], (self.id, d)
        if "iters_min" in e:
            assert d["iters"] >= e["iters_min"] >= 2, (self.id, d)
        if "four_way" in e:
            assert all(reduce_four_way(n) == e["four_way"] for n in d["items"].values()), (self.id, d)
        if "items" in e:
            assert all(n == e["items"] for n in d["items"].values()), (self.id, d)
        return d


FWD_TS = (1, 5, 301)


def fwd_cases(dtype, cross, nq, nkv):
    for T in FWD_TS:
        for pos in (False, True):
            for nb1 in (NB1S if cross else (0,)):
                yield Case("fwd", dtype, cross, nq, nkv, nb1, T, pos)


# forward only, (1, 1) heads, self: more tokens than the 32768 waves of the capped grid take in one pass, with a tail
GRID_CAP_T = {F32: 131075, BF: 262150}                   # 5^2 7^2 107 and twice that: S = 175
# n_waves = 384 / 385 / 386 around the reduce kernel's four-way loop (it + 384 < n_waves), and 700 (loop plus tail everywhere)
TOK_REDUCE_T = {F32: ((1535, 384), (1537, 385), (1541, 386), (2799, 700)), BF: ((3069, 384), (3075, 385), (3085, 386), (5595, 700))}
TOK_CAP_T = {F32: 32773, BF: 65541}                      # just over 8192 waves x rows per wave
HM_CAP_T = {F32: 2737, BF: 5467}                         # (6, 3) cross: just over rows per wave x (8192 / 12 = 682) waves per head


def bwd_cases():
    out = []
    for dt in (F32, BF):
        tok = TOK[dt]
        hms = head_major(dt, False, 0)
        # --- token-major self kernels
        for nq, nkv in HEADS:
            for pos in (False, True):
                out.append(Case("tok_default", dt, False, nq, nkv, 0, 301, pos, kernel=tok, iters=1, four_way=False))
        out.append(Case("tok_3waves", dt, False, 2, 1, 0, 101, True, scratch=3 * 128, kernel=tok, waves=3, iters_min=2))
        out.append(Case("tok_3waves", dt, False, 4, 1, 0, 101, False, scratch=3 * 128, kernel=tok, waves=3, iters_min=2))
        # ((6, 3) heads: the entry point wants NH * 64 = 576 floats, which is four token-major waves)
        out.append(Case("tok_4waves", dt, False, 6, 3, 0, 101, False, scratch=9 * 64, kernel=tok, waves=4, iters_min=2))
        for T, nw in TOK_REDUCE_T[dt]:
            out.append(Case("tok_reduce", dt, False, 2, 1, 0, T, nw % 2 == 0, kernel=tok, waves=nw, iters=1, four_way=nw > 384))
        # (ops' default scratch for a self call, 8192 * 64 floats, holds 4096 token-major rows of 128: the 8192-wave cap itself
        # needs twice that)
        out.append(Case("tok_cap", dt, False, 1, 1, 0, TOK_CAP_T[dt], True, kernel=tok, waves=4096, iters=3, four_way=True))
        out.append(Case("tok_cap", dt, False, 1, 1, 0, TOK_CAP_T[dt], True, scratch=8192 * 128, kernel=tok, waves=8192, iters=2,
                        four_way=True))
        # --- the smallest scratch the entry point accepts, NH * 64 floats: still one token-major wave (a head-major fallback of the
        #     self call would need fewer than 128 floats, which the argument check refuses: see test_self_scratch_below_one_wave_is_refused)
        out.append(Case("tok_min_scratch", dt, False, 1, 1, 0, 101, True, scratch=128, kernel=tok, waves=1, iters_min=2))
        out.append(Case("tok_min_scratch", dt, False, 2, 1, 0, 101, False, scratch=192, kernel=tok, waves=1, iters_min=2))
        # --- self on the head-major kernels: the row-major switch
        out.append(Case("hm_self", dt, False, 2, 1, 0, 301, True, row_major=True, kernel=hms, iters=1))
        out.append(Case("hm_self", dt, False, 6, 3, 0, 101, False, scratch=2 * 9 * 64, row_major=True, kernel=hms, waves=2, iters_min=2))
        out.append(Case("hm_self", dt, False, 1, 1, 0, 101, True, scratch=128, row_major=True, kernel=hms, waves=1, iters_min=2))
        # --- head-major cross kernels
        for nb1 in NB1S:
            for pos in (False, True):
                out.append(Case("hm_cross", dt, True, 2, 1, nb1, 301, pos, kernel=head_major(dt, True, nb1), iters=1))
        for nb1 in (4, 5):
            out.append(Case("hm_cross_cap", dt, True, 6, 3, nb1, HM_CAP_T[dt], nb1 == 5, kernel=head_major(dt, True, nb1), waves=682,
                            iters=2, four_way=True))
        for wph in (1, 2):
            for (nq, nkv), nb1 in (((2, 1), 4), ((6, 3), 5)):
                out.append(Case("hm_cross_scratch", dt, True, nq, nkv, nb1, 101, wph == 1, scratch=wph * min_scratch(True, nb1, nq, nkv),
                                kernel=head_major(dt, True, nb1), waves=wph, iters_min=2))
    return out


BWD_CASES = bwd_cases()


# ---------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------
def rope_tables(P, theta=1e6):
    inv_freq = 1.0 / (theta ** (torch.arange(0, 64, 2, dtype=torch.int64).to(F32) / 64))
    freqs = torch.arange(P, dtype=F32)[:, None] * inv_freq[None, :]
    emb = torch.cat((freqs, freqs), dim=-1)
    return emb.cos(), emb.sin()


def unused_row(nb1):
    """the bias row no token uses (nb1 = 1 has none to spare)"""
    return nb1 - 2 if nb1 > 1 else -1


def planted(c):
    """(token, head) of the all-zero q row and of the all-zero k row (head index among q|k heads); T < 4 plants none - with a
    single token and (1, 1) heads nothing else would be left to check"""
    return ((c.T // 2, c.nq - 1), (c.T // 2 + 1, c.nq)) if c.T >= 4 else ()


def make_inputs(c, backward=True):
    """Values of the activation type held as fp32; weights 1 + 0.1 randn; a RoPE table of S + 5 rows; pos_ids (when the case
    has them) repeat positions and use the rows >= S; act_idx leaves one bias row without a token."""
    g = torch.Generator().manual_seed(zlib.crc32(c.id.encode()))
    T, nq, nkv, nb1, S = c.T, c.nq, c.nkv, c.nb1, c.S
    rnd = lambda *s: torch.randn(*s, generator=g).to(c.dtype).float()
    inp = dict(qkv=rnd(T, (nq + 2 * nkv) * 64), wq=1 + 0.1 * torch.randn(64, generator=g), wk=1 + 0.1 * torch.randn(64, generator=g))
    for t, h in planted(c):
        inp["qkv"][t, h * 64:(h + 1) * 64] = 0.0
    P = S + 5
    inp["cos"], inp["sin"] = rope_tables(P)
    inp["pos"] = None
    if c.pos:
        pos = torch.randint(0, P, (T,), generator=g).int()
        pos[0] = P - 1
        if T >= 4:
            pos[1] = pos[2] = S
        inp["pos"] = pos
    if c.cross:
        rows = torch.tensor([r for r in range(nb1) if r != unused_row(nb1)])
        inp["act"] = rows[torch.randint(0, len(rows), (T,), generator=g)].int()
        inp["bq"], inp["bk"], inp["bv"] = (0.5 * torch.randn(nb1, n * 64, generator=g) for n in (nq, nkv, nkv))
    if backward:
        inp["dq"], inp["dk"], inp["dv"] = rnd(T, nq * 64), rnd(T, nkv * 64), rnd(T, nkv * 64)
        # dwq, dwk, dbias_* are added to: what they hold before the call
        inp["base"] = {k: 0.25 * torch.randn(*s, generator=g) for k, s in
                       (("dwq", (64,)), ("dwk", (64,)), ("dbq", (nb1, nq * 64)), ("dbk", (nb1, nkv * 64)), ("dbv", (nb1, nkv * 64)))
                       if c.cross or k in ("dwq", "dwk")}
    return inp


# ---------------------------------------------------------------------------------------------------------------------------
# fp64 reference
# ---------------------------------------------------------------------------------------------------------------------------
def _ste_bf16(x):
    """the value rounded to bf16, identity gradient"""
    return x + (x.to(BF).to(x.dtype) - x).detach()


def _graph(c, inp, qkv, wq, wk, bq, bk, bv, lo, hi):
    n, nq, nkv = hi - lo, c.nq, c.nkv
    q = qkv[:, :nq * 64].view(n, nq, 64)
    k = qkv[:, nq * 64:(nq + nkv) * 64].view(n, nkv, 64)
    v = qkv[:, (nq + nkv) * 64:].view(n, nkv, 64)
    if c.cross:
        a = inp["act"][lo:hi].long()
        q, k, v = q + bq[a].view(n, nq, 64), k + bk[a].view(n, nkv, 64), v + bv[a].view(n, nkv, 64)
        if c.dtype == BF:
            v = _ste_bf16(v)                                  # v + bias_v goes back into the bf16 buffer
    pos = inp["pos"][lo:hi].long() if inp["pos"] is not None else torch.arange(lo, hi) % c.S
    cs, sn = inp["cos"][pos].double()[:, None, :], inp["sin"][pos].double()[:, None, :]

    def norm(x, w):
        xn = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + EPS)
        if c.dtype == BF and not c.cross:
            xn = _ste_bf16(xn)                                # Qwen3MoeRMSNorm on a bf16 tensor: .to(input_dtype) before * weight
        return w * xn

    def rope(y):
        return y * cs + torch.cat((-y[..., 32:], y[..., :32]), -1) * sn
    return rope(norm(q, wq)).reshape(n, -1), rope(norm(k, wk)).reshape(n, -1), v.reshape(n, -1)


def ref64_fwd(c, inp, lo=0, hi=None):
    """q_rot, k_rot and the v columns of rows [lo, hi), fp64, no gradient (the grid-cap cases walk their rows in chunks)"""
    hi = c.T if hi is None else hi
    with torch.no_grad():
        b = [inp[k].double() for k in ("bq", "bk", "bv")] if c.cross else [None] * 3
        q, k, v = _graph(c, inp, inp["qkv"][lo:hi].double(), inp["wq"].double(), inp["wk"].double(), *b, lo, hi)
    return dict(q=q, k=k, v=v)


def ref64(c, inp):
    """forward outputs and, from autograd, dqkv[:, :q|k], dwq, dwk, dbias_q / _k / _v (without what the buffers held before)"""
    names = ["qkv", "wq", "wk"] + (["bq", "bk", "bv"] if c.cross else [])
    leaves = [inp[k].double().requires_grad_(True) for k in names]
    q, k, v = _graph(c, inp, *leaves, *([None] * (6 - len(leaves))), 0, c.T)
    loss = (q * inp["dq"].double()).sum() + (k * inp["dk"].double()).sum()
    if c.cross:
        loss = loss + (v * inp["dv"].double()).sum()
    loss.backward()
    ref = dict(q=q.detach(), k=k.detach(), v=v.detach(), dqkv=leaves[0].grad[:, :(c.nq + c.nkv) * 64], dwq=leaves[1].grad, dwk=leaves[2].grad)
    if c.cross:
        ref.update(dbq=leaves[3].grad, dbk=leaves[4].grad, dbv=leaves[5].grad)
    return ref


def writeback(c, inp):
    """What the forward must leave in qkv, bit for bit (one IEEE addition per element, one rounding): self - unchanged; cross
    fp32 - q | k | v each with its bias row added; cross bf16 - q | k unchanged, v + bias_v rounded to bf16."""
    x = inp["qkv"].clone()
    if c.cross:
        a, nqk = inp["act"].long(), (c.nq + c.nkv) * 64
        x[:, nqk:] = (x[:, nqk:] + inp["bv"][a]).to(c.dtype).float()
        if c.dtype == F32:
            x[:, :nqk] = x[:, :nqk] + torch.cat((inp["bq"][a], inp["bk"][a]), 1)
    return x


# ---------------------------------------------------------------------------------------------------------------------------
# the kernels' formulas in plain fp32 torch, in their operation order
# ---------------------------------------------------------------------------------------------------------------------------
def emu32(c, inp, backward=True, lo=0, hi=None):
    hi = c.T if hi is None else hi
    n, nq, nkv = hi - lo, c.nq, c.nkv
    nqk = nq + nkv
    rd = lambda t: t.to(c.dtype).float()
    x = inp["qkv"][lo:hi, :nqk * 64].view(n, nqk, 64)
    out = {}
    if c.cross:
        a = inp["act"][lo:hi].long()
        x = x + torch.cat((inp["bq"][a].view(n, nq, 64), inp["bk"][a].view(n, nkv, 64)), 1)
        out["v"] = rd(inp["qkv"][lo:hi, nqk * 64:] + inp["bv"][a])
    w = torch.cat((inp["wq"].expand(nq, 64), inp["wk"].expand(nkv, 64)), 0)
    pos = inp["pos"][lo:hi].long() if inp["pos"] is not None else torch.arange(lo, hi) % c.S
    cs, sn = inp["cos"][pos][:, None, :], inp["sin"][pos][:, None, :]
    one = torch.ones(32)
    swap = lambda t: torch.cat((t[..., 32:], t[..., :32]), -1)               # the RoPE partner d +- 32
    rstd = torch.rsqrt((x * x).sum(-1, keepdim=True, dtype=F32) * (1.0 / 64.0) + EPS)
    xh = x * rstd
    xn = rd(xh) if (c.dtype == BF and not c.cross) else xh
    y = w * xn
    o = rd(y * cs + torch.cat((-one, one)) * swap(y) * sn)
    out["q"], out["k"] = o[:, :nq].reshape(n, -1), o[:, nq:].reshape(n, -1)
    if not backward:
        return out
    d = torch.cat((inp["dq"].view(n, nq, 64), inp["dk"].view(n, nkv, 64)), 1)
    dy = d * cs + torch.cat((one, -one)) * swap(d) * sn                     # transpose of the rotation
    dwt = dy * xn
    out["dwq"], out["dwk"] = dwt[:, :nq].sum((0, 1), dtype=F32), dwt[:, nq:].sum((0, 1), dtype=F32)
    gg = dy * w
    dot = (gg * xh).sum(-1, keepdim=True, dtype=F32) * (1.0 / 64.0)
    dx = rstd * (gg - xh * dot)
    out["dqkv"] = rd(dx.reshape(n, -1))
    if c.cross:
        for key, src, cols in (("dbq", dx[:, :nq].reshape(n, -1), nq * 64), ("dbk", dx[:, nq:].reshape(n, -1), nkv * 64),
                               ("dbv", inp["dv"], nkv * 64)):
            out[key] = torch.zeros(c.nb1, cols).index_add_(0, a, src)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# metrics
# ---------------------------------------------------------------------------------------------------------------------------
def rel(got, ref):
    """the existing tests' _rel: the largest error over the largest reference magnitude"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def planted_mask(c):
    """the cells of dqkv[:, :q|k] that belong to a planted all-zero row of a SELF case: there rstd = eps^-1/2 = 1000 and the
    gradient is a thousand times the others - under `rel` those cells alone would set the scale, so they are judged apart"""
    m = torch.zeros(c.T, (c.nq + c.nkv) * 64, dtype=torch.bool)
    if not c.cross:
        for t, h in planted(c):
            m[t, h * 64:(h + 1) * 64] = True
    return m


def metrics(c, got, ref, backward=True):
    """metric name -> value, for whatever of q, k, v, dqkv, dwq, dwk, dbq, dbk, dbv `got` holds; gradients in `got` are without
    what the buffers held before"""
    m = dict(fwd=max(rel(got["q"], ref["q"]), rel(got["k"], ref["k"])))
    if c.cross:
        m["v"] = rel(got["v"], ref["v"])
    if not backward:
        return m
    pm = planted_mask(c)
    g, r = got["dqkv"].detach().double().cpu(), ref["dqkv"]
    m["dqkv"] = rel(torch.where(pm, 0.0, g), torch.where(pm, 0.0, r))
    if bool(pm.any()):
        m["dqkv_planted"] = rel(g[pm], r[pm])
    m["dw"] = max(rel(got["dwq"], ref["dwq"]), rel(got["dwk"], ref["dwk"]))
    if c.cross:
        m["dbias"] = max(rel(got["dbq"], ref["dbq"]), rel(got["dbk"], ref["dbk"]))
        m["dbias_v"] = rel(got["dbv"], ref["dbv"])
    return m


# bars the existing tests (test_ops_gpu.test_qknorm_rope_fwd_bwd, test_bf16_gpu.test_qknorm_rope_bf16) hold these quantities to
ULP16 = 2.0 ** -8
EXISTING = {F32: dict(fwd=3e-6, v=3e-6, dqkv=2e-5, dqkv_planted=2e-5, dw=2e-5, dbias=2e-5, dbias_v=2e-5),
            BF: dict(fwd=1.5 * ULP16, v=1.5 * ULP16, dqkv=2 * ULP16, dqkv_planted=2 * ULP16, dw=1e-3, dbias=1e-3, dbias_v=1e-3)}


def bar(dtype, metric, worst):
    """four times the restatement's worst value, never above the existing bar - unless the restatement itself misses that one"""
    return 4 * worst if worst > EXISTING[dtype][metric] else min(EXISTING[dtype][metric], 4 * worst)


CHUNK = 32768


def calibrate():
    worst = {}

    def note(c, m):
        for k, v in m.items():
            worst[c.dtype, k] = max(worst.get((c.dtype, k), 0.0), v)

    for dt in (F32, BF):
        for cross in (False, True):
            for nq, nkv in HEADS:
                for c in fwd_cases(dt, cross, nq, nkv):
                    inp = make_inputs(c, backward=False)
                    note(c, metrics(c, emu32(c, inp, backward=False), ref64_fwd(c, inp), backward=False))
        c = Case("fwd_grid_cap", dt, False, 1, 1, 0, GRID_CAP_T[dt], False)
        inp = make_inputs(c, backward=False)
        for lo in range(0, c.T, CHUNK):
            hi = min(c.T, lo + CHUNK)
            note(c, metrics(c, emu32(c, inp, False, lo, hi), ref64_fwd(c, inp, lo, hi), backward=False))
    for c in BWD_CASES:
        c.check_regime()
        inp = make_inputs(c)
        note(c, metrics(c, emu32(c, inp), ref64(c, inp)))
    print(f"{'metric':22s} {'fp32 torch, worst':>18s} {'x4':>10s} {'existing':>10s} {'bar':>10s}")
    for (dt, k), v in sorted(worst.items(), key=lambda kv: (NAME[kv[0][0]] != "f32", kv[0][1])):
        print(f"{NAME[dt] + ' ' + k:22s} {v:18.3e} {4 * v:10.3e} {EXISTING[dt][k]:10.3e} {bar(dt, k, v):10.3e}")


if __name__ == "__main__":
    calibrate()
