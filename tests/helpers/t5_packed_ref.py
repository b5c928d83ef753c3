"""Reference code of the packed (variable-length) T5 attention tests (tests/test_tiger_packed_gpu.py): one case runs the packed entry
points on the gathered rows, the dense entry points with the right-padding key mask of the same lengths, the fp64 restatement and
the fp32 torch restatement, and returns all four in the PACKED layouts.  The inputs are drawn as tests/helpers/t5_attention_ref.case
draws them (scores of O(10)); d_o is zero on the padding queries, as it is in the model, whose padded encoder rows nothing reads."""
import torch

import t5_attention_ref as ref

DEV = ref.DEV
NB, MAXD = ref.NB, ref.MAXD
QUANTITIES = ref.QUANTITIES


def _offsets(lens):
    from gamer_amd import ops
    return ops.T5Offsets.from_lengths(torch.tensor(lens), DEV)


def _rows(lens, S):
    """the flat [B S] indices of the real tokens"""
    return torch.cat([b * S + torch.arange(n) for b, n in enumerate(lens)]) if sum(lens) else torch.zeros(0, dtype=torch.long)


def case(long, lens, h, d, bias, causal, p, Sd=None, max_s=None, seed=(7 << 32) | 0x51, rows=None, n_slab=None, torch32=True,
         truth=True, dense=True, salt=0):
    """``lens``: the rows' key lengths.  Self attention (Sd None): the queries are the same tokens.  Cross attention: Sd dense
    queries per row, no bias.  ``max_s``: the padded length (default: the longest row).  ``rows``: keep these batch rows only
    (after the draw, so that a row's numbers do not depend on its neighbours).
    -> (packed, dense, fp64, fp32 torch), dicts of o, lse [h, Tq], dq, dk, dv (+ drel, dtable, slabs) on the real rows"""
    from gamer_amd import ops
    from gamer_amd.tiger import bucket_vector
    lens = list(lens)
    B, Sk = len(lens), max_s or max(lens)
    cross = Sd is not None
    Sq = Sd if cross else Sk
    qlens = [Sq] * B if cross else lens
    g = torch.Generator().manual_seed(100003 * Sq + 1009 * Sk + 101 * h + 7 * d + B + (3 if bias else 0) + (5 if causal else 0) + salt)
    I, R = h * d, Sq + Sk - 1
    q = torch.randn(B, Sq, I, generator=g) * (10.0 / d) ** 0.5
    k = torch.randn(B, Sk, I, generator=g)
    v = torch.randn(B, Sk, I, generator=g)
    d_o = torch.randn(B, Sq, I, generator=g)
    table = torch.randn(NB, h, generator=g) if bias else None
    if rows is not None:
        sel = torch.tensor(rows)
        q, k, v, d_o, B = q[sel], k[sel], v[sel], d_o[sel], len(rows)
        lens, qlens = [lens[r] for r in rows], [qlens[r] for r in rows]
    keep = torch.arange(Sk)[None, :] < torch.tensor(lens)[:, None]
    qreal = torch.arange(Sq)[None, :] < torch.tensor(qlens)[:, None]
    d_o = d_o * qreal[:, :, None]
    qrows, krows = _rows(qlens, Sq), _rows(lens, Sk)
    Tq, Tk = qrows.numel(), krows.numel()
    bucket = bucket_vector(max(Sq, Sk), not causal, NB, MAXD)
    bucket = bucket[max(Sq, Sk) - Sq:max(Sq, Sk) - Sq + R].contiguous()
    bd = bucket.to(DEV)
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)
    rel = None
    if bias:
        rel = nan(h, R)
        ops.t5_bias_expand(table.to(DEV), bd, rel)
    n = n_slab or ops.t5_n_slab(B, h)
    fwd, bwd = (ops.t5_attn_long_packed_fwd, ops.t5_attn_long_packed_bwd) if long else (ops.t5_attn_packed_fwd, ops.t5_attn_packed_bwd)
    dfwd, dbwd = (ops.t5_attn_long_fwd, ops.t5_attn_long_bwd) if long else (ops.t5_attn_fwd, ops.t5_attn_bwd)

    def buffers(qf, kf, vf, nq, nk):
        """(q, k, v, dq, dk, dv) as the model lays them out: column blocks of one q|k|v buffer, or q and one k|v buffer"""
        if not cross:
            buf, dbuf = torch.cat([qf, kf, vf], 1).to(DEV), nan(nq, 3 * I)
            return buf[:, :I], buf[:, I:2 * I], buf[:, 2 * I:], dbuf[:, :I], dbuf[:, I:2 * I], dbuf[:, 2 * I:]
        kvb, dkv = torch.cat([kf, vf], 1).to(DEV), nan(nk, 2 * I)
        return qf.to(DEV), kvb[:, :I], kvb[:, I:], nan(nq, I), dkv[:, :I], dkv[:, I:]

    def finish(res, slabs):
        if bias:
            dtable = nan(NB, h)
            ops.t5_bias_fold(slabs, bd, dtable)
            res.update(drel=slabs[0].sum(0), dtable=dtable, slabs=slabs)
        return res
    flat = lambda x, S: x.reshape(B * S, I)
    # ---- the packed entry points on the gathered rows
    q_off, k_off = _offsets(qlens), _offsets(lens)
    if not cross:
        k_off = q_off                                                  # self attention passes one array twice
    qd, kd, vd, dq, dk, dv = buffers(flat(q, Sq)[qrows], flat(k, Sk)[krows], flat(v, Sk)[krows], Tq, Tk)
    o, lse = nan(Tq, I), nan(h, Tq)
    fwd(qd, kd, vd, rel, q_off, k_off, B, Sq, Sk, h, d, causal, p, seed, o, lse)
    slabs = nan(1, n, h, R) if bias else None
    bwd(qd, kd, vd, rel, q_off, k_off, B, Sq, Sk, h, d, causal, p, seed, flat(d_o, Sq)[qrows].to(DEV), lse, dq, dk, dv,
        None if slabs is None else slabs[0])
    packed = finish(dict(o=o, lse=lse, dq=dq, dk=dk, dv=dv), slabs)
    torch.cuda.synchronize()

    def to_packed(res):
        """a dense run's outputs on the real rows, in the packed layouts"""
        out = dict(o=res["o"][qrows.to(res["o"].device)], dq=res["dq"][qrows.to(res["o"].device)],
                   dk=res["dk"][krows.to(res["o"].device)], dv=res["dv"][krows.to(res["o"].device)],
                   lse=res["lse"].permute(1, 0, 2).reshape(h, B * Sq)[:, qrows.to(res["o"].device)])
        out.update({k_: res[k_] for k_ in ("drel", "dtable", "slabs") if k_ in res})
        return out
    # ---- the dense entry points with the right-padding mask of the same lengths
    dn = None
    if dense:
        qd, kd, vd, dq, dk, dv = buffers(flat(q, Sq), flat(k, Sk), flat(v, Sk), B * Sq, B * Sk)
        keepd = keep.to(torch.uint8).to(DEV)
        o, lse = nan(B * Sq, I), nan(B, h, Sq)
        dfwd(qd, kd, vd, rel, keepd, B, Sq, Sk, h, d, causal, p, seed, o, lse)
        slabs = nan(1, n, h, R) if bias else None
        dbwd(qd, kd, vd, rel, keepd, B, Sq, Sk, h, d, causal, p, seed, flat(d_o, Sq).to(DEV), lse, dq, dk, dv,
             None if slabs is None else slabs[0])
        dn = to_packed(finish(dict(o=o, lse=lse, dq=dq, dk=dk, dv=dv), slabs))
        torch.cuda.synchronize()
    if not truth:
        return packed, dn, None, None
    mult = ref.keep_mask(p, seed, B, h, Sq, Sk) if p > 0 else None       # the DENSE geometry

    def restate(dtype, dev):
        leaf = lambda t: None if t is None else t.to(dev).to(dtype).requires_grad_(True)
        heads = lambda x, S: x.view(B, S, h, d).permute(0, 2, 1, 3)
        ql, kl, vl, tl = leaf(q), leaf(k), leaf(v), leaf(table)
        r = None
        if bias:
            r = tl[bucket.long().to(dev)].t()
            r.retain_grad()
        ctx, l = ref.attention(heads(ql, Sq), heads(kl, Sk), heads(vl, Sk), r, keep.to(dev), causal,
                               None if mult is None else mult.to(dev).to(dtype))
        out = ctx.permute(0, 2, 1, 3).reshape(B * Sq, I)
        (out * flat(d_o, Sq).to(dev).to(dtype)).sum().backward()
        res = dict(o=out, lse=l, dq=flat(ql.grad, Sq), dk=flat(kl.grad, Sk), dv=flat(vl.grad, Sk))
        if bias:
            res.update(drel=r.grad, dtable=tl.grad)
        return to_packed({k_: t.detach() for k_, t in res.items()})
    return packed, dn, restate(torch.float64, "cpu"), (restate(torch.float32, DEV) if torch32 else None)


def grid_errors(cases):
    """{quantity: [(case, packed error, fp32 torch error, reference magnitude, packed magnitude, largest input gradient, packed
    against dense)]} over ``cases`` = keyword dicts of case(); asserts that no NaN of the pre-filled packed outputs survives"""
    errs = {k: [] for k in QUANTITIES}
    for c in cases:
        packed, dn, truth, t32 = case(**c)
        tag = tuple(sorted(c.items()))
        gmax = max(float(truth[k].abs().max()) for k in ("dq", "dk", "dv") if truth[k].numel())
        for k in truth:
            fin = torch.isfinite(truth[k])
            got = packed[k]
            errs[k].append((tag, ref.rel_err(got, truth[k]), ref.rel_err(t32[k], truth[k]),
                            float(truth[k][fin].abs().max()) if bool(fin.any()) else 0.0,
                            float(got[torch.isfinite(got)].abs().max()) if bool(torch.isfinite(got).any()) else 0.0, gmax,
                            _against(got, dn[k], truth[k])))
        for k, t in packed.items():
            assert not bool(torch.isnan(t).any()), (c, k)              # (every output was poisoned with NaN before the launch)
    return errs


def _against(got, other, truth):
    """the packed-against-dense difference on the scale of the reference tensor (what rel_err divides by)"""
    got, other, truth = got.detach().double().cpu(), other.detach().double().cpu(), truth.detach().double().cpu()
    fin = torch.isfinite(truth)
    if not bool(torch.equal(torch.isfinite(got), torch.isfinite(other))):
        return float("inf")
    if not bool(fin.any()):
        return 0.0
    return float((got[fin] - other[fin]).abs().max() / truth[fin].abs().max().clamp_min(1e-30))
