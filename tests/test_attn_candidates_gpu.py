"""gamer_attn_candidates (csrc/candidates.hip): the cached decode attention for any number of rows per sample, against a dense fp64
softmax attention and against gamer_attn_decode where that kernel can run.

B = 3 left-padded samples: sample 0 has a single allowed prompt key, sample 1 has none (a cross block: uniform = 1 gives the mean
of V over all L0 + t keys; uniform = 0 gives exact zeros, which is what gamer_attn_decode gives for such a row - compared at
nb = 1 below), sample 2 a random mask.  The operands are drawn as tests/test_decode.py draws them for gamer_attn_decode and the
bar is the one that test holds the old kernel to: max |error| / max |reference| < 2e-6.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV, B, TMAX, SCALE, BAR = "cuda", 3, 4, 0.125, 2e-6
HEADS = [(2, 2), (6, 3)]                      # (nq, nkv): G = 1 and G = 2, every group size the kernels are built for
_cache = {}


def _inputs(nq, nkv, nb, L0):
    """Operands (host fp32) and masks of a shape, drawn once."""
    key = (nq, nkv, nb, L0)
    if key not in _cache:
        g = torch.Generator().manual_seed(1000 * L0 + 10 * nb + nq)
        N = B * nb
        q = torch.randn(N, nq * 64, generator=g)
        kp, vp = torch.randn(B * L0, nkv * 64, generator=g), torch.randn(B * L0, nkv * 64, generator=g)
        kg, vg = torch.randn(N, TMAX, nkv * 64, generator=g), torch.randn(N, TMAX, nkv * 64, generator=g)
        ok = (torch.rand(B, L0, generator=g) < 0.6).to(torch.int32)
        ok[0] = 0
        ok[0, L0 - 2] = 1                                    # a single allowed key behind the left padding
        ok[1] = 0                                            # nothing allowed
        ok[2, :5] = 0                                        # left padding
        ok[2, -1] = 1
        _cache[key] = (q, kp, vp, kg, vg, ok)
    return _cache[key]


def _dense(q, kp, vp, kg, vg, ok, nq, nkv, nb, L0, t, gen_ok, uniform):
    """fp64 softmax attention of every row and head; a row without an allowed key: mean of V (uniform) or zeros."""
    N, G = B * nb, nq // nkv
    qd = q.double().view(B, nb, nkv, G, 64)
    K = torch.cat([kp.double().view(B, 1, L0, nkv, 64).expand(B, nb, L0, nkv, 64), kg.double().view(B, nb, TMAX, nkv, 64)[:, :, :t]], 2)
    V = torch.cat([vp.double().view(B, 1, L0, nkv, 64).expand(B, nb, L0, nkv, 64), vg.double().view(B, nb, TMAX, nkv, 64)[:, :, :t]], 2)
    allowed = torch.cat([ok.bool(), torch.full((B, t), bool(gen_ok))], 1)                  # [B, L0 + t]
    s = torch.einsum("bnkgd,bnjkd->bnkgj", qd, K) * SCALE
    s = s.masked_fill(~allowed[:, None, None, None, :], float("-inf"))
    none = ~allowed.any(1)
    s[none] = 0.0
    out = torch.einsum("bnkgj,bnjkd->bnkgd", torch.softmax(s, -1), V)
    for b in range(B):
        if none[b]:
            out[b] = V[b].mean(1)[:, :, None, :].expand(nb, nkv, G, 64) if uniform is not None and uniform[b] else 0.0
    return out.reshape(N, nq * 64)


def _run(fn, q, kp, vp, kg, vg, ok, nq, nkv, nb, L0, t, gen_ok, uniform):
    vbuf = torch.zeros(B * L0, (nq + 2 * nkv) * 64)          # v lives inside a wider buffer in the engine
    vbuf[:, (nq + nkv) * 64:] = vp
    o = torch.full((B * nb, nq * 64), float("nan"), device=DEV)
    fn(q.to(DEV), kp.to(DEV), vbuf.to(DEV)[:, (nq + nkv) * 64:], ok.to(DEV), kg.to(DEV), vg.to(DEV), t, gen_ok,
       None if uniform is None else uniform.to(DEV), B, nb, L0, nq, nkv, SCALE, o)
    return o.cpu()


def _relerr(got, ref):
    return float((got.double() - ref.double()).abs().max() / ref.abs().max())


@pytest.mark.parametrize("nq,nkv", HEADS)
@pytest.mark.parametrize("nb", [1, 33, 130])
@pytest.mark.parametrize("L0", [37, 64])
@pytest.mark.parametrize("t", [1, 3])
def test_against_dense_fp64(nq, nkv, nb, L0, t):
    from gamer_amd import ops
    q, kp, vp, kg, vg, ok = _inputs(nq, nkv, nb, L0)
    # stale generated rows beyond t are NaN: they must not reach the output
    kg, vg = kg.clone(), vg.clone()
    kg[:, t:] = float("nan")
    vg[:, t:] = float("nan")
    ok_self = ok.clone()
    ok_self[1, -3:] = 1                                      # a self block always has kept keys
    uni = (ok.sum(1) == 0).to(torch.int32)
    cases = [("self", ok_self, True, None), ("cross-uniform", ok, False, uni), ("cross-zero", ok, False, torch.zeros_like(uni)),
             ("self-no-prompt-key", ok, True, None)]        # gen_ok = 1 with sample 1's prompt fully masked: its own positions only
    for name, kok, gen_ok, uniform in cases:
        args = (q, kp, vp, kg, vg, kok, nq, nkv, nb, L0, t, gen_ok, uniform)
        o = _run(ops.attn_candidates, *args)
        ref = _dense(*args)
        assert torch.isfinite(o).all(), name
        err = _relerr(o, ref)
        print(f"attn_candidates nq={nq} nkv={nkv} nb={nb} L0={L0} t={t} {name}: rel err {err:.3e}")
        assert err < BAR, (name, err)
        if name == "cross-zero":
            assert float(o.view(B, nb, -1)[1].abs().max()) == 0.0
        assert torch.equal(o, _run(ops.attn_candidates, *args)), name          # no atomics: the same bits on every call
        if nb * (nq // nkv) <= 64:
            # where the old kernel can run, the two agree within the bar (they add the keys in different orders)
            old = _run(ops.attn_decode, *args)
            assert _relerr(o, old.double()) < BAR, name
            if name == "cross-zero":
                assert float(old.view(B, nb, -1)[1].abs().max()) == 0.0        # gamer_attn_decode's answer for such a row: zeros


def test_host_checks_report_errors():
    from gamer_amd import _lib, ops
    nq, nkv, nb, L0 = 2, 2, 3, 37
    q, kp, vp, kg, vg, ok = _inputs(nq, nkv, 1, L0)
    q = q.repeat(nb, 1)
    kg, vg = kg.repeat(nb, 1, 1), vg.repeat(nb, 1, 1)
    lib = _lib.load()
    with pytest.raises(RuntimeError, match="gamer_attn_candidates"):
        _run(ops.attn_candidates, q, kp, vp, kg, vg, ok, nq, nkv, nb, L0, TMAX + 1, True, None)          # t > tmax
    assert b"gamer_attn_candidates" in lib.gamer_last_error()
    with pytest.raises(RuntimeError, match="L0"):
        big = torch.zeros(1, 8000, dtype=torch.int32)
        o = torch.empty(1, nq * 64, device=DEV)
        z = torch.zeros(8000, nkv * 64, device=DEV)
        ops.attn_candidates(q[:1].to(DEV), z, z, big.to(DEV), kg[:1].to(DEV), vg[:1].to(DEV), 1, True, None, 1, 1, 8000, nq, nkv,
                            SCALE, o)


def test_token_logprob_against_log_softmax():
    from gamer_amd import ops
    g = torch.Generator().manual_seed(5)
    N, V, ld = 37, 333, 336
    logits = (torch.randn(2 * N, ld, generator=g) * 3).to(DEV)
    rows = torch.randperm(2 * N, generator=g)[:N].to(DEV, torch.int32)
    tok = torch.randint(0, V, (N,), generator=g).to(DEV)
    out = torch.empty(N, device=DEV)
    ops.token_logprob(logits, rows, tok, V, out)
    ref = torch.log_softmax(logits[rows.long(), :V].double(), -1).gather(1, tok[:, None])[:, 0]
    assert float((out.double() - ref).abs().max()) < 1e-5
    ops.token_logprob(logits, None, tok, V, out, accumulate=True)
    ref2 = ref + torch.log_softmax(logits[:N, :V].double(), -1).gather(1, tok[:, None])[:, 0]
    assert float((out.double() - ref2).abs().max()) < 2e-5
