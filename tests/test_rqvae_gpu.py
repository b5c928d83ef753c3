"""The RQ-VAE item tokenizer on the GPU: the two quantiser kernels against fp64 restatements that follow the kernel's own
indices, the model against the real reference classes (tests/golden/rqvae_small.npz, tools/make_golden_rqvae.py), and the two
commands end to end.

Bars.  Indices: (a) the chosen code's fp64 distance is at most (1 + 1e-5) times the fp64 minimum plus 1e-12; (b) wherever the
fp64 gap between the best and the second-best distance is at least 1e-4 (relative), the index is the fp64 argmin, and such (row,
level) pairs are at least 95 % of all.  Values: the error against the fp64 chain, as a fraction of the largest magnitude of the
quantity, may be 4 times the error of the same maths written as fp32 torch ops on the same inputs and indices (only the order of
the sums differs; the kernels keep their long sums - a row's |e - r|^2, the loss sums, the scatter into a code - in fp64 and round
once, so the order of a long sum is not what the comparison measures).  Model against the
reference: the bars of test_mbstr_gpu.py's model fixture, 2e-5 outputs / 1e-5 loss / 2e-4 gradients (the generator recorded the
reference's own fp32 error against its fp64 self: 3e-7 outputs, 5e-8 losses, 4e-7 gradients, so those bars carry over)."""
import argparse
import json
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MU = 0.25
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("needs the GPU")
    from gamer_amd import build
    build.build()
    yield
    print("\n[rqvae worst] " + json.dumps(WORST, sort_keys=True))


@pytest.fixture(scope="module")
def fx(golden):
    return golden("rqvae_small")


def _note(key, got, bar=None):
    WORST[key] = max(WORST.get(key, 0.0), float(got))
    if bar is not None:
        WORST[key + "_torch"] = max(WORST.get(key + "_torch", 0.0), float(bar))


def _err(got, ref):
    return float((got.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def _offsets(ks):
    return [0] + list(np.cumsum(ks))


def _inputs(B, D, ks, seed):
    g = torch.Generator().manual_seed(seed)
    r = torch.randn(B, D, generator=g).to(DEV)
    E = (0.05 * torch.randn(sum(ks), D, generator=g)).to(DEV)
    return r, E


def _fwd(r, E, ks, modes=None, lvl0=0, lvl1=None, idx=None, xq=None, dist=False, keep=True):
    from gamer_amd import ops
    B, D = r.shape
    L = len(ks)
    lvl1 = L if lvl1 is None else lvl1
    f32 = dict(dtype=torch.float32, device=DEV)
    o = dict(idx=torch.full((B, L), -1, dtype=torch.int32, device=DEV) if idx is None else idx.clone(),
             xq=torch.zeros(B, D, **f32) if xq is None else xq.clone(), res=torch.zeros(B, D, **f32),
             r_levels=torch.zeros(L, B, D, **f32) if keep else None, sums=torch.zeros(L, **f32),
             dist=torch.zeros(B, ks[lvl1 - 1], **f32) if dist else None)
    ops.rvq_fwd(r, E, _offsets(ks), modes or [0] * L, lvl0, lvl1, o["idx"], o["xq"], o["res"], o["r_levels"], o["dist"], o["sums"])
    torch.cuda.synchronize()
    return o


def _chain(r, E, ks, idx, dtype):
    """the quantiser along given indices, in ``dtype``, written as the reference writes it: (x_q, residual, loss sums, distances,
    the residual entering every level)"""
    off = _offsets(ks)
    r = r.to(dtype)
    xq, sums, dists, rs = torch.zeros_like(r), [], [], []
    for l in range(len(ks)):
        rs.append(r)
        El = E[off[l]:off[l + 1]].to(dtype)
        dists.append(torch.sum(r ** 2, dim=1, keepdim=True) + torch.sum(El ** 2, dim=1, keepdim=True).t() - 2 * torch.matmul(r, El.t()))
        e = El[idx[:, l].long()]
        sums.append(((e - r) ** 2).sum())
        if dtype == torch.float64:
            x_res = e                                        # r_{l+1} = r_l - E_l[idx_l]
        else:
            x_res = r + (e - r)
        xq, r = xq + x_res, r - x_res
    return xq, r, torch.stack(sums), dists, rs


def _bar(torch_err):
    return 4.0 * torch_err


# ---- forward kernel ---------------------------------------------------------------------------------------------------------------
CODEBOOKS = [[3], [20, 24, 20, 32], [256] * 4, [1024, 5]]


@pytest.mark.parametrize("ks", CODEBOOKS, ids=lambda k: "K" + "-".join(map(str, k[:2])) + f"x{len(k)}")
@pytest.mark.parametrize("D", [8, 32, 64])
@pytest.mark.parametrize("B", [1, 37, 130])
def test_forward_against_the_fp64_chain(B, D, ks):
    r, E = _inputs(B, D, ks, 1000 * B + 10 * D + len(ks))
    o = _fwd(r, E, ks)
    idx = o["idx"]
    L = len(ks)
    assert all(int(idx[:, l].min()) >= 0 and int(idx[:, l].max()) < ks[l] for l in range(L))
    xq64, r64, s64, d64, rs64 = _chain(r, E, ks, idx, torch.float64)
    xq32, r32, s32, d32, rs32 = _chain(r, E, ks, idx, torch.float32)
    clear = total = 0
    for l in range(L):
        two = torch.topk(d64[l], min(2, ks[l]), dim=1, largest=False).values
        chosen = d64[l].gather(1, idx[:, l:l + 1].long())[:, 0]
        assert bool((chosen <= (1 + 1e-5) * two[:, 0] + 1e-12).all()), f"rule (a), level {l}"
        gap = (two[:, -1] - two[:, 0]) / two[:, 0] if ks[l] > 1 else torch.full_like(chosen, float("inf"))
        ok = gap >= 1e-4
        assert torch.equal(idx[:, l][ok].long(), d64[l].argmin(1)[ok]), f"rule (b), level {l}"
        clear, total = clear + int(ok.sum()), total + B
    assert clear >= 0.95 * total, (clear, total)
    for name, got, ref, t32 in (("x_q", o["xq"], xq64, xq32), ("residual", o["res"], r64, r32), ("loss_sums", o["sums"], s64, s32)):
        e, t = _err(got, ref), _err(t32, ref)
        print(f"B={B} D={D} K={ks}: {name} kernel {e:.3e} torch {t:.3e}")
        _note("fwd_" + name, e, t)
        assert e <= _bar(t), (name, e, t)
    for l in range(L):                                     # the residual entering every level, as the backward reads it
        assert _err(o["r_levels"][l], rs64[l]) <= _bar(_err(rs32[l], rs64[l])), l
    # distance-only on the last level: nothing of that level but d; the levels before it as in the full run
    od = _fwd(r, E, ks, dist=True)
    assert torch.equal(od["idx"][:, :L - 1], idx[:, :L - 1]) and bool((od["idx"][:, L - 1] == -1).all())
    assert torch.equal(od["res"], o["r_levels"][L - 1]) and torch.equal(od["sums"][:L - 1], o["sums"][:L - 1])
    e, t = _err(od["dist"], d64[L - 1]), _err(d32[L - 1], d64[L - 1])
    print(f"B={B} D={D} K={ks}: dist kernel {e:.3e} torch {t:.3e}")
    _note("fwd_dist", e, t)
    assert e <= _bar(t), ("dist", e, t)
    # ... and the level run again with the index given continues to the same result
    o2 = _fwd(od["res"], E, ks, modes=[0] * (L - 1) + [1], lvl0=L - 1, idx=idx, xq=od["xq"])
    assert torch.equal(o2["xq"], o["xq"]) and torch.equal(o2["res"], o["res"]) and torch.equal(o2["sums"][L - 1], o["sums"][L - 1])


def test_the_issue_recipe_leaves_few_unclear_pairs():
    """N(0, 1) rows, N(0, 0.05) codebooks at 1024 x [256] * 4: the pairs below a gap of 1e-4 are a fraction of a per cent"""
    ks = [256] * 4
    r, E = _inputs(1024, 32, ks, 7)
    o = _fwd(r, E, ks, keep=False)
    d64 = _chain(r, E, ks, o["idx"], torch.float64)[3]
    unclear = 0
    for l in range(4):
        two = torch.topk(d64[l], 2, dim=1, largest=False).values
        ok = (two[:, 1] - two[:, 0]) / two[:, 0] >= 1e-4
        assert torch.equal(o["idx"][:, l][ok].long(), d64[l].argmin(1)[ok])
        unclear += int((~ok).sum())
    assert unclear <= 0.05 * 4096
    again = _fwd(r, E, ks, keep=False)
    assert all(torch.equal(again[k], o[k]) for k in ("idx", "xq", "res", "sums"))


def test_identical_codes_the_lower_index_wins():
    ks = [40, 40]
    r, E = _inputs(9, 16, ks, 3)
    E[7], E[19], E[30] = E[3], E[3], E[3]                 # another lane of the row, the same lane, and both
    r[:] = E[3] + 1e-3 * r
    E[40 + 33] = E[40 + 17]
    idx = _fwd(r, E, ks)["idx"]
    assert bool((idx[:, 0] == 3).all())
    assert not bool((idx[:, 1] == 33).any())


def test_a_row_equal_to_a_code_chooses_it():
    ks = [24]
    r, E = _inputs(5, 32, ks, 4)
    E *= 20                                                # codes of the rows' size: a distance near 0 is cancellation
    r[2] = E[11]
    o = _fwd(r, E, ks)
    assert int(o["idx"][2, 0]) == 11 and float(o["res"][2].abs().max()) == 0.0 and torch.equal(o["xq"][2], E[11])
    d = _fwd(r, E, ks, dist=True)["dist"]
    assert abs(float(d[2, 11])) <= 1e-5 * float((E[11] ** 2).sum()) and int(d[2].argmin()) == 11


def test_given_indices_reproduce_the_argmin_run_bit_for_bit():
    ks = [20, 24, 20, 32]
    r, E = _inputs(37, 8, ks, 5)
    o = _fwd(r, E, ks)
    g = _fwd(r, E, ks, modes=[1] * 4, idx=o["idx"])
    assert all(torch.equal(g[k], o[k]) for k in ("idx", "xq", "res", "sums", "r_levels"))


def test_memory_outside_the_tensors_is_neither_read_nor_written():
    from gamer_amd import ops
    ks, B, D, pad = [20, 24, 20, 37], 37, 8, 5
    L = len(ks)
    r, E = _inputs(B, D, ks, 6)
    clean = _fwd(r, E, ks)
    nan = float("nan")
    rb = torch.full((B + pad, D + 4), nan, device=DEV)
    rb[:B, :D] = r
    Eb = torch.full((sum(ks) + 64, D), nan, device=DEV)
    Eb[:sum(ks)] = E
    idx = torch.full((B + pad, L), -7, dtype=torch.int32, device=DEV)
    xq, res = torch.full((B + pad, D), 777.0, device=DEV), torch.full((B + pad, D), 777.0, device=DEV)
    sums = torch.zeros(L, device=DEV)
    dist = torch.full((B + pad, ks[-1]), 777.0, device=DEV)
    ops.rvq_fwd(rb[:B, :D], Eb, _offsets(ks), [0] * L, 0, L, idx, xq, res, None, None, sums)
    torch.cuda.synchronize()
    assert torch.equal(idx[:B], clean["idx"]) and torch.equal(xq[:B], clean["xq"]) and torch.equal(res[:B], clean["res"])
    assert torch.equal(sums, clean["sums"])
    assert bool((idx[B:] == -7).all()) and bool((xq[B:] == 777.0).all()) and bool((res[B:] == 777.0).all())
    ops.rvq_fwd(rb[:B, :D], Eb, _offsets(ks), [0] * L, 0, L, idx, xq, res, None, dist, sums)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dist[:B]).all()) and bool((dist[B:] == 777.0).all())
    assert bool(torch.isnan(rb[B:]).all()) and bool(torch.isnan(rb[:, D:]).all()) and bool(torch.isnan(Eb[sum(ks):]).all())
    assert torch.equal(rb[:B, :D], r) and torch.equal(Eb[:sum(ks)], E)


def test_refusals_name_the_entry_point_and_launch_nothing():
    from gamer_amd import ops

    def refused(fn, name):
        with pytest.raises(RuntimeError, match=name):
            fn()
        torch.cuda.synchronize()

    def bufs(B, D, L):
        return (torch.full((B, L), -7, dtype=torch.int32, device=DEV), torch.full((B, D), 777.0, device=DEV),
                torch.full((B, D), 777.0, device=DEV))

    for D, ks in ((65, [8]), (8, [1025]), (8, [4] * 9)):
        L = len(ks)
        r, E = torch.zeros(4, D, device=DEV), torch.zeros(sum(ks), D, device=DEV)
        idx, xq, res = bufs(4, D, L)
        refused(lambda: ops.rvq_fwd(r, E, _offsets(ks), [0] * L, 0, L, idx, xq, res), "gamer_rvq_fwd")
        assert bool((idx == -7).all()) and bool((xq == 777.0).all()) and bool((res == 777.0).all())
        dz, dE = torch.full((4, D), 777.0, device=DEV), torch.full((sum(ks), D), 777.0, device=DEV)
        refused(lambda: ops.rvq_bwd(idx, torch.zeros(L, 4, D, device=DEV), E, _offsets(ks), None, torch.ones(L, device=DEV), MU, dz, dE),
                "gamer_rvq_bwd")
        assert bool((dz == 777.0).all()) and bool((dE == 777.0).all())
    r, E = torch.zeros(4, 8, device=DEV), torch.zeros(8, 8, device=DEV)
    idx, xq, res = bufs(4, 8, 1)
    refused(lambda: ops.rvq_fwd(r, None, [0, 8], [0], 0, 1, idx, xq, res), "gamer_rvq_fwd")
    refused(lambda: ops.rvq_fwd(r, E, [0, 8], [0], 0, 1, None, xq, res), "gamer_rvq_fwd")
    refused(lambda: ops.rvq_fwd(r, E, [0, 8], [2], 0, 1, idx, xq, res), "gamer_rvq_fwd")
    refused(lambda: ops.rvq_fwd(r, E, [0, 8], [0], 1, 1, idx, xq, res), "gamer_rvq_fwd")
    assert bool((idx == -7).all()) and bool((xq == 777.0).all()) and bool((res == 777.0).all())
    dz, dE = torch.full((4, 8), 777.0, device=DEV), torch.full((8, 8), 777.0, device=DEV)
    refused(lambda: ops.rvq_bwd(idx, None, E, [0, 8], None, torch.ones(1, device=DEV), MU, dz, dE), "gamer_rvq_bwd")
    assert bool((dz == 777.0).all()) and bool((dE == 777.0).all())


# ---- backward kernel --------------------------------------------------------------------------------------------------------------
def _bwd(o, E, ks, g_xq, g_level):
    from gamer_amd import ops
    L, B, D = o["r_levels"].shape
    dz, dE = torch.full((B, D), 777.0, device=DEV), torch.full_like(E, 777.0)
    ops.rvq_bwd(o["idx"], o["r_levels"], E, _offsets(ks), g_xq, g_level, MU, dz, dE)
    torch.cuda.synchronize()
    return dz, dE


def _autograd(r, E, ks, idx, g_xq, g_level, dtype):
    """(dz, dE) of sum_l g_l (mse(e, sg r) + MU mse(sg e, r)) + <g_xq, x_q> through the reference's composition"""
    off = _offsets(ks)
    z = r.to(dtype).clone().requires_grad_(True)
    Ed = E.to(dtype).clone().requires_grad_(True)
    res, xq, loss = z, 0, 0
    for l in range(len(ks)):
        e = Ed[off[l]:off[l + 1]][idx[:, l].long()]
        loss = loss + g_level[l].to(dtype) * (torch.nn.functional.mse_loss(e, res.detach()) + MU * torch.nn.functional.mse_loss(e.detach(), res))
        x_res = res + (e - res).detach()
        res, xq = res - x_res, xq + x_res
    (loss + (g_xq.to(dtype) * xq).sum()).backward()
    return z.grad, Ed.grad


@pytest.mark.parametrize("ks", [[20, 24, 20, 32], [256] * 4], ids=["K20", "K256"])
@pytest.mark.parametrize("D", [8, 32])
@pytest.mark.parametrize("B", [1, 37, 130])
def test_backward_against_fp64_autograd(B, D, ks):
    r, E = _inputs(B, D, ks, 77 * B + D + len(ks))
    g = torch.Generator().manual_seed(B + D)
    g_xq, g_level = torch.randn(B, D, generator=g).to(DEV), (0.5 + torch.rand(len(ks), generator=g)).to(DEV)
    o = _fwd(r, E, ks)
    dz, dE = _bwd(o, E, ks, g_xq, g_level)
    dz64, dE64 = _autograd(r, E, ks, o["idx"], g_xq, g_level, torch.float64)
    dz32, dE32 = _autograd(r, E, ks, o["idx"], g_xq, g_level, torch.float32)
    for name, got, ref, t32 in (("dz", dz, dz64, dz32), ("dE", dE, dE64, dE32)):
        e, t = _err(got, ref), _err(t32, ref)
        print(f"B={B} D={D} K={ks[0]}: {name} kernel {e:.3e} torch {t:.3e}")
        _note("bwd_" + name, e, t)
        assert e <= _bar(t), (name, e, t)
    chosen = torch.zeros(sum(ks), dtype=torch.bool, device=DEV)
    for l in range(len(ks)):
        chosen[_offsets(ks)[l] + o["idx"][:, l].long()] = True
    assert bool((dE[~chosen] == 0).all()) and bool((dE[chosen].abs().amax(1) > 0).all())
    dz_b, dE_b = _bwd(o, E, ks, g_xq, g_level)
    assert torch.equal(dz_b, dz) and torch.equal(dE_b, dE)
    # without an upstream gradient of x_q
    dz0, dE0 = _bwd(o, E, ks, None, g_level)
    none = torch.zeros_like(g_xq)
    ref0, t0 = _autograd(r, E, ks, o["idx"], none, g_level, torch.float64)[0], _autograd(r, E, ks, o["idx"], none, g_level, torch.float32)[0]
    assert torch.equal(dE0, dE) and _err(dz0, ref0) <= _bar(_err(t0, ref0))


def test_backward_when_every_row_chooses_one_code():
    ks, B, D = [24, 24], 130, 32
    r, E = _inputs(B, D, ks, 9)
    E[:24] += 100.0
    E[5] = r.mean(0)
    o = _fwd(r, E, ks)
    assert bool((o["idx"][:, 0] == 5).all())
    g_xq, g_level = torch.zeros(B, D, device=DEV), torch.tensor([1.0, 0.5], device=DEV)
    dz, dE = _bwd(o, E, ks, g_xq, g_level)
    dz64, dE64 = _autograd(r, E, ks, o["idx"], g_xq, g_level, torch.float64)
    dz32, dE32 = _autograd(r, E, ks, o["idx"], g_xq, g_level, torch.float32)
    assert _err(dE, dE64) <= _bar(_err(dE32, dE64)) and _err(dz, dz64) <= _bar(_err(dz32, dz64))
    rest = [k for k in range(24) if k != 5]
    assert bool((dE[rest] == 0).all()) and float(dE[5].abs().max()) > 0


def test_a_rows_dz_does_not_depend_on_the_order_of_the_other_rows():
    ks, B, D = [20, 24, 20, 32], 130, 8
    r, E = _inputs(B, D, ks, 10)
    g_xq, g_level = torch.randn(B, D, device=DEV), torch.ones(4, device=DEV)
    perm = torch.randperm(B, device=DEV)
    o, op = _fwd(r, E, ks), _fwd(r[perm].contiguous(), E, ks)
    assert torch.equal(op["idx"], o["idx"][perm]) and torch.equal(op["xq"], o["xq"][perm])
    dz, _ = _bwd(o, E, ks, g_xq, g_level)
    dzp, _ = _bwd(op, E, ks, g_xq[perm].contiguous(), g_level)
    assert torch.equal(dzp, dz[perm])


# ---- the model against the real class ---------------------------------------------------------------------------------------------
def _model(z, meta, cfg, **kw):
    from gamer_amd.rqvae import RQVAE
    c = dict(meta["configs"][cfg])
    c.update(kw)
    m = RQVAE(in_dim=meta["in_dim"], num_emb_list=meta["num_emb_list"], e_dim=meta["e_dim"], layers=meta["layers"],
              cf_embedding=z["cf_embedding"], cluster_backend="sklearn", **c)
    m.load_state_dict({k: torch.from_numpy(z[f"{cfg}/sd/{k}"]) for k in meta[f"{cfg}_keys"]}, strict=True)
    return m.to(DEV)


@pytest.mark.parametrize("cfg", ["a", "b"])
def test_model_matches_the_reference(fx, cfg):
    z, meta = fx
    m = _model(z, meta, cfg).train()
    x = torch.from_numpy(z["x"]).to(DEV)
    labels = json.loads(str(z["labels_json"]))
    random.seed(meta["py_seed"])
    out, rq_loss, indices, x_q = m(x, labels)
    total, cf_loss, recon, quant = m.compute_loss(out, rq_loss, torch.arange(meta["B"]), x_q, xs=x)
    total.backward()
    assert indices.dtype == torch.int64 and torch.equal(indices.cpu(), torch.from_numpy(z[f"{cfg}/indices"]))
    if meta["configs"][cfg]["beta"] > 0:
        assert torch.equal(m.rq.last_positives.cpu(), torch.from_numpy(z[f"{cfg}/positives"]))
    e_out, e_xq = _err(out.detach().cpu(), torch.from_numpy(z[f"{cfg}/out"]).double()), _err(x_q.detach().cpu(), torch.from_numpy(z[f"{cfg}/x_q"]).double())
    _note(f"model_{cfg}_out", max(e_out, e_xq))
    assert e_out < 2e-5 and e_xq < 2e-5, (e_out, e_xq)
    for got, want, name in zip((total, cf_loss, recon, quant), z[f"{cfg}/losses"], meta["loss_order"]):
        if float(want) == 0.0:
            assert float(got.detach()) == 0.0, name
            continue
        e = abs(float(got.detach()) - float(want)) / abs(float(want))
        _note(f"model_{cfg}_loss", e)
        assert e <= 1e-5, (name, float(got), float(want))
    for k, p in m.named_parameters():
        ref = torch.from_numpy(z[f"{cfg}/grad/{k}"]).double()
        assert p.grad is not None and float(ref.abs().max()) > 0, k
        e = _err(p.grad.cpu(), ref)
        _note(f"model_{cfg}_grad", e)
        assert e < 2e-4, (k, e)
    m.eval()
    assert torch.equal(m.get_indices(x, labels, use_sk=False).cpu(), torch.from_numpy(z[f"{cfg}/get_indices"]))
    for q in m.rq.vq_layers[:-1]:
        q.sk_epsilon = 0.0
    if m.rq.vq_layers[-1].sk_epsilon == 0.0:
        m.rq.vq_layers[-1].sk_epsilon = 0.003
    got = m.get_indices(x[meta["group"]], labels, use_sk=True)
    assert torch.equal(got.cpu(), torch.from_numpy(z[f"{cfg}/get_indices_sk_group"]))


def test_kmeans_initialisation_fills_the_codebooks():
    from gamer_amd.rqvae import RQVAE
    torch.manual_seed(0)
    m = RQVAE(in_dim=16, num_emb_list=[256, 256], e_dim=8, layers=[16], sk_epsilons=[0.0, 0.003], kmeans_init=True, alpha=0.0,
              beta=0.0, cluster_backend="sklearn").to(DEV)
    x = torch.randn(600, 16, device=DEV)
    m.eval()
    m.vq_initialization(x)
    w0, w1 = (q.embedding.weight.detach() for q in m.rq.vq_layers)
    assert all(q.initted for q in m.rq.vq_layers) and float(w0.abs().max()) > 0 and float(w1.abs().max()) > 0
    z = m.encoder(x).detach()
    d0 = torch.cdist(z, w0).min(1).values
    assert float(d0.mean()) < float(z.norm(dim=1).mean())                    # the centres lie in the data, not at the origin
    m.train()
    out, rq_loss, idx, _ = m(x, None)
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(rq_loss)) and idx.shape == (600, 2)


# ---- the commands -----------------------------------------------------------------------------------------------------------------
def _items(tmp_path, n, dim, copies, seed):
    g = np.random.default_rng(seed)
    x = g.standard_normal((n, dim)).astype(np.float32)
    src = g.choice(n - copies, copies, replace=False)
    x[n - copies:] = x[src]
    path = str(tmp_path / "items.npy")
    np.save(path, x)
    return path, x, src


def test_tokenising(tmp_path, capsys):
    from gamer_amd import tokenize_items, train_rqvae
    from gamer_amd.rqvae import RQVAE
    path, x, src = _items(tmp_path, 300, 24, 20, 11)
    torch.manual_seed(3)
    model = RQVAE(in_dim=24, num_emb_list=[20, 24, 20, 32], e_dim=8, layers=[32, 16], alpha=0.0, beta=0.0, cluster_backend="none")
    for q in model.rq.vq_layers:
        q.embedding.weight.data.normal_(0.0, 0.05)
    a = train_rqvae.build_parser().parse_args(["--data_path", path, "--ckpt_dir", str(tmp_path / "ck"), "--kmeans_init", "False",
                                               "--beta", "0", "--cluster_backend", "none"])
    ckpt = train_rqvae.Trainer(model, a, train_rqvae.EmbDataset(path), torch.device("cpu")).save_checkpoint(0, 0.5, "best_collision_model.pth")
    out = tokenize_items.main(["--dataset", "Toy", "--data_path", path, "--output_dir", str(tmp_path / "out"), "--ckpt_path", ckpt,
                               "--cluster_backend", "none", "--device", DEV, "--epoch", "2"])
    assert os.path.basename(out) == "Toy.index.epoch2.alpha0.2-beta0.0001.json"
    report = [ln for ln in capsys.readouterr().out.splitlines() if " rounds, collision rate " in ln][-1]
    rounds, final_rate = int(report.split(" rounds")[0].split()[-1]), float(report.split("collision rate ")[1].split(",")[0])
    assert rounds <= tokenize_items.MAX_ROUNDS
    table = json.load(open(out))
    assert sorted(table, key=int) == [str(i) for i in range(300)]
    codes = [table[str(i)] for i in range(300)]
    for c in codes:
        assert len(c) == 4 and all(s.startswith(f"<{p}_") and s.endswith(">") and s[3:-1].isdigit() for s, p in zip(c, "abcd"))
    # the first pass (one batch of at most 1024 items, use_sk=False) against get_indices row by row
    fresh, _ = tokenize_items.load_model(ckpt, 24, torch.device(DEV), "none")
    xd = torch.from_numpy(x).to(DEV)
    first = fresh.get_indices(xd, None, use_sk=False).cpu().numpy()
    rows = torch.cat([fresh.get_indices(xd[i:i + 1], None, use_sk=False) for i in range(300)]).cpu().numpy()
    assert np.array_equal(first, rows)
    rate = lambda strs: 1 - len(set(strs)) / len(strs)                      # noqa: E731
    first_rate = rate([str(c) for c in tokenize_items.codes_of(first)])
    assert abs(rate([str(c) for c in codes]) - final_rate) < 1e-6 and final_rate <= first_rate
    for j, s in enumerate(src):
        assert codes[280 + j] == codes[s]                                   # exact copies keep colliding, as in the reference


@pytest.mark.parametrize("extra", [["--cluster_backend", "sklearn"], ["--cluster_backend", "none", "--beta", "0"]], ids=["sklearn", "none"])
def test_training_two_epochs(tmp_path, extra):
    from gamer_amd import tokenize_items, train_rqvae
    from gamer_amd.rqvae import RQVAE
    path, x, _ = _items(tmp_path, 200, 24, 0, 12)
    tr = train_rqvae.main(["--data_path", path, "--ckpt_dir", str(tmp_path / "ck"), "--epochs", "2", "--eval_step", "1", "--batch_size", "64",
                           "--layers", "32", "16", "--e_dim", "8", "--num_emb_list", "20", "24", "20", "32", "--kmeans_init", "False",
                           "--device", DEV, "--cf_emb", str(tmp_path / "none.pt")] + extra)
    assert all(np.isfinite(v) for v in tr.last_losses) and np.isfinite(tr.best_loss)
    assert 0.0 <= tr.last_collision_rate <= 1.0 and 0.0 <= tr.best_collision_rate <= 1.0
    names = sorted(os.path.basename(p) for p in set(tr.saved))
    assert "best_collision_model.pth" in names and any(n.startswith("epoch_1_collision_") for n in names)
    last = [p for p in tr.saved if os.path.basename(p).startswith("epoch_1_")][0]
    ck = torch.load(last, map_location="cpu", weights_only=False)
    assert list(ck) == ["args", "epoch", "best_loss", "best_collision_rate", "state_dict", "optimizer"]
    assert isinstance(ck["args"], argparse.Namespace) and ck["epoch"] == 1
    a = ck["args"]
    m = RQVAE(in_dim=a.in_dim, num_emb_list=a.num_emb_list, e_dim=a.e_dim, layers=a.layers, kmeans_init=False, sk_epsilons=a.sk_epsilons,
              sk_iters=a.sk_iters, alpha=a.alpha, beta=a.beta, cluster_backend="sklearn")
    m.load_state_dict(ck["state_dict"], strict=True)
    m = m.to(DEV).eval()
    xd = torch.from_numpy(x).to(DEV)
    tr.model.eval()
    want = tr.model.get_indices(xd, tr.labels)
    assert torch.equal(m.get_indices(xd, tr.labels), want)
    m2, _ = tokenize_items.load_model(last, 24, torch.device(DEV), "none")
    assert torch.equal(m2.get_indices(xd, None), want)
