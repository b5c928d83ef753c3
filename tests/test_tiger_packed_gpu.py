"""TIGER on packed rows (no padding tokens) on the GPU: the packed entry points of both T5 attention families
(gamer_t5_attn_packed_* and gamer_t5_attn_long_packed_*) against the fp64 restatement AND against the dense entry points run with
the right-padding key mask of the same lengths, their invariants, refusals and memory; then ``TIGER.forward(packed=True)``, beam
search and the train commands' ``--pack_rows`` against the fixtures of the real class that the padded run is tested on.

Bars (the project's rule, tests/test_tiger_gpu.py and tests/test_tiger_long_gpu.py).  Attention: every case of the grid also runs
the restatement as fp32 torch ops on the GPU; per quantity the packed kernel may err against fp64 by at most twice the
restatement's worst relative error over this file's grid, and never by more than 1e-4; the packed-against-dense difference, on the
same scale, gets the same bar.  Model: per fixture, twice the worst error of the fp32 torch restatement of the whole model against
the fixture, never above 1e-3, for the packed run against the fixture and for the packed run against the padded run.  Relative
error = largest absolute difference over the largest reference magnitude of the tensor, on the real rows."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import t5_attention_ref as ref  # noqa: E402
import t5_packed_ref as pref  # noqa: E402
import tiger_weights as tw  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
DEV = ref.DEV


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("needs the GPU")
    from gamer_amd import build
    build.build()


def _fixture(name):
    z = np.load(os.path.join(GOLDEN, name))
    return z, json.loads(str(z["meta_json"]))


@pytest.fixture(scope="module")
def small():
    return _fixture("tiger_small.npz")


@pytest.fixture(scope="module")
def long_fx():
    return _fixture("tiger_long.npz")


@pytest.fixture(scope="module")
def smb_fx():
    return _fixture("tiger_smb.npz")


# ---- the kernel grid ---------------------------------------------------------------------------------------------------------------------
RESIDENT = ([23, 9, 17, 1, 12], [16, 128, 127, 15])                  # a 16-tile edge inside a row, a one-token row; exact tiles, the bound
LONG = ([300, 129, 512, 1], [130, 257, 64, 65])                       # the edges of the 64-key blocks
ZERO = {False: [9, 0, 17], True: [130, 0, 70]}                        # a row of length 0 between two others


def _grid():
    """dropout 0.1 on every other case"""
    cases = []
    for lens in RESIDENT:
        for h in (1, 6):
            for d in (32, 64):
                for causal in (False, True):
                    cases.append(dict(long=False, lens=lens, h=h, d=d, bias=True, causal=causal))
    for h, d in ((1, 32), (6, 64)):
        cases.append(dict(long=False, lens=[101, 1, 37], h=h, d=d, bias=False, causal=False, Sd=5))
    for lens in LONG:
        for h, d in ((1, 32), (6, 64)):
            for causal in (False, True):
                cases.append(dict(long=True, lens=lens, h=h, d=d, bias=True, causal=causal))
    for h, d in ((1, 32), (6, 64)):
        cases.append(dict(long=True, lens=[300, 1, 129], h=h, d=d, bias=False, causal=False, Sd=5))   # Sq <= 16: the split-key path
    for long in (False, True):
        cases.append(dict(long=long, lens=ZERO[long], h=2, d=32, bias=True, causal=False))
        cases.append(dict(long=long, lens=ZERO[long], h=2, d=64, bias=False, causal=False, Sd=5))
    for n, c in enumerate(cases):
        c["p"] = 0.1 if n % 2 else 0.0
    return cases


@pytest.fixture(scope="module")
def grid():
    return pref.grid_errors(_grid())


def _live(rows):
    return [r for r in rows if r[3] > 1e-12 * max(r[5], 1e-30)]


@pytest.mark.parametrize("quantity", pref.QUANTITIES)
def test_packed_attention_against_fp64_and_against_the_dense_kernels(grid, quantity):
    rows = grid[quantity]
    assert len(rows) == (26 if quantity in ("drel", "dtable") else 32)
    live = _live(rows)
    worst = max(r[2] for r in live)
    print(f"{quantity}: packed {max(r[1] for r in live):.3e}  fp32 torch {worst:.3e}  packed against dense {max(r[6] for r in live):.3e}  "
          f"({len(live)} of {len(rows)} cases)")
    for c, ek, et, mag, gotmag, gmax, against in rows:
        if mag > 1e-12 * max(gmax, 1e-30):
            assert ek <= 2.0 * worst and ek <= 1e-4, (quantity, c, ek, worst)
            assert against <= 2.0 * worst and against <= 1e-4, (quantity, c, against, worst)
        else:
            # zero in exact arithmetic (one allowed key in every row): rounding residue, held to 1e-4 of the largest input gradient
            assert gotmag <= 1e-4 * gmax, (quantity, c, gotmag, gmax)


def test_the_grid_covers_both_families_and_dropout():
    cases = _grid()
    for long in (False, True):
        mine = [c for c in cases if c["long"] == long]
        assert {c["p"] for c in mine} == {0.0, 0.1} and {c["causal"] for c in mine} == {True, False}
        assert any(c.get("Sd") for c in mine) and any(0 in c["lens"] for c in mine)
        assert {(c["h"], c["d"]) for c in mine} >= {(1, 32), (6, 64)}
        assert max(max(c["lens"]) for c in mine) == (512 if long else 128)


@pytest.mark.parametrize("long", [False, True])
def test_a_row_of_length_zero(long):
    """self attention: the row has no queries and no keys, so its key-side gradients are absent; cross attention: its dense query
    rows give zeros and -inf, and zero gradients"""
    lens = ZERO[long]
    got, dn, truth, _ = pref.case(long, lens, 2, 32, True, False, 0.0, torch32=False)
    assert got["dk"].shape[0] == got["o"].shape[0] == sum(lens)
    got, dn, truth, _ = pref.case(long, lens, 2, 64, False, False, 0.0, Sd=5, torch32=False)
    o, dq, lse = got["o"].view(3, 5, -1), got["dq"].view(3, 5, -1), got["lse"].view(2, 3, 5)
    assert float(o[1].abs().max()) == 0.0 and float(dq[1].abs().max()) == 0.0
    assert bool(torch.isinf(lse[:, 1]).all()) and bool((lse[:, 1] < 0).all()) and bool(torch.isfinite(lse[:, 0]).all())
    assert got["dk"].shape[0] == sum(lens)
    for k in truth:
        assert ref.rel_err(got[k], truth[k]) < 1e-4, k


@pytest.mark.parametrize("kw", [dict(long=False, lens=[23, 9, 17, 1, 12], h=6, d=64, bias=True, causal=False),
                                dict(long=False, lens=[101, 1, 37], h=2, d=32, bias=False, causal=False, Sd=5),
                                dict(long=True, lens=[130, 257, 64, 65], h=6, d=64, bias=True, causal=False),
                                dict(long=True, lens=[300, 1, 129], h=2, d=32, bias=True, causal=True)])
def test_two_calls_bit_identical_with_dropout(kw):
    a = pref.case(p=0.1, truth=False, dense=False, **kw)[0]
    b = pref.case(p=0.1, truth=False, dense=False, **kw)[0]
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("long,lens,h,d,causal", [(False, [23, 9, 17, 1, 12], 2, 32, False), (False, [16, 128, 127, 15], 6, 64, True),
                                                   (True, [300, 129, 512, 1], 2, 32, False), (True, [130, 257, 64, 65], 6, 64, True)])
def test_rows_are_independent(long, lens, h, d, causal):
    """row 2 alone gives the bits that it gives among its neighbours, whatever their lengths and offsets"""
    full = pref.case(long, lens, h, d, True, causal, 0.0, truth=False, dense=False)[0]
    one = pref.case(long, lens, h, d, True, causal, 0.0, rows=[2], max_s=max(lens), truth=False, dense=False)[0]
    a, n = sum(lens[:2]), lens[2]
    for k in ("o", "dq", "dk", "dv"):
        assert torch.equal(one[k], full[k][a:a + n]), k
    assert torch.equal(one["lse"], full["lse"][:, a:a + n])


@pytest.mark.parametrize("long", [False, True])
@pytest.mark.parametrize("B,n_slab", [(7, 3), (7, 1), (5, 5)])
def test_backward_walks_several_rows_per_workgroup(long, B, n_slab):
    """fewer slabs than rows: workgroup (slot, head) walks the rows slot, slot + n_slab, ... and writes its slab once, in full"""
    lens = ([130, 70, 257, 1, 64, 200, 129] if long else [23, 9, 128, 1, 16, 100, 17])[:B]
    got, _, truth, _ = pref.case(long, lens, 2, 64, True, False, 0.1, n_slab=n_slab, torch32=False, dense=False)
    assert got["slabs"].shape[1] == n_slab and not bool(torch.isnan(got["slabs"]).any())
    for k in truth:
        assert ref.rel_err(got[k], truth[k]) < 1e-4, (k, ref.rel_err(got[k], truth[k]))


def test_beam_rows_read_their_users_packed_keys():
    from gamer_amd import ops
    users, beams, Sq, h, d = 3, 4, 5, 6, 64
    lens = [300, 5, 129]
    I, N, Sk = h * d, users * beams, max(lens)
    g = torch.Generator().manual_seed(11)
    q = (torch.randn(N * Sq, I, generator=g) * (10.0 / d) ** 0.5).to(DEV)
    kv = torch.randn(sum(lens), 2 * I, generator=g).to(DEV)
    k_off, q_off = ops.T5Offsets.from_lengths(torch.tensor(lens), DEV), ops.T5Offsets.uniform(N, Sq, DEV)
    rows = torch.arange(users, dtype=torch.int32).repeat_interleave(beams).to(DEV)
    o1, l1 = torch.full((N * Sq, I), float("nan"), device=DEV), torch.full((h, N * Sq), float("nan"), device=DEV)
    ops.t5_attn_long_packed_fwd(q, kv[:, :I], kv[:, I:], None, q_off, k_off, N, Sq, Sk, h, d, False, 0.0, 0, o1, l1, kv_rows=rows,
                                kv_batch=users)
    # every beam with its own copy of its user's keys
    parts = torch.split(kv, lens)
    kvr = torch.cat([parts[u] for u in rows.tolist()]).contiguous()
    r_off = ops.T5Offsets.from_lengths(torch.tensor([lens[u] for u in rows.tolist()]), DEV)
    o2, l2 = torch.empty_like(o1), torch.empty_like(l1)
    ops.t5_attn_long_packed_fwd(q, kvr[:, :I], kvr[:, I:], None, q_off, r_off, N, Sq, Sk, h, d, False, 0.0, 0, o2, l2)
    assert torch.equal(o1, o2) and torch.equal(l1, l2) and bool(torch.isfinite(o1).all()) and bool(torch.isfinite(l1).all())


def test_refusals_leave_the_outputs_untouched():
    from gamer_amd import _lib, ops
    t = torch.full((1024, 64), 7.0, device=DEV)
    lse = torch.full((2, 1, 1024), 7.0, device=DEV)
    p, lp = t.data_ptr(), lse.data_ptr()
    good = ops.T5Offsets.from_lengths(torch.tensor([8, 3]), DEV)
    host = lambda *v: torch.tensor(v, dtype=torch.int32)

    def both(q_host, max_s=(8, 8), h=1, d=64, ldq=64, match="", long=(False, True)):
        for lg in long:
            stem = "gamer_t5_attn_long_packed_" if lg else "gamer_t5_attn_packed_"
            off = (good.dev.data_ptr(), good.dev.data_ptr(), q_host.data_ptr(), q_host.data_ptr())
            with pytest.raises(RuntimeError, match=match):
                _lib.call(stem + "fwd", p, ldq, p, 64, p, 64, None, *off, None, 2, 0, *max_s, h, d, 0, 0.0, 0, p, 64, lp, ops.stream_ptr())
            with pytest.raises(RuntimeError, match=match):
                _lib.call(stem + "bwd", p, ldq, p, 64, p, 64, None, *off, 2, *max_s, h, d, 0, 0.0, 0, p, 64, lp, p, 64, p, 64, p, 64, None, 1,
                          *((lp,) if lg else ()), ops.stream_ptr())
    both(host(1, 8, 11), match="start at 0")
    both(host(0, 8, 5), match="decreases")
    both(host(0, 9, 11), match="more than max")
    both(host(0, 0, 0), match="no token")
    both(good.host, max_s=(129, 8), match="bad shape", long=(False,))
    both(good.host, max_s=(8, 513), match="bad shape", long=(True,))
    both(good.host, h=17, match="bad shape")
    both(good.host, d=48, match="bad shape")
    both(good.host, ldq=66, match="leading dims")
    # the wrappers refuse the same before the library is touched
    with pytest.raises(ValueError, match="decrease"):
        ops.T5Offsets(host(0, 8, 5), DEV)
    with pytest.raises(ValueError, match="more than max"):
        ops.t5_attn_packed_fwd(t[:11], t[:11], t[:11], None, good, good, 2, 7, 7, 1, 64, False, 0.0, 0, t[:11], lse.view(-1)[:11])
    with pytest.raises(NotImplementedError):
        ops.t5_attn_packed_fwd(t[:11], t[:11], t[:11], None, good, good, 2, 129, 129, 1, 64, False, 0.0, 0, t[:11], lse.view(-1)[:11])
    torch.cuda.synchronize()
    assert bool((t == 7.0).all()) and bool((lse == 7.0).all())


def test_packed_attention_takes_less_temporary_memory_than_the_dense_call():
    """64 rows of mean length 200 at max_s 512 against the dense call on [64, 512]: the only temporaries are the long backward's row
    terms, 2 h Tq floats against 2 B h S"""
    from gamer_amd import ops
    B, S, h, d = 64, 512, 6, 64
    I = h * d
    g = torch.Generator().manual_seed(5)
    lens = torch.randint(1, 400, (B,), generator=g)
    lens[0] = S
    lens = (lens.float() * (200.0 * B / float(lens.sum()))).long().clamp(1, S)
    off = ops.T5Offsets.from_lengths(lens, DEV)
    assert abs(off.total / B - 200) < 8
    rel = torch.randn(h, 2 * S - 1, device=DEV)

    def extra(T, run):
        qkv = torch.randn(T, 3 * I, device=DEV) * 0.3
        dqkv, o, d_o, lse = torch.empty_like(qkv), torch.empty(T, I, device=DEV), torch.randn(T, I, device=DEV), torch.empty(h * T, device=DEV)
        slabs = torch.empty(ops.t5_n_slab(B, h), h, 2 * S - 1, device=DEV)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        run((qkv[:, :I], qkv[:, I:2 * I], qkv[:, 2 * I:]), o, lse, d_o, (dqkv[:, :I], dqkv[:, I:2 * I], dqkv[:, 2 * I:]), slabs)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base                  # (read before the checks below allocate anything)
        assert bool(torch.isfinite(dqkv).all()) and bool(torch.isfinite(slabs).all()) and bool(torch.isfinite(o).all())
        return peak

    def packed(qkv, o, lse, d_o, dqkv, slabs):
        ops.t5_attn_long_packed_fwd(*qkv, rel, off, off, B, S, S, h, d, False, 0.1, 3, o, lse)
        ops.t5_attn_long_packed_bwd(*qkv, rel, off, off, B, S, S, h, d, False, 0.1, 3, d_o, lse, *dqkv, slabs)

    def dense(qkv, o, lse, d_o, dqkv, slabs):
        ops.t5_attn_long_fwd(*qkv, rel, None, B, S, S, h, d, False, 0.1, 3, o, lse)
        ops.t5_attn_long_bwd(*qkv, rel, None, B, S, S, h, d, False, 0.1, 3, d_o, lse, *dqkv, slabs)
    ep, ed = extra(off.total, packed), extra(B * S, dense)
    print(f"temporaries: packed {ep / 1e6:.2f} MB, dense {ed / 1e6:.2f} MB")
    assert ep < ed, (ep, ed)


# ---- the model against the real class, from the fixtures of the padded run ------------------------------------------------------------
def _batch(z, tag):
    return (torch.from_numpy(z[f"{tag}/{k}"].astype(np.int64)) for k in ("input_ids", "attention_mask", "labels"))


def _step(m, ids, am, labels, **kw):
    m.train()                                                           # (dropout_rate 0: the training path, CatalogCEFn and all)
    for p in m.parameters():
        p.grad = None
    loss, logits = m(ids.to(DEV), am.to(DEV), labels=labels.to(DEV), want_logits=True, **kw)
    loss.backward()
    return loss.detach().clone(), logits, {k: p.grad.clone() for k, p in m.named_parameters()}


def _model_errors(fx, name, tag):
    """(packed against the fixture, fp32 torch against the fixture, packed against padded), per quantity"""
    z, meta = fx
    m, sd = ref.load_model(z, meta, name)
    ids, am, labels = _batch(z, tag)
    lens = am.sum(1)
    loss, logits, grads = _step(m, ids, am, labels, packed=True, lengths=lens)
    d_loss, d_logits, d_grads = _step(m, ids, am, labels)
    m_loss, m_logits, m_grads = _step(m, ids, am, labels, packed=True)            # the lengths read from the mask: the same bits
    assert torch.equal(m_loss, loss) and torch.equal(m_logits, logits) and all(torch.equal(m_grads[k], grads[k]) for k in grads)
    r_loss, r_logits, r_grads = ref.restated_model(sd, meta["configs"][name], ids, am, labels, meta["temperature"])
    assert set(grads) == set(meta[name]["param_keys"])
    kernel, torch32, against = {}, {}, {}
    smb = f"{tag}/logit_cols" in z.files
    if smb:                                                             # the labelled rows at the fixture's columns
        cols, on = torch.from_numpy(z[f"{tag}/logit_cols"]).to(DEV), (labels != -100).to(DEV)
        want, want_sumsq = z[f"{tag}/logits"], float(z[f"{tag}/logits_sumsq"])
        for out, lg in ((kernel, logits), (torch32, r_logits)):
            out["logits"] = ref.rel_err(lg[on][:, cols], want)
            out["sumsq/logits"] = 0.5 * abs(float((lg[on].double() ** 2).sum()) - want_sumsq) / want_sumsq
        against["logits"] = ref.rel_err(logits[on], d_logits[on])
    else:
        kernel["logits"], torch32["logits"] = ref.rel_err(logits, z[f"{tag}/logits"]), ref.rel_err(r_logits, z[f"{tag}/logits"])
        against["logits"] = ref.rel_err(logits, d_logits)
    ref_loss = float(z[f"{tag}/loss"])
    kernel["loss"], torch32["loss"] = abs(float(loss) - ref_loss) / abs(ref_loss), abs(float(r_loss) - ref_loss) / abs(ref_loss)
    against["loss"] = abs(float(loss) - float(d_loss)) / abs(float(d_loss))
    for k, gk in grads.items():
        want_rows = torch.from_numpy(z[f"{tag}/grad/{k}"])
        rows = torch.from_numpy(z[f"{tag}/table_rows"]) if smb and k == "shared.weight" else tw.sample_rows(gk.shape)
        kernel[k], torch32[k] = ref.rel_err(gk[rows.to(DEV)], want_rows), ref.rel_err(r_grads[k][rows.to(DEV)], want_rows)
        want = float(z[f"{tag}/grad_checksum/{k}"][1])
        kernel["sumsq/" + k] = 0.5 * abs(float(tw.checksums({k: gk.cpu()})[0][1]) - want) / want
        torch32["sumsq/" + k] = 0.5 * abs(float(tw.checksums({k: r_grads[k].cpu()})[0][1]) - want) / want
        against[k] = ref.rel_err(gk, d_grads[k])
    return kernel, torch32, against


@pytest.mark.parametrize("which,name,tag", [("small", "a", "a"), ("long", "c", "c"), ("long", "d", "d"), ("smb", "s", "s/short"),
                                            ("smb", "s", "s/long")])
def test_packed_model_matches_the_reference_and_the_padded_run(small, long_fx, smb_fx, which, name, tag):
    """a: rows of 23, 9, 17, 1 and 12 tokens; c: 300, 129, 512 and 1 in one batch; d: 257 / 200 at 6 heads of 32; the SMB batches of
    1 .. 126 tokens (resident family) and 1, 6, 131, 151 (key-streaming family)"""
    fx = dict(small=small, long=long_fx, smb=smb_fx)[which]
    kernel, torch32, against = _model_errors(fx, name, tag)
    bar = min(2.0 * max(torch32.values()), 1e-3)
    worst, wa = max(kernel, key=kernel.get), max(against, key=against.get)
    print(f"{tag}: packed worst {kernel[worst]:.3e} ({worst}), logits {kernel['logits']:.3e}, loss {kernel['loss']:.3e}; packed against "
          f"padded worst {against[wa]:.3e} ({wa}); fp32 torch worst {max(torch32.values()):.3e}; bar {bar:.3e}")
    for k, e in kernel.items():
        assert e <= bar, (k, e, bar)
    for k, e in against.items():
        assert e <= bar, ("against padded", k, e, bar)


def test_encode_packed_returns_the_real_rows_and_their_offsets(small):
    z, meta = small
    m, _ = ref.load_model(z, meta, "a")
    m.eval()
    ids, am, _ = _batch(z, "a")
    with torch.no_grad():
        enc, pack = m.encode(ids.to(DEV), am.to(DEV), packed=True)
        dense, keep = m.encode(ids.to(DEV), am.to(DEV))
    lens = am.sum(1)
    assert pack.off.host.tolist() == [0] + lens.cumsum(0).tolist() and enc.shape == (int(lens.sum()), dense.shape[2])
    assert ref.rel_err(enc, dense[keep.bool()]) < 1e-5


def test_a_mask_that_is_not_right_padded_is_refused(small):
    z, meta = small
    m, _ = ref.load_model(z, meta, "a")
    ids, am, labels = _batch(z, "a")
    left = torch.flip(am, [1])
    assert not torch.equal(left, am)
    with pytest.raises(ValueError, match="row 1"):
        m(ids.to(DEV), left.to(DEV), labels=labels.to(DEV), packed=True)


@pytest.mark.parametrize("nb", [4, 20])
@pytest.mark.parametrize("which,tag", [("small", "a"), ("small", "a/prefix"), ("long", "c")])
def test_packed_beam_search_finds_generates_beams(small, long_fx, which, tag, nb):
    from gamer_amd import tiger
    from gamer_amd.decode import ItemTrie
    z, meta = small if which == "small" else long_fx
    name, kind = tag[0], "prefix" if tag.endswith("prefix") else "plain"
    m, _ = ref.load_model(z, meta, name)
    ids, am, _ = _batch(z, name)
    ids, am = ids[:3].to(DEV), am[:3].to(DEV)
    trie = ItemTrie(z[f"{name}/trie_{kind}"].tolist(), device=DEV, pad_token_id=0)
    prefix = torch.from_numpy(z[f"{name}/prefix_{kind}"]) if kind == "prefix" else None
    steps = z[f"{name}/beams_{kind}_{nb}"].shape[1] - (prefix.shape[1] if prefix is not None else 1)
    seqs, scores = tiger.beam_search(m, ids, am, trie, nb, steps, decoder_prefix=prefix, packed=True)
    assert torch.equal(seqs.cpu(), torch.from_numpy(z[f"{name}/beams_{kind}_{nb}"]))
    assert ref.rel_err(scores, torch.from_numpy(z[f"{name}/scores_{kind}_{nb}"])) < 1e-3
    # the lengths from the host, one user alone: the same beams
    one_s, one_sc = tiger.beam_search(m, ids[1:2], am[1:2], trie, nb, steps, decoder_prefix=None if prefix is None else prefix[1:2],
                                      packed=True, lengths=am[1:2].sum(1).cpu())
    assert torch.equal(one_s, seqs[nb:2 * nb]) and torch.allclose(one_sc, scores[nb:2 * nb], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("nb", [4, 20])
def test_packed_beam_search_per_behaviour_finds_generates_beams(smb_fx, tmp_path, nb):
    from gamer_amd import synthetic, t5_mb_data, tiger
    from gamer_amd.decode import ItemTrie
    z, meta = smb_fx
    synthetic.write_smb_dataset(str(tmp_path), meta["smb"]["name"], **meta["smb"]["kw"])
    smb = t5_mb_data.T5SMBData(str(tmp_path), meta["smb"]["name"], "smb_explicit")
    m, _ = ref.load_model(z, meta, "s")
    base = smb.samples("test", meta["max_his_len"])
    coll = t5_mb_data.EncDecCollator(1024, smb.token_count)
    for b in meta["beam_behaviors"]:
        rec = meta["s"]["beams"][b]
        inputs, _ = coll.test(base.filter_by_behavior(b), rec["users"])
        lens = tiger.packed_lengths(inputs["attention_mask"])
        assert lens.tolist() == rec["enc_lens"]
        trie = ItemTrie(smb.trie_sequences(b, 0), device=DEV, pad_token_id=0)
        prefix = torch.tensor([0, smb.behavior_token_ids[b]])
        seqs, scores = tiger.beam_search(m, inputs["input_ids"].to(DEV), inputs["attention_mask"].to(DEV), trie, nb, smb.sole_item_len,
                                         decoder_prefix=prefix, packed=True, lengths=lens)
        assert torch.equal(seqs.cpu(), torch.from_numpy(z[f"s/beams/{b}/{nb}"]).long()), (b, nb)
        assert ref.rel_err(scores, torch.from_numpy(z[f"s/scores/{b}/{nb}"])) < 1e-3


def test_packed_dropout_is_repeatable_from_the_seed_counters(small):
    from gamer_amd import modules, rec_common
    z, meta = small
    m, _ = ref.load_model(z, meta, "a", dropout=0.1)
    m.train()
    ids, am, labels = (t.to(DEV) for t in _batch(z, "a"))

    def run(seed):
        modules._SeedCounter.value, rec_common._Seeds.value = 1000 + seed, 2000 + seed
        for p in m.parameters():
            p.grad = None
        loss, _ = m(ids, am, labels=labels, packed=True)
        loss.backward()
        return loss.detach().clone(), [p.grad.clone() for p in m.parameters()]
    l1, g1 = run(0)
    l2, g2 = run(0)
    l3, _ = run(1)
    assert torch.equal(l1, l2) and all(torch.equal(a, b) for a, b in zip(g1, g2))
    assert not torch.equal(l1, l3) and abs(float(l1) - float(z["a/loss"])) > 1e-4
    assert all(bool(torch.isfinite(g).all()) for g in g1)


def test_train_tiger_smb_pack_rows_end_to_end(smb_fx, tmp_path, capsys, monkeypatch):
    """histories of up to 30 items = 151 tokens: the key-streaming family; the checkpoint tested with and without the flag gives the
    same result rows"""
    from gamer_amd import synthetic, train_tiger_smb
    _, meta = smb_fx
    root = tmp_path / "data"
    synthetic.write_smb_dataset(str(root), "Toy", **meta["smb"]["kw"])
    base = tmp_path / "base"
    base.mkdir()
    (base / "config.json").write_text(json.dumps(dict(d_model=64, d_kv=64, d_ff=128, num_layers=2, num_decoder_layers=2, num_heads=2,
                                                      dropout_rate=0.1, vocab_size=32128)))
    out = tmp_path / "ckpt"
    common = ["--base_model", str(base), "--data_path", str(root), "--dataset", "Toy", "--tasks", "smb_explicit", "--max_his_len", "30",
              "--output_dir", str(out), "--per_device_batch_size", "32", "--gradient_accumulation_steps", "1", "--test_batch_size", "16",
              "--num_beams", "10", "--metrics", "hit@1,hit@5,ndcg@5", "--results_file", str(tmp_path / "res.json")]
    seen = []
    from gamer_amd import tiger
    real = tiger.PackedRows.build
    monkeypatch.setattr(tiger.PackedRows, "build", classmethod(lambda cls, lengths, B, S, device: (seen.append(S), real(lengths, B, S, device))[1]))
    res = train_tiger_smb.main(common + ["--pack_rows", "--epochs", "2", "--learning_rate", "3e-3", "--warmup_ratio", "0.0"])
    log = capsys.readouterr().out
    packed = train_tiger_smb.main(common + ["--only_test", "--pack_rows"])
    n_packed = len(seen)
    padded = train_tiger_smb.main(common + ["--only_test"])
    rows = [l for l in log.splitlines() if l.startswith("[train_tiger_smb] epoch ")]
    train = [float(l.split(" loss ")[1].split()[0]) for l in rows]
    assert len(train) == 2 and all(np.isfinite(train)) and train[1] < train[0], train
    assert max(seen) > 128 and len(seen) == n_packed                  # the long family ran packed; the run without the flag never packs
    assert res == packed == padded
