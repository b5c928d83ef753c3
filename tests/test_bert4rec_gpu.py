"""BERT4Rec's kernels and model on the GPU: the biased catalogue head (CE, top K) against fp64 torch, the cloze-mask kernel
against a torch restatement of its rule fed with the kernel's own hash words, and the model against the real reference class
(tests/golden/bert4rec_small.npz, tools/make_golden_bert4rec.py)."""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import bert4rec_weights as bw  # noqa: E402

pytestmark = pytest.mark.gpu
FX = os.path.join(os.path.dirname(__file__), "golden", "bert4rec_small.npz")
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("needs the GPU")
    from gamer_amd import build
    build.build()


def _rel(got, ref):
    got, ref = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(ref).detach().double().cpu()
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


# ---- the biased head ---------------------------------------------------------------------------------------------------------
def _ce_case(V, R, H, seed):
    """E has V + 1 rows, the last filled with 1e30: the kernels score rows [0, V) only, so it must not move any result."""
    from gamer_amd import ops
    g = torch.Generator().manual_seed(seed)
    n_rows = 2 * R + 3
    hfull = torch.randn(n_rows, H, generator=g, dtype=torch.float64) * 0.3
    E = torch.randn(V + 1, H, generator=g, dtype=torch.float64) * 0.5
    E[V] = 1e30
    bias = torch.randn(V, generator=g, dtype=torch.float64)                     # of order 1
    rows = torch.randperm(n_rows, generator=g)[:R].to(torch.int64)
    tgt = torch.randint(0, V, (R,), generator=g)
    hd, Ed, bd = hfull.float().to(DEV), E.float().to(DEV).contiguous(), bias.float().to(DEV)
    rows_d, tgt_d = rows.to(DEV), tgt.to(DEV)
    lse, loss = torch.empty(R, device=DEV), torch.empty((), device=DEV)
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.catalog_ce_bias_fwd(hd, rows_d, Ed, bd, tgt_d, lse, loss, bad, V=V)
    dE, dh = torch.zeros_like(Ed), torch.zeros_like(hd)
    dbias = torch.full((V,), 7.0, device=DEV)                                   # written, not accumulated
    dl = torch.full((), 1.5, device=DEV)
    ops.catalog_ce_bias_bwd(hd, rows_d, Ed, bd, tgt_d, lse, dl, 1.0 / R, dE=dE, dh=dh, dbias=dbias, V=V)
    torch.cuda.synchronize()
    h64 = hd.double().cpu()[rows].requires_grad_(True)
    E64 = Ed.double().cpu()[:V].requires_grad_(True)
    b64 = bd.double().cpu().requires_grad_(True)
    logits = h64 @ E64.t() + b64
    ref_loss = torch.nn.functional.cross_entropy(logits, tgt)
    (1.5 * ref_loss).backward()
    ref_dh = torch.zeros(n_rows, H, dtype=torch.float64)
    ref_dh[rows] = h64.grad
    return dict(lse=lse, loss=loss, dE=dE, dh=dh, dbias=dbias, bad=bad, ref_lse=torch.logsumexp(logits, 1).detach(),
                ref_loss=ref_loss.detach(), ref_dE=E64.grad, ref_dh=ref_dh, ref_dbias=b64.grad)


@pytest.mark.parametrize("V", [1, 17, 8193, 40009])
@pytest.mark.parametrize("R", [1, 5, 300, 5000])
@pytest.mark.parametrize("H", [64, 128, 256])
def test_biased_ce_against_fp64(V, R, H):
    """the bars of test_sasrec_gpu.py::test_catalog_ce_against_fp64 for the same quantities; dbias at dE's bar"""
    c = _ce_case(V, R, H, seed=V * 7 + R * 3 + H)
    assert int(c["bad"].item()) == 0
    print(f"V={V} R={R} H={H}: loss {abs(float(c['loss']) - float(c['ref_loss'])):.3e} lse {_rel(c['lse'], c['ref_lse']):.3e} "
          f"dE {_rel(c['dE'][:V], c['ref_dE']):.3e} dh {_rel(c['dh'], c['ref_dh']):.3e} dbias {_rel(c['dbias'], c['ref_dbias']):.3e}")
    assert abs(float(c["loss"]) - float(c["ref_loss"])) <= 1e-6 * max(1.0, abs(float(c["ref_loss"])))
    assert _rel(c["lse"], c["ref_lse"]) < 1e-6
    assert _rel(c["dE"][:V], c["ref_dE"]) < 1e-5
    assert float(c["dE"][V].abs().sum()) == 0                                   # the row past V gets nothing
    assert _rel(c["dh"], c["ref_dh"]) < 1e-5
    assert _rel(c["dbias"], c["ref_dbias"]) < 1e-5


def test_biased_ce_two_calls_bit_identical():
    a, b = _ce_case(8193, 300, 128, seed=1), _ce_case(8193, 300, 128, seed=1)
    for k in ("lse", "loss", "dE", "dh", "dbias"):
        assert torch.equal(a[k], b[k]), k


def test_bias_gradient_alone_and_without_it():
    """any of dE / dh / dbias may be left out: what is asked for has the bits of the full call"""
    from gamer_amd import ops
    g = torch.Generator().manual_seed(6)
    R, V, H = 130, 1000, 64
    h, E = (torch.randn(R, H, generator=g) * 0.3).to(DEV), (torch.randn(V + 1, H, generator=g) * 0.5).to(DEV)
    bias, tgt = torch.randn(V, generator=g).to(DEV), torch.randint(0, V, (R,), generator=g).to(DEV)
    lse, loss, bad = torch.empty(R, device=DEV), torch.empty((), device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.catalog_ce_bias_fwd(h, None, E, bias, tgt, lse, loss, bad, V=V)
    dE, dh, db = torch.zeros_like(E), torch.zeros_like(h), torch.empty(V, device=DEV)
    ops.catalog_ce_bias_bwd(h, None, E, bias, tgt, lse, None, 1.0 / R, dE=dE, dh=dh, dbias=db, V=V)
    db_only = torch.empty(V, device=DEV)
    ops.catalog_ce_bias_bwd(h, None, E, bias, tgt, lse, None, 1.0 / R, dbias=db_only, V=V)
    dE2, dh2 = torch.zeros_like(E), torch.zeros_like(h)
    ops.catalog_ce_bias_bwd(h, None, E, bias, tgt, lse, None, 1.0 / R, dE=dE2, dh=dh2, V=V)
    assert torch.equal(db, db_only) and torch.equal(dE, dE2) and torch.equal(dh, dh2)
    assert abs(float(db.sum())) < 1e-5                                          # the rows of softmax - onehot sum to zero


@pytest.mark.parametrize("V,R,H", [(17, 5, 64), (8193, 300, 128), (3001, 70, 256)])
def test_null_bias_equals_the_old_entry_points(V, R, H):
    from gamer_amd import ops
    g = torch.Generator().manual_seed(V + R)
    h, E = (torch.randn(R + 4, H, generator=g) * 0.3).to(DEV), (torch.randn(V, H, generator=g) * 0.5).to(DEV)
    rows = torch.randperm(R + 4, generator=g)[:R].to(DEV)
    tgt = torch.randint(0, V, (R,), generator=g).to(DEV)
    dl = torch.full((), 1.5, device=DEV)
    out = []
    for new in (False, True):
        lse, loss, bad = torch.empty(R, device=DEV), torch.empty((), device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
        dE, dh = torch.zeros_like(E), torch.zeros_like(h)
        if new:
            ops.catalog_ce_bias_fwd(h, rows, E, None, tgt, lse, loss, bad)
            ops.catalog_ce_bias_bwd(h, rows, E, None, tgt, lse, dl, 1.0 / R, dE=dE, dh=dh)
            idx, sc = ops.catalog_topk_bias(h, E, None, 10, row_idx=rows)
        else:
            ops.catalog_ce_fwd(h, rows, E, tgt, lse, loss, bad)
            ops.catalog_ce_bwd(h, rows, E, tgt, lse, dl, 1.0 / R, dE=dE, dh=dh)
            idx, sc = ops.catalog_topk(h, E, 10, row_idx=rows)
        out.append((lse, loss, dE, dh, idx, sc))
    for a, b in zip(*out):
        assert torch.equal(a, b)


def test_biased_topk_against_stable_argsort():
    from gamer_amd import ops
    g = torch.Generator().manual_seed(4)
    R, V, H = 9, 3000, 128
    base = torch.randn(50, H, generator=g)
    pick = torch.randint(0, 50, (V,), generator=g)
    E = torch.cat([base[pick], torch.full((1, H), 1e30)])                       # exact ties; the row past V is never scored
    bias = torch.randint(0, 3, (50,), generator=g).float()[pick]                # equal rows get equal biases: the ties stay
    h = torch.randn(R, H, generator=g)
    idx, sc = ops.catalog_topk_bias(h.to(DEV), E.to(DEV), bias.to(DEV), 40, V=V)
    scores = h.double() @ E[:V].double().t() + bias.double()
    ref = torch.argsort(-scores, dim=1, stable=True)[:, :40]
    assert torch.equal(idx.cpu(), ref)
    assert torch.allclose(sc.double().cpu(), torch.gather(scores, 1, ref), atol=1e-5)
    # a sub-range, and K larger than it
    idx, sc = ops.catalog_topk_bias(h.to(DEV), E.to(DEV), bias.to(DEV), 20, 2990, 3000, V=V)
    ref = torch.argsort(-scores[:, 2990:], dim=1, stable=True) + 2990
    assert torch.equal(idx[:, :10].cpu(), ref) and bool((idx[:, 10:] == -1).all())


def test_bias_alone_reorders_the_top():
    from gamer_amd import ops
    V, H = 500, 64
    E = torch.zeros(V + 1, H)
    E[:V, 0] = torch.arange(V).float() * 1e-3                                   # without a bias the best items are V-1, V-2, ...
    E[V] = 1e30
    h = torch.zeros(3, H)
    h[:, 0] = 1.0
    bias = torch.zeros(V)
    bias[[7, 3, 11]] = torch.tensor([5.0, 5.0, 4.0])                            # 3 and 7 tie on the bias: 7 wins on the dot product
    plain, _ = ops.catalog_topk_bias(h.to(DEV), E.to(DEV), None, 4, V=V)
    assert plain[0].tolist() == [V - 1, V - 2, V - 3, V - 4]
    idx, sc = ops.catalog_topk_bias(h.to(DEV), E.to(DEV), bias.to(DEV), 4, V=V)
    assert idx.cpu().tolist() == [[7, 3, 11, V - 1]] * 3
    assert torch.allclose(sc[0].cpu(), torch.tensor([5.007, 5.003, 4.011, (V - 1) * 1e-3]), atol=1e-6)


def test_bias_wrappers_refuse_bad_arguments():
    from gamer_amd import ops
    h, E = torch.randn(4, 64, device=DEV), torch.randn(10, 64, device=DEV)
    tgt = torch.zeros(4, dtype=torch.long, device=DEV)
    lse, loss, bad = torch.empty(4, device=DEV), torch.empty((), device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="bias"):
        ops.catalog_ce_bias_fwd(h, None, E, torch.zeros(9, device=DEV), tgt, lse, loss, bad)
    with pytest.raises(RuntimeError, match="V = 11"):
        ops.catalog_ce_bias_fwd(h, None, E, None, tgt, lse, loss, bad, V=11)
    with pytest.raises(RuntimeError, match="dbias"):
        ops.catalog_ce_bias_bwd(h, None, E, None, tgt, lse, None, 0.25, dbias=torch.zeros(9, device=DEV))
    ops.catalog_ce_bias_fwd(h, None, E, None, torch.tensor([0, 9, 3, 3], device=DEV), lse, loss, bad, V=9)
    assert int(bad.item()) == 1                                                 # a target at V is outside the head


# ---- the cloze mask ------------------------------------------------------------------------------------------------------------
def _ragged(B, L, n_items, seed, lens=None):
    g = torch.Generator().manual_seed(seed)
    if lens is None:
        lens = torch.randint(1, L + 1, (B,), generator=g)
        lens[0], lens[1] = 1, L                                                  # a length-1 row and a full-length row
    ids = torch.randint(1, n_items + 1, (B, L), generator=g)
    ids[torch.arange(L)[None, :] >= lens[:, None]] = 0
    return ids, lens


def _restate(ids, lens, words, mask_ratio, ft_ratio, mask_token, max_len):
    """the rule of gamer_cloze_mask in torch, with the kernel's words as the uniforms: u < ratio <=> word < ratio 2^32.
    ft_row[b] = u_row(b) < ft_ratio; m[b, s] = u(b, s) < mask_ratio and ids[b, s] != 0 and not ft_row[b];
    m[b, p_b] |= ft_row[b], p_b = min(seq_len[b], max_len - 1); labels = ids * m; masked = mask_token where m else ids"""
    from gamer_amd import ops
    B, L = ids.shape

    def below(w, ratio):
        return torch.ones_like(w, dtype=torch.bool) if ratio >= 1 else w < ops.cloze_threshold(ratio)
    ft_row = below(words[B * L:], ft_ratio)
    m = below(words[:B * L].view(B, L), mask_ratio) & (ids != 0) & ~ft_row[:, None]
    p = torch.minimum(lens, torch.tensor(max_len - 1))
    m[torch.arange(B), p] |= ft_row
    labels = torch.where(m, ids, torch.zeros_like(ids))
    masked = torch.where(m, torch.full_like(ids, mask_token), ids)
    rows = labels.flatten().nonzero()[:, 0]
    return masked, labels, rows, labels.flatten()[rows]


@pytest.mark.parametrize("ft_ratio", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("mask_ratio", [0.0, 0.2, 1.0])
@pytest.mark.parametrize("B,L", [(7, 8), (300, 20), (33, 50)])
def test_cloze_mask_against_the_rule(ft_ratio, mask_ratio, B, L):
    from gamer_amd import ops
    ids, lens = _ragged(B, L, 1000, seed=B + L)
    seed = 0x1234_5678_9ABC + B
    out = ops.cloze_mask(ids.to(DEV), lens.to(DEV), mask_ratio, ft_ratio, 1001, L, seed, want_words=True)
    masked, labels, rows, targets, count, words = [t.cpu() for t in out]
    assert int(words.min()) >= 0 and int(words.max()) < 2 ** 32
    r_masked, r_labels, r_rows, r_targets = _restate(ids, lens, words, mask_ratio, ft_ratio, 1001, L)
    M = int(count)
    assert torch.equal(masked, r_masked) and torch.equal(labels, r_labels)
    assert M == r_rows.numel() and torch.equal(rows[:M], r_rows) and torch.equal(targets[:M], r_targets)
    if mask_ratio == 1.0 and ft_ratio == 0.0:
        assert M == int(lens.sum())
    if mask_ratio == 0.0 and ft_ratio == 0.0:
        assert M == 0 and torch.equal(masked, ids)


def test_cloze_mask_invariants_and_rates():
    from gamer_amd import ops
    B, L, p, ft = 4096, 50, 0.2, 0.5
    ids, lens = _ragged(B, L, 50_000, seed=9)
    tok = 50_001
    seed = 4242
    a = [t.cpu() for t in ops.cloze_mask(ids.to(DEV), lens.to(DEV), p, ft, tok, L, seed)]
    b = [t.cpu() for t in ops.cloze_mask(ids.to(DEV), lens.to(DEV), p, ft, tok, L, seed)]
    c = [t.cpu() for t in ops.cloze_mask(ids.to(DEV), lens.to(DEV), p, ft, tok, L, seed + 1)]
    masked, labels, rows, targets, count = a
    M = int(count)
    for x, y in zip(a[:2] + [rows[:M], targets[:M], count], b[:2] + [b[2][:M], b[3][:M], b[4]]):
        assert torch.equal(x, y)                                                 # same seed: same bits
    assert not torch.equal(masked, c[0])                                         # next seed: different bits
    is_mask = masked == tok
    pad = ids == 0
    appended = is_mask & pad
    # a fine-tuning row is one whose slot min(seq_len, L - 1) is masked and nothing else is
    slot = torch.clamp_max(lens, L - 1)
    ft_row = is_mask[torch.arange(B), slot] & (is_mask.sum(1) == 1)
    assert bool((appended.sum(1) <= 1).all())
    assert bool((appended.any(1) <= ft_row).all())                              # a masked padding slot only as a fine-tuning row's
    assert bool(appended[torch.arange(B), slot][appended.any(1)].all())          # ... and only at the appended slot
    cloze_row = ~ft_row
    assert torch.equal(labels, ids * is_mask) and bool((masked[~is_mask] == ids[~is_mask]).all())
    assert M == int((labels != 0).sum()) and bool((rows[1:M] > rows[:M - 1]).all())
    assert torch.equal(targets[:M], labels.flatten()[rows[:M]])
    # rates (derived, not measured): a binomial count lies within 5 standard deviations of its mean.  A cloze row that drew
    # exactly one mask at its last slot looks like a fine-tuning row: only full-length rows can (probability p (1 - p)^(L - 1)
    # = 4e-6 per row at L = 50: less than 0.02 rows expected), so the fine-tuning count is taken as it reads.
    k_ft = int(ft_row.sum())
    assert abs(k_ft - B * ft) <= 5 * math.sqrt(B * ft * (1 - ft)), k_ft
    N = int(lens[cloze_row].sum())
    k = int(is_mask[cloze_row].sum())
    assert abs(k - N * p) <= 5 * math.sqrt(N * p * (1 - p)), (k, N)


# ---- the model against the real reference class ------------------------------------------------------------------------------
def _model():
    from gamer_amd.bert4rec import BERT4Rec, BERT4RecConfig
    z = np.load(FX)
    m = json.loads(str(z["meta_json"]))
    model = BERT4Rec(BERT4RecConfig(**m["config"]), m["n_items"], m["max_his_len"])
    sd = bw.init_state_dict({k: tuple(s) for k, s in zip(m["keys"], m["shapes"])}, m["weight_seed"])
    model.load_state_dict(sd, strict=True)
    return model.to(DEV), z, m


def test_bert4rec_forward_loss_and_grads_match_reference():
    """the bars of test_sasrec_gpu.py::test_sasrec_forward_loss_and_grads_match_reference"""
    model, z, m = _model()
    masked, labels = torch.from_numpy(z["masked"]).to(DEV), torch.from_numpy(z["labels"]).to(DEV)
    model.train()                                          # (dropout_prob 0 in the fixture's config)
    logits, valid_labels = model(masked, labels)
    assert torch.equal(valid_labels.cpu(), torch.from_numpy(z["valid_labels"]))
    assert logits.shape == (valid_labels.numel(), m["n_items"] + 1)
    cols = torch.from_numpy(z["cols"])
    assert _rel(logits.cpu()[:, cols], z["logits_cols"]) < 2e-5
    model.zero_grad()
    loss = model.calculate_loss(dict(inputs=torch.from_numpy(z["inputs"]).to(DEV), seq_len=torch.from_numpy(z["seq_len"]).to(DEV)),
                                masked_labels=(masked, labels))
    loss.backward()
    assert model.last_masked_count == valid_labels.numel()
    assert abs(float(loss.detach()) - float(z["loss"])) <= 1e-5 * abs(float(z["loss"]))
    seen = 0
    for k, p in model.named_parameters():
        if k in m["no_grad"]:
            assert p.grad is None, k
        elif k.endswith("key.bias"):
            # softmax is invariant to a per-row shift: the key bias gradient is zero up to rounding on both sides
            assert p.grad is None or float(p.grad.abs().max()) < 1e-6
        elif "grad/" + k in z.files:
            assert p.grad is not None and p.grad.shape == p.shape and _rel(p.grad, z["grad/" + k]) < 2e-4, k
            seen += 1
    assert seen >= 20 and "grad/head.bias" in z.files
    gb = model.head.bias.grad
    assert int((gb != 0).sum()) == m["head_bias_grad_nonzero"] == m["n_items"] + 1          # dense: every item's softmax mass
    gi = model.item_embedding.weight.grad
    rows = torch.from_numpy(z["rows"])
    assert m["n_items"] + 1 in rows.tolist() and 0 in rows.tolist()
    assert _rel(gi.cpu()[rows], z["grad_item_rows"]) < 2e-4
    assert float(gi[0].abs().sum()) > 0 and float(gi[-1].abs().sum()) > 0      # the head reaches row 0, the gather reaches <MASK>
    ck = bw.checksums({"g": gi.cpu()})[0]
    ref = z["grad_item_checksum"]
    assert abs(ck[0] - ref[0]) < 2e-4 * np.sqrt(ref[1]) * 10 and abs(ck[1] - ref[1]) < 1e-3 * ref[1]


def test_bert4rec_full_sort_matches_reference():
    model, z, m = _model()
    model.eval()
    inter = dict(inputs=torch.from_numpy(z["eval_inputs"]).to(DEV), seq_len=torch.from_numpy(z["eval_seq_len"]).to(DEV))
    scores = model.full_sort_predict(dict(inter))
    assert scores.shape == (inter["inputs"].shape[0], m["n_items"] + 1)
    cols = torch.from_numpy(z["cols"])
    assert _rel(scores.cpu()[:, cols], z["scores_cols"]) < 2e-5
    assert bool(z["scores_equal_with_item_range"])                              # the reference ignores item_range ...
    ranged = model.full_sort_predict(dict(inter, item_range=(3001, 6001)))
    assert torch.equal(ranged, scores) and bool(torch.isfinite(ranged).all())   # ... and so does this
    idx, sc = model.full_sort_topk(dict(inter), 10)
    assert int(idx.max()) <= m["n_items"] and int(idx.min()) >= 0               # <MASK> is never returned
    ref_top = torch.from_numpy(z["top10"])
    full = scores.cpu()
    for b in range(idx.shape[0]):
        for q in range(10):
            a, r = int(idx[b, q]), int(ref_top[b, q])
            # identical ranks unless two neighbours' scores lie within fp32 noise of each other
            assert a == r or abs(float(full[b, a]) - float(full[b, r])) < 1e-5, (b, q, a, r)
    assert _rel(sc, torch.gather(full, 1, idx.cpu())) < 1e-5


def test_bert4rec_index_error_and_no_masked_position():
    model, z, m = _model()
    model.train()
    inputs, seq_len = torch.from_numpy(z["inputs"]).to(DEV), torch.from_numpy(z["seq_len"]).to(DEV)
    assert m["index_error"] == "index 5 is out of bounds for dimension 1 with size 5"
    with pytest.raises(IndexError, match="seq_len.*5|5.*seq_len"):
        model.reconstruct_train_data(inputs[1:4, :5], seq_len[1:4])
    with pytest.raises(IndexError, match="seq_len"):
        model.reconstruct_train_data(inputs, seq_len * 0)
    with pytest.raises(IndexError, match="seq_len"):
        model.calculate_loss(dict(inputs=inputs, seq_len=seq_len + 8))
    masked, labels = model.reconstruct_train_data(inputs, seq_len, seed=3)
    again = model.reconstruct_train_data(inputs, seq_len, seed=3)
    assert torch.equal(masked, again[0]) and torch.equal(labels, again[1])
    assert bool(((masked == inputs) | (masked == m["n_items"] + 1)).all())
    # M = 0, as recorded from the reference: NaN loss, backward() works, every gradient exactly zero, none NaN
    assert m["m0_loss_is_nan"] and m["m0_grads_all_zero"]
    model.mask_ratio, model.ft_ratio = 0.0, 0.0
    model.zero_grad()
    loss = model.calculate_loss(dict(inputs=inputs, seq_len=seq_len))
    assert model.last_masked_count == 0 and bool(torch.isnan(loss))
    loss.backward()
    assert [k for k, p in model.named_parameters() if p.grad is None] == m["m0_no_grad"]
    assert all(bool((p.grad == 0).all()) for p in model.parameters() if p.grad is not None)


def test_training_step_does_not_materialise_logits():
    from gamer_amd.bert4rec import BERT4Rec, BERT4RecConfig
    B, V, S = 4096, 200_000, 20
    torch.manual_seed(0)
    model = BERT4Rec(BERT4RecConfig(dropout_prob=0.0, n_layers=1, hidden_size=64, inner_size=128), V - 1, S).to(DEV)
    g = torch.Generator().manual_seed(1)
    inter = dict(inputs=torch.randint(1, V, (B, S), generator=g).to(DEV), seq_len=torch.full((B,), S, device=DEV))
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
    assert M > B                                          # about mask_ratio of half the tokens + half the rows: more rows than B
    limit = M * V * 4                                     # one [M, V] fp32 logits tensor
    print(f"M {M} peak {peak / 2 ** 20:.0f} MiB, [M, V] {limit / 2 ** 20:.0f} MiB")
    assert peak < 0.3 * limit, (peak, limit)              # the whole step, encoder activations included (SASRec's assertion)


def test_bert4rec_dropout_training_is_finite_and_repeatable():
    from gamer_amd import modules, rec_common
    model, z, m = _model()
    model.dropout_prob = 0.5
    for layer in model.trm_encoder.layer:
        layer.dropout_p = 0.5
    model.train()
    inter = dict(inputs=torch.from_numpy(z["inputs"]).to(DEV), seq_len=torch.from_numpy(z["seq_len"]).to(DEV))
    res = []
    for _ in range(2):
        rec_common._Seeds.value = 77                       # (the cloze masks and the input block's dropout draw from this counter)
        modules._SeedCounter.value = 99
        model.zero_grad()
        loss = model.calculate_loss(inter)
        loss.backward()
        res.append((loss.detach().clone(), model.item_embedding.weight.grad.clone(), model.position_embedding.weight.grad.clone(),
                    model.head.bias.grad.clone()))
    assert torch.isfinite(res[0][0]) and model.last_masked_count > 0
    for a, b in zip(res[0], res[1]):
        assert torch.equal(a, b)


def test_train_bert4rec_two_epochs_and_only_test(tmp_path):
    """One batch per epoch (batch size >= the number of training users): the reference-faithful IndexError of the cloze masking
    fires on a batch whose longest row is shorter than max_his_len, and the synthetic users are few; among 60 users with up to
    9 sessions several have at least 8 interactions before their validation session."""
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
    run = lambda extra: subprocess.run([sys.executable, "-m", "gamer_amd.train_bert4rec", *common, *extra], cwd=root,
                                       capture_output=True, text=True, timeout=300)
    r = run(["--epochs", "2"])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    losses = [float(l.split(" loss ")[1].split()[0]) for l in r.stdout.splitlines() if l.startswith("[train_bert4rec] epoch")]
    assert len(losses) == 2 and all(math.isfinite(x) for x in losses), r.stdout
    meta = json.loads(str(np.load(FX)["meta_json"]))
    sd = torch.load(tmp_path / "out" / "best_model.pth", map_location="cpu")
    assert list(sd) == meta["keys"]
    assert sd["item_embedding.weight"].shape[0] == sd["head.bias"].shape[1] + 1 and torch.equal(sd["item_embedding.weight"], sd["head.token_embeddings.weight"])
    res = json.load(open(tmp_path / "res" / "result-smb_dis_target_diff.json"))
    metrics = "hit@1,hit@5,hit@10,recall@1,recall@5,recall@10,ndcg@5,ndcg@10".split(",")
    assert [e["eval_type"] for e in res] == ["Behavior click", "Behavior cart", "Behavior buy", "Merged Behavior"]
    assert all(all(m in e and math.isfinite(e[m]) for m in metrics) for e in res)
    r2 = run(["--only_test"])
    assert r2.returncode == 0, r2.stdout[-2000:] + r2.stderr[-2000:]
    assert json.load(open(tmp_path / "res" / "result-smb_dis_target_diff.json")) == res
