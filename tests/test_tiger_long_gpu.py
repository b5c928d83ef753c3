"""TIGER's key-streaming attention (csrc/t5_attention_long.hip, Sq, Sk <= 512) on the GPU: the kernels against an fp64 torch
restatement on the fp32-rounded inputs, their invariants, refusals and memory; the model at encoder lengths above 128 against the
real reference class (tests/golden/tiger_long.npz, tools/make_golden_tiger_long.py), beam search against HF's ``generate`` and the
train command at 201 tokens.

Bars (those of tests/test_tiger_gpu.py).  Attention: every case of the grid also runs the restatement as fp32 torch ops on the GPU;
per quantity the kernel may err by at most twice the restatement's worst relative error over the grid, and never by more than
1e-4.  Model: per config, twice the worst error of an fp32 torch restatement of the whole model against the fixture, never above
1e-3.  Relative error = largest absolute difference over the largest reference magnitude of the tensor.  The kernels' blocks are 64
queries by 64 keys, a power of two, so the grid below needs no extra block-edge shapes."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import t5_attention_ref as ref  # noqa: E402
import tiger_weights as tw  # noqa: E402

pytestmark = pytest.mark.gpu
FX = os.path.join(os.path.dirname(__file__), "golden", "tiger_long.npz")
DEV = ref.DEV

SHAPES = [(1, 129), (5, 300), (8, 512), (129, 129), (130, 257), (257, 130), (257, 257), (512, 512)]
TWO_ROWS = {(257, 257), (512, 512)}                                  # B = 2 only: keeps the module fixture near ten seconds
HAND_OVER = [(7, 7), (101, 101), (5, 128), (128, 128)]               # the resident family's shapes closest to the hand-over


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


def _grid(shapes=SHAPES):
    """every shape with h in {1, 6}, d in {32, 64}, B in {1, 3} (B = 2 for TWO_ROWS) with and without the bias; causality (square
    shapes), the key masks and dropout rotate so that each value meets every shape, and dropout meets both bias settings"""
    cases, n = [], 0
    for Sq, Sk in shapes:
        for h in (1, 6):
            for d in (32, 64):
                for B in ((2,) if (Sq, Sk) in TWO_ROWS else (1, 3)):
                    for bias in (True, False):
                        mask = ref.MASKS[n % 5]
                        if mask == "empty" and B == 1:
                            mask = "holes"
                        cases.append((Sq, Sk, h, d, B, bias, Sq == Sk and n % 3 == 0, mask, 0.1 if n % 4 in (1, 2) else 0.0))
                        n += 1
    return cases


@pytest.fixture(scope="module")
def grid():
    return ref.grid_errors(_grid())


def _worst_torch(rows):
    return max(r[2] for r in rows if r[3] > 1e-12 * max(r[5], 1e-30))


def _assert_rows(quantity, rows, worst_torch):
    for c, ek, et, mag, gotmag, gmax in rows:
        if mag > 1e-12 * max(gmax, 1e-30):
            assert ek <= 2.0 * worst_torch and ek <= 1e-4, (quantity, c, ek, worst_torch)
        else:
            # zero in exact arithmetic (one allowed key in every row): rounding residue, held to 1e-4 of the largest input gradient
            assert gotmag <= 1e-4 * gmax, (quantity, c, gotmag, gmax)


@pytest.mark.parametrize("quantity", ref.QUANTITIES)
def test_attention_against_fp64_within_twice_the_fp32_torch_error(grid, quantity):
    rows = grid[quantity]
    assert len(rows) >= 50
    live = [r for r in rows if r[3] > 1e-12 * max(r[5], 1e-30)]
    worst = _worst_torch(rows)
    print(f"{quantity}: kernel {max(r[1] for r in live):.3e}  fp32 torch {worst:.3e}  ({len(live)} of {len(rows)} cases)")
    _assert_rows(quantity, rows, worst)


def test_masks_cover_the_grid():
    cases = _grid()
    for Sq, Sk in SHAPES:
        mine = [c for c in cases if c[:2] == (Sq, Sk)]
        assert {c[2] for c in mine} == {1, 6} and {c[3] for c in mine} == {32, 64}
        assert {c[4] for c in mine} == ({2} if (Sq, Sk) in TWO_ROWS else {1, 3})
        assert {(c[5], c[8]) for c in mine} == {(True, 0.0), (True, 0.1), (False, 0.0), (False, 0.1)}
        assert set(ref.MASKS) <= {c[7] for c in mine}
        if Sq == Sk:
            assert {c[6] for c in mine} == {True, False}


def test_both_families_agree_where_both_run(grid):
    """the key-streaming entry points on the resident family's shapes next to the hand-over, held to the grid's bar"""
    errs = ref.grid_errors([c for c in _grid(HAND_OVER) if c[2:5] in ((6, 64, 3), (1, 32, 3), (6, 32, 1), (1, 64, 1))])
    for quantity in ref.QUANTITIES:
        live = [r for r in errs[quantity] if r[3] > 1e-12 * max(r[5], 1e-30)]
        print(f"{quantity}: kernel {max(r[1] for r in live):.3e}  fp32 torch (these shapes) {_worst_torch(errs[quantity]):.3e}")
        assert len(errs[quantity]) >= 8
        _assert_rows(quantity, errs[quantity], _worst_torch(grid[quantity]))


def test_a_row_with_no_kept_key_gives_zeros_and_zero_gradients():
    Sq, Sk = 130, 257
    got, truth, _ = ref.case(Sq, Sk, 2, 32, 3, True, False, "empty", 0.0, torch32=False)
    o, dq, lse = got["o"].view(3, Sq, -1), got["dq"].view(3, Sq, -1), got["lse"]
    assert float(o[2].abs().max()) == 0.0 and float(dq[2].abs().max()) == 0.0
    assert float(got["dk"].view(3, Sk, -1)[2].abs().max()) == 0.0 and float(got["dv"].view(3, Sk, -1)[2].abs().max()) == 0.0
    assert bool(torch.isinf(lse[2]).all()) and bool((lse[2] < 0).all()) and bool(torch.isfinite(lse[:2]).all())
    for k in truth:
        assert ref.rel_err(got[k], truth[k]) < 1e-4, k


@pytest.mark.parametrize("case", [(257, 257, 6, 64, 3, True, False, "right", 0.1), (257, 257, 2, 32, 2, True, True, "none", 0.1),
                                  (5, 300, 2, 32, 3, False, False, "holes", 0.0)])
def test_two_calls_bit_identical(case):
    a, _, _ = ref.case(*case, truth=False)
    b, _, _ = ref.case(*case, truth=False)
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("Sq,Sk,h,d,causal", [(257, 257, 2, 32, False), (129, 129, 6, 64, True), (5, 300, 6, 64, False)])
def test_rows_are_independent(Sq, Sk, h, d, causal):
    full, _, _ = ref.case(Sq, Sk, h, d, 3, True, causal, "right", 0.0, truth=False)
    one, _, _ = ref.case(Sq, Sk, h, d, 3, True, causal, "right", 0.0, rows=[2], truth=False)
    for k, S in (("o", Sq), ("dq", Sq), ("dk", Sk), ("dv", Sk)):
        assert torch.equal(one[k], full[k][2 * S:3 * S]), k
    assert torch.equal(one["lse"][0], full["lse"][2])


@pytest.mark.parametrize("B,n_slab", [(7, 3), (7, 1), (5, 5)])
def test_backward_walks_several_rows_per_workgroup(B, n_slab):
    """fewer slabs than rows: a workgroup adds the offsets of all its rows and query blocks and writes its slab once, in full"""
    got, truth, _ = ref.case(130, 130, 2, 64, B, True, False, "left", 0.1, n_slab=n_slab, torch32=False)
    assert got["slabs"].shape[1] == n_slab and not bool(torch.isnan(got["slabs"]).any())
    for k in truth:
        assert ref.rel_err(got[k], truth[k]) < 1e-4, (k, ref.rel_err(got[k], truth[k]))


def test_a_stacks_table_gradient_is_the_sum_of_its_layers_folds_in_layer_order():
    from gamer_amd import ops
    from gamer_amd.tiger import bucket_vector
    layers = []
    for l in range(3):
        got, _, _ = ref.case(257, 257, 6, 64, 3, True, False, "right", 0.0, seed=l, truth=False)
        layers.append(got["slabs"][0] * (1.0 + l))
    slabs = torch.stack(layers).contiguous()
    assert slabs.shape[-1] == 513
    bd = bucket_vector(257, True, ref.NB, ref.MAXD).to(DEV)
    whole = torch.empty(ref.NB, 6, device=DEV)
    ops.t5_bias_fold(slabs, bd, whole)
    acc = None
    for l in range(3):
        one = torch.empty(ref.NB, 6, device=DEV)
        ops.t5_bias_fold(slabs[l:l + 1].contiguous(), bd, one)
        acc = one if acc is None else acc + one
    assert torch.equal(whole, acc)


def test_beam_rows_read_their_users_keys_and_values():
    from gamer_amd import ops
    users, beams, Sq, Sk, h, d = 3, 4, 5, 300, 6, 64
    I, N = h * d, users * beams
    g = torch.Generator().manual_seed(11)
    q = (torch.randn(N * Sq, I, generator=g) * (10.0 / d) ** 0.5).to(DEV)
    kv = torch.randn(users * Sk, 2 * I, generator=g).to(DEV)
    keep = ref.key_mask("right", users, Sk, g).to(torch.uint8).to(DEV)
    rows = torch.arange(users, dtype=torch.int32).repeat_interleave(beams).to(DEV)
    o1, l1 = torch.full((N * Sq, I), float("nan"), device=DEV), torch.full((N, h, Sq), float("nan"), device=DEV)
    ops.t5_attn_long_fwd(q, kv[:, :I], kv[:, I:], None, keep, N, Sq, Sk, h, d, False, 0.0, 0, o1, l1, kv_rows=rows, kv_batch=users)
    kvr = kv.view(users, Sk, 2 * I).repeat_interleave(beams, 0).reshape(N * Sk, 2 * I).contiguous()
    o2, l2 = torch.empty_like(o1), torch.empty_like(l1)
    ops.t5_attn_long_fwd(q, kvr[:, :I], kvr[:, I:], None, keep.repeat_interleave(beams, 0).contiguous(), N, Sq, Sk, h, d, False, 0.0, 0, o2, l2)
    assert torch.equal(o1, o2) and torch.equal(l1, l2) and bool(torch.isfinite(o1).all())


def test_refusals_leave_the_outputs_untouched():
    from gamer_amd import _lib, ops
    t = torch.zeros(1024, 64, device=DEV)
    lse = torch.zeros(1, 1, 1024, device=DEV)
    p = t.data_ptr()
    for Sq, Sk, h, d in ((513, 8, 1, 64), (8, 513, 1, 64), (8, 8, 17, 64), (8, 8, 1, 48), (0, 8, 1, 64)):
        with pytest.raises(NotImplementedError):
            ops.t5_long_check_limits(Sq, Sk, h, d)
        with pytest.raises(RuntimeError, match="bad shape"):
            _lib.call("gamer_t5_attn_long_fwd", p, 64, p, 64, p, 64, None, None, None, 1, Sq, Sk, h, d, 0, 0.0, 0, p, 64, lse.data_ptr(),
                      ops.stream_ptr())
        with pytest.raises(RuntimeError, match="bad shape"):
            _lib.call("gamer_t5_attn_long_bwd", p, 64, p, 64, p, 64, None, None, 1, Sq, Sk, h, d, 0, 0.0, 0, p, 64, lse.data_ptr(), p, 64,
                      p, 64, p, 64, None, 1, lse.data_ptr(), ops.stream_ptr())
    with pytest.raises(RuntimeError, match="n_slab"):
        _lib.call("gamer_t5_attn_long_bwd", p, 64, p, 64, p, 64, None, None, 2, 130, 130, 1, 64, 0, 0.0, 0, p, 64, lse.data_ptr(), p, 64, p, 64,
                  p, 64, None, 3, lse.data_ptr(), ops.stream_ptr())
    # the resident entry points keep their bound
    with pytest.raises(RuntimeError, match="bad shape"):
        _lib.call("gamer_t5_attn_fwd", p, 64, p, 64, p, 64, None, None, None, 1, 129, 8, 1, 64, 0, 0.0, 0, p, 64, lse.data_ptr(), ops.stream_ptr())
    torch.cuda.synchronize()
    assert float(t.abs().max()) == 0.0 and float(lse.abs().max()) == 0.0


def test_attention_needs_no_score_sized_memory():
    """forward + backward with dropout and the bias at B 64, S 512: beyond inputs, outputs, gradients and slabs the kernels take the
    two row terms of B h S floats each (1.6 MB); the bar is a tenth of one [B, h, S, S] fp32 tensor (40 MB of 403 MB)"""
    from gamer_amd import ops
    B, S, h, d = 64, 512, 6, 64
    I = h * d
    qkv = torch.randn(B * S, 3 * I, device=DEV) * 0.3
    dqkv, o, d_o = torch.empty_like(qkv), torch.empty(B * S, I, device=DEV), torch.randn(B * S, I, device=DEV)
    lse, rel = torch.empty(B, h, S, device=DEV), torch.randn(h, 2 * S - 1, device=DEV)
    slabs = torch.empty(ops.t5_n_slab(B, h), h, 2 * S - 1, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ops.t5_attn_long_fwd(qkv[:, :I], qkv[:, I:2 * I], qkv[:, 2 * I:], rel, None, B, S, S, h, d, False, 0.1, 3, o, lse)
    ops.t5_attn_long_bwd(qkv[:, :I], qkv[:, I:2 * I], qkv[:, 2 * I:], rel, None, B, S, S, h, d, False, 0.1, 3, d_o, lse, dqkv[:, :I],
                         dqkv[:, I:2 * I], dqkv[:, 2 * I:], slabs)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base
    print(f"extra memory {extra / 1e6:.2f} MB")
    assert extra < B * h * S * S * 4 // 10, extra
    assert bool(torch.isfinite(dqkv).all()) and bool(torch.isfinite(slabs).all()) and bool(torch.isfinite(o).all())


# ---- the model against the real class -------------------------------------------------------------------------------------------------
def _batch(z, name):
    return (torch.from_numpy(z[f"{name}/{k}"].astype(np.int64)) for k in ("input_ids", "attention_mask", "labels"))


@pytest.mark.parametrize("name", ["c", "d"])
def test_model_logits_loss_and_every_gradient_match_the_reference(fx, name):
    """config c holds rows of 300, 129, 512 and 1 tokens in one batch 512 wide: the length-1 row runs the key-streaming kernels too"""
    z, meta = fx
    m, sd = ref.load_model(z, meta, name)
    ids, am, labels = _batch(z, name)
    assert ids.shape[1] == max(meta["enc_lens"][name]) > 128
    m.train()                                                       # (dropout_rate 0: the training path, CatalogCEFn and all)
    loss, logits = m(ids.to(DEV), am.to(DEV), labels=labels.to(DEV), want_logits=True)
    loss.backward()
    r_loss, r_logits, r_grads = ref.restated_model(sd, meta["configs"][name], ids, am, labels, meta["temperature"])
    params = dict(m.named_parameters())
    assert set(params) == set(meta[name]["param_keys"]) and meta[name]["no_grad"] == []
    kernel, torch32 = {}, {}
    kernel["logits"], torch32["logits"] = ref.rel_err(logits, z[f"{name}/logits"]), ref.rel_err(r_logits, z[f"{name}/logits"])
    ref_loss = float(z[f"{name}/loss"])
    kernel["loss"], torch32["loss"] = abs(float(loss.detach()) - ref_loss) / abs(ref_loss), abs(float(r_loss) - ref_loss) / abs(ref_loss)
    for k, p in params.items():
        want_rows = torch.from_numpy(z[f"{name}/grad/{k}"])
        rows = tw.sample_rows(p.shape)
        assert p.grad is not None, k
        kernel[k], torch32[k] = ref.rel_err(p.grad[rows.to(DEV)], want_rows), ref.rel_err(r_grads[k][rows.to(DEV)], want_rows)
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


@pytest.mark.parametrize("nb", [4, 20])
def test_beam_search_finds_generates_beams(fx, nb):
    from gamer_amd import tiger
    from gamer_amd.decode import ItemTrie
    z, meta = fx
    m, _ = ref.load_model(z, meta, "c")
    ids, am, _ = _batch(z, "c")
    ids, am = ids[:3].to(DEV), am[:3].to(DEV)
    trie = ItemTrie(z["c/trie_plain"].tolist(), device=DEV, pad_token_id=0)
    steps = z[f"c/beams_plain_{nb}"].shape[1] - 1
    seqs, scores = tiger.beam_search(m, ids, am, trie, nb, steps)
    assert torch.equal(seqs.cpu(), torch.from_numpy(z[f"c/beams_plain_{nb}"]))
    assert ref.rel_err(scores, torch.from_numpy(z[f"c/scores_plain_{nb}"])) < 1e-3
    # one user alone: the same beams as that user's rows of the batch
    one_s, one_sc = tiger.beam_search(m, ids[1:2], am[1:2], trie, nb, steps)
    assert torch.equal(one_s, seqs[nb:2 * nb]) and torch.allclose(one_sc, scores[nb:2 * nb], rtol=1e-5, atol=1e-6)


def test_train_tiger_end_to_end_at_201_tokens(tmp_path, capsys):
    from gamer_amd import synthetic, train_tiger
    root = tmp_path / "data"
    synthetic.write_seqrec_dataset(str(root), "Toy", n_users=20, n_items=60, codebook=8, seed=1, min_len=40, max_len=60)
    base = tmp_path / "base"
    base.mkdir()
    (base / "config.json").write_text(json.dumps(dict(d_model=64, d_kv=32, d_ff=128, num_layers=2, num_decoder_layers=2, num_heads=2,
                                                      dropout_rate=0.1, vocab_size=32128)))
    out = tmp_path / "ckpt"
    common = ["--base_model", str(base), "--data_path", str(root), "--dataset", "Toy", "--max_his_len", "50", "--output_dir", str(out),
              "--per_device_batch_size", "64", "--test_batch_size", "16", "--num_beams", "10", "--metrics", "hit@1,hit@5,ndcg@5",
              "--results_file", str(tmp_path / "res.json")]
    res = train_tiger.main(common + ["--epochs", "2", "--learning_rate", "3e-3", "--warmup_ratio", "0.0"])
    log = capsys.readouterr().out
    losses = [float(l.split(" eval_loss ")[1].split()[0]) for l in log.splitlines() if " eval_loss " in l and "epoch" in l]
    assert len(losses) == 2 and losses[1] < losses[0], log                  # the evaluation loss falls
    from gamer_amd.tiger import TIGER, TigerConfig
    sd = torch.load(out / "best_model.pth", map_location="cpu")
    fresh = TIGER(TigerConfig.from_pretrained(str(base)))
    fresh.resize_token_embeddings(sd["shared.weight"].shape[0])
    fresh.load_state_dict(sd, strict=True)
    again = train_tiger.main(common + ["--only_test"])
    assert again == res and set(res) >= {"hit@1", "hit@5", "ndcg@5"} and all(0.0 <= res[k] <= 1.0 for k in ("hit@1", "hit@5", "ndcg@5"))
