"""PBATransformer on the GPU: the router and activation kernels against their host / fp64 restatements, the model against the real
reference classes (tests/golden/pbatransformer_small.npz, tools/make_golden_pbatransformer.py), beam search against the reference's
``generate(use_cache=False)``, dropout, and the train command.

Bars.  relu_tbl: one add, one compare and one multiply per element, no reduction: 1e-6 relative against fp64 torch on the
fp32-rounded inputs.  Model: per config, twice the worst error of an fp32 torch restatement of the whole model (run on the GPU,
tests/helpers/pbatransformer_ref.py) against the fixture, never above 1e-3 - the bar of tests/test_tiger_gpu.py.  Relative error =
largest absolute difference over the largest reference magnitude of the tensor."""
import json
import os
import sys
from collections import OrderedDict

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import pbatransformer_ref as pref  # noqa: E402
import pbatransformer_weights as pw  # noqa: E402
import t5_attention_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
FX = os.path.join(os.path.dirname(__file__), "golden", "pbatransformer_small.npz")
TIGER_FX = os.path.join(os.path.dirname(__file__), "golden", "tiger_small.npz")
DEV = ref.DEV


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


def _model(fx, name, dropout=0.0, **over):
    from gamer_amd.pbatransformer import PBATransformerConfig, PBATransformerForConditionalGeneration
    z, meta = fx
    src = meta[name].get("config", name)                            # ("long" runs config a's weights)
    cfg = PBATransformerConfig(**dict(meta["configs"][name], dropout_rate=dropout, **over))
    torch.manual_seed(0)
    m = PBATransformerForConditionalGeneration(cfg)
    shapes = OrderedDict(zip(meta[src]["keys"], [tuple(s) for s in meta[src]["shapes"]]))
    sd = pw.init_state_dict(shapes, meta[name]["weight_seed"])
    assert np.allclose(pw.checksums(sd), z[f"{src}/weight_checksums"], rtol=1e-12, atol=1e-9)
    m.load_state_dict(sd, strict=True)                              # a reference-shaped state dict
    m.set_hyper(meta["temperature"])
    return m.to(DEV), sd


def _batch(z, name):
    return tuple(torch.from_numpy(z[f"{name}/{k}"]) for k in ("input_ids", "attention_mask", "labels"))


# ---- the router kernel ----------------------------------------------------------------------------------------------------------------
def _route(m, ids, decoder):
    r = m.route(torch.as_tensor(ids).to(DEV), decoder)
    torch.cuda.synchronize()
    return r


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_router_kernel_equals_the_reference_routers(fx, name):
    z, meta = fx
    m, _ = _model(fx, name)
    cfg = meta["configs"][name]
    NB1, E = cfg["num_behavior"] + 1, meta[name]["num_experts"]
    for tag, ids, decoder in (("enc", z[f"{name}/input_ids"], False), ("dec", z[f"{name}/decoder_input_ids"], True)):
        r = _route(m, ids, decoder)
        pos, beh = torch.from_numpy(z[f"{name}/router/{tag}_pos"]), torch.from_numpy(z[f"{name}/router/{tag}_beh"])
        assert torch.equal(r.expert.cpu(), pos) and torch.equal(r.beh.cpu(), beh), (name, tag)
        assert torch.equal(r.key.cpu(), torch.where(pos < E, pos * NB1 + beh, torch.full_like(pos, -1)))
    m.check_inputs()                                                # no unmapped behaviour token so far


def test_router_kernel_on_the_decoder_lengths_and_a_padded_row(fx):
    z, meta = fx
    m, _ = _model(fx, "a")
    cfg = meta["configs"]["a"]
    P = cfg["num_positions"]
    full = [[0, 11, 30, 31, 32], [0, 10, 33, 1, 0], [0, 1, 0, 0, 0]]      # the worked example, a row ending early, all padding after </s>
    for S in (1, 2, P + 1):
        ids = [row[:S] for row in full]
        r = _route(m, ids, True)
        pos, beh, bad = pref.route_host(ids, cfg, True)
        assert r.expert.cpu().tolist() == pos and r.beh.cpu().tolist() == beh and bad == 0, S
    assert _route(m, full, True).beh.cpu().tolist() == [[0, 0, 2, 2, 2], [0, 0, 1, 0, 0], [0, 0, 0, 0, 0]]
    enc = [[10, 20, 21, 22, 11, 23, 24, 25, 10, 26, 27, 28, 1], [11, 20, 21, 22, 10, 23, 24, 25, 1, 0, 0, 0, 0], [1] + [0] * 12]
    r = _route(m, enc, False)
    assert r.expert.cpu().tolist()[:2] == [[1, 2, 3, 4, 1, 2, 3, 4, 1, 2, 3, 4, 0], [1, 2, 3, 4, 1, 2, 3, 4, 0, 0, 0, 0, 0]]
    assert r.beh.cpu().tolist()[:2] == [[0, 1, 1, 1, 0, 2, 2, 2, 0, 1, 1, 1, 0], [0, 2, 2, 2, 0, 1, 1, 1, 0, 0, 0, 0, 0]]
    assert r.expert.cpu().tolist()[2] == [0] * 13 and r.beh.cpu().tolist()[2] == [0] * 13
    m.check_inputs()
    with pytest.raises(ValueError, match="num_positions"):
        m.route(torch.zeros(2, 12, dtype=torch.int64, device=DEV), False)
    with pytest.raises(ValueError, match="decoder rows"):
        m.route(torch.zeros(2, P + 3, dtype=torch.int64, device=DEV), True)


def test_an_unmapped_behaviour_token_at_a_used_slot_raises_and_on_a_padded_tail_does_not(fx):
    z, meta = fx
    m, _ = _model(fx, "a")
    cfg = meta["configs"]["a"]
    tail = [[10, 20, 21, 22, 1, 0, 0, 0, 40, 0, 0, 0, 0]]                  # token 40 in a behaviour slot of the padded tail
    _route(m, tail, False)
    m.check_inputs()
    used = [[10, 20, 21, 22, 40, 23, 24, 25, 1, 0, 0, 0, 0]]               # ... and where three tokens use it
    r = _route(m, used, False)
    assert pref.route_host(used, cfg, False)[2] == 3 and r.beh.cpu().tolist()[0][4:8] == [0, 0, 0, 0]
    with pytest.raises(ValueError, match="behavior_maps"):
        m.check_inputs()
    m.check_inputs()                                                # the counter was cleared by the raise
    _route(m, [[0, 40, 30, 31, 32]], True)
    with pytest.raises(ValueError, match="3 positions"):
        m.check_inputs()


# ---- relu_tbl ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_tbl", [False, True])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_relu_tbl_forward_and_in_place_backward_against_fp64(with_tbl, p):
    # (5, 260, 520): 65 quads per row, a second trip of the lane loop with one lane
    for T, I, ld in ((70, 36, 44), (5, 260, 520)):
        _relu_tbl_case(T, I, ld, with_tbl, p)


def _relu_tbl_case(T, I, ld, with_tbl, p):
    from gamer_amd import ops
    G, seed = 5, (3 << 32) | 77
    g = torch.Generator().manual_seed(11 + int(with_tbl))
    pre = torch.randn(T, ld, generator=g)
    tbl = torch.randn(G, I, generator=g)
    group = torch.tensor([(0, 1, 2, 4)[i % 4] for i in range(T)], dtype=torch.int32)       # group 3 is empty
    group[T - 2 if T < 7 else 5], group[T - 1 if T < 7 else 6] = -1, G    # two rows of no group: they add nothing
    add = torch.zeros(T, I)
    if with_tbl:
        ok = (group >= 0) & (group < G)
        add[ok] = tbl[group[ok].long()]
    pre[::3, :I] = 0.25 - add[::3]                                    # sums of exactly 0.25 ...
    pre[::7, 4:9] = -add[::7, 4:9]                                    # ... and exact zeros of pre + tbl
    summed = pre[:, :I] + add
    assert int((summed == 0).sum()) >= 4 * len(range(0, T, 7)) and bool((summed > 0).any()) and bool((summed < 0).any())
    dact = torch.randn(T, I, generator=g)
    args = (tbl.to(DEV), group.to(DEV), G) if with_tbl else ()

    def fwd(x):
        act = torch.full((T, I), float("nan"), device=DEV)
        ops.relu_tbl_fwd(x, ld, T, I, p, seed, act, *args)
        return act
    # the mask from the kernel itself: an all-positive input with the same seed and geometry
    ones = torch.full((T, ld), 2.0) - torch.cat([add, torch.zeros(T, ld - I)], 1)
    raw = fwd(ones.to(DEV)).cpu().double() / 2.0
    scale = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
    kept = raw > 0.5
    assert float((raw[kept] - scale).abs().max()) < 1e-5 and float(raw[~kept].abs().sum()) == 0.0
    assert (0.03 < float((~kept).double().mean()) < 0.2) if p > 0 else bool(kept.all())
    mult = torch.where(kept, torch.tensor(scale, dtype=torch.float64), torch.zeros((), dtype=torch.float64))
    pre_d = pre.to(DEV)
    act = fwd(pre_d).cpu()
    want = torch.relu(summed.double()) * mult
    assert float((act.double() - want).abs().max()) <= 1e-6 * float(want.abs().max())
    assert torch.equal(pre_d.cpu(), pre)                              # the forward leaves pre alone
    ops.relu_tbl_bwd(pre_d, ld, T, I, dact.to(DEV), p, seed, *args)
    torch.cuda.synchronize()
    got = pre_d.cpu()
    want_d = dact.double() * mult * (summed.double() > 0)
    assert float((got[:, :I].double() - want_d).abs().max()) <= 1e-6 * float(want_d.abs().max())
    assert float(got[:, :I][summed == 0].abs().max()) == 0.0          # the derivative at exactly 0 is 0, as torch's
    assert torch.equal(got[:, I:], pre[:, I:])                        # the columns behind the width are not touched


def test_relu_tbl_refuses_bad_arguments():
    from gamer_amd import ops
    x, act = torch.zeros(8, 16, device=DEV), torch.zeros(8, 16, device=DEV)
    with pytest.raises(ValueError, match="come together"):
        ops.relu_tbl_fwd(x, 16, 8, 16, 0.0, 0, act, tbl=torch.zeros(2, 16, device=DEV))
    with pytest.raises(RuntimeError, match="bad arguments"):
        ops.relu_tbl_fwd(x, 16, 8, 14, 0.0, 0, act)
    with pytest.raises(ValueError, match="holds"):
        ops.relu_tbl_bwd(x, 16, 9, 16, act, 0.0, 0)


# ---- the model against the real classes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a", "b", "c", "long"])
def test_model_logits_loss_and_every_gradient_match_the_reference(fx, name):
    z, meta = fx
    m, sd = _model(fx, name)
    cfg = meta["configs"][name]
    ids, am, labels = _batch(z, name)
    if name == "long":
        from gamer_amd import tiger
        assert ids.shape[1] == 133 > tiger.MAX_ENCODER_LEN            # the key-streaming attention family
    m.train()                                                       # (dropout_rate 0: the training path, CatalogCEFn and all)
    loss, logits = m(ids.to(DEV), am.to(DEV), labels=labels.to(DEV), want_logits=True)
    loss.backward()
    m.check_inputs()
    r_loss, r_logits, r_grads = pref.restated_model(sd, cfg, ids, am, labels, meta["temperature"])
    kernel, torch32 = {}, {}
    kernel["logits"], torch32["logits"] = ref.rel_err(logits, z[f"{name}/logits"]), ref.rel_err(r_logits, z[f"{name}/logits"])
    ref_loss = float(z[f"{name}/loss"])
    kernel["loss"], torch32["loss"] = abs(float(loss.detach()) - ref_loss) / abs(ref_loss), abs(float(r_loss) - ref_loss) / abs(ref_loss)
    params = dict(m.named_parameters())
    if name != "long":
        assert set(params) == set(meta[name]["param_keys"]) and meta[name]["no_grad"] == []
        for k, p in params.items():
            want = torch.from_numpy(z[f"{name}/grad/{k}"])
            rows = pw.sample_rows(p.shape)
            assert p.grad is not None, k
            kernel[k], torch32[k] = ref.rel_err(p.grad[rows.to(DEV)], want), ref.rel_err(r_grads[k][rows.to(DEV)], want)
            # the rows the fixture does not hold: the whole tensor's sum of squares, whose relative error is twice the values'
            sumsq = float(z[f"{name}/grad_checksum/{k}"][1])
            kernel["sumsq/" + k] = 0.5 * abs(float(pw.checksums({k: p.grad.cpu()})[0][1]) - sumsq) / sumsq
            torch32["sumsq/" + k] = 0.5 * abs(float(pw.checksums({k: r_grads[k].cpu()})[0][1]) - sumsq) / sumsq
    else:
        for k, p in params.items():                                   # no recorded gradients: ours against the restatement's
            kernel["vs torch/" + k] = ref.rel_err(p.grad, r_grads[k])
    bar = min(2.0 * max(torch32.values()), 1e-3)
    worst = max((k for k in kernel if not k.startswith("vs torch/")), key=kernel.get)
    print(f"config {name}: kernel worst {kernel[worst]:.3e} ({worst}), logits {kernel['logits']:.3e}, loss {kernel['loss']:.3e}; "
          f"fp32 torch worst {max(torch32.values()):.3e}, logits {torch32['logits']:.3e}; bar {bar:.3e}")
    for k, e in kernel.items():
        assert e <= (1e-3 if k.startswith("vs torch/") else bar), (k, e, bar)


def test_expert_routing_is_real(fx):
    """exchanging the weights of experts 1 and 2 changes config a's logits; with every layer dense there is no expert to exchange"""
    z, meta = fx
    m, sd = _model(fx, "a")
    ids, am, labels = (t.to(DEV) for t in _batch(z, "a"))
    m.eval()
    with torch.no_grad():
        _, base = m(ids, am, labels=labels)
        swapped = OrderedDict(sd)
        for k in sd:
            if ".expert_1." in k:
                k2 = k.replace(".expert_1.", ".expert_2.")
                swapped[k], swapped[k2] = sd[k2], sd[k]
        m.load_state_dict(swapped, strict=True)
        _, moved = m(ids, am, labels=labels)
    assert ref.rel_err(moved, base) > 1e-2
    assert ref.rel_err(base, z["a/logits"]) < 1e-3
    from gamer_amd.pbatransformer import PBATransformerConfig, PBATransformerForConditionalGeneration
    dense = PBATransformerForConditionalGeneration(PBATransformerConfig(**dict(meta["configs"]["c"], sparse_layers_encoder=[],
                                                                               sparse_layers_decoder=[])))
    assert not any(".experts." in k for k in dense.state_dict())      # nothing to exchange: the layers hold one mlp each


def test_forward_without_labels_and_refusals(fx):
    z, meta = fx
    m, _ = _model(fx, "a")
    m.eval()
    ids, am, labels = (t.to(DEV) for t in _batch(z, "a"))
    with torch.no_grad():
        loss, logits = m(ids, am, decoder_input_ids=m._shift_right(labels))
        loss2, logits2 = m(ids, am, labels=labels)
    assert loss is None and ref.rel_err(logits, z["a/logits"]) < 1e-3 and torch.equal(logits, logits2)
    assert abs(float(loss2) - float(z["a/loss"])) < 1e-3 * float(z["a/loss"])
    with pytest.raises(NotImplementedError, match="packed"):
        m(ids, am, labels=labels, packed=True)
    with pytest.raises(RuntimeError, match="HIP device only"):
        m(ids.cpu(), am.cpu(), labels=labels.cpu())


# ---- beam search ------------------------------------------------------------------------------------------------------------------------
def test_beam_search_finds_generates_beams(fx):
    from gamer_amd import pbatransformer
    from gamer_amd.decode import ItemTrie
    z, meta = fx
    m, _ = _model(fx, "a")
    nb, new = meta["num_beams"], meta["max_new_tokens"]
    assert meta["a"]["smallest_gap"] > 1e-3
    ids, am = torch.from_numpy(z["gen/input_ids"]).to(DEV), torch.from_numpy(z["gen/attention_mask"]).to(DEV)
    trie = ItemTrie(z["gen/trie"].tolist(), device=DEV, pad_token_id=0)
    seqs, scores = pbatransformer.beam_search(m, ids, am, trie, nb, new)
    assert torch.equal(seqs.cpu(), torch.from_numpy(z["gen/sequences"]))
    assert ref.rel_err(scores, z["gen/sequences_scores"]) < 1e-3
    assert len({int(t) for t in seqs[:, 1].cpu()}) == 2               # hypotheses of both behaviours: each is routed by its own token
    one_s, one_sc = pbatransformer.beam_search(m, ids[1:2], am[1:2], trie, nb, new)
    assert torch.equal(one_s, seqs[nb:2 * nb]) and torch.allclose(one_sc, scores[nb:2 * nb], rtol=1e-5, atol=1e-6)


# ---- dropout, end to end ----------------------------------------------------------------------------------------------------------------
def test_dropout_is_repeatable_from_the_seed_counters(fx):
    from gamer_amd import modules, rec_common
    z, meta = fx
    m, _ = _model(fx, "a", dropout=0.1)
    m.train()
    ids, am, labels = (t.to(DEV) for t in _batch(z, "a"))

    def run(seed):
        modules._SeedCounter.value, rec_common._Seeds.value = 1000 + seed, 2000 + seed
        for p in m.parameters():
            p.grad = None
        loss, _ = m(ids, am, labels=labels)
        loss.backward()
        return loss.detach().clone(), [p.grad.clone() for p in m.parameters()]
    l1, g1 = run(0)
    l2, g2 = run(0)
    l3, g3 = run(1)
    assert torch.equal(l1, l2) and all(torch.equal(a, b) for a, b in zip(g1, g2))
    assert not torch.equal(l1, l3) and any(not torch.equal(a, b) for a, b in zip(g1, g3))
    assert abs(float(l1) - float(z["a/loss"])) > 1e-4
    assert all(bool(torch.isfinite(g).all()) for g in g1 + g3)


# ---- TIGER's half ------------------------------------------------------------------------------------------------------------------------
def test_an_all_dense_model_without_injection_is_tiger_bit_for_bit():
    """The attention half of the block, the stacks' frame, the loss and the beam search are TIGER's code: with every layer dense and
    no injection, TIGER's weights under the PBATransformer names give TIGER's loss, logits and gradients bit for bit (dropout off:
    ReLU is exact in both activation kernels, every matrix product is the same call)."""
    from gamer_amd import tiger
    from gamer_amd.decode import ItemTrie
    from gamer_amd.pbatransformer import PBATransformerConfig, PBATransformerForConditionalGeneration
    z = np.load(TIGER_FX)
    meta = json.loads(str(z["meta_json"]))
    t, sd = ref.load_model(z, meta, "a")
    c = meta["configs"]["a"]
    cfg = PBATransformerConfig(**dict(c, num_positions=4, num_behavior=2, n_positions=50, use_behavior_token=False))
    m = PBATransformerForConditionalGeneration(cfg)
    m.load_state_dict(OrderedDict((k.replace("DenseReluDense.", "mlp.mlp."), v) for k, v in sd.items()), strict=True)
    m.set_hyper(meta["temperature"])
    m.to(DEV)
    ids, am, labels = (torch.from_numpy(z[f"a/{k}"]).to(DEV) for k in ("input_ids", "attention_mask", "labels"))
    outs = []
    for model in (t, m):
        model.train()
        loss, logits = model(ids, am, labels=labels, want_logits=True)
        loss.backward()
        outs.append((loss.detach(), logits, {k.replace("DenseReluDense.", "mlp.mlp."): p.grad for k, p in model.named_parameters()}))
    (l_t, lg_t, g_t), (l_m, lg_m, g_m) = outs
    assert torch.equal(l_t, l_m) and torch.equal(lg_t, lg_m)
    assert set(g_t) == set(g_m) and all(torch.equal(g_t[k], g_m[k]) for k in g_t)
    trie = ItemTrie(z["a/trie_plain"].tolist(), device=DEV, pad_token_id=0)
    steps = z["a/beams_plain_4"].shape[1] - 1
    s_t, sc_t = tiger.beam_search(t, ids[:3], am[:3], trie, 4, steps)
    s_m, sc_m = tiger.beam_search(m, ids[:3], am[:3], trie, 4, steps)
    assert torch.equal(s_t, s_m) and torch.equal(sc_t, sc_m)
    assert torch.equal(s_t.cpu(), torch.from_numpy(z["a/beams_plain_4"]))


# ---- the command ----------------------------------------------------------------------------------------------------------------------
def test_train_pbatransformer_end_to_end(tmp_path, capsys):
    from gamer_amd import synthetic, t5_mb_data, train_pbatransformer
    root = tmp_path / "data"
    synthetic.write_smb_dataset(str(root), "Toy", n_users=40, n_items=60, codebook=8, seed=1)
    base = tmp_path / "base"
    base.mkdir()
    (base / "config.json").write_text(json.dumps(dict(
        d_model=64, d_kv=64, d_ff=128, num_layers=2, num_decoder_layers=2, num_heads=2, dropout_rate=0.1, vocab_size=32128,
        behavior_injection=True, behavior_embedding_dim=16, sparse_layers_encoder=[], sparse_layers_decoder=[0, 1],
        behavior_injection_encoder=[0], behavior_injection_decoder=[0], model_type="switch_transformers")))
    out = tmp_path / "ckpt"
    metrics = "hit@1,hit@5,ndcg@5"
    common = ["--base_model", str(base), "--data_path", str(root), "--dataset", "Toy", "--tasks", "smb_explicit", "--max_his_len", "8",
              "--output_dir", str(out), "--per_device_batch_size", "16", "--gradient_accumulation_steps", "1", "--test_batch_size", "16",
              "--num_beams", "10", "--metrics", metrics, "--results_file", str(tmp_path / "res.json")]
    res = train_pbatransformer.main(common + ["--epochs", "2", "--learning_rate", "3e-3", "--warmup_ratio", "0.0"])
    log = capsys.readouterr().out
    rows = [l for l in log.splitlines() if l.startswith("[train_pbatransformer] epoch ")]
    train = [float(l.split(" loss ")[1].split()[0]) for l in rows]
    assert len(train) == 2 and all(np.isfinite(train)) and train[1] < train[0], log
    data = t5_mb_data.T5SMBData(str(root), "Toy", "smb_explicit")
    sd = torch.load(out / "best_model.pth", map_location="cpu")
    E = data.token_count + 1
    assert sd["shared.weight"].shape == (data.vocab_size, 64) and "lm_head.weight" in sd
    assert sd[f"decoder.block.1.layer.2.mlp.experts.expert_{E - 1}.wi.weight"].shape == (128, 64)
    assert sd["decoder.block.0.layer.2.mlp.experts.expert_0.wi.weight"].shape == (128, 80)
    assert sd["encoder.block.0.layer.1.mlp.behavior_embedding.weight"].shape == (len(data.behaviors) + 1, 16)
    assert [r["eval_type"] for r in res] == [f"Behavior {b}" for b in data.behaviors] + ["Merged Behavior"]
    for m_ in metrics.split(","):
        assert all(0.0 <= r[m_] <= 1.0 for r in res)
    again = train_pbatransformer.main(common + ["--only_test"])
    assert again == res and json.load(open(tmp_path / "res.json")) == res
