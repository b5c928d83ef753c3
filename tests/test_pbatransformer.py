"""PBATransformer without a GPU: the config and its refusals, the module's names and shapes against the real reference classes
(tests/golden/pbatransformer_small.npz), a reference-named state dict, the init recipe, the command's parser, the host restatement
of the two routers against the reference's router outputs, and the model restatement the GPU tests lean on against the recorded
loss and logits in fp64."""
import json
import math
import os
import sys
from collections import OrderedDict

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import pbatransformer_ref as pref  # noqa: E402
import pbatransformer_weights as pw  # noqa: E402

from gamer_amd import pbatransformer as pb  # noqa: E402
from gamer_amd.pbatransformer import PBATransformerConfig, PBATransformerForConditionalGeneration  # noqa: E402

FX = os.path.join(os.path.dirname(__file__), "golden", "pbatransformer_small.npz")


@pytest.fixture(scope="module")
def fx():
    z = np.load(FX)
    return z, json.loads(str(z["meta_json"]))


def _cfg(meta, name, **over):
    return PBATransformerConfig(**dict(meta["configs"][name], **over))


# ---- config ------------------------------------------------------------------------------------------------------------------------------
def test_config_derives_the_experts_and_drops_unknown_keys(fx):
    _, meta = fx
    c = _cfg(meta, "a", task_specific_params={"x": 1}, architectures=["y"], num_experts=99)
    assert c.num_experts == c.num_positions + 1 == 5 == meta["a"]["num_experts"] and not hasattr(c, "architectures")
    assert _cfg(meta, "b").num_experts == 2 == meta["b"]["num_experts"]
    assert c.behavior_maps == {10: 0, 11: 1}                          # the keys of a config.json are strings
    assert c.sparse_layers_decoder == [0, 1] and c.behavior_injection_encoder == [0, 1]
    d = PBATransformerConfig()
    assert (d.sparse_layers_encoder, d.behavior_maps, d.num_positions, d.behavior_embedding_dim, d.n_positions) == ([], {}, 4, 64, 50)
    assert (d.d_model, d.d_ff, d.num_layers, d.num_decoder_layers, d.num_heads, d.dense_act_fn) == (768, 2048, 12, 12, 12, "relu")
    d.sparse_layers_encoder.append(1)
    assert PBATransformerConfig().sparse_layers_encoder == []         # no list shared between instances
    assert PBATransformerConfig.from_dict(c.to_dict()).to_dict() == c.to_dict()


def test_the_shipped_config_reads_as_the_reference_reads_it(fx, tmp_path):
    _, meta = fx
    shipped = meta["shipped_config"]
    (tmp_path / "config.json").write_text(json.dumps(dict(shipped, architectures=["PBATransformersForConditionalGeneration"],
                                                          task_specific_params={}, model_type="switch_transformers")))
    c = PBATransformerConfig.from_pretrained(str(tmp_path))
    for k, v in shipped.items():
        assert getattr(c, k) == v, k
    PBATransformerForConditionalGeneration(PBATransformerConfig(**dict(c.to_dict(), vocab_size=128)))    # inside the limits


@pytest.mark.parametrize("over,what", [
    (dict(shared_expert=True), "shared_expert"), (dict(use_user_token=True), "use_user_token"),
    (dict(dense_act_fn="gelu_new"), "relu"), (dict(feed_forward_proj="gated-gelu"), "relu"),
    (dict(tie_word_embeddings=False), "tie_word_embeddings"), (dict(d_model=512), "d_model"), (dict(d_kv=48), "d_kv"),
    (dict(num_heads=17), "num_heads"), (dict(num_positions=15, num_behavior=4), "row groups"),
    (dict(behavior_embedding_dim=18), "behavior_embedding_dim"), (dict(num_behavior=16, Moe_behavior_only=True), "num_behavior <")])
def test_what_is_not_built_is_refused_by_name(fx, over, what):
    _, meta = fx
    with pytest.raises(NotImplementedError, match=what):
        PBATransformerForConditionalGeneration(_cfg(meta, "a", **over))


# ---- names, shapes, state dict, init -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_state_dict_keys_and_shapes_are_the_reference_classes(fx, name):
    _, meta = fx
    m = PBATransformerForConditionalGeneration(_cfg(meta, name))
    sd = m.state_dict()
    assert list(sd) == meta[name]["keys"]
    assert [list(v.shape) for v in sd.values()] == meta[name]["shapes"]
    assert [k for k, _ in m.named_parameters()] == meta[name]["param_keys"]
    for k in pw.TIED[1:]:
        assert sd[k].data_ptr() == sd["shared.weight"].data_ptr()
    if name == "a":
        assert sd["encoder.block.0.layer.1.mlp.mlp.wi.weight"].shape == (96, 64 + 16)
        assert sd["encoder.block.0.layer.1.mlp.behavior_embedding.weight"].shape == (3, 16)
        assert sd["decoder.block.1.layer.2.mlp.experts.expert_4.wi.weight"].shape == (96, 64)
        assert "encoder.block.1.layer.1.mlp.experts.expert_0.wo.weight" in sd and "encoder.block.1.layer.1.layer_norm.weight" in sd


def test_a_reference_named_state_dict_round_trips(fx):
    z, meta = fx
    shapes = OrderedDict(zip(meta["a"]["keys"], [tuple(s) for s in meta["a"]["shapes"]]))
    sd = pw.init_state_dict(shapes, meta["a"]["weight_seed"])
    assert np.allclose(pw.checksums(sd), z["a/weight_checksums"], rtol=1e-12, atol=1e-9)
    m = PBATransformerForConditionalGeneration(_cfg(meta, "a"))
    m.load_state_dict(sd, strict=True)
    out = m.state_dict()
    assert list(out) == list(sd) and all(torch.equal(out[k], sd[k]) for k in sd)
    m2 = PBATransformerForConditionalGeneration(_cfg(meta, "a"))
    m2.load_state_dict(out, strict=True)
    assert m2.lm_head.weight is m2.shared.weight and m2.encoder.embed_tokens is m2.shared
    e = m.resize_token_embeddings(70)
    assert e.weight.shape == (70, 64) and m.lm_head.weight is m.shared.weight and m.config.vocab_size == 70
    assert torch.equal(e.weight[:64], sd["shared.weight"])


def test_init_follows_the_reference_formulas():
    """per tensor, the sample standard deviation within 5 / sqrt(2 n) relative of model.py:69-137's (n values: the sampling error
    of a standard deviation is sigma / sqrt(2 n)); the sparse-MLP branch leaves wi AND wo at d_model ** -0.5"""
    torch.manual_seed(3)
    c = PBATransformerConfig(vocab_size=512, d_model=128, d_kv=64, num_heads=4, d_ff=256, num_layers=2, num_decoder_layers=2,
                             behavior_embedding_dim=64, num_positions=4, num_behavior=7, sparse_layers_encoder=[1], sparse_layers_decoder=[0],
                             behavior_injection_encoder=[0, 1], behavior_injection_decoder=[0], initializer_factor=0.5)
    m = PBATransformerForConditionalGeneration(c)
    f, D = c.initializer_factor, c.d_model
    seen = set()
    for k, p in m.named_parameters():
        if k.endswith("layer_norm.weight"):
            assert bool((p == f).all()), k
            continue
        if k == "shared.weight":
            want = f
        elif k.endswith("behavior_embedding.weight"):
            want = 1.0
        elif k.endswith(("wi.weight", "wo.weight", ".k.weight", ".v.weight", "relative_attention_bias.weight")):
            want = f * D ** -0.5
        elif k.endswith(".q.weight"):
            want = f * (D * c.d_kv) ** -0.5
        elif k.endswith(".o.weight"):
            want = f * (c.num_heads * c.d_kv) ** -0.5
        else:
            raise AssertionError(k)
        seen.add(k.rsplit(".", 2)[-2])
        n = p.numel()
        assert abs(float(p.std()) / want - 1.0) < 5.0 / math.sqrt(2 * n), (k, float(p.std()), want)
        assert abs(float(p.mean())) < 5.0 * want / math.sqrt(n), k
    assert seen >= {"wi", "wo", "q", "k", "v", "o", "behavior_embedding", "relative_attention_bias", "shared"}


# ---- the command's parser -----------------------------------------------------------------------------------------------------------
def test_parse_args_defaults_and_refusals():
    from gamer_amd import train_pbatransformer as cmd
    a = cmd.parse_args([])
    assert (a.backbone, a.base_model, a.tasks, a.test_task) == ("PBATransformer", "./config/s2s-models/PBATransformer", "smb_explicit", "smb_explicit")
    assert (a.max_his_len, a.epochs, a.learning_rate, a.per_device_batch_size, a.gradient_accumulation_steps) == (20, 200, 5e-4, 256, 2)
    assert (a.num_beams, a.test_batch_size, a.temperature, a.model_max_length, a.only_test) == (20, 16, 1.0, 1024, False)
    assert cmd.parse_args(["--tasks", "smb_explicit_decoder_3"]).tasks == "smb_explicit_decoder_3"
    for argv, what in ((["--backbone", "TIGER"], "trains PBATransformer"), (["--tasks", "seqrec"], "train_decoder"),
                       (["--tasks", "mb_explicit"], "train_MB_decoder"), (["--pack_rows"], "packed rows"), (["--bf16"], "bf16"),
                       (["--tasks", "smb"], "smb"), (["--max_his_len", "200"], "max_his_len")):
        with pytest.raises(NotImplementedError, match=what):
            cmd.parse_args(argv)


def test_the_tiger_commands_still_refuse_the_backbone():
    from gamer_amd import train_tiger, train_tiger_smb
    with pytest.raises(NotImplementedError, match="PBATransformer"):
        train_tiger.parse_args(["--backbone", "PBATransformer"])
    with pytest.raises(NotImplementedError, match="PBATransformer"):
        train_tiger_smb.parse_args(["--backbone", "PBATransformer", "--tasks", "smb_explicit"])


def test_the_command_derives_the_config_from_the_data(fx):
    from gamer_amd import train_pbatransformer as cmd
    _, meta = fx

    class Data:
        behaviors = ["click", "cart", "buy"]
        behavior_token_ids = {"buy": 300, "click": 100, "cart": 200}
        token_count = 5
    c = cmd.derive_config(PBATransformerConfig(**meta["shipped_config"]), Data, 30)
    assert c.behavior_maps == {100: 0, 200: 1, 300: 2} and c.num_behavior == 3 and c.use_behavior_token
    assert (c.num_positions, c.num_experts, c.n_positions, c.use_user_token) == (5, 6, 30, False)
    assert c.behavior_injection_encoder == [0, 1] and c.behavior_injection_decoder == [0, 1]
    Data.behavior_token_ids, Data.token_count = {}, 4
    c = cmd.derive_config(PBATransformerConfig(**dict(meta["shipped_config"], Moe_behavior_only=True)), Data, 20)
    assert not c.use_behavior_token and not c.behavior_injection and c.behavior_injection_encoder == [] == c.behavior_injection_decoder
    assert (c.num_positions, c.num_experts, c.num_behavior) == (4, 2, 0)


# ---- the routers ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_host_routers_equal_the_reference_routers(fx, name):
    z, meta = fx
    cfg = meta["configs"][name]
    for tag, ids, decoder in (("enc", z[f"{name}/input_ids"], False), ("dec", z[f"{name}/decoder_input_ids"], True)):
        pos, beh, bad = pref.route_host(ids, cfg, decoder)
        assert pos == z[f"{name}/router/{tag}_pos"].tolist() and beh == z[f"{name}/router/{tag}_beh"].tolist() and bad == 0


def test_host_routers_on_the_worked_example():
    cfg = dict(num_positions=4, n_positions=50, pad_token_id=0, eos_token_id=1, use_behavior_token=True, Moe_behavior_only=False,
               behavior_maps={10: 0, 11: 1})
    enc = [[10, 20, 21, 22, 11, 23, 24, 25, 10, 26, 27, 28, 1], [11, 20, 21, 22, 10, 23, 24, 25, 1, 0, 0, 0, 0]]
    pos, beh, bad = pref.route_host(enc, cfg, False)
    assert pos == [[1, 2, 3, 4, 1, 2, 3, 4, 1, 2, 3, 4, 0], [1, 2, 3, 4, 1, 2, 3, 4, 0, 0, 0, 0, 0]]
    assert beh == [[0, 1, 1, 1, 0, 2, 2, 2, 0, 1, 1, 1, 0], [0, 2, 2, 2, 0, 1, 1, 1, 0, 0, 0, 0, 0]] and bad == 0
    assert pref.route_host([[0, 11, 30, 31, 32]], cfg, True) == ([[0, 1, 2, 3, 4]], [[0, 0, 2, 2, 2]], 0)
    assert pref.route_host([[0]], cfg, True) == ([[0]], [[0]], 0) and pref.route_host([[0, 11]], cfg, True) == ([[0, 1]], [[0, 0]], 0)
    assert pref.route_host(enc[:1], dict(cfg, Moe_behavior_only=True), False)[0] == [[1, 2, 2, 2, 1, 2, 2, 2, 1, 2, 2, 2, 0]]
    assert pref.route_host(enc[:1], dict(cfg, Moe_behavior_only=True, use_behavior_token=False), False)[:2] == ([[1] * 12 + [0]], [[0] * 13])
    assert pref.route_host([[0, 40, 30, 31, 1]], cfg, True) == ([[0, 1, 2, 3, 0]], [[0, 0, 0, 0, 0]], 2)


def test_the_model_has_no_cpu_path(fx):
    z, meta = fx
    m = PBATransformerForConditionalGeneration(_cfg(meta, "a"))
    ids = torch.from_numpy(z["a/input_ids"])
    with pytest.raises(RuntimeError, match="HIP device only"):
        m(ids, torch.ones_like(ids), labels=torch.from_numpy(z["a/labels"]))
    assert "use_cache=False" in pb.beam_search.__doc__ and "cached_input_id_sequence" in pb.beam_search.__doc__


# ---- the restatement the GPU tests measure against ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_the_model_restatement_gives_the_recorded_loss_and_logits_in_fp64(fx, name):
    """an independent statement of the model (shared relative bias, routed and injected feed-forward layers) agrees with what the
    real classes recorded to the rounding of their fp32 arithmetic: the fixture holds the model, not an accident of the shims"""
    z, meta = fx
    shapes = OrderedDict(zip(meta[name]["keys"], [tuple(s) for s in meta[name]["shapes"]]))
    sd = pw.init_state_dict(shapes, meta[name]["weight_seed"])
    ids, am, labels = (torch.from_numpy(z[f"{name}/{k}"]) for k in ("input_ids", "attention_mask", "labels"))
    loss, logits, grads = pref.restated_model(sd, meta["configs"][name], ids, am, labels, meta["temperature"], dev="cpu", dtype=torch.float64)
    want = torch.from_numpy(z[f"{name}/logits"]).double()
    assert abs(float(loss) - float(z[f"{name}/loss"])) < 1e-5 * float(z[f"{name}/loss"])
    assert float((logits - want).abs().max()) < 1e-4 * float(want.abs().max())
    k = "decoder.block.0.layer.2.mlp.experts.expert_1.wi.weight"
    g = torch.from_numpy(z[f"{name}/grad/{k}"]).double()
    assert float((grads[k][pw.sample_rows(grads[k].shape)] - g).abs().max()) < 1e-4 * float(g.abs().max())
