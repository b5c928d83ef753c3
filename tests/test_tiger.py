"""TIGER without a GPU: the config, the state dict against HF's (tests/golden/tiger_small.npz holds the key list and shapes of the
real class), initialisation, refusals and limits, the host-side bucket vector and the train command's defaults."""
import json
import math
import os
import sys
from collections import OrderedDict

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import tiger_weights as tw  # noqa: E402

from gamer_amd import ops, rec_common, tiger, train_tiger  # noqa: E402

FX = os.path.join(os.path.dirname(__file__), "golden", "tiger_small.npz")
SMALL = dict(d_model=64, d_kv=64, d_ff=128, num_layers=2, num_decoder_layers=2, num_heads=2, vocab_size=120)


@pytest.fixture(scope="module")
def fx():
    z = np.load(FX)
    return z, json.loads(str(z["meta_json"]))


def test_config_defaults_and_dropped_keys(fx, tmp_path):
    _, meta = fx
    shipped = meta["shipped_config"]
    (tmp_path / "config.json").write_text(json.dumps(dict(
        {k: v for k, v in shipped.items() if k not in ("num_decoder_layers", "relative_attention_max_distance", "feed_forward_proj",
                                                        "tie_word_embeddings")},
        architectures=["T5ForConditionalGeneration"], task_specific_params={"summarization": {"num_beams": 4}}, n_positions=512,
        output_past=True, model_type="t5", is_encoder_decoder=True)))
    cfg = tiger.TigerConfig.from_pretrained(str(tmp_path))
    assert cfg.to_dict() == shipped                                  # (the keys the file is silent about take T5Config's defaults)
    assert not hasattr(cfg, "task_specific_params") and not hasattr(cfg, "n_positions")
    assert tiger.TigerConfig(num_layers=3).num_decoder_layers == 3
    with pytest.raises(ValueError, match="configuration file"):
        tiger.TigerConfig.from_pretrained(str(tmp_path / "nowhere"))


@pytest.mark.parametrize("name", ["a", "b"])
def test_state_dict_keys_shapes_and_aliases_equal_hf(fx, name):
    _, meta = fx
    m = tiger.TIGER(tiger.TigerConfig(**meta["configs"][name]))
    sd = m.state_dict()
    assert list(sd) == meta[name]["keys"]
    assert [list(v.shape) for v in sd.values()] == meta[name]["shapes"]
    assert len({sd[k].data_ptr() for k in tw.TIED}) == 1
    assert [k for k, _ in m.named_parameters()] == meta[name]["param_keys"]
    assert "encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight" in sd
    assert "encoder.block.1.layer.0.SelfAttention.relative_attention_bias.weight" not in sd


def test_state_dict_round_trip(fx, tmp_path):
    _, meta = fx
    torch.manual_seed(1)
    a = tiger.TIGER(tiger.TigerConfig(**meta["configs"]["a"]))
    torch.save(a.state_dict(), tmp_path / "m.pth")
    b = tiger.TIGER(tiger.TigerConfig(**meta["configs"]["a"]))
    b.load_state_dict(torch.load(tmp_path / "m.pth"), strict=True)
    for (k, x), (_, y) in zip(a.state_dict().items(), b.state_dict().items()):
        assert torch.equal(x, y), k
    assert b.lm_head.weight is b.shared.weight and b.encoder.embed_tokens is b.shared and b.decoder.embed_tokens is b.shared
    # the pinned weights of the fixture load under HF's names
    shapes = OrderedDict(zip(meta["a"]["keys"], [tuple(s) for s in meta["a"]["shapes"]]))
    b.load_state_dict(tw.init_state_dict(shapes, meta["a"]["weight_seed"]), strict=True)


def test_init_standard_deviations_follow_hf(fx):
    _, meta = fx
    c = meta["shipped_config"]
    torch.manual_seed(0)
    m = tiger.TIGER(tiger.TigerConfig(**dict(c, vocab_size=2000)))
    D, dkv, h, dff = c["d_model"], c["d_kv"], c["num_heads"], c["d_ff"]
    want = {".q.weight": (D * dkv) ** -0.5, ".k.weight": D ** -0.5, ".v.weight": D ** -0.5, ".o.weight": (h * dkv) ** -0.5,
            ".wi.weight": D ** -0.5, ".wo.weight": dff ** -0.5, "shared.weight": 1.0, "relative_attention_bias.weight": D ** -0.5}
    seen = set()
    for k, p in m.named_parameters():
        if k.endswith("layer_norm.weight"):
            assert bool((p == 1).all()), k
            continue
        suffix = next(s for s in want if k.endswith(s))
        seen.add(suffix)
        assert abs(float(p.detach().std()) - want[suffix]) < 0.1 * want[suffix], (k, float(p.detach().std()), want[suffix])
    assert seen == set(want)


def test_refusals_and_limits(fx):
    _, meta = fx
    cfg = lambda **kw: tiger.TigerConfig(**dict(SMALL, **kw))
    for kw in (dict(feed_forward_proj="gated-gelu"), dict(tie_word_embeddings=False), dict(d_kv=16), dict(d_kv=128), dict(d_model=258),
               dict(d_model=512), dict(num_heads=17)):
        with pytest.raises(NotImplementedError):
            tiger.TIGER(cfg(**kw))
    m = tiger.TIGER(cfg())
    ids = torch.ones(2, 5, dtype=torch.long)
    with pytest.raises(RuntimeError, match="HIP device only"):      # no CPU fallback
        m(ids, torch.ones_like(ids), labels=ids)
    for name in ("head_mask", "inputs_embeds", "output_attentions", "decoder_head_mask"):
        with pytest.raises(NotImplementedError, match=name):
            m(ids, torch.ones_like(ids), labels=ids, **{name: True})
    with pytest.raises(ValueError, match="decoder_input_ids or labels"):
        m(ids, torch.ones_like(ids))
    # lengths are checked before any launch
    with pytest.raises(NotImplementedError, match="encoder length"):
        m._check(_FakeCuda(1, 129), tiger.MAX_ENCODER_LEN, "encoder")
    with pytest.raises(NotImplementedError, match="decoder length"):
        m._check(_FakeCuda(1, 9), tiger.MAX_DECODER_LEN, "decoder")
    for Sq, Sk, h, d in ((129, 8, 2, 64), (8, 129, 2, 64), (8, 8, 17, 64), (8, 8, 2, 48), (0, 8, 2, 64)):
        with pytest.raises(NotImplementedError):
            ops.t5_check_limits(Sq, Sk, h, d)
    ops.t5_check_limits(128, 128, 16, 32)
    assert 1 <= ops.t5_n_slab(3, 6) <= 3 and ops.t5_n_slab(1024, 6) * 6 <= 512


class _FakeCuda:
    """what _check reads of a tensor"""
    is_cuda = True

    def __init__(self, *shape):
        self.shape = shape

    def dim(self):
        return len(self.shape)


def test_shift_right_and_resize(fx):
    m = tiger.TIGER(tiger.TigerConfig(**SMALL))
    labels = torch.tensor([[5, 6, 1, -100], [7, 1, -100, -100]])
    assert m._shift_right(labels).tolist() == [[0, 5, 6, 1], [0, 7, 1, 0]]
    old = m.shared.weight.detach().clone()
    emb = m.resize_token_embeddings(150)
    sd = m.state_dict()
    assert emb is m.shared and m.config.vocab_size == 150 and all(sd[k].shape == (150, 64) for k in tw.TIED)
    assert len({sd[k].data_ptr() for k in tw.TIED}) == 1 and torch.equal(m.shared.weight[:120], old)
    m.set_hyper(0.7)
    assert m.temperature == 0.7


@pytest.mark.parametrize("S", [1, 8, 101, 128, 300])
@pytest.mark.parametrize("bidirectional", [True, False])
def test_bucket_vector_equals_hf(fx, S, bidirectional):
    z, _ = fx
    got = tiger.bucket_vector(S, bidirectional, 32, 128)
    assert got.dtype == torch.int32 and got.shape == (2 * S - 1,)
    assert np.array_equal(got.numpy(), z[f"bucket/{'bi' if bidirectional else 'uni'}/{S}"])


def test_shared_grad_hands_over_to_a_second_gather():
    one = rec_common._SharedGrad()                                  # what the existing models see: one gather, which returns the buffer
    one.dE = torch.ones(2, 2)
    t = rec_common._SharedGrad.take(one, (2, 2), "cpu")
    assert one.dE is None and rec_common._SharedGrad.give(one, t) is t
    two = rec_common._SharedGrad(gathers=2)
    two.dE = torch.ones(2, 2)
    t = rec_common._SharedGrad.take(two, (2, 2), "cpu")
    assert rec_common._SharedGrad.give(two, t) is None and two.dE is t
    t2 = rec_common._SharedGrad.take(two, (2, 2), "cpu")
    assert t2 is t and rec_common._SharedGrad.give(two, t2) is t and two.dE is None
    assert rec_common._SharedGrad.give(None, t) is t


def test_train_tiger_defaults_are_train_decoders(fx):
    _, meta = fx
    ref = meta["train_decoder_defaults"]
    a = vars(train_tiger.parse_args([]))
    for k in ("seed", "backbone", "base_model", "output_dir", "data_path", "tasks", "dataset", "index_file", "max_his_len", "optim",
              "epochs", "learning_rate", "per_device_batch_size", "model_max_length", "weight_decay", "warmup_ratio",
              "lr_scheduler_type", "patience", "temperature", "resume_from_checkpoint", "fp16", "bf16", "deepspeed"):
        assert a[k] == ref[k], (k, a[k], ref[k])
    assert a["num_beams"] == 20 and a["only_test"] is False
    for flag in (["--fp16"], ["--bf16"], ["--deepspeed", "ds.json"], ["--resume_from_checkpoint", "x"]):
        with pytest.raises(NotImplementedError, match=flag[0][2:]):
            train_tiger.parse_args(flag)
    with pytest.raises(NotImplementedError):
        train_tiger.parse_args(["--backbone", "PBATransformer"])


def test_synthetic_seqrec_dataset_loads(tmp_path):
    from gamer_amd import synthetic
    from gamer_amd.seqrec_data import EncoderDecoderCollator, SeqRecData
    synthetic.write_seqrec_dataset(str(tmp_path), "Toy", n_users=40, n_items=60, codebook=8, seed=1)
    data = SeqRecData(str(tmp_path), "Toy")
    assert len(data.item_ptr) - 1 == 60 and len(data.all_items()[1]) == 0 and data.vocab_size == 32100 + 32
    train = data.samples("train", 10)
    assert len(train) > 40 and len(data.samples("test", 10)) == 40
    b = EncoderDecoderCollator(data)(train, [0, 1, 2])
    assert b["labels"].shape == (3, 5) and b["input_ids"].shape[1] <= 41


def test_abi_symbols_cover_the_new_prototypes():
    from gamer_amd import _lib
    syms = set(_lib.header_symbols())
    new = {"gamer_t5_attn_fwd", "gamer_t5_attn_bwd", "gamer_t5_bias_expand", "gamer_t5_bias_fold"}
    assert new <= syms and new <= set(_lib._SIGNATURES)
    assert len(_lib._SIGNATURES["gamer_t5_attn_fwd"]) == 21 and len(_lib._SIGNATURES["gamer_t5_attn_bwd"]) == 28
