"""TIGER at encoder lengths up to 512 without a GPU: the constants and limits of the key-streaming attention kernels, the length
checks of the model and of the train command, and the bucket vector at 512 against HF's (tests/golden/tiger_long.npz,
tools/make_golden_tiger_long.py)."""
import json
import os

import numpy as np
import pytest
import torch

from gamer_amd import ops, tiger, train_tiger

FX = os.path.join(os.path.dirname(__file__), "golden", "tiger_long.npz")
SMALL = dict(d_model=64, d_kv=64, d_ff=128, num_layers=2, num_decoder_layers=2, num_heads=2, vocab_size=120)


class _FakeCuda:
    """what _check reads of a tensor"""
    is_cuda = True

    def __init__(self, *shape):
        self.shape = shape

    def dim(self):
        return len(self.shape)


def test_long_limits():
    assert ops.T5_LONG_MAX_S == 512 and ops.T5_MAX_S == 128
    ops.t5_long_check_limits(512, 512, 16, 32)
    ops.t5_long_check_limits(1, 1, 1, 64)
    for Sq, Sk, h, d in ((513, 8, 1, 64), (8, 513, 1, 64), (8, 8, 17, 64), (8, 8, 1, 48), (0, 8, 1, 64), (8, 0, 1, 64), (8, 8, 0, 64)):
        with pytest.raises(NotImplementedError, match="512"):
            ops.t5_long_check_limits(Sq, Sk, h, d)
    # the resident family keeps its own bound
    with pytest.raises(NotImplementedError):
        ops.t5_check_limits(129, 8, 1, 64)


def test_encoder_length_constants_and_checks():
    assert tiger.MAX_LONG_ENCODER_LEN == 512 and tiger.MAX_ENCODER_LEN == 128 and tiger.MAX_DECODER_LEN == 8
    m = tiger.TIGER(tiger.TigerConfig(**SMALL))
    m._check(_FakeCuda(1, 512), tiger.MAX_LONG_ENCODER_LEN, "encoder")
    with pytest.raises(NotImplementedError, match=r"encoder length in \[1, 512\]"):
        m._check(_FakeCuda(1, 513), tiger.MAX_LONG_ENCODER_LEN, "encoder")


def test_the_model_checks_the_encoder_against_the_long_limit(monkeypatch):
    """encode and forward hand the long limit to _check (a 129-token encoder is no longer refused by length)"""
    m = tiger.TIGER(tiger.TigerConfig(**SMALL))
    seen = []

    class Stop(Exception):
        pass

    def check(ids, limit, what):
        seen.append((what, limit))
        raise Stop
    monkeypatch.setattr(m, "_check", check)
    ids = torch.ones(1, 129, dtype=torch.long)
    with pytest.raises(Stop):
        m.encode(ids)
    with pytest.raises(Stop):
        m(ids, labels=torch.ones(1, 3, dtype=torch.long))
    assert seen == [("encoder", 512), ("encoder", 512)]


def test_attention_dispatch_picks_the_family_by_shape(monkeypatch):
    calls = []
    for name in ("t5_attn_fwd", "t5_attn_long_fwd", "t5_attn_bwd", "t5_attn_long_bwd"):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **kw: calls.append((_n, a[6], a[7])))
    for Sq, Sk in ((128, 128), (5, 128), (129, 129), (5, 129), (8, 512)):
        tiger._attn_fwd(None, None, None, None, None, 1, Sq, Sk, 2, 64, False, 0.0, 0, None, None)
        tiger._attn_bwd(None, None, None, None, None, 1, Sq, Sk, 2, 64, False, 0.0, 0, None, None, None, None, None, None)
    assert calls == [("t5_attn_fwd", 128, 128), ("t5_attn_bwd", 128, 128), ("t5_attn_fwd", 5, 128), ("t5_attn_bwd", 5, 128),
                     ("t5_attn_long_fwd", 129, 129), ("t5_attn_long_bwd", 129, 129), ("t5_attn_long_fwd", 5, 129),
                     ("t5_attn_long_bwd", 5, 129), ("t5_attn_long_fwd", 8, 512), ("t5_attn_long_bwd", 8, 512)]


def test_train_tiger_refuses_a_longer_model_max_length_when_parsing():
    assert train_tiger.parse_args(["--model_max_length", "512", "--max_his_len", "100"]).model_max_length == 512
    assert train_tiger.parse_args([]).model_max_length == 512
    for n in ("513", "0"):
        with pytest.raises(NotImplementedError, match="512"):
            train_tiger.parse_args(["--model_max_length", n])


@pytest.mark.parametrize("bidirectional", [True, False])
def test_bucket_vector_at_512_equals_hf(bidirectional):
    z = np.load(FX)
    meta = json.loads(str(z["meta_json"]))
    cfg = meta["configs"]["c"]
    got = tiger.bucket_vector(512, bidirectional, cfg["relative_attention_num_buckets"], cfg["relative_attention_max_distance"])
    want = z[f"bucket/{'bi' if bidirectional else 'uni'}/512"]
    assert got.dtype == torch.int32 and got.shape == (1023,) and np.array_equal(got.numpy(), want)
    assert int(got.min()) >= 0 and int(got.max()) < cfg["relative_attention_num_buckets"]
