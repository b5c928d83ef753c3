"""TIGER on packed rows, the parts that need no GPU: the offsets and the right-padding rule, the ``--pack_rows`` flag of the three
commands, and the argument checks of the packed attention wrappers, which refuse before the library is touched."""
import pytest
import torch


def test_offsets_from_lengths():
    from gamer_amd import ops
    off = ops.T5Offsets.from_lengths(torch.tensor([23, 9, 0, 1]))
    assert off.host.dtype == torch.int32 and off.host.tolist() == [0, 23, 32, 32, 33]
    assert (off.n, off.total, off.max_len) == (4, 33, 23) and off.dev is None
    assert ops.T5Offsets.uniform(3, 5).host.tolist() == [0, 5, 10, 15]
    with pytest.raises(ValueError, match="start at 0"):
        ops.T5Offsets(torch.tensor([1, 4, 9]))
    with pytest.raises(ValueError, match="decrease at row 1"):
        ops.T5Offsets(torch.tensor([0, 4, 3, 9]))
    with pytest.raises(ValueError, match="none negative"):
        ops.T5Offsets.from_lengths(torch.tensor([3, -1]))


def test_lengths_of_right_padded_masks_and_the_refusal_of_every_other_form():
    from gamer_amd import tiger
    mask = torch.tensor([[1, 1, 1, 1], [1, 1, 0, 0], [0, 0, 0, 0], [1, 0, 0, 0]])
    assert tiger.packed_lengths(mask).tolist() == [4, 2, 0, 1]             # (an all-zero row is a row of no tokens)
    with pytest.raises(ValueError, match="row 1 "):                         # left padding
        tiger.packed_lengths(torch.tensor([[1, 1, 1, 1], [0, 0, 1, 1]]))
    with pytest.raises(ValueError, match="row 2 "):                         # a hole
        tiger.packed_lengths(torch.tensor([[1, 1, 1, 1], [1, 0, 0, 0], [1, 0, 1, 1]]))
    with pytest.raises(ValueError, match=r"\[B, S\]"):
        tiger.packed_lengths(torch.ones(4))


def test_packed_rows_index_the_kept_tokens():
    from gamer_amd import tiger
    pack = tiger.PackedRows.build(torch.tensor([3, 0, 1]), 3, 4, "cpu")
    assert pack.off.host.tolist() == [0, 3, 3, 4] and pack.S == 4 and pack.rows.tolist() == [0, 1, 2, 8]
    with pytest.raises(ValueError, match="row 1 holds 5 tokens of 4"):
        tiger.PackedRows.build(torch.tensor([3, 5, 1]), 3, 4, "cpu")
    with pytest.raises(ValueError, match="no token"):
        tiger.PackedRows.build(torch.tensor([0, 0]), 2, 4, "cpu")
    with pytest.raises(ValueError, match=r"CPU int tensor \[3\]"):
        tiger.PackedRows.build(torch.tensor([3, 1]), 3, 4, "cpu")


def test_pack_rows_is_off_by_default_in_the_three_commands():
    from gamer_amd import train_tiger, train_tiger_mb, train_tiger_smb
    assert train_tiger.parse_args([]).pack_rows is False and train_tiger.parse_args(["--pack_rows"]).pack_rows is True
    assert train_tiger_smb.parse_args(["--tasks", "smb_explicit"]).pack_rows is False
    assert train_tiger_smb.parse_args(["--tasks", "smb_explicit", "--pack_rows"]).pack_rows is True
    assert train_tiger_mb.parse_args(["--tasks", "mb"]).pack_rows is False
    assert train_tiger_mb.parse_args(["--tasks", "mb", "--pack_rows"]).pack_rows is True
    a = train_tiger.parse_args([])
    batch = dict(attention_mask=torch.tensor([[1, 1, 0], [1, 0, 0]]))
    assert train_tiger.pack_kwargs(a, batch) == {}
    kw = train_tiger.pack_kwargs(train_tiger.parse_args(["--pack_rows"]), batch)
    assert kw["packed"] is True and kw["lengths"].tolist() == [2, 1] and not kw["lengths"].is_cuda


def test_the_wrappers_refuse_before_the_library_is_touched(monkeypatch):
    from gamer_amd import _lib, ops
    monkeypatch.setattr(_lib, "load", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the library was touched")))
    monkeypatch.setattr(ops, "call", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the library was touched")))
    t, lse = torch.zeros(11, 64), torch.zeros(11)
    off = ops.T5Offsets.from_lengths(torch.tensor([8, 3]))
    fwd = lambda f, max_s, o=off, h=1, d=64: f(t, t, t, None, o, o, 2, max_s, max_s, h, d, False, 0.0, 0, t, lse)
    bwd = lambda f, max_s, o=off: f(t, t, t, None, o, o, 2, max_s, max_s, 1, 64, False, 0.0, 0, t, lse, t, t, t, None)
    with pytest.raises(ValueError, match="decrease"):                      # decreasing offsets never become a T5Offsets
        ops.T5Offsets(torch.tensor([0, 8, 5]))
    for f in (ops.t5_attn_packed_fwd, ops.t5_attn_long_packed_fwd):
        with pytest.raises(ValueError, match="row 0 of q_start holds 8 tokens, more than max 7"):
            fwd(f, 7)
        with pytest.raises(NotImplementedError):
            fwd(f, 8, h=17)
        with pytest.raises(NotImplementedError):
            fwd(f, 8, d=48)
        with pytest.raises(RuntimeError, match="T5Offsets of 2 rows"):
            fwd(f, 8, o=ops.T5Offsets.from_lengths(torch.tensor([8, 2, 1])))
    for f in (ops.t5_attn_packed_bwd, ops.t5_attn_long_packed_bwd):
        with pytest.raises(ValueError, match="more than max 7"):
            bwd(f, 7)
    # the wrong family: the resident wrappers stop at 128, the key-streaming ones at 512
    with pytest.raises(NotImplementedError, match="Sq, Sk <= 128"):
        fwd(ops.t5_attn_packed_fwd, 129)
    with pytest.raises(NotImplementedError, match="Sq, Sk <= 128"):
        bwd(ops.t5_attn_packed_bwd, 129)
    with pytest.raises(NotImplementedError, match="Sq, Sk <= 512"):
        fwd(ops.t5_attn_long_packed_fwd, 513)
    with pytest.raises(RuntimeError, match="device copy"):                 # (offsets without a device copy: no CPU path, no library call)
        fwd(ops.t5_attn_long_packed_fwd, 129)


def test_forward_refuses_a_bad_mask_before_any_kernel(monkeypatch):
    from gamer_amd import tiger
    m = tiger.TIGER(tiger.TigerConfig(vocab_size=40, d_model=32, d_kv=32, d_ff=64, num_layers=1, num_heads=1))
    ids = torch.ones(2, 4, dtype=torch.long)
    with pytest.raises(ValueError, match="row 1 "):
        m._pack(ids, torch.tensor([[1, 1, 1, 1], [0, 1, 1, 1]]), None)
    with pytest.raises(ValueError, match=r"CPU int tensor \[2\]"):
        m._pack(ids, None, torch.tensor([4, 4, 4]))
