"""gamer_moe_action_router_prep, Qwen3MoeAction's one prep launch: ``expert`` (the FFN's index) and ``act_idx`` against the
torch restatement of the reference's routing (tests/helpers/moe_action_routing.py, itself held equal to the real router's
stored outputs on the CPU), every other output bit for bit against gamer_moe_router_prep on the same input - integer work, so
equal means equal - and gamer_expert_lists over the resulting index with 21 groups.  Lengths at P = 5: one token, S = n P,
S = n P + 1 with a non-special last token (6 and 46), a ragged tail (33), and more than one scan block (2048)."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

import moe_action_routing as routing  # noqa: E402
from gamer_amd import ops, synthetic  # noqa: E402
from gamer_amd.config import Qwen3MoeActionConfig  # noqa: E402

DEV = "cuda"
CB, NB, P, B = 8, 4, 5, 3
N_ITEMS = 410                                   # the router's table: 410 * 5 + 1 = 2051 >= 2048
SHARED_KEYS = ("beh_idx", "kl_self", "empty_self", "tile_empty_self", "bad_token")


def _config(behavior_only: bool):
    cfg = Qwen3MoeActionConfig(vocab_size=synthetic.vocab_size(CB, NB), num_positions=P, n_positions=N_ITEMS,
                               Moe_behavior_only=behavior_only, num_experts=2 if behavior_only else P + 1, num_behavior=NB,
                               behavior_maps={str(k): v for k, v in synthetic.behavior_maps(CB, NB).items()})
    cfg.validate()
    return cfg


def _inputs(S: int, left: bool, seed: int):
    """B rows of items (behaviour token + 4 semantic tokens) kept over S, 2/3 S and 1/3 S tokens, padded elsewhere.  Row 0
    keeps every token, so its last one is NOT special; it has an item start outside behavior_maps (bad_token).  Row 1 has an
    eos inside its kept part."""
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(S)
    ids = synthetic.N_SPECIAL + CB * ((t % P).clamp(min=1) - 1)[None, :] + torch.randint(0, CB, (B, S), generator=g)
    beh = synthetic.N_SPECIAL + 4 * CB + torch.randint(0, NB, (B, S), generator=g)
    ids = torch.where((t % P == 0)[None, :], beh, ids)
    kept = [S, max(1, 2 * S // 3), max(1, S // 3)]
    am = torch.zeros(B, S, dtype=torch.int64)
    for b, n in enumerate(kept):
        if left:
            am[b, S - n:] = 1
        else:
            am[b, :n] = 1
    ids = torch.where(am.bool(), ids, torch.full_like(ids, synthetic.PAD_ID))
    if S >= 5:
        ids[0, (S // 2) // P * P] = synthetic.N_SPECIAL + 1          # a semantic token where an item starts
        ids[1, int(am[1].nonzero()[1])] = synthetic.EOS_ID
    return ids, am


def _outputs(S: int):
    i32 = dict(dtype=torch.int32, device=DEV)
    out = {k: torch.full((B, S), -7, **i32) for k in ("expert", "beh_idx", "act_idx", "kl_self", "empty_self")}
    out["tile_empty_self"] = torch.full((B, (S + 31) // 32), -7, **i32)
    out["bad_token"] = torch.zeros(1, **i32)
    return out


def _table(cfg):
    tbl = cfg.position_experts()
    return None if tbl == list(range(1, P + 1)) else torch.tensor(tbl, dtype=torch.int32, device=DEV)


@pytest.mark.parametrize("S", [1, 5, 6, 33, 46, 2048])
def test_launch_equals_the_restated_routing_and_the_router_prep(S):
    for left in (False, True):
        ids_c, am_c = _inputs(S, left, seed=S + int(left))
        ids, am = ids_c.to(DEV).contiguous(), am_c.to(DEV).contiguous()
        for behavior_only in (False, True):
            cfg = _config(behavior_only)
            E, n_ffn = cfg.num_experts, cfg.num_ffn_experts
            lut = cfg.behavior_lut().to(DEV)
            full = torch.tensor(cfg.position_experts(), dtype=torch.int32, device=DEV)
            # the table as the engine passes it (NULL for the shipped one) and, for the shipped one, spelled out
            for table in ([_table(cfg)] if behavior_only else [None, full]):
                for zero_col in ([None] if S < 6 else [None, S - 3]):
                    tag = (S, left, behavior_only, table is None, zero_col)
                    got, ref = _outputs(S), _outputs(S)
                    i32 = dict(dtype=torch.int32, device=DEV)
                    pos, pos_r = torch.full((B, S), -7, **i32), torch.full((B, S), -7, **i32)
                    nxt, nxt_r = torch.full((B,), -7, **i32), torch.full((B,), -7, **i32)
                    ops.moe_action_router_prep(ids, am, lut, table, P, N_ITEMS, True, cfg.pad_token_id, cfg.eos_token_id, E - 1,
                                               n_ffn, got, pos_ids=pos, next_pos=nxt, act_zero_col=zero_col)
                    ops.moe_router_prep(ids, am, lut, table, P, N_ITEMS, True, cfg.pad_token_id, cfg.eos_token_id, ref,
                                        pos_ids=pos_r, next_pos=nxt_r)
                    for k in SHARED_KEYS:
                        assert torch.equal(got[k], ref[k]), (tag, k)
                    assert torch.equal(pos, pos_r) and torch.equal(nxt, nxt_r), tag
                    want = routing.route(ids_c, P, E, cfg.behavior_maps, cfg.pad_token_id, cfg.eos_token_id,
                                         cfg.position_experts(), N_ITEMS, act_zero_col=zero_col)
                    assert torch.equal(got["act_idx"].cpu().long(), want["action"]), tag
                    assert torch.equal(got["expert"].cpu().long(), want["ffn_index"]), tag
                    assert torch.equal(ref["expert"].cpu().long(), want["position"]), tag
                    assert torch.equal(got["beh_idx"].cpu().long(), want["behavior"]), tag
                    assert int(got["bad_token"]) == want["bad_token"] == (1 if S >= 5 else 0), tag
                    assert all(int((v == -7).sum()) == 0 for v in list(got.values()) + [pos, nxt]), tag
                    # what the inputs were built to trigger
                    act = got["act_idx"].cpu()
                    if S % P == 1:                                      # S = n P + 1: action 0 in the last column, not special
                        assert int(ids_c[0, S - 1]) not in (cfg.pad_token_id, cfg.eos_token_id), tag
                        assert int(act[0, S - 1]) == 0 and int(got["expert"][0, S - 1]) == 0, tag
                    elif zero_col is None and S >= 10:
                        assert int(act[0, S - 1]) > 0, tag
                    if S >= 10:                                         # (shorter: row 0's first item is the bad one)
                        assert int(act[0, 0]) > 0, tag                   # the behaviour token carries its own action
                    if zero_col is not None:
                        assert int(act[:, zero_col].abs().sum()) == 0, tag
                    if behavior_only and S == 2048:
                        assert int(got["expert"].max()) == n_ffn, tag    # rows whose index names no expert
    # without a mask every token is kept
    cfg = _config(False)
    ids_c, _ = _inputs(S, False, seed=S)
    got = _outputs(S)
    ops.moe_action_router_prep(ids_c.to(DEV), None, cfg.behavior_lut().to(DEV), None, P, N_ITEMS, True, cfg.pad_token_id,
                               cfg.eos_token_id, P, cfg.num_ffn_experts, got)
    assert int(got["kl_self"].abs().sum()) == 0
    assert torch.equal(got["expert"].cpu().long(), routing.route(ids_c, P, P + 1, cfg.behavior_maps, cfg.pad_token_id,
                                                                 cfg.eos_token_id, cfg.position_experts(), N_ITEMS)["ffn_index"])


@pytest.mark.parametrize("S", [6, 46, 2048])
def test_expert_lists_over_the_action_index_with_21_groups(S):
    cfg = _config(False)
    n_ffn = cfg.num_ffn_experts
    assert n_ffn == 21
    ids_c, am_c = _inputs(S, False, seed=7 * S)
    # the rows use behaviours 0 and 2 only: the experts of behaviours 1 and 3 are empty groups
    first = ids_c[:, 0::P]
    tok = [synthetic.behavior_token(b, CB) for b in range(NB)]
    first[first == tok[1]] = tok[0]
    first[first == tok[3]] = tok[2]
    ids_c[:, 0::P] = torch.where(am_c[:, 0::P].bool(), first, torch.full_like(first, synthetic.PAD_ID))
    got = _outputs(S)
    ops.moe_action_router_prep(ids_c.to(DEV), am_c.to(DEV), cfg.behavior_lut().to(DEV), None, P, N_ITEMS, True, cfg.pad_token_id,
                               cfg.eos_token_id, P, n_ffn, got)
    T = B * S
    i32 = dict(dtype=torch.int32, device=DEV)
    perm, slot, offsets = torch.full((T,), -7, **i32), torch.full((T,), -7, **i32), torch.full((n_ffn + 1,), -7, **i32)
    ops.expert_lists(got["expert"], n_ffn, perm, slot, offsets, torch.zeros((B + 1) * n_ffn, **i32))
    e = got["expert"].cpu().long().view(-1)
    counts = torch.bincount(e, minlength=n_ffn)
    assert int((counts == 0).sum()) >= 2 * P                               # several empty groups
    assert torch.equal(offsets.cpu().long(), torch.cat([torch.zeros(1, dtype=torch.int64), counts.cumsum(0)]))
    assert torch.equal(perm.cpu().long().sort().values, torch.arange(T))
    assert torch.equal(slot.cpu().long().sort().values, torch.arange(T))
    assert torch.equal(slot.cpu().long()[perm.cpu().long()], torch.arange(T))
    # expert-major, then token order
    sorted_e = e[perm.cpu().long()]
    assert bool((sorted_e[1:] >= sorted_e[:-1]).all())
    same = sorted_e[1:] == sorted_e[:-1]
    assert bool((perm.cpu().long()[1:][same] > perm.cpu().long()[:-1][same]).all())


def test_host_refuses_bad_arguments_without_a_launch():
    cfg = _config(False)
    ids_c, am_c = _inputs(47, False, seed=3)
    ids, am, lut = ids_c.to(DEV), am_c.to(DEV), cfg.behavior_lut().to(DEV)
    args = (P, 9, True, cfg.pad_token_id, cfg.eos_token_id, P)
    got = _outputs(47)
    with pytest.raises(RuntimeError, match="gamer_moe_action_router_prep.*router's table"):
        ops.moe_action_router_prep(ids, am, lut, None, *args, 21, got)
    with pytest.raises(ValueError, match="at most 64 groups"):
        ops.moe_action_router_prep(ids, am, lut, None, P, N_ITEMS, True, cfg.pad_token_id, cfg.eos_token_id, P, 65, got)
    with pytest.raises(RuntimeError, match="act_zero_col"):
        ops.moe_action_router_prep(ids, am, lut, None, P, N_ITEMS, True, cfg.pad_token_id, cfg.eos_token_id, P, 21, got,
                                   act_zero_col=47)
    torch.cuda.synchronize()
    assert all(bool((got[k] == -7).all()) for k in ("expert", "beh_idx", "act_idx", "kl_self", "empty_self", "tile_empty_self"))
    assert int(got["bad_token"]) == 0
