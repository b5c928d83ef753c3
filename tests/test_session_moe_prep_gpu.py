"""gamer_session_moe_prep, Qwen3SessionMoe's one prep launch, bit for bit against the two kernels it is built from:
``expert`` / ``beh_idx`` / ``bad_token`` are gamer_moe_router_prep's and ``kl_self`` / ``span_self`` / ``pos_ids`` /
``empty_self`` / ``tile_empty_self`` / ``violations`` are gamer_session_prep's for the same inputs - integer work, so equal
means equal.  Lengths: one token, one item, not a whole number of items, the fixtures' 46 and the LDS bound 2048."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from gamer_amd import ops, synthetic  # noqa: E402
from gamer_amd.config import Qwen3SessionMoeConfig  # noqa: E402

DEV = "cuda"
CB, NB, P, B = 8, 3, 5, 3
N_ITEMS = 410                                   # the router's table: 410 * 5 + 1 = 2051 >= 2048
ROUTER_KEYS = ("expert", "beh_idx", "bad_token")
MASK_KEYS = ("kl_self", "span_self", "pos_ids", "empty_self", "tile_empty_self", "violations")


def _config(behavior_only: bool, use_beh: bool):
    kw = dict(vocab_size=synthetic.vocab_size(CB, NB), num_positions=P, model_max_length=4096, n_positions=N_ITEMS,
              Moe_behavior_only=behavior_only, num_experts=2 if behavior_only else P + 1)
    if use_beh:
        kw.update(num_behavior=NB, behavior_maps={str(k): v for k, v in synthetic.behavior_maps(CB, NB).items()})
    else:
        kw.update(num_behavior=0, behavior_maps={}, use_behavior_token=False, behavior_injection_decoder=[])
    cfg = Qwen3SessionMoeConfig(**kw)
    cfg.validate()
    return cfg


def _inputs(S: int, left: bool, seed: int):
    """B rows of items (behaviour token + 4 semantic tokens) kept over S, 2/3 S and 1/3 S tokens; sessions of 1, 2 and 3
    items with raw ids that neither start at 0 nor are consecutive; row 2's session ids DECREASE (violations); row 0 has an
    item start outside behavior_maps (bad_token) and, from two tokens on, an eos as its last token."""
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
    ids[0, (S // 2) // P * P] = synthetic.N_SPECIAL + 1          # a semantic token where an item starts
    if S > 1:
        ids[0, S - 1] = synthetic.EOS_ID
    rank = torch.stack([(t // P) // (B - b) for b in range(B)])         # row 0: 3 items per session, row 2: 1
    sid = (2 * rank + 3) * am
    sid[2] = (sid[2].max() + 3 - sid[2]) * am[2]
    ext = ((rank * P + t % P).clamp(max=S - 1)) * am
    return ids, am, sid, ext


def _outputs(S: int):
    i32 = dict(dtype=torch.int32, device=DEV)
    out = {k: torch.full((B, S), -7, **i32) for k in ("expert", "beh_idx", "kl_self", "pos_ids", "empty_self")}
    out["span_self"] = torch.full((B, S, 4), -7, **i32)
    out["tile_empty_self"] = torch.full((B, (S + 31) // 32), -7, **i32)
    out["bad_token"] = torch.zeros(1, **i32)
    out["violations"] = torch.zeros(1, **i32)
    return out


def _table(cfg):
    tbl = cfg.position_experts()
    return None if tbl == list(range(1, P + 1)) else torch.tensor(tbl, dtype=torch.int32, device=DEV)


@pytest.mark.parametrize("S", [1, 5, 33, 46, 2048])
def test_one_launch_equals_the_router_prep_and_the_session_prep(S):
    for left in (False, True):
        ids, am, sid, ext = (x.to(DEV).contiguous() for x in _inputs(S, left, seed=S + int(left)))
        for with_ext in (True, False):
            for behavior_only in (False, True):
                for use_beh in (True, False):
                    cfg = _config(behavior_only, use_beh)
                    lut, table, e = cfg.behavior_lut().to(DEV), _table(cfg), ext if with_ext else None
                    tag = (S, left, with_ext, behavior_only, use_beh)
                    got, ref_r, ref_m = _outputs(S), _outputs(S), _outputs(S)
                    ops.session_moe_prep(ids, am, sid, e, lut, table, P, N_ITEMS, use_beh, cfg.pad_token_id, cfg.eos_token_id,
                                         S, got)
                    ops.moe_router_prep(ids, am, lut, table, P, N_ITEMS, use_beh, cfg.pad_token_id, cfg.eos_token_id, ref_r)
                    ops.session_prep(sid, e, am, P, S, ref_m)
                    for k in ROUTER_KEYS:
                        assert torch.equal(got[k], ref_r[k]), (tag, k)
                    for k in MASK_KEYS:
                        assert torch.equal(got[k], ref_m[k]), (tag, k)
                    assert all(int((got[k] == -7).sum()) == 0 for k in ("expert", "beh_idx", "kl_self", "pos_ids", "empty_self",
                                                                       "tile_empty_self")), tag
                    # what the inputs were built to trigger
                    assert int(got["bad_token"]) == (1 if use_beh else 0), tag
                    if S >= 33:
                        assert int(got["violations"]) > 0, tag
                    if S > 1:
                        assert int(got["expert"][0, S - 1]) == 0, tag                     # eos
                    if behavior_only and use_beh and S >= 5:
                        assert got["expert"][1][am[1] != 0].max().item() == 2, tag
    # in-order rows alone raise no violation
    ids, am, sid, ext = (x[:2].to(DEV).contiguous() for x in _inputs(S, False, seed=S))
    cfg = _config(False, True)
    got = {k: v[:2].contiguous() if v.dim() > 1 else v for k, v in _outputs(S).items()}
    ops.session_moe_prep(ids, am, sid, ext, cfg.behavior_lut().to(DEV), None, P, N_ITEMS, True, cfg.pad_token_id,
                         cfg.eos_token_id, S, got)
    assert int(got["violations"]) == 0


@pytest.mark.parametrize("S, n_items, what", [(2049, N_ITEMS, "2048"), (47, 9, "router's table")])
def test_host_refuses_lengths_past_the_lds_bound_and_the_routers_table_without_a_launch(S, n_items, what):
    cfg = _config(False, True)
    ids, am, sid, ext = (x.to(DEV).contiguous() for x in _inputs(S, False, seed=3))
    got = _outputs(S)
    with pytest.raises(RuntimeError, match="gamer_session_moe_prep") as err:
        ops.session_moe_prep(ids, am, sid, ext, cfg.behavior_lut().to(DEV), None, P, n_items, True, cfg.pad_token_id,
                             cfg.eos_token_id, S, got)
    assert what in str(err.value)
    torch.cuda.synchronize()
    assert all(bool((got[k] == -7).all()) for k in ("expert", "beh_idx", "kl_self", "span_self", "pos_ids", "empty_self",
                                                    "tile_empty_self"))
    assert int(got["bad_token"]) == 0 and int(got["violations"]) == 0
