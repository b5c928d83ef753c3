"""A torch restatement of Qwen3MoeAction's routing (ref:SeqRec/models/generative/Qwen3Multi/router.py:74-201 called with
cache_position = arange(S), and Qwen3MoeAction/FFN.py:43-44), written from the reference's text and held equal to the router
outputs the real class stored in tests/golden/moe_action_*.npz (tests/test_qwen3moe_action.py).  It is what the GPU tests
compare gamer_moe_action_router_prep with.  CPU only, no gamer_amd import."""
import torch


def route(ids: torch.Tensor, num_positions: int, num_experts: int, behavior_maps: dict, pad_id: int, eos_id: int,
          position_experts, n_items: int, use_behavior_token: bool = True, act_zero_col=None):
    """ids [B, S] int64 -> dict(position, behavior, action, ffn_index [B, S] int64, bad_token int).

    ``position_experts``: the router's table over one item (config.position_experts()); ``n_items``: the router's item count
    (config.n_positions), whose table ends with the eos slot n_items * P.  ``bad_token`` counts the non-special item starts
    outside behavior_maps (the reference puts the raw token id into its index there and fails; the kernel writes 0)."""
    B, S = ids.shape
    P = int(num_positions)
    t = torch.arange(S)
    p = t % P
    special = (ids == pad_id) | (ids == eos_id)
    in_table = (t < n_items * P)[None, :].expand(B, S)
    pos = torch.tensor(list(position_experts), dtype=torch.int64)[p][None, :].expand(B, S).clone()
    pos[~in_table] = 0                                   # the table's eos slot
    pos[special] = 0
    beh = torch.zeros(B, S, dtype=torch.int64)
    act = torch.zeros(B, S, dtype=torch.int64)
    bad = 0
    if use_behavior_token:
        start = ids[:, t - p]                            # the item's first token: its behaviour token
        mapped = torch.full_like(start, -1)
        for tok, idx in behavior_maps.items():
            mapped[start == int(tok)] = int(idx)
        both = (mapped + 1) * in_table                   # repeat_interleave(behaviour + 1, P) + the eos slot's 0
        beh = both.clone()
        beh[:, p == 0] = 0                               # router.py:139, behaviour index only
        beh[special] = 0
        act = both.clone()
        eos_col = ((S + P - 2) // P) * P                 # the action table's own eos slot: n_items of THIS sequence
        if eos_col < S:
            act[:, eos_col] = 0
        act[special] = 0
        if act_zero_col is not None:
            act[:, act_zero_col] = 0
        bad = int(((p == 0)[None, :] & ~special & in_table & (mapped < 0)).sum())
    idx = ((int(num_experts) - 1) * (act - 1) + pos).clamp(min=0)
    return dict(position=pos, behavior=beh, action=act, ffn_index=idx, bad_token=bad)


def route_config(ids, cfg: dict, **kw):
    """``route`` with the fields of a config dict (a fixture's ``meta["config"]``)."""
    P = int(cfg["num_positions"])
    table = ([1] + [2] * (P - 1)) if cfg.get("Moe_behavior_only") else list(range(1, P + 1))
    return route(ids, P, cfg["num_experts"], cfg["behavior_maps"], cfg["pad_token_id"], cfg["eos_token_id"], table,
                 cfg["n_positions"], cfg.get("use_behavior_token", True), **kw)
