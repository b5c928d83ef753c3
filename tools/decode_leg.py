#!/usr/bin/env python3
"""bench.py's decode leg on its own (GAMER_DECODE_GRAPH=0/1): python tools/decode_leg.py [users] [--dtype f32|bf16]

--dtype bf16: the same workload (users x 20 beams, history 100, 4 new tokens, shipped architecture) searched by
Engine(dtype="bf16") - timed the way bench.decode_leg times the fp32 engine - plus the time per call of gamer_attn_decode_bf16 on
the session's own caches against its cache-read bound, B * nkv * L0 * 64 * 2 (K, V) * 2 bytes."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


def bf16_leg(users: int, beams: int = 20, his: int = 100, catalogue: int = 20000, iters: int = 4):
    import torch
    from gamer_amd import ops, synthetic
    from gamer_amd.config import synthetic_config
    from gamer_amd.decode import ItemTrie, beam_search
    from gamer_amd.engine import Engine
    cfg = synthetic_config()
    eng = Engine(cfg, temperature=0.7, dtype="bf16")
    eng.init_weights(seed=0)
    cat = synthetic.make_catalogue(catalogue, 256, seed=3)
    tb = 2
    trie = ItemTrie(synthetic.item_tokens(cat, tb, 256).tolist())
    batch = synthetic.make_eval_batch(users, his, cat, tb, 256, 3, min_his=his, seed=5, behavior_probs=[0.7, 0.25, 0.05])

    def timed(fn, n_warm, n):
        for _ in range(n_warm):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n
    search = lambda new: beam_search(eng, batch["input_ids"], batch["attention_mask"], batch["actions"], trie, beams, new)
    ms_all = timed(lambda: search(4), 3, iters)
    ms_first = timed(lambda: search(1), 3, iters)
    per_token_ms = max(ms_all - ms_first, 1e-6) / 3.0
    # the kernel alone, on the caches the last 4-token search left (layer 0's self block, three generated positions)
    search(4)
    st = next(s for k, s in eng._decode_static.items() if k[3] == 4)
    L0 = batch["input_ids"].shape[1]
    nq, nkv = cfg.num_attention_heads, cfg.num_key_value_heads
    kp, vp = st.kp[(0, "self")], st.vp[(0, "self")]
    kg, vg = st.gen[(0, "self")]
    q, o, ok = st.buf["q"], torch.empty_like(st.buf["ao"]), st.small["ok_self"]
    call = lambda: ops.attn_decode_bf16(q, kp, vp, ok, kg, vg, 3, True, users, beams, L0, nq, nkv, 0.125, o)
    kernel_ms = timed(call, 10, 100)
    bound_bytes = users * nkv * L0 * 64 * 2 * 2
    n_attn = cfg.num_hidden_layers + len(cfg.cross_attention_decoder)
    return {"name": f"decode_bf16_bs{users}_beams{beams}", "value": users / (ms_all * 1e-3), "unit": "users/s", "ms_per_batch": ms_all,
            "prefill_plus_first_token_ms": ms_first, "per_token_step_ms": per_token_ms,
            "attn_decode_bf16": {"ms_per_call": kernel_ms, "calls_per_token": n_attn, "cache_read_bound_bytes": bound_bytes,
                                 "achieved_GBs": bound_bytes / (kernel_ms * 1e-3) / 1e9,
                                 "frac_of_hbm_peak": bound_bytes / (kernel_ms * 1e-3) / 1e9 / bench.HBM_PEAK_GBS},
            "workload": f"{users} users x {beams} beams, history {his} items (prompts of {L0} tokens), 4 new tokens, bf16 engine"}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("users", nargs="?", type=int, default=256)
    ap.add_argument("--dtype", choices=("f32", "bf16"), default="f32")
    a = ap.parse_args()
    if a.dtype == "bf16":
        print(json.dumps(bf16_leg(a.users)))
    else:
        r = bench.decode_leg(users=a.users, cpu_users=0)
        print(json.dumps({k: r[k] for k in ("value", "ms_per_batch", "prefill_plus_first_token_ms", "per_token_step_ms")}),
              r["per_token_roofline"]["frac"])
