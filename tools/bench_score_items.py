#!/usr/bin/env python3
"""Exact scoring of given candidates: users/s of ``decode.score_items`` against the cache-free forward over prompt + item.

  python tools/bench_score_items.py [--B 256] [--C 1001] [--his 100] [--matmul split3] [--slice-rows 1024]

Qwen3Multi (shipped architecture, synthetic weights), prompts of ``--his`` items, ``--C`` candidates per user (one shared list).
Measures, in one process and after a warm-up of every shape:
  * ``score_items``: median wall time of ``--iters`` calls ending in a device synchronise -> users/s;
  * the cache-free way (the only one without score_items): ``DecodeSession._eval_forward`` of ``--slice-rows`` (user, candidate)
    sequences of prompt + 3 item tokens and the log-softmax at the 4 positions, timed on that slice and scaled by
    B * C / slice rows (the whole set would take minutes); the two agree on the slice (max |score difference| is printed);
  * one ``gamer_attn_candidates`` call at the step shape of a chunk (B users x chunk rows, t = 2; device events, self and
    cross masks of the session) and one ``gamer_attn_decode`` call at B users x 20 beams, for orientation;
  * the algorithmic FLOP of an attention call (4 * rows * nq * 64 * (L0 + t)) over its time.
Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gamer_amd import decode, ops, synthetic  # noqa: E402
from gamer_amd.config import synthetic_config  # noqa: E402
from gamer_amd.engine import Engine  # noqa: E402


def _note(msg):
    print(f"[bench_score_items] {msg}", file=sys.stderr, flush=True)


def _wall(fn, iters):
    times = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return statistics.median(times), min(times), max(times)


def _event_ms(fn, iters=20, warm=3):
    for _ in range(warm):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in ev)


def _attn_ms(eng, kernel, B, nb, L0, t, ok, uniform, gen_ok, **kw):
    cfg = eng.cfg
    nq, nkv = cfg.num_attention_heads, cfg.num_key_value_heads
    g = torch.Generator(device="cuda").manual_seed(1)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)
    q, o = rnd(B * nb, nq * 64), torch.empty(B * nb, nq * 64, device="cuda")
    kp, vp = rnd(B * L0, nkv * 64), rnd(B * L0, nkv * 64)
    kg, vg = rnd(B * nb, 4, nkv * 64), rnd(B * nb, 4, nkv * 64)
    ms = _event_ms(lambda: kernel(q, kp, vp, ok, kg, vg, t, gen_ok, uniform, B, nb, L0, nq, nkv, 0.125, o, **kw))
    flop = 4.0 * B * nb * nq * 64 * (L0 + t)
    return dict(ms=ms, tflops=flop / (ms * 1e-3) / 1e12, rows=B * nb)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=256)
    ap.add_argument("--C", type=int, default=1001)
    ap.add_argument("--his", type=int, default=100)
    ap.add_argument("--items", type=int, default=20000, help="catalogue size the candidates are drawn from")
    ap.add_argument("--matmul", default="split3")
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--max-rows", dest="max_rows", type=int, default=65536)
    ap.add_argument("--slice-rows", dest="slice_rows", type=int, default=1024)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a timing tool: it needs the GPU"
    cfg = synthetic_config()
    eng = Engine(cfg, temperature=0.7, matmul=args.matmul)
    eng.init_weights(seed=0)
    tb, B, C = 2, args.B, args.C
    cat = synthetic.make_catalogue(args.items, 256, seed=3)
    batch = synthetic.make_eval_batch(B, args.his, cat, tb, 256, 3, min_his=args.his, seed=5, behavior_probs=[0.7, 0.25, 0.05])
    pick = torch.randperm(cat.shape[0], generator=torch.Generator().manual_seed(11))[:C]
    items = synthetic.item_tokens(cat[pick], tb, 256)[:, 1:].contiguous().cuda()
    ids, am, act = (batch[k].cuda() for k in ("input_ids", "attention_mask", "actions"))
    L0, T = ids.shape[1], items.shape[1]

    run = lambda: decode.score_items(eng, ids, am, act, items, max_rows=args.max_rows)
    _note(f"prompts {tuple(ids.shape)}, items {tuple(items.shape)}: warm-up")
    scores = run()                                            # warm-up: buffers, code objects, weight maxima
    med, lo, hi = _wall(run, args.iters)
    st = next(iter(eng._score_static.values()))
    chunk = st.gen[next(iter(st.gen))][0].shape[0] // B
    ok_self, ok_cross, uniform = (st.small[k].clone() for k in ("ok_self", "ok_cross", "uniform_cross"))
    out = dict(metric="exact scoring users/s, Qwen3Multi, given candidates on the cached decode path", value=B / med, unit="users/s",
               ms_per_batch=med * 1e3, ms_min=lo * 1e3, ms_max=hi * 1e3,
               config=dict(workload=f"{B} users x {C} candidates, history {args.his} items ({L0} prompt tokens), {T} item tokens, "
                                    f"fp32 matmul={args.matmul}, chunks of {chunk} candidates per user ({B * chunk} rows)"))

    # the cache-free way on a slice of the same (user, candidate) pairs: whole sequences of prompt + item, log-softmax at T positions
    n_users = max(1, min(B, args.slice_rows // 64))
    per_user = max(1, args.slice_rows // n_users)
    S = L0 + T - 1
    flat = torch.cat([ids[:n_users, None, :].expand(n_users, per_user, L0), items[None, :per_user, :T - 1].expand(n_users, per_user, T - 1)],
                     2).reshape(-1, S).contiguous()
    am_s = torch.cat([am[:n_users], am.new_ones(n_users, T - 1)], 1).repeat_interleave(per_user, 0)
    act_s = torch.cat([act[:n_users], act[:n_users, -1:].expand(n_users, T - 1)], 1).repeat_interleave(per_user, 0)
    rows = flat.shape[0]
    tgt = items[None, :per_user].expand(n_users, per_user, T).reshape(rows, T, 1)

    def rerun():
        decode.DecodeSession._eval_forward(eng, flat, am_s, act_s, {}, L0)
        lg = eng.ws.logits[:rows * S].view(rows, S, -1)[:, L0 - 1:, :cfg.vocab_size]
        return torch.log_softmax(lg, -1).gather(2, tgt).squeeze(2).mean(1).view(n_users, per_user)
    _note(f"score_items {med * 1e3:.1f} ms per batch; cache-free forward on {rows} sequences")
    ref = rerun()
    rmed, rlo, rhi = _wall(rerun, args.iters)
    scaled = rmed * (B * C) / rows
    out["cache_free_forward"] = dict(rows=rows, ms_slice=rmed * 1e3, ms_slice_min=rlo * 1e3, ms_slice_max=rhi * 1e3,
                                     ms_scaled_to_batch=scaled * 1e3, users_per_s_scaled=B / scaled,
                                     max_score_diff_on_slice=float((ref - scores[:n_users, :per_user]).abs().max()),
                                     note=f"{n_users} users x {per_user} candidates timed, scaled by B*C/rows")
    out["speedup_vs_cache_free_scaled"] = scaled / med

    _note(f"cache-free forward {rmed * 1e3:.1f} ms per {rows} sequences; attention calls")
    # the step attention alone, at the session's own masks
    out["attn_candidates_self"] = _attn_ms(eng, ops.attn_candidates, B, chunk, L0, 2, ok_self, None, True)
    out["attn_candidates_cross"] = _attn_ms(eng, ops.attn_candidates, B, chunk, L0, 2, ok_cross, uniform, False)
    out["attn_decode_self_20_beams"] = _attn_ms(eng, ops.attn_decode, B, 20, L0, 2, ok_self, None, True)
    out["attn_decode_cross_20_beams"] = _attn_ms(eng, ops.attn_decode, B, 20, L0, 2, ok_cross, uniform, False)
    out["attn_candidates_self_20_rows"] = _attn_ms(eng, ops.attn_candidates, B, 20, L0, 2, ok_self, None, True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
