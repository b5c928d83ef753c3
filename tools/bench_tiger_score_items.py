#!/usr/bin/env python3
"""Exact scoring of given candidates on TIGER: users/s of ``tiger.score_items`` against ``forward`` over repeated encoder rows, and
the candidates cross attention against the resident kernel with its row map.

  python tools/bench_tiger_score_items.py [--B 256] [--C 1001] [--enc 100] [--T 5] [--slice-rows 1024] [--only-score]

TIGER at the shipped config (d_model 128, 6 heads of 64, 4 + 4 layers, d_ff 1024, the T5 vocabulary of 32,128 rows, random weights),
``--B`` users with encoders of ``--enc`` tokens, ``--C`` candidates per user (one shared list) of ``--T`` tokens.  In one process,
after a warm-up of every shape:
  * ``score_items``: median wall time of ``--iters`` calls ending in a device synchronise -> ms per batch, users/s;
  * the way without it: ``forward(decoder_input_ids=...)`` over ``--slice-rows`` (user, candidate) sequences, the encoder rows
    repeated per candidate, and the log-softmax at the T positions; timed on that slice and scaled by B * C / slice rows, on the
    assumption that forward's time is linear in the rows at that size (the whole set would take minutes and its [rows, T, V] logits
    do not fit); the two agree on the slice (max |score difference| is printed);
  * kernel A/B at the step shape (B users x chunk x (T) query rows, encoder length ``--enc``): one gamer_t5_attn_candidates call against
    one gamer_t5_attn_fwd call with kv_rows on the same tensors - device events, median of 20 - each also as GB/s of LDS staging
    (bytes written into LDS by the K / V staging of all workgroups) and TFLOP/s (4 rows h d Sk) against the 157 TFLOP/s fp32 matrix
    peak.
``--only-score``: nothing but warm-up + ``--iters`` score_items calls (the process a kernel trace is taken from:
``rocprofv3 --kernel-trace --stats -- python tools/bench_tiger_score_items.py --only-score``).
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
from gamer_amd import ops, tiger  # noqa: E402

SHIPPED = dict(d_model=128, d_kv=64, d_ff=1024, num_layers=4, num_decoder_layers=4, num_heads=6, dropout_rate=0.1, vocab_size=32128)
FP32_MATRIX_PEAK_TFLOPS = 157.0


def _note(msg):
    print(f"[bench_tiger_score_items] {msg}", file=sys.stderr, flush=True)


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


def _kernel_ab(B, chunk, S, Sk, h, d):
    """the cross attention of one decoder layer of a chunk: B users x chunk sequences x S positions against Sk keys"""
    g = torch.Generator(device="cuda").manual_seed(1)
    I, N = h * d, B * chunk
    q = torch.randn(N * S, I, device="cuda", generator=g) * (10.0 / d) ** 0.5
    kv = torch.randn(B * Sk, 2 * I, device="cuda", generator=g)
    k, v = kv[:, :I], kv[:, I:]
    keep = torch.ones(B, Sk, dtype=torch.uint8, device="cuda")
    o_new, o_old = torch.empty(N * S, I, device="cuda"), torch.empty(N * S, I, device="cuda")
    lse = torch.empty(N, h, S, device="cuda")
    kv_rows = (torch.arange(N, dtype=torch.int32, device="cuda") // chunk).contiguous()
    new = lambda: ops.t5_attn_candidates(q, k, v, keep, B, chunk * S, Sk, h, d, o_new)
    old = lambda: ops.t5_attn_fwd(q, k, v, None, keep, N, S, Sk, h, d, False, 0.0, 0, o_old, lse, kv_rows=kv_rows, kv_batch=B)
    ms_new, ms_old = _event_ms(new), _event_ms(old)
    ms_new2 = _event_ms(new)                                   # A B A: the first kernel again, for drift
    Sk16 = (Sk + 15) // 16 * 16
    stage = 2 * Sk16 * (d + 4) * 4                             # bytes one workgroup writes into LDS for K and V
    wg_new, wg_old = B * h * ((chunk * S + 63) // 64), N * h
    flop = 4.0 * N * S * h * d * Sk
    row = lambda ms, wgs: dict(ms=ms, workgroups=wgs, lds_staging_gb=wgs * stage / 1e9, lds_staging_gbps=wgs * stage / (ms * 1e-3) / 1e9,
                               tflops=flop / (ms * 1e-3) / 1e12, share_of_fp32_matrix_peak=flop / (ms * 1e-3) / 1e12 / FP32_MATRIX_PEAK_TFLOPS)
    return dict(shape=f"{B} users x {chunk * S} query rows ({chunk} sequences x {S}), {Sk} keys, {h} heads of {d}",
                t5_attn_candidates=row(ms_new, wg_new), t5_attn_candidates_again=dict(ms=ms_new2),
                t5_attn_fwd_kv_rows=row(ms_old, wg_old), speedup=ms_old / ms_new, bit_equal=bool(torch.equal(o_new, o_old)),
                max_abs_diff=float((o_new - o_old).abs().max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=256)
    ap.add_argument("--C", type=int, default=1001)
    ap.add_argument("--enc", type=int, default=100)
    ap.add_argument("--T", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--max-rows", dest="max_rows", type=int, default=65536)
    ap.add_argument("--slice-rows", dest="slice_rows", type=int, default=1024)
    ap.add_argument("--only-score", dest="only_score", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a timing tool: it needs the GPU"
    torch.manual_seed(0)
    model = tiger.TIGER(tiger.TigerConfig(**SHIPPED)).cuda().eval()
    B, C, T, V = args.B, args.C, args.T, SHIPPED["vocab_size"]
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(2, V, (B, args.enc), generator=g).cuda()
    am = torch.ones_like(ids)
    items = torch.randint(2, V, (C, T), generator=g).cuda()
    run = lambda: tiger.score_items(model, ids, am, items, max_rows=args.max_rows)
    _note(f"encoder {tuple(ids.shape)}, items {tuple(items.shape)}: warm-up")
    scores = run()
    med, lo, hi = _wall(run, args.iters)
    chunk = -(-C // -(-C // max(1, args.max_rows // B)))
    out = dict(metric="exact scoring users/s, TIGER, given candidates", value=B / med, unit="users/s", ms_per_batch=med * 1e3,
               ms_min=lo * 1e3, ms_max=hi * 1e3,
               config=dict(workload=f"{B} users x {C} candidates, encoder length {args.enc}, {T} item tokens, fp32, chunks of {chunk} "
                                    f"candidates per user ({B * chunk} decoder sequences of {T} positions)"))
    if args.only_score:
        print(json.dumps(out))
        return
    # forward over repeated encoder rows on a slice of the same (user, candidate) pairs
    n_users = max(1, min(B, args.slice_rows // 64))
    per_user = max(1, min(C, args.slice_rows // n_users))
    rows = n_users * per_user
    dec_in = torch.cat([torch.zeros(rows, 1, dtype=torch.int64, device="cuda"),
                        items[None, :per_user, :T - 1].expand(n_users, per_user, T - 1).reshape(rows, T - 1)], 1).contiguous()
    ids_r, am_r = ids[:n_users].repeat_interleave(per_user, 0), am[:n_users].repeat_interleave(per_user, 0)
    tgt = items[None, :per_user].expand(n_users, per_user, T).reshape(rows, T, 1)

    def rerun():
        with torch.no_grad():
            _, logits = model(ids_r, am_r, decoder_input_ids=dec_in)
        return torch.log_softmax(logits, -1).gather(2, tgt).squeeze(2).mean(1).view(n_users, per_user)
    _note(f"score_items {med * 1e3:.1f} ms per batch; forward on {rows} sequences")
    ref = rerun()
    rmed, rlo, rhi = _wall(rerun, args.iters)
    scaled = rmed * (B * C) / rows
    out["forward_repeated_rows"] = dict(rows=rows, ms_slice=rmed * 1e3, ms_slice_min=rlo * 1e3, ms_slice_max=rhi * 1e3,
                                        ms_scaled_to_batch=scaled * 1e3, users_per_s_scaled=B / scaled,
                                        max_score_diff_on_slice=float((ref - scores[:n_users, :per_user]).abs().max()),
                                        note=f"{n_users} users x {per_user} candidates timed, scaled by B*C/rows (assumes forward is "
                                             f"linear in the rows from {rows} on)")
    out["speedup_vs_forward_scaled"] = scaled / med
    _note(f"forward {rmed * 1e3:.1f} ms per {rows} sequences; kernel A/B")
    c = model.config
    out["kernel_ab"] = _kernel_ab(B, chunk, T, args.enc, c.num_heads, c.d_kv)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
