#!/usr/bin/env python3
"""Do two builds of libgamer_hip.so compute the same bits in the resident attention kernels (csrc/attention_res.hip)?

  python tools/attn_res_bits.py --a OLD/libgamer_hip.so --b NEW/libgamer_hip.so [--out profiles/NAME.txt]

Each library runs the one case list below in a process of its own (GAMER_LIB_PATH) and prints the SHA-1 of o, lse, dq, dk and dv of
ops.attn_fwd_split / ops.attn_bwd_split in the three-product fp16 form (h2: the form of Engine(matmul="split3")).  One line per
case: the digests and `same`, or `MISS` with, per tensor that differs, how many elements differ and by how many units in the last
place at most (the two processes then run the differing cases again and hand the tensors over in files).  Exit status 1 on any miss.

The cases: S = 37, 263, 300, 505, 600 (one, two and three key blocks of 256, a ragged last tile); B = 2 and 5 with 6 / 3 heads;
self attention, cross attention through the row order and without it; dropout 0 and 0.25; both unit forms of a workgroup
(GAMER_ATTN_RES_SPLIT = 0 / 1).  Values, levels and padding are a fixed integer hash of the element index, so both processes see the
same inputs whatever the random number generators do.
"""
import argparse
import hashlib
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NQ, NKV, SEED = 6, 3, (5 << 32) | 91


def cases():
    """(name, S, B, mode, p, split)"""
    out = []
    for S in (37, 263, 300, 505, 600):
        for B in (2, 5):
            for mode in ("self", "cross+order", "cross"):
                for p in (0.0, 0.25):
                    for split in (0, 1):
                        out.append((f"S={S} B={B} {mode} p={p} split={split}", S, B, mode, p, split))
    return out


def worker(only, dump):
    import torch
    sys.path.insert(0, ROOT)
    from gamer_amd import ops
    dev = "cuda"

    def hashed(n, k):
        """n 32-bit words: a multiplicative hash of the element index (k: which tensor of the case)"""
        i = torch.arange(n, device=dev, dtype=torch.int64)
        h = ((i + 1 + 7919 * k) * 2654435761) % (1 << 32)
        return ((h ^ (h >> 15)) * 1540483477) % (1 << 32)             # (every product stays below 2^63)

    def values(n, k):
        return ((hashed(n, k).double() / float(1 << 32) - 0.5) * 4.0).float()

    def digest(t):
        return hashlib.sha1(t.contiguous().view(torch.int32).cpu().numpy().tobytes()).hexdigest()[:16]

    for name, S, B, mode, p, split in cases():
        if only is not None and name not in only:
            continue
        T, cross = B * S, mode != "self"
        pos = torch.arange(S, device=dev)
        if cross:                                     # levels 0..3 on both sides: a key is allowed for the queries of a higher level behind it
            kl = (hashed(T, 10) >> 7) % 4
            ql = (hashed(T, 11) >> 9) % 4
        else:                                         # kept keys 0, padding 1 (sequence 0: its first S / 3 tokens; a few more anywhere)
            kl = ((hashed(T, 10) >> 7) % 16 == 0).long()
            kl.view(B, S)[0, :max(1, S // 3)] = 1
            ql = torch.ones(T, device=dev, dtype=torch.int64)
        kl, ql = kl.view(B, S).int(), ql.view(B, S).int()
        ok = (pos[None, None, :] <= pos[None, :, None]) & (kl[:, None, :] < ql[:, :, None])
        row_empty = (~ok.any(-1)).int().contiguous()
        n_t = (S + 31) // 32
        pad = torch.zeros(B, n_t * 32, dtype=torch.int32, device=dev)
        pad[:, :S] = row_empty
        tile_empty = pad.view(B, n_t, 32).amax(-1).int().contiguous()
        order = None
        if mode == "cross+order":
            order = (torch.empty(B, S, dtype=torch.int32, device=dev), torch.empty(B, n_t, dtype=torch.int32, device=dev),
                     torch.empty(B, n_t, dtype=torch.int32, device=dev))
            ops.attn_row_order(row_empty, *order)
        q, k, d_o = values(T * NQ * 64, 0).view(T, -1), values(T * NKV * 64, 1).view(T, -1), values(T * NQ * 64, 3).view(T, -1)
        ldv = (NQ + 2 * NKV) * 64                     # v lives inside a q|k|v buffer, as in the model
        qkv = torch.zeros(T, ldv, device=dev)
        qkv[:, (NQ + NKV) * 64:] = values(T * NKV * 64, 2).view(T, -1)
        v = qkv[:, (NQ + NKV) * 64:]
        o = torch.full((T, NQ * 64), float("nan"), device=dev)
        lse = torch.full((B, NQ, S), float("nan"), device=dev)
        delta = torch.zeros(B, NQ, S, device=dev)
        dq = torch.full((T, NQ * 64), float("nan"), device=dev)
        dk = torch.full((T, NKV * 64), float("nan"), device=dev)
        dqkv = torch.zeros(T, ldv, device=dev)
        dv = dqkv[:, (NQ + NKV) * 64:]
        with ops.env_switches(GAMER_ATTN_RES=1, GAMER_ATTN_RES_SPLIT=split):
            ops.attn_fwd_split(q, NQ * 64, k, NKV * 64, v, ldv, kl, ql if cross else None, row_empty, B, S, NQ, NKV, 0.125, p, SEED, o, lse,
                               order=order, h2=True)
            ops.attn_bwd_split(q, NQ * 64, k, NKV * 64, v, ldv, o, d_o, lse, kl, ql if cross else None, row_empty, tile_empty, B, S, NQ,
                               NKV, 0.125, p, SEED, delta, dq, NQ * 64, dk, NKV * 64, dv, ldv, order=order, h2=True)
            torch.cuda.synchronize()
        outs = {"o": o, "lse": lse, "dq": dq, "dk": dk, "dv": dv.contiguous()}
        print("CASE\t" + name + "\t" + " ".join(f"{k_}={digest(t)}" for k_, t in outs.items()), flush=True)
        if dump:
            torch.save({k_: t.cpu() for k_, t in outs.items()}, os.path.join(dump, hashlib.sha1(name.encode()).hexdigest() + ".pt"))


def run_worker(lib, extra, timeout=600):
    env = dict(os.environ, GAMER_LIB_PATH=os.path.abspath(lib))
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", *extra], env=env, capture_output=True, text=True,
                           timeout=timeout)
    except subprocess.TimeoutExpired:
        sys.stderr.write(f"the run of {lib} took more than {timeout} s\n")
        sys.exit(2)
    if r.returncode != 0:                             # (status 2: no comparison was made; nothing more is started)
        sys.stderr.write(f"the run of {lib} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}\n")
        sys.exit(2)
    return {f[1]: f[2] for f in (line.split("\t") for line in r.stdout.splitlines()) if f[0] == "CASE"}


def ulp_report(a, b):
    """per tensor that differs: elements that differ / elements, and the largest distance in units of the last place"""
    import torch
    out = []
    for k in a:
        x, y = a[k], b[k]
        if torch.equal(x.view(torch.int32), y.view(torch.int32)):
            continue
        xi, yi = (t.contiguous().view(torch.int32).long() for t in (x, y))
        xi, yi = (torch.where(t < 0, -(t + (1 << 31)), t) for t in (xi, yi))      # sign-magnitude onto one monotonic integer line
        d = (xi - yi).abs()
        out.append(f"{k}: {int((d > 0).sum())} of {d.numel()} elements differ, by at most {int(d.max())} ulp")
    return "; ".join(out)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--a", help="the first libgamer_hip.so")
    ap.add_argument("--b", help="the second libgamer_hip.so")
    ap.add_argument("--out", help="also write the report to this file")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--only", help=argparse.SUPPRESS)
    ap.add_argument("--dump", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(open(args.only).read().splitlines() if args.only else None, args.dump)
    a, b = run_worker(args.a, []), run_worker(args.b, [])
    names = [c[0] for c in cases()]
    missed = [n for n in names if a.get(n) is None or a.get(n) != b.get(n)]
    why = {}
    if missed:
        import torch
        with tempfile.TemporaryDirectory() as tmp:
            open(os.path.join(tmp, "only"), "w").write("\n".join(missed))
            for side, lib in (("a", args.a), ("b", args.b)):
                os.makedirs(os.path.join(tmp, side))
                run_worker(lib, ["--only", os.path.join(tmp, "only"), "--dump", os.path.join(tmp, side)])
            for n in missed:
                f = hashlib.sha1(n.encode()).hexdigest() + ".pt"
                why[n] = ulp_report(torch.load(os.path.join(tmp, "a", f)), torch.load(os.path.join(tmp, "b", f)))
    lines = [f"# a = {args.a}", f"# b = {args.b}", f"# {len(names)} cases, {len(missed)} missed"]
    for n in names:
        lines.append(f"{n:44s} {a.get(n, 'absent')}  " + ("same" if n not in why else f"MISS (b: {b.get(n, 'absent')}) {why[n]}"))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        open(args.out, "w").write(text)
    return 1 if missed else 0


if __name__ == "__main__":
    sys.exit(main())
