#!/usr/bin/env python3
"""Do two builds of libgamer_hip.so compute the same bits in the FFN activation kernels (csrc/ffn_act.hip)?

  python tools/ffn_act_bits.py --a OLD/libgamer_hip.so --b NEW/libgamer_hip.so [--out profiles/NAME.txt]

Each library runs the one case list below in a process of its own (GAMER_LIB_PATH) and prints the SHA-1 of every tensor a call
wrote - and of the two maxima slots, which every SwiGLU / SiLU call gets armed (gamer_amax_sink).  One line per case: the digests
and `same`, or `MISS` with, per tensor that differs, how many elements differ and by how many units in the last place at most (the
two processes then run the differing cases again and hand the tensors over in files).  Exit status 1 on any miss.

The cases: all sixteen entry points; dropout 0 and 0.2; fp32 and bf16 where the entry has both; the table present and absent, for
ReLU with one row of group -1 and one of group n_groups; the shapes of SHAPES / FLAT_N.  Inputs are a fixed integer hash of the
element index, so both processes see the same values whatever the random number generators do.
"""
import argparse
import hashlib
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (T, I, ld): one quad; padding columns and fewer quads than lanes; 65 quads = a second trip of the lane loop with one lane; more rows
# than the 4 * 8192 waves of the largest grid = a second trip of the row loop
SHAPES = [(1, 4, 8), (37, 96, 200), (5, 260, 520), (32768 + 5, 4, 8)]
# the contiguous pair: the same element counts, and more quads than the 16384 blocks of 256 threads of its largest grid
FLAT_N = [T * I for T, I, _ in SHAPES] + [4 * (16384 * 256 + 3)]
GROUPS, SEED = 5, (3 << 32) | 77


def cases():
    """(name, entry point, dtype name, p, shape, table?)"""
    out = []
    for p in (0.0, 0.2):
        for d in ("fwd", "bwd"):
            for dt in ("f32", "bf16"):
                sfx = "_bf16" if dt == "bf16" else ""
                out += [(f"swiglu_{d}{sfx} n={n} p={p}", f"gamer_swiglu_{d}{sfx}", dt, p, n, False) for n in FLAT_N]
                for act in ("swiglu", "silu"):
                    out += [(f"{act}_{d}_ld{sfx} T={s[0]} I={s[1]} ld={s[2]} p={p}", f"gamer_{act}_{d}_ld{sfx}", dt, p, s, False) for s in SHAPES]
            out += [(f"swiglu_{d}_ld_tbl T={s[0]} I={s[1]} ld={s[2]} p={p}", f"gamer_swiglu_{d}_ld_tbl", "f32", p, s, True) for s in SHAPES]
            out += [(f"relu_tbl_{d} tbl={int(tbl)} T={s[0]} I={s[1]} ld={s[2]} p={p}", f"gamer_relu_tbl_{d}", "f32", p, s, tbl)
                    for tbl in (False, True) for s in SHAPES]
    # the ReLU pair leaves an armed sink alone: the SiLU forward launched after it is the one that fills the slots
    out.append(("relu_tbl_fwd then silu_fwd_ld, sink armed before both", "gamer_relu_tbl_fwd+", "f32", 0.2, SHAPES[1], True))
    return out


def worker(only, dump):
    import torch
    sys.path.insert(0, ROOT)
    from gamer_amd._lib import call, ptr, stream_ptr
    dev = "cuda"

    def values(n, k, dtype):
        """n values in [-4, 4): a multiplicative hash of the element index (k: which tensor of the case)"""
        i = torch.arange(n, device=dev, dtype=torch.int64)
        h = ((i + 1 + 7919 * k) * 2654435761) % (1 << 32)
        h = ((h ^ (h >> 15)) * 1540483477) % (1 << 32)             # (every product stays below 2^63)
        return ((h.double() / float(1 << 32) - 0.5) * 8.0).to(dtype)

    def digest(t):
        raw = t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).cpu().numpy().tobytes()
        return hashlib.sha1(raw).hexdigest()

    for name, entry, dt, p, shape, tbl_on in cases():
        if only is not None and name not in only:
            continue
        dtype = torch.float32 if dt == "f32" else torch.bfloat16
        bwd = "_bwd" in entry
        slots = torch.zeros(2, 256, dtype=torch.int32, device=dev)          # (a slot: 16 words, 16 words apart)
        arm = "relu" not in entry or entry.endswith("+")
        outs = {}
        if isinstance(shape, int):                                          # the contiguous pair
            n = shape
            g, u, o = values(n, 0, dtype), values(n, 1, dtype), values(n, 2, dtype)
            call("gamer_amax_sink", ptr(slots[0]), ptr(slots[1]))
            if bwd:
                call(entry, ptr(g), ptr(u), ptr(o), n, p, SEED, stream_ptr())
                outs = {"dg": g, "du": u}
            else:
                call(entry, ptr(g), ptr(u), n, p, SEED, ptr(o), stream_ptr())
                outs = {"hm": o}
        else:
            T, I, ld = shape
            nin = 2 if "swiglu" in entry else 1
            x = values(T * ld, 0, dtype).view(T, ld)
            o = values(T * I, 2, dtype).view(T, I)                           # dhm, or what the forward overwrites
            tail = []
            if "relu" in entry:
                group = torch.tensor([(0, 1, 2, 4)[i % 4] for i in range(T)], dtype=torch.int32)
                if T >= 5:
                    group[1], group[3] = -1, GROUPS                         # two rows of no group
                table = values(GROUPS * nin * I, 3, torch.float32)
                group_d = group.to(dev)
                tail = [ptr(table) if tbl_on else None, ptr(group_d) if tbl_on else None, GROUPS if tbl_on else 0]
            elif tbl_on:
                group_d = torch.tensor([(0, 1, 2, 4)[i % 4] for i in range(T)], dtype=torch.int32, device=dev)
                table = values(GROUPS * nin * I, 3, torch.float32)
                tail = [ptr(table), ptr(group_d)]
            if arm:
                call("gamer_amax_sink", ptr(slots[0]), ptr(slots[1]))
            e = entry.rstrip("+")
            if bwd:
                call(e, ptr(x), ld, T, I, ptr(o), p, SEED, *tail, stream_ptr())
                outs = {"x": x}
            else:
                call(e, ptr(x), ld, T, I, p, SEED, ptr(o), *tail, stream_ptr())
                outs = {"hm": o, "x": x}                                   # (x: the forward writes nothing into its input)
            if entry.endswith("+"):
                assert int(slots.abs().sum()) == 0, "the ReLU forward took the armed sink"
                hm2 = torch.empty(T, I, device=dev)
                call("gamer_silu_fwd_ld", ptr(x), ld, T, I, p, SEED, ptr(hm2), stream_ptr())
                outs["silu_hm"] = hm2
        if arm:
            outs["amax0"], outs["amax1"] = slots[0], slots[1]
        torch.cuda.synchronize()
        print("CASE\t" + name + "\t" + " ".join(f"{k}={digest(t)}" for k, t in outs.items()), flush=True)
        if dump:
            torch.save({k: t.cpu() for k, t in outs.items()}, os.path.join(dump, hashlib.sha1(name.encode()).hexdigest() + ".pt"))


def run_worker(lib, extra, timeout=300):
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
        if torch.equal(x, y):
            continue
        xi, yi = (t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).long() for t in (x, y))
        if x.dtype != torch.int32:                       # floats are sign-magnitude: onto one monotonic integer line
            top = 1 << (15 if x.dtype == torch.bfloat16 else 31)
            xi, yi = (torch.where(t < 0, -(t + top), t) for t in (xi, yi))
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
    missed = [n for n in names if a.get(n) != b.get(n)]
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
        lines.append(f"{n:64s} {a.get(n, 'absent')}  " + ("same" if n not in why else f"MISS (b: {b.get(n, 'absent')}) {why[n]}"))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        open(args.out, "w").write(text)
    return 1 if missed else 0


if __name__ == "__main__":
    sys.exit(main())
