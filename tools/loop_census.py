#!/usr/bin/env python3
"""What do the hot loops of a kernel issue?  Reads compiler output (hipcc -S) only; needs no GPU.

  hipcc -O3 --offload-arch=gfx950 -std=c++20 --cuda-device-only -S -Igamer_amd/csrc -Iinclude gamer_amd/csrc/attention_res.hip -o res.s
  python tools/loop_census.py res.s attn_fwd_r_kernelILi2ELb1ELb0ELb0E [--min-mfma 1] [--max-paths 24]

For every kernel whose (mangled) name contains the substring: the control-flow graph of its basic blocks, its innermost loops
(natural loops of the back edges that contain no other loop header) and, per loop, every path of one trip - header to back edge -
that issues at least --min-mfma MFMAs.  Per loop and per path, instructions by class:

  mfma   v_mfma_*                                lds_r / lds_w   ds_read* / ds_write* (others under lds_o: atomics, permutes)
  addr   integer add / sub / shift / or / mad    mov             v_mov_*, v_accvgpr_* (the latter also under agpr)
  cmp    v_cmp*, v_cndmask*                      trans           v_exp / v_log / v_rcp / v_rsq / v_sqrt / v_sin / v_cos
  valu   every other v_* instruction             vmem            global_ / buffer_ / flat_ / scratch_
  nop    s_nop (the count of instructions, and of wait states)   wait   s_waitcnt*, s_barrier
  salu   every other s_* instruction

The compiler lays the variants of a tile (masked / unmasked / ...) out as a chain, each behind a test of its own flag, so the graph
has paths that run several variants in one trip; a wave runs one.  Every path names the blocks that hold its MFMAs: pick the
paths of one variant by them, and keep the others out with --max-mfma (the MFMAs of one tile).  Paths with equal counts are listed once, fewest MFMAs and then
fewest vector instructions first.

vec/MFMA = (everything the vector issue port takes that is no MFMA: addr + mov + cmp + trans + valu + lds + vmem) / mfma.
With --constants N the tool also lists the integer adds of the loop whose literal operand is >= N (LDS bases the immediate
offset of a ds instruction cannot reach).
"""
import argparse
import collections
import re
import sys

CLASSES = ["mfma", "lds_r", "lds_w", "lds_o", "addr", "mov", "agpr", "cmp", "trans", "valu", "vmem", "nop", "nop_states", "wait", "salu"]
ADDR = re.compile(r"^v_(add|sub|subrev|addc|subb)(_co)?_[ui]32|^v_add3_u32|^v_(lshl|lshr|ashr)(rev)?_[bi](32|64)|^v_lshl_add_u(32|64)|^v_add_lshl_u32"
                  r"|^v_lshl_or_b32|^v_or3?_b32|^v_and_or_b32|^v_mad_[ui]32_[ui]24|^v_mad_[ui]64_[ui]32|^v_mul_lo_u32")
TRANS = re.compile(r"^v_(exp|log|rcp|rsq|sqrt|sin|cos)_")
BRANCH = re.compile(r"^s_(c?branch\w*)\s+(\.L\w+)")
LABEL = re.compile(r"^(\.L\w+|[A-Za-z_]\w*):")


def classify(op, text):
    """class names of one instruction (agpr moves count under mov and agpr)"""
    if op.startswith("v_mfma") or op.startswith("v_smfmac"):
        return ["mfma"]
    if op.startswith("ds_"):
        if op.startswith(("ds_read", "ds_load")):
            return ["lds_r"]
        return ["lds_w"] if op.startswith(("ds_write", "ds_store")) else ["lds_o"]
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return ["vmem"]
    if op.startswith("v_accvgpr"):
        return ["mov", "agpr"]
    if op.startswith(("v_mov_", "v_pk_mov_")):
        return ["mov"]
    if op.startswith(("v_cmp", "v_cndmask")):
        return ["cmp"]
    if TRANS.match(op):
        return ["trans"]
    if ADDR.match(op):
        return ["addr"]
    if op.startswith("v_"):
        return ["valu"]
    if op == "s_nop":
        return ["nop"]
    if op.startswith("s_waitcnt") or op == "s_barrier":
        return ["wait"]
    if op.startswith("s_"):
        return ["salu"]
    return []


class Block:
    def __init__(self, name):
        self.name, self.ins, self.succ, self.counts = name, [], [], collections.Counter()


def kernels(lines, needle):
    """(name, lines of the body) of every function whose name contains needle"""
    out, cur, name = [], None, None
    for ln in lines:
        s = ln.strip()
        m = LABEL.match(s)
        if m and not m.group(1).startswith(".L") and cur is None and needle in m.group(1) and s.split(";")[0].strip().endswith(":"):
            name, cur = m.group(1), []
            continue
        if cur is not None:
            if s.startswith(".Lfunc_end"):
                out.append((name, cur))
                cur = None
            else:
                cur.append(s)
    return out


def blocks_of(body):
    blocks = [Block("entry")]
    for s in body:
        s = s.split(";")[0].strip() if not s.startswith(";") else ""
        if not s or s.startswith("//"):
            continue
        m = LABEL.match(s)
        if m:
            blocks.append(Block(m.group(1)))
            continue
        if s.startswith("."):
            continue
        op = s.split()[0]
        b = blocks[-1]
        b.ins.append(s)
        for c in classify(op, s):
            b.counts[c] += 1
        if op == "s_nop":
            b.counts["nop_states"] += int(s.split()[1], 0) + 1
        if op.startswith(("s_cbranch", "s_branch")):             # (the block that follows a branch carries no label of its own)
            blocks.append(Block(f"{b.name.split('+')[0]}+{len(blocks)}"))
    by_name = {b.name: i for i, b in enumerate(blocks)}
    for i, b in enumerate(blocks):
        ended = False
        for s in b.ins:                       # (a block may hold a conditional branch followed by more code only at its end)
            m = BRANCH.match(s)
            if m and m.group(2) in by_name:
                b.succ.append(by_name[m.group(2)])
                if m.group(1) == "branch":
                    ended = True
            if s.startswith(("s_endpgm", "s_setpc")):
                ended = True
        if not ended and i + 1 < len(blocks):
            b.succ.append(i + 1)
    return blocks


def innermost_loops(blocks):
    """[(header, body set)] of the natural loops that contain no other loop's header"""
    n = len(blocks)
    color, back = [0] * n, []
    stack = [(0, iter(blocks[0].succ))]
    color[0] = 1
    while stack:
        u, it = stack[-1]
        for v in it:
            if color[v] == 0:
                color[v] = 1
                stack.append((v, iter(blocks[v].succ)))
                break
            if color[v] == 1:
                back.append((u, v))
        else:
            color[u] = 2
            stack.pop()
    pred = collections.defaultdict(list)
    for i, b in enumerate(blocks):
        for v in b.succ:
            pred[v].append(i)
    loops = {}
    for t, h in back:
        body, work = loops.setdefault(h, {h}), [t]
        while work:
            x = work.pop()
            if x not in body:
                body.add(x)
                work.extend(pred[x])
    heads = set(loops)
    return [(h, body) for h, body in sorted(loops.items()) if not (body - {h}) & heads]


def trip_paths(blocks, h, body, max_paths):
    """paths header -> ... -> (edge back to the header), inside the loop body"""
    out, truncated = [], False
    stack = [(h, [h])]
    while stack:
        u, path = stack.pop()
        for v in blocks[u].succ:
            if v == h:
                if len(out) < max_paths:
                    out.append(path)
                else:
                    truncated = True
            elif v in body and v not in path:
                stack.append((v, path + [v]))
    return out, truncated


def line_of(c):
    vec = sum(c[k] for k in ("addr", "mov", "cmp", "trans", "valu", "lds_r", "lds_w", "lds_o", "vmem"))
    cells = " ".join(f"{k}={c[k]}" for k in CLASSES if k not in ("nop_states",))
    ratio = f"{vec / c['mfma']:.2f}" if c["mfma"] else "-"
    return f"{cells} nop_states={c['nop_states']} | vector={vec} vec/MFMA={ratio}"


def resources(path):
    """kernel -> figures, from the remarks of hipcc -Rpass-analysis=kernel-resource-usage (its stderr, saved to a file)"""
    out, cur = {}, None
    for ln in open(path):
        m = re.search(r"remark:\s+(Function Name|TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|SGPRs Spill|VGPRs Spill"
                      r"|LDS Size \[bytes/block\]): (\S+)", ln)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = out.setdefault(m.group(2), {})
        elif cur is not None:
            cur[m.group(1).split(" [")[0].replace(" ", "_")] = m.group(2)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("asm")
    ap.add_argument("kernel", help="substring of the kernel's (mangled) name")
    ap.add_argument("--min-mfma", type=int, default=1, help="list only loops / paths with at least this many MFMAs")
    ap.add_argument("--max-paths", type=int, default=24)
    ap.add_argument("--constants", type=lambda s: int(s, 0), default=None, help="list integer adds with a literal >= this")
    ap.add_argument("--resources", help="stderr of the same compile with -Rpass-analysis=kernel-resource-usage: registers, spills, scratch")
    ap.add_argument("--max-mfma", type=int, default=1 << 30, help="list only paths with at most this many MFMAs")
    ap.add_argument("--blocks", action="store_true", help="also list every basic block of a loop with its successors")
    args = ap.parse_args()
    found = kernels(open(args.asm).read().splitlines(), args.kernel)
    if not found:
        sys.exit(f"no kernel with '{args.kernel}' in its name in {args.asm}")
    res = resources(args.resources) if args.resources else {}
    for name, body in found:
        blocks = blocks_of(body)
        total = collections.Counter()
        for b in blocks:
            total.update(b.counts)
        print(f"== {name}")
        if name in res:
            print("   resources: " + " ".join(f"{k}={v}" for k, v in res[name].items()))
        print(f"   whole kernel: {line_of(total)}")
        for h, lbody in innermost_loops(blocks):
            c = collections.Counter()
            for i in lbody:
                c.update(blocks[i].counts)
            if c["mfma"] < args.min_mfma:
                continue
            print(f" loop at {blocks[h].name} ({len(lbody)} blocks, all paths together): {line_of(c)}")
            if args.constants is not None:
                big = collections.Counter()
                for i in sorted(lbody):
                    for s in blocks[i].ins:
                        if s.startswith(("v_add_u32", "v_add_co_u32", "v_add3_u32", "v_or_b32", "v_lshl_add_u32")):
                            for lit in re.findall(r"\b0x[0-9a-f]+\b|(?<![\w.\[:])\d+\b", s.split(None, 1)[1]):
                                if int(lit, 0) >= args.constants:
                                    big[hex(int(lit, 0))] += 1
                print(f"   integer adds with a literal >= {hex(args.constants)}: {sum(big.values())}  " + " ".join(f"{k}x{v}" for k, v in sorted(big.items())))
            if args.blocks:
                for i in sorted(lbody):
                    last = [s.split()[0] for s in blocks[i].ins if s.startswith(("s_cbranch", "s_branch"))]
                    print(f"   block {blocks[i].name:12s} -> {','.join(blocks[v].name for v in blocks[i].succ):28s} {'/'.join(last):32s} {line_of(blocks[i].counts)}")
            paths, trunc = trip_paths(blocks, h, lbody, 20000)
            paths = [p for p in paths if args.min_mfma <= sum(blocks[i].counts["mfma"] for i in p) <= args.max_mfma]
            rows = {}
            for p in paths:
                pc = collections.Counter()
                for i in p:
                    pc.update(blocks[i].counts)
                if pc["mfma"] >= args.min_mfma:
                    vec = int(line_of(pc).split("vector=")[1].split()[0])
                    rows.setdefault(line_of(pc), ((pc["mfma"], vec), [blocks[i].name for i in p if blocks[i].counts["mfma"]]))
            for n, (text, (_, where)) in enumerate(sorted(rows.items(), key=lambda kv: (kv[1][0], kv[0]))[:args.max_paths]):
                print(f"   path {n + 1} (MFMAs in {','.join(where)}): {text}")
            if trunc or len(rows) > args.max_paths:
                print(f"   ({len(rows)} distinct paths{', enumeration cut short' if trunc else ''}: the first {args.max_paths} are listed)")


if __name__ == "__main__":
    main()
