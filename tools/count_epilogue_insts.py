#!/usr/bin/env python3
"""What the persistent block GEMM (csrc/gemm_bf16_v7.hip) executes per tile outside its K-loop, counted in the gfx950 assembly of the
tagged kernel <1>.  Needs hipcc, no GPU.

    python tools/count_epilogue_insts.py [BASE]

Epilogue = the text between the ticket draw that follows the K-loop (the inline `global_atomic_add ... sc0` inside the tile loop) and
the counted wait that ends it (`s_waitcnt vmcnt(16)`).  Listed: instructions, VALU, v_readlane / v_writelane among them (SGPR spills),
`s_waitcnt lgkmcnt(0)`, LDS operations, global stores, branches — for the whole region, and for every straight-line run in it (no label,
no branch) that holds the 16 stores of a full tile: such a run is ONE path through the epilogue, the whole region is all of them.
K-loop = the blocks of the inner loop (Depth=2), the once-per-tile switch of the stream's source included: instructions, VALU, SALU,
v_readlane / v_writelane, a digest of the opcode sequence, and a digest of the phase plan alone (MFMAs, fragment reads, LDS-DMA
pieces, barriers, priorities and waits with their counts, in program order), so that two trees can be compared: an equal phase-plan
digest = the K-tile body of gemm_tile256.h came out the same, whatever the scalar code of the switch around it did.
BASE (a git revision or a tree, as for tools/diff_kernel_isa.py) is listed first."""
import hashlib
import os
import re
import sys
import tempfile

from diff_kernel_isa import ROOT, assembly, extract

KERNEL = re.compile(r"^(_Z\S*gemm_bf16_nt_v7_kernelILi1E(?:Lb0E)?E\S*):")      # (Lb0E: the <1, false> of a BASE from before the FOLD parameter left)
LANE = ("v_readlane", "v_writelane")
PLAN = ("v_mfma", "ds_read", "buffer_load", "global_load", "s_barrier", "s_waitcnt", "s_setprio")      # what the phase plan of gemm_tile256.h orders


def kernel_body(text):
    body, on = [], False
    for line in text.splitlines():
        if KERNEL.match(line):
            on = True
        elif on:
            if re.match(r"^\.Lfunc_end", line):
                break
            body.append(line)
    return body


def instr(line):
    s = line.split(";")[0].strip()
    return "" if not s or s.endswith(":") or s.startswith(".") else s


def counts(ins):
    op = [x.split()[0] for x in ins]
    return dict(instructions=len(op), valu=sum(o.startswith("v_") for o in op), lane=sum(o.startswith(LANE) for o in op),
                salu=sum(o.startswith("s_") and not o.startswith(("s_waitcnt", "s_nop", "s_cbranch", "s_branch", "s_barrier")) for o in op),
                lgkm0=sum(bool(re.match(r"s_waitcnt (.*\s)?lgkmcnt\(0\)", x)) for x in ins), lds=sum(o.startswith("ds_") for o in op),
                stores=sum(o.startswith("global_store") for o in op), branches=sum(o.startswith(("s_cbranch", "s_branch")) for o in op))


def epilogue(body):
    draws = [i for i, l in enumerate(body) if re.match(r"\s*global_atomic_add v\d+, v\[\d+:\d+\], v\d+, off sc0", l)]
    end = [i for i, l in enumerate(body) if "s_waitcnt vmcnt(16)" in l]
    assert len(draws) >= 2 and end, "epilogue markers not found"
    region = body[draws[1]:end[-1]]
    runs, cur = [], []
    for line in region:
        s = instr(line)
        if re.match(r"^\.LBB", line) or s.startswith(("s_cbranch", "s_branch")):
            runs.append(cur)
            cur = []
        elif s:
            cur.append(s)
    runs.append(cur)
    full = [r for r in runs if sum(x.startswith("global_store_dwordx4") for x in r) == 16]
    return [x for x in map(instr, region) if x], full


def kloop(body):
    ins, depth = [], 0
    for line in body:
        m = re.search(r"Depth=(\d)", line)
        if m and (re.match(r"^\.LBB", line) or re.match(r"^; %bb\.", line)):
            depth = int(m.group(1))
        elif re.match(r"^\.LBB", line) or re.match(r"^; %bb\.", line):
            depth = 0
        s = instr(line)
        if s and depth == 2:
            ins.append(s)
    return ins


def fmt(c):
    return (f"{c['instructions']:5d} instructions  {c['valu']:5d} VALU ({c['lane']:3d} v_readlane/v_writelane)  {c['salu']:4d} SALU  "
            f"{c['lgkm0']:3d} lgkmcnt(0)  {c['lds']:3d} LDS  {c['stores']:3d} stores  {c['branches']:3d} branches")


def main():
    with tempfile.TemporaryDirectory() as tmp:
        trees = ([("base", sys.argv[1] if os.path.isdir(sys.argv[1]) else extract(sys.argv[1], tmp))] if len(sys.argv) > 1 else []) + [("work", ROOT)]
        for label, tree in trees:
            body = kernel_body(assembly(tree, "gemm_bf16_v7.hip", ""))
            region, full = epilogue(body)
            print(f"{label}: gemm_bf16_nt_v7_kernel<1>")
            print(f"  epilogue, all paths     {fmt(counts(region))}")
            for r in full:
                gelu = sum(x.startswith("v_pk_fma_f32") for x in r) > 64
                print(f"  full-tile path ({'GELU' if gelu else 'bias'})   {fmt(counts(r))}")
            if not full:
                print("  (no straight-line full-tile path: every store sits behind its own bounds test)")
            k = kloop(body)
            ops = hashlib.sha256("\n".join(x.split()[0] for x in k).encode()).hexdigest()[:12]
            plan = [x if x.startswith("s_waitcnt") else x.split()[0] for x in k if x.startswith(PLAN)]
            skel = hashlib.sha256("\n".join(plan).encode()).hexdigest()[:12]
            print(f"  K-loop (two K-tiles)    {fmt(counts(k))}  opcodes {ops}  phase plan ({len(plan)}) {skel}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
