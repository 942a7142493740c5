#!/usr/bin/env python3
"""Vector / scalar ALU instructions in the load sections of the 256-tile block GEMMs' K-loop (csrc/gemm_tile256.h), from the gfx950
assembly of gemm_bf16_v6.hip and gemm_bf16_v7.hip.  Needs hipcc, no GPU.

    python tools/count_load_section_valu.py [BASE]

A load section = the instructions between two s_barrier that hold exactly two LDS-DMA pieces and no MFMA (the sections of the prologue
hold more pieces and are not listed).  Per kernel and section, in program order: VALU instructions, those of them that are
v_cndmask / v_lshl_add_u64 / v_cmp (per-lane address selection), SALU instructions.  The straight-line text between two barriers is
counted: a section that contains a branch (v7: the once-per-tile switch of the stream's source at the top of P2) counts both sides.
BASE (a git revision or a tree, as for tools/diff_kernel_isa.py) is listed first when given."""
import os
import re
import sys
import tempfile

from diff_kernel_isa import ROOT, assembly, extract

DMA = re.compile(r"(buffer_load_dwordx4 .* lds|global_load_lds_dwordx4)")


def kernels(text):
    out, name, body = {}, None, []
    for line in text.splitlines():
        m = re.match(r"^(_Z\S*gemm_bf16_nt_v\d_kernel\S*):", line)
        if m:
            name, body = m.group(1), []
        elif name:
            body.append(line)
            if re.match(r"^\.Lfunc_end", line):
                out[name] = body
                name = None
    return out


def sections(body):
    secs, cur = [], []
    for line in body:
        s = line.split(";")[0].strip()
        if not s or s.endswith(":") or s.startswith("."):
            continue
        if s.startswith("s_barrier"):
            secs.append(cur)
            cur = []
        else:
            cur.append(s)
    rows = []
    for sec in secs:
        if sum(1 for x in sec if DMA.match(x)) != 2 or any(x.startswith("v_mfma") for x in sec):
            continue
        valu = [x.split()[0] for x in sec if x.startswith("v_")]
        salu = sum(1 for x in sec if x.startswith("s_") and not x.startswith(("s_waitcnt", "s_nop", "s_cbranch")))
        rows.append((len(valu), sum(1 for v in valu if v.startswith(("v_cndmask", "v_lshl_add_u64", "v_cmp"))), salu))
    return rows


def main():
    with tempfile.TemporaryDirectory() as tmp:
        trees = ([("base", sys.argv[1] if len(sys.argv) > 1 and os.path.isdir(sys.argv[1]) else extract(sys.argv[1], tmp))]
                 if len(sys.argv) > 1 else []) + [("work", ROOT)]
        for label, tree in trees:
            for f in ("gemm_bf16_v7.hip", "gemm_bf16_v6.hip"):
                for name, body in kernels(assembly(tree, f, "")).items():
                    rows = sections(body)
                    kern = re.search(r"gemm_bf16_nt_v\d_kernelI(\w+?)EEv", name)
                    print(f"{label} {f} <{kern.group(1) if kern else name}>: (VALU, address selects among them, SALU) per load section")
                    print("    " + " ".join(f"({v},{b},{s})" for v, b, s in rows))
    return 0


if __name__ == "__main__":
    sys.exit(main())
