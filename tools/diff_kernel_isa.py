#!/usr/bin/env python3
"""Device assembly of the HIP sources of two trees, compared after a normalisation: the gate for refactors of hand-counted kernels
("the compiler emits the same instructions").  Needs hipcc, no GPU.

    python tools/diff_kernel_isa.py BASE [--work DIR] [--files a.hip ...] [--defines "" "MEDP_V7_PHASE_TRACE" ...] [--by-function]
                                    [--merged NEW.hip=OLD1.hip,OLD2.hip ...] [--split OLD.hip=NEW1.hip,NEW2.hip ...]

BASE is a git revision (its csrc/ and include/ are extracted to a temporary directory) or a directory holding a tree; the other side
is the work tree (--work: another directory).  Every file is compiled for gfx950 at the flags of build.py with `-S --cuda-device-only`,
once per -D set.  Default: every csrc/*.hip plain, plus gemm_bf16_v7.hip under each of its three build switches.  Dropped before the
comparison: comments, .file / .ident / .loc lines, the per-translation-unit __hip_cuid_* symbol; the zero-chunk symbols (g_zero16*)
are renamed to one name.  The resource-usage block of every kernel (.amdhsa_* lines) is part of the compared text.
Prints IDENTICAL, REORDERED (every function and kernel descriptor identical and the same lines around them, in another order: what a
change of the host code's template instantiation order does) or the first differing hunk per file and -D set; with --by-function a differing file is also listed function by
function (for a change that deliberately removes or edits one kernel of a file).  --merged: NEW.hip of the work tree took over the
kernels of several files of BASE; those are compiled one by one and NEW.hip is listed function by function against their union.
--split: the reverse, OLD.hip of BASE was divided over several files of the work tree (OLD.hip itself may be one of them).
Exit status 1 on any difference."""
import argparse
import concurrent.futures
import difflib
import glob
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "multimodal_edema_prediction_amd"
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
V7_DEFINES = ["MEDP_V7_PHASE_TRACE", "MEDP_V7_ABLATE_MFMA", "MEDP_V7_ABLATE_LOADS"]


def extract(rev: str, dst: str) -> str:
    """csrc/ and include/ of a git revision under dst"""
    ar = subprocess.run(["git", "-C", ROOT, "archive", rev, f"{PKG}/csrc", "include"], stdout=subprocess.PIPE, check=True)
    subprocess.run(["tar", "-x", "-C", dst], input=ar.stdout, check=True)
    return dst


def assembly(tree: str, name: str, define: str) -> str:
    csrc = os.path.join(tree, PKG, "csrc")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-x", "hip", "-I", csrc, "-I", os.path.join(tree, "include"),
           "-Wno-unused-result", "-Wno-unused-value", "--cuda-device-only", "-S", os.path.join(csrc, name), "-o", "-"]
    if define:
        cmd[1:1] = ["-D" + d for d in define.split(",")]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed on {tree}/{name} [{define}]:\n{r.stderr[-3000:]}")
    return r.stdout


def normalise(text: str) -> list:
    out = []
    for line in text.splitlines():
        line = re.sub(r"\s*;.*$", "", line).rstrip()
        s = line.strip()
        if not s or s.startswith((".file", ".ident", ".loc")) or "__hip_cuid_" in s:
            continue
        out.append(re.sub(r"[\w.$]*g_zero16[\w.$]*", "g_zero16", line))
    return out


def functions(lines: list, rest: list = None) -> dict:
    """name -> body, for every function (label ... .Lfunc_end) and every kernel descriptor (.amdhsa_kernel ... .end_amdhsa_kernel);
    the lines outside them are appended to `rest`"""
    fns, name, body = {}, None, []
    for i, line in enumerate(lines):
        if name is None and rest is not None:
            rest.append(re.sub(r"\.(LBB|Lfunc_end|Lfunc_begin)\d+", r".\1", line))
        m = re.match(r"^([A-Za-z_][\w.$]*):$", line)
        if name is None and m and i > 0 and "@function" in lines[i - 1]:
            name, body = m.group(1), []
        elif name is None and line.strip().startswith(".amdhsa_kernel"):
            name, body = "descriptor of " + line.split()[1], []
        elif name is not None:
            body.append(re.sub(r"\.(LBB|Lfunc_end|Lfunc_begin)\d+", r".\1", line))     # (local labels carry the function's index in the file)
            if re.match(r"^\.Lfunc_end\d+:$", line) or line.strip() == ".end_amdhsa_kernel":
                fns[name] = body
                name = None
    return fns


def first_hunk(a: list, b: list) -> str:
    for group in difflib.SequenceMatcher(None, a, b, autojunk=False).get_grouped_opcodes(2):
        lo, hi = group[0][1], group[-1][2]
        text = [f"@@ base line {lo + 1} @@"]
        for tag, i1, i2, j1, j2 in group:
            if tag == "equal":
                text += ["  " + x for x in a[i1:i2]]
            else:
                text += ["- " + x for x in a[i1:i2]] + ["+ " + x for x in b[j1:j2]]
        return "\n".join(text[:60]) + f"\n({sum(1 for x, y in zip(a, b) if x != y) + abs(len(a) - len(b))} of {max(len(a), len(b))} lines differ by position)"
    return ""


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("base", help="git revision, or a directory that holds a tree")
    ap.add_argument("--work", default=ROOT, help="the other tree (default: the work tree)")
    ap.add_argument("--files", nargs="*", help="sources under csrc/ (default: all *.hip)")
    ap.add_argument("--defines", nargs="*", help='-D sets, comma-separated names, "" for none (default: "" and, for gemm_bf16_v7.hip, its switches)')
    ap.add_argument("--by-function", action="store_true", help="list the functions of a differing file one by one")
    ap.add_argument("--merged", nargs="*", default=[], metavar="NEW.hip=OLD1.hip,OLD2.hip", help="a work-tree file set against several files of the base")
    ap.add_argument("--split", nargs="*", default=[], metavar="OLD.hip=NEW1.hip,NEW2.hip", help="a file of the base set against several work-tree files")
    ap.add_argument("-j", type=int, default=min(8, os.cpu_count() or 1))
    args = ap.parse_args()

    with tempfile.TemporaryDirectory() as tmp:
        base = args.base if os.path.isdir(args.base) else extract(args.base, tmp)
        names = args.files or sorted(os.path.basename(f) for f in glob.glob(os.path.join(args.work, PKG, "csrc", "*.hip")))
        merged = {new: olds.split(",") for new, olds in (m.split("=") for m in args.merged)}
        split = {old: news.split(",") for old, news in (m.split("=") for m in args.split)}
        names = [n for n in names if n in split or not any(n in news for news in split.values())]
        jobs = []
        for n in names:
            for d in (args.defines if args.defines is not None else [""] + (V7_DEFINES if n == "gemm_bf16_v7.hip" else [])):
                jobs.append((n, d))
        with concurrent.futures.ThreadPoolExecutor(args.j) as pool:
            futs = {(t, n, d): pool.submit(assembly, t, n, d) for n, d in jobs for t in (base, args.work) if t == args.work or n not in merged}
            futs.update({(base, o, ""): pool.submit(assembly, base, o, "") for olds in merged.values() for o in olds})
            futs.update({(args.work, x, ""): pool.submit(assembly, args.work, x, "") for news in split.values() for x in news})
            differ = 0
            for n, d in jobs:
                label = n + (f" [-D{d}]" if d else "")
                if n in merged or n in split:
                    if n in merged:
                        fa = {k: v for o in merged[n] for k, v in functions(normalise(futs[(base, o, "")].result())).items()}
                        fb = functions(normalise(futs[(args.work, n, d)].result()))
                    else:
                        fa = functions(normalise(futs[(base, n, d)].result()))
                        fb = {k: v for x in split[n] for k, v in functions(normalise(futs[(args.work, x, "")].result())).items()}
                    states = {k: "only in base" if k not in fb else "only in work" if k not in fa else "identical" if fa[k] == fb[k] else "DIFFERENT"
                              for k in sorted(set(fa) | set(fb))}
                    same = sum(s == "identical" for s in states.values())
                    differ += same != len(states)
                    print(f"{'MERGED' if n in merged else 'SPLIT':10s} {label} {'<-' if n in merged else '->'} {' + '.join((merged if n in merged else split)[n])}"
                          f"  ({same} of {len(states)} functions identical)")
                    for k, state in states.items():
                        print(f"    {state:13s} {k}")
                    continue
                a, b = normalise(futs[(base, n, d)].result()), normalise(futs[(args.work, n, d)].result())
                if a == b:
                    print(f"IDENTICAL  {label}  ({len(a)} lines)")
                    continue
                ra, rb = [], []
                fa, fb = functions(a, ra), functions(b, rb)
                if fa == fb and sorted(ra) == sorted(rb):      # the templates were instantiated in another order: same code, another layout
                    print(f"REORDERED  {label}  ({len(fa)} functions and descriptors identical, emitted in another order)")
                    continue
                differ += 1
                print(f"DIFFERENT  {label}\n{first_hunk(a, b)}")
                if args.by_function:
                    for k in sorted(set(fa) | set(fb)):
                        state = "only in base" if k not in fb else "only in work" if k not in fa else "identical" if fa[k] == fb[k] else "DIFFERENT"
                        print(f"    {state:13s} {k}")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
