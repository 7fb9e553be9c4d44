"""Are the kernels of two source trees the same machine code?  Compiles every csrc/*.hip of both trees to gfx950 assembly (the
Makefile's flags + --cuda-device-only -S) and compares, kernel by kernel, the instruction stream and the .amdhsa_* descriptor block
(registers, LDS, scratch), with branch labels renumbered and the kernel's own symbol masked -- so that a refactor that only removes
kernels or drops a template parameter shows as "same" for every kernel it keeps.  No GPU needed.

    python tools/isa_compare.py --before <parent checkout>/mvsdet_amd/csrc [--after mvsdet_amd/csrc] [--out profiles/NAME.txt] [--brief]

One line per kernel: name, VGPRs (arch + acc), SGPRs, LDS and scratch bytes, instructions, hash before, hash after, verdict.
Exit status 1 if a kernel present on both sides differs."""
import argparse
import hashlib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CXXFILT = os.environ.get("CXXFILT", "c++filt")
FLAGS = "-O3 --offload-arch=gfx950 -std=c++17 -fPIC -ffp-contract=off -fno-math-errno -Wall -Wno-unused-function".split()

# Template parameters that a kernel had in --before and no longer has in --after: (index, the value every kept instantiation had).
# A --before instantiation with another value there has no counterpart and is listed as removed.
# Filled in for the comparison at hand -- {"mvsdet::store_pattern_kernel": (2, "false")} when its PAIR parameter went, for
# profiles/retired_forms_isa.txt -- and empty when the kernels of both trees have the same template parameters.
DROPPED_PARAMS = {}
# Template parameters that a kernel has gained at its END in --after: the values that stand for the --before kernel.  An --after
# instantiation with exactly these trailing values is compared under its --before name; any other is listed as ADDED.
# {"mvsdet::plane_sweep_variance_kernel": ["0", "0"]} for the store / load policies (profiles/r10_sweep_store_policy_isa.txt).
ADDED_PARAMS = {}


def assemble(src: str, out: str) -> None:
    if os.path.exists(out):   # --asm-dir: kept from an earlier run
        return
    subprocess.run([HIPCC, *FLAGS, "--cuda-device-only", "-S", os.path.basename(src), "-o", out], cwd=os.path.dirname(src),
                   check=True, stderr=subprocess.DEVNULL)


def demangle(names):
    if not names:
        return []
    out = subprocess.run([CXXFILT, "-p"], input="\n".join(names) + "\n", capture_output=True, text=True, check=True)
    return [re.sub(r"^void ", "", n.strip()) for n in out.stdout.splitlines()]


def split_args(s: str):
    args, depth, cur = [], 0, ""
    for ch in s:
        if ch in "<(":
            depth += 1
        elif ch in ">)":
            depth -= 1
        if ch == "," and depth == 0:
            args.append(cur.strip())
            cur = ""
        else:
            cur += ch
    return args + [cur.strip()] if cur.strip() else args


def drop_param(name: str) -> str:
    m = re.match(r"^([\w:]+)<(.*)>$", name)
    if not m or m.group(1) not in DROPPED_PARAMS:
        return name
    idx, kept = DROPPED_PARAMS[m.group(1)]
    args = split_args(m.group(2))
    if idx < len(args) and args[idx] == kept:
        del args[idx]
        return f"{m.group(1)}<{', '.join(args)}>"
    return name + "   [retired form]"


def strip_added(name: str) -> str:
    m = re.match(r"^([\w:]+)<(.*)>$", name)
    if not m or m.group(1) not in ADDED_PARAMS:
        return name
    tail = ADDED_PARAMS[m.group(1)]
    args = split_args(m.group(2))
    if args[-len(tail):] == tail:
        return f"{m.group(1)}<{', '.join(args[:-len(tail)])}>"
    return name


def kernels_of(asm_path: str, before: bool):
    """{demangled kernel name: (figures, hash, instruction count)}"""
    text = open(asm_path).read()
    lines = text.splitlines()
    mangled = re.findall(r"^\s*\.amdhsa_kernel (\S+)", text, re.M)
    pretty = demangle(mangled)
    res = {}
    for sym, name in zip(mangled, pretty):
        start = lines.index(next(l for l in lines if l.startswith(sym + ":")))
        labels, body = {}, []
        i = start + 1
        while not lines[i].startswith(".Lfunc_end"):
            l = lines[i].split(";")[0].rstrip()
            i += 1
            if not l.strip() or (l.lstrip().startswith(".") and not l.rstrip().endswith(":")):
                continue   # comments, directives (.p2align ...)
            body.append(l.strip())
        ninstr = sum(1 for l in body if not l.endswith(":"))

        def label(m):
            return labels.setdefault(m.group(0), f".L{len(labels)}")
        body = [re.sub(r"\.LBB\d+_\d+", label, l).replace(sym, "@K") for l in body]
        d0 = next(k for k, l in enumerate(lines) if l.strip() == ".amdhsa_kernel " + sym)
        d1 = next(k for k in range(d0, len(lines)) if lines[k].strip() == ".end_amdhsa_kernel")
        desc = [l.strip() for l in lines[d0 + 1:d1]]
        val = {l.split()[0]: l.split()[1] for l in desc}
        h = hashlib.sha256("\n".join(body + desc).encode()).hexdigest()[:16]
        vg, acc = int(val[".amdhsa_next_free_vgpr"]), int(val[".amdhsa_accum_offset"])
        fig = (f"vgpr {min(vg, acc)}+{max(vg - acc, 0)}", f"sgpr {val['.amdhsa_next_free_sgpr']}", f"lds {val['.amdhsa_group_segment_fixed_size']}",
               f"scratch {val['.amdhsa_private_segment_fixed_size']}")
        res[drop_param(name) if before else strip_added(name)] = (fig, h, ninstr)
    return res


def tree(csrc: str, tmp: str, tag: str, jobs: int):
    srcs = sorted(f for f in os.listdir(csrc) if f.endswith(".hip"))
    outs = {f: os.path.join(tmp, f"{tag}_{f}.s") for f in srcs}
    with ThreadPoolExecutor(jobs) as ex:
        list(ex.map(lambda f: assemble(os.path.join(csrc, f), outs[f]), srcs))
    return {f: kernels_of(outs[f], tag == "before") for f in srcs}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap.add_argument("--before", required=True, help="csrc directory of the tree to compare against")
    ap.add_argument("--after", default=os.path.join(here, "mvsdet_amd", "csrc"))
    ap.add_argument("--out", default=None, help="also write the table to this file")
    ap.add_argument("--jobs", type=int, default=4)
    ap.add_argument("--asm-dir", default=None, help="keep the assembly here (before_*.s, after_*.s) and reuse what is already there")
    ap.add_argument("--brief", action="store_true", help="list only the kernels that are not the same; each file's line counts the rest")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmpdir:
        tmp = os.path.abspath(a.asm_dir) if a.asm_dir else tmpdir   # assemble() runs the compiler inside the source directory
        os.makedirs(tmp, exist_ok=True)
        before = tree(os.path.abspath(a.before), tmp, "before", a.jobs)
        after = tree(os.path.abspath(a.after), tmp, "after", a.jobs)
    rows, same, differ, removed, added = [], 0, 0, 0, 0
    for f in sorted(set(before) | set(after)):
        kb, ka = before.get(f, {}), after.get(f, {})
        unlisted = sum(1 for name in set(kb) & set(ka) if kb[name] == ka[name]) if a.brief else 0
        rows.append(f"## {f}: {len(kb)} kernels before, {len(ka)} after" + (f", {unlisted} of them same and not listed" if a.brief else ""))
        for name in sorted(set(kb) | set(ka)):
            b, k = kb.get(name), ka.get(name)
            fig, n = (k or b)[0], (k or b)[2]
            if b and k:
                ok = b == k
                same, differ = same + ok, differ + (not ok)
                verdict = "same" if ok else f"DIFFERENT (before: {', '.join(b[0])}, {b[2]} instructions)"
            else:
                removed, added = removed + (k is None), added + (b is None)
                verdict = "removed" if k is None else "ADDED"
            if a.brief and verdict == "same":
                continue
            rows.append(f"{name} | {' | '.join(fig)} | {n} instructions | {b[1] if b else '-':16} | {k[1] if k else '-':16} | {verdict}")
    rows.append(f"## total: {same} same, {differ} different, {removed} removed, {added} added")
    text = "\n".join(["# kernel | registers | LDS | scratch | instructions | hash before | hash after | verdict (tools/isa_compare.py)"] + rows) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)
    return 1 if differ or added else 0


if __name__ == "__main__":
    sys.exit(main())
