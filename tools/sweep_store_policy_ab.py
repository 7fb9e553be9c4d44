#!/usr/bin/env python3
"""A/B of the plane sweep's cache policies (options "sweep_store" / "sweep_box_load"): the job behind
profiles/r10_sweep_store_policy_ab.txt.  One job on one box, a fresh process per line, every GPU step under its own `timeout`,
and the first step that fails ends the job.

Libraries (built beforehand, where the compiler is):
    P  the parent commit's library                 (make in a checkout of the parent; --parent, default build_ab/libP.so)
    Z  this tree's default build, sweep_store 0    (make;                              mvsdet_amd/libmvsdet_hip.so)
    D  the same at its defaults (sweep_store -1: what ships per class)
    C  the A/B build under one candidate flavour   (make SWEEP_STORE_MATRIX=1;         --matrix, default build_ab/libM.so)
A candidate is "STORE,LOAD": sweep_store 1 plain, 2 sc1, 3 sc0 sc1, 4 nt sc1, 5 nt through the buffer store (the control: the
shipped policy on the other store instruction); sweep_box_load 1 = nt box DMA and reference loads.  Label C<store><load>.

Stages (--stages, comma separated; the default is all of them in this order):
    probe     stores alone: ops.store_pattern_probe per store flavour at the headline volume, 5 launches each
    headline  bench.py --gpus 1 --steps 20 --warmup 3, alternating P, Z and every candidate, --rounds rounds (5)
    shapes    the same at arkit_50v_96d_60x80 and scannet_ref_40v_12d_60x80, --shape-rounds rounds (3)
    dump      bench.py --dump-outputs at the headline, P against --chosen: every array must be EQUAL
    trace     rocprofv3 --kernel-trace --stats around one plain bench.py run, P and --chosen
    pmc       rocprofv3 --pmc alone (no tracing beside it): L2 hit / miss and write-request counters of one sweep launch, P and --chosen
Everything is printed and also written to <--out>/record.txt; the rule of the issue is evaluated at the end of `headline` / `shapes`.

    python tools/sweep_store_policy_ab.py --candidates 1,0 2,0 3,0 4,0 5,0 0,1 --chosen 2,0
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
from collections import defaultdict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = "scannet_40v_64d_120x160"
OTHER_SHAPES = ("arkit_50v_96d_60x80", "scannet_ref_40v_12d_60x80")
STORE_NAMES = {0: "nt", 1: "plain", 2: "sc1", 3: "sc0 sc1", 4: "nt sc1", 5: "nt (buffer store)"}
# one set per run (rocprofv3 collects what fits one pass); the TCC write-request counters as this rocprofv3 names them
PMC_SETS = ("TCC_HIT_sum TCC_MISS_sum TCC_REQ_sum", "TCC_READ_sum TCC_WRITE_sum TCC_EA0_WRREQ_sum TCC_EA0_WRREQ_64B_sum",
            "FETCH_SIZE", "WRITE_SIZE")   # derived counters: one per pass (three in one pass: "exceeds the capabilities of the hardware")

_record = None


def say(line):
    print(line, flush=True)
    if _record:
        _record.write(line + "\n")
        _record.flush()


def step(cmd, env_extra, seconds, what):
    """one GPU step in a fresh process under its own time limit; a failure ends the job (nothing more starts on the GPU)"""
    env = dict(os.environ, PYTHONPATH=ROOT, **env_extra)
    r = subprocess.run(["timeout", "-k", "10", str(seconds)] + cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        say(f"FAILED ({r.returncode}): {what}: {' '.join(cmd)}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
        sys.exit(r.returncode or 1)
    return r.stdout


def env_of(label, a):
    """P, Z, D or C<store><load> -> the environment that selects the library and the flavour"""
    if label == "P":
        return {"MVSDET_HIP_LIB": os.path.abspath(a.parent)}
    if label == "Z":
        return {"MVSDET_HIP_LIB": os.path.join(ROOT, "mvsdet_amd", "libmvsdet_hip.so"), "MVSDET_SWEEP_STORE": "0", "MVSDET_SWEEP_BOX_LOAD": "0"}
    if label == "D":
        return {"MVSDET_HIP_LIB": os.path.join(ROOT, "mvsdet_amd", "libmvsdet_hip.so")}
    return {"MVSDET_HIP_LIB": os.path.abspath(a.matrix), "MVSDET_SWEEP_STORE": label[1], "MVSDET_SWEEP_BOX_LOAD": label[2]}


def label_of(cand):
    s, l = cand.split(",")
    return f"C{int(s)}{int(l)}"


def bench_line(label, rnd, workload, a, extra=()):
    out = step([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "3", "--workload", workload, *extra],
               env_of(label, a), 240, f"bench {label} {workload}")
    j = json.loads([l for l in out.splitlines() if l.startswith("{")][-1])
    r = j["roofline"]
    say(f"{label} {rnd} {workload} ms_per_step {j['ms_per_step']} value {j['value']} kernel_ms {r['kernel_ms']} "
        f"{r['kernel_ms_min_median_max']} table_kernel_ms {r['table_kernel_ms']} checksum {j['checksum']}")
    return j


def median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def ab(workload, labels, rounds, a):
    runs = defaultdict(list)
    for rnd in range(1, rounds + 1):
        for label in labels:
            runs[label].append(bench_line(label, rnd, workload, a))
    say(f"\nPer build at {workload} over the {rounds} runs (min / median / max):")
    stat = {}
    for label in labels:
        ms = [j["ms_per_step"] for j in runs[label]]
        km = [j["roofline"]["kernel_ms"] for j in runs[label]]
        val = [j["value"] for j in runs[label]]
        stat[label] = (ms, val)
        say(f"{label} {workload}: ms_per_step {min(ms):.4f} / {median(ms):.4f} / {max(ms):.4f}; kernel_ms {min(km):.4f} / {median(km):.4f} / "
            f"{max(km):.4f}; cost volumes/s {min(val):.1f} / {median(val):.1f} / {max(val):.1f}")
    if len({j["checksum"] for js in runs.values() for j in js}) != 1:
        say(f"CHECKSUMS DIFFER at {workload}")
        sys.exit(1)
    # the rule: every C run above every P run in cost volumes/s, and the fall of the median ms_per_step at least twice P's own spread
    p_ms, p_val = stat["P"]
    spread = max(p_ms) - min(p_ms)
    say(f"P's own spread at {workload}: {spread:.4f} ms = {100 * spread / median(p_ms):.2f} % of its median {median(p_ms):.4f}")
    for label in labels:
        if label == "P":
            continue
        ms, val = stat[label]
        fall = median(p_ms) - median(ms)
        if label == "Z":
            inside = min(p_ms) <= median(ms) <= max(p_ms)
            say(f"Z median {median(ms):.4f} {'inside' if inside else 'OUTSIDE'} P's range [{min(p_ms):.4f}, {max(p_ms):.4f}]")
            continue
        above = min(val) > max(p_val)
        passes = above and fall >= 2 * spread
        say(f"{label} ({describe(label)}): median falls by {fall:+.4f} ms ({100 * fall / median(p_ms):+.2f} %), {fall / spread if spread else float('inf'):.2f} x P's spread; "
            f"every run above every P run: {above} -> {'PASSES' if passes else 'does not pass'} the rule; "
            f"{'loses beyond P spread' if -fall > spread else 'no loss beyond P spread'}")
    return stat


def describe(label):
    if label == "D":
        return "this tree's default build at its defaults: sweep_store -1, what ships per class"
    return f"sweep_store {STORE_NAMES[int(label[1])]}, box loads {'nt' if label[2] == '1' else 'default'}"


def probe_child(workload):
    """(child process) the store pattern alone under the MVSDET_SWEEP_STORE of the environment"""
    import torch
    sys.path.insert(0, ROOT)
    import bench
    from mvsdet_amd import _lib
    sp = bench.store_pattern_ceiling(bench.WORKLOADS[workload], torch.device("cuda:0"), reps=5)
    print(json.dumps({"sweep_store": _lib.get_option("sweep_store"), **sp}))


def stage_probe(a):
    say(f"## stores alone: ops.store_pattern_probe at {HEADLINE}, median of 5 launches (bench.store_pattern_ceiling), library C")
    for s in sorted(STORE_NAMES):
        out = step([sys.executable, os.path.abspath(__file__), "--probe-child", HEADLINE],
                   {"MVSDET_HIP_LIB": os.path.abspath(a.matrix), "MVSDET_SWEEP_STORE": str(s)}, 180, f"probe {s}")
        j = json.loads(out.splitlines()[-1])
        assert j["sweep_store"] == s
        say(f"probe sweep_store {s} ({STORE_NAMES[s]}): {j['ms']} ms {j['GBps']} GB/s tile {j['tile']} bytes {j['bytes']}")


def stage_dump(a):
    import numpy as np
    say(f"\n## --dump-outputs at the headline, P against {label_of(a.chosen)} (bench.py --steps 3 --warmup 1)")
    dirs = {}
    for label in ("P", label_of(a.chosen)):
        dirs[label] = os.path.join(a.out, "dump_" + label)
        os.makedirs(dirs[label], exist_ok=True)
        step([sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1", "--workload", HEADLINE, "--dump-outputs", dirs[label]],
             env_of(label, a), 300, f"dump {label}")
    bad = 0
    for f in sorted(os.listdir(dirs["P"])):
        if not f.endswith(".npy"):
            continue
        x, y = np.load(os.path.join(dirs["P"], f)), np.load(os.path.join(dirs[label_of(a.chosen)], f))
        eq = x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x, y, equal_nan=True)
        bad += not eq
        say(f"{f}: {x.dtype} {x.shape} {'EQUAL' if eq else 'DIFFERENT'}")
    for d in dirs.values():   # the arrays are large: the record keeps the verdicts
        for f in os.listdir(d):
            os.remove(os.path.join(d, f))
    if bad:
        sys.exit(1)


def stage_trace(a):
    say("\n## rocprofv3 --kernel-trace --stats of a plain bench.py run (23 launches: 3 warm-up + 20)")
    for label in ("P", label_of(a.chosen)):
        d = os.path.join(a.out, "kt_" + label)
        step(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "bench", "--", sys.executable, "bench.py", "--gpus", "1",
              "--steps", "20", "--warmup", "3", "--workload", HEADLINE], env_of(label, a), 420, f"kernel trace {label}")
        for path in glob.glob(d + "/**/*kernel_stats.csv", recursive=True):
            for i, line in enumerate(open(path).read().splitlines()[:6]):
                say(f"{label} {line[:200]}")
        for path in glob.glob(d + "/**/*kernel_trace.csv", recursive=True):
            os.remove(path)


def stage_pmc(a):
    say("\n## rocprofv3 --pmc, runs of their own (tools/profile_sweep.py scannet_40v_64d_120x160 1 tabled: one launch, seed-0 scene)")
    for label in ("P", label_of(a.chosen)):
        for i, cset in enumerate(PMC_SETS, 1):
            d = os.path.join(a.out, f"pmc_{label}_{i}")
            step(["rocprofv3", "--pmc", *cset.split(), "--output-format", "csv", "-d", d, "-o", "pmc", "--", sys.executable, "tools/profile_sweep.py",
                  HEADLINE, "1", "tabled"], env_of(label, a), 300, f"pmc {label} set {i}")
            for path in glob.glob(d + "/**/*counter_collection.csv", recursive=True):
                acc = defaultdict(lambda: defaultdict(float))
                with open(path) as f:
                    for row in csv.DictReader(f):
                        if "plane_sweep_variance_kernel" in row["Kernel_Name"]:
                            acc[row["Counter_Name"]][row["Dispatch_Id"]] += float(row["Counter_Value"])
                for c, per in sorted(acc.items()):
                    say(f"{label} set {i} plane_sweep_variance_kernel {c:24s} dispatches={len(per)} mean={sum(per.values()) / len(per):.5e}")
                os.remove(path)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent", default=os.path.join(ROOT, "build_ab", "libP.so"))
    ap.add_argument("--matrix", default=os.path.join(ROOT, "build_ab", "libM.so"))
    ap.add_argument("--candidates", nargs="*", default=["1,0", "2,0", "3,0", "4,0", "5,0", "0,1"])
    ap.add_argument("--chosen", default=None, help="STORE,LOAD of the flavour that dump / trace / pmc set against P")
    ap.add_argument("--stages", default="probe,headline,shapes,dump,trace,pmc")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shape-rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "build_ab", "sweep_store_policy_ab"),
                    help="directory for record.txt and the profiler's files (build_ab/ is untracked)")
    ap.add_argument("--probe-child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.probe_child:
        return probe_child(a.probe_child)
    global _record
    os.makedirs(a.out, exist_ok=True)
    _record = open(os.path.join(a.out, "record.txt"), "a")
    labels = ["P", "Z", "D"] + [label_of(c) for c in a.candidates]
    stages = a.stages.split(",")
    if a.chosen is None and {"dump", "trace", "pmc"} & set(stages):
        ap.error("--chosen STORE,LOAD is needed for dump / trace / pmc")
    say(f"# stages {a.stages}; candidates {' '.join(f'{label_of(c)} = {describe(label_of(c))}' for c in a.candidates)}")
    for st in stages:
        if st == "probe":
            stage_probe(a)
        elif st == "headline":
            say(f"\n## A/B at the headline, {a.rounds} rounds")
            ab(HEADLINE, labels, a.rounds, a)
        elif st == "shapes":
            for wl in OTHER_SHAPES:
                say(f"\n## A/B at {wl}, {a.shape_rounds} rounds")
                ab(wl, labels, a.shape_rounds, a)
        elif st == "dump":
            stage_dump(a)
        elif st == "trace":
            stage_trace(a)
        elif st == "pmc":
            stage_pmc(a)
        else:
            ap.error(f"unknown stage {st}")


if __name__ == "__main__":
    main()
