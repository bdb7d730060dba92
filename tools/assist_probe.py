"""Assist probe: the step time of the bench batch (32 x 128 phonemes at full model size, synthetic weights, forced durations) without an assist
text, with ONE 32-token assist text shared by all rows, and with 32 distinct 32-token assist texts (weight 0.7): the median wall time of
`--iters` steps (Pipeline.run + sync) after two warm-up steps.  The step without is timed twice, before and after the steps with, so that the
record carries its own run-to-run spread.  A library without the assist entry point (an older commit) reports the step without only, so the
same file measures both sides of a comparison.

  python tools/assist_probe.py --report profiles/assist_probe.txt --other DIR [--rounds 2] [--iters 10]
      everything profiles/assist_probe.txt holds, written by this call: the steps of this tree and of the tree at DIR (the parent commit,
      built), and the two assist kernels' times from a rocprofv3 kernel trace of this tree.  Every measurement is a fresh child process, the
      two trees alternate (tree, other, other, tree, ...), and nothing more is started after a child that failed.
  python tools/assist_probe.py [--root DIR] [--iters 10]
      one process of the step timings of the tree at DIR (this one without), as one JSON line.
  python tools/assist_probe.py --only-kernels [--iters 4]
      steps with the shared and with the distinct assist texts alone, for a kernel trace (k_assist_mean, k_gather_cols_assist)."""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("k_assist_mean", "k_gather_cols_assist")
CASES = ("shared", "distinct")
ASSIST_TOKENS, WEIGHT = 32, 0.7


def child(cmd, cwd, limit):
    """One measurement in a process of its own -> its stdout; a failure ends the probe (nothing more is started on the device)."""
    r = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=limit)
    if r.returncode != 0:
        print(r.stdout[-2000:], r.stderr[-2000:])
        raise SystemExit(f"{' '.join(cmd)} in {cwd} ended with {r.returncode}")
    return r.stdout


def alternating(rounds):
    for i in range(rounds):
        yield from ("tree", "other") if i % 2 == 0 else ("other", "tree")


def kernel_name(traced):
    """k_assist_mean of "sbv2::k_assist_mean(sbv2::Plane, int const*, int const*, int, float*) [clone .kd]" and its like."""
    return traced.replace("(anonymous namespace)::", "").split("(")[0].split("<")[0].split("::")[-1].split(".")[0].split()[-1].strip()


def cell(v):
    return f"{v[0]:.3f} ({v[1]:.3f}, {v[2]:.3f})"


def report(a):
    me, roots = os.path.abspath(__file__), {"tree": ROOT, "other": os.path.abspath(a.other)}
    out = ["Assist text: what the extra DeBERTa columns and the two assist kernels add to a step of the bench batch, and what the step without an",
           f"assist costs beside the parent commit.  Written by tools/assist_probe.py --report --other DIR --rounds {a.rounds} --iters {a.iters} in one call",
           "on one MI355X; `tree` is this tree, `other` the parent commit built at DIR; every line of the table is one process, in the order in which",
           "they ran.",
           "",
           "Workload: the bench batch (32 x 128 phonemes, full model shapes, synthetic weights, forced durations; 1088 DeBERTa tokens).  shared: one",
           f"{ASSIST_TOKENS}-token assist text named by all 32 rows (+{ASSIST_TOKENS} tokens); distinct: 32 different {ASSIST_TOKENS}-token assist texts, one per row",
           f"(+{32 * ASSIST_TOKENS} tokens); weight {WEIGHT}.  Median (min, max) wall time in ms of {a.iters} steps (sbv2_pipeline_run* + sync) after two warm-up",
           "steps; the step without is measured before and after the steps with.", ""]
    # the kernels under the tracer, in a process of their own and ahead of the timed ones
    with tempfile.TemporaryDirectory() as d:
        child(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "run", "--", sys.executable, me, "--only-kernels", "--iters", "4"],
              ROOT, 900)
        rows = [r for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True) for r in csv.DictReader(open(f))]
    named = [(kernel_name(r["Kernel_Name"]), r) for r in rows]
    if not all(any(n == k for n, _ in named) for k in KERNELS):
        raise SystemExit(f"the trace does not hold {KERNELS}: {sorted({r['Kernel_Name'] for r in rows})[:40]}")
    # 1. the steps
    recs = []
    for name in alternating(a.rounds):
        rec = [json.loads(ln) for ln in child([sys.executable, me, "--root", roots[name], "--iters", str(a.iters)], roots[name], 900).splitlines()
               if ln.startswith("{")][-1]
        recs.append((name, rec))
        print(name, rec, flush=True)
    out.append(f"  {'':8}{'without, before':28}{'without, after':28}{'shared':28}{'distinct':28}")
    for name, rec in recs:
        with_ = [cell(rec[f"{c}_ms"]) if f"{c}_ms" in rec else "-" for c in CASES]
        out.append(f"  {name:8}{cell(rec['none_ms_1']):28}{cell(rec['none_ms_2']):28}{with_[0]:28}{with_[1]:28}")
    out.append("")
    med = {n: [rec[k][0] for nn, rec in recs if nn == n for k in ("none_ms_1", "none_ms_2")] for n in roots}
    add = {c: [rec[f"{c}_ms"][0] - 0.5 * (rec["none_ms_1"][0] + rec["none_ms_2"][0]) for _, rec in recs if f"{c}_ms" in rec] for c in CASES}
    out.append(f"  medians of the step without an assist: tree {min(med['tree']):.3f} - {max(med['tree']):.3f} ms, other {min(med['other']):.3f} - "
               f"{max(med['other']):.3f} ms")
    out.append("  the step with, above the mean of the same process's two medians without: " +
               ", ".join(f"{c} {min(add[c]):+.3f} .. {max(add[c]):+.3f} ms" for c in CASES))
    out.append("")
    # 2. the kernels
    out += ["Kernel trace of this tree (rocprofv3 --kernel-trace, a process of its own: 4 steps with the shared text and 4 with the distinct ones,",
            "alternating; us; the larger launches of k_assist_mean are the distinct case's)",
            f"  {'kernel':24}{'launches':10}{'median':10}{'min':10}{'max':10}{'workgroups x lanes of the last launch'}"]
    for k in KERNELS:
        sel = [r for n, r in named if n == k]
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in sel]
        wg = int(sel[-1]["Workgroup_Size_X"])
        grid = " x ".join(str(int(sel[-1][f"Grid_Size_{ax}"]) // max(int(sel[-1][f"Workgroup_Size_{ax}"]), 1)) for ax in "XY")
        out.append(f"  {k:24}{len(us):<10}{statistics.median(us):<10.2f}{min(us):<10.2f}{max(us):<10.2f}{grid} x {wg}")
        print(out[-1], flush=True)
    plain = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for n, r in named if n == "k_gather_cols"]
    if plain:
        out.append(f"  (k_gather_cols, the gather without an assist, in the same trace: {len(plain)} launches, median {statistics.median(plain):.2f} us)")
    open(a.report, "w").write("\n".join(out) + "\n")
    print(f"wrote {a.report}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--report")
    ap.add_argument("--other")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--only-kernels", action="store_true")
    a = ap.parse_args()
    if a.report:
        if not a.other:
            raise SystemExit("--report needs --other DIR, the built tree of the parent commit")
        return report(a)
    root = os.path.abspath(a.root)
    for p in (root, os.path.join(root, "oracle")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import numpy as np
    import sbv2_oracle as O
    from sbv2_api_amd import _lib, model, synth

    has = "sbv2_pipeline_run_assist" in _lib.SYMBOLS
    bc, vc = O.DEBERTA_FULL, O.VITS_FULL
    bs = model.load_model(synth.pack_blob(synth.KIND_BERT, bc, synth.make_deberta_weights(bc, 1)), True)
    vs = model.load_model(synth.pack_blob(synth.KIND_VITS, vc, synth.make_vits_weights(vc, 2)), False)
    pipe = model.Pipeline(bs, vs)
    utts = [synth.make_utterance(128, bc, vc, seed=i) for i in range(32)]

    def text(i):
        body = 3 + np.floor(synth.hash_uniform(0xA5515 + i, ASSIST_TOKENS - 2) * (bc["vocab_size"] - 3)).astype(np.int64)
        return [1] + [int(t) for t in body] + [2]

    batches = {"none": pipe.prepare(utts, forced=True)}
    if has:
        batches["shared"] = pipe.prepare([dict(u, assist_ids=text(0), assist_weight=WEIGHT) for u in utts], forced=True)
        batches["distinct"] = pipe.prepare([dict(u, assist_ids=text(i), assist_weight=WEIGHT) for i, u in enumerate(utts)], forced=True)
        assert batches["shared"].assist.n_texts == 1 and batches["distinct"].assist.n_texts == 32 and batches["none"].assist is None

    def step(b):
        pipe.run(b)
        pipe.sync()

    if a.only_kernels:
        for _ in range(a.iters):
            for c in CASES if has else ("none",):
                step(batches[c])
        pipe.close(); bs.close(); vs.close()
        return

    def timeit(b):
        for _ in range(2):
            step(b)
        t = []
        for _ in range(a.iters):
            t0 = time.perf_counter()
            step(b)
            t.append(time.perf_counter() - t0)
        return [round(float(v) * 1e3, 3) for v in (np.median(t), np.min(t), np.max(t))]

    rec = {"iters": a.iters, "none_ms_1": timeit(batches["none"])}
    for c in CASES:
        if c in batches:
            rec[f"{c}_ms"] = timeit(batches[c])
    rec["none_ms_2"] = timeit(batches["none"])
    print(json.dumps(rec))
    pipe.close(); bs.close(); vs.close()


if __name__ == "__main__":
    main()
