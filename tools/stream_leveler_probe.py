"""Loudness target on streams on the long-form stream that §8k measures: the full model, 2000 phonemes, 256-frame chunks (55
calls), at 16 kHz s16 and 44.1 kHz f32.  (a) the level stream without a leveler, whole-stream time and first-chunk time, of this tree and of
the parent's: the claim to check is that it stays within the parent's own run-to-run spread; (b) the same stream with
StreamLeveler(-16): what the follower adds to the stream and to the first delivered samples; (c) the five launches' times per replay from a
kernel trace.  A library without the entry point (the parent commit) reports the stream without a leveler only, so the same file measures
both sides of the comparison.

  python tools/stream_leveler_probe.py --report profiles/stream_leveler_probe.txt --other DIR [--rounds 2] [--runs 5]
      everything the report holds, written by this call: every measurement is a fresh child process, the two trees alternate (tree, other,
      other, tree, ...), and nothing more is started after a child that failed.
  python tools/stream_leveler_probe.py [--root DIR] [--runs 5]
      one process of the stream timings of the tree at DIR (this one without), as JSON lines.
  python tools/stream_leveler_probe.py --only-kernels
      one levelled stream per format, for a kernel trace."""
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
FORMATS = ((16000, "s16"), (44100, "f32"))
KERNELS = ("k_lvl_zero", "k_lvl_fold", "k_lvl_rerun", "k_lvl_schedule", "k_lvl_apply")


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
    return traced.replace("(anonymous namespace)::", "").split("(")[0].split("<")[0].split("::")[-1].split(".")[0].split()[-1].strip()


def cell(v):
    return f"{v[0]:.2f} ({v[1]:.2f}, {v[2]:.2f})"


def report(a):
    me, roots = os.path.abspath(__file__), {"tree": ROOT, "other": os.path.abspath(a.other)}
    out = ["Loudness target on streams: what the fed leveler adds to the long-form level stream, and what the level stream without it costs beside",
           f"the parent commit.  Written by tools/stream_leveler_probe.py --report --other DIR --rounds {a.rounds} --runs {a.runs} in one call on one",
           "MI355X; `tree` is this tree, `other` the parent commit built at DIR; every line of a table is one process, in the order in which they ran.",
           "", "Workload: one utterance of 2000 phonemes at full model shapes, forced durations, 256-frame chunks, streamed as a request of one row with",
           "StreamLevel(0, -1); with = StreamLeveler(-16) besides.  whole = begin to the last piece, first = begin to the first piece that holds",
           f"samples; median (min, max) in ms of {a.runs} streams after one warm-up.  The stream without a leveler is measured before and after.", ""]
    recs = []
    for name in alternating(a.rounds):
        lines = [json.loads(ln) for ln in child([sys.executable, me, "--root", roots[name], "--runs", str(a.runs)], roots[name], 900).splitlines()
                 if ln.startswith("{")]
        recs.append((name, lines))
        print(name, lines, flush=True)
    for what in ("whole", "first"):
        out.append(f"  {what:6}{'':6}{'format':12}{'without, before':28}{'without, after':28}{'with':28}")
        for name, lines in recs:
            for rec in lines:
                with_ = cell(rec[f"leveler_{what}"]) if f"leveler_{what}" in rec else "-"
                out.append(f"  {'':6}{name:6}{rec['format']:12}{cell(rec[f'plain_1_{what}']):28}{cell(rec[f'plain_2_{what}']):28}{with_:28}")
        out.append("")
    for r, e in FORMATS:
        fmt = f"{e} {r}"
        for what in ("whole", "first"):
            med = {n: [rec[k][0] for nn, lines in recs if nn == n for rec in lines if rec["format"] == fmt for k in (f"plain_1_{what}", f"plain_2_{what}")]
                   for n in roots}
            add = [rec[f"leveler_{what}"][0] - 0.5 * (rec[f"plain_1_{what}"][0] + rec[f"plain_2_{what}"][0]) for _, lines in recs for rec in lines
                   if rec["format"] == fmt and f"leveler_{what}" in rec]
            out.append(f"  {fmt} {what}: medians without a leveler, tree {min(med['tree']):.2f} - {max(med['tree']):.2f} ms, other {min(med['other']):.2f} - "
                       f"{max(med['other']):.2f} ms; with, above the mean of the same process's two medians without: {min(add):+.2f} .. {max(add):+.2f} ms")
    out.append("")
    # the kernels under the tracer, in a process of their own
    with tempfile.TemporaryDirectory() as d:
        child(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "run", "--", sys.executable, me, "--only-kernels"], ROOT, 900)
        rows = [r for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True) for r in csv.DictReader(open(f))]
    named = [(kernel_name(r["Kernel_Name"]), r) for r in rows]
    out += ["Kernel trace of this tree (rocprofv3 --kernel-trace, a process of its own: one levelled stream per format; us per launch, one launch of",
            "each per replay that completes a segment / a quarter / holds a sample)",
            f"  {'kernel':22}{'launches':10}{'median':10}{'min':10}{'max':10}{'sum, ms':10}"]
    for k in KERNELS:
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for n, r in named if n == k]
        if not us:
            raise SystemExit(f"the trace does not hold {k}: {sorted({n for n, _ in named})[:60]}")
        out.append(f"  {k:22}{len(us):<10}{statistics.median(us):<10.2f}{min(us):<10.2f}{max(us):<10.2f}{sum(us) / 1e3:<10.3f}")
        print(out[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.report)), exist_ok=True)
    open(a.report, "w").write("\n".join(out) + "\n")
    print(f"wrote {a.report}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
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

    has = "sbv2_stream_begin_request_leveler" in _lib.SYMBOLS
    bc, vc = O.DEBERTA_FULL, O.VITS_FULL
    bs = model.load_model(synth.pack_blob(synth.KIND_BERT, bc, synth.make_deberta_weights(bc, 0x5B72)), True)
    vs = model.load_model(synth.pack_blob(synth.KIND_VITS, vc, synth.make_vits_weights(vc, 0x5B72)), False)
    u = synth.make_utterance(2000, bc, vc, seed=991)

    def stream(fmt, levelled):
        kw = dict(leveler=model.StreamLeveler(-16.0)) if levelled else {}
        t0 = time.perf_counter()
        st = model.StreamHandle(bs, vs, [u], 256, fmt=fmt, gaps=[0], level=model.StreamLevel(0.0, -1.0), forced=True, **kw)
        first = None
        while (c := st.next()) is not None:
            if first is None and len(c):
                first = time.perf_counter() - t0
        whole = time.perf_counter() - t0
        stats = st.leveler_stats() if levelled else None
        st.close()
        return whole * 1e3, first * 1e3, stats

    if a.only_kernels:
        for r, e in FORMATS:
            stream(model.PcmFormat(r, e), True)
        bs.close(); vs.close()
        return

    def timeit(fmt, levelled):
        stream(fmt, levelled)
        t = [stream(fmt, levelled) for _ in range(a.runs)]
        d = {w: [round(float(f([x[i] for x in t])), 3) for f in (np.median, np.min, np.max)] for i, w in enumerate(("whole", "first"))}
        return d, t[-1][2]

    for r, e in FORMATS:
        fmt = model.PcmFormat(r, e)
        rec = {"format": f"{e} {r}", "runs": a.runs}
        for key, levelled in [("plain_1", False)] + ([("leveler", True)] if has else []) + [("plain_2", False)]:
            d, stats = timeit(fmt, levelled)
            for w, v in d.items():
                rec[f"{key}_{w}"] = v
            if stats is not None:
                rec["leveler_stats"] = [round(v, 4) if np.isfinite(v) else None for v in stats]
        print(json.dumps(rec), flush=True)
    bs.close(); vs.close()


if __name__ == "__main__":
    main()
