"""Voice on streams on the long-form stream that §8k measures: the full model, 2000 phonemes, 256-frame chunks (55 calls).
(a) the stream without a voice, whole-stream time and first-chunk time, of this tree and of the parent's; (b) the same stream with
StreamVoice(1.2, 1.0, q) for q = 1 and 0.8 at 44.1 kHz f32 and 16 kHz s16: what the stage adds to the stream and to the first delivered
samples; the three launches' times from a kernel trace; (c) bench.py of both trees.  A library without the entry point (the parent commit)
reports the stream without a voice only, so the same file measures both sides of the comparison.

  python tools/stream_voice_probe.py --report profiles/stream_voice_probe.txt --other DIR [--rounds 2] [--runs 5]
      everything the report holds, written by this call: every measurement is a fresh child process, the two trees alternate (tree, other,
      other, tree, ...), and nothing more is started after a child that failed.
  python tools/stream_voice_probe.py [--root DIR] [--runs 5]
      one process of the stream timings of the tree at DIR (this one without), as JSON lines.
  python tools/stream_voice_probe.py --only-kernels
      one f32 voice stream at q = 1 and one at q = 0.8, for a kernel trace."""
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
FORMATS = ((44100, "f32"), (16000, "s16"))
SCALES = (1.0, 0.8)
PIVOT = 150.0   # the pivot moves targets, not the amount of work
KERNELS = ("k_stream_pitch", "k_voice_marks_fed", "k_voice_gather", "k_voice_gather_fmt")


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
    out = ["Voice on streams: what the fed shifter adds to the long-form stream, and what the stream without it and bench.py cost beside the parent",
           f"commit.  Written by tools/stream_voice_probe.py --report --other DIR --rounds {a.rounds} --runs {a.runs} in one call on one MI355X; `tree` is",
           "this tree, `other` the parent commit built at DIR; every line of a table is one process, in the order in which they ran.", "",
           "Workload: one utterance of 2000 phonemes at full model shapes, forced durations, 256-frame chunks, streamed as a request of one row.",
           f"whole = begin to the last piece, first = begin to the first piece that holds samples; median (min, max) in ms of {a.runs} streams after one",
           "warm-up.  The stream without a voice is measured before and after the streams with.", ""]
    recs = []
    for name in alternating(a.rounds):
        lines = [json.loads(ln) for ln in child([sys.executable, me, "--root", roots[name], "--runs", str(a.runs)], roots[name], 900).splitlines()
                 if ln.startswith("{")]
        recs.append((name, lines))
        print(name, lines, flush=True)
    for what in ("whole", "first"):
        out.append(f"  {what:6}{'':6}{'format':12}{'without, before':28}{'without, after':28}" + "".join(f"{'q = ' + str(q):28}" for q in SCALES))
        for name, lines in recs:
            for rec in lines:
                with_ = [cell(rec[f"voice_{q}_{what}"]) if f"voice_{q}_{what}" in rec else "-" for q in SCALES]
                out.append(f"  {'':6}{name:6}{rec['format']:12}{cell(rec[f'plain_1_{what}']):28}{cell(rec[f'plain_2_{what}']):28}" +
                           "".join(f"{w:28}" for w in with_))
        out.append("")
    for r, e in FORMATS:
        fmt = f"{e} {r}"
        for what in ("whole", "first"):
            med = {n: [rec[k][0] for nn, lines in recs if nn == n for rec in lines if rec["format"] == fmt for k in (f"plain_1_{what}", f"plain_2_{what}")]
                   for n in roots}
            add = {q: [rec[f"voice_{q}_{what}"][0] - 0.5 * (rec[f"plain_1_{what}"][0] + rec[f"plain_2_{what}"][0]) for _, lines in recs for rec in lines
                       if rec["format"] == fmt and f"voice_{q}_{what}" in rec] for q in SCALES}
            out.append(f"  {fmt} {what}: medians without a voice, tree {min(med['tree']):.2f} - {max(med['tree']):.2f} ms, other {min(med['other']):.2f} - "
                       f"{max(med['other']):.2f} ms; with, above the mean of the same process's two medians without: " +
                       ", ".join(f"q = {q} {min(add[q]):+.2f} .. {max(add[q]):+.2f} ms" for q in SCALES))
    lk = [rec["lookahead"] for _, lines in recs for rec in lines if "lookahead" in rec]
    if lk:
        out.append(f"  of the added first-piece time, A_v / 44100 = {lk[0]} / 44100 = {lk[0] / 44.1:.1f} ms is audio the decoder must produce first")
    out.append("")
    # the kernels under the tracer, in a process of their own
    with tempfile.TemporaryDirectory() as d:
        child(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "run", "--", sys.executable, me, "--only-kernels"], ROOT, 900)
        rows = [r for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True) for r in csv.DictReader(open(f))]
    named = [(kernel_name(r["Kernel_Name"]), r) for r in rows]
    out += ["Kernel trace of this tree (rocprofv3 --kernel-trace, a process of its own: one f32 voice stream at q = 1 and one at q = 0.8; us per launch)",
            f"  {'kernel':22}{'launches':10}{'median':10}{'min':10}{'max':10}{'sum, ms':10}"]
    for k in KERNELS:
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for n, r in named if n == k]
        if not us:
            raise SystemExit(f"the trace does not hold {k}: {sorted({n for n, _ in named})[:60]}")
        out.append(f"  {k:22}{len(us):<10}{statistics.median(us):<10.2f}{min(us):<10.2f}{max(us):<10.2f}{sum(us) / 1e3:<10.3f}")
        print(out[-1], flush=True)
    out.append("")
    out += ["bench.py --gpus 1 --steps 8 --warmup 2 (the bench never streams), in the order run:"]
    ms = {n: [] for n in roots}
    for name in alternating(a.rounds):
        line = [ln for ln in child([sys.executable, "bench.py", "--gpus", "1", "--steps", "8", "--warmup", "2"], roots[name], 300).splitlines()
                if ln.startswith("{")][-1]
        ms[name].append(float(json.loads(line)["ms_per_step"]))
        out.append(f"  {name:6}{ms[name][-1]:.3f} ms per step")
        print(out[-1], flush=True)
    out.append("  " + "; ".join(f"{n}: {min(ms[n]):.3f} - {max(ms[n]):.3f} ms per step, mean {statistics.mean(ms[n]):.3f}" for n in roots))
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

    has = "sbv2_stream_begin_request_voice" in _lib.SYMBOLS
    bc, vc = O.DEBERTA_FULL, O.VITS_FULL
    bs = model.load_model(synth.pack_blob(synth.KIND_BERT, bc, synth.make_deberta_weights(bc, 0x5B72)), True)
    vs = model.load_model(synth.pack_blob(synth.KIND_VITS, vc, synth.make_vits_weights(vc, 0x5B72)), False)
    u = synth.make_utterance(2000, bc, vc, seed=991)

    def stream(fmt, q):
        kw = dict(voice=model.StreamVoice(1.2, 1.0, q, PIVOT)) if q is not None else {}
        t0 = time.perf_counter()
        st = model.StreamHandle(bs, vs, [u], 256, fmt=fmt, gaps=[0], forced=True, **kw)
        first = None
        while (c := st.next()) is not None:
            if first is None and len(c):
                first = time.perf_counter() - t0
        whole = time.perf_counter() - t0
        st.close()
        return whole * 1e3, first * 1e3

    if a.only_kernels:
        for q in SCALES:
            stream(model.PcmFormat(44100, "f32"), q)
        bs.close(); vs.close()
        return

    def timeit(fmt, q):
        stream(fmt, q)
        t = [stream(fmt, q) for _ in range(a.runs)]
        return {w: [round(float(f([x[i] for x in t])), 3) for f in (np.median, np.min, np.max)] for i, w in enumerate(("whole", "first"))}

    for r, e in FORMATS:
        fmt = model.PcmFormat(r, e)
        rec = {"format": f"{e} {r}", "runs": a.runs}
        if has:
            rec["lookahead"] = model.stream_voice_lookahead(model.StreamVoice(1.2, 1.0, 1.0, PIVOT))
        plan = [("plain_1", None)] + ([(f"voice_{q}", q) for q in SCALES] if has else []) + [("plain_2", None)]
        for key, q in plan:
            for w, v in timeit(fmt, q).items():
                rec[f"{key}_{w}"] = v
        print(json.dumps(rec), flush=True)
    bs.close(); vs.close()


if __name__ == "__main__":
    main()
