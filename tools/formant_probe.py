"""Formant probe: a Voice(1.2, 1.0) request fetch of the bench batch (32 x 128 phonemes at full model size, all rows on one joined timeline)
without a formant scale and with formant_scale 0.8 and 1.25, at 16 kHz s16 and 44.1 kHz f32: the median wall time of `--iters` fetches into
pinned host memory after one warm-up.  The fetch without is timed twice, before and after the fetches with, so that the record carries its
own run-to-run spread.  A library without the formant entry point (an older commit) reports the fetch without it only, so the same file
measures both sides of a comparison.

  python tools/formant_probe.py --report profiles/formant_probe.txt --other DIR [--rounds 2] [--iters 25]
      everything profiles/formant_probe.txt holds, written by this call: the fetches of this tree and of the tree at DIR (the parent commit,
      built), the two gather kernels' times from a rocprofv3 kernel trace of this tree, and bench.py --gpus 1 --steps 8 --warmup 2 of both
      trees.  Every measurement is a fresh child process, the two trees alternate (tree, other, other, tree, ...), and nothing more is started
      after a child that failed.
  python tools/formant_probe.py [--root DIR] [--iters 25]
      one process of the fetch timings of the tree at DIR (this one without), as JSON lines.
  python tools/formant_probe.py --only-kernels [--iters 10]
      the f32 fetches without and with formant_scale 0.8 alone, for a kernel trace (k_voice_gather, k_voice_gather_fmt)."""
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
SCALES = (0.8, 1.25)
GAP = 22050   # native samples of silence between the rows (the orchestrator's sentence gap)
KERNELS = ("k_pitch_yin", "k_voice_marks", "k_voice_gather", "k_voice_gather_fmt")


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
    """k_voice_gather of "sbv2::(anonymous namespace)::k_voice_gather(sbv2::(anonymous namespace)::VoiceGatherArgs) [clone .kd]" and its like."""
    return traced.replace("(anonymous namespace)::", "").split("(")[0].split("<")[0].split("::")[-1].split(".")[0].split()[-1].strip()


def cell(v):
    return f"{v[0]:.3f} ({v[1]:.3f}, {v[2]:.3f})"


def report(a):
    me, roots = os.path.abspath(__file__), {"tree": ROOT, "other": os.path.abspath(a.other)}
    out = ["Formant scale: what k_voice_gather_fmt adds to a shifted request fetch, and what the fetch without it and bench.py cost beside the parent",
           f"commit.  Written by tools/formant_probe.py --report --other DIR --rounds {a.rounds} --iters {a.iters} in one call on one MI355X; `tree` is this",
           "tree, `other` the parent commit built at DIR; every line of a table is one process, in the order in which they ran.",
           "",
           "Workload: the bench batch (32 x 128 phonemes, full model shapes, forced durations), all 32 rows on one joined timeline with 22050-sample",
           "gaps.  sbv2_pipeline_fetch_request_voice with Voice(1.2, 1.0), and sbv2_pipeline_fetch_request_formant with the same voice and",
           f"formant_scale 0.8 / 1.25.  Destination: pinned host memory.  Median (min, max) wall time in ms of {a.iters} fetches after one warm-up; the",
           "fetch without is measured before and after the fetches with.", ""]
    # the kernels under the tracer, in a process of their own and ahead of the timed ones
    with tempfile.TemporaryDirectory() as d:
        child(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "run", "--", sys.executable, me, "--only-kernels", "--iters", "10"],
              ROOT, 600)
        rows = [r for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True) for r in csv.DictReader(open(f))]
    named = [(kernel_name(r["Kernel_Name"]), r) for r in rows]
    if not all(any(n == k for n, _ in named) for k in KERNELS):
        raise SystemExit(f"the trace does not hold {KERNELS}: {sorted({r['Kernel_Name'] for r in rows})[:40]}")
    # 1. the fetches
    recs = []
    for name in alternating(a.rounds):
        lines = [json.loads(ln) for ln in child([sys.executable, me, "--root", roots[name], "--iters", str(a.iters)], roots[name], 600).splitlines()
                 if ln.startswith("{")]
        recs.append((name, lines))
        print(name, lines, flush=True)
    out.append(f"  {'':6}{'format':12}{'without, before':26}{'without, after':26}{'q = 0.8':26}{'q = 1.25':26}")
    for name, lines in recs:
        for rec in lines:
            with_ = [cell(rec[f"voice_formant_{q}_ms"]) if f"voice_formant_{q}_ms" in rec else "-" for q in SCALES]
            out.append(f"  {name:6}{rec['format']:12}{cell(rec['voice_ms_1']):26}{cell(rec['voice_ms_2']):26}{with_[0]:26}{with_[1]:26}")
    out.append("")
    for r, e in FORMATS:
        fmt = f"{e} {r}"
        med = {n: [rec[k][0] for nn, lines in recs if nn == n for rec in lines if rec["format"] == fmt for k in ("voice_ms_1", "voice_ms_2")]
               for n in roots}
        add = {q: [rec[f"voice_formant_{q}_ms"][0] - 0.5 * (rec["voice_ms_1"][0] + rec["voice_ms_2"][0]) for _, lines in recs for rec in lines
                   if rec["format"] == fmt and f"voice_formant_{q}_ms" in rec] for q in SCALES}
        out.append(f"  {fmt}: medians of the fetch without, tree {min(med['tree']):.3f} - {max(med['tree']):.3f} ms, other {min(med['other']):.3f} - "
                   f"{max(med['other']):.3f} ms\n    the fetch with, above the mean of the same process's two medians without: " +
                   ", ".join(f"q = {q} {min(add[q]):+.3f} .. {max(add[q]):+.3f} ms" for q in SCALES))
    out.append("")
    # 2. the kernels
    out += ["Kernel trace of this tree (rocprofv3 --kernel-trace, a process of its own: 10 f32 fetches without and 10 with formant_scale 0.8,",
            "alternating; us)", f"  {'kernel':22}{'launches':10}{'median':10}{'min':10}{'max':10}{'workgroups x lanes, LDS bytes'}"]
    med = {}
    for k in KERNELS:
        sel = [r for n, r in named if n == k]
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in sel]
        wg = int(sel[-1]["Workgroup_Size_X"])
        grid = " x ".join(str(int(sel[-1][f"Grid_Size_{ax}"]) // max(int(sel[-1][f"Workgroup_Size_{ax}"]), 1)) for ax in "XY")
        med[k] = statistics.median(us)
        out.append(f"  {k:22}{len(us):<10}{med[k]:<10.2f}{min(us):<10.2f}{max(us):<10.2f}{grid} x {wg}, {sel[-1].get('LDS_Block_Size', '?')}")
        print(out[-1], flush=True)
    out.append(f"  k_voice_gather_fmt / k_voice_gather at q = 0.8: {med['k_voice_gather_fmt'] / med['k_voice_gather']:.2f} "
               f"({med['k_voice_gather_fmt'] - med['k_voice_gather']:+.1f} us)")
    out.append("")
    # 3. the flagship benchmark, which never brings a formant scale
    out += ["bench.py --gpus 1 --steps 8 --warmup 2 (the bench never brings a formant scale), in the order run:"]
    ms = {n: [] for n in roots}
    for name in alternating(2 * a.rounds):
        line = [ln for ln in child([sys.executable, "bench.py", "--gpus", "1", "--steps", "8", "--warmup", "2"], roots[name], 300).splitlines()
                if ln.startswith("{")][-1]
        ms[name].append(float(json.loads(line)["ms_per_step"]))
        out.append(f"  {name:6}{ms[name][-1]:.3f} ms per step")
        print(out[-1], flush=True)
    out.append("  " + "; ".join(f"{n}: {min(ms[n]):.3f} - {max(ms[n]):.3f} ms per step, mean {statistics.mean(ms[n]):.3f}" for n in roots))
    open(a.report, "w").write("\n".join(out) + "\n")
    print(f"wrote {a.report}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=25)
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

    has = "sbv2_pipeline_fetch_request_formant" in _lib.SYMBOLS
    bc, vc = O.DEBERTA_FULL, O.VITS_FULL
    bs = model.load_model(synth.pack_blob(synth.KIND_BERT, bc, synth.make_deberta_weights(bc, 1)), True)
    vs = model.load_model(synth.pack_blob(synth.KIND_VITS, vc, synth.make_vits_weights(vc, 2)), False)
    pipe = model.Pipeline(bs, vs)
    utts = [synth.make_utterance(128, bc, vc, seed=i) for i in range(32)]
    b = pipe.prepare(utts, forced=True)
    pipe.run(b)
    pipe.sync()
    rows = list(range(len(utts)))
    place = [int(v) for v in np.concatenate([[0], np.cumsum(b.lens[:-1] + GAP)])]
    joined = place[-1] + int(b.lens[-1])
    C, l = model.C, model._lib.lib()
    rw, pl = np.asarray(rows, np.int32), np.asarray(place, np.int64)
    pinned = model.PinnedArray(joined)   # pinned host memory: room for f32 at 44.1 kHz, no page faults in the timed region
    got = C.c_int64(0)
    voice = model.Voice(1.2, 1.0)

    def fetch(f, q):
        req = model.Sbv2FetchRequest(rw.ctypes.data_as(C.POINTER(C.c_int32)), rw.size, pl.ctypes.data_as(model.i64p), joined, C.pointer(f.c), None,
                                     None, 0)
        tail = (pinned.array.ctypes.data, pinned.array.nbytes, C.byref(got), None)
        cv = voice.c
        if q is not None:
            cf = _lib.Sbv2Formant(q, 0.0)
            model.check(l.sbv2_pipeline_fetch_request_formant(pipe.h, b.ticket, C.byref(req), C.byref(cv), None, None, None, C.byref(cf), *tail, None,
                                                              None, None))
        else:
            model.check(l.sbv2_pipeline_fetch_request_voice(pipe.h, b.ticket, C.byref(req), C.byref(cv), *tail, None, None))

    if a.only_kernels:
        f = model.PcmFormat(44100, "f32")
        for _ in range(a.iters):
            fetch(f, None)
            if has:
                fetch(f, 0.8)
        pinned.close(); pipe.close(); bs.close(); vs.close()
        return

    def timeit(fn):
        fn()
        t = []
        for _ in range(a.iters):
            t0 = time.perf_counter()
            fn()
            t.append(time.perf_counter() - t0)
        return [round(float(v) * 1e3, 3) for v in (np.median(t), np.min(t), np.max(t))]

    lines = []
    for r, e in FORMATS:
        f = model.PcmFormat(r, e)
        rec = {"format": f"{e} {r}", "audio_s": round(joined / 44100, 1), "iters": a.iters}
        rec["voice_ms_1"] = timeit(lambda: fetch(f, None))
        if has:
            for q in SCALES:
                rec[f"voice_formant_{q}_ms"] = timeit(lambda: fetch(f, q))
        rec["voice_ms_2"] = timeit(lambda: fetch(f, None))
        lines.append(json.dumps(rec))
    print("\n".join(lines))
    pinned.close(); pipe.close(); bs.close(); vs.close()


if __name__ == "__main__":
    main()
