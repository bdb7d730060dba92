"""Formant contour probe: the marks fetch of the bench batch (32 x 128 phonemes at full model size, all rows on one joined timeline; token levels, a
10 ms envelope and a 10 ms pitch contour) without a formant contour and with one (4 formants, the defaults: 25 ms windows, order 2 + rate //
1000, every 10 ms), at 16 kHz s16 and 44.1 kHz f32: the median wall time of `--iters` fetches into pinned host memory after one warm-up, and
the share of frames whose root iteration hit its cap.  The fetch without is timed twice, before and after the fetch with, so that the record
carries its own run-to-run spread.  A library without the entry point (an older commit) reports the fetch without it only, so the same file
measures both sides of a comparison.

  python tools/formant_contour_probe.py --report profiles/formant_contour_probe.txt --other DIR [--rounds 2] [--iters 25]
      everything profiles/formant_contour_probe.txt holds, written by this call: the fetches of this tree and of the tree at DIR (the parent
      commit, built), bench.py --gpus 1 --steps 8 --warmup 2 of both trees, and, in a traced run of its own (rocprofv3 --kernel-trace),
      the time of k_formant_lpc beside k_pitch_yin's of the same fetches.  Every measurement is a fresh child process, the two trees
      alternate (tree, other, other, tree, ...), and nothing more is started after a child that failed.
  python tools/formant_contour_probe.py [--root DIR] [--iters 25] [--with-only]
      one process of the fetch timings of the tree at DIR (this one without), as JSON lines; --with-only: the fetches with a contour alone (what
      the traced run executes)."""
import argparse
import csv
import glob
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMATS = ((16000, "s16"), (44100, "f32"))
GAP = 22050   # native samples of silence between the rows (the orchestrator's sentence gap)
N_FORMANTS = 4
ENTRY = "sbv2_pipeline_fetch_request_formant_contour"


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


def cell(v):
    return f"{v[0]:.3f} ({v[1]:.3f}, {v[2]:.3f})"


def traced_kernels(me, iters):
    """{kernel: (launches, mean us)} of k_formant_lpc and k_pitch_yin from one traced child that runs the fetches with a contour; None when the
    tracer is not there or its trace holds neither (the report then says so)."""
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(prof):
        return None
    with tempfile.TemporaryDirectory() as d:
        child([prof, "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "run", "--", sys.executable, me, "--iters", str(iters), "--with-only"],
              ROOT, 600)
        rows = [r for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True) for r in csv.DictReader(open(f))]
    found = {}   # by instantiation: <short, 4> is the 16 kHz s16 fetch, <float, 1> the 44.1 kHz f32 one
    for r in rows:
        m = re.search(r"(k_formant_lpc|k_pitch_yin)\w*(<[^(]*>)?", r["Kernel_Name"])
        if m:
            found.setdefault(m.group(0), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    return {k: (len(v), statistics.mean(v)) for k, v in found.items()} or None


def report(a):
    me, roots = os.path.abspath(__file__), {"tree": ROOT, "other": os.path.abspath(a.other)}
    out = ["Formant contour: what k_formant_lpc adds to a marks fetch, and what the fetch without it and bench.py cost beside the parent commit.",
           f"Written by tools/formant_contour_probe.py --report --other DIR --rounds {a.rounds} --iters {a.iters} in one call on one MI355X; `tree` is",
           "this tree, `other` the parent commit built at DIR; every line of a table is one process, in the order in which they ran.",
           "",
           "Workload: the bench batch (32 x 128 phonemes, full model shapes, forced durations), all 32 rows on one joined timeline with 22050-sample",
           "gaps; a request fetch with marks (token levels, a 10 ms envelope) and a 10 ms pitch contour, without a formant contour and with 4",
           "formants at the defaults (25 ms windows, order 18 at 16 kHz and 46 at 44.1 kHz) every 10 ms.  Destination: pinned host memory.  Median",
           f"(min, max) wall time in ms of {a.iters} fetches after one warm-up; the fetch without is measured before and after the fetch with.", ""]
    recs = []
    for name in alternating(a.rounds):
        lines = [json.loads(ln) for ln in child([sys.executable, me, "--root", roots[name], "--iters", str(a.iters)], roots[name], 600).splitlines()
                 if ln.startswith("{")]
        recs.append((name, lines))
        print(name, lines, flush=True)
    out.append(f"  {'':6}{'format':12}{'frames':10}{'without, before':26}{'without, after':26}{'with 4 formants':26}{'cap hit':10}")
    for name, lines in recs:
        for rec in lines:
            with_ = cell(rec["contour_ms"]) if "contour_ms" in rec else "-"
            cap = f"{rec['cap_hit']}/{rec['frames']}" if "cap_hit" in rec else "-"
            out.append(f"  {name:6}{rec['format']:12}{rec['frames']:<10}{cell(rec['marks_ms_1']):26}{cell(rec['marks_ms_2']):26}{with_:26}{cap:10}")
    out.append("")
    for r, e in FORMATS:
        fmt = f"{e} {r}"
        med = {n: [rec[k][0] for nn, lines in recs if nn == n for rec in lines if rec["format"] == fmt for k in ("marks_ms_1", "marks_ms_2")]
               for n in roots}
        add = [rec["contour_ms"][0] - 0.5 * (rec["marks_ms_1"][0] + rec["marks_ms_2"][0]) for _, lines in recs for rec in lines
               if rec["format"] == fmt and "contour_ms" in rec]
        out.append(f"  {fmt}: medians of the fetch without, tree {min(med['tree']):.3f} - {max(med['tree']):.3f} ms, other {min(med['other']):.3f} - "
                   f"{max(med['other']):.3f} ms\n    the fetch with, above the mean of the same process's two medians without: "
                   f"{min(add):+.3f} .. {max(add):+.3f} ms")
    out += ["", "bench.py --gpus 1 --steps 8 --warmup 2 (the bench never brings a formant contour), in the order run:"]
    ms = {n: [] for n in roots}
    for name in alternating(2 * a.rounds):
        line = [ln for ln in child([sys.executable, "bench.py", "--gpus", "1", "--steps", "8", "--warmup", "2"], roots[name], 300).splitlines()
                if ln.startswith("{")][-1]
        ms[name].append(float(json.loads(line)["ms_per_step"]))
        out.append(f"  {name:6}{ms[name][-1]:.3f} ms per step")
        print(out[-1], flush=True)
    out.append("  " + "; ".join(f"{n}: {min(ms[n]):.3f} - {max(ms[n]):.3f} ms per step, mean {statistics.mean(ms[n]):.3f}" for n in roots))
    out += ["", "Kernel times (a traced run of its own, rocprofv3 --kernel-trace, of the fetches with a contour at both formats; the host is",
            "slower under the tracer, the kernels are not):"]
    k = traced_kernels(me, min(a.iters, 5))
    if k is None:
        out.append("  not measured: the traced run wrote no kernel trace")
    else:
        out += [f"  {name:44}{c:5} launches, mean {us:9.1f} us" for name, (c, us) in sorted(k.items())]
    open(a.report, "w").write("\n".join(out) + "\n")
    print(f"wrote {a.report}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=25)
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--report")
    ap.add_argument("--other")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--with-only", action="store_true")
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

    has = ENTRY in _lib.SYMBOLS
    if a.with_only and not has:
        raise SystemExit(f"--with-only needs a library with {ENTRY}")
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
    ntok = int(sum(int(v) for v in b.t_lens))
    f64p = lambda x: x.ctypes.data_as(C.POINTER(C.c_double))
    last = {}

    def fetch(f, with_contour):
        out_len, hop = model.pcm_format_length(f, joined), f.sample_rate // 100
        nenv = -(-out_len // hop)
        tok = [np.zeros(ntok, np.int64), np.zeros(ntok, np.int64), np.zeros(ntok, np.float64), np.zeros(ntok, np.float64)]
        env = [np.zeros(nenv, np.float64), np.zeros(nenv, np.float64)]
        cm = _lib.Sbv2Marks(ntok, tok[0].ctypes.data_as(model.i64p), tok[1].ctypes.data_as(model.i64p), f64p(tok[2]), f64p(tok[3]), 0, hop, 0, nenv,
                            f64p(env[0]), f64p(env[1]), 0)
        cp, keep_p = model.Pitch(hop).c_struct(out_len)
        req = model.Sbv2FetchRequest(rw.ctypes.data_as(C.POINTER(C.c_int32)), rw.size, pl.ctypes.data_as(model.i64p), joined, C.pointer(f.c), None,
                                     None, 0)
        args = (pipe.h, b.ticket, C.byref(req), None, None, None, None, None, pinned.array.ctypes.data, pinned.array.nbytes, C.byref(got), None, None,
                C.byref(cm), C.byref(cp))
        if with_contour:
            cfc, keep = model.FormantContour(hop, N_FORMANTS).c_struct(out_len, f.sample_rate)
            model.check(getattr(l, ENTRY)(*args, None, C.byref(cfc)))
            last["cap_hit"] = int((keep[2][:cfc.n_frames] & 1).sum())
        else:
            model.check(l.sbv2_pipeline_fetch_request_formant(*args))
        return nenv

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
        if a.with_only:
            rec["contour_ms"] = timeit(lambda: fetch(f, True))
        else:
            rec["frames"] = fetch(f, False)
            rec["marks_ms_1"] = timeit(lambda: fetch(f, False))
            if has:
                rec["contour_ms"] = timeit(lambda: fetch(f, True))
                rec["cap_hit"] = last["cap_hit"]
            rec["marks_ms_2"] = timeit(lambda: fetch(f, False))
        lines.append(json.dumps(rec))
    print("\n".join(lines))
    pinned.close(); pipe.close(); bs.close(); vs.close()


if __name__ == "__main__":
    main()
