"""Formant track probe: the marks fetch of the bench batch (32 x 128 phonemes at full model size, all rows on one joined timeline; token levels, a
10 ms envelope and a 10 ms pitch contour) with a formant contour of 3 formants every 10 ms, plain and tracked (6 candidates, the usual
costs), at 16 kHz s16 and 44.1 kHz f32: the median wall time of `--iters` fetches into pinned host memory after one warm-up.  The plain
fetch is timed twice, before and after the tracked one, so that the record carries its own run-to-run spread.  A library without the entry
point (an older commit) reports the plain fetch only, so the same file measures both sides of a comparison.

  python tools/formant_track_probe.py --report profiles/formant_track_probe.txt --other DIR [--rounds 2] [--iters 15]
      everything profiles/formant_track_probe.txt holds, written by this call: the fetches of this tree and of the tree at DIR (the parent
      commit, built), bench.py --gpus 1 --steps 8 --warmup 2 of both trees, and, in a traced run of its own (rocprofv3 --kernel-trace), the
      times of k_ftrack_runs and k_ftrack_path beside k_formant_lpc's of the same fetches, and k_ftrack_path on one table walked as ONE run by
      one wavefront and as runs of 100 frames side by side.  Every measurement is a fresh child process, the two trees alternate (tree,
      other, other, tree, ...), and nothing more is started after a child that failed.
  python tools/formant_track_probe.py [--root DIR] [--iters 15] [--with-only]
      one process of the fetch timings of the tree at DIR, as JSON lines; --with-only: the tracked fetches and the two tables alone (what
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
TRACKS, CANDIDATES = 3, 6
ENTRY, PLAIN = "sbv2_pipeline_fetch_request_formant_track", "sbv2_pipeline_fetch_request_formant_contour"
TABLE_FRAMES, TABLE_RUN, TABLE_REPS = 6000, 100, 5   # the table of the one-run / side-by-side comparison


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
    """({kernel: (launches, mean us)} of the fetches, (one run us, side by side us) of the tables) from one traced child; None when the tracer
    is not there or its trace holds no k_ftrack_path (the report then says so)."""
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(prof):
        return None
    with tempfile.TemporaryDirectory() as d:
        child([prof, "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "run", "--", sys.executable, me, "--iters", str(iters), "--with-only"],
              ROOT, 600)
        rows = [r for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True) for r in csv.DictReader(open(f))]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    paths, scans = ([r for r in rows if k in r["Kernel_Name"]] for k in ("k_ftrack_path", "k_ftrack_runs"))
    if len(paths) <= 2 * TABLE_REPS or len(scans) != len(paths):   # (every tracked call is one launch of each)
        return None
    tables = paths[-2 * TABLE_REPS:]   # the child's last launches: TABLE_REPS of the one run, then TABLE_REPS of the runs side by side
    first_table = int(scans[-2 * TABLE_REPS]["Start_Timestamp"])
    found = {}
    for r in rows:
        m = re.search(r"(k_ftrack_path|k_ftrack_runs|k_formant_lpc)\w*(<[^(]*>)?", r["Kernel_Name"])
        if m and int(r["Start_Timestamp"]) < first_table:   # (the fetches' launches)
            found.setdefault(m.group(0), []).append(us(r))
    return ({k: (len(v), statistics.mean(v)) for k, v in found.items()},
            (statistics.mean(us(r) for r in tables[:TABLE_REPS]), statistics.mean(us(r) for r in tables[TABLE_REPS:])))


def report(a):
    me, roots = os.path.abspath(__file__), {"tree": ROOT, "other": os.path.abspath(a.other)}
    out = ["Formant track: what k_ftrack_runs + k_ftrack_path add to a marks fetch with a formant contour, and what that fetch without tracking and",
           "bench.py cost beside the parent commit.",
           f"Written by tools/formant_track_probe.py --report --other DIR --rounds {a.rounds} --iters {a.iters} in one call on one MI355X; `tree` is",
           "this tree, `other` the parent commit built at DIR; every line of a table is one process, in the order in which they ran.",
           "",
           "Workload: the bench batch (32 x 128 phonemes, full model shapes, forced durations), all 32 rows on one joined timeline with 22050-sample",
           "gaps; a request fetch with marks (token levels, a 10 ms envelope), a 10 ms pitch contour and a formant contour of 3 formants every 10 ms",
           "at the defaults, plain (both trees) and tracked (6 candidates, references 500 / 1500 / 2500 Hz, costs 1, 1, 4).  Destination: pinned",
           f"host memory.  Median (min, max) wall time in ms of {a.iters} fetches after one warm-up; the plain fetch is measured before and after.", ""]
    recs = []
    for name in alternating(a.rounds):
        lines = [json.loads(ln) for ln in child([sys.executable, me, "--root", roots[name], "--iters", str(a.iters)], roots[name], 600).splitlines()
                 if ln.startswith("{")]
        recs.append((name, lines))
        print(name, lines, flush=True)
    out.append(f"  {'':6}{'format':12}{'frames':10}{'plain, before':26}{'plain, after':26}{'tracked':26}{'frames in runs':16}")
    for name, lines in recs:
        for rec in lines:
            with_ = cell(rec["track_ms"]) if "track_ms" in rec else "-"
            inr = f"{rec['tracked_frames']}/{rec['frames']}" if "tracked_frames" in rec else "-"
            out.append(f"  {name:6}{rec['format']:12}{rec['frames']:<10}{cell(rec['plain_ms_1']):26}{cell(rec['plain_ms_2']):26}{with_:26}{inr:16}")
    out.append("")
    for r, e in FORMATS:
        fmt = f"{e} {r}"
        med = {n: [rec[k][0] for nn, lines in recs if nn == n for rec in lines if rec["format"] == fmt for k in ("plain_ms_1", "plain_ms_2")]
               for n in roots}
        add = [rec["track_ms"][0] - 0.5 * (rec["plain_ms_1"][0] + rec["plain_ms_2"][0]) for _, lines in recs for rec in lines
               if rec["format"] == fmt and "track_ms" in rec]
        inside = min(med["other"]) <= min(med["tree"]) and max(med["tree"]) <= max(med["other"])
        out.append(f"  {fmt}: medians of the plain fetch, tree {min(med['tree']):.3f} - {max(med['tree']):.3f} ms, other {min(med['other']):.3f} - "
                   f"{max(med['other']):.3f} ms: the tree's are {'inside' if inside else 'NOT inside'} the other's range\n    the tracked fetch, above "
                   f"the mean of the same process's two plain medians: {min(add):+.3f} .. {max(add):+.3f} ms")
    out += ["", "bench.py --gpus 1 --steps 8 --warmup 2 (the bench never brings a formant contour), in the order run:"]
    ms = {n: [] for n in roots}
    for name in alternating(2 * a.rounds):
        line = [ln for ln in child([sys.executable, "bench.py", "--gpus", "1", "--steps", "8", "--warmup", "2"], roots[name], 300).splitlines()
                if ln.startswith("{")][-1]
        ms[name].append(float(json.loads(line)["ms_per_step"]))
        out.append(f"  {name:6}{ms[name][-1]:.3f} ms per step")
        print(out[-1], flush=True)
    inside = min(ms["other"]) <= min(ms["tree"]) and max(ms["tree"]) <= max(ms["other"])
    out.append("  " + "; ".join(f"{n}: {min(ms[n]):.3f} - {max(ms[n]):.3f} ms per step, mean {statistics.mean(ms[n]):.3f}" for n in roots)
               + f": the tree's runs are {'inside' if inside else 'NOT inside'} the other's range")
    out += ["", "Kernel times (a traced run of its own, rocprofv3 --kernel-trace, of the tracked fetches at both formats; the host is slower under",
            "the tracer, the kernels are not):"]
    k = traced_kernels(me, min(a.iters, 5))
    if k is None:
        out.append("  not measured: the traced run wrote no kernel trace with k_ftrack_path")
    else:
        out += [f"  {name:44}{c:5} launches, mean {us:9.1f} us" for name, (c, us) in sorted(k[0].items())]
        out += ["", f"k_ftrack_path<{TRACKS}> on one seeded table of {TABLE_FRAMES} frames with {CANDIDATES} candidates each (the hook, the stage skipped), "
                f"mean of {TABLE_REPS} launches:",
                f"  one run, walked by one wavefront:                    {k[1][0]:9.1f} us",
                f"  a cut after every {TABLE_RUN - 1} frames, {TABLE_FRAMES // TABLE_RUN} runs side by side:   {k[1][1]:9.1f} us"]
    open(a.report, "w").write("\n".join(out) + "\n")
    print(f"wrote {a.report}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=15)
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

    def fetch(f, tracked):
        out_len, hop = model.pcm_format_length(f, joined), f.sample_rate // 100
        nenv = -(-out_len // hop)
        tok = [np.zeros(ntok, np.int64), np.zeros(ntok, np.int64), np.zeros(ntok, np.float64), np.zeros(ntok, np.float64)]
        env = [np.zeros(nenv, np.float64), np.zeros(nenv, np.float64)]
        cm = _lib.Sbv2Marks(ntok, tok[0].ctypes.data_as(model.i64p), tok[1].ctypes.data_as(model.i64p), f64p(tok[2]), f64p(tok[3]), 0, hop, 0, nenv,
                            f64p(env[0]), f64p(env[1]), 0)
        cp, keep_p = model.Pitch(hop).c_struct(out_len)
        req = model.Sbv2FetchRequest(rw.ctypes.data_as(C.POINTER(C.c_int32)), rw.size, pl.ctypes.data_as(model.i64p), joined, C.pointer(f.c), None,
                                     None, 0)
        cfc, keep = model.FormantContour(hop, TRACKS).c_struct(out_len, f.sample_rate)
        args = (pipe.h, b.ticket, C.byref(req), None, None, None, None, None, pinned.array.ctypes.data, pinned.array.nbytes, C.byref(got), None, None,
                C.byref(cm), C.byref(cp), None, C.byref(cfc))
        if tracked:
            ct = model.FormantTrack((500.0, 1500.0, 2500.0), CANDIDATES).c
            model.check(getattr(l, ENTRY)(*args, C.byref(ct)))
            last["tracked_frames"] = int((keep[0][:cfc.n_frames * TRACKS].reshape(-1, TRACKS)[:, -1] > 0).sum())   # (all 3 tracks: in a run)
        else:
            model.check(getattr(l, PLAIN)(*args))
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
            rec["track_ms"] = timeit(lambda: fetch(f, True))
        else:
            rec["frames"] = fetch(f, False)
            rec["plain_ms_1"] = timeit(lambda: fetch(f, False))
            if has:
                rec["track_ms"] = timeit(lambda: fetch(f, True))
                rec["tracked_frames"] = last["tracked_frames"]
            rec["plain_ms_2"] = timeit(lambda: fetch(f, False))
        lines.append(json.dumps(rec))
    if a.with_only:   # the same table as one run and as runs side by side: the LAST launches of this process, in this order
        rng = np.random.default_rng(0)
        cf = np.sort(rng.integers(200, 5000, (TABLE_FRAMES, CANDIDATES)), axis=1).astype(np.float64)
        cb = rng.integers(20, 400, (TABLE_FRAMES, CANDIDATES)).astype(np.float64)
        cut_f, cut_b = cf.copy(), cb.copy()
        cut_f[TABLE_RUN - 1::TABLE_RUN], cut_b[TABLE_RUN - 1::TABLE_RUN] = 0.0, 0.0
        ft = model.FormantTrack((500.0, 1500.0, 2500.0), CANDIDATES)
        for tab in ((cf, cb), (cut_f, cut_b)):
            for _ in range(TABLE_REPS):
                model.debug_formant_track(None, 16000, model.FormantContour(160, TRACKS), ft, cand=tab)
    print("\n".join(lines))
    pinned.close(); pipe.close(); bs.close(); vs.close()


if __name__ == "__main__":
    main()
