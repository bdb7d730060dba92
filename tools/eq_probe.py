"""EQ probe: the request fetch of the bench batch (32 x 128 phonemes at full model size, all rows on one joined timeline) without an EQ and with
one of 1, 2, 4 and 8 bands, at 16 kHz s16 and 44.1 kHz f32: the median wall time of `--iters` fetches into pinned host memory after one
warm-up.  The fetch without is timed twice, before and after the fetches with, so that the record carries its own run-to-run spread.  The
same process times a plain device-to-device copy of as many bytes as k_eq_apply moves (4 in and 4 out per native sample), by device events:
the yardstick of that kernel.  A library without the entry point (an older commit) reports the fetch without only, so the same file measures
both sides of a comparison.

  python tools/eq_probe.py --report profiles/eq_probe.txt --other DIR [--rounds 2] [--iters 25] [--ratios FILE]
      everything profiles/eq_probe.txt holds, written by this call: the fetches of this tree and of the tree at DIR (the parent commit, built),
      the kernels' times from a rocprofv3 kernel trace of this tree, and bench.py --gpus 1 --steps 8 --warmup 2 of both trees.  Every
      measurement is a fresh child process, the two trees alternate (tree, other, other, tree, ...), and nothing more is started after a child
      that failed.  FILE: the output of pytest tests/test_eq.py -m gpu -s, whose "eq ..." lines (the accuracy ratios) are copied in.
  python tools/eq_probe.py [--root DIR] [--iters 25]
      one process of the fetch timings of the tree at DIR (this one without), as JSON lines.
  python tools/eq_probe.py --only-kernels [--iters 10]
      the f32 fetches with each table, and with a token gain, alone, for a kernel trace."""
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
GAP = 22050   # native samples of silence between the rows (the orchestrator's sentence gap)
ALL8 = [("highpass", 20, 0, 0.7071), ("lowshelf", 120, 6, 0.7071), ("peak", 300, -4, 1.0), ("peak", 1000, 3, 1.4), ("peak", 3000, 5, 2.0),
        ("peak", 6500, -9, 4.0), ("highshelf", 9000, 4, 0.7071), ("lowpass", 16000, 0, 0.7071)]
COUNTS = (1, 2, 4, 8)   # the first S bands of ALL8


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
    """k_eq_apply<8> from the traced name (the template argument is the band count)."""
    s = traced.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0].split("::")[-1].split(".")[0].strip()
    return s.replace("<(int)", "<")


def cell(v):
    return f"{v[0]:.3f} ({v[1]:.3f}, {v[2]:.3f})"


def report(a):
    me, roots = os.path.abspath(__file__), {"tree": ROOT, "other": os.path.abspath(a.other)}
    out = ["Parametric EQ: what the three kernels add to a request fetch, and what the fetch without them and bench.py cost beside the parent commit.",
           f"Written by tools/eq_probe.py --report --other DIR --rounds {a.rounds} --iters {a.iters} in one call on one MI355X; `tree` is this tree,",
           "`other` the parent commit built at DIR; every line of a table is one process, in the order in which they ran.",
           "",
           "Workload: the bench batch (32 x 128 phonemes, full model shapes, forced durations), all 32 rows on one joined timeline with 22050-sample",
           "gaps.  sbv2_pipeline_fetch_request, and sbv2_pipeline_fetch_request_eq with the first 1, 2, 4 and 8 bands of: high-pass 20, low shelf",
           "120 +6, peaks 300 -4, 1000 +3, 3000 +5 and 6500 -9, high shelf 9000 +4, low-pass 16000.  Destination: pinned host memory.  Median",
           f"(min, max) wall time in ms of {a.iters} fetches after one warm-up; the fetch without is measured before and after the fetches with.",
           "copy: a device-to-device copy of 4 bytes x the batch's native samples (as many bytes read and written as k_eq_apply moves), device",
           "events around 20 copies, in the same process.", ""]
    with tempfile.TemporaryDirectory() as d:   # the kernels under the tracer, in a process of their own and ahead of the timed ones
        child(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "run", "--", sys.executable, me, "--only-kernels",
               "--iters", "10"], ROOT, 600)
        rows = [r for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True) for r in csv.DictReader(open(f))]
    named = [(kernel_name(r["Kernel_Name"]), r) for r in rows]
    recs = []
    for name in alternating(a.rounds):
        lines = [json.loads(ln) for ln in child([sys.executable, me, "--root", roots[name], "--iters", str(a.iters)], roots[name], 600).splitlines()
                 if ln.startswith("{")]
        recs.append((name, lines))
        print(name, lines, flush=True)
    out.append(f"  {'':6}{'format':12}{'without, before':24}{'without, after':24}" + "".join(f"{f'{s} band(s)':24}" for s in COUNTS) + "copy, ms")
    for name, lines in recs:
        for rec in lines:
            with_ = "".join(f"{cell(rec['eq_ms'][str(s)]) if 'eq_ms' in rec else '-':24}" for s in COUNTS)
            out.append(f"  {name:6}{rec['format']:12}{cell(rec['plain_ms_1']):24}{cell(rec['plain_ms_2']):24}{with_}{rec['copy_ms']:.4f}")
    out.append("")
    for r, e in FORMATS:
        fmt = f"{e} {r}"
        med = {n: [rec[k][0] for nn, lines in recs if nn == n for rec in lines if rec["format"] == fmt for k in ("plain_ms_1", "plain_ms_2")]
               for n in roots}
        out.append(f"  {fmt}: medians of the fetch without, tree {min(med['tree']):.3f} - {max(med['tree']):.3f} ms, other {min(med['other']):.3f} - "
                   f"{max(med['other']):.3f} ms")
        for s in COUNTS:
            add = [rec["eq_ms"][str(s)][0] - 0.5 * (rec["plain_ms_1"][0] + rec["plain_ms_2"][0]) for _, lines in recs for rec in lines
                   if rec["format"] == fmt and "eq_ms" in rec]
            out.append(f"    {s} band(s), above the mean of the same process's two medians without: {min(add):+.3f} .. {max(add):+.3f} ms")
    first = recs[0][1][0]
    out += ["", f"Kernel trace of this tree (rocprofv3 --kernel-trace --stats, a process of its own, no counters: 10 f32 fetches per table, and 10 with a",
            f"token gain for k_tgain_apply; us).  The batch has {first['native_samples']} native samples in its rows.  Tile: 256 lanes x L = 64 samples; L = 32",
            "and L = 128: not traced.",
            f"  {'kernel':22}{'launches':10}{'median':10}{'min':10}{'max':10}{'workgroups x lanes, LDS bytes'}"]
    med = {}
    for k in sorted({n for n, _ in named if n.startswith("k_eq_") or n == "k_tgain_apply"}):
        sel = [r for n, r in named if n == k]
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in sel]
        wg = int(sel[-1]["Workgroup_Size_X"])
        med[k] = statistics.median(us)
        out.append(f"  {k:22}{len(us):<10}{med[k]:<10.2f}{min(us):<10.2f}{max(us):<10.2f}{int(sel[-1]['Grid_Size_X']) // wg} x {wg}, "
                   f"{sel[-1].get('LDS_Block_Size', '?')}")
        print(out[-1], flush=True)
    copies = [rec["copy_ms"] * 1e3 for n, lines in recs if n == "tree" for rec in lines]
    moved, cp = 8 * first["native_samples"], statistics.median(copies)
    out.append(f"  the kernels move {moved} bytes; the plain copy of the same bytes took {min(copies):.2f} - {max(copies):.2f} us "
               f"({moved / cp / 1e6:.2f} TB/s)")
    for s in COUNTS:
        k = f"k_eq_apply<{s}>"
        if k in med:
            flops = 2 * 5 * s * 2 * first["native_samples"]   # two passes of 5 fma per section and sample
            out.append(f"  {k}: {moved / med[k] / 1e6:.2f} TB/s, {med[k] / cp:.2f} x the copy, {flops / med[k] / 1e6:.2f} TFLOP/s f64 in the lanes' "
                       "two passes (the scan not counted)")
        else:
            out.append(f"  {k}: not measured")
    if "k_tgain_apply" in med:
        out.append(f"  k_tgain_apply: {moved / med['k_tgain_apply'] / 1e6:.2f} TB/s, {med['k_tgain_apply'] / cp:.2f} x the copy")
    if a.ratios and os.path.exists(a.ratios):
        out += ["", "Accuracy (tests/test_eq.py -m gpu -s on the same machine type): max |y64 - ref| of the device, of the sample-by-sample numpy f64",
                "cascade, and their ratio, ref = the cascade in numpy longdouble; per band set and signal, over all the test's row lengths."]
        out += ["  " + ln.strip().lstrip(".F") for ln in open(a.ratios) if ln.lstrip(".F").startswith("eq ")]
    else:
        out += ["", "Accuracy ratios: not measured in this call."]
    out += ["", "bench.py --gpus 1 --steps 8 --warmup 2 (the bench never brings an EQ), in the order run:"]
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
    ap.add_argument("--ratios")
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

    has = "sbv2_pipeline_fetch_request_eq" in _lib.SYMBOLS
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
    ntok = int(sum(int(b.t_lens[r]) for r in rows))
    tables = {s: model.Eq(ALL8[:s]).c_struct() for s in COUNTS} if has else {}

    def fetch(f, s=0, token_gain=None):
        req = model.Sbv2FetchRequest(rw.ctypes.data_as(C.POINTER(C.c_int32)), rw.size, pl.ctypes.data_as(model.i64p), joined, C.pointer(f.c), None,
                                     None, 0)
        tail = (pinned.array.ctypes.data, pinned.array.nbytes, C.byref(got), None)
        if s or token_gain is not None:
            ctg, _keep = token_gain.c_struct() if token_gain is not None else (None, None)
            model.check(l.sbv2_pipeline_fetch_request_eq(pipe.h, b.ticket, C.byref(req), None, None, None, None, None, *tail, None, None, None, None,
                                                         None, None, C.byref(ctg) if ctg is not None else None, C.byref(tables[s]) if s else None))
        else:
            model.check(l.sbv2_pipeline_fetch_request(pipe.h, b.ticket, C.byref(req), *tail))

    if a.only_kernels:
        f = model.PcmFormat(44100, "f32")
        for s in COUNTS:
            for _ in range(a.iters):
                fetch(f, s)
        for _ in range(a.iters):
            fetch(f, 0, model.TokenGain(np.full(ntok, 0.05), "rms", 441, 4.0))
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

    def copy_ms(n):
        """A device-to-device copy of n floats, ms per copy: device events around 20 copies after 3 warm-ups."""
        path = next(ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln)   # the HIP runtime the library runs on
        hip = C.CDLL(path)

        def ok(rc):
            if rc != 0:
                raise SystemExit(f"HIP error {rc} in the copy yardstick")

        x, y, e0, e1, ms = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_float()
        size = C.c_size_t(4 * n)
        ok(hip.hipMalloc(C.byref(x), size)), ok(hip.hipMalloc(C.byref(y), size)), ok(hip.hipMemset(x, 0, size))
        ok(hip.hipEventCreate(C.byref(e0))), ok(hip.hipEventCreate(C.byref(e1)))
        copy = lambda: ok(hip.hipMemcpyAsync(y, x, size, 3, None))   # 3 = hipMemcpyDeviceToDevice
        for _ in range(3):
            copy()
        ok(hip.hipEventRecord(e0, None))
        for _ in range(20):
            copy()
        ok(hip.hipEventRecord(e1, None)), ok(hip.hipEventSynchronize(e1)), ok(hip.hipEventElapsedTime(C.byref(ms), e0, e1))
        ok(hip.hipEventDestroy(e0)), ok(hip.hipEventDestroy(e1)), ok(hip.hipFree(x)), ok(hip.hipFree(y))
        return ms.value / 20

    native = int(sum(int(b.lens[r]) for r in rows))
    lines = []
    for r, e in FORMATS:
        f = model.PcmFormat(r, e)
        rec = {"format": f"{e} {r}", "audio_s": round(joined / 44100, 1), "iters": a.iters, "native_samples": native}
        rec["plain_ms_1"] = timeit(lambda: fetch(f))
        if has:
            rec["eq_ms"] = {str(s): timeit(lambda: fetch(f, s)) for s in COUNTS}
        rec["plain_ms_2"] = timeit(lambda: fetch(f))
        rec["copy_ms"] = round(copy_ms(native), 5)
        lines.append(json.dumps(rec))
    print("\n".join(lines))
    pinned.close(); pipe.close(); bs.close(); vs.close()


if __name__ == "__main__":
    main()
