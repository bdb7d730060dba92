"""Token gain probe: the request fetch of the bench batch (32 x 128 phonemes at full model size, all rows on one joined timeline) without a
token gain and with a full table (every token a target RMS, 10 ms ramps), at 16 kHz s16 and 44.1 kHz f32: the median wall time of `--iters`
fetches into pinned host memory after one warm-up.  The fetch without is timed twice, before and after the fetch with, so that the record
carries its own run-to-run spread.  The same process times a plain device-to-device copy of as many bytes as k_tgain_apply moves (4 in and 4
out per native sample), by device events: the yardstick of that kernel.  A library without the entry point (an older commit) reports the
fetch without only, so the same file measures both sides of a comparison.

  python tools/token_gain_probe.py --report profiles/token_gain_probe.txt --other DIR [--rounds 2] [--iters 25]
      everything profiles/token_gain_probe.txt holds, written by this call: the fetches of this tree and of the tree at DIR (the parent
      commit, built), the three kernels' times from a rocprofv3 kernel trace of this tree, and bench.py --gpus 1 --steps 8 --warmup 2 of both
      trees.  Every measurement is a fresh child process, the two trees alternate (tree, other, other, tree, ...), and nothing more is started
      after a child that failed.
  python tools/token_gain_probe.py [--root DIR] [--iters 25]
      one process of the fetch timings of the tree at DIR (this one without), as JSON lines.
  python tools/token_gain_probe.py --only-kernels [--iters 10]
      the f32 fetches with the table alone, for a kernel trace (k_tgain_level, k_tgain_factors, k_tgain_apply)."""
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
KERNELS = ("k_tgain_level", "k_tgain_factors", "k_tgain_apply")


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
    return f"{v[0]:.3f} ({v[1]:.3f}, {v[2]:.3f})"


def report(a):
    me, roots = os.path.abspath(__file__), {"tree": ROOT, "other": os.path.abspath(a.other)}
    out = ["Token gain: what the three kernels add to a request fetch, and what the fetch without them and bench.py cost beside the parent commit.",
           f"Written by tools/token_gain_probe.py --report --other DIR --rounds {a.rounds} --iters {a.iters} in one call on one MI355X; `tree` is this",
           "tree, `other` the parent commit built at DIR; every line of a table is one process, in the order in which they ran.",
           "",
           "Workload: the bench batch (32 x 128 phonemes, full model shapes, forced durations), all 32 rows on one joined timeline with 22050-sample",
           "gaps.  sbv2_pipeline_fetch_request, and sbv2_pipeline_fetch_request_token_gain with a full table (kind 1, every token a target RMS,",
           f"ramp 441, max_ratio 4).  Destination: pinned host memory.  Median (min, max) wall time in ms of {a.iters} fetches after one warm-up; the",
           "fetch without is measured before and after the fetch with.  copy: a device-to-device copy of 4 bytes x the batch's native samples",
           "(as many bytes read and written as k_tgain_apply moves), device events around 20 copies, in the same process.", ""]
    with tempfile.TemporaryDirectory() as d:   # the kernels under the tracer, in a process of their own and ahead of the timed ones
        child(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "run", "--", sys.executable, me, "--only-kernels", "--iters", "10"],
              ROOT, 600)
        rows = [r for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True) for r in csv.DictReader(open(f))]
    named = [(kernel_name(r["Kernel_Name"]), r) for r in rows]
    if not all(any(n == k for n, _ in named) for k in KERNELS):
        raise SystemExit(f"the trace does not hold {KERNELS}: {sorted({r['Kernel_Name'] for r in rows})[:40]}")
    recs = []
    for name in alternating(a.rounds):
        lines = [json.loads(ln) for ln in child([sys.executable, me, "--root", roots[name], "--iters", str(a.iters)], roots[name], 600).splitlines()
                 if ln.startswith("{")]
        recs.append((name, lines))
        print(name, lines, flush=True)
    out.append(f"  {'':6}{'format':12}{'without, before':26}{'without, after':26}{'with a full table':26}{'copy, ms':12}")
    for name, lines in recs:
        for rec in lines:
            with_ = cell(rec["token_gain_ms"]) if "token_gain_ms" in rec else "-"
            out.append(f"  {name:6}{rec['format']:12}{cell(rec['plain_ms_1']):26}{cell(rec['plain_ms_2']):26}{with_:26}{rec['copy_ms']:.4f}")
    out.append("")
    for r, e in FORMATS:
        fmt = f"{e} {r}"
        med = {n: [rec[k][0] for nn, lines in recs if nn == n for rec in lines if rec["format"] == fmt for k in ("plain_ms_1", "plain_ms_2")]
               for n in roots}
        add = [rec["token_gain_ms"][0] - 0.5 * (rec["plain_ms_1"][0] + rec["plain_ms_2"][0]) for _, lines in recs for rec in lines
               if rec["format"] == fmt and "token_gain_ms" in rec]
        out.append(f"  {fmt}: medians of the fetch without, tree {min(med['tree']):.3f} - {max(med['tree']):.3f} ms, other {min(med['other']):.3f} - "
                   f"{max(med['other']):.3f} ms\n    the fetch with, above the mean of the same process's two medians without: "
                   f"{min(add):+.3f} .. {max(add):+.3f} ms")
    first = recs[0][1][0]
    out += ["", f"Kernel trace of this tree (rocprofv3 --kernel-trace, a process of its own: 10 f32 fetches with the table; us).  The batch has "
            f"{first['native_samples']} native samples", f"in its rows and {first['tokens']} tokens.",
            f"  {'kernel':22}{'launches':10}{'median':10}{'min':10}{'max':10}{'workgroups x lanes, LDS bytes'}"]
    med = {}
    for k in KERNELS:
        sel = [r for n, r in named if n == k]
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in sel]
        wg = int(sel[-1]["Workgroup_Size_X"])
        med[k] = statistics.median(us)
        out.append(f"  {k:22}{len(us):<10}{med[k]:<10.2f}{min(us):<10.2f}{max(us):<10.2f}{int(sel[-1]['Grid_Size_X']) // wg} x {wg}, "
                   f"{sel[-1].get('LDS_Block_Size', '?')}")
        print(out[-1], flush=True)
    copies = [rec["copy_ms"] * 1e3 for n, lines in recs if n == "tree" for rec in lines]
    moved = 8 * first["native_samples"]
    out.append(f"  k_tgain_apply moves {moved} bytes: {moved / med['k_tgain_apply'] / 1e6:.2f} TB/s; the plain copy of the same bytes took "
               f"{min(copies):.2f} - {max(copies):.2f} us ({moved / statistics.median(copies) / 1e6:.2f} TB/s): the kernel takes "
               f"{med['k_tgain_apply'] / statistics.median(copies):.2f} x the copy")
    out += ["", "bench.py --gpus 1 --steps 8 --warmup 2 (the bench never brings a token gain), in the order run:"]
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

    has = "sbv2_pipeline_fetch_request_token_gain" in _lib.SYMBOLS
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
    table = model.TokenGain(np.full(ntok, 0.05), "rms", 441, 4.0) if has else None

    def fetch(f, with_table):
        req = model.Sbv2FetchRequest(rw.ctypes.data_as(C.POINTER(C.c_int32)), rw.size, pl.ctypes.data_as(model.i64p), joined, C.pointer(f.c), None,
                                     None, 0)
        tail = (pinned.array.ctypes.data, pinned.array.nbytes, C.byref(got), None)
        if with_table:
            ctg, _keep = table.c_struct()
            model.check(l.sbv2_pipeline_fetch_request_token_gain(pipe.h, b.ticket, C.byref(req), None, None, None, None, None, *tail, None, None,
                                                                 None, None, None, None, C.byref(ctg)))
        else:
            model.check(l.sbv2_pipeline_fetch_request(pipe.h, b.ticket, C.byref(req), *tail))

    if a.only_kernels:
        for _ in range(a.iters):
            fetch(model.PcmFormat(44100, "f32"), True)
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
        rec = {"format": f"{e} {r}", "audio_s": round(joined / 44100, 1), "iters": a.iters, "native_samples": native, "tokens": ntok}
        rec["plain_ms_1"] = timeit(lambda: fetch(f, False))
        if has:
            rec["token_gain_ms"] = timeit(lambda: fetch(f, True))
        rec["plain_ms_2"] = timeit(lambda: fetch(f, False))
        rec["copy_ms"] = round(copy_ms(native), 5)
        lines.append(json.dumps(rec))
    print("\n".join(lines))
    pinned.close(); pipe.close(); bs.close(); vs.close()


if __name__ == "__main__":
    main()
