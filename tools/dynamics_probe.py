"""Compressor probe: a request fetch of the bench batch (32 x 128 phonemes at full model size, all rows on one joined timeline) through the
look-ahead limiter, without and with the speech compressor in front of it, at 16 kHz s16 and 44.1 kHz f32: the median wall time of `--iters`
fetches into pinned host memory after one warm-up.  A library without the compressor (an older commit) reports the fetch without it only, so the
same file measures both sides of a comparison.

  python tools/dynamics_probe.py [--iters 25] [--out FILE]
  python tools/dynamics_probe.py --table
      the device's L_out on the speech-like test signal (tests/test_limiter.py) at 8, 16, 44.1 and 48 kHz: limiter alone and compressor +
      limiter, through the two test hooks; the numpy column of DESIGN.md 8q is tests/test_dynamics.py's.
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python tools/dynamics_probe.py --iters 20 --only-kernels
      the compressed fetches alone, without timing, for the per-kernel table (run it as its own process)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

FORMATS = ((16000, "s16"), (44100, "f32"))
GAP = 22050   # native samples of silence between the rows (the orchestrator's sentence gap)


def table():
    from sbv2_api_amd import model
    from test_limiter import speech_like
    lim, dyn = model.Limiter(-16.0, -1.0, 6.0), model.Dynamics()
    for rate in (8000, 16000, 44100, 48000):
        y = speech_like(rate)
        _, s0 = model.debug_limiter([y], rate, lim)
        parts, ds = model.debug_dynamics([y], rate, dyn)
        _, s1 = model.debug_limiter([parts[0].y], rate, lim)
        print(json.dumps({"rate": rate, "L_out_limiter": round(float(s0[0, 3]), 2), "L_out_compressor_limiter": round(float(s1[0, 3]), 2),
                          "depth_limiter": round(float(s0[0, 5]), 1), "depth_with_compressor": round(float(s1[0, 5]), 1),
                          "deepest_compression_db": round(float(ds[0, 2]), 2), "L": round(float(ds[0, 0]), 2)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=25)
    ap.add_argument("--only-kernels", action="store_true")
    ap.add_argument("--table", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.table:
        return table()
    import sbv2_oracle as O
    from sbv2_api_amd import model, synth

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
    lim = model.Limiter(-16.0, -1.0, 6.0)
    dyn = model.Dynamics() if hasattr(model, "Dynamics") else None
    C, l = model.C, model._lib.lib()
    rw, pl = np.asarray(rows, np.int32), np.asarray(place, np.int64)
    pinned = model.PinnedArray(joined)   # pinned host memory: room for f32 at 44.1 kHz, no page faults in the timed region
    got, s6, s3 = C.c_int64(0), np.zeros(6, np.float64), np.zeros(3, np.float64)
    f64p = C.POINTER(C.c_double)

    def fetch(f, compressed):
        req = model.Sbv2FetchRequest(rw.ctypes.data_as(C.POINTER(C.c_int32)), rw.size, pl.ctypes.data_as(model.i64p), joined, C.pointer(f.c), None,
                                     C.pointer(lim.c), 0)
        tail = (pinned.array.ctypes.data, pinned.array.nbytes, C.byref(got), s6.ctypes.data_as(f64p))
        if compressed:
            model.check(l.sbv2_pipeline_fetch_request_dynamics(pipe.h, b.ticket, C.byref(req), None, None, C.byref(dyn.c), *tail,
                                                               s3.ctypes.data_as(f64p), None, None))
        else:
            model.check(l.sbv2_pipeline_fetch_request(pipe.h, b.ticket, C.byref(req), *tail))
        return s6.copy(), s3.copy()

    if a.only_kernels:
        for r, e in FORMATS:
            for _ in range(a.iters):
                fetch(model.PcmFormat(r, e), True)
        return

    def timeit(fn):
        fn()
        t = []
        for _ in range(a.iters):
            t0 = time.perf_counter()
            fn()
            t.append(time.perf_counter() - t0)
        return float(np.median(t)) * 1e3, float(np.min(t)) * 1e3, float(np.max(t)) * 1e3

    lines = []
    for r, e in FORMATS:
        f = model.PcmFormat(r, e)
        rec = {"format": f"{e} {r}", "audio_s": round(joined / 44100, 1), "iters": a.iters}
        for rep in (1, 2):   # twice, so that the record carries its own run-to-run spread
            rec[f"limiter_ms_{rep}"] = [round(v, 3) for v in timeit(lambda: fetch(f, False))]
        if dyn is not None:
            rec["compressor_limiter_ms"] = [round(v, 3) for v in timeit(lambda: fetch(f, True))]
            st, ds = fetch(f, True)
            s0, _ = fetch(f, False)
            rec["L_out_limiter"], rec["L_out_compressor_limiter"] = round(float(s0[3]), 2), round(float(st[3]), 2)
            rec["depth_limiter"], rec["depth_with_compressor"], rec["deepest_compression_db"] = round(float(s0[5]), 2), round(float(st[5]), 2), round(float(ds[2]), 2)
        lines.append(json.dumps(rec))
    print("\n".join(lines))
    if a.out:
        open(a.out, "w").write("\n".join(lines) + "\n")
    pinned.close(); pipe.close(); bs.close(); vs.close()


if __name__ == "__main__":
    main()
