"""Pitch probe: what a 100 Hz pitch contour adds to a marks fetch on the bench batch (32 x 128 phonemes at full model size, all rows on one
joined timeline) at 16 kHz s16 and 44.1 kHz f32: the median wall time of `--iters` fetches into pinned memory with token marks and a 100 Hz
envelope (the code path of sbv2_pipeline_fetch_request_marks, which must stay what it was) and of the same fetches with a contour of
sample_rate // 100 samples per frame, 70 - 600 Hz (sbv2_pipeline_fetch_request_pitch).

  python tools/pitch_probe.py [--iters 20] [--out FILE]
  rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/pitch_probe.py --iters 20 --only-kernels pitch
      the fetches with a contour alone, for the per-kernel table (its own process); --only-kernels marks: the fetches without, whose trace
      must show no k_pitch_yin launch."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--only-kernels", choices=["marks", "pitch"])
    ap.add_argument("--out")
    a = ap.parse_args()
    import sbv2_oracle as O
    from sbv2_api_amd import _lib, model, orchestrator, synth

    bc, vc = O.DEBERTA_FULL, O.VITS_FULL
    bs = model.load_model(synth.pack_blob(synth.KIND_BERT, bc, synth.make_deberta_weights(bc, 1)), True)
    vs = model.load_model(synth.pack_blob(synth.KIND_VITS, vc, synth.make_vits_weights(vc, 2)), False)
    pipe = model.Pipeline(bs, vs)
    utts = [synth.make_utterance(128, bc, vc, seed=i) for i in range(32)]
    b = pipe.prepare(utts, forced=True)
    pipe.run(b)
    pipe.sync()
    place, joined = orchestrator.joined_placement(b.lens, list(range(32)), 32)
    rows, pl = np.arange(32, dtype=np.int32), np.asarray(place, np.int64)
    pinned = model.PinnedArray(joined)
    l = _lib.lib()
    ntok = int(b.t_lens.sum())
    f64p = C.POINTER(C.c_double)
    got = C.c_int64()

    def fetch(f, with_pitch):
        req = _lib.Sbv2FetchRequest(rows.ctypes.data_as(C.POINTER(C.c_int32)), 32, pl.ctypes.data_as(_lib.i64p), joined, C.pointer(f.c), None, None, 0)
        hop = f.sample_rate // 100
        n = -(-model.pcm_format_length(f, joined) // hop)
        st, en, ss, pk = np.zeros(ntok, np.int64), np.zeros(ntok, np.int64), np.zeros(ntok), np.zeros(ntok)
        es, ep = np.zeros(n), np.zeros(n)
        m = _lib.Sbv2Marks(ntok, st.ctypes.data_as(_lib.i64p), en.ctypes.data_as(_lib.i64p), ss.ctypes.data_as(f64p), pk.ctypes.data_as(f64p), 0, hop, 0,
                           n, es.ctypes.data_as(f64p), ep.ctypes.data_as(f64p), 0)
        args = (pipe.h, b.ticket, C.byref(req), pinned.array.ctypes.data, pinned.array.nbytes, C.byref(got), None, C.byref(m))
        if not with_pitch:
            _lib.check(l.sbv2_pipeline_fetch_request_marks(*args))
            return n, 0
        f0, apd, lag = np.zeros(n), np.zeros(n), np.zeros(n, np.int32)
        q = _lib.Sbv2Pitch(hop, 0, 70.0, 600.0, model.PITCH_THRESHOLD, n, f0.ctypes.data_as(f64p), apd.ctypes.data_as(f64p),
                           lag.ctypes.data_as(C.POINTER(C.c_int32)), 0)
        _lib.check(l.sbv2_pipeline_fetch_request_pitch(*args, C.byref(q)))
        return q.n_frames, int((f0 > 0).sum())

    formats = (model.PcmFormat(16000, "s16"), model.PcmFormat())
    if a.only_kernels:
        for f in formats:
            for _ in range(a.iters):
                fetch(f, a.only_kernels == "pitch")
        return

    def timeit(fn):
        fn()
        t = []
        for _ in range(a.iters):
            t0 = time.perf_counter()
            fn()
            t.append(time.perf_counter() - t0)
        return round(float(np.median(t)) * 1e3, 3), round(float(np.min(t)) * 1e3, 3), round(float(np.max(t)) * 1e3, 3)

    lines = []
    for f in formats:
        # marks, pitch, marks again: the second marks figure shows the run-to-run spread of the unchanged path on this machine
        t = [timeit(lambda: fetch(f, mode)) for mode in (False, True, False)]
        nf, voiced = fetch(f, True)
        lines.append(json.dumps({"format": f"{f.encoding} {f.sample_rate}", "audio_s": round(joined / 44100, 1), "pitch_frames": nf, "voiced": voiced,
                                 "lags": list(model.pitch_lags(f.sample_rate, 70.0, 600.0)), "fetch_marks_ms": t[0][0],
                                 "fetch_marks_min_max_ms": t[0][1:], "fetch_marks_pitch_ms": t[1][0], "fetch_marks_pitch_min_max_ms": t[1][1:],
                                 "fetch_marks_again_ms": t[2][0], "iters": a.iters}))
    print("\n".join(lines))
    if a.out:
        open(a.out, "w").write("\n".join(lines) + "\n")
    pinned.close(); pipe.close(); bs.close(); vs.close()


if __name__ == "__main__":
    main()
