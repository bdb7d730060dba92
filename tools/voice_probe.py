"""Voice probe: what pitch_scale / intonation_scale add to a request fetch on the bench batch (32 x 128 phonemes at full model size, all rows on
one joined timeline) at 44.1 kHz f32 and 16 kHz s16: the median wall time of `--iters` fetches into pinned memory without a voice (the code path
of sbv2_pipeline_fetch_request, which must stay what it was), with Voice(1.2, 1.0) (sbv2_pipeline_fetch_request_voice: the contour of every row
at 200 frames per second, the marks, the overlap-add gather, then the same formatter) and without again.

  python tools/voice_probe.py [--iters 20] [--out FILE]
  rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/voice_probe.py --iters 20 --only-kernels voice
      the fetches with a voice alone, for the per-kernel table that splits the difference into contour (k_pitch_yin), marks (k_voice_marks) and
      gather (k_voice_gather), in its own process; --only-kernels plain: the fetches without, whose trace must show none of the three."""
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
    ap.add_argument("--only-kernels", choices=["plain", "voice"])
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
    got = C.c_int64()
    voice = _lib.Sbv2Voice(1.2, 1.0, 0.0, 0.0, 0.0, 0, 0)

    def fetch(f, with_voice):
        req = _lib.Sbv2FetchRequest(rows.ctypes.data_as(C.POINTER(C.c_int32)), 32, pl.ctypes.data_as(_lib.i64p), joined, C.pointer(f.c), None, None, 0)
        if with_voice:
            _lib.check(l.sbv2_pipeline_fetch_request_voice(pipe.h, b.ticket, C.byref(req), C.byref(voice), pinned.array.ctypes.data, pinned.array.nbytes,
                                                           C.byref(got), None, None, None))
        else:
            _lib.check(l.sbv2_pipeline_fetch_request(pipe.h, b.ticket, C.byref(req), pinned.array.ctypes.data, pinned.array.nbytes, C.byref(got), None))

    formats = (model.PcmFormat(), model.PcmFormat(16000, "s16"))
    if a.only_kernels:
        for f in formats:
            for _ in range(a.iters):
                fetch(f, a.only_kernels == "voice")
        return

    def timeit(fn):
        fn()
        t = []
        for _ in range(a.iters):
            t0 = time.perf_counter()
            fn()
            t.append(time.perf_counter() - t0)
        return round(float(np.median(t)) * 1e3, 3), round(float(np.min(t)) * 1e3, 3), round(float(np.max(t)) * 1e3, 3)

    frames = int(sum(-(-int(n) // (44100 // 200)) for n in b.lens))
    lines = []
    for f in formats:
        # plain, voice, plain again: the second plain figure shows the run-to-run spread of the unchanged path on this machine
        t = [timeit(lambda: fetch(f, mode)) for mode in (False, True, False)]
        fetch(f, False)
        plain = pinned.array[:got.value].copy() if f.encoding == "f32" else None
        fetch(f, True)
        changed = None if plain is None else round(float((pinned.array[:got.value] != plain).mean()), 4)
        lines.append(json.dumps({"format": f"{f.encoding} {f.sample_rate}", "audio_s": round(joined / 44100, 1), "rows": 32, "contour_frames": frames,
                                 "samples_changed": changed, "fetch_ms": t[0][0], "fetch_min_max_ms": t[0][1:], "fetch_voice_ms": t[1][0],
                                 "fetch_voice_min_max_ms": t[1][1:], "fetch_again_ms": t[2][0], "iters": a.iters}))
    print("\n".join(lines))
    if a.out:
        open(a.out, "w").write("\n".join(lines) + "\n")
    pinned.close(); pipe.close(); bs.close(); vs.close()


if __name__ == "__main__":
    main()
