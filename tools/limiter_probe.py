"""Limiter probe: the s16 fetch with loudness normalisation (scale only) and through the look-ahead limiter, same target and ceiling, on the
bench batch (32 x 128 phonemes at full model size) at 44.1 and 16 kHz: the median wall time of `--iters` fetches into pinned memory, and
what the limiter buys on this audio (peak-to-loudness ratio, scale-only loudness, limited loudness per utterance).

  python tools/limiter_probe.py [--iters 20] [--target -16] [--out FILE]
  rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/limiter_probe.py --iters 20 --only-kernels
      the limited fetches alone, without timing, for the per-kernel table (run it as its own process)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

RATES = (44100, 16000)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--target", type=float, default=-16.0)
    ap.add_argument("--max-reduction", type=float, default=6.0)
    ap.add_argument("--only-kernels", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
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
    n = int(b.lens.sum())
    pinned = model.PinnedArray(n)   # room for s16 at <= 44.1 kHz
    l = model._lib.lib()
    outs = np.zeros(len(utts), np.int64)
    s3, s6 = np.zeros((len(utts), 3), np.float64), np.zeros((len(utts), 6), np.float64)
    f64p = model.C.POINTER(model.C.c_double)
    ln, lim = model.Loudness(a.target, -1.0), model.Limiter(a.target, -1.0, a.max_reduction)

    def fetch(f, limited):
        if limited:
            model.check(l.sbv2_pipeline_fetch_pcm_limited(pipe.h, b.ticket, f.c, lim.c, None, 0, pinned.array.ctypes.data, pinned.array.nbytes,
                                                          outs.ctypes.data_as(model.i64p), s6.ctypes.data_as(f64p)))
        else:
            model.check(l.sbv2_pipeline_fetch_pcm_loudness(pipe.h, b.ticket, f.c, ln.c, None, 0, pinned.array.ctypes.data, pinned.array.nbytes,
                                                           outs.ctypes.data_as(model.i64p), s3.ctypes.data_as(f64p)))

    if a.only_kernels:
        for r in RATES:
            for _ in range(a.iters):
                fetch(model.PcmFormat(r, "s16"), True)
        return

    def timeit(fn):
        fn()
        t = []
        for _ in range(a.iters):
            t0 = time.perf_counter()
            fn()
            t.append(time.perf_counter() - t0)
        return float(np.median(t)) * 1e3

    def rng(v):
        return [round(float(np.min(v)), 2), round(float(np.median(v)), 2), round(float(np.max(v)), 2)]

    lines = []
    for r in RATES:
        f = model.PcmFormat(r, "s16")
        t_scale = timeit(lambda: fetch(f, False))
        t_lim = timeit(lambda: fetch(f, True))
        lines.append(json.dumps({
            "format": f"s16 {r}", "target_lufs": a.target, "max_reduction_db": a.max_reduction, "loudness_ms": round(t_scale, 3),
            "limited_ms": round(t_lim, 3), "ratio": round(t_lim / t_scale, 2), "audio_s": round(n / 44100, 1),
            "min_med_max": {"PLR_db": rng(s6[:, 1] - s6[:, 0]), "scale_only_lufs": rng(s3[:, 0] + s3[:, 2]), "limited_lufs": rng(s6[:, 3]),
                            "G_db": rng(s6[:, 2]), "TP_out_dbtp": rng(s6[:, 4]), "depth_db": rng(s6[:, 5])},
            "max_TP_out_over_ceiling_db": float(f"{float(np.max(s6[:, 4])) + 1.0:.3e}")}))
    print("\n".join(lines))
    if a.out:
        open(a.out, "w").write("\n".join(lines) + "\n")
    pinned.close(); pipe.close(); bs.close(); vs.close()


if __name__ == "__main__":
    main()
