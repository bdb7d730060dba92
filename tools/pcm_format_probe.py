"""Output-format probe: the plain f32 fetch against the formatted fetch (resample / quantise on the device, then D2H) on the bench-shaped batch
(full model, 32 utterances x 128 phonemes, forced durations: 10.4 s of 44.1 kHz audio each).

  python tools/pcm_format_probe.py [--iters 20] [--out FILE]
      wall time per fetch (device sync included: a fetch returns once the host holds the bytes) for f32 / 44.1 kHz and every rate x {f32, s16};
      JSON lines, one per format.
  rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/pcm_format_probe.py --iters 20 --only-kernels
      the same fetches without timing, for the kernel trace (run it as its own process);
  python tools/pcm_format_probe.py --summarise DIR/.../run_results.db [--iters 20]
      per format: the median k_pcm_resample time and its rate in bytes/s (f32 PCM read once + output written).  SBV2_PCM_TAPS=branch on the
      traced run gives the [L][T] tap layout for comparison.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

RATES = (8000, 16000, 22050, 24000, 32000, 44100, 48000)
NATIVE = 32 * (7 * 128 + 1) * 512    # samples of the bench batch


def summarise(path, iters):
    """path: the run_results.db (rocpd SQLite) rocprofv3 writes for the --only-kernels run, which launches the formats in RATES x (f32, s16)
    order, `iters` fetches each, one k_pcm_resample per fetch (f32 at 44.1 kHz per utterance is the plain copy: no kernel)."""
    import sqlite3
    if not os.path.exists(path):
        raise SystemExit(f"{path}: no such trace")
    rows = list(sqlite3.connect(path).execute("select duration from kernels where name like '%k_pcm_resample%' order by start"))
    fmts = [(r, e) for r in RATES for e in ("f32", "s16") if (r, e) != (44100, "f32")]
    if len(rows) != len(fmts) * iters:
        raise SystemExit(f"{len(rows)} k_pcm_resample dispatches, expected {len(fmts) * iters}")
    for i, (rate, enc) in enumerate(fmts):
        ns = [r[0] for r in rows[i * iters:(i + 1) * iters]]
        med = float(np.median(ns))
        g = int(np.gcd(rate, 44100))
        out = -(-NATIVE * (rate // g) // (44100 // g))
        moved = NATIVE * 4 + out * (2 if enc == "s16" else 4)
        print(json.dumps({"format": f"{enc} {rate}", "kernel_us_median": round(med / 1e3, 1), "kernel_us_min": round(min(ns) / 1e3, 1),
                          "bytes_read_written": moved, "GBps": round(moved / med, 1)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--only-kernels", action="store_true")
    ap.add_argument("--summarise")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.summarise is not None:
        summarise(a.summarise, a.iters)
        return
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
    assert n == NATIVE, n
    plain = model.PinnedArray(n)
    pinned = model.PinnedArray(n * 2)   # room for f32 at 48 kHz
    results = []

    def timeit(fn):
        fn()
        t = []
        for _ in range(a.iters):
            t0 = time.perf_counter()
            fn()
            t.append(time.perf_counter() - t0)
        return float(np.median(t)) * 1e3

    l = model._lib.lib()
    outs = np.zeros(len(utts), np.int64)

    def fetch_plain():
        model.check(l.sbv2_pipeline_fetch_pcm_ticket(pipe.h, b.ticket, plain.array.ctypes.data, n, 0))

    def fetch_fmt(f):
        model.check(l.sbv2_pipeline_fetch_pcm_format(pipe.h, b.ticket, f.c, None, 0, pinned.array.ctypes.data, pinned.array.nbytes,
                                                     outs.ctypes.data_as(model.i64p)))

    if a.only_kernels:
        for r in RATES:
            for enc in ("f32", "s16"):
                f = model.PcmFormat(r, enc)
                for _ in range(a.iters):
                    fetch_fmt(f)
        return
    ms = timeit(fetch_plain)
    results.append({"format": "plain f32 44100 (sbv2_pipeline_fetch_pcm_ticket)", "bytes": n * 4, "wall_ms": round(ms, 3)})
    for r in RATES:
        for enc in ("f32", "s16"):
            f = model.PcmFormat(r, enc)
            ms = timeit(lambda: fetch_fmt(f))
            out = int(outs.sum())
            results.append({"format": f"{enc} {r}", "bytes": out * (2 if enc == "s16" else 4), "wall_ms": round(ms, 3)})
    lines = [json.dumps(dict(r, pinned_dst=True, audio_s=round(n / 44100, 1))) for r in results]
    print("\n".join(lines))
    if a.out:
        open(a.out, "w").write("\n".join(lines) + "\n")
    plain.close(); pinned.close(); pipe.close(); bs.close(); vs.close()


if __name__ == "__main__":
    main()
