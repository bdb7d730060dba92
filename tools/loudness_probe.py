"""Loudness probe: the s16 fetch with no normalisation, with peak normalisation and with loudness normalisation (-23 LUFS, -1 dBTP) on the
bench-shaped batch (full model, 32 utterances x 128 phonemes, forced durations: 10.4 s of 44.1 kHz audio each), at 44.1 and 16 kHz.

  python tools/loudness_probe.py [--iters 20] [--out FILE]
      wall time per fetch (device sync included: a fetch returns once the host holds the bytes and stats); JSON lines, one per fetch kind.
  rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/loudness_probe.py --iters 20 --only-kernels
      the loudness fetches alone, without timing, for the kernel trace (run it as its own process);
  python tools/loudness_probe.py --summarise DIR/.../run_results.db [--iters 20]
      per rate: the median time of each loudness kernel (k_kw_zero, k_kw_carry, k_kw_rerun, k_true_peak, k_gate, k_pcm_gain_sig) and
      of the f64 resampling pass they follow, and their sum.
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

RATES = (44100, 16000)
KERNELS = ("k_pcm_resample", "k_kw_zero", "k_kw_carry", "k_kw_rerun", "k_true_peak", "k_gate", "k_pcm_gain_sig")
NATIVE = 32 * (7 * 128 + 1) * 512    # samples of the bench batch


def summarise(path, iters):
    """path: the run_results.db (rocpd SQLite) rocprofv3 writes for the --only-kernels run, which makes `iters` loudness fetches per rate in
    RATES order: one dispatch of each kernel per fetch."""
    import sqlite3
    if not os.path.exists(path):
        raise SystemExit(f"{path}: no such trace")
    db = sqlite3.connect(path)
    for i, rate in enumerate(RATES):
        row = {"rate": rate, "samples": -(-NATIVE * rate // 44100)}
        total = 0.0
        for k in KERNELS:
            ns = [r[0] for r in db.execute(f"select duration from kernels where name like '%{k}%' order by start")]
            if len(ns) != len(RATES) * iters:
                raise SystemExit(f"{len(ns)} {k} dispatches, expected {len(RATES) * iters}")
            med = float(np.median(ns[i * iters:(i + 1) * iters])) / 1e3
            row[f"{k}_us"] = round(med, 1)
            if k != "k_pcm_resample":
                total += med
        row["new_kernels_us"] = round(total, 1)
        print(json.dumps(row))


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
    pinned = model.PinnedArray(n)   # room for s16 at <= 44.1 kHz
    l = model._lib.lib()
    outs = np.zeros(len(utts), np.int64)
    stats = np.zeros((len(utts), 3), np.float64)
    ln = model.Loudness(-23.0, -1.0)

    def fetch(f, loud):
        if loud:
            model.check(l.sbv2_pipeline_fetch_pcm_loudness(pipe.h, b.ticket, f.c, ln.c, None, 0, pinned.array.ctypes.data,
                                                           pinned.array.nbytes, outs.ctypes.data_as(model.i64p),
                                                           stats.ctypes.data_as(model.C.POINTER(model.C.c_double))))
        else:
            model.check(l.sbv2_pipeline_fetch_pcm_format(pipe.h, b.ticket, f.c, None, 0, pinned.array.ctypes.data, pinned.array.nbytes,
                                                         outs.ctypes.data_as(model.i64p)))

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

    lines = []
    for r in RATES:
        for kind, f, loud in (("none", model.PcmFormat(r, "s16"), False), ("peak", model.PcmFormat(r, "s16", True), False),
                              ("loudness -23 LUFS", model.PcmFormat(r, "s16"), True)):
            ms = timeit(lambda: fetch(f, loud))
            row = {"format": f"s16 {r}", "normalisation": kind, "bytes": int(outs.sum()) * 2, "wall_ms": round(ms, 3)}
            if loud:
                row["L_range"] = [round(float(stats[:, 0].min()), 2), round(float(stats[:, 0].max()), 2)]
            lines.append(json.dumps(dict(row, pinned_dst=True, audio_s=round(n / 44100, 1))))
    print("\n".join(lines))
    if a.out:
        open(a.out, "w").write("\n".join(lines) + "\n")
    pinned.close(); pipe.close(); bs.close(); vs.close()


if __name__ == "__main__":
    main()
