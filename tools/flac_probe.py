"""FLAC probe: the s16 formatted fetch against the FLAC fetch (s16 formatting, then the three encoder launches, then D2H of the encoded bytes)
on the bench-shaped batch (full model, 32 utterances x 128 phonemes, forced durations: 10.4 s of 44.1 kHz audio each).

  python tools/flac_probe.py [--iters 20] [--out FILE]
      wall time per fetch (device sync included: a fetch returns once the host holds the bytes) of sbv2_pipeline_fetch_pcm_format(s16) and
      sbv2_pipeline_fetch_flac at 44.1 and 16 kHz into pinned memory, plus the plain f32 fetch; JSON lines, one per fetch kind.
  rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/flac_probe.py --iters 20 --only-kernels
      the same FLAC fetches without timing, for the kernel trace (run it as its own process);
  python tools/flac_probe.py --summarise DIR/.../run_results.db [--iters 20]
      per rate: the median time of each FLAC kernel and of the s16 formatting kernel that feeds it.
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
NATIVE = 32 * (7 * 128 + 1) * 512    # samples of the bench batch
KERNELS = ("k_pcm_resample", "k_flac_analyse", "k_flac_scan", "k_flac_pack")


def summarise(path, iters):
    """path: the run_results.db (rocpd SQLite) rocprofv3 writes for the --only-kernels run, which makes `iters` FLAC fetches per rate in RATES
    order: one launch of each of KERNELS per fetch."""
    import sqlite3
    if not os.path.exists(path):
        raise SystemExit(f"{path}: no such trace")
    db = sqlite3.connect(path)
    for k in KERNELS:
        rows = [r[0] for r in db.execute(f"select duration from kernels where name like '%{k}%' order by start")]
        if len(rows) != len(RATES) * iters:
            raise SystemExit(f"{len(rows)} {k} dispatches, expected {len(RATES) * iters}")
        for i, rate in enumerate(RATES):
            ns = rows[i * iters:(i + 1) * iters]
            print(json.dumps({"rate": rate, "kernel": k, "us_median": round(float(np.median(ns)) / 1e3, 1), "us_min": round(min(ns) / 1e3, 1)}))


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
    pinned = model.PinnedArray(n)   # 4 n bytes: room for s16 and for every FLAC bound at <= 44.1 kHz
    l = model._lib.lib()
    outs = np.zeros(len(utts), np.int64)

    def fetch_plain():
        model.check(l.sbv2_pipeline_fetch_pcm_ticket(pipe.h, b.ticket, plain.array.ctypes.data, n, 0))

    def fetch_s16(f):
        model.check(l.sbv2_pipeline_fetch_pcm_format(pipe.h, b.ticket, f.c, None, 0, pinned.array.ctypes.data, pinned.array.nbytes,
                                                     outs.ctypes.data_as(model.i64p)))

    def fetch_flac(f):
        model.check(l.sbv2_pipeline_fetch_flac(pipe.h, b.ticket, f.c, None, 0, pinned.array.ctypes.data, pinned.array.nbytes,
                                               outs.ctypes.data_as(model.i64p)))

    if a.only_kernels:
        for r in RATES:
            f = model.PcmFormat(r, "s16")
            for _ in range(a.iters):
                fetch_flac(f)
        return

    def timeit(fn):
        fn()
        t = []
        for _ in range(a.iters):
            t0 = time.perf_counter()
            fn()
            t.append(time.perf_counter() - t0)
        return float(np.median(t)) * 1e3

    results = [{"fetch": "plain f32 44100 (sbv2_pipeline_fetch_pcm_ticket)", "bytes": n * 4, "wall_ms": round(timeit(fetch_plain), 3)}]
    for r in RATES:
        f = model.PcmFormat(r, "s16")
        ms = timeit(lambda: fetch_s16(f))
        s16_bytes = int(outs.sum()) * 2
        results.append({"fetch": f"s16 {r}", "bytes": s16_bytes, "wall_ms": round(ms, 3)})
        ms = timeit(lambda: fetch_flac(f))
        fl = int(outs.sum())
        results.append({"fetch": f"flac {r}", "bytes": fl, "ratio_to_s16": round(fl / s16_bytes, 4), "wall_ms": round(ms, 3)})
    lines = [json.dumps(dict(r, pinned_dst=True, audio_s=round(n / 44100, 1))) for r in results]
    print("\n".join(lines))
    if a.out:
        open(a.out, "w").write("\n".join(lines) + "\n")
    plain.close(); pinned.close(); pipe.close(); bs.close(); vs.close()


if __name__ == "__main__":
    main()
