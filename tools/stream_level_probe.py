"""Level stream against the s16 formatted stream on the long-form input (2000 phonemes, 162.6 s of audio, 256-frame chunks), one process:
(a) time from sbv2_stream_begin_* to the return of the next call that delivers the first sample (the level stream runs A samples behind, so
its first call delivers A samples fewer, not nothing, at these chunk sizes), (b) the time of each later call: median, min and max over the
chunks of a run, then medians of those over --runs, (c) the level stats.  The two kinds alternate run by run.
Usage: python tools/stream_level_probe.py [--runs 10] [--rates 44100,16000] [--gain-db 12]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))

import sbv2_oracle as O  # noqa: E402
from sbv2_api_amd import model, synth  # noqa: E402


def one(bs, vs, u, chunk, fmt, level):
    t0 = time.perf_counter()
    st = model.StreamHandle(bs, vs, u, chunk, fmt=fmt, level=level, forced=True)
    first, later, samples, chunks = None, [], 0, 0
    t = t0
    while (c := st.next()) is not None:
        now = time.perf_counter()
        chunks += 1
        samples += c.size
        if first is None:
            if c.size:
                first = (now - t0) * 1e3
        else:
            later.append((now - t) * 1e3)
        t = now
    stats = st.level_stats() if level is not None else None
    st.close()
    return first, later, samples, chunks, stats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--rates", default="44100,16000")
    ap.add_argument("--phonemes", type=int, default=2000)
    ap.add_argument("--chunk", type=int, default=256)
    ap.add_argument("--gain-db", type=float, default=12.0)
    a = ap.parse_args()
    bc, vc = O.DEBERTA_FULL, O.VITS_FULL
    bs = model.load_model(synth.pack_blob(synth.KIND_BERT, bc, synth.make_deberta_weights(bc, 0x5B72)), True)
    vs = model.load_model(synth.pack_blob(synth.KIND_VITS, vc, synth.make_vits_weights(vc, 0x5B72)), False)
    u = synth.make_utterance(a.phonemes, bc, vc, seed=991)
    lv = model.StreamLevel(a.gain_db, -1.0)
    for rate in (int(r) for r in a.rates.split(",")):
        fmt = model.PcmFormat(rate, "s16")
        for level in (None, lv):      # captures the graphs and grows every buffer: not measured
            one(bs, vs, u, a.chunk, fmt, level)
        rows = {False: [], True: []}
        for _ in range(a.runs):
            for level in (None, lv):
                rows[level is not None].append(one(bs, vs, u, a.chunk, fmt, level))
        for on in (False, True):
            r = rows[on]
            out = {"rate": rate, "kind": "level" if on else "s16", "runs": a.runs, "chunks": r[0][3], "samples": r[0][2],
                   "lookahead": model.stream_level_lookahead(fmt) if on else 0,
                   "first_ms_median": round(statistics.median(x[0] for x in r), 3), "first_ms_min": round(min(x[0] for x in r), 3),
                   "first_ms_max": round(max(x[0] for x in r), 3),
                   "later_chunk_ms_median": round(statistics.median(statistics.median(x[1]) for x in r), 4),
                   "later_chunk_ms_min": round(statistics.median(min(x[1]) for x in r), 4),
                   "later_chunk_ms_max": round(statistics.median(max(x[1]) for x in r), 4),
                   # (a burst replay delivers 8 chunks at once: most calls only copy, so the mean is the per-chunk cost of the stream)
                   "later_chunk_ms_mean": round(statistics.median(sum(x[1]) / max(len(x[1]), 1) for x in r), 4),
                   "later_total_ms_median": round(statistics.median(sum(x[1]) for x in r), 3)}
            if on:
                out["gain_db"], out["depth_db"], out["max_abs_x"] = a.gain_db, round(r[0][4][0], 3), round(r[0][4][1], 6)
            print(json.dumps(out), flush=True)
    bs.close()
    vs.close()


if __name__ == "__main__":
    main()
