"""FLAC stream against the s16 formatted stream on the long-form input (2000 phonemes, 162.6 s of audio, 256-frame chunks), one process:
(a) time from sbv2_stream_begin_* to the return of the first next call, (b) mean time per later chunk, (c) bytes delivered.
The two kinds alternate run by run; medians over --runs.  Usage: python tools/flac_stream_probe.py [--runs 10] [--rates 44100,16000]"""
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


def one(bs, vs, u, chunk, fmt, flac):
    t0 = time.perf_counter()
    st = model.StreamHandle(bs, vs, u, chunk, fmt=fmt, flac=flac, forced=True)
    c = st.next()
    t1 = time.perf_counter()
    nbytes, chunks = len(c) if flac else c.nbytes, 1
    while (c := st.next()) is not None:
        nbytes += len(c) if flac else c.nbytes
        chunks += 1
    t2 = time.perf_counter()
    st.close()
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3 / max(chunks - 1, 1), nbytes, chunks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--rates", default="44100,16000")
    ap.add_argument("--phonemes", type=int, default=2000)
    ap.add_argument("--chunk", type=int, default=256)
    a = ap.parse_args()
    bc, vc = O.DEBERTA_FULL, O.VITS_FULL
    bs = model.load_model(synth.pack_blob(synth.KIND_BERT, bc, synth.make_deberta_weights(bc, 0x5B72)), True)
    vs = model.load_model(synth.pack_blob(synth.KIND_VITS, vc, synth.make_vits_weights(vc, 0x5B72)), False)
    u = synth.make_utterance(a.phonemes, bc, vc, seed=991)
    for rate in (int(r) for r in a.rates.split(",")):
        fmt = model.PcmFormat(rate, "s16")
        for flac in (False, True):      # captures the graphs and grows every buffer: not measured
            one(bs, vs, u, a.chunk, fmt, flac)
        rows = {False: [], True: []}
        for _ in range(a.runs):
            for flac in (False, True):
                rows[flac].append(one(bs, vs, u, a.chunk, fmt, flac))
        for flac in (False, True):
            first = [r[0] for r in rows[flac]]
            later = [r[1] for r in rows[flac]]
            print(json.dumps({"rate": rate, "kind": "flac" if flac else "s16", "runs": a.runs, "chunks": rows[flac][0][3],
                              "first_ms_median": round(statistics.median(first), 3), "first_ms_min": round(min(first), 3),
                              "first_ms_max": round(max(first), 3), "later_chunk_ms_median": round(statistics.median(later), 4),
                              "later_chunk_ms_min": round(min(later), 4), "later_chunk_ms_max": round(max(later), 4),
                              "bytes": rows[flac][0][2]}), flush=True)
    bs.close()
    vs.close()


if __name__ == "__main__":
    main()
