"""G.711 probe: the 8 kHz formatted fetch of the bench-shaped batch (full model, 32 utterances x 128 phonemes, forced durations: 10.4 s of
44.1 kHz audio each) as s16, mu-law and A-law.

  python tools/g711_probe.py [--iters 25] [--rounds 3] [--out FILE]
      wall time per fetch (device sync included: a fetch returns once the host holds the bytes, in pinned memory).  The three encodings
      alternate fetch by fetch in one process, so clock and neighbour drift hits them alike; every round gives one median of `iters`
      fetches per encoding, and the spread of the s16 medians over the rounds is the yardstick for a difference between the rows.
      JSON lines, one per encoding.  The codes are checked against sbv2_g711_encode of the s16 samples before anything is timed.
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

RATE = 8000
ENCODINGS = ("s16", "mulaw", "alaw")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=25)
    ap.add_argument("--rounds", type=int, default=3)
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
    fmts = {e: model.PcmFormat(RATE, e) for e in ENCODINGS}
    total = sum(model.pcm_format_length(fmts["s16"], int(x)) for x in b.lens)
    pinned = model.PinnedArray(total)   # 4 bytes per sample: room for every encoding
    l = model._lib.lib()
    outs = np.zeros(len(utts), np.int64)

    def fetch(e):
        model.check(l.sbv2_pipeline_fetch_pcm_format(pipe.h, b.ticket, fmts[e].c, None, 0, pinned.array.ctypes.data, pinned.array.nbytes,
                                                     outs.ctypes.data_as(model.i64p)))

    s16 = np.concatenate(pipe.fetch_format(b, fmts["s16"]))
    for e in ENCODINGS[1:]:
        assert np.array_equal(np.concatenate(pipe.fetch_format(b, fmts[e])), model.g711_encode(s16, e)), e
    for e in ENCODINGS:   # warm-up: tables, buffers
        fetch(e)
    medians = {e: [] for e in ENCODINGS}
    for _ in range(a.rounds):
        t = {e: [] for e in ENCODINGS}
        for _ in range(a.iters):
            for e in ENCODINGS:
                t0 = time.perf_counter()
                fetch(e)
                t[e].append(time.perf_counter() - t0)
        for e in ENCODINGS:
            medians[e].append(float(np.median(t[e])) * 1e3)
    lines = []
    for e in ENCODINGS:
        m = medians[e]
        lines.append(json.dumps({"format": f"{e} {RATE}", "store": "one byte per thread" if e != "s16" else "one s16 per thread",
                                 "bytes": total * np.dtype(fmts[e].dtype).itemsize, "wall_ms_median_per_round": [round(v, 3) for v in m],
                                 "wall_ms": round(float(np.median(m)), 3), "spread_ms": round(max(m) - min(m), 3), "iters": a.iters,
                                 "pinned_dst": True, "audio_s": round(n / 44100, 1)}))
    print("\n".join(lines))
    if a.out:
        open(a.out, "w").write("\n".join(lines) + "\n")
    pinned.close(); pipe.close(); bs.close(); vs.close()


if __name__ == "__main__":
    main()
