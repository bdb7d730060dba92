"""Request streams (a multi-sentence request delivered sentence by sentence) and the long-form stream they share their code with, one process.
(a) --request: a request of --sentences x --phonemes phonemes on the full-size models, s16 at --rate: time to the first and to the last piece
    through orchestrator.easy_synthesize_stream(split=True), against orchestrator.easy_synthesize of the same request (one answer at the end)
    and against the same text as ONE utterance through the single-utterance stream (split=False).  Skipped on a tree without request streams.
(b) --longform: the 2000-phoneme utterance (162.6 s of audio) as an s16 stream at 44.1 kHz in 256-frame chunks: time to the first chunk and
    to the last one.  Runs on any tree with formatted streams, so two trees can be compared on one machine.
Medians over --runs after one unmeasured run (graph capture, buffer growth).  One JSON line per measurement.
Usage: python tools/stream_sentences_probe.py [--request] [--longform] [--runs 7] [--tag NAME]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))

import numpy as np  # noqa: E402
import sbv2_oracle as O  # noqa: E402
from sbv2_api_amd import model, orchestrator, synth  # noqa: E402


def timed_pieces(make):
    """(ms to the first piece after the header, ms to the last piece, pieces, bytes) of one streamed answer."""
    t0 = time.perf_counter()
    st = make()
    first, n, size = None, 0, 0
    for i, p in enumerate(st):
        if i >= 1 and first is None:   # (piece 0 is the WAV header, written before any sample exists)
            first = (time.perf_counter() - t0) * 1e3
        n += 1
        size += len(p)
    return first, (time.perf_counter() - t0) * 1e3, n, size


def med(rows, k):
    return round(statistics.median(r[k] for r in rows), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--request", action="store_true")
    ap.add_argument("--longform", action="store_true")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--sentences", type=int, default=4)
    ap.add_argument("--phonemes", type=int, default=64)
    ap.add_argument("--rate", type=int, default=24000)
    ap.add_argument("--chunk", type=int, default=64)
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    bc, vc = O.DEBERTA_FULL, O.VITS_FULL
    bs = model.load_model(synth.pack_blob(synth.KIND_BERT, bc, synth.make_deberta_weights(bc, 0x5B72)), True)
    vs = model.load_model(synth.pack_blob(synth.KIND_VITS, vc, synth.make_vits_weights(vc, 0x5B72)), False)
    if a.request and hasattr(model, "stream_min_gap"):
        keys = ("input_ids", "word2ph", "phones", "tones", "langs")
        sent = [{k: synth.make_utterance(a.phonemes, bc, vc, seed=300 + i)[k] for k in keys} for i in range(a.sentences)]
        whole = {k: synth.make_utterance(a.phonemes * a.sentences, bc, vc, seed=300)[k] for k in keys}
        styles = synth.hash_normal(77, 3 * vc["style_dim"]).reshape(3, -1).astype(np.float32)
        opts = orchestrator.SynthesizeOptions(sample_rate=a.rate, encoding="s16")
        pipe = model.Pipeline(bs, vs)
        kinds = {
            "request_stream": lambda: timed_pieces(lambda: orchestrator.easy_synthesize_stream(bs, vs, sent, styles, 1, 0, opts, noise_seed=7,
                                                                                               chunk_frames=a.chunk, split=True)),
            "one_utterance_stream": lambda: timed_pieces(lambda: orchestrator.easy_synthesize_stream(bs, vs, [whole], styles, 1, 0, opts, noise_seed=7,
                                                                                                     chunk_frames=a.chunk)),
        }

        def whole_answer():
            t0 = time.perf_counter()
            wav = orchestrator.easy_synthesize(pipe, sent, styles, 1, 0, opts, noise_seed=7)
            ms = (time.perf_counter() - t0) * 1e3
            return ms, ms, 1, len(wav)

        kinds["easy_synthesize"] = whole_answer
        rows = {k: [] for k in kinds}
        for r in range(a.runs + 1):
            for k, f in kinds.items():
                row = f()
                if r:
                    rows[k].append(row)
        for k, r in rows.items():
            print(json.dumps({"tag": a.tag, "kind": k, "sentences": a.sentences, "phonemes": a.phonemes, "rate": a.rate, "chunk": a.chunk, "runs": a.runs,
                              "first_ms_median": med(r, 0), "first_ms_min": round(min(x[0] for x in r), 3), "last_ms_median": med(r, 1),
                              "last_ms_min": round(min(x[1] for x in r), 3), "pieces": r[0][2], "bytes": r[0][3]}), flush=True)
        pipe.close()
    if a.longform:
        u = synth.make_utterance(2000, bc, vc, seed=991)
        fmt = model.PcmFormat(44100, "s16")
        rows = []
        for r in range(a.runs + 1):
            t0 = time.perf_counter()
            st = model.StreamHandle(bs, vs, u, 256, fmt=fmt, forced=True)
            first, n, samples = None, 0, 0
            while (c := st.next()) is not None:
                if first is None:
                    first = (time.perf_counter() - t0) * 1e3
                n += 1
                samples += c.size
            last = (time.perf_counter() - t0) * 1e3
            st.close()
            if r:
                rows.append((first, last, n, samples))
        print(json.dumps({"tag": a.tag, "kind": "longform_s16_44100", "runs": a.runs, "chunks": rows[0][2], "samples": rows[0][3],
                          "first_ms_median": med(rows, 0), "last_ms_median": med(rows, 1), "last_ms_min": round(min(x[1] for x in rows), 3),
                          "last_ms_max": round(max(x[1] for x in rows), 3)}), flush=True)
    bs.close()
    vs.close()


if __name__ == "__main__":
    main()
