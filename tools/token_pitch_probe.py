"""Token pitch probe: a Voice(1.2, 1.0) request fetch of the bench batch (32 x 128 phonemes at full model size, all rows on one joined
timeline) without and with a full token table (every token edited, ratios, smooth 2), at 16 kHz s16 and 44.1 kHz f32: the median wall time of
`--iters` fetches into pinned host memory after one warm-up.  The fetch without the table is timed twice, so that the record carries its own
run-to-run spread.  A library without token pitch (an older commit) reports the fetch without it only, so the same file measures both sides of
a comparison.

  python tools/token_pitch_probe.py [--iters 25] [--out FILE]"""
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

FORMATS = ((16000, "s16"), (44100, "f32"))
GAP = 22050   # native samples of silence between the rows (the orchestrator's sentence gap)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=25)
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
    rows = list(range(len(utts)))
    place = [int(v) for v in np.concatenate([[0], np.cumsum(b.lens[:-1] + GAP)])]
    joined = place[-1] + int(b.lens[-1])
    n_tok = int(sum(int(b.t_lens[r]) for r in rows))
    C, l = model.C, model._lib.lib()
    rw, pl = np.asarray(rows, np.int32), np.asarray(place, np.int64)
    pinned = model.PinnedArray(joined)   # pinned host memory: room for f32 at 44.1 kHz, no page faults in the timed region
    got = C.c_int64(0)
    voice = model.Voice(1.2, 1.0)
    tp = model.TokenPitch(0.8 + 0.05 * (np.arange(n_tok) % 9), "ratio", 2) if hasattr(model, "TokenPitch") else None

    def fetch(f, table):
        req = model.Sbv2FetchRequest(rw.ctypes.data_as(C.POINTER(C.c_int32)), rw.size, pl.ctypes.data_as(model.i64p), joined, C.pointer(f.c), None,
                                     None, 0)
        tail = (pinned.array.ctypes.data, pinned.array.nbytes, C.byref(got), None)
        cv = voice.c
        if table:
            ctp, keep = tp.c_struct()
            model.check(l.sbv2_pipeline_fetch_request_token_pitch(pipe.h, b.ticket, C.byref(req), C.byref(cv), None, None, C.byref(ctp), *tail, None,
                                                                  None, None))
            return tp.take(keep)
        model.check(l.sbv2_pipeline_fetch_request_voice(pipe.h, b.ticket, C.byref(req), C.byref(cv), *tail, None, None))

    def timeit(fn):
        fn()
        t = []
        for _ in range(a.iters):
            t0 = time.perf_counter()
            fn()
            t.append(time.perf_counter() - t0)
        return [round(float(v) * 1e3, 3) for v in (np.median(t), np.min(t), np.max(t))]

    lines = []
    for r, e in FORMATS:
        f = model.PcmFormat(r, e)
        rec = {"format": f"{e} {r}", "audio_s": round(joined / 44100, 1), "tokens": n_tok, "iters": a.iters}
        rec["voice_ms_1"] = timeit(lambda: fetch(f, False))
        if tp is not None:
            rec["voice_token_table_ms"] = timeit(lambda: fetch(f, True))
            t = fetch(f, True)
            rec["tokens_with_a_voiced_frame"] = int((t.src_f0 > 0).sum())
        rec["voice_ms_2"] = timeit(lambda: fetch(f, False))
        lines.append(json.dumps(rec))
    print("\n".join(lines))
    if a.out:
        open(a.out, "w").write("\n".join(lines) + "\n")
    pinned.close(); pipe.close(); bs.close(); vs.close()


if __name__ == "__main__":
    main()
