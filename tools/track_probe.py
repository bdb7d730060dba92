"""Track probe: what pitch tracking (octave-error repair) adds to a request fetch on the bench batch (32 x 128 phonemes at full model size, all rows
on one joined timeline) at 44.1 kHz f32 and 16 kHz s16: the median wall time of `--iters` fetches into pinned memory with marks and a 100 Hz
pitch contour untracked (sbv2_pipeline_fetch_request_pitch, which must stay what it was), tracked (sbv2_pipeline_fetch_request_tracked),
untracked again, with Voice(1.2, 1.0) untracked and with Voice(1.2, 1.0) tracked.  On a tree without the tracked entry point (the parent commit)
the untracked modes alone are timed.

  python tools/track_probe.py [--iters 20] [--out FILE]
  rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/track_probe.py --iters 10 --only-kernels tracked
      the tracked fetches alone, for the per-kernel table (k_pitch_yin_cand, k_track_runs, k_track_path), in its own process;
      --only-kernels plain: the untracked ones, whose trace must show none of the three.
      --only-kernels voice-tracked: the tracked Voice(1.2, 1.0) fetches alone (32 k_pitch_yin_cand launches and ONE tracker call for all rows).
  rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/track_probe.py --iters 10 --only-kernels path-split
      k_track_path alone through the hook, on the candidate table of the 16 kHz fetch as it is: its runs side by side.
      --only-kernels path-whole, in a process and a trace of its own: the same table with one dear candidate put into every cut, so that no cut
      is left and ONE wave walks the whole signal."""
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
    ap.add_argument("--only-kernels", choices=["plain", "tracked", "voice-tracked", "path-split", "path-whole"])
    ap.add_argument("--out")
    a = ap.parse_args()
    import sbv2_oracle as O
    from sbv2_api_amd import _lib, model, orchestrator, synth

    has_track = "sbv2_pipeline_fetch_request_tracked" in _lib.SYMBOLS
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
    track = model.PitchTrack().c if has_track else None
    ntok = int(sum(int(n) for n in b.t_lens))
    tok = [np.zeros(ntok, np.int64), np.zeros(ntok, np.int64), np.zeros(ntok), np.zeros(ntok)]
    f64p = C.POINTER(C.c_double)
    last = {}

    def fetch(f, with_voice, tracked, contour=True):
        out_len = model.pcm_format_length(f, joined)
        hop = f.sample_rate // 100
        nf = -(-out_len // hop)
        env = [np.zeros(nf), np.zeros(nf)]
        req = _lib.Sbv2FetchRequest(rows.ctypes.data_as(C.POINTER(C.c_int32)), 32, pl.ctypes.data_as(_lib.i64p), joined, C.pointer(f.c), None, None, 0)
        cm = _lib.Sbv2Marks(ntok, tok[0].ctypes.data_as(_lib.i64p), tok[1].ctypes.data_as(_lib.i64p), tok[2].ctypes.data_as(f64p), tok[3].ctypes.data_as(f64p),
                            0, hop, 0, nf, env[0].ctypes.data_as(f64p), env[1].ctypes.data_as(f64p), 0)
        f0, apc, lag = np.zeros(nf), np.zeros(nf), np.zeros(nf, np.int32)
        cp = _lib.Sbv2Pitch(hop, 0, 70.0, 600.0, 0.15, nf, f0.ctypes.data_as(f64p), apc.ctypes.data_as(f64p), lag.ctypes.data_as(C.POINTER(C.c_int32)), 0)
        args = (pinned.array.ctypes.data, pinned.array.nbytes, C.byref(got), None, C.byref(cm), C.byref(cp) if contour else None)
        v = C.byref(voice) if with_voice else None
        if tracked:
            _lib.check(l.sbv2_pipeline_fetch_request_tracked(pipe.h, b.ticket, C.byref(req), v, C.byref(track), *args))
        else:
            _lib.check(l.sbv2_pipeline_fetch_request_voice(pipe.h, b.ticket, C.byref(req), v, *args))
        last.update(f0=f0, ap=apc, lag=lag, nf=nf)

    formats = (model.PcmFormat(), model.PcmFormat(16000, "s16"))
    if a.only_kernels in ("plain", "tracked"):
        for f in formats:
            for _ in range(a.iters):
                fetch(f, False, a.only_kernels == "tracked")
        return
    if a.only_kernels == "voice-tracked":
        for f in formats:
            for _ in range(a.iters):
                fetch(f, True, True, False)
        return
    if a.only_kernels in ("path-split", "path-whole"):
        f = formats[1]
        samples, _ = pipe.fetch_request(b, rows, f, place, joined)
        r = model.debug_pitch_track(samples, f.sample_rate, model.Pitch(f.sample_rate // 100), model.PitchTrack())
        whole = r.cand.copy()
        cut = whole[:, 0] == 0
        whole[cut, 0], whole[cut, 1], whole[cut, 8] = 1, 100, 65536
        for _ in range(a.iters):
            model.debug_pitch_track(None, 0, None, model.PitchTrack(), cand=r.cand if a.only_kernels == "path-split" else whole)
        print(json.dumps({"frames": int(len(cut)), "cuts": int(cut.sum()), "runs": int(cut.sum()) + int(not cut[0])}))
        return

    def timeit(fn):
        fn()
        t = []
        for _ in range(a.iters):
            t0 = time.perf_counter()
            fn()
            t.append(time.perf_counter() - t0)
        return round(float(np.median(t)) * 1e3, 3), round(float(np.min(t)) * 1e3, 3), round(float(np.max(t)) * 1e3, 3)

    lines = []
    for f in formats:
        d = {"format": f"{f.encoding} {f.sample_rate}", "audio_s": round(joined / 44100, 1), "rows": 32, "iters": a.iters}
        modes = [("pitch_ms", False, False, True)]
        if has_track:
            modes += [("pitch_tracked_ms", False, True, True)]
        modes += [("pitch_again_ms", False, False, True), ("voice_ms", True, False, False)]
        if has_track:
            modes += [("voice_tracked_ms", True, True, False)]
        for name, v, t, contour in modes:
            med, lo, hi = timeit(lambda: fetch(f, v, t, contour))
            d[name], d[name.replace("_ms", "_min_max_ms")] = med, [lo, hi]
            if name == "pitch_ms":
                d.update(contour_frames=last["nf"], voiced_plain=int((last["f0"] > 0).sum()), cut_frames=int((last["ap"] == 1.0).sum()))
                plain_lag = last["lag"].copy()
            if name == "pitch_tracked_ms":
                d.update(voiced_tracked=int((last["f0"] > 0).sum()), lags_changed=int((last["lag"] != plain_lag).sum()))
        lines.append(json.dumps(d))
    print("\n".join(lines))
    if a.out:
        open(a.out, "w").write("\n".join(lines) + "\n")
    pinned.close(); pipe.close(); bs.close(); vs.close()


if __name__ == "__main__":
    main()
