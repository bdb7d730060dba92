"""The spectrum of a stream on the long-form stream that §8k / §8l / §8n measure: the full model, 2000 phonemes, 256-frame
chunks, one process.  Per configuration and kind: time from the begin call to the return of the first next(), and the time of the whole stream,
medians over --runs with the spread beside them; the kinds alternate run by run.
  kind "off": the stream as it was;  "spectrum": StreamHandle(spectrum=), next_spectrum() after every chunk (its cost included).
Configurations (rate:encoding:n_fft:hop:n_mels): 16000:s16:400:160:80, 44100:f32:2048:441:0, 44100:f32:2048:441:128.
--tree DIR imports the package from another checkout (the parent commit built beside this one); a tree without the feature measures "off"
only and says so: that run gives the parent's figures and their run-to-run spread, which "a stream without a spectrum costs what it did" is
read against.
  python tools/stream_spectrum_probe.py [--runs 7] [--report profiles/stream_spectrum_probe.txt] [--tag parent] [--tree DIR]
--groups measures the work split instead, on the fed stage alone (sbv2_debug_stream_spectrum): a 44.1 kHz f32 signal as long as the stream,
pushed in pieces of a burst replay's size, at n_fft 2048 / hop 441 with 0 and 128 mel bands, with one group and with the rule's count,
alternating; the hook's uploads and copies are the same in both, so the difference of the wall times is the kernels'.
--trace runs ONE stream with a spectrum per configuration and nothing else, for a kernel trace of its own
(rocprofv3 --kernel-trace --stats -d DIR -- python tools/stream_spectrum_probe.py --trace); --groups can be traced the same way.
--summarise DB reads the rocpd database of such a run (no GPU needed): k_stream_spectrum's launches per instance and group count (the grid's
second dimension) with their times."""
import argparse
import json
import os
import statistics
import sys
import time

CONFIGS = ["16000:s16:400:160:80", "44100:f32:2048:441:0", "44100:f32:2048:441:128"]


def one(model, bs, vs, u, chunk, fmt, spectrum):
    kw = dict(spectrum=model.Spectrum(*spectrum)) if spectrum else {}
    t0 = time.perf_counter()
    st = model.StreamHandle(bs, vs, [u], chunk, fmt=fmt, gaps=[0], forced=True, **kw)
    first, samples, chunks, frames = None, 0, 0, 0
    while (c := st.next()) is not None:
        if spectrum:
            frames += len(st.next_spectrum()[1])
        chunks += 1
        samples += c.size
        if first is None:
            first = (time.perf_counter() - t0) * 1e3
    total = (time.perf_counter() - t0) * 1e3
    assert not spectrum or frames == st.n_spec == -(-samples // spectrum[1]), (frames, st.n_spec, samples)
    st.close()
    return first, total, samples, chunks, frames


def summarise(path, emit):
    import sqlite3
    db = sqlite3.connect(path)
    rows = list(db.execute("select name, grid_y / workgroup_y, grid_x / workgroup_x, duration from kernels where name like '%k_stream_spectrum%'"))
    for key in sorted(set((r[0], r[1]) for r in rows)):
        us = [r[3] / 1e3 for r in rows if (r[0], r[1]) == key]
        wg = [r[2] for r in rows if (r[0], r[1]) == key]
        emit({"kernel": key[0].replace("void ", "").replace("sbv2::", "").replace("(anonymous namespace)::", "").split("(")[0], "groups": key[1],
              "launches": len(us), "us_median": round(statistics.median(us), 2), "us_min": round(min(us), 2), "us_max": round(max(us), 2),
              "us_sum": round(sum(us), 2), "grid_x_min": min(wg), "grid_x_max": max(wg)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--phonemes", type=int, default=2000)
    ap.add_argument("--chunk", type=int, default=256)
    ap.add_argument("--groups", action="store_true")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--report", help="append the result lines to this file")
    ap.add_argument("--tag", default="head", help="what the lines in --report start with (parent / head)")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the checkout whose package is measured")
    ap.add_argument("--summarise", metavar="DB", help="summarise the rocpd database of a traced run instead of running anything")
    a = ap.parse_args()

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        if a.report:
            with open(a.report, "a") as f:
                f.write(f"{a.tag:<12}{line}\n")

    if a.summarise:
        summarise(a.summarise, emit)
        return
    sys.path.insert(0, os.path.abspath(a.tree))
    sys.path.insert(0, os.path.join(os.path.abspath(a.tree), "oracle"))
    import numpy as np
    import sbv2_oracle as O
    from sbv2_api_amd import model, synth
    med = lambda v: round(statistics.median(v), 3)
    if a.groups:
        one_chunk = a.chunk * 512                     # the stream's replays: one chunk, then bursts of eight (hop 512)
        n = 7168512
        x = (0.25 * np.random.default_rng(7).uniform(-1.0, 1.0, n)).astype(np.float32)
        cuts = list(range(one_chunk, n, 8 * one_chunk))
        for mels in (0, 128):
            run = lambda g: model.debug_stream_spectrum(x, cuts, 44100, model.Spectrum(2048, 441, mels), groups=g)
            run(1), run(0)
            ms = {1: [], 0: []}
            for _ in range(a.runs):
                for g in (1, 0):
                    t0 = time.perf_counter()
                    run(g)
                    ms[g].append((time.perf_counter() - t0) * 1e3)
            emit({"fed_stage": "44100:f32:2048:441:%d" % mels, "pushes": len(cuts) + 1, "frames": -(-n // 441), "runs": a.runs,
                  "one_group_ms_median": med(ms[1]), "one_group_ms_spread": round(max(ms[1]) - min(ms[1]), 3),
                  "rule_ms_median": med(ms[0]), "rule_ms_spread": round(max(ms[0]) - min(ms[0]), 3)})
        return
    has = hasattr(model.StreamHandle, "next_spectrum")   # (False on a tree without the feature: the parent commit)
    bc, vc = O.DEBERTA_FULL, O.VITS_FULL
    bs = model.load_model(synth.pack_blob(synth.KIND_BERT, bc, synth.make_deberta_weights(bc, 0x5B72)), True)
    vs = model.load_model(synth.pack_blob(synth.KIND_VITS, vc, synth.make_vits_weights(vc, 0x5B72)), False)
    u = synth.make_utterance(a.phonemes, bc, vc, seed=991)
    for cfg in a.configs.split(","):
        rate, enc, n_fft, hop, mels = cfg.split(":")
        fmt, spec = model.PcmFormat(int(rate), enc), (int(n_fft), int(hop), int(mels))
        kinds = {"off": None, "spectrum": spec} if has else {"off": None}
        if a.trace:
            r = one(model, bs, vs, u, a.chunk, fmt, spec)
            emit({"trace": cfg, "chunks": r[3], "samples": r[2], "frames": r[4]})
            continue
        for k in kinds.values():      # captures the graphs, grows every buffer and uploads the tables: not measured
            one(model, bs, vs, u, a.chunk, fmt, k)
        rows = {k: [] for k in kinds}
        for _ in range(a.runs):
            for k, s in kinds.items():
                rows[k].append(one(model, bs, vs, u, a.chunk, fmt, s))
        for k, r in rows.items():
            emit({"config": cfg, "kind": k, "tree_has_spectrum": has, "runs": a.runs, "chunks": r[0][3], "samples": r[0][2], "frames": r[0][4],
                  "first_ms_median": med(x[0] for x in r), "first_ms_spread": round(max(x[0] for x in r) - min(x[0] for x in r), 3),
                  "total_ms_median": med(x[1] for x in r), "total_ms_spread": round(max(x[1] for x in r) - min(x[1] for x in r), 3)})
    bs.close()
    vs.close()


if __name__ == "__main__":
    main()
