"""The pitch contour of a stream on the long-form stream that §8k / §8l measure: the full model, 2000 phonemes, 256-frame chunks,
s16 at 16 kHz and f32 at 44.1 kHz, a 100 Hz contour over 70 - 600 Hz, one process.  Per format and kind: time from the begin call to the return of
the first next(), and the time of every later call (median / mean per chunk, total), medians over --runs; the kinds alternate run by run.
  kind "off": the stream as it was;  "levels": tokens + a 100 Hz envelope, next_marks() after every chunk (§8l's "on");
  "pitch": the contour alone, next_pitch() after every chunk (its cost included);  "both": levels and pitch.
--tree DIR imports the package from another checkout (the parent commit built beside this one).  A tree without the feature has no
StreamHandle.next_pitch: the script then measures "off" and "levels" only and says so, so that one file run against the parent's tree gives the
parent's figures and their run-to-run spread, which is what "pitch off costs nothing" is read against.
  python tools/stream_pitch_probe.py [--runs 7] [--formats 16000:s16,44100:f32] [--out profiles/stream_pitch_probe.txt] [--tag parent] [--tree DIR]
Every result line is printed and, with --out, appended to that file with --tag in front.
With --trace KIND the script runs ONE stream of that kind per format and nothing else, for a kernel trace of its own:
  rocprofv3 --kernel-trace --stats -d DIR -o both -- python tools/stream_pitch_probe.py --trace both
  python tools/stream_pitch_probe.py --summarise DIR/.../both_results.db --tag trace-both [--out FILE]
--summarise reads the rocpd database of such a run (no GPU needed): the launches in all and those of k_stream_pitch per instance with their
times, grid, registers and LDS (one launch per replay is what the trace of "pitch" must hold, none that of "off")."""
import argparse
import json
import os
import statistics
import sys
import time

KINDS = {"off": (False, False), "levels": (True, False), "pitch": (False, True), "both": (True, True)}


def one(model, bs, vs, u, chunk, fmt, kind):
    levels, pitch = KINDS[kind]
    kw = dict(levels=True, env_hop=fmt.sample_rate // 100) if levels else {}
    if pitch:
        kw["pitch"] = model.Pitch(fmt.sample_rate // 100, 70.0, 600.0)
    t0 = time.perf_counter()
    st = model.StreamHandle(bs, vs, u, chunk, fmt=fmt, forced=True, **kw)
    first, later, samples, chunks, entries, frames = None, [], 0, 0, 0, 0
    t = t0
    while (c := st.next()) is not None:
        if levels:
            m = st.next_marks()
            entries += len(m[1]) + len(m[4])
        if pitch:
            frames += len(st.next_pitch()[1])
        now = time.perf_counter()
        chunks += 1
        samples += c.size
        if first is None:
            first = (now - t0) * 1e3
        else:
            later.append((now - t) * 1e3)
        t = now
    if levels:
        assert entries == st.n_tokens + st.n_env, (entries, st.n_tokens, st.n_env)
    if pitch:
        assert frames == st.n_pitch == -(-samples // (fmt.sample_rate // 100)), (frames, st.n_pitch, samples)
    st.close()
    return first, later, samples, chunks, entries, frames


def summarise(path, emit):
    import collections
    import sqlite3
    if not os.path.exists(path):
        raise SystemExit(f"{path}: no such trace")
    db = sqlite3.connect(path)
    short = lambda n: n.replace("void ", "").replace("sbv2::", "").replace("(anonymous namespace)::", "").split("(")[0]
    names = collections.Counter(short(r[0]) for r in db.execute("select name from kernels"))
    emit({"trace": os.path.basename(path), "launches": sum(names.values()),
          "k_stream_pitch_launches": sum(n for k, n in names.items() if "k_stream_pitch" in k),
          "k_stream_levels_launches": sum(n for k, n in names.items() if "k_stream_levels" in k),
          "copy_fill_launches": {k: n for k, n in names.items() if k.startswith("__amd_rocclr")}})
    rows = list(db.execute("select name, duration, grid_x / workgroup_x, vgpr_count, sgpr_count, lds_size, scratch_size from kernels "
                           "where name like '%k_stream_pitch%' order by start"))
    for name in sorted(set(r[0] for r in rows)):
        r = [x for x in rows if x[0] == name]
        us = [x[1] / 1e3 for x in r]
        emit({"kernel": short(name), "launches": len(r),
              "us_median": round(statistics.median(us), 2), "us_min": round(min(us), 2), "us_max": round(max(us), 2), "us_sum": round(sum(us), 2),
              "workgroups_min": min(x[2] for x in r), "workgroups_max": max(x[2] for x in r), "workgroups_sum": sum(x[2] for x in r),
              "vgpr_count": r[0][3], "sgpr_count": r[0][4], "lds_size": r[0][5], "scratch_size": r[0][6]})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--formats", default="16000:s16,44100:f32")
    ap.add_argument("--phonemes", type=int, default=2000)
    ap.add_argument("--chunk", type=int, default=256)
    ap.add_argument("--trace", choices=list(KINDS), default=None)
    ap.add_argument("--out", help="append the result lines to this file")
    ap.add_argument("--tag", default="head", help="what the lines in --out start with (parent / head)")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the checkout whose package is measured")
    ap.add_argument("--summarise", metavar="DB", help="summarise the rocpd database of a --trace run instead of running anything")
    a = ap.parse_args()

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(f"{a.tag:<12}{line}\n")

    if a.summarise is not None:
        summarise(a.summarise, emit)
        return
    sys.path.insert(0, os.path.abspath(a.tree))
    sys.path.insert(0, os.path.join(os.path.abspath(a.tree), "oracle"))
    import sbv2_oracle as O
    from sbv2_api_amd import model, synth
    has_pitch = hasattr(model.StreamHandle, "next_pitch")   # (False on a tree without the feature: the parent commit)
    bc, vc = O.DEBERTA_FULL, O.VITS_FULL
    bs = model.load_model(synth.pack_blob(synth.KIND_BERT, bc, synth.make_deberta_weights(bc, 0x5B72)), True)
    vs = model.load_model(synth.pack_blob(synth.KIND_VITS, vc, synth.make_vits_weights(vc, 0x5B72)), False)
    u = synth.make_utterance(a.phonemes, bc, vc, seed=991)
    kinds = list(KINDS) if has_pitch else ["off", "levels"]
    for spec in a.formats.split(","):
        rate, enc = spec.split(":")
        fmt = model.PcmFormat(int(rate), enc)
        if a.trace is not None:
            r = one(model, bs, vs, u, a.chunk, fmt, a.trace)
            emit({"trace": a.trace, "rate": fmt.sample_rate, "encoding": enc, "chunks": r[3], "samples": r[2], "entries": r[4], "pitch_frames": r[5]})
            continue
        for kind in kinds:      # captures the graphs and grows every buffer: not measured
            one(model, bs, vs, u, a.chunk, fmt, kind)
        rows = {k: [] for k in kinds}
        for _ in range(a.runs):
            for kind in kinds:
                rows[kind].append(one(model, bs, vs, u, a.chunk, fmt, kind))
        for kind in kinds:
            r = rows[kind]
            totals = [x[0] + sum(x[1]) for x in r]
            emit({"rate": fmt.sample_rate, "encoding": enc, "kind": kind, "tree_has_pitch": has_pitch, "runs": a.runs,
                  "chunks": r[0][3], "samples": r[0][2], "entries": r[0][4], "pitch_frames": r[0][5],
                  "first_ms_median": round(statistics.median(x[0] for x in r), 3), "first_ms_min": round(min(x[0] for x in r), 3),
                  "first_ms_max": round(max(x[0] for x in r), 3), "first_ms_spread": round(max(x[0] for x in r) - min(x[0] for x in r), 3),
                  "later_chunk_ms_median": round(statistics.median(statistics.median(x[1]) for x in r), 4),
                  # (a burst replay delivers 8 chunks at once: most calls only copy, so the mean is the per-chunk cost of the stream)
                  "later_chunk_ms_mean": round(statistics.median(sum(x[1]) / max(len(x[1]), 1) for x in r), 4),
                  "total_ms_median": round(statistics.median(totals), 3), "total_ms_min": round(min(totals), 3),
                  "total_ms_max": round(max(totals), 3), "total_ms_spread": round(max(totals) - min(totals), 3)})
    bs.close()
    vs.close()


if __name__ == "__main__":
    main()
