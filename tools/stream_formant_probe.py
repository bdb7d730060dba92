"""The formant contour of a stream on the long-form stream that §8k / §8l / §8n / §8x measure: the full model, 2000 phonemes,
256-frame chunks, one process per section.  Per configuration and kind: time from the begin call to the return of the first next(), and the
time of the whole stream, medians over --runs with the spread beside them; the kinds alternate run by run.
  kind "off": the stream as it was;  "formants": StreamHandle(formants=), next_formants() after every chunk (its cost included).
Configurations (rate:encoding): 16000:s16, 44100:f32, each with a 100 Hz contour of 4 formants at the rate's default window and order.
  python tools/stream_formant_probe.py [--runs 7] [--report profiles/stream_formant_probe.txt] [--tag head]
--other PARENT_BUILD measures the stream WITHOUT a contour and bench.py in this tree and in the parent commit's build beside it, one child
process per measurement, the trees alternating; without a parent build it writes one line that says so.
--pack N (0 = the rule of csrc/formants.h, 1 / 4 forced) runs the fed stage alone (sbv2_debug_stream_formant_contour) for a kernel trace of
its own: a 16 kHz s16 signal as long as the stream, pushed as the stream's replays are (one chunk, then bursts of eight), and the same
with chunks half as long, whose first push completes fewer frames than the device has compute units:
  rocprofv3 --kernel-trace --stats -f rocpd -d DIR -- python tools/stream_formant_probe.py --pack N
--summarise DB reads the rocpd database of such a run (no GPU needed): k_stream_formant's launches per instance and grid with their times."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

CONFIGS = ["16000:s16", "44100:f32"]
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def one(model, bs, vs, u, chunk, fmt, contour):
    kw = dict(formants=model.FormantContour(*contour)) if contour else {}
    t0 = time.perf_counter()
    st = model.StreamHandle(bs, vs, [u], chunk, fmt=fmt, gaps=[0], forced=True, **kw)
    first, samples, chunks, frames = None, 0, 0, 0
    while (c := st.next()) is not None:
        if contour:
            frames += len(st.next_formants()[1])
        chunks += 1
        samples += c.size
        if first is None:
            first = (time.perf_counter() - t0) * 1e3
    total = (time.perf_counter() - t0) * 1e3
    assert not contour or frames == st.n_formant_frames == -(-samples // contour[0]), (frames, samples)
    st.close()
    return first, total, samples, chunks, frames


def summarise(path, emit):
    import sqlite3
    db = sqlite3.connect(path)
    rows = list(db.execute("select name, grid_x / workgroup_x, duration from kernels where name like '%k_stream_formant%'"))
    for key in sorted(set((r[0], r[1]) for r in rows)):
        us = [r[2] / 1e3 for r in rows if (r[0], r[1]) == key]
        emit({"kernel": key[0].replace("void ", "").replace("sbv2::", "").replace("(anonymous namespace)::", "").split("(")[0], "workgroups": key[1],
              "launches": len(us), "us_median": round(statistics.median(us), 2), "us_min": round(min(us), 2), "us_max": round(max(us), 2)})


def other(a, emit):
    """This tree and the parent's build, a child process per measurement, alternating."""
    if not a.other or not os.path.exists(os.path.join(a.other, "sbv2-api_amd", "libsbv2_hip.so")):
        emit({"other": a.other, "note": "no parent build stood beside this tree: the stream without a contour and bench.py were not measured against it"})
        return
    trees = {"parent": os.path.abspath(a.other), "head": HERE}
    rows = {(t, k): [] for t in trees for k in ("stream", "bench")}
    for _ in range(a.rounds):
        for t, root in trees.items():
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--tree", root, "--off-only", "--runs", str(a.runs)], check=True,
                                 capture_output=True, text=True, timeout=600).stdout
            rows[(t, "stream")] += [json.loads(ln) for ln in out.splitlines() if ln.startswith("{")]
            out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"], check=True,
                                 capture_output=True, text=True, timeout=600, cwd=root).stdout
            rows[(t, "bench")].append(json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1]))
    for t in trees:
        for cfg in a.configs.split(","):
            r = [x for x in rows[(t, "stream")] if x["config"] == cfg]
            emit({"tree": t, "config": cfg, "kind": "off", "processes": len(r), "runs_each": a.runs, "first_ms_medians": [x["first_ms_median"] for x in r],
                  "total_ms_medians": [x["total_ms_median"] for x in r]})
        emit({"tree": t, "bench_ms_per_step": [x["ms_per_step"] for x in rows[(t, "bench")]], "bench_value": [x["value"] for x in rows[(t, "bench")]]})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=2, help="--other: processes per tree and measurement")
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--phonemes", type=int, default=2000)
    ap.add_argument("--chunk", type=int, default=256)
    ap.add_argument("--pack", type=int, choices=(0, 1, 4))
    ap.add_argument("--other", metavar="PARENT_BUILD", nargs="?", const="")
    ap.add_argument("--off-only", action="store_true", help="the stream without a contour alone (what --other runs in each tree)")
    ap.add_argument("--report", help="append the result lines to this file")
    ap.add_argument("--tag", default="head", help="what the lines in --report start with")
    ap.add_argument("--tree", default=HERE, help="the checkout whose package is measured")
    ap.add_argument("--summarise", metavar="DB", help="summarise the rocpd database of a traced run instead of running anything")
    a = ap.parse_args()

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        if a.report:
            with open(a.report, "a") as f:
                f.write(f"{a.tag:<12}{line}\n")

    if a.summarise:
        return summarise(a.summarise, emit)
    if a.other is not None:
        return other(a, emit)
    sys.path.insert(0, os.path.abspath(a.tree))
    sys.path.insert(0, os.path.join(os.path.abspath(a.tree), "oracle"))
    import numpy as np
    import sbv2_oracle as O
    from sbv2_api_amd import model, synth
    med = lambda v: round(statistics.median(v), 3)
    if a.pack is not None:
        n = 2600821                                  # the long-form stream's delivered samples at 16 kHz
        x = np.rint(8000.0 * np.random.default_rng(7).uniform(-1.0, 1.0, n)).astype(np.int16)
        for chunk in (a.chunk, a.chunk // 2):
            piece = chunk * 512 * 16000 // 44100     # a chunk's delivered samples; the stream's replays: one chunk, then bursts of eight
            cuts = list(range(piece, n, 8 * piece))
            for _ in range(3):
                fc, _, per = model.debug_stream_formant_contour(x, cuts, 16000, model.FormantContour(160, 4), pack=a.pack)
            emit({"fed_stage": "16000:s16:100Hz:4", "pack": a.pack, "chunk": chunk, "pushes": len(cuts) + 1, "first_push_frames": int(per[0]),
                  "burst_push_frames": int(per[1]), "frames": int(per.sum()), "cap_hit": int((fc.status & 1).sum())})
        return
    has = hasattr(model.StreamHandle, "next_formants") and not a.off_only   # (False on a tree without the feature: the parent commit)
    bc, vc = O.DEBERTA_FULL, O.VITS_FULL
    bs = model.load_model(synth.pack_blob(synth.KIND_BERT, bc, synth.make_deberta_weights(bc, 0x5B72)), True)
    vs = model.load_model(synth.pack_blob(synth.KIND_VITS, vc, synth.make_vits_weights(vc, 0x5B72)), False)
    u = synth.make_utterance(a.phonemes, bc, vc, seed=991)
    for cfg in a.configs.split(","):
        rate, enc = cfg.split(":")
        fmt, contour = model.PcmFormat(int(rate), enc), (int(rate) // 100, 4)
        kinds = {"off": None, "formants": contour} if has else {"off": None}
        for k in kinds.values():      # captures the graphs, grows every buffer and uploads the tables: not measured
            one(model, bs, vs, u, a.chunk, fmt, k)
        rows = {k: [] for k in kinds}
        for _ in range(a.runs):
            for k, s in kinds.items():
                rows[k].append(one(model, bs, vs, u, a.chunk, fmt, s))
        for k, r in rows.items():
            emit({"config": cfg, "kind": k, "runs": a.runs, "chunks": r[0][3], "samples": r[0][2], "frames": r[0][4],
                  "first_ms_median": med(x[0] for x in r), "first_ms_spread": round(max(x[0] for x in r) - min(x[0] for x in r), 3),
                  "total_ms_median": med(x[1] for x in r), "total_ms_spread": round(max(x[1] for x in r) - min(x[1] for x in r), 3)})
    bs.close()
    vs.close()


if __name__ == "__main__":
    main()
