"""Builder tool (GPU box): what the stochastic duration predictor costs a batched run, by the share of rows that use it.

32 utterances of 128 phonemes (the flagship's shapes), full model shapes, forced durations, per-utterance options through sbv2_pipeline_run_opts;
`share` of the rows (every second one at 0.5) carry sdp_ratio 0.3, the others 0.  Each share is timed with the predictor for the rows that need it
(the default: a second text layout when only some do) and with sbv2_debug_set_sdp_all(1) (every row, the full layout), alternating in one process.
A library without the setter (an older build) is timed once per share.  Prints one JSON line.

    python3 tools/sdp_rows_probe.py [runs]
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from sbv2_api_amd import _lib, configs, model, synth

RUNS = int(sys.argv[1]) if len(sys.argv) > 1 else 12
bc, vc = configs.DEBERTA_FULL, configs.VITS_FULL
bs = model.load_model(synth.pack_blob(synth.KIND_BERT, bc, synth.make_deberta_weights(bc)), True)
vs = model.load_model(synth.pack_blob(synth.KIND_VITS, vc, synth.make_vits_weights(vc)), False)
pipe = model.Pipeline(bs, vs)
lib = _lib.lib()
setter = getattr(lib, "sbv2_debug_set_sdp_all", None) if "sbv2_debug_set_sdp_all" in _lib.SYMBOLS else None
utts = [synth.make_utterance(128, bc, vc, seed=100 + i) for i in range(32)]


def timed(b, n):
    ts = []
    for _ in range(n):
        a = time.perf_counter()
        pipe.run(b)
        pipe.sync()
        ts.append((time.perf_counter() - a) * 1e3)
    return ts


out = {"config": "32 x 128 phonemes, full shapes, forced durations, per-utterance options, un-pipelined run + sync", "runs": RUNS, "shares": {}}
for name, needs in (("0", lambda i: False), ("1/32", lambda i: i == 5), ("1/2", lambda i: i % 2 == 1), ("1", lambda i: True)):
    rows = [dict(u, sdp_ratio=0.3 if needs(i) else 0.0, noise_index=i) for i, u in enumerate(utts)]
    b = pipe.prepare(rows, forced=True, noise_scale=0.667, noise_scale_w=0.8, noise_seed=7)
    timed(b, 3)
    res = {"rows": [], "all": []}
    for _ in range(3 if setter else 1):   # alternate the two settings: drift of the clocks hits both alike
        res["rows"] += timed(b, RUNS)
        if setter:
            prev = setter(1)
            timed(b, 1)
            res["all"] += timed(b, RUNS)
            setter(prev)
            timed(b, 1)
    out["shares"][name] = {k: {"median_ms": round(float(np.median(v)), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)} for k, v in res.items() if v}
print(json.dumps(out), flush=True)
