"""Builder tool (GPU box): the serving path under load.  N client threads each submit single 128-phoneme utterances back to back for a few
seconds, through the serial-lock path (a lock around orchestrator.easy_synthesize, as rest.py without batching) and through
batcher.RequestBatcher; full-shape synthetic weights, predicted durations, noise on.  Prints one JSON line per (path, N): audio-s/s, median and
p95 latency.  On a tree without batcher.py only the serial path is measured (the parent's numbers).

    python3 tools/batcher_load.py [seconds per case, default 4] [--clients=1,8,32]
"""
import json
import os
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from sbv2_api_amd import configs, model, orchestrator, synth

try:
    from sbv2_api_amd import batcher
except ImportError:
    batcher = None

args = [a for a in sys.argv[1:] if not a.startswith("--")]
SECONDS = float(args[0]) if args else 4.0
CLIENTS = [int(v) for a in sys.argv[1:] if a.startswith("--clients=") for v in a.split("=")[1].split(",")] or [1, 8, 32]
KEYS = ("input_ids", "word2ph", "phones", "tones", "langs")
bc, vc = configs.DEBERTA_FULL, configs.VITS_FULL
bs = model.load_model(synth.pack_blob(synth.KIND_BERT, bc, synth.make_deberta_weights(bc)), True)
vs = model.load_model(synth.pack_blob(synth.KIND_VITS, vc, synth.make_vits_weights(vc)), False)
pipe = model.Pipeline(bs, vs)
styles = synth.hash_normal(77, 2 * vc["style_dim"]).reshape(2, -1).astype(np.float32) * 0.1
sentences = [[{k: synth.make_utterance(128, bc, vc, seed=5000 + i)[k] for k in KEYS}] for i in range(64)]


def load(n_clients, submit):
    """submit(sentences, seed) -> WAV bytes; -> (audio seconds per second, latencies)."""
    lat, audio, lock = [], [0.0], threading.Lock()
    t_end = time.perf_counter() + SECONDS

    def client(c):
        k = 0
        while time.perf_counter() < t_end:
            t0 = time.perf_counter()
            wav = submit(sentences[(c * 7 + k) % len(sentences)], 1000 * c + k)
            dt = time.perf_counter() - t0
            with lock:
                lat.append(dt)
                audio[0] += (len(wav) - 68) / 4 / orchestrator.SAMPLE_RATE
            k += 1

    t0 = time.perf_counter()
    threads = [threading.Thread(target=client, args=(c,)) for c in range(n_clients)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    return audio[0] / (time.perf_counter() - t0), lat


def report(path, n, rate, lat):
    print(json.dumps({"path": path, "clients": n, "audio_s_per_s": round(rate, 1), "requests": len(lat),
                      "latency_ms_median": round(float(np.median(lat)) * 1e3, 2), "latency_ms_p95": round(float(np.percentile(lat, 95)) * 1e3, 2)}), flush=True)


serial_lock = threading.Lock()


def serial(s, seed):
    with serial_lock:
        return orchestrator.easy_synthesize(pipe, s, styles, 1, 0, None, noise_seed=seed)


for _ in range(3):
    serial(sentences[0], 1)
for n in CLIENTS:
    report("serial-lock", n, *load(n, serial))
if batcher is not None:
    rb = batcher.RequestBatcher(pipe)
    for n in CLIENTS:
        report("batched", n, *load(n, lambda s, seed: rb.submit(s, styles, 1, 0, None, noise_seed=seed).result()))
    rb.close()
pipe.close()
bs.close()
vs.close()
