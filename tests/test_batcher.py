"""batcher.RequestBatcher: the window rule, arrival order, per-request rows / options / noise keys, error isolation, drain, and the rule that a
run is fetched before its execution context is reused: against a fake pipeline on the CPU; on a real tiny pipeline, co-batching independence and
the end-to-end bytes of mixed requests from several threads."""
import io
import random
import struct
import threading
import types

import numpy as np
import pytest

import flac_reader as R
import sbv2_oracle as O
from helpers import blob, make_utts, oracle_noise_w, weights
from sbv2_api_amd import batcher, holder, model, orchestrator, synth

gpu = pytest.mark.gpu
STYLES = np.zeros((2, 4), np.float32)


class FakePipe:
    """Records every call; the PCM of row i of a run is lens[i] samples of the row's tag."""

    def __init__(self, bert=None, vits=None):
        self.log, self.runs, self.batches = [], 0, []

    def prepare(self, utts, **kw):
        b = types.SimpleNamespace(utts=[dict(u) for u in utts], kw=kw, lens=np.array([len(u["phones"]) for u in utts], np.int64), ticket=None)
        self.log.append(("prepare", len(utts)))
        return b

    def run(self, b):
        self.runs += 1
        b.ticket = self.runs
        self.log.append(("run", b.ticket))
        self.batches.append(b)
        if any(u.get("boom") for u in b.utts):
            raise model.Sbv2Error("boom")
        return b.lens

    def fetch(self, b):
        self.log.append(("fetch", b.ticket))
        return [np.full(int(n), u["tag"], np.float32) for n, u in zip(b.lens, b.utts)]

    def fetch_request(self, b, rows, fmt, place, joined_len, gain=None, flac=False):
        self.log.append(("fetch", b.ticket))
        if any(b.utts[r].get("bad_fetch") for r in rows):
            raise model.Sbv2Error("bad fetch")
        t = np.zeros(int(joined_len), np.float32)
        for r, p in zip(rows, place):
            t[p:p + int(b.lens[r])] = b.utts[r]["tag"]
        return t.astype(fmt.dtype), None

    def close(self):
        pass


def _sent(tag, n=3, **extra):
    return dict(phones=[0] * n, tag=float(tag), **extra)


def _tags(wav):
    """The distinct non-zero sample values of a float WAV made by the fake."""
    data = np.frombuffer(wav[wav.index(b"data") + 8:], "<f4")
    return sorted(set(data[data != 0].tolist()))


def _opts(**kw):
    return orchestrator.SynthesizeOptions(**kw)


def _runs(pipe):
    """Per successful or failed run: the tags of its rows, in row order."""
    return [[u["tag"] for u in b.utts] for b in pipe.batches]


def _queued(pipe, requests, **kw):
    """All requests queued before the worker starts, then drained: the window rule without a race."""
    rb = batcher.RequestBatcher(pipe, start=False, clock=lambda: 0.0, max_wait_ms=1000.0, **kw)
    futs = [rb.submit(s, STYLES, options=o, noise_seed=seed) for s, o, seed in requests]
    rb.start()
    rb.close()
    return futs


def test_window_rule_max_utts_keeps_arrival_order_and_never_splits_a_request():
    pipe = FakePipe()
    reqs = [([_sent(1)] * 3, None, 1), ([_sent(2)] * 30, None, 2), ([_sent(3)] * 2, None, 3)]
    futs = _queued(pipe, reqs, max_utts=32)
    assert _runs(pipe) == [[1.0] * 3, [2.0] * 30 + [3.0] * 2]
    assert [_tags(f.result(0)) for f in futs] == [[1.0], [2.0], [3.0]]


def test_window_rule_max_symbols_and_a_lone_oversized_request():
    pipe = FakePipe()
    reqs = [([_sent(1, 40)], None, 1), ([_sent(2, 50)], None, 2), ([_sent(3, 20)], None, 3), ([_sent(4, 500)], None, 4), ([_sent(5, 5)], None, 5)]
    futs = _queued(pipe, reqs, max_symbols=100)
    assert _runs(pipe) == [[1.0, 2.0], [3.0], [4.0], [5.0]]     # 40 + 50 fit, + 20 would not; 500 alone exceeds the limit and runs alone
    assert [_tags(f.result(0)) for f in futs] == [[1.0], [2.0], [3.0], [4.0], [5.0]]
    pipe = FakePipe()
    futs = _queued(pipe, [([_sent(1)] * 40, None, 1), ([_sent(2)], None, 2)], max_utts=32)
    assert _runs(pipe) == [[1.0] * 40, [2.0]]


def test_time_limit_closes_the_run_by_the_injected_clock():
    """The clock is read when the first request is taken and before every further one: 0 ms, 1 ms (inside the 2 ms window), 5 ms (outside)."""
    ticks = iter([0.0, 0.001, 0.005])
    last = [0.005]

    def clock():
        last[0] = next(ticks, last[0] + 1.0)
        return last[0]

    pipe = FakePipe()
    rb = batcher.RequestBatcher(pipe, start=False, clock=clock, max_wait_ms=2.0)
    futs = [rb.submit([_sent(t)], STYLES, noise_seed=t) for t in (1, 2, 3)]
    rb.start()
    rb.close()
    assert _runs(pipe) == [[1.0, 2.0], [3.0]]
    assert all(f.done() for f in futs)


def test_rows_carry_their_requests_options_and_noise_keys():
    pipe = FakePipe()
    reqs = [([_sent(1), None, _sent(1)], _opts(sdp_ratio=0.2, length_scale=1.5), 111), ([_sent(2)] * 3, _opts(sdp_ratio=0.9, length_scale=0.7), 222)]
    _queued(pipe, reqs)
    (b,) = pipe.batches
    assert b.kw == {}     # nothing is a scalar of the run any more
    got = [(u["tag"], u["sdp_ratio"], u["length_scale"], u["noise_scale"], u["noise_scale_w"], u["noise_seed"], u["noise_index"]) for u in b.utts]
    ns, nsw = orchestrator.NOISE_SCALE, orchestrator.NOISE_SCALE_W
    assert got == [(1.0, 0.2, 1.5, ns, nsw, 111, 0), (1.0, 0.2, 1.5, ns, nsw, 111, 1),
                   (2.0, 0.9, 0.7, ns, nsw, 222, 0), (2.0, 0.9, 0.7, ns, nsw, 222, 1), (2.0, 0.9, 0.7, ns, nsw, 222, 2)]


def test_a_failing_request_fails_alone():
    pipe = FakePipe()
    reqs = [([_sent(1)], None, 1), ([_sent(2)], _opts(length_scale=-1.0), 2), ([_sent(3, boom=True)], None, 3), ([None], None, 4),
            ([_sent(5, bad_fetch=True)], _opts(sample_rate=16000, encoding="s16"), 5), ([_sent(6)], None, 6)]
    futs = _queued(pipe, reqs)
    assert _tags(futs[0].result(0)) == [1.0] and _tags(futs[5].result(0)) == [6.0]
    for i, word in ((1, "length_scale"), (2, "boom"), (3, "nothing to synthesize"), (4, "bad fetch")):
        with pytest.raises(model.Sbv2Error, match=word):
            futs[i].result(0)
    assert all(2.0 not in run for run in _runs(pipe))     # refused before it reached a run


def test_close_drains_and_a_closed_batcher_refuses():
    pipe = FakePipe()
    rb = batcher.RequestBatcher(pipe, max_wait_ms=1000.0)
    futs = [rb.submit([_sent(t)], STYLES, noise_seed=t) for t in range(1, 6)]
    rb.close()
    assert [_tags(f.result(0)) for f in futs] == [[float(t)] for t in range(1, 6)]
    with pytest.raises(model.Sbv2Error, match="closed"):
        rb.submit([_sent(9)], STYLES)
    rb = batcher.RequestBatcher(FakePipe(), start=False)
    f = rb.submit([_sent(1)], STYLES)
    rb.close()      # never started: cancelled, not left pending
    assert f.cancelled()


def _assert_fetches_precede_context_reuse(log, depth):
    launched = 0
    for what, k in log:
        if what == "run":
            launched = k
        elif what == "fetch":
            assert launched < k + depth, f"run {k} fetched after run {launched} was launched (depth {depth})"


@pytest.mark.parametrize("depth", [1, 2, 3])
def test_every_fetch_of_a_run_precedes_the_reuse_of_its_context(depth):
    pipe = FakePipe()
    reqs = [([_sent(t, boom=(t == 7))] * (1 + t % 3), _opts(sample_rate=16000, encoding="s16") if t % 2 else None, t) for t in range(1, 15)]
    rb = batcher.RequestBatcher(pipe, start=False, clock=lambda: 0.0, max_wait_ms=1000.0, max_utts=4, depth=depth)
    futs = [rb.submit(s, STYLES, options=o, noise_seed=seed) for s, o, seed in reqs]
    rb.start()
    rb.close()
    assert sum(1 for w, _ in pipe.log if w == "run") >= 5
    _assert_fetches_precede_context_reuse(pipe.log, depth)
    assert all(f.done() for f in futs) and sum(f.exception() is not None for f in futs) == 1


def test_eight_client_threads_get_their_own_audio_within_the_limits():
    pipe = FakePipe()
    rb = batcher.RequestBatcher(pipe, max_utts=8, max_symbols=60, max_wait_ms=0.2)
    results, lock = {}, threading.Lock()

    def client(c):
        rng = random.Random(c)
        for k in range(25):
            tag = 1 + c * 25 + k
            sents = [_sent(tag, rng.randint(1, 12)) for _ in range(rng.randint(1, 4))]
            opts = _opts(sample_rate=16000, encoding="s16") if rng.random() < 0.3 else None
            out = rb.submit(sents, STYLES, options=opts, noise_seed=tag).result(60)
            with lock:
                results[tag] = (out, opts)

    threads = [threading.Thread(target=client, args=(c,)) for c in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    rb.close()
    assert len(results) == 200
    for tag, (out, opts) in results.items():
        if opts is None:
            assert _tags(out) == [float(tag)]
        else:
            data = np.frombuffer(out[44:], "<i2")
            assert set(data[data != 0].tolist()) == {tag}
    for b in pipe.batches:
        single = len({u["noise_seed"] for u in b.utts}) == 1
        assert single or (len(b.utts) <= 8 and int(b.lens.sum()) <= 60)
    _assert_fetches_precede_context_reuse(pipe.log, rb.depth)


class _Session:
    def __init__(self, data, is_bert):
        self.closed = False

    def close(self):
        self.closed = True


def _style_json():
    import json
    return json.dumps({"shape": [2, 4], "data": [[0.0] * 4, [1.0] * 4]}).encode()


def test_holder_keeps_one_batcher_per_model_and_drains_it_on_eviction():
    pipes = []

    def make(bert, vits):
        pipes.append(FakePipe())
        return pipes[-1]

    h = holder.TTSModelHolder(b"bert", max_loaded_models=1, load_session=_Session, make_pipeline=make)
    h.load("a", _style_json(), b"A")
    h.load("b", _style_json(), b"B")
    fa = [h.easy_synthesize_batched("a", [_sent(t)], noise_seed=t, batching=dict(max_wait_ms=1000.0)) for t in (1, 2)]
    ba = h._find("a").batcher
    assert ba is not None and h._find("a").batcher is ba
    fb = h.easy_synthesize_batched("b", [_sent(3)], noise_seed=3)     # loads b: a, the first entry, is evicted, and its batcher drained first
    assert all(f.done() for f in fa) and [_tags(f.result(0)) for f in fa] == [[1.0], [2.0]]
    assert h.models() == ["b"] and len(pipes) == 2
    assert _tags(fb.result(60)) == [3.0]
    h.close()


def test_rest_with_batching_answers_overlapping_requests():
    """Two requests overlap: the first is still waiting for its window when the second arrives (the lock is held only while a request is
    queued), and both come back 200 audio/wav from ONE run."""
    from fastapi.testclient import TestClient
    from sbv2_api_amd import rest
    pipes = []

    def make(bert, vits):
        pipes.append(FakePipe())
        return pipes[-1]

    h = holder.TTSModelHolder(b"bert", parse_text=lambda t: _sent(len(t), len(t)), load_session=_Session, make_pipeline=make)
    h.load("m", _style_json(), b"M")
    c = TestClient(rest.make_app(h, batching=dict(max_utts=2, max_wait_ms=60000.0)), raise_server_exceptions=False)
    out = {}

    def post(text):
        out[text] = c.post("/synthesize", json={"text": text, "ident": "m"})

    threads = [threading.Thread(target=post, args=(t,)) for t in ("ab", "cde")]
    for t in threads:
        t.start()
    for t in threads:
        t.join(120)
    for text, r in out.items():
        assert r.status_code == 200 and r.headers["content-type"] == "audio/wav" and _tags(r.content) == [float(len(text))]
    assert len(out) == 2 and len(pipes[0].batches) == 1      # max_utts = 2 closed the run the moment the second request joined it
    r = c.post("/synthesize", json={"text": "x", "ident": "nope"})
    assert r.status_code == 500 and "model not found" in r.text
    h.close()


def test_rest_batched_synthesize_arrives_while_a_stream_is_being_sent_on_one_event_loop():
    """One app on ONE event loop (the TestClient as a context manager keeps one portal): a stream holds the lock and sends piece after piece
    with the loop's help; a batched /synthesize that arrives in the middle must wait for the lock on a worker thread, never on the loop, or
    the stream could not advance and the server would hang.  The stream goes on only once the second request has reached the app."""
    from fastapi.testclient import TestClient
    from sbv2_api_amd import rest
    arrived = threading.Event()

    class H:
        def models(self):
            return ["m"]

        def easy_synthesize_stream(self, ident, text, style_id, speaker_id, options):
            def pieces():
                yield b"fLaC"
                assert arrived.wait(60)
                for i in range(50):      # every piece needs a turn of the event loop
                    yield bytes([i])
            return pieces()

        def easy_synthesize_batched(self, ident, text, style_id, speaker_id, options, batching=None):
            from concurrent.futures import Future
            f = Future()
            f.set_result(orchestrator.array_to_wav(np.ones((1, 1, 10), np.float32)))
            return f

    app = rest.make_app(H(), batching={})

    async def watched(scope, receive, send):
        if scope["type"] == "http" and scope["path"] == "/synthesize":
            arrived.set()
        await app(scope, receive, send)

    out = {}
    with TestClient(watched, raise_server_exceptions=False) as c:
        def post(path):
            out[path] = c.post(path, json={"text": "abc", "ident": "m", "encoding": "flac" if "stream" in path else "f32"})

        ta = threading.Thread(target=post, args=("/synthesize_stream",))
        ta.start()
        tb = threading.Thread(target=post, args=("/synthesize",))
        tb.start()
        ta.join(120)
        tb.join(120)
        assert not ta.is_alive() and not tb.is_alive(), "the server hangs: the event loop is parked on the lock"
    assert out["/synthesize_stream"].status_code == 200 and out["/synthesize_stream"].content == b"fLaC" + bytes(range(50))
    assert out["/synthesize"].status_code == 200 and out["/synthesize"].headers["content-type"] == "audio/wav"


def test_a_stream_has_the_model_to_itself_while_it_is_open(monkeypatch):
    """A stream runs on the handles that are the pipeline's first execution context.  Opening one pauses the model's batcher: the run that was
    open is launched and every run in flight answered BEFORE the stream begins, nothing is launched while it is open (requests queue), and
    the queue is served once it is closed; a batcher created while a stream is open starts paused."""
    pipes = []

    def make(bert, vits):
        pipes.append(FakePipe())
        return pipes[-1]

    def fake_stream(bert, vits, sentences, *a, **kw):
        pipes[0].log.append(("stream_begin", 0))
        return orchestrator.SynthesisStream(None, b"head", lambda c: c)

    monkeypatch.setattr(orchestrator, "easy_synthesize_stream", fake_stream)
    h = holder.TTSModelHolder(b"bert", load_session=_Session, make_pipeline=make)
    h.load("m", _style_json(), b"M")
    before = h.easy_synthesize_batched("m", [_sent(1)], noise_seed=1, batching=dict(max_wait_ms=5.0))     # in the queue, in its window or launched
    st = h.easy_synthesize_stream("m", [_sent(9)])
    during = h.easy_synthesize_batched("m", [_sent(2)], noise_seed=2)
    st2 = h.easy_synthesize_stream("m", [_sent(9)])     # two streams: both must be closed before the batcher goes on
    assert list(st) == [b"head"]                          # the end of the pieces closes it
    assert not during.done()
    pipes[0].log.append(("streams_closed", 0))
    st2.close()
    st2.close()     # idempotent: resumes once
    assert _tags(during.result(60)) == [2.0] and _tags(before.result(60)) == [1.0]
    log = list(pipes[0].log)
    i0, i1 = log.index(("stream_begin", 0)), log.index(("streams_closed", 0))
    launched = {k for w, k in log[:i0] if w == "run"}
    assert launched == {k for w, k in log[:i0] if w == "fetch"}          # whatever was launched before the stream was answered before it
    assert before.done() == bool(launched) or before.done()
    assert all(w == "stream_begin" for w, _ in log[i0:i1])               # the pipeline is the streams' while they are open
    assert any(w == "run" for w, _ in log[i1:])
    assert h._find("m").streams == 0 and h._find("m").batcher._paused == 0
    h.close()
    # a batcher that is created while a stream is open starts paused
    pipes.clear()
    h = holder.TTSModelHolder(b"bert", load_session=_Session, make_pipeline=make)
    h.load("m", _style_json(), b"M")
    h.easy_synthesize(  # (creates the pipeline the stream's fake logs to)
        "m", [_sent(5)], noise_seed=5)
    st = h.easy_synthesize_stream("m", [_sent(9)])
    f = h.easy_synthesize_batched("m", [_sent(3)], noise_seed=3)
    assert not f.done() and not any(w == "run" for w, _ in pipes[0].log[pipes[0].log.index(("stream_begin", 0)):])
    st.close()
    assert _tags(f.result(60)) == [3.0]
    h.close()


def test_a_failing_worker_fails_the_futures_it_holds():
    class Broken(FakePipe):
        def fetch(self, b):
            raise KeyboardInterrupt     # not an Exception: nothing in the worker's per-request handling catches it

    rb = batcher.RequestBatcher(Broken(), start=False, clock=lambda: 0.0, max_wait_ms=1000.0, max_utts=1)
    futs = [rb.submit([_sent(t)], STYLES, noise_seed=t) for t in (1, 2, 3)]
    rb.start()
    for f in futs:
        with pytest.raises(model.Sbv2Error, match="worker failed"):
            f.result(60)
    with pytest.raises(model.Sbv2Error, match="closed"):
        rb.submit([_sent(9)], STYLES)
    rb.close()


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------------------------

KEYS = ("input_ids", "word2ph", "phones", "tones", "langs")


@pytest.fixture
def tiny(monkeypatch):
    monkeypatch.setenv("SBV2_PIPELINE_DEPTH", "1")     # one execution context: sbv2_vits_fetch_durations reads the last run
    bc, _ = weights("bert", "tiny", 3)
    vc, _ = weights("vits", "tiny", 5)
    bs, vs = model.load_model(blob("bert", "tiny", 3), True), model.load_model(blob("vits", "tiny", 5), False)
    pipe = model.Pipeline(bs, vs)
    yield pipe, vs, bc, vc
    pipe.close(); bs.close(); vs.close()


def _sentences(bc, vc, sizes, seed0):
    return [{k: u[k] for k in KEYS} for u in make_utts(sizes, bc, vc, seed0=seed0, with_bert=False)]


A_SIZES, A_SEED0, A_NOISE = [7, 15], 151, 4242
A_OPTS = dict(sdp_ratio=0.3, length_scale=1.1)


def _a_oracle_margin():
    bc, bw = weights("bert", "tiny", 3)
    vc, vw = weights("vits", "tiny", 5)
    style = orchestrator.get_style_vector(_styles(vc), 1, 1.0)
    worst = 1.0
    for j, s in enumerate(_sentences(bc, vc, A_SIZES, A_SEED0)):
        bert = O.expand_bert_features(O.deberta_forward(bw, bc, s["input_ids"]), s["word2ph"])
        T = len(s["phones"])
        r = O.vits_forward(vw, vc, bert, s["phones"], s["tones"], s["langs"], 0, style, A_OPTS["sdp_ratio"], A_OPTS["length_scale"],
                           noise_w=oracle_noise_w(A_NOISE, j, T, orchestrator.NOISE_SCALE_W), noise_z=None, return_all=True)
        w = np.exp(r["logw"].astype(np.float64)) * A_OPTS["length_scale"]
        worst = min(worst, float(np.abs(w - np.round(w)).min()))
    return worst


def _styles(vc):
    return synth.hash_normal(77, 3 * vc["style_dim"]).reshape(3, -1).astype(np.float32) * 0.1


def test_request_a_is_off_the_ceil_edges_on_the_oracle():
    """request A of the co-batching test has every exp(logw) * length_scale at least 1e-3 away from an integer (oracle, no GPU)."""
    assert _a_oracle_margin() >= 1e-3


def _wav_f32(wav):
    return np.frombuffer(wav[wav.index(b"data") + 8:], "<f4")


@gpu
def test_co_batching_leaves_a_request_as_it_is_alone(tiny):
    """Request A (2 sentences) alone through easy_synthesize with seed s, and behind request B (3 sentences, other options) in one run of the
    batcher: the same integer durations, PCM within the oracle tolerance of the tiny noisy runs (2e-4; DeBERTa's small-grid summation order
    differs between batch sizes, so no bits are asked for)."""
    pipe, vs, bc, vc = tiny
    sa, sb = _sentences(bc, vc, A_SIZES, A_SEED0), _sentences(bc, vc, [4, 22, 9], 171)
    sv = _styles(vc)
    oa, ob = orchestrator.SynthesizeOptions(**A_OPTS), orchestrator.SynthesizeOptions(sdp_ratio=0.8, length_scale=0.9)
    alone = orchestrator.easy_synthesize(pipe, sa, sv, 1, 0, oa, noise_seed=A_NOISE)
    ta = sum(len(s["phones"]) for s in sa)
    d_alone, _ = model.fetch_durations(vs, ta)
    rb = batcher.RequestBatcher(pipe, start=False, max_wait_ms=1000.0)
    fb = rb.submit(sb, sv, 2, 0, ob, noise_seed=99)
    fa = rb.submit(sa, sv, 1, 0, oa, noise_seed=A_NOISE)
    rb.start()
    rb.close()
    tb = sum(len(s["phones"]) for s in sb)
    d_both, _ = model.fetch_durations(vs, ta + tb)
    np.testing.assert_array_equal(d_both[tb:], d_alone)
    x, y = _wav_f32(fa.result(0)), _wav_f32(alone)
    assert x.shape == y.shape
    print(f"[co-batching] request A alone vs behind B: max-abs {float(np.abs(x - y).max()):.3e}")
    np.testing.assert_allclose(x, y, atol=2e-4, rtol=0)
    assert fb.result(0)[:4] == b"RIFF"


class _Recorder:
    """A pipeline proxy that keeps the utterances of every run."""

    def __init__(self, pipe):
        self._pipe, self.runs = pipe, []

    def prepare(self, utts, **kw):
        self.runs.append([dict(u) for u in utts])
        return self._pipe.prepare(utts, **kw)

    def __getattr__(self, name):
        return getattr(self._pipe, name)


@gpu
def test_batcher_end_to_end_on_a_tiny_pipeline(tiny):
    """6 requests from 3 threads, mixed options and encodings: every answer parses, and equals finish_request on the same rows of an identical
    hand-built run (the recorded utterances of the run the request was in, prepared again)."""
    import scipy.io.wavfile as W
    pipe, vs, bc, vc = tiny
    sv = _styles(vc)
    SO = orchestrator.SynthesizeOptions
    specs = [([6, 11], SO()), ([9], SO(sample_rate=24000, encoding="s16", length_scale=1.2)), ([5, 3, 8], SO(encoding="flac", sample_rate=16000, sdp_ratio=0.5)),
             ([12], SO(loudness=-16.0, limiter=True, encoding="s16")), ([7], SO(loudness=-23.0, sample_rate=48000)), ([4, 10], SO(length_scale=0.8))]
    reqs = [(_sentences(bc, vc, sizes, 700 + 10 * i), o, 9000 + i) for i, (sizes, o) in enumerate(specs)]
    rec = _Recorder(pipe)
    rb = batcher.RequestBatcher(rec, max_wait_ms=50.0)
    futs = [None] * 6

    def client(c):
        for i in (2 * c, 2 * c + 1):
            futs[i] = rb.submit(reqs[i][0], sv, 1, 0, reqs[i][1], noise_seed=reqs[i][2])

    threads = [threading.Thread(target=client, args=(c,)) for c in range(3)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    rb.close()
    outs = [f.result(0) for f in futs]
    for (sents, o, seed), out in zip(reqs, outs):
        if o.encoding == "flac":
            d = R.read(out)
            assert d["rate"] == o.sample_rate and len(d["samples"]) > 0
        else:
            rate, data = W.read(io.BytesIO(out))
            assert rate == o.sample_rate and data.dtype == (np.int16 if o.encoding == "s16" else np.float32) and len(data) > 0
        run = next(r for r in rec.runs if any(u["noise_seed"] == seed for u in r))
        r0 = next(i for i, u in enumerate(run) if u["noise_seed"] == seed)
        assert [u["noise_index"] for u in run[r0:r0 + len(sents)]] == list(range(len(sents)))
        b = pipe.prepare(run)
        pipe.run(b)
        want = orchestrator.finish_request(pipe, b, r0, r0 + len(sents), orchestrator.RequestPlan(sents, sv, 1, 0, o))
        assert out == want, (seed, len(out), len(want))
    # ... and independently of finish_request's own bookkeeping: two of the requests against easy_synthesize of the request ALONE (the options and
    # noise keys the batcher put on the rows are then the request's own): same length = same integer durations, samples within 2e-4 (f32) / 7 LSB
    # (s16 at 24 kHz: 2e-4 of full scale, rounded up)
    for i in (0, 1):
        sents, o, seed = reqs[i]
        rate, got = W.read(io.BytesIO(outs[i]))
        _, ref = W.read(io.BytesIO(orchestrator.easy_synthesize(pipe, sents, sv, 1, 0, o, noise_seed=seed)))
        assert got.shape == ref.shape
        tol = 2e-4 if got.dtype == np.float32 else 7
        assert np.abs(got.astype(np.float64) - ref.astype(np.float64)).max() <= tol
