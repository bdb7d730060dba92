"""FLAC on a stream (csrc/flac_encode.hip FlacStreamEncoder, sbv2_stream_begin_flac / _next_flac, POST /synthesize_stream): the encoder fed
piece by piece gives, for any way of cutting a signal into pushes, the frames of the one-shot encoder; a synthesis stream delivers them as its
chunks complete 4096-sample blocks.  Everything on the device side is equality: the frame bytes are a function of (samples, frame number, rate).
CPU tests run anywhere; GPU tests (@pytest.mark.gpu) need an MI355X."""
import ctypes
import io

import numpy as np
import pytest

import flac_reader as R
from helpers import blob, make_utts, weights
from sbv2_api_amd import _lib, model, orchestrator, synth

RATES = (8000, 16000, 22050, 24000, 32000, 44100, 48000)


def stream_bound(n):
    """42 + 16 ceil((n + 4095) / 4096) + 2 (n + 4095): the header, then a carried tail of up to 4095 samples and n new ones at the VERBATIM bound."""
    return 42 + 16 * (-(-(n + 4095) // 4096)) + 2 * (n + 4095)


# ---- CPU ----------------------------------------------------------------------------------------------------------------------------------

def test_abi_exports_and_stream_bound_values():
    l = _lib.lib()
    for name in ("sbv2_flac_stream_bound", "sbv2_stream_begin_flac", "sbv2_stream_next_flac", "sbv2_debug_flac_stream_encode"):
        assert hasattr(l, name), name
    for r in RATES:
        f = model.PcmFormat(r, "s16")
        for n in (0, 1, 16 * 512, 4095, 4096, 4097, 256 * 512, 10 ** 6):
            assert model.flac_stream_bound(f, n) == stream_bound(model.pcm_format_length(f, n)), (r, n)
    assert model.flac_stream_bound(model.PcmFormat(8000, "s16"), 16 * 512) == 42 + 32 + 2 * (1487 + 4095)
    assert l.sbv2_flac_stream_bound(_lib.Sbv2PcmFormat(44100, 0, 0, 0), 100) == -1
    assert b"s16" in l.sbv2_last_error()
    assert l.sbv2_flac_stream_bound(_lib.Sbv2PcmFormat(44100, 1, 1, 0), 100) == -1
    assert b"normali" in l.sbv2_last_error()
    assert l.sbv2_flac_stream_bound(_lib.Sbv2PcmFormat(11025, 1, 0, 0), 100) == -1
    assert b"sample rate" in l.sbv2_last_error()
    with pytest.raises(model.Sbv2Error, match="s16"):
        model.flac_stream_bound(model.PcmFormat(16000, "f32"), 10)


def test_rest_synthesize_stream_reaches_holder_and_streams_in_order():
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient
    from sbv2_api_amd import rest

    class Holder:
        def __init__(self):
            self.opts, self.whole = [], []

        def models(self):
            return ["m"]

        def easy_synthesize(self, ident, text, style_id, speaker_id, options):
            self.whole.append(options)
            return b"fLaC" if options.encoding == "flac" else b"RIFF"

        def easy_synthesize_stream(self, ident, text, style_id, speaker_id, options):
            self.opts.append((ident, text, style_id, speaker_id, options))
            # (the real one refuses these before it returns its generator: orchestrator.easy_synthesize_stream)
            if options.normalize or options.loudness is not None or options.limiter:
                raise model.Sbv2Error("needs the whole signal")
            head = b"fLaC" if options.encoding == "flac" else b"RIFF"
            return iter([head, b"one", b"two", b"three"])

    h = Holder()
    c = TestClient(rest.make_app(h))
    r = c.post("/synthesize_stream", json={"text": "a\nb", "ident": "m", "encoding": "flac", "sample_rate": 16000, "style_id": 2, "speaker_id": 1,
                                           "sdp_ratio": 0.25, "length_scale": 1.5})
    assert r.status_code == 200 and r.headers["content-type"] == "audio/flac" and r.content == b"fLaConetwothree"
    ident, text, style_id, speaker_id, o = h.opts[-1]
    assert (ident, text, style_id, speaker_id) == ("m", "a\nb", 2, 1)
    assert (o.encoding, o.sample_rate, o.sdp_ratio, o.length_scale, o.normalize, o.loudness, o.limiter) == ("flac", 16000, 0.25, 1.5, False, None, False)
    r = c.post("/synthesize_stream", json={"text": "a", "ident": "m", "encoding": "s16"})
    assert r.status_code == 200 and r.headers["content-type"] == "audio/wav" and r.content == b"RIFFonetwothree"
    for extra in ({"loudness": -23.0}, {"normalize": True}, {"loudness": -16.0, "limiter": True}):
        r = c.post("/synthesize_stream", json={"text": "a", "ident": "m", "encoding": "flac", **extra})
        assert r.status_code == 500 and r.text == "Something went wrong: needs the whole signal", extra
    # the lock was given back after the refusals and after the streams: the plain routes still answer, unchanged
    r = c.post("/synthesize", json={"text": "a", "ident": "m", "encoding": "flac", "sample_rate": 16000})
    assert r.status_code == 200 and r.headers["content-type"] == "audio/flac" and r.content == b"fLaC"
    assert (h.whole[-1].encoding, h.whole[-1].sample_rate) == ("flac", 16000)
    r = c.post("/synthesize", json={"text": "a", "ident": "m"})
    assert r.status_code == 200 and r.headers["content-type"] == "audio/wav" and r.content == b"RIFF"
    assert c.get("/models").json() == ["m"]


class _Pieces:
    """A stub of orchestrator.SynthesisStream: an iterator with close() that records what happened to it."""

    def __init__(self, items):
        self.items, self.asked, self.closed = list(items), 0, 0

    def __iter__(self):
        return self

    def __next__(self):
        self.asked += 1
        if self.closed or not self.items:
            raise StopIteration
        return self.items.pop(0)

    def close(self):
        self.closed += 1


def _answers_in_time(client, path, seconds=5.0):
    """GET path on a worker thread: its JSON, or None when no answer came in time (a lock that was never given back)."""
    import threading
    out = []
    t = threading.Thread(target=lambda: out.append(client.get(path).json()), daemon=True)
    t.start()
    t.join(seconds)
    return out[0] if out else None


def test_rest_synthesize_stream_gives_the_lock_back_when_the_client_goes_away():
    """A client that hangs up while the holder is still working on its request (DeBERTa + flow of a long text) leaves a response whose body is
    never asked for.  The lock and the stream must be given back all the same: the other routes answer, the pieces were closed."""
    pytest.importorskip("fastapi")
    import asyncio
    import json
    from fastapi.testclient import TestClient
    from sbv2_api_amd import rest

    class Holder:
        def __init__(self):
            self.streams = []

        def models(self):
            return ["m"]

        def easy_synthesize_stream(self, ident, text, style_id, speaker_id, options):
            self.streams.append(_Pieces([b"fLaC", b"one", b"two"]))
            return self.streams[-1]

    h = Holder()
    app = rest.make_app(h)
    body = json.dumps({"text": "a", "ident": "m", "encoding": "flac"}).encode()

    def drive(asgi, send_fails):
        """One POST /synthesize_stream as a raw ASGI call whose client is gone once the request body has been read."""
        scope = {"type": "http", "http_version": "1.1", "method": "POST", "path": "/synthesize_stream", "raw_path": b"/synthesize_stream",
                 "root_path": "", "scheme": "http", "query_string": b"", "server": ("test", 80), "client": ("test", 1),
                 "headers": [(b"content-type", b"application/json"), (b"content-length", str(len(body)).encode())]}
        if asgi:
            scope["asgi"] = asgi
        inbox = [{"type": "http.request", "body": body, "more_body": False}]
        sent = []

        async def receive():
            return inbox.pop(0) if inbox else {"type": "http.disconnect"}

        async def send(message):
            if send_fails and message["type"] == "http.response.body":
                raise OSError("client gone")       # ASGI >= 2.4: a send after the disconnect fails
            sent.append(message["type"])

        async def run():
            try:
                await asyncio.wait_for(app(scope, receive, send), 20)
            except Exception:
                pass                                # (a disconnect may surface as an exception of the server's: not the point here)
        asyncio.run(run())
        return sent

    client = TestClient(app)
    for asgi, send_fails in ((None, False), ({"version": "3.0", "spec_version": "2.4"}, True)):
        sent = drive(asgi, send_fails)
        assert sent[:1] == ["http.response.start"] and sent.count("http.response.body") < 4, sent   # (the answer began and was never finished)
        st = h.streams[-1]
        assert st.closed == 1, (asgi, st.closed, st.asked)
        assert _answers_in_time(client, "/models") == ["m"], f"the holder's lock was not given back (asgi = {asgi})"
    # the control: a client that stays gets every piece, the pieces are closed once, and the lock is free again
    r = client.post("/synthesize_stream", json={"text": "a", "ident": "m", "encoding": "flac"})
    assert r.status_code == 200 and r.content == b"fLaConetwo" and h.streams[-1].closed == 1
    assert _answers_in_time(client, "/models") == ["m"]


def test_synthesis_stream_closes_its_handle_however_it_ends():
    class Handle:
        def __init__(self, chunks, fail_at=None):
            self.chunks, self.fail_at, self.closed, self.calls = list(chunks), fail_at, 0, 0

        def next(self):
            self.calls += 1
            if self.calls == self.fail_at:
                raise model.Sbv2Error("boom")
            return self.chunks.pop(0) if self.chunks else None

        def close(self):
            self.closed += 1

    # to the end: header first, empty chunks skipped, closed once
    st = Handle([b"a", b"", b"b"])
    assert list(orchestrator.SynthesisStream(st, b"H", lambda c: c.upper())) == [b"H", b"A", b"B"] and st.closed == 1
    # dropped without a single next, and dropped half way
    st = Handle([b"a"])
    s = orchestrator.SynthesisStream(st, None, lambda c: c)
    del s
    assert st.closed == 1 and st.calls == 0
    st = Handle([b"a", b"b"])
    s = orchestrator.SynthesisStream(st, None, lambda c: c)
    assert next(s) == b"a"
    s.close()
    s.close()
    assert st.closed == 1 and list(s) == []
    # a failing chunk closes it too
    st = Handle([b"a", b"b"], fail_at=2)
    s = orchestrator.SynthesisStream(st, None, lambda c: c)
    assert next(s) == b"a"
    with pytest.raises(model.Sbv2Error, match="boom"):
        next(s)
    assert st.closed == 1


def test_stream_options_that_need_the_whole_signal_are_refused_before_any_gpu_work():
    styles = np.zeros((2, 4), np.float32)
    for opts, why in ((orchestrator.SynthesizeOptions(normalize=True), "whole signal"),
                      (orchestrator.SynthesizeOptions(loudness=-23.0), "whole signal"),
                      (orchestrator.SynthesizeOptions(loudness=-16.0, limiter=True), "whole signal")):
        with pytest.raises(model.Sbv2Error, match=why):
            orchestrator.easy_synthesize_stream(None, None, [{"x": 1}], styles, 0, 0, opts)
    with pytest.raises(model.Sbv2Error, match="one utterance"):
        orchestrator.easy_synthesize_stream(None, None, [{"x": 1}, None, {"x": 2}], styles, 0, 0, None, noise_seed=1)
    with pytest.raises(model.Sbv2Error, match="nothing to synthesize"):
        orchestrator.easy_synthesize_stream(None, None, [None], styles, 0, 0, None, noise_seed=1)


def test_wav_stream_header_names_the_right_byte_counts():
    import scipy.io.wavfile as W
    rng = np.random.default_rng(3)
    for rate, n in ((16000, 12345), (44100, 1), (8000, 0)):
        x = rng.integers(-32768, 32768, n).astype(np.int16)
        head = orchestrator.wav_stream_header(rate, "s16", n)
        assert len(head) == 44 and head + x.tobytes() == orchestrator.pcm16_wav(x, rate)
        if n:
            got_rate, y = W.read(io.BytesIO(head + x.astype("<i2").tobytes()))
            assert got_rate == rate and y.dtype == np.int16
            np.testing.assert_array_equal(y, x)
        assert int.from_bytes(head[4:8], "little") == 36 + 2 * n and int.from_bytes(head[40:44], "little") == 2 * n
    x = rng.normal(0, 0.1, 777).astype(np.float32)
    head = orchestrator.wav_stream_header(48000, "f32", x.size)
    assert head + x.tobytes() == orchestrator.float_wav(x, 48000)
    got_rate, y = W.read(io.BytesIO(head + x.tobytes()))
    assert got_rate == 48000 and y.dtype == np.float32
    np.testing.assert_array_equal(y, x)


# ---- GPU: the fed encoder on its own ---------------------------------------------------------------------------------------------------------

def speech_like(n, rate=44100, seed=77):
    """Voiced bursts (a gliding f0 with 1/k harmonics) between near-silent gaps, -60 dBFS noise: blocks of every kind the encoder tells apart."""
    rng = np.random.default_rng(seed)
    if n == 0:
        return np.zeros(0, np.int16)
    t = np.arange(n) / rate
    f0 = 130 + 30 * np.sin(2 * np.pi * 0.9 * t)
    ph = 2 * np.pi * np.cumsum(f0) / rate
    y = sum(np.sin(k * ph) / k for k in range(1, 12))
    env = np.clip(np.sin(2 * np.pi * 1.7 * t), 0, None) ** 2
    y = 0.6 * y / max(np.abs(y).max(), 1e-9) * env + rng.normal(0, 1e-3, n)
    return np.rint(np.clip(y, -1, 1) * 32767).astype(np.int16)


def edge_signals():
    """The signals of test_flac.test_debug_encode_round_trips_edge_signals (restated: they are built inside that test)."""
    rng = np.random.default_rng(11)
    sigs = []
    for n in (0, 1, 15, 4095, 4096, 4097, 3 * 4096 + 17):
        sigs.append(np.zeros(n, np.int16))
        sigs.append(np.full(n, -1234, np.int16))
        sigs.append(np.where((np.arange(n) // 37) % 2, 32767, -32767).astype(np.int16))
        sigs.append(rng.integers(-32768, 32768, n).astype(np.int16))
        sigs.append(np.rint(8000 * np.sin(np.arange(n) * 0.05) + rng.normal(0, 30, n)).astype(np.int16))
    return sigs


def check_fed_stream(parts, cuts, x, rate, one_shot, decoded=None):
    """The contract of the fed encoder for one signal and one set of cuts.  decoded: streams already read, by their bytes (every set of cuts
    must give the same bytes, and reading them again would tell nothing new)."""
    x = np.asarray(x, np.int16)
    data = b"".join(parts)
    assert len(parts) == len(cuts) + 1
    assert sum(len(p) for p in parts) == len(data)
    assert data[12:18] == bytes(6), "STREAMINFO min / max frame size of a fed stream must be 0 (unknown)"
    assert data[:12] == one_shot[:12] and data[18:] == one_shot[18:], "the fed stream differs from the one-shot stream outside bytes 12..17"
    got = decoded[data] if decoded is not None and data in decoded else R.read(data)
    if decoded is not None:
        decoded[data] = got
    np.testing.assert_array_equal(got["samples"], x)
    assert got["rate"] == rate and got["total"] == x.size and (got["min_block"], got["max_block"]) == (4096, 4096)
    assert (got["min_frame"], got["max_frame"]) == (0, 0) and got["md5"] == bytes(16)
    assert [f["number"] for f in got["frames"]] == list(range(-(-x.size // 4096)))
    # every push delivers exactly the frames its samples complete: the sizes follow from the sample counts and the decoded frame sizes
    sizes = [f["size"] for f in got["frames"]]
    edges = [0] + [int(c) for c in cuts] + [x.size]
    done = 0
    for i, p in enumerate(parts):
        upto = -(-x.size // 4096) if i == len(parts) - 1 else edges[i + 1] // 4096
        want = sum(sizes[done:upto]) + (42 if i == 0 else 0)
        assert len(p) == want, (i, len(p), want)
        if upto == done:
            assert len(p) == (42 if i == 0 else 0)
        done = upto
    assert done == len(sizes)


def cut_sets(n, rng):
    sets = [[], list(range(4096, n, 4096)), list(range(1000, n, 1000)), [c for c in (1, 2, 3) if c <= n]]
    if n >= 1:
        sets.append([n - 1])
    for _ in range(20):
        k = int(rng.integers(0, 12))
        c = np.sort(rng.integers(0, n + 1, k))
        if k >= 2 and rng.random() < 0.5:
            c[int(rng.integers(1, k))] = c[0]      # repeated positions: empty pushes in the middle ...
            c = np.sort(c)
        if k and rng.random() < 0.3:
            c[-1] = n                              # ... and an empty last push
        sets.append([int(v) for v in c])
    return sets


@pytest.mark.gpu
def test_fed_encoder_is_invariant_to_the_cuts():
    rng = np.random.default_rng(2025)
    sigs = edge_signals() + [speech_like(100_000)]
    for n in (0, 1, 4095, 4096, 4097, 3 * 4096):
        sigs.append(speech_like(n, seed=n + 1))
    shots = model.debug_flac_encode(sigs, 44100)
    checked = 0
    for x, one_shot in zip(sigs, shots):
        decoded = {}
        for cuts in cut_sets(x.size, rng):
            parts = model.debug_flac_stream_encode(x, cuts, 44100)
            check_fed_stream(parts, cuts, x, 44100, one_shot, decoded)
            checked += 1
        assert len(decoded) == 1
    assert checked >= len(sigs) * 24
    # the same samples and the same cuts: the same bytes
    x = sigs[35]
    cuts = [5, 5, 4096, 9000, x.size]
    assert model.debug_flac_stream_encode(x, cuts, 44100) == model.debug_flac_stream_encode(x, cuts, 44100)


@pytest.mark.gpu
def test_fed_encoder_every_rate():
    for r in RATES:
        x = speech_like(r // 2 + 13, rate=r, seed=r)
        one_shot = model.debug_flac_encode([x], r)[0]
        cuts = sorted(min(c, x.size) for c in (700, 4096, 4097, 9000, 9000, x.size - 1))
        check_fed_stream(model.debug_flac_stream_encode(x, cuts, r), cuts, x, r, one_shot)
    with pytest.raises(model.Sbv2Error, match="sample rate"):
        model.debug_flac_stream_encode(np.zeros(10, np.int16), [], 11025)
    with pytest.raises(model.Sbv2Error, match="ascend"):
        model.debug_flac_stream_encode(np.zeros(10, np.int16), [5, 4], 8000)


# ---- GPU: the synthesis stream -----------------------------------------------------------------------------------------------------------------

def _tiny():
    bc, _ = weights("bert", "tiny", 3)
    vc, _ = weights("vits", "tiny", 5)
    return bc, vc, model.load_model(blob("bert", "tiny", 3), True), model.load_model(blob("vits", "tiny", 5), False)


def _hop(vs):
    return _lib.lib().sbv2_vits_hop(vs.handle)


def _formatted_chunks(bs, vs, u, chunk, fmt, **kw):
    st = model.StreamHandle(bs, vs, u, chunk, fmt=fmt, **kw)
    parts = []
    while (c := st.next()) is not None:
        parts.append(c)
    total = st.total_samples
    st.close()
    return parts, total


def _flac_calls(bs, vs, u, chunk, fmt, **kw):
    """[(bytes, samples consumed)] per sbv2_stream_next_flac call that consumed samples, and total_samples."""
    l = _lib.lib()
    st = model.StreamHandle(bs, vs, u, chunk, fmt=fmt, flac=True, **kw)
    assert st.buf.nbytes == model.flac_stream_bound(fmt, chunk * _hop(vs))
    calls = []
    nb, ns = ctypes.c_int64(), ctypes.c_int64()
    while True:
        _lib.check(l.sbv2_stream_next_flac(st.h, st.buf.ctypes.data, st.buf.nbytes, ctypes.byref(nb), ctypes.byref(ns)))
        if ns.value == 0:
            assert nb.value == 0
            break
        calls.append((st.buf[:nb.value].tobytes(), ns.value))
    # the end marker repeats
    _lib.check(l.sbv2_stream_next_flac(st.h, st.buf.ctypes.data, st.buf.nbytes, ctypes.byref(nb), ctypes.byref(ns)))
    assert (nb.value, ns.value) == (0, 0)
    total = st.total_samples
    st.close()
    return calls, total


def check_stream_contract(bs, vs, u, chunk, fmt, **kw):
    """Section 2 of the feature's contract for one utterance / chunk size / format; returns the per-call byte counts."""
    hop = _hop(vs)
    pcm, total = _formatted_chunks(bs, vs, u, chunk, fmt, **kw)
    calls, total_f = _flac_calls(bs, vs, u, chunk, fmt, **kw)
    x = np.concatenate(pcm)
    assert total == total_f == x.size and x.dtype == np.int16
    # the formatted stream's own convention: chunk c of native samples [a, b) emits output samples [ceil(a L / M), ceil(b L / M))
    plain = model.StreamHandle(bs, vs, u, chunk, **kw)
    frames = plain.total_samples // hop
    plain.close()
    assert plain.total_samples == frames * hop and total == model.pcm_format_length(fmt, frames * hop)
    edges = [model.pcm_format_length(fmt, min(c * chunk, frames) * hop) for c in range(-(-frames // chunk) + 1)]
    assert [p.size for p in pcm] == list(np.diff(edges)), "the formatted stream's chunk sizes"
    assert [n for _, n in calls] == [p.size for p in pcm], "n_samples per call must equal the formatted stream's chunk"
    data = b"".join(b for b, _ in calls)
    got = R.read(data)                                  # CRCs, consecutive frame numbers, STREAMINFO total == decoded count
    np.testing.assert_array_equal(got["samples"], x)
    assert got["rate"] == fmt.sample_rate and got["total"] == x.size and (got["min_frame"], got["max_frame"]) == (0, 0)
    one_shot = model.debug_flac_encode([x], fmt.sample_rate)[0]
    assert data[12:18] == bytes(6) and data[:12] == one_shot[:12] and data[18:] == one_shot[18:]
    # each call holds the frames its samples complete
    sizes = [f["size"] for f in got["frames"]]
    done = 0
    for i, (b, _) in enumerate(calls):
        upto = len(sizes) if i == len(calls) - 1 else edges[i + 1] // 4096
        assert len(b) == sum(sizes[done:upto]) + (42 if i == 0 else 0), (i, len(b))
        assert len(b) <= model.flac_stream_bound(fmt, chunk * hop)
        done = upto
    # run twice: identical bytes
    again, _ = _flac_calls(bs, vs, u, chunk, fmt, **kw)
    assert again == calls
    return x, [len(b) for b, _ in calls]


@pytest.mark.gpu
def test_flac_stream_contract_tiny():
    """The tiny decoder (hop 16, halo ~70 exact samples: the 44.1 / 48 / 24 kHz filters fit, see test_pcm_format) with utterances long
    enough for the burst plan (more than 2 chunks) whose lengths do not end on a block edge; predicted durations and noise once."""
    bc, vc, bs, vs = _tiny()
    for n, kw in ((700, dict(forced=True)), (500, dict(sdp_ratio=0.2, noise_scale=0.667, noise_scale_w=0.8, noise_seed=5))):
        u = make_utts([n], bc, vc, seed0=300 + n, with_bert=False)[0]
        for rate in (44100, 48000, 24000):
            for chunk in (16, 64):
                x, nbytes = check_stream_contract(bs, vs, u, chunk, model.PcmFormat(rate, "s16"), **kw)
                assert len(nbytes) > 2 and x.size % 4096 != 0, (n, rate, chunk, len(nbytes), x.size)
                assert x.size > 4096, "the utterance must span several FLAC frames"
                # 16- and 64-frame chunks of this decoder are <= 1115 samples: most calls complete no frame
                assert any(b == 0 for b in nbytes[1:]) and nbytes[0] >= 42
    bs.close(); vs.close()


@pytest.fixture(scope="module")
def full_models():
    bs, vs = model.load_model(blob("bert", "full"), True), model.load_model(blob("vits", "full"), False)
    yield weights("bert", "full")[0], weights("vits", "full")[0], bs, vs
    bs.close(); vs.close()


@pytest.mark.gpu
def test_flac_stream_contract_full_model_44k_16k_8k(full_models):
    """The full-size decoder (hop 512), whose halo holds the 16 and 8 kHz filters (the tiny one's does not): 44 100, 16 000 and 8 000 Hz,
    16- and 64-frame chunks.  At 8 kHz a 16-frame chunk is 1486 or 1487 samples: calls that consume samples and deliver no byte."""
    bc, vc, bs, vs = full_models
    assert _hop(vs) == 512
    u = synth.make_utterance(60, bc, vc, seed=91)
    for rate in (44100, 16000, 8000):
        for chunk in (16, 64):
            x, nbytes = check_stream_contract(bs, vs, u, chunk, model.PcmFormat(rate, "s16"), forced=True)
            assert len(nbytes) > 2 and x.size % 4096 != 0, (rate, chunk, len(nbytes), x.size)
            if (rate, chunk) == (8000, 16):
                assert sum(1 for b in nbytes[1:] if b == 0) >= 1 and nbytes[0] == 42


@pytest.mark.gpu
def test_flac_stream_refusals_and_retry_with_more_room():
    bc, vc, bs, vs = _tiny()
    l = _lib.lib()
    u = make_utts([700], bc, vc, seed0=500, with_bert=False)[0]
    with pytest.raises(model.Sbv2Error, match="s16"):
        model.StreamHandle(bs, vs, u, 64, fmt=model.PcmFormat(48000, "f32"), flac=True, forced=True)
    with pytest.raises(model.Sbv2Error, match="normali"):
        model.StreamHandle(bs, vs, u, 64, fmt=model.PcmFormat(48000, "s16", True), flac=True, forced=True)
    with pytest.raises(model.Sbv2Error, match="halo"):      # the halo check of the formatted stream applies unchanged
        model.StreamHandle(bs, vs, u, 64, fmt=model.PcmFormat(16000, "s16"), flac=True, forced=True)
    with pytest.raises(model.Sbv2Error, match="format"):
        model.StreamHandle(bs, vs, u, 64, flac=True, forced=True)
    fmt = model.PcmFormat(48000, "s16")
    pcm, total = _formatted_chunks(bs, vs, u, 64, fmt, forced=True)
    x = np.concatenate(pcm)
    # the other two ways of taking chunks are refused on a FLAC stream ...
    st = model.StreamHandle(bs, vs, u, 64, fmt=fmt, flac=True, forced=True)
    n, nb = ctypes.c_int64(), ctypes.c_int64()
    assert l.sbv2_stream_next_format(st.h, st.buf.ctypes.data, st.buf.nbytes, ctypes.byref(n)) != 0
    assert b"sbv2_stream_next_flac" in l.sbv2_last_error()
    assert l.sbv2_stream_next(st.h, st.buf.ctypes.data, st.buf.nbytes // 4, ctypes.byref(n)) != 0
    assert b"sbv2_stream_next_flac" in l.sbv2_last_error()
    # ... and nothing was consumed by them.  Too small a capacity: refused, nothing written, the call can be repeated with the bound
    parts = []
    small = np.full(41, 0xA5, np.uint8)
    refused = 0
    while True:
        rc = l.sbv2_stream_next_flac(st.h, small.ctypes.data, small.nbytes, ctypes.byref(nb), ctypes.byref(n))
        if rc != 0:
            assert b"too small" in l.sbv2_last_error() and (small == 0xA5).all()
            refused += 1
            _lib.check(l.sbv2_stream_next_flac(st.h, st.buf.ctypes.data, st.buf.nbytes, ctypes.byref(nb), ctypes.byref(n)))
            parts.append(st.buf[:nb.value].tobytes())
        else:
            if n.value == 0:
                break
            assert nb.value <= small.nbytes
            parts.append(small[:nb.value].tobytes())
            small[:] = 0xA5
    st.close()
    assert refused >= 2                                   # the header call and every call that completed a frame
    data = b"".join(parts)
    np.testing.assert_array_equal(R.read(data)["samples"], x)
    one_shot = model.debug_flac_encode([x], 48000)[0]
    assert data[:12] == one_shot[:12] and data[18:] == one_shot[18:]
    # _next_flac on the other kinds of stream
    for kw in (dict(fmt=fmt), dict()):
        st = model.StreamHandle(bs, vs, u, 64, forced=True, **kw)
        buf = np.empty(1 << 16, np.uint8)
        assert l.sbv2_stream_next_flac(st.h, buf.ctypes.data, buf.nbytes, ctypes.byref(nb), ctypes.byref(n)) != 0
        assert b"not begun as FLAC" in l.sbv2_last_error()
        st.close()
    bs.close(); vs.close()


@pytest.mark.gpu
def test_flac_stream_long_form_full_shapes(full_models):
    """The 2000-phoneme long-form input of test_config4_streaming_long_form_full_shapes at 44.1 kHz in 256-frame chunks: a valid stream that
    decodes to the formatted stream's samples."""
    bc, vc, bs, vs = full_models
    u = synth.make_utterance(2000, bc, vc, seed=991)
    fmt = model.PcmFormat(44100, "s16")
    pcm, total = _formatted_chunks(bs, vs, u, 256, fmt, forced=True)
    x = np.concatenate(pcm)
    assert total == x.size == 512 * 14001 and len(pcm) == 55
    pieces = list(model.stream_synthesize(bs, vs, u, 256, fmt=fmt, flac=True, forced=True))
    assert len(pieces) == 55 and all(isinstance(p, bytes) and len(p) <= model.flac_stream_bound(fmt, 256 * 512) for p in pieces)
    data = b"".join(pieces)
    got = R.read(data)
    np.testing.assert_array_equal(got["samples"], x)
    assert got["total"] == x.size and len(got["frames"]) == -(-x.size // 4096)
    print(f"long form: {x.size} samples, s16 {2 * x.size} bytes, FLAC stream {len(data)} bytes ({len(data) / (2 * x.size):.3f})")
    assert len(data) < 2 * x.size


@pytest.mark.gpu
def test_easy_synthesize_stream_flac_decodes_to_its_s16_wav():
    import scipy.io.wavfile as W
    bc, vc, bs, vs = _tiny()
    keys = ("input_ids", "word2ph", "phones", "tones", "langs")
    text = {k: synth.make_utterance(600, bc, vc, seed=777)[k] for k in keys}
    styles = synth.hash_normal(77, 3 * vc["style_dim"]).reshape(3, -1).astype(np.float32)
    for rate in (48000, 44100):
        wav = b"".join(orchestrator.easy_synthesize_stream(bs, vs, [text, None], styles, 1, 0,
                                                           orchestrator.SynthesizeOptions(sample_rate=rate, encoding="s16"), noise_seed=1234, chunk_frames=64))
        got_rate, y = W.read(io.BytesIO(wav))
        assert got_rate == rate and y.dtype == np.int16 and len(wav) == 44 + 2 * y.size and y.size > 4096
        pieces = list(orchestrator.easy_synthesize_stream(bs, vs, [text, None], styles, 1, 0,
                                                          orchestrator.SynthesizeOptions(sample_rate=rate, encoding="flac"), noise_seed=1234, chunk_frames=64))
        assert all(len(p) > 0 for p in pieces) and pieces[0][:4] == b"fLaC"
        got = R.read(b"".join(pieces))
        assert got["rate"] == rate
        np.testing.assert_array_equal(got["samples"], y)
    # f32 is offered the same way as s16; the default format is the plain stream
    wav = b"".join(orchestrator.easy_synthesize_stream(bs, vs, [text], styles, 1, 0, None, noise_seed=1234, chunk_frames=64))
    got_rate, z = W.read(io.BytesIO(wav))
    assert got_rate == 44100 and z.dtype == np.float32 and z.size == y.size
    assert np.abs(np.rint(np.clip(z.astype(np.float64), -1, 1) * 32767) - y).max() <= 1
    # the holder resolves the model and joins the text into one utterance
    from sbv2_api_amd import holder as H
    import json
    hd = H.TTSModelHolder(blob("bert", "tiny", 3), parse_text=lambda t: text)
    hd.load("m", json.dumps({"shape": list(styles.shape), "data": styles.tolist()}).encode(), blob("vits", "tiny", 5))
    got = R.read(b"".join(hd.easy_synthesize_stream("m", "line one\nline two", 1, 0, orchestrator.SynthesizeOptions(encoding="flac"),
                                                    noise_seed=1234, chunk_frames=64)))
    np.testing.assert_array_equal(got["samples"], y)
    with pytest.raises(H.ModelNotFoundError):
        hd.easy_synthesize_stream("nope", "x", 0, 0)
    hd.close()
    bs.close(); vs.close()
