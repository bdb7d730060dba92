"""G.711 output (sbv2_pcm_format.encoding 7 = mu-law, 6 = A-law; csrc/pcm_format.hip, csrc/marks.hip): one byte per sample, the code of the s16
integer that encoding 1 delivers for the same sample.

The reference is the numpy restatement below of the convention in include/sbv2_hip.h (above sbv2_pcm_format), written from its formulas; it is
not the library's host functions.  Every comparison is an equality of bytes or of f64 bits: a mu-law / A-law delivery is enc(the s16 delivery)
of the same call, the levels are the exact integer sums of dec(delivered bytes), the stats of a gain stage are those of the s16 call.
CPU tests run anywhere; GPU tests (@pytest.mark.gpu) need an MI355X."""
import ctypes as C
import struct
import types

import numpy as np
import pytest

from helpers import blob, make_utts, weights
from sbv2_api_amd import _lib, batcher, model, orchestrator, synth

gpu = pytest.mark.gpu
LAWS = ("mulaw", "alaw")
TAG = {"mulaw": 7, "alaw": 6}
RATES = (8000, 16000, 22050, 24000, 32000, 44100, 48000)
f64p = C.POINTER(C.c_double)


# ---- the numpy restatement ----------------------------------------------------------------------------------------------------------------

def lg(m):
    """floor(log2 m) of integers 1 <= m < 2^16."""
    m = np.asarray(m, np.int64)
    r = np.zeros_like(m)
    for k in range(1, 16):
        r[m >= (1 << k)] = k
    return r


def enc_np(q, law):
    q = np.maximum(np.asarray(q).astype(np.int64), -32767)   # (-32768 is taken as -32767: the quantiser never delivers it)
    if law == "mulaw":
        s = (q < 0).astype(np.int64)
        m = np.minimum(np.abs(q), 32635) + 132
        e = lg(m) - 7
        mant = (m >> (e + 3)) & 15
        return (~(s * 0x80 | e << 4 | mant) & 0xFF).astype(np.uint8)
    p = (q >= 0).astype(np.int64)
    m = np.where(q >= 0, q, -q - 1) >> 3
    e = np.where(m < 32, 0, lg(np.maximum(m, 1)) - 4)
    mant = np.where(e == 0, (m >> 1) & 15, (m >> e) & 15)
    return ((p * 0x80 | e << 4 | mant) ^ 0x55).astype(np.uint8)


def dec_np(code, law):
    code = np.asarray(code).astype(np.int64)
    if law == "mulaw":
        u = ~code & 0xFF
        t = (((u & 15) << 3) + 132) << ((u >> 4) & 7)
        return np.where(u & 0x80, 132 - t, t - 132)
    a = code ^ 0x55
    e = (a >> 4) & 7
    t = ((a & 15) << 4) + 8
    t = np.where(e >= 1, (t + 256) << np.maximum(e - 1, 0), t)
    return np.where(a & 0x80, t, -t)


def levels_np(v, start, end):
    """(sumsq, peak) of the integers v over [start, end) in int64 arithmetic; 0 for an empty span."""
    v = np.asarray(v, np.int64)
    ss, pk = np.zeros(len(start)), np.zeros(len(start))
    for i, (a, b) in enumerate(zip(start, end)):
        w = v[int(a):int(b)]
        if w.size:
            ss[i], pk[i] = float(int((w * w).sum())), float(int(np.abs(w).max()))
    return ss, pk


ALL_Q = np.arange(-32768, 32768).astype(np.int16)
ALL_CODES = np.arange(256).astype(np.uint8)


# ---- CPU: the host functions ----------------------------------------------------------------------------------------------------------------

def test_new_symbols_are_exported_and_declared():
    l = _lib.lib()
    for name in ("sbv2_g711_encode", "sbv2_g711_decode", "sbv2_debug_pcm_cast"):
        assert name in _lib.SYMBOLS and getattr(l, name).restype is C.c_int, name
    assert model.ENCODINGS == {"f32": 0, "s16": 1, "mulaw": 7, "alaw": 6}
    for law in LAWS:
        assert model.PcmFormat(8000, law).dtype is np.uint8 and model.PcmFormat(8000, law).c.encoding == TAG[law]
    assert model.PcmFormat(8000, "s16").dtype is np.int16 and model.PcmFormat().dtype is np.float32


@pytest.mark.parametrize("law", LAWS)
def test_host_codec_equals_the_restatement_on_every_value(law):
    codes = model.g711_encode(ALL_Q, law)
    assert codes.dtype == np.uint8
    np.testing.assert_array_equal(codes, enc_np(ALL_Q, law))
    assert codes[0] == codes[1]                                            # -32768 is taken as -32767
    table = model.g711_decode(ALL_CODES, law)
    assert table.dtype == np.int16
    np.testing.assert_array_equal(table, dec_np(ALL_CODES, law))
    np.testing.assert_array_equal(model.g711_decode(bytes(range(256)), law), table)   # bytes are taken as codes


@pytest.mark.parametrize("law", LAWS)
def test_host_codec_anchors_and_properties(law):
    q = ALL_Q[1:]                                                          # the 65535 values the quantiser delivers
    qi = q.astype(np.int64)
    codes = model.g711_encode(q, law)
    enc = lambda v: int(model.g711_encode(np.array([v], np.int16), law)[0])
    table = model.g711_decode(ALL_CODES, law).astype(np.int64)
    if law == "mulaw":
        assert (enc(0), enc(-1), enc(32767), enc(-32767)) == (0xFF, 0x7F, 0x80, 0x00)
        assert (table.min(), table.max()) == (-32124, 32124)
    else:
        assert (enc(0), enc(-1), enc(32767), enc(-32767)) == (0xD5, 0x55, 0xAA, 0x2A)
        assert (table.min(), table.max()) == (-32256, 32256)
    # round trip: every code but mu-law's minus zero
    again = model.g711_encode(table.astype(np.int16), law)
    keep = ALL_CODES != 0x7F if law == "mulaw" else np.ones(256, bool)
    np.testing.assert_array_equal(again[keep], ALL_CODES[keep])
    if law == "mulaw":
        assert table[0x7F] == 0 and again[0x7F] == 0xFF
    # monotone
    back = model.g711_decode(codes, law).astype(np.int64)
    assert (np.diff(back) >= 0).all()
    # error bound: half the step of the code's segment; mu-law saturates above 32635 with an error of at most 643
    err = np.abs(back - qi)
    if law == "mulaw":
        e = ((~codes.astype(np.int64) & 0xFF) >> 4) & 7
        inside = np.abs(qi) <= 32635
        assert (2 * err[inside] <= (1 << (e[inside] + 3))).all()
        assert (err[~inside] <= 643).all() and err.max() == 643
        assert (np.abs(back[~inside]) == 32124).all()                      # saturation, never a wrap
    else:
        e = ((codes.astype(np.int64) ^ 0x55) >> 4) & 7
        step = np.where(e == 0, 16, 8 << e)
        assert (2 * err <= step).all()
    assert (np.sign(back) * np.sign(qi) >= 0).all()


def test_host_codec_refuses_other_encodings():
    l = _lib.lib()
    q, c = np.zeros(4, np.int16), np.full(4, 0xEE, np.uint8)
    for bad in (0, 1, 2, 5, 8, -1):
        assert l.sbv2_g711_encode(bad, q.ctypes.data, 4, c.ctypes.data) != 0 and b"encoding" in l.sbv2_last_error()
        assert l.sbv2_g711_decode(bad, c.ctypes.data, 4, q.ctypes.data) != 0 and b"encoding" in l.sbv2_last_error()
    assert (c == 0xEE).all() and (q == 0).all()
    with pytest.raises(model.Sbv2Error, match="encoding"):
        model.g711_encode(q, "s16")
    with pytest.raises(model.Sbv2Error, match="encoding"):
        model.g711_decode(c, "flac")
    assert model.g711_encode(np.zeros(0, np.int16), "alaw").size == 0


def test_decoders_and_alaw_encoder_equal_audioop():
    """(the mu-law encoder is the 16-bit form of Sun's g711.c; audioop's drops two bits first and differs on 381 values: not compared)"""
    audioop = pytest.importorskip("audioop")
    q = ALL_Q[1:]
    np.testing.assert_array_equal(np.frombuffer(audioop.ulaw2lin(bytes(range(256)), 2), "<i2"), model.g711_decode(ALL_CODES, "mulaw"))
    np.testing.assert_array_equal(np.frombuffer(audioop.alaw2lin(bytes(range(256)), 2), "<i2"), model.g711_decode(ALL_CODES, "alaw"))
    np.testing.assert_array_equal(np.frombuffer(audioop.lin2alaw(q.astype("<i2").tobytes(), 2), np.uint8), model.g711_encode(q, "alaw"))


# ---- CPU: formats, bounds, the WAV writer -----------------------------------------------------------------------------------------------------

def test_format_length_accepts_the_laws_and_the_old_refusals_stand():
    l = _lib.lib()
    for r in RATES:
        _, L, M = model.pcm_format_taps(r)
        for law in LAWS:
            f = model.PcmFormat(r, law)
            for n in (0, 1, 511, 512, 44099, 10 ** 7):
                assert model.pcm_format_length(f, n) == -(-n * L // M), (r, law, n)
            assert l.sbv2_pcm_format_length(_lib.Sbv2PcmFormat(r, TAG[law], 0, 0), 441) == -(-441 * L // M)
    for enc in (2, 3, 4, 5, 8, -1):
        assert l.sbv2_pcm_format_length(_lib.Sbv2PcmFormat(16000, enc, 0, 0), 100) == -1
        assert "encoding" in l.sbv2_last_error().decode(), enc
    for bad in ("u8", "s24", "ulaw", "MULAW"):
        with pytest.raises(model.Sbv2Error, match="encoding"):
            model.PcmFormat(16000, bad)
    assert l.sbv2_pcm_format_length(_lib.Sbv2PcmFormat(11025, 7, 0, 0), 100) == -1 and "sample rate" in l.sbv2_last_error().decode()
    # the level stream's bound counts one byte per sample
    for law in LAWS:
        f, s = model.PcmFormat(8000, law), model.PcmFormat(8000, "s16")
        assert 2 * model.stream_level_bound(f, 4096, False) == model.stream_level_bound(s, 4096, False)
        A = model.stream_level_lookahead(s)
        assert model.stream_level_bound(f, 4096, False) == model.pcm_format_length(f, 4096) + A == model.stream_level_bound(f, 4096)
        # the look-ahead query keeps its first contract (f32 / s16 formats: A depends on the rate alone); the Python wrapper asks at the rate
        assert l.sbv2_stream_level_lookahead(C.byref(f.c)) == -1 and "encoding" in l.sbv2_last_error().decode()
        assert model.stream_level_lookahead(f) == A


def test_everything_flac_refuses_the_laws():
    l = _lib.lib()
    for law in LAWS:
        f = model.PcmFormat(8000, law)
        assert l.sbv2_flac_bound(C.byref(f.c), 1000) == -1 and "s16" in l.sbv2_last_error().decode()
        assert l.sbv2_flac_stream_bound(C.byref(f.c), 1000) == -1 and "s16" in l.sbv2_last_error().decode()
        assert l.sbv2_stream_level_bound(C.byref(f.c), 1000, 1) == -1 and "s16" in l.sbv2_last_error().decode()
        with pytest.raises(model.Sbv2Error, match="s16"):
            model.flac_bound(f, 1000)
    assert model.flac_bound(model.PcmFormat(8000, "s16"), 1000) > 0


def _parse_g711_wav(b):
    assert b[:4] == b"RIFF" and b[8:12] == b"WAVE" and b[12:16] == b"fmt " and b[38:42] == b"fact" and b[50:54] == b"data"
    riff, = struct.unpack("<I", b[4:8])
    fmt_len, tag, ch, rate, byte_rate, align, bits, cb = struct.unpack("<IHHIIHHH", b[16:38])
    fact_len, n_fact = struct.unpack("<II", b[42:50])
    n_data, = struct.unpack("<I", b[54:58])
    return dict(riff=riff, fmt_len=fmt_len, tag=tag, ch=ch, rate=rate, byte_rate=byte_rate, align=align, bits=bits, cb=cb, fact_len=fact_len,
                n_fact=n_fact, n_data=n_data, body=b[58:])


@pytest.mark.parametrize("law", LAWS)
@pytest.mark.parametrize("n", [0, 1, 2, 4001, 4002])
def test_g711_wav_layout_pad_and_stream_header(law, n):
    codes = np.random.default_rng(n + 1).integers(0, 256, n).astype(np.uint8)
    b = orchestrator.g711_wav(codes, 8000, law)
    h = _parse_g711_wav(b)
    assert (h["fmt_len"], h["tag"], h["ch"], h["rate"], h["byte_rate"], h["align"], h["bits"], h["cb"]) == (18, TAG[law], 1, 8000, 8000, 1, 8, 0)
    assert (h["fact_len"], h["n_fact"], h["n_data"]) == (4, n, n)
    assert h["riff"] == 50 + n + (n & 1) == len(b) - 8 and len(b) == 58 + n + (n & 1)
    assert h["body"][:n] == codes.tobytes() and h["body"][n:] == b"\0" * (n & 1)
    assert orchestrator.g711_wav(codes.tobytes(), 8000, law) == b                       # bytes are taken as codes
    head = orchestrator.wav_stream_header(8000, law, n)
    assert len(head) == 58 and head + codes.tobytes() + b"\0" * (n & 1) == b
    # the other two headers are what they were
    assert orchestrator.wav_stream_header(16000, "s16", n) == orchestrator.pcm16_wav(np.zeros(n, np.int16), 16000)[:44]
    assert orchestrator.wav_stream_header(16000, "f32", n) == orchestrator.float_wav(np.zeros(n, np.float32), 16000)[:-4 * n or None]


def test_g711_wav_refuses_other_encodings():
    for bad in ("s16", "f32", "flac", "u8"):
        with pytest.raises(model.Sbv2Error, match="encoding"):
            orchestrator.g711_wav(np.zeros(4, np.uint8), 8000, bad)


class _FakeStream:
    """The part of model.StreamHandle that orchestrator.SynthesisStream uses."""

    def __init__(self, chunks):
        self.chunks, self.closed, self.level = list(chunks), 0, None

    def next(self):
        return self.chunks.pop(0) if self.chunks else None

    def close(self):
        self.closed += 1


@pytest.mark.parametrize("n", [7, 8])
def test_synthesis_stream_ends_an_odd_g711_total_with_one_pad_byte(n):
    codes = np.arange(n).astype(np.uint8)
    st = _FakeStream([codes[:3], codes[3:3], codes[3:]])
    s = orchestrator.SynthesisStream(st, orchestrator.wav_stream_header(8000, "alaw", n), lambda c: c.tobytes(), tail=b"\0" if n & 1 else None)
    pieces = list(s)
    assert b"".join(pieces) == orchestrator.g711_wav(codes, 8000, "alaw") and st.closed == 1
    assert len(pieces) == 3 + (n & 1) and all(pieces)
    # on_close (the holder's lock) runs once, after the last byte has been handed out: not before the pad byte, not before the last chunk
    st = _FakeStream([codes])
    s = orchestrator.SynthesisStream(st, None, lambda c: c.tobytes(), tail=b"\0" if n & 1 else None)
    done = []
    s.on_close = lambda: done.append(1)
    for i, piece in enumerate(s):
        assert done == [] and piece == (codes.tobytes(), b"\0")[i]
    assert done == [1] and st.closed == 1 and i == (n & 1)
    # a stream closed early hands out nothing more, the pad included
    st = _FakeStream([codes])
    s = orchestrator.SynthesisStream(st, b"head", lambda c: c.tobytes(), tail=b"\0")
    assert next(s) == b"head"
    s.close()
    assert list(s) == [] and st.closed == 1


# ---- CPU: the option travels through REST, the batcher and the plan -----------------------------------------------------------------------------

STYLES = np.zeros((2, 4), np.float32)
FAKE_HOP = 4


class FakePipe:
    """Row i of a run: FAKE_HOP samples per phone, every sample the row's tag; fetch_request answers in fmt.dtype and records the format."""

    def __init__(self):
        self.calls, self.runs = [], 0

    def prepare(self, utts, **kw):
        lens = np.array([FAKE_HOP * len(u["phones"]) for u in utts], np.int64)
        return types.SimpleNamespace(utts=[dict(u) for u in utts], kw=kw, lens=lens, ticket=None, t_lens=np.array([len(u["phones"]) for u in utts]))

    def run(self, b):
        self.runs += 1
        b.ticket = self.runs
        return b.lens

    def fetch(self, b):
        return [np.full(int(n), u["tag"], np.float32) for n, u in zip(b.lens, b.utts)]

    def fetch_request(self, b, rows, fmt, place, joined_len, gain=None, flac=False, marks=False, env_hop=0, levels=True):
        self.calls.append(dict(rows=list(rows), rate=fmt.sample_rate, encoding=fmt.encoding, normalize=fmt.normalize, flac=flac, marks=marks))
        n = model.pcm_format_length(fmt, int(joined_len))
        out = b"fLaC" if flac else np.full(n, 0x2A if fmt.dtype is np.uint8 else 1, fmt.dtype)
        if not marks:
            return out, None
        k = sum(len(b.utts[r]["phones"]) for r in rows)
        return out, None, model.Marks(np.arange(k), np.arange(k) + 1, np.full(k, 32767.0 ** 2), np.full(k, 32767.0), 0, None, None, n)

    def close(self):
        pass


def _sent(tag, n):
    return dict(phones=[1] * n, word2ph=[n], tag=float(tag))


REQUEST = [_sent(0.5, 5), None, _sent(0.25, 3)]


@pytest.mark.parametrize("law", LAWS)
def test_plan_and_easy_synthesize_carry_the_law(law):
    opts = orchestrator.SynthesizeOptions(sample_rate=8000, encoding=law)
    plan = orchestrator.RequestPlan(REQUEST, STYLES, 0, 0, opts)
    assert (plan.fmt.sample_rate, plan.fmt.encoding, plan.fmt.dtype, plan.flac, plan.fmt.is_default) == (8000, law, np.uint8, False, False)
    pipe = FakePipe()
    wav = orchestrator.easy_synthesize(pipe, REQUEST, STYLES, options=opts, noise_seed=1)
    assert pipe.calls == [dict(rows=[0, 1], rate=8000, encoding=law, normalize=False, flac=False, marks=False)]
    h = _parse_g711_wav(wav)
    joined = FAKE_HOP * 8 + orchestrator.SENTENCE_GAP
    n = -(-joined * 80 // 441)
    assert (h["tag"], h["rate"], h["n_fact"], h["n_data"]) == (TAG[law], 8000, n, n) and h["body"][:n] == bytes([0x2A]) * n
    # marks: levels of the decoded integers re 32767, like s16
    audio, mk = orchestrator.easy_synthesize_marks(pipe, REQUEST, STYLES, options=opts, noise_seed=1)
    assert audio == wav and pipe.calls[-1]["marks"] and pipe.calls[-1]["encoding"] == law
    assert all(t["peak"] == 1.0 and t["level_dbfs"] == 0.0 for t in mk["tokens"])
    assert model.level_dbfs(32767.0 ** 2 * 10, 10, law) == 0.0 == model.level_dbfs(32767.0 ** 2 * 10, 10, "s16") and model.level_dbfs(10.0, 10, "f32") == 0.0
    # loudness and limiter compose: the plan keeps them next to the law
    plan = orchestrator.RequestPlan(REQUEST, STYLES, 0, 0, orchestrator.SynthesizeOptions(sample_rate=8000, encoding=law, loudness=-23.0, limiter=True))
    assert isinstance(plan.gain, model.Limiter) and plan.fmt.encoding == law


def test_flac_and_the_defaults_are_what_they_were():
    plan = orchestrator.RequestPlan(REQUEST, STYLES, 0, 0, orchestrator.SynthesizeOptions(sample_rate=16000, encoding="flac"))
    assert (plan.fmt.encoding, plan.flac, plan.fmt.dtype) == ("s16", True, np.int16)
    pipe = FakePipe()
    assert orchestrator.easy_synthesize(pipe, REQUEST, STYLES, options=orchestrator.SynthesizeOptions(sample_rate=16000, encoding="flac"),
                                        noise_seed=1) == b"fLaC"
    assert pipe.calls == [dict(rows=[0, 1], rate=16000, encoding="s16", normalize=False, flac=True, marks=False)]
    d = orchestrator.SynthesizeOptions()
    assert (d.sample_rate, d.encoding, d.normalize) == (44100, "f32", False)
    plan = orchestrator.RequestPlan(REQUEST, STYLES, 0, 0, None)
    assert plan.fmt.is_default and not plan.flac and plan.gain is None
    pipe = FakePipe()
    wav = orchestrator.easy_synthesize(pipe, REQUEST, STYLES, noise_seed=1)
    assert pipe.calls == []                                              # the default answer needs no formatted fetch, as before
    want = np.concatenate([np.full(20, 0.5, np.float32), np.zeros(orchestrator.SENTENCE_GAP, np.float32), np.full(12, 0.25, np.float32)])
    assert wav == orchestrator.float_wav(want, 44100)
    s16 = orchestrator.easy_synthesize(pipe, REQUEST, STYLES, options=orchestrator.SynthesizeOptions(sample_rate=16000, encoding="s16"), noise_seed=1)
    assert s16[:4] == b"RIFF" and struct.unpack("<H", s16[20:22])[0] == 1 and pipe.calls[-1]["encoding"] == "s16"
    for bad in ("u8", "s24"):
        with pytest.raises(model.Sbv2Error, match="encoding"):
            orchestrator.RequestPlan(REQUEST, STYLES, 0, 0, orchestrator.SynthesizeOptions(encoding=bad))


def test_batcher_plans_carry_the_law_per_request():
    pipe = FakePipe()
    rb = batcher.RequestBatcher(pipe, start=False, clock=lambda: 0.0, max_wait_ms=1000.0)
    futs = [rb.submit(REQUEST, STYLES, noise_seed=1, options=orchestrator.SynthesizeOptions(sample_rate=8000, encoding="mulaw")),
            rb.submit([_sent(0.75, 2)], STYLES, noise_seed=2, options=orchestrator.SynthesizeOptions(sample_rate=8000, encoding="alaw"), marks=True),
            rb.submit([_sent(0.75, 2)], STYLES, noise_seed=3, options=orchestrator.SynthesizeOptions(sample_rate=8000, encoding="flac")),
            rb.submit([_sent(0.125, 2)], STYLES, noise_seed=4)]
    rb.start()
    rb.close()
    assert pipe.runs == 1
    a, (b, mk), c, d = [f.result(0) for f in futs]
    assert [(x["rows"], x["encoding"], x["flac"], x["marks"]) for x in pipe.calls] == [([0, 1], "mulaw", False, False), ([2], "alaw", False, True),
                                                                                    ([3], "s16", True, False)]
    assert _parse_g711_wav(a)["tag"] == 7 and _parse_g711_wav(b)["tag"] == 6 and mk["sample_rate"] == 8000 and c == b"fLaC"
    assert d == orchestrator.float_wav(np.full(8, 0.125, np.float32), 44100)   # the default request of the same run: its bytes of before


def test_rest_passes_the_law_through_and_keeps_audio_wav():
    from fastapi.testclient import TestClient
    from sbv2_api_amd import rest

    class Pieces:
        marks = None

        def __init__(self):
            self.it = iter([b"ab", b"cd"])

        def __iter__(self):
            return self

        def __next__(self):
            return next(self.it)

    class Holder:
        def __init__(self):
            self.seen = []

        def models(self):
            return ["m"]

        def _take(self, route, options):
            self.seen.append((route, options.sample_rate, options.encoding))
            orchestrator.RequestPlan([_sent(1, 1)], STYLES, 0, 0, options)      # what the real holder does first: a bad encoding is refused here

        def easy_synthesize(self, ident, text, style_id, speaker_id, options):
            self._take("synthesize", options)
            return b"RIFF"

        def easy_synthesize_marks(self, ident, text, style_id, speaker_id, options):
            self._take("marks", options)
            return b"RIFF", {"sample_rate": options.sample_rate, "tokens": [], "words": []}

        def easy_synthesize_stream(self, ident, text, style_id, speaker_id, options):
            self._take("stream", options)
            return Pieces()

    h = Holder()
    c = TestClient(rest.make_app(h), raise_server_exceptions=False)
    for law in LAWS:
        body = {"text": "a", "ident": "m", "sample_rate": 8000, "encoding": law}
        r = c.post("/synthesize", json=body)
        assert r.status_code == 200 and r.headers["content-type"] == "audio/wav" and h.seen[-1] == ("synthesize", 8000, law)
        r = c.post("/synthesize_marks", json=body)
        assert r.status_code == 200 and r.json()["media_type"] == "audio/wav" and h.seen[-1] == ("marks", 8000, law)
        r = c.post("/synthesize_stream", json=body)
        assert r.status_code == 200 and r.headers["content-type"] == "audio/wav" and r.content == b"abcd" and h.seen[-1] == ("stream", 8000, law)
    r = c.post("/synthesize", json={"text": "a", "ident": "m", "encoding": "flac", "sample_rate": 16000})
    assert r.status_code == 200 and r.headers["content-type"] == "audio/flac" and h.seen[-1] == ("synthesize", 16000, "flac")
    assert c.post("/synthesize", json={"text": "a", "ident": "m"}).status_code == 200 and h.seen[-1] == ("synthesize", 44100, "f32")
    r = c.post("/synthesize", json={"text": "a", "ident": "m", "encoding": "u8"})
    assert r.status_code == 500 and r.text.startswith("Something went wrong: ") and "encoding" in r.text


# ---- GPU: the gain-stage kernel through its hook ------------------------------------------------------------------------------------------------

def quantise_np(x, g):
    return np.clip(np.rint((np.asarray(x, np.float64) * g) * 32767.0), -32767, 32767).astype(np.int64)


@gpu
@pytest.mark.parametrize("law", LAWS)
def test_cast_hook_every_value_and_clamping(law):
    x = np.arange(-32767, 32768) / 32767.0
    (one,) = model.debug_pcm_cast([x], [1.0], law)
    assert one.dtype == np.uint8
    np.testing.assert_array_equal(one, enc_np(np.arange(-32767, 32768), law))
    gains = [0.5, 1.7]
    got = model.debug_pcm_cast([x, x], gains, law)
    s16 = model.debug_pcm_cast([x, x], gains, "s16")
    for g, c, s in zip(gains, got, s16):
        np.testing.assert_array_equal(s, quantise_np(x, g))                # the s16 delivery is what the header says
        np.testing.assert_array_equal(c, enc_np(quantise_np(x, g), law))
        np.testing.assert_array_equal(c, enc_np(s, law))
    assert (quantise_np(x, 1.7) == 32767).sum() > 10000                    # clamped, then encoded: the top code, never a wrapped one
    assert got[1][-1] == (0x80 if law == "mulaw" else 0xAA) and got[1][0] == (0x00 if law == "mulaw" else 0x2A)
    (f,) = model.debug_pcm_cast([x], [0.5], "f32")
    np.testing.assert_array_equal(f, (x * 0.5).astype(np.float32))


CAST_LENS = [1, 2, 3, 5, 63, 64, 65, 255, 257, 1021]


@gpu
@pytest.mark.parametrize("law", LAWS)
def test_cast_hook_signals_back_to_back_equal_each_alone(law):
    """Signals start at odd byte offsets and end mid-dword; each has its own gain (the guard bands are checked by the hook on the device and by
    debug_pcm_cast on the host)."""
    rng = np.random.default_rng(711)
    offs = np.concatenate([[0], np.cumsum(CAST_LENS)])
    assert (offs[1:-1] % 2 == 1).any() and (offs[1:-1] % 4 != 0).sum() >= 6 and sum(CAST_LENS) > 256   # more than one block
    sigs = [rng.standard_normal(n) * 0.4 for n in CAST_LENS]
    gains = [0.3 + 0.37 * i for i in range(len(CAST_LENS))]               # up to 3.6: some signals clamp
    together = model.debug_pcm_cast(sigs, gains, law)
    assert [c.size for c in together] == CAST_LENS
    for i, (x, g, c) in enumerate(zip(sigs, gains, together)):
        (alone,) = model.debug_pcm_cast([x], [g], law)
        np.testing.assert_array_equal(c, alone, err_msg=f"signal {i}")
        np.testing.assert_array_equal(c, enc_np(quantise_np(x, g), law), err_msg=f"signal {i}")
    # empty signals in between change nothing
    holes = model.debug_pcm_cast([sigs[0], [], sigs[1], []], [gains[0], 9.0, gains[1], 9.0], law)
    assert [c.size for c in holes] == [1, 0, 2, 0]
    np.testing.assert_array_equal(np.concatenate(holes), np.concatenate(together[:2]))
    l = _lib.lib()
    assert l.sbv2_debug_pcm_cast(0, None, np.array([0], np.int64).ctypes.data_as(_lib.i64p), 1, np.ones(1).ctypes.data_as(f64p), 2, None) != 0
    assert b"encoding" in l.sbv2_last_error()


# ---- GPU: the level reduction through its hook ----------------------------------------------------------------------------------------------------

SEG_LENS = [0, 1, 2, 63, 64, 65, 255, 256, 257, 4097, 0, 3, 5000]
N_CODES = 12000


@gpu
@pytest.mark.parametrize("law", LAWS)
def test_segment_levels_of_codes(law):
    rng = np.random.default_rng(6)
    codes = rng.integers(0, 256, N_CODES).astype(np.uint8)
    codes[100:300] = 0x80 if law == "mulaw" else 0xAA                      # a run at the top level
    edges = np.concatenate([[0], np.cumsum(SEG_LENS)])
    st, en = np.append(edges[:-1], edges[-1]).astype(np.int64), np.append(edges[1:], N_CODES).astype(np.int64)
    assert (st % 2 == 1).any() and (st % 4 == 3).any() and en[-1] == N_CODES
    ss, pk = model.debug_segment_levels(codes, st, en, encoding=law)
    rs, rp = levels_np(dec_np(codes, law), st, en)
    np.testing.assert_array_equal(ss, rs)
    np.testing.assert_array_equal(pk, rp)
    assert ss[0] == 0.0 and pk[0] == 0.0 and pk.max() == (32124 if law == "mulaw" else 32256)
    moved = model.debug_segment_levels(np.concatenate([np.zeros(3, np.uint8), codes]), st + 3, en + 3, encoding=law)
    assert moved[0].tobytes() == ss.tobytes() and moved[1].tobytes() == pk.tobytes()
    # the s16 reduction of the decoded integers says the same
    s2, p2 = model.debug_segment_levels(dec_np(codes, law).astype(np.int16), st, en)
    assert s2.tobytes() == ss.tobytes() and p2.tobytes() == pk.tobytes()


# ---- GPU: the fetches ---------------------------------------------------------------------------------------------------------------------------------

FRAMES = [69, 164, 100]   # 16-sample frames: the delivered lengths are odd at 8 and 16 kHz, so signals 1 and 2 start at odd bytes


def _tiny():
    bc, _ = weights("bert", "tiny", 3)
    vc, _ = weights("vits", "tiny", 5)
    return bc, vc, model.load_model(blob("bert", "tiny", 3), True), model.load_model(blob("vits", "tiny", 5), False)


@pytest.fixture(scope="module")
def run3():
    bc, vc, bs, vs = _tiny()
    pipe = model.Pipeline(bs, vs)
    utts = make_utts([9, 23, 14], bc, vc, seed0=401, with_bert=False)
    for u, f in zip(utts, FRAMES):
        d = np.array(u["forced_durations"], np.int64)
        assert d.sum() <= f
        d[-1] += f - d.sum()
        u["forced_durations"] = d
    b = pipe.prepare(utts, forced=True)
    pipe.run(b)
    hop = _lib.lib().sbv2_vits_hop(vs.handle)
    assert [int(n) for n in b.lens] == [hop * f for f in FRAMES]
    lens = [int(n) for n in b.lens]
    place = [3000, 0, 3000 + lens[0] + 41]                                  # out of order, one gap shorter than a filter span
    joined = place[2] + lens[2] + 777
    yield types.SimpleNamespace(pipe=pipe, b=b, lens=lens, place=place, joined=joined)
    pipe.close(); bs.close(); vs.close()


def _same_codes(got, s16, law, what):
    assert len(got) == len(s16), what
    for i, (c, s) in enumerate(zip(got, s16)):
        assert c.dtype == np.uint8 and s.dtype == np.int16 and c.size == s.size, (what, i)
        np.testing.assert_array_equal(c, enc_np(s, law), err_msg=f"{what} signal {i}")


@gpu
@pytest.mark.parametrize("law", LAWS)
@pytest.mark.parametrize("rate", [8000, 16000])
def test_fetches_equal_enc_of_the_s16_fetch(run3, rate, law):
    r, pipe, b = run3, run3.pipe, run3.b
    f, s = model.PcmFormat(rate, law), model.PcmFormat(rate, "s16")
    per = pipe.fetch_format(b, s)
    assert all(x.size % 2 == 1 for x in per) and len({x.size for x in per}) == 3 and max(np.abs(x).max() for x in per) > 0
    _same_codes(pipe.fetch_format(b, f), per, law, "per utterance")
    _same_codes(pipe.fetch_format(b, f, r.place, r.joined), pipe.fetch_format(b, s, r.place, r.joined), law, "joined")
    fn, sn = model.PcmFormat(rate, law, True), model.PcmFormat(rate, "s16", True)
    norm = pipe.fetch_format(b, sn)
    assert all(np.abs(x.astype(np.int64)).max() == 32767 for x in norm)
    _same_codes(pipe.fetch_format(b, fn), norm, law, "normalised")
    _same_codes(pipe.fetch_format(b, fn, r.place, r.joined), pipe.fetch_format(b, sn, r.place, r.joined), law, "normalised joined")
    ln = model.Loudness(-23.0, -1.0)
    (got, st), (want, st16) = pipe.fetch_loudness(b, f, ln), pipe.fetch_loudness(b, s, ln)
    _same_codes(got, want, law, "loudness")
    assert st.tobytes() == st16.tobytes() and np.isfinite(st).all()
    (got, st), (want, st16) = pipe.fetch_loudness(b, f, ln, r.place, r.joined), pipe.fetch_loudness(b, s, ln, r.place, r.joined)
    _same_codes(got, want, law, "loudness joined")
    assert st.tobytes() == st16.tobytes()
    # a target 3 dB above what the plain scale reaches on the signal with the smallest peak-to-loudness ratio (measured by the s16 fetch): the
    # limiter cannot be idle on it
    _, meas = pipe.fetch_loudness(b, s, None)
    plr = [tp - lu for lu, tp, _ in meas if np.isfinite(lu)]
    assert plr, meas
    lim = model.Limiter(min(-5.0, -1.0 - min(plr) + 3.0), -1.0, 6.0)
    (got, st), (want, st16) = pipe.fetch_limited(b, f, lim), pipe.fetch_limited(b, s, lim)
    _same_codes(got, want, law, "limited")
    assert st.tobytes() == st16.tobytes()
    print(f"[g711] {rate} {law}: limiter depths {st[:, 5]}")
    assert (st[:, 5] < 0).any(), "the limiter is active on at least one signal"
    # a request of two of the three rows, with each gain stage
    rows, place = [2, 0], [r.place[2], r.place[0]]
    for gain in (None, ln, lim):
        (got, st), (want, st16) = pipe.fetch_request(b, rows, f, place, r.joined, gain=gain), pipe.fetch_request(b, rows, s, place, r.joined, gain=gain)
        _same_codes([got], [want], law, f"request {gain}")
        assert (st is None and st16 is None) if gain is None else st.tobytes() == st16.tobytes()
    with pytest.raises(model.Sbv2Error, match="normalize"):
        pipe.fetch_loudness(b, fn, ln)


@gpu
def test_fetch_at_44100_identity_rate(run3):
    pipe, b = run3.pipe, run3.b
    s16 = pipe.fetch_format(b, model.PcmFormat(44100, "s16"))
    native = pipe.fetch(b)
    for law in LAWS:
        got = pipe.fetch_format(b, model.PcmFormat(44100, law))
        _same_codes(got, s16, law, "44100")
        for c, x in zip(got, native):                                       # no resampling: the codes of the native samples
            np.testing.assert_array_equal(c, enc_np(quantise_np(x, 1.0), law))


@gpu
@pytest.mark.parametrize("law", LAWS)
def test_capacity_one_byte_short_is_refused_with_nothing_written(run3, law):
    l, pipe, b = _lib.lib(), run3.pipe, run3.b
    f = model.PcmFormat(8000, law)
    n = sum(model.pcm_format_length(f, x) for x in b.lens)
    dst = np.full(n + 8, 0xA5, np.uint8)
    outs = np.full(3, -5, np.int64)
    rc = l.sbv2_pipeline_fetch_pcm_format(pipe.h, b.ticket, f.c, None, 0, dst.ctypes.data, n - 1, outs.ctypes.data_as(_lib.i64p))
    assert rc != 0 and b"too small" in l.sbv2_last_error() and (dst == 0xA5).all() and (outs == -5).all()
    _lib.check(l.sbv2_pipeline_fetch_pcm_format(pipe.h, b.ticket, f.c, None, 0, dst.ctypes.data, n, outs.ctypes.data_as(_lib.i64p)))
    assert int(outs.sum()) == n and (dst[n:] == 0xA5).all()                  # samples are bytes: exactly n written
    np.testing.assert_array_equal(dst[:n], np.concatenate(pipe.fetch_format(b, f)))
    # the request fetch counts bytes the same way
    rows, pl = np.array([1], np.int32), np.array([0], np.int64)
    req = _lib.Sbv2FetchRequest(rows.ctypes.data_as(C.POINTER(C.c_int32)), 1, pl.ctypes.data_as(_lib.i64p), int(b.lens[1]), C.pointer(f.c), None, None, 0)
    m = model.pcm_format_length(f, int(b.lens[1]))
    got = C.c_int64(-5)
    dst[:] = 0xA5
    assert l.sbv2_pipeline_fetch_request(pipe.h, b.ticket, C.byref(req), dst.ctypes.data, m - 1, C.byref(got), None) != 0
    assert b"too small" in l.sbv2_last_error() and (dst == 0xA5).all() and got.value == -5


@gpu
@pytest.mark.parametrize("law", LAWS)
def test_flac_is_refused_with_a_g711_format(run3, law):
    l, pipe, b = _lib.lib(), run3.pipe, run3.b
    f = model.PcmFormat(8000, law)
    dst, outs = np.full(1 << 16, 0xA5, np.uint8), np.full(3, -5, np.int64)
    assert l.sbv2_pipeline_fetch_flac(pipe.h, b.ticket, f.c, None, 0, dst.ctypes.data, dst.nbytes, outs.ctypes.data_as(_lib.i64p)) != 0
    assert b"s16" in l.sbv2_last_error() and (dst == 0xA5).all() and (outs == -5).all()
    rows, pl = np.array([1], np.int32), np.array([0], np.int64)
    req = _lib.Sbv2FetchRequest(rows.ctypes.data_as(C.POINTER(C.c_int32)), 1, pl.ctypes.data_as(_lib.i64p), int(b.lens[1]), C.pointer(f.c), None, None, 1)
    got = C.c_int64(-5)
    assert l.sbv2_pipeline_fetch_request(pipe.h, b.ticket, C.byref(req), dst.ctypes.data, dst.nbytes, C.byref(got), None) != 0
    assert b"s16" in l.sbv2_last_error() and (dst == 0xA5).all() and got.value == -5
    for call in (lambda: pipe.fetch_flac(b, f), lambda: pipe.fetch_request(b, [1], f, [0], int(b.lens[1]), flac=True)):
        with pytest.raises(model.Sbv2Error, match="s16"):
            call()


# ---- GPU: marks -----------------------------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("law", LAWS)
@pytest.mark.parametrize("gain", [None, model.Loudness(-23.0, -1.0)], ids=["plain", "loudness"])
def test_marks_are_the_exact_levels_of_the_decoded_bytes(run3, law, gain):
    r, pipe, b = run3, run3.pipe, run3.b
    f = model.PcmFormat(8000, law)
    rows, place = [2, 0], [r.place[2], r.place[0]]
    plain, st0 = pipe.fetch_request(b, rows, f, place, r.joined, gain=gain)
    plain = plain.copy()
    out_len = model.pcm_format_length(f, r.joined)
    for env_hop in (80, 333):
        out, st, m = pipe.fetch_request(b, rows, f, place, r.joined, gain=gain, marks=True, env_hop=env_hop)
        assert out.dtype == np.uint8 and out.tobytes() == plain.tobytes() and out.size == out_len      # the audio of the fetch without marks
        assert (st is None and st0 is None) if gain is None else st.tobytes() == st0.tobytes()
        v = dec_np(out, law)
        ts, tp = levels_np(v, m.start, m.end)
        np.testing.assert_array_equal(m.sumsq, ts)
        np.testing.assert_array_equal(m.peak, tp)
        assert (m.start % 2 == 1).any() and (m.sumsq > 0).any()
        fs = np.arange(0, out_len, env_hop)
        es, ep = levels_np(v, fs, np.minimum(fs + env_hop, out_len))
        np.testing.assert_array_equal(m.env_sumsq, es)
        np.testing.assert_array_equal(m.env_peak, ep)
    # the spans are those of the s16 fetch: the rate alone decides them
    _, _, m16 = pipe.fetch_request(b, rows, model.PcmFormat(8000, "s16"), place, r.joined, gain=gain, marks=True, levels=False)
    np.testing.assert_array_equal(m.start, m16.start)
    np.testing.assert_array_equal(m.end, m16.end)


# ---- GPU: streams ---------------------------------------------------------------------------------------------------------------------------------

def _hop(vs):
    return _lib.lib().sbv2_vits_hop(vs.handle)


def _chunks(bs, vs, u, chunk, fmt, **kw):
    st = model.StreamHandle(bs, vs, u, chunk, fmt=fmt, **kw)
    parts = []
    while (c := st.next()) is not None:
        parts.append(c)
    total = st.total_samples
    st.close()
    return parts, total


def _level_calls(bs, vs, u, chunk, fmt, lv, **kw):
    """([(delivered, n_consumed)] per call that consumed samples, total_samples, level stats)."""
    l = _lib.lib()
    st = model.StreamHandle(bs, vs, u, chunk, fmt=fmt, level=lv, **kw)
    assert st.buf.nbytes == model.stream_level_bound(fmt, chunk * _hop(vs), False)
    calls = []
    no, nc = C.c_int64(), C.c_int64()
    while True:
        _lib.check(l.sbv2_stream_next_level(st.h, st.buf.ctypes.data, st.buf.nbytes, C.byref(no), C.byref(nc)))
        if nc.value == 0:
            break
        calls.append((st.buf[:no.value * np.dtype(fmt.dtype).itemsize].view(fmt.dtype).copy(), nc.value))
    total, stats = st.total_samples, st.level_stats()
    st.close()
    return calls, total, stats


@pytest.fixture(scope="module")
def stream_models():
    bc, vc, bs, vs = _tiny()
    u = make_utts([700], bc, vc, seed0=1000, with_bert=False)[0]
    yield bs, vs, u
    bs.close(); vs.close()


@gpu
@pytest.mark.parametrize("law,rate,chunk", [("mulaw", 48000, 64), ("mulaw", 24000, 50), ("alaw", 48000, 16), ("mulaw", 44100, 64)])
def test_format_stream_equals_enc_of_the_s16_stream(stream_models, law, rate, chunk):
    bs, vs, u = stream_models
    want, total16 = _chunks(bs, vs, u, chunk, model.PcmFormat(rate, "s16"), forced=True)
    got, total = _chunks(bs, vs, u, chunk, model.PcmFormat(rate, law), forced=True)
    assert total == total16 == sum(c.size for c in got) and [c.size for c in got] == [c.size for c in want] and len(got) > 2
    assert all(c.dtype == np.uint8 for c in got)
    np.testing.assert_array_equal(np.concatenate(got), enc_np(np.concatenate(want), law))
    assert (np.cumsum([c.size for c in got])[:-1] % 2 == 1).any() or rate == 44100      # chunks end at odd bytes


@gpu
@pytest.mark.parametrize("law,rate,chunk", [("mulaw", 44100, 16), ("alaw", 48000, 64)])
def test_level_stream_equals_enc_of_the_s16_level_stream(stream_models, law, rate, chunk):
    """44.1 kHz with 16-frame chunks of the tiny decoder (hop 16): 256 samples a chunk against a look-ahead of 452, so the first call consumes
    samples and emits none."""
    bs, vs, u = stream_models
    y = np.concatenate(_chunks(bs, vs, u, 64, model.PcmFormat(rate, "f32"), forced=True)[0])
    ceiling = -1.0 if np.abs(y).max() > 0.02 else -20.0
    lv = model.StreamLevel(float(np.round(ceiling - 20 * np.log10(np.abs(y).max()) + 9.0, 2)), ceiling)   # the peak 9 dB over the ceiling
    want, total16, stats16 = _level_calls(bs, vs, u, chunk, model.PcmFormat(rate, "s16"), lv, forced=True)
    got, total, stats = _level_calls(bs, vs, u, chunk, model.PcmFormat(rate, law), lv, forced=True)
    assert total == total16 == sum(d.size for d, _ in got)
    assert [(d.size, n) for d, n in got] == [(d.size, n) for d, n in want]
    assert stats == stats16 and stats[0] < -3.0, stats                       # the limiter engages; the stats are the s16 stream's, bit for bit
    if chunk == 16 and rate == 44100:
        assert got[0][0].size == 0 and got[0][1] == 256 and got[1][0].size == 2 * 256 - 452
    codes = np.concatenate([d for d, _ in got])
    assert codes.dtype == np.uint8
    np.testing.assert_array_equal(codes, enc_np(np.concatenate([d for d, _ in want]), law))
    # under the ceiling before the quantiser; the code then stands for a level at most half the widest step (1024) away
    assert np.abs(dec_np(codes, law)).max() <= np.rint(10 ** (ceiling / 20) * 32767) + 512


@gpu
def test_stream_refusals_with_a_g711_format(stream_models):
    bs, vs, u = stream_models
    for law in LAWS:
        with pytest.raises(model.Sbv2Error, match="s16"):
            model.StreamHandle(bs, vs, u, 64, fmt=model.PcmFormat(48000, law), flac=True, forced=True)
        with pytest.raises(model.Sbv2Error, match="s16"):
            model.StreamHandle(bs, vs, u, 64, fmt=model.PcmFormat(48000, law), flac=True, level=model.StreamLevel(3.0, -1.0), forced=True)
        with pytest.raises(model.Sbv2Error, match="normali"):
            model.StreamHandle(bs, vs, u, 64, fmt=model.PcmFormat(48000, law, True), forced=True)
    # too small a buffer for a chunk is refused with nothing written; the chunk can be taken again
    st = model.StreamHandle(bs, vs, u, 64, fmt=model.PcmFormat(48000, "mulaw"), forced=True)
    small, n = np.full(64, 0xA5, np.uint8), C.c_int64(-5)
    assert _lib.lib().sbv2_stream_next_format(st.h, small.ctypes.data, small.nbytes, C.byref(n)) != 0
    assert b"too small" in _lib.lib().sbv2_last_error() and (small == 0xA5).all()
    st.close()


@gpu
def test_easy_synthesize_stream_is_the_g711_wav_of_its_codes():
    bc, vc, bs, vs = _tiny()
    keys = ("input_ids", "word2ph", "phones", "tones", "langs")
    text = {k: synth.make_utterance(600, bc, vc, seed=777)[k] for k in keys}
    styles = synth.hash_normal(77, 3 * vc["style_dim"]).reshape(3, -1).astype(np.float32)

    def run(**kw):
        st = orchestrator.easy_synthesize_stream(bs, vs, [text], styles, 1, 0, orchestrator.SynthesizeOptions(**kw), noise_seed=1234, chunk_frames=64)
        return b"".join(st), st

    parities = set()
    for rate, scale in ((48000, 1.0), (24000, 1.0), (48000, 1.1), (24000, 1.1), (48000, 1.3), (24000, 1.3)):
        s16, _ = run(encoding="s16", sample_rate=rate, length_scale=scale)
        x = np.frombuffer(s16[44:], "<i2")
        for law in LAWS:
            wav, _ = run(encoding=law, sample_rate=rate, length_scale=scale)
            assert wav == orchestrator.g711_wav(enc_np(x, law), rate, law), (rate, scale, law)
            assert len(wav) == 58 + x.size + (x.size & 1)
        parities.add(x.size & 1)
        if parities == {0, 1}:
            break
    assert 1 in parities, "no candidate gave an odd total: the pad byte was not exercised"
    # with a level: the codes of the s16 level stream, the same stats
    s16, st16 = run(encoding="s16", sample_rate=48000, gain_db=12.0, true_peak_max=-3.0)
    wav, stm = run(encoding="mulaw", sample_rate=48000, gain_db=12.0, true_peak_max=-3.0)
    assert wav == orchestrator.g711_wav(enc_np(np.frombuffer(s16[44:], "<i2"), "mulaw"), 48000, "mulaw")
    assert stm.level_stats == st16.level_stats and stm.level_stats is not None
    with pytest.raises(model.Sbv2Error, match="normalise"):
        run(encoding="mulaw", sample_rate=48000, normalize=True)
    bs.close(); vs.close()
