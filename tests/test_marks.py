"""Speech marks (sbv2_marks, sbv2_pipeline_fetch_request_marks, sbv2_marks_spans, sbv2_stream_marks; csrc/marks.hip): the span arithmetic
against a numpy restatement and the host-side refusals (CPU), the orchestrator / batcher / REST contracts against fakes (CPU), the level
reduction launch by launch, and the pipeline, FLAC sink, stream and batcher on tiny models (GPU).

Tolerances.  s16: squares and sums are integers below 2^53, so sumsq and peak are EQUAL to numpy's.  f32: peak is equal; every square is exact
in f64 and a sum of n non-negative terms in ANY order lies within n 2^-52 relative of any other order (each of the n - 1 additions loses at most
2^-53 relative of a partial sum that never exceeds the total; twice that for the two orders compared), which is the bound asserted."""
import base64
import contextlib
import ctypes as C
import json
import os
import re
import types

import numpy as np
import pytest

import flac_reader as R
import sbv2_oracle as O
from helpers import blob, make_utts, weights
from sbv2_api_amd import _lib, batcher, model, orchestrator, synth

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["sbv2_pipeline_fetch_request_marks", "sbv2_marks_spans", "sbv2_stream_marks", "sbv2_debug_segment_levels"]
RATES = {44100: (1, 1), 48000: (160, 147), 22050: (1, 2), 8000: (80, 441)}
HOP = 512
f64p = C.POINTER(C.c_double)


def spans_np(d, hop, place, rate):
    """Section 'Token spans' of the header, restated: J(a) = ceil(a L / M) at the edges place + hop c[t] (c = exclusive prefix sum of d)."""
    L, M = RATES[rate] if rate in RATES else (rate // np.gcd(rate, 44100), 44100 // np.gcd(rate, 44100))
    c = np.concatenate([[0], np.cumsum(np.asarray(d, np.int64))])
    edges = -((-(place + hop * c) * L) // M)
    return edges[:-1].astype(np.int64), edges[1:].astype(np.int64)


def levels_np(x, start, end):
    """(sumsq, peak) of the delivered samples x over [start, end): int64 arithmetic for s16, float64 for f32; 0 for an empty span."""
    ss, pk = np.zeros(len(start)), np.zeros(len(start))
    for i, (a, b) in enumerate(zip(start, end)):
        v = x[int(a):int(b)]
        if v.size:
            if x.dtype == np.int16:
                w = v.astype(np.int64)
                ss[i], pk[i] = float(int((w * w).sum())), float(int(np.abs(w).max()))
            else:
                w = v.astype(np.float64)
                ss[i], pk[i] = float((w * w).sum()), float(np.abs(w).max())
    return ss, pk


def check_levels(x, start, end, sumsq, peak, what):
    rs, rp = levels_np(x, start, end)
    np.testing.assert_array_equal(peak, rp, err_msg=what + ": peak")
    if x.dtype == np.int16:
        np.testing.assert_array_equal(sumsq, rs, err_msg=what + ": sumsq (s16 is exact)")
        return
    n = (np.asarray(end) - np.asarray(start)).astype(np.float64)
    err = np.abs(np.asarray(sumsq) - rs)
    worst = float((err / np.maximum(n * 2.0 ** -52 * rs, 1e-300)).max()) if len(rs) else 0.0
    print(f"[marks] {what}: f32 sumsq error / (len 2^-52 sumsq) worst {worst:.3f}")
    assert (err <= n * 2.0 ** -52 * rs).all(), what


# ---- CPU: ABI ---------------------------------------------------------------------------------------------------------------------------------------

def test_new_symbols_are_exported_and_declared():
    header = open(os.path.join(ROOT, "include", "sbv2_hip.h")).read()
    l = _lib.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.SYMBOLS and getattr(l, name) is not None, name
    assert "} sbv2_marks;" in header
    assert C.sizeof(_lib.Sbv2Marks) == 88


DURS = [0, 1, 0, 0, 7, 1, 100000, 3, 0, 2, 0]


@pytest.mark.parametrize("rate", sorted(RATES))
@pytest.mark.parametrize("place", [0, 1000003])
def test_marks_spans_equal_the_restatement(rate, place):
    assert place == 0 or (place % 147 and place % 441 and place % 2)
    fmt = model.PcmFormat(rate, "s16")
    st, en = model.marks_spans(DURS, HOP, place, fmt)
    rs, re_ = spans_np(DURS, HOP, place, rate)
    np.testing.assert_array_equal(st, rs)
    np.testing.assert_array_equal(en, re_)
    # the partition properties of the contract
    J = lambda a: model.pcm_format_length(fmt, a)
    assert st[0] == J(place) and en[-1] == J(place + HOP * sum(DURS))
    np.testing.assert_array_equal(en[:-1], st[1:])
    assert (en >= st).all()
    for d, a, b in zip(DURS, st, en):
        assert d > 0 or a == b
    # the all-zero row: one synthesised frame that belongs to no token
    st, en = model.marks_spans([0, 0, 0], HOP, place, fmt)
    assert (st == J(place)).all() and (en == J(place)).all() and J(place + HOP) > J(place)
    st, en = model.marks_spans([], HOP, place, fmt)
    assert st.size == 0 and en.size == 0


def test_marks_spans_refusals():
    l = _lib.lib()
    d, out = np.array([1, -1, 2], np.int64), np.full(6, 77, np.int64)
    f = model.PcmFormat(16000, "s16")
    p = lambda a, o=0: C.cast(a.ctypes.data + 8 * o, _lib.i64p)
    for args, word in (((p(d), 3, HOP, 0, C.byref(f.c)), "negative duration"), ((p(d), 1, 0, 0, C.byref(f.c)), "hop"),
                       ((p(d), 1, HOP, -1, C.byref(f.c)), "place"), ((p(d), 1, HOP, 0, None), "")):
        assert l.sbv2_marks_spans(*args, p(out), p(out, 3)) != 0
        assert word in l.sbv2_last_error().decode()
    bad = _lib.Sbv2PcmFormat(12345, 0, 0, 0)
    assert l.sbv2_marks_spans(p(d), 1, HOP, 0, C.byref(bad), p(out), p(out, 3)) != 0


def _c_marks(ntok, nenv, env_hop=0, reserved=0, levels=True, fill=77):
    a = types.SimpleNamespace(start=np.full(ntok + 2, fill, np.int64), end=np.full(ntok + 2, fill, np.int64), sumsq=np.full(ntok + 2, fill, np.float64),
                              peak=np.full(ntok + 2, fill, np.float64), esumsq=np.full(nenv + 2, fill, np.float64), epeak=np.full(nenv + 2, fill, np.float64))
    q = lambda x, t: C.cast(x.ctypes.data + 8, t)   # (one guard word in front, one behind)
    a.c = _lib.Sbv2Marks(ntok, q(a.start, _lib.i64p), q(a.end, _lib.i64p), q(a.sumsq, f64p) if levels else None, q(a.peak, f64p) if levels else None, -9,
                         env_hop, reserved, nenv, q(a.esumsq, f64p), q(a.epeak, f64p), -9)
    a.untouched = lambda: all((x == fill).all() for x in (a.start, a.end, a.sumsq, a.peak, a.esumsq, a.epeak)) and a.c.n_tokens == -9 and a.c.n_env == -9
    a.guards = lambda: all(x[0] == fill and x[-1] == fill for x in (a.start, a.end, a.sumsq, a.peak, a.esumsq, a.epeak))
    return a


def test_marks_refusals_that_need_no_run():
    l = _lib.lib()
    f = model.PcmFormat(16000, "s16")
    rows, place = np.array([0], np.int32), np.array([0], np.int64)
    dst, got = np.full(16, 77, np.uint8), C.c_int64(-5)
    req = lambda fmt: _lib.Sbv2FetchRequest(rows.ctypes.data_as(C.POINTER(C.c_int32)), 1, place.ctypes.data_as(_lib.i64p), 10, fmt, None, None, 0)
    call = lambda r, m: l.sbv2_pipeline_fetch_request_marks(None, 1, C.byref(r), dst.ctypes.data, dst.nbytes, C.byref(got), None, C.byref(m.c))
    bad = _lib.Sbv2PcmFormat(12345, 1, 0, 0)
    for m, r, word in ((_c_marks(4, 4, reserved=1), req(C.pointer(f.c)), "reserved"), (_c_marks(4, 4, env_hop=-1), req(C.pointer(f.c)), "env_hop"),
                       (_c_marks(4, 4), req(C.pointer(bad)), "12345")):
        assert call(r, m) != 0
        assert word in l.sbv2_last_error().decode(), l.sbv2_last_error()
        assert m.untouched() and (dst == 77).all() and got.value == -5
    m = _c_marks(4, 4, env_hop=160)
    m.c.env_sumsq = None
    assert call(req(C.pointer(f.c)), m) != 0 and b"env_sumsq" in l.sbv2_last_error()
    m = _c_marks(4, 4)
    assert call(req(C.pointer(f.c)), m) != 0 and b"bad arguments" in l.sbv2_last_error()   # everything static passed: the null handle itself
    assert l.sbv2_pipeline_fetch_request_marks(None, 1, C.byref(req(C.pointer(f.c))), dst.ctypes.data, dst.nbytes, C.byref(got), None, None) != 0
    assert m.untouched() and (dst == 77).all() and got.value == -5


# ---- CPU: orchestrator, batcher, REST -----------------------------------------------------------------------------------------------------------------

STYLES = np.zeros((2, 4), np.float32)
FAKE_HOP = 4


class FakePipe:
    """Row i of a run: d = phones[t] + 1 frames of FAKE_HOP samples per token, every sample the row's tag; marks as the library defines them."""

    def __init__(self):
        self.calls, self.runs = [], 0

    def prepare(self, utts, **kw):
        lens = np.array([FAKE_HOP * sum(int(p) + 1 for p in u["phones"]) for u in utts], np.int64)
        return types.SimpleNamespace(utts=[dict(u) for u in utts], kw=kw, lens=lens, ticket=None, t_lens=np.array([len(u["phones"]) for u in utts]))

    def run(self, b):
        self.runs += 1
        b.ticket = self.runs
        return b.lens

    def fetch(self, b):
        return [np.full(int(n), u["tag"], np.float32) for n, u in zip(b.lens, b.utts)]

    def fetch_request(self, b, rows, fmt, place, joined_len, gain=None, flac=False, marks=False, env_hop=0, levels=True):
        self.calls.append(dict(rows=list(rows), rate=fmt.sample_rate, marks=marks, env_hop=env_hop))
        t = np.zeros(int(joined_len), np.float32)
        st, en = [], []
        for r, p in zip(rows, place):
            t[p:p + int(b.lens[r])] = b.utts[r]["tag"]
            s, e = spans_np([int(x) + 1 for x in b.utts[r]["phones"]], FAKE_HOP, p, 44100)
            st, en = st + list(s), en + list(e)
        out = t.astype(fmt.dtype)
        if not marks:
            return out, None
        ss, pk = levels_np(out, st, en)
        fs = np.arange(0, len(out), env_hop) if env_hop else np.zeros(0, np.int64)
        es, ep = levels_np(out, fs, np.minimum(fs + env_hop, len(out)))
        return out, None, model.Marks(np.array(st), np.array(en), ss, pk, env_hop, es if env_hop else None, ep if env_hop else None, len(out))

    def close(self):
        pass


def _sent(tag, phones, word2ph):
    return dict(phones=list(phones), word2ph=list(word2ph), tag=float(tag))


REQUEST = [_sent(0.5, [0, 2, 0, 1, 0], [1, 0, 3, 1]), None, _sent(0.25, [0, 3, 0], [2, 1]), None]


def test_marks_dict_words_are_unions_gaps_are_unowned_and_the_audio_is_unchanged():
    pipe = FakePipe()
    plain = orchestrator.easy_synthesize(pipe, REQUEST, STYLES, noise_seed=1)
    assert pipe.calls == []                                   # the default path of easy_synthesize needs no formatted fetch, as before
    audio, mk = orchestrator.easy_synthesize_marks(pipe, REQUEST, STYLES, noise_seed=1, options=orchestrator.SynthesizeOptions(envelope_hz=4410))
    assert audio == plain
    assert pipe.calls == [dict(rows=[0, 1], rate=44100, marks=True, env_hop=10)]   # ONE fetch with marks at the identity format
    json.dumps(mk)                                            # JSON ready
    assert mk["sample_rate"] == 44100 and set(mk) == {"sample_rate", "tokens", "words", "envelope"}
    toks, words = mk["tokens"], mk["words"]
    assert [(t["line"], t["index"], t["phone"]) for t in toks] == [(0, i, p) for i, p in enumerate([0, 2, 0, 1, 0])] + [(2, i, p) for i, p in enumerate([0, 3, 0])]
    len0 = FAKE_HOP * sum(p + 1 for p in REQUEST[0]["phones"])
    assert toks[0]["start"] == 0 and toks[4]["end"] == len0
    assert toks[5]["start"] == len0 + orchestrator.SENTENCE_GAP     # the gap between the sentences belongs to no token
    total = len(plain[plain.index(b"data") + 8:]) // 4
    assert toks[-1]["end"] == total - orchestrator.SENTENCE_GAP      # line 2 is not the last line: its gap is unowned too
    for t in toks:
        assert t["start_s"] == t["start"] / 44100 and t["end_s"] == t["end"] / 44100
        tag = 0.5 if t["line"] == 0 else 0.25
        assert t["peak"] == tag and abs(t["level_dbfs"] - 20 * np.log10(tag)) < 1e-9
    # words: the union of their tokens' spans; a word without tokens is empty where the next one starts
    w = [(x["line"], x["index"], x["start"], x["end"]) for x in words]
    assert w[0] == (0, 0, toks[0]["start"], toks[0]["end"])
    assert w[1] == (0, 1, toks[1]["start"], toks[1]["start"])
    assert w[2] == (0, 2, toks[1]["start"], toks[3]["end"])
    assert w[3] == (0, 3, toks[4]["start"], toks[4]["end"])
    assert w[4] == (2, 0, toks[5]["start"], toks[6]["end"]) and w[5] == (2, 1, toks[7]["start"], toks[7]["end"])
    env = mk["envelope"]
    assert env["hop"] == 10 and len(env["level_dbfs"]) == len(env["peak"]) == -(-total // 10)
    assert env["peak"][0] == 0.5 and env["level_dbfs"][len0 // 10 + 1] is None        # silence has no level
    # an empty span has no level
    m = model.Marks(np.array([3]), np.array([3]), np.array([0.0]), np.array([0.0]))
    d = orchestrator.marks_dict([_sent(1, [5], [1])], [0], model.PcmFormat(), m)
    assert d["tokens"][0]["level_dbfs"] is None and "envelope" not in d
    with pytest.raises(model.Sbv2Error):
        orchestrator.easy_synthesize_marks(pipe, REQUEST, STYLES, noise_seed=1, options=orchestrator.SynthesizeOptions(envelope_hz=0))


def test_s16_levels_are_taken_re_full_scale():
    assert model.level_dbfs(32767.0 ** 2 * 10, 10, "s16") == 0.0 and model.level_dbfs(10.0, 10, "f32") == 0.0
    assert model.level_dbfs(0.0, 10) is None and model.level_dbfs(0.0, 0) is None


def test_batcher_gives_a_request_the_marks_of_its_own_rows():
    other = [_sent(0.75, [1, 1], [2])]
    alone_audio, alone = orchestrator.easy_synthesize_marks(FakePipe(), REQUEST, STYLES, noise_seed=1, options=orchestrator.SynthesizeOptions(sample_rate=44100))
    pipe = FakePipe()
    rb = batcher.RequestBatcher(pipe, start=False, clock=lambda: 0.0, max_wait_ms=1000.0)
    f0 = rb.submit(other, STYLES, noise_seed=7)
    f1 = rb.submit(REQUEST, STYLES, noise_seed=1, marks=True)
    f2 = rb.submit(other, STYLES, noise_seed=8, marks=True)
    rb.start()
    rb.close()
    assert pipe.runs == 1
    assert isinstance(f0.result(0), bytes)                       # a request without marks is answered as before
    audio, mk = f1.result(0)
    assert audio == alone_audio and mk == alone                  # rows 1..2 of the shared run, on the request's own timeline
    assert [c["rows"] for c in pipe.calls if c["marks"]] == [[1, 2], [3]]
    assert f2.result(0)[1]["tokens"][0]["start"] == 0


def test_rest_synthesize_marks_and_the_untouched_routes():
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient
    from sbv2_api_amd import rest
    wav = orchestrator.array_to_wav(np.zeros((1, 1, 10), np.float32))
    marks = {"sample_rate": 16000, "tokens": [{"line": 0, "index": 0, "phone": 3, "start": 0, "end": 10, "start_s": 0.0, "end_s": 10 / 16000,
                                                "level_dbfs": None, "peak": 0.0}],
             "words": [{"line": 0, "index": 0, "start": 0, "end": 10, "start_s": 0.0, "end_s": 10 / 16000}]}

    class Pieces:
        def __init__(self):
            self.marks, self.it = marks, iter([b"ab", b"cd"])

        def __iter__(self):
            return self

        def __next__(self):
            return next(self.it)

    class H:
        calls = []

        def easy_synthesize(self, ident, text, style_id, speaker_id, options):
            return wav

        def easy_synthesize_marks(self, ident, text, style_id, speaker_id, options):
            if ident != "m":
                raise RuntimeError(f"model not found: {ident}")
            self.calls.append((text, options.sample_rate, options.encoding, options.envelope_hz))
            return wav, marks

        def easy_synthesize_stream(self, ident, text, style_id, speaker_id, options):
            return Pieces()

    h = H()
    c = TestClient(rest.make_app(h), raise_server_exceptions=False)
    r = c.post("/synthesize", json={"text": "x", "ident": "m"})
    assert r.status_code == 200 and r.headers["content-type"] == "audio/wav" and r.content == wav     # /synthesize is untouched
    r = c.post("/synthesize_marks", json={"text": "x", "ident": "m", "sample_rate": 16000, "encoding": "s16", "envelope_hz": 100})
    assert r.status_code == 200 and r.headers["content-type"] == "application/json"
    j = r.json()
    assert set(j) == {"audio", "media_type", "sample_rate", "marks"}
    assert base64.b64decode(j["audio"]) == wav and j["media_type"] == "audio/wav" and j["sample_rate"] == 16000 and j["marks"] == marks
    assert h.calls[-1] == ("x", 16000, "s16", 100)
    assert c.post("/synthesize_marks", json={"text": "x", "ident": "m", "encoding": "flac"}).json()["media_type"] == "audio/flac"
    assert h.calls[-1][3] is None
    r = c.post("/synthesize_marks", json={"text": "x", "ident": "nope"})
    assert r.status_code == 500 and r.text == "Something went wrong: model not found: nope"
    r = c.post("/synthesize_stream", json={"text": "x", "ident": "m"})
    assert r.content == b"abcd" and "x-speech-marks" not in r.headers                                   # unchanged unless asked for
    r = c.post("/synthesize_stream", json={"text": "x", "ident": "m", "marks": True})
    assert r.content == b"abcd"
    assert json.loads(r.headers["x-speech-marks"]) == {"sample_rate": 16000, "tokens": [[0, 0, 3, 0, 10]], "words": [[0, 0, 0, 10]]}


# ---- GPU: the kernel, launch by launch ------------------------------------------------------------------------------------------------------------------

SEG_LENS = [0, 1, 63, 64, 65, 255, 256, 257, 4097, 0, 3, 60000]
N_SAMPLES = 70000


def _segments():
    """Adjacent segments of SEG_LENS from sample 0, then the rest up to N_SAMPLES: every sample is read once, starts odd and even."""
    edges = np.concatenate([[0], np.cumsum(SEG_LENS)])
    assert edges[-1] < N_SAMPLES
    st, en = list(edges[:-1]), list(edges[1:])
    st.append(edges[-1]); en.append(N_SAMPLES)
    st, en = np.array(st, np.int64), np.array(en, np.int64)
    assert (st % 2 == 1).any() and (st % 2 == 0).any() and en[-1] == N_SAMPLES
    return st, en


def _guarded_levels(x, st, en):
    l = _lib.lib()
    n = len(st)
    ss, pk = np.full(n + 2, 77.0), np.full(n + 2, 77.0)
    q = lambda a: C.cast(a.ctypes.data + 8, f64p)
    _lib.check(l.sbv2_debug_segment_levels(0, x.ctypes.data_as(C.c_void_p), int(x.dtype == np.int16), x.size, st.ctypes.data_as(_lib.i64p),
                                           en.ctypes.data_as(_lib.i64p), n, q(ss), q(pk)))
    assert ss[0] == ss[-1] == pk[0] == pk[-1] == 77.0, "guard words"
    return ss[1:-1], pk[1:-1]


@gpu
@pytest.mark.parametrize("dtype", ["s16", "f32"])
def test_segment_levels_kernel(dtype):
    rng = np.random.default_rng(2026)
    st, en = _segments()
    if dtype == "s16":
        x = rng.integers(-32768, 32768, N_SAMPLES).astype(np.int16)
        x[100:400] = 32767; x[5000:9500] = -32767; x[20000:68000:2] = 32767; x[20001:68000:2] = -32767
    else:
        x = (rng.standard_normal(N_SAMPLES) * np.exp(rng.uniform(-12, 2, N_SAMPLES))).astype(np.float32)
    ss, pk = _guarded_levels(x, st, en)
    check_levels(x, st, en, ss, pk, f"kernel {dtype}")
    assert ss[0] == 0.0 and pk[0] == 0.0                      # the empty segment
    again = _guarded_levels(x, st, en)
    assert again[0].tobytes() == ss.tobytes() and again[1].tobytes() == pk.tobytes()
    # the order of a segment's sum depends on its length alone: the same samples elsewhere in the buffer give the same bits
    y = np.concatenate([np.zeros(3, x.dtype), x])
    moved = _guarded_levels(y, st + 3, en + 3)
    assert moved[0].tobytes() == ss.tobytes() and moved[1].tobytes() == pk.tobytes()
    # a segment outside the buffer is refused before anything runs
    assert _lib.lib().sbv2_debug_segment_levels(0, x.ctypes.data_as(C.c_void_p), int(dtype == "s16"), x.size, st.ctypes.data_as(_lib.i64p),
                                                (en + 1).ctypes.data_as(_lib.i64p), len(st), ss.ctypes.data_as(f64p), pk.ctypes.data_as(f64p)) != 0


# ---- GPU: the pipeline --------------------------------------------------------------------------------------------------------------------------------

FORCED = [[1, 3, 0, 2, 1, 5, 0, 4, 1], [2, 0, 1, 1, 3, 0, 0, 2, 6, 1, 1], [1, 4, 0, 1, 40, 2, 0, 3, 1, 1, 7, 0, 2]]
FORMATS = [model.PcmFormat(), model.PcmFormat(16000, "s16"), model.PcmFormat(48000, "f32")]


def _three(forced):
    bc, _ = weights("bert", "tiny", 3)
    vc, _ = weights("vits", "tiny", 5)
    utts = make_utts([4, 5, 6], bc, vc, seed0=811, with_bert=False)
    assert [len(u["phones"]) for u in utts] == [len(d) for d in FORCED]
    if forced:
        utts = [dict(u, forced_durations=np.array(d, np.int64)) for u, d in zip(utts, FORCED)]
    return utts


@pytest.fixture
def sessions():
    """Sessions of a test's own: a pipeline's first execution context IS its two sessions, so no other test may run on forced_run's."""
    bs, vs = model.load_model(blob("bert", "tiny", 3), True), model.load_model(blob("vits", "tiny", 5), False)
    yield bs, vs
    bs.close(); vs.close()


@pytest.fixture(scope="module")
def forced_run():
    bs, vs = model.load_model(blob("bert", "tiny", 3), True), model.load_model(blob("vits", "tiny", 5), False)
    pipe = model.Pipeline(bs, vs)
    b = pipe.prepare(_three(True), forced=True)
    pipe.run(b)
    hop = _lib.lib().sbv2_vits_hop(vs.handle)
    assert [int(n) for n in b.lens] == [hop * sum(d) for d in FORCED]
    rows = [2, 0]
    place = [777, 777 + int(b.lens[2]) + 5001]
    joined = place[1] + int(b.lens[0]) + 123
    yield pipe, b, hop, rows, place, joined
    pipe.close(); bs.close(); vs.close()


def _want_spans(hop, rows, place, rate):
    parts = [spans_np(FORCED[r], hop, p, rate) for r, p in zip(rows, place)]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


@gpu
@pytest.mark.parametrize("fmt", FORMATS, ids=repr)
def test_pipeline_marks_with_forced_durations(forced_run, fmt):
    pipe, b, hop, rows, place, joined = forced_run
    plain, _ = pipe.fetch_request(b, rows, fmt, place, joined)
    plain = plain.copy()
    out_len = model.pcm_format_length(fmt, joined)
    odd = 1000 + (out_len % 1000 == 0)
    assert out_len % odd != 0 and len(plain) == out_len
    ws, we = _want_spans(hop, rows, place, fmt.sample_rate)
    for env_hop in (fmt.sample_rate // 100, odd):
        out, stats, m = pipe.fetch_request(b, rows, fmt, place, joined, marks=True, env_hop=env_hop)
        assert stats is None and out.dtype == plain.dtype and out.tobytes() == plain.tobytes()     # the audio of the same fetch without marks
        np.testing.assert_array_equal(m.start, ws)
        np.testing.assert_array_equal(m.end, we)
        for r, p in zip(rows, place):   # ... which is also what the library's own host function says
            s, e = model.marks_spans(FORCED[r], hop, p, fmt)
            k = 0 if r == rows[0] else len(FORCED[rows[0]])
            np.testing.assert_array_equal(m.start[k:k + len(s)], s)
            np.testing.assert_array_equal(m.end[k:k + len(e)], e)
        assert m.end[len(FORCED[2]) - 1] == model.pcm_format_length(fmt, place[0] + int(b.lens[2])) and m.start[0] == model.pcm_format_length(fmt, place[0])
        check_levels(out, m.start, m.end, m.sumsq, m.peak, f"tokens {fmt!r}")
        assert (m.sumsq[m.start == m.end] == 0).all() and (m.sumsq[m.end - m.start > 100] > 0).any()
        fs = np.arange(0, out_len, env_hop)
        assert len(m.env_sumsq) == len(fs) == -(-out_len // env_hop)
        check_levels(out, fs, np.minimum(fs + env_hop, out_len), m.env_sumsq, m.env_peak, f"envelope {env_hop} {fmt!r}")
    # timing only: the spans without levels
    out, _, m = pipe.fetch_request(b, rows, fmt, place, joined, marks=True, levels=False)
    assert out.tobytes() == plain.tobytes() and m.sumsq is None and m.env_sumsq is None
    np.testing.assert_array_equal(m.start, ws)


@gpu
@pytest.mark.parametrize("gain", [model.Loudness(-23.0, -1.0), model.Limiter(-16.0, -1.0, 6.0)], ids=["loudness", "limiter"])
def test_pipeline_marks_with_predicted_durations_are_post_gain_and_repeatable(sessions, gain):
    bs, vs = sessions
    pipe = model.Pipeline(bs, vs)
    try:
        b = pipe.prepare(_three(False), sdp_ratio=0.2, noise_scale=0.6, noise_scale_w=0.8, noise_seed=31)
        pipe.run(b)
        hop = _lib.lib().sbv2_vits_hop(vs.handle)
        rows = [1, 2, 0]
        place, joined = orchestrator.joined_placement([int(b.lens[r]) for r in rows], [0, 1, 2], 4)
        for fmt in (model.PcmFormat(16000, "s16"), model.PcmFormat(48000, "f32")):
            plain, pstats = pipe.fetch_request(b, rows, fmt, place, joined, gain=gain)
            plain, pstats = plain.copy(), pstats.copy()
            out, stats, m = pipe.fetch_request(b, rows, fmt, place, joined, gain=gain, marks=True, env_hop=fmt.sample_rate // 100)
            assert out.tobytes() == plain.tobytes() and stats.tobytes() == pstats.tobytes()
            # the spans partition each row's delivered range
            k = 0
            for r, p in zip(rows, place):
                T = int(b.t_lens[r])
                s, e = m.start[k:k + T], m.end[k:k + T]
                assert int(b.lens[r]) >= hop
                assert s[0] == model.pcm_format_length(fmt, p) and e[-1] == model.pcm_format_length(fmt, p + int(b.lens[r]))
                np.testing.assert_array_equal(e[:-1], s[1:])
                assert (e >= s).all()
                k += T
            assert k == len(m.start)
            check_levels(out, m.start, m.end, m.sumsq, m.peak, f"post-gain tokens {fmt!r}")
            fs = np.arange(0, len(out), m.env_hop)
            check_levels(out, fs, np.minimum(fs + m.env_hop, len(out)), m.env_sumsq, m.env_peak, f"post-gain envelope {fmt!r}")
            raw, _, m0 = pipe.fetch_request(b, rows, fmt, place, joined, marks=True)
            if stats[2] != 0.0 and raw.tobytes() != out.tobytes():      # a gain was applied: the levels moved with the samples
                assert m0.sumsq.tobytes() != m.sumsq.tobytes()
            np.testing.assert_array_equal(m0.start, m.start)
            out2, stats2, m2 = pipe.fetch_request(b, rows, fmt, place, joined, gain=gain, marks=True, env_hop=fmt.sample_rate // 100)
            assert out2.tobytes() == out.tobytes() and stats2.tobytes() == stats.tobytes()
            for x, y in zip(m.arrays(), m2.arrays()):
                assert x.tobytes() == y.tobytes()
    finally:
        pipe.close()


@gpu
def test_marks_behind_the_flac_sink(forced_run):
    pipe, b, hop, rows, place, joined = forced_run
    fmt = model.PcmFormat(16000, "s16")
    env_hop = 160
    pcm, _, mp = pipe.fetch_request(b, rows, fmt, place, joined, marks=True, env_hop=env_hop)
    pcm = pcm.copy()
    plain, _ = pipe.fetch_request(b, rows, fmt, place, joined, flac=True)
    fl, _, mf = pipe.fetch_request(b, rows, fmt, place, joined, flac=True, marks=True, env_hop=env_hop)
    assert fl == plain
    d = R.read(fl)
    assert d["rate"] == 16000
    x = np.asarray(d["samples"], np.int16)
    np.testing.assert_array_equal(x, pcm)
    check_levels(x, mf.start, mf.end, mf.sumsq, mf.peak, "flac tokens")
    fs = np.arange(0, len(x), env_hop)
    check_levels(x, fs, np.minimum(fs + env_hop, len(x)), mf.env_sumsq, mf.env_peak, "flac envelope")
    for a, c in zip(mp.arrays(), mf.arrays()):
        assert a.tobytes() == c.tobytes()


@gpu
def test_marks_capacity_refusals_write_nothing_and_keep_the_ticket(forced_run):
    pipe, b, hop, rows, place, joined = forced_run
    l = _lib.lib()
    fmt = model.PcmFormat(16000, "s16")
    ntok, env_hop = sum(len(FORCED[r]) for r in rows), 160
    nenv = -(-model.pcm_format_length(fmt, joined) // env_hop)
    rw, pl = np.asarray(rows, np.int32), np.asarray(place, np.int64)
    req = _lib.Sbv2FetchRequest(rw.ctypes.data_as(C.POINTER(C.c_int32)), len(rw), pl.ctypes.data_as(_lib.i64p), joined, C.pointer(fmt.c), None, None, 0)

    def call(m):
        dst, got = np.full(1 << 18, 77, np.uint8), C.c_int64(-5)
        rc = l.sbv2_pipeline_fetch_request_marks(pipe.h, b.ticket, C.byref(req), dst.ctypes.data, dst.nbytes, C.byref(got), None, C.byref(m.c))
        return rc, l.sbv2_last_error().decode(), bool((dst == 77).all() and got.value == -5), dst, got.value

    for m, word in ((_c_marks(ntok - 1, nenv, env_hop), "token arrays too small"), (_c_marks(ntok, nenv - 1, env_hop), "envelope arrays too small")):
        rc, msg, clean, _, _ = call(m)
        assert rc != 0 and word in msg and clean and m.untouched(), (word, rc, msg)
    m = _c_marks(ntok, nenv, env_hop)
    rc, msg, _, dst, n = call(m)                  # the ticket is still fetchable, and exact capacities suffice
    assert rc == 0, msg
    assert m.guards() and m.c.n_tokens == ntok and m.c.n_env == nenv
    ref, _, mr = pipe.fetch_request(b, rows, fmt, place, joined, marks=True, env_hop=env_hop)
    assert dst[:2 * n].tobytes() == ref.tobytes()
    assert m.sumsq[1:-1].tobytes() == mr.sumsq.tobytes() and m.esumsq[1:-1].tobytes() == mr.env_sumsq.tobytes()
    np.testing.assert_array_equal(m.start[1:-1], mr.start)


@gpu
@pytest.mark.parametrize("flac", [False, True], ids=["format", "flac"])
def test_stream_marks(forced_run, sessions, flac):
    pipe, b, hop, rows, place, joined = forced_run
    fmt = model.PcmFormat(48000, "s16" if flac else "f32")
    _, _, mp = pipe.fetch_request(b, [2], fmt, [0], int(b.lens[2]), marks=True, levels=False)     # the pipeline's spans of that row at place 0
    bs, vs = sessions
    if True:
        st = model.StreamHandle(bs, vs, _three(True)[2], 16, fmt=fmt, flac=flac, forced=True)
        try:
            assert sum(FORCED[2]) > 3 * 16                 # several chunks
            s0, e0 = st.marks()                            # before the first chunk
            np.testing.assert_array_equal(s0, mp.start)
            np.testing.assert_array_equal(e0, mp.end)
            delivered = 0
            while True:
                c = st.next()
                if c is None:
                    break
                delivered += 0 if flac else len(c)
            delivered = st.samples_taken if flac else delivered
            s1, e1 = st.marks()                            # after the last
            np.testing.assert_array_equal(s1, s0)
            np.testing.assert_array_equal(e1, e0)
            assert delivered == e0[-1] == st.total_samples
            l = _lib.lib()
            got = C.c_int64(-5)
            assert l.sbv2_stream_marks(st.h, s0.ctypes.data_as(_lib.i64p), e0.ctypes.data_as(_lib.i64p), len(s0) - 1, C.byref(got)) != 0
            assert b"too small" in l.sbv2_last_error() and got.value == -5
        finally:
            st.close()
        plain = model.StreamHandle(bs, vs, _three(True)[2], 16, forced=True)   # no format: native samples
        try:
            s, e = plain.marks()
            ws, we = spans_np(FORCED[2], hop, 0, 44100)
            np.testing.assert_array_equal(s, ws)
            np.testing.assert_array_equal(e, we)
        finally:
            plain.close()


@contextlib.contextmanager
def _size_independent_dispatch():
    """The dispatch on which a batch row equals its call alone bit for bit (tests/test_gpu_parity.py): no launch shapes chosen by batch size."""
    lib = _lib.lib()
    prev_clx, prev_ks = lib.sbv2_debug_set_clx(0), lib.sbv2_debug_set_ksplit(0)
    try:
        yield
    finally:
        lib.sbv2_debug_set_clx(prev_clx)
        lib.sbv2_debug_set_ksplit(prev_ks)


@gpu
def test_batcher_marks_equal_the_request_alone(sessions):
    bs, vs = sessions
    bc, _ = weights("bert", "tiny", 3)
    vc, _ = weights("vits", "tiny", 5)
    keys = ("input_ids", "word2ph", "phones", "tones", "langs")
    sents = lambda sizes, seed0: [{k: u[k] for k in keys} for u in make_utts(sizes, bc, vc, seed0=seed0, with_bert=False)]
    sv = synth.hash_normal(77, 3 * vc["style_dim"]).reshape(3, -1).astype(np.float32) * 0.1
    SO = orchestrator.SynthesizeOptions
    reqs = [(sents([7, 15], 151), SO(sdp_ratio=0.3, length_scale=1.1, sample_rate=16000, encoding="s16", envelope_hz=100), 4242),
            (sents([4, 9], 171), SO(sdp_ratio=0.8, length_scale=0.9), 99)]
    pipe = model.Pipeline(bs, vs)
    try:
        with _size_independent_dispatch():
            rb = batcher.RequestBatcher(pipe, start=False, max_wait_ms=1000.0)
            futs = [rb.submit(s, sv, 1, 0, o, noise_seed=seed, marks=True) for s, o, seed in reqs]
            rb.start()
            rb.close()
            for (s, o, seed), f in zip(reqs, futs):
                audio, mk = f.result(0)
                alone_audio, alone = orchestrator.easy_synthesize_marks(pipe, s, sv, 1, 0, o, noise_seed=seed)
                assert [(t["start"], t["end"]) for t in mk["tokens"]] == [(t["start"], t["end"]) for t in alone["tokens"]]
                assert audio == alone_audio
                assert mk == alone
                assert audio == orchestrator.easy_synthesize(pipe, s, sv, 1, 0, o, noise_seed=seed)      # and the audio is easy_synthesize's
                assert len(mk["tokens"]) == sum(len(x["phones"]) for x in s) and ("envelope" in mk) == (o.envelope_hz is not None)
    finally:
        pipe.close()
