"""A stream over the n rows of one batched forward (sbv2_stream_begin_request): a multi-sentence request as one signal, sentence by sentence.

CPU: the exported symbols, the minimum gap, the timeline arithmetic against a numpy restatement, the orchestrator / REST plumbing on stubs.
GPU: the stream_windows launch against numpy, and the request stream on the tiny models (hop 16) bit for bit against the joined fetch of a
pipeline run of the same batch, for plain formats, FLAC, the level stream and the marks; one test on the full model."""
import ctypes as C
import io
import math

import numpy as np
import pytest

import flac_reader as R
from helpers import blob, make_utts, weights
from sbv2_api_amd import _lib, model, orchestrator, synth

MIN_GAP = {8000: 354, 16000: 178, 22050: 128, 24000: 118, 32000: 90, 44100: 0, 48000: 64}
F32_ROUNDING_DEV = 1.192e-07   # the single-utterance level stream's tolerances (test_stream_level.py)
S16_STEP = 1


def _geometry(rate):
    g = math.gcd(rate, 44100)
    return rate // g, 44100 // g


def J(a, rate):
    L, M = _geometry(rate)
    return 0 if a <= 0 else -(-a * L // M)


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------------

def test_abi_exports_the_request_stream_symbols():
    l = _lib.lib()
    for name in ("sbv2_stream_begin_request", "sbv2_stream_min_gap", "sbv2_stream_timeline", "sbv2_stream_layout", "sbv2_stream_call_bound",
                 "sbv2_debug_stream_windows"):
        assert name in _lib.SYMBOLS and getattr(l, name) is not None
    assert C.sizeof(_lib.Sbv2StreamRequest) == 3 * C.sizeof(C.c_void_p) + 8


def test_min_gap_values_and_rule():
    assert model.stream_min_gap(None) == 0
    for rate, want in MIN_GAP.items():
        got = model.stream_min_gap(model.PcmFormat(rate, "s16"))
        taps, L, M = model.pcm_format_taps(rate)
        half = (len(taps) - 1) // 2
        assert (L, M) == _geometry(rate)
        assert got == want == 2 * -(-half // L), (rate, got, half, L)
    bad = model.PcmFormat(44100, "f32")
    bad.c.sample_rate = 12345
    assert _lib.lib().sbv2_stream_min_gap(C.byref(bad.c)) == -1 and b"sample rate" in _lib.lib().sbv2_last_error()


def ref_timeline(frames, gaps, hop, chunk, rate):
    """The contract of include/sbv2_hip.h restated: (place, joined, call_samples)."""
    n = len(frames)
    lens = [f * hop for f in frames]
    place = [0] * n
    for i in range(1, n):
        place[i] = place[i - 1] + lens[i - 1] + gaps[i - 1]
    joined = place[-1] + lens[-1] + gaps[-1]
    m = [place[i] + lens[i] + gaps[i] // 2 for i in range(n - 1)] + [joined]
    calls = []
    for i in range(n):
        k = -(-frames[i] // chunk)
        for c in range(k):
            a = place[i] + c * chunk * hop
            b = place[i] + min((c + 1) * chunk, frames[i]) * hop
            if c == 0:
                a = m[i - 1] if i else 0
            if c == k - 1:
                b = m[i]
            calls.append(J(b, rate) - J(a, rate))
    return place, joined, calls


@pytest.mark.parametrize("rate", (44100, 48000, 24000, 8000))
def test_timeline_against_numpy(rate):
    fmt = model.PcmFormat(rate, "s16")
    mg = MIN_GAP[rate]
    frames = [1, 7, 16, 17, 50]
    for hop in (16, 512):
        for chunk in (16, 50):
            for gaps in ([mg] * 4 + [0], [333 if 333 >= mg else mg + 1] * 4 + [22050], [22050, mg, 333 + mg | 1, 22050, 0], [mg, 22050, mg, 441000, 22050]):
                place, joined, calls = model.stream_timeline(frames, gaps, hop, chunk, fmt)
                rp, rj, rc = ref_timeline(frames, gaps, hop, chunk, rate)
                assert list(place) == rp and joined == rj and list(calls) == rc, (hop, chunk, gaps)
                assert len(calls) == sum(-(-f // chunk) for f in frames) and int(calls.sum()) == J(joined, rate)
                assert (calls > 0).all()
    # one row, no gap: the single-utterance stream's chunks
    place, joined, calls = model.stream_timeline([50], [0], 512, 16, fmt)
    edges = [J(min(c * 16, 50) * 512, rate) for c in range(5)]
    assert list(place) == [0] and joined == 50 * 512 and list(calls) == list(np.diff(edges))


def test_timeline_refusals():
    f48 = model.PcmFormat(48000, "s16")
    with pytest.raises(model.Sbv2Error, match="minimum gap of 64"):
        model.stream_timeline([20, 20], [63, 0], 16, 16, f48)
    model.stream_timeline([20, 20], [64, 0], 16, 16, f48)
    model.stream_timeline([20, 20], [0, 0], 16, 16, None)          # at 44.1 kHz sentences may abut
    model.stream_timeline([20, 20], [64, 3], 16, 16, f48)          # the trailing gap has no minimum
    with pytest.raises(model.Sbv2Error, match=r"outside \[0, 441000\]"):
        model.stream_timeline([20, 20], [-1, 0], 16, 16, None)
    with pytest.raises(model.Sbv2Error, match=r"outside \[0, 441000\]"):
        model.stream_timeline([20, 20], [100, 441001], 16, 16, None)
    with pytest.raises(model.Sbv2Error, match="at least one row"):
        model.stream_timeline([], [], 16, 16, None)
    l = _lib.lib()
    fr, gp = np.array([40, 40], np.int64), np.array([100, 0], np.int64)
    place, calls, joined, nc = np.zeros(2, np.int64), np.full(5, -7, np.int64), C.c_int64(), C.c_int64()
    p = lambda a: a.ctypes.data_as(_lib.i64p)
    assert l.sbv2_stream_timeline(p(fr), p(gp), 2, 16, 16, None, p(place), C.byref(joined), p(calls), 5, C.byref(nc)) != 0
    assert b"too small" in l.sbv2_last_error() and nc.value == 6 and (calls == -7).all()
    assert l.sbv2_stream_timeline(p(fr), p(gp), 2, 16, 16, None, p(place), C.byref(joined), None, 0, C.byref(nc)) == 0 and nc.value == 6
    assert l.sbv2_stream_timeline(p(fr), None, 2, 16, 16, None, p(place), C.byref(joined), None, 0, C.byref(nc)) != 0


class _StubHandle:
    seen = []
    total_samples = 10

    def __init__(self, bert, vits, utt, chunk_frames, fmt=None, flac=False, level=None, **kw):
        type(self).seen.append((utt, kw))
        self.level, self.chunks = level, [np.ones(10, np.float32)]
        self.n = sum(len(u["phones"]) for u in utt) if isinstance(utt, list) else len(utt["phones"])

    def marks(self):
        return np.arange(self.n, dtype=np.int64), np.arange(1, self.n + 1, dtype=np.int64)

    def next(self):
        return self.chunks.pop(0) if self.chunks else None

    def close(self):
        pass


def test_split_hands_the_rows_and_gaps_of_joined_placement(monkeypatch):
    monkeypatch.setattr(model, "StreamHandle", _StubHandle)
    styles = np.zeros((2, 4), np.float32)
    s = [{"phones": [1, 2, 3][:k], "word2ph": [k]} for k in (1, 2, 3)]
    for lines, live in (([s[0], None, s[1], s[2]], [0, 2, 3]), ([s[0], None], [0])):
        _StubHandle.seen.clear()
        st = orchestrator.easy_synthesize_stream(None, None, lines, styles, 1, 7, None, noise_seed=5, split=True)
        (utt, kw), = _StubHandle.seen
        rows = [lines[i] for i in live]
        assert isinstance(utt, list) and [u["phones"] for u in utt] == [r["phones"] for r in rows]
        assert all(u["sid"] == 7 and u["style"].shape == (4,) for u in utt) and kw["noise_seed"] == 5
        # the gaps are what joined_placement puts between rows of any lengths, and behind the last one
        lens = [1000 * (k + 1) for k in range(len(rows))]
        place, joined = orchestrator.joined_placement(lens, live, len(lines))
        ends = [p + n for p, n in zip(place, lens)]
        assert kw["gaps"] == [b - a for a, b in zip(ends, place[1:] + [joined])]
        assert kw["gaps"][-1] == (orchestrator.SENTENCE_GAP if lines[-1] is None else 0)
        assert [t["line"] for t in st.marks["tokens"]] == [i for i in live for _ in lines[i]["phones"]]
        assert b"".join(st)[:4] == b"RIFF"
    # split=False: one utterance, a dict, no gaps; a second live sentence is still refused
    _StubHandle.seen.clear()
    orchestrator.easy_synthesize_stream(None, None, [s[0], None], styles, 1, 7, None, noise_seed=5)
    (utt, kw), = _StubHandle.seen
    assert isinstance(utt, dict) and "gaps" not in kw
    with pytest.raises(model.Sbv2Error, match="one utterance"):
        orchestrator.easy_synthesize_stream(None, None, [s[0], None, s[1]], styles, 1, 7, None, noise_seed=5)
    with pytest.raises(model.Sbv2Error, match="one utterance"):
        orchestrator.easy_synthesize_stream(None, None, [s[0], None, s[1]], styles, 1, 7, None, noise_seed=5, split=False)


def test_rest_passes_split_sentences_to_the_holder():
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient
    from sbv2_api_amd import rest

    class Pieces:
        marks = {"sample_rate": 44100, "tokens": [{"line": 2, "index": 0, "phone": 5, "start": 0, "end": 9}], "words": []}

        def __iter__(self):
            return iter([b"RIFF", b"one"])

    class Holder:
        def __init__(self):
            self.split = []

        def models(self):
            return ["m"]

        def easy_synthesize_stream(self, ident, text, style_id, speaker_id, options, **kw):
            self.split.append((text, kw))      # (what the route names, not what a default of this stub would fill in)
            return Pieces()

    h = Holder()
    c = TestClient(rest.make_app(h))
    r = c.post("/synthesize_stream", json={"text": "a\n\nb", "ident": "m"})
    assert r.status_code == 200 and r.content == b"RIFFone" and h.split[-1] == ("a\n\nb", {})
    r = c.post("/synthesize_stream", json={"text": "a\n\nb", "ident": "m", "split_sentences": True, "marks": True})
    assert r.status_code == 200 and h.split[-1] == ("a\n\nb", {"split": True})
    assert '"tokens":[[2,0,5,0,9]]' in r.headers["x-speech-marks"]
    # False is sent as the holder's own default: the keyword is left out, so a holder written before it (five-argument signature) still serves
    r = c.post("/synthesize_stream", json={"text": "a", "ident": "m", "split_sentences": False})
    assert r.status_code == 200 and h.split[-1] == ("a", {})

    class OldHolder(Holder):
        def easy_synthesize_stream(self, ident, text, style_id, speaker_id, options):
            self.split.append((text, None))
            return Pieces()

    old = OldHolder()
    c = TestClient(rest.make_app(old))
    assert c.post("/synthesize_stream", json={"text": "a", "ident": "m"}).status_code == 200 and old.split == [("a", None)]
    r = c.post("/synthesize_stream", json={"text": "a", "ident": "m", "split_sentences": True})
    assert r.status_code == 500 and "split" in r.text      # asked of a holder that cannot: an error, never a silent unsplit answer


# ---- GPU: the window launch ---------------------------------------------------------------------------------------------------------------

def _stream_windows(z, table, W, conds):
    C_, L = z.shape
    nwin, (nrows, cd) = len(table), conds.shape
    z = np.ascontiguousarray(z, np.float32)
    tab = np.ascontiguousarray(table, np.int32)
    conds = np.ascontiguousarray(conds, np.float32)
    zo, mo, co = np.zeros((nwin, C_, W), np.float32), np.zeros((nwin, W), np.uint8), np.zeros((nwin, cd), np.float32)
    f = lambda a: a.ctypes.data_as(_lib.f32p)
    _lib.check(_lib.lib().sbv2_debug_stream_windows(0, f(z), C_, L, tab.ctypes.data_as(C.POINTER(C.c_int32)), W, nwin, f(conds), nrows, cd, f(zo),
                                                    mo.ctypes.data, f(co)))
    return zo, mo, co


@pytest.mark.gpu
@pytest.mark.parametrize("W", (20, 300))
def test_stream_windows_equals_numpy(W):
    """Exact: the launch only copies.  The rows lie in one plane with NaN between and around them; no NaN may reach the output, and the hook
    fails the call when a byte outside the output is written."""
    rng = np.random.default_rng(W)
    halo = 4
    for row_lens in ((37, 1), (W + 9, 1, 2 * W + 5)):
        starts, pos = [], 3
        for n in row_lens:
            starts.append(pos)
            pos += n + 5
        z = np.full((3, pos + 2), np.nan, np.float32)
        for s, n in zip(starts, row_lens):
            z[:, s:s + n] = rng.standard_normal((3, n)).astype(np.float32)
        conds = rng.standard_normal((len(row_lens), 6)).astype(np.float32)
        # every kind of window: before a row (first = -halo), straddling its end, wholly past the end, on the 1-frame row, past the request
        kinds = []
        for r, (s, n) in enumerate(zip(starts, row_lens)):
            kinds += [(s, n, -halo, r), (s, n, max(n - W // 2, 0), r), (s, n, n + 3, r), (s, n, 0, r), (s, n, -W - 1, r)]
        kinds.append((0, 0, 0, 0))
        for nwin in (1, 2, 8, 16):
            for rep in range(2):
                pick = rng.permutation(len(kinds))[:nwin] if nwin <= len(kinds) else rng.integers(0, len(kinds), nwin)
                table = [kinds[i] for i in pick]
                if nwin >= 2 and rep == 0:   # two windows of one replay from different rows with different cond vectors
                    table[0], table[1] = (starts[0], row_lens[0], -halo, 0), (starts[1], row_lens[1], -halo, 1)
                zo, mo, co = _stream_windows(z, table, W, conds)
                assert not np.isnan(zo).any() and not np.isnan(co).any()
                for w, (z0, n, first, row) in enumerate(table):
                    q = first + np.arange(W)
                    ok = (q >= 0) & (q < n)
                    want = np.zeros((3, W), np.float32)
                    want[:, ok] = z[:, z0 + q[ok]]
                    assert np.array_equal(zo[w].view(np.uint32), want.view(np.uint32)), (W, nwin, w, table[w])
                    assert np.array_equal(mo[w], ok.astype(np.uint8)), (W, nwin, w)
                    assert np.array_equal(co[w], conds[row] if n > 0 else np.zeros(6, np.float32)), (W, nwin, w)
    with pytest.raises(model.Sbv2Error, match="outside the plane"):
        _stream_windows(z, [(pos, 5, 0, 0)], W, conds)


# ---- GPU: the request stream on the tiny models -------------------------------------------------------------------------------------------

def _tiny():
    bc, _ = weights("bert", "tiny", 3)
    vc, _ = weights("vits", "tiny", 5)
    return bc, vc, model.load_model(blob("bert", "tiny", 3), True), model.load_model(blob("vits", "tiny", 5), False)


def _hop(vs):
    return _lib.lib().sbv2_vits_hop(vs.handle)


CASES = ((dict(forced=True)), (dict(sdp_ratio=0.2, noise_scale=0.667, noise_scale_w=0.8, noise_seed=5)))


@pytest.fixture(scope="module")
def tiny_run():
    """The tiny models, a pipeline on them and the three rows (40, 7, 23 tokens) every test below streams."""
    bc, vc, bs, vs = _tiny()
    utts = make_utts([40, 7, 23], bc, vc, seed0=171, with_bert=False)
    pipe = model.Pipeline(bs, vs)
    yield dict(bc=bc, vc=vc, bs=bs, vs=vs, utts=utts, pipe=pipe)
    pipe.close(); bs.close(); vs.close()


def _joined(pipe, utts, kw, fmt, gaps):
    """(batch, lens, place, joined_len) of a pipeline run of the rows, placed as the stream's contract places them; the caller fetches from it
    before a stream reuses the handles' context."""
    b = pipe.prepare(utts, **kw)
    pipe.run(b)
    lens = [int(n) for n in b.lens]
    place = [0]
    for n, g in zip(lens[:-1], gaps[:-1]):
        place.append(place[-1] + n + g)
    joined = place[-1] + lens[-1] + gaps[-1]
    return b, lens, place, joined


def _take_all(st):
    parts = []
    while (c := st.next()) is not None:
        parts.append(c)
    return parts


def _gap_sets(fmt):
    mg = model.stream_min_gap(fmt)
    return ((1000, 333, 0), (mg, mg, 22050))


@pytest.mark.gpu
@pytest.mark.parametrize("case", (0, 1))
def test_request_stream_tiny_equals_joined_fetch_bit_for_bit(tiny_run, case):
    t = tiny_run
    bs, vs, pipe, utts, kw = t["bs"], t["vs"], t["pipe"], t["utts"], CASES[case]
    hop = _hop(vs)
    fmts = (None, model.PcmFormat(44100, "f32"), model.PcmFormat(48000, "s16"), model.PcmFormat(24000, "s16"), model.PcmFormat(48000, "mulaw"))
    two_rows_in_a_replay, short_row = {n: False for n in range(2, 17)}, False
    for fmt in fmts:
        ff = fmt or model.PcmFormat(44100, "f32")
        for gaps in _gap_sets(fmt):
            b, lens, place, joined = _joined(pipe, utts, kw, ff, gaps)
            want = pipe.fetch_format(b, ff, place, joined)[0]      # (fetched before a stream reuses the handles' context)
            frames = [n // hop for n in lens]
            for chunk in (16, 50, 64):
                st = model.StreamHandle(bs, vs, utts, chunk, fmt=fmt, gaps=gaps, **kw)
                pl, ln, jl = st.layout()
                assert list(pl) == place and list(ln) == lens and jl == joined and st.total_samples == want.size
                tp, tj, calls = model.stream_timeline(frames, gaps, hop, chunk, fmt)
                assert list(tp) == place and tj == joined
                assert st.buf.nbytes >= int(calls.max()) * np.dtype(ff.dtype).itemsize
                parts = _take_all(st)
                assert st.next() is None
                st.close()
                assert [p.size for p in parts] == list(calls), (fmt, gaps, chunk)
                got = np.concatenate(parts)
                assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), (fmt, gaps, chunk, int(np.argmax(got != want)))
                # coverage, from the layout: call 0 runs alone, every later replay takes the next nwin calls.  The library's choice of nwin is
                # not restated here: the cases must put two rows into one replay for EVERY burst size a plan can have (2 .. 16 windows)
                per_row = [-(-f // chunk) for f in frames]
                rows_of_calls = [r for r, k in enumerate(per_row) for _ in range(k)]
                for nwin in two_rows_in_a_replay:
                    two_rows_in_a_replay[nwin] |= any(len(set(rows_of_calls[c0:c0 + nwin])) >= 2 for c0 in range(1, len(rows_of_calls), nwin))
                short_row |= any(f < chunk for f in frames)
    assert all(two_rows_in_a_replay.values()) and short_row, two_rows_in_a_replay
    with pytest.raises(model.Sbv2Error, match="halo"):
        model.StreamHandle(bs, vs, utts, 16, fmt=model.PcmFormat(16000, "s16"), gaps=(178, 178, 0), **kw)


@pytest.mark.gpu
def test_one_row_request_equals_begin_format_call_by_call(tiny_run):
    t = tiny_run
    bs, vs, u = t["bs"], t["vs"], t["utts"][0]
    for fmt in (model.PcmFormat(48000, "s16"), model.PcmFormat(44100, "f32")):
        for chunk in (16, 50):
            a = model.StreamHandle(bs, vs, u, chunk, fmt=fmt, forced=True)
            pa, ta = _take_all(a), a.total_samples
            a.close()
            r = model.StreamHandle(bs, vs, [u], chunk, fmt=fmt, gaps=[0], forced=True)
            pr, tr = _take_all(r), r.total_samples
            r.close()
            assert ta == tr and len(pa) == len(pr)
            for x, y in zip(pa, pr):
                assert x.dtype == y.dtype and x.tobytes() == y.tobytes()


@pytest.mark.gpu
def test_request_stream_flac(tiny_run):
    t = tiny_run
    bs, vs, pipe, utts, kw = t["bs"], t["vs"], t["pipe"], t["utts"], CASES[1]
    fmt = model.PcmFormat(48000, "s16")
    gaps = (64, 333, 22050)
    b, lens, place, joined = _joined(pipe, utts, kw, fmt, gaps)
    x = pipe.fetch_format(b, fmt, place, joined)[0]
    (want,) = model.debug_flac_encode([x], 48000)
    l = _lib.lib()
    for chunk in (16, 64):
        st = model.StreamHandle(bs, vs, utts, chunk, fmt=fmt, flac=True, gaps=gaps, **kw)
        _, _, calls = model.stream_timeline([n // _hop(vs) for n in lens], gaps, _hop(vs), chunk, fmt)
        # too small a buffer: refused, nothing written, nothing consumed; the repeat succeeds
        small = np.full(8, 0x5A, np.uint8)
        nb, ns = C.c_int64(-3), C.c_int64(-3)
        assert l.sbv2_stream_next_flac(st.h, small.ctypes.data, small.nbytes, C.byref(nb), C.byref(ns)) != 0
        assert b"too small" in l.sbv2_last_error() and (small == 0x5A).all()
        pieces, taken = [], []
        while True:
            _lib.check(l.sbv2_stream_next_flac(st.h, st.buf.ctypes.data, st.buf.nbytes, C.byref(nb), C.byref(ns)))
            if ns.value == 0:
                break
            pieces.append(st.buf[:nb.value].tobytes())
            taken.append(ns.value)
        st.close()
        assert taken == list(calls)
        data = b"".join(pieces)
        assert len(data) == len(want) and data[:12] == want[:12] and data[18:] == want[18:], chunk
        got = R.read(data)
        assert got["rate"] == 48000 and got["total"] == x.size
        np.testing.assert_array_equal(got["samples"], x)


def _delivery(consumed, A):
    out, fed, sent = [], 0, 0
    for i, n in enumerate(consumed):
        fed += int(n)
        upto = fed if i == len(consumed) - 1 else max(0, fed - A)
        out.append(upto - sent)
        sent = upto
    return out


def _level_calls(st, fmt):
    l = _lib.lib()
    calls, no, nc = [], C.c_int64(), C.c_int64()
    while True:
        _lib.check(l.sbv2_stream_next_level(st.h, st.buf.ctypes.data, st.buf.nbytes, C.byref(no), C.byref(nc)))
        if nc.value == 0:
            assert no.value == 0
            break
        calls.append((st.buf[:no.value * np.dtype(fmt.dtype).itemsize].view(fmt.dtype).copy(), nc.value))
    return calls, st.level_stats()


def _active_gain(y, ceiling, over_db=9.0):
    g = ceiling - 20 * np.log10(np.abs(y).max()) + over_db
    assert -40.0 <= g <= 40.0, g
    return float(np.round(g, 2))


@pytest.mark.gpu
def test_request_stream_level(tiny_run):
    t = tiny_run
    bs, vs, pipe, utts, kw = t["bs"], t["vs"], t["pipe"], t["utts"], CASES[0]
    hop = _hop(vs)
    # 44.1 kHz f32: the resampler is the identity, so the level stream is float32(one-shot limiter of float64(joined plain)) in every bit
    fmt = model.PcmFormat(44100, "f32")
    gaps = (1000, 333, 700)
    b, lens, place, joined = _joined(pipe, utts, kw, fmt, gaps)
    plain = pipe.fetch_format(b, fmt, place, joined)[0]
    ceiling = -1.0 if np.abs(plain).max() > 0.02 else -20.0
    lv = model.StreamLevel(_active_gain(plain, ceiling), ceiling)
    (one,), st1 = model.debug_limiter_fixed([plain.astype(np.float64)], 44100, lv)
    want = one.astype(np.float32)
    assert st1[0, 0] < -3.0, st1
    frames = [n // hop for n in lens]
    for chunk in (16, 64):
        st = model.StreamHandle(bs, vs, utts, chunk, fmt=fmt, level=lv, gaps=gaps, **kw)
        _, _, cs = model.stream_timeline(frames, gaps, hop, chunk, fmt)
        calls, stats = _level_calls(st, fmt)
        assert st.total_samples == plain.size
        st.close()
        assert [n for _, n in calls] == list(cs)
        assert [d.size for d, _ in calls] == _delivery(cs, model.stream_level_lookahead(fmt))
        got = np.concatenate([d for d, _ in calls])
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (chunk, int(np.argmax(got != want)))
        assert stats == (st1[0, 0], st1[0, 1])
    # 48 kHz: against the hook on the f64 of the f32 joined fetch, the tolerances of the single-utterance case
    f32, s16 = model.PcmFormat(48000, "f32"), model.PcmFormat(48000, "s16")
    gaps = (64, 333, 700)
    b, lens, place, joined = _joined(pipe, utts, kw, f32, gaps)
    y32 = pipe.fetch_format(b, f32, place, joined)[0]
    ceiling = -1.0 if np.abs(y32).max() > 0.02 else -20.0
    lv = model.StreamLevel(_active_gain(y32, ceiling), ceiling)
    c = 10 ** (ceiling / 20)
    (one,), st1 = model.debug_limiter_fixed([y32.astype(np.float64)], 48000, lv)
    assert st1[0, 0] < -3.0
    _, _, cs = model.stream_timeline(frames, gaps, hop, 64, f32)
    st = model.StreamHandle(bs, vs, utts, 64, fmt=f32, level=lv, gaps=gaps, **kw)
    calls, stats = _level_calls(st, f32)
    st.close()
    assert [n for _, n in calls] == list(cs) and [d.size for d, _ in calls] == _delivery(cs, model.stream_level_lookahead(f32))
    got = np.concatenate([d for d, _ in calls]).astype(np.float64)
    dev = float(np.abs(got - one.astype(np.float32)).max())
    assert abs(stats[0] - st1[0, 0]) < 1e-4 and stats[1] <= c
    st = model.StreamHandle(bs, vs, utts, 64, fmt=s16, level=lv, gaps=gaps, **kw)
    calls16, stats16 = _level_calls(st, s16)
    st.close()
    assert [d.size for d, _ in calls16] == [d.size for d, _ in calls] and stats16 == stats
    got16 = np.concatenate([d for d, _ in calls16]).astype(np.int64)
    dev16 = int(np.abs(got16 - np.clip(np.rint(one * 32767.0), -32767, 32767).astype(np.int64)).max())
    print(f"request level stream 48 kHz: f32 deviation {dev:.3e}, s16 deviation {dev16} steps, depth {stats[0]:.2f} dB")
    assert dev16 <= S16_STEP and dev <= min(8 * F32_ROUNDING_DEV, 1 / 32767)


@pytest.mark.gpu
def test_request_stream_marks_equal_the_joined_fetch(tiny_run):
    t = tiny_run
    bs, vs, pipe, utts, kw = t["bs"], t["vs"], t["pipe"], t["utts"], CASES[1]
    for fmt, gaps in ((model.PcmFormat(44100, "f32"), (0, 333, 0)), (model.PcmFormat(48000, "s16"), (64, 22050, 100))):
        b, lens, place, joined = _joined(pipe, utts, kw, fmt, gaps)
        _, _, m = pipe.fetch_request(b, range(3), fmt, place, joined, marks=True, levels=False)
        st = model.StreamHandle(bs, vs, utts, 50, fmt=fmt, gaps=gaps, **kw)
        s, e = st.marks()
        st.close()
        assert np.array_equal(s, m.start) and np.array_equal(e, m.end) and s.size == sum(int(n) for n in b.t_lens)


@pytest.mark.gpu
def test_request_stream_refusals(tiny_run):
    t = tiny_run
    bs, vs, utts = t["bs"], t["vs"], t["utts"]
    kw = dict(forced=True)
    f48 = model.PcmFormat(48000, "s16")
    with pytest.raises(model.Sbv2Error, match="minimum gap of 64"):
        model.StreamHandle(bs, vs, utts, 16, fmt=f48, gaps=(64, 63, 0), **kw)
    with pytest.raises(model.Sbv2Error, match="normali"):
        model.StreamHandle(bs, vs, utts, 16, fmt=model.PcmFormat(48000, "s16", True), gaps=(64, 64, 0), **kw)
    with pytest.raises(model.Sbv2Error, match="s16"):
        model.StreamHandle(bs, vs, utts, 16, fmt=model.PcmFormat(48000, "f32"), flac=True, gaps=(64, 64, 0), **kw)
    # non-zero reserved, NULL gap_after, and sbv2_stream_begin_format with two rows: through the C ABI
    l = _lib.lib()
    b = model.Pipeline.prepare(None, utts, **kw)
    args = (bs.handle, vs.handle, C.byref(b.c))
    tail = (b.ids.ctypes.data_as(_lib.i64p), b.s_lens.ctypes.data_as(_lib.i64p), b.w2p.ctypes.data_as(_lib.i64p), 16)
    gp = np.array([64, 64, 0], np.int64)
    h, tot = C.c_void_p(), C.c_int64()
    rq = _lib.Sbv2StreamRequest(gp.ctypes.data_as(_lib.i64p), C.pointer(f48.c), None, 0, 1)
    assert l.sbv2_stream_begin_request(*args, None, *tail, C.byref(rq), C.byref(h), C.byref(tot)) != 0 and b"reserved" in l.sbv2_last_error()
    rq = _lib.Sbv2StreamRequest(None, C.pointer(f48.c), None, 0, 0)
    assert l.sbv2_stream_begin_request(*args, None, *tail, C.byref(rq), C.byref(h), C.byref(tot)) != 0 and b"gap_after" in l.sbv2_last_error()
    assert l.sbv2_stream_begin_request(*args, None, *tail, None, C.byref(h), C.byref(tot)) != 0
    assert l.sbv2_stream_begin_format(*args, *tail, C.byref(f48.c), C.byref(h), C.byref(tot)) != 0 and b"one utterance" in l.sbv2_last_error()
    assert not h.value
    # after the refusals a well-formed stream on the same handles works; the plain next is refused on it
    st = model.StreamHandle(bs, vs, utts, 16, fmt=f48, gaps=(64, 64, 0), **kw)
    n = C.c_int64()
    assert l.sbv2_stream_next(st.h, st.buf.ctypes.data, st.buf.size // 4, C.byref(n)) != 0 and b"sbv2_stream_next_format" in l.sbv2_last_error()
    parts = _take_all(st)
    assert sum(p.size for p in parts) == st.total_samples
    st.close()


@pytest.mark.gpu
def test_orchestrator_split_stream_equals_easy_synthesize():
    import json
    import scipy.io.wavfile as W
    from sbv2_api_amd import holder as H
    bc, vc, bs, vs = _tiny()
    pipe = model.Pipeline(bs, vs)
    keys = ("input_ids", "word2ph", "phones", "tones", "langs")
    sent = [{k: synth.make_utterance(n, bc, vc, seed=610 + n)[k] for k in keys} for n in (11, 6, 17)]
    lines = [sent[0], None, sent[1], sent[2]]
    styles = synth.hash_normal(77, 3 * vc["style_dim"]).reshape(3, -1).astype(np.float32)
    opts = orchestrator.SynthesizeOptions(sample_rate=48000, encoding="s16")
    wav, marks = orchestrator.easy_synthesize_marks(pipe, lines, styles, 1, 0, opts, noise_seed=1234)
    assert wav == orchestrator.easy_synthesize(pipe, lines, styles, 1, 0, opts, noise_seed=1234)
    _, y = W.read(io.BytesIO(wav))
    st = orchestrator.easy_synthesize_stream(bs, vs, lines, styles, 1, 0, opts, noise_seed=1234, chunk_frames=64, split=True)
    strip = lambda rows: [{k: v for k, v in r.items() if k in ("line", "index", "phone", "start", "end")} for r in rows]
    assert strip(st.marks["tokens"]) == strip(marks["tokens"]) and strip(st.marks["words"]) == strip(marks["words"])
    assert b"".join(st) == wav
    fl = orchestrator.easy_synthesize_stream(bs, vs, lines, styles, 1, 0, orchestrator.SynthesizeOptions(sample_rate=48000, encoding="flac"),
                                             noise_seed=1234, chunk_frames=64, split=True)
    got = R.read(b"".join(fl))
    np.testing.assert_array_equal(got["samples"], y)
    # the default format: the same samples as easy_synthesize's (its WAV header has another form)
    base = orchestrator.easy_synthesize(pipe, lines, styles, 1, 0, None, noise_seed=1234)
    _, x = W.read(io.BytesIO(base))
    _, xs = W.read(io.BytesIO(b"".join(orchestrator.easy_synthesize_stream(bs, vs, lines, styles, 1, 0, None, noise_seed=1234, chunk_frames=64,
                                                                          split=True))))
    assert x.tobytes() == xs.tobytes()
    pipe.close()
    # the holder: splits the text on '\n', closes the handle and resumes as it does today
    by_text = {"one": sent[0], "two": sent[1], "three": sent[2]}
    hd = H.TTSModelHolder(blob("bert", "tiny", 3), parse_text=lambda s: by_text[s])
    hd.load("m", json.dumps({"shape": list(styles.shape), "data": styles.tolist()}).encode(), blob("vits", "tiny", 5))
    hs = hd.easy_synthesize_stream("m", "one\n\ntwo\nthree", 1, 0, opts, noise_seed=1234, chunk_frames=64, split=True)
    m = hd._find("m")
    assert m.streams == 1
    assert b"".join(hs) == wav
    assert m.streams == 0 and hs._st is None
    hd.close()
    bs.close(); vs.close()


@pytest.fixture(scope="module")
def full_models():
    bs, vs = model.load_model(blob("bert", "full"), True), model.load_model(blob("vits", "full"), False)
    yield weights("bert", "full")[0], weights("vits", "full")[0], bs, vs
    bs.close(); vs.close()


@pytest.mark.gpu
def test_full_model_request_stream(full_models):
    """Two rows (60 and 30 phonemes), gap 22050, chunk 64 on the full-size models, against the joined fetch of a pipeline run: the bounds the
    single-utterance stream is held to at this size (test_pcm_format.py test_full_model_stream_16k_48k_s16): +-1 step at 16 kHz s16, 1e-5 at
    8 kHz f32 (the streamed native PCM agrees with the whole-sequence PCM to f32 rounding there).  Measured on an MI355X: 1 step and 2.8e-7."""
    bc, vc, bs, vs = full_models
    pipe = model.Pipeline(bs, vs)
    utts = [synth.make_utterance(60, bc, vc, seed=91), synth.make_utterance(30, bc, vc, seed=92)]
    gaps = (22050, 0)
    fmts = (model.PcmFormat(16000, "s16"), model.PcmFormat(8000, "f32"))
    b, lens, place, joined = _joined(pipe, utts, dict(forced=True), fmts[0], gaps)
    wholes = [pipe.fetch_format(b, f, place, joined)[0] for f in fmts]
    for f, whole in zip(fmts, wholes):
        st = model.StreamHandle(bs, vs, utts, 64, fmt=f, gaps=gaps, forced=True)
        got = np.concatenate(_take_all(st))
        assert st.total_samples == whole.size == got.size
        st.close()
        dev = np.abs(got.astype(np.float64) - whole.astype(np.float64)).max()
        print(f"full model request stream {f}: max deviation {dev:.3e}")
        if f.encoding == "s16":
            assert dev <= 1, f
        else:
            assert dev <= 1e-5, f
    pipe.close()
