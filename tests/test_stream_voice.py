"""Pitch, intonation and formant scale on request streams (sbv2_stream_voice, sbv2_stream_begin_request_voice, sbv2_debug_voice_stream;
StreamVoice and k_voice_marks_fed of csrc/voice.hip): the ABI, the host-side refusals, the look-ahead and the delivery rule on the CPU; on the
GPU the fed shifter against the one-shot shifter bit for bit at every cut set, and a voice stream against the fetch of the shifted request.
The yardstick of the kernels is the one-shot hook (sbv2_debug_voice_shift / _formant) with the row's own mean as the pivot; for any other pivot
it is the numpy restatement below (test_voice.voice_ref with the pivot in place of the mean)."""
import ctypes as C
import functools
import math
import os
import re

import numpy as np
import pytest

import flac_reader as R
from helpers import blob, make_utts, weights
from sbv2_api_amd import _lib, model, orchestrator, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu
NEW_SYMBOLS = ["sbv2_stream_begin_request_voice", "sbv2_stream_voice_lookahead", "sbv2_stream_voice_timeline", "sbv2_debug_voice_stream"]
SR, H = 16000, 80
SETTINGS = [(1.3, 0.8, 1.0), (0.5, 1.0, 1.0), (2.0, 0.0, 1.0), (1.0, 1.0, 0.5), (1.2, 1.5, 1.25)]


def lookahead_np(sr, q, f0_min=70.0, hop=0):
    """The header's closed form: A_v = G + 2 W + X + tau_max + H div 2."""
    hop = hop or sr // 200
    tau_max = math.ceil(sr / f0_min)
    W = max(tau_max + 1, sr // 200) + 2
    G = math.ceil(W / min(q, 1.0)) + 1
    X = math.ceil((max(q, 1.0) - 1.0) * W)
    return G + 2 * W + X + tau_max + hop // 2


def delivery(edges, n, A):
    """Final samples per push by the delivery rule: max(0, S - A) while the row has not ended, everything with its last sample."""
    out, at = [], 0
    for e in edges:
        fin = n if e >= n else max(0, e - A)
        out.append(fin - at)
        at = fin
    return out


# ---- CPU ------------------------------------------------------------------------------------------------------------------------------------

def test_new_symbols_are_exported_and_declared():
    header = open(os.path.join(ROOT, "include", "sbv2_hip.h")).read()
    l = _lib.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.SYMBOLS and getattr(l, name) is not None, name
    assert "} sbv2_stream_voice;" in header
    assert C.sizeof(_lib.Sbv2StreamVoice) == 48 + 8 + 8 + 16
    assert C.sizeof(_lib.Sbv2Voice) == 48                                        # the existing struct is as it was
    assert "stream entry point either" not in header                             # the note above sbv2_voice names the stream form now


def _sv(p=1.3, s=0.8, q=1.0, pivot=(150.0,), reserved=(0.0, 0.0), **kw):
    v = model.StreamVoice(p, s, q, pivot, **kw)
    c, keep = v.c_struct(0 if pivot is None else len(pivot))
    c.reserved[0], c.reserved[1] = reserved
    return c, keep


BAD = [(dict(pivot=None), "pivot_hz"), (dict(pivot=(float("nan"),)), "pivot_hz"), (dict(pivot=(float("inf"),)), "pivot_hz"),
       (dict(pivot=(69.9,)), "pivot_hz"), (dict(pivot=(600.1,)), "pivot_hz"), (dict(pivot=(150.0,), f0_min=200.0), "pivot_hz"),
       (dict(p=1.0, s=1.0, q=1.0), "without a voice"), (dict(reserved=(0.0, 1.0)), "reserved"), (dict(reserved=(float("nan"), 0.0)), "reserved"),
       (dict(p=2.5), "pitch_scale"), (dict(s=-0.1), "intonation_scale"), (dict(q=0.4), "formant_scale"), (dict(q=float("nan")), "formant_scale")]


@pytest.mark.parametrize("kw,word", BAD)
def test_refusals_that_need_no_run(kw, word):
    l = _lib.lib()
    c, keep = _sv(**kw)
    x, y, per = np.zeros(64, np.float32), np.zeros(64, np.float32), np.zeros(1, np.int64)
    i64p = C.POINTER(C.c_int64)
    # the hook checks everything before any device call: device 99 is never touched
    assert l.sbv2_debug_voice_stream(99, x.ctypes.data_as(_lib.f32p), 64, None, 0, SR, C.byref(c), None, None, y.ctypes.data_as(_lib.f32p),
                                     per.ctypes.data_as(i64p)) != 0
    assert word in l.sbv2_last_error().decode(), l.sbv2_last_error()
    if word != "pivot_hz":                                                       # (the look-ahead query does not look at the pivot)
        assert l.sbv2_stream_voice_lookahead(C.byref(c), SR) == -1
    # the begin call refuses the struct before it looks at the handles (all NULL here)
    batch = _lib.Sbv2Batch()
    batch.n = 1
    assert l.sbv2_stream_begin_request_voice(None, None, C.byref(batch), None, None, None, None, None, 16, None, None, None, C.byref(c), None, None,
                                             None, None, None) != 0
    assert word in l.sbv2_last_error().decode(), l.sbv2_last_error()


def test_track_and_token_pitch_stay_refused_with_a_stream_voice():
    v = model.StreamVoice(1.2, 1.0, 1.0, 150.0)
    with pytest.raises(model.Sbv2Error, match="not tracked"):
        model.StreamHandle(None, None, [{}], 16, gaps=[0], voice=v, track=model.PitchTrack())
    with pytest.raises(model.Sbv2Error, match="a stream takes no token_pitch"):
        model.StreamHandle(None, None, [{}], 16, gaps=[0], voice=v, token_pitch=model.TokenPitch([0.0]), forced=True)
    SO = orchestrator.SynthesizeOptions
    for o, word in ((SO(pitch_scale=1.2, voice_pivot_hz=150.0, pitch_track=True), "pitch_track"),
                    (SO(pitch_scale=1.2, voice_pivot_hz=150.0, token_pitch=[0.0, 200.0, 0.0]), "token_pitch")):
        with pytest.raises(model.Sbv2Error, match=word):
            orchestrator.easy_synthesize_stream(None, None, [dict(phones=[0, 1, 0], word2ph=[1, 1, 1])], np.zeros((1, 4), np.float32), options=o)


@pytest.mark.parametrize("sr", (8000, 16000, 44100))
@pytest.mark.parametrize("q", (0.5, 1.0, 2.0))
def test_lookahead_equals_the_closed_form(sr, q):
    v = model.StreamVoice(1.2, 1.0, q, 150.0)
    assert model.stream_voice_lookahead(v, sr) == lookahead_np(sr, q)
    hi = model.StreamVoice(1.2, 1.0, q, 250.0, f0_min=200.0)                    # a higher f0_min shortens it
    assert model.stream_voice_lookahead(hi, sr) == lookahead_np(sr, q, 200.0) < lookahead_np(sr, q)
    if sr == 44100 and q == 1.0:
        assert lookahead_np(sr, q) == 2640                                       # the figure the header quotes


@pytest.mark.parametrize("rate,enc", ((44100, "f32"), (16000, "s16"), (8000, "mulaw")))
def test_voice_timeline_sums_to_the_total_and_follows_the_rule(rate, enc):
    fmt = model.PcmFormat(rate, enc)
    hop, frames = 256, [37, 5, 64]
    mg = model.stream_min_gap(fmt)
    gaps = [mg + 100, mg, 777]
    v = model.StreamVoice(1.2, 1.0, 0.8, 150.0)
    A = model.stream_voice_lookahead(v)
    for chunk in (16, 50):
        place, joined, calls = model.stream_timeline(frames, gaps, hop, chunk, fmt)
        got = model.stream_voice_timeline(frames, gaps, hop, chunk, v, fmt)
        assert got.size == calls.size and (got >= 0).all() and int(got.sum()) == int(calls.sum()) == model.pcm_format_length(fmt, joined)
        # the rule, restated: a row's last call ends where it always ended; before that, the outputs whose newest tap lies below place + S - A
        L, M = (rate // math.gcd(rate, 44100)), (44100 // math.gcd(rate, 44100))
        half = 0 if rate == 44100 else 32 * max(L, M)
        want, prev, c, ends = [], 0, 0, np.cumsum(calls)
        for r, f in enumerate(frames):
            for f0 in range(0, f, chunk):
                S = min((f0 + chunk) * hop, f * hop)
                now = prev
                if S >= f * hop:
                    now = int(ends[c])
                elif S > A:
                    top = (int(place[r]) + S - A) * L - 1 - half
                    if top >= 0:
                        now = max(prev, min(top // M + 1, int(ends[c])))
                want.append(now - prev)
                prev, c = now, c + 1
        assert list(got) == want, (rate, chunk)
        assert (np.cumsum(got) <= ends).all()                                    # delivery only ever runs late


# ---- GPU: the fed shifter against the one-shot shifter ---------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def signal():
    """About 0.5 s at 16 kHz: silence, a voiced stretch of 130 Hz, noise, a voiced stretch of 300 Hz, a voiced end (180 Hz); f32, default_rng(7)."""
    rng = np.random.default_rng(7)
    ms = lambda t: int(round(t * SR / 1000.0))

    def tone(f, t_ms):
        t = np.arange(ms(t_ms)) / SR
        x = sum(np.sin(2 * np.pi * k * f * t + k) / k for k in range(1, 5))
        return x / np.abs(x).max() * 0.7
    x = np.concatenate([np.zeros(ms(40)), tone(130.0, 130), rng.standard_normal(ms(60)) * 0.05, tone(300.0, 120), rng.standard_normal(ms(40)) * 0.05,
                        tone(180.0, 110) + 0.0]).astype(np.float32)
    x.setflags(write=False)
    return x


def one_shot(x, p, s, q, period=None, voiced=None, **kw):
    v = model.Voice(p, s, H, **kw)
    if q == 1.0:
        return model.debug_voice_shift(x, SR, v, period, voiced)[0]
    return model.debug_voice_formant(x, SR, v, model.Formant(q), period, voiced)[0]


def mean_f0(period, voiced):
    """The header's integer sum: m = double(sum llrint(f0 65536)) / (65536.0 count)."""
    vv = np.asarray(voiced) != 0
    qq = np.rint((float(SR) / np.asarray(period)[vv]) * 65536.0).astype(np.int64)
    return float(int(qq.sum())) / (65536.0 * float(qq.size))


@functools.lru_cache(maxsize=None)
def yardstick(p, s, q):
    r = one_shot(signal(), p, s, q)
    return r, mean_f0(r.period, r.voiced)


def cut_sets(n, A, onset):
    rng = np.random.default_rng(11)
    irregular = np.sort(rng.integers(0, n + 1, 40))
    irregular = np.sort(np.concatenate([irregular, irregular[::5]]))             # repeated cuts: empty pushes
    tile = model.voice_tile()
    return {"none": [], "every sample across an onset": list(range(onset - 150, onset + 150)), "every H": list(range(H, n, H)),
            "every tile": list(range(tile, n, tile)), "every tile - 1": list(range(tile - 1, n, tile - 1)),
            "every tile + 1": list(range(tile + 1, n, tile + 1)), "irregular": [int(c) for c in irregular],
            "shorter and longer than A_v": [A - 1, 2 * A - 1 + 1, n - 1]}


@gpu
@pytest.mark.parametrize("p,s,q", SETTINGS)
def test_fed_shifter_equals_the_one_shot_at_every_cut_set(p, s, q):
    x = signal()
    n = x.size
    ref, m = yardstick(p, s, q)
    assert ref.voiced.any() and ref.y.tobytes() != x.tobytes()
    sv = model.StreamVoice(p, s, q, m, hop=H)
    A = model.stream_voice_lookahead(sv, SR)
    assert A == lookahead_np(SR, q, hop=H) and 2 * A + 1 < n
    onset = int(np.argmax(ref.voiced != 0)) * H
    peak = float(np.abs(x).max())
    for name, cuts in cut_sets(n, A, onset).items():
        y, per = model.debug_voice_stream(x, cuts, SR, sv)
        assert list(per) == delivery(list(cuts) + [n], n, A), name
        bad = np.nonzero(y.view(np.uint32) != ref.y.view(np.uint32))[0]
        assert bad.size == 0, (name, p, s, q, int(bad[0]), bad.size)
        assert float(np.abs(y).max()) <= peak


def voice_ref_pivot(x, sr, p, s, hop, period, voiced, pivot, f0_min=70.0, f0_max=600.0):
    """test_voice.voice_ref with m := pivot (the header's stream form), plain gather."""
    n = x.size
    nf = -(-n // hop)
    voiced = np.asarray(voiced)[:nf] != 0
    T = np.where(voiced, np.asarray(period, np.float64)[:nf], 1.0)
    f0 = float(sr) / T
    inc_u = int(np.rint(4294967296.0 / float(sr // 200)))
    g = np.minimum(np.maximum(p * (pivot + s * (f0 - pivot)), f0_min / 2.0), 2.0 * f0_max)
    inc_a = np.where(voiced, np.rint(4294967296.0 / T).astype(np.int64), inc_u)
    inc_s = np.where(voiced, np.rint(4294967296.0 / (float(sr) / g)).astype(np.int64), inc_u)
    frame = np.arange(n) // hop
    phi_a = np.cumsum(inc_a[frame])
    mark_a = (phi_a >> 32) != (np.concatenate([[0], phi_a[:-1]]) >> 32)
    vs = voiced[frame]
    phi_s = phi_a.copy()
    starts = np.nonzero(vs & ~np.concatenate([[False], vs[:-1]]))[0]
    ends = np.nonzero(vs & ~np.concatenate([vs[1:], [False]]))[0] + 1
    for k0, k1 in zip(starts, ends):
        phi_s[k0:k1] = (int(phi_a[k0 - 1]) if k0 > 0 else 0) + np.cumsum(inc_s[frame[k0:k1]])
    mark_s = np.where(vs, (phi_s >> 32) != (np.concatenate([[0], phi_s[:-1]]) >> 32), mark_a)
    ta, ts = np.nonzero(mark_a)[0], np.nonzero(mark_s)[0]
    hi = np.searchsorted(ta, ts)
    lo = np.maximum(hi - 1, 0)
    hi = np.minimum(hi, ta.size - 1)
    mp = np.where(ts - ta[lo] <= ta[hi] - ts, lo, hi)
    mp = np.where(ts <= ta[0], 0, np.where(ts >= ta[-1], ta.size - 1, mp))
    num, den, xd = np.zeros(n), np.zeros(n), x.astype(np.float64)
    for j in range(ts.size):
        mm = int(mp[j])
        a = int(ta[mm])
        L = a - int(ta[mm - 1]) if mm > 0 else a + 1
        Rr = int(ta[mm + 1]) - a if mm + 1 < ta.size else n - a
        u = np.arange(-L + 1, Rr)
        k = int(ts[j]) + u
        ok = (k >= 0) & (k < n)
        u, k = u[ok], k[ok]
        v = np.abs(u).astype(np.float64) / np.where(u < 0, float(L), float(Rr))
        w = 1.0 - (v * v) * (3.0 - 2.0 * v)
        if mm == 0:
            w[u < 0] = 1.0
        if mm == ta.size - 1:
            w[u > 0] = 1.0
        num[k] += w * xd[a + u]
        den[k] += w
    return (num / np.maximum(den, 1.0)).astype(np.float32)


@gpu
def test_a_pivot_that_is_not_the_mean_gives_the_restatement_at_that_pivot():
    x = signal()
    ref, m = yardstick(1.3, 0.8, 1.0)
    pivot = m * 1.25
    want = voice_ref_pivot(x, SR, 1.3, 0.8, H, ref.period, ref.voiced, pivot)
    assert want.tobytes() != ref.y.tobytes()                                     # the pivot matters
    assert voice_ref_pivot(x, SR, 1.3, 0.8, H, ref.period, ref.voiced, m).tobytes() == ref.y.tobytes()   # ... and the restatement is the one-shot's
    for cuts in ([], list(range(H, x.size, H))):
        y, _ = model.debug_voice_stream(x, cuts, SR, model.StreamVoice(1.3, 0.8, 1.0, pivot, hop=H))
        assert y.tobytes() == want.tobytes()


def _given_cases():
    tau_max, tile = math.ceil(SR / 70.0), 256
    long_n = 3 * lookahead_np(SR, 0.5, hop=H) + 17                             # several look-aheads long at every q used here: pushes deliver early
    nf = -(-long_n // H)
    top = np.full(nf, tau_max + 1.0)
    ones, zeros = np.ones(nf, np.int32), np.zeros(nf, np.int32)
    single = zeros.copy()
    single[nf // 2] = 1
    cases = [("every frame at tau_max + 1, q 0.5, p 0.5", long_n, 0.5, 1.0, 0.5, top, ones),
             ("every frame at tau_max + 1, q 0.5, p 2", long_n, 2.0, 1.0, 0.5, top, ones),
             ("a single voiced frame", long_n, 1.3, 0.8, 1.0, np.full(nf, 100.0), single),
             ("voiced from frame 0 to the last", long_n, 1.3, 0.5, 1.25, np.full(nf, 61.5), ones)]
    for n in (1, H - 1, tile - 1, tile, tile + 1):
        f = -(-n // H)
        cases.append((f"n = {n}", n, 1.3, 0.8, 1.0, np.full(f, 90.0), np.ones(f, np.int32)))
    cases.append(("no analysis mark (copied)", 60, 1.3, 0.8, 1.0, np.full(1, 200.0), np.ones(1, np.int32)))
    return cases


@gpu
@pytest.mark.parametrize("case", _given_cases(), ids=lambda c: c[0])
def test_given_contours_at_the_edges_equal_the_one_shot(case):
    name, n, p, s, q, period, voiced = case
    rng = np.random.default_rng(n)
    x = (rng.standard_normal(n) * 0.3).astype(np.float32)
    ref = one_shot(x, p, s, q, period, voiced)
    m = mean_f0(period, voiced)
    pivot = m
    if not 70.0 <= m <= 600.0:
        # Periods of tau_max + 1 put the row's mean below f0_min, where no pivot may lie.  The nearest allowed pivot is f0_min; the one-shot stays
        # the yardstick because both targets round to the same increments, which is checked here in the header's own f64 expressions.
        pivot = 70.0
        f0 = float(SR) / np.asarray(period, np.float64)[np.asarray(voiced) != 0]
        inc = [np.rint(4294967296.0 / (float(SR) / np.minimum(np.maximum(p * (c + s * (f0 - c)), 35.0), 1200.0))) for c in (m, pivot)]
        assert (inc[0] == inc[1]).all()
    sv = model.StreamVoice(p, s, q, pivot, hop=H)
    A = model.stream_voice_lookahead(sv, SR)
    for cuts in (list(range(1, n)), list(range(H, n, H))):
        y, per = model.debug_voice_stream(x, cuts, SR, sv, period, voiced)
        assert list(per) == delivery(list(cuts) + [n], n, A), name
        if n > 1000:                                                             # the long rows: most samples leave before the row has ended
            assert n >= 3 * A and int(per[:-1].sum()) >= n - A - H, (name, n, A)
            assert ref.y.tobytes() != x.tobytes()
        bad = np.nonzero(y.view(np.uint32) != ref.y.view(np.uint32))[0]
        assert bad.size == 0, (name, len(cuts), int(bad[0]) if bad.size else -1, bad.size)
        assert float(np.abs(y).max()) <= float(np.abs(x).max())
    if name.startswith("no analysis"):
        assert ref.ta.size == 0 and ref.y.tobytes() == x.tobytes()


# ---- GPU: through the stream, on the tiny models ----------------------------------------------------------------------------------------------

KW = dict(forced=True)
SCALES = (1.3, 0.8, 0.8)
VKW = dict(f0_min=200.0)                                                         # tau_max 221: A_v = 1060 native samples, below the rows' lengths


@pytest.fixture(scope="module")
def tiny():
    bc, _ = weights("bert", "tiny", 3)
    vc, _ = weights("vits", "tiny", 5)
    bs, vs = model.load_model(blob("bert", "tiny", 3), True), model.load_model(blob("vits", "tiny", 5), False)
    utts = make_utts([40, 23], bc, vc, seed0=171, with_bert=False)
    pipe = model.Pipeline(bs, vs)
    b = pipe.prepare(utts, **KW)
    pipe.run(b)
    native = [x.copy() for x in pipe.fetch(b)]
    # the rows' own means, from the one-shot contour of the native rows
    pivots = []
    for x in native:
        r = model.debug_voice_shift(x, 44100, model.Voice(SCALES[0], SCALES[1], **VKW))[0]
        vv = r.voiced != 0
        qq = np.rint((44100.0 / r.period[vv]) * 65536.0).astype(np.int64)
        assert vv.any(), "a tiny-model row without a voiced frame: no pivot would matter and the stream tests would show nothing"
        pivots.append(float(int(qq.sum())) / (65536.0 * float(qq.size)))
    yield dict(bs=bs, vs=vs, utts=utts, pipe=pipe, native=native, pivots=pivots, hop=_lib.lib().sbv2_vits_hop(vs.handle))
    pipe.close(); bs.close(); vs.close()


def _fetch(t, rows, fmt, gaps, **kw):
    pipe = t["pipe"]
    b = pipe.prepare([t["utts"][r] for r in rows], **KW)
    pipe.run(b)
    lens = [int(n) for n in b.lens]
    place = [0]
    for n, g in zip(lens[:-1], gaps[:-1]):
        place.append(place[-1] + n + g)
    joined = place[-1] + lens[-1] + gaps[-1]
    voice = model.Voice(SCALES[0], SCALES[1], **VKW)
    # (the pivot of a fetch is the row's own mean: the stream is handed the same bits)
    return pipe.fetch_request(b, range(len(rows)), fmt, place, joined, voice=voice, formant_scale=SCALES[2], **kw), lens, joined


def _take(st):
    parts = []
    while (c := st.next()) is not None:
        parts.append(c)
    return parts


def _svoice(t, rows):
    return model.StreamVoice(*SCALES, [t["pivots"][r] for r in rows], **VKW)


@gpu
@pytest.mark.parametrize("rate,enc", ((44100, "f32"), (16000, "s16"), (8000, "mulaw")))
def test_one_row_voice_stream_equals_the_shifted_fetch(tiny, rate, enc):
    t, fmt, rows, gaps = tiny, model.PcmFormat(rate, enc), [0], [0]
    want = _fetch(t, rows, fmt, gaps)[0][0].copy()
    sv = _svoice(t, rows)
    late = False
    for chunk in (16, 50):
        st = model.StreamHandle(t["bs"], t["vs"], [t["utts"][0]], chunk, fmt=fmt, gaps=gaps, voice=sv, **KW)
        parts = _take(st)
        st.close()
        frames = [len(t["native"][0]) // t["hop"]]
        calls = model.stream_voice_timeline(frames, gaps, t["hop"], chunk, sv, fmt)
        assert [p.size for p in parts] == list(calls), (rate, chunk)
        late |= any(0 < p.size for p in parts[:-1])
        got = np.concatenate(parts)
        assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), (rate, chunk, int(np.argmax(got != want)))
    assert late, "no call before the last delivered anything: the row is shorter than the look-ahead and the test shows nothing"


@gpu
def test_voice_stream_flac_and_level(tiny):
    t, fmt, rows, gaps = tiny, model.PcmFormat(16000, "s16"), [0], [0]
    sv = _svoice(t, rows)
    want = _fetch(t, rows, fmt, gaps)[0][0].copy()
    whole = _fetch(t, rows, fmt, gaps, flac=True)[0][0]
    st = model.StreamHandle(t["bs"], t["vs"], [t["utts"][0]], 16, fmt=fmt, flac=True, gaps=gaps, voice=sv, **KW)
    got = b"".join(_take(st))
    st.close()
    d = R.read(got)
    assert np.asarray(d["samples"], np.int16).tobytes() == want.tobytes()
    keep = lambda bts: bts[:12] + bts[18:]                                       # every byte outside 12..17 (STREAMINFO's frame sizes: 0 on a stream)
    assert keep(got) == keep(bytes(whole))
    # behind a level: the fixed-gain limiter of the shifted f64 signal
    f32 = model.PcmFormat(44100, "f32")
    y = _fetch(t, rows, f32, gaps)[0][0].astype(np.float64)
    lv = model.StreamLevel(6.0, -1.0)
    ref = model.debug_limiter_fixed([y], 44100, lv)[0][0].astype(np.float32)
    st = model.StreamHandle(t["bs"], t["vs"], [t["utts"][0]], 50, fmt=f32, level=lv, gaps=gaps, voice=sv, **KW)
    got = np.concatenate(_take(st))
    st.close()
    assert got.tobytes() == ref.tobytes()


@gpu
@pytest.mark.parametrize("rate,enc", ((16000, "s16"), (44100, "f32")))
def test_two_rows_with_a_gap_and_per_row_pivots(tiny, rate, enc):
    t, fmt, rows = tiny, model.PcmFormat(rate, enc), [0, 1]
    gaps = [model.stream_min_gap(fmt) + 333, 500]
    sv = _svoice(t, rows)
    (res, lens, joined) = _fetch(t, rows, fmt, gaps)
    want = res[0].copy()
    for chunk in (16, 64):
        st = model.StreamHandle(t["bs"], t["vs"], t["utts"], chunk, fmt=fmt, gaps=gaps, voice=sv, **KW)
        parts = _take(st)
        st.close()
        calls = model.stream_voice_timeline([n // t["hop"] for n in lens], gaps, t["hop"], chunk, sv, fmt)
        assert [p.size for p in parts] == list(calls)
        got = np.concatenate(parts)
        assert got.tobytes() == want.tobytes(), (rate, chunk, int(np.argmax(got != want)))


@gpu
def test_levels_and_pitch_of_a_voice_stream_are_those_of_the_shifted_fetch(tiny):
    t, fmt, rows, gaps = tiny, model.PcmFormat(16000, "s16"), [0], [0]
    pq = model.Pitch(80)
    res = _fetch(t, rows, fmt, gaps, marks=True, env_hop=160, pitch=pq)[0]
    m, pw = res[2], res[3]
    st = model.StreamHandle(t["bs"], t["vs"], [t["utts"][0]], 16, fmt=fmt, gaps=gaps, voice=_svoice(t, rows), levels=True, env_hop=160,
                            pitch=model.Pitch(80), **KW)
    ss, pk, es, f0 = [], [], [], []
    while st.next() is not None:
        mk, pt = st.next_marks(), st.next_pitch()
        ss.append(mk[1]); pk.append(mk[2]); es.append(mk[4]); f0.append(pt[1])
    mk, pt = st.next_marks(), st.next_pitch()
    ss.append(mk[1]); pk.append(mk[2]); es.append(mk[4]); f0.append(pt[1])
    st.close()
    assert np.concatenate(ss).tobytes() == np.asarray(m.sumsq, np.float64).tobytes()
    assert np.concatenate(pk).tobytes() == np.asarray(m.peak, np.float64).tobytes()
    assert np.concatenate(es).tobytes() == np.asarray(m.env_sumsq, np.float64).tobytes()
    assert np.concatenate(f0).tobytes() == np.asarray(pw.f0, np.float64).tobytes()


@gpu
def test_a_stream_without_a_voice_is_what_it_was_and_refusals(tiny):
    t, fmt = tiny, model.PcmFormat(24000, "s16")
    gaps = [model.stream_min_gap(fmt), 0]
    b = t["pipe"].prepare(t["utts"], **KW)
    t["pipe"].run(b)
    lens = [int(n) for n in b.lens]
    place, joined = [0, lens[0] + gaps[0]], lens[0] + gaps[0] + lens[1]
    want = t["pipe"].fetch_format(b, fmt, place, joined)[0].copy()
    st = model.StreamHandle(t["bs"], t["vs"], t["utts"], 50, fmt=fmt, gaps=gaps, **KW)
    parts = _take(st)
    st.close()
    _, _, calls = model.stream_timeline([n // t["hop"] for n in lens], gaps, t["hop"], 50, fmt)
    assert [p.size for p in parts] == list(calls) and np.concatenate(parts).tobytes() == want.tobytes()
    with pytest.raises(model.Sbv2Error, match="pivot_hz"):
        model.StreamHandle(t["bs"], t["vs"], t["utts"], 50, fmt=fmt, gaps=gaps, voice=model.StreamVoice(1.2, 1.0, 1.0, [150.0, 1000.0]), **KW)
    with pytest.raises(model.Sbv2Error, match="without a voice"):
        model.StreamHandle(t["bs"], t["vs"], t["utts"], 50, fmt=fmt, gaps=gaps, voice=model.StreamVoice(1.0, 1.0, 1.0, 150.0), **KW)
    # a voice stream is taken with sbv2_stream_next_level only, and in order only
    st = model.StreamHandle(t["bs"], t["vs"], t["utts"], 50, fmt=fmt, gaps=gaps, voice=_svoice(t, [0, 1]), **KW)
    n = C.c_int64()
    assert _lib.lib().sbv2_stream_next_format(st.h, st.buf.ctypes.data_as(C.c_void_p), st.buf.nbytes, C.byref(n)) != 0
    assert "sbv2_stream_next_level" in _lib.lib().sbv2_last_error().decode()
    assert sum(p.size for p in _take(st)) == want.size
    st.close()


@gpu
def test_a_stream_pivot_that_is_not_the_mean_changes_the_bytes(tiny):
    """The per-row pivots reach the device: the row's own mean gives the shifted fetch (the tests above), another pivot gives other samples,
    and only in the row whose pivot was changed."""
    t, fmt, rows = tiny, model.PcmFormat(44100, "f32"), [0, 1]
    gaps = [model.stream_min_gap(fmt) + 333, 500]
    (res, lens, joined) = _fetch(t, rows, fmt, gaps)
    want = res[0].copy()
    piv = [t["pivots"][0], min(t["pivots"][1] * 1.3, 600.0)]
    assert piv[1] != t["pivots"][1]
    st = model.StreamHandle(t["bs"], t["vs"], t["utts"], 50, fmt=fmt, gaps=gaps, voice=model.StreamVoice(*SCALES, piv, **VKW), **KW)
    got = np.concatenate(_take(st))
    st.close()
    cut = lens[0] + gaps[0] // 2
    assert got[:cut].tobytes() == want[:cut].tobytes() and got[cut:].tobytes() != want[cut:].tobytes()


# ---- up the stack: options, orchestrator, REST ------------------------------------------------------------------------------------------------

def test_options_check_the_pivot_at_construction_and_whole_signal_routes_refuse_it():
    SO = orchestrator.SynthesizeOptions
    assert SO().voice_pivot_hz is None and SO(voice_pivot_hz=150).voice_pivot_hz == 150.0 and SO(voice_pivot_hz=[100, 200.5]).voice_pivot_hz == [100.0, 200.5]
    for bad in (69.9, 600.1, float("nan"), float("inf"), "150", True, [], [150.0, None], [150.0, 700.0]):
        with pytest.raises(model.Sbv2Error, match="voice_pivot_hz"):
            SO(voice_pivot_hz=bad)
    sent = [dict(phones=[0, 1, 0], word2ph=[1, 1, 1])]
    styles = np.zeros((1, 4), np.float32)
    for f in (orchestrator.easy_synthesize, orchestrator.easy_synthesize_marks):
        with pytest.raises(model.Sbv2Error, match="/synthesize_stream"):
            f(None, sent, styles, options=SO(pitch_scale=1.2, voice_pivot_hz=150.0))
    # without the pivot the stream refuses as it always did; the message now names the way out
    with pytest.raises(model.Sbv2Error, match="/synthesize_marks.*voice_pivot_hz"):
        orchestrator.easy_synthesize_stream(None, None, sent, styles, options=SO(pitch_scale=1.2))
    with pytest.raises(model.Sbv2Error, match="formant_scale.*/synthesize_marks"):
        orchestrator.easy_synthesize_stream(None, None, sent, styles, options=SO(formant_scale=1.2))


def test_easy_synthesize_stream_hands_the_scales_and_pivots_to_the_handle(monkeypatch):
    SO = orchestrator.SynthesizeOptions
    seen = []

    class Stop(Exception):
        pass

    class FakeHandle:
        def __init__(self, bert, vits, utt, chunk_frames=256, fmt=None, flac=False, level=None, gaps=None, levels=False, env_hop=0, pitch=None,
                     voice=None, **kw):
            seen.append(dict(rows=len(utt) if isinstance(utt, list) else None, gaps=gaps, fmt=fmt, levels=levels, voice=voice))
            raise Stop()

    monkeypatch.setattr(model, "StreamHandle", FakeHandle)
    a, b2 = dict(phones=[0, 1, 0], word2ph=[1, 1, 1]), dict(phones=[0, 2, 0], word2ph=[1, 1, 1])
    styles = np.zeros((1, 4), np.float32)

    def run(options, sentences=(a,), **kw):
        with pytest.raises(Stop):
            orchestrator.easy_synthesize_stream(None, None, list(sentences), styles, options=options, **kw)
        return seen[-1]
    got = run(SO(pitch_scale=1.2, intonation_scale=0.5, formant_scale=0.8, voice_pivot_hz=151.5))
    v = got["voice"]
    assert (v.voice.pitch_scale, v.voice.intonation_scale, v.formant_scale, list(v.pivot_hz)) == (1.2, 0.5, 0.8, [151.5])
    assert got["fmt"] is not None                                                # a voice stream always formats
    got = run(SO(formant_scale=1.25, voice_pivot_hz=[100.0, 200.0]), (a, None, b2), split=True, levels=True)
    v = got["voice"]
    assert got["rows"] == 2 and got["levels"] and (v.voice.pitch_scale, v.formant_scale, list(v.pivot_hz)) == (1.0, 1.25, [100.0, 200.0])
    assert run(SO(voice_pivot_hz=150.0))["voice"] is None                        # no scale away from 1: the stream it always was
    assert run(SO())["voice"] is None
    n = len(seen)
    with pytest.raises(model.Sbv2Error, match="voice_pivot_hz holds 3 pivots"):
        orchestrator.easy_synthesize_stream(None, None, [a, b2], styles, options=SO(pitch_scale=1.2, voice_pivot_hz=[100.0, 150.0, 200.0]), split=True)
    assert len(seen) == n

    class OldHandle:                                                             # a handle from before the entry point: refused, not served unshifted
        def __init__(self, bert, vits, utt, chunk_frames=256, fmt=None, flac=False, level=None, gaps=None, levels=False, env_hop=0, pitch=None):
            raise AssertionError("never constructed")

    monkeypatch.setattr(model, "StreamHandle", OldHandle)
    with pytest.raises(model.Sbv2Error, match="not served unshifted"):
        orchestrator.easy_synthesize_stream(None, None, [a], styles, options=SO(pitch_scale=1.2, voice_pivot_hz=150.0))


def test_rest_stream_routes_take_the_pivot_and_the_others_refuse_it():
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient
    from sbv2_api_amd import rest
    wav = orchestrator.array_to_wav(np.zeros((1, 1, 10), np.float32))

    class Pieces(list):
        marks = {"sample_rate": 44100, "tokens": [], "words": []}
        total_samples = 10

        def close(self):
            pass

        def take_marks(self):
            return {}

    class H:
        calls = []

        def easy_synthesize(self, ident, text, style_id, speaker_id, options):
            orchestrator.RequestPlan([dict(phones=[0], word2ph=[1])], np.zeros((1, 4), np.float32), 0, 0, options)   # what every whole-signal route plans
            self.calls.append(("plain",))
            return wav

        def easy_synthesize_marks(self, ident, text, style_id, speaker_id, options):
            orchestrator.RequestPlan([dict(phones=[0], word2ph=[1])], np.zeros((1, 4), np.float32), 0, 0, options)
            self.calls.append(("marks",))
            return wav, Pieces.marks

        def easy_synthesize_stream(self, ident, text, style_id, speaker_id, options, **kw):
            self.calls.append(("stream", options.pitch_scale, options.intonation_scale, options.formant_scale, options.voice_pivot_hz, kw))
            return Pieces([wav])

    h = H()
    c = TestClient(rest.make_app(h), raise_server_exceptions=False)
    body = {"text": "x", "ident": "m", "pitch_scale": 1.25, "intonation_scale": 0.5, "formant_scale": 0.8, "voice_pivot_hz": 151.5}
    r = c.post("/synthesize_stream", json=body)
    assert r.status_code == 200 and r.content == wav and h.calls[-1][:5] == ("stream", 1.25, 0.5, 0.8, 151.5)
    r = c.post("/synthesize_stream", json=dict(body, voice_pivot_hz=[100.0, 200.0], split_sentences=True))
    assert r.status_code == 200 and h.calls[-1][4] == [100.0, 200.0] and h.calls[-1][5] == {"split": True}
    n = len(h.calls)
    for route in ("/synthesize_stream", "/synthesize_stream_marks"):
        old = c.post(route, json={k: v for k, v in body.items() if k != "voice_pivot_hz"})       # without a pivot: the 400 there always was
        assert old.status_code == 400 and "/synthesize_marks" in old.text
        bad = c.post(route, json=dict(body, voice_pivot_hz=1000.0))
        assert bad.status_code == 400 and "voice_pivot_hz" in bad.text
        for extra in ({"pitch_track": True}, {"token_pitch": [0.0]}):                            # these stay refused, pivot or not
            assert c.post(route, json=dict(body, **extra)).status_code == 400
    assert len(h.calls) == n                                                                     # ... all before the holder is asked
    for route in ("/synthesize", "/synthesize_marks"):
        r = c.post(route, json=body)
        assert r.status_code >= 400 and "voice_pivot_hz" in r.text and "/synthesize_stream" in r.text
    assert len(h.calls) == n
    assert c.post("/synthesize", json={k: v for k, v in body.items() if k != "voice_pivot_hz"}).content == wav


@gpu
def test_rest_round_trip_with_a_pivot_answers_the_bytes_of_synthesize():
    pytest.importorskip("fastapi")
    import io
    import json
    import scipy.io.wavfile as W
    from fastapi.testclient import TestClient
    from sbv2_api_amd import holder as HD, rest
    bc, _ = weights("bert", "tiny", 3)
    vc, _ = weights("vits", "tiny", 5)
    keys = ("input_ids", "word2ph", "phones", "tones", "langs")
    sent = {k: synth.make_utterance(40, bc, vc, seed=171)[k] for k in keys}
    styles = synth.hash_normal(77, 3 * vc["style_dim"]).reshape(3, -1).astype(np.float32)
    hd = HD.TTSModelHolder(blob("bert", "tiny", 3), parse_text=lambda s: sent)
    hd.load("m", json.dumps({"shape": list(styles.shape), "data": styles.tolist()}).encode(), blob("vits", "tiny", 5))

    class Seeded:                                                                # the routes draw a fresh noise seed: pin it, change nothing else
        def __getattr__(self, name):
            f = getattr(hd, name)
            return (lambda *a, **kw: f(*a, noise_seed=1234, **kw)) if name.startswith("easy_synthesize") else f

    c = TestClient(rest.make_app(Seeded()), raise_server_exceptions=False)
    scales = {"pitch_scale": 1.3, "intonation_scale": 0.8, "formant_scale": 0.8}
    base = {"text": "one", "ident": "m", "style_id": 1}
    _, native = W.read(io.BytesIO(c.post("/synthesize", json=base).content))
    # The pivot is the row's own mean in the routes' f0 range.  The tiny models speak noise, which that range may find unvoiced throughout;
    # any pivot then gives the samples of /synthesize (no frame has a target), and the formant scale still moves every grain.  That a pivot
    # reaches the device and matters is shown on rows with voiced frames in test_a_stream_pivot_that_is_not_the_mean_changes_the_bytes.
    r = model.debug_voice_shift(np.ascontiguousarray(native, np.float32), 44100, model.Voice(1.3, 0.8))[0]
    vv = r.voiced != 0
    m = 150.0
    if vv.any():
        qq = np.rint((44100.0 / r.period[vv]) * 65536.0).astype(np.int64)
        m = float(int(qq.sum())) / (65536.0 * float(qq.size))
    whole = c.post("/synthesize", json=dict(base, **scales))
    assert whole.status_code == 200
    _, want = W.read(io.BytesIO(whole.content))
    assert want.tobytes() != native.tobytes()
    for route_body in (dict(base, **scales, voice_pivot_hz=m), dict(base, **scales, voice_pivot_hz=[m], split_sentences=True)):
        got = c.post("/synthesize_stream", json=route_body)
        assert got.status_code == 200, got.text
        _, y = W.read(io.BytesIO(got.content))
        assert y.dtype == want.dtype and y.tobytes() == want.tobytes()
    assert c.post("/synthesize_stream", json=dict(base, **scales)).status_code == 400
    hd.close()
