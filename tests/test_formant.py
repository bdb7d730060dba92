"""Formant scale (sbv2_formant, sbv2_pipeline_fetch_request_formant, sbv2_debug_voice_formant; k_voice_gather_fmt of csrc/voice.hip): the ABI and
its host-side refusals, a numpy restatement judged as a formant shifter, the orchestrator / batcher / REST contracts against fakes (CPU); the
kernel against that restatement bit for bit, and the pipeline, batcher and REST on tiny models (GPU).

The reference is `formant_ref` below: the section above sbv2_formant in include/sbv2_hip.h restated in numpy on top of the marks of `voice_ref`
(tests/test_voice.py): float64 throughout, one Python loop over the synthesis marks in ascending order.

Tolerances.  Behind a contour everything is integer arithmetic and f64 arithmetic in a stated order, so ta, ts, map are EQUAL to the device's and
y is equal bit for bit; the GPU tests hand the device's own period_out / voiced_out to the reference, as tests/test_voice.py does.
As a formant shifter the reference is held to what the definition can promise on a harmonic signal: the harmonic comb samples the envelope
every f0, so the strongest harmonic about a moved formant q F lies within 1.5 harmonic spacings of q F, and f0 (autocorrelation) stays within
1 % of p 120 Hz.  The band searched about q F runs to the midpoint between neighbouring moved formants (beyond it a harmonic belongs to the
neighbour) and 2.5 spacings outwards where there is no neighbour, so the bound of 1.5 can be missed."""
import ctypes as C
import functools
import math
import os
import re
import threading
import types

import numpy as np
import pytest

import flac_reader as R
from helpers import blob, make_utts, weights
from sbv2_api_amd import _lib, batcher, model, orchestrator, synth
from test_token_pitch import TokenPipe, _tracked_contour, edits  # noqa: F401
from test_voice import (PAIRS, REQUEST, SIGNALS, STYLES, OldPipe, _join, _payload, five_rows, signal, signal_contour, voice_ref)  # noqa: F401

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["sbv2_pipeline_fetch_request_formant", "sbv2_debug_voice_formant"]
f64p, i32p, i64p = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
QS = [0.5, 0.8, 1.25, 2.0]


# ---- the reference ----------------------------------------------------------------------------------------------------------------------------------

def formant_ref(x, sr, p, s, hop, period, voiced, q, **kw):
    """The gather of include/sbv2_hip.h above sbv2_formant on the marks of voice_ref -> namespace(y, ta, ts, map, den)."""
    base = voice_ref(x, sr, p, s, hop, period, voiced, **kw)
    x = np.asarray(x)
    n = x.size
    ta, ts, mp = base.ta, base.ts, base.map
    if n == 0 or ta.size == 0:
        return types.SimpleNamespace(y=x.copy(), ta=ta, ts=ts, map=mp, den=np.ones(n))
    vo = np.asarray(voiced)[:-(-n // hop)] != 0
    xd = x.astype(np.float64)
    X = lambda i: np.where((i >= 0) & (i < n), xd[np.clip(i, 0, n - 1)], 0.0)
    num, den = np.zeros(n), np.zeros(n)
    for j in range(ts.size):
        mm = int(mp[j])
        a = int(ta[mm])
        L = a - int(ta[mm - 1]) if mm > 0 else a + 1
        Rr = int(ta[mm + 1]) - a if mm + 1 < ta.size else n - a
        reach = int(math.ceil(max(L, Rr) / min(q, 1.0))) + 1
        u = np.arange(-reach, reach + 1)
        k = int(ts[j]) + u
        ok = (k >= 0) & (k < n)
        u, k = u[ok], k[ok]
        du = u.astype(np.float64)
        pp = q * du
        pw = pp if vo[a // hop] else du
        ok = (pw > -float(L)) & (pw < float(Rr))
        k, pp, pw = k[ok], pp[ok], pw[ok]
        v = np.abs(pw) / np.where(pw < 0, float(L), float(Rr))
        w = 1.0 - (v * v) * (3.0 - 2.0 * v)
        if mm == 0:
            w[pw < 0] = 1.0
        if mm == ta.size - 1:
            w[pw > 0] = 1.0
        i0 = np.floor(pp)
        fr = pp - i0
        idx = a + i0.astype(np.int64)
        val = (1.0 - fr) * X(idx) + fr * X(idx + 1)
        num[k] += w * val
        den[k] += w
    return types.SimpleNamespace(y=(num / np.maximum(den, 1.0)).astype(np.float32), ta=ta, ts=ts, map=mp, den=den)


FORMANTS = ((700.0, 80.0), (1200.0, 100.0), (2600.0, 150.0))   # Hz, bandwidth
VOWEL_F0 = 120.0


@functools.lru_cache(maxsize=None)
def vowel(sr):
    """0.4 s of a 120 Hz pulse train through three resonators (each pulse adds the sampled responses exp(-pi B t) sin(2 pi F t), the pulses at
    their exact, fractional times), peak 0.7, f32; with its given contour: every frame voiced at sr / 120."""
    n = int(0.4 * sr)
    t = np.arange(n) / sr
    x = np.zeros(n)
    for k in range(int(0.4 * VOWEL_F0) + 1):
        d = t - k / VOWEL_F0
        on = d >= 0
        for F, B in FORMANTS:
            x[on] += np.exp(-np.pi * B * d[on]) * np.sin(2 * np.pi * F * d[on])
    x = (x / np.abs(x).max() * 0.7).astype(np.float32)
    x.setflags(write=False)
    return x


def harmonic_levels(y, sr, f0):
    """|spectrum| at the harmonics h f0 of the middle half of y (Hann window, the largest bin within f0 / 4 of each harmonic)."""
    n = y.size
    seg = y[n // 4:3 * n // 4].astype(np.float64)
    nfft = 1 << 17
    sp = np.abs(np.fft.rfft(seg * np.hanning(seg.size), nfft))
    hz = sr / nfft
    hs = np.arange(1, int(0.45 * sr / f0))
    lev = np.array([sp[int((h * f0 - f0 / 4) / hz):int((h * f0 + f0 / 4) / hz) + 1].max() for h in hs])
    return hs * f0, lev


def f0_by_autocorrelation(y, sr, near):
    n = y.size
    seg = y[n // 4:3 * n // 4].astype(np.float64)
    ac = np.correlate(seg, seg, "full")[seg.size - 1:]
    lo, hi = int(sr / near * 0.8), int(sr / near * 1.25)
    k = lo + int(np.argmax(ac[lo:hi + 1]))
    d = ac[k - 1] - 2 * ac[k] + ac[k + 1]
    return sr / (k + (0.5 * (ac[k - 1] - ac[k + 1]) / d if d < 0 else 0.0))


# ---- CPU: ABI and host-side refusals ----------------------------------------------------------------------------------------------------------------

def test_new_symbols_are_exported_and_declared():
    header = open(os.path.join(ROOT, "include", "sbv2_hip.h")).read()
    l = _lib.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.SYMBOLS and getattr(l, name) is not None, name
    assert "} sbv2_formant;" in header and C.sizeof(_lib.Sbv2Formant) == 16
    assert C.sizeof(_lib.Sbv2Voice) == 48 and C.sizeof(_lib.Sbv2TokenPitch) == 48   # the existing structs are as they were
    assert "formant_scale" in open(os.path.join(ROOT, "include", "sbv2_core.hpp")).read()


def test_formant_refusals_that_need_no_run():
    """The checks of sbv2_formant come before anything touches a handle or a device; nothing is written."""
    l = _lib.lib()
    f = model.PcmFormat()
    rows, place = np.array([0], np.int32), np.array([0], np.int64)
    req = _lib.Sbv2FetchRequest(rows.ctypes.data_as(i32p), 1, place.ctypes.data_as(i64p), 10, C.pointer(f.c), None, None, 0)
    x, lens = np.zeros(500, np.float32), np.array([500], np.int64)
    voice = _lib.Sbv2Voice(1.0, 1.0, 0.0, 0.0, 0.0, 0, 0)
    for fm, word in ((_lib.Sbv2Formant(0.49, 0.0), "formant_scale"), (_lib.Sbv2Formant(2.01, 0.0), "formant_scale"),
                     (_lib.Sbv2Formant(float("nan"), 0.0), "formant_scale"), (_lib.Sbv2Formant(1.2, 1.0), "reserved"),
                     (_lib.Sbv2Formant(1.0, float("nan")), "reserved")):
        for v in (None, C.byref(voice)):
            dst, got = np.full(16, 77, np.uint8), C.c_int64(-5)
            assert l.sbv2_pipeline_fetch_request_formant(None, 1, C.byref(req), v, None, None, None, C.byref(fm), dst.ctypes.data, dst.nbytes, C.byref(got),
                                                         None, None, None, None) != 0
            assert word in l.sbv2_last_error().decode(), l.sbv2_last_error()
            assert (dst == 77).all() and got.value == -5
        y = np.full(500, 77, np.float32)
        assert l.sbv2_debug_voice_formant(0, x.ctypes.data_as(_lib.f32p), lens.ctypes.data_as(i64p), 1, 44100, C.byref(voice), C.byref(fm), None, None, None,
                                          None, None, None, None, None, y.ctypes.data_as(_lib.f32p)) != 0
        assert word in l.sbv2_last_error().decode(), l.sbv2_last_error()
        assert (y == 77).all()
    dst, got = np.full(16, 77, np.uint8), C.c_int64(-5)
    for fm in (None, C.byref(_lib.Sbv2Formant(1.0, 0.0)), C.byref(_lib.Sbv2Formant(0.5, 0.0)), C.byref(_lib.Sbv2Formant(2.0, 0.0))):   # good ones reach the handle
        assert l.sbv2_pipeline_fetch_request_formant(None, 1, C.byref(req), None, None, None, None, fm, dst.ctypes.data, dst.nbytes, C.byref(got), None,
                                                     None, None, None) != 0
        assert b"bad arguments" in l.sbv2_last_error()
    y = np.full(500, 77, np.float32)
    assert l.sbv2_debug_voice_formant(0, x.ctypes.data_as(_lib.f32p), lens.ctypes.data_as(i64p), 1, 44100, C.byref(voice), None, None, None, None, None,
                                      None, None, None, None, y.ctypes.data_as(_lib.f32p)) != 0 and (y == 77).all()


def test_options_are_checked_at_construction():
    SO = orchestrator.SynthesizeOptions
    assert SO().formant_scale == 1.0 and orchestrator.formant_options(SO()) is None
    assert orchestrator.formant_options(SO(formant_scale=1.25)) == 1.25
    for bad in (0.49, 2.01, float("nan"), float("inf"), "1", True, None):
        with pytest.raises(model.Sbv2Error, match="formant_scale"):
            SO(formant_scale=bad)
    for ok in (0.5, 2, 1, 1.0):
        SO(formant_scale=ok)
    SO(pitch_track=True, formant_scale=0.9)                                     # the shifter runs: there is a contour to track
    with pytest.raises(model.Sbv2Error, match="pitch_track"):
        SO(pitch_track=True)


# ---- CPU: the routes against fakes --------------------------------------------------------------------------------------------------------------------

class FormantPipe(TokenPipe):
    """TokenPipe whose fetch_request knows formant_scale: the samples are multiplied by it (so the bytes tell which scale a request had)."""

    def fetch_request(self, b, rows, fmt, place, joined_len, formant_scale=1.0, **kw):
        res = super().fetch_request(b, rows, fmt, place, joined_len, **kw)
        self.calls[-1]["formant_scale"] = formant_scale
        return (res[0] * np.float32(formant_scale),) + tuple(res[1:])


def test_routes_carry_or_refuse_the_scale():
    SO = orchestrator.SynthesizeOptions
    pipe = FormantPipe()
    plain = orchestrator.easy_synthesize(pipe, REQUEST, STYLES, noise_seed=1)
    assert pipe.calls[-1] == dict(plain=True)
    assert orchestrator.easy_synthesize(pipe, REQUEST, STYLES, noise_seed=1, options=SO(formant_scale=1.0)) == plain
    assert pipe.calls[-1] == dict(plain=True)                                  # 1: the plain fetch there always was
    wav = orchestrator.easy_synthesize(pipe, REQUEST, STYLES, noise_seed=1, options=SO(formant_scale=1.5))
    assert pipe.calls[-1]["rows"] == [0, 1] and pipe.calls[-1]["formant_scale"] == 1.5 and pipe.calls[-1]["voice"] is None
    assert len(wav) == len(plain) and (_payload(wav) == np.float32(1.5) * _payload(plain)).all()
    wav2, mk = orchestrator.easy_synthesize_marks(pipe, REQUEST, STYLES, noise_seed=1, options=SO(formant_scale=0.5, pitch_scale=2.0, pitch_track=True))
    assert pipe.calls[-1]["formant_scale"] == 0.5 and pipe.calls[-1]["voice"] == (2.0, 1.0) and pipe.calls[-1]["track"] and pipe.calls[-1]["marks"]
    assert (_payload(wav2) == _payload(plain)).all() and mk["formant_scale"] == 0.5
    _, mk0 = orchestrator.easy_synthesize_marks(pipe, REQUEST, STYLES, noise_seed=1)
    assert "formant_scale" not in mk0 and {k: v for k, v in mk.items() if k != "formant_scale"} == mk0   # the spans do not move
    # a pipeline from before the option: refused with a clear message before any run, not served unshifted; at 1 it serves as ever
    for old in (OldPipe(), TokenPipe()):
        for call in (orchestrator.easy_synthesize, orchestrator.easy_synthesize_marks):
            with pytest.raises(model.Sbv2Error, match="formant_scale needs a pipeline"):
                call(old, REQUEST, STYLES, noise_seed=1, options=SO(formant_scale=1.2))
        assert old.runs == 0 and old.calls == []
        rb = batcher.RequestBatcher(old, start=False, clock=lambda: 0.0, max_wait_ms=1000.0)
        f = rb.submit(REQUEST, STYLES, options=SO(formant_scale=1.2), noise_seed=1)
        rb.start()
        rb.close()
        with pytest.raises(model.Sbv2Error, match="formant_scale needs a pipeline"):
            f.result(0)
        assert orchestrator.easy_synthesize(old, REQUEST, STYLES, noise_seed=1, options=SO(formant_scale=1.0)) == plain
    # streams refuse, before any GPU work, naming the whole-signal routes
    for kw in (dict(), dict(split=True), dict(levels=True)):
        with pytest.raises(model.Sbv2Error, match="formant_scale.*/synthesize_marks"):
            orchestrator.easy_synthesize_stream(None, None, REQUEST[:1], STYLES, options=SO(formant_scale=1.1), **kw)
    # the batcher: per request, with marks too
    rb = batcher.RequestBatcher(pipe, start=False, clock=lambda: 0.0, max_wait_ms=1000.0)
    f0 = rb.submit(REQUEST, STYLES, options=SO(formant_scale=2.0), noise_seed=1)
    f1 = rb.submit(REQUEST, STYLES, options=SO(formant_scale=0.5), noise_seed=1, marks=True)
    f2 = rb.submit(REQUEST, STYLES, noise_seed=1)
    n = len(pipe.calls)
    rb.start()
    rb.close()
    assert (_payload(f0.result(0)) == np.float32(2.0) * _payload(plain)).all()
    assert (_payload(f1.result(0)[0]) == np.float32(0.5) * _payload(plain)).all() and f1.result(0)[1] == dict(mk0, formant_scale=0.5)
    assert f2.result(0) == plain
    assert [c.get("formant_scale") for c in pipe.calls[n:] if "rows" in c] == [2.0, 0.5], pipe.calls[n:]


def test_a_pipeline_whose_fetch_request_cannot_be_inspected_is_refused():
    """Not known to take formant_scale: refused before any run, like one known not to; at 1 nothing is asked of it."""
    SO = orchestrator.SynthesizeOptions

    class Opaque:
        fetch_request = 5                                                       # inspect.signature raises TypeError

    class Missing:
        pass

    class Builtin:
        fetch_request = dict.update                                             # a builtin without a readable signature, or without the keyword

    for pipe in (Opaque(), Missing(), Builtin()):
        with pytest.raises(model.Sbv2Error, match="formant_scale needs a pipeline"):
            orchestrator.require_formant(pipe, SO(formant_scale=1.2))
        orchestrator.require_formant(pipe, SO())
        orchestrator.require_formant(pipe, SO(formant_scale=1.0, pitch_scale=1.2))


def test_rest_models_accept_the_scale_and_the_stream_routes_refuse_it():
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient
    from sbv2_api_amd import rest
    wav = orchestrator.array_to_wav(np.zeros((1, 1, 10), np.float32))
    marks = {"sample_rate": 44100, "tokens": [], "words": []}

    class H:
        calls = []

        def easy_synthesize(self, ident, text, style_id, speaker_id, options):
            self.calls.append(("plain", options.formant_scale, options.pitch_scale))
            return wav

        def easy_synthesize_batched(self, ident, text, style_id, speaker_id, options, batching=None, marks=False):
            from concurrent.futures import Future
            self.calls.append(("batched", options.formant_scale, options.pitch_scale))
            f = Future()
            f.set_result(wav)
            return f

        def easy_synthesize_marks(self, ident, text, style_id, speaker_id, options):
            self.calls.append(("marks", options.formant_scale, options.pitch_scale))
            return wav, marks

        def easy_synthesize_stream(self, ident, text, style_id, speaker_id, options, **kw):
            raise AssertionError("a stream with a formant scale must be refused before the holder is asked")

    h = H()
    c = TestClient(rest.make_app(h), raise_server_exceptions=False)
    body = {"text": "x", "ident": "m", "formant_scale": 0.8, "pitch_scale": 1.25}
    assert c.post("/synthesize", json=body).content == wav and h.calls[-1] == ("plain", 0.8, 1.25)
    assert c.post("/synthesize", json={"text": "x", "ident": "m"}).content == wav and h.calls[-1] == ("plain", 1.0, 1.0)
    assert c.post("/synthesize_marks", json=body).status_code == 200 and h.calls[-1] == ("marks", 0.8, 1.25)
    cb = TestClient(rest.make_app(h, batching={}), raise_server_exceptions=False)
    assert cb.post("/synthesize", json=body).content == wav and h.calls[-1] == ("batched", 0.8, 1.25)
    n = len(h.calls)
    r = c.post("/synthesize", json=dict(body, formant_scale=2.5))
    assert r.status_code >= 400 and "formant_scale" in r.text and len(h.calls) == n   # out of range: never reaches the holder
    for route in ("/synthesize_stream", "/synthesize_stream_marks"):
        for q in (1.25, 0.5, 9.0):
            r = c.post(route, json={"text": "x", "ident": "m", "formant_scale": q})
            assert r.status_code == 400 and "formant_scale" in r.text and "/synthesize_marks" in r.text, (route, r.status_code, r.text)


# ---- CPU: the reference judged as a formant shifter -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p,s", PAIRS)
@pytest.mark.parametrize("sr,hop", SIGNALS)
def test_the_reference_at_scale_1_is_the_shifter(sr, hop, p, s):
    x = signal(sr)
    r, T = signal_contour(sr, hop)
    a, b = formant_ref(x, sr, p, s, hop, T, r.voiced, 1.0), voice_ref(x, sr, p, s, hop, T, r.voiced)
    assert a.y.tobytes() == b.y.tobytes() and a.y.tobytes() != x.tobytes()


@pytest.mark.parametrize("sr,hop", SIGNALS)
def test_the_reference_moves_the_formants_and_keeps_the_pitch(sr, hop):
    """The strongest harmonic about every moved formant within 1.5 harmonic spacings of q F; f0 within 1 % of p 120 Hz.  Measured when written:
    see the printed table (worst distance 1.17 spacings in the issue's prototype)."""
    x = vowel(sr)
    nf = -(-x.size // hop)
    period, voiced = np.full(nf, sr / VOWEL_F0), np.ones(nf, np.int32)
    worst_d = worst_f = 0.0
    for p in (1.0, 1.25):
        for q in (0.8, 0.9, 1.15, 1.3):
            y = formant_ref(x, sr, p, 1.0, hop, period, voiced, q).y
            f0 = p * VOWEL_F0
            freq, lev = harmonic_levels(y, sr, f0)
            centres = [q * F for F, _ in FORMANTS]
            cells = []
            for i, cF in enumerate(centres):
                lo = 0.5 * (centres[i - 1] + cF) if i > 0 else cF - 2.5 * f0
                hi = 0.5 * (cF + centres[i + 1]) if i + 1 < len(centres) else cF + 2.5 * f0
                band = (freq >= lo) & (freq <= hi)
                assert band.sum() >= 2, (sr, p, q, cF)
                peak = freq[band][int(np.argmax(lev[band]))]
                cells.append(abs(peak - cF) / f0)
            got = f0_by_autocorrelation(y, sr, f0)
            worst_d, worst_f = max(worst_d, max(cells)), max(worst_f, abs(got - f0) / f0)
            rms = float(np.sqrt(np.mean(y.astype(np.float64) ** 2) / np.mean(x.astype(np.float64) ** 2)))
            print(f"[formant] {sr} Hz p = {p} q = {q}: peak distance from q F in harmonic spacings " + " ".join(f"{c:.2f}" for c in cells) +
                  f"; f0 {got:.2f} Hz ({100 * abs(got - f0) / f0:.3f} %); RMS ratio {rms:.2f}")
            assert max(cells) <= 1.5, (sr, p, q, cells)
            assert abs(got - f0) <= 0.01 * f0, (sr, p, q, got)
            assert np.abs(y).max() <= np.abs(x).max()
    print(f"[formant] {sr} Hz: worst distance {worst_d:.2f} spacings, worst f0 error {100 * worst_f:.3f} %")


@pytest.mark.parametrize("sr,hop", SIGNALS)
def test_the_reference_keeps_its_promises(sr, hop):
    rng = np.random.default_rng(7)
    x = signal(sr)
    r, T = signal_contour(sr, hop)
    noise = (rng.standard_normal(x.size) * 0.3).astype(np.float32)
    nf = -(-x.size // hop)
    rv = (rng.random(nf) < 0.6).astype(np.int32)                                # a random contour over noise: every rule is exercised, nothing is tuned
    rT = rng.uniform(sr / 400.0, sr / 90.0, nf)
    for q in (0.5, 0.77, 1.3, 2.0):
        for sig, per, vo, p, s in ((x, T, r.voiced, 1.3, 0.8), (x, T, r.voiced, 1.0, 1.0), (noise, rT, rv, 0.7, 1.0)):
            o, base = formant_ref(sig, sr, p, s, hop, per, vo, q), voice_ref(sig, sr, p, s, hop, per, vo)
            assert o.y.size == sig.size and o.y.dtype == np.float32
            assert np.abs(o.y).max() <= np.abs(sig).max(), (q, p, s)
            assert np.array_equal(o.ta, base.ta) and np.array_equal(o.ts, base.ts) and np.array_equal(o.map, base.map)
            assert o.y.tobytes() != base.y.tobytes()
        # an all-unvoiced row: the windows stay complementary in the output domain
        o = formant_ref(noise, sr, 1.3, 0.8, hop, rT, np.zeros(nf, np.int32), q)
        inside = np.arange(noise.size)
        inside = (inside >= o.ta[0]) & (inside <= o.ta[-1])
        assert inside.sum() > noise.size // 2 and np.abs(o.den[inside] - 1.0).max() <= 2.0 ** -52, q
        assert np.array_equal(o.ta, o.ts) and o.y.tobytes() != noise.tobytes() and np.abs(o.y).max() <= np.abs(noise).max()


# ---- GPU: the kernel against the reference --------------------------------------------------------------------------------------------------------------

def assert_equal_to_ref(got, x, sr, p, s, hop, q, what):
    """One row of debug_voice_formant against formant_ref fed the device's own contour: marks and map equal, y bit-equal."""
    ref = formant_ref(x, sr, p, s, hop, got.period, got.voiced, q)
    assert got.y.size == x.size, what
    np.testing.assert_array_equal(got.ta, ref.ta, err_msg=what + ": ta")
    np.testing.assert_array_equal(got.ts, ref.ts, err_msg=what + ": ts")
    np.testing.assert_array_equal(got.map, ref.map, err_msg=what + ": map")
    bad = np.nonzero(got.y.view(np.uint32) != ref.y.view(np.uint32))[0]
    assert bad.size == 0, (what, "y differs at", bad[:8], got.y[bad[:8]], ref.y[bad[:8]])
    return ref


@gpu
@pytest.mark.parametrize("p,s", [(1.0, 1.0), (1.3, 0.8), (0.5, 1.0)])
@pytest.mark.parametrize("q", QS)
@pytest.mark.parametrize("sr,hop", SIGNALS)
def test_hook_equals_the_reference(sr, hop, q, p, s):
    x = signal(sr)
    got, = model.debug_voice_formant(x, sr, model.Voice(p, s, hop=hop), model.Formant(q))
    ref = assert_equal_to_ref(got, x, sr, p, s, hop, q, f"{sr} Hz q = {q} p = {p} s = {s}")
    assert got.voiced.any() and ref.ts.size > 20
    assert got.y.tobytes() != x.tobytes() and np.abs(got.y).max() <= np.abs(x).max()
    plain, = model.debug_voice_shift(x, sr, model.Voice(p, s, hop=hop))
    assert np.array_equal(plain.ta, got.ta) and np.array_equal(plain.ts, got.ts) and np.array_equal(plain.map, got.map)   # the marks of the call without
    assert plain.period.tobytes() == got.period.tobytes() and plain.y.tobytes() != got.y.tobytes()


@gpu
@pytest.mark.parametrize("sr,hop", SIGNALS)
def test_hook_at_scale_1_is_the_shifter_and_a_second_call_gives_equal_bits(sr, hop):
    x = signal(sr)
    for p, s in ((1.3, 0.8), (1.0, 1.0), (2.0, 1.0)):
        v = model.Voice(p, s, hop=hop)
        one, = model.debug_voice_formant(x, sr, v, model.Formant(1.0))
        plain, = model.debug_voice_shift(x, sr, v)
        assert one.y.tobytes() == plain.y.tobytes(), (p, s)
    a, = model.debug_voice_formant(x, sr, model.Voice(1.3, 0.8, hop=hop), model.Formant(0.77))
    b, = model.debug_voice_formant(x, sr, model.Voice(1.3, 0.8, hop=hop), model.Formant(0.77))
    assert a.y.tobytes() == b.y.tobytes()


def _rows_16k():
    """The packed rows of one call at 16 kHz, hop 80, named: lengths about the gather's tile, and the contours that take each branch."""
    sr = 16000
    x = signal(sr)
    tile = model.voice_tile()
    assert tile == 256
    rng = np.random.default_rng(2)                                             # (the noise row of tests/test_voice.py: no frame of it is voiced)
    t = np.arange(3 * tile + 17) / sr
    tone = sum(np.sin(2 * np.pi * k * 150.0 * t + k) / k for k in range(1, 5))
    tone = (tone / np.abs(tone).max() * 0.7).astype(np.float32)
    a = 50 * sr // 1000 + 200                                                    # inside the tone of `signal`
    rows = [("one sample", x[a:a + 1]), ("tile - 1", x[a:a + tile - 1]), ("tile", x[a:a + tile]), ("tile + 1", x[a:a + tile + 1]),
            ("3 tiles + 17", x[a:a + 3 * tile + 17]), ("all zeros", np.zeros(700, np.float32)),
            ("all noise", (rng.standard_normal(2000) * 0.05).astype(np.float32)), ("empty", np.zeros(0, np.float32)),
            ("all tone", tone), ("the whole signal", x)]
    return sr, 80, rows


@gpu
@pytest.mark.parametrize("q", [0.5, 1.25])
def test_packed_rows_of_every_edge_shape_in_one_call(q):
    sr, hop, rows = _rows_16k()
    v, fm = model.Voice(1.3, 0.8, hop=hop), model.Formant(q)
    got = model.debug_voice_formant([r for _, r in rows], sr, v, fm)
    assert len(got) == len(rows)
    seen = {}
    for (name, x), g in zip(rows, got):
        seen[name] = (g, assert_equal_to_ref(g, x, sr, 1.3, 0.8, hop, q, name))
    assert seen["empty"][0].y.size == 0
    g, ref = seen["one sample"]
    assert g.y.size == 1 and abs(g.y[0]) <= abs(rows[0][1][0])
    g, ref = seen["all zeros"]
    assert not g.voiced.any() and not g.y.any()
    g, ref = seen["all noise"]
    assert not g.voiced.any() and np.array_equal(g.ta, g.ts) and g.y.tobytes() != rows[6][1].tobytes()   # unvoiced grains are read at q u too
    g, ref = seen["all tone"]
    assert g.voiced.any() and g.ts.size > g.ta.size
    for name in ("tile - 1", "tile", "tile + 1", "3 tiles + 17"):
        assert seen[name][0].y.tobytes() != dict(rows)[name].tobytes(), name
    # a row without an analysis mark is copied: a given contour whose only frame is voiced with a period longer than the row
    short = rows[1][1][:60]
    g, = model.debug_voice_formant(short, sr, v, fm, period=np.full(1, 200.0), voiced=np.ones(1, np.int32))
    assert g.ta.size == 0 and g.y.tobytes() == short.tobytes()
    # a row whose first and last frames are voiced (the estimator reads zeros beyond a row's ends, so the contour is given): no unvoiced edge
    tone = dict(rows)["all tone"]
    nf = -(-tone.size // hop)
    per, vo = np.full(nf, sr / 150.0), np.ones(nf, np.int32)
    g, = model.debug_voice_formant(tone, sr, v, fm, period=per, voiced=vo)
    ref = formant_ref(tone, sr, 1.3, 0.8, hop, per, vo, q)
    assert np.array_equal(g.ts, ref.ts) and np.array_equal(g.map, ref.map) and g.y.tobytes() == ref.y.tobytes() and g.voiced.all()
    # each row equals the same row alone, and in another order
    back = model.debug_voice_formant([r for _, r in rows[::-1]], sr, v, fm)[::-1]
    for (name, x), g, h in zip(rows, got, back):
        assert g.y.tobytes() == h.y.tobytes(), name
        alone, = model.debug_voice_formant(x, sr, v, fm)
        assert alone.y.tobytes() == g.y.tobytes(), name


@gpu
def test_a_given_contour_gives_the_reference_bits():
    """period_in: a constant 200-sample period over a pulse train with one unvoiced gap, voiced in its first and last frames."""
    sr, hop = 44100, 220
    n = 40 * hop + 57
    x = np.zeros(n, np.float32)
    x[::200] = 0.5
    x += (np.random.default_rng(3).standard_normal(n) * 0.01).astype(np.float32)
    nf = -(-n // hop)
    period, voiced = np.full(nf, 200.0), np.ones(nf, np.int32)
    voiced[15:22] = 0
    for q in (0.5, 0.77, 1.3, 2.0):
        for p, s in ((1.3, 0.8), (1.0, 1.0)):
            got, = model.debug_voice_formant(x, sr, model.Voice(p, s, hop=hop), model.Formant(q), period=period, voiced=voiced)
            ref = formant_ref(x, sr, p, s, hop, period, voiced, q)
            np.testing.assert_array_equal(got.ta, ref.ta)
            np.testing.assert_array_equal(got.ts, ref.ts)
            np.testing.assert_array_equal(got.map, ref.map)
            assert got.y.tobytes() == ref.y.tobytes(), (q, p, s)
            assert np.abs(got.y).max() <= np.abs(x).max()


DENSE_SR, DENSE_HOP, DENSE_F0_MAX = 16000, 80, 4000.0


@functools.lru_cache(maxsize=None)
def dense_row():
    """A row whose tiles stage more synthesis marks than the gather's block holds, which needs a raised f0_max (at the default 600 Hz no
    tile can reach more than 100): 27 frames at 16 kHz, hop 80, of a given contour: frames 0 - 15 voiced at a period of 4 samples (f0_max =
    sample_rate / 4 allows it), 16 - 20 voiced at 229 (grains 229 samples to a side), 21 - 22 unvoiced, 23 - 26 voiced at 4; noise and a tone.
    At pitch_scale 2 the synthesis marks of the short periods lie 2 samples apart."""
    n = 8 * 256 + 37
    rng = np.random.default_rng(11)
    x = (0.3 * rng.standard_normal(n) + 0.3 * np.sin(2 * np.pi * np.arange(n) / 8.0)).astype(np.float32)
    nf = -(-n // DENSE_HOP)
    period, voiced = np.full(nf, 4.0), np.ones(nf, np.int32)
    period[16:21] = 229.0
    voiced[21:23] = 0
    for a in (x, period, voiced):
        a.setflags(write=False)
    return x, period, voiced


def marks_staged(ts, n, sr, q, f0_min=70.0):
    """Per tile of the gather the synthesis marks it stages: those in [t0 - half, t1 + half), half = ceil(h / min(q, 1)) + 1 with
    h = max(tau_max + 1, sr / 200) + 2 (voice_spec and formant_spec of csrc/voice.hip)."""
    tile = 256
    h = max(int(math.ceil(sr / f0_min)) + 1, sr // 200) + 2
    half = int(math.ceil(h / min(q, 1.0))) + 1
    return [int(np.searchsorted(ts, min(t0 + tile, n) + half) - np.searchsorted(ts, t0 - half)) for t0 in range(0, n, tile)]


@pytest.mark.parametrize("s", [1.0, 0.0])
@pytest.mark.parametrize("q", [0.5, 1.25])
def test_the_dense_row_stages_more_marks_than_a_block(q, s):
    """What the GPU test below relies on, from the reference's ts alone; with intonation_scale 0 every voiced frame has the short synthesis
    period, so the 229-sample grains lie 2 - 3 samples apart and one output sample sums contributions of more than one chunk."""
    x, period, voiced = dense_row()
    ref = formant_ref(x, DENSE_SR, 2.0, s, DENSE_HOP, period, voiced, q, f0_max=DENSE_F0_MAX)
    staged = marks_staged(ref.ts, x.size, DENSE_SR, q)
    print(f"[formant] dense row q = {q} s = {s}: {ref.ts.size} synthesis marks, staged per tile {staged}")
    assert max(staged) > 256 and (q > 0.5 or s == 0.0 or max(staged) > 512)   # two passes of the chunk loop, three at q = 0.5 and marks 2 apart
    assert np.abs(ref.y).max() <= np.abs(x).max() and ref.y.tobytes() != x.tobytes()
    if s == 0.0:                                                                # a sample under the long grains: far more contributions than one chunk holds
        k = int(ref.ta[np.argmax(np.diff(ref.ta))])
        assert ref.den[k] > 1.0 and np.searchsorted(ref.ts, k + 229) - np.searchsorted(ref.ts, k - 229) > 100


@gpu
@pytest.mark.parametrize("s", [1.0, 0.0])
@pytest.mark.parametrize("q", [0.5, 1.25])
def test_hook_equals_the_reference_where_a_tile_stages_more_marks_than_a_block(q, s):
    """The chunk loop of k_voice_gather_fmt beyond its first pass: the marks restaged after the trailing barrier, the voiced bit of later
    chunks (voiced, unvoiced and voiced marks follow each other), the sum in ascending j across chunks."""
    x, period, voiced = dense_row()
    v = model.Voice(2.0, s, hop=DENSE_HOP, f0_max=DENSE_F0_MAX)
    got, = model.debug_voice_formant(x, DENSE_SR, v, model.Formant(q), period=period, voiced=voiced)
    staged = marks_staged(got.ts, x.size, DENSE_SR, q)
    assert max(staged) > 256 and (q > 0.5 or s == 0.0 or max(staged) > 512), staged
    ref = formant_ref(x, DENSE_SR, 2.0, s, DENSE_HOP, period, voiced, q, f0_max=DENSE_F0_MAX)
    np.testing.assert_array_equal(got.ta, ref.ta)
    np.testing.assert_array_equal(got.ts, ref.ts)
    np.testing.assert_array_equal(got.map, ref.map)
    bad = np.nonzero(got.y.view(np.uint32) != ref.y.view(np.uint32))[0]
    assert bad.size == 0, ("y differs at", bad[:8], got.y[bad[:8]], ref.y[bad[:8]])
    # the dense row packed between two others equals itself alone: the tiles of a row find their own marks
    other = signal(DENSE_SR)[1000:1700]
    nfo = -(-other.size // DENSE_HOP)
    po, vo = np.full(nfo, 100.0), (np.arange(nfo) % 3 != 0).astype(np.int32)
    three = model.debug_voice_formant([other, x, other[:300]], DENSE_SR, v, model.Formant(q), period=[po, period, po[:4]], voiced=[vo, voiced, vo[:4]])
    assert three[1].y.tobytes() == got.y.tobytes() and np.array_equal(three[1].ts, got.ts)
    assert three[0].y.tobytes() == formant_ref(other, DENSE_SR, 2.0, s, DENSE_HOP, po, vo, q, f0_max=DENSE_F0_MAX).y.tobytes()


@gpu
@pytest.mark.parametrize("q", [0.5, 1.25])
def test_packed_rows_with_given_contours_in_one_call(q):
    """The two edge shapes that need a given contour, inside a grid of several rows: a row without an analysis mark (copied) between rows that
    have marks, and a row voiced from its first frame to its last."""
    sr, hop, rows = _rows_16k()
    named = dict(rows)
    v, fm = model.Voice(1.3, 0.8, hop=hop), model.Formant(q)
    frames = lambda a: -(-a.size // hop)
    tone, short, zeros, t1 = named["all tone"], named["tile - 1"][:60], named["all zeros"], named["tile + 1"]
    gap = np.ones(frames(named["3 tiles + 17"]), np.int32)
    gap[3:5] = 0
    given = [("tile + 1, voiced", t1, np.full(frames(t1), sr / 150.0), np.ones(frames(t1), np.int32)),
             ("no analysis mark", short, np.full(1, 200.0), np.ones(1, np.int32)),                  # one voiced frame, its period longer than the row
             ("voiced to both ends", tone, np.full(frames(tone), sr / 150.0), np.ones(frames(tone), np.int32)),
             ("no analysis mark again", short[:7], np.full(1, 200.0), np.ones(1, np.int32)),
             ("all zeros, unvoiced", zeros, np.full(frames(zeros), 100.0), np.zeros(frames(zeros), np.int32)),
             ("3 tiles + 17, a gap", named["3 tiles + 17"], np.full(gap.size, sr / 150.0), gap)]
    got = model.debug_voice_formant([g[1] for g in given], sr, v, fm, period=[g[2] for g in given], voiced=[g[3] for g in given])
    for (name, x, per, vo), g in zip(given, got):
        ref = formant_ref(x, sr, 1.3, 0.8, hop, per, vo, q)
        assert np.array_equal(g.ta, ref.ta) and np.array_equal(g.ts, ref.ts) and np.array_equal(g.map, ref.map), name
        assert g.y.tobytes() == ref.y.tobytes(), name
        alone, = model.debug_voice_formant(x, sr, v, fm, period=per, voiced=vo)
        assert alone.y.tobytes() == g.y.tobytes(), name
    for i in (1, 3):
        assert got[i].ta.size == 0 and got[i].y.tobytes() == given[i][1].tobytes()
    assert got[2].voiced.all() and got[2].ts.size > got[2].ta.size and got[2].y.tobytes() != tone.tobytes()
    assert got[0].y.tobytes() != t1.tobytes() and got[5].y.tobytes() != named["3 tiles + 17"].tobytes()


# ---- GPU: the pipeline ----------------------------------------------------------------------------------------------------------------------------------

VOICE = (1.3, 0.8)


def _hooked(c, rows, q, voice=None, **kw):
    got = model.debug_voice_formant([c.native[r] for r in rows], 44100, voice or model.Voice(1.0, 1.0), model.Formant(q), **kw)
    return {r: g.y for r, g in zip(rows, got)}


@gpu
def test_pipeline_formant_is_the_hook_on_the_native_rows(five_rows, edits):
    c, e = five_rows, edits
    pipe, b, rows, place, joined = c.pipe, c.b, c.rows, c.place, c.joined
    f0 = model.PcmFormat()
    l = _lib.lib()
    # formant NULL and scale 1 are sbv2_pipeline_fetch_request_token_pitch byte for byte: through the C ABI, with a voice and a table
    rw, pl = np.asarray(rows, np.int32), np.asarray(place, np.int64)
    req = _lib.Sbv2FetchRequest(rw.ctypes.data_as(i32p), rw.size, pl.ctypes.data_as(i64p), joined, C.pointer(f0.c), None, None, 0)
    cv = model.Voice(*VOICE).c

    def raw(fn, *formant):
        ctp, keep = e.tp().c_struct()
        dst, got = np.zeros(joined, np.float32), C.c_int64(0)
        model.check(fn(pipe.h, b.ticket, C.byref(req), C.byref(cv), None, None, C.byref(ctp), *formant, dst.ctypes.data, dst.nbytes, C.byref(got), None, None,
                       None, None))
        assert got.value == joined
        return dst.tobytes(), keep[0].tobytes(), keep[1].tobytes()

    parent = raw(l.sbv2_pipeline_fetch_request_token_pitch)
    one = _lib.Sbv2Formant(1.0, 0.0)
    assert raw(l.sbv2_pipeline_fetch_request_formant, None) == parent and raw(l.sbv2_pipeline_fetch_request_formant, C.byref(one)) == parent
    plain = pipe.fetch_request(b, rows, f0, place, joined)[0].copy()
    assert pipe.fetch_request(b, rows, f0, place, joined, formant_scale=1.0)[0].tobytes() == plain.tobytes()
    # q = 1.2 without a voice: the hook at p = s = 1 on the native rows
    shifted = _hooked(c, rows, 1.2)
    changed = [r for r in rows if shifted[r].tobytes() != c.native[r].tobytes()]
    print(f"[formant] rows {rows} of {[len(c.native[r]) for r in rows]} samples: {changed} changed by q = 1.2")
    assert rows[0] in changed                                                   # (a row without an analysis mark is copied)
    got = pipe.fetch_request(b, rows, f0, place, joined, formant_scale=1.2)[0].copy()
    assert got.dtype == np.float32 and got.size == joined and got.tobytes() == _join(shifted, rows, place, joined).tobytes()
    assert pipe.fetch_request(b, rows, f0, place, joined, formant_scale=1.2)[0].tobytes() == got.tobytes()          # twice: identical
    # with a voice, and with the identity voice named
    vs = _hooked(c, rows, 1.2, voice=model.Voice(*VOICE))
    gv = pipe.fetch_request(b, rows, f0, place, joined, voice=model.Voice(*VOICE), formant_scale=1.2)[0].copy()
    assert gv.tobytes() == _join(vs, rows, place, joined).tobytes() and gv.tobytes() != got.tobytes()
    assert pipe.fetch_request(b, rows, f0, place, joined, voice=model.Voice(1.0, 1.0), formant_scale=1.2)[0].tobytes() == got.tobytes()
    # the marks' spans are those of the call without
    _, _, pm = pipe.fetch_request(b, rows, f0, place, joined, marks=True)
    out, _, m = pipe.fetch_request(b, rows, f0, place, joined, marks=True, formant_scale=1.2)
    assert out.tobytes() == got.tobytes() and m.start.tobytes() == pm.start.tobytes() and m.end.tobytes() == pm.end.tobytes()
    ss, pk = model.debug_segment_levels(out, m.start, m.end)
    assert ss.tobytes() == m.sumsq.tobytes() and pk.tobytes() == m.peak.tobytes()                # the levels of the delivered samples
    # refusals through the handle write nothing and leave the ticket fetchable
    for bad in (0.4, 2.5, float("nan")):
        with pytest.raises(model.Sbv2Error, match="formant_scale"):
            pipe.fetch_request(b, rows, f0, place, joined, formant_scale=bad)
    assert pipe.fetch_request(b, rows, f0, place, joined)[0].tobytes() == plain.tobytes()
    assert [x.tobytes() for x in pipe.fetch(b)] == [x.tobytes() for x in c.native]                # the run's PCM was only read


@gpu
def test_pipeline_formant_with_table_tracking_compressor_loudness_and_flac(five_rows, edits):
    c, e = five_rows, edits
    pipe, b, rows, place, joined = c.pipe, c.b, c.rows, c.place, c.joined
    sr, hop = 44100, 44100 // 200
    track = model.PitchTrack(cand_max=1.0, unvoiced_cost=0.9, switch_cost=0.2, jump_cost=0.25)
    # voice, tracking, the table and the scale at the identity format: the marks kernel's outputs are those of the call without formant
    f0 = model.PcmFormat()
    kw = dict(voice=model.Voice(*VOICE), track=track)
    base, _, tb = pipe.fetch_request(b, rows, f0, place, joined, token_pitch=e.tp(), **kw)
    base = base.copy()
    got, _, tp = pipe.fetch_request(b, rows, f0, place, joined, token_pitch=e.tp(), formant_scale=0.8, **kw)
    assert tp.applied.tobytes() == tb.applied.tobytes() and tp.src_f0.tobytes() == tb.src_f0.tobytes() and (tp.src_f0 > 0).any()
    assert got.size == base.size and got.tobytes() != base.tobytes()
    contour = [_tracked_contour(c.native[r], sr, hop, track) for r in rows]
    alone = pipe.fetch_request(b, rows, f0, place, joined, track=track, formant_scale=0.8)[0]    # tracking needs no voice when the formants move
    want = _hooked(c, rows, 0.8, period=[p for p, _ in contour], voiced=[v for _, v in contour])
    assert alone.tobytes() == _join(want, rows, place, joined).tobytes()
    # everything together into the FLAC sink: it decodes to the s16 fetch of the same chain
    f = model.PcmFormat(16000, "s16")
    all_ = dict(gain=model.Loudness(-23.0), dynamics=model.Dynamics(), token_pitch=None, formant_scale=0.8, **kw)
    s16, st, ds, t16 = pipe.fetch_request(b, rows, f, place, joined, **dict(all_, token_pitch=e.tp()))
    s16 = s16.copy()
    fl, st2, ds2, tfl = pipe.fetch_request(b, rows, f, place, joined, flac=True, **dict(all_, token_pitch=e.tp()))
    d = R.read(fl)
    assert d["rate"] == 16000 and np.asarray(d["samples"], np.int16).tobytes() == s16.tobytes()
    assert st.tobytes() == st2.tobytes() and ds.tobytes() == ds2.tobytes()
    assert tfl.applied.tobytes() == tb.applied.tobytes() and tfl.src_f0.tobytes() == tb.src_f0.tobytes() and t16.applied.tobytes() == tb.applied.tobytes()
    without = pipe.fetch_request(b, rows, f, place, joined, **dict(all_, token_pitch=e.tp(), formant_scale=1.0))
    assert without[0].tobytes() != s16.tobytes() and without[3].applied.tobytes() == tb.applied.tobytes()
    # marks and pitch of the delivered samples compose too
    out, _, m, pc, _, _ = pipe.fetch_request(b, rows, f, place, joined, marks=True, pitch=model.Pitch(160), **dict(all_, token_pitch=e.tp()))
    assert out.tobytes() == s16.tobytes() and pc.f0.size == -(-out.size // 160)
    assert [x.tobytes() for x in pipe.fetch(b)] == [x.tobytes() for x in c.native]


# the fetch-request ladder, narrowest first: each symbol takes what the one before takes and one stage more
RUNGS = ["", "_marks", "_pitch", "_voice", "_tracked", "_dynamics", "_token_pitch", "_formant"]


@gpu
@pytest.mark.parametrize("rung", RUNGS)
def test_every_rung_of_the_fetch_request_ladder_is_the_widest_call(five_rows, edits, rung):
    """include/sbv2_hip.h states each narrower sbv2_pipeline_fetch_request* symbol as exactly the next wider call with NULL.  Python reaches the
    widest only, so each symbol is called raw here with the richest arguments it can carry (marks with levels and an envelope, a Pitch,
    Voice(1.3, 0.8), a PitchTrack, a Dynamics in front of a loudness target, the token table, a scale), into s16 at 48 kHz so that the resampler
    and the quantiser run, and compared bit for bit with sbv2_pipeline_fetch_request_formant given the same arguments and NULL for the rest."""
    c, e, l = five_rows, edits, _lib.lib()
    k = RUNGS.index(rung)
    f = model.PcmFormat(48000, "s16")
    n_out = model.pcm_format_length(f, c.joined)
    rw, pl, gain = np.asarray(c.rows, np.int32), np.asarray(c.place, np.int64), model.Loudness(-23.0)
    req = _lib.Sbv2FetchRequest(rw.ctypes.data_as(i32p), rw.size, pl.ctypes.data_as(i64p), c.joined, C.pointer(f.c), C.pointer(gain.c), None, 0)
    ntok, env_hop = sum(e.counts), 480
    nenv = -(-n_out // env_hop)

    def fetch(widest):
        dst, got, stats, dyn = np.zeros(n_out, np.int16), C.c_int64(-1), np.full(3, np.nan), np.full(3, np.nan)
        mi = [np.full(ntok, -1, np.int64) for _ in range(2)]
        mf = [np.full(n, np.nan) for n in (ntok, ntok, nenv, nenv)]
        cm = _lib.Sbv2Marks(ntok, mi[0].ctypes.data_as(i64p), mi[1].ctypes.data_as(i64p), mf[0].ctypes.data_as(f64p), mf[1].ctypes.data_as(f64p), -1,
                            env_hop, 0, nenv, mf[2].ctypes.data_as(f64p), mf[3].ctypes.data_as(f64p), -1)
        cp, parr = model.Pitch(240).c_struct(n_out)
        ctp, tparr = e.tp().c_struct()
        stages = [model.Voice(*VOICE).c, model.PitchTrack().c, model.Dynamics().c, ctp, _lib.Sbv2Formant(1.2, 0.0)]
        n_stages = max(0, k - 2)                                                  # voice .. formant: what this rung can name
        stages = [C.byref(s) if i < n_stages else None for i, s in enumerate(stages)]
        tail = [C.byref(cm) if k >= 1 else None, C.byref(cp) if k >= 2 else None]
        out = [dst.ctypes.data, dst.nbytes, C.byref(got), stats.ctypes.data_as(f64p)]
        dyn_p = dyn.ctypes.data_as(f64p) if k >= 5 else None
        if widest:
            model.check(l.sbv2_pipeline_fetch_request_formant(c.pipe.h, c.b.ticket, C.byref(req), *stages, *out, dyn_p, *tail))
        else:
            fn = getattr(l, "sbv2_pipeline_fetch_request" + rung)
            model.check(fn(c.pipe.h, c.b.ticket, C.byref(req), *stages[:n_stages], *out, *([dyn_p] if k >= 5 else []), *tail[:min(k, 2)]))
        return dict(dst=dst.tobytes(), got=got.value, stats=stats.tobytes(), dyn=dyn.tobytes(), marks=[a.tobytes() for a in mi + mf],
                    marks_n=(cm.n_tokens, cm.n_env), pitch=[a.tobytes() for a in parr], pitch_n=cp.n_frames, tokens=[a.tobytes() for a in tparr])

    mine, widest = fetch(False), fetch(True)
    assert mine == widest, [name for name in mine if mine[name] != widest[name]]
    # ... and the arguments did reach the routine: whatever this rung names was filled, whatever it cannot name was left alone
    assert mine["got"] == n_out and not np.isnan(np.frombuffer(mine["stats"])).any()
    assert mine["marks_n"] == ((ntok, nenv) if k >= 1 else (-1, -1)) and np.isfinite(np.frombuffer(mine["marks"][2])).all() == (k >= 1)
    assert mine["pitch_n"] == (-(-n_out // 240) if k >= 2 else 0)
    assert (not np.isnan(np.frombuffer(mine["dyn"])).any()) == (k >= 5)
    assert (np.frombuffer(mine["tokens"][1]) > 0).any() == (k >= 6)                 # src_f0: measured where the table is given
    plain = c.pipe.fetch_request(c.b, c.rows, f, c.place, c.joined, gain=gain)[0].tobytes()
    assert (mine["dst"] == plain) == (k < 3)                                        # from the voice on, the signal is another


@gpu
def test_batcher_and_rest_carry_the_scale(monkeypatch):
    """Two concurrent requests with different scales each get the bytes of the request run alone, through the batcher and through REST (without
    the decoder's noise, as tests/test_voice.py explains)."""
    monkeypatch.setattr(orchestrator, "NOISE_SCALE", 0.0)
    monkeypatch.setattr(orchestrator, "NOISE_SCALE_W", 0.0)
    quiet = dict(noise_scale=0.0, noise_scale_w=0.0)
    bs, vs = model.load_model(blob("bert", "tiny", 3), True), model.load_model(blob("vits", "tiny", 5), False)
    bc, _ = weights("bert", "tiny", 3)
    vc, _ = weights("vits", "tiny", 5)
    keys = ("input_ids", "word2ph", "phones", "tones", "langs")
    sv = synth.hash_normal(77, 3 * vc["style_dim"]).reshape(3, -1).astype(np.float32) * 0.1
    SO = orchestrator.SynthesizeOptions
    o1, o2 = (lambda: SO(formant_scale=1.2)), (lambda: SO(sample_rate=16000, encoding="s16", formant_scale=0.8, pitch_scale=1.1))
    pipe = model.Pipeline(bs, vs)
    try:
        sents = [{k: u[k] for k in keys} for u in make_utts([14, 40], bc, vc, seed0=151, with_bert=False)]
        plain = orchestrator.easy_synthesize(pipe, sents, sv, 1, 0, SO(), noise_seed=4242, **quiet)
        alone1 = orchestrator.easy_synthesize(pipe, sents, sv, 1, 0, o1(), noise_seed=4242, **quiet)
        alone2, marks2 = orchestrator.easy_synthesize_marks(pipe, sents, sv, 1, 0, o2(), noise_seed=99, **quiet)
        scaled2 = orchestrator.easy_synthesize(pipe, sents, sv, 1, 0, SO(sample_rate=16000, encoding="s16", pitch_scale=1.1), noise_seed=99, **quiet)
        assert len(alone1) == len(plain) and alone1 != plain and len(alone2) == len(scaled2) and alone2 != scaled2   # unvoiced grains move too
        assert marks2["formant_scale"] == 0.8
        rb = batcher.RequestBatcher(pipe, start=False, max_wait_ms=1000.0)
        f1 = rb.submit(sents, sv, 1, 0, o1(), noise_seed=4242)
        f2 = rb.submit(sents, sv, 1, 0, o2(), noise_seed=99, marks=True)
        f3 = rb.submit(sents, sv, 1, 0, SO(), noise_seed=4242)
        rb.start()
        rb.close()
        assert f1.result(0) == alone1 and f2.result(0)[0] == alone2 and f2.result(0)[1] == marks2 and f3.result(0) == plain
        pytest.importorskip("fastapi")
        from fastapi.testclient import TestClient
        from sbv2_api_amd import rest

        class H:
            def easy_synthesize(self, ident, text, style_id, speaker_id, options):
                return orchestrator.easy_synthesize(pipe, sents, sv, style_id, speaker_id, options, noise_seed=4242, **quiet)

            def easy_synthesize_stream(self, ident, text, style_id, speaker_id, options, **kw):
                return orchestrator.easy_synthesize_stream(bs, vs, sents[:1], sv, style_id, speaker_id, options, noise_seed=4242, **kw)

            def easy_synthesize_batched(self, ident, text, style_id, speaker_id, options, batching=None, marks=False):
                return rbs[0].submit(sents, sv, style_id, speaker_id, options, noise_seed=4242, marks=marks)

        cl = TestClient(rest.make_app(H()), raise_server_exceptions=False)
        r = cl.post("/synthesize", json={"text": "x", "ident": "m", "style_id": 1, "formant_scale": 1.2})
        assert r.status_code == 200 and r.content == alone1
        assert cl.post("/synthesize", json={"text": "x", "ident": "m", "style_id": 1}).content == plain
        for route in ("/synthesize_stream", "/synthesize_stream_marks"):
            assert cl.post(route, json={"text": "x", "ident": "m", "style_id": 1, "formant_scale": 1.2}).status_code == 400, route
        # a batching app: two posts with different scales overlap and share ONE run (max_utts = their four rows closes it when the second joins)
        alone3 = orchestrator.easy_synthesize(pipe, sents, sv, 1, 0, SO(formant_scale=0.8), noise_seed=4242, **quiet)
        assert alone3 not in (alone1, plain)
        runs = []
        run = pipe.run
        monkeypatch.setattr(pipe, "run", lambda b, *a, **kw: (runs.append(len(b.lens)), run(b, *a, **kw))[1])
        rbs = [batcher.RequestBatcher(pipe, max_utts=4, max_wait_ms=60000.0)]
        cb = TestClient(rest.make_app(H(), batching={}), raise_server_exceptions=False)
        out = {}

        def post(q):
            out[q] = cb.post("/synthesize", json={"text": "x", "ident": "m", "style_id": 1, "formant_scale": q})

        threads = [threading.Thread(target=post, args=(q,)) for q in (1.2, 0.8)]
        try:
            for t in threads:
                t.start()
            for t in threads:
                t.join(120)
        finally:
            rbs[0].close()
        assert len(out) == 2 and all(r.status_code == 200 for r in out.values()), {q: (r.status_code, r.text[:200]) for q, r in out.items()}
        assert out[1.2].content == alone1 and out[0.8].content == alone3
        assert runs == [4], runs
    finally:
        pipe.close(); bs.close(); vs.close()
