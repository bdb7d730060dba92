"""Pitch and intonation scale (sbv2_voice, sbv2_pipeline_fetch_request_voice, sbv2_debug_voice_shift; csrc/voice.hip): the ABI and its host-side
refusals, a numpy restatement of the shifter judged as a shifter, the orchestrator / batcher / REST contracts against fakes (CPU); the kernels
against that restatement bit for bit, and the pipeline, batcher and REST on tiny models (GPU).

The reference is `voice_ref` below: the section above sbv2_voice in include/sbv2_hip.h restated in numpy, int64 phases, float64 windows, one
Python loop over the synthesis marks in ascending order; `yin_ref` is this file's own copy of the YIN restatement of tests/test_pitch.py.

Tolerances.  Given a contour (period, voiced per frame) everything behind it is integer arithmetic and f64 arithmetic in a stated order: ta, ts,
map are EQUAL to the device's and y is equal bit for bit.  The GPU tests therefore hand the device's own period_out / voiced_out to the
reference.  The contour itself is YIN on f32 samples, where only the order of the sums is the library's: the rule of tests/test_pitch.py (c
within 1e-9; a frame whose decision the reference takes by less than 1e-9 is exempt, at most 2 % of them), on signals where the reference
exempts none (asserted on the CPU).
As a shifter the reference is held to: median relative f0 error <= 1 %, 90th percentile <= 3 %, >= 85 % of the input's voiced frames voiced in
both contours (measured when written, 44.1 kHz / 16 kHz, worst pair: see test_the_reference_shifts_the_pitch)."""
import ctypes as C
import functools
import math
import os
import re
import types

import numpy as np
import pytest

import flac_reader as R
from helpers import blob, make_utts, weights
from sbv2_api_amd import _lib, batcher, model, orchestrator, synth

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["sbv2_pipeline_fetch_request_voice", "sbv2_debug_voice_shift", "sbv2_voice_tile"]
F0_MIN, F0_MAX, THRESHOLD = 70.0, 600.0, 0.15
MARGIN = 1e-9
PAIRS = [(1.5, 1.0), (0.75, 1.0), (2.0, 1.0), (0.5, 1.0), (1.0, 1.5), (1.2, 0.5)]
SIGNALS = [(44100, 220), (16000, 80)]
f64p, i32p, i64p = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)


# ---- the reference ----------------------------------------------------------------------------------------------------------------------------------

def lags_np(sr, f0_min=F0_MIN, f0_max=F0_MAX):
    return math.floor(sr / f0_max), math.ceil(sr / f0_min)


def yin_ref(v, sr, hop, f0_min=F0_MIN, f0_max=F0_MAX, threshold=THRESHOLD):
    """YIN steps 2 - 5 as include/sbv2_hip.h states them above sbv2_pitch, on float64 samples.  Per-frame arrays: lag, voiced, c3 (c(lag - 1),
    c(lag), c(lag + 1)), f0, marginal (the decision hangs on a difference below MARGIN)."""
    v = np.asarray(v)
    assert v.dtype == np.float64
    n = v.size
    tau_min, tau_max = lags_np(sr, f0_min, f0_max)
    W = tau_max
    nf = -(-n // hop) if n else 0
    tau = np.arange(1, W + 1)
    out = types.SimpleNamespace(lag=np.zeros(nf, np.int32), voiced=np.zeros(nf, np.int32), c3=np.zeros((nf, 3)), f0=np.zeros(nf),
                                marginal=np.zeros(nf, bool), tau_min=tau_min, tau_max=tau_max)
    for f in range(nf):
        b = f * hop + hop // 2 - tau_max
        idx = b + np.arange(2 * W)
        ok = (idx >= 0) & (idx < n)
        w = np.where(ok, v[np.clip(idx, 0, max(n - 1, 0))], 0.0)
        rows = np.lib.stride_tricks.sliding_window_view(w, W)[1:W + 1]          # row tau - 1 = w[tau : tau + W]
        e = w[None, :W] - rows
        d = (e * e).sum(axis=1)
        S = np.cumsum(d)
        with np.errstate(invalid="ignore", divide="ignore"):
            c = np.where(S == 0, 1.0, d * tau.astype(np.float64) / S)
        c = np.concatenate([[np.nan], c])                                        # c[tau]
        under = np.nonzero(c[tau_min:tau_max + 1] < threshold)[0]
        marginal = False
        if under.size:
            first = lag = tau_min + int(under[0])
            marginal |= bool((np.abs(c[tau_min:first + 1] - threshold) < MARGIN).any())
            while lag + 1 <= tau_max:
                marginal |= bool(abs(c[lag + 1] - c[lag]) < MARGIN)
                if not c[lag + 1] < c[lag]:
                    break
                lag += 1
            voiced = 1
        else:
            marginal |= bool((np.abs(c[tau_min:tau_max + 1] - threshold) < MARGIN).any())
            lag = tau_min + int(np.argmin(c[tau_min:tau_max + 1]))
            ruled = np.concatenate([[False], S == 0])
            near = c[tau_min:tau_max + 1] - c[lag] < MARGIN
            near &= ~(ruled[tau_min:tau_max + 1] & ruled[lag])
            near[lag - tau_min] = False
            marginal |= bool(near.any())
            voiced = 0
        c0 = c[lag]
        cm = c[lag - 1] if lag - 1 >= 1 else c0
        cp = c[lag + 1] if lag + 1 <= tau_max else c0
        den = cm - 2.0 * c0 + cp
        delta = 0.5 * (cm - cp) / den if den > 0 and lag - 1 >= 1 and lag + 1 <= tau_max else 0.0
        out.lag[f], out.voiced[f], out.c3[f], out.marginal[f] = lag, voiced, (cm, c0, cp), marginal
        out.f0[f] = sr / (lag + delta) if voiced else 0.0
    return out


def periods_of(r):
    """T_f = lag + delta of a contour of yin_ref (delta limited to [-1, 1], as the header states)."""
    cm, c0, cp = r.c3[:, 0], r.c3[:, 1], r.c3[:, 2]
    den = cm - 2.0 * c0 + cp
    both = (r.lag - 1 >= 1) & (r.lag + 1 <= r.tau_max)
    with np.errstate(invalid="ignore", divide="ignore"):
        delta = np.where((den > 0.0) & both, 0.5 * (cm - cp) / den, 0.0)
    return r.lag.astype(np.float64) + np.minimum(np.maximum(delta, -1.0), 1.0)


def voice_ref(x, sr, p, s, hop, period, voiced, f0_min=F0_MIN, f0_max=F0_MAX):
    """The shifter of include/sbv2_hip.h behind a given contour (period [nf] f64 = T_f, voiced [nf]) -> namespace(y, ta, ts, map)."""
    x = np.asarray(x)
    assert x.dtype == np.float32
    n = x.size
    nf = -(-n // hop) if n else 0
    period, voiced = np.asarray(period, np.float64)[:nf], np.asarray(voiced)[:nf] != 0
    assert period.size == nf and voiced.size == nf
    none = types.SimpleNamespace(y=x.copy(), ta=np.zeros(0, np.int64), ts=np.zeros(0, np.int64), map=np.zeros(0, np.int64))
    if n == 0:
        return none
    T = np.where(voiced, period, 1.0)
    f0 = float(sr) / T
    inc_u = int(np.rint(4294967296.0 / float(sr // 200)))
    if voiced.any():
        q = np.rint(f0[voiced] * 65536.0).astype(np.int64)
        m = float(int(q.sum())) / (65536.0 * float(q.size))
    else:
        m = 0.0
    g = p * (m + s * (f0 - m))
    g = np.minimum(np.maximum(g, f0_min / 2.0), 2.0 * f0_max)
    Tp = float(sr) / g
    inc_a = np.where(voiced, np.rint(4294967296.0 / T).astype(np.int64), inc_u)
    inc_s = np.where(voiced, np.rint(4294967296.0 / Tp).astype(np.int64), inc_u)
    frame = np.arange(n) // hop
    phi_a = np.cumsum(inc_a[frame])
    mark_a = (phi_a >> 32) != (np.concatenate([[0], phi_a[:-1]]) >> 32)
    vs = voiced[frame]
    phi_s = phi_a.copy()
    starts = np.nonzero(vs & ~np.concatenate([[False], vs[:-1]]))[0]
    ends = np.nonzero(vs & ~np.concatenate([vs[1:], [False]]))[0] + 1
    for k0, k1 in zip(starts, ends):                                             # a voiced run: phi_s(k0 - 1) = phi_a(k0 - 1)
        base = int(phi_a[k0 - 1]) if k0 > 0 else 0
        phi_s[k0:k1] = base + np.cumsum(inc_s[frame[k0:k1]])
    mark_s = np.where(vs, (phi_s >> 32) != (np.concatenate([[0], phi_s[:-1]]) >> 32), mark_a)
    ta, ts = np.nonzero(mark_a)[0], np.nonzero(mark_s)[0]
    if ta.size == 0:
        return none
    hi = np.searchsorted(ta, ts)                                                 # the first analysis mark at or after ts
    lo = np.maximum(hi - 1, 0)
    hi = np.minimum(hi, ta.size - 1)
    mp = np.where(ts - ta[lo] <= ta[hi] - ts, lo, hi)                            # the nearest, a tie to the earlier
    mp = np.where(ts <= ta[0], 0, np.where(ts >= ta[-1], ta.size - 1, mp))
    num, den = np.zeros(n), np.zeros(n)
    xd = x.astype(np.float64)
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
    y = (num / np.maximum(den, 1.0)).astype(np.float32)
    return types.SimpleNamespace(y=y, ta=ta, ts=ts, map=mp)


# ---- the signals --------------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def signal(sr):
    """50 ms noise (sigma 0.05), 200 ms of a 150 Hz tone (harmonics 1 .. 4, amplitude 1 / k, phase k, peak 0.7), 50 ms noise, a 200 ms glide from
    120 to 240 Hz with the same harmonics, 30 ms of zeros; f32, default_rng(1)."""
    rng = np.random.default_rng(1)
    ms = lambda t: int(round(t * sr / 1000.0))
    n1 = rng.standard_normal(ms(50)) * 0.05
    t = np.arange(ms(200)) / sr
    tone = sum(np.sin(2 * np.pi * k * 150.0 * t + k) / k for k in range(1, 5))
    tone = tone / np.abs(tone).max() * 0.7
    n2 = rng.standard_normal(ms(50)) * 0.05
    ph = 2 * np.pi * np.cumsum(np.linspace(120.0, 240.0, ms(200))) / sr
    gl = sum(np.sin(k * ph + k) / k for k in range(1, 5))
    gl = gl / np.abs(gl).max() * 0.7
    x = np.concatenate([n1, tone, n2, gl, np.zeros(ms(30))]).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def signal_contour(sr, hop):
    r = yin_ref(signal(sr).astype(np.float64), sr, hop)
    return r, periods_of(r)


@functools.lru_cache(maxsize=None)
def shifted_ref(sr, hop, p, s):
    r, T = signal_contour(sr, hop)
    return voice_ref(signal(sr), sr, p, s, hop, T, r.voiced)


# ---- CPU: ABI and host-side refusals ----------------------------------------------------------------------------------------------------------------

def test_new_symbols_are_exported_and_declared():
    header = open(os.path.join(ROOT, "include", "sbv2_hip.h")).read()
    l = _lib.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.SYMBOLS and getattr(l, name) is not None, name
    assert "} sbv2_voice;" in header
    assert C.sizeof(_lib.Sbv2Voice) == 48
    assert C.sizeof(_lib.Sbv2Pitch) == 72 and C.sizeof(_lib.Sbv2Marks) == 88   # the existing structs are as they were
    assert model.voice_tile() >= 64 and model.voice_tile() % 64 == 0


def _c_voice(p=1.3, s=0.8, f0_min=0.0, f0_max=0.0, threshold=0.0, hop=0, reserved=0):
    return _lib.Sbv2Voice(p, s, f0_min, f0_max, threshold, hop, reserved)


BAD_VOICES = [(dict(p=0.49), "pitch_scale"), (dict(p=2.01), "pitch_scale"), (dict(p=float("nan")), "pitch_scale"), (dict(s=-0.1), "intonation_scale"),
              (dict(s=2.1), "intonation_scale"), (dict(s=float("nan")), "intonation_scale"), (dict(hop=43), "hop"), (dict(hop=883), "hop"),
              (dict(hop=-1), "hop"), (dict(reserved=1), "reserved"), (dict(f0_min=39.0), "f0_min"), (dict(f0_max=44100 / 4 + 1), "f0_max"),
              (dict(f0_min=700.0), "below f0_max"), (dict(threshold=1.0), "threshold"), (dict(threshold=-0.2), "threshold")]


def test_voice_refusals_that_need_no_run():
    """The checks of sbv2_voice come before anything touches a handle or a device: a null handle reaches them (and is refused itself when they
    pass), and the hook refuses before its first device call; nothing is written."""
    l = _lib.lib()
    f = model.PcmFormat()
    rows, place = np.array([0], np.int32), np.array([0], np.int64)
    req = _lib.Sbv2FetchRequest(rows.ctypes.data_as(i32p), 1, place.ctypes.data_as(i64p), 10, C.pointer(f.c), None, None, 0)
    x, lens = np.zeros(500, np.float32), np.array([500], np.int64)
    for kw, word in BAD_VOICES:
        v = _c_voice(**kw)
        dst, got = np.full(16, 77, np.uint8), C.c_int64(-5)
        assert l.sbv2_pipeline_fetch_request_voice(None, 1, C.byref(req), C.byref(v), dst.ctypes.data, dst.nbytes, C.byref(got), None, None, None) != 0
        assert word in l.sbv2_last_error().decode(), (kw, l.sbv2_last_error())
        assert (dst == 77).all() and got.value == -5
        y = np.full(500, 77, np.float32)
        assert l.sbv2_debug_voice_shift(0, x.ctypes.data_as(_lib.f32p), lens.ctypes.data_as(i64p), 1, 44100, C.byref(v), None, None, None, None, None,
                                        None, None, None, y.ctypes.data_as(_lib.f32p)) != 0
        assert word in l.sbv2_last_error().decode(), (kw, l.sbv2_last_error())
        assert (y == 77).all()
    ok, dst, got = _c_voice(), np.full(16, 77, np.uint8), C.c_int64(-5)
    for v in (C.byref(ok), None, C.byref(_c_voice(1.0, 1.0))):
        assert l.sbv2_pipeline_fetch_request_voice(None, 1, C.byref(req), v, dst.ctypes.data, dst.nbytes, C.byref(got), None, None, None) != 0
        assert b"bad arguments" in l.sbv2_last_error()
    y = np.full(500, 77, np.float32)
    for rate, word in ((999, "sample rate"), (48001, "sample rate")):
        assert l.sbv2_debug_voice_shift(0, x.ctypes.data_as(_lib.f32p), lens.ctypes.data_as(i64p), 1, rate, C.byref(ok), None, None, None, None, None, None,
                                        None, None, y.ctypes.data_as(_lib.f32p)) != 0
        assert word in l.sbv2_last_error().decode(), l.sbv2_last_error()
    per = np.full(3, 200.0)
    assert l.sbv2_debug_voice_shift(0, x.ctypes.data_as(_lib.f32p), lens.ctypes.data_as(i64p), 1, 44100, C.byref(ok), per.ctypes.data_as(f64p), None,
                                    None, None, None, None, None, None, y.ctypes.data_as(_lib.f32p)) != 0
    assert b"together" in l.sbv2_last_error() and (y == 77).all()


def test_options_are_checked_at_construction():
    SO = orchestrator.SynthesizeOptions
    o = SO()
    assert o.pitch_scale == 1.0 and o.intonation_scale == 1.0 and orchestrator.voice_options(o) is None
    v = orchestrator.voice_options(SO(pitch_scale=1.25, intonation_scale=0))
    assert (v.pitch_scale, v.intonation_scale, v.hop) == (1.25, 0.0, 0) and not v.is_identity()
    for kw in (dict(pitch_scale=0.49), dict(pitch_scale=2.01), dict(pitch_scale=float("nan")), dict(pitch_scale="1"), dict(pitch_scale=True),
               dict(pitch_scale=None), dict(intonation_scale=-0.01), dict(intonation_scale=2.5), dict(intonation_scale=float("inf"))):
        with pytest.raises(model.Sbv2Error):
            SO(**kw)
    for kw in (dict(pitch_scale=0.5), dict(pitch_scale=2), dict(intonation_scale=0.0), dict(intonation_scale=2.0)):
        SO(**kw)


# ---- CPU: the routes against fakes --------------------------------------------------------------------------------------------------------------------

STYLES = np.zeros((2, 4), np.float32)
FAKE_HOP = 4


def _sent(tag, phones, word2ph):
    return dict(phones=list(phones), word2ph=list(word2ph), tag=float(tag))


REQUEST = [_sent(0.5, [0, 2, 0, 1, 0], [1, 0, 3, 1]), None, _sent(0.25, [0, 3, 0], [2, 1]), None]


class FakePipe:
    """Row i of a run: phones[t] + 1 frames of FAKE_HOP samples per token, every sample the row's tag; a fetch with a voice multiplies the samples
    by its pitch_scale (so the bytes tell which voice a request was fetched with)."""

    def __init__(self):
        self.calls, self.runs = [], 0

    def prepare(self, utts, **kw):
        lens = np.array([FAKE_HOP * sum(int(p) + 1 for p in u["phones"]) for u in utts], np.int64)
        return types.SimpleNamespace(utts=[dict(u) for u in utts], lens=lens, ticket=None, t_lens=np.array([len(u["phones"]) for u in utts]))

    def run(self, b):
        self.runs += 1
        b.ticket = self.runs
        return b.lens

    def fetch(self, b):
        self.calls.append(dict(plain=True))
        return [np.full(int(n), u["tag"], np.float32) for n, u in zip(b.lens, b.utts)]

    def _fetch(self, b, rows, fmt, place, joined_len, marks, voice):
        t = np.zeros(int(joined_len), np.float32)
        st, en = [], []
        for r, p in zip(rows, place):
            t[p:p + int(b.lens[r])] = b.utts[r]["tag"] * (voice.pitch_scale if voice is not None else 1.0)
            c = p + FAKE_HOP * np.concatenate([[0], np.cumsum([int(x) + 1 for x in b.utts[r]["phones"]])])
            st, en = st + list(c[:-1]), en + list(c[1:])
        out = t.astype(fmt.dtype)
        m = model.Marks(np.array(st), np.array(en), np.zeros(len(st)), np.zeros(len(st)), 0, None, None, len(out)) if marks else None
        return (out, None, m) if marks else (out, None)

    def fetch_request(self, b, rows, fmt, place, joined_len, gain=None, flac=False, marks=False, env_hop=0, levels=True, pitch=None, voice=None):
        self.calls.append(dict(rows=list(rows), marks=marks, voice=None if voice is None else (voice.pitch_scale, voice.intonation_scale, voice.hop)))
        return self._fetch(b, rows, fmt, place, joined_len, marks, voice)

    def close(self):
        pass


class OldPipe(FakePipe):
    """A pipeline from before this option: its fetch_request has no `voice` argument."""

    def fetch_request(self, b, rows, fmt, place, joined_len, gain=None, flac=False, marks=False, env_hop=0, levels=True, pitch=None):
        self.calls.append(dict(rows=list(rows), marks=marks, voice="never named"))
        return self._fetch(b, rows, fmt, place, joined_len, marks, None)


def _payload(wav):
    return np.frombuffer(wav[wav.index(b"data") + 8:], np.float32)


def test_routes_carry_or_refuse_the_scales():
    SO = orchestrator.SynthesizeOptions
    pipe = FakePipe()
    plain = orchestrator.easy_synthesize(pipe, REQUEST, STYLES, noise_seed=1)
    assert pipe.calls[-1] == dict(plain=True)                                  # the defaults: the plain fetch there always was
    wav = orchestrator.easy_synthesize(pipe, REQUEST, STYLES, noise_seed=1, options=SO(pitch_scale=1.5, intonation_scale=0.5))
    assert pipe.calls[-1] == dict(rows=[0, 1], marks=False, voice=(1.5, 0.5, 0))   # ONE fetch of the request's rows, with the voice
    assert len(wav) == len(plain) and (_payload(wav) == np.float32(1.5) * _payload(plain)).all()
    wav2, mk = orchestrator.easy_synthesize_marks(pipe, REQUEST, STYLES, noise_seed=1, options=SO(intonation_scale=1.5))
    assert pipe.calls[-1] == dict(rows=[0, 1], marks=True, voice=(1.0, 1.5, 0)) and _payload(wav2).tobytes() == _payload(plain).tobytes()
    _, mk0 = orchestrator.easy_synthesize_marks(pipe, REQUEST, STYLES, noise_seed=1)
    assert pipe.calls[-1]["voice"] is None and mk == mk0                       # the spans do not move
    # a pipeline that has never heard of `voice` serves every request at the defaults
    old = OldPipe()
    assert orchestrator.easy_synthesize_marks(old, REQUEST, STYLES, noise_seed=1)[0] == wav2
    assert orchestrator.easy_synthesize(old, REQUEST, STYLES, noise_seed=1, options=SO(sample_rate=44100, encoding="s16")) is not None
    assert [c["voice"] for c in old.calls] == ["never named"] * 2
    # streams refuse, before any GPU work, naming the whole-signal routes
    for kw in (dict(), dict(split=True), dict(levels=True)):
        for o in (SO(pitch_scale=1.1), SO(intonation_scale=0.9)):
            with pytest.raises(model.Sbv2Error, match="/synthesize_marks"):
                orchestrator.easy_synthesize_stream(None, None, REQUEST[:1], STYLES, options=o, **kw)
    # the batcher: per request, with marks too
    rb = batcher.RequestBatcher(pipe, start=False, clock=lambda: 0.0, max_wait_ms=1000.0)
    f0 = rb.submit(REQUEST, STYLES, options=SO(pitch_scale=2.0), noise_seed=1)
    f1 = rb.submit(REQUEST, STYLES, options=SO(pitch_scale=0.5), noise_seed=1, marks=True)
    f2 = rb.submit(REQUEST, STYLES, noise_seed=1)
    n = len(pipe.calls)
    rb.start()
    rb.close()
    assert (_payload(f0.result(0)) == np.float32(2.0) * _payload(plain)).all()
    assert (_payload(f1.result(0)[0]) == np.float32(0.5) * _payload(plain)).all() and f1.result(0)[1] == mk0
    assert f2.result(0) == plain
    voices = [c.get("voice") for c in pipe.calls[n:] if "rows" in c]
    assert voices == [(2.0, 1.0, 0), (0.5, 1.0, 0)], pipe.calls[n:]


def test_rest_models_accept_the_scales_and_the_stream_routes_refuse_them():
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient
    from sbv2_api_amd import rest
    wav = orchestrator.array_to_wav(np.zeros((1, 1, 10), np.float32))
    marks = {"sample_rate": 44100, "tokens": [], "words": []}

    class H:
        calls = []

        def easy_synthesize(self, ident, text, style_id, speaker_id, options):
            self.calls.append(("plain", options.pitch_scale, options.intonation_scale))
            return wav

        def easy_synthesize_batched(self, ident, text, style_id, speaker_id, options, batching=None, marks=False):
            from concurrent.futures import Future
            self.calls.append(("batched", options.pitch_scale, options.intonation_scale))
            f = Future()
            f.set_result(wav)
            return f

        def easy_synthesize_marks(self, ident, text, style_id, speaker_id, options):
            self.calls.append(("marks", options.pitch_scale, options.intonation_scale))
            return wav, marks

        def easy_synthesize_stream(self, ident, text, style_id, speaker_id, options, **kw):
            raise AssertionError("a stream with scales must be refused before the holder is asked")

    h = H()
    c = TestClient(rest.make_app(h), raise_server_exceptions=False)
    body = {"text": "x", "ident": "m", "pitch_scale": 1.25, "intonation_scale": 0.5}
    assert c.post("/synthesize", json=body).content == wav and h.calls[-1] == ("plain", 1.25, 0.5)
    assert c.post("/synthesize", json={"text": "x", "ident": "m"}).content == wav and h.calls[-1] == ("plain", 1.0, 1.0)
    assert c.post("/synthesize_marks", json=body).status_code == 200 and h.calls[-1] == ("marks", 1.25, 0.5)
    cb = TestClient(rest.make_app(h, batching={}), raise_server_exceptions=False)
    assert cb.post("/synthesize", json=body).content == wav and h.calls[-1] == ("batched", 1.25, 0.5)
    n = len(h.calls)
    assert c.post("/synthesize", json=dict(body, pitch_scale=2.5)).status_code == 500 and len(h.calls) == n   # out of range: never reaches the holder
    for route in ("/synthesize_stream", "/synthesize_stream_marks"):
        for extra in ({"pitch_scale": 1.25}, {"intonation_scale": 0.5}, {"pitch_scale": 9.0}):
            r = c.post(route, json={"text": "x", "ident": "m", **extra})
            assert 400 <= r.status_code < 500 and "/synthesize_marks" in r.text, (route, r.status_code, r.text)


# ---- CPU: the reference judged as a shifter -----------------------------------------------------------------------------------------------------------

def _mean_f0(f0, voiced):
    q = np.rint(f0[voiced] * 65536.0).astype(np.int64)
    return float(int(q.sum())) / (65536.0 * q.size)


@pytest.mark.parametrize("sr,hop", SIGNALS)
def test_the_reference_leaves_no_marginal_frame_and_keeps_its_promises(sr, hop):
    x = signal(sr)
    r, T = signal_contour(sr, hop)
    assert not r.marginal.any() and r.voiced.any() and not r.voiced.all()
    same = voice_ref(x, sr, 1.0, 1.0, hop, T, r.voiced)
    assert same.y.tobytes() == x.tobytes() and np.array_equal(same.ta, same.ts) and np.array_equal(same.map, np.arange(same.ta.size))
    # samples of unvoiced frames farther than tau_max + hop + 2 from every voiced frame
    vs = (r.voiced != 0)[np.arange(x.size) // hop]
    reach = r.tau_max + hop + 2
    near = np.convolve(vs.astype(np.float64), np.ones(2 * reach + 1), "same") > 0.5
    far = ~near
    assert far.sum() > 500
    for p, s in PAIRS:
        o = shifted_ref(sr, hop, p, s)
        assert o.y.size == x.size and o.y.dtype == np.float32
        assert np.abs(o.y).max() <= np.abs(x).max(), (p, s)
        assert (o.y[far] == x[far]).all(), (p, s)
        assert o.y.tobytes() != x.tobytes()


@pytest.mark.parametrize("p,s", PAIRS)
@pytest.mark.parametrize("sr,hop", SIGNALS)
def test_the_reference_shifts_the_pitch(sr, hop, p, s):
    """f0 of the output (yin_ref again) against clip(p (m + s (f0_in - m))) on the frames voiced in both contours.  Measured when written, worst
    pair of each signal: 44.1 kHz median 0.30 %, 90th percentile 1.55 %, voiced in both 90.5 %; 16 kHz 0.34 %, 1.55 %, 88.2 %."""
    r, T = signal_contour(sr, hop)
    vin = r.voiced != 0
    f0 = np.where(vin, sr / np.where(vin, T, 1.0), 0.0)
    m = _mean_f0(f0, vin)
    o = shifted_ref(sr, hop, p, s)
    ro = yin_ref(o.y.astype(np.float64), sr, hop)
    both = vin & (ro.voiced != 0)
    target = np.clip(p * (m + s * (f0 - m)), F0_MIN / 2.0, 2.0 * F0_MAX)
    err = np.abs(ro.f0[both] - target[both]) / target[both]
    med, p90, share = float(np.median(err)), float(np.percentile(err, 90)), both.sum() / vin.sum()
    print(f"[voice] {sr} Hz p = {p} s = {s}: median {100 * med:.3f} %, 90th percentile {100 * p90:.3f} %, voiced in both {100 * share:.1f} %")
    assert med <= 0.01 and p90 <= 0.03 and share >= 0.85, (med, p90, share)


# ---- GPU: the kernels against the reference -------------------------------------------------------------------------------------------------------------

def assert_equal_to_ref(got, x, sr, p, s, hop, what, **kw):
    """One row of debug_voice_shift against voice_ref fed the device's own contour: marks and map equal, y bit-equal."""
    ref = voice_ref(x, sr, p, s, hop, got.period, got.voiced, **kw)
    assert got.y.size == x.size, what
    np.testing.assert_array_equal(got.ta, ref.ta, err_msg=what + ": ta")
    np.testing.assert_array_equal(got.ts, ref.ts, err_msg=what + ": ts")
    np.testing.assert_array_equal(got.map, ref.map, err_msg=what + ": map")
    bad = np.nonzero(got.y.view(np.uint32) != ref.y.view(np.uint32))[0]
    assert bad.size == 0, (what, "y differs at", bad[:8], got.y[bad[:8]], ref.y[bad[:8]])
    return ref


@gpu
@pytest.mark.parametrize("p,s", PAIRS + [(1.0, 1.0)])
@pytest.mark.parametrize("sr,hop", SIGNALS)
def test_hook_equals_the_reference(sr, hop, p, s):
    x = signal(sr)
    got, = model.debug_voice_shift(x, sr, model.Voice(p, s, hop=hop))
    ref = assert_equal_to_ref(got, x, sr, p, s, hop, f"{sr} Hz p = {p} s = {s}")
    assert got.voiced.any() and ref.ts.size > 20
    if (p, s) == (1.0, 1.0):                                                   # forced through the kernels: the identity
        assert got.y.tobytes() == x.tobytes() and np.array_equal(got.ta, got.ts)
    else:
        assert got.y.tobytes() != x.tobytes() and np.abs(got.y).max() <= np.abs(x).max()
    again, = model.debug_voice_shift(x, sr, model.Voice(p, s, hop=hop))
    assert again.y.tobytes() == got.y.tobytes() and again.period.tobytes() == got.period.tobytes()   # every order is fixed


@gpu
@pytest.mark.parametrize("sr,hop", SIGNALS)
def test_device_contour_against_the_reference(sr, hop):
    """YIN on f32 under the rule of tests/test_pitch.py (c within 1e-9, marginal frames exempt, at most 2 % of them; the signals leave none),
    and the refinement on the device: period_out has the bits of the header's expression on the device's own c values."""
    x = signal(sr)
    r, T = signal_contour(sr, hop)
    got, = model.debug_voice_shift(x, sr, model.Voice(1.2, 1.0, hop=hop))
    pitch, c3, voiced = model.debug_pitch(x, sr, model.Pitch(hop))
    keep = ~r.marginal
    assert r.marginal.sum() <= 0.02 * r.lag.size
    np.testing.assert_array_equal(got.voiced[keep], r.voiced[keep])
    np.testing.assert_array_equal(got.voiced, voiced)
    np.testing.assert_array_equal(pitch.lag[keep], r.lag[keep])
    err = float(np.abs(c3[keep] - r.c3[keep]).max())
    print(f"[voice] {sr} Hz: f32 c error worst {err:.3e}, {int(r.marginal.sum())} of {r.lag.size} frames marginal")
    assert err <= 1e-9
    dev = types.SimpleNamespace(c3=c3, lag=pitch.lag, tau_max=r.tau_max)
    assert got.period.tobytes() == periods_of(dev).tobytes()
    np.testing.assert_allclose(got.period[keep], T[keep], rtol=1e-6, atol=0)


def _rows_16k():
    """The packed rows of one call at 16 kHz, hop 80 (tau_min 26, tau_max 229), named."""
    sr = 16000
    x = signal(sr)
    tile = model.voice_tile()
    rng = np.random.default_rng(2)
    t = np.arange(2000) / sr
    tone = sum(np.sin(2 * np.pi * k * 150.0 * t + k) / k for k in range(1, 5))
    tone = (tone / np.abs(tone).max() * 0.7).astype(np.float32)
    a = 50 * sr // 1000                                                         # the tone of `signal` starts here
    rows = [("empty", np.zeros(0, np.float32)), ("one sample", x[a + 5:a + 6]), ("shorter than tau_min", x[a:a + 20]),
            ("one period", tone[:107]), ("no multiple of the hop", x[:1234]), ("all noise", (rng.standard_normal(2000) * 0.05).astype(np.float32)),
            ("all tone", tone), ("cut inside a voiced frame", x[:a + 1600 + 37]), ("tile - 1", x[a + 100:a + 100 + 5 * tile - 1]),
            ("tile", x[a + 100:a + 100 + 5 * tile]), ("tile + 1", x[a + 100:a + 100 + 5 * tile + 1]), ("one tile - 1", tone[:tile - 1]),
            ("one tile", tone[:tile]), ("one tile + 1", tone[:tile + 1])]
    return sr, 80, rows


@gpu
def test_packed_rows_of_every_edge_shape_in_one_call():
    sr, hop, rows = _rows_16k()
    assert lags_np(sr) == (26, 229)
    got = model.debug_voice_shift([r for _, r in rows], sr, model.Voice(1.3, 0.8, hop=hop))
    assert len(got) == len(rows)
    seen = {}
    for (name, x), g in zip(rows, got):
        ref = assert_equal_to_ref(g, x, sr, 1.3, 0.8, hop, name)
        assert g.period.size == g.voiced.size == (-(-x.size // hop) if x.size else 0), name
        seen[name] = (g, ref)
    assert seen["empty"][0].y.size == 0 and seen["one sample"][0].y.tobytes() == rows[1][1].tobytes()
    g, ref = seen["all noise"]
    assert not g.voiced.any() and g.y.tobytes() == rows[5][1].tobytes() and np.array_equal(g.ta, g.ts)   # an exact copy
    g, ref = seen["all tone"]
    inside = [f for f in range(g.voiced.size) if f * hop + hop // 2 - 229 >= 0 and f * hop + hop // 2 + 229 <= 2000]   # (the row's ends read zeros)
    assert len(inside) >= 15 and g.voiced[inside].all() and g.y.tobytes() != rows[6][1].tobytes() and g.ts.size > g.ta.size
    g, ref = seen["cut inside a voiced frame"]
    cut = rows[7][1].size
    assert cut % hop and signal_contour(sr, hop)[0].voiced[cut // hop] == 1 and g.voiced.any()   # voiced in the uncut signal
    for name in ("tile - 1", "tile", "tile + 1"):
        assert seen[name][0].voiced.any() and seen[name][0].y.tobytes() != dict(rows)[name].tobytes()
    # a row's result does not depend on its neighbours: the same rows in another order and alone
    back = model.debug_voice_shift([r for _, r in rows[::-1]], sr, model.Voice(1.3, 0.8, hop=hop))[::-1]
    for (name, _), g, h in zip(rows, got, back):
        assert g.y.tobytes() == h.y.tobytes() and np.array_equal(g.ts, h.ts), name
    alone, = model.debug_voice_shift(rows[7][1], sr, model.Voice(1.3, 0.8, hop=hop))
    assert alone.y.tobytes() == got[7].y.tobytes()


@gpu
def test_a_given_contour_gives_the_reference_bits():
    """period_in: a constant 200-sample period over a pulse train with one unvoiced gap; everything behind the contour is exact arithmetic."""
    sr, hop = 44100, 220
    n = 40 * hop + 57
    x = np.zeros(n, np.float32)
    x[::200] = 0.5
    x += (np.random.default_rng(3).standard_normal(n) * 0.01).astype(np.float32)
    nf = -(-n // hop)
    period, voiced = np.full(nf, 200.0), np.ones(nf, np.int32)
    voiced[15:22] = 0
    period[15:22] = 12345.0                                                     # (an unvoiced frame's period is not looked at)
    for p, s in ((1.3, 0.8), (0.5, 1.0), (2.0, 0.0), (1.0, 1.0)):
        got, = model.debug_voice_shift(x, sr, model.Voice(p, s, hop=hop), period=period, voiced=voiced)
        assert got.period[voiced != 0].tobytes() == period[voiced != 0].tobytes() and np.array_equal(got.voiced, voiced)
        ref = voice_ref(x, sr, p, s, hop, period, voiced)
        np.testing.assert_array_equal(got.ta, ref.ta)
        np.testing.assert_array_equal(got.ts, ref.ts)
        np.testing.assert_array_equal(got.map, ref.map)
        assert got.y.tobytes() == ref.y.tobytes(), (p, s)
        if p == 1.0:
            assert got.y.tobytes() == x.tobytes()
        else:                                                                   # a constant contour: the synthesis marks are p times as dense
            inside = (ref.ts > 0) & (ref.ts < 15 * hop)
            assert abs(np.diff(ref.ts[inside]).mean() - 200.0 / p) < 1.0
    with pytest.raises(model.Sbv2Error, match="period_in"):
        model.debug_voice_shift(x, sr, model.Voice(1.3, 0.8, hop=hop), period=np.full(nf, 5000.0), voiced=voiced)
    with pytest.raises(model.Sbv2Error, match="period_in"):
        model.debug_voice_shift(x, sr, model.Voice(1.3, 0.8, hop=hop), period=np.full(nf, np.nan), voiced=voiced)


# ---- GPU: the pipeline ----------------------------------------------------------------------------------------------------------------------------------

VOICE = (1.3, 0.8)


@pytest.fixture(scope="module")
def five_rows():
    bc, _ = weights("bert", "tiny", 3)
    vc, _ = weights("vits", "tiny", 5)
    bs, vs = model.load_model(blob("bert", "tiny", 3), True), model.load_model(blob("vits", "tiny", 5), False)
    pipe = model.Pipeline(bs, vs)
    b = pipe.prepare(make_utts([9, 1, 23, 14, 40], bc, vc, seed0=501, with_bert=False), forced=True)
    pipe.run(b)
    native = [x.copy() for x in pipe.fetch(b)]
    rows = [3, 1]
    place = [1000, 1000 + len(native[3]) + 22050]
    joined = place[1] + len(native[1]) + 333
    shifted = {r: g.y for r, g in zip(rows, model.debug_voice_shift([native[r] for r in rows], 44100, model.Voice(*VOICE)))}
    yield types.SimpleNamespace(pipe=pipe, b=b, native=native, rows=rows, place=place, joined=joined, shifted=shifted)
    pipe.close(); bs.close(); vs.close()


def _join(signals, rows, place, joined):
    t = np.zeros(joined, np.float32)
    for r, p in zip(rows, place):
        t[p:p + len(signals[r])] = signals[r]
    return t


@gpu
def test_pipeline_voice_is_the_hook_on_the_native_rows(five_rows):
    c = five_rows
    pipe, b, rows, place, joined = c.pipe, c.b, c.rows, c.place, c.joined
    f0 = model.PcmFormat()
    plain = pipe.fetch_request(b, rows, f0, place, joined)[0].copy()
    assert plain.tobytes() == _join(c.native, rows, place, joined).tobytes()
    for v in (None, model.Voice(1.0, 1.0)):                                     # no voice, and the identity: the bytes of fetch_request
        assert pipe.fetch_request(b, rows, f0, place, joined, voice=v)[0].tobytes() == plain.tobytes()
    changed = [r for r in rows if c.shifted[r].tobytes() != c.native[r].tobytes()]
    print(f"[voice] rows {rows}: {len(changed)} changed by Voice{VOICE}")
    assert changed, "the synthetic rows hold no voiced frame: the pipeline tests would show nothing"
    want = _join(c.shifted, rows, place, joined)
    got = pipe.fetch_request(b, rows, f0, place, joined, voice=model.Voice(*VOICE))[0].copy()
    assert got.dtype == np.float32 and got.tobytes() == want.tobytes()
    assert pipe.fetch_request(b, rows, f0, place, joined, voice=model.Voice(*VOICE))[0].tobytes() == got.tobytes()   # twice: identical
    assert pipe.fetch_request(b, rows, f0, place, joined)[0].tobytes() == plain.tobytes()                            # the run's PCM was only read
    assert [x.tobytes() for x in pipe.fetch(b)] == [x.tobytes() for x in c.native]
    # 16 kHz s16: the formatter's launches on the shifted rows
    f = model.PcmFormat(16000, "s16")
    s16 = pipe.fetch_request(b, rows, f, place, joined, voice=model.Voice(*VOICE))[0].copy()
    x = np.concatenate([c.shifted[r] for r in rows])
    pieces = [(0, place[0], len(c.shifted[rows[0]])), (len(c.shifted[rows[0]]), place[1], len(c.shifted[rows[1]]))]
    ref = model.debug_pcm_format(x, pieces, [(0, model.pcm_format_length(f, joined), 0, 2)], f)[0]
    assert s16.dtype == np.int16 and s16.tobytes() == ref.tobytes()
    assert s16.tobytes() != pipe.fetch_request(b, rows, f, place, joined)[0].tobytes()
    # the FLAC sink decodes to the s16 fetch
    fl = pipe.fetch_request(b, rows, f, place, joined, flac=True, voice=model.Voice(*VOICE))[0]
    d = R.read(fl)
    assert d["rate"] == 16000 and np.asarray(d["samples"], np.int16).tobytes() == s16.tobytes()
    # a refusal through the handle writes nothing and leaves the ticket fetchable
    with pytest.raises(model.Sbv2Error, match="pitch_scale"):
        pipe.fetch_request(b, rows, f0, place, joined, voice=model.Voice(2.5, 1.0))
    assert pipe.fetch_request(b, rows, f0, place, joined, voice=model.Voice(*VOICE))[0].tobytes() == got.tobytes()


@gpu
def test_pipeline_voice_with_marks_pitch_and_gain(five_rows):
    c = five_rows
    pipe, b, rows, place, joined = c.pipe, c.b, c.rows, c.place, c.joined
    v = lambda: model.Voice(*VOICE)
    f = model.PcmFormat(16000, "s16")
    hop = 160
    plain, _, pm = pipe.fetch_request(b, rows, f, place, joined, marks=True, env_hop=hop)
    want = pipe.fetch_request(b, rows, f, place, joined, voice=v())[0].copy()
    out, _, m, p = pipe.fetch_request(b, rows, f, place, joined, marks=True, env_hop=hop, pitch=model.Pitch(hop), voice=v())
    assert out.tobytes() == want.tobytes()
    assert m.start.tobytes() == pm.start.tobytes() and m.end.tobytes() == pm.end.tobytes()       # the spans are those without voice
    ss, pk = model.debug_segment_levels(out, m.start, m.end)
    assert ss.tobytes() == m.sumsq.tobytes() and pk.tobytes() == m.peak.tobytes()               # the levels of the delivered, shifted samples
    nenv = len(m.env_sumsq)
    es, ep = model.debug_segment_levels(out, np.arange(nenv) * hop, np.minimum((np.arange(nenv) + 1) * hop, len(out)))
    assert es.tobytes() == m.env_sumsq.tobytes() and ep.tobytes() == m.env_peak.tobytes()
    h, _, _ = model.debug_pitch(out, 16000, model.Pitch(hop))
    assert h.f0.tobytes() == p.f0.tobytes() and h.ap.tobytes() == p.ap.tobytes() and (h.lag == p.lag).all()
    # loudness and limiter compose: their stats are those of the debug hooks on the shifted signal (identity format: the samples themselves)
    f0 = model.PcmFormat()
    t = _join(c.shifted, rows, place, joined).astype(np.float64)
    ln, lim = model.Loudness(-23.0, -1.0), model.Limiter(-16.0, -1.0, 6.0)
    got, st = pipe.fetch_request(b, rows, f0, place, joined, gain=ln, voice=v())
    ref = model.debug_loudness([t], 44100, ln)[0]
    print(f"[voice] loudness stats {st} vs the hook's {ref}")
    np.testing.assert_allclose(st, ref, rtol=0, atol=1e-9)
    np.testing.assert_allclose(got, (t * 10 ** (ref[2] / 20)).astype(np.float32), rtol=1e-6, atol=1e-9)
    plain_st = pipe.fetch_request(b, rows, f0, place, joined, gain=ln)[1]
    assert plain_st.tobytes() != st.tobytes()
    got, st = pipe.fetch_request(b, rows, f0, place, joined, gain=lim, voice=v())
    ref_y, ref = model.debug_limiter([t], 44100, lim)
    print(f"[voice] limiter stats {st} vs the hook's {ref[0]}")
    np.testing.assert_allclose(st, ref[0], rtol=0, atol=1e-9)
    np.testing.assert_allclose(got, ref_y[0].astype(np.float32), rtol=1e-6, atol=1e-9)


@gpu
def test_batcher_and_rest_carry_the_scales(monkeypatch):
    """The synthetic voices are noise at the reference's noise scales and YIN finds nothing to move in them: this test runs every route without
    the decoder's noise (the batcher takes its scales from the orchestrator's constants), where the synthetic rows are periodic."""
    monkeypatch.setattr(orchestrator, "NOISE_SCALE", 0.0)
    monkeypatch.setattr(orchestrator, "NOISE_SCALE_W", 0.0)
    quiet = dict(noise_scale=0.0, noise_scale_w=0.0)
    bs, vs = model.load_model(blob("bert", "tiny", 3), True), model.load_model(blob("vits", "tiny", 5), False)
    bc, _ = weights("bert", "tiny", 3)
    vc, _ = weights("vits", "tiny", 5)
    keys = ("input_ids", "word2ph", "phones", "tones", "langs")
    sv = synth.hash_normal(77, 3 * vc["style_dim"]).reshape(3, -1).astype(np.float32) * 0.1
    SO = orchestrator.SynthesizeOptions
    o1, o2 = (lambda: SO(pitch_scale=1.3, intonation_scale=0.8)), (lambda: SO(sample_rate=16000, encoding="s16", pitch_scale=0.7))
    pipe = model.Pipeline(bs, vs)
    try:
        # take the first request in which both scales find voiced frames to move (or the test shows nothing)
        for seed0 in range(151, 175):
            sents = [{k: u[k] for k in keys} for u in make_utts([14, 40], bc, vc, seed0=seed0, with_bert=False)]
            plain = orchestrator.easy_synthesize(pipe, sents, sv, 1, 0, SO(), noise_seed=4242, **quiet)
            alone1 = orchestrator.easy_synthesize(pipe, sents, sv, 1, 0, o1(), noise_seed=4242, **quiet)
            alone2, marks2 = orchestrator.easy_synthesize_marks(pipe, sents, sv, 1, 0, o2(), noise_seed=99, **quiet)
            plain2 = orchestrator.easy_synthesize(pipe, sents, sv, 1, 0, SO(sample_rate=16000, encoding="s16"), noise_seed=99, **quiet)
            if alone1 != plain and alone2 != plain2:
                break
        print(f"[voice] the request of seed {seed0}")
        assert len(alone1) == len(plain) and alone1 != plain                    # the length is kept, the samples are not
        assert len(alone2) == len(plain2) and alone2 != plain2
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

        c = TestClient(rest.make_app(H()), raise_server_exceptions=False)
        r = c.post("/synthesize", json={"text": "x", "ident": "m", "style_id": 1, "pitch_scale": 1.3, "intonation_scale": 0.8})
        assert r.status_code == 200 and r.content == alone1
        assert c.post("/synthesize", json={"text": "x", "ident": "m", "style_id": 1}).content == plain
        for route in ("/synthesize_stream", "/synthesize_stream_marks"):
            r = c.post(route, json={"text": "x", "ident": "m", "style_id": 1, "pitch_scale": 1.3})
            assert 400 <= r.status_code < 500, (route, r.status_code)
    finally:
        pipe.close(); bs.close(); vs.close()
