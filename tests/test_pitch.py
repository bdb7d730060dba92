"""The pitch contour of the speech marks (sbv2_pitch, sbv2_pipeline_fetch_request_pitch, sbv2_pitch_lags, sbv2_debug_pitch; k_pitch_yin in
csrc/marks.hip): the host-side checks and a numpy restatement of the estimator judged as an estimator (CPU), the orchestrator / batcher / REST
contracts against fakes (CPU), the kernel launch by launch against that restatement, and the pipeline, batcher and REST on tiny models (GPU).

The reference is `yin_ref` below: the section above sbv2_pitch in include/sbv2_hip.h restated in numpy, int64 for the integer encodings (s16,
and the integers G.711 codes decode to), float64 for f32.

Tolerances.  Integer encodings: d and S are integers, d tau and S stay below 2^53 (asserted where the bound is reached), so c = d tau / S has
one rounding and lag, voiced and the three c values are EQUAL to numpy's, bit for bit; f0 and ap are host arithmetic of those (asserted within
1e-12 relative, the library's is C++ and numpy's is numpy).  f32: only the order of the sums differs, c within 1e-9; a frame whose decision the
reference itself takes by less than 1e-9 (`marginal`) is exempt from the lag / voiced comparison, at most 2 % of the frames, and the seeds are
chosen so that the reference leaves out none (asserted on the CPU).  f32 samples that are s16 integers / 32768 give the s16 bits: the power of
two cancels in c."""
import base64
import ctypes as C
import functools
import json
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
NEW_SYMBOLS = ["sbv2_pipeline_fetch_request_pitch", "sbv2_pitch_lags", "sbv2_debug_pitch"]
ALL_RATES = [8000, 16000, 22050, 24000, 32000, 44100, 48000]
RATES = [8000, 16000, 44100, 48000]
F0_MIN, F0_MAX, THRESHOLD = 70.0, 600.0, 0.15
TONES = [75.3, 110.0, 173.9, 261.6, 392.0, 555.5]
MARGIN = 1e-9
f64p, i32p = C.POINTER(C.c_double), C.POINTER(C.c_int32)


# ---- the reference ----------------------------------------------------------------------------------------------------------------------------------

def mulaw_decode_np(code):
    u = ~np.asarray(code, np.uint8).astype(np.int64) & 0xFF
    t = (((u & 15) << 3) + 132) << ((u >> 4) & 7)
    return np.where(u & 0x80, 132 - t, t - 132)


def alaw_decode_np(code):
    a = np.asarray(code, np.uint8).astype(np.int64) ^ 0x55
    e = (a >> 4) & 7
    t = ((a & 15) << 4) + 8
    t = np.where(e >= 1, (t + 256) << np.maximum(e - 1, 0), t)
    return np.where(a & 0x80, t, -t)


def values_of(x, encoding=None):
    """The values the estimator reads: int64 for the integer encodings, float64 for f32."""
    x = np.asarray(x)
    if encoding == "mulaw":
        return mulaw_decode_np(x)
    if encoding == "alaw":
        return alaw_decode_np(x)
    return x.astype(np.int64) if x.dtype == np.int16 else x.astype(np.float64)


def lags_np(sr, f0_min=F0_MIN, f0_max=F0_MAX):
    return math.floor(sr / f0_max), math.ceil(sr / f0_min)


def yin_ref(v, sr, hop, f0_min=F0_MIN, f0_max=F0_MAX, threshold=THRESHOLD):
    """YIN steps 2 - 5 as include/sbv2_hip.h states them, on v (int64 or float64).  Returns a namespace of per-frame arrays: lag, voiced, c3
    (c(lag - 1), c(lag), c(lag + 1)), f0, ap, marginal (the decision hangs on a difference below MARGIN), and the largest d tau and S met."""
    v = np.asarray(v)
    assert v.dtype in (np.int64, np.float64)
    n = v.size
    tau_min, tau_max = lags_np(sr, f0_min, f0_max)
    W = tau_max
    nf = -(-n // hop) if n else 0
    tau = np.arange(1, W + 1)
    out = types.SimpleNamespace(lag=np.zeros(nf, np.int32), voiced=np.zeros(nf, np.int32), c3=np.zeros((nf, 3)), f0=np.zeros(nf), ap=np.zeros(nf),
                                marginal=np.zeros(nf, bool), max_dtau=0, max_S=0, tau_min=tau_min, tau_max=tau_max)
    for f in range(nf):
        b = f * hop + hop // 2 - tau_max
        idx = b + np.arange(2 * W)
        ok = (idx >= 0) & (idx < n)
        w = np.where(ok, v[np.clip(idx, 0, max(n - 1, 0))], 0).astype(v.dtype)
        rows = np.lib.stride_tricks.sliding_window_view(w, W)[1:W + 1]          # row tau - 1 = w[tau : tau + W]
        e = w[None, :W] - rows
        d = (e * e).sum(axis=1)                                                  # int64: exact; float64: numpy's order
        S = np.cumsum(d)
        if v.dtype == np.int64:
            out.max_dtau, out.max_S = max(out.max_dtau, int((d * tau).max())), max(out.max_S, int(S.max()))
        with np.errstate(invalid="ignore", divide="ignore"):
            c = np.where(S == 0, 1.0, d.astype(np.float64) * tau.astype(np.float64) / S.astype(np.float64))
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
            lag = tau_min + int(np.argmin(c[tau_min:tau_max + 1]))               # (argmin: the first of equal minima)
            # ... unless another lag comes within MARGIN of it (two values that are both 1 by the S = 0 rule are equal by definition, not by
            # arithmetic: every implementation has them equal, as in a silent window)
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
        out.ap[f] = c0
    return out


# ---- the signals --------------------------------------------------------------------------------------------------------------------------------------

def tone(f0, sr, seconds=0.25):
    """Harmonics 1 .. 4 of f0, amplitude 1 / k, phase k, peak 0.7 of full scale, quantised to s16."""
    t = np.arange(int(seconds * sr)) / sr
    x = sum(np.sin(2 * np.pi * k * f0 * t + k) / k for k in range(1, 5))
    return np.round(x / np.abs(x).max() * 0.7 * 32767).astype(np.int16)


def noise(sr, seed, seconds=0.25):
    """Gaussian noise of sigma = 0.05 full scale, s16."""
    return np.round(np.random.default_rng(seed).standard_normal(int(seconds * sr)) * 0.05 * 32767).astype(np.int16)


@functools.lru_cache(maxsize=None)
def medley(sr):
    """The six tones and the noise, one after the other (the changes between them are frames of their own kind)."""
    return np.concatenate([tone(f, sr) for f in TONES] + [noise(sr, 5)])


@functools.lru_cache(maxsize=None)
def glide(sr=16000):
    """A noise head, a glide from 110 to 220 Hz (harmonics 1 .. 3), a silent tail."""
    n = int(0.4 * sr)
    f = np.linspace(110.0, 220.0, n)
    ph = 2 * np.pi * np.cumsum(f) / sr
    x = sum(np.sin(k * ph) / k for k in range(1, 4))
    g = np.round(x / np.abs(x).max() * 0.6 * 32767).astype(np.int16)
    return np.concatenate([noise(sr, 9, 0.1), g, np.zeros(int(0.1 * sr), np.int16)])


def encoded(x, encoding):
    """s16 samples as the hook takes them under `encoding`: themselves, or their G.711 codes."""
    return x if encoding == "s16" else model.g711_encode(x, encoding)


@functools.lru_cache(maxsize=None)
def medley_ref(sr, encoding):
    x = encoded(medley(sr), encoding)
    return x, yin_ref(values_of(x, None if encoding == "s16" else encoding), sr, sr // 100)


F32_SEEDS = [11, 12]


@functools.lru_cache(maxsize=None)
def f32_case(seed, sr=16000):
    """A seeded Gaussian f32 signal with a voiced stretch: noise throughout, a 140 Hz tone over its middle half."""
    rng = np.random.default_rng(seed)
    n = int(0.3 * sr)
    x = rng.standard_normal(n) * 0.03
    x[n // 4:3 * n // 4] += 0.4 * tone(140.0, sr, 0.3)[n // 4:3 * n // 4] / 32767.0
    x = x.astype(np.float32)
    return x, yin_ref(x.astype(np.float64), sr, sr // 100)


# ---- CPU: ABI -------------------------------------------------------------------------------------------------------------------------------------------

def test_new_symbols_are_exported_and_declared():
    header = open(os.path.join(ROOT, "include", "sbv2_hip.h")).read()
    l = _lib.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.SYMBOLS and getattr(l, name) is not None, name
    assert "} sbv2_pitch;" in header
    assert C.sizeof(_lib.Sbv2Pitch) == 72
    assert C.sizeof(_lib.Sbv2Marks) == 88                    # the existing struct is as it was


@pytest.mark.parametrize("rate", ALL_RATES)
def test_pitch_lags_agree_with_the_formula(rate):
    for lo, hi in ((F0_MIN, F0_MAX), (40.0, rate / 4), (40.0, 40.5), (123.4, 567.8), (75.0, 500.0)):
        assert model.pitch_lags(rate, lo, hi) == lags_np(rate, lo, hi), (rate, lo, hi)
    assert model.pitch_lags(rate, 40.0, 2000.0)[1] <= 1200   # the bound the exactness of the integer encodings rests on
    assert model.pitch_lags(48000, 40.0, 600.0) == (80, 1200)


def _c_pitch(n, hop=160, f0_min=F0_MIN, f0_max=F0_MAX, threshold=THRESHOLD, reserved=0, capacity=None, fill=77):
    a = types.SimpleNamespace(f0=np.full(n + 2, fill, np.float64), ap=np.full(n + 2, fill, np.float64), lag=np.full(n + 2, fill, np.int32))
    a.c = _lib.Sbv2Pitch(hop, reserved, f0_min, f0_max, threshold, n if capacity is None else capacity, C.cast(a.f0.ctypes.data + 8, f64p),
                         C.cast(a.ap.ctypes.data + 8, f64p), C.cast(a.lag.ctypes.data + 4, i32p), -9)   # (one guard entry in front, one behind)
    a.untouched = lambda: all((x == fill).all() for x in (a.f0, a.ap, a.lag)) and a.c.n_frames == -9
    a.guards = lambda: all(x[0] == fill and x[-1] == fill for x in (a.f0, a.ap, a.lag))
    return a


BAD_PARAMETERS = [(dict(f0_min=39.9), "f0_min"), (dict(f0_max=4000.1), "f0_max"), (dict(f0_min=600.0), "below f0_max"),
                  (dict(f0_min=700.0), "below f0_max"), (dict(threshold=0.0), "threshold"), (dict(threshold=1.0), "threshold"),
                  (dict(hop=0), "hop"), (dict(reserved=1), "reserved"), (dict(f0_min=float("nan")), "f0_min"),
                  (dict(threshold=float("nan")), "threshold")]


def test_pitch_refusals_that_need_no_run():
    l = _lib.lib()
    a, b = C.c_int32(-5), C.c_int32(-5)
    for args, word in (((16000, 39.9, 600.0), "f0_min"), ((16000, 70.0, 4000.1), "f0_max"), ((8000, 70.0, 2000.5), "f0_max"),
                       ((16000, 600.0, 600.0), "below f0_max"), ((16000, 700.0, 600.0), "below f0_max"), ((0, 70.0, 600.0), "sample rate"),
                       ((96000, 70.0, 600.0), "sample rate"), ((16000, float("nan"), 600.0), "f0_min")):
        assert l.sbv2_pitch_lags(*args, C.byref(a), C.byref(b)) != 0, args
        assert word in l.sbv2_last_error().decode(), (args, l.sbv2_last_error())
        assert a.value == -5 and b.value == -5
    assert l.sbv2_pitch_lags(16000, 70.0, 600.0, None, None) != 0
    # threshold, hop and reserved travel in sbv2_pitch: refused by the fetch before the handle is looked at, with nothing written
    f = model.PcmFormat(16000, "s16")
    rows, place = np.array([0], np.int32), np.array([0], np.int64)
    dst, got = np.full(16, 77, np.uint8), C.c_int64(-5)
    req = _lib.Sbv2FetchRequest(rows.ctypes.data_as(C.POINTER(C.c_int32)), 1, place.ctypes.data_as(_lib.i64p), 10, C.pointer(f.c), None, None, 0)
    call = lambda q: l.sbv2_pipeline_fetch_request_pitch(None, 1, C.byref(req), dst.ctypes.data, dst.nbytes, C.byref(got), None, None, C.byref(q.c))
    for kw, word in BAD_PARAMETERS:
        q = _c_pitch(4, **kw)
        assert call(q) != 0, kw
        assert word in l.sbv2_last_error().decode(), (kw, l.sbv2_last_error())
        assert q.untouched() and (dst == 77).all() and got.value == -5
    q = _c_pitch(4)
    q.c.f0 = None
    assert call(q) != 0 and b"f0 must not be NULL" in l.sbv2_last_error()
    q = _c_pitch(4)
    assert call(q) != 0 and b"bad arguments" in l.sbv2_last_error()    # everything static passed: the null handle itself
    assert q.untouched() and (dst == 77).all() and got.value == -5


# ---- CPU: the restatement as an estimator -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rate", RATES)
def test_the_reference_finds_the_tones_and_leaves_noise_and_silence_unvoiced(rate):
    """Steady frames (centre more than 2 tau_max from both ends of a tone) are voiced and within 1 % of the truth; measured worst cases of the
    restatement: 0.28 % at 8 kHz, 0.05 % at 16 kHz, under 0.01 % at 44.1 / 48 kHz.  The 1 % is about the estimator's design: the kernel's
    correctness is carried by the bit comparisons further down."""
    hop = rate // 100
    tau_max = lags_np(rate)[1]
    worst, nearest = 0.0, np.inf
    for f0 in TONES:
        x = tone(f0, rate)
        r = yin_ref(values_of(x), rate, hop)
        centre = np.arange(r.lag.size) * hop + hop // 2
        steady = (centre > 2 * tau_max) & (centre < x.size - 2 * tau_max)
        assert steady.sum() >= 5, (rate, f0)
        assert (r.voiced[steady] == 1).all(), (rate, f0)
        err = np.abs(r.f0[steady] / f0 - 1.0).max()
        worst, nearest = max(worst, err), min(nearest, np.abs(r.ap[steady] - THRESHOLD).min())
        assert err < 0.01, (rate, f0, err)
    for x in (noise(rate, 5), np.zeros(rate // 4, np.int16)):
        r = yin_ref(values_of(x), rate, hop)
        assert r.lag.size == -(-x.size // hop) and (r.voiced == 0).all() and (r.f0 == 0).all()
        nearest = min(nearest, np.abs(r.ap - THRESHOLD).min())
        assert (r.lag >= lags_np(rate)[0]).all() and (r.lag <= tau_max).all()
    assert (yin_ref(np.zeros(rate // 4, np.int64), rate, hop).ap == 1.0).all()     # S = 0: c = 1
    print(f"[pitch] {rate} Hz: worst f0 error on steady frames {100 * worst:.3f} %, nearest c(lag) to the threshold {nearest:.3f}")


def test_the_f32_seeds_leave_no_marginal_frame_and_the_scaled_s16_reference_has_the_s16_bits():
    for seed in F32_SEEDS:
        x, r = f32_case(seed)
        assert not r.marginal.any(), seed
        assert r.voiced.any() and not r.voiced.all()          # both decisions are exercised
    x = medley(8000)
    a, b = yin_ref(values_of(x), 8000, 80), yin_ref((x / 32768.0).astype(np.float32).astype(np.float64), 8000, 80)
    assert a.c3.tobytes() == b.c3.tobytes() and (a.lag == b.lag).all() and (a.voiced == b.voiced).all()


# ---- CPU: the marks dict and the routes ---------------------------------------------------------------------------------------------------------------

STYLES = np.zeros((2, 4), np.float32)
FAKE_HOP = 4


def _sent(tag, phones, word2ph):
    return dict(phones=list(phones), word2ph=list(word2ph), tag=float(tag))


REQUEST = [_sent(0.5, [0, 2, 0, 1, 0], [1, 0, 3, 1]), None, _sent(0.25, [0, 3, 0], [2, 1]), None]


class FakePipe:
    """Row i of a run: phones[t] + 1 frames of FAKE_HOP samples per token; a fetch with pitch answers frame f with f0 = 100 + f (every third
    frame unvoiced)."""

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
        return [np.full(int(n), u["tag"], np.float32) for n, u in zip(b.lens, b.utts)]

    def fetch_request(self, b, rows, fmt, place, joined_len, gain=None, flac=False, marks=False, env_hop=0, levels=True, pitch=None):
        self.calls.append(dict(rows=list(rows), marks=marks, pitch=None if pitch is None else (pitch.hop, pitch.f0_min, pitch.f0_max)))
        t = np.zeros(int(joined_len), np.float32)
        st, en = [], []
        for r, p in zip(rows, place):
            t[p:p + int(b.lens[r])] = b.utts[r]["tag"]
            c = p + FAKE_HOP * np.concatenate([[0], np.cumsum([int(x) + 1 for x in b.utts[r]["phones"]])])
            st, en = st + list(c[:-1]), en + list(c[1:])
        out = t.astype(fmt.dtype)
        m = model.Marks(np.array(st), np.array(en), np.zeros(len(st)), np.zeros(len(st)), 0, None, None, len(out)) if marks else None
        if pitch is None:
            return (out, None, m) if marks else (out, None)
        nf = pitch.n_frames(len(out))
        pitch.f0 = np.where(np.arange(nf) % 3 == 2, 0.0, 100.0 + np.arange(nf))
        pitch.ap, pitch.lag = np.full(nf, 0.05), np.full(nf, 100, np.int32)
        return out, None, m, pitch

    def close(self):
        pass


def test_marks_dict_token_means_edges_and_absent_keys():
    # tokens [0, 10), [10, 10), [10, 25), [25, 31), [31, 40); hop 5: centres 2, 7, 12, ..., 37
    m = model.Marks(np.array([0, 10, 10, 25, 31]), np.array([10, 10, 25, 31, 40]), np.zeros(5), np.zeros(5), 0, None, None, 40)
    utts, fmt = [_sent(1, [1, 2, 3, 4, 5], [5])], model.PcmFormat(16000, "s16")
    p = model.Pitch(5)
    p.f0 = np.array([100.0, 0.0, 110.0, 120.0, 0.0, 0.0, 0.0, 200.0])
    p.ap, p.lag = np.linspace(0.0, 0.7, 8), np.full(8, 100, np.int32)
    d = orchestrator.marks_dict(utts, [0], fmt, m, p)
    json.dumps(d)
    assert d["pitch"] == {"hop": 5, "f0_hz": [100.0, None, 110.0, 120.0, None, None, None, 200.0], "aperiodicity": list(np.linspace(0.0, 0.7, 8))}
    t = d["tokens"]
    assert t[0]["f0_hz"] == 100.0 and t[0]["voiced"] == 0.5                   # centres 2, 7; 7 is unvoiced
    assert t[1]["f0_hz"] is None and t[1]["voiced"] == 0.0                    # an empty span holds no centre
    assert t[2]["f0_hz"] == 115.0 and t[2]["voiced"] == 2 / 3                 # centres 12, 17, 22
    assert t[3]["f0_hz"] is None and t[3]["voiced"] == 0.0                    # centre 27 alone, unvoiced (32 belongs to the next span)
    assert t[4]["f0_hz"] == 200.0 and t[4]["voiced"] == 0.5                   # centres 32, 37
    # a centre exactly on a boundary belongs to the span that starts there
    m2 = model.Marks(np.array([0, 7]), np.array([7, 40]), np.zeros(2), np.zeros(2), 0, None, None, 40)
    t = orchestrator.marks_dict([_sent(1, [1, 2], [2])], [0], fmt, m2, p)["tokens"]
    assert t[0]["f0_hz"] == 100.0 and t[0]["voiced"] == 1.0 and t[1]["voiced"] == 3 / 7
    # without pitch: exactly the keys there were
    d0 = orchestrator.marks_dict(utts, [0], fmt, m)
    assert set(d0) == {"sample_rate", "tokens", "words"} and set(d0["tokens"][0]) == {"line", "index", "phone", "start", "end", "start_s", "end_s",
                                                                                      "level_dbfs", "peak"}


def test_routes_carry_or_refuse_pitch_hz():
    SO = orchestrator.SynthesizeOptions
    pipe = FakePipe()
    plain_audio, plain = orchestrator.easy_synthesize_marks(pipe, REQUEST, STYLES, noise_seed=1)
    assert pipe.calls[-1]["pitch"] is None and "pitch" not in plain and "f0_hz" not in plain["tokens"][0]
    audio, mk = orchestrator.easy_synthesize_marks(pipe, REQUEST, STYLES, noise_seed=1, options=SO(pitch_hz=900, pitch_min_hz=80.0, pitch_max_hz=500.0))
    assert audio == plain_audio and pipe.calls[-1] == dict(rows=[0, 1], marks=True, pitch=(49, 80.0, 500.0))   # hop = rate // pitch_hz, ONE fetch
    total = len(audio[audio.index(b"data") + 8:]) // 4
    assert mk["pitch"]["hop"] == 49 and len(mk["pitch"]["f0_hz"]) == len(mk["pitch"]["aperiodicity"]) == -(-total // 49)
    assert {k: v for k, v in mk.items() if k != "pitch"}.keys() == plain.keys()
    for a, b in zip(mk["tokens"], plain["tokens"]):
        assert {k: v for k, v in a.items() if k not in ("f0_hz", "voiced")} == b
    # refused before any GPU work
    runs = pipe.runs
    for bad in (SO(pitch_hz=0), SO(pitch_hz=1001), SO(pitch_hz=100.0), SO(pitch_hz=True), SO(pitch_hz=100, pitch_min_hz=39.0),
                SO(pitch_hz=100, pitch_max_hz=44100 / 4 + 1), SO(pitch_hz=100, pitch_min_hz=600.0), SO(pitch_hz=100, pitch_min_hz="70")):
        with pytest.raises(model.Sbv2Error):
            orchestrator.easy_synthesize_marks(pipe, REQUEST, STYLES, noise_seed=1, options=bad)
    with pytest.raises(model.Sbv2Error, match="/synthesize_marks"):
        orchestrator.easy_synthesize(pipe, REQUEST, STYLES, noise_seed=1, options=SO(pitch_hz=100))
    for kw in (dict(), dict(split=True), dict(levels=True)):
        with pytest.raises(model.Sbv2Error, match="/synthesize_marks"):
            orchestrator.easy_synthesize_stream(None, None, REQUEST[:1], STYLES, options=SO(pitch_hz=100), **kw)
    assert pipe.runs == runs
    # the batcher: carried with marks, refused without
    rb = batcher.RequestBatcher(pipe, start=False, clock=lambda: 0.0, max_wait_ms=1000.0)
    f0 = rb.submit(REQUEST, STYLES, options=SO(pitch_hz=900), noise_seed=1, marks=True)
    f1 = rb.submit(REQUEST, STYLES, options=SO(pitch_hz=900), noise_seed=1)
    f2 = rb.submit(REQUEST, STYLES, options=SO(pitch_hz=0), noise_seed=1, marks=True)
    rb.start()
    rb.close()
    assert f0.result(0)[1]["pitch"]["hop"] == 49
    for f in (f1, f2):
        with pytest.raises(model.Sbv2Error):
            f.result(0)
    assert "/synthesize_marks" in str(f1.exception(0))


def test_rest_models_accept_the_pitch_fields():
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient
    from sbv2_api_amd import rest
    wav = orchestrator.array_to_wav(np.zeros((1, 1, 10), np.float32))
    marks = {"sample_rate": 16000, "tokens": [], "words": [], "pitch": {"hop": 160, "f0_hz": [None], "aperiodicity": [1.0]}}

    class H:
        calls = []

        def easy_synthesize(self, ident, text, style_id, speaker_id, options):
            orchestrator.refuse_pitch(options, "easy_synthesize (/synthesize)")
            return wav

        def easy_synthesize_marks(self, ident, text, style_id, speaker_id, options):
            self.calls.append((options.pitch_hz, options.pitch_min_hz, options.pitch_max_hz))
            return wav, marks

        def easy_synthesize_stream(self, ident, text, style_id, speaker_id, options, **kw):
            orchestrator.refuse_pitch(options, "a stream (/synthesize_stream, /synthesize_stream_marks)")
            raise AssertionError("not reached in this test")

    h = H()
    c = TestClient(rest.make_app(h), raise_server_exceptions=False)
    r = c.post("/synthesize_marks", json={"text": "x", "ident": "m", "pitch_hz": 100, "pitch_min_hz": 80.0, "pitch_max_hz": 400.0})
    assert r.status_code == 200 and r.json()["marks"] == marks and base64.b64decode(r.json()["audio"]) == wav
    assert h.calls[-1] == (100, 80.0, 400.0)
    assert c.post("/synthesize_marks", json={"text": "x", "ident": "m"}).status_code == 200 and h.calls[-1] == (None, 70.0, 600.0)
    assert c.post("/synthesize", json={"text": "x", "ident": "m"}).content == wav
    for route in ("/synthesize", "/synthesize_stream", "/synthesize_stream_marks"):
        r = c.post(route, json={"text": "x", "ident": "m", "pitch_hz": 100})
        assert r.status_code == 500 and "/synthesize_marks" in r.text, (route, r.text)


# ---- GPU: the kernel, launch by launch ----------------------------------------------------------------------------------------------------------------

def hook(x, sr, hop, encoding=None, **kw):
    """sbv2_debug_pitch between guard entries -> a namespace shaped like yin_ref's."""
    x = np.ascontiguousarray(x)
    enc = model.ENCODINGS[encoding] if encoding else int(x.dtype == np.int16)
    nf = -(-x.size // hop) if x.size else 0
    q = _c_pitch(nf, hop, **kw)
    c3, voiced = np.full((nf + 2, 3), 77.0), np.full(nf + 2, 77, np.int32)
    _lib.check(_lib.lib().sbv2_debug_pitch(0, x.ctypes.data_as(C.c_void_p) if x.size else None, enc, x.size, sr, C.byref(q.c),
                                           C.cast(c3.ctypes.data + 24, f64p), C.cast(voiced.ctypes.data + 4, i32p)))
    assert q.guards() and (c3[0] == 77).all() and (c3[-1] == 77).all() and voiced[0] == 77 and voiced[-1] == 77, "guard entries"
    assert q.c.n_frames == nf
    return types.SimpleNamespace(lag=q.lag[1:-1].copy(), voiced=voiced[1:-1].copy(), c3=c3[1:-1].copy(), f0=q.f0[1:-1].copy(), ap=q.ap[1:-1].copy())


def assert_equal_bits(got, ref, what):
    assert got.lag.size == ref.lag.size, what
    np.testing.assert_array_equal(got.lag, ref.lag, err_msg=what + ": lag")
    np.testing.assert_array_equal(got.voiced, ref.voiced, err_msg=what + ": voiced")
    assert got.c3.tobytes() == ref.c3.tobytes(), (what, "c values", int((got.c3 != ref.c3).sum()), float(np.abs(got.c3 - ref.c3).max()))
    np.testing.assert_allclose(got.f0, ref.f0, rtol=1e-12, atol=0, err_msg=what + ": f0")
    np.testing.assert_allclose(got.ap, ref.ap, rtol=1e-12, atol=0, err_msg=what + ": ap")
    assert ((got.f0 == 0) == (got.voiced == 0)).all(), what


def assert_close_f32(got, ref, what):
    """The f32 rule: c within 1e-9; lag and voiced equal except on frames the reference itself calls marginal, at most 2 % of them."""
    assert got.lag.size == ref.lag.size, what
    keep = ~ref.marginal
    assert ref.marginal.sum() <= 0.02 * ref.lag.size, (what, int(ref.marginal.sum()), ref.lag.size)
    np.testing.assert_array_equal(got.lag[keep], ref.lag[keep], err_msg=what + ": lag")
    np.testing.assert_array_equal(got.voiced[keep], ref.voiced[keep], err_msg=what + ": voiced")
    err = float(np.abs(got.c3[keep] - ref.c3[keep]).max()) if keep.any() else 0.0
    print(f"[pitch] {what}: f32 c error worst {err:.3e}, {int(ref.marginal.sum())} of {ref.lag.size} frames marginal")
    assert err <= 1e-9, (what, err)
    np.testing.assert_allclose(got.f0[keep], ref.f0[keep], rtol=1e-7, atol=0, err_msg=what + ": f0")


@gpu
@pytest.mark.parametrize("encoding", ["s16", "mulaw", "alaw"])
@pytest.mark.parametrize("rate", RATES)
def test_hook_equals_the_reference_on_tones_and_noise(rate, encoding):
    x, ref = medley_ref(rate, encoding)
    got = hook(x, rate, rate // 100, None if encoding == "s16" else encoding)
    assert_equal_bits(got, ref, f"medley {rate} {encoding}")
    assert ref.voiced.any() and not ref.voiced.all()
    again = hook(x, rate, rate // 100, None if encoding == "s16" else encoding)
    assert again.c3.tobytes() == got.c3.tobytes() and again.f0.tobytes() == got.f0.tobytes()


@gpu
@pytest.mark.parametrize("encoding", ["s16", "mulaw", "alaw"])
def test_hook_equals_the_reference_on_a_glide_and_on_random_samples(encoding):
    enc = None if encoding == "s16" else encoding
    x = encoded(glide(), encoding)
    ref = yin_ref(values_of(x, enc), 16000, 160)
    assert_equal_bits(hook(x, 16000, 160, enc), ref, f"glide {encoding}")
    assert ref.voiced[12:49].all() and (np.diff(ref.f0[12:49]) > 0).all() and 110 < ref.f0[12] < 125 and 205 < ref.f0[48] < 222   # it IS a glide
    assert (ref.voiced[:9] == 0).all()                                                                                   # the noise head
    assert (ref.voiced[-8:] == 0).all() and (ref.ap[-8:] == 1.0).all()                                                   # the silent tail
    rng = np.random.default_rng(77)
    x = encoded(rng.integers(-32768, 32768, 3000).astype(np.int16), encoding)
    for hop, rng_hz in ((80, (F0_MIN, F0_MAX)), (37, (100.0, 2000.0)), (80, (40.0, 41.0))):
        ref = yin_ref(values_of(x, enc), 8000, hop, *rng_hz)
        assert_equal_bits(hook(x, 8000, hop, enc, f0_min=rng_hz[0], f0_max=rng_hz[1]), ref, f"random {encoding} hop {hop} {rng_hz}")


EDGE_SHAPES = [(0, 80), (1, 80), (114, 80), (80, 80), (81, 80), (300, 1), (300, 500), (300, 1000), (115, 80), (229, 80), (231, 7)]


@gpu
def test_hook_edge_shapes():
    """8 kHz, 70 - 600 Hz: tau_max = 115.  n = 0 (no frame, no launch), 1, tau_max - 1, hop, hop + 1 (a last frame whose centre 120 lies beyond
    n), hop = 1, a hop larger than n with its centre inside (250 < 300) and beyond it (500 > 300)."""
    assert lags_np(8000) == (13, 115)
    rng = np.random.default_rng(3)
    for n, hop in EDGE_SHAPES:
        x = rng.integers(-32768, 32768, n).astype(np.int16)
        if n == 300 and hop == 1:
            x = np.concatenate([tone(173.9, 8000)[:200], x[200:]])            # voiced and unvoiced frames, one sample apart
        ref = yin_ref(values_of(x), 8000, hop)
        assert ref.lag.size == (-(-n // hop) if n else 0)
        assert_equal_bits(hook(x, 8000, hop), ref, f"edge n = {n}, hop = {hop}")
        y = x.astype(np.float32) / np.float32(32768.0)
        assert hook(y, 8000, hop).c3.tobytes() == ref.c3.tobytes(), (n, hop)
    # refusals of the hook write nothing
    x = rng.integers(-32768, 32768, 400).astype(np.int16)
    for kw, word in BAD_PARAMETERS + [(dict(capacity=4), "too small")]:
        q = _c_pitch(5, **dict(dict(hop=80), **kw))
        c3, voiced = np.full((5, 3), 77.0), np.full(5, 77, np.int32)
        rc = _lib.lib().sbv2_debug_pitch(0, x.ctypes.data_as(C.c_void_p), 1, x.size, 8000, C.byref(q.c), c3.ctypes.data_as(f64p), voiced.ctypes.data_as(i32p))
        assert rc != 0 and word in _lib.lib().sbv2_last_error().decode(), (kw, _lib.lib().sbv2_last_error())
        assert q.untouched() and (c3 == 77).all() and (voiced == 77).all()


@gpu
def test_the_bound_case_keeps_equal_bits():
    """48 kHz, f0_min = 40: tau_max = 1200, the largest window.  A square wave of half-period 1200 between -32768 and 32767: at tau = 1200 every
    difference is 65535, d = 1200 * 65535^2 = 5.2e12 and d tau = 6.2e15, above 2^52 and below 2^53; a 32-bit sum wraps and an f64 sum of f64
    squares is exact only by luck of the order, a 64-bit integer sum is exact always."""
    sr, hop = 48000, 1200
    assert lags_np(sr, 40.0, 600.0) == (80, 1200)
    n = 4 * hop
    x = np.where((np.arange(n) // 1200) % 2 == 0, -32768, 32767).astype(np.int16)
    ref = yin_ref(values_of(x), sr, hop, 40.0, 600.0)
    assert ref.lag.size == 4
    assert 2 ** 52 < ref.max_dtau < 2 ** 53 and ref.max_S < 2 ** 53, (ref.max_dtau, ref.max_S)
    got = hook(x, sr, hop, f0_min=40.0, f0_max=600.0)
    assert_equal_bits(got, ref, "bound case")
    # ... with noise on top the sums are no longer round numbers
    y = np.clip(x.astype(np.int64) + np.random.default_rng(1).integers(-3000, 3001, n), -32768, 32767).astype(np.int16)
    ref = yin_ref(values_of(y), sr, hop, 40.0, 600.0)
    assert 2 ** 52 < ref.max_dtau < 2 ** 53 and ref.max_S < 2 ** 53
    assert_equal_bits(hook(y, sr, hop, f0_min=40.0, f0_max=600.0), ref, "bound case with noise")


@gpu
def test_f32_samples():
    for rate in (8000, 44100):      # s16 / 32768 as f32: the bits of the s16 result (one and three lags per lane)
        x, ref = medley_ref(rate, "s16")
        y = x.astype(np.float32) / np.float32(32768.0)
        assert_equal_bits(hook(y, rate, rate // 100), ref, f"scaled s16 as f32 {rate}")
    for seed in F32_SEEDS:
        x, ref = f32_case(seed)
        assert not ref.marginal.any()
        got = hook(x, 16000, 160)
        assert_close_f32(got, ref, f"gaussian f32 seed {seed}")
        assert hook(x, 16000, 160).c3.tobytes() == got.c3.tobytes()          # the order is fixed


# ---- GPU: the pipeline ----------------------------------------------------------------------------------------------------------------------------------

FORMS = [("s16", 16000, False), ("mulaw", 8000, False), ("f32", 44100, False), ("s16", 16000, True)]


@pytest.fixture(scope="module")
def two_sentences():
    """One request of two sentences as rows of one run, on the timeline easy_synthesize gives it."""
    bs, vs = model.load_model(blob("bert", "tiny", 3), True), model.load_model(blob("vits", "tiny", 5), False)
    pipe = model.Pipeline(bs, vs)
    bc, _ = weights("bert", "tiny", 3)
    vc, _ = weights("vits", "tiny", 5)
    utts = make_utts([9, 14], bc, vc, seed0=431, with_bert=False)
    b = pipe.prepare(utts, sdp_ratio=0.2, noise_scale=0.6, noise_scale_w=0.8, noise_seed=17)
    pipe.run(b)
    place, joined = orchestrator.joined_placement([int(n) for n in b.lens], [0, 1], 3)
    yield pipe, b, [0, 1], place, joined
    pipe.close(); bs.close(); vs.close()


@gpu
@pytest.mark.parametrize("gain", [None, "loudness"])
@pytest.mark.parametrize("encoding,rate,flac", FORMS, ids=["s16-16k", "mulaw-8k", "f32-44k", "flac-16k"])
def test_pipeline_pitch(two_sentences, encoding, rate, flac, gain):
    pipe, b, rows, place, joined = two_sentences
    fmt = model.PcmFormat(rate, encoding)
    g = model.Loudness(-23.0, -1.0) if gain else None
    hop = rate // 100
    kw = dict(gain=g, flac=flac, marks=True, env_hop=hop)
    plain, pstats, pm = pipe.fetch_request(b, rows, fmt, place, joined, **kw)
    plain = plain if flac else plain.copy()
    out, stats, m, p = pipe.fetch_request(b, rows, fmt, place, joined, pitch=model.Pitch(hop), **kw)
    assert (out == plain) if flac else (out.dtype == plain.dtype and out.tobytes() == plain.tobytes())
    assert (stats is None and pstats is None) or stats.tobytes() == pstats.tobytes()
    for x, y in zip(pm.arrays(), m.arrays()):
        assert x.tobytes() == y.tobytes()
    samples = np.asarray(R.read(out)["samples"], np.int16) if flac else out
    out_len = model.pcm_format_length(fmt, joined)
    assert len(samples) == out_len and len(p.f0) == len(p.ap) == len(p.lag) == -(-out_len // hop)
    enc = encoding if encoding in ("mulaw", "alaw") else None
    h = hook(samples, rate, hop, enc)                                        # the hook run on the fetched samples
    assert h.f0.tobytes() == p.f0.tobytes() and h.ap.tobytes() == p.ap.tobytes() and (h.lag == p.lag).all()
    ref = yin_ref(values_of(samples, enc), rate, hop)
    got = types.SimpleNamespace(lag=p.lag, voiced=(p.f0 > 0).astype(np.int32), c3=h.c3, f0=p.f0, ap=p.ap)
    (assert_close_f32 if encoding == "f32" else assert_equal_bits)(got, ref, f"pipeline {encoding} {rate} flac={flac} gain={gain}")
    # a fetch with pitch alone, and a second fetch of the same ticket: identical bits
    out2, stats2, m2, p2 = pipe.fetch_request(b, rows, fmt, place, joined, gain=g, flac=flac, pitch=model.Pitch(hop))
    assert m2 is None and ((out2 == plain) if flac else out2.tobytes() == plain.tobytes())
    for x, y in ((p.f0, p2.f0), (p.ap, p2.ap), (p.lag, p2.lag)):
        assert x.tobytes() == y.tobytes()
    # the timeline holds the silent gap between the sentences: unvoiced frames with c = 1
    gap = (np.arange(len(p.f0)) * hop > m.end[int(b.t_lens[0]) - 1] + 3 * ref.tau_max) & (np.arange(len(p.f0)) * hop + hop < m.start[int(b.t_lens[0])] - 3 * ref.tau_max)
    assert gap.any() and (p.f0[gap] == 0).all() and (p.ap[gap] == 1.0).all()


@gpu
def test_pipeline_pitch_refusals_leave_the_arrays_untouched(two_sentences):
    pipe, b, rows, place, joined = two_sentences
    l = _lib.lib()
    fmt = model.PcmFormat(16000, "s16")
    nf = -(-model.pcm_format_length(fmt, joined) // 160)
    rw, pl = np.asarray(rows, np.int32), np.asarray(place, np.int64)
    req = _lib.Sbv2FetchRequest(rw.ctypes.data_as(C.POINTER(C.c_int32)), len(rw), pl.ctypes.data_as(_lib.i64p), joined, C.pointer(fmt.c), None, None, 0)

    def call(q):
        dst, got = np.full(1 << 20, 77, np.uint8), C.c_int64(-5)
        rc = l.sbv2_pipeline_fetch_request_pitch(pipe.h, b.ticket, C.byref(req), dst.ctypes.data, dst.nbytes, C.byref(got), None, None, C.byref(q.c))
        return rc, l.sbv2_last_error().decode(), bool((dst == 77).all() and got.value == -5), dst, got.value

    for kw, word in BAD_PARAMETERS + [(dict(capacity=nf - 1), "pitch arrays too small"), (dict(f0_max=4000.1), "f0_max")]:
        q = _c_pitch(nf, **kw)
        rc, msg, clean, _, _ = call(q)
        assert rc != 0 and word in msg and clean and q.untouched(), (kw, rc, msg)
    q = _c_pitch(nf)
    q.c.f0 = None
    rc, msg, clean, _, _ = call(q)
    assert rc != 0 and "f0 must not be NULL" in msg and clean and q.untouched()
    q = _c_pitch(nf)                               # the ticket is still fetchable, exact capacity suffices, ap and lag may be NULL
    q.c.ap, q.c.lag = None, None
    rc, msg, _, dst, n = call(q)
    assert rc == 0, msg
    assert q.guards() and q.c.n_frames == nf and (q.ap == 77).all() and (q.lag == 77).all()
    ref, _, _, p = pipe.fetch_request(b, rows, fmt, place, joined, marks=True, pitch=model.Pitch(160))
    assert dst[:2 * n].tobytes() == ref.tobytes() and q.f0[1:-1].tobytes() == p.f0.tobytes()


@gpu
def test_batcher_and_rest_carry_the_pitch_block():
    bs, vs = model.load_model(blob("bert", "tiny", 3), True), model.load_model(blob("vits", "tiny", 5), False)
    bc, _ = weights("bert", "tiny", 3)
    vc, _ = weights("vits", "tiny", 5)
    keys = ("input_ids", "word2ph", "phones", "tones", "langs")
    sents = [{k: u[k] for k in keys} for u in make_utts([7, 12], bc, vc, seed0=151, with_bert=False)]
    sv = synth.hash_normal(77, 3 * vc["style_dim"]).reshape(3, -1).astype(np.float32) * 0.1
    opts = lambda: orchestrator.SynthesizeOptions(sample_rate=16000, encoding="s16", pitch_hz=100, envelope_hz=100)
    pipe = model.Pipeline(bs, vs)

    def check(audio, mk):
        out_len = (len(audio) - 44) // 2
        assert mk["pitch"]["hop"] == 160 and len(mk["pitch"]["f0_hz"]) == len(mk["pitch"]["aperiodicity"]) == -(-out_len // 160)
        assert all(v is None or F0_MIN * 0.99 < v < F0_MAX * 1.01 for v in mk["pitch"]["f0_hz"])
        assert all("f0_hz" in t and 0.0 <= t["voiced"] <= 1.0 for t in mk["tokens"])
        x = np.frombuffer(audio[44:], np.int16)
        ref = yin_ref(values_of(x), 16000, 160)
        assert [v is None for v in mk["pitch"]["f0_hz"]] == [v == 0 for v in ref.f0]
        np.testing.assert_allclose([v or 0.0 for v in mk["pitch"]["f0_hz"]], ref.f0, rtol=1e-12, atol=0)
        assert mk["pitch"]["aperiodicity"] == list(ref.ap)

    try:
        alone_audio, alone = orchestrator.easy_synthesize_marks(pipe, sents, sv, 1, 0, opts(), noise_seed=4242)
        check(alone_audio, alone)
        rb = batcher.RequestBatcher(pipe, start=False, max_wait_ms=1000.0)
        fut = rb.submit(sents, sv, 1, 0, opts(), noise_seed=4242, marks=True)
        rb.start()
        rb.close()
        audio, mk = fut.result(0)
        check(audio, mk)
        fastapi = pytest.importorskip("fastapi")
        from fastapi.testclient import TestClient
        from sbv2_api_amd import rest

        class H:
            def easy_synthesize_marks(self, ident, text, style_id, speaker_id, options):
                return orchestrator.easy_synthesize_marks(pipe, sents, sv, style_id, speaker_id, options, noise_seed=4242)

        c = TestClient(rest.make_app(H()), raise_server_exceptions=False)
        r = c.post("/synthesize_marks", json={"text": "x", "ident": "m", "style_id": 1, "sample_rate": 16000, "encoding": "s16", "pitch_hz": 100,
                                              "envelope_hz": 100})
        assert r.status_code == 200, r.text
        j = r.json()
        assert base64.b64decode(j["audio"]) == alone_audio and j["marks"] == json.loads(json.dumps(alone))
        check(base64.b64decode(j["audio"]), j["marks"])
    finally:
        pipe.close(); bs.close(); vs.close()
