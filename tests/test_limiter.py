"""Look-ahead true-peak limiter (csrc/limiter.hip, sbv2_pipeline_fetch_pcm_limited / _fetch_flac_limited): loudness targets that the scale-only
gain of csrc/loudness.hip misses because the true peak binds first.

The reference is a numpy / scipy restatement of the convention of include/sbv2_hip.h (sbv2_limiter) in float64, built on the meter functions
of test_loudness.py.  CPU tests run anywhere; GPU tests (@pytest.mark.gpu) need an MI355X."""
import ctypes as C
import io

import numpy as np
import pytest

import flac_reader as R
from helpers import blob, make_utts, weights
from sbv2_api_amd import _lib, model, orchestrator, synth
from test_loudness import RATES, _debug_signals, close_stats, h4, integrated, true_peak
from test_pcm_format import check_format, ref_format

TARGETS = (-23.0, -16.0, -14.0)
# max |x_device - x_numpy| / max |x_numpy| over the signals of test_debug_limiter_equals_numpy: the largest value measured on an MI355X over
# the seven rates and three limiter settings was 1.03e-13, at 48 kHz (f64 sums in different orders, and the pre-gain G_2
# carries the meter's own differences between summation orders into every sample); asserted with a margin of 10x.
X_REL_TOL = 1.03e-12


# ---- the numpy reference ------------------------------------------------------------------------------------------------------------------

def envelope(y):
    """e[n] = max |z[4 n + d]|, d in -3..3, z the true-peak meter's 4x interpolation (0 outside the signal)."""
    import scipy.signal as S
    n = y.size
    z = np.abs(S.resample_poly(y, 4, 1, window=h4() / 4))
    zp = np.concatenate([np.zeros(3), z, np.zeros(3)])
    e = np.zeros(n)
    for d in range(7):
        e = np.maximum(e, zp[d:d + 4 * n:4])
    return e


def hann(K):
    h = np.sin(np.pi * (np.arange(K) + 0.5) / K) ** 2
    return h / h.sum()


def sliding_min_ahead(r, K):
    """m[n] = min r[n .. n + K - 1], r = 1 past the end."""
    from scipy.ndimage import minimum_filter1d
    rp = np.concatenate([r, np.ones(K - 1)])
    return minimum_filter1d(rp, size=K, mode="constant", cval=1.0)[K // 2:K // 2 + r.size]   # centred window: [i - K // 2, i - K // 2 + K)


def gain_curve(e, g0, c, K):
    """(r, s, s_sum) of step 2: s_sum the plain sum, s with the rounding guard s <= r."""
    with np.errstate(divide="ignore"):
        r = np.minimum(1.0, c / (g0 * e))
    m = sliding_min_ahead(r, K)
    s = np.convolve(np.concatenate([np.full(K - 1, m[0]), m]), hann(K), mode="valid")   # s[n] = sum_k h[k] m[n - k], m = m[0] before the start
    return r, np.minimum(s, r), s


def limit(y, rate, target, ceiling=-1.0, D=6.0):
    """The convention on one float64 signal: (x, stats[6], detail).  detail: idle, and of the last evaluation when active r, s, the
    unguarded sum s_sum and x_sum = y g0 s_sum (what the convention gives before its two rounding guards)."""
    y = np.asarray(y, np.float64)
    L, tp = integrated(y, rate), true_peak(y)
    if not np.isfinite(L) or min(target - L, ceiling - tp + D) <= ceiling - tp:   # idle: the scale-only gain of sbv2_loudness
        G = min(target - L, ceiling - tp) if np.isfinite(L) else 0.0
        x = y * 10 ** (G / 20)
        return x, np.array([L, tp, G, integrated(x, rate), true_peak(x), 0.0]), {"idle": True}
    K, c, cap = rate // 100, 10 ** (ceiling / 20), ceiling - tp + D
    e = envelope(y)
    G = min(target - L, cap)
    for i in range(3):
        g0 = 10 ** (G / 20)
        r, s, s_sum = gain_curve(e, g0, c, K)
        x = np.clip(y * g0 * s, -c, c)
        Lx = integrated(x, rate)
        if i < 2 and np.isfinite(Lx):
            G = min(G + target - Lx, cap)
    return x, np.array([L, tp, G, Lx, true_peak(x), 20 * np.log10(s.min())]), {"idle": False, "r": r, "s": s, "s_sum": s_sum, "x_sum": y * g0 * s_sum}


def quantise(x, encoding):
    return np.clip(np.rint(np.asarray(x, np.float64) * 32767.0), -32767, 32767) if encoding == "s16" else np.asarray(x, np.float64)


def speech_like(rate, sec=6.0):
    """Harmonic voiced segments under a syllable envelope with pauses, plus short noise bursts: a peak-to-loudness ratio above 20 dB."""
    rng = np.random.default_rng(rate)   # fixed seed per rate
    t = np.arange(int(sec * rate)) / rate
    f0 = 120 * (1 + 0.1 * np.sin(2 * np.pi * 0.7 * t))
    ph = 2 * np.pi * np.cumsum(f0) / rate
    nh = min(30, int(rate / 2 / 140))
    v = sum(np.cos(k * ph + rng.uniform(0, 2 * np.pi)) / (1 + (k * 120 / 700.) ** 2) for k in range(1, nh))
    am = np.clip(np.sin(2 * np.pi * 3.1 * t), 0, None) ** 2 * (np.sin(2 * np.pi * 0.45 * t) > -0.6) * (0.6 + 0.4 * np.sin(2 * np.pi * 0.23 * t))
    x = v * am
    x /= np.sqrt(np.mean(x ** 2))
    for a in rng.uniform(0.2, sec - 0.2, 6):
        i, n = int(a * rate), int(0.004 * rate)
        x[i:i + n] += 4 * rng.standard_normal(n) * np.hanning(n)
    return 0.05 * x


# ---- CPU ----------------------------------------------------------------------------------------------------------------------------------

def test_sliding_min_and_envelope_helpers():
    rng = np.random.default_rng(3)
    for K in (2, 5, 80, 441):
        r = rng.uniform(0.1, 1.0, 1000)
        rp = np.concatenate([r, np.ones(K - 1)])
        want = np.lib.stride_tricks.sliding_window_view(rp, K).min(axis=1)
        np.testing.assert_array_equal(sliding_min_ahead(r, K), want)
    y = rng.standard_normal(500)
    e = envelope(y)
    assert (e >= np.abs(y) * (1 - 1e-15)).all() and abs(20 * np.log10(e.max()) - true_peak(y)) < 1e-12   # z[4 n] is y[n] within rounding
    assert abs(hann(441).sum() - 1) < 1e-15 and hann(80).size == 80


@pytest.mark.parametrize("rate", RATES)
def test_numpy_limiter_bounds_and_reach(rate):
    y = speech_like(rate)
    ceiling, D = -1.0, 6.0
    c = 10 ** (ceiling / 20)
    L, tp = integrated(y, rate), true_peak(y)
    assert tp - L > 20, (rate, L, tp)   # the premise: speech-like peak-to-loudness ratio
    for target in TARGETS:
        x, st, det = limit(y, rate, target, ceiling, D)
        scale_only = L + min(target - L, ceiling - tp)
        print(f"{rate} target {target}: L {L:.3f} TP {tp:.3f} scale-only {scale_only:.3f} G {st[2]:.3f} L_out {st[3]:.4f} "
              f"TP_out - ceiling {st[4] - ceiling:.2e} depth {st[5]:.3f}")
        assert np.abs(x).max() <= c, (rate, target)
        assert st[4] <= ceiling + 1e-3, (rate, target, st)
        peak_bound = target - L > ceiling - tp
        assert det["idle"] == (not peak_bound)
        if not peak_bound:
            assert abs(st[3] - target) <= 0.01 and st[5] == 0.0
            continue
        _check_unguarded(det, c, (rate, target))
        assert (det["s"] <= det["r"]).all()
        assert det["s"].min() >= 10 ** (-D / 20) * (1 - 1e-12), (rate, target, st)
        assert st[5] <= 0 and st[3] > scale_only, (rate, target, st)
        if st[2] < ceiling - tp + D:   # Gcap does not bind: the target is met
            assert abs(st[3] - target) <= 0.01, (rate, target, st)


EPS = 8 * np.finfo(np.float64).eps   # the taps sum to 1 within an ulp or two, the products round once each


def _check_unguarded(det, c, what):
    """The bounds are properties of the curve, not of the guards: the plain sum and the unclamped product keep them up to rounding, at
    every sample, so the guards (min with r, clamp to +-c) move nothing by more than that."""
    assert (det["s_sum"] <= det["r"] * (1 + EPS)).all(), what
    assert np.abs(det["x_sum"]).max() <= c * (1 + EPS), what
    assert np.abs(det["s"] - det["s_sum"]).max() <= EPS, what


def test_numpy_limiter_loud_onset_keeps_the_bound_without_the_guards():
    """A signal that is above the ceiling from its first sample, and one with a peak inside the first window: the gain starts at the first
    window's minimum and moves smoothly; nothing is left to the guards, and there is no step between neighbouring samples."""
    rate, ceiling, D = 16000, -1.0, 6.0
    K, c = rate // 100, 10 ** (ceiling / 20)
    rng = np.random.default_rng(11)
    for onset in (5, K // 2, K - 2):
        y = 0.03 * rng.standard_normal(2 * rate)
        y[:onset] = -0.9   # loud at n = 0 .. onset - 1
        y[rate] = 0.7
        x, st, det = limit(y, rate, -14.0, ceiling, D)
        assert not det["idle"] and st[5] < 0
        _check_unguarded(det, c, onset)
        assert np.abs(x).max() <= c
        s = det["s"]
        assert s[0] == det["r"][:K].min() or abs(s[0] - det["r"][:K].min()) <= EPS   # starts at the first window's gain, not at 1
        step = np.abs(np.diff(20 * np.log10(s))).max()
        print(f"onset {onset}: s[0] {s[0]:.4f} min r[0:K] {det['r'][:K].min():.4f} largest step {step:.4f} dB per sample")
        # s moves by at most (1 - 10^(-D / 20)) max h = (1 - 10^(-D / 20)) 2 / K per sample, from a level of at least 10^(-D / 20)
        assert step <= 20 * np.log10(1 + (10 ** (D / 20) - 1) * 2 / K) * (1 + 1e-9)
    # the rule that was not chosen, m = 1 before the start: the sum ignores r over the first K - 1 samples
    r = np.ones(1000)
    r[:5] = 0.5
    m = sliding_min_ahead(r, K)
    s1 = np.convolve(np.concatenate([np.ones(K - 1), m]), hann(K), mode="valid")
    assert s1[0] > 0.999 and (s1[:5] > r[:5] * 1.9).all()


def test_numpy_limiter_idle_and_degenerate_cases():
    rate = 16000
    y = speech_like(rate, 3.0)
    L, tp = integrated(y, rate), true_peak(y)
    for target, D in ((-40.0, 6.0), (-14.0, 0.0)):
        x, st, det = limit(y, rate, target, -1.0, D)
        G = min(target - L, -1.0 - tp)
        assert det["idle"] and st[2] == G and st[5] == 0.0
        np.testing.assert_array_equal(x, y * 10 ** (G / 20))
    for y in (np.zeros(0), np.zeros(5000)):
        x, st, det = limit(y, rate, -16.0)
        assert det["idle"] and st[0] == -np.inf and st[2] == 0.0 and x.size == y.size


def test_options_rest_and_limiter_carry_the_new_fields():
    d = orchestrator.SynthesizeOptions()
    assert (d.limiter, d.max_reduction, d.loudness, d.true_peak_max, d.normalize) == (False, 6.0, None, -1.0, False)
    o = orchestrator.SynthesizeOptions(loudness=-16, limiter=True, max_reduction=3.0)
    assert (o.loudness, o.limiter, o.max_reduction) == (-16, True, 3.0)
    with pytest.raises(model.Sbv2Error, match="loudness"):
        orchestrator.SynthesizeOptions(limiter=True)
    with pytest.raises(model.Sbv2Error, match="normalize"):
        orchestrator.SynthesizeOptions(normalize=True, loudness=-16, limiter=True)
    lim = model.Limiter(-16)
    assert (lim.target_lufs, lim.true_peak_max, lim.max_reduction) == (-16.0, -1.0, 6.0)
    assert (lim.c.target_lufs, lim.c.true_peak_max_dbtp, lim.c.max_reduction_db, lim.c.reserved) == (-16.0, -1.0, 6.0, 0.0)
    for bad in ((-80, -1, 6), (-3, -1, 6), (-16, 0.5, 6), (-16, -25, 6), (-16, -1, -0.1), (-16, -1, 12.5), (float("nan"), -1, 6),
                (-16, -1, float("inf"))):
        with pytest.raises(model.Sbv2Error, match="outside"):
            model.Limiter(*bad)
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient
    from sbv2_api_amd import rest

    class Holder:
        def __init__(self):
            self.opts = []

        def models(self):
            return ["m"]

        def easy_synthesize(self, ident, text, style_id, speaker_id, options):
            self.opts.append(options)
            return b"RIFF"

    h = Holder()
    c = TestClient(rest.make_app(h))
    assert c.post("/synthesize", json={"text": "a", "ident": "m"}).status_code == 200
    o = h.opts[-1]
    assert (o.limiter, o.max_reduction, o.loudness, o.true_peak_max, o.normalize, o.sample_rate, o.encoding) == \
        (False, 6.0, None, -1.0, False, 44100, "f32")
    r = c.post("/synthesize", json={"text": "a", "ident": "m", "loudness": -16, "limiter": True, "max_reduction": 4, "encoding": "s16"})
    assert r.status_code == 200
    assert (h.opts[-1].loudness, h.opts[-1].limiter, h.opts[-1].max_reduction) == (-16, True, 4)
    n = len(h.opts)
    r = c.post("/synthesize", json={"text": "a", "ident": "m", "limiter": True})
    assert r.status_code == 500 and r.text.startswith("Something went wrong: ") and "loudness" in r.text
    assert len(h.opts) == n


def test_lib_binds_the_limiter_entry_points():
    assert C.sizeof(_lib.Sbv2Limiter) == 32
    assert [(n, t) for n, t in _lib.Sbv2Limiter._fields_] == [("target_lufs", C.c_double), ("true_peak_max_dbtp", C.c_double),
                                                            ("max_reduction_db", C.c_double), ("reserved", C.c_double)]
    assert [getattr(_lib.Sbv2Limiter, n).offset for n, _ in _lib.Sbv2Limiter._fields_] == [0, 8, 16, 24]
    l = _lib.lib()
    for name in ("sbv2_pipeline_fetch_pcm_limited", "sbv2_pipeline_fetch_flac_limited", "sbv2_debug_limiter"):
        assert name in _lib.SYMBOLS and getattr(l, name).restype is C.c_int
    assert _lib.SYMBOLS["sbv2_pipeline_fetch_pcm_limited"][1][3] == C.POINTER(_lib.Sbv2Limiter)


# ---- GPU: the limiter on host signals -----------------------------------------------------------------------------------------------------

def _limiter_signals(rate):
    K = rate // 100
    rng = np.random.default_rng(rate + 1)
    sigs = [speech_like(rate)] + _debug_signals(rate)
    short = 0.02 * rng.standard_normal(K - 7)   # shorter than the look-ahead window, with one peak
    short[K // 3] = 0.8
    sigs.append(short)
    a, b = 0.03 * rng.standard_normal(rate), 0.03 * rng.standard_normal(rate)   # loud at the shared edge: a window must not cross it
    a[-5:] = 0.9
    b[:5] = -0.9
    sigs += [a, b]
    return sigs


@pytest.mark.gpu
@pytest.mark.parametrize("rate", RATES)
def test_debug_limiter_equals_numpy(rate):
    sigs = _limiter_signals(rate)
    worst, active = 0.0, 0
    for lim in (model.Limiter(-16.0, -1.0, 6.0), model.Limiter(-14.0, -2.0, 12.0), model.Limiter(-30.0, -1.0, 6.0)):
        ref = [limit(y, rate, lim.target_lufs, lim.true_peak_max, lim.max_reduction) for y in sigs]
        got, stats = model.debug_limiter(sigs, rate, lim)
        assert stats.shape == (len(sigs), 6) and len(got) == len(sigs)
        close_stats(stats, np.array([r[1] for r in ref]), what=f"{rate} {lim}")
        c = 10 ** (lim.true_peak_max / 20)
        for i, (g, (x, st, det)) in enumerate(zip(got, ref)):
            assert g.shape == x.shape
            if not x.size:
                continue
            assert np.abs(g).max() <= c or det["idle"], (rate, lim, i)
            scale = np.abs(x).max()
            if scale > 0:
                worst = max(worst, float(np.abs(g - x).max() / scale))
            else:
                assert not g.any()
            if det["idle"]:
                assert stats[i, 5] == 0.0
            else:
                active += 1
                assert stats[i, 5] < 0.0
    print(f"{rate}: x max-abs error {worst:.3e} of the peak over {active} active signal evaluations")
    assert active >= 8   # the speech-like one, the noise lengths, the short one and the edge pair, at two settings
    assert worst <= X_REL_TOL, (rate, worst)
    l = _lib.lib()
    out, st, lens = np.zeros(8), np.zeros(6), np.array([8], np.int64)
    for bad in (_lib.Sbv2Limiter(-80.0, -1.0, 6.0, 0.0), _lib.Sbv2Limiter(-16.0, 1.0, 6.0, 0.0), _lib.Sbv2Limiter(-16.0, -1.0, 13.0, 0.0),
                _lib.Sbv2Limiter(-16.0, -1.0, float("nan"), 0.0)):
        rc = l.sbv2_debug_limiter(0, out.ctypes.data, lens.ctypes.data_as(_lib.i64p), 1, rate, bad, out.ctypes.data, st.ctypes.data_as(C.POINTER(C.c_double)))
        assert rc != 0 and b"outside" in l.sbv2_last_error()
    rc = l.sbv2_debug_limiter(0, out.ctypes.data, lens.ctypes.data_as(_lib.i64p), 1, rate, _lib.Sbv2Limiter(-16.0, -1.0, 6.0, 1.0), out.ctypes.data,
                              st.ctypes.data_as(C.POINTER(C.c_double)))
    assert rc != 0 and b"reserved" in l.sbv2_last_error()


# ---- GPU: the pipeline --------------------------------------------------------------------------------------------------------------------

def _tiny():
    bc, _ = weights("bert", "tiny", 3)
    vc, _ = weights("vits", "tiny", 5)
    bs, vs = model.load_model(blob("bert", "tiny", 3), True), model.load_model(blob("vits", "tiny", 5), False)
    return bc, vc, bs, vs


def _tiny_run(pipe, bc, vc):
    utts = make_utts([9, 1, 23, 14, 40], bc, vc, seed0=501, with_bert=False)
    b = pipe.prepare(utts, forced=True)
    pipe.run(b)
    native = pipe.fetch(b)
    place, pos = [], 0
    for x in native:
        place.append(pos)
        pos += len(x) + orchestrator.SENTENCE_GAP
    joined = pos - orchestrator.SENTENCE_GAP
    timeline = np.zeros(joined, np.float32)
    for p, x in zip(place, native):
        timeline[p:p + len(x)] = x
    return b, native, place, joined, timeline


def _active_target(signals, rate, ceiling=-1.0):
    """A target 3 dB above what the plain scale reaches on the signal with the smallest peak-to-loudness ratio, from the numpy meter
    alone: every signal with a finite loudness is peak-bound, so the limiter cannot be idle."""
    plr = [true_peak(y) - integrated(y, rate) for y in signals if np.isfinite(integrated(y, rate))]
    return min(-5.0, ceiling - min(plr) + 3.0)


def _check_limited(got, stats, y, rate, enc, lim, what):
    x, ref, det = limit(y, rate, lim.target_lufs, lim.true_peak_max, lim.max_reduction)
    close_stats(stats, ref, what=what)
    check_format(got, quantise(x, enc), enc, what)
    if enc == "s16" and got.size:
        assert np.abs(got.astype(np.int64)).max() <= np.rint(10 ** (lim.true_peak_max / 20) * 32767), what
    return det


@pytest.mark.gpu
def test_fetch_limited_every_rate_encoding_layout():
    bc, vc, bs, vs = _tiny()
    pipe = model.Pipeline(bs, vs)
    b, native, place, joined, timeline = _tiny_run(pipe, bc, vc)
    for rate in RATES:
        ys = [ref_format(x, rate, "f32", False) for x in native]
        yj = ref_format(timeline, rate, "f32", False)
        lim = model.Limiter(_active_target(ys + [yj], rate), -1.0, 6.0)
        for enc in ("f32", "s16"):
            f = model.PcmFormat(rate, enc)
            got, stats = pipe.fetch_limited(b, f, lim)
            assert len(got) == len(native) and stats.shape == (len(native), 6)
            for i, (g, y) in enumerate(zip(got, ys)):
                assert g.dtype == f.dtype
                det = _check_limited(g, stats[i], y, rate, enc, lim, f"{f} {lim} utterance {i}")
                assert not det["idle"] and stats[i, 5] < 0, (rate, enc, i, stats[i])
            gj, sj = pipe.fetch_limited(b, f, lim, place, joined)
            assert len(gj) == 1
            det = _check_limited(gj[0], sj[0], yj, rate, enc, lim, f"{f} {lim} joined")
            assert not det["idle"] and sj[0, 5] < 0, (rate, enc, sj)
            # two fetches of one run: identical bytes and stats
            again, stats2 = pipe.fetch_limited(b, f, lim)
            assert np.concatenate(again).tobytes() == np.concatenate(got).tobytes() and stats2.tobytes() == stats.tobytes(), f
            aj, sj2 = pipe.fetch_limited(b, f, lim, place, joined)
            assert aj[0].tobytes() == gj[0].tobytes() and sj2.tobytes() == sj.tobytes(), f
    with pytest.raises(model.Sbv2Error, match="normali"):
        pipe.fetch_limited(b, model.PcmFormat(16000, "s16", True), model.Limiter(-16.0))
    with pytest.raises(model.Sbv2Error, match="Limiter"):
        pipe.fetch_limited(b, model.PcmFormat(16000, "s16"), None)
    l = _lib.lib()
    f = model.PcmFormat(16000, "s16")
    dst = np.zeros(1 << 20, np.int16)
    outs = np.zeros(len(native), np.int64)
    rc = l.sbv2_pipeline_fetch_pcm_limited(pipe.h, b.ticket, f.c, None, None, 0, dst.ctypes.data, dst.nbytes, outs.ctypes.data_as(_lib.i64p), None)
    assert rc != 0 and b"limiter" in l.sbv2_last_error()
    pipe.close(); bs.close(); vs.close()


@pytest.mark.gpu
def test_idle_limiter_returns_the_bytes_of_the_loudness_fetch():
    bc, vc, bs, vs = _tiny()
    pipe = model.Pipeline(bs, vs)
    b, native, place, joined, _ = _tiny_run(pipe, bc, vc)
    for rate in RATES:
        for enc in ("f32", "s16"):
            f = model.PcmFormat(rate, enc)
            for target, D in ((-45.0, 6.0), (-8.0, 0.0)):   # a quiet target the scale reaches; a loud one with no depth allowed
                ln, lim = model.Loudness(target, -1.0), model.Limiter(target, -1.0, D)
                for pl, jl in ((None, None), (place, joined)):
                    want, ws = pipe.fetch_loudness(b, f, ln, pl, jl)
                    got, gs = pipe.fetch_limited(b, f, lim, pl, jl)
                    assert np.concatenate(got).tobytes() == np.concatenate(want).tobytes(), (f, target, D, pl is None)
                    assert gs[:, :3].tobytes() == ws.tobytes() and (gs[:, 5] == 0).all(), (f, target, D)
                    if target == -45.0:
                        assert (np.abs(gs[:, 2] - (target - gs[:, 0]))[np.isfinite(gs[:, 0])] < 1e-9).all()   # the scale was not peak-bound
                    if enc == "s16":
                        wf, _ = pipe.fetch_flac_loudness(b, f, ln, pl, jl)
                        gf, gfs = pipe.fetch_flac_limited(b, f, lim, pl, jl)
                        assert gf == wf and gfs.tobytes() == gs.tobytes(), (f, target, D)
    pipe.close(); bs.close(); vs.close()


@pytest.mark.gpu
def test_fetch_flac_limited_decodes_to_the_s16_signals():
    bc, vc, bs, vs = _tiny()
    pipe = model.Pipeline(bs, vs)
    b, native, place, joined, timeline = _tiny_run(pipe, bc, vc)
    for rate in (16000, 44100, 48000):
        f = model.PcmFormat(rate, "s16")
        lim = model.Limiter(_active_target([ref_format(x, rate, "f32", False) for x in native], rate), -1.0, 6.0)
        for pl, jl in ((None, None), (place, joined)):
            pcm, s1 = pipe.fetch_limited(b, f, lim, pl, jl)
            streams, s2 = pipe.fetch_flac_limited(b, f, lim, pl, jl)
            assert s1.tobytes() == s2.tobytes() and (s1[:, 5] < 0).any()
            assert len(streams) == len(pcm)
            for st, x in zip(streams, pcm):
                d = R.read(st)
                assert d["rate"] == rate
                np.testing.assert_array_equal(d["samples"], x)
            again, s3 = pipe.fetch_flac_limited(b, f, lim, pl, jl)
            assert again == streams and s3.tobytes() == s2.tobytes()
    with pytest.raises(model.Sbv2Error, match="s16"):
        pipe.fetch_flac_limited(b, model.PcmFormat(16000, "f32"), model.Limiter(-16.0))
    pipe.close(); bs.close(); vs.close()


@pytest.mark.gpu
def test_easy_synthesize_limiter_wav_and_flac():
    import scipy.io.wavfile as W
    bc, vc, bs, vs = _tiny()
    pipe = model.Pipeline(bs, vs)
    keys = ("input_ids", "word2ph", "phones", "tones", "langs")
    sent = [{k: synth.make_utterance(n, bc, vc, seed=710 + n)[k] for k in keys} for n in (11, 6, 17)]
    lines = [sent[0], None, sent[1], sent[2]]
    styles = synth.hash_normal(77, 3 * vc["style_dim"]).reshape(3, -1).astype(np.float32)
    for sr, enc in ((44100, "s16"), (16000, "f32"), (48000, "flac")):
        base, st0, st = orchestrator.SynthesizeOptions(sample_rate=sr, encoding=enc, loudness=-16), [], []
        orchestrator.easy_synthesize(pipe, lines, styles, 1, 0, base, noise_seed=4321, loudness_stats=st0)
        opts = orchestrator.SynthesizeOptions(sample_rate=sr, encoding=enc, loudness=-16, limiter=True)
        data = orchestrator.easy_synthesize(pipe, lines, styles, 1, 0, opts, noise_seed=4321, loudness_stats=st)
        if enc == "flac":
            d = R.read(data)
            got_rate, sig = d["rate"], d["samples"].astype(np.float64) / 32767
        else:
            got_rate, s = W.read(io.BytesIO(data))
            sig = s.astype(np.float64) / (32767 if enc == "s16" else 1)
        assert got_rate == sr and len(st0) == 1 and len(st0[0]) == 3 and len(st) == 1 and len(st[0]) == 6
        L, tp, G = st0[0]
        assert st[0][:2] == [L, tp]
        c = 10 ** (-1 / 20)   # f32: the cast's rounding; s16 / FLAC: no sample beyond rint(c 32767)
        assert np.abs(sig).max() <= (c * (1 + 1e-7) if enc == "f32" else np.rint(c * 32767) / 32767), (sr, enc)
        assert abs(integrated(sig, sr) - st[0][3]) <= 0.01, (sr, enc, st)
        if -16 - L > -1 - tp:   # the first fetch was peak-bound: the limiter delivers more than the scale's L + G
            assert st[0][3] > L + G and st[0][5] < 0, (sr, enc, st0, st)
        else:
            assert st[0][2] == G and st[0][5] == 0
        # a second request 3 dB beyond what the scale reaches on this signal (from the stats of the first): the limiter is active
        loud = min(-5.0, -1.0 - (tp - L) + 3.0)
        sa = []
        opts = orchestrator.SynthesizeOptions(sample_rate=sr, encoding=enc, loudness=loud, limiter=True)
        data = orchestrator.easy_synthesize(pipe, lines, styles, 1, 0, opts, noise_seed=4321, loudness_stats=sa)
        sig = R.read(data)["samples"].astype(np.float64) / 32767 if enc == "flac" else \
            W.read(io.BytesIO(data))[1].astype(np.float64) / (32767 if enc == "s16" else 1)
        assert loud - L > -1 - tp and len(sa[0]) == 6 and sa[0][5] < 0, (sr, enc, loud, sa)
        assert sa[0][3] > L + (-1 - tp) and abs(integrated(sig, sr) - sa[0][3]) <= 0.01, (sr, enc, loud, sa)
        assert np.abs(sig).max() <= (c * (1 + 1e-7) if enc == "f32" else np.rint(c * 32767) / 32767), (sr, enc)
    opts = orchestrator.SynthesizeOptions(loudness=-16, limiter=True)
    opts.loudness = None   # set after construction: easy_synthesize refuses the pair itself
    with pytest.raises(model.Sbv2Error, match="loudness"):
        orchestrator.easy_synthesize(pipe, lines, styles, 1, 0, opts, noise_seed=1)
    pipe.close(); bs.close(); vs.close()


@pytest.fixture(scope="module")
def full_models():
    bs, vs = model.load_model(blob("bert", "full"), True), model.load_model(blob("vits", "full"), False)
    yield weights("bert", "full")[0], weights("vits", "full")[0], bs, vs
    bs.close(); vs.close()


@pytest.mark.gpu
def test_full_shape_batch_limited_44k_16k_s16(full_models):
    """The bench-shaped batch (32 x 128 phonemes, 10.4 s each at full model size) through the limiter, s16, against the reference."""
    bc, vc, bs, vs = full_models
    pipe = model.Pipeline(bs, vs)
    utts = [synth.make_utterance(128, bc, vc, seed=i) for i in range(32)]
    b = pipe.prepare(utts, forced=True)
    pipe.run(b)
    native = pipe.fetch(b)
    for rate in (44100, 16000):
        f = model.PcmFormat(rate, "s16")
        ys = {i: ref_format(native[i], rate, "f32", False) for i in (0, 7, 31)}
        lim = model.Limiter(_active_target(list(ys.values()), rate), -1.0, 6.0)
        got, stats = pipe.fetch_limited(b, f, lim)
        for i, y in ys.items():
            det = _check_limited(got[i], stats[i], y, rate, "s16", lim, f"{rate} {lim} utterance {i}")
            L, tp = stats[i, 0], stats[i, 1]
            print(f"{rate} utterance {i}: target {lim.target_lufs:.2f} L {L:.2f} TP {tp:.2f} PLR {tp - L:.2f} scale-only "
                  f"{L + min(lim.target_lufs - L, -1 - tp):.2f} limited {stats[i, 3]:.2f} TP_out {stats[i, 4]:.4f} depth {stats[i, 5]:.2f}")
            assert not det["idle"] and stats[i, 5] < 0 and stats[i, 3] > L + min(lim.target_lufs - L, -1 - tp), stats[i]
            sig = got[i].astype(np.float64) / 32767
            assert abs(integrated(sig, rate) - stats[i, 3]) <= 0.01, (rate, i, stats[i])
        assert all(g.size == model.pcm_format_length(f, x.size) for g, x in zip(got, native))
    pipe.close()
