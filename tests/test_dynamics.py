"""Speech compressor in front of the loudness stage (csrc/dynamics.hip, sbv2_pipeline_fetch_request_dynamics, sbv2_debug_dynamics): it evens
out syllables and sentences so that the look-ahead limiter behind it is left with the crest only.

The reference is a numpy restatement of the convention of include/sbv2_hip.h (sbv2_dynamics) in float64 and int64, built on the meter and
limiter functions of test_loudness.py / test_limiter.py.  CPU tests run anywhere; GPU tests (@pytest.mark.gpu) need an MI355X."""
import ctypes as C
import math
import types

import numpy as np
import pytest

import flac_reader as R
from sbv2_api_amd import _lib, model, orchestrator
from test_limiter import X_REL_TOL, _check_limited, _tiny, _tiny_run, envelope, hann, limit, quantise, speech_like
from test_loudness import close_stats, integrated, meter, true_peak
from test_pcm_format import check_format, ref_format

gpu = pytest.mark.gpu
USUAL = (8.0, 4.0, 600.0, 60.0)   # threshold_lu, ratio, attack and release in dB/s


# ---- the numpy reference ------------------------------------------------------------------------------------------------------------------

def rates_q(rate, attack, release):
    """(rho, alpha): release and attack per sample in units of 1 / 65536 dB."""
    return max(1, int(np.rint(release * 65536.0 / rate))), max(1, int(np.rint(attack * 65536.0 / rate)))


def static_curve(e, T, ratio):
    """dq[n] = llrint(65536 d[n]), d = k (20 log10 e - T) where e > 0 and that is > 0, else 0."""
    k = 1.0 - 1.0 / ratio
    with np.errstate(divide="ignore", invalid="ignore"):
        d = k * (20.0 * np.log10(e) - T)
    d = np.where((e > 0) & (d > 0), d, 0.0)
    return np.rint(d * 65536.0).astype(np.int64)


def ballistics_seq(dq, rho, alpha):
    """u by the sequential recurrences p[n] = max(dq[n], p[n - 1] - rho), a[n] = max(dq[n], a[n + 1] - alpha)."""
    n = len(dq)
    p, a = [0] * n, [0] * n
    for i in range(n):
        p[i] = int(dq[i]) if i == 0 else max(int(dq[i]), p[i - 1] - rho)
    for i in range(n - 1, -1, -1):
        a[i] = int(dq[i]) if i == n - 1 else max(int(dq[i]), a[i + 1] - alpha)
    return np.maximum(np.array(p, np.int64), np.array(a, np.int64)).reshape(n)


def ballistics_scan(dq, rho, alpha):
    """u by the two maximum scans: prefixmax(dq[i] + rho i) - rho n and suffixmax(dq[i] - alpha i) + alpha n."""
    dq = np.asarray(dq, np.int64)
    i = np.arange(dq.size, dtype=np.int64)
    p = np.maximum.accumulate(dq + rho * i) - rho * i
    a = np.maximum.accumulate((dq - alpha * i)[::-1])[::-1] + alpha * i
    return np.maximum(p, a)


def taps_libm(K):
    """The window as the library's host code forms it: libm's sin, the sum in ascending k.  (hann(K) sums pairwise and may differ by an ulp.)"""
    h = [math.sin(math.pi * (k + 0.5) / K) ** 2 for k in range(K)]
    s = 0.0
    for v in h:
        s += v
    return np.array([v / s for v in h])


def smooth(u, K, h=None):
    """ut[n] = sum_{k < K} h[k] double(u[clamp(n + c0 - k, 0, N - 1)]) / 65536 in ascending k, c0 = K - 1 - K // 2, never contracted."""
    h = hann(K) if h is None else h
    n = u.size
    U = u.astype(np.float64) / 65536.0
    Up = np.concatenate([np.full(K // 2, U[0]), U, np.full(K - 1 - K // 2, U[-1])])   # Up[j] = U[clamp(j - K // 2)]
    acc = np.zeros(n)
    for k in range(K):
        acc = acc + h[k] * Up[K - 1 - k:K - 1 - k + n]
    return acc


def compress(y, rate, threshold=8.0, ratio=4.0, attack=600.0, release=60.0, h=None):
    """The convention on one float64 signal: (yc, stats[3], detail)."""
    y = np.asarray(y, np.float64)
    L = integrated(y, rate)
    T = L + threshold
    if y.size == 0 or not np.isfinite(L) or ratio == 1:
        return y.copy(), np.array([L, T, 0.0]), {"idle": True, "s": np.ones(y.size)}
    rho, alpha = rates_q(rate, attack, release)
    e = envelope(y)
    dq = static_curve(e, T, ratio)
    u = ballistics_scan(dq, rho, alpha)
    ut = smooth(u, rate // 100, h)
    s = 10 ** (-ut / 20)
    return y * s, np.array([L, T, -ut.max()]), {"idle": False, "e": e, "dq": dq, "u": u, "ut": ut, "s": s}


# ---- CPU ----------------------------------------------------------------------------------------------------------------------------------

def test_sequential_recurrences_equal_the_scan_forms():
    rng = np.random.default_rng(5)
    for n in (1, 2, 1000):
        for rho in (1, 7, 8192):
            for alpha in (1, 7, 8192):
                dq = rng.integers(0, 40 * 65536, n) * (rng.random(n) < 0.05)   # sparse peaks of up to 40 dB over zeros
                np.testing.assert_array_equal(ballistics_scan(dq, rho, alpha), ballistics_seq(dq, rho, alpha))
                dense = rng.integers(0, 3 * rho + 3, n)                        # neighbours within reach of one step
                np.testing.assert_array_equal(ballistics_scan(dense, rho, alpha), ballistics_seq(dense, rho, alpha))
    assert rates_q(8000, 10, 1) == (8, 82) and rates_q(48000, 10, 1) == (1, 14) and rates_q(44100, 600, 60) == (89, 892)
    assert abs(taps_libm(441).sum() - 1) < 1e-15 and np.abs(taps_libm(80) - hann(80)).max() < 1e-17


def test_identity_and_silence_return_the_signal_bit_for_bit():
    rate = 16000
    y = speech_like(rate, 2.0)
    for sig, kw in ((y, {"ratio": 1.0}), (np.zeros(5000), {}), (np.zeros(0), {})):
        yc, st, det = compress(sig, rate, **kw)
        assert det["idle"] and st[2] == 0.0 and yc.tobytes() == np.asarray(sig, np.float64).tobytes()
    # the curve itself at ratio 1 (what the kernels compute, which never take the shortcut): d = 0 throughout, s = 1
    dq = static_curve(envelope(y), integrated(y, rate) + 8.0, 1.0)
    assert not dq.any() and (10 ** (-smooth(ballistics_scan(dq, 5, 50), rate // 100) / 20) == 1.0).all()


def test_gain_never_exceeds_one():
    for rate in (8000, 44100):
        y = speech_like(rate, 3.0)
        for args in (USUAL, (0.0, 20.0, 10000.0, 1000.0), (3.0, 2.0, 10.0, 1.0)):
            yc, st, det = compress(y, rate, *args)
            s = det["s"]
            assert not det["idle"] and (s > 0).all() and (s <= 1.0).all() and s.min() < 1.0, (rate, args)
            assert (np.abs(yc) <= np.abs(y)).all() and st[2] < 0 and st[1] == st[0] + args[0]


@pytest.mark.parametrize("rate", (8000, 16000, 44100, 48000))
def test_compressor_brings_the_limiter_nearer_the_target(rate):
    y = speech_like(rate)
    yc, st, det = compress(y, rate, *USUAL)
    alone = limit(y, rate, -16.0, -1.0, 6.0)[1]
    both = limit(yc, rate, -16.0, -1.0, 6.0)[1]
    plr = [true_peak(v) - integrated(v, rate) for v in (y, yc)]
    gain = abs(alone[3] + 16.0) - abs(both[3] + 16.0)
    print(f"{rate}: L_out limiter alone {alone[3]:.2f}, compressor + limiter {both[3]:.2f} ({gain:.2f} LU nearer -16); limiter depth "
          f"{alone[5]:.1f} -> {both[5]:.1f}; deepest compression {st[2]:.2f} dB; PLR {plr[0]:.1f} -> {plr[1]:.1f}")
    assert gain > 1.0, (rate, alone, both)


def test_options_model_and_rest_carry_the_compressor():
    d = model.Dynamics()
    assert (d.threshold_lu, d.ratio, d.attack, d.release) == USUAL and not d.is_identity() and model.Dynamics(ratio=1).is_identity()
    assert (d.c.threshold_lu, d.c.ratio, d.c.attack_db_per_s, d.c.release_db_per_s, d.c.reserved) == USUAL + (0.0,)
    nan, inf = float("nan"), float("inf")
    for bad in ((-0.1, 4, 600, 60), (30.5, 4, 600, 60), (8, 0.9, 600, 60), (8, 20.5, 600, 60), (8, 4, 9, 60), (8, 4, 10001, 60), (8, 4, 600, 0.5),
                (8, 4, 600, 1001), (nan, 4, 600, 60), (8, nan, 600, 60), (8, 4, inf, 60), (8, 4, 600, nan), (8, 0, 600, 60)):
        with pytest.raises(model.Sbv2Error, match="outside"):
            model.Dynamics(*bad)
    SO = orchestrator.SynthesizeOptions
    o = SO()
    assert (o.compressor, o.comp_threshold, o.comp_ratio, o.comp_attack, o.comp_release) == (False,) + USUAL
    assert orchestrator.dynamics_options(o) is None
    o = SO(loudness=-16, limiter=True, compressor=True, comp_ratio=3.0)
    assert o.compressor and orchestrator.dynamics_options(o).ratio == 3.0
    with pytest.raises(model.Sbv2Error, match="loudness"):
        SO(compressor=True)
    with pytest.raises(model.Sbv2Error, match="outside"):
        SO(loudness=-16, compressor=True, comp_ratio=25.0)
    with pytest.raises(model.Sbv2Error, match="true or false"):
        SO(loudness=-16, compressor=1)
    with pytest.raises(model.Sbv2Error, match="number"):
        SO(loudness=-16, compressor=True, comp_attack="fast")
    # a plan carries it; options changed after construction are refused by the plan itself
    sent = [{"input_ids": [1], "word2ph": [1], "phones": [1], "tones": [0], "langs": [0]}]
    styles = np.zeros((2, 4), np.float32)
    plan = orchestrator.RequestPlan(sent, styles, 0, 0, SO(loudness=-16, compressor=True))
    assert isinstance(plan.dynamics, model.Dynamics) and isinstance(plan.gain, model.Loudness)
    assert orchestrator.RequestPlan(sent, styles, 0, 0, SO(loudness=-16)).dynamics is None
    o = SO(loudness=-16, compressor=True)
    o.loudness = None
    with pytest.raises(model.Sbv2Error, match="loudness"):
        orchestrator.RequestPlan(sent, styles, 0, 0, o)
    # a stream refuses it before anything is touched, and says why
    with pytest.raises(model.Sbv2Error, match="whole signal's loudness.*looks ahead"):
        orchestrator.easy_synthesize_stream(None, None, sent, styles, options=SO(loudness=-16, compressor=True))
    assert orchestrator.dynamics_dict([-30.0, -22.0, -4.5]) == {"loudness_lufs": -30.0, "threshold_lufs": -22.0, "deepest_db": -4.5}
    assert orchestrator.dynamics_dict([-np.inf, -np.inf, 0.0]) == {"loudness_lufs": None, "threshold_lufs": None, "deepest_db": 0.0}


class FakePipe:
    """One row per sentence, 100 samples each; fetch_request records its keywords and answers as model.Pipeline does."""

    def __init__(self):
        self.calls = []

    def prepare(self, utts, **kw):
        return types.SimpleNamespace(lens=np.full(len(utts), 100, np.int64), t_lens=np.array([len(u["phones"]) for u in utts]), ticket=1)

    def run(self, b):
        pass

    def fetch_request(self, b, rows, fmt, place, joined_len, gain=None, flac=False, marks=False, env_hop=0, levels=True, pitch=None, **kw):
        self.calls.append(dict(kw, gain=gain, marks=marks))
        n = model.pcm_format_length(fmt, joined_len)
        out = [np.zeros(n, fmt.dtype), np.zeros(6 if isinstance(gain, model.Limiter) else 3) if gain is not None else None]
        if marks:
            ntok = int(sum(b.t_lens[r] for r in rows))
            out.append(model.Marks(np.zeros(ntok, np.int64), np.zeros(ntok, np.int64), np.zeros(ntok), np.zeros(ntok), 0, None, None, n))
        if "dynamics" in kw:
            out.append(None if kw["dynamics"].is_identity() else np.array([-30.0, -22.0, -4.5]))
        return tuple(out)


def test_finish_request_names_the_compressor_only_when_asked_for():
    sent = [{"input_ids": [1, 2], "word2ph": [1, 1], "phones": [1, 2], "tones": [0, 0], "langs": [0, 0]}]
    styles = np.zeros((2, 4), np.float32)
    SO = orchestrator.SynthesizeOptions
    pipe = FakePipe()
    ds, ls = [], []
    wav = orchestrator.easy_synthesize(pipe, sent, styles, options=SO(loudness=-16, limiter=True, compressor=True, encoding="s16"), noise_seed=1,
                                       loudness_stats=ls, dynamics_stats=ds)
    assert wav[:4] == b"RIFF" and ds == [[-30.0, -22.0, -4.5]] and len(ls[0]) == 6
    assert isinstance(pipe.calls[-1]["dynamics"], model.Dynamics) and isinstance(pipe.calls[-1]["gain"], model.Limiter)
    orchestrator.easy_synthesize(pipe, sent, styles, options=SO(loudness=-16, encoding="s16"), noise_seed=1)
    assert "dynamics" not in pipe.calls[-1]                                    # a request without it is the call it always was
    _, marks = orchestrator.easy_synthesize_marks(pipe, sent, styles, options=SO(loudness=-16, compressor=True), noise_seed=1)
    assert marks["dynamics"] == {"loudness_lufs": -30.0, "threshold_lufs": -22.0, "deepest_db": -4.5} and pipe.calls[-1]["marks"]
    _, marks = orchestrator.easy_synthesize_marks(pipe, sent, styles, options=SO(loudness=-16), noise_seed=1)
    assert "dynamics" not in marks and "dynamics" not in pipe.calls[-1]
    _, marks = orchestrator.easy_synthesize_marks(pipe, sent, styles, options=SO(loudness=-16, compressor=True, comp_ratio=1.0), noise_seed=1)
    assert "dynamics" not in marks                                             # ratio 1: the stage did not run, there are no stats


def test_rest_takes_the_fields_and_streams_answer_400():
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient
    from sbv2_api_amd import rest

    class Holder:
        def __init__(self):
            self.opts, self.streams = [], 0

        def models(self):
            return ["m"]

        def easy_synthesize(self, ident, text, style_id, speaker_id, options):
            self.opts.append(options)
            return b"RIFF"

        def easy_synthesize_marks(self, ident, text, style_id, speaker_id, options):
            self.opts.append(options)
            return b"RIFF", {"sample_rate": 44100, "tokens": [], "words": [], "dynamics": orchestrator.dynamics_dict([-30.0, -22.0, -4.5])}

        def easy_synthesize_stream(self, *a, **kw):
            self.streams += 1
            raise AssertionError("a refused request must not reach the holder")

    h = Holder()
    c = TestClient(rest.make_app(h))
    assert c.post("/synthesize", json={"text": "a", "ident": "m"}).status_code == 200
    o = h.opts[-1]
    assert (o.compressor, o.comp_threshold, o.comp_ratio, o.comp_attack, o.comp_release) == (False,) + USUAL
    body = {"text": "a", "ident": "m", "loudness": -16, "limiter": True, "compressor": True, "comp_threshold": 6, "comp_ratio": 3, "comp_attack": 500,
            "comp_release": 50}
    assert c.post("/synthesize", json=body).status_code == 200
    o = h.opts[-1]
    assert (o.compressor, o.comp_threshold, o.comp_ratio, o.comp_attack, o.comp_release, o.limiter, o.loudness) == (True, 6, 3, 500, 50, True, -16)
    r = c.post("/synthesize_marks", json=body)
    assert r.status_code == 200 and r.json()["marks"]["dynamics"]["deepest_db"] == -4.5 and h.opts[-1].compressor
    n = len(h.opts)
    r = c.post("/synthesize", json={"text": "a", "ident": "m", "compressor": True})
    assert r.status_code == 500 and r.text.startswith("Something went wrong: ") and "loudness" in r.text and len(h.opts) == n
    r = c.post("/synthesize", json=dict(body, comp_ratio=40))
    assert r.status_code == 500 and "outside" in r.text and len(h.opts) == n
    for route in ("/synthesize_stream", "/synthesize_stream_marks"):
        r = c.post(route, json={"text": "a", "ident": "m", "compressor": True})
        assert r.status_code == 400 and "whole signal's loudness" in r.text and "looks ahead" in r.text, r.text
    assert h.streams == 0


def _c_dyn(threshold=8.0, ratio=4.0, attack=600.0, release=60.0, reserved=0.0):
    return _lib.Sbv2Dynamics(threshold, ratio, attack, release, reserved)


def test_lib_binds_the_compressor_and_refuses_what_needs_no_run():
    assert C.sizeof(_lib.Sbv2Dynamics) == 40
    assert [(n, t) for n, t in _lib.Sbv2Dynamics._fields_] == [("threshold_lu", C.c_double), ("ratio", C.c_double), ("attack_db_per_s", C.c_double),
                                                             ("release_db_per_s", C.c_double), ("reserved", C.c_double)]
    l = _lib.lib()
    for name in ("sbv2_pipeline_fetch_request_dynamics", "sbv2_debug_dynamics"):
        assert name in _lib.SYMBOLS and getattr(l, name).restype is C.c_int
    assert _lib.SYMBOLS["sbv2_pipeline_fetch_request_dynamics"][1][5] == C.POINTER(_lib.Sbv2Dynamics)
    assert model.dynamics_tile() == l.sbv2_dynamics_tile() and model.dynamics_tile() >= 64
    f = model.PcmFormat(16000, "s16")
    ln, lim = model.Loudness(-23.0), model.Limiter(-16.0)
    rows, place = np.array([0], np.int32), np.array([0], np.int64)
    dst, got, st, dst3 = np.full(16, 77, np.uint8), C.c_int64(-5), np.full(6, 7.0), np.full(3, 7.0)
    req = lambda fmt, a=None, b=None: _lib.Sbv2FetchRequest(rows.ctypes.data_as(C.POINTER(C.c_int32)), 1, place.ctypes.data_as(_lib.i64p), 10,
                                                            C.pointer(fmt.c), C.pointer(a.c) if a else None, C.pointer(b.c) if b else None, 0)
    f64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    call = lambda r, d: l.sbv2_pipeline_fetch_request_dynamics(None, 1, C.byref(r), None, None, C.byref(d) if d is not None else None,
                                                               dst.ctypes.data, dst.nbytes, C.byref(got), f64(st), f64(dst3), None, None)
    nan = float("nan")
    for d, r, word in ((_c_dyn(threshold=31.0), req(f, ln), "outside [0, 30]"), (_c_dyn(ratio=0.5), req(f, ln), "outside [1, 20]"),
                       (_c_dyn(attack=5.0), req(f, ln), "outside [10, 10000]"), (_c_dyn(release=2000.0), req(f, ln), "outside [1, 1000]"),
                       (_c_dyn(ratio=nan), req(f, ln), "outside"), (_c_dyn(threshold=nan), req(f, None, lim), "outside"),
                       (_c_dyn(ratio=1.0, release=nan), req(f, ln), "outside"), (_c_dyn(reserved=1.0), req(f, ln), "reserved"),
                       (_c_dyn(), req(f), "loudness target or a limiter"),
                       (_c_dyn(), req(f, ln, lim), "not both"), (_c_dyn(), req(f, ln), "bad arguments"), (None, req(f, ln), "bad arguments"),
                       (_c_dyn(ratio=1.0), req(f), "bad arguments")):
        assert call(r, d) != 0
        assert word in l.sbv2_last_error().decode(), (word, l.sbv2_last_error())
        assert (dst == 77).all() and got.value == -5 and (st == 7.0).all() and (dst3 == 7.0).all()
    # the hook refuses the same fields
    x, lens, out = np.zeros(8), np.array([8], np.int64), np.zeros(3)
    hook = lambda d: l.sbv2_debug_dynamics(0, x.ctypes.data, lens.ctypes.data_as(_lib.i64p), 1, 16000, d, None, None, None, None, None, f64(out))
    assert hook(_c_dyn(ratio=21.0)) != 0 and b"outside" in l.sbv2_last_error()
    assert hook(_c_dyn(reserved=2.0)) != 0 and b"reserved" in l.sbv2_last_error()
    assert hook(None) != 0 and b"dynamics" in l.sbv2_last_error()


# ---- GPU: the compressor on host signals --------------------------------------------------------------------------------------------------

def _hook_signals(rate):
    """The lengths around the window and the tile; low-level noise, the two longest with a full-scale sample in their first tile and one at
    their last sample; an all-zero signal; and the leak pair: a signal that ends in a full-scale sample, directly followed by zeros and
    noise at -60 dB."""
    tile, K = model.dynamics_tile(), rate // 100
    rng = np.random.default_rng(rate + 7)
    lens = (1, K - 1, K, K + 1, tile - 1, tile, tile + 1, 2 * tile + 3, 5 * tile + 17)
    sigs = [0.01 * rng.standard_normal(n) for n in lens]
    for y in sigs[-2:]:
        y[tile // 3] = 1.0
        y[-1] = -1.0
    sigs.append(np.zeros(2 * tile + 5))
    a = 0.01 * rng.standard_normal(3 * tile + 11)
    a[-1] = 1.0
    b = np.concatenate([np.zeros(tile // 2), 0.001 * rng.standard_normal(3 * tile)])
    return sigs + [a, b], len(sigs) - 1, len(sigs) + 1   # the signals, the all-zero one, the follower


def _check_hook(sigs, rate, dyn, exact_taps):
    parts, stats = model.debug_dynamics(sigs, rate, dyn)
    K = rate // 100
    rho, alpha = rates_q(rate, dyn.attack, dyn.release)
    assert stats.shape == (len(sigs), 3) and len(parts) == len(sigs)
    flips = total = 0
    worst_e = worst_s = worst_y = 0.0
    for i, (y, p) in enumerate(zip(sigs, parts)):
        what = f"{rate} {dyn} signal {i} ({y.size} samples)"
        L = stats[i, 0]
        close_stats(stats[i, :1], np.array([integrated(y, rate)]), what=what)
        assert stats[i, 1] == L + dyn.threshold_lu, what
        assert p.y.shape == y.shape and p.u.dtype == np.int64
        idle = not np.isfinite(L) or dyn.ratio == 1.0
        e = envelope(y)
        if e.max() > 0:
            worst_e = max(worst_e, float(np.abs(p.e - e).max() / e.max()))
        else:
            assert not p.e.any(), what
        # the static curve on the device's own envelope and L: a 1 - 2 ulp log10 may flip a rounding, by one unit
        want = np.zeros(y.size, np.int64) if idle else static_curve(p.e, L + dyn.threshold_lu, dyn.ratio)
        d = np.abs(p.dq - want)
        assert d.max() <= 1, (what, int(d.max()))
        flips += int((d > 0).sum())
        total += y.size
        # the ballistics on the device's own dq: exact
        np.testing.assert_array_equal(p.u, ballistics_seq(p.dq, rho, alpha), err_msg=what)
        # smoothing, 10^x and the multiply on the device's own u
        ut = smooth(p.u, K)
        s = 10 ** (-ut / 20)
        assert (p.s > 0).all() and (p.s <= 1.0).all(), what
        worst_s = max(worst_s, float(np.abs(p.s - s).max() / s.max()))
        if np.abs(y).max() > 0:
            worst_y = max(worst_y, float(np.abs(p.y - y * s).max() / np.abs(y * s).max()))
        deepest = -smooth(p.u, K, exact_taps).max()
        print(f"{what}: L {L:.3f} deepest {stats[i, 2]:.6f} dB (restated {deepest:.6f}, diff {stats[i, 2] - deepest:.3e}) idle {idle}")
        assert stats[i, 2] == deepest, what
        assert stats[i, 2] <= 0 and (stats[i, 2] < 0) == bool(p.u.any()), what
        if idle or not p.u.any():
            assert p.y.tobytes() == y.tobytes() and (p.s == 1.0).all(), what
    print(f"{rate} {dyn}: e {worst_e:.2e}, s {worst_s:.2e}, yc {worst_y:.2e} of the peak; dq off by one unit in {flips} of {total} samples")
    assert flips <= 1e-4 * total, (flips, total)
    assert worst_e <= X_REL_TOL and worst_s <= X_REL_TOL and worst_y <= X_REL_TOL, (worst_e, worst_s, worst_y)
    return parts, stats


@gpu
@pytest.mark.parametrize("rate", (8000, 44100))
def test_debug_dynamics_equals_numpy(rate):
    tile, K = model.dynamics_tile(), rate // 100
    sigs, zero, follower = _hook_signals(rate)
    taps = taps_libm(K)
    slow = model.Dynamics(8.0, 4.0, 10.0, 1.0)   # the release tail and the attack ramp cross every tile edge of the long signals
    parts, stats = _check_hook(sigs, rate, slow, taps)
    rho, alpha = rates_q(rate, slow.attack, slow.release)
    long = parts[8]
    first, last = tile // 3, sigs[8].size - 1
    assert long.dq[first] > 3 * tile * rho and long.dq[last] > 3 * tile * alpha                  # both reach across three tiles and more
    n = np.arange(first + 1, last)                                              # between the two: the tail or the ramp, whichever is higher
    ramp = long.dq[last] - alpha * (last - n)
    assert (long.u[n] == np.maximum(long.dq[first] - rho * (n - first), ramp)).all()
    lead = parts[follower - 1]                                                  # no tail in front of this one: the attack ramp itself
    last = lead.u.size - 1
    assert lead.dq[last] > 3 * tile * alpha
    assert (lead.u[last - 3 * tile - 1:last] == lead.dq[last] - alpha * np.arange(3 * tile + 1, 0, -1)).all()
    assert stats[8, 2] < -3.0 and np.isfinite(stats[8, 0])
    # the all-zero signal is idle and comes back bit for bit; the follower's curve is its own (the full-scale sample before it ends a signal)
    assert stats[zero, 0] == -np.inf and stats[zero, 2] == 0 and not parts[zero].u.any() and not parts[zero].y.any()
    # (a leaked release tail would start at lead.dq[-1] - rho and fall by rho a sample: the follower stays far below it throughout)
    assert lead.dq[-1] > 10 * 65536 and parts[follower].u.max() < lead.dq[-1] - rho * parts[follower].u.size - 5 * 65536
    np.testing.assert_array_equal(parts[follower].u, ballistics_seq(parts[follower].dq, rho, alpha))
    alone, _ = model.debug_dynamics([sigs[follower]], rate, slow)
    assert alone[0].u.tobytes() == parts[follower].u.tobytes() and alone[0].y.tobytes() == parts[follower].y.tobytes()
    # the usual values
    parts, stats = _check_hook(sigs, rate, model.Dynamics(), taps)
    assert stats[8, 2] < 0 and parts[8].y.tobytes() != sigs[8].tobytes()
    # ratio 1 inside the same mixed call, through the kernels: every signal comes back bit for bit
    parts, stats = _check_hook(sigs, rate, model.Dynamics(ratio=1.0), taps)
    for y, p in zip(sigs, parts):
        assert p.y.tobytes() == y.tobytes() and not p.dq.any() and not p.u.any()
    assert (stats[:, 2] == 0).all()


# ---- GPU: the pipeline --------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tiny_run():
    bc, vc, bs, vs = _tiny()
    pipe = model.Pipeline(bs, vs)
    b, native, place, joined, timeline = _tiny_run(pipe, bc, vc)
    rows = list(range(len(native)))
    y = {rate: ref_format(timeline, rate, "f32", False) for rate in (16000, 44100)}
    yc = {rate: compress(v, rate, *USUAL) for rate, v in y.items()}   # computed once, shared, never changed
    yield types.SimpleNamespace(pipe=pipe, b=b, native=native, rows=rows, place=place, joined=joined, timeline=timeline, y=y, yc=yc)
    pipe.close(); bs.close(); vs.close()


@gpu
def test_no_dynamics_and_ratio_one_are_the_fetch_without(tiny_run):
    c = tiny_run
    pipe, b = c.pipe, c.b
    for fmt, gain, flac in ((model.PcmFormat(), None, False), (model.PcmFormat(44100, "f32"), model.Loudness(-23.0), False),
                            (model.PcmFormat(16000, "s16"), model.Limiter(-16.0), False), (model.PcmFormat(8000, "mulaw"), model.Loudness(-23.0), False),
                            (model.PcmFormat(16000, "s16"), model.Limiter(-16.0), True)):
        want, ws = pipe.fetch_request(b, c.rows, fmt, c.place, c.joined, gain=gain, flac=flac)
        want = want if flac else want.copy()
        got, gs, ds = pipe.fetch_request(b, c.rows, fmt, c.place, c.joined, gain=gain, flac=flac, dynamics=model.Dynamics(ratio=1.0))
        assert ds is None and (got if flac else got.tobytes()) == (want if flac else want.tobytes()), (fmt, gain, flac)
        assert (gs is None and ws is None) or gs.tobytes() == ws.tobytes()
        # dynamics = NULL through the new entry point itself
        rw, pl = np.asarray(c.rows, np.int32), np.asarray(c.place, np.int64)
        limited = isinstance(gain, model.Limiter)
        req = _lib.Sbv2FetchRequest(rw.ctypes.data_as(C.POINTER(C.c_int32)), rw.size, pl.ctypes.data_as(_lib.i64p), c.joined, C.pointer(fmt.c),
                                    C.pointer(gain.c) if gain is not None and not limited else None, C.pointer(gain.c) if limited else None, int(flac))
        dst = np.zeros(max(len(want), 1) * (1 if flac else want.itemsize) + 64, np.uint8)
        n, st, d3 = C.c_int64(0), np.zeros(6), np.full(3, 7.0)
        _lib.check(_lib.lib().sbv2_pipeline_fetch_request_dynamics(pipe.h, b.ticket, C.byref(req), None, None, None, dst.ctypes.data, dst.nbytes, C.byref(n),
                                                                   st.ctypes.data_as(C.POINTER(C.c_double)), d3.ctypes.data_as(C.POINTER(C.c_double)),
                                                                   None, None))
        nbytes = n.value * (1 if flac else want.itemsize)
        assert dst[:nbytes].tobytes() == (want if flac else want.tobytes()) and (d3 == 7.0).all()
        if ws is not None:
            assert st[:ws.size].tobytes() == ws.tobytes()


@gpu
@pytest.mark.parametrize("rate", (16000, 44100))
def test_compressed_fetch_is_the_stage_behind_on_the_restated_yc(tiny_run, rate):
    c = tiny_run
    pipe, b = c.pipe, c.b
    y, (yc, dref, det) = c.y[rate], c.yc[rate]
    assert not det["idle"] and dref[2] < 0, dref
    f = model.PcmFormat(rate, "s16")
    dyn, lim, ln = model.Dynamics(), model.Limiter(-16.0), model.Loudness(-23.0)
    # the limiter behind the compressor
    got, st, ds = pipe.fetch_request(b, c.rows, f, c.place, c.joined, gain=lim, dynamics=dyn)
    got = got.copy()
    print(f"{rate}: compressor stats {ds} (restated {dref}); limiter stats {st}")
    close_stats(ds, dref, what=f"{rate} compressor stats")
    _check_limited(got, st, yc, rate, "s16", lim, f"{rate} compressor + {lim}")
    plain, pst = pipe.fetch_request(b, c.rows, f, c.place, c.joined, gain=lim)
    assert plain.tobytes() != got.tobytes() and pst[0] == ds[0]             # L of y is what the plain fetch measures
    # two fetches are identical; the run's PCM was only read
    again, st2, ds2 = pipe.fetch_request(b, c.rows, f, c.place, c.joined, gain=lim, dynamics=dyn)
    assert again.tobytes() == got.tobytes() and st2.tobytes() == st.tobytes() and ds2.tobytes() == ds.tobytes()
    assert [x.tobytes() for x in pipe.fetch(b)] == [x.tobytes() for x in c.native]
    # the FLAC sink decodes to the s16 fetch's integers
    fl, fst, fds = pipe.fetch_request(b, c.rows, f, c.place, c.joined, gain=lim, flac=True, dynamics=dyn)
    d = R.read(fl)
    assert d["rate"] == rate and np.asarray(d["samples"], np.int16).tobytes() == got.tobytes()
    assert fst.tobytes() == st.tobytes() and fds.tobytes() == ds.tobytes()
    # the loudness gain behind the compressor: the meter and the scale on yc
    got, st, ds = pipe.fetch_request(b, c.rows, f, c.place, c.joined, gain=ln, dynamics=dyn)
    ref = meter(yc, rate, ln.target_lufs, ln.true_peak_max)
    close_stats(st, ref, what=f"{rate} compressor + {ln}")
    close_stats(ds, dref, what=f"{rate} compressor stats")
    check_format(got, quantise(yc * 10 ** (ref[2] / 20), "s16"), "s16", f"{rate} compressor + {ln}")
    # the marks' levels are those of the delivered samples, their spans those of the fetch without
    hop = rate // 100
    out, mst, m, mds = pipe.fetch_request(b, c.rows, f, c.place, c.joined, gain=ln, marks=True, env_hop=hop, dynamics=dyn)
    _, _, pm = pipe.fetch_request(b, c.rows, f, c.place, c.joined, gain=ln, marks=True, env_hop=hop)
    assert out.tobytes() == got.tobytes() and mst.tobytes() == st.tobytes() and mds.tobytes() == ds.tobytes()
    assert m.start.tobytes() == pm.start.tobytes() and m.end.tobytes() == pm.end.tobytes()
    ss, pk = model.debug_segment_levels(out, m.start, m.end)
    assert ss.tobytes() == m.sumsq.tobytes() and pk.tobytes() == m.peak.tobytes() and ss.tobytes() != pm.sumsq.tobytes()
    nenv = len(m.env_sumsq)
    es, ep = model.debug_segment_levels(out, np.arange(nenv) * hop, np.minimum((np.arange(nenv) + 1) * hop, len(out)))
    assert es.tobytes() == m.env_sumsq.tobytes() and ep.tobytes() == m.env_peak.tobytes()
    # pitch rides along: the contour of the delivered, compressed samples
    out, _, _, p, _ = pipe.fetch_request(b, c.rows, f, c.place, c.joined, gain=ln, marks=True, pitch=model.Pitch(hop), dynamics=dyn)
    h, _, _ = model.debug_pitch(out, rate, model.Pitch(hop))
    assert out.tobytes() == got.tobytes() and h.f0.tobytes() == p.f0.tobytes()


@gpu
def test_voice_and_compressor_together(tiny_run):
    c = tiny_run
    pipe, b = c.pipe, c.b
    f0 = model.PcmFormat()
    v, dyn, ln = model.Voice(1.3, 0.8), model.Dynamics(), model.Loudness(-23.0)
    y = pipe.fetch_request(b, c.rows, f0, c.place, c.joined, voice=v)[0].astype(np.float64)   # the identity format exposes y itself
    yc, dref, det = compress(y, 44100, *USUAL)
    ref = meter(yc, 44100, ln.target_lufs, ln.true_peak_max)
    got, st, ds = pipe.fetch_request(b, c.rows, f0, c.place, c.joined, gain=ln, voice=v, dynamics=dyn)
    print(f"voice + compressor: stats {ds} (restated {dref}); loudness {st} (restated {ref})")
    close_stats(ds, dref, what="voice + compressor")
    close_stats(st, ref, what="voice + compressor, loudness")
    assert not det["idle"] and ds[2] < 0
    check_format(got, yc * 10 ** (ref[2] / 20), "f32", "voice + compressor")


@gpu
def test_refusals_through_the_handle_write_nothing(tiny_run):
    c = tiny_run
    pipe, b = c.pipe, c.b
    l = _lib.lib()
    f, fn = model.PcmFormat(16000, "s16"), model.PcmFormat(16000, "s16", True)
    ln, lim = model.Loudness(-23.0), model.Limiter(-16.0)
    rw, pl = np.asarray(c.rows, np.int32), np.asarray(c.place, np.int64)
    dst, got, st, d3 = np.full(1 << 20, 77, np.uint8), C.c_int64(-5), np.full(6, 7.0), np.full(3, 7.0)
    f64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    req = lambda fmt, a=None, bb=None, joined=c.joined: _lib.Sbv2FetchRequest(
        rw.ctypes.data_as(C.POINTER(C.c_int32)), rw.size, pl.ctypes.data_as(_lib.i64p), joined, C.pointer(fmt.c), C.pointer(a.c) if a else None,
        C.pointer(bb.c) if bb else None, 0)
    call = lambda r, d, ticket=b.ticket, cap=dst.nbytes: l.sbv2_pipeline_fetch_request_dynamics(
        pipe.h, ticket, C.byref(r), None, None, C.byref(d), dst.ctypes.data, cap, C.byref(got), f64(st), f64(d3), None, None)
    nan = float("nan")
    for d, r, kw, word in ((_c_dyn(), req(f), {}, "loudness target or a limiter"), (_c_dyn(), req(fn, ln), {}, "normalize"),
                           (_c_dyn(ratio=30.0), req(f, ln), {}, "outside [1, 20]"), (_c_dyn(attack=nan), req(f, None, lim), {}, "outside"),
                           (_c_dyn(threshold=-1.0), req(f, ln), {}, "outside [0, 30]"), (_c_dyn(release=0.0), req(f, ln), {}, "outside [1, 1000]"),
                           (_c_dyn(reserved=0.5), req(f, ln), {}, "reserved"), (_c_dyn(), req(f, ln, lim), {}, "not both"),
                           (_c_dyn(), req(f, ln), {"ticket": b.ticket + 5}, "ticket"), (_c_dyn(), req(f, ln), {"cap": 16}, "too small"),
                           (_c_dyn(), req(f, ln, joined=10), {}, "outside the joined timeline")):
        assert call(r, d, **kw) != 0
        assert word in l.sbv2_last_error().decode(), (word, l.sbv2_last_error())
        assert (dst == 77).all() and got.value == -5 and (st == 7.0).all() and (d3 == 7.0).all(), word
    with pytest.raises(model.Sbv2Error, match="loudness target or a limiter"):
        pipe.fetch_request(b, c.rows, f, c.place, c.joined, dynamics=model.Dynamics())
    # the ticket is still fetchable
    out, st2, ds = pipe.fetch_request(b, c.rows, f, c.place, c.joined, gain=ln, dynamics=model.Dynamics())
    assert out.size == model.pcm_format_length(f, c.joined) and ds[2] < 0
