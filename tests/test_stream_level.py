"""Level control on streams (csrc/limiter.hip StreamLimiter, sbv2_stream_begin_level / _next_level, POST /synthesize_stream gain_db): step 2
of the limiter's convention (include/sbv2_hip.h, sbv2_limiter) at a gain the caller fixes, in one shot and fed piece by piece with an O(K)
tail carried on the device.  The one-shot path is checked against the numpy restatement of test_limiter.py; the fed path against the
one-shot path, bit for bit, for any way of cutting the signal.  CPU tests run anywhere; GPU tests (@pytest.mark.gpu) need an MI355X."""
import ctypes as C
import io

import numpy as np
import pytest

import flac_reader as R
from helpers import blob, make_utts, weights
from sbv2_api_amd import _lib, model, orchestrator, synth
from test_limiter import X_REL_TOL, envelope, gain_curve

RATES = (8000, 16000, 22050, 24000, 32000, 44100, 48000)
NEW_SYMBOLS = ("sbv2_stream_level_lookahead", "sbv2_stream_level_bound", "sbv2_stream_begin_level", "sbv2_stream_next_level",
               "sbv2_stream_level_stats", "sbv2_debug_limiter_fixed", "sbv2_debug_limiter_stream")
# The level stream limits y in f64; the yardstick of the pipeline tests limits the f64 of the f32-FORMATTED stream, i.e. y rounded to f32.
# The only difference is that rounding: relative 2^-24 per sample of y, carried through e, r, s and the product, then the f32 cast of x.
# Largest deviation of an f32 delivery measured on an MI355X over the resampled cases below: 1.192e-07 of full scale (two f32 steps below
# 1) on the tiny model at 48 kHz, 5.960e-08 on the full model at 16 kHz; asserted with a margin of 8x, and never looser
# than one s16 step.  An s16 delivery may differ by the one quantiser step that such a deviation can flip (measured: 1 in both cases),
# never by more.
F32_ROUNDING_DEV = 1.192e-07
S16_STEP = 1


def A_of(rate):
    return rate // 100 + 11


def fixed_ref(y, rate, gain_db, ceiling=-1.0):
    """(x, s) of step 2 at g0 = 10^(gain_db / 20) in numpy: no make-up loop, no idle rule."""
    y = np.asarray(y, np.float64)
    if y.size == 0:
        return y.copy(), np.ones(0)
    K, c, g0 = rate // 100, 10 ** (ceiling / 20), 10 ** (gain_db / 20)
    _, s, _ = gain_curve(envelope(y), g0, c, K)
    return np.clip(y * g0 * s, -c, c), s


def delivery(sizes, A):
    """What each push of `sizes` samples emits: max(0, S - A) after S samples in all, the last push the rest."""
    fed = np.cumsum(sizes)
    upto = np.maximum(0, fed - A)
    upto[-1] = fed[-1]
    return list(np.diff(np.concatenate([[0], upto])))


# ---- CPU ----------------------------------------------------------------------------------------------------------------------------------

def test_abi_exports_the_level_symbols():
    l = _lib.lib()
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS and hasattr(l, name), name
    assert C.sizeof(_lib.Sbv2StreamLevel) == 32
    assert [getattr(_lib.Sbv2StreamLevel, n).offset for n, _ in _lib.Sbv2StreamLevel._fields_] == [0, 8, 16]


def test_lookahead_and_bound_values():
    l = _lib.lib()
    for r in RATES:
        for enc in ("f32", "s16"):
            f = model.PcmFormat(r, enc)
            A = model.stream_level_lookahead(f)
            assert A == r // 100 + 11 == A_of(r)
            for chunk in (0, 1, 16 * 16, 16 * 512, 256 * 512):
                n = model.pcm_format_length(f, chunk)
                assert model.stream_level_bound(f, chunk) == (n + A) * (2 if enc == "s16" else 4) >= (n + A) * np.dtype(f.dtype).itemsize
                if enc == "s16":   # the FLAC bound's shape for a push of n + A samples
                    m = n + A
                    assert model.stream_level_bound(f, chunk, flac=True) == 42 + 16 * (-(-(m + 4095) // 4096)) + 2 * (m + 4095) >= 2 * m
    assert l.sbv2_stream_level_lookahead(_lib.Sbv2PcmFormat(11025, 0, 0, 0)) == -1 and b"sample rate" in l.sbv2_last_error()
    assert l.sbv2_stream_level_lookahead(_lib.Sbv2PcmFormat(16000, 7, 0, 0)) == -1 and b"encoding" in l.sbv2_last_error()
    assert l.sbv2_stream_level_lookahead(None) == -1
    assert l.sbv2_stream_level_bound(_lib.Sbv2PcmFormat(16000, 0, 0, 0), 100, 1) == -1 and b"s16" in l.sbv2_last_error()
    assert l.sbv2_stream_level_bound(_lib.Sbv2PcmFormat(16000, 1, 1, 0), 100, 0) == -1 and b"normali" in l.sbv2_last_error()
    assert l.sbv2_stream_level_bound(_lib.Sbv2PcmFormat(16000, 1, 0, 0), -1, 0) == -1


def test_level_struct_is_checked_before_any_device_call():
    """Range, non-finite and reserved-field refusals of sbv2_stream_level through both hooks: the checks run on the host first."""
    l = _lib.lib()
    x, out, st = np.zeros(8), np.zeros(8), np.zeros(2)
    per, lens = np.zeros(1, np.int64), np.array([8], np.int64)
    f64p = C.POINTER(C.c_double)

    def both(level, rate=16000, cuts=None, ncuts=0):
        rc1 = l.sbv2_debug_limiter_stream(0, x.ctypes.data, 8, cuts, ncuts, rate, level, out.ctypes.data, per.ctypes.data_as(_lib.i64p),
                                          st.ctypes.data_as(f64p))
        e1 = l.sbv2_last_error()
        rc2 = l.sbv2_debug_limiter_fixed(0, x.ctypes.data, lens.ctypes.data_as(_lib.i64p), 1, rate, level, out.ctypes.data, st.ctypes.data_as(f64p))
        return rc1, e1, rc2, l.sbv2_last_error()

    z2 = (C.c_double * 2)(0.0, 0.0)
    for g, c in ((-40.5, -1.0), (40.5, -1.0), (float("nan"), -1.0), (float("inf"), -1.0), (0.0, 0.5), (0.0, -20.5), (0.0, float("nan"))):
        rc1, e1, rc2, e2 = both(_lib.Sbv2StreamLevel(g, c, z2))
        assert rc1 != 0 and rc2 != 0 and b"outside" in e1 and b"outside" in e2, (g, c)
    for res in ((1.0, 0.0), (0.0, -2.0)):
        rc1, e1, rc2, e2 = both(_lib.Sbv2StreamLevel(0.0, -1.0, (C.c_double * 2)(*res)))
        assert rc1 != 0 and rc2 != 0 and b"reserved" in e1 and b"reserved" in e2, res
    rc1, e1, rc2, e2 = both(None)
    assert rc1 != 0 and rc2 != 0 and b"level" in e1 and b"level" in e2
    ok = _lib.Sbv2StreamLevel(6.0, -1.0, z2)
    rc1, e1, rc2, e2 = both(ok, rate=11025)
    assert rc1 != 0 and rc2 != 0 and b"sample rate" in e1 and b"sample rate" in e2
    bad = np.array([5, 4], np.int64)
    rc1, e1, _, _ = both(ok, cuts=bad.ctypes.data_as(_lib.i64p), ncuts=2)
    assert rc1 != 0 and b"ascend" in e1
    for bad_args in ((-41, -1), (41, -1), (0, 0.1), (0, -21), (float("nan"), -1)):
        with pytest.raises(model.Sbv2Error, match="outside"):
            model.StreamLevel(*bad_args)
    lv = model.StreamLevel(7.5)
    assert (lv.gain_db, lv.true_peak_max, lv.c.gain_db, lv.c.true_peak_max_dbtp, tuple(lv.c.reserved)) == (7.5, -1.0, 7.5, -1.0, (0.0, 0.0))


def test_gain_db_option_contracts(monkeypatch):
    styles = np.zeros((2, 4), np.float32)
    d = orchestrator.SynthesizeOptions()
    assert d.gain_db is None
    # the whole-signal routes refuse it and point to loudness, before any GPU work (RequestPlan is what easy_synthesize, the marks route
    # and the batcher all build first)
    opts = orchestrator.SynthesizeOptions(gain_db=6.0)
    for call in (lambda: orchestrator.easy_synthesize(None, [{"x": 1}], styles, 0, 0, opts),
                 lambda: orchestrator.easy_synthesize_marks(None, [{"x": 1}], styles, 0, 0, opts),
                 lambda: orchestrator.RequestPlan([{"x": 1}], styles, 0, 0, opts)):
        with pytest.raises(model.Sbv2Error, match="loudness"):
            call()
    from sbv2_api_amd import batcher

    class Pipe:
        pass

    rb = batcher.RequestBatcher(Pipe(), max_wait_ms=1)
    try:
        with pytest.raises(model.Sbv2Error, match="loudness"):
            r = rb.submit([{"x": 1}], styles, 0, 0, opts, noise_seed=1)
            r.result(timeout=10)
    finally:
        rb.close()
    # the three existing stream refusals stand word for word, with or without a gain
    for kw, msg in ((dict(normalize=True), "a stream cannot normalise: the peak needs the whole signal (use /synthesize)"),
                    (dict(loudness=-23.0), "a stream has no loudness or limiter: integrated loudness needs the whole signal (use /synthesize)"),
                    (dict(loudness=-16.0, limiter=True), "a stream has no loudness or limiter: integrated loudness needs the whole signal (use /synthesize)")):
        for gain in (None, 3.0):
            with pytest.raises(model.Sbv2Error) as e:
                orchestrator.easy_synthesize_stream(None, None, [{"x": 1}], styles, 0, 0, orchestrator.SynthesizeOptions(gain_db=gain, **kw))
            assert str(e.value) == msg
    with pytest.raises(model.Sbv2Error, match="outside"):
        orchestrator.easy_synthesize_stream(None, None, [{"x": 1}], styles, 0, 0, orchestrator.SynthesizeOptions(gain_db=50.0))
    # accepted on the stream path: the handle is opened with a StreamLevel at the ceiling, an explicit format also for the default one
    seen = []

    class Handle:
        total_samples = 10

        def __init__(self, bert, vits, utt, chunk_frames, fmt=None, flac=False, level=None, **kw):
            seen.append((fmt, flac, level))
            self.level, self.chunks = level, [np.zeros(0, np.float32), np.ones(10, np.float32)]

        def marks(self):
            return np.zeros(1, np.int64), np.full(1, 10, np.int64)

        def next(self):
            return self.chunks.pop(0) if self.chunks else None

        def level_stats(self):
            return (-3.5, 0.89)

        def close(self):
            pass

    monkeypatch.setattr(model, "StreamHandle", Handle)
    text = {"phones": [1], "word2ph": [1]}
    for enc, rate in (("f32", 44100), ("s16", 16000), ("flac", 48000)):
        st = orchestrator.easy_synthesize_stream(None, None, [text], styles, 0, 0,
                                                 orchestrator.SynthesizeOptions(gain_db=4.0, true_peak_max=-2.0, encoding=enc, sample_rate=rate))
        fmt, flac, level = seen[-1]
        assert fmt is not None and (fmt.sample_rate, fmt.encoding, fmt.normalize) == (rate, "f32" if enc == "f32" else "s16", False)
        assert flac == (enc == "flac") and (level.gain_db, level.true_peak_max) == (4.0, -2.0)
        assert st.level_stats is None
        pieces = list(st)
        assert len(pieces) == (1 if enc == "flac" else 2) and st.level_stats == (-3.5, 0.89)
        if enc != "flac":   # the WAV header names the full length: the total is the same with a level
            assert pieces[0] == orchestrator.wav_stream_header(rate, enc, 10)
    orchestrator.easy_synthesize_stream(None, None, [text], styles, 0, 0, None)
    assert seen[-1] == (None, False, None)   # without a gain: the plain stream, as before


def test_rest_hands_gain_db_to_the_holder():
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient
    from sbv2_api_amd import rest

    class Holder:
        def __init__(self):
            self.stream_opts = []

        def models(self):
            return ["m"]

        def easy_synthesize(self, ident, text, style_id, speaker_id, options):
            orchestrator.RequestPlan([{"x": 1}], np.zeros((1, 4), np.float32), 0, 0, options)   # (the real one plans the request first)
            return b"RIFF"

        def easy_synthesize_stream(self, ident, text, style_id, speaker_id, options):
            self.stream_opts.append(options)
            return iter([b"RIFF", b"one"])

    h = Holder()
    c = TestClient(rest.make_app(h))
    r = c.post("/synthesize_stream", json={"text": "a", "ident": "m", "encoding": "s16", "gain_db": 7.5, "true_peak_max": -2.0})
    assert r.status_code == 200 and r.content == b"RIFFone" and r.headers["content-type"] == "audio/wav"
    o = h.stream_opts[-1]
    assert (o.gain_db, o.true_peak_max, o.encoding, o.loudness, o.limiter, o.normalize) == (7.5, -2.0, "s16", None, False, False)
    r = c.post("/synthesize_stream", json={"text": "a", "ident": "m"})
    assert r.status_code == 200 and h.stream_opts[-1].gain_db is None
    r = c.post("/synthesize", json={"text": "a", "ident": "m", "gain_db": 3.0})
    assert r.status_code == 500 and "loudness" in r.text
    assert c.post("/synthesize", json={"text": "a", "ident": "m"}).status_code == 200


# ---- GPU: the hooks --------------------------------------------------------------------------------------------------------------------------

def _loud(n, rng, peaks=(), amp=0.2):
    y = amp * rng.standard_normal(n)
    for p in peaks:
        if 0 <= p < n:
            y[p] = 0.9 * (-1) ** p
    return y


def _fixed_signals(rate):
    """(signal, silent) pairs: the lengths at which the kernels change path, a loud onset inside the first K samples, a peak inside the
    last K, a silent signal.  Every non-silent one holds a sample at 0.9, which a gain of 12 dB puts at 3.6 c."""
    K, A = rate // 100, A_of(rate)
    rng = np.random.default_rng(rate + 7)
    out = [(np.zeros(0), True), (np.array([0.8]), False)]
    for n in (K - 1, K, A, A + 1, 1024, 1025, 3001):
        out.append((_loud(n, rng, peaks=(n // 2,)), False))
    onset = _loud(3000, rng, peaks=(K // 3,))
    onset[:3] = -0.9
    out.append((onset, False))
    out.append((_loud(3000, rng, peaks=(3000 - K // 2,), amp=0.01), False))
    out.append((np.zeros(2500), True))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("rate", (8000, 16000, 44100, 48000))
def test_fixed_one_shot_equals_numpy(rate):
    sigs = _fixed_signals(rate)
    worst = 0.0
    for gain_db, ceiling in ((12.0, -1.0), (20.0, -6.0)):
        lv = model.StreamLevel(gain_db, ceiling)
        c = 10 ** (ceiling / 20)
        got, stats = model.debug_limiter_fixed([y for y, _ in sigs], rate, lv)
        assert stats.shape == (len(sigs), 2) and len(got) == len(sigs)
        for i, ((y, silent), g) in enumerate(zip(sigs, got)):
            x, s = fixed_ref(y, rate, gain_db, ceiling)
            assert g.shape == x.shape
            if silent:
                assert not g.any() and stats[i, 1] == 0.0 and abs(stats[i, 0]) < 1e-12, (rate, i, stats[i])   # (min(sum over ones, 1): within an ulp of 1)
                continue
            assert np.abs(g).max() <= c, (rate, i)
            assert s.min() < 0.9, (rate, i, s.min())   # the premise: the curve is not idle on this signal
            assert stats[i, 0] < 20 * np.log10(0.9) and abs(stats[i, 0] - 20 * np.log10(s.min())) < 1e-9, (rate, i, stats[i])
            assert stats[i, 1] == np.abs(g).max(), (rate, i)
            worst = max(worst, float(np.abs(g - x).max() / np.abs(x).max()))
    print(f"{rate}: fixed one-shot x max-abs error {worst:.3e} of the peak")
    assert worst <= X_REL_TOL, (rate, worst)


def _cut_sets(n, A, peak, rng):
    sets = [[], list(range(max(A - 1, 1), n, max(A - 1, 1))), list(range(37, n, 37)), [c for c in (1, A, A + 1, n - 1, n) if 0 <= c <= n],
            [c for c in (A, A, A) if c <= n], [c for c in (peak, peak + 1) if 0 <= c <= n], [c for c in (peak - 3, peak + 5) if 0 <= c <= n]]
    sets.append(sorted(c for k in range(1, n // 1024 + 2) for c in (1024 * k - 1, 1024 * k, 1024 * k, 1024 * k + 1) if 0 <= c <= n))
    sets.append([c for c in (n,) * 2])
    for _ in range(11):
        k = int(rng.integers(1, 9))
        c = np.sort(rng.integers(0, n + 1, k))
        if k >= 2 and rng.random() < 0.5:
            c[int(rng.integers(1, k))] = c[0]
            c = np.sort(c)
        sets.append([int(v) for v in c])
    return [sorted(s) for s in sets]


@pytest.mark.gpu
def test_fed_limiter_is_invariant_to_the_cuts_bit_for_bit():
    rng = np.random.default_rng(4242)
    cases = []   # (rate, signal, a peak's position)
    for rate, sizes in ((16000, (0, 1, 170, 171, 172, 342, 343, 1024, 1025, 2048 + 171, 3000, 5000)), (8000, (91, 93, 2500)),
                        (44100, (452, 453, 4000)), (48000, (3500, 491))):
        for n in sizes:
            peak = int(rng.integers(0, max(n, 1)))
            y = _loud(n, rng, peaks=(peak, n - 2, 1))
            cases.append((rate, y, peak))
    cases.append((16000, np.zeros(1500), 700))
    assert len(cases) >= 20
    lv = model.StreamLevel(12.0, -1.0)
    shots = {}
    checked = 0
    for rate, y, peak in cases:
        A = A_of(rate)
        if rate not in shots:
            group = [c[1] for c in cases if c[0] == rate]
            xs, st = model.debug_limiter_fixed(group, rate, lv)
            shots[rate] = {id(g): (x, s) for g, x, s in zip(group, xs, st)}
        one, one_stats = shots[rate][id(y)]
        assert not y.any() or one_stats[0] < 20 * np.log10(0.9), (rate, y.size, one_stats)
        for cuts in _cut_sets(y.size, A, peak, rng):
            parts, stats = model.debug_limiter_stream(y, cuts, rate, lv)
            sizes = np.diff([0] + cuts + [y.size])
            assert [p.size for p in parts] == delivery(sizes, A), (rate, y.size, cuts)
            got = np.concatenate(parts)
            assert np.array_equal(got.view(np.uint64), one.view(np.uint64)), (rate, y.size, cuts, int(np.argmax(got != one)))
            assert np.array_equal(stats.view(np.uint64), np.asarray(one_stats).view(np.uint64)), (rate, y.size, cuts, stats, one_stats)
            checked += 1
    assert checked >= 20 * len(cases)
    rate, y, peak = cases[10]
    cuts = [5, 5, 1024, 2000, y.size]
    a, sa = model.debug_limiter_stream(y, cuts, rate, lv)
    b, sb = model.debug_limiter_stream(y, cuts, rate, lv)
    assert np.concatenate(a).tobytes() == np.concatenate(b).tobytes() and sa.tobytes() == sb.tobytes()


@pytest.mark.gpu
def test_frame_sized_pushes_at_8k_concatenate_to_the_one_shot():
    """Pushes the size of single 512-sample decoder frames at 8 kHz (92 or 93 samples against A = 91), and pushes of a third of that, which
    take samples and emit none: the pieces still concatenate to the one-shot signal."""
    rate, A = 8000, A_of(8000)
    f = model.PcmFormat(rate, "f32")
    edges = [model.pcm_format_length(f, 512 * k) for k in range(41)]
    assert set(np.diff(edges)) == {92, 93} and A == 91
    rng = np.random.default_rng(8)
    y = _loud(edges[-1], rng, peaks=(5, 900, 901, 2000, edges[-1] - 4))
    lv = model.StreamLevel(12.0, -1.0)
    (one,), st1 = model.debug_limiter_fixed([y], rate, lv)
    assert st1[0, 0] < 20 * np.log10(0.9)
    for cuts in (edges[1:-1], list(range(31, y.size, 31))):
        parts, st = model.debug_limiter_stream(y, cuts, rate, lv)
        sizes = np.diff([0] + list(cuts) + [y.size])
        assert [p.size for p in parts] == delivery(sizes, A)
        assert np.array_equal(np.concatenate(parts).view(np.uint64), one.view(np.uint64)) and st.tobytes() == st1[0].tobytes()
    assert [p.size for p in parts][:3] == [0, 0, 2]   # 31, 62, 93 samples fed: nothing, nothing, 93 - 91


# ---- GPU: the synthesis stream -----------------------------------------------------------------------------------------------------------------

def _tiny():
    bc, _ = weights("bert", "tiny", 3)
    vc, _ = weights("vits", "tiny", 5)
    return bc, vc, model.load_model(blob("bert", "tiny", 3), True), model.load_model(blob("vits", "tiny", 5), False)


def _hop(vs):
    return _lib.lib().sbv2_vits_hop(vs.handle)


def _chunks(bs, vs, u, chunk, fmt=None, **kw):
    st = model.StreamHandle(bs, vs, u, chunk, fmt=fmt, **kw)
    parts = []
    while (c := st.next()) is not None:
        parts.append(c)
    st.close()
    return parts


def _level_calls(bs, vs, u, chunk, fmt, lv, flac=False, **kw):
    """([(delivered, n_consumed)] per sbv2_stream_next_level call that consumed samples, total_samples, level stats)."""
    l = _lib.lib()
    st = model.StreamHandle(bs, vs, u, chunk, fmt=fmt, flac=flac, level=lv, **kw)
    assert st.buf.nbytes == model.stream_level_bound(fmt, chunk * _hop(vs), flac)
    with pytest.raises(model.Sbv2Error, match="complete"):
        st.level_stats()
    calls = []
    no, nc = C.c_int64(), C.c_int64()
    while True:
        _lib.check(l.sbv2_stream_next_level(st.h, st.buf.ctypes.data, st.buf.nbytes, C.byref(no), C.byref(nc)))
        if nc.value == 0:
            assert no.value == 0
            break
        calls.append((st.buf[:no.value].tobytes() if flac else st.buf[:no.value * np.dtype(fmt.dtype).itemsize].view(fmt.dtype).copy(), nc.value))
    _lib.check(l.sbv2_stream_next_level(st.h, st.buf.ctypes.data, st.buf.nbytes, C.byref(no), C.byref(nc)))
    assert (no.value, nc.value) == (0, 0)   # the end marker repeats
    total, stats = st.total_samples, st.level_stats()
    st.close()
    return calls, total, stats


def _active_gain(y, ceiling, over_db=9.0):
    """The gain that puts the peak of y over_db above the ceiling (within the struct's range): the limiter cannot be idle."""
    g = ceiling - 20 * np.log10(np.abs(y).max()) + over_db
    assert -40.0 <= g <= 40.0, g
    return float(np.round(g, 2))


def _check_rule(calls, total, fmt, frames, chunk, hop):
    edges = [model.pcm_format_length(fmt, min(c * chunk, frames) * hop) for c in range(-(-frames // chunk) + 1)]
    assert [n for _, n in calls] == list(np.diff(edges)), "n_consumed per call = the formatted stream's chunk"
    assert edges[-1] == total
    return delivery(np.diff(edges), model.stream_level_lookahead(fmt))


@pytest.mark.gpu
def test_level_stream_tiny_identity_rate_bit_for_bit():
    """44.1 kHz f32 on the tiny decoder (hop 16): the resampler is the identity, so y is the plain stream's f32 PCM exactly and the level
    stream must equal float32(one-shot limiter of float64(plain)) in every bit, for 16- and 64-frame chunks (256 and 1024 samples
    against A = 452: the first 16-frame call consumes samples and delivers none)."""
    bc, vc, bs, vs = _tiny()
    hop = _hop(vs)
    u = make_utts([700], bc, vc, seed0=1000, with_bert=False)[0]
    fmt = model.PcmFormat(44100, "f32")
    plain = np.concatenate(_chunks(bs, vs, u, 64, forced=True))
    ceiling = -1.0 if np.abs(plain).max() > 0.02 else -20.0
    lv = model.StreamLevel(_active_gain(plain, ceiling), ceiling)
    (one,), st1 = model.debug_limiter_fixed([plain.astype(np.float64)], 44100, lv)
    want = one.astype(np.float32)
    assert st1[0, 0] < -3.0, st1   # the limiter is active
    for chunk in (16, 64):
        calls, total, stats = _level_calls(bs, vs, u, chunk, fmt, lv, forced=True)
        assert total == plain.size
        rule = _check_rule(calls, total, fmt, plain.size // hop, chunk, hop)
        assert [d.size for d, _ in calls] == rule
        got = np.concatenate([d for d, _ in calls])
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (chunk, int(np.argmax(got != want)))
        assert stats == (st1[0, 0], st1[0, 1]) and stats[0] < -3.0
        if chunk == 16:
            assert rule[0] == 0 and rule[1] == 2 * 256 - 452 and calls[0][1] == 256
    # the marks are those of the formatted stream: time is not shifted
    a = model.StreamHandle(bs, vs, u, 64, fmt=fmt, forced=True)
    b = model.StreamHandle(bs, vs, u, 64, fmt=fmt, level=lv, forced=True)
    ma, mb = a.marks(), b.marks()
    a.close(); b.close()
    assert np.array_equal(ma[0], mb[0]) and np.array_equal(ma[1], mb[1])
    bs.close(); vs.close()


def _check_resampled(bs, vs, u, chunk, rate, what, **kw):
    """s16 and f32 level streams at a resampled rate against the hook on the f64 of the f32-formatted stream; returns the f32 deviation."""
    hop = _hop(vs)
    f32, s16 = model.PcmFormat(rate, "f32"), model.PcmFormat(rate, "s16")
    y32 = np.concatenate(_chunks(bs, vs, u, chunk, fmt=f32, **kw))
    ceiling = -1.0 if np.abs(y32).max() > 0.02 else -20.0
    lv = model.StreamLevel(_active_gain(y32, ceiling), ceiling)
    c = 10 ** (ceiling / 20)
    (one,), st1 = model.debug_limiter_fixed([y32.astype(np.float64)], rate, lv)
    assert st1[0, 0] < -3.0, (what, st1)
    frames = model.StreamHandle(bs, vs, u, chunk, **kw)
    nfr = frames.total_samples // hop
    frames.close()
    calls, total, stats = _level_calls(bs, vs, u, chunk, f32, lv, **kw)
    assert [d.size for d, _ in calls] == _check_rule(calls, total, f32, nfr, chunk, hop) and total == y32.size
    got = np.concatenate([d for d, _ in calls]).astype(np.float64)
    dev = float(np.abs(got - one.astype(np.float32)).max())
    assert stats[0] < -3.0 and abs(stats[0] - st1[0, 0]) < 1e-4 and stats[1] <= c
    calls16, total16, stats16 = _level_calls(bs, vs, u, chunk, s16, lv, **kw)
    assert [d.size for d, _ in calls16] == [d.size for d, _ in calls] and total16 == total and stats16 == stats   # the same x before the quantiser
    got16 = np.concatenate([d for d, _ in calls16]).astype(np.int64)
    want16 = np.clip(np.rint(one * 32767.0), -32767, 32767).astype(np.int64)
    dev16 = int(np.abs(got16 - want16).max())
    print(f"{what}: f32 deviation {dev:.3e} of full scale, s16 deviation {dev16} steps, depth {stats[0]:.2f} dB, max |x| {stats[1]:.6f} (c = {c:.6f})")
    assert np.abs(got16).max() <= np.rint(c * 32767), what
    assert dev16 <= S16_STEP, (what, dev16)
    assert dev <= min(8 * F32_ROUNDING_DEV, 1 / 32767), (what, dev)
    return dev


@pytest.mark.gpu
def test_level_stream_tiny_resampled_48k():
    bc, vc, bs, vs = _tiny()
    u = make_utts([700], bc, vc, seed0=1000, with_bert=False)[0]
    _check_resampled(bs, vs, u, 64, 48000, "tiny 48 kHz", forced=True)
    bs.close(); vs.close()


@pytest.fixture(scope="module")
def full_models():
    bs, vs = model.load_model(blob("bert", "full"), True), model.load_model(blob("vits", "full"), False)
    yield weights("bert", "full")[0], weights("vits", "full")[0], bs, vs
    bs.close(); vs.close()


@pytest.mark.gpu
def test_level_stream_full_model_16k(full_models):
    bc, vc, bs, vs = full_models
    assert _hop(vs) == 512
    u = synth.make_utterance(60, bc, vc, seed=91)
    _check_resampled(bs, vs, u, 64, 16000, "full 16 kHz", forced=True)


@pytest.mark.gpu
def test_level_flac_stream_decodes_to_the_s16_level_stream():
    bc, vc, bs, vs = _tiny()
    u = make_utts([700], bc, vc, seed0=1000, with_bert=False)[0]
    for rate, chunk in ((44100, 16), (48000, 64)):
        fmt = model.PcmFormat(rate, "s16")
        y = np.concatenate(_chunks(bs, vs, u, chunk, fmt=model.PcmFormat(rate, "f32"), forced=True))
        ceiling = -1.0 if np.abs(y).max() > 0.02 else -20.0
        lv = model.StreamLevel(_active_gain(y, ceiling), ceiling)
        pcm, total, stats = _level_calls(bs, vs, u, chunk, fmt, lv, forced=True)
        x = np.concatenate([d for d, _ in pcm])
        fl, total_f, stats_f = _level_calls(bs, vs, u, chunk, fmt, lv, flac=True, forced=True)
        assert total_f == total == x.size and stats_f == stats and stats[0] < -3.0
        assert [n for _, n in fl] == [n for _, n in pcm]
        data = b"".join(b for b, _ in fl)
        got = R.read(data)
        np.testing.assert_array_equal(got["samples"], x)
        assert got["rate"] == rate and got["total"] == x.size and x.size > 4096
        one_shot = model.debug_flac_encode([x], rate)[0]
        assert data[12:18] == bytes(6) and data[:12] == one_shot[:12] and data[18:] == one_shot[18:]
        assert all(len(b) <= model.stream_level_bound(fmt, chunk * _hop(vs), True) for b, _ in fl) and len(fl[0][0]) >= 42
        # each call holds the frames that the samples delivered so far complete
        sizes = [f["size"] for f in got["frames"]]
        upto_s = np.cumsum([d.size for d, _ in pcm])
        done = 0
        for i, (b, _) in enumerate(fl):
            upto = len(sizes) if i == len(fl) - 1 else int(upto_s[i]) // 4096
            assert len(b) == sum(sizes[done:upto]) + (42 if i == 0 else 0), (rate, i)
            done = upto
    bs.close(); vs.close()


@pytest.mark.gpu
def test_level_stream_refusals_and_retry_with_more_room():
    bc, vc, bs, vs = _tiny()
    l = _lib.lib()
    u = make_utts([700], bc, vc, seed0=1000, with_bert=False)[0]
    lv = model.StreamLevel(20.0, -6.0)
    with pytest.raises(model.Sbv2Error, match="normali"):
        model.StreamHandle(bs, vs, u, 64, fmt=model.PcmFormat(48000, "s16", True), level=lv, forced=True)
    with pytest.raises(model.Sbv2Error, match="s16"):
        model.StreamHandle(bs, vs, u, 64, fmt=model.PcmFormat(48000, "f32"), flac=True, level=lv, forced=True)
    with pytest.raises(model.Sbv2Error, match="format"):
        model.StreamHandle(bs, vs, u, 64, level=lv, forced=True)
    with pytest.raises(model.Sbv2Error, match="halo"):      # the halo check of the formatted stream applies unchanged
        model.StreamHandle(bs, vs, u, 64, fmt=model.PcmFormat(16000, "s16"), level=lv, forced=True)
    fmt = model.PcmFormat(48000, "s16")
    want, total, stats = _level_calls(bs, vs, u, 64, fmt, lv, forced=True)
    x = np.concatenate([d for d, _ in want])
    n, nb, nc = C.c_int64(), C.c_int64(), C.c_int64()
    for flac in (False, True):
        st = model.StreamHandle(bs, vs, u, 64, fmt=fmt, flac=flac, level=lv, forced=True)
        # the other three ways of taking chunks are refused on a level stream, and consume nothing
        assert l.sbv2_stream_next(st.h, st.buf.ctypes.data, st.buf.nbytes // 4, C.byref(n)) != 0 and b"sbv2_stream_next_level" in l.sbv2_last_error()
        assert l.sbv2_stream_next_format(st.h, st.buf.ctypes.data, st.buf.nbytes, C.byref(n)) != 0 and b"sbv2_stream_next_level" in l.sbv2_last_error()
        assert l.sbv2_stream_next_flac(st.h, st.buf.ctypes.data, st.buf.nbytes, C.byref(nb), C.byref(n)) != 0
        assert b"sbv2_stream_next_level" in l.sbv2_last_error()
        st_err = np.zeros(2)
        assert l.sbv2_stream_level_stats(st.h, st_err.ctypes.data_as(C.POINTER(C.c_double))) != 0 and b"complete" in l.sbv2_last_error()
        # too small a capacity: refused, nothing written, nothing consumed; the repeat with the bound succeeds
        small = np.full(41, 0xA5, np.uint8)
        parts, refused = [], 0
        while True:
            rc = l.sbv2_stream_next_level(st.h, small.ctypes.data, small.nbytes, C.byref(nb), C.byref(nc))
            if rc != 0:
                assert b"too small" in l.sbv2_last_error() and (small == 0xA5).all()
                refused += 1
                _lib.check(l.sbv2_stream_next_level(st.h, st.buf.ctypes.data, st.buf.nbytes, C.byref(nb), C.byref(nc)))
                parts.append(st.buf[:nb.value * (1 if flac else 2)].tobytes())
            else:
                if nc.value == 0:
                    break
                parts.append(small[:nb.value * (1 if flac else 2)].tobytes())
                small[:] = 0xA5
        assert refused >= 2 and st.level_stats() == stats
        st.close()
        data = b"".join(parts)
        got = R.read(data)["samples"] if flac else np.frombuffer(data, np.int16)
        np.testing.assert_array_equal(got, x)
    # _next_level on the other kinds of stream
    for kw in (dict(fmt=fmt, flac=True), dict(fmt=fmt), dict()):
        st = model.StreamHandle(bs, vs, u, 64, forced=True, **kw)
        buf = np.empty(1 << 16, np.uint8)
        assert l.sbv2_stream_next_level(st.h, buf.ctypes.data, buf.nbytes, C.byref(nb), C.byref(nc)) != 0
        assert b"not begun with a level" in l.sbv2_last_error()
        assert l.sbv2_stream_level_stats(st.h, np.zeros(2).ctypes.data_as(C.POINTER(C.c_double))) != 0
        st.close()
    bs.close(); vs.close()


@pytest.mark.gpu
def test_easy_synthesize_stream_with_gain_wav_and_flac():
    import scipy.io.wavfile as W
    bc, vc, bs, vs = _tiny()
    keys = ("input_ids", "word2ph", "phones", "tones", "langs")
    text = {k: synth.make_utterance(600, bc, vc, seed=777)[k] for k in keys}
    styles = synth.hash_normal(77, 3 * vc["style_dim"]).reshape(3, -1).astype(np.float32)

    def run(**kw):
        st = orchestrator.easy_synthesize_stream(bs, vs, [text], styles, 1, 0, orchestrator.SynthesizeOptions(**kw), noise_seed=1234, chunk_frames=64)
        return b"".join(st), st

    plain, _ = run()
    _, y = W.read(io.BytesIO(plain))
    ceiling = -1.0 if np.abs(y).max() > 0.02 else -20.0
    gain = _active_gain(y, ceiling)
    c = 10 ** (ceiling / 20)
    wav, st = run(gain_db=gain, true_peak_max=ceiling)   # the default format becomes an explicit 44.1 kHz f32 one
    rate, z = W.read(io.BytesIO(wav))
    assert rate == 44100 and z.dtype == np.float32 and z.size == y.size and len(wav) == len(plain)
    assert st.level_stats is not None and st.level_stats[0] < -3.0 and st.level_stats[1] <= c
    (one,), _ = model.debug_limiter_fixed([y.astype(np.float64)], 44100, model.StreamLevel(gain, ceiling))
    assert np.array_equal(z, one.astype(np.float32))
    wav16, st16 = run(gain_db=gain, true_peak_max=ceiling, encoding="s16", sample_rate=48000)
    rate, z16 = W.read(io.BytesIO(wav16))
    assert rate == 48000 and z16.dtype == np.int16 and len(wav16) == 44 + 2 * z16.size and np.abs(z16.astype(np.int64)).max() <= np.rint(c * 32767)
    pieces, stf = run(gain_db=gain, true_peak_max=ceiling, encoding="flac", sample_rate=48000)
    got = R.read(pieces)
    assert got["rate"] == 48000 and stf.level_stats == st16.level_stats
    np.testing.assert_array_equal(got["samples"], z16)
    bs.close(); vs.close()
