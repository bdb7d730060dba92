"""Loudness normalisation (csrc/loudness.hip, sbv2_pipeline_fetch_pcm_loudness / _fetch_flac_loudness): BS.1770-4 integrated loudness with both
gates, a 4x true-peak meter and the per-signal gain G = min(target - L, ceiling - TP) dB, on the device.

The reference is a numpy / scipy restatement of the convention of include/sbv2_hip.h (sbv2_loudness), in float64, checked itself against the
BS.1770-4 coefficient table and the EBU Tech 3341 cases 1-5 (mono: amplitude x sqrt(2)).  CPU tests run anywhere; GPU tests
(@pytest.mark.gpu) need an MI355X."""
import io

import numpy as np
import pytest

import flac_reader as R
from helpers import blob, make_utts, weights
from sbv2_api_amd import _lib, model, orchestrator, synth
from test_pcm_format import check_format, ref_format

RATES = (8000, 16000, 22050, 24000, 32000, 44100, 48000)
BS1770_48K = ([1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585],
              [1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621])
# EBU Tech 3341 cases 1-5: [(dBFS, seconds)] of 1 kHz tones -> expected LUFS
EBU = [([(-23, 20)], -23.0), ([(-33, 20)], -33.0), ([(-36, 10), (-23, 60), (-36, 10)], -23.0),
       ([(-72, 10), (-36, 10), (-23, 60), (-36, 10), (-72, 10)], -23.0), ([(-26, 20), (-20, 20.1), (-26, 20)], -23.0)]


# ---- the numpy reference ------------------------------------------------------------------------------------------------------------------

def kweight(rate):
    """[shelf b0 b1 b2 a1 a2, high-pass b0 b1 b2 a1 a2] in the libebur128 form."""
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = np.tan(np.pi * f0 / rate)
    Vh = 10 ** (G / 20)
    Vb = Vh ** 0.4996667741545416
    a0 = 1 + K / Q + K * K
    shelf = [(Vh + Vb * K / Q + K * K) / a0, 2 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0, 2 * (K * K - 1) / a0, (1 - K / Q + K * K) / a0]
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = np.tan(np.pi * f0 / rate)
    d = 1 + K / Q + K * K
    return np.array(shelf + [1.0, -2.0, 1.0, 2 * (K * K - 1) / d, (1 - K / Q + K * K) / d])


def h4():
    n = np.arange(-48, 49)
    h = np.sinc(n / 4) * np.i0(8.6 * np.sqrt(1 - (n / 48.0) ** 2)) / np.i0(8.6)
    for p in range(4):
        h[n % 4 == p] /= h[n % 4 == p].sum()
    return h


def integrated(y, rate):
    """L (LUFS) of a float64 signal at rate."""
    import scipy.signal as S
    y = np.asarray(y, np.float64)
    n = y.size
    if n == 0:
        return -np.inf
    c = kweight(rate)
    w = S.lfilter(c[5:8], [1.0, c[8], c[9]], S.lfilter(c[0:3], [1.0, c[3], c[4]], y))
    q = rate // 10
    if n < 4 * q:
        z = np.array([np.sum(w * w) / n])
    else:
        nq = n // q
        qs = (w[:nq * q] ** 2).reshape(nq, q).sum(axis=1)
        z = (qs[:-3] + qs[1:-2] + qs[2:-1] + qs[3:]) / (4 * q)
    with np.errstate(divide="ignore"):
        lj = -0.691 + 10 * np.log10(z)
        keep = lj > -70
        if not keep.any():
            return -np.inf
        gate = -0.691 + 10 * np.log10(z[keep].mean()) - 10
        keep &= lj > gate
        return -0.691 + 10 * np.log10(z[keep].mean())


def true_peak(y):
    import scipy.signal as S
    y = np.asarray(y, np.float64)
    if y.size == 0:
        return -np.inf
    m = np.abs(S.resample_poly(y, 4, 1, window=h4() / 4)).max()
    with np.errstate(divide="ignore"):
        return 20 * np.log10(m)


def meter(y, rate, target=None, ceiling=-1.0):
    """(L, TP, G) of the convention; target None: measure only (G = 0)."""
    L, tp = integrated(y, rate), true_peak(y)
    G = min(target - L, ceiling - tp) if target is not None and np.isfinite(L) else 0.0
    return np.array([L, tp, G])


def apply_gain(y, G, encoding):
    v = np.asarray(y, np.float64) * 10 ** (G / 20)
    return np.clip(np.rint(v * 32767.0), -32767, 32767) if encoding == "s16" else v


def tone(parts, rate, freq=1000.0):
    x = [np.sqrt(2) * 10 ** (db / 20) * np.sin(2 * np.pi * freq * np.arange(int(round(s * rate))) / rate) for db, s in parts]
    return np.concatenate(x)


def close_stats(got, ref, tol=1e-6, what=""):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, what
    for g, r in zip(got.reshape(-1), ref.reshape(-1)):
        if np.isinf(r):
            assert g == r, f"{what}: {got} vs {ref}"
        else:
            assert abs(g - r) <= tol, f"{what}: {got} vs {ref}"


# ---- CPU ----------------------------------------------------------------------------------------------------------------------------------

def test_kweight_matches_bs1770_table_and_derivation():
    c = model.loudness_kweight(48000)
    assert np.abs(c[:5] - BS1770_48K[0]).max() <= 1e-12
    assert np.abs(c[5:] - BS1770_48K[1]).max() <= 1e-12
    for r in RATES:
        assert np.abs(model.loudness_kweight(r) - kweight(r)).max() <= 1e-12, r
    for bad in (44000, 96000, 0):
        with pytest.raises(model.Sbv2Error, match="sample rate"):
            model.loudness_kweight(bad)


@pytest.mark.parametrize("rate", RATES)
def test_numpy_meter_passes_ebu_3341_cases_1_to_5(rate):
    for parts, want in EBU:
        got = integrated(tone(parts, rate), rate)
        assert abs(got - want) <= 0.1, (rate, parts, got)


def test_numpy_true_peak_reference_points():
    import scipy.signal as S
    y = np.sin(2 * np.pi * np.arange(4800) / 4 + np.pi / 4)   # fs / 4 at 45 degrees: samples at +-0.707
    assert abs(20 * np.log10(np.abs(y).max()) + 3.0103) < 1e-3
    z = S.resample_poly(y, 4, 1, window=h4() / 4)
    assert abs(20 * np.log10(np.abs(z[400:-400]).max())) < 1e-3   # away from the edges' ringing: the tone's peak, 0 dB
    assert true_peak(y) >= 0.0
    x = np.random.default_rng(5).standard_normal(999)
    assert true_peak(x) >= 20 * np.log10(np.abs(x).max())


def test_options_and_rest_carry_loudness():
    d = orchestrator.SynthesizeOptions()
    assert (d.loudness, d.true_peak_max, d.normalize) == (None, -1.0, False)
    o = orchestrator.SynthesizeOptions(loudness=-16, true_peak_max=-2.0)
    assert (o.loudness, o.true_peak_max) == (-16, -2.0)
    with pytest.raises(model.Sbv2Error, match="normalize"):
        orchestrator.SynthesizeOptions(normalize=True, loudness=-16)
    for bad in ((-80, -1), (-3, -1), (-16, 0.5), (-16, -25), (float("nan"), -1), (-16, float("inf"))):
        with pytest.raises(model.Sbv2Error, match="outside"):
            model.Loudness(*bad)
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
    assert (o.loudness, o.true_peak_max, o.normalize, o.sample_rate, o.encoding) == (None, -1.0, False, 44100, "f32")
    r = c.post("/synthesize", json={"text": "a", "ident": "m", "loudness": -23, "true_peak_max": -2, "encoding": "s16"})
    assert r.status_code == 200 and r.headers["content-type"] == "audio/wav"
    assert (h.opts[-1].loudness, h.opts[-1].true_peak_max) == (-23, -2)
    n = len(h.opts)
    r = c.post("/synthesize", json={"text": "a", "ident": "m", "loudness": -16, "normalize": True})
    assert r.status_code == 500 and r.text.startswith("Something went wrong: ") and "normalize" in r.text
    assert len(h.opts) == n


# ---- GPU: the meter on host signals -------------------------------------------------------------------------------------------------------

def _debug_signals(rate):
    S = rate // 10
    rng = np.random.default_rng(rate)
    sigs = [tone(p, rate) for p, _ in EBU]
    burst = np.zeros(3 * rate)   # tone bursts in silence: the gates leave the silent blocks out
    for a in (0.2 * rate, 1.4 * rate, 2.5 * rate):
        a = int(a)
        burst[a:a + rate // 3] = 0.3 * np.sin(2 * np.pi * 440 * np.arange(rate // 3) / rate)
    sigs.append(burst)
    for n in (0, 1, 4 * S - 1, 4 * S, 4 * S + 1):
        sigs.append(0.25 * rng.standard_normal(n))
    sigs.append(np.zeros(2 * rate))
    sigs.append(np.sin(2 * np.pi * np.arange(rate) / 4 + np.pi / 4))
    return sigs


@pytest.mark.gpu
@pytest.mark.parametrize("rate", RATES)
def test_debug_meter_equals_numpy_and_ebu(rate):
    sigs = _debug_signals(rate)
    ref = np.array([meter(x, rate) for x in sigs])
    got = model.debug_loudness(sigs, rate)
    close_stats(got, ref, what=f"{rate} measure only")
    for i, (_, want) in enumerate(EBU):
        assert abs(got[i, 0] - want) <= 0.1, (rate, i, got[i])
    assert got[len(EBU) + 1, 0] == -np.inf and got[-2, 0] == -np.inf and got[-2, 1] == -np.inf   # empty, silence
    assert got[-1, 1] >= 0.0 > 20 * np.log10(np.abs(sigs[-1]).max()) + 3   # fs / 4 at 45 degrees: TP 3 dB above the sample peak
    # G follows the rule: loudness-limited at -16 LUFS, true-peak-limited at -5 LUFS under a -6 dBTP ceiling
    for target, ceiling in ((-16.0, -1.0), (-5.0, -6.0)):
        g = model.debug_loudness(sigs, rate, model.Loudness(target, ceiling))
        close_stats(g, np.array([meter(x, rate, target, ceiling) for x in sigs]), what=f"{rate} {target} {ceiling}")
    g = model.debug_loudness(sigs[:1], rate, model.Loudness(-16.0, -1.0))[0]
    assert abs(g[2] - (-16.0 - g[0])) < 1e-9 and g[1] + g[2] < -1.0
    g = model.debug_loudness(sigs[:1], rate, model.Loudness(-5.0, -6.0))[0]
    assert abs(g[2] - (-6.0 - g[1])) < 1e-9 and g[0] + g[2] < -5.0


# ---- GPU: the pipeline --------------------------------------------------------------------------------------------------------------------

def _tiny():
    bc, _ = weights("bert", "tiny", 3)
    vc, _ = weights("vits", "tiny", 5)
    bs, vs = model.load_model(blob("bert", "tiny", 3), True), model.load_model(blob("vits", "tiny", 5), False)
    return bc, vc, bs, vs


def _check_loudness(got, stats, y, rate, enc, ln, what):
    ref = meter(y, rate, ln.target_lufs, ln.true_peak_max)
    close_stats(stats, ref, what=what)
    check_format(got, apply_gain(y, ref[2], enc), enc, what)


@pytest.mark.gpu
def test_fetch_loudness_every_rate_encoding_layout():
    bc, vc, bs, vs = _tiny()
    pipe = model.Pipeline(bs, vs)
    utts = make_utts([9, 1, 23, 14, 40], bc, vc, seed0=501, with_bert=False)
    b = pipe.prepare(utts, forced=True)
    pipe.run(b)
    native = pipe.fetch(b)
    lens = [len(x) for x in native]
    place, pos = [], 0
    for n in lens:   # the joined timeline of easy_synthesize: 22050 silent samples between sentences
        place.append(pos)
        pos += n + orchestrator.SENTENCE_GAP
    joined = pos - orchestrator.SENTENCE_GAP
    timeline = np.zeros(joined, np.float32)
    for p, x in zip(place, native):
        timeline[p:p + len(x)] = x
    ln = model.Loudness(-20.0, -1.0)
    for rate in RATES:
        for enc in ("f32", "s16"):
            f = model.PcmFormat(rate, enc)
            before = [pipe.fetch_format(b, g) for g in (f, model.PcmFormat(rate, enc, True))]
            got, stats = pipe.fetch_loudness(b, f, ln)
            assert len(got) == len(utts) and stats.shape == (len(utts), 3)
            for i, (g, x) in enumerate(zip(got, native)):
                assert g.dtype == f.dtype
                _check_loudness(g, stats[i], ref_format(x, rate, "f32", False), rate, enc, ln, f"{f} utterance {i}")
            gj, sj = pipe.fetch_loudness(b, f, ln, place, joined)
            assert len(gj) == 1
            _check_loudness(gj[0], sj[0], ref_format(timeline, rate, "f32", False), rate, enc, ln, f"{f} joined")
            # measure only: the bytes of fetch_format, stats with G = 0
            for pl, jl in ((None, None), (place, joined)):
                m, ms = pipe.fetch_loudness(b, f, None, pl, jl)
                assert np.concatenate(m).tobytes() == np.concatenate(pipe.fetch_format(b, f, pl, jl)).tobytes(), (f, pl is None)
                assert (ms[:, 2] == 0).all()
            # repeatable, and the shared scratch leaves the other formats' bytes as they were
            again, stats2 = pipe.fetch_loudness(b, f, ln)
            assert np.concatenate(again).tobytes() == np.concatenate(got).tobytes() and stats2.tobytes() == stats.tobytes(), f
            after = [pipe.fetch_format(b, g) for g in (f, model.PcmFormat(rate, enc, True))]
            for x, y in zip(before, after):
                assert np.concatenate(x).tobytes() == np.concatenate(y).tobytes(), f
    with pytest.raises(model.Sbv2Error, match="normali"):
        pipe.fetch_loudness(b, model.PcmFormat(16000, "s16", True), ln)
    l = _lib.lib()
    f = model.PcmFormat(16000, "s16")
    dst = np.zeros(1 << 20, np.int16)
    outs = np.zeros(len(utts), np.int64)
    for bad in (_lib.Sbv2Loudness(-80.0, -1.0), _lib.Sbv2Loudness(-16.0, 1.0), _lib.Sbv2Loudness(float("nan"), -1.0)):
        rc = l.sbv2_pipeline_fetch_pcm_loudness(pipe.h, b.ticket, f.c, bad, None, 0, dst.ctypes.data, dst.nbytes, outs.ctypes.data_as(_lib.i64p),
                                                None)
        assert rc != 0 and b"outside" in l.sbv2_last_error()
    pipe.close(); bs.close(); vs.close()


@pytest.mark.gpu
def test_fetch_flac_loudness_decodes_to_the_s16_signals():
    bc, vc, bs, vs = _tiny()
    pipe = model.Pipeline(bs, vs)
    utts = make_utts([12, 30, 5], bc, vc, seed0=533, with_bert=False)
    b = pipe.prepare(utts, sdp_ratio=0.3, noise_scale=0.667, noise_scale_w=0.8, noise_seed=9)
    pipe.run(b)
    lens = [int(n) for n in b.lens]
    place = [0, lens[0] + 22050, lens[0] + lens[1] + 44100]
    joined = place[-1] + lens[2]
    for rate in (16000, 44100, 48000):
        f = model.PcmFormat(rate, "s16")
        for ln in (model.Loudness(-16.0, -1.0), None):
            for pl, jl in ((None, None), (place, joined)):
                pcm, s1 = pipe.fetch_loudness(b, f, ln, pl, jl)
                streams, s2 = pipe.fetch_flac_loudness(b, f, ln, pl, jl)
                assert s1.tobytes() == s2.tobytes()
                assert len(streams) == len(pcm)
                for st, x in zip(streams, pcm):
                    d = R.read(st)
                    assert d["rate"] == rate
                    np.testing.assert_array_equal(d["samples"], x)
    with pytest.raises(model.Sbv2Error, match="s16"):
        pipe.fetch_flac_loudness(b, model.PcmFormat(16000, "f32"), model.Loudness(-16.0))
    pipe.close(); bs.close(); vs.close()


@pytest.mark.gpu
def test_easy_synthesize_loudness_wav_and_flac():
    import scipy.io.wavfile as W
    bc, vc, bs, vs = _tiny()
    pipe = model.Pipeline(bs, vs)
    keys = ("input_ids", "word2ph", "phones", "tones", "langs")
    sent = [{k: synth.make_utterance(n, bc, vc, seed=710 + n)[k] for k in keys} for n in (11, 6, 17)]
    lines = [sent[0], None, sent[1], sent[2]]
    styles = synth.hash_normal(77, 3 * vc["style_dim"]).reshape(3, -1).astype(np.float32)
    rate, x = W.read(io.BytesIO(orchestrator.easy_synthesize(pipe, lines, styles, 1, 0, None, noise_seed=4321)))
    assert rate == 44100 and x.dtype == np.float32
    for sr, enc in ((44100, "f32"), (16000, "s16"), (48000, "flac")):
        opts = orchestrator.SynthesizeOptions(sample_rate=sr, encoding=enc, loudness=-16)
        st = []
        data = orchestrator.easy_synthesize(pipe, lines, styles, 1, 0, opts, noise_seed=4321, loudness_stats=st)
        if enc == "flac":
            d = R.read(data)
            got_rate, sig = d["rate"], d["samples"].astype(np.float64) / 32767
        else:
            got_rate, s = W.read(io.BytesIO(data))
            sig = s.astype(np.float64) / (32767 if enc == "s16" else 1)
        assert got_rate == sr
        y = ref_format(x, sr, "f32", False)   # the request's timeline, silent gaps included
        ref = meter(y, sr, -16.0, -1.0)
        assert len(st) == 1
        close_stats(st[0], ref, what=f"{sr} {enc}")
        L, tp = integrated(sig, sr), true_peak(sig)
        assert abs(L + 16) <= 0.01 or abs(tp + 1) <= 0.01, (sr, enc, L, tp, st)
    opts = orchestrator.SynthesizeOptions(loudness=-16)
    opts.normalize = True   # set after construction: easy_synthesize refuses the pair itself
    with pytest.raises(model.Sbv2Error, match="normalize"):
        orchestrator.easy_synthesize(pipe, lines, styles, 1, 0, opts, noise_seed=1)
    pipe.close(); bs.close(); vs.close()


@pytest.fixture(scope="module")
def full_models():
    bs, vs = model.load_model(blob("bert", "full"), True), model.load_model(blob("vits", "full"), False)
    yield weights("bert", "full")[0], weights("vits", "full")[0], bs, vs
    bs.close(); vs.close()


@pytest.mark.gpu
def test_full_shape_batch_loudness_44k_16k_s16(full_models):
    """The bench-shaped batch (32 x 128 phonemes, 10.4 s each at full model size) at -23 LUFS, s16, against the reference."""
    bc, vc, bs, vs = full_models
    pipe = model.Pipeline(bs, vs)
    utts = [synth.make_utterance(128, bc, vc, seed=i) for i in range(32)]
    b = pipe.prepare(utts, forced=True)
    pipe.run(b)
    native = pipe.fetch(b)
    ln = model.Loudness(-23.0, -1.0)
    for rate in (44100, 16000):
        f = model.PcmFormat(rate, "s16")
        got, stats = pipe.fetch_loudness(b, f, ln)
        for i in (0, 7, 31):
            y = ref_format(native[i], rate, "f32", False)
            _check_loudness(got[i], stats[i], y, rate, "s16", ln, f"{rate} utterance {i}")
            assert stats[i, 0] > -60, stats[i]   # away from the -70 gate
            sig = got[i].astype(np.float64) / 32767
            if stats[i, 0] + stats[i, 2] > -23.0 - 1e-9:   # loudness-limited: the delivered signal reads the target
                assert abs(integrated(sig, rate) + 23) <= 0.01, (rate, i, stats[i])
            else:
                assert abs(true_peak(sig) + 1) <= 0.01, (rate, i, stats[i])
        assert all(g.size == model.pcm_format_length(f, x.size) for g, x in zip(got, native))
    pipe.close()
