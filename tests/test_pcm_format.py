"""Output formats of the PCM (csrc/pcm_format.hip): resampling 44.1 kHz -> common rates, peak normalisation and the s16 quantiser on the device.

The reference here is a numpy restatement of the convention of include/sbv2_hip.h (sbv2_pcm_format):
    y[j] = sum_k h[j M - k L + half] x[k],  j < ceil(N L / M),  x = 0 outside [0, N),
    s16 = clamp(rint(y g 32767), -32767, 32767),  g = 1 / max|y| when normalising (1 for a silent signal),
checked itself against scipy.signal.resample_poly(x, L, M, window = h / L) (an independent implementation of the same indexing).
CPU tests run anywhere; GPU tests (@pytest.mark.gpu) need an MI355X."""
import ctypes
import io
import wave

import numpy as np
import pytest

import sbv2_oracle as O
from helpers import blob, make_utts, weights
from sbv2_api_amd import _lib, model, orchestrator, synth

RATES = (8000, 16000, 22050, 24000, 32000, 44100, 48000)


# ---- the numpy reference ------------------------------------------------------------------------------------------------------------------

def branches(h, L):
    """[L][T] polyphase table: branch p = h[p], h[p + L], ... zero-padded."""
    T = -(-len(h) // L)
    H = np.zeros((L, T))
    for p in range(L):
        v = np.asarray(h[p::L], np.float64)
        H[p, :len(v)] = v
    return H


def ref_resample(x, h, L, M):
    """The convention, in float64: y[j] = sum_t H[p_j][t] x[kmax_j - t]."""
    x = np.asarray(x, np.float64)
    N = len(x)
    J = -(-N * L // M)
    half = (len(h) - 1) // 2
    H = branches(h, L)
    T = H.shape[1]
    j = np.arange(J, dtype=np.int64)
    i0 = j * M + half
    kmax = i0 // L
    p = i0 - kmax * L
    xp = np.concatenate([np.zeros(T), x, np.zeros(T + half // L + 2)])
    y = np.zeros(J)
    for t in range(T):
        y += H[p, t] * xp[kmax - t + T]
    return y


def ref_format(x, rate, encoding, normalize):
    h, L, M = model.pcm_format_taps(rate)
    y = ref_resample(x, h, L, M)
    pk = np.abs(y).max() if y.size else 0.0
    g = 1.0 / pk if normalize and pk > 0 else 1.0
    y = y * g
    if encoding == "s16":
        return np.clip(np.rint(y * 32767.0), -32767, 32767)
    return y


def check_format(got, ref, encoding, what=""):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if got.size == 0:
        return
    if encoding == "f32":
        scale = max(float(np.abs(ref).max()), 1e-30)
        err = float(np.abs(got.astype(np.float64) - ref).max()) / scale
        assert err <= 1e-5, f"{what}: f32 max-abs error {err:.2e} of peak"
    else:
        d = np.abs(got.astype(np.int64) - ref.astype(np.int64))
        assert d.max() <= 1, f"{what}: s16 off by {d.max()} LSB"
        assert (d > 0).mean() < 1e-3, f"{what}: {100 * (d > 0).mean():.3f} % of the samples off by one"


def ceil_len(n, L, M):
    return -(-n * L // M)


# ---- CPU ----------------------------------------------------------------------------------------------------------------------------------

def test_format_length_matches_ceil_and_refuses_bad_formats():
    for r in RATES:
        _, L, M = model.pcm_format_taps(r)
        for enc in ("f32", "s16"):
            f = model.PcmFormat(r, enc)
            for n in (0, 1, 511, 512, 44099, 10 ** 7):
                assert model.pcm_format_length(f, n) == ceil_len(n, L, M), (r, n)
    l = _lib.lib()
    for bad, word in (((44000, 0, 0, 0), "sample rate"), ((96000, 0, 0, 0), "sample rate"), ((16000, 2, 0, 0), "encoding"),
                      ((16000, 0, 2, 0), "normalize"), ((16000, 1, 0, 7), "reserved")):
        assert l.sbv2_pcm_format_length(_lib.Sbv2PcmFormat(*bad), 100) == -1
        assert word in l.sbv2_last_error().decode(), bad
    with pytest.raises(model.Sbv2Error, match="encoding"):
        model.PcmFormat(16000, "s24")
    with pytest.raises(model.Sbv2Error, match="sample rate"):
        model.pcm_format_taps(11025)


@pytest.mark.parametrize("rate", RATES)
def test_filter_branches_response_and_convention(rate):
    import scipy.signal as S
    h, L, M = model.pcm_format_taps(rate)
    hd = h.astype(np.float64)
    if rate == 44100:
        assert (L, M) == (1, 1) and list(h) == [1.0]
        return
    assert len(h) % 2 == 1 and (len(h) - 1) // 2 == 32 * max(L, M)
    assert np.gcd(L, M) == 1 and 44100 * L == rate * M
    sums = branches(hd, L).sum(axis=1)
    assert np.abs(sums - 1).max() <= 1e-6
    w, resp = S.freqz(hd / L, worN=1 << 17, fs=44100 * L)
    db = 20 * np.log10(np.abs(resp) + 1e-300)
    lo = min(44100, rate)
    pb = db[w <= 0.4 * lo]
    assert pb.max() - pb.min() <= 0.01, f"passband ripple {pb.max() - pb.min():.4f} dB"
    assert db[w >= 0.5 * lo].max() <= -80, f"stopband {db[w >= 0.5 * lo].max():.1f} dB"
    x = np.random.default_rng(rate).standard_normal(3001)
    for n in (3001, 700, 1):
        ref = S.resample_poly(x[:n], L, M, window=hd / L)
        got = ref_resample(x[:n], hd, L, M)
        assert got.shape == ref.shape
        assert np.abs(got - ref).max() <= 1e-12


def test_wav_writers_read_back():
    import scipy.io.wavfile as W
    s = (np.random.default_rng(3).integers(-32767, 32768, 4001)).astype(np.int16)
    b = orchestrator.pcm16_wav(s, 16000)
    assert b[:4] == b"RIFF" and b[8:16] == b"WAVEfmt " and len(b) == 44 + 2 * s.size
    with wave.open(io.BytesIO(b)) as wf:
        assert (wf.getframerate(), wf.getsampwidth(), wf.getnchannels(), wf.getnframes()) == (16000, 2, 1, s.size)
        np.testing.assert_array_equal(np.frombuffer(wf.readframes(s.size), "<i2"), s)
    rate, data = W.read(io.BytesIO(b))
    assert rate == 16000 and data.dtype == np.int16
    np.testing.assert_array_equal(data, s)
    f = np.random.default_rng(4).standard_normal(3000).astype(np.float32) * 0.3
    rate, data = W.read(io.BytesIO(orchestrator.float_wav(f, 48000)))
    assert rate == 48000 and data.dtype == np.float32
    np.testing.assert_array_equal(data, f)
    # the default writer is unchanged: array_to_wav == the float writer at 44.1 kHz
    assert orchestrator.array_to_wav(f.reshape(1, 1, -1)) == orchestrator.float_wav(f, 44100)


def test_joined_placement_follows_the_gap_rule():
    place, n = orchestrator.joined_placement([100, 200, 50], [0, 2, 3], 5)
    assert place == [0, 100 + 22050, 100 + 22050 + 200 + 22050] and n == place[-1] + 50 + 22050
    place, n = orchestrator.joined_placement([100, 200], [0, 2], 3)
    assert place == [0, 22150] and n == 22350
    assert orchestrator.joined_placement([100, 200], [0, 1], 2, split_sentences=False) == ([0, 100], 300)


def test_rest_carries_format_fields():
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
            if options.encoding not in ("f32", "s16"):
                raise model.Sbv2Error(f"unsupported PCM encoding {options.encoding!r}")
            return b"RIFF"

    h = Holder()
    c = TestClient(rest.make_app(h))
    assert c.post("/synthesize", json={"text": "a", "ident": "m"}).status_code == 200
    o = h.opts[-1]
    assert (o.sample_rate, o.encoding, o.normalize) == (44100, "f32", False)
    assert c.post("/synthesize", json={"text": "a", "ident": "m", "sample_rate": 16000, "encoding": "s16", "normalize": True}).status_code == 200
    o = h.opts[-1]
    assert (o.sample_rate, o.encoding, o.normalize) == (16000, "s16", True)
    r = c.post("/synthesize", json={"text": "a", "ident": "m", "encoding": "u8"})
    assert r.status_code == 500 and r.text.startswith("Something went wrong: ")
    d = orchestrator.SynthesizeOptions()
    assert (d.sample_rate, d.encoding, d.normalize) == (44100, "f32", False)


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------------

def _tiny():
    bc, _ = weights("bert", "tiny", 3)
    vc, _ = weights("vits", "tiny", 5)
    bs, vs = model.load_model(blob("bert", "tiny", 3), True), model.load_model(blob("vits", "tiny", 5), False)
    return bc, vc, bs, vs


@pytest.mark.gpu
def test_fetch_format_every_rate_encoding_normalize():
    bc, vc, bs, vs = _tiny()
    pipe = model.Pipeline(bs, vs)
    utts = make_utts([9, 1, 23, 14, 40], bc, vc, seed0=401, with_bert=False)
    b = pipe.prepare(utts, forced=True)
    pipe.run(b)
    native = pipe.fetch(b)
    lens = [len(x) for x in native]
    assert min(lens) < 353 and any(n % 441 for n in lens)    # one utterance shorter than the widest filter span; lengths not multiples of M
    # joined timeline with gaps (one of them shorter than a filter span), utterances out of order
    place = [5000, 0, 5000 + lens[0] + 40, 20000, 20000 + lens[3] + 3000]
    joined = place[-1] + lens[4] + 777
    timeline = np.zeros(joined, np.float32)
    for p, x in zip(place, native):
        timeline[p:p + len(x)] = x
    for rate in RATES:
        for enc in ("f32", "s16"):
            for norm in (False, True):
                f = model.PcmFormat(rate, enc, norm)
                got = pipe.fetch_format(b, f)
                assert len(got) == len(utts)
                for i, (g, x) in enumerate(zip(got, native)):
                    assert g.dtype == f.dtype
                    ref = ref_format(x, rate, enc, norm)
                    check_format(g, ref, enc, f"{f} utterance {i}")
                    if norm and enc == "s16" and g.size:
                        assert np.abs(g.astype(np.int64)).max() == 32767
                gj = pipe.fetch_format(b, f, place, joined)
                assert len(gj) == 1
                check_format(gj[0], ref_format(timeline, rate, enc, norm), enc, f"{f} joined")
                if norm and enc == "s16":
                    assert np.abs(gj[0].astype(np.int64)).max() == 32767
    # bad placements are refused
    for bad in ([0, 0, 5000, 20000, 30000], [-1] + place[1:], place[:-1] + [joined - lens[4] + 1]):
        with pytest.raises(model.Sbv2Error, match="overlap|outside"):
            pipe.fetch_format(b, model.PcmFormat(16000, "s16"), bad, joined)
    pipe.close(); bs.close(); vs.close()


@pytest.mark.gpu
def test_fetch_format_identity_repeatability_capacity():
    bc, vc, bs, vs = _tiny()
    pipe = model.Pipeline(bs, vs)
    utts = make_utts([12, 30, 5], bc, vc, seed0=433, with_bert=False)
    b = pipe.prepare(utts, sdp_ratio=0.3, noise_scale=0.667, noise_scale_w=0.8, noise_seed=9)
    pipe.run(b)
    native = np.concatenate(pipe.fetch(b))
    ident = np.concatenate(pipe.fetch_format(b, model.PcmFormat(44100, "f32", False)))
    assert ident.tobytes() == native.tobytes()
    for f in (model.PcmFormat(16000, "s16", True), model.PcmFormat(48000, "f32", True), model.PcmFormat(8000, "s16", False)):
        a = np.concatenate(pipe.fetch_format(b, f))
        c = np.concatenate(pipe.fetch_format(b, f))
        assert a.tobytes() == c.tobytes(), f
    # a destination one sample short is refused and left untouched
    l = _lib.lib()
    f = model.PcmFormat(16000, "s16")
    n = sum(model.pcm_format_length(f, x) for x in b.lens)
    dst = np.full(n, 1234, np.int16)
    outs = np.full(3, -5, np.int64)
    rc = l.sbv2_pipeline_fetch_pcm_format(pipe.h, b.ticket, f.c, None, 0, dst.ctypes.data, dst.nbytes - 2, outs.ctypes.data_as(_lib.i64p))
    assert rc != 0 and b"too small" in l.sbv2_last_error()
    assert (dst == 1234).all() and (outs == -5).all()
    pipe.close(); bs.close(); vs.close()


def _stream_all(bs, vs, u, chunk, fmt, **kw):
    st = model.StreamHandle(bs, vs, u, chunk, fmt=fmt, **kw)
    parts = []
    while True:
        c = st.next()
        if c is None:
            break
        parts.append(c)
    total = st.total_samples
    st.close()
    return np.concatenate(parts), total


@pytest.mark.gpu
def test_stream_format_tiny_equals_whole_bit_for_bit():
    """On the tiny decoder the streamed native PCM equals the whole-utterance PCM bit for bit (test_gpu_parity), so the formatted chunks do too.
    The tiny generator's halo leaves ~70 exact samples past a chunk edge: 48 / 24 kHz filters fit, the 16 kHz one is refused."""
    bc, vc, bs, vs = _tiny()
    pipe = model.Pipeline(bs, vs)
    for n, kw in ((40, dict(forced=True)), (23, dict(sdp_ratio=0.2, noise_scale=0.667, noise_scale_w=0.8, noise_seed=5))):
        u = make_utts([n], bc, vc, seed0=171 + n, with_bert=False)[0]
        b = pipe.prepare([u], **kw)
        pipe.run(b)
        fmts = (model.PcmFormat(48000, "s16"), model.PcmFormat(48000, "f32"), model.PcmFormat(24000, "s16"), model.PcmFormat(44100, "f32"))
        wholes = [pipe.fetch_format(b, f)[0] for f in fmts]   # (a stream reuses the handles' context: fetch the run's results first)
        for f, whole in zip(fmts, wholes):
            for chunk in (16, 50, 64):
                got, total = _stream_all(bs, vs, u, chunk, f, **kw)
                assert total == whole.size == got.size, (f, chunk)
                assert got.dtype == whole.dtype
                np.testing.assert_array_equal(got, whole, err_msg=f"{f} chunk {chunk}")
        with pytest.raises(model.Sbv2Error, match="halo"):
            model.StreamHandle(bs, vs, u, 16, fmt=model.PcmFormat(16000, "s16"), **kw)
    u = make_utts([20], bc, vc, seed0=7, with_bert=False)[0]
    with pytest.raises(model.Sbv2Error, match="normali"):
        model.StreamHandle(bs, vs, u, 16, fmt=model.PcmFormat(48000, "s16", True), forced=True)
    # the plain next is refused on a formatted stream
    st = model.StreamHandle(bs, vs, u, 16, fmt=model.PcmFormat(48000, "s16"), forced=True)
    n = ctypes.c_int64()
    assert _lib.lib().sbv2_stream_next(st.h, st.buf.ctypes.data, st.buf.size, ctypes.byref(n)) != 0
    assert b"sbv2_stream_next_format" in _lib.lib().sbv2_last_error()
    st.close()
    pipe.close(); bs.close(); vs.close()


@pytest.mark.gpu
def test_easy_synthesize_s16_16k_equals_oracle_of_default_wav():
    import scipy.io.wavfile as W
    bc, vc, bs, vs = _tiny()
    pipe = model.Pipeline(bs, vs)
    keys = ("input_ids", "word2ph", "phones", "tones", "langs")
    sent = [{k: synth.make_utterance(n, bc, vc, seed=610 + n)[k] for k in keys} for n in (11, 6, 17)]
    lines = [sent[0], None, sent[1], sent[2]]
    styles = synth.hash_normal(77, 3 * vc["style_dim"]).reshape(3, -1).astype(np.float32)
    base = orchestrator.easy_synthesize(pipe, lines, styles, 1, 0, None, noise_seed=1234)
    rate, x = W.read(io.BytesIO(base))
    assert rate == 44100 and x.dtype == np.float32
    opts = orchestrator.SynthesizeOptions(sample_rate=16000, encoding="s16")
    wav = orchestrator.easy_synthesize(pipe, lines, styles, 1, 0, opts, noise_seed=1234)
    rate, y = W.read(io.BytesIO(wav))
    assert rate == 16000 and y.dtype == np.int16 and len(wav) == 44 + 2 * y.size
    check_format(y, ref_format(x, 16000, "s16", False), "s16", "easy_synthesize 16 kHz s16")
    opts = orchestrator.SynthesizeOptions(sample_rate=48000, encoding="f32", normalize=True)
    rate, z = W.read(io.BytesIO(orchestrator.easy_synthesize(pipe, lines, styles, 1, 0, opts, noise_seed=1234)))
    assert rate == 48000 and z.dtype == np.float32
    check_format(z, ref_format(x, 48000, "f32", True), "f32", "easy_synthesize 48 kHz f32 normalised")
    with pytest.raises(model.Sbv2Error, match="sample rate"):
        orchestrator.easy_synthesize(pipe, lines, styles, 1, 0, orchestrator.SynthesizeOptions(sample_rate=12345), noise_seed=1)
    pipe.close(); bs.close(); vs.close()


@pytest.fixture(scope="module")
def full_models():
    bs, vs = model.load_model(blob("bert", "full"), True), model.load_model(blob("vits", "full"), False)
    yield weights("bert", "full")[0], weights("vits", "full")[0], bs, vs
    bs.close(); vs.close()


@pytest.mark.gpu
def test_full_shape_batch_16k_s16(full_models):
    """The bench-shaped batch (32 x 128 phonemes, 10.4 s each at full model size) formatted at 16 kHz s16 against the reference."""
    bc, vc, bs, vs = full_models
    pipe = model.Pipeline(bs, vs)
    utts = [synth.make_utterance(128, bc, vc, seed=i) for i in range(32)]
    b = pipe.prepare(utts, forced=True)
    pipe.run(b)
    native = pipe.fetch(b)
    f = model.PcmFormat(16000, "s16")
    got = pipe.fetch_format(b, f)
    for i in (0, 7, 31):
        check_format(got[i], ref_format(native[i], 16000, "s16", False), "s16", f"utterance {i}")
    assert all(g.size == model.pcm_format_length(f, x.size) for g, x in zip(got, native))
    pipe.close()


@pytest.mark.gpu
def test_full_model_stream_16k_48k_s16(full_models):
    """Full-size decoder: the streamed chunks at 16 and 48 kHz s16 equal the formatted whole utterance within +-1 LSB (the streamed native PCM
    agrees with the whole-sequence PCM to f32 rounding at this size)."""
    bc, vc, bs, vs = full_models
    pipe = model.Pipeline(bs, vs)
    u = synth.make_utterance(60, bc, vc, seed=91)
    b = pipe.prepare([u], forced=True)
    pipe.run(b)
    fmts = (model.PcmFormat(16000, "s16"), model.PcmFormat(48000, "s16"), model.PcmFormat(8000, "f32"))
    wholes = [pipe.fetch_format(b, f)[0] for f in fmts]   # (a stream reuses the handles' context: fetch the run's results first)
    for f, whole in zip(fmts, wholes):
        for chunk in (64, 100):
            got, total = _stream_all(bs, vs, u, chunk, f, forced=True)
            assert total == whole.size == got.size
            if f.encoding == "s16":
                assert np.abs(got.astype(np.int64) - whole).max() <= 1, (f, chunk)
            else:
                np.testing.assert_allclose(got, whole, atol=1e-5, rtol=0)
    pipe.close()
