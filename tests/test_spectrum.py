"""The spectrum of a delivered signal (struct sbv2_spectrum, csrc/spectrum.hip): the mel bank and every refusal on the host, the stage against a
plain float64 restatement of the definition in include/sbv2_hip.h on the GPU, and the request fetch that carries it.

The error of a case is E = max over frames of max_band |B_dev - B_ref| / max_band B_ref, B_ref the float64 restatement; the yardstick is E32, the
same quantity for a numpy float32 restatement (f32 operands, f32 matmul), computed here on the CPU.  Required: E <= 4 E32 (the operands carry 22
mantissa bits where f32 carries 24; the margin is what is left for the f32 accumulation order of the matrix cores)."""
import base64
import ctypes as C
import functools
import inspect
import re
import os

import numpy as np
import pytest

import flac_reader as R
from helpers import blob, make_utts, weights
from sbv2_api_amd import _lib, batcher, model, orchestrator
from test_formant import REQUEST, STYLES, FormantPipe, TokenPipe, _payload

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = {"sbv2_pipeline_fetch_request_spectrum": 16, "sbv2_spectrum_bands": 3, "sbv2_debug_spectrum": 6}


# ---- the float64 restatement -----------------------------------------------------------------------------------------------------------------
def mel_bank_ref(sr, n_fft, n_mels, f_min, f_max):
    step = np.log(6.4) / 27.0
    mel = lambda f: 15.0 + np.log(f / 1000.0) / step if f >= 1000.0 else f / (200.0 / 3.0)
    hz = lambda m: 1000.0 * np.exp(step * (m - 15.0)) if m >= 15.0 else (200.0 / 3.0) * m
    m0, m1 = mel(f_min), mel(f_max)
    e = np.array([hz(m0 + (m1 - m0) * i / (n_mels + 1)) for i in range(n_mels + 2)])
    f = np.arange(n_fft // 2 + 1, dtype=np.float64) * sr / n_fft
    up = (f[None, :] - e[:-2, None]) / (e[1:-1] - e[:-2])[:, None]
    down = (e[2:, None] - f[None, :]) / (e[2:] - e[1:-1])[:, None]
    return np.maximum(0.0, np.minimum(up, down)) * (2.0 / (e[2:] - e[:-2]))[:, None]


@functools.lru_cache(maxsize=None)
def basis(n_fft):
    r = np.outer(np.arange(n_fft), np.arange(n_fft // 2 + 1)) % n_fft
    return np.cos(2.0 * np.pi * r / n_fft), np.sin(2.0 * np.pi * r / n_fft), (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft) / n_fft)).astype(np.float32)


def spectrum_ref(u, sr, n_fft, hop, n_mels, f_min, f_max):
    """(B in float64, B of the float32 restatement) of u (float32 values, already divided by 32768 for the integer encodings)."""
    cs, sn, w = basis(n_fft)
    nf = -(-len(u) // hop) if len(u) else 0
    padded = np.concatenate([np.zeros(n_fft, np.float32), u, np.zeros(n_fft + hop, np.float32)])
    idx = (np.arange(nf) * hop + hop // 2 - n_fft // 2 + n_fft)[:, None] + np.arange(n_fft)[None, :]
    a = padded[idx] * w[None, :]                                                 # f32, one rounding
    a64 = a.astype(np.float64)
    p = (a64 @ cs) ** 2 + (a64 @ sn) ** 2
    p32 = (a @ cs.astype(np.float32)) ** 2 + (a @ sn.astype(np.float32)) ** 2
    if n_mels == 0:
        return p, p32
    bank = mel_bank_ref(sr, n_fft, n_mels, f_min, f_max).astype(np.float32)
    return p @ bank.astype(np.float64).T, p32 @ bank.T


def worst(got, ref):
    """E, over the frames that hold anything; a frame of zeros must be zeros."""
    top = ref.max(axis=1) if ref.size else np.zeros(0)
    assert (got[top == 0] == 0).all()
    live = top > 0
    return float((np.abs(got[live] - ref[live]).max(axis=1) / top[live]).max()) if live.any() else 0.0


# ---- host only -----------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_exported_and_declared():
    header = open(os.path.join(ROOT, "include", "sbv2_hip.h")).read()
    for name, nargs in NEW_SYMBOLS.items():
        assert name in _lib.SYMBOLS and len(_lib.SYMBOLS[name][1]) == nargs
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert decl and decl.group(1).count(",") + 1 == nargs
        assert getattr(_lib.lib(), name)


BANKS = [(16000, 400, 80, 0.0, 8000.0), (44100, 1024, 128, 50.0, 16000.0), (8000, 64, 1, 0.0, 4000.0), (16000, 64, 128, 0.0, 8000.0)]


@pytest.mark.parametrize("sr,n_fft,n_mels,f_min,f_max", BANKS)
def test_the_bank_is_the_float64_bank_rounded(sr, n_fft, n_mels, f_min, f_max):
    n_bands, bank = model.spectrum_bands(sr, model.Spectrum(n_fft, n_fft, n_mels, f_min, f_max))
    want = mel_bank_ref(sr, n_fft, n_mels, f_min, f_max).astype(np.float32)
    assert n_bands == n_mels and bank.shape == want.shape and bank.tobytes() == want.tobytes()
    empty = int((bank.max(axis=1) == 0).sum())
    print(f"[spectrum] bank {sr} {n_fft} {n_mels}: {empty} empty triangles")
    assert (empty > 0) == (n_fft == 64 and n_mels == 128)                        # 128 bands over 33 bins: some triangles hold no bin
    assert model.spectrum_bands(sr, model.Spectrum(n_fft, 1, 0)) == (n_fft // 2 + 1, None)


def test_refusals_that_need_no_run():
    l = _lib.lib()
    ok = dict(n_fft=400, hop=160, n_mels=80, reserved=0, f_min=0.0, f_max=8000.0)
    nan = float("nan")
    bad = [("n_fft", 32), ("n_fft", 2080), ("n_fft", 408), ("hop", 0), ("hop", 401), ("n_mels", -1), ("n_mels", 129), ("f_min", -1.0),
           ("f_min", 8000.0), ("f_max", 8000.5), ("f_min", nan), ("f_max", nan), ("reserved", 1)]
    power = np.full(8, 7.0, np.float32)

    def struct(capacity=8, ptr=True, **kw):
        v = dict(ok, **kw)
        return _lib.Sbv2Spectrum(v["n_fft"], v["hop"], v["n_mels"], v["reserved"], v["f_min"], v["f_max"], capacity,
                                 power.ctypes.data_as(_lib.f32p) if ptr else None, -3, -3)

    x = np.zeros(100, np.int16)
    for field, value in bad:
        for call in (lambda c: l.sbv2_spectrum_bands(16000, C.byref(c), None),
                     lambda c: l.sbv2_debug_spectrum(0, x.ctypes.data, 1, x.size, 16000, C.byref(c))):
            c = struct(**{field: value})
            assert call(c) == 1, (field, value)
            assert field in l.sbv2_last_error().decode() and (c.n_frames, c.n_bands) == (-3, -3)
    for sr in (0, 48001):
        assert l.sbv2_spectrum_bands(sr, C.byref(struct(f_max=1.0)), None) == 1 and "sample rate" in l.sbv2_last_error().decode()
    # what the hook checks before it touches a device: capacity (1 frame of 80 bands here) and the array
    assert l.sbv2_debug_spectrum(0, x.ctypes.data, 1, x.size, 16000, C.byref(struct(capacity=79))) == 1 and "too small" in l.sbv2_last_error().decode()
    assert l.sbv2_debug_spectrum(0, x.ctypes.data, 1, x.size, 16000, C.byref(struct(capacity=80, ptr=False))) == 1
    assert "power must not be NULL" in l.sbv2_last_error().decode() and (power == 7.0).all()
    c = struct()
    assert l.sbv2_spectrum_bands(16000, C.byref(c), None) == 0 and c.n_bands == 80
    assert "spectrum" in inspect.signature(model.Pipeline.fetch_request).parameters
    assert model._fetch_fields() == ["signal", "stats"] and model._fetch_fields(spectrum=True) == ["signal", "stats", "spectrum"]


class SpecPipe(FormantPipe):
    """FormantPipe whose fetch_request knows spectrum: power[f][m] = f + m / 1000 for 3 frames (so the marks tell what was fetched)."""

    def fetch_request(self, b, rows, fmt, place, joined_len, spectrum=None, **kw):
        res = super().fetch_request(b, rows, fmt, place, joined_len, **kw)
        self.calls[-1]["spectrum"] = None if spectrum is None else (spectrum.n_fft, spectrum.hop, spectrum.n_mels, spectrum.f_min, spectrum.f_max)
        if spectrum is None:
            return res
        nb = spectrum.n_bands()
        spectrum.power = (np.arange(3)[:, None] + np.arange(nb)[None, :] / 1000.0).astype(np.float32)
        spectrum.used_f_max = fmt.sample_rate / 2.0 if spectrum.f_max is None else spectrum.f_max
        return tuple(res) + (spectrum,)


def test_routes_carry_or_refuse_the_spectrum():
    SO = orchestrator.SynthesizeOptions
    pipe = SpecPipe()
    plain = orchestrator.easy_synthesize(pipe, REQUEST, STYLES, noise_seed=1)
    _, mk0 = orchestrator.easy_synthesize_marks(pipe, REQUEST, STYLES, noise_seed=1)
    assert "spectrum" not in mk0 and pipe.calls[-1]["spectrum"] is None
    wav, mk = orchestrator.easy_synthesize_marks(pipe, REQUEST, STYLES, noise_seed=1, options=SO(spectrum_mels=80, sample_rate=16000, encoding="s16"))
    assert pipe.calls[-1]["spectrum"] == (416, 160, 80, 0.0, None)              # the defaults: 10 ms, the multiple of 32 nearest to 25 ms (a tie goes up)
    s = mk["spectrum"]
    assert {k: s[k] for k in ("n_fft", "hop", "n_bands", "f_min", "f_max", "shape")} == dict(n_fft=416, hop=160, n_bands=80, f_min=0.0, f_max=8000.0,
                                                                                             shape=[3, 80])
    db = np.frombuffer(base64.b64decode(s["db"]), "<f4").reshape(3, 80)
    want = 10.0 * np.log10(np.maximum((np.arange(3)[:, None] + np.arange(80)[None, :] / 1000.0).astype(np.float32).astype(np.float64), 1e-10))
    assert db.tobytes() == want.astype("<f4").tobytes() and db[0, 0] == -100.0
    _, mk = orchestrator.easy_synthesize_marks(pipe, REQUEST, STYLES, noise_seed=1,
                                               options=SO(spectrum_mels=0, spectrum_fft=400, spectrum_hop=100, spectrum_fmin=50.0, spectrum_fmax=9000.0))
    assert pipe.calls[-1]["spectrum"] == (400, 100, 0, 50.0, 9000.0) and mk["spectrum"]["shape"] == [3, 201]
    assert {k: v for k, v in mk.items() if k != "spectrum"} == mk0
    # bad values and fields without spectrum_mels: refused before any run
    runs = pipe.runs
    for kw in (dict(spectrum_mels=129), dict(spectrum_mels=80, spectrum_fft=408), dict(spectrum_mels=80, spectrum_hop=0),
               dict(spectrum_mels=80, spectrum_fmax=30000.0), dict(spectrum_mels=80, spectrum_fmin=float("nan"))):
        with pytest.raises(orchestrator.SpectrumError, match="spectrum"):
            orchestrator.easy_synthesize_marks(pipe, REQUEST, STYLES, noise_seed=1, options=SO(**kw))
    for kw in (dict(spectrum_fft=400), dict(spectrum_hop=160), dict(spectrum_fmin=50.0), dict(spectrum_fmax=4000.0), dict(spectrum_mels=True),
               dict(spectrum_mels=80, spectrum_fft=400.5)):
        with pytest.raises(orchestrator.SpectrumError, match="spectrum_"):
            SO(**kw)
    # every route without marks refuses and names the one that carries it
    with pytest.raises(orchestrator.SpectrumError, match="/synthesize_marks"):
        orchestrator.easy_synthesize(pipe, REQUEST, STYLES, noise_seed=1, options=SO(spectrum_mels=80))
    for kw in (dict(), dict(split=True), dict(levels=True)):
        with pytest.raises(orchestrator.SpectrumError, match="/synthesize_marks"):
            orchestrator.easy_synthesize_stream(None, None, REQUEST[:1], STYLES, options=SO(spectrum_mels=80), **kw)
    # a pipeline from before the option: refused, never served without
    old = TokenPipe()
    with pytest.raises(model.Sbv2Error, match="spectrum_mels needs a pipeline"):
        orchestrator.easy_synthesize_marks(old, REQUEST, STYLES, noise_seed=1, options=SO(spectrum_mels=80))
    assert pipe.runs == runs and old.runs == 0
    # the batcher: per request, with marks only
    rb = batcher.RequestBatcher(pipe, start=False, clock=lambda: 0.0, max_wait_ms=1000.0)
    f0 = rb.submit(REQUEST, STYLES, options=SO(spectrum_mels=40), noise_seed=1, marks=True)
    f1 = rb.submit(REQUEST, STYLES, options=SO(spectrum_mels=40), noise_seed=1)
    f2 = rb.submit(REQUEST, STYLES, noise_seed=1, marks=True)
    rb.start()
    rb.close()
    assert f0.result(0)[1]["spectrum"]["shape"] == [3, 40] and f0.result(0)[1]["spectrum"]["n_fft"] == 1088 and f2.result(0)[1] == mk0
    assert _payload(f0.result(0)[0]).tobytes() == _payload(plain).tobytes()
    with pytest.raises(orchestrator.SpectrumError, match="/synthesize_marks"):
        f1.result(0)


def test_rest_carries_the_fields_on_synthesize_marks_and_answers_400_elsewhere():
    pytest.importorskip("fastapi")
    from concurrent.futures import Future
    from fastapi.testclient import TestClient
    from sbv2_api_amd import rest
    wav = orchestrator.array_to_wav(np.zeros((1, 1, 10), np.float32))
    seen = []

    class H:
        def easy_synthesize(self, ident, text, style_id, speaker_id, options):
            orchestrator.refuse_spectrum(options, "easy_synthesize (/synthesize)")
            return wav

        def easy_synthesize_batched(self, ident, text, style_id, speaker_id, options, batching=None, marks=False):
            f = Future()
            try:
                if not marks:
                    orchestrator.refuse_spectrum(options, "a request without marks (/synthesize)")
                seen.append(orchestrator.spectrum_options(options, options.sample_rate))
                f.set_result((wav, {"sample_rate": 44100, "tokens": [], "words": []}) if marks else wav)
            except Exception as e:
                f.set_exception(e)
            return f

        def easy_synthesize_marks(self, ident, text, style_id, speaker_id, options):
            seen.append(orchestrator.spectrum_options(options, options.sample_rate))
            return wav, {"sample_rate": 44100, "tokens": [], "words": []}

        def easy_synthesize_stream(self, ident, text, style_id, speaker_id, options, **kw):
            raise AssertionError("a stream with a spectrum must be refused before the holder is asked")

    body = {"text": "x", "ident": "m", "spectrum_mels": 80, "spectrum_fft": 400, "spectrum_hop": 160, "sample_rate": 16000, "encoding": "s16"}
    for c in (TestClient(rest.make_app(H()), raise_server_exceptions=False), TestClient(rest.make_app(H(), batching={}), raise_server_exceptions=False)):
        assert c.post("/synthesize_marks", json=body).status_code == 200
        assert (seen[-1].n_fft, seen[-1].hop, seen[-1].n_mels, seen[-1].f_min, seen[-1].f_max) == (400, 160, 80, 0.0, None)
        assert c.post("/synthesize_marks", json={"text": "x", "ident": "m"}).status_code == 200 and seen[-1] is None
        r = c.post("/synthesize_marks", json=dict(body, spectrum_fft=408))
        assert r.status_code == 400 and "n_fft" in r.text
        for route in ("/synthesize", "/synthesize_stream", "/synthesize_stream_marks"):
            for b in (body, {"text": "x", "ident": "m", "spectrum_hop": 160}):
                r = c.post(route, json=b)
                assert r.status_code == 400 and "spectrum" in r.text and "/synthesize_marks" in r.text, (route, r.status_code, r.text)
        assert c.post("/synthesize", json={"text": "x", "ident": "m"}).content == wav


# ---- the stage against float64 ---------------------------------------------------------------------------------------------------------------
def make_signal(kind, n, n_fft, seed):
    rng = np.random.default_rng(seed)
    if kind == "impulse":
        u = np.zeros(n, np.float32)
        u[min(n - 1, n_fft // 2 + 37)] = 0.75
        return u
    if kind == "sine":                                                           # the centre of bin n_fft / 8
        return (0.5 * np.sin(2.0 * np.pi * np.arange(n) / 8.0 + 0.3)).astype(np.float32)
    if kind == "zeros":
        return np.zeros(n, np.float32)
    return (10.0 ** (float(kind) / 20.0) * np.sqrt(3.0) * rng.uniform(-1.0, 1.0, n)).astype(np.float32)   # noise at `kind` dBFS (RMS)


WIDE = 128 * 256   # frames above which the stage takes its 128-frame tiles (spectrum.h)
# (sr, n_fft, hop, n_mels, encoding, n, signal)
CASES = ([(8000, 64, 1, m, "f32", n, "-6") for m, n in ((0, 31), (1, 32), (0, 33), (80, 127), (0, 128), (128, 129))] +      # tiles of 32: tails
         [(8000, 64, 1, 0, "s16", WIDE, "-6"), (8000, 64, 1, 80, "f32", WIDE + 1, "-6"), (8000, 64, 1, 0, "mulaw", WIDE + 128, "-6"),
          (8000, 64, 1, 80, "s16", WIDE + 127, "-6"),
          (8000, 64, 1, 128, "f32", WIDE + 129, "sine")] +                                                                   # tiles of 128: tails
         [(16000, 400, 160, 80, "s16", 5000, "-6"), (16000, 400, 160, 0, "f32", 5000, "impulse"), (16000, 400, 400, 80, "f32", 5000, "-70"),
          (16000, 400, 160, 128, "mulaw", 4000, "-6"), (16000, 400, 160, 0, "f32", 4000, "sine"), (16000, 400, 1, 80, "s16", 300, "-70")] +
         [(44100, 2048, 160, 128, "f32", 3000, "-6"), (44100, 2048, 2048, 0, "s16", 9000, "-6"), (44100, 2048, 160, 0, "f32", 3000, "impulse"),
          (44100, 2048, 1, 1, "f32", 40, "sine"), (44100, 2048, 160, 80, "f32", 3000, "-70")] +
         [(16000, 400, 160, 80, "f32", 150, "-6"), (16000, 400, 160, 0, "s16", 1, "-6"), (16000, 400, 160, 80, "f32", 0, "-6"),
          (16000, 400, 160, 80, "f32", 3000, "zeros"), (8000, 64, 64, 0, "s16", 700, "zeros")])


@gpu
@pytest.mark.parametrize("sr,n_fft,hop,n_mels,encoding,n,kind", CASES)
def test_stage_against_float64(sr, n_fft, hop, n_mels, encoding, n, kind):
    u = make_signal(kind, n, n_fft, seed=n_fft + n)
    if encoding == "f32":
        x, enc = u, None
    else:
        x = np.clip(np.rint(u * 32768.0), -32768, 32767).astype(np.int16)
        if encoding == "mulaw":
            x = model.g711_encode(x, "mulaw")
        enc = "mulaw" if encoding == "mulaw" else None
        u = (model.g711_decode(x, "mulaw") if encoding == "mulaw" else x).astype(np.float32) / np.float32(32768.0)
    sp = model.debug_spectrum(x, sr, model.Spectrum(n_fft, hop, n_mels, 0.0, None), encoding=enc)
    ref, ref32 = spectrum_ref(u, sr, n_fft, hop, n_mels, 0.0, sr / 2.0)
    assert sp.power.dtype == np.float32 and sp.power.shape == ref.shape == (-(-n // hop), n_mels or n_fft // 2 + 1)
    assert np.isfinite(sp.power).all() and (sp.power >= 0).all()
    e, e32 = worst(sp.power.astype(np.float64), ref), worst(ref32.astype(np.float64), ref)
    print(f"[spectrum] sr={sr} n_fft={n_fft} hop={hop} mels={n_mels} {encoding} n={n} {kind}: E={e:.3e} E32={e32:.3e} E/E32={e / e32 if e32 else 0.0:.2f}")
    if kind == "zeros":
        assert not sp.power.any()
    assert e <= 4.0 * e32
    again = model.debug_spectrum(x, sr, model.Spectrum(n_fft, hop, n_mels, 0.0, None), encoding=enc)
    assert again.power.tobytes() == sp.power.tobytes()


# ---- through the pipeline ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def request_rows():
    bc, _ = weights("bert", "tiny", 3)
    vc, _ = weights("vits", "tiny", 5)
    bs, vs = model.load_model(blob("bert", "tiny", 3), True), model.load_model(blob("vits", "tiny", 5), False)
    pipe = model.Pipeline(bs, vs)
    b = pipe.prepare(make_utts([9, 1, 23, 14], bc, vc, seed0=501, with_bert=False), forced=True)
    lens = pipe.run(b)
    rows, place = [3, 1], [1000, 1000 + int(lens[3]) + 4410]
    yield pipe, b, rows, place, place[1] + int(lens[1]) + 333
    pipe.close(); bs.close(); vs.close()


FORMS = [("f32", 44100, False, 2048, 0), ("s16", 16000, False, 400, 80), ("mulaw", 8000, False, 192, 40), ("s16", 16000, True, 400, 80)]


@gpu
@pytest.mark.parametrize("encoding,rate,flac,n_fft,n_mels", FORMS, ids=["f32-44k", "s16-16k", "mulaw-8k", "flac-16k"])
def test_pipeline_spectrum(request_rows, encoding, rate, flac, n_fft, n_mels):
    pipe, b, rows, place, joined = request_rows
    fmt, hop = model.PcmFormat(rate, encoding), rate // 100
    kw = dict(gain=model.Loudness(-23.0, -1.0), flac=flac, marks=True, env_hop=hop, pitch=model.Pitch(hop))
    plain, pstats, pm, pp = pipe.fetch_request(b, rows, fmt, place, joined, **kw)
    plain = plain if flac else plain.copy()
    pf0 = pp.f0.copy()
    out, stats, m, p, sp = pipe.fetch_request(b, rows, fmt, place, joined, spectrum=model.Spectrum(n_fft, hop, n_mels), **kw)
    assert (out == plain) if flac else (out.dtype == plain.dtype and out.tobytes() == plain.tobytes())
    assert stats.tobytes() == pstats.tobytes() and p.f0.tobytes() == pf0.tobytes()
    for x, y in zip(pm.arrays(), m.arrays()):
        assert x.tobytes() == y.tobytes()
    samples = np.asarray(R.read(out)["samples"], np.int16) if flac else out
    nf = -(-model.pcm_format_length(fmt, joined) // hop)
    assert sp.power.shape == (nf, n_mels or n_fft // 2 + 1) and sp.power.max() > 0
    hook = model.debug_spectrum(samples, rate, model.Spectrum(n_fft, hop, n_mels), encoding=encoding if encoding == "mulaw" else None)
    assert hook.power.tobytes() == sp.power.tobytes()                            # the hook on the fetched samples
    out2, _, sp2 = pipe.fetch_request(b, rows, fmt, place, joined, gain=kw["gain"], flac=flac, spectrum=model.Spectrum(n_fft, hop, n_mels))
    assert ((out2 == plain) if flac else out2.tobytes() == plain.tobytes()) and sp2.power.tobytes() == sp.power.tobytes()   # a second fetch


@gpu
def test_the_formant_symbol_is_the_new_one_with_null_and_refusals_write_nothing(request_rows):
    pipe, b, rows, place, joined = request_rows
    l, fmt = _lib.lib(), model.PcmFormat(16000, "s16")
    rw, pl = np.asarray(rows, np.int32), np.asarray(place, np.int64)
    req = _lib.Sbv2FetchRequest(rw.ctypes.data_as(C.POINTER(C.c_int32)), len(rw), pl.ctypes.data_as(_lib.i64p), joined, C.pointer(fmt.c), None, None, 0)
    n = model.pcm_format_length(fmt, joined)

    def raw(fn, *tail):
        dst, got = np.full(n + 8, 77, np.int16), C.c_int64(-5)
        rc = fn(pipe.h, b.ticket, C.byref(req), None, None, None, None, None, dst.ctypes.data, dst.nbytes, C.byref(got), None, None, None, None, *tail)
        return rc, dst.tobytes(), got.value

    parent = raw(l.sbv2_pipeline_fetch_request_formant)
    assert parent[0] == 0 and parent[2] == n and raw(l.sbv2_pipeline_fetch_request_spectrum, None) == parent
    power = np.full(10, 7.0, np.float32)
    for kw, word in ((dict(n_fft=408), "n_fft"), (dict(f_max=8001.0), "f_max"), (dict(reserved=1), "reserved"), (dict(), "too small")):
        v = dict(dict(n_fft=400, hop=160, n_mels=80, reserved=0, f_max=8000.0), **kw)
        c = _lib.Sbv2Spectrum(v["n_fft"], v["hop"], v["n_mels"], v["reserved"], 0.0, v["f_max"], 10, power.ctypes.data_as(_lib.f32p), -3, -3)
        rc, dst, got = raw(l.sbv2_pipeline_fetch_request_spectrum, C.byref(c))
        assert rc == 1 and word in l.sbv2_last_error().decode() and got == -5 and dst == np.full(n + 8, 77, np.int16).tobytes()
        assert (power == 7.0).all() and (c.n_frames, c.n_bands) == (-3, -3)
    assert raw(l.sbv2_pipeline_fetch_request_formant) == parent                  # the ticket is still there
