"""Formant contour (sbv2_formant_contour and its three entry points; k_formant_lpc of csrc/formants.hip): the definition restated in numpy and
judged as a formant tracker, the host-side checks and defaults, the orchestrator / batcher / REST contracts against fakes (CPU); the kernel
against that restatement and against numpy's roots, and the pipeline, easy_synthesize_marks and the batcher on tiny models (GPU).

The reference is `contour_ref` below: the section above sbv2_formant_contour in include/sbv2_hip.h restated in numpy, autocorrelation and
Levinson in longdouble (and again in float64, whose distance from longdouble is the yardstick), the roots by np.roots on float64 coefficients.

Bounds (DESIGN.md 8y has the measured figures).  Coefficients: E = max over a case's frames of max |a - a_ref| / max |a_ref| <= 4 max(E64,
2^-52), E64 the same for the float64 restatement (2^-52: one frame's E64 can be 0 by luck; no f64 result is closer than half an ulp).  Roots: the
residual |A(z)| / sum |a_k| |z|^(p-k) of every delivered (F, B) mapped back to z <= 2 times the worst residual of np.roots on the device's own
coefficients in that frame.  Selection: some root of A lies within p |A(z) / A'(z)| of z, so a delivered root and numpy's differ by at most the
sum of the two, evaluated in float64 (hence 8 eps of the evaluation's own error on top), turned into Hz by dF = dz sr / (2 pi |z|), dB = 2 dF."""
import ctypes as C
import functools
import inspect
import math
import os
import re

import numpy as np
import pytest

import flac_reader as R
from helpers import blob, make_utts, weights
from sbv2_api_amd import _lib, batcher, model, orchestrator, synth
from test_formant import FORMANTS, REQUEST, STYLES, TokenPipe, _payload, vowel
from test_spectrum import SpecPipe, request_rows  # noqa: F401

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = {"sbv2_pipeline_fetch_request_formant_contour": 17, "sbv2_formant_contour_defaults": 2, "sbv2_debug_formant_contour": 8}
FC = model.FormantContour
EPS = 2.0 ** -52


# ---- the reference ----------------------------------------------------------------------------------------------------------------------------
def frames_ref(u, sr, hop, W):
    """s [n_frames][W] in float64: pre-emphasis from 50 Hz, then the Gaussian window."""
    n, alpha = len(u), math.exp(-2.0 * math.pi * 50.0 / sr)
    i = np.arange(W, dtype=np.float64)
    w = (np.exp(-12.0 * ((i - (W - 1) / 2.0) / (W + 1)) ** 2) - math.exp(-12.0)) / (1.0 - math.exp(-12.0))
    pad = np.concatenate([np.zeros(W + 1), np.asarray(u, np.float64), np.zeros(W + hop + 1)])
    out = np.zeros((-(-n // hop) if n else 0, W))
    for f in range(len(out)):
        seg = pad[f * hop + hop // 2 - W // 2 + W:][:W + 1]                      # u[b - 1 .. b + W - 1]
        out[f] = (seg[1:] - alpha * seg[:-1]) * w
    return out


def lpc_ref(s, p, dt):
    """a[0 .. p] of one frame: autocorrelation and Levinson-Durbin in dtype dt."""
    s = s.astype(dt)
    r = np.array([np.sum(s[:len(s) - k] * s[k:], dtype=dt) for k in range(p + 1)], dt)
    a, E = np.eye(1, p + 1, dtype=dt)[0], r[0]
    for m in range(1, p + 1 if r[0] != 0 else 0):
        k = -(r[m] + np.sum(a[1:m] * r[m - 1:0:-1], dtype=dt)) / E
        a[1:m] = a[1:m] + k * a[m - 1:0:-1]
        a[m] = k
        E = E * (1 - k * k)
        if not E > 0:
            break
    return a


def select_ref(z, sr, c):
    """(F [k], B [k], z [k]) of the kept roots by ascending F, zeros where there are fewer; near: a root within 1 Hz of a limit."""
    F, B = np.angle(z) * sr / (2.0 * np.pi), -np.log(np.abs(z)) * sr / np.pi
    keep = (F >= c.f_lo) & (F <= c.f_hi) & (B > 0) & (B <= c.bw_max)
    near = bool((np.minimum(np.abs(F - c.f_lo), np.abs(F - c.f_hi)) < 1.0).any() or (np.abs(B - c.bw_max) < 1.0).any())
    order = np.argsort(F[keep], kind="stable")[:c.n_formants]
    pad = lambda v: np.concatenate([v[keep][order], np.zeros(c.n_formants - len(order), v.dtype)])
    return pad(F), pad(B), pad(z), near


def poly_terms(a, z):
    """|A(z)|, |A'(z)| and sum |a_k| |z|^(p-k) at the points z, in float64."""
    p = len(a) - 1
    pw = z[:, None] ** (p - np.arange(p + 1))[None, :]
    return np.abs((a * pw).sum(1)), np.abs(np.polyval(np.polyder(a), z)), (np.abs(a) * np.abs(pw)).sum(1)


def contour_ref(u, sr, c):
    """Per frame the longdouble and the float64 coefficients of the restatement, and its selection (from np.roots of the float64 ones)."""
    S = frames_ref(u, sr, c.hop, c.window)
    al = [lpc_ref(s, c.order, np.longdouble) for s in S]
    a64 = [lpc_ref(s, c.order, np.float64) for s in S]
    sel = [select_ref(np.roots(a), sr, c) if a[1:].any() else (np.zeros(c.n_formants),) * 3 + (False,) for a in a64]
    return al, a64, sel


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------------
# (sr, order, window, hop, n, encoding, kept, limits): smallest and largest lane counts of the root step, both ownerships (window <= 512: four
# frames to a workgroup), windows reaching outside the signal on both sides, a hop above the window, a stretch of exact zeros
NOLIM = (None, None, None)   # (f_lo, f_hi, bw_max): the defaults
CASES = [(8000, 4, 64, 80, 241, "f32", 2, NOLIM), (8000, 4, 200, 80, 199, "mulaw", 2, NOLIM), (8000, 10, 200, 33, 700, "s16", 3, (None, None, 400.0)),
         (16000, 18, 400, 160, 2401, "zeros", 4, NOLIM), (16000, 18, 400, 160, 1, "f32", 4, NOLIM), (16000, 18, 400, 160, 0, "s16", 4, NOLIM),
         (16000, 18, 512, 160, 481, "s16", 3, (300.0, 4000.0, 600.0)), (44100, 46, 1102, 441, 1324, "f32", 8, NOLIM),
         (48000, 50, 1200, 480, 1441, "mulaw", 5, NOLIM), (48000, 50, 2048, 480, 2047, "s16", 4, NOLIM), (48000, 50, 2048, 3000, 6001, "f32", 4, NOLIM)]


@functools.lru_cache(maxsize=None)
def case(sr, order, window, hop, n, encoding, kept, limits):
    """The vowel plus seeded noise 40 dB below it (so that r is well conditioned) as the device reads it: (x, hook encoding, u, spec, ref)."""
    rng = np.random.default_rng(sr + order + window + n)
    u = (np.resize(vowel(sr), n) + 0.007 * rng.standard_normal(n)).astype(np.float32)
    zeros = encoding == "zeros"
    if zeros:
        u[800:1600], encoding = 0.0, "s16"
    x, enc = u, None
    if encoding != "f32":
        x = np.clip(np.rint(u * 32768.0), -32768, 32767).astype(np.int16)
        if encoding == "mulaw":
            x, enc = model.g711_encode(x, "mulaw"), "mulaw"
        u = (model.g711_decode(x, "mulaw") if enc else x).astype(np.float64) / 32768.0
    c = FC(hop, kept, order, window, *limits)
    model.formant_contour_defaults(sr, c)
    return x, enc, u, c, contour_ref(u, sr, c), zeros


# ---- host only ------------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_exported_and_declared():
    header = open(os.path.join(ROOT, "include", "sbv2_hip.h")).read()
    for name, nargs in NEW_SYMBOLS.items():
        assert name in _lib.SYMBOLS and len(_lib.SYMBOLS[name][1]) == nargs
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert decl and decl.group(1).count(",") + 1 == nargs
        assert getattr(_lib.lib(), name)
    assert "formants" in inspect.signature(model.Pipeline.fetch_request).parameters and model._fetch_fields(formants=True)[-1] == "formants"


def test_the_restatement_tracks_the_vowel():
    """120 Hz pulses through resonators at 700 / 1200 / 2600 Hz at 16 kHz, the defaults (order 18, 25 ms): F1 .. F3 of the inner frames."""
    sr, c = 16000, FC(160, 3, bw_max=400.0)
    model.formant_contour_defaults(sr, c)
    _, _, sel = contour_ref(vowel(sr).astype(np.float64), sr, c)
    F = np.array([s[0] for s in sel])[3:-3]
    off = np.abs(F - np.array([f for f, _ in FORMANTS])[None, :])
    print(f"[formant contour] the restatement on the vowel: worst |F - resonator| = {off.max(axis=0)} Hz over {len(F)} frames")
    assert (off.max(axis=0) <= 60.0).all()                                       # half a harmonic spacing: the comb samples the envelope every 120 Hz


def test_defaults_and_refusals_that_need_no_run():
    l, nan = _lib.lib(), float("nan")
    for sr, want in ((8000, (200, 10, 3950.0, 4000.0)), (16000, (400, 18, 5500.0, 8000.0)), (44100, (1102, 46, 5500.0, 22050.0)),
                     (48000, (1200, 50, 5500.0, 24000.0))):
        c = FC(sr // 100)
        assert model.formant_contour_defaults(sr, c, 3 * c.hop + 1) == 4 and (c.window, c.order, c.f_hi, c.bw_max) == want and c.f_lo == 50.0
    ok = dict(hop=160, window=400, order=18, n_formants=4, f_lo=50.0, f_hi=5500.0, bw_max=8000.0, reserved=0)
    bad = [(dict(hop=0), "hop"), (dict(window=63), "window"), (dict(window=2049), "window"), (dict(order=2), "order"), (dict(order=52), "order"),
           (dict(order=17), "order"), (dict(order=100), "order"), (dict(order=16, window=64), "window / 4"), (dict(n_formants=0), "n_formants"),
           (dict(n_formants=9), "n_formants"), (dict(n_formants=3, order=4, window=64), "n_formants"), (dict(f_lo=-1.0), "f_lo"),
           (dict(f_lo=5500.0), "f_lo"), (dict(f_hi=8000.0), "f_hi"), (dict(f_lo=nan), "f_lo"), (dict(f_hi=nan), "f_hi"), (dict(bw_max=-1.0), "bw_max"),
           (dict(bw_max=nan), "bw_max"), (dict(reserved=1), "reserved")]
    out, x = np.full(8, 7.0), np.zeros(100, np.int16)

    def struct(capacity=1, ptr=True, **kw):
        v = dict(ok, **kw)
        p = out.ctypes.data_as(C.POINTER(C.c_double)) if ptr else None
        return _lib.Sbv2FormantContour(v["hop"], v["window"], v["order"], v["n_formants"], v["f_lo"], v["f_hi"], v["bw_max"], v["reserved"], capacity,
                                       p, p, None, 0)

    for kw, word in bad:
        for call in (lambda c: l.sbv2_formant_contour_defaults(16000, C.byref(c)),
                     lambda c: l.sbv2_debug_formant_contour(0, x.ctypes.data, 1, x.size, 16000, C.byref(c), None, None)):
            c = struct(**kw)
            assert call(c) == 1 and c.n_frames == 0 and word in l.sbv2_last_error().decode(), (kw, l.sbv2_last_error())
    for sr in (0, 48001):
        assert l.sbv2_formant_contour_defaults(sr, C.byref(struct())) == 1 and "sample rate" in l.sbv2_last_error().decode()
    assert l.sbv2_debug_formant_contour(0, x.ctypes.data, 1, x.size, 16000, C.byref(struct(capacity=0)), None, None) == 1   # 1 frame here
    assert "too small" in l.sbv2_last_error().decode()
    assert l.sbv2_debug_formant_contour(0, x.ctypes.data, 1, x.size, 16000, C.byref(struct(ptr=False)), None, None) == 1
    assert "must not be NULL" in l.sbv2_last_error().decode() and (out == 7.0).all()


@pytest.mark.parametrize("sr,order,window,hop,n,encoding,kept,limits", CASES)
def test_the_cases_keep_clear_of_the_limits(sr, order, window, hop, n, encoding, kept, limits):
    """The condition of the selection comparison, on the restatement alone: at most 2 % of a case's frames have a root within 1 Hz of a limit."""
    *_, (_, _, sel), _ = case(sr, order, window, hop, n, encoding, kept, limits)
    assert sum(s[3] for s in sel) <= 0.02 * len(sel)


class ContourPipe(SpecPipe):
    """SpecPipe whose fetch_request knows formants: 3 frames, F[f][q] = 500 (q + 1) + f, and no F2 in frame 1."""

    def fetch_request(self, b, rows, fmt, place, joined_len, formants=None, **kw):
        res = super().fetch_request(b, rows, fmt, place, joined_len, **kw)
        self.calls[-1]["formants"] = None if formants is None else (formants.hop, formants.n_formants, formants.order, formants.window, formants.f_hi)
        if formants is None:
            return res
        formants.f_hz = 500.0 * (np.arange(formants.n_formants)[None, :] + 1) + np.arange(3.0)[:, None]
        formants.f_hz[1, 1:] = 0.0
        formants.bw_hz, formants.status, formants.order = formants.f_hz / 10.0, np.zeros(3, np.int32), formants.order or 18
        return tuple(res) + (formants,)


def test_routes_carry_or_refuse_the_contour():
    SO = orchestrator.SynthesizeOptions
    pipe = ContourPipe()
    plain = orchestrator.easy_synthesize(pipe, REQUEST, STYLES, noise_seed=1)
    _, mk0 = orchestrator.easy_synthesize_marks(pipe, REQUEST, STYLES, noise_seed=1)
    assert "formants" not in mk0 and pipe.calls[-1]["formants"] is None
    _, mk = orchestrator.easy_synthesize_marks(pipe, REQUEST, STYLES, noise_seed=1, options=SO(formants=2, sample_rate=16000, encoding="s16"))
    assert pipe.calls[-1]["formants"] == (160, 2, 18, 400, 5500.0)              # the defaults, resolved by the library before the run
    assert mk["formants"] == {"hop": 160, "order": 18, "f_hz": [[500.0, 1000.0], [501.0, 0.0], [502.0, 1002.0]],
                              "bw_hz": [[50.0, 100.0], [50.1, 0.0], [50.2, 100.2]]}
    centre = np.arange(3) * 160 + 80
    for t in mk["tokens"]:                                                        # the mean of the non-zero F1 / F2 of the frames centred in the span
        f = [mk["formants"]["f_hz"][k] for k in range(3) if t["start"] <= centre[k] < t["end"]]
        for q, name in enumerate(("f1_hz", "f2_hz")):
            v = [r[q] for r in f if r[q] > 0]
            assert t[name] == (float(np.mean(v)) if v else None)
    strip = lambda m: dict({k: v for k, v in m.items() if k != "formants"}, tokens=[{k: v for k, v in t.items() if k not in ("f1_hz", "f2_hz")}
                                                                                    for t in m["tokens"]])
    _, mk = orchestrator.easy_synthesize_marks(pipe, REQUEST, STYLES, noise_seed=1,
                                               options=SO(formants=3, formants_hz=200, formants_max_hz=5000.0, formants_order=12, formants_window=512))
    assert pipe.calls[-1]["formants"] == (220, 3, 12, 512, 5000.0) and strip(mk) == mk0
    runs = pipe.runs
    for kw in (dict(formants=9), dict(formants=0), dict(formants=4, formants_order=7), dict(formants=4, formants_window=32),
               dict(formants=4, formants_max_hz=30000.0), dict(formants=4, formants_order=50, formants_window=128)):
        with pytest.raises(orchestrator.FormantsError, match="formants"):
            orchestrator.easy_synthesize_marks(pipe, REQUEST, STYLES, noise_seed=1, options=SO(**kw))
    for kw in (dict(formants_hz=50), dict(formants_max_hz=4000.0), dict(formants_order=12), dict(formants_window=400), dict(formants=True),
               dict(formants=4, formants_hz=0), dict(formants=4, formants_max_hz=float("nan")), dict(formants=4, formants_order=12.5)):
        with pytest.raises(orchestrator.FormantsError, match="formants"):         # the dependent fields need formants; the types
            SO(**kw)
    with pytest.raises(orchestrator.FormantsError, match="/synthesize_marks"):    # every route without whole-signal marks names the one with
        orchestrator.easy_synthesize(pipe, REQUEST, STYLES, noise_seed=1, options=SO(formants=4))
    for kw in (dict(), dict(split=True), dict(levels=True), dict(levels=True, spectrum=True)):
        with pytest.raises(orchestrator.FormantsError, match="/synthesize_marks"):
            orchestrator.easy_synthesize_stream(None, None, REQUEST[:1], STYLES, options=SO(formants=4, spectrum_mels=40), **kw)
    old = TokenPipe()
    with pytest.raises(model.Sbv2Error, match="formants needs a pipeline"):       # a pipeline from before the option: never served without
        orchestrator.easy_synthesize_marks(old, REQUEST, STYLES, noise_seed=1, options=SO(formants=4))
    assert pipe.runs == runs and old.runs == 0
    rb = batcher.RequestBatcher(pipe, start=False, clock=lambda: 0.0, max_wait_ms=1000.0)
    f0 = rb.submit(REQUEST, STYLES, options=SO(formants=1), noise_seed=1, marks=True)
    f1 = rb.submit(REQUEST, STYLES, options=SO(formants=1), noise_seed=1)
    rb.start()
    rb.close()
    assert f0.result(0)[1]["formants"]["f_hz"] == [[500.0], [501.0], [502.0]] and _payload(f0.result(0)[0]).tobytes() == _payload(plain).tobytes()
    with pytest.raises(orchestrator.FormantsError, match="/synthesize_marks"):
        f1.result(0)


def test_rest_carries_the_fields_on_synthesize_marks_and_answers_400_elsewhere():
    pytest.importorskip("fastapi")
    from concurrent.futures import Future
    from fastapi.testclient import TestClient
    from sbv2_api_amd import rest
    wav, seen, marks = orchestrator.array_to_wav(np.zeros((1, 1, 10), np.float32)), [], {"sample_rate": 44100, "tokens": [], "words": []}

    class H:
        def easy_synthesize(self, ident, text, style_id, speaker_id, options):
            return wav

        def easy_synthesize_batched(self, ident, text, style_id, speaker_id, options, batching=None, marks=False):
            f = Future()
            try:
                f.set_result(self.easy_synthesize_marks(ident, text, style_id, speaker_id, options) if marks else wav)
            except Exception as e:
                f.set_exception(e)
            return f

        def easy_synthesize_marks(self, ident, text, style_id, speaker_id, options):
            seen.append(orchestrator.formants_options(options, options.sample_rate))
            return wav, marks

        def easy_synthesize_stream(self, ident, text, style_id, speaker_id, options, **kw):
            raise AssertionError("a stream with formants must be refused before the holder is asked")

    body = {"text": "x", "ident": "m", "formants": 3, "formants_hz": 200, "formants_order": 12, "sample_rate": 16000, "encoding": "s16"}
    for c in (TestClient(rest.make_app(H()), raise_server_exceptions=False), TestClient(rest.make_app(H(), batching={}), raise_server_exceptions=False)):
        assert c.post("/synthesize_marks", json=body).status_code == 200
        assert (seen[-1].hop, seen[-1].n_formants, seen[-1].order, seen[-1].window) == (80, 3, 12, 400)
        assert c.post("/synthesize_marks", json={"text": "x", "ident": "m"}).status_code == 200 and seen[-1] is None
        r = c.post("/synthesize_marks", json=dict(body, formants_order=13))
        assert r.status_code == 400 and "order" in r.text
        for route in ("/synthesize", "/synthesize_stream", "/synthesize_stream_marks"):
            for b in (body, {"text": "x", "ident": "m", "formants_hz": 50}):
                r = c.post(route, json=b)
                assert r.status_code == 400 and "formants" in r.text and "/synthesize_marks" in r.text, (route, r.status_code, r.text)
        assert c.post("/synthesize", json={"text": "x", "ident": "m"}).content == wav


# ---- the stage against the restatement and numpy's roots -------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("sr,order,window,hop,n,encoding,kept,limits", CASES)
def test_stage_against_the_restatement(sr, order, window, hop, n, encoding, kept, limits):
    x, enc, u, c, (al, a64, _), zeros = case(sr, order, window, hop, n, encoding, kept, limits)
    got, lpc = model.debug_formant_contour(x, sr, FC(hop, kept, order, window, c.f_lo, c.f_hi, c.bw_max), encoding=enc)
    nf, p = -(-n // hop), order
    assert got.f_hz.shape == got.bw_hz.shape == (nf, kept) and lpc.shape == (nf, p + 1) and got.status.shape == (nf,)
    assert np.isfinite(got.f_hz).all() and np.isfinite(got.bw_hz).all() and np.isfinite(lpc).all() and not got.status.any()
    silent = [f for f in range(nf) if not al[f][1:].any()]                   # (exact zeros under the whole window, or a window past the signal's end)
    assert (silent or not zeros) and all(not got.f_hz[f].any() and not got.bw_hz[f].any() and not lpc[f][1:].any() for f in silent)
    worst = lambda a, f: float(np.max(np.abs(a - al[f])) / np.max(np.abs(al[f])))
    e, e64 = max([worst(lpc[f], f) for f in range(nf)], default=0.0), max([worst(a64[f], f) for f in range(nf)], default=0.0)
    k_res, k_sel, skipped = 0.0, 0.0, 0
    for f in set(range(nf)) - set(silent):
        a, znp = lpc[f], np.roots(lpc[f])
        F, B, zr, near = select_ref(znp, sr, c)
        live = got.f_hz[f] > 0
        z = np.exp(-np.pi * got.bw_hz[f][live] / sr + 2j * np.pi * got.f_hz[f][live] / sr)
        A, dA, S = poly_terms(a, z)
        An, _, Sn = poly_terms(a, znp)
        k_res = max(k_res, float((A / S).max() / (An / Sn).max()) if live.any() else 0.0)
        assert (A / S <= 2.0 * (An / Sn).max()).all(), (f, A / S, (An / Sn).max())
        if near:
            skipped += 1
            continue
        assert (live == (F > 0)).all(), (f, got.f_hz[f], F)
        Ar, dAr, Sr = poly_terms(a, zr[live])
        dz = p * ((A + 8 * EPS * S) / dA + (Ar + 8 * EPS * Sr) / dAr)
        tol = dz * sr / (2.0 * np.pi * np.abs(z))
        dF, dB = np.abs(got.f_hz[f][live] - F[live]), np.abs(got.bw_hz[f][live] - B[live])
        k_sel = max(k_sel, float((dF / tol).max()), float((dB / (2 * tol)).max())) if live.any() else k_sel
        assert (dF <= tol).all() and (dB <= 2 * tol).all(), (f, dF, dB, tol)
    print(f"[formant contour] sr={sr} p={p} W={window} hop={hop} n={n} {encoding}: E={e:.3e} E64={e64:.3e} E/max(E64,eps)={e / max(e64, EPS):.2f} "
          f"residual/numpy's={k_res:.3f} selection/tolerance={k_sel:.3f} skipped={skipped}/{nf}")
    assert e <= 4.0 * max(e64, EPS) and skipped <= 0.02 * nf
    again, lpc2 = model.debug_formant_contour(x, sr, FC(hop, kept, order, window, c.f_lo, c.f_hi, c.bw_max), encoding=enc)
    assert again.f_hz.tobytes() == got.f_hz.tobytes() and again.bw_hz.tobytes() == got.bw_hz.tobytes() and lpc2.tobytes() == lpc.tobytes()


# ---- through the pipeline ----------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("encoding,rate,flac", [("f32", 44100, False), ("s16", 16000, False), ("mulaw", 8000, False), ("s16", 16000, True)], ids=["f32-44k", "s16-16k", "mulaw-8k", "flac-16k"])
def test_pipeline_contour(request_rows, encoding, rate, flac):
    pipe, b, rows, place, joined = request_rows
    fmt, hop = model.PcmFormat(rate, encoding), rate // 100
    kw = dict(gain=model.Loudness(-23.0, -1.0), flac=flac, marks=True, env_hop=hop, pitch=model.Pitch(hop), spectrum=model.Spectrum(512, hop, 40))
    plain, pstats, pm, pp, ps = pipe.fetch_request(b, rows, fmt, place, joined, **kw)
    plain, pf0, ppow = plain if flac else plain.copy(), pp.f0.copy(), ps.power.copy()
    out, stats, m, p, s, fc = pipe.fetch_request(b, rows, fmt, place, joined, formants=FC(hop, 4), **kw)
    assert (out == plain) if flac else (out.dtype == plain.dtype and out.tobytes() == plain.tobytes())
    assert stats.tobytes() == pstats.tobytes() and p.f0.tobytes() == pf0.tobytes() and s.power.tobytes() == ppow.tobytes()
    for x, y in zip(pm.arrays(), m.arrays()):
        assert x.tobytes() == y.tobytes()
    samples = np.asarray(R.read(out)["samples"], np.int16) if flac else out
    nf = -(-model.pcm_format_length(fmt, joined) // hop)
    assert fc.f_hz.shape == (nf, 4) and fc.f_hz.max() > 0 and fc.order == (2 + rate // 1000 + 1) // 2 * 2 and fc.window == rate // 40
    hook, _ = model.debug_formant_contour(samples, rate, FC(hop, 4), encoding=encoding if encoding == "mulaw" else None)
    assert hook.f_hz.tobytes() == fc.f_hz.tobytes() and hook.bw_hz.tobytes() == fc.bw_hz.tobytes() and hook.status.tobytes() == fc.status.tobytes()
    out2, _, fc2 = pipe.fetch_request(b, rows, fmt, place, joined, gain=kw["gain"], flac=flac, formants=FC(hop, 4))   # a second fetch, no other stage
    assert ((out2 == plain) if flac else out2.tobytes() == plain.tobytes()) and (fc2.f_hz.tobytes(), fc2.bw_hz.tobytes()) == (fc.f_hz.tobytes(), fc.bw_hz.tobytes())


@gpu
def test_marks_routes_carry_the_block():
    bs, vs = model.load_model(blob("bert", "tiny", 3), True), model.load_model(blob("vits", "tiny", 5), False)
    bc, vc = weights("bert", "tiny", 3)[0], weights("vits", "tiny", 5)[0]
    sv = synth.hash_normal(77, 3 * vc["style_dim"]).reshape(3, -1).astype(np.float32) * 0.1
    sents = [{k: u[k] for k in ("input_ids", "word2ph", "phones", "tones", "langs")} for u in make_utts([14, 40], bc, vc, seed0=151, with_bert=False)]
    o = lambda **kw: orchestrator.SynthesizeOptions(sample_rate=16000, encoding="s16", **kw)
    pipe = model.Pipeline(bs, vs)
    try:
        wav0, mk0 = orchestrator.easy_synthesize_marks(pipe, sents, sv, 1, 0, o(), noise_seed=99)
        wav, mk = orchestrator.easy_synthesize_marks(pipe, sents, sv, 1, 0, o(formants=3), noise_seed=99)
        fm = mk["formants"]
        nf = -(-mk["tokens"][-1]["end"] // 160)
        assert wav == wav0 and (fm["hop"], fm["order"]) == (160, 18) and len(fm["f_hz"]) == len(fm["bw_hz"]) >= nf and len(fm["f_hz"][0]) == 3
        assert np.max(fm["f_hz"]) > 0 and all("f1_hz" in t and "f2_hz" in t for t in mk["tokens"]) and "formants" not in mk0
        rb = batcher.RequestBatcher(pipe, start=False, max_wait_ms=1000.0)
        f1 = rb.submit(sents, sv, 1, 0, o(formants=3), noise_seed=99, marks=True)
        rb.start()
        rb.close()
        assert f1.result(0)[0] == wav and f1.result(0)[1] == mk
    finally:
        pipe.close(); bs.close(); vs.close()
