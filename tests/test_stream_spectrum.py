"""The spectrum of a stream's delivered samples: the fed stage (csrc/spectrum.hip StreamSpectrum / k_stream_spectrum, sbv2_debug_stream_spectrum),
the C ABI (sbv2_stream_begin_request_spectrum, sbv2_stream_next_spectrum), model.StreamHandle(spectrum=), orchestrator.easy_synthesize_stream(
spectrum=True) and POST /synthesize_stream_marks with spectrum_stream.

The fed stage is held to what test_spectrum.py holds the one-shot stage to, E <= 4 E32 against the float64 restatement there, and to the one-shot
stage itself bit for bit, at every group count.  The tiny decoder's stream halo holds no resampling filter below 24 kHz (test_stream_pitch.py
notes it), so the streams here run at 44.1 and 24 kHz; the 16 kHz / n_fft 400 / hop 160 and 8 kHz shapes are covered by the fed stage."""
import base64
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from helpers import blob
from sbv2_api_amd import _lib, model, orchestrator
from test_spectrum import make_signal, spectrum_ref, worst
from test_stream_marks_levels import LINES, STYLES, FakeHandle
from test_stream_pitch import F, _delivered_samples, _four, _gaps

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = {"sbv2_stream_begin_request_spectrum": 22, "sbv2_stream_next_spectrum": 2, "sbv2_debug_stream_spectrum": 10}


def per_push_np(cuts, n, hop, n_fft):
    """The completion rule of the header, stated directly: the frames each push completes when the pushes end at cuts + [n]."""
    f = np.arange(-(-n // hop) if n > 0 else 0, dtype=np.int64)
    done = [int((np.minimum(f * hop + hop // 2 + n_fft // 2, n) <= D).sum()) for D in list(cuts) + [n]]
    return list(np.diff([0] + done))


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_exported_and_declared():
    header = open(os.path.join(ROOT, "include", "sbv2_hip.h")).read()
    for name, nargs in NEW_SYMBOLS.items():
        assert name in _lib.SYMBOLS and len(_lib.SYMBOLS[name][1]) == nargs and getattr(_lib.lib(), name)
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert decl and re.sub(r"/\*.*?\*/", "", decl.group(1)).count(",") + 1 == nargs
    assert C.sizeof(_lib.Sbv2StreamSpectrum) == 32 and C.sizeof(_lib.Sbv2StreamSpectrumPart) == 40
    assert "the spectrum on streams" not in header


def test_refusals_that_need_no_run():
    l = _lib.lib()
    gap = np.zeros(1, np.int64)
    f8 = F(8000, "s16")
    rq8 = _lib.Sbv2StreamRequest(gap.ctypes.data_as(_lib.i64p), C.pointer(f8.c), None, 0, 0)
    ok = dict(n_fft=400, hop=160, n_mels=80, reserved=0, f_min=0.0, f_max=4000.0)
    for field, value in (("n_fft", 32), ("n_fft", 408), ("hop", 0), ("hop", 401), ("n_mels", 129), ("f_max", 4000.5), ("reserved", 1)):
        v = dict(ok, **{field: value})
        cs = _lib.Sbv2StreamSpectrum(v["n_fft"], v["hop"], v["n_mels"], v["reserved"], v["f_min"], v["f_max"])
        h, ns, nb = C.c_void_p(0x55), C.c_int64(-5), C.c_int32(-6)
        rc = l.sbv2_stream_begin_request_spectrum(None, None, None, None, None, None, None, None, 16, C.byref(rq8), None, None, None, None, C.byref(cs),
                                                  C.byref(h), None, None, None, None, C.byref(ns), C.byref(nb))
        assert rc != 0 and field in l.sbv2_last_error().decode() and (h.value, ns.value, nb.value) == (0x55, -5, -6), (field, l.sbv2_last_error())
    cs = _lib.Sbv2StreamSpectrum(400, 160, 80, 0, 0.0, 4000.0)   # everything static passed: the null handles themselves
    assert l.sbv2_stream_begin_request_spectrum(*[None] * 8, 16, C.byref(rq8), None, None, None, None, C.byref(cs), *[None] * 7) != 0
    assert b"bad arguments" in l.sbv2_last_error()
    assert l.sbv2_stream_next_spectrum(None, None) != 0 and b"bad arguments" in l.sbv2_last_error()
    x, per = np.zeros(100, np.int16), np.zeros(2, np.int64)
    c, _ = model.Spectrum(400, 160, 80).c_struct(100, 16000)
    for kw, word in ((dict(cuts=[50, 40]), "cuts must ascend"), (dict(groups=9), "groups")):
        cuts = np.asarray(kw.get("cuts", [50]), np.int64)
        assert l.sbv2_debug_stream_spectrum(99, x.ctypes.data, 1, 100, cuts.ctypes.data_as(_lib.i64p), cuts.size, 16000, C.byref(c), kw.get("groups", 0),
                                            per.ctypes.data_as(_lib.i64p)) != 0 and word in l.sbv2_last_error().decode()


class SpecFakeHandle(FakeHandle):
    """FakeHandle with a spectrum that follows the completion rule: power[f][m] = f + m / 1000."""

    def __init__(self, *a, spectrum=None, **kw):
        super().__init__(*a, **kw)
        self.sp, self.s0 = spectrum, 0

    def next_spectrum(self):
        n = model.stream_spectrum_complete(self.D, self.sp.hop, self.sp.n_fft, self.total_samples)
        a, self.s0 = self.s0, n
        return a, (np.arange(a, n)[:, None] + np.arange(self.sp.n_bands())[None, :] / 1000.0).astype(np.float32), self.D


def _blocks_are_the_spectrum(blocks, head, total):
    db = np.concatenate([np.frombuffer(base64.b64decode(b["db"]), "<f4").reshape(b["shape"]) for b in blocks])
    nf, nb = -(-total // head["hop"]), head["n_bands"]
    want = 10.0 * np.log10(np.maximum((np.arange(nf)[:, None] + np.arange(nb)[None, :] / 1000.0).astype(np.float32).astype(np.float64), 1e-10))
    assert head["n_frames"] == nf and db.tobytes() == want.astype("<f4").tobytes()
    assert [b["first"] for b in blocks] == list(np.cumsum([0] + [b["shape"][0] for b in blocks[:-1]]))


def test_orchestrator_and_rest_carry_the_spectrum_on_the_new_words_only(monkeypatch):
    monkeypatch.setattr(model, "StreamHandle", SpecFakeHandle)
    O, SO = orchestrator, orchestrator.SynthesizeOptions
    opts = SO(spectrum_mels=40, spectrum_fft=400, spectrum_hop=160, sample_rate=16000, encoding="s16")
    plain = b"".join(O.easy_synthesize_stream(None, None, LINES, STYLES, options=SO(sample_rate=16000, encoding="s16"), noise_seed=5, split=True))
    for kw in (dict(), dict(levels=True)):                                       # without the new word: refused as before
        with pytest.raises(O.SpectrumError, match="/synthesize_marks"):
            O.easy_synthesize_stream(None, None, LINES, STYLES, options=opts, split=True, **kw)
    with pytest.raises(O.SpectrumError, match="levels=True"):
        O.easy_synthesize_stream(None, None, LINES, STYLES, options=opts, split=True, spectrum=True)
    with pytest.raises(O.SpectrumError, match="spectrum_mels"):
        O.easy_synthesize_stream(None, None, LINES, STYLES, options=SO(), split=True, levels=True, spectrum=True)
    for split in (True, False):
        st = O.easy_synthesize_stream(None, None, LINES if split else LINES[:1], STYLES, options=opts, noise_seed=5, split=split, levels=True, spectrum=True)
        sp = SpecFakeHandle.seen[-1][1]
        assert "spectrum" not in sp and (st._st.sp.n_fft, st._st.sp.hop, st._st.sp.n_mels, st._st.sp.f_max) == (400, 160, 40, None)
        head = st.marks["spectrum"]
        assert {k: head[k] for k in ("n_fft", "hop", "n_bands", "f_min", "f_max")} == dict(n_fft=400, hop=160, n_bands=40, f_min=0.0, f_max=8000.0)
        audio, blocks = [], []
        for piece in st:
            audio.append(piece)
            blocks.append(st.take_marks()["spectrum"])
        _blocks_are_the_spectrum(blocks, head, st.total_samples)
        assert not split or b"".join(audio) == plain

    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient
    from sbv2_api_amd import rest

    class Holder:
        calls = []

        def easy_synthesize_stream(self, ident, text, style_id, speaker_id, options, **kw):
            self.calls.append(kw)
            return O.easy_synthesize_stream(None, None, LINES, STYLES, style_id, speaker_id, options, noise_seed=5, **kw)

    c = TestClient(rest.make_app(Holder()))
    body = {"text": "a\n\nb", "ident": "m", "split_sentences": True, "sample_rate": 16000, "encoding": "s16", "spectrum_mels": 40, "spectrum_fft": 400}
    r = c.post("/synthesize_stream_marks", json=dict(body, spectrum_stream=True))
    assert r.status_code == 200 and Holder.calls[-1] == {"levels": True, "split": True, "spectrum": True}
    lines = [json.loads(s) for s in r.content.decode().splitlines()]
    assert lines[0]["spectrum"] == dict(n_fft=400, hop=160, n_bands=40, n_frames=-(-737 // 160), f_min=0.0, f_max=8000.0)
    _blocks_are_the_spectrum([ln["spectrum"] for ln in lines[1:]], lines[0]["spectrum"], 737)
    assert b"".join(base64.b64decode(ln["audio"]) for ln in lines[1:]) == plain
    n = len(Holder.calls)
    for route, b in (("/synthesize_stream_marks", body), ("/synthesize_stream", body), ("/synthesize_stream", dict(body, spectrum_stream=True))):
        r = c.post(route, json=b)
        assert r.status_code == 400 and "/synthesize_marks" in r.text
    for b in (dict(body, spectrum_stream=True, spectrum_fft=408), {k: v for k, v in dict(body, spectrum_stream=True).items() if k != "spectrum_mels"}):
        assert c.post("/synthesize_stream_marks", json=b).status_code == 400
    assert len(Holder.calls) == n


# ---- GPU, the fed stage ------------------------------------------------------------------------------------------------------------------------
H1 = (8000, 64, 1, "f32", 200, "-6")     # hop 1: with D samples in, the frames f + 32 <= D are complete
# (sr, n_fft, hop, encoding, n, signal), n_mels, (f_min, f_max or None), cuts
CASES = ([(H1, m, (0.0, None), cuts) for m in (0, 80) for cuts in ([10], list(range(7, 200, 7)), [40, 72, 105], [50, 50], [100, 200])] +
         [((16000, 400, 160, enc, 5000, "-6"), 80, (0.0, None), [1, 399, 400, 401, 2500]) for enc in ("s16", "mulaw")] +
         [((44100, 2048, 441, "f32", 9000, "-6"), m, (0.0, None), list(range(1000, 9000, 1000))) for m in (0, 128)] +
         [((8000, 64, 64, "s16", 700, "-6"), 0, (0.0, None), [64, 65, 300]), ((16000, 400, 160, "f32", 1, "-6"), 80, (0.0, None), [1]),
          ((16000, 400, 160, "f32", 0, "-6"), 80, (0.0, None), [0]), ((16000, 400, 160, "f32", 3000, "zeros"), 80, (0.0, None), [1000]),
          ((8000, 2048, 80, "s16", 3000, "-6"), 80, (300.0, 3400.0), [500, 1700])])   # 26 of 33 blocks in the bank, up to 6 groups, narrow low bands


@gpu
@pytest.mark.parametrize("shape,n_mels,band,cuts", CASES, ids=[f"{c[0][1]}-{c[0][2]}-{c[0][3]}-{c[0][4]}-m{c[1]}-{len(c[3])}cuts" for c in CASES])
def test_fed_stage_against_float64_and_the_one_shot(shape, n_mels, band, cuts):
    sr, n_fft, hop, encoding, n, kind = shape
    u = make_signal(kind, n, n_fft, seed=n_fft + n)
    x, enc = u, None
    if encoding != "f32":
        x = np.clip(np.rint(u * 32768.0), -32768, 32767).astype(np.int16)
        if encoding == "mulaw":
            x, enc = model.g711_encode(x, "mulaw"), "mulaw"
        u = (model.g711_decode(x, "mulaw") if enc else x).astype(np.float32) / np.float32(32768.0)
    spec = lambda: model.Spectrum(n_fft, hop, n_mels, *band)
    one = model.debug_spectrum(x, sr, spec(), encoding=enc)
    ref, ref32 = spectrum_ref(u, sr, n_fft, hop, n_mels, band[0], sr / 2.0 if band[1] is None else band[1])
    e32 = worst(ref32.astype(np.float64), ref)
    if n_fft == 64:
        assert per_push_np([40, 72, 105], 200, 1, 64)[1:3] == [32, 33]
    for groups in (1, 0, 8):             # one group, the rule's count, the largest the spec allows
        sp, per = model.debug_stream_spectrum(x, cuts, sr, spec(), encoding=enc, groups=groups)
        e = worst(sp.power.astype(np.float64), ref)
        print(f"[stream spectrum] {shape} mels={n_mels} groups={groups}: E={e:.3e} E32={e32:.3e}")
        assert sp.power.shape == ref.shape and e <= 4.0 * e32
        assert sp.power.tobytes() == one.power.tobytes(), np.argwhere(sp.power != one.power)[:4]
        assert list(per) == per_push_np(cuts, n, hop, n_fft)
        assert kind != "zeros" or not sp.power.any()


# ---- GPU, the stream on the tiny models ----------------------------------------------------------------------------------------------------------
# name -> (fmt or None = the identity format, flac, level, spectrum parameters)
FORMS = {"f32-44k": (None, False, False, (2048, 441, 0)), "s16-24k": (F(24000, "s16"), False, False, (400, 240, 80)),
         "flac-24k": (F(24000, "s16"), True, False, (400, 240, 80)), "mulaw-24k-level": (F(24000, "mulaw"), False, True, (256, 120, 40))}


@pytest.fixture(scope="module")
def tiny():
    """The tiny sessions, four rows with gaps, and from ONE pipeline run before any stream reuses the sessions the fetch of every form without a level."""
    bs, vs = model.load_model(blob("bert", "tiny", 3), True), model.load_model(blob("vits", "tiny", 5), False)
    pipe, utts = model.Pipeline(bs, vs), _four()
    b = pipe.prepare(utts, forced=True)
    pipe.run(b)
    lens, fetched = [int(v) for v in b.lens], {}
    for name, (fmt, flac, level, sp) in FORMS.items():
        gaps = _gaps(fmt)
        place = [0] + list(np.cumsum([n + g for n, g in zip(lens[:-1], gaps[:-1])]))
        if not level:
            res = pipe.fetch_request(b, range(4), fmt or F(44100, "f32"), place, place[-1] + lens[-1] + gaps[-1], flac=flac, spectrum=model.Spectrum(*sp))
            fetched[name] = res[-1].power.copy()
    yield dict(bs=bs, vs=vs, utts=utts, fetched=fetched)
    pipe.close(); bs.close(); vs.close()


@gpu
@pytest.mark.parametrize("chunk", [16, 50])
@pytest.mark.parametrize("name", list(FORMS))
def test_stream_spectrum_on_the_tiny_models(tiny, name, chunk):
    fmt, flac, level, sp = FORMS[name]
    ff = fmt or F(44100, "f32")
    kw = dict(fmt=fmt, flac=flac, level=model.StreamLevel(6.0) if level else None, gaps=_gaps(fmt), forced=True, levels=True, env_hop=ff.sample_rate // 100)
    plain = model.StreamHandle(tiny["bs"], tiny["vs"], tiny["utts"], chunk, **kw)
    plain_pieces, plain_marks = [], []
    while (p := plain.next()) is not None:
        plain_pieces.append(p)
        plain_marks.append(plain.next_marks())
    with pytest.raises(model.Sbv2Error, match="begun without a spectrum"):
        plain.next_spectrum()
    plain.close()
    st = model.StreamHandle(tiny["bs"], tiny["vs"], tiny["utts"], chunk, spectrum=model.Spectrum(*sp), **kw)
    nb = sp[2] or sp[0] // 2 + 1
    assert (st.n_spec, st.n_bands) == (-(-st.total_samples // sp[1]), nb)
    pieces, marks, power, at = [], [], [], 0
    while (p := st.next()) is not None:
        pieces.append(p)
        marks.append(st.next_marks())
        first, pw, D = st.next_spectrum()
        assert first == at and at + len(pw) == model.stream_spectrum_complete(D, sp[1], sp[0], st.total_samples)
        at += len(pw)
        power.append(pw)
    assert st.next_spectrum()[1].shape == (0, nb) and at == st.n_spec
    st.close()
    assert len(pieces) == len(plain_pieces) and all(bytes(memoryview(a)) == bytes(memoryview(b)) for a, b in zip(pieces, plain_pieces))
    assert all(a[0] == b[0] and a[6] == b[6] and all(a[i].tobytes() == b[i].tobytes() for i in (1, 2, 4, 5)) for a, b in zip(marks, plain_marks))
    power = np.concatenate(power)
    x = _delivered_samples(pieces, flac)
    hook = model.debug_spectrum(x, ff.sample_rate, model.Spectrum(*sp), encoding="mulaw" if ff.encoding == "mulaw" else None)
    assert power.tobytes() == hook.power.tobytes() and power.max() > 0
    assert level or power.tobytes() == tiny["fetched"][name].tobytes()            # ... and the joined fetch's of the same batch
