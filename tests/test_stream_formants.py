"""The formant contour of a stream's delivered samples: the fed stage (csrc/formants.hip StreamFormants / k_stream_formant,
sbv2_debug_stream_formant_contour), the C ABI (sbv2_stream_begin_request_formant_contour, sbv2_stream_next_formant_contour),
model.StreamHandle(formants=), orchestrator.easy_synthesize_stream(formants=True) and POST /synthesize_stream_marks with formants_stream.

The fed stage is held to the one-shot stage bit for bit, at every ownership (pack 0 = the rule, 1 and 4 forced); the one shot is held to the
longdouble restatement by test_formant_contour.py.  The tiny decoder's stream refuses rates below 24 kHz (test_stream_pitch.py notes it), so
the streams here run at 44.1 and 24 kHz; the 8, 16 and 22.05 kHz shapes are covered by the fed stage."""
import base64
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from helpers import blob
from sbv2_api_amd import _lib, model, orchestrator
from test_formant_contour import FC, case
from test_stream_marks_levels import LINES, STYLES, FakeHandle
from test_stream_pitch import F, _delivered_samples, _four, _gaps

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = {"sbv2_stream_begin_request_formant_contour": 24, "sbv2_stream_next_formant_contour": 2, "sbv2_debug_stream_formant_contour": 12}


def complete_np(D, total, hop, window):
    """The completion rule of the header, stated directly: the frames with min(b + window, total) <= D."""
    f = np.arange(-(-total // hop) if total > 0 else 0, dtype=np.int64)
    return int((np.minimum(f * hop + hop // 2 - window // 2 + window, total) <= D).sum())


def per_push_np(cuts, n, hop, window):
    return list(np.diff([0] + [complete_np(D, n, hop, window) for D in list(cuts) + [n]]))


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_exported_and_declared():
    header = open(os.path.join(ROOT, "include", "sbv2_hip.h")).read()
    for name, nargs in NEW_SYMBOLS.items():
        assert name in _lib.SYMBOLS and len(_lib.SYMBOLS[name][1]) == nargs and getattr(_lib.lib(), name)
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert decl and re.sub(r"/\*.*?\*/", "", decl.group(1)).count(",") + 1 == nargs
    assert C.sizeof(_lib.Sbv2StreamFormantContour) == 48 and C.sizeof(_lib.Sbv2StreamFormantPart) == 56
    assert "the contour on streams" not in header


def test_refusals_that_need_no_run():
    l = _lib.lib()
    gap = np.zeros(1, np.int64)
    f8 = F(8000, "s16")
    rq8 = _lib.Sbv2StreamRequest(gap.ctypes.data_as(_lib.i64p), C.pointer(f8.c), None, 0, 0)
    ok = dict(hop=80, window=200, order=10, n_formants=3, f_lo=0.0, f_hi=0.0, bw_max=0.0, reserved=0)
    begin = lambda cf, *out: l.sbv2_stream_begin_request_formant_contour(*[None] * 8, 16, C.byref(rq8), *[None] * 5, C.byref(cf), *out)
    for field, value in (("hop", 0), ("window", 63), ("window", 2049), ("order", 5), ("order", 52), ("order", 50), ("n_formants", 0), ("n_formants", 6),
                         ("f_lo", -1.0), ("f_hi", 4000.0), ("bw_max", -1.0), ("reserved", 1)):
        cf = _lib.Sbv2StreamFormantContour(*dict(ok, **{field: value}).values())
        h, tot, nff = C.c_void_p(0x55), C.c_int64(-4), C.c_int64(-5)
        rc = begin(cf, C.byref(h), C.byref(tot), *[None] * 5, C.byref(nff))
        assert rc != 0 and field in l.sbv2_last_error().decode() and (h.value, tot.value, nff.value) == (0x55, -4, -5), (field, l.sbv2_last_error())
    assert begin(_lib.Sbv2StreamFormantContour(*ok.values()), *[None] * 8) != 0 and b"bad arguments" in l.sbv2_last_error()
    assert l.sbv2_stream_next_formant_contour(None, None) != 0 and b"bad arguments" in l.sbv2_last_error()
    x, per, cuts = np.zeros(100, np.int16), np.zeros(3, np.int64), np.array([50, 40], np.int64)
    c, _ = FC(80, 3, 10, 64).c_struct(100, 8000)
    assert l.sbv2_debug_stream_formant_contour(99, x.ctypes.data, 1, 100, cuts.ctypes.data_as(_lib.i64p), 2, 8000, C.byref(c), None, None, 0,
                                               per.ctypes.data_as(_lib.i64p)) != 0 and b"cuts must ascend" in l.sbv2_last_error()


@pytest.mark.parametrize("hop,window,total", [(1, 64, 200), (160, 400, 5000), (220, 551, 3000), (3000, 2048, 6001), (160, 400, 1), (160, 400, 0)])
def test_the_completion_rule(hop, window, total):
    got = [model.stream_formants_complete(D, hop, window, total) for D in range(total + 1)]
    assert got == [complete_np(D, total, hop, window) for D in range(total + 1)] and got[-1] == (-(-total // hop) if total else 0)
    assert got == sorted(got)   # frames complete in order


class FormFakeHandle(FakeHandle):
    """FakeHandle with a contour that follows the completion rule: f_hz[f][q] = f + q / 1000, bw_hz a tenth of it."""

    def __init__(self, *a, formants=None, **kw):
        super().__init__(*a, **kw)
        self.fc, self.g0 = formants, 0

    def next_formants(self):
        n = model.stream_formants_complete(self.D, self.fc.hop, self.fc.window, self.total_samples)
        a, self.g0 = self.g0, n
        f = np.arange(a, n)[:, None] + np.arange(self.fc.n_formants)[None, :] / 1000.0
        return a, f, f / 10.0, np.zeros(n - a, np.int32), self.D


def _blocks_are_the_contour(blocks, head, total):
    nf = -(-total // head["hop"])
    want = np.arange(nf)[:, None] + np.arange(head["n_formants"])[None, :] / 1000.0
    f, b = (np.array([row for blk in blocks for row in blk[k]]).reshape(-1, head["n_formants"]) for k in ("f_hz", "bw_hz"))
    assert head["n_frames"] == nf and f.tobytes() == want.tobytes() and b.tobytes() == (want / 10.0).tobytes()
    assert [blk["first"] for blk in blocks] == list(np.cumsum([0] + [len(blk["f_hz"]) for blk in blocks[:-1]]))


def test_orchestrator_and_rest_carry_the_contour_on_the_new_words_only(monkeypatch):
    monkeypatch.setattr(model, "StreamHandle", FormFakeHandle)
    O, SO = orchestrator, orchestrator.SynthesizeOptions
    opts = SO(formants=3, formants_hz=100, sample_rate=16000, encoding="s16")
    plain = b"".join(O.easy_synthesize_stream(None, None, LINES, STYLES, options=SO(sample_rate=16000, encoding="s16"), noise_seed=5, split=True))
    for kw in (dict(), dict(levels=True)):                                       # without the new word: refused as before
        with pytest.raises(O.FormantsError, match="/synthesize_marks"):
            O.easy_synthesize_stream(None, None, LINES, STYLES, options=opts, split=True, **kw)
    with pytest.raises(O.FormantsError, match="levels=True"):
        O.easy_synthesize_stream(None, None, LINES, STYLES, options=opts, split=True, formants=True)
    with pytest.raises(O.FormantsError, match="options.formants"):
        O.easy_synthesize_stream(None, None, LINES, STYLES, options=SO(), split=True, levels=True, formants=True)
    want_head = dict(hop=160, order=18, n_formants=3)
    for split in (True, False):
        st = O.easy_synthesize_stream(None, None, LINES if split else LINES[:1], STYLES, options=opts, noise_seed=5, split=split, levels=True, formants=True)
        assert "formants" not in FormFakeHandle.seen[-1][1] and (st._st.fc.hop, st._st.fc.n_formants, st._st.fc.window) == (160, 3, 400)
        head = st.marks["formants"]
        assert {k: head[k] for k in want_head} == want_head
        audio, blocks = [], []
        for piece in st:
            audio.append(piece)
            blocks.append(st.take_marks()["formants"])
        _blocks_are_the_contour(blocks, head, st.total_samples)
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
    body = {"text": "a\n\nb", "ident": "m", "split_sentences": True, "sample_rate": 16000, "encoding": "s16", "formants": 3}
    r = c.post("/synthesize_stream_marks", json=dict(body, formants_stream=True))
    assert r.status_code == 200 and Holder.calls[-1] == {"levels": True, "split": True, "formants": True}
    lines = [json.loads(s) for s in r.content.decode().splitlines()]
    assert lines[0]["formants"] == dict(want_head, n_frames=-(-737 // 160))
    _blocks_are_the_contour([ln["formants"] for ln in lines[1:]], lines[0]["formants"], 737)
    assert b"".join(base64.b64decode(ln["audio"]) for ln in lines[1:]) == plain
    n = len(Holder.calls)
    for route, b in (("/synthesize_stream_marks", body), ("/synthesize_stream", body), ("/synthesize_stream", dict(body, formants_stream=True))):
        r = c.post(route, json=b)
        assert r.status_code == 400 and "/synthesize_marks" in r.text
    for b in (dict(body, formants_stream=True, formants_order=5), {k: v for k, v in dict(body, formants_stream=True).items() if k != "formants"}):
        assert c.post("/synthesize_stream_marks", json=b).status_code == 400
    assert len(Holder.calls) == n


# ---- GPU, the fed stage ------------------------------------------------------------------------------------------------------------------------
# (sr, order, window, hop, n, encoding) as test_formant_contour.case takes them, then the cuts
H1 = (8000, 4, 64, 1, 200, "f32")   # hop 1: with D samples in, the frames f + 32 <= D are complete
CASES = ([(H1, cuts) for cuts in ([10], list(range(7, 200, 7)), [40, 72, 105], [50, 50], [100, 200])] +
         [((16000, 18, 400, 160, 5000, enc), [1, 399, 400, 401, 2500]) for enc in ("s16", "mulaw")] +
         [((22050, 24, 551, 220, 3000, "s16"), [275, 276, 277, 1500]), ((44100, 46, 1102, 441, 9000, "f32"), list(range(1000, 9000, 1000))),
          ((48000, 50, 2048, 3000, 6001, "f32"), [2048, 2049, 5000]), ((16000, 18, 400, 160, 1, "f32"), [1]), ((16000, 18, 400, 160, 0, "f32"), [0]),
          ((16000, 18, 400, 160, 2401, "zeros"), [1000])])


@gpu
@pytest.mark.parametrize("shape,cuts", CASES, ids=[f"{c[0][0]}-{c[0][2]}-{c[0][3]}-{c[0][4]}-{c[0][5]}-{len(c[1])}cuts" for c in CASES])
def test_fed_stage_against_the_one_shot(shape, cuts):
    sr, order, window, hop, n, encoding = shape
    kept = min(4, order // 2)
    x, enc, _, _, _, zeros = case(sr, order, window, hop, n, encoding, kept, (None, None, None))
    fc = lambda: FC(hop, kept, order, window)
    one, lpc1 = model.debug_formant_contour(x, sr, fc(), encoding=enc)
    assert not zeros or not (x[800:1600].any() or one.f_hz[6:9].any())      # (the frames wholly inside the stretch are silent)
    if window == 64:
        assert per_push_np([40, 72, 105], 200, 1, 64)[1:3] == [32, 33]
    for pack in (0, 1, 4):
        got, lpc, per = model.debug_stream_formant_contour(x, cuts, sr, fc(), encoding=enc, pack=pack)
        for name, a, b in (("f_hz", got.f_hz, one.f_hz), ("bw_hz", got.bw_hz, one.bw_hz), ("status", got.status, one.status), ("lpc", lpc, lpc1)):
            assert a.shape == b.shape and a.tobytes() == b.tobytes(), (pack, name, np.argwhere(a != b)[:4])
        assert list(per) == per_push_np(cuts, n, hop, window)
        still = model.g711_encode(np.zeros(n, np.int16), "mulaw") if enc else np.zeros_like(x)
        silent, lpc0, _ = model.debug_stream_formant_contour(still, cuts, sr, fc(), encoding=enc, pack=pack)
        assert not silent.f_hz.any() and not silent.bw_hz.any() and not silent.status.any() and not lpc0[:, 1:].any()
    assert n <= 1 or one.f_hz.any()


# ---- GPU, the stream on the tiny models ----------------------------------------------------------------------------------------------------------
# name -> (fmt or None = the identity format, flac, level, (hop, n_formants, order, window); None = the defaults at the rate)
FORMS = {"f32-44k": (None, False, False, (441, 4, None, None)), "s16-24k": (F(24000, "s16"), False, False, (240, 4, None, None)),
         "flac-24k": (F(24000, "s16"), True, False, (240, 4, None, None)), "mulaw-24k-level": (F(24000, "mulaw"), False, True, (120, 3, 12, 256))}


@pytest.fixture(scope="module")
def tiny():
    """The tiny sessions, four rows with gaps, and from ONE pipeline run before any stream reuses the sessions the fetch of every form without a level."""
    bs, vs = model.load_model(blob("bert", "tiny", 3), True), model.load_model(blob("vits", "tiny", 5), False)
    pipe, utts = model.Pipeline(bs, vs), _four()
    b = pipe.prepare(utts, forced=True)
    pipe.run(b)
    lens, fetched = [int(v) for v in b.lens], {}
    for name, (fmt, flac, level, q) in FORMS.items():
        gaps = _gaps(fmt)
        place = [0] + list(np.cumsum([n + g for n, g in zip(lens[:-1], gaps[:-1])]))
        if not level:
            fc = pipe.fetch_request(b, range(4), fmt or F(44100, "f32"), place, place[-1] + lens[-1] + gaps[-1], flac=flac, formants=FC(*q))[-1]
            fetched[name] = fc.f_hz.tobytes(), fc.bw_hz.tobytes(), fc.status.tobytes()
    yield dict(bs=bs, vs=vs, utts=utts, fetched=fetched)
    pipe.close(); bs.close(); vs.close()


@gpu
@pytest.mark.parametrize("chunk", [16, 50])
@pytest.mark.parametrize("name", list(FORMS))
def test_stream_formants_on_the_tiny_models(tiny, name, chunk):
    fmt, flac, level, q = FORMS[name]
    ff = fmt or F(44100, "f32")
    kw = dict(fmt=fmt, flac=flac, level=model.StreamLevel(6.0) if level else None, gaps=_gaps(fmt), forced=True, levels=True, env_hop=ff.sample_rate // 100)
    plain = model.StreamHandle(tiny["bs"], tiny["vs"], tiny["utts"], chunk, **kw)
    plain_pieces, plain_marks = [], []
    while (p := plain.next()) is not None:
        plain_pieces.append(p)
        plain_marks.append(plain.next_marks())
    with pytest.raises(model.Sbv2Error, match="begun without a formant contour"):
        plain.next_formants()
    plain.close()
    want = FC(*q)
    model.formant_contour_defaults(ff.sample_rate, want)
    st = model.StreamHandle(tiny["bs"], tiny["vs"], tiny["utts"], chunk, formants=FC(*q), **kw)
    assert st.n_formant_frames == -(-st.total_samples // q[0])
    pieces, marks, parts, at = [], [], [], 0
    while (p := st.next()) is not None:
        pieces.append(p)
        marks.append(st.next_marks())
        first, f, b, status, D = st.next_formants()
        assert first == at and at + len(f) == complete_np(D, st.total_samples, q[0], want.window) and len(b) == len(status) == len(f)
        at += len(f)
        parts.append((f, b, status))
    assert st.next_formants()[1].shape == (0, q[1]) and at == st.n_formant_frames
    st.close()
    assert len(pieces) == len(plain_pieces) and all(bytes(memoryview(a)) == bytes(memoryview(b)) for a, b in zip(pieces, plain_pieces))
    assert all(a[0] == b[0] and a[6] == b[6] and all(a[i].tobytes() == b[i].tobytes() for i in (1, 2, 4, 5)) for a, b in zip(marks, plain_marks))
    got = tuple(np.concatenate([p[i] for p in parts]).tobytes() for i in range(3))
    x = _delivered_samples(pieces, flac)
    hook, _ = model.debug_formant_contour(x, ff.sample_rate, FC(*q), encoding="mulaw" if ff.encoding == "mulaw" else None)
    assert got == (hook.f_hz.tobytes(), hook.bw_hz.tobytes(), hook.status.tobytes()) and hook.f_hz.max() > 0
    assert level or got == tiny["fetched"][name]                                 # ... and the joined fetch's of the same batch
