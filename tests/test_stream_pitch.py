"""The pitch contour of a stream's speech marks: the fed estimator (csrc/marks.hip StreamPitch / k_stream_pitch, sbv2_debug_stream_pitch), the
C ABI (sbv2_stream_begin_request_pitch, sbv2_stream_next_pitch), model.StreamHandle(pitch=), orchestrator.easy_synthesize_stream(pitch=True) and
POST /synthesize_stream_marks with pitch_hz.

The yardstick of every contour is the one-shot estimator over the whole signal (sbv2_debug_pitch, held to numpy by test_pitch.py): a frame's sums
depend on its window and on tau_max only, so a streamed frame has the one-shot frame's bits, whatever the pushes, for every encoding (f32
included).  Every comparison here is bit for bit (tobytes()); nothing has a tolerance.  For the integer encodings the contour is compared with
the numpy restatement of test_pitch.py (yin_ref) as well: lag, voiced and the c values are integers and one rounding, f0 and ap the same IEEE
operations in the same order."""
import base64
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import flac_reader as R
from helpers import blob, make_utts, weights
from sbv2_api_amd import _lib, model, orchestrator, synth
from test_marks import FORCED
from test_pitch import encoded, lags_np, noise, tone, values_of, yin_ref
from test_stream_marks_levels import LINES, STYLES, FakeHandle, level_delivery, rule_np

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["sbv2_stream_begin_request_pitch", "sbv2_stream_next_pitch", "sbv2_debug_stream_pitch"]
f64p, i32p = C.POINTER(C.c_double), C.POINTER(C.c_int32)
FILL = 77.0
F = model.PcmFormat


# ---- the completion rule of the header, stated directly ----------------------------------------------------------------------------------------

def complete_np(D, hop, tau_max, total):
    """Frames f < ceil(total / hop) with min(f hop + hop // 2 + tau_max, total) <= D, as a mask."""
    f = np.arange(-(-total // hop) if total > 0 else 0, dtype=np.int64)
    return np.minimum(f * hop + hop // 2 + tau_max, total) <= D


def per_call_np(delivered, hop, tau_max, total):
    """delivered = D after each call -> per call (first, n): the frames that became complete since the call before."""
    out, at = [], 0
    for D in delivered:
        n = int(complete_np(D, hop, tau_max, total).sum())
        out.append((at, n - at))
        at = n
    return out


# ---- CPU: ABI, refusals, the rule ------------------------------------------------------------------------------------------------------------

def test_new_symbols_are_exported_and_declared():
    header = open(os.path.join(ROOT, "include", "sbv2_hip.h")).read()
    l = _lib.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.SYMBOLS and getattr(l, name) is not None, name
    assert "} sbv2_stream_pitch;" in header and "} sbv2_stream_pitch_part;" in header
    assert C.sizeof(_lib.Sbv2StreamPitch) == 32 and C.sizeof(_lib.Sbv2StreamPitchPart) == 56
    assert C.sizeof(_lib.Sbv2StreamLevels) == 16 and C.sizeof(_lib.Sbv2StreamMarksPart) == 88 and C.sizeof(_lib.Sbv2Pitch) == 72   # as they were
    assert "pitch on a stream (DESIGN.md)" not in header     # no longer listed as not done


def test_begin_and_next_refusals_that_need_no_run():
    l = _lib.lib()
    gap = np.zeros(1, np.int64)
    f8 = F(8000, "s16")
    rq8 = _lib.Sbv2StreamRequest(gap.ctypes.data_as(_lib.i64p), C.pointer(f8.c), None, 0, 0)
    SP = _lib.Sbv2StreamPitch

    def begin(sp, rq=None, lv=None, outs=True):
        h, tot, nt, ne, nq = C.c_void_p(0x55), C.c_int64(-5), C.c_int64(-6), C.c_int64(-7), C.c_int64(-8)
        o = (C.byref(h), C.byref(tot), C.byref(nt), C.byref(ne), C.byref(nq)) if outs else (None,) * 5
        rc = l.sbv2_stream_begin_request_pitch(None, None, None, None, None, None, None, 16, C.byref(rq) if rq is not None else None,
                                               C.byref(lv) if lv is not None else None, C.byref(sp) if sp is not None else None, *o)
        return rc, l.sbv2_last_error().decode(), (h.value, tot.value, nt.value, ne.value, nq.value)

    for sp, rq, word in ((SP(160, 1, 70.0, 600.0, 0.15), None, "reserved"), (SP(0, 0, 70.0, 600.0, 0.15), None, "hop"),
                         (SP(-3, 0, 70.0, 600.0, 0.15), None, "hop"), (SP(160, 0, 39.9, 600.0, 0.15), None, "f0_min"),
                         (SP(160, 0, 600.0, 600.0, 0.15), None, "below f0_max"), (SP(160, 0, 70.0, 600.0, 0.0), None, "threshold"),
                         (SP(160, 0, 70.0, 600.0, 1.0), None, "threshold"), (SP(160, 0, float("nan"), 600.0, 0.15), None, "f0_min"),
                         (SP(160, 0, 70.0, 44100 / 4 + 1, 0.15), None, "f0_max"),       # a NULL request, like a NULL fmt: the identity format's 44100 Hz
                         (SP(80, 0, 70.0, 2000.5, 0.15), rq8, "f0_max")):                # the rate is the format's: 2000.5 > 8000 / 4
        rc, err, outs = begin(sp, rq)
        assert rc != 0 and word in err, (word, err)
        assert outs == (0x55, -5, -6, -7, -8), "a refused call wrote something"
    # the levels' fields are checked as in sbv2_stream_begin_request_levels
    rc, err, _ = begin(SP(160, 0, 70.0, 600.0, 0.15), lv=_lib.Sbv2StreamLevels(2, 0, (C.c_int32 * 2)(0, 0)))
    assert rc != 0 and "tokens" in err
    # everything static passed (2000 Hz is fine at 44100 Hz, and 2000.0 at 8000 Hz): the null handles themselves
    for sp, rq in ((SP(160, 0, 70.0, 2000.0, 0.15), None), (SP(80, 0, 70.0, 2000.0, 0.15), rq8), (None, None)):
        rc, err, _ = begin(sp, rq, outs=False)
        assert rc != 0 and "bad arguments" in err, err
    assert l.sbv2_stream_next_pitch(None, None) != 0 and b"bad arguments" in l.sbv2_last_error()


def _hook(x, enc, cuts, sr, hop, f0_min=70.0, f0_max=600.0, threshold=0.15, device=0, capacity=None, reserved=0):
    """sbv2_debug_stream_pitch with a guard entry around every output -> (rc, namespace-like dict without guards, all arrays)."""
    x = np.ascontiguousarray(x)
    cuts = np.ascontiguousarray(np.asarray(cuts, np.int64).reshape(-1))
    nf = -(-x.size // hop) if x.size and hop > 0 else 0
    f0, ap, lag = np.full(nf + 2, FILL), np.full(nf + 2, FILL), np.full(nf + 2, 77, np.int32)
    c3, voiced, per = np.full((nf + 2, 3), FILL), np.full(nf + 2, 77, np.int32), np.full(cuts.size + 3, 77, np.int64)
    q = _lib.Sbv2Pitch(hop, reserved, f0_min, f0_max, threshold, nf if capacity is None else capacity, C.cast(f0.ctypes.data + 8, f64p),
                       C.cast(ap.ctypes.data + 8, f64p), C.cast(lag.ctypes.data + 4, i32p), -9)
    rc = _lib.lib().sbv2_debug_stream_pitch(device, x.ctypes.data_as(C.c_void_p) if x.size else None, enc, x.size,
                                            cuts.ctypes.data_as(_lib.i64p) if cuts.size else None, cuts.size, sr, C.byref(q),
                                            C.cast(c3.ctypes.data + 24, f64p), C.cast(voiced.ctypes.data + 4, i32p), C.cast(per.ctypes.data + 8, _lib.i64p))
    arrs = [f0, ap, lag, c3, voiced, per]
    got = dict(f0=f0[1:-1], ap=ap[1:-1], lag=lag[1:-1], c3=c3[1:-1], voiced=voiced[1:-1], per=per[1:-1], n_frames=q.n_frames)
    return rc, got, arrs


def test_hook_refusals_that_need_no_run():
    l = _lib.lib()
    x = np.arange(400, dtype=np.int16)
    for cuts, enc, kw, word in (([50, 40], 1, {}, "cuts must ascend"),                   # unsorted
                                ([50, 401], 1, {}, "cuts must ascend"),                  # beyond n
                                ([-1], 1, {}, "cuts must ascend"),
                                ([50], 5, {}, "bad arguments"),                          # an unknown encoding
                                ([50], 1, dict(f0_min=39.9), "f0_min"), ([50], 1, dict(f0_max=2000.5), "f0_max"),
                                ([50], 1, dict(f0_min=600.0), "below f0_max"), ([50], 1, dict(threshold=1.0), "threshold"),
                                ([50], 1, dict(reserved=1), "reserved"), ([50], 1, dict(capacity=4), "too small")):
        rc, got, arrs = _hook(x, enc, cuts, 8000, 80, device=99, **kw)   # (refused before the device is looked at)
        assert rc != 0 and word in l.sbv2_last_error().decode(), (word, l.sbv2_last_error())
        assert all((a == 77).all() for a in arrs) and got["n_frames"] == -9, "a refused call wrote something"
    with pytest.raises(model.Sbv2Error):
        model.debug_stream_pitch(x.astype(np.float64), [], 8000, model.Pitch(80))


@pytest.mark.parametrize("hop", [1, 80, 160, 441, 5000])
def test_completion_rule(hop):
    """model.stream_pitch_complete against the direct statement, for every D: frames complete in order, none twice, all at D = total."""
    for tau_max in (64, 229, 1200):
        for total in (0, 1, tau_max - 1, hop, 7 * hop + 3):
            nf = -(-total // hop) if total > 0 else 0
            f = np.arange(nf, dtype=np.int64)
            pos = np.minimum(f * hop + hop // 2 + tau_max, total)      # where each frame completes: ascending
            assert (np.diff(pos) >= 0).all()
            Ds = np.arange(total + 1, dtype=np.int64)
            want = (pos[None, :] <= Ds[:, None]).sum(axis=1) if nf else np.zeros(total + 1, np.int64)
            got = np.array([model.stream_pitch_complete(int(D), hop, tau_max, total) for D in Ds])
            assert np.array_equal(got, want), (hop, tau_max, total)
            for D in Ds[:: max(1, total // 50)]:                       # the complete ones are the FIRST ones
                m = complete_np(int(D), hop, tau_max, total)
                assert m[:int(m.sum())].all()
            assert (np.diff(got) >= 0).all() and got[-1] == nf          # in order, nothing twice, everything at the end
            calls = per_call_np(list(Ds), hop, tau_max, total)
            assert sum(n for _, n in calls) == nf and all(b[0] == a[0] + a[1] for a, b in zip(calls, calls[1:]))
    assert model.stream_pitch_complete(0, 80, 64, 0) == 0


# ---- CPU: orchestrator, REST and holder on a fake handle ------------------------------------------------------------------------------------

class PitchFakeHandle(FakeHandle):
    """FakeHandle with a contour that follows the completion rule: frame f has f0 = 0 (unvoiced) when f % 3 == 0, else 100 + 7 f."""
    seen = []

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.q = self.kw.get("pitch")
        self.q0 = self.pitch_calls = 0
        if self.q is not None:
            self.tau_max = model.pitch_lags(self.fmt.sample_rate, self.q.f0_min, self.q.f0_max)[1]
            self.n_pitch = -(-self.total_samples // self.q.hop)
            f = np.arange(self.n_pitch)
            self.all_f0 = np.where(f % 3 == 0, 0.0, 100.0 + 7.0 * f)
            self.all_ap = 0.01 * (f + 1)

    def next_pitch(self):
        assert self.q is not None, "next_pitch on a stream begun without pitch"
        self.pitch_calls += 1
        n = int(complete_np(self.D, self.q.hop, self.tau_max, self.total_samples).sum())
        a, self.q0 = self.q0, n
        return a, self.all_f0[a:n].copy(), self.all_ap[a:n].copy(), np.full(n - a, 50, np.int32), self.D


def _filled_pitch(h):
    p = model.Pitch(h.q.hop, h.q.f0_min, h.q.f0_max)
    p.f0, p.ap, p.lag = h.all_f0, h.all_ap, np.full(h.n_pitch, 50, np.int32)
    return p


def _fake_marks(h, hop_env):
    lv = lambda a, b: (float((h.x[a:b].astype(np.float64) ** 2).sum()), float(np.abs(h.x[a:b].astype(np.float64)).max()) if b > a else 0.0)
    tok = [lv(int(a), int(b)) for a, b in zip(h.start, h.end)]
    m = model.Marks(h.start, h.end, np.array([v[0] for v in tok]), np.array([v[1] for v in tok]), env_hop=hop_env, out_len=h.total_samples)
    if hop_env:
        env = [lv(a, min(a + hop_env, h.total_samples)) for a in range(0, h.total_samples, hop_env)]
        m.env_sumsq, m.env_peak = np.array([v[0] for v in env]), np.array([v[1] for v in env])
    return m


def test_orchestrator_pitch_on_a_stream(monkeypatch):
    monkeypatch.setattr(model, "StreamHandle", PitchFakeHandle)
    O = orchestrator
    SO = O.SynthesizeOptions
    args = (None, None, LINES, STYLES, 1, 7)
    # refused before any handle is made: pitch=True without pitch_hz, or without levels=True; pitch_hz without pitch=True as before
    PitchFakeHandle.seen.clear()
    with pytest.raises(model.Sbv2Error, match="pitch_hz"):
        O.easy_synthesize_stream(*args, SO(), noise_seed=5, split=True, levels=True, pitch=True)
    with pytest.raises(model.Sbv2Error, match="levels=True"):
        O.easy_synthesize_stream(*args, SO(pitch_hz=100), noise_seed=5, split=True, pitch=True)
    for kw in (dict(), dict(levels=True)):
        with pytest.raises(model.Sbv2Error, match="/synthesize_marks"):
            O.easy_synthesize_stream(*args, SO(pitch_hz=100), noise_seed=5, split=True, **kw)
    for bad in (SO(pitch_hz=0), SO(pitch_hz=1001), SO(pitch_hz=2.5), SO(pitch_hz=True), SO(pitch_hz=100, pitch_min_hz=39.0),
                SO(pitch_hz=100, pitch_min_hz=700.0)):
        with pytest.raises(model.Sbv2Error):
            O.easy_synthesize_stream(*args, bad, noise_seed=5, split=True, levels=True, pitch=True)
    assert PitchFakeHandle.seen == []
    # the default call and the call with levels do not name pitch
    for kw in (dict(), dict(levels=True)):
        st = O.easy_synthesize_stream(*args, SO(envelope_hz=100), noise_seed=5, split=True, **kw)
        assert "pitch" not in PitchFakeHandle.seen[-1][1]
        h = st._st
        plain = b"".join(st)
        assert h.pitch_calls == 0 and "pitch" not in st.marks and "f0_hz" not in st.marks["tokens"][0]
        if kw:
            assert "pitch" not in st.take_marks()
    for enc, rate in (("f32", 44100), ("s16", 16000)):
        opts = SO(encoding=enc, sample_rate=rate, envelope_hz=100, pitch_hz=100, pitch_min_hz=80.0, pitch_max_hz=500.0)
        plain = b"".join(O.easy_synthesize_stream(*args, SO(encoding=enc, sample_rate=rate), noise_seed=5, split=True))
        st = O.easy_synthesize_stream(*args, opts, noise_seed=5, split=True, levels=True, pitch=True)
        kw = PitchFakeHandle.seen[-1][1]
        q = kw["pitch"]
        hop = rate // 100
        assert kw["levels"] is True and (q.hop, q.f0_min, q.f0_max) == (hop, 80.0, 500.0)
        h, got, f0, ap, firsts, sizes, delivered = st._st, [], [], [], [], [], []
        assert st.marks["pitch"] == {"hop": hop, "f0_hz": [], "aperiodicity": []}
        for i, piece in enumerate(st):
            got.append(piece)
            d = st.take_marks()
            json.dumps(d)
            assert d["pitch"]["first"] == len(f0) and d["pitch"]["hop"] == hop and set(d["pitch"]) == {"first", "hop", "f0_hz", "aperiodicity"}
            if i % 2 == 0:      # (not asking loses nothing, asking twice gives nothing twice)
                d2 = st.take_marks()
                assert d2["pitch"]["f0_hz"] == [] and d2["pitch"]["first"] == d["pitch"]["first"] + len(d["pitch"]["f0_hz"])
            f0 += d["pitch"]["f0_hz"]; ap += d["pitch"]["aperiodicity"]
            firsts.append(d["pitch"]["first"]); sizes.append(len(d["pitch"]["f0_hz"])); delivered.append(d["delivered"])
        assert b"".join(got) == plain                                  # the audio is that of the call without
        assert st.take_marks()["pitch"]["f0_hz"] == []
        # the pieces' blocks concatenate to the final block, which is marks_dict's, tokens' f0_hz / voiced included
        want = O.marks_dict([s for s in LINES if s], [0, 2], model.PcmFormat(rate, enc), _fake_marks(h, hop), _filled_pitch(h))
        assert st.marks == want
        assert f0 == want["pitch"]["f0_hz"] and ap == want["pitch"]["aperiodicity"] and len(f0) == h.n_pitch == -(-h.total_samples // hop)
        assert None in f0 and any(v for v in f0) and firsts == sorted(firsts) and firsts[0] == 0
        assert any(t["f0_hz"] is not None for t in want["tokens"]) and all("voiced" in t for t in want["tokens"])
        # the frames came by the rule: with D samples out, exactly the frames complete at D (the header piece delivers nothing)
        tau_max = lags_np(rate, 80.0, 500.0)[1]
        assert list(zip(firsts, sizes)) == per_call_np(delivered, hop, tau_max, h.total_samples) and delivered[0] == 0
        assert delivered[-1] == h.total_samples and sizes[0] == 0 and sum(sizes) == h.n_pitch


def test_rest_stream_marks_with_pitch(monkeypatch):
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient
    from sbv2_api_amd import rest
    monkeypatch.setattr(model, "StreamHandle", PitchFakeHandle)

    class Holder:
        calls = []

        def models(self):
            return ["m"]

        def easy_synthesize_stream(self, ident, text, style_id, speaker_id, options, **kw):
            self.calls.append(kw)
            return orchestrator.easy_synthesize_stream(None, None, LINES, STYLES, style_id, speaker_id, options, noise_seed=5, **kw)

    h = Holder()
    c = TestClient(rest.make_app(h))
    body = {"text": "a\n\nb", "ident": "m", "split_sentences": True, "sample_rate": 16000, "encoding": "s16"}
    plain = c.post("/synthesize_stream", json=body)
    assert plain.status_code == 200 and h.calls[-1] == {"split": True}
    # without pitch_hz the holder is called as it always was, and no line has a pitch block
    r = c.post("/synthesize_stream_marks", json=dict(body, envelope_hz=100))
    assert r.status_code == 200 and h.calls[-1] == {"levels": True, "split": True}
    assert all("pitch" not in json.loads(s) for s in r.content.decode().splitlines())
    r = c.post("/synthesize_stream_marks", json={k: v for k, v in body.items() if k != "split_sentences"})
    assert r.status_code == 500 and h.calls[-1] == {"levels": True}        # (two live lines unsplit: refused, but called with levels alone)
    # with pitch_hz: pitch=True, the opening line names the contour, the pieces carry it
    r = c.post("/synthesize_stream_marks", json=dict(body, envelope_hz=100, pitch_hz=100, pitch_min_hz=80.0))
    assert r.status_code == 200 and h.calls[-1] == {"levels": True, "split": True, "pitch": True}
    lines = [json.loads(s) for s in r.content.decode().splitlines()]
    first, rest_ = lines[0], lines[1:]
    n_frames = -(-737 // 160)
    assert first["total_samples"] == 737 and first["pitch"] == {"hop": 160, "n_frames": n_frames}
    assert set(first["marks"]) == {"sample_rate", "tokens", "words"}
    assert b"".join(base64.b64decode(l["audio"]) for l in rest_) == plain.content
    at = 0
    for l in rest_:
        assert l["pitch"]["first"] == at and l["pitch"]["hop"] == 160 and len(l["pitch"]["f0_hz"]) == len(l["pitch"]["aperiodicity"])
        at += len(l["pitch"]["f0_hz"])
    assert at == n_frames and rest_[-1]["delivered"] == 737
    tau_max = lags_np(16000, 80.0, 600.0)[1]
    assert [(l["pitch"]["first"], len(l["pitch"]["f0_hz"])) for l in rest_] == per_call_np([l["delivered"] for l in rest_], 160, tau_max, 737)
    assert sum(len(l["envelope"]["peak"]) for l in rest_) == n_frames and [t["token"] for l in rest_ for t in l["tokens"]] == list(range(8))
    # a bad pitch_hz: the error mapping, and the lock is given back
    r = c.post("/synthesize_stream_marks", json=dict(body, pitch_hz=0))
    assert r.status_code == 500 and "pitch_hz" in r.text
    # /synthesize_stream keeps refusing the field, naming the route that carries a whole-signal contour
    r = c.post("/synthesize_stream", json=dict(body, pitch_hz=100))
    assert r.status_code == 500 and "/synthesize_marks" in r.text and h.calls[-1] == {"split": True}
    assert c.post("/synthesize_stream", json=body).content == plain.content


def test_holder_passes_pitch_through(monkeypatch):
    """The real TTSModelHolder (fake sessions) in front of the real orchestrator: pitch=True reaches the handle, the default does not name it."""
    from sbv2_api_amd import holder
    monkeypatch.setattr(model, "StreamHandle", PitchFakeHandle)
    by_text = {"one": LINES[0], "two": LINES[2]}
    hd = holder.TTSModelHolder(b"bert", parse_text=lambda s: by_text[s], load_session=lambda data, is_bert: object(),
                               make_pipeline=lambda bert, vits: None)
    hd.load("m", json.dumps({"shape": [2, 4], "data": STYLES.tolist()}).encode(), b"vits")
    opts = orchestrator.SynthesizeOptions(envelope_hz=100)
    PitchFakeHandle.seen.clear()
    want = b"".join(hd.easy_synthesize_stream("m", "one\n\ntwo", 1, 0, opts, noise_seed=3, split=True))
    assert "pitch" not in PitchFakeHandle.seen[-1][1] and "levels" not in PitchFakeHandle.seen[-1][1]
    lv = hd.easy_synthesize_stream("m", "one\n\ntwo", 1, 0, opts, noise_seed=3, split=True, levels=True)
    assert "pitch" not in PitchFakeHandle.seen[-1][1] and PitchFakeHandle.seen[-1][1]["levels"] is True
    lv.close()
    opts = orchestrator.SynthesizeOptions(envelope_hz=100, pitch_hz=50)
    st = hd.easy_synthesize_stream("m", "one\n\ntwo", 1, 0, opts, noise_seed=3, split=True, levels=True, pitch=True)
    q = PitchFakeHandle.seen[-1][1]["pitch"]
    assert (q.hop, q.f0_min, q.f0_max) == (44100 // 50, 70.0, 600.0)
    assert b"".join(st) == want
    d = st.take_marks()
    assert len(d["pitch"]["f0_hz"]) == len(st.marks["pitch"]["f0_hz"]) == -(-st.total_samples // 882) and "voiced" in st.marks["tokens"][0]
    with pytest.raises(model.Sbv2Error, match="pitch_hz"):
        hd.easy_synthesize_stream("m", "one\n\ntwo", 1, 0, orchestrator.SynthesizeOptions(), noise_seed=3, split=True, levels=True, pitch=True)
    assert hd._find("m").streams == 0     # every stream gave the model back, the refused one included


# ---- GPU, the hook: bit equality with the one-shot estimator -----------------------------------------------------------------------------------

# (rate, f0_min, f0_max, tau_max, encoding, lanes, P): the three launch widths and 1, 3 and 5 lags per lane
CASES = [(8000, 125.0, 2000.0, 64, "s16", 64, 1), (8000, 70.0, 600.0, 115, "mulaw", 128, 1), (8000, 70.0, 600.0, 115, "alaw", 128, 1),
         (16000, 70.0, 600.0, 229, "s16", 256, 1), (16000, 70.0, 600.0, 229, "f32", 256, 1), (44100, 70.0, 600.0, 630, "f32", 256, 3),
         (48000, 40.0, 600.0, 1200, "s16", 256, 5)]
N_HOP1 = 61   # the short signal that takes hop = 1: one frame per sample, every one reading zeros on both sides of the signal
NUMPY_BUDGET = 4e8   # frames x tau_max^2 up to which the numpy restatement is run beside the one shot (its cost: a few seconds beyond)


def _case_signal(rate, tau_max, encoding, n):
    """A harmonic tone plus noise with a silent stretch in it; at 48 kHz the full-scale square wave of half-period 1200 (test_pitch.py's bound
    case: d tau above 2^52) with the silent stretch."""
    sec = n / rate + 0.01
    if tau_max == 1200:
        x = np.where((np.arange(n) // 1200) % 2 == 0, -32768, 32767).astype(np.int16)
    else:
        t = tone(173.9 if rate > 8000 else 261.6, rate, sec)[:n].astype(np.int64)
        x = np.clip(t + noise(rate, 21, sec)[:n].astype(np.int64) // 2, -32768, 32767).astype(np.int16)
    if n > 4 * tau_max:
        x[n // 2:n // 2 + 2 * tau_max + 9] = 0
    if encoding == "f32":
        rng = np.random.default_rng(8)
        return (x.astype(np.float64) / 32768.0 * (1.0 + 0.01 * rng.standard_normal(n))).astype(np.float32)   # (not s16 / 32768: sums that round)
    return encoded(x, encoding)


def _cut_sets(n, hop, W, rng):
    """Cut lists for a signal of n samples (each ascending within [0, n])."""
    nf = -(-n // hop)
    pos = np.minimum(np.arange(nf, dtype=np.int64) * hop + hop // 2 + W, n)
    clip = lambda a: sorted(int(v) for v in a if 0 <= v <= n)
    sets = {"none": [], "at every completion": clip(pos), "completion - 1": clip(pos - 1), "completion + 1": clip(pos + 1),
            "empty pushes": clip([0, 0, 0, n // 3, n // 3, n // 3, n, n]),
            "random": clip(sorted(rng.integers(0, n + 1, 12)) if n else [])}
    if n > 45:
        s = max(0, min(n - 41, W + hop // 2 - 20))     # around the first frame's completion where it lies inside
        sets["40 one-sample pushes"] = list(range(s, s + 41))
    if n > 2 * W:
        sets["pushes of 2 tau_max"] = list(range(2 * W, n, 2 * W))
    if n > 6 * W + 3:
        sets["three carry lengths then one sample"] = [n - 1 - 6 * W, n - 1]
    return sets


@gpu
@pytest.mark.parametrize("rate,f0_min,f0_max,tau_max,encoding,lanes,P", CASES, ids=[f"{c[0]}-{c[3]}-{c[4]}" for c in CASES])
def test_fed_estimator_has_the_bits_of_the_one_shot(rate, f0_min, f0_max, tau_max, encoding, lanes, P):
    assert model.pitch_lags(rate, f0_min, f0_max)[1] == tau_max == lags_np(rate, f0_min, f0_max)[1]
    assert lanes == (64 if tau_max <= 64 else 128 if tau_max <= 128 else 256) and P == -(-tau_max // lanes)
    law = encoding if encoding in ("mulaw", "alaw") else None
    enc = model.ENCODINGS[encoding]
    rng = np.random.default_rng(31)
    W, hop100 = tau_max, rate // 100
    n_main = 6 * 2 * W + 37
    # (W + 25 at hop 1 besides the short signal: there the frames complete one per sample, not all with the end)
    shapes = [(n_main, hop100), (n_main, 2 * W + 3), (1, hop100), (W - 1, hop100), (2 * W, hop100), (hop100, hop100), (N_HOP1, 1), (W + 25, 1)]
    runs, voiced_seen, unvoiced_seen = 0, False, False
    for n, hop in shapes:
        x = _case_signal(rate, W, encoding, n)
        p, c3, voiced = model.debug_pitch(x, rate, model.Pitch(hop, f0_min, f0_max), encoding=law)      # the one shot: once per shape
        nf = -(-n // hop)
        assert len(p.f0) == nf
        if encoding != "f32" and ((n, hop) != (W + 25, 1) or nf * W * W <= NUMPY_BUDGET):     # ... itself equal to the numpy restatement
            ref = yin_ref(values_of(x, law), rate, hop, f0_min, f0_max)
            assert np.array_equal(p.lag, ref.lag) and np.array_equal(voiced, ref.voiced) and c3.tobytes() == ref.c3.tobytes(), (n, hop)
            assert p.f0.tobytes() == ref.f0.tobytes() and p.ap.tobytes() == ref.ap.tobytes(), (n, hop)
            if W == 1200 and n == n_main:
                assert 2 ** 52 < ref.max_dtau < 2 ** 53
        voiced_seen |= bool(voiced.any()); unvoiced_seen |= bool((voiced == 0).any())
        for name, cuts in _cut_sets(n, hop, W, rng).items():
            rc, got, arrs = _hook(x, enc, cuts, rate, hop, f0_min, f0_max)
            what = f"{rate} {encoding} n={n} hop={hop} cuts={name}"
            assert rc == 0, (what, _lib.lib().sbv2_last_error())
            assert all((a[0] == 77).all() and (a[-1] == 77).all() for a in arrs), what + ": guard entries"
            assert got["n_frames"] == nf, what
            assert np.array_equal(got["lag"], p.lag) and np.array_equal(got["voiced"], voiced), (what, np.flatnonzero(got["lag"] != p.lag)[:8])
            assert got["c3"].tobytes() == c3.tobytes(), (what, np.flatnonzero((got["c3"] != c3).any(axis=1))[:8])
            assert got["f0"].tobytes() == p.f0.tobytes() and got["ap"].tobytes() == p.ap.tobytes(), what
            want = per_call_np(list(cuts) + [n], hop, W, n)
            assert list(got["per"][:len(cuts) + 1]) == [w[1] for w in want], what
            runs += 1
    assert runs >= 8 * 6 + 6 and unvoiced_seen and (voiced_seen or W == 1200)     # (the square wave's period lies beyond tau_max)
    # the wrapper gives the same answer
    x = _case_signal(rate, W, encoding, n_main)
    a = model.debug_pitch(x, rate, model.Pitch(hop100, f0_min, f0_max), encoding=law)
    b = model.debug_stream_pitch(x, [5, 5, W, 3 * W + 1], rate, model.Pitch(hop100, f0_min, f0_max), encoding=law)
    assert a[0].f0.tobytes() == b[0].f0.tobytes() and a[1].tobytes() == b[1].tobytes() and int(b[3].sum()) == len(a[0].f0)


# ---- GPU: streams of the tiny models (the fixture pattern of test_stream_marks_levels.py) -------------------------------------------------------

LONG_ROW = [2, 300, 0, 1, 5]
ROWS = FORCED + [LONG_ROW]
GAPS = (64, 22050, 100, 0)
# The tiny decoder's halo holds no filter below 24 kHz (a stream at 8 or 16 kHz on it is refused, as test_flac_stream.py notes), so the G.711
# stream with the range 100 - 400 Hz and the 200-frame chunks runs at 24 kHz here and at 8 kHz on the full-size models below.
STREAMS = {   # name -> (fmt or None = the identity format, flac, level, (f0_min, f0_max), chunk sizes)
    "identity": (None, False, False, (70.0, 600.0), (16, 50)), "48k-s16": (F(48000, "s16"), False, False, (70.0, 600.0), (16, 50)),
    "24k-mulaw": (F(24000, "mulaw"), False, False, (100.0, 400.0), (16, 50, 200)), "flac": (F(48000, "s16"), True, False, (70.0, 600.0), (16, 50)),
    "level-f32": (F(48000, "f32"), False, True, (70.0, 600.0), (16, 50)), "level-s16-flac": (F(48000, "s16"), True, True, (70.0, 600.0), (16, 50)),
}


def _gaps(fmt):
    mg = model.stream_min_gap(fmt)
    return tuple(max(g, mg) if i < len(GAPS) - 1 else g for i, g in enumerate(GAPS))


def _four():
    bc, _ = weights("bert", "tiny", 3)
    vc, _ = weights("vits", "tiny", 5)
    utts = make_utts([4, 5, 6, 2], bc, vc, seed0=811, with_bert=False)
    assert [len(u["phones"]) for u in utts] == [len(d) for d in ROWS]
    return [dict(u, forced_durations=np.array(d, np.int64)) for u, d in zip(utts, ROWS)]


@pytest.fixture(scope="module")
def tiny():
    """The two tiny sessions and, fetched from ONE pipeline run before any stream reuses the sessions, the contour of the joined fetch in every
    format a non-level stream below delivers."""
    bs, vs = model.load_model(blob("bert", "tiny", 3), True), model.load_model(blob("vits", "tiny", 5), False)
    hop = _lib.lib().sbv2_vits_hop(vs.handle)
    assert hop == 16
    pipe = model.Pipeline(bs, vs)
    utts = _four()
    b = pipe.prepare(utts, forced=True)
    pipe.run(b)
    lens = [int(n) for n in b.lens]
    fetched = {}
    for name, (fmt, flac, level, (lo, hi), _) in STREAMS.items():
        ff = fmt or F(44100, "f32")
        gaps, place = _gaps(fmt), [0]
        for n, g in zip(lens[:-1], gaps[:-1]):
            place.append(place[-1] + n + g)
        joined = place[-1] + lens[-1] + gaps[-1]
        if not level and (ff.sample_rate, ff.encoding) not in fetched:
            out, _, _, p = pipe.fetch_request(b, range(4), ff, place, joined, pitch=model.Pitch(ff.sample_rate // 100, lo, hi))
            fetched[(ff.sample_rate, ff.encoding)] = (out.copy(), p)
    yield dict(bs=bs, vs=vs, hop=hop, utts=utts, frames=[n // hop for n in lens], fetched=fetched)
    pipe.close(); bs.close(); vs.close()


def _take(st, levels, short_at=None):
    """Every piece of the stream, sbv2_stream_next_pitch (and with levels sbv2_stream_next_marks) after each -> (pieces, per call (first, n,
    delivered), (f0, ap, lag), the next_marks results).  short_at = (call, pending): there a capacity one short and a NULL f0 are tried first:
    refused, nothing written, nothing lost."""
    l = _lib.lib()
    pieces, calls, acc, marks = [], [], [[], [], []], []
    while (p := st.next()) is not None:
        if short_at is not None and len(pieces) == short_at[0]:
            n = short_at[1]
            for cap, null_f0, word in ((n - 1, False, "pitch arrays too small"), (n, True, "NULL f0")):
                f0, ap, lag = np.full(n + 2, FILL), np.full(n + 2, FILL), np.full(n + 2, 77, np.int32)
                part = _lib.Sbv2StreamPitchPart(cap, None if null_f0 else C.cast(f0.ctypes.data + 8, f64p), C.cast(ap.ctypes.data + 8, f64p),
                                                C.cast(lag.ctypes.data + 4, i32p), -3, -3, -3)
                assert l.sbv2_stream_next_pitch(st.h, C.byref(part)) != 0 and word in l.sbv2_last_error().decode(), l.sbv2_last_error()
                assert all((a == 77).all() for a in (f0, ap, lag)) and (part.first, part.n, part.delivered) == (-3, -3, -3)
        pieces.append(p)
        if levels:
            marks.append(st.next_marks())
        first, f0, ap, lag, D = st.next_pitch()
        calls.append((first, len(f0), D))
        for a, v in zip(acc, (f0, ap, lag)):
            a.append(v)
    first, f0, _, _, D = st.next_pitch()     # after the end: nothing is pending
    assert len(f0) == 0 and first == st.n_pitch and D == st.total_samples
    return pieces, calls, [np.concatenate(a) for a in acc], marks


def _delivered_samples(pieces, flac):
    return R.read(b"".join(pieces))["samples"].astype(np.int16) if flac else np.concatenate(pieces)


def _same_marks(a, b):
    return len(a) == len(b) and all(x[0] == y[0] and x[3] == y[3] and x[6] == y[6] and all(x[i].tobytes() == y[i].tobytes() for i in (1, 2, 4, 5))
                                    for x, y in zip(a, b))


def _check_streams(bs, vs, utts, gaps, name, fmt, flac, level, lo, hi, chunks, call_samples, fetched=None):
    """The stream `name` at every chunk size, with pitch alone and with pitch and levels, against the same stream without.
    call_samples(chunk, plain_pieces) -> the samples every call covers."""
    ff = fmt or F(44100, "f32")
    lv = model.StreamLevel(6.0) if level else None
    p_hop = env_hop = ff.sample_rate // 100
    law = ff.encoding if ff.encoding in model.G711 else None
    W = model.pitch_lags(ff.sample_rate, lo, hi)[1]
    longest = shortest = None
    for chunk in chunks:
        kw = dict(fmt=fmt, flac=flac, level=lv, gaps=gaps, forced=True)
        what = f"{name} chunk {chunk}"
        plain = model.StreamHandle(bs, vs, utts, chunk, **kw)
        plain_spans, plain_pieces = plain.marks(), []
        while (p := plain.next()) is not None:
            plain_pieces.append(p)
        with pytest.raises(model.Sbv2Error, match="begun without pitch"):
            plain.next_pitch()
        plain.close()
        with_levels = model.StreamHandle(bs, vs, utts, chunk, levels=True, env_hop=env_hop, **kw)
        level_marks = []
        while with_levels.next() is not None:
            level_marks.append(with_levels.next_marks())
        with pytest.raises(model.Sbv2Error, match="begun without pitch"):
            with_levels.next_pitch()
        with_levels.close()
        cs = np.asarray(call_samples(chunk, plain_pieces), np.int64)
        total = int(cs.sum())
        D = level_delivery(cs, model.stream_level_lookahead(ff)) if level else [int(v) for v in np.cumsum(cs)]
        longest, shortest = max(longest or 0, int(cs.max())), min(shortest or total, int(cs.min()))
        want = per_call_np(D, p_hop, W, total)
        short = next((i, n) for i, (_, n) in enumerate(want) if n >= 1)
        x = contour = None
        for levels in (False, True):
            st = model.StreamHandle(bs, vs, utts, chunk, pitch=model.Pitch(p_hop, lo, hi), **(dict(levels=True, env_hop=env_hop) if levels else {}), **kw)
            assert st.total_samples == total and st.n_pitch == -(-total // p_hop), what
            assert (st.n_tokens > 0 and st.n_env > 0) if levels else (st.n_tokens == 0 and st.n_env == 0), what
            s, e = st.marks()
            assert np.array_equal(s, plain_spans[0]) and np.array_equal(e, plain_spans[1]), what             # sbv2_stream_marks is unchanged
            if not levels:
                with pytest.raises(model.Sbv2Error, match="begun without levels"):
                    st.next_marks()
            pieces, calls, (f0, ap, lag), marks = _take(st, levels, short)
            st.close()
            # the audio is that of the same stream without pitch, and so are the levels
            assert len(pieces) == len(plain_pieces) and all(bytes(memoryview(a)) == bytes(memoryview(b)) for a, b in zip(pieces, plain_pieces)), what
            assert not levels or _same_marks(marks, level_marks), what
            # the frames came by the rule
            assert [c[:2] for c in calls] == want and [c[2] for c in calls] == D, what
            # the contour is the one-shot contour of the delivered samples
            if x is None:
                x = _delivered_samples(pieces, flac)
                assert x.size == total
                contour = model.debug_pitch(x, ff.sample_rate, model.Pitch(p_hop, lo, hi), encoding=law)[0]
            assert f0.tobytes() == contour.f0.tobytes() and ap.tobytes() == contour.ap.tobytes() and lag.tobytes() == contour.lag.tobytes(), \
                (what, levels, np.flatnonzero(lag != contour.lag)[:8])
            assert (f0 == 0).any() and len(set(lag.tolist())) > 1, what     # (the silent gaps are unvoiced)
        if fetched is not None:   # ... and, the audio being byte-equal to the joined fetch, the fetch's contour
            out, p = fetched
            assert out.tobytes() == x.tobytes(), what
            assert p.f0.tobytes() == f0.tobytes() and p.ap.tobytes() == ap.tobytes() and p.lag.tobytes() == lag.tobytes(), what
    return W, longest, shortest


@gpu
@pytest.mark.parametrize("name", list(STREAMS))
def test_stream_pitch_on_the_tiny_models(tiny, name):
    fmt, flac, level, (lo, hi), chunks = STREAMS[name]
    ff = fmt or F(44100, "f32")
    gaps = _gaps(fmt)
    cs = lambda chunk, _: model.stream_timeline(tiny["frames"], gaps, tiny["hop"], chunk, fmt)[2]
    W, longest, shortest = _check_streams(tiny["bs"], tiny["vs"], tiny["utts"], gaps, name, fmt, flac, level, lo, hi, chunks, cs,
                                          None if level else tiny["fetched"][(ff.sample_rate, ff.encoding)])
    # every stream has pushes shorter than the carry (the new carry is part old carry, part x) and one longer (the one that holds the 22050-sample
    # gap); with 200-frame chunks a chunk of audio alone is longer
    assert shortest < 2 * W < longest and (200 not in chunks or 200 * tiny["hop"] * ff.sample_rate // 44100 > 2 * W)


@pytest.fixture(scope="module")
def full_models():
    bs, vs = model.load_model(blob("bert", "full"), True), model.load_model(blob("vits", "full"), False)
    yield weights("bert", "full")[0], weights("vits", "full")[0], bs, vs
    bs.close(); vs.close()


@gpu
def test_full_model_stream_pitch(full_models):
    """Two rows (60 and 30 phonemes), gap 22050, chunk 64, 16 kHz s16 on the full-size models (as test_full_model_stream_levels): the contour
    equals the one-shot contour of the delivered samples."""
    bc, vc, bs, vs = full_models
    utts = [synth.make_utterance(60, bc, vc, seed=91), synth.make_utterance(30, bc, vc, seed=92)]
    st = model.StreamHandle(bs, vs, utts, 64, fmt=F(16000, "s16"), gaps=(22050, 0), pitch=model.Pitch(160), forced=True)
    pieces, calls, (f0, ap, lag), _ = _take(st, False)
    st.close()
    x = np.concatenate(pieces)
    assert x.size == st.total_samples and len(pieces) > 2
    p = model.debug_pitch(x, 16000, model.Pitch(160))[0]
    assert f0.tobytes() == p.f0.tobytes() and ap.tobytes() == p.ap.tobytes() and lag.tobytes() == p.lag.tobytes()
    assert len(f0) == -(-x.size // 160)


@gpu
def test_full_model_stream_pitch_8k_mulaw(full_models):
    """8 kHz mu-law, 100 - 400 Hz, chunks of 16, 50 and 200 frames on the full-size models, whose halo holds the 8 kHz filter: everything the tiny
    streams are held to but the fetch (the full-size stream is within one step of the fetch, not equal to it)."""
    bc, vc, bs, vs = full_models
    utts = [synth.make_utterance(60, bc, vc, seed=91), synth.make_utterance(30, bc, vc, seed=92)]
    fmt = F(8000, "mulaw")
    W, longest, _ = _check_streams(bs, vs, utts, (22050, 0), "full 8k-mulaw", fmt, False, False, 100.0, 400.0, (16, 50, 200),
                                   lambda chunk, pieces: [p.size for p in pieces])
    assert W == 80 and longest > 2 * W
