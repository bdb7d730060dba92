"""Per-token pitch targets (sbv2_token_pitch, sbv2_pipeline_fetch_request_token_pitch, sbv2_debug_voice_tokens; the token phase of k_voice_marks in
csrc/voice.hip): the ABI and its host-side refusals, a numpy restatement of the definition judged as an editor, the orchestrator / batcher / REST
contracts against fakes (CPU); the kernels against that restatement bit for bit, and the pipeline, batcher and REST on tiny models (GPU).

The reference is `token_ref` below: the section above sbv2_token_pitch in include/sbv2_hip.h restated in numpy in front of the shifter of
tests/test_voice.py (whose helpers, signals and YIN restatement are imported, not copied).  Given a contour, everything behind it is integer
arithmetic and f64 arithmetic in a stated order, so the GPU tests hand the device's own period_out / voiced_out to the reference and compare ta,
ts and map for equality and y, R_f, applied and src_f0 bit for bit.

As an editor the restatement is held to 1.5 x what it measured when this file was written for the token means and the median frame error, and
to 0.9 x the measured share of frames voiced in both contours (see test_the_reference_edits_the_tokens for the figures).  The share is lower than
the global scale's: a frame whose YIN window straddles a ratio step sees two periods and goes unvoiced."""
import ctypes as C
import functools
import os
import re
import types

import numpy as np
import pytest

import flac_reader as R
from helpers import blob, make_utts, weights
from sbv2_api_amd import _lib, batcher, model, orchestrator, synth
from test_voice import (F0_MAX, F0_MIN, FakePipe, REQUEST, STYLES, _join, _payload, five_rows, lags_np, signal, signal_contour,  # noqa: F401
                        voice_ref, yin_ref)

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["sbv2_pipeline_fetch_request_token_pitch", "sbv2_debug_voice_tokens"]
SIGNALS = [(44100, 220), (16000, 80)]
TOKEN_MS = (50, 115, 185, 250, 300, 400, 500)
HZ = [0.0, 180.0, 0.0, 120.0, 0.0, 200.0, 150.0, 0.0]
RATIOS = [0.0, 1.3, 0.0, 0.8, 0.0, 1.0, 1.5, 0.0]
f64p, i32p, i64p = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)


# ---- the reference ----------------------------------------------------------------------------------------------------------------------------------

def token_ends(sr, n):
    """The eight tokens of `signal`: ends at 50, 115, 185, 250, 300, 400, 500 ms and the signal's end, in samples."""
    return np.array([int(round(t * sr / 1000.0)) for t in TOKEN_MS] + [n], np.int64)


def token_ratios_ref(n, sr, p, s, hop, period, voiced, ends, values, kind, smooth):
    """The token stage as include/sbv2_hip.h states it -> namespace(ratio [nf] = R_f, applied, src_f0 [nt], tok [nf] = the frame's token, nt for
    none, m = the row's mean)."""
    nf = -(-n // hop) if n else 0
    ends, values = np.asarray(ends, np.int64).reshape(-1), np.asarray(values, np.float64).reshape(-1)
    nt = ends.size
    assert values.size == nt
    period, voiced = np.asarray(period, np.float64)[:nf], np.asarray(voiced)[:nf] != 0
    f0 = float(sr) / np.where(voiced, period, 1.0)
    q = np.where(voiced, np.rint(f0 * 65536.0), 0.0).astype(np.int64)
    m = float(int(q.sum())) / (65536.0 * float(int(voiced.sum()))) if voiced.any() else 0.0
    centre = np.minimum(np.arange(nf, dtype=np.int64) * hop + hop // 2, n - 1)
    tok = np.searchsorted(ends, centre, side="right")                            # the first token whose end lies behind the centre
    rho_t, src = np.full(nt, 65536, np.int64), np.zeros(nt)
    for t in range(nt):
        sel = (tok == t) & voiced
        c = int(sel.sum())
        M = float(int(q[sel].sum())) / (65536.0 * float(c)) if c else 0.0
        src[t] = M
        v = float(values[t])
        if v == 0.0:
            continue
        if kind == 0:
            rho_t[t] = int(np.rint(v * 65536.0))
        elif c:
            G = np.float64(p * (m + s * (M - m)))
            with np.errstate(divide="ignore"):
                r = np.minimum(np.maximum(np.float64(v) / G, 0.5), 2.0)
            rho_t[t] = int(np.rint(r * 65536.0))
    rho_f = np.where(tok < nt, rho_t[np.minimum(tok, nt - 1)], 65536) if nt else np.full(nf, 65536, np.int64)
    cs = np.concatenate([[0], np.cumsum(rho_f)]).astype(np.int64)
    f = np.arange(nf)
    i0, i1 = np.maximum(f - smooth, 0), np.minimum(f + smooth, nf - 1)
    ratio = (cs[i1 + 1] - cs[i0]).astype(np.float64) / (65536.0 * (i1 - i0 + 1).astype(np.float64)) if nf else np.zeros(0)
    return types.SimpleNamespace(ratio=ratio, applied=rho_t.astype(np.float64) / 65536.0, src_f0=src, tok=tok, m=m)


def token_ref(x, sr, p, s, hop, period, voiced, ends, values, kind, smooth, f0_min=F0_MIN, f0_max=F0_MAX):
    """The shifter of include/sbv2_hip.h with the per-token factor R_f in its target -> namespace(y, ta, ts, map, ratio, applied, src_f0, g, tok):
    voice_ref of tests/test_voice.py with g_f = R_f (p (m + s (f0_f - m))); g [nf] is the clamped target (0 on unvoiced frames)."""
    x = np.asarray(x)
    assert x.dtype == np.float32
    n = x.size
    nf = -(-n // hop) if n else 0
    tr = token_ratios_ref(n, sr, p, s, hop, period, voiced, ends, values, kind, smooth)
    period, voiced = np.asarray(period, np.float64)[:nf], np.asarray(voiced)[:nf] != 0
    none = types.SimpleNamespace(y=x.copy(), ta=np.zeros(0, np.int64), ts=np.zeros(0, np.int64), map=np.zeros(0, np.int64), ratio=tr.ratio,
                                 applied=tr.applied, src_f0=tr.src_f0, g=np.zeros(nf), tok=tr.tok, m=tr.m)
    if n == 0:
        return none
    T = np.where(voiced, period, 1.0)
    f0 = float(sr) / T
    inc_u = int(np.rint(4294967296.0 / float(sr // 200)))
    m = tr.m
    g = tr.ratio * (p * (m + s * (f0 - m)))
    g = np.minimum(np.maximum(g, f0_min / 2.0), 2.0 * f0_max)
    none.g = np.where(voiced, g, 0.0)
    Tp = float(sr) / g
    inc_a = np.where(voiced, np.rint(4294967296.0 / T).astype(np.int64), inc_u)
    inc_s = np.where(voiced, np.rint(4294967296.0 / Tp).astype(np.int64), inc_u)
    frame = np.arange(n) // hop
    phi_a = np.cumsum(inc_a[frame])
    mark_a = (phi_a >> 32) != (np.concatenate([[0], phi_a[:-1]]) >> 32)
    vs = voiced[frame]
    phi_s = phi_a.copy()
    starts = np.nonzero(vs & ~np.concatenate([[False], vs[:-1]]))[0]
    stops = np.nonzero(vs & ~np.concatenate([vs[1:], [False]]))[0] + 1
    for k0, k1 in zip(starts, stops):                                            # a voiced run: phi_s(k0 - 1) = phi_a(k0 - 1)
        base = int(phi_a[k0 - 1]) if k0 > 0 else 0
        phi_s[k0:k1] = base + np.cumsum(inc_s[frame[k0:k1]])
    mark_s = np.where(vs, (phi_s >> 32) != (np.concatenate([[0], phi_s[:-1]]) >> 32), mark_a)
    ta, ts = np.nonzero(mark_a)[0], np.nonzero(mark_s)[0]
    if ta.size == 0:
        return none
    hi = np.searchsorted(ta, ts)
    lo = np.maximum(hi - 1, 0)
    hi = np.minimum(hi, ta.size - 1)
    mp = np.where(ts - ta[lo] <= ta[hi] - ts, lo, hi)
    mp = np.where(ts <= ta[0], 0, np.where(ts >= ta[-1], ta.size - 1, mp))
    num, den = np.zeros(n), np.zeros(n)
    xd = x.astype(np.float64)
    for j in range(ts.size):
        mm = int(mp[j])
        a = int(ta[mm])
        L = a - int(ta[mm - 1]) if mm > 0 else a + 1
        Rr = int(ta[mm + 1]) - a if mm + 1 < ta.size else n - a
        u = np.arange(-L + 1, Rr)
        k = int(ts[j]) + u
        ok = (k >= 0) & (k < n)
        u, k = u[ok], k[ok]
        v = np.abs(u).astype(np.float64) / np.where(u < 0, float(L), float(Rr))
        w = 1.0 - (v * v) * (3.0 - 2.0 * v)
        if mm == 0:
            w[u < 0] = 1.0
        if mm == ta.size - 1:
            w[u > 0] = 1.0
        num[k] += w * xd[a + u]
        den[k] += w
    y = (num / np.maximum(den, 1.0)).astype(np.float32)
    return types.SimpleNamespace(y=y, ta=ta, ts=ts, map=mp, ratio=tr.ratio, applied=tr.applied, src_f0=tr.src_f0, g=none.g, tok=tr.tok, m=tr.m)


@functools.lru_cache(maxsize=None)
def edited_ref(sr, hop, p, s, kind, smooth):
    r, T = signal_contour(sr, hop)
    x = signal(sr)
    return token_ref(x, sr, p, s, hop, T, r.voiced, token_ends(sr, x.size), HZ if kind == 1 else RATIOS, kind, smooth)


def judge(sr, hop, p, s, kind, smooth):
    """The edited signal's contour (yin_ref again) against the targets, on the frames voiced in both contours -> (worst relative error of an
    edited token's mean f0 against its target, median relative frame error against g_f, share of the input's voiced frames voiced in both)."""
    r, _ = signal_contour(sr, hop)
    vin = r.voiced != 0
    o = edited_ref(sr, hop, p, s, kind, smooth)
    ro = yin_ref(o.y.astype(np.float64), sr, hop)
    both = vin & (ro.voiced != 0)
    err = np.abs(ro.f0[both] - o.g[both]) / o.g[both]
    worst = 0.0
    for t, v in enumerate(HZ if kind == 1 else RATIOS):
        if v == 0.0:
            continue
        sel = both & (o.tok == t)
        assert sel.sum() >= 3, (t, int(sel.sum()))
        want = v if kind == 1 else o.applied[t] * (p * (o.m + s * (o.src_f0[t] - o.m)))
        got = float(ro.f0[sel].mean())
        print(f"[token pitch] {sr} Hz kind {kind} smooth {smooth} p = {p} s = {s}: token {t} measured {o.src_f0[t]:.2f} Hz, applied {o.applied[t]:.4f}, "
              f"target {want:.2f} Hz, mean of the output {got:.2f} Hz ({100 * abs(got - want) / want:.2f} %) over {int(sel.sum())} frames")
        worst = max(worst, abs(got - want) / want)
    med, share = float(np.median(err)), both.sum() / vin.sum()
    print(f"[token pitch] {sr} Hz kind {kind} smooth {smooth} p = {p} s = {s}: token mean within {100 * worst:.2f} %, median frame error "
          f"{100 * med:.3f} %, voiced in both {100 * share:.1f} %")
    return worst, med, share


# ---- CPU: ABI and host-side refusals ----------------------------------------------------------------------------------------------------------------

def test_new_symbols_are_exported_and_declared():
    header = open(os.path.join(ROOT, "include", "sbv2_hip.h")).read()
    core = open(os.path.join(ROOT, "include", "sbv2_core.hpp")).read()
    l = _lib.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.SYMBOLS and getattr(l, name) is not None, name
    assert "} sbv2_token_pitch;" in header and "sbv2_pipeline_fetch_request_token_pitch(" in core and "struct TokenPitch" in core
    assert C.sizeof(_lib.Sbv2TokenPitch) == 48
    assert C.sizeof(_lib.Sbv2Voice) == 48 and C.sizeof(_lib.Sbv2Pitch) == 72 and C.sizeof(_lib.Sbv2Marks) == 88   # the existing structs are as they were
    assert _lib.SYMBOLS["sbv2_pipeline_fetch_request_token_pitch"][1][6] == C.POINTER(_lib.Sbv2TokenPitch)
    # the older entry points keep their signatures
    assert len(_lib.SYMBOLS["sbv2_pipeline_fetch_request_dynamics"][1]) == 13 and len(_lib.SYMBOLS["sbv2_debug_voice_shift"][1]) == 15


def _c_tp(values, kind=1, smooth=2, reserved=0, n=None, null_value=False):
    v = np.ascontiguousarray(np.asarray(values, np.float64))
    applied, src = np.full(max(v.size, 1), 77.0), np.full(max(v.size, 1), 77.0)
    c = _lib.Sbv2TokenPitch(None if null_value else v.ctypes.data_as(f64p), v.size if n is None else n, kind, smooth, applied.ctypes.data_as(f64p),
                            src.ctypes.data_as(f64p), reserved)
    return c, (v, applied, src)


BAD_TABLES = [(dict(kind=2), "kind"), (dict(kind=-1), "kind"), (dict(smooth=-1), "smooth"), (dict(smooth=21), "smooth"), (dict(reserved=1), "reserved"),
              (dict(null_value=True), "value must not be NULL"), (dict(n=-1), "n_tokens"),
              (dict(values=[0, -180.0, 0]), "value of token 1"), (dict(values=[0, 0, float("nan")]), "value of token 2"),
              (dict(values=[float("inf"), 0, 0]), "value of token 0"), (dict(values=[0, 34.9, 0]), "value of token 1"),
              (dict(values=[0, 1200.1, 0]), "value of token 1"), (dict(values=[0, 0.49, 0], kind=0), "value of token 1"),
              (dict(values=[0, 2.01, 0], kind=0), "value of token 1"), (dict(values=[180.0, 0, 0], kind=0), "value of token 0")]


def test_token_pitch_refusals_that_need_no_run():
    """The checks of sbv2_token_pitch come before anything touches a handle or a device: a null handle reaches them (and is refused itself when
    they pass), and the hook refuses before its first device call; nothing is written."""
    l = _lib.lib()
    f = model.PcmFormat()
    rows, place = np.array([0], np.int32), np.array([0], np.int64)
    req = _lib.Sbv2FetchRequest(rows.ctypes.data_as(i32p), 1, place.ctypes.data_as(i64p), 10, C.pointer(f.c), None, None, 0)
    x, lens = np.zeros(500, np.float32), np.array([500], np.int64)
    counts, ends = np.array([3], np.int64), np.array([100, 300, 500], np.int64)
    voice = _lib.Sbv2Voice(1.0, 1.0, 0.0, 0.0, 0.0, 0, 0)
    fetch = lambda tp, v=None: l.sbv2_pipeline_fetch_request_token_pitch(None, 1, C.byref(req), v, None, None, tp, dst.ctypes.data, dst.nbytes,
                                                                         C.byref(got), None, None, None, None)
    hook = lambda tp, cnt=counts: l.sbv2_debug_voice_tokens(0, x.ctypes.data_as(_lib.f32p), lens.ctypes.data_as(i64p), 1, 44100, C.byref(voice), None,
                                                            None, cnt.ctypes.data_as(i64p), ends.ctypes.data_as(i64p), tp, None, None, None, None, None, None,
                                                            y.ctypes.data_as(_lib.f32p), None)
    for kw, word in BAD_TABLES:
        kw = dict(kw)
        c, keep = _c_tp(kw.pop("values", [0, 180.0, 0]), **kw)
        dst, got, y = np.full(16, 77, np.uint8), C.c_int64(-5), np.full(500, 77, np.float32)
        assert fetch(C.byref(c)) != 0
        assert word in l.sbv2_last_error().decode(), (kw, l.sbv2_last_error())
        assert (dst == 77).all() and got.value == -5 and (keep[1] == 77).all() and (keep[2] == 77).all()
        if "n" in kw:
            continue                                                            # (the hook counts the tokens itself: see below)
        assert hook(C.byref(c)) != 0
        assert word in l.sbv2_last_error().decode(), (kw, l.sbv2_last_error())
        assert (y == 77).all() and (keep[1] == 77).all() and (keep[2] == 77).all()
    # a table that passes: the null handle is what is refused, with or without a voice, edited or all zeros or NULL
    dst, got, y = np.full(16, 77, np.uint8), C.c_int64(-5), np.full(500, 77, np.float32)
    for tp in (_c_tp([0, 180.0, 0]), _c_tp([0, 0, 0]), _c_tp([1.3, 0, 0.5], kind=0, smooth=0), _c_tp([35.0, 1200.0, 0], smooth=20), None):
        for v in (None, C.byref(voice)):
            assert fetch(C.byref(tp[0]) if tp else None, v) != 0
            assert b"bad arguments" in l.sbv2_last_error(), l.sbv2_last_error()
    assert (dst == 77).all() and got.value == -5
    # the range of kind 1 follows the voice's: [f0_min / 2, 2 f0_max]
    narrow = _lib.Sbv2Voice(1.0, 1.0, 100.0, 400.0, 0.0, 0, 0)
    c, keep = _c_tp([0, 45.0, 0])
    assert fetch(C.byref(c), C.byref(narrow)) != 0 and "value of token 1" in l.sbv2_last_error().decode()
    c, keep = _c_tp([0, 50.0, 800.0])
    assert fetch(C.byref(c), C.byref(narrow)) != 0 and b"bad arguments" in l.sbv2_last_error()
    # everything the dynamics call refuses is refused here too
    bad_voice = _lib.Sbv2Voice(2.5, 1.0, 0.0, 0.0, 0.0, 0, 0)
    c, keep = _c_tp([0, 180.0, 0])
    assert fetch(C.byref(c), C.byref(bad_voice)) != 0 and "pitch_scale" in l.sbv2_last_error().decode()
    # the hook: a count that differs from the rows' names both numbers; ends that descend; a missing table
    c, keep = _c_tp([0, 180.0])
    assert hook(C.byref(c)) != 0
    assert re.search(r"n_tokens is 2 .* 3 tokens", l.sbv2_last_error().decode()), l.sbv2_last_error()
    ends[:] = [100, 50, 500]
    c, keep = _c_tp([0, 180.0, 0])
    assert hook(C.byref(c)) != 0 and b"ascend" in l.sbv2_last_error()
    assert hook(None) != 0 and b"bad arguments" in l.sbv2_last_error()
    assert (y == 77).all()


def test_options_are_checked_at_construction():
    SO = orchestrator.SynthesizeOptions
    o = SO()
    assert o.token_pitch is None and o.token_pitch_kind == "hz" and o.token_pitch_smooth == 2 and not orchestrator.edits_tokens(o)
    o = SO(token_pitch=[0, 180, 0.0, 35, 1200], token_pitch_smooth=0)
    assert o.token_pitch == [0.0, 180.0, 0.0, 35.0, 1200.0] and orchestrator.edits_tokens(o)
    assert not orchestrator.edits_tokens(SO(token_pitch=[0, 0, 0])) and not orchestrator.edits_tokens(SO(token_pitch=[]))
    SO(token_pitch=np.array([0.5, 2.0, 0.0]), token_pitch_kind="ratio", token_pitch_smooth=20)
    SO(token_pitch=[0, 180.0], pitch_track=True)                               # the shifter's contour is there to track
    for kw in (dict(token_pitch=[0, -1.0]), dict(token_pitch=[float("nan")]), dict(token_pitch=[float("inf")]), dict(token_pitch=[34.0]),
               dict(token_pitch=[1201.0]), dict(token_pitch=[180.0], token_pitch_kind="ratio"), dict(token_pitch=[0.4], token_pitch_kind="ratio"),
               dict(token_pitch=["180"]), dict(token_pitch=[True]), dict(token_pitch=[None]), dict(token_pitch="180"), dict(token_pitch=180.0),
               dict(token_pitch_kind="cents"), dict(token_pitch_kind=1), dict(token_pitch_smooth=-1), dict(token_pitch_smooth=21),
               dict(token_pitch_smooth=2.0), dict(token_pitch_smooth=True)):
        with pytest.raises(orchestrator.TokenPitchError):
            SO(**kw)
    assert issubclass(orchestrator.TokenPitchError, model.Sbv2Error)
    with pytest.raises(model.Sbv2Error, match="pitch_track"):
        SO(token_pitch=[0, 0], pitch_track=True)                               # all zeros: nothing shifts, nothing to track
    with pytest.raises(model.Sbv2Error, match="kind"):
        model.TokenPitch([0, 180.0], kind="cents")


# ---- CPU: the routes against fakes --------------------------------------------------------------------------------------------------------------------

N_TOKENS = sum(len(s["phones"]) for s in REQUEST if s)                          # 5 + 3


class TokenPipe(FakePipe):
    """FakePipe whose fetch_request knows token_pitch: the samples of a request are multiplied by the mean of its non-zero values (so the bytes
    tell which table a request was fetched with), applied = the values with 1 for 0, src_f0 = 100 + the token's number."""

    def fetch_request(self, b, rows, fmt, place, joined_len, gain=None, flac=False, marks=False, env_hop=0, levels=True, pitch=None, voice=None,
                      track=None, token_pitch=None):
        self.calls.append(dict(rows=list(rows), marks=marks, voice=None if voice is None else (voice.pitch_scale, voice.intonation_scale),
                               track=track is not None,
                               token_pitch=None if token_pitch is None else (list(token_pitch.values), token_pitch.kind, token_pitch.smooth)))
        res = self._fetch(b, rows, fmt, place, joined_len, marks, voice)
        if token_pitch is None:
            return res
        v = token_pitch.values
        assert v.size == sum(int(b.t_lens[r]) for r in rows)
        token_pitch.applied, token_pitch.src_f0 = np.where(v == 0, 1.0, v), 100.0 + np.arange(v.size)
        token_pitch.src_f0[0] = 0.0
        return (res[0] * np.float32(v[v != 0].mean()),) + tuple(res[1:]) + (token_pitch,)


def test_routes_carry_or_refuse_the_table():
    SO = orchestrator.SynthesizeOptions
    pipe = TokenPipe()
    table = [0.0, 1.5, 0.0, 0.0, 0.0, 0.0, 0.5, 0.0]
    assert len(table) == N_TOKENS
    plain = orchestrator.easy_synthesize(pipe, REQUEST, STYLES, noise_seed=1)
    assert pipe.calls[-1] == dict(plain=True)                                  # the defaults: the plain fetch there always was
    assert orchestrator.easy_synthesize(pipe, REQUEST, STYLES, noise_seed=1, options=SO(token_pitch=[0.0] * N_TOKENS)) == plain
    assert pipe.calls[-1] == dict(plain=True)                                  # all zeros too
    o = lambda **kw: SO(token_pitch=table, token_pitch_kind="ratio", token_pitch_smooth=3, **kw)
    wav = orchestrator.easy_synthesize(pipe, REQUEST, STYLES, noise_seed=1, options=o())
    assert pipe.calls[-1] == dict(rows=[0, 1], marks=False, voice=None, track=False, token_pitch=(table, "ratio", 3))   # ONE fetch, with the table
    assert len(wav) == len(plain) and (_payload(wav) == np.float32(1.0) * _payload(plain)).all()
    wav2, mk = orchestrator.easy_synthesize_marks(pipe, REQUEST, STYLES, noise_seed=1, options=o(pitch_scale=2.0, pitch_track=True))
    assert pipe.calls[-1] == dict(rows=[0, 1], marks=True, voice=(2.0, 1.0), track=True, token_pitch=(table, "ratio", 3))
    assert (_payload(wav2) == np.float32(2.0) * _payload(plain)).all()
    assert mk["pitch_edit"] == {"kind": "ratio", "smooth": 3, "applied": [1.0, 1.5, 1.0, 1.0, 1.0, 1.0, 0.5, 1.0],
                                "src_f0_hz": [None] + [100.0 + t for t in range(1, N_TOKENS)]}
    _, mk0 = orchestrator.easy_synthesize_marks(pipe, REQUEST, STYLES, noise_seed=1)
    assert "pitch_edit" not in mk0 and {k: v for k, v in mk.items() if k != "pitch_edit"} == mk0       # the spans do not move
    # a list of another length: refused with the expected count before any run, edited or not
    runs = pipe.runs
    for bad in (table[:-1], table + [0.0], [0.0] * 3):
        for call in (orchestrator.easy_synthesize, orchestrator.easy_synthesize_marks):
            with pytest.raises(orchestrator.TokenPitchError, match=f"expected {N_TOKENS}"):
                call(pipe, REQUEST, STYLES, noise_seed=1, options=SO(token_pitch=bad, token_pitch_kind="ratio"))
    assert pipe.runs == runs
    # streams refuse, before any GPU work, naming the whole-signal routes
    for kw in (dict(), dict(split=True), dict(levels=True)):
        for opt in (o(), SO(token_pitch=[0.0] * N_TOKENS)):
            with pytest.raises(orchestrator.TokenPitchError, match="/synthesize_marks"):
                orchestrator.easy_synthesize_stream(None, None, REQUEST[:1], STYLES, options=opt, **kw)
    # the batcher: per request, with marks too
    other = [0.0, 0.0, 0.0, 2.0, 0.0, 0.0, 0.0, 0.0]
    rb = batcher.RequestBatcher(pipe, start=False, clock=lambda: 0.0, max_wait_ms=1000.0)
    f0 = rb.submit(REQUEST, STYLES, options=o(), noise_seed=1)
    f1 = rb.submit(REQUEST, STYLES, options=SO(token_pitch=other, token_pitch_kind="ratio"), noise_seed=1, marks=True)
    f2 = rb.submit(REQUEST, STYLES, noise_seed=1)
    f3 = rb.submit(REQUEST, STYLES, options=SO(token_pitch=other[:-1], token_pitch_kind="ratio"), noise_seed=1)
    n = len(pipe.calls)
    rb.start()
    rb.close()
    assert f0.result(0) == wav and f2.result(0) == plain
    assert (_payload(f1.result(0)[0]) == np.float32(2.0) * _payload(plain)).all() and f1.result(0)[1]["pitch_edit"]["applied"][3] == 2.0
    with pytest.raises(orchestrator.TokenPitchError, match=f"expected {N_TOKENS}"):
        f3.result(0)
    tables = [c.get("token_pitch") for c in pipe.calls[n:] if "rows" in c]
    assert tables == [(table, "ratio", 3), (other, "ratio", 2)], pipe.calls[n:]


def test_rest_models_accept_the_table_and_the_stream_routes_refuse_it():
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient
    from sbv2_api_amd import rest
    wav = orchestrator.array_to_wav(np.zeros((1, 1, 10), np.float32))
    marks = {"sample_rate": 44100, "tokens": [], "words": []}
    seen = lambda o: (o.token_pitch, o.token_pitch_kind, o.token_pitch_smooth)

    class H:
        calls = []

        def _count(self, options):
            if options.token_pitch is not None and len(options.token_pitch) != 3:
                raise orchestrator.TokenPitchError("token_pitch holds 2 values but the text has 3 tokens: expected 3")

        def easy_synthesize(self, ident, text, style_id, speaker_id, options):
            self._count(options)
            self.calls.append(("plain",) + seen(options))
            return wav

        def easy_synthesize_batched(self, ident, text, style_id, speaker_id, options, batching=None, marks=False):
            from concurrent.futures import Future
            self.calls.append(("batched",) + seen(options))
            f = Future()
            try:
                self._count(options)
                f.set_result((wav, {}) if marks else wav)
            except Exception as e:
                f.set_exception(e)
            return f

        def easy_synthesize_marks(self, ident, text, style_id, speaker_id, options):
            self._count(options)
            self.calls.append(("marks",) + seen(options))
            return wav, marks

        def easy_synthesize_stream(self, ident, text, style_id, speaker_id, options, **kw):
            raise AssertionError("a stream with a token table must be refused before the holder is asked")

    h = H()
    c = TestClient(rest.make_app(h), raise_server_exceptions=False)
    body = {"text": "x", "ident": "m", "token_pitch": [0, 180, 0], "token_pitch_smooth": 0}
    assert c.post("/synthesize", json=body).content == wav and h.calls[-1] == ("plain", [0.0, 180.0, 0.0], "hz", 0)
    assert c.post("/synthesize", json={"text": "x", "ident": "m"}).content == wav and h.calls[-1] == ("plain", None, "hz", 2)
    ratio = dict(body, token_pitch=[0, 1.3, 0.5], token_pitch_kind="ratio", token_pitch_smooth=5)
    assert c.post("/synthesize_marks", json=ratio).status_code == 200 and h.calls[-1] == ("marks", [0.0, 1.3, 0.5], "ratio", 5)
    cb = TestClient(rest.make_app(h, batching={}), raise_server_exceptions=False)
    assert cb.post("/synthesize", json=body).content == wav and h.calls[-1] == ("batched", [0.0, 180.0, 0.0], "hz", 0)
    n = len(h.calls)
    for route in ("/synthesize", "/synthesize_marks"):
        for extra in ({"token_pitch": [0, 5000.0, 0]}, {"token_pitch": [0, -1, 0]}, {"token_pitch_kind": "cents"}, {"token_pitch_smooth": 21},
                      {"token_pitch": [0, 1.3, 0], "token_pitch_kind": "hz"}):
            r = c.post(route, json=dict(body, **extra))
            assert r.status_code == 400 and "token_pitch" in r.text, (route, extra, r.status_code, r.text)
    assert len(h.calls) == n                                                    # a bad value never reaches the holder
    for client in (c, cb):
        for route in ("/synthesize", "/synthesize_marks"):
            r = client.post(route, json=dict(body, token_pitch=[0, 180]))       # a count that does not match the text
            assert r.status_code == 400 and "expected 3" in r.text, (route, r.status_code, r.text)
    for route in ("/synthesize_stream", "/synthesize_stream_marks"):
        for extra in ({"token_pitch": [0, 180, 0]}, {"token_pitch": [0, 0, 0]}, {"token_pitch": [9000.0]}):
            r = c.post(route, json={"text": "x", "ident": "m", **extra})
            assert r.status_code == 400 and "/synthesize_marks" in r.text, (route, r.status_code, r.text)


# ---- CPU: the restatement keeps its promises ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sr,hop", SIGNALS)
def test_the_reference_keeps_its_promises(sr, hop):
    x = signal(sr)
    r, T = signal_contour(sr, hop)
    ends = token_ends(sr, x.size)
    for p, s in ((1.0, 1.0), (1.2, 0.5)):
        plain = voice_ref(x, sr, p, s, hop, T, r.voiced)
        for kind in (0, 1):
            for smooth in (0, 2, 20):                                            # all zeros: the call without, whatever the kind and K
                o = token_ref(x, sr, p, s, hop, T, r.voiced, ends, np.zeros(8), kind, smooth)
                assert o.y.tobytes() == plain.y.tobytes() and np.array_equal(o.ts, plain.ts) and (o.ratio == 1.0).all() and (o.applied == 1.0).all()
        assert token_ref(x, sr, p, s, hop, T, r.voiced, [], [], 1, 2).y.tobytes() == plain.y.tobytes()   # ... and no token at all
    assert token_ref(x, sr, 1.0, 1.0, hop, T, r.voiced, ends, np.zeros(8), 1, 2).y.tobytes() == x.tobytes()    # the bytes of the input
    for kind, smooth, p, s in ((1, 2, 1.0, 1.0), (1, 0, 1.2, 0.5), (0, 2, 1.0, 1.0), (0, 0, 1.2, 0.5)):
        o = edited_ref(sr, hop, p, s, kind, smooth)
        assert o.y.size == x.size and o.y.dtype == np.float32 and o.y.tobytes() != x.tobytes()
        assert np.abs(o.y).max() <= np.abs(x).max(), (kind, smooth)
        assert o.src_f0[0] == 0.0 and o.src_f0[4] == 0.0 and o.src_f0[7] == 0.0 and abs(o.src_f0[1] - 150.0) < 0.5      # the noise, the tone
        assert (o.applied[[0, 2, 4, 7]] == 1.0).all()
    # applied shows the clamp: 500 Hz and 60 Hz on the 150 Hz tone
    o = token_ref(x, sr, 1.0, 1.0, hop, T, r.voiced, ends, [0, 500.0, 0, 60.0, 0, 0, 0, 0], 1, 2)
    assert o.applied[1] == 2.0 and o.applied[3] == 0.5 and np.abs(o.y).max() <= np.abs(x).max()
    # a token without a voiced frame (the noise, the zeros) and a zero-duration token are left alone and change nothing
    ends9 = np.concatenate([ends[:2], ends[1:]])                                 # token 2 is empty
    none = token_ref(x, sr, 1.0, 1.0, hop, T, r.voiced, ends9, [200.0, 0, 200.0, 0, 0, 200.0, 0, 0, 200.0], 1, 2)
    assert (none.applied == 1.0).all() and none.y.tobytes() == x.tobytes() and not (none.tok == 2).any()
    assert none.src_f0[2] == 0.0 and none.src_f0[1] > 0
    step = token_ref(x, sr, 1.0, 1.0, hop, T, r.voiced, ends9, [0, 0, 1.5, 0, 0, 0, 0, 0, 0], 0, 0)   # kind 0 on the empty token: applied, but no frame has it
    assert step.applied[2] == 1.5 and (step.ratio == 1.0).all() and step.y.tobytes() == x.tobytes()


EDITS = [(1, 2, 1.0, 1.0, 0.0462, 0.00516, 0.754), (1, 0, 1.2, 0.5, 0.0189, 0.00447, 0.754), (0, 2, 1.0, 1.0, 0.0413, 0.00498, 0.790),
         (0, 0, 1.2, 0.5, 0.0275, 0.00357, 0.742)]


@pytest.mark.parametrize("kind,smooth,p,s,tok_max,med_max,share_min", EDITS)
@pytest.mark.parametrize("sr,hop", SIGNALS)
def test_the_reference_edits_the_tokens(sr, hop, kind, smooth, p, s, tok_max, med_max, share_min):
    """The edited tokens' mean f0 of the output (yin_ref again, frames voiced in both contours) against their targets (kind 1: the value; kind 0:
    applied_t p (m + s (M_t - m))), and every such frame against g_f.  Measured when written, (44.1 kHz, 16 kHz):
      Hz [0, 180, 0, 120, 0, 200, 150, 0], smooth 2, p = s = 1:       token mean within 2.53 %, 3.08 %; median frame error 0.248 %, 0.344 %; voiced in both 83.8 %, 84.2 %
      the same, smooth 0, p = 1.2, s = 0.5:                           0.98 %, 1.26 %; 0.167 %, 0.298 %; 83.8 %, 85.5 %
      ratios [0, 1.3, 0, 0.8, 0, 1, 1.5, 0], smooth 2, p = s = 1:     2.35 %, 2.75 %; 0.332 %, 0.247 %; 87.8 %, 89.5 %
      the same, smooth 0, p = 1.2, s = 0.5:                           1.60 %, 1.83 %; 0.147 %, 0.238 %; 82.4 %, 86.8 %
    The bounds are 1.5 x the worse of the two rates for the token mean and the median (the figures move by about that much with the token cut
    between the rates) and 0.9 x the smaller share.  No 90th percentile: the frames at a ratio step dominate it."""
    worst, med, share = judge(sr, hop, p, s, kind, smooth)
    assert worst <= tok_max and med <= med_max and share >= share_min, (worst, med, share)


# ---- GPU: the kernels against the reference -------------------------------------------------------------------------------------------------------------

def assert_equal_to_ref(got, x, sr, p, s, hop, ends, values, kind, smooth, what, **kw):
    """One row of debug_voice_tokens against token_ref fed the device's own contour: marks and map equal; y, R_f, applied, src_f0 bit-equal."""
    ref = token_ref(x, sr, p, s, hop, got.period, got.voiced, ends, values, kind, smooth, **kw)
    assert got.y.size == x.size, what
    np.testing.assert_array_equal(got.ta, ref.ta, err_msg=what + ": ta")
    np.testing.assert_array_equal(got.ts, ref.ts, err_msg=what + ": ts")
    np.testing.assert_array_equal(got.map, ref.map, err_msg=what + ": map")
    for name in ("ratio", "applied", "src_f0"):
        a, b = getattr(got, name), getattr(ref, name)
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), (what, name, a, b)
    bad = np.nonzero(got.y.view(np.uint32) != ref.y.view(np.uint32))[0]
    assert bad.size == 0, (what, "y differs at", bad[:8], got.y[bad[:8]], ref.y[bad[:8]])
    return ref


@gpu
@pytest.mark.parametrize("p,s", [(1.0, 1.0), (1.2, 0.5)])
@pytest.mark.parametrize("smooth", [0, 2, 20])
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("sr,hop", SIGNALS)
def test_hook_equals_the_reference(sr, hop, kind, smooth, p, s):
    x = signal(sr)
    ends, values = token_ends(sr, x.size), HZ if kind == 1 else RATIOS
    tp = model.TokenPitch(values, "hz" if kind else "ratio", smooth)
    (got,), tp = model.debug_voice_tokens(x, sr, model.Voice(p, s, hop=hop), ends, tp)
    ref = assert_equal_to_ref(got, x, sr, p, s, hop, ends, values, kind, smooth, f"{sr} Hz kind {kind} smooth {smooth} p = {p} s = {s}")
    assert got.voiced.any() and ref.ts.size > 20 and tp.applied.tobytes() == got.applied.tobytes()
    assert (got.applied[[0, 2, 4, 7]] == 1.0).all() and got.applied[1] != 1.0 and (got.ratio != 1.0).any()
    assert got.y.tobytes() != x.tobytes() and np.abs(got.y).max() <= np.abs(x).max()


@gpu
@pytest.mark.parametrize("sr,hop", SIGNALS)
def test_all_zeros_is_the_call_without_and_a_second_call_gives_equal_bits(sr, hop):
    x = signal(sr)
    ends = token_ends(sr, x.size)
    for kind in ("hz", "ratio"):                                                 # forced through k_voice_marks_tok: the identity
        (got,), tp = model.debug_voice_tokens(x, sr, model.Voice(1.0, 1.0, hop=hop), ends, model.TokenPitch(np.zeros(8), kind, 2))
        assert got.y.tobytes() == x.tobytes() and np.array_equal(got.ta, got.ts) and (got.ratio == 1.0).all() and (tp.applied == 1.0).all()
        assert tp.src_f0[0] == 0.0 and abs(tp.src_f0[1] - 150.0) < 0.5           # ... and the means are measured all the same
    plain, = model.debug_voice_shift(x, sr, model.Voice(1.2, 0.5, hop=hop))
    (got,), _ = model.debug_voice_tokens(x, sr, model.Voice(1.2, 0.5, hop=hop), ends, model.TokenPitch(np.zeros(8), "hz", 20))
    assert got.y.tobytes() == plain.y.tobytes() and np.array_equal(got.ts, plain.ts) and got.period.tobytes() == plain.period.tobytes()
    (a,), ta = model.debug_voice_tokens(x, sr, model.Voice(1.2, 0.5, hop=hop), ends, model.TokenPitch(HZ, "hz", 2))
    (b,), tb = model.debug_voice_tokens(x, sr, model.Voice(1.2, 0.5, hop=hop), ends, model.TokenPitch(HZ, "hz", 2))
    assert a.y.tobytes() == b.y.tobytes() and a.ratio.tobytes() == b.ratio.tobytes() and ta.applied.tobytes() == tb.applied.tobytes()
    assert ta.src_f0.tobytes() == tb.src_f0.tobytes() and a.y.tobytes() != plain.y.tobytes()


def _rows_16k():
    """The packed rows of one call at 16 kHz, hop 80, smooth 20 (2 K + 1 = 41 frames), kind 1: (name, samples, token ends, values)."""
    sr = 16000
    x = signal(sr)
    tile = model.voice_tile()
    rng = np.random.default_rng(2)
    t = np.arange(2000) / sr
    tone = sum(np.sin(2 * np.pi * k * 150.0 * t + k) / k for k in range(1, 5))
    tone = (tone / np.abs(tone).max() * 0.7).astype(np.float32)
    a = 50 * sr // 1000                                                         # the tone of `signal` starts here
    many = np.sort(rng.integers(0, x.size + 1, 299))                            # 300 tokens on 106 frames: most own no frame or one
    many_v = np.where(np.arange(300) % 3 == 0, 0.0, 100.0 + 2.0 * (np.arange(300) % 97))
    rows = [("empty", np.zeros(0, np.float32), [0, 0], [180.0, 0.0]),
            ("shorter than one frame", x[a:a + 20], [5, 20], [180.0, 200.0]),
            ("fewer frames than the window", x[:1234], [300, 900, 1234], [0.0, 180.0, 120.0]),
            ("300 tokens", x, list(many) + [x.size], many_v),
            ("one token", tone, [2000], [180.0]),
            ("first and last token empty", tone, [0, 700, 1400, 2000, 2000], [300.0, 120.0, 0.0, 200.0, 300.0]),
            ("no voiced frame", (rng.standard_normal(2000) * 0.05).astype(np.float32), [500, 2000], [180.0, 120.0]),
            ("tokens end before the row", tone, [400, 1000], [180.0, 120.0]),
            ("tokens end beyond the row", tone, [1000, 5000, 9000], [120.0, 180.0, 240.0]),
            ("no token", tone, [], []),
            ("tile - 1", x[a + 100:a + 100 + 5 * tile - 1], [640, 5 * tile - 1], [120.0, 180.0]),
            ("tile", x[a + 100:a + 100 + 5 * tile], [640, 5 * tile], [120.0, 180.0]),
            ("tile + 1", x[a + 100:a + 100 + 5 * tile + 1], [640, 5 * tile + 1], [120.0, 180.0]),
            ("one tile - 1", tone[:tile - 1], [100, tile - 1], [180.0, 120.0]), ("one tile", tone[:tile], [100, tile], [180.0, 120.0]),
            ("one tile + 1", tone[:tile + 1], [100, tile + 1], [180.0, 120.0])]
    return sr, 80, 20, rows


@gpu
def test_packed_rows_of_every_edge_shape_in_one_call():
    sr, hop, smooth, rows = _rows_16k()
    assert lags_np(sr) == (26, 229)
    values = np.concatenate([np.asarray(v, np.float64) for _, _, _, v in rows])
    tp = model.TokenPitch(values, "hz", smooth)
    got, tp = model.debug_voice_tokens([r for _, r, _, _ in rows], sr, model.Voice(1.2, 0.5, hop=hop), [e for _, _, e, _ in rows], tp)
    assert len(got) == len(rows) and tp.applied.size == values.size
    seen = {}
    for (name, x, ends, v), g in zip(rows, got):
        ref = assert_equal_to_ref(g, x, sr, 1.2, 0.5, hop, ends, v, 1, smooth, name)
        assert g.ratio.size == g.voiced.size == (-(-x.size // hop) if x.size else 0), name
        seen[name] = (g, ref)
    assert seen["empty"][0].y.size == 0 and (seen["empty"][0].applied == 1.0).all()
    assert seen["shorter than one frame"][0].ratio.size == 1 and 0 < seen["fewer frames than the window"][0].ratio.size < 2 * smooth + 1
    g, ref = seen["300 tokens"]
    owned = np.bincount(ref.tok, minlength=301)[:300]
    assert g.applied.size == 300 > 256 and (owned == 0).sum() > 150 and (owned <= 1).sum() > 250 and (g.applied != 1.0).sum() > 20
    assert (g.applied[owned == 0] == 1.0).all() and (g.src_f0[owned == 0] == 0.0).all()
    g, ref = seen["one token"]
    assert g.applied[0] != 1.0 and np.ptp(g.ratio) == 0.0 and g.ratio[0] == g.applied[0]
    g, ref = seen["first and last token empty"]
    assert g.applied[0] == 1.0 and g.applied[4] == 1.0 and g.applied[1] != 1.0 and g.applied[2] == 1.0
    g, ref = seen["no voiced frame"]
    assert not g.voiced.any() and (g.applied == 1.0).all() and (g.src_f0 == 0.0).all() and g.y.tobytes() == rows[6][1].tobytes()
    g, ref = seen["tokens end before the row"]
    assert (ref.tok[-5:] == 2).all() and g.ratio[-1] != g.applied[1]             # the last frames have no token: rho 65536 in their windows
    g, ref = seen["no token"]
    plain, = model.debug_voice_shift(rows[9][1], sr, model.Voice(1.2, 0.5, hop=hop))
    assert (g.ratio == 1.0).all() and g.y.tobytes() == plain.y.tobytes()
    for name in ("tile - 1", "tile", "tile + 1"):                                # (five tiles long: a row of one tile is too short for a voiced frame)
        assert seen[name][0].voiced.any() and (seen[name][0].applied != 1.0).any(), name
    # a row's result does not depend on its neighbours: the same rows in another order
    back, tb = model.debug_voice_tokens([r for _, r, _, _ in rows[::-1]], sr, model.Voice(1.2, 0.5, hop=hop), [e for _, _, e, _ in rows[::-1]],
                                        model.TokenPitch(np.concatenate([np.asarray(v, np.float64) for _, _, _, v in rows[::-1]]), "hz", smooth))
    for (name, _, _, _), g, h in zip(rows, got, back[::-1]):
        assert g.y.tobytes() == h.y.tobytes() and g.ratio.tobytes() == h.ratio.tobytes() and g.applied.tobytes() == h.applied.tobytes(), name


@gpu
def test_a_given_contour_gives_the_reference_bits():
    """period_in: a 200-sample period, then 210, over a pulse train with one unvoiced gap; everything behind the contour is exact arithmetic."""
    sr, hop = 44100, 220
    n = 40 * hop + 57
    x = np.zeros(n, np.float32)
    x[::200] = 0.5
    x += (np.random.default_rng(3).standard_normal(n) * 0.01).astype(np.float32)
    nf = -(-n // hop)
    period, voiced = np.full(nf, 200.0), np.ones(nf, np.int32)
    period[30:] = 210.0
    voiced[15:22] = 0
    period[15:22] = 12345.0                                                     # (an unvoiced frame's period is not looked at)
    ends = [7 * hop, 15 * hop + 3, 22 * hop, 30 * hop, n]
    for kind, values, smooth, p, s in ((0, [1.3, 0, 0, 0.5, 2.0], 2, 1.0, 1.0), (1, [0, 300.0, 150.0, 0, 100.0], 0, 1.3, 0.8),
                                       (1, [1200.0, 0, 35.0, 0, 0], 20, 0.5, 2.0)):
        (got,), tp = model.debug_voice_tokens(x, sr, model.Voice(p, s, hop=hop), ends, model.TokenPitch(values, "hz" if kind else "ratio", smooth),
                                              period=period, voiced=voiced)
        assert got.period[voiced != 0].tobytes() == period[voiced != 0].tobytes() and np.array_equal(got.voiced, voiced)
        ref = token_ref(x, sr, p, s, hop, period, voiced, ends, values, kind, smooth)
        np.testing.assert_array_equal(got.ta, ref.ta)
        np.testing.assert_array_equal(got.ts, ref.ts)
        np.testing.assert_array_equal(got.map, ref.map)
        assert got.y.tobytes() == ref.y.tobytes() and got.ratio.tobytes() == ref.ratio.tobytes(), (kind, smooth)
        assert tp.applied.tobytes() == ref.applied.tobytes() and tp.src_f0.tobytes() == ref.src_f0.tobytes()
        assert abs(tp.src_f0[0] - 220.5) < 1e-3 and tp.src_f0[2] == 0.0 and abs(tp.src_f0[4] - 210.0) < 1e-3
    assert tp.applied[0] == 2.0 and tp.applied[2] == 1.0                        # the clamp of r_t; a token without a voiced frame


# ---- GPU: the pipeline ----------------------------------------------------------------------------------------------------------------------------------

VOICE = (1.3, 0.8)


@pytest.fixture(scope="module")
def edits(five_rows):
    """The token ends of five_rows' two rows (hop c[t + 1], read off the marks of the identity format) and a table of ratios over them."""
    c = five_rows
    _, _, m = c.pipe.fetch_request(c.b, c.rows, model.PcmFormat(), c.place, c.joined, marks=True, levels=False)
    counts = [int(c.b.t_lens[r]) for r in c.rows]
    at = np.concatenate([[0], np.cumsum(counts)])
    ends = [m.end[at[k]:at[k + 1]] - c.place[k] for k in range(len(c.rows))]
    assert all(e[-1] == len(c.native[r]) for e, r in zip(ends, c.rows))
    values = np.where(np.arange(at[-1]) % 3 == 1, 0.0, 0.7 + 0.1 * (np.arange(at[-1]) % 7))
    return types.SimpleNamespace(counts=counts, at=at, ends=ends, values=values, tp=lambda **kw: model.TokenPitch(values, "ratio", **kw))


def _hooked(c, e, rows, ends, values, kind="ratio", smooth=2, voice=None, **kw):
    got, tp = model.debug_voice_tokens([c.native[r] for r in rows], 44100, voice or model.Voice(1.0, 1.0), ends, model.TokenPitch(values, kind, smooth), **kw)
    return {r: g.y for r, g in zip(rows, got)}, tp


@gpu
def test_pipeline_token_pitch_is_the_hook_on_the_native_rows(five_rows, edits):
    c, e = five_rows, edits
    pipe, b, rows, place, joined = c.pipe, c.b, c.rows, c.place, c.joined
    f0 = model.PcmFormat()
    plain = pipe.fetch_request(b, rows, f0, place, joined)[0].copy()
    zeros, _, tz = pipe.fetch_request(b, rows, f0, place, joined, token_pitch=model.TokenPitch(np.zeros(e.at[-1]), "hz"))
    assert zeros.tobytes() == plain.tobytes() and (tz.applied == 1.0).all() and (tz.src_f0 == 0.0).all()       # all zeros: the bytes of the call without
    shifted, th = _hooked(c, e, rows, e.ends, e.values)
    changed = [r for r in rows if shifted[r].tobytes() != c.native[r].tobytes()]
    print(f"[token pitch] rows {rows}: {len(changed)} changed; applied {th.applied}, src_f0 {np.round(th.src_f0, 1)}")
    assert changed, "the synthetic rows hold no voiced frame: the pipeline tests would show nothing"
    got, _, tp = pipe.fetch_request(b, rows, f0, place, joined, token_pitch=e.tp())
    got = got.copy()
    assert got.dtype == np.float32 and got.tobytes() == _join(shifted, rows, place, joined).tobytes()
    assert tp.applied.tobytes() == th.applied.tobytes() and tp.src_f0.tobytes() == th.src_f0.tobytes() and (tp.src_f0 > 0).any()
    again, _, t2 = pipe.fetch_request(b, rows, f0, place, joined, token_pitch=e.tp())                              # twice: identical
    assert again.tobytes() == got.tobytes() and t2.applied.tobytes() == tp.applied.tobytes() and t2.src_f0.tobytes() == tp.src_f0.tobytes()
    # with a voice: the hook with the same voice
    vshift, tv = _hooked(c, e, rows, e.ends, e.values, voice=model.Voice(*VOICE), smooth=0)
    gv, _, tpv = pipe.fetch_request(b, rows, f0, place, joined, voice=model.Voice(*VOICE), token_pitch=e.tp(smooth=0))
    assert gv.tobytes() == _join(vshift, rows, place, joined).tobytes() and tpv.applied.tobytes() == tv.applied.tobytes() and gv.tobytes() != got.tobytes()
    # kind "hz": targets at the measured means of the first fetch times the same ratios give the same ratios, up to Q16
    hz = np.where((e.values != 0) & (tp.src_f0 > 0), np.clip(e.values * tp.src_f0, 35.0, 1200.0), 0.0)
    hshift, thz = _hooked(c, e, rows, e.ends, hz, kind="hz")
    gh, _, tph = pipe.fetch_request(b, rows, f0, place, joined, token_pitch=model.TokenPitch(hz, "hz"))
    assert gh.tobytes() == _join(hshift, rows, place, joined).tobytes() and tph.applied.tobytes() == thz.applied.tobytes()
    on = hz != 0
    assert on.any() and np.abs(tph.applied[on] - np.clip(hz[on] / tp.src_f0[on], 0.5, 2.0)).max() <= 2.0 ** -16
    # 16 kHz s16: the formatter's launches on the edited rows; the FLAC sink decodes to it
    f = model.PcmFormat(16000, "s16")
    s16 = pipe.fetch_request(b, rows, f, place, joined, token_pitch=e.tp())[0].copy()
    x = np.concatenate([shifted[r] for r in rows])
    pieces = [(0, place[0], len(shifted[rows[0]])), (len(shifted[rows[0]]), place[1], len(shifted[rows[1]]))]
    ref = model.debug_pcm_format(x, pieces, [(0, model.pcm_format_length(f, joined), 0, 2)], f)[0]
    assert s16.dtype == np.int16 and s16.tobytes() == ref.tobytes() and s16.tobytes() != pipe.fetch_request(b, rows, f, place, joined)[0].tobytes()
    fl, _, tfl = pipe.fetch_request(b, rows, f, place, joined, flac=True, token_pitch=e.tp())
    d = R.read(fl)
    assert d["rate"] == 16000 and np.asarray(d["samples"], np.int16).tobytes() == s16.tobytes() and tfl.applied.tobytes() == tp.applied.tobytes()
    # a subset of rows in another order takes its values in the order of the request's rows
    sub, splace = [rows[1], rows[0]], [500, 500 + len(c.native[rows[1]]) + 1000]
    sjoined = splace[1] + len(c.native[rows[0]]) + 7
    svalues = np.concatenate([e.values[e.at[1]:e.at[2]], e.values[e.at[0]:e.at[1]]])
    sshift, ts_ = _hooked(c, e, sub, [e.ends[1], e.ends[0]], svalues)
    gs, _, tps = pipe.fetch_request(b, sub, f0, splace, sjoined, token_pitch=model.TokenPitch(svalues, "ratio"))
    assert gs.tobytes() == _join(sshift, sub, splace, sjoined).tobytes() and tps.applied.tobytes() == ts_.applied.tobytes()
    assert all(sshift[r].tobytes() == shifted[r].tobytes() for r in rows)        # a row's edit does not depend on its neighbours
    one, _, tp1 = pipe.fetch_request(b, rows[:1], f0, [0], len(c.native[rows[0]]), token_pitch=model.TokenPitch(e.values[:e.at[1]], "ratio"))
    assert one.tobytes() == shifted[rows[0]].tobytes() and tp1.src_f0.tobytes() == tp.src_f0[:e.at[1]].tobytes()
    # refusals through the handle write nothing and leave the ticket fetchable: the count (both numbers), a value, the voice
    with pytest.raises(model.Sbv2Error, match=rf"n_tokens is {e.at[-1] - 1} .* {e.at[-1]} tokens"):
        pipe.fetch_request(b, rows, f0, place, joined, token_pitch=model.TokenPitch(e.values[:-1], "ratio"))
    with pytest.raises(model.Sbv2Error, match="value of token 0"):
        pipe.fetch_request(b, rows, f0, place, joined, token_pitch=model.TokenPitch(np.full(e.at[-1], 3.0), "ratio"))
    with pytest.raises(model.Sbv2Error, match="pitch_scale"):
        pipe.fetch_request(b, rows, f0, place, joined, voice=model.Voice(2.5, 1.0), token_pitch=e.tp())
    # the ticket is fetched again without edits afterwards and is unchanged: the run's PCM was only read
    assert pipe.fetch_request(b, rows, f0, place, joined)[0].tobytes() == plain.tobytes()
    assert pipe.fetch_request(b, rows, f0, place, joined, token_pitch=None)[0].tobytes() == plain.tobytes()
    assert [x.tobytes() for x in pipe.fetch(b)] == [x.tobytes() for x in c.native]


def _tracked_contour(x, sr, hop, track):
    """T_f and voiced of the tracked contour of one row, as the shifter forms them (the recipe of tests/test_pitch_track.py)."""
    _, tau_max = lags_np(sr)
    t = model.debug_pitch_track(x, sr, model.Pitch(hop), track)
    _, c3, _ = model.debug_pitch(x, sr, model.Pitch(hop))
    c3 = c3.copy()
    on = t.state < model.TRACK_CAND
    c3[on] = t.c3[np.nonzero(on)[0], t.state[on]]
    lag = t.pitch.lag.astype(np.float64)
    den = c3[:, 0] - 2.0 * c3[:, 1] + c3[:, 2]
    both = (t.pitch.lag - 1 >= 1) & (t.pitch.lag + 1 <= tau_max)
    with np.errstate(invalid="ignore", divide="ignore"):
        delta = np.where((den > 0) & both, 0.5 * (c3[:, 0] - c3[:, 2]) / den, 0.0)
    return lag + np.clip(delta, -1.0, 1.0), on.astype(np.int32)


@gpu
def test_pipeline_token_pitch_with_marks_pitch_tracking_loudness_and_compressor(five_rows, edits):
    from test_dynamics import USUAL, check_format, close_stats, compress, meter
    c, e = five_rows, edits
    pipe, b, rows, place, joined = c.pipe, c.b, c.rows, c.place, c.joined
    f0 = model.PcmFormat()
    sr, hop = 44100, 44100 // 200
    track = model.PitchTrack(cand_max=1.0, unvoiced_cost=0.9, switch_cost=0.2, jump_cost=0.25)
    contour = [_tracked_contour(c.native[r], sr, hop, track) for r in rows]
    want, th = _hooked(c, e, rows, e.ends, e.values, voice=model.Voice(*VOICE), period=[p for p, _ in contour], voiced=[v for _, v in contour])
    # voice, tracking and the table: the hook fed the tracked contour, bit for bit
    got, _, tp = pipe.fetch_request(b, rows, f0, place, joined, voice=model.Voice(*VOICE), track=track, token_pitch=e.tp())
    y = _join(want, rows, place, joined)
    assert got.tobytes() == y.tobytes() and tp.applied.tobytes() == th.applied.tobytes() and tp.src_f0.tobytes() == th.src_f0.tobytes()
    # tracking the shifter's contour needs no voice when tokens are edited
    alone, _, _ = pipe.fetch_request(b, rows, f0, place, joined, track=track, token_pitch=e.tp())
    w1, _ = _hooked(c, e, rows, e.ends, e.values, period=[p for p, _ in contour], voiced=[v for _, v in contour])
    assert alone.tobytes() == _join(w1, rows, place, joined).tobytes()
    # everything together: the chain (compressor, loudness gain) on the hook's output; marks and pitch of the delivered samples
    dyn, ln = model.Dynamics(), model.Loudness(-23.0)
    yc, dref, det = compress(y.astype(np.float64), sr, *USUAL)
    ref = meter(yc, sr, ln.target_lufs, ln.true_peak_max)
    ph = 441
    out, st, m, pc, ds, tpa = pipe.fetch_request(b, rows, f0, place, joined, gain=ln, marks=True, env_hop=ph, pitch=model.Pitch(ph), voice=model.Voice(*VOICE),
                                                 track=track, dynamics=dyn, token_pitch=e.tp())
    out = out.copy()
    print(f"[token pitch] all together: compressor {ds} (restated {dref}); loudness {st} (restated {ref})")
    close_stats(ds, dref, what="token pitch + compressor")
    close_stats(st, ref, what="token pitch + compressor, loudness")
    check_format(out, yc * 10 ** (ref[2] / 20), "f32", "token pitch + voice + tracking + compressor + loudness")
    assert tpa.applied.tobytes() == tp.applied.tobytes() and tpa.src_f0.tobytes() == tp.src_f0.tobytes()
    _, _, pm = pipe.fetch_request(b, rows, f0, place, joined, marks=True, env_hop=ph)
    assert m.start.tobytes() == pm.start.tobytes() and m.end.tobytes() == pm.end.tobytes()       # the spans are those without any of it
    ss, pk = model.debug_segment_levels(out, m.start, m.end)
    assert ss.tobytes() == m.sumsq.tobytes() and pk.tobytes() == m.peak.tobytes()
    h = model.debug_pitch_track(out, sr, model.Pitch(ph), track).pitch
    assert h.f0.tobytes() == pc.f0.tobytes() and (h.lag == pc.lag).all()
    # the same call with all zeros is the parent call's bytes; afterwards the ticket is what it was
    base = pipe.fetch_request(b, rows, f0, place, joined, gain=ln, marks=True, env_hop=ph, pitch=model.Pitch(ph), voice=model.Voice(*VOICE), track=track,
                              dynamics=dyn)
    zero = pipe.fetch_request(b, rows, f0, place, joined, gain=ln, marks=True, env_hop=ph, pitch=model.Pitch(ph), voice=model.Voice(*VOICE), track=track,
                              dynamics=dyn, token_pitch=model.TokenPitch(np.zeros(e.at[-1]), "ratio", 0))
    assert zero[0].tobytes() == base[0].tobytes() and zero[1].tobytes() == base[1].tobytes() and zero[4].tobytes() == base[4].tobytes()
    assert zero[3].f0.tobytes() == base[3].f0.tobytes() and zero[2].sumsq.tobytes() == base[2].sumsq.tobytes() and zero[0].tobytes() != out.tobytes()
    assert [x.tobytes() for x in pipe.fetch(b)] == [x.tobytes() for x in c.native]


@gpu
def test_batcher_and_rest_carry_the_table(monkeypatch):
    """Without the decoder's noise the synthetic rows are periodic (see tests/test_voice.py): two concurrent requests with different tables each
    get the answer of the request run alone, through the batcher and through REST."""
    monkeypatch.setattr(orchestrator, "NOISE_SCALE", 0.0)
    monkeypatch.setattr(orchestrator, "NOISE_SCALE_W", 0.0)
    quiet = dict(noise_scale=0.0, noise_scale_w=0.0)
    bs, vs = model.load_model(blob("bert", "tiny", 3), True), model.load_model(blob("vits", "tiny", 5), False)
    bc, _ = weights("bert", "tiny", 3)
    vc, _ = weights("vits", "tiny", 5)
    keys = ("input_ids", "word2ph", "phones", "tones", "langs")
    sv = synth.hash_normal(77, 3 * vc["style_dim"]).reshape(3, -1).astype(np.float32) * 0.1
    SO = orchestrator.SynthesizeOptions
    pipe = model.Pipeline(bs, vs)
    try:
        for seed0 in range(151, 175):   # the first request in which both tables find voiced frames to move (or the test shows nothing)
            sents = [{k: u[k] for k in keys} for u in make_utts([14, 40], bc, vc, seed0=seed0, with_bert=False)]
            n = sum(len(s["phones"]) for s in sents)
            t1 = [0.0 if t % 4 == 0 else 0.7 + 0.1 * (t % 6) for t in range(n)]
            t2 = [0.0 if t % 2 else 1.6 for t in range(n)]
            o1 = lambda: SO(token_pitch=t1, token_pitch_kind="ratio")
            o2 = lambda: SO(sample_rate=16000, encoding="s16", token_pitch=t2, token_pitch_kind="ratio", token_pitch_smooth=0, pitch_scale=0.9)
            plain = orchestrator.easy_synthesize(pipe, sents, sv, 1, 0, SO(), noise_seed=4242, **quiet)
            alone1 = orchestrator.easy_synthesize(pipe, sents, sv, 1, 0, o1(), noise_seed=4242, **quiet)
            alone2, marks2 = orchestrator.easy_synthesize_marks(pipe, sents, sv, 1, 0, o2(), noise_seed=99, **quiet)
            scaled2 = orchestrator.easy_synthesize(pipe, sents, sv, 1, 0, SO(sample_rate=16000, encoding="s16", pitch_scale=0.9), noise_seed=99, **quiet)
            if alone1 != plain and alone2 != scaled2:
                break
        print(f"[token pitch] the request of seed {seed0}: {n} tokens")
        assert len(alone1) == len(plain) and alone1 != plain and len(alone2) == len(scaled2) and alone2 != scaled2
        edit = marks2["pitch_edit"]
        assert edit["kind"] == "ratio" and edit["smooth"] == 0 and edit["applied"] == [1.0 if v == 0 else round(v * 65536) / 65536.0 for v in t2] and len(edit["src_f0_hz"]) == n
        assert any(v is not None for v in edit["src_f0_hz"])
        rb = batcher.RequestBatcher(pipe, start=False, max_wait_ms=1000.0)
        f1 = rb.submit(sents, sv, 1, 0, o1(), noise_seed=4242)
        f2 = rb.submit(sents, sv, 1, 0, o2(), noise_seed=99, marks=True)
        f3 = rb.submit(sents, sv, 1, 0, SO(), noise_seed=4242)
        rb.start()
        rb.close()
        assert f1.result(0) == alone1 and f2.result(0)[0] == alone2 and f2.result(0)[1] == marks2 and f3.result(0) == plain
        pytest.importorskip("fastapi")
        from fastapi.testclient import TestClient
        from sbv2_api_amd import rest

        class H:
            def easy_synthesize(self, ident, text, style_id, speaker_id, options):
                return orchestrator.easy_synthesize(pipe, sents, sv, style_id, speaker_id, options, noise_seed=4242, **quiet)

            def easy_synthesize_stream(self, ident, text, style_id, speaker_id, options, **kw):
                return orchestrator.easy_synthesize_stream(bs, vs, sents[:1], sv, style_id, speaker_id, options, noise_seed=4242, **kw)

        cl = TestClient(rest.make_app(H()), raise_server_exceptions=False)
        body = {"text": "x", "ident": "m", "style_id": 1, "token_pitch": t1, "token_pitch_kind": "ratio"}
        r = cl.post("/synthesize", json=body)
        assert r.status_code == 200 and r.content == alone1
        assert cl.post("/synthesize", json={"text": "x", "ident": "m", "style_id": 1}).content == plain
        r = cl.post("/synthesize", json=dict(body, token_pitch=t1[:-1]))
        assert r.status_code == 400 and f"expected {n}" in r.text
        for route in ("/synthesize_stream", "/synthesize_stream_marks"):
            assert cl.post(route, json=body).status_code == 400, route
    finally:
        pipe.close(); bs.close(); vs.close()
