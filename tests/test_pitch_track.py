"""The pitch contour tracked across frames (sbv2_pitch_track, sbv2_pipeline_fetch_request_tracked, sbv2_debug_pitch_track; csrc/track.hip and the
candidate output of k_pitch_yin_cand in csrc/marks.hip): the ABI and its refusals, a numpy restatement of the definition judged as a tracker
(CPU), the routes against fakes (CPU), the kernels launch by launch against that restatement and the pipeline on tiny models (GPU).

The references.  `candidates_ref` restates the candidates of a frame from int64 sums (float64 for f32), `track_ref` the best path: SEQUENTIAL,
frame after frame, in Python integers, with no knowledge of cuts or runs.  Everything after the c values is integer arithmetic, so the device's
path equals track_ref's everywhere, bit for bit, whatever the library does with runs; for the integer encodings c has one rounding (§8m), so
the candidates (ncand, tau, q, c3) are equal bit for bit as well.  f32: the order of the sums is the library's own, c within 1e-9 (§8m's rule);
a frame whose candidate list the reference itself decides by less than 1e-9 is exempt from the list comparison (at most 2 % of the frames), and
the path is pinned by feeding track_ref the device's own candidates."""
import base64
import ctypes as C
import functools
import json
import os
import re
import types

import numpy as np
import pytest

import flac_reader as R
from helpers import blob, make_utts, weights
from sbv2_api_amd import _lib, batcher, model, orchestrator, synth
from test_pitch import (F0_MAX, F0_MIN, MARGIN, THRESHOLD, encoded, f32_case, glide, hook, lags_np, medley, noise, tone, values_of, yin_ref)

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["sbv2_pipeline_fetch_request_tracked", "sbv2_debug_pitch_track"]
NCAND, REC = 7, 15
DEFAULTS = dict(cand_max=0.5, unvoiced_cost=0.30, switch_cost=0.20, jump_cost=1.0)
f64p, i32p = C.POINTER(C.c_double), C.POINTER(C.c_int32)


def fixed(v):
    """llrint(v * 65536): numpy rounds half to even as llrint does."""
    return int(np.rint(np.float64(v) * 65536.0))


# ---- the references -------------------------------------------------------------------------------------------------------------------------------------

def cmnd_frames(v, sr, hop, f0_min=F0_MIN, f0_max=F0_MAX):
    """c(1 .. tau_max) of every frame as sbv2_pitch defines it (yin_ref's arithmetic): [nf][tau_max + 1], entry 0 unused (NaN)."""
    v = np.asarray(v)
    assert v.dtype in (np.int64, np.float64)
    n = v.size
    tau_min, W = lags_np(sr, f0_min, f0_max)
    nf = -(-n // hop) if n else 0
    tau = np.arange(1, W + 1)
    out = np.full((nf, W + 1), np.nan)
    for f in range(nf):
        b = f * hop + hop // 2 - W
        idx = b + np.arange(2 * W)
        ok = (idx >= 0) & (idx < n)
        w = np.where(ok, v[np.clip(idx, 0, max(n - 1, 0))], 0).astype(v.dtype)
        rows = np.lib.stride_tricks.sliding_window_view(w, W)[1:W + 1]
        e = w[None, :W] - rows
        d = (e * e).sum(axis=1)
        S = np.cumsum(d)
        with np.errstate(invalid="ignore", divide="ignore"):
            out[f, 1:] = np.where(S == 0, 1.0, d.astype(np.float64) * tau.astype(np.float64) / S.astype(np.float64))
    return out


def candidates_ref(c, tau_min, cand_max):
    """The candidates of every frame from its c values -> table [nf][15] int32 (ncand, 7 tau, 7 q; 0 in absent slots), c3 [nf][7][3], and
    marginal [nf]: a dip test or the choice of the 7 smallest hangs on a difference below MARGIN."""
    nf, W = c.shape[0], c.shape[1] - 1
    tab, c3, marginal = np.zeros((nf, REC), np.int32), np.zeros((nf, NCAND, 3)), np.zeros(nf, bool)
    for f in range(nf):
        cf = np.concatenate([c[f], [np.inf]])
        t = np.arange(tau_min, W + 1)
        with np.errstate(invalid="ignore"):
            dip = (cf[t] < cf[t - 1]) & (cf[t] <= cf[t + 1]) & (cf[t] < cand_max)
            near = (np.abs(cf[t] - cf[t - 1]) < MARGIN) | (np.abs(cf[t] - cf[t + 1]) < MARGIN) | (np.abs(cf[t] - cand_max) < MARGIN)
        marginal[f] = bool(near.any())
        dips = t[dip]
        order = sorted(dips, key=lambda a: (cf[a], a))
        if len(order) > NCAND:
            marginal[f] |= bool(cf[order[NCAND]] - cf[order[NCAND - 1]] < MARGIN)
        keep = sorted(order[:NCAND])
        tab[f, 0] = len(keep)
        for i, a in enumerate(keep):
            c0 = cf[a]
            tab[f, 1 + i], tab[f, 1 + NCAND + i] = a, fixed(c0)
            c3[f, i] = (cf[a - 1] if a - 1 >= 1 else c0, c0, cf[a + 1] if a + 1 <= W else c0)
            marginal[f] |= bool(abs(c0 * 65536.0 - np.floor(c0 * 65536.0) - 0.5) < 1e-4)     # q's rounding
    return tab, c3, marginal


def track_ref(tab, U, Sw, J):
    """The path of include/sbv2_hip.h's definition: frame after frame, Python integers, ties to the smaller index.  -> state [nf] int32."""
    tab = np.asarray(tab, np.int64).reshape(-1, REC)
    nf = len(tab)
    state = np.zeros(nf, np.int32)
    if nf == 0:
        return state

    def states(f):      # [(index, tau or None, local)]
        n = int(tab[f, 0])
        return [(k, int(tab[f, 1 + k]), int(tab[f, 1 + NCAND + k])) for k in range(n)] + [(7, None, U)]

    def trans(tj, tk):
        if tj is None and tk is None:
            return 0
        if tj is None or tk is None:
            return Sw
        return (J * abs(tk - tj)) // max(tk, tj)

    prev = states(0)
    cost = {k: loc for k, _, loc in prev}
    bp = [dict()]
    for f in range(1, nf):
        cur = states(f)
        new, back = {}, {}
        for k, tk, loc in cur:
            best, arg = None, None
            for j, tj, _ in prev:                       # ascending j: the first minimum is the smallest j
                v = cost[j] + trans(tj, tk)
                if best is None or v < best:
                    best, arg = v, j
            new[k], back[k] = loc + best, arg
        bp.append(back)
        cost, prev = new, cur
    last = min(sorted(cost), key=lambda k: cost[k])     # (min over a sorted list: the smallest k of equal costs)
    assert max(cost.values()) < 2 ** 52
    for f in range(nf - 1, -1, -1):
        state[f] = last
        if f:
            last = bp[f][last]
    return state


def compose_ref(plain, tab, c3, state, sr, tau_max):
    """The tracked contour from the plain one (a yin_ref-shaped namespace), the candidates and the path."""
    nf = len(state)
    out = types.SimpleNamespace(lag=plain.lag.copy(), voiced=np.zeros(nf, np.int32), c3=plain.c3.copy(), f0=np.zeros(nf), ap=np.zeros(nf))
    for f in range(nf):
        k = int(state[f])
        if k < NCAND:
            assert k < tab[f, 0]
            out.lag[f], out.voiced[f], out.c3[f] = tab[f, 1 + k], 1, c3[f, k]
        cm, c0, cp = out.c3[f]
        lag = int(out.lag[f])
        den = cm - 2.0 * c0 + cp
        delta = 0.5 * (cm - cp) / den if den > 0 and lag - 1 >= 1 and lag + 1 <= tau_max else 0.0
        out.f0[f] = sr / (lag + delta) if out.voiced[f] else 0.0
        out.ap[f] = c0
    return out


def tracked_ref(v, sr, hop, params=DEFAULTS, f0_min=F0_MIN, f0_max=F0_MAX):
    """Everything at once from the values v -> (tracked contour, plain contour, table, c3, state, marginal)."""
    tau_min, tau_max = lags_np(sr, f0_min, f0_max)
    plain = yin_ref(v, sr, hop, f0_min, f0_max)
    tab, c3, marginal = candidates_ref(cmnd_frames(v, sr, hop, f0_min, f0_max), tau_min, params["cand_max"])
    state = track_ref(tab, fixed(params["unvoiced_cost"]), fixed(params["switch_cost"]), fixed(params["jump_cost"]))
    return compose_ref(plain, tab, c3, state, sr, tau_max), plain, tab, c3, state, marginal


# ---- the signal built to defeat plain YIN ---------------------------------------------------------------------------------------------------------------
# a1(t) sin(w t) + sin(2 w t): its period is T = sr / f0, and c(T / 2) = 2 a^2 / (1 + a^2) for a steady a1 = a (the second harmonic cancels at
# T / 2, the mean of d over the lags up to T / 2 is 1 + a^2).  a1 = 0.6 gives 0.53: plain YIN answers T.  In a burst a1 drops and c(T / 2) falls
# under the threshold 0.15: "the first lag under the threshold" answers T / 2, i.e. 2 f0, although c(T) is 0.
# 16 kHz / hop 160: the window (2 tau_max = 458 samples) fits into a burst of 3 frames, a1 = 0.2 there gives 0.077.
# 44.1 kHz / hop 220: the window (1260 samples) is LONGER than a burst of 5 frames (1100), so it always sees a1 outside the burst as well, and
# with 0.6 / 0.2 the mean a^2 of a 3-frame burst's window is 0.19: c(T / 2) = 0.32, no octave error at all.  As the issue provides, a1 is
# adjusted there until the reference alone shows the error: 0.35 outside (c(T / 2) = 0.22, still above the threshold) and 0.05 inside (a 3-frame
# burst's window: mean a^2 = 0.060, c(T / 2) = 0.11).
DEFEAT = {(16000, 160): dict(a_out=0.6, a_in=0.2), (44100, 220): dict(a_out=0.35, a_in=0.05)}
DEFEAT_F0 = 131.0
BURSTS = [(12, 3), (24, 5), (38, 4)]       # (first frame, frames) within the tone


@functools.lru_cache(maxsize=None)
def defeat(sr, hop):
    """noise | the tone with its bursts | silence, s16; -> (x, tone start, tone end, [(burst start, burst end)] in samples)."""
    p = DEFEAT[(sr, hop)]
    nt = 52 * hop
    a1 = np.full(nt, p["a_out"])
    for f, k in BURSTS:
        a1[f * hop:(f + k) * hop] = p["a_in"]
    t = np.arange(nt) / sr
    w = 2 * np.pi * DEFEAT_F0
    x = a1 * np.sin(w * t) + np.sin(2 * w * t)
    head, tail = noise(sr, 21, 0.1), np.zeros(int(0.1 * sr), np.int16)
    head = head[:len(head) // hop * hop]                 # (the tone starts on a frame boundary, so the bursts cover whole frames)
    tone_ = np.round(x * 0.4 * 32767).astype(np.int16)
    s = len(head)
    return np.concatenate([head, tone_, tail]), s, s + nt, [(s + f * hop, s + (f + k) * hop) for f, k in BURSTS]


@functools.lru_cache(maxsize=None)
def defeat_ref(sr, hop):
    x = defeat(sr, hop)[0]
    return tracked_ref(values_of(x), sr, hop)


# ---- CPU: ABI and refusals --------------------------------------------------------------------------------------------------------------------------------

def c_track(reserved=(0, 0), **kw):
    p = dict(DEFAULTS, **kw)
    return _lib.Sbv2PitchTrack(p["cand_max"], p["unvoiced_cost"], p["switch_cost"], p["jump_cost"], (C.c_int32 * 2)(*reserved))


def test_new_symbols_are_exported_and_declared():
    header = open(os.path.join(ROOT, "include", "sbv2_hip.h")).read()
    l = _lib.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.SYMBOLS and getattr(l, name) is not None, name
    assert "} sbv2_pitch_track;" in header
    assert C.sizeof(_lib.Sbv2PitchTrack) == 40
    assert C.sizeof(_lib.Sbv2Pitch) == 72 and C.sizeof(_lib.Sbv2Voice) == 48          # the existing structs are as they were
    t = model.PitchTrack()
    assert (t.cand_max, t.unvoiced_cost, t.switch_cost, t.jump_cost) == tuple(DEFAULTS[k] for k in ("cand_max", "unvoiced_cost", "switch_cost", "jump_cost"))
    # the three "not built" sentences moved on
    assert "Octave-error repair is sbv2_pitch_track" in header and "contour smoothing and octave-error repair" not in header


BAD_TRACK = [(dict(cand_max=0.0), "cand_max"), (dict(cand_max=1.0001), "cand_max"), (dict(cand_max=float("nan")), "cand_max"),
             (dict(unvoiced_cost=-0.001), "unvoiced_cost"), (dict(unvoiced_cost=4.001), "unvoiced_cost"), (dict(unvoiced_cost=float("nan")), "unvoiced_cost"),
             (dict(switch_cost=-1.0), "switch_cost"), (dict(switch_cost=4.5), "switch_cost"), (dict(switch_cost=float("nan")), "switch_cost"),
             (dict(jump_cost=-0.5), "jump_cost"), (dict(jump_cost=16.5), "jump_cost"), (dict(jump_cost=float("inf")), "jump_cost"),
             (dict(reserved=(1, 0)), "reserved"), (dict(reserved=(0, -1)), "reserved")]


def _table(rows):
    """rows: per frame a list of (tau, q) -> [nf][15] int32."""
    tab = np.zeros((len(rows), REC), np.int32)
    for f, r in enumerate(rows):
        tab[f, 0] = len(r)
        for i, (tau, q) in enumerate(r):
            tab[f, 1 + i], tab[f, 1 + NCAND + i] = tau, q
    return tab


def _bad_tables():
    ok = _table([[(50, 100), (100, 200)], [], [(60, 0)]])
    out = []
    for (f, col, val), word in ((((0, 0, 8), "ncand"), ((1, 0, -1), "ncand"), ((0, 1, 0), "tau"), ((0, 2, 1201), "tau"), ((0, 2, 50), "ascending"),
                                 ((0, 2, 49), "ascending"), ((2, 8, -1), "q of"), ((0, 9, 65537), "q of"))):
        t = ok.copy()
        t[f, col] = val
        out.append((t, word))
    return ok, out


def test_refusals_through_a_null_handle_and_through_the_hook_write_nothing():
    l = _lib.lib()
    f = model.PcmFormat(16000, "s16")
    rows, place = np.array([0], np.int32), np.array([0], np.int64)
    dst, got = np.full(16, 77, np.uint8), C.c_int64(-5)
    req = _lib.Sbv2FetchRequest(rows.ctypes.data_as(i32p), 1, place.ctypes.data_as(_lib.i64p), 10, C.pointer(f.c), None, None, 0)
    f0 = np.full(6, 77.0)
    shifting, identity = _lib.Sbv2Voice(1.2, 0.8, 0, 0, 0, 0, 0), _lib.Sbv2Voice(1.0, 1.0, 0, 0, 0, 0, 0)

    def fetch(track, pitch=True, voice=None):
        q = _lib.Sbv2Pitch(160, 0, F0_MIN, F0_MAX, THRESHOLD, 4, C.cast(f0.ctypes.data + 8, f64p), None, None, -9)
        rc = l.sbv2_pipeline_fetch_request_tracked(None, 1, C.byref(req), C.byref(voice) if voice is not None else None,
                                                   C.byref(track) if track is not None else None, dst.ctypes.data, dst.nbytes, C.byref(got), None, None,
                                                   C.byref(q) if pitch else None)
        assert (f0 == 77).all() and q.n_frames == -9 and (dst == 77).all() and got.value == -5
        return rc, l.sbv2_last_error().decode()

    for kw, word in BAD_TRACK:
        rc, msg = fetch(c_track(**kw))
        assert rc != 0 and word in msg, (kw, msg)
    rc, msg = fetch(c_track(), pitch=False)                           # track with neither a pitch nor a voice that shifts
    assert rc != 0 and "needs a pitch contour or a voice" in msg
    rc, msg = fetch(c_track(), pitch=False, voice=identity)
    assert rc != 0 and "needs a pitch contour or a voice" in msg
    for kw in (dict(), dict(pitch=False, voice=shifting), dict(unvoiced_cost=0.0, switch_cost=0.0, jump_cost=0.0), dict(cand_max=1.0, jump_cost=16.0)):
        voice = kw.pop("voice", None)
        pitch = kw.pop("pitch", True)
        rc, msg = fetch(c_track(**kw), pitch=pitch, voice=voice)     # everything static passed (0 is a value, not "default"): the null handle itself
        assert rc != 0 and "bad arguments" in msg, (kw, msg)
    rc, msg = fetch(None)                                             # track NULL forwards: the same refusal as the voice entry point
    assert rc != 0 and "bad arguments" in msg
    # the hook: parameters and tables are refused before any device call
    state = np.full(5, 77, np.int32)
    ok, bad = _bad_tables()

    def hook_table(tab, track):
        rc = l.sbv2_debug_pitch_track(0, None, 0, 0, 0, None, C.byref(track) if track is not None else None, tab.ctypes.data_as(i32p), None, len(tab), None,
                                      None, state.ctypes.data_as(i32p))
        assert (state == 77).all()
        return rc, l.sbv2_last_error().decode()

    for kw, word in BAD_TRACK:
        rc, msg = hook_table(ok, c_track(**kw))
        assert rc != 0 and word in msg, (kw, msg)
    for tab, word in bad:
        rc, msg = hook_table(tab, c_track())
        assert rc != 0 and word in msg, (word, msg)
    rc, msg = hook_table(ok, None)
    assert rc != 0 and "bad arguments" in msg
    x = np.zeros(400, np.int16)
    for kw, word in BAD_TRACK + [(dict(hop=0), "hop"), (dict(f0_min=39.0), "f0_min"), (dict(capacity=2), "too small")]:
        pk = {k: kw[k] for k in ("hop", "f0_min", "capacity") if k in kw}
        tk = {k: v for k, v in kw.items() if k not in pk}
        q = _lib.Sbv2Pitch(pk.get("hop", 80), 0, pk.get("f0_min", F0_MIN), F0_MAX, THRESHOLD, pk.get("capacity", 4), C.cast(f0.ctypes.data + 8, f64p), None,
                           None, -9)
        tab = np.full((5, REC), 77, np.int32)
        rc = l.sbv2_debug_pitch_track(0, x.ctypes.data_as(C.c_void_p), 1, x.size, 8000, C.byref(q), C.byref(c_track(**tk)), None, None, 0,
                                      tab.ctypes.data_as(i32p), None, state.ctypes.data_as(i32p))
        assert rc != 0 and word in l.sbv2_last_error().decode(), (kw, l.sbv2_last_error())
        assert (f0 == 77).all() and q.n_frames == -9 and (tab == 77).all() and (state == 77).all()


# ---- CPU: the restatement as a tracker --------------------------------------------------------------------------------------------------------------------

U0, SW0, J0 = fixed(0.30), fixed(0.20), fixed(1.0)


def test_track_ref_repairs_a_single_octave_slip():
    """Steady candidates T = 100 (q small) and T / 2 = 50 (q larger); in frame 5 the half-period has the smaller q, as in a burst."""
    rows = [[(50, 30000), (100, 1000)] for _ in range(11)]
    rows[5] = [(50, 500), (100, 1500)]
    st = track_ref(_table(rows), U0, SW0, J0)
    assert (st == 1).all()                                           # the path stays on T although frame 5 alone prefers T / 2
    # frame by frame (J = 0, nothing to pay for a jump) the slip is there: that is what plain per-frame choice does
    assert list(track_ref(_table(rows), U0, SW0, 0)) == [1] * 5 + [0] + [1] * 5


def test_track_ref_keeps_a_dropout_unvoiced_and_its_neighbours_undisturbed():
    rows = [[(50, 30000), (100, 1000)] for _ in range(9)]
    whole = track_ref(_table(rows), U0, SW0, J0)
    rows[4] = []
    st = track_ref(_table(rows), U0, SW0, J0)
    assert st[4] == 7 and (np.delete(st, 4) == np.delete(whole, 4)).all() and (whole == 1).all()
    # the two sides do not influence each other: each equals the path of its own run with the cut attached
    left, right = track_ref(_table(rows[:5]), U0, SW0, J0), track_ref(_table(rows[4:]), U0, SW0, J0)
    assert list(st) == list(left) + list(right[1:])


def test_track_ref_ties_go_to_the_smaller_index():
    rows = [[(80, 700)] * 1 + [(81 + i, 700) for i in range(6)] for _ in range(6)]      # seven candidates of equal q; J = 0: every path costs the same
    assert (track_ref(_table(rows), fixed(4.0), 0, 0) == 0).all()
    assert (track_ref(_table(rows), 700, 0, 0) == 0).all()                               # unvoiced ties with them too: the smaller index wins
    assert (track_ref(_table(rows), 699, 0, 0) == 7).all()
    dup = [[(80, 5), (90, 5)], [(80, 5), (90, 5)], [(80, 5), (90, 5)]]
    assert list(track_ref(_table(dup), U0, SW0, 0)) == [0, 0, 0]
    assert list(track_ref(_table(dup), U0, SW0, J0)) == [0, 0, 0]                       # 0 -> 0 -> 0 and 1 -> 1 -> 1 tie: the last frame takes k = 0


@pytest.mark.parametrize("sr,hop", sorted(DEFEAT))
def test_the_defaults_repair_the_signal_that_defeats_plain_yin(sr, hop):
    """(a) the reference alone shows the octave error in every burst; (b) the tracked contour with the default PitchTrack is voiced and within 1 %
    (the bound test_pitch.py applies to its tones) in every frame whose window lies wholly inside the tone and unvoiced in every frame whose
    window lies wholly in noise or silence.  Left out: the frames whose window straddles an edge, at most 2 (tau_max + hop) / hop per edge."""
    x, t0, t1, bursts = defeat(sr, hop)
    tracked, plain, tab, c3, state, _ = defeat_ref(sr, hop)
    tau_max = lags_np(sr)[1]
    nf = plain.lag.size
    centre = np.arange(nf) * hop + hop // 2
    lo, hi = centre - tau_max, centre + tau_max                      # the window [lo, hi)
    # (a)
    for b0, b1 in bursts:
        inb = (centre >= b0) & (centre < b1)
        octave = inb & (plain.voiced == 1) & (np.abs(plain.f0 / (2 * DEFEAT_F0) - 1.0) < 0.03)
        assert octave.any(), (sr, b0, plain.f0[inb])
    # (b)
    inside = (lo >= t0) & (hi <= t1)
    outside = (hi <= t0) | (lo >= t1)
    edge = ~inside & ~outside
    assert inside.sum() >= 30 and outside.sum() >= 5
    assert edge.sum() <= 2 * (2 * (tau_max + hop) // hop), (int(edge.sum()), tau_max, hop)
    assert (tracked.voiced[inside] == 1).all(), (sr, np.nonzero(inside & (tracked.voiced == 0))[0])
    err = np.abs(tracked.f0[inside] / DEFEAT_F0 - 1.0)
    print(f"[track] {sr} Hz hop {hop}: plain YIN wrong in {int((inside & (np.abs(plain.f0 / DEFEAT_F0 - 1.0) >= 0.01)).sum())} of {int(inside.sum())} "
          f"inner frames, tracked worst error {100 * err.max():.3f} %")
    assert err.max() < 0.01, (sr, float(err.max()))
    assert (tracked.voiced[outside] == 0).all() and (tracked.f0[outside] == 0).all()
    assert (plain.voiced[inside] == 1).all()                        # plain YIN is voiced there too: it is its lag that slips


# ---- CPU: options and routes ------------------------------------------------------------------------------------------------------------------------------

STYLES = np.zeros((2, 4), np.float32)
FAKE_HOP = 4
REQUEST = [dict(phones=[0, 2, 0, 1, 0], word2ph=[1, 0, 3, 1], tag=0.5), None, dict(phones=[0, 3, 0], word2ph=[2, 1], tag=0.25), None]


class FakePipe:
    """test_pitch.py's fake with the voice and track keywords: records which keywords a fetch was called with."""

    def __init__(self):
        self.calls, self.runs = [], 0

    def prepare(self, utts, **kw):
        lens = np.array([FAKE_HOP * sum(int(p) + 1 for p in u["phones"]) for u in utts], np.int64)
        return types.SimpleNamespace(utts=[dict(u) for u in utts], lens=lens, ticket=None, t_lens=np.array([len(u["phones"]) for u in utts]))

    def run(self, b):
        self.runs += 1
        b.ticket = self.runs
        return b.lens

    def fetch(self, b):
        return [np.full(int(n), u["tag"], np.float32) for n, u in zip(b.lens, b.utts)]

    def fetch_request(self, b, rows, fmt, place, joined_len, gain=None, flac=False, marks=False, env_hop=0, levels=True, pitch=None, **kw):
        self.calls.append(dict(kw, marks=marks, pitch=pitch is not None))
        out = np.zeros(int(joined_len), np.float32).astype(fmt.dtype)
        st = list(range(sum(len(b.utts[r]["phones"]) for r in rows)))
        m = model.Marks(np.array(st), np.array(st) + 1, np.zeros(len(st)), np.zeros(len(st)), 0, None, None, len(out)) if marks else None
        if pitch is None:
            return (out, None, m) if marks else (out, None)
        nf = pitch.n_frames(len(out))
        pitch.f0, pitch.ap, pitch.lag = np.full(nf, 100.0), np.full(nf, 0.05), np.full(nf, 100, np.int32)
        return out, None, m, pitch

    def close(self):
        pass


def test_option_validation():
    SO = orchestrator.SynthesizeOptions
    assert SO().pitch_track is False and orchestrator.track_options(SO()) is None
    for ok in (SO(pitch_track=True, pitch_hz=100), SO(pitch_track=True, pitch_scale=1.2), SO(pitch_track=True, intonation_scale=0.5)):
        t = orchestrator.track_options(ok)
        assert isinstance(t, model.PitchTrack) and t.cand_max == 0.5
    for bad in (dict(pitch_track=True), dict(pitch_track=1, pitch_hz=100), dict(pitch_track="yes", pitch_hz=100), dict(pitch_track=None)):
        with pytest.raises(model.Sbv2Error, match="pitch_track"):
            SO(**bad)
    with pytest.raises(model.Sbv2Error, match="fetch"):
        model.StreamHandle(None, None, {}, track=model.PitchTrack())


def test_routes_name_the_keyword_only_when_asked_and_streams_refuse():
    SO = orchestrator.SynthesizeOptions
    pipe = FakePipe()
    _, mk = orchestrator.easy_synthesize_marks(pipe, REQUEST, STYLES, noise_seed=1, options=SO(pitch_hz=900))
    assert "track" not in pipe.calls[-1] and "tracked" not in mk["pitch"]                        # off: the call it always was
    _, mk = orchestrator.easy_synthesize_marks(pipe, REQUEST, STYLES, noise_seed=1, options=SO(pitch_hz=900, pitch_track=True))
    assert isinstance(pipe.calls[-1]["track"], model.PitchTrack) and mk["pitch"]["tracked"] is True and "voice" not in pipe.calls[-1]
    json.dumps(mk)
    _, mk = orchestrator.easy_synthesize_marks(pipe, REQUEST, STYLES, noise_seed=1, options=SO(pitch_scale=1.2, pitch_track=True))
    assert isinstance(pipe.calls[-1]["track"], model.PitchTrack) and "pitch" not in mk          # the shifter's contour alone: no block to label
    orchestrator.easy_synthesize(pipe, REQUEST, STYLES, noise_seed=1, options=SO(pitch_scale=1.2, pitch_track=True))
    assert isinstance(pipe.calls[-1]["track"], model.PitchTrack) and isinstance(pipe.calls[-1]["voice"], model.Voice)
    orchestrator.easy_synthesize(pipe, REQUEST, STYLES, noise_seed=1, options=SO(pitch_scale=1.2))
    assert "track" not in pipe.calls[-1]
    runs = pipe.runs
    for kw in (dict(), dict(split=True), dict(levels=True, pitch=True)):
        with pytest.raises(model.Sbv2Error, match="/synthesize_marks"):
            orchestrator.easy_synthesize_stream(None, None, REQUEST[:1], STYLES, options=SO(pitch_hz=100, pitch_track=True), **kw)
    assert pipe.runs == runs
    # the batcher carries it per request
    rb = batcher.RequestBatcher(pipe, start=False, clock=lambda: 0.0, max_wait_ms=1000.0)
    f0 = rb.submit(REQUEST, STYLES, options=SO(pitch_hz=900, pitch_track=True), noise_seed=1, marks=True)
    f1 = rb.submit(REQUEST, STYLES, options=SO(pitch_hz=900), noise_seed=1, marks=True)
    rb.start()
    rb.close()
    assert f0.result(0)[1]["pitch"]["tracked"] is True and "tracked" not in f1.result(0)[1]["pitch"]


def test_rest_takes_pitch_track_and_the_stream_routes_answer_400():
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient
    from sbv2_api_amd import rest
    wav = orchestrator.array_to_wav(np.zeros((1, 1, 10), np.float32))

    class H:
        seen = []

        def easy_synthesize(self, ident, text, style_id, speaker_id, options):
            self.seen.append(options.pitch_track)
            return wav

        def easy_synthesize_marks(self, ident, text, style_id, speaker_id, options):
            self.seen.append(options.pitch_track)
            return wav, {"sample_rate": 16000, "tokens": [], "words": []}

        def easy_synthesize_stream(self, *a, **kw):
            raise AssertionError("not reached: the request is refused first")

    h = H()
    c = TestClient(rest.make_app(h), raise_server_exceptions=False)
    assert c.post("/synthesize_marks", json={"text": "x", "ident": "m", "pitch_hz": 100, "pitch_track": True}).status_code == 200 and h.seen[-1] is True
    assert c.post("/synthesize_marks", json={"text": "x", "ident": "m", "pitch_hz": 100}).status_code == 200 and h.seen[-1] is False
    assert c.post("/synthesize", json={"text": "x", "ident": "m", "pitch_scale": 1.3, "pitch_track": True}).status_code == 200 and h.seen[-1] is True
    r = c.post("/synthesize", json={"text": "x", "ident": "m", "pitch_track": True})           # nothing to track
    assert r.status_code == 500 and "pitch_track" in r.text
    for route in ("/synthesize_stream", "/synthesize_stream_marks"):
        r = c.post(route, json={"text": "x", "ident": "m", "pitch_hz": 100, "pitch_track": True})
        assert r.status_code == 400 and "/synthesize_marks" in r.text, (route, r.text)


# ---- GPU: the path alone ------------------------------------------------------------------------------------------------------------------------------------

def random_table(rng, nf, cuts=(), p_cut=0.1, tau_lo=4, tau_hi=1200, q_hi=65536):
    rows = []
    for f in range(nf):
        n = 0 if (f in cuts or rng.random() < p_cut) else int(rng.integers(1, NCAND + 1))
        taus = np.sort(rng.choice(np.arange(tau_lo, tau_hi + 1), n, replace=False))
        rows.append([(int(t), int(rng.integers(0, q_hi + 1))) for t in taus])
    return _table(rows)


def path_on_device(tab, **kw):
    return model.debug_pitch_track(None, 0, None, model.PitchTrack(**dict(DEFAULTS, **kw)), cand=tab)


@gpu
@pytest.mark.parametrize("nf", [0, 1, 2, 63, 64, 65, 1000])
def test_the_path_alone_on_random_tables(nf):
    rng = np.random.default_rng(100 + nf)
    last = max(nf - 1, 0)
    for cuts, p_cut in (((), 0.1), ((0,), 0.1), ((last,), 0.1), ((0, last), 0.0), ((nf // 2, nf // 2 + 1), 0.05), ((), 0.0), (tuple(range(nf)), 0.0)):
        tab = random_table(rng, nf, set(cuts), p_cut)
        got = path_on_device(tab)
        np.testing.assert_array_equal(got, track_ref(tab, U0, SW0, J0), err_msg=f"nf {nf} cuts {cuts[:4]} p {p_cut}")
    tab = random_table(rng, nf, (), 0.1, tau_lo=40, tau_hi=60, q_hi=3000)       # near lags, low costs: voiced paths, jumps that are worth paying
    np.testing.assert_array_equal(path_on_device(tab, jump_cost=0.3), track_ref(tab, U0, SW0, fixed(0.3)))
    assert path_on_device(tab).tobytes() == path_on_device(tab).tobytes()


@gpu
def test_the_path_alone_on_ties_on_the_largest_costs_and_on_more_runs_than_the_grid():
    # all ties: duplicates, J = 0 and Sw = 0 (and U equal to the candidates' q: unvoiced ties too)
    rows = [[(80 + i, 700) for i in range(NCAND)] if f % 5 else [(80, 700), (90, 700)] for f in range(130)]
    for u in (4.0, 700 / 65536.0, 699 / 65536.0):
        tab = _table(rows)
        got = path_on_device(tab, unvoiced_cost=u, switch_cost=0.0, jump_cost=0.0)
        np.testing.assert_array_equal(got, track_ref(tab, fixed(u), 0, 0), err_msg=f"ties, U = {u}")
    assert (path_on_device(_table(rows), unvoiced_cost=4.0, switch_cost=0.0, jump_cost=0.0) == 0).all()
    # the largest costs: q = 65536, lags from 4 to 1200, every cost at its ceiling
    rng = np.random.default_rng(5)
    rows = [[(int(t), 65536) for t in np.sort(rng.choice([4, 5, 600, 1199, 1200, 37, 300, 900, 64], NCAND, replace=False))] for f in range(300)]
    tab = _table(rows)
    for kw in (dict(unvoiced_cost=4.0, switch_cost=4.0, jump_cost=16.0), dict(unvoiced_cost=1.5, switch_cost=4.0, jump_cost=16.0),
               dict(unvoiced_cost=4.0, switch_cost=0.0, jump_cost=16.0)):
        got = path_on_device(tab, **kw)
        np.testing.assert_array_equal(got, track_ref(tab, fixed(kw["unvoiced_cost"]), fixed(kw["switch_cost"]), fixed(kw["jump_cost"])), err_msg=str(kw))
    # 5000 frames, more than a thousand cuts: more runs than workgroups, so every workgroup takes several
    tab = random_table(np.random.default_rng(6), 5000, (), 0.3)
    assert (tab[:, 0] == 0).sum() > 1100
    np.testing.assert_array_equal(path_on_device(tab), track_ref(tab, U0, SW0, J0))


# ---- GPU: extraction, path and composition on samples -------------------------------------------------------------------------------------------------------

def track_hook(x, sr, hop, encoding=None, params=DEFAULTS, **pk):
    r = model.debug_pitch_track(x, sr, model.Pitch(hop, **pk), model.PitchTrack(**params), encoding=encoding)
    r.voiced = (r.state < NCAND).astype(np.int32)
    return r


def assert_tracked_equal(got, x, sr, hop, enc, what, params=DEFAULTS, **pk):
    """Integer encodings: candidates, path and the tracked contour bit for bit."""
    tracked, plain, tab, c3, state, _ = tracked_ref(values_of(x, enc), sr, hop, params, **pk)
    np.testing.assert_array_equal(got.cand, tab, err_msg=what + ": candidates")
    assert got.c3.tobytes() == c3.tobytes(), (what, "candidates' c values")
    np.testing.assert_array_equal(got.state, state, err_msg=what + ": path")
    np.testing.assert_array_equal(got.pitch.lag, tracked.lag, err_msg=what + ": lag")
    np.testing.assert_allclose(got.pitch.f0, tracked.f0, rtol=1e-12, atol=0, err_msg=what + ": f0")
    np.testing.assert_allclose(got.pitch.ap, tracked.ap, rtol=1e-12, atol=0, err_msg=what + ": ap")
    assert ((got.pitch.f0 == 0) == (got.state == NCAND)).all(), what
    return tracked, plain, tab, state


@gpu
@pytest.mark.parametrize("encoding", ["s16", "mulaw", "alaw"])
def test_extraction_path_and_contour_equal_the_reference(encoding):
    enc = None if encoding == "s16" else encoding
    for name, x, sr in (("medley", medley(8000), 8000), ("glide", glide(), 16000), ("defeat", defeat(16000, 160)[0], 16000)):
        y = encoded(x, encoding)
        before = hook(y, sr, sr // 100, enc)
        got = track_hook(y, sr, sr // 100, enc)
        tracked, plain, tab, state = assert_tracked_equal(got, y, sr, sr // 100, enc, f"{name} {encoding}")
        after = hook(y, sr, sr // 100, enc)                          # the candidate output does not disturb the plain kernel
        assert before.c3.tobytes() == after.c3.tobytes() and (before.lag == after.lag).all() and (before.voiced == after.voiced).all()
        assert (before.lag == plain.lag).all()
        assert (tab[:, 0] > 0).any() and (state == NCAND).any() and (state < NCAND).any()
    rng = np.random.default_rng(78)
    y = encoded(rng.integers(-32768, 32768, 3000).astype(np.int16), encoding)
    for hop, (lo, hi), params in ((80, (F0_MIN, F0_MAX), dict(DEFAULTS, cand_max=1.0)), (37, (100.0, 2000.0), dict(DEFAULTS, cand_max=1.0, unvoiced_cost=1.0)),
                                  (80, (40.0, 41.0), dict(DEFAULTS, cand_max=0.9, unvoiced_cost=2.0, jump_cost=0.1))):
        got = track_hook(y, 8000, hop, enc, params, f0_min=lo, f0_max=hi)
        _, _, tab, _ = assert_tracked_equal(got, y, 8000, hop, enc, f"random {encoding} hop {hop} {lo}-{hi}", params, f0_min=lo, f0_max=hi)
        assert tab[:, 0].max() == NCAND or hi == 41.0                # more dips than slots: the seven smallest were chosen


@gpu
def test_extraction_at_the_large_window_and_the_repair_on_the_device():
    """44.1 kHz: three lags per lane, four waves per frame; the defeat signal's octave errors are there in the plain contour and gone in the
    tracked one, on the device as in the reference."""
    x = defeat(44100, 220)[0]
    got = track_hook(x, 44100, 220)
    tracked, plain, tab, state, _ = (lambda r: (r[0], r[1], r[2], r[4], r[5]))(defeat_ref(44100, 220))
    np.testing.assert_array_equal(got.cand, tab)
    np.testing.assert_array_equal(got.state, state)
    np.testing.assert_array_equal(got.pitch.lag, tracked.lag)
    np.testing.assert_allclose(got.pitch.f0, tracked.f0, rtol=1e-12, atol=0)
    h = hook(x, 44100, 220)
    assert (np.abs(h.f0 / (2 * DEFEAT_F0) - 1.0) < 0.03).any() and not (np.abs(got.pitch.f0 / (2 * DEFEAT_F0) - 1.0) < 0.03).any()


@gpu
def test_extraction_on_f32_under_the_f32_rule():
    for seed in (11, 12):
        x, _ = f32_case(seed)
        c = cmnd_frames(x.astype(np.float64), 16000, 160)
        tab, c3, marginal = candidates_ref(c, lags_np(16000)[0], 0.5)
        got = track_hook(x, 16000, 160)
        assert marginal.sum() <= 0.02 * len(tab), (seed, int(marginal.sum()))
        keep = ~marginal
        np.testing.assert_array_equal(got.cand[keep, :1 + NCAND], tab[keep, :1 + NCAND], err_msg=f"seed {seed}: ncand and tau")
        assert np.abs(got.cand[keep, 1 + NCAND:].astype(np.int64) - tab[keep, 1 + NCAND:]).max() <= 1          # q: c within 1e-9 moves a rounding at most
        assert np.abs(got.c3[keep] - c3[keep]).max() <= 1e-9
        np.testing.assert_array_equal(got.state, track_ref(got.cand, U0, SW0, J0), err_msg=f"seed {seed}: the path on the device's own candidates")
        assert track_hook(x, 16000, 160).cand.tobytes() == got.cand.tobytes()
    x = medley(8000)                                                 # s16 / 32768 as f32: the s16 bits
    a, b = track_hook(x, 8000, 80), track_hook(x.astype(np.float32) / np.float32(32768.0), 8000, 80)
    assert a.cand.tobytes() == b.cand.tobytes() and a.c3.tobytes() == b.c3.tobytes() and (a.state == b.state).all()


@gpu
def test_edge_shapes():
    """8 kHz: tau_max = 115 (one wave per frame at tau_max <= 64 needs a higher f0_min: 130 Hz gives 62).  n = 0, 1, below tau_min, one frame,
    all silence (every frame a cut)."""
    rng = np.random.default_rng(4)
    for n, hop, lo in ((0, 80, F0_MIN), (1, 80, F0_MIN), (9, 80, F0_MIN), (80, 80, F0_MIN), (81, 80, F0_MIN), (300, 7, F0_MIN), (700, 80, 130.0)):
        x = np.concatenate([tone(173.9, 8000)[:n // 2], rng.integers(-3000, 3000, n - n // 2).astype(np.int16)])
        got = track_hook(x, 8000, hop, None, dict(DEFAULTS, cand_max=0.9), f0_min=lo)
        assert len(got.state) == (-(-n // hop) if n else 0)
        assert_tracked_equal(got, x, 8000, hop, None, f"edge n = {n} hop = {hop} f0_min = {lo}", dict(DEFAULTS, cand_max=0.9), f0_min=lo)
    x = np.zeros(1000, np.int16)
    got = track_hook(x, 8000, 80)
    assert (got.cand == 0).all() and (got.state == NCAND).all() and (got.pitch.f0 == 0).all() and (got.pitch.ap == 1.0).all()
    assert_tracked_equal(got, x, 8000, 80, None, "silence")


# ---- GPU: the pipeline ----------------------------------------------------------------------------------------------------------------------------------------

FORMS = [("s16", 16000, False), ("mulaw", 8000, False), ("f32", 44100, False), ("s16", 16000, True)]
VOICE = (1.2, 0.8)
# The tiny models' rows are noise-like and SHORT (432 - 928 native samples: 10 - 21 ms on a timeline that is mostly the silent gaps), shorter
# than the window of the default range (2 tau_max = 458 samples at 16 kHz): measured at 16 kHz s16 with 70 - 600 Hz, 2 of 104 frames have any dip
# of c under 1 and none under the default cand_max.  The pipeline tests therefore look for pitch where such rows have structure, in
# [rate / 32, rate / 4] Hz (lags 4 .. 32, a window of 64 samples) at 400 frames per second, and track with every dip a candidate and a dear
# "unvoiced": paths through candidates in every form, and the silent gaps for cuts.
LOOSE = dict(cand_max=1.0, unvoiced_cost=0.9, switch_cost=0.2, jump_cost=0.25)


def short_range(rate):
    return dict(f0_min=rate / 32.0, f0_max=rate / 4.0)


@pytest.fixture(scope="module")
def run():
    bs, vs = model.load_model(blob("bert", "tiny", 3), True), model.load_model(blob("vits", "tiny", 5), False)
    pipe = model.Pipeline(bs, vs)
    bc, _ = weights("bert", "tiny", 3)
    vc, _ = weights("vits", "tiny", 5)
    b = pipe.prepare(make_utts([9, 14, 23], bc, vc, seed0=431, with_bert=False), sdp_ratio=0.2, noise_scale=0.6, noise_scale_w=0.8, noise_seed=17)
    pipe.run(b)
    native = [x.copy() for x in pipe.fetch(b)]
    rows = [0, 2]
    place, joined = orchestrator.joined_placement([len(native[r]) for r in rows], [0, 1], 3)
    yield types.SimpleNamespace(pipe=pipe, b=b, rows=rows, place=place, joined=joined, native=native)
    pipe.close(); bs.close(); vs.close()


@gpu
@pytest.mark.parametrize("encoding,rate,flac", FORMS, ids=["s16-16k", "mulaw-8k", "f32-44k", "flac-16k"])
def test_pipeline_tracked_contour(run, encoding, rate, flac):
    pipe, b, rows, place, joined = run.pipe, run.b, run.rows, run.place, run.joined
    fmt, hop, pk = model.PcmFormat(rate, encoding, True), rate // 400, short_range(rate)          # (peak-normalised: the tiny models' rows are faint)
    assert lags_np(rate, **pk) == (4, 32)
    kw = dict(flac=flac, marks=True, env_hop=hop)
    plain, _, pm, pp = pipe.fetch_request(b, rows, fmt, place, joined, pitch=model.Pitch(hop, **pk), **kw)
    plain = plain if flac else plain.copy()
    out, _, m, p = pipe.fetch_request(b, rows, fmt, place, joined, pitch=model.Pitch(hop, **pk), track=model.PitchTrack(**LOOSE), **kw)
    assert (out == plain) if flac else (out.dtype == plain.dtype and out.tobytes() == plain.tobytes())     # the audio bytes of the untracked fetch
    for x, y in zip(pm.arrays(), m.arrays()):
        assert x.tobytes() == y.tobytes()
    samples = np.asarray(R.read(out)["samples"], np.int16) if flac else out
    enc = encoding if encoding in ("mulaw", "alaw") else None
    h = track_hook(samples, rate, hop, enc, LOOSE, **pk)             # the hook on the delivered samples
    assert h.pitch.f0.tobytes() == p.f0.tobytes() and h.pitch.ap.tobytes() == p.ap.tobytes() and (h.pitch.lag == p.lag).all()
    if encoding != "f32":
        assert_tracked_equal(h, samples, rate, hop, enc, f"pipeline {encoding} {rate}", LOOSE, **pk)
    assert (h.cand[:, 0] == 0).any() and (h.cand[:, 0] > 1).any()    # the cuts of the silent gaps, and frames with a choice
    on = h.state < NCAND
    print(f"[track] pipeline {encoding} {rate}: {int(on.sum())} of {len(on)} frames on candidates, {int((p.lag != pp.lag).sum())} lags differ from the plain contour's")
    assert on.sum() >= 3 and (~on).any()                             # a path through candidates in every form (the rows are a few frames long)
    assert (p.f0 > 0).tolist() == on.tolist()
    # track = None is the call without; a second tracked fetch of the ticket: identical bits
    out0, _, m0, p0 = pipe.fetch_request(b, rows, fmt, place, joined, pitch=model.Pitch(hop, **pk), track=None, **kw)
    assert p0.f0.tobytes() == pp.f0.tobytes() and p0.lag.tobytes() == pp.lag.tobytes() and p0.ap.tobytes() == pp.ap.tobytes()
    out2, _, _, p2 = pipe.fetch_request(b, rows, fmt, place, joined, pitch=model.Pitch(hop, **pk), track=model.PitchTrack(**LOOSE), **kw)
    assert ((out2 == plain) if flac else out2.tobytes() == plain.tobytes())
    assert p2.f0.tobytes() == p.f0.tobytes() and p2.ap.tobytes() == p.ap.tobytes() and p2.lag.tobytes() == p.lag.tobytes()
    with pytest.raises(model.Sbv2Error, match="needs a pitch contour or a voice"):
        pipe.fetch_request(b, rows, fmt, place, joined, track=model.PitchTrack())


@gpu
def test_pipeline_tracked_voice_is_the_hook_fed_the_tracked_contour(run):
    pipe, b, rows, place, joined = run.pipe, run.b, run.rows, run.place, run.joined
    f0 = model.PcmFormat(44100, "f32")
    sr, hop = 44100, 44100 // 200
    tau_min, tau_max = lags_np(sr)
    period, voiced = [], []
    for r in rows:                                                   # the tracked contour of every native row, as the shifter forms its periods
        t = model.debug_pitch_track(run.native[r], sr, model.Pitch(hop), model.PitchTrack(**LOOSE))
        plain = hook(run.native[r], sr, hop)
        c3 = plain.c3.copy()
        on = t.state < NCAND
        c3[on] = t.c3[np.nonzero(on)[0], t.state[on]]
        lag = t.pitch.lag.astype(np.float64)
        den = c3[:, 0] - 2.0 * c3[:, 1] + c3[:, 2]
        both = (t.pitch.lag - 1 >= 1) & (t.pitch.lag + 1 <= tau_max)
        with np.errstate(invalid="ignore", divide="ignore"):
            delta = np.where((den > 0) & both, 0.5 * (c3[:, 0] - c3[:, 2]) / den, 0.0)
        period.append(lag + np.clip(delta, -1.0, 1.0))
        voiced.append(on.astype(np.int32))
        assert on.any() and not (t.pitch.lag == plain.lag).all()     # a contour with voiced frames, and another one than the plain
    want_rows = model.debug_voice_shift([run.native[r] for r in rows], sr, model.Voice(*VOICE), period=period, voiced=voiced)
    want = np.zeros(joined, np.float32)
    for g, pl in zip(want_rows, place):
        want[pl:pl + len(g.y)] = g.y
    got = pipe.fetch_request(b, rows, f0, place, joined, voice=model.Voice(*VOICE), track=model.PitchTrack(**LOOSE))[0].copy()
    assert got.tobytes() == want.tobytes()
    assert pipe.fetch_request(b, rows, f0, place, joined, voice=model.Voice(*VOICE), track=model.PitchTrack(**LOOSE))[0].tobytes() == got.tobytes()
    # track = None gives the bytes (and marks) of fetch_request(voice=...)
    a, _, am = pipe.fetch_request(b, rows, f0, place, joined, voice=model.Voice(*VOICE), marks=True)
    a = a.copy()
    c, _, cm = pipe.fetch_request(b, rows, f0, place, joined, voice=model.Voice(*VOICE), marks=True, track=None)
    assert a.tobytes() == c.tobytes() and all(x.tobytes() == y.tobytes() for x, y in zip(am.arrays(), cm.arrays()))
    assert a.tobytes() != got.tobytes()                              # ... which are not the tracked fetch's
    assert [x.tobytes() for x in pipe.fetch(b)] == [x.tobytes() for x in run.native]            # the run's PCM was only read


@gpu
def test_batcher_and_rest_carry_tracked():
    bs, vs = model.load_model(blob("bert", "tiny", 3), True), model.load_model(blob("vits", "tiny", 5), False)
    bc, _ = weights("bert", "tiny", 3)
    vc, _ = weights("vits", "tiny", 5)
    keys = ("input_ids", "word2ph", "phones", "tones", "langs")
    sents = [{k: u[k] for k in keys} for u in make_utts([7, 12], bc, vc, seed0=151, with_bert=False)]
    sv = synth.hash_normal(77, 3 * vc["style_dim"]).reshape(3, -1).astype(np.float32) * 0.1
    # (the range and frame rate at which the tiny models' short rows have structure, see LOOSE; the tracker's parameters are the defaults here)
    opts = lambda **kw: orchestrator.SynthesizeOptions(sample_rate=16000, encoding="s16", normalize=True, pitch_hz=400, pitch_min_hz=500.0,
                                                       pitch_max_hz=4000.0, **kw)
    pipe = model.Pipeline(bs, vs)

    def check(audio, mk):
        assert mk["pitch"]["tracked"] is True
        x = np.frombuffer(audio[44:], np.int16)
        tracked, plain, tab, _, state, _ = tracked_ref(values_of(x), 16000, 40, DEFAULTS, 500.0, 4000.0)
        print(f"[track] batcher / REST: {int((tab[:, 0] > 0).sum())} of {len(tab)} frames have candidates, {int((state < NCAND).sum())} lie on one, "
              f"{int((tracked.lag != plain.lag).sum())} lags differ from the plain contour's")
        assert (tab[:, 0] > 0).any() and (tab[:, 0] == 0).any()      # candidates under the default cand_max, and cuts
        assert [v is None for v in mk["pitch"]["f0_hz"]] == [v == 0 for v in tracked.f0]
        np.testing.assert_allclose([v or 0.0 for v in mk["pitch"]["f0_hz"]], tracked.f0, rtol=1e-12, atol=0)

    try:
        plain_audio, plain = orchestrator.easy_synthesize_marks(pipe, sents, sv, 1, 0, opts(), noise_seed=4242)
        assert "tracked" not in plain["pitch"]
        alone_audio, alone = orchestrator.easy_synthesize_marks(pipe, sents, sv, 1, 0, opts(pitch_track=True), noise_seed=4242)
        assert alone_audio == plain_audio
        check(alone_audio, alone)
        rb = batcher.RequestBatcher(pipe, start=False, max_wait_ms=1000.0)
        fut = rb.submit(sents, sv, 1, 0, opts(pitch_track=True), noise_seed=4242, marks=True)
        rb.start()
        rb.close()
        audio, mk = fut.result(0)
        assert audio == alone_audio and mk == alone
        pytest.importorskip("fastapi")
        from fastapi.testclient import TestClient
        from sbv2_api_amd import rest

        class H:
            def easy_synthesize_marks(self, ident, text, style_id, speaker_id, options):
                return orchestrator.easy_synthesize_marks(pipe, sents, sv, style_id, speaker_id, options, noise_seed=4242)

        c = TestClient(rest.make_app(H()), raise_server_exceptions=False)
        r = c.post("/synthesize_marks", json={"text": "x", "ident": "m", "style_id": 1, "sample_rate": 16000, "encoding": "s16", "normalize": True, "pitch_hz": 400,
                                              "pitch_min_hz": 500.0, "pitch_max_hz": 4000.0, "pitch_track": True})
        assert r.status_code == 200, r.text
        assert base64.b64decode(r.json()["audio"]) == alone_audio and r.json()["marks"] == json.loads(json.dumps(alone))
    finally:
        pipe.close(); bs.close(); vs.close()
