"""Levels and envelope in a stream's speech marks: the fed level reduction (csrc/marks.hip StreamLevels, sbv2_debug_stream_levels), the C ABI
(sbv2_stream_begin_request_levels, sbv2_stream_next_marks), model.StreamHandle(levels=, env_hop=), orchestrator.easy_synthesize_stream(levels=True)
and POST /synthesize_stream_marks.  The yardstick of every level is the one-shot reduction (sbv2_debug_segment_levels, held to numpy by
test_marks.py): a streamed level has its f64 bits, whatever the pushes."""
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
from test_marks import FORCED, N_SAMPLES, SEG_LENS, check_levels

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["sbv2_stream_begin_request_levels", "sbv2_stream_next_marks", "sbv2_debug_stream_levels"]
f64p = C.POINTER(C.c_double)
FILL = 77.0


# ---- the completion rule of the header, restated -------------------------------------------------------------------------------------------

def rule_np(ends, env_hop, total, delivered):
    """With D samples out, token t is complete once end[t] <= D and frame f once min((f + 1) env_hop, total) <= D.  delivered = D after each
    call -> per call (tok_first, n_tok, env_first, n_env): what became complete since the call before."""
    ends = np.asarray(ends, np.int64)
    nenv = -(-total // env_hop) if env_hop > 0 else 0
    out, t0, f0 = [], 0, 0
    for D in delivered:
        t1 = int((ends <= D).sum())
        f1 = 0 if not nenv else nenv if D >= total else D // env_hop
        out.append((t0, t1 - t0, f0, f1 - f0))
        t0, f0 = t1, f1
    return out


def level_delivery(consumed, A):
    """The level stream's delivery rule: max(0, S - A) samples out after S were fed, everything with the last call."""
    out, fed = [], 0
    for i, n in enumerate(consumed):
        fed += int(n)
        out.append(fed if i == len(consumed) - 1 else max(0, fed - A))
    return out


# ---- CPU: ABI, refusals, the rule ------------------------------------------------------------------------------------------------------------

def test_new_symbols_are_exported_and_declared():
    header = open(os.path.join(ROOT, "include", "sbv2_hip.h")).read()
    l = _lib.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.SYMBOLS and getattr(l, name) is not None, name
    assert "} sbv2_stream_levels;" in header and "} sbv2_stream_marks_part;" in header
    assert C.sizeof(_lib.Sbv2StreamLevels) == 16 and C.sizeof(_lib.Sbv2StreamMarksPart) == 88
    assert "NOT built on streams" not in header


def test_begin_refusals_that_need_no_run():
    l = _lib.lib()
    for lv, word in ((_lib.Sbv2StreamLevels(1, 160, (C.c_int32 * 2)(0, 1)), "reserved"), (_lib.Sbv2StreamLevels(1, 160, (C.c_int32 * 2)(3, 0)), "reserved"),
                     (_lib.Sbv2StreamLevels(2, 160, (C.c_int32 * 2)(0, 0)), "tokens"), (_lib.Sbv2StreamLevels(-1, 0, (C.c_int32 * 2)(0, 0)), "tokens"),
                     (_lib.Sbv2StreamLevels(1, -1, (C.c_int32 * 2)(0, 0)), "env_hop")):
        h, tot, nt, ne = C.c_void_p(0x55), C.c_int64(-5), C.c_int64(-6), C.c_int64(-7)
        assert l.sbv2_stream_begin_request_levels(None, None, None, None, None, None, None, 16, None, C.byref(lv), C.byref(h), C.byref(tot), C.byref(nt),
                                                  C.byref(ne)) != 0
        assert word in l.sbv2_last_error().decode(), l.sbv2_last_error()
        assert h.value == 0x55 and (tot.value, nt.value, ne.value) == (-5, -6, -7)
    # everything static passed: the null handles themselves
    lv = _lib.Sbv2StreamLevels(1, 160, (C.c_int32 * 2)(0, 0))
    assert l.sbv2_stream_begin_request_levels(None, None, None, None, None, None, None, 16, None, C.byref(lv), None, None, None, None) != 0
    assert b"bad arguments" in l.sbv2_last_error()
    assert l.sbv2_stream_next_marks(None, None) != 0 and b"bad arguments" in l.sbv2_last_error()


def _hook(x, enc, cuts, st, en, hop, device=0):
    """sbv2_debug_stream_levels with a guard word around every output -> (rc, outputs without guards, all arrays)."""
    cuts, st, en = (np.ascontiguousarray(np.asarray(a, np.int64).reshape(-1)) for a in (cuts, st, en))
    nenv = -(-x.size // hop) if hop > 0 else 0
    arrs = [np.full(n + 2, FILL) for n in (st.size, st.size, nenv, nenv)] + [np.full(cuts.size + 3, 77, np.int64) for _ in range(2)]
    q = lambda a, t: C.cast(a.ctypes.data + 8, t)
    rc = _lib.lib().sbv2_debug_stream_levels(device, x.ctypes.data_as(C.c_void_p), enc, x.size, cuts.ctypes.data_as(_lib.i64p) if cuts.size else None,
                                             cuts.size, st.ctypes.data_as(_lib.i64p), en.ctypes.data_as(_lib.i64p), st.size, hop,
                                             *(q(a, f64p) for a in arrs[:4]), *(q(a, _lib.i64p) for a in arrs[4:]))
    return rc, [a[1:-1] for a in arrs], arrs


def test_hook_refusals_that_need_no_run():
    l = _lib.lib()
    x = np.arange(100, dtype=np.int16)
    for cuts, st, en, hop, word in (([], [0, 10, 5], [3, 20, 8], 0, "monotone and disjoint"),     # goes back
                                    ([], [0, 10], [11, 20], 0, "monotone and disjoint"),          # overlaps by one sample
                                    ([], [0, 10], [3, 9], 0, "outside"),                          # end before start
                                    ([], [0, 90], [3, 101], 0, "outside"),                        # past the signal
                                    ([50, 40], [0, 10], [3, 20], 7, "cuts must ascend"),
                                    ([50, 101], [0, 10], [3, 20], 7, "cuts must ascend"),
                                    ([], [0, 10], [3, 20], -1, "env_hop")):
        rc, _, arrs = _hook(x, 1, cuts, st, en, hop, device=99)   # (refused before the device is looked at)
        assert rc != 0 and word in l.sbv2_last_error().decode(), (word, l.sbv2_last_error())
        assert all((a == 77).all() for a in arrs), "a refused call wrote something"


def test_completion_rule_partitions_tokens_and_frames_in_order():
    # empty spans at 0, a token that ends exactly at a call's edge (300), unowned silence (300 .. 340), an empty span inside, the last one short of the end
    st = np.array([0, 0, 0, 120, 300, 340, 340, 900], np.int64)
    en = np.array([0, 0, 120, 300, 300, 340, 900, 1000], np.int64)
    total, hop = 1010, 64
    calls = [300, 0, 45, 555, 110]
    D = list(np.cumsum(calls))
    got = rule_np(en, hop, total, D)
    assert got[0] == (0, 5, 0, 4)            # both empty spans at 0, the token ending AT the edge and the empty one there; frames 0 .. 3 (256 <= 300)
    assert got[1] == (5, 0, 4, 0)            # an empty call completes nothing
    assert got[2] == (5, 1, 4, 1)            # D = 345: the empty span at 340, frame 4 (320)
    nenv = -(-total // hop)
    assert sum(g[1] for g in got) == len(en) and sum(g[3] for g in got) == nenv
    for a, b in zip(got, got[1:]):           # contiguous, in order
        assert b[0] == a[0] + a[1] and b[2] == a[2] + a[3]
    assert got[-1][2] + got[-1][3] == nenv and (nenv - 1) * hop < total < nenv * hop   # the short last frame completes with the end only
    # D = 0 before anything is delivered: the empty spans at 0 are complete at once
    assert rule_np(en, hop, total, [0])[0] == (0, 2, 0, 0)
    # the level rule: the first call feeds less than A and emits nothing, the last call emits the rest
    A = 491
    D = level_delivery(calls, A)
    assert D == [0, 0, 0, 409, 1010]
    got = rule_np(en, hop, total, D)
    assert got[0] == (0, 2, 0, 0) and got[3][1] > 0 and got[4][0] + got[4][1] == len(en) and got[4][2] + got[4][3] == nenv
    # tokens only / envelope only
    assert all(g[3] == 0 for g in rule_np(en, 0, total, D))
    assert all(g[1] == 0 for g in rule_np([], hop, total, D))


# ---- GPU, the hook: bit equality with the one-shot kernel ---------------------------------------------------------------------------------------

def _layout(holes):
    """SEG_LENS laid adjacent from sample 0, or with unowned holes of 1 and 500 samples (in turn) between them; the tail belongs to nobody."""
    st, en, at = [], [], 0
    for i, n in enumerate(SEG_LENS):
        st.append(at); en.append(at + n)
        at += n + ((1, 500)[i % 2] if holes else 0)
    assert en[-1] < N_SAMPLES
    return np.array(st, np.int64), np.array(en, np.int64)


def _cut_sets(st, en, rng):
    edges = sorted(set(int(v) for v in np.concatenate([st, en])))
    k = lambda n: int(st[SEG_LENS.index(n)])
    s255, s256, s257, s4097, s60000 = k(255), k(256), k(257), k(4097), k(60000)
    through = sorted(set(c for s0, n in ((s255, 255), (s256, 256), (s257, 257)) for c in range(s0 + 50, s0 + n, 50)))
    assert len([c for c in through if s255 < c < s255 + 255]) >= 4            # a short segment spans more than 3 pushes
    inside = [s60000 + o for o in (1, 255, 257, 1000, 4097, 30001, 59999)]
    assert all((c - s60000) % 256 for c in inside)
    return {
        "none": [],
        "every 1000": list(range(1000, N_SAMPLES, 1000)),
        "on every edge": [e for e in edges if 0 <= e <= N_SAMPLES],
        "edges +- 1": sorted(set(c for e in edges for c in (e - 1, e + 1) if 0 <= c <= N_SAMPLES)),
        "20 random with repeats": sorted(list(rng.integers(0, N_SAMPLES + 1, 14)) + [0, 0, 777, 777, N_SAMPLES, N_SAMPLES]),
        "one sample": [64, 65, 66, 67],
        "pushes of 50": through,
        "inside 4097": [s4097 + 257, s4097 + 4096],
        "inside 60000": inside,
    }


def _signal(kind):
    rng = np.random.default_rng(2027)
    if kind == "s16":
        x = rng.integers(-32768, 32768, N_SAMPLES).astype(np.int16)
        x[100:400] = 32767; x[5000:9500] = -32767; x[20000:68000:2] = 32767; x[20001:68000:2] = -32767
        return x, 1, None
    if kind == "f32":
        return (rng.standard_normal(N_SAMPLES) * np.exp(rng.uniform(-12, 2, N_SAMPLES))).astype(np.float32), 0, None
    return rng.integers(0, 256, N_SAMPLES).astype(np.uint8), model.ENCODINGS["mulaw"], "mulaw"


@gpu
@pytest.mark.parametrize("kind", ["s16", "f32", "mulaw"])
def test_fed_reduction_has_the_bits_of_the_one_shot_kernel(kind):
    x, enc, law = _signal(kind)
    decoded = model.g711_decode(x, law).astype(np.int16) if law else x
    rng = np.random.default_rng(5)
    # (4999 besides the issue's four: 70000 = 14 * 5000, so only 4999 ends on a SHORT last frame behind whole-workgroup frames)
    hops = (7, 64, 441, 5000, 4999)
    assert N_SAMPLES % 5000 == 0 and 0 < N_SAMPLES % 4999 <= 4096
    env = {}
    for hop in hops:   # the envelope's yardstick: once per hop
        fs = np.arange(0, N_SAMPLES, hop, dtype=np.int64)
        fe = np.minimum(fs + hop, N_SAMPLES)
        env[hop] = (fs, fe) + model.debug_segment_levels(x, fs, fe, encoding=law)
        check_levels(decoded, fs, fe, env[hop][2], env[hop][3], f"one-shot envelope {hop} {kind}")
    runs = 0
    for holes in (False, True):
        st, en = _layout(holes)
        ws, wp = model.debug_segment_levels(x, st, en, encoding=law)
        check_levels(decoded, st, en, ws, wp, f"one-shot segments {kind}")
        assert ws[0] == 0 and ws[SEG_LENS.index(60000)] > 0
        for name, cuts in _cut_sets(st, en, rng).items():
            D = list(cuts) + [N_SAMPLES]
            for hop in hops:
                rc, (ss, pk, es, ep, sp, epp), arrs = _hook(x, enc, cuts, st, en, hop)
                assert rc == 0, _lib.lib().sbv2_last_error()
                what = f"{kind} holes={holes} cuts={name} hop={hop}"
                assert all(a[0] == 77 and a[-1] == 77 for a in arrs), what + ": guard words"
                assert ss.tobytes() == ws.tobytes() and pk.tobytes() == wp.tobytes(), (what, np.flatnonzero(ss != ws), np.flatnonzero(pk != wp))
                assert es.tobytes() == env[hop][2].tobytes() and ep.tobytes() == env[hop][3].tobytes(), (what, np.flatnonzero(es != env[hop][2])[:8])
                want = rule_np(en, hop, N_SAMPLES, D)
                assert list(sp[:len(D)]) == [w[1] for w in want] and list(epp[:len(D)]) == [w[3] for w in want], what
                runs += 1
        # the same samples 3 further on, segments and cuts moved with them: the same bits
        y = np.concatenate([np.zeros(3, x.dtype), x])
        rc, (ss, pk, *_), _ = _hook(y, enc, [c + 3 for c in _cut_sets(st, en, rng)["edges +- 1"] if c + 3 <= y.size], st + 3, en + 3, 441)
        assert rc == 0 and ss.tobytes() == ws.tobytes() and pk.tobytes() == wp.tobytes(), f"{kind} holes={holes}: moved by 3"
    assert runs == 2 * 9 * 5
    # the wrapper gives the same answer
    st, en = _layout(True)
    got = model.debug_stream_levels(x, [1000, 1000, 30000], st, en, 441, encoding=law)
    assert got[0].tobytes() == ws.tobytes() and got[2].tobytes() == env[441][2].tobytes() and got[4].sum() == len(st)


# ---- GPU: streams of the tiny models ------------------------------------------------------------------------------------------------------------

LONG_ROW = [2, 300, 0, 1, 5]
ROWS = FORCED + [LONG_ROW]
GAPS = (64, 22050, 100, 0)


def _gaps(fmt):
    """GAPS, an inner gap raised to the format's minimum where it lies below (24 kHz: 118 native samples; a shorter one is refused)."""
    mg = model.stream_min_gap(fmt)
    return tuple(max(g, mg) if i < len(GAPS) - 1 else g for i, g in enumerate(GAPS))

F = model.PcmFormat
STREAMS = {   # name -> (fmt or None = the identity format, flac, level)
    "identity": (None, False, False), "44k1-f32": (F(44100, "f32"), False, False), "48k-s16": (F(48000, "s16"), False, False),
    "24k-s16": (F(24000, "s16"), False, False), "48k-mulaw": (F(48000, "mulaw"), False, False), "flac": (F(48000, "s16"), True, False),
    "level-f32": (F(48000, "f32"), False, True), "level-s16-flac": (F(48000, "s16"), True, True),
}


def _four():
    bc, _ = weights("bert", "tiny", 3)
    vc, _ = weights("vits", "tiny", 5)
    utts = make_utts([4, 5, 6, 2], bc, vc, seed0=811, with_bert=False)
    assert [len(u["phones"]) for u in utts] == [len(d) for d in ROWS]
    return [dict(u, forced_durations=np.array(d, np.int64)) for u, d in zip(utts, ROWS)]


@pytest.fixture(scope="module")
def tiny():
    """The two tiny sessions and, fetched from ONE pipeline run before any stream reuses the sessions, the marks of the joined fetch in every
    format a non-level stream below delivers."""
    bs, vs = model.load_model(blob("bert", "tiny", 3), True), model.load_model(blob("vits", "tiny", 5), False)
    hop = _lib.lib().sbv2_vits_hop(vs.handle)
    assert hop == 16
    pipe = model.Pipeline(bs, vs)
    utts = _four()
    b = pipe.prepare(utts, forced=True)
    pipe.run(b)
    lens = [int(n) for n in b.lens]
    assert lens == [hop * sum(d) for d in ROWS]
    fetched = {}
    for name, (fmt, flac, level) in STREAMS.items():
        ff = fmt or F(44100, "f32")
        gaps, place = _gaps(fmt), [0]
        for n, g in zip(lens[:-1], gaps[:-1]):
            place.append(place[-1] + n + g)
        joined = place[-1] + lens[-1] + gaps[-1]
        if not level and (ff.sample_rate, ff.encoding) not in fetched:
            out, _, m = pipe.fetch_request(b, range(4), ff, place, joined, marks=True, env_hop=ff.sample_rate // 100)
            fetched[(ff.sample_rate, ff.encoding)] = (out.copy(), m)
    yield dict(bs=bs, vs=vs, hop=hop, utts=utts, frames=[n // hop for n in lens], fetched=fetched)
    pipe.close(); bs.close(); vs.close()


def _take_with_marks(st, short_at=None):
    """Every piece of the stream, sbv2_stream_next_marks after each -> (pieces, per call (tok_first, n_tok, env_first, n_env, delivered), the
    levels in order).  short_at: at that call a capacity one short is tried first: refused, nothing written, nothing lost."""
    l = _lib.lib()
    pieces, calls, acc = [], [], [[], [], [], []]
    while (p := st.next()) is not None:
        if short_at is not None and len(pieces) == short_at[0]:
            nt, ne = short_at[1], short_at[2]
            for tc, ec, word in ((nt - 1, ne, "token arrays too small"), (nt, ne - 1, "envelope arrays too small")):
                bufs = [np.full(max(nt, ne, 1) + 2, FILL) for _ in range(4)]
                part = _lib.Sbv2StreamMarksPart(tc, bufs[0].ctypes.data_as(f64p), bufs[1].ctypes.data_as(f64p), -3, -3, ec,
                                                bufs[2].ctypes.data_as(f64p), bufs[3].ctypes.data_as(f64p), -3, -3, -3)
                assert l.sbv2_stream_next_marks(st.h, C.byref(part)) != 0 and word in l.sbv2_last_error().decode(), l.sbv2_last_error()
                assert all((a == FILL).all() for a in bufs) and (part.tok_first, part.n_tok, part.env_first, part.n_env, part.delivered) == (-3,) * 5
            # NULL result arrays with entries pending: refused likewise, with the count named
            for null_tok, word in ((True, "NULL token arrays"), (False, "NULL envelope arrays")):
                bufs = [np.full(max(nt, ne, 1) + 2, FILL) for _ in range(4)]
                p4 = [None if (i < 2) == null_tok else b.ctypes.data_as(f64p) for i, b in enumerate(bufs)]
                part = _lib.Sbv2StreamMarksPart(nt, p4[0], p4[1], -3, -3, ne, p4[2], p4[3], -3, -3, -3)
                assert l.sbv2_stream_next_marks(st.h, C.byref(part)) != 0 and word in l.sbv2_last_error().decode(), l.sbv2_last_error()
                assert all((a == FILL).all() for a in bufs) and (part.tok_first, part.n_tok, part.env_first, part.n_env, part.delivered) == (-3,) * 5
        pieces.append(p)
        t0, ss, pk, f0, es, ep, D = st.next_marks()
        calls.append((t0, len(ss), f0, len(es), D))
        for a, v in zip(acc, (ss, pk, es, ep)):
            a.append(v)
    t0, ss, _, f0, es, _, D = st.next_marks()     # after the end: nothing is pending
    assert len(ss) == 0 and len(es) == 0 and D == st.total_samples and t0 == st.n_tokens and f0 == st.n_env
    return pieces, calls, [np.concatenate(a) for a in acc]


def _delivered_samples(pieces, fmt, flac):
    if flac:
        return R.read(b"".join(pieces))["samples"].astype(np.int16)
    return np.concatenate(pieces)


@gpu
@pytest.mark.parametrize("name", list(STREAMS))
def test_stream_levels_on_the_tiny_models(tiny, name):
    fmt, flac, level = STREAMS[name]
    ff = fmt or F(44100, "f32")
    bs, vs, hop, utts = tiny["bs"], tiny["vs"], tiny["hop"], tiny["utts"]
    lv = model.StreamLevel(6.0) if level else None
    env_hop = ff.sample_rate // 100
    law = ff.encoding if ff.encoding in model.G711 else None
    first_emits_nothing = False
    gaps = _gaps(fmt)
    assert gaps == GAPS or ff.sample_rate == 24000
    for chunk in (16, 50):
        kw = dict(fmt=fmt, flac=flac, level=lv, gaps=gaps, forced=True)
        plain = model.StreamHandle(bs, vs, utts, chunk, **kw)
        plain_marks, plain_pieces = plain.marks(), []
        while (p := plain.next()) is not None:
            plain_pieces.append(p)
        with pytest.raises(model.Sbv2Error, match="begun without levels"):
            plain.next_marks()
        plain.close()
        _, _, cs = model.stream_timeline(tiny["frames"], gaps, hop, chunk, fmt)
        total = int(cs.sum())
        D = level_delivery(cs, model.stream_level_lookahead(ff)) if level else list(np.cumsum(cs))
        first_emits_nothing |= level and D[0] == 0
        assert 4800 in [hop * d for d in LONG_ROW] and (chunk > 16 or 300 // chunk >= 18)     # the stride-256 token lies across 19 chunks of 16 frames

        st = model.StreamHandle(bs, vs, utts, chunk, levels=True, env_hop=env_hop, **kw)
        s, e = st.marks()
        assert st.total_samples == total and st.n_tokens == len(s) == sum(len(d) for d in ROWS) and st.n_env == -(-total // env_hop)
        assert np.array_equal(s, plain_marks[0]) and np.array_equal(e, plain_marks[1])              # sbv2_stream_marks is unchanged
        assert ((e - s).max() > 4096 or ff.sample_rate < 44100) and (e[:-1] <= s[1:]).all()     # (a stride-256 token at every rate from 44.1 kHz up)
        want = rule_np(e, env_hop, total, D)
        short = next((i, w[1], w[3]) for i, w in enumerate(want) if w[1] >= 1 and w[3] >= 1)
        pieces, calls, (ss, pk, es, ep) = _take_with_marks(st, short)
        st.close()
        what = f"{name} chunk {chunk}"
        assert [c[:4] for c in calls] == want and [c[4] for c in calls] == D, what
        assert calls[-1][0] + calls[-1][1] == len(s) and calls[-1][2] + calls[-1][3] == -(-total // env_hop), what     # the last call completes the rest
        # the audio is that of the same stream without levels
        assert len(pieces) == len(plain_pieces) and all(bytes(memoryview(a)) == bytes(memoryview(b)) for a, b in zip(pieces, plain_pieces)), what
        # the levels are those of the one-shot reduction on the delivered samples
        x = _delivered_samples(pieces, ff, flac)
        assert x.size == total
        fs = np.arange(0, total, env_hop, dtype=np.int64)
        fe = np.minimum(fs + env_hop, total)
        ws, wp = model.debug_segment_levels(x, s, e, encoding=law)
        wes, wep = model.debug_segment_levels(x, fs, fe, encoding=law)
        assert ss.tobytes() == ws.tobytes() and pk.tobytes() == wp.tobytes(), (what, np.flatnonzero(ss != ws))
        assert es.tobytes() == wes.tobytes() and ep.tobytes() == wep.tobytes(), (what, np.flatnonzero(es != wes)[:8])
        assert (ss[s == e] == 0).all() and ss[(e - s).argmax()] > 0
        if not level:   # ... and, the audio being byte-equal to the joined fetch, those of the fetch's marks
            out, m = tiny["fetched"][(ff.sample_rate, ff.encoding)]
            assert out.tobytes() == x.tobytes() and np.array_equal(m.start, s) and np.array_equal(m.end, e), what
            assert m.sumsq.tobytes() == ss.tobytes() and m.peak.tobytes() == pk.tobytes(), what
            assert m.env_sumsq.tobytes() == es.tobytes() and m.env_peak.tobytes() == ep.tobytes(), what
    assert first_emits_nothing == bool(level)


@gpu
def test_one_utterance_with_levels_is_its_request_stream_with_gap_0(tiny):
    bs, vs, u = tiny["bs"], tiny["vs"], tiny["utts"][3]
    fmt = F(48000, "s16")
    a = model.StreamHandle(bs, vs, u, 16, fmt=fmt, levels=True, env_hop=480, forced=True)
    pa, ca, la = _take_with_marks(a)
    a.close()
    r = model.StreamHandle(bs, vs, [u], 16, fmt=fmt, gaps=[0], levels=True, env_hop=480, forced=True)
    pr, cr, lr = _take_with_marks(r)
    r.close()
    assert ca == cr and len(pa) == len(pr) > 18 and all(x.tobytes() == y.tobytes() for x, y in zip(pa, pr))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(la, lr)) and la[0].max() > 0
    # tokens only, envelope only: the other table is empty; levels off is the stream without
    t = model.StreamHandle(bs, vs, u, 16, fmt=fmt, levels=True, forced=True)
    _, ct, lt = _take_with_marks(t)
    t.close()
    assert t.n_env == 0 and lt[0].tobytes() == la[0].tobytes() and lt[2].size == 0 and [c[:2] for c in ct] == [c[:2] for c in ca]
    e = model.StreamHandle(bs, vs, u, 16, fmt=fmt, env_hop=480, forced=True)
    _, ce, le = _take_with_marks(e)
    e.close()
    assert e.n_tokens == 0 and le[2].tobytes() == la[2].tobytes() and le[0].size == 0 and [c[2:] for c in ce] == [c[2:] for c in ca]


@pytest.fixture(scope="module")
def full_models():
    bs, vs = model.load_model(blob("bert", "full"), True), model.load_model(blob("vits", "full"), False)
    yield weights("bert", "full")[0], weights("vits", "full")[0], bs, vs
    bs.close(); vs.close()


@gpu
def test_full_model_stream_levels(full_models):
    """Two rows (60 and 30 phonemes), gap 22050, chunk 64, 16 kHz s16 on the full-size models (as test_full_model_request_stream).  The stream is
    within +-1 step of the fetch there, not equal to it, so the levels are held to the one-shot reduction of the DELIVERED samples (bit for
    bit) and to numpy (exact for s16)."""
    bc, vc, bs, vs = full_models
    utts = [synth.make_utterance(60, bc, vc, seed=91), synth.make_utterance(30, bc, vc, seed=92)]
    fmt = F(16000, "s16")
    st = model.StreamHandle(bs, vs, utts, 64, fmt=fmt, gaps=(22050, 0), levels=True, env_hop=160, forced=True)
    s, e = st.marks()
    pieces, calls, (ss, pk, es, ep) = _take_with_marks(st)
    total = st.total_samples
    st.close()
    x = np.concatenate(pieces)
    assert x.size == total and len(pieces) > 2
    assert [c[:4] for c in calls] == rule_np(e, 160, total, list(np.cumsum([p.size for p in pieces])))
    fs = np.arange(0, total, 160, dtype=np.int64)
    fe = np.minimum(fs + 160, total)
    ws, wp = model.debug_segment_levels(x, s, e)
    wes, wep = model.debug_segment_levels(x, fs, fe)
    assert ss.tobytes() == ws.tobytes() and pk.tobytes() == wp.tobytes() and es.tobytes() == wes.tobytes() and ep.tobytes() == wep.tobytes()
    check_levels(x, s, e, ss, pk, "full model tokens")
    check_levels(x, fs, fe, es, ep, "full model envelope")
    assert ss.max() > 0 and es.max() > 0


# ---- CPU: orchestrator and REST on a fake handle ---------------------------------------------------------------------------------------------------

class FakeHandle:
    """A model.StreamHandle that follows the completion rule on a signal of its own: every token 100 samples but one empty, 37 unowned samples at
    the end, pieces of 250 samples."""
    seen = []

    def __init__(self, bert, vits, utt, chunk_frames, fmt=None, flac=False, level=None, **kw):
        type(self).seen.append((utt, kw))
        self.level, self.kw, self.fmt = level, kw, fmt or model.PcmFormat(44100, "f32")
        n = sum(len(u["phones"]) for u in utt) if isinstance(utt, list) else len(utt["phones"])
        lens = np.full(n, 100, np.int64)
        lens[1] = 0
        self.end = np.cumsum(lens)
        self.start = self.end - lens
        self.total_samples = int(self.end[-1]) + 37
        x = np.sin(np.arange(self.total_samples) * 0.37) * 0.5
        self.x = x.astype(np.float32) if self.fmt.encoding == "f32" else np.rint(x * 32767).astype(np.int16)
        self.at = self.D = self.t0 = self.f0 = 0
        self.mark_calls = 0

    def marks(self):
        return self.start, self.end

    def next(self):
        if self.at >= self.total_samples:
            return None
        c = self.x[self.at:self.at + 250]
        self.at += c.size
        self.D = self.at
        return c

    def next_marks(self):
        assert self.kw.get("levels"), "next_marks on a stream begun without levels"
        self.mark_calls += 1
        hop = self.kw.get("env_hop", 0)
        (t0, nt, f0, ne), = rule_np(self.end, hop, self.total_samples, [self.D])
        nt, ne = t0 + nt - self.t0, f0 + ne - self.f0
        lv = lambda a, b: (float((self.x[a:b].astype(np.float64) ** 2).sum()), float(np.abs(self.x[a:b].astype(np.float64)).max()) if b > a else 0.0)
        tok = [lv(int(self.start[t]), int(self.end[t])) for t in range(self.t0, self.t0 + nt)]
        env = [lv(f * hop, min((f + 1) * hop, self.total_samples)) for f in range(self.f0, self.f0 + ne)]
        out = (self.t0, np.array([v[0] for v in tok]), np.array([v[1] for v in tok]), self.f0, np.array([v[0] for v in env]),
               np.array([v[1] for v in env]), self.D)
        self.t0, self.f0 = self.t0 + nt, self.f0 + ne
        return out

    def close(self):
        pass


STYLES = np.zeros((2, 4), np.float32)
LINES = [{"phones": [0, 5, 0, 7, 0], "word2ph": [1, 3, 1]}, None, {"phones": [0, 3, 0], "word2ph": [2, 1]}]


def test_orchestrator_default_is_unchanged_and_levels_complete_the_marks(monkeypatch):
    monkeypatch.setattr(model, "StreamHandle", FakeHandle)
    O = orchestrator
    for enc in ("f32", "s16"):
        opts = O.SynthesizeOptions(encoding=enc, sample_rate=44100 if enc == "f32" else 16000, envelope_hz=100)
        # the default: the bytes it yields today (header of the known length, then the samples), no levels asked of the handle, envelope_hz ignored
        FakeHandle.seen.clear()
        st = O.easy_synthesize_stream(None, None, LINES, STYLES, 1, 7, opts, noise_seed=5, split=True)
        (utt, kw), = FakeHandle.seen
        assert "levels" not in kw and "env_hop" not in kw
        h = st._st
        plain = b"".join(st)
        assert plain == O.wav_stream_header(opts.sample_rate, enc, h.total_samples) + h.x.astype({"f32": "<f4", "s16": "<i2"}[enc]).tobytes()
        assert h.mark_calls == 0 and "envelope" not in st.marks and "level_dbfs" not in st.marks["tokens"][0]
        with pytest.raises(model.Sbv2Error, match="without levels"):
            st.take_marks()
        # levels=True: the same bytes; the union of take_marks() is the final .marks, which has marks_dict's shape and values
        FakeHandle.seen.clear()
        st = O.easy_synthesize_stream(None, None, LINES, STYLES, 1, 7, opts, noise_seed=5, split=True, levels=True)
        (utt, kw), = FakeHandle.seen
        hop = opts.sample_rate // 100
        assert kw["levels"] is True and kw["env_hop"] == hop
        h, got, toks, env, firsts, delivered = st._st, [], [], ([], []), [], []
        for i, piece in enumerate(st):
            got.append(piece)
            d = st.take_marks()
            json.dumps(d)
            if i % 2 == 0:     # (not asking loses nothing: the next call returns everything pending)
                d2 = st.take_marks()
                assert d2["tokens"] == [] and d2["envelope"]["level_dbfs"] == [] and d2["envelope"]["first"] == d["envelope"]["first"] + len(d["envelope"]["peak"])
            toks += d["tokens"]
            firsts.append(d["envelope"]["first"])
            assert d["envelope"]["first"] == len(env[0]) and d["envelope"]["hop"] == hop
            env[0].extend(d["envelope"]["level_dbfs"]); env[1].extend(d["envelope"]["peak"])
            delivered.append(d["delivered"])
        assert b"".join(got) == plain and delivered[0] == 0 and delivered[-1] == h.total_samples == st.total_samples
        last = st.take_marks()
        assert last["tokens"] == [] and last["envelope"]["peak"] == []
        assert [t["token"] for t in toks] == list(range(8))
        fmt = model.PcmFormat(opts.sample_rate, enc)
        m = model.Marks(h.start, h.end, *[np.array(v) for v in zip(*[(float((h.x[a:b].astype(np.float64) ** 2).sum()),
                                                                        float(np.abs(h.x[a:b].astype(np.float64)).max()) if b > a else 0.0)
                                                                       for a, b in zip(h.start, h.end)])],
                        env_hop=hop, env_sumsq=None, env_peak=None, out_len=h.total_samples)
        fs = range(0, h.total_samples, hop)
        m.env_sumsq = np.array([float((h.x[a:a + hop].astype(np.float64) ** 2).sum()) for a in fs])
        m.env_peak = np.array([float(np.abs(h.x[a:a + hop].astype(np.float64)).max()) for a in fs])
        want = O.marks_dict([s for s in LINES if s], [0, 2], fmt, m)
        assert st.marks == want
        assert [(t["level_dbfs"], t["peak"]) for t in toks] == [(t["level_dbfs"], t["peak"]) for t in want["tokens"]]
        assert env[0] == want["envelope"]["level_dbfs"] and env[1] == want["envelope"]["peak"]
        assert want["tokens"][1]["level_dbfs"] is None and want["tokens"][0]["level_dbfs"] is not None
    # without envelope_hz: tokens only
    st = O.easy_synthesize_stream(None, None, LINES, STYLES, 1, 7, O.SynthesizeOptions(), noise_seed=5, split=True, levels=True)
    assert FakeHandle.seen[-1][1]["env_hop"] == 0
    list(st)
    d = st.take_marks()
    assert "envelope" not in d and "envelope" not in st.marks and len(d["tokens"]) == 8
    # a bad envelope_hz is refused before any handle exists; without levels it stays ignored
    FakeHandle.seen.clear()
    for hz in (0, -5, 44101, 2.5, True):
        with pytest.raises(model.Sbv2Error, match="envelope_hz"):
            O.easy_synthesize_stream(None, None, LINES, STYLES, 1, 7, O.SynthesizeOptions(envelope_hz=hz), noise_seed=5, split=True, levels=True)
    assert FakeHandle.seen == []
    list(O.easy_synthesize_stream(None, None, LINES, STYLES, 1, 7, O.SynthesizeOptions(envelope_hz=0), noise_seed=5, split=True))


def test_rest_synthesize_stream_marks_and_the_untouched_stream_route(monkeypatch):
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient
    from sbv2_api_amd import rest
    monkeypatch.setattr(model, "StreamHandle", FakeHandle)

    class Holder:
        calls = []

        def models(self):
            return ["m"]

        def easy_synthesize_stream(self, ident, text, style_id, speaker_id, options, **kw):
            self.calls.append(kw)
            return orchestrator.easy_synthesize_stream(None, None, LINES, STYLES, style_id, speaker_id, options, noise_seed=5, **kw)

    h = Holder()
    app = rest.make_app(h)
    c = TestClient(app)
    body = {"text": "a\n\nb", "ident": "m", "split_sentences": True, "sample_rate": 16000, "encoding": "s16"}
    plain = c.post("/synthesize_stream", json=dict(body, marks=True))
    assert plain.status_code == 200 and h.calls[-1] == {"split": True}
    r = c.post("/synthesize_stream_marks", json=dict(body, envelope_hz=100))
    assert r.status_code == 200 and r.headers["content-type"].startswith("application/x-ndjson") and h.calls[-1] == {"levels": True, "split": True}
    lines = [json.loads(s) for s in r.content.decode().splitlines()]
    first, rest_ = lines[0], lines[1:]
    assert first["media_type"] == "audio/wav" and first["sample_rate"] == 16000 and first["total_samples"] == 737
    assert set(first["marks"]) == {"sample_rate", "tokens", "words"} and len(first["marks"]["tokens"]) == 8
    assert [t["line"] for t in first["marks"]["tokens"]] == [0] * 5 + [2] * 3
    assert b"".join(base64.b64decode(l["audio"]) for l in rest_) == plain.content
    assert rest_[-1]["delivered"] == first["total_samples"] and [l["delivered"] for l in rest_] == sorted(l["delivered"] for l in rest_)
    assert [t["token"] for l in rest_ for t in l["tokens"]] == list(range(8))
    assert sum(len(l["envelope"]["peak"]) for l in rest_) == -(-737 // 160)
    at = 0
    for l in rest_:
        assert l["envelope"]["first"] == at and l["envelope"]["hop"] == 160
        at += len(l["envelope"]["level_dbfs"])
    # errors before the first byte map as on the other routes, and give the lock back
    r = c.post("/synthesize_stream_marks", json=dict(body, envelope_hz=0))
    assert r.status_code == 500 and "envelope_hz" in r.text
    assert c.post("/synthesize_stream_marks", json=dict(body, normalize=True)).status_code == 500
    again = c.post("/synthesize_stream", json=dict(body, marks=True))
    # /synthesize_stream is the same with and without the new route registered
    bare = rest.make_app(h)
    bare.router.routes[:] = [x for x in bare.router.routes if getattr(x, "path", "") != "/synthesize_stream_marks"]
    cb = TestClient(bare)
    assert cb.post("/synthesize_stream_marks", json=body).status_code == 404
    other = cb.post("/synthesize_stream", json=dict(body, marks=True))
    for a in (again, other):
        assert a.status_code == 200 and a.content == plain.content and a.headers["x-speech-marks"] == plain.headers["x-speech-marks"]
        assert a.headers["content-type"] == plain.headers["content-type"]


def test_holder_passes_levels_through(monkeypatch):
    """The real TTSModelHolder (fake sessions) in front of the real orchestrator: levels=True reaches the handle, the default does not name it."""
    from sbv2_api_amd import holder
    monkeypatch.setattr(model, "StreamHandle", FakeHandle)
    by_text = {"one": LINES[0], "two": LINES[2]}
    hd = holder.TTSModelHolder(b"bert", parse_text=lambda s: by_text[s], load_session=lambda data, is_bert: object(),
                               make_pipeline=lambda bert, vits: None)
    hd.load("m", json.dumps({"shape": [2, 4], "data": STYLES.tolist()}).encode(), b"vits")
    opts = orchestrator.SynthesizeOptions(envelope_hz=100)
    FakeHandle.seen.clear()
    plain = hd.easy_synthesize_stream("m", "one\n\ntwo", 1, 0, opts, noise_seed=3, split=True)
    assert "levels" not in FakeHandle.seen[-1][1] and "env_hop" not in FakeHandle.seen[-1][1]
    want = b"".join(plain)
    with_levels = hd.easy_synthesize_stream("m", "one\n\ntwo", 1, 0, opts, noise_seed=3, split=True, levels=True)
    assert FakeHandle.seen[-1][1]["levels"] is True and FakeHandle.seen[-1][1]["env_hop"] == 441
    assert b"".join(with_levels) == want
    d = with_levels.take_marks()
    assert len(d["tokens"]) == 8 and d["delivered"] == with_levels.total_samples and "level_dbfs" in with_levels.marks["tokens"][0]
    assert hd._find("m").streams == 0     # both streams gave the model back
