"""The formatting launches of csrc/pcm_format.hip (k_pcm_resample<0|1|2|3|4|5>, k_pcm_gain<ENC>) launch by launch through sbv2_debug_pcm_format
(csrc/test_hooks.cpp: PcmFormatter::run on a host table of pieces and signals, every piece between NaN words, the output between guard bands), against
a sparse float64 reference that uses the library's own f32 tap table (model.pcm_format_taps).

Reference, for output j of a signal (all index arithmetic in int64):
    i0 = j M + half, kmax = i0 // L, p = i0 - kmax L,   y = sum_{t < T} h[p + t L] x(kmax - t),   B = sum_t |h| |x|,
x(k) looked up in the signal's pieces [p0, p1) only, 0 elsewhere.

Tolerances (all derived, none measured; the worst error / tolerance ratio of each case is printed).  u = 2^-53.
- f64 (expose_y): |got - y| <= tol64 = 2 T u B.  The products h x are exact in f64 (24 x 24 bits); the kernel's fma chain of T terms errs by at most
  gamma_(T-1) B and so does the reference's sum; 2 (T - 1) u / (1 - T u) < 2 T u.  B = 0 gives tol64 = 0: exact zeros.
- f32: tol64 + 2^-24 |y| + 2^-150 (the cast of the kernel's sum: half an ulp in the normal range, half the smallest denormal below it; the cast's share
  of the kernel's own error, 2^-24 tol64, is inside the slack between 2 (T - 1) and 2 T).
- s16: equal to clip(rint(32767 y), -32767, 32767) wherever |frac(32767 y) - 0.5| > 32767 tol64; a sample inside that window is undecided.  The CPU part
  asserts on the reference alone that NO sample of any case is undecided, so the GPU part compares every sample.  mu-law / A-law: the code
  sbv2_g711_encode gives for that integer.
- normalised: pk = max |y| of the signal, known to tol_pk = the largest tol64 of the signal; the kernel forms y * fl(1 / pk), two roundings:
  |got - y / pk| <= tolN = (tol64 + |y| tol_pk / pk) / pk + 2^-51 |y| / pk, the f32 cast and the s16 window follow from tolN as above.  The sample at
  the peak must be exactly +-32767 (+-1.0f): pk * fl(1 / pk) is within one ulp of 1.  A silent signal has gain 1.
- layouts that must agree bit for bit (stream windows against the whole row, positions beyond 2^33 against the same piece near 0): array_equal on the
  f64 bits: every output is the same ordered sum of the same T products.

Two statements of the issue cannot hold as written and are tested as far as they can:
- "at every rate some output's span crosses at least four pieces": at 44100 the filter has one tap (T = 1), a span is one sample.  The condition is
  asserted at the six resampled rates, and T == 1 at 44100.
- "ties rounded away from zero" as a wrong reference: 32767 y = n + 1/2 with y a finite sum of products of binary fractions needs y itself to be an
  odd multiple of 1/2, so the only ties the quantiser can meet are +-16383.5 (y = +-0.5; +-1.5 and beyond are clipped), and there half-to-even and
  half-away both give +-16384.  test_wrong_quantisers shows that on the identity case, and shows that the neighbouring mistake, ties rounded up
  (floor(v + 0.5)), does fail it at -0.5.
f32 accumulation cannot differ at 44100 either (one product, exact); it is asserted at the six resampled rates.  The last tap dropped and f32
accumulation exceed the f64 and f32 tolerances at every rate they can, but err by less than an s16 step at some: the s16 check of the wrong references
is asserted for those that misplace samples.

On the MI355X every f64 output equalled the reference bit for bit (ratio 0.000 in all 24 cases) and the f32 casts reached 0.92 - 1.00 of their bound.
"""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from sbv2_api_amd import _lib, model
from test_pcm_format import ref_resample

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATES = (8000, 16000, 22050, 24000, 32000, 44100, 48000)
H_RATES = (8000, 22050, 48000)
U53 = 2.0 ** -53
LAWS = ("mulaw", "alaw")
U_AMPS = [1.0, 1e-6, 0.0, 1e-3, 1.0, 1.0, 30.0, 1.0]        # the normalised runs: signal 2 is all-zero
SPIKE = 12.0


@functools.lru_cache(None)
def geometry(rate):
    """(h zero-padded to T L as float64, L, M, half, T) of a rate, from the library's f32 prototype."""
    h, L, M = model.pcm_format_taps(rate)
    half, T = (len(h) - 1) // 2, -(-len(h) // L)
    hp = np.zeros(T * L)
    hp[:len(h)] = h
    hp.setflags(write=False)
    return hp, L, M, half, T


def ceil_div(a, b):
    return -(-a // b)


# ---- the sparse float64 reference (and its deliberately wrong variants) ------------------------------------------------------------------

def ref_signal(x, pieces, sig, rate, bug=None):
    """(y, B) of one signal (j0, j1, p0, p1).  bug: one of the wrong references of the CPU part."""
    hp, L, M, half, T = geometry(rate)
    j0, j1, p0, p1 = (int(v) for v in sig)
    j = np.arange(0, j1 - j0, dtype=np.int64) if bug == "j0_ignored" else np.arange(j0, j1, dtype=np.int64)
    if j.size == 0:
        return np.zeros(0), np.zeros(0)
    i0 = j * M + half
    kmax = i0 // L
    p = i0 - kmax * L
    if bug == "kmax_high":
        kmax = kmax + 1
    lo, hi = int(kmax.min()) - T + 1, int(kmax.max()) + 1
    dense = np.zeros(hi - lo)
    for q in (range(len(pieces)) if bug == "all_pieces" else range(p0, p1)):
        off, t0, n = (int(v) for v in pieces[q])
        if bug == "end_inclusive":
            n = min(n + 1, len(x) - off)
        a, b = max(t0, lo), min(t0 + n, hi)
        if a < b:
            dense[a - lo:b - lo] = x[off + a - t0:off + b - t0]
    y, B = np.zeros(j.size), np.zeros(j.size)
    y32 = np.zeros(j.size, np.float32)
    for t in range(T - 1 if bug == "last_tap" else T):
        hh, xv = hp[p + t * L], dense[kmax - t - lo]
        y += hh * xv
        B += np.abs(hh) * np.abs(xv)
        y32 = (y32.astype(np.float64) + hh * xv).astype(np.float32)
    return (y32.astype(np.float64) if bug == "f32_accumulation" else y), B


class Ref:
    """The reference of one case at one rate: y, B, tol64 over all outputs in delivery order, the signal of each output, and the normalised
    values v = y / pk with their bound tolN.  Computed once (reference()), shared, read-only."""

    def __init__(self, case, rate, bug=None, peak_of=None):
        T = geometry(rate)[4]
        ys, Bs = zip(*[ref_signal(case["x"], case["pieces"], s, rate, bug) for s in case["sigs"]])
        self.lens = [len(v) for v in ys]
        self.y, self.B = np.concatenate(ys), np.concatenate(Bs)
        self.tol64 = 2 * T * U53 * self.B
        self.tol32 = self.tol64 + 2.0 ** -24 * np.abs(self.y) + 2.0 ** -150
        self.sig = np.repeat(np.arange(len(ys)), self.lens)
        self.pk = np.array([np.abs(v).max() if v.size else 0.0 for v in ys])
        self.tol_pk = np.array([self.tol64[self.sig == s].max() if n else 0.0 for s, n in enumerate(self.lens)])
        pk_used = self.pk if peak_of is None else self.pk[peak_of]
        pk, tpk = pk_used[self.sig], self.tol_pk[self.sig]
        live = pk > 0
        d = np.where(live, pk, 1.0)
        self.v = self.y / d
        self.tolN = np.where(live, (self.tol64 + np.abs(self.y) * tpk / d) / d + 2.0 ** -51 * np.abs(self.y) / d, self.tol64)
        self.tolN32 = self.tolN + 2.0 ** -24 * np.abs(self.v) + 2.0 ** -150
        for a in vars(self).values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)

    def split(self, a):
        return np.split(a, np.cumsum(self.lens)[:-1])


def quantise(v, lo=-32767, ties="even"):
    a = 32767.0 * np.asarray(v, np.float64)
    r = {"even": np.rint, "away": lambda z: np.sign(z) * np.floor(np.abs(z) + 0.5), "up": lambda z: np.floor(z + 0.5)}[ties](a)
    return np.clip(r, lo, 32767).astype(np.int64)


def undecided(v, tol):
    a = 32767.0 * np.asarray(v, np.float64)
    return np.abs(a - np.floor(a) - 0.5) <= 32767.0 * np.asarray(tol)


# ---- the layouts -----------------------------------------------------------------------------------------------------------------------------

def packed_case(lens, rate, x):
    L, M = geometry(rate)[1:3]
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]])
    return {"x": x, "pieces": np.array([[o, 0, n] for o, n in zip(offs, lens)], np.int64),
            "sigs": np.array([[0, ceil_div(n * L, M), i, i + 1] for i, n in enumerate(lens)], np.int64)}


def case_U(rate, normalised=False):
    """Per utterance, packed: one piece per signal at t0 = 0.  Signal 3 has a positive spike on its first native sample, signal 5 a negative one on
    its last; the normalised data scales every signal by its own amplitude."""
    S = geometry(rate)[4]
    lens = [0, 1, 37, 700, 0, 1500, 2 * S + 3, 0]
    offs = np.concatenate([[0], np.cumsum(lens)])
    x = (0.5 * np.random.default_rng(1000 + rate).standard_normal(int(offs[-1]))).astype(np.float32)
    x[offs[3]] = SPIKE
    x[offs[6] - 1] = -SPIKE
    if normalised:
        for i, a in enumerate(U_AMPS):
            x[offs[i]:offs[i + 1]] *= np.float32(a)
    return packed_case(lens, rate, x)


J_LENS, J_LEAD = [1, 2, 1, 300, 5, 900, 64], 17


def case_J(rate, normalised=False):
    """Joined: one signal over seven pieces on a silent timeline."""
    _, L, M, _, S = geometry(rate)
    gaps = [0, 1, 3, S // 2, 0, 2 * S + 5]
    x = (0.5 * np.random.default_rng(2000 + rate).standard_normal(sum(J_LENS))).astype(np.float32)
    pieces, off, t = [], 0, J_LEAD
    for i, n in enumerate(J_LENS):
        pieces.append([off, t, n])
        off += n
        t += n + (gaps[i] if i < len(gaps) else 0)
    N = t + S + 9
    return {"x": x, "pieces": np.array(pieces, np.int64), "sigs": np.array([[0, ceil_div(N * L, M), 0, len(pieces)]], np.int64), "N": N}


W_ROW, W_PLACE, W_WIDE, W_STEP, W_HALO = 4000, 1234, 1152, 768, 192
W_NWIN = ceil_div(W_ROW, W_STEP)


def case_W(rate, normalised=False):
    """Stream windows: piece w = window w clipped to the row, signal w = the outputs of the window's middle samples, pieces [w, w + 1)."""
    L, M = geometry(rate)[1:3]
    x = (0.5 * np.random.default_rng(3000 + rate).standard_normal(W_ROW)).astype(np.float32)
    pieces, sigs = [], []
    for w in range(W_NWIN):
        m0 = W_PLACE + W_STEP * w
        ws = m0 - W_HALO
        lo, hi = max(W_PLACE, ws), min(W_PLACE + W_ROW, ws + W_WIDE)
        pieces.append([lo - W_PLACE, lo, hi - lo])
        sigs.append([ceil_div(m0 * L, M), ceil_div((m0 + W_STEP) * L, M), w, w + 1])
    return {"x": x, "pieces": np.array(pieces, np.int64), "sigs": np.array(sigs, np.int64)}


def case_W_whole(rate):
    c = case_W(rate)
    return {"x": c["x"], "pieces": np.array([[0, W_PLACE, W_ROW]], np.int64), "sigs": np.array([[c["sigs"][0, 0], c["sigs"][-1, 1], 0, 1]], np.int64)}


def case_H(rate, far):
    """One 500-sample piece at t0 = 5 (far = False) or M K + 5, K = 2^33 // M; the far signal starts three outputs before the first output whose span
    reaches the piece and both end three outputs after the last one."""
    _, L, M, half, T = geometry(rate)
    K = 2 ** 33 // M
    x = (0.5 * np.random.default_rng(4000 + rate).standard_normal(500)).astype(np.float32)
    ja = ceil_div(5 * L - half, M) - 3                  # kmax(j) >= 5  <=>  j M + half >= 5 L   (negative near 0: the near signal starts at 0)
    jb = ((504 + T) * L - half - 1) // M + 1 + 3        # kmax(j) - T + 1 <= 504  <=>  j M + half < (504 + T) L
    assert ((jb - 4) * M + half) // L - T + 1 <= 504 < ((jb - 3) * M + half) // L - T + 1
    if far:
        return {"x": x, "pieces": np.array([[0, M * K + 5, 500]], np.int64), "sigs": np.array([[L * K + ja, L * K + jb, 0, 1]], np.int64), "lead": -ja}
    return {"x": x, "pieces": np.array([[0, 5, 500]], np.int64), "sigs": np.array([[max(ja, 0), jb, 0, 1]], np.int64), "lead": 0}


def case_I():
    """Identity rate: signed zeros, ties, clipping values, denormals, a lead-in, a gap between two pieces and a tail."""
    d = np.float32(1e-40)
    a = np.array([-0.0, 0.0, 0.5, -0.5, 1.0, -1.0, 1.5, -1.5, d, -d, np.float32(1.4e-45), 0.25, -0.75, 16383.5 / 32768], np.float32)
    b = np.array([-0.0, 0.123, -0.0], np.float32)
    x = np.concatenate([a, b])
    N = 2 + len(a) + 3 + len(b) + 2
    want = np.zeros(N, np.float32)
    want[2:2 + len(a)] = a
    want[5 + len(a):5 + len(a) + len(b)] = b
    return {"x": x, "pieces": np.array([[0, 2, len(a)], [len(a), 5 + len(a), len(b)]], np.int64), "sigs": np.array([[0, N, 0, 2]], np.int64),
            "want": want}


CASES = {"U": case_U, "J": case_J, "W": case_W}


@functools.lru_cache(None)
def case(name, rate, normalised=False):
    c = CASES[name](rate, normalised)
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


@functools.lru_cache(None)
def reference(name, rate, normalised=False):
    return Ref(case(name, rate, normalised), rate)


def _ratio(err, tol):
    """max err / tol; an error where the tolerance is 0 counts as inf, a NaN stays a NaN (and fails every <=)."""
    err, tol = np.asarray(err, np.float64), np.asarray(tol, np.float64)
    if err.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(tol > 0, err / tol, np.where(err == 0, 0.0, np.where(np.isnan(err), np.nan, np.inf)))
    return float(np.nan if np.isnan(r).any() else r.max())


# ---- CPU part ------------------------------------------------------------------------------------------------------------------------------------

def test_hook_is_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "sbv2_hip.h")).read()
    assert re.search(r"\bint sbv2_debug_pcm_format\(", hdr)
    assert "sbv2_debug_pcm_format" in _lib.SYMBOLS and _lib.lib().sbv2_debug_pcm_format.restype is C.c_int
    assert len(_lib.SYMBOLS["sbv2_debug_pcm_format"][1]) == 11


@pytest.mark.parametrize("rate", RATES)
def test_reference_equals_the_dense_timeline_and_scipy(rate):
    import scipy.signal as S
    hp, L, M, half, T = geometry(rate)
    h = hp[:2 * half + 1]
    for name in ("U", "J", "W"):
        c, r = case(name, rate), reference(name, rate)
        ys, tols = r.split(r.y), r.split(r.tol64)
        if name == "U":
            dense = [(np.asarray(c["x"][o:o + n], np.float64), 0) for o, _, n in c["pieces"]]
        else:
            line = np.zeros(c["N"] if name == "J" else W_PLACE + W_STEP * W_NWIN)
            for o, t0, n in c["pieces"]:
                line[t0:t0 + n] = c["x"][o:o + n]
            dense = [(line, s[0]) for s in c["sigs"]]
        for (xd, j0), y, tol in zip(dense, ys, tols):
            if xd.size == 0:
                assert y.size == 0
                continue
            full = ref_resample(xd, h, L, M)
            assert j0 + y.size <= full.size
            assert np.all(np.abs(full[j0:j0 + y.size] - y) <= tol), (name, rate)
            sp = S.resample_poly(xd, L, M, window=h / L)
            assert sp.shape == full.shape
            assert np.abs(sp[j0:j0 + y.size] - y).max() <= 1e-12 * max(np.abs(full).max(), 1e-300), (name, rate)


@pytest.mark.parametrize("rate", RATES)
def test_layouts_meet_their_conditions(rate):
    _, L, M, half, T = geometry(rate)
    # U: three signals in one 64-output wave, a boundary strictly inside a wave, a signal over two 256-thread blocks
    r = reference("U", rate)
    assert r.lens[0] == r.lens[4] == r.lens[7] == 0 and all(r.lens[i] > 0 for i in (1, 2, 3, 5, 6))
    waves = [set(r.sig[o:o + 64]) for o in range(0, len(r.sig), 64)]
    assert max(len(w) for w in waves) >= 3
    bounds = np.cumsum(r.lens)[:-1]
    assert any(b % 64 and 0 < b < len(r.sig) for b in bounds)
    assert any(len(set(np.flatnonzero(r.sig == s) // 256)) >= 2 for s in range(8))
    assert any(len(w) == 1 for w in waves) or len(r.sig) < 64 * 3   # (and a wave of one signal: the reduce-first branch)
    # the peaks of the normalised data: first output, last output, a negative sample; the silent signal
    rn = reference("U", rate, True)
    ys = rn.split(rn.y)
    assert int(np.abs(ys[3]).argmax()) == 0 and ys[3][0] > 0
    assert int(np.abs(ys[5]).argmax()) == len(ys[5]) - 1 and ys[5][-1] < 0
    assert rn.pk[2] == 0 and rn.lens[2] > 0 and not np.any(rn.B[rn.sig == 2])
    assert rn.pk[6] > 30 * rn.pk[3] > 0 and 0 < rn.pk[1] < 1e-5
    # J: some output's span crosses four pieces (a one-tap filter cannot: the module docstring)
    c = case("J", rate)
    j = np.arange(c["sigs"][0, 1], dtype=np.int64)
    kmax = (j * M + half) // L
    crossed = sum(((kmax >= t0) & (kmax - T + 1 < t0 + n)).astype(int) for _, t0, n in c["pieces"])
    assert (crossed.max() >= 4) if rate != 44100 else (T == 1 and crossed.max() == 1)
    assert c["pieces"][0, 1] == J_LEAD and c["N"] - (c["pieces"][-1, 1] + c["pieces"][-1, 2]) == T + 9
    # W: the pieces of neighbouring signals overlap in time, every output's span lies inside its own window
    c = case("W", rate)
    assert len(c["sigs"]) == W_NWIN == 6
    for w in range(W_NWIN):
        j = np.arange(c["sigs"][w, 0], c["sigs"][w, 1], dtype=np.int64)
        kmax = (j * M + half) // L
        ws = W_PLACE + W_STEP * w - W_HALO
        assert kmax.max() < ws + W_WIDE and kmax.min() - T + 1 >= ws
        if w:
            assert c["pieces"][w - 1, 1] + c["pieces"][w - 1, 2] > c["pieces"][w, 1]
            assert c["sigs"][w, 0] == c["sigs"][w - 1, 1]
    assert W_HALO >= ceil_div(half, L) and (rate != 8000 or ceil_div(half, L) == 177)
    # H: positions beyond 2^31 (beyond 2^33), the far signal three outputs ahead of the first one the piece reaches
    if rate in H_RATES:
        f, n = case_H(rate, True), case_H(rate, False)
        assert f["pieces"][0, 1] > 2 ** 33 - M and f["sigs"][0, 0] * M + half > 2 ** 33 - 8 * M and n["sigs"][0, 0] == 0 and f["lead"] > 3
        rf = Ref(f, rate)
        assert not np.any(rf.B[:3]) and rf.B[3] > 0 and not np.any(rf.B[-3:]) and np.any(rf.B[-8:-3])


@pytest.mark.parametrize("rate", RATES)
def test_no_sample_is_undecided(rate):
    for name in ("U", "J", "W"):
        r = reference(name, rate)
        assert not undecided(r.y, r.tol64).any(), (name, rate)
        rn = reference(name, rate, True)
        assert not undecided(rn.v, rn.tolN).any(), (name, rate)
        # the peak samples quantise to exactly +-32767 in the reference as well
        for s, n in enumerate(rn.lens):
            if n and rn.pk[s] > 0:
                assert np.abs(quantise(rn.v[rn.sig == s])).max() == 32767


RESAMPLE_BUGS = ("last_tap", "kmax_high", "end_inclusive", "all_pieces", "f32_accumulation")


@pytest.mark.parametrize("rate", RATES)
def test_wrong_resamplers_exceed_the_tolerance(rate):
    """The last tap dropped, kmax one too high, a piece's end taken inclusive, all pieces searched instead of [p0, p1), f32 accumulation: each on
    layout U; j0 ignored: on layout W (U's signals start at j0 = 0; W's pieces hold the same row, so searching all of them changes nothing there).
    The inclusive end also on layout J, where pieces end inside the timeline: at 44100 U's outputs stop where its pieces stop, nothing can read past one.
    Each must exceed the f64 AND the (wider) f32 tolerance somewhere; those that misplace samples must also move an s16 sample (none is undecided)."""
    for name, bugs in (("U", RESAMPLE_BUGS), ("J", ("end_inclusive",)), ("W", ("j0_ignored",))):
        r, q = reference(name, rate), quantise(reference(name, rate).y)
        for bug in bugs:
            w = Ref(case(name, rate), rate, bug)
            err = np.abs(w.y - r.y)
            if rate == 44100 and (bug == "f32_accumulation" or (bug, name) == ("end_inclusive", "U")):
                assert not err.any()   # one exact product: nothing to accumulate; one tap: no output looks at the sample behind a piece
                continue
            assert _ratio(err, r.tol64) > 1 and _ratio(err, r.tol32) > 1, (name, bug, rate)
            if bug not in ("f32_accumulation", "last_tap"):   # (those two err by parts in 10^5 and less of the peak: below an s16 step at some rates)
                assert np.any(quantise(w.y) != q), (name, bug, rate)
            print(f"[wrong {bug} {name} {rate}] error / f64 tolerance = {_ratio(err, r.tol64):.3g}, / f32 tolerance = {_ratio(err, r.tol32):.3g}")


@pytest.mark.parametrize("rate", RATES)
def test_wrong_peak_exceeds_the_tolerance(rate):
    """Each signal scaled by the peak of the next non-silent signal."""
    r = reference("U", rate, True)
    loud = [s for s in range(8) if r.pk[s] > 0]
    other = np.arange(8)
    for a, b in zip(loud, loud[1:] + loud[:1]):
        other[a] = b
    w = Ref(case("U", rate, True), rate, peak_of=other)
    err = np.abs(w.v - r.v)
    assert _ratio(err, r.tolN32) > 1 and np.any(quantise(w.v) != quantise(r.v))
    for s in loud:
        assert _ratio(err[r.sig == s], r.tolN32[r.sig == s]) > 1, (rate, s)


def test_wrong_quantisers():
    """Clamp at -32768: layout U holds samples below -1.  Ties: see the module docstring; the identity case holds the only reachable tie."""
    for rate in RATES:
        r = reference("U", rate)
        assert r.y.min() < -1 - 1.0 / 32767
        assert np.any(quantise(r.y, lo=-32768) != quantise(r.y)), rate
    x = case_I()["want"].astype(np.float64)
    assert np.any(quantise(x, lo=-32768) != quantise(x))
    tie = np.abs(32767 * x - np.floor(32767 * x) - 0.5) == 0
    assert set(np.abs(x[tie])) == {0.5, 1.5}
    assert np.array_equal(quantise(x, ties="away"), quantise(x))              # half away from zero cannot be told from half to even here ...
    assert quantise(-0.5, ties="up") == -16383 != quantise(-0.5) == -16384   # ... ties rounded up can
    assert np.any(quantise(x, ties="up") != quantise(x))


# ---- the hook's argument checks: before any device call, so they run (and are tested) without a GPU as well ---------------------------------------

def _refusals():
    x = np.arange(10, dtype=np.float32)
    ok_p, ok_s = [[0, 0, 5], [5, 7, 5]], [[0, 4, 0, 2]]
    f = model.PcmFormat(16000, "s16")
    bad_enc = model.PcmFormat(16000, "s16")
    bad_enc.c.encoding = 2
    bad_rate = model.PcmFormat(11025, "s16")
    norm = model.PcmFormat(16000, "f32", True)
    for what, args, kw in (("sorted", (x, [[0, 7, 5], [5, 0, 5]], ok_s, f), {}),
                           ("overlap", (x, [[0, 0, 5], [5, 4, 5]], ok_s, f), {}),
                           ("no range", (x, ok_p, [[5, 3, 0, 2]], f), {}),
                           ("no range", (x, ok_p, [[-1, 3, 0, 2]], f), {}),
                           ("no range", (x, ok_p, [[0, 4, 1, 0]], f), {}),
                           ("no range", (x, ok_p, [[0, 4, 0, 3]], f), {}),
                           ("outside", (x, [[6, 0, 5]], [[0, 4, 0, 1]], f), {}),
                           ("outside", (x, [[-1, 0, 5]], [[0, 4, 0, 1]], f), {}),
                           ("sample rate", (x, ok_p, ok_s, bad_rate), {}),
                           ("encoding", (x, ok_p, ok_s, bad_enc), {}),
                           ("expose_y", (x, ok_p, ok_s, norm), {"expose_y": True})):
        with pytest.raises(model.Sbv2Error, match=what):   # (the wrapper raises another error if anything was written)
            model.debug_pcm_format(*args, **kw)


def test_bad_tables_are_refused_before_any_device_call():
    _refusals()


# ---- GPU part ------------------------------------------------------------------------------------------------------------------------------------

def _check_all_deliveries(name, rate):
    c, r = case(name, rate), reference(name, rate)
    table = (c["x"], c["pieces"], c["sigs"])
    worst = {}
    got = np.concatenate(model.debug_pcm_format(*table, model.PcmFormat(rate, "f32"), expose_y=True))
    assert got.dtype == np.float64 and got.shape == r.y.shape
    worst["f64"] = _ratio(np.abs(got - r.y), r.tol64)
    got = np.concatenate(model.debug_pcm_format(*table, model.PcmFormat(rate, "f32")))
    assert got.dtype == np.float32
    worst["f32"] = _ratio(np.abs(got.astype(np.float64) - r.y), r.tol32)
    q = quantise(r.y)
    decided = ~undecided(r.y, r.tol64)
    got = np.concatenate(model.debug_pcm_format(*table, model.PcmFormat(rate, "s16")))
    assert got.dtype == np.int16
    wrong = {"s16": int((got[decided] != q[decided]).sum())}
    for law in LAWS:
        got = np.concatenate(model.debug_pcm_format(*table, model.PcmFormat(rate, law)))
        wrong[law] = int((got[decided] != model.g711_encode(q.astype(np.int16), law)[decided]).sum())
    # peak-normalised
    c, r = case(name, rate, True), reference(name, rate, True)
    table = (c["x"], c["pieces"], c["sigs"])
    outs, pk = model.debug_pcm_format(*table, model.PcmFormat(rate, "f32", True), peaks=True)
    got = np.concatenate(outs)
    worst["peak"] = _ratio(np.abs(pk - r.pk), r.tol_pk)
    worst["f32 normalised"] = _ratio(np.abs(got.astype(np.float64) - r.v), r.tolN32)
    at_peak = np.abs(r.y) == r.pk[r.sig]
    live = r.pk[r.sig] > 0
    assert np.all(np.abs(got[at_peak & live]) == np.float32(1.0)) and np.array_equal(np.sign(got[at_peak & live]), np.sign(r.y[at_peak & live]))
    assert not np.any(got[~live])   # a silent signal: gain 1, zeros
    q = quantise(r.v)
    decided = ~undecided(r.v, r.tolN)
    outs, pk16 = model.debug_pcm_format(*table, model.PcmFormat(rate, "s16", True), peaks=True)
    got = np.concatenate(outs)
    assert np.array_equal(pk16, pk)
    wrong["s16 normalised"] = int((got[decided] != q[decided]).sum())
    assert np.all(np.abs(got[at_peak & live].astype(np.int64)) == 32767) and np.array_equal(np.sign(got[at_peak & live]), np.sign(r.y[at_peak & live]))
    print(f"[pcm_format {name} {rate}] worst error / tolerance: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()) +
          "; samples off: " + ", ".join(f"{k} {v}" for k, v in wrong.items()))
    assert all(v <= 1.0 for v in worst.values()), worst
    assert not any(wrong.values()), wrong
    assert decided.all()


@gpu
@pytest.mark.parametrize("rate", RATES)
def test_per_utterance_packed(rate):
    _check_all_deliveries("U", rate)


@gpu
@pytest.mark.parametrize("rate", RATES)
def test_joined_timeline(rate):
    _check_all_deliveries("J", rate)


@gpu
@pytest.mark.parametrize("rate", RATES)
def test_stream_windows(rate):
    _check_all_deliveries("W", rate)
    c = case("W", rate)
    fmt = model.PcmFormat(rate, "f32")
    parts = np.concatenate(model.debug_pcm_format(c["x"], c["pieces"], c["sigs"], fmt, expose_y=True))
    w = case_W_whole(rate)
    whole = model.debug_pcm_format(w["x"], w["pieces"], w["sigs"], fmt, expose_y=True)[0]
    assert np.array_equal(parts.view(np.uint64), whole.view(np.uint64))


@gpu
@pytest.mark.parametrize("rate", H_RATES)
def test_positions_beyond_2_33(rate):
    fmt = model.PcmFormat(rate, "f32")
    far, near = case_H(rate, True), case_H(rate, False)
    r = Ref(far, rate)
    yf = model.debug_pcm_format(far["x"], far["pieces"], far["sigs"], fmt, expose_y=True)[0]
    yn = model.debug_pcm_format(near["x"], near["pieces"], near["sigs"], fmt, expose_y=True)[0]
    ratio = _ratio(np.abs(yf - r.y), r.tol64)
    print(f"[pcm_format H {rate}] worst error / tolerance: f64 {ratio:.3f}; outputs compared bit for bit: {yn.size}")
    assert ratio <= 1.0
    assert yn.size > 500 * geometry(rate)[1] // geometry(rate)[2] and yf.size == yn.size + far["lead"]
    assert np.array_equal(yf[far["lead"]:].view(np.uint64), yn.view(np.uint64))
    q = model.debug_pcm_format(far["x"], far["pieces"], far["sigs"], model.PcmFormat(rate, "s16"))[0]
    decided = ~undecided(r.y, r.tol64)
    assert np.array_equal(q[decided], quantise(r.y)[decided]) and decided.mean() > 0.999


@gpu
def test_identity_rate_returns_the_input_bits():
    c = case_I()
    table = (c["x"], c["pieces"], c["sigs"])
    want = c["want"]
    got = model.debug_pcm_format(*table, model.PcmFormat(44100, "f32"))[0]
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))   # -0.0 stays -0.0, the gap is +0.0, denormals survive
    got = model.debug_pcm_format(*table, model.PcmFormat(44100, "f32"), expose_y=True)[0]
    assert np.array_equal(got.view(np.uint64), want.astype(np.float64).view(np.uint64))
    q = quantise(want)
    assert q[want == 0.5] == 16384 and q[want == -0.5] == -16384 and q[want == 1.5] == 32767 and q[want == -1.5] == -32767
    got = model.debug_pcm_format(*table, model.PcmFormat(44100, "s16"))[0]
    assert np.array_equal(got, q)
    for law in LAWS:
        got = model.debug_pcm_format(*table, model.PcmFormat(44100, law))[0]
        assert np.array_equal(got, model.g711_encode(q.astype(np.int16), law))


@gpu
def test_bad_tables_are_refused_with_a_device_present():
    _refusals()
    # and a good call right after a refused one is served
    out = model.debug_pcm_format(np.ones(4, np.float32), [[0, 0, 4]], [[0, 4, 0, 1]], model.PcmFormat(44100, "s16"))[0]
    assert list(out) == [32767] * 4
