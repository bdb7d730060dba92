"""The launches of csrc/loudness.hip (k_kw_zero, k_kw_carry, k_kw_rerun, k_true_peak, k_gate) and of csrc/limiter.hip's fixed-gain path
(k_lim_interp, k_lim_curve) launch by launch, through sbv2_debug_loudness_parts / sbv2_debug_limiter_parts (csrc/test_hooks.cpp:
LoudnessMeter::measure / Limiter::run_fixed as they are, the packed input between NaN words, every returned device array pre-filled with the
byte 0x5A), against numpy references.  u = 2^-53.

References (numpy only, computed once per module, read-only):
- K-weighting: the cascade run sequentially in np.longdouble (the module fails where longdouble is not the 64-bit-mantissa format), with the
  library's coefficients (sbv2_loudness_kweight): per segment the true start state st, the zero-start end state e and part = sum w^2 from the
  true start: the kernel's recurrence (transposed direct form II) written out, the signals of a case side by side and one loop over
  time for the start states, the segments side by side for e and part.
- gate: quarters, blocks and both gates restated in longdouble, evaluated on the `part` array the HOOK returns, so none of the filter's error
  is allowed twice.  L must agree within tol_L = (10 / ln 10) 2 (4 qs + ceil(nb / 256) + 16) u + 8 u max(1, |L|): every sum is over
  non-negative terms (qs segments a quarter, 4 quarters, a lane's ceil(nb / 256) blocks, the 8 levels of the tree, two divisions), so its
  relative error is at most (number of additions) u, once for the kernel and once for the reference's rounding to f64; log10 and the final
  sum cost a few ulp of L.  The CPU part asserts on the longdouble partials that no block of any case lies within 1e-6 dB of either gate.
  TP must be 20 log10 of the largest returned bmax / peak of the signal within 8 u max(1, |TP|).
- interpolator: z_p[o] = sum_d h[p][d] y[o + 12 - d] in float64 with the taps the hook returns (y = 0 outside the signal), tolerance
  2 * 24 * u * sum |h| |y| per phase; t[o] = max_p |z_p| and v[o] = max(|y[o]|, t[o]) carry the largest of their phases' tolerances, a maximum
  over samples the largest of its samples'.  bmax[b] of a workgroup inside one signal; exactly 0 for one that straddles signals; peak[s] over
  the straddling workgroups only, exactly 0 where there is none.
- curve: e, r, m, s, x of the header's convention from the reference's own t, tolerances propagated through the 1-Lipschitz steps:
  tau_r = r (delta_e / e + 3 u) where r < 1, else 0; tau_m = the largest tau_r of the window; tau_s = the largest tau_m in reach + 2 K u;
  |dx| <= |y| g0 (tau_s + 4 u); smin[tile] within the tile's largest tau_s.  A tile with no r < 1 within reach must give
  x = y * g0 * min(hsum, 1) bit for bit (hsum = the sequential float64 sum of the returned taps) and smin = min(hsum, 1).  The level is
  +20 dB, so that g0 = 10 exactly on both sides.  The CPU part asserts that no sample's c / (g0 e) lies within its tolerance of 1.
  A "loud sample" of the issue is a spike of 0.2 in noise of 0.002: r < 1 exactly at the spike and its two neighbours (asserted), and the
  tile-edge cases place that set's last / first position where the issue places the loud sample.

The one measured tolerance (e, st, part): the componentwise |A^m| majorant of the scan diverges, so the scan's error is measured on the CPU on
a float64 numpy mirror (k_kw_zero's runs by the same recurrence in float64, 256 lanes, c = ceil(nseg / 256), A^m by repeated products, P[d] by squaring,
unfused), per signal: err = max |mirror - longdouble| over the signal's segments (and components).  tol = max(8 err, 64 u max |state|) for
e and for st, each with its own err and its own largest component; tol_k = max(8 err_part, 4 m u part_k) for part.  The error is taken per
signal, not per segment: a segment's own error is a sum of signed terms and can vanish by chance.  The K-weighting cases of a rate hold
about 1 M samples; the gate's block counts (255, 256, 257, 513 blocks of 800 samples) add another 1 M at 8 kHz, run in a pass of their own.

Measured.  The mirror's errors on the CPU, worst signal per rate, as err / (u x the signal's largest component) for e, st and
err / (u x the largest part) for part (test_kweighting_cases_cover_the_edges prints every signal's):
    8000: e 3.2e3, st 3.2e3, part 8.0e2;   44100: e 9.1e4, st 7.9e5, part 3.1e6;   48000: e 9.4e4, st 3.0e5, part 9.1e5
(e's worst is the impulse case, whose zero-start states are tiny; on noise e stays below 1.2e4).  On the MI355X, worst error / tolerance
per family over all cases (the GPU tests print every case's: "[kw ...]", "[tp ...]", "[curve ...]"):
    e 0.20, st 0.34, part 0.23 (the kernel's error is 0.74 - 2.7 times the mirror's, against the 8 allowed);  L 0.18, TP 0.29;
    t 0.068, bmax and peak 0 (bit-equal);  x 0.0095, smin 0.0011, 16 of the 36 tiles of every curve case bit-exact idle.
No sentinel was left, no NaN appeared, no pad word changed.

One wrong reference of the issue cannot exceed the tolerance: the final min(s, r[n]) only takes rounding off (s <= r[n] holds exactly in
exact arithmetic), so leaving it out moves a sample by a few ulp, inside tau_s >= 2 K u.  test_wrong_curves states the samples where the
guard bites and asserts that it moves them, by less than the tolerance."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from sbv2_api_amd import _lib, model

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sbv2-api_amd", "csrc")
HOOKS = ("sbv2_debug_loudness_parts", "sbv2_debug_limiter_parts")
LD = np.longdouble
U = 2.0 ** -53
# restated from the sources (test_mirrors_match_the_sources)
SEG_LEN = {8000: 200, 16000: 200, 32000: 200, 22050: 245, 44100: 245, 24000: 240, 48000: 240}
SCAN_LANES, TP_WG, TP_BACK, TP_TAPS, TILE, MAX_K = 256, 256, 12, 24, 1024, 480
KW_RATES = (8000, 44100, 48000)
TP_RATES = (8000, 48000)
CURVE_RATES = (8000, 16000, 22050, 44100, 48000)      # K = 80, 160, 220, 441, 480
LEVEL_DB, CEILING_DB = 20.0, -1.0
G0, CEIL = 10.0, 10 ** (CEILING_DB / 20)
QUIET, LOUD = 0.002, 0.2


def ceil_div(a, b):
    return -(-a // b)


def _freeze(obj):
    for a in (obj.values() if isinstance(obj, dict) else obj):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
        elif isinstance(a, (dict, list, tuple)):
            _freeze(a)
    return obj


def _ratio(err, tol):
    """max err / tol; an error where the tolerance is 0 counts as inf, a NaN stays a NaN (and fails every <=)."""
    err, tol = np.asarray(err, np.float64), np.asarray(tol, np.float64)
    if err.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(tol > 0, err / tol, np.where(err == 0, 0.0, np.where(np.isnan(err), np.nan, np.inf)))
    return float(np.nan if np.isnan(r).any() else r.max())


def _ld_ok():
    assert np.finfo(LD).eps <= 2.0 ** -63, "np.longdouble is no wider than float64 here: the K-weighting reference needs the 64-bit mantissa"


# ---- K-weighting: the longdouble reference and the float64 mirror of the scan -------------------------------------------------------------

def _kw_step(c, s, x):
    """One sample through the cascade in the kernel's order of operations (unfused): (w, the new states)."""
    u = c[0] * x + s[0]
    s0 = c[1] * x + (s[1] - c[3] * u)
    s1 = c[2] * x - c[4] * u
    w = c[5] * u + s[2]
    return w, [s0, s1, c[6] * u + (s[3] - c[8] * w), c[7] * u - c[9] * w]


def _cascade(c, x, z):
    """x [rows, len] through the cascade from the states z [rows, 4] -> (sum w^2 in sample order, end states), in x's dtype."""
    s, acc = [z[:, i].copy() for i in range(4)], np.zeros(x.shape[0], x.dtype)
    for i in range(x.shape[1]):
        w, s = _kw_step(c, s, x[:, i])
        acc = acc + w * w
    return acc, np.stack(s, axis=1)


def kw_runs(y, c, m, st=None):
    """Every segment of y on its own, from st[k] (zero when None): (end states [nseg, 4], sum w^2 [nseg]) in y's dtype."""
    nseg, nfull = ceil_div(y.size, m), y.size // m
    end, part = np.zeros((nseg, 4), y.dtype), np.zeros(nseg, y.dtype)
    for rows, x in ((slice(0, nfull), y[:nfull * m].reshape(nfull, m)), (slice(nfull, nseg), y[nfull * m:].reshape(1, -1))):
        if x.size:
            part[rows], end[rows] = _cascade(c.astype(y.dtype), np.ascontiguousarray(x.T).T, np.zeros((x.shape[0], 4), y.dtype) if st is None else st[rows])
    return end, part


def kw_sequential(sigs, c, m):
    """The true start state of every segment of every signal: the signals side by side, one loop over time, in c's dtype."""
    longest = max([y.size for y in sigs] + [0])
    X = np.zeros((longest, len(sigs)), c.dtype)
    for i, y in enumerate(sigs):
        X[:y.size, i] = y
    s, at = [np.zeros(len(sigs), c.dtype) for _ in range(4)], np.zeros((ceil_div(longest, m), len(sigs), 4), c.dtype)
    for t in range(longest):
        if t % m == 0:
            at[t // m] = np.stack(s, axis=1)
        _, s = _kw_step(c, s, X[t])
    return [at[:ceil_div(y.size, m), i] for i, y in enumerate(sigs)]


def transition(c):
    a1, a2, h0, h1, h2, d1, d2 = c[3], c[4], c[5], c[6], c[7], c[8], c[9]
    return np.array([[-a1, 1, 0, 0], [-a2, 0, 0, 0], [h1 - d1 * h0, 0, -d1, 1], [h2 - d2 * h0, 0, -d2, 0]], c.dtype)


def _mm(X, Y):
    R = np.zeros((4, 4))
    for k in range(4):
        R = R + X[:, k:k + 1] * Y[k:k + 1, :]
    return R


def _mv(M, v, r0):
    """rows of r0 + M v, the products added in column order."""
    a = r0.copy()
    for j in range(4):
        a = a + v[:, j:j + 1] * M[None, :, j]
    return a


@functools.lru_cache(None)
def seg_matrix(rate):
    """A^m in float64 as LoudnessMeter::tables builds it: m - 1 products A1 (A1 ...)."""
    A1 = transition(model.loudness_kweight(rate))
    R = A1.copy()
    for _ in range(1, SEG_LEN[rate]):
        R = _mm(A1, R)
    R.setflags(write=False)
    return R


def scan_mirror(e, Am, bug=None):
    """k_kw_carry in float64 numpy: the start state of every segment from the zero-start end states e [nseg, 4]."""
    nseg = e.shape[0]
    c, t = ceil_div(nseg, SCAN_LANES), np.arange(SCAN_LANES)
    lo, hi = np.minimum(nseg, t * c), np.minimum(nseg, (t + 1) * c)
    if bug == "partial_chunk":   # balanced chunks (some of c - 1 segments before others of c), every chunk map still (A^m)^c
        size = nseg // SCAN_LANES + (t < nseg % SCAN_LANES)
        hi = np.cumsum(size)
        lo = hi - size
    r, b, p = np.eye(4), Am.copy(), c
    while p:
        if p & 1:
            r = _mm(r, b)
        if p > 1:
            b = _mm(b, b)
        p >>= 1
    P = [r]
    for _ in range(1, 8):
        P.append(_mm(P[-1], P[-1]))
    Q = np.zeros((SCAN_LANES, 4))
    for j in range(int((hi - lo).max())):
        live = lo + j < hi
        Q[live] = _mv(Am, Q[live], e[(lo + j)[live]])
    for d in range(8):
        sh = 1 << d
        Qn = Q.copy()
        Qn[sh:] = _mv(P[d], Q[:-sh], Q[sh:])
        Q = Qn
    s = np.zeros((SCAN_LANES, 4))
    if bug != "zero_chunk_start":
        s[1:] = Q[:-1]
    st = np.zeros((nseg, 4))
    for j in range(int((hi - lo).max())):
        live = lo + j < hi
        k = (lo + j)[live]
        st[k] = s[live]
        s[live] = _mv(Am, s[live], e[k])
    return st


def kw_signal(y, rate, st):
    """Reference (from the true start states st), mirror and tolerances of one signal."""
    m, c = SEG_LEN[rate], model.loudness_kweight(rate)
    yl, cl = y.astype(LD), c.astype(LD)
    e, _ = kw_runs(yl, cl, m)
    _, part = kw_runs(yl, cl, m, st)
    em, _ = kw_runs(y, c, m)
    stm = scan_mirror(em, seg_matrix(rate)) if y.size else np.zeros((0, 4))
    _, partm = kw_runs(y, c, m, stm)
    top = lambda a: float(np.abs(a).max()) if a.size else 0.0
    r = {"n": y.size, "st": st, "e": e, "part": part, "st_m": stm, "e_m": em, "part_m": partm,
         "err_e": top(em - e), "err_st": top(stm - st), "err_part": top(partm - part), "top_e": top(e), "top_st": top(st)}
    r["tol_e"] = max(8 * r["err_e"], 64 * U * r["top_e"])
    r["tol_st"] = max(8 * r["err_st"], 64 * U * r["top_st"])
    r["tol_part"] = np.maximum(8 * r["err_part"], 4 * m * U * part.astype(np.float64))
    return r


def _noise(seed, n, amp=0.25, dc=0.0):
    return amp * np.random.default_rng(seed).standard_normal(n) + dc


def kw_cases(rate):
    """name -> list of signals (one launch each)."""
    m, S = SEG_LEN[rate], rate // 10
    counts_last = ((1, m), (2, 1), (255, 4), (256, m), (257, m - 1), (511, 1), (512, m), (513, 4))
    A = [_noise(rate + i, (k - 1) * m + last) for i, (k, last) in enumerate(counts_last)]
    B = [_noise(rate + 100 + i, n, 0.25, 0.9) for i, n in enumerate((256 * m + m - 1, 0, 1, 4 * S - 1, 4 * S, 4 * S + 1, 512 * m + 4))]
    sine = lambda n: 0.5 * np.sin(2 * np.pi * 30.0 * np.arange(n) / rate)
    last, first = np.zeros(3 * m), np.zeros(3 * m)
    last[m - 1] = 1.0    # the unit impulse as the last sample of segment 0 ...
    first[m] = 1.0       # ... and as the first of segment 1
    cases = {"A": A, "B": B, "C": [sine(256 * m + m - 1), last, first, sine(512 * m)]}
    if rate == 8000:     # the gate's cases: amplitude-stepped noise, block counts 255, 256, 257, 513 (half a quarter left over) and the single-block form
        G = []
        for i, nb in enumerate((255, 256, 257, 513)):
            n = (nb + 3) * S + S // 2
            amp = np.array([0.1, 0.1 * 10 ** (-14.3 / 20), 1e-4, 1e-4])[(np.arange(n) // (12 * S) + i) % 4]   # the middle level: between the two gates of test_wrong_gates
            G.append(amp * np.random.default_rng(900 + i).standard_normal(n))
        G += [_noise(950, 1), _noise(951, 4 * S - 1), np.zeros(0), 1e-5 * np.random.default_rng(952).standard_normal(5 * S)]
        cases["G"] = G
    return cases


@functools.lru_cache(None)
def kw_case(rate, name):
    return _freeze(kw_cases(rate)[name])


@functools.lru_cache(None)
def kw_true_starts(rate, group):
    """name -> the longdouble start states of its signals: the signals of a group of cases in one pass."""
    _ld_ok()
    st = kw_sequential([y for k in group for y in kw_case(rate, k)], model.loudness_kweight(rate).astype(LD), SEG_LEN[rate])
    out, i = {}, 0
    for k in group:
        out[k] = st[i:i + len(kw_case(rate, k))]
        i += len(out[k])
    return out


@functools.lru_cache(None)
def kw_reference(rate, name):
    starts = kw_true_starts(rate, "G" if name == "G" else "ABC")[name]
    return _freeze([kw_signal(y, rate, st) for y, st in zip(kw_case(rate, name), starts)])


def kw_names(rate):
    return ("A", "B", "C", "G") if rate == 8000 else ("A", "B", "C")


# ---- gate ---------------------------------------------------------------------------------------------------------------------------------

def gate_ref(part, n, m, S, bug=None):
    """(L, margin): the convention on the segment partials of one signal in longdouble; margin = the smallest distance in dB of a block from a
    gate it is compared with."""
    part = np.asarray(part).astype(LD)
    lufs = lambda z: LD(-0.691) + 10 * np.log10(z)
    above = (lambda a, b: a >= b) if bug == "ge" else (lambda a, b: a > b)
    with np.errstate(divide="ignore", invalid="ignore"):
        if n == 0:
            return -np.inf, np.inf
        if n < 4 * S:
            l = lufs(part.sum() / n)
            return (float(l) if above(l, -70) else -np.inf), float(abs(l + 70))
        qs, nq = S // m, n // S
        q = part[:nq * qs].reshape(nq, qs).sum(axis=1)
        z = (q[:-3] + q[1:-2] + q[2:-1] + q[3:]) / (4 * S)
        l = lufs(z)
        keep = above(l, -70)
        margin = float(np.abs(l + 70).min())
        if not keep.any():
            return -np.inf, margin
        gate = lufs(z.mean() if bug == "all_blocks" else z[keep].mean()) - 10
        margin = min(margin, float(np.abs(l[keep] - gate).min()))
        keep &= above(l, gate)
        return float(lufs(z[keep].mean())), margin


def gate_tol(L, n, m, S):
    if not np.isfinite(L):
        return 0.0
    adds = ceil_div(n, m) + 4 if n < 4 * S else 4 * (S // m) + ceil_div(n // S - 3, 256) + 16
    return 10 / np.log(10) * 2 * adds * U + 8 * U * max(1.0, abs(L))


# ---- interpolator -------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(None)
def numpy_taps():
    """loudness_true_peak_taps restated: h[p - 1][d] = h4(p + 4 (d - 12)), every phase of h4 scaled to sum to 1."""
    n = np.arange(-48, 49)
    h4 = np.sinc(n / 4) * np.i0(8.6 * np.sqrt(1 - (n / 48.0) ** 2)) / np.i0(8.6)
    h = np.array([[h4[p + 4 * (d - TP_BACK) + 48] / h4[n % 4 == p].sum() for d in range(TP_TAPS)] for p in (1, 2, 3)])
    h.setflags(write=False)
    return h


def interp_ref(sigs, taps, bug=None):
    """Packed (t, tol, v): per sample the largest interpolated magnitude, its tolerance, and max(|y|, t)."""
    x = np.concatenate(sigs) if sigs else np.zeros(0)
    packed = np.concatenate([np.zeros(TP_BACK - 1), x, np.zeros(TP_BACK)])
    ts, tols, vs, off = [], [], [], 0
    for y in sigs:
        n = y.size
        pad = packed[off:off + n + 2 * TP_BACK - 1] if bug == "uncut" else np.concatenate([np.zeros(TP_BACK - 1), y, np.zeros(TP_BACK)])
        z, B = np.zeros((3, n)), np.zeros((3, n))
        for d in range(TP_TAPS):
            xs = pad[2 * TP_BACK - 1 - d:2 * TP_BACK - 1 - d + n]      # y[o + 12 - d]
            hd = (taps[:, d + 1] if d + 1 < TP_TAPS else np.zeros(3)) if bug == "shift" else taps[:, d]
            z += hd[:, None] * xs
            B += np.abs(hd)[:, None] * np.abs(xs)
        t = np.abs(z).max(axis=0)
        ts.append(t)
        tols.append((2 * TP_TAPS * U * B).max(axis=0))
        vs.append(t if bug == "no_y" else np.maximum(np.abs(y), t))
        off += n
    cat = lambda a: np.concatenate(a) if a else np.zeros(0)
    return cat(ts), cat(tols), cat(vs)


def tp_layout(lens):
    """(signal of every sample, straddling flag of every workgroup)."""
    sig_of = np.repeat(np.arange(len(lens)), lens)
    total = sig_of.size
    b0 = np.arange(ceil_div(total, TP_WG)) * TP_WG
    return sig_of, sig_of[b0] != sig_of[np.minimum(b0 + TP_WG - 1, total - 1)]


def peak_ref(lens, v, tol):
    """(bmax, its tolerance, peak, its tolerance) from the per-sample maxima."""
    sig_of, straddle = tp_layout(lens)
    nblk, nsig = straddle.size, len(lens)
    bmax, tb, peak, tpk = np.zeros(nblk), np.zeros(nblk), np.zeros(nsig), np.zeros(nsig)
    for b in range(nblk):
        sl = slice(b * TP_WG, (b + 1) * TP_WG)
        if not straddle[b]:
            bmax[b], tb[b] = v[sl].max(), tol[sl].max()
        else:
            for s in np.unique(sig_of[sl]):
                pick = sig_of[sl] == s
                peak[s], tpk[s] = max(peak[s], v[sl][pick].max()), max(tpk[s], tol[sl][pick].max())
    return bmax, tb, peak, tpk


# signal lengths of the true-peak case: edges at workgroup offsets 0, 1, 11, 12, 13, 243, 244, 245, 255; lengths 1, 23, 24, 25; four signals
# in wave 0 of workgroup 3; workgroup 4 = four signals of 64 (one per wave); an empty signal; a partial last workgroup inside one signal
TP_LENS = (513, 266, 1, 1, 230, 1, 1, 10, 1, 64, 64, 64, 64, 23, 24, 25, 0, 1061, 300)
TP_AMP = (0.1, 1e-3, 0.3, 0.3, 1e-3, 0.3, 0.3, 0.1, 0.3, 0.1, 0.2, 0.1, 0.2, 0.1, 0.1, 1e-3, 0.0, 0.1, 0.1)
TP_SPIKES = ((0, 5, 1.5), (0, 512, 1.0), (17, 0, 1.0), (17, 1792 + 100 - 1352, 2.0), (18, 50, -2.0))   # (signal, position, value)


@functools.lru_cache(None)
def tp_case():
    rng = np.random.default_rng(77)
    sigs = [a * rng.standard_normal(n) for n, a in zip(TP_LENS, TP_AMP)]
    for s, p, val in TP_SPIKES:
        sigs[s][p] = val
    return _freeze(sigs)


@functools.lru_cache(None)
def tp_reference(taps_bytes):
    taps = np.frombuffer(taps_bytes, np.float64).reshape(3, TP_TAPS)
    t, tol, v = interp_ref(tp_case(), taps)
    return _freeze({"t": t, "tol": tol, "v": v, "peaks": peak_ref(TP_LENS, v, tol)})


# ---- curve --------------------------------------------------------------------------------------------------------------------------------

def numpy_hann(K):
    v = np.sin(np.pi * (np.arange(K) + 0.5) / K) ** 2
    s = 0.0
    for a in v:
        s += a
    return v / s


def seq_sum(h):
    s = 0.0
    for a in h:
        s += a
    return s


def _windows(a, W, fill, op):
    """op over a[n .. n + W - 1], a continued with `fill`."""
    return op(np.lib.stride_tricks.sliding_window_view(np.concatenate([a, np.full(W - 1, fill)]), W), axis=1)


def _curve_from_r(r, tau_r, K, h, bug=None):
    """(m, s_sum, tau_s) of one signal's r."""
    n, W = r.size, K - 1 if bug == "short_window" else K
    m = _windows(r, W, 1.0, np.min)
    tau_m = _windows(tau_r, W, 0.0, np.max)
    mp = np.concatenate([np.full(K - 1, 1.0 if bug == "m_one" else m[0]), m])   # m[j] = mp[j + K - 1]
    s = np.zeros(n)
    for k in range(K):
        s = s + h[k] * mp[K - 1 - k:K - 1 - k + n]
    tp = np.concatenate([np.full(K - 1, tau_m[0]), tau_m])
    tau_s = np.lib.stride_tricks.sliding_window_view(tp, K).max(axis=1) + 2 * K * U
    return m, s, tau_s


def curve_ref(sigs, taps, K, h, bug=None):
    """Per signal: r, tau_r, m, s (guarded), s_sum, tau_s, x, tol_x, the undecided flag of every sample and the idle flag of every tile."""
    t_all, tol_all, _ = interp_ref(sigs, taps)
    out, off = [], 0
    for y in sigs:
        n = y.size
        t, tol_t = t_all[off:off + n], tol_all[off:off + n]
        off += n
        e = np.maximum(np.maximum(np.concatenate([[0.0], t[:-1]]), np.abs(y)), t)
        de = np.maximum(np.concatenate([[0.0], tol_t[:-1]]), tol_t)
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(e > 0, CEIL / (G0 * e), np.inf)
            rel = np.where(e > 0, de / e + 3 * U, 0.0)
        r = np.minimum(1.0, q)
        out.append({"y": y, "r": r, "tau_r": np.where(r < 1, r * rel, 0.0), "undecided": np.isfinite(q) & (np.abs(q - 1) <= q * rel)})
    if bug == "cross_edge":     # the sliding minimum and the Hann sum run over the packed r as if it were one signal
        lens = [d["r"].size for d in out]
        m, s, tau_s = _curve_from_r(np.concatenate([d["r"] for d in out]), np.concatenate([d["tau_r"] for d in out]), K, h)
        cuts = np.cumsum(lens)[:-1]
        parts = zip(np.split(m, cuts), np.split(s, cuts), np.split(tau_s, cuts))
    else:
        parts = []
        for d in out:
            n = d["r"].size
            if n == 0:
                parts.append((np.zeros(0), np.zeros(0), np.zeros(0)))
            elif bug == "halo_short":    # every tile sees r one sample less far on either side
                m, s, tau_s = np.zeros(n), np.zeros(n), np.zeros(n)
                for n0 in range(0, n, TILE):
                    pos = np.arange(n)
                    seen = (pos >= n0 - (K - 2)) & (pos <= n0 + TILE + K - 3)
                    mm, ss, tt = _curve_from_r(np.where(seen, d["r"], 1.0), d["tau_r"], K, h)
                    m[n0:n0 + TILE], s[n0:n0 + TILE], tau_s[n0:n0 + TILE] = mm[n0:n0 + TILE], ss[n0:n0 + TILE], tt[n0:n0 + TILE]
                parts.append((m, s, tau_s))
            else:
                parts.append(_curve_from_r(d["r"], d["tau_r"], K, h, bug))
    hs = min(seq_sum(h), 1.0)
    for d, (m, s_sum, tau_s) in zip(out, parts):
        y, n = d["y"], d["y"].size
        s = s_sum if bug == "no_min" else np.minimum(s_sum, d["r"])
        d.update(m=m, s_sum=s_sum, s=s, tau_s=tau_s, x=np.clip(y * G0 * s, -CEIL, CEIL), tol_x=np.abs(y) * G0 * (tau_s + 4 * U))
        pos = np.arange(n)
        d["idle"] = np.array([not np.any(d["r"][(pos >= n0 - (K - 1)) & (pos <= n0 + TILE + K - 2)] < 1) for n0 in range(0, n, TILE)], bool)
        d["x_idle"] = np.clip(y * G0 * hs, -CEIL, CEIL)
    return out


LONG = 3 * TILE + 5
N0 = TILE     # the tile the edge cases look at: samples [1024, 2048) of a signal of LONG


def curve_layout(K):
    """[(length, spike positions)]: the packed signals of the curve case at window K; the names of the special ones -> their index."""
    lay = [(1, [0]), (K - 1, [0]), (K, [K - 1]), (K + 1, [K]), (1023, [0]), (1024, [1023]), (1025, [1024]), (LONG, [1023]), (LONG, [1024]), (0, [])]
    names = {}
    # r < 1 at the spike p and at p - 1, p + 1: the set's last position at N0 - (K - 1) (reaches s[N0] through h[K - 1] alone) or N0 - K (not at
    # all), its first at N0 + 1024 + K - 2 (reaches s[N0 + 1023] through h[0] alone) or one further (not at all)
    for name, p in (("left_bite", N0 - (K - 1) - 1), ("left_idle", N0 - K - 1), ("right_bite", N0 + TILE + K - 2 + 1), ("right_idle", N0 + TILE + K - 1 + 1)):
        names[name] = len(lay)
        lay.append((LONG, [p]))
    names["edge_pair"] = len(lay)
    lay += [(300, [299]), (300, []), (300, []), (300, [0])]
    return lay, names


@functools.lru_cache(None)
def curve_case(rate):
    rng = np.random.default_rng(5000 + rate)
    sigs = []
    for n, spikes in curve_layout(rate // 100)[0]:
        y = QUIET * rng.standard_normal(n)
        for p in spikes:
            y[p] = LOUD if p % 2 else -LOUD
        sigs.append(y)
    return _freeze(sigs)


@functools.lru_cache(None)
def curve_reference(rate, taps_bytes, h_bytes):
    taps, h = np.frombuffer(taps_bytes, np.float64).reshape(3, TP_TAPS), np.frombuffer(h_bytes, np.float64)
    return _freeze(curve_ref(curve_case(rate), taps, rate // 100, h))


def cpu_curve_reference(rate):
    return curve_reference(rate, numpy_taps().tobytes(), numpy_hann(rate // 100).tobytes())


# ---- CPU part -----------------------------------------------------------------------------------------------------------------------------

def test_hooks_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "sbv2_hip.h")).read()
    l = _lib.lib()
    for name in HOOKS:
        assert re.search(r"\bint " + name + r"\(", hdr), name
        assert name in _lib.SYMBOLS and getattr(l, name).restype is C.c_int, name
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", hdr).group(1)
        assert len(decl.split(",")) == len(_lib.SYMBOLS[name][1]), name   # as many argtypes as declared parameters


def test_mirrors_match_the_sources():
    ld = open(os.path.join(CSRC, "loudness.hip")).read()
    table = {}
    for cases, m in re.findall(r"((?:case \d+: )+)return (\d+);", ld[ld.index("int segment_len(int rate)"):]):
        for r in re.findall(r"case (\d+):", cases):
            table[int(r)] = int(m)
    assert table == SEG_LEN
    assert int(re.search(r"constexpr int kScanLanes = (\d+);", ld).group(1)) == SCAN_LANES
    assert int(re.search(r"constexpr int kScanLevels = (\d+);", ld).group(1)) == 8 and 1 << 8 == SCAN_LANES
    assert int(re.search(r"constexpr int kTpBack = (\d+);", ld).group(1)) == TP_BACK
    assert int(re.search(r"constexpr int kTpTaps = (\d+);", ld).group(1)) == TP_TAPS
    assert "hipLaunchKernelGGL(k_true_peak, dim3((unsigned)((total + 255) / 256)), blk" in ld and "const int64_t base = (int64_t)blockIdx.x * 256;" in ld
    assert TP_WG == 256 and "const int64_t c = (nseg + kScanLanes - 1) / kScanLanes;" in ld
    lim = open(os.path.join(CSRC, "limiter.hip")).read()
    assert int(re.search(r"constexpr int kTile = (\d+);", lim).group(1)) == TILE
    assert int(re.search(r"constexpr int kMaxK = (\d+);", lim).group(1)) == MAX_K == max(CURVE_RATES) // 100
    assert int(re.search(r"constexpr int kTpBack = (\d+);", lim).group(1)) == TP_BACK
    assert "const int K = rate / 100;" in lim and "const int K = a.K, len = kTile + 2 * K - 2;" in lim
    assert model.PARTS_SENTINEL.tobytes() == b"\x5a" * 8 and "constexpr unsigned char kCtxSentinel = 0x5A;" in open(os.path.join(CSRC, "test_hooks.cpp")).read()
    assert abs(10 ** (LEVEL_DB / 20) - G0) == 0


def test_reference_filter_is_long_double():
    """The reference runs in longdouble and is the kernel's recurrence: the state-space pass and the per-segment runs agree with a plain
    Python loop of the recurrence within a few longdouble ulp, and the float64 run differs from them by far more."""
    _ld_ok()
    rate, m = 48000, 100
    c = model.loudness_kweight(rate).astype(LD)
    y = _noise(1, 5 * m, 0.25, 0.9)
    s, acc, want = [LD(0)] * 4, LD(0), []
    for i, x in enumerate(y.astype(LD)):
        if i % m == 0:
            want.append(np.array(s))
            acc = LD(0)
        w, s = _kw_step(c, s, x)
        acc += w * w
    st = kw_sequential([y, y[:7]], c, m)
    eps = float(np.finfo(LD).eps)
    top = float(np.abs(st[0]).max())
    assert st[0].dtype == LD and st[0].shape == (5, 4) and st[1].shape == (1, 4) and float(np.abs(st[0] - np.array(want)).max()) <= 4096 * eps * top
    end, part = kw_runs(y.astype(LD), c, m, st[0])
    assert end.dtype == part.dtype == LD and float(np.abs(end[4] - np.array(s)).max()) <= 4096 * eps * top and abs(float(part[4] - acc)) <= 4096 * eps * float(acc)
    end64, _ = kw_runs(y, model.loudness_kweight(rate), m, st[0].astype(np.float64))
    assert end64.dtype == np.float64 and float(np.abs(end64[4] - end[4]).max()) > 16 * 4096 * eps * top


@pytest.mark.parametrize("rate", KW_RATES)
def test_kweighting_cases_cover_the_edges(rate):
    m, S = SEG_LEN[rate], rate // 10
    assert S % m == 0 and m % 5 == 0
    A, B, Cc = (kw_case(rate, k) for k in "ABC")
    assert [ceil_div(y.size, m) for y in A] == [1, 2, 255, 256, 257, 511, 512, 513]
    assert {ceil_div(ceil_div(y.size, m), SCAN_LANES) for y in A} == {1, 2, 3}
    assert {(y.size - 1) % m + 1 for y in A} == {1, 4, m - 1, m}
    assert [y.size for y in B] == [257 * m - 1, 0, 1, 4 * S - 1, 4 * S, 4 * S + 1, 512 * m + 4] and ceil_div(B[0].size, m) == 257 and ceil_div(B[6].size, m) == 513
    assert ceil_div(B[0].size, m) % 256 and all(abs(y.mean() - 0.9) < 0.1 for y in B if y.size > 100)    # a workgroup of k_kw_zero straddles signals; DC
    ref = kw_reference(rate, "C")
    c = model.loudness_kweight(rate).astype(LD)
    col = np.array([c[1] - c[3] * c[0], c[2] - c[4] * c[0], c[6] * c[0] - c[8] * (c[5] * c[0]), c[7] * c[0] - c[9] * (c[5] * c[0])])
    assert float(np.abs(ref[1]["st"][1] - col).max()) <= 8 * float(np.finfo(LD).eps)               # the impulse response's first column
    assert not ref[2]["st"][1].any() and np.array_equal(ref[2]["e"][1], ref[2]["st"][2]) and ref[2]["st"][2].any()
    total = sum(y.size for k in kw_names(rate) for y in kw_case(rate, k))
    assert total < 2.2e6 if rate == 8000 else total < 1.1e6
    for name in kw_names(rate):
        for i, r in enumerate(kw_reference(rate, name)):
            print(f"[mirror {rate} {name}{i}] n {r['n']}: err / (u top) e {r['err_e'] / (U * r['top_e'] or 1):.3g} st {r['err_st'] / (U * (r['top_st'] or 1)):.3g}; "
                  f"err part / (u max part) {r['err_part'] / (U * float(r['part'].max()) if r['n'] else 1):.3g}")


@pytest.mark.parametrize("rate", KW_RATES)
def test_no_gate_block_is_marginal(rate):
    m, S = SEG_LEN[rate], rate // 10
    for name in kw_names(rate):
        for i, r in enumerate(kw_reference(rate, name)):
            L, margin = gate_ref(r["part"], r["n"], m, S)
            assert margin > 1e-6, (rate, name, i, L, margin)
    if rate == 8000:   # the stepped cases: blocks under the absolute gate, blocks under the relative gate alone, so the passes count different sets
        for i, r in enumerate(kw_reference(rate, "G")[:4]):
            part = r["part"]
            nq = r["n"] // S
            q = part[:nq * (S // m)].reshape(nq, S // m).sum(axis=1)
            l = -0.691 + 10 * np.log10(((q[:-3] + q[1:-2] + q[2:-1] + q[3:]) / (4 * S)).astype(np.float64))
            L, _ = gate_ref(part, r["n"], m, S)
            first = l > -70
            gate = -0.691 + 10 * np.log10(np.mean(10 ** ((l[first] + 0.691) / 10))) - 10
            assert l.size == (255, 256, 257, 513)[i] and 0 < (~first).sum() and 0 < (first & (l <= gate)).sum() and (first & (l > gate)).sum() > 0
        G = kw_case(rate, "G")
        assert [y.size for y in G[4:]] == [1, 4 * S - 1, 0, 5 * S] and gate_ref(kw_reference(rate, "G")[7]["part"], 5 * S, m, S)[0] == -np.inf


@pytest.mark.parametrize("rate", KW_RATES)
def test_wrong_scans_exceed_the_tolerance(rate):
    """The start state of segment k - 1 used for k; a zero start at every chunk's first segment; (A^m)^c applied across a chunk of fewer than c
    segments (balanced chunks): each must leave the tolerance of st, and of part after the rerun, on every signal it can touch."""
    m, c = SEG_LEN[rate], model.loudness_kweight(rate)
    for name in ("A", "B"):
        for i, (y, r) in enumerate(zip(kw_case(rate, name), kw_reference(rate, name))):
            nseg = ceil_div(y.size, m)
            if nseg < 3:
                continue
            cc = ceil_div(nseg, SCAN_LANES)
            wrong = {"prev_start": np.concatenate([np.zeros((1, 4)), r["st_m"][:-1]]), "zero_chunk_start": scan_mirror(r["e_m"], seg_matrix(rate), "zero_chunk_start")}
            if nseg > SCAN_LANES and nseg % SCAN_LANES and nseg % SCAN_LANES < SCAN_LANES - 1:   # a short chunk ahead of full ones
                wrong["partial_chunk"] = scan_mirror(r["e_m"], seg_matrix(rate), "partial_chunk")
            for bug, st in wrong.items():
                rs = _ratio(np.abs(st - r["st"]).max(), r["tol_st"])
                _, part = kw_runs(y, c, m, st)
                rp = _ratio(np.abs(part - r["part"]), r["tol_part"])
                print(f"[wrong scan {bug} {rate} {name}{i}] error / tolerance: st {rs:.3g}, part {rp:.3g}")
                assert rs > 1 and rp > 1, (bug, rate, name, i, cc)
    assert any(ceil_div(y.size, m) in (257, 513) for y in kw_case(rate, "A"))


def test_wrong_gates():
    """>= for > on a constructed tie (a block at exactly -70 LUFS in the reference's arithmetic); the relative gate from all blocks."""
    _ld_ok()
    z = LD(10) ** ((LD(-70) + LD(-0.691) * -1) / 10)
    tie = None
    for _ in range(4096):
        if LD(-0.691) + 10 * np.log10(z) == -70:
            tie = z
            break
        z = np.nextafter(z, LD(1) if LD(-0.691) + 10 * np.log10(z) < -70 else LD(0))
    assert tie is not None
    part = np.array([tie], LD)
    assert gate_ref(part, 1, 200, 800)[0] == -np.inf and gate_ref(part, 1, 200, 800, "ge")[0] == -70.0
    m, S = SEG_LEN[8000], 800
    for i, r in enumerate(kw_reference(8000, "G")[:4]):
        L, _ = gate_ref(r["part"], r["n"], m, S)
        W, _ = gate_ref(r["part"], r["n"], m, S, "all_blocks")
        assert abs(W - L) > 1e3 * gate_tol(L, r["n"], m, S), (i, L, W)


def test_true_peak_case_covers_the_edges():
    lens = np.array(TP_LENS)
    off = np.concatenate([[0], np.cumsum(lens)])
    edges = {int(o) % TP_WG for o in off[:-1][lens > 0]} | {int(o) % TP_WG for o in off[1:][lens > 0]}
    assert {0, 1, 11, 12, 13, 243, 244, 245, 255} <= edges and {1, 23, 24, 25} <= set(TP_LENS) and 0 in TP_LENS
    sig_of, straddle = tp_layout(TP_LENS)
    waves = [set(sig_of[o:o + 64]) for o in range(0, sig_of.size, 64)]
    assert max(len(w) for w in waves) >= 3                                        # the lane-level atomics
    four = [b for b in range(len(waves) // 4) if all(len(waves[4 * b + w]) == 1 for w in range(4)) and len({min(waves[4 * b + w]) for w in range(4)}) == 4]
    assert four == [4] and straddle[4]                                            # the wave-level branch: one signal per wave, four in the workgroup
    assert sig_of.size % TP_WG and not straddle[-1] and (~straddle).sum() >= 5 and straddle.sum() >= 5
    ref = tp_reference(numpy_taps().tobytes())
    sigs = tp_case()
    # a full-scale last sample beside a quiet successor, a full-scale first sample beside a quiet predecessor
    assert sigs[0][-1] == 1.0 and np.abs(sigs[1]).max() < 0.01 and sigs[17][0] == 1.0 and np.abs(sigs[15]).max() < 0.01
    regions = set()
    for s, n in enumerate(TP_LENS):
        if n:
            p = int(np.argmax(ref["v"][off[s]:off[s] + n]))
            regions.add(("edge" if min(p, n - 1 - p) < TP_BACK else "inner", "straddling" if straddle[(off[s] + p) // TP_WG] else "interior"))
    assert regions == {("edge", "straddling"), ("edge", "interior"), ("inner", "straddling"), ("inner", "interior")}
    bmax, _, peak, _ = ref["peaks"]
    assert not bmax[straddle].any() and bmax[~straddle].all() and peak[9] and not peak[16]


def test_wrong_interpolators_exceed_the_tolerance():
    """The window not cut at the signal's edge; |y| left out of the maximum; the taps shifted by one."""
    ref, sigs = tp_reference(numpy_taps().tobytes()), tp_case()
    bmax, tb, peak, tpk = ref["peaks"]
    off = np.concatenate([[0], np.cumsum(TP_LENS)])
    for bug in ("uncut", "no_y", "shift"):
        t, _, v = interp_ref(sigs, numpy_taps(), bug)
        wb, _, wp, _ = peak_ref(TP_LENS, v, ref["tol"])
        rt, rb, rp = _ratio(np.abs(t - ref["t"]), ref["tol"]), _ratio(np.abs(wb - bmax), tb), _ratio(np.abs(wp - peak), tpk)
        print(f"[wrong interpolator {bug}] error / tolerance: t {rt:.3g}, bmax {rb:.3g}, peak {rp:.3g}")
        # (no workgroup inside one signal holds an edge between two signals, so the uncut window cannot move bmax; without |y|, t is unchanged)
        assert {"uncut": rt > 1 and rp > 1, "no_y": rb > 1 and rp > 1, "shift": rt > 1 and rb > 1 and rp > 1}[bug], bug
        if bug == "uncut":   # the quiet neighbours of the two full-scale samples are where it leaks
            for s in (1, 15):
                sl = slice(off[s], off[s + 1])
                assert _ratio(np.abs(t[sl] - ref["t"][sl]), ref["tol"][sl]) > 1e6


@pytest.mark.parametrize("rate", CURVE_RATES)
def test_curve_case_covers_the_edges(rate):
    K = rate // 100
    lay, names = curve_layout(K)
    ref = cpu_curve_reference(rate)
    assert {n for n, _ in lay} >= {1, K - 1, K, K + 1, 1023, 1024, 1025, LONG, 0} and 2 <= K <= MAX_K
    hsum = seq_sum(numpy_hann(K))
    for (n, spikes), d in zip(lay, ref):
        assert not d["undecided"].any()
        want = sorted({q for p in spikes for q in (p - 1, p, p + 1) if 0 <= q < n})
        assert list(np.flatnonzero(d["r"] < 1)) == want, (rate, n, spikes)
    # m[0] before the start: a loud first sample holds the gain down over the first K - 1 samples of the Hann sum
    assert ref[1]["s"][0] < 0.6 and ref[4]["s"][K // 2] < 0.9
    lb, li, rb, ri = (ref[names[k]] for k in ("left_bite", "left_idle", "right_bite", "right_idle"))
    h = numpy_hann(K)
    assert lb["m"][N0 - K + 1] < 1 and np.all(lb["m"][N0 - K + 2:N0 + 1] == 1) and not lb["idle"][1]
    assert abs(lb["s_sum"][N0] - (hsum - h[K - 1] * (1 - lb["m"][N0 - K + 1]))) <= 2 * K * U and hsum - lb["s_sum"][N0] > 1e3 * lb["tau_s"][N0]
    assert np.all(lb["m"][N0 - K + 2:N0 + TILE] == 1)
    assert li["idle"][1] and not li["idle"][0] and list(lb["idle"]) == [False, False, True, True]
    assert rb["m"][N0 + TILE - 1] < 1 and np.all(rb["m"][N0 - K + 1:N0 + TILE - 1] == 1) and not rb["idle"][1]
    assert abs(rb["s_sum"][N0 + TILE - 1] - (hsum - h[0] * (1 - rb["m"][N0 + TILE - 1]))) <= 2 * K * U
    assert hsum - rb["s_sum"][N0 + TILE - 1] > 1e3 * rb["tau_s"][N0 + TILE - 1]
    assert ri["idle"][1] and not ri["idle"][2] and list(ri["idle"]) == [True, True, False, ri["idle"][3]]
    e0 = names["edge_pair"]
    assert not ref[e0]["idle"][0] and ref[e0 + 1]["idle"].all() and ref[e0 + 2]["idle"].all() and not ref[e0 + 3]["idle"][0]
    assert sum(d["idle"].sum() for d in ref) >= 8 and sum((~d["idle"]).sum() for d in ref) >= 8


@pytest.mark.parametrize("rate", CURVE_RATES)
def test_wrong_curves(rate):
    """A window of K - 1; m = 1 before the start; a window crossing the signal's edge; a halo one sample short: each leaves the tolerance of x.
    The final min(s, r[n]) omitted cannot (module docstring): where the guard bites it moves x by less than the tolerance."""
    K = rate // 100
    lay, names = curve_layout(K)
    ref, sigs = cpu_curve_reference(rate), curve_case(rate)
    for bug in ("short_window", "m_one", "cross_edge", "halo_short"):
        w = curve_ref(sigs, numpy_taps(), K, numpy_hann(K), bug)
        ratios = [_ratio(np.abs(a["x"] - b["x"]), b["tol_x"]) for a, b in zip(w, ref)]
        print(f"[wrong curve {bug} {rate}] worst error / tolerance: {max(ratios):.3g}")
        assert max(ratios) > 1, (bug, rate)
        if bug == "m_one":
            assert ratios[1] > 1 and ratios[4] > 1                                      # the signals with a loud first sample
        if bug == "cross_edge":
            assert ratios[names["edge_pair"] + 1] > 1 and ratios[names["edge_pair"] + 2] > 1   # the quiet neighbours of the loud edges
        if bug == "halo_short":
            for k, n in (("left_bite", N0), ("right_bite", N0 + TILE - 1)):
                a, b = w[names[k]], ref[names[k]]
                assert abs(a["x"][n] - b["x"][n]) > b["tol_x"][n] > 0, (rate, k)
    w = curve_ref(sigs, numpy_taps(), K, numpy_hann(K), "no_min")
    bites = [(i, int(n)) for i, d in enumerate(ref) for n in np.flatnonzero(d["s_sum"] > d["r"])]
    for i, n in bites:
        assert w[i]["s"][n] > ref[i]["s"][n] and abs(w[i]["x"][n] - ref[i]["x"][n]) <= ref[i]["tol_x"][n]
    print(f"[wrong curve no_min {rate}] the guard bites at (signal, sample) {bites[:8]}{' ...' if len(bites) > 8 else ''}: {len(bites)} samples, all inside the tolerance")
    assert max(_ratio(np.abs(a["x"] - b["x"]), b["tol_x"]) for a, b in zip(w, ref)) <= 1


def _refusals():
    l = _lib.lib()
    f64p, marker = C.POINTER(C.c_double), 123.25
    x = np.ones(8)
    bufs = [np.full(64, marker) for _ in range(7)]
    counts = np.full(4, 77, np.int64)
    p = lambda a: a.ctypes.data_as(f64p)

    def loud(rate, lens, null=None):
        ln = np.array(lens, np.int64)
        args = [p(b) for b in bufs]
        if null is not None:
            args[null] = None
        return l.sbv2_debug_loudness_parts(0, x.ctypes.data, ln.ctypes.data_as(_lib.i64p), len(lens), rate, args[0], 8, 8, *args[1:], counts.ctypes.data_as(_lib.i64p))

    def lim(rate, lens, level, null=None):
        ln = np.array(lens, np.int64)
        args = [p(b) for b in bufs[:5]]
        if null is not None:
            args[null] = None
        return l.sbv2_debug_limiter_parts(0, x.ctypes.data, ln.ctypes.data_as(_lib.i64p), len(lens), rate, C.byref(level), 8, *args, counts.ctypes.data_as(_lib.i64p))

    ok = model.StreamLevel(LEVEL_DB, CEILING_DB).c
    calls = [lambda: loud(44000, [8]), lambda: loud(8000, [4, -1]), lambda: loud(8000, [8], null=0), lambda: loud(8000, [8], null=6),
             lambda: loud(8000, [8], null=3), lambda: lim(11025, [8], ok), lambda: lim(8000, [-8], ok), lambda: lim(8000, [8], ok, null=0),
             lambda: lim(8000, [8], ok, null=4), lambda: lim(8000, [8], _lib.Sbv2StreamLevel(50.0, -1.0, (C.c_double * 2)(0.0, 0.0)))]
    for i, call in enumerate(calls):
        assert call() != 0, i
        assert all(np.all(b == marker) for b in bufs) and np.all(counts == 77), i
    for what, call in (("sample rate", lambda: model.debug_loudness_parts([x], 12345)), ("negative", calls[1]), ("bad arguments", calls[2])):
        if what == "sample rate":
            with pytest.raises(model.Sbv2Error, match=what):
                call()
        else:
            assert call() != 0 and what in l.sbv2_last_error().decode()


def test_bad_calls_are_refused_before_any_device_call():
    _refusals()


# ---- GPU part -----------------------------------------------------------------------------------------------------------------------------

def _clean(arrays, strays, what):
    """No sentinel left, no NaN, no pad word touched."""
    assert strays == 0, (what, strays)
    for k, a in arrays.items():
        assert not np.isnan(a).any(), (what, k)
        assert not np.any(a.view(np.uint64) == model.PARTS_SENTINEL.view(np.uint64)), (what, k)


def _check_meter_stats(got, lens, rate, what):
    """L from the returned part, TP from the returned bmax / peak, G = 0."""
    m, S = SEG_LEN[rate], rate // 10
    seg0 = np.concatenate([[0], np.cumsum([ceil_div(n, m) for n in lens])])
    off = np.concatenate([[0], np.cumsum(lens)])
    worst = {"L": 0.0, "TP": 0.0}
    for s, n in enumerate(lens):
        L, margin = gate_ref(got["part"][seg0[s]:seg0[s + 1]], n, m, S)
        gl, gtp, gg = got["stats"][s]
        assert margin > 1e-6 and gg == 0.0, (what, s)
        if np.isfinite(L):
            worst["L"] = max(worst["L"], _ratio(abs(gl - L), gate_tol(L, n, m, S)))
        else:
            assert gl == L, (what, s, gl)
        pk = max(got["bmax"][off[s] // TP_WG:(off[s] + n - 1) // TP_WG + 1].max(), got["peak"][s]) if n else 0.0
        with np.errstate(divide="ignore"):
            tp = 20 * np.log10(pk)
        if np.isfinite(tp):
            worst["TP"] = max(worst["TP"], _ratio(abs(gtp - tp), 8 * U * max(1.0, abs(tp))))
        else:
            assert gtp == tp, (what, s, gtp)
    return worst


@gpu
@pytest.mark.parametrize("rate", KW_RATES)
def test_kweighting_launches(rate):
    m = SEG_LEN[rate]
    for name in kw_names(rate):
        sigs, ref = kw_case(rate, name), kw_reference(rate, name)
        got = model.debug_loudness_parts(sigs, rate)
        _clean({k: got[k] for k in ("e", "st", "part", "bmax", "peak")}, got["strays"], (rate, name))
        assert got["m"] == m and got["e"].shape == got["st"].shape == (sum(ceil_div(y.size, m) for y in sigs), 4)
        worst, k0 = {"e": 0.0, "st": 0.0, "part": 0.0, "vs mirror e": 0.0, "vs mirror st": 0.0}, 0
        for r in ref:
            k1 = k0 + r["e"].shape[0]
            for key in ("e", "st"):
                err = float(np.abs(got[key][k0:k1] - r[key]).max()) if k1 > k0 else 0.0
                worst[key] = max(worst[key], _ratio(err, r["tol_" + key]))
                if r["err_" + key]:
                    worst["vs mirror " + key] = max(worst["vs mirror " + key], err / r["err_" + key])
            worst["part"] = max(worst["part"], _ratio(np.abs(got["part"][k0:k1] - r["part"]), r["tol_part"]))
            k0 = k1
        worst.update(_check_meter_stats(got, [y.size for y in sigs], rate, (rate, name)))
        print(f"[kw {rate} {name}] worst error / tolerance: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items() if not k.startswith("vs")) +
              f"; kernel error / mirror error: e {worst['vs mirror e']:.3g}, st {worst['vs mirror st']:.3g}")
        assert all(v <= 1.0 for k, v in worst.items() if not k.startswith("vs")), worst


@gpu
@pytest.mark.parametrize("rate", TP_RATES)
def test_true_peak_and_interpolator_launches(rate):
    sigs = tp_case()
    got = model.debug_loudness_parts(sigs, rate)
    lim = model.debug_limiter_parts(sigs, rate, model.StreamLevel(0.0, CEILING_DB))
    _clean({k: got[k] for k in ("e", "st", "part", "bmax", "peak")}, got["strays"], ("tp", rate))
    _clean({k: lim[k] for k in ("t", "x", "smin")}, lim["strays"], ("tp lim", rate))
    assert float(np.abs(got["taps"] - numpy_taps()).max()) <= 64 * U
    ref = tp_reference(got["taps"].tobytes())
    bmax, tb, peak, tpk = ref["peaks"]
    _, straddle = tp_layout(TP_LENS)
    assert not got["bmax"][straddle].any() and not got["peak"][peak == 0].any()
    worst = {"t": _ratio(np.abs(lim["t"] - ref["t"]), ref["tol"]), "bmax": _ratio(np.abs(got["bmax"] - bmax), tb), "peak": _ratio(np.abs(got["peak"] - peak), tpk)}
    worst.update(_check_meter_stats(got, TP_LENS, rate, ("tp", rate)))
    print(f"[tp {rate}] worst error / tolerance: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), worst


@gpu
@pytest.mark.parametrize("rate", CURVE_RATES)
def test_curve_launches(rate):
    K, sigs = rate // 100, curve_case(rate)
    got = model.debug_limiter_parts(sigs, rate, model.StreamLevel(LEVEL_DB, CEILING_DB))
    _clean({k: got[k] for k in ("t", "x", "smin")}, got["strays"], ("curve", rate))
    assert got["K"] == K and got["taps"].size == K and float(np.abs(got["taps"] - numpy_hann(K)).max()) <= 8 * U
    hsum = seq_sum(got["taps"])
    assert got["hsum"] == hsum
    taps = model.debug_loudness_parts([np.zeros(1)], rate)["taps"]
    ref = curve_reference(rate, taps.tobytes(), got["taps"].tobytes())
    worst, off, tile, idle_tiles = {"x": 0.0, "smin": 0.0}, 0, 0, 0
    for d in ref:
        n = d["y"].size
        x = got["x"][off:off + n]
        assert not d["undecided"].any()
        worst["x"] = max(worst["x"], _ratio(np.abs(x - d["x"]), d["tol_x"]))
        for i, idle in enumerate(d["idle"]):
            sl = slice(i * TILE, min((i + 1) * TILE, n))
            if idle:
                assert np.array_equal(x[sl].view(np.uint64), d["x_idle"][sl].view(np.uint64)), (rate, n, i)
                assert got["smin"][tile] == min(hsum, 1.0), (rate, n, i)
                idle_tiles += 1
            else:
                worst["smin"] = max(worst["smin"], _ratio(abs(got["smin"][tile] - d["s"][sl].min()), d["tau_s"][sl].max()))
            tile += 1
        off += n
    assert tile == got["smin"].size
    print(f"[curve {rate}] worst error / tolerance: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()) + f"; tiles bit-exact idle: {idle_tiles} of {tile}")
    assert all(v <= 1.0 for v in worst.values()), worst


@gpu
def test_bad_calls_are_refused_with_a_device_present():
    _refusals()
    got = model.debug_limiter_parts([np.zeros(3)], 8000, model.StreamLevel(LEVEL_DB, CEILING_DB))   # and a good call right after is served
    assert not got["x"].any() and got["smin"].size == 1
