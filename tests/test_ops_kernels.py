"""The non-GEMM kernels of csrc/ops.hip launch by launch (the sbv2_debug_* hooks of csrc/test_hooks.cpp: one launcher of ops.h on host data, planes at
the library's pitches, packed layouts from the models' own make_layout) against float64 numpy statements of the same operation.

Tolerances (the worst error / tolerance ratio of each case is printed; none is taken from a kernel's output):
- f32 kernels: max(4 err32, floor); err32 = the same reference evaluated in float32 on the same data, floor = 8 ulp (8 * 2^-24) of the output's scale.
  LayerNorm: per column, and the scale also covers |mean| * rstd * max|gamma| (the column mean is a number of the input's magnitude: its f32 rounding alone
  moves every output of the column by that much).  A column of one dyadic constant is exact in any summation order: the plain result must EQUAL beta.
- split-operand planes (hi + lo against the f32 result y of the same launch): two bf16 parts, each a rounding to 8 significant bits (half an ulp = 2^-8
  relative), the second of what the first left: |y - hi - lo| <= 2^-16 |y| (the figure tests/test_attention_kernels.py uses for the same split);
  the f16 pair is f16(y) and f16((y - hi) * 2^11), each 2^-11 relative in f16's normal range and 2^-25 absolute below it: <= 2^-22 |y| + 2^-36; both plus
  2^-24 |y| for the f32 sum the hook returns.  Tail columns (split_store1) and whole quads (split_store4) get the same bound.
- spline: max(4 err32, 8 ulp of the tail bound); values outside the tails come back bit for bit.  The spline is C1 across knots, so a kernel that picks the
  neighbouring bin at a knot is inside the tolerance; bin indices are not compared.
- durations: see test_durations' docstring for the undecidable window.
- noise: hash_normal is evaluated in double on both sides and rounded to float once; double results that differ in their last bits round to the same or
  the neighbouring float, so the claim to test was 1 f32 ulp.  On the MI355X not one of 16 000 samples differed from numpy's, at scale 1 and at 0.6, so
  the test asserts equality.
- movers: assert_array_equal.
Every numeric family has a deliberately wrong reference (numpy) that must exceed the tolerance on the same data: the CPU part of this module.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sbv2_oracle as O
from helpers import noise_key
from sbv2_api_amd import _lib, synth

gpu = pytest.mark.gpu
f32p, i64p = _lib.f32p, _lib.i64p
i32p = C.POINTER(C.c_int32)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS32 = 2.0 ** -24
TEXT, FRAMES = 0, 1
TEXT_GAP, FRAME_GAP = 16, 4   # kTextGap / kFrameGap of csrc/models.h (checked against the library's layout in test_layout_hook)
ACT_NONE, ACT_GELU = 0, 2
HOOKS = ["sbv2_debug_layout", "sbv2_debug_layernorm", "sbv2_debug_deberta_embed_ln", "sbv2_debug_spline_inverse", "sbv2_debug_durations",
         "sbv2_debug_affine_reverse", "sbv2_debug_convflow_pre", "sbv2_debug_noise_fill", "sbv2_debug_expand_frames", "sbv2_debug_conv_post_tanh",
         "sbv2_debug_linear_vec", "sbv2_debug_gather_rows", "sbv2_debug_text_embed", "sbv2_debug_add_segvec", "sbv2_debug_plane_op",
         "sbv2_debug_copy_segments"]


def _f(a):
    return None if a is None else a.ctypes.data_as(f32p)


def _i32(a):
    return a.ctypes.data_as(i32p)


def _i64(a):
    return a.ctypes.data_as(i64p)


def _c32(a):
    return None if a is None else np.ascontiguousarray(a, np.float32)


def _u8(a):
    return None if a is None else np.ascontiguousarray(a, np.uint8)


def _report(name, err, tol):
    ratio = float(np.max(np.asarray(err, np.float64) / tol))
    print(f"[{name}] worst error / tolerance = {ratio:.3f}")
    return ratio


# ---- LayerNorm: the dispatch of launch_layernorm (csrc/ops.hip), mirrored -----------------------------------------------------------------------------

def ln_kernel(C_, L, ksplit, dw=False):
    """Which instantiation launch_layernorm takes (planes of the library: every pitch a multiple of 64, so the quad kernel's alignment test holds)."""
    if ksplit and 512 <= C_ <= 8 * 128 and L <= 256:
        return "ch<8,2>"
    if ksplit and C_ < 512 and C_ <= 6 * 32 and L <= 1024:
        return "ch<6,8>"
    if not dw and C_ <= 6 * 32:
        return "q4<6,8>"
    if not dw and 512 <= C_ <= 32 * 32 and L <= 8192:
        return "ch<32,8>"
    cpt = (C_ + 7) // 8
    for lim in (8, 24, 32, 128):
        if cpt <= lim:
            return f"ch<{lim},32>"
    return "ch<0,32>"


# (C, L, small-grid switch, instantiation): k_layernorm_ch<false, 8 | 24, 32> cannot be reached at the library's pitches (C <= 192 goes to the quad kernel);
# those two run as k_layernorm_ch<true, ...> in DW_CASES
LN_CASES = [
    (1024, 66, 1, "ch<8,2>"), (768, 255, 1, "ch<8,2>"), (513, 1, 1, "ch<8,2>"), (1024, 256, 1, "ch<8,2>"),
    (192, 257, 1, "ch<6,8>"), (29, 1024, 1, "ch<6,8>"), (191, 7, 1, "ch<6,8>"),
    (192, 1025, 1, "q4<6,8>"), (192, 1, 0, "q4<6,8>"), (191, 3, 0, "q4<6,8>"), (96, 4, 0, "q4<6,8>"), (2, 5, 0, "q4<6,8>"), (1, 31, 0, "q4<6,8>"),
    (192, 32, 0, "q4<6,8>"), (191, 33, 0, "q4<6,8>"), (96, 1025, 0, "q4<6,8>"), (192, 37, 0, "q4<6,8>"),
    (1024, 257, 1, "ch<32,8>"), (1024, 257, 0, "ch<32,8>"), (520, 8192, 0, "ch<32,8>"), (1000, 50, 0, "ch<32,8>"),
    (1024, 8193, 0, "ch<128,32>"), (520, 8193, 1, "ch<128,32>"), (300, 70, 0, "ch<128,32>"), (511, 33, 1, "ch<128,32>"),
    (256, 100, 0, "ch<32,32>"), (200, 33, 1, "ch<32,32>"), (193, 1, 0, "ch<32,32>"),
    (1025, 45, 0, "ch<0,32>"), (1500, 31, 1, "ch<0,32>"),
]
# dds_dw_ln_gelu: (C, small-grid switch, instantiation <true, ...>); every one it can reach (<true, 32, 8> is excluded by the launcher)
DW_CASES = [(192, 0, "ch<24,32>"), (64, 0, "ch<8,32>"), (3, 0, "ch<8,32>"), (192, 1, "ch<6,8>"), (200, 1, "ch<32,32>"), (300, 0, "ch<128,32>"),
            (600, 1, "ch<8,2>"), (600, 0, "ch<128,32>"), (1030, 1, "ch<0,32>")]
ALL_LN = {"ch<8,2>", "ch<6,8>", "q4<6,8>", "ch<32,8>", "ch<8,32>", "ch<24,32>", "ch<32,32>", "ch<128,32>", "ch<0,32>"}


def _ln_id(c):
    return f"C{c[0]}-L{c[1]}-{'small' if c[2] else 'batch'}-{c[3]}"


def _ln_data(C_, L, kind, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((C_, L))
    if kind == "offset":
        x = x + 1000.0
    x = x.astype(np.float32)
    const = L // 2 if L > 1 else -1   # (none in a one-column plane)
    if const >= 0:
        x[:, const] = 1000.0 if kind == "offset" else 1.5   # variance 0: rstd = 1 / sqrt(eps), the result is beta
    gamma = (1.0 + 0.3 * rng.standard_normal(C_)).astype(np.float32)
    beta = (0.2 * rng.standard_normal(C_)).astype(np.float32)
    res = rng.standard_normal((C_, L)).astype(np.float32)
    mask = (rng.random(L) > 0.3).astype(np.uint8)
    return x, gamma, beta, res, mask, const


def _ln_ref(x, gamma, beta, eps, act, res, mask, dt, ddof=0):
    x, gamma, beta = x.astype(dt), gamma.astype(dt), beta.astype(dt)
    mu = x.mean(axis=0, keepdims=True)
    xc = x - mu
    var = (xc * xc).sum(axis=0, keepdims=True) / dt(x.shape[0] - ddof if x.shape[0] > ddof else 1)
    y = xc / np.sqrt(var + dt(eps)) * gamma[:, None] + beta[:, None]
    if ddof == 0:   # the oracle's own statement, where it applies
        y = O.channel_layer_norm(x, gamma, beta, eps).astype(dt)
    if act == ACT_GELU:
        y = O.gelu(y)
    if res is not None:
        y = y + res.astype(dt)
    if mask is not None:
        y = y * mask.astype(dt)[None, :]
    return y


def _ln_tol(x, gamma, eps, ref, ref32):
    """Per column (module docstring)."""
    x64 = x.astype(np.float64)
    mu = x64.mean(axis=0)
    rstd = 1.0 / np.sqrt(x64.var(axis=0) + eps)
    scale = np.maximum(1.0, np.maximum(np.abs(ref).max(axis=0), np.abs(mu) * rstd * float(np.abs(gamma).max())))
    err32 = np.abs(ref32.astype(np.float64) - ref).max(axis=0)
    return np.maximum(4 * err32, 8 * EPS32 * scale)[None, :]


def _split_bound(y, code):
    y = np.abs(y.astype(np.float64))
    return (2.0 ** -16 + EPS32) * y + 1e-37 if code == 2 else (2.0 ** -22 + EPS32) * y + 2.0 ** -36


def _dw_pre(x, w, b, dil, dt):
    x, w, b = x.astype(dt), w.astype(dt), b.astype(dt)
    L = x.shape[1]
    v = np.repeat(b[:, None], L, axis=1)
    for j in range(3):
        s = (j - 1) * dil
        lo, hi = max(0, -s), min(L, L - s)
        if hi > lo:
            v[:, lo:hi] += w[:, j:j + 1] * x[:, lo + s:hi + s]
    return v


# ---- references of the other families (dtype-parametrised, so err32 is "the same reference in float32") ------------------------------------------------

def _spline_ref(P, z1, inv, dt, **kw):
    P = P.astype(dt)
    u = P[:20] * dt(np.float32(inv))
    return O.rq_spline_inverse(z1.astype(dt), u[:10].T.copy(), u[10:20].T.copy(), P[20:].T.copy(), 5.0, **kw)


def _knots(P, inv):
    """float64 knots of the heights (ch of the oracle) [T, 11]"""
    u = (P[10:20].astype(np.float64) * float(np.float32(inv))).T
    w = 1e-3 + (1 - 1e-3 * 10) * O.softmax(u, axis=-1)
    c = np.concatenate([np.zeros((u.shape[0], 1)), np.cumsum(w, axis=-1)], axis=-1) * 10.0 - 5.0
    c[:, 0], c[:, -1] = -5.0, 5.0
    return c


def _conv_post_ref(x, w, dt, shift=0):
    """tanh(conv_post(leaky_relu(x, 0.01))) over the whole gapped plane, zero padding; shift != 0 moves the tap window (the wrong reference)"""
    C_, L = x.shape
    k = w.shape[1]
    v = O.leaky_relu(x.astype(dt), 0.01)
    half = k // 2 + shift
    vp = np.zeros((C_, L + 2 * (k + 1)), dt)
    vp[:, k + 1:k + 1 + L] = v
    a = np.zeros(L, dt)
    for j in range(k):
        o = k + 1 + j - half
        a += (w[:, j:j + 1].astype(dt) * vp[:, o:o + L]).sum(axis=0, dtype=dt)
    return np.tanh(a)


def _layout(lens, kind):
    """The layout make_layout gives (csrc/model_common.cpp), restated; test_layout_hook checks it against the library."""
    gap, rnd = (FRAME_GAP, 32) if kind == FRAMES else (TEXT_GAP, 4)
    pos, start = 0, []
    for v in lens:
        st = (pos + 3) // 4 * 4
        start.append(st)
        pos = st + v + gap
    L = (max(pos, 4) + rnd - 1) // rnd * rnd
    return start, L


def _seg_of(lens, start, L):
    seg = np.full(L, -1, np.int64)
    for u, (s, n) in enumerate(zip(start, lens)):
        seg[s:s + n] = u
    return seg


def _noise_ref(lens, start, L, seg_utt, seed, stream, rows, row_stride_is_L=False):
    out = np.zeros((rows, L), np.float32)
    for u, (s, n) in enumerate(zip(start, lens)):
        key = noise_key(seed, int(seg_utt[u]), stream)
        if row_stride_is_L:   # the wrong reference: element index r * L + t
            h = synth.hash_normal(key, rows * L).reshape(rows, L)[:, :n]
        else:
            h = synth.hash_normal(key, rows * n).reshape(rows, n)
        out[:, s:s + n] = h
    return out


def _dur_window(sdp, dp, ratio, ls):
    """float64 product p = exp(lw) * ls and the half-width of the f32 evaluation error around it (test_durations' docstring)."""
    r, r1 = float(np.float32(ratio)), float(np.float32(1.0) - np.float32(ratio))
    a, b = sdp.astype(np.float64) * r, dp.astype(np.float64) * r1
    lw = a + b
    dlw = EPS32 * (np.abs(a) + np.abs(b) + np.abs(lw))
    p = np.exp(lw) * float(np.float32(ls))
    return lw, dlw, p, 1.01 * p * (np.expm1(dlw) + 2.0 ** -23 + EPS32)


def _dur_inputs(seed, L=20000):
    rng = np.random.default_rng(seed)
    return (1.2 * rng.standard_normal(L)).astype(np.float32), (1.2 * rng.standard_normal(L)).astype(np.float32), (rng.random(L) > 0.1).astype(np.uint8)


DUR_CASES = [(0.0, 1.0), (0.5, 1.0), (1.0, 1.0), (0.5, 0.7), (1.0, 1.3), (0.0, 2.0)]


# ---- CPU part: hooks declared, dispatch coverage, wrong references, the durations cap -----------------------------------------------------------------

def test_hooks_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "sbv2_hip.h")).read()
    l = _lib.lib()
    for name in HOOKS:
        assert re.search(r"\bint " + name + r"\(", hdr), name
        assert name in _lib.SYMBOLS and getattr(l, name).restype is C.c_int, name


def test_layernorm_cases_cover_the_dispatch():
    for c in LN_CASES:
        assert ln_kernel(c[0], c[1], c[2]) == c[3], c
    for C_, k, name in DW_CASES:
        for L in (1, 26, 28):
            assert ln_kernel(C_, L, k, dw=True) == name, (C_, k)
    assert {c[3] for c in LN_CASES} == ALL_LN - {"ch<8,32>", "ch<24,32>"}
    assert {c[3] for c in LN_CASES} | {c[2] for c in DW_CASES} == ALL_LN
    assert {c[2] for c in DW_CASES} == ALL_LN - {"q4<6,8>", "ch<32,8>"}   # every <true, ...> instantiation the launcher can take
    assert any(c[1] % 4 and c[3] == "q4<6,8>" and c[1] > 4 for c in LN_CASES)   # tail columns and whole quads in one plane
    src = open(os.path.join(ROOT, "sbv2-api_amd", "csrc", "ops.hip")).read()
    body = src[src.index("static void launch_layernorm"):src.index("void layernorm_ch(")]
    inst = set(re.findall(r"k_layernorm_ch<DW, (\d+), (\d+)>", body))
    assert {f"ch<{a},{b}>" for a, b in inst} | {"q4<6,8>"} == ALL_LN and "k_layernorm_q4<6, 8>" in body


@pytest.mark.parametrize("case", [c for c in LN_CASES if c[0] > 1 and c[0] * c[1] < 600000], ids=_ln_id)
def test_layernorm_wrong_reference_exceeds_the_tolerance(case):
    """Variance divided by C - 1 instead of C."""
    C_, L = case[0], case[1]
    x, gamma, beta, res, mask, const = _ln_data(C_, L, "gauss", C_ * 7 + L)
    ref = _ln_ref(x, gamma, beta, 1e-5, ACT_NONE, None, None, np.float64)
    tol = _ln_tol(x, gamma, 1e-5, ref, _ln_ref(x, gamma, beta, 1e-5, ACT_NONE, None, None, np.float32))
    bad = _ln_ref(x, gamma, beta, 1e-5, ACT_NONE, None, None, np.float64, ddof=1)
    keep = np.arange(L) != const
    assert (np.abs(bad - ref) / tol)[:, keep].max() > 1.0
    y32 = _ln_ref(x, gamma, beta, 1e-5, ACT_NONE, None, None, np.float32)
    hi_bf16 = (y32.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)   # the split bound sees a missing lo part (hi alone)
    for code, hi in ((2, hi_bf16), (4, y32.astype(np.float16).astype(np.float32))):
        assert (np.abs(y32.astype(np.float64) - hi) / _split_bound(y32, code)).max() > 1.0


def _spline_cases(seed):
    """name -> (params [29][T], z1 [T]) with inv_sqrt_f = 1 / sqrt(192)"""
    rng = np.random.default_rng(seed)
    inv = 1.0 / np.sqrt(np.float32(192.0))
    s = float(np.sqrt(192.0))
    out = {}
    T = 4096
    P = rng.standard_normal((29, T)).astype(np.float32)
    P[:20] *= 2 * s
    out["uniform"] = (P, np.linspace(-5, 5, T).astype(np.float32))
    P = rng.standard_normal((29, 64)).astype(np.float32)
    P[:20] *= s
    f = np.float32
    edge = np.array([5.0, -5.0, np.nextafter(f(5), f(9)), np.nextafter(f(5), f(0)), np.nextafter(f(-5), f(-9)), np.nextafter(f(-5), f(0)), 7.5, -1e30], f)
    out["tails"] = (P, np.resize(edge, 64))
    P = rng.standard_normal((29, 33 * 4)).astype(np.float32)
    P[:20] *= 1.5 * s
    kn = _knots(P, inv)
    out["knots"] = (P, np.array([kn[t, t % 11] for t in range(P.shape[1])]).astype(np.float32))
    P = rng.standard_normal((29, 1024)).astype(np.float32)
    P[:20] *= 30 * s   # one bin takes nearly everything, the others sit at the 1e-3 minimum
    out["saturated"] = (P, rng.uniform(-5, 5, 1024).astype(np.float32))
    P = rng.standard_normal((29, 1000)).astype(np.float32)
    P[:20] *= s
    for i, d in enumerate((-30.0, 0.0, 19.9, 20.1, 60.0)):
        P[20:, i * 200:(i + 1) * 200] = d
    P[20:, ::7] = rng.choice([-30.0, 0.0, 19.9, 20.1, 60.0], size=(9, len(range(0, 1000, 7))))
    out["derivatives"] = (P, rng.uniform(-5, 5, 1000).astype(np.float32))
    return out, inv


SPLINE_FLOOR = 8 * EPS32 * 8.0   # 8 ulp of the tail bound (5 lies in [4, 8): ulp = 2^-21)


def test_spline_wrong_references_exceed_the_tolerance():
    cases, inv = _spline_cases(3)
    P, z1 = cases["uniform"]
    ref = _spline_ref(P, z1, inv, np.float64)
    tol = max(4 * float(np.abs(_spline_ref(P, z1, inv, np.float32) - ref).max()), SPLINE_FLOOR)
    assert np.abs(_spline_ref(P, z1, inv, np.float64, min_d=0.0) - ref).max() > tol      # without min_d
    shifted = P.copy()
    shifted[20:] = np.roll(P[20:], 1, axis=0)                                              # the neighbouring bin's derivatives
    assert np.abs(_spline_ref(shifted, z1, inv, np.float64) - ref).max() > tol
    assert tol < 1e-3


@pytest.mark.parametrize("ratio,ls", DUR_CASES)
def test_durations_exclusion_cap_holds_for_the_reference(ratio, ls):
    sdp, dp, _ = _dur_inputs(int(ratio * 10 + ls * 100))
    _, _, p, w = _dur_window(sdp, dp, ratio, ls)
    undec = np.abs(p - np.round(p)) <= w
    assert undec.mean() <= 1e-3, undec.sum()
    assert (np.ceil(p * 1.01) != np.ceil(p)).mean() > 1e-3   # a 1 % fault in the product changes more durations than the cap may exclude


def test_conv_post_and_noise_wrong_references_exceed_the_tolerance():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((16, 700)).astype(np.float32)
    w = (0.05 * rng.standard_normal((16, 7))).astype(np.float32)
    ref = _conv_post_ref(x, w, np.float64)
    tol = max(4 * float(np.abs(_conv_post_ref(x, w, np.float32) - ref).max()), 8 * EPS32)
    assert np.abs(_conv_post_ref(x, w, np.float64, shift=1) - ref).max() > tol and tol < 1e-5
    lens = [5, 9, 3]
    start, L = _layout(lens, TEXT)
    good = _noise_ref(lens, start, L, [2, 0, 1], 11, 0, 2)
    bad = _noise_ref(lens, start, L, [2, 0, 1], 11, 0, 2, row_stride_is_L=True)
    np.testing.assert_array_equal(good[0], bad[0])
    assert (np.abs(good[1] - bad[1]) > 2 * np.spacing(np.abs(good[1])))[_seg_of(lens, start, L) >= 0].mean() > 0.9
    ident = _noise_ref(lens, start, L, [0, 1, 2], 11, 0, 2)   # seg_utt ignored
    assert (good != ident)[:, _seg_of(lens, start, L) >= 0].mean() > 0.9


# ---- GPU: the layout hook -----------------------------------------------------------------------------------------------------------------------------

@gpu
def test_layout_hook():
    for kind in (TEXT, FRAMES):
        for lens in ([1], [5, 9, 3], [255, 256, 257, 31], [64] * 5):
            ln = np.asarray(lens, np.int64)
            st = np.zeros(len(lens), np.int32)
            L = C.c_int64(0)
            _lib.check(_lib.lib().sbv2_debug_layout(_i64(ln), len(lens), kind, _i32(st), C.byref(L)))
            start, Lr = _layout(lens, kind)
            assert list(st) == start and L.value == Lr, (kind, lens)
            assert start[0] == 0 and all(b - (a + n) >= (FRAME_GAP if kind else TEXT_GAP) for a, n, b in zip(start, lens, start[1:] + [Lr]))


# ---- GPU: LayerNorm -----------------------------------------------------------------------------------------------------------------------------------

def _ln(x, gamma, beta, eps, act=ACT_NONE, res=None, mask=None, dw=None, dil=1, inplace=0, split=0, poison=1):
    C_, L = x.shape
    x, gamma, beta, res, mask = _c32(x), _c32(gamma), _c32(beta), _c32(res), _u8(mask)
    dw_w, dw_b = (None, None) if dw is None else (_c32(dw[0]), _c32(dw[1]))
    y = np.empty((C_, L), np.float32)
    ys = np.empty((C_, L), np.float32) if split else None
    stray = C.c_int64(-1)
    _lib.check(_lib.lib().sbv2_debug_layernorm(0, _f(x), _f(gamma), _f(beta), eps, act, _f(res), None if mask is None else mask.ctypes.data, _f(dw_w),
                                               _f(dw_b), dil, C_, L, inplace, split, poison, _f(y), _f(ys), C.byref(stray)))
    return y, ys, stray.value


class _Ksplit:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.prev = _lib.lib().sbv2_debug_set_ksplit(self.on)

    def __exit__(self, *a):
        _lib.lib().sbv2_debug_set_ksplit(self.prev)


@gpu
@pytest.mark.parametrize("case", LN_CASES, ids=_ln_id)
def test_layernorm(case):
    """layernorm_ch at one (C, L, small-grid switch) of LN_CASES: plain, GELU, residual, column mask, in place, and both split-operand formats, on Gaussian
    data at eps 1e-5; plain and GELU + residual + mask on columns with mean 1e3 and spread 1 at DeBERTa's eps 1e-7.  Every plane has one constant column
    (the plain result there must equal beta).  Inputs are poisoned behind L; no launch may write there (stray == 0)."""
    C_, L, ks, name = case
    worst = 0.0
    with _Ksplit(ks):
        for kind, eps in (("gauss", 1e-5), ("offset", 1e-7)):
            x, gamma, beta, res, mask, const = _ln_data(C_, L, kind, C_ * 7 + L)
            variants = [("plain", ACT_NONE, None, None, 0, 0), ("gelu+res+mask", ACT_GELU, res, mask, 0, 0)]
            if kind == "gauss":
                variants += [("gelu", ACT_GELU, None, None, 0, 0), ("res", ACT_NONE, res, None, 0, 0), ("mask", ACT_NONE, None, mask, 0, 0),
                             ("inplace", ACT_NONE, None, None, 1, 0), ("inplace+res", ACT_GELU, res, mask, 1, 0),
                             ("split-bf16", ACT_NONE, None, None, 0, 2), ("split-f16", ACT_GELU, res, mask, 0, 4), ("split-f16-inplace", ACT_NONE, None, None, 1, 4)]
            base = _ln_ref(x, gamma, beta, eps, ACT_NONE, None, None, np.float64), _ln_ref(x, gamma, beta, eps, ACT_NONE, None, None, np.float32)
            for vn, act, r, m, inpl, split in variants:
                ref, ref32 = (_ln_ref(x, gamma, beta, eps, act, r, m, dt) for dt in (np.float64, np.float32)) if (act or r is not None or m is not None) else base
                tol = _ln_tol(x, gamma, eps, ref, ref32)
                y, ys, stray = _ln(x, gamma, beta, eps, act, r, m, inplace=inpl, split=split)
                assert stray == 0, (case, kind, vn, stray)
                assert np.isfinite(y).all(), (case, kind, vn)
                ratio = float((np.abs(y.astype(np.float64) - ref) / tol).max())
                if split:
                    ratio = max(ratio, float((np.abs(ys.astype(np.float64) - y.astype(np.float64)) / _split_bound(y, split)).max()))
                assert ratio <= 1.0, (case, kind, vn, ratio)
                worst = max(worst, ratio)
                if vn == "plain" and const >= 0:
                    np.testing.assert_array_equal(y[:, const], beta, err_msg=f"{case} {kind}: constant column")
    print(f"[layernorm {_ln_id(case)}] worst error / tolerance = {worst:.3f}")


@gpu
@pytest.mark.parametrize("C_,ks,name", DW_CASES, ids=[f"C{c[0]}-{'small' if c[1] else 'batch'}-{c[2]}" for c in DW_CASES])
def test_dds_dw_ln_gelu(C_, ks, name):
    """The depthwise-conv variant at dilations 1, 3, 9, 27 and L below, on and just above the dilation (both outer taps outside the plane), plus L = 100."""
    worst = 0.0
    with _Ksplit(ks):
        for dil in (1, 3, 9, 27):
            for L in sorted({max(dil - 1, 1), dil, dil + 1, 100}):
                rng = np.random.default_rng(C_ + 31 * dil + L)
                x = rng.standard_normal((C_, L)).astype(np.float32)
                w = (0.5 * rng.standard_normal((C_, 3))).astype(np.float32)
                b = (0.1 * rng.standard_normal(C_)).astype(np.float32)
                gamma = (1.0 + 0.3 * rng.standard_normal(C_)).astype(np.float32)
                beta = (0.2 * rng.standard_normal(C_)).astype(np.float32)
                mask = (rng.random(L) > 0.2).astype(np.uint8)
                for m in (None, mask):
                    refs = []
                    for dt in (np.float64, np.float32):
                        refs.append(_ln_ref(_dw_pre(x, w, b, dil, dt), gamma, beta, 1e-5, ACT_GELU, None, m, dt))
                    pre = _dw_pre(x, w, b, dil, np.float64)
                    tol = _ln_tol(pre, gamma, 1e-5, refs[0], refs[1]) if C_ > 1 else None
                    y, _, stray = _ln(x, gamma, beta, 1e-5, dw=(w, b), dil=dil, mask=m)
                    assert stray == 0 and np.isfinite(y).all(), (C_, dil, L)
                    ratio = float((np.abs(y.astype(np.float64) - refs[0]) / tol).max())
                    assert ratio <= 1.0, (C_, dil, L, ratio)
                    worst = max(worst, ratio)
                    if dil == 1 and L == 100 and m is None:   # a reference without the dilation's outer taps at the edges must fail
                        bad = _ln_ref(_dw_pre(x, np.concatenate([w[:, :2], np.zeros((C_, 1), np.float32)], 1), b, dil, np.float64), gamma, beta, 1e-5, ACT_GELU, None, m, np.float64)
                        assert (np.abs(bad - refs[0]) / tol).max() > 1.0
    print(f"[dds_dw_ln_gelu C{C_} {name}] worst error / tolerance = {worst:.3f}")


@gpu
@pytest.mark.parametrize("H,V,N", [(1024, 50, 66), (192, 7, 5), (1000, 3, 1), (33, 300, 257)])
def test_deberta_embed_ln(H, V, N):
    """ids 0, the last row of the table, and a negative id (a zero column)."""
    rng = np.random.default_rng(H + N)
    emb = rng.standard_normal((V, H)).astype(np.float32)
    gamma = (1.0 + 0.3 * rng.standard_normal(H)).astype(np.float32)
    beta = (0.2 * rng.standard_normal(H)).astype(np.float32)
    ids = rng.integers(0, V, N).astype(np.int32)
    ids[0] = 0
    ids[-1] = V - 1
    if N > 2:
        ids[1] = -1
    y = np.empty((H, N), np.float32)
    stray = C.c_int64(-1)
    _lib.check(_lib.lib().sbv2_debug_deberta_embed_ln(0, _i32(ids), _f(emb), V, H, _f(gamma), _f(beta), 1e-7, N, 1, _f(y), C.byref(stray)))
    assert stray.value == 0
    x = emb[np.maximum(ids, 0)].T
    keep = (ids >= 0).astype(np.uint8)
    ref, ref32 = (_ln_ref(x, gamma, beta, 1e-7, ACT_NONE, None, keep, dt) for dt in (np.float64, np.float32))
    tol = _ln_tol(x, gamma, 1e-7, ref, ref32)
    assert _report(f"deberta_embed_ln H{H} N{N}", np.abs(y - ref), tol) <= 1.0
    assert (y[:, ids < 0] == 0).all()
    bad = _ln_ref(x, gamma, beta, 1e-7, ACT_NONE, None, keep, np.float64, ddof=1)
    assert (np.abs(bad - ref) / tol).max() > 1.0


# ---- GPU: the duration flow's pieces ------------------------------------------------------------------------------------------------------------------

def _spline(P, z, mask, inv, poison=1):
    P, z, mask = _c32(P), _c32(z), _u8(mask)
    out = np.empty_like(z)
    stray = C.c_int64(-1)
    _lib.check(_lib.lib().sbv2_debug_spline_inverse(0, _f(P), _f(z), mask.ctypes.data, z.shape[1], 10, 5.0, inv, poison, _f(out), C.byref(stray)))
    return out, stray.value


@gpu
def test_spline_inverse_golden(golden_dir):
    """The kernel on the transformers vectors of tests/golden/spline_inverse.npz (y is transformers' float32 output: its own error is one more err32)."""
    g = np.load(os.path.join(golden_dir, "spline_inverse.npz"))
    P = np.concatenate([g["uw"].T, g["uh"].T, g["ud"].T], axis=0)
    z = np.stack([np.arange(64, dtype=np.float32), g["x"]])
    out, stray = _spline(P, z, np.ones(64, np.uint8), 1.0)
    assert stray == 0
    np.testing.assert_array_equal(out[0], z[0])
    r64 = O.rq_spline_inverse(g["x"].astype(np.float64), g["uw"].astype(np.float64), g["uh"].astype(np.float64), g["ud"].astype(np.float64), 5.0)
    err32 = float(np.abs(O.rq_spline_inverse(g["x"], g["uw"], g["uh"], g["ud"], 5.0) - r64).max())
    tol = max(4 * err32, SPLINE_FLOOR) + err32
    assert _report("spline golden", np.abs(out[1].astype(np.float64) - g["y"]), tol) <= 1.0
    outside = np.abs(g["x"]) > 5
    np.testing.assert_array_equal(out[1][outside], g["x"][outside])


@gpu
def test_spline_inverse_constructed():
    """x across the interval, exactly +-tail and one float either side (outside: returned bit for bit), on every float64 knot, saturated bin softmaxes,
    derivative logits around the softplus cut, masked columns (both rows come back 0)."""
    cases, inv = _spline_cases(3)
    for name, (P, z1) in cases.items():
        T = z1.shape[0]
        rng = np.random.default_rng(T)
        mask = (rng.random(T) > 0.1).astype(np.uint8)
        if name in ("tails", "knots"):
            mask[:] = 1
            mask[-1] = 0
        z = np.stack([rng.standard_normal(T).astype(np.float32), z1])
        Pp = P.copy()
        Pp[:, mask == 0] = np.nan   # nothing of a masked column may be used
        out, stray = _spline(Pp, z, mask, float(inv))
        assert stray == 0, name
        m = mask.astype(bool)
        assert (out[:, ~m] == 0).all(), name
        np.testing.assert_array_equal(out[0][m], z[0][m])
        ref = _spline_ref(P, z1, inv, np.float64)
        tol = max(4 * float(np.abs(_spline_ref(P, z1, inv, np.float32) - ref).max()), SPLINE_FLOOR)
        assert np.isfinite(out[1][m]).all(), name
        assert _report(f"spline {name}", np.abs(out[1].astype(np.float64) - ref)[m], tol) <= 1.0, name
        outside = m & ~((z1 >= -5) & (z1 <= 5))
        np.testing.assert_array_equal(out[1][outside], z1[outside])
        if name == "tails":
            assert outside.sum() >= 4 * 7 and (m & ~outside).sum() >= 4 * 7


@gpu
@pytest.mark.parametrize("ratio,ls", DUR_CASES)
def test_durations(ratio, ls):
    """dur = ceil(exp(lw) * length_scale), lw = sdp * ratio + dp * (1 - ratio), against float64 from the f32 inputs.

    The window of undecidable elements.  In f32 the kernel forms a = sdp * ratio, b = dp * (1 - ratio) and their sum: three roundings, each at most
    2^-24 relative to its own result, so |lw32 - lw| <= dlw = 2^-24 (|a| + |b| + |lw|) (a fused multiply-add only removes one of them; ratio is 0, 0.5
    or 1, so ratio and 1 - ratio are exact).  expf is documented at 1 ulp (<= 2^-23 relative), the product with length_scale rounds once more (2^-24).
    The f32 product therefore lies within p (e^dlw - 1 + 2^-23 + 2^-24) of the float64 product p, times 1.01 for the second-order terms.  An element
    whose p is that close to an integer is undecidable: it may differ from the reference by at most 1 and is left out of the exact comparison; at most
    0.1 % of a case may be left out (checked on the reference alone in the CPU part)."""
    sdp, dp, mask = _dur_inputs(int(ratio * 10 + ls * 100))
    L = sdp.shape[0]
    logw, dur = np.empty(L, np.float32), np.empty(L, np.int32)
    stray = C.c_int64(-1)
    _lib.check(_lib.lib().sbv2_debug_durations(0, _f(sdp), _f(dp), mask.ctypes.data, L, ratio, ls, _f(logw), _i32(dur), C.byref(stray)))
    assert stray.value == 0
    lw, dlw, p, w = _dur_window(sdp, dp, ratio, ls)
    m = mask.astype(bool)
    assert (dur[~m] == 0).all() and (logw[~m] == 0).all()
    assert (np.abs(logw.astype(np.float64) - lw)[m] <= dlw[m] + 1e-45).all()
    ref = np.ceil(p).astype(np.int64)
    undec = np.abs(p - np.round(p)) <= w
    print(f"[durations ratio {ratio} length_scale {ls}] undecidable elements: {int((undec & m).sum())} of {int(m.sum())}")
    assert (undec & m).sum() <= 1e-3 * m.sum()
    np.testing.assert_array_equal(dur[m & ~undec], ref[m & ~undec])
    assert (np.abs(dur.astype(np.int64) - ref)[m & undec] <= 1).all()


@gpu
def test_durations_exact_cases():
    z, one = np.zeros(5, np.float32), np.ones(5, np.uint8)
    for ls, want in ((0.5, 1), (1.0, 1), (1.3, 2), (2.0, 2)):
        for ratio in (0.0, 0.5, 1.0):
            logw, dur = np.empty(5, np.float32), np.empty(5, np.int32)
            _lib.check(_lib.lib().sbv2_debug_durations(0, _f(z), _f(z), one.ctypes.data, 5, ratio, ls, _f(logw), _i32(dur), None))
            assert (dur == want).all() and (logw == 0).all(), (ls, ratio, dur)


@gpu
@pytest.mark.parametrize("L", [1, 255, 256, 257, 1000])
def test_affine_reverse_and_convflow_pre(L):
    rng = np.random.default_rng(L)
    z = rng.standard_normal((2, L)).astype(np.float32)
    mask = (rng.random(L) > 0.2).astype(np.uint8)
    mask[0] = 1
    m2, logs = np.array([0.3, -0.7], np.float32), np.array([0.4, -1.1], np.float32)
    scale = np.exp(-logs.astype(np.float64)).astype(np.float32)
    for form in ("logs", "scale"):
        out = np.empty_like(z)
        stray = C.c_int64(-1)
        _lib.check(_lib.lib().sbv2_debug_affine_reverse(0, _f(z), _f(m2), _f(logs) if form == "logs" else None, None if form == "logs" else _f(scale),
                                                        mask.ctypes.data, L, _f(out), C.byref(stray)))
        assert stray.value == 0
        if form == "scale":   # exact in f32
            np.testing.assert_array_equal(out, (z - m2[:, None]) * scale[:, None] * mask[None, :].astype(np.float32))
        else:
            ref = (z.astype(np.float64) - m2[:, None]) * np.exp(-logs.astype(np.float64))[:, None] * mask[None, :]
            ref32 = (z - m2[:, None]) * np.exp(-logs)[:, None] * mask[None, :].astype(np.float32)
            tol = max(4 * float(np.abs(ref32 - ref).max()), 8 * EPS32 * max(1.0, float(np.abs(ref).max())))
            assert _report(f"affine_reverse logs L{L}", np.abs(out - ref), tol) <= 1.0
            assert (out[:, mask == 0] == 0).all()
    Cc = 37
    w, b = rng.standard_normal(Cc).astype(np.float32), rng.standard_normal(Cc).astype(np.float32)
    cond = rng.standard_normal((Cc, L)).astype(np.float32)
    condp = cond.copy()
    condp[:, mask == 0] = np.nan
    z0 = np.where(mask, z[0], np.float32(np.nan)).astype(np.float32)
    out = np.empty((Cc, L), np.float32)
    stray = C.c_int64(-1)
    _lib.check(_lib.lib().sbv2_debug_convflow_pre(0, _f(z0), _f(w), _f(b), _f(condp), mask.ctypes.data, Cc, L, _f(out), C.byref(stray)))
    assert stray.value == 0
    ref = (w.astype(np.float64)[:, None] * z[0][None, :] + b[:, None] + cond) * mask[None, :]
    ref32 = (w[:, None] * z[0][None, :] + b[:, None] + cond) * mask[None, :].astype(np.float32)
    tol = max(4 * float(np.abs(ref32 - ref).max()), 8 * EPS32 * max(1.0, float(np.abs(ref).max())))
    assert _report(f"convflow_pre L{L}", np.abs(out - ref), tol) <= 1.0
    assert (out[:, mask == 0] == 0).all()
    assert np.abs((w.astype(np.float64)[:, None] * z[1][None, :] + b[:, None] + cond) * mask[None, :] - ref).max() > tol   # the other row of z


# ---- GPU: noise ---------------------------------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("kind,lens,seg_utt", [(TEXT, [5, 9, 3, 257], [2, 0, 3, 1]), (TEXT, [1], [6]), (FRAMES, [300, 31, 1025], [1, 2, 0])])
def test_noise_fill(kind, lens, seg_utt):
    """noise_fill against synth.hash_normal(noise_key(seed, seg_utt[segment], stream), rows * len)[row * len + t]: several segments, seg_utt a permutation
    that is not the identity, both streams, 2 and 3 rows; scale 1 and 0.6: bit-identical (the count of samples that are not is printed before the assertion);
    scale 0: zeros; gap columns: zeros."""
    start, L = _layout(lens, kind)
    ln, su = np.asarray(lens, np.int64), np.asarray(seg_utt, np.int32)
    inside = _seg_of(lens, start, L) >= 0
    for rows, stream, seed, scale in ((2, 0, 1234, 1.0), (3, 1, 2 ** 63 + 5, 1.0), (2, 0, 77, 0.6), (2, 1, 77, 0.0)):
        y = np.empty((rows, L), np.float32)
        stray = C.c_int64(-1)
        _lib.check(_lib.lib().sbv2_debug_noise_fill(0, _i64(ln), len(lens), kind, _i32(su), seed, stream, scale, rows, _f(y), C.byref(stray)))
        assert stray.value == 0
        ref = _noise_ref(lens, start, L, seg_utt, seed, stream, rows) * np.float32(scale)
        assert (y[:, ~inside] == 0).all()
        if scale == 0.0:
            assert (y == 0).all()
            continue
        ulps = np.abs(y.astype(np.float64) - ref) / np.spacing(np.abs(ref)).astype(np.float64)
        nd = int((y != ref).sum())
        print(f"[noise_fill {lens} rows {rows} stream {stream} scale {scale}] not bit-identical: {nd} of {int(inside.sum()) * rows}, worst {ulps.max():.2f} ulp")
        np.testing.assert_array_equal(y, ref)


@gpu
def test_expand_frames():
    """expand_frames: z = m_p[tok] + hash_normal(key(seed, seg_utt, 1))[c * len + t] * noise_scale * exp(logs_p[tok]); noise_scale 0 is a pure gather (bit
    exact); tok_of_frame -1 (gaps, and one frame inside an utterance) gives 0."""
    rng = np.random.default_rng(9)
    Cc, tlens, flens, seg_utt, seed = 5, [4, 7, 2], [37, 300, 2], [2, 0, 1], 99
    tstart, Lt = _layout(tlens, TEXT)
    fstart, Lf = _layout(flens, FRAMES)
    m_p = rng.standard_normal((Cc, Lt)).astype(np.float32)
    logs_p = (0.5 * rng.standard_normal((Cc, Lt))).astype(np.float32)
    tok = np.full(Lf, -1, np.int32)
    for u in range(3):
        tok[fstart[u]:fstart[u] + flens[u]] = tstart[u] + np.sort(rng.integers(0, tlens[u], flens[u]))
    tok[fstart[1] + 5] = -1
    ln, su = np.asarray(flens, np.int64), np.asarray(seg_utt, np.int32)
    noise = _noise_ref(flens, fstart, Lf, seg_utt, seed, 1, Cc)
    for ns in (0.0, 0.667):
        y = np.empty((Cc, Lf), np.float32)
        stray = C.c_int64(-1)
        _lib.check(_lib.lib().sbv2_debug_expand_frames(0, _f(m_p), _f(logs_p), Cc, Lt, _i32(tok), _i64(ln), 3, _i32(su), seed, ns, _f(y), C.byref(stray)))
        assert stray.value == 0
        ok = tok >= 0
        tk = np.maximum(tok, 0)
        assert (y[:, ~ok] == 0).all()
        if ns == 0.0:
            np.testing.assert_array_equal(y[:, ok], m_p[:, tk][:, ok])
            continue
        ref = (m_p[:, tk].astype(np.float64) + noise.astype(np.float64) * float(np.float32(ns)) * np.exp(logs_p[:, tk].astype(np.float64))) * ok
        ref32 = (m_p[:, tk] + noise * np.float32(ns) * np.exp(logs_p[:, tk])) * ok.astype(np.float32)
        tol = max(4 * float(np.abs(ref32 - ref).max()), 8 * EPS32 * max(1.0, float(np.abs(ref).max())))
        assert _report("expand_frames", np.abs(y - ref), tol) <= 1.0
        wrong = _noise_ref(flens, fstart, Lf, seg_utt, seed, 1, Cc, row_stride_is_L=True)
        bad = (m_p[:, tk].astype(np.float64) + wrong.astype(np.float64) * float(np.float32(ns)) * np.exp(logs_p[:, tk].astype(np.float64))) * ok
        assert np.abs(bad - ref).max() > tol


# ---- GPU: the generator tail --------------------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("cl,Cc,k", [(0, 32, 7), (1, 16, 7), (1, 8, 3), (1, 8, 11), (1, 32, 3), (1, 32, 7), (1, 32, 11), (0, 5, 3)],
                         ids=lambda v: str(v))
def test_conv_post_tanh(cl, Cc, k):
    """conv_post_tanh (cl = 0) and conv_post_tanh_cl (cl = 1; 16 channels x 7 taps is the compiled-size instance, the others the generic one) on several
    utterances in one plane with the decoder's frame gap: up = 1 with lengths that end 1 before, on and 1 after a 256-sample workgroup border (the first
    utterance starts at column 0), and the full model's total upsampling factor with short utterances.  The reference convolves the whole gapped plane
    (gaps are zeros, as in the decoder) and gathers the utterances.  Some columns are scaled so that |a| > 10 (tanh's ends).  make_layout always leaves at
    least the gap behind the last utterance, so 'the last one ends at L' cannot be built with the models' layout; the plane's end is reached by the halo of
    the last workgroup only through zero columns."""
    up_full = O.hop_length(O.VITS_FULL)
    worst = 0.0
    for up, lens in ((1, [255, 256, 257, 1, 511, 513]), (1, [3]), (up_full, [1, 2, 3])):
        rng = np.random.default_rng(Cc * 100 + k + up)
        start, Lf = _layout(lens, FRAMES)
        L = Lf * up
        inside = np.repeat(_seg_of(lens, start, Lf) >= 0, up)
        x = rng.standard_normal((Cc, L)).astype(np.float32)
        x[:, rng.random(L) < 0.05] *= 40.0
        x[:, ~inside] = 0.0
        w = (0.05 * rng.standard_normal((Cc, k))).astype(np.float32)
        ln = np.asarray(lens, np.int64)
        pcm = np.empty(int(ln.sum()) * up, np.float32)
        stray = C.c_int64(-1)
        _lib.check(_lib.lib().sbv2_debug_conv_post_tanh(0, _f(x), _f(w), Cc, k, _i64(ln), len(lens), up, cl, _f(pcm), C.byref(stray)))
        assert stray.value == 0
        gather = np.concatenate([np.arange(s * up, (s + n) * up) for s, n in zip(start, lens)])
        a64 = _conv_post_ref(x, w, np.float64)
        ref, ref32 = a64[gather], _conv_post_ref(x, w, np.float32)[gather]
        tol = max(4 * float(np.abs(ref32 - ref).max()), 8 * EPS32)
        assert (len(lens) == 1 or (np.abs(ref) > 0.9999).any()) and np.isfinite(pcm).all()
        worst = max(worst, _report(f"conv_post cl{cl} C{Cc} k{k} up{up}", np.abs(pcm - ref), tol))
        assert np.abs(_conv_post_ref(x, w, np.float64, shift=1)[gather] - ref).max() > tol
    assert worst <= 1.0


# ---- GPU: movers and small ops ------------------------------------------------------------------------------------------------------------------------

def _plane_op(op, x, a=0, b=0, map_=None, out_shape=None):
    x = _c32(x)
    y = np.empty(out_shape, np.float32)
    mo = np.zeros(max(b, 1), np.uint8)
    stray = C.c_int64(-1)
    _lib.check(_lib.lib().sbv2_debug_plane_op(0, op, _f(x), x.shape[0], x.shape[1], None if map_ is None else _i32(map_), a, b, _f(y), mo.ctypes.data,
                                              C.byref(stray)))
    assert stray.value == 0, (op, a, b)
    return y, mo


@gpu
def test_plane_movers():
    rng = np.random.default_rng(1)
    for Cc, L in ((5, 300), (33, 70), (1, 1), (64, 257)):
        x = rng.standard_normal((Cc, L)).astype(np.float32)
        # gather_cols: map with -1
        for Lo in (1, 255, 257):
            mp = rng.integers(-1, L, Lo).astype(np.int32)
            mp[0] = -1
            mp[-1] = L - 1 if Lo > 1 else -1
            y, _ = _plane_op(0, x, a=Lo, map_=mp, out_shape=(Cc, Lo))
            np.testing.assert_array_equal(y, np.where(mp[None, :] >= 0, x[:, np.maximum(mp, 0)], np.float32(0)))
        # transpose_out: C and T not multiples of 32, col0 > 0
        for col0, T in ((0, L), (3, L - 3), (1, 1)):
            if T < 1 or col0 + T > L:
                continue
            y, _ = _plane_op(1, x, a=col0, b=T, out_shape=(T, Cc))
            np.testing.assert_array_equal(y, x[:, col0:col0 + T].T)
        # window_cols: col0 negative, straddling the end, entirely outside on both sides
        for col0, W in ((-7, 40), (L - 5, 64), (L + 3, 9), (-300, 256), (0, L), (-1, L + 2)):
            y, mo = _plane_op(2, x, a=col0, b=W, out_shape=(Cc, W))
            q = col0 + np.arange(W)
            ok = (q >= 0) & (q < L)
            np.testing.assert_array_equal(y, np.where(ok[None, :], x[:, np.clip(q, 0, L - 1)], np.float32(0)))
            np.testing.assert_array_equal(mo, ok.astype(np.uint8))
        y, _ = _plane_op(3, x, out_shape=(Cc, L))   # flip_channels (odd C among them)
        np.testing.assert_array_equal(y, x[::-1])
    for L in (1, 255, 256, 257):
        x = rng.standard_normal((2, L)).astype(np.float32)
        y, _ = _plane_op(4, x, out_shape=(2, L))
        np.testing.assert_array_equal(y, x[::-1])


@gpu
def test_copy_segments():
    """Source / destination offsets of every residue mod 4 in combination, lengths 0, 1, 3, 4, 5, 67 and one above 64 x 1024 (the grid-stride loop turns);
    what no segment covers keeps its contents."""
    rng = np.random.default_rng(2)
    big = 64 * 1024 + 1029
    table, so, do = [], 0, 0
    lens = [0, 1, 3, 4, 5, 67]
    i = 0
    for a in range(4):
        for b in range(4):
            n = lens[i % len(lens)]
            i += 1
            so = (so + 3) // 4 * 4 + a
            do = (do + 3) // 4 * 4 + b
            table.append((so, do + 2, n))
            so += n
            do += n + 3
    for a, b in ((0, 0), (1, 1), (2, 3)):
        so = (so + 3) // 4 * 4 + a
        do = (do + 3) // 4 * 4 + b
        table.append((so, do + 2, big))
        so += big
        do += big + 3
    src = rng.standard_normal(so + 8).astype(np.float32)
    dst0 = rng.standard_normal(do + 16).astype(np.float32)
    dst = dst0.copy()
    tab = np.asarray(table, np.int64)
    _lib.check(_lib.lib().sbv2_debug_copy_segments(0, _f(src), src.size, _i64(tab), len(table), _f(dst), dst.size))
    want = dst0.copy()
    for s, d, n in table:
        want[d:d + n] = src[s:s + n]
    np.testing.assert_array_equal(dst, want)
    assert {(s % 4, d % 4) for s, d, _ in table} == {(a, b) for a in range(4) for b in range(4)}


@gpu
def test_segment_vector_ops():
    """add_segvec (div 1 and 4, gap columns, masked columns, with and without a mask), add_segvec_cl, gather_rows, text_embed (gap columns give 0, the last
    row of every table), all exact in f32."""
    rng = np.random.default_rng(3)
    lens = [5, 9, 3, 66]
    n = len(lens)
    ln = np.asarray(lens, np.int64)
    tm = (rng.random(sum(lens)) > 0.25).astype(np.uint8)
    for kind, div, Cc, use_mask, cl in ((TEXT, 1, 7, 1, 0), (TEXT, 1, 7, 0, 0), (FRAMES, 4, 3, 1, 0), (FRAMES, 4, 3, 0, 0), (FRAMES, 1, 16, 1, 1), (TEXT, 1, 4, 1, 1),
                                        (FRAMES, 1, 260, 1, 0)):
        start, Ll = _layout(lens, kind)
        seg = _seg_of(lens, start, Ll)
        mask = np.zeros(Ll, bool)
        mask[seg >= 0] = tm.astype(bool)
        x = rng.standard_normal((Cc, Ll * div)).astype(np.float32)
        vec = rng.standard_normal((n, Cc)).astype(np.float32)
        y = np.empty_like(x)
        stray = C.c_int64(-1)
        _lib.check(_lib.lib().sbv2_debug_add_segvec(0, _f(x), _f(vec), Cc, _i64(ln), n, kind, div, tm.ctypes.data, use_mask, cl, _f(y), C.byref(stray)))
        assert stray.value == 0
        sg = np.repeat(seg, div)
        keep = (sg >= 0) & (np.repeat(mask, div) if use_mask else True)
        want = np.where(keep[None, :], x + vec[np.maximum(sg, 0)].T, np.float32(0))
        np.testing.assert_array_equal(y, want, err_msg=str((kind, div, Cc, use_mask, cl)))
    for V, K, B in ((5, 1, 1), (9, 255, 3), (9, 257, 4)):
        table = rng.standard_normal((V, K)).astype(np.float32)
        idx = rng.integers(0, V, B).astype(np.int32)
        idx[0] = V - 1
        y = np.empty((B, K), np.float32)
        _lib.check(_lib.lib().sbv2_debug_gather_rows(0, _f(table), V, K, _i32(idx), B, _f(y)))
        np.testing.assert_array_equal(y, table[idx])
    for H in (192, 5, 66):
        start, Ll = _layout(lens, TEXT)
        seg = _seg_of(lens, start, Ll)
        nph, ntone, nlang = 11, 4, 3
        emb, te, le = (rng.standard_normal((v, H)).astype(np.float32) for v in (nph, ntone, nlang))
        ph, tn, lg = (rng.integers(0, v, Ll).astype(np.int32) for v in (nph, ntone, nlang))
        ph[start[0]], tn[start[0]], lg[start[0]] = nph - 1, ntone - 1, nlang - 1
        for a in (ph, tn, lg):
            a[seg < 0] = 2 ** 30   # symbols of gap columns are never used
        bp = rng.standard_normal((H, Ll)).astype(np.float32)
        sp = rng.standard_normal((n, H)).astype(np.float32)
        scale = np.float32(np.sqrt(np.float32(H)))
        y = np.empty((H, Ll), np.float32)
        stray = C.c_int64(-1)
        _lib.check(_lib.lib().sbv2_debug_text_embed(0, _i32(ph), _i32(tn), _i32(lg), _i64(ln), n, _f(emb), nph, _f(te), ntone, _f(le), nlang, _f(bp), _f(sp),
                                                    float(scale), H, _f(y), C.byref(stray)))
        assert stray.value == 0
        ok = seg >= 0
        s0 = np.maximum(seg, 0)
        want = ((((emb[np.where(ok, ph, 0)].T + te[np.where(ok, tn, 0)].T) + le[np.where(ok, lg, 0)].T) + bp) + sp[s0].T) * scale
        np.testing.assert_array_equal(y, np.where(ok[None, :], want, np.float32(0)))


@gpu
@pytest.mark.parametrize("K", [1, 63, 64, 65, 256])
def test_linear_vec(K):
    """M not a multiple of 4, with and without bias; max(4 err32, 8 ulp of the output's scale); a reference that drops the last term must fail."""
    rng = np.random.default_rng(K)
    worst = 0.0
    for M, B in ((7, 3), (1, 1), (194, 2)):
        W = rng.standard_normal((M, K)).astype(np.float32)
        bias = rng.standard_normal(M).astype(np.float32)
        v = rng.standard_normal((B, K)).astype(np.float32)
        for bb in (bias, None):
            y = np.empty((B, M), np.float32)
            _lib.check(_lib.lib().sbv2_debug_linear_vec(0, _f(W), _f(bb), M, K, _f(v), B, _f(y)))
            ref = v.astype(np.float64) @ W.astype(np.float64).T + (0 if bb is None else bb.astype(np.float64))
            ref32 = v @ W.T + (np.float32(0) if bb is None else bb)
            tol = max(4 * float(np.abs(ref32 - ref).max()), 8 * EPS32 * max(1.0, float(np.abs(ref).max())))
            worst = max(worst, float(np.abs(y - ref).max()) / tol)
            bad = v[:, :K - 1].astype(np.float64) @ W[:, :K - 1].astype(np.float64).T + (0 if bb is None else bb.astype(np.float64))
            assert np.abs(bad - ref).max() > tol
    print(f"[linear_vec K{K}] worst error / tolerance = {worst:.3f}")
    assert worst <= 1.0
