"""The HiFi-GAN decoder's ResBlock kernels (csrc/conv_cl.hip, conv_clx.hip, respair_cl.hip, respair_clx.hip, respair_x16.hip, resbranch_clx.hip) launch by
launch through sbv2_debug_respair, sbv2_debug_resbranch (/ _ys), sbv2_debug_conv1d_cl, sbv2_debug_conv1d_clx and sbv2_debug_conv_transpose1d_clx, against float64
numpy statements of the same operations: at lengths on and beside every launcher's tile edge, with the column masks of the decoder (mask[pos >> shift],
mask_div = the stage's upsampling factor) and with inputs that name a wrong tap, channel or tile (impulses, channel scales 2^-10 .. 2^10, all-negative
activations) beside dense normal data.

References.  PLAIN: the kernels' headers in float64 (respair_cl.hip line 3: y' = beta (conv2(lrelu(mask (conv1(lrelu(y), d) + b1))) + b2 + y) [+ previous],
then the column mask; three such steps for a branch; conv1d "same"; ConvTranspose1d with pre-activation), cross-checked against oracle/sbv2_oracle.py.
SPLIT RESTATEMENT: the same chain with the arithmetic the kernels are specified to do.  The device rule (respair_cl.hip store_x, conv_clx.hip k_split_cl and
epilogue; decoder_cl.cpp pack_cl for the weights): a = lrelu(v) in float32 with the float slope 0.1f, hi = bf16(a) round to nearest even, lo = bf16(a - hi)
(the subtraction is exact in float32); a product is hi hi + hi lo + lo hi (lo lo dropped), each exact, summed here in float64; the intermediate is rounded to
float32, activated, masked and split again; the epilogue is ((sum + b2) + y) beta [+ previous], masked.  What remains between it and a correct kernel is
float32 accumulation and epilogue rounding.

Tolerances (derived; nothing measured on the kernels enters; every family prints its worst error / tolerance ratio):
- against the split restatement: A(v) = max(4 |v32 - v64|_max, 8 ulp of |v64|_max), v32 the same restatement with float32 accumulation.  One convolution:
  A(y).  Fused step: A(y) + |beta| max_co sum |w2| A(t), t the intermediate before activation.  A chain of steps (a branch compared directly): E_q = own_q +
  (1 + max sum|w1_q| max sum|w2_q|) E_{q-1}: with the decoder-like weights (sum |w| about 10) that gain is 100 per step and the bound says nothing, so chains
  are compared directly only on LOW-GAIN weights (sum |w| = 1 per output channel: gain 2 per step); on decoder-like weights a chain is held step by step (each
  fused step against the restatement evaluated on the plane the previous launch returned) and by the bit-equality relations below.  The wide stages' conv_clx
  chain returns every step's plane and parts through sbv2_debug_resbranch_ys for this, as the C <= 64 branches are rerun step by step.
- against the plain reference (single convolutions): the GEMM module's C_BF16X3 sum |w| |x| + 4 err32.
- parts outputs (ys), per element: |ys - lrelu(y)| <= (2^-16 + 2^-24) |lrelu(y)| + floor (_split_bound) on the plane the same launch returned.
- exact: masked columns are zero; respair_clx = respair_cl bit for bit at C = 32 / 64; the default step kernel too at k = 3; the fused branch = three default
  steps (C <= 64) = six conv_cl launches (C >= 32, k = 3; at C <= 64 only where nothing accumulates: there beta * sum + previous is one fma in the fused
  kernels, product then sum in conv_cl.hip); conv_clx's residual epilogue = ((y + r) beta) of its own plain result.
Wrong references that must exceed the tolerance of their case by 2x on the CPU (test_wrong_references_exceed_the_tolerance): one lo part dropped (four
places), neighbouring taps swapped, conv1's dilation off by one, two input channels of a chunk swapped, the intermediate not masked, the residual added after
beta, accumulate ignored, slope 0.01, a tile edge that reads its left halo as zero; for the transposed convolution two phases swapped and a tap off by one.

Lengths: 1, the one-sided halo, nto - 1, nto, nto + 1, 2 nto, 8 nto, 8 nto + 1, 17 nto + 3 for the nto (outputs per workgroup) of every kernel a case
reaches (at C = 64 both respair_cl's 256-position and the other step kernels' 128-position tiles): grids are rounded up to 8 workgroups in XCD-contiguous
order, so 1, 8, 9 and 18 tiles.  The phased transposed convolution takes whole tiles only, so its list starts at 256 (255 is asserted refused).  The wide
stages' chain runs the whole list at every C, k; from eight tiles on a length is a parametrised case of its own and runs the masked data in both epilogue
modes, the unmasked run only where the mask leaves few columns.  The nto mirrors below are checked against the sources.
Masks: "a masked run that ends exactly on a tile edge" needs a unit edge that is also a tile edge inside N: always at mask_div 1 and 4, at the decoder's
mask_div only where a multiple of nto is one of the unit (conv_clx's 256-position tiles at 8 / 64; none at 128 .. 512 within these lengths); elsewhere the
pattern is a run from 0 that ends on the unit edge at or before the first tile edge, or straddles it.

Measured worst error / tolerance ratios on an MI355X (every masked column zero, every bit-equality relation held, the accumulation factor 4 everywhere):
fused step (nine C, k cases) respair_cl 0.07 .. 0.25, default dispatch 0.07 .. 0.35, respair_clx 0.07 .. 0.35 (the largest at C = 16, k = 3, all-negative
input); the branch's steps one by one 0.16 .. 0.33; the low-gain chain 0.04 .. 0.07 for every variant of the branch; the wide stages' conv_clx chain
(variant 3, all six C, k cases at 1 .. 18 tiles) 0.02 .. 0.05 on low-gain weights, 0.01 .. 0.02 of the summed tolerances from the conv_cl chain, and step by
step on decoder-like weights 0.03 .. 0.06; conv_cl 0.24 .. 0.77 against the restatement (the largest at 256 -> 256, k = 3) and 0.15 .. 0.21 against the plain
reference; conv_clx 0.46 .. 0.69 and 0.18 .. 0.25; the phased transposed convolution 0.46 .. 0.53 and 0.21 .. 0.26.  No case takes more than 3.1 s.

Found while writing it: with beta * sum + previous contents the fused kernels of C <= 64 and the six conv_cl launches are one ulp apart (2.4e-7 at C = 32):
one fma against product then sum.  The older test asserts that relation only where nothing accumulates (and at C = 128, where it holds); so does this one.
"""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import sbv2_oracle as O
from sbv2_api_amd import _lib
from test_gemm_conv_kernels import C_BF16X3, EPS32, _bf16_parts, _Prof
from test_ops_kernels import _report, _split_bound

gpu = pytest.mark.gpu
f32p, i64p = _lib.f32p, _lib.i64p
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sbv2-api_amd", "csrc")
SLOPE = float(np.float32(0.1))                      # the kernels' slope is the float 0.1f
BETA3 = float(np.float32(1.0 / 3.0))
DECODER_U = {256: 8, 128: 64, 64: 128, 32: 256, 16: 512}   # mask_div of the stage with C channels (upsampling rates 8, 8, 2, 2, 2)
HOOKS = ["sbv2_debug_respair", "sbv2_debug_resbranch", "sbv2_debug_resbranch_ys", "sbv2_debug_conv1d_cl", "sbv2_debug_conv1d_clx",
         "sbv2_debug_conv_transpose1d_clx"]
KINDS = ("normal", "scales", "negative", "impulse")
PATTERNS = ("all_kept", "all_masked", "run_to_edge", "straddle", "one_kept")


# ---- the launchers' tiles, mirrored (test_mirrors_match_the_sources holds them to the sources) ---------------------------------------------------------------

def nto_respair_cl(C_, k):
    return 256 - (k - 1)                               # respair_cl.hip: kRpNT = 256; nto = kRpNT - 2 * h2


def nto_respair_clx(C_, k):
    return (128 if C_ == 64 else 256) - (k - 1)        # respair_clx.hip RpxCfg: WN = C == 64 ? 2 : 4, NT = 64 * WN; launch_rpx: nto = K::NT - (NTAPS - 1)


def nto_respair_x16(C_, k):
    return (128 if C_ == 64 else 256) - (k - 1)        # respair_x16.hip X6Cfg: WN = C == 64 ? 2 : 4, NT = 64 * WN; launch_x6: nto = K::NT - (NTAPS - 1)


def respair_x16_usable(C_, k, dil):
    return C_ in (32, 64) and k in (7, 11) and dil >= 1 and dil * (k - 1) <= 64


def respair_clx_usable(C_, k, dil):
    return C_ in (16, 32, 64) and k in (3, 7, 11) and dil >= 1 and dil * (k - 1) <= 64


def respair_default(C_, k, dil):
    """respair_cl.hip respair_default: the kernel variant 1 of sbv2_debug_respair runs"""
    return "x16" if respair_x16_usable(C_, k, dil) else ("clx" if respair_clx_usable(C_, k, dil) else "cl")


def nto_step(C_, k, variant, dil=1):
    kern = {0: "cl", 2: "clx"}.get(variant) or respair_default(C_, k, dil)
    return {"cl": nto_respair_cl, "clx": nto_respair_clx, "x16": nto_respair_x16}[kern](C_, k)


def rb_rows(C_, k):
    """resbranch_clx.hip rb_rows: window rows of the instance launch_resbranch picks (0: none)"""
    if k == 3:
        return {128: 192, 64: 384, 32: 256, 16: 256}.get(C_, 0)
    return 512 if C_ == 16 and k in (7, 11) else 0


def rb_margin(k):
    return 6 if k <= 3 else ((5 * (k - 1) // 2 + 1) & ~1)


def rb_halo(k, dils):
    return sum((d + 1) * (k - 1) // 2 for d in dils)


def resbranch_usable(C_, k, dils):
    R = rb_rows(C_, k)
    return R > 0 and all(d >= 1 and d * (k - 1) // 2 <= rb_margin(k) for d in dils) and 4 * rb_halo(k, dils) <= R


def nto_resbranch(C_, k, dils=(1, 3, 5)):
    return rb_rows(C_, k) - 2 * rb_halo(k, dils)       # launch_rb: nto = K::R - 2 * p.halo


NT_CONV = 256                                          # conv_cl.hip kClNT, conv_clx.hip kClxNT: positions per workgroup
CLX_FRONT = 64                                         # common.h kClxFront


def conv_clx_usable(cin, cout, k, dil, L=1):
    span = (k - 1) * dil
    return k in (3, 5, 7, 11) and cin % 32 == 0 and cout % 64 == 0 and span <= 64 and -(dil * (k - 1) // 2) >= -CLX_FRONT and L >= 1


def upx_usable(cin, cout, k, s, L):
    """decoder_cl.cpp build_upx + conv_clx_usable's phased rules: 2 or 4 taps per phase, whole-tile launches"""
    pad = (k - s) // 2
    if k - 2 * pad != s or not 1 <= s <= 8 or cout % 64 or cin % 32:
        return False
    per_phase = {len([j for j in range(k) if (j - r - pad) % s == 0]) for r in range(s)}
    return per_phase <= {2, 4} and len(per_phase) == 1 and L >= NT_CONV


def lengths(nto, halo):
    return sorted({1, halo, nto - 1, nto, nto + 1, 2 * nto, 8 * nto, 8 * nto + 1, 17 * nto + 3})


# ---- references ---------------------------------------------------------------------------------------------------------------------------------------------

def lrelu(v, slope=SLOPE):
    """leaky ReLU in v's own type with the float32 slope (float32 in: the device's fmaxf(v, v * slope) / select, the same value for 0 <= slope <= 1)"""
    return np.where(v >= 0, v, v * v.dtype.type(slope))


def tapsum(x, w, dil, pad_l, dt):
    """sum_ci sum_j w[co][ci][j] x[ci][n + j dil - pad_l], zero outside [0, L)"""
    cout, cin, k = w.shape
    L = x.shape[1]
    cols = np.zeros((k, cin, L), dt)                  # (one product over all taps: the taps' shifted copies of x under each other)
    for j in range(k):
        s = j * dil - pad_l
        lo, hi = max(0, -s), min(L, L - s)
        if hi > lo:
            cols[j, :, lo:hi] = x[:, lo + s:hi + s]
    return np.ascontiguousarray(w.transpose(0, 2, 1), dt).reshape(cout, k * cin) @ cols.reshape(k * cin, L)


def split_sum(a32, w32, dil, dt, drop=(), pad_l=None):
    """the split-bf16 product of an ACTIVATED float32 operand: hi hi + hi lo + lo hi, accumulated in dt.  drop: "x" / "w" leaves that operand's lo part out."""
    k = w32.shape[2]
    pad_l = dil * (k - 1) // 2 if pad_l is None else pad_l
    xh, xl = _bf16_parts(np.ascontiguousarray(a32, np.float32), 2)
    wh, wl = _bf16_parts(np.ascontiguousarray(w32, np.float32), 2)
    if np.dtype(dt) == np.float64 and not drop:       # hi hi + lo hi = (hi + lo) hi, the sum and every product exact in float64: two products for three
        return tapsum(xh.astype(np.float64) + xl, wh, dil, pad_l, dt) + tapsum(xh, wl, dil, pad_l, dt)
    y = tapsum(xh, wh, dil, pad_l, dt)
    if "x" not in drop:
        y = y + tapsum(xl, wh, dil, pad_l, dt)
    if "w" not in drop:
        y = y + tapsum(xh, wl, dil, pad_l, dt)
    return y


def plain_sum(a, w32, dil, dt=np.float64, pad_l=None):
    k = w32.shape[2]
    return tapsum(a, w32, dil, dil * (k - 1) // 2 if pad_l is None else pad_l, dt)


def _swap_taps(w, j):
    w = w.copy()
    w[:, :, [j, j + 1]] = w[:, :, [j + 1, j]]
    return w


def _swap_channels(w, a, b):
    w = w.copy()
    w[:, [a, b], :] = w[:, [b, a], :]
    return w


def step_sums(x, w1, b1, w2, k, dil, dt, keep=None, split=True, wrong=None, seam=None):
    """(t, s2): conv1's sum + b1 before activation, and conv2's sum, of one ResBlock step on x [C][N] float32.  split: the restatement (operands split, the
    intermediate rounded to float32) else the plain float64 statement.  wrong: one of the deliberately wrong references."""
    slope = 0.01 if wrong == "slope" else SLOPE
    d1 = dil + 1 if wrong == "dilation" else dil
    if wrong == "taps1":
        w1 = _swap_taps(w1, k // 2)
    if wrong == "taps2":
        w2 = _swap_taps(w2, 0)
    if wrong == "channels":
        w1 = _swap_channels(w1, 7, 8)
    drop1 = {"drop_c1x": "x", "drop_c1w": "w"}.get(wrong, "")
    drop2 = {"drop_c2t": "x", "drop_c2w": "w"}.get(wrong, "")
    if split:
        a = lrelu(x.astype(np.float32), slope)
        t = split_sum(a, w1, d1, dt, drop1) + b1.astype(dt)[:, None]
        u = lrelu(t.astype(np.float32), slope)
    else:
        t = plain_sum(lrelu(x.astype(dt), slope), w1, d1, dt) + b1.astype(dt)[:, None]
        u = lrelu(t, slope)
    if keep is not None and wrong != "mid_unmasked":
        u = u * keep.astype(u.dtype)[None, :]
    conv2 = (lambda v: split_sum(v, w2, 1, dt, drop2)) if split else (lambda v: plain_sum(v, w2, 1, dt))
    s2 = conv2(u)
    if wrong == "tile_edge" and seam is not None and 0 < seam < x.shape[1]:
        z = u.copy()
        z[:, :seam] = 0                               # the first column of the second tile reads its left halo as zero
        s2[:, seam] = conv2(z)[:, seam]
    return t, s2


def step_epilogue(s2, x, b2, dt, keep=None, beta=1.0, prev=None, wrong=None):
    """((sum + b2) + y) beta [+ previous], then the column mask (respair_cl.hip's epilogue; conv_cl's and conv_clx's order)"""
    b = dt(np.float32(beta))
    v = s2 + b2.astype(dt)[:, None]
    v = v * b + x.astype(dt) if wrong == "res_after_beta" else (v + x.astype(dt)) * b
    if prev is not None and wrong != "no_accumulate":
        v = v + prev.astype(dt)
    if keep is not None:
        v = v * keep.astype(dt)[None, :]
    return v


def step_ref(x, w1, b1, w2, b2, k, dil, dt, keep=None, beta=1.0, prev=None, split=True, wrong=None, seam=None):
    t, s2 = step_sums(x, w1, b1, w2, k, dil, dt, keep, split, wrong, seam)
    return step_epilogue(s2, x, b2, dt, keep, beta, prev, wrong), t


def acc_term(v64, v32):
    """the project's accumulation term: 4 x the float32 evaluation's deviation, and no less than 8 ulp of the scale"""
    return max(4.0 * float(np.abs(v32.astype(np.float64) - v64).max()), 8.0 * EPS32 * float(np.abs(v64).max()))


def abs_rows(w):
    return float(np.abs(w.astype(np.float64)).sum(axis=(1, 2)).max())


def step_tol(y64, y32, t64, t32, w2, beta):
    return acc_term(y64, y32) + abs(float(np.float32(beta))) * abs_rows(w2) * acc_term(t64, t32) + 1e-37


def step_case(x, w1, b1, w2, b2, k, dil, keep=None, beta=1.0, prev=None, wrong=None, seam=None):
    """(reference, tolerance) of one step against the split restatement"""
    y64, t64 = step_ref(x, w1, b1, w2, b2, k, dil, np.float64, keep, beta, prev)
    y32, t32 = step_ref(x, w1, b1, w2, b2, k, dil, np.float32, keep, beta, prev)
    return y64, step_tol(y64, y32, t64, t32, w2, beta)


def chain_cases(x, w, b, k, dils, keep=None, modes=((1.0, None),), wrong=None):
    """[(reference, tolerance)] of a branch = three steps, each step's result rounded to float32 (the plane the next step reads), compared directly, for every
    (beta, previous contents) of the last step: E_q = own_q + (1 + max sum|w1_q| max sum|w2_q|) E_{q-1}, the last step's beta on all of it.
    wrong = (step, name) puts one wrong reference into one step (the tolerance stays the right chain's)."""
    y = x.astype(np.float32)
    E = 0.0
    out = []
    for q in range(3):
        wr = wrong[1] if wrong is not None and wrong[0] == q else None
        x1, w1, b1, w2, b2 = y, w[2 * q], b[2 * q], w[2 * q + 1], b[2 * q + 1]
        t64, s64 = step_sums(x1, w1, b1, w2, k, dils[q], np.float64, keep)
        t32, s32 = step_sums(x1, w1, b1, w2, k, dils[q], np.float32, keep)
        sbad = step_sums(x1, w1, b1, w2, k, dils[q], np.float64, keep, wrong=wr)[1] if wr else s64
        gain = 1.0 + abs_rows(w1) * abs_rows(w2)
        for beta, prev in (modes if q == 2 else ((1.0, None),)):
            y64, y32 = step_epilogue(s64, x1, b2, np.float64, keep, beta, prev), step_epilogue(s32, x1, b2, np.float32, keep, beta, prev)
            tol = step_tol(y64, y32, t64, t32, w2, beta) + abs(float(np.float32(beta))) * gain * E
            ybad = step_epilogue(sbad, x1, b2, np.float64, keep, beta, prev, wr) if wr else y64
            if q == 2:
                out.append((ybad, tol))
        if q < 2:
            E = tol
            y = ybad.astype(np.float32)
    return out


def chain_case(x, w, b, k, dils, keep=None, beta=1.0, prev=None, wrong=None):
    return chain_cases(x, w, b, k, dils, keep, ((beta, prev),), wrong)[0]


def conv_case(x, w, bias, dil, pre_slope=SLOPE):
    """one convolution on lrelu(x): (restatement, its tolerance, plain reference, its tolerance)"""
    a = lrelu(x.astype(np.float32), pre_slope)
    bb = bias.astype(np.float64)[:, None]
    r64 = split_sum(a, w, dil, np.float64) + bb
    r32 = split_sum(a, w, dil, np.float32) + bias.astype(np.float32)[:, None]
    a64 = lrelu(x.astype(np.float64), pre_slope)
    p64 = plain_sum(a64, w, dil) + bb
    p32 = plain_sum(lrelu(x.astype(np.float32), pre_slope), w, dil, np.float32) + bias.astype(np.float32)[:, None]
    S = plain_sum(np.abs(a64), np.abs(w.astype(np.float64)), dil)
    return r64, acc_term(r64, r32) + 1e-37, p64, C_BF16X3 * S + 4.0 * float(np.abs(p32 - p64).max()) + 1e-37


def upconv_sum(a, w, s, dt, split=True, wrong=None):
    """ConvTranspose1d(k, stride s, padding (k - s) / 2) of an activated operand a [cin][L], w [cin][cout][k]: y[co][m s - p + j] += w[ci][co][j] a[ci][m]"""
    cin, cout, k = w.shape
    L = a.shape[1]
    p = (k - s) // 2
    parts = [(a, w)]
    if split:
        ah, al = _bf16_parts(np.ascontiguousarray(a, np.float32), 2)
        wh, wl = _bf16_parts(np.ascontiguousarray(w, np.float32), 2)
        parts = [(ah, wh), (al, wh), (ah, wl)]
    full = np.zeros((cout, (L - 1) * s + k + 2), dt)
    for pa, pw in parts:
        taps = (np.ascontiguousarray(pw.transpose(2, 1, 0), dt).reshape(k * cout, cin) @ pa.astype(dt)).reshape(k, cout, L)   # every tap's product at once
        for j in range(k):
            o = j + (1 if wrong == "tap_off_one" else 0)
            full[:, o:o + (L - 1) * s + 1:s] += taps[j]
    y = full[:, p:p + L * s].copy()
    if wrong == "phases_swapped":
        y[:, 0::s], y[:, 1::s] = y[:, 1::s].copy(), y[:, 0::s].copy()
    return y


def upconv_case(x, w, bias, s, keep=None, wrong=None):
    a = lrelu(x.astype(np.float32))
    ko = None if keep is None else np.repeat(keep, s).astype(np.float64)[None, :]
    r64 = upconv_sum(a, w, s, np.float64, wrong=wrong) + bias.astype(np.float64)[:, None]
    r32 = upconv_sum(a, w, s, np.float32) + bias.astype(np.float32)[:, None]
    a64 = lrelu(x.astype(np.float64))
    p64 = upconv_sum(a64, w, s, np.float64, split=False) + bias.astype(np.float64)[:, None]
    p32 = upconv_sum(a, w, s, np.float32, split=False) + bias.astype(np.float32)[:, None]
    S = upconv_sum(np.abs(a64), np.abs(w.astype(np.float64)), s, np.float64, split=False)
    if ko is not None:
        r64, r32, p64, p32 = r64 * ko, r32 * ko.astype(np.float32), p64 * ko, p32 * ko.astype(np.float32)
    good = r64 if wrong is None else upconv_case(x, w, bias, s, keep)[0]
    return r64, acc_term(good, r32) + 1e-37, p64, C_BF16X3 * S + 4.0 * float(np.abs(p32 - p64).max()) + 1e-37


# ---- data -------------------------------------------------------------------------------------------------------------------------------------------------

def make_x(kind, C_, N, rng, nto):
    """normal | scales (channel scales 2^-10 .. 2^10) | negative (every activation takes the slope) | impulse (zeros but for single values at positions 0, 1,
    nto - 1, nto, N - 1, in the first, a middle and the last channel of a 16-channel chunk: the response names the tap, the channel and the tile it crossed)"""
    if kind == "impulse":
        x = np.zeros((C_, N), np.float32)
        for i, pos in enumerate(sorted({p for p in (0, 1, nto - 1, nto, N - 1) if 0 <= p < N})):
            ch = (16 * i) % C_ + (0, 7, 15)[i % 3]
            x[ch, pos] = 1.0 + i / 8.0
        return x
    x = rng.standard_normal((C_, N))
    if kind == "scales":
        x = x * 2.0 ** rng.integers(-10, 11, C_)[:, None]
    if kind == "negative":
        x = -np.abs(x)
    return x.astype(np.float32)


def make_w(shape, rng, low_gain=False):
    """[..., cout, cin, k] weights: decoder-like (unit output variance) or low gain (sum |w| = 1 per output channel: a step passes an error on at most twice)"""
    w = rng.standard_normal(shape)
    if low_gain:
        w = w / np.abs(w).sum(axis=(-1, -2), keepdims=True)
    else:
        w = w / math.sqrt(shape[-1] * shape[-2])
    return w.astype(np.float32)


def make_mask(pattern, N, div, nto):
    """mask bytes [ceil(N / div)] for units of div positions, around the first tile edges of a kernel with nto outputs per workgroup.  run_to_edge ends on a
    tile edge only where a unit edge meets one inside N (always at mask_div 1 and 4): at the decoder's larger mask_div it is mostly a run from 0 that ends on
    the unit edge at or before the first tile edge, or straddles it"""
    nu = -(-N // div)
    m = np.ones(nu, np.uint8)
    edge = next((e for e in range(nto, N, nto) if e % div == 0), None)   # a tile edge that is also a unit edge
    if pattern == "all_masked":
        m[:] = 0
    elif pattern == "run_to_edge":          # a masked run that ends exactly on a tile edge (where a unit edge meets one; else on the unit edge at or before nto)
        u1 = max(1, (edge if edge is not None else min(nto, N)) // div)
        m[max(0, u1 - 2):u1] = 0
    elif pattern == "straddle":             # a masked run over a tile edge
        e = nto if nto < N else N // 2
        m[max(0, (e - 1) // div - (1 if div <= 4 else 0)):min(nu, e // div + 1 + (1 if div <= 4 else 0))] = 0
    elif pattern == "one_kept":             # one kept unit between masked ones
        m[:] = 0
        m[min(nu - 1, (nto if nto < N else N // 2) // div)] = 1
    return m


def keep_of(mask, div, N):
    return mask[np.arange(N) // div].astype(np.float32)


def plan(ci, i, C_):
    """the input kind, mask pattern and mask_div of length i of case ci: rotations that cover every combination the CPU part checks"""
    divs = (DECODER_U[C_], 1, 4)
    return KINDS[(i + ci) % 4], PATTERNS[(i + 2 * ci) % 5], divs[(i + i // 3 + ci) % 3]


STEP_CASES = [(C_, k) for C_ in (16, 32, 64) for k in (3, 7, 11)]
BRANCH_CASES = [(16, 3), (32, 3), (64, 3), (128, 3), (16, 7), (16, 11)]
ORDERS = ((1, 3, 5), (5, 1, 3))
CONV_CL_CASES = [(16, 16, 11), (32, 32, 7), (64, 64, 3), (128, 128, 7), (128, 128, 3), (256, 256, 3), (64, 32, 11)]
CONV_CLX_CASES = [(128, 128, 3), (128, 128, 11), (256, 256, 7), (128, 256, 7), (256, 128, 3)]
UPX_CASES = [(128, 64, 16, 8), (256, 128, 16, 8), (128, 64, 8, 2), (64, 128, 8, 2)]
UPX_LENGTHS = (256, 257, 511, 512, 2048, 2049, 17 * 256 + 3)   # (the phased launch takes whole tiles only: nothing below 256)
CHAIN_CASES = [(128, 3), (128, 7), (128, 11), (256, 3), (256, 7), (256, 11)]
CHAIN_GROUPS = {"to2tiles": (0, 2 * NT_CONV), "8tiles": (8 * NT_CONV, 8 * NT_CONV), "9tiles": (8 * NT_CONV + 1, 8 * NT_CONV + 1),
                "18tiles": (17 * NT_CONV + 3, 17 * NT_CONV + 3)}


def chain_lengths(C_, k, group=None):
    """[(index, N)] of a wide-stage chain case: the whole list of lengths(); a group is the part of it one parametrised case runs (the float64 restatement of
    256 channels x 11 taps x 4355 positions is 130 GFLOP, so the long lengths are cases of their own)"""
    lo, hi = CHAIN_GROUPS[group] if group else (0, 1 << 30)
    return [(i, n) for i, n in enumerate(lengths(NT_CONV, rb_halo(k, ORDERS[0]))) if lo <= n <= hi]


def chain_plan(i, C_, N):
    """the dilation order, input kind, mask_div, mask pattern of length i of a chain case, and whether the unmasked run is made beside the masked ones: always
    up to two tiles; from eight tiles on only where the mask leaves few columns (one_kept, all_masked), else the masked runs carry dense data over every tile"""
    pat = PATTERNS[(i + 2) % 5]
    return ORDERS[i % 2], KINDS[i % 4], (DECODER_U[C_], 1, 4)[i % 3], pat, N < 8 * NT_CONV or pat in ("one_kept", "all_masked")


def step_lengths(C_, k):
    ns = set(lengths(nto_step(C_, k, 1, 1), 3 * (k - 1)))
    if nto_step(C_, k, 0) != nto_step(C_, k, 1):      # C = 64: respair_cl's 256-position tiles beside the 128-position ones
        ns |= set(lengths(nto_step(C_, k, 0), 3 * (k - 1)))
    return sorted(ns)


# ---- CPU part ------------------------------------------------------------------------------------------------------------------------------------------------

def test_hooks_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "sbv2_hip.h")).read()
    l = _lib.lib()
    for name in HOOKS:
        assert re.search(r"\bint " + name + r"\(", hdr), name
        assert name in _lib.SYMBOLS and getattr(l, name).restype is C.c_int, name
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", hdr).group(1)
        assert len(decl.split(",")) == len(_lib.SYMBOLS[name][1]), name


def test_mirrors_match_the_sources():
    src = {n: open(os.path.join(CSRC, n)).read() for n in ("respair_cl.hip", "respair_clx.hip", "respair_x16.hip", "resbranch_clx.hip", "conv_cl.hip",
                                                            "conv_clx.hip", "common.h", "decoder_cl.cpp")}
    for name, texts in {
        "respair_cl.hip": ("constexpr int kRpNT = 256;", "const int nto = kRpNT - 2 * h2;", "if (respair_x16_usable(p)) return BranchKernel::respair_x16;",
                           "if (respair_clx_usable(p)) return BranchKernel::respair_clx;", "p.dil * (p.k - 1) <= 64"),
        "respair_clx.hip": ("static constexpr int WN = WNP > 0 ? WNP : (C == 64 ? 2 : 4);", "static constexpr int NT = 64 * WN;",
                            "constexpr int nto = K::NT - (NTAPS - 1);", "const int grid = ((ntiles + 7) >> 3) * 8;",
                            "(p.C == 16 || p.C == 32 || p.C == 64) && (p.k == 3 || p.k == 7 || p.k == 11) && p.dil >= 1 && p.dil * (p.k - 1) <= 64"),
        "respair_x16.hip": ("static constexpr int WN = C == 64 ? 2 : 4;", "static constexpr int NT = 64 * WN;", "constexpr int nto = K::NT - (NTAPS - 1);",
                            "const int grid = ((ntiles + 7) >> 3) * 8;", "(p.C == 32 || p.C == 64) && (p.k == 7 || p.k == 11) && p.dil >= 1 && p.dil * (p.k - 1) <= 64"),
        "resbranch_clx.hip": ("if (k == 3) return C == 128 ? 192 : (C == 64 ? 384 : ((C == 32 || C == 16) ? 256 : 0));", "if (C == 16 && (k == 7 || k == 11)) return 512;",
                              "const int nto = K::R - 2 * p.halo;", "p.halo += (p.dil[q] + 1) * (p.k - 1) / 2;", "static constexpr int R = 64 * WN;",
                              "launch_rb<128, 3, 3, 3, 2>", "launch_rb<64, 3, 6, 3, 3>", "launch_rb<32, 3, 4, 4, 3>", "launch_rb<16, 3, 4, 4, 3>", "launch_rb<16, 7, 8, 4, 3>",
                              "launch_rb<16, 11, 8, 6, 3>", "return halo * 4 <= R;", "p.dil[q] * (p.k - 1) / 2 > rb_margin(p.k)",
                              "constexpr int rb_margin(int k) { return k <= 3 ? kResBranchMargin : ((5 * (k - 1) / 2 + 1) & ~1); }",
                              "const int grid = ((ntiles + 7) >> 3) * 8;"),
        "conv_cl.hip": ("constexpr int kClNT = 256;",),
        "conv_clx.hip": ("constexpr int kClxNT = 256;", "const int ntx = round_up((p.N + kClxNT - 1) / kClxNT, 8);", "if ((p.K & 31) || (p.M & 63) || p.K != p.X.C) return false;",
                         "if (span > kClxXR - kClxNT || p.shift0 < -kClxFront || p.shift0 + span > 64) return false;", "p.Ykm || p.N < kClxNT ||"),
        "common.h": ("constexpr int kClxFront = 64;", "constexpr int kResBranchMargin = 6;", "constexpr int kResBranchSteps = 3;"),
        "decoder_cl.cpp": ("if (U != 2 && U != 4) return u;", "s > kMaxPhases || (cout & 63) || (cin & 31)) return u;"),
    }.items():
        for t in texts:
            assert t in src[name], (name, t)
    # the outputs per workgroup as read from the launchers
    assert [nto_respair_x16(64, k) for k in (7, 11)] == [122, 118] and [nto_respair_x16(32, k) for k in (7, 11)] == [250, 246]
    assert [nto_resbranch(c, 3) for c in (16, 32, 64, 128)] == [232, 232, 360, 168] and nto_resbranch(16, 7) == 440 and nto_resbranch(16, 11) == 392
    assert nto_resbranch(16, 11, (5, 1, 3)) == 392 and [nto_respair_cl(64, k) for k in (3, 7, 11)] == [254, 250, 246]
    assert [nto_respair_clx(64, k) for k in (3, 7, 11)] == [126, 122, 118] and [nto_respair_clx(16, k) for k in (3, 7, 11)] == [254, 250, 246]
    assert respair_default(32, 7, 5) == "x16" and respair_default(64, 3, 5) == "clx" and respair_default(16, 11, 5) == "clx" and respair_default(16, 11, 7) == "cl"
    assert resbranch_usable(128, 3, (1, 3, 5)) and resbranch_usable(16, 11, (5, 1, 3)) and not resbranch_usable(32, 7, (1, 3, 5))
    assert not resbranch_usable(64, 3, (1, 3, 9)) and not resbranch_usable(256, 3, (1, 3, 5))
    assert conv_clx_usable(256, 128, 11, 5) and not conv_clx_usable(128, 128, 11, 7) and not conv_clx_usable(48, 64, 3, 1)
    assert all(upx_usable(*c, 256) and not upx_usable(*c, 255) for c in UPX_CASES) and not upx_usable(128, 32, 16, 8, 256)


def test_cases_cover_the_tiles_masks_and_inputs():
    """every case's lengths hit 1, 8, 9 and 18 tiles of every kernel it reaches, on and beside the edge; the rotations reach every input kind and mask pattern
    with every mask_div class on every step kernel; a masked run that ends on a tile edge exists wherever a unit edge can meet one"""
    seen = {}
    for ci, (C_, k) in enumerate(STEP_CASES):
        ns = step_lengths(C_, k)
        for v in (0, 1, 2):
            nto = nto_step(C_, k, v)
            assert {nto - 1, nto, nto + 1, 8 * nto, 8 * nto + 1} <= set(ns) and {-(-n // nto) for n in ns} >= {1, 2, 8, 9, 18}, (C_, k, v)
        assert max(ns) * C_ <= 400000
        for i, N in enumerate(ns):
            kind, pat, div = plan(ci, i, C_)
            seen.setdefault(respair_default(C_, k, 1), set()).add((kind, pat, "decoder" if div == DECODER_U[C_] else div))
    for kern in ("clx", "x16"):
        assert {s[0] for s in seen[kern]} == set(KINDS) and {s[1:] for s in seen[kern]} >= {(p, d) for p in PATTERNS for d in ("decoder", 1, 4)}, kern
    for ci, (C_, k) in enumerate(BRANCH_CASES):
        nto = nto_resbranch(C_, k)
        ns = lengths(nto, rb_halo(k, ORDERS[0]))
        assert {-(-n // nto) for n in ns} >= {1, 2, 8, 9, 18} and max(ns) * C_ <= 400000      # (planes of at most 1.6 MB)
        assert {plan(ci, i, C_)[1] for i in range(len(ns))} == set(PATTERNS)
    for C_, k in CHAIN_CASES:
        ns = chain_lengths(C_, k)
        assert [n for _, n in ns] == lengths(NT_CONV, rb_halo(k, ORDERS[0])) and {-(-n // NT_CONV) for _, n in ns} >= {1, 2, 8, 9, 18}
        assert {255, 256, 257, 2048, 2049} <= {n for _, n in ns}
        assert sorted(ns) == sorted(sum((chain_lengths(C_, k, g) for g in CHAIN_GROUPS), [])), "a length is in no group, or in two"
        plans = [chain_plan(i, C_, n) for i, n in ns]
        assert {p[3] for p in plans} == set(PATTERNS) and {p[2] for p in plans} == {DECODER_U[C_], 1, 4} and {p[1] for p in plans} == set(KINDS)
        assert all(p[3] in ("all_kept", "run_to_edge", "straddle") or p[4] for p in plans)      # every length runs dense data
        assert any(p[2] == DECODER_U[C_] and p[3] not in ("all_masked", "one_kept") for (i, n), p in zip(ns, plans) if n >= 8 * NT_CONV)
    for conv_ns in (lengths(NT_CONV, 5), UPX_LENGTHS):
        assert {-(-n // NT_CONV) for n in conv_ns} >= {1, 2, 8, 9, 18}
    # the masks are what their names say
    for nto, div, N in ((254, 1, 600), (254, 4, 1100), (232, 8, 2000), (122, 128, 977), (360, 128, 3000)):
        for pat in PATTERNS:
            keep = keep_of(make_mask(pat, N, div, nto), div, N)
            if pat == "all_kept":
                assert keep.all()
            elif pat == "all_masked":
                assert not keep.any()
            elif pat == "straddle":
                assert not keep[nto - 1] and not keep[nto] and keep.any()
            elif pat == "one_kept":
                assert keep[nto] and keep.sum() == min(div, N - (nto // div) * div)
            else:
                z = np.flatnonzero(keep == 0)
                assert len(z) and keep[z[-1] + 1] and ((z[-1] + 1) % nto == 0 or div > 4), (nto, div)


def test_references_agree_with_the_oracle():
    rng = np.random.default_rng(11)
    x = rng.standard_normal((16, 70)).astype(np.float32)
    for k, dil in ((3, 1), (7, 3), (11, 5)):
        w = make_w((2, 16, 16, k), rng)
        b = rng.standard_normal((2, 16)).astype(np.float32)
        got = plain_sum(lrelu(x.astype(np.float64)), w[0], dil) + b[0].astype(np.float64)[:, None]
        want = O.conv1d_same(O.leaky_relu(x.astype(np.float64), SLOPE), w[0].astype(np.float64), b[0].astype(np.float64), dil)
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
        y, _ = step_ref(x, w[0], b[0], w[1], b[1], k, dil, np.float64, split=False)
        t = O.conv1d_same(O.leaky_relu(x.astype(np.float64), SLOPE), w[0].astype(np.float64), b[0].astype(np.float64), dil)
        want = O.conv1d_same(O.leaky_relu(t, SLOPE), w[1].astype(np.float64), b[1].astype(np.float64), 1) + x
        np.testing.assert_allclose(y, want, rtol=0, atol=1e-12)
        # the restatement is the plain statement up to the split's 3 * 2^-16 per product, carried through conv2
        ys, _ = step_ref(x, w[0], b[0], w[1], b[1], k, dil, np.float64)
        assert float(np.abs(ys - y).max()) < 2 * C_BF16X3 * (1 + abs_rows(w[1])) * 16
    for cin, cout, k, s in ((32, 16, 16, 8), (16, 24, 8, 2)):
        xx = rng.standard_normal((cin, 37)).astype(np.float32)
        w = rng.standard_normal((cin, cout, k)).astype(np.float32)
        b = rng.standard_normal(cout).astype(np.float32)
        want = O.conv_transpose1d(O.leaky_relu(xx.astype(np.float64), SLOPE), w.astype(np.float64), b.astype(np.float64), s, (k - s) // 2)
        np.testing.assert_allclose(upconv_case(xx, w, b, s)[2], want, rtol=0, atol=1e-12)
    # the split: hi + lo leaves at most 2^-16 of the value (2^-17.x in fact), and the parts are bf16
    v = rng.standard_normal(4096).astype(np.float32) * np.float32(3.7)
    hi, lo = _bf16_parts(v, 2)
    assert not (hi.view(np.uint32) & 0xFFFF).any() and not (lo.view(np.uint32) & 0xFFFF).any()
    assert float((np.abs(v.astype(np.float64) - hi - lo) / np.abs(v)).max()) <= 2.0 ** -16


STEP_WRONG = ("drop_c1x", "drop_c1w", "drop_c2t", "drop_c2w", "taps1", "taps2", "dilation", "channels", "mid_unmasked", "res_after_beta", "no_accumulate", "slope",
              "tile_edge")


@pytest.mark.parametrize("C_,k,dil", [(16, 3, 1), (32, 7, 3), (64, 11, 5), (64, 3, 5), (16, 11, 1), (128, 3, 1), (256, 7, 3)])
def test_wrong_references_exceed_the_tolerance(C_, k, dil):
    """every deliberately wrong reference of a fused step is at least 2 x the tolerance of the case away from the right one, on the data the GPU cases use
    (dense normal, masked, beta = 1 / 3 with accumulate; the impulses for the tile edge: a dense intermediate hides nothing there either, both are checked)"""
    nto = nto_step(C_, k, 1, dil)
    N = 2 * nto + 1
    rng = np.random.default_rng(C_ * 100 + k)
    w1, w2 = make_w((C_, C_, k), rng), make_w((C_, C_, k), rng)
    b1, b2 = rng.standard_normal(C_).astype(np.float32), rng.standard_normal(C_).astype(np.float32)
    mask = make_mask("straddle", N, 4, nto // 2)
    keep = keep_of(mask, 4, N)
    for kind in ("normal", "impulse"):
        x = make_x(kind, C_, N, rng, nto) * keep[None, :]
        prev = rng.standard_normal((C_, N)).astype(np.float32) * keep[None, :]
        ref, tol = step_case(x, w1, b1, w2, b2, k, dil, keep, BETA3, prev)
        for wrong in STEP_WRONG:
            if kind == "impulse" and wrong not in ("tile_edge", "taps1", "taps2", "channels", "dilation"):
                continue
            if kind == "impulse" and wrong == "channels" and not x[7:9].any():    # (at C >= 128 no impulse sits in the two swapped channels: dense data only)
                continue
            bad, _ = step_ref(x, w1, b1, w2, b2, k, dil, np.float64, keep, BETA3, prev, wrong=wrong, seam=nto)
            r = float(np.abs(bad - ref).max()) / tol
            assert r >= 2.0, (kind, wrong, r)


def test_wrong_references_of_single_convolutions_and_chains():
    rng = np.random.default_rng(3)
    # one convolution (conv_cl / conv_clx): against the restatement and against the plain reference
    for cin, cout, k, dil in ((128, 128, 7, 3), (32, 64, 11, 5)):
        x = make_x("normal", cin, 300, rng, 256)
        w, b = make_w((cout, cin, k), rng), rng.standard_normal(cout).astype(np.float32)
        r64, rtol, p64, ptol = conv_case(x, w, b, dil)
        assert (np.abs(r64 - p64) / ptol).max() <= 1.0
        a = lrelu(x)
        bb = b.astype(np.float64)[:, None]
        for name, bad in (("drop_x", split_sum(a, w, dil, np.float64, "x") + bb), ("drop_w", split_sum(a, w, dil, np.float64, "w") + bb),
                          ("taps", split_sum(a, _swap_taps(w, 1), dil, np.float64) + bb), ("channels", split_sum(a, _swap_channels(w, 17, 18), dil, np.float64) + bb),
                          ("dilation", split_sum(a, w, dil + 1, np.float64) + bb), ("slope", split_sum(lrelu(x, 0.01), w, dil, np.float64) + bb)):
            assert float(np.abs(bad - r64).max()) / rtol >= 2.0, name
            assert float((np.abs(bad - p64) / ptol).max()) >= 2.0, name
    # the transposed convolution
    for cin, cout, k, s in ((64, 64, 16, 8), (32, 64, 8, 2)):
        x = make_x("normal", cin, 90, rng, 256)
        w = (rng.standard_normal((cin, cout, k)) / math.sqrt(cin * k / s)).astype(np.float32)
        b = rng.standard_normal(cout).astype(np.float32)
        r64, rtol, p64, ptol = upconv_case(x, w, b, s)
        assert (np.abs(r64 - p64) / ptol).max() <= 1.0
        for wrong in ("phases_swapped", "tap_off_one"):
            bad = upconv_case(x, w, b, s, wrong=wrong)[0]
            assert float(np.abs(bad - r64).max()) / rtol >= 2.0 and float((np.abs(bad - p64) / ptol).max()) >= 2.0, wrong
    # a chain on low-gain weights: a wrong reference in the first or the last step is still seen at the end.  Not conv1's lo parts: what they leave (2^-9 of a
    # product) passes through a conv2 of gain 1 and stays at 0.1 .. 1.4 of the chain tolerance; the fused-step and single-convolution cases hold them.
    for C_, k in ((128, 3), (16, 11), (256, 3)):
        N = 200
        x = make_x("normal", C_, N, rng, 168)
        w, b = make_w((6, C_, C_, k), rng, low_gain=True), rng.standard_normal((6, C_)).astype(np.float32)
        keep = keep_of(make_mask("straddle", N, 4, 100), 4, N)
        x = x * keep[None, :]
        prev = rng.standard_normal((C_, N)).astype(np.float32) * keep[None, :]
        ref, tol = chain_case(x, w, b, k, (1, 3, 5), keep, BETA3, prev)
        for q in (0, 2):
            for wrong in ("drop_c2t", "drop_c2w", "taps1", "taps2", "dilation", "channels", "mid_unmasked", "slope") + (("res_after_beta", "no_accumulate") if q == 2 else ()):
                bad, _ = chain_case(x, w, b, k, (1, 3, 5), keep, BETA3, prev, wrong=(q, wrong))
                assert float(np.abs(bad - ref).max()) / tol >= 2.0, (C_, k, q, wrong, float(np.abs(bad - ref).max()) / tol)
        bad, _ = chain_case(x, w, b, k, (5, 1, 3), keep, BETA3, prev)
        assert float(np.abs(bad - ref).max()) / tol >= 2.0


# ---- GPU part ------------------------------------------------------------------------------------------------------------------------------------------------

def _P(a):
    return None if a is None else a.ctypes.data_as(f32p)


def _cl(a):
    """channel-major [C][N] -> the hooks' channels-last [N][C]"""
    return None if a is None else np.array(a.T, np.float32, order="C", copy=True)   # (a copy also at N = 1, where the transpose is contiguous as it is)


def _respair(x, w1, w2, b1, b2, k, dil, mask, div, beta, prev, variant):
    C_, N = x.shape
    y = _cl(prev) if prev is not None else np.zeros((N, C_), np.float32)
    xs = _cl(x)
    _lib.check(_lib.lib().sbv2_debug_respair(0, _P(xs), _P(w1), _P(w2), _P(b1), _P(b2), C_, N, k, dil, None if mask is None else mask.ctypes.data, div,
                                             float(beta), int(prev is not None), variant, _P(y)))
    return np.ascontiguousarray(y.T)


def _resbranch(x, w, b, k, dils, mask, div, beta, prev, variant, want_ys=False, want_steps=False):
    """want_ys (variant 3): also the parts of the result; want_steps: also [(plane, parts)] of the first two steps"""
    C_, N = x.shape
    y = _cl(prev) if prev is not None else np.zeros((N, C_), np.float32)
    xs, d = _cl(x), np.asarray(dils, np.int64)
    mp = None if mask is None else mask.ctypes.data
    if want_ys:
        ys = np.empty((N, C_), np.float32)
        st, sts = (np.empty((2, N, C_), np.float32), np.empty((2, N, C_), np.float32)) if want_steps else (None, None)
        _lib.check(_lib.lib().sbv2_debug_resbranch_ys(0, _P(xs), _P(w), _P(b), C_, N, k, d.ctypes.data_as(i64p), mp, div, float(beta), int(prev is not None), 0,
                                                      _P(y), _P(ys), _P(st), _P(sts), None))
        if want_steps:
            return np.ascontiguousarray(y.T), np.ascontiguousarray(ys.T), [(np.ascontiguousarray(st[q].T), np.ascontiguousarray(sts[q].T)) for q in (0, 1)]
        return np.ascontiguousarray(y.T), np.ascontiguousarray(ys.T)
    _lib.check(_lib.lib().sbv2_debug_resbranch(0, _P(xs), _P(w), _P(b), C_, N, k, d.ctypes.data_as(i64p), mp, div, float(beta), int(prev is not None), variant,
                                               0, _P(y), None))
    return np.ascontiguousarray(y.T)


def _masked_zero(y, keep, what):
    assert not np.any(y[:, keep == 0]), f"{what}: a masked column is not exactly zero"


def _modes(C_, N, keep, rng):
    """the epilogue modes of a masked run: beta = 1 / 3 onto previous contents (a branch's last step), and beta = 1"""
    prev = rng.standard_normal((C_, N)).astype(np.float32) * keep[None, :]
    return ((BETA3, prev), (1.0, None))


@gpu
@pytest.mark.parametrize("C_,k", STEP_CASES, ids=[f"C{c}-k{k}" for c, k in STEP_CASES])
def test_fused_step(C_, k):
    """sbv2_debug_respair, variants 0 (respair_cl), 1 (the default dispatch: respair_x16 at C >= 32, k >= 7, else respair_clx) and 2 (respair_clx), each
    against the split restatement; the bit-equality relations between them; masked columns exactly zero"""
    ci = STEP_CASES.index((C_, k))
    rng = np.random.default_rng(1000 * C_ + k)
    w1, w2 = make_w((C_, C_, k), rng), make_w((C_, C_, k), rng)
    b1, b2 = rng.standard_normal(C_).astype(np.float32), rng.standard_normal(C_).astype(np.float32)
    worst = {0: 0.0, 1: 0.0, 2: 0.0}

    def run(x, dil, mask, div, keep, beta, prev, tag):
        ref, tol = step_case(x, w1, b1, w2, b2, k, dil, keep, beta, prev)
        got = {v: _respair(x, w1, w2, b1, b2, k, dil, mask, div, beta, prev, v) for v in (0, 1, 2)}
        for v in (0, 1, 2):
            assert np.isfinite(got[v]).all()
            worst[v] = max(worst[v], _report(f"respair v{v} C{C_} k{k} d{dil} {tag}", np.abs(got[v] - ref), tol))
            if keep is not None:
                _masked_zero(got[v], keep, f"v{v} {tag}")
        if C_ >= 32:
            np.testing.assert_array_equal(got[2], got[0], err_msg=f"respair_clx != respair_cl, {tag}")
        if respair_default(C_, k, dil) == "clx":
            np.testing.assert_array_equal(got[1], got[2], err_msg=f"default != respair_clx, {tag}")

    for i, N in enumerate(step_lengths(C_, k)):
        dil = (1, 3, 5)[i % 3]
        kind, pat, div = plan(ci, i, C_)
        nto = nto_step(C_, k, 1, dil)
        x = make_x(kind, C_, N, rng, nto)
        run(x, dil, None, 1, None, 1.0, None, f"N{N} {kind}")
        mask = make_mask(pat, N, div, nto)
        keep = keep_of(mask, div, N)
        xm = x * keep[None, :]                            # (a masked column holds zeros in the decoder's planes)
        for beta, prev in _modes(C_, N, keep, rng):
            run(xm, dil, mask, div, keep, beta, prev, f"N{N} {kind} {pat}/{div} beta{beta:.2f}")
    print(f"[respair C{C_} k{k}] worst ratios: respair_cl {worst[0]:.3f}, default {worst[1]:.3f}, respair_clx {worst[2]:.3f}")
    assert max(worst.values()) <= 1.0, worst


@gpu
@pytest.mark.parametrize("C_,k", BRANCH_CASES, ids=[f"C{c}-k{k}" for c, k in BRANCH_CASES])
def test_fused_branch(C_, k):
    """sbv2_debug_resbranch: variant 1 (resbranch_clx.hip) = variant 0 (three default steps, C <= 64) = variant 2 (six conv_cl launches, C >= 32) bit for bit on
    decoder-like weights, where the chain is held step by step: each default step against the restatement on the plane the previous one returned, the last
    one's bits = variant 0's.  On low-gain weights every variant directly against the three-step restatement with the chain tolerance."""
    ci = BRANCH_CASES.index((C_, k))
    rng = np.random.default_rng(2000 * C_ + k)
    w, wl = make_w((6, C_, C_, k), rng), make_w((6, C_, C_, k), rng, low_gain=True)
    b = rng.standard_normal((6, C_)).astype(np.float32)
    variants = [v for v in (0, 1, 2) if (v != 0 or C_ <= 64)]
    worst = {"steps": 0.0, 0: 0.0, 1: 0.0, 2: 0.0}

    def run(x, dils, mask, div, keep, modes, tag0):
        for (beta, prev), (ref, tol) in zip(modes, chain_cases(x, wl, b, k, dils, keep, modes)):
            run1(x, dils, mask, div, keep, beta, prev, ref, tol, f"{tag0} beta{beta:.2f}")

    def run1(x, dils, mask, div, keep, beta, prev, ref, tol, tag):
        got = {v: _resbranch(x, w, b, k, dils, mask, div, beta, prev, v) for v in variants}
        if C_ <= 64:
            np.testing.assert_array_equal(got[1], got[0], err_msg=f"fused branch != three steps, {tag}")
            y = x
            for q in range(3):
                bq, pq = (beta, prev) if q == 2 else (1.0, None)
                sref, stol = step_case(y, w[2 * q], b[2 * q], w[2 * q + 1], b[2 * q + 1], k, dils[q], keep, bq, pq)
                y = _respair(y, w[2 * q], w[2 * q + 1], b[2 * q], b[2 * q + 1], k, dils[q], mask, div, bq, pq, 1)
                worst["steps"] = max(worst["steps"], _report(f"branch step {q} C{C_} k{k} {tag}", np.abs(y - sref), stol))
            np.testing.assert_array_equal(got[0], y, err_msg=f"three steps != the steps one by one, {tag}")
        # (beta * sum + previous: the fused kernels of C <= 64 round it as ONE fma, as the fused step does; conv_cl.hip as product, then sum: one ulp apart, 2.4e-7
        # measured at C = 32.  At C = 128 the fused branch writes product-then-sum and the relation holds there too.)
        if C_ >= 32 and (prev is None or C_ == 128):
            np.testing.assert_array_equal(got[1], got[2], err_msg=f"fused branch != six conv_cl launches, {tag}")
        for v in variants:
            g = _resbranch(x, wl, b, k, dils, mask, div, beta, prev, v)
            assert np.isfinite(g).all() and np.isfinite(got[v]).all()
            worst[v] = max(worst[v], _report(f"resbranch v{v} low gain C{C_} k{k} {tag}", np.abs(g - ref), tol))
            if keep is not None:
                _masked_zero(g, keep, f"v{v} {tag}")
                _masked_zero(got[v], keep, f"v{v} {tag}")

    nto = nto_resbranch(C_, k)
    for i, N in enumerate(lengths(nto, rb_halo(k, ORDERS[0]))):
        dils = ORDERS[i % 2]
        kind, pat, div = plan(ci, i, C_)
        x = make_x(kind, C_, N, rng, nto)
        run(x, dils, None, 1, None, ((1.0, None),), f"N{N} {kind} {dils}")
        mask = make_mask(pat, N, div, nto)
        keep = keep_of(mask, div, N)
        run(x * keep[None, :], dils, mask, div, keep, _modes(C_, N, keep, rng), f"N{N} {kind} {dils} {pat}/{div}")
    print(f"[resbranch C{C_} k{k}] worst ratios: step by step {worst['steps']:.3f}, low-gain chain v0 {worst[0]:.3f} v1 {worst[1]:.3f} v2 {worst[2]:.3f}")
    assert max(worst.values()) <= 1.0, worst


def _conv1d_cl(x, w, b, dil):
    cout, cin, k = w.shape
    y = np.empty((cout, x.shape[1]), np.float32)
    _lib.check(_lib.lib().sbv2_debug_conv1d_cl(0, _P(x), _P(w), _P(b), cin, cout, k, x.shape[1], dil, SLOPE, 1, 0, _P(y), None))
    return y


def _conv1d_clx(x, w, b, dil, res=None, beta=1.0, want_ys=False):
    cout, cin, k = w.shape
    y = np.empty((cout, x.shape[1]), np.float32)
    ys = np.empty_like(y) if want_ys else None
    _lib.check(_lib.lib().sbv2_debug_conv1d_clx(0, _P(x), _P(w), _P(b), _P(res), cin, cout, k, x.shape[1], dil, SLOPE, float(beta), 0, _P(y), _P(ys), None))
    return y, ys


def _check_parts(ys, y, what):
    lr = lrelu(y)
    assert np.all(np.abs(ys.astype(np.float64) - lr) <= _split_bound(lr, 2)), f"{what}: the parts are not the split of lrelu(the result)"


@gpu
@pytest.mark.parametrize("cin,cout,k", CONV_CL_CASES, ids=[f"{a}-{b}-k{k}" for a, b, k in CONV_CL_CASES])
def test_conv_cl(cin, cout, k):
    """conv_cl.hip's split-bf16 channels-last launch (sbv2_debug_conv1d_cl, mode 1) against the restatement and the plain reference, around its 256-position tiles"""
    rng = np.random.default_rng(cin * 7 + cout + k)
    w, b = make_w((cout, cin, k), rng), rng.standard_normal(cout).astype(np.float32)
    worst = [0.0, 0.0]
    for i, N in enumerate(lengths(NT_CONV, 5 * (k - 1) // 2)):
        dil, kind = (1, 3, 5)[i % 3], KINDS[i % 4]
        x = make_x(kind, cin, N, rng, NT_CONV)
        r64, rtol, p64, ptol = conv_case(x, w, b, dil)
        y = _conv1d_cl(x, w, b, dil)
        assert np.isfinite(y).all()
        worst[0] = max(worst[0], _report(f"conv_cl {cin}->{cout} k{k} d{dil} N{N} {kind} / restatement", np.abs(y - r64), rtol))
        worst[1] = max(worst[1], _report(f"conv_cl {cin}->{cout} k{k} d{dil} N{N} {kind} / plain", np.abs(y - p64), ptol))
    print(f"[conv_cl {cin}->{cout} k{k}] worst ratios: restatement {worst[0]:.3f}, plain {worst[1]:.3f}")
    assert max(worst) <= 1.0, worst


@gpu
@pytest.mark.parametrize("cin,cout,k", CONV_CLX_CASES, ids=[f"{a}-{b}-k{k}" for a, b, k in CONV_CLX_CASES])
def test_conv_clx(cin, cout, k):
    """conv_clx.hip on split_cl's parts (sbv2_debug_conv1d_clx) against the restatement and the plain reference around its 256-position tiles (a ragged last tile
    is moved left and overlaps its neighbour; below 256 positions the guarded epilogue runs); the parts it emits are the split of its own result; its residual
    epilogue is ((y + r) beta) of its plain result, exactly"""
    rng = np.random.default_rng(cin * 5 + cout + k)
    w, b = make_w((cout, cin, k), rng), rng.standard_normal(cout).astype(np.float32)
    worst = [0.0, 0.0]
    for i, N in enumerate(lengths(NT_CONV, 5 * (k - 1) // 2)):
        dil, kind = (1, 3, 5)[i % 3], KINDS[i % 4]
        x = make_x(kind, cin, N, rng, NT_CONV)
        r64, rtol, p64, ptol = conv_case(x, w, b, dil)
        y, ys = _conv1d_clx(x, w, b, dil, want_ys=True)
        assert np.isfinite(y).all()
        worst[0] = max(worst[0], _report(f"conv_clx {cin}->{cout} k{k} d{dil} N{N} {kind} / restatement", np.abs(y - r64), rtol))
        worst[1] = max(worst[1], _report(f"conv_clx {cin}->{cout} k{k} d{dil} N{N} {kind} / plain", np.abs(y - p64), ptol))
        _check_parts(ys, y, f"N{N} {kind}")
        r = rng.standard_normal((cout, N)).astype(np.float32)
        y2, _ = _conv1d_clx(x, w, b, dil, res=r, beta=BETA3)
        np.testing.assert_array_equal(y2, ((y + r) * np.float32(BETA3)).astype(np.float32), err_msg=f"residual epilogue, N{N}")
    print(f"[conv_clx {cin}->{cout} k{k}] worst ratios: restatement {worst[0]:.3f}, plain {worst[1]:.3f}")
    assert max(worst) <= 1.0, worst


def _upx(x, w, b, s, mask=None, div=1, want_ys=False):
    cin, cout, k = w.shape
    L = x.shape[1]
    y = np.empty((cout, L * s), np.float32)
    ys = np.empty_like(y) if want_ys else None
    _lib.check(_lib.lib().sbv2_debug_conv_transpose1d_clx(0, _P(x), _P(w), _P(b), cin, cout, k, L, s, SLOPE, None if mask is None else mask.ctypes.data, div, 0,
                                                          _P(y), _P(ys), None))
    return y, ys


@gpu
@pytest.mark.parametrize("cin,cout,k,s", UPX_CASES, ids=[f"{a}-{b}-k{k}-s{s}" for a, b, k, s in UPX_CASES])
def test_conv_transpose_clx(cin, cout, k, s):
    """the phased conv_clx launch of a ConvTranspose1d (sbv2_debug_conv_transpose1d_clx) against the restatement and the plain reference, plain and with column
    masks on the input positions (mask_div 1, 4, 8, 64); every output row written; the parts of lrelu(result) it leaves for the ResBlocks"""
    rng = np.random.default_rng(cin + cout + 10 * k + s)
    w = (rng.standard_normal((cin, cout, k)) / math.sqrt(cin * k / s)).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    worst = [0.0, 0.0]
    for i, L in enumerate(UPX_LENGTHS):
        kind = KINDS[i % 4]
        x = make_x(kind, cin, L, rng, NT_CONV)
        r64, rtol, p64, ptol = upconv_case(x, w, b, s)
        y, ys = _upx(x, w, b, s, want_ys=True)
        assert np.isfinite(y).all(), "an output row was not written"
        worst[0] = max(worst[0], _report(f"upx {cin}->{cout} k{k} s{s} L{L} {kind} / restatement", np.abs(y - r64), rtol))
        worst[1] = max(worst[1], _report(f"upx {cin}->{cout} k{k} s{s} L{L} {kind} / plain", np.abs(y - p64), ptol))
        _check_parts(ys, y, f"L{L} {kind}")
        div = (1, 4, 8, 64)[i % 4]
        mask = make_mask(PATTERNS[(i + 2) % 5], L, div, NT_CONV)
        keep = keep_of(mask, div, L)
        xm = x * keep[None, :]
        r64, rtol, p64, ptol = upconv_case(xm, w, b, s, keep)
        y, ys = _upx(xm, w, b, s, mask, div, want_ys=True)
        worst[0] = max(worst[0], _report(f"upx {cin}->{cout} k{k} s{s} L{L} {kind} masked / restatement", np.abs(y - r64), rtol))
        _masked_zero(y, np.repeat(keep, s), f"L{L}")
        _check_parts(ys, y, f"L{L} {kind} masked")
    print(f"[upx {cin}->{cout} k{k} s{s}] worst ratios: restatement {worst[0]:.3f}, plain {worst[1]:.3f}")
    assert max(worst) <= 1.0, worst


CHAIN_RUNS = [(c, k, g) for c, k in CHAIN_CASES for g in CHAIN_GROUPS]


@gpu
@pytest.mark.parametrize("C_,k,group", CHAIN_RUNS, ids=[f"C{c}-k{k}-{g}" for c, k, g in CHAIN_RUNS])
def test_wide_stage_step_chain(C_, k, group):
    """sbv2_debug_resbranch variant 3: the six conv_clx launches of a branch as the decoder's wide stages make them (the input's parts by split_cl, conv1 writes
    parts only, conv2 reads them; column mask with the stage's shift; beta and accumulate on the last launch; optionally the parts of the result).  On low-gain
    weights against the three-step restatement; against variant 2 (six conv_cl launches) and, at C = 128, k = 3, variant 1 (the fused branch), each within the
    sum of the two tolerances; the emitted parts are the split of the returned plane.  On decoder-like weights (up to two tiles) the chain is held step by step
    as the C <= 64 branches are: every step's plane against the restatement of one step on the plane the previous step returned, with the fused step's
    tolerance, and the parts every conv2 launch wrote for the next conv1 against the plane of the same launch."""
    rng = np.random.default_rng(3000 * C_ + k)
    wl, w = make_w((6, C_, C_, k), rng, low_gain=True), make_w((6, C_, C_, k), rng)
    b = rng.standard_normal((6, C_)).astype(np.float32)
    worst = {3: 0.0, 2: 0.0, 1: 0.0, "3-2": 0.0, "steps": 0.0}
    others = [2] + ([1] if resbranch_usable(C_, k, ORDERS[0]) else [])
    for i, N in chain_lengths(C_, k, group):
        dils, kind, div, pat, with_plain = chain_plan(i, C_, N)
        rng = np.random.default_rng(3000 * C_ + 16 * k + i)          # (a length's data does not depend on the group it runs in)
        x = make_x(kind, C_, N, rng, NT_CONV)
        mask = make_mask(pat, N, div, NT_CONV)
        keep = keep_of(mask, div, N)
        xm = x * keep[None, :]
        modes = _modes(C_, N, keep, rng)
        runs = [(x, None, 1, None, 1.0, None) + chain_case(x, wl, b, k, dils)] if with_plain else []
        runs += [(xm, mask, div, keep, beta, prev, ref, tol) for (beta, prev), (ref, tol) in zip(modes, chain_cases(xm, wl, b, k, dils, keep, modes))]
        for xx, m, d, kp, beta, prev, ref, tol in runs:
            tag = f"N{N} {kind} {dils} {'plain' if m is None else pat + '/' + str(d)} beta{beta:.2f}"
            y3, ys = _resbranch(xx, wl, b, k, dils, m, d, beta, prev, 3, want_ys=True)
            assert np.isfinite(y3).all()
            worst[3] = max(worst[3], _report(f"clx chain C{C_} k{k} {tag}", np.abs(y3 - ref), tol))
            np.testing.assert_array_equal(_resbranch(xx, wl, b, k, dils, m, d, beta, prev, 3), y3, err_msg="with and without the parts output")
            _check_parts(ys, y3, tag)
            if kp is not None:
                _masked_zero(y3, kp, tag)
            for v in others:
                g = _resbranch(xx, wl, b, k, dils, m, d, beta, prev, v)
                worst[v] = max(worst[v], _report(f"v{v} C{C_} k{k} {tag}", np.abs(g - ref), tol))
                if v == 2:
                    worst["3-2"] = max(worst["3-2"], _report(f"clx chain - conv_cl chain C{C_} k{k} {tag}", np.abs(y3 - g), 2 * tol))
        if N > 2 * NT_CONV:
            continue
        # decoder-like weights, step by step, on the masked data with beta = 1 / 3 onto previous contents
        beta, prev = modes[0]
        tag = f"N{N} {kind} {dils} {pat}/{div} decoder-like"
        y3, ys, steps = _resbranch(xm, w, b, k, dils, mask, div, beta, prev, 3, want_ys=True, want_steps=True)
        yin = xm
        for q, (yq, ysq) in enumerate(steps + [(y3, ys)]):
            bq, pq = (beta, prev) if q == 2 else (1.0, None)
            sref, stol = step_case(yin, w[2 * q], b[2 * q], w[2 * q + 1], b[2 * q + 1], k, dils[q], keep, bq, pq)
            assert np.isfinite(yq).all()
            worst["steps"] = max(worst["steps"], _report(f"clx chain step {q} C{C_} k{k} {tag}", np.abs(yq - sref), stol))
            _check_parts(ysq, yq, f"step {q} {tag}")
            _masked_zero(yq, keep, f"step {q} {tag}")
            yin = yq
    print(f"[clx chain C{C_} k{k} {group}] worst ratios: variant 3 {worst[3]:.3f}, variant 2 {worst[2]:.3f}, variant 1 {worst[1]:.3f}, 3 against 2 "
          f"{worst['3-2']:.3f}, decoder-like step by step {worst['steps']:.3f}")
    assert max(worst.values()) <= 1.0, worst


@gpu
def test_launch_counts_and_refusals():
    """sbv2_prof_begin / _end: one launch per fused step or fused branch, three for the branch as steps, six for the conv_cl and conv_clx chains; shapes and
    lengths a launcher does not take are refused with an error, not run"""
    rng = np.random.default_rng(9)
    k, N = 3, 300
    for C_ in (32, 128):
        x = make_x("normal", C_, N, rng, 100)
        w, b = make_w((6, C_, C_, k), rng), rng.standard_normal((6, C_)).astype(np.float32)
        if C_ == 32:
            for v in (0, 1, 2):
                with _Prof() as p:
                    _respair(x, w[0], w[1], b[0], b[1], k, 1, None, 1, 1.0, None, v)
                assert p.launches == 1, (v, p.launches, p.kernels)
        for v, n in ((0, 3), (1, 1), (2, 6), (3, 6)):
            if (v == 0 and C_ > 64) or (v == 3 and C_ < 128):
                continue
            with _Prof() as p:
                _resbranch(x, w, b, k, (1, 3, 5), None, 1, 1.0, None, v)
            assert p.launches == n, (C_, v, p.launches, p.kernels)
    x = make_x("normal", 32, N, rng, 100)
    w7, b7 = make_w((6, 32, 32, 7), rng), rng.standard_normal((6, 32)).astype(np.float32)
    w3, b3 = make_w((6, 64, 64, 3), rng), rng.standard_normal((6, 64)).astype(np.float32)
    w11 = make_w((2, 32, 32, 11), rng)
    x64 = make_x("normal", 64, N, rng, 100)
    assert not resbranch_usable(32, 7, (1, 3, 5)) and not resbranch_usable(64, 3, (1, 3, 9)) and not respair_clx_usable(32, 11, 7)
    with pytest.raises(_lib.Sbv2Error):
        _resbranch(x, w7, b7, 7, (1, 3, 5), None, 1, 1.0, None, 1)
    with pytest.raises(_lib.Sbv2Error):
        _resbranch(x64, w3, b3, 3, (1, 3, 9), None, 1, 1.0, None, 1)
    for v in (0, 1, 2):
        with pytest.raises(_lib.Sbv2Error):
            _respair(x, w11[0], w11[1], b7[0], b7[1], 11, 7, None, 1, 1.0, None, v)
    with pytest.raises(_lib.Sbv2Error):
        _resbranch(x, w7, b7, 7, (1, 3, 5), None, 1, 1.0, None, 3)     # the conv_clx chain is the path of the >= 128-channel stages
    xw = make_x("normal", 128, N, rng, 100)
    assert not conv_clx_usable(128, 128, 11, 7) and not upx_usable(128, 64, 16, 8, 255)
    with pytest.raises(_lib.Sbv2Error):
        _conv1d_clx(xw, make_w((128, 128, 11), rng), rng.standard_normal(128).astype(np.float32), 7)
    with pytest.raises(_lib.Sbv2Error):
        _upx(xw[:, :255].copy(), make_w((128, 64, 16), rng), rng.standard_normal(64).astype(np.float32), 8)
