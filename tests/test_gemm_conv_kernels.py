"""The convolution / GEMM launchers (csrc/gemm_conv.hip, gemm_skinny.hip, gemm_bfs.hip, the k-major side of conv_cl.hip and conv_cl_small.hip) launch by
launch through conv_plain, conv_bfs, conv_km_to_cl / conv_cl_to_km and linear_tokmajor with the arguments the MODELS pass (activations, residual with
alpha = -1, beta with accumulate, masks with mask_div 1 and 4, pre_slope, null bias, y_rows / ys_row0, parts-only output), against float64 numpy statements
of the same operation.  The hooks (csrc/test_hooks.cpp) put every plane at the library's pitch, NaN behind L in every input, a sentinel in every output,
and count the pad words a launch changed.

Epilogue order (csrc/common.h, ConvParams / ConvClParams / GemmBfsParams; read from the kernels): bias, act, alpha, residual, beta, accumulate, mask.  It is
how oracle/sbv2_oracle.py states the steps that use it: the flow coupling x1 = (x1 - m) * mask is act none, alpha -1, residual x1, mask; the FFN is
(conv(relu(.)) + b + x) * mask; the k-major ResBlock sum is xs += (conv + b + y) / nk.  The channels-last conv_cl epilogue (the FFN's intermediate) has no
activation and no alpha.  Epilogue implementations: conv_gemm_kernel's staged-tile form (interior and edge sub-tiles; the ring instantiations share it) and
its scalar form (16-row MFMA), gemm_skinny's, gemm_bfs' interior and generic forms, conv_cl's k-major and channels-last ones, conv_cl_small's.

Tolerances (derived; the worst error / tolerance ratio of every case is printed):
- f32 MFMA (launch_conv, the skinny kernels, linear_tokmajor): max(4 err32, 8 ulp of the output's scale); err32 = the largest deviation of the same
  reference evaluated in float32, the scale = the largest |reference|.
- split operands, per output element: c * sum_k,tap |w| |x| times the epilogue's Lipschitz factor (|alpha| |beta|; 1 for ReLU / tanh, 1.13 for GELU)
  + 4 err32 for the f32 accumulation and epilogue.  With the conventions of tests/test_ops_kernels.py (a bf16 part leaves 2^-8 relative, an f16 part 2^-11):
  bf16x3: two parts leave 2^-16 of each operand, the dropped lo * lo term is 2^-16: c = 3 * 2^-16.  f16x3 (split_store4: hi = f16(x), lo = f16((x - hi)
  2^11)): 2^-22 each, dropped 2^-22: c = 3 * 2^-22.  bf16x6: three parts leave 2^-24 each, dropped mid * lo + lo * mid = 2 * 2^-24, lo * lo = 2^-32:
  c = 5 * 2^-24 (f32-grade).  Parts outputs add _split_bound of test_ops_kernels.py (three bf16 parts: 2^-24 relative).
- plain bf16 / f16 conv_cl modes: each operand is rounded once, half an ulp = 2^-8 / 2^-11 relative: that factor times sum |w| |x|, + 4 err32 (the terms'
  errors do not align; an impulse, where only w rounds, comes closest to the bound).
- masked columns, rows a plane does not receive (sentinel) and the f32 path's impulse responses: exact.  Stray count: 0.
- the FFN pair: the intermediate against the float64 first convolution with the bf16x3 bound; the output against the second convolution evaluated on the
  intermediate THE HOOK RETURNS, with the bf16x3 bound of that convolution alone (nothing of the first stage's error is allowed twice).
Every family has deliberately wrong references that must exceed its tolerance on the same data (the CPU part of this module).  One cannot be seen
everywhere: GELU's tanh approximation is at most 4.7e-4 from the erf form, inside what plain bf16 / f16 operands allow, so on conv_cl's k-major epilogue
only the bf16x3 cases hold the GELU form; the plain bf16 / f16 cases hold its argument, scaling and order.
Every GPU case also asks the library's launch profile (sbv2_prof_begin / _end) which kernel family and tile ran, and compares it with the mirror's answer.

launch_conv's grouped form (GemmGroup) is run by the unfused attention variants of tests/test_attention_kernels.py and is left out here.

Measured worst error / tolerance ratios on an MI355X (every stray count 0, no NaN from a poisoned pad): f32 tiled 0.74, f32 skinny 0.52, linear_tokmajor 0.25;
k-major conv_cl bf16x3 0.19, bf16 0.95, f16 0.95 (both on the impulses); the FFN pair 0.07 (intermediate) / 0.01 (output); gemm_bfs f32 plane / parts:
bf16x3 0.16 / 0.20, f16x3 0.25 / 0.15, bf16x6 0.25 / 0.14.  The impulse responses of the f32 path are exact in every instantiation.
"""
import ctypes as C
import json
import math
import os
import re

import numpy as np
import pytest

import sbv2_oracle as O
from sbv2_api_amd import _lib
from test_ops_kernels import _report, _split_bound

gpu = pytest.mark.gpu
f32p, i64p = _lib.f32p, _lib.i64p
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sbv2-api_amd", "csrc")
EPS32 = 2.0 ** -24
NCU = 256
ACT_NONE, ACT_RELU, ACT_GELU, ACT_TANH = 0, 1, 2, 3
GELU_SLOPE = 1.13   # max of d/dx gelu = Phi(x) + x phi(x), reached at x = sqrt(2): 0.9214 + 0.2076
C_BF16X3, C_F16X3, C_BF16X6 = 3 * 2.0 ** -16, 3 * 2.0 ** -22, 5 * 2.0 ** -24
C_BF16, C_F16 = 2.0 ** -8, 2.0 ** -11
SENTINEL = np.array([0x5A5A5A5A], np.uint32).view(np.float32)[0]
HOOKS = ["sbv2_debug_conv_plain", "sbv2_debug_conv_ffn_cl", "sbv2_debug_gemm_bfs_ex", "sbv2_debug_linear_tokmajor"]


def _f(a):
    return None if a is None else a.ctypes.data_as(f32p)


def _c32(a):
    return None if a is None else np.ascontiguousarray(a, np.float32)


def _u8p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _cdiv(a, b):
    return -(-a // b)


# ---- the dispatch of launch_conv / launch_gemm_skinny* (csrc/gemm_conv.hip, gemm_skinny.hip) and launch_gemm_bfs (csrc/gemm_bfs.hip), mirrored --------------

def conv_kernel(M, N, K, ntaps, span=0, skinny_max=128, ncu=NCU):
    """The instantiation launch_conv takes for an ungrouped, unphased launch on planes of the library (pitches multiples of 4, N <= nb, shift 0 when
    ntaps == 1): the template argument list of launch_cfg<...>, or the skinny kernel.  span = max shift - floor4(min shift) (the taps kernel's window).
    The thresholds are workgroup counts written for 256 CUs; the launcher itself does not read the device's count."""
    assert ncu == 256
    blocks = lambda mt, nt: _cdiv(M, mt) * _cdiv(N, nt)
    if M <= 16:
        return "16,1,4,1,4,16"
    if M <= 32:
        return "32,1,2,1,4,16" if blocks(32, 256) >= 512 else "32,1,1,1,4,16"
    if ntaps == 1:
        if blocks(64, 64) < (skinny_max + skinny_max // 2 if K >= 512 else skinny_max) and K % 16 == 0 and K >= 16:
            return "skinny<1,16>" if _cdiv(M, 16) * _cdiv(N, 16) <= 1024 else "skinny<2,16>"
        ring = K % 16 == 0 and K >= 48
        if ring and 384 <= blocks(128, 128) <= 512:
            return "32,2,2,2,2,16,true"
        if ring:
            return "32,1,1,2,2,16,true"
        if blocks(64, 128) >= 512:
            return "32,1,2,2,2,16"
        if blocks(64, 64) < 128 and N <= 128:
            return "32,1,1,1,4,64"
        return "32,1,1,2,2,16"
    if blocks(64, 64) < skinny_max and K % 16 == 0 and K >= 16 and 16 + span <= 64 and _cdiv(M, 16) * _cdiv(N, 16) <= 2048:
        return "skinny_taps"
    if blocks(64, 256) >= 512:
        return "32,2,2,1,4,16"
    if blocks(64, 128) >= 256:
        return "32,1,2,2,2,16"
    return "32,1,1,2,2,16"


CONV_ALL = {"16,1,4,1,4,16", "32,1,2,1,4,16", "32,1,1,1,4,16", "32,2,2,2,2,16,true", "32,1,1,2,2,16,true", "32,1,2,2,2,16", "32,1,1,1,4,64",
            "32,1,1,2,2,16", "32,2,2,1,4,16"}
SKINNY_ALL = {"skinny<1,16>", "skinny<2,16>", "skinny_taps"}
# launch sites (not instantiations) no argument can reach, with the reason
UNREACHABLE = {
    "if (ring) return launch_cfg<32, 1, 1, 2, 2, 16, true>(kp, Mx, Nx, stream);":
        "launch_conv tests `ring` twice in the ntaps == 1 branch; the first test returns, so the second one (behind the Nx <= 128 test) never sees ring == true",
}


def bfs_kernel(parts, M, N, K, ksplit, ncu=NCU, ws_bytes=48 << 20, ncounters=1024):
    """The instantiation launch_gemm_bfs takes (parts code 2 = bf16x3, 3 = bf16x6, 4 = f16x3; the hooks pass 48 MB of K-split scratch and 1024 counters)."""
    blocks = lambda mt, nt: _cdiv(M, mt) * _cdiv(N, nt)
    big, lone, k32 = blocks(128, 128) >= 128, blocks(128, 128) <= ncu, K % 32 == 0
    if parts == 4:
        if big:
            return "2,1,2,2,2,1,4,true"
        tiles, nch, ks = blocks(64, 64), K // 16, 1
        if ksplit and tiles <= ncounters and nch >= 128:
            while ks < 8 and tiles * ks * 2 <= ncu and nch % (ks * 2) == 0 and nch // (ks * 2) >= 32 and tiles * ks * 2 * 32768 <= ws_bytes:
                ks *= 2
        if ks > 1:
            return "2,1,1,2,2,1,8,true,true"
        if ksplit and nch % 4 == 0 and nch >= 32 and blocks(32, 32) <= ncu:
            return "2,1,1,1,1,1,4,true,false,4"
        return "2,1,1,2,2,1,8,true"
    if parts == 2:
        return "2,1,1,2,2,1,8" if not big else ("2,2,2,2,2,2,4" if k32 and lone else "2,2,2,2,2,1,5")
    return "3,1,1,2,2,1,6" if not big else ("3,2,2,2,2,1,6" if lone else "3,2,2,2,2,1,3")


BFS_ALL = {"2,1,2,2,2,1,4,true", "2,1,1,2,2,1,8,true,true", "2,1,1,1,1,1,4,true,false,4", "2,1,1,2,2,1,8,true", "2,1,1,2,2,1,8", "2,2,2,2,2,2,4",
           "2,2,2,2,2,1,5", "3,1,1,2,2,1,6", "3,2,2,2,2,1,6", "3,2,2,2,2,1,3"}


def cl_kernel(M, N, cl_parts):
    """conv_plain's k-major conv_cl launch (k >= 3): conv_cl_kernel<TM, PREC, true, true>; pack_cl's row tiling and launch_conv_cl's small-grid rule"""
    tm = 2 if M >= 64 else 1
    nmt = _cdiv(_cdiv(M, 32), tm) * tm
    if tm == 2 and _cdiv(N, 256) * (nmt // 2) < 128:
        tm = 1
    return f"cl_km<{tm},{ {1: 'bf16', 2: 'bf16x3', 3: 'f16'}[cl_parts] }>"


def _nt(name):
    """columns per workgroup tile of an instantiation (the seams the impulses sit on)"""
    if name.startswith("skinny"):
        return 32 if name == "skinny<2,16>" else 16
    if name.startswith("cl"):
        return 256
    a = [int(v) for v in name.split(",")[:6]]
    return a[0] * a[2] * a[4]


# ---- cases ------------------------------------------------------------------------------------------------------------------------------------------------
# epilogue variants: every act, residual with alpha -1, beta 1/3 with accumulate, mask_div 1 and 4, pre_slope 1 / 0.1 / 0, a null bias
VARIANTS = {
    "plain": dict(),
    "relu-mask1-pre.1": dict(act=ACT_RELU, mask_div=1, pre_slope=0.1),
    "gelu-res-alpha-1-mask4-pre0": dict(act=ACT_GELU, res=True, alpha=-1.0, mask_div=4, pre_slope=0.0),
    "tanh-acc-beta-nobias": dict(act=ACT_TANH, res=True, beta=1.0 / 3.0, accumulate=True, bias=False),
}
ALLV = tuple(VARIANTS)
# (cout M, L N, cin K, k, dilation, skinny_max, variants, instantiation[, pad_l]); pad_l defaults to the symmetric dilation (k - 1) / 2, the cases that name
# it run a causal window (pad_l = (k - 1) dilation) or one that only looks ahead (0): another floor4(min shift) than the symmetric one.  Smallest shapes that reach each instantiation with a partial row tile and
# N = q NT + 1; K at the minimum of the branch (16; 48 for the ring; 512 for the long-product skinny threshold) or odd where the kernel zero-fills the K tail
# (19, 35: three chunks = the 1x1 loop with two chunks in flight, 67 with 64-channel chunks).
CONV_CASES = [
    (13, 257, 19, 3, 2, 128, ALLV, "16,1,4,1,4,16"),
    (29, 130817, 35, 1, 1, 128, ("plain", "relu-mask1-pre.1"), "32,1,2,1,4,16"),
    (29, 129, 19, 5, 1, 128, ALLV, "32,1,1,1,4,16"),
    (129, 24577, 48, 1, 1, 128, ("plain", "tanh-acc-beta-nobias", "relu-mask1-pre.1"), "32,2,2,2,2,16,true"),
    (65, 4097, 48, 1, 1, 128, ALLV, "32,1,1,2,2,16,true"),
    (65, 16257, 16, 3, 1, 128, ALLV, "32,1,2,2,2,16"),
    (65, 32641, 35, 1, 1, 128, ("plain",), "32,1,2,2,2,16"),
    (65, 101, 67, 1, 1, 128, ALLV, "32,1,1,1,4,64"),
    (65, 65, 19, 3, 3, 0, ALLV, "32,1,1,2,2,16"),
    (65, 129, 35, 1, 1, 128, ("plain", "gelu-res-alpha-1-mask4-pre0"), "32,1,1,2,2,16"),
    (65, 65281, 16, 3, 1, 128, ("plain", "tanh-acc-beta-nobias"), "32,2,2,1,4,16"),
    (37, 21, 16, 1, 1, 128, ALLV, "skinny<1,16>"),
    (513, 513, 16, 1, 1, 128, ALLV, "skinny<2,16>"),
    (65, 4097, 512, 1, 1, 128, ("plain", "relu-mask1-pre.1"), "skinny<2,16>"),
    (37, 21, 16, 3, 1, 128, ALLV, "skinny_taps"),
    (37, 49, 32, 5, 2, 128, ALLV, "skinny_taps"),
    (29, 129, 19, 5, 2, 128, ("plain", "relu-mask1-pre.1"), "32,1,1,1,4,16", 8),
    (65, 65, 19, 3, 3, 0, ("plain", "gelu-res-alpha-1-mask4-pre0"), "32,1,1,2,2,16", 0),
    (37, 21, 16, 3, 1, 128, ("plain", "tanh-acc-beta-nobias"), "skinny_taps", 0),
    (37, 49, 32, 5, 2, 128, ("plain", "relu-mask1-pre.1"), "skinny_taps", 8),
]
# conv_plain on cl_parts 2 / 1 / 3 (k >= 3): the k-major conv_cl launch
CL_CASES = [
    (37, 257, 19, 5, 1, 2, ALLV, "cl_km<1,bf16x3>"),
    (65, 300, 16, 3, 2, 2, ALLV, "cl_km<1,bf16x3>"),
    (65, 16129, 16, 3, 1, 2, ALLV, "cl_km<2,bf16x3>"),
    (37, 257, 19, 5, 1, 1, ("plain", "gelu-res-alpha-1-mask4-pre0"), "cl_km<1,bf16>"),
    (65, 16129, 16, 3, 1, 1, ("plain", "relu-mask1-pre.1"), "cl_km<2,bf16>"),
    (37, 257, 19, 5, 1, 3, ("plain", "tanh-acc-beta-nobias"), "cl_km<1,f16>"),
    (65, 16129, 16, 3, 1, 3, ("plain", "gelu-res-alpha-1-mask4-pre0"), "cl_km<2,f16>"),
    (37, 257, 19, 5, 1, 2, ("plain", "relu-mask1-pre.1"), "cl_km<1,bf16x3>", 4),
    (65, 300, 16, 3, 2, 2, ("plain", "gelu-res-alpha-1-mask4-pre0"), "cl_km<1,bf16x3>", 0),
]
# (parts code, M, N, K, ksplit, instantiation)
BFS_CASES = [
    (4, 65, 16260, 16, 1, "2,1,2,2,2,1,4,true"),
    (4, 65, 68, 2048, 1, "2,1,1,2,2,1,8,true,true"),
    (4, 33, 36, 512, 1, "2,1,1,1,1,1,4,true,false,4"),
    (4, 65, 68, 16, 1, "2,1,1,2,2,1,8,true"),
    (4, 65, 68, 2048, 0, "2,1,1,2,2,1,8,true"),
    (2, 65, 68, 16, 1, "2,1,1,2,2,1,8"),
    (2, 129, 8068, 96, 1, "2,2,2,2,2,2,4"),
    (2, 129, 8068, 48, 1, "2,2,2,2,2,1,5"),
    (2, 129, 16388, 32, 1, "2,2,2,2,2,1,5"),
    (3, 65, 68, 16, 1, "3,1,1,2,2,1,6"),
    (3, 129, 8068, 16, 1, "3,2,2,2,2,1,6"),
    (3, 129, 16388, 16, 1, "3,2,2,2,2,1,3"),
]
# linear_tokmajor: (tokens L = M, cout = N, cin = K, ldy, skinny_max, instantiation)
TOK_CASES = [
    (66, 192, 192, 192, 128, "skinny<1,16>"),
    (66, 192, 192, 196, 0, "32,1,1,2,2,16,true"),
    (66, 100, 35, 100, 128, "32,1,1,1,4,64"),
    (66, 100, 35, 103, 128, "32,1,1,1,4,64"),
    (13, 70, 19, 72, 128, "16,1,4,1,4,16"),
    (29, 129, 19, 132, 128, "32,1,1,1,4,16"),
]
# the encoders' FFN pair: (H, F, k, L, skinny_max): conv_km_to_cl (channels-last epilogue) then conv_cl_to_km on conv_cl_small (small grids) / conv_cl
FFN_CASES = [(20, 48, 3, 300, 128), (20, 48, 3, 300, 0), (70, 80, 5, 521, 128), (70, 80, 5, 521, 0)]


def _pad(c):
    return c[8] if len(c) > 8 else c[4] * (c[3] - 1) // 2


def _conv_id(c):
    return f"M{c[0]}-N{c[1]}-K{c[2]}-k{c[3]}-d{c[4]}-{c[7]}" + ("" if c[5] == 128 else f"-skinny{c[5]}") + (f"-pad{c[8]}" if len(c) > 8 else "")


def _cl_id(c):
    return f"M{c[0]}-N{c[1]}-K{c[2]}-k{c[3]}-d{c[4]}-{c[7]}" + (f"-pad{c[8]}" if len(c) > 8 else "")


def prof_name(name):
    """what the library's launch profile (csrc/gemm_conv.hip: kCfgNames, cfg_id) calls the kernel of a mirror's answer: the tiled kernels by MF, TM, TN, WM
    (the ring and the 64-channel chunk share their tile's entry), every skinny kernel as one, conv_cl by layout, row tiling and precision"""
    if name.startswith("skinny"):
        return "gemm_skinny<16x16x4>"
    if name.startswith("cl_km"):
        tm, prec = name[6:-1].split(",")
        return f"conv_cl_km<{tm},{'split-bf16' if prec == 'bf16x3' else prec}>"
    a = name.split(",")
    return "conv_gemm<" + ",".join(a[:5] + ["16"]) + ">"


def _bfs_id(c):
    return f"M{c[1]}-N{c[2]}-K{c[3]}-{'ksplit' if c[4] else 'unsplit'}-<{c[5]}>"


def _span(k, dil, pad_l):
    smin, smax = -pad_l, (k - 1) * dil - pad_l
    return smax - (smin // 4) * 4


# ---- references: one dtype-parametrised statement per operation ---------------------------------------------------------------------------------------------

def _gelu_tanh(x):
    return 0.5 * x * (1.0 + np.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


def epilogue(v, dt, bias=None, act=ACT_NONE, alpha=1.0, res=None, beta=1.0, prev=None, mask=None, mask_div=1, wrong=None):
    """bias, act, alpha, residual, beta, accumulate, mask"""
    if bias is not None:
        v = v + bias.astype(dt)[:, None]
    if wrong == "res_before_alpha" and res is not None:
        v = v + res.astype(dt)
    if act == ACT_RELU:
        v = np.maximum(v, dt(0))
    elif act == ACT_GELU:
        v = _gelu_tanh(v) if wrong == "gelu_tanh" else O.gelu(v)
    elif act == ACT_TANH:
        v = np.tanh(v)
    v = v * dt(np.float32(alpha))
    if res is not None and wrong != "res_before_alpha":
        v = v + res.astype(dt)
    v = v * dt(np.float32(beta))
    if prev is not None:
        v = v + prev.astype(dt)
    if mask is not None:
        n = np.arange(v.shape[1])
        keep = mask[np.minimum(n, len(mask) - 1)] if wrong == "mask_no_div" else mask[n // mask_div]
        v = v * keep.astype(dt)[None, :]
    return v


def conv_sum(x, w, dil, pad_l, dt, pre_slope=1.0, wrong=None, seam=None):
    """sum_ci sum_j w[co][ci][j] lrelu(x, pre_slope)[ci][n + j dil - pad_l], zero outside [0, L): one matmul per tap"""
    x = x.astype(dt)
    if pre_slope != 1.0:
        x = O.leaky_relu(x, pre_slope)
    w = w.astype(dt)
    cout, cin, k = w.shape
    L = x.shape[1]
    y = np.zeros((cout, L), dt)
    for j in range(k):
        s = j * dil - pad_l + (1 if wrong == "shift_off_one" and j == 0 else 0)
        lo, hi = max(0, -s), min(L, L - s)
        if hi > lo:
            y[:, lo:hi] += w[:, :, k - 1 - j if wrong == "taps_reversed" else j] @ x[:, lo + s:hi + s]
    if wrong == "seam_copy":
        y[:, seam] = y[:, seam - 1]
    return y


def conv_ref(x, w, dil, pad_l, dt, pre_slope=1.0, wrong=None, seam=None, **epi):
    return epilogue(conv_sum(x, w, dil, pad_l, dt, pre_slope, wrong, seam), dt, wrong=wrong, **epi)


def abs_sum(x, w, dil, pad_l, pre_slope=1.0):
    """sum |w| |lrelu(x)| (float64): what the operand-rounding bounds scale with"""
    return conv_sum(np.abs(O.leaky_relu(x.astype(np.float64), pre_slope)), np.abs(w.astype(np.float64)), dil, pad_l, np.float64)


def _lip(act=ACT_NONE, alpha=1.0, beta=1.0, **_):
    return (GELU_SLOPE if act == ACT_GELU else 1.0) * abs(alpha) * abs(float(np.float32(beta)))


def tol_f32(ref, ref32):
    err32 = float(np.abs(ref32.astype(np.float64) - ref).max())
    return max(4 * err32, 8 * EPS32 * float(np.abs(ref).max()))


def tol_split(c, S, ref, ref32, epi):
    err32 = float(np.abs(ref32.astype(np.float64) - ref).max())
    return c * S * _lip(**epi) + 4 * err32 + 1e-37


def parts_bound(y, code):
    return (2.0 ** -24 + EPS32) * np.abs(y.astype(np.float64)) + 1e-37 if code == 3 else _split_bound(y, code)


def _bf16_parts(a, n):
    """the first n bf16 parts of a (round to nearest even, each of what the previous ones left), as float32"""
    out, r = [], a.astype(np.float32)
    for _ in range(n):
        u = r.view(np.uint32).astype(np.uint64)
        h = (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(np.float32)
        out.append(h)
        r = (r - h).astype(np.float32)
    return out


def _first_part(a, family):
    return a.astype(np.float16).astype(np.float32) if "f16" in family else _bf16_parts(a, 1)[0]


def ys_sentinel(code):
    """what the hooks' recombination makes of untouched parts (every 16-bit word 0x5A5A)"""
    if code == 4:
        h = np.array([0x5A5A], np.uint16).view(np.float16).astype(np.float32)[0]
        return np.float32(h + np.float32(h * np.float32(1.0 / 2048.0)))
    v = np.array([0x5A5A0000], np.uint32).view(np.float32)[0]
    acc = np.float32(0)
    for _ in range(code):
        acc = np.float32(acc + v)
    return acc


# ---- data -------------------------------------------------------------------------------------------------------------------------------------------------

def conv_data(M, N, K, k, kind, seed, epi):
    """x, w and the epilogue operands of one launch; kind: normal | offset (x + 100, mixed-sign weights: the result cancels) | impulseA / impulseB (x zero but
    for single ones: A at columns 0, NT - 1, 2 NT - 1, B at NT, 2 NT, L - 1, each in a channel of its own so that responses do not overlap)"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((K, N))
    if kind == "offset":
        x = x + 100.0
    w = (rng.standard_normal((M, K, k)) / math.sqrt(K * k)).astype(np.float32)
    d = dict(epi)
    d["bias"] = rng.standard_normal(M).astype(np.float32) if d.get("bias", True) else None
    d["res"] = rng.standard_normal((M, N)).astype(np.float32) if d.get("res") else None
    d["prev"] = rng.standard_normal((M, N)).astype(np.float32) if d.pop("accumulate", False) else None
    md = d.get("mask_div")
    if md:
        d["mask"] = (rng.random(_cdiv(N, md)) > 0.3).astype(np.uint8)
    else:
        d.pop("mask_div", None)
    return x.astype(np.float32), w, d


def impulses(K, N, nt, which):
    cols = [0, nt - 1, 2 * nt - 1] if which == "A" else [nt, 2 * nt, N - 1]
    x = np.zeros((K, N), np.float32)
    for i, c in enumerate(sorted({c for c in cols if 0 <= c < N})):
        x[i % K, c] = 1.0
    return x


# ---- CPU part ------------------------------------------------------------------------------------------------------------------------------------------------

def test_hooks_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "sbv2_hip.h")).read()
    l = _lib.lib()
    for name in HOOKS + ["sbv2_debug_conv1d", "sbv2_debug_gemm_bfs", "sbv2_debug_gemm_bfs_alt"]:
        assert re.search(r"\bint " + name + r"\(", hdr), name
        assert name in _lib.SYMBOLS and getattr(l, name).restype is C.c_int, name
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", hdr).group(1)
        assert len(decl.split(",")) == len(_lib.SYMBOLS[name][1]), name   # as many argtypes as declared parameters


def test_mirrors_match_the_sources():
    src = open(os.path.join(CSRC, "gemm_conv.hip")).read()
    body = src[src.index("void launch_conv(const ConvParams& p"):]
    sites = re.findall(r"launch_cfg<([^>]*)>\(kp", body)
    assert {s.replace(" ", "") for s in sites} == CONV_ALL
    for line, why in UNREACHABLE.items():
        assert body.count(line) == 2 and why     # the reachable twin and the dead one
    assert len(sites) == 12 and "launch_gemm_skinny(p, kp.mask_shift, stream)" in body and "launch_gemm_skinny_taps(p, kp.mask_shift, stream)" in body
    sk = open(os.path.join(CSRC, "gemm_skinny.hip")).read()
    assert set(re.findall(r"launch_skinny<(\d+), (\d+)>\(kp", sk)) == {("1", "16"), ("2", "16")} and "gemm_skinny_taps_kernel, grid" in sk
    bfs = open(os.path.join(CSRC, "gemm_bfs.hip")).read()
    bbody = bfs[bfs.index("void launch_gemm_bfs(const GemmBfsParams& p"):]
    assert {s.replace(" ", "") for s in re.findall(r"launch_bfs_cfg<([^>]*)>\(kp", bbody)} == BFS_ALL
    # the thresholds the mirrors restate
    for text in ("blocks(64, 64) < (p.K >= 512 ? skinny_max + skinny_max / 2 : skinny_max)", "blocks(128, 128) >= 384 && blocks(128, 128) <= 512",
                 "blocks(64, 128) >= 512", "blocks(64, 64) < 128 && Nx <= 128", "blocks(64, 256) >= 512", "blocks(64, 128) >= 256", "blocks(32, 256) >= 512",
                 "p.K >= 48"):
        assert text in body, text
    for text in ("blocks(128, 128) >= 128", "blocks(128, 128) <= ncu", "nch >= 128", "nch / (ks * 2) >= 32", "nch % 4 == 0 && nch >= 32 && blocks(32, 32) <= ncu"):
        assert text in bbody, text


def test_cases_cover_the_dispatch():
    for c in CONV_CASES:
        M, N, K, k, dil, smax, _, name = c[:8]
        assert conv_kernel(M, N, K, k, _span(k, dil, _pad(c)), smax) == name and 0 <= _pad(c) <= (k - 1) * dil, c
        nt = _nt(name)
        assert N % nt in (1, 5, N) or N < nt, c            # N = q NT + 1 (or one partial tile)
    reached = {c[7] for c in CONV_CASES}
    assert reached == CONV_ALL | SKINNY_ALL
    # a causal and a look-ahead window on a tiled kernel, the taps kernel and the k-major conv_cl: floor4(min shift) differs from the symmetric case's
    for cases, names in ((CONV_CASES, ("32,", "skinny_taps")), (CL_CASES, ("cl_km",))):
        for pre in names:
            pads = {(_pad(c) == 0, _pad(c) == (c[3] - 1) * c[4]) for c in cases if len(c) > 8 and c[7].startswith(pre)}
            assert pads == {(True, False), (False, True)}, pre
    assert prof_name("32,1,1,1,4,64") == "conv_gemm<32,1,1,1,4,16>" and prof_name("32,2,2,2,2,16,true") == "conv_gemm<32,2,2,2,2,16>"
    assert prof_name("cl_km<1,bf16x3>") == "conv_cl_km<1,split-bf16>" and prof_name("cl_km<2,f16>") == "conv_cl_km<2,f16>"
    names = open(os.path.join(CSRC, "gemm_conv.hip")).read()
    for c in CONV_CASES + CL_CASES:
        assert '"' + prof_name(c[7]) + '"' in names, c[7]
    # what the mirror can return at all: a sweep over shapes finds nothing outside the two sets
    seen = set()
    for M in (1, 16, 17, 32, 33, 64, 65, 129, 513, 4096):
        for N in (1, 16, 100, 128, 129, 4097, 24577, 32641, 65281, 130817):
            for K in (16, 19, 48, 512):
                for k in (1, 3):
                    for smax in (0, 128):
                        seen.add(conv_kernel(M, N, K, k, 4, smax))
    assert seen == CONV_ALL | SKINNY_ALL
    for c in CL_CASES:
        assert cl_kernel(c[0], c[1], c[5]) == c[7] and c[3] >= 3, c
    assert {c[7] for c in CL_CASES} == {f"cl_km<{t},{p}>" for t in (1, 2) for p in ("bf16x3", "bf16", "f16")}
    for c in BFS_CASES:
        assert bfs_kernel(c[0], c[1], c[2], c[3], c[4]) == c[5], c
        assert c[2] % 4 == 0 and c[3] % 16 == 0
    assert {c[5] for c in BFS_CASES} == BFS_ALL
    seen = {bfs_kernel(p, M, N, K, ks) for p in (2, 3, 4) for M in (1, 65, 129, 1024) for N in (4, 68, 8068, 16388) for K in (16, 48, 512, 2048, 4096)
            for ks in (0, 1)}
    assert seen == BFS_ALL
    for L, cout, cin, ldy, smax, name in TOK_CASES:
        assert conv_kernel(L, cout, cin, 1, 0, smax) == name
    # every feature meets a small tile, a large tile, the scalar epilogue, a ring, both skinny kernels and the k-major conv_cl
    for must in ("32,1,1,1,4,16", "32,1,2,2,2,16", "16,1,4,1,4,16", "32,1,1,2,2,16,true", "skinny<1,16>", "skinny_taps"):
        assert any(c[7] == must and set(c[6]) == set(ALLV) for c in CONV_CASES), must
    assert any(set(c[6]) == set(ALLV) for c in CL_CASES if c[7] == "cl_km<1,bf16x3>") and any(set(c[6]) == set(ALLV) for c in CL_CASES if c[7] == "cl_km<2,bf16x3>")
    feats = [VARIANTS[v] for v in ALLV]
    assert {f.get("act", 0) for f in feats} == {0, 1, 2, 3} and {f.get("mask_div") for f in feats} >= {1, 4}
    assert {f.get("pre_slope", 1.0) for f in feats} == {1.0, 0.1, 0.0} and any(f.get("alpha") == -1.0 and f.get("res") for f in feats)
    assert any(f.get("accumulate") and f.get("beta") == 1.0 / 3.0 for f in feats) and any(f.get("bias") is False for f in feats)


def test_reference_agrees_with_the_oracle():
    rng = np.random.default_rng(5)
    for k, dil in ((1, 1), (3, 1), (5, 2), (7, 3)):
        x = rng.standard_normal((7, 50)).astype(np.float32)
        w = rng.standard_normal((5, 7, k)).astype(np.float32)
        b = rng.standard_normal(5).astype(np.float32)
        got = conv_ref(x, w, dil, dil * (k - 1) // 2, np.float64, pre_slope=0.1, bias=b)
        want = O.conv1d_same(O.leaky_relu(x.astype(np.float64), 0.1), w.astype(np.float64), b.astype(np.float64), dil)
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
    assert abs(max(0.5 * (1 + math.erf(t / math.sqrt(2))) + t * math.exp(-t * t / 2) / math.sqrt(2 * math.pi) for t in np.linspace(0, 4, 4001)) - 1.129) < 1e-3
    assert SENTINEL.view(np.uint32) == 0x5A5A5A5A


# tolerance families: name -> (operand-rounding constant or None for the f32 bound, f32-grade?)
FAMILIES = {"f32": (None, True), "cl_bf16x3": (C_BF16X3, False), "cl_bf16": (C_BF16, False), "cl_f16": (C_F16, False), "bfs_bf16x3": (C_BF16X3, False),
            "bfs_f16x3": (C_F16X3, True), "bfs_bf16x6": (C_BF16X6, True), "ffn_cl_bf16x3": (C_BF16X3, False)}
STRUCTURAL = ("taps_reversed", "shift_off_one", "mask_no_div", "res_before_alpha", "seam_copy")


@pytest.mark.parametrize("family", list(FAMILIES))
def test_wrong_references_exceed_the_tolerance(family):
    """On the data of a small case of the family (k = 3 convolution for the conv families, the 1x1 product for gemm_bfs): taps reversed, the first tap's shift
    off by one, the mask indexed without mask_div, the residual added before alpha, one tile-seam column copied from its neighbour (every family; 1x1
    products have no taps to reverse or shift); one hi * lo cross term of one tap dropped (the split families); GELU's tanh approximation for its erf form
    (the f32-grade families and bf16x3: the approximation is 4.7e-4 off, inside what plain bf16 / f16 operands allow, so those two families cannot see it).
    bf16x6 drops w_hi * x_lo with x_lo the THIRD part (2^-16 of x): one term of the six-term product, not the first part's whole remainder.
    The FFN family: see _ffn_wrong_references."""
    if family.startswith("ffn"):
        return _ffn_wrong_references()
    c, f32_grade = FAMILIES[family]
    bfs = family.startswith("bfs")
    M, N, K, k, dil = (65, 68, 16, 1, 1) if bfs else (37, 300, 16, 3, 1)
    pad_l = dil * (k - 1) // 2
    seam = 64 if bfs else (256 if family.startswith("cl") else 128)
    epi = dict(res=True, alpha=-1.0, mask_div=4, act=ACT_GELU)
    x, w, d = conv_data(M, N, K, k, "normal", 77, epi)

    def tol_of(ref, ref32, e):
        return tol_f32(ref, ref32) if c is None else tol_split(c, abs_sum(x, w, dil, pad_l), ref, ref32, e)

    ref, ref32 = conv_ref(x, w, dil, pad_l, np.float64, **d), conv_ref(x, w, dil, pad_l, np.float32, **d)
    tol = tol_of(ref, ref32, d)
    assert (np.abs(ref32 - ref) / tol).max() <= 0.25 + 1e-9 or c is None
    kinds = [s for s in STRUCTURAL if not (bfs and s in ("taps_reversed", "shift_off_one"))]
    if f32_grade or c == C_BF16X3:
        kinds.append("gelu_tanh")
    for wrong in kinds:
        bad = conv_ref(x, w, dil, pad_l, np.float64, wrong=wrong, seam=seam, **d)
        assert (np.abs(bad - ref) / tol).max() > 1.0, wrong
    if c is not None and family not in ("cl_bf16", "cl_f16"):
        # the product without w_hi * x_lo on the middle tap (x_lo = what the first part leaves), plain epilogue
        d0 = dict(bias=d["bias"])
        ref0, ref032 = conv_ref(x, w, dil, pad_l, np.float64, **d0), conv_ref(x, w, dil, pad_l, np.float32, **d0)
        j = k // 2
        s = j * dil - pad_l
        x_lo = (_bf16_parts(x, 3)[2] if family == "bfs_bf16x6" else x - _first_part(x, family)).astype(np.float64)
        w_hi = _first_part(w[:, :, j].copy(), family).astype(np.float64)
        term = np.zeros_like(ref0)
        lo, hi = max(0, -s), min(N, N - s)
        term[:, lo:hi] = w_hi @ x_lo[:, lo + s:hi + s]
        assert (np.abs(term) / tol_of(ref0, ref032, d0)).max() > 1.0, "cross term"


def ffn_data(H, F, k, L, kind):
    rng = np.random.default_rng(H + F + L + len(kind))
    x = (rng.standard_normal((H, L)) + (100.0 if kind == "offset" else 0.0)).astype(np.float32)
    w1 = (rng.standard_normal((F, H, k)) / math.sqrt(H * k)).astype(np.float32)
    w2 = (rng.standard_normal((H, F, k)) / math.sqrt(F * k)).astype(np.float32)
    b1, b2 = rng.standard_normal(F).astype(np.float32), rng.standard_normal(H).astype(np.float32)
    res = rng.standard_normal((H, L)).astype(np.float32)
    mask = (rng.random(L) > 0.2).astype(np.uint8)
    return x, w1, b1, w2, b2, res, mask


def ffn_mid_ref(x, w1, b1, mask, pad, dt):
    return conv_ref(x, w1, 1, pad, dt, bias=b1, mask=mask, mask_div=1)


def ffn_out_ref(mid, w2, b2, res, mask, pad, dt, pre_slope=0.0, wrong=None):
    """the second convolution on a given intermediate (the tests pass the one the hook returned): ReLU as pre_slope 0, bias, residual, mask"""
    return conv_ref(mid, w2, 1, pad, dt, pre_slope=pre_slope, wrong=wrong, bias=b2, res=res, mask=mask, mask_div=1)


def ffn_out_tol(mid, w2, pad, y64, y32):
    return tol_split(C_BF16X3, abs_sum(mid, w2, 1, pad, 0.0), y64, y32, {})


def _ffn_wrong_references():
    """The output bound of test_conv_ffn_cl on the data of its cases, with a float32 rounding of the reference intermediate standing in for the hook's: the
    second convolution with its taps reversed, its first tap shifted, w_hi * relu(mid)_lo dropped on its middle tap, and a leaky slope of 0.001 where the
    ReLU belongs must each exceed it."""
    for H, F, k, L in sorted({c[:4] for c in FFN_CASES}):
        pad = (k - 1) // 2
        x, w1, b1, w2, b2, res, mask = ffn_data(H, F, k, L, "normal")
        mid = ffn_mid_ref(x, w1, b1, mask, pad, np.float64).astype(np.float32)
        y64, y32 = ffn_out_ref(mid, w2, b2, res, mask, pad, np.float64), ffn_out_ref(mid, w2, b2, res, mask, pad, np.float32)
        tol = ffn_out_tol(mid, w2, pad, y64, y32)
        keep = mask != 0
        for wrong in ("taps_reversed", "shift_off_one"):
            bad = ffn_out_ref(mid, w2, b2, res, mask, pad, np.float64, wrong=wrong)
            assert (np.abs(bad - y64) / tol)[:, keep].max() > 1.0, (wrong, H, F)
        bad = ffn_out_ref(mid, w2, b2, res, mask, pad, np.float64, pre_slope=0.001)
        assert (np.abs(bad - y64) / tol)[:, keep].max() > 1.0, ("slope", H, F)
        j = k // 2
        r = np.maximum(mid, 0)
        r_lo = (r - _bf16_parts(r, 1)[0]).astype(np.float64)
        term = conv_sum(r_lo, _bf16_parts(w2[:, :, j:j + 1].copy(), 1)[0], 1, 0, np.float64)
        assert (np.abs(term) / tol)[:, keep].max() > 1.0, ("cross term", H, F)


# ---- GPU part ------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def device():
    import torch
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    assert ncu == NCU, f"the cases were built for {NCU} compute units (launch_gemm_bfs' `lone` test reads the device's count), this device has {ncu}"
    return 0


class _Skinny:
    def __init__(self, v):
        self.v = v

    def __enter__(self):
        self.prev = _lib.lib().sbv2_debug_set_skinny_max(self.v)

    def __exit__(self, *a):
        _lib.lib().sbv2_debug_set_skinny_max(self.prev)


class _Ksplit:
    def __init__(self, v):
        self.v = v

    def __enter__(self):
        self.prev = _lib.lib().sbv2_debug_set_ksplit(self.v)

    def __exit__(self, *a):
        _lib.lib().sbv2_debug_set_ksplit(self.prev)


class _Prof:
    """the kernels the library's launch profile saw inside the block"""
    def __enter__(self):
        _lib.check(_lib.lib().sbv2_prof_begin())
        self.kernels = set()
        return self

    def __exit__(self, *a):
        buf = C.create_string_buffer(1 << 14)
        _lib.check(_lib.lib().sbv2_prof_end(buf, len(buf)))
        rec = [r for r in json.loads(buf.value.decode()) if r["launches"] > 0]
        self.kernels, self.launches = {r["kernel"] for r in rec}, sum(r["launches"] for r in rec)


def _conv_plain(x, w, dil, pad_l, cl_parts, bias=None, act=ACT_NONE, pre_slope=1.0, res=None, alpha=1.0, beta=1.0, prev=None, mask=None, mask_div=1):
    M, K, k = w.shape
    N = x.shape[1]
    y = np.empty((M, N), np.float32) if prev is None else prev.copy()
    stray = C.c_int64(-1)
    xs, ws, bs, rs = _c32(x), _c32(w), _c32(bias), _c32(res)
    _lib.check(_lib.lib().sbv2_debug_conv_plain(0, _f(xs), _f(ws), _f(bs), K, M, k, N, dil, pad_l, cl_parts, _u8p(mask), mask_div, act, pre_slope, _f(rs),
                                               alpha, float(np.float32(beta)), int(prev is not None), _f(y), C.byref(stray)))
    return y, stray.value


def _check_masked(y, d):
    if d.get("mask") is not None:
        keep = d["mask"][np.arange(y.shape[1]) // d["mask_div"]]
        assert not np.any(y[:, keep == 0]), "a masked column is not exactly zero"


def _run_conv_case(case, cl_parts, c):
    M, N, K, k, dil, smax, variants, name = case[:8]
    pad_l = _pad(case)
    worst = 0.0
    runs = [(v, "normal") for v in variants] + [("plain", "offset")]
    for vi, (vname, kind) in enumerate(runs):
        x, w, d = conv_data(M, N, K, k, kind, 1000 * M + N + 7 * vi, VARIANTS[vname])
        with _Prof() as prof:
            y, stray = _conv_plain(x, w, dil, pad_l, cl_parts, **d)
        assert prof.kernels == {prof_name(name)}, f"the mirror names {name}, the library ran {prof.kernels}"
        ref, ref32 = conv_ref(x, w, dil, pad_l, np.float64, **d), conv_ref(x, w, dil, pad_l, np.float32, **d)
        tol = tol_f32(ref, ref32) if c is None else tol_split(c, abs_sum(x, w, dil, pad_l, d.get("pre_slope", 1.0)), ref, ref32, d)
        assert np.isfinite(y).all(), f"{vname}/{kind}: a NaN or infinity reached the output (poisoned pads)"
        worst = max(worst, _report(f"{name} M{M} N{N} K{K} k{k} {vname}/{kind}", np.abs(y - ref), tol))
        assert stray == 0, f"{vname}/{kind}: {stray} pad words changed"
        _check_masked(y, d)
    # impulses: the response is f32(w[:, c, tap] + bias) at column - shift[tap] and the bias elsewhere, exactly, on the f32 path
    rng = np.random.default_rng(M + N)
    w = (rng.standard_normal((M, K, k)) / math.sqrt(K * k)).astype(np.float32)
    b = rng.standard_normal(M).astype(np.float32)
    for which in "AB":
        x = impulses(K, N, _nt(name), which)
        y, stray = _conv_plain(x, w, dil, pad_l, cl_parts, bias=b)
        ref = conv_ref(x, w, dil, pad_l, np.float64, bias=b)
        assert stray == 0
        if c is None:
            hits = conv_sum(x, np.ones_like(w), dil, pad_l, np.float64)
            assert hits.max() <= 1.0          # no two responses overlap: every output is one rounding of w + bias
            np.testing.assert_array_equal(y, ref.astype(np.float32), err_msg=f"impulses {which}")
        else:
            tol = tol_split(c, abs_sum(x, w, dil, pad_l), ref, ref.astype(np.float32), {})
            worst = max(worst, _report(f"{name} impulses {which}", np.abs(y - ref), tol))
    assert worst <= 1.0, worst


@gpu
@pytest.mark.parametrize("case", CONV_CASES, ids=_conv_id)
def test_conv_plain_f32(case, device):
    with _Skinny(case[5]):
        _run_conv_case(case, 0, None)


@gpu
@pytest.mark.parametrize("case", CL_CASES, ids=_cl_id)
def test_conv_plain_cl_km(case, device):
    _run_conv_case(case[:5] + (128,) + case[6:], case[5], {2: C_BF16X3, 1: C_BF16, 3: C_F16}[case[5]])


@gpu
@pytest.mark.parametrize("case", TOK_CASES, ids=[f"L{c[0]}-cout{c[1]}-cin{c[2]}-ldy{c[3]}-{c[5]}" for c in TOK_CASES])
def test_linear_tokmajor(case, device):
    L, cout, cin, ldy, smax, name = case
    worst = 0.0
    for kind in ("normal", "offset", "nobias"):
        rng = np.random.default_rng(L + cout + cin + len(kind))
        x = (rng.standard_normal((cin, L)) + (100.0 if kind == "offset" else 0.0)).astype(np.float32)
        w = (rng.standard_normal((cout, cin)) / math.sqrt(cin)).astype(np.float32)
        b = None if kind == "nobias" else rng.standard_normal(cout).astype(np.float32)
        y = np.empty((L, cout), np.float32)
        stray = C.c_int64(-1)
        with _Skinny(smax):
            _lib.check(_lib.lib().sbv2_debug_linear_tokmajor(0, _f(x), _f(w), _f(b), cin, cout, L, ldy, _f(y), C.byref(stray)))

        def ref_of(dt):
            v = x.astype(dt).T @ w.astype(dt).T
            return v if b is None else v + b.astype(dt)[None, :]
        ref, ref32 = ref_of(np.float64), ref_of(np.float32)
        assert np.isfinite(y).all()
        worst = max(worst, _report(f"linear_tokmajor {name} L{L} cout{cout} cin{cin} ldy{ldy} {kind}", np.abs(y - ref), tol_f32(ref, ref32)))
        assert stray.value == 0, f"{stray.value} words outside y changed"
    assert worst <= 1.0


@gpu
@pytest.mark.parametrize("H,F,k,L,smax", FFN_CASES, ids=[f"H{c[0]}-F{c[1]}-k{c[2]}-L{c[3]}-{'cl_small' if c[4] else 'conv_cl'}" for c in FFN_CASES])
def test_conv_ffn_cl(H, F, k, L, smax, device):
    """conv_km_to_cl (channels-last epilogue: bias, mask; no activation) then conv_cl_to_km with the ReLU as pre_slope = 0 and the residual, split-bf16.
    The intermediate is held to the float64 first convolution; the output to the second convolution of the intermediate the hook returned, with that
    convolution's own bound (module docstring).  Which kernels ran: two conv_cl launches with a k-major side in the profile (conv_cl_small reports there too)."""
    worst = 0.0
    pad = (k - 1) // 2
    for kind in ("normal", "offset"):
        x, w1, b1, w2, b2, res, mask = ffn_data(H, F, k, L, kind)
        y, mid = np.empty((H, L), np.float32), np.empty((F, L), np.float32)
        stray = C.c_int64(-1)
        with _Skinny(smax), _Prof() as prof:
            _lib.check(_lib.lib().sbv2_debug_conv_ffn_cl(0, _f(x), _f(w1), _f(b1), _f(w2), _f(b2), H, F, k, L, _u8p(mask), _f(res), _f(y), _f(mid),
                                                        C.byref(stray)))
        assert prof.launches == 2 and all(n.startswith("conv_cl_km<") and n.endswith("split-bf16>") for n in prof.kernels), prof.kernels
        assert np.isfinite(y).all() and np.isfinite(mid).all()
        m64, m32 = ffn_mid_ref(x, w1, b1, mask, pad, np.float64), ffn_mid_ref(x, w1, b1, mask, pad, np.float32)
        worst = max(worst, _report(f"ffn H{H} F{F} k{k} L{L} {kind} mid", np.abs(mid - m64), tol_split(C_BF16X3, abs_sum(x, w1, 1, pad), m64, m32, {})))
        y64, y32 = ffn_out_ref(mid, w2, b2, res, mask, pad, np.float64), ffn_out_ref(mid, w2, b2, res, mask, pad, np.float32)
        worst = max(worst, _report(f"ffn H{H} F{F} k{k} L{L} {kind} out", np.abs(y - y64), ffn_out_tol(mid, w2, pad, y64, y32)))
        assert stray.value == 0
        assert not np.any(mid[:, mask == 0]) and not np.any(y[:, mask == 0])
    assert worst <= 1.0


def _bfs(x, w, code, bias=None, res=None, act=ACT_NONE, split_out=0, mask=None, mask_div=1, alpha=1.0, beta=1.0, y_rows=-1, ys_row0=0, want_y=1):
    M, K = w.shape
    N = x.shape[1]
    y, ys = np.empty((M, N), np.float32), np.empty((M, N), np.float32)
    stray, ms = C.c_int64(-1), C.c_float()
    _lib.check(_lib.lib().sbv2_debug_gemm_bfs_ex(0, _f(_c32(x)), _f(_c32(w)), _f(_c32(bias)), _f(_c32(res)), M, N, K, code, act, split_out, 0, _u8p(mask),
                                                mask_div, alpha, beta, y_rows, ys_row0, want_y, _f(y), _f(ys) if split_out else None, C.byref(ms),
                                                C.byref(stray)))
    return y, ys, stray.value


@gpu
@pytest.mark.parametrize("case", BFS_CASES, ids=_bfs_id)
def test_gemm_bfs_epilogues(case, device):
    """Every launch_bfs_cfg instantiation with what the models pass: a mask (mask_div 4: the generic epilogue; 1: the interior one), a residual with alpha /
    beta, y_rows / ys_row0 off the 32-row sub-tile (generic) and on it (interior), parts only (Y = nullptr) with GELU, offset data and impulses."""
    code, M, N, K, ks, name = case
    c = {2: C_BF16X3, 3: C_BF16X6, 4: C_F16X3}[code]
    rng = np.random.default_rng(code * 100000 + M + N + K)
    w = (rng.standard_normal((M, K)) / math.sqrt(K)).astype(np.float32)
    bias = rng.standard_normal(M).astype(np.float32)
    res = rng.standard_normal((M, N)).astype(np.float32)
    xn = rng.standard_normal((K, N)).astype(np.float32)
    xo = (xn + 100.0).astype(np.float32)
    nt = 32 * int(name.split(",")[2]) * int(name.split(",")[4])     # columns per workgroup tile
    xi = np.maximum(impulses(K, N, nt, "A"), impulses(K, N, nt, "B"))   # (a 1x1 product: columns do not mix)
    r_odd = M // 2 + 3
    m4, m1 = (rng.random(_cdiv(N, 4)) > 0.3).astype(np.uint8), (rng.random(N) > 0.3).astype(np.uint8)
    launches = [
        ("mask4-res-alpha-beta-rows", xn, dict(bias=bias, res=res, alpha=-1.0, beta=0.5, mask=m4, mask_div=4, split_out=code, y_rows=r_odd, ys_row0=r_odd)),
        ("parts-only-gelu-mask1", xn, dict(act=ACT_GELU, mask=m1, mask_div=1, split_out=code, want_y=0)),
        ("relu-res-rows32", xn, dict(bias=bias, act=ACT_RELU, res=res, split_out=code, y_rows=32, ys_row0=32)),
        ("offset", xo, dict(bias=bias)),
        ("impulses", xi, dict(bias=bias)),
    ]
    worst = 0.0
    w3 = w[:, :, None]
    with _Ksplit(ks):
        for lname, x, a in launches:
            with _Prof() as prof:
                y, ys, stray = _bfs(x, w, code, **a)
            assert prof.kernels == {"gemm_bfs<" + {2: "bf16x3", 3: "bf16x6", 4: "f16x3"}[code] + ">"}, prof.kernels
            epi = {k_: v for k_, v in a.items() if k_ in ("bias", "res", "act", "alpha", "beta", "mask", "mask_div")}
            ref, ref32 = conv_ref(x, w3, 1, 0, np.float64, **epi), conv_ref(x, w3, 1, 0, np.float32, **epi)
            tol = tol_split(c, abs_sum(x, w3, 1, 0), ref, ref32, epi)
            yr = M if a.get("y_rows", -1) < 0 else a["y_rows"]
            if a.get("want_y", 1):
                assert np.isfinite(y[:yr]).all(), lname
                worst = max(worst, _report(f"bfs<{name}> {lname} f32 plane", np.abs(y[:yr] - ref[:yr]), tol[:yr]))
                assert np.all(y[yr:].view(np.uint32) == 0x5A5A5A5A), f"{lname}: rows >= y_rows were written"
                _check_masked(y[:yr], epi)
            else:
                assert np.all(y.view(np.uint32) == 0x5A5A5A5A), f"{lname}: an f32 plane was written without one being passed"
            if a.get("split_out"):
                r0 = a.get("ys_row0", 0)
                assert np.isfinite(ys[r0:]).all(), lname
                worst = max(worst, _report(f"bfs<{name}> {lname} parts", np.abs(ys[r0:] - ref[r0:]), tol[r0:] + parts_bound(ref[r0:], code)))
                if a.get("want_y", 1) and yr > r0:       # against the f32 plane of the same launch: the split alone
                    worst = max(worst, _report(f"bfs<{name}> {lname} parts vs plane", np.abs(ys[r0:yr] - y[r0:yr]), parts_bound(y[r0:yr], code)))
                assert np.all(ys[:r0] == ys_sentinel(code)), f"{lname}: parts rows < ys_row0 were written"
                _check_masked(ys[r0:], epi)
            assert stray == 0, f"{lname}: {stray} pad words changed"
    assert worst <= 1.0
