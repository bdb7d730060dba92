"""Repeatability screen of the inline-asm MFMA kernels under load: respair_x16.hip, respair_clx.hip, resbranch_clx.hip, conv_clx.hip (plain, the
phased upsamplers and the flow FFN pair), attn_flash.hip's k_vits_flash_x3q and gemm_bfs.hip's f16x3 batch and K-split instantiations.

The hazards DESIGN 4.2 records for these loops (a VALU write consumed by an MFMA without wait states, v_permlane32_swap sunk between its consumers, a ds_read
landing in the source registers of a queued MFMA) are invisible to the compiler and depend on how deep MFMAs queue and when VALU results become visible, i.e.
on what else runs on the CU.  The other kernel tests launch once or twice on an idle chip with a few dozen workgroups.  Here every instance is launched
REPS = 100 times back to back on one stream (csrc/test_hooks.cpp: run_repeated), alternately on two inputs and two output planes, the output restored by a
device-to-device copy before each repetition (the previous contents under accumulate, NaN otherwise), and a comparison kernel counts after each repetition the
32-bit words that differ from the FIRST result of the same input.  The kernels have no floating-point atomics and no order-dependent reduction, so bit
equality is an exact oracle: mismatch[i] == 0 for every repetition.  Two regimes per instance:
  (a) full chip: the smallest N whose grid is at least 256 CUs x the kernel's resident workgroups per CU, plus one partial tile; no neighbour, the pressure
      is the kernel's own co-resident workgroups;
  (b) quarter chip (a grid of 64 workgroups, N no multiple of the tile) while a second stream receives, from the same host loop, alternately a LayerNorm
      [1024][8192] and a gemm_bfs f16x3 product 1024 x 1024 x 2048 (the batch instantiation): the other execution context of production.  The two streams
      are fed from one host loop, launch by launch; nothing paces one against the other (the screen must not poll), so that they overlapped in time is by
      enqueue order only and was NOT observed (no trace was taken): the neighbour may run ahead of a backlogged stream or finish before it.
Sizes come from the launchers' tile geometry, mirrored below and compared with the sources by the CPU part.  Workgroups per CU are DERIVED (160 KB of LDS
per CU over the configuration's LDS bytes, at most 32 waves per CU: an upper bound, registers could only lower it); they are not measured here and nobody has
measured them at these shapes.
The launch profile (sbv2_prof_begin / _end) names the family bucket that ran and its launch count.  respair_x16 and respair_clx share the buckets
respair_cl<C=64> / respair_cl<C<=32>, so the profile cannot tell the two apart; the hook's variant does: 3 = launch_respair_x16, which refuses what
respair_x16.hip does not take instead of falling back, 2 = launch_respair_clx.  resbranch_clx is counted in the same buckets, and at C = 128 with
conv_clx<split-bf16>; launch_resbranch has no other kernel to fall back to.

The first result of each input is also held against float64: the whole plane in regime (b); in regime (a) position windows (both ends, the first / a
middle / the last tile boundary, four random ones; 512 positions each = 4608; masked columns lie in every one of them: the mask drops 15 % of the 4-column
groups), each evaluated on its span widened by the chain's reach sum d (k - 1) / 2, zero padding only at the plane's true ends.  The fused step is DESIGN's
y = keep (conv2(lrelu(keep (conv1(lrelu(x), d) + b1))) + b2 + x), result keep (beta y [+ previous]); the branch is three of them.
Tolerance per element, conventions of tests/test_gemm_conv_kernels.py: c = 3 * 2^-16 (bf16x3); one convolution c (|w| conv |operand|); a chain to first
order on the bounds (lrelu: Lipschitz 1): E_t = c (|w1| conv |lrelu x|) + |w1| conv E_x, E_y = c (|w2| conv |lrelu t|) + |w2| conv E_t + E_x, the result
|beta| E_y, + 4 err32 (the same reference in float32).  That bound grows by sum |w| = 0.8 sqrt(C k) per convolution: fine for one step, but through the
six convolutions of a branch it reaches 5 .. 90 around values of rms 1.3 and sees nothing.  So a second bound is held as well, on every chain, which rests on
ASSUMPTIONS, not on a derivation: the same graph run on VARIANCES (V_t = c^2 (w1^2 conv lrelu(x)^2) + w1^2 conv V_x, V_y = c^2 (w2^2 conv lrelu(t)^2) + w2^2 conv V_t + V_x), tolerance 8 sqrt(V) |beta|
+ 4 err32.  Assumed: the roundings of distinct operand elements are independent and of either sign, so their variances add where the first-order bound adds
magnitudes; c, a bound of one product's relative error, stands in for its standard deviation (larger than it); 8 standard deviations over the 10^7 elements of
a plane leaves no room for chance, and sum w^2 = 1 for these weights, so the bound does not grow along the chain.  Masked columns are exactly zero.  conv_clx's parts planes hold the split of lrelu(its own f32 result).
Deliberately wrong references (one tap's dilation off by one, lrelu missing on the intermediate / the operand, beta before the residual, the mask only at the
end) must exceed the tolerance on the same data (CPU part).

The phased upsamplers, gemm_bfs, k_vits_flash_x3q and the flow FFN pair have their own sections below (references and tolerances of tests/test_gpu_parity.py's
statement, tests/test_gemm_conv_kernels.py and tests/test_attention_kernels.py, by import); where a launcher cannot start the grids of the two regimes, the
section says which grid is run instead and why.  sbv2_debug_conv_ffn_cl's conv_km_to_cl / conv_cl_to_km launch conv_cl.hip, so the FFN pair is screened as
VitsModel::run_encoder launches it on conv_clx.hip, with the weights from that hook's builders.

Record of the first green run on an MI355X: RECORD below (kernel bucket the profile named, grids, reps, mismatches, worst error / tolerance ratios, seconds
per family).
"""
import ctypes as C
import json
import os
import re
import zlib

import numpy as np
import pytest

import sbv2_oracle as O
from sbv2_api_amd import _lib
import test_attention_kernels as A
import test_gemm_conv_kernels as G
from test_ops_kernels import _report, _split_bound

gpu = pytest.mark.gpu
f32p, i64p = _lib.f32p, _lib.i64p
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sbv2-api_amd", "csrc")
NCU, LDS_CU, WAVES_CU = 256, 160 * 1024, 32
REPS = 100
C_BF16X3 = 3 * 2.0 ** -16
SLOPE = 0.1
DILS = (1, 3, 5)
HOOKS = ["sbv2_debug_repeat_respair", "sbv2_debug_repeat_resbranch", "sbv2_debug_repeat_conv1d_clx", "sbv2_debug_repeat_conv_transpose1d_clx",
         "sbv2_debug_repeat_gemm_bfs", "sbv2_debug_repeat_vits_attention", "sbv2_debug_repeat_conv_ffn_clx"]

RECORD = """First green run on an MI355X (256 CUs): reps = 100 everywhere, 0 mismatches in every case of every family, every flip case saw exactly its one word.
Profile buckets (100 launches each; + 50 gemm_bfs<f16x3> launches of the neighbour in regime (b)): respair_x16 / respair_clx / resbranch_clx: respair_cl<C=64>
at C = 64, respair_cl<C<=32> below; resbranch_clx at C = 128 and conv_clx: conv_clx<split-bf16>; the upsamplers: conv_cl<2,split-bf16> (where the profile has
always counted transposed convolutions); the FFN pair: conv_clx_ffn<split-bf16>, 200; gemm_bfs: gemm_bfs<f16x3>; attention: not recorded by the profile.
Grids (a) / (b): respair_x16 776 / 64; respair_clx 1032 (C = 16), 776 (C = 64) / 64; resbranch_clx 1288, 776, 264, 264 (C = 16, 32, 64, 128 at k = 3), 520 (C = 16,
k = 7 / 11) / 64; conv_clx 784 (C = 128), 800 (C = 256), 528 / 544 for k = 11 at dilation 5 (320-row windows, two per CU) / 64; up2 896 / 128 (64 working);
up4 784 / 64; FFN pair 3168 + 792 / 96 + 24; gemm_bfs batch 784 / 128, K split 256 / 64; k_vits_flash_x3q 256 (8 waves) / 64 (4 waves).
Worst error / tolerance (first-order | 8-sigma where a chain has both) and seconds per family (all its cases, host reference included):
  respair_x16: 0.015 | 0.059, 3.4 s
  respair_clx: 0.031 | 0.062, 1.0 s
  resbranch_clx: 0.000 | 0.060, 6.1 s
  conv_clx: 0.065, 10.7 s
  conv_clx_up2: 0.065, 1.7 s
  conv_clx_up4: 0.060, 1.5 s
  conv_clx_ffn: 0.003 | 0.055, 1.2 s
  gemm_bfs: 0.400, 1.5 s
  k_vits_flash_x3q: 0.015, 0.8 s
"""


def _cdiv(a, b):
    return -(-a // b)


def _up(a, b):
    return _cdiv(a, b) * b


# ---- the launchers' geometry, mirrored (X6Cfg, RpxCfg, RbCfg, launch_clx_e) ---------------------------------------------------------------------------------

def x16_cfg(C_, k):
    """respair_x16.hip: X6Cfg<C, NTAPS> and launch_x6 -> (outputs per workgroup, waves, LDS bytes)"""
    nch, nmt, wn = C_ // 16, C_ // 32, 2 if C_ == 64 else 4
    nw, nt = nmt * wn, 64 * wn
    t = 64 * nw
    wreg, rb = 2 * nch * 2048, t // 4
    rows1, rows2 = _cdiv(nt + 64, rb) * rb, nt + k + 1
    xreg = max(2 * 2 * rows1 * 32, 2 * nch * rows2 * 32)
    main = max(wreg + xreg, nw * 64 * 36 * 4)
    return nt - (k - 1), nw, _up(main + 512 + rows2 + 16, 16)


def rpx_cfg(C_, k):
    """respair_clx.hip: RpxCfg<C, NTAPS, GT> with launch_respair_clx's GT (2 at C = 64, else 4) and launch_rpx"""
    gt = 2 if C_ == 64 else 4
    nch, nmt, wn, two = C_ // 16, 2 if C_ == 64 else 1, 2 if C_ == 64 else 4, C_ == 16
    nw, nt = nmt * wn, 64 * wn
    t = 64 * nw
    ntw = (k + 1) // 2 if two else k
    g = min(ntw, gt)
    wreg, rb = 2 * g * nmt * 2048, t // 4
    rows1, rows2 = _cdiv(nt + 64, rb) * rb, nt + k + 1
    x1half = _up(rows1 * 16, 256) if two else rows1 * 16 + 64
    x2half = _up(rows2 * 16, 256) if two else rows2 * 16
    xreg = max(2 * 2 * x1half, 2 * nch * 2 * x2half)
    main = max(wreg + xreg, nw * 64 * (20 if two else 36) * 4)
    return nt - (k - 1), nw, _up(main + 512 + rows2 + 16, 16)


RB_INSTANCES = {(128, 3): (3, 3, 2), (64, 3): (6, 3, 3), (32, 3): (4, 4, 3), (16, 3): (4, 4, 3), (16, 7): (8, 4, 3), (16, 11): (8, 6, 3)}   # (WN, GT, NBUF)


def rb_cfg(C_, k, dils=DILS):
    """resbranch_clx.hip: RbCfg<C, NTAPS, WN, GT, NBUF> of launch_resbranch's instance and launch_rb (outputs = window rows - 2 halo)"""
    wn, gt, nbuf = RB_INSTANCES[(C_, k)]
    nch, nmt, two = C_ // 16, C_ // 32 if C_ >= 32 else 1, C_ == 16
    nw, r = nmt * wn, 64 * wn
    ntw = (k + 1) // 2 if two else k
    g = min(ntw, gt)
    wreg = nbuf * g * nmt * 2048
    marg = 6 if k <= 3 else ((5 * (k - 1) // 2 + 1) & ~1)
    xrows = r + 2 * marg
    xhalf = _up(xrows * 16, 256) if two else xrows * 16
    xreg = 2 * nch * 2 * xhalf
    main = max(wreg + xreg, nw * 64 * (20 if two else 36) * 4)
    halo = sum((d + 1) * (k - 1) // 2 for d in dils)
    return r - 2 * halo, nw, _up(main + 2 * 3 * C_ * 4 + r, 16)


def clx_cfg(k, dil):
    """conv_clx.hip: launch_conv_clx's window choice (288 rows while 256 + tap span fits, else 320) and launch_clx_e's LDS: 256 positions x 64 rows, 4 waves"""
    xr = 288 if 256 + dil * (k - 1) <= 288 else 320
    return 256, 4, max(4 * 4096 + 2 * 2 * xr * 32, 4 * 64 * 36 * 4)


def residency(nw, lds):
    """workgroups per CU, derived: what LDS and the wave slots of a CU admit.  An upper bound: the kernels ask for amdgpu_waves_per_eu(3) / (2), i.e. registers
    for AT LEAST that many waves per SIMD, and registers can only lower the count, so a grid of 256 x this many workgroups fills the chip either way.  Not
    measured."""
    return max(1, min(LDS_CU // lds, WAVES_CU // nw))


def tiled_grid(N, nto):
    return _up(_cdiv(N, nto), 8)          # launch_x6 / launch_rpx / launch_rb: ((ntiles + 7) >> 3) * 8


def clx_grid(N, M):
    return _up(_cdiv(N, 256), 8) * (M // 64)    # launch_clx_e: round_up(ceil(N / 256), 8) * gy


def tiled_N(regime, nto, res):
    """(a): 256 x residency whole tiles and a partial one; (b): 60 whole tiles and a partial one = a grid of 64"""
    return (NCU * res if regime == "a" else 60) * nto + nto // 2 + 1


def clx_N(regime, M, res):
    gy = M // 64
    ntx = _up(_cdiv(NCU * res, gy), 8) if regime == "a" else 64 // gy
    return (ntx if regime == "a" else ntx - 1) * 256 + 129


# ---- the instances ------------------------------------------------------------------------------------------------------------------------------------------
# variants: plain, and a column mask (mask_div 4) + beta 1/3 + accumulate
PLAIN, FULL = "plain", "mask4-beta-acc"


def _cases():
    out = []
    for regime in "ab":
        for C_ in (32, 64):
            for k in (7, 11):
                nto, nw, lds = x16_cfg(C_, k)
                for var, dil in ((PLAIN, 3), (FULL, 5)):
                    out.append(dict(fam="respair_x16", C=C_, k=k, dil=dil, var=var, regime=regime, nto=nto, res=residency(nw, lds),
                                    N=tiled_N(regime, nto, residency(nw, lds)), variant=3, bucket="respair_cl<C=64>" if C_ == 64 else "respair_cl<C<=32>"))
        for C_, k in ((16, 7), (64, 3)):
            nto, nw, lds = rpx_cfg(C_, k)
            for var, dil in ((PLAIN, 3), (FULL, 5)):
                out.append(dict(fam="respair_clx", C=C_, k=k, dil=dil, var=var, regime=regime, nto=nto, res=residency(nw, lds),
                                N=tiled_N(regime, nto, residency(nw, lds)), variant=2, bucket="respair_cl<C=64>" if C_ == 64 else "respair_cl<C<=32>"))
        for C_, k in ((16, 3), (32, 3), (64, 3), (128, 3), (16, 7), (16, 11)):
            nto, nw, lds = rb_cfg(C_, k)
            for var in (PLAIN, FULL):
                out.append(dict(fam="resbranch_clx", C=C_, k=k, dil=DILS, var=var, regime=regime, nto=nto, res=residency(nw, lds),
                                N=tiled_N(regime, nto, residency(nw, lds)),
                                bucket="conv_clx<split-bf16>" if C_ == 128 else ("respair_cl<C=64>" if C_ == 64 else "respair_cl<C<=32>")))
        for C_ in (128, 256):
            for k in (3, 7, 11):
                for var, dil in (("ys", 3), ("res-beta", 5)):
                    nto, nw, lds = clx_cfg(k, dil)
                    out.append(dict(fam="conv_clx", C=C_, k=k, dil=dil, var=var, regime=regime, nto=nto, res=residency(nw, lds),
                                    N=clx_N(regime, C_, residency(nw, lds)), bucket="conv_clx<split-bf16>"))
    for c in out:
        c["grid"] = clx_grid(c["N"], c["C"]) if c["fam"] == "conv_clx" else tiled_grid(c["N"], c["nto"])
    return out


CASES = _cases()


def _up_cases():
    """the phased upsamplers (build_upx): rows = phases x cout (gy = rows / 64), 288-row windows: three workgroups per CU.  launch_clx_e rounds the position
    tiles up to 8, so the 2-tap form (16 row blocks) cannot start fewer than 128 workgroups: regime (b) gives it 4 position tiles = 64 WORKING workgroups
    (the other 64 find no tile and leave)"""
    out = []
    for regime in "ab":
        for name, cin, cout, k, s in (("up2", 256, 128, 16, 8), ("up4", 128, 64, 8, 2)):
            gy, (_, nw, lds) = s * cout // 64, clx_cfg(3, 1)
            res = residency(nw, lds)
            tiles = _up(_cdiv(NCU * res, gy), 8) if regime == "a" else 64 // gy - 1
            for var in ("ys", "mask4"):
                N = tiles * 256 + 129
                out.append(dict(fam="conv_clx_" + name, cin=cin, C=cout, k=k, s=s, var=var, regime=regime, N=N, nto=256, res=res, gy=gy,
                                grid=_up(_cdiv(N, 256), 8) * gy, work=_cdiv(N, 256) * gy, bucket="conv_cl<2,split-bf16>"))
    return out


def _bfs_cases():
    """gemm_bfs f16x3: the batch instantiation (64 x 128 tiles, a 4-slot ring of 12 KB slots = 48 KB: three per CU; launch_gemm_bfs takes it from 128 blocks of
    128 x 128 on, so its smallest grid is 128 workgroups: regime (b)) and the small-grid K split (64 x 64 tiles x up to 8 K groups, capped by the launcher at
    one workgroup per CU: regime (a) is that cap, 256 workgroups, DeBERTa's FFN down projection at 68 columns)"""
    return [dict(fam="gemm_bfs", inst="2,1,2,2,2,1,4,true", M=1024, K=1024, N=(NCU * 3 // 16) * 128 + 68, regime="a", res=3, nto=128, grid=16 * (NCU * 3 // 16 + 1)),
            dict(fam="gemm_bfs", inst="2,1,2,2,2,1,4,true", M=64, K=1024, N=127 * 128 + 68, regime="b", res=3, nto=128, grid=128),
            dict(fam="gemm_bfs", inst="2,1,1,2,2,1,8,true,true", M=1024, K=4096, N=68, regime="a", res=1, nto=64, grid=256),
            dict(fam="gemm_bfs", inst="2,1,1,2,2,1,8,true,true", M=256, K=4096, N=68, regime="b", res=1, nto=64, grid=64)]


UP_CASES, BFS_CASES = _up_cases(), _bfs_cases()


def _id(c):
    if c["fam"] == "gemm_bfs":
        return f"gemm_bfs<{c['inst']}>-M{c['M']}-N{c['N']}-K{c['K']}-{c['regime']}"
    return f"{c['fam']}-C{c['C']}-k{c['k']}-{c['var']}-{c['regime']}"


# ---- references ---------------------------------------------------------------------------------------------------------------------------------------------

def lrelu(x, slope=SLOPE):
    return O.leaky_relu(x, slope)


def _tap(x, wj, shift):
    """the contribution of ONE tap: y[:, n] += wj @ x[:, n + shift] (zero outside)"""
    L = x.shape[1]
    y = np.zeros((wj.shape[0], L), x.dtype)
    lo, hi = max(0, -shift), min(L, L - shift)
    if hi > lo:
        y[:, lo:hi] = wj @ x[:, lo + shift:hi + shift]
    return y


def conv(x, w, b, dil, wrong=None):
    y = O.conv1d_same(x, w, b, dil)
    if wrong == "tap-dilation":     # the last tap reads one position further out
        k = w.shape[2]
        s = dil * (k - 1) // 2
        y = y - _tap(x, w[:, :, k - 1], s) + _tap(x, w[:, :, k - 1], s + 1)
    return y


def chain_ref(x, steps, keep, beta, prev, dt, wrong=None, bound=False):
    """The fused steps (w1, b1, w2, b2, dilation) in a row on x [C][L]; keep [L] in {0, 1}.  bound: also the two error bounds of the module docstring (the
    first-order one, and 8 standard deviations of the same graph run on variances)."""
    cast = lambda a: None if a is None else np.asarray(a, dt)
    y, kp = cast(x), cast(keep)[None, :]
    E = V = np.zeros_like(y) if bound else None
    A, S, cs = np.abs, np.square, O.conv1d_same
    for q, (w1, b1, w2, b2, d) in enumerate(steps):
        w1, b1, w2, b2 = cast(w1), cast(b1), cast(w2), cast(b2)
        last = q + 1 == len(steps)
        a = lrelu(y)
        t = conv(a, w1, b1, d, wrong if last else None)
        if wrong != "mask-end":
            t = kp * t
        u = t if (wrong == "no-lrelu" and last) else lrelu(t)
        z = cs(u, w2, b2, 1)
        if bound:
            Et = kp * (C_BF16X3 * cs(A(a), A(w1), None, d) + cs(E, A(w1), None, d))
            E = kp * (C_BF16X3 * cs(A(u), A(w2), None, 1) + cs(Et, A(w2), None, 1) + E)
            Vt = kp * (C_BF16X3 ** 2 * cs(S(a), S(w1), None, d) + cs(V, S(w1), None, d))
            V = kp * (C_BF16X3 ** 2 * cs(S(u), S(w2), None, 1) + cs(Vt, S(w2), None, 1) + V)
        y = dt(beta) * z + y if (wrong == "beta-first" and last) else z + y
        if last:
            if wrong != "beta-first":
                y = dt(beta) * y
            if prev is not None:
                y = y + cast(prev)
            y = kp * y
        elif wrong != "mask-end":
            y = kp * y
    return (y, abs(beta) * E, abs(beta) * 8.0 * np.sqrt(V)) if bound else y


def clx_ref(x, w, b, res, dil, beta, dt, wrong=None, bound=False):
    """conv_clx: y = beta (conv(lrelu(x), d) + b + res); one convolution: the first-order bound serves as both"""
    cast = lambda a: None if a is None else np.asarray(a, dt)
    x, w, b, res = cast(x), cast(w), cast(b), cast(res)
    a = x if wrong == "no-lrelu" else lrelu(x)
    z = conv(a, w, b, dil, wrong)
    r = 0 if res is None else res
    y = dt(beta) * z + r if wrong == "beta-first" else dt(beta) * (z + r)
    if not bound:
        return y
    E = abs(beta) * C_BF16X3 * O.conv1d_same(np.abs(a), np.abs(w), None, dil)
    return y, E, E


def reach(c):
    k = c["k"]
    if c["fam"] == "conv_clx":
        return c["dil"] * (k - 1) // 2
    dils = c["dil"] if c["fam"] == "resbranch_clx" else (c["dil"],)
    return sum((d + 1) * (k - 1) // 2 for d in dils)


def windows(c, rng, W=512):
    """regime (a): [s, e) position windows of W columns: both ends, the first / a middle / the last tile boundary, four random ones"""
    N, nto = c["N"], c["nto"]
    nt = _cdiv(N, nto)
    starts = [0, N - W] + [b * nto - W // 2 for b in (1, nt // 2, nt - 1)] + [int(v) for v in rng.integers(0, N - W, 4)]
    return [(max(0, min(s, N - W)), max(0, min(s, N - W)) + W) for s in starts]


def on_windows(fn, N, wins, R, scale=1):
    """fn(lo, hi) evaluates the reference on columns [lo, hi) as if they were a whole plane and returns arrays [C][hi - lo]; the columns within R of a cut end
    that is not the plane's end see zero padding where the plane has data and are dropped (scale: output columns per position: the upsamplers).  Returns one
    tuple of arrays per window."""
    out = []
    for s, e in wins:
        lo, hi = max(0, s - R), min(N, e + R)
        out.append(tuple(a[:, (s - lo) * scale:(e - lo) * scale] for a in fn(lo, hi)))
    return out


# ---- data ---------------------------------------------------------------------------------------------------------------------------------------------------

def make_data(c, seed=None):
    C_, k, N = c["C"], c["k"], c["N"]
    rng = np.random.default_rng(seed if seed is not None else zlib.crc32(_id(c).encode()))
    sd = 1.0 / np.sqrt(C_ * k)
    d = dict(rng=rng, xa=rng.standard_normal((C_, N), np.float32), xb=rng.standard_normal((C_, N), np.float32))
    if c["fam"] == "conv_clx":
        d["w"], d["b"] = (rng.standard_normal((C_, C_, k)) * sd).astype(np.float32), rng.standard_normal(C_).astype(np.float32)
        d["res"] = rng.standard_normal((C_, N), np.float32) if c["var"] == "res-beta" else None
        d["beta"] = float(np.float32(1.0 / 3)) if c["var"] == "res-beta" else 1.0
        return d
    nsteps = 3 if c["fam"] == "resbranch_clx" else 1
    d["w"] = (rng.standard_normal((2 * nsteps, C_, C_, k)) * sd).astype(np.float32)
    d["b"] = rng.standard_normal((2 * nsteps, C_)).astype(np.float32)
    dils = c["dil"] if nsteps == 3 else (c["dil"],)
    d["steps"] = [(d["w"][2 * q], d["b"][2 * q], d["w"][2 * q + 1], d["b"][2 * q + 1], dils[q]) for q in range(nsteps)]
    full = c["var"] == FULL
    d["mask"] = (rng.random(_cdiv(N, 4)) > 0.15).astype(np.uint8) if full else None
    d["keep"] = np.repeat(d["mask"], 4)[:N].astype(np.float32) if full else np.ones(N, np.float32)
    d["xa"] *= d["keep"][None, :]      # (a masked column holds zeros in the real planes)
    d["xb"] *= d["keep"][None, :]
    d["prev"] = rng.standard_normal((C_, N), np.float32) if full else None
    d["beta"] = float(np.float32(1.0 / 3)) if full else 1.0
    return d


def reference(c, d, x, lo, hi, dt, wrong=None, bound=False):
    sl = lambda a: None if a is None else a[..., lo:hi]
    if c["fam"] == "conv_clx":
        return clx_ref(sl(x), d["w"], d["b"], sl(d["res"]), c["dil"], d["beta"], dt, wrong, bound)
    return chain_ref(sl(x), d["steps"], sl(d["keep"]), d["beta"], sl(d["prev"]), dt, wrong, bound)


def tolerance(c, d, x, lo, hi):
    """(float64 reference, first-order tolerance, 8-sigma tolerance) on columns [lo, hi) taken as a whole plane"""
    ref, E, S8 = reference(c, d, x, lo, hi, np.float64, bound=True)
    e32 = 4.0 * np.abs(reference(c, d, x, lo, hi, np.float32).astype(np.float64) - ref)
    return ref, E + e32, S8 + e32


# ---- CPU part -----------------------------------------------------------------------------------------------------------------------------------------------

def test_hooks_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "sbv2_hip.h")).read()
    src = open(os.path.join(CSRC, "test_hooks.cpp")).read()
    for h in HOOKS:
        assert re.search(rf"\bint {h}\(", hdr), f"{h} is not declared in include/sbv2_hip.h"
        assert re.search(rf"\bint {h}\(", src), f"{h} is not defined in csrc/test_hooks.cpp"
        assert h in _lib.SYMBOLS, f"{h} is not bound in _lib.py"
        assert len(_lib.SYMBOLS[h][1]) == len(re.search(rf"\bint {h}\(([^)]*)\)", hdr).group(1).split(",")), f"{h}: argument count"


def test_mirrors_match_the_sources():
    rd = lambda n: open(os.path.join(CSRC, n)).read()
    x16, rpx, rb, clx = rd("respair_x16.hip"), rd("respair_clx.hip"), rd("resbranch_clx.hip"), rd("conv_clx.hip")
    for src in (x16, rpx):
        assert "constexpr int nto = K::NT - (NTAPS - 1);" in src and "const int grid = ((ntiles + 7) >> 3) * 8;" in src
    assert "const int nto = K::R - 2 * p.halo;" in rb and "const int grid = ((ntiles + 7) >> 3) * 8;" in rb
    assert "halo += (p.dil[q] + 1) * (p.k - 1) / 2;" in rb
    for (C_, k), (wn, gt, nbuf) in RB_INSTANCES.items():
        assert f"launch_rb<{C_}, {k}, {wn}, {gt}, {nbuf}>(p, stream)" in rb
    assert "launch_rpx<64, 3, 2>" in rpx and "launch_rpx<CC, KK, 4>" in rpx
    assert "kp.gy = p.M / 64;" in clx and "const int ntx = round_up((p.N + kClxNT - 1) / kClxNT, 8);" in clx and "constexpr int kClxNT = 256;" in clx
    assert "if (kp.xrows <= 288) {" in clx and "(size_t)WR * 4096 + (size_t)XB * 2 * XR * 32" in clx
    # what the launchers' own comments and static_asserts say about LDS and workgroups per CU
    for C_ in (32, 64):
        for k in (7, 11):
            assert x16_cfg(C_, k)[2] * 3 <= LDS_CU and x16_cfg(C_, k)[1] == 4          # static_assert(K::LDS * 3 <= 160 * 1024); T == 256
    assert rpx_cfg(64, 3)[2] // 1024 <= 52 and residency(*rpx_cfg(64, 3)[1:]) == 3         # "52 KB of LDS, three workgroups per CU"
    # (launch_resbranch's comment says 155 / 137 / 59 / 74 KB; RbCfg's arithmetic gives)
    assert [round(rb_cfg(C_, k)[2] / 1024) for C_, k in ((128, 3), (64, 3), (16, 7), (16, 11))] == [153, 137, 59, 73]
    assert [residency(*rb_cfg(C_, k)[1:]) for C_, k in ((128, 3), (64, 3), (32, 3), (16, 3), (16, 7), (16, 11))] == [1, 1, 3, 5, 2, 2]   # (C = 16, k = 3: LDS would take five; the launcher's comment counts three)
    assert [rb_cfg(C_, k)[0] for C_, k in ((16, 3), (64, 3), (128, 3), (16, 7), (16, 11))] == [232, 360, 168, 440, 392]
    assert [residency(*clx_cfg(k, d)[1:]) for k, d in ((3, 5), (7, 5), (11, 3), (11, 5))] == [3, 3, 3, 2]   # "52 KB, THREE workgroups per CU ... (76 KB), two"
    assert [x16_cfg(64, 7)[0], x16_cfg(64, 11)[0], x16_cfg(32, 7)[0], x16_cfg(32, 11)[0], rpx_cfg(16, 7)[0]] == [122, 118, 250, 246, 250]


def test_grid_sizes_of_the_regimes():
    """every regime (a) case reaches 256 x residency workgroups with a partial last tile, every regime (b) case 48 .. 80; every family and instance is there"""
    assert len({_id(c) for c in CASES}) == len(CASES)
    for c in CASES:
        tile = 256 if c["fam"] == "conv_clx" else c["nto"]
        assert c["N"] % tile, _id(c)
        if c["regime"] == "a":
            assert c["grid"] >= NCU * c["res"], (_id(c), c["grid"])
            whole = c["N"] // tile               # ... with the fewest whole tiles that do, and one partial tile behind them
            if c["fam"] == "conv_clx":
                gy = c["C"] // 64
                assert whole % 8 == 0 and whole * gy >= NCU * c["res"] > (whole - 8) * gy, _id(c)
            else:
                assert whole == NCU * c["res"], _id(c)
        else:
            assert 48 <= c["grid"] <= 80, (_id(c), c["grid"])
        assert c["N"] * c["C"] < 2 ** 31
    fams = {(c["fam"], c["C"], c["k"]) for c in CASES}
    assert {("respair_x16", C_, k) for C_ in (32, 64) for k in (7, 11)} | {("respair_clx", 16, 7), ("respair_clx", 64, 3)} <= fams
    assert {("resbranch_clx", C_, 3) for C_ in (16, 32, 64, 128)} | {("resbranch_clx", 16, 7), ("resbranch_clx", 16, 11)} <= fams
    assert {("conv_clx", C_, k) for C_ in (128, 256) for k in (3, 7, 11)} <= fams


WRONG = ("tap-dilation", "no-lrelu", "beta-first", "mask-end")
WRONG_CASES = [("respair_x16", 32, 7), ("respair_x16", 64, 11), ("respair_clx", 16, 7), ("resbranch_clx", 16, 3), ("resbranch_clx", 64, 3), ("resbranch_clx", 128, 3),
               ("resbranch_clx", 16, 11), ("conv_clx", 128, 3), ("conv_clx", 256, 11)]


@pytest.mark.parametrize("fam,C_,k", WRONG_CASES)
def test_wrong_references_exceed_the_tolerance(fam, C_, k):
    """A reference with one tap's dilation off by one, without lrelu on the intermediate (conv_clx: on its operand), with beta before the residual, or with the
    mask only at the end (conv_clx has no mask) lies outside the tolerance of the right one on the same data.  On the fused step and on conv_clx that is the
    first-order bound.  On resbranch_clx the first-order bound cannot see them: it grows by sum |w| = 0.8 sqrt(C k) per convolution, six in a row, and reaches
    5 .. 90 around values of rms 1.3 (C = 16 .. 128); there the 8-sigma bound (no growth: sum w^2 = 1) is the one they must exceed."""
    c = dict(fam=fam, C=C_, k=k, dil=DILS if fam == "resbranch_clx" else 3, var="res-beta" if fam == "conv_clx" else FULL, regime="b", N=601, nto=100)
    d = make_data(c, seed=5)
    ref, tol, tol8 = tolerance(c, d, d["xa"], 0, c["N"])
    keep = d.get("keep", np.ones(c["N"])) > 0
    assert np.all(tol[:, keep] > 0) and np.all(tol8[:, keep] > 0)
    for wrong in WRONG[:3 if fam == "conv_clx" else 4]:
        err = np.abs(reference(c, d, d["xa"], 0, c["N"], np.float64, wrong=wrong) - ref)[:, keep]
        assert (err / tol8[:, keep]).max() > 1.0, (fam, wrong)
        if fam != "resbranch_clx":
            assert (err / tol[:, keep]).max() > 1.0, (fam, wrong)


def test_window_evaluation_equals_the_whole_plane():
    """a window widened by the chain's reach gives the whole plane's values (to float64 rounding: BLAS blocks another shape differently), also at the plane's ends"""
    c = dict(fam="resbranch_clx", C=16, k=3, dil=DILS, var=FULL, regime="a", N=3001, nto=232)
    d = make_data(c, seed=6)
    whole = reference(c, d, d["xa"], 0, c["N"], np.float64)
    wins = windows(c, d["rng"])
    assert sum(e - s for s, e in wins) >= 4096 and wins[0][0] == 0 and wins[1][1] == c["N"]
    for (s, e), (got,) in zip(wins, on_windows(lambda lo, hi: (reference(c, d, d["xa"], lo, hi, np.float64),), c["N"], wins, reach(c))):
        np.testing.assert_allclose(got, whole[:, s:e], rtol=0, atol=1e-13)


# ---- GPU part -----------------------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def device():
    import torch
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    assert ncu == NCU, f"the grids were sized for {NCU} compute units, this device has {ncu}"
    return 0


def _f(a):
    return None if a is None else a.ctypes.data_as(f32p)


class _Prof:
    """launches per kernel bucket that the library's launch profile saw inside the block"""
    def __enter__(self):
        _lib.check(_lib.lib().sbv2_prof_begin())
        self.launches = {}
        return self

    def __exit__(self, *a):
        buf = C.create_string_buffer(1 << 14)
        _lib.check(_lib.lib().sbv2_prof_end(buf, len(buf)))
        self.launches = {r["kernel"]: r["launches"] for r in json.loads(buf.value.decode()) if r["launches"] > 0}


def launch(c, d, reps=REPS, flip_at=-1, flip_word=0):
    """-> first results ya, yb as [C][N] (conv_clx: also the parts' sums ysa, ysb, else None), mismatch [reps], first_bad [reps], the profile"""
    C_, N, k = c["C"], c["N"], c["k"]
    nb = int(c["regime"] == "b")
    mm, fb = np.full(reps, -7, np.int64), np.full(reps, -7, np.int64)
    P64 = lambda a: a.ctypes.data_as(i64p)
    lib = _lib.lib()
    ysa = ysb = None
    with _Prof() as prof:
        if c["fam"] == "conv_clx":
            ya, yb = np.empty((C_, N), np.float32), np.empty((C_, N), np.float32)
            want_ys = int(c["var"] == "ys")
            if want_ys:
                ysa, ysb = np.empty((C_, N), np.float32), np.empty((C_, N), np.float32)
            _lib.check(lib.sbv2_debug_repeat_conv1d_clx(0, _f(d["xa"]), _f(d["xb"]), _f(d["w"]), _f(d["b"]), _f(d["res"]), C_, C_, k, N, c["dil"], SLOPE, d["beta"],
                                                        want_ys, reps, nb, flip_at, flip_word, _f(ya), _f(yb), _f(ysa), _f(ysb), P64(mm), P64(fb)))
            return ya, yb, ysa, ysb, mm, fb, prof
        T = lambda a: None if a is None else np.ascontiguousarray(a.T)
        xa, xb, prev = T(d["xa"]), T(d["xb"]), T(d["prev"])
        ya, yb = np.empty((N, C_), np.float32), np.empty((N, C_), np.float32)
        m = None if d["mask"] is None else d["mask"].ctypes.data
        if c["fam"] == "resbranch_clx":
            dl = np.asarray(c["dil"], np.int64)
            _lib.check(lib.sbv2_debug_repeat_resbranch(0, _f(xa), _f(xb), _f(d["w"]), _f(d["b"]), C_, N, k, P64(dl), m, 4, d["beta"], _f(prev), reps, nb, flip_at,
                                                       flip_word, _f(ya), _f(yb), P64(mm), P64(fb)))
        else:
            w, b = d["w"], d["b"]
            _lib.check(lib.sbv2_debug_repeat_respair(0, _f(xa), _f(xb), _f(w[0]), _f(w[1]), _f(b[0]), _f(b[1]), C_, N, k, c["dil"], m, 4, d["beta"], _f(prev),
                                                     c["variant"], reps, nb, flip_at, flip_word, _f(ya), _f(yb), P64(mm), P64(fb)))
    return ya.T, yb.T, None, None, mm, fb, prof


def _where(c, word):
    n = c["N"] * c["C"]
    return f"(row {word // c['C']}, channel {word % c['C']})" if word < n else f"(parts planes, word {word - n})"


def _check_profile(c, prof, reps):
    want = {c["bucket"]: reps}
    if c["regime"] == "b":
        want["gemm_bfs<f16x3>"] = reps // 2
    assert prof.launches == want, f"{_id(c)}: the profile saw {prof.launches}, expected {want}"


@gpu
@pytest.mark.parametrize("c", CASES, ids=_id)
def test_repeated_launches_give_the_same_bits(c, device):
    d = make_data(c)
    ya, yb, ysa, ysb, mm, fb, prof = launch(c, d)
    _check_profile(c, prof, REPS)
    shape = f"{c['fam']} C{c['C']} k{c['k']} dil{c['dil']} {c['var']} N{c['N']} grid{c['grid']} regime ({c['regime']})"
    bad = np.flatnonzero(mm != 0)
    assert bad.size == 0, f"{shape}: " + "; ".join(f"repetition {i}: {mm[i]} words differ, the first at {_where(c, int(fb[i]))}" for i in bad[:8])
    assert np.all(fb == -1)
    print(f"[{shape}] {REPS} repetitions, {prof.launches}, 0 mismatches")
    # the first results against float64
    N, worst, worst8 = c["N"], 0.0, 0.0
    wins = [(0, N)] if c["regime"] == "b" else windows(c, d["rng"])
    for name, x, y, ys in (("a", d["xa"], ya, ysa), ("b", d["xb"], yb, ysb)):
        assert np.isfinite(y).all(), f"{shape} input {name}: a row was not written, or a NaN came out"
        if d.get("mask") is not None:
            assert not np.any(y[:, d["keep"] == 0]), f"{shape} input {name}: a masked column is not exactly zero"
        for (s, e), (ref, tol, tol8) in zip(wins, on_windows(lambda lo, hi: tolerance(c, d, x, lo, hi), N, wins, reach(c))):
            keep = d["keep"][s:e] > 0 if "keep" in d else np.ones(e - s, bool)
            err = np.abs(y[:, s:e] - ref)[:, keep]
            worst, worst8 = max(worst, float((err / tol[:, keep]).max())), max(worst8, float((err / tol8[:, keep]).max()))
        if ys is not None:
            lr = lrelu(y)
            assert np.all(np.abs(ys.astype(np.float64) - lr) <= _split_bound(lr, 2)), f"{shape} input {name}: the parts are not the split of lrelu(result)"
    _report(shape + " first-order", worst, 1.0)
    _report(shape + " 8-sigma", worst8, 1.0)
    assert worst <= 1.0 and worst8 <= 1.0, (worst, worst8)


FLIP_AT = 37


@gpu
@pytest.mark.parametrize("fam", ["respair_x16", "respair_clx", "resbranch_clx", "conv_clx"])
def test_a_flipped_bit_is_counted(fam, device):
    """the screen's self-check: one bit of one word of repetition 37 flipped before its comparison = exactly one differing word, there, and nowhere else"""
    c = next(c for c in CASES if c["fam"] == fam and c["regime"] == "b" and c["var"] in (FULL, "ys"))
    d = make_data(c)
    n = c["N"] * c["C"]
    word = n + 12345 if fam == "conv_clx" else (c["N"] // 2) * c["C"] + 5     # conv_clx: a word of the parts planes, behind the f32 plane
    *_, mm, fb, prof = launch(c, d, flip_at=FLIP_AT, flip_word=word)
    _check_profile(c, prof, REPS)
    want = np.zeros(REPS, np.int64)
    want[FLIP_AT] = 1
    np.testing.assert_array_equal(mm, want)
    assert fb[FLIP_AT] == word and np.all(np.delete(fb, FLIP_AT) == -1), fb


# ---- the phased upsamplers and gemm_bfs -----------------------------------------------------------------------------------------------------------------------

def up_data(c, seed=None):
    rng = np.random.default_rng(zlib.crc32(_id(c).encode()) if seed is None else seed)
    cin, cout, k, s, N = c["cin"], c["C"], c["k"], c["s"], c["N"]
    d = dict(rng=rng, xa=rng.standard_normal((cin, N), np.float32), xb=rng.standard_normal((cin, N), np.float32),
             w=(rng.standard_normal((cin, cout, k)) / np.sqrt(cin * k / s)).astype(np.float32), b=rng.standard_normal(cout).astype(np.float32))
    d["mask"] = (rng.random(_cdiv(N, 4)) > 0.15).astype(np.uint8) if c["var"] == "mask4" else None
    d["keep"] = np.repeat(d["mask"], 4)[:N].astype(np.float32) if d["mask"] is not None else np.ones(N, np.float32)
    d["xa"] *= d["keep"][None, :]
    d["xb"] *= d["keep"][None, :]
    # the same weights stored tap-major for the reference: O.conv_transpose1d multiplies w[:, :, j].T, which then has a unit stride (BLAS instead of
    # numpy's strided fallback loop, 20x slower at 256 x 128 x 16)
    d["wr"] = np.ascontiguousarray(d["w"].transpose(2, 1, 0)).transpose(2, 1, 0)
    return d


def up_ref(c, d, x, lo, hi, dt, wrong=None):
    """keep (ConvTranspose1d(lrelu(x), stride s, padding (k - s) / 2)) on input positions [lo, hi) -> output columns [lo s, hi s)"""
    k, s = c["k"], c["s"]
    a = x[:, lo:hi].astype(dt)
    if wrong != "no-lrelu":
        a = lrelu(a)
    y = O.conv_transpose1d(a, d["wr"].astype(dt), d["b"].astype(dt), s, (k - s) // 2)
    if wrong == "phase-shift":      # phase 1 reads its taps one input position late
        late = np.concatenate([np.zeros_like(a[:, :1]), a[:, :-1]], axis=1)
        y[:, 1::s] = O.conv_transpose1d(late, d["wr"].astype(dt), d["b"].astype(dt), s, (k - s) // 2)[:, 1::s]
    return y * np.repeat(d["keep"][lo:hi], s).astype(dt)[None, :]


def up_tolerance(c, d, x, lo, hi):
    ref = up_ref(c, d, x, lo, hi, np.float64)
    S = O.conv_transpose1d(np.abs(lrelu(x[:, lo:hi].astype(np.float64))), np.abs(d["wr"].astype(np.float64)), np.zeros(c["C"]), c["s"], (c["k"] - c["s"]) // 2)
    return ref, C_BF16X3 * S + 4.0 * np.abs(up_ref(c, d, x, lo, hi, np.float32).astype(np.float64) - ref) + 1e-37


def test_grid_sizes_of_the_upsamplers_and_gemm_bfs():
    for c in UP_CASES:
        assert c["N"] % 256 and c["N"] >= 256
        if c["regime"] == "a":
            whole = c["N"] // 256
            assert whole % 8 == 0 and whole * c["gy"] >= NCU * c["res"] > (whole - 8) * c["gy"] and c["grid"] >= NCU * c["res"], _id(c)
        else:
            assert 48 <= c["work"] <= 80 and c["grid"] == max(c["work"], 8 * c["gy"]), _id(c)
    for c in BFS_CASES:
        assert G.bfs_kernel(4, c["M"], c["N"], c["K"], 1) == c["inst"], _id(c)
        assert c["N"] % c["nto"] and c["N"] % 4 == 0
    a, b, ka, kb = BFS_CASES
    assert a["grid"] == _up(_cdiv(a["M"], 64) * _cdiv(a["N"], 128), 8) >= NCU * a["res"] > _cdiv(a["M"], 64) * (a["N"] // 128 - 1)
    # the batch instantiation's smallest grid: one row tile, and one 128-column block fewer is no longer `big`
    assert b["grid"] == _cdiv(b["N"], 128) == 128 and G.bfs_kernel(4, b["M"], b["N"] - 128, b["K"], 1) != b["inst"]
    # the K split's largest grid: tiles x 8 K groups = one workgroup per CU; twice the row tiles would halve the split
    assert ka["grid"] == _cdiv(ka["M"], 64) * _cdiv(ka["N"], 64) * 8 == NCU and 48 <= kb["grid"] == _cdiv(kb["M"], 64) * _cdiv(kb["N"], 64) * 8 <= 80
    src = open(os.path.join(CSRC, "gemm_bfs.hip")).read()
    assert "while (ks < 8 && tiles * (ks * 2) <= ncu" in src and "hipLaunchKernelGGL(kern, dim3(round_up(kp.total, 8))" in src
    assert "launch_bfs_cfg<2, 1, 2, 2, 2, 1, 4, true>(kp, stream);" in src and "launch_bfs_cfg<2, 1, 1, 2, 2, 1, 8, true, true>(kp, stream, ks);" in src


@pytest.mark.parametrize("name", ["up2", "up4"])
def test_wrong_upsampler_references_exceed_the_tolerance(name):
    """one phase's taps shifted by one input position, or lrelu missing on the operand"""
    c = dict(next(c for c in UP_CASES if c["fam"] == "conv_clx_" + name and c["var"] == "mask4"), N=301)
    d = up_data(c, seed=7)
    ref, tol = up_tolerance(c, d, d["xa"], 0, c["N"])
    keep = np.repeat(d["keep"], c["s"]) > 0
    for wrong in ("phase-shift", "no-lrelu"):
        assert (np.abs(up_ref(c, d, d["xa"], 0, c["N"], np.float64, wrong) - ref)[:, keep] / tol[:, keep]).max() > 1.0, (name, wrong)


def _no_mismatch(shape, mm, fb, where):
    bad = np.flatnonzero(mm != 0)
    assert bad.size == 0, f"{shape}: " + "; ".join(f"repetition {i}: {mm[i]} words differ, the first at {where(int(fb[i]))}" for i in bad[:8])
    assert np.all(fb == -1)


def up_launch(c, d, reps=REPS, flip_at=-1, flip_word=0):
    cout, N, s = c["C"], c["N"], c["s"]
    mm, fb = np.full(reps, -7, np.int64), np.full(reps, -7, np.int64)
    want_ys = int(c["var"] == "ys")
    ya, yb = np.empty((cout, N * s), np.float32), np.empty((cout, N * s), np.float32)
    ysa, ysb = (np.empty_like(ya), np.empty_like(ya)) if want_ys else (None, None)
    m = None if d["mask"] is None else d["mask"].ctypes.data
    with _Prof() as prof:
        _lib.check(_lib.lib().sbv2_debug_repeat_conv_transpose1d_clx(0, _f(d["xa"]), _f(d["xb"]), _f(d["w"]), _f(d["b"]), c["cin"], cout, c["k"], N, s, SLOPE, m, 4,
                                                                     want_ys, reps, int(c["regime"] == "b"), flip_at, flip_word, _f(ya), _f(yb), _f(ysa), _f(ysb),
                                                                     mm.ctypes.data_as(i64p), fb.ctypes.data_as(i64p)))
    return ya, yb, ysa, ysb, mm, fb, prof


@gpu
@pytest.mark.parametrize("c", UP_CASES, ids=_id)
def test_repeated_upsampler_launches_give_the_same_bits(c, device):
    d = up_data(c)
    ya, yb, ysa, ysb, mm, fb, prof = up_launch(c, d)
    _check_profile(c, prof, REPS)
    N, s, cout = c["N"], c["s"], c["C"]
    shape = f"{c['fam']} {c['cin']}->{cout} k{c['k']} stride{s} {c['var']} N{N} grid{c['grid']} regime ({c['regime']})"
    _no_mismatch(shape, mm, fb, lambda wd: f"(row {wd // cout}, channel {wd % cout})" if wd < N * s * cout else f"(parts planes, word {wd - N * s * cout})")
    print(f"[{shape}] {REPS} repetitions, {prof.launches}, 0 mismatches")
    wins, worst = [(0, N)] if c["regime"] == "b" else windows(c, d["rng"]), 0.0
    for name, x, y, ys in (("a", d["xa"], ya, ysa), ("b", d["xb"], yb, ysb)):
        assert np.isfinite(y).all(), f"{shape} input {name}: a row was not written, or a NaN came out"
        assert not np.any(y[:, np.repeat(d["keep"], s) == 0]), f"{shape} input {name}: a masked column is not exactly zero"
        for (s0, e0), (ref, tol) in zip(wins, on_windows(lambda lo, hi: up_tolerance(c, d, x, lo, hi), N, wins, c["k"] // s + 1, s)):
            keep = np.repeat(d["keep"][s0:e0], s) > 0
            worst = max(worst, float((np.abs(y[:, s0 * s:e0 * s] - ref)[:, keep] / tol[:, keep]).max()))
        if ys is not None:
            lr = lrelu(y)
            assert np.all(np.abs(ys.astype(np.float64) - lr) <= _split_bound(lr, 2)), f"{shape} input {name}: the parts are not the split of lrelu(result)"
    _report(shape, worst, 1.0)
    assert worst <= 1.0, worst


def bfs_launch(c, d, reps=REPS, flip_at=-1, flip_word=0):
    M, N, K = c["M"], c["N"], c["K"]
    mm, fb = np.full(reps, -7, np.int64), np.full(reps, -7, np.int64)
    ya, yb, ysa, ysb = (np.empty((M, N), np.float32) for _ in range(4))
    with G._Ksplit(1), _Prof() as prof:
        _lib.check(_lib.lib().sbv2_debug_repeat_gemm_bfs(0, _f(d["xa"]), _f(d["xb"]), _f(d["w"]), _f(d["b"]), _f(d["res"]), M, N, K, 4, 4, reps,
                                                         int(c["regime"] == "b"), flip_at, flip_word, _f(ya), _f(yb), _f(ysa), _f(ysb), mm.ctypes.data_as(i64p),
                                                         fb.ctypes.data_as(i64p)))
    return ya, yb, ysa, ysb, mm, fb, prof


def bfs_data(c):
    rng = np.random.default_rng(zlib.crc32(_id(c).encode()))
    M, N, K = c["M"], c["N"], c["K"]
    return dict(xa=rng.standard_normal((K, N), np.float32), xb=rng.standard_normal((K, N), np.float32), w=(rng.standard_normal((M, K)) / np.sqrt(K)).astype(np.float32),
                b=rng.standard_normal(M).astype(np.float32), res=rng.standard_normal((M, N), np.float32))


def _bfs_profile(c, prof, reps):
    want = {"gemm_bfs<f16x3>": reps + (reps // 2 if c["regime"] == "b" else 0)}
    assert prof.launches == want, f"{_id(c)}: the profile saw {prof.launches}, expected {want}"


@gpu
@pytest.mark.parametrize("c", BFS_CASES, ids=_id)
def test_repeated_gemm_bfs_launches_give_the_same_bits(c, device):
    """y = w x + bias + res with the parts copy, f16x3; reference and tolerance of tests/test_gemm_conv_kernels.py (the whole plane in both regimes: a 1x1 product)"""
    d = bfs_data(c)
    ya, yb, ysa, ysb, mm, fb, prof = bfs_launch(c, d)
    _bfs_profile(c, prof, REPS)
    M, N, ld = c["M"], c["N"], _up(c["N"], 64)
    shape = f"gemm_bfs<{c['inst']}> M{M} N{N} K{c['K']} grid{c['grid']} regime ({c['regime']})"
    _no_mismatch(shape, mm, fb, lambda wd: f"(row {wd // ld}, column {wd % ld})" if wd < M * ld else f"(parts planes, word {wd - M * ld})")
    print(f"[{shape}] {REPS} repetitions, {prof.launches}, 0 mismatches")
    w3, epi, worst = d["w"][:, :, None], dict(bias=d["b"], res=d["res"]), 0.0
    for name, x, y, ys in (("a", d["xa"], ya, ysa), ("b", d["xb"], yb, ysb)):
        assert np.isfinite(y).all() and np.isfinite(ys).all(), f"{shape} input {name}: an element was not written, or a NaN came out"
        ref, ref32 = G.conv_ref(x, w3, 1, 0, np.float64, **epi), G.conv_ref(x, w3, 1, 0, np.float32, **epi)
        tol = G.tol_split(G.C_F16X3, G.abs_sum(x, w3, 1, 0), ref, ref32, epi)
        worst = max(worst, float((np.abs(y - ref) / tol).max()), float((np.abs(ys - y.astype(np.float64)) / G.parts_bound(y, 4)).max()))
    _report(shape, worst, 1.0)
    assert worst <= 1.0, worst


@gpu
@pytest.mark.parametrize("fam", ["conv_clx_up2", "conv_clx_up4", "gemm_bfs"])
def test_a_flipped_bit_is_counted_upsampler_and_gemm_bfs(fam, device):
    want = np.zeros(REPS, np.int64)
    want[FLIP_AT] = 1
    if fam == "gemm_bfs":
        c = BFS_CASES[3]
        word = 17 * _up(c["N"], 64) + 5
        *_, mm, fb, prof = bfs_launch(c, bfs_data(c), flip_at=FLIP_AT, flip_word=word)
        _bfs_profile(c, prof, REPS)
    else:
        c = next(c for c in UP_CASES if c["fam"] == fam and c["regime"] == "b" and c["var"] == "mask4")
        word = (c["N"] * c["s"] // 2) * c["C"] + 5
        *_, mm, fb, prof = up_launch(c, up_data(c), flip_at=FLIP_AT, flip_word=word)
        _check_profile(c, prof, REPS)
    np.testing.assert_array_equal(mm, want)
    assert fb[FLIP_AT] == word and np.all(np.delete(fb, FLIP_AT) == -1), fb


# ---- k_vits_flash_x3q -----------------------------------------------------------------------------------------------------------------------------------------
# The flow's full shape: 2 heads of 96, window 4.  vits_flash_attention_parts starts ceil(T / (32 NW)) x (utterances x heads) workgroups, NW = 4 waves (128
# queries) while that leaves at most one workgroup per CU, else 8 waves (256 queries); either shape holds 4 x 2 x 96 x 128 bytes of K / V tiles plus band state
# in LDS (> 80 KB): one workgroup per CU.  (a): 32 utterances of 897 frames = 4 x 64 = 256 workgroups of 8 waves, the last query tile partial; (b): 8
# utterances of 449 frames = 4 x 16 = 64 workgroups of 4 waves.  The launch profile does not record attention launches: the hook takes only head dimensions
# k_vits_flash_x3q takes and forces that kernel.
ATTN = dict(heads=2, dk=96, w=4)
ATTN_CASES = [dict(fam="vits_flash_x3q", regime="a", nutt=32, T=897, check=(0, 1, 15, 31)), dict(fam="vits_flash_x3q", regime="b", nutt=8, T=449, check=tuple(range(8)))]


def attn_grid(T, nutt, heads=ATTN["heads"], ncu=NCU):
    ng = nutt * heads
    nw = 8 if _cdiv(T, 128) * ng > ncu else 4
    return nw, _cdiv(T, 32 * nw) * ng


def test_grid_sizes_of_the_attention_cases():
    src = open(os.path.join(CSRC, "attn_flash.hip")).read()
    assert "const dim3 grid((maxT + 32 * NW - 1) / (32 * NW), ngroups);" in src and "(int64_t)((maxT + 127) / 128) * ngroups > device_cu_count()" in src
    assert "constexpr int kFaMaxWin = 4;" in src and "constexpr int kFaBand = 2 * kFaMaxWin + 1;" in src
    lds = lambda nw: 4 * 2 * 96 * 128 + 4 * (2 * 9 * 96 + 2 * nw * 9 * 32) + nw * 64 * 4 + (nw * 6 * 1024 if nw == 4 else 0)     # launch_flash_x3q, DT = 3
    assert LDS_CU // lds(4) == 1 and LDS_CU // lds(8) == 1
    a, b = ATTN_CASES
    assert attn_grid(a["T"], a["nutt"]) == (8, NCU) and a["T"] % 256 and attn_grid(a["T"] - 256, a["nutt"])[1] < NCU
    assert attn_grid(b["T"], b["nutt"]) == (4, 64) and b["T"] % 128


def attn_data(c):
    rng = np.random.default_rng(zlib.crc32(f"attn-{c['regime']}".encode()))
    H, N = ATTN["heads"] * ATTN["dk"], c["nutt"] * c["T"]
    a, b = A._vits_inputs(rng, H, N, ATTN["dk"], ATTN["w"]), A._vits_inputs(rng, H, N, ATTN["dk"], ATTN["w"])
    return a[:3], b[:3], a[3], a[4]


def attn_launch(c, d, reps=REPS, flip_at=-1, flip_word=0):
    (qa, ka, va), (qb, kb, vb), erk, erv = d
    mm, fb = np.full(reps, -7, np.int64), np.full(reps, -7, np.int64)
    ca, cb = np.empty_like(qa), np.empty_like(qa)
    lens, ld = np.full(c["nutt"], c["T"], np.int64), C.c_int64(0)
    _lib.check(_lib.lib().sbv2_debug_repeat_vits_attention(0, _f(qa), _f(ka), _f(va), _f(qb), _f(kb), _f(vb), _f(erk), _f(erv), lens.ctypes.data_as(i64p), c["nutt"],
                                                           ATTN["heads"], ATTN["dk"], ATTN["w"], reps, int(c["regime"] == "b"), flip_at, flip_word, _f(ca), _f(cb),
                                                           C.byref(ld), mm.ctypes.data_as(i64p), fb.ctypes.data_as(i64p)))
    return ca, cb, ld.value, mm, fb


@gpu
@pytest.mark.parametrize("c", ATTN_CASES, ids=lambda c: f"vits_flash_x3q-{c['regime']}")
def test_repeated_attention_launches_give_the_same_bits(c, device):
    """reference and tolerance of tests/test_attention_kernels.py; regime (a) holds the first two, a middle and the last utterance against float64"""
    d = attn_data(c)
    ca, cb, ld, mm, fb = attn_launch(c, d)
    nw, grid = attn_grid(c["T"], c["nutt"])
    shape = f"k_vits_flash_x3q<3,{nw}> {c['nutt']} x {c['T']} frames, 2 heads of 96, grid{grid} regime ({c['regime']})"
    _no_mismatch(shape, mm, fb, lambda wd: f"(row {wd // ld}, plane column {wd % ld})")
    print(f"[{shape}] {REPS} repetitions, 0 mismatches")
    T, worst, (erk, erv) = c["T"], 0.0, d[2:]
    for name, (q, k, v), got in (("a", d[0], ca), ("b", d[1], cb)):
        assert np.isfinite(got).all(), (shape, name)
        for u in c["check"]:
            sl = slice(u * T, (u + 1) * T)
            args = (q[:, sl], k[:, sl], v[:, sl], erk, erv, [T], ATTN["heads"], ATTN["dk"], ATTN["w"])
            ref = A._vits_ref(*args, np.float64)
            err32 = float(np.abs(A._vits_ref(*args, np.float32) - ref).max())
            worst = max(worst, float((np.abs(got[:, sl] - ref) / (A._vits_bound(*args) + 4 * err32 + 1e-7)).max()))
    _report(shape, worst, 1.0)
    assert worst <= 1.0, worst


@gpu
def test_a_flipped_bit_is_counted_attention(device):
    c = ATTN_CASES[1]
    word = 100 * 4096 + 77          # row 100 of the ctx plane (its pitch is >= 8 x 449 columns)
    *_, ld, mm, fb = attn_launch(c, attn_data(c), flip_at=FLIP_AT, flip_word=word)
    want = np.zeros(REPS, np.int64)
    want[FLIP_AT] = 1
    np.testing.assert_array_equal(mm, want)
    assert fb[FLIP_AT] == word and np.all(np.delete(fb, FLIP_AT) == -1), fb


# ---- the flow FFN pair on conv_clx ------------------------------------------------------------------------------------------------------------------------------
# 192 -> 768 -> 192, k = 5: conv_1 (12 row blocks of 64) then conv_2 (3 row blocks), both on 288-row windows = three workgroups per CU; one repetition = both
# launches.  (a): conv_2, the smaller grid, reaches 256 x 3 workgroups (conv_1 then starts four times as many); (b): launch_clx_e rounds the position tiles
# up to 8, so conv_1 cannot start fewer than 96 workgroups: 8 tiles, the last partial = 96 (conv_1) and 24 (conv_2) workgroups.
FFN = dict(H=192, F=768, k=5)
FFN_CASES = [dict(fam="conv_clx_ffn", regime="a", N=_up(_cdiv(NCU * 3, 3), 8) * 256 + 129, nto=256), dict(fam="conv_clx_ffn", regime="b", N=7 * 256 + 129, nto=256)]


def ffn_data(c, seed=None):
    rng = np.random.default_rng(zlib.crc32(f"ffn-{c['regime']}".encode()) if seed is None else seed)
    H, F, k, N = FFN["H"], FFN["F"], FFN["k"], c["N"]
    d = dict(rng=rng, xa=rng.standard_normal((H, N), np.float32), xb=rng.standard_normal((H, N), np.float32),
             w1=(rng.standard_normal((F, H, k)) / np.sqrt(H * k)).astype(np.float32), b1=rng.standard_normal(F).astype(np.float32),
             w2=(rng.standard_normal((H, F, k)) / np.sqrt(F * k)).astype(np.float32), b2=rng.standard_normal(H).astype(np.float32))
    d["mask"] = (rng.random(N) > 0.15).astype(np.uint8)
    d["keep"] = d["mask"].astype(np.float32)
    d["xa"] *= d["keep"][None, :]
    d["xb"] *= d["keep"][None, :]
    return d


def ffn_ref(d, x, lo, hi, dt, wrong=None, bound=False):
    """y = keep (conv_2(relu(keep (conv_1(x) + b1))) + b2 + x) on columns [lo, hi); bound: also the first-order and the 8-sigma bound (module docstring)"""
    cast = lambda a: np.asarray(a, dt)
    x, kp, cs = cast(x[:, lo:hi]), cast(d["keep"][lo:hi])[None, :], O.conv1d_same
    w1, b1, w2, b2 = cast(d["w1"]), cast(d["b1"]), cast(d["w2"]), cast(d["b2"])
    t = conv(x, w1, b1, 1, wrong)
    if wrong != "mask-end":
        t = kp * t
    u = t if wrong == "no-relu" else np.maximum(t, dt(0))
    y = kp * (cs(u, w2, b2, 1) + x)
    if not bound:
        return y
    A, S = np.abs, np.square
    E = kp * (C_BF16X3 * cs(A(u), A(w2), None, 1) + cs(kp * C_BF16X3 * cs(A(x), A(w1), None, 1), A(w2), None, 1))
    V = kp * (C_BF16X3 ** 2 * cs(S(u), S(w2), None, 1) + cs(kp * C_BF16X3 ** 2 * cs(S(x), S(w1), None, 1), S(w2), None, 1))
    return y, E, 8.0 * np.sqrt(V)


def ffn_tolerance(d, x, lo, hi):
    ref, E, S8 = ffn_ref(d, x, lo, hi, np.float64, bound=True)
    e32 = 4.0 * np.abs(ffn_ref(d, x, lo, hi, np.float32).astype(np.float64) - ref)
    return ref, E + e32, S8 + e32


def test_ffn_grids_and_wrong_references():
    a, b = FFN_CASES
    g = lambda N, M: clx_grid(N, M)
    assert residency(*clx_cfg(5, 1)[1:]) == 3 and g(a["N"], 192) >= (a["N"] // 256) * 3 >= NCU * 3 > (a["N"] // 256 - 8) * 3 and a["N"] % 256
    assert (g(b["N"], 768), g(b["N"], 192)) == (96, 24) and b["N"] % 256 and g(300, 768) == 96          # (8 position tiles are the launcher's minimum)
    src = open(os.path.join(CSRC, "vits.cpp")).read()
    assert "p1.ys_slope = 0.0f;     // ReLU" in src and "p2.Rkm = x.p;" in src and "p1.mask_shift = 0;" in src
    c = dict(N=601)
    d = ffn_data(c, seed=11)
    ref, tol, tol8 = ffn_tolerance(d, d["xa"], 0, 601)
    keep = d["keep"] > 0
    for wrong in ("tap-dilation", "no-relu", "mask-end"):
        err = np.abs(ffn_ref(d, d["xa"], 0, 601, np.float64, wrong) - ref)[:, keep]
        assert (err / tol[:, keep]).max() > 1.0 and (err / tol8[:, keep]).max() > 1.0, wrong


def ffn_launch(c, d, reps=REPS, flip_at=-1, flip_word=0):
    H, F, k, N = FFN["H"], FFN["F"], FFN["k"], c["N"]
    mm, fb = np.full(reps, -7, np.int64), np.full(reps, -7, np.int64)
    ya, yb = np.empty((H, N), np.float32), np.empty((H, N), np.float32)
    with _Prof() as prof:
        _lib.check(_lib.lib().sbv2_debug_repeat_conv_ffn_clx(0, _f(d["xa"]), _f(d["xb"]), _f(d["w1"]), _f(d["b1"]), _f(d["w2"]), _f(d["b2"]), H, F, k, N,
                                                             d["mask"].ctypes.data, reps, int(c["regime"] == "b"), flip_at, flip_word, _f(ya), _f(yb),
                                                             mm.ctypes.data_as(i64p), fb.ctypes.data_as(i64p)))
    want = {"conv_clx_ffn<split-bf16>": 2 * reps}
    if c["regime"] == "b":
        want["gemm_bfs<f16x3>"] = reps // 2
    assert prof.launches == want, f"the profile saw {prof.launches}, expected {want}"
    return ya, yb, mm, fb


@gpu
@pytest.mark.parametrize("c", FFN_CASES, ids=lambda c: f"conv_clx_ffn-{c['regime']}")
def test_repeated_ffn_pair_launches_give_the_same_bits(c, device):
    d = ffn_data(c)
    ya, yb, mm, fb = ffn_launch(c, d)
    N = c["N"]
    shape = f"conv_clx_ffn 192->768->192 k5 N{N} grids {clx_grid(N, 768)} + {clx_grid(N, 192)} regime ({c['regime']})"
    _no_mismatch(shape, mm, fb, lambda wd: f"(word {wd} of the intermediate's parts planes, then y [192][{_up(N, 64)}])")
    print(f"[{shape}] {REPS} repetitions of both launches, 0 mismatches")
    wins, worst, worst8 = [(0, N)] if c["regime"] == "b" else windows(c, d["rng"]), 0.0, 0.0
    for name, x, y in (("a", d["xa"], ya), ("b", d["xb"], yb)):
        assert np.isfinite(y).all(), f"{shape} input {name}: an element was not written, or a NaN came out"
        assert not np.any(y[:, d["keep"] == 0]), f"{shape} input {name}: a masked column is not exactly zero"
        for (s0, e0), (ref, tol, tol8) in zip(wins, on_windows(lambda lo, hi: ffn_tolerance(d, x, lo, hi), N, wins, 4)):
            keep = d["keep"][s0:e0] > 0
            err = np.abs(y[:, s0:e0] - ref)[:, keep]
            worst, worst8 = max(worst, float((err / tol[:, keep]).max())), max(worst8, float((err / tol8[:, keep]).max()))
    _report(shape + " first-order", worst, 1.0)
    _report(shape + " 8-sigma", worst8, 1.0)
    assert worst <= 1.0 and worst8 <= 1.0, (worst, worst8)


@gpu
def test_a_flipped_bit_is_counted_ffn_pair(device):
    c = FFN_CASES[1]
    word = 4321                     # a word of the intermediate's parts planes
    *_, mm, fb = ffn_launch(c, ffn_data(c), flip_at=FLIP_AT, flip_word=word)
    want = np.zeros(REPS, np.int64)
    want[FLIP_AT] = 1
    np.testing.assert_array_equal(mm, want)
    assert fb[FLIP_AT] == word and np.all(np.delete(fb, FLIP_AT) == -1), fb
