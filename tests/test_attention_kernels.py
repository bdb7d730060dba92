"""The attention kernels launch by launch (sbv2_debug_vits_attention / sbv2_debug_deberta_attention: the models' own layouts and plan builders) against
float64 references of the same operation (sbv2_oracle.rel_attention_core / disentangled_attention), at the lengths, head dimensions and masks where a
tiled online softmax goes wrong: 32-key steps, 64-key tiles, 128 / 256-query workgroups, forced rescales of the running maximum, masked key tiles.

Tolerances (derived per test; the worst error / tolerance ratio of each case is printed):
- exact-f32 paths (VITS unfused and k_vits_flash, every DeBERTa path): max(4 err32, floor), err32 = the same reference evaluated in float32.
- split-bf16 paths (k_vits_flash_x3 / x3p / x3q): x = hi + lo with |x - hi - lo| <= 2^-16 |x| and the lo * lo product dropped.  Per element the logit
  s_ij is allowed e_ij = 2 2^-16 qscale sum_d |q_di k_dj| (the error terms have random signs: their sum stays well below this), which moves an output by
  at most sum_j p_ij (e_ij + sum_k p_ik e_ik) (|v_dj| or |emb_rel_v| in the band), plus 2 2^-16 sum_j p_ij |v_dj| from P V's own split, plus 4 err32 for
  the f32 parts.  A reference that drops one hi * lo cross term instead (~2^-9 relative) must exceed this bound: checked in numpy on the same data.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import sbv2_oracle as O
from sbv2_api_amd import _lib

pytestmark = pytest.mark.gpu
f32p, i64p = _lib.f32p, _lib.i64p
TEXT, FRAMES = 0, 1
U = 2.0 ** -16
PACKED = [1, 2, 5, 9, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 897]


def _p(a):
    return a.ctypes.data_as(f32p)


def _vits(q, k, v, erk, erv, lens, heads, dk, w, layout, variant, poison=0):
    q, k, v, erk, erv = (np.ascontiguousarray(a, np.float32) for a in (q, k, v, erk, erv))
    ln = np.asarray(lens, np.int64)
    ctx = np.empty_like(q)
    stray = C.c_int64(-1)
    _lib.check(_lib.lib().sbv2_debug_vits_attention(0, _p(q), _p(k), _p(v), _p(erk), _p(erv), ln.ctypes.data_as(i64p), len(lens), heads, dk, w, layout,
                                                    variant, poison, _p(ctx), C.byref(stray)))
    return ctx, stray.value


def _deberta(q, k, v, pk, pq, lens, heads, d, buckets, max_rel, mask, gap, variant, poison=0):
    q, k, v, pk, pq = (np.ascontiguousarray(a, np.float32) for a in (q, k, v, pk, pq))
    ln = np.asarray(lens, np.int64)
    m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
    ctx = np.empty_like(q)
    stray = C.c_int64(-1)
    _lib.check(_lib.lib().sbv2_debug_deberta_attention(0, _p(q), _p(k), _p(v), _p(pk), _p(pq), ln.ctypes.data_as(i64p), len(lens), heads, d, buckets,
                                                       max_rel, None if m is None else m.ctypes.data, gap, variant, poison, _p(ctx), C.byref(stray)))
    return ctx, stray.value


def _segs(lens):
    o = np.concatenate([[0], np.cumsum(lens)])
    return [slice(int(o[i]), int(o[i + 1])) for i in range(len(lens))]


def _bf16_split(x):
    t = torch.from_numpy(np.ascontiguousarray(x, np.float32))
    hi = t.to(torch.bfloat16).to(torch.float32)
    lo = (t - hi).to(torch.bfloat16).to(torch.float32)
    return hi.numpy().astype(np.float64), lo.numpy().astype(np.float64)


# ---- VITS ---------------------------------------------------------------------------------------------------------------------------------------------

def _vits_ref(q, k, v, erk, erv, lens, heads, dk, w, dtype):
    out = np.empty(q.shape, np.float64)
    for s in _segs(lens):
        T = s.stop - s.start
        r = O.rel_attention_core(*(a[:, s].astype(dtype).reshape(heads, dk, T) for a in (q, k, v)), erk.astype(dtype), erv.astype(dtype), w)
        out[:, s] = r.reshape(heads * dk, T)
    return out


def _vits_bound(q, k, v, erk, erv, lens, heads, dk, w, block=512):
    """Per-element bound of the split-bf16 error (module docstring), f64, blocked over queries."""
    tol = np.empty(q.shape, np.float64)
    qs = 1.0 / np.sqrt(dk)
    for s in _segs(lens):
        T = s.stop - s.start
        for h in range(heads):
            rows = slice(h * dk, (h + 1) * dk)
            qh, kh, vh = (a[rows, s].astype(np.float64) for a in (q, k, v))
            for i0 in range(0, T, block):
                i1 = min(T, i0 + block)
                sc = qs * (qh[:, i0:i1].T @ kh)
                rl = qs * (qh[:, i0:i1].T @ erk.T.astype(np.float64))
                idx = np.arange(i1 - i0)
                for r in range(-w, w + 1):
                    i = idx[(i0 + idx + r >= 0) & (i0 + idx + r < T)]
                    sc[i, i0 + i + r] += rl[i, r + w]
                p = np.exp(sc - sc.max(axis=1, keepdims=True))
                p /= p.sum(axis=1, keepdims=True)
                e = 2 * U * qs * (np.abs(qh[:, i0:i1]).T @ np.abs(kh))              # logit error bound e_ij
                pe = p * (e + (p * e).sum(axis=1, keepdims=True))                    # |dp_ij| <= p_ij (e_ij + sum_k p_ik e_ik)
                B = pe @ np.abs(vh).T + 2 * U * (p @ np.abs(vh).T)                   # [B, dk]: softmax sensitivity + P V's own split
                for r in range(-w, w + 1):
                    i = idx[(i0 + idx + r >= 0) & (i0 + idx + r < T)]
                    B[i] += pe[i, i0 + i + r][:, None] * np.abs(erv[r + w]).astype(np.float64)[None, :]
                tol[rows, s.start + i0:s.start + i1] = B.T
    return tol


def _vits_dropped_cross_term(q, k, v, erk, erv, T, dk, w):
    """One head of one utterance (columns 0 .. T) with the logits' lo(q) * hi(k) term dropped: q . k -> hi(q) . (hi(k) + lo(k))."""
    qh, _ = _bf16_split(q[:dk, :T])
    kh, kl = _bf16_split(k[:dk, :T])
    q64, v64 = q[:dk, :T].astype(np.float64), v[:dk, :T].astype(np.float64)
    qs = 1.0 / np.sqrt(dk)
    sc = qs * (qh.T @ (kh + kl))
    rl = qs * (q64.T @ erk.T.astype(np.float64))
    idx = np.arange(T)
    for r in range(-w, w + 1):
        i = idx[(idx + r >= 0) & (idx + r < T)]
        sc[i, i + r] += rl[i, r + w]
    p = O.softmax(sc, axis=-1)
    o = p @ v64.T
    for r in range(-w, w + 1):
        i = idx[(idx + r >= 0) & (idx + r < T)]
        o[i] += p[i, i + r][:, None] * erv[r + w].astype(np.float64)[None, :]
    return o.T


def _vits_inputs(rng, H, N, dk, w, scale=1.0):
    q = (rng.standard_normal((H, N)) * scale).astype(np.float32)
    k = (rng.standard_normal((H, N)) * scale).astype(np.float32)
    v = rng.standard_normal((H, N)).astype(np.float32)
    erk = (rng.standard_normal((2 * w + 1, dk)) * 0.5).astype(np.float32)
    erv = (rng.standard_normal((2 * w + 1, dk)) * 0.5).astype(np.float32)
    return q, k, v, erk, erv


def _check_vits(name, q, k, v, erk, erv, lens, heads, dk, w, layout, variants, check_drop=True):
    """Every variant against the f64 reference; returns the outputs by variant."""
    ref = _vits_ref(q, k, v, erk, erv, lens, heads, dk, w, np.float64)
    err32 = float(np.abs(_vits_ref(q, k, v, erk, erv, lens, heads, dk, w, np.float32) - ref).max())
    floor = 5e-6 * max(1.0, float(np.abs(ref).max()))
    tol_exact = max(4 * err32, floor)
    tol_split = None
    outs = {}
    for var in variants:
        got, _ = _vits(q, k, v, erk, erv, lens, heads, dk, w, layout, var)
        assert np.isfinite(got).all(), (name, var)
        err = np.abs(got.astype(np.float64) - ref)
        exact = var in (0, 1) or (var == -1 and dk % 16 != 0)
        if exact:
            ratio = float(err.max()) / tol_exact
        else:
            if tol_split is None:
                tol_split = _vits_bound(q, k, v, erk, erv, lens, heads, dk, w) + 4 * err32 + 1e-7
                if check_drop:   # the bound is tight enough to see one missing hi * lo term
                    T = next(n for n in sorted(lens, reverse=True) if n <= 300)
                    s = _segs(lens)[list(lens).index(T)]
                    drop = _vits_dropped_cross_term(q[:, s], k[:, s], v[:, s], erk, erv, T, dk, w)
                    dr = float((np.abs(drop - ref[:dk, s]) / tol_split[:dk, s]).max())
                    assert dr > 1.0, f"{name}: a dropped hi*lo term stays inside the split-bf16 tolerance (ratio {dr:.2f})"
            ratio = float((err / tol_split).max())
        print(f"[vits {name} variant {var}] worst error / tolerance = {ratio:.3f}")
        assert ratio <= 1.0, (name, var, ratio)
        outs[var] = got
    return outs


@pytest.mark.parametrize("w", [4, 2])
@pytest.mark.parametrize("dk", [16, 40, 48, 64, 96])
def test_vits_attention_packed_batch(dk, w):
    """Every variant (-1 .. 5) on one packed batch of lengths 1 .. 897 (every 32-key step, 64-key tile and 128 / 256-query workgroup edge; 9 = 2w + 1) in
    the flow's frame layout, head dimensions 16 (padded MFMA rows), 40 (even, not a multiple of 16: no split-bf16 flow attention, x3q still takes it), 48,
    64, 96, against float64 (tolerances: module docstring).  Then the contracts: each utterance packed = the same utterance alone, bit for bit, per variant;
    variants 2 .. 5 give the same bits; with poison on (NaN in every column outside an utterance, ctx pre-filled with a sentinel) every output is finite,
    bit-equal to the clean run, and no ctx column outside an utterance is written."""
    rng = np.random.default_rng(dk * 10 + w)
    heads = 2
    H, N = heads * dk, sum(PACKED)
    q, k, v, erk, erv = _vits_inputs(rng, H, N, dk, w)
    variants = [-1, 0, 1, 2, 3, 4, 5]
    outs = _check_vits(f"dk{dk} w{w}", q, k, v, erk, erv, PACKED, heads, dk, w, FRAMES, variants)
    for var in (3, 4, 5):
        np.testing.assert_array_equal(outs[var], outs[2], err_msg=f"variant {var} vs k_vits_flash_x3")
    for var in range(6):
        got, stray = _vits(q, k, v, erk, erv, PACKED, heads, dk, w, FRAMES, var, poison=1)
        assert stray == 0, (var, stray)
        np.testing.assert_array_equal(got, outs[var], err_msg=f"poisoned gaps change variant {var}")
    for s, T in zip(_segs(PACKED), PACKED):
        for var in range(6):
            alone, _ = _vits(q[:, s], k[:, s], v[:, s], erk, erv, [T], heads, dk, w, FRAMES, var)
            np.testing.assert_array_equal(alone, outs[var][:, s], err_msg=f"T={T} variant {var}: packed != alone")


def test_vits_attention_text_layout_exact():
    """The text encoder's layout (16-column gaps, columns rounded to 4) on the exact-f32 paths (unfused and k_vits_flash: what decides the integer
    durations), full head dimension, the packed batch plus poison; tolerance max(4 err32, floor)."""
    rng = np.random.default_rng(7)
    heads, dk, w = 2, 96, 4
    q, k, v, erk, erv = _vits_inputs(rng, heads * dk, sum(PACKED), dk, w)
    outs = _check_vits("text", q, k, v, erk, erv, PACKED, heads, dk, w, TEXT, [0, 1])
    for var in (0, 1):
        got, stray = _vits(q, k, v, erk, erv, PACKED, heads, dk, w, TEXT, var, poison=1)
        assert stray == 0
        np.testing.assert_array_equal(got, outs[var])


@pytest.mark.parametrize("T,layout,variants", [(4097, FRAMES, [-1, 0, 1, 2, 3, 4, 5]), (14001, FRAMES, [-1, 1, 2, 3, 4, 5]), (4001, TEXT, [1])])
def test_vits_attention_long_sequences(T, layout, variants):
    """Single long sequences: 4097 and 14 001 frames (the long-form flow) and 4001 text tokens (the text encoder, exact f32), one head of 96, against
    float64 computed in query blocks (no T x T f64 matrix)."""
    rng = np.random.default_rng(T)
    heads, dk, w = 1, 96, 4
    q, k, v, erk, erv = _vits_inputs(rng, heads * dk, T, dk, w)
    _check_vits(f"T{T}", q, k, v, erk, erv, [T], heads, dk, w, layout, variants, check_drop=False)


def test_vits_attention_large_batch_takes_the_8_wave_kernel():
    """32 x 897 frames x 2 heads of 96: the flow's own choice (variant -1) is k_vits_flash_x3q's 8-wave shape; the same bits as variant 5, and both
    within the split-bf16 bound of float64; the 4-wave shape forced on the same batch gives the same bits."""
    rng = np.random.default_rng(32)
    heads, dk, w = 2, 96, 4
    lens = [897] * 32
    q, k, v, erk, erv = _vits_inputs(rng, heads * dk, sum(lens), dk, w)
    outs = _check_vits("32x897", q, k, v, erk, erv, lens, heads, dk, w, FRAMES, [-1, 5], check_drop=False)
    np.testing.assert_array_equal(outs[-1], outs[5])
    four, _ = _vits(q, k, v, erk, erv, lens, heads, dk, w, FRAMES, 4)
    np.testing.assert_array_equal(four, outs[5])


def _spiked(case, dk, w, T, rng):
    """Inputs whose online softmax must rescale at a chosen late key step (scores up to ~+-60 in natural-log units)."""
    H = dk
    q, k, v, erk, erv = _vits_inputs(rng, H, T, dk, w, scale=0.3)
    u = rng.standard_normal(dk)
    u /= np.linalg.norm(u)
    big = 60.0 * np.sqrt(dk)            # q . k / sqrt(dk) = 60 for a unit-norm pair scaled by sqrt(big)
    jstar = T - 40                      # a key in a late 32-key step
    if case in ("some_lanes", "all_lanes"):
        k[:, jstar] = (np.sqrt(big) * u).astype(np.float32)
        sel = np.arange(T) if case == "all_lanes" else np.arange(0, T, 3)   # every third query: part of each wave's lanes
        q[:, sel] = (np.sqrt(big) * u[:, None] * rng.uniform(0.3, 1.0, sel.size)[None, :]).astype(np.float32)
    elif case == "decreasing":          # every query's maximum sits at key 0: no rescale after the first step
        c = np.linspace(1.0, -1.0, T)
        k[:, :] = (np.sqrt(big) * u[:, None] * c[None, :] + 0.01 * rng.standard_normal((dk, T))).astype(np.float32)
        q[:, :] = (np.sqrt(big) * u[:, None] * rng.uniform(0.5, 1.0, T)[None, :]).astype(np.float32)
    elif case == "band":                # the relative-key term dominates: every maximum lies within +-w of the diagonal
        q[:, :] = (np.sqrt(big) * u[:, None] * rng.uniform(0.3, 1.0, T)[None, :]).astype(np.float32)
        erk[:, :] = (np.sqrt(big) * u[None, :] * rng.uniform(-1.0, 1.0, 2 * w + 1)[:, None]).astype(np.float32)
    return q, k, v, erk, erv


@pytest.mark.parametrize("case", ["some_lanes", "all_lanes", "decreasing", "band"])
@pytest.mark.parametrize("dk", [16, 96])
def test_vits_attention_forced_rescale(case, dk):
    """The online softmax's rescale forced at a chosen late key step (cdna_hip_programming item 26: a rescale that is wrong whenever it runs passes on
    random data): one key spiked against every third query (k_vits_flash_x3q's ballot(alpha != 1) partly true) or against all of them, scores decreasing
    from key 0 (no rescale after step 0), and a dominant relative-key band; every variant against float64."""
    rng = np.random.default_rng(hash((case, dk)) & 0xFFFF)
    w = 4
    lens = [300, 129]
    q, k, v, erk, erv = _spiked(case, dk, w, sum(lens), rng)
    # _spiked puts the spike at key T - 40 of what it is given: key 89 of the second utterance (step 2 of 5), and key 260 (step 8 of 10) of the first
    if case in ("some_lanes", "all_lanes"):
        q2, k2, v2, e2, f2 = _spiked(case, dk, w, lens[0], np.random.default_rng(1))
        q[:, :lens[0]], k[:, :lens[0]], v[:, :lens[0]] = q2, k2, v2
    outs = _check_vits(f"{case} dk{dk}", q, k, v, erk, erv, lens, 1, dk, w, FRAMES, [-1, 0, 1, 2, 3, 4, 5], check_drop=False)
    for var in (3, 4, 5):
        np.testing.assert_array_equal(outs[var], outs[2])


# ---- DeBERTa ------------------------------------------------------------------------------------------------------------------------------------------

SHAPES = {"tiny": (4, 16, 8, 32, 0), "full": (16, 64, 256, 512, 1), "one": (1, 64, 256, 512, 1)}   # heads, d, buckets, max_rel, gap
LENGTHS = [1, 2, 3, 17, 63, 64, 65, 100, 127, 128, 129, 160, 300, 515, 1000]


def _db_inputs(rng, heads, d, span, N):
    H = heads * d
    q, k, v = (rng.standard_normal((H, N)).astype(np.float32) for _ in range(3))
    pk, pq = (rng.standard_normal((H, 2 * span)).astype(np.float32) for _ in range(2))
    return q, k, v, pk, pq


def _db_ref(q, k, v, pk, pq, lens, heads, d, buckets, max_rel, mask, dtype):
    span = buckets if buckets > 0 else max_rel
    out = np.empty(q.shape, np.float64)
    P = lambda a: a.astype(dtype).reshape(heads, d, 2 * span).transpose(0, 2, 1)
    for s in _segs(lens):
        T = s.stop - s.start
        qkv = [a[:, s].astype(dtype).reshape(heads, d, T).transpose(0, 2, 1) for a in (q, k, v)]
        rel = O.relative_position_vector(T, buckets, max_rel)
        m = np.ones(T, dtype) if mask is None else mask[s].astype(dtype)
        r = O.disentangled_attention(*qkv, P(pk), P(pq), rel, m, span, dtype(np.sqrt(d * 3)))
        out[:, s] = r.transpose(0, 2, 1).reshape(heads * d, T)
    return out


def _mask(kind, T):
    m = np.ones(T, np.uint8)
    if kind == "tail":
        m[max(1, T - T // 4):] = 0
    elif kind == "head":
        m[:70] = 0
    elif kind == "tile":
        m[32:64] = 0
    elif kind == "alternate":
        m[1::2] = 0
    elif kind == "single":
        m[:] = 0
        m[T // 2] = 1
    return m


def _check_deberta(name, q, k, v, pk, pq, lens, shape, mask, variants):
    heads, d, buckets, max_rel, gap = SHAPES[shape]
    ref = _db_ref(q, k, v, pk, pq, lens, heads, d, buckets, max_rel, mask, np.float64)
    r32 = _db_ref(q, k, v, pk, pq, lens, heads, d, buckets, max_rel, mask, np.float32)
    rows = np.ones(q.shape[1], bool) if mask is None else mask.astype(bool)      # unmasked queries
    err32 = float(np.abs(r32 - ref)[:, rows].max()) if rows.any() else 0.0
    tol = max(4 * err32, 5e-6 * max(1.0, float(np.abs(ref[:, rows]).max()) if rows.any() else 1.0))
    outs = {}
    for var in variants:
        try:
            got, _ = _deberta(q, k, v, pk, pq, lens, heads, d, buckets, max_rel, mask, gap, var)
        except _lib.Sbv2Error as e:
            assert var in (1, 2, 3) and "does not fit" in str(e), (name, var, e)
            continue
        assert np.isfinite(got).all(), (name, var)
        ratio = float(np.abs(got.astype(np.float64) - ref)[:, rows].max()) / tol if rows.any() else 0.0
        print(f"[deberta {name} variant {var}] worst error / tolerance = {ratio:.3f}")
        assert ratio <= 1.0, (name, var, ratio)
        outs[var] = got
    return outs


def _fits(var, T):
    return {1: T <= 64, 2: 64 < T <= 128, 3: 128 < T <= 8192}.get(var, True)


@pytest.mark.parametrize("shape", ["tiny", "full"])
def test_deberta_attention_lengths(shape):
    """Every variant (-1 .. 3) at T = 1 .. 1000 (single utterances; at the full shape, lengths past 128 reach the log-bucket range), each where its kernel
    fits (a forced kernel that does not fit must refuse with an error, not launch), against float64; tolerance max(4 err32, floor).  Poisoned gaps change
    no bit and no ctx column outside the utterance is written."""
    heads, d, buckets, max_rel, gap = SHAPES[shape]
    span = buckets if buckets > 0 else max_rel
    for T in LENGTHS:
        rng = np.random.default_rng(T)
        q, k, v, pk, pq = _db_inputs(rng, heads, d, span, T)
        outs = _check_deberta(f"{shape} T{T}", q, k, v, pk, pq, [T], shape, None, [-1, 0, 1, 2, 3])
        for var in (1, 2, 3):
            assert (var in outs) == _fits(var, T), (T, var)
        for var, o in outs.items():
            got, stray = _deberta(q, k, v, pk, pq, [T], heads, d, buckets, max_rel, None, gap, var, poison=1)
            assert stray == 0, (T, var, stray)
            np.testing.assert_array_equal(got, o, err_msg=f"T={T} variant {var}: poisoned gaps")


@pytest.mark.parametrize("kind", ["tail", "head", "tile", "alternate", "single"])
@pytest.mark.parametrize("shape", ["tiny", "full"])
def test_deberta_attention_masks(shape, kind):
    """Masked keys: the tail (as the models' tests have it), the first 70 keys (the long kernel's first key tiles are entirely masked: its online softmax
    starts from -FLT_MAX), one whole 32-key tile in the middle, every other key, a single unmasked key.  Unmasked query rows against float64, every output
    finite."""
    heads, d, buckets, max_rel, gap = SHAPES[shape]
    span = buckets if buckets > 0 else max_rel
    for T in (17, 64, 100, 128, 300, 1000):
        if kind == "head" and T <= 70 or kind == "tile" and T < 64:
            continue
        rng = np.random.default_rng(T + 1)
        q, k, v, pk, pq = _db_inputs(rng, heads, d, span, T)
        _check_deberta(f"{shape} T{T} {kind}", q, k, v, pk, pq, [T], shape, _mask(kind, T), [-1, 0, 1, 2, 3])


@pytest.mark.parametrize("mask", [None, "head"])
def test_deberta_attention_8192_tokens(mask):
    """The long kernel's limit, 8192 tokens, one head of 64 (full buckets), unmasked and with the first 70 keys masked, against float64 (query blocks);
    the unfused path on the same input."""
    heads, d, buckets = SHAPES["one"][:3]
    T = 8192
    rng = np.random.default_rng(8192)
    q, k, v, pk, pq = _db_inputs(rng, heads, d, buckets, T)
    m = None if mask is None else _mask(mask, T)
    outs = _check_deberta(f"T8192 {mask}", q, k, v, pk, pq, [T], "one", m, [-1, 0, 3])
    assert 3 in outs
    np.testing.assert_array_equal(outs[-1], outs[3])


@pytest.mark.parametrize("shape", ["tiny", "full"])
def test_deberta_attention_mixed_batch_dispatch(shape):
    """A mixed batch (short, 128-token and long utterances) under the model's dispatch (-1) equals each utterance forced onto its own class's kernel, bit
    for bit; the unfused path on batches whose longest utterance is <= 64, <= 128 and > 128 tokens (k_deberta_softmax_reg<64>, _reg<128> and the generic
    softmax) against float64."""
    heads, d, buckets, max_rel, gap = SHAPES[shape]
    span = buckets if buckets > 0 else max_rel
    lens = [17, 100, 300, 64, 1, 129]
    rng = np.random.default_rng(99)
    q, k, v, pk, pq = _db_inputs(rng, heads, d, span, sum(lens))
    m = np.concatenate([_mask("tail", T) for T in lens])
    auto, _ = _deberta(q, k, v, pk, pq, lens, heads, d, buckets, max_rel, m, gap, -1)
    for s, T in zip(_segs(lens), lens):
        var = 1 if T <= 64 else (2 if T <= 128 else 3)
        alone, _ = _deberta(q[:, s], k[:, s], v[:, s], pk, pq, [T], heads, d, buckets, max_rel, m[s], gap, var)
        np.testing.assert_array_equal(auto[:, s], alone, err_msg=f"T={T}")
    for sub in ([17, 64, 1], [100, 17, 1], lens):
        idx = [lens.index(T) for T in sub]
        segs = _segs(lens)
        cat = lambda a: np.concatenate([a[:, segs[i]] for i in idx], axis=1)
        mm = np.concatenate([m[segs[i]] for i in idx])
        _check_deberta(f"{shape} unfused {sub}", cat(q), cat(k), cat(v), pk, pq, sub, shape, mm, [0])
