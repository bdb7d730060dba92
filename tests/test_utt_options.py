"""Options per utterance (sbv2_utt_options, sbv2_pipeline_run_opts) and the fetch of a subset of a run's rows (sbv2_pipeline_fetch_request):
the ABI and its host-side refusals (CPU), the three kernels that read a row's options (launch by launch), the forward (a row depends on its
own options only; every row against the numpy oracle run alone) and the subset fetch against the references of the format / FLAC / loudness
tests."""
import ctypes as C
import io
import os
import re

import numpy as np
import pytest

import flac_reader as R
import sbv2_oracle as O
from helpers import blob, make_utts, noise_key, oracle_noise_w, oracle_noise_z, weights
from sbv2_api_amd import _lib, model, orchestrator, synth
from test_loudness import apply_gain, close_stats, meter
from test_ops_kernels import FRAMES, TEXT, _dur_window, _f, _i32, _i64, _layout, _noise_ref
from test_pcm_format import check_format, ref_format

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["sbv2_vits_synthesize_batch_opts", "sbv2_pipeline_run_opts", "sbv2_pipeline_fetch_request", "sbv2_debug_durations_rows",
               "sbv2_debug_noise_fill_rows", "sbv2_debug_expand_frames_rows"]
G64 = 0x9E3779B97F4A7C15
M64 = 2 ** 64 - 1


def _u64(a):
    return np.ascontiguousarray(a, np.uint64).ctypes.data_as(C.POINTER(C.c_uint64))


# ---- CPU ----------------------------------------------------------------------------------------------------------------------------------------------

def test_new_symbols_are_exported_and_declared():
    header = open(os.path.join(ROOT, "include", "sbv2_hip.h")).read()
    l = _lib.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.SYMBOLS and getattr(l, name) is not None, name
    for struct in ("sbv2_utt_options", "sbv2_fetch_request"):
        assert "} %s;" % struct in header


def _host_batch(n=3):
    utts = [synth.make_utterance(4 + i, O.DEBERTA_TINY, O.VITS_TINY, seed=900 + i) for i in range(n)]
    return model._Batch(utts, 0.2, 1.0, 0.6, 0.8, 5, False, False)


@pytest.mark.parametrize("field,value,word", [("length_scale", 0.0, "length_scale of row 1"), ("length_scale", -1.0, "length_scale of row 1"),
                                              ("length_scale", float("nan"), "length_scale of row 1"), ("length_scale", float("inf"), "length_scale of row 1"),
                                              ("sdp_ratio", 1.5, "sdp_ratio of row 1"), ("sdp_ratio", -0.1, "sdp_ratio of row 1"),
                                              ("sdp_ratio", float("nan"), "sdp_ratio of row 1"), ("noise_scale", -0.5, "noise_scale of row 1"),
                                              ("noise_scale_w", -0.5, "noise_scale_w of row 1"), ("noise_index", -1, "noise_index of row 1")])
def test_utt_options_are_refused_on_the_host_with_the_row_named(field, value, word):
    """The checks of sbv2_utt_options come before anything touches a handle: a null handle reaches them (and is refused itself when they pass)."""
    l = _lib.lib()
    b = _host_batch()
    arr = np.array([0, value, 0] if field == "noise_index" else [0.5, value, 0.5], np.int64 if field == "noise_index" else np.float32)
    o = _lib.Sbv2UttOptions()
    setattr(o, field, arr.ctypes.data_as(_lib.i64p if field == "noise_index" else _lib.f32p))
    for call in (lambda: l.sbv2_pipeline_run_opts(None, C.byref(b.c), C.byref(o), None, None, None, None),
                 lambda: l.sbv2_vits_synthesize_batch_opts(None, C.byref(b.c), C.byref(o), None)):
        assert call() != 0
        assert word in l.sbv2_last_error().decode(), l.sbv2_last_error()
    ok = _lib.Sbv2UttOptions()
    assert l.sbv2_pipeline_run_opts(None, C.byref(b.c), C.byref(ok), None, None, None, None) != 0
    assert b"bad arguments" in l.sbv2_last_error()


def test_fetch_request_refusals_that_need_no_run():
    l = _lib.lib()
    f, ln, lim = model.PcmFormat(16000, "s16"), model.Loudness(-23.0), model.Limiter(-16.0)
    rows, place = np.array([0], np.int32), np.array([0], np.int64)
    dst, got = np.full(16, 77, np.uint8), C.c_int64(-5)
    both = _lib.Sbv2FetchRequest(rows.ctypes.data_as(C.POINTER(C.c_int32)), 1, place.ctypes.data_as(_lib.i64p), 10, C.pointer(f.c), C.pointer(ln.c),
                                 C.pointer(lim.c), 0)
    assert l.sbv2_pipeline_fetch_request(None, 1, C.byref(both), dst.ctypes.data, dst.nbytes, C.byref(got), None) != 0
    assert b"not both" in l.sbv2_last_error()
    norows = _lib.Sbv2FetchRequest(None, 2, None, 10, C.pointer(f.c), None, None, 0)
    assert l.sbv2_pipeline_fetch_request(None, 1, C.byref(norows), dst.ctypes.data, dst.nbytes, C.byref(got), None) != 0
    assert b"bad fetch request" in l.sbv2_last_error()
    assert l.sbv2_pipeline_fetch_request(None, 1, None, dst.ctypes.data, dst.nbytes, C.byref(got), None) != 0
    assert (dst == 77).all() and got.value == -5


def test_prepare_builds_row_options_only_when_an_utterance_overrides():
    utts = [synth.make_utterance(4 + i, O.DEBERTA_TINY, O.VITS_TINY, seed=900 + i) for i in range(3)]
    b = model._Batch(utts, 0.25, 1.5, 0.6, 0.8, 5, False, False)
    b.set_row_options(utts)
    assert b.opts is None
    utts[1] = dict(utts[1], length_scale=0.5, noise_seed=2 ** 64 - 3)
    utts[2] = dict(utts[2], noise_index=7, sdp_ratio=1.0)
    b.set_row_options(utts)
    assert b.opts is not None
    sdp, ls, ns, nsw, seed, idx = b.rows
    np.testing.assert_array_equal(sdp, np.array([0.25, 0.25, 1.0], np.float32))
    np.testing.assert_array_equal(ls, np.array([1.5, 0.5, 1.5], np.float32))
    np.testing.assert_array_equal(ns, np.full(3, 0.6, np.float32))
    np.testing.assert_array_equal(nsw, np.full(3, 0.8, np.float32))
    assert seed.tolist() == [5, 2 ** 64 - 3, 5] and idx.tolist() == [0, 1, 7]


# ---- GPU: the kernels ---------------------------------------------------------------------------------------------------------------------------------

LENS = [1, 37, 300]   # shorter than a wave, no multiple of 64, across blocks


@gpu
def test_durations_rows():
    """Rows with their own (ratio, length_scale): logw and the integers equal the scalar hook's on each segment bit for bit; against float64 with the
    window of undecidable elements of test_ops_kernels.test_durations; gaps and masked columns 0."""
    l = _lib.lib()
    start, L = _layout(LENS, TEXT)
    rng = np.random.default_rng(31)
    sdp, dp = (1.2 * rng.standard_normal(L)).astype(np.float32), (1.2 * rng.standard_normal(L)).astype(np.float32)
    mask = np.zeros(L, np.uint8)
    for s, n in zip(start, LENS):
        mask[s:s + n] = 1
    mask[start[2] + 17] = 0   # a masked column inside a segment
    ratio, ls = np.array([0.0, 0.5, 1.0], np.float32), np.array([2.0, 0.7, 1.3], np.float32)
    logw, dur = np.empty(L, np.float32), np.empty(L, np.int32)
    stray = C.c_int64(-1)
    _lib.check(l.sbv2_debug_durations_rows(0, _f(sdp), _f(dp), mask.ctypes.data, _i64(np.asarray(LENS, np.int64)), 3, _f(ratio), _f(ls), _f(logw), _i32(dur),
                                           C.byref(stray)))
    assert stray.value == 0
    assert (logw[mask == 0] == 0).all() and (dur[mask == 0] == 0).all()
    for u, (s, n) in enumerate(zip(start, LENS)):
        lw1, d1 = np.empty(n, np.float32), np.empty(n, np.int32)
        a, b, m = sdp[s:s + n].copy(), dp[s:s + n].copy(), mask[s:s + n].copy()
        _lib.check(l.sbv2_debug_durations(0, _f(a), _f(b), m.ctypes.data, n, float(ratio[u]), float(ls[u]), _f(lw1), _i32(d1), None))
        np.testing.assert_array_equal(logw[s:s + n].view(np.uint32), lw1.view(np.uint32))
        np.testing.assert_array_equal(dur[s:s + n], d1)
        lw, dlw, p, w = _dur_window(a, b, float(ratio[u]), float(ls[u]))
        k = m.astype(bool)
        assert (np.abs(logw[s:s + n].astype(np.float64) - lw)[k] <= dlw[k] + 1e-45).all()
        ref, undec = np.ceil(p).astype(np.int64), np.abs(p - np.round(p)) <= w
        print(f"[durations_rows segment {u}] undecidable elements: {int((undec & k).sum())} of {int(k.sum())}")
        np.testing.assert_array_equal(dur[s:s + n][k & ~undec], ref[k & ~undec])
        assert (np.abs(dur[s:s + n].astype(np.int64) - ref)[k & undec] <= 1).all()


SEEDS = np.array([1234, 2 ** 63 + 5, 77], np.uint64)
INDEX = np.array([2, 0, 5], np.int32)


@gpu
@pytest.mark.parametrize("kind", [TEXT, FRAMES])
def test_noise_fill_rows(kind):
    """Row u draws hash_normal(noise_key(seed[u], index[u], stream)) scaled by scale[u]: the scalar hook's bits on every segment, synth.hash_normal's bits,
    exact zeros for a row whose scale is 0 and in the gaps, nothing written outside the plane."""
    l = _lib.lib()
    start, L = _layout(LENS, kind)
    ln = np.asarray(LENS, np.int64)
    scale = np.array([1.0, 0.0, 0.6], np.float32)
    for rows, stream in ((2, 0), (3, 1)):
        y = np.empty((rows, L), np.float32)
        stray = C.c_int64(-1)
        _lib.check(l.sbv2_debug_noise_fill_rows(0, _i64(ln), 3, kind, _u64(SEEDS), _i32(INDEX), stream, _f(scale), rows, _f(y), C.byref(stray)))
        assert stray.value == 0
        ref = np.zeros((rows, L), np.float32)
        for u in range(3):
            one = np.empty((rows, L), np.float32)
            _lib.check(l.sbv2_debug_noise_fill(0, _i64(ln), 3, kind, _i32(np.full(3, INDEX[u], np.int32)), int(SEEDS[u]), stream, float(scale[u]), rows, _f(one),
                                               None))
            s, n = start[u], LENS[u]
            np.testing.assert_array_equal(y[:, s:s + n].view(np.uint32), one[:, s:s + n].view(np.uint32))
            ref[:, s:s + n] = _noise_ref(LENS, start, L, np.full(3, INDEX[u]), int(SEEDS[u]), stream, rows)[:, s:s + n] * scale[u]
        np.testing.assert_array_equal(y, ref)
        assert (y[:, start[1]:start[1] + LENS[1]] == 0).all()


@gpu
def test_expand_frames_rows():
    """Row u's prior noise: key (seed[u], index[u], 1), scale noise_scale[u]; the scalar hook's bits per segment, a row with noise_scale 0 is the plain
    gather, gaps and unmapped frames 0."""
    l = _lib.lib()
    rng = np.random.default_rng(9)
    Cc, tlens = 5, [2, 7, 4]
    tstart, Lt = _layout(tlens, TEXT)
    fstart, Lf = _layout(LENS, FRAMES)
    m_p = rng.standard_normal((Cc, Lt)).astype(np.float32)
    logs_p = (0.5 * rng.standard_normal((Cc, Lt))).astype(np.float32)
    tok = np.full(Lf, -1, np.int32)
    for u in range(3):
        tok[fstart[u]:fstart[u] + LENS[u]] = tstart[u] + np.sort(rng.integers(0, tlens[u], LENS[u]))
    tok[fstart[2] + 5] = -1
    ln = np.asarray(LENS, np.int64)
    ns = np.array([0.667, 0.0, 0.3], np.float32)
    y = np.empty((Cc, Lf), np.float32)
    stray = C.c_int64(-1)
    _lib.check(l.sbv2_debug_expand_frames_rows(0, _f(m_p), _f(logs_p), Cc, Lt, _i32(tok), _i64(ln), 3, _u64(SEEDS), _i32(INDEX), _f(ns), _f(y), C.byref(stray)))
    assert stray.value == 0
    ok = tok >= 0
    assert (y[:, ~ok] == 0).all()
    for u in range(3):
        one = np.empty((Cc, Lf), np.float32)
        _lib.check(l.sbv2_debug_expand_frames(0, _f(m_p), _f(logs_p), Cc, Lt, _i32(tok), _i64(ln), 3, _i32(np.full(3, INDEX[u], np.int32)), int(SEEDS[u]),
                                              float(ns[u]), _f(one), None))
        s, n = fstart[u], LENS[u]
        np.testing.assert_array_equal(y[:, s:s + n].view(np.uint32), one[:, s:s + n].view(np.uint32))
    s, n = fstart[1], LENS[1]
    np.testing.assert_array_equal(y[:, s:s + n], m_p[:, tok[s:s + n]])   # noise_scale 0: the noise-free result exactly
    noise = _noise_ref(LENS, fstart, Lf, np.full(3, INDEX[0]), int(SEEDS[0]), 1, Cc)
    s, n = fstart[0], LENS[0]
    tk = tok[s:s + n]
    ref = m_p[:, tk].astype(np.float64) + noise[:, s:s + n].astype(np.float64) * float(ns[0]) * np.exp(logs_p[:, tk].astype(np.float64))
    assert np.abs(y[:, s:s + n] - ref).max() <= 1e-5 * max(1.0, np.abs(ref).max())


# ---- GPU: the forward ---------------------------------------------------------------------------------------------------------------------------------

T_SIZES = [7, 15, 4, 22]      # the sizes of test_gpu_parity.test_node_shards_equal_single_gpu_call
UTT_SEED0 = 151
ROW_OPTS = [dict(sdp_ratio=0.0, length_scale=1.0, noise_scale=0.667, noise_scale_w=0.8, noise_seed=11, noise_index=5),
            dict(sdp_ratio=0.3, length_scale=1.1, noise_scale=0.5, noise_scale_w=0.6, noise_seed=2 ** 63 + 5, noise_index=0),
            dict(sdp_ratio=0.7, length_scale=0.8, noise_scale=0.9, noise_scale_w=1.0, noise_seed=77, noise_index=9),
            dict(sdp_ratio=1.0, length_scale=1.3, noise_scale=0.3, noise_scale_w=0.4, noise_seed=123456789, noise_index=2)]
SCALARS = ("sdp_ratio", "length_scale", "noise_scale", "noise_scale_w")


@pytest.fixture
def tiny_pipe(monkeypatch):
    """One execution context: every run is the one sbv2_vits_fetch_durations reads."""
    monkeypatch.setenv("SBV2_PIPELINE_DEPTH", "1")
    bs, vs = model.load_model(blob("bert", "tiny", 3), True), model.load_model(blob("vits", "tiny", 5), False)
    pipe = model.Pipeline(bs, vs)
    yield pipe, vs
    pipe.close(); bs.close(); vs.close()


def _utts():
    bc, _ = weights("bert", "tiny", 3)
    vc, _ = weights("vits", "tiny", 5)
    return make_utts(T_SIZES, bc, vc, seed0=UTT_SEED0, with_bert=False)


def _run(pipe, vs, utts, **kw):
    b = pipe.prepare(utts, **kw)
    pipe.run(b)
    d, lw = model.fetch_durations(vs, sum(u["T_text"] for u in utts))
    return d, lw, pipe.fetch(b)


def _oracle_row(u, o):
    bc, bw = weights("bert", "tiny", 3)
    vc, vw = weights("vits", "tiny", 5)
    bert = O.expand_bert_features(O.deberta_forward(bw, bc, u["input_ids"]), u["word2ph"])
    return O.vits_forward(vw, vc, bert, u["phones"], u["tones"], u["langs"], u.get("sid", 0), u["style"], o["sdp_ratio"], o["length_scale"],
                          noise_w=oracle_noise_w(o["noise_seed"], o["noise_index"], u["T_text"], o["noise_scale_w"]),
                          noise_z=oracle_noise_z(o["noise_seed"], o["noise_index"], vc["inter"], o["noise_scale"]), return_all=True)


def _ceil_margin(r, length_scale):
    w = np.exp(r["logw"].astype(np.float64)) * length_scale
    return float(np.abs(w - np.round(w)).min())


def test_oracle_durations_of_the_forward_cases_are_off_the_ceil_edges():
    """the utterances of the forward tests are chosen so that exp(logw) * length_scale is at least 1e-3 away from an integer on every symbol
    (checked on the oracle alone, without a GPU): the equality of integer durations below is then not left to luck."""
    for u, o in zip(_utts(), ROW_OPTS):
        assert _ceil_margin(_oracle_row(u, o), o["length_scale"]) >= 1e-3


@gpu
@pytest.mark.parametrize("kw", [dict(forced=True), dict(sdp_ratio=0.3, length_scale=1.1, noise_scale=0.667, noise_scale_w=0.8, noise_seed=123)],
                         ids=["forced", "predicted-noisy"])
def test_broadcast_options_are_the_identity(tiny_pipe, kw):
    pipe, vs = tiny_pipe
    utts = _utts()
    d0, lw0, pcm0 = _run(pipe, vs, utts, **kw)
    rows = [dict(u, sdp_ratio=kw.get("sdp_ratio", 0.0), length_scale=kw.get("length_scale", 1.0), noise_scale=kw.get("noise_scale", 0.0),
                 noise_scale_w=kw.get("noise_scale_w", 0.0), noise_seed=kw.get("noise_seed", 0), noise_index=i) for i, u in enumerate(utts)]
    b = pipe.prepare(rows, forced=bool(kw.get("forced")))
    assert b.opts is not None
    d1, lw1, pcm1 = _run(pipe, vs, rows, forced=bool(kw.get("forced")))
    np.testing.assert_array_equal(d1, d0)
    np.testing.assert_array_equal(lw1.view(np.uint32), lw0.view(np.uint32))
    assert len(pcm1) == len(pcm0)
    for x, y in zip(pcm1, pcm0):
        np.testing.assert_array_equal(x, y)


@gpu
def test_a_row_depends_on_its_own_options_only(tiny_pipe):
    """A mixed run (four rows, all five values different) against four uniform runs of the same utterances through the scalar entry point, run i with
    row i's scalars and the seed that gives row i the same noise key: row i's logw, durations and PCM bit for bit; and every row of the mixed run
    against the numpy oracle run alone on that utterance (tolerances of test_gpu_parity.test_vits_tiny_batch_mixed: logw 1e-3 with SDP noise, PCM 2e-4)."""
    pipe, vs = tiny_pipe
    utts = _utts()
    dm, lwm, pcmm = _run(pipe, vs, [dict(u, **o) for u, o in zip(utts, ROW_OPTS)])
    offs = np.concatenate([[0], np.cumsum([u["T_text"] for u in utts])])
    for i, o in enumerate(ROW_OPTS):
        seed = (o["noise_seed"] + 2 * (o["noise_index"] - i) * G64) & M64   # noise_key(seed, i, s) == noise_key(noise_seed, noise_index, s)
        assert noise_key(seed, i, 1) == noise_key(o["noise_seed"], o["noise_index"], 1)
        du, lwu, pcmu = _run(pipe, vs, utts, noise_seed=seed, **{k: o[k] for k in SCALARS})
        sl = slice(offs[i], offs[i + 1])
        np.testing.assert_array_equal(lwm[sl].view(np.uint32), lwu[sl].view(np.uint32))
        np.testing.assert_array_equal(dm[sl], du[sl])
        np.testing.assert_array_equal(pcmm[i], pcmu[i])
        r = _oracle_row(utts[i], o)
        assert _ceil_margin(r, o["length_scale"]) >= 1e-3
        np.testing.assert_allclose(lwm[sl], r["logw"], atol=1e-3, rtol=0)
        np.testing.assert_array_equal(dm[sl], r["durations"])
        assert pcmm[i].shape == r["pcm"].shape
        np.testing.assert_allclose(pcmm[i], r["pcm"], atol=2e-4, rtol=0)


# ---- GPU: the subset fetch ----------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def five_rows():
    bc, _ = weights("bert", "tiny", 3)
    vc, _ = weights("vits", "tiny", 5)
    bs, vs = model.load_model(blob("bert", "tiny", 3), True), model.load_model(blob("vits", "tiny", 5), False)
    pipe = model.Pipeline(bs, vs)
    b = pipe.prepare(make_utts([9, 1, 23, 14, 40], bc, vc, seed0=501, with_bert=False), forced=True)
    pipe.run(b)
    native = [x.copy() for x in pipe.fetch(b)]
    yield pipe, b, native
    pipe.close(); bs.close(); vs.close()


def _join(native, rows, place, joined):
    t = np.zeros(joined, np.float32)
    for r, p in zip(rows, place):
        t[p:p + len(native[r])] = native[r]
    return t


@gpu
def test_fetch_request_of_all_rows_equals_the_six_joined_fetches(five_rows):
    pipe, b, native = five_rows
    place, joined = orchestrator.joined_placement(b.lens, [0, 2, 3, 5, 6], 8)
    rows = range(5)
    ln, lim = model.Loudness(-20.0, -1.0), model.Limiter(-16.0, -1.0, 6.0)
    for f in (model.PcmFormat(16000, "s16"), model.PcmFormat(48000, "s16")):
        assert pipe.fetch_request(b, rows, f, place, joined)[0].tobytes() == pipe.fetch_format(b, f, place, joined)[0].tobytes()
        assert pipe.fetch_request(b, rows, f, place, joined, flac=True)[0] == pipe.fetch_flac(b, f, place, joined)[0]
        for gain, pcm, flac in ((ln, pipe.fetch_loudness, pipe.fetch_flac_loudness), (lim, pipe.fetch_limited, pipe.fetch_flac_limited)):
            ref, rs = pcm(b, f, gain, place, joined)
            got, gs = pipe.fetch_request(b, rows, f, place, joined, gain=gain)
            assert got.tobytes() == ref[0].tobytes() and gs.tobytes() == rs[0].tobytes()
            ref, rs = flac(b, f, gain, place, joined)
            got, gs = pipe.fetch_request(b, rows, f, place, joined, gain=gain, flac=True)
            assert got == ref[0] and gs.tobytes() == rs[0].tobytes()
    f = model.PcmFormat(22050, "f32", True)
    assert pipe.fetch_request(b, rows, f, place, joined)[0].tobytes() == pipe.fetch_format(b, f, place, joined)[0].tobytes()


@gpu
def test_fetch_request_subset_data_movement_formats_and_repeatability(five_rows):
    pipe, b, native = five_rows
    rows = [3, 1]
    place = [1000, 1000 + len(native[3]) + 22050]
    joined = place[1] + len(native[1]) + 333
    t = _join(native, rows, place, joined)
    got, stats = pipe.fetch_request(b, rows, model.PcmFormat(), place, joined)
    assert stats is None and got.dtype == np.float32
    np.testing.assert_array_equal(got, t)   # identity format: pure data movement
    f = model.PcmFormat(16000, "s16")
    s16, _ = pipe.fetch_request(b, rows, f, place, joined)
    s16 = s16.copy()
    check_format(s16, ref_format(t, 16000, "s16", False), "s16", "rows 3,1 at 16 kHz s16")
    fl, _ = pipe.fetch_request(b, rows, f, place, joined, flac=True)
    d = R.read(fl)
    assert d["rate"] == 16000
    np.testing.assert_array_equal(d["samples"], s16)
    ln = model.Loudness(-23.0, -1.0)
    loud, st = pipe.fetch_request(b, rows, f, place, joined, gain=ln)
    y = ref_format(t, 16000, "f32", False)
    ref = meter(y, 16000, ln.target_lufs, ln.true_peak_max)
    close_stats(st, ref, what="rows 3,1 loudness")
    check_format(loud, apply_gain(y, ref[2], "s16"), "s16", "rows 3,1 loudness")
    # another subset in between, then the first again: the run's PCM is only read
    other = [0, 4, 2]
    oplace, ojoined = orchestrator.joined_placement([len(native[r]) for r in other], [0, 1, 2], 3)
    o16, _ = pipe.fetch_request(b, other, f, oplace, ojoined)
    check_format(o16, ref_format(_join(native, other, oplace, ojoined), 16000, "s16", False), "s16", "rows 0,4,2")
    again, _ = pipe.fetch_request(b, rows, f, place, joined)
    assert again.tobytes() == s16.tobytes()
    for x, y in zip(pipe.fetch(b), native):
        np.testing.assert_array_equal(x, y)


@gpu
def test_fetch_request_refusals_write_nothing(five_rows):
    pipe, b, native = five_rows
    l = _lib.lib()
    f, ln, lim = model.PcmFormat(16000, "s16"), model.Loudness(-23.0), model.Limiter(-16.0)
    lens = [len(x) for x in native]

    def call(rows, place, joined, ticket=None, cap=None, loud=None, limiter=None, flac=0):
        rw, pl = np.asarray(rows, np.int32), np.asarray(place, np.int64)
        dst, got = np.full(1 << 18, 77, np.uint8), C.c_int64(-5)
        req = _lib.Sbv2FetchRequest(rw.ctypes.data_as(C.POINTER(C.c_int32)), len(rw), pl.ctypes.data_as(_lib.i64p), joined, C.pointer(f.c), loud, limiter, flac)
        rc = l.sbv2_pipeline_fetch_request(pipe.h, b.ticket if ticket is None else ticket, C.byref(req), dst.ctypes.data,
                                           dst.nbytes if cap is None else cap, C.byref(got), None)
        return rc, l.sbv2_last_error().decode(), bool((dst == 77).all() and got.value == -5)

    joined = lens[3] + lens[1] + 100
    assert call([3, 1], [0, lens[3]], joined)[0] == 0
    for args, kw, word in ((([3, 3], [0, lens[3]], joined + lens[3]), {}, "listed twice"),
                           (([3, 5], [0, lens[3]], joined), {}, "outside the run"),
                           (([3, -1], [0, lens[3]], joined), {}, "outside the run"),
                           (([3, 1], [0, lens[3]], joined), dict(loud=C.pointer(ln.c), limiter=C.pointer(lim.c)), "not both"),
                           (([3, 1], [0, lens[3] - 1], joined), {}, "overlap"),
                           (([3, 1], [0, joined - 1], joined), {}, "outside the joined timeline"),
                           (([3, 1], [-1, lens[3]], joined), {}, "outside the joined timeline"),
                           (([3, 1], [0, lens[3]], joined), dict(ticket=b.ticket + 1), "unknown pipeline ticket"),
                           (([3, 1], [0, lens[3]], joined), dict(cap=16), "too small"),
                           (([3, 1], [0, lens[3]], joined), dict(cap=16, flac=1), "too small")):
        rc, msg, clean = call(*args, **kw)
        assert rc != 0 and word in msg and clean, (word, rc, msg, clean)
