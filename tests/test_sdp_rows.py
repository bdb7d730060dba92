"""The stochastic duration predictor runs only for the rows whose sdp_ratio is not 0, and bert_proj runs before the word2ph repeat.

Every comparison of the first part is between sbv2_debug_set_sdp_all(1) (every row through the predictor on the full text layout: what the
library did before) and (0) (the default) in ONE process: same utterances, same seeds, predicted durations, noise scales non-zero.  The two
must agree bit for bit: k_durations keeps the expression s * ratio + dp * (1 - ratio) with s = 0.0f where the predictor did not run, and a
row that does go through it sits on a text layout of its own on which every kernel of the chain is column-local or segment-local and the
LayerNorm kernels, whose summation order depends on the column count they are chosen for, are chosen for the whole batch's width.  The launch
profile (sbv2_prof_begin / _end) counts what was saved: the predictor's exact-f32 products, a number derived from the model's config.

The second part holds the device-resident path (bert_proj over DeBERTa's own columns, then the gather of H rows) to the host-feature path,
which still repeats the 1024-row features first and projects afterwards."""
import ctypes as C
import json

import numpy as np
import pytest

import sbv2_oracle as O
from helpers import blob, make_utts, oracle_noise_w, oracle_noise_z, weights
from sbv2_api_amd import _lib, model

gpu = pytest.mark.gpu

T_SIZES = [7, 15, 4, 22]      # tests/test_utt_options.py: unequal lengths, gaps between the segments
UTT_SEED0 = 151
NOISE = dict(length_scale=1.1, noise_scale=0.667, noise_scale_w=0.8)


def test_symbol_is_exported_and_declared():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "sbv2_hip.h")).read()
    assert re.search(r"\bsbv2_debug_set_sdp_all\(", header)
    assert "sbv2_debug_set_sdp_all" in _lib.SYMBOLS and _lib.lib().sbv2_debug_set_sdp_all is not None


def sdp_products(vc):
    """Exact-f32 implicit-GEMM launches of one pass through the predictor, from the config: sdp.pre and sdp.proj, one 1x1 per DDSConv layer of the
    conditioning stack, and per ConvFlow that runs in reverse (all but the first of sdp_flows) its DDSConv layers and its projection."""
    dds, convflows = vc["sdp_dds_layers"], vc["sdp_flows"] - 1
    return 2 + dds + convflows * (dds + 1)


def test_sdp_products_of_the_shipped_shape():
    assert sdp_products(dict(sdp_dds_layers=3, sdp_flows=4)) == 17   # the JP-Extra shape: 2 + 3 + 3 * 4
    assert sdp_products(dict(sdp_dds_layers=2, sdp_flows=2)) == 7    # one ConvFlow in reverse: 2 + 2 + 1 * 3


@pytest.fixture(scope="module")
def tiny():
    """One execution context, so that sbv2_vits_fetch_durations reads the run just made."""
    mp = pytest.MonkeyPatch()
    mp.setenv("SBV2_PIPELINE_DEPTH", "1")
    bs, vs = model.load_model(blob("bert", "tiny", 3), True), model.load_model(blob("vits", "tiny", 5), False)
    pipe = model.Pipeline(bs, vs)
    yield pipe, bs, vs
    pipe.close(); bs.close(); vs.close()
    mp.undo()
    assert _lib.lib().sbv2_debug_set_sdp_all(0) == 0   # every test put the default back


def _utts(sizes=T_SIZES, seed0=UTT_SEED0):
    bc, _ = weights("bert", "tiny", 3)
    vc, _ = weights("vits", "tiny", 5)
    return make_utts(sizes, bc, vc, seed0=seed0, with_bert=False)


def _rows(utts, ratios, index=None):
    return [dict(u, sdp_ratio=r, noise_seed=1000 + 7 * i, noise_index=i if index is None else index[i], **NOISE) for i, (u, r) in enumerate(zip(utts, ratios))]


def _run(pipe, vs, rows, sdp_all, profile=False):
    """(durations, logw, [pcm per row], implicit-GEMM launches or None) of one pipeline run under sbv2_debug_set_sdp_all(sdp_all)."""
    lib = _lib.lib()
    prev = lib.sbv2_debug_set_sdp_all(sdp_all)
    try:
        b = pipe.prepare(rows)
        assert b.opts is not None
        if profile:
            _lib.check(lib.sbv2_prof_begin())
        pipe.run(b)
        pcm = [x.copy() for x in pipe.fetch(b)]
        launches = None
        if profile:
            buf = C.create_string_buffer(1 << 16)
            _lib.check(lib.sbv2_prof_end(buf, len(buf)))
            launches = sum(int(r["launches"]) for r in json.loads(buf.value.decode()))
        d, lw = model.fetch_durations(vs, sum(u["T_text"] for u in rows))
        return d.copy(), lw.copy(), pcm, launches
    finally:
        lib.sbv2_debug_set_sdp_all(prev)


def _same(a, b, what, logw_bits=True):
    da, lwa, pa, _ = a
    db, lwb, pb, _ = b
    np.testing.assert_array_equal(da, db, err_msg=what + ": durations")
    if logw_bits:
        np.testing.assert_array_equal(lwa.view(np.uint32), lwb.view(np.uint32), err_msg=what + ": logw bits")
    else:
        assert (lwa == lwb).all(), what + ": logw"   # == : the sign of an exact zero may differ at ratio 0 (k_durations' header comment)
    assert len(pa) == len(pb)
    for i, (x, y) in enumerate(zip(pa, pb)):
        assert x.size > 0
        np.testing.assert_array_equal(x, y, err_msg=f"{what}: PCM of row {i}")


@gpu
def test_no_row_uses_the_predictor(tiny):
    """All rows at ratio 0: equal integers, logw equal under ==, PCM bit-identical, and exactly the predictor's products fewer in the launch profile."""
    pipe, _, vs = tiny
    vc, _ = weights("vits", "tiny", 5)
    rows = _rows(_utts(), [0.0] * 4)
    old, new = _run(pipe, vs, rows, 1, profile=True), _run(pipe, vs, rows, 0, profile=True)
    _same(old, new, "all rows at ratio 0", logw_bits=False)
    print(f"[sdp rows] implicit-GEMM launches: {old[3]} with the predictor for every row, {new[3]} without; derived difference {sdp_products(vc)}")
    assert old[3] - new[3] == sdp_products(vc)


@gpu
def test_every_row_uses_the_predictor(tiny):
    """All rows at 0.3: nothing changed, bits and launch count."""
    pipe, _, vs = tiny
    rows = _rows(_utts(), [0.3] * 4)
    old, new = _run(pipe, vs, rows, 1, profile=True), _run(pipe, vs, rows, 0, profile=True)
    _same(old, new, "all rows at ratio 0.3")
    assert old[3] == new[3] and old[3] > 0


def _alone(pipe, vs, row):
    """The row as a batch of one (its noise_index keeps its noise key)."""
    return _run(pipe, vs, [row], 0)


MIXED_RATIOS = [0.0, 0.3, 0.0, 1.0]


def _ceil_margin(row):
    """tests/test_utt_options.py's guard: the distance of exp(logw) * length_scale to the nearest integer, smallest over the row's symbols, on the numpy
    oracle run alone with the row's own options and noise."""
    bc, bw = weights("bert", "tiny", 3)
    vc, vw = weights("vits", "tiny", 5)
    bert = O.expand_bert_features(O.deberta_forward(bw, bc, row["input_ids"]), row["word2ph"])
    r = O.vits_forward(vw, vc, bert, row["phones"], row["tones"], row["langs"], row.get("sid", 0), row["style"], row["sdp_ratio"], row["length_scale"],
                       noise_w=oracle_noise_w(row["noise_seed"], row["noise_index"], row["T_text"], row["noise_scale_w"]),
                       noise_z=oracle_noise_z(row["noise_seed"], row["noise_index"], vc["inter"], row["noise_scale"]), return_all=True)
    w = np.exp(r["logw"].astype(np.float64)) * row["length_scale"]
    return float(np.abs(w - np.round(w)).min())


def test_needed_rows_of_the_mixed_case_are_off_the_ceil_edges():
    """A batch row and the same row alone agree in logw to 1e-3 only (other launch shapes); their integer durations are compared below, so, as in
    tests/test_utt_options.py, the rows are checked on the oracle (no GPU) to keep exp(logw) * length_scale at least 1e-3 away from every integer."""
    for r in _rows(_utts(), MIXED_RATIOS):
        if r["sdp_ratio"] != 0.0:
            assert _ceil_margin(r) >= 1e-3


@gpu
@pytest.mark.parametrize("perm", [[0, 1, 2, 3], [1, 0, 2, 3]], ids=["skipped-first", "needed-first-and-last"])
def test_some_rows_use_the_predictor(tiny, perm):
    """Ratios [0, 0.3, 0, 1] and the permutation with a needed row first and last: per row, durations, logw and PCM of the run on the second
    layout equal the run with every row through the predictor; and each needed row against the same row run alone, held to what
    tests/test_utt_options.py holds a batch row to against its utterance alone (logw 1e-3 with the predictor's noise, equal integers, PCM 2e-4; the
    integers are off the ceil edges, test_needed_rows_of_the_mixed_case_are_off_the_ceil_edges)."""
    pipe, _, vs = tiny
    rows = _rows(_utts(), MIXED_RATIOS)
    rows = [rows[i] for i in perm]
    old, new = _run(pipe, vs, rows, 1, profile=True), _run(pipe, vs, rows, 0, profile=True)
    _same(old, new, f"mixed rows {perm}", logw_bits=False)
    assert old[3] == new[3]   # the predictor still runs once: its launches cover fewer columns, they are not fewer
    offs = np.concatenate([[0], np.cumsum([r["T_text"] for r in rows])])
    for i, r in enumerate(rows):
        sl = slice(offs[i], offs[i + 1])
        if r["sdp_ratio"] != 0.0:   # a needed row: the very bits, zero signs included
            np.testing.assert_array_equal(old[1][sl].view(np.uint32), new[1][sl].view(np.uint32))
            d1, lw1, pcm1, _ = _alone(pipe, vs, r)
            np.testing.assert_allclose(new[1][sl], lw1, atol=1e-3, rtol=0)
            np.testing.assert_array_equal(new[0][sl], d1)
            assert new[2][i].shape == pcm1[0].shape
            np.testing.assert_allclose(new[2][i], pcm1[0], atol=2e-4, rtol=0)


@gpu
@pytest.mark.parametrize("case", ["one-row-0", "one-row-1", "needed-T1", "needed-between-skipped", "denormal-ratio"])
def test_smallest_shapes(tiny, case):
    pipe, _, vs = tiny
    vc, _ = weights("vits", "tiny", 5)
    if case == "one-row-0":
        rows, saved = _rows(_utts([7]), [0.0]), sdp_products(vc)
    elif case == "one-row-1":
        rows, saved = _rows(_utts([7]), [1.0]), 0
    elif case == "needed-T1":
        # the shortest text the front end produces for one phone has T_text > 1; a row of ONE column is built by cutting an utterance down
        u = _utts([1], seed0=400)[0]
        T = u["T_text"]
        u1 = dict(u, phones=u["phones"][:1], tones=u["tones"][:1], langs=u["langs"][:1], T_text=1,
                  word2ph=_first_column_word2ph(u["word2ph"]), forced_durations=u["forced_durations"][:1])
        assert T >= 1 and sum(u1["word2ph"]) == 1
        rows, saved = _rows([_utts([7])[0], u1, _utts([4], seed0=300)[0]], [0.0, 0.6, 0.0]), 0
    elif case == "needed-between-skipped":
        rows, saved = _rows(_utts([15, 7, 22]), [0.0, 0.5, 0.0]), 0   # the second layout's gaps differ from the text layout's
    else:
        # 1e-30f and a true f32 denormal: neither is 0, so the predictor runs for both rows (were it skipped, sdp_products(vc) launches would be missing below)
        rows, saved = _rows(_utts(), [0.0, 1e-30, 1e-40, 0.0]), 0
        assert np.float32(1e-30) != 0 and 0 < np.float32(1e-40) < np.finfo(np.float32).tiny
    old, new = _run(pipe, vs, rows, 1, profile=True), _run(pipe, vs, rows, 0, profile=True)
    _same(old, new, case, logw_bits=False)
    assert old[3] - new[3] == saved
    offs = np.concatenate([[0], np.cumsum([r["T_text"] for r in rows])])
    for i, r in enumerate(rows):
        if np.float32(r["sdp_ratio"]) != 0:
            sl = slice(offs[i], offs[i + 1])
            np.testing.assert_array_equal(old[1][sl].view(np.uint32), new[1][sl].view(np.uint32))


@gpu
@pytest.mark.parametrize("ratios", [[0.0, 0.3, 0.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0, 0.3]], ids=["one-needed", "first-and-last-needed"])
def test_second_layout_across_the_layernorm_threshold(tiny, ratios):
    """LayerNorm takes its small-grid kernels up to 1024 columns (launch_layernorm, ops.hip) and other kernels above; they sum a column's channels in
    another order.  Five rows of 201 .. 241 columns are more than 1024 columns on the text layout, the needed rows alone (at most 201 + 241 and two
    gaps) fewer: the predictor's LayerNorms on the second layout must still take the kernels of the whole batch's width, or a needed row's logw
    differs in f32 rounding from the run with every row through the predictor."""
    pipe, _, vs = tiny
    utts = _utts([100, 120, 105, 110, 115], seed0=600)
    assert sum(u["T_text"] for u in utts) > 1024
    assert sum(u["T_text"] + 64 for u, r in zip(utts, ratios) if r != 0.0) <= 1024   # (64: more than any gap and rounding of a text layout)
    rows = _rows(utts, ratios)
    old, new = _run(pipe, vs, rows, 1, profile=True), _run(pipe, vs, rows, 0, profile=True)
    _same(old, new, f"across the LayerNorm threshold {ratios}", logw_bits=False)
    assert old[3] == new[3]
    offs = np.concatenate([[0], np.cumsum([r["T_text"] for r in rows])])
    for i, r in enumerate(rows):
        if r["sdp_ratio"] != 0.0:
            sl = slice(offs[i], offs[i + 1])
            np.testing.assert_array_equal(old[1][sl].view(np.uint32), new[1][sl].view(np.uint32))


def _first_column_word2ph(word2ph):
    """word2ph of the utterance cut to its first text column: the first token that has columns keeps one, every other token none."""
    w = np.zeros_like(np.asarray(word2ph))
    w[int(np.nonzero(np.asarray(word2ph))[0][0])] = 1
    return w


@gpu
@pytest.mark.parametrize("ratio", [0.0, 0.3])
def test_bert_projection_before_the_repeat(tiny, ratio):
    """sbv2_pipeline_run (features stay on the device: bert_proj over DeBERTa's columns, then the gather) against sbv2_bert_predict_batch + the repeat
    on the host + sbv2_vits_synthesize_batch (host features: the repeat first, bert_proj over the text columns): the same DeBERTa launch, the same
    VITS launches behind bert_proj, so durations, logw and PCM are held to bit equality."""
    pipe, bs, vs = tiny
    utts = _utts()
    kw = dict(sdp_ratio=ratio, noise_seed=123, **NOISE)
    b = pipe.prepare(utts, **kw)
    assert b.opts is None
    pipe.run(b)
    got = [x.copy() for x in pipe.fetch(b)]
    total = sum(u["T_text"] for u in utts)
    d, lw = (a.copy() for a in model.fetch_durations(vs, total))
    hs = model.predict_batch(bs, [u["input_ids"] for u in utts])
    host = [dict(u, bert=np.repeat(h, np.asarray(u["word2ph"], np.int64), axis=0).T.copy()) for h, u in zip(hs, utts)]
    ref = model.synthesize_batch(vs, host, **kw)
    dr, lwr = model.fetch_durations(vs, total)
    np.testing.assert_array_equal(d, dr)
    np.testing.assert_array_equal(lw.view(np.uint32), lwr.view(np.uint32))
    assert len(got) == len(ref)
    for x, y in zip(got, ref):
        assert x.size > 0
        np.testing.assert_array_equal(x, y)
