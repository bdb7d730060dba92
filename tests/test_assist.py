"""Assist text (sbv2_assist, include/sbv2_hip.h): a second text's mean DeBERTa feature mixed into every token's feature of the spoken text.

CPU: a numpy restatement of the header's mean (one f64 order) and blend (two f32 products, one f32 sum) against the plain upstream formula and its
own properties; the oracle margin of the assisted rows the GPU tests use; the contracts of options, plan, batch, batcher, holder and REST against
fakes; the header and every refusal of the struct's fields, which need no GPU.
GPU (tiny models): the two kernels through sbv2_debug_assist_blend bit for bit against the restatement; the identity of a call without an
assist; an assisted row beside unassisted ones; the oracle; the effect on the text encoder; request streams; orchestrator and batcher."""
import ctypes as C
import functools
import os
import re
import types

import numpy as np
import pytest

import sbv2_oracle as O
from helpers import blob, make_utts, oracle_noise_w, oracle_noise_z, weights
from sbv2_api_amd import _lib, batcher, holder, model, orchestrator, synth

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
i64p, i32p, f64p = _lib.i64p, C.POINTER(C.c_int32), C.POINTER(C.c_double)
SO = orchestrator.SynthesizeOptions
NEW_SYMBOLS = ("sbv2_pipeline_run_assist", "sbv2_stream_begin_request_assist", "sbv2_debug_assist_blend")
SENTINEL = 0x5A5A5A5A


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------------------

def mean_ref(F, start, S):
    """The header's mean of the columns [start, start + S) of the f32 plane F [C][ld]: lane l adds the columns l, l + 64, ... in ascending order
    in f64 from 0.0, the 64 lanes fold pairwise (h = 32 .. 1: acc[l] += acc[l + h] for l < h), float(acc[0] / S)."""
    seg = np.asarray(F, np.float32)[:, start:start + S].astype(np.float64)
    seg = np.concatenate([seg, np.zeros((seg.shape[0], (-S) % 64))], axis=1).reshape(seg.shape[0], -1, 64)   # (x + 0.0 is exact)
    acc = np.zeros((seg.shape[0], 64))
    for k in range(seg.shape[1]):
        acc = acc + seg[:, k, :]
    h = 32
    while h >= 1:
        acc[:, :h] = acc[:, :h] + acc[:, h:2 * h]
        h //= 2
    return (acc[:, 0] / np.float64(S)).astype(np.float32)


def blend_ref(F, col_map, row_of, means, text_of, weight):
    """The header's blend: out[c][t] = F[c][q] * float(1.0 - w) + mean[c] * float(w) in f32 (numpy rounds each product and the sum: no fused
    multiply-add); a row without a text or with w == 0 is copied; a padding column stays 0."""
    F = np.asarray(F, np.float32)
    out = np.zeros((F.shape[0], len(col_map)), np.float32)
    for t, q in enumerate(col_map):
        if q < 0:
            continue
        u = row_of[t]
        if text_of[u] < 0 or weight[u] == 0:
            out[:, t] = F[:, q]
        else:
            wf, omw = np.float32(weight[u]), np.float32(1.0 - float(weight[u]))
            out[:, t] = F[:, q] * omw + means[text_of[u]] * wf
    return out


def word2ph_map(word2ph, col0=0):
    return [col0 + i for i, k in enumerate(np.asarray(word2ph).reshape(-1)) for _ in range(int(k))]


def assisted_features(h, word2ph, ha, w):
    """[bert_dim][T]: the features h [S][C] of a text, blended with the mean of the assist text's ha [S_a][C] at weight w and repeated by word2ph:
    what the library's gather hands the text encoder, by the restatement above."""
    F = np.concatenate([np.asarray(h, np.float32).T, np.asarray(ha, np.float32).T], axis=1)
    S, Sa = h.shape[0], ha.shape[0]
    cm = word2ph_map(word2ph)
    return blend_ref(F, cm, [0] * len(cm), [mean_ref(F, S, Sa)], [0], [w])


# ---- the models and requests the tests share ------------------------------------------------------------------------------------------------------------

KEYS = ("input_ids", "word2ph", "phones", "tones", "langs")
AIDS = [1, 17, 44, 9, 71, 30, 5, 62, 2]            # the assist text of the GPU tests, 9 tokens ([CLS] .. [SEP])
AIDS2 = [1, 80, 12, 55, 2]                         # ... and another one
W = 0.7
ROW_OPTS = dict(sdp_ratio=0.3, length_scale=1.1, noise_scale=orchestrator.NOISE_SCALE, noise_scale_w=orchestrator.NOISE_SCALE_W, noise_seed=4242)
G_SIZES, G_SEED0 = [7, 15, 5], 211                 # the three rows of the composition tests; row 1 is the assisted one
A_SIZES, A_SEED0, A_NOISE = [7, 15], 151, 4242     # request A of the orchestrator / batcher test (both sentences assisted)
A_OPTS = dict(sdp_ratio=0.3, length_scale=1.1)


def _cfgs():
    return weights("bert", "tiny", 3), weights("vits", "tiny", 5)


def _styles(vc):
    return synth.hash_normal(77, 3 * vc["style_dim"]).reshape(3, -1).astype(np.float32) * 0.1


def g_rows():
    """The three rows with their options and noise keys on them (row u draws the noise of index u wherever it runs)."""
    (bc, _), (vc, _) = _cfgs()
    return [dict(u, noise_index=i, **ROW_OPTS) for i, u in enumerate(make_utts(G_SIZES, bc, vc, seed0=G_SEED0, with_bert=False))]


def assisted(u, ids=AIDS, w=W):
    return dict(u, assist_ids=ids, assist_weight=w)


def a_sentences():
    (bc, _), (vc, _) = _cfgs()
    return [{k: u[k] for k in KEYS} for u in make_utts(A_SIZES, bc, vc, seed0=A_SEED0, with_bert=False)]


@functools.lru_cache(maxsize=None)
def _features(ids):
    (bc, bw), _ = _cfgs()
    return O.deberta_forward(bw, bc, np.asarray(ids, np.int64))


@functools.lru_cache(maxsize=None)
def oracle_assisted(which):
    """vits_forward's dict for an assisted row of the GPU tests: ("g", 1) = row 1 of the composition batch, ("a", j) = sentence j of request A."""
    (bc, bw), (vc, vw) = _cfgs()
    kind, j = which
    if kind == "g":
        u, o, style = g_rows()[j], dict(ROW_OPTS, noise_index=j), None
    else:
        u = a_sentences()[j]
        o = dict(A_OPTS, noise_scale=orchestrator.NOISE_SCALE, noise_scale_w=orchestrator.NOISE_SCALE_W, noise_seed=A_NOISE, noise_index=j)
        style = orchestrator.get_style_vector(_styles(vc), 1, 1.0)
    bert = assisted_features(_features(tuple(int(t) for t in u["input_ids"])), u["word2ph"], _features(tuple(AIDS)), W)
    T = len(u["phones"])
    return O.vits_forward(vw, vc, bert, u["phones"], u["tones"], u["langs"], 0, u["style"] if style is None else style, o["sdp_ratio"], o["length_scale"],
                          noise_w=oracle_noise_w(o["noise_seed"], o["noise_index"], T, o["noise_scale_w"]),
                          noise_z=oracle_noise_z(o["noise_seed"], o["noise_index"], vc["inter"], o["noise_scale"]), return_all=True)


# ---- CPU: the restatement against upstream's formula, and its own properties --------------------------------------------------------------------------------

@pytest.mark.parametrize("w", [0.7, 0.25, 1.0])
def test_restatement_is_upstreams_formula_to_f32_rounding(w):
    """res * (1 - w) + res_a.mean(0) * w in plain f32 on the tiny model's oracle features: per element within (S_a + 4) 2^-24 max|F|, the rounding of
    an f32 mean of S_a terms plus three f32 operations."""
    u = g_rows()[1]
    res, res_a = _features(tuple(int(t) for t in u["input_ids"])).astype(np.float32), _features(tuple(AIDS)).astype(np.float32)
    Sa = res_a.shape[0]
    up = res * np.float32(1 - w) + res_a.mean(0, dtype=np.float32) * np.float32(w)                       # [S][C]
    want = np.repeat(up, np.asarray(u["word2ph"]), axis=0).T
    got = assisted_features(res, u["word2ph"], res_a, w)
    bound = (Sa + 4) * 2.0 ** -24 * float(max(np.abs(res).max(), np.abs(res_a).max()))
    err = float(np.abs(got.astype(np.float64) - want).max())
    print(f"[assist] restatement vs upstream f32, w = {w}: max-abs {err:.3e} (bound {bound:.3e})")
    assert got.shape == want.shape == (res.shape[1], len(u["phones"])) and err < bound


def test_restatement_properties():
    rng = np.random.default_rng(5)
    F = (rng.standard_normal((9, 200)) * 3).astype(np.float32)
    m = mean_ref(F, 70, 130)
    np.testing.assert_allclose(m, F[:, 70:200].astype(np.float64).mean(1), rtol=1e-6, atol=1e-7)
    assert (mean_ref(F, 4, 1) == F[:, 4]).all()                                                           # one token: its own feature
    # w = 1: every column of the row is the mean; the row beside it is copied
    out = blend_ref(F, [3, 9, -1, 11], [0, 0, 0, 1], [m], [0, -1], [1.0, 0.3])
    assert (out[:, 0] == m).all() and (out[:, 1] == m).all() and (out[:, 2] == 0).all() and (out[:, 3] == F[:, 11]).all()
    # w = 0 is the copy, whatever the mean
    assert (blend_ref(F, [3], [0], [np.full(9, np.nan, np.float32)], [0], [0.0])[:, 0] == F[:, 3]).all()
    # w = 0.5 on two rows sharing a text: the planes differ by half the features' difference, to the rounding of the two sums
    out = blend_ref(F, [3, 9], [0, 1], [m], [0, 0], [0.5, 0.5]).astype(np.float64)
    d = (out[:, 0] - out[:, 1]) - 0.5 * (F[:, 3].astype(np.float64) - F[:, 9])
    assert np.abs(d).max() <= 2 * 2.0 ** -24 * np.abs(F).max()
    # the mean depends on its own columns only
    G = F.copy()
    G[:, :70] = 1e9
    assert (mean_ref(G, 70, 130) == m).all()


def test_assisted_rows_are_off_the_ceil_edges_on_the_oracle():
    """every assisted row the GPU tests compare durations of has each exp(logw) * length_scale at least 1e-3 from an integer (oracle)."""
    worst = 1.0
    for which, ls in ((("g", 1), ROW_OPTS["length_scale"]), (("a", 0), A_OPTS["length_scale"]), (("a", 1), A_OPTS["length_scale"])):
        w = np.exp(oracle_assisted(which)["logw"].astype(np.float64)) * ls
        worst = min(worst, float(np.abs(w - np.round(w)).min()))
    print(f"[assist] oracle ceil margin of the assisted rows: {worst:.3e}")
    assert worst >= 1e-3


# ---- CPU: header, ABI and the refusals that need no GPU ------------------------------------------------------------------------------------------------------

def test_new_symbols_are_exported_and_declared():
    header = open(os.path.join(ROOT, "include", "sbv2_hip.h")).read()
    core = open(os.path.join(ROOT, "include", "sbv2_core.hpp")).read()
    l = _lib.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in core, name
        assert name in _lib.SYMBOLS and getattr(l, name) is not None, name
    assert "} sbv2_assist;" in header and "sbv2_assist" in core and C.sizeof(_lib.Sbv2Assist) == 48
    assert C.sizeof(_lib.Sbv2UttOptions) == 48                                   # the existing struct is as it was
    for word in ("Not built", "sbv2_node_", "ascending", "h = 32, 16, 8, 4, 2, 1"):
        assert word in header[header.index("new: assist text"):header.index("} sbv2_assist;")], word


def c_assist(texts, text_of, weight, reserved=0, null=None, n_texts=None):
    """(struct, keep-alive) from python lists; null: the name of an array handed in as NULL."""
    ids = np.ascontiguousarray(np.concatenate([np.asarray(t, np.int64) for t in texts]) if texts else np.zeros(0, np.int64))
    lens, of, w = np.array([len(t) for t in texts], np.int64), np.array(text_of, np.int32), np.array(weight, np.float64)
    p = dict(token_ids=ids.ctypes.data_as(i64p), s_lens=lens.ctypes.data_as(i64p), text_of=of.ctypes.data_as(i32p), weight=w.ctypes.data_as(f64p))
    if null:
        p[null] = None
    return _lib.Sbv2Assist(len(texts) if n_texts is None else n_texts, p["token_ids"], p["s_lens"], p["text_of"], p["weight"], reserved), (ids, lens, of, w)


def _tail(b):
    return b.ids.ctypes.data_as(i64p), b.s_lens.ctypes.data_as(i64p), b.w2p.ctypes.data_as(i64p)


def test_every_refusal_of_the_structs_fields_comes_before_the_handles():
    l = _lib.lib()
    b = model.Pipeline.prepare(None, g_rows()[:2])
    big = [1] * 4
    bad = [(c_assist([AIDS], [0, -1], [0.5, 0.0], reserved=1), "reserved"),
           (c_assist([], [0, -1], [0.5, 0.0]), "n_texts"),
           (c_assist([AIDS], [0, -1], [0.5, 0.0], n_texts=-3), "n_texts"),
           (c_assist([AIDS, big], [0, -1], [0.5, 0.0]), None)]   # (a good one: see below)
    for name in ("token_ids", "s_lens", "text_of", "weight"):
        bad.append((c_assist([AIDS], [0, -1], [0.5, 0.0], null=name), "null"))
    zero_len = c_assist([AIDS, big], [0, -1], [0.5, 0.0])
    zero_len[1][1][1] = 0
    too_long = c_assist([AIDS, big], [0, -1], [0.5, 0.0])
    too_long[1][1][1] = 1 << 20
    bad += [(zero_len, "assist text 1"), (too_long, "assist text 1"),
            (c_assist([AIDS], [0, 1], [0.5, 0.5]), "text_of of row 1"), (c_assist([AIDS], [-2, 0], [0.5, 0.5]), "text_of of row 0"),
            (c_assist([AIDS], [0, 0], [0.5, float("nan")]), "weight of row 1"), (c_assist([AIDS], [0, 0], [-0.01, 0.5]), "weight of row 0"),
            (c_assist([AIDS], [-1, 0], [0.5, 1.01]), "weight of row 1")]
    rq_gaps = np.zeros(2, np.int64)
    rq = _lib.Sbv2StreamRequest(rq_gaps.ctypes.data_as(i64p), None, None, 0, 0)
    h, tot = C.c_void_p(), C.c_int64(-5)
    for (a, keep), word in bad:
        lens = np.full(2, -7, np.int64)
        rc = l.sbv2_pipeline_run_assist(None, C.byref(b.c), None, C.byref(a), *_tail(b), lens.ctypes.data_as(i64p))
        msg = l.sbv2_last_error().decode()
        assert rc != 0 and (lens == -7).all()
        assert (word in msg) if word else ("bad arguments" in msg), (word, msg)          # a good struct reaches the (NULL) handle
        rc = l.sbv2_stream_begin_request_assist(None, None, C.byref(b.c), None, C.byref(a), *_tail(b), 16, C.byref(rq), None, None, C.byref(h), C.byref(tot),
                                                None, None, None)
        msg = l.sbv2_last_error().decode()
        assert rc != 0 and not h.value and tot.value == -5
        assert (word in msg) if word else ("bad arguments" in msg), (word, msg)
    # a weight is not read where text_of is -1; an unused assist text is allowed; NULL is the call without
    good = [c_assist([AIDS, big], [-1, 0], [float("nan"), 1.0]), c_assist([AIDS], [-1, -1], [7.0, -3.0]), (None, None)]   # (struct, its arrays)
    for a, keep in good:
        rc = l.sbv2_pipeline_run_assist(None, C.byref(b.c), None, C.byref(a) if a is not None else None, *_tail(b), np.zeros(2, np.int64).ctypes.data_as(i64p))
        assert rc != 0 and b"bad arguments" in l.sbv2_last_error()
    # the hook checks its tables the same way, before any device call
    F = np.zeros((2, 8), np.float32)
    for kw, word in ((dict(text_of=[1]), "text_of of row 0"), (dict(weight=[1.5]), "weight of row 0"), (dict(a_len=[9]), "assist sequence 0"),
                     (dict(col_map=[8]), "column map"), (dict(row_of=[1]), "row_of")):
        args = dict(col_map=[1], row_of=[0], a_start=[2], a_len=[3], text_of=[0], weight=[0.5])
        args.update(kw)
        with pytest.raises(model.Sbv2Error, match=word):
            model.debug_assist_blend(F, device=0, **args)


# ---- CPU: the contracts of the Python layers, against fakes ------------------------------------------------------------------------------------------------

STYLES = np.zeros((2, 4), np.float32)


class FakePipe:
    """Records every run; the PCM of row i is lens[i] samples of the row's tag."""
    entry_points = model.Pipeline.entry_points

    def __init__(self, bert=None, vits=None):
        self.runs, self.batches = 0, []

    def prepare(self, utts, **kw):
        return types.SimpleNamespace(utts=[dict(u) for u in utts], kw=kw, lens=np.array([len(u["phones"]) for u in utts], np.int64), ticket=None)

    def run(self, b):
        self.runs += 1
        b.ticket = self.runs
        self.batches.append(b)
        return b.lens

    def fetch(self, b):
        return [np.full(int(n), u["tag"], np.float32) for n, u in zip(b.lens, b.utts)]

    def close(self):
        pass


class OldPipe(FakePipe):
    """A pipeline from before the assist: it does not name sbv2_pipeline_run_assist."""
    entry_points = ("sbv2_pipeline_run", "sbv2_pipeline_run_opts")


class NoListPipe(FakePipe):
    entry_points = None


def _sent(tag, n=3, **extra):
    return dict(dict(phones=[0] * n, tag=float(tag), input_ids=[1, 5, 2]), **extra)


def _pairs(b):
    return [(u.get("assist_ids"), u.get("assist_weight")) for u in b.utts]


def test_options_are_checked_at_construction():
    o = SO()
    assert o.assist_ids is None and o.assist_weight == 0.7 and orchestrator.assist_options(o) is None
    assert orchestrator.assist_options(SO(assist=AIDS)) == (AIDS, 0.7)
    assert orchestrator.assist_options(SO(assist=dict(input_ids=np.array(AIDS), word2ph=[1]), assist_weight=1)) == (AIDS, 1.0)
    assert orchestrator.assist_options(SO(assist=AIDS, assist_weight=0)) is None and orchestrator.assist_options(SO(assist=AIDS, assist_weight=0.0)) is None
    for bad in (-0.01, 1.01, float("nan"), float("inf"), "0.5", True, None, [0.5]):
        with pytest.raises(model.Sbv2Error, match="assist_weight"):
            SO(assist=AIDS, assist_weight=bad)
        with pytest.raises(model.Sbv2Error, match="assist_weight"):
            SO(assist_weight=bad)
    for bad in (5, dict(word2ph=[1]), [], [1, -2], [1.5], [True], b"ab"):
        with pytest.raises(model.Sbv2Error, match="assist"):
            SO(assist=bad)
    # a str is a text for a holder to parse: the routes refuse it unparsed, and at a weight of 0 it is nothing
    with pytest.raises(model.Sbv2Error, match="not parsed"):
        orchestrator.easy_synthesize(FakePipe(), [_sent(1)], STYLES, options=SO(assist="happy"), noise_seed=1)
    assert orchestrator.assist_options(SO(assist="happy", assist_weight=0)) is None


def test_plan_puts_the_pair_on_every_utterance():
    plan = orchestrator.RequestPlan([_sent(1), None, _sent(2)], STYLES, 0, 0, SO(assist=AIDS, assist_weight=0.4))
    assert [(u["assist_ids"], u["assist_weight"]) for u in plan.utts] == [(AIDS, 0.4)] * 2
    for o in (None, SO(), SO(assist=AIDS, assist_weight=0.0), SO(assist_weight=0.9)):
        plan = orchestrator.RequestPlan([_sent(1), _sent(2)], STYLES, 0, 0, o)
        assert all("assist_ids" not in u and "assist_weight" not in u for u in plan.utts)


def test_batch_deduplicates_equal_id_sequences():
    rows = g_rows()
    b = model.Pipeline.prepare(None, [assisted(rows[0], AIDS, 0.7), assisted(rows[1], AIDS2, 0.2), assisted(rows[2], list(AIDS), 1.0)])
    assert b.assist.n_texts == 2 and list(b.assist_of) == [0, 1, 0] and list(b.assist_w) == [0.7, 0.2, 1.0]
    assert list(b.assist_lens) == [len(AIDS), len(AIDS2)] and list(b.assist_ids) == AIDS + AIDS2
    b = model.Pipeline.prepare(None, [rows[0], assisted(rows[1], AIDS2, 0.2), assisted(rows[2], AIDS, 0.0)])   # a weight of 0 is no assist
    assert b.assist.n_texts == 1 and list(b.assist_of) == [-1, 0, -1] and list(b.assist_ids) == AIDS2
    assert model.Pipeline.prepare(None, rows).assist is None and model.Pipeline.prepare(None, [assisted(rows[0], AIDS, 0)]).assist is None
    for bad, word in ((dict(assist_ids=AIDS), "assist_weight"), (dict(assist_ids=AIDS, assist_weight=1.5), r"\[0, 1\]"),
                      (dict(assist_ids=AIDS, assist_weight=float("nan")), r"\[0, 1\]"), (dict(assist_ids=[], assist_weight=0.5), "empty")):
        with pytest.raises(model.Sbv2Error, match=word):
            model.Pipeline.prepare(None, [rows[0], dict(rows[1], **bad)])
    # a single-utterance stream cannot carry one: refused before any call, the request stream named
    fake = types.SimpleNamespace(handle=None)
    with pytest.raises(model.Sbv2Error, match="gaps="):
        model.StreamHandle(fake, fake, assisted(rows[0]), 16)


def test_routes_and_batcher_carry_the_assist_per_request():
    pipe = FakePipe()
    req = [_sent(1), _sent(2)]
    plain = orchestrator.easy_synthesize(pipe, req, STYLES, noise_seed=1)
    assert _pairs(pipe.batches[-1]) == [(None, None)] * 2
    for o in (SO(assist=AIDS, assist_weight=0.0), SO(assist_weight=0.3)):
        assert orchestrator.easy_synthesize(pipe, req, STYLES, noise_seed=1, options=o) == plain and _pairs(pipe.batches[-1]) == [(None, None)] * 2
    orchestrator.easy_synthesize(pipe, req, STYLES, noise_seed=1, options=SO(assist=AIDS))
    assert _pairs(pipe.batches[-1]) == [(AIDS, 0.7)] * 2
    # the batcher: three requests in one run, each row with its own request's pair
    rb = batcher.RequestBatcher(pipe, start=False, clock=lambda: 0.0, max_wait_ms=1000.0)
    futs = [rb.submit(req, STYLES, options=SO(assist=AIDS, assist_weight=0.7), noise_seed=1), rb.submit([_sent(3)], STYLES, noise_seed=2),
            rb.submit([_sent(4)], STYLES, options=SO(assist=AIDS2, assist_weight=0.25), noise_seed=3)]
    n = pipe.runs
    rb.start()
    rb.close()
    assert all(f.result(0)[:4] == b"RIFF" for f in futs) and pipe.runs == n + 1
    assert _pairs(pipe.batches[-1]) == [(AIDS, 0.7), (AIDS, 0.7), (None, None), (AIDS2, 0.25)]
    # a pipeline without the entry point: refused before any run, not served unassisted; without an assist it serves as ever
    for old in (OldPipe(), NoListPipe(), types.SimpleNamespace()):
        for call in (orchestrator.easy_synthesize, orchestrator.easy_synthesize_marks):
            with pytest.raises(model.Sbv2Error, match="sbv2_pipeline_run_assist"):
                call(old, req, STYLES, noise_seed=1, options=SO(assist=AIDS))
        assert getattr(old, "runs", 0) == 0
    old = OldPipe()
    rb = batcher.RequestBatcher(old, start=False, clock=lambda: 0.0, max_wait_ms=1000.0)
    f0, f1 = rb.submit(req, STYLES, options=SO(assist=AIDS), noise_seed=1), rb.submit(req, STYLES, options=SO(assist=AIDS, assist_weight=0), noise_seed=1)
    rb.start()
    rb.close()
    with pytest.raises(model.Sbv2Error, match="sbv2_pipeline_run_assist"):
        f0.result(0)
    assert f1.result(0) == plain and old.runs == 1


class _Session:
    def __init__(self, data, is_bert):
        pass

    def close(self):
        pass


def test_holder_parses_the_assist_text_with_its_front_end():
    import json
    style = json.dumps({"shape": [2, 4], "data": [[0.0] * 4, [1.0] * 4]}).encode()
    pipes = []

    def make(bert, vits):
        pipes.append(FakePipe())
        return pipes[-1]

    parse = lambda t: _sent(len(t), len(t), input_ids=[1] + [3 + ord(ch) % 50 for ch in t] + [2])
    h = holder.TTSModelHolder(b"bert", parse_text=parse, load_session=_Session, make_pipeline=make)
    h.load("m", style, b"M")
    o = SO(assist="happy!", assist_weight=0.6)
    h.easy_synthesize("m", "ab\ncde", options=o, noise_seed=1)
    assert _pairs(pipes[0].batches[-1]) == [(parse("happy!")["input_ids"], 0.6)] * 2 and o.assist_ids is None   # (the caller's options are not written to)
    h.easy_synthesize("m", "ab", options=SO(assist="happy!", assist_weight=0.0), noise_seed=1)
    assert _pairs(pipes[0].batches[-1]) == [(None, None)]
    fut = h.easy_synthesize_batched("m", "ab", options=o, noise_seed=1, batching=dict(max_wait_ms=1.0))
    assert fut.result(60)[:4] == b"RIFF" and _pairs(pipes[0].batches[-1]) == [(parse("happy!")["input_ids"], 0.6)]
    h.close()
    h = holder.TTSModelHolder(b"bert", load_session=_Session, make_pipeline=make)   # no front end: a refusal, as for `text`
    h.load("m", style, b"M")
    for call in (h.easy_synthesize, h.easy_synthesize_marks, h.easy_synthesize_batched, h.easy_synthesize_stream):
        with pytest.raises(model.Sbv2Error, match="no text front end"):
            call("m", [_sent(1)], options=o)
    h.close()


def test_rest_carries_the_two_fields_on_the_four_routes():
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient
    from sbv2_api_amd import rest
    wav = orchestrator.array_to_wav(np.zeros((1, 1, 10), np.float32))
    marks = {"sample_rate": 44100, "tokens": [], "words": []}

    class Pieces:
        total_samples = 10

        def __init__(self):
            self._left, self.marks = [wav], marks

        def __iter__(self):
            return self

        def __next__(self):
            if not self._left:
                raise StopIteration
            return self._left.pop()

        def take_marks(self):
            return {"delivered": 10, "tokens": []}

        def close(self):
            pass

    class H:
        calls = []

        def _note(self, route, options):
            self.calls.append((route, options.assist_text, options.assist_ids, options.assist_weight))

        def easy_synthesize(self, ident, text, style_id, speaker_id, options):
            self._note("plain", options)
            return wav

        def easy_synthesize_batched(self, ident, text, style_id, speaker_id, options, batching=None, marks=False):
            from concurrent.futures import Future
            self._note("batched", options)
            f = Future()
            f.set_result(wav)
            return f

        def easy_synthesize_marks(self, ident, text, style_id, speaker_id, options):
            self._note("marks", options)
            return wav, marks

        def easy_synthesize_stream(self, ident, text, style_id, speaker_id, options, **kw):
            self._note("stream_marks" if kw.get("levels") else "stream", options)
            return Pieces()

    h = H()
    c, cb = TestClient(rest.make_app(h), raise_server_exceptions=False), TestClient(rest.make_app(h, batching={}), raise_server_exceptions=False)
    body = {"text": "x", "ident": "m", "assist_text": "I am so happy!", "assist_text_weight": 0.4}
    routes = (("/synthesize", "plain", c), ("/synthesize_marks", "marks", c), ("/synthesize_stream", "stream", c), ("/synthesize_stream_marks", "stream_marks", c),
              ("/synthesize", "batched", cb))
    seen = []
    real = orchestrator.SynthesizeOptions

    def spy(**kw):
        seen.append(kw)
        return real(**kw)

    for route, name, client in routes:
        r = client.post(route, json=body)
        assert r.status_code == 200 and h.calls[-1] == (name, "I am so happy!", None, 0.4), (route, r.status_code, r.text)
        r = client.post(route, json=dict(body, assist_text_weight=0.7))
        assert r.status_code == 200 and h.calls[-1] == (name, "I am so happy!", None, 0.7)
        # the defaults (and an empty text) build the options that were built before: neither keyword is named
        orchestrator.SynthesizeOptions = spy
        try:
            for bd in ({"text": "x", "ident": "m"}, {"text": "x", "ident": "m", "assist_text": None, "assist_text_weight": 0.7}):
                assert client.post(route, json=bd).status_code == 200 and h.calls[-1] == (name, None, None, 0.7)
                assert "assist" not in seen[-1] and "assist_weight" not in seen[-1]
            assert client.post(route, json={"text": "x", "ident": "m", "assist_text": ""}).status_code == 200 and h.calls[-1][1] is None
        finally:
            orchestrator.SynthesizeOptions = real
        # a bad weight never reaches the holder: 4xx / 500 as a bad formant_scale on that route
        n = len(h.calls)
        for bad in (1.5, -0.1):
            for bd in (dict(body, assist_text_weight=bad), {"text": "x", "ident": "m", "assist_text_weight": bad}):
                r = client.post(route, json=bd)
                assert r.status_code == (400 if "stream" in route else 500) and "assist_weight" in r.text and len(h.calls) == n, (route, r.status_code, r.text)


# ---- GPU: the two kernels through the hook -------------------------------------------------------------------------------------------------------------------

S_AS = (1, 2, 63, 64, 65, 129, 512)
COL0, NSRC = 3, 40        # the assist sequences start at column 3 and abut; the batch's 40 source columns follow them; two unused columns end the plane


@functools.lru_cache(maxsize=None)
def hook_case(Cn):
    rng = np.random.default_rng(100 + Cn)
    starts = [COL0 + sum(S_AS[:a]) for a in range(len(S_AS))]
    src0 = starts[-1] + S_AS[-1]
    ld = src0 + NSRC + 2
    assert ld % 64 != 0
    F = (rng.standard_normal((Cn, ld)) * np.exp(rng.uniform(-6, 6, (Cn, 1)))).astype(np.float32)
    F[:, :COL0] = np.nan          # columns no sequence and no map entry names: a read outside a sequence poisons its mean
    F[:, src0 + NSRC:] = np.nan
    means = [mean_ref(F, s, S) for s, S in zip(starts, S_AS)]
    return F, starts, src0, means


#          row:  0     1    2    3    4    5
TEXT_OF = [-1,    2,   3,   5,   5,   6]
WEIGHT = [0.9,  0.0, 1.0, 0.7, 0.7, 0.3]   # (row 0's weight is not read)


@gpu
@pytest.mark.parametrize("L", [1, 255, 256, 257])
@pytest.mark.parametrize("Cn", [1, 5, 1024])
def test_hook_equals_the_restatement_bit_for_bit(Cn, L):
    F, starts, src0, means = hook_case(Cn)
    col_map = [-1 if t % 9 == 4 else src0 + (t * 7) % NSRC for t in range(L)]
    row_of = [(t * 5 + 3) % 6 for t in range(L)]
    mean, out, stray, (mean_w, out_w) = model.debug_assist_blend(F, col_map, row_of, starts, S_AS, TEXT_OF, WEIGHT)
    assert stray == 0                                                             # nothing outside the outputs changed
    assert not (mean_w == SENTINEL).any() and not (out_w == SENTINEL).any()       # ... and nothing inside them was left out
    assert not np.isnan(mean).any() and not np.isnan(out).any()
    want_mean = np.stack(means)
    assert (mean_w == want_mean.view(np.uint32)).all(), int(np.argmax(mean_w != want_mean.view(np.uint32)))
    want = blend_ref(F, col_map, row_of, means, TEXT_OF, WEIGHT)
    assert (out_w == want.view(np.uint32)).all(), int(np.argmax(out_w != want.view(np.uint32)))
    pads = [t for t, q in enumerate(col_map) if q < 0]
    assert (out_w[:, pads] == 0).all()                                            # a padding column is exactly +0
    rows = np.asarray(row_of)
    for t in np.flatnonzero((rows == 0) | (rows == 1)):                           # no text, or a weight of 0: the plain gather's bits
        if col_map[t] >= 0:
            assert (out_w[:, t] == F[:, col_map[t]].view(np.uint32)).all()


# ---- GPU: the pipeline on the tiny models -------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tiny():
    prev = os.environ.get("SBV2_PIPELINE_DEPTH")
    os.environ["SBV2_PIPELINE_DEPTH"] = "1"           # one execution context: sbv2_vits_fetch_durations and the traces read the last run
    try:
        bs, vs = model.load_model(blob("bert", "tiny", 3), True), model.load_model(blob("vits", "tiny", 5), False)
        pipe = model.Pipeline(bs, vs)
    finally:
        if prev is None:
            del os.environ["SBV2_PIPELINE_DEPTH"]
        else:
            os.environ["SBV2_PIPELINE_DEPTH"] = prev
    yield types.SimpleNamespace(pipe=pipe, bs=bs, vs=vs)
    pipe.close(); bs.close(); vs.close()


def _run(t, utts, entry=None, assist="own", **kw):
    """(durations, [pcm per row]) of one run of `utts`.  entry None: Pipeline.run's own choice; "opts" / "assist": that C entry point called
    directly, the latter with `assist` (a struct, None = NULL, "own" = the batch's)."""
    l = _lib.lib()
    b = t.pipe.prepare(utts, **kw)
    if entry is None:
        t.pipe.run(b)
    else:
        opts = C.byref(b.opts) if b.opts is not None else None
        tail = _tail(b) + (b.lens.ctypes.data_as(i64p),)
        if entry == "opts":
            model.check(l.sbv2_pipeline_run_opts(t.pipe.h, C.byref(b.c), opts, *tail))
        else:
            a = b.assist if assist == "own" else assist
            model.check(l.sbv2_pipeline_run_assist(t.pipe.h, C.byref(b.c), opts, C.byref(a) if a is not None else None, *tail))
        b.ticket = l.sbv2_pipeline_last_ticket(t.pipe.h)
    pcm = [p.copy() for p in t.pipe.fetch(b)]
    d, _ = model.fetch_durations(t.vs, int(sum(len(u["phones"]) for u in utts)))
    return d, pcm


def _same_bits(x, y):
    return x.shape == y.shape and x.tobytes() == y.tobytes()


@gpu
def test_a_call_without_an_assist_is_the_call_it_always_was(tiny):
    """sbv2_pipeline_run_assist with assist = NULL, and with every text_of = -1, against sbv2_pipeline_run_opts: two rows, noise on."""
    rows = g_rows()[:2]
    d0, p0 = _run(tiny, rows, "opts")
    none_named, keep = c_assist([AIDS, AIDS2], [-1, -1], [0.5, float("nan")])
    for a in (None, none_named):
        d, p = _run(tiny, rows, "assist", a)
        np.testing.assert_array_equal(d, d0)
        assert all(_same_bits(x, y) for x, y in zip(p, p0))
    d, p = _run(tiny, rows)                                                      # ... and Pipeline.run keeps choosing it
    np.testing.assert_array_equal(d, d0)
    assert all(_same_bits(x, y) for x, y in zip(p, p0))


def _composition(tiny):
    rows = g_rows()
    t0, t1 = len(rows[0]["phones"]), len(rows[1]["phones"])
    d_plain, p_plain = _run(tiny, rows)
    d_mixed, p_mixed = _run(tiny, [rows[0], assisted(rows[1]), rows[2]])
    d_alone, p_alone = _run(tiny, [assisted(rows[1])])
    return (t0, t1), (d_plain, p_plain), (d_mixed, p_mixed), (d_alone, p_alone)


@gpu
def test_an_assisted_row_beside_unassisted_ones_size_independent_dispatch(tiny):
    """Only row 1 of 3 is assisted, under sbv2_debug_set_ksplit(0): rows 0 and 2 have the durations and PCM bytes of the run without any assist,
    row 1 those of the same utterance run assisted alone."""
    l = _lib.lib()
    prev = l.sbv2_debug_set_ksplit(0)
    try:
        (t0, t1), (d_plain, p_plain), (d_mixed, p_mixed), (d_alone, p_alone) = _composition(tiny)
    finally:
        l.sbv2_debug_set_ksplit(prev)
    np.testing.assert_array_equal(d_mixed[:t0], d_plain[:t0])
    np.testing.assert_array_equal(d_mixed[t0 + t1:], d_plain[t0 + t1:])
    np.testing.assert_array_equal(d_mixed[t0:t0 + t1], d_alone)
    assert _same_bits(p_mixed[0], p_plain[0]) and _same_bits(p_mixed[2], p_plain[2]) and _same_bits(p_mixed[1], p_alone[0])
    assert not _same_bits(p_mixed[1], p_plain[1])                                # (the assist does change the row it is on)


@gpu
def test_an_assisted_row_beside_unassisted_ones_default_dispatch(tiny):
    """The same three comparisons under the default dispatch: equal integer durations, PCM within 2e-4 (DeBERTa's small-grid summation order moves
    with the column count, as test_co_batching_leaves_a_request_as_it_is_alone says)."""
    (t0, t1), (d_plain, p_plain), (d_mixed, p_mixed), (d_alone, p_alone) = _composition(tiny)
    np.testing.assert_array_equal(d_mixed[:t0], d_plain[:t0])
    np.testing.assert_array_equal(d_mixed[t0 + t1:], d_plain[t0 + t1:])
    np.testing.assert_array_equal(d_mixed[t0:t0 + t1], d_alone)
    for name, x, y in (("row 0", p_mixed[0], p_plain[0]), ("row 2", p_mixed[2], p_plain[2]), ("row 1", p_mixed[1], p_alone[0])):
        assert x.shape == y.shape
        print(f"[assist] {name}, mixed run vs its own run: max-abs {float(np.abs(x - y).max()):.3e}")
        np.testing.assert_allclose(x, y, atol=2e-4, rtol=0)


@gpu
def test_the_assisted_row_against_the_oracle_and_the_effect_on_the_encoder(tiny):
    rows = g_rows()
    t0, t1 = len(rows[0]["phones"]), len(rows[1]["phones"])
    model.set_trace(tiny.vs, True)
    try:
        _run(tiny, rows)
        x_plain = [model.get_trace(tiny.vs, "x", u) for u in (0, 1)]
        d, p = _run(tiny, [rows[0], assisted(rows[1]), rows[2]])
        x_mixed = [model.get_trace(tiny.vs, "x", u) for u in (0, 1)]
    finally:
        model.set_trace(tiny.vs, False)
    r = oracle_assisted(("g", 1))
    np.testing.assert_array_equal(d[t0:t0 + t1], r["durations"])
    assert p[1].shape == r["pcm"].shape
    print(f"[assist] assisted row vs oracle on the restated blend: max-abs {float(np.abs(p[1] - r['pcm']).max()):.3e}")
    np.testing.assert_allclose(p[1], r["pcm"], atol=2e-4, rtol=0)
    # the blend reached the model: the text encoder's output of the assisted row moved, its neighbour's did not
    moved, still = float(np.abs(x_mixed[1] - x_plain[1]).max()), float(np.abs(x_mixed[0] - x_plain[0]).max())
    print(f"[assist] text encoder output, assisted vs not: row 1 moved by {moved:.3e}, row 0 by {still:.3e}")
    assert x_mixed[1].shape == x_plain[1].shape and moved > 1e-2 and still < 1e-4


# ---- GPU: streams -------------------------------------------------------------------------------------------------------------------------------------------

def _take_all(st):
    parts = []
    while (c := st.next()) is not None:
        parts.append(c)
    return parts


@gpu
@pytest.mark.parametrize("fmt", [None, model.PcmFormat(24000, "s16")], ids=["44k1-f32", "24k-s16"])
def test_request_stream_with_an_assisted_row_equals_the_joined_fetch(tiny, fmt):
    """(24 kHz s16 stands for the issue's 16 kHz s16: the tiny model's hop refuses 16 kHz, as the existing request-stream tests note.)"""
    rows = g_rows()
    utts = [rows[0], assisted(rows[1]), assisted(rows[2], AIDS2, 0.35)]
    ff = fmt or model.PcmFormat(44100, "f32")
    mg = model.stream_min_gap(fmt)
    gaps = (mg + 700, mg, 22050)
    b = tiny.pipe.prepare(utts)
    tiny.pipe.run(b)
    lens = [int(n) for n in b.lens]
    place = [0, lens[0] + gaps[0], lens[0] + gaps[0] + lens[1] + gaps[1]]
    joined = place[2] + lens[2] + gaps[2]
    want = tiny.pipe.fetch_format(b, ff, place, joined)[0]                       # (fetched before the stream reuses the handles' context)
    for chunk in (16, 50):
        st = model.StreamHandle(tiny.bs, tiny.vs, utts, chunk, fmt=fmt, gaps=gaps)
        assert st.total_samples == want.size
        got = np.concatenate(_take_all(st))
        st.close()
        assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), (chunk, int(np.argmax(got != want)))
    # a single utterance with an assist: refused, the request stream named; as a request of one row it streams
    with pytest.raises(model.Sbv2Error, match="gaps="):
        model.StreamHandle(tiny.bs, tiny.vs, utts[1], 16, fmt=fmt)
    st = model.StreamHandle(tiny.bs, tiny.vs, [utts[1]], 16, fmt=fmt, gaps=[0])
    one = np.concatenate(_take_all(st))
    st.close()
    assert one.size == model.pcm_format_length(ff, lens[1])


@gpu
def test_a_stream_without_an_assist_keeps_its_bytes(tiny, monkeypatch):
    """sbv2_stream_begin_request_assist with assist = NULL, and with every text_of = -1, delivers the bytes of sbv2_stream_begin_request_pitch."""
    l = _lib.lib()
    rows, gaps = g_rows(), (500, 0, 100)
    none_named, keep = c_assist([AIDS], [-1, -1, -1], [0.5, 0.5, 0.5])
    real_pitch, real_assist = l.sbv2_stream_begin_request_pitch, l.sbv2_stream_begin_request_assist
    got = {}
    for name in ("pitch", "null", "none_named"):
        def begin(bert, vits, batch, opts, ids, s_lens, w2p, chunk, rq, out, total, name=name):   # in place of sbv2_stream_begin_request
            if name == "pitch":
                return real_pitch(bert, vits, batch, opts, ids, s_lens, w2p, chunk, rq, None, None, out, total, None, None, None)
            a = C.byref(none_named) if name == "none_named" else None
            return real_assist(bert, vits, batch, opts, a, ids, s_lens, w2p, chunk, rq, None, None, out, total, None, None, None)
        monkeypatch.setattr(l, "sbv2_stream_begin_request", begin)
        st = model.StreamHandle(tiny.bs, tiny.vs, rows, 32, gaps=gaps)
        got[name] = np.concatenate(_take_all(st))
        st.close()
        monkeypatch.undo()
    assert got["pitch"].size > 0 and _same_bits(got["null"], got["pitch"]) and _same_bits(got["none_named"], got["pitch"])


# ---- GPU: orchestrator and batcher, end to end ------------------------------------------------------------------------------------------------------------------

def _wav_f32(wav):
    return np.frombuffer(wav[wav.index(b"data") + 8:], "<f4")


class _Recorder:
    """A pipeline proxy that keeps the number of assist sequences of every run (None: the run had no assist)."""

    def __init__(self, pipe):
        self._pipe, self.n_texts = pipe, []

    def run(self, b):
        self.n_texts.append(b.assist.n_texts if b.assist is not None else None)
        return self._pipe.run(b)

    def __getattr__(self, name):
        return getattr(self._pipe, name)


@gpu
def test_orchestrator_and_batcher_end_to_end(tiny):
    """Request A (2 sentences, assisted at 0.7) alone through easy_synthesize, and behind request B (3 sentences, another assist, other options) in
    one batcher run: the same integer durations (those of the oracle on the restated blend), PCM within 2e-4.  Two requests with the same assist
    ids in one run: the run holds one assist sequence."""
    (bc, _), (vc, _) = _cfgs()
    sa = a_sentences()
    sb = [{k: u[k] for k in KEYS} for u in make_utts([4, 22, 9], bc, vc, seed0=171, with_bert=False)]
    sv = _styles(vc)
    oa, ob = SO(assist=AIDS, assist_weight=W, **A_OPTS), SO(assist=dict(input_ids=AIDS2), assist_weight=0.4, sdp_ratio=0.8, length_scale=0.9)
    rec = _Recorder(tiny.pipe)
    alone = orchestrator.easy_synthesize(rec, sa, sv, 1, 0, oa, noise_seed=A_NOISE)
    ta, tb = sum(len(s["phones"]) for s in sa), sum(len(s["phones"]) for s in sb)
    d_alone, _ = model.fetch_durations(tiny.vs, ta)
    np.testing.assert_array_equal(d_alone, np.concatenate([oracle_assisted(("a", j))["durations"] for j in (0, 1)]))
    unassisted = orchestrator.easy_synthesize(rec, sa, sv, 1, 0, SO(**A_OPTS), noise_seed=A_NOISE)
    assert rec.n_texts == [1, None] and unassisted != alone
    rb = batcher.RequestBatcher(rec, start=False, max_wait_ms=1000.0)
    fb, fa = rb.submit(sb, sv, 2, 0, ob, noise_seed=99), rb.submit(sa, sv, 1, 0, oa, noise_seed=A_NOISE)
    rb.start()
    rb.close()
    d_both, _ = model.fetch_durations(tiny.vs, ta + tb)
    np.testing.assert_array_equal(d_both[tb:], d_alone)
    x, y = _wav_f32(fa.result(0)), _wav_f32(alone)
    assert x.shape == y.shape and rec.n_texts[-1] == 2 and fb.result(0)[:4] == b"RIFF"
    print(f"[assist] request A alone vs behind B (each with its own assist): max-abs {float(np.abs(x - y).max()):.3e}")
    np.testing.assert_allclose(x, y, atol=2e-4, rtol=0)
    # the same assist ids on two requests of one run: one sequence
    rb = batcher.RequestBatcher(rec, start=False, max_wait_ms=1000.0)
    f1, f2 = rb.submit(sb, sv, 2, 0, SO(assist=AIDS, assist_weight=0.2), noise_seed=5), rb.submit(sa, sv, 1, 0, oa, noise_seed=A_NOISE)
    rb.start()
    rb.close()
    assert rec.n_texts[-1] == 1 and f1.result(0)[:4] == b"RIFF"
    z = _wav_f32(f2.result(0))
    assert z.shape == y.shape
    np.testing.assert_allclose(z, y, atol=2e-4, rtol=0)
