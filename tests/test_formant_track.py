"""Formant tracking (sbv2_formant_track and its entry points; k_ftrack_runs / k_ftrack_path of csrc/formant_track.hip): the definition above the
struct in include/sbv2_hip.h restated in Python ints (`track_ref`), checked against brute force and judged as a tracker (CPU); the kernels, the
hook on samples, the pipeline and the refusals against that restatement, bit for bit (GPU).

The tracker's experiment.  The issue's signal (the 700 / 1200 / 2600 Hz vowel at 16 kHz with bursts of a weak resonance near 250 Hz) does not
shift the plain contour by a slot through THIS stage: at order 18 the fit never gives the extra resonance a root of its own, it drags the F1
root down instead (pulse-driven resonators at 200 - 300 Hz, 15 - 800 Hz wide, level 0.02 - 3 of the vowel's peak, and gated sinusoids at 100 -
250 Hz: F1 off by 61 - 443 Hz, never a seventh root).  No choice among the kept roots can repair a root that is not there.  So
the spurious root is placed where the tracker works, among the candidates: in bursts of a few frames a wide low root (250 Hz, 300 Hz wide)
enters the K = 6 candidates that the numpy restatement of the stage finds on the clean vowel, in front of F1, the sixth leaving.  The plain
first-3 selection then follows it on every burst frame (12 of 34 inner frames are a slot off); the tracked F1 .. F3 stay within 60 Hz of the
resonators on all 34 (worst 33.6 Hz, the stage's own figure) with the usual costs (1, 1, 4) and references 500 / 1500 / 2500 Hz.  The table
is constructed, not produced by a signal: the inserted root is far from every reference and 300 Hz wide, so nearly any positive costs win on
it.  The counts 12 / 0 show that the definition repairs a slot shift; they do not single out (1, 1, 4) among other values."""
import ctypes as C
import itertools

import numpy as np
import pytest

from sbv2_api_amd import _lib, batcher, model, orchestrator
from test_formant import FORMANTS, vowel
from test_formant_contour import FC, REQUEST, STYLES, ContourPipe, contour_ref
from test_spectrum import request_rows  # noqa: F401

gpu = pytest.mark.gpu
FT = model.FormantTrack
NEW_SYMBOLS = {"sbv2_pipeline_fetch_request_formant_track": 18, "sbv2_formant_track_check": 3, "sbv2_debug_formant_track": 13,
               "sbv2_stream_begin_request_formant_track": 25}
REFS = (500.0, 1500.0, 2500.0, 3500.0, 4500.0)
USUAL = (1.0, 1.0, 4.0)


def track_ref(cf, cb, T, ref_hz, freq_cost, bw_cost, jump_cost):
    """The definition in Python ints, run by run -> (f_hz [nf][T], bw_hz [nf][T], state [nf], the runs' path costs)."""
    Wf, Wb, Wj = (int(np.rint(v * 65536.0)) for v in (freq_cost, bw_cost, jump_cost))
    Rq = [max(int(np.rint(r)), 1) for r in ref_hz[:T]]
    nf = len(cf)
    Fq = [[max(int(np.rint(v)), 1) for v in row if v > 0] for row in cf]
    Bq = [[int(np.rint(min(v, 2.0 ** 24))) for v in row] for row in cb]
    of, ob, state, costs = np.zeros((nf, T)), np.zeros((nf, T)), -np.ones(nf, np.int32), []
    f = 0
    while f < nf:
        m = len(Fq[f])
        if m < T:                                                                # a cut: the plain contour's values
            of[f, :m], ob[f, :m] = cf[f][:m], cb[f][:m]
            f += 1
            continue
        e = f
        while e < nf and len(Fq[e]) >= T:
            e += 1
        states, cost, bps = None, None, []
        for g in range(f, e):
            now = list(itertools.combinations(range(len(Fq[g])), T))            # lexicographic
            loc = [sum(Wf * abs(Fq[g][c] - Rq[t]) // Rq[t] + Wb * Bq[g][c] // Fq[g][c] for t, c in enumerate(k)) for k in now]
            if states is None:
                cost, bp = loc, None
            else:
                jump = [[Wj * abs(b - a) // max(a, b) for b in Fq[g]] for a in Fq[g - 1]]
                best = [min((cost[ji] + sum(jump[j[t]][k[t]] for t in range(T)), ji) for ji, j in enumerate(states)) for k in now]
                cost, bp = [l + b[0] for l, b in zip(loc, best)], [b[1] for b in best]
            states = now
            bps.append((now, bp))
        k = cost.index(min(cost))
        costs.append(min(cost))
        for g in range(e - 1, f - 1, -1):
            now, bp = bps[g - f]
            state[g] = k
            of[g], ob[g] = [cf[g][c] for c in now[k]], [cb[g][c] for c in now[k]]
            k = bp[k] if bp else k
        f = e
    return of, ob, state, costs


def table(T, K, runs, seed, cuts=(1, 2, 1)):
    """Seeded integer-valued candidates: cuts[0] cut frames, then the runs with cut stretches of cuts[1], cuts[2], cuts[1], ... frames between
    them; m varies between T and K within a run and below T on a cut; F from a range narrow enough for ties."""
    rng, rows = np.random.default_rng(seed), []
    cut = lambda n: rows.extend(int(rng.integers(0, T)) for _ in range(n))
    cut(cuts[0])
    for i, n in enumerate(runs):
        rows.extend(int(rng.integers(T, K + 1)) for _ in range(n))
        cut(cuts[1 + i % 2])
    cf, cb = np.zeros((len(rows), K)), np.zeros((len(rows), K))
    for f, m in enumerate(rows):
        cf[f, :m], cb[f, :m] = np.sort(rng.integers(400, 400 + 6 * K, m)), rng.integers(0, 60, m)
    return cf, cb


# ---- host only ------------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_exported():
    for name, nargs in NEW_SYMBOLS.items():
        assert len(_lib.SYMBOLS[name][1]) == nargs and getattr(_lib.lib(), name)


@pytest.mark.parametrize("T,K,nf,seed", [(1, 1, 3, 0), (1, 3, 4, 1), (2, 2, 4, 2), (2, 3, 4, 3), (2, 3, 3, 4)])
def test_the_restatement_against_brute_force(T, K, nf, seed):
    cf, cb = table(T, K, (nf,), seed, cuts=(0, 0, 0))
    _, _, state, (cost,) = track_ref(cf, cb, T, REFS, 1.0, 0.5, 2.0)
    Fq, Bq = [[int(v) for v in r if v > 0] for r in cf], cb.astype(np.int64).tolist()
    every = []
    for path in itertools.product(*[list(itertools.combinations(range(len(r)), T)) for r in Fq]):
        c = sum(65536 * abs(Fq[f][k] - int(REFS[t])) // int(REFS[t]) + 32768 * Bq[f][k] // Fq[f][k] for f, st in enumerate(path) for t, k in enumerate(st))
        c += sum(131072 * abs(Fq[f][k] - Fq[f - 1][j]) // max(Fq[f][k], Fq[f - 1][j]) for f in range(1, nf) for j, k in zip(path[f - 1], path[f]))
        every.append(c)
    assert cost == min(every) and (state >= 0).all()


def test_the_restatement_as_a_tracker():
    sr, c = 16000, FC(160, 6)
    model.formant_contour_defaults(sr, c)
    _, _, sel = contour_ref(vowel(sr).astype(np.float64), sr, c)
    cf, cb, want = np.array([s[0] for s in sel]), np.array([s[1] for s in sel]), np.array([f for f, _ in FORMANTS])
    assert (cf > 0).all()
    for a, b in ((9, 13), (20, 23), (28, 33)):                                   # the bursts: a wide low root in front, the sixth leaves
        cf[a:b, 1:], cb[a:b, 1:] = cf[a:b, :-1].copy(), cb[a:b, :-1].copy()
        cf[a:b, 0], cb[a:b, 0] = 250.0, 300.0
    plain = (np.abs(cf[3:-3, :3] - want) > 60.0).any(axis=1)
    tf, _, state, _ = track_ref(cf, cb, 3, REFS, *USUAL)
    off = np.abs(tf[3:-3] - want)
    print(f"[formant track] plain first-3 a slot off on {plain.sum()} of {plain.size} inner frames; tracked worst |F - resonator| = {off.max(axis=0)} Hz")
    assert plain.sum() == 12 and (np.abs(cf[10, :3] - [250.0, 700.0, 1200.0]) <= 60.0).all()   # F1 arrives as F2
    assert (off <= 60.0).all() and (state >= 0).all()


def test_refusals_that_need_no_run():
    nan, ok, fc = float("nan"), FT(REFS[:3], 6, *USUAL), FC(160, 3)
    model.formant_track_check(16000, fc, ok)
    model.formant_track_check(16000, FC(160, 5), FT(REFS, 7, 0.0, 16.0, 0.0))
    for bad, what in ((FT((), 6), "n_tracks"), (FT(REFS + (5500.0,), 7), "n_tracks"), (FT(REFS[:3], 2), "candidates"), (FT(REFS[:3], 8), "candidates"),
                      (FT((500.0, 500.0, 2500.0)), "ref_hz"), (FT((0.0, 1500.0, 2500.0)), "ref_hz"), (FT((500.0, 1500.0, 8000.0)), "ref_hz"),
                      (FT((500.0, nan, 2500.0)), "ref_hz"), (FT(REFS[:3], 6, -0.1), "freq_cost"), (FT(REFS[:3], 6, 1.0, 16.5), "bw_cost"),
                      (FT(REFS[:3], 6, 1.0, 1.0, nan), "jump_cost")):
        with pytest.raises(model.Sbv2Error, match=what):
            model.formant_track_check(16000, fc, bad)
    with pytest.raises(model.Sbv2Error, match="candidates"):                     # K > order / 2
        model.formant_track_check(16000, FC(160, 3, order=10), ok)
    with pytest.raises(model.Sbv2Error, match="n_tracks"):                       # the contour's columns are the tracks
        model.formant_track_check(16000, FC(160, 4), ok)
    c, ct = fc.c_struct(0, 16000)[0], ok.c
    ct.reserved = 1
    assert _lib.lib().sbv2_formant_track_check(16000, C.byref(c), C.byref(ct)) == 1 and b"reserved" in _lib.lib().sbv2_last_error()
    ct.reserved = 0                                                              # a stream entry refuses a track before it looks at anything
    nul = [None] * 16
    assert _lib.lib().sbv2_stream_begin_request_formant_track(*nul[:8], 0, *nul[:7], C.byref(ct), *nul[:8]) == 1
    assert b"sbv2_pipeline_fetch_request_formant_track" in _lib.lib().sbv2_last_error()
    with pytest.raises(model.Sbv2Error, match="formant track needs formants"):
        model.Pipeline.fetch_request(None, None, [0], model.PcmFormat(16000, "s16"), [0], 0, formant_track=ok)


class TrackPipe(ContourPipe):
    """ContourPipe whose fetch_request knows formant_track: a tracked contour is the plain one doubled."""

    def fetch_request(self, b, rows, fmt, place, joined_len, formants=None, formant_track=None, **kw):
        res = super().fetch_request(b, rows, fmt, place, joined_len, formants=formants, **kw)
        self.calls[-1]["formant_track"] = formant_track
        if formant_track is not None:
            formants.f_hz = 2.0 * formants.f_hz
        return res


class UntrackedPipe(ContourPipe):
    """A pipeline from before the option: its fetch_request takes formants and no formant_track."""

    def fetch_request(self, b, rows, fmt, place, joined_len, formants=None, gain=None, flac=False, marks=False, env_hop=0):
        raise AssertionError("refused before any run")


def spec(ft):
    return ft and (ft.ref_hz, ft.candidates, ft.freq_cost, ft.bw_cost, ft.jump_cost)


def test_routes_carry_or_refuse_the_track():
    SO, so, pipe = orchestrator.SynthesizeOptions, dict(formants=2, formants_hz=1000, sample_rate=16000, encoding="s16"), TrackPipe()   # (frames centred in the stub's short tokens)
    ask = lambda p=pipe, **kw: orchestrator.easy_synthesize_marks(p, REQUEST, STYLES, noise_seed=1, options=SO(**dict(so, **kw)))[1]
    mk0 = ask()
    assert pipe.calls[-1]["formant_track"] is None and "tracked" not in mk0["formants"]
    mk = ask(formants_track=True)
    assert spec(pipe.calls[-1]["formant_track"]) == ((500.0, 1500.0), 5, *USUAL)   # the usual values
    assert mk["formants"] == dict(mk0["formants"], f_hz=[[2.0 * v for v in r] for r in mk0["formants"]["f_hz"]], tracked=True)
    for name in ("f1_hz", "f2_hz"):                                              # the tokens' means are of the tracked values
        assert [t[name] for t in mk["tokens"]] == [t[name] and 2.0 * t[name] for t in mk0["tokens"]] and any(t[name] for t in mk["tokens"])
    ask(formants_track=True, formants_candidates=7, formants_ref_hz=[400.0, 1400], formants_freq_cost=0.5, formants_bw_cost=2, formants_jump_cost=16.0)
    assert spec(pipe.calls[-1]["formant_track"]) == ((400.0, 1400.0), 7, 0.5, 2.0, 16.0)
    ask(formants_track=True, formants_order=8)
    assert pipe.calls[-1]["formant_track"].candidates == 4                       # order / 2 caps the default
    runs = pipe.runs
    for kw, what in ((dict(formants_candidates=9), "candidates"), (dict(formants_candidates=1), "candidates"), (dict(formants_jump_cost=17.0), "jump_cost"),
                     (dict(formants_ref_hz=[1500.0, 500.0]), "ref_hz"), (dict(formants_order=8, formants_candidates=5), "candidates"),
                     (dict(formants_freq_cost=float("nan")), "freq_cost")):
        with pytest.raises(orchestrator.FormantsError, match=what):
            ask(formants_track=True, **kw)
    for kw in (dict(formants_track=True), dict(formants=2, formants_candidates=5), dict(formants=2, formants_jump_cost=1.0), dict(formants=2, formants_track=1),
               dict(formants=6, formants_track=True), dict(formants=2, formants_track=True, formants_ref_hz=[500.0]),
               dict(formants=2, formants_track=True, formants_ref_hz="500"), dict(formants=2, formants_track=True, formants_candidates=5.0)):
        with pytest.raises(orchestrator.FormantsError, match="formants"):        # it needs formants, its fields need it; the types
            SO(**kw)
    with pytest.raises(orchestrator.FormantsError, match="/synthesize_marks"):
        orchestrator.easy_synthesize(pipe, REQUEST, STYLES, noise_seed=1, options=SO(formants_track=True, **so))
    for kw, what in ((dict(), "/synthesize_marks"), (dict(levels=True, formants=True), "one path")):
        with pytest.raises(orchestrator.FormantsError, match=what):              # every stream, the one with a formant contour included
            orchestrator.easy_synthesize_stream(None, None, REQUEST[:1], STYLES, options=SO(formants_track=True, **so), **kw)
    old = UntrackedPipe()
    with pytest.raises(model.Sbv2Error, match="formants_track needs a pipeline"): # never served untracked
        ask(old, formants_track=True)
    assert pipe.runs == runs and old.runs == 0
    rb = batcher.RequestBatcher(pipe, start=False, clock=lambda: 0.0, max_wait_ms=1000.0)
    f0 = rb.submit(REQUEST, STYLES, options=SO(formants_track=True, **so), noise_seed=1, marks=True)
    f1 = rb.submit(REQUEST, STYLES, options=SO(formants_track=True, **so), noise_seed=1)
    rb.start()
    rb.close()
    assert f0.result(0)[1]["formants"] == mk["formants"]
    with pytest.raises(orchestrator.FormantsError, match="/synthesize_marks"):
        f1.result(0)


def test_rest_carries_the_track_on_synthesize_marks_and_answers_400_elsewhere():
    pytest.importorskip("fastapi")
    from concurrent.futures import Future
    from fastapi.testclient import TestClient
    from sbv2_api_amd import rest
    wav, seen, marks = orchestrator.array_to_wav(np.zeros((1, 1, 10), np.float32)), [], {"sample_rate": 16000, "tokens": [], "words": []}

    class H:
        def easy_synthesize(self, ident, text, style_id, speaker_id, options):
            return wav

        def easy_synthesize_batched(self, ident, text, style_id, speaker_id, options, batching=None, marks=False):
            f = Future()
            try:
                f.set_result(self.easy_synthesize_marks(ident, text, style_id, speaker_id, options) if marks else wav)
            except Exception as e:
                f.set_exception(e)
            return f

        def easy_synthesize_marks(self, ident, text, style_id, speaker_id, options):
            fc = orchestrator.formants_options(options, options.sample_rate)
            seen.append(spec(orchestrator.formants_track_options(options, options.sample_rate, fc)))
            return wav, marks

        def easy_synthesize_stream(self, ident, text, style_id, speaker_id, options, **kw):
            raise AssertionError("a stream with a formant track must be refused before the holder is asked")

    body = {"text": "x", "ident": "m", "formants": 3, "sample_rate": 16000, "encoding": "s16", "formants_track": True, "formants_candidates": 7,
            "formants_ref_hz": [450, 1450, 2450], "formants_bw_cost": 2.0}
    for c in (TestClient(rest.make_app(H()), raise_server_exceptions=False), TestClient(rest.make_app(H(), batching={}), raise_server_exceptions=False)):
        assert c.post("/synthesize_marks", json=body).status_code == 200 and seen[-1] == ((450.0, 1450.0, 2450.0), 7, 1.0, 2.0, 4.0)
        assert c.post("/synthesize_marks", json={"text": "x", "ident": "m", "formants": 3}).status_code == 200 and seen[-1] is None
        for bad, what in ((dict(body, formants_candidates=8), "candidates"), (dict(body, formants=None), "formants"), (dict(body, formants_track=False), "formants_track")):
            r = c.post("/synthesize_marks", json=bad)
            assert r.status_code == 400 and what in r.text, (bad, r.status_code, r.text)
        for route, b in (("/synthesize", body), ("/synthesize_stream", body), ("/synthesize_stream_marks", body),
                         ("/synthesize_stream_marks", dict(body, formants_stream=True)), ("/synthesize", {"text": "x", "ident": "m", "formants_track": True})):
            r = c.post(route, json=b)
            assert r.status_code == 400 and "formants" in r.text and "/synthesize_marks" in r.text, (route, r.status_code, r.text)


# ---- the kernels on a table ---------------------------------------------------------------------------------------------------------------------
LENGTHS = (1, 2, 63, 64, 65, 129)
TABLES = [(T, K, LENGTHS, (1, 2, 1), (1.0, 0.5, 2.0)) for T, K in ((1, 1), (1, 7), (3, 7), (4, 7), (5, 5), (5, 7))]
TABLES += [(3, 7, (), (40, 0, 0), USUAL), (2, 3, (1, 2) * 600, (1, 1, 2), USUAL), (3, 6, (200,), (0, 0, 0), USUAL)]
IDS = [f"T{T}K{K}" for T, K in ((1, 1), (1, 7), (3, 7), (4, 7), (5, 5), (5, 7))] + ["all-cut", "1200-runs", "one-run"]


@gpu
@pytest.mark.parametrize("T,K,runs,cuts,costs", TABLES, ids=IDS)
def test_path_on_a_table(T, K, runs, cuts, costs):
    cf, cb = table(T, K, runs, 7 * T + K, cuts)
    assert len(runs) <= 1 or ((cf[0] > 0).sum() < T and (cf[-1] > 0).sum() < T)  # cuts at both ends
    want = track_ref(cf, cb, T, REFS, *costs)
    got, _, _, state = model.debug_formant_track(None, 16000, FC(160, T), FT(REFS[:T], K, *costs), cand=(cf, cb))
    assert np.array_equal(state, want[2]) and got.f_hz.tobytes() == want[0].tobytes() and got.bw_hz.tobytes() == want[1].tobytes()
    assert (state >= 0).sum() == sum(runs)


@gpu
@pytest.mark.parametrize("T,K,nf", [(3, 7, 131), (4, 7, 70), (1, 1, 65)])
def test_every_minimum_ties(T, K, nf):
    """An all-equal table, all three costs 0: the smallest j wins every back-pointer and the smallest k the last frame."""
    cf, cb = np.full((nf, K), 500.0), np.full((nf, K), 80.0)
    want = track_ref(cf, cb, T, REFS, 0.0, 0.0, 0.0)
    got, _, _, state = model.debug_formant_track(None, 16000, FC(160, T), FT(REFS[:T], K, 0.0, 0.0, 0.0), cand=(cf, cb))
    assert not want[2].any() and np.array_equal(state, want[2]) and got.f_hz.tobytes() == want[0].tobytes()


@gpu
def test_a_bad_table_is_refused():
    cf, cb = table(3, 6, (5,), 1, (0, 0, 0))
    for f, b, what in ((-cf, cb, "F"), (cf[:, ::-1], cb, "ascending"), (cf, -cb - 1, "B"), (cf * 100, cb, "F")):
        with pytest.raises(model.Sbv2Error, match=what):
            model.debug_formant_track(None, 16000, FC(160, 3), FT(REFS[:3], 6), cand=(np.ascontiguousarray(f), b))


# ---- the hook on samples, the pipeline -------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dtype", [np.float32, np.int16], ids=["f32", "s16"])
def test_hook_on_samples(dtype):
    """The vowel with bursts of a 250 Hz tone and a stretch of digital silence (cuts), and a T = 5 of 6 track that some frames cannot fill."""
    sr, u = 16000, vowel(16000).astype(np.float64).copy()
    gate = np.zeros(u.size)
    for a, b in ((9, 13), (20, 23), (28, 33)):
        gate[a * 160:b * 160] = 1.0
    u += 0.4 * np.sin(2 * np.pi * 250.0 * np.arange(u.size) / sr) * gate
    u[2400:3400] = 0.0
    x = u.astype(np.float32) if dtype is np.float32 else np.clip(np.rint(u * 20000.0), -32768, 32767).astype(np.int16)
    for T, K, f_hi in ((3, 6, None), (5, 6, 4300.0)):
        got, cf, cb, state = model.debug_formant_track(x, sr, FC(160, T, f_hi=f_hi), FT(REFS[:T], K, *USUAL))
        want = track_ref(cf, cb, T, REFS, *USUAL)
        assert np.array_equal(state, want[2]) and got.f_hz.tobytes() == want[0].tobytes() and got.bw_hz.tobytes() == want[1].tobytes()
        plain, _ = model.debug_formant_contour(x, sr, FC(160, T, f_hi=f_hi))
        wide, _ = model.debug_formant_contour(x, sr, FC(160, K, f_hi=f_hi))
        cut = state < 0
        assert cut.any() and not cut.all() and got.f_hz[cut].tobytes() == plain.f_hz[cut].tobytes() and got.bw_hz[cut].tobytes() == plain.bw_hz[cut].tobytes()
        assert cf.tobytes() == wide.f_hz.tobytes() and cb.tobytes() == wide.bw_hz.tobytes() and got.status.tobytes() == plain.status.tobytes()


@gpu
@pytest.mark.parametrize("encoding,rate", [("f32", 44100), ("s16", 16000)], ids=["f32-44k", "s16-16k"])
def test_pipeline_track(request_rows, encoding, rate):
    pipe, b, rows, place, joined = request_rows
    fmt, hop, ft = model.PcmFormat(rate, encoding), rate // 100, FT(REFS[:3], 6, *USUAL)
    kw = dict(gain=model.Loudness(-23.0, -1.0), marks=True, env_hop=hop, pitch=model.Pitch(hop))
    plain, pstats, pm, pp, pfc = pipe.fetch_request(b, rows, fmt, place, joined, formants=FC(hop, 3), **kw)
    plain, pf0, pF, pst = plain.copy(), pp.f0.copy(), pfc.f_hz.copy(), pfc.status.copy()
    out, stats, m, p, fc = pipe.fetch_request(b, rows, fmt, place, joined, formants=FC(hop, 3), formant_track=ft, **kw)
    assert out.tobytes() == plain.tobytes() and stats.tobytes() == pstats.tobytes() and p.f0.tobytes() == pf0.tobytes() and fc.status.tobytes() == pst.tobytes()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(pm.arrays(), m.arrays()))
    hook, _, _, state = model.debug_formant_track(out, rate, FC(hop, 3), ft)
    assert (state >= 0).any() and hook.f_hz.tobytes() == fc.f_hz.tobytes() and hook.bw_hz.tobytes() == fc.bw_hz.tobytes()
    _, _, fc2 = pipe.fetch_request(b, rows, fmt, place, joined, gain=kw["gain"], formants=FC(hop, 3), formant_track=ft)
    assert (fc2.f_hz.tobytes(), fc2.bw_hz.tobytes()) == (fc.f_hz.tobytes(), fc.bw_hz.tobytes())
    _, _, fc3 = pipe.fetch_request(b, rows, fmt, place, joined, gain=kw["gain"], formants=FC(hop, 3))   # no track: the old call's contour
    assert fc3.f_hz.tobytes() == pF.tobytes()
    for bad, what in ((dict(formants=FC(hop, 4), formant_track=ft), "n_tracks"), (dict(formants=FC(hop, 3, order=10), formant_track=ft), "candidates"),
                      (dict(formants=FC(hop, 3), formant_track=FT(REFS[:3], 6, 17.0)), "freq_cost")):
        with pytest.raises(model.Sbv2Error, match=what):
            pipe.fetch_request(b, rows, fmt, place, joined, gain=kw["gain"], **bad)
    req = _lib.Sbv2FetchRequest(None, 0, None, 0, C.pointer(fmt.c), None, None, 0)   # a track without a contour, through the C ABI
    cft, dst, got = ft.c, np.zeros(16, np.uint8), C.c_int64(0)
    assert _lib.lib().sbv2_pipeline_fetch_request_formant_track(pipe.h, b.ticket, C.byref(req), *[None] * 5, dst.ctypes.data_as(C.c_void_p), 16, C.byref(got),
                                                                 *[None] * 6, C.byref(cft)) == 1
    assert b"needs a formant contour" in _lib.lib().sbv2_last_error()
