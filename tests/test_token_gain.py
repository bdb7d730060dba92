"""Per-token volume targets (sbv2_token_gain, csrc/token_gain.hip): a numpy float64 restatement of the definition in include/sbv2_hip.h, with the
stated summation order, and the device against it bit for bit: the kernels through sbv2_debug_token_gain at the smallest shapes at which
they can go wrong, then the loop through the pipeline on the tiny models.  The CPU tests hold the restatement to the definition's promises
and the options / REST contract to its refusals."""
import numpy as np
import pytest

import flac_reader as R
from sbv2_api_amd import _lib, batcher, model, orchestrator
from test_voice import FakePipe, REQUEST, STYLES, VOICE, _join, _payload, five_rows  # noqa: F401

gpu = pytest.mark.gpu
HOP, TILE = 512, 2048   # the model's hop; TokenGain::kTile (checked against the library in the GPU test)
N_TOKENS = sum(len(s["phones"]) for s in REQUEST if s)


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------------------

def span_sumsq(x):
    """S_t in the stated order: lane-strided partial sums in ascending order, a tree over each 64, the groups in ascending order."""
    stride = 64 if x.size <= 4096 else 256
    sq = np.zeros(-(-x.size // stride) * stride if x.size else stride, np.float64)   # (adding 0.0 changes no bit of a non-negative sum)
    sq[:x.size] = x.astype(np.float64) * x.astype(np.float64)
    part = np.zeros(stride, np.float64)
    for row in sq.reshape(-1, stride):
        part = part + row
    g = part.reshape(-1, 64).copy()
    for d in (32, 16, 8, 4, 2, 1):
        g[:, :d] = g[:, :d] + g[:, d:2 * d]
    s = g[0, 0]
    for w in range(1, g.shape[0]):
        s = s + g[w, 0]
    return s


def restate(rows, ends, values, kind, ramp, max_ratio):
    """(edited rows, applied, src_rms, ramp spans per row) by the definition above sbv2_token_gain."""
    out, applied, rms, spans, k = [], [], [], [], 0
    lo, hi = np.float64(1.0) / np.float64(max_ratio), np.float64(max_ratio)
    for x, E in zip(rows, ends):
        E = np.asarray(E, np.int64)
        st = np.concatenate([[0], E[:-1]]).astype(np.int64)
        g = np.ones(E.size, np.float64)
        for t in range(E.size):
            n, v = int(E[t] - st[t]), np.float64(values[k + t])
            M = span_sumsq(x[st[t]:E[t]]) / np.float64(n) if n else np.float64(0.0)
            r = np.sqrt(M)
            if v != 0 and n > 0 and M != 0:
                g[t] = v if kind == 0 else v / r
            g[t] = min(max(g[t], lo), hi)
            rms.append(r)
        gain = np.ones(x.size, np.float64)
        for t in range(E.size):
            gain[st[t]:E[t]] = g[t]
        if E.size:
            gain[E[-1]:] = g[-1]
        sp = []
        for t in range(E.size - 1):
            b, Rb = int(E[t]), int(min(ramp, E[t] - st[t], E[t + 1] - E[t])) & ~1
            if Rb:
                n = np.arange(b - Rb // 2, b + Rb // 2)
                u = (2 * (n - b) + Rb + 1).astype(np.float64) / np.float64(2 * Rb)
                gain[n] = g[t] + (g[t + 1] - g[t]) * ((u * u) * (3.0 - 2.0 * u))
                sp.append((b - Rb // 2, b + Rb // 2))
        out.append((x.astype(np.float64) * gain).astype(np.float32))
        applied += list(g)
        spans.append(sp)
        k += E.size
    return out, np.array(applied), np.array(rms), spans


def noise(n, seed):
    return np.random.default_rng(seed).uniform(-0.5, 0.5, n).astype(np.float32)   # (RMS 0.29)


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------------------------

def test_symbols_are_declared():
    assert {"sbv2_pipeline_fetch_request_token_gain", "sbv2_debug_token_gain", "sbv2_token_gain_tile"} <= set(_lib.SYMBOLS)
    assert model._fetch_fields(token_gain=True)[-1] == "token_gain"


def test_the_restatement_keeps_the_definitions_promises():
    x, E = noise(8 * HOP, 1), np.array([1, 3, 4, 8]) * HOP
    target = np.array([0.05, 0.0, 0.2, 1e-6])
    (y,), applied, rms, (spans,) = restate([x], [E], target, 1, 300, 8.0)
    # kind 1 lands a token's interior (the token outside its ramps) on the target.  y is f32: every sample carries a relative error <= 2^-24,
    # so the interior's RMS, a root of a sum of squares, is off by at most 2^-24 relative, plus the f64 roundings of n additions (n 2^-53)
    st = np.concatenate([[0], E[:-1]])
    for t in (0, 2):
        a, b = st[t] + (150 if t else 0), E[t] - 150
        got = np.sqrt(np.mean(y[a:b].astype(np.float64) ** 2)) / (np.sqrt(np.mean(x[a:b].astype(np.float64) ** 2)) * applied[t])
        assert abs(got - 1.0) <= 2.0 ** -24 + (b - a) * 2.0 ** -53, (t, got)
        assert abs(applied[t] * rms[t] / target[t] - 1.0) <= 2.0 ** -51 and 0.125 < applied[t] < 8.0
    assert applied[1] == 1.0 and applied[3] == 0.125 and rms[3] * applied[3] > target[3]        # not edited; the clamp shows in applied
    assert restate([x], [E], [100.0, 0, 0, 0], 0, 0, 4.0)[1][0] == 4.0
    # ramps never overlap, however long the ramp: each is even, centred on its boundary and inside its two tokens
    for ramp in (300, HOP, 10 ** 6):
        (sp,) = restate([x], [E], target, 1, ramp, 4.0)[3]
        assert len(sp) == 3 and all(a1 <= b0 for (_, a1), (b0, _) in zip(sp, sp[1:])) and all((b - a) % 2 == 0 and b - a <= ramp for a, b in sp)
    assert restate([x], [E], target, 1, 10 ** 6, 4.0)[3][0] == [(256, 768), (1280, 1792), (1792, 2304)]
    # the identity: zeros, or ratios of 1, leave every bit
    for v, k in ((np.zeros(4), 1), (np.ones(4), 0)):
        assert restate([x], [E], v, k, 300, 4.0)[0][0].tobytes() == x.tobytes()


class GainPipe(FakePipe):
    """FakePipe whose fetch_request knows token_gain: the samples are multiplied by the largest ratio (so the bytes tell the table)."""

    def fetch_request(self, b, rows, fmt, place, joined_len, gain=None, flac=False, marks=False, env_hop=0, levels=True, pitch=None, voice=None,
                      track=None, token_gain=None):
        self.calls.append(dict(rows=list(rows), marks=marks, token_gain=None if token_gain is None else (
            [round(float(v), 6) for v in token_gain.values], token_gain.kind, token_gain.ramp, round(token_gain.max_ratio, 6))))
        res = self._fetch(b, rows, fmt, place, joined_len, marks, voice)
        if token_gain is None:
            return res
        token_gain.applied, token_gain.src_rms = np.where(token_gain.values == 0, 1.0, 2.0), np.r_[0.0, np.full(token_gain.values.size - 1, 0.1)]
        return (res[0] * np.float32(token_gain.values.max()),) + tuple(res[1:]) + (token_gain,)


def test_routes_carry_or_refuse_the_table():
    SO, pipe = orchestrator.SynthesizeOptions, GainPipe()
    db = [0.0, 20.0, 0, 0, 0, 0, -20.0, 0]
    plain = orchestrator.easy_synthesize(pipe, REQUEST, STYLES, noise_seed=1)
    assert orchestrator.easy_synthesize(pipe, REQUEST, STYLES, noise_seed=1, options=SO(token_gain=[0.0] * N_TOKENS)) == plain
    assert orchestrator.easy_synthesize(pipe, REQUEST, STYLES, noise_seed=1, options=SO(token_gain=[None] * N_TOKENS, token_gain_kind="rms_db")) == plain
    assert pipe.calls[-1] == dict(plain=True)                                   # zeros and nulls: the plain fetch there always was
    wav, mk = orchestrator.easy_synthesize_marks(pipe, REQUEST, STYLES, noise_seed=1, options=SO(token_gain=db, token_gain_ramp_ms=5, token_gain_max_db=20))
    assert pipe.calls[-1] == dict(rows=[0, 1], marks=True, token_gain=([0, 10.0, 0, 0, 0, 0, 0.1, 0], "ratio", 220, 10.0))   # dB -> ratios here
    assert (_payload(wav) == np.float32(10.0) * _payload(plain)).all()
    assert mk["volume_edit"]["applied_db"][1] == pytest.approx(6.0206, abs=1e-4) and mk["volume_edit"]["src_rms_db"][:2] == [None, pytest.approx(-20.0)]
    orchestrator.easy_synthesize(pipe, REQUEST, STYLES, noise_seed=1, options=SO(token_gain=[-20.0] + [None] * 7, token_gain_kind="rms_db"))
    assert pipe.calls[-1]["token_gain"] == ([0.1] + [0] * 7, "rms", 441, round(10 ** 0.6, 6))
    runs = pipe.runs
    for bad in (db[:-1], db + [0.0]):                                           # another length: the expected count, before any run
        with pytest.raises(orchestrator.TokenGainError, match=f"expected {N_TOKENS}"):
            orchestrator.easy_synthesize(pipe, REQUEST, STYLES, noise_seed=1, options=SO(token_gain=bad))
    assert pipe.runs == runs
    for kw in (dict(token_gain=[61.0]), dict(token_gain=[float("nan")]), dict(token_gain=[1.0], token_gain_kind="rms_db"), dict(token_gain_kind="x"),
               dict(token_gain_ramp_ms=-1), dict(token_gain_max_db=float("nan")), dict(token_gain=[None])):
        with pytest.raises(orchestrator.TokenGainError, match="token_gain"):
            SO(**kw)
    with pytest.raises(orchestrator.TokenGainError, match="/synthesize_marks"):  # streams refuse, edited or not
        orchestrator.easy_synthesize_stream(None, None, REQUEST[:1], STYLES, options=SO(token_gain=[0.0] * 5))
    with pytest.raises(model.Sbv2Error, match="not served unedited"):           # a pipeline without the entry point is refused
        orchestrator.easy_synthesize(FakePipe(), REQUEST, STYLES, noise_seed=1, options=SO(token_gain=db))
    rb = batcher.RequestBatcher(pipe, start=False, clock=lambda: 0.0, max_wait_ms=1000.0)   # the batcher: per request
    f0, f1 = rb.submit(REQUEST, STYLES, options=SO(token_gain=db), noise_seed=1), rb.submit(REQUEST, STYLES, noise_seed=1)
    rb.start()
    rb.close()
    assert (_payload(f0.result(0)) == np.float32(10.0) * _payload(plain)).all() and f1.result(0) == plain


def test_rest_answers_400_with_the_count_and_on_the_stream_routes():
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient
    from sbv2_api_amd import rest
    wav = orchestrator.array_to_wav(np.zeros((1, 1, 10), np.float32))

    class H:
        seen = None

        def easy_synthesize(self, ident, text, style_id, speaker_id, options):
            if len(options.token_gain) != 3:
                raise orchestrator.TokenGainError("token_gain holds 2 values but the text has 3 tokens: expected 3")
            H.seen = (options.token_gain, options.token_gain_kind, options.token_gain_ramp_ms, options.token_gain_max_db)
            return wav

        def easy_synthesize_marks(self, *a):
            return self.easy_synthesize(*a), {"sample_rate": 44100, "tokens": [], "words": []}

    c = TestClient(rest.make_app(H()), raise_server_exceptions=False)
    body = {"text": "x", "ident": "m", "token_gain": [0, -18, None], "token_gain_kind": "rms_db", "token_gain_max_db": 9}
    assert c.post("/synthesize", json=body).content == wav and H.seen == ([0.0, -18.0, None], "rms_db", 10, 9)
    assert c.post("/synthesize_marks", json=body).status_code == 200
    for route in ("/synthesize", "/synthesize_marks"):
        assert "expected 3" in c.post(route, json=dict(body, token_gain=[0, -18])).text
        for extra in ({"token_gain": [0, 3.0, 0]}, {"token_gain_kind": "ratio"}, {"token_gain_ramp_ms": 2000}):
            r = c.post(route, json=dict(body, **extra))
            assert r.status_code == 400 and "token_gain" in r.text, (route, extra, r.text)
    for route in ("/synthesize_stream", "/synthesize_stream_marks"):
        r = c.post(route, json={"text": "x", "ident": "m", "token_gain": [0, 0, 0]})
        assert r.status_code == 400 and "/synthesize_marks" in r.text, (route, r.text)


# ---- GPU: the kernels through the hook ------------------------------------------------------------------------------------------------------------

# name -> (row lengths, token ends per row, values, kind, ramp, max_ratio, samples zeroed per row)
H_, T_ = HOP, TILE
SHAPES = {
    # a token of one hop between longer ones, and a ramp longer than it
    "one_hop_long_ramp": ([8 * H_], [[3 * H_, 4 * H_, 8 * H_]], [2.0, 0.5, 1.5], 0, 3000, 4.0, None),
    # boundaries exactly on a tile edge, one hop before and one hop behind it; three tiles
    "tile_edges": ([3 * T_], [[T_ - H_, T_, T_ + H_, 2 * T_, 3 * T_]], [0.5, 2.0, 0.7, 1.9, 0.6], 0, 400, 4.0, None),
    # packed offsets 1027 and 6030: no multiple of 4 floats; ends off the hop grid; a ramp over a tile edge; a row shorter than a group
    "unaligned_rows": ([1027, 5003, 3], [[500, 1027], [13, T_ - 3, T_ + 40, 5003], [3]], [0.5, 2.0, 3.0, 0.4, 1.7, 0.9, 2.0], 0, 64, 4.0, None),
    # a row of a single token; an empty row with and without tokens; a row with samples and no token; value 0 between two edited tokens
    "single_empty_zero": ([T_ + 8, 0, 0, 700, 4 * H_], [[T_ + 8], [], [0, 0], [], [H_, 3 * H_, 4 * H_]], [0.5, 2.0, 2.0, 2.0, 0.0, 0.5], 0, 200, 4.0, None),
    # kind 1: targets inside the clamp, at each clamp, a zero-energy token, an untouched one; a span above 4096 samples (one workgroup)
    "rms_targets": ([22 * H_], [[2 * H_, 3 * H_, 5 * H_, 6 * H_, 8 * H_, 22 * H_]], [0.1, 1e-9, 2.0, 0.2, 0.0, 0.1], 1, 441, 4.0, (5 * H_, 6 * H_)),
    # more zero-duration tokens than a tile stages: the table is read in HBM
    "many_empty_tokens": ([3 * T_], [[H_] + [2 * H_] * 20 + [T_ + 100, 3 * T_]], [2.0] + [3.0] * 20 + [0.5, 1.5], 0, 300, 4.0, None),
}


@pytest.fixture(scope="module")
def hooked():
    """Every shape once through the hook and once through the restatement."""
    assert model.token_gain_tile() == TILE
    out = {}
    for i, (name, (lens, ends, values, kind, ramp, mx, zero)) in enumerate(SHAPES.items()):
        rows = [noise(n, 10 * i + k) for k, n in enumerate(lens)]
        if zero:
            rows[0][zero[0]:zero[1]] = 0.0
        got, tg = model.debug_token_gain(rows, ends, model.TokenGain(values, ("ratio", "rms")[kind], ramp, mx))
        out[name] = (rows, got, tg, restate(rows, ends, values, kind, ramp, mx))
    return out


@gpu
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_hook_equals_the_restatement_bit_for_bit(hooked, name):
    rows, got, tg, (want, applied, rms, _) = hooked[name]
    assert tg.applied.tobytes() == applied.tobytes() and tg.src_rms.tobytes() == rms.tobytes(), (tg.applied, applied, tg.src_rms, rms)
    for k, (g, w) in enumerate(zip(got, want)):
        bad = np.flatnonzero(g.view(np.uint32) != w.view(np.uint32))
        assert bad.size == 0, (name, k, bad[:8], g[bad[:4]], w[bad[:4]])
    if name == "rms_targets":
        assert list(tg.applied[[1, 3, 4]]) == [0.25, 1.0, 1.0] and tg.applied[2] == 4.0 and tg.src_rms[3] == 0.0   # both clamps, silence, value 0
    assert any(g.tobytes() != x.tobytes() for g, x in zip(got, rows))


# ---- GPU: the loop through the pipeline -----------------------------------------------------------------------------------------------------------

@gpu
def test_pipeline_token_gain_is_the_formatter_on_the_restatements_rows(five_rows):
    c = five_rows
    pipe, b, rows, place, joined = c.pipe, c.b, c.rows, c.place, c.joined
    f0 = model.PcmFormat()
    _, _, m0 = pipe.fetch_request(b, rows, f0, place, joined, marks=True, levels=False)
    at = np.concatenate([[0], np.cumsum([int(b.t_lens[r]) for r in rows])])
    ends = [m0.end[at[k]:at[k + 1]] - place[k] for k in range(len(rows))]
    nt = int(at[-1])
    values = np.where(np.arange(nt) % 3 == 1, 0.0, 0.02 * (1 + np.arange(nt) % 5))
    tg = lambda v=values, kind="rms": model.TokenGain(v, kind, 441, 8.0)
    formats = [f0, model.PcmFormat(16000, "s16"), model.PcmFormat(8000, "mulaw")]
    for f in formats:                                                           # the identity: the fetch without, byte for byte
        plain = pipe.fetch_request(b, rows, f, place, joined)[0].copy()
        for ident in (tg(np.zeros(nt)), tg(np.ones(nt), "ratio")):
            z, _, t = pipe.fetch_request(b, rows, f, place, joined, token_gain=ident)
            assert z.tobytes() == plain.tobytes() and (t.applied == 1.0).all() and (t.src_rms == 0.0).all()
    fl = pipe.fetch_request(b, rows, formats[1], place, joined, flac=True)[0]
    assert pipe.fetch_request(b, rows, formats[1], place, joined, flac=True, token_gain=tg(np.zeros(nt)))[0] == fl
    for voice, src in ((None, {r: c.native[r] for r in rows}), (model.Voice(*VOICE), c.shifted)):   # the shifter off and on
        kw = dict(voice=voice) if voice else {}
        want, applied, rms, _ = restate([src[r] for r in rows], ends, values, 1, 441, 8.0)
        want = dict(zip(rows, want))
        got, _, mk, t = pipe.fetch_request(b, rows, f0, place, joined, marks=True, levels=False, token_gain=tg(), **kw)
        assert got.tobytes() == _join(want, rows, place, joined).tobytes() and got.tobytes() != _join(src, rows, place, joined).tobytes()
        assert t.applied.tobytes() == applied.tobytes() and t.src_rms.tobytes() == rms.tobytes()
        assert mk.start.tobytes() == m0.start.tobytes() and mk.end.tobytes() == m0.end.tobytes() and got.size == joined   # spans and lengths
        x = np.concatenate([want[r] for r in rows])
        pieces = [(0, place[0], len(want[rows[0]])), (len(want[rows[0]]), place[1], len(want[rows[1]]))]
        for f in formats[1:]:                                                   # the formatter applied to the restatement's rows
            ref = model.debug_pcm_format(x, pieces, [(0, model.pcm_format_length(f, joined), 0, 2)], f)[0]
            assert pipe.fetch_request(b, rows, f, place, joined, token_gain=tg(), **kw)[0].tobytes() == ref.tobytes()
        d = R.read(pipe.fetch_request(b, rows, formats[1], place, joined, flac=True, token_gain=tg(), **kw)[0])
        ref = model.debug_pcm_format(x, pieces, [(0, model.pcm_format_length(formats[1], joined), 0, 2)], formats[1])[0]
        assert np.asarray(d["samples"], np.int16).tobytes() == ref.tobytes()
    with pytest.raises(model.Sbv2Error, match=rf"n_tokens is {nt - 1} .* {nt} tokens"):   # the count, both numbers; nothing is written
        pipe.fetch_request(b, rows, f0, place, joined, token_gain=tg(values[:-1]))
    for bad in (tg(-values), model.TokenGain(values, "rms", -1, 8.0), model.TokenGain(values, "rms", 441, 0.5), tg(values * np.nan)):
        with pytest.raises(model.Sbv2Error, match="sbv2_token_gain"):
            pipe.fetch_request(b, rows, f0, place, joined, token_gain=bad)
    # the run's PCM was only read: the ticket fetched again without a table
    assert pipe.fetch_request(b, rows, f0, place, joined)[0].tobytes() == _join(c.native, rows, place, joined).tobytes()
    assert [x.tobytes() for x in pipe.fetch(b)] == [x.tobytes() for x in c.native]
