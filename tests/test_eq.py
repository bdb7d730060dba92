"""Parametric EQ (sbv2_eq, csrc/eq.hip): the design against what the Audio-EQ-Cookbook guarantees, the refusals of every layer, the kernels
through sbv2_debug_eq against the plain sample-by-sample cascade in numpy longdouble at the tile's and the lanes' edges, then the stage in
the pipeline on the tiny models."""
import numpy as np
import pytest

import flac_reader as R
from sbv2_api_amd import _lib, model, orchestrator
from test_voice import FakePipe, REQUEST, STYLES, _join, _payload, five_rows  # noqa: F401

gpu = pytest.mark.gpu
LD = np.longdouble
FS, Q7 = 44100, 0.5 ** 0.5
T, L = 16384, 64   # Eq::kTile and Eq::kLane (checked against the library in the GPU fixture)
BANDS = {
    "hp20": [("highpass", 20, 0, Q7)],   # poles next to 1
    "peak": [("peak", 3000, 5, 1.4)],
    "all8": [("highpass", 20, 0, Q7), ("lowshelf", 120, 6, Q7), ("peak", 300, -4, 1.0), ("peak", 1000, 3, 1.4), ("peak", 3000, 5, 2.0),
             ("peak", 6500, -9, 4.0), ("highshelf", 9000, 4, Q7), ("lowpass", 16000, 0, Q7)],
}


def gain_db(c, f):
    """20 log10 |H| of one section b0 b1 b2 a1 a2 at f Hz, in longdouble."""
    b0, b1, b2, a1, a2 = (LD(v) for v in c)
    w = 2 * np.pi * LD(f) / LD(FS)
    z1, z2 = np.exp(-1j * w.astype(np.clongdouble)), np.exp(-2j * w.astype(np.clongdouble))
    return 20 * np.log10(abs((b0 + b1 * z1 + b2 * z2) / (1 + a1 * z1 + a2 * z2)))


def cascade(coef, x, dtype):
    """The definition: x [n, columns] through the sections in order, transposed direct form II, every column from zero state."""
    y = x.astype(dtype)
    for b0, b1, b2, a1, a2 in coef.astype(dtype):
        s0, s1 = np.zeros(y.shape[1], dtype), np.zeros(y.shape[1], dtype)
        for n in range(y.shape[0]):
            v = y[n]
            w = b0 * v + s0
            s0 = b1 * v - a1 * w + s1
            s1 = b2 * v - a2 * w
            y[n] = w
    return y


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", sorted(model.Eq.KINDS))
def test_design_is_the_cookbooks(kind):
    """1e-9 dB: f64 closed forms.  The shelves are evaluated at 0 Hz and fs / 2, not at 10 Hz and 0.45 fs: there a second-order shelf is still
    1e-4 .. 1e-7 dB from its asymptote, and at z = +-1 its value is the asymptote itself."""
    for f0 in (20, 120, 1000, 9000):
        for g in ((0,) if kind in ("highpass", "lowpass") else (-24, -3, 6, 24)):
            for q in (Q7,) if kind in ("highpass", "lowpass") else (0.3, Q7, 4):
                (c,) = model.Eq([(kind, f0, g, q)]).design()
                if kind == "peak":
                    assert abs(gain_db(c, f0) - g) <= 1e-9, (f0, g, q)
                elif kind in ("highpass", "lowpass"):
                    assert abs(gain_db(c, f0) - 10 * np.log10(LD(0.5))) <= 1e-9, f0   # -3.0103 dB
                else:
                    far, near = (0, FS / 2) if kind == "lowshelf" else (FS / 2, 0)
                    assert abs(gain_db(c, far) - g) <= 1e-9 and abs(gain_db(c, near)) <= 1e-9, (f0, g, q)
    for f0 in (10, 0.45 * FS):                                                  # every pole inside the unit circle at the ranges' corners
        for g in ((0,) if kind in ("highpass", "lowpass") else (-24, 24)):
            for q in (0.1, 20):
                (c,) = model.Eq([(kind, f0, g, q)]).design()
                assert (abs(np.roots([1.0, c[3], c[4]])) < 1).all(), (f0, g, q)


BAD = {"kind": [(5, 1000, 0, 1)], "f0_hz": [("peak", 9.9, 0, 1)], "f0_hz ": [("peak", 0.46 * FS, 0, 1)], "gain_db": [("peak", 1000, 24.5, 1)],
       "gain_db ": [("highpass", 80, 1, 1)], "gain_db  ": [("lowshelf", 80, float("nan"), 1)], "q": [("peak", 1000, 0, 0.05)],
       "q ": [("peak", 1000, 0, float("nan"))], "f0_hz  ": [("lowpass", float("nan"), 0, 1)], "n_bands": [("peak", 1000, 0, 1)] * 9}


@pytest.mark.parametrize("field", sorted(BAD))
def test_library_refuses_by_name(field):
    eq = model.Eq(BAD[field][:8])
    c = eq.c_struct()
    if field == "n_bands":
        c.n_bands = 9
    rc = _lib.lib().sbv2_eq_design(c, FS, None)
    assert rc != 0 and "sbv2_eq." + field.strip() in _lib.lib().sbv2_last_error().decode()


def test_reserved_and_symbols():
    assert _lib.lib().sbv2_eq_design(model.Eq([("peak", 1000, 0, 1)]).c_struct(reserved=1), FS, None) != 0
    assert "sbv2_eq.reserved" in _lib.lib().sbv2_last_error().decode()
    counts = {"sbv2_pipeline_fetch_request_eq": 20, "sbv2_eq_design": 3, "sbv2_debug_eq": 7, "sbv2_eq_tile": 0}
    assert {k: len(_lib.SYMBOLS[k][1]) for k in counts} == counts


class EqPipe(FakePipe):
    """FakePipe whose fetch_request knows eq: the samples are halved (so the bytes tell that a table ran)."""

    def fetch_request(self, b, rows, fmt, place, joined_len, gain=None, flac=False, marks=False, env_hop=0, levels=True, pitch=None, voice=None,
                      track=None, eq=None):
        self.calls.append(dict(rows=list(rows), marks=marks, eq=None if eq is None else eq.bands))
        res = self._fetch(b, rows, fmt, place, joined_len, marks, voice)
        return res if eq is None else (res[0] * np.float32(0.5),) + tuple(res[1:])


def test_routes_carry_or_refuse_the_table():
    SO, pipe = orchestrator.SynthesizeOptions, EqPipe()
    bands = [{"kind": "highpass", "f0_hz": 80}, {"kind": "peak", "f0_hz": 3000, "gain_db": 3, "q": 1.4}]
    plain = orchestrator.easy_synthesize(pipe, REQUEST, STYLES, noise_seed=1)
    for ident in ([], [{"kind": "lowshelf", "f0_hz": 200}, {"kind": "peak", "f0_hz": 1000, "gain_db": 0.0, "q": 2}]):
        assert orchestrator.easy_synthesize(pipe, REQUEST, STYLES, noise_seed=1, options=SO(eq=ident)) == plain
        assert pipe.calls[-1] == dict(plain=True)                               # no band, 0 dB bands: the plain fetch there always was
    wav, mk = orchestrator.easy_synthesize_marks(pipe, REQUEST, STYLES, noise_seed=1, options=SO(eq=bands))
    assert pipe.calls[-1] == dict(rows=[0, 1], marks=True, eq=[(0, 80.0, 0.0, Q7), (4, 3000.0, 3.0, 1.4)])
    assert (_payload(wav) == np.float32(0.5) * _payload(plain)).all()
    assert mk["eq"] == {"bands": [dict(kind="highpass", f0_hz=80.0, gain_db=0.0, q=Q7), dict(kind="peak", f0_hz=3000.0, gain_db=3.0, q=1.4)]}
    for bad, field in (([{"kind": "notch", "f0_hz": 80}], r"eq\[0\].kind"), ([bands[0], {"kind": "peak"}], r"eq\[1\].f0_hz"),
                       ([{"kind": "peak", "f0_hz": 5}], r"eq\[0\].f0_hz"), ([{"kind": "peak", "f0_hz": 500, "gain_db": 30}], r"eq\[0\].gain_db"),
                       ([{"kind": "lowpass", "f0_hz": 500, "gain_db": 3}], r"eq\[0\].gain_db"), ([{"kind": "peak", "f0_hz": 500, "q": float("nan")}], r"eq\[0\].q"),
                       ([{"kind": "peak", "f0_hz": 500, "slope": 1}], "slope"), ([bands[0]] * 9, "at most 8"), ("highpass", "list of bands")):
        with pytest.raises(orchestrator.EqError, match=field):
            SO(eq=bad)
    with pytest.raises(orchestrator.EqError, match="/synthesize"):              # streams refuse, filtering or not
        orchestrator.easy_synthesize_stream(None, None, REQUEST[:1], STYLES, options=SO(eq=[]))
    with pytest.raises(model.Sbv2Error, match="not served unfiltered"):         # a pipeline without the keyword is refused
        orchestrator.easy_synthesize(FakePipe(), REQUEST, STYLES, noise_seed=1, options=SO(eq=bands))


def test_rest_answers_400_naming_the_field_and_on_the_stream_routes():
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient
    from sbv2_api_amd import rest
    wav = orchestrator.array_to_wav(np.zeros((1, 1, 10), np.float32))

    class H:
        seen = None

        def easy_synthesize(self, ident, text, style_id, speaker_id, options):
            H.seen = options.eq
            return wav

        def easy_synthesize_marks(self, *a):
            return self.easy_synthesize(*a), {"sample_rate": 44100, "tokens": [], "words": []}

    c = TestClient(rest.make_app(H()), raise_server_exceptions=False)
    body = {"text": "x", "ident": "m", "eq": [{"kind": "highpass", "f0_hz": 300}]}
    assert c.post("/synthesize", json=body).content == wav and H.seen == [dict(kind="highpass", f0_hz=300.0, gain_db=0.0, q=Q7)]
    assert c.post("/synthesize_marks", json=body).status_code == 200
    for route in ("/synthesize", "/synthesize_marks"):
        r = c.post(route, json=dict(body, eq=[{"kind": "peak", "f0_hz": 300, "q": 50}]))
        assert r.status_code == 400 and "eq[0].q" in r.text, (route, r.text)
    for route in ("/synthesize_stream", "/synthesize_stream_marks"):
        r = c.post(route, json=body)
        assert r.status_code == 400 and "/synthesize" in r.text and "eq" in r.text, (route, r.text)


# ---- GPU: the kernels through the hook ------------------------------------------------------------------------------------------------------------

LENS = [1, L - 1, L, L + 1, T - 1, T, T + 1, 2 * T + 777] + [5, 0, T, 100]   # ... then one group: an empty row, heads off the 16-byte grid, T exactly
SIGNALS = ("noise_dc", "impulse_0", "impulse_T-1")
R_BOUND = 4 * 7.58   # 4 times the largest ratio measured on the MI355X over these cases (profiles/eq_probe.txt; DESIGN.md, the EQ's section)


@pytest.fixture(scope="module")
def hooked():
    """Per band set: every signal's rows once through the hook (one call each), and all of them at once through both host cascades."""
    assert model.eq_tile() == T and T // 256 == L
    rng = np.random.default_rng(7)
    x = np.zeros((len(SIGNALS), max(LENS), len(LENS)), np.float32)
    for k, n in enumerate(LENS):
        x[0, :n, k] = rng.uniform(-0.5, 0.5, n).astype(np.float32) + np.float32(0.3)
        x[1, :min(n, 1), k] = 1.0
        x[2, T - 1:min(n, T), k] = 1.0
    cols = np.concatenate(list(x), axis=1)
    out = {}
    for name, bands in BANDS.items():
        eq = model.Eq(bands)
        got = [model.debug_eq([x[s, :n, k] for k, n in enumerate(LENS)], eq) for s in range(len(SIGNALS))]
        ref, seq = cascade(eq.design(), cols, LD), cascade(eq.design(), cols, np.float64)
        out[name] = (got, np.split(ref, len(SIGNALS), axis=1), np.split(seq, len(SIGNALS), axis=1))
    return out


@gpu
@pytest.mark.parametrize("signal", range(len(SIGNALS)), ids=SIGNALS)
@pytest.mark.parametrize("name", sorted(BANDS))
def test_hook_is_the_cascade(hooked, name, signal):
    got, ref, seq = hooked[name]
    (y, y64), ref, seq = got[signal], ref[signal], seq[signal]
    dev = host = LD(0)
    for k, n in enumerate(LENS):
        assert y[k].size == n and y[k].tobytes() == y64[k].astype(np.float32).tobytes(), (name, k)   # the cast is the only f32 operation
        if n:
            dev, host = max(dev, abs(y64[k] - ref[:n, k]).max()), max(host, abs(seq[:n, k] - ref[:n, k]).max())
    print(f"eq {name} {SIGNALS[signal]}: device {float(dev):.3e} host f64 {float(host):.3e} ratio {float(dev / host) if host else float('inf'):.2f}")
    assert dev <= R_BOUND * host, (name, SIGNALS[signal], float(dev), float(host))


# ---- GPU: the stage in the pipeline ---------------------------------------------------------------------------------------------------------------

@gpu
def test_pipeline_eq_is_the_hook_on_the_rows_the_formatter_would_read(five_rows):
    c = five_rows
    pipe, b, rows, place, joined = c.pipe, c.b, c.rows, c.place, c.joined
    f0, s16 = model.PcmFormat(), model.PcmFormat(16000, "s16")
    eq = model.Eq(BANDS["all8"])
    cut = lambda sig: {r: sig[p:p + len(c.native[r])] for r, p in zip(rows, place)}
    hook = lambda src: dict(zip(rows, model.debug_eq([src[r] for r in rows], eq, wide=False)[0]))
    plain = pipe.fetch_request(b, rows, f0, place, joined)[0].copy()
    fl = pipe.fetch_request(b, rows, s16, place, joined, flac=True)[0]
    for ident in (model.Eq(), model.Eq([("lowshelf", 200, 0, Q7), ("peak", 1000, 0, 2)])):   # the identity: the fetch without, byte for byte
        assert pipe.fetch_request(b, rows, f0, place, joined, eq=ident)[0].tobytes() == plain.tobytes()
        assert pipe.fetch_request(b, rows, s16, place, joined, flac=True, eq=ident)[0] == fl
    want = _join(hook(c.native), rows, place, joined)                           # every row the hook's, the gaps silent
    got = pipe.fetch_request(b, rows, f0, place, joined, eq=eq)[0].copy()
    assert got.tobytes() == want.tobytes() and got.tobytes() != plain.tobytes()
    nt = sum(int(b.t_lens[r]) for r in rows)
    tg = lambda: model.TokenGain(np.where(np.arange(nt) % 2, 2.0, 0.5), "ratio", 441, 4.0)
    scaled = pipe.fetch_request(b, rows, f0, place, joined, token_gain=tg())[0].copy()
    both = pipe.fetch_request(b, rows, f0, place, joined, token_gain=tg(), eq=eq)
    assert both[0].tobytes() == _join(hook(cut(scaled)), rows, place, joined).tobytes() and len(both) == 3   # behind the token gain
    m0, m1 = pipe.fetch_request(b, rows, f0, place, joined, marks=True)[2], pipe.fetch_request(b, rows, f0, place, joined, marks=True, eq=eq)[2]
    assert m1.end.tobytes() == m0.end.tobytes() and m1.sumsq.tobytes() != m0.sumsq.tobytes()   # same spans, the levels of the filtered signal
    a16, b16 = pipe.fetch_request(b, rows, s16, place, joined)[0], pipe.fetch_request(b, rows, s16, place, joined, eq=eq)[0]
    assert a16.size == b16.size and a16.tobytes() != b16.tobytes()
    assert np.asarray(R.read(pipe.fetch_request(b, rows, s16, place, joined, flac=True, eq=eq)[0])["samples"], np.int16).tobytes() == b16.tobytes()
    with pytest.raises(model.Sbv2Error, match=r"sbv2_eq.q\[1\]"):               # refused by name, nothing enqueued
        pipe.fetch_request(b, rows, f0, place, joined, eq=model.Eq([("peak", 500, 1, 1), ("peak", 500, 1, 25)]))
    # the run's PCM was only read: with and without, in either order, the same bytes each time
    assert pipe.fetch_request(b, rows, f0, place, joined)[0].tobytes() == plain.tobytes()
    assert pipe.fetch_request(b, rows, f0, place, joined, eq=eq)[0].tobytes() == got.tobytes()
    assert [x.tobytes() for x in pipe.fetch(b)] == [x.tobytes() for x in c.native]
