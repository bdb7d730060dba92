"""FLAC output (csrc/flac_encode.hip, sbv2_pipeline_fetch_flac): streams encoded on the device, read back by tests/flac_reader.py, a decoder
written from the specification.  A stream must decode bit for bit to the s16 samples fetch_format returns for the same PcmFormat.
CPU tests run anywhere; GPU tests (@pytest.mark.gpu) need an MI355X."""
import io

import numpy as np
import pytest

import flac_reader as R
from helpers import blob, make_utts, weights
from sbv2_api_amd import _lib, model, orchestrator, synth

RATES = (8000, 16000, 22050, 24000, 32000, 44100, 48000)


def bound(n):
    """42 + per frame (13-byte largest header + 1 + 2 n_f VERBATIM subframe + 2 CRC-16)."""
    return 42 + 16 * (-(-n // 4096)) + 2 * n


# ---- a bit writer for streams assembled by hand ---------------------------------------------------------------------------------------------

class BitWriter:
    def __init__(self):
        self.bits = []

    def put(self, v, n):
        self.bits.extend((v >> (n - 1 - i)) & 1 for i in range(n))

    def signed(self, v, n):
        self.put(v & ((1 << n) - 1), n)

    def rice(self, e, k):
        u = 2 * e if e >= 0 else -2 * e - 1
        self.bits.extend([0] * (u >> k) + [1])
        self.put(u & ((1 << k) - 1), k)

    def pad(self):
        while len(self.bits) % 8:
            self.bits.append(0)

    def bytes(self):
        return bytes(np.packbits(np.array(self.bits, np.uint8)))


def hand_frame(number, x, kind, coef=(), shift=0, p=0, k=3):
    """One frame of a 16 kHz stream: CONSTANT, VERBATIM, FIXED (order len(coef)) or LPC (coefficients coef, first = the sample right before
    x[i]); 2^p Rice partitions with parameter k, or k[i] for partition i."""
    n = len(x)
    ks = [k] * (1 << p) if np.isscalar(k) else list(k)
    assert len(ks) == 1 << p and n % (1 << p) == 0
    w = BitWriter()
    w.put(0xFFF8, 16)
    w.put(0b1100 if n == 4096 else 0b0110 if n <= 256 else 0b0111, 4)   # block size: 4096, or 8 / 16 bits of n - 1 after the number
    w.put(0b0101, 4)          # 16 kHz
    w.put(0b0000, 4)
    w.put(0b100, 3)
    w.put(0, 1)
    for b in chr(number).encode("utf-8"):   # the frame number, coded like a code point
        w.put(b, 8)
    if n != 4096:
        w.put(n - 1, 8 if n <= 256 else 16)
    w.put(R.crc8(w.bytes()), 8)
    order = len(coef)
    w.put(0, 1)
    if kind == "CONSTANT":
        w.put(0, 6)
    elif kind == "VERBATIM":
        w.put(1, 6)
    elif kind == "FIXED":
        w.put(8 + order, 6)
    else:
        w.put(31 + order, 6)
    w.put(0, 1)
    if kind == "CONSTANT":
        w.signed(int(x[0]), 16)
    elif kind == "VERBATIM":
        for v in x:
            w.signed(int(v), 16)
    else:
        for v in x[:order]:
            w.signed(int(v), 16)
        if kind == "LPC":
            w.put(15 - 1, 4)
            w.signed(shift, 5)
            for c in coef:
                w.signed(c, 15)
        w.put(0, 2)
        w.put(p, 4)
        P = n >> p
        for i in range(order, n):
            if i % P == 0 or i == order:
                w.put(ks[i // P], 4)
            acc = sum(c * int(x[i - 1 - j]) for j, c in enumerate(coef))
            w.rice(int(x[i]) - (acc >> shift), ks[i // P])
    w.pad()
    b = w.bytes()
    return b + R.crc16(b).to_bytes(2, "big")


def stream_info(total, frames, rate=16000):
    si = (4096).to_bytes(2, "big") * 2
    si += min(len(f) for f in frames).to_bytes(3, "big") + max(len(f) for f in frames).to_bytes(3, "big")
    si += ((rate << 44) | (15 << 36) | total).to_bytes(8, "big") + bytes(16)
    return b"fLaC" + bytes([0x80, 0, 0, 34]) + si


# ---- CPU ----------------------------------------------------------------------------------------------------------------------------------

def test_reader_crc_check_values():
    assert R.crc8(b"123456789") == 0xF4
    assert R.crc16(b"123456789") == 0xFEE8


def test_reader_decodes_hand_built_stream_and_pins_coefficient_order():
    rng = np.random.default_rng(5)
    a = rng.integers(-3000, 3000, 40)
    b = np.cumsum(rng.integers(-20, 20, 50)).astype(np.int64) + 100
    # an LPC-2 signal: c = [3, -1] / 2, the 3 multiplying x[i - 1]; with the order swapped the decode would differ
    c = [int(v) for v in rng.integers(-50, 50, 2)]
    for i in range(2, 60):
        c.append(((3 * c[i - 1] - c[i - 2]) >> 1) + int(rng.integers(-4, 5)))
    c = np.asarray(c)
    frames = [hand_frame(0, a, "VERBATIM"), hand_frame(1, b, "FIXED", (2, -1)), hand_frame(2, c, "LPC", (3, -1), shift=1)]
    data = stream_info(150, frames) + b"".join(frames)
    got = R.read(data)
    np.testing.assert_array_equal(got["samples"], np.concatenate([a, b, c]).astype(np.int16))
    assert [f["type"] for f in got["frames"]] == ["VERBATIM", "FIXED", "LPC"]
    assert got["frames"][2]["coef"] == [3, -1] and got["frames"][2]["shift"] == 1
    assert (got["rate"], got["total"], got["min_frame"], got["max_frame"]) == (16000, 150, min(map(len, frames)), max(map(len, frames)))
    # a flipped bit is caught by a CRC
    bad = bytearray(data)
    bad[-5] ^= 0x10
    with pytest.raises(R.FlacError, match="CRC"):
        R.read(bytes(bad))


def test_flac_bound_values_and_refusals():
    for r in RATES:
        f = model.PcmFormat(r, "s16")
        for n in (0, 1, 4095, 4096, 4097, 44100, 10 ** 6):
            m = model.pcm_format_length(f, n)
            assert model.flac_bound(f, n) == bound(m), (r, n)
    assert model.flac_bound(model.PcmFormat(44100, "s16"), 0) == 42
    l = _lib.lib()
    assert l.sbv2_flac_bound(_lib.Sbv2PcmFormat(44100, 0, 0, 0), 100) == -1
    assert b"s16" in l.sbv2_last_error()
    assert l.sbv2_flac_bound(_lib.Sbv2PcmFormat(11025, 1, 0, 0), 100) == -1
    assert b"sample rate" in l.sbv2_last_error()
    assert l.sbv2_flac_bound(_lib.Sbv2PcmFormat(16000, 2, 0, 0), 100) == -1
    with pytest.raises(model.Sbv2Error, match="s16"):
        model.flac_bound(model.PcmFormat(16000, "f32"), 10)


def test_rest_flac_encoding_reaches_holder_and_sets_media_type():
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient
    from sbv2_api_amd import rest

    class Holder:
        def __init__(self):
            self.opts = []

        def models(self):
            return ["m"]

        def easy_synthesize(self, ident, text, style_id, speaker_id, options):
            self.opts.append(options)
            return b"fLaC" if options.encoding == "flac" else b"RIFF"

    h = Holder()
    c = TestClient(rest.make_app(h))
    r = c.post("/synthesize", json={"text": "a", "ident": "m", "encoding": "flac", "sample_rate": 16000})
    assert r.status_code == 200 and r.headers["content-type"] == "audio/flac" and r.content == b"fLaC"
    assert (h.opts[-1].encoding, h.opts[-1].sample_rate) == ("flac", 16000)
    r = c.post("/synthesize", json={"text": "a", "ident": "m"})
    assert r.status_code == 200 and r.headers["content-type"] == "audio/wav"
    r = c.post("/synthesize", json={"text": "a", "ident": "m", "encoding": "s16"})
    assert r.headers["content-type"] == "audio/wav"


def test_pcm_format_keeps_its_encodings():
    with pytest.raises(model.Sbv2Error, match="encoding"):
        model.PcmFormat(16000, "flac")


# ---- the numpy restatement of the compression bar -----------------------------------------------------------------------------------------

def voiced_signal(rate, seconds=4.0, seed=2024):
    """f0 = 140 +- 20 Hz at 0.7 Hz, harmonics 1/k below 0.45 rate each with a slow tremolo, peak 0.7, Gaussian noise at -60 dBFS."""
    t = np.arange(int(seconds * rate)) / rate
    f0 = 140 + 20 * np.sin(2 * np.pi * 0.7 * t)
    ph = 2 * np.pi * np.cumsum(f0) / rate
    y = np.zeros_like(t)
    k = 1
    while k * 160 < 0.45 * rate:
        y += np.sin(k * ph) / k * (1 + 0.3 * np.sin(2 * np.pi * (0.2 + 0.05 * k) * t + k))
        k += 1
    y *= 0.7 / np.abs(y).max()
    y += np.random.default_rng(seed).standard_normal(t.size) * 10 ** (-60 / 20)
    return np.clip(np.rint(y * 32767), -32767, 32767).astype(np.int16)




def _rice_bits(e, order, n):
    """Method + partition order (6 bits) and the cheapest partitioned Rice coding of the residuals e of a block of n, over every valid p <= 8."""
    u = np.concatenate([np.zeros(order, np.int64), np.where(e >= 0, 2 * e, -2 * e - 1).astype(np.int64)])
    ks = np.arange(15, dtype=np.int64)[:, None]
    hi = u[None, :] >> ks                  # (the warm-up samples count as zeros and are taken out of partition 0's count below)
    best = None
    for p in range(9):
        if n % (1 << p) or (n >> p) <= order:
            continue
        count = np.full(1 << p, n >> p, np.int64)
        count[0] -= order
        cost = hi.reshape(15, 1 << p, n >> p).sum(2) + count[None, :] * (ks + 1)
        bits = 6 + 4 * (1 << p) + int(cost.min(0).sum())
        best = bits if best is None else min(best, bits)
    return best


def _lpc_all(x, maxorder):
    """[(quantised coefficients, shift)] for LPC orders 1, 2, ... up to maxorder from one Levinson-Durbin pass (Tukey 0.5 window, libFLAC's
    precision-15 quantiser); the pass stops, as the encoder's does, where the error or a coefficient stops being a positive / finite number."""
    import scipy.signal.windows as SW
    n = x.size
    w = SW.tukey(n, 0.5)
    xw = x * w
    R_ = np.array([np.dot(xw[l:], xw[:n - l]) for l in range(maxorder + 1)])
    a, err = np.zeros(0), R_[0]
    out = []
    for o in range(maxorder):
        if not err > 0:
            break
        k = -(R_[o + 1] + np.dot(a, R_[o:0:-1][:o])) / err
        a = np.concatenate([a + k * a[::-1], [k]])
        err *= 1 - k * k
        if not np.isfinite(a).all():
            break
        lp = -a
        cmax = np.abs(lp).max()
        shift = int(min(max(13 - np.floor(np.log2(cmax)), 0), 15)) if cmax > 0 else 0
        q, acc = [], 0.0
        for c in lp:
            acc += c * 2.0 ** shift
            v = int(min(max(np.floor(acc + 0.5) if acc >= 0 else -np.floor(-acc + 0.5), -16384), 16383))
            acc -= v
            q.append(v)
        out.append((q, shift))
    return out


def restated_frame_bytes(x, lpc_orders=(8, 12)):
    """Sum of frame sizes of the best of FIXED 0-4 and the LPC orders asked for (8 and 12, or any of 1..12; Tukey 0.5, precision 15, p <= 8)
    per 4096-sample block."""
    total = 0
    for f0 in range(0, x.size, 4096):
        b = x[f0:f0 + 4096].astype(np.int64)
        n = b.size
        cands = []
        for order, coef in R.FIXED.items():
            if order < n:
                pred = sum(c * b[order - 1 - j:n - 1 - j] for j, c in enumerate(coef)) if coef else 0
                cands.append(8 + 16 * order + _rice_bits(b[order:] - pred, order, n))
        lpc = _lpc_all(b.astype(np.float64), min(max(lpc_orders, default=0), n - 1))
        for order in lpc_orders:
            if order <= len(lpc):
                q, sh = lpc[order - 1]
                acc = sum(c * b[order - 1 - j:n - 1 - j] for j, c in enumerate(q))
                cands.append(8 + 16 * order + 9 + 15 * order + _rice_bits(b[order:] - (acc >> sh), order, n))
        cands.append(8 + 16 * n)
        hdr = 4 + len(chr(f0 // 4096).encode("utf-8")) + (0 if n == 4096 else 1 if n <= 256 else 2) + 1
        total += hdr + (min(cands) + 7) // 8 + 2
    return total


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------------

def check_stream(data, x, rate):
    got = R.read(data)
    np.testing.assert_array_equal(got["samples"], np.asarray(x, np.int16))
    assert got["rate"] == rate and got["total"] == len(x)
    assert (got["min_block"], got["max_block"]) == (4096, 4096)
    sizes = [f["size"] for f in got["frames"]]
    assert (got["min_frame"], got["max_frame"]) == ((min(sizes), max(sizes)) if sizes else (0, 0))
    assert got["md5"] == bytes(16)
    assert sum(sizes) + 42 == len(data)
    return got


@pytest.mark.gpu
def test_debug_encode_round_trips_edge_signals():
    rng = np.random.default_rng(11)
    sigs = []
    for n in (0, 1, 15, 4095, 4096, 4097, 3 * 4096 + 17):
        sigs.append(np.zeros(n, np.int16))
        sigs.append(np.full(n, -1234, np.int16))
        sigs.append(np.where((np.arange(n) // 37) % 2, 32767, -32767).astype(np.int16))
        sigs.append(rng.integers(-32768, 32768, n).astype(np.int16))
        sigs.append(np.rint(8000 * np.sin(np.arange(n) * 0.05) + rng.normal(0, 30, n)).astype(np.int16))
    out = model.debug_flac_encode(sigs, 44100)
    assert len(out) == len(sigs)
    for i, (x, data) in enumerate(zip(sigs, out)):
        got = check_stream(data, x, 44100)
        kind = i % 5
        if kind in (0, 1):   # (a block of < 7 zeros can be cheaper as FIXED 0 than as CONSTANT)
            assert all(f["type"] == "CONSTANT" and f["size"] <= 16 for f in got["frames"] if f["n"] >= 7), i
        if kind == 3:
            assert all(f["size"] <= 13 + 1 + 2 * f["n"] + 2 for f in got["frames"])
        assert len(data) <= bound(x.size)
    # several signals in one call give the streams of one call each
    for x, data in zip(sigs[::6], out[::6]):
        assert model.debug_flac_encode([x], 44100)[0] == data
    # identical bytes over two calls
    assert model.debug_flac_encode(sigs, 44100) == out


@pytest.mark.gpu
def test_debug_encode_every_rate():
    for r in RATES:
        x = voiced_signal(r, seconds=0.5)
        data = model.debug_flac_encode([x], r)[0]
        got = check_stream(data, x, r)
        assert got["frames"] and R.RATE_CODES[r] == data[42 + 2] & 0x0F


@pytest.mark.gpu
@pytest.mark.parametrize("rate,ratio_hint", [(44100, 0.55), (16000, 0.67)])
def test_compression_bar(rate, ratio_hint):
    x = voiced_signal(rate)
    data = model.debug_flac_encode([x], rate)[0]
    got = check_stream(data, x, rate)
    frames = len(data) - 42
    ref = restated_frame_bytes(x)
    print(f"\n{rate} Hz: FLAC frames {frames} B = {frames / (2 * x.size):.3f} of s16; restatement {ref} B = {ref / (2 * x.size):.3f};"
          f" LPC frames {sum(f['type'] == 'LPC' for f in got['frames'])} / {len(got['frames'])}")
    assert frames <= 1.01 * ref


def tone_signal(rate, seconds=1.0, seed=7):
    """Four steady partials up to 5.1 kHz, noise at -80 dBFS: a signal on which LPC beats every fixed predictor by far."""
    t = np.arange(int(seconds * rate)) / rate
    y = sum(a * np.sin(2 * np.pi * f * t + i) for i, (a, f) in enumerate(((0.3, 440), (0.2, 1230), (0.15, 3310), (0.1, 5120))))
    y += np.random.default_rng(seed).standard_normal(t.size) * 10 ** (-80 / 20)
    return np.clip(np.rint(y * 32767), -32767, 32767).astype(np.int16)


@pytest.mark.gpu
@pytest.mark.parametrize("rate", (44100, 16000))
def test_lpc_path_beats_fixed_on_tones(rate):
    """The restatement gives ~0.43 / 0.40 of the s16 bytes with LPC and ~0.73 / 0.93 with FIXED alone: only a working LPC path meets this."""
    x = tone_signal(rate)
    data = model.debug_flac_encode([x], rate)[0]
    got = check_stream(data, x, rate)
    frames = len(data) - 42
    fixed = restated_frame_bytes(x, lpc_orders=())
    print(f"\n{rate} Hz tones: FLAC frames {frames / (2 * x.size):.3f} of s16, FIXED-only restatement {fixed / (2 * x.size):.3f}")
    assert frames <= 1.01 * restated_frame_bytes(x)
    assert frames <= 0.75 * fixed
    assert sum(f["type"] == "LPC" for f in got["frames"]) >= len(got["frames"]) - 1


def _tiny():
    bc, _ = weights("bert", "tiny", 3)
    vc, _ = weights("vits", "tiny", 5)
    bs, vs = model.load_model(blob("bert", "tiny", 3), True), model.load_model(blob("vits", "tiny", 5), False)
    return bc, vc, bs, vs


@pytest.mark.gpu
def test_fetch_flac_equals_fetch_format_tiny():
    bc, vc, bs, vs = _tiny()
    pipe = model.Pipeline(bs, vs)
    utts = make_utts([9, 1, 23, 14, 40], bc, vc, seed0=401, with_bert=False)
    b = pipe.prepare(utts, forced=True)
    pipe.run(b)
    lens = [int(v) for v in b.lens]
    place = [5000, 0, 5000 + lens[0] + 40, 20000, 20000 + lens[3] + 3000]
    joined = place[-1] + lens[4] + 777
    for rate in (44100, 16000):
        for norm in (False, True):
            f = model.PcmFormat(rate, "s16", norm)
            ref = pipe.fetch_format(b, f)
            got = pipe.fetch_flac(b, f)
            assert len(got) == len(utts)
            for x, data in zip(ref, got):
                check_stream(data, x, rate)
            refj = pipe.fetch_format(b, f, place, joined)
            gotj = pipe.fetch_flac(b, f, place, joined)
            assert len(gotj) == 1
            check_stream(gotj[0], refj[0], rate)
            assert pipe.fetch_flac(b, f, place, joined) == gotj
    with pytest.raises(model.Sbv2Error, match="s16"):
        pipe.fetch_flac(b, model.PcmFormat(16000, "f32"))
    # f32 is refused by the C entry point too, and a short destination is refused and left untouched
    l = _lib.lib()
    f = model.PcmFormat(16000, "s16")
    need = sum(len(d) for d in pipe.fetch_flac(b, f))
    dst = np.full(need, 77, np.uint8)
    outs = np.full(len(utts), -5, np.int64)
    rc = l.sbv2_pipeline_fetch_flac(pipe.h, b.ticket, model.PcmFormat(16000, "f32").c, None, 0, dst.ctypes.data, dst.nbytes,
                                    outs.ctypes.data_as(_lib.i64p))
    assert rc != 0 and b"s16" in l.sbv2_last_error()
    rc = l.sbv2_pipeline_fetch_flac(pipe.h, b.ticket, f.c, None, 0, dst.ctypes.data, need - 1, outs.ctypes.data_as(_lib.i64p))
    assert rc != 0 and b"too small" in l.sbv2_last_error()
    assert (dst == 77).all() and (outs == -5).all()
    rc = l.sbv2_pipeline_fetch_flac(pipe.h, b.ticket, f.c, None, 0, dst.ctypes.data, need, outs.ctypes.data_as(_lib.i64p))
    assert rc == 0 and int(outs.sum()) == need
    pipe.close(); bs.close(); vs.close()


@pytest.mark.gpu
def test_easy_synthesize_flac_equals_s16_wav():
    import scipy.io.wavfile as W
    bc, vc, bs, vs = _tiny()
    pipe = model.Pipeline(bs, vs)
    keys = ("input_ids", "word2ph", "phones", "tones", "langs")
    sent = [{k: synth.make_utterance(n, bc, vc, seed=610 + n)[k] for k in keys} for n in (11, 6, 17)]
    lines = [sent[0], None, sent[1], sent[2]]
    styles = synth.hash_normal(77, 3 * vc["style_dim"]).reshape(3, -1).astype(np.float32)
    for rate, norm in ((16000, False), (44100, True)):
        wav = orchestrator.easy_synthesize(pipe, lines, styles, 1, 0, orchestrator.SynthesizeOptions(sample_rate=rate, encoding="s16",
                                                                                                      normalize=norm), noise_seed=1234)
        r, y = W.read(io.BytesIO(wav))
        assert r == rate and y.dtype == np.int16
        fl = orchestrator.easy_synthesize(pipe, lines, styles, 1, 0, orchestrator.SynthesizeOptions(sample_rate=rate, encoding="flac",
                                                                                                     normalize=norm), noise_seed=1234)
        assert fl[:4] == b"fLaC"
        check_stream(fl, y, rate)
    pipe.close(); bs.close(); vs.close()


@pytest.mark.gpu
def test_full_shape_batch_44k():
    """The bench-shaped batch (32 x 128 phonemes at full model size) at 44.1 kHz: every stream's size and STREAMINFO, three streams decoded
    in full.  Synthetic weights: the ratio printed says nothing about speech."""
    bc, _ = weights("bert", "full")
    vc, _ = weights("vits", "full")
    bs, vs = model.load_model(blob("bert", "full"), True), model.load_model(blob("vits", "full"), False)
    pipe = model.Pipeline(bs, vs)
    utts = [synth.make_utterance(128, bc, vc, seed=i) for i in range(32)]
    b = pipe.prepare(utts, forced=True)
    pipe.run(b)
    f = model.PcmFormat(44100, "s16")
    ref = pipe.fetch_format(b, f)
    got = pipe.fetch_flac(b, f)
    assert len(got) == 32
    for i, (x, data) in enumerate(zip(ref, got)):
        assert data[:4] == b"fLaC" and int.from_bytes(data[18:26], "big") & ((1 << 36) - 1) == x.size
        assert len(data) <= bound(x.size)
    for i in (0, 7, 31):
        check_stream(got[i], ref[i], 44100)
    ratio = sum(map(len, got)) / sum(2 * x.size for x in ref)
    print(f"\nfull-shape batch, 44.1 kHz: FLAC / s16 bytes = {ratio:.3f} (synthetic weights)")
    pipe.close(); bs.close(); vs.close()
