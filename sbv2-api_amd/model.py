"""Host mirror of crates/sbv2_core/src/model.rs (`load_model`, `synthesize`) and bert.rs (`predict`) over the C ABI.

Same names, argument order and meaning as the reference; numpy arrays stand in for ndarray.  The batched /
pipeline entry points are the new capabilities (the reference is strictly batch 1).
"""
import ctypes as C
import os
from collections import namedtuple

import numpy as np

from . import _lib
from ._lib import Sbv2Batch, Sbv2Error, Sbv2FetchRequest, Sbv2UttOptions, check, f32p, i64p

__all__ = ["Session", "load_model", "predict", "synthesize", "predict_batch", "synthesize_batch", "Pipeline", "Node", "Comm", "deal", "Sbv2Error",
           "PcmFormat", "pcm_format_length", "pcm_format_taps", "flac_bound", "debug_flac_encode", "flac_stream_bound", "debug_flac_stream_encode", "Loudness", "loudness_kweight",
           "debug_loudness", "Limiter", "debug_limiter"]


def _i64(a):
    a = np.ascontiguousarray(a, dtype=np.int64)
    return a, a.ctypes.data_as(i64p)


def _f32(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return a, a.ctypes.data_as(f32p)


class Session:
    """Opaque model handle; stands in for `ort::session::Session` (model.rs:6, tts.rs:32-46)."""

    def __init__(self, handle, bert):
        self.handle, self.bert = handle, bert

    def close(self):
        if self.handle:
            (_lib.lib().sbv2_bert_destroy if self.bert else _lib.lib().sbv2_vits_destroy)(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def load_model(model_file: bytes, bert: bool, device: int = 0) -> Session:
    """model.rs:6-50 `load_model(model_file, bert)`; the EP list / thread options have no meaning here."""
    l = _lib.lib()
    h = C.c_void_p()
    buf = (C.c_char * len(model_file)).from_buffer_copy(model_file) if not isinstance(model_file, (bytearray, memoryview)) else \
        (C.c_char * len(model_file)).from_buffer(model_file)
    fn = l.sbv2_bert_create if bert else l.sbv2_vits_create
    check(fn(C.cast(buf, C.c_void_p), len(model_file), device, C.byref(h)))
    return Session(h, bert)


def predict(session: Session, token_ids, attention_masks) -> np.ndarray:
    """bert.rs:6-24 `predict(session, token_ids, attention_masks) -> Array2<f32> [S, 1024]`."""
    ids, pi = _i64(token_ids)
    msk, pm = _i64(attention_masks)
    if ids.shape != msk.shape or ids.ndim != 1:
        raise Sbv2Error("token_ids and attention_masks must be 1-D and of equal length")
    l = _lib.lib()
    out = np.empty((ids.shape[0], l.sbv2_bert_hidden(session.handle)), np.float32)
    check(l.sbv2_bert_predict(session.handle, pi, pm, ids.shape[0], out.ctypes.data_as(f32p)))
    return out


def predict_batch(session: Session, token_ids_list, attention_masks_list=None):
    l = _lib.lib()
    lens = np.array([len(t) for t in token_ids_list], np.int64)
    ids, pi = _i64(np.concatenate([np.asarray(t, np.int64) for t in token_ids_list]))
    pm = None
    if attention_masks_list is not None:
        msk, pm = _i64(np.concatenate([np.asarray(t, np.int64) for t in attention_masks_list]))
    out = np.empty((int(lens.sum()), l.sbv2_bert_hidden(session.handle)), np.float32)
    check(l.sbv2_bert_predict_batch(session.handle, len(lens), pi, pm, lens.ctypes.data_as(i64p), out.ctypes.data_as(f32p)))
    return np.split(out, np.cumsum(lens)[:-1], axis=0)


def fresh_noise_seed() -> int:
    """A new 64-bit seed per call: the reference's graph draws fresh RandomNormalLike noise on every run (tts.rs:313-314 passes
    noise_scale 0.677 / noise_scale_w 0.8), so an unseeded request must not be bit-reproducible here either."""
    return int.from_bytes(os.urandom(8), "little")


def synthesize(session: Session, bert_ori, x_tst, spk_ids, tones, lang_ids, style_vector, sdp_ratio, length_scale, noise_scale,
               noise_scale_w, noise_seed: int | None = None) -> np.ndarray:
    """model.rs:53-111 `synthesize(...) -> Array3<f32> [1, 1, L]` (same argument order).  noise_seed None = fresh noise per call."""
    l = _lib.lib()
    if noise_seed is None:
        noise_seed = fresh_noise_seed()
    b, pb = _f32(bert_ori)
    x, px = _i64(x_tst)
    t, pt = _i64(tones)
    g, pg = _i64(lang_ids)
    s, ps = _f32(style_vector)
    T = x.shape[0]
    if b.shape != (l.sbv2_vits_bert_dim(session.handle), T) or t.shape != (T,) or g.shape != (T,):
        raise Sbv2Error("input shapes do not agree (bert [1024, T], x_tst / tones / lang_ids [T])")
    sid = int(np.asarray(spk_ids).reshape(-1)[0])
    pcm = f32p()
    n = C.c_int64()
    check(l.sbv2_vits_synthesize(session.handle, pb, px, pt, pg, T, sid, ps, sdp_ratio, length_scale, noise_scale, noise_scale_w,
                                 noise_seed, C.byref(pcm), C.byref(n)))
    try:
        out = np.ctypeslib.as_array(pcm, shape=(n.value,)).copy()
    finally:
        l.sbv2_pcm_free(pcm)
    return out.reshape(1, 1, -1)


ENCODINGS = {"f32": 0, "s16": 1, "mulaw": 7, "alaw": 6}   # the G.711 laws under their WAVE format tags
G711 = ("mulaw", "alaw")
_DTYPES = {"f32": np.float32, "s16": np.int16, "mulaw": np.uint8, "alaw": np.uint8}


class PcmFormat:
    """Output format of the PCM (struct sbv2_pcm_format): sample_rate in {8000, 16000, 22050, 24000, 32000, 44100, 48000}, encoding "f32",
    "s16", or G.711 "mulaw" / "alaw" (one byte per sample: the code of the s16 sample), normalize = peak of each output signal to full
    scale.  Resampling, normalisation and quantisation run on the device."""

    def __init__(self, sample_rate: int = 44100, encoding: str = "f32", normalize: bool = False):
        if encoding not in ENCODINGS:
            raise Sbv2Error(f"unsupported PCM encoding {encoding!r} (f32, s16, mulaw, alaw)")
        self.sample_rate, self.encoding, self.normalize = int(sample_rate), encoding, bool(normalize)
        self.c = _lib.Sbv2PcmFormat(self.sample_rate, ENCODINGS[encoding], int(self.normalize), 0)

    @property
    def dtype(self):
        return _DTYPES[self.encoding]

    @property
    def is_default(self) -> bool:
        return self.sample_rate == 44100 and self.encoding == "f32" and not self.normalize

    def __repr__(self):
        return f"PcmFormat({self.sample_rate}, {self.encoding!r}, normalize={self.normalize})"


def pcm_format_length(fmt: PcmFormat, n_native: int) -> int:
    """Samples of an n_native-sample 44.1 kHz signal in `fmt`: ceil(n L / M) (host only)."""
    n = _lib.lib().sbv2_pcm_format_length(C.byref(fmt.c), int(n_native))
    if n < 0:
        raise Sbv2Error(_lib.lib().sbv2_last_error().decode(errors="replace"))
    return n


def _g711_law(encoding) -> int:
    if encoding not in G711:
        raise Sbv2Error(f"unsupported G.711 encoding {encoding!r} (mulaw, alaw)")
    return ENCODINGS[encoding]


def g711_encode(q, encoding: str) -> np.ndarray:
    """The G.711 codes (uint8) of int16 samples q under "mulaw" / "alaw": the library's own rule, on the host (sbv2_g711_encode)."""
    law = _g711_law(encoding)
    q = np.ascontiguousarray(np.asarray(q, np.int16))
    out = np.empty(q.shape, np.uint8)
    check(_lib.lib().sbv2_g711_encode(law, q.ctypes.data_as(C.c_void_p), q.size, out.ctypes.data_as(C.c_void_p)))
    return out


def g711_decode(codes, encoding: str) -> np.ndarray:
    """The int16 samples that G.711 codes (uint8 array or bytes) stand for under "mulaw" / "alaw" (sbv2_g711_decode; host only)."""
    law = _g711_law(encoding)
    c = np.frombuffer(codes, np.uint8) if isinstance(codes, (bytes, bytearray, memoryview)) else np.asarray(codes, np.uint8)
    c = np.ascontiguousarray(c)
    out = np.empty(c.shape, np.int16)
    check(_lib.lib().sbv2_g711_decode(law, c.ctypes.data_as(C.c_void_p), c.size, out.ctypes.data_as(C.c_void_p)))
    return out


def debug_pcm_cast(signals, gains, encoding: str, device: int = 0, guard: int = 64):
    """Test hook: the gain-stage kernel of the output chain on host float64 signals laid back to back, signal i times gains[i], delivered in
    `encoding` -> one array per signal.  The host destination lies between two `guard`-byte bands of 0xA5, checked here; the hook checks
    the bands around its device output."""
    if encoding not in ENCODINGS:
        raise Sbv2Error(f"unsupported PCM encoding {encoding!r} (f32, s16, mulaw, alaw)")
    sigs = [np.ascontiguousarray(np.asarray(x, np.float64)).reshape(-1) for x in signals]
    x = np.concatenate(sigs) if sigs else np.zeros(0, np.float64)
    lens = np.array([s.size for s in sigs], np.int64)
    g = np.ascontiguousarray(np.asarray(gains, np.float64).reshape(-1))
    if g.size != len(sigs):
        raise Sbv2Error(f"one gain per signal ({len(sigs)})")
    dt = np.dtype(_DTYPES[encoding])
    nb = x.size * dt.itemsize
    buf = np.full(nb + 2 * guard, 0xA5, np.uint8)
    check(_lib.lib().sbv2_debug_pcm_cast(int(device), x.ctypes.data_as(C.c_void_p) if x.size else None, lens.ctypes.data_as(i64p), len(sigs),
                                         _f64p(g), ENCODINGS[encoding], buf[guard:].ctypes.data_as(C.c_void_p)))
    if not (np.all(buf[:guard] == 0xA5) and np.all(buf[guard + nb:] == 0xA5)):
        raise Sbv2Error("sbv2_debug_pcm_cast wrote outside its destination")
    out = buf[guard:guard + nb].copy().view(dt)
    return np.split(out, np.cumsum(lens)[:-1])


def debug_pcm_format(x, pieces, sigs, fmt: PcmFormat, expose_y: bool = False, peaks: bool = False, device: int = 0, guard: int = 64):
    """Test hook: the formatting launches (resampler, peak normalisation) on a table of pieces and signals.  x = native float32 samples;
    pieces = rows (offset into x, t0, len); sigs = rows (j0, j1, p0, p1): outputs [j0, j1) of the timeline that holds pieces [p0, p1).
    Returns one array per signal in fmt's encoding, or float64 with expose_y (the resampler's sum before the gain stage); with peaks also
    max |y| of every signal (fmt must normalise).  The host destination lies between two `guard`-byte bands of 0xA5, checked here."""
    x = np.ascontiguousarray(np.asarray(x, np.float32).reshape(-1))
    pc = np.ascontiguousarray(np.asarray(pieces, np.int64).reshape(-1, 3))
    sg = np.ascontiguousarray(np.asarray(sigs, np.int64).reshape(-1, 4))
    dt = np.dtype(np.float64 if expose_y else fmt.dtype)
    lens = sg[:, 1] - sg[:, 0]
    n_out = int(np.clip(lens, 0, None).sum())
    nb = n_out * dt.itemsize if n_out <= 1 << 26 else 0   # (a table with j1 < j0 or more samples than that is refused by the hook)
    buf = np.full(nb + 2 * guard, 0xA5, np.uint8)
    pk = np.full(len(sg), np.nan) if peaks else None
    rc = _lib.lib().sbv2_debug_pcm_format(int(device), x.ctypes.data_as(f32p) if x.size else None, x.size, pc.ctypes.data_as(i64p) if pc.size else None,
                                          len(pc), sg.ctypes.data_as(i64p), len(sg), C.byref(fmt.c), int(bool(expose_y)),
                                          buf[guard:].ctypes.data_as(C.c_void_p), _f64p(pk) if peaks else None)
    if not (np.all(buf[:guard] == 0xA5) and np.all(buf[guard + nb:] == 0xA5)) or (rc != 0 and not np.all(buf == 0xA5)):
        raise Sbv2Error("sbv2_debug_pcm_format wrote outside its destination, or wrote although it failed")
    check(rc)
    out = np.split(buf[guard:guard + nb].copy().view(dt), np.cumsum(lens)[:-1])
    return (out, pk) if peaks else out


def pcm_format_taps(sample_rate: int):
    """(h, L, M): the library's resampling prototype for a rate (host only; test hook)."""
    l = _lib.lib()
    n, L, M = C.c_int64(), C.c_int32(), C.c_int32()
    check(l.sbv2_pcm_format_taps(sample_rate, None, 0, C.byref(n), C.byref(L), C.byref(M)))
    h = np.empty(n.value, np.float32)
    check(l.sbv2_pcm_format_taps(sample_rate, h.ctypes.data_as(f32p), h.size, C.byref(n), C.byref(L), C.byref(M)))
    return h, L.value, M.value


def flac_bound(fmt: PcmFormat, n_native: int) -> int:
    """Upper bound on the bytes of the FLAC stream of an n_native-sample 44.1 kHz signal in `fmt` (s16 only; host only)."""
    n = _lib.lib().sbv2_flac_bound(C.byref(fmt.c), int(n_native))
    if n < 0:
        raise Sbv2Error(_lib.lib().sbv2_last_error().decode(errors="replace"))
    return n


def _split_bytes(buf, sizes):
    out, o = [], 0
    for n in sizes:
        out.append(bytes(buf[o:o + int(n)]))
        o += int(n)
    return out


def debug_flac_encode(signals, sample_rate: int, device: int = 0):
    """Test hook: the device FLAC encoder on host int16 signals -> one FLAC stream (bytes) per signal."""
    sigs = [np.ascontiguousarray(np.asarray(x, np.int16)).reshape(-1) for x in signals]
    x = np.concatenate(sigs) if sigs else np.zeros(0, np.int16)
    lens = np.array([s.size for s in sigs], np.int64)
    cap = sum(42 + 16 * (-(-int(n) // 4096)) + 2 * int(n) for n in lens)
    dst = np.empty(max(cap, 1), np.uint8)
    got = np.zeros(len(sigs), np.int64)
    check(_lib.lib().sbv2_debug_flac_encode(int(device), x.ctypes.data_as(C.c_void_p) if x.size else None, lens.ctypes.data_as(i64p), len(sigs),
                                            int(sample_rate), dst.ctypes.data_as(C.c_void_p), dst.nbytes, got.ctypes.data_as(i64p)))
    return _split_bytes(dst, got)


def flac_stream_bound(fmt: PcmFormat, n_native: int) -> int:
    """Bytes that always suffice for one call of a FLAC stream whose chunks hold n_native 44.1 kHz samples (s16, not normalised; host only)."""
    n = _lib.lib().sbv2_flac_stream_bound(C.byref(fmt.c), int(n_native))
    if n < 0:
        raise Sbv2Error(_lib.lib().sbv2_last_error().decode(errors="replace"))
    return n


def debug_flac_stream_encode(x, cuts, sample_rate: int, device: int = 0):
    """Test hook: the device FLAC encoder fed piece by piece.  The host int16 signal x is cut at the ascending sample positions `cuts` into
    len(cuts) + 1 pushes (empty ones allowed) -> the bytes each push delivered, in order (their concatenation is the FLAC stream)."""
    x = np.ascontiguousarray(np.asarray(x, np.int16)).reshape(-1)
    cuts = np.ascontiguousarray(np.asarray(cuts, np.int64)).reshape(-1)
    dst = np.empty(42 + 16 * (-(-x.size // 4096)) + 2 * x.size, np.uint8)
    got = np.zeros(cuts.size + 1, np.int64)
    check(_lib.lib().sbv2_debug_flac_stream_encode(int(device), x.ctypes.data_as(C.c_void_p) if x.size else None, x.size,
                                                   cuts.ctypes.data_as(i64p) if cuts.size else None, cuts.size, int(sample_rate),
                                                   dst.ctypes.data_as(C.c_void_p), dst.nbytes, got.ctypes.data_as(i64p)))
    return _split_bytes(dst, got)


class Loudness:
    """Loudness normalisation of each output signal (struct sbv2_loudness): integrated loudness (BS.1770-4 gating) to target_lufs in
    [-70, -5], capped so the 4x true peak stays at or below true_peak_max dBTP in [-20, 0].  Measurement and gain run on the device."""

    def __init__(self, target_lufs: float, true_peak_max: float = -1.0):
        self.target_lufs, self.true_peak_max = float(target_lufs), float(true_peak_max)
        if not (np.isfinite(self.target_lufs) and -70.0 <= self.target_lufs <= -5.0):
            raise Sbv2Error(f"loudness target {target_lufs} LUFS is outside [-70, -5]")
        if not (np.isfinite(self.true_peak_max) and -20.0 <= self.true_peak_max <= 0.0):
            raise Sbv2Error(f"true-peak ceiling {true_peak_max} dBTP is outside [-20, 0]")
        self.c = _lib.Sbv2Loudness(self.target_lufs, self.true_peak_max)

    def __repr__(self):
        return f"Loudness({self.target_lufs}, true_peak_max={self.true_peak_max})"


def _loudness_arg(ln):
    return C.byref(ln.c) if ln is not None else None


def _f64p(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def loudness_kweight(sample_rate: int):
    """The library's K-weighting at a rate (host only): [shelf b0 b1 b2 a1 a2, high-pass b0 b1 b2 a1 a2]."""
    c = np.zeros(10, np.float64)
    check(_lib.lib().sbv2_loudness_kweight(int(sample_rate), _f64p(c)))
    return c


def debug_loudness(signals, sample_rate: int, loudness=None, device: int = 0):
    """Test hook: the device meter on host float64 signals at sample_rate -> stats [n, 3] (L LUFS, TP dBTP, G dB)."""
    sigs = [np.ascontiguousarray(np.asarray(x, np.float64)).reshape(-1) for x in signals]
    x = np.concatenate(sigs) if sigs else np.zeros(0, np.float64)
    lens = np.array([s.size for s in sigs], np.int64)
    stats = np.zeros((len(sigs), 3), np.float64)
    check(_lib.lib().sbv2_debug_loudness(int(device), x.ctypes.data_as(C.c_void_p) if x.size else None, lens.ctypes.data_as(i64p), len(sigs),
                                         int(sample_rate), _loudness_arg(loudness), _f64p(stats)))
    return stats


class Limiter:
    """Look-ahead true-peak limiter of each output signal (struct sbv2_limiter): integrated loudness to target_lufs in [-70, -5] with the
    sample peaks held at or below true_peak_max dBTP in [-20, 0] by a 10 ms look-ahead gain curve that takes no sample down by more than
    max_reduction dB in [0, 12].  Reaches targets that Loudness misses because the true peak binds first; where the plain scale fits (or
    max_reduction is 0) the output equals Loudness's bit for bit.  Runs on the device."""

    def __init__(self, target_lufs: float, true_peak_max: float = -1.0, max_reduction: float = 6.0):
        self.target_lufs, self.true_peak_max, self.max_reduction = float(target_lufs), float(true_peak_max), float(max_reduction)
        if not (np.isfinite(self.target_lufs) and -70.0 <= self.target_lufs <= -5.0):
            raise Sbv2Error(f"loudness target {target_lufs} LUFS is outside [-70, -5]")
        if not (np.isfinite(self.true_peak_max) and -20.0 <= self.true_peak_max <= 0.0):
            raise Sbv2Error(f"true-peak ceiling {true_peak_max} dBTP is outside [-20, 0]")
        if not (np.isfinite(self.max_reduction) and 0.0 <= self.max_reduction <= 12.0):
            raise Sbv2Error(f"limiter depth {max_reduction} dB is outside [0, 12]")
        self.c = _lib.Sbv2Limiter(self.target_lufs, self.true_peak_max, self.max_reduction, 0.0)

    def __repr__(self):
        return f"Limiter({self.target_lufs}, true_peak_max={self.true_peak_max}, max_reduction={self.max_reduction})"


def debug_limiter(signals, sample_rate: int, limiter: Limiter, device: int = 0):
    """Test hook: the device limiter on host float64 signals at sample_rate -> (the limited float64 signals, stats [n, 6]: L LUFS, TP dBTP,
    G dB, L_out LUFS, TP_out dBTP, deepest reduction dB)."""
    sigs = [np.ascontiguousarray(np.asarray(x, np.float64)).reshape(-1) for x in signals]
    x = np.concatenate(sigs) if sigs else np.zeros(0, np.float64)
    lens = np.array([s.size for s in sigs], np.int64)
    out = np.zeros(max(x.size, 1), np.float64)
    stats = np.zeros((len(sigs), 6), np.float64)
    check(_lib.lib().sbv2_debug_limiter(int(device), x.ctypes.data_as(C.c_void_p) if x.size else None, lens.ctypes.data_as(i64p), len(sigs),
                                        int(sample_rate), C.byref(limiter.c), out.ctypes.data_as(C.c_void_p), _f64p(stats)))
    return np.split(out[:x.size], np.cumsum(lens)[:-1]), stats


class Dynamics:
    """Speech compressor in front of a Loudness or a Limiter (struct sbv2_dynamics): what lies more than threshold_lu in [0, 30] dB above
    the signal's own integrated loudness is taken down by ratio in [1, 20] (1: nothing happens), the gain moving by attack in [10, 10000]
    dB/s ahead of a peak and by release in [1, 1000] dB/s behind it.  It evens out syllables and sentences so that the limiter is left with
    the crest only; it does not bound the signal and does not remove the crest factor.  Runs on the device."""

    def __init__(self, threshold_lu: float = 8.0, ratio: float = 4.0, attack: float = 600.0, release: float = 60.0):
        self.threshold_lu, self.ratio, self.attack, self.release = float(threshold_lu), float(ratio), float(attack), float(release)
        if not (np.isfinite(self.threshold_lu) and 0.0 <= self.threshold_lu <= 30.0):
            raise Sbv2Error(f"compressor threshold {threshold_lu} LU is outside [0, 30]")
        if not (np.isfinite(self.ratio) and 1.0 <= self.ratio <= 20.0):
            raise Sbv2Error(f"compressor ratio {ratio} is outside [1, 20]")
        if not (np.isfinite(self.attack) and 10.0 <= self.attack <= 10000.0):
            raise Sbv2Error(f"compressor attack {attack} dB/s is outside [10, 10000]")
        if not (np.isfinite(self.release) and 1.0 <= self.release <= 1000.0):
            raise Sbv2Error(f"compressor release {release} dB/s is outside [1, 1000]")
        self.c = _lib.Sbv2Dynamics(self.threshold_lu, self.ratio, self.attack, self.release, 0.0)

    def is_identity(self) -> bool:
        return self.ratio == 1.0

    def __repr__(self):
        return f"Dynamics({self.threshold_lu}, ratio={self.ratio}, attack={self.attack}, release={self.release})"


def dynamics_tile() -> int:
    """Samples per workgroup of the compressor's scans."""
    return int(_lib.lib().sbv2_dynamics_tile())


def debug_dynamics(signals, sample_rate: int, dynamics: Dynamics, device: int = 0):
    """Test hook: the device compressor on host float64 signals at sample_rate, always through the kernels -> (parts, stats [n, 3]: L LUFS,
    T, deepest compression dB); parts[i] has e, dq (int64), u (int64), s and y (the compressed signal) of signal i."""
    import types
    sigs = [np.ascontiguousarray(np.asarray(x, np.float64)).reshape(-1) for x in signals]
    x = np.concatenate(sigs) if sigs else np.zeros(0, np.float64)
    lens = np.array([s.size for s in sigs], np.int64)
    n = max(x.size, 1)
    e, s_, y = np.zeros(n, np.float64), np.zeros(n, np.float64), np.zeros(n, np.float64)
    dq, u = np.zeros(n, np.int64), np.zeros(n, np.int64)
    stats = np.zeros((len(sigs), 3), np.float64)
    check(_lib.lib().sbv2_debug_dynamics(int(device), x.ctypes.data_as(C.c_void_p) if x.size else None, lens.ctypes.data_as(i64p), len(sigs),
                                         int(sample_rate), C.byref(dynamics.c), _f64p(e), dq.ctypes.data_as(i64p), u.ctypes.data_as(i64p),
                                         _f64p(s_), _f64p(y), _f64p(stats)))
    cuts = np.cumsum(lens)[:-1]
    parts = [types.SimpleNamespace(e=a, dq=b, u=c, s=d, y=f)
             for a, b, c, d, f in zip(*(np.split(v[:x.size], cuts) for v in (e, dq, u, s_, y)))]
    return parts, stats


class StreamLevel:
    """Level control of a stream (struct sbv2_stream_level): a fixed gain of gain_db in [-40, 40] and the look-ahead gain curve of Limiter at
    that gain, which holds every sample at or below true_peak_max dBTP in [-20, 0].  No loudness target and no depth bound: the gain is the
    caller's (for a consistent level, target - L from the loudness stats of the voice), the depth is reported by StreamHandle.level_stats."""

    def __init__(self, gain_db: float, true_peak_max: float = -1.0):
        self.gain_db, self.true_peak_max = float(gain_db), float(true_peak_max)
        if not (np.isfinite(self.gain_db) and -40.0 <= self.gain_db <= 40.0):
            raise Sbv2Error(f"stream gain {gain_db} dB is outside [-40, 40]")
        if not (np.isfinite(self.true_peak_max) and -20.0 <= self.true_peak_max <= 0.0):
            raise Sbv2Error(f"true-peak ceiling {true_peak_max} dBTP is outside [-20, 0]")
        self.c = _lib.Sbv2StreamLevel(self.gain_db, self.true_peak_max, (C.c_double * 2)(0.0, 0.0))

    def __repr__(self):
        return f"StreamLevel({self.gain_db}, true_peak_max={self.true_peak_max})"


def stream_level_lookahead(fmt: PcmFormat) -> int:
    """A: the delivered samples a level stream runs behind, sample_rate // 100 + 11 (host only).  A depends on the rate alone; the C query
    takes f32 / s16 formats only, so a G.711 format asks with the s16 format of its rate."""
    c = PcmFormat(fmt.sample_rate, "s16").c if fmt.encoding in G711 else fmt.c
    n = _lib.lib().sbv2_stream_level_lookahead(C.byref(c))
    if n < 0:
        raise Sbv2Error(_lib.lib().sbv2_last_error().decode(errors="replace"))
    return n


def stream_level_bound(fmt: PcmFormat, n_native: int, flac: bool = False) -> int:
    """Bytes that always suffice for one call of a level stream whose chunks hold n_native 44.1 kHz samples (host only)."""
    n = _lib.lib().sbv2_stream_level_bound(C.byref(fmt.c), int(n_native), int(bool(flac)))
    if n < 0:
        raise Sbv2Error(_lib.lib().sbv2_last_error().decode(errors="replace"))
    return n


def debug_limiter_fixed(signals, sample_rate: int, level: StreamLevel, device: int = 0):
    """Test hook: the limiter's gain curve at the fixed gain of `level`, in one shot, on host float64 signals -> (the limited float64
    signals, stats [n, 2]: deepest reduction dB, max |x|)."""
    sigs = [np.ascontiguousarray(np.asarray(x, np.float64)).reshape(-1) for x in signals]
    x = np.concatenate(sigs) if sigs else np.zeros(0, np.float64)
    lens = np.array([s.size for s in sigs], np.int64)
    out = np.zeros(max(x.size, 1), np.float64)
    stats = np.zeros((len(sigs), 2), np.float64)
    check(_lib.lib().sbv2_debug_limiter_fixed(int(device), x.ctypes.data_as(C.c_void_p) if x.size else None, lens.ctypes.data_as(i64p), len(sigs),
                                              int(sample_rate), C.byref(level.c), out.ctypes.data_as(C.c_void_p), _f64p(stats)))
    return np.split(out[:x.size], np.cumsum(lens)[:-1]), stats


PARTS_SENTINEL = np.frombuffer(b"\x5a" * 8, np.float64)[0]   # what the *_parts hooks fill every returned device array with before the run


def _packed(signals):
    sigs = [np.ascontiguousarray(np.asarray(x, np.float64)).reshape(-1) for x in signals]
    x = np.concatenate(sigs) if sigs else np.zeros(0, np.float64)
    return x, np.array([s.size for s in sigs], np.int64)


def debug_loudness_parts(signals, sample_rate: int, device: int = 0):
    """Test hook: what each launch of the device meter leaves, on host float64 signals -> dict: stats [n, 3], m (segment length), e and st
    [nseg, 4], part [nseg], bmax [ceil(total / 256)], peak [n], taps [3, 24], strays (pad words a launch changed).  A slot of a device array
    that no launch wrote holds PARTS_SENTINEL."""
    x, lens = _packed(signals)
    cap_seg, cap_blk = int(np.sum(-(-lens // 200))) + 1, -(-x.size // 256) + 1
    stats, peak, taps, counts = np.zeros((len(lens), 3)), np.zeros(len(lens)), np.zeros((3, 24)), np.zeros(4, np.int64)
    e, st, part, bmax = np.zeros((cap_seg, 4)), np.zeros((cap_seg, 4)), np.zeros(cap_seg), np.zeros(cap_blk)
    check(_lib.lib().sbv2_debug_loudness_parts(int(device), x.ctypes.data_as(C.c_void_p) if x.size else None, lens.ctypes.data_as(i64p), len(lens),
                                               int(sample_rate), _f64p(stats), cap_seg, cap_blk, _f64p(e), _f64p(st), _f64p(part), _f64p(bmax),
                                               _f64p(peak), _f64p(taps), counts.ctypes.data_as(i64p)))
    m, nseg, nblk, strays = (int(v) for v in counts)
    return {"stats": stats, "m": m, "e": e[:nseg], "st": st[:nseg], "part": part[:nseg], "bmax": bmax[:nblk], "peak": peak, "taps": taps,
            "strays": strays}


def debug_limiter_parts(signals, sample_rate: int, level: StreamLevel, device: int = 0):
    """Test hook: what each launch of the fixed-gain limiter leaves, on host float64 signals -> dict: t and x [total], smin [tiles], taps [K],
    hsum, K, strays (pad words a launch changed).  A slot of a device array that no launch wrote holds PARTS_SENTINEL."""
    x, lens = _packed(signals)
    cap = int(np.sum(-(-lens // 1024))) + 1
    t, out, smin, taps, hsum, counts = np.zeros(x.size + 1), np.zeros(x.size + 1), np.zeros(cap), np.zeros(480), np.zeros(1), np.zeros(3, np.int64)
    check(_lib.lib().sbv2_debug_limiter_parts(int(device), x.ctypes.data_as(C.c_void_p) if x.size else None, lens.ctypes.data_as(i64p), len(lens),
                                              int(sample_rate), C.byref(level.c), cap, _f64p(t), _f64p(out), _f64p(smin), _f64p(taps), _f64p(hsum),
                                              counts.ctypes.data_as(i64p)))
    K, tiles, strays = (int(v) for v in counts)
    return {"t": t[:x.size], "x": out[:x.size], "smin": smin[:tiles], "taps": taps[:K], "hsum": float(hsum[0]), "K": K, "strays": strays}


def debug_limiter_stream(x, cuts, sample_rate: int, level: StreamLevel, device: int = 0):
    """Test hook: the same limiter fed piece by piece.  The host float64 signal x is cut at the ascending sample positions `cuts` into
    len(cuts) + 1 pushes (empty ones allowed) -> (the samples each push emitted, in order; stats [2])."""
    x = np.ascontiguousarray(np.asarray(x, np.float64)).reshape(-1)
    cuts = np.ascontiguousarray(np.asarray(cuts, np.int64)).reshape(-1)
    out = np.zeros(max(x.size, 1), np.float64)
    got = np.zeros(cuts.size + 1, np.int64)
    stats = np.zeros(2, np.float64)
    check(_lib.lib().sbv2_debug_limiter_stream(int(device), x.ctypes.data_as(C.c_void_p) if x.size else None, x.size,
                                               cuts.ctypes.data_as(i64p) if cuts.size else None, cuts.size, int(sample_rate), C.byref(level.c),
                                               out.ctypes.data_as(C.c_void_p), got.ctypes.data_as(i64p), _f64p(stats)))
    return np.split(out[:x.size], np.cumsum(got)[:-1]), stats


class StreamLeveler:
    """Loudness target of a level stream (struct sbv2_stream_leveler): the gain starts at the StreamLevel's gain_db (the guess) and follows
    target_lufs - (the gated BS.1770 loudness of everything heard so far), within gain_db +- range_db, at most slew_db_per_s, and not before
    hold_blocks 400 ms blocks have passed the absolute gate.  The StreamLevel's limiter runs behind it under its ceiling.  The loudness
    heard and the gain reached are reported by StreamHandle.leveler_stats: the next request of the voice can begin there."""

    def __init__(self, target_lufs: float, range_db: float = 12.0, slew_db_per_s: float = 3.0, hold_blocks: int = 10):
        self.target_lufs, self.range_db, self.slew_db_per_s = float(target_lufs), float(range_db), float(slew_db_per_s)
        if not (np.isfinite(self.target_lufs) and -70.0 <= self.target_lufs <= -5.0):
            raise Sbv2Error(f"leveler target {target_lufs} LUFS is outside [-70, -5]")
        if not (np.isfinite(self.range_db) and 0.0 <= self.range_db <= 20.0):
            raise Sbv2Error(f"leveler range {range_db} dB is outside [0, 20]")
        if not (np.isfinite(self.slew_db_per_s) and 0.0 < self.slew_db_per_s <= 20.0):
            raise Sbv2Error(f"leveler slew {slew_db_per_s} dB/s is outside (0, 20]")
        if isinstance(hold_blocks, bool) or not isinstance(hold_blocks, (int, np.integer)) or not 1 <= hold_blocks <= 100:
            raise Sbv2Error(f"leveler hold of {hold_blocks} blocks is outside [1, 100]")
        self.hold_blocks = int(hold_blocks)
        self.c = _lib.Sbv2StreamLeveler(self.target_lufs, self.range_db, self.slew_db_per_s, self.hold_blocks, 0)

    def __repr__(self):
        return f"StreamLeveler({self.target_lufs}, range_db={self.range_db}, slew_db_per_s={self.slew_db_per_s}, hold_blocks={self.hold_blocks})"


def debug_leveler_stream(x, cuts, sample_rate: int, level: StreamLevel, leveler: StreamLeveler, device: int = 0):
    """Test hook: the fed leveler and the stream limiter behind it.  The host float64 signal x is cut at the ascending sample positions `cuts`
    into len(cuts) + 1 pushes (empty ones allowed; none = the one shot) -> (the samples each push emitted, in order; g_k in dB for
    k = 0 .. len(x) // (sample_rate // 10); stats [6]: L_in, last g, min g, max g, deepest reduction dB, max |x|)."""
    x = np.ascontiguousarray(np.asarray(x, np.float64)).reshape(-1)
    cuts = np.ascontiguousarray(np.asarray(cuts, np.int64)).reshape(-1)
    out = np.zeros(max(x.size, 1), np.float64)
    got = np.zeros(cuts.size + 1, np.int64)
    gains = np.zeros(x.size // (int(sample_rate) // 10 or 1) + 1, np.float64)
    stats = np.zeros(6, np.float64)
    check(_lib.lib().sbv2_debug_leveler_stream(int(device), x.ctypes.data_as(C.c_void_p) if x.size else None, x.size,
                                               cuts.ctypes.data_as(i64p) if cuts.size else None, cuts.size, int(sample_rate), C.byref(level.c),
                                               C.byref(leveler.c), out.ctypes.data_as(C.c_void_p), got.ctypes.data_as(i64p), _f64p(gains), gains.size,
                                               _f64p(stats)))
    return np.split(out[:x.size], np.cumsum(got)[:-1]), gains, stats


class Marks:
    """Speech marks of one fetched signal (struct sbv2_marks): per token of the listed rows, in row then token order, the delivered-sample span
    [start, end) and, when levels were asked for, sumsq / peak of the delivered samples in it (s16 as integers; None otherwise); env_sumsq /
    env_peak per envelope frame of env_hop delivered samples (None without an envelope); out_len = the delivered samples of the signal."""

    def __init__(self, start, end, sumsq=None, peak=None, env_hop=0, env_sumsq=None, env_peak=None, out_len=0):
        self.start, self.end, self.sumsq, self.peak = start, end, sumsq, peak
        self.env_hop, self.env_sumsq, self.env_peak, self.out_len = int(env_hop), env_sumsq, env_peak, int(out_len)

    def arrays(self):
        return [a for a in (self.start, self.end, self.sumsq, self.peak, self.env_sumsq, self.env_peak) if a is not None]


PITCH_THRESHOLD = 0.15   # YIN's usual absolute threshold


class Pitch:
    """Options and, once a call has filled it, results of the pitch estimator (struct sbv2_pitch: YIN per frame of `hop` delivered samples,
    include/sbv2_hip.h states it).  Results: f0 [n] in Hz (0 for an unvoiced frame), ap [n] = c(lag), the aperiodicity, lag [n] in samples;
    frame f has its centre at f hop + hop // 2.  None before a call."""

    def __init__(self, hop: int, f0_min: float = 70.0, f0_max: float = 600.0, threshold: float = PITCH_THRESHOLD):
        self.hop, self.f0_min, self.f0_max, self.threshold = int(hop), float(f0_min), float(f0_max), float(threshold)
        self.f0 = self.ap = self.lag = None

    def n_frames(self, n: int) -> int:
        return -(-int(n) // self.hop) if n > 0 and self.hop > 0 else 0

    def c_struct(self, n: int):
        """A sbv2_pitch over fresh arrays for a signal of n delivered samples; take() keeps them once the call has succeeded."""
        nf = self.n_frames(n)
        arrays = np.zeros(max(nf, 1), np.float64), np.zeros(max(nf, 1), np.float64), np.zeros(max(nf, 1), np.int32)
        c = _lib.Sbv2Pitch(self.hop if -2 ** 31 <= self.hop < 2 ** 31 else 0, 0, self.f0_min, self.f0_max, self.threshold, nf, _f64p(arrays[0]),
                           _f64p(arrays[1]), arrays[2].ctypes.data_as(C.POINTER(C.c_int32)), 0)
        return c, arrays

    def take(self, c, arrays):
        assert c.n_frames == c.capacity, (c.n_frames, c.capacity)
        self.f0, self.ap, self.lag = (a[:c.n_frames] for a in arrays)
        return self


def pitch_lags(sample_rate: int, f0_min: float, f0_max: float):
    """(tau_min, tau_max) = (floor(sr / f0_max), ceil(sr / f0_min)) under the library's checks: 40 <= f0_min < f0_max <= sr / 4
    (sbv2_pitch_lags; host only)."""
    a, b = C.c_int32(0), C.c_int32(0)
    check(_lib.lib().sbv2_pitch_lags(int(sample_rate), float(f0_min), float(f0_max), C.byref(a), C.byref(b)))
    return a.value, b.value


def debug_pitch(x, sample_rate: int, pitch: Pitch, device: int = 0, encoding: str | None = None):
    """Test hook: the pitch estimator on host samples (sbv2_debug_pitch).  x: int16 or float32 samples, or with encoding "mulaw" / "alaw"
    uint8 codes -> (pitch with f0 / ap / lag filled, cmnd3 [n][3] = c(lag - 1), c(lag), c(lag + 1), voiced [n])."""
    x = np.ascontiguousarray(x).reshape(-1)
    if encoding is None and x.dtype not in (np.int16, np.float32):
        raise Sbv2Error(f"pitch is taken of int16 or float32 samples, not {x.dtype}")
    if encoding is not None and (encoding not in ENCODINGS or x.dtype != _DTYPES[encoding]):
        raise Sbv2Error(f"pitch of {encoding!r} samples is not taken of {x.dtype}")
    enc = ENCODINGS[encoding] if encoding is not None else int(x.dtype == np.int16)
    c, arrays = pitch.c_struct(x.size)
    c3, voiced = np.zeros((len(arrays[0]), 3), np.float64), np.zeros(len(arrays[0]), np.int32)   # (at least one entry: never a NULL)
    check(_lib.lib().sbv2_debug_pitch(int(device), x.ctypes.data_as(C.c_void_p) if x.size else None, enc, x.size, int(sample_rate), C.byref(c),
                                      _f64p(c3), voiced.ctypes.data_as(C.POINTER(C.c_int32))))
    return pitch.take(c, arrays), c3[:c.n_frames], voiced[:c.n_frames]


class PitchTrack:
    """Octave-error repair of a pitch contour (struct sbv2_pitch_track: one best path through the frames' candidates, include/sbv2_hip.h states
    it).  cand_max in (0, 1]: a dip of c at or above it is no candidate; unvoiced_cost and switch_cost in [0, 4], jump_cost in [0, 16], all in
    units of c.  The defaults live here only: the library takes every value as given (0 is 0) and checks the ranges."""

    def __init__(self, cand_max: float = 0.5, unvoiced_cost: float = 0.30, switch_cost: float = 0.20, jump_cost: float = 1.0):
        self.cand_max, self.unvoiced_cost = float(cand_max), float(unvoiced_cost)
        self.switch_cost, self.jump_cost = float(switch_cost), float(jump_cost)

    @property
    def c(self):
        return _lib.Sbv2PitchTrack(self.cand_max, self.unvoiced_cost, self.switch_cost, self.jump_cost, (C.c_int32 * 2)(0, 0))

    def __repr__(self):
        return f"PitchTrack({self.cand_max}, {self.unvoiced_cost}, {self.switch_cost}, {self.jump_cost})"


TRACK_CAND = 7   # candidates a frame keeps; a record is (ncand, 7 tau, 7 q)


def debug_pitch_track(x, sample_rate: int, pitch, track: PitchTrack, device: int = 0, encoding: str | None = None, cand=None):
    """Test hook: the tracker (sbv2_debug_pitch_track).  x as for debug_pitch -> a namespace: pitch (f0 / ap / lag of the TRACKED contour), cand
    [n][15] int32 (ncand, 7 tau, 7 q), c3 [n][7][3] (c-, c0, c+ of every candidate), state [n] (0 .. 6 the candidate, 7 unvoiced).
    With cand (an int32 table [n][15]) the path alone is found on that table: x, sample_rate and pitch are not looked at -> state [n]."""
    import types
    i32p = C.POINTER(C.c_int32)
    ct = track.c
    if cand is not None:
        tab = np.ascontiguousarray(np.asarray(cand, np.int32).reshape(-1, 2 * TRACK_CAND + 1))
        state = np.zeros(max(len(tab), 1), np.int32)
        pad = tab if len(tab) else np.zeros((1, 2 * TRACK_CAND + 1), np.int32)   # (never a NULL: NULL means "extract")
        check(_lib.lib().sbv2_debug_pitch_track(int(device), None, 0, 0, 0, None, C.byref(ct), pad.ctypes.data_as(i32p), None, len(tab), None, None,
                                                state.ctypes.data_as(i32p)))
        return state[:len(tab)]
    x = np.ascontiguousarray(x).reshape(-1)
    if encoding is None and x.dtype not in (np.int16, np.float32):
        raise Sbv2Error(f"pitch is taken of int16 or float32 samples, not {x.dtype}")
    if encoding is not None and (encoding not in ENCODINGS or x.dtype != _DTYPES[encoding]):
        raise Sbv2Error(f"pitch of {encoding!r} samples is not taken of {x.dtype}")
    enc = ENCODINGS[encoding] if encoding is not None else int(x.dtype == np.int16)
    c, arrays = pitch.c_struct(x.size)
    nf = len(arrays[0])   # (at least one entry: never a NULL)
    tab, c3, state = np.zeros((nf, 2 * TRACK_CAND + 1), np.int32), np.zeros((nf, TRACK_CAND, 3), np.float64), np.zeros(nf, np.int32)
    check(_lib.lib().sbv2_debug_pitch_track(int(device), x.ctypes.data_as(C.c_void_p) if x.size else None, enc, x.size, int(sample_rate), C.byref(c),
                                            C.byref(ct), None, None, 0, tab.ctypes.data_as(i32p), _f64p(c3), state.ctypes.data_as(i32p)))
    n = c.n_frames
    return types.SimpleNamespace(pitch=pitch.take(c, arrays), cand=tab[:n], c3=c3[:n], state=state[:n])


class Voice:
    """Pitch and intonation scale of a fetched request (struct sbv2_voice: a length-preserving TD-PSOLA of the run's native rows on the device,
    include/sbv2_hip.h states it).  pitch_scale in [0.5, 2] multiplies f0, intonation_scale in [0, 2] scales its excursions about the rows' mean;
    hop = native samples per contour frame (0 = rate // 200); f0_min / f0_max / threshold as Pitch has them (0 = 70, 600, 0.15).  Ranges are
    checked by the library."""

    def __init__(self, pitch_scale: float = 1.0, intonation_scale: float = 1.0, hop: int = 0, f0_min: float = 0.0, f0_max: float = 0.0,
                 threshold: float = 0.0):
        self.pitch_scale, self.intonation_scale, self.hop = float(pitch_scale), float(intonation_scale), int(hop)
        self.f0_min, self.f0_max, self.threshold = float(f0_min), float(f0_max), float(threshold)

    @property
    def c(self):
        return _lib.Sbv2Voice(self.pitch_scale, self.intonation_scale, self.f0_min, self.f0_max, self.threshold,
                              self.hop if -2 ** 31 <= self.hop < 2 ** 31 else -1, 0)

    def is_identity(self) -> bool:
        return self.pitch_scale == 1.0 and self.intonation_scale == 1.0

    def __repr__(self):
        return f"Voice({self.pitch_scale}, {self.intonation_scale}, hop={self.hop})"


class TokenPitch:
    """Per-token pitch targets of a fetched request (struct sbv2_token_pitch, include/sbv2_hip.h states it): values, one per token of the listed
    rows in marks order, 0 = not edited; kind "hz" (the token's target mean f0) or "ratio" (in [0.5, 2]); smooth = contour frames to each side
    over which the ratio changes (0 = steps).  Ranges are checked by the library.  Once a call has filled it: applied [n] (the ratio used, 1.0
    where not edited) and src_f0 [n] (the token's measured mean f0 before any shift, 0 where it has no voiced frame); None before."""
    KINDS = {"ratio": 0, "hz": 1}

    def __init__(self, values, kind: str = "hz", smooth: int = 2):
        if kind not in self.KINDS:
            raise Sbv2Error(f"token pitch kind must be \"hz\" or \"ratio\", not {kind!r}")
        self.values = np.ascontiguousarray(np.asarray(values, np.float64).reshape(-1))
        self.kind, self.smooth = kind, int(smooth)
        self.applied = self.src_f0 = None

    def c_struct(self):
        """A sbv2_token_pitch over fresh output arrays; take() keeps them once the call has succeeded."""
        n = self.values.size
        arrays = np.ones(max(n, 1), np.float64), np.zeros(max(n, 1), np.float64)
        pad = self.values if n else np.zeros(1, np.float64)   # (never a NULL for an empty table)
        c = _lib.Sbv2TokenPitch(_f64p(pad), n, self.KINDS[self.kind], self.smooth if -2 ** 31 <= self.smooth < 2 ** 31 else -1, _f64p(arrays[0]),
                                _f64p(arrays[1]), 0)
        return c, arrays + (pad,)

    def take(self, arrays):
        self.applied, self.src_f0 = arrays[0][:self.values.size], arrays[1][:self.values.size]
        return self

    def __repr__(self):
        return f"TokenPitch({self.values.size} tokens, {self.kind!r}, smooth={self.smooth})"


class Formant:
    """Formant scale of a fetched request (struct sbv2_formant, include/sbv2_hip.h states it): every grain of the shifter is read at
    formant_scale times its offset, which moves the spectral envelope by that factor and leaves f0, the marks and the length alone.
    formant_scale in [0.5, 2], 1 = the identity; checked by the library."""

    def __init__(self, formant_scale: float = 1.0):
        self.formant_scale = float(formant_scale)

    @property
    def c(self):
        return _lib.Sbv2Formant(self.formant_scale, 0.0)

    def is_identity(self) -> bool:
        return self.formant_scale == 1.0

    def __repr__(self):
        return f"Formant({self.formant_scale})"


def voice_tile() -> int:
    """Output samples per workgroup of the shifter's overlap-add gather (sbv2_voice_tile)."""
    return int(_lib.lib().sbv2_voice_tile())


def debug_voice_shift(rows, sample_rate: int, voice: Voice, period=None, voiced=None, device: int = 0, formant=None):
    """Test hook: the shifter on host rows (sbv2_debug_voice_shift), always through its kernels.  rows: float32 arrays (one array = one row);
    period / voiced: per row, the contour to use instead of the estimated one (both or neither) -> a list of namespaces, one per row: y, period
    and voiced (per frame, as used), ta, ts, map.  formant: a Formant -> sbv2_debug_voice_formant, always through the formant gather."""
    import types
    if isinstance(rows, np.ndarray):
        rows = [rows]
    rows = [np.ascontiguousarray(r).reshape(-1) for r in rows]
    for r in rows:
        if r.dtype != np.float32:
            raise Sbv2Error(f"the shifter takes float32 rows, not {r.dtype}")
    lens = np.array([r.size for r in rows], np.int64)
    x = np.ascontiguousarray(np.concatenate(rows + [np.zeros(0, np.float32)]))
    c = voice.c
    hop = voice.hop if voice.hop else int(sample_rate) // 200
    nfs = [-(-int(n) // hop) if n and hop > 0 else 0 for n in lens]
    nf, total = int(sum(nfs)), int(lens.sum())
    i32p = C.POINTER(C.c_int32)
    pin = vin = None
    if (period is None) != (voiced is None):
        raise Sbv2Error("period and voiced are given together or not at all")
    if period is not None:
        if isinstance(period, np.ndarray):
            period, voiced = [period], [voiced]
        pin = np.ascontiguousarray(np.concatenate([np.asarray(a, np.float64).reshape(-1) for a in period] + [np.zeros(0)]))
        vin = np.ascontiguousarray(np.concatenate([np.asarray(a).reshape(-1) for a in voiced] + [np.zeros(0)]).astype(np.int32))
        if pin.size != nf or vin.size != nf:
            raise Sbv2Error(f"the contour must hold one entry per frame ({nf})")
        pin, vin = np.concatenate([pin, [0.0]]), np.concatenate([vin, [0]]).astype(np.int32)   # (never a NULL for an empty contour)
    pout, vout = np.zeros(nf + 1, np.float64), np.zeros(nf + 1, np.int32)
    ta, ts, mp = (np.zeros(total + len(rows) + 1, np.int32) for _ in range(3))
    nm = np.zeros((len(rows) + 1, 2), np.int64)
    y = np.zeros(total + 1, np.float32)
    head = (int(device), x.ctypes.data_as(_lib.f32p) if total else None, lens.ctypes.data_as(i64p) if len(rows) else None, len(rows), int(sample_rate),
            C.byref(c))
    tail = (_f64p(pin) if pin is not None else None, vin.ctypes.data_as(i32p) if vin is not None else None, _f64p(pout), vout.ctypes.data_as(i32p),
            ta.ctypes.data_as(i32p), ts.ctypes.data_as(i32p), mp.ctypes.data_as(i32p), nm.ctypes.data_as(i64p), y.ctypes.data_as(_lib.f32p))
    if formant is not None:
        cf = formant.c
        check(_lib.lib().sbv2_debug_voice_formant(*head, C.byref(cf), *tail))
    else:
        check(_lib.lib().sbv2_debug_voice_shift(*head, *tail))
    out, at, fa, ma = [], 0, 0, 0
    for i, n in enumerate(lens):
        n, na, ns = int(n), int(nm[i, 0]), int(nm[i, 1])
        out.append(types.SimpleNamespace(y=y[at:at + n].copy(), period=pout[fa:fa + nfs[i]].copy(), voiced=vout[fa:fa + nfs[i]].copy(),
                                         ta=ta[ma:ma + na].astype(np.int64), ts=ts[ma:ma + ns].astype(np.int64), map=mp[ma:ma + ns].astype(np.int64)))
        at, fa, ma = at + n, fa + nfs[i], ma + n + 1
    return out


def debug_voice_formant(rows, sample_rate: int, voice: Voice, formant: Formant, period=None, voiced=None, device: int = 0):
    """Test hook: the shifter with a formant scale on host rows (sbv2_debug_voice_formant), always through k_voice_gather_fmt (scale 1
    included); arguments and results as debug_voice_shift has them."""
    return debug_voice_shift(rows, sample_rate, voice, period, voiced, device, formant=formant)


class StreamVoice:
    """Pitch, intonation and formant scale of a request STREAM (struct sbv2_stream_voice, include/sbv2_hip.h states it): the shifter of Voice
    and Formant fed chunk by chunk on the device.  pivot_hz: the f0 the intonation scale pivots about in place of the row's mean, which a stream
    cannot know ahead: one value for every row or one per row, each in [f0_min, f0_max]; read it from a /synthesize_marks answer of the same
    voice.  The identity (all three scales 1) is refused by the library: begin the stream without a voice."""

    def __init__(self, pitch_scale: float = 1.0, intonation_scale: float = 1.0, formant_scale: float = 1.0, pivot_hz=None, hop: int = 0,
                 f0_min: float = 0.0, f0_max: float = 0.0, threshold: float = 0.0):
        self.voice = Voice(pitch_scale, intonation_scale, hop, f0_min, f0_max, threshold)
        self.formant_scale = float(formant_scale)
        self.pivot_hz = None if pivot_hz is None else np.ascontiguousarray(np.asarray(pivot_hz, np.float64).reshape(-1))

    def c_struct(self, rows: int):
        """(sbv2_stream_voice, the pivot array it points to) for a stream of `rows` rows: a scalar pivot is repeated, None stays NULL."""
        piv = self.pivot_hz
        if piv is not None:
            if piv.size == 1 and rows != 1:
                piv = np.ascontiguousarray(np.repeat(piv, max(rows, 1)))
            if piv.size != rows:
                raise Sbv2Error(f"pivot_hz must be one value or one per row ({rows}), not {piv.size}")
        return _lib.Sbv2StreamVoice(self.voice.c, self.formant_scale, _f64p(piv) if piv is not None else None, (C.c_double * 2)(0.0, 0.0)), piv

    def __repr__(self):
        return f"StreamVoice({self.voice.pitch_scale}, {self.voice.intonation_scale}, {self.formant_scale}, pivot_hz={self.pivot_hz})"


def stream_voice_lookahead(voice: StreamVoice, sample_rate: int = 44100) -> int:
    """A_v: the native samples of a row that must follow a shifted sample before it is final (sbv2_stream_voice_lookahead; host only)."""
    c, _keep = voice.c_struct(0 if voice.pivot_hz is None else voice.pivot_hz.size)
    a = int(_lib.lib().sbv2_stream_voice_lookahead(C.byref(c), int(sample_rate)))
    if a < 0:
        raise Sbv2Error(_lib.lib().sbv2_last_error().decode())
    return a


def stream_voice_timeline(frames, gaps, hop: int, chunk_frames: int, voice: StreamVoice, fmt: PcmFormat | None = None):
    """The samples every call of a voice stream without a level delivers (sbv2_stream_voice_timeline; host only)."""
    fr, fp = _i64(frames)
    gp_a, gp = _i64(gaps)
    n = int(fr.size)
    cap = int(sum(-(-int(f) // max(int(chunk_frames), 1)) for f in fr if f > 0)) + 1
    calls, ncalls = np.zeros(cap, np.int64), C.c_int64()
    c, _keep = voice.c_struct(0 if voice.pivot_hz is None else voice.pivot_hz.size)
    check(_lib.lib().sbv2_stream_voice_timeline(fp, gp, n, int(hop), int(chunk_frames), C.byref(fmt.c) if fmt is not None else None, C.byref(c),
                                                calls.ctypes.data_as(i64p), cap, C.byref(ncalls)))
    return calls[:ncalls.value]


def debug_voice_stream(x, cuts, sample_rate: int, voice: StreamVoice, period=None, voiced=None, device: int = 0):
    """Test hook: the fed shifter on one float32 row cut at `cuts` into len(cuts) + 1 pushes (sbv2_debug_voice_stream) -> (y, per_push): the
    pushes' final samples back to back and their counts.  period / voiced: the contour to use instead of the estimated one."""
    x = np.ascontiguousarray(x).reshape(-1)
    if x.dtype != np.float32:
        raise Sbv2Error(f"the shifter takes float32 rows, not {x.dtype}")
    ct, cp = _i64(cuts)
    i32p = C.POINTER(C.c_int32)
    pin = vin = None
    if (period is None) != (voiced is None):
        raise Sbv2Error("period and voiced are given together or not at all")
    if period is not None:
        pin = np.concatenate([np.asarray(period, np.float64).reshape(-1), [0.0]])
        vin = np.concatenate([np.asarray(voiced).reshape(-1), [0]]).astype(np.int32)
    c, _keep = voice.c_struct(1)
    y, per = np.zeros(x.size + 1, np.float32), np.zeros(ct.size + 1, np.int64)
    check(_lib.lib().sbv2_debug_voice_stream(int(device), x.ctypes.data_as(_lib.f32p) if x.size else None, x.size, cp if ct.size else None, ct.size,
                                             int(sample_rate), C.byref(c), _f64p(pin) if pin is not None else None,
                                             vin.ctypes.data_as(i32p) if vin is not None else None, y.ctypes.data_as(_lib.f32p),
                                             per.ctypes.data_as(i64p)))
    return y[:x.size].copy(), per


def debug_voice_tokens(rows, sample_rate: int, voice: Voice, tok_ends, token_pitch: TokenPitch, period=None, voiced=None, device: int = 0):
    """Test hook: the shifter with a token table on host rows (sbv2_debug_voice_tokens), always through its kernels.  rows, period, voiced as
    for debug_voice_shift; tok_ends: per row the ascending end positions of its tokens in samples (one array = one row); token_pitch: the
    values of all rows' tokens back to back -> (a list of namespaces as debug_voice_shift gives, each with ratio [frames] = R_f, applied and
    src_f0 [the row's tokens] besides; token_pitch with applied / src_f0 of all tokens filled)."""
    import types
    if isinstance(rows, np.ndarray):
        rows = [rows]
        tok_ends = [tok_ends]
    rows = [np.ascontiguousarray(r).reshape(-1) for r in rows]
    for r in rows:
        if r.dtype != np.float32:
            raise Sbv2Error(f"the shifter takes float32 rows, not {r.dtype}")
    ends = [np.asarray(e, np.int64).reshape(-1) for e in tok_ends]
    if len(ends) != len(rows):
        raise Sbv2Error(f"tok_ends must hold one array per row ({len(rows)})")
    counts = np.array([e.size for e in ends] + [0], np.int64)
    ends_all = np.ascontiguousarray(np.concatenate(ends + [np.zeros(1, np.int64)]))
    lens = np.array([r.size for r in rows], np.int64)
    x = np.ascontiguousarray(np.concatenate(rows + [np.zeros(0, np.float32)]))
    c = voice.c
    hop = voice.hop if voice.hop else int(sample_rate) // 200
    nfs = [-(-int(n) // hop) if n and hop > 0 else 0 for n in lens]
    nf, total = int(sum(nfs)), int(lens.sum())
    i32p = C.POINTER(C.c_int32)
    pin = vin = None
    if (period is None) != (voiced is None):
        raise Sbv2Error("period and voiced are given together or not at all")
    if period is not None:
        if isinstance(period, np.ndarray):
            period, voiced = [period], [voiced]
        pin = np.ascontiguousarray(np.concatenate([np.asarray(a, np.float64).reshape(-1) for a in period] + [np.zeros(0)]))
        vin = np.ascontiguousarray(np.concatenate([np.asarray(a).reshape(-1) for a in voiced] + [np.zeros(0)]).astype(np.int32))
        if pin.size != nf or vin.size != nf:
            raise Sbv2Error(f"the contour must hold one entry per frame ({nf})")
        pin, vin = np.concatenate([pin, [0.0]]), np.concatenate([vin, [0]]).astype(np.int32)
    pout, vout, rout = np.zeros(nf + 1, np.float64), np.zeros(nf + 1, np.int32), np.zeros(nf + 1, np.float64)
    ta, ts, mp = (np.zeros(total + len(rows) + 1, np.int32) for _ in range(3))
    nm = np.zeros((len(rows) + 1, 2), np.int64)
    y = np.zeros(total + 1, np.float32)
    ctp, tparr = token_pitch.c_struct()
    check(_lib.lib().sbv2_debug_voice_tokens(int(device), x.ctypes.data_as(_lib.f32p) if total else None, lens.ctypes.data_as(i64p) if len(rows) else None,
                                             len(rows), int(sample_rate), C.byref(c), _f64p(pin) if pin is not None else None,
                                             vin.ctypes.data_as(i32p) if vin is not None else None, counts.ctypes.data_as(i64p),
                                             ends_all.ctypes.data_as(i64p), C.byref(ctp), _f64p(pout), vout.ctypes.data_as(i32p),
                                             ta.ctypes.data_as(i32p), ts.ctypes.data_as(i32p), mp.ctypes.data_as(i32p), nm.ctypes.data_as(i64p),
                                             y.ctypes.data_as(_lib.f32p), _f64p(rout)))
    token_pitch.take(tparr)
    out, at, fa, ma, tk = [], 0, 0, 0, 0
    for i, n in enumerate(lens):
        n, na, ns, nt = int(n), int(nm[i, 0]), int(nm[i, 1]), int(counts[i])
        out.append(types.SimpleNamespace(y=y[at:at + n].copy(), period=pout[fa:fa + nfs[i]].copy(), voiced=vout[fa:fa + nfs[i]].copy(),
                                         ta=ta[ma:ma + na].astype(np.int64), ts=ts[ma:ma + ns].astype(np.int64), map=mp[ma:ma + ns].astype(np.int64),
                                         ratio=rout[fa:fa + nfs[i]].copy(), applied=token_pitch.applied[tk:tk + nt].copy(),
                                         src_f0=token_pitch.src_f0[tk:tk + nt].copy()))
        at, fa, ma, tk = at + n, fa + nfs[i], ma + n + 1, tk + nt
    return out, token_pitch


def debug_stream_pitch(x, cuts, sample_rate: int, pitch: Pitch, device: int = 0, encoding: str | None = None):
    """Test hook: the fed pitch estimator on its own (sbv2_debug_stream_pitch).  x as for debug_pitch, cut at the ascending positions `cuts`
    into len(cuts) + 1 pushes -> debug_pitch's results and per_push [len(cuts) + 1], the frames each push completed."""
    x = np.ascontiguousarray(x).reshape(-1)
    if encoding is None and x.dtype not in (np.int16, np.float32):
        raise Sbv2Error(f"pitch is taken of int16 or float32 samples, not {x.dtype}")
    if encoding is not None and (encoding not in ENCODINGS or x.dtype != _DTYPES[encoding]):
        raise Sbv2Error(f"pitch of {encoding!r} samples is not taken of {x.dtype}")
    enc = ENCODINGS[encoding] if encoding is not None else int(x.dtype == np.int16)
    cuts = np.ascontiguousarray(np.asarray(cuts, np.int64).reshape(-1))
    c, arrays = pitch.c_struct(x.size)
    c3, voiced = np.zeros((len(arrays[0]), 3), np.float64), np.zeros(len(arrays[0]), np.int32)
    per_push = np.zeros(cuts.size + 1, np.int64)
    check(_lib.lib().sbv2_debug_stream_pitch(int(device), x.ctypes.data_as(C.c_void_p) if x.size else None, enc, x.size,
                                             cuts.ctypes.data_as(i64p) if cuts.size else None, cuts.size, int(sample_rate), C.byref(c), _f64p(c3),
                                             voiced.ctypes.data_as(C.POINTER(C.c_int32)), per_push.ctypes.data_as(i64p)))
    return pitch.take(c, arrays), c3[:c.n_frames], voiced[:c.n_frames], per_push


def stream_pitch_complete(D: int, hop: int, tau_max: int, total: int) -> int:
    """The completion rule of a stream's pitch contour (above sbv2_stream_next_pitch): the number of frames f < ceil(total / hop) with
    min(f hop + hop // 2 + tau_max, total) <= D.  They are the first ones: frames complete in order."""
    D, hop, tau_max, total = int(D), int(hop), int(tau_max), int(total)
    nf = -(-total // hop) if total > 0 else 0
    if D >= total:
        return nf
    r = D - tau_max - hop // 2
    return 0 if r < 0 else min(nf, r // hop + 1)


def full_scale(encoding: str) -> float:
    """Full scale of the delivered samples' levels: 32767 for s16 and for G.711 (levels of the decoded integers), 1 for f32."""
    return 1.0 if encoding == "f32" else 32767.0


def level_dbfs(sumsq, n, encoding: str = "f32"):
    """10 log10(sumsq / n) re full scale (s16, mulaw, alaw: 32767) of a span of n delivered samples; None for an empty or all-zero one."""
    if n <= 0 or sumsq <= 0:
        return None
    return float(10.0 * np.log10(float(sumsq) / n / full_scale(encoding) ** 2))


def marks_spans(durations, hop: int, place: int, fmt: PcmFormat):
    """(start, end): delivered-sample spans of one row's tokens with `durations` frames each, the row at native sample `place`, in fmt's
    rate (sbv2_marks_spans; host only)."""
    d = np.ascontiguousarray(np.asarray(durations, np.int64).reshape(-1))
    st, en = np.zeros(d.size, np.int64), np.zeros(d.size, np.int64)
    check(_lib.lib().sbv2_marks_spans(d.ctypes.data_as(i64p), d.size, int(hop), int(place), C.byref(fmt.c), st.ctypes.data_as(i64p),
                                      en.ctypes.data_as(i64p)))
    return st, en


def debug_stream_levels(x, cuts, starts, ends, env_hop: int = 0, device: int = 0, encoding: str | None = None):
    """Test hook: the fed level reduction on its own (sbv2_debug_stream_levels).  x as for debug_segment_levels, cut at the ascending positions
    `cuts` into len(cuts) + 1 pushes; segments monotone and disjoint -> (sumsq, peak, env_sumsq, env_peak, seg_per_push, env_per_push)."""
    x = np.ascontiguousarray(x).reshape(-1)
    if encoding is None and x.dtype not in (np.int16, np.float32):
        raise Sbv2Error(f"levels are taken of int16 or float32 samples, not {x.dtype}")
    if encoding is not None and (encoding not in ENCODINGS or x.dtype != _DTYPES[encoding]):
        raise Sbv2Error(f"levels of {encoding!r} samples are not taken of {x.dtype}")
    enc = ENCODINGS[encoding] if encoding is not None else int(x.dtype == np.int16)
    st, en, cuts = (np.ascontiguousarray(np.asarray(a, np.int64).reshape(-1)) for a in (starts, ends, cuts))
    nenv = -(-x.size // int(env_hop)) if env_hop > 0 else 0
    ss, pk, es, ep = (np.zeros(max(n, 1), np.float64) for n in (st.size, st.size, nenv, nenv))
    sp, epp = np.zeros(cuts.size + 1, np.int64), np.zeros(cuts.size + 1, np.int64)
    check(_lib.lib().sbv2_debug_stream_levels(int(device), x.ctypes.data_as(C.c_void_p) if x.size else None, enc, x.size,
                                              cuts.ctypes.data_as(i64p) if cuts.size else None, cuts.size, st.ctypes.data_as(i64p),
                                              en.ctypes.data_as(i64p), st.size, int(env_hop), _f64p(ss), _f64p(pk), _f64p(es), _f64p(ep),
                                              sp.ctypes.data_as(i64p), epp.ctypes.data_as(i64p)))
    return ss[:st.size], pk[:st.size], es[:nenv], ep[:nenv], sp, epp


def debug_segment_levels(x, starts, ends, device: int = 0, encoding: str | None = None):
    """Test hook: the device level reduction on host samples x (int16 or float32; uint8 G.711 codes with encoding "mulaw" / "alaw") ->
    (sumsq, peak) per segment [starts[i], ends[i])."""
    x = np.ascontiguousarray(x).reshape(-1)
    if encoding is None and x.dtype not in (np.int16, np.float32):
        raise Sbv2Error(f"levels are taken of int16 or float32 samples, not {x.dtype}")
    if encoding is not None and (encoding not in ENCODINGS or x.dtype != _DTYPES[encoding]):
        raise Sbv2Error(f"levels of {encoding!r} samples are not taken of {x.dtype}")
    enc = ENCODINGS[encoding] if encoding is not None else int(x.dtype == np.int16)
    st, en = (np.ascontiguousarray(np.asarray(a, np.int64).reshape(-1)) for a in (starts, ends))
    ss, pk = np.zeros(st.size, np.float64), np.zeros(st.size, np.float64)
    check(_lib.lib().sbv2_debug_segment_levels(int(device), x.ctypes.data_as(C.c_void_p) if x.size else None, enc, x.size,
                                               st.ctypes.data_as(i64p), en.ctypes.data_as(i64p), st.size, _f64p(ss), _f64p(pk)))
    return ss, pk


def debug_assist_blend(F, col_map, row_of, a_start, a_len, text_of, weight, device: int = 0):
    """(mean [A][C], out [C][L], stray, raw) of the two assist kernels on the host plane F [C][ld] (sbv2_debug_assist_blend): assist sequence a
    is F's columns [a_start[a], a_start[a] + a_len[a]), text column t reads column col_map[t] (< 0: padding) and belongs to row row_of[t];
    text_of / weight per row as in sbv2_assist.  mean and out come back as uint32 words too (raw), so that a word the kernels never wrote
    (0x5A5A5A5A) can be told from a value."""
    F = np.ascontiguousarray(F, np.float32)
    i32 = lambda a: np.ascontiguousarray(np.asarray(a, np.int32).reshape(-1))
    m, r, st, ln, to = i32(col_map), i32(row_of), i32(a_start), i32(a_len), i32(text_of)
    w = np.ascontiguousarray(np.asarray(weight, np.float64).reshape(-1))
    Cn, ld = F.shape
    mean, out, stray = np.zeros((st.size, Cn), np.float32), np.zeros((Cn, m.size), np.float32), C.c_int64(-1)
    p32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    check(_lib.lib().sbv2_debug_assist_blend(int(device), F.ctypes.data_as(f32p), Cn, ld, p32(m), p32(r), m.size, st.size, p32(st), p32(ln), to.size,
                                             p32(to), _f64p(w), mean.ctypes.data_as(f32p), out.ctypes.data_as(f32p), C.byref(stray)))
    return mean, out, stray.value, (mean.view(np.uint32), out.view(np.uint32))


class _Batch:
    """Keeps the numpy buffers of one sbv2_batch alive."""

    def __init__(self, utts, sdp_ratio, length_scale, noise_scale, noise_scale_w, noise_seed, forced, with_bert):
        self.keep = []
        cat = lambda key, dt: np.ascontiguousarray(np.concatenate([np.asarray(u[key]).reshape(-1) for u in utts]), dtype=dt)
        self.t_lens = np.array([len(u["phones"]) for u in utts], np.int64)
        self.x, self.tones, self.langs = cat("phones", np.int64), cat("tones", np.int64), cat("langs", np.int64)
        self.sids = np.array([int(u.get("sid", 0)) for u in utts], np.int64)
        self.styles = np.ascontiguousarray(np.stack([np.asarray(u["style"], np.float32) for u in utts]))
        self.bert = cat("bert", np.float32) if with_bert else None
        self.forced = cat("forced_durations", np.int64) if forced else None
        p = lambda a, t: a.ctypes.data_as(t) if a is not None else None
        self.c = Sbv2Batch(len(utts), p(self.t_lens, i64p), p(self.x, i64p), p(self.tones, i64p), p(self.langs, i64p), p(self.sids, i64p),
                           p(self.styles, f32p), p(self.bert, f32p), sdp_ratio, length_scale, noise_scale, noise_scale_w, noise_seed,
                           p(self.forced, i64p))
        self.opts = None   # Sbv2UttOptions when an utterance overrides an option (set_row_options)
        self.assist = None   # Sbv2Assist when an utterance carries an assist text (set_assist)

    ROW_KEYS = ("sdp_ratio", "length_scale", "noise_scale", "noise_scale_w", "noise_seed", "noise_index")

    def set_row_options(self, utts):
        """Per-utterance options (struct sbv2_utt_options): a key of ROW_KEYS in an utterance dict wins over the batch's scalar; noise_index
        defaults to the row number.  Nothing is built when no utterance overrides anything: the run is then the scalar call."""
        if not any(k in u for u in utts for k in self.ROW_KEYS):
            return
        col = lambda key, dt, default: np.array([u.get(key, default(i)) for i, u in enumerate(utts)], dt)
        self.rows = [col(k, np.float32, lambda i, k=k: getattr(self.c, k)) for k in self.ROW_KEYS[:4]]
        self.rows.append(np.array([int(u.get("noise_seed", self.c.noise_seed)) & (2 ** 64 - 1) for u in utts], np.uint64))
        self.rows.append(col("noise_index", np.int64, lambda i: i))
        self.opts = Sbv2UttOptions(*[a.ctypes.data_as(t) for a, t in zip(self.rows, [f32p] * 4 + [C.POINTER(C.c_uint64), i64p])])


    def set_assist(self, utts):
        """Assist texts (struct sbv2_assist): an utterance dict may carry assist_ids (the token ids of a second text whose mean DeBERTa feature
        is mixed into the utterance's own) with assist_weight in [0, 1].  Equal id sequences become ONE assist text of the run.  An utterance
        without assist_ids, or with a weight of 0, has none; nothing is built when no utterance has one: the run is then the call without."""
        texts, text_of, weight = {}, [], []
        for i, u in enumerate(utts):
            ids = u.get("assist_ids")
            if ids is None:
                text_of.append(-1)
                weight.append(0.0)
                continue
            if u.get("assist_weight") is None:
                raise Sbv2Error(f"utterance {i} carries assist_ids without an assist_weight")
            ids = tuple(int(t) for t in np.asarray(ids).reshape(-1))
            w = float(u["assist_weight"])
            if not ids:
                raise Sbv2Error(f"assist_ids of utterance {i} is empty")
            if not 0.0 <= w <= 1.0:   # (a NaN fails both)
                raise Sbv2Error(f"assist_weight of utterance {i} must be in [0, 1]: {w}")
            if w == 0.0:
                text_of.append(-1)
                weight.append(0.0)
                continue
            text_of.append(texts.setdefault(ids, len(texts)))
            weight.append(w)
        if not texts:
            return
        self.assist_ids = np.ascontiguousarray(np.concatenate([np.asarray(t, np.int64) for t in texts]))
        self.assist_lens = np.array([len(t) for t in texts], np.int64)
        self.assist_of = np.array(text_of, np.int32)
        self.assist_w = np.array(weight, np.float64)
        self.assist = _lib.Sbv2Assist(len(texts), self.assist_ids.ctypes.data_as(i64p), self.assist_lens.ctypes.data_as(i64p),
                                      self.assist_of.ctypes.data_as(C.POINTER(C.c_int32)), self.assist_w.ctypes.data_as(C.POINTER(C.c_double)), 0)


def synthesize_batch(session: Session, utts, sdp_ratio=0.0, length_scale=1.0, noise_scale=0.0, noise_scale_w=0.0, noise_seed=0,
                     forced=False, fetch=True):
    """New capability: a list of utterance dicts (bert [1024,T], phones, tones, langs, style, sid[, forced_durations])
    in one call.  Returns a list of PCM arrays (or the lengths when fetch=False: PCM stays in HBM)."""
    l = _lib.lib()
    b = _Batch(utts, sdp_ratio, length_scale, noise_scale, noise_scale_w, noise_seed, forced, True)
    lens = np.zeros(len(utts), np.int64)
    check(l.sbv2_vits_synthesize_batch(session.handle, C.byref(b.c), lens.ctypes.data_as(i64p)))
    if not fetch:
        return lens
    pcm = np.empty(int(lens.sum()), np.float32)
    check(l.sbv2_vits_fetch_pcm(session.handle, pcm.ctypes.data_as(f32p), pcm.size))
    return np.split(pcm, np.cumsum(lens)[:-1])


class PinnedArray:
    """float32 numpy view of page-locked host memory from the library (sbv2_host_alloc): the destination of overlapped D2H copies."""

    def __init__(self, n: int):
        self.ptr = _lib.lib().sbv2_host_alloc(4 * max(n, 1))
        if not self.ptr:
            raise Sbv2Error(_lib.lib().sbv2_last_error().decode(errors="replace"))
        self.array = np.ctypeslib.as_array(C.cast(self.ptr, f32p), shape=(n,))

    def close(self):
        if self.ptr:
            self.array = None
            _lib.lib().sbv2_host_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def fetch_durations(session: Session, total_t: int):
    d = np.zeros(total_t, np.int64)
    lw = np.zeros(total_t, np.float32)
    check(_lib.lib().sbv2_vits_fetch_durations(session.handle, d.ctypes.data_as(i64p), lw.ctypes.data_as(f32p), total_t))
    return d, lw


def set_trace(session: Session, on: bool):
    check(_lib.lib().sbv2_vits_set_trace(session.handle, int(on)))


def get_trace(session: Session, name: str, utt: int = 0) -> np.ndarray:
    l = _lib.lib()
    r, c = C.c_int64(), C.c_int64()
    check(l.sbv2_vits_get_trace(session.handle, name.encode(), utt, None, 0, C.byref(r), C.byref(c)))
    out = np.empty((r.value, c.value), np.float32)
    check(l.sbv2_vits_get_trace(session.handle, name.encode(), utt, out.ctypes.data_as(f32p), out.size, C.byref(r), C.byref(c)))
    return out


# What a Pipeline.fetch_request result holds, by name (None: not there, or there and None)
FetchResult = namedtuple("FetchResult", "signal stats marks pitch dyn_stats token_pitch", defaults=(None,) * 4)


def _fetch_fields(marks=False, pitch=False, dynamics=False, token_pitch=False):
    """THE rule of the shape of a Pipeline.fetch_request result, from which of these four options were given: (signal, stats); then
    marks-or-None if marks or pitch was; then the filled Pitch if pitch was; then the compressor's stats-or-None if dynamics was; then the
    filled TokenPitch if token_pitch was."""
    there = (True, True, marks or pitch, pitch, dynamics, token_pitch)
    return [name for name, t in zip(FetchResult._fields, there) if t]


def fetch_result(r: FetchResult, **given) -> tuple:
    """The tuple Pipeline.fetch_request returns when the options `given` were (_fetch_fields), from its named fields."""
    return tuple(getattr(r, name) for name in _fetch_fields(**given))


def split_fetch_result(res, **given) -> FetchResult:
    """... and such a tuple taken apart again, for the same options."""
    return FetchResult(**dict(zip(_fetch_fields(**given), res, strict=True)))   # (ValueError for a tuple of another length)


class Pipeline:
    """New capability: bert::predict -> word2ph feature repeat (tts_util.rs:129-154) -> model::synthesize for a batch,
    device resident between the stages."""

    #: the run entry points this pipeline calls (orchestrator.require_assist looks for the last one before it hands over an assisted request)
    entry_points = ("sbv2_pipeline_run", "sbv2_pipeline_run_opts", "sbv2_pipeline_run_assist")

    def __init__(self, bert: Session, vits: Session):
        self.bert, self.vits = bert, vits
        self.h = C.c_void_p()
        check(_lib.lib().sbv2_pipeline_create(bert.handle, vits.handle, C.byref(self.h)))

    def prepare(self, utts, sdp_ratio=0.0, length_scale=1.0, noise_scale=0.0, noise_scale_w=0.0, noise_seed=0, forced=False):
        """Pack the host-side inputs once (outside any timed region)."""
        b = _Batch(utts, sdp_ratio, length_scale, noise_scale, noise_scale_w, noise_seed, forced, False)
        b.ids = np.ascontiguousarray(np.concatenate([np.asarray(u["input_ids"], np.int64) for u in utts]))
        b.s_lens = np.array([len(u["input_ids"]) for u in utts], np.int64)
        b.w2p = np.ascontiguousarray(np.concatenate([np.asarray(u["word2ph"], np.int64) for u in utts]))
        b.lens = np.zeros(len(utts), np.int64)
        b.set_row_options(utts)   # keys sdp_ratio / length_scale / noise_scale / noise_scale_w / noise_seed / noise_index of an utterance win
        b.set_assist(utts)        # keys assist_ids / assist_weight of an utterance: equal id sequences are one assist text of the run
        return b

    def run(self, b):
        tail = (b.ids.ctypes.data_as(i64p), b.s_lens.ctypes.data_as(i64p), b.w2p.ctypes.data_as(i64p), b.lens.ctypes.data_as(i64p))
        if b.assist is not None:   # (only then: a run without an assist is the call it always was)
            check(_lib.lib().sbv2_pipeline_run_assist(self.h, C.byref(b.c), C.byref(b.opts) if b.opts is not None else None, C.byref(b.assist), *tail))
        elif b.opts is not None:
            check(_lib.lib().sbv2_pipeline_run_opts(self.h, C.byref(b.c), C.byref(b.opts), *tail))
        else:
            check(_lib.lib().sbv2_pipeline_run(self.h, C.byref(b.c), *tail))
        b.ticket = _lib.lib().sbv2_pipeline_last_ticket(self.h)   # identifies this run's results until `depth` further runs
        return b.lens

    def wait(self, ticket: int):
        check(_lib.lib().sbv2_pipeline_wait(self.h, ticket))

    def fetch_ticket_to_device(self, ticket: int, device_ptr: int, capacity: int):
        check(_lib.lib().sbv2_pipeline_fetch_pcm_ticket(self.h, ticket, C.c_void_p(device_ptr), capacity, 1))

    def sync(self):
        check(_lib.lib().sbv2_pipeline_sync(self.h))

    def fetch(self, b, out=None):
        """PCM of the run that `b` was last submitted as (by ticket: a later run of another batch does not change what this returns;
        once the pipeline has reused that run's context the ticket is stale and the library raises).  `out`: optional preallocated
        float32 array (e.g. a view of pinned memory from `pinned_array`) of at least sum(b.lens) samples."""
        n = int(b.lens.sum())
        pcm = np.empty(n, np.float32) if out is None else out
        check(_lib.lib().sbv2_pipeline_fetch_pcm_ticket(self.h, b.ticket, pcm.ctypes.data_as(C.c_void_p), pcm.size, 0))
        return np.split(pcm[:n], np.cumsum(b.lens)[:-1])

    def _layout(self, b, place, joined_len):
        """(native lengths of the fetch's signals, place pointer, joined_len): the one place a placement is validated."""
        lens = [int(v) for v in b.lens]
        if place is None:
            return lens, None, 0
        if joined_len is None:
            raise Sbv2Error("a placement needs joined_len")
        pl, pp = _i64(place)
        if pl.shape != (len(lens),):
            raise Sbv2Error(f"place must hold one offset per utterance ({len(lens)})")
        return [int(joined_len)], pp, int(joined_len)

    def _fetch(self, symbol, sizes, dtype, b, fmt, gain, place, joined_len, nstats):
        """One formatted fetch through the C entry point `symbol`: sizes(fmt, n) bounds a signal of n native samples in `dtype` elements;
        gain: the option arguments between fmt and place.  -> (buffer, per-signal counts, stats [n, nstats] or None)."""
        native, pp, jl = self._layout(b, place, joined_len)
        dst = np.empty(max(sum(sizes(fmt, n) for n in native), 1), dtype)
        got = np.zeros(len(native), np.int64)
        stats = np.zeros((len(native), nstats), np.float64) if nstats else None
        tail = (_f64p(stats),) if nstats else ()
        check(getattr(_lib.lib(), symbol)(self.h, b.ticket, C.byref(fmt.c), *gain, pp, jl, dst.ctypes.data_as(C.c_void_p), dst.nbytes,
                                          got.ctypes.data_as(i64p), *tail))
        return dst, got, stats

    def _fetch_pcm(self, symbol, b, fmt, gain, place, joined_len, nstats=0):
        out, got, stats = self._fetch(symbol, pcm_format_length, fmt.dtype, b, fmt, gain, place, joined_len, nstats)
        signals = np.split(out[:int(got.sum())], np.cumsum(got)[:-1])
        return (signals, stats) if nstats else signals

    def _fetch_flac(self, symbol, b, fmt, gain, place, joined_len, nstats=0):
        if fmt.encoding != "s16":
            raise Sbv2Error(f"FLAC needs an s16 PcmFormat, not {fmt.encoding!r}")
        dst, got, stats = self._fetch(symbol, flac_bound, np.uint8, b, fmt, gain, place, joined_len, nstats)
        return (_split_bytes(dst, got), stats) if nstats else _split_bytes(dst, got)

    def fetch_format(self, b, fmt: PcmFormat, place=None, joined_len=None):
        """PCM of the run `b` in the output format `fmt` (resampled / normalised / quantised on the device; int16 or float32 arrays, uint8 G.711 codes).
        place None: one array per utterance.  place [n] native-sample offsets + joined_len: ONE array, the utterances laid on a silent
        timeline of joined_len native samples."""
        return self._fetch_pcm("sbv2_pipeline_fetch_pcm_format", b, fmt, (), place, joined_len)

    def fetch_loudness(self, b, fmt: PcmFormat, loudness=None, place=None, joined_len=None):
        """(signals, stats): the signals of fetch_format(b, fmt, place, joined_len), each measured (BS.1770-4 integrated loudness, 4x true
        peak) and scaled to `loudness` (a Loudness; None: measure only, the signals equal fetch_format's) on the device.  fmt must not
        normalise.  stats [n, 3]: L (LUFS) and TP (dBTP) before the gain, the applied gain G (dB)."""
        return self._fetch_pcm("sbv2_pipeline_fetch_pcm_loudness", b, fmt, (_loudness_arg(loudness),), place, joined_len, 3)

    def fetch_flac_loudness(self, b, fmt: PcmFormat, loudness=None, place=None, joined_len=None):
        """(streams, stats): the signals of fetch_loudness(b, fmt, loudness, place, joined_len), each as one FLAC stream encoded on the
        device; fmt must be s16."""
        return self._fetch_flac("sbv2_pipeline_fetch_flac_loudness", b, fmt, (_loudness_arg(loudness),), place, joined_len, 3)

    def fetch_limited(self, b, fmt: PcmFormat, limiter: Limiter, place=None, joined_len=None):
        """(signals, stats): the signals of fetch_format(b, fmt, place, joined_len), each brought to limiter.target_lufs through the
        look-ahead true-peak limiter on the device.  fmt must not normalise.  stats [n, 6]: L (LUFS) and TP (dBTP) before, the pre-gain G
        (dB), L_out and TP_out of the delivered signal, the deepest gain reduction (dB, <= 0; 0 when the plain scale was enough)."""
        if limiter is None:
            raise Sbv2Error("fetch_limited needs a Limiter")
        return self._fetch_pcm("sbv2_pipeline_fetch_pcm_limited", b, fmt, (C.byref(limiter.c),), place, joined_len, 6)

    def fetch_flac_limited(self, b, fmt: PcmFormat, limiter: Limiter, place=None, joined_len=None):
        """(streams, stats): the signals of fetch_limited(b, fmt, limiter, place, joined_len), each as one FLAC stream encoded on the
        device; fmt must be s16."""
        if limiter is None:
            raise Sbv2Error("fetch_flac_limited needs a Limiter")
        return self._fetch_flac("sbv2_pipeline_fetch_flac_limited", b, fmt, (C.byref(limiter.c),), place, joined_len, 6)

    def fetch_flac(self, b, fmt: PcmFormat, place=None, joined_len=None):
        """The signals of fetch_format(b, fmt, place, joined_len), each as one FLAC stream (bytes) encoded on the device; fmt must be s16."""
        return self._fetch_flac("sbv2_pipeline_fetch_flac", b, fmt, (), place, joined_len)

    def fetch_request(self, b, rows, fmt: PcmFormat, place, joined_len, gain=None, flac=False, marks=False, env_hop=0, levels=True, pitch=None,
                      voice=None, track=None, dynamics=None, token_pitch=None, formant_scale=1.0):
        """(signal, stats): ONE signal made of the listed rows of run `b` only, row rows[k] starting at place[k] on a silent timeline of
        joined_len native samples, through the same output chain as the fetches above.  gain: None, a Loudness
        or a Limiter (stats [3] / [6], else None); flac: the s16 signal as one FLAC stream (bytes) instead of samples.  The run's PCM is only
        read: the requests that share a run are fetched one by one from the same ticket.
        Whatever is asked for, this is ONE call of sbv2_pipeline_fetch_request_formant, the widest of the C symbols, with NULL for every stage
        that is not; the shape of the result follows _fetch_fields.
        marks=True: (signal, stats, Marks): the listed rows' token spans on the delivered timeline, with
        their levels (levels=False: timing only, no kernel) and, with env_hop > 0 delivered samples, the envelope.  The signal and stats are
        those of the same call without marks.
        pitch: a Pitch -> a fourth element, that Pitch with the contour of the delivered signal; the third is
        None without marks.  Signal, stats and marks are those of the same call without pitch.
        voice: a Voice -> the listed rows are shifted on the device before the formatter; everything else,
        the returned shape included, is the same call on the shifted rows.  None or Voice(1, 1): exactly the call without.
        track: a PitchTrack -> the contours are tracked: the delivered one (pitch) and the shifter's own
        (a voice that shifts); it needs one of the two.  None: exactly the call without.
        dynamics: a Dynamics -> the compressor runs in front of `gain`, which must be given, and the
        returned tuple gains a last element: the stage's stats [3] (L of the uncompressed signal, the threshold T, the deepest compression
        in dB), or None at ratio 1, which is exactly the call without.  `stats` are then those of the compressed signal.
        token_pitch: a TokenPitch -> the listed rows' tokens are edited in the shifter, whatever the
        voice is, and the returned tuple gains a last element: that TokenPitch with applied [n] (the ratio used per token) and src_f0 [n]
        (the token's measured mean f0, 0 without a voiced frame) filled.  All zeros: the bytes of the call without.
        formant_scale: in [0.5, 2] -> the listed rows' formants are moved by that factor in the shifter's gather, whatever the voice is
        (model.Formant states it); the returned tuple is that of the call without.  1.0: exactly that call."""
        fm = None if formant_scale == 1.0 else Formant(formant_scale)   # (a NaN is carried on and refused by the library)
        if flac and fmt.encoding != "s16":
            raise Sbv2Error(f"FLAC needs an s16 PcmFormat, not {fmt.encoding!r}")
        rw = np.ascontiguousarray(np.asarray(rows, np.int32).reshape(-1))
        pl, pp = _i64(place)
        if pl.shape != rw.shape:
            raise Sbv2Error(f"place must hold one offset per listed row ({rw.size})")
        limited = isinstance(gain, Limiter)
        nstats = 0 if gain is None else 6 if limited else 3
        req = Sbv2FetchRequest(rw.ctypes.data_as(C.POINTER(C.c_int32)), rw.size, pp, int(joined_len), C.pointer(fmt.c),
                               None if gain is None or limited else C.pointer(gain.c), C.pointer(gain.c) if limited else None, int(bool(flac)))
        out_len = pcm_format_length(fmt, int(joined_len))
        dst = np.empty(max(flac_bound(fmt, int(joined_len)) if flac else out_len, 1), np.uint8 if flac else fmt.dtype)
        got = C.c_int64(0)
        stats = np.zeros(nstats, np.float64) if nstats else None
        dst_stats = None if dynamics is None or dynamics.is_identity() else np.zeros(3, np.float64)
        cp, parr = pitch.c_struct(out_len) if pitch is not None else (None, None)
        ctp, tparr = token_pitch.c_struct() if token_pitch is not None else (None, None)
        m = cm = None
        if marks:
            ntok = int(sum(int(b.t_lens[r]) for r in rw))
            nenv = -(-out_len // int(env_hop)) if env_hop > 0 else 0
            m = Marks(np.zeros(ntok, np.int64), np.zeros(ntok, np.int64), np.zeros(ntok, np.float64) if levels else None,
                      np.zeros(ntok, np.float64) if levels else None, env_hop, np.zeros(nenv, np.float64) if env_hop > 0 else None,
                      np.zeros(nenv, np.float64) if env_hop > 0 else None, out_len)
            cm = _lib.Sbv2Marks(ntok, m.start.ctypes.data_as(i64p), m.end.ctypes.data_as(i64p), _f64p(m.sumsq) if levels else None,
                                _f64p(m.peak) if levels else None, 0, int(env_hop), 0, nenv, _f64p(m.env_sumsq) if env_hop > 0 else None,
                                _f64p(m.env_peak) if env_hop > 0 else None, 0)
        ref = lambda c: C.byref(c) if c is not None else None   # (NULL for every stage not asked for; a struct is read during the call only)
        opt = lambda o: ref(o.c if o is not None else None)
        check(_lib.lib().sbv2_pipeline_fetch_request_formant(
            self.h, b.ticket, C.byref(req), opt(voice), opt(track), opt(dynamics), ref(ctp), opt(fm), dst.ctypes.data_as(C.c_void_p), dst.nbytes,
            C.byref(got), _f64p(stats) if nstats else None, _f64p(dst_stats) if dst_stats is not None else None, ref(cm), ref(cp)))
        if marks:
            assert cm.n_tokens == ntok and cm.n_env == nenv, (cm.n_tokens, ntok, cm.n_env, nenv)
        res = FetchResult(dst[:got.value].tobytes() if flac else dst[:got.value], stats, m, pitch.take(cp, parr) if pitch is not None else None,
                          dst_stats, token_pitch.take(tparr) if token_pitch is not None else None)
        return fetch_result(res, marks=bool(marks), pitch=pitch is not None, dynamics=dynamics is not None, token_pitch=token_pitch is not None)

    def close(self):
        if self.h:
            _lib.lib().sbv2_pipeline_destroy(self.h)
            self.h = None


def stream_synthesize(bert: Session, vits: Session, utt, chunk_frames=256, **kw):
    """Generator over the PCM chunks of ONE long utterance (BASELINE configs[4]): whole-sequence DeBERTa / text / flow, then the HiFi-GAN
    decoder chunk by chunk through a captured hipGraph.  Yields float32 arrays; `.info` of the generator's first item is not needed:
    use stream_open for the handle-level interface.  With fmt=PcmFormat(...) the chunks come in that format, with flac=True as well as
    the pieces (bytes, possibly empty) of one FLAC stream of those s16 samples."""
    st = StreamHandle(bert, vits, utt, chunk_frames, **kw)
    try:
        while True:
            c = st.next()
            if c is None:
                return
            yield c
    finally:
        st.close()


def stream_min_gap(fmt: PcmFormat | None) -> int:
    """The smallest gap (native samples) between two utterances of a request stream at fmt's rate: 2 ceil(half / L); 0 at 44.1 kHz (host only)."""
    n = _lib.lib().sbv2_stream_min_gap(C.byref(fmt.c) if fmt is not None else None)
    if n < 0:
        raise Sbv2Error(_lib.lib().sbv2_last_error().decode(errors="replace"))
    return int(n)


def stream_timeline(frames, gaps, hop: int, chunk_frames: int, fmt: PcmFormat | None = None):
    """(place, joined_len, call_samples): the timeline of a request stream over rows of `frames` frames with `gaps` native samples of silence
    after each (sbv2_stream_timeline; host only): where the rows lie, the length of the timeline, and the samples every call covers."""
    fr, fp = _i64(frames)
    gp_a, gp = _i64(gaps)
    n = int(fr.size)
    cap = int(sum(-(-int(f) // max(int(chunk_frames), 1)) for f in fr if f > 0)) + 1
    place, joined, calls, ncalls = np.zeros(max(n, 1), np.int64), C.c_int64(), np.zeros(cap, np.int64), C.c_int64()
    if gp_a.size != n:
        raise Sbv2Error(f"gaps must hold one entry per row ({n})")
    check(_lib.lib().sbv2_stream_timeline(fp, gp, n, int(hop), int(chunk_frames), C.byref(fmt.c) if fmt is not None else None,
                                          place.ctypes.data_as(i64p), C.byref(joined), calls.ctypes.data_as(i64p), cap, C.byref(ncalls)))
    return place[:n], joined.value, calls[:ncalls.value]


class StreamHandle:
    """utt: one utterance dict, or a LIST of them with gaps= (native samples of silence after each entry, the last one trailing): the rows of
    one batched forward delivered as one signal, sentence by sentence (sbv2_stream_begin_request; fmt None = 44.1 kHz f32; next() returns one
    piece per chunk of a row, the half gaps with a row's first and last piece; layout() tells where the rows lie, marks() covers all rows).
    fmt (PcmFormat, optional): the chunks leave the device in that format (normalize is refused: a stream cannot know the peak ahead);
    total_samples is then counted at fmt.sample_rate.  flac=True (fmt must be s16): the chunks' samples are encoded on the device as ONE FLAC
    stream; next() returns the bytes of the frames the chunk completed (b"" when it completed none: FLAC frames hold 4096 samples), the
    42-byte stream header in front of the first ones; samples_taken counts the s16 samples consumed so far.
    level (StreamLevel; needs fmt, any encoding; flac with s16 only): the samples pass a fixed gain and the look-ahead limiter on the device,
    carried from chunk to chunk.  Delivery runs stream_level_lookahead(fmt) samples behind the chunks: next() returns what the chunk
    completed (possibly an empty array or b""), the last chunk everything; samples_taken counts the chunks' samples; level_stats() after
    the end.
    levels=True / env_hop > 0 (delivered samples per envelope frame): the levels of the delivered samples per token / per frame are reduced on
    the device chunk by chunk (sbv2_stream_begin_request_levels); next_marks() hands out what the pieces taken so far completed.  A single
    utterance then runs as the request stream with gaps=[0] (the same code, the same bytes; fmt None = 44.1 kHz f32).
    pitch (a Pitch: hop, range, threshold at the stream's delivered rate; with or without levels): the pitch contour of the delivered samples is
    estimated on the device chunk by chunk as well (sbv2_stream_begin_request_pitch): n_pitch frames in all, next_pitch() hands out the ones the
    pieces taken so far completed, with the bits of debug_pitch over the whole delivered signal.
    assist: an utterance of a LIST may carry assist_ids / assist_weight (sbv2_stream_begin_request_assist, as Pipeline.run takes them); a single
    utterance dict that carries them is refused, gaps= named: a request of one row serves it.
    voice (a StreamVoice: the three scales and the pivot): the voice is shifted on the device ahead of the formatter, carried chunk by chunk
    (sbv2_stream_begin_request_voice); delivery runs stream_voice_lookahead native samples behind within a row, so next() returns what the
    chunk completed, possibly nothing, and a row's last chunk the rest; stream_voice_timeline gives the counts ahead.  A single utterance
    runs as the request stream with gaps=[0].
    leveler (a StreamLeveler; needs level): the level's gain_db becomes the starting gain of a loudness follower carried chunk by chunk
    (sbv2_stream_begin_request_leveler) in front of the level's limiter; the delivery rule is the level stream's; leveler_stats() after the
    end.  A single utterance runs as the request stream with gaps=[0]."""

    def __init__(self, bert: Session, vits: Session, utt, chunk_frames=256, fmt: PcmFormat | None = None, flac: bool = False,
                 level: "StreamLevel | None" = None, gaps=None, levels: bool = False, env_hop: int = 0, pitch: "Pitch | None" = None, track=None,
                 voice: "StreamVoice | None" = None, token_pitch=None, leveler: "StreamLeveler | None" = None, **kw):
        if leveler is not None and not hasattr(_lib.lib(), "sbv2_stream_begin_request_leveler"):
            raise Sbv2Error("this library has no sbv2_stream_begin_request_leveler: a stream cannot follow a loudness target (it is never served "
                            "unlevelled)")
        if leveler is not None and level is None:
            raise Sbv2Error("a stream leveler needs level=StreamLevel(gain_db, true_peak_max): the starting gain and the ceiling")
        if token_pitch is not None:
            raise Sbv2Error("a stream takes no token_pitch: a token's mean f0 needs all of the token's frames and the row's mean, and a stream hands "
                            "its samples out before they exist; fetch the whole signal instead (Pipeline.fetch_request(token_pitch=), /synthesize, "
                            "/synthesize_marks)")
        if voice is not None and not hasattr(_lib.lib(), "sbv2_stream_begin_request_voice"):
            raise Sbv2Error("this library has no sbv2_stream_begin_request_voice: a stream cannot shift the voice (it is never served unshifted)")
        if track is not None:
            raise Sbv2Error("a stream's contour is not tracked: one best path needs every frame of the signal, and a stream hands its frames out "
                            "as they complete; fetch the whole signal instead (Pipeline.fetch_request(track=), /synthesize, /synthesize_marks)")
        l = _lib.lib()
        self.request = isinstance(utt, (list, tuple))
        self.levels, self.env_hop, self.n_tokens, self.n_env, self._marks_buf = bool(levels), int(env_hop), 0, 0, None
        self.pitch, self.n_pitch, self._pitch_buf = pitch, 0, None
        self.voice, self.leveler = voice, leveler
        if (self.levels or self.env_hop or pitch is not None or voice is not None or leveler is not None) and not self.request:
            if gaps is not None:
                raise Sbv2Error("gaps= belongs to a stream over a list of utterances")
            utt, gaps, self.request = [utt], [0], True
        self.b = Pipeline.prepare(None, list(utt) if self.request else [utt], **kw)
        self.h = C.c_void_p()
        self.fmt, self.flac, self.level, self.samples_taken = fmt, bool(flac), level, 0
        if flac and fmt is None:
            raise Sbv2Error("a FLAC stream needs a format: fmt=PcmFormat(rate, \"s16\")")
        tot = C.c_int64()
        args = (bert.handle, vits.handle, C.byref(self.b.c), self.b.ids.ctypes.data_as(i64p), self.b.s_lens.ctypes.data_as(i64p),
                self.b.w2p.ctypes.data_as(i64p), chunk_frames)
        if self.request:
            # the rows of ONE batched forward as one signal (sbv2_stream_begin_request): always a formatted stream, fmt None = the identity format
            if gaps is None:
                raise Sbv2Error("a stream over several utterances needs gaps= (native samples of silence after each, the last one trailing)")
            self.gaps, gp = _i64(gaps)
            if self.gaps.shape != (len(utt),):
                raise Sbv2Error(f"gaps must hold one entry per utterance ({len(utt)})")
            rq = _lib.Sbv2StreamRequest(gp, C.pointer(fmt.c) if fmt is not None else None, C.pointer(level.c) if level is not None else None,
                                        int(self.flac), 0)
            opts = C.byref(self.b.opts) if self.b.opts is not None else None
            if self.b.assist is not None or voice is not None or leveler is not None:
                # an assisted row, a shifted voice or a leveler: the one entry that takes them, with the levels and the pitch the stream may carry (NULL: without)
                on = self.levels or self.env_hop
                lv = _lib.Sbv2StreamLevels(int(self.levels), self.env_hop, (C.c_int32 * 2)(0, 0)) if on or pitch is not None else None
                sp = None
                if pitch is not None:
                    sp = _lib.Sbv2StreamPitch(pitch.hop if -2 ** 31 <= pitch.hop < 2 ** 31 else 0, 0, pitch.f0_min, pitch.f0_max, pitch.threshold)
                nt, ne, nq = C.c_int64(), C.c_int64(), C.c_int64()
                head = (args[0], args[1], args[2], opts, C.byref(self.b.assist) if self.b.assist is not None else None, *args[3:], C.byref(rq),
                        C.byref(lv) if lv is not None else None, C.byref(sp) if sp is not None else None)
                tail = (C.byref(self.h), C.byref(tot), C.byref(nt), C.byref(ne), C.byref(nq))
                cv, _keep = voice.c_struct(len(utt)) if voice is not None else (None, None)
                if leveler is not None:
                    check(l.sbv2_stream_begin_request_leveler(*head, C.byref(cv) if cv is not None else None, C.byref(leveler.c), *tail))
                elif voice is not None:
                    check(l.sbv2_stream_begin_request_voice(*head, C.byref(cv), *tail))
                else:
                    check(l.sbv2_stream_begin_request_assist(*head, *tail))
                self.n_tokens, self.n_env, self.n_pitch = nt.value, ne.value, nq.value
            elif pitch is not None:
                lv, nt, ne, nq = _lib.Sbv2StreamLevels(int(self.levels), self.env_hop, (C.c_int32 * 2)(0, 0)), C.c_int64(), C.c_int64(), C.c_int64()
                sp = _lib.Sbv2StreamPitch(pitch.hop if -2 ** 31 <= pitch.hop < 2 ** 31 else 0, 0, pitch.f0_min, pitch.f0_max, pitch.threshold)
                check(l.sbv2_stream_begin_request_pitch(args[0], args[1], args[2], opts, *args[3:], C.byref(rq), C.byref(lv), C.byref(sp),
                                                        C.byref(self.h), C.byref(tot), C.byref(nt), C.byref(ne), C.byref(nq)))
                self.n_tokens, self.n_env, self.n_pitch = nt.value, ne.value, nq.value
            elif self.levels or self.env_hop:
                lv, nt, ne = _lib.Sbv2StreamLevels(int(self.levels), self.env_hop, (C.c_int32 * 2)(0, 0)), C.c_int64(), C.c_int64()
                check(l.sbv2_stream_begin_request_levels(args[0], args[1], args[2], opts, *args[3:], C.byref(rq), C.byref(lv), C.byref(self.h),
                                                         C.byref(tot), C.byref(nt), C.byref(ne)))
                self.n_tokens, self.n_env = nt.value, ne.value
            else:
                check(l.sbv2_stream_begin_request(args[0], args[1], args[2], opts, *args[3:], C.byref(rq), C.byref(self.h), C.byref(tot)))
            if fmt is None:
                self.fmt = PcmFormat(44100, "f32")
            self.buf = np.empty(max(int(l.sbv2_stream_call_bound(self.h)), 1), np.uint8)
            self.total_samples = tot.value
            self.uses_graph = bool(l.sbv2_stream_uses_graph(self.h))
            self.workspace_bytes = l.sbv2_stream_workspace_bytes(self.h)
            return
        if gaps is not None:
            raise Sbv2Error("gaps= belongs to a stream over a list of utterances")
        if self.b.assist is not None:
            raise Sbv2Error("a single-utterance stream cannot carry an assist text: stream it as a request of one row, "
                            "StreamHandle(bert, vits, [utt], gaps=[0])")
        if level is not None and fmt is None:
            raise Sbv2Error("a level stream needs a format: fmt=PcmFormat(rate, encoding), any encoding")
        if fmt is None:
            check(l.sbv2_stream_begin(*args, C.byref(self.h), C.byref(tot)))
            self.buf = np.empty(chunk_frames * l.sbv2_vits_hop(vits.handle), np.float32)
        elif level is not None:
            check(l.sbv2_stream_begin_level(*args, C.byref(fmt.c), C.byref(level.c), int(self.flac), C.byref(self.h), C.byref(tot)))
            self.buf = np.empty(stream_level_bound(fmt, chunk_frames * l.sbv2_vits_hop(vits.handle), self.flac), np.uint8)
        elif flac:
            check(l.sbv2_stream_begin_flac(*args, C.byref(fmt.c), C.byref(self.h), C.byref(tot)))
            self.buf = np.empty(flac_stream_bound(fmt, chunk_frames * l.sbv2_vits_hop(vits.handle)), np.uint8)
        else:
            check(l.sbv2_stream_begin_format(*args, C.byref(fmt.c), C.byref(self.h), C.byref(tot)))
            self.buf = np.empty(pcm_format_length(fmt, chunk_frames * l.sbv2_vits_hop(vits.handle)) + 1, fmt.dtype)
        self.total_samples = tot.value
        self.uses_graph = bool(l.sbv2_stream_uses_graph(self.h))
        self.workspace_bytes = l.sbv2_stream_workspace_bytes(self.h)

    def next(self):
        n = C.c_int64()
        if self.level is not None or self.voice is not None:   # (delivery runs behind the chunks: what the call delivers, what it consumed)
            out = C.c_int64()
            check(_lib.lib().sbv2_stream_next_level(self.h, self.buf.ctypes.data_as(C.c_void_p), self.buf.nbytes, C.byref(out), C.byref(n)))
            self.samples_taken += n.value
            if n.value == 0:
                return None
            return self.buf[:out.value].tobytes() if self.flac else self.buf[:out.value * np.dtype(self.fmt.dtype).itemsize].view(self.fmt.dtype).copy()
        if self.flac:
            nb = C.c_int64()
            check(_lib.lib().sbv2_stream_next_flac(self.h, self.buf.ctypes.data_as(C.c_void_p), self.buf.nbytes, C.byref(nb), C.byref(n)))
            self.samples_taken += n.value
            return None if n.value == 0 else self.buf[:nb.value].tobytes()
        if self.fmt is None:
            check(_lib.lib().sbv2_stream_next(self.h, self.buf.ctypes.data_as(C.c_void_p), self.buf.size, C.byref(n)))
        else:
            check(_lib.lib().sbv2_stream_next_format(self.h, self.buf.ctypes.data_as(C.c_void_p), self.buf.nbytes, C.byref(n)))
        if self.request:   # (the request stream's buffer is sized in bytes: sbv2_stream_call_bound)
            return None if n.value == 0 else self.buf[:n.value * np.dtype(self.fmt.dtype).itemsize].view(self.fmt.dtype).copy()
        return None if n.value == 0 else self.buf[:n.value].copy()

    def level_stats(self):
        """(deepest reduction in dB, max |x|) of a level stream, once next() has returned None or the last chunk (sbv2_stream_level_stats)."""
        st = np.zeros(2, np.float64)
        check(_lib.lib().sbv2_stream_level_stats(self.h, _f64p(st)))
        return float(st[0]), float(st[1])

    def leveler_stats(self):
        """(L_in LUFS, last g, min g, max g in dB, deepest reduction in dB, max |x|) of a levelled stream, once next() has returned None or the
        last chunk (sbv2_stream_leveler_stats)."""
        st = np.zeros(6, np.float64)
        check(_lib.lib().sbv2_stream_leveler_stats(self.h, _f64p(st)))
        return tuple(float(v) for v in st)

    def next_marks(self):
        """(tok_first, sumsq, peak, env_first, env_sumsq, env_peak, delivered): the levels that the pieces taken since the previous call completed
        (sbv2_stream_next_marks; host only).  Tokens [tok_first, tok_first + len(sumsq)) in the numbering of marks(), frames likewise; delivered =
        the samples the stream has handed out so far.  Refused on a stream begun without levels=True / env_hop."""
        if self._marks_buf is None:   # (sized for the whole stream once: a call hands out what is pending, at most everything)
            self._marks_buf = [np.zeros(max(n, 1), np.float64) for n in (self.n_tokens, self.n_tokens, self.n_env, self.n_env)]
        ts, tp, es, ep = self._marks_buf
        part = _lib.Sbv2StreamMarksPart(self.n_tokens, _f64p(ts), _f64p(tp), 0, 0, self.n_env, _f64p(es), _f64p(ep), 0, 0, 0)
        check(_lib.lib().sbv2_stream_next_marks(self.h, C.byref(part)))
        return (int(part.tok_first), ts[:part.n_tok].copy(), tp[:part.n_tok].copy(), int(part.env_first), es[:part.n_env].copy(),
                ep[:part.n_env].copy(), int(part.delivered))

    def next_pitch(self):
        """(first, f0, ap, lag, delivered): the frames of the pitch contour that the pieces taken since the previous call completed
        (sbv2_stream_next_pitch; host only; the rule: stream_pitch_complete).  Frames [first, first + len(f0)); f0 in Hz, 0 for an unvoiced
        frame.  Refused on a stream begun without pitch=."""
        if self._pitch_buf is None:   # (sized for the whole stream once)
            n = max(self.n_pitch, 1)
            self._pitch_buf = np.zeros(n, np.float64), np.zeros(n, np.float64), np.zeros(n, np.int32)
        f0, ap, lag = self._pitch_buf
        part = _lib.Sbv2StreamPitchPart(self.n_pitch, _f64p(f0), _f64p(ap), lag.ctypes.data_as(C.POINTER(C.c_int32)), 0, 0, 0)
        check(_lib.lib().sbv2_stream_next_pitch(self.h, C.byref(part)))
        return int(part.first), f0[:part.n].copy(), ap[:part.n].copy(), lag[:part.n].copy(), int(part.delivered)

    def marks(self):
        """(start, end): the spans of the utterance's tokens in delivered samples of this stream (sbv2_stream_marks; host only, complete from
        the moment the stream exists).  The levels come piece by piece: next_marks()."""
        n = int(np.asarray(self.b.t_lens).sum())   # (a request stream: the tokens of all rows, row after row)
        st, en, got = np.zeros(n, np.int64), np.zeros(n, np.int64), C.c_int64()
        check(_lib.lib().sbv2_stream_marks(self.h, st.ctypes.data_as(i64p), en.ctypes.data_as(i64p), n, C.byref(got)))
        return st[:got.value], en[:got.value]

    def layout(self):
        """(place, lens, joined_len) in native samples: where the stream's rows lie on its timeline (sbv2_stream_layout; host only)."""
        n = len(self.b.t_lens)
        place, lens, got, joined = np.zeros(n, np.int64), np.zeros(n, np.int64), C.c_int64(), C.c_int64()
        check(_lib.lib().sbv2_stream_layout(self.h, place.ctypes.data_as(i64p), lens.ctypes.data_as(i64p), n, C.byref(got), C.byref(joined)))
        return place[:got.value], lens[:got.value], joined.value

    def close(self):
        if self.h:
            _lib.lib().sbv2_stream_end(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def deal(costs, world: int) -> np.ndarray:
    """rank_of[i] for every utterance: the library's longest-processing-time-first deal (csrc/node.cpp; host only)."""
    c = np.ascontiguousarray(costs, np.int64)
    out = np.zeros(len(c), np.int32)
    check(_lib.lib().sbv2_deal(len(c), c.ctypes.data_as(i64p), world, out.ctypes.data_as(C.POINTER(C.c_int32))))
    return out


class Node:
    """One process, N devices: utterance-sharded synthesis with the PCM gathered to device 0 inside the library."""

    def __init__(self, bert_bytes: bytes, vits_bytes: bytes, devices):
        self.h = C.c_void_p()
        dv = (C.c_int * len(devices))(*devices)
        bb = (C.c_char * len(bert_bytes)).from_buffer_copy(bert_bytes)
        vb = (C.c_char * len(vits_bytes)).from_buffer_copy(vits_bytes)
        check(_lib.lib().sbv2_node_create(C.cast(bb, C.c_void_p), len(bert_bytes), C.cast(vb, C.c_void_p), len(vits_bytes), dv, len(devices),
                                          C.byref(self.h)))

    def prepare(self, utts, **kw):
        return Pipeline.prepare(self, utts, **kw)

    def synthesize(self, b, out=None):
        """Runs the prepared batch; returns the list of PCM arrays in the caller's utterance order."""
        l = _lib.lib()
        grow = out is None
        if grow:
            # capacity: exact when durations are forced (hop = 512 for every JP-Extra checkpoint; a larger hop shows up as a capacity error and
            # is retried below); with predicted durations ~8 frames per text symbol, grown on demand (the library refuses, it never overflows)
            cap = int(b.forced.sum()) * 512 if b.forced is not None else int(b.t_lens.sum()) * 512 * 8
            out = np.empty(max(cap, 1), np.float32)
        for _ in range(4):
            rc = l.sbv2_node_synthesize(self.h, C.byref(b.c), b.ids.ctypes.data_as(i64p), b.s_lens.ctypes.data_as(i64p), b.w2p.ctypes.data_as(i64p),
                                        b.lens.ctypes.data_as(i64p), out.ctypes.data_as(C.c_void_p), out.size)
            if rc == 0 or not grow or b"too small" not in l.sbv2_last_error():
                break
            out = np.empty(out.size * 4, np.float32)     # the shards are synthesised again: a rare path (unusually slow speech)
        check(rc)
        n = int(b.lens.sum())
        return np.split(out[:n], np.cumsum(b.lens)[:-1])

    def last_deal(self, n: int) -> np.ndarray:
        r = np.zeros(n, np.int32)
        check(_lib.lib().sbv2_node_last_deal(self.h, r.ctypes.data_as(C.POINTER(C.c_int32)), n))
        return r

    @property
    def uses_rccl(self) -> bool:
        return bool(_lib.lib().sbv2_node_uses_rccl(self.h))

    def close(self):
        if self.h:
            _lib.lib().sbv2_node_destroy(self.h)
            self.h = None


class Comm:
    """One process per GPU: the RCCL communicator of the library (no torch).  Rank 0 creates the id, the launcher distributes it."""

    @staticmethod
    def unique_id() -> bytes:
        buf = C.create_string_buffer(128)
        check(_lib.lib().sbv2_comm_unique_id(buf))
        return buf.raw

    def __init__(self, uid: bytes, rank: int, world: int, device: int):
        self.h = C.c_void_p()
        self.rank, self.world = rank, world
        check(_lib.lib().sbv2_comm_create(uid, rank, world, device, C.byref(self.h)))

    def barrier(self):
        check(_lib.lib().sbv2_comm_barrier(self.h))

    def max(self, v: float) -> float:
        d = C.c_double(v)
        check(_lib.lib().sbv2_comm_max_f64(self.h, C.byref(d)))
        return d.value

    def gather_pcm(self, pipe: Pipeline, ticket: int, dst: np.ndarray | None, root: int = 0) -> np.ndarray:
        """counts[world]; on the root `dst` (float32, possibly a PinnedArray view) receives the ranks' PCM in rank order."""
        counts = np.zeros(self.world, np.int64)
        check(_lib.lib().sbv2_comm_gather_pcm(self.h, pipe.h, ticket, root, dst.ctypes.data_as(C.c_void_p) if dst is not None else None,
                                              dst.size if dst is not None else 0, counts.ctypes.data_as(i64p)))
        return counts

    def close(self):
        if self.h:
            _lib.lib().sbv2_comm_destroy(self.h)
            self.h = None
