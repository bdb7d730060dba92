"""Host-side mirror of the reference's per-request orchestration around the hot path.

Reference behaviour restated here (crates/sbv2_core/src):
  style.rs:11-17    load_style          {"shape": [n, 256], "data": [[...], ...]} JSON -> [n, 256] f32
  style.rs:19-28    get_style_vector    mean + (style_vectors[style_id] - mean) * weight, mean = row 0
  tts.rs:280-349    easy_synthesize     split on '\\n', skip empty lines, synthesize each sentence with noise_scale 0.677 and
                                        noise_scale_w 0.8, append 22050 zero samples after every sentence that is not the LAST
                                        LINE of the request (empty trailing lines included in that test), concatenate
  tts_util.rs:163-180 array_to_vec      44.1 kHz mono 32-bit IEEE-float WAV through hound 3.5.1 (Cargo.lock:848)

What is different, on purpose: the sentence loop of the reference calls bert::predict and model::synthesize once per sentence;
here all sentences of a request go through ONE batched pipeline call (DeBERTa -> word2ph repeat -> VITS2, device resident), which
is where the MI355X path gets its throughput.  Every sentence's PCM equals its batch-1 result bit for bit (packed-batch design,
tests/test_gpu_parity.py), so the WAV is the same as the sequential loop's given the same noise seeds.

The text front-end (G2P, tokenizer: tts_util.rs:14-155) is out of scope: callers pass per-sentence
dicts {input_ids, word2ph, phones, tones, langs} exactly as parse_text produces them, or None for an empty line.
"""
import copy
import json
import struct

import numpy as np

from . import model

SAMPLE_RATE = 44100
SENTENCE_GAP = 22050        # tts.rs:321 Array3::zeros((1, 1, 22050))
NOISE_SCALE = 0.677         # tts.rs:313 / :343
NOISE_SCALE_W = 0.8         # tts.rs:314 / :344


class SynthesizeOptions:
    """tts.rs:359-375 (same defaults).  sample_rate / encoding / normalize are new (the reference writes 44.1 kHz f32 only): when any of
    them differs from its default the request's WAV signal is resampled / normalised / quantised on the device (model.PcmFormat).
    encoding "flac": the same signal as s16, returned as a FLAC stream encoded on the device instead of a WAV.
    encoding "mulaw" / "alaw" (new): the same signal as G.711 codes, one byte per sample, encoded on the device from the s16 samples and
    returned as a WAV with format tag 7 / 6 (g711_wav); what telephony links carry, usually at sample_rate 8000.
    loudness (target LUFS) / true_peak_max (dBTP) are new as well: the signal's integrated loudness is brought to the target, capped by the
    true-peak ceiling (model.Loudness); it replaces peak normalisation, so normalize=True with a loudness is refused.  That gain is one
    scale, so a target is missed whenever the signal's peak-to-loudness ratio exceeds true_peak_max - loudness (speech: about 20 dB, which
    puts -16 and -14 LUFS out of reach under -1 dBTP).  limiter=True (new) reaches such targets with a look-ahead true-peak limiter that
    takes peaks down by at most max_reduction dB (model.Limiter); it needs a loudness target.
    envelope_hz (new; read by easy_synthesize_marks only): the speech marks carry a level envelope of sample_rate // envelope_hz delivered
    samples per frame.
    gain_db (new; read by easy_synthesize_stream only, refused everywhere else): a fixed gain in dB on a stream, with the limiter's gain curve
    holding the samples under true_peak_max (model.StreamLevel).  A stream cannot measure its loudness; the caller names the gain, for
    example target - L from the loudness stats of an earlier answer of the same voice.
    level_target (new; read by easy_synthesize_stream only, refused everywhere else) with level_range ([0, 20] dB), level_slew ((0, 20] dB/s) and
    level_hold ([1, 100] blocks): a loudness target in LUFS followed on a stream (model.StreamLeveler).  gain_db is then the STARTING gain (0
    when absent), true_peak_max the ceiling; the gain walks towards level_target - (the gated loudness of everything heard so far), and the
    iterator's `.leveler_stats` reports the loudness heard and the gain reached, so the next request of the voice can begin there.
    pitch_hz (new; easy_synthesize_marks only, refused everywhere else): the speech marks carry a pitch contour of pitch_hz frames per second
    (an integer in [1, 1000]; sample_rate // pitch_hz delivered samples per frame), estimated on the device from the delivered samples within
    [pitch_min_hz, pitch_max_hz] (model.Pitch).
    pitch_scale in [0.5, 2] / intonation_scale in [0, 2] (new; checked here): the voice is raised or lowered, its melody flattened or
    exaggerated about its mean, by a length-preserving overlap-add of the synthesized rows on the device before anything else of the output
    chain (model.Voice); whole-signal routes only (easy_synthesize, easy_synthesize_marks, the batcher), refused on streams.  The defaults
    1.0 / 1.0 are the calls and the bytes there always were.
    pitch_track (new; checked here): octave-error repair.  The contours the request uses (the marks' pitch_hz contour, the shifter's own) are
    tracked across frames on the device: one best path through every frame's candidate lags (model.PitchTrack at its defaults) instead of a
    decision per frame.  It needs pitch_hz or a pitch_scale / intonation_scale away from 1; whole-signal routes only, refused on streams (a best
    path needs the future).  pitch_hz counts on the routes that carry a contour only: without marks (easy_synthesize, /synthesize, the batcher
    without marks) pitch_hz itself is refused, with or without pitch_track, so tracking is never dropped in silence; there a scale away from 1 is
    what pitch_track needs.  False is the calls and the bytes there always were.
    compressor (new; checked here) with comp_threshold (LU above the signal's own loudness, [0, 30]), comp_ratio ([1, 20]), comp_attack
    ([10, 10000] dB/s) and comp_release ([1, 1000] dB/s): a speech compressor in front of the loudness gain or the limiter (model.Dynamics),
    which evens out syllables and sentences so that a loud target comes nearer; it needs a loudness target, as limiter does.  Whole-signal
    routes only (easy_synthesize, easy_synthesize_marks, the batcher), refused on streams.  False is the calls and the bytes there always were.
    token_pitch (new; checked here) with token_pitch_kind ("hz" | "ratio") and token_pitch_smooth ([0, 20] contour frames): one value per token
    of the request's live sentences, in the order of the speech marks; 0 leaves the token alone, "hz" asks for that mean f0 of the token
    (within [35, 1200] Hz: the shifter's clamp at its default range), "ratio" multiplies its f0 (within [0.5, 2]); the edit is made by the
    shifter of pitch_scale on the device (model.TokenPitch) and composes with the two scales.  A list of another length than the request's token
    count is refused with the expected count (TokenPitchError), before any GPU work.  Whole-signal routes only, refused on streams.  The marks
    then carry "pitch_edit": {"applied", "src_f0_hz"}.  None, or all zeros, is the calls and the bytes there always were.
    formant_scale in [0.5, 2] (new; checked here): the voice's formants are moved by that factor, which changes the perceived size, age and
    character of the speaker and leaves f0, the length and the token spans alone; it is made by the shifter of pitch_scale on the device
    (model.Formant: every grain is read at the scaled offset) and composes with pitch_scale, intonation_scale, pitch_track and token_pitch.
    The level drops somewhat (set loudness to restore it).  Whole-signal routes only, refused on streams.  The marks then carry
    "formant_scale".  1.0 is the calls and the bytes there always were.
    assist (new; checked here) with assist_weight in [0, 1]: upstream Style-Bert-VITS2's assist_text / assist_text_weight.  assist is a second
    text, parsed (a sentence dict, of which only input_ids is read) or as a list of token ids (a str is taken by a holder only, which parses it
    with its parse_text); it goes through the same DeBERTa in the same
    run, and the mean of its features is mixed into every token's feature of every sentence of the request, feature * (1 - w) + mean * w, on
    the device (model._Batch.set_assist, sbv2_assist): it steers HOW the text is spoken (towards "I am so happy!") and leaves the style vector
    alone.  0.7 is this layer's default, chosen to match upstream's.  It acts before the model, so every route takes it, streams included.
    None, or a weight of 0, is the calls and the bytes there always were."""

    def __init__(self, sdp_ratio=0.0, length_scale=1.0, style_weight=1.0, split_sentences=True, sample_rate=SAMPLE_RATE, encoding="f32",
                 normalize=False, loudness=None, true_peak_max=-1.0, limiter=False, max_reduction=6.0, envelope_hz=None, gain_db=None,
                 pitch_hz=None, pitch_min_hz=70.0, pitch_max_hz=600.0, pitch_scale=1.0, intonation_scale=1.0, pitch_track=False,
                 compressor=False, comp_threshold=8.0, comp_ratio=4.0, comp_attack=600.0, comp_release=60.0, token_pitch=None, token_pitch_kind="hz",
                 token_pitch_smooth=2, formant_scale=1.0, assist=None, assist_weight=0.7, voice_pivot_hz=None, level_target=None,
                 level_range=12.0, level_slew=3.0, level_hold=10):
        self.voice_pivot_hz = check_voice_pivot(voice_pivot_hz)
        self.level_target, self.level_range, self.level_slew, self.level_hold = level_target, level_range, level_slew, level_hold
        if level_target is not None:
            stream_leveler_options(self)   # the ranges, by model.StreamLeveler
        # (a str is a text still to be parsed: holder.TTSModelHolder does that with its parse_text; the routes below refuse it as it is)
        self.assist_text = assist if isinstance(assist, str) and assist else None
        self.assist_ids, self.assist_weight = check_assist(None if isinstance(assist, str) else assist, assist_weight)
        if isinstance(formant_scale, bool) or not isinstance(formant_scale, (int, float)) or not 0.5 <= formant_scale <= 2.0:   # (a NaN fails)
            raise model.Sbv2Error(f"formant_scale must be a number in [0.5, 2.0]: {formant_scale!r}")
        self.formant_scale = float(formant_scale)
        self.token_pitch, self.token_pitch_kind, self.token_pitch_smooth = check_token_pitch(token_pitch, token_pitch_kind, token_pitch_smooth)
        if not isinstance(compressor, bool):
            raise model.Sbv2Error(f"compressor must be true or false: {compressor!r}")
        for name, v in (("comp_threshold", comp_threshold), ("comp_ratio", comp_ratio), ("comp_attack", comp_attack), ("comp_release", comp_release)):
            if isinstance(v, bool) or not isinstance(v, (int, float)):
                raise model.Sbv2Error(f"{name} must be a number: {v!r}")
        if compressor and loudness is None:
            raise model.Sbv2Error("compressor needs a loudness target: set loudness (LUFS); without make-up it only makes the signal quieter")
        self.compressor = compressor
        self.comp_threshold, self.comp_ratio, self.comp_attack, self.comp_release = comp_threshold, comp_ratio, comp_attack, comp_release
        if compressor:
            dynamics_options(self)   # the ranges, by model.Dynamics
        for name, v, lo, hi in (("pitch_scale", pitch_scale, 0.5, 2.0), ("intonation_scale", intonation_scale, 0.0, 2.0)):
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not lo <= v <= hi:   # (a NaN fails the comparison)
                raise model.Sbv2Error(f"{name} must be a number in [{lo}, {hi}]: {v!r}")
        self.pitch_scale, self.intonation_scale = float(pitch_scale), float(intonation_scale)
        if not isinstance(pitch_track, bool):
            raise model.Sbv2Error(f"pitch_track must be true or false: {pitch_track!r}")
        if (pitch_track and pitch_hz is None and self.pitch_scale == 1.0 and self.intonation_scale == 1.0 and not edits_tokens(self)
                and self.formant_scale == 1.0):
            raise model.Sbv2Error("pitch_track tracks a pitch contour: it needs pitch_hz (the marks' contour) or a pitch_scale / intonation_scale "
                                  "away from 1 (the shifter's)")
        self.pitch_track = pitch_track
        if loudness is not None and normalize:
            raise model.Sbv2Error("normalize (peak) and loudness are exclusive: choose one")
        if limiter and loudness is None:
            raise model.Sbv2Error("limiter needs a loudness target: set loudness (LUFS)")
        self.limiter, self.max_reduction = bool(limiter), max_reduction
        self.sdp_ratio, self.length_scale, self.style_weight, self.split_sentences = sdp_ratio, length_scale, style_weight, split_sentences
        self.sample_rate, self.encoding, self.normalize = sample_rate, encoding, normalize
        self.loudness, self.true_peak_max = loudness, true_peak_max
        self.envelope_hz = envelope_hz
        self.gain_db = gain_db
        self.pitch_hz, self.pitch_min_hz, self.pitch_max_hz = pitch_hz, pitch_min_hz, pitch_max_hz


def stream_leveler_options(options):
    """The model.StreamLeveler of a request's options, or None without a level_target (options of an older shape have none)."""
    if getattr(options, "level_target", None) is None:
        return None
    for name in ("level_target", "level_range", "level_slew"):
        v = getattr(options, name)
        if isinstance(v, bool) or not isinstance(v, (int, float)):
            raise model.Sbv2Error(f"{name} must be a number: {v!r}")
    return model.StreamLeveler(options.level_target, options.level_range, options.level_slew, options.level_hold)


def refuse_level_target(options, where):
    if getattr(options, "level_target", None) is not None:
        raise model.Sbv2Error(f"level_target is the loudness follower of a stream (/synthesize_stream), not of {where}: a whole signal is measured, "
                              "set loudness (LUFS) instead")


def check_voice_pivot(pivot):
    """voice_pivot_hz of a request: None, or the f0 in Hz that intonation_scale pivots about on a STREAM in place of the mean a stream cannot
    know (model.StreamVoice): one number for every sentence or a list with one per live sentence, each finite and in [70, 600], the shifter's
    range.  It is what opens pitch_scale / intonation_scale / formant_scale on the stream routes; the whole-signal routes refuse it.  Returns
    None, a float or a list of floats."""
    if pivot is None:
        return None
    many = isinstance(pivot, (list, tuple))
    values = list(pivot) if many else [pivot]
    if many and not values:
        raise model.Sbv2Error("voice_pivot_hz must be a number or a non-empty list of numbers (Hz)")
    for v in values:
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not 70.0 <= v <= 600.0:   # (a NaN fails the comparison)
            raise model.Sbv2Error(f"voice_pivot_hz must be finite and in [70, 600] Hz (the shifter's f0 range): {v!r}")
    return [float(v) for v in values] if many else float(pivot)


def refuse_voice_pivot(options, what: str):
    """voice_pivot_hz where a whole signal is shifted: refused, the row's own mean f0 is the pivot there; the stream routes take it."""
    if getattr(options, "voice_pivot_hz", None) is not None:
        raise model.Sbv2Error(f"voice_pivot_hz names the pivot of a STREAM's intonation_scale: {what} shifts a whole signal about its own mean f0; "
                              "leave it out here, or ask /synthesize_stream, /synthesize_stream_marks (easy_synthesize_stream)")


def stream_voice_options(options, rows: int):
    """The model.StreamVoice of a stream request: None when no scale is away from 1 (the stream is then the call it always was, pivot or not);
    otherwise the three scales about options.voice_pivot_hz, a list holding one pivot per live sentence."""
    p, s, q = (float(getattr(options, k, 1.0)) for k in ("pitch_scale", "intonation_scale", "formant_scale"))
    if p == 1.0 and s == 1.0 and q == 1.0:
        return None
    pivot = getattr(options, "voice_pivot_hz", None)
    if isinstance(pivot, list) and len(pivot) != rows:
        raise model.Sbv2Error(f"voice_pivot_hz holds {len(pivot)} pivots, the stream has {rows} sentence(s): name one number, or one per live sentence")
    return model.StreamVoice(p, s, q, pivot)


def check_assist(assist, weight):
    """(the assist text's token ids as a list of ints or None, the weight as a float) under the checks SynthesizeOptions states."""
    if isinstance(weight, (bool, np.bool_)) or not isinstance(weight, (int, float, np.integer, np.floating)) or not 0.0 <= weight <= 1.0:   # (a NaN fails)
        raise model.Sbv2Error(f"assist_weight must be a number in [0, 1]: {weight!r}")
    if assist is None:
        return None, float(weight)
    ids = assist.get("input_ids") if isinstance(assist, dict) else assist
    if ids is None or isinstance(ids, (str, bytes)) or not isinstance(ids, (list, tuple, np.ndarray)):
        raise model.Sbv2Error("assist must be a parsed sentence (a dict with input_ids) or a list of token ids")
    out = []
    for t, v in enumerate(np.asarray(ids, object).reshape(-1)):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or v < 0:
            raise model.Sbv2Error(f"assist token id {t} must be an integer >= 0: {v!r}")
        out.append(int(v))
    if not out:
        raise model.Sbv2Error("assist holds no token ids")
    return out, float(weight)


def assist_options(options):
    """(token ids, weight) of a request's assist text, or None without one or at a weight of 0: the request is then the call it always was."""
    ids, w = getattr(options, "assist_ids", None), float(getattr(options, "assist_weight", 0.0))
    if ids is None and getattr(options, "assist_text", None) is not None and w != 0.0:
        raise model.Sbv2Error("the assist text is not parsed: a holder parses it with its parse_text (TTSModelHolder), or pass the parsed "
                              "sentence or its token ids as assist")
    return None if ids is None or w == 0.0 else (list(ids), w)


def parsed_assist(options, parse_text):
    """`options` with its assist text parsed by parse_text (a copy; `options` itself when there is nothing to parse or the weight is 0).  No
    front end is a refusal, as for the spoken text."""
    if getattr(options, "assist_text", None) is None or getattr(options, "assist_ids", None) is not None or options.assist_weight == 0.0:
        return options
    if parse_text is None:
        raise model.Sbv2Error("no text front end configured (parse_text): pass the assist as a parsed sentence or token ids instead")
    out = copy.copy(options)
    out.assist_ids, _ = check_assist(parse_text(options.assist_text), options.assist_weight)
    return out


def with_assist(utts, options):
    """The request's rows with its assist on every one of them (the keys model._Batch.set_assist reads); the rows as they are without one."""
    a = assist_options(options)
    return utts if a is None else [dict(u, assist_ids=a[0], assist_weight=a[1]) for u in utts]


def require_assist(pipe, options):
    """A request with an assist needs a pipeline that runs sbv2_pipeline_run_assist (it says so in `entry_points`, as model.Pipeline does): any
    other is refused, not served unassisted."""
    names = getattr(pipe, "entry_points", None)
    if assist_options(options) is not None and not (isinstance(names, (tuple, list, set, frozenset)) and "sbv2_pipeline_run_assist" in names):
        raise model.Sbv2Error(f"assist needs a pipeline that runs sbv2_pipeline_run_assist: {type(pipe).__name__} does not name it in its "
                              "entry_points, and the request is not served unassisted")


class TokenPitchError(model.Sbv2Error):
    """A token_pitch the request itself is at fault for: a bad value, kind or smoothing, or a list that does not match the text's token count."""


TOKEN_PITCH_RANGES = {"hz": (35.0, 1200.0), "ratio": (0.5, 2.0)}   # the library's, at the shifter's default range of 70 .. 600 Hz


def check_token_pitch(values, kind, smooth):
    """(values as a list of floats or None, kind, smooth) under the checks SynthesizeOptions states; TokenPitchError otherwise."""
    if kind not in TOKEN_PITCH_RANGES:
        raise TokenPitchError(f"token_pitch_kind must be \"hz\" or \"ratio\": {kind!r}")
    if isinstance(smooth, bool) or not isinstance(smooth, int) or not 0 <= smooth <= 20:
        raise TokenPitchError(f"token_pitch_smooth must be an integer in [0, 20]: {smooth!r}")
    if values is None:
        return None, kind, smooth
    if isinstance(values, (str, bytes)) or not isinstance(values, (list, tuple, np.ndarray)):
        raise TokenPitchError(f"token_pitch must be a list of numbers, one per token: {values!r}")
    lo, hi = TOKEN_PITCH_RANGES[kind]
    out = []
    for t, v in enumerate(values):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) or not (v == 0 or lo <= v <= hi):   # (a NaN fails)
            raise TokenPitchError(f"token_pitch[{t}] must be 0 (not edited) or a number in [{lo}, {hi}] ({kind}): {v!r}")
        out.append(float(v))
    return out, kind, smooth


def edits_tokens(options) -> bool:
    """Whether the request edits any token (None and all zeros do not: the request is then the call it always was)."""
    v = getattr(options, "token_pitch", None)
    return v is not None and any(x != 0.0 for x in v)


def token_pitch_options(options, utts):
    """The model.TokenPitch of a request over its live sentences `utts` (None when no token is edited).  A list of another length than the
    request's token count is refused with the expected count, edited or not."""
    v = getattr(options, "token_pitch", None)
    if v is None:
        return None
    n = sum(int(np.asarray(u["phones"]).size) for u in utts)
    if len(v) != n:
        raise TokenPitchError(f"token_pitch holds {len(v)} values but the text has {n} tokens: expected {n}, one per token of the speech marks")
    if not edits_tokens(options):
        return None
    return model.TokenPitch(v, getattr(options, "token_pitch_kind", "hz"), getattr(options, "token_pitch_smooth", 2))


def refuse_token_pitch(options, what: str):
    """token_pitch where rows leave chunk by chunk: refused, with the routes that edit a whole signal."""
    if getattr(options, "token_pitch", None) is not None:
        raise TokenPitchError(f"token_pitch edits a whole signal: {what} hands out chunks before the rows are complete, ask /synthesize, "
                              "/synthesize_marks (easy_synthesize, easy_synthesize_marks) or the batcher instead")


def pitch_edit_dict(tp) -> dict:
    """The "pitch_edit" block of a marks dict from a filled model.TokenPitch: per token the ratio used and its measured mean f0 before any shift
    (None where it has no voiced frame)."""
    return {"kind": tp.kind, "smooth": int(tp.smooth), "applied": [float(v) for v in tp.applied],
            "src_f0_hz": [float(v) if v > 0 else None for v in tp.src_f0]}


def load_style(data: bytes) -> np.ndarray:
    d = json.loads(bytes(data).decode("utf-8"))
    shape = tuple(int(v) for v in d["shape"])
    flat = np.asarray([v for row in d["data"] for v in row], np.float32)
    if len(shape) != 2 or flat.size != shape[0] * shape[1]:
        raise model.Sbv2Error(f"style vectors: {flat.size} values do not fill shape {list(shape)}")   # ndarray ShapeError in the reference
    return flat.reshape(shape)


def get_style_vector(style_vectors: np.ndarray, style_id: int, weight: float) -> np.ndarray:
    sv = np.asarray(style_vectors, np.float32)
    if not 0 <= int(style_id) < sv.shape[0]:
        raise IndexError(f"style_id {style_id} out of range (the reference panics on the slice)")
    mean = sv[0]
    return (mean + (sv[int(style_id)] - mean) * np.float32(weight)).astype(np.float32)


def array_to_wav(audio: np.ndarray) -> bytes:
    """[B, 1, L] f32 -> WAV bytes.  hound writes WAVE_FORMAT_EXTENSIBLE for anything but <= 16-bit integer PCM: 40-byte fmt chunk,
    sub-format KSDATAFORMAT_SUBTYPE_IEEE_FLOAT, channel mask = the lowest `channels` bits, no fact chunk.  (Layout restated from
    the crate's documented behaviour; the crate itself is not available here, so the header bytes are unpinned.  The payload,
    sizes and rate are checked by reading the file back with an independent WAV reader in tests/.)"""
    a = np.ascontiguousarray(np.asarray(audio, np.float32))
    if a.ndim != 3:
        raise ValueError("audio must be [B, 1, L]")
    return float_wav(a[:, 0, :].reshape(-1), SAMPLE_RATE)


def _riff(fmt: bytes, data: bytes) -> bytes:
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"data" + struct.pack("<I", len(data)) + data
    return b"RIFF" + struct.pack("<I", len(body)) + body


def float_wav(samples: np.ndarray, rate: int) -> bytes:
    """Mono 32-bit float WAV at any rate, in the WAVE_FORMAT_EXTENSIBLE form of array_to_wav."""
    data = np.ascontiguousarray(samples, dtype="<f4").tobytes()
    channels, bits = 1, 32
    block = channels * bits // 8
    fmt = struct.pack("<HHIIHHHHI", 0xFFFE, channels, rate, rate * block, block, bits, 22, bits, (1 << channels) - 1)
    fmt += bytes([0x03, 0x00, 0x00, 0x00, 0x00, 0x00, 0x10, 0x00, 0x80, 0x00, 0x00, 0xAA, 0x00, 0x38, 0x9B, 0x71])
    return _riff(fmt, data)


def pcm16_wav(samples: np.ndarray, rate: int) -> bytes:
    """Mono 16-bit integer WAV at any rate: WAVE_FORMAT_PCM, 16-byte fmt chunk, 44-byte header (hound's form for <= 16-bit integer mono)."""
    data = np.ascontiguousarray(samples, dtype="<i2").tobytes()
    channels, bits = 1, 16
    block = channels * bits // 8
    return _riff(struct.pack("<HHIIHH", 0x0001, channels, rate, rate * block, block, bits), data)


G711_TAGS = {"mulaw": 7, "alaw": 6}   # WAVE_FORMAT_MULAW / WAVE_FORMAT_ALAW


def _g711_header(rate: int, encoding: str, n: int) -> bytes:
    if encoding not in G711_TAGS:
        raise model.Sbv2Error(f"unsupported G.711 encoding {encoding!r} (mulaw, alaw)")
    n = int(n)
    fmt = struct.pack("<HHIIHHH", G711_TAGS[encoding], 1, rate, rate, 1, 8, 0)   # 18 bytes: the non-PCM form, cbSize 0
    return (b"RIFF" + struct.pack("<I", 50 + n + (n & 1)) + b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt +
            b"fact" + struct.pack("<II", 4, n) + b"data" + struct.pack("<I", n))


def g711_wav(codes, rate: int, encoding: str) -> bytes:
    """Mono G.711 WAV ("mulaw": format tag 7, "alaw": 6) at any rate: the 18-byte fmt chunk of a non-PCM format (8 bits, block align 1, byte
    rate = rate, cbSize 0), a fact chunk with the sample count, then the codes; 58 bytes of header, one zero pad byte after an odd count."""
    data = np.ascontiguousarray(np.frombuffer(codes, np.uint8) if isinstance(codes, (bytes, bytearray, memoryview)) else codes, dtype=np.uint8).tobytes()
    return _g711_header(rate, encoding, len(data)) + data + b"\0" * (len(data) & 1)


def _pcm_wav(out, fmt) -> bytes:
    """The WAV of delivered samples `out` in the PcmFormat fmt."""
    if fmt.encoding in G711_TAGS:
        return g711_wav(out, fmt.sample_rate, fmt.encoding)
    return pcm16_wav(out, fmt.sample_rate) if fmt.encoding == "s16" else float_wav(out, fmt.sample_rate)


def joined_placement(lens, live_index, n_lines, split_sentences=True):
    """Offsets of the live sentences on the WAV timeline of easy_synthesize (22050 zero samples after every sentence that is not the last
    line) and the timeline's length, in native samples."""
    place, pos = [], 0
    for n, i in zip(lens, live_index):
        place.append(pos)
        pos += int(n)
        if split_sentences and i != n_lines - 1:
            pos += SENTENCE_GAP
    return place, pos


class RequestPlan:
    """Everything easy_synthesize decides about one request before the run: the output side (fmt, flac, gain) and the request's rows
    (utts: one dict per live sentence, ready for Pipeline.prepare; live: their line numbers among the request's n_lines lines)."""

    def __init__(self, sentences, style_vectors, style_id, speaker_id, options):
        options = options or SynthesizeOptions()
        refuse_voice_pivot(options, "/synthesize, /synthesize_marks (easy_synthesize, easy_synthesize_marks, the batcher)")
        if options.gain_db is not None:
            raise model.Sbv2Error("gain_db is the level control of a stream (/synthesize_stream): a whole signal is measured, set loudness (LUFS) instead")
        refuse_level_target(options, "/synthesize, /synthesize_marks (easy_synthesize, easy_synthesize_marks, the batcher)")
        if options.loudness is not None and options.normalize:
            raise model.Sbv2Error("normalize (peak) and loudness are exclusive: choose one")
        self.limited = bool(options.limiter)
        if self.limited and options.loudness is None:
            raise model.Sbv2Error("limiter needs a loudness target: set loudness (LUFS)")
        if self.limited:
            self.gain = model.Limiter(options.loudness, options.true_peak_max, options.max_reduction)
        else:
            self.gain = model.Loudness(options.loudness, options.true_peak_max) if options.loudness is not None else None
        self.dynamics = dynamics_options(options)
        if self.dynamics is not None and self.gain is None:
            raise model.Sbv2Error("compressor needs a loudness target: set loudness (LUFS); without make-up it only makes the signal quieter")
        style = get_style_vector(style_vectors, style_id, options.style_weight)
        live = [(i, s) for i, s in enumerate(sentences) if s]
        if not live:
            raise model.Sbv2Error("nothing to synthesize (the reference's concatenate fails on an empty list)")
        self.flac = options.encoding == "flac"   # a FLAC stream of the s16 signal, encoded on the device
        self.fmt = model.PcmFormat(options.sample_rate, "s16" if self.flac else options.encoding, options.normalize)
        model.pcm_format_length(self.fmt, 0)   # a bad rate is refused before any GPU work
        self.options, self.n_lines = options, len(sentences)
        self.live = [i for i, _ in live]
        self.utts = with_assist([dict(s, style=style, sid=speaker_id) for _, s in live], options)   # (the pair on every row of the request)
        self.token_pitch = token_pitch_options(options, self.utts)   # (a list of the wrong length is refused before any GPU work)


def envelope_hop(options, rate: int) -> int:
    """Delivered samples per envelope frame of a request: rate // envelope_hz, 0 without an envelope."""
    hz = getattr(options, "envelope_hz", None)
    if hz is None:
        return 0
    if not (isinstance(hz, int) and not isinstance(hz, bool) and 1 <= hz <= rate):
        raise model.Sbv2Error(f"envelope_hz must be an integer in [1, {rate}]: {hz!r}")
    return rate // hz


def pitch_options(options, rate: int):
    """The model.Pitch of a request with marks (None without pitch_hz): rate // pitch_hz delivered samples per frame.  A bad pitch_hz or
    range is refused here, before any GPU work (the range by the library's own host check)."""
    hz = getattr(options, "pitch_hz", None)
    if hz is None:
        return None
    if not (isinstance(hz, int) and not isinstance(hz, bool) and 1 <= hz <= 1000):
        raise model.Sbv2Error(f"pitch_hz must be an integer in [1, 1000]: {hz!r}")
    lo, hi = getattr(options, "pitch_min_hz", 70.0), getattr(options, "pitch_max_hz", 600.0)
    for name, v in (("pitch_min_hz", lo), ("pitch_max_hz", hi)):
        if isinstance(v, bool) or not isinstance(v, (int, float)):
            raise model.Sbv2Error(f"{name} must be a number: {v!r}")
    model.pitch_lags(rate, lo, hi)
    return model.Pitch(rate // hz, lo, hi)


def refuse_pitch(options, what: str):
    """pitch_hz where no marks are returned: refused, with the route that carries a contour."""
    if getattr(options, "pitch_hz", None) is not None:
        raise model.Sbv2Error(f"pitch_hz needs the speech marks of a whole signal: {what} carries none, ask /synthesize_marks "
                              "(easy_synthesize_marks) instead")


def voice_options(options):
    """The model.Voice of a request (None at the defaults: the request is then the call it always was)."""
    p, s = float(getattr(options, "pitch_scale", 1.0)), float(getattr(options, "intonation_scale", 1.0))
    return None if p == 1.0 and s == 1.0 else model.Voice(p, s)


def formant_options(options):
    """The formant_scale of a request (None at 1: the request is then the call it always was)."""
    q = float(getattr(options, "formant_scale", 1.0))
    return None if q == 1.0 else q


def require_formant(pipe, options):
    """A request with a formant_scale needs a pipeline whose fetch_request takes it: an older one is refused, not served unshifted."""
    if formant_options(options) is None:
        return
    import inspect
    try:
        params = inspect.signature(pipe.fetch_request).parameters
    except (AttributeError, TypeError, ValueError):   # no fetch_request, or one whose parameters cannot be read: not known to take it
        raise model.Sbv2Error(f"formant_scale needs a pipeline whose fetch_request is known to take formant_scale: that of {type(pipe).__name__} "
                              "cannot be inspected, and the request is not served with its formants unmoved")
    if "formant_scale" not in params and not any(p.kind is inspect.Parameter.VAR_KEYWORD for p in params.values()):
        raise model.Sbv2Error(f"formant_scale needs a pipeline whose fetch_request takes formant_scale: {type(pipe).__name__} does not, "
                              "and the request is not served with its formants unmoved")


def refuse_voice(options, what: str):
    """pitch_scale / intonation_scale / formant_scale where rows leave chunk by chunk, WITHOUT voice_pivot_hz: refused, with the routes that
    shift a whole signal.  With the pivot named the stream shifts them itself (stream_voice_options)."""
    if getattr(options, "voice_pivot_hz", None) is not None:
        return
    if formant_options(options) is not None:
        raise model.Sbv2Error(f"formant_scale shifts a whole signal: {what} hands out chunks before the rows are complete, ask "
                              "/synthesize, /synthesize_marks (easy_synthesize, easy_synthesize_marks) or the batcher instead, or name voice_pivot_hz")
    if voice_options(options) is not None:
        raise model.Sbv2Error(f"pitch_scale / intonation_scale shift a whole signal: {what} hands out chunks before the rows are complete, ask "
                              "/synthesize, /synthesize_marks (easy_synthesize, easy_synthesize_marks) or the batcher instead, or name voice_pivot_hz")


def track_options(options):
    """The model.PitchTrack of a request (None without pitch_track: the request is then the call it always was)."""
    return model.PitchTrack() if getattr(options, "pitch_track", False) else None


def refuse_track(options, what: str):
    """pitch_track where the signal leaves chunk by chunk: refused, with the routes that fetch a whole signal."""
    if getattr(options, "pitch_track", False):
        raise model.Sbv2Error(f"pitch_track chooses one path through all frames of a signal: {what} hands out chunks before the signal is complete, "
                              "ask /synthesize, /synthesize_marks (easy_synthesize, easy_synthesize_marks, Pipeline.fetch_request) or the batcher "
                              "instead")


def dynamics_options(options):
    """The model.Dynamics of a request (None without compressor: the request is then the call it always was)."""
    if not getattr(options, "compressor", False):
        return None
    return model.Dynamics(getattr(options, "comp_threshold", 8.0), getattr(options, "comp_ratio", 4.0), getattr(options, "comp_attack", 600.0),
                          getattr(options, "comp_release", 60.0))


def refuse_dynamics(options, what: str):
    """compressor where the signal leaves chunk by chunk: refused, with the reason and the routes that fetch a whole signal."""
    if getattr(options, "compressor", False):
        raise model.Sbv2Error(f"compressor works on a whole signal: its threshold needs the whole signal's loudness and its attack looks ahead "
                              f"without bound, and {what} hands out chunks before the signal is complete; ask /synthesize, /synthesize_marks "
                              "(easy_synthesize, easy_synthesize_marks) or the batcher instead")


def dynamics_dict(stats) -> dict:
    """The "dynamics" block of a marks dict from the compressor's three stats."""
    L, T, deepest = (float(v) for v in stats)
    return {"loudness_lufs": L if np.isfinite(L) else None, "threshold_lufs": T if np.isfinite(T) else None, "deepest_db": deepest}


def token_marks(utts, live, rate: int, start, end):
    """The timing part of the marks dict: utts = the request's live sentences (phones, word2ph), live = their line numbers, start / end = the
    delivered-sample spans of their tokens, sentence after sentence.  tokens: one entry per phone id (blanks included); words: one entry per
    word2ph entry (`index` = its position in input_ids), the union of its tokens' spans, empty at the running position when it has none."""
    tokens, words, e = [], [], 0
    sec = lambda n: int(n) / float(rate)
    for line, u in zip(live, utts):
        first = e
        for t, ph in enumerate(np.asarray(u["phones"]).reshape(-1)):
            s0, s1 = int(start[e]), int(end[e])
            tokens.append({"line": int(line), "index": t, "phone": int(ph), "start": s0, "end": s1, "start_s": sec(s0), "end_s": sec(s1)})
            e += 1
        k = first
        for w, cnt in enumerate(np.asarray(u["word2ph"]).reshape(-1)):
            cnt = int(cnt)
            if cnt > 0:
                s0, s1 = int(start[k]), int(end[k + cnt - 1])
            else:
                s0 = s1 = int(start[k]) if k < e else (int(end[e - 1]) if e > first else 0)
            words.append({"line": int(line), "index": w, "start": s0, "end": s1, "start_s": sec(s0), "end_s": sec(s1)})
            k += cnt
        if k != e:
            raise model.Sbv2Error("sum(word2ph) must equal the text length (tts_util.rs:122-127)")
    return {"sample_rate": int(rate), "tokens": tokens, "words": words}


def marks_dict(utts, live, fmt, m, pitch=None, tracked=False) -> dict:
    """The JSON-ready speech marks of one request from a model.Marks of its rows: token_marks plus, per token, level_dbfs (10 log10 of the mean
    square of its delivered samples re full scale; None for an empty or silent span) and peak (largest |sample| re full scale), and `envelope`
    {hop, level_dbfs [n], peak [n]} when the marks hold one.  The gaps between sentences belong to no token.
    pitch (a filled model.Pitch): `pitch` {hop, f0_hz [n] (None for an unvoiced frame), aperiodicity [n]}, and per token f0_hz (the mean over
    the voiced frames whose centre f hop + hop // 2 lies in its span; None when there is none) and voiced (the share of the frames centred in
    its span that are voiced; 0.0 when none is centred there).  Without pitch the dict has none of these keys.
    tracked: the contour is a tracked one (options.pitch_track): the `pitch` block says "tracked": true (the key is absent otherwise)."""
    d = token_marks(utts, live, fmt.sample_rate, m.start, m.end)
    full = model.full_scale(fmt.encoding)
    if m.sumsq is not None:
        for t, ss, pk in zip(d["tokens"], m.sumsq, m.peak):
            t["level_dbfs"] = model.level_dbfs(ss, t["end"] - t["start"], fmt.encoding)
            t["peak"] = float(pk) / full
    if m.env_hop > 0:
        n = [min(m.env_hop, m.out_len - f * m.env_hop) for f in range(len(m.env_sumsq))]   # (the last frame may be short)
        d["envelope"] = {"hop": int(m.env_hop), "level_dbfs": [model.level_dbfs(ss, k, fmt.encoding) for ss, k in zip(m.env_sumsq, n)],
                         "peak": [float(pk) / full for pk in m.env_peak]}
    if pitch is not None:
        f0 = np.asarray(pitch.f0, np.float64)
        d["pitch"] = {"hop": int(pitch.hop), "f0_hz": [float(v) if v > 0 else None for v in f0], "aperiodicity": [float(v) for v in pitch.ap]}
        if tracked:
            d["pitch"]["tracked"] = True
        token_pitch(d["tokens"], f0, pitch.hop)
    return d


def token_pitch(tokens, f0, hop: int):
    """Per token of a marks dict, from the contour f0 [n] (0 = unvoiced) of frames with their centres at f hop + hop // 2: f0_hz and voiced as
    marks_dict states them."""
    f0 = np.asarray(f0, np.float64)
    centre = np.arange(f0.size, dtype=np.int64) * hop + hop // 2
    for t in tokens:
        k0, k1 = np.searchsorted(centre, [t["start"], t["end"]])   # the frames with start <= centre < end
        v = f0[k0:k1][f0[k0:k1] > 0]
        t["f0_hz"] = float(v.mean()) if v.size else None
        t["voiced"] = float(v.size) / (k1 - k0) if k1 > k0 else 0.0


def finish_request(pipe: "model.Pipeline", b, r0: int, r1: int, plan: RequestPlan, loudness_stats=None, pcm=None, marks=None,
                   dynamics_stats=None) -> bytes:
    """The answer of one request from rows r0 .. r1 - 1 of run `b` (plan.utts were prepared as those rows): the request's WAV or FLAC bytes,
    whatever else the run holds.  pcm: the run's plain fetch (pipe.fetch(b)) when the caller already has it.
    marks: an optional list that receives the request's speech marks (marks_dict); the signal then always comes from ONE fetch of the
    request's rows with marks (at the identity format for the default output: the same samples, hence the same bytes).
    dynamics_stats: an optional list that receives the compressor's [L, T, deepest compression] when plan.dynamics compresses; the marks then
    carry them as a "dynamics" block (dynamics_dict), and loudness_stats are those of the compressed signal."""
    options, fmt, ln = plan.options, plan.fmt, plan.gain
    lens = b.lens[r0:r1]
    # every option is named only when asked for: a request at the defaults is the call it always was
    dyn, voice, tp, fq = getattr(plan, "dynamics", None), voice_options(options), getattr(plan, "token_pitch", None), formant_options(options)
    if fq is not None:
        require_formant(pipe, options)
    kw = {k: v for k, v in (("voice", voice), ("dynamics", dyn), ("token_pitch", tp), ("formant_scale", fq)) if v is not None}
    shifts = voice is not None or tp is not None or fq is not None
    if ln is not None or not fmt.is_default or marks is not None or shifts:
        # ONE fetch of the request's rows: the WAV signal below, resampled / normalised / quantised as a whole on the device; with a loudness target
        # it is measured and scaled (or limited) as a whole too (the gates leave the silent gaps out); flac: its s16 form encoded on the device
        place, joined = joined_placement(lens, plan.live, plan.n_lines, options.split_sentences)
        kw.update(gain=ln, flac=plan.flac)
        pitch = None
        if marks is not None:
            kw.update(marks=True, env_hop=envelope_hop(options, fmt.sample_rate))
            pitch = pitch_options(options, fmt.sample_rate)
            if pitch is not None:
                kw["pitch"] = pitch
        track = track_options(options)
        if track is not None and (pitch is not None or shifts):   # (it needs a contour or a shift)
            kw["track"] = track
        got = model.split_fetch_result(pipe.fetch_request(b, range(r0, r1), fmt, place, joined, **kw), marks=marks is not None,
                                       pitch=pitch is not None, dynamics=dyn is not None, token_pitch=tp is not None)
        out, stats, dstats = got.signal, got.stats, got.dyn_stats
        if marks is not None:
            marks.append(marks_dict(plan.utts, plan.live, fmt, got.marks, got.pitch, **({"tracked": True} if "track" in kw and pitch is not None else {})))
            if dstats is not None:
                marks[-1]["dynamics"] = dynamics_dict(dstats)
            if tp is not None:
                marks[-1]["pitch_edit"] = pitch_edit_dict(got.token_pitch)
            if fq is not None:
                marks[-1]["formant_scale"] = fq
        if dstats is not None and dynamics_stats is not None:
            dynamics_stats.append([float(v) for v in dstats])
        if stats is not None and loudness_stats is not None:
            loudness_stats.append([float(v) for v in stats])
        return out if plan.flac else _pcm_wav(out, fmt)
    if pcm is None:
        pcm = pipe.fetch(b)
    parts = []
    for i, wav in zip(plan.live, pcm[r0:r1]):
        parts.append(wav)
        if options.split_sentences and i != plan.n_lines - 1:
            parts.append(np.zeros(SENTENCE_GAP, np.float32))
    return array_to_wav(np.concatenate(parts).reshape(1, 1, -1))


def easy_synthesize(pipe: "model.Pipeline", sentences, style_vectors, style_id=0, speaker_id=0, options=None, noise_seed=None,
                    noise_scale=NOISE_SCALE, noise_scale_w=NOISE_SCALE_W, loudness_stats=None, dynamics_stats=None) -> bytes:
    """tts.rs:280-349 for one request whose lines are already parsed: `sentences` is the list obtained from text.split('\\n'),
    each entry a dict {input_ids, word2ph, phones, tones, langs} (parse_text's products) or None / {} for an empty line.
    With options.split_sentences False the caller passes the single parsed text as a one-element list.
    loudness_stats: an optional list that receives [L, TP, G] of the signal when options.loudness is set, or the limiter's 6 values
    [L, TP, G, L_out, TP_out, deepest reduction] when options.limiter is set as well.
    dynamics_stats: an optional list that receives the compressor's [L, T, deepest compression] when options.compressor is set; the
    loudness_stats are then those of the compressed signal.
    = finish_request over all rows of a run that holds this request alone (batcher.RequestBatcher: the same, several requests to a run)."""
    refuse_pitch(options, "easy_synthesize (/synthesize)")
    plan = RequestPlan(sentences, style_vectors, style_id, speaker_id, options)
    require_formant(pipe, plan.options)   # (before any GPU work)
    require_assist(pipe, plan.options)
    if noise_seed is None:      # the reference draws fresh noise per request; tests pass an explicit seed
        noise_seed = model.fresh_noise_seed()
    b = pipe.prepare(plan.utts, sdp_ratio=plan.options.sdp_ratio, length_scale=plan.options.length_scale, noise_scale=noise_scale,
                     noise_scale_w=noise_scale_w, noise_seed=noise_seed)
    pipe.run(b)
    return finish_request(pipe, b, 0, len(plan.utts), plan, loudness_stats, **({} if dynamics_stats is None else {"dynamics_stats": dynamics_stats}))


def easy_synthesize_marks(pipe: "model.Pipeline", sentences, style_vectors, style_id=0, speaker_id=0, options=None, noise_seed=None,
                          noise_scale=NOISE_SCALE, noise_scale_w=NOISE_SCALE_W, loudness_stats=None, dynamics_stats=None):
    """(audio_bytes, marks): easy_synthesize's bytes for the same arguments, and the speech marks of that signal (marks_dict): when each
    phone id and each word (word2ph entry) is spoken, in samples and seconds of the delivered signal, how loud it is there, and with
    options.envelope_hz a level envelope.  Levels are computed on the device from the delivered samples (also behind the FLAC sink)."""
    plan = RequestPlan(sentences, style_vectors, style_id, speaker_id, options)
    require_formant(pipe, plan.options)   # (before any GPU work)
    require_assist(pipe, plan.options)
    envelope_hop(plan.options, plan.fmt.sample_rate)   # a bad envelope_hz is refused before any GPU work
    pitch_options(plan.options, plan.fmt.sample_rate)  # ... and so is a bad pitch_hz or range
    if noise_seed is None:
        noise_seed = model.fresh_noise_seed()
    b = pipe.prepare(plan.utts, sdp_ratio=plan.options.sdp_ratio, length_scale=plan.options.length_scale, noise_scale=noise_scale,
                     noise_scale_w=noise_scale_w, noise_seed=noise_seed)
    pipe.run(b)
    got = []
    audio = finish_request(pipe, b, 0, len(plan.utts), plan, loudness_stats, marks=got,
                           **({} if dynamics_stats is None else {"dynamics_stats": dynamics_stats}))
    return audio, got[0]


def wav_stream_header(rate: int, encoding: str, n_samples: int) -> bytes:
    """The header of pcm16_wav ("s16") / float_wav ("f32") / g711_wav ("mulaw", "alaw") for a signal of n_samples whose samples follow later:
    the same bytes as the header of the finished file (after an odd number of G.711 codes the file ends with one zero pad byte)."""
    if encoding in G711_TAGS:
        return _g711_header(rate, encoding, n_samples)
    empty = pcm16_wav(np.zeros(0, np.int16), rate) if encoding == "s16" else float_wav(np.zeros(0, np.float32), rate)
    data = int(n_samples) * (2 if encoding == "s16" else 4)
    riff = struct.unpack("<I", empty[4:8])[0] + data
    return empty[:4] + struct.pack("<I", riff) + empty[8:-4] + struct.pack("<I", data)


class SynthesisStream:
    """The pieces (bytes) of one streamed answer, in order: an iterator that owns the model.StreamHandle behind it.  The handle is closed when
    the pieces run out, when one fails, by close(), and when the object is dropped, iterated or not: the replays of a stream are already
    enqueued when this object is returned, so its end cannot hang on a generator's `finally`, which never runs for a generator nobody started."""

    def __init__(self, st, head, to_bytes, marks=None, tail=None, levels=None, pitch=None):
        self._st, self._head, self._to_bytes, self._tail = st, head, to_bytes, tail   # tail: bytes that follow the last chunk (a pad byte)
        self.marks = marks   # token_marks of the utterance at the stream's rate: complete before the first piece
        self.level_stats = None   # a level stream's (deepest reduction in dB, max |x|), once its last piece has been handed out
        self.leveler_stats = None   # a levelled stream's (L_in, last g, min g, max g, deepest reduction, max |x|), likewise
        # levels=(fmt, env_hop, total_samples): the stream was begun with levels (easy_synthesize_stream(levels=True)); take_marks() hands out
        # what the pieces so far completed, and once the last piece is out `.marks` holds them all, in marks_dict's shape
        self._levels, self.delivered = levels, 0
        self.total_samples = int(getattr(st, "total_samples", 0))   # delivered samples of the whole answer
        self._new_tokens, self._new_env, self._env_first = [], ([], []), 0
        if levels is not None and levels[1] > 0:
            self.marks["envelope"] = {"hop": int(levels[1]), "level_dbfs": [], "peak": []}
        # pitch (a model.Pitch, with levels): the stream was begun with a contour; take_marks() hands out the frames the pieces so far completed
        # too, and once the last piece is out `.marks` has the "pitch" block and the tokens' f0_hz / voiced of marks_dict
        self._pitch, self._f0, self._new_pitch, self._pitch_first = pitch, [], ([], []), 0
        if pitch is not None:
            self.marks["pitch"] = {"hop": int(pitch.hop), "f0_hz": [], "aperiodicity": []}

    def _collect(self):
        """The levels the handle has completed since the last look -> `.marks` and the lists take_marks() hands out next."""
        if self._levels is None or self._st is None:
            return
        fmt, hop, total = self._levels
        full = model.full_scale(fmt.encoding)
        t0, ss, pk, f0, es, ep, self.delivered = self._st.next_marks()
        for i, (s, p) in enumerate(zip(ss, pk)):
            tok = self.marks["tokens"][t0 + i]
            tok["level_dbfs"], tok["peak"] = model.level_dbfs(s, tok["end"] - tok["start"], fmt.encoding), float(p) / full
            self._new_tokens.append({"token": t0 + i, "level_dbfs": tok["level_dbfs"], "peak": tok["peak"]})
        for i, (s, p) in enumerate(zip(es, ep)):
            db = model.level_dbfs(s, min(hop, total - (f0 + i) * hop), fmt.encoding)   # (the last frame may be short)
            for lst, v in ((self.marks["envelope"]["level_dbfs"], db), (self.marks["envelope"]["peak"], float(p) / full),
                           (self._new_env[0], db), (self._new_env[1], float(p) / full)):
                lst.append(v)
        if self._pitch is not None:
            _, f0, ap, _, _ = self._st.next_pitch()
            self._f0.extend(float(v) for v in f0)
            for lst, vals in ((self.marks["pitch"]["f0_hz"], f0), (self._new_pitch[0], f0)):
                lst.extend(float(v) if v > 0 else None for v in vals)
            for lst in (self.marks["pitch"]["aperiodicity"], self._new_pitch[1]):
                lst.extend(float(v) for v in ap)

    def take_marks(self) -> dict:
        """JSON-ready: the levels that the pieces handed out so far have completed and that no earlier call returned.  {"delivered": samples out
        so far, "tokens": [{"token": its index in .marks["tokens"], "level_dbfs", "peak"}, ...], "envelope": {"first", "hop", "level_dbfs" [n],
        "peak" [n]} (with an envelope), "pitch": {"first", "hop", "f0_hz" [n] (None = unvoiced), "aperiodicity" [n]} (with pitch)}.  A token is
        complete once its last sample has been delivered, an envelope frame likewise, a pitch frame once its window has been
        (model.stream_pitch_complete)."""
        if self._levels is None:
            raise model.Sbv2Error("this stream was begun without levels (easy_synthesize_stream(levels=True))")
        self._collect()
        d = {"delivered": int(self.delivered), "tokens": self._new_tokens}
        if self._levels[1] > 0:
            d["envelope"] = {"first": self._env_first, "hop": int(self._levels[1]), "level_dbfs": self._new_env[0], "peak": self._new_env[1]}
            self._env_first += len(self._new_env[0])
        if self._pitch is not None:
            d["pitch"] = {"first": self._pitch_first, "hop": int(self._pitch.hop), "f0_hz": self._new_pitch[0], "aperiodicity": self._new_pitch[1]}
            self._pitch_first += len(self._new_pitch[0])
        self._new_tokens, self._new_env, self._new_pitch = [], ([], []), ([], [])
        return d

    def __iter__(self):
        return self

    def __next__(self):
        if self._head is not None:
            head, self._head = self._head, None
            return head
        try:
            while self._st is not None:
                c = self._st.next()
                if c is None:
                    self._collect()     # (everything is complete now: what take_marks() has not seen yet waits for its next call)
                    if self._pitch is not None:
                        token_pitch(self.marks["tokens"], self._f0, self._pitch.hop)
                    if getattr(self._st, "level", None) is not None:
                        self.level_stats = self._st.level_stats()
                    if getattr(self._st, "leveler", None) is not None:
                        self.leveler_stats = self._st.leveler_stats()
                    st, self._st = self._st, None
                    st.close()      # the device side is done; on_close waits until the last byte has been handed out
                    break
                if len(c):
                    return self._to_bytes(c)
        except BaseException:
            self.close()
            raise
        tail, self._tail = self._tail, None
        if tail:
            return tail     # close(), and on_close with it, follows on the next call: the holder's lock is held until the last byte
        self.close()
        raise StopIteration

    on_close = None   # optional callable, run once when the stream is closed (the holder resumes the model's batcher with it)

    def close(self):
        st, self._st, self._head, self._tail = self._st, None, None, None
        try:
            if st is not None:
                st.close()
        finally:
            cb, self.on_close = self.on_close, None
            if cb is not None:
                cb()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def easy_synthesize_stream(bert, vits, sentences, style_vectors, style_id=0, speaker_id=0, options=None, noise_seed=None,
                           noise_scale=NOISE_SCALE, noise_scale_w=NOISE_SCALE_W, chunk_frames=256, split=False, levels=False, pitch=False):
    """easy_synthesize delivered while it is synthesised: an iterator (SynthesisStream; close() it when it is abandoned early) over the pieces
    of the request's container.  The forward (DeBERTa / text / flow) runs once over the whole request, then the decoder runs chunk by chunk
    (model.StreamHandle).

    split=False (the default): the stream takes ONE utterance, so `sentences` must hold one parsed text: the request's lines joined, as
    options.split_sentences = False passes them (empty entries are skipped, a second live one is refused).

    split=True: `sentences` is the request's line list as easy_synthesize takes it (None for an empty line).  The live sentences become the rows
    of ONE batched forward (the request's seed, the row number as noise key: what easy_synthesize prepares) and leave as one signal, sentence
    by sentence (a model.StreamHandle over a list): SENTENCE_GAP native samples of silence after every live sentence that is not the last
    line, joined_placement's rule.  With the same seed and options the streamed bytes are easy_synthesize's (at the default format the WAV
    headers differ in form, the samples do not).

    Either way.  encoding "flac": the pieces of one FLAC stream encoded on the device, as its frames complete (chunks that complete none
    yield nothing); "s16" / "f32": the WAV header of pcm16_wav / float_wav written with the known total length, then the chunks' samples;
    "mulaw" / "alaw": the header of g711_wav, the chunks' codes, and one zero pad byte after the last chunk when the total is odd.
    normalize, loudness and limiter are refused: they need the whole signal before the first sample can leave.
    options.gain_db: the level stream (model.StreamLevel(gain_db, true_peak_max)) for every encoding alike: a fixed gain, no sample above
    the ceiling; the pieces run stream_level_lookahead samples behind the decoder, the total length is unchanged, and after the last piece
    the iterator's `.level_stats` holds (deepest reduction in dB, max |x|).
    options.level_target (with level_range / level_slew / level_hold): the same level stream with a loudness follower in front of its limiter
    (model.StreamLeveler): gain_db is then the starting gain, 0 when absent; after the last piece `.leveler_stats` holds (L_in LUFS, last g, min
    g, max g in dB, deepest reduction in dB, max |x|).  A handle class that takes no leveler= is refused, never served unlevelled.
    Everything up to the first replay (options, DeBERTa, flow, the header) runs before the iterator is returned.
    The iterator's `.marks` holds the token and word timing of every row with its line number (token_marks: every duration is known before
    the first replay).
    levels=True: the levels of the delivered samples per token, and with options.envelope_hz per envelope frame, are reduced on the device
    chunk by chunk (model.StreamHandle(levels=True, env_hop=...)): the iterator's take_marks() returns what the pieces so far completed, and
    once the last piece is out `.marks` has marks_dict's shape.  The audio bytes are those of the same call without levels (the default,
    which ignores envelope_hz).  On a level stream (gain_db) the levels are those of the samples the limiter emits.
    pitch=True (needs levels=True and options.pitch_hz; hop and range as pitch_options reads them): the pitch contour of the delivered samples
    is estimated on the device chunk by chunk as well (model.StreamHandle(pitch=...)): take_marks() pieces gain a "pitch" block, and once the
    last piece is out `.marks` has marks_dict's "pitch" block and the tokens' f0_hz / voiced.  Without pitch=True, pitch_hz is refused.
    options.assist: every row carries the assist (sbv2_stream_begin_request_assist); with split=False the utterance then runs as a request of
    one row without a gap, the only stream kind that takes one."""
    options = options or SynthesizeOptions()
    refuse_voice(options, "a stream (/synthesize_stream, /synthesize_stream_marks)")
    refuse_token_pitch(options, "a stream (/synthesize_stream, /synthesize_stream_marks)")
    refuse_track(options, "a stream (/synthesize_stream, /synthesize_stream_marks)")
    refuse_dynamics(options, "a stream (/synthesize_stream, /synthesize_stream_marks)")
    if pitch:
        if not levels:
            raise model.Sbv2Error("pitch=True on a stream comes with its speech marks: pass levels=True as well")
        if getattr(options, "pitch_hz", None) is None:
            raise model.Sbv2Error("pitch=True needs options.pitch_hz (frames per second of the contour)")
    else:
        refuse_pitch(options, "a stream without pitch=True (/synthesize_stream)")
    if options.normalize:
        raise model.Sbv2Error("a stream cannot normalise: the peak needs the whole signal (use /synthesize)")
    if options.loudness is not None or options.limiter:
        raise model.Sbv2Error("a stream has no loudness or limiter: integrated loudness needs the whole signal (use /synthesize)")
    if noise_seed is None:
        noise_seed = model.fresh_noise_seed()
    style = get_style_vector(style_vectors, style_id, options.style_weight)
    live = [s for s in sentences if s]
    if not live:
        raise model.Sbv2Error("nothing to synthesize (the reference's concatenate fails on an empty list)")
    if not split and len(live) != 1:
        raise model.Sbv2Error(f"a stream takes one utterance, not {len(live)} sentences: pass the text parsed as a whole (split_sentences = False)")
    flac = options.encoding == "flac"
    fmt = model.PcmFormat(options.sample_rate, "s16" if flac else options.encoding, False)
    model.pcm_format_length(fmt, 0)   # a bad rate is refused before any GPU work
    # (with a level the default format is an explicit one: the level stream always formats)
    leveler = stream_leveler_options(options)
    start_db = options.gain_db if options.gain_db is not None else (0.0 if leveler is not None else None)
    level = model.StreamLevel(start_db, options.true_peak_max) if start_db is not None else None
    kw = dict(fmt=None if fmt.is_default and level is None else fmt, flac=flac, level=level, sdp_ratio=options.sdp_ratio,
              length_scale=options.length_scale, noise_scale=noise_scale, noise_scale_w=noise_scale_w, noise_seed=noise_seed)
    if levels:
        kw.update(levels=True, env_hop=envelope_hop(options, fmt.sample_rate))   # (a bad envelope_hz is refused before any GPU work)
    contour = pitch_options(options, fmt.sample_rate) if pitch else None   # (a bad pitch_hz or range likewise)
    if contour is not None:
        kw.update(pitch=contour)
    if leveler is not None:
        import inspect
        if "leveler" not in inspect.signature(model.StreamHandle.__init__).parameters:
            raise model.Sbv2Error("level_target on a stream needs a StreamHandle that takes leveler=: this one does not, and the request is not "
                                  "served unlevelled")
        kw.update(leveler=leveler)
    sv = stream_voice_options(options, len(live))   # (pitch_scale / intonation_scale / formant_scale about voice_pivot_hz: refused above without it)
    if sv is not None:
        # a handle class without the entry point is refused, never served unshifted (the formant_scale rule)
        import inspect
        params = inspect.signature(model.StreamHandle.__init__).parameters
        if "voice" not in params:
            raise model.Sbv2Error("pitch_scale / intonation_scale / formant_scale on a stream need a StreamHandle that takes voice=: this one does "
                                  "not, and the request is not served unshifted")
        kw.update(voice=sv, fmt=fmt)   # (a voice stream always formats: the identity format is an explicit one)
    if split:
        lines = [i for i, s in enumerate(sentences) if s]
        gaps = [SENTENCE_GAP if i != len(sentences) - 1 else 0 for i in lines]
        st = model.StreamHandle(bert, vits, with_assist([dict(s, style=style, sid=speaker_id) for s in live], options), chunk_frames, gaps=gaps, **kw)
    else:
        lines = [sentences.index(live[0])]
        if assist_options(options) is not None:
            # the plain single-utterance entries take no assist: the same utterance as a request of one row without a gap (the same samples)
            st = model.StreamHandle(bert, vits, with_assist([dict(live[0], style=style, sid=speaker_id)], options), chunk_frames, gaps=[0], **kw)
        else:
            st = model.StreamHandle(bert, vits, dict(live[0], style=style, sid=speaker_id), chunk_frames, **kw)
    try:
        marks = token_marks(live, lines, fmt.sample_rate, *st.marks())
    except BaseException:
        st.close()
        raise
    lv = (fmt, kw["env_hop"], st.total_samples) if levels else None
    if flac:
        return SynthesisStream(st, None, lambda c: c, marks, levels=lv, pitch=contour)
    dtype = {"s16": "<i2", "f32": "<f4"}.get(fmt.encoding, "u1")
    pad = b"\0" if fmt.encoding in G711_TAGS and st.total_samples & 1 else None
    return SynthesisStream(st, wav_stream_header(fmt.sample_rate, fmt.encoding, st.total_samples),
                           lambda c: np.ascontiguousarray(c, dtype).tobytes(), marks, tail=pad, levels=lv, pitch=contour)
