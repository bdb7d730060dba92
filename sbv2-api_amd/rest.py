"""The REST surface of crates/sbv2_api/src/main.rs over a TTSModelHolder (holder.py): same routes, request schema, defaults, content types
and error mapping, so that a client of the reference's server cannot tell the difference.

  GET  /            "Hello, World!"                                              main.rs:193
  GET  /models      JSON list of idents                                          main.rs:24-33
  POST /synthesize  {text, ident, sdp_ratio = 0.0, length_scale = 1.0, style_id = 0, speaker_id = 0} -> audio/wav     main.rs:51-100
                    (+ sample_rate = 44100, encoding = "f32" | "s16" | "flac" | "mulaw" | "alaw", normalize = false: new output formats, defaults = the
                    reference's; "flac" -> audio/flac; "mulaw" / "alaw" -> audio/wav holding G.711 codes, format tag 7 / 6; loudness = null (target LUFS), true_peak_max = -1.0 (dBTP): loudness
                    normalisation, exclusive with normalize.  The loudness gain is one scale: a target louder than the signal's
                    true_peak_max - (TP - L), about -21 LUFS for speech under -1 dBTP, is missed unless limiter = true (default false;
                    max_reduction = 6.0 dB): a look-ahead true-peak limiter that reaches it; limiter needs loudness)
  POST /synthesize_stream  new: the same request, answered while it is synthesised (chunked transfer): the text as ONE utterance (joined, as
                    split_sentences = false does), encoding "flac" -> audio/flac, one FLAC stream encoded on the device chunk by chunk;
                    "s16" / "f32" / "mulaw" / "alaw" -> audio/wav, the header written with the known length, then the chunks.  normalize / loudness / limiter
                    are refused (they need the whole signal).  gain_db = null (new): a fixed gain in dB with the limiter's look-ahead gain
                    curve holding every sample under true_peak_max, carried from chunk to chunk on the device; same length, same header;
                    the other routes refuse it.  level_target = null (new; with level_range = 12, level_slew = 3, level_hold = 10): a loudness
                    target in LUFS that a follower on the device walks towards from gain_db (the starting gain, 0 when absent) while the
                    stream runs, under the same ceiling; the other routes refuse it and point to loudness.  Errors before the first byte map as below; the lock is held until the last byte
                    has left or the client has gone, whichever comes first (_HeldPieces, _ClosingStream).
                    marks = true (new, default false): the response carries the header X-Speech-Marks, compact JSON {"sample_rate", "tokens":
                    [[line, index, phone, start, end], ...], "words": [[line, index, start, end], ...]} in delivered samples: the timing of the
                    whole utterance, known before the first audio byte (a header rather than a leading body part: the body stays the audio alone).
                    No levels on this route (the body stays the audio alone): /synthesize_stream_marks.  A server in front may cap header
                    sizes: very long texts should ask /synthesize_marks or /synthesize_stream_marks instead.
  POST /synthesize_stream_marks  new: the body of /synthesize_stream (its marks field is ignored) plus envelope_hz = null -> application/x-ndjson,
                    one JSON object per line while the request is synthesised.  First line {"media_type", "sample_rate", "total_samples",
                    "marks": the timing of the whole answer (orchestrator.token_marks)}.  Then one line per piece of /synthesize_stream's body
                    {"audio": base64 of that piece, "delivered": samples out so far, "tokens": [{"token", "level_dbfs", "peak"}, ...],
                    "envelope": {"first", "hop", "level_dbfs", "peak"} (with envelope_hz)}: the levels of the tokens and envelope frames whose
                    last sample that piece delivered, reduced on the device chunk by chunk.  The pieces' audio concatenates to /synthesize_stream's
                    body; the last line's delivered equals total_samples.  Same lock and closing discipline as /synthesize_stream.
                    pitch_hz = null (new; range as for /synthesize_marks): the first line gains "pitch": {"hop", "n_frames"} and every later
                    line "pitch": {"first", "hop", "f0_hz", "aperiodicity"}, the frames of the contour whose window that piece completed
                    (about 1 / pitch_min_hz seconds behind the audio), estimated on the device chunk by chunk with the one-shot contour's bits.
  pitch_scale = 1.0, intonation_scale = 1.0 (new; /synthesize and /synthesize_marks, batched or not): the voice's f0 multiplied by pitch_scale
                    ([0.5, 2]) and its excursions about the mean scaled by intonation_scale ([0, 2]), by an overlap-add of the synthesized signal
                    on the device; the signal keeps its length, so marks keep their spans.  The stream routes answer 400 for other values.
  pitch_track = false (new; the same routes): octave-error repair.  The contours the request uses (pitch_hz's in the marks, the shifter's own)
                    are tracked across frames on the device, one best path through every frame's candidate lags; the marks' "pitch" block then
                    says "tracked": true.  It needs pitch_hz or a scale away from 1.  The stream routes answer 400 for true.
  compressor = false (new; the same routes; comp_threshold = 8.0, comp_ratio = 4.0, comp_attack = 600.0, comp_release = 60.0): a speech compressor
                    in front of the loudness gain or the limiter, on the device: what lies more than comp_threshold dB above the signal's own
                    loudness is taken down by comp_ratio, at comp_attack / comp_release dB per second.  It needs loudness, as limiter does.  The
                    marks of /synthesize_marks then carry "dynamics": {"loudness_lufs", "threshold_lufs", "deepest_db"}.  The stream routes answer
                    400 for true: the threshold needs the whole signal's loudness and the attack looks ahead without bound.
  token_pitch = null (new; the same routes; token_pitch_kind = "hz", token_pitch_smooth = 2): one value per token of the speech marks, 0 = leave
                    the token alone; "hz": the mean f0 the token shall have ([35, 1200]), "ratio": a factor on its f0 ([0.5, 2]); the ratio changes
                    over token_pitch_smooth contour frames ([0, 20]) to each side of a token boundary.  Query /synthesize_marks with pitch_hz, edit
                    the tokens' f0_hz, ask again with the same text: the edit is made by the shifter of pitch_scale on the device and composes
                    with the scales.  The marks of /synthesize_marks then carry "pitch_edit": {"kind", "smooth", "applied" (the ratio used per
                    token), "src_f0_hz" (the token's measured mean, null without a voiced frame)}.  A bad value, kind or smoothing and a list of
                    another length than the text's token count (the message names the expected count) answer 400, and so do the stream routes
                    for any list.
  formant_scale = 1.0 (new; the same routes): the voice's formants moved by that factor in [0.5, 2], f0 and the length left alone (below 1 a
                    larger, darker speaker, above 1 a smaller, brighter one); made by the shifter of pitch_scale on the device, it composes with
                    pitch_scale, intonation_scale, pitch_track and token_pitch.  The marks of /synthesize_marks then carry "formant_scale".  The
                    stream routes answer 400 for a value other than 1 unless voice_pivot_hz is named.
  voice_pivot_hz = null (new; /synthesize_stream and /synthesize_stream_marks): the f0 in Hz, in [70, 600], that intonation_scale pivots about on a
                    stream, in place of the mean f0 a stream cannot know ahead: one number, or with split_sentences one per non-empty line.
                    With it the stream routes take pitch_scale, intonation_scale and formant_scale and shift the voice on the device chunk by
                    chunk; audio then runs about 60 ms further behind the synthesis within a sentence.  Read it from the "pitch" block of a
                    /synthesize_marks answer of the same voice (the mean of its voiced f0_hz); with that value the stream's samples are those of
                    /synthesize.  A value outside the range answers 400 there; /synthesize and /synthesize_marks refuse the field and name the
                    stream routes.  pitch_track and token_pitch stay refused on streams.
  assist_text = null (new; all four synthesis routes, streams included; assist_text_weight = 0.7): a second text ("I am so happy!") that steers
                    HOW the text is spoken, upstream Style-Bert-VITS2's assist_text: it is parsed by the holder's parse_text, runs through the
                    same DeBERTa in the same run, and the mean of its features is mixed into every token's feature with that weight in [0, 1] on
                    the device.  A weight outside [0, 1] answers 500 on /synthesize and /synthesize_marks and 400 on the stream routes, before
                    the holder is asked; null, "" or a weight of 0 is the request it always was.
  POST /synthesize_marks  new: the body of /synthesize plus envelope_hz = null -> application/json {"audio": base64 of the bytes /synthesize
                    answers with, "media_type", "sample_rate", "marks"}: when each phone id and word is spoken in that audio and how loud
                    (orchestrator.marks_dict; levels computed on the device), with envelope_hz a level envelope of sample_rate // envelope_hz
                    samples per frame.  With batching the request shares runs like /synthesize.
                    pitch_hz = null (new; with pitch_min_hz = 70, pitch_max_hz = 600): the marks also carry "pitch" {"hop", "f0_hz" (null for an
                    unvoiced frame), "aperiodicity"}, pitch_hz frames per second estimated on the device from the delivered samples, and every
                    token "f0_hz" and "voiced".  /synthesize_stream_marks carries the field too; every other route refuses it.
  any error         500 text/plain "Something went wrong: <message>"            sbv2_api/src/error.rs:10-18
  one request at a time (Arc<Mutex<TTSModelHolder>>, main.rs:86,104)             -> a lock around the holder
  make_app(holder, batching={...})  new, off by default: concurrent /synthesize requests share pipeline runs (batcher.py)

FastAPI / starlette are plumbing here; `python -m sbv2_api_amd.rest` is not provided on purpose: a deployment needs the text front end
(G2P + tokenizer, out of scope: SURVEY.md §2 #7-12) plugged into the holder's `parse_text`."""
import base64
import json
import threading
from typing import List, Optional, Union


class _HeldPieces:
    """The pieces of one streamed answer together with the holder's lock, which the handler took before it asked the holder for them.
    close() ends the pieces (their own close(), if they have one) and gives the lock back, exactly once, whoever calls it: the end of the
    pieces, a failing piece, the response once it is over (_ClosingStream), or the collector.  Nothing here hangs on a generator's `finally`:
    a client that goes away before the first piece is asked for leaves a generator that was never started, and such a one never runs it.
    next and close exclude each other, so a piece still being fetched on a worker thread is never cut off by a close from the event loop."""

    def __init__(self, lock, pieces):
        self._lock, self._pieces, self._busy, self._open = lock, iter(pieces), threading.Lock(), True
        self._close_pieces = getattr(pieces, "close", None)

    def __iter__(self):
        return self

    def __next__(self):
        with self._busy:
            if not self._open:
                raise StopIteration
            try:
                return next(self._pieces)
            except BaseException:      # the end (StopIteration) or a failing piece
                self._close()
                raise

    def close(self):
        with self._busy:
            self._close()

    def _close(self):
        if not self._open:
            return
        self._open = False
        try:
            if self._close_pieces is not None:
                self._close_pieces()
        finally:
            self._lock.release()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _MarksLines:
    """The NDJSON lines of /synthesize_stream_marks over an orchestrator.SynthesisStream begun with levels: the opening line, then one line per
    piece with the levels that piece completed.  close() closes the stream (_HeldPieces calls it, once, however the response ends)."""

    def __init__(self, pieces, media_type, sample_rate, total_samples):
        self._pieces, self.close = pieces, pieces.close
        self._first = {"media_type": media_type, "sample_rate": sample_rate, "total_samples": total_samples,
                       "marks": {k: pieces.marks[k] for k in ("sample_rate", "tokens", "words")}}
        if "pitch" in pieces.marks:   # (a stream begun with pitch: what the contour will hold, before its first frame)
            hop = int(pieces.marks["pitch"]["hop"])
            self._first["pitch"] = {"hop": hop, "n_frames": -(-int(total_samples) // hop)}

    def __iter__(self):
        return self

    def __next__(self):
        if self._first is not None:
            # (the timing as it stands before the first piece: the levels follow line by line)
            line, self._first = json.dumps(self._first), None
            return (line + "\n").encode()
        audio = next(self._pieces)
        d = self._pieces.take_marks()
        return (json.dumps({"audio": base64.b64encode(audio).decode("ascii"), **d}) + "\n").encode()


def make_app(holder, batching=None):
    """batching None: one request at a time, as the reference.  A dict of batcher.RequestBatcher keyword arguments (max_utts, max_symbols,
    max_wait_ms; {} = the defaults): /synthesize holds the lock only while the request is parsed and queued, then awaits its answer, so
    concurrent requests for a model share pipeline runs.  /synthesize_stream keeps the lock either way: a /synthesize that arrives during a
    stream waits for it on a worker thread, and the holder keeps the streamed model's batcher paused while the stream is open."""
    from fastapi import FastAPI, Request
    from fastapi.responses import JSONResponse, PlainTextResponse, Response, StreamingResponse
    from pydantic import BaseModel

    from . import orchestrator

    class SynthesizeRequest(BaseModel):      # main.rs:51-63
        text: str
        ident: str
        sdp_ratio: float = 0.0
        length_scale: float = 1.0
        style_id: int = 0
        speaker_id: int = 0
        sample_rate: int = 44100            # new: output format of the WAV (the reference's is 44.1 kHz f32)
        encoding: str = "f32"               # "f32" | "s16" | "flac" | "mulaw" | "alaw" (G.711 in a WAV, tag 7 / 6)
        normalize: bool = False             # peak of the signal -> full scale
        loudness: Optional[float] = None    # integrated loudness target (LUFS, BS.1770-4); exclusive with normalize
        true_peak_max: float = -1.0         # true-peak ceiling (dBTP) of the loudness gain
        limiter: bool = False               # look-ahead true-peak limiter for targets the plain gain misses; needs loudness
        max_reduction: float = 6.0          # the limiter's deepest gain reduction (dB)
        gain_db: Optional[float] = None     # /synthesize_stream only: fixed gain (dB) under the true_peak_max ceiling; refused elsewhere
        level_target: Optional[float] = None   # new: /synthesize_stream, /synthesize_stream_marks: loudness target (LUFS) followed on the stream, gain_db the starting gain; refused elsewhere
        level_range: float = 12.0           # how far the follower may move from gain_db (dB), [0, 20]
        level_slew: float = 3.0             # its fastest move (dB per second), (0, 20]
        level_hold: int = 10                # 400 ms blocks above the absolute gate before it moves, [1, 100]
        pitch_hz: Optional[int] = None      # /synthesize_marks, /synthesize_stream_marks: frames per second of the pitch contour in the marks; refused elsewhere
        pitch_min_hz: float = 70.0          # the contour's search range (Hz)
        pitch_max_hz: float = 600.0
        pitch_scale: float = 1.0            # new: multiplies the voice's f0, [0.5, 2]; /synthesize, /synthesize_marks (batched or not); refused on the stream routes
        intonation_scale: float = 1.0       # new: scales f0's excursions about its mean, [0, 2]; the same routes
        pitch_track: bool = False           # new: octave-error repair of the contours in use (needs pitch_hz or a scale away from 1); the same routes
        compressor: bool = False            # new: speech compressor in front of the loudness stage; needs loudness; the same routes
        comp_threshold: float = 8.0         # dB above the signal's own integrated loudness, [0, 30]
        comp_ratio: float = 4.0             # [1, 20]
        comp_attack: float = 600.0          # dB per second, [10, 10000]
        comp_release: float = 60.0          # dB per second, [1, 1000]
        token_pitch: Optional[List[float]] = None   # new: per token of the speech marks, 0 = not edited; /synthesize, /synthesize_marks; 400 on the stream routes
        token_pitch_kind: str = "hz"        # "hz": the token's target mean f0, [35, 1200]; "ratio": a factor on its f0, [0.5, 2]
        token_pitch_smooth: int = 2         # contour frames to each side over which the ratio changes, [0, 20]
        assist_text: Optional[str] = None   # new: a second text whose DeBERTa features steer the delivery (upstream's assist_text); all four routes
        assist_text_weight: float = 0.7     # its weight, [0, 1] (upstream's default); 0 = none
        formant_scale: float = 1.0          # new: moves the voice's formants, [0.5, 2]; /synthesize, /synthesize_marks (batched or not); 400 on the stream routes without voice_pivot_hz
        voice_pivot_hz: Optional[Union[float, List[float]]] = None   # new: /synthesize_stream, /synthesize_stream_marks: the f0 (Hz, [70, 600]) that intonation_scale pivots about, one number or one per sentence; it opens the three scales on the stream routes; 400 elsewhere

    class SynthesizeMarksRequest(SynthesizeRequest):
        envelope_hz: Optional[int] = None   # frames per second of the level envelope; null = none

    class SynthesizeStreamRequest(SynthesizeRequest):
        marks: bool = False                 # the utterance's timing in the X-Speech-Marks response header
        split_sentences: bool = False       # the text's lines as sentences of one batched run, streamed one after the other with /synthesize's pauses

    class SynthesizeStreamMarksRequest(SynthesizeStreamRequest):
        envelope_hz: Optional[int] = None   # frames per second of the level envelope; null = none

    class _ClosingStream(StreamingResponse):
        """A StreamingResponse that closes its _HeldPieces when the response is over, however it ends: sent to the end, cut by the client's
        disconnect (before the first piece was asked for included) or failed."""

        def __init__(self, held, **kw):
            super().__init__(held, **kw)
            self._held = held

        async def __call__(self, scope, receive, send):
            try:
                await super().__call__(scope, receive, send)
            finally:
                self._held.close()

    app = FastAPI(docs_url="/docs")          # main.rs:196 serves the OpenAPI document at /docs as well
    lock = threading.Lock()

    @app.exception_handler(Exception)
    async def _err(_: Request, exc: Exception):
        return PlainTextResponse(f"Something went wrong: {exc}", status_code=500)

    @app.get("/", response_class=PlainTextResponse)
    def root():
        return "Hello, World!"

    @app.get("/models")
    def models():
        with lock:
            return JSONResponse(holder.models())

    def options_of(req):
        return orchestrator.SynthesizeOptions(sdp_ratio=req.sdp_ratio, length_scale=req.length_scale, sample_rate=req.sample_rate,
                                              encoding=req.encoding, normalize=req.normalize, loudness=req.loudness,
                                              true_peak_max=req.true_peak_max, limiter=req.limiter, max_reduction=req.max_reduction,
                                              envelope_hz=getattr(req, "envelope_hz", None), gain_db=req.gain_db, pitch_hz=req.pitch_hz,
                                              pitch_min_hz=req.pitch_min_hz, pitch_max_hz=req.pitch_max_hz, pitch_scale=req.pitch_scale,
                                              intonation_scale=req.intonation_scale, **({"pitch_track": True} if getattr(req, "pitch_track", False) else {}),
                                              **({"compressor": True, "comp_threshold": req.comp_threshold, "comp_ratio": req.comp_ratio,
                                                  "comp_attack": req.comp_attack, "comp_release": req.comp_release}
                                                 if getattr(req, "compressor", False) else {}),
                                              **({"token_pitch": req.token_pitch, "token_pitch_kind": req.token_pitch_kind,
                                                  "token_pitch_smooth": req.token_pitch_smooth}
                                                 if getattr(req, "token_pitch", None) is not None else {}),
                                              **({"formant_scale": req.formant_scale} if getattr(req, "formant_scale", 1.0) != 1.0 else {}),
                                              **({"voice_pivot_hz": req.voice_pivot_hz} if getattr(req, "voice_pivot_hz", None) is not None else {}),
                                              **({"level_target": req.level_target, "level_range": req.level_range, "level_slew": req.level_slew,
                                                  "level_hold": req.level_hold} if getattr(req, "level_target", None) is not None else {}),
                                              **({"assist": req.assist_text or None, "assist_weight": req.assist_text_weight}
                                                 if getattr(req, "assist_text", None) or getattr(req, "assist_text_weight", 0.7) != 0.7 else {}))

    def bad_request(e):
        """400 for what the request itself is at fault for in token_pitch (a bad value, a count that does not match the text)."""
        return PlainTextResponse(f"Something went wrong: {e}", status_code=400)

    def synthesize(req: SynthesizeRequest):
        try:
            with lock:
                wav = holder.easy_synthesize(req.ident, req.text, req.style_id, req.speaker_id, options_of(req))
        except orchestrator.TokenPitchError as e:
            return bad_request(e)
        except Exception as e:                # any error -> 500 + text, like AppError::into_response
            return PlainTextResponse(f"Something went wrong: {e}", status_code=500)
        return Response(content=wav, media_type="audio/flac" if req.encoding == "flac" else "audio/wav")

    def synthesize_batched(req: SynthesizeRequest):
        # a plain function: it runs on a worker thread, so neither the lock (which a stream holds until its last byte has left, and gives back
        # only with the event loop's help) nor parse_text, a model load or an eviction's drain inside the holder ever stall the event loop
        try:
            with lock:                        # parse and queue only: the answer is awaited without it
                fut = holder.easy_synthesize_batched(req.ident, req.text, req.style_id, req.speaker_id, options_of(req), batching=batching)
            wav = fut.result()
        except orchestrator.TokenPitchError as e:
            return bad_request(e)
        except Exception as e:
            return PlainTextResponse(f"Something went wrong: {e}", status_code=500)
        return Response(content=wav, media_type="audio/flac" if req.encoding == "flac" else "audio/wav")

    app.post("/synthesize")(synthesize if batching is None else synthesize_batched)

    @app.post("/synthesize_marks")
    def synthesize_marks(req: SynthesizeMarksRequest):
        try:
            if batching is None:
                with lock:
                    audio, marks = holder.easy_synthesize_marks(req.ident, req.text, req.style_id, req.speaker_id, options_of(req))
            else:
                with lock:
                    fut = holder.easy_synthesize_batched(req.ident, req.text, req.style_id, req.speaker_id, options_of(req), batching=batching,
                                                         marks=True)
                audio, marks = fut.result()
        except orchestrator.TokenPitchError as e:
            return bad_request(e)
        except Exception as e:
            return PlainTextResponse(f"Something went wrong: {e}", status_code=500)
        return JSONResponse({"audio": base64.b64encode(audio).decode("ascii"), "media_type": "audio/flac" if req.encoding == "flac" else "audio/wav",
                             "sample_rate": marks["sample_rate"], "marks": marks})

    def stream_marks_header(marks):
        return json.dumps({"sample_rate": marks["sample_rate"],
                           "tokens": [[t["line"], t["index"], t["phone"], t["start"], t["end"]] for t in marks["tokens"]],
                           "words": [[w["line"], w["index"], w["start"], w["end"]] for w in marks["words"]]}, separators=(",", ":"))

    def refuse_stream_voice(req):
        """A 400 for pitch_scale / intonation_scale / pitch_track / compressor on a stream route, and for an assist_text_weight outside [0, 1] (the
        request is at fault, nothing was tried), None at the defaults."""
        try:
            orchestrator.refuse_dynamics(req, "a stream (/synthesize_stream, /synthesize_stream_marks)")
            orchestrator.check_voice_pivot(getattr(req, "voice_pivot_hz", None))   # (a bad pivot is the request's fault)
            orchestrator.refuse_voice(req, "a stream (/synthesize_stream, /synthesize_stream_marks)")
            orchestrator.refuse_token_pitch(req, "a stream (/synthesize_stream, /synthesize_stream_marks)")
            orchestrator.refuse_track(req, "a stream (/synthesize_stream, /synthesize_stream_marks)")
            orchestrator.check_assist(None, getattr(req, "assist_text_weight", 0.7))   # (a stream takes an assist; a bad weight is the request's fault)
        except Exception as e:
            return PlainTextResponse(f"Something went wrong: {e}", status_code=400)
        return None

    @app.post("/synthesize_stream")
    def synthesize_stream(req: SynthesizeStreamRequest):
        refused = refuse_stream_voice(req)
        if refused is not None:
            return refused
        lock.acquire()                        # one request at a time: given back by _HeldPieces.close when the response is over
        try:
            # split_sentences = False is the holder's own default (split=False), and it is sent by leaving the keyword out, on purpose: a holder
            # written before request streams takes five arguments and keeps serving every request that does not ask for a split.  Asked of such
            # a holder, a split is a TypeError, answered as the error below, never a silent unsplit stream.
            pieces = holder.easy_synthesize_stream(req.ident, req.text, req.style_id, req.speaker_id, options_of(req),
                                                   **({"split": True} if req.split_sentences else {}))
            held = _HeldPieces(lock, pieces)
            headers = {"X-Speech-Marks": stream_marks_header(pieces.marks)} if req.marks else None
        except BaseException as e:            # before the first byte: the same mapping
            lock.release()
            if not isinstance(e, Exception):
                raise
            return PlainTextResponse(f"Something went wrong: {e}", status_code=500)
        return _ClosingStream(held, media_type="audio/flac" if req.encoding == "flac" else "audio/wav", headers=headers)

    @app.post("/synthesize_stream_marks")
    def synthesize_stream_marks(req: SynthesizeStreamMarksRequest):
        refused = refuse_stream_voice(req)
        if refused is not None:
            return refused
        lock.acquire()                        # as /synthesize_stream: given back by _HeldPieces.close when the response is over
        try:
            # (pitch is sent like split: named only when the request asks for it, so a request without pitch_hz is the call it always was)
            pieces = holder.easy_synthesize_stream(req.ident, req.text, req.style_id, req.speaker_id, options_of(req), levels=True,
                                                   **({"split": True} if req.split_sentences else {}),
                                                   **({"pitch": True} if req.pitch_hz is not None else {}))
            try:
                lines = _MarksLines(pieces, "audio/flac" if req.encoding == "flac" else "audio/wav", pieces.marks["sample_rate"],
                                    pieces.total_samples)
            except BaseException:
                pieces.close()
                raise
            held = _HeldPieces(lock, lines)
        except BaseException as e:            # before the first byte: the same mapping
            lock.release()
            if not isinstance(e, Exception):
                raise
            return PlainTextResponse(f"Something went wrong: {e}", status_code=500)
        return _ClosingStream(held, media_type="application/x-ndjson")

    return app
