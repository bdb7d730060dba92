// Streaming long-form synthesis (BASELINE configs[4]; the reference has no counterpart: it synthesises a sentence per session.run and
// splits long text on '\n' only, crates/sbv2_core/src/tts.rs:290-321).
//
// DeBERTa, the text encoder, the duration predictors and the flow use global attention and run whole-sequence; the HiFi-GAN decoder, 82 %
// of the work and all of the output bytes, is purely convolutional and runs on fixed-size frame windows (chunk + 16-frame halo per side),
// one hipGraph captured per window shape and replayed per chunk (VitsModel::stream_begin / stream_next, vits.cpp).  The first PCM is
// available after the flow + ONE chunk instead of after the whole decoder, and the decoder workspace is bounded by the window.
// A request stream (sbv2_stream_begin_request) is the same over the n rows of ONE batched forward: the rows on a silent timeline, each cut into
// chunks on its own frame grid, delivered row after row; the single-utterance streams are its n = 1 case (begin_stream below).
#include "api_internal.h"

struct sbv2_stream {
    sbv2_bert* bert = nullptr;
    sbv2_vits* vits = nullptr;
    int64_t calls = 0, next = 0;   // the stream's calls (its rows' chunks, row after row) and the next one to deliver
    // speech marks (sbv2_stream_marks): the rows' expanded durations (row i's tokens are [offs[i], offs[i + 1])), on the host since the forward's
    // one sync, and the delivered format
    std::vector<int64_t> durations, offs;
    PcmFmtSpec spec;
    // the entries sbv2_stream_next_marks and the frames sbv2_stream_next_pitch have handed out so far
    int64_t tok_out = 0, env_out = 0, pitch_out = 0;
    // what the stream was begun with is the model's to say: its output side, nullptr for a plain stream (native f32)
    const StreamOutput* output() const { return vits->m->stream_output(); }
};

namespace {
// the checked format of a FLAC stream: s16, not normalised (throws with the reason otherwise)
PcmFmtSpec flac_stream_spec(const sbv2_pcm_format* fmt) {
    const PcmFmtSpec spec = pcm_format_spec(fmt);
    SBV2_REQUIRE(spec.encoding == kEncS16, "FLAC needs encoding = 1 (s16): f32 samples and G.711 codes have no FLAC form");
    SBV2_REQUIRE(!spec.normalize, "a FLAC stream cannot normalise (normalize must be 0): the peak of the utterance is not known ahead");
    return spec;
}

// The one path behind every sbv2_stream_begin*: the forward of the batch's rows with skip_decoder, then the stream over them.  spec == nullptr:
// a plain stream (native f32, one row); gap_after == nullptr: one row without gaps.  Every check of the arguments has happened before.
void begin_stream(sbv2_bert* bert, sbv2_vits* vits, const VitsBatch& v, const int64_t* token_ids, const int64_t* s_lens, const int64_t* word2ph,
                  int64_t chunk_frames, const PcmFmtSpec* spec, bool flac, const StreamLevelSpec* level, const int64_t* gap_after, sbv2_stream** out,
                  int64_t* total_samples, const StreamMarksSpec* marks = nullptr, const AssistSpec* assist = nullptr,
                  const StreamVoiceSpec* voice = nullptr, const StreamLevelerSpec* leveler = nullptr) {
    VitsBatch run = v;
    run.skip_decoder = true;
    pipeline_run_one(*bert->m, *vits->m, run, token_ids, s_lens, word2ph, assist);
    std::unique_ptr<sbv2_stream> s(new sbv2_stream);
    s->bert = bert;
    s->vits = vits;
    s->durations = vits->m->used_durations();
    s->offs = vits->m->used_offs();
    if (spec) s->spec = *spec;
    s->calls = vits->m->stream_begin((int)chunk_frames, spec, flac, level, gap_after, marks, voice, leveler);
    if (total_samples) *total_samples = pcm_format_out_len(s->spec, vits->m->stream_layout().joined);
    *out = s.release();
}

// The one place that refuses the wrong kind of sbv2_stream_next* call for a stream, in each call's own words and order
enum NextKind { kNextPlain, kNextFormat, kNextFlac, kNextLevel };
void require_kind(const sbv2_stream* s, NextKind want) {
    const StreamOutput* o = s->output();
    const bool level = o && o->level(), flac = o && o->flac(), voice = o && o->voice();
    if (want == kNextLevel) {
        SBV2_REQUIRE(level || voice, "this stream was not begun with a level: take its chunks with the sbv2_stream_next call of its kind");
    } else {
        SBV2_REQUIRE(!level, "this stream was begun with a level: take its chunks with sbv2_stream_next_level");
        SBV2_REQUIRE(!voice, "this stream was begun with a voice, and delivery runs behind its chunks: take them with sbv2_stream_next_level");
    }
    if (want == kNextFlac) SBV2_REQUIRE(flac, "this stream was not begun as FLAC: take its chunks with sbv2_stream_next or sbv2_stream_next_format");
    else if (want != kNextLevel) SBV2_REQUIRE(!flac, "this stream was begun as FLAC: take its chunks with sbv2_stream_next_flac");
    if (want == kNextFormat) SBV2_REQUIRE(o, "this stream has no output format: take its chunks with sbv2_stream_next");
    else if (want == kNextPlain) SBV2_REQUIRE(!o, "this stream was begun with an output format: take its chunks with sbv2_stream_next_format");
}
// the stream's next call -> dst; all zero once the stream is complete
StreamOutput::Taken take_next(sbv2_stream* s, void* dst, int64_t capacity_bytes) {
    if (s->next >= s->calls) return StreamOutput::Taken{};
    const StreamOutput::Taken t = s->vits->m->stream_next(s->next, dst, capacity_bytes);
    s->next += 1;
    return t;
}
}  // namespace

extern "C" {

// One utterance (batch->n must be 1; same inputs as sbv2_pipeline_run).  chunk_frames: frames of PCM per sbv2_stream_next call (hop = 512
// samples per frame; 256 frames = 2.97 s).  *total_samples = length of the whole utterance.  The two handles must not be used for anything
// else until sbv2_stream_end.
int sbv2_stream_begin(sbv2_bert* bert, sbv2_vits* vits, const sbv2_batch* batch, const int64_t* token_ids, const int64_t* s_lens,
                      const int64_t* word2ph, int64_t chunk_frames, sbv2_stream** out, int64_t* total_samples) {
    API_BEGIN
    SBV2_REQUIRE(bert && vits && batch && token_ids && s_lens && word2ph && out, "bad arguments");
    SBV2_REQUIRE(batch->n == 1, "sbv2_stream_begin takes one utterance");
    SBV2_REQUIRE(bert->m->device() == vits->m->device(), "bert and vits handles live on different devices");
    begin_stream(bert, vits, to_batch(batch), token_ids, s_lens, word2ph, chunk_frames, nullptr, false, nullptr, nullptr, out, total_samples);
    API_END
}

// Next chunk of PCM (utterance order) -> dst (host, capacity samples; >= chunk_frames * hop always suffices).  *n = samples written,
// 0 once the utterance is complete.
int sbv2_stream_next(sbv2_stream* s, float* dst, int64_t capacity, int64_t* n) {
    API_BEGIN
    SBV2_REQUIRE(s && dst && n, "bad arguments");
    require_kind(s, kNextPlain);
    *n = 0;   // (also when the call below is refused)
    *n = take_next(s, dst, capacity * (int64_t)sizeof(float)).samples;
    API_END
}

// Same as sbv2_stream_begin with the chunks leaving the device in `fmt` (formatted by one launch per decoder replay, StreamOutput::push, stream_output.cpp).
int sbv2_stream_begin_format(sbv2_bert* bert, sbv2_vits* vits, const sbv2_batch* batch, const int64_t* token_ids, const int64_t* s_lens,
                             const int64_t* word2ph, int64_t chunk_frames, const sbv2_pcm_format* fmt, sbv2_stream** out, int64_t* total_samples) {
    API_BEGIN
    SBV2_REQUIRE(bert && vits && batch && token_ids && s_lens && word2ph && out, "bad arguments");
    SBV2_REQUIRE(batch->n == 1, "sbv2_stream_begin_format takes one utterance");
    SBV2_REQUIRE(bert->m->device() == vits->m->device(), "bert and vits handles live on different devices");
    const PcmFmtSpec spec = pcm_format_spec(fmt);
    SBV2_REQUIRE(!spec.normalize, "a formatted stream cannot normalise (normalize must be 0): the peak of the utterance is not known ahead");
    begin_stream(bert, vits, to_batch(batch), token_ids, s_lens, word2ph, chunk_frames, &spec, false, nullptr, nullptr, out, total_samples);
    API_END
}

int sbv2_stream_next_format(sbv2_stream* s, void* dst, int64_t capacity_bytes, int64_t* n) {
    API_BEGIN
    SBV2_REQUIRE(s && dst && n, "bad arguments");
    require_kind(s, kNextFormat);
    *n = 0;
    *n = take_next(s, dst, capacity_bytes).samples;
    API_END
}

// Host only: bytes that always suffice for one sbv2_stream_next_flac call of a stream with chunks of chunk_native_samples (-1: bad fmt)
int64_t sbv2_flac_stream_bound(const sbv2_pcm_format* fmt, int64_t chunk_native_samples) {
    try {
        const PcmFmtSpec spec = flac_stream_spec(fmt);
        SBV2_REQUIRE(chunk_native_samples >= 0, "negative sample count");
        return flac_stream_bound(pcm_format_out_len(spec, chunk_native_samples));
    } catch (const std::exception& e) {
        set_last_error(e.what());
        return -1;
    }
}

// Same as sbv2_stream_begin_format (fmt: s16, normalize 0) with the chunks' samples encoded as ONE FLAC stream on the device, replay by
// replay (StreamOutput::push, stream_output.cpp, flac_encode.hip FlacStreamEncoder).
int sbv2_stream_begin_flac(sbv2_bert* bert, sbv2_vits* vits, const sbv2_batch* batch, const int64_t* token_ids, const int64_t* s_lens,
                           const int64_t* word2ph, int64_t chunk_frames, const sbv2_pcm_format* fmt, sbv2_stream** out, int64_t* total_samples) {
    API_BEGIN
    SBV2_REQUIRE(bert && vits && batch && token_ids && s_lens && word2ph && out, "bad arguments");
    SBV2_REQUIRE(batch->n == 1, "sbv2_stream_begin_flac takes one utterance");
    SBV2_REQUIRE(bert->m->device() == vits->m->device(), "bert and vits handles live on different devices");
    const PcmFmtSpec spec = flac_stream_spec(fmt);
    begin_stream(bert, vits, to_batch(batch), token_ids, s_lens, word2ph, chunk_frames, &spec, true, nullptr, nullptr, out, total_samples);
    API_END
}

// The bytes of every FLAC frame that the next chunk's samples complete -> dst (host; the stream header in front on the first call).
// *n_samples = s16 samples the chunk consumed (0 once the utterance is complete), *n_bytes may be 0 while *n_samples > 0.
int sbv2_stream_next_flac(sbv2_stream* s, uint8_t* dst, int64_t capacity_bytes, int64_t* n_bytes, int64_t* n_samples) {
    API_BEGIN
    SBV2_REQUIRE(s && dst && n_bytes && n_samples, "bad arguments");
    require_kind(s, kNextFlac);
    *n_bytes = *n_samples = 0;
    const StreamOutput::Taken t = take_next(s, dst, capacity_bytes);
    *n_bytes = t.bytes;
    *n_samples = t.samples;
    API_END
}

// Host only: A, the delivered samples a level stream runs behind (-1: bad fmt).  A depends on the rate alone and this call keeps its first
// contract: encodings 0 and 1 only (a G.711 level stream runs the A of its rate: ask with either)
int64_t sbv2_stream_level_lookahead(const sbv2_pcm_format* fmt) {
    try {
        SBV2_REQUIRE(!fmt || !pcm_encoding_g711(fmt->encoding),
                     "unsupported PCM encoding " + std::to_string(fmt->encoding) + " for the look-ahead query (0 = f32, 1 = s16: A depends on the rate alone)");
        return stream_level_lookahead(pcm_format_spec(fmt).rate);
    } catch (const std::exception& e) {
        set_last_error(e.what());
        return -1;
    }
}

// Host only: bytes that always suffice for one sbv2_stream_next_level call of a stream with chunks of chunk_native_samples: a call hands
// back at most the chunk's samples and the A the stream held back (-1: bad fmt)
int64_t sbv2_stream_level_bound(const sbv2_pcm_format* fmt, int64_t chunk_native_samples, int flac) {
    try {
        const PcmFmtSpec spec = flac ? flac_stream_spec(fmt) : pcm_format_spec(fmt);
        SBV2_REQUIRE(!spec.normalize, "a level stream cannot normalise (normalize must be 0): the peak of the utterance is not known ahead");
        SBV2_REQUIRE(chunk_native_samples >= 0, "negative sample count");
        const int64_t n = pcm_format_out_len(spec, chunk_native_samples) + stream_level_lookahead(spec.rate);
        return flac ? flac_stream_bound(n) : n * spec.bytes();
    } catch (const std::exception& e) {
        set_last_error(e.what());
        return -1;
    }
}

// Same as sbv2_stream_begin_format (or, with flac, sbv2_stream_begin_flac) with the fixed-gain limiter of `level` between the resampler and
// the cast / quantiser (StreamOutput::push, stream_output.cpp, limiter.hip StreamLimiter).
int sbv2_stream_begin_level(sbv2_bert* bert, sbv2_vits* vits, const sbv2_batch* batch, const int64_t* token_ids, const int64_t* s_lens,
                            const int64_t* word2ph, int64_t chunk_frames, const sbv2_pcm_format* fmt, const sbv2_stream_level* level, int flac,
                            sbv2_stream** out, int64_t* total_samples) {
    API_BEGIN
    SBV2_REQUIRE(bert && vits && batch && token_ids && s_lens && word2ph && out, "bad arguments");
    SBV2_REQUIRE(batch->n == 1, "sbv2_stream_begin_level takes one utterance");
    SBV2_REQUIRE(bert->m->device() == vits->m->device(), "bert and vits handles live on different devices");
    const PcmFmtSpec spec = flac ? flac_stream_spec(fmt) : pcm_format_spec(fmt);
    SBV2_REQUIRE(!spec.normalize, "a level stream cannot normalise (normalize must be 0): the peak of the utterance is not known ahead");
    const StreamLevelSpec lv = stream_level_spec(level);
    begin_stream(bert, vits, to_batch(batch), token_ids, s_lens, word2ph, chunk_frames, &spec, flac != 0, &lv, nullptr, out, total_samples);
    API_END
}

// What the next chunk completes -> dst (host): *n_out samples in the stream's encoding, or with FLAC the *n_out bytes of the frames that
// those samples complete (the stream header in front on the first call).  *n_consumed = samples of the chunk taken, 0 once the utterance
// is complete; *n_out may be 0 while *n_consumed > 0.
int sbv2_stream_next_level(sbv2_stream* s, void* dst, int64_t capacity_bytes, int64_t* n_out, int64_t* n_consumed) {
    API_BEGIN
    SBV2_REQUIRE(s && dst && n_out && n_consumed, "bad arguments");
    require_kind(s, kNextLevel);
    const StreamOutput::Taken t = take_next(s, dst, capacity_bytes);
    *n_out = s->output()->flac() ? t.bytes : t.samples;
    *n_consumed = t.fed;
    API_END
}

// 20 log10 min s (the deepest reduction, <= 0) and max |x| (before the cast / quantiser) over the utterance, once its last chunk was taken
int sbv2_stream_level_stats(sbv2_stream* s, double* stats) {
    API_BEGIN
    SBV2_REQUIRE(s && stats, "bad arguments");
    SBV2_REQUIRE(s->output() && s->output()->level(), "this stream was not begun with a level");
    SBV2_REQUIRE(s->next >= s->calls, "the level stats exist once the stream is complete: take its chunks to the end first");
    s->output()->level_stats(stats, s->vits->m->stream());
    API_END
}

// L_in, the last, the lowest and the highest g in dB, then the two of sbv2_stream_level_stats, once the last chunk of a levelled stream was taken
int sbv2_stream_leveler_stats(sbv2_stream* s, double* stats) {
    API_BEGIN
    SBV2_REQUIRE(s && stats, "bad arguments");
    SBV2_REQUIRE(s->output() && s->output()->leveler(), "this stream was not begun with a leveler");
    SBV2_REQUIRE(s->next >= s->calls, "the leveler stats exist once the stream is complete: take its chunks to the end first");
    s->output()->leveler_stats(stats, s->vits->m->stream());
    API_END
}

// Host only: the token spans of the stream's rows at its delivered rate (marks.h), row i at place[i] of the stream's timeline, in row order
// then token order: what sbv2_pipeline_fetch_request_marks gives for the joined fetch.  Every duration is known once _begin* has returned, so
// the whole timing is there before the first chunk is decoded.
int sbv2_stream_marks(sbv2_stream* s, int64_t* tok_start, int64_t* tok_end, int64_t capacity, int64_t* n_tokens) {
    API_BEGIN
    SBV2_REQUIRE(s && n_tokens, "bad arguments");
    const int64_t n = (int64_t)s->durations.size();
    SBV2_REQUIRE(capacity >= n, "token arrays too small: " + std::to_string(capacity) + " < " + std::to_string(n) + " tokens");
    SBV2_REQUIRE(n == 0 || (tok_start && tok_end), "bad arguments");
    marks_spans_rows(s->durations, s->offs, nullptr, (int64_t)s->offs.size() - 1, s->vits->m->stream_layout().place.data(), s->vits->m->cfg().hop(),
                     s->spec, tok_start, tok_end);
    *n_tokens = n;
    API_END
}

// ---- a stream over the n rows of ONE batched forward (the contract above sbv2_stream_begin_request, include/sbv2_hip.h) ----
// Host only: the smallest gap between two rows at fmt's rate, 2 ceil(half / L) native samples (NULL = the identity format = 0; -1: bad fmt)
int64_t sbv2_stream_min_gap(const sbv2_pcm_format* fmt) {
    try {
        return fmt ? stream_min_gap(pcm_format_spec(fmt)) : 0;
    } catch (const std::exception& e) {
        set_last_error(e.what());
        return -1;
    }
}

// Host only: placement, joined length and per-call sample counts of a request stream (stream_timeline, vits.cpp: the library's own arithmetic)
int sbv2_stream_timeline(const int64_t* frames, const int64_t* gap_after, int64_t n, int32_t hop, int64_t chunk_frames, const sbv2_pcm_format* fmt,
                         int64_t* place, int64_t* joined_len, int64_t* call_samples, int64_t capacity, int64_t* n_calls) {
    API_BEGIN
    const PcmFmtSpec spec = fmt ? pcm_format_spec(fmt) : PcmFmtSpec();
    const StreamTimeline t = stream_timeline(frames, gap_after, n, hop, chunk_frames, spec);
    const int64_t calls = (int64_t)t.calls.size();
    if (n_calls) *n_calls = calls;
    SBV2_REQUIRE(!call_samples || capacity >= calls, "call_samples too small: " + std::to_string(capacity) + " < " + std::to_string(calls) + " calls");
    if (place) std::copy(t.place.begin(), t.place.end(), place);
    if (joined_len) *joined_len = t.joined;
    if (call_samples)
        for (int64_t c = 0; c < calls; ++c) call_samples[c] = t.calls[c].j1 - t.calls[c].j0;
    API_END
}

namespace {
// sbv2_stream_begin_request, with or without levels: every check before any GPU work
void begin_request(sbv2_bert* bert, sbv2_vits* vits, const sbv2_batch* batch, const sbv2_utt_options* opts, const int64_t* token_ids, const int64_t* s_lens,
                   const int64_t* word2ph, int64_t chunk_frames, const sbv2_stream_request* rq, const StreamMarksSpec* marks, sbv2_stream** out,
                   int64_t* total_samples, const AssistSpec* assist = nullptr, const StreamVoiceSpec* voice = nullptr,
                   const StreamLevelerSpec* leveler = nullptr) {
    SBV2_REQUIRE(bert && vits && batch && token_ids && s_lens && word2ph && out, "bad arguments");
    SBV2_REQUIRE(rq, "no sbv2_stream_request given");
    SBV2_REQUIRE(rq->gap_after, "sbv2_stream_request.gap_after must not be NULL (one entry per row, the last one = trailing silence)");
    SBV2_REQUIRE(batch->n >= 1, "sbv2_stream_begin_request takes at least one row");
    SBV2_REQUIRE(rq->reserved == 0, "sbv2_stream_request.reserved must be 0");
    SBV2_REQUIRE(rq->flac == 0 || rq->flac == 1, "sbv2_stream_request.flac must be 0 or 1");
    SBV2_REQUIRE(bert->m->device() == vits->m->device(), "bert and vits handles live on different devices");
    SBV2_REQUIRE(!rq->flac || rq->fmt, "FLAC needs encoding = 1 (s16): the identity format (fmt NULL) is f32");
    const PcmFmtSpec spec = rq->flac ? flac_stream_spec(rq->fmt) : rq->fmt ? pcm_format_spec(rq->fmt) : PcmFmtSpec();
    SBV2_REQUIRE(!spec.normalize, "a request stream cannot normalise (normalize must be 0): the peak of the signal is not known ahead");
    StreamLevelSpec lv;
    if (rq->level) lv = stream_level_spec(rq->level);
    SBV2_REQUIRE(!leveler || rq->level, "a stream leveler needs sbv2_stream_request.level: its true_peak_max_dbtp is the ceiling, its gain_db the starting gain");
    VitsBatch v = to_batch(batch);
    apply_utt_options(&v, opts);
    stream_check_gaps(rq->gap_after, batch->n, spec);
    begin_stream(bert, vits, v, token_ids, s_lens, word2ph, chunk_frames, &spec, rq->flac != 0, rq->level ? &lv : nullptr, rq->gap_after, out,
                 total_samples, marks, assist, voice, leveler);
}
}  // namespace

int sbv2_stream_begin_request(sbv2_bert* bert, sbv2_vits* vits, const sbv2_batch* batch, const sbv2_utt_options* opts, const int64_t* token_ids,
                              const int64_t* s_lens, const int64_t* word2ph, int64_t chunk_frames, const sbv2_stream_request* rq, sbv2_stream** out,
                              int64_t* total_samples) {
    API_BEGIN
    begin_request(bert, vits, batch, opts, token_ids, s_lens, word2ph, chunk_frames, rq, nullptr, out, total_samples);
    API_END
}

namespace {
// sbv2_stream_levels' fields, checked before the handles are looked at; true when anything is on
bool levels_spec(const sbv2_stream_levels* lv, StreamMarksSpec* marks) {
    if (lv) {
        SBV2_REQUIRE(lv->reserved[0] == 0 && lv->reserved[1] == 0, "sbv2_stream_levels.reserved must be 0");
        SBV2_REQUIRE(lv->tokens == 0 || lv->tokens == 1, "sbv2_stream_levels.tokens must be 0 or 1");
        SBV2_REQUIRE(lv->env_hop >= 0, "sbv2_stream_levels.env_hop must be >= 0 (0 = no envelope)");
        marks->tokens = lv->tokens == 1;
        marks->env_hop = lv->env_hop;
    }
    return marks->tokens || marks->env_hop > 0;
}
}  // namespace

// The same stream with the levels of its delivered samples reduced replay by replay (StreamLevels, marks.hip).  lv NULL or all off: exactly the
// call above.  The levels' fields are checked first, before the handles are looked at.
int sbv2_stream_begin_request_levels(sbv2_bert* bert, sbv2_vits* vits, const sbv2_batch* batch, const sbv2_utt_options* opts, const int64_t* token_ids,
                                     const int64_t* s_lens, const int64_t* word2ph, int64_t chunk_frames, const sbv2_stream_request* rq,
                                     const sbv2_stream_levels* lv, sbv2_stream** out, int64_t* total_samples, int64_t* n_tokens, int64_t* n_env) {
    API_BEGIN
    StreamMarksSpec marks;
    const bool on = levels_spec(lv, &marks);
    begin_request(bert, vits, batch, opts, token_ids, s_lens, word2ph, chunk_frames, rq, on ? &marks : nullptr, out, total_samples);
    const StreamLevels* l = (*out)->output()->levels();
    if (n_tokens) *n_tokens = l ? l->n_tok() : 0;
    if (n_env) *n_env = l ? l->n_env() : 0;
    API_END
}

// ... and with the pitch contour of the same samples, fed by the same pushes (StreamPitch, marks.hip).  sp NULL: exactly the call above.  The
// levels' and the pitch's fields are checked first, before the handles are looked at: the rate is the format's, a NULL fmt = 44100 Hz.
int sbv2_stream_begin_request_pitch(sbv2_bert* bert, sbv2_vits* vits, const sbv2_batch* batch, const sbv2_utt_options* opts, const int64_t* token_ids,
                                    const int64_t* s_lens, const int64_t* word2ph, int64_t chunk_frames, const sbv2_stream_request* rq,
                                    const sbv2_stream_levels* lv, const sbv2_stream_pitch* sp, sbv2_stream** out, int64_t* total_samples,
                                    int64_t* n_tokens, int64_t* n_env, int64_t* n_pitch) {
    return sbv2_stream_begin_request_assist(bert, vits, batch, opts, nullptr, token_ids, s_lens, word2ph, chunk_frames, rq, lv, sp, out, total_samples,
                                            n_tokens, n_env, n_pitch);
}

// ... and with an assist text steering the rows' delivery (the contract above sbv2_assist, include/sbv2_hip.h): the stream gets it from the one
// function the pipeline gets it from (pipeline_run_one).  assist NULL, or no row naming a text: exactly the call above.  The assist's fields are
// checked with the levels' and the pitch's, before the handles are looked at.
int sbv2_stream_begin_request_assist(sbv2_bert* bert, sbv2_vits* vits, const sbv2_batch* batch, const sbv2_utt_options* opts, const sbv2_assist* assist,
                                     const int64_t* token_ids, const int64_t* s_lens, const int64_t* word2ph, int64_t chunk_frames,
                                     const sbv2_stream_request* rq, const sbv2_stream_levels* lv, const sbv2_stream_pitch* sp, sbv2_stream** out,
                                     int64_t* total_samples, int64_t* n_tokens, int64_t* n_env, int64_t* n_pitch) {
    return sbv2_stream_begin_request_voice(bert, vits, batch, opts, assist, token_ids, s_lens, word2ph, chunk_frames, rq, lv, sp, nullptr, out,
                                           total_samples, n_tokens, n_env, n_pitch);
}

// Host only: A_v of a stream voice at a rate (-1: what the begin call refuses; the pivot is not looked at)
int64_t sbv2_stream_voice_lookahead(const sbv2_stream_voice* v, int32_t sample_rate) {
    try {
        SBV2_REQUIRE(v, "no sbv2_stream_voice given");
        SBV2_REQUIRE(v->voice.reserved == 0, "sbv2_voice.reserved must be 0");
        return stream_voice_spec(sample_rate, v->voice.pitch_scale, v->voice.intonation_scale, v->voice.hop, v->voice.f0_min, v->voice.f0_max,
                                 v->voice.threshold, v->formant_scale, nullptr, 0, v->reserved[0], v->reserved[1])
            .lookahead;
    } catch (const std::exception& e) {
        set_last_error(e.what());
        return -1;
    }
}

// Host only: what every call of a voice stream without a level delivers (stream_voice_upto, vits.cpp: the library's own arithmetic)
int sbv2_stream_voice_timeline(const int64_t* frames, const int64_t* gap_after, int64_t n, int32_t hop, int64_t chunk_frames, const sbv2_pcm_format* fmt,
                               const sbv2_stream_voice* v, int64_t* call_delivered, int64_t capacity, int64_t* n_calls) {
    API_BEGIN
    const int64_t A = sbv2_stream_voice_lookahead(v, kNativeRate);
    SBV2_REQUIRE(A >= 0, sbv2_last_error());
    const PcmFmtSpec spec = fmt ? pcm_format_spec(fmt) : PcmFmtSpec();
    const StreamTimeline t = stream_timeline(frames, gap_after, n, hop, chunk_frames, spec);
    const std::vector<int64_t> upto = stream_voice_upto(t, hop, chunk_frames, spec, A);
    const int64_t calls = (int64_t)upto.size();
    if (n_calls) *n_calls = calls;
    SBV2_REQUIRE(!call_delivered || capacity >= calls, "call_delivered too small: " + std::to_string(capacity) + " < " + std::to_string(calls) + " calls");
    if (call_delivered)
        for (int64_t c = 0; c < calls; ++c) call_delivered[c] = upto[(size_t)c] - (c ? upto[(size_t)(c - 1)] : 0);
    API_END
}

// ... and with the voice shifted on the way (the contract above sbv2_stream_voice, include/sbv2_hip.h): the fed shifter ahead of the formatter
// (StreamVoice, voice.hip; StreamOutput::push).  voice NULL: exactly the call above.  Its fields are checked with the others', before the
// handles are looked at.
int sbv2_stream_begin_request_voice(sbv2_bert* bert, sbv2_vits* vits, const sbv2_batch* batch, const sbv2_utt_options* opts, const sbv2_assist* assist,
                                    const int64_t* token_ids, const int64_t* s_lens, const int64_t* word2ph, int64_t chunk_frames,
                                    const sbv2_stream_request* rq, const sbv2_stream_levels* lv, const sbv2_stream_pitch* sp,
                                    const sbv2_stream_voice* voice, sbv2_stream** out, int64_t* total_samples, int64_t* n_tokens, int64_t* n_env,
                                    int64_t* n_pitch) {
    return sbv2_stream_begin_request_leveler(bert, vits, batch, opts, assist, token_ids, s_lens, word2ph, chunk_frames, rq, lv, sp, voice, nullptr, out,
                                             total_samples, n_tokens, n_env, n_pitch);
}

// ... and with a loudness target followed on the way (the contract above sbv2_stream_leveler, include/sbv2_hip.h): the fed leveler between the
// formatter and the stream limiter (StreamLeveler, leveler.hip; StreamOutput::push).  leveler NULL: exactly the call above.  Its fields are
// checked with the others', before the handles are looked at; it needs rq->level.
int sbv2_stream_begin_request_leveler(sbv2_bert* bert, sbv2_vits* vits, const sbv2_batch* batch, const sbv2_utt_options* opts, const sbv2_assist* assist,
                                      const int64_t* token_ids, const int64_t* s_lens, const int64_t* word2ph, int64_t chunk_frames,
                                      const sbv2_stream_request* rq, const sbv2_stream_levels* lv, const sbv2_stream_pitch* sp,
                                      const sbv2_stream_voice* voice, const sbv2_stream_leveler* leveler, sbv2_stream** out, int64_t* total_samples,
                                      int64_t* n_tokens, int64_t* n_env, int64_t* n_pitch) {
    API_BEGIN
    StreamMarksSpec marks;
    bool on = levels_spec(lv, &marks);
    StreamLevelerSpec ls;
    if (leveler) {
        ls = stream_leveler_spec(leveler);
        SBV2_REQUIRE(rq && rq->level, "a stream leveler needs sbv2_stream_request.level: its true_peak_max_dbtp is the ceiling, its gain_db the starting gain");
    }
    StreamVoiceSpec vs;
    if (voice) {
        SBV2_REQUIRE(batch && batch->n >= 1, "sbv2_stream_begin_request takes at least one row");
        SBV2_REQUIRE(voice->voice.reserved == 0, "sbv2_voice.reserved must be 0");
        vs = stream_voice_spec(kNativeRate, voice->voice.pitch_scale, voice->voice.intonation_scale, voice->voice.hop, voice->voice.f0_min,
                               voice->voice.f0_max, voice->voice.threshold, voice->formant_scale, voice->pivot_hz, batch->n, voice->reserved[0],
                               voice->reserved[1]);
    }
    if (sp) {
        SBV2_REQUIRE(sp->reserved == 0, "sbv2_stream_pitch.reserved must be 0");
        const int rate = rq && rq->fmt ? pcm_format_spec(rq->fmt).rate : PcmFmtSpec().rate;
        marks.pitch_spec = pitch_spec(rate, sp->hop, sp->f0_min, sp->f0_max, sp->threshold);
        marks.pitch = on = true;
    }
    AssistSpec as;
    if (assist) {
        SBV2_REQUIRE(batch && batch->n >= 1, "sbv2_stream_begin_request takes at least one row");
        as = assist_spec(assist, batch->n);
    }
    begin_request(bert, vits, batch, opts, token_ids, s_lens, word2ph, chunk_frames, rq, on ? &marks : nullptr, out, total_samples, &as,
                  voice ? &vs : nullptr, leveler ? &ls : nullptr);
    const StreamLevels* l = (*out)->output()->levels();
    const StreamPitch* q = (*out)->output()->pitch();
    if (n_tokens) *n_tokens = l ? l->n_tok() : 0;
    if (n_env) *n_env = l ? l->n_env() : 0;
    if (n_pitch) *n_pitch = q ? q->n_frames() : 0;
    API_END
}

// The levels completed since the previous call (the delivery rule above sbv2_stream_next_marks, include/sbv2_hip.h).  Host only: every entry
// handed out was copied to the pinned mirror before the event of a replay whose samples the stream has already delivered.
int sbv2_stream_next_marks(sbv2_stream* s, sbv2_stream_marks_part* part) {
    API_BEGIN
    SBV2_REQUIRE(s && part, "bad arguments");
    const StreamLevels* l = s->output() ? s->output()->levels() : nullptr;
    SBV2_REQUIRE(l, "this stream was begun without levels: begin it with sbv2_stream_begin_request_levels");
    const int64_t D = s->next >= s->calls ? l->total() : s->output()->delivered();
    const int64_t nt = l->tok_complete(D) - s->tok_out, ne = l->env_complete(D) - s->env_out;
    SBV2_REQUIRE(part->tok_capacity >= nt, "token arrays too small: " + std::to_string(part->tok_capacity) + " < " + std::to_string(nt) + " pending tokens");
    SBV2_REQUIRE(part->env_capacity >= ne, "envelope arrays too small: " + std::to_string(part->env_capacity) + " < " + std::to_string(ne) + " pending frames");
    SBV2_REQUIRE(nt == 0 || (part->tok_sumsq && part->tok_peak), "NULL token arrays with " + std::to_string(nt) + " pending tokens");
    SBV2_REQUIRE(ne == 0 || (part->env_sumsq && part->env_peak), "NULL envelope arrays with " + std::to_string(ne) + " pending frames");
    for (int64_t i = 0; i < nt; ++i) {
        part->tok_sumsq[i] = l->tok_host()[2 * (s->tok_out + i)];
        part->tok_peak[i] = l->tok_host()[2 * (s->tok_out + i) + 1];
    }
    for (int64_t i = 0; i < ne; ++i) {
        part->env_sumsq[i] = l->env_host()[2 * (s->env_out + i)];
        part->env_peak[i] = l->env_host()[2 * (s->env_out + i) + 1];
    }
    part->tok_first = s->tok_out;
    part->n_tok = nt;
    part->env_first = s->env_out;
    part->n_env = ne;
    part->delivered = D;
    s->tok_out += nt;
    s->env_out += ne;
    API_END
}

// The pitch frames completed since the previous call (the rule above sbv2_stream_next_pitch, include/sbv2_hip.h), finished on the host as the
// fetch finishes them.  Host only, for the reason given above sbv2_stream_next_marks.
int sbv2_stream_next_pitch(sbv2_stream* s, sbv2_stream_pitch_part* part) {
    API_BEGIN
    SBV2_REQUIRE(s && part, "bad arguments");
    const StreamPitch* q = s->output() ? s->output()->pitch() : nullptr;
    SBV2_REQUIRE(q, "this stream was begun without pitch: begin it with sbv2_stream_begin_request_pitch");
    const int64_t D = s->next >= s->calls ? q->total() : s->output()->delivered();
    const int64_t n = q->complete(D) - s->pitch_out;
    SBV2_REQUIRE(part->capacity >= n, "pitch arrays too small: " + std::to_string(part->capacity) + " < " + std::to_string(n) + " pending frames");
    SBV2_REQUIRE(n == 0 || part->f0, "NULL f0 with " + std::to_string(n) + " pending frames");
    for (int64_t i = 0; i < n; ++i) {
        const int64_t f = s->pitch_out + i;
        pitch_finish(q->spec(), q->lag_host(f), q->voiced_host(f), q->c3_host(f), part->f0 + i, part->ap ? part->ap + i : nullptr);
        if (part->lag) part->lag[i] = q->lag_host(f);
    }
    part->first = s->pitch_out;
    part->n = n;
    part->delivered = D;
    s->pitch_out += n;
    API_END
}

// Host only, valid from begin onwards: where the stream's rows lie (place[i], pcm_lens[i] native samples) and the timeline's length
int sbv2_stream_layout(const sbv2_stream* s, int64_t* place, int64_t* pcm_lens, int64_t capacity, int64_t* n, int64_t* joined_len) {
    API_BEGIN
    SBV2_REQUIRE(s, "bad arguments");
    const StreamTimeline& t = s->vits->m->stream_layout();
    const int64_t rows = (int64_t)t.place.size();
    if (n) *n = rows;
    SBV2_REQUIRE((!place && !pcm_lens) || capacity >= rows, "row arrays too small: " + std::to_string(capacity) + " < " + std::to_string(rows) + " rows");
    if (place) std::copy(t.place.begin(), t.place.end(), place);
    if (pcm_lens) std::copy(t.len.begin(), t.len.end(), pcm_lens);
    if (joined_len) *joined_len = t.joined;
    API_END
}

// Host only: bytes that suffice for any one sbv2_stream_next* call of THIS stream (-1: no stream)
int64_t sbv2_stream_call_bound(const sbv2_stream* s) { return s ? s->vits->m->stream_call_bound() : -1; }

// 1 when the decoder of this stream replays a captured hipGraph (0: eager launches, SBV2_STREAM_GRAPH=0)
int sbv2_stream_uses_graph(const sbv2_stream* s) { return s && s->vits->m->stream_graph_captured() ? 1 : 0; }
// device workspace of the chunk decoder in bytes (bounded by the window, whatever the utterance length)
int64_t sbv2_stream_workspace_bytes(const sbv2_stream* s) { return s ? (int64_t)s->vits->m->stream_workspace_bytes() : -1; }

void sbv2_stream_end(sbv2_stream* s) { delete s; }

}  // extern "C"
