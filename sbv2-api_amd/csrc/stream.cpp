// Streaming long-form synthesis (BASELINE configs[4]; the reference has no counterpart: it synthesises a sentence per session.run and
// splits long text on '\n' only, crates/sbv2_core/src/tts.rs:290-321).
//
// DeBERTa, the text encoder, the duration predictors and the flow use global attention and run whole-sequence; the HiFi-GAN decoder, 82 %
// of the work and all of the output bytes, is purely convolutional and runs on fixed-size frame windows (chunk + 16-frame halo per side),
// one hipGraph captured per window shape and replayed per chunk (VitsModel::stream_begin / stream_chunk, vits.cpp).  The first PCM is
// available after the flow + ONE chunk instead of after the whole decoder, and the decoder workspace is bounded by the window.
#include "api_internal.h"

struct sbv2_stream {
    sbv2_bert* bert = nullptr;
    sbv2_vits* vits = nullptr;
    int64_t frames = 0, next = 0, chunk = 0;
    bool formatted = false, flac = false, level = false;
    // speech marks (sbv2_stream_marks): the utterance's expanded durations, on the host since the forward's one sync, and the delivered format
    std::vector<int64_t> durations;
    PcmFmtSpec spec;
};

namespace {
// the checked format of a FLAC stream: s16, not normalised (throws with the reason otherwise)
PcmFmtSpec flac_stream_spec(const sbv2_pcm_format* fmt) {
    const PcmFmtSpec spec = pcm_format_spec(fmt);
    SBV2_REQUIRE(spec.encoding == kEncS16, "FLAC needs encoding = 1 (s16): f32 samples and G.711 codes have no FLAC form");
    SBV2_REQUIRE(!spec.normalize, "a FLAC stream cannot normalise (normalize must be 0): the peak of the utterance is not known ahead");
    return spec;
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
    VitsBatch v = to_batch(batch);
    v.skip_decoder = true;
    pipeline_run_one(*bert->m, *vits->m, v, token_ids, s_lens, word2ph);
    std::unique_ptr<sbv2_stream> s(new sbv2_stream);
    s->bert = bert;
    s->vits = vits;
    s->chunk = chunk_frames;
    s->durations = vits->m->used_durations();
    s->frames = vits->m->stream_begin((int)chunk_frames);
    if (total_samples) *total_samples = s->frames * vits->m->cfg().hop();
    *out = s.release();
    API_END
}

// Next chunk of PCM (utterance order) -> dst (host, capacity samples; >= chunk_frames * hop always suffices).  *n = samples written,
// 0 once the utterance is complete.
int sbv2_stream_next(sbv2_stream* s, float* dst, int64_t capacity, int64_t* n) {
    API_BEGIN
    SBV2_REQUIRE(s && dst && n, "bad arguments");
    SBV2_REQUIRE(!s->level, "this stream was begun with a level: take its chunks with sbv2_stream_next_level");
    SBV2_REQUIRE(!s->flac, "this stream was begun as FLAC: take its chunks with sbv2_stream_next_flac");
    SBV2_REQUIRE(!s->formatted, "this stream was begun with an output format: take its chunks with sbv2_stream_next_format");
    *n = 0;
    if (s->next < s->frames) {
        *n = s->vits->m->stream_chunk(s->next, dst, capacity);
        s->next += s->chunk;
    }
    API_END
}

// Same as sbv2_stream_begin with the chunks leaving the device in `fmt` (formatted by one launch per decoder replay, vits.cpp stream_enqueue).
int sbv2_stream_begin_format(sbv2_bert* bert, sbv2_vits* vits, const sbv2_batch* batch, const int64_t* token_ids, const int64_t* s_lens,
                             const int64_t* word2ph, int64_t chunk_frames, const sbv2_pcm_format* fmt, sbv2_stream** out, int64_t* total_samples) {
    API_BEGIN
    SBV2_REQUIRE(bert && vits && batch && token_ids && s_lens && word2ph && out, "bad arguments");
    SBV2_REQUIRE(batch->n == 1, "sbv2_stream_begin_format takes one utterance");
    SBV2_REQUIRE(bert->m->device() == vits->m->device(), "bert and vits handles live on different devices");
    const PcmFmtSpec spec = pcm_format_spec(fmt);
    SBV2_REQUIRE(!spec.normalize, "a formatted stream cannot normalise (normalize must be 0): the peak of the utterance is not known ahead");
    VitsBatch v = to_batch(batch);
    v.skip_decoder = true;
    pipeline_run_one(*bert->m, *vits->m, v, token_ids, s_lens, word2ph);
    std::unique_ptr<sbv2_stream> s(new sbv2_stream);
    s->bert = bert;
    s->vits = vits;
    s->chunk = chunk_frames;
    s->durations = vits->m->used_durations();
    s->spec = spec;
    s->formatted = true;
    s->frames = vits->m->stream_begin((int)chunk_frames, &spec);
    if (total_samples) *total_samples = pcm_format_out_len(spec, s->frames * vits->m->cfg().hop());
    *out = s.release();
    API_END
}

int sbv2_stream_next_format(sbv2_stream* s, void* dst, int64_t capacity_bytes, int64_t* n) {
    API_BEGIN
    SBV2_REQUIRE(s && dst && n, "bad arguments");
    SBV2_REQUIRE(!s->level, "this stream was begun with a level: take its chunks with sbv2_stream_next_level");
    SBV2_REQUIRE(!s->flac, "this stream was begun as FLAC: take its chunks with sbv2_stream_next_flac");
    SBV2_REQUIRE(s->formatted, "this stream has no output format: take its chunks with sbv2_stream_next");
    *n = 0;
    if (s->next < s->frames) {
        *n = s->vits->m->stream_chunk_format(s->next, dst, capacity_bytes);
        s->next += s->chunk;
    }
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
// replay (vits.cpp stream_enqueue, flac_encode.hip FlacStreamEncoder).
int sbv2_stream_begin_flac(sbv2_bert* bert, sbv2_vits* vits, const sbv2_batch* batch, const int64_t* token_ids, const int64_t* s_lens,
                           const int64_t* word2ph, int64_t chunk_frames, const sbv2_pcm_format* fmt, sbv2_stream** out, int64_t* total_samples) {
    API_BEGIN
    SBV2_REQUIRE(bert && vits && batch && token_ids && s_lens && word2ph && out, "bad arguments");
    SBV2_REQUIRE(batch->n == 1, "sbv2_stream_begin_flac takes one utterance");
    SBV2_REQUIRE(bert->m->device() == vits->m->device(), "bert and vits handles live on different devices");
    const PcmFmtSpec spec = flac_stream_spec(fmt);
    VitsBatch v = to_batch(batch);
    v.skip_decoder = true;
    pipeline_run_one(*bert->m, *vits->m, v, token_ids, s_lens, word2ph);
    std::unique_ptr<sbv2_stream> s(new sbv2_stream);
    s->bert = bert;
    s->vits = vits;
    s->chunk = chunk_frames;
    s->durations = vits->m->used_durations();
    s->spec = spec;
    s->formatted = s->flac = true;
    s->frames = vits->m->stream_begin((int)chunk_frames, &spec, true);
    if (total_samples) *total_samples = pcm_format_out_len(spec, s->frames * vits->m->cfg().hop());
    *out = s.release();
    API_END
}

// The bytes of every FLAC frame that the next chunk's samples complete -> dst (host; the stream header in front on the first call).
// *n_samples = s16 samples the chunk consumed (0 once the utterance is complete), *n_bytes may be 0 while *n_samples > 0.
int sbv2_stream_next_flac(sbv2_stream* s, uint8_t* dst, int64_t capacity_bytes, int64_t* n_bytes, int64_t* n_samples) {
    API_BEGIN
    SBV2_REQUIRE(s && dst && n_bytes && n_samples, "bad arguments");
    SBV2_REQUIRE(!s->level, "this stream was begun with a level: take its chunks with sbv2_stream_next_level");
    SBV2_REQUIRE(s->flac, "this stream was not begun as FLAC: take its chunks with sbv2_stream_next or sbv2_stream_next_format");
    *n_bytes = *n_samples = 0;
    if (s->next < s->frames) {
        *n_samples = s->vits->m->stream_chunk_flac(s->next, dst, capacity_bytes, n_bytes);
        s->next += s->chunk;
    }
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
// the cast / quantiser (vits.cpp stream_enqueue, limiter.hip StreamLimiter).
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
    VitsBatch v = to_batch(batch);
    v.skip_decoder = true;
    pipeline_run_one(*bert->m, *vits->m, v, token_ids, s_lens, word2ph);
    std::unique_ptr<sbv2_stream> s(new sbv2_stream);
    s->bert = bert;
    s->vits = vits;
    s->chunk = chunk_frames;
    s->durations = vits->m->used_durations();
    s->spec = spec;
    s->formatted = s->level = true;
    s->flac = flac != 0;
    s->frames = vits->m->stream_begin((int)chunk_frames, &spec, flac != 0, &lv);
    if (total_samples) *total_samples = pcm_format_out_len(spec, s->frames * vits->m->cfg().hop());
    *out = s.release();
    API_END
}

// What the next chunk completes -> dst (host): *n_out samples in the stream's encoding, or with FLAC the *n_out bytes of the frames that
// those samples complete (the stream header in front on the first call).  *n_consumed = samples of the chunk taken, 0 once the utterance
// is complete; *n_out may be 0 while *n_consumed > 0.
int sbv2_stream_next_level(sbv2_stream* s, void* dst, int64_t capacity_bytes, int64_t* n_out, int64_t* n_consumed) {
    API_BEGIN
    SBV2_REQUIRE(s && dst && n_out && n_consumed, "bad arguments");
    SBV2_REQUIRE(s->level, "this stream was not begun with a level: take its chunks with the sbv2_stream_next call of its kind");
    if (s->next < s->frames) {
        int64_t out = 0;
        const int64_t taken = s->vits->m->stream_chunk_level(s->next, dst, capacity_bytes, &out);
        *n_out = out;
        *n_consumed = taken;
        s->next += s->chunk;
    } else {
        *n_out = *n_consumed = 0;
    }
    API_END
}

// 20 log10 min s (the deepest reduction, <= 0) and max |x| (before the cast / quantiser) over the utterance, once its last chunk was taken
int sbv2_stream_level_stats(sbv2_stream* s, double* stats) {
    API_BEGIN
    SBV2_REQUIRE(s && stats, "bad arguments");
    SBV2_REQUIRE(s->level, "this stream was not begun with a level");
    SBV2_REQUIRE(s->next >= s->frames, "the level stats exist once the stream is complete: take its chunks to the end first");
    s->vits->m->stream_level_stats(stats);
    API_END
}

// Host only: the token spans of the stream's utterance at its delivered rate (marks.h; place 0).  Every duration is known once _begin* has
// returned, so the whole timing is there before the first chunk is decoded.
int sbv2_stream_marks(sbv2_stream* s, int64_t* tok_start, int64_t* tok_end, int64_t capacity, int64_t* n_tokens) {
    API_BEGIN
    SBV2_REQUIRE(s && n_tokens, "bad arguments");
    const int64_t n = (int64_t)s->durations.size();
    SBV2_REQUIRE(capacity >= n, "token arrays too small: " + std::to_string(capacity) + " < " + std::to_string(n) + " tokens");
    SBV2_REQUIRE(n == 0 || (tok_start && tok_end), "bad arguments");
    marks_spans(s->durations.data(), n, s->vits->m->cfg().hop(), 0, s->spec, tok_start, tok_end);
    *n_tokens = n;
    API_END
}

// 1 when the decoder of this stream replays a captured hipGraph (0: eager launches, SBV2_STREAM_GRAPH=0)
int sbv2_stream_uses_graph(const sbv2_stream* s) { return s && s->vits->m->stream_graph_captured() ? 1 : 0; }
// device workspace of the chunk decoder in bytes (bounded by the window, whatever the utterance length)
int64_t sbv2_stream_workspace_bytes(const sbv2_stream* s) { return s ? (int64_t)s->vits->m->stream_workspace_bytes() : -1; }

void sbv2_stream_end(sbv2_stream* s) { delete s; }

}  // extern "C"
