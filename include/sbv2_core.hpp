// sbv2_core.hpp — C++ host mirror of the reference's operator interface for the hot path, above the C ABI of sbv2_hip.h.
//
// The reference is Rust (crates/sbv2_core); no Rust toolchain exists in the build image, so the host side that a Rust shim would
// provide is mirrored here in C++ with the same names, argument order, shapes and error behaviour:
//
//   reference (file:line)                                              here
//   model::load_model(model_file, bert) -> Result<Session>   model.rs:6   sbv2_core::load_model(bytes, len, bert[, device]) -> Session
//   bert::predict(&mut Session, ids, masks) -> Array2<f32>   bert.rs:6    sbv2_core::predict(Session&, ids, masks) -> Array2f [S, 1024]
//   model::synthesize(&mut Session, bert_ori, x_tst, sid, tones, lang_ids, style_vector, sdp_ratio, length_scale, noise_scale,
//                     noise_scale_w) -> Array3<f32>          model.rs:53  sbv2_core::synthesize(...) -> Array3f [1, 1, L]
//   error::Error (ORT failures -> OrtError, others -> OtherError(String))  error.rs:6-31   sbv2_core::Error (what() = sbv2_last_error())
//
// Header only; link with libsbv2_hip.so.  A Session is move-only and used by one caller at a time (`&mut Session`).
#ifndef SBV2_CORE_HPP
#define SBV2_CORE_HPP

#include <cstdint>
#include <random>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "sbv2_hip.h"

namespace sbv2_core {

// Result<T, Error> of the reference becomes an exception; the message is the library's (error.rs:29-30 OtherError(String)).
struct Error : std::runtime_error {
    using std::runtime_error::runtime_error;
};
inline void check(int rc) {
    if (rc != 0) throw Error(sbv2_last_error());
}

// row-major owned arrays with ndarray's shapes
struct Array2f {
    std::vector<float> data;
    size_t rows = 0, cols = 0;
    float& operator()(size_t r, size_t c) { return data[r * cols + c]; }
    float operator()(size_t r, size_t c) const { return data[r * cols + c]; }
};
struct Array3f {
    std::vector<float> data;
    size_t d0 = 0, d1 = 0, d2 = 0;
};

class Session {
  public:
    Session() = default;
    Session(Session&& o) noexcept { *this = std::move(o); }
    Session& operator=(Session&& o) noexcept {
        if (this != &o) {
            reset();
            bert_ = o.bert_;
            vits_ = o.vits_;
            o.bert_ = nullptr;
            o.vits_ = nullptr;
        }
        return *this;
    }
    Session(const Session&) = delete;
    Session& operator=(const Session&) = delete;
    ~Session() { reset(); }
    bool is_bert() const { return bert_ != nullptr; }
    sbv2_bert* bert() const { return bert_; }
    sbv2_vits* vits() const { return vits_; }

  private:
    friend Session load_model(const uint8_t*, size_t, bool, int);
    void reset() {
        if (bert_) sbv2_bert_destroy(bert_);
        if (vits_) sbv2_vits_destroy(vits_);
        bert_ = nullptr;
        vits_ = nullptr;
    }
    sbv2_bert* bert_ = nullptr;
    sbv2_vits* vits_ = nullptr;
};

// model.rs:6-50.  `bert` selects which of the two graphs the bytes hold, as in the reference (it only changes session options there).
inline Session load_model(const uint8_t* model_file, size_t len, bool bert, int device = 0) {
    Session s;
    if (bert) check(sbv2_bert_create(model_file, len, device, &s.bert_));
    else check(sbv2_vits_create(model_file, len, device, &s.vits_));
    return s;
}
inline Session load_model(const std::vector<uint8_t>& model_file, bool bert, int device = 0) {
    return load_model(model_file.data(), model_file.size(), bert, device);
}

// bert.rs:6-24: token_ids and attention_masks of one sentence -> [S, hidden]
inline Array2f predict(Session& session, const std::vector<int64_t>& token_ids, const std::vector<int64_t>& attention_masks) {
    if (!session.is_bert()) throw Error("predict: the session does not hold the BERT graph");
    if (token_ids.size() != attention_masks.size()) throw Error("predict: token_ids and attention_masks differ in length");
    Array2f out;
    out.rows = token_ids.size();
    out.cols = (size_t)sbv2_bert_hidden(session.bert());
    out.data.resize(out.rows * out.cols);
    check(sbv2_bert_predict(session.bert(), token_ids.data(), attention_masks.data(), (int64_t)token_ids.size(), out.data.data()));
    return out;
}

// model.rs:53-111: bert_ori [1024, T]; x_tst, tones, lang_ids i64[T]; sid i64[1]; style_vector f32[256] -> [1, 1, L].
// noise_seed is not part of the reference signature: it selects the counter-based stream standing in for the graph's RandomNormalLike.
// Like the reference (ONNX Runtime draws fresh noise on every run) the default is a fresh seed per call; pass one for reproducible output.
inline uint64_t fresh_noise_seed() {
    static std::random_device rd;
    return ((uint64_t)rd() << 32) ^ (uint64_t)rd();
}
inline Array3f synthesize(Session& session, const Array2f& bert_ori, const std::vector<int64_t>& x_tst, const std::vector<int64_t>& sid,
                          const std::vector<int64_t>& tones, const std::vector<int64_t>& lang_ids, const std::vector<float>& style_vector,
                          float sdp_ratio, float length_scale, float noise_scale, float noise_scale_w, uint64_t noise_seed = fresh_noise_seed()) {
    if (session.is_bert() || !session.vits()) throw Error("synthesize: the session does not hold the VITS graph");
    const size_t T = x_tst.size();
    if (bert_ori.cols != T || tones.size() != T || lang_ids.size() != T) throw Error("synthesize: sequence lengths differ");
    if (bert_ori.rows != (size_t)sbv2_vits_bert_dim(session.vits())) throw Error("synthesize: bert_ori must be [bert_dim, T]");
    if (style_vector.size() != (size_t)sbv2_vits_style_dim(session.vits())) throw Error("synthesize: style_vector has the wrong length");
    if (sid.size() != 1) throw Error("synthesize: sid must hold one speaker id");
    float* pcm = nullptr;
    int64_t len = 0;
    check(sbv2_vits_synthesize(session.vits(), bert_ori.data.data(), x_tst.data(), tones.data(), lang_ids.data(), (int64_t)T, sid[0],
                               style_vector.data(), sdp_ratio, length_scale, noise_scale, noise_scale_w, noise_seed, &pcm, &len));
    Array3f out;
    out.d0 = out.d1 = 1;
    out.d2 = (size_t)len;
    out.data.assign(pcm, pcm + len);   // the reference copies into an owned Array3 as well (model.rs:108)
    sbv2_pcm_free(pcm);
    return out;
}

// Not in the reference: per-token pitch targets of a fetched request (sbv2_token_pitch in sbv2_hip.h states them).  values: one per token of the
// listed rows in marks order, 0 = not edited; hz: targets in Hz, else ratios; smooth: contour frames to each side.  applied / src_f0 are filled
// by fetch_request_token_pitch.
struct TokenPitch {
    std::vector<double> values;
    bool hz = true;
    int smooth = 2;
    std::vector<double> applied, src_f0;
};
// sbv2_pipeline_fetch_request_token_pitch with owned arrays: voice, track, dynamics, marks and pitch may each be NULL as there.
inline void fetch_request_token_pitch(sbv2_pipeline* p, int64_t ticket, const sbv2_fetch_request& req, const sbv2_voice* voice,
                                      const sbv2_pitch_track* track, const sbv2_dynamics* dynamics, TokenPitch& tp, void* dst, int64_t capacity_bytes,
                                      int64_t* out_count, double* stats = nullptr, double* dyn_stats = nullptr, sbv2_marks* marks = nullptr,
                                      sbv2_pitch* pitch = nullptr) {
    tp.applied.assign(tp.values.size(), 1.0);
    tp.src_f0.assign(tp.values.size(), 0.0);
    const sbv2_token_pitch c{tp.values.data(), (int64_t)tp.values.size(), tp.hz ? 1 : 0, tp.smooth, tp.applied.data(), tp.src_f0.data(), 0};
    check(sbv2_pipeline_fetch_request_token_pitch(p, ticket, &req, voice, track, dynamics, &c, dst, capacity_bytes, out_count, stats, dyn_stats, marks,
                                                  pitch));
}

// Not in the reference: the formant scale of a fetched request (sbv2_formant in sbv2_hip.h states it).  sbv2_pipeline_fetch_request_formant with
// owned arrays: fetch_request_token_pitch with formant_scale behind the table; 1 is exactly that call.
inline void fetch_request_formant(sbv2_pipeline* p, int64_t ticket, const sbv2_fetch_request& req, const sbv2_voice* voice,
                                  const sbv2_pitch_track* track, const sbv2_dynamics* dynamics, TokenPitch* tp, double formant_scale, void* dst,
                                  int64_t capacity_bytes, int64_t* out_count, double* stats = nullptr, double* dyn_stats = nullptr,
                                  sbv2_marks* marks = nullptr, sbv2_pitch* pitch = nullptr) {
    sbv2_token_pitch c{};
    if (tp) {
        tp->applied.assign(tp->values.size(), 1.0);
        tp->src_f0.assign(tp->values.size(), 0.0);
        c = sbv2_token_pitch{tp->values.data(), (int64_t)tp->values.size(), tp->hz ? 1 : 0, tp->smooth, tp->applied.data(), tp->src_f0.data(), 0};
    }
    const sbv2_formant f{formant_scale, 0.0};
    check(sbv2_pipeline_fetch_request_formant(p, ticket, &req, voice, track, dynamics, tp ? &c : nullptr, &f, dst, capacity_bytes, out_count, stats,
                                              dyn_stats, marks, pitch));
}

// Not in the reference (upstream Style-Bert-VITS2's assist_text / assist_text_weight; sbv2_assist in sbv2_hip.h states it): assist texts of a run
// with owned arrays.  texts: the distinct assist sequences' token ids; text_of / weight: one entry per row of the batch (-1 = none).
struct Assist {
    std::vector<std::vector<int64_t>> texts;
    std::vector<int32_t> text_of;
    std::vector<double> weight;
    // the C struct over flat copies that live as long as this object is not changed
    const sbv2_assist* c_struct() {
        ids_.clear();
        lens_.clear();
        for (const auto& t : texts) {
            ids_.insert(ids_.end(), t.begin(), t.end());
            lens_.push_back((int64_t)t.size());
        }
        c_ = sbv2_assist{(int64_t)texts.size(), ids_.data(), lens_.data(), text_of.data(), weight.data(), 0};
        return &c_;
    }

  private:
    std::vector<int64_t> ids_, lens_;
    sbv2_assist c_{};
};
// sbv2_pipeline_run_assist: sbv2_pipeline_run_opts with the rows' assist texts; assist == nullptr is exactly that call.
inline void pipeline_run_assist(sbv2_pipeline* p, const sbv2_batch& batch, const sbv2_utt_options* opts, Assist* assist, const int64_t* token_ids,
                                const int64_t* s_lens, const int64_t* word2ph, int64_t* pcm_lens) {
    check(sbv2_pipeline_run_assist(p, &batch, opts, assist ? assist->c_struct() : nullptr, token_ids, s_lens, word2ph, pcm_lens));
}
// sbv2_stream_begin_request_assist: sbv2_stream_begin_request_pitch with the rows' assist texts; assist == nullptr is exactly that call.
inline sbv2_stream* stream_begin_request_assist(sbv2_bert* bert, sbv2_vits* vits, const sbv2_batch& batch, const sbv2_utt_options* opts, Assist* assist,
                                                const int64_t* token_ids, const int64_t* s_lens, const int64_t* word2ph, int64_t chunk_frames,
                                                const sbv2_stream_request& rq, const sbv2_stream_levels* lv = nullptr,
                                                const sbv2_stream_pitch* sp = nullptr, int64_t* total_samples = nullptr, int64_t* n_tokens = nullptr,
                                                int64_t* n_env = nullptr, int64_t* n_pitch = nullptr) {
    sbv2_stream* s = nullptr;
    check(sbv2_stream_begin_request_assist(bert, vits, &batch, opts, assist ? assist->c_struct() : nullptr, token_ids, s_lens, word2ph, chunk_frames, &rq,
                                           lv, sp, &s, total_samples, n_tokens, n_env, n_pitch));
    return s;
}
// (the kernels on their own are the test hook sbv2_debug_assist_blend of sbv2_hip.h: plain arrays in, plain arrays out, nothing to own here)

// Not in the reference (sbv2_stream_voice in sbv2_hip.h states it): pitch, intonation and formant scale of a request STREAM about the pivots the
// caller names, with the pivots owned.  pivot_hz: one entry per row of the batch.
struct StreamVoice {
    double pitch_scale = 1.0, intonation_scale = 1.0, formant_scale = 1.0;
    std::vector<double> pivot_hz;
    double f0_min = 0.0, f0_max = 0.0, threshold = 0.0;   // 0 = 70, 600, 0.15
    int32_t hop = 0;                                       // 0 = rate / 200
    // the C struct over this object's pivots, valid as long as it is not changed
    const sbv2_stream_voice* c_struct() {
        c_ = sbv2_stream_voice{sbv2_voice{pitch_scale, intonation_scale, f0_min, f0_max, threshold, hop, 0}, formant_scale,
                               pivot_hz.empty() ? nullptr : pivot_hz.data(), {0.0, 0.0}};
        return &c_;
    }
    // A_v at a rate (sbv2_stream_voice_lookahead; throws on parameters the begin call refuses)
    int64_t lookahead(int32_t sample_rate = 44100) {
        const int64_t a = sbv2_stream_voice_lookahead(c_struct(), sample_rate);
        if (a < 0) check(1);
        return a;
    }

  private:
    sbv2_stream_voice c_{};
};
// sbv2_stream_begin_request_voice: sbv2_stream_begin_request_assist with the voice shifted on the way; voice == nullptr is exactly that call.
// The chunks of a voice stream are taken with sbv2_stream_next_level (delivery runs behind them).
inline sbv2_stream* stream_begin_request_voice(sbv2_bert* bert, sbv2_vits* vits, const sbv2_batch& batch, const sbv2_utt_options* opts, Assist* assist,
                                               const int64_t* token_ids, const int64_t* s_lens, const int64_t* word2ph, int64_t chunk_frames,
                                               const sbv2_stream_request& rq, StreamVoice* voice, const sbv2_stream_levels* lv = nullptr,
                                               const sbv2_stream_pitch* sp = nullptr, int64_t* total_samples = nullptr, int64_t* n_tokens = nullptr,
                                               int64_t* n_env = nullptr, int64_t* n_pitch = nullptr) {
    sbv2_stream* s = nullptr;
    check(sbv2_stream_begin_request_voice(bert, vits, &batch, opts, assist ? assist->c_struct() : nullptr, token_ids, s_lens, word2ph, chunk_frames, &rq,
                                          lv, sp, voice ? voice->c_struct() : nullptr, &s, total_samples, n_tokens, n_env, n_pitch));
    return s;
}
// every call's delivered count of a voice stream without a level (sbv2_stream_voice_timeline)
inline std::vector<int64_t> stream_voice_timeline(const std::vector<int64_t>& frames, const std::vector<int64_t>& gap_after, int32_t hop,
                                                  int64_t chunk_frames, const sbv2_pcm_format* fmt, StreamVoice& voice) {
    int64_t calls = 0;
    check(sbv2_stream_voice_timeline(frames.data(), gap_after.data(), (int64_t)frames.size(), hop, chunk_frames, fmt, voice.c_struct(), nullptr, 0, &calls));
    std::vector<int64_t> out((size_t)calls);
    check(sbv2_stream_voice_timeline(frames.data(), gap_after.data(), (int64_t)frames.size(), hop, chunk_frames, fmt, voice.c_struct(), out.data(), calls,
                                     &calls));
    return out;
}

// Not in the reference (sbv2_stream_leveler in sbv2_hip.h states it): a loudness target followed on a request STREAM, from the gain_db of the
// request's level towards target_lufs - (the gated loudness heard so far).  The defaults are the usual values.
struct StreamLeveler {
    double target_lufs = -16.0, range_db = 12.0, slew_db_per_s = 3.0;
    int32_t hold_blocks = 10;
    sbv2_stream_leveler c_struct() const { return sbv2_stream_leveler{target_lufs, range_db, slew_db_per_s, hold_blocks, 0}; }
};
// sbv2_stream_begin_request_leveler: sbv2_stream_begin_request_voice with the leveler in front of the level's limiter (rq.level must be set);
// leveler == nullptr is exactly that call.  The chunks are taken with sbv2_stream_next_level.
inline sbv2_stream* stream_begin_request_leveler(sbv2_bert* bert, sbv2_vits* vits, const sbv2_batch& batch, const sbv2_utt_options* opts, Assist* assist,
                                                 const int64_t* token_ids, const int64_t* s_lens, const int64_t* word2ph, int64_t chunk_frames,
                                                 const sbv2_stream_request& rq, StreamVoice* voice, const StreamLeveler* leveler,
                                                 const sbv2_stream_levels* lv = nullptr, const sbv2_stream_pitch* sp = nullptr,
                                                 int64_t* total_samples = nullptr, int64_t* n_tokens = nullptr, int64_t* n_env = nullptr,
                                                 int64_t* n_pitch = nullptr) {
    sbv2_stream* s = nullptr;
    sbv2_stream_leveler c{};
    if (leveler) c = leveler->c_struct();
    check(sbv2_stream_begin_request_leveler(bert, vits, &batch, opts, assist ? assist->c_struct() : nullptr, token_ids, s_lens, word2ph, chunk_frames, &rq,
                                            lv, sp, voice ? voice->c_struct() : nullptr, leveler ? &c : nullptr, &s, total_samples, n_tokens, n_env,
                                            n_pitch));
    return s;
}
// (L_in, last g, min g, max g, deepest reduction in dB, max |x|) of a levelled stream, once its last chunk was taken
inline std::vector<double> stream_leveler_stats(sbv2_stream* s) {
    std::vector<double> st(6);
    check(sbv2_stream_leveler_stats(s, st.data()));
    return st;
}

}  // namespace sbv2_core

#endif
