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

// Not in the reference: per-token volume targets of a fetched request (sbv2_token_gain in sbv2_hip.h states them).  values: one per token of the
// listed rows in marks order, 0 = not edited; rms: target RMS (full scale = 1.0), else amplitude ratios; ramp: native samples about a token
// boundary; every factor within [1 / max_ratio, max_ratio].  applied / src_rms are filled by fetch_request_token_gain.
struct TokenGain {
    std::vector<double> values;
    bool rms = false;
    int64_t ramp = 441;
    double max_ratio = 4.0;
    std::vector<double> applied, src_rms;
};
// sbv2_pipeline_fetch_request_token_gain with owned arrays: the widest request fetch with the table behind it; everything else may be NULL as
// there (contour with formant_track, as sbv2_pipeline_fetch_request_formant_track has it).
inline void fetch_request_token_gain(sbv2_pipeline* p, int64_t ticket, const sbv2_fetch_request& req, const sbv2_voice* voice,
                                     const sbv2_pitch_track* track, const sbv2_dynamics* dynamics, const sbv2_token_pitch* token_pitch,
                                     const sbv2_formant* formant, TokenGain& tg, void* dst, int64_t capacity_bytes, int64_t* out_count,
                                     double* stats = nullptr, double* dyn_stats = nullptr, sbv2_marks* marks = nullptr, sbv2_pitch* pitch = nullptr,
                                     sbv2_spectrum* spectrum = nullptr, sbv2_formant_contour* contour = nullptr,
                                     const sbv2_formant_track* formant_track = nullptr) {
    tg.applied.assign(tg.values.size(), 1.0);
    tg.src_rms.assign(tg.values.size(), 0.0);
    const sbv2_token_gain c{tg.values.data(), (int64_t)tg.values.size(), tg.ramp, tg.max_ratio, tg.rms ? 1 : 0, 0, tg.applied.data(), tg.src_rms.data()};
    check(sbv2_pipeline_fetch_request_token_gain(p, ticket, &req, voice, track, dynamics, token_pitch, formant, dst, capacity_bytes, out_count, stats,
                                                 dyn_stats, marks, pitch, spectrum, contour, formant_track, &c));
}

// Not in the reference: a parametric EQ of a fetched request (sbv2_eq in sbv2_hip.h states it).  bands: at most 8, run in the given order; kind
// 0 high-pass, 1 low-pass, 2 low shelf, 3 high shelf, 4 peak.
struct Eq {
    struct Band {
        int kind = 4;
        double f0_hz = 1000.0, gain_db = 0.0, q = 0.70710678118654752;
    };
    std::vector<Band> bands;
    sbv2_eq c() const {   // (more than 8 bands: n_bands says so and the library refuses it)
        sbv2_eq e{};
        e.n_bands = (int32_t)bands.size();
        for (size_t i = 0; i < bands.size() && i < SBV2_EQ_MAX_BANDS; ++i)
            e.kind[i] = bands[i].kind, e.f0_hz[i] = bands[i].f0_hz, e.gain_db[i] = bands[i].gain_db, e.q[i] = bands[i].q;
        return e;
    }
};
// sbv2_pipeline_fetch_request_eq with owned arrays: the widest request fetch, the EQ behind the token gain (tg NULL: none); everything else may
// be NULL as in fetch_request_token_gain.
inline void fetch_request_eq(sbv2_pipeline* p, int64_t ticket, const sbv2_fetch_request& req, const sbv2_voice* voice, const sbv2_pitch_track* track,
                             const sbv2_dynamics* dynamics, const sbv2_token_pitch* token_pitch, const sbv2_formant* formant, TokenGain* tg,
                             const Eq& eq, void* dst, int64_t capacity_bytes, int64_t* out_count, double* stats = nullptr,
                             double* dyn_stats = nullptr, sbv2_marks* marks = nullptr, sbv2_pitch* pitch = nullptr, sbv2_spectrum* spectrum = nullptr,
                             sbv2_formant_contour* contour = nullptr, const sbv2_formant_track* formant_track = nullptr) {
    sbv2_token_gain g{};
    if (tg) {
        tg->applied.assign(tg->values.size(), 1.0);
        tg->src_rms.assign(tg->values.size(), 0.0);
        g = sbv2_token_gain{tg->values.data(), (int64_t)tg->values.size(), tg->ramp, tg->max_ratio, tg->rms ? 1 : 0, 0, tg->applied.data(), tg->src_rms.data()};
    }
    const sbv2_eq e = eq.c();
    check(sbv2_pipeline_fetch_request_eq(p, ticket, &req, voice, track, dynamics, token_pitch, formant, dst, capacity_bytes, out_count, stats, dyn_stats,
                                         marks, pitch, spectrum, contour, formant_track, tg ? &g : nullptr, &e));
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

// Not in the reference: the spectrum of a fetched request (sbv2_spectrum in sbv2_hip.h states it).  n_mels = 0: the n_fft / 2 + 1 bins; f_max
// <= 0: half the delivered rate.  power [n_frames][n_bands] is filled by fetch_request_spectrum.
struct Spectrum {
    int n_fft = 400, hop = 160, n_mels = 80;
    double f_min = 0.0, f_max = 0.0;
    std::vector<float> power;
    int64_t n_frames = 0;
    int n_bands = 0;
};
// sbv2_pipeline_fetch_request_spectrum with owned arrays: fetch_request_formant with the spectrum of the delivered signal behind it.  out_len =
// the delivered samples of the request (sbv2_pcm_format_length of its joined_len), which sizes the array.
inline void fetch_request_spectrum(sbv2_pipeline* p, int64_t ticket, const sbv2_fetch_request& req, const sbv2_voice* voice,
                                   const sbv2_pitch_track* track, const sbv2_dynamics* dynamics, TokenPitch* tp, double formant_scale, Spectrum& sp,
                                   void* dst, int64_t capacity_bytes, int64_t* out_count, double* stats = nullptr, double* dyn_stats = nullptr,
                                   sbv2_marks* marks = nullptr, sbv2_pitch* pitch = nullptr) {
    sbv2_token_pitch c{};
    if (tp) {
        tp->applied.assign(tp->values.size(), 1.0);
        tp->src_f0.assign(tp->values.size(), 0.0);
        c = sbv2_token_pitch{tp->values.data(), (int64_t)tp->values.size(), tp->hz ? 1 : 0, tp->smooth, tp->applied.data(), tp->src_f0.data(), 0};
    }
    const sbv2_formant f{formant_scale, 0.0};
    const int rate = req.fmt ? req.fmt->sample_rate : 44100;
    sbv2_spectrum s{sp.n_fft, sp.hop, sp.n_mels, 0, sp.f_min, sp.f_max > 0.0 ? sp.f_max : rate / 2.0, 0, nullptr, 0, 0};
    check(sbv2_spectrum_bands(rate, &s, nullptr));   // the ranges, and n_bands
    const int64_t out_len = sbv2_pcm_format_length(req.fmt, req.joined_len);
    if (out_len < 0) throw Error(sbv2_last_error());
    sp.power.assign((size_t)((out_len + sp.hop - 1) / sp.hop) * s.n_bands + 1, 0.0f);
    s.capacity = (int64_t)sp.power.size();
    s.power = sp.power.data();
    check(sbv2_pipeline_fetch_request_spectrum(p, ticket, &req, voice, track, dynamics, tp ? &c : nullptr, &f, dst, capacity_bytes, out_count, stats,
                                               dyn_stats, marks, pitch, &s));
    sp.n_frames = s.n_frames;
    sp.n_bands = s.n_bands;
    sp.power.resize((size_t)(s.n_frames * s.n_bands));
}

// Not in the reference: the formant contour of a fetched request (sbv2_formant_contour in sbv2_hip.h states it).  window / order / f_lo / f_hi /
// bw_max 0: the defaults at the delivered rate, which fetch_request_formant_contour writes back.  f_hz / bw_hz [n_frames][n_formants] and
// status [n_frames] are filled by it.
struct FormantContour {
    int hop = 160, window = 0, order = 0, n_formants = 4;
    double f_lo = 0.0, f_hi = 0.0, bw_max = 0.0;
    std::vector<double> f_hz, bw_hz;
    std::vector<int32_t> status;
    int64_t n_frames = 0;
};
// Not in the reference: tracking of that contour across frames (sbv2_formant_track in sbv2_hip.h states it).  ref_hz holds one reference per track
// (1 to 5, strictly ascending); FormantContour::n_formants must equal their number.
struct FormantTrack {
    std::vector<double> ref_hz{500.0, 1500.0, 2500.0};
    int candidates = 6;
    double freq_cost = 1.0, bw_cost = 1.0, jump_cost = 4.0;
    sbv2_formant_track c_struct() const {
        sbv2_formant_track t{};
        t.n_tracks = (int32_t)ref_hz.size(), t.candidates = candidates;
        for (size_t i = 0; i < ref_hz.size() && i < 5; ++i) t.ref_hz[i] = ref_hz[i];
        t.freq_cost = freq_cost, t.bw_cost = bw_cost, t.jump_cost = jump_cost;
        return t;
    }
};
// sbv2_pipeline_fetch_request_formant_track with owned arrays: the call below with the contour tracked (ft == nullptr: exactly the call below).
inline void fetch_request_formant_track(sbv2_pipeline* p, int64_t ticket, const sbv2_fetch_request& req, const sbv2_voice* voice,
                                        const sbv2_pitch_track* track, const sbv2_dynamics* dynamics, const sbv2_token_pitch* token_pitch,
                                        const sbv2_formant* formant, FormantContour& fc, const FormantTrack* ft, void* dst, int64_t capacity_bytes,
                                        int64_t* out_count, double* stats = nullptr, double* dyn_stats = nullptr, sbv2_marks* marks = nullptr,
                                        sbv2_pitch* pitch = nullptr, sbv2_spectrum* spectrum = nullptr);
// sbv2_pipeline_fetch_request_formant_contour with owned arrays: sbv2_pipeline_fetch_request_formant (no spectrum) with the formant contour of
// the delivered signal behind it.
inline void fetch_request_formant_contour(sbv2_pipeline* p, int64_t ticket, const sbv2_fetch_request& req, const sbv2_voice* voice,
                                          const sbv2_pitch_track* track, const sbv2_dynamics* dynamics, const sbv2_token_pitch* token_pitch,
                                          const sbv2_formant* formant, FormantContour& fc, void* dst, int64_t capacity_bytes, int64_t* out_count,
                                          double* stats = nullptr, double* dyn_stats = nullptr, sbv2_marks* marks = nullptr,
                                          sbv2_pitch* pitch = nullptr, sbv2_spectrum* spectrum = nullptr) {
    fetch_request_formant_track(p, ticket, req, voice, track, dynamics, token_pitch, formant, fc, nullptr, dst, capacity_bytes, out_count, stats, dyn_stats,
                                marks, pitch, spectrum);
}
inline void fetch_request_formant_track(sbv2_pipeline* p, int64_t ticket, const sbv2_fetch_request& req, const sbv2_voice* voice,
                                        const sbv2_pitch_track* track, const sbv2_dynamics* dynamics, const sbv2_token_pitch* token_pitch,
                                        const sbv2_formant* formant, FormantContour& fc, const FormantTrack* ft, void* dst, int64_t capacity_bytes,
                                        int64_t* out_count, double* stats, double* dyn_stats, sbv2_marks* marks, sbv2_pitch* pitch,
                                        sbv2_spectrum* spectrum) {
    const int rate = req.fmt ? req.fmt->sample_rate : 44100;
    const int64_t out_len = sbv2_pcm_format_length(req.fmt, req.joined_len);
    if (out_len < 0) throw Error(sbv2_last_error());
    sbv2_formant_contour c{fc.hop, fc.window, fc.order, fc.n_formants, fc.f_lo, fc.f_hi, fc.bw_max, 0, 0, nullptr, nullptr, nullptr, out_len};
    check(sbv2_formant_contour_defaults(rate, &c));   // the ranges, the defaults, and n_frames of out_len
    fc.window = c.window, fc.order = c.order, fc.f_lo = c.f_lo, fc.f_hi = c.f_hi, fc.bw_max = c.bw_max;
    const size_t nf = (size_t)c.n_frames;
    fc.f_hz.assign(nf * fc.n_formants + 1, 0.0);
    fc.bw_hz.assign(nf * fc.n_formants + 1, 0.0);
    fc.status.assign(nf + 1, 0);
    c.capacity = (int64_t)nf;
    c.f_hz = fc.f_hz.data(), c.bw_hz = fc.bw_hz.data(), c.status = fc.status.data();
    sbv2_formant_track t{};
    if (ft) t = ft->c_struct();
    check(sbv2_pipeline_fetch_request_formant_track(p, ticket, &req, voice, track, dynamics, token_pitch, formant, dst, capacity_bytes, out_count, stats,
                                                    dyn_stats, marks, pitch, spectrum, &c, ft ? &t : nullptr));
    fc.n_frames = c.n_frames;
    fc.f_hz.resize(nf * fc.n_formants), fc.bw_hz.resize(nf * fc.n_formants), fc.status.resize(nf);
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

// Not in the reference (sbv2_stream_spectrum in sbv2_hip.h states it): the spectrum of a request STREAM's delivered samples, frame by frame.
struct StreamSpectrum {
    int32_t n_fft = 400, hop = 160, n_mels = 80;
    double f_min = 0.0, f_max = 8000.0;
    int64_t n_frames = 0;   // out, set by stream_begin_request_spectrum: ceil(total_samples / hop)
    int32_t n_bands = 0;    // out: n_mels, or n_fft / 2 + 1
    sbv2_stream_spectrum c_struct() const { return sbv2_stream_spectrum{n_fft, hop, n_mels, 0, f_min, f_max}; }
};
// sbv2_stream_begin_request_spectrum: sbv2_stream_begin_request_leveler with the spectrum of the delivered samples; spectrum == nullptr is
// exactly that call.
inline sbv2_stream* stream_begin_request_spectrum(sbv2_bert* bert, sbv2_vits* vits, const sbv2_batch& batch, const sbv2_utt_options* opts, Assist* assist,
                                                  const int64_t* token_ids, const int64_t* s_lens, const int64_t* word2ph, int64_t chunk_frames,
                                                  const sbv2_stream_request& rq, StreamVoice* voice, const StreamLeveler* leveler,
                                                  StreamSpectrum* spectrum, const sbv2_stream_levels* lv = nullptr,
                                                  const sbv2_stream_pitch* sp = nullptr, int64_t* total_samples = nullptr, int64_t* n_tokens = nullptr,
                                                  int64_t* n_env = nullptr, int64_t* n_pitch = nullptr) {
    sbv2_stream* s = nullptr;
    sbv2_stream_leveler c{};
    sbv2_stream_spectrum q{};
    if (leveler) c = leveler->c_struct();
    if (spectrum) q = spectrum->c_struct();
    int64_t n_spec = 0;
    int32_t n_bands = 0;
    check(sbv2_stream_begin_request_spectrum(bert, vits, &batch, opts, assist ? assist->c_struct() : nullptr, token_ids, s_lens, word2ph, chunk_frames,
                                             &rq, lv, sp, voice ? voice->c_struct() : nullptr, leveler ? &c : nullptr, spectrum ? &q : nullptr, &s,
                                             total_samples, n_tokens, n_env, n_pitch, &n_spec, &n_bands));
    if (spectrum) spectrum->n_frames = n_spec, spectrum->n_bands = n_bands;
    return s;
}
// sbv2_stream_next_spectrum: the frames completed since the previous call, appended to power ([frames][n_bands]); returns how many
inline int64_t stream_next_spectrum(sbv2_stream* s, const StreamSpectrum& spectrum, std::vector<float>* power) {
    const size_t at = power->size();
    power->resize(at + (size_t)(spectrum.n_frames * spectrum.n_bands));   // (room for everything that can be pending)
    sbv2_stream_spectrum_part part{spectrum.n_frames * spectrum.n_bands, power->data() + at, 0, 0, 0};
    const int rc = sbv2_stream_next_spectrum(s, &part);
    power->resize(at + (rc == 0 ? (size_t)(part.n * spectrum.n_bands) : 0));
    check(rc);
    return part.n;
}

// Not in the reference (sbv2_stream_formant_contour in sbv2_hip.h states it): the formant contour of a request STREAM's delivered samples,
// frame by frame.
struct StreamFormantContour {
    int32_t hop = 160, window = 0, order = 0, n_formants = 4;
    double f_lo = 0.0, f_hi = 0.0, bw_max = 0.0;
    int64_t n_frames = 0;   // out, set by stream_begin_request_formant_contour: ceil(total_samples / hop)
    sbv2_stream_formant_contour c_struct() const { return sbv2_stream_formant_contour{hop, window, order, n_formants, f_lo, f_hi, bw_max, 0}; }
};
// sbv2_stream_begin_request_formant_contour: stream_begin_request_spectrum with the formant contour of the delivered samples; contour ==
// nullptr is exactly that call.
inline sbv2_stream* stream_begin_request_formant_contour(sbv2_bert* bert, sbv2_vits* vits, const sbv2_batch& batch, const sbv2_utt_options* opts,
                                                         Assist* assist, const int64_t* token_ids, const int64_t* s_lens, const int64_t* word2ph,
                                                         int64_t chunk_frames, const sbv2_stream_request& rq, StreamVoice* voice,
                                                         const StreamLeveler* leveler, StreamSpectrum* spectrum, StreamFormantContour* contour,
                                                         const sbv2_stream_levels* lv = nullptr, const sbv2_stream_pitch* sp = nullptr,
                                                         int64_t* total_samples = nullptr, int64_t* n_tokens = nullptr, int64_t* n_env = nullptr,
                                                         int64_t* n_pitch = nullptr) {
    sbv2_stream* s = nullptr;
    sbv2_stream_leveler c{};
    sbv2_stream_spectrum q{};
    sbv2_stream_formant_contour fc{};
    if (leveler) c = leveler->c_struct();
    if (spectrum) q = spectrum->c_struct();
    if (contour) fc = contour->c_struct();
    int64_t n_spec = 0, n_formant = 0;
    int32_t n_bands = 0;
    check(sbv2_stream_begin_request_formant_contour(bert, vits, &batch, opts, assist ? assist->c_struct() : nullptr, token_ids, s_lens, word2ph,
                                                    chunk_frames, &rq, lv, sp, voice ? voice->c_struct() : nullptr, leveler ? &c : nullptr,
                                                    spectrum ? &q : nullptr, contour ? &fc : nullptr, &s, total_samples, n_tokens, n_env, n_pitch,
                                                    &n_spec, &n_bands, &n_formant));
    if (spectrum) spectrum->n_frames = n_spec, spectrum->n_bands = n_bands;
    if (contour) contour->n_frames = n_formant;
    return s;
}
// sbv2_stream_next_formant_contour: the frames completed since the previous call, appended to f_hz / bw_hz ([frames][n_formants]) and status
// ([frames]); returns how many
inline int64_t stream_next_formant_contour(sbv2_stream* s, const StreamFormantContour& contour, std::vector<double>* f_hz, std::vector<double>* bw_hz,
                                           std::vector<int32_t>* status) {
    const size_t at = f_hz->size(), at_b = bw_hz->size(), at_s = status->size(), nk = (size_t)contour.n_formants;
    f_hz->resize(at + (size_t)contour.n_frames * nk);   // (room for everything that can be pending)
    bw_hz->resize(at_b + (size_t)contour.n_frames * nk);
    status->resize(at_s + (size_t)contour.n_frames);
    sbv2_stream_formant_part part{contour.n_frames, f_hz->data() + at, bw_hz->data() + at_b, status->data() + at_s, 0, 0, 0};
    const int rc = sbv2_stream_next_formant_contour(s, &part);
    const size_t n = rc == 0 ? (size_t)part.n : 0;
    f_hz->resize(at + n * nk);
    bw_hz->resize(at_b + n * nk);
    status->resize(at_s + n);
    check(rc);
    return part.n;
}

}  // namespace sbv2_core

#endif
