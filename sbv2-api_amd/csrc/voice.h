// Pitch and intonation scale (voice.hip): a length-preserving TD-PSOLA of the run's native f32 rows, in front of the formatter (fetch_formatted,
// fetch.cpp), as include/sbv2_hip.h states it above sbv2_voice.  Used by sbv2_pipeline_fetch_request_voice and the test hook sbv2_debug_voice_shift.
// Three steps on one stream: the YIN contour of every listed row (k_pitch_yin of marks.hip on f32, one launch per row), the marks of every row
// (k_voice_marks, one workgroup per row: mean f0, phase increments, ta / ts / map) and the overlap-add gather (k_voice_gather, the hot path).
// Per-token pitch targets (sbv2_token_pitch, sbv2_pipeline_fetch_request_token_pitch, sbv2_debug_voice_tokens) are one more phase of the marks
// kernel, launched as k_voice_marks_tok only by a call that brings a token table.  A formant scale (sbv2_formant, sbv2_pipeline_fetch_request_formant,
// sbv2_debug_voice_formant) is a second instantiation of the gather, launched as k_voice_gather_fmt only by a call that brings one.
#pragma once
#include "common.h"
#include "marks.h"
#include "track.h"

namespace sbv2 {

// Checked parameters (voice_spec): the pitch spec of the contour (its hop is the frame hop H), the two scales and what follows from the rate.
struct VoiceSpec {
    PitchSpec pitch;
    double pitch_scale = 1.0, intonation_scale = 1.0;
    double g_lo = 0.0, g_hi = 0.0;   // the clamp of the target f0: [f0_min / 2, 2 f0_max]
    int64_t inc_u = 0;               // the increment of an unvoiced frame, llrint(2^32 / (sr / 200))
    int half = 0;                    // no window half-width exceeds it: max(tau_max + 1, sr / 200) + 2
    int min_a = 0, min_s = 0;        // no two analysis / synthesis marks of a row lie closer than this
    bool identity() const { return pitch_scale == 1.0 && intonation_scale == 1.0; }
};
constexpr int kVoiceMinRate = 1000;
// throws: pitch_scale in [0.5, 2], intonation_scale in [0, 2], 1000 <= sr <= 48000, hop in [sr / 1000, sr / 50] (0 = sr / 200), f0_min / f0_max /
// threshold as pitch_spec has them (0 = 70, 600, 0.15); NaNs fail every comparison and are refused
VoiceSpec voice_spec(int sample_rate, double pitch_scale, double intonation_scale, int64_t hop, double f0_min, double f0_max, double threshold);

// Formant scale (sbv2_formant in include/sbv2_hip.h): the factor q by which every grain is read, and the range of synthesis marks that can reach
// an output sample, which grows as a voiced grain widens by 1 / q.
struct FormantSpec {
    double scale = 1.0;
    int half = 0;   // ceil(VoiceSpec::half / min(q, 1)) + 1
    bool identity() const { return scale == 1.0; }
};
// The checks of a sbv2_formant's two fields, in one place for the fetch and the test hook.  throws: reserved == 0, formant_scale in [0.5, 2];
// a NaN fails the comparisons and is refused
FormantSpec formant_spec(double formant_scale, double reserved, const VoiceSpec& v);

// One row of a call: x[x_off .. x_off + n) -> y[x_off .. x_off + n)
struct VoiceRow {
    int64_t off, n;
};

// Per-token pitch edits of a call, as include/sbv2_hip.h states them above sbv2_token_pitch.  HOST arrays, the rows' tokens back to back: token t
// of a row owns the samples [ends[t - 1], ends[t]) of that row (the first from 0); ends ascend within a row and may lie beyond its length.
struct VoiceTokens {
    const int64_t* counts;   // [nrows] tokens of every row
    const int64_t* ends;     // [sum counts]
    const double* value;     // [sum counts] 0 = not edited
    int kind, smooth;        // 0 = ratio, 1 = Hz; K contour frames to each side
};
constexpr int kVoiceMaxSmooth = 20;
// throws: kind in {0, 1}, smooth in [0, 20], every value 0 or in [0.5, 2] (kind 0) / [f0_min / 2, 2 f0_max] (kind 1); a NaN is refused
void voice_tokens_check(const double* value, int64_t n_tokens, int kind, int smooth, const VoiceSpec& sp);

// Device state of the shifter of one execution context: the contour, the per-frame phases, the marks and the shifted rows, grown on demand;
// nothing is allocated before the first run.  No atomics; every sum's order is fixed, so equal rows give equal bits.
class Voice {
  public:
    Voice() = default;
    Voice(const Voice&) = delete;
    Voice& operator=(const Voice&) = delete;
    static constexpr int kTile = 256;   // output samples per workgroup of the gather
    // Enqueues on s: rows[i] of x (device, f32) shifted into the same positions of the scratch buffer, which spans `span` floats (>= every
    // off + n) and is returned.  period_in / voiced_in (HOST, one entry per frame, rows back to back; both or neither): the contour to use
    // instead of the estimated one; a voiced entry outside [tau_min - 1, tau_max + 1] is refused.  Rows and parameters are checked before
    // anything is enqueued (throws).
    // tr (not with a given contour): the estimated contour is tracked, every row apart from the others, before the marks are placed (track.h).
    // tok: the per-token edits (checked here, throws); k_voice_marks_tok then forms M_t, rho_t and R_f between the contour and the marks, and
    // applied / src_f0 are on their way to pinned memory when run returns.  Without tok every launch, argument and byte is that of a call
    // from before token edits existed.
    // fm: the gather is k_voice_gather_fmt with this scale, 1 included (the test hook); without fm it is k_voice_gather as it always was.
    // Contour, marks and token results do not depend on it.
    float* run(const float* x, int64_t span, const VoiceRow* rows, int nrows, const VoiceSpec& sp, hipStream_t s, const double* period_in = nullptr,
               const int32_t* voiced_in = nullptr, const TrackSpec* tr = nullptr, const VoiceTokens* tok = nullptr, const FormantSpec* fm = nullptr);
    // Results of the last run for the test hook, valid once results_to_host() has been enqueued and s synchronised: per frame (rows back to
    // back) the period T_f and voiced; per row the marks at mark_off(i), n_a(i) analysis and n_s(i) synthesis ones.
    void results_to_host(hipStream_t s);
    int64_t n_frames() const { return nf_; }
    const double* period_host() const { return h_period_; }
    const int32_t* voiced_host() const { return h_voiced_; }
    int32_t n_a(int i) const { return h_count_[4 * i]; }
    int32_t n_s(int i) const { return h_count_[4 * i + 1]; }
    int32_t status(int i) const { return h_count_[4 * i + 2]; }   // 0, or 1 = more marks than planned (nothing was written beyond the plan)
    const int32_t* ta_host(int i) const { return h_ta_ + cap_off_[i]; }
    const int32_t* ts_host(int i) const { return h_ts_ + cap_off_[i]; }
    const int32_t* map_host(int i) const { return h_map_ + cap_off_[i]; }
    // Of a run with a token table, valid once s is synchronised: per token applied and src_f0; per frame R_f (after results_to_host()).
    int64_t n_tokens() const { return nt_ > 0 ? nt_ : 0; }
    const double* applied_host() const { return h_tout_; }
    const double* src_f0_host() const { return h_tout_ + n_tokens(); }
    const double* ratio_host() const { return h_ratio_; }

  private:
    DeviceBuffer dev_, out_;   // tables | contour | phases | marks (| the candidates of a tracked contour) ; the shifted rows
    Track track_;
    PinnedBuffer host_;
    std::vector<int64_t> cap_off_;
    int64_t nf_ = 0, ncap_ = 0, nt_ = -1;   // nt_ < 0: the last run had no token table
    int nrows_ = 0;
    // the layout of the last run (device pointers and the pinned mirror's)
    double* d_period_ = nullptr;
    int32_t *d_voiced_ = nullptr, *d_count_ = nullptr, *d_ta_ = nullptr, *d_ts_ = nullptr, *d_map_ = nullptr;
    double* h_period_ = nullptr;
    int32_t *h_voiced_ = nullptr, *h_count_ = nullptr, *h_ta_ = nullptr, *h_ts_ = nullptr, *h_map_ = nullptr;
    double *d_tout_ = nullptr, *d_ratio_ = nullptr, *h_tout_ = nullptr, *h_ratio_ = nullptr;
};

}  // namespace sbv2
