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

// The shifter on a stream (sbv2_stream_voice in include/sbv2_hip.h): the two scales, the formant scale and the pivot the caller names for
// every row in place of the row's mean f0.  Checked by stream_voice_spec.
struct StreamVoiceSpec {
    VoiceSpec voice;
    FormantSpec formant;          // identity(): the plain gather
    std::vector<double> pivot;    // [rows] Hz, each in [f0_min, f0_max]
    int64_t lookahead = 0;        // A_v (stream_voice_lookahead)
};
// A_v = G + 2 W + X + tau_max + H div 2 with W = VoiceSpec::half, G = ceil(W / min(q, 1)) + 1 and X = ceil((max(q, 1) - 1) W), as
// include/sbv2_hip.h derives it
int64_t stream_voice_lookahead(const VoiceSpec& v, double formant_scale);
// throws: everything voice_spec and formant_spec refuse, the identity (p = s = q = 1), a non-zero reserved, a NULL pivot with rows > 0, a pivot
// that is not finite or lies outside [f0_min, f0_max]
StreamVoiceSpec stream_voice_spec(int sample_rate, double pitch_scale, double intonation_scale, int64_t hop, double f0_min, double f0_max, double threshold,
                                  double formant_scale, const double* pivot, int64_t rows, double reserved0, double reserved1);

// The same shifter FED piece by piece (a stream's replays).  The rows' lengths are known at begin, and the fed samples and the shifted ones
// are kept whole on the device (two buffers of the joined length), so no sample is carried; what a row carries from push to push is its two
// Q32 phases, the voiced-run bit, its mark counts and how many synthesis marks are mapped (k_voice_marks_fed), besides the frame cursor the
// host keeps by the estimator's completion rule.
// A push is up to three launches on the caller's stream: the contour of the frames it completed (pitch_launch_fed: k_stream_pitch's frames,
// the per-frame body of every estimator here), k_voice_marks_fed over them, and k_voice_gather / k_voice_gather_fmt over the outputs that
// became final.  The delivery rule: with S samples of a row fed and the row not ended, max(0, S - A_v) of its outputs are final; the push
// that feeds its last sample makes all of them final.  No atomics, nothing read back, nothing allocated after begin.
// Bits: with the row's own mean as the pivot, Voice::run's, whatever the pushes.
class StreamVoice {
  public:
    StreamVoice() = default;
    ~StreamVoice();
    StreamVoice(const StreamVoice&) = delete;
    StreamVoice& operator=(const StreamVoice&) = delete;
    // rows[i] = where row i lies in the two buffers of `span` floats; sp.pivot holds one entry per row.  period_in / voiced_in (HOST, as
    // Voice::run takes them): the contour to use instead of the estimated one (the test hook).  Waits for s once (an earlier stream's buffers
    // are reused) only if its uploads are still in flight or a buffer grows.  throws on rows outside the span, a pivot count that differs, a bad given contour.
    void begin(const StreamVoiceSpec& sp, const VoiceRow* rows, int nrows, int64_t span, hipStream_t s, const double* period_in = nullptr,
               const int32_t* voiced_in = nullptr);
    // The next n samples of row `row` (device, f32; n = 0 allowed), rows in any order, each row's samples in order.  Returns how many of the
    // row's outputs are final after it (final_after).
    int64_t push(int row, const float* x, int64_t n, hipStream_t s);
    int64_t final_after(int row, int64_t fed) const;   // the delivery rule
    int64_t fed(int row) const { return rows_[(size_t)row].fed; }
    int64_t lookahead() const { return sp_.lookahead; }
    const float* out(int row) const { return y_ + rows_[(size_t)row].off; }   // the row's shifted samples, final ones valid
    // status of every row -> the pinned mirror (0, or 1 = more marks than planned); valid once s is synchronised
    void status_to_host(hipStream_t s);
    int32_t status(int row) const { return h_count_[4 * row + 2]; }

  private:
    struct Row {
        int64_t off, n, f_off, nf, fed, frames, done;   // samples fed, frames placed, outputs final
    };
    StreamVoiceSpec sp_;
    std::vector<Row> rows_;
    DeviceBuffer dev_;
    PinnedBuffer host_;
    char* d_ = nullptr;
    size_t o_res_ = 0, o_period_ = 0, o_i64_ = 0, o_i32_ = 0, o_count_ = 0, o_state_ = 0, o_marks_ = 0;
    int64_t nf_ = 0, ncap_ = 0;
    float *x_ = nullptr, *y_ = nullptr;
    int32_t* h_count_ = nullptr;
    bool given_ = false;
    hipEvent_t uploaded_ = nullptr;   // behind the last begin's uploads from the pinned buffer
};

}  // namespace sbv2
