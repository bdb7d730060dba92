// Speech marks (marks.hip): where each token lies in a delivered signal (host arithmetic, marks_spans) and how loud it is there (one
// segmented reduction over the samples a formatted fetch leaves in HBM: sum of squares and peak per [start, end) segment).  Used by
// sbv2_pipeline_fetch_request_marks (fetch_formatted, fetch.cpp), sbv2_stream_marks (stream.cpp) and the test hook sbv2_debug_segment_levels.
// Beside them the pitch contour of the same samples (Pitch: YIN per frame; sbv2_pipeline_fetch_request_pitch, sbv2_debug_pitch) and the same
// contour fed replay by replay (StreamPitch; sbv2_stream_begin_request_pitch, sbv2_debug_stream_pitch).
#pragma once
#include "common.h"
#include "pcm_format.h"

namespace sbv2 {

// Delivered index of native position a at rate L / M: ceil(a L / M), the rule of pcm_format_out_len.
inline int64_t marks_delivered(const PcmFmtSpec& s, int64_t a) { return (a * s.L + s.M - 1) / s.M; }
// Token t of a row with durations d (frames, >= 0), placed at native sample `place` of its timeline, hop samples per frame:
// [start[t], end[t]) = [J(place + hop c[t]), J(place + hop c[t + 1])), c the exclusive prefix sum of d.  Throws for a negative duration,
// hop < 1, place < 0 and positions that leave the int64 range of a L.
void marks_spans(const int64_t* d, int64_t n, int64_t hop, int64_t place, const PcmFmtSpec& s, int64_t* start, int64_t* end);
// The span table of n_rows rows of one forward, packed in the order given: row rows[k] (rows == nullptr: row k), whose durations are
// used[offs[r], offs[r + 1]), placed at place[k].  The fetch's marks, sbv2_stream_marks and a stream's token levels all read this table.
inline void marks_spans_rows(const std::vector<int64_t>& used, const std::vector<int64_t>& offs, const int32_t* rows, int64_t n_rows,
                             const int64_t* place, int64_t hop, const PcmFmtSpec& s, int64_t* start, int64_t* end) {
    for (int64_t k = 0, e = 0; k < n_rows; ++k) {
        const int64_t r = rows ? rows[k] : k, nt = offs[r + 1] - offs[r];
        marks_spans(used.data() + offs[r], nt, hop, place[k], s, start + e, end + e);
        e += nt;
    }
}

// Device state of the level reduction of one execution context: the segment table (pinned + device) and the results (device + pinned), grown
// on demand; nothing is allocated before the first run.  One launch per run, no atomics: a segment's sum is formed in an order that depends
// on its length only, so equal samples give equal bits.
class Marks {
  public:
    Marks() = default;
    Marks(const Marks&) = delete;
    Marks& operator=(const Marks&) = delete;
    // segments longer than this take a whole workgroup (256 lanes) instead of one wave
    static constexpr int64_t kLongSegment = 4096;
    // Enqueues on s: sumsq / peak of x[seg[2 i], seg[2 i + 1]) for i < nseg, x = n delivered samples on the device (encoding 0 = f32,
    // 1 = s16, taken as integers, 7 / 6 = G.711 codes, taken as the integers they decode to), and the copy of the results to the host: sumsq_host()[i] / peak_host()[i] hold them once s has been
    // synchronised.  Every segment is checked against [0, n] before anything is enqueued (throws); nseg = 0 enqueues nothing.
    void run(const void* x, int encoding, int64_t n, const int64_t* seg, int64_t nseg, hipStream_t s);
    const double* sumsq_host() const { return res_host_; }
    const double* peak_host() const { return res_host_ + nseg_; }

  private:
    PinnedBuffer host_;   // segment table | order, then the results
    DeviceBuffer dev_;    // the same
    double* res_host_ = nullptr;
    int64_t nseg_ = 0;
};

// The pitch contour of a delivered signal: YIN (de Cheveigne & Kawahara 2002, steps 2 - 5) per frame of `hop` delivered samples, as
// include/sbv2_hip.h states it above sbv2_pitch.  Checked parameters and the lag range they give:
struct PitchSpec {
    int sample_rate = 0;
    int64_t hop = 0;
    int tau_min = 0, tau_max = 0;   // floor(sr / f0_max), ceil(sr / f0_min); the window W = tau_max
    double threshold = 0.0;
};
// The exactness bound of the integer encodings rests on tau_max <= kPitchMaxTau: with |v| <= 32768 a difference is at most 65535, so
// d(tau) <= 1200 * 65535^2 < 2^43, d(tau) tau and S(tau) <= 1200 * 1200 * 65535^2 = 6.2e15 < 2^53 = 9.0e15: both convert to f64 unrounded and
// c(tau) has ONE rounding, its division.  40 Hz at 48 kHz gives exactly 1200; anything that would exceed it is refused.
constexpr int kPitchMaxTau = 1200;
constexpr double kPitchMinF0 = 40.0;
constexpr int kPitchMaxRate = 48000;
// throws: 40 <= f0_min < f0_max <= sr / 4, 0 < threshold < 1, hop >= 1, 0 < sr <= 48000 (NaNs fail every comparison and are refused)
PitchSpec pitch_spec(int sample_rate, int64_t hop, double f0_min, double f0_max, double threshold);
inline int64_t pitch_frames(int64_t n, int64_t hop) { return n > 0 ? (n + hop - 1) / hop : 0; }
// What the host makes of a frame's device results (plain f64 arithmetic, never contracted): the parabolic refinement of the lag through
// c(lag - 1), c(lag), c(lag + 1), f0 = sr / (lag + delta) for a voiced frame and 0 otherwise, ap = c(lag).
void pitch_finish(const PitchSpec& sp, int32_t lag, int32_t voiced, const double* c3, double* f0, double* ap);

// The estimator's one launch (k_pitch_yin) into the caller's device arrays c3 [nf][3], lag [nf], voiced [nf], nf = pitch_frames(n, sp.hop);
// x = n samples on the device (encoding as Marks::run).  n = 0 enqueues nothing.  Pitch::run and the shifter's contour (voice.hip) go through it.
// With cand (k_pitch_yin_cand): besides, every frame's candidates for the tracker (track.h) as include/sbv2_hip.h states them above
// sbv2_pitch_track: cand [nf][kTrackRec] = ncand, 7 tau (ascending; 0 in absent slots), 7 q = llrint(c 65536); cand_c3 [nf][7][3] = c-, c0, c+
// under the neighbour rule.  c3 / lag / voiced are the plain kernel's bits either way.
constexpr int kTrackCand = 7, kTrackRec = 1 + 2 * kTrackCand;
void pitch_launch(const void* x, int encoding, int64_t n, const PitchSpec& sp, double* c3, int32_t* lag, int32_t* voiced, hipStream_t s,
                  double cand_max = 0.0, int32_t* cand = nullptr, double* cand_c3 = nullptr);

struct TrackSpec;   // track.h
class Track;

// Device state of the pitch estimator of one execution context (k_pitch_yin, marks.hip): results on the device and their pinned mirror, grown
// on demand; nothing is allocated before the first run.  One launch per run, one workgroup per frame, no atomics.
class Pitch {
  public:
    Pitch() = default;
    Pitch(const Pitch&) = delete;
    Pitch& operator=(const Pitch&) = delete;
    // Enqueues on s the estimator over x = n delivered samples on the device (encoding as Marks::run) and the copy of its results to the
    // host: lag_host()[f], voiced_host()[f] and c3_host()[3 f ..] = c(lag - 1), c(lag), c(lag + 1) (a neighbour outside [1, tau_max] replaced
    // by c(lag)) hold frame f < n_frames() once s has been synchronised.  n = 0 enqueues nothing.
    // With tr (and tk, the tracker's state): the contour is TRACKED before the copy (track.h): two more launches, k_pitch_yin_cand instead of
    // k_pitch_yin; lag / voiced / c3 of the frames on the path's candidates are the candidates'.
    void run(const void* x, int encoding, int64_t n, const PitchSpec& sp, hipStream_t s, const TrackSpec* tr = nullptr, Track* tk = nullptr);
    int64_t n_frames() const { return nf_; }
    const double* c3_host() const { return static_cast<const double*>(host_.get()); }
    const int32_t* lag_host() const { return reinterpret_cast<const int32_t*>(c3_host() + 3 * nf_); }
    const int32_t* voiced_host() const { return lag_host() + nf_; }

  private:
    PinnedBuffer host_;   // c3 [nf][3] | lag [nf] | voiced [nf]
    DeviceBuffer dev_;    // the same
    int64_t nf_ = 0;
};

// The same reduction FED piece by piece (a stream's replays): two segment tables fixed at begin, the token spans (monotone, disjoint, empty
// ones and unowned holes allowed) and the envelope frames [f hop, min((f + 1) hop, total)); a push covers the delivered samples [D0, D0 + n)
// that have just been written on the device.  Lane (o mod stride) of a segment adds the squares at offsets o in increasing order, stride by
// the segment's TOTAL length (64 up to Marks::kLongSegment, 256 above), exactly as k_segment_levels does; a segment that a push leaves open
// keeps its lanes' (ss, pk) on the device and the next push goes on from them, the push that ends it runs the same tree.  So the results
// have the bits of Marks::run over the whole signal, whatever the pushes.  At most one segment per table is open between two pushes: the
// carry is 2 tables x 256 lanes x 2 doubles, held twice (a push reads one copy and writes the other: the segment it continues and the
// segment it leaves open may differ and run in different workgroups of one launch) = 16 KB whatever the stream's length.  No atomics.
// A push passes scalars by value only; nothing is allocated and no table is copied after begin.  Results: one device array of pairs
// {sumsq, peak}, tokens then frames, zero at begin (an empty segment stays 0, 0), with a pinned mirror; a push copies the slots it completed.
class StreamLevels {
  public:
    StreamLevels() = default;
    StreamLevels(const StreamLevels&) = delete;
    StreamLevels& operator=(const StreamLevels&) = delete;
    struct Done {
        int64_t tok, env;   // entries the push completed: tokens with end <= D0 + n, frames likewise, that no earlier push completed
    };
    // Host only, throws: spans within [0, total], start <= end, end[i] <= start[i + 1]; env_hop >= 0 with fewer than 2^30 frames
    static void check(const int64_t* seg, int64_t nseg, int64_t env_hop, int64_t total);
    static int64_t env_frames(int64_t env_hop, int64_t total) { return env_hop > 0 ? (total + env_hop - 1) / env_hop : 0; }
    // seg = [nseg][2] (nseg = 0: no token levels), env_hop = 0: no envelope.  Waits for s once (the buffers of an earlier stream are reused).
    void begin(const int64_t* seg, int64_t nseg, int64_t env_hop, int64_t total, hipStream_t s);
    // x = the sample at delivered position D0 (device), D0 = fed(); n = 0 enqueues nothing
    Done push(const void* x, int encoding, int64_t D0, int64_t n, hipStream_t s);
    int64_t fed() const { return fed_; }
    int64_t total() const { return total_; }
    int64_t env_hop() const { return env_hop_; }
    int64_t n_tok() const { return ntok_; }
    int64_t n_env() const { return nenv_; }
    // the completion rule: entries complete once D samples are out (tokens: end <= D; frames: min((f + 1) hop, total) <= D)
    int64_t tok_complete(int64_t D) const;
    int64_t env_complete(int64_t D) const { return nenv_ == 0 ? 0 : D >= total_ ? nenv_ : D / env_hop_; }
    // pairs {sumsq, peak}; entry i is valid once the push that completed it has run on s
    const double* tok_host() const { return res_host_; }
    const double* env_host() const { return res_host_ + 2 * ntok_; }

  private:
    std::vector<int64_t> seg_;   // the token table (host copy: which segments a push meets and completes)
    PinnedBuffer host_;          // the token table for its upload, then the results' mirror
    DeviceBuffer dev_;           // token table | carry (2 copies) | results
    int64_t* d_seg_ = nullptr;
    double *d_carry_ = nullptr, *d_res_ = nullptr, *res_host_ = nullptr;
    int64_t ntok_ = 0, nenv_ = 0, env_hop_ = 0, total_ = 0, fed_ = 0, tok_done_ = 0, env_done_ = 0;
    int parity_ = 0;
};

// The same estimator FED piece by piece (a stream's replays), by sbv2_pitch's convention unchanged: frame f has its centre at f hop + hop / 2,
// its window is [centre - tau_max, centre + tau_max), positions outside [0, total) read as 0, n_frames = ceil(total / hop).
// The completion rule: frame f is complete once min(f hop + hop / 2 + tau_max, total) <= D, D the samples fed (or, for what a stream hands out,
// delivered) so far.  Frames complete in order and about tau_max samples late; after the last push everything is complete.
// The carry: the last min(D, 2 tau_max) fed samples, in the sample's own type (float, int16_t, one-byte G.711 code), on the device.  That is
// enough: the first incomplete frame has centre + tau_max > D, so its window starts after D - 2 tau_max.  Sized once for 2 kPitchMaxTau
// elements and held twice (a push reads one copy and writes the other: a push shorter than the carry keeps part of the old one, and no workgroup
// reads what another one of the same launch overwrites) = 19 KB whatever the stream's length.
// A push is ONE launch (k_stream_pitch: one workgroup per frame it completed, staging the window from the carry and from x and then running
// k_pitch_yin's own per-frame body, and behind them the workgroups that write the next carry) and one copy of the completed slots to the pinned
// mirror; a push that completes no frame still updates the carry, n = 0 enqueues nothing.  Scalars by value, nothing allocated after begin, no
// atomics.
// Bits: a frame's sums depend on its window and on tau_max only, so lag, voiced and the three c values of every frame equal Pitch::run over the
// whole signal bit for bit, for every encoding (f32 included), whatever the pushes.
struct PitchFrame {   // one frame's device results (32 bytes): what Pitch keeps as c3 | lag | voiced, side by side so that a push copies one range
    double c3[3];
    int32_t lag, voiced;
};
// the completion rule on its own: the frames of a signal of `total` samples that are complete once D of them are in
int64_t pitch_frames_complete(const PitchSpec& sp, int64_t total, int64_t D);
// k_stream_pitch over a signal that is fed into ONE device buffer (the stream form of the shifter, voice.hip): x holds the first `fed` of its
// `total` f32 samples; the complete frames [first, first + count) go to res[first ...] with the bits of pitch_launch over the whole signal.
// No carry is read or written.  count = 0 enqueues nothing; frames that are not complete are refused (throws).
void pitch_launch_fed(const float* x, int64_t fed, int64_t total, const PitchSpec& sp, int64_t first, int64_t count, PitchFrame* res, hipStream_t s);
class StreamPitch {
  public:
    StreamPitch() = default;
    StreamPitch(const StreamPitch&) = delete;
    StreamPitch& operator=(const StreamPitch&) = delete;
    // Host only, throws: the spec's lags within kPitchMaxTau, fewer than 2^30 frames
    static void check(const PitchSpec& sp, int64_t total);
    // Waits for s once (the buffers of an earlier stream are reused).
    void begin(const PitchSpec& sp, int encoding, int64_t total, hipStream_t s);
    // x = the sample at delivered position D0 (device), D0 = fed(); returns the frames this push completed; n = 0 enqueues nothing
    int64_t push(const void* x, int64_t D0, int64_t n, hipStream_t s);
    int64_t fed() const { return fed_; }
    int64_t total() const { return total_; }
    int64_t n_frames() const { return nf_; }
    const PitchSpec& spec() const { return sp_; }
    int64_t complete(int64_t D) const;   // the completion rule: frames complete once D samples are in
    // frame f is valid once the push that completed it has run on s
    const double* c3_host(int64_t f) const { return res_host_[f].c3; }
    int32_t lag_host(int64_t f) const { return res_host_[f].lag; }
    int32_t voiced_host(int64_t f) const { return res_host_[f].voiced; }

  private:
    static constexpr size_t kCarryBytes = 2 * (size_t)kPitchMaxTau * sizeof(float);   // one copy, in the widest sample type
    PinnedBuffer host_;   // the results' mirror
    DeviceBuffer dev_;    // carry (2 copies) | results
    PitchSpec sp_;
    char* d_carry_ = nullptr;
    PitchFrame *d_res_ = nullptr, *res_host_ = nullptr;
    int64_t total_ = 0, nf_ = 0, fed_ = 0, done_ = 0;
    int encoding_ = 0, parity_ = 0;
};

}  // namespace sbv2
