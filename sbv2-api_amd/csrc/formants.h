// The formant contour of a delivered signal (formants.hip): per frame the linear-prediction polynomial of the pre-emphasised, Gauss-windowed
// samples a formatted fetch leaves in HBM, its roots, and the first n_formants resonances (frequency, bandwidth) among them, as
// include/sbv2_hip.h states it above sbv2_formant_contour.  The time axis is that of the pitch contour and of the spectrum (marks.h).
// Used by sbv2_pipeline_fetch_request_formant_contour (fetch.cpp), sbv2_formant_contour_defaults (api.cpp) and the test hook
// sbv2_debug_formant_contour; fed replay by replay (StreamFormants below) by sbv2_stream_begin_request_formant_contour (stream_output.cpp) and
// the test hook sbv2_debug_stream_formant_contour.  (The formant SCALE, which moves the formants, is voice.h's.)
#pragma once
#include <map>

#include "common.h"
#include "pcm_format.h"

namespace sbv2 {

constexpr int kFormantMinWindow = 64, kFormantMaxWindow = 2048, kFormantMinOrder = 4, kFormantMaxOrder = 50, kFormantMaxKept = 8,
              kFormantMaxRate = 48000, kFormantMaxIter = 64;
constexpr double kFormantPreHz = 50.0, kFormantStart = 0.9, kFormantTol = 1e-14;
// a frame's status word: 0 = converged (or silent: nothing to converge)
constexpr int32_t kFormantCapHit = 1, kFormantLevinsonStopped = 2;

// Checked parameters, the zeros replaced by their defaults.
struct FormantContourSpec {
    int sample_rate = 0;
    int64_t hop = 0;
    int window = 0, order = 0, n_formants = 0;
    double f_lo = 0.0, f_hi = 0.0, bw_max = 0.0;
    double alpha() const;   // the pre-emphasis coefficient exp(-2 pi 50 / sr)
};
// THE check of the parameters at sample_rate; throws on anything outside the ranges that include/sbv2_hip.h states (NaNs fail every
// comparison and are refused).  The C entry, the host-only helper and the hook all come here (through check_formant_contour, api_internal.h).
FormantContourSpec formant_contour_spec(int sample_rate, int64_t hop, int window, int order, int n_formants, double f_lo, double f_hi, double bw_max);
inline int64_t formant_frames(int64_t n, int64_t hop) { return n > 0 ? (n + hop - 1) / hop : 0; }
// The Gaussian window of the definition, in f64.
void formant_window(int window, std::vector<double>* w);

// Frames per workgroup of four waves.  A frame's work is a short parallel head (staging, p + 1 dot products over the window) and a long
// serial tail on ONE wave (Levinson, then the root iteration with a lane per root), so a workgroup that owns one frame leaves three waves
// idle through the tail.  Windows of up to kFormantPackWindow samples (25 ms at up to 20.48 kHz: the 8 and 16 kHz cases) are packed four
// to a workgroup, a wave per frame from staging to the last store; a longer window takes the workgroup, its lags dealt over the four
// waves, and wave 0 runs the tail.  Either way a frame's sums run in one order: lag k is one wave's lane-strided sum and one butterfly.
constexpr int kFormantPackWindow = 512;
inline int formant_frames_per_block(int window) { return window <= kFormantPackWindow ? 4 : 1; }

// Device state of the stage of one execution context: the window tables (by window length, at most kMaxWindows of 16 KB), the results on
// the device and their pinned mirror, grown on demand; nothing is allocated before the first run.  One launch per run (k_formant_lpc), no
// atomics.  The first run with a window length forms the table on the host, uploads it from pinned staging and synchronises s once for it.
class Formants {
  public:
    Formants() = default;
    Formants(const Formants&) = delete;
    Formants& operator=(const Formants&) = delete;
    // Enqueues on s the stage over x = n delivered samples on the device (encoding as Marks::run) and the copy of its results to the host:
    // f_host()[f n_formants + q], bw_host() likewise and status_host()[f] hold frame f < n_frames() once s has been synchronised, and with
    // lpc = true lpc_host()[f (order + 1) + k] the frame's polynomial (the hook's).  n = 0 enqueues nothing.
    void run(const void* x, int encoding, int64_t n, const FormantContourSpec& sp, hipStream_t s, bool lpc = false);
    int64_t n_frames() const { return nf_; }
    const double* f_host() const { return host_.as<double>(); }
    const double* bw_host() const { return host_.as<double>() + nf_ * nk_; }
    const double* lpc_host() const { return host_.as<double>() + 2 * nf_ * nk_; }
    const int32_t* status_host() const { return reinterpret_cast<const int32_t*>(host_.as<double>() + 2 * nf_ * nk_ + nlpc_); }
    // F and B of the last run on the device, [n_frames][n_formants] each: the tracker's candidates (formant_track.h)
    const double* f_device() const { return dev_.as<double>(); }
    const double* bw_device() const { return dev_.as<double>() + nf_ * nk_; }

  private:
    static constexpr size_t kMaxWindows = 8;
    std::map<int, DeviceBuffer> windows_;   // by window length: [window] f64
    PinnedBuffer stage_;                    // upload staging of a window
    DeviceBuffer dev_;                      // F [nf][nk] | B [nf][nk] | lpc [nf][p + 1] (asked for only) | status [nf]
    PinnedBuffer host_;
    int64_t nf_ = 0, nk_ = 0, nlpc_ = 0;
};

// The same stage FED piece by piece (a stream's replays), by sbv2_formant_contour's convention unchanged: frame f reads the window
// [b, b + window) and the sample at b - 1, b = f hop + hop / 2 - window / 2; positions outside [0, total) read as 0; n_frames = ceil(total / hop).
// The completion rule: frame f is complete once min(b + window, total) <= D, D the samples fed (or, for what a stream hands out, delivered)
// so far.  Frames complete in order (b ascends with f); after the last push everything is complete.
// The carry: the last min(D, window) fed samples, in the sample's own type, on the device.  That is enough: the first incomplete frame has
// b + window > D, so its earliest read b - 1 is >= D - window.  Sized once for kFormantMaxWindow elements of the widest type and held twice (a
// push reads one copy and writes the other: a push shorter than the carry keeps part of the old one, and no workgroup reads what another
// one of the same launch overwrites) = 16 KB whatever the stream's length.
// A push is ONE launch (k_stream_formant) and one copy of the frames it completed from the push's device records to the pinned mirror, which
// holds every frame of the stream as a record {F [n_formants] | B [n_formants] | lpc [order + 1] (asked for only) | status} until the next
// begin; a push that completes no frame still updates the carry, n = 0 enqueues nothing.  The window table is uploaded in begin.  No atomics.
//
// Ownership on a stream.  formant_frames_per_block is tuned for tens of thousands of frames; a push completes a few hundred at most and the
// first chunk far fewer, fewer than the device has compute units, and four frames to a workgroup then leave most of the chip idle while one
// wave computes all order + 1 lags of its frame.  So a push that completes no more frames than the device has compute units (read once in
// begin) takes ONE frame per workgroup whatever the window, the head dealt over four waves and wave 0 running the tail; above that count it
// takes formant_frames_per_block(window).  The bits do not depend on the choice (above: a lag is one wave's lane-strided sum and one
// butterfly under either).  Measured (DESIGN.md 8z, 16 kHz, window 400): a first push of 147 frames takes 46 us against 58 us with four frames
// to a workgroup.  One frame per workgroup was also the faster one above the count (1.10 - 1.20 times at 296 to 2378 frames): the threshold
// is where the rule stops, not where the other ownership starts to win, and has not been swept.
inline int formant_stream_frames_per_block(int64_t frames, int window, int cus) { return frames <= cus ? 1 : formant_frames_per_block(window); }
// the completion rule on its own: the frames of a signal of `total` samples that are complete once D of them are in
int64_t formant_frames_complete(const FormantContourSpec& sp, int64_t total, int64_t D);
class StreamFormants {
  public:
    StreamFormants() = default;
    StreamFormants(const StreamFormants&) = delete;
    StreamFormants& operator=(const StreamFormants&) = delete;
    // Host only, throws: the spec within the stage's limits, fewer than 2^30 frames
    static void check(const FormantContourSpec& sp, int64_t total);
    // Uploads the window table the previous stream did not leave, sizes the push's records for pushes of up to `most` samples (a longer one
    // grows them, which waits for s) and waits for s once.  pack: 0 = the rule above; 1 / 4 = that many frames per workgroup in every push
    // (4 with window > kFormantPackWindow runs as 1).  lpc: the records keep the polynomial (the hook's).
    void begin(const FormantContourSpec& sp, int encoding, int64_t total, int64_t most, hipStream_t s, int pack = 0, bool lpc = false);
    // x = the sample at delivered position D0 (device), D0 = fed(); returns the frames this push completed; n = 0 enqueues nothing
    int64_t push(const void* x, int64_t D0, int64_t n, hipStream_t s);
    int64_t fed() const { return fed_; }
    int64_t total() const { return total_; }
    int64_t n_frames() const { return nf_; }
    const FormantContourSpec& spec() const { return sp_; }
    int64_t complete(int64_t D) const { return formant_frames_complete(sp_, total_, D); }
    // frame f is valid once the push that completed it has run on s: n_formants values each, order + 1 for the polynomial
    const double* f_host(int64_t f) const { return host_.as<double>() + f * rec_; }
    const double* bw_host(int64_t f) const { return f_host(f) + sp_.n_formants; }
    const double* lpc_host(int64_t f) const { return f_host(f) + 2 * sp_.n_formants; }
    int32_t status_host(int64_t f) const { return *reinterpret_cast<const int32_t*>(f_host(f) + rec_ - 1); }

  private:
    static constexpr size_t kCarryBytes = (size_t)kFormantMaxWindow * sizeof(float);   // one copy, in the widest sample type
    PinnedBuffer host_, stage_;   // the records' mirror; upload staging of the window
    DeviceBuffer window_, carry_, out_;
    FormantContourSpec sp_;
    int64_t total_ = 0, nf_ = 0, fed_ = 0, done_ = 0, rec_ = 0;   // rec_: f64 words per record (the status takes the last one)
    int encoding_ = 0, parity_ = 0, forced_ = 0, cus_ = 0, window_len_ = 0;
    bool lpc_ = false;
};

}  // namespace sbv2
