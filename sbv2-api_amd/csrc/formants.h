// The formant contour of a delivered signal (formants.hip): per frame the linear-prediction polynomial of the pre-emphasised, Gauss-windowed
// samples a formatted fetch leaves in HBM, its roots, and the first n_formants resonances (frequency, bandwidth) among them, as
// include/sbv2_hip.h states it above sbv2_formant_contour.  The time axis is that of the pitch contour and of the spectrum (marks.h).
// Used by sbv2_pipeline_fetch_request_formant_contour (fetch.cpp), sbv2_formant_contour_defaults (api.cpp) and the test hook
// sbv2_debug_formant_contour.  (The formant SCALE, which moves the formants, is voice.h's.)
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

  private:
    static constexpr size_t kMaxWindows = 8;
    std::map<int, DeviceBuffer> windows_;   // by window length: [window] f64
    PinnedBuffer stage_;                    // upload staging of a window
    DeviceBuffer dev_;                      // F [nf][nk] | B [nf][nk] | lpc [nf][p + 1] (asked for only) | status [nf]
    PinnedBuffer host_;
    int64_t nf_ = 0, nk_ = 0, nlpc_ = 0;
};

}  // namespace sbv2
