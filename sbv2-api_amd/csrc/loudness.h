// Integrated loudness (ITU-R BS.1770-4 gating, EBU R128) and true peak of formatted signals on the device (loudness.hip): the meter of
// sbv2_pipeline_fetch_pcm_loudness / _fetch_flac_loudness (the loudness GainStage of PcmFormatter::run, on the f64 signal y its resampler
// leaves in HBM), and of the test hook sbv2_debug_loudness.
#pragma once
#include "common.h"
#include "pcm_format.h"

struct sbv2_loudness;

namespace sbv2 {

// a checked sbv2_loudness; apply = false: measure only (G = 0)
struct LoudnessSpec {
    bool apply = false;
    double target = 0.0, ceiling = 0.0;
};
// throws with a message for out-of-range or non-finite fields; NULL -> measure only
LoudnessSpec loudness_spec(const sbv2_loudness* ln);
// the K-weighting at a supported rate (libebur128 form): coef = shelf b0 b1 b2 a1 a2, then high-pass b0 b1 b2 a1 a2; throws for other rates
void loudness_kweight(int rate, double coef[10]);
// samples per K-weighting segment at a supported rate, a divisor of rate / 10 (the meter's and the stream leveler's); throws for other rates
int loudness_segment_len(int rate);
// the true-peak interpolator's phases 1..3 (the kernel arguments of k_true_peak): h[p][d] = h4(p + 1 + 4 (d - 12)), d in [0, 24)
constexpr int kTruePeakTaps = 24;
void loudness_true_peak_taps(double h[3][kTruePeakTaps]);

// Device state of the meter of one execution context: the signal table (pinned + device), the per-segment K-weighting states and partial
// sums, the per-signal true peaks, stats and gains (all grown on demand; growing synchronises the stream).
class LoudnessMeter {
  public:
    LoudnessMeter() = default;
    LoudnessMeter(const LoudnessMeter&) = delete;
    LoudnessMeter& operator=(const LoudnessMeter&) = delete;
    // Enqueues on s the meter of the signals sig[i] = y[out_off, out_off + j1 - j0) (y: device f64, may be null when every signal is
    // empty) at `rate`: K-weighting (three launches), true peak, gate.  Returns the device gains 10^(G / 20), one per signal, and enqueues
    // the copy of the stats to the host: stats_host() holds 3 doubles per signal (L, TP, G) once s has been synchronised.
    // with_peak = false (the limiter's intermediate evaluations, limiter.hip) leaves the true-peak pass out: TP reads -inf.
    const double* measure(const double* y, const std::vector<FmtSignal>& sig, int rate, const LoudnessSpec& ln, hipStream_t s,
                          bool with_peak = true);
    const double* stats_host() const { return stats_host_; }
    // the device copy of the last measure()'s stats (valid on its stream, until the next measure())
    const double* stats_dev() const { return stats_dev_; }
    // Where the last measure() left what its launches write (device; read only; valid like stats_dev()): e and st [nseg][4], part [nseg],
    // bmax [nblk], peak [nsig], each followed by pad words up to the next array (the last one up to `end`), and the segment length m.  For
    // the test hook sbv2_debug_loudness_parts.
    struct Parts {
        const double *e = nullptr, *st = nullptr, *part = nullptr, *bmax = nullptr, *end = nullptr;
        const unsigned long long* peak = nullptr;
        int64_t nseg = 0, nblk = 0;
        int m = 0;
    };
    const Parts& parts() const { return parts_; }

  private:
    const std::vector<double>& tables(int rate);
    std::map<int, std::vector<double>> tables_;
    PinnedBuffer host_;   // signal table, then the stats
    DeviceBuffer dev_;    // signal table, peaks, stats, gains, then the per-segment states and partial sums
    double* stats_host_ = nullptr;
    double* stats_dev_ = nullptr;
    Parts parts_;
};

}  // namespace sbv2
