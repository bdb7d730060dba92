// Look-ahead true-peak limiter on the device (limiter.hip): the stage between the loudness meter and the gain / quantiser / FLAC encoder of
// sbv2_pipeline_fetch_pcm_limited / _fetch_flac_limited (the limiter GainStage of PcmFormatter::run), and of the test hook
// sbv2_debug_limiter.  The convention is the header comment of struct sbv2_limiter (include/sbv2_hip.h).
#pragma once
#include "common.h"
#include "loudness.h"
#include "pcm_format.h"

struct sbv2_limiter;

namespace sbv2 {

// a checked sbv2_limiter
struct LimiterSpec {
    double target = 0.0, ceiling = 0.0, depth = 0.0;   // LUFS, dBTP, max_reduction_db
};
// throws with a message for a null pointer, out-of-range or non-finite fields and a non-zero reserved field
LimiterSpec limiter_spec(const sbv2_limiter* lim);

// Device state of the limiter of one execution context, beside the LoudnessMeter and outside the activation arena: the signal table, the
// per-signal gains and stats, the interpolated magnitudes, the evaluated signal x and the per-tile minima (grown on demand; growing
// synchronises the stream), and a second meter for the evaluations of x.
class Limiter {
  public:
    Limiter() = default;
    Limiter(const Limiter&) = delete;
    Limiter& operator=(const Limiter&) = delete;
    // Enqueues on s: meter.measure(y) (L, TP and the scale-only gain of the signals sig[i] = y[out_off, out_off + j1 - j0) at `rate`), the
    // envelope, three evaluations of the gain curve with the meter on each, and the stats.  Returns the device signal x (f64, laid out as
    // y; y itself when there is no sample); *unit receives one gain of 1.0 per signal, so that the existing gain kernels deliver x as it
    // is.  stats_host() holds 6 doubles per signal (L, TP, G, L_out, TP_out, deepest reduction in dB) once s has been synchronised.
    const double* run(const double* y, const std::vector<FmtSignal>& sig, int rate, const LimiterSpec& lim, LoudnessMeter& meter, hipStream_t s,
                      const double** unit);
    const double* stats_host() const { return stats_host_; }

  private:
    LoudnessMeter xmeter_;   // the meter of x (its own scratch: the stats of y stay in the caller's meter)
    PinnedBuffer host_;      // signal table, Hann taps, then the stats
    DeviceBuffer dev_;
    double* stats_host_ = nullptr;
};

}  // namespace sbv2
