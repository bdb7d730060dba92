// Speech compressor on the device (dynamics.hip): the stage in front of the loudness gain / look-ahead limiter of
// sbv2_pipeline_fetch_request_dynamics (PcmFormatter::run hands its output to the GainStage in place of y), and of the test hook
// sbv2_debug_dynamics.  The convention is the header comment of struct sbv2_dynamics (include/sbv2_hip.h).
#pragma once
#include "common.h"
#include "limiter.h"
#include "loudness.h"
#include "pcm_format.h"

struct sbv2_dynamics;

namespace sbv2 {

// a checked sbv2_dynamics
struct DynamicsSpec {
    double threshold = 0.0, ratio = 1.0, attack = 0.0, release = 0.0;   // LU above the signal's own loudness, -, dB/s, dB/s
    bool identity() const { return ratio == 1.0; }
};
// throws with a message for a null pointer, out-of-range or non-finite fields and a non-zero reserved field
DynamicsSpec dynamics_spec(const sbv2_dynamics* d);

// Device state of the compressor of one execution context, beside the LoudnessMeter and the Limiter: the signal table, the window's taps, the
// per-tile key maxima and carries, the interpolated magnitudes t, the static curve dq, the gain curve u and the compressed signal yc (grown
// on demand; growing synchronises the stream).  Nothing is allocated before the first run.
class Dynamics {
  public:
    static constexpr int kTile = kLimTile;   // samples per workgroup of the scans
    Dynamics() = default;
    Dynamics(const Dynamics&) = delete;
    Dynamics& operator=(const Dynamics&) = delete;
    // Enqueues on s: meter.measure(y) without the true peak (L of the signals sig[i] = y[out_off, out_off + j1 - j0) at `rate`), the
    // limiter's envelope, the static curve with the tiles' key maxima, the carries, the tiles' scans, the smoothing with the multiply, and
    // the stats.  Returns the device signal yc (f64, laid out as y; y itself when there is no sample).  L is read on the device and kept in
    // this object's stats before the stage behind measures yc with the same meter.  stats_host() holds 3 doubles per signal (L, T, -max ut)
    // once s has been synchronised.  keep_parts: e and s of every sample are written too (the test hook's view).
    const double* run(const double* y, const std::vector<FmtSignal>& sig, int rate, const DynamicsSpec& d, LoudnessMeter& meter, hipStream_t s,
                      bool keep_parts = false);
    const double* stats_host() const { return stats_host_; }
    // Where the last run left what its launches write (device; read only; valid on its stream until the next run); e and s only with
    // keep_parts.  For the test hook sbv2_debug_dynamics.
    struct Parts {
        const double *e = nullptr, *s = nullptr, *yc = nullptr;
        const int64_t *dq = nullptr, *u = nullptr;
    };
    const Parts& parts() const { return parts_; }

  private:
    Parts parts_;
    PinnedBuffer host_;   // signal table, Hann taps, then the stats
    DeviceBuffer dev_;
    double* stats_host_ = nullptr;
};

}  // namespace sbv2
