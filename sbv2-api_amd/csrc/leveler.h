// Loudness follower of a stream (leveler.hip): the stage between the formatter's f64 signal y and the stream limiter (StreamLimiter,
// limiter.h) of a level stream begun with a sbv2_stream_leveler.  The convention is the header comment of struct sbv2_stream_leveler
// (include/sbv2_hip.h): the BS.1770 meter of loudness.hip as a fold carried from push to push, its gated mean over everything heard so far, and
// a gain that walks from the caller's gain_db towards target - loudness at a bounded rate, decided per quarter (S = fs / 10 samples) from
// complete earlier quarters only and applied as a linear ramp.  Nothing here looks ahead: the stream still runs the limiter's A samples late.
#pragma once
#include "common.h"

struct sbv2_stream_leveler;

namespace sbv2 {

// a checked sbv2_stream_leveler
struct StreamLevelerSpec {
    double target = 0.0, range = 0.0, slew = 0.0;   // LUFS, dB, dB per second
    int hold = 0;                                   // blocks above the absolute gate before the gain moves
};
// throws with a message for a null pointer, out-of-range or non-finite fields and a non-zero reserved field
StreamLevelerSpec stream_leveler_spec(const sbv2_stream_leveler* lv);

// The follower fed piece by piece: begin, then pushes in stream order, each in place on the samples the formatter just wrote.  Every sample
// leaves with the bits it would have if the whole signal were pushed at once, however the signal is cut: what is carried on the device is the
// 4-double filter state, the samples of the unfinished K-weighting segment (< m), the segment partials of the unfinished quarter, the last
// three quarter energies, the block history z_j and the schedule g_k / a_k (ceil(total / S) doubles each, sized at begin), the running stats.
// Nothing here waits for the GPU after begin (which may grow the buffers): which segments and quarters a push completes follows from the counts.
class StreamLeveler {
  public:
    StreamLeveler() = default;
    StreamLeveler(const StreamLeveler&) = delete;
    StreamLeveler& operator=(const StreamLeveler&) = delete;
    // a stream of total_samples at `rate`, fed in pushes of up to max_push samples, starting at gain_db
    void begin(int rate, int64_t total_samples, int64_t max_push, const StreamLevelerSpec& spec, double gain_db, hipStream_t s);
    // The n samples at y (device f64) join the stream and are scaled in place; `last`: the stream ends with them.  At most five launches:
    // k_lvl_zero, k_lvl_fold, k_lvl_rerun (when the push completes a segment), k_lvl_schedule (when it completes a quarter), k_lvl_apply.  The
    // last push also enqueues the copy of the stats to the host.
    void push(double* y_inout, int64_t n, bool last, hipStream_t s);
    int64_t fed() const { return fed_; }
    // (L_in = the gated loudness of the last complete quarter, the last g, min g, max g), valid once s has passed the last push
    void stats(double* out) const;
    // g_k in dB, k = 0 .. quarters() (device; valid on the stream behind the pushes): quarters() = the complete quarters fed so far
    const double* gains_dev() const { return g_; }
    int64_t quarters() const { return fed_ / S_; }

  private:
    DeviceBuffer dev_;    // carry | tail | quarter partials | e | st | z history | g | a
    PinnedBuffer host_;   // the stats
    double *carry_ = nullptr, *tail_ = nullptr, *part_ = nullptr, *e_ = nullptr, *st_ = nullptr, *hist_ = nullptr, *g_ = nullptr, *a_ = nullptr;
    StreamLevelerSpec spec_;
    double tab_[26] = {};   // c[10], A^m[16]
    double gain_db_ = 0.0;
    int rate_ = 0, m_ = 0, S_ = 0;
    int64_t total_ = 0, max_push_ = 0, fed_ = 0, nq_cap_ = 0;
    bool done_ = false;
};

}  // namespace sbv2
