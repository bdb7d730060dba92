// Look-ahead true-peak limiter on the device (limiter.hip): the stage between the loudness meter and the gain / quantiser / FLAC encoder of
// sbv2_pipeline_fetch_pcm_limited / _fetch_flac_limited (the limiter GainStage of PcmFormatter::run), and of the test hook
// sbv2_debug_limiter.  The convention is the header comment of struct sbv2_limiter (include/sbv2_hip.h).  Its step 2 alone, at a gain the
// caller fixes, is the level control of a stream (struct sbv2_stream_level): in one shot (Limiter::run_fixed) or fed piece by piece with an
// O(K) tail carried on the device (StreamLimiter; StreamOutput::push, stream_output.cpp, and the sbv2_debug_limiter_fixed / _stream hooks).
#pragma once
#include "common.h"
#include "loudness.h"
#include "pcm_format.h"

struct sbv2_limiter;
struct sbv2_stream_level;

namespace sbv2 {

// a checked sbv2_limiter
struct LimiterSpec {
    double target = 0.0, ceiling = 0.0, depth = 0.0;   // LUFS, dBTP, max_reduction_db
};
// throws with a message for a null pointer, out-of-range or non-finite fields and a non-zero reserved field
LimiterSpec limiter_spec(const sbv2_limiter* lim);

// a checked sbv2_stream_level
struct StreamLevelSpec {
    double gain_db = 0.0, ceiling = 0.0;   // dB, dBTP
};
// throws with a message for a null pointer, out-of-range or non-finite fields and non-zero reserved fields
StreamLevelSpec stream_level_spec(const sbv2_stream_level* lv);
// A = K - 1 + 12 at `rate`: the samples that must follow a sample before its gain is final (throws for a rate the limiter has no window for)
int64_t stream_level_lookahead(int rate);

// What the limiter shares with the compressor in front of it (dynamics.hip), so that both read ONE envelope and ONE window: the signal table,
// step 1 of sbv2_limiter and the taps of its smoothing window.
constexpr int kLimTile = 1024;   // samples per workgroup of the curve kernels; a tile never straddles a signal edge
struct LimSig {
    int64_t off, n, tile0;   // samples y[off, off + n); its tiles are [tile0, tile0 + ceil(n / kLimTile))
};
__device__ __forceinline__ int lim_find_tile(const LimSig* sig, int nsig, int64_t k) {   // last signal with tile0 <= k
    int lo = 0, hi = nsig - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (sig[mid].tile0 <= k) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}
// e[p] of step 1 from the interpolated magnitudes t (limiter_interp) of ONE signal, 0 <= p < n: y and t are indexed by the position in it
__device__ __forceinline__ double lim_envelope_at(const double* y, const double* t, int64_t p) {
    return fmax(fmax(p > 0 ? t[p - 1] : 0.0, fabs(y[p])), t[p]);
}
// t[o] = max |z[4 o + 1 .. 4 o + 3]| of the `total` samples y of the signals in sig (device table), one launch on s
void limiter_interp(const double* y, const LimSig* sig, int nsig, int64_t total, double* t, hipStream_t s);
// K = rate / 100 (throws for a rate the window does not cover); sin^2(pi (k + 0.5) / K) scaled to sum to 1 into h[K], returns their sum
// in ascending k
constexpr int kLimMaxK = 480;   // 10 ms at 48 kHz
int limiter_window(int rate);
double limiter_hann_taps(int K, double* h);

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
    // Step 2 alone at the fixed gain of lv, once, without a meter: returns x as run does; stats_host() then holds 2 doubles per signal
    // (20 log10 min s, max |x|) once s has been synchronised.
    const double* run_fixed(const double* y, const std::vector<FmtSignal>& sig, int rate, const StreamLevelSpec& lv, hipStream_t s);
    const double* stats_host() const { return stats_host_; }
    // Where the last run left what its launches read and write (device; read only; valid on its stream until the next run): the Hann taps
    // h [K] with their sum as the kernel gets it, t and x [total], smin [tiles], each of the three followed by pad words up to the next array
    // (smin up to `end`).  For the test hook sbv2_debug_limiter_parts.
    struct Parts {
        const double *h = nullptr, *t = nullptr, *x = nullptr, *smin = nullptr, *end = nullptr;
        int64_t total = 0, tiles = 0;
        int K = 0;
        double hsum = 0.0;
    };
    const Parts& parts() const { return parts_; }

  private:
    Parts parts_;
    LoudnessMeter xmeter_;   // the meter of x (its own scratch: the stats of y stay in the caller's meter)
    PinnedBuffer host_;      // signal table, Hann taps, then the stats
    DeviceBuffer dev_;
    double* stats_host_ = nullptr;
};

// The fixed-gain limiter fed piece by piece (a synthesis stream's replays): begin, then pushes in stream order.  Every emitted sample has the
// bits run_fixed gives it on the whole signal, however the signal is cut.  After pushes of S samples in all, max(0, S - A) samples have been
// emitted, A = stream_level_lookahead(rate); the last push emits the rest.  Nothing here waits for the GPU after begin (which may grow the
// buffers): what a push emits follows from the sample counts.
class StreamLimiter {
  public:
    StreamLimiter() = default;
    StreamLimiter(const StreamLimiter&) = delete;
    StreamLimiter& operator=(const StreamLimiter&) = delete;
    // a stream of total_samples at `rate`, fed in pushes of up to max_push samples: nothing fed, the running stats at (1, 0)
    void begin(int rate, int64_t total_samples, int64_t max_push, const StreamLevelSpec& lv, hipStream_t s);
    // where the next push's f64 samples go (device): right behind the carried tail
    double* dst() const;
    // The n samples at dst() join the stream; `last`: the stream ends with them.  Writes the samples this push completes to out (device f64,
    // up to n + A of them) and returns their count = emitted_after(fed) - emitted_after(fed before).  The last push also enqueues the copy
    // of the stats to the host.
    int64_t push(int64_t n, bool last, double* out, hipStream_t s);
    int64_t emitted_after(int64_t fed, bool last) const;
    int64_t lookahead() const { return A_; }
    int64_t fed() const { return fed_; }   // samples pushed so far
    double* out_buffer() const;     // max_push + A doubles of this object's for `out`
    const double* unit() const;     // one device double of 1.0: the gain the cast kernel multiplies the emitted x by
    // (20 log10 min s, max |x|) over the whole stream; valid once s has passed the last push
    void stats(double* out) const;

  private:
    DeviceBuffer buf_[2];   // [tail | new samples], taking turns
    DeviceBuffer t_;        // the window's interpolated magnitudes
    DeviceBuffer x_;
    DeviceBuffer aux_;      // running stats and the unit gain | Hann taps | per-tile min s | per-tile max |x|
    PinnedBuffer host_;     // Hann taps, then the stats
    int K_ = 0, cur_ = 0;
    int64_t A_ = 0, total_ = 0, max_push_ = 0, fed_ = 0, emitted_ = 0, pos0_ = 0, tail_ = 0;
    double g0_ = 1.0, c_ = 1.0, hsum_ = 1.0;
    bool done_ = false;
};

}  // namespace sbv2
