// Output formats of the PCM (pcm_format.hip): rational polyphase resampling from 44.1 kHz, optional peak normalisation and the f32 -> s16
// quantiser, on the device, next to the PCM a run leaves in HBM.  Used by the pipeline fetch (api.cpp) and the streaming decoder (vits.cpp).
#pragma once
#include "common.h"

struct sbv2_pcm_format;

namespace sbv2 {

constexpr int kNativeRate = 44100;

// A checked output format and its filter geometry: y[j] = sum_k h[j M - k L + half] x[k], h of length 2 half + 1 at 44100 L Hz,
// seen as L polyphase branches of T taps each (branch p = h[p], h[p + L], ..., zero-padded).
struct PcmFmtSpec {
    int rate = kNativeRate, encoding = 0, normalize = 0;
    int L = 1, M = 1, half = 0, T = 1;
    int bytes() const { return encoding == 1 ? 2 : 4; }
    bool identity() const { return L == 1 && M == 1 && encoding == 0 && normalize == 0; }
};
// throws with a message for unsupported rates / encodings / normalise modes and a non-zero reserved field
PcmFmtSpec pcm_format_spec(const sbv2_pcm_format* f);
// ceil(n L / M)
int64_t pcm_format_out_len(const PcmFmtSpec& s, int64_t n);
// the prototype h[2 half + 1] of a rate: Kaiser-windowed sinc (cutoff 0.45 min(44100, rate), beta 8.6, half = 32 max(L, M)), every polyphase
// branch scaled to sum to 1; h = {1} at 44100
std::vector<double> pcm_format_prototype(int rate, int* L, int* M, int* half);

// the modified Bessel function I0 (Kaiser windows)
double bessel_i0(double x);

// Input of one formatting launch.  A piece = native samples src[0, len) lying at positions [t0, t0 + len) of a signal's silent timeline;
// a signal = output samples [j0, j1) of that timeline, written at dst[out_off ...]; its pieces are [p0, p1), sorted by t0, disjoint.
struct FmtPiece {
    const float* src;
    int64_t t0, len;
};
struct FmtSignal {
    int64_t j0, j1, out_off;
    int32_t p0, p1;
};

class LoudnessMeter;   // loudness.h
struct LoudnessSpec;
class Limiter;   // limiter.h
struct LimiterSpec;

// Device state of the formatting launches of one execution context: the polyphase tables (per rate, built once), the tables of pieces /
// signals (one pinned + device pair per `slot`: a slot's host copy is rewritten only once the launch that used it has completed), the
// per-signal peaks, the f64 intermediate of the normalising path and an output buffer.
class PcmFormatter {
  public:
    explicit PcmFormatter(int device) : device_(device) {}
    ~PcmFormatter();
    PcmFormatter(const PcmFormatter&) = delete;
    PcmFormatter& operator=(const PcmFormatter&) = delete;
    // device buffer of >= bytes, used on stream s only (grown on demand; growing synchronises s, callers size it before a stream starts)
    void* out_buffer(size_t bytes, hipStream_t s);
    // enqueues the formatting of `sig` on `s`: total = sum of the signals' j1 - j0 samples into dst_dev (device, total * spec.bytes() bytes)
    void run(const PcmFmtSpec& spec, const std::vector<FmtPiece>& pieces, const std::vector<FmtSignal>& sig, int64_t total, void* dst_dev,
             int slot, hipStream_t s);
    // the same with a loudness gain (spec.normalize must be 0): y in f64, meter.measure(y) (loudness.hip), then y times each signal's gain.
    // Runs the meter also when every signal is empty.
    void run_loudness(const PcmFmtSpec& spec, const std::vector<FmtPiece>& pieces, const std::vector<FmtSignal>& sig, int64_t total,
                      void* dst_dev, int slot, hipStream_t s, LoudnessMeter& meter, const LoudnessSpec& ln);

    // the same through the look-ahead limiter (spec.normalize must be 0): y in f64, limiter.run(y, meter) (limiter.hip), then its x as it is.
    void run_limited(const PcmFmtSpec& spec, const std::vector<FmtPiece>& pieces, const std::vector<FmtSignal>& sig, int64_t total,
                     void* dst_dev, int slot, hipStream_t s, LoudnessMeter& meter, Limiter& limiter, const LimiterSpec& lim);

  private:
    void run_impl(const PcmFmtSpec& spec, const std::vector<FmtPiece>& pieces, const std::vector<FmtSignal>& sig, int64_t total, void* dst_dev,
                  int slot, hipStream_t s, LoudnessMeter* meter, const LoudnessSpec* ln, Limiter* limiter = nullptr,
                  const LimiterSpec* lim = nullptr);
    struct Slot {
        void* host = nullptr;
        void* dev = nullptr;
        size_t cap = 0;
    };
    const float* taps(const PcmFmtSpec& spec, hipStream_t s);
    int device_;
    std::map<int, float*> taps_;       // rate -> [L][T] polyphase table
    std::vector<Slot> slots_;
    double* tmp_ = nullptr;            // normalising path: y before the gain
    size_t tmp_cap_ = 0;
    unsigned long long* peak_ = nullptr;   // max |y| (f64 bit pattern), one per signal
    size_t peak_cap_ = 0;
    void* out_ = nullptr;
    size_t out_cap_ = 0;
};

}  // namespace sbv2
