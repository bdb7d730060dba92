// Output formats of the PCM (pcm_format.hip): rational polyphase resampling from 44.1 kHz, optional peak normalisation and the f32 -> s16
// quantiser (with the G.711 mu-law / A-law codes of its integers as two more deliveries), on the device, next to the PCM a run leaves in HBM.  Used by the formatted fetches (fetch_formatted, fetch.cpp) and the streaming decoder (vits.cpp).
#pragma once
#include "common.h"

struct sbv2_pcm_format;

namespace sbv2 {

constexpr int kNativeRate = 44100;

// sbv2_pcm_format.encoding: f32, s16 and the two G.711 laws under their WAVE format tags (one byte per sample)
constexpr int kEncF32 = 0, kEncS16 = 1, kEncAlaw = 6, kEncMulaw = 7;
inline bool pcm_encoding_known(int e) { return e == kEncF32 || e == kEncS16 || e == kEncAlaw || e == kEncMulaw; }
inline bool pcm_encoding_g711(int e) { return e == kEncAlaw || e == kEncMulaw; }
inline int pcm_encoding_bytes(int e) { return e == kEncS16 ? 2 : pcm_encoding_g711(e) ? 1 : 4; }

// G.711 on the s16 integer q in [-32767, 32767] (the convention above sbv2_pcm_format, include/sbv2_hip.h), in integer arithmetic: the same
// lines serve the device quantisers (pcm_format.hip), the level reduction (marks.hip) and the host functions sbv2_g711_encode / _decode.
__host__ __device__ inline int g711_lg(int m) {   // floor(log2 m), m >= 1
#ifdef __HIP_DEVICE_COMPILE__
    return 31 - __clz(m);
#else
    return 31 - __builtin_clz((unsigned)m);
#endif
}
__host__ __device__ inline uint8_t mulaw_encode(int q) {
    const int a = q < 0 ? -q : q, m = (a < 32635 ? a : 32635) + 132;   // saturates, never wraps
    const int e = g711_lg(m) - 7;                                      // 0 .. 7
    return (uint8_t)~((q < 0 ? 0x80 : 0) | e << 4 | ((m >> (e + 3)) & 15));
}
__host__ __device__ inline int mulaw_decode(uint8_t code) {
    const int u = ~code & 0xFF, t = (((u & 15) << 3) + 132) << ((u >> 4) & 7);
    return u & 0x80 ? 132 - t : t - 132;
}
__host__ __device__ inline uint8_t alaw_encode(int q) {
    const int m = (q >= 0 ? q : -q - 1) >> 3;
    const int e = m < 32 ? 0 : g711_lg(m) - 4;   // 0 .. 7
    return (uint8_t)(((q >= 0 ? 0x80 : 0) | e << 4 | ((m >> (e == 0 ? 1 : e)) & 15)) ^ 0x55);
}
__host__ __device__ inline int alaw_decode(uint8_t code) {
    const int a = code ^ 0x55, e = (a >> 4) & 7;
    int t = ((a & 15) << 4) + 8;
    if (e >= 1) t = (t + 256) << (e - 1);
    return a & 0x80 ? t : -t;
}

// A checked output format and its filter geometry: y[j] = sum_k h[j M - k L + half] x[k], h of length 2 half + 1 at 44100 L Hz,
// seen as L polyphase branches of T taps each (branch p = h[p], h[p + L], ..., zero-padded).
struct PcmFmtSpec {
    int rate = kNativeRate, encoding = 0, normalize = 0;
    int L = 1, M = 1, half = 0, T = 1;
    int bytes() const { return pcm_encoding_bytes(encoding); }
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
class Dynamics;   // dynamics.h
struct DynamicsSpec;

// The gain stage of a formatting run, between the resampler and the quantiser: none (peak-normalise or not, as spec.normalize says), a
// loudness gain from `meter` (loudness.hip), or the look-ahead limiter (limiter.hip).  A fourth kind ends the run at the stage's input: y
// (f64) is written to a caller-given address and nothing else happens (the level control of a stream takes it from there, stream_output.cpp).
// A loudness or limiter stage may have the speech compressor (dynamics.hip) in front of it: the stage then works on its output yc in place of y.
struct GainStage {
    enum Kind { kNone, kLoudness, kLimiter, kExposeY };
    GainStage() = default;
    explicit GainStage(double* y_dev) : kind(kExposeY), y_out(y_dev) {}
    GainStage(LoudnessMeter& m, const LoudnessSpec& l, Dynamics* dy = nullptr, const DynamicsSpec* ds = nullptr)
        : kind(kLoudness), meter(&m), ln(&l), dynamics(dy), dyn(ds) {}
    GainStage(LoudnessMeter& m, Limiter& li, const LimiterSpec& l, Dynamics* dy = nullptr, const DynamicsSpec* ds = nullptr)
        : kind(kLimiter), meter(&m), limiter(&li), lim(&l), dynamics(dy), dyn(ds) {}
    const Kind kind = kNone;
    LoudnessMeter* const meter = nullptr;   // the meter of y (both stages)
    const LoudnessSpec* const ln = nullptr;
    Limiter* const limiter = nullptr;
    const LimiterSpec* const lim = nullptr;
    Dynamics* const dynamics = nullptr;     // the compressor in front of the stage (both stages), or none
    const DynamicsSpec* const dyn = nullptr;
    double* const y_out = nullptr;          // kExposeY: total doubles on the device
};

// Device state of the formatting launches of one execution context: the polyphase tables (per rate, built once), the tables of pieces /
// signals (one pinned + device pair per `slot`: a slot's host copy is rewritten only once the launch that used it has completed), the
// per-signal peaks, the f64 intermediate of the normalising path and an output buffer.  Nothing is allocated before the first run.
class PcmFormatter {
  public:
    PcmFormatter() = default;
    PcmFormatter(const PcmFormatter&) = delete;
    PcmFormatter& operator=(const PcmFormatter&) = delete;
    // device buffer of >= bytes, used on stream s only (grown on demand; growing synchronises s, callers size it before a stream starts)
    void* out_buffer(size_t bytes, hipStream_t s) { return out_.reserve(bytes, s); }
    // enqueues the formatting of `sig` on `s`: total = sum of the signals' j1 - j0 samples into dst_dev (device, total * spec.bytes() bytes).
    // With a gain stage (spec.normalize must be 0): y in f64, then meter.measure(y) and y times each signal's gain, or limiter.run(y, meter)
    // and its x as it is; the stage runs also when every signal is empty, so that its stats are written.  kExposeY: y to gain.y_out, dst_dev unused.
    void run(const PcmFmtSpec& spec, const std::vector<FmtPiece>& pieces, const std::vector<FmtSignal>& sig, int64_t total, void* dst_dev,
             int slot, hipStream_t s, const GainStage& gain = GainStage());
    // max |y| of each signal of the last peak-normalised run that had samples (device, valid once that run's launches have completed; the
    // test hook's view of the gain k_pcm_gain applies)
    const double* peaks_device() const { return peak_.as<double>(); }

  private:
    struct Slot {
        PinnedBuffer host;
        DeviceBuffer dev;
    };
    const float* taps(const PcmFmtSpec& spec, hipStream_t s);
    std::map<int, DeviceBuffer> taps_;   // rate -> [L][T] polyphase table
    std::vector<Slot> slots_;
    DeviceBuffer tmp_;    // normalising path: y (f64) before the gain
    DeviceBuffer peak_;   // max |y| (f64 bit pattern), one per signal
    DeviceBuffer out_;
};

// n f64 samples x (device) times *unit (one device double) -> dst in `encoding` (0: f32, 1: s16, 7 / 6: G.711 codes), with the cast /
// quantiser of the gain stages
void pcm_cast(const double* x, int64_t n, const double* unit, int encoding, void* dst_dev, hipStream_t s);
// The gain-stage kernel on its own (the test hook's entry): total f64 samples y (device) of the signals in `sig` (device, nsig entries; only
// out_off is read), sample o times gain[its signal] (device) -> dst in `encoding`
void pcm_gain_signals(const double* y, const FmtSignal* sig, int nsig, const double* gain, int64_t total, int encoding, void* dst_dev, hipStream_t s);

}  // namespace sbv2
