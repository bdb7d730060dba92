// PCM output formats on the device: 44.1 kHz -> R rational polyphase resampling, optional per-signal peak normalisation, f32 -> s16 quantiser,
// G.711 mu-law / A-law codes of the s16 integers.
//
// Convention (the one tests/test_pcm_format.py pins): for a native signal x[0, N) (zero outside), L / M = R / 44100 in lowest terms,
//   y[j] = sum_k h[j M - k L + half] x[k],   j in [0, ceil(N L / M)),
// which is scipy.signal.resample_poly(x, L, M, window = h / L).  h: odd-length Kaiser-windowed sinc at 44100 L Hz, designed here on the host.
//
// Kernel design: one thread per output sample, f64 accumulation; the thread's polyphase branch (T <= 353 taps) and its input span are read
// through the caches.  Neighbouring lanes read neighbouring input spans (the span of lane i + 1 starts M / L input samples later), so the PCM
// comes from HBM once; the table is stored tap-major ([T][L]), so at step t a wave's 64 tap loads fall in one L-float row (3 - 10 cache lines)
// instead of 64 branch rows (the largest table is 110 KB: it stays in every XCD's L2).  The input is a table of pieces on silent timelines,
// so one launch formats a whole run (utterance per signal, or all utterances on one joined timeline, or the windows of a streaming replay).
// Every output is the same ordered sum of T products whatever the piece layout around it (samples outside every piece enter as zeros), so
// a streamed window and the whole utterance give the same bits.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>
#include <type_traits>

#include "../../include/sbv2_hip.h"
#include "dynamics.h"
#include "limiter.h"
#include "loudness.h"
#include "pcm_format.h"

namespace sbv2 {

namespace {

constexpr int kRates[] = {8000, 16000, 22050, 24000, 32000, 44100, 48000};
constexpr int kZeroCrossings = 32;
constexpr double kCutoff = 0.45, kBeta = 8.6;

bool branch_major() {
    static const bool on = getenv("SBV2_PCM_TAPS") && std::string(getenv("SBV2_PCM_TAPS")) == "branch";
    return on;
}

struct KArgs {
    const FmtPiece* pieces;
    const FmtSignal* sig;
    int nsig;
    const float* taps;   // tap t of branch p at taps[p * sp + t * st]
    int L, M, half, T;
    int sp, st;
    int64_t total;
};

__device__ __forceinline__ int find_signal(const FmtSignal* sig, int nsig, int64_t o) {
    int lo = 0, hi = nsig - 1;   // last signal with out_off <= o (an empty signal shares its out_off with the next one)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (sig[mid].out_off <= o) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// y of output o (o < total), summed in f64 (the s16 quantiser then rounds the exact value: no f32 accumulation error moves a sample to the
// next step); *s = its signal
__device__ __forceinline__ double resample_one(const KArgs& a, int64_t o, int* s_out) {
    const int s = find_signal(a.sig, a.nsig, o);
    *s_out = s;
    const FmtSignal g = a.sig[s];
    const int64_t j = g.j0 + (o - g.out_off);
    const int64_t i0 = j * a.M + a.half;   // >= 0
    const int64_t kmax = i0 / a.L;
    const float* h = a.taps + (size_t)(i0 - kmax * a.L) * a.sp;
    // last piece starting at or before kmax
    int q = g.p0 - 1;
    {
        int lo = g.p0, hi = g.p1 - 1;
        while (lo <= hi) {
            const int mid = (lo + hi) >> 1;
            if (a.pieces[mid].t0 <= kmax) {
                q = mid;
                lo = mid + 1;
            } else {
                hi = mid - 1;
            }
        }
    }
    int64_t ct0 = INT64_MIN, cend = INT64_MIN;
    const float* csrc = nullptr;
    if (q >= g.p0) {
        ct0 = a.pieces[q].t0;
        cend = ct0 + a.pieces[q].len;
        csrc = a.pieces[q].src;
    }
    double acc = 0.0;
    for (int t = 0; t < a.T; ++t) {
        const int64_t k = kmax - t;
        while (k < ct0) {   // the span crosses into an earlier piece (or before the first one)
            --q;
            if (q >= g.p0) {
                ct0 = a.pieces[q].t0;
                cend = ct0 + a.pieces[q].len;
                csrc = a.pieces[q].src;
            } else {
                ct0 = cend = INT64_MIN;
            }
        }
        const double x = k < cend ? (double)csrc[k - ct0] : 0.0;
        acc = t == 0 ? (double)h[0] * x : fma((double)h[(size_t)t * a.st], x, acc);   // (first product, not 0 + product: the identity rate keeps -0.0)
    }
    return acc;
}

__device__ __forceinline__ short quantise(double v) {
    return (short)fmin(fmax(rint(v * 32767.0), -32767.0), 32767.0);
}

// The G.711 quantisers: the code of the s16 integer that quantise() delivers (mulaw_encode / alaw_encode, pcm_format.h), one byte per sample
__device__ __forceinline__ uint8_t quantise_mulaw(double v) { return mulaw_encode(quantise(v)); }
__device__ __forceinline__ uint8_t quantise_alaw(double v) { return alaw_encode(quantise(v)); }

// The delivered encodings as the kernels number them (ENC): 0 f32, 1 s16, 4 mu-law, 5 A-law (2 and 3 are the f64 paths below; the public
// values of sbv2_pcm_format.encoding are translated in with_enc and mean nothing here).  One store per thread: signals lie back to back, so a
// G.711 signal starts at any byte offset and a byte store needs no alignment, no tail and no care for a dword that straddles two signals.
constexpr int kEncKernelMulaw = 4, kEncKernelAlaw = 5;
template <int ENC>
__device__ __forceinline__ void deliver(void* dst, int64_t o, double v) {
    static_assert(ENC == 0 || ENC == 1 || ENC == kEncKernelMulaw || ENC == kEncKernelAlaw, "not a delivered encoding");
    if constexpr (ENC == 0) static_cast<float*>(dst)[o] = (float)v;
    else if constexpr (ENC == 1) static_cast<short*>(dst)[o] = quantise(v);
    else if constexpr (ENC == kEncKernelMulaw) static_cast<uint8_t*>(dst)[o] = quantise_mulaw(v);
    else static_cast<uint8_t*>(dst)[o] = quantise_alaw(v);
}
// f(std::integral_constant<int, ENC>) for the ENC of a checked sbv2_pcm_format.encoding
template <class F>
void with_enc(int encoding, F&& f) {
    switch (encoding) {
        case kEncF32: f(std::integral_constant<int, 0>()); break;
        case kEncS16: f(std::integral_constant<int, 1>()); break;
        case kEncMulaw: f(std::integral_constant<int, kEncKernelMulaw>()); break;
        case kEncAlaw: f(std::integral_constant<int, kEncKernelAlaw>()); break;
        default: SBV2_REQUIRE(false, "internal: unknown PCM encoding " + std::to_string(encoding));
    }
}

// ENC 0 / 1 / 4 / 5: delivered as above, 2: f64 y into dst + per-signal max |y| for the normalising pass (atomicMax on the bit pattern of a non-negative
// double: exact and order-independent, so the gain is the same on every run), 3: f64 y alone (the loudness path: its meter finds the peak)
template <int ENC>
__global__ __launch_bounds__(256) void k_pcm_resample(KArgs a, void* dst, unsigned long long* peak) {
    const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = o < a.total;
    int s = -1;
    double y = 0.0;
    if (live) y = resample_one(a, o, &s);
    if constexpr (ENC == 3) {
        if (live) static_cast<double*>(dst)[o] = y;
    } else if constexpr (ENC != 2) {
        if (live) deliver<ENC>(dst, o, y);
    } else {
        if (live) static_cast<double*>(dst)[o] = y;
        double m = live ? fabs(y) : 0.0;
        const int s0 = __shfl(s, 0);
        if (__all(!live || s == s0)) {   // one signal in the wave: reduce first, one atomic
            for (int d = 32; d >= 1; d >>= 1) m = fmax(m, __shfl_xor(m, d));
            if (threadIdx.x % warpSize == 0 && s0 >= 0) atomicMax(peak + s0, (unsigned long long)__double_as_longlong(m));
        } else if (live) {
            atomicMax(peak + s, (unsigned long long)__double_as_longlong(m));
        }
    }
}

// y * g, g = 1 / peak of y's signal (1 for a silent signal), -> a delivered encoding
template <int ENC>
__global__ __launch_bounds__(256) void k_pcm_gain(const double* y, const FmtSignal* sig, int nsig, const unsigned long long* peak, int64_t total,
                                                  void* dst) {
    const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= total) return;
    const int s = find_signal(sig, nsig, o);
    const double pk = __longlong_as_double((long long)peak[s]);
    const double g = pk > 0.0 ? 1.0 / pk : 1.0;
    deliver<ENC>(dst, o, y[o] * g);
}

// y * gain[s] (the loudness gain of y's signal, loudness.hip) -> a delivered encoding
template <int ENC>
__global__ __launch_bounds__(256) void k_pcm_gain_sig(const double* y, const FmtSignal* sig, int nsig, const double* gain, int64_t total,
                                                      void* dst) {
    const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= total) return;
    deliver<ENC>(dst, o, y[o] * gain[find_signal(sig, nsig, o)]);
}

}  // namespace

double bessel_i0(double x) {
    double sum = 1.0, term = 1.0;
    for (int k = 1; k < 500; ++k) {
        term *= (x / (2.0 * k)) * (x / (2.0 * k));
        sum += term;
        if (term < 1e-17 * sum) break;
    }
    return sum;
}

// L, M and half of a supported rate: the one place both the table (pcm_format_prototype) and the kernel geometry (pcm_format_spec) come from
static void rate_geometry(int rate, int* L, int* M, int* half) {
    SBV2_REQUIRE(std::find(std::begin(kRates), std::end(kRates), rate) != std::end(kRates),
                 "unsupported sample rate " + std::to_string(rate) + " (8000 16000 22050 24000 32000 44100 48000)");
    const int g = std::gcd(rate, kNativeRate);
    *L = rate / g;
    *M = kNativeRate / g;
    *half = *L == *M ? 0 : kZeroCrossings * std::max(*L, *M);
}

std::vector<double> pcm_format_prototype(int rate, int* L, int* M, int* half) {
    rate_geometry(rate, L, M, half);
    const int l = *L, hf = *half;
    if (hf == 0) return {1.0};
    const double fs_up = (double)kNativeRate * l, fc = kCutoff * std::min(kNativeRate, rate), i0b = bessel_i0(kBeta);
    std::vector<double> h(2 * (size_t)hf + 1);
    for (int n = -hf; n <= hf; ++n) {
        const double x = 2.0 * fc / fs_up * n, r = (double)n / hf;
        const double sinc = n == 0 ? 1.0 : std::sin(M_PI * x) / (M_PI * x);
        h[n + hf] = sinc * bessel_i0(kBeta * std::sqrt(std::max(0.0, 1.0 - r * r))) / i0b;
    }
    for (int p = 0; p < l; ++p) {   // every polyphase branch sums to 1: a constant passes unchanged at every output phase
        double sum = 0.0;
        for (size_t i = p; i < h.size(); i += l) sum += h[i];
        for (size_t i = p; i < h.size(); i += l) h[i] /= sum;
    }
    return h;
}

PcmFmtSpec pcm_format_spec(const sbv2_pcm_format* f) {
    SBV2_REQUIRE(f, "no PCM format given");
    SBV2_REQUIRE(pcm_encoding_known(f->encoding),
                 "unsupported PCM encoding " + std::to_string(f->encoding) + " (0 = f32, 1 = s16, 7 = G.711 mu-law, 6 = G.711 A-law)");
    SBV2_REQUIRE(f->normalize == 0 || f->normalize == 1, "unsupported normalize mode " + std::to_string(f->normalize) + " (0 = none, 1 = peak)");
    SBV2_REQUIRE(f->reserved == 0, "sbv2_pcm_format.reserved must be 0");
    PcmFmtSpec s;
    s.rate = f->sample_rate;
    s.encoding = f->encoding;
    s.normalize = f->normalize;
    rate_geometry(s.rate, &s.L, &s.M, &s.half);
    s.T = (2 * s.half + 1 + s.L - 1) / s.L;
    return s;
}

int64_t pcm_format_out_len(const PcmFmtSpec& s, int64_t n) { return n <= 0 ? 0 : (n * s.L + s.M - 1) / s.M; }

const float* PcmFormatter::taps(const PcmFmtSpec& spec, hipStream_t s) {
    auto it = taps_.find(spec.rate);
    if (it != taps_.end()) return it->second.as<float>();
    int L, M, half;
    const std::vector<double> h = pcm_format_prototype(spec.rate, &L, &M, &half);
    // default [T][L]: tap t of branch p = h[p + t L] sits at t L + p, i.e. the table is h itself, zero-padded to T L.  At step t the lanes of a wave
    // (consecutive outputs, branches spread over all L) read one contiguous L-float row.  SBV2_PCM_TAPS=branch: [L][T] (each branch contiguous,
    // every lane on its own row: the A/B of DESIGN.md §8b; same values, same summation order, same bits)
    std::vector<float> tab((size_t)L * spec.T, 0.f);
    for (size_t i = 0; i < h.size(); ++i) tab[branch_major() ? (i % L) * spec.T + i / L : i] = (float)h[i];
    float* d = static_cast<float*>(taps_[spec.rate].reserve(sizeof(float) * tab.size(), s));
    HIP_CHECK(hipMemcpyAsync(d, tab.data(), sizeof(float) * tab.size(), hipMemcpyHostToDevice, s));
    HIP_CHECK(hipStreamSynchronize(s));
    return d;
}

// the stage on the f64 signal y (null when there is no sample): returns the signal to deliver, *gain = one gain per signal for it
static const double* apply_gain(const GainStage& g, const double* y, const std::vector<FmtSignal>& sig, int rate, hipStream_t s,
                                const double** gain) {
    if (g.dynamics) y = g.dynamics->run(y, sig, rate, *g.dyn, *g.meter, s);   // yc takes y's place; the meter is free again behind it
    if (g.kind == GainStage::kLimiter) return g.limiter->run(y, sig, rate, *g.lim, *g.meter, s, gain);   // its own x and unit gains
    *gain = g.meter->measure(y, sig, rate, *g.ln, s);
    return y;
}

void PcmFormatter::run(const PcmFmtSpec& spec, const std::vector<FmtPiece>& pieces, const std::vector<FmtSignal>& sig, int64_t total, void* dst_dev,
                       int slot, hipStream_t s, const GainStage& stage) {
    const bool staged = stage.kind != GainStage::kNone;
    SBV2_REQUIRE(!(staged && spec.normalize), "internal: a gain stage on a peak-normalised format");
    if (sig.empty()) return;
    const double* gain = nullptr;
    if (total <= 0) {
        if (staged && stage.kind != GainStage::kExposeY) apply_gain(stage, nullptr, sig, spec.rate, s, &gain);
        return;
    }
    const float* tp = taps(spec, s);
    if ((int)slots_.size() <= slot) slots_.resize(slot + 1);
    Slot& sl = slots_[slot];
    const size_t pb = sizeof(FmtPiece) * pieces.size(), bytes = round_up64((int64_t)pb, 64) + sizeof(FmtSignal) * sig.size();
    const size_t cap = std::max<size_t>(bytes * 2, 4096);
    char* hb = static_cast<char*>(sl.host.reserve(bytes, cap, s));
    char* db = static_cast<char*>(sl.dev.reserve(bytes, cap, s));
    const size_t so = round_up64((int64_t)pb, 64);
    if (pb) std::memcpy(hb, pieces.data(), pb);
    std::memcpy(hb + so, sig.data(), sizeof(FmtSignal) * sig.size());
    HIP_CHECK(hipMemcpyAsync(db, hb, bytes, hipMemcpyHostToDevice, s));
    KArgs a;
    a.pieces = reinterpret_cast<const FmtPiece*>(db);
    a.sig = reinterpret_cast<const FmtSignal*>(db + so);
    a.nsig = (int)sig.size();
    a.taps = tp;
    a.L = spec.L;
    a.M = spec.M;
    a.half = spec.half;
    a.T = spec.T;
    a.sp = branch_major() ? spec.T : 1;
    a.st = branch_major() ? 1 : spec.L;
    a.total = total;
    const dim3 grid((unsigned)((total + 255) / 256)), block(256);
    if (!spec.normalize && !staged) {
        with_enc(spec.encoding, [&](auto e) { hipLaunchKernelGGL(k_pcm_resample<decltype(e)::value>, grid, block, 0, s, a, dst_dev, nullptr); });
        HIP_CHECK(hipGetLastError());
        return;
    }
    if (stage.kind == GainStage::kExposeY) {
        hipLaunchKernelGGL(k_pcm_resample<3>, grid, block, 0, s, a, stage.y_out, nullptr);
        HIP_CHECK(hipGetLastError());
        return;
    }
    double* tmp = static_cast<double*>(tmp_.reserve(sizeof(double) * (size_t)total, s));
    auto* peak = static_cast<unsigned long long*>(peak_.reserve(sizeof(unsigned long long) * sig.size(), s));
    if (staged) {
        hipLaunchKernelGGL(k_pcm_resample<3>, grid, block, 0, s, a, tmp, nullptr);
        const double* x = apply_gain(stage, tmp, sig, spec.rate, s, &gain);
        pcm_gain_signals(x, a.sig, a.nsig, gain, total, spec.encoding, dst_dev, s);
        return;
    }
    HIP_CHECK(hipMemsetAsync(peak, 0, sizeof(unsigned long long) * sig.size(), s));
    hipLaunchKernelGGL(k_pcm_resample<2>, grid, block, 0, s, a, tmp, peak);
    with_enc(spec.encoding, [&](auto e) { hipLaunchKernelGGL(k_pcm_gain<decltype(e)::value>, grid, block, 0, s, tmp, a.sig, a.nsig, peak, total, dst_dev); });
    HIP_CHECK(hipGetLastError());
}

void pcm_gain_signals(const double* y, const FmtSignal* sig, int nsig, const double* gain, int64_t total, int encoding, void* dst_dev, hipStream_t s) {
    if (total <= 0) return;
    const dim3 grid((unsigned)((total + 255) / 256)), block(256);
    with_enc(encoding, [&](auto e) { hipLaunchKernelGGL(k_pcm_gain_sig<decltype(e)::value>, grid, block, 0, s, y, sig, nsig, gain, total, dst_dev); });
    HIP_CHECK(hipGetLastError());
}

void pcm_cast(const double* x, int64_t n, const double* unit, int encoding, void* dst_dev, hipStream_t s) {
    // (one signal: find_signal answers 0 without reading the table)
    pcm_gain_signals(x, nullptr, 1, unit, n, encoding, dst_dev, s);
}

}  // namespace sbv2
