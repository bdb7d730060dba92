// Look-ahead true-peak limiter on the device: reaches loudness targets that the scale-only gain of loudness.hip misses because the true peak
// binds first.  All of it in f64 on y (the resampled signal before any gain), between the meter and the f32 cast / s16 quantiser / FLAC encoder.
//
// Convention (struct sbv2_limiter in include/sbv2_hip.h; tests/test_limiter.py restates it in numpy): c = 10^(ceiling / 20), K = fs / 100,
//   e[n] = max |z[4 n + d]|, d in -3..3, z the 4x interpolation of the true-peak meter (z = 0 outside the signal);
//   r[n] = min(1, c / (g0 e[n])); m[n] = min r[n .. n + K - 1] (r = 1 past the end); s[n] = sum_k h[k] m[n - k] (m = m[0] before the
//   start, h a sin^2 window of K taps summing to 1); x[n] = y[n] g0 s[n].  Every m[n - k], m[0] for n < K - 1 included, is a minimum over
//   a window that contains n, so s[n] <= r[n] and |x[n]| <= c up to rounding; min(s, r[n]) and a clamp of x to +-c take the rounding off.
//   (m = 1 before the start, the first draft of the convention, breaks that for the first K - 1 samples: a loud onset would then be held
//   under the ceiling by the min alone, sample by sample, with steps of up to D dB between neighbours.)
//   G_0 = min(target - L, Gcap), Gcap = ceiling - TP + D, G_{i+1} = min(G_i + target - L(x at G_i), Gcap), delivered: x at G_2.
//   A signal with G_0 <= ceiling - TP (the scale alone fits, or D = 0) or L = -inf is idle: x = y times the gain of loudness.hip, bit for bit.
//
// Kernel design.
//   k_lim_interp  one thread per sample, the tiling and the tap order of k_true_peak (loudness.hip): t[n] = max |z[4 n + 1 .. 4 n + 3]| to HBM.
//                 e[n] = max(t[n - 1], |y[n]|, t[n]) is formed where it is read; it does not depend on G, so this runs once per fetch.
//   k_lim_init    one lane per signal: Gcap, G_0, the idle flag (an idle signal takes the meter's G and gain as they are).
//   k_lim_curve   one workgroup per tile of 1024 samples of ONE signal (tiles never straddle a signal edge; outside the signal r = 1, and
//                 the signal starts at the gain of its first window, m[0]).  r of the tile and a halo of 2 K - 2 samples goes to LDS (at
//                 most 1982 doubles); the sliding
//                 minimum is log2 K in-place doubling passes (a[i] = min(a[i], a[i + w])) and one min of two overlapping power-of-two
//                 windows; the Hann sum runs over k = 0 .. K - 1 in that order for every sample (4 samples per lane, taps read uniformly).
//                 A tile whose r is 1 throughout takes s = the same sum over ones (a kernel argument) without the K-tap loop.  Writes x
//                 and the tile's min s.  min is exact and order-free; every sum has a fixed order; no atomics.
//   k_lim_update  one wave per signal after the meter's k_gate on x: evaluations 0 and 1 move G, the last one writes the 6 stats.
// The meter of x is a second LoudnessMeter (the K-weighting passes and k_gate as they are; the true-peak pass only on the last evaluation).
//
// Fixed gain (struct sbv2_stream_level: step 2 alone at a pre-gain the caller names; no meter, no make-up loop, no idle rule).
//   One shot (Limiter::run_fixed): k_lim_fixed_init writes the states, then k_lim_interp and k_lim_curve once, k_lim_fixed_stats folds min s
//   and max |x| per signal.
//   Fed piece by piece (StreamLimiter): sample n of x depends on y[n - K - 11, n + K + 11] and on nothing else (t[o] reads y[o - 11, o + 12],
//   r[p] reads t[p - 1 .. p], m[j] reads r[j .. j + K - 1], s[n] reads m[n - K + 1 .. n]), so with S samples fed, x[0, S - A) is final,
//   A = K - 1 + 12.  A push runs the <true> instantiations of the same two kernels on the window [carried y | new y] as ONE signal: same
//   tap order, same exact minimum, same Hann sum, same shortcut; only the tile origin differs (the first sample not yet emitted instead of a
//   multiple of 1024), and no value depends on it.  The window starts A samples before the first sample to emit (or at the utterance's
//   start, where the m[0] rule then is the convention's) and ends A samples after the last one (or at the utterance's end, where r = 1
//   past it is the convention's): what the kernels assume beyond a window edge that is not a signal edge reaches no emitted sample.
//   k_lim_stream_fold folds the tiles' min s / max |x| into the stream's running pair (min and max are exact: no order to keep).
#include <algorithm>
#include <cmath>
#include <cstring>

#include "../../include/sbv2_hip.h"
#include "limiter.h"

namespace sbv2 {

namespace {

constexpr int kTile = 1024;
constexpr int kLanes = 256;
constexpr int kMaxK = 480;                        // 10 ms at 48 kHz
static_assert(kTile == kLimTile && kMaxK == kLimMaxK, "limiter.h states the same two for the compressor");
constexpr int kLdsLen = kTile + 2 * kMaxK - 2;   // r of a tile and its halo
constexpr int kTpBack = 12;                       // the interpolator's window is y[o - 11, o + 12] (loudness.hip)
static_assert(kLdsLen <= 8 * kLanes && kTile + kMaxK - 1 <= 6 * kLanes && kTile == 4 * kLanes, "k_lim_curve's per-lane counts");

struct LimState {
    double G, g0, Gcap;   // the pre-gain in dB and linear, its cap
    int64_t idle;         // the scale alone fits: x = y g0, g0 the meter's gain
};

__device__ __forceinline__ int find_off(const LimSig* sig, int nsig, int64_t o) {   // last signal with off <= o
    int lo = 0, hi = nsig - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (sig[mid].off <= o) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

struct InterpArgs {
    const double* y;
    const LimSig* sig;
    int nsig;
    int64_t total;
    double h[3][kTruePeakTaps];
    double* t;   // [total]: max |z| over the three interpolated samples after y[n]
};

// kStream: y is ONE signal of a.total samples (a stream's window, StreamLimiter::push); no table is read
template <bool kStream>
__global__ __launch_bounds__(kLanes) void k_lim_interp(InterpArgs a) {
    constexpr int kStage = kLanes + 2 * kTpBack - 1;
    __shared__ double tile[kStage];   // y[base - 11, base + 268)
    const int64_t base = (int64_t)blockIdx.x * kLanes;
    for (int i = threadIdx.x; i < kStage; i += kLanes) {
        const int64_t g = base - (kTpBack - 1) + i;
        tile[i] = g >= 0 && g < a.total ? a.y[g] : 0.0;
    }
    __syncthreads();
    const int64_t o = base + threadIdx.x;
    if (o >= a.total) return;
    const LimSig g = kStream ? LimSig{0, a.total, 0} : a.sig[find_off(a.sig, a.nsig, o)];
    const double* w = tile + threadIdx.x + 2 * kTpBack - 1;   // w[-d] = y[o + 12 - d]
    double z[3] = {0.0, 0.0, 0.0};
    if (o - (kTpBack - 1) >= g.off && o + kTpBack < g.off + g.n) {
#pragma unroll
        for (int d = 0; d < kTruePeakTaps; ++d) {
            const double x = w[-d];
#pragma unroll
            for (int p = 0; p < 3; ++p) z[p] = fma(a.h[p][d], x, z[p]);
        }
    } else {   // the window crosses the signal's edge: y = 0 outside it
#pragma unroll
        for (int d = 0; d < kTruePeakTaps; ++d) {
            const int64_t j = o + kTpBack - d;
            const double x = j >= g.off && j < g.off + g.n ? w[-d] : 0.0;
#pragma unroll
            for (int p = 0; p < 3; ++p) z[p] = fma(a.h[p][d], x, z[p]);
        }
    }
    a.t[o] = fmax(fabs(z[0]), fmax(fabs(z[1]), fabs(z[2])));
}

struct InitArgs {
    const double* ystats;   // [nsig][3] of the meter on y: L, TP, the scale-only G
    const double* ygain;    // [nsig] 10^(G / 20) of the meter
    int nsig;
    double target, ceiling, depth;
    LimState* st;
    double* unit;           // [nsig] <- 1.0
};

__global__ __launch_bounds__(kLanes) void k_lim_init(InitArgs a) {
    const int i = blockIdx.x * kLanes + threadIdx.x;
    if (i >= a.nsig) return;
    const double L = a.ystats[3 * i], tp = a.ystats[3 * i + 1];
    LimState st;
    st.G = a.ystats[3 * i + 2];
    st.g0 = a.ygain[i];
    st.Gcap = 0.0;
    st.idle = 1;
    if (isfinite(L)) {
        st.Gcap = a.ceiling - tp + a.depth;
        const double G0 = fmin(a.target - L, st.Gcap);
        if (!(G0 <= a.ceiling - tp)) {
            st.G = G0;
            st.g0 = pow(10.0, G0 / 20.0);
            st.idle = 0;
        }
    }
    a.st[i] = st;
    a.unit[i] = 1.0;
}

struct CurveArgs {
    const double* y;
    const double* t;
    const LimSig* sig;
    int nsig, K, first;   // first: evaluation 0 (an idle signal's x is written once)
    double c, hsum;    // the ceiling (linear); sum_k h[k] in the kernel's order
    const double* h;   // [K]
    const LimState* st;
    double* x;
    double* smin;      // [tiles]
    // a stream's window (k_lim_curve<true>): y and t hold win_n samples of ONE signal, tile b is the samples [lo + 1024 b, hi) of it, written
    // to x[1024 b ...]; the pre-gain is g0 and there is no idle rule
    int64_t win_n, lo, hi;
    double g0;
    double* xmax;      // [tiles] max |x| of the tile
};

__device__ __forceinline__ double ratio_at(const double* y, const double* t, int64_t p, double c, double g0) {   // r[p], 0 <= p < n
    const double e = lim_envelope_at(y, t, p);
    return e > 0.0 ? fmin(1.0, c / (g0 * e)) : 1.0;
}

template <bool kStream>
__global__ __launch_bounds__(kLanes) void k_lim_curve(CurveArgs a) {
    __shared__ double r[kLdsLen];
    __shared__ double red[kLanes / 64];
    __shared__ int active;
    const int t = threadIdx.x;
    const int si = kStream ? 0 : lim_find_tile(a.sig, a.nsig, blockIdx.x);
    const LimSig g = kStream ? LimSig{0, a.win_n, 0} : a.sig[si];
    const LimState st = kStream ? LimState{0.0, a.g0, 0.0, 0} : a.st[si];
    const int64_t n0 = kStream ? a.lo + (int64_t)blockIdx.x * kTile : ((int64_t)blockIdx.x - g.tile0) * kTile;
    const int cnt = (int)min((int64_t)kTile, (kStream ? a.hi : g.n) - n0);
    const double* y = a.y + g.off;   // indexed by the position in the signal
    const double* tt = a.t + g.off;
    double* x = kStream ? a.x - a.lo : a.x + g.off;
    if (st.idle) {   // the product of the scale-only path (k_pcm_gain_sig), so that its bytes come out
        if (!a.first) return;
        for (int u = t; u < cnt; u += kLanes) x[n0 + u] = y[n0 + u] * st.g0;
        if (t == 0) a.smin[blockIdx.x] = 1.0;
        return;
    }
    const int K = a.K, len = kTile + 2 * K - 2;
    if (t == 0) active = 0;
    __syncthreads();
    bool act = false;
    for (int i = t; i < len; i += kLanes) {   // r[i] at position n0 - (K - 1) + i
        const int64_t p = n0 - (K - 1) + i;
        const double v = p >= 0 && p < g.n ? ratio_at(y, tt, p, a.c, st.g0) : 1.0;
        r[i] = v;
        act |= v < 1.0;
    }
    if (act) active = 1;
    __syncthreads();
    double s[4];
    if (!active) {   // (workgroup-uniform) nothing to reduce within reach of this tile
        for (int q = 0; q < 4; ++q) s[q] = fmin(a.hsum, 1.0);
    } else {
        int w = 1;
        for (; 2 * w <= K; w *= 2) {   // r[i] <- min r[i .. i + 2 w - 1]
            double v[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int i = t + kLanes * q;
                if (i + w < len) v[q] = fmin(r[i], r[i + w]);
            }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int i = t + kLanes * q;
                if (i + w < len) r[i] = v[q];
            }
            __syncthreads();
        }
        {   // m[j] = min r[j .. j + K - 1] from two windows of w; m[0] before the signal's start
            const int mlen = kTile + K - 1;
            double v[6];
#pragma unroll
            for (int q = 0; q < 6; ++q) {
                const int j = t + kLanes * q;
                const int jj = n0 - (K - 1) + j < 0 ? (int)(K - 1 - n0) : j;   // before the start: m[0] (n0 = 0 there, but for a stream's tile)
                if (j < mlen) v[q] = fmin(r[jj], r[jj + K - w]);
            }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < 6; ++q) {
                const int j = t + kLanes * q;
                if (j < mlen) r[j] = v[q];
            }
            __syncthreads();
        }
        const double* mm = r + (K - 1) + t;   // mm[256 q - k] = m[n - k] of sample n = n0 + t + 256 q
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        for (int k = 0; k < K; ++k) {
            const double hk = a.h[k];
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q] = fma(hk, mm[kLanes * q - k], acc[q]);
        }
        for (int q = 0; q < 4; ++q) {
            const int u = t + kLanes * q;
            s[q] = u < cnt ? fmin(acc[q], ratio_at(y, tt, n0 + u, a.c, st.g0)) : 1.0;
        }
    }
    double mn = 1.0, mx = 0.0;
    for (int q = 0; q < 4; ++q) {
        const int u = t + kLanes * q;
        if (u < cnt) {
            const double v = fmin(fmax(y[n0 + u] * st.g0 * s[q], -a.c), a.c);
            x[n0 + u] = v;
            mn = fmin(mn, s[q]);
            if constexpr (kStream) mx = fmax(mx, fabs(v));
        }
    }
    for (int d = 32; d >= 1; d >>= 1) mn = fmin(mn, __shfl_xor(mn, d));
    if (t % 64 == 0) red[t / 64] = mn;
    __syncthreads();
    if (t == 0) a.smin[blockIdx.x] = fmin(fmin(red[0], red[1]), fmin(red[2], red[3]));
    if constexpr (kStream) {
        for (int d = 32; d >= 1; d >>= 1) mx = fmax(mx, __shfl_xor(mx, d));
        __syncthreads();
        if (t % 64 == 0) red[t / 64] = mx;
        __syncthreads();
        if (t == 0) a.xmax[blockIdx.x] = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
    }
}

struct UpdateArgs {
    const LimSig* sig;
    const double* ystats;   // [nsig][3] of y
    const double* xstats;   // [nsig][3] of x at the current G
    const double* smin;
    int last;
    double target;
    LimState* st;
    double* stats;          // [nsig][6]
};

__global__ __launch_bounds__(64) void k_lim_update(UpdateArgs a) {
    const int i = blockIdx.x, t = threadIdx.x;
    LimState st = a.st[i];
    const double Lx = a.xstats[3 * i];
    if (!a.last) {
        if (t == 0 && !st.idle && isfinite(Lx)) {
            st.G = fmin(st.G + a.target - Lx, st.Gcap);
            st.g0 = pow(10.0, st.G / 20.0);
            a.st[i] = st;
        }
        return;
    }
    const LimSig g = a.sig[i];
    const int64_t nt = (g.n + kTile - 1) / kTile;
    double mn = 1.0;
    for (int64_t k = t; k < nt; k += 64) mn = fmin(mn, a.smin[g.tile0 + k]);
    for (int d = 32; d >= 1; d >>= 1) mn = fmin(mn, __shfl_xor(mn, d));
    if (t == 0) {
        double* o = a.stats + 6 * i;
        o[0] = a.ystats[3 * i];
        o[1] = a.ystats[3 * i + 1];
        o[2] = st.G;
        o[3] = Lx;
        o[4] = a.xstats[3 * i + 1];
        o[5] = st.idle ? 0.0 : 20.0 * log10(mn);
    }
}

// ---- fixed gain ----

__global__ __launch_bounds__(kLanes) void k_lim_fixed_init(LimState* st, int nsig, double G, double g0) {
    const int i = blockIdx.x * kLanes + threadIdx.x;
    if (i < nsig) st[i] = LimState{G, g0, 0.0, 0};
}

// one workgroup per signal: stats[2 i] = 20 log10 min s over its tiles, stats[2 i + 1] = max |x| over its samples
__global__ __launch_bounds__(kLanes) void k_lim_fixed_stats(const LimSig* sig, const double* smin, const double* x, double* stats) {
    __shared__ double red[2][kLanes / 64];
    const int t = threadIdx.x;
    const LimSig g = sig[blockIdx.x];
    const int64_t nt = (g.n + kTile - 1) / kTile;
    double mn = 1.0, mx = 0.0;
    for (int64_t k = t; k < nt; k += kLanes) mn = fmin(mn, smin[g.tile0 + k]);
    for (int64_t k = t; k < g.n; k += kLanes) mx = fmax(mx, fabs(x[g.off + k]));
    for (int d = 32; d >= 1; d >>= 1) {
        mn = fmin(mn, __shfl_xor(mn, d));
        mx = fmax(mx, __shfl_xor(mx, d));
    }
    if (t % 64 == 0) red[0][t / 64] = mn, red[1][t / 64] = mx;
    __syncthreads();
    if (t == 0) {
        stats[2 * blockIdx.x] = 20.0 * log10(fmin(fmin(red[0][0], red[0][1]), fmin(red[0][2], red[0][3])));
        stats[2 * blockIdx.x + 1] = fmax(fmax(red[1][0], red[1][1]), fmax(red[1][2], red[1][3]));
    }
}

// run = {min s, max |x|} of a stream so far, then the unit gain the cast kernel multiplies by
__global__ void k_lim_stream_init(double* run) {
    run[0] = 1.0;
    run[1] = 0.0;
    run[2] = 1.0;
}

__global__ __launch_bounds__(64) void k_lim_stream_fold(const double* smin, const double* xmax, int tiles, double* run) {
    const int t = threadIdx.x;
    double mn = 1.0, mx = 0.0;
    for (int k = t; k < tiles; k += 64) {
        mn = fmin(mn, smin[k]);
        mx = fmax(mx, xmax[k]);
    }
    for (int d = 32; d >= 1; d >>= 1) {
        mn = fmin(mn, __shfl_xor(mn, d));
        mx = fmax(mx, __shfl_xor(mx, d));
    }
    if (t == 0) {
        run[0] = fmin(run[0], mn);
        run[1] = fmax(run[1], mx);
    }
}

}  // namespace

// sin^2(pi (k + 0.5) / K), scaled to sum to 1, into h[K]; returns their sum in the kernel's order
double limiter_hann_taps(int K, double* h) {
    double sum = 0.0, hsum = 0.0;
    for (int k = 0; k < K; ++k) {
        const double v = std::sin(M_PI * (k + 0.5) / K);
        h[k] = v * v;
        sum += h[k];
    }
    for (int k = 0; k < K; ++k) {
        h[k] /= sum;
        hsum += h[k];   // = fma(h[k], 1, acc): the kernel's sum over a window of ones
    }
    return hsum;
}

int limiter_window(int rate) {
    const int K = rate / 100;
    SBV2_REQUIRE(K >= 2 && K <= kMaxK, "internal: limiter window");
    return K;
}

void limiter_interp(const double* y, const LimSig* sig, int nsig, int64_t total, double* t, hipStream_t s) {
    if (total <= 0) return;
    InterpArgs a;
    a.y = y;
    a.sig = sig;
    a.nsig = nsig;
    a.total = total;
    loudness_true_peak_taps(a.h);
    a.t = t;
    hipLaunchKernelGGL(k_lim_interp<false>, dim3((unsigned)((total + kLanes - 1) / kLanes)), dim3(kLanes), 0, s, a);
}

LimiterSpec limiter_spec(const sbv2_limiter* lim) {
    SBV2_REQUIRE(lim, "no limiter given");
    SBV2_REQUIRE(std::isfinite(lim->target_lufs) && lim->target_lufs >= -70.0 && lim->target_lufs <= -5.0,
                 "loudness target " + std::to_string(lim->target_lufs) + " LUFS is outside [-70, -5]");
    SBV2_REQUIRE(std::isfinite(lim->true_peak_max_dbtp) && lim->true_peak_max_dbtp >= -20.0 && lim->true_peak_max_dbtp <= 0.0,
                 "true-peak ceiling " + std::to_string(lim->true_peak_max_dbtp) + " dBTP is outside [-20, 0]");
    SBV2_REQUIRE(std::isfinite(lim->max_reduction_db) && lim->max_reduction_db >= 0.0 && lim->max_reduction_db <= 12.0,
                 "limiter depth " + std::to_string(lim->max_reduction_db) + " dB is outside [0, 12]");
    SBV2_REQUIRE(lim->reserved == 0.0, "sbv2_limiter.reserved must be 0");
    LimiterSpec s;
    s.target = lim->target_lufs;
    s.ceiling = lim->true_peak_max_dbtp;
    s.depth = lim->max_reduction_db;
    return s;
}

namespace {

// What one run of the limiter over `sig` works on, shared by Limiter::run and Limiter::run_fixed so that the make-up path and the fixed-gain
// path (the yardstick of the streamed one) launch k_lim_interp and k_lim_curve on the same table, taps and layout.
struct LimWork {
    const double* y = nullptr;
    int nsig = 0, K = 0;
    int64_t tiles = 0, total = 0;
    double hsum = 0.0;
    const LimSig* sig = nullptr;
    LimState* st = nullptr;
    double *stats = nullptr, *unit = nullptr, *t = nullptr, *x = nullptr, *smin = nullptr, *stats_host = nullptr;
    const double* h = nullptr;
    const double* end = nullptr;   // behind the per-tile minima and their pad words

    Limiter::Parts parts() const { return Limiter::Parts{h, t, x, smin, end, total, tiles, K, hsum}; }
    void interp(hipStream_t s) const { limiter_interp(y, sig, nsig, total, t, s); }
    void curve(double ceiling_db, bool first, hipStream_t s) const {
        if (tiles <= 0) return;
        CurveArgs a{};
        a.y = y;
        a.t = t;
        a.sig = sig;
        a.nsig = nsig;
        a.K = K;
        a.first = first;
        a.c = std::pow(10.0, ceiling_db / 20.0);
        a.hsum = hsum;
        a.h = h;
        a.st = st;
        a.x = x;
        a.smin = smin;
        hipLaunchKernelGGL(k_lim_curve<false>, dim3((unsigned)tiles), dim3(kLanes), 0, s, a);
    }
};

// the signal table and the Hann taps on the device, every buffer of the run placed (grown on demand)
LimWork lim_setup(const double* y, const std::vector<FmtSignal>& sig, int rate, DeviceBuffer& dev, PinnedBuffer& host, hipStream_t s) {
    LimWork w;
    w.y = y;
    w.nsig = (int)sig.size();
    SBV2_REQUIRE(w.nsig >= 1, "internal: no signal to limit");
    w.K = limiter_window(rate);
    const int nsig = w.nsig;
    std::vector<LimSig> tab(nsig);
    for (int i = 0; i < nsig; ++i) {
        const int64_t n = sig[i].j1 - sig[i].j0;
        tab[i] = LimSig{sig[i].out_off, n, w.tiles};
        w.tiles += (n + kTile - 1) / kTile;
        w.total = std::max(w.total, sig[i].out_off + n);
    }
    SBV2_REQUIRE(w.total == 0 || y, "internal: no signal data");
    // device layout: table | states | stats | unit gains | Hann taps | t | x | per-tile minima (each part 64-byte aligned)
    const size_t tb = round_up64((int64_t)(sizeof(LimSig) * nsig), 64), sb = round_up64((int64_t)(sizeof(LimState) * nsig), 64),
                 stb = round_up64(48 * nsig, 64), ub = round_up64(8 * nsig, 64), hb = round_up64(8 * kMaxK, 64),
                 xb = round_up64(8 * std::max<int64_t>(w.total, 1), 64);
    const size_t o_st = tb, o_stats = o_st + sb, o_unit = o_stats + stb, o_h = o_unit + ub, o_t = o_h + hb, o_x = o_t + xb, o_smin = o_x + xb,
                 dbytes = o_smin + round_up64(8 * std::max<int64_t>(w.tiles, 1), 64);
    const size_t hbytes = tb + hb + stb;
    char* d = static_cast<char*>(dev.reserve(dbytes, dbytes * 2, s));
    char* h = static_cast<char*>(host.reserve(hbytes, std::max<size_t>(hbytes * 2, 8192), s));
    std::memcpy(h, tab.data(), sizeof(LimSig) * nsig);
    double* hann = reinterpret_cast<double*>(h + tb);   // sin^2(pi (k + 0.5) / K), scaled to sum to 1
    w.hsum = limiter_hann_taps(w.K, hann);
    w.stats_host = reinterpret_cast<double*>(h + tb + hb);
    HIP_CHECK(hipMemcpyAsync(d, h, sizeof(LimSig) * nsig, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(d + o_h, hann, sizeof(double) * w.K, hipMemcpyHostToDevice, s));
    w.sig = reinterpret_cast<const LimSig*>(d);
    w.st = reinterpret_cast<LimState*>(d + o_st);
    w.stats = reinterpret_cast<double*>(d + o_stats);
    w.unit = reinterpret_cast<double*>(d + o_unit);
    w.h = reinterpret_cast<const double*>(d + o_h);
    w.t = reinterpret_cast<double*>(d + o_t);
    w.x = reinterpret_cast<double*>(d + o_x);
    w.smin = reinterpret_cast<double*>(d + o_smin);
    w.end = reinterpret_cast<const double*>(d + dbytes);
    return w;
}

}  // namespace

const double* Limiter::run(const double* y, const std::vector<FmtSignal>& sig, int rate, const LimiterSpec& lim, LoudnessMeter& meter,
                           hipStream_t s, const double** unit) {
    SBV2_REQUIRE(!sig.empty(), "internal: no signal to limit");
    LoudnessSpec scale;
    scale.apply = true;
    scale.target = lim.target;
    scale.ceiling = lim.ceiling;
    const double* ygain = meter.measure(y, sig, rate, scale, s);   // refuses unsupported rates
    const LimWork w = lim_setup(y, sig, rate, dev_, host_, s);
    stats_host_ = w.stats_host;
    parts_ = w.parts();
    const double* ystats = meter.stats_dev();
    w.interp(s);
    {
        InitArgs a;
        a.ystats = ystats;
        a.ygain = ygain;
        a.nsig = w.nsig;
        a.target = lim.target;
        a.ceiling = lim.ceiling;
        a.depth = lim.depth;
        a.st = w.st;
        a.unit = w.unit;
        hipLaunchKernelGGL(k_lim_init, dim3((unsigned)((w.nsig + kLanes - 1) / kLanes)), dim3(kLanes), 0, s, a);
    }
    HIP_CHECK(hipGetLastError());
    const LoudnessSpec measure_only;
    for (int it = 0; it < 3; ++it) {
        w.curve(lim.ceiling, it == 0, s);
        xmeter_.measure(w.total > 0 ? w.x : nullptr, sig, rate, measure_only, s, it == 2);
        UpdateArgs u;
        u.sig = w.sig;
        u.ystats = ystats;
        u.xstats = xmeter_.stats_dev();
        u.smin = w.smin;
        u.last = it == 2;
        u.target = lim.target;
        u.st = w.st;
        u.stats = w.stats;
        hipLaunchKernelGGL(k_lim_update, dim3(w.nsig), dim3(64), 0, s, u);
        HIP_CHECK(hipGetLastError());
    }
    HIP_CHECK(hipMemcpyAsync(stats_host_, w.stats, 48 * (size_t)w.nsig, hipMemcpyDeviceToHost, s));
    *unit = w.unit;
    return w.total > 0 ? w.x : y;
}

StreamLevelSpec stream_level_spec(const sbv2_stream_level* lv) {
    SBV2_REQUIRE(lv, "no stream level given");
    SBV2_REQUIRE(std::isfinite(lv->gain_db) && lv->gain_db >= -40.0 && lv->gain_db <= 40.0,
                 "stream gain " + std::to_string(lv->gain_db) + " dB is outside [-40, 40]");
    SBV2_REQUIRE(std::isfinite(lv->true_peak_max_dbtp) && lv->true_peak_max_dbtp >= -20.0 && lv->true_peak_max_dbtp <= 0.0,
                 "true-peak ceiling " + std::to_string(lv->true_peak_max_dbtp) + " dBTP is outside [-20, 0]");
    SBV2_REQUIRE(lv->reserved[0] == 0.0 && lv->reserved[1] == 0.0, "sbv2_stream_level.reserved must be 0");
    StreamLevelSpec s;
    s.gain_db = lv->gain_db;
    s.ceiling = lv->true_peak_max_dbtp;
    return s;
}

// The interpolator's window of t[o] is y[o - 11, o + 12] (kTpBack; k_lim_interp stages [base - 11, base + 268) for 256 samples: 11 back,
// 12 ahead), and s[n] needs r, hence t, up to n + K - 1: y up to n + K - 1 + 12.
int64_t stream_level_lookahead(int rate) { return limiter_window(rate) - 1 + kTpBack; }

const double* Limiter::run_fixed(const double* y, const std::vector<FmtSignal>& sig, int rate, const StreamLevelSpec& lv, hipStream_t s) {
    const LimWork w = lim_setup(y, sig, rate, dev_, host_, s);
    stats_host_ = w.stats_host;
    parts_ = w.parts();
    hipLaunchKernelGGL(k_lim_fixed_init, dim3((unsigned)((w.nsig + kLanes - 1) / kLanes)), dim3(kLanes), 0, s, w.st, w.nsig, lv.gain_db,
                       std::pow(10.0, lv.gain_db / 20.0));
    w.interp(s);
    w.curve(lv.ceiling, true, s);
    hipLaunchKernelGGL(k_lim_fixed_stats, dim3(w.nsig), dim3(kLanes), 0, s, w.sig, w.smin, w.x, w.stats);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(stats_host_, w.stats, 16 * (size_t)w.nsig, hipMemcpyDeviceToHost, s));
    return w.total > 0 ? w.x : y;
}

// ---- the fixed-gain limiter fed piece by piece ----
//
// Two y buffers of 2 A + max_push doubles: a push's window is [carried y | new y] in the current one (the caller writes the new samples at
// dst()); afterwards the samples from A before the first one not yet emitted to the end (at most 2 A: O(K), whatever the utterance's
// length) go to the front of the OTHER buffer with one device-to-device copy, so source and destination never overlap however short the
// push was, and the buffers swap.  Which samples a push emits follows from the counts alone: nothing here waits for the GPU after begin.

void StreamLimiter::begin(int rate, int64_t total_samples, int64_t max_push, const StreamLevelSpec& lv, hipStream_t s) {
    K_ = limiter_window(rate);
    A_ = stream_level_lookahead(rate);
    SBV2_REQUIRE(total_samples >= 0 && max_push >= 0, "stream level: length out of range");
    total_ = total_samples;
    max_push_ = max_push;
    fed_ = emitted_ = pos0_ = tail_ = 0;
    cur_ = 0;
    done_ = false;
    g0_ = std::pow(10.0, lv.gain_db / 20.0);
    c_ = std::pow(10.0, lv.ceiling / 20.0);
    const size_t win = sizeof(double) * (size_t)(2 * A_ + max_push), tiles = (size_t)((max_push + A_ + kTile - 1) / kTile + 1);
    for (DeviceBuffer& b : buf_) b.reserve(win, s);
    t_.reserve(win, s);
    x_.reserve(sizeof(double) * (size_t)(max_push + A_ + 1), s);
    // [running min s, max |x|, the unit gain | Hann taps | per-tile min s | per-tile max |x|]
    aux_.reserve(64 + 8 * kMaxK + 16 * tiles, s);
    double* hann = static_cast<double*>(host_.reserve(8 * kMaxK + 64, s));
    hsum_ = limiter_hann_taps(K_, hann);
    HIP_CHECK(hipMemcpyAsync(aux_.as<char>() + 64, hann, sizeof(double) * K_, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_lim_stream_init, dim3(1), dim3(1), 0, s, aux_.as<double>());
    HIP_CHECK(hipGetLastError());
}

double* StreamLimiter::dst() const { return buf_[cur_].as<double>() + tail_; }
double* StreamLimiter::out_buffer() const { return x_.as<double>(); }
const double* StreamLimiter::unit() const { return aux_.as<double>() + 2; }

int64_t StreamLimiter::emitted_after(int64_t fed, bool last) const { return last ? total_ : std::max<int64_t>(0, fed - A_); }

int64_t StreamLimiter::push(int64_t n, bool last, double* out, hipStream_t s) {
    SBV2_REQUIRE(K_ > 0 && !done_, "stream level: push without begin, or after the last push");
    SBV2_REQUIRE(n >= 0 && n <= max_push_ && fed_ + n <= total_, "stream level: push of " + std::to_string(n) + " samples outgrows what begin announced");
    SBV2_REQUIRE(!last || fed_ + n == total_, "stream level: the last push ends " + std::to_string(total_ - fed_ - n) + " samples short of the announced length");
    const int64_t have = tail_ + n, fed = fed_ + n;   // the window holds samples [pos0_, fed) of the stream
    const int64_t upto = emitted_after(fed, last), cnt = upto - emitted_;
    double* y = buf_[cur_].as<double>();
    double* aux = aux_.as<double>();
    if (cnt > 0) {
        SBV2_REQUIRE(out, "stream level: no output buffer");
        const int tiles = (int)((cnt + kTile - 1) / kTile);
        double* smin = aux + 8 + kMaxK;
        double* xmax = smin + (max_push_ + A_ + kTile - 1) / kTile + 1;
        InterpArgs ia;
        ia.y = y;
        ia.sig = nullptr;
        ia.nsig = 1;
        ia.total = have;
        loudness_true_peak_taps(ia.h);
        ia.t = t_.as<double>();
        hipLaunchKernelGGL(k_lim_interp<true>, dim3((unsigned)((have + kLanes - 1) / kLanes)), dim3(kLanes), 0, s, ia);
        CurveArgs a{};
        a.y = y;
        a.t = t_.as<double>();
        a.nsig = 1;
        a.K = K_;
        a.first = 1;
        a.c = c_;
        a.hsum = hsum_;
        a.h = aux + 8;
        a.x = out;
        a.smin = smin;
        a.win_n = have;
        a.lo = emitted_ - pos0_;
        a.hi = upto - pos0_;
        a.g0 = g0_;
        a.xmax = xmax;
        hipLaunchKernelGGL(k_lim_curve<true>, dim3((unsigned)tiles), dim3(kLanes), 0, s, a);
        hipLaunchKernelGGL(k_lim_stream_fold, dim3(1), dim3(64), 0, s, smin, xmax, tiles, aux);
        HIP_CHECK(hipGetLastError());
    }
    if (last) {
        HIP_CHECK(hipMemcpyAsync(host_.as<double>() + kMaxK, aux, 16, hipMemcpyDeviceToHost, s));   // behind the taps' host copy
        tail_ = 0;
    } else {
        const int64_t p1 = std::max<int64_t>(0, upto - A_), rest = fed - p1;   // (p1 >= pos0_: upto never moves back)
        if (p1 != pos0_) {
            if (rest) HIP_CHECK(hipMemcpyAsync(buf_[cur_ ^ 1].get(), y + (p1 - pos0_), sizeof(double) * (size_t)rest, hipMemcpyDeviceToDevice, s));
            cur_ ^= 1;
        }
        pos0_ = p1;
        tail_ = rest;
    }
    fed_ = fed;
    emitted_ = upto;
    done_ = last;
    return cnt;
}

void StreamLimiter::stats(double* out) const {
    SBV2_REQUIRE(done_, "stream level: the stats exist once the last push has been made");
    const double* h = host_.as<double>() + kMaxK;
    out[0] = 20.0 * std::log10(h[0]);
    out[1] = h[1];
}

}  // namespace sbv2
