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
constexpr int kLdsLen = kTile + 2 * kMaxK - 2;   // r of a tile and its halo
constexpr int kTpBack = 12;                       // the interpolator's window is y[o - 11, o + 12] (loudness.hip)
static_assert(kLdsLen <= 8 * kLanes && kTile + kMaxK - 1 <= 6 * kLanes && kTile == 4 * kLanes, "k_lim_curve's per-lane counts");

struct LimSig {
    int64_t off, n, tile0;   // samples y[off, off + n); its tiles are [tile0, tile0 + ceil(n / kTile))
};

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

__device__ __forceinline__ int find_tile(const LimSig* sig, int nsig, int64_t k) {   // last signal with tile0 <= k
    int lo = 0, hi = nsig - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (sig[mid].tile0 <= k) lo = mid;
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
    const LimSig g = a.sig[find_off(a.sig, a.nsig, o)];
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
};

__device__ __forceinline__ double ratio_at(const double* y, const double* t, int64_t p, double c, double g0) {   // r[p], 0 <= p < n
    const double e = fmax(fmax(p > 0 ? t[p - 1] : 0.0, fabs(y[p])), t[p]);
    return e > 0.0 ? fmin(1.0, c / (g0 * e)) : 1.0;
}

__global__ __launch_bounds__(kLanes) void k_lim_curve(CurveArgs a) {
    __shared__ double r[kLdsLen];
    __shared__ double red[kLanes / 64];
    __shared__ int active;
    const int t = threadIdx.x;
    const int si = find_tile(a.sig, a.nsig, blockIdx.x);
    const LimSig g = a.sig[si];
    const LimState st = a.st[si];
    const int64_t n0 = ((int64_t)blockIdx.x - g.tile0) * kTile;
    const int cnt = (int)min((int64_t)kTile, g.n - n0);
    const double* y = a.y + g.off;   // indexed by the position in the signal
    const double* tt = a.t + g.off;
    double* x = a.x + g.off;
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
                const int jj = n0 - (K - 1) + j < 0 ? K - 1 : j;   // before the start (first tile only): m[0]
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
    double mn = 1.0;
    for (int q = 0; q < 4; ++q) {
        const int u = t + kLanes * q;
        if (u < cnt) {
            x[n0 + u] = fmin(fmax(y[n0 + u] * st.g0 * s[q], -a.c), a.c);
            mn = fmin(mn, s[q]);
        }
    }
    for (int d = 32; d >= 1; d >>= 1) mn = fmin(mn, __shfl_xor(mn, d));
    if (t % 64 == 0) red[t / 64] = mn;
    __syncthreads();
    if (t == 0) a.smin[blockIdx.x] = fmin(fmin(red[0], red[1]), fmin(red[2], red[3]));
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

}  // namespace

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

const double* Limiter::run(const double* y, const std::vector<FmtSignal>& sig, int rate, const LimiterSpec& lim, LoudnessMeter& meter,
                           hipStream_t s, const double** unit) {
    const int nsig = (int)sig.size();
    SBV2_REQUIRE(nsig >= 1, "internal: no signal to limit");
    LoudnessSpec scale;
    scale.apply = true;
    scale.target = lim.target;
    scale.ceiling = lim.ceiling;
    const double* ygain = meter.measure(y, sig, rate, scale, s);   // refuses unsupported rates
    const int K = rate / 100;
    SBV2_REQUIRE(K >= 2 && K <= kMaxK, "internal: limiter window");
    std::vector<LimSig> tab(nsig);
    int64_t tiles = 0, total = 0;
    for (int i = 0; i < nsig; ++i) {
        const int64_t n = sig[i].j1 - sig[i].j0;
        tab[i] = LimSig{sig[i].out_off, n, tiles};
        tiles += (n + kTile - 1) / kTile;
        total = std::max(total, sig[i].out_off + n);
    }
    SBV2_REQUIRE(total == 0 || y, "internal: no signal data");
    // device layout: table | states | stats | unit gains | Hann taps | t | x | per-tile minima (each part 64-byte aligned)
    const size_t tb = round_up64((int64_t)(sizeof(LimSig) * nsig), 64), sb = round_up64((int64_t)(sizeof(LimState) * nsig), 64),
                 stb = round_up64(48 * nsig, 64), ub = round_up64(8 * nsig, 64), hb = round_up64(8 * kMaxK, 64),
                 xb = round_up64(8 * std::max<int64_t>(total, 1), 64);
    const size_t o_st = tb, o_stats = o_st + sb, o_unit = o_stats + stb, o_h = o_unit + ub, o_t = o_h + hb, o_x = o_t + xb, o_smin = o_x + xb,
                 dbytes = o_smin + round_up64(8 * std::max<int64_t>(tiles, 1), 64);
    const size_t hbytes = tb + hb + stb;
    char* d = static_cast<char*>(dev_.reserve(dbytes, dbytes * 2, s));
    char* h = static_cast<char*>(host_.reserve(hbytes, std::max<size_t>(hbytes * 2, 8192), s));
    std::memcpy(h, tab.data(), sizeof(LimSig) * nsig);
    double* hann = reinterpret_cast<double*>(h + tb);   // sin^2(pi (k + 0.5) / K), scaled to sum to 1
    double sum = 0.0, hsum = 0.0;
    for (int k = 0; k < K; ++k) {
        const double v = std::sin(M_PI * (k + 0.5) / K);
        hann[k] = v * v;
        sum += hann[k];
    }
    for (int k = 0; k < K; ++k) {
        hann[k] /= sum;
        hsum += hann[k];   // = fma(h[k], 1, acc): the kernel's sum over a window of ones
    }
    stats_host_ = reinterpret_cast<double*>(h + tb + hb);
    HIP_CHECK(hipMemcpyAsync(d, h, sizeof(LimSig) * nsig, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(d + o_h, hann, sizeof(double) * K, hipMemcpyHostToDevice, s));
    const LimSig* sig_dev = reinterpret_cast<const LimSig*>(d);
    auto* st = reinterpret_cast<LimState*>(d + o_st);
    auto* stats = reinterpret_cast<double*>(d + o_stats);
    auto* unit_dev = reinterpret_cast<double*>(d + o_unit);
    auto* x = reinterpret_cast<double*>(d + o_x);
    const double* ystats = meter.stats_dev();
    if (total > 0) {
        InterpArgs a;
        a.y = y;
        a.sig = sig_dev;
        a.nsig = nsig;
        a.total = total;
        loudness_true_peak_taps(a.h);
        a.t = reinterpret_cast<double*>(d + o_t);
        hipLaunchKernelGGL(k_lim_interp, dim3((unsigned)((total + kLanes - 1) / kLanes)), dim3(kLanes), 0, s, a);
    }
    {
        InitArgs a;
        a.ystats = ystats;
        a.ygain = ygain;
        a.nsig = nsig;
        a.target = lim.target;
        a.ceiling = lim.ceiling;
        a.depth = lim.depth;
        a.st = st;
        a.unit = unit_dev;
        hipLaunchKernelGGL(k_lim_init, dim3((unsigned)((nsig + kLanes - 1) / kLanes)), dim3(kLanes), 0, s, a);
    }
    HIP_CHECK(hipGetLastError());
    const LoudnessSpec measure_only;
    for (int it = 0; it < 3; ++it) {
        if (tiles > 0) {
            CurveArgs a;
            a.y = y;
            a.t = reinterpret_cast<const double*>(d + o_t);
            a.sig = sig_dev;
            a.nsig = nsig;
            a.K = K;
            a.first = it == 0;
            a.c = std::pow(10.0, lim.ceiling / 20.0);
            a.hsum = hsum;
            a.h = reinterpret_cast<const double*>(d + o_h);
            a.st = st;
            a.x = x;
            a.smin = reinterpret_cast<double*>(d + o_smin);
            hipLaunchKernelGGL(k_lim_curve, dim3((unsigned)tiles), dim3(kLanes), 0, s, a);
        }
        xmeter_.measure(total > 0 ? x : nullptr, sig, rate, measure_only, s, it == 2);
        UpdateArgs u;
        u.sig = sig_dev;
        u.ystats = ystats;
        u.xstats = xmeter_.stats_dev();
        u.smin = reinterpret_cast<const double*>(d + o_smin);
        u.last = it == 2;
        u.target = lim.target;
        u.st = st;
        u.stats = stats;
        hipLaunchKernelGGL(k_lim_update, dim3(nsig), dim3(64), 0, s, u);
        HIP_CHECK(hipGetLastError());
    }
    HIP_CHECK(hipMemcpyAsync(stats_host_, stats, 48 * (size_t)nsig, hipMemcpyDeviceToHost, s));
    *unit = unit_dev;
    return total > 0 ? x : y;
}

}  // namespace sbv2
