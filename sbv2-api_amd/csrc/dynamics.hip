// Speech compressor on the device: evens out the level differences between syllables and between the sentences of a joined request, so that
// the look-ahead limiter behind it (limiter.hip) is left with the crest only.  All of it in f64 on y (the resampled signal before any gain);
// its output yc takes y's place in front of the meter, the loudness gain, the limiter, the cast and the quantisers.
//
// Convention (struct sbv2_dynamics in include/sbv2_hip.h; tests/test_dynamics.py restates it in numpy): L = the integrated loudness of y,
//   T = L + threshold_lu, k = 1 - 1 / ratio, e[n] = the envelope of sbv2_limiter step 1;
//   d[n] = k (20 log10 e[n] - T) where e[n] > 0 and that is > 0, else 0; dq[n] = llrint(65536 d[n]) (int64, 1 / 65536 dB);
//   rho = max(1, llrint(65536 release / fs)), alpha = max(1, llrint(65536 attack / fs));
//   p[n] = max_{i <= n} (dq[i] - rho (n - i)) = prefixmax(dq[i] + rho i)[n] - rho n        (hold, then a release linear in dB);
//   a[n] = max_{i >= n} (dq[i] - alpha (i - n)) = suffixmax(dq[i] - alpha i)[n] + alpha n   (the attack ramp ahead of a peak);
//   u[n] = max(p[n], a[n]); ut[n] = sum_{k < K} h[k] double(u[clamp(n + c0 - k, 0, N - 1)]) / 65536 in ascending k, K = fs / 100, h the
//   limiter's window, c0 = K - 1 - K / 2; s[n] = 10^(-ut[n] / 20); yc[n] = y[n] s[n].
//   A signal with L = -inf (or ratio = 1) is idle: d = 0 throughout, hence u = 0, ut = 0, s = 1 and yc = y bit for bit.
//   The maxima are exact and order-free; the one sum has a fixed order and is never contracted (this file is built with contraction off).
//
// Kernel design.  A fixed number of launches, whatever the number and the lengths of the signals; no atomics, no host round trip.
//   limiter_interp  (limiter.hip) t[n], from which e[n] = lim_envelope_at(y, t, n) is formed where it is read: the limiter's own code.
//   k_dyn_detect    one workgroup per tile of 1024 samples of ONE signal (the limiter's table: tiles never straddle a signal edge): dq to
//                   HBM, and the tile's maxima of the two keys dq[i] + rho i and dq[i] - alpha i.  L is read from the meter's device stats.
//   k_dyn_carry     one wave per signal: the exclusive prefix maximum of the first key and the exclusive suffix maximum of the second over
//                   the signal's tiles, 64 tiles per step with a running carry.
//   k_dyn_scan      one workgroup per tile: each lane scans its 4 consecutive samples, the wave scans the lanes' totals by shuffles, LDS joins
//                   the 4 waves, the carries seed the tile; u to HBM.
//   k_dyn_apply     one workgroup per tile: u of the tile and a halo of K - 1 samples (clamped to the signal) as doubles in LDS, the K-tap
//                   sum in ascending k for every sample (4 samples per lane, taps read uniformly; a tile with u = 0 within reach skips
//                   the loop: the sum over zeros is 0), 10^x, the multiply, and the tile's max ut.
//   k_dyn_stats     one wave per signal: L, T and -max ut over the signal's tiles.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>

#include "../../include/sbv2_hip.h"
#include "dynamics.h"

namespace sbv2 {

namespace {

constexpr int kTile = Dynamics::kTile;
constexpr int kLanes = 256;
constexpr int kPer = kTile / kLanes;
constexpr int kLdsLen = kTile + kLimMaxK - 1;   // u of a tile and its halo
constexpr long long kNoKey = LLONG_MIN;          // takes part in maxima only, never in arithmetic
static_assert(kPer == 4 && kLanes % 64 == 0, "k_dyn_scan's per-lane counts");

struct DynArgs {
    const double* y;
    const double* t;
    const LimSig* sig;
    int nsig, K;
    const double* ystats;   // [nsig][3] of the meter on y: L first
    double thr, k;          // threshold_lu, 1 - 1 / ratio
    long long rho, alpha;
    const double* h;        // [K]
    long long *dq, *u;      // [total]
    long long *keyf, *keyb, *carf, *carb;   // [tiles]
    double* utmax;          // [tiles]
    double *yc, *e_out, *s_out;   // [total]; the last two may be null
    double* stats;          // [nsig][3]
};

__device__ __forceinline__ long long max64(long long a, long long b) { return a > b ? a : b; }

// the maximum over the workgroup's 256 lanes, returned to every lane
__device__ __forceinline__ long long block_max(long long v, long long* red) {
    for (int d = 32; d >= 1; d >>= 1) v = max64(v, __shfl_xor(v, d));
    __syncthreads();   // (red may still be read from an earlier call)
    if (threadIdx.x % 64 == 0) red[threadIdx.x / 64] = v;
    __syncthreads();
    return max64(max64(red[0], red[1]), max64(red[2], red[3]));
}

__global__ __launch_bounds__(kLanes) void k_dyn_detect(DynArgs a) {
    __shared__ long long red[kLanes / 64];
    const int t = threadIdx.x;
    const int si = lim_find_tile(a.sig, a.nsig, blockIdx.x);
    const LimSig g = a.sig[si];
    const int64_t n0 = ((int64_t)blockIdx.x - g.tile0) * kTile;
    const int cnt = (int)min((int64_t)kTile, g.n - n0);
    const double L = a.ystats[3 * si];
    const bool idle = !isfinite(L) || a.k == 0.0;
    const double T = L + a.thr;
    const double* y = a.y + g.off;   // indexed by the position in the signal
    const double* tt = a.t + g.off;
    long long kf = kNoKey, kb = kNoKey;
    for (int q = 0; q < kPer; ++q) {
        const int j = t + kLanes * q;
        if (j >= cnt) continue;
        const int64_t p = n0 + j;
        const double e = lim_envelope_at(y, tt, p);
        double d = !idle && e > 0.0 ? a.k * (20.0 * log10(e) - T) : 0.0;
        d = d > 0.0 ? fmin(d, 8192.0) : 0.0;   // (a finite e stays below 6300 dB: the cap holds an infinite one inside int64)
        const long long dq = llrint(d * 65536.0);
        a.dq[g.off + p] = dq;
        if (a.e_out) a.e_out[g.off + p] = e;
        kf = max64(kf, dq + a.rho * p);
        kb = max64(kb, dq - a.alpha * p);
    }
    kf = block_max(kf, red);
    kb = block_max(kb, red);
    if (t == 0) {
        a.keyf[blockIdx.x] = kf;
        a.keyb[blockIdx.x] = kb;
    }
}

// inclusive maximum over the lanes at or below this one (up) / at or above it (down)
__device__ __forceinline__ long long wave_scan_up(long long v, int lane) {
    for (int d = 1; d < 64; d *= 2) {
        const long long o = __shfl_up(v, d);
        if (lane >= d) v = max64(v, o);
    }
    return v;
}
__device__ __forceinline__ long long wave_scan_down(long long v, int lane) {
    for (int d = 1; d < 64; d *= 2) {
        const long long o = __shfl_down(v, d);
        if (lane + d < 64) v = max64(v, o);
    }
    return v;
}

__global__ __launch_bounds__(64) void k_dyn_carry(DynArgs a) {
    const int lane = threadIdx.x;
    const LimSig g = a.sig[blockIdx.x];
    const int64_t nt = (g.n + kTile - 1) / kTile;
    long long run = kNoKey;
    for (int64_t base = 0; base < nt; base += 64) {   // forward: carf[b] = max keyf[tiles of the signal before b]
        const int64_t i = base + lane;
        const long long v = wave_scan_up(i < nt ? a.keyf[g.tile0 + i] : kNoKey, lane);
        const long long before = __shfl_up(v, 1);
        if (i < nt) a.carf[g.tile0 + i] = max64(run, lane > 0 ? before : kNoKey);
        run = max64(run, __shfl(v, 63));
    }
    run = kNoKey;
    for (int64_t base = 0; base < nt; base += 64) {   // backward, from the signal's last tile: carb[b] = max keyb[tiles after b]
        const int64_t i = nt - 1 - (base + lane);
        const long long v = wave_scan_up(i >= 0 ? a.keyb[g.tile0 + i] : kNoKey, lane);
        const long long before = __shfl_up(v, 1);
        if (i >= 0) a.carb[g.tile0 + i] = max64(run, lane > 0 ? before : kNoKey);
        run = max64(run, __shfl(v, 63));
    }
}

__global__ __launch_bounds__(kLanes) void k_dyn_scan(DynArgs a) {
    __shared__ long long wf[kLanes / 64], wb[kLanes / 64];
    const int t = threadIdx.x, lane = t % 64, wave = t / 64;
    const int si = lim_find_tile(a.sig, a.nsig, blockIdx.x);
    const LimSig g = a.sig[si];
    const int64_t n0 = ((int64_t)blockIdx.x - g.tile0) * kTile;
    const int cnt = (int)min((int64_t)kTile, g.n - n0);
    const long long* dq = a.dq + g.off + n0;
    long long f[kPer], b[kPer];   // the keys of samples n0 + 4 t + j
    for (int j = 0; j < kPer; ++j) {
        const int i = kPer * t + j;
        const bool in = i < cnt;
        const long long v = in ? dq[i] : 0;
        f[j] = in ? v + a.rho * (n0 + i) : kNoKey;
        b[j] = in ? v - a.alpha * (n0 + i) : kNoKey;
    }
    for (int j = 1; j < kPer; ++j) f[j] = max64(f[j], f[j - 1]);
    for (int j = kPer - 2; j >= 0; --j) b[j] = max64(b[j], b[j + 1]);
    const long long fi = wave_scan_up(f[kPer - 1], lane), bi = wave_scan_down(b[0], lane);
    if (lane == 63) wf[wave] = fi;
    if (lane == 0) wb[wave] = bi;
    const long long fprev = __shfl_up(fi, 1), bnext = __shfl_down(bi, 1);
    __syncthreads();
    long long sf = max64(a.carf[blockIdx.x], lane > 0 ? fprev : kNoKey), sb = max64(a.carb[blockIdx.x], lane < 63 ? bnext : kNoKey);
    for (int w = 0; w < kLanes / 64; ++w) {
        if (w < wave) sf = max64(sf, wf[w]);
        if (w > wave) sb = max64(sb, wb[w]);
    }
    for (int j = 0; j < kPer; ++j) {
        const int i = kPer * t + j;
        if (i >= cnt) break;
        const long long p = max64(f[j], sf) - a.rho * (n0 + i), at = max64(b[j], sb) + a.alpha * (n0 + i);
        a.u[g.off + n0 + i] = max64(p, at);
    }
}

__global__ __launch_bounds__(kLanes) void k_dyn_apply(DynArgs a) {
    __shared__ double w[kLdsLen];
    __shared__ double red[kLanes / 64];
    __shared__ int active;
    const int t = threadIdx.x;
    const int si = lim_find_tile(a.sig, a.nsig, blockIdx.x);
    const LimSig g = a.sig[si];
    const int64_t n0 = ((int64_t)blockIdx.x - g.tile0) * kTile;
    const int cnt = (int)min((int64_t)kTile, g.n - n0);
    const int K = a.K, len = kTile + K - 1;
    const long long* u = a.u + g.off;   // indexed by the position in the signal
    if (t == 0) active = 0;
    __syncthreads();
    bool act = false;
    for (int i = t; i < len; i += kLanes) {   // w[i] = u at position n0 - K / 2 + i, clamped to the signal
        const int64_t p = min(max(n0 - K / 2 + i, (int64_t)0), g.n - 1);
        const double v = (double)u[p] / 65536.0;
        w[i] = v;
        act |= v != 0.0;
    }
    if (act) active = 1;
    __syncthreads();
    double acc[kPer] = {0.0, 0.0, 0.0, 0.0};
    if (active) {   // (workgroup-uniform)
        const double* mm = w + (K - 1) + t;   // mm[256 q - k] = u[n + c0 - k] of sample n = n0 + t + 256 q
        for (int k = 0; k < K; ++k) {
            const double hk = a.h[k];
#pragma unroll
            for (int q = 0; q < kPer; ++q) acc[q] = acc[q] + hk * mm[kLanes * q - k];
        }
    }
    double mx = 0.0;
    for (int q = 0; q < kPer; ++q) {
        const int j = t + kLanes * q;
        if (j >= cnt) continue;
        const int64_t o = g.off + n0 + j;
        const double ut = acc[q];
        const double s = ut == 0.0 ? 1.0 : fmin(pow(10.0, -ut / 20.0), 1.0);
        a.yc[o] = a.y[o] * s;
        if (a.s_out) a.s_out[o] = s;
        mx = fmax(mx, ut);
    }
    for (int d = 32; d >= 1; d >>= 1) mx = fmax(mx, __shfl_xor(mx, d));
    if (t % 64 == 0) red[t / 64] = mx;
    __syncthreads();
    if (t == 0) a.utmax[blockIdx.x] = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
}

__global__ __launch_bounds__(64) void k_dyn_stats(DynArgs a) {
    const int i = blockIdx.x, t = threadIdx.x;
    const LimSig g = a.sig[i];
    const int64_t nt = (g.n + kTile - 1) / kTile;
    double mx = 0.0;
    for (int64_t k = t; k < nt; k += 64) mx = fmax(mx, a.utmax[g.tile0 + k]);
    for (int d = 32; d >= 1; d >>= 1) mx = fmax(mx, __shfl_xor(mx, d));
    if (t == 0) {
        const double L = a.ystats[3 * i];
        double* o = a.stats + 3 * i;
        o[0] = L;
        o[1] = L + a.thr;
        o[2] = mx > 0.0 ? -mx : 0.0;
    }
}

}  // namespace

DynamicsSpec dynamics_spec(const sbv2_dynamics* d) {
    SBV2_REQUIRE(d, "no dynamics given");
    SBV2_REQUIRE(std::isfinite(d->threshold_lu) && d->threshold_lu >= 0.0 && d->threshold_lu <= 30.0,
                 "compressor threshold " + std::to_string(d->threshold_lu) + " LU is outside [0, 30]");
    SBV2_REQUIRE(std::isfinite(d->ratio) && d->ratio >= 1.0 && d->ratio <= 20.0,
                 "compressor ratio " + std::to_string(d->ratio) + " is outside [1, 20]");
    SBV2_REQUIRE(std::isfinite(d->attack_db_per_s) && d->attack_db_per_s >= 10.0 && d->attack_db_per_s <= 10000.0,
                 "compressor attack " + std::to_string(d->attack_db_per_s) + " dB/s is outside [10, 10000]");
    SBV2_REQUIRE(std::isfinite(d->release_db_per_s) && d->release_db_per_s >= 1.0 && d->release_db_per_s <= 1000.0,
                 "compressor release " + std::to_string(d->release_db_per_s) + " dB/s is outside [1, 1000]");
    SBV2_REQUIRE(d->reserved == 0.0, "sbv2_dynamics.reserved must be 0");
    DynamicsSpec s;
    s.threshold = d->threshold_lu;
    s.ratio = d->ratio;
    s.attack = d->attack_db_per_s;
    s.release = d->release_db_per_s;
    return s;
}

const double* Dynamics::run(const double* y, const std::vector<FmtSignal>& sig, int rate, const DynamicsSpec& d, LoudnessMeter& meter,
                            hipStream_t s, bool keep_parts) {
    const int nsig = (int)sig.size();
    SBV2_REQUIRE(nsig >= 1, "internal: no signal to compress");
    const LoudnessSpec measure_only;
    meter.measure(y, sig, rate, measure_only, s, false);   // refuses unsupported rates
    const int K = limiter_window(rate);
    std::vector<LimSig> tab(nsig);
    int64_t tiles = 0, total = 0;
    for (int i = 0; i < nsig; ++i) {
        const int64_t n = sig[i].j1 - sig[i].j0;
        tab[i] = LimSig{sig[i].out_off, n, tiles};
        tiles += (n + kTile - 1) / kTile;
        total = std::max(total, sig[i].out_off + n);
    }
    SBV2_REQUIRE(total == 0 || y, "internal: no signal data");
    // device layout: table | stats | Hann taps | 4 per-tile key arrays | per-tile max ut | t | dq | u | yc [| e | s] (each part 64-byte aligned)
    const size_t tb = round_up64((int64_t)(sizeof(LimSig) * nsig), 64), stb = round_up64(24 * nsig, 64), hb = round_up64(8 * kLimMaxK, 64),
                 kb = round_up64(8 * std::max<int64_t>(tiles, 1), 64), xb = round_up64(8 * std::max<int64_t>(total, 1), 64);
    const size_t o_stats = tb, o_h = o_stats + stb, o_key = o_h + hb, o_ut = o_key + 4 * kb, o_t = o_ut + kb, o_dq = o_t + xb, o_u = o_dq + xb,
                 o_yc = o_u + xb, o_e = o_yc + xb, o_s = o_e + xb, dbytes = keep_parts ? o_s + xb : o_e;
    const size_t hbytes = tb + hb + stb;
    char* dv = static_cast<char*>(dev_.reserve(dbytes, dbytes * 2, s));
    char* h = static_cast<char*>(host_.reserve(hbytes, std::max<size_t>(hbytes * 2, 8192), s));
    std::memcpy(h, tab.data(), sizeof(LimSig) * nsig);
    double* hann = reinterpret_cast<double*>(h + tb);
    limiter_hann_taps(K, hann);
    stats_host_ = reinterpret_cast<double*>(h + tb + hb);
    HIP_CHECK(hipMemcpyAsync(dv, h, sizeof(LimSig) * nsig, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(dv + o_h, hann, sizeof(double) * K, hipMemcpyHostToDevice, s));
    DynArgs a{};
    a.y = y;
    double* const t = reinterpret_cast<double*>(dv + o_t);
    a.t = t;
    a.sig = reinterpret_cast<const LimSig*>(dv);
    a.nsig = nsig;
    a.K = K;
    a.ystats = meter.stats_dev();
    a.thr = d.threshold;
    a.k = 1.0 - 1.0 / d.ratio;
    a.rho = std::max<long long>(1, std::llrint(d.release * 65536.0 / rate));
    a.alpha = std::max<long long>(1, std::llrint(d.attack * 65536.0 / rate));
    a.h = reinterpret_cast<const double*>(dv + o_h);
    a.dq = reinterpret_cast<long long*>(dv + o_dq);
    a.u = reinterpret_cast<long long*>(dv + o_u);
    a.keyf = reinterpret_cast<long long*>(dv + o_key);
    a.keyb = reinterpret_cast<long long*>(dv + o_key + kb);
    a.carf = reinterpret_cast<long long*>(dv + o_key + 2 * kb);
    a.carb = reinterpret_cast<long long*>(dv + o_key + 3 * kb);
    a.utmax = reinterpret_cast<double*>(dv + o_ut);
    a.yc = reinterpret_cast<double*>(dv + o_yc);
    a.e_out = keep_parts ? reinterpret_cast<double*>(dv + o_e) : nullptr;
    a.s_out = keep_parts ? reinterpret_cast<double*>(dv + o_s) : nullptr;
    a.stats = reinterpret_cast<double*>(dv + o_stats);
    parts_ = Parts{a.e_out, a.s_out, a.yc, reinterpret_cast<const int64_t*>(a.dq), reinterpret_cast<const int64_t*>(a.u)};
    if (tiles > 0) {
        limiter_interp(y, a.sig, nsig, total, t, s);
        hipLaunchKernelGGL(k_dyn_detect, dim3((unsigned)tiles), dim3(kLanes), 0, s, a);
        hipLaunchKernelGGL(k_dyn_carry, dim3(nsig), dim3(64), 0, s, a);
        hipLaunchKernelGGL(k_dyn_scan, dim3((unsigned)tiles), dim3(kLanes), 0, s, a);
        hipLaunchKernelGGL(k_dyn_apply, dim3((unsigned)tiles), dim3(kLanes), 0, s, a);
    }
    hipLaunchKernelGGL(k_dyn_stats, dim3(nsig), dim3(64), 0, s, a);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(stats_host_, a.stats, 24 * (size_t)nsig, hipMemcpyDeviceToHost, s));
    return total > 0 ? a.yc : y;
}

}  // namespace sbv2
