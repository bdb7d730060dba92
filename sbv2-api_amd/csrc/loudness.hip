// Loudness of formatted signals on the device: BS.1770-4 integrated loudness with its two gates, a 4x true-peak meter and the per-signal gain
// G = min(target - L, ceiling - TP) dB.  All of it in f64, on y (the resampled signal before any gain); the K-weighted signal never goes to HBM.
//
// Convention (the one tests/test_loudness.py pins): w = y through the K-weighting cascade (shelf, then high-pass; transposed direct form II,
// zero initial state), S = fs / 10, quarter q = sum w^2 over [q S, (q + 1) S) (complete quarters only), block j = quarters j..j+3,
// z_j = sum / (4 S), l_j = -0.691 + 10 log10 z_j; gates l_j > -70 and l_j > mean-of-passing - 10 (in the log domain); L = -0.691 + 10 log10
// (mean z of the blocks that pass both), -inf when none does; a signal shorter than 4 S is one block over its whole length.  TP = 20 log10
// max |resample_poly(y, 4, 1, window = h4 / 4)|, h4 a Kaiser(8.6) windowed sinc of 97 taps, each phase summing to 1.
//
// Kernel design.  The cascade is a linear recurrence on a 4-double state s: over m samples s_end = A^m s_start + e, e = the end state of a
// zero-start run.  Each signal is cut into segments of m samples (m divides S, so a quarter is a whole number of segments):
//   k_kw_zero   one lane per segment runs from zero state and writes e;
//   k_kw_carry  one workgroup per signal: each lane folds a chunk of consecutive segments, a Hillis-Steele scan over the lanes' chunk maps
//               (powers of A^(m c) in LDS) gives every chunk's start, each lane walks its chunk again and writes every segment's start state;
//   k_kw_rerun  one lane per segment reruns its segment from its true start and sums w^2 in sample order (the segment's partial);
//   k_true_peak one thread per sample: phases 1-3 of the interpolator from an LDS tile (the 72 taps are kernel arguments, uniform across a
//               wave), max with |y|, then one max per workgroup; a workgroup that straddles a signal edge uses atomicMax on the bit pattern of
//               the non-negative double per wave or lane instead (exact, order-free; rare, so no address sees many of them);
//   k_gate      one workgroup per signal: quarters from the segment partials, blocks from quarters, both gates with fixed-order reductions,
//               the true peak from the workgroup maxima and the atomic one, then L, TP, G and the gain.
// Every sum runs in a fixed order and no value goes through a float atomic add, so two fetches of one run give the same bits.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "../../include/sbv2_hip.h"
#include "kweight.h"
#include "loudness.h"

namespace sbv2 {

namespace {

constexpr int kTpHalf = 48;     // true-peak interpolator: taps n in [-48, 48] at 4 fs
constexpr int kTpTaps = 24;     // per phase 1..3: n = p + 4 d, d in [-12, 11]
constexpr int kTpBack = 12;     // y[o - d] for d in [-12, 11]: the window is y[o - 11, o + 12]
constexpr int kScanLanes = 256;
constexpr int kScanLevels = 8;  // log2(kScanLanes)

// samples per K-weighting segment at each rate, a divisor of S = fs / 10 (S / m segments per quarter) near 240.  The three K-weighting passes
// take well under 0.1 ms at these lengths on the bench batch; other lengths were not measured.
int segment_len(int rate) {
    switch (rate) {
        case 8000: case 16000: case 32000: return 200;
        case 22050: case 44100: return 245;
        case 24000: case 48000: return 240;
    }
    SBV2_REQUIRE(false, "unsupported sample rate " + std::to_string(rate) + " (8000 16000 22050 24000 32000 44100 48000)");
    return 0;
}

struct LSig {
    int64_t off, n, seg0;   // samples y[off, off + n); its segments are [seg0, seg0 + ceil(n / m))
};

struct KwArgs {
    const double* y;
    const LSig* sig;
    int nsig, m;
    int64_t nseg;
    double c[10];   // shelf b0 b1 b2 a1 a2, high-pass b0 b1 b2 a1 a2
    double A[16];   // A^m, row-major
    double* e;      // [nseg][4] zero-start end states
    double* st;     // [nseg][4] true start states
    double* part;   // [nseg] sum of w^2 over the segment
};

__device__ __forceinline__ int find_sig_seg(const LSig* sig, int nsig, int64_t k) {   // last signal with seg0 <= k
    int lo = 0, hi = nsig - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (sig[mid].seg0 <= k) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ int find_sig_off(const LSig* sig, int nsig, int64_t o) {   // last signal with off <= o
    int lo = 0, hi = nsig - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (sig[mid].off <= o) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ void matmul(const double* X, const double* Y, double* R) {
    double t[16];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            double a = 0.0;
            for (int k = 0; k < 4; ++k) a = fma(X[4 * i + k], Y[4 * k + j], a);
            t[4 * i + j] = a;
        }
    for (int i = 0; i < 16; ++i) R[i] = t[i];
}

// the segment of lane k: samples y[*start, *start + *len)
__device__ __forceinline__ bool segment_of(const KwArgs& a, int64_t k, int64_t* start, int* len) {
    if (k >= a.nseg) return false;
    const LSig g = a.sig[find_sig_seg(a.sig, a.nsig, k)];
    const int64_t first = (k - g.seg0) * a.m;
    *start = g.off + first;
    *len = (int)min((int64_t)a.m, g.n - first);
    return true;
}

// runs y[start, start + len) through the cascade from state s; returns sum w^2 in sample order.  Five samples are loaded ahead of use
// (m is a multiple of 5 at every rate): a lane's stream is serial, so the loads must not wait on the recurrence.
__device__ __forceinline__ double kw_run(const KwArgs& a, int64_t start, int len, double* s) {
    const double* x = a.y + start;
    double acc = 0.0;
    int i = 0;
    for (; i + 5 <= len; i += 5) {
        double v[5];
#pragma unroll
        for (int r = 0; r < 5; ++r) v[r] = x[i + r];
#pragma unroll
        for (int r = 0; r < 5; ++r) {
            const double w = kw_step(a.c, s, v[r]);
            acc = fma(w, w, acc);
        }
    }
    for (; i < len; ++i) {
        const double w = kw_step(a.c, s, x[i]);
        acc = fma(w, w, acc);
    }
    return acc;
}

__global__ __launch_bounds__(256) void k_kw_zero(KwArgs a) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int64_t start;
    int len;
    if (!segment_of(a, k, &start, &len)) return;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    kw_run(a, start, len, s);
    for (int i = 0; i < 4; ++i) a.e[4 * k + i] = s[i];
}

// one workgroup per signal: lane t owns segments [t c, min((t + 1) c, nseg)) of it, c = ceil(nseg / 256)
__global__ __launch_bounds__(kScanLanes) void k_kw_carry(KwArgs a) {
    __shared__ double P[kScanLevels][16];   // (A^m)^(c 2^d)
    __shared__ double Q[kScanLanes][4];
    const LSig g = a.sig[blockIdx.x];
    const int64_t nseg = (g.n + a.m - 1) / a.m;
    if (nseg == 0) return;
    const int t = threadIdx.x;
    const int64_t c = (nseg + kScanLanes - 1) / kScanLanes;
    if (t == 0) {   // (A^m)^c by squaring, then its squares
        double r[16], b[16];
        for (int i = 0; i < 16; ++i) {
            r[i] = i % 5 == 0 ? 1.0 : 0.0;
            b[i] = a.A[i];
        }
        for (int64_t p = c; p; p >>= 1) {
            if (p & 1) matmul(r, b, r);
            if (p > 1) matmul(b, b, b);
        }
        for (int i = 0; i < 16; ++i) P[0][i] = r[i];
        for (int d = 1; d < kScanLevels; ++d) matmul(P[d - 1], P[d - 1], P[d]);
    }
    const int64_t lo = g.seg0 + min(nseg, t * c), hi = g.seg0 + min(nseg, (t + 1) * c);
    double f[4] = {0.0, 0.0, 0.0, 0.0};   // the chunk's end state from a zero start
    for (int64_t k = lo; k < hi; ++k) kw_matvec(a.A, f, a.e + 4 * k, f);
    for (int i = 0; i < 4; ++i) Q[t][i] = f[i];
    __syncthreads();
    for (int d = 0; d < kScanLevels; ++d) {   // Q[t] = end state of chunk t from the signal's zero start
        const int sh = 1 << d;
        double v[4] = {0.0, 0.0, 0.0, 0.0};
        if (t >= sh) kw_matvec(P[d], Q[t - sh], Q[t], v);
        __syncthreads();
        if (t >= sh)
            for (int i = 0; i < 4; ++i) Q[t][i] = v[i];
        __syncthreads();
    }
    double s[4];
    for (int i = 0; i < 4; ++i) s[i] = t == 0 ? 0.0 : Q[t - 1][i];
    for (int64_t k = lo; k < hi; ++k) {
        for (int i = 0; i < 4; ++i) a.st[4 * k + i] = s[i];
        kw_matvec(a.A, s, a.e + 4 * k, s);
    }
}

__global__ __launch_bounds__(256) void k_kw_rerun(KwArgs a) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int64_t start;
    int len;
    if (!segment_of(a, k, &start, &len)) return;
    double s[4];
    for (int i = 0; i < 4; ++i) s[i] = a.st[4 * k + i];
    a.part[k] = kw_run(a, start, len, s);
}

struct TpArgs {
    const double* y;
    const LSig* sig;
    int nsig;
    int64_t total;
    double h[3][kTpTaps];   // phase p + 1, tap d + 12: h4(p + 1 + 4 d)
    unsigned long long* peak;   // per signal: max over the straddling workgroups (bit pattern)
    double* bmax;               // per workgroup: its max when it lies in one signal, else 0
};

__global__ __launch_bounds__(256) void k_true_peak(TpArgs a) {
    constexpr int kTile = 256 + 2 * kTpBack - 1;
    __shared__ double tile[kTile];   // y[base - 11, base + 268)
    const int64_t base = (int64_t)blockIdx.x * 256;
    for (int i = threadIdx.x; i < kTile; i += 256) {
        const int64_t g = base - (kTpBack - 1) + i;
        tile[i] = g >= 0 && g < a.total ? a.y[g] : 0.0;
    }
    __syncthreads();
    const int64_t o = base + threadIdx.x;
    const bool live = o < a.total;
    int s = -1;
    double m = 0.0;
    if (live) {
        s = find_sig_off(a.sig, a.nsig, o);
        const LSig g = a.sig[s];
        const double* w = tile + threadIdx.x + 2 * kTpBack - 1;   // w[-d] = y[o - d]
        double z[3] = {0.0, 0.0, 0.0};
        if (o - (kTpBack - 1) >= g.off && o + kTpBack < g.off + g.n) {
#pragma unroll
            for (int d = 0; d < kTpTaps; ++d) {
                const double x = w[-d];
#pragma unroll
                for (int p = 0; p < 3; ++p) z[p] = fma(a.h[p][d], x, z[p]);
            }
        } else {   // the window crosses the signal's edge: y = 0 outside it
#pragma unroll
            for (int d = 0; d < kTpTaps; ++d) {
                const int64_t j = o + kTpBack - d;
                const double x = j >= g.off && j < g.off + g.n ? w[-d] : 0.0;
#pragma unroll
                for (int p = 0; p < 3; ++p) z[p] = fma(a.h[p][d], x, z[p]);
            }
        }
        m = fmax(fmax(fabs(tile[threadIdx.x + kTpBack - 1]), fabs(z[0])), fmax(fabs(z[1]), fabs(z[2])));
    }
    // (the same test in every lane: a workgroup-uniform branch)
    if (find_sig_off(a.sig, a.nsig, base) == find_sig_off(a.sig, a.nsig, min(base + 255, a.total - 1))) {
        __shared__ double wmax[4];
        for (int d = 32; d >= 1; d >>= 1) m = fmax(m, __shfl_xor(m, d));
        if (threadIdx.x % 64 == 0) wmax[threadIdx.x / 64] = m;
        __syncthreads();
        if (threadIdx.x == 0) a.bmax[blockIdx.x] = fmax(fmax(wmax[0], wmax[1]), fmax(wmax[2], wmax[3]));
        return;
    }
    if (threadIdx.x == 0) a.bmax[blockIdx.x] = 0.0;
    const int s0 = __shfl(s, 0);
    if (__all(!live || s == s0)) {   // one signal in the wave: reduce first, one atomic
        for (int d = 32; d >= 1; d >>= 1) m = fmax(m, __shfl_xor(m, d));
        if (threadIdx.x % warpSize == 0 && s0 >= 0) atomicMax(a.peak + s0, (unsigned long long)__double_as_longlong(m));
    } else if (live) {
        atomicMax(a.peak + s, (unsigned long long)__double_as_longlong(m));
    }
}

struct GateArgs {
    const LSig* sig;
    const double* part;
    const unsigned long long* peak;
    const double* bmax;
    int m, S;
    int apply;
    double target, ceiling;
    double* stats;   // [nsig][3]: L, TP, G
    double* gain;    // [nsig]
};

// sum (or max) of v over the workgroup in a fixed order (a tree over the lanes' values); every lane gets the result
template <bool MAX = false>
__device__ double block_reduce(double v, double* red) {
    const int t = threadIdx.x;
    __syncthreads();
    red[t] = v;
    __syncthreads();
    for (int h = 128; h >= 1; h >>= 1) {
        if (t < h) red[t] = MAX ? fmax(red[t], red[t + h]) : red[t] + red[t + h];
        __syncthreads();
    }
    return red[0];
}

__device__ __forceinline__ double lufs(double z) { return -0.691 + 10.0 * log10(z); }

__global__ __launch_bounds__(256) void k_gate(GateArgs a) {
    __shared__ double red[256];
    const LSig g = a.sig[blockIdx.x];
    const int t = threadIdx.x;
    const int qs = a.S / a.m;   // segments per quarter
    const double* part = a.part + g.seg0;
    double L = -INFINITY;
    if (g.n > 0 && g.n < 4 * (int64_t)a.S) {   // one block over the whole signal
        if (t == 0) {
            const int64_t nseg = (g.n + a.m - 1) / a.m;
            double q = 0.0;
            for (int64_t k = 0; k < nseg; ++k) q += part[k];
            const double l = lufs(q / (double)g.n);
            if (l > -70.0) L = l;
        }
    } else if (g.n > 0) {
        const int64_t nb = g.n / a.S - 3;
        auto block_z = [&](int64_t j) {
            double z = 0.0;
            for (int q = 0; q < 4; ++q) {
                double sq = 0.0;
                const double* p = part + (j + q) * qs;
                for (int i = 0; i < qs; ++i) sq += p[i];
                z += sq;
            }
            return z / (4.0 * a.S);
        };
        double sum = 0.0, cnt = 0.0;
        for (int64_t j = t; j < nb; j += 256) {
            const double z = block_z(j);
            if (lufs(z) > -70.0) {
                sum += z;
                cnt += 1.0;
            }
        }
        sum = block_reduce(sum, red);
        cnt = block_reduce(cnt, red);
        if (cnt > 0.0) {
            const double gate = lufs(sum / cnt) - 10.0;
            sum = cnt = 0.0;
            for (int64_t j = t; j < nb; j += 256) {
                const double z = block_z(j), l = lufs(z);
                if (l > -70.0 && l > gate) {
                    sum += z;
                    cnt += 1.0;
                }
            }
            sum = block_reduce(sum, red);
            cnt = block_reduce(cnt, red);
            L = lufs(sum / cnt);
        }
    }
    double pk = 0.0;   // the true peak: the maxima of the workgroups inside the signal, then the straddling ones'
    if (g.n > 0)
        for (int64_t b = g.off / 256 + t; b <= (g.off + g.n - 1) / 256; b += 256) pk = fmax(pk, a.bmax[b]);
    pk = fmax(block_reduce<true>(pk, red), __longlong_as_double((long long)a.peak[blockIdx.x]));
    if (t == 0) {
        const double tp = 20.0 * log10(pk);
        const double G = a.apply && isfinite(L) ? fmin(a.target - L, a.ceiling - tp) : 0.0;
        a.stats[3 * blockIdx.x] = L;
        a.stats[3 * blockIdx.x + 1] = tp;
        a.stats[3 * blockIdx.x + 2] = G;
        a.gain[blockIdx.x] = G == 0.0 ? 1.0 : pow(10.0, G / 20.0);
    }
}

}  // namespace

static_assert(kTpTaps == kTruePeakTaps, "loudness.h states the tap count");

int loudness_segment_len(int rate) { return segment_len(rate); }

// the 4x interpolator's phases 1..3: h[p][d] = h4(p + 1 + 4 (d - 12)), every phase of h4 scaled to sum to 1
void loudness_true_peak_taps(double h[3][kTruePeakTaps]) {
    double h4[2 * kTpHalf + 1], sum[4] = {0, 0, 0, 0};
    const double i0b = bessel_i0(8.6);
    for (int n = -kTpHalf; n <= kTpHalf; ++n) {
        const double x = n / 4.0, r = (double)n / kTpHalf;
        const double sinc = n == 0 ? 1.0 : std::sin(M_PI * x) / (M_PI * x);
        h4[n + kTpHalf] = sinc * bessel_i0(8.6 * std::sqrt(std::max(0.0, 1.0 - r * r))) / i0b;
        sum[((n % 4) + 4) % 4] += h4[n + kTpHalf];
    }
    for (int p = 1; p <= 3; ++p)
        for (int d = 0; d < kTpTaps; ++d) {
            const int n = p + 4 * (d - kTpBack);
            h[p - 1][d] = h4[n + kTpHalf] / sum[p];
        }
}

void loudness_kweight(int rate, double coef[10]) {
    segment_len(rate);   // refuses unsupported rates
    const double fs = rate;
    {   // high-shelf
        const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
        const double K = std::tan(M_PI * f0 / fs), Vh = std::pow(10.0, G / 20.0), Vb = std::pow(Vh, 0.4996667741545416);
        const double a0 = 1.0 + K / Q + K * K;
        coef[0] = (Vh + Vb * K / Q + K * K) / a0;
        coef[1] = 2.0 * (K * K - Vh) / a0;
        coef[2] = (Vh - Vb * K / Q + K * K) / a0;
        coef[3] = 2.0 * (K * K - 1.0) / a0;
        coef[4] = (1.0 - K / Q + K * K) / a0;
    }
    {   // high-pass
        const double f0 = 38.13547087602444, Q = 0.5003270373238773;
        const double K = std::tan(M_PI * f0 / fs), d = 1.0 + K / Q + K * K;
        coef[5] = 1.0;
        coef[6] = -2.0;
        coef[7] = 1.0;
        coef[8] = 2.0 * (K * K - 1.0) / d;
        coef[9] = (1.0 - K / Q + K * K) / d;
    }
}

LoudnessSpec loudness_spec(const sbv2_loudness* ln) {
    LoudnessSpec s;
    if (!ln) return s;
    SBV2_REQUIRE(std::isfinite(ln->target_lufs) && ln->target_lufs >= -70.0 && ln->target_lufs <= -5.0,
                 "loudness target " + std::to_string(ln->target_lufs) + " LUFS is outside [-70, -5]");
    SBV2_REQUIRE(std::isfinite(ln->true_peak_max_dbtp) && ln->true_peak_max_dbtp >= -20.0 && ln->true_peak_max_dbtp <= 0.0,
                 "true-peak ceiling " + std::to_string(ln->true_peak_max_dbtp) + " dBTP is outside [-20, 0]");
    s.apply = true;
    s.target = ln->target_lufs;
    s.ceiling = ln->true_peak_max_dbtp;
    return s;
}

// c[10], A^m[16], then the true-peak taps [3][24] of a rate: built once per rate
const std::vector<double>& LoudnessMeter::tables(int rate) {
    auto it = tables_.find(rate);
    if (it != tables_.end()) return it->second;
    std::vector<double> v(10 + 16 + 3 * kTpTaps);
    kw_table(rate, v.data());
    loudness_true_peak_taps(reinterpret_cast<double(*)[kTpTaps]>(v.data() + 26));
    return tables_[rate] = std::move(v);
}

const double* LoudnessMeter::measure(const double* y, const std::vector<FmtSignal>& sig, int rate, const LoudnessSpec& ln, hipStream_t s,
                                     bool with_peak) {
    const int nsig = (int)sig.size();
    SBV2_REQUIRE(nsig >= 1, "internal: no signal to measure");
    const int m = segment_len(rate), S = rate / 10;
    std::vector<LSig> tab(nsig);
    int64_t nseg = 0, total = 0;
    for (int i = 0; i < nsig; ++i) {
        const int64_t n = sig[i].j1 - sig[i].j0;
        tab[i] = LSig{sig[i].out_off, n, nseg};
        nseg += (n + m - 1) / m;
        total = std::max(total, sig[i].out_off + n);
    }
    SBV2_REQUIRE(total == 0 || y, "internal: no signal data");
    // device layout: table | peaks | stats | gains | e | st | part | per-workgroup true peaks (8-byte words, each part 64-byte aligned)
    const size_t tb = round_up64((int64_t)(sizeof(LSig) * nsig), 64), pk = round_up64(8 * nsig, 64), stb = round_up64(24 * nsig, 64);
    const size_t o_peak = tb, o_stats = o_peak + pk, o_gain = o_stats + stb, o_e = o_gain + pk, o_st = o_e + round_up64(32 * nseg, 64),
                 o_part = o_st + round_up64(32 * nseg, 64), o_bmax = o_part + round_up64(8 * std::max<int64_t>(nseg, 1), 64),
                 dbytes = o_bmax + round_up64(8 * std::max<int64_t>((total + 255) / 256, 1), 64);
    const size_t hbytes = tb + stb;
    char* d = static_cast<char*>(dev_.reserve(dbytes, dbytes * 2, s));
    char* h = static_cast<char*>(host_.reserve(hbytes, std::max<size_t>(hbytes * 2, 4096), s));
    std::memcpy(h, tab.data(), sizeof(LSig) * nsig);
    stats_host_ = reinterpret_cast<double*>(h + tb);
    HIP_CHECK(hipMemcpyAsync(d, h, sizeof(LSig) * nsig, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemsetAsync(d + o_peak, 0, 8 * nsig, s));
    const LSig* sig_dev = reinterpret_cast<const LSig*>(d);
    auto* peak = reinterpret_cast<unsigned long long*>(d + o_peak);
    auto* stats = reinterpret_cast<double*>(d + o_stats);
    stats_dev_ = stats;
    auto* gain = reinterpret_cast<double*>(d + o_gain);
    parts_ = Parts{reinterpret_cast<const double*>(d + o_e),    reinterpret_cast<const double*>(d + o_st), reinterpret_cast<const double*>(d + o_part),
                   reinterpret_cast<const double*>(d + o_bmax), reinterpret_cast<const double*>(d + dbytes), peak, nseg, (total + 255) / 256, m};
    if (total > 0) {
        KwArgs a;
        a.y = y;
        a.sig = sig_dev;
        a.nsig = nsig;
        a.m = m;
        a.nseg = nseg;
        const std::vector<double>& tv = tables(rate);
        std::memcpy(a.c, tv.data(), sizeof(a.c));
        std::memcpy(a.A, tv.data() + 10, sizeof(a.A));
        a.e = reinterpret_cast<double*>(d + o_e);
        a.st = reinterpret_cast<double*>(d + o_st);
        a.part = reinterpret_cast<double*>(d + o_part);
        const dim3 sg((unsigned)((nseg + 255) / 256)), blk(256);
        hipLaunchKernelGGL(k_kw_zero, sg, blk, 0, s, a);
        hipLaunchKernelGGL(k_kw_carry, dim3(nsig), dim3(kScanLanes), 0, s, a);
        hipLaunchKernelGGL(k_kw_rerun, sg, blk, 0, s, a);
        TpArgs t;
        t.y = y;
        t.sig = sig_dev;
        t.nsig = nsig;
        t.total = total;
        std::memcpy(t.h, tv.data() + 26, sizeof(t.h));
        t.peak = peak;
        t.bmax = reinterpret_cast<double*>(d + o_bmax);
        if (with_peak) hipLaunchKernelGGL(k_true_peak, dim3((unsigned)((total + 255) / 256)), blk, 0, s, t);
        else HIP_CHECK(hipMemsetAsync(t.bmax, 0, 8 * (size_t)((total + 255) / 256), s));   // no peak: k_gate reports TP = -inf
    }
    GateArgs g;
    g.sig = sig_dev;
    g.part = reinterpret_cast<const double*>(d + o_part);
    g.peak = peak;
    g.bmax = reinterpret_cast<const double*>(d + o_bmax);
    g.m = m;
    g.S = S;
    g.apply = ln.apply;
    g.target = ln.target;
    g.ceiling = ln.ceiling;
    g.stats = stats;
    g.gain = gain;
    hipLaunchKernelGGL(k_gate, dim3(nsig), dim3(256), 0, s, g);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(stats_host_, stats, 24 * (size_t)nsig, hipMemcpyDeviceToHost, s));
    return gain;
}

}  // namespace sbv2
