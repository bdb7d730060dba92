// The formant contour of a delivered signal (formants.h; the definition is above sbv2_formant_contour in include/sbv2_hip.h): one launch,
// k_formant_lpc, from the samples a formatted fetch leaves in HBM to F / B / status of every frame.  Everything is f64 and latency-bound, as
// k_track_path is: matrix instructions have no place here (the only products that could feed them, p + 1 dot products per frame, are a few
// per cent of a frame's work and would have to leave f64).
//
// A frame has a short parallel head and a long serial tail.
//   Head.  The window is staged ONCE in LDS as s[i] = (u[b + i] - alpha u[b + i - 1]) w[i] in f64 (at most 2048 x 8 B = 16 KB), the
//     pre-emphasis and the window product applied on the way in; positions outside the signal read as 0, nothing outside [0, n) is addressed.
//     Lag k of the autocorrelation is ONE wave's sum: lane l adds s[i] s[i + k] over i = l, l + 64, ... in ascending order, then the 64
//     partial sums meet in an xor butterfly, which leaves the same bits in every lane.  The p + 1 lags are dealt over the frame's waves.
//   Tail, on one wave, in registers: lane j holds r[j], then a[j].  A Levinson step is one butterfly sum (the reflection coefficient) and two
//     shuffles (r[m - j], a[m - j]).  The roots: ONE LANE PER ROOT (p <= 50 < 64).  An Aberth step per lane is a complex Horner pass for A(z_i) and
//     A'(z_i), then sum_{j != i} 1 / (z_i - z_j).  Both loops take their operand of step k (a[k], z_k) from lane k by v_readlane: the loop
//     counter is wave-uniform, so the value arrives in scalar registers and enters the lanes' arithmetic as a scalar operand.  The
//     alternative, a broadcast read from LDS, would need a[] and every iteration's z[] written there first, with a wave barrier per
//     iteration, for the same bits; with nothing in LDS the tail has no barrier at all and the frame's other waves can leave.
//     The convergence vote is wave-wide (__all).  Selection is a rank count across lanes: each kept root counts the kept roots below it.
// Ownership (formant_frames_per_block, formants.h): four short frames to a workgroup, a wave each, or one long frame to a workgroup.
#include "formants.h"

#include <cmath>
#include <cstring>

namespace sbv2 {

namespace {

constexpr int kBlock = 256, kWave = 64;
constexpr double kPi = 3.14159265358979323846;

struct FormantArgs {
    const void* x;
    int64_t n, hop, n_frames;
    int window, order, n_formants;
    double alpha, rate, f_lo, f_hi, bw_max;
    const double* w;    // [window]
    double* F;          // [n_frames][n_formants]
    double* B;          // [n_frames][n_formants]
    double* lpc;        // [n_frames][order + 1], or NULL
    int32_t* status;    // [n_frames]
};

struct MulawCode {
    uint8_t c;
};
struct AlawCode {
    uint8_t c;
};
// u[j] of the definition: exact in f64 for the integer encodings
__device__ inline double formant_load(const float* x, int64_t i) { return (double)x[i]; }
__device__ inline double formant_load(const int16_t* x, int64_t i) { return (double)x[i] * (1.0 / 32768.0); }
__device__ inline double formant_load(const MulawCode* x, int64_t i) { return (double)mulaw_decode(x[i].c) * (1.0 / 32768.0); }
__device__ inline double formant_load(const AlawCode* x, int64_t i) { return (double)alaw_decode(x[i].c) * (1.0 / 32768.0); }

// the sum of the wave's 64 values in a fixed tree; every lane receives the same bits (a + b = b + a at every level)
__device__ inline double wave_sum(double v) {
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) v += __shfl_xor(v, d, kWave);
    return v;
}
// lane l's value in every lane; l is wave-uniform
__device__ inline double from_lane(double v, int l) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l), hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}

// The tail of one frame on one wave (all 64 lanes active): r[lane] in, F / B / lpc / status of frame f out.
__device__ inline void formant_tail(const FormantArgs& a, int64_t f, int lane, double r) {
    const int p = a.order, nk = a.n_formants;
    double aj = lane == 0 ? 1.0 : 0.0;   // a[lane]
    int32_t st = 0;
    const double r0 = from_lane(r, 0);
    if (r0 == 0.0) {   // digital silence: no formants (wave-uniform)
        if (lane < nk) a.F[f * nk + lane] = 0.0, a.B[f * nk + lane] = 0.0;
        if (a.lpc && lane <= p) a.lpc[f * (p + 1) + lane] = aj;
        if (lane == 0) a.status[f] = 0;
        return;
    }

    // Levinson-Durbin: after step m, a[1 .. m] predict with error E
    double E = r0;
    for (int m = 1; m <= p; ++m) {
        const bool inner = lane >= 1 && lane < m;
        const int src = (m - lane) & (kWave - 1);
        const double rmj = __shfl(r, src, kWave), amj = __shfl(aj, src, kWave);
        const double acc = wave_sum(inner ? aj * rmj : 0.0);
        const double k = -(from_lane(r, m) + acc) / E;
        if (inner) aj += k * amj;
        if (lane == m) aj = k;
        E *= 1.0 - k * k;
        if (!(E > 0.0)) {   // (a NaN stops it too)
            st |= kFormantLevinsonStopped;
            break;
        }
    }
    if (a.lpc && lane <= p) a.lpc[f * (p + 1) + lane] = aj;

    // Aberth-Ehrlich: every root corrected at once from the previous iteration's roots
    const bool root = lane < p;
    const double ang = (2.0 * kPi * (double)lane + 0.5) / (double)p;
    double zr = kFormantStart * cos(ang), zi = kFormantStart * sin(ang);
    bool conv = false;
    for (int it = 0; it < kFormantMaxIter && !conv; ++it) {
        double br = 1.0, bi = 0.0, cr = 0.0, ci = 0.0;   // A(z), A'(z)
        for (int k = 1; k <= p; ++k) {
            const double ak = from_lane(aj, k);
            const double tr = cr * zr - ci * zi + br;
            ci = cr * zi + ci * zr + bi;
            cr = tr;
            const double ur = br * zr - bi * zi + ak;
            bi = br * zi + bi * zr;
            br = ur;
        }
        const double c2 = cr * cr + ci * ci;
        const double qr = (br * cr + bi * ci) / c2, qi = (bi * cr - br * ci) / c2;   // A / A'
        double sr = 0.0, si = 0.0;   // sum_{j != lane} 1 / (z - z_j), ascending j
        for (int j = 0; j < p; ++j) {
            const double dr = zr - from_lane(zr, j), di = zi - from_lane(zi, j);
            if (j != lane) {
                const double inv = 1.0 / (dr * dr + di * di);
                sr += dr * inv;
                si -= di * inv;
            }
        }
        const double gr = 1.0 - (qr * sr - qi * si), gi = -(qr * si + qi * sr);
        const double g2 = gr * gr + gi * gi;
        const double wr = (qr * gr + qi * gi) / g2, wi = (qi * gr - qr * gi) / g2;
        zr -= wr;
        zi -= wi;
        const double lim = kFormantTol * kFormantTol * fmax(1.0, zr * zr + zi * zi);   // |w| < tol max(1, |z|), squared
        conv = __all(!root || wr * wr + wi * wi < lim);
    }
    if (!conv) st |= kFormantCapHit;

    // selection: the kept roots in ascending F, by rank
    const double F = atan2(zi, zr) * a.rate / (2.0 * kPi), B = -0.5 * log(zr * zr + zi * zi) * a.rate / kPi;
    const bool keep = root && F >= a.f_lo && F <= a.f_hi && B > 0.0 && B <= a.bw_max;
    const unsigned long long kept = __ballot(keep);
    int rank = 0;
    for (int j = 0; j < p; ++j) {
        const double Fj = from_lane(F, j);
        if (((kept >> j) & 1) && (Fj < F || (Fj == F && j < lane))) ++rank;
    }
    const int count = __popcll(kept);
    if (keep && rank < nk) a.F[f * nk + rank] = F, a.B[f * nk + rank] = B;
    if (lane < nk && lane >= count) a.F[f * nk + lane] = 0.0, a.B[f * nk + lane] = 0.0;
    if (lane == 0) a.status[f] = st;
}

// FPB frames per workgroup: 4 (a wave per frame, window <= kFormantPackWindow) or 1 (four waves share the head)
template <class T, int FPB>
__global__ __launch_bounds__(kBlock) void k_formant_lpc(const FormantArgs a) {
    constexpr int WPF = kBlock / kWave / FPB, LANES = kWave * WPF, SLOT = FPB == 1 ? kFormantMaxWindow : kFormantPackWindow;
    __shared__ double sh_s[FPB * SLOT];
    __shared__ double sh_r[FPB][kWave];
    const int wave = (int)threadIdx.x / kWave, lane = (int)threadIdx.x % kWave;
    const int slot = wave / WPF, wf = wave % WPF;
    const int64_t f = (int64_t)blockIdx.x * FPB + slot;
    const bool live = f < a.n_frames;
    const int W = a.window, p = a.order;
    double* s = sh_s + slot * SLOT;
    if (live) {
        const T* x = static_cast<const T*>(a.x);
        const int64_t n = a.n, b = f * a.hop + a.hop / 2 - W / 2;
        const auto at = [x, n](int64_t i) -> double { return i >= 0 && i < n ? formant_load(x, i) : 0.0; };
        for (int i = wf * kWave + lane; i < W; i += LANES) s[i] = (at(b + i) - a.alpha * at(b + i - 1)) * a.w[i];
    }
    __syncthreads();
    if (live)
        for (int k = wf; k <= p; k += WPF) {
            double acc = 0.0;
            for (int i = lane; i + k < W; i += kWave) acc += s[i] * s[i + k];
            acc = wave_sum(acc);
            if (lane == 0) sh_r[slot][k] = acc;
        }
    __syncthreads();
    if (!live || wf != 0) return;   // (no barrier below)
    formant_tail(a, f, lane, lane <= p ? sh_r[slot][lane] : 0.0);
}

template <class T>
void launch_formant(const FormantArgs& a, hipStream_t s) {
    const int fpb = formant_frames_per_block(a.window);
    const dim3 grid((unsigned)((a.n_frames + fpb - 1) / fpb)), blk(kBlock);
    if (fpb == 4) hipLaunchKernelGGL((k_formant_lpc<T, 4>), grid, blk, 0, s, a);
    else hipLaunchKernelGGL((k_formant_lpc<T, 1>), grid, blk, 0, s, a);
    HIP_CHECK(hipGetLastError());
}

}  // namespace

double FormantContourSpec::alpha() const { return std::exp(-2.0 * kPi * kFormantPreHz / (double)sample_rate); }

FormantContourSpec formant_contour_spec(int sample_rate, int64_t hop, int window, int order, int n_formants, double f_lo, double f_hi, double bw_max) {
    const std::string who = "formant contour: ";
    SBV2_REQUIRE(sample_rate > 0 && sample_rate <= kFormantMaxRate,
                 who + "sample rate must be in [1, " + std::to_string(kFormantMaxRate) + "]: " + std::to_string(sample_rate));
    SBV2_REQUIRE(hop >= 1, who + "hop must be >= 1: " + std::to_string(hop));
    FormantContourSpec sp;
    sp.sample_rate = sample_rate;
    sp.hop = hop;
    sp.window = window ? window : sample_rate / 40;
    SBV2_REQUIRE(sp.window >= kFormantMinWindow && sp.window <= kFormantMaxWindow,
                 who + "window must be in [64, 2048] (0: sample_rate / 40): " + std::to_string(sp.window));
    sp.order = order ? order : (2 + sample_rate / 1000 + 1) / 2 * 2;
    SBV2_REQUIRE(sp.order >= kFormantMinOrder && sp.order <= kFormantMaxOrder && sp.order % 2 == 0,
                 who + "order must be even and in [4, 50] (0: 2 + sample_rate / 1000, rounded up to even): " + std::to_string(sp.order));
    SBV2_REQUIRE(sp.order < sp.window / 4, who + "order must be below window / 4 = " + std::to_string(sp.window / 4) + ": " + std::to_string(sp.order));
    sp.n_formants = n_formants;
    SBV2_REQUIRE(n_formants >= 1 && n_formants <= kFormantMaxKept && n_formants <= sp.order / 2,
                 who + "n_formants must be in [1, min(8, order / 2)]: " + std::to_string(n_formants));
    sp.f_lo = f_lo == 0.0 ? 50.0 : f_lo;
    sp.f_hi = f_hi == 0.0 ? std::min(5500.0, sample_rate / 2.0 - 50.0) : f_hi;
    sp.bw_max = bw_max == 0.0 ? sample_rate / 2.0 : bw_max;
    SBV2_REQUIRE(sp.f_lo > 0.0 && sp.f_lo < sp.f_hi && sp.f_hi < sample_rate / 2.0,
                 who + "0 < f_lo < f_hi < sample_rate / 2 must hold: " + std::to_string(sp.f_lo) + ", " + std::to_string(sp.f_hi));
    SBV2_REQUIRE(sp.bw_max > 0.0, who + "bw_max must be > 0: " + std::to_string(sp.bw_max));
    return sp;
}

void formant_window(int window, std::vector<double>* w) {
    w->resize((size_t)window);
    const double c = (double)(window - 1) / 2.0, e = std::exp(-12.0);
    for (int i = 0; i < window; ++i) {
        const double t = ((double)i - c) / (double)(window + 1);
        (*w)[i] = (std::exp(-12.0 * t * t) - e) / (1.0 - e);
    }
}

void Formants::run(const void* x, int encoding, int64_t n, const FormantContourSpec& sp, hipStream_t s, bool lpc) {
    SBV2_REQUIRE(pcm_encoding_known(encoding), "internal: formants of an unknown encoding");
    SBV2_REQUIRE(n >= 0 && sp.hop >= 1 && sp.window >= kFormantMinWindow && sp.window <= kFormantMaxWindow && sp.order >= kFormantMinOrder &&
                     sp.order <= kFormantMaxOrder && sp.order < kWave && sp.order < sp.window && sp.n_formants >= 1 &&
                     sp.n_formants <= kFormantMaxKept && sp.sample_rate > 0,
                 "internal: bad formant contour spec");
    const int64_t nf = formant_frames(n, sp.hop);
    SBV2_REQUIRE(nf < (1 << 30), "too many formant frames: " + std::to_string(nf) + " >= 2^30");
    nf_ = nf;
    nk_ = sp.n_formants;
    nlpc_ = lpc ? nf * (sp.order + 1) : 0;
    if (nf == 0) return;
    SBV2_REQUIRE(x, "internal: no samples");

    if (!windows_.count(sp.window) && windows_.size() >= kMaxWindows) {   // (nothing enqueued reads what is dropped)
        HIP_CHECK(hipStreamSynchronize(s));
        windows_.clear();
    }
    DeviceBuffer& wb = windows_[sp.window];
    if (!wb.get()) {   // once per window length and context; s is synchronised because the staging is reused
        std::vector<double> w;
        formant_window(sp.window, &w);
        const size_t wbytes = sizeof(double) * w.size();
        std::memcpy(stage_.reserve(wbytes, sizeof(double) * kFormantMaxWindow, s), w.data(), wbytes);
        HIP_CHECK(hipMemcpyAsync(wb.reserve(wbytes, s), stage_.get(), wbytes, hipMemcpyHostToDevice, s));
        HIP_CHECK(hipStreamSynchronize(s));
    }

    const size_t doubles = (size_t)(2 * nf * nk_ + nlpc_), bytes = sizeof(double) * doubles + sizeof(int32_t) * (size_t)nf;
    char* h = static_cast<char*>(host_.reserve(bytes, std::max<size_t>(bytes * 2, 4096), s));
    double* d = static_cast<double*>(dev_.reserve(bytes, std::max<size_t>(bytes * 2, 4096), s));
    FormantArgs a;
    a.x = x;
    a.n = n;
    a.hop = sp.hop;
    a.n_frames = nf;
    a.window = sp.window;
    a.order = sp.order;
    a.n_formants = sp.n_formants;
    a.alpha = sp.alpha();
    a.rate = (double)sp.sample_rate;
    a.f_lo = sp.f_lo;
    a.f_hi = sp.f_hi;
    a.bw_max = sp.bw_max;
    a.w = wb.as<double>();
    a.F = d;
    a.B = d + nf * nk_;
    a.lpc = lpc ? d + 2 * nf * nk_ : nullptr;
    a.status = reinterpret_cast<int32_t*>(d + doubles);
    if (encoding == kEncS16) launch_formant<int16_t>(a, s);
    else if (encoding == kEncMulaw) launch_formant<MulawCode>(a, s);
    else if (encoding == kEncAlaw) launch_formant<AlawCode>(a, s);
    else launch_formant<float>(a, s);
    HIP_CHECK(hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, s));
}

}  // namespace sbv2
