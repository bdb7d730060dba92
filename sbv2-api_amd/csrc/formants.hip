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
//
// The stage fed replay by replay (StreamFormants, k_stream_formant) runs the same frame body, formant_frame: only where a sample comes from
// differs (a carry of the last `window` samples and the replay, not one signal), and the ownership: a replay completes fewer frames than
// the chip has compute units, so every frame gets a workgroup, the lags dealt over its four waves, whatever the window length.
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
    // row r of F and B starts at word r * ld, of lpc at r * ld_lpc, of status at r * ld_st (the one shot: planes; a stream: records)
    int64_t ld, ld_lpc, ld_st;
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

// The tail of one frame on one wave (all 64 lanes active): r[lane] in, F / B / lpc / status of the frame out, into row `row`.
__device__ inline void formant_tail(const FormantArgs& a, int64_t row, int lane, double r) {
    const int p = a.order, nk = a.n_formants;
    double* const Fo = a.F + row * a.ld;
    double* const Bo = a.B + row * a.ld;
    double* const Lo = a.lpc ? a.lpc + row * a.ld_lpc : nullptr;
    int32_t* const So = a.status + row * a.ld_st;
    double aj = lane == 0 ? 1.0 : 0.0;   // a[lane]
    int32_t st = 0;
    const double r0 = from_lane(r, 0);
    if (r0 == 0.0) {   // digital silence: no formants (wave-uniform)
        if (lane < nk) Fo[lane] = 0.0, Bo[lane] = 0.0;
        if (Lo && lane <= p) Lo[lane] = aj;
        if (lane == 0) *So = 0;
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
    if (Lo && lane <= p) Lo[lane] = aj;

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
    if (keep && rank < nk) Fo[rank] = F, Bo[rank] = B;
    if (lane < nk && lane >= count) Fo[lane] = 0.0, Bo[lane] = 0.0;
    if (lane == 0) *So = st;
}

// The frame body of both kernels: a workgroup of four waves holds FPB frames, 4 (a wave per frame, window <= kFormantPackWindow) or 1 (four
// waves share the head).  Slot `slot` (= wave / WPF) owns frame f when live and writes row `row`; at(j) = u[j] of the definition, 0 outside the
// signal.  Every thread of the workgroup comes here (two barriers).  s[i] is one expression per element and lag k one wave's lane-strided
// sum and one butterfly, whichever wave takes it: the bits depend on neither FPB nor the accessor's source.
template <int FPB, class At>
__device__ __forceinline__ void formant_frame(const FormantArgs& a, int64_t f, int64_t row, bool live, const At& at) {
    constexpr int WPF = kBlock / kWave / FPB, LANES = kWave * WPF, SLOT = FPB == 1 ? kFormantMaxWindow : kFormantPackWindow;
    __shared__ double sh_s[FPB * SLOT];
    __shared__ double sh_r[FPB][kWave];
    const int wave = (int)threadIdx.x / kWave, lane = (int)threadIdx.x % kWave;
    const int slot = wave / WPF, wf = wave % WPF;
    const int W = a.window, p = a.order;
    double* s = sh_s + slot * SLOT;
    if (live) {
        const int64_t b = f * a.hop + a.hop / 2 - W / 2;
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
    formant_tail(a, row, lane, lane <= p ? sh_r[slot][lane] : 0.0);
}

template <class T, int FPB>
__global__ __launch_bounds__(kBlock) void k_formant_lpc(const FormantArgs a) {
    const int slot = (int)threadIdx.x / kWave / (kBlock / kWave / FPB);
    const int64_t f = (int64_t)blockIdx.x * FPB + slot;
    const T* x = static_cast<const T*>(a.x);
    const int64_t n = a.n;
    formant_frame<FPB>(a, f, f, f < a.n_frames, [x, n](int64_t i) -> double { return i >= 0 && i < n ? formant_load(x, i) : 0.0; });
}

// The fed stage (StreamFormants, formants.h), one launch per push.  Workgroup g < blocks: the frames first + g FPB ... of the push's `count`
// completed frames, into the push's records (a.F ... hold row 0 = frame `first`).  A frame's sample at j comes from the carry when j < d0 (the
// cl samples before d0, in the sample's own type), from x when d0 <= j < d1, and is 0 outside [0, total): nothing outside carry_in[0, cl) and
// x[0, d1 - d0) is addressed, whatever the arguments.  The workgroups g >= blocks write the next carry, the last cl_out fed samples, into
// the OTHER copy: no workgroup reads what one of the same launch writes.
struct StreamFormantArgs {
    FormantArgs a;          // x = the sample at d0; n and n_frames unused
    const void* carry_in;   // positions [d0 - cl, d0)
    void* carry_out;        // positions [d1 - cl_out, d1)
    int64_t d0, d1, total, first;
    int32_t count, blocks, cl, cl_out;
};

template <class T, int FPB>
__global__ __launch_bounds__(kBlock) void k_stream_formant(const StreamFormantArgs p) {
    const T* x = static_cast<const T*>(p.a.x);
    const T* cin = static_cast<const T*>(p.carry_in);
    const int64_t d0 = p.d0, d1 = p.d1, c0 = p.d0 - p.cl, total = p.total;
    if ((int)blockIdx.x >= p.blocks) {   // the carry: a push shorter than it keeps the end of the old one in front of x (uniform: no barrier here)
        T* cout = static_cast<T*>(p.carry_out);
        const int j = ((int)blockIdx.x - p.blocks) * kBlock + (int)threadIdx.x;
        if (j >= p.cl_out) return;
        const int64_t i = d1 - p.cl_out + j;
        if (i >= d0) cout[j] = x[i - d0];
        else if (i >= c0) cout[j] = cin[i - c0];
        return;
    }
    const int slot = (int)threadIdx.x / kWave / (kBlock / kWave / FPB);
    const int64_t r = (int64_t)blockIdx.x * FPB + slot;
    formant_frame<FPB>(p.a, p.first + r, r, r < p.count, [x, cin, d0, d1, c0, total](int64_t j) -> double {
        if (j < 0 || j >= total) return 0.0;
        if (j >= d0) return j < d1 ? formant_load(x, j - d0) : 0.0;
        return j >= c0 ? formant_load(cin, j - c0) : 0.0;
    });
}

template <class T>
void launch_formant(const FormantArgs& a, hipStream_t s) {
    const int fpb = formant_frames_per_block(a.window);
    const dim3 grid((unsigned)((a.n_frames + fpb - 1) / fpb)), blk(kBlock);
    if (fpb == 4) hipLaunchKernelGGL((k_formant_lpc<T, 4>), grid, blk, 0, s, a);
    else hipLaunchKernelGGL((k_formant_lpc<T, 1>), grid, blk, 0, s, a);
    HIP_CHECK(hipGetLastError());
}

template <class T>
void launch_stream_formant(const StreamFormantArgs& p, int fpb, hipStream_t s) {
    const dim3 grid((unsigned)(p.blocks + (p.cl_out + kBlock - 1) / kBlock)), blk(kBlock);
    if (fpb == 4) hipLaunchKernelGGL((k_stream_formant<T, 4>), grid, blk, 0, s, p);
    else hipLaunchKernelGGL((k_stream_formant<T, 1>), grid, blk, 0, s, p);
    HIP_CHECK(hipGetLastError());
}

// the checks Formants::run and StreamFormants::check share
void check_formant_spec(const FormantContourSpec& sp, int64_t n) {
    SBV2_REQUIRE(n >= 0 && sp.hop >= 1 && sp.window >= kFormantMinWindow && sp.window <= kFormantMaxWindow && sp.order >= kFormantMinOrder &&
                     sp.order <= kFormantMaxOrder && sp.order < kWave && sp.order < sp.window && sp.n_formants >= 1 &&
                     sp.n_formants <= kFormantMaxKept && sp.sample_rate > 0,
                 "internal: bad formant contour spec");
    const int64_t nf = formant_frames(n, sp.hop);
    SBV2_REQUIRE(nf < (1 << 30), "too many formant frames: " + std::to_string(nf) + " >= 2^30");
}

// what a launch takes of the spec
void formant_args(const FormantContourSpec& sp, const double* w, FormantArgs* a) {
    a->hop = sp.hop;
    a->window = sp.window;
    a->order = sp.order;
    a->n_formants = sp.n_formants;
    a->alpha = sp.alpha();
    a->rate = (double)sp.sample_rate;
    a->f_lo = sp.f_lo;
    a->f_hi = sp.f_hi;
    a->bw_max = sp.bw_max;
    a->w = w;
}

// The Gaussian window of a length, formed on the host and uploaded from pinned staging on s, which is synchronised (the staging is reused).
void upload_formant_window(int window, DeviceBuffer* wb, PinnedBuffer* stage, hipStream_t s) {
    std::vector<double> w;
    formant_window(window, &w);
    const size_t wbytes = sizeof(double) * w.size();
    std::memcpy(stage->reserve(wbytes, sizeof(double) * kFormantMaxWindow, s), w.data(), wbytes);
    HIP_CHECK(hipMemcpyAsync(wb->reserve(wbytes, s), stage->get(), wbytes, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipStreamSynchronize(s));
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
    check_formant_spec(sp, n);
    const int64_t nf = formant_frames(n, sp.hop);
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
    if (!wb.get()) upload_formant_window(sp.window, &wb, &stage_, s);   // once per window length and context

    const size_t doubles = (size_t)(2 * nf * nk_ + nlpc_), bytes = sizeof(double) * doubles + sizeof(int32_t) * (size_t)nf;
    char* h = static_cast<char*>(host_.reserve(bytes, std::max<size_t>(bytes * 2, 4096), s));
    double* d = static_cast<double*>(dev_.reserve(bytes, std::max<size_t>(bytes * 2, 4096), s));
    FormantArgs a;
    formant_args(sp, wb.as<double>(), &a);
    a.x = x;
    a.n = n;
    a.n_frames = nf;
    a.ld = nk_;
    a.ld_lpc = sp.order + 1;
    a.ld_st = 1;
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

// ---- the fed stage (StreamFormants, formants.h) ----
void StreamFormants::check(const FormantContourSpec& sp, int64_t total) { check_formant_spec(sp, total); }

int64_t formant_frames_complete(const FormantContourSpec& sp, int64_t total, int64_t D) {
    const int64_t nf = formant_frames(total, sp.hop);
    if (nf == 0 || D >= total) return nf;
    const int64_t r = D - (sp.hop / 2 - sp.window / 2 + sp.window);   // frame f: b + window = f hop + hop / 2 - window / 2 + window <= D
    return r < 0 ? 0 : std::min(nf, r / sp.hop + 1);
}

void StreamFormants::begin(const FormantContourSpec& sp, int encoding, int64_t total, int64_t most, hipStream_t s, int pack, bool lpc) {
    SBV2_REQUIRE(pcm_encoding_known(encoding), "internal: formants of an unknown encoding");
    SBV2_REQUIRE(most >= 0 && (pack == 0 || pack == 1 || pack == 4), "internal: bad formant stream");
    check(sp, total);
    sp_ = sp;
    encoding_ = encoding;
    total_ = total;
    nf_ = formant_frames(total, sp.hop);
    fed_ = done_ = 0;
    parity_ = 0;
    forced_ = pack == 4 && sp.window > kFormantPackWindow ? 1 : pack;
    lpc_ = lpc;
    cus_ = device_cu_count();
    rec_ = 2 * sp.n_formants + (lpc ? sp.order + 1 : 0) + 1;
    if (window_len_ != sp.window) {   // kept from the previous stream of this context when it is the same
        upload_formant_window(sp.window, &window_, &stage_, s);
        window_len_ = sp.window;
    }
    // device: the carry (two copies, each kFormantMaxWindow elements of the widest sample type), the records of one push; pinned: every frame
    const size_t row = sizeof(double) * (size_t)rec_, h_bytes = row * (size_t)nf_;
    const size_t push_bytes = row * (size_t)std::min(nf_, (most + sp.window) / sp.hop + 2);
    carry_.reserve(2 * kCarryBytes, s);
    out_.reserve(std::max<size_t>(push_bytes, 4096), s);
    host_.reserve(std::max<size_t>(h_bytes, 64), std::max<size_t>(h_bytes, 4096), s);
    HIP_CHECK(hipStreamSynchronize(s));   // (an earlier stream's copies into the mirror are done)
}

int64_t StreamFormants::push(const void* x, int64_t D0, int64_t n, hipStream_t s) {
    SBV2_REQUIRE(n >= 0 && D0 == fed_ && D0 + n <= total_, "internal: a formant push of [" + std::to_string(D0) + ", " + std::to_string(D0 + n) +
                                                               ") out of stream order (" + std::to_string(fed_) + " of " + std::to_string(total_) + " fed)");
    const int64_t D1 = D0 + n, now = complete(D1), done = now - done_;
    fed_ = D1;
    if (n > 0) {
        SBV2_REQUIRE(x, "internal: no samples to push");
        const size_t row = sizeof(double) * (size_t)rec_;
        double* out = static_cast<double*>(out_.reserve(std::max<size_t>(row * (size_t)done, 4096), s));   // (sized at begin for a push of up to `most`)
        const int nk = sp_.n_formants;
        const int fpb = forced_ ? forced_ : formant_stream_frames_per_block(done, sp_.window, cus_);
        StreamFormantArgs p{};
        formant_args(sp_, window_.as<double>(), &p.a);
        p.a.x = x;
        p.a.F = out;
        p.a.B = out + nk;
        p.a.lpc = lpc_ ? out + 2 * nk : nullptr;
        p.a.status = reinterpret_cast<int32_t*>(out + rec_ - 1);   // (the low word of the record's last f64 word; the high one is never read)
        p.a.ld = p.a.ld_lpc = rec_;
        p.a.ld_st = 2 * rec_;
        p.carry_in = carry_.as<char>() + (size_t)parity_ * kCarryBytes;
        p.carry_out = carry_.as<char>() + (size_t)(parity_ ^ 1) * kCarryBytes;
        p.d0 = D0;
        p.d1 = D1;
        p.total = total_;
        p.first = done_;
        p.count = (int32_t)done;
        p.blocks = (int32_t)((done + fpb - 1) / fpb);
        p.cl = (int32_t)std::min<int64_t>(D0, sp_.window);
        p.cl_out = (int32_t)std::min<int64_t>(D1, sp_.window);
        if (encoding_ == kEncS16) launch_stream_formant<int16_t>(p, fpb, s);
        else if (encoding_ == kEncMulaw) launch_stream_formant<MulawCode>(p, fpb, s);
        else if (encoding_ == kEncAlaw) launch_stream_formant<AlawCode>(p, fpb, s);
        else launch_stream_formant<float>(p, fpb, s);
        parity_ ^= 1;
        if (done) HIP_CHECK(hipMemcpyAsync(host_.as<char>() + row * (size_t)done_, out, row * (size_t)done, hipMemcpyDeviceToHost, s));
    }
    done_ = now;
    return done;
}

}  // namespace sbv2
