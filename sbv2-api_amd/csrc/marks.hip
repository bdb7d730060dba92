// Speech marks: token spans on the delivered timeline (host) and the level of every span / envelope frame (one segmented reduction on gfx950).
//
// The reduction.  A fetch with marks has two kinds of segments over the delivered samples: token spans (a few thousand samples each, now and
// then 10^5 for a pause or a forced duration, now and then none) and envelope frames (tens to hundreds of samples, tens of thousands of them).
// One launch covers both:
//   * a segment of <= kLongSegment samples is reduced by ONE wave (four segments per 256-lane workgroup): lane l takes the samples at offsets
//     l, l + 64, l + 128, ... of the segment, then the 64 partial results meet in a shuffle tree;
//   * a longer segment takes a whole workgroup: lane l of 256 takes offsets l, l + 256, ..., the four waves' results meet in LDS in wave order.
// Offsets are relative to the segment's start, loads are single elements (a wave reads 64 consecutive samples: 256 or 128 contiguous bytes),
// so an odd start in an s16 buffer needs no peeling and nothing outside [start, end) is ever addressed.  The order of the additions depends
// on the segment's length alone: no atomics, equal samples give equal bits wherever the segment lies.  s16 samples are squared as integers
// (exact in f64, as are their sums below 2^53), and so are the integers that G.711 codes decode to (one byte per sample, any start); an f32 sample's square is exact in f64 too, so only the order of the sum is this kernel's own.
// Each sample is read once per table it appears in (tokens, frames): the launch is bound by its few MB of HBM reads.
// The pitch contour of the same samples (k_pitch_yin, and k_stream_pitch for a stream's replays) is at the end of the file.
#include "marks.h"
#include "track.h"

#include <climits>
#include <cmath>
#include <cstring>

namespace sbv2 {

void marks_spans(const int64_t* d, int64_t n, int64_t hop, int64_t place, const PcmFmtSpec& s, int64_t* start, int64_t* end) {
    SBV2_REQUIRE(n >= 0 && (n == 0 || (d && start && end)), "bad arguments");
    SBV2_REQUIRE(hop >= 1 && hop <= (1 << 20), "hop must be in [1, 2^20]");
    SBV2_REQUIRE(place >= 0, "place must be >= 0");
    const int64_t limit = INT64_MAX / std::max(s.L, 1) - s.M;   // a L + M - 1 stays in range below it
    SBV2_REQUIRE(place < limit, "position out of range");
    int64_t a = place;
    for (int64_t t = 0; t < n; ++t) {
        SBV2_REQUIRE(d[t] >= 0, "negative duration of token " + std::to_string(t));
        SBV2_REQUIRE(d[t] <= (limit - a) / hop, "position out of range");
        start[t] = marks_delivered(s, a);
        a += hop * d[t];
        end[t] = marks_delivered(s, a);
    }
}

namespace {

constexpr int kBlock = 256, kWave = 64, kWavesPerBlock = kBlock / kWave;

struct LevelArgs {
    const void* x;
    const int64_t* seg;     // [nseg][2]
    const int32_t* order;   // the short segments' indices, then the long ones'
    int32_t nshort, short_blocks;
    double* sumsq;          // [nseg]
    double* peak;           // [nseg]
};

template <class T>
__device__ inline double level_load(const T* x, int64_t i) {
    return (double)x[i];
}
// G.711: the delivered byte is a code; its level is that of the integer it decodes to (pcm_format.h), exact like an s16 sample's
struct MulawCode {
    uint8_t c;
};
struct AlawCode {
    uint8_t c;
};
__device__ inline double level_load(const MulawCode* x, int64_t i) { return (double)mulaw_decode(x[i].c); }
__device__ inline double level_load(const AlawCode* x, int64_t i) { return (double)alaw_decode(x[i].c); }

// partial results of the lanes of a wave -> lane 0, in a fixed tree
__device__ inline void wave_reduce(double& ss, double& pk) {
#pragma unroll
    for (int d = kWave / 2; d >= 1; d >>= 1) {
        ss += __shfl_down(ss, d, kWave);
        pk = fmax(pk, __shfl_down(pk, d, kWave));
    }
}

template <class T>
__global__ __launch_bounds__(kBlock) void k_segment_levels(const LevelArgs a) {
    __shared__ double sh_ss[kWavesPerBlock], sh_pk[kWavesPerBlock];
    const T* x = static_cast<const T*>(a.x);
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const bool whole_block = (int)blockIdx.x >= a.short_blocks;   // uniform over the workgroup
    int k, first, stride;
    if (whole_block) {
        k = a.nshort + ((int)blockIdx.x - a.short_blocks);
        first = threadIdx.x;
        stride = kBlock;
    } else {
        k = (int)blockIdx.x * kWavesPerBlock + wave;
        if (k >= a.nshort) return;   // (no barrier on this path)
        first = lane;
        stride = kWave;
    }
    const int sgi = a.order[k];
    const int64_t s0 = a.seg[2 * sgi], len = a.seg[2 * sgi + 1] - s0;
    const T* p = x + s0;
    double ss = 0.0, pk = 0.0;
    int64_t i = first;
    for (; i + 3 * stride < len; i += 4 * stride) {   // four independent loads in flight per lane
        const double v0 = level_load(p, i), v1 = level_load(p, i + stride), v2 = level_load(p, i + 2 * stride), v3 = level_load(p, i + 3 * stride);
        ss += v0 * v0;
        ss += v1 * v1;
        ss += v2 * v2;
        ss += v3 * v3;
        pk = fmax(fmax(pk, fabs(v0)), fmax(fabs(v1), fmax(fabs(v2), fabs(v3))));
    }
    for (; i < len; i += stride) {
        const double v = level_load(p, i);
        ss += v * v;
        pk = fmax(pk, fabs(v));
    }
    wave_reduce(ss, pk);
    if (!whole_block) {
        if (lane == 0) a.sumsq[sgi] = ss, a.peak[sgi] = pk;
        return;
    }
    if (lane == 0) sh_ss[wave] = ss, sh_pk[wave] = pk;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = sh_ss[0], m = sh_pk[0];
        for (int w = 1; w < kWavesPerBlock; ++w) t += sh_ss[w], m = fmax(m, sh_pk[w]);
        a.sumsq[sgi] = t;
        a.peak[sgi] = m;
    }
}

}  // namespace

void Marks::run(const void* x, int encoding, int64_t n, const int64_t* seg, int64_t nseg, hipStream_t s) {
    SBV2_REQUIRE(pcm_encoding_known(encoding), "internal: levels of an unknown encoding");
    SBV2_REQUIRE(nseg >= 0 && nseg < (1 << 30) && n >= 0, "internal: bad segment table");
    nseg_ = nseg;
    if (nseg == 0) return;
    SBV2_REQUIRE(seg && (x || n == 0), "internal: no segment data");
    int64_t nshort = 0;
    for (int64_t i = 0; i < nseg; ++i) {
        SBV2_REQUIRE(seg[2 * i] >= 0 && seg[2 * i] <= seg[2 * i + 1] && seg[2 * i + 1] <= n,
                     "segment " + std::to_string(i) + " [" + std::to_string(seg[2 * i]) + ", " + std::to_string(seg[2 * i + 1]) + ") is outside the " +
                         std::to_string(n) + " delivered samples");
        nshort += seg[2 * i + 1] - seg[2 * i] <= kLongSegment;
    }
    // table | order | sumsq | peak (8-byte words, each part 64-byte aligned); the device buffer has the same layout
    const size_t o_order = round_up64(16 * nseg, 64), o_res = o_order + round_up64(4 * nseg, 64), bytes = o_res + 16 * (size_t)nseg;
    char* h = static_cast<char*>(host_.reserve(bytes, std::max<size_t>(bytes * 2, 4096), s));
    char* d = static_cast<char*>(dev_.reserve(bytes, std::max<size_t>(bytes * 2, 4096), s));
    std::memcpy(h, seg, 16 * (size_t)nseg);
    int32_t* order = reinterpret_cast<int32_t*>(h + o_order);
    int64_t ks = 0, kl = nshort;
    for (int64_t i = 0; i < nseg; ++i) (seg[2 * i + 1] - seg[2 * i] <= kLongSegment ? order[ks++] : order[kl++]) = (int32_t)i;
    res_host_ = reinterpret_cast<double*>(h + o_res);
    HIP_CHECK(hipMemcpyAsync(d, h, o_order + 4 * (size_t)nseg, hipMemcpyHostToDevice, s));
    LevelArgs a;
    a.x = x;
    a.seg = reinterpret_cast<const int64_t*>(d);
    a.order = reinterpret_cast<const int32_t*>(d + o_order);
    a.nshort = (int32_t)nshort;
    a.short_blocks = (int32_t)((nshort + kWavesPerBlock - 1) / kWavesPerBlock);
    a.sumsq = reinterpret_cast<double*>(d + o_res);
    a.peak = a.sumsq + nseg;
    const dim3 grid((unsigned)(a.short_blocks + (nseg - nshort))), blk(kBlock);
    if (encoding == kEncS16) hipLaunchKernelGGL(k_segment_levels<int16_t>, grid, blk, 0, s, a);
    else if (encoding == kEncMulaw) hipLaunchKernelGGL(k_segment_levels<MulawCode>, grid, blk, 0, s, a);
    else if (encoding == kEncAlaw) hipLaunchKernelGGL(k_segment_levels<AlawCode>, grid, blk, 0, s, a);
    else hipLaunchKernelGGL(k_segment_levels<float>, grid, blk, 0, s, a);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(res_host_, a.sumsq, 16 * (size_t)nseg, hipMemcpyDeviceToHost, s));
}

// ---- the fed reduction (StreamLevels, marks.h) ----
namespace {

constexpr int kCarryTable = 2 * kBlock;   // doubles per table in one copy of the carry: {ss, pk} per lane

struct StreamLevelArgs {
    const void* x;             // the sample at delivered position d0
    int64_t d0, d1;            // the push
    const int64_t* seg;        // the token table [ntok][2]
    int64_t ntok;
    int32_t tok_first, tok_count;   // the tokens this push may meet: one workgroup each
    int64_t env_hop, total, env_first;
    int32_t env_count, env_packed;   // the frames it meets; packed: four (short) frames per workgroup, one per wave
    const double* carry_in;    // [2 tables][256 lanes][2]
    double* carry_out;
    double* res;               // [ntok + nenv][2]
};

// One segment per wave (stride 64) or per workgroup (stride 256), by the segment's total length.  The piece [max(s, d0), min(e, d1)): the lane
// of offset o is o mod stride, so a lane goes on with the offsets k_segment_levels gives it, in the same order, from the carried partials.
template <class T>
__global__ __launch_bounds__(kBlock) void k_stream_levels(const StreamLevelArgs a) {
    __shared__ double sh_ss[kWavesPerBlock], sh_pk[kWavesPerBlock];
    const T* x = static_cast<const T*>(a.x);
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    int table;
    bool packed = false;
    int64_t slot, s, e;
    if ((int)blockIdx.x < a.tok_count) {
        table = 0;
        slot = a.tok_first + (int)blockIdx.x;
        s = a.seg[2 * slot];
        e = a.seg[2 * slot + 1];
    } else {
        table = 1;
        const int eb = (int)blockIdx.x - a.tok_count;
        packed = a.env_packed != 0;
        const int64_t k = packed ? (int64_t)eb * kWavesPerBlock + wave : eb;
        if (k >= a.env_count) return;   // (packed only: no barrier on that path)
        const int64_t f = a.env_first + k;
        s = f * a.env_hop;
        e = min(s + a.env_hop, a.total);
        slot = a.ntok + f;
    }
    const bool whole_block = e - s > Marks::kLongSegment;   // uniform over the workgroup (never with packed frames)
    if (!whole_block && !packed && wave) return;            // a short segment alone in its workgroup: wave 0
    const int64_t lo = max(s, a.d0), hi = min(e, a.d1);
    if (lo >= hi) return;   // (uniform over the segment's lanes: an empty span, or a segment this push does not reach)
    const int stride = whole_block ? kBlock : kWave, me = whole_block ? (int)threadIdx.x : lane;
    double ss = 0.0, pk = 0.0;
    if (lo > s) {
        const double* c = a.carry_in + table * kCarryTable + 2 * me;
        ss = c[0];
        pk = c[1];
    }
    const int64_t o0 = lo - s, len = hi - s, base = s - a.d0;   // x[base + o] is offset o of the segment; base + o >= lo - d0 >= 0
    int64_t i = o0 + ((me - (int)(o0 & (stride - 1))) & (stride - 1));
    for (; i + 3 * stride < len; i += 4 * stride) {
        const double v0 = level_load(x, base + i), v1 = level_load(x, base + i + stride), v2 = level_load(x, base + i + 2 * stride),
                     v3 = level_load(x, base + i + 3 * stride);
        ss += v0 * v0;
        ss += v1 * v1;
        ss += v2 * v2;
        ss += v3 * v3;
        pk = fmax(fmax(pk, fabs(v0)), fmax(fabs(v1), fmax(fabs(v2), fabs(v3))));
    }
    for (; i < len; i += stride) {
        const double v = level_load(x, base + i);
        ss += v * v;
        pk = fmax(pk, fabs(v));
    }
    if (hi < e) {   // the segment stays open: the lanes' partials wait for the next push
        double* c = a.carry_out + table * kCarryTable + 2 * me;
        c[0] = ss;
        c[1] = pk;
        return;
    }
    wave_reduce(ss, pk);
    if (!whole_block) {
        if (lane == 0) a.res[2 * slot] = ss, a.res[2 * slot + 1] = pk;
        return;
    }
    if (lane == 0) sh_ss[wave] = ss, sh_pk[wave] = pk;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = sh_ss[0], m = sh_pk[0];
        for (int w = 1; w < kWavesPerBlock; ++w) t += sh_ss[w], m = fmax(m, sh_pk[w]);
        a.res[2 * slot] = t;
        a.res[2 * slot + 1] = m;
    }
}

}  // namespace

void StreamLevels::check(const int64_t* seg, int64_t nseg, int64_t env_hop, int64_t total) {
    SBV2_REQUIRE(total >= 0 && nseg >= 0 && nseg < (1 << 30) && (nseg == 0 || seg), "bad segment table");
    SBV2_REQUIRE(env_hop >= 0, "env_hop must be >= 0");
    SBV2_REQUIRE(env_frames(env_hop, total) < (1 << 30), "too many envelope frames: " + std::to_string(env_frames(env_hop, total)) + " >= 2^30");
    int64_t at = 0;
    for (int64_t i = 0; i < nseg; ++i) {
        const int64_t s0 = seg[2 * i], e0 = seg[2 * i + 1];
        SBV2_REQUIRE(s0 >= 0 && s0 <= e0 && e0 <= total, "segment " + std::to_string(i) + " [" + std::to_string(s0) + ", " + std::to_string(e0) +
                                                             ") is outside the " + std::to_string(total) + " delivered samples");
        SBV2_REQUIRE(s0 >= at, "segment " + std::to_string(i) + " [" + std::to_string(s0) + ", " + std::to_string(e0) +
                                   ") starts before its predecessor ends: a stream's segments must be monotone and disjoint");
        at = e0;
    }
}

void StreamLevels::begin(const int64_t* seg, int64_t nseg, int64_t env_hop, int64_t total, hipStream_t s) {
    check(seg, nseg, env_hop, total);
    ntok_ = nseg;
    env_hop_ = env_hop;
    total_ = total;
    nenv_ = env_frames(env_hop, total);
    fed_ = tok_done_ = env_done_ = 0;
    parity_ = 0;
    seg_.assign(seg, seg + 2 * nseg);
    const int64_t nres = ntok_ + nenv_;
    // device: table | carry (two copies) | results; pinned: table | results
    const size_t o_carry = round_up64(16 * (size_t)ntok_, 64), carry_bytes = 2 * 2 * kCarryTable * sizeof(double), o_res = o_carry + carry_bytes,
                 bytes = o_res + 16 * (size_t)nres, h_res = o_carry, h_bytes = h_res + 16 * (size_t)nres;
    char* d = static_cast<char*>(dev_.reserve(bytes, std::max<size_t>(bytes * 2, 32768), s));
    char* h = static_cast<char*>(host_.reserve(h_bytes, std::max<size_t>(h_bytes * 2, 4096), s));
    HIP_CHECK(hipStreamSynchronize(s));   // (an earlier stream's copies into the mirror are done)
    d_seg_ = reinterpret_cast<int64_t*>(d);
    d_carry_ = reinterpret_cast<double*>(d + o_carry);
    d_res_ = reinterpret_cast<double*>(d + o_res);
    res_host_ = reinterpret_cast<double*>(h + h_res);
    std::memset(res_host_, 0, 16 * (size_t)nres);
    if (ntok_) {
        std::memcpy(h, seg, 16 * (size_t)ntok_);
        HIP_CHECK(hipMemcpyAsync(d_seg_, h, 16 * (size_t)ntok_, hipMemcpyHostToDevice, s));
    }
    HIP_CHECK(hipMemsetAsync(d_carry_, 0, carry_bytes + 16 * (size_t)nres, s));
}

int64_t StreamLevels::tok_complete(int64_t D) const {
    int64_t lo = 0, hi = ntok_;   // ends ascend: the first token with end > D
    while (lo < hi) {
        const int64_t mid = (lo + hi) / 2;
        if (seg_[2 * mid + 1] <= D) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

StreamLevels::Done StreamLevels::push(const void* x, int encoding, int64_t D0, int64_t n, hipStream_t s) {
    SBV2_REQUIRE(pcm_encoding_known(encoding), "internal: levels of an unknown encoding");
    SBV2_REQUIRE(n >= 0 && D0 == fed_ && D0 + n <= total_, "internal: a levels push of [" + std::to_string(D0) + ", " + std::to_string(D0 + n) +
                                                               ") out of stream order (" + std::to_string(fed_) + " of " + std::to_string(total_) + " fed)");
    const int64_t D1 = D0 + n;
    fed_ = D1;
    const int64_t tok_new = tok_complete(D1), env_new = env_complete(D1);
    const Done done{tok_new - tok_done_, env_new - env_done_};
    if (n > 0 && ntok_ + nenv_ > 0) {
        SBV2_REQUIRE(x, "internal: no samples to push");
        StreamLevelArgs a{};
        a.x = x;
        a.d0 = D0;
        a.d1 = D1;
        a.seg = d_seg_;
        a.ntok = ntok_;
        // tokens: every one before tok_done_ ended at or before D0; the push meets those that start before D1 (empty ones among them do nothing)
        int64_t t1 = tok_done_;
        while (t1 < ntok_ && seg_[2 * t1] < D1) ++t1;
        a.tok_first = (int32_t)tok_done_;
        a.tok_count = (int32_t)(t1 - tok_done_);
        a.env_hop = env_hop_;
        a.total = total_;
        int64_t env_blocks = 0;
        if (nenv_) {
            a.env_first = D0 / env_hop_;
            a.env_count = (int32_t)((D1 - 1) / env_hop_ - a.env_first + 1);
            a.env_packed = env_hop_ <= Marks::kLongSegment;
            env_blocks = a.env_packed ? (a.env_count + kWavesPerBlock - 1) / kWavesPerBlock : a.env_count;
        }
        a.carry_in = d_carry_ + (size_t)parity_ * 2 * kCarryTable;
        a.carry_out = d_carry_ + (size_t)(parity_ ^ 1) * 2 * kCarryTable;
        a.res = d_res_;
        const int64_t blocks = a.tok_count + env_blocks;
        if (blocks > 0) {
            const dim3 grid((unsigned)blocks), blk(kBlock);
            if (encoding == kEncS16) hipLaunchKernelGGL(k_stream_levels<int16_t>, grid, blk, 0, s, a);
            else if (encoding == kEncMulaw) hipLaunchKernelGGL(k_stream_levels<MulawCode>, grid, blk, 0, s, a);
            else if (encoding == kEncAlaw) hipLaunchKernelGGL(k_stream_levels<AlawCode>, grid, blk, 0, s, a);
            else hipLaunchKernelGGL(k_stream_levels<float>, grid, blk, 0, s, a);
            HIP_CHECK(hipGetLastError());
            parity_ ^= 1;
        }
        // the slots this push completed -> the mirror (tokens and frames are two contiguous ranges of the one array)
        if (done.tok) HIP_CHECK(hipMemcpyAsync(res_host_ + 2 * tok_done_, d_res_ + 2 * tok_done_, 16 * (size_t)done.tok, hipMemcpyDeviceToHost, s));
        if (done.env)
            HIP_CHECK(hipMemcpyAsync(res_host_ + 2 * (ntok_ + env_done_), d_res_ + 2 * (ntok_ + env_done_), 16 * (size_t)done.env, hipMemcpyDeviceToHost, s));
    }
    tok_done_ = tok_new;
    env_done_ = env_new;
    return done;
}

// ---- the pitch contour (Pitch, marks.h) ----
// YIN per frame as include/sbv2_hip.h states it: one workgroup per frame.  The 2 tau_max samples of the frame's window are staged once in LDS
// (integers for s16 and the G.711 codes, f64 for f32; positions outside [0, n) are zeros written there, nothing outside is addressed).  Lane
// l owns the lags l + 1, l + 1 + nt, ... (P of them, in registers) and walks j over the window: a[j] is one broadcast read for all of them,
// a[j + tau] is consecutive across lanes.  Integer differences are 32-bit, their squares are accumulated in 64 bits; f32 differences and
// squares are taken in f64, j ascending.  d(tau) goes to LDS, a chunked scan gives S(tau) (each thread sums its run of consecutive lags, one
// lane scans the runs' totals: exact for integers, one fixed order per tau_max for f32), every thread divides for its own lags, and the
// decision is two index minima over the workgroup and a short walk by one lane.  No atomics.
namespace {

struct PitchArgs {
    const void* x;
    int64_t n, hop;
    int32_t tau_min, tau_max;
    double threshold;
    double* c3;        // [nf][3]
    int32_t* lag;      // [nf]
    int32_t* voiced;   // [nf]
};

template <class T>
struct PitchTypes {   // staged sample, accumulator
    using S = int32_t;
    using D = int64_t;
};
template <>
struct PitchTypes<float> {
    using S = double;
    using D = double;
};

constexpr int kPitchMaxP = (kPitchMaxTau + kBlock - 1) / kBlock;   // lags per lane at the largest window

// One frame, by the workgroup that owns it: `at(i)` gives the sample at delivered position i (zero outside the signal) and is the only thing
// the one-shot kernel and the fed one (k_stream_pitch) do differently; everything behind the staging is this one body.
// cand (CAND only): besides, the frame's candidates for the tracker (track.h), as include/sbv2_hip.h states them above sbv2_pitch_track.  Without
// CAND nothing below exists: the body, its LDS and its results are the plain kernel's.
template <class T, int P, class At, bool CAND = false>
__device__ inline void pitch_frame(const At& at, int64_t b, int tau_min, int W, double threshold, double* o, int32_t* o_lag, int32_t* o_voiced,
                                   double cand_max = 0.0, int32_t* o_cand = nullptr, double* o_cand_c3 = nullptr) {
    using S = typename PitchTypes<T>::S;
    using D = typename PitchTypes<T>::D;
    __shared__ S win[2 * kPitchMaxTau];
    __shared__ D dd[kPitchMaxTau + 1];
    __shared__ double cc[kPitchMaxTau + 1];
    __shared__ D part[kBlock];
    __shared__ int sh_first[kWavesPerBlock], sh_arg[kWavesPerBlock];
    __shared__ double sh_min[kWavesPerBlock];
    const int nt = blockDim.x, tid = threadIdx.x;   // nt P >= W (pitch_lanes)
    for (int k = tid; k < 2 * W; k += nt) win[k] = at(b + k);
    __syncthreads();
    int tau[P];
    D acc[P];
#pragma unroll
    for (int p = 0; p < P; ++p) {
        tau[p] = 1 + tid + p * nt;
        if (tau[p] > W) tau[p] = 0;   // a lane without a lag in this round reads inside the window and its sum is dropped
        acc[p] = D(0);
    }
#pragma unroll 4
    for (int j = 0; j < W; ++j) {   // j + tau <= 2 W - 1
        const S v = win[j];
#pragma unroll
        for (int p = 0; p < P; ++p) {
            const S e = v - win[j + tau[p]];   // |e| <= 65535 for the integer encodings
            acc[p] += (D)e * (D)e;
        }
    }
#pragma unroll
    for (int p = 0; p < P; ++p)
        if (tau[p]) dd[tau[p]] = acc[p];
    __syncthreads();
    // S(tau): thread t owns the lags [lo, hi], K consecutive ones
    const int K = (W + nt - 1) / nt, lo = 1 + tid * K, hi = min(lo + K - 1, W);
    D run = D(0);
    for (int t = lo; t <= hi; ++t) run += dd[t];
    part[tid] = run;
    __syncthreads();
    if (tid == 0) {
        D before = D(0);
        for (int t = 0; t < nt; ++t) {
            const D v = part[t];
            part[t] = before;
            before += v;
        }
    }
    __syncthreads();
    run = part[tid];
    int first = INT_MAX, arg = INT_MAX;   // the smallest lag in range under the threshold; the smallest lag in range that attains min c
    double cmin = INFINITY;
    for (int t = lo; t <= hi; ++t) {
        const D d = dd[t];
        run += d;
        const double c = run == D(0) ? 1.0 : (double)d * (double)t / (double)run;   // both exact below 2^53 for integers: one rounding
        cc[t] = c;
        if (t >= tau_min) {
            if (c < threshold && first == INT_MAX) first = t;
            if (c < cmin) cmin = c, arg = t;
        }
    }
#pragma unroll
    for (int s = kWave / 2; s >= 1; s >>= 1) {
        first = min(first, __shfl_down(first, s, kWave));
        const double oc = __shfl_down(cmin, s, kWave);
        const int oa = __shfl_down(arg, s, kWave);
        if (oc < cmin || (oc == cmin && oa < arg)) cmin = oc, arg = oa;
    }
    const int lane = tid & (kWave - 1), wave = tid / kWave;
    if (lane == 0) sh_first[wave] = first, sh_min[wave] = cmin, sh_arg[wave] = arg;
    __syncthreads();   // (also: every cc[] is written)
    if (tid == 0) {
        for (int w = 1; w < nt / kWave; ++w) {
            first = min(first, sh_first[w]);
            if (sh_min[w] < cmin || (sh_min[w] == cmin && sh_arg[w] < arg)) cmin = sh_min[w], arg = sh_arg[w];
        }
        const bool voiced = first != INT_MAX;
        int lag = voiced ? first : arg != INT_MAX ? arg : tau_min;   // (no minimum: every c is a NaN, from non-finite f32 samples)
        if (voiced)
            while (lag + 1 <= W && cc[lag + 1] < cc[lag]) ++lag;
        const double c0 = cc[lag];
        o[0] = lag - 1 >= 1 ? cc[lag - 1] : c0;
        o[1] = c0;
        o[2] = lag + 1 <= W ? cc[lag + 1] : c0;
        *o_lag = lag;
        *o_voiced = voiced;
    }
    if constexpr (CAND) {
        // The dips among this thread's lags [lo, hi] (every cc[] is complete).  Round r takes the smallest (c, tau) above round r - 1's pick:
        // nothing is marked, a thread looks at its few lags again.  The index minimum is the one of `arg` above, with every lane given the result.
        __shared__ double sh_cc[kWavesPerBlock];
        __shared__ int sh_ct[kWavesPerBlock];
        __shared__ int sh_pick[kTrackCand];
        double last_c = -1.0;
        int last_t = 0, npick = 0;
        for (int r = 0; r < kTrackCand; ++r) {
            double bc = INFINITY;
            int bt = INT_MAX;
            for (int t = max(lo, max(tau_min, 2)); t <= hi; ++t) {   // (c(tau - 1) exists)
                const double c = cc[t];
                const bool dip = c < cc[t - 1] && (t + 1 > W || c <= cc[t + 1]) && c < cand_max;
                if (dip && (c > last_c || (c == last_c && t > last_t)) && (c < bc || (c == bc && t < bt))) bc = c, bt = t;
            }
#pragma unroll
            for (int s = kWave / 2; s >= 1; s >>= 1) {
                const double oc = __shfl_xor(bc, s, kWave);
                const int ot = __shfl_xor(bt, s, kWave);
                if (oc < bc || (oc == bc && ot < bt)) bc = oc, bt = ot;
            }
            if (lane == 0) sh_cc[wave] = bc, sh_ct[wave] = bt;
            __syncthreads();
            for (int w = 0; w < nt / kWave; ++w)
                if (sh_cc[w] < bc || (sh_cc[w] == bc && sh_ct[w] < bt)) bc = sh_cc[w], bt = sh_ct[w];
            __syncthreads();   // (the next round writes sh_cc / sh_ct again)
            if (bt == INT_MAX) break;   // (uniform) no dip is left
            if (tid == 0) sh_pick[r] = bt;
            last_c = bc;
            last_t = bt;
            npick = r + 1;
        }
        if (tid == 0) {   // (its own writes to sh_pick) the picks in ascending tau
            int pick[kTrackCand];
            for (int i = 0; i < npick; ++i) {
                const int t = sh_pick[i];
                int k = i;
                for (; k > 0 && pick[k - 1] > t; --k) pick[k] = pick[k - 1];
                pick[k] = t;
            }
            o_cand[0] = npick;
            for (int i = 0; i < kTrackCand; ++i) {
                const int t = i < npick ? pick[i] : 0;
                const double c0 = i < npick ? cc[t] : 0.0;
                o_cand[1 + i] = t;
                o_cand[1 + kTrackCand + i] = i < npick ? (int32_t)llrint(c0 * 65536.0) : 0;
                o_cand_c3[3 * i] = i < npick ? (t - 1 >= 1 ? cc[t - 1] : c0) : 0.0;
                o_cand_c3[3 * i + 1] = c0;
                o_cand_c3[3 * i + 2] = i < npick ? (t + 1 <= W ? cc[t + 1] : c0) : 0.0;
            }
        }
    }
}

template <class T, int P>
__global__ __launch_bounds__(kBlock) void k_pitch_yin(const PitchArgs a) {
    using S = typename PitchTypes<T>::S;
    const T* x = static_cast<const T*>(a.x);
    const int64_t n = a.n;
    const auto at = [x, n](int64_t i) -> S { return i >= 0 && i < n ? static_cast<S>(level_load(x, i)) : S(0); };
    const int64_t f = blockIdx.x;
    pitch_frame<T, P>(at, f * a.hop + a.hop / 2 - a.tau_max, a.tau_min, a.tau_max, a.threshold, a.c3 + 3 * f, a.lag + f, a.voiced + f);
}

// k_pitch_yin with the candidate record of every frame besides (cand [nf][15] = ncand, 7 tau, 7 q; cand_c3 [nf][7][3])
struct PitchCandArgs {
    PitchArgs a;
    double cand_max;
    int32_t* cand;
    double* cand_c3;
};
template <class T, int P>
__global__ __launch_bounds__(kBlock) void k_pitch_yin_cand(const PitchCandArgs ca) {
    using S = typename PitchTypes<T>::S;
    const PitchArgs& a = ca.a;
    const T* x = static_cast<const T*>(a.x);
    const int64_t n = a.n;
    const auto at = [x, n](int64_t i) -> S { return i >= 0 && i < n ? static_cast<S>(level_load(x, i)) : S(0); };
    const int64_t f = blockIdx.x;
    pitch_frame<T, P, decltype(at), true>(at, f * a.hop + a.hop / 2 - a.tau_max, a.tau_min, a.tau_max, a.threshold, a.c3 + 3 * f, a.lag + f,
                                          a.voiced + f, ca.cand_max, ca.cand + kTrackRec * f, ca.cand_c3 + 3 * kTrackCand * f);
}

// The fed estimator (StreamPitch, marks.h): the workgroups [0, count) take the frames first, first + 1, ... that this push completed, the
// workgroups behind them write the next carry.  A frame's window lies in [d0 - cl, d1): positions below d0 come from the carry (the cl
// samples before d0, in the sample's own type), the rest from x (the sample at d0 onwards); nothing outside carry_in[0, cl) and x[0, d1 - d0)
// is addressed, whatever the arguments.
struct StreamPitchArgs {
    const void* x;
    const void* carry_in;   // positions [d0 - cl, d0)
    void* carry_out;        // positions [d1 - cl_out, d1)
    int64_t d0, d1, total, hop, first;
    int32_t count, cl, cl_out;
    int32_t tau_min, tau_max;
    double threshold;
    PitchFrame* res;        // [nf]
};

template <class T, int P>
__global__ __launch_bounds__(kBlock) void k_stream_pitch(const StreamPitchArgs a) {
    using S = typename PitchTypes<T>::S;
    const T* x = static_cast<const T*>(a.x);
    const T* cin = static_cast<const T*>(a.carry_in);
    const int64_t d0 = a.d0, d1 = a.d1, c0 = a.d0 - a.cl;
    if ((int)blockIdx.x >= a.count) {   // the carry: a push shorter than it keeps the end of the old one in front of x (uniform: no barrier here)
        T* cout = static_cast<T*>(a.carry_out);
        const int j = ((int)blockIdx.x - a.count) * (int)blockDim.x + (int)threadIdx.x;
        if (j >= a.cl_out) return;
        const int64_t i = d1 - a.cl_out + j;
        if (i >= d0) cout[j] = x[i - d0];
        else if (i >= c0) cout[j] = cin[i - c0];
        return;
    }
    const int64_t total = a.total;
    const auto at = [x, cin, d0, d1, c0, total](int64_t i) -> S {
        if (i < 0 || i >= total) return S(0);
        if (i >= d0) return i < d1 ? static_cast<S>(level_load(x, i - d0)) : S(0);
        return i >= c0 ? static_cast<S>(level_load(cin, i - c0)) : S(0);
    };
    const int64_t f = a.first + (int)blockIdx.x;
    PitchFrame* r = a.res + f;
    pitch_frame<T, P>(at, f * a.hop + a.hop / 2 - a.tau_max, a.tau_min, a.tau_max, a.threshold, r->c3, &r->lag, &r->voiced);
}

#define SBV2_PITCH_LAUNCH(KERNEL)                                                             \
    static_assert(kPitchMaxP == 5, "one case per lag count");                                 \
    switch (P) {                                                                              \
        case 1: hipLaunchKernelGGL((KERNEL<T, 1>), grid, blk, 0, s, a); break;                \
        case 2: hipLaunchKernelGGL((KERNEL<T, 2>), grid, blk, 0, s, a); break;                \
        case 3: hipLaunchKernelGGL((KERNEL<T, 3>), grid, blk, 0, s, a); break;                \
        case 4: hipLaunchKernelGGL((KERNEL<T, 4>), grid, blk, 0, s, a); break;                \
        default: hipLaunchKernelGGL((KERNEL<T, 5>), grid, blk, 0, s, a); break;               \
    }
template <class T>
void launch_pitch(int P, dim3 grid, dim3 blk, hipStream_t s, const PitchArgs& a) {
    SBV2_PITCH_LAUNCH(k_pitch_yin)
}
template <class T>
void launch_pitch_cand(int P, dim3 grid, dim3 blk, hipStream_t s, const PitchCandArgs& a) {
    SBV2_PITCH_LAUNCH(k_pitch_yin_cand)
}
template <class T>
void launch_stream_pitch(int P, dim3 grid, dim3 blk, hipStream_t s, const StreamPitchArgs& a) {
    SBV2_PITCH_LAUNCH(k_stream_pitch)
}
#undef SBV2_PITCH_LAUNCH

// a small window (8 or 16 kHz) takes one or two waves per frame instead of four; a large one several lags per lane
inline int pitch_lanes(int tau_max) { return tau_max <= kWave ? kWave : tau_max <= 2 * kWave ? 2 * kWave : kBlock; }

}  // namespace

PitchSpec pitch_spec(int sample_rate, int64_t hop, double f0_min, double f0_max, double threshold) {
    SBV2_REQUIRE(sample_rate > 0 && sample_rate <= kPitchMaxRate,
                 "pitch: sample rate must be in [1, " + std::to_string(kPitchMaxRate) + "]: " + std::to_string(sample_rate));
    SBV2_REQUIRE(hop >= 1, "pitch: hop must be >= 1: " + std::to_string(hop));
    SBV2_REQUIRE(f0_min >= kPitchMinF0, "pitch: f0_min must be >= 40 Hz (the window of tau_max samples stays within " + std::to_string(kPitchMaxTau) +
                                            ", the bound that keeps integer samples exact): " + std::to_string(f0_min));
    SBV2_REQUIRE(f0_min < f0_max, "pitch: f0_min must be below f0_max: " + std::to_string(f0_min) + " >= " + std::to_string(f0_max));
    SBV2_REQUIRE(f0_max <= sample_rate / 4.0,
                 "pitch: f0_max must be <= sample_rate / 4 = " + std::to_string(sample_rate / 4.0) + ": " + std::to_string(f0_max));
    SBV2_REQUIRE(threshold > 0.0 && threshold < 1.0, "pitch: threshold must be in (0, 1): " + std::to_string(threshold));
    PitchSpec sp;
    sp.sample_rate = sample_rate;
    sp.hop = hop;
    sp.tau_min = (int)std::floor(sample_rate / f0_max);
    sp.tau_max = (int)std::ceil(sample_rate / f0_min);
    sp.threshold = threshold;
    SBV2_REQUIRE(sp.tau_min >= 4 && sp.tau_min <= sp.tau_max && sp.tau_max <= kPitchMaxTau, "internal: pitch lags out of range");
    return sp;
}

void pitch_finish(const PitchSpec& sp, int32_t lag, int32_t voiced, const double* c3, double* f0, double* ap) {
#pragma clang fp contract(off)
    const double cm = c3[0], c0 = c3[1], cp = c3[2];
    const double den = cm - 2.0 * c0 + cp;
    const bool both = lag - 1 >= 1 && lag + 1 <= sp.tau_max;
    const double delta = den > 0.0 && both ? 0.5 * (cm - cp) / den : 0.0;
    *f0 = voiced ? (double)sp.sample_rate / ((double)lag + delta) : 0.0;
    if (ap) *ap = c0;
}

void pitch_launch(const void* x, int encoding, int64_t n, const PitchSpec& sp, double* c3, int32_t* lag, int32_t* voiced, hipStream_t s,
                  double cand_max, int32_t* cand, double* cand_c3) {
    SBV2_REQUIRE(pcm_encoding_known(encoding), "internal: pitch of an unknown encoding");
    SBV2_REQUIRE(n >= 0 && sp.hop >= 1 && sp.tau_min >= 1 && sp.tau_min <= sp.tau_max && sp.tau_max <= kPitchMaxTau, "internal: bad pitch spec");
    const int64_t nf = pitch_frames(n, sp.hop);
    SBV2_REQUIRE(nf < (1 << 30), "too many pitch frames: " + std::to_string(nf) + " >= 2^30");
    if (nf == 0) return;
    SBV2_REQUIRE(x && c3 && lag && voiced, "internal: no samples");
    PitchArgs a;
    a.x = x;
    a.n = n;
    a.hop = sp.hop;
    a.tau_min = sp.tau_min;
    a.tau_max = sp.tau_max;
    a.threshold = sp.threshold;
    a.c3 = c3;
    a.lag = lag;
    a.voiced = voiced;
    const int nt = pitch_lanes(sp.tau_max), P = (sp.tau_max + nt - 1) / nt;
    const dim3 grid((unsigned)nf), blk(nt);
    if (cand) {   // the same frames with their candidates besides
        SBV2_REQUIRE(cand_c3 && cand_max > 0.0 && cand_max <= 1.0, "internal: bad candidate output");
        const PitchCandArgs ca{a, cand_max, cand, cand_c3};
        if (encoding == kEncS16) launch_pitch_cand<int16_t>(P, grid, blk, s, ca);
        else if (encoding == kEncMulaw) launch_pitch_cand<MulawCode>(P, grid, blk, s, ca);
        else if (encoding == kEncAlaw) launch_pitch_cand<AlawCode>(P, grid, blk, s, ca);
        else launch_pitch_cand<float>(P, grid, blk, s, ca);
        HIP_CHECK(hipGetLastError());
        return;
    }
    if (encoding == kEncS16) launch_pitch<int16_t>(P, grid, blk, s, a);
    else if (encoding == kEncMulaw) launch_pitch<MulawCode>(P, grid, blk, s, a);
    else if (encoding == kEncAlaw) launch_pitch<AlawCode>(P, grid, blk, s, a);
    else launch_pitch<float>(P, grid, blk, s, a);
    HIP_CHECK(hipGetLastError());
}

void Pitch::run(const void* x, int encoding, int64_t n, const PitchSpec& sp, hipStream_t s, const TrackSpec* tr, Track* tk) {
    SBV2_REQUIRE(n >= 0 && sp.hop >= 1, "internal: bad pitch spec");
    SBV2_REQUIRE(!tr == !tk, "internal: a tracked contour needs the tracker's state");
    const int64_t nf = pitch_frames(n, sp.hop);
    SBV2_REQUIRE(nf < (1 << 30), "too many pitch frames: " + std::to_string(nf) + " >= 2^30");
    nf_ = nf;
    if (nf == 0) return;
    const size_t bytes = 32 * (size_t)nf;   // c3 (24) | lag (4) | voiced (4) per frame
    // tracked: behind them, on the device only, the candidates' c3 (168) | their records (60) per frame
    const size_t d_bytes = bytes + (tr ? (24 * kTrackCand + 4 * kTrackRec) * (size_t)nf : 0);
    char* h = static_cast<char*>(host_.reserve(bytes, std::max<size_t>(bytes * 2, 4096), s));
    char* d = static_cast<char*>(dev_.reserve(d_bytes, std::max<size_t>(d_bytes * 2, 4096), s));
    double* c3 = reinterpret_cast<double*>(d);
    int32_t* lag = reinterpret_cast<int32_t*>(d + 24 * (size_t)nf);
    if (tr) {
        double* cand_c3 = reinterpret_cast<double*>(d + bytes);
        int32_t* cand = reinterpret_cast<int32_t*>(d + bytes + 24 * kTrackCand * (size_t)nf);
        pitch_launch(x, encoding, n, sp, c3, lag, lag + nf, s, tr->cand_max, cand, cand_c3);
        tk->run(cand, cand_c3, nf, *tr, c3, lag, lag + nf, s);
    } else {
        pitch_launch(x, encoding, n, sp, c3, lag, lag + nf, s);
    }
    HIP_CHECK(hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, s));
}

// ---- the fed estimator (StreamPitch, marks.h) ----
void StreamPitch::check(const PitchSpec& sp, int64_t total) {
    SBV2_REQUIRE(total >= 0 && sp.hop >= 1 && sp.tau_min >= 1 && sp.tau_min <= sp.tau_max && sp.tau_max <= kPitchMaxTau, "internal: bad pitch spec");
    const int64_t nf = pitch_frames(total, sp.hop);
    SBV2_REQUIRE(nf < (1 << 30), "too many pitch frames: " + std::to_string(nf) + " >= 2^30");
}

int64_t pitch_frames_complete(const PitchSpec& sp, int64_t total, int64_t D) {
    const int64_t nf = pitch_frames(total, sp.hop);
    if (nf == 0 || D >= total) return nf;
    const int64_t r = D - sp.tau_max - sp.hop / 2;   // frame f: f hop + hop / 2 + tau_max <= D
    return r < 0 ? 0 : std::min(nf, r / sp.hop + 1);
}

int64_t StreamPitch::complete(int64_t D) const { return pitch_frames_complete(sp_, total_, D); }

void pitch_launch_fed(const float* x, int64_t fed, int64_t total, const PitchSpec& sp, int64_t first, int64_t count, PitchFrame* res, hipStream_t s) {
    SBV2_REQUIRE(fed >= 0 && fed <= total && sp.hop >= 1 && sp.tau_min >= 1 && sp.tau_min <= sp.tau_max && sp.tau_max <= kPitchMaxTau,
                 "internal: bad pitch spec");
    SBV2_REQUIRE(first >= 0 && count >= 0 && first + count <= pitch_frames_complete(sp, total, fed), "internal: pitch frames that are not complete yet");
    if (count == 0) return;
    SBV2_REQUIRE(x && res, "internal: no samples");
    StreamPitchArgs a{};   // no carry: every fed sample lies at x
    a.x = x;
    a.d0 = 0;
    a.d1 = fed;
    a.total = total;
    a.hop = sp.hop;
    a.first = first;
    a.count = (int32_t)count;
    a.tau_min = sp.tau_min;
    a.tau_max = sp.tau_max;
    a.threshold = sp.threshold;
    a.res = res;
    const int nt = pitch_lanes(sp.tau_max), P = (sp.tau_max + nt - 1) / nt;
    launch_stream_pitch<float>(P, dim3((unsigned)count), dim3(nt), s, a);
    HIP_CHECK(hipGetLastError());
}

void StreamPitch::begin(const PitchSpec& sp, int encoding, int64_t total, hipStream_t s) {
    SBV2_REQUIRE(pcm_encoding_known(encoding), "internal: pitch of an unknown encoding");
    check(sp, total);
    sp_ = sp;
    encoding_ = encoding;
    total_ = total;
    nf_ = pitch_frames(total, sp.hop);
    fed_ = done_ = 0;
    parity_ = 0;
    // device: carry (two copies, each 2 kPitchMaxTau elements of the widest sample type) | results; pinned: the results
    const size_t o_res = 2 * kCarryBytes, bytes = o_res + sizeof(PitchFrame) * (size_t)nf_, h_bytes = sizeof(PitchFrame) * (size_t)nf_;
    char* d = static_cast<char*>(dev_.reserve(bytes, std::max<size_t>(bytes * 2, 32768), s));
    char* h = static_cast<char*>(host_.reserve(std::max<size_t>(h_bytes, 64), std::max<size_t>(h_bytes * 2, 4096), s));
    HIP_CHECK(hipStreamSynchronize(s));   // (an earlier stream's copies into the mirror are done)
    d_carry_ = d;
    d_res_ = reinterpret_cast<PitchFrame*>(d + o_res);
    res_host_ = reinterpret_cast<PitchFrame*>(h);
    HIP_CHECK(hipMemsetAsync(d_carry_, 0, 2 * kCarryBytes, s));
}

int64_t StreamPitch::push(const void* x, int64_t D0, int64_t n, hipStream_t s) {
    SBV2_REQUIRE(n >= 0 && D0 == fed_ && D0 + n <= total_, "internal: a pitch push of [" + std::to_string(D0) + ", " + std::to_string(D0 + n) +
                                                               ") out of stream order (" + std::to_string(fed_) + " of " + std::to_string(total_) + " fed)");
    const int64_t D1 = D0 + n, now = complete(D1), done = now - done_;
    fed_ = D1;
    if (n > 0) {
        SBV2_REQUIRE(x, "internal: no samples to push");
        const int64_t keep = 2 * (int64_t)sp_.tau_max;
        StreamPitchArgs a{};
        a.x = x;
        a.carry_in = d_carry_ + (size_t)parity_ * kCarryBytes;
        a.carry_out = d_carry_ + (size_t)(parity_ ^ 1) * kCarryBytes;
        a.d0 = D0;
        a.d1 = D1;
        a.total = total_;
        a.hop = sp_.hop;
        a.first = done_;
        a.count = (int32_t)done;
        a.cl = (int32_t)std::min(D0, keep);
        a.cl_out = (int32_t)std::min(D1, keep);
        a.tau_min = sp_.tau_min;
        a.tau_max = sp_.tau_max;
        a.threshold = sp_.threshold;
        a.res = d_res_;
        const int nt = pitch_lanes(sp_.tau_max), P = (sp_.tau_max + nt - 1) / nt;
        const dim3 grid((unsigned)(done + (a.cl_out + nt - 1) / nt)), blk(nt);
        if (encoding_ == kEncS16) launch_stream_pitch<int16_t>(P, grid, blk, s, a);
        else if (encoding_ == kEncMulaw) launch_stream_pitch<MulawCode>(P, grid, blk, s, a);
        else if (encoding_ == kEncAlaw) launch_stream_pitch<AlawCode>(P, grid, blk, s, a);
        else launch_stream_pitch<float>(P, grid, blk, s, a);
        HIP_CHECK(hipGetLastError());
        parity_ ^= 1;
        if (done) HIP_CHECK(hipMemcpyAsync(res_host_ + done_, d_res_ + done_, sizeof(PitchFrame) * (size_t)done, hipMemcpyDeviceToHost, s));
    }
    done_ = now;
    return done;
}

}  // namespace sbv2
