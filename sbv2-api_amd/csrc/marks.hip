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
#include "marks.h"

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

}  // namespace sbv2
