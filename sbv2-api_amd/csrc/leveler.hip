// Loudness follower of a stream on the device (leveler.h; the convention is the header comment of struct sbv2_stream_leveler,
// include/sbv2_hip.h).  All of it in f64, no atomics, every sum in an order that depends on sample, segment and block indices alone, so the
// delivered samples and the gain schedule do not depend on how the stream is cut into pushes.
//
// The meter is loudness.hip's: the K-weighting cascade as a linear recurrence over segments of m samples (kweight.h), st_{s+1} = A^m st_s + e_s.
// A whole signal lets the meter scan the segments' maps in a tree; a stream cannot (the tree's shape would move with the cuts), so the states
// are folded one after the other from the carried one, by ONE wavefront: 16 dependent fused multiply-adds per segment and nothing else on the
// chain (the zero-start end states are staged through LDS 64 segments at a time, so no global load waits on the recurrence).
// Per push, on the stream, with no host wait:
//   k_lvl_zero      one lane per segment the push completes runs from zero state and writes e; the first segment starts with the carried
//                   samples of the previous pushes (at most m - 1), the others lie in the push alone;
//   k_lvl_fold      one wavefront: every segment's true start state from the carried state, which it moves on;
//   k_lvl_rerun     one lane per segment from its true start: the sum of w^2 in sample order, behind the carried partials of the open quarter;
//   k_lvl_schedule  one workgroup, for each quarter the push completes, in order: E_k from its S / m partials, z_j into the block history, both
//                   gates over the history (lane t takes blocks t, t + 256, ... in ascending order, then a fixed tree over the lanes), g_{k+1}
//                   and a_{k+1}, the running stats; at the end the partials of the quarter left open go to the front;
//   k_lvl_apply     one thread per sample: the ramp between a_{k-1} and a_k in place, and the samples of the segment left open into the tail.
// A push that completes no segment launches the last one only; one that completes no quarter leaves the schedule out.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "../../include/sbv2_hip.h"
#include "kweight.h"
#include "leveler.h"

namespace sbv2 {

namespace {

// the carried doubles: the filter state at the start of the next segment, E of the last three quarters, then the stats
enum { kCarryState = 0, kCarryE = 4, kCarryL = 7, kCarryG = 8, kCarryGmin = 9, kCarryGmax = 10, kCarryNabs = 11, kCarryWords = 16 };
constexpr int kMaxSeg = 245;   // the longest segment (loudness_segment_len)

struct MeterArgs {
    const double* y;      // the push's n samples
    const double* tail;   // the r samples carried in front of them
    int r, m, pc;         // pc: partials of the open quarter in front of this push's
    int64_t nseg;         // segments the push completes
    double c[10];
    double A[16];         // A^m, row-major
    double* e;            // [nseg][4]
    double* st;           // [nseg][4]
    double* part;         // [pc + nseg]
    double* carry;
};

// runs segment k of [tail | y] through the cascade from state s; returns sum w^2 in sample order.  Five samples are loaded ahead of use (m is
// a multiple of 5 at every rate): a lane's stream is serial, so the loads must not wait on the recurrence.  Only segment 0 reads the tail.
__device__ __forceinline__ double lvl_run(const MeterArgs& a, int64_t k, double* s) {
    double acc = 0.0;
    if (k == 0 && a.r > 0) {
        for (int i = 0; i < a.m; i += 5) {
            double v[5];
#pragma unroll
            for (int q = 0; q < 5; ++q) {
                const int j = i + q;
                const double* p = j < a.r ? a.tail + j : a.y + (j - a.r);
                v[q] = *p;
            }
#pragma unroll
            for (int q = 0; q < 5; ++q) {
                const double w = kw_step(a.c, s, v[q]);
                acc = fma(w, w, acc);
            }
        }
        return acc;
    }
    const double* x = a.y + (k * a.m - a.r);
    for (int i = 0; i < a.m; i += 5) {
        double v[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) v[q] = x[i + q];
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            const double w = kw_step(a.c, s, v[q]);
            acc = fma(w, w, acc);
        }
    }
    return acc;
}

__global__ __launch_bounds__(256) void k_lvl_zero(MeterArgs a) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= a.nseg) return;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    lvl_run(a, k, s);
    for (int i = 0; i < 4; ++i) a.e[4 * k + i] = s[i];
}

__global__ __launch_bounds__(64) void k_lvl_fold(MeterArgs a) {
    __shared__ double se[64 * 4], ss[64 * 4];
    const int lane = threadIdx.x;
    double s[4];   // (every lane holds the same state: the LDS reads below are broadcasts)
    for (int i = 0; i < 4; ++i) s[i] = a.carry[kCarryState + i];
    for (int64_t base = 0; base < a.nseg; base += 64) {
        const int cnt = (int)min((int64_t)64, a.nseg - base);
        for (int i = lane; i < 4 * cnt; i += 64) se[i] = a.e[4 * base + i];
        __syncthreads();
        for (int j = 0; j < cnt; ++j) {
            if (lane == 0)
                for (int i = 0; i < 4; ++i) ss[4 * j + i] = s[i];
            kw_matvec(a.A, s, se + 4 * j, s);
        }
        __syncthreads();
        for (int i = lane; i < 4 * cnt; i += 64) a.st[4 * base + i] = ss[i];
        __syncthreads();
    }
    if (lane == 0)
        for (int i = 0; i < 4; ++i) a.carry[kCarryState + i] = s[i];
}

__global__ __launch_bounds__(256) void k_lvl_rerun(MeterArgs a) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= a.nseg) return;
    double s[4];
    for (int i = 0; i < 4; ++i) s[i] = a.st[4 * k + i];
    a.part[a.pc + k] = lvl_run(a, k, s);
}

struct SchedArgs {
    double* part;      // [nq qs + rem]: the partials of the quarters this push completes, then those of the one left open
    int qs, rem, S, hold;
    int64_t nq, k0;    // quarters k0 .. k0 + nq - 1 complete
    double target, lo, hi, step;
    double* carry;
    double* hist;      // z_j at [j - 3]
    double* g;
    double* a;
};

// sum of v over the workgroup in a fixed order (a tree over the lanes' values); every lane gets the result
__device__ double lvl_reduce(double v, double* red) {
    const int t = threadIdx.x;
    __syncthreads();
    red[t] = v;
    __syncthreads();
    for (int h = 128; h >= 1; h >>= 1) {
        if (t < h) red[t] = red[t] + red[t + h];
        __syncthreads();
    }
    return red[0];
}

__device__ __forceinline__ double lvl_lufs(double z) { return -0.691 + 10.0 * log10(z); }

__global__ __launch_bounds__(256) void k_lvl_schedule(SchedArgs a) {
    __shared__ double red[256];
    const int t = threadIdx.x;
    for (int64_t q = 0; q < a.nq; ++q) {
        const int64_t k = a.k0 + q;
        if (t == 0) {
            const double* p = a.part + q * a.qs;
            double E = 0.0;
            for (int i = 0; i < a.qs; ++i) E += p[i];
            double* c = a.carry + kCarryE;   // E_{k-3}, E_{k-2}, E_{k-1}
            if (k >= 3) a.hist[k - 3] = (((c[0] + c[1]) + c[2]) + E) / (4.0 * a.S);
            c[0] = c[1];
            c[1] = c[2];
            c[2] = E;
        }
        __syncthreads();   // (the history's new entry is visible to the workgroup)
        const int64_t nb = k >= 3 ? k - 2 : 0;
        double sum = 0.0, cnt = 0.0;
        for (int64_t j = t; j < nb; j += 256) {
            const double z = a.hist[j];
            if (lvl_lufs(z) > -70.0) {
                sum += z;
                cnt += 1.0;
            }
        }
        sum = lvl_reduce(sum, red);
        const double nabs = lvl_reduce(cnt, red);
        double L = -INFINITY;
        if (nabs > 0.0) {   // (the same in every lane)
            const double gate = lvl_lufs(sum / nabs) - 10.0;
            sum = cnt = 0.0;
            for (int64_t j = t; j < nb; j += 256) {
                const double z = a.hist[j], l = lvl_lufs(z);
                if (l > -70.0 && l > gate) {
                    sum += z;
                    cnt += 1.0;
                }
            }
            sum = lvl_reduce(sum, red);
            cnt = lvl_reduce(cnt, red);
            if (cnt > 0.0) L = lvl_lufs(sum / cnt);
        }
        if (t == 0) {
            const double gp = a.g[k];
            double gn = gp;
            if (nabs >= (double)a.hold && isfinite(L)) {
                const double want = fmin(fmax(a.target - L, a.lo), a.hi);
                gn = gp + fmin(fmax(want - gp, -a.step), a.step);
            }
            a.g[k + 1] = gn;
            a.a[k + 1] = pow(10.0, gn / 20.0);
            a.carry[kCarryL] = L;
            a.carry[kCarryG] = gn;
            a.carry[kCarryGmin] = fmin(a.carry[kCarryGmin], gn);
            a.carry[kCarryGmax] = fmax(a.carry[kCarryGmax], gn);
            a.carry[kCarryNabs] = nabs;
        }
    }
    __syncthreads();
    const double v = t < a.rem ? a.part[a.nq * a.qs + t] : 0.0;
    __syncthreads();
    if (t < a.rem) a.part[t] = v;
}

__global__ void k_lvl_init(double* carry, double* g, double* a, double gain_db) {
    for (int i = 0; i < kCarryWords; ++i) carry[i] = 0.0;
    carry[kCarryL] = -INFINITY;
    carry[kCarryG] = carry[kCarryGmin] = carry[kCarryGmax] = gain_db;
    g[0] = gain_db;
    a[0] = pow(10.0, gain_db / 20.0);
}

struct ApplyArgs {
    double* y;
    int64_t n, fed;   // the push's samples are [fed, fed + n) of the stream
    int S, r, m;
    int64_t keep;     // the push's samples from keep on stay unmetered: they go to the tail
    const double* a;
    double* tail;
};

__global__ __launch_bounds__(256) void k_lvl_apply(ApplyArgs p) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= p.n) return;
    const int64_t pos = p.fed + i, k = pos / p.S;
    const int ii = (int)(pos - k * p.S);
    const double a1 = p.a[k], a0 = p.a[k > 0 ? k - 1 : 0];
    const double yv = p.y[i];
    if (i >= p.keep) p.tail[(p.keep == 0 ? p.r : 0) + (i - p.keep)] = yv;   // (keep == 0: no segment completed, the carried samples stay in front)
    p.y[i] = yv * (a0 + (a1 - a0) * (double)(ii + 1) / (double)p.S);
}

}  // namespace

StreamLevelerSpec stream_leveler_spec(const sbv2_stream_leveler* lv) {
    SBV2_REQUIRE(lv, "no stream leveler given");
    SBV2_REQUIRE(std::isfinite(lv->target_lufs) && lv->target_lufs >= -70.0 && lv->target_lufs <= -5.0,
                 "leveler target " + std::to_string(lv->target_lufs) + " LUFS is outside [-70, -5]");
    SBV2_REQUIRE(std::isfinite(lv->range_db) && lv->range_db >= 0.0 && lv->range_db <= 20.0,
                 "leveler range " + std::to_string(lv->range_db) + " dB is outside [0, 20]");
    SBV2_REQUIRE(std::isfinite(lv->slew_db_per_s) && lv->slew_db_per_s > 0.0 && lv->slew_db_per_s <= 20.0,
                 "leveler slew " + std::to_string(lv->slew_db_per_s) + " dB/s is outside (0, 20]");
    SBV2_REQUIRE(lv->hold_blocks >= 1 && lv->hold_blocks <= 100, "leveler hold of " + std::to_string(lv->hold_blocks) + " blocks is outside [1, 100]");
    SBV2_REQUIRE(lv->reserved == 0, "sbv2_stream_leveler.reserved must be 0");
    StreamLevelerSpec s;
    s.target = lv->target_lufs;
    s.range = lv->range_db;
    s.slew = lv->slew_db_per_s;
    s.hold = lv->hold_blocks;
    return s;
}

void StreamLeveler::begin(int rate, int64_t total_samples, int64_t max_push, const StreamLevelerSpec& spec, double gain_db, hipStream_t s) {
    kw_table(rate, tab_);   // refuses unsupported rates
    SBV2_REQUIRE(total_samples >= 0 && max_push >= 0, "stream leveler: length out of range");
    rate_ = rate;
    m_ = loudness_segment_len(rate);
    S_ = rate / 10;
    SBV2_REQUIRE(m_ <= kMaxSeg && m_ % 5 == 0 && S_ % m_ == 0, "internal: the leveler's segment length");
    spec_ = spec;
    gain_db_ = gain_db;
    total_ = total_samples;
    max_push_ = max_push;
    fed_ = 0;
    done_ = false;
    // a push completes at most segcap segments ((m - 1 carried + max_push) / m); the partials of the open quarter (< S / m) lie in front of them
    const int64_t segcap = (max_push + m_ - 1) / m_ + 1, qs = S_ / m_;
    nq_cap_ = total_samples / S_ + 2;   // g_k, a_k for k = 0 .. total / S; z_j for j - 3 < total / S
    const int64_t o_tail = kCarryWords, o_part = o_tail + round_up64(kMaxSeg, 8), o_e = o_part + round_up64(qs + segcap, 8), o_st = o_e + 4 * segcap,
                  o_hist = o_st + 4 * segcap, o_g = o_hist + round_up64(nq_cap_, 8), o_a = o_g + round_up64(nq_cap_, 8),
                  words = o_a + round_up64(nq_cap_, 8);
    double* d = static_cast<double*>(dev_.reserve(sizeof(double) * (size_t)words, s));
    carry_ = d;
    tail_ = d + o_tail;
    part_ = d + o_part;
    e_ = d + o_e;
    st_ = d + o_st;
    hist_ = d + o_hist;
    g_ = d + o_g;
    a_ = d + o_a;
    host_.reserve(64, s);
    hipLaunchKernelGGL(k_lvl_init, dim3(1), dim3(1), 0, s, carry_, g_, a_, gain_db);
    HIP_CHECK(hipGetLastError());
}

void StreamLeveler::push(double* y, int64_t n, bool last, hipStream_t s) {
    SBV2_REQUIRE(m_ > 0 && !done_, "stream leveler: push without begin, or after the last push");
    SBV2_REQUIRE(n >= 0 && n <= max_push_ && fed_ + n <= total_, "stream leveler: push of " + std::to_string(n) + " samples outgrows what begin announced");
    SBV2_REQUIRE(!last || fed_ + n == total_, "stream leveler: the last push ends " + std::to_string(total_ - fed_ - n) + " samples short of the announced length");
    SBV2_REQUIRE(n == 0 || y, "stream leveler: no samples");
    const int qs = S_ / m_, r = (int)(fed_ % m_), pc = (int)((fed_ / m_) % qs);
    const int64_t nseg = (r + n) / m_, nq = (pc + nseg) / qs;
    if (nseg > 0) {
        MeterArgs a;
        a.y = y;
        a.tail = tail_;
        a.r = r;
        a.m = m_;
        a.pc = pc;
        a.nseg = nseg;
        std::memcpy(a.c, tab_, sizeof(a.c));
        std::memcpy(a.A, tab_ + 10, sizeof(a.A));
        a.e = e_;
        a.st = st_;
        a.part = part_;
        a.carry = carry_;
        const dim3 sg((unsigned)((nseg + 255) / 256)), blk(256);
        hipLaunchKernelGGL(k_lvl_zero, sg, blk, 0, s, a);
        hipLaunchKernelGGL(k_lvl_fold, dim3(1), dim3(64), 0, s, a);
        hipLaunchKernelGGL(k_lvl_rerun, sg, blk, 0, s, a);
    }
    if (nq > 0) {
        SchedArgs c;
        c.part = part_;
        c.qs = qs;
        c.rem = (int)((pc + nseg) % qs);
        c.S = S_;
        c.hold = spec_.hold;
        c.nq = nq;
        c.k0 = fed_ / S_;
        c.target = spec_.target;
        c.lo = gain_db_ - spec_.range;
        c.hi = gain_db_ + spec_.range;
        c.step = spec_.slew / 10.0;
        c.carry = carry_;
        c.hist = hist_;
        c.g = g_;
        c.a = a_;
        SBV2_REQUIRE(c.k0 + nq + 1 <= nq_cap_, "internal: the leveler's schedule outgrows its history");
        hipLaunchKernelGGL(k_lvl_schedule, dim3(1), dim3(256), 0, s, c);
    }
    if (n > 0) {
        ApplyArgs p;
        p.y = y;
        p.n = n;
        p.fed = fed_;
        p.S = S_;
        p.r = r;
        p.m = m_;
        p.keep = nseg > 0 ? nseg * m_ - r : 0;
        p.a = a_;
        p.tail = tail_;
        hipLaunchKernelGGL(k_lvl_apply, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, p);
    }
    HIP_CHECK(hipGetLastError());
    fed_ += n;
    if (last) {
        HIP_CHECK(hipMemcpyAsync(host_.get(), carry_ + kCarryL, 4 * sizeof(double), hipMemcpyDeviceToHost, s));
        done_ = true;
    }
}

void StreamLeveler::stats(double* out) const {
    SBV2_REQUIRE(done_, "stream leveler: the stats exist once the last push has been made");
    std::memcpy(out, host_.get(), 4 * sizeof(double));
}

}  // namespace sbv2
