// The formant tracker: one best path through the kept roots of the formant contour on gfx950, as include/sbv2_hip.h states it above
// sbv2_formant_track.  All of it is integer arithmetic, so the path equals a sequential restatement bit for bit.
//
// k_ftrack_path is bound by latency and by one wave's issue rate, as k_track_path is, but the problem has another shape.  The pitch tracker has
// 8 scalar states per frame and spends its 64 lanes on the 8 x 8 state PAIRS.  Here a state is a strictly increasing T-tuple over the frame's m
// candidates, up to C(7, 4) = 35 of them and 35 x 35 = 1225 transitions per frame: pairs do not fit the wave.  What does fit is that the
// transition cost is a SUM OVER TRACKS of a per-candidate-pair jump cost, so a frame needs only an m_prev x m_cur table (<= 49 entries).
//   * Side by side: a frame with fewer than T candidates (a "cut") has no state, so the runs between cuts are independent.  k_ftrack_runs counts
//     every frame's m once, delivers the cuts on the spot and scans the runs' first frames and the cuts behind them into a list of pairs; one
//     wavefront walks one run.  (k_track_runs is not reused: its entries are the cuts themselves, read from int32 records, with row starts
//     folded in; here a cut belongs to no run and the candidates are f64 planes.  The scan is the same.)
//   * Ahead of the chain, for 16 frames at a time: the frames' F / B are on their way from memory in registers while the previous 16 frames'
//     chain runs; they are quantised into LDS, and then ALL 64 lanes form the tables: lane (a, b) the jump cost of candidate a of frame f - 1
//     to candidate b of frame f, lanes (t, c) < 8 T the local cost of candidate c on track t.  Every integer division of the definition is here
//     (one f64 division and an exact correction each: numerators stay below 2^52), none on the chain.
//   * The chain: the lanes are the states of frame f; lane k keeps its tuple's digits (from the combination table, constant data staged once in
//     LDS) and cost(f, k) in registers.  The loop over the predecessor states j is wave-uniform: cost(f - 1, j) and j's packed digits arrive by
//     v_readlane as scalars, a step is T LDS reads of the jump table addressed by (j's digit, the lane's own digit), T adds and one 64-bit minimum
//     with j folded into the key's low 6 bits (ties to the smaller j for nothing).  No shuffle and no reduction per frame: lane k's new cost is
//     its own minimum.  The state count changes from frame to frame; lanes without a state compute on digits 0 and are never read.
//   * The back-pointers go out as one byte per (frame, state), 40 to a frame.  The backtrace takes them back 64 frames at a time into LDS,
//     walks them with broadcast byte reads, and the lanes then write state[] and the chosen candidates' F / B.
// Range.  The lanes carry cost(f, k) - cost(f0 - 1, 0), f0 the first frame of the block of 16: a constant per frame changes no minimum's place,
// and state 0 is present in every frame of a run.  With P = T (2^20 2^15 + 2^20 2^24 + 2^20) < 2^47 the most one frame can add, the costs of one
// frame lie within P of each other, so what a lane holds stays within 17 P < 2^52 and the key below 2^58, whatever n_frames is.
// No matrix instructions: int64 minima along one dependent chain.  Vector stores and plain C++ only, no atomics.
#include "formant_track.h"

#include <cmath>
#include <cstring>

namespace sbv2 {

namespace {

constexpr int kWave = 64, kRunsBlock = 1024;
constexpr int kNB = 16;                   // frames whose tables are formed ahead of the chain
constexpr int kSlots = (kNB + 1) * 8;     // candidate slots of the frames f0 - 1 .. f0 + kNB - 1
constexpr int kSlotRegs = (kSlots + kWave - 1) / kWave;
constexpr int kBpWords = kWave * kFtBpStride / 4;
constexpr long long kNever = 0x7fffffffffffffffll;
static_assert(kFtMaxStates <= kFtBpStride && kFtMaxStates <= kWave && kFtBpStride % 8 == 0, "a state per lane, a byte per state");

// The strictly increasing T-tuples over 0 .. m - 1 in lexicographic order, 3 bits per digit, digit t at bits [3 t, 3 t + 3); count = C(m, T).
struct CombTable {
    uint32_t pk[kFtMaxTracks][8][kWave];
    int32_t count[kFtMaxTracks][8];
};
constexpr CombTable make_comb() {
    CombTable tb{};
    for (int T = 1; T <= kFtMaxTracks; ++T)
        for (int m = T; m <= kFtMaxCand; ++m) {
            int c[kFtMaxTracks] = {0, 1, 2, 3, 4}, n = 0;
            for (;;) {
                uint32_t p = 0;
                for (int t = 0; t < T; ++t) p |= (uint32_t)c[t] << (3 * t);
                tb.pk[T - 1][m][n++] = p;
                int i = T - 1;
                while (i >= 0 && c[i] == m - T + i) --i;
                if (i < 0) break;
                ++c[i];
                for (int j = i + 1; j < T; ++j) c[j] = c[j - 1] + 1;
            }
            tb.count[T - 1][m] = n;
        }
    return tb;
}
constexpr CombTable kCombHost = make_comb();
static_assert(kCombHost.count[3][7] == kFtMaxStates && kCombHost.count[2][7] == kFtMaxStates && kCombHost.count[4][5] == 1, "C(7, 4) = C(7, 3) = 35");
__device__ const CombTable kComb = make_comb();

struct FtRunArgs {
    const double* cf;   // [nf][K]
    const double* cb;
    int64_t nf;
    int32_t K, T;
    int32_t* runs;      // [nf + 2]: (first frame, end) of every run
    int32_t* nruns;
    uint8_t* mc;        // [nf]: the frames' candidate counts
    int32_t* state;     // [nf]
    double* F;          // [nf][T]
    double* B;
};

// One workgroup of 1024: thread t owns the frames [t chunk, (t + 1) chunk).  A frame is an entry iff it is a cut and its predecessor is not, or
// the other way round (frame -1 counts as a cut): the entries alternate first frame, end, first frame, ... and nf closes the last pair.
__global__ __launch_bounds__(kRunsBlock) void k_ftrack_runs(const FtRunArgs a) {
    __shared__ int32_t part[kRunsBlock];
    const int tid = threadIdx.x;
    const int64_t chunk = (a.nf + kRunsBlock - 1) / kRunsBlock, lo = min(tid * chunk, a.nf), hi = min(lo + chunk, a.nf);
    const auto count = [&a](int64_t f) -> int {
        int m = 0;
        for (int c = 0; c < a.K; ++c) m += a.cf[f * a.K + c] > 0.0;
        return m;
    };
    const bool cut_before = lo == 0 || count(lo - 1) < a.T;
    bool prev = cut_before;
    int32_t cnt = 0;
    for (int64_t f = lo; f < hi; ++f) {
        const int m = count(f);
        const bool cut = m < a.T;
        a.mc[f] = (uint8_t)m;
        if (cut) {   // delivered here: what the plain contour gives with n_formants = T
            a.state[f] = -1;
            for (int t = 0; t < a.T; ++t) {
                a.F[f * a.T + t] = t < m ? a.cf[f * a.K + t] : 0.0;
                a.B[f * a.T + t] = t < m ? a.cb[f * a.K + t] : 0.0;
            }
        }
        cnt += cut != prev;
        prev = cut;
    }
    part[tid] = cnt;
    __syncthreads();
    if (tid == 0) {
        int32_t before = 0;
        for (int t = 0; t < kRunsBlock; ++t) {
            const int32_t v = part[t];
            part[t] = before;
            before += v;
        }
        a.runs[before] = (int32_t)a.nf;
        *a.nruns = (before + 1) / 2;
    }
    __syncthreads();
    int32_t at = part[tid];
    prev = cut_before;
    for (int64_t f = lo; f < hi; ++f) {   // (its own writes)
        const bool cut = a.mc[f] < a.T;
        if (cut != prev) a.runs[at++] = (int32_t)f;
        prev = cut;
    }
}

struct FtPathArgs {
    const double* cf;   // [nf][K]
    const double* cb;
    int64_t nf;
    int32_t K;
    const int32_t* runs;
    const int32_t* nruns;
    const uint8_t* mc;
    int32_t Wf, Wb, Wj;   // <= 2^20
    int32_t R0, R1, R2, R3, R4;   // >= 1
    uint8_t* bp;          // [nf][kFtBpStride]
    int32_t* state;
    double* F;            // [nf][T]
    double* B;
};

// floor(num / den) for 0 <= num < 2^52, 1 <= den < 2^31: the f64 quotient is within 1/2 of the true one, so its integer part is off by one at most
__device__ inline long long idiv(long long num, long long den) {
    long long q = (long long)((double)num / (double)den);
    const long long r = num - q * den;
    if (r < 0) --q;
    else if (r >= den) ++q;
    return q;
}
// lane l's value in every lane; l is wave-uniform
__device__ inline long long from_lane(long long v, int l) {
    const int lo = __builtin_amdgcn_readlane((int)(uint32_t)v, l), hi = __builtin_amdgcn_readlane((int)(uint32_t)((unsigned long long)v >> 32), l);
    return (long long)(((unsigned long long)(uint32_t)hi << 32) | (uint32_t)lo);
}

template <int T>
__global__ __launch_bounds__(kWave) void k_ftrack_path(const FtPathArgs a) {
    __shared__ uint32_t tabs[8][kWave];      // the tuples of (m, T), a state per lane
    __shared__ int32_t cnt[8];               // how many states (m, T) has
    __shared__ int32_t fq[kSlots], bq[kSlots], ms[kNB + 1];
    __shared__ int32_t jt[kNB][kWave];       // jump cost of candidate a of frame f - 1 to candidate b of frame f at [a * 8 + b]
    __shared__ long long lt[kNB][T * 8];     // local cost of candidate c on track t at [t * 8 + c]
    __shared__ uint32_t bps[kBpWords];       // the back-pointers of 64 frames
    const int lane = threadIdx.x;
    for (int m = 0; m < 8; ++m) tabs[m][lane] = kComb.pk[T - 1][m][lane];
    if (lane < 8) cnt[lane] = kComb.count[T - 1][lane];   // (beside the tuples: no load from global memory on the chain)
    const int K = a.K;
    const int32_t nruns = *a.nruns;
    for (int32_t r = blockIdx.x; r < nruns; r += gridDim.x) {
        const int64_t s = a.runs[2 * r], e = a.runs[2 * r + 1];   // the run [s, e), s < e <= nf, every frame with m >= T
        double rf[kSlotRegs], rb[kSlotRegs];
        int32_t rm = 0;
        // the candidates of the frames f0 - 1 .. f0 + kNB - 1, those outside [s, e) as zeros (never used)
        const auto fetch = [&](int64_t f0) {
#pragma unroll
            for (int q = 0; q < kSlotRegs; ++q) {
                const int slot = lane + q * kWave, c = slot & 7;
                const int64_t f = f0 - 1 + (slot >> 3);
                const bool in = slot < kSlots && c < K && f >= s && f < e;
                rf[q] = in ? a.cf[f * K + c] : 0.0;
                rb[q] = in ? a.cb[f * K + c] : 0.0;
            }
            const int64_t f = f0 - 1 + lane;
            rm = lane <= kNB && f >= s && f < e ? a.mc[f] : 0;
        };
        fetch(s);
        long long cost = 0;
        uint32_t pk_prev = 0;
        int S_prev = 0;
        for (int64_t f0 = s; f0 < e; f0 += kNB) {
            __syncthreads();   // (the previous block's reads of the tables are done)
#pragma unroll
            for (int q = 0; q < kSlotRegs; ++q) {
                const int slot = lane + q * kWave;
                if (slot < kSlots) {
                    fq[slot] = rf[q] > 0.0 ? (int32_t)max(llrint(rf[q]), 1ll) : 0;
                    bq[slot] = (int32_t)llrint(fmin(rb[q], kFtMaxB));
                }
            }
            if (lane <= kNB) ms[lane] = rm;
            __syncthreads();
            if (f0 + kNB < e) fetch(f0 + kNB);   // in flight during the chain below
            {
                const int hi3 = lane >> 3, lo3 = lane & 7;
                const int32_t Rt = hi3 == 0 ? a.R0 : hi3 == 1 ? a.R1 : hi3 == 2 ? a.R2 : hi3 == 3 ? a.R3 : a.R4;
                for (int i = 0; i < kNB; ++i) {
                    const int32_t fa = fq[i * 8 + hi3], fb = fq[(i + 1) * 8 + lo3];
                    const int32_t d = fb > fa ? fb - fa : fa - fb;
                    jt[i][lane] = (int32_t)idiv((long long)a.Wj * d, max(max(fa, fb), 1));
                    if (hi3 < T) {   // candidate lo3 of frame f0 + i on track hi3
                        const int32_t Fc = max(fb, 1), dr = Fc > Rt ? Fc - Rt : Rt - Fc;
                        lt[i][lane] = idiv((long long)a.Wf * dr, Rt) + idiv((long long)a.Wb * bq[(i + 1) * 8 + lo3], Fc);
                    }
                }
            }
            __syncthreads();
            if (f0 > s) cost -= from_lane(cost, 0);   // (the header's range argument)
            const int nb = (int)min((int64_t)kNB, e - f0);
            for (int i = 0; i < nb; ++i) {
                const int m_cur = __builtin_amdgcn_readfirstlane(ms[i + 1]);
                const uint32_t pk = tabs[m_cur][lane];
                const int S_cur = cnt[m_cur];
                int own[T];
                long long loc = 0;
#pragma unroll
                for (int t = 0; t < T; ++t) {
                    own[t] = (int)((pk >> (3 * t)) & 7);
                    loc += lt[i][t * 8 + own[t]];
                }
                if (f0 + i == s) {   // the first frame of the run takes its local cost (uniform)
                    cost = loc;
                } else {
                    const int32_t* J = jt[i];
                    long long best = kNever;
                    for (int j = 0; j < S_prev; ++j) {
                        const uint32_t sj = (uint32_t)__builtin_amdgcn_readlane((int)pk_prev, j);
                        int32_t tr = 0;
#pragma unroll
                        for (int t = 0; t < T; ++t) tr += J[((sj >> (3 * t)) & 7) * 8 + own[t]];
                        best = min(best, (from_lane(cost, j) + tr) * 64 + j);
                    }
                    if (lane < S_cur) a.bp[(f0 + i) * kFtBpStride + lane] = (uint8_t)(best & 63);
                    cost = (best >> 6) + loc;
                }
                pk_prev = pk;
                S_prev = S_cur;
            }
        }
        // the last frame's state: the smallest k that attains the minimum
        long long fin = lane < S_prev ? cost * 64 + lane : kNever;
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) fin = min(fin, __shfl_xor(fin, d, kWave));
        int cur = __builtin_amdgcn_readfirstlane((int)(fin & 63));
        __threadfence();   // this wave's back-pointers, read back by its other lanes
        __syncthreads();
        for (int64_t hi = e; hi > s; hi -= kWave) {
            const int64_t base = hi - kWave;   // lane i has frame base + i; only the frames in (s, e) have back-pointers
            for (int w = lane; w < kBpWords; w += kWave) {
                const int64_t f = base + w / (kFtBpStride / 4);
                bps[w] = f > s ? reinterpret_cast<const uint32_t*>(a.bp)[f * (kFtBpStride / 4) + w % (kFtBpStride / 4)] : 0u;
            }
            __syncthreads();
            int mine = 0;
            for (int i = kWave - 1; i >= 0; --i) {
                if (base + i >= s) {   // (uniform)
                    if (lane == i) mine = cur;
                    if (base + i > s) cur = __builtin_amdgcn_readfirstlane((int)reinterpret_cast<const uint8_t*>(bps)[i * kFtBpStride + cur]);
                }
            }
            const int64_t g = base + lane;
            if (g >= s) {
                a.state[g] = mine;
                const uint32_t pk = tabs[a.mc[g]][mine];
#pragma unroll
                for (int t = 0; t < T; ++t) {
                    const int c = (int)((pk >> (3 * t)) & 7);
                    a.F[g * T + t] = a.cf[g * K + c];
                    a.B[g * T + t] = a.cb[g * K + c];
                }
            }
            __syncthreads();   // (bps is rewritten)
        }
    }
}

}  // namespace

FormantTrackSpec formant_track_spec(int n_tracks, int candidates, const double* ref_hz, double freq_cost, double bw_cost, double jump_cost, int reserved,
                                    int sample_rate, int order) {
    const std::string who = "formant track: ";
    SBV2_REQUIRE(reserved == 0, "sbv2_formant_track.reserved must be 0");
    SBV2_REQUIRE(n_tracks >= 1 && n_tracks <= kFtMaxTracks, who + "n_tracks must be in [1, 5]: " + std::to_string(n_tracks));
    SBV2_REQUIRE(candidates >= n_tracks && candidates <= kFtMaxCand && candidates <= order / 2,
                 who + "candidates must be in [n_tracks, min(7, order / 2)] = [" + std::to_string(n_tracks) + ", " +
                     std::to_string(std::min(kFtMaxCand, order / 2)) + "]: " + std::to_string(candidates));
    SBV2_REQUIRE(ref_hz, who + "ref_hz must not be NULL");
    FormantTrackSpec sp;
    sp.T = n_tracks;
    sp.K = candidates;
    for (int t = 0; t < n_tracks; ++t) {
        SBV2_REQUIRE(ref_hz[t] > (t ? ref_hz[t - 1] : 0.0) && ref_hz[t] < sample_rate / 2.0,
                     who + "ref_hz must ascend strictly within (0, sample_rate / 2): ref_hz[" + std::to_string(t) + "] = " + std::to_string(ref_hz[t]));
        sp.Rq[t] = std::max<int64_t>(std::llrint(ref_hz[t]), 1);
    }
    SBV2_REQUIRE(freq_cost >= 0.0 && freq_cost <= 16.0, who + "freq_cost must be in [0, 16]: " + std::to_string(freq_cost));
    SBV2_REQUIRE(bw_cost >= 0.0 && bw_cost <= 16.0, who + "bw_cost must be in [0, 16]: " + std::to_string(bw_cost));
    SBV2_REQUIRE(jump_cost >= 0.0 && jump_cost <= 16.0, who + "jump_cost must be in [0, 16]: " + std::to_string(jump_cost));
    sp.Wf = std::llrint(freq_cost * 65536.0);
    sp.Wb = std::llrint(bw_cost * 65536.0);
    sp.Wj = std::llrint(jump_cost * 65536.0);
    return sp;
}

void formant_track_check_table(const double* cand_f, const double* cand_b, int64_t nf, int K) {
    SBV2_REQUIRE(nf >= 0 && K >= 1 && K <= kFtMaxCand && (nf == 0 || (cand_f && cand_b)), "formant track: bad candidate table");
    for (int64_t f = 0; f < nf; ++f)
        for (int c = 0; c < K; ++c) {
            const double F = cand_f[f * K + c], B = cand_b[f * K + c], before = c ? cand_f[f * K + c - 1] : 0.0;
            const std::string at = " of frame " + std::to_string(f) + ", candidate " + std::to_string(c);
            SBV2_REQUIRE(F >= 0.0 && F <= kFtMaxF, "formant track: F" + at + " is outside [0, 32768]: " + std::to_string(F));
            SBV2_REQUIRE(c == 0 || (F > 0.0 ? before > 0.0 && F >= before : true),
                         "formant track: F" + at + " is not ascending (the positive entries first, in non-descending order)");
            SBV2_REQUIRE(B >= 0.0 && B <= kFtMaxB, "formant track: B" + at + " is outside [0, 2^24]: " + std::to_string(B));
        }
}

void FormantTrack::run(const double* cand_f, const double* cand_b, int64_t nf, const FormantTrackSpec& sp, hipStream_t s) {
    SBV2_REQUIRE(nf >= 0 && nf < (1 << 30), "too many formant frames: " + std::to_string(nf) + " >= 2^30");
    SBV2_REQUIRE(sp.T >= 1 && sp.T <= kFtMaxTracks && sp.K >= sp.T && sp.K <= kFtMaxCand && sp.Wf >= 0 && sp.Wf <= (16 << 16) && sp.Wb >= 0 &&
                     sp.Wb <= (16 << 16) && sp.Wj >= 0 && sp.Wj <= (16 << 16),
                 "internal: bad formant track spec");
    for (int t = 0; t < sp.T; ++t) SBV2_REQUIRE(sp.Rq[t] >= 1 && sp.Rq[t] <= (int64_t)kFtMaxF, "internal: bad formant track reference");
    nf_ = nf;
    T_ = sp.T;
    if (nf == 0) return;
    SBV2_REQUIRE(cand_f && cand_b, "internal: no candidates");
    const size_t F = (size_t)nf, out = 16 * F * (size_t)sp.T + 4 * F;
    const size_t o_runs = round_up64((int64_t)out, 64), o_mc = o_runs + round_up64(4 * ((int64_t)nf + 3), 64), o_bp = o_mc + round_up64(nf, 64),
                 bytes = o_bp + (size_t)kFtBpStride * F;
    char* h = static_cast<char*>(host_.reserve(out, std::max<size_t>(out * 2, 4096), s));
    char* d = static_cast<char*>(dev_.reserve(bytes, std::max<size_t>(bytes * 2, 65536), s));
    FtRunArgs ra{};
    ra.cf = cand_f;
    ra.cb = cand_b;
    ra.nf = nf;
    ra.K = sp.K;
    ra.T = sp.T;
    ra.runs = reinterpret_cast<int32_t*>(d + o_runs);
    ra.nruns = ra.runs + nf + 2;
    ra.mc = reinterpret_cast<uint8_t*>(d + o_mc);
    ra.F = reinterpret_cast<double*>(d);
    ra.B = ra.F + nf * sp.T;
    ra.state = reinterpret_cast<int32_t*>(ra.B + nf * sp.T);
    hipLaunchKernelGGL(k_ftrack_runs, dim3(1), dim3(kRunsBlock), 0, s, ra);
    HIP_CHECK(hipGetLastError());
    FtPathArgs pa{};
    pa.cf = cand_f;
    pa.cb = cand_b;
    pa.nf = nf;
    pa.K = sp.K;
    pa.runs = ra.runs;
    pa.nruns = ra.nruns;
    pa.mc = ra.mc;
    pa.Wf = (int32_t)sp.Wf;
    pa.Wb = (int32_t)sp.Wb;
    pa.Wj = (int32_t)sp.Wj;
    pa.R0 = (int32_t)std::max<int64_t>(sp.Rq[0], 1);
    pa.R1 = (int32_t)std::max<int64_t>(sp.Rq[1], 1);
    pa.R2 = (int32_t)std::max<int64_t>(sp.Rq[2], 1);
    pa.R3 = (int32_t)std::max<int64_t>(sp.Rq[3], 1);
    pa.R4 = (int32_t)std::max<int64_t>(sp.Rq[4], 1);
    pa.bp = reinterpret_cast<uint8_t*>(d + o_bp);
    pa.state = ra.state;
    pa.F = ra.F;
    pa.B = ra.B;
    const dim3 grid((unsigned)std::min<int64_t>((nf + 1) / 2, kFtGrid)), blk(kWave);   // (a run and the cut behind it take two frames)
    switch (sp.T) {
        case 1: hipLaunchKernelGGL(k_ftrack_path<1>, grid, blk, 0, s, pa); break;
        case 2: hipLaunchKernelGGL(k_ftrack_path<2>, grid, blk, 0, s, pa); break;
        case 3: hipLaunchKernelGGL(k_ftrack_path<3>, grid, blk, 0, s, pa); break;
        case 4: hipLaunchKernelGGL(k_ftrack_path<4>, grid, blk, 0, s, pa); break;
        default: hipLaunchKernelGGL(k_ftrack_path<5>, grid, blk, 0, s, pa); break;
    }
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(h, d, out, hipMemcpyDeviceToHost, s));
}

}  // namespace sbv2
