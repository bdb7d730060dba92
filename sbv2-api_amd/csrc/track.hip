// The pitch tracker: one best path through the per-frame candidates of the YIN contour on gfx950, as include/sbv2_hip.h states it above
// sbv2_pitch_track.  All of it is integer arithmetic, so the path equals a sequential restatement bit for bit.
//
// k_track_path is bound by latency, not by bandwidth: frame f needs the eight costs of frame f - 1, so a run of frames is one chain of
// dependent steps and the kernel's job is to keep that chain short and to run many chains side by side.
//   * Side by side: a frame without a candidate (a "cut") has the single state "unvoiced", so the choices before and after it do not influence
//     each other.  k_track_runs turns the cuts (and the rows' first frames) into a list of runs on the device; one wavefront walks one run.
//   * Short: the 64 lanes are the 8 x 8 pairs (k = lane >> 3 the state of frame f, j = lane & 7 the state of frame f - 1).  A step is one add,
//     a three-step minimum over the 8 lanes of a group with the index j in the key's low bits (ties to the smaller j for nothing), one add of
//     the local cost and one shuffle that hands cost(f, j) to the lanes that need it next.  The transition costs (an integer division each)
//     and the local costs do not depend on the chain: they are formed for 16 frames at a time from records staged in LDS, while the records
//     of the next 16 frames are already on their way from memory in registers.  The chain itself holds no memory access.
//   * The back-pointers go out as one byte per (frame, state).  The backtrace reads them back 64 frames at a time (one 8-byte word per lane)
//     and walks them with scalar reads of the lanes' words; the lanes then write state[] and, where asked, the tracked lag / voiced / c3.
// Absent states carry the cost 2^58 exactly: it is assigned, never accumulated, so it cannot overflow (real costs stay below 2^52 and the key
// is cost * 8 + j < 2^62), and it cannot win, because "unvoiced" is present in every frame.  Vector stores and plain C++ only, no atomics.
#include "track.h"

#include <cmath>
#include <cstring>

namespace sbv2 {

namespace {

constexpr int kWave = 64, kRunsBlock = 1024;
constexpr int kChunk = 16;                        // frames whose costs are formed ahead of the chain
constexpr int kStage = (kChunk + 1) * kTrackRec;  // int32 words of the records of frames f0 - 1 .. f0 + kChunk - 1
constexpr int kStageRegs = (kStage + kWave - 1) / kWave;
constexpr int32_t kRowFlag = 1 << 30, kFrameMask = kRowFlag - 1;   // a run entry: its first frame, and whether that frame begins a row
constexpr long long kAbsent = 1ll << 58;
static_assert(kTrackStates == 8, "the lanes are 8 x 8 state pairs");

struct TrackRunArgs {
    const int32_t* cand;
    int64_t nf;
    const int64_t* row_off;
    int32_t row_stride, nrows;
    int32_t* runs;    // [nf + 1]: the runs' entries, then nf
    int32_t* nruns;
    int32_t* flags;   // [nf] scratch: every frame's entry, formed once (the back-pointers' buffer, not yet in use)
};

// One workgroup of 1024: thread t owns the frames [t chunk, (t + 1) chunk); a frame starts a run iff it is the first of a row or has no candidate.
__global__ __launch_bounds__(kRunsBlock) void k_track_runs(const TrackRunArgs a) {
    __shared__ int32_t part[kRunsBlock];
    const int tid = threadIdx.x;
    const int64_t chunk = (a.nf + kRunsBlock - 1) / kRunsBlock, lo = min(tid * chunk, a.nf), hi = min(lo + chunk, a.nf);
    const auto entry = [&a](int64_t f) -> int32_t {   // 0: the frame goes on with its predecessor's run
        bool row = f == 0;
        if (!row && a.nrows > 0) {
            int lo = 0, hi = a.nrows;   // the first row that starts at or after f
            while (lo < hi) {
                const int mid = (lo + hi) / 2;
                if (a.row_off[(int64_t)mid * a.row_stride] < f) lo = mid + 1;
                else hi = mid;
            }
            row = lo < a.nrows && a.row_off[(int64_t)lo * a.row_stride] == f;
        }
        if (row) return (int32_t)f | kRowFlag;
        return a.cand[kTrackRec * f] == 0 ? (int32_t)f : 0;   // (frame 0 is a row's first: a plain entry is never 0)
    };
    int32_t cnt = 0;
    for (int64_t f = lo; f < hi; ++f) {
        const int32_t en = entry(f);
        a.flags[f] = en;
        cnt += en != 0;
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
        *a.nruns = before;
    }
    __syncthreads();
    int32_t at = part[tid];
    for (int64_t f = lo; f < hi; ++f) {   // (its own writes)
        const int32_t en = a.flags[f];
        if (en) a.runs[at++] = en;
    }
}

struct TrackPathArgs {
    const int32_t* cand;      // [nf][kTrackRec]
    const double* cand_c3;    // [nf][7][3] (with lag)
    int64_t nf;
    const int32_t* runs;
    const int32_t* nruns;
    int32_t U, Sw, J;         // <= 2^18, 2^18, 2^20
    uint8_t* bp;              // [nf][8]
    int32_t* state;           // [nf]
    double* c3;               // [nf][3], lag, voiced: the plain contour in, the tracked one out (or all NULL)
    int32_t* lag;
    int32_t* voiced;
};

// The minimum of the 8 lanes of a group, in every one of them: three DPP moves (lane ^ 1 and lane ^ 2 within the quad, then the mirror image
// within the 8 lanes, which lies in the other quad), no LDS round trip in the chain.  Every lane is active where this is called.
template <int CTRL>
__device__ inline long long dpp_move(long long v) {
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, CTRL, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)((unsigned long long)v >> 32), CTRL, 0xF, 0xF, false);
    return (long long)(((unsigned long long)(uint32_t)hi << 32) | (uint32_t)lo);
}
__device__ inline long long group_min(long long key) {
    key = min(key, dpp_move<0xB1>(key));    // quad_perm [1, 0, 3, 2]
    key = min(key, dpp_move<0x4E>(key));    // quad_perm [2, 3, 0, 1]
    key = min(key, dpp_move<0x141>(key));   // row_half_mirror
    return key;
}

__global__ __launch_bounds__(kWave) void k_track_path(const TrackPathArgs a) {
    __shared__ int32_t rec[kStage];
    const int lane = threadIdx.x, k = lane >> 3, j = lane & 7;
    const int32_t nruns = *a.nruns;
    for (int32_t r = blockIdx.x; r < nruns; r += gridDim.x) {
        const int32_t en0 = a.runs[r], en1 = a.runs[r + 1];
        const int64_t s = en0 & kFrameMask, e = en1 & kFrameMask;   // the run [s, e), s < e <= nf
        const bool to_cut = e < a.nf && !(en1 & kRowFlag);          // the frame behind it is a cut of the same row
        int32_t raw[kStageRegs];
        // the records of frames f0 - 1 .. f0 + kChunk - 1, those outside [0, e) as zeros (no candidate; never used)
        const auto fetch = [&](int64_t f0) {
            const int64_t base = (f0 - 1) * kTrackRec, first = max(f0 - 1, (int64_t)0) * kTrackRec, end = min(f0 + kChunk, e) * kTrackRec;
#pragma unroll
            for (int q = 0; q < kStageRegs; ++q) {
                const int64_t i = base + lane + q * kWave;
                raw[q] = lane + q * kWave < kStage && i >= first && i < end ? a.cand[i] : 0;
            }
        };
        fetch(s);
        long long cost = j == kTrackCand ? 0 : kAbsent;   // before the run: "unvoiced" at no cost, so that cost(s, k) = local(k)
        for (int64_t f0 = s; f0 < e; f0 += kChunk) {
            __syncthreads();   // (the previous chunk's reads of rec are done)
#pragma unroll
            for (int q = 0; q < kStageRegs; ++q)
                if (lane + q * kWave < kStage) rec[lane + q * kWave] = raw[q];
            __syncthreads();
            if (f0 + kChunk < e) fetch(f0 + kChunk);   // in flight during the chain below
            int32_t tr[kChunk], loc[kChunk];
#pragma unroll
            for (int i = 0; i < kChunk; ++i) {
                const int32_t* pr = rec + i * kTrackRec;   // frame f - 1
                const int32_t* cu = pr + kTrackRec;        // frame f
                const bool here = k == kTrackCand || k < cu[0], there = j == kTrackCand || j < pr[0];
                loc[i] = !here ? -1 : k == kTrackCand ? a.U : cu[1 + kTrackCand + min(k, kTrackCand - 1)];
                int32_t t = 0;
                if (f0 + i > s && here && there) {
                    if (k == kTrackCand || j == kTrackCand) {
                        t = k == j ? 0 : a.Sw;
                    } else {
                        const int32_t tk = cu[1 + k], tj = pr[1 + j];
                        const uint32_t d = (uint32_t)(tk > tj ? tk - tj : tj - tk), m = (uint32_t)max(max(tk, tj), 1);
                        t = (int32_t)((uint32_t)a.J * d / m);   // J d <= 2^20 * 1199 < 2^31
                    }
                }
                tr[i] = t;
            }
#pragma unroll
            for (int i = 0; i < kChunk; ++i) {
                if (f0 + i < e) {   // (uniform)
                    const long long key = group_min(((cost + tr[i]) << 3) | j);
                    const long long nc = loc[i] < 0 ? kAbsent : (key >> 3) + loc[i];
                    if (j == 0) a.bp[(f0 + i) * kTrackStates + k] = (uint8_t)(key & 7);
                    cost = __shfl(nc, j << 3, kWave);
                }
            }
        }
        // the last frame's state: towards a cut the switch is part of the choice
        const long long fin = group_min(((cost + (to_cut && j != kTrackCand ? a.Sw : 0)) << 3) | j);
        int cur = __builtin_amdgcn_readfirstlane((int)(fin & 7));
        __threadfence_block();   // this wave's back-pointers, read back by its other lanes
        __syncthreads();
        for (int64_t hi = e; hi > s; hi -= kWave) {
            const int64_t g = hi - kWave + lane;   // lane i has frame hi - 64 + i
            const uint64_t w = g >= s ? *reinterpret_cast<const uint64_t*>(a.bp + g * kTrackStates) : 0;
            const int wlo = (int)(uint32_t)w, whi = (int)(uint32_t)(w >> 32);
            int mine = kTrackCand;
#pragma unroll
            for (int i = kWave - 1; i >= 0; --i) {
                if (hi - kWave + i >= s) {   // (uniform)
                    if (lane == i) mine = cur;
                    const uint32_t half = (uint32_t)(cur < 4 ? __builtin_amdgcn_readlane(wlo, i) : __builtin_amdgcn_readlane(whi, i));
                    cur = (int)((half >> (8 * (cur & 3))) & 7);   // the state of frame hi - 64 + i - 1
                }
            }
            if (g >= s) {
                a.state[g] = mine;
                if (a.lag) {
                    if (mine < kTrackCand) {
                        const double* c = a.cand_c3 + (g * kTrackCand + mine) * 3;
                        a.lag[g] = a.cand[g * kTrackRec + 1 + mine];
                        a.voiced[g] = 1;
                        a.c3[3 * g] = c[0];
                        a.c3[3 * g + 1] = c[1];
                        a.c3[3 * g + 2] = c[2];
                    } else {
                        a.voiced[g] = 0;   // (lag and c3 stay the plain contour's)
                    }
                }
            }
        }
    }
}

}  // namespace

TrackSpec track_spec(double cand_max, double unvoiced_cost, double switch_cost, double jump_cost) {
    SBV2_REQUIRE(cand_max > 0.0 && cand_max <= 1.0, "pitch track: cand_max must be in (0, 1]: " + std::to_string(cand_max));
    SBV2_REQUIRE(unvoiced_cost >= 0.0 && unvoiced_cost <= 4.0, "pitch track: unvoiced_cost must be in [0, 4]: " + std::to_string(unvoiced_cost));
    SBV2_REQUIRE(switch_cost >= 0.0 && switch_cost <= 4.0, "pitch track: switch_cost must be in [0, 4]: " + std::to_string(switch_cost));
    SBV2_REQUIRE(jump_cost >= 0.0 && jump_cost <= 16.0, "pitch track: jump_cost must be in [0, 16]: " + std::to_string(jump_cost));
    TrackSpec t;
    t.cand_max = cand_max;
    t.U = std::llrint(unvoiced_cost * 65536.0);
    t.Sw = std::llrint(switch_cost * 65536.0);
    t.J = std::llrint(jump_cost * 65536.0);
    return t;
}

void track_check_table(const int32_t* cand, int64_t nf) {
    SBV2_REQUIRE(nf >= 0 && (nf == 0 || cand), "pitch track: bad candidate table");
    for (int64_t f = 0; f < nf; ++f) {
        const int32_t* r = cand + kTrackRec * f;
        SBV2_REQUIRE(r[0] >= 0 && r[0] <= kTrackCand, "pitch track: ncand of frame " + std::to_string(f) + " is outside [0, 7]: " + std::to_string(r[0]));
        for (int i = 0; i < r[0]; ++i) {
            const int32_t tau = r[1 + i], q = r[1 + kTrackCand + i];
            SBV2_REQUIRE(tau >= 1 && tau <= kPitchMaxTau, "pitch track: tau of frame " + std::to_string(f) + " is outside [1, " +
                                                              std::to_string(kPitchMaxTau) + "]: " + std::to_string(tau));
            SBV2_REQUIRE(i == 0 || tau > r[i], "pitch track: tau of frame " + std::to_string(f) + " is not ascending");
            SBV2_REQUIRE(q >= 0 && q <= 65536, "pitch track: q of frame " + std::to_string(f) + " is outside [0, 65536]: " + std::to_string(q));
        }
    }
}

void Track::run(const int32_t* cand, const double* cand_c3, int64_t nf, const TrackSpec& sp, double* c3, int32_t* lag, int32_t* voiced, hipStream_t s,
                const int64_t* row_off, int row_stride, int nrows) {
    SBV2_REQUIRE(nf >= 0 && nf < (1 << 30), "too many pitch frames: " + std::to_string(nf) + " >= 2^30");
    SBV2_REQUIRE((!lag == !voiced) && (!lag == !c3) && (!lag == !cand_c3), "internal: the tracked contour's arrays are given together or not at all");
    SBV2_REQUIRE(sp.U >= 0 && sp.U <= (4 << 16) && sp.Sw >= 0 && sp.Sw <= (4 << 16) && sp.J >= 0 && sp.J <= (16 << 16), "internal: bad track spec");
    SBV2_REQUIRE(nrows >= 0 && (nrows == 0 || (row_off && row_stride >= 1)), "internal: bad rows");
    if (nf == 0) return;
    SBV2_REQUIRE(cand, "internal: no candidates");
    const size_t o_state = round_up64(4 * ((size_t)nf + 2), 64), o_bp = o_state + round_up64(4 * (size_t)nf, 64), bytes = o_bp + 8 * (size_t)nf;
    char* d = static_cast<char*>(dev_.reserve(bytes, std::max<size_t>(bytes * 2, 65536), s));
    TrackRunArgs ra{};
    ra.cand = cand;
    ra.nf = nf;
    ra.row_off = row_off;
    ra.row_stride = row_stride;
    ra.nrows = nrows;
    ra.runs = reinterpret_cast<int32_t*>(d);
    ra.nruns = ra.runs + nf + 1;
    ra.flags = reinterpret_cast<int32_t*>(d + o_bp);
    hipLaunchKernelGGL(k_track_runs, dim3(1), dim3(kRunsBlock), 0, s, ra);
    HIP_CHECK(hipGetLastError());
    TrackPathArgs pa{};
    pa.cand = cand;
    pa.cand_c3 = cand_c3;
    pa.nf = nf;
    pa.runs = ra.runs;
    pa.nruns = ra.nruns;
    pa.U = (int32_t)sp.U;
    pa.Sw = (int32_t)sp.Sw;
    pa.J = (int32_t)sp.J;
    pa.bp = reinterpret_cast<uint8_t*>(d + o_bp);
    pa.state = d_state_ = reinterpret_cast<int32_t*>(d + o_state);
    pa.c3 = c3;
    pa.lag = lag;
    pa.voiced = voiced;
    hipLaunchKernelGGL(k_track_path, dim3((unsigned)std::min<int64_t>(nf, kTrackGrid)), dim3(kWave), 0, s, pa);
    HIP_CHECK(hipGetLastError());
}

}  // namespace sbv2
