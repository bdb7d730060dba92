// Pitch and intonation scale: TD-PSOLA of the run's native f32 rows on gfx950, as include/sbv2_hip.h states it above sbv2_voice.
//
// Three steps on one stream, no atomics, every f64 expression in the header's order (this file is built with -ffp-contract=off and says so
// itself below: bit equality with the numpy restatement depends on it).
//   * The contour: k_pitch_yin on f32 (marks.hip, pitch_launch), one launch per row, into this file's frame arrays.
//   * k_voice_marks, one workgroup per row.  Lanes take frames: the parabolic refinement (the f64 expression of pitch_finish), the integer sum of
//     f0 (int64, so the tree's order does not matter), the two Q32 increments.  One lane walks the frames once for the phases at the frames'
//     starts and the running mark counts: the increment is constant within a frame, so nothing walks the samples.  Lanes take frames again and
//     place each frame's marks by one division per mark, then take synthesis marks and find each one's nearest analysis mark by bisection.
//   * k_voice_gather, the hot path: a workgroup owns kTile consecutive output samples of one row, one per lane.  The synthesis marks whose
//     window can reach the tile are those with ts in [tile - half, tile + half): two bisections by one lane.  They are staged in LDS 256 at a
//     time with their analysis mark's position and its two half-widths, and every lane walks them in ascending j, adding w and w x in f64 where
//     the window covers its sample.  A staged mark is a broadcast read; x[ta + u] is consecutive across lanes.  Reads stay inside the row:
//     ta - L >= -1 and ta + R <= n by the definition of L and R, and the index is checked besides.
// Formant scaling (sbv2_formant) is a second instantiation of the gather (k_voice_gather_fmt) that only a call with a formant scale launches: a
// staged mark carries its voiced bit besides, the range of marks that may reach a tile is wider by 1 / min(q, 1), and every lane reads its grain
// at q u: two adjacent floats, interpolated in f64, each checked against the row (an unvoiced grain keeps its window and reads up to q times as
// far).  Lanes hold consecutive k, so their addresses advance by q: a wavefront touches 64 q floats of one grain, one to four cache lines
// a load.  LDS, the launch shape and the ascending order of the sum are the plain gather's.
// Per-token pitch edits (sbv2_token_pitch) are one more phase of k_voice_marks, in a second instantiation of it (k_voice_marks_tok) that only a call
// with a token table launches: between the row's mean and the increments, where T_f and m are at hand.  The frames' llrint(f0 65536) and voiced
// flags are prefix-summed over the row (an LDS scan, kBlock frames at a time), lanes take tokens (M_t from two prefix entries, rho_t, applied,
// src_f0), lanes take frames (the frame's token by bisection of the tokens' frame ends, then the integer window sum R_f).  Nothing loops over a
// token's frames or a frame's tokens, so a token that is the whole row and a row of a thousand empty tokens cost the same.
#include "voice.h"

#include <cmath>
#include <cstddef>
#include <cstring>

#pragma clang fp contract(off)

namespace sbv2 {

namespace {

constexpr int kBlock = 256;
static_assert(Voice::kTile == kBlock, "one output sample per lane");

struct VoiceRowDev {   // one row of a call, on the device
    int64_t off, n;    // samples [off, off + n) of x and y
    int64_t f_off, nf; // its frames in the frame arrays
    int64_t m_off, cap;   // its marks in ta / ts / map, and how many each may hold
};

struct VoiceMarkArgs {
    const VoiceRowDev* rows;
    const double* c3;        // the YIN results (not read with a given contour)
    const int32_t* lag;
    const int32_t* yvoiced;
    int32_t given;           // period / voiced hold the caller's contour
    double* period;          // [NF] T_f
    int32_t* voiced;         // [NF] 0 / 1
    int64_t *inc_a, *inc_s, *phi_a, *phi_s;   // [NF] increments; phases at the sample before the frame's first
    int32_t *off_a, *off_s;                   // [NF] marks before the frame
    int32_t *ta, *ts, *map;
    int32_t* count;          // [nrows][4]: n_a, n_s, status, 0
    double sr, p, s, g_lo, g_hi;
    int64_t inc_u, hop;
    int32_t tau_max;
};

struct VoiceTokRowDev {   // the tokens of one row in the token arrays
    int64_t t_off, nt;
};

struct VoiceTokArgs {
    const VoiceTokRowDev* rows;
    const double* value;      // [NT] the edit of every token, 0 = none
    const int32_t* fend;      // [NT] frames of the row whose centre lies before the token's end (ascending within a row)
    double *applied, *src;    // [NT] out
    int64_t* fq;              // [NF] llrint(f0 65536) of a voiced frame, 0 otherwise; then its inclusive prefix sum within the row
    int32_t* fc;              // [NF] the inclusive prefix count of voiced frames within the row
    int32_t* rho_t;           // [NT]
    int32_t* rho_f;           // [NF] the rho of the frame's token, 65536 where it has none
    double* ratio;            // [NF] R_f
    int32_t kind, smooth;
};

constexpr double kTwo32 = 4294967296.0;

// the marks of one frame: positions k = first + c - 1 for the c at which phi + c inc reaches the next integers (0 < inc <= 2^32: at most one a sample)
__device__ inline void place_marks(int64_t phi, int64_t inc, int64_t len, int64_t first, int32_t* out) {
    const int64_t B = phi >> 32, E = (phi + len * inc) >> 32;
    for (int64_t q = 1; q <= E - B; ++q) {
        const int64_t D = ((B + q) << 32) - phi;   // > 0
        out[q - 1] = (int32_t)(first + (D + inc - 1) / inc - 1);
    }
}

// T_f of a frame from the estimator's results: the parabolic refinement (the f64 expression of pitch_finish), limited to one sample
__device__ inline double refined_period(double cm, double c0, double cp, int32_t lag, int32_t tau_max) {
    const double den = cm - 2.0 * c0 + cp;
    const bool both = lag - 1 >= 1 && lag + 1 <= tau_max;
    double delta = den > 0.0 && both ? 0.5 * (cm - cp) / den : 0.0;
    delta = fmin(fmax(delta, -1.0), 1.0);
    return (double)lag + delta;
}

// the two increments of a voiced frame of period T whose target is g (before the clamp)
__device__ inline void voiced_increments(double sr, double g_lo, double g_hi, double T, double g, int64_t* ia, int64_t* is) {
    g = fmin(fmax(g, g_lo), g_hi);
    const double Tp = sr / g;
    *ia = llrint(kTwo32 / T);
    *is = llrint(kTwo32 / Tp);
}

// the analysis mark nearest to t among ta[0, na), na >= 1, a tie to the earlier
__device__ inline int32_t nearest_mark(const int32_t* ta, int32_t na, int32_t t) {
    int32_t lo = 0, hi = na;   // the first analysis mark at or after t
    while (lo < hi) {
        const int32_t mid = (lo + hi) / 2;
        if (ta[mid] < t) lo = mid + 1;
        else hi = mid;
    }
    if (lo == 0) return 0;
    if (lo == na) return na - 1;
    return t - ta[lo - 1] <= ta[lo] - t ? lo - 1 : lo;
}

// The per-token phase of k_voice_marks_tok: fq / voiced of the row are written, m is its mean.  sh_q / sh_c are the kernel's reduction arrays.
__device__ inline void token_ratios(const VoiceMarkArgs& a, const VoiceTokArgs& t, const VoiceRowDev& r, double m, int64_t* sh_q, int32_t* sh_c) {
    const int tid = threadIdx.x;
    const int64_t nf = r.nf;
    const VoiceTokRowDev tr = t.rows[blockIdx.x];
    __syncthreads();   // every lane has read the row's sums
    // inclusive prefix sums of q and voiced over the row's frames (integers: any order gives these values)
    int64_t carry_q = 0;
    int32_t carry_c = 0;
    for (int64_t base = 0; base < nf; base += kBlock) {
        const int64_t f = base + tid, F = r.f_off + f;
        sh_q[tid] = f < nf ? t.fq[F] : 0;
        sh_c[tid] = f < nf ? a.voiced[F] : 0;
        __syncthreads();
        for (int d = 1; d < kBlock; d <<= 1) {
            const int64_t q = tid >= d ? sh_q[tid - d] : 0;
            const int32_t c = tid >= d ? sh_c[tid - d] : 0;
            __syncthreads();
            sh_q[tid] += q;
            sh_c[tid] += c;
            __syncthreads();
        }
        if (f < nf) {
            t.fq[F] = carry_q + sh_q[tid];
            t.fc[F] = carry_c + sh_c[tid];
        }
        carry_q += sh_q[kBlock - 1];
        carry_c += sh_c[kBlock - 1];
        __syncthreads();
    }
    // lanes take tokens: the measured mean, the ratio
    for (int64_t i = tid; i < tr.nt; i += kBlock) {
        const int64_t I = tr.t_off + i;
        const int64_t fb = min((int64_t)(i ? t.fend[I - 1] : 0), nf), fe = min((int64_t)t.fend[I], nf);
        int64_t q = 0;
        int32_t c = 0;
        if (fe > fb) {
            q = t.fq[r.f_off + fe - 1] - (fb ? t.fq[r.f_off + fb - 1] : 0);
            c = t.fc[r.f_off + fe - 1] - (fb ? t.fc[r.f_off + fb - 1] : 0);
        }
        const double M = c ? (double)q / (65536.0 * (double)c) : 0.0;
        const double val = t.value[I];
        int64_t rho = 65536;
        if (val != 0.0) {
            if (t.kind == 0) {
                rho = llrint(val * 65536.0);
            } else if (c) {
                const double G = a.p * (m + a.s * (M - m));
                rho = llrint(fmin(fmax(val / G, 0.5), 2.0) * 65536.0);
            }
        }
        t.rho_t[I] = (int32_t)rho;
        t.applied[I] = (double)rho / 65536.0;
        t.src[I] = M;
    }
    __syncthreads();
    // lanes take frames: the frame's token is the first whose frames end behind it
    for (int64_t f = tid; f < nf; f += kBlock) {
        int64_t lo = 0, hi = tr.nt;
        while (lo < hi) {
            const int64_t mid = (lo + hi) / 2;
            if (t.fend[tr.t_off + mid] <= f) lo = mid + 1;
            else hi = mid;
        }
        t.rho_f[r.f_off + f] = lo < tr.nt ? t.rho_t[tr.t_off + lo] : 65536;
    }
    __syncthreads();
    for (int64_t f = tid; f < nf; f += kBlock) {
        const int64_t i0 = max(f - t.smooth, (int64_t)0), i1 = min(f + t.smooth, nf - 1);
        int64_t sum = 0;
        for (int64_t i = i0; i <= i1; ++i) sum += t.rho_f[r.f_off + i];
        t.ratio[r.f_off + f] = (double)sum / (65536.0 * (double)(i1 - i0 + 1));
    }
}

// kTok: with the per-token phase and R_f in the target; without, t is not looked at and the code is what it was before token edits existed
template <bool kTok>
__device__ __forceinline__ void voice_marks_body(const VoiceMarkArgs& a, const VoiceTokArgs* t) {
    __shared__ int64_t sh_sum[kBlock];
    __shared__ int32_t sh_cnt[kBlock];
    __shared__ int32_t sh_n[2];
    const VoiceRowDev r = a.rows[blockIdx.x];
    const int tid = threadIdx.x;
    const int64_t nf = r.nf;
    // the contour and the integer sum of f0
    int64_t sum = 0;
    int32_t cnt = 0;
    for (int64_t f = tid; f < nf; f += kBlock) {
        const int64_t F = r.f_off + f;
        double T;
        int32_t v;
        if (a.given) {
            T = a.period[F];
            v = a.voiced[F] != 0;
        } else {
            T = refined_period(a.c3[3 * F], a.c3[3 * F + 1], a.c3[3 * F + 2], a.lag[F], a.tau_max);
            v = a.yvoiced[F] != 0;
            a.period[F] = T;
        }
        a.voiced[F] = v;
        if (v) {
            const int64_t q = llrint((a.sr / T) * 65536.0);
            sum += q;
            ++cnt;
            if constexpr (kTok) t->fq[F] = q;
        } else if constexpr (kTok) {
            t->fq[F] = 0;
        }
    }
    sh_sum[tid] = sum;
    sh_cnt[tid] = cnt;
    __syncthreads();
    for (int d = kBlock / 2; d >= 1; d >>= 1) {
        if (tid < d) sh_sum[tid] += sh_sum[tid + d], sh_cnt[tid] += sh_cnt[tid + d];
        __syncthreads();
    }
    const int32_t nv = sh_cnt[0];
    const double m = nv ? (double)sh_sum[0] / (65536.0 * (double)nv) : 0.0;
    if constexpr (kTok) token_ratios(a, *t, r, m, sh_sum, sh_cnt);
    // the increments
    for (int64_t f = tid; f < nf; f += kBlock) {
        const int64_t F = r.f_off + f;
        int64_t ia = a.inc_u, is = a.inc_u;
        if (a.voiced[F]) {
            const double T = a.period[F], f0 = a.sr / T;
            double g = a.p * (m + a.s * (f0 - m));
            if constexpr (kTok) g = t->ratio[F] * g;
            voiced_increments(a.sr, a.g_lo, a.g_hi, T, g, &ia, &is);
        }
        a.inc_a[F] = ia;
        a.inc_s[F] = is;
    }
    __syncthreads();
    // the phases at the frames' starts and the marks before each frame: one lane, once over the frames
    if (tid == 0) {
        int64_t pa = 0, ps = 0, ca = 0, cs = 0;
        bool prev = false;
        for (int64_t f = 0; f < nf; ++f) {
            const int64_t F = r.f_off + f, len = min(a.hop, r.n - f * a.hop), ia = a.inc_a[F], is = a.inc_s[F];
            const bool v = a.voiced[F] != 0;
            if (!v || !prev) ps = pa;   // an unvoiced frame has the analysis marks; a voiced run starts from the analysis phase
            a.phi_a[F] = pa;
            a.phi_s[F] = ps;
            a.off_a[F] = (int32_t)min(ca, r.cap);
            a.off_s[F] = (int32_t)min(cs, r.cap);
            ca += ((pa + len * ia) >> 32) - (pa >> 32);
            cs += ((ps + len * is) >> 32) - (ps >> 32);
            pa += len * ia;
            ps += len * is;
            prev = v;
        }
        const bool fits = ca <= r.cap && cs <= r.cap;
        sh_n[0] = fits ? (int32_t)ca : 0;
        sh_n[1] = fits ? (int32_t)cs : 0;
        int32_t* c = a.count + 4 * blockIdx.x;
        c[0] = sh_n[0];
        c[1] = sh_n[1];
        c[2] = fits ? 0 : 1;
        c[3] = 0;
    }
    __syncthreads();
    const int32_t na = sh_n[0], ns = sh_n[1];
    if (na == 0 && ns == 0) return;   // (uniform) no marks, or more than planned: nothing is written
    int32_t* ta = a.ta + r.m_off;
    int32_t* ts = a.ts + r.m_off;
    int32_t* mp = a.map + r.m_off;
    for (int64_t f = tid; f < nf; f += kBlock) {
        const int64_t F = r.f_off + f, len = min(a.hop, r.n - f * a.hop);
        place_marks(a.phi_a[F], a.inc_a[F], len, f * a.hop, ta + a.off_a[F]);
        place_marks(a.phi_s[F], a.inc_s[F], len, f * a.hop, ts + a.off_s[F]);
    }
    __syncthreads();
    if (na == 0) return;
    // the nearest analysis mark of every synthesis mark, a tie to the earlier
    for (int32_t j = tid; j < ns; j += kBlock) mp[j] = nearest_mark(ta, na, ts[j]);
}

__global__ __launch_bounds__(kBlock) void k_voice_marks(const VoiceMarkArgs a) { voice_marks_body<false>(a, nullptr); }
__global__ __launch_bounds__(kBlock) void k_voice_marks_tok(const VoiceMarkArgs a, const VoiceTokArgs t) { voice_marks_body<true>(a, &t); }

// the first j in [0, n) with v[j] >= t (n if none)
__device__ inline int32_t first_at_or_after(const int32_t* v, int32_t n, int64_t t) {
    int32_t lo = 0, hi = n;
    while (lo < hi) {
        const int32_t mid = (lo + hi) / 2;
        if (v[mid] < t) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// The fed marks kernel (StreamVoice::push): ONE workgroup takes the frames [f0, f1) of one row that a push completed and goes on from the
// row's carried state: the phases and the voiced-run bit behind frame f0 - 1 (state[0 .. 3)), the mark counts and the number of mapped
// synthesis marks (count[0], [1], [3]).  a.rows / a.count point at THAT row's entries.  The target pivots about d.pivot, the caller's, where
// k_voice_marks has the row's mean; every other expression is that kernel's (the helpers above), so with the mean's bits as the pivot the
// lists are its lists.  The prefix over the frames is latency-bound, as k_track_path is: lanes stage kBlock frames' increments in LDS,
// one lane walks them there and leaves phases and offsets in LDS, lanes write them out: the walk waits for LDS, never for memory.
// Mapping: a synthesis mark is mapped once the first analysis mark at or after it is known, which is when it lies at or before the last
// known analysis mark, or when the row's last frame is in (d.last): the bisection over the known list then answers what it answers over
// the whole one.  More marks than planned: status is set, nothing more is written by this or any later push.
struct VoiceFedArgs {
    const PitchFrame* res;   // [NF] the estimator's results (not read with a given contour)
    int64_t* state;          // [3] phi_a, phi_s at the last sample before frame f0; 1 if frame f0 - 1 is voiced
    double pivot;
    int64_t f0, f1;
    int32_t last;            // f1 is the row's frame count
};

__global__ __launch_bounds__(kBlock) void k_voice_marks_fed(const VoiceMarkArgs a, const VoiceFedArgs d) {
    __shared__ int64_t s_ia[kBlock], s_is[kBlock], s_pa[kBlock], s_ps[kBlock];
    __shared__ int32_t s_v[kBlock], s_oa[kBlock], s_os[kBlock];
    __shared__ int64_t s_st[5];   // phi_a, phi_s, voiced before, n_a, n_s
    __shared__ int32_t s_n[3];    // status, mapped before, mapped after
    const VoiceRowDev r = a.rows[0];
    const int tid = threadIdx.x;
    if (tid == 0) {
        s_st[0] = d.state[0];
        s_st[1] = d.state[1];
        s_st[2] = d.state[2];
        s_st[3] = a.count[0];
        s_st[4] = a.count[1];
        s_n[0] = a.count[2];
        s_n[1] = a.count[3];
    }
    __syncthreads();
    if (s_n[0]) return;   // (uniform) an earlier push found more marks than planned
    for (int64_t base = d.f0; base < d.f1; base += kBlock) {
        const int64_t f = base + tid, F = r.f_off + f;
        if (f < d.f1) {
            double T;
            int32_t v;
            if (a.given) {
                T = a.period[F];
                v = a.voiced[F] != 0;
            } else {
                const PitchFrame pf = d.res[F];
                T = refined_period(pf.c3[0], pf.c3[1], pf.c3[2], pf.lag, a.tau_max);
                v = pf.voiced != 0;
                a.period[F] = T;
            }
            a.voiced[F] = v;
            int64_t ia = a.inc_u, is = a.inc_u;
            if (v) voiced_increments(a.sr, a.g_lo, a.g_hi, T, a.p * (d.pivot + a.s * (a.sr / T - d.pivot)), &ia, &is);
            a.inc_a[F] = ia;
            a.inc_s[F] = is;
            s_ia[tid] = ia;
            s_is[tid] = is;
            s_v[tid] = v;
        }
        __syncthreads();
        if (tid == 0) {   // k_voice_marks' walk, from the carried state
            int64_t pa = s_st[0], ps = s_st[1], ca = s_st[3], cs = s_st[4];
            bool prev = s_st[2] != 0;
            const int cn = (int)min((int64_t)kBlock, d.f1 - base);
            for (int i = 0; i < cn; ++i) {
                const int64_t len = min(a.hop, r.n - (base + i) * a.hop), ia = s_ia[i], is = s_is[i];
                const bool v = s_v[i] != 0;
                if (!v || !prev) ps = pa;
                s_pa[i] = pa;
                s_ps[i] = ps;
                s_oa[i] = (int32_t)min(ca, r.cap);
                s_os[i] = (int32_t)min(cs, r.cap);
                ca += ((pa + len * ia) >> 32) - (pa >> 32);
                cs += ((ps + len * is) >> 32) - (ps >> 32);
                pa += len * ia;
                ps += len * is;
                prev = v;
            }
            s_st[0] = pa;
            s_st[1] = ps;
            s_st[2] = prev;
            s_st[3] = ca;
            s_st[4] = cs;
        }
        __syncthreads();
        if (f < d.f1) {
            a.phi_a[F] = s_pa[tid];
            a.phi_s[F] = s_ps[tid];
            a.off_a[F] = s_oa[tid];
            a.off_s[F] = s_os[tid];
        }
        __syncthreads();   // (the next round writes the staged frames again)
    }
    const int64_t ca = s_st[3], cs = s_st[4];
    if (ca > r.cap || cs > r.cap) {   // (uniform) the counts stay where they were: the gather reads nothing beyond them
        if (tid == 0) a.count[2] = 1;
        return;
    }
    const int32_t na = (int32_t)ca, ns = (int32_t)cs;
    int32_t* ta = a.ta + r.m_off;
    int32_t* ts = a.ts + r.m_off;
    int32_t* mp = a.map + r.m_off;
    for (int64_t f = d.f0 + tid; f < d.f1; f += kBlock) {   // (frame f's phases were written by this lane)
        const int64_t F = r.f_off + f, len = min(a.hop, r.n - f * a.hop);
        place_marks(a.phi_a[F], a.inc_a[F], len, f * a.hop, ta + a.off_a[F]);
        place_marks(a.phi_s[F], a.inc_s[F], len, f * a.hop, ts + a.off_s[F]);
    }
    __syncthreads();
    const int32_t mapped = s_n[1];
    if (tid == 0) {
        int32_t upto = mapped;
        if (na > 0) upto = d.last ? ns : max(mapped, first_at_or_after(ts, ns, (int64_t)ta[na - 1] + 1));
        s_n[2] = upto;
    }
    __syncthreads();
    const int32_t upto = s_n[2];
    for (int32_t j = mapped + tid; j < upto; j += kBlock) mp[j] = nearest_mark(ta, na, ts[j]);
    if (tid == 0) {
        d.state[0] = s_st[0];
        d.state[1] = s_st[1];
        d.state[2] = s_st[2];
        a.count[0] = na;
        a.count[1] = ns;
        a.count[3] = upto;
    }
}

struct VoiceGatherArgs {
    const VoiceRowDev* rows;
    const float* x;
    float* y;
    const int32_t *ta, *ts, *map, *count;
    int32_t half;
    int64_t k0, k1;   // the launch covers the outputs [k0, min(k1, n)) of every row (a whole row: 0 and any k1 >= n)
};

struct VoiceFmtArgs {   // what k_voice_gather_fmt needs besides
    const int32_t* voiced;   // [NF] the contour the marks were placed by
    double q;                // formant_scale
    int64_t hop;
    int32_t half;            // the widened search range: ceil(half / min(q, 1)) + 1
};

// kFmt: every grain is read at q u by linear interpolation (sbv2_formant); without, f is not looked at and the code is what it was before
// formant scaling existed
template <bool kFmt>
__device__ __forceinline__ void voice_gather_body(const VoiceGatherArgs& a, const VoiceFmtArgs* f) {
    __shared__ int32_t s_ts[kBlock], s_ta[kBlock], s_L[kBlock], s_R[kBlock], s_edge[kBlock];
    __shared__ int32_t s_range[2];
    const VoiceRowDev r = a.rows[blockIdx.y];
    const int64_t t0 = a.k0 + (int64_t)blockIdx.x * Voice::kTile, end = min(r.n, a.k1);
    if (t0 >= end) return;   // (uniform: this row has fewer tiles than the longest)
    const int tid = threadIdx.x;
    const int64_t n = r.n, k = t0 + tid, t1 = min(t0 + Voice::kTile, end);
    const bool mine = k < end;
    const float* x = a.x + r.off;
    float* y = a.y + r.off;
    const int32_t na = a.count[4 * blockIdx.y], ns = a.count[4 * blockIdx.y + 1];
    if (na == 0) {   // (uniform) a row without an analysis mark is copied
        if (mine) y[k] = x[k];
        return;
    }
    const int32_t* ta = a.ta + r.m_off;
    const int32_t* ts = a.ts + r.m_off;
    const int32_t* mp = a.map + r.m_off;
    int32_t half = a.half;
    if constexpr (kFmt) half = f->half;
    if (tid == 0) {
        s_range[0] = first_at_or_after(ts, ns, t0 - half);
        s_range[1] = first_at_or_after(ts, ns, t1 + half);
    }
    __syncthreads();
    const int32_t j0 = s_range[0], j1 = s_range[1];
    double num = 0.0, den = 0.0;
    for (int32_t c = j0; c < j1; c += kBlock) {
        const int32_t j = c + tid;
        if (j < j1) {
            const int32_t m = mp[j], am = ta[m];
            s_ts[tid] = ts[j];
            s_ta[tid] = am;
            s_L[tid] = m > 0 ? am - ta[m - 1] : am + 1;
            s_R[tid] = m + 1 < na ? ta[m + 1] - am : (int32_t)(n - am);
            int32_t e = (m == 0 ? 1 : 0) | (m == na - 1 ? 2 : 0);
            if constexpr (kFmt) e |= f->voiced[r.f_off + am / f->hop] ? 4 : 0;   // (am < n: a frame of the row)
            s_edge[tid] = e;
        }
        __syncthreads();
        const int32_t cn = min(kBlock, j1 - c);
        if (mine) {
            for (int32_t i = 0; i < cn; ++i) {   // ascending j
                const int64_t u = k - s_ts[i];
                const int32_t L = s_L[i], R = s_R[i];
                if constexpr (kFmt) {
                    const int32_t e = s_edge[i];
                    const double du = (double)u, p = f->q * du, pw = (e & 4) ? p : du;
                    if (!(pw > -(double)L && pw < (double)R)) continue;
                    const double v = fabs(pw) / (double)(pw < 0.0 ? L : R);
                    double w = 1.0 - (v * v) * (3.0 - 2.0 * v);
                    if ((pw < 0.0 && (e & 1)) || (pw > 0.0 && (e & 2))) w = 1.0;
                    const double fl = floor(p), fr = p - fl;
                    const int64_t src = s_ta[i] + (int64_t)fl;   // X is 0 outside the row: an unvoiced grain reads up to q times its width
                    const double x0 = src >= 0 && src < n ? (double)x[src] : 0.0;
                    const double x1 = src + 1 >= 0 && src + 1 < n ? (double)x[src + 1] : 0.0;
                    const double val = (1.0 - fr) * x0 + fr * x1;
                    num += w * val;
                    den += w;
                } else {
                    if (u <= -(int64_t)L || u >= R) continue;
                    const int64_t src = s_ta[i] + u;
                    if (src < 0 || src >= n) continue;   // (never, by the definition of L and R)
                    const double v = (double)(u < 0 ? -u : u) / (double)(u < 0 ? L : R);
                    double w = 1.0 - (v * v) * (3.0 - 2.0 * v);
                    const int32_t e = s_edge[i];
                    if ((u < 0 && (e & 1)) || (u > 0 && (e & 2))) w = 1.0;
                    num += w * (double)x[src];
                    den += w;
                }
            }
        }
        __syncthreads();
    }
    if (mine) y[k] = (float)(num / fmax(den, 1.0));
}

__global__ __launch_bounds__(kBlock) void k_voice_gather(const VoiceGatherArgs a) { voice_gather_body<false>(a, nullptr); }
__global__ __launch_bounds__(kBlock) void k_voice_gather_fmt(const VoiceGatherArgs a, const VoiceFmtArgs f) { voice_gather_body<true>(a, &f); }

}  // namespace

VoiceSpec voice_spec(int sample_rate, double pitch_scale, double intonation_scale, int64_t hop, double f0_min, double f0_max, double threshold) {
    SBV2_REQUIRE(pitch_scale >= 0.5 && pitch_scale <= 2.0, "voice: pitch_scale must be in [0.5, 2]: " + std::to_string(pitch_scale));
    SBV2_REQUIRE(intonation_scale >= 0.0 && intonation_scale <= 2.0, "voice: intonation_scale must be in [0, 2]: " + std::to_string(intonation_scale));
    SBV2_REQUIRE(sample_rate >= kVoiceMinRate && sample_rate <= kPitchMaxRate,
                 "voice: sample rate must be in [" + std::to_string(kVoiceMinRate) + ", " + std::to_string(kPitchMaxRate) + "]: " + std::to_string(sample_rate));
    if (hop == 0) hop = sample_rate / 200;
    SBV2_REQUIRE(hop >= sample_rate / 1000 && hop <= sample_rate / 50, "voice: hop must be in [sample_rate / 1000, sample_rate / 50] = [" +
                                                                            std::to_string(sample_rate / 1000) + ", " + std::to_string(sample_rate / 50) +
                                                                            "] (0 = sample_rate / 200): " + std::to_string(hop));
    VoiceSpec v;
    v.pitch = pitch_spec(sample_rate, hop, f0_min == 0.0 ? 70.0 : f0_min, f0_max == 0.0 ? 600.0 : f0_max, threshold == 0.0 ? 0.15 : threshold);
    v.pitch_scale = pitch_scale;
    v.intonation_scale = intonation_scale;
    const double lo = f0_min == 0.0 ? 70.0 : f0_min, hi = f0_max == 0.0 ? 600.0 : f0_max;
    v.g_lo = lo / 2.0;
    v.g_hi = 2.0 * hi;
    const int tu = sample_rate / 200;
    v.inc_u = std::llrint(kTwo32 / (double)tu);
    v.half = std::max(v.pitch.tau_max + 1, tu) + 2;
    // the shortest synthesis period is sr / (2 f0_max) >= 2, the shortest analysis period tau_min - 1 is longer; a rounded increment may bring two
    // marks one sample closer than the period's floor
    v.min_s = std::max(1, std::min((int)std::floor(sample_rate / v.g_hi), tu) - 1);
    v.min_a = std::max(1, std::min(v.pitch.tau_min - 1, tu) - 1);
    return v;
}

FormantSpec formant_spec(double formant_scale, double reserved, const VoiceSpec& v) {
    SBV2_REQUIRE(reserved == 0.0, "sbv2_formant.reserved must be 0");   // (a NaN fails)
    SBV2_REQUIRE(formant_scale >= 0.5 && formant_scale <= 2.0, "voice: formant_scale must be in [0.5, 2]: " + std::to_string(formant_scale));   // (a NaN fails)
    FormantSpec f;
    f.scale = formant_scale;
    f.half = (int)std::ceil((double)v.half / std::min(formant_scale, 1.0)) + 1;
    return f;
}

void voice_tokens_check(const double* value, int64_t n_tokens, int kind, int smooth, const VoiceSpec& sp) {
    SBV2_REQUIRE(n_tokens >= 0 && (value || n_tokens == 0), "token pitch: value must not be NULL");
    SBV2_REQUIRE(kind == 0 || kind == 1, "token pitch: kind must be 0 (ratio) or 1 (Hz): " + std::to_string(kind));
    SBV2_REQUIRE(smooth >= 0 && smooth <= kVoiceMaxSmooth, "token pitch: smooth must be in [0, " + std::to_string(kVoiceMaxSmooth) + "]: " + std::to_string(smooth));
    const double lo = kind == 0 ? 0.5 : sp.g_lo, hi = kind == 0 ? 2.0 : sp.g_hi;
    for (int64_t t = 0; t < n_tokens; ++t)   // (a NaN fails both comparisons)
        SBV2_REQUIRE(value[t] == 0.0 || (value[t] >= lo && value[t] <= hi),
                     "token pitch: value of token " + std::to_string(t) + " must be 0 or in [" + std::to_string(lo) + ", " + std::to_string(hi) + "] (" +
                         (kind == 0 ? "a ratio" : "Hz") + "): " + std::to_string(value[t]));
}

float* Voice::run(const float* x, int64_t span, const VoiceRow* rows, int nrows, const VoiceSpec& sp, hipStream_t s, const double* period_in,
                  const int32_t* voiced_in, const TrackSpec* tr, const VoiceTokens* tok, const FormantSpec* fm) {
    SBV2_REQUIRE(nrows >= 0 && nrows <= 65535 && span >= 0 && (nrows == 0 || rows), "voice: bad rows");
    SBV2_REQUIRE(!period_in == !voiced_in, "voice: period_in and voiced_in are given together or not at all");
    const int64_t hop = sp.pitch.hop;
    std::vector<VoiceRowDev> rd((size_t)nrows);
    int64_t NF = 0, NCAP = 0, longest = 0;
    cap_off_.assign((size_t)nrows, 0);
    for (int i = 0; i < nrows; ++i) {
        SBV2_REQUIRE(rows[i].n >= 0 && rows[i].n < (1 << 30) && rows[i].off >= 0 && rows[i].off + rows[i].n <= span,
                     "voice: row " + std::to_string(i) + " is outside the buffer or longer than 2^30 samples");
        rd[i].off = rows[i].off;
        rd[i].n = rows[i].n;
        rd[i].f_off = NF;
        rd[i].nf = pitch_frames(rows[i].n, hop);
        rd[i].m_off = NCAP;
        rd[i].cap = rows[i].n / std::min(sp.min_a, sp.min_s) + rd[i].nf + 2;
        cap_off_[i] = NCAP;
        NF += rd[i].nf;
        NCAP += rd[i].cap;
        longest = std::max(longest, rows[i].n);
    }
    SBV2_REQUIRE(NF < (1 << 30) && NCAP < (int64_t(1) << 31), "voice: too many frames or marks in one call");
    if (period_in)
        for (int64_t f = 0; f < NF; ++f)
            SBV2_REQUIRE(!voiced_in[f] || (period_in[f] >= sp.pitch.tau_min - 1 && period_in[f] <= sp.pitch.tau_max + 1),
                         "voice: period_in of voiced frame " + std::to_string(f) + " is outside [tau_min - 1, tau_max + 1]: " + std::to_string(period_in[f]));
    // the token table: every token's frames by the centre rule, a running frame index per row (the centres ascend, and so do the ends)
    std::vector<VoiceTokRowDev> trd;
    std::vector<int32_t> fend;
    int64_t NT = 0;
    if (tok) {
        SBV2_REQUIRE(nrows == 0 || tok->counts, "voice: the token table needs the rows' token counts");
        trd.resize((size_t)nrows);
        for (int i = 0; i < nrows; ++i) {
            SBV2_REQUIRE(tok->counts[i] >= 0 && tok->counts[i] < (1 << 30), "voice: bad token count of row " + std::to_string(i));
            trd[i] = VoiceTokRowDev{NT, tok->counts[i]};
            NT += tok->counts[i];
            SBV2_REQUIRE(NT < (1 << 30), "voice: too many tokens in one call");
        }
        SBV2_REQUIRE(NT == 0 || tok->ends, "voice: the token table needs the tokens' ends");
        voice_tokens_check(tok->value, NT, tok->kind, tok->smooth, sp);
        fend.resize((size_t)NT);
        for (int i = 0; i < nrows; ++i) {
            int64_t f = 0, prev = 0;
            for (int64_t t = 0; t < trd[i].nt; ++t) {
                const int64_t e = tok->ends[trd[i].t_off + t];
                SBV2_REQUIRE(e >= prev, "voice: the token ends of row " + std::to_string(i) + " must ascend from 0");
                while (f < rd[i].nf && std::min(f * hop + hop / 2, rd[i].n - 1) < e) ++f;
                fend[(size_t)(trd[i].t_off + t)] = (int32_t)f;
                prev = e;
            }
        }
    }
    nrows_ = nrows;
    nf_ = NF;
    ncap_ = NCAP;
    nt_ = tok ? NT : -1;
    float* y = static_cast<float*>(out_.reserve(sizeof(float) * (size_t)std::max<int64_t>(span, 16), s));
    if (nrows == 0) return y;
    // device: rows | c3 | period | inc_a inc_s phi_a phi_s | lag yvoiced voiced off_a off_s | count | ta ts map   (8-byte parts first)
    const size_t nF = (size_t)NF, nC = (size_t)NCAP;
    const size_t o_c3 = round_up64(sizeof(VoiceRowDev) * nrows, 64), o_period = o_c3 + 24 * nF, o_i64 = o_period + 8 * nF, o_i32 = o_i64 + 32 * nF,
                 o_count = round_up64(o_i32 + 20 * nF, 64), o_marks = o_count + round_up64(16 * (size_t)nrows, 64),
                 o_cand_c3 = round_up64(o_marks + 12 * nC, 64), o_cand = o_cand_c3 + 24 * kTrackCand * nF,
                 bytes0 = tr && !period_in ? o_cand + 4 * kTrackRec * nF : o_marks + 12 * nC;
    // with a token table, behind everything else: token rows | value | fend (the upload) ; applied | src ; fq | ratio ; rho_t | fc | rho_f
    const size_t nT = (size_t)std::max<int64_t>(NT, 0), up_bytes = sizeof(VoiceTokRowDev) * (size_t)nrows + 12 * nT, o_up = round_up64(bytes0, 64),
                 o_tout = round_up64(o_up + up_bytes, 64), o_fq = o_tout + 16 * nT, o_ratio = o_fq + 8 * nF, o_rho_t = o_ratio + 8 * nF,
                 o_fc = o_rho_t + 4 * nT, o_rho_f = o_fc + 4 * nF, bytes = tok ? o_rho_f + 4 * nF : bytes0;
    // pinned: rows | period | voiced (the upload) ; period | voiced | count | ta ts map (the mirror)
    const size_t h_period_in = round_up64(sizeof(VoiceRowDev) * nrows, 64), h_voiced_in = h_period_in + 8 * nF, h_mirror = round_up64(h_voiced_in + 4 * nF, 64),
                 h_voiced = h_mirror + 8 * nF, h_count = round_up64(h_voiced + 4 * nF, 64), h_marks = h_count + round_up64(16 * (size_t)nrows, 64),
                 h_bytes0 = h_marks + 12 * nC;
    // ... ; token rows | value | fend (the upload) ; applied | src | ratio (the mirror)
    const size_t h_up = round_up64(h_bytes0, 64), h_tout = round_up64(h_up + up_bytes, 64), h_ratio = h_tout + 16 * nT,
                 h_bytes = tok ? h_ratio + 8 * nF : h_bytes0;
    char* d = static_cast<char*>(dev_.reserve(bytes, std::max<size_t>(bytes * 2, 65536), s));
    char* h = static_cast<char*>(host_.reserve(h_bytes, std::max<size_t>(h_bytes * 2, 65536), s));
    VoiceMarkArgs m{};
    m.rows = reinterpret_cast<const VoiceRowDev*>(d);
    double* c3 = reinterpret_cast<double*>(d + o_c3);
    m.c3 = c3;
    m.period = d_period_ = reinterpret_cast<double*>(d + o_period);
    m.inc_a = reinterpret_cast<int64_t*>(d + o_i64);
    m.inc_s = m.inc_a + nF;
    m.phi_a = m.inc_s + nF;
    m.phi_s = m.phi_a + nF;
    int32_t* lag = reinterpret_cast<int32_t*>(d + o_i32);
    int32_t* yvoiced = lag + nF;
    m.lag = lag;
    m.yvoiced = yvoiced;
    m.voiced = d_voiced_ = yvoiced + nF;
    m.off_a = m.voiced + nF;
    m.off_s = m.off_a + nF;
    m.count = d_count_ = reinterpret_cast<int32_t*>(d + o_count);
    m.ta = d_ta_ = reinterpret_cast<int32_t*>(d + o_marks);
    m.ts = d_ts_ = d_ta_ + nC;
    m.map = d_map_ = d_ts_ + nC;
    h_period_ = reinterpret_cast<double*>(h + h_mirror);
    h_voiced_ = reinterpret_cast<int32_t*>(h + h_voiced);
    h_count_ = reinterpret_cast<int32_t*>(h + h_count);
    h_ta_ = reinterpret_cast<int32_t*>(h + h_marks);
    h_ts_ = h_ta_ + nC;
    h_map_ = h_ts_ + nC;
    std::memcpy(h, rd.data(), sizeof(VoiceRowDev) * (size_t)nrows);
    HIP_CHECK(hipMemcpyAsync(d, h, sizeof(VoiceRowDev) * (size_t)nrows, hipMemcpyHostToDevice, s));
    m.given = period_in != nullptr;
    if (m.given && NF > 0) {
        std::memcpy(h + h_period_in, period_in, 8 * nF);
        std::memcpy(h + h_voiced_in, voiced_in, 4 * nF);
        HIP_CHECK(hipMemcpyAsync(m.period, h + h_period_in, 8 * nF, hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemcpyAsync(m.voiced, h + h_voiced_in, 4 * nF, hipMemcpyHostToDevice, s));
    } else if (tr) {   // every row's candidates besides, then one path per row through them (the rows' runs side by side)
        double* cand_c3 = reinterpret_cast<double*>(d + o_cand_c3);
        int32_t* cand = reinterpret_cast<int32_t*>(d + o_cand);
        for (int i = 0; i < nrows; ++i)
            pitch_launch(x + rd[i].off, kEncF32, rd[i].n, sp.pitch, c3 + 3 * rd[i].f_off, lag + rd[i].f_off, yvoiced + rd[i].f_off, s, tr->cand_max,
                         cand + kTrackRec * rd[i].f_off, cand_c3 + 3 * kTrackCand * rd[i].f_off);
        static_assert(sizeof(VoiceRowDev) % sizeof(int64_t) == 0 && offsetof(VoiceRowDev, f_off) % sizeof(int64_t) == 0, "the rows' first frames are read in place");
        track_.run(cand, cand_c3, NF, *tr, c3, lag, yvoiced, s, reinterpret_cast<const int64_t*>(d + offsetof(VoiceRowDev, f_off)),
                   (int)(sizeof(VoiceRowDev) / sizeof(int64_t)), nrows);
    } else {
        for (int i = 0; i < nrows; ++i)
            pitch_launch(x + rd[i].off, kEncF32, rd[i].n, sp.pitch, c3 + 3 * rd[i].f_off, lag + rd[i].f_off, yvoiced + rd[i].f_off, s);
    }
    m.sr = (double)sp.pitch.sample_rate;
    m.p = sp.pitch_scale;
    m.s = sp.intonation_scale;
    m.g_lo = sp.g_lo;
    m.g_hi = sp.g_hi;
    m.inc_u = sp.inc_u;
    m.hop = hop;
    m.tau_max = sp.pitch.tau_max;
    if (tok) {
        VoiceTokArgs t{};
        char* up = h + h_up;
        std::memcpy(up, trd.data(), sizeof(VoiceTokRowDev) * (size_t)nrows);
        if (nT) {
            std::memcpy(up + sizeof(VoiceTokRowDev) * (size_t)nrows, tok->value, 8 * nT);
            std::memcpy(up + sizeof(VoiceTokRowDev) * (size_t)nrows + 8 * nT, fend.data(), 4 * nT);
        }
        HIP_CHECK(hipMemcpyAsync(d + o_up, up, up_bytes, hipMemcpyHostToDevice, s));
        t.rows = reinterpret_cast<const VoiceTokRowDev*>(d + o_up);
        t.value = reinterpret_cast<const double*>(d + o_up + sizeof(VoiceTokRowDev) * (size_t)nrows);
        t.fend = reinterpret_cast<const int32_t*>(t.value + nT);
        t.applied = d_tout_ = reinterpret_cast<double*>(d + o_tout);
        t.src = t.applied + nT;
        t.fq = reinterpret_cast<int64_t*>(d + o_fq);
        t.ratio = d_ratio_ = reinterpret_cast<double*>(d + o_ratio);
        t.rho_t = reinterpret_cast<int32_t*>(d + o_rho_t);
        t.fc = reinterpret_cast<int32_t*>(d + o_fc);
        t.rho_f = reinterpret_cast<int32_t*>(d + o_rho_f);
        t.kind = tok->kind;
        t.smooth = tok->smooth;
        h_tout_ = reinterpret_cast<double*>(h + h_tout);
        h_ratio_ = reinterpret_cast<double*>(h + h_ratio);
        hipLaunchKernelGGL(k_voice_marks_tok, dim3((unsigned)nrows), dim3(kBlock), 0, s, m, t);
        HIP_CHECK(hipGetLastError());
        if (nT) HIP_CHECK(hipMemcpyAsync(h_tout_, d_tout_, 16 * nT, hipMemcpyDeviceToHost, s));   // applied | src: in pinned memory by the caller's synchronisation
    } else {
        hipLaunchKernelGGL(k_voice_marks, dim3((unsigned)nrows), dim3(kBlock), 0, s, m);
        HIP_CHECK(hipGetLastError());
    }
    if (longest > 0) {
        VoiceGatherArgs g{};
        g.rows = m.rows;
        g.x = x;
        g.y = y;
        g.ta = m.ta;
        g.ts = m.ts;
        g.map = m.map;
        g.count = m.count;
        g.half = sp.half;
        g.k0 = 0;
        g.k1 = longest;
        const dim3 grid((unsigned)((longest + kTile - 1) / kTile), (unsigned)nrows);
        if (fm) {
            VoiceFmtArgs f{};
            f.voiced = m.voiced;
            f.q = fm->scale;
            f.hop = hop;
            f.half = fm->half;
            hipLaunchKernelGGL(k_voice_gather_fmt, grid, dim3(kBlock), 0, s, g, f);
        } else {
            hipLaunchKernelGGL(k_voice_gather, grid, dim3(kBlock), 0, s, g);
        }
        HIP_CHECK(hipGetLastError());
    }
    // (the status of every row is looked at by the caller after its synchronisation)
    HIP_CHECK(hipMemcpyAsync(h_count_, d_count_, 16 * (size_t)nrows, hipMemcpyDeviceToHost, s));
    return y;
}

// ---- the fed shifter (StreamVoice, voice.h) ----
int64_t stream_voice_lookahead(const VoiceSpec& v, double formant_scale) {
    const int64_t W = v.half, G = (int64_t)std::ceil((double)W / std::min(formant_scale, 1.0)) + 1;
    const int64_t X = (int64_t)std::ceil((std::max(formant_scale, 1.0) - 1.0) * (double)W);   // an unvoiced grain is read up to q times as far
    return G + 2 * W + X + v.pitch.tau_max + v.pitch.hop / 2;
}

StreamVoiceSpec stream_voice_spec(int sample_rate, double pitch_scale, double intonation_scale, int64_t hop, double f0_min, double f0_max, double threshold,
                                  double formant_scale, const double* pivot, int64_t rows, double reserved0, double reserved1) {
    SBV2_REQUIRE(reserved0 == 0.0 && reserved1 == 0.0, "sbv2_stream_voice.reserved must be 0");   // (a NaN fails)
    StreamVoiceSpec sp;
    sp.voice = voice_spec(sample_rate, pitch_scale, intonation_scale, hop, f0_min, f0_max, threshold);
    sp.formant = formant_spec(formant_scale, 0.0, sp.voice);
    SBV2_REQUIRE(!(sp.voice.identity() && sp.formant.identity()),
                 "a stream voice with pitch_scale = intonation_scale = formant_scale = 1 shifts nothing: begin the stream without a voice");
    SBV2_REQUIRE(rows >= 0 && (pivot || rows == 0), "sbv2_stream_voice.pivot_hz must not be NULL (one entry per row: the f0 the intonation scale pivots about)");
    const double lo = 2.0 * sp.voice.g_lo, hi = sp.voice.g_hi / 2.0;   // (f0_min, f0_max after the defaults: halving and doubling are exact)
    for (int64_t i = 0; i < rows; ++i)   // (a NaN fails both comparisons)
        SBV2_REQUIRE(pivot[i] >= lo && pivot[i] <= hi, "sbv2_stream_voice.pivot_hz[" + std::to_string(i) + "] must be finite and in [f0_min, f0_max] = [" +
                                                           std::to_string(lo) + ", " + std::to_string(hi) + "] Hz: " + std::to_string(pivot[i]));
    sp.pivot.assign(pivot, pivot + rows);
    sp.lookahead = stream_voice_lookahead(sp.voice, formant_scale);
    return sp;
}

void StreamVoice::begin(const StreamVoiceSpec& sp, const VoiceRow* rows, int nrows, int64_t span, hipStream_t s, const double* period_in,
                        const int32_t* voiced_in) {
    SBV2_REQUIRE(nrows >= 0 && nrows <= 65535 && span >= 0 && (nrows == 0 || rows), "stream voice: bad rows");
    SBV2_REQUIRE((int64_t)sp.pivot.size() == nrows, "stream voice: one pivot per row");
    SBV2_REQUIRE(!period_in == !voiced_in, "stream voice: period_in and voiced_in are given together or not at all");
    sp_ = sp;
    const VoiceSpec& v = sp_.voice;
    const int64_t hop = v.pitch.hop;
    std::vector<VoiceRowDev> rd((size_t)nrows);
    rows_.assign((size_t)nrows, Row{});
    int64_t NF = 0, NCAP = 0;
    for (int i = 0; i < nrows; ++i) {
        SBV2_REQUIRE(rows[i].n >= 0 && rows[i].n < (1 << 30) && rows[i].off >= 0 && rows[i].off + rows[i].n <= span,
                     "stream voice: row " + std::to_string(i) + " is outside the buffer or longer than 2^30 samples");
        rd[i].off = rows[i].off;
        rd[i].n = rows[i].n;
        rd[i].f_off = NF;
        rd[i].nf = pitch_frames(rows[i].n, hop);
        rd[i].m_off = NCAP;
        rd[i].cap = rows[i].n / std::min(v.min_a, v.min_s) + rd[i].nf + 2;
        rows_[(size_t)i] = Row{rd[i].off, rd[i].n, NF, rd[i].nf, 0, 0, 0};
        NF += rd[i].nf;
        NCAP += rd[i].cap;
    }
    SBV2_REQUIRE(NF < (1 << 30) && NCAP < (int64_t(1) << 31), "stream voice: too many frames or marks in one stream");
    if (period_in)
        for (int64_t f = 0; f < NF; ++f)
            SBV2_REQUIRE(!voiced_in[f] || (period_in[f] >= v.pitch.tau_min - 1 && period_in[f] <= v.pitch.tau_max + 1),
                         "voice: period_in of voiced frame " + std::to_string(f) + " is outside [tau_min - 1, tau_max + 1]: " + std::to_string(period_in[f]));
    nf_ = NF;
    ncap_ = NCAP;
    given_ = period_in != nullptr;
    // device: rows | results | period | inc_a inc_s phi_a phi_s | voiced off_a off_s | count | state | ta ts map | x | y   (8-byte parts first)
    const size_t nF = (size_t)NF, nC = (size_t)NCAP, nR = (size_t)nrows, nS = (size_t)std::max<int64_t>(span, 16);
    o_res_ = round_up64(sizeof(VoiceRowDev) * nR, 64);
    o_period_ = o_res_ + sizeof(PitchFrame) * nF;
    o_i64_ = o_period_ + 8 * nF;
    o_i32_ = o_i64_ + 32 * nF;
    o_count_ = round_up64(o_i32_ + 12 * nF, 64);
    o_state_ = o_count_ + round_up64(16 * nR, 64);
    o_marks_ = o_state_ + round_up64(24 * nR, 64);
    const size_t o_x = round_up64(o_marks_ + 12 * nC, 64), o_y = o_x + round_up64(4 * nS, 64), bytes = o_y + 4 * nS;
    // pinned: rows | period | voiced (the upload) ; count (the mirror)
    const size_t h_period = round_up64(sizeof(VoiceRowDev) * nR, 64), h_voiced = h_period + 8 * nF, h_count = round_up64(h_voiced + 4 * nF, 64),
                 h_bytes = h_count + std::max<size_t>(16 * nR, 64);
    d_ = static_cast<char*>(dev_.reserve(bytes, std::max<size_t>(bytes + bytes / 4, 65536), s));
    char* h = static_cast<char*>(host_.reserve(h_bytes, std::max<size_t>(h_bytes * 2, 4096), s));
    // an earlier stream's uploads out of the pinned buffer are done (its event has long fired: no wait on the path to the first chunk)
    if (uploaded_) HIP_CHECK(hipEventSynchronize(uploaded_));
    x_ = reinterpret_cast<float*>(d_ + o_x);
    y_ = reinterpret_cast<float*>(d_ + o_y);
    h_count_ = reinterpret_cast<int32_t*>(h + h_count);
    if (nrows == 0) return;
    std::memcpy(h, rd.data(), sizeof(VoiceRowDev) * nR);
    HIP_CHECK(hipMemcpyAsync(d_, h, sizeof(VoiceRowDev) * nR, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemsetAsync(d_ + o_count_, 0, o_marks_ - o_count_, s));   // counts, status and every row's carried state
    if (given_ && NF > 0) {
        std::memcpy(h + h_period, period_in, 8 * nF);
        std::memcpy(h + h_voiced, voiced_in, 4 * nF);
        HIP_CHECK(hipMemcpyAsync(d_ + o_period_, h + h_period, 8 * nF, hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemcpyAsync(d_ + o_i32_, h + h_voiced, 4 * nF, hipMemcpyHostToDevice, s));
    }
    if (!uploaded_) HIP_CHECK(hipEventCreateWithFlags(&uploaded_, hipEventDisableTiming));
    HIP_CHECK(hipEventRecord(uploaded_, s));
}

StreamVoice::~StreamVoice() {
    if (uploaded_) (void)hipEventDestroy(uploaded_);
}

int64_t StreamVoice::final_after(int row, int64_t fed) const {
    const Row& r = rows_[(size_t)row];
    return fed >= r.n ? r.n : std::max<int64_t>(0, fed - sp_.lookahead);
}

int64_t StreamVoice::push(int row, const float* x, int64_t n, hipStream_t s) {
    SBV2_REQUIRE(row >= 0 && row < (int)rows_.size(), "internal: a voice push of a row the stream does not have");
    Row& r = rows_[(size_t)row];
    SBV2_REQUIRE(n >= 0 && r.fed + n <= r.n, "internal: a voice push of " + std::to_string(n) + " samples behind " + std::to_string(r.fed) + " of " +
                                                 std::to_string(r.n) + " of row " + std::to_string(row));
    const VoiceSpec& v = sp_.voice;
    if (n > 0) {
        SBV2_REQUIRE(x, "internal: no samples to push");
        HIP_CHECK(hipMemcpyAsync(x_ + r.off + r.fed, x, sizeof(float) * (size_t)n, hipMemcpyDeviceToDevice, s));
    }
    r.fed += n;
    const int64_t frames = pitch_frames_complete(v.pitch, r.n, r.fed);
    const size_t nF = (size_t)nf_, nC = (size_t)ncap_;
    const VoiceRowDev* d_rows = reinterpret_cast<const VoiceRowDev*>(d_) + row;
    int32_t* count = reinterpret_cast<int32_t*>(d_ + o_count_) + 4 * row;
    int32_t* ta = reinterpret_cast<int32_t*>(d_ + o_marks_);
    int32_t* voiced = reinterpret_cast<int32_t*>(d_ + o_i32_);
    if (frames > r.frames) {
        PitchFrame* res = reinterpret_cast<PitchFrame*>(d_ + o_res_);
        if (!given_) pitch_launch_fed(x_ + r.off, r.fed, r.n, v.pitch, r.frames, frames - r.frames, res + r.f_off, s);
        VoiceMarkArgs m{};
        m.rows = d_rows;
        m.given = given_;
        m.period = reinterpret_cast<double*>(d_ + o_period_);
        m.voiced = voiced;
        m.inc_a = reinterpret_cast<int64_t*>(d_ + o_i64_);
        m.inc_s = m.inc_a + nF;
        m.phi_a = m.inc_s + nF;
        m.phi_s = m.phi_a + nF;
        m.off_a = voiced + nF;
        m.off_s = m.off_a + nF;
        m.ta = ta;
        m.ts = ta + nC;
        m.map = m.ts + nC;
        m.count = count;
        m.sr = (double)v.pitch.sample_rate;
        m.p = v.pitch_scale;
        m.s = v.intonation_scale;
        m.g_lo = v.g_lo;
        m.g_hi = v.g_hi;
        m.inc_u = v.inc_u;
        m.hop = v.pitch.hop;
        m.tau_max = v.pitch.tau_max;
        VoiceFedArgs d{};
        d.res = res;
        d.state = reinterpret_cast<int64_t*>(d_ + o_state_) + 3 * row;
        d.pivot = sp_.pivot[(size_t)row];
        d.f0 = r.frames;
        d.f1 = frames;
        d.last = frames == r.nf;
        hipLaunchKernelGGL(k_voice_marks_fed, dim3(1), dim3(kBlock), 0, s, m, d);
        HIP_CHECK(hipGetLastError());
        r.frames = frames;
    }
    const int64_t fin = final_after(row, r.fed);
    if (fin > r.done) {
        VoiceGatherArgs g{};
        g.rows = d_rows;
        g.x = x_;
        g.y = y_;
        g.ta = ta;
        g.ts = ta + nC;
        g.map = g.ts + nC;
        g.count = count;
        g.half = v.half;
        g.k0 = r.done;
        g.k1 = fin;
        const dim3 grid((unsigned)((fin - r.done + Voice::kTile - 1) / Voice::kTile), 1);
        if (!sp_.formant.identity()) {
            VoiceFmtArgs f{};
            f.voiced = voiced;
            f.q = sp_.formant.scale;
            f.hop = v.pitch.hop;
            f.half = sp_.formant.half;
            hipLaunchKernelGGL(k_voice_gather_fmt, grid, dim3(kBlock), 0, s, g, f);
        } else {
            hipLaunchKernelGGL(k_voice_gather, grid, dim3(kBlock), 0, s, g);
        }
        HIP_CHECK(hipGetLastError());
        r.done = fin;
    }
    return fin;
}

void StreamVoice::status_to_host(hipStream_t s) {
    if (!rows_.empty()) HIP_CHECK(hipMemcpyAsync(h_count_, d_ + o_count_, 16 * rows_.size(), hipMemcpyDeviceToHost, s));
}

void Voice::results_to_host(hipStream_t s) {
    if (nrows_ == 0) return;
    if (nf_) {
        HIP_CHECK(hipMemcpyAsync(h_period_, d_period_, 8 * (size_t)nf_, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipMemcpyAsync(h_voiced_, d_voiced_, 4 * (size_t)nf_, hipMemcpyDeviceToHost, s));
    }
    if (ncap_) HIP_CHECK(hipMemcpyAsync(h_ta_, d_ta_, 12 * (size_t)ncap_, hipMemcpyDeviceToHost, s));
    if (nt_ >= 0 && nf_) HIP_CHECK(hipMemcpyAsync(h_ratio_, d_ratio_, 8 * (size_t)nf_, hipMemcpyDeviceToHost, s));
}

}  // namespace sbv2
