// Per-token volume targets on gfx950: the level of every token's span, the factors, and the gain curve applied to the rows (token_gain.h has
// the stage's place in a fetch and the tile rule; include/sbv2_hip.h above sbv2_token_gain has the definition these kernels restate).
//
// k_tgain_level.  The summation order of a span of `len` samples, stated in the header so that a restatement can follow it: with stride = 64
// (len <= kLongSpan) or 256 (longer), lane l adds the squares at offsets l, l + stride, l + 2 stride, ... in ascending order, each square an
// exact f64 product of an f32 sample; the 64 partial sums of a wave meet in the tree d = 32, 16, ..., 1 (lane i += lane i + d); the four waves
// of a long span are added in wave order.  The order depends on the span's length alone.  It is the order of the marks reduction (marks.hip)
// with its own kernel: the marks' bits and launches stay what they are, and this one reads f32 rows only and forms no peak.
//
// k_tgain_factors.  One lane per token, f64 add / multiply / divide / sqrt / compare only (this file is compiled without contraction): every
// operation is correctly rounded and numpy gives the same bits.  It leaves one 32-byte record {E, g, R} per token: the sample of its row the
// token ends at, its factor, and the ramp length at that end (0 at a row's last token).
//
// k_tgain_apply.  A workgroup owns one tile of one row.  A sample n of token t is moved by at most one ramp, the one at its left end (n < E[t-1]
// + R[t-1] / 2) or the one at its right end (n >= E[t] - R[t] / 2): R <= the lengths of both neighbours, so the two never meet.  The gain of a
// sample therefore needs the records t - 1, t and t + 1 and nothing else.  The workgroup bisects the row's ends once for the first token
// that ends behind the tile's first sample, stages that token's left neighbour and the kStage - 1 records behind it in LDS (768 bytes), and
// every lane then walks the staged ends forward as its samples ascend: no lane touches the table in HBM again.  A lane takes 16-byte groups
// of 4 consecutive samples, 256 lanes side by side (4 KB contiguous per load instruction), the tile's second half in a second round.  A
// group that lies inside one token's flat part takes four conversions, four f64 multiplies by one g and one 16-byte store; a group that
// meets a ramp or a boundary forms g(n) per sample.  Groups are aligned to 16 BYTES, not to the tile: a row whose head in the packed buffer
// is off by m floats has its groups shifted left by m, and the two groups that hang over the tile's ends move their samples one by one.
// HBM traffic: 4 bytes in and 4 bytes out per sample, the records through L2 once per tile.
#include "token_gain.h"

#include <cmath>
#include <cstring>

namespace sbv2 {

TokenGainSpec token_gain_spec(const double* value, int64_t n_tokens, int kind, int64_t ramp, double max_ratio, int64_t reserved) {
    SBV2_REQUIRE(reserved == 0, "sbv2_token_gain.reserved must be 0");
    SBV2_REQUIRE(n_tokens >= 0 && n_tokens < (1 << 30), "sbv2_token_gain.n_tokens must be in [0, 2^30): " + std::to_string(n_tokens));
    SBV2_REQUIRE(value || n_tokens == 0, "sbv2_token_gain.value must not be NULL");
    SBV2_REQUIRE(kind == 0 || kind == 1, "sbv2_token_gain.kind must be 0 (ratio) or 1 (target RMS): " + std::to_string(kind));
    SBV2_REQUIRE(ramp >= 0 && ramp < (1 << 30), "sbv2_token_gain.ramp must be in [0, 2^30) native samples: " + std::to_string(ramp));
    SBV2_REQUIRE(max_ratio >= 1.0 && std::isfinite(max_ratio), "sbv2_token_gain.max_ratio must be finite and >= 1: " + std::to_string(max_ratio));
    TokenGainSpec sp{value, n_tokens, kind, ramp, max_ratio, false};
    for (int64_t t = 0; t < n_tokens; ++t) {
        SBV2_REQUIRE(value[t] >= 0.0 && std::isfinite(value[t]),
                     "sbv2_token_gain.value[" + std::to_string(t) + "] must be finite and >= 0 (0 = token not edited): " + std::to_string(value[t]));
        sp.edits = sp.edits || (value[t] != 0.0 && !(kind == 0 && value[t] == 1.0));
    }
    return sp;
}

namespace {

constexpr int kBlock = 256, kWave = 64, kWavesPerBlock = kBlock / kWave;
constexpr int kTile = TokenGain::kTile, kStage = TokenGain::kStage;
static_assert(kTile % 512 == 0 && kTile % (4 * kBlock) == 0, "a tile is a whole number of hops and of 16-byte rounds");

struct RowDev {
    int64_t off, n;       // the row in the packed buffer
    int64_t tok0, ntok;   // its tokens in the tables
    int64_t tile0;        // its first workgroup of k_tgain_apply
};
struct Rec {
    int64_t E;   // the sample of its row the token ends at
    double g;    // its factor, clamped
    int64_t R;   // the ramp length at E: even, <= both neighbours' lengths, 0 at a row's last token
    int64_t pad;
};
struct Tables {
    const int64_t* ends;       // [nt], relative to the token's row
    const double* value;       // [nt]
    const int32_t* tok_row;    // [nt]
    const int32_t* order;      // [nt]: the short spans' tokens, then the long ones'
    const RowDev* rows;        // [nrows]
    const int32_t* tile_row;   // [tiles]
    double* ss;                // [nt]
    Rec* rec;                  // [nt]
    double* applied;           // [nt]
    double* rms;               // [nt]
};

__global__ __launch_bounds__(kBlock) void k_tgain_level(const float* __restrict__ x, const Tables a, const int nshort, const int short_blocks) {
    __shared__ double sh[kWavesPerBlock];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const bool whole_block = (int)blockIdx.x >= short_blocks;   // uniform over the workgroup
    int k, first, stride;
    if (whole_block) {
        k = nshort + ((int)blockIdx.x - short_blocks);
        first = threadIdx.x;
        stride = kBlock;
    } else {
        k = (int)blockIdx.x * kWavesPerBlock + wave;
        if (k >= nshort) return;   // (no barrier on this path)
        first = lane;
        stride = kWave;
    }
    const int t = a.order[k];
    const RowDev r = a.rows[a.tok_row[t]];
    const int64_t s0 = t == r.tok0 ? 0 : a.ends[t - 1], len = a.ends[t] - s0;
    const float* p = x + r.off + s0;
    double ss = 0.0;
    int64_t i = first;
    for (; i + 3 * stride < len; i += 4 * stride) {   // four independent loads in flight per lane, added in ascending order
        const double v0 = (double)p[i], v1 = (double)p[i + stride], v2 = (double)p[i + 2 * stride], v3 = (double)p[i + 3 * stride];
        ss += v0 * v0;
        ss += v1 * v1;
        ss += v2 * v2;
        ss += v3 * v3;
    }
    for (; i < len; i += stride) {
        const double v = (double)p[i];
        ss += v * v;
    }
#pragma unroll
    for (int d = kWave / 2; d >= 1; d >>= 1) ss += __shfl_down(ss, d, kWave);
    if (!whole_block) {
        if (lane == 0) a.ss[t] = ss;
        return;
    }
    if (lane == 0) sh[wave] = ss;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = sh[0];
        for (int w = 1; w < kWavesPerBlock; ++w) s += sh[w];
        a.ss[t] = s;
    }
}

__global__ __launch_bounds__(kBlock) void k_tgain_factors(const Tables a, const int64_t nt, const int kind, const int64_t ramp, const double lo,
                                                          const double hi) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= nt) return;
    const RowDev r = a.rows[a.tok_row[t]];
    const bool last = t == r.tok0 + r.ntok - 1;
    const int64_t E = a.ends[t], len = E - (t == r.tok0 ? 0 : a.ends[t - 1]);
    const double M = len > 0 ? a.ss[t] / (double)len : 0.0;
    const double rms = sqrt(M), v = a.value[t];
    double g = 1.0;
    if (v != 0.0 && len > 0 && M != 0.0) g = kind == 0 ? v : v / rms;
    g = g < lo ? lo : g;
    g = g > hi ? hi : g;
    int64_t R = 0;
    if (!last) {
        const int64_t next = a.ends[t + 1] - E;
        R = ramp < len ? ramp : len;
        R = (R < next ? R : next) & ~(int64_t)1;
    }
    a.rec[t] = Rec{E, g, R, 0};
    a.applied[t] = g;
    a.rms[t] = rms;
}

// g(n) inside the ramp about boundary b, in the stated order of operations
__device__ __forceinline__ double ramp_gain(int64_t n, int64_t b, int64_t R, double ga, double gb) {
    const double u = (double)(2 * (n - b) + R + 1) / (double)(2 * R);
    const double w = (u * u) * (3.0 - 2.0 * u);
    return ga + (gb - ga) * w;
}

// The four samples [q, q + 4) of a row under the records r[0 .. lim): r[0] is the row's first token or the left neighbour of the first token
// that can hold a sample of this tile; r[last] is the row's last token (last < 0: it is not among them, and no sample here reaches it).
// i: a record index at or before the token of the group's first sample; it is walked forward and returned.  [c0, c1) clips the group to the
// samples that are the tile's; vec: the group is whole and both of its addresses are 16-byte aligned.
__device__ __forceinline__ int gain_group(const Rec* r, int lim, int last, int i, const float* __restrict__ xr, float* __restrict__ yr, int64_t q,
                                          int64_t c0, int64_t c1, bool vec, int64_t row_n) {
    const int64_t n0 = q > c0 ? q : c0, n1 = q + 4 < c1 ? q + 4 : c1;   // the group's own samples
    if (n0 >= n1) return i;
    float v[4];
    if (vec) {
        const float4 in = *reinterpret_cast<const float4*>(xr + q);
        v[0] = in.x, v[1] = in.y, v[2] = in.z, v[3] = in.w;
    } else {
        for (int k = 0; k < 4; ++k) v[k] = (q + k >= n0 && q + k < n1) ? xr[q + k] : 0.0f;
    }
    if (lim == 0) {   // a row without tokens: nothing to edit
        for (int k = 0; k < 4; ++k) v[k] = (float)((double)v[k] * 1.0);
    } else {
        while (i < lim - 1 && r[i].E <= n0) ++i;
        const int64_t flat_lo = i > 0 ? r[i - 1].E + r[i - 1].R / 2 : 0;
        const int64_t flat_hi = i == last ? row_n : r[i].E - r[i].R / 2;
        if (n0 >= flat_lo && n1 <= flat_hi) {   // the one-multiply path
            const double g = r[i].g;
            for (int k = 0; k < 4; ++k) v[k] = (float)((double)v[k] * g);
        } else {
            int j = i;
            for (int k = 0; k < 4; ++k) {
                const int64_t n = q + k;
                if (n < n0 || n >= n1) continue;
                while (j < lim - 1 && r[j].E <= n) ++j;
                double g = r[j].g;
                if (j > 0 && r[j - 1].R > 0 && n < r[j - 1].E + r[j - 1].R / 2) g = ramp_gain(n, r[j - 1].E, r[j - 1].R, r[j - 1].g, g);
                else if (r[j].R > 0 && n >= r[j].E - r[j].R / 2) g = ramp_gain(n, r[j].E, r[j].R, g, r[j + 1].g);   // (R > 0: j + 1 is in the row)
                v[k] = (float)((double)v[k] * g);
            }
        }
    }
    if (vec) {
        *reinterpret_cast<float4*>(yr + q) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
        for (int k = 0; k < 4; ++k)
            if (q + k >= n0 && q + k < n1) yr[q + k] = v[k];
    }
    return i;
}

__global__ __launch_bounds__(kBlock) void k_tgain_apply(const float* __restrict__ x, float* __restrict__ y, const Tables a) {
    __shared__ Rec sh[kStage];
    const RowDev row = a.rows[a.tile_row[blockIdx.x]];
    const int64_t p0 = ((int64_t)blockIdx.x - row.tile0) * kTile, p1 = p0 + kTile < row.n ? p0 + kTile : row.n;
    const float* xr = x + row.off;
    float* yr = y + row.off;
    // the first token that ends behind p0 (the row's last one when none does), by one bisection of the row's ends: uniform, scalar loads
    const int64_t* ends = a.ends + row.tok0;
    int64_t lo = 0, hi = row.ntok;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (ends[mid] > p0) hi = mid;
        else lo = mid + 1;
    }
    const int64_t t0 = lo < row.ntok ? lo : row.ntok - 1;
    const int64_t s0 = t0 > 0 ? t0 - 1 : 0;
    const int cnt = (int)(row.ntok - s0 < kStage ? row.ntok - s0 : kStage);   // (0 for a row without tokens)
    if ((int)threadIdx.x < cnt) sh[threadIdx.x] = a.rec[row.tok0 + s0 + threadIdx.x];
    __syncthreads();
    const bool to_end = s0 + cnt == row.ntok;
    const bool staged = to_end || sh[cnt - 2].E >= p1;   // (not to_end: cnt = kStage; record cnt - 2 covers the tile, cnt - 1 is its right neighbour)
    // 16-byte groups: sample p of the row is aligned iff (p + mis) % 4 == 0, so the groups start at p0 - mis + 4 j
    const int mis_x = (int)((reinterpret_cast<uintptr_t>(xr) >> 2) & 3), mis_y = (int)((reinterpret_cast<uintptr_t>(yr) >> 2) & 3);
    const bool aligned = mis_x == mis_y;   // (the stage's buffer is laid out like its input: always, unless the input's base is odd)
    const int mis = aligned ? mis_x : 0;
    const int groups = (kTile + mis + 3) / 4;   // kTile / 4, and one more for a shifted row
    int i = 0;
    for (int j = threadIdx.x; j < groups; j += kBlock) {
        const int64_t q = p0 - mis + 4 * (int64_t)j;
        const bool vec = aligned && q >= p0 && q + 4 <= p1;
        if (staged) {
            i = gain_group(sh, cnt, to_end ? cnt - 1 : -1, i, xr, yr, q, p0, p1, vec, row.n);
        } else {   // more zero-duration tokens than the stage holds: the table in HBM, a bisection per group
            const int64_t n0 = q > p0 ? q : p0;
            int64_t l = 0, h = row.ntok;
            while (l < h) {
                const int64_t mid = (l + h) >> 1;
                if (ends[mid] > n0) h = mid;
                else l = mid + 1;
            }
            (void)gain_group(a.rec + row.tok0, (int)row.ntok, (int)row.ntok - 1, (int)(l < row.ntok ? l : row.ntok - 1), xr, yr, q, p0, p1, vec, row.n);
        }
    }
}

inline size_t up64(size_t v) { return (v + 63) & ~(size_t)63; }

}  // namespace

const float* TokenGain::run(const float* x, int64_t total, const TokenGainRow* rows, int nrows, const int64_t* tok_counts, const int64_t* tok_ends,
                            const TokenGainSpec& sp, hipStream_t s) {
    SBV2_REQUIRE(nrows >= 0 && total >= 0 && (x || total == 0) && (nrows == 0 || (rows && tok_counts)), "internal: bad token gain arguments");
    const int64_t nt = sp.n_tokens;
    SBV2_REQUIRE(nt >= 0 && nt < (1 << 30) && (nt == 0 || (tok_ends && sp.value)), "internal: bad token gain table");
    // every address the kernels form is decided here: the rows inside the buffer, the ends inside their rows
    int64_t tiles = 0, nshort = 0;
    for (int64_t k = 0, e = 0; k < nrows; ++k) {
        SBV2_REQUIRE(rows[k].n >= 0 && rows[k].off >= 0 && rows[k].off <= total - rows[k].n, "internal: row " + std::to_string(k) + " is outside the buffer");
        SBV2_REQUIRE(tok_counts[k] >= 0 && tok_counts[k] <= nt - e, "the rows' token counts exceed sbv2_token_gain.n_tokens");
        for (int64_t t = 0, prev = 0; t < tok_counts[k]; ++t, ++e) {
            SBV2_REQUIRE(tok_ends[e] >= prev && tok_ends[e] <= rows[k].n, "the token ends of row " + std::to_string(k) + " must ascend within its " +
                                                                              std::to_string(rows[k].n) + " samples");
            nshort += tok_ends[e] - prev <= kLongSpan;
            prev = tok_ends[e];
        }
        tiles += (rows[k].n + kTile - 1) / kTile;
        if (k == nrows - 1) SBV2_REQUIRE(e == nt, "sbv2_token_gain.n_tokens is " + std::to_string(nt) + " but the rows have " + std::to_string(e) + " tokens");
    }
    SBV2_REQUIRE(nrows > 0 || nt == 0, "sbv2_token_gain.n_tokens is " + std::to_string(nt) + " but there are no rows");
    SBV2_REQUIRE(tiles < (1LL << 31), "internal: too many tiles");
    nt_ = nt;
    // ends | value | tok_row | order | rows | tile_row (uploaded) | ss | rec | applied | rms; the pinned buffer holds the uploaded part and,
    // at o_res, the mirror of applied | rms
    const size_t n = (size_t)nt;
    const size_t o_val = up64(8 * n), o_trow = o_val + up64(8 * n), o_order = o_trow + up64(4 * n), o_rows = o_order + up64(4 * n);
    const size_t o_tile = o_rows + up64(sizeof(RowDev) * (size_t)nrows), o_up = o_tile + up64(4 * (size_t)tiles);
    const size_t o_ss = o_up, o_rec = o_ss + up64(8 * n), o_res = o_rec + up64(sizeof(Rec) * n), bytes = o_res + 16 * n + 64;
    char* h = static_cast<char*>(host_.reserve(bytes, std::max<size_t>(bytes * 2, 4096), s));
    char* d = static_cast<char*>(dev_.reserve(bytes, std::max<size_t>(bytes * 2, 4096), s));
    float* y = static_cast<float*>(out_.reserve(sizeof(float) * (size_t)std::max<int64_t>(total, 4), s));
    if (nt) std::memcpy(h, tok_ends, 8 * n), std::memcpy(h + o_val, sp.value, 8 * n);
    int32_t* tok_row = reinterpret_cast<int32_t*>(h + o_trow);
    int32_t* order = reinterpret_cast<int32_t*>(h + o_order);
    RowDev* hrows = reinterpret_cast<RowDev*>(h + o_rows);
    int32_t* tile_row = reinterpret_cast<int32_t*>(h + o_tile);
    int64_t ks = 0, kl = nshort, tile = 0;
    for (int64_t k = 0, e = 0; k < nrows; ++k) {
        hrows[k] = RowDev{rows[k].off, rows[k].n, e, tok_counts[k], tile};
        for (int64_t t = 0, prev = 0; t < tok_counts[k]; ++t, ++e) {
            tok_row[e] = (int32_t)k;
            (tok_ends[e] - prev <= kLongSpan ? order[ks++] : order[kl++]) = (int32_t)e;
            prev = tok_ends[e];
        }
        for (int64_t i = 0; i < (rows[k].n + kTile - 1) / kTile; ++i) tile_row[tile++] = (int32_t)k;
    }
    res_host_ = reinterpret_cast<double*>(h + o_res);
    if (o_up) HIP_CHECK(hipMemcpyAsync(d, h, o_up, hipMemcpyHostToDevice, s));
    Tables a;
    a.ends = reinterpret_cast<const int64_t*>(d);
    a.value = reinterpret_cast<const double*>(d + o_val);
    a.tok_row = reinterpret_cast<const int32_t*>(d + o_trow);
    a.order = reinterpret_cast<const int32_t*>(d + o_order);
    a.rows = reinterpret_cast<const RowDev*>(d + o_rows);
    a.tile_row = reinterpret_cast<const int32_t*>(d + o_tile);
    a.ss = reinterpret_cast<double*>(d + o_ss);
    a.rec = reinterpret_cast<Rec*>(d + o_rec);
    a.applied = reinterpret_cast<double*>(d + o_res);
    a.rms = a.applied + nt;
    if (nt) {
        const int short_blocks = (int)((nshort + kWavesPerBlock - 1) / kWavesPerBlock);
        hipLaunchKernelGGL(k_tgain_level, dim3((unsigned)(short_blocks + (nt - nshort))), dim3(kBlock), 0, s, x, a, (int)nshort, short_blocks);
        HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(k_tgain_factors, dim3((unsigned)((nt + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, a, nt, sp.kind, sp.ramp,
                           1.0 / sp.max_ratio, sp.max_ratio);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(res_host_, a.applied, 16 * n, hipMemcpyDeviceToHost, s));
    }
    if (tiles) {
        hipLaunchKernelGGL(k_tgain_apply, dim3((unsigned)tiles), dim3(kBlock), 0, s, x, y, a);
        HIP_CHECK(hipGetLastError());
    }
    return y;
}

}  // namespace sbv2
