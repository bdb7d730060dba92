// Parametric EQ on gfx950: a cascade of S <= 8 biquads in f64 over the listed rows' native f32 samples (eq.h has the stage's place in a fetch,
// the split into tiles and lanes and the LDS budget; include/sbv2_hip.h above sbv2_eq has the definition these kernels restate).
//
// The section step (eq_step) is kw_step of kweight.h for S sections: w = fma(b0, x, s0); s0 = fma(b1, x, fma(-a1, w, s1)); s1 = fma(b2, x,
// -a2 w); the next section's x is w.  f64 add, multiply and fma only.
//
// A tile in LDS.  The tile's samples are staged once with 16-byte loads, 256 lanes side by side; sample p lies at word p + p / kLane, i.e.
// lane t's kLane samples at a row stride of kLane + 1 words, so the lanes' serial walks meet 64 different banks.  Groups are aligned to 16
// BYTES, not to the tile: a row whose head is off the 16-byte grid takes scalar loads (and stores) at the tile's two edges.  Samples behind
// the row's end are staged as zeros; they feed lanes whose results nobody reads.
//
// k_eq_apply, per workgroup: (1) stage; (2) every lane runs the cascade over its samples from zero state (lane 0: from the tile's entry
// state) -> its e; (3) eight Kogge-Stone steps v_t += M_{kLane 2^k} v_{t - 2^k} through the exchange buffer [N][256] (conflict-free), the
// matrix a broadcast read from LDS -> v_t = the state at lane t's end; (4) lane t reruns its samples from v_{t-1}, writes y64 if asked and
// float(w) over its words in LDS; (5) the tile leaves with 16-byte stores.  The partials of (2) are recomputed here, not stored by
// k_eq_tiles: storing them would add 16 N bytes of HBM traffic per kLane samples (S = 8: as much again as the samples).
// k_eq_tiles is (1) - (3) from zero state; lane 255's v is the tile's e.  k_eq_carry walks a row's tiles with the lanes as matrix rows and a
// shuffle for the product.
#include "eq.h"

#include <cmath>
#include <cstring>

namespace sbv2 {

EqSpec eq_spec(int n_bands, const int32_t* kind, const double* f0_hz, const double* gain_db, const double* q, int reserved, int rate) {
    SBV2_REQUIRE(reserved == 0, "sbv2_eq.reserved must be 0");
    SBV2_REQUIRE(n_bands >= 0 && n_bands <= kEqMaxBands, "sbv2_eq.n_bands must be in [0, 8]: " + std::to_string(n_bands));
    SBV2_REQUIRE(rate > 0, "sbv2_eq_design: rate must be positive: " + std::to_string(rate));
    EqSpec sp;
    sp.n_bands = n_bands;
    const double pi = 3.14159265358979323846;
    for (int b = 0; b < n_bands; ++b) {
        const std::string at = "[" + std::to_string(b) + "]";
        const int k = kind[b];
        const double f = f0_hz[b], g = gain_db[b], Q = q[b];
        SBV2_REQUIRE(k >= 0 && k <= 4, "sbv2_eq.kind" + at + " must be 0 (high-pass), 1 (low-pass), 2 (low shelf), 3 (high shelf) or 4 (peak): " +
                                           std::to_string(k));
        SBV2_REQUIRE(f >= 10.0 && f <= 0.45 * rate, "sbv2_eq.f0_hz" + at + " must be in [10, " + std::to_string(0.45 * rate) + "]: " + std::to_string(f));
        SBV2_REQUIRE(g >= -24.0 && g <= 24.0, "sbv2_eq.gain_db" + at + " must be in [-24, 24]: " + std::to_string(g));
        SBV2_REQUIRE(k >= 2 || g == 0.0, "sbv2_eq.gain_db" + at + " must be 0 for a high-pass or low-pass: " + std::to_string(g));
        SBV2_REQUIRE(Q >= 0.1 && Q <= 20.0, "sbv2_eq.q" + at + " must be in [0.1, 20]: " + std::to_string(Q));
        sp.filters = sp.filters || k < 2 || g != 0.0;
        const double w0 = 2.0 * pi * f / rate, cs = std::cos(w0), alpha = std::sin(w0) / (2.0 * Q), A = std::pow(10.0, g / 40.0);
        const double h = std::sin(0.5 * w0), omc = 2.0 * h * h;   // 1 - cos(w0) without the cancellation at low f0
        double b0, b1, b2, a0, a1, a2;
        if (k == 0) {
            b0 = 0.5 * (1.0 + cs), b1 = -(1.0 + cs), b2 = b0, a0 = 1.0 + alpha, a1 = -2.0 * cs, a2 = 1.0 - alpha;
        } else if (k == 1) {
            b0 = 0.5 * omc, b1 = omc, b2 = b0, a0 = 1.0 + alpha, a1 = -2.0 * cs, a2 = 1.0 - alpha;
        } else if (k == 4) {
            b0 = 1.0 + alpha * A, b1 = -2.0 * cs, b2 = 1.0 - alpha * A, a0 = 1.0 + alpha / A, a1 = -2.0 * cs, a2 = 1.0 - alpha / A;
        } else {
            const double r = 2.0 * std::sqrt(A) * alpha, sg = k == 2 ? 1.0 : -1.0;   // the high shelf is the low shelf with cos -> -cos, z -> -z
            const double p = (A + 1.0) - sg * (A - 1.0) * cs, m = (A + 1.0) + sg * (A - 1.0) * cs;
            b0 = A * (p + r), b1 = sg * 2.0 * A * ((A - 1.0) - sg * (A + 1.0) * cs), b2 = A * (p - r);
            a0 = m + r, a1 = -sg * 2.0 * ((A - 1.0) + sg * (A + 1.0) * cs), a2 = m - r;
        }
        double* c = sp.coef + 5 * b;
        c[0] = b0 / a0, c[1] = b1 / a0, c[2] = b2 / a0, c[3] = a1 / a0, c[4] = a2 / a0;
    }
    return sp;
}

// The powers are squared in long double and rounded to f64 once each.  The cascade's transition is far from normal (a 20 Hz high-pass has a
// pole pair next to 1, and eight sections feed one another), and 6 to 14 squarings in f64 itself leave an error in M_m that the scan then
// multiplies into every state: measured on the 8-band set of tests/test_eq.py, 1.2e-10 against the sample-by-sample f64 cascade's 1.2e-12.
// With the extended format's 11 more bits the matrices are exact to an f64 ulp and the scan's own rounding is what remains.
void eq_powers(const EqSpec& sp, double* pw) {
    using real = long double;
    const int N = 2 * sp.n_bands;
    std::vector<real> A((size_t)N * N), B((size_t)N * N);
    for (int j = 0; j < N; ++j) {   // column j of the one-sample transition: the section step on unit vector j with zero input
        real s[2 * kEqMaxBands] = {0};
        s[j] = 1.0L;
        real x = 0.0L;
        for (int b = 0; b < sp.n_bands; ++b) {
            const double* c = sp.coef + 5 * b;
            const real w = (real)c[0] * x + s[2 * b];
            s[2 * b] = (real)c[1] * x - (real)c[3] * w + s[2 * b + 1];
            s[2 * b + 1] = (real)c[2] * x - (real)c[4] * w;
            x = w;
        }
        for (int i = 0; i < N; ++i) A[(size_t)i * N + j] = s[i];
    }
    auto square = [&](std::vector<real>& X, std::vector<real>& R) {
        for (int i = 0; i < N; ++i)
            for (int j = 0; j < N; ++j) {
                real a = 0.0L;
                for (int k = 0; k < N; ++k) a += X[(size_t)i * N + k] * X[(size_t)k * N + j];
                R[(size_t)i * N + j] = a;
            }
        X.swap(R);
    };
    for (int m = 1; m < Eq::kLane; m *= 2) square(A, B);
    for (int k = 0; k <= 8; ++k) {
        for (int i = 0; i < N * N; ++i) pw[(size_t)k * N * N + i] = (double)A[i];
        square(A, B);
    }
}

namespace {

constexpr int kBlock = 256, kWave = 64, kSteps = 8;
constexpr int kLane = Eq::kLane, kTile = Eq::kTile;
constexpr int kTileWords = kBlock * (kLane + 1);
static_assert(kTile == kBlock * kLane && (1 << kSteps) == kBlock && kLane % 4 == 0 && (kTileWords * 4) % 8 == 0, "the tile rule of eq.h");

struct RowDev {
    int64_t off, n;   // the row in the packed buffer
    int64_t tile0;    // its first tile
};
struct Tables {
    const RowDev* rows;        // [nrows]
    const int32_t* tile_row;   // [tiles]
    const double* coef;        // [5 S]
    const double* pw;          // [9][N N]
    double* tile_e;            // [tiles][N]: a tile's end state from zero entry (tiles with a successor)
    double* entry;             // [tiles][N]: the state a tile is entered with (tiles behind a row's first)
};

constexpr size_t eq_lds_bytes(int S) { return sizeof(float) * kTileWords + sizeof(double) * (size_t)(kSteps * 4 * S * S + 2 * S * kBlock); }

__device__ __forceinline__ int word_of(int p) { return p + p / kLane; }

template <int S>
__device__ __forceinline__ double eq_step(const double (&c)[5 * S], double (&s)[2 * S], double x) {
#pragma unroll
    for (int k = 0; k < S; ++k) {
        const double w = fma(c[5 * k], x, s[2 * k]);
        s[2 * k] = fma(c[5 * k + 1], x, fma(-c[5 * k + 3], w, s[2 * k + 1]));
        s[2 * k + 1] = fma(c[5 * k + 2], x, -c[5 * k + 4] * w);
        x = w;
    }
    return x;
}

// the tile's cnt samples at g into sh, zeros behind them
__device__ __forceinline__ void stage_tile(float* sh, const float* __restrict__ g, int cnt) {
    const int t = threadIdx.x;
    const int lead = (int)((4 - ((reinterpret_cast<uintptr_t>(g) >> 2) & 3)) & 3), a = lead < cnt ? lead : cnt, groups = (cnt - a) / 4;
    if (t < a) sh[word_of(t)] = g[t];
    for (int j = t; j < groups; j += kBlock) {
        const int p = a + 4 * j;
        const float4 v = *reinterpret_cast<const float4*>(g + p);
        sh[word_of(p)] = v.x, sh[word_of(p + 1)] = v.y, sh[word_of(p + 2)] = v.z, sh[word_of(p + 3)] = v.w;
    }
    for (int p = a + 4 * groups + t; p < cnt; p += kBlock) sh[word_of(p)] = g[p];
    for (int p = cnt + t; p < kTile; p += kBlock) sh[word_of(p)] = 0.0f;
}

// ... and its cnt samples from sh to g
__device__ __forceinline__ void store_tile(const float* sh, float* __restrict__ g, int cnt) {
    const int t = threadIdx.x;
    const int lead = (int)((4 - ((reinterpret_cast<uintptr_t>(g) >> 2) & 3)) & 3), a = lead < cnt ? lead : cnt, groups = (cnt - a) / 4;
    if (t < a) g[t] = sh[word_of(t)];
    for (int j = t; j < groups; j += kBlock) {
        const int p = a + 4 * j;
        *reinterpret_cast<float4*>(g + p) = make_float4(sh[word_of(p)], sh[word_of(p + 1)], sh[word_of(p + 2)], sh[word_of(p + 3)]);
    }
    for (int p = a + 4 * groups + t; p < cnt; p += kBlock) g[p] = sh[word_of(p)];
}

// Steps (1) - (3) of the file comment.  v: in, the state lane 0 starts from (the others' is zero); out, the state at this lane's end.
template <int S>
__device__ __forceinline__ void tile_scan(float* sh, double* P, double* ex, const float* __restrict__ g, int cnt, const Tables& a,
                                          const double (&c)[5 * S], double (&v)[2 * S]) {
    constexpr int N = 2 * S;
    const int t = threadIdx.x;
    stage_tile(sh, g, cnt);
    for (int i = t; i < kSteps * N * N; i += kBlock) P[i] = a.pw[i];
    __syncthreads();
    if (t * kLane < cnt) {   // (a lane behind the row's end: zeros from zero state, e = 0)
        const float* w = sh + t * (kLane + 1);
#pragma unroll 2
        for (int n = 0; n < kLane; ++n) (void)eq_step<S>(c, v, (double)w[n]);
    }
#pragma unroll 1
    for (int k = 0; k < kSteps; ++k) {
        const int d = 1 << k;
#pragma unroll
        for (int j = 0; j < N; ++j) ex[j * kBlock + t] = v[j];
        __syncthreads();
        double u[N];
#pragma unroll
        for (int j = 0; j < N; ++j) u[j] = t >= d ? ex[j * kBlock + t - d] : 0.0;
        __syncthreads();
        if (t >= d) {
            const double* M = P + k * N * N;
#pragma unroll
            for (int i = 0; i < N; ++i) {
                double acc = v[i];
#pragma unroll
                for (int j = 0; j < 2 * (i / 2) + 2; ++j) acc = fma(M[i * N + j], u[j], acc);   // (the block lower triangle: the rest is 0)
                v[i] = acc;
            }
        }
    }
}

template <int S>
__global__ __launch_bounds__(kBlock) void k_eq_tiles(const float* __restrict__ x, const Tables a) {
    extern __shared__ double lds[];
    constexpr int N = 2 * S;
    const RowDev row = a.rows[a.tile_row[blockIdx.x]];
    const int64_t p0 = ((int64_t)blockIdx.x - row.tile0) * kTile;
    if (p0 + kTile >= row.n) return;   // the row's last tile hands nothing on (uniform: no barrier is missed)
    float* sh = reinterpret_cast<float*>(lds);
    double* P = lds + kTileWords / 2;
    double* ex = P + kSteps * N * N;
    double c[5 * S], v[N];
#pragma unroll
    for (int i = 0; i < 5 * S; ++i) c[i] = a.coef[i];
#pragma unroll
    for (int j = 0; j < N; ++j) v[j] = 0.0;
    tile_scan<S>(sh, P, ex, x + row.off + p0, kTile, a, c, v);
    if (threadIdx.x == kBlock - 1) {
#pragma unroll
        for (int j = 0; j < N; ++j) a.tile_e[(int64_t)blockIdx.x * N + j] = v[j];
    }
}

// one wavefront per row: lane r is row r of M_T and element r of the state
__global__ __launch_bounds__(kWave) void k_eq_carry(const Tables a, const int N) {
    const RowDev row = a.rows[blockIdx.x];
    const int r = threadIdx.x, rr = r < N ? r : 0;
    const int64_t nt = (row.n + kTile - 1) / kTile;
    const double* MT = a.pw + (size_t)kSteps * N * N;
    double m[2 * kEqMaxBands];
#pragma unroll
    for (int j = 0; j < 2 * kEqMaxBands; ++j) m[j] = j < N ? MT[rr * N + j] : 0.0;
    double s = 0.0;
    for (int64_t i = 0; i + 1 < nt; ++i) {
        double acc = a.tile_e[(row.tile0 + i) * N + rr];
#pragma unroll
        for (int j = 0; j < 2 * kEqMaxBands; ++j) {
            const double sj = __shfl(s, j, kWave);
            if (j < N) acc = fma(m[j], sj, acc);
        }
        s = acc;
        if (r < N) a.entry[(row.tile0 + i + 1) * N + r] = s;
    }
}

template <int S>
__global__ __launch_bounds__(kBlock) void k_eq_apply(const float* __restrict__ x, float* __restrict__ y, double* __restrict__ y64, const Tables a) {
    extern __shared__ double lds[];
    constexpr int N = 2 * S;
    const int t = threadIdx.x;
    const RowDev row = a.rows[a.tile_row[blockIdx.x]];
    const int64_t p0 = ((int64_t)blockIdx.x - row.tile0) * kTile;
    const int cnt = (int)(row.n - p0 < kTile ? row.n - p0 : kTile);
    float* sh = reinterpret_cast<float*>(lds);
    double* P = lds + kTileWords / 2;
    double* ex = P + kSteps * N * N;
    const double* entry = a.entry + (int64_t)blockIdx.x * N;
    const bool seeded = p0 > 0;   // (a row starts from zero state at its head)
    double c[5 * S], v[N];
#pragma unroll
    for (int i = 0; i < 5 * S; ++i) c[i] = a.coef[i];
#pragma unroll
    for (int j = 0; j < N; ++j) v[j] = (seeded && t == 0) ? entry[j] : 0.0;
    tile_scan<S>(sh, P, ex, x + row.off + p0, cnt, a, c, v);
#pragma unroll
    for (int j = 0; j < N; ++j) ex[j * kBlock + t] = v[j];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < N; ++j) v[j] = t > 0 ? ex[j * kBlock + t - 1] : seeded ? entry[j] : 0.0;
    if (t * kLane < cnt) {
        float* w = sh + t * (kLane + 1);
        const int mine = cnt - t * kLane < kLane ? cnt - t * kLane : kLane;   // this lane's samples of the row
        double* wide = y64 ? y64 + row.off + p0 + t * kLane : nullptr;
#pragma unroll 2
        for (int n = 0; n < kLane; ++n) {
            const double o = eq_step<S>(c, v, (double)w[n]);
            if (wide && n < mine) wide[n] = o;
            w[n] = (float)o;
        }
    }
    __syncthreads();
    store_tile(sh, y + row.off + p0, cnt);
}

template <int S>
void launch_eq(const float* x, float* y, double* y64, const Tables& a, int64_t tiles, int nrows, bool handoff, hipStream_t s) {
    static std::atomic<uint64_t> tiles_allowed{0}, apply_allowed{0};   // per (kernel instantiation, device)
    constexpr size_t lds = eq_lds_bytes(S);
    static_assert(lds <= 160 * 1024, "a workgroup's LDS");
    if (handoff) {   // (no row has a second tile: every tile starts from zero state)
        allow_full_lds(reinterpret_cast<const void*>(k_eq_tiles<S>), tiles_allowed);
        hipLaunchKernelGGL(k_eq_tiles<S>, dim3((unsigned)tiles), dim3(kBlock), lds, s, x, a);
        HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(k_eq_carry, dim3((unsigned)nrows), dim3(kWave), 0, s, a, 2 * S);
        HIP_CHECK(hipGetLastError());
    }
    allow_full_lds(reinterpret_cast<const void*>(k_eq_apply<S>), apply_allowed);
    hipLaunchKernelGGL(k_eq_apply<S>, dim3((unsigned)tiles), dim3(kBlock), lds, s, x, y, y64, a);
    HIP_CHECK(hipGetLastError());
}

inline size_t up64(size_t v) { return (v + 63) & ~(size_t)63; }

}  // namespace

const float* Eq::run(const float* x, int64_t total, const EqRow* rows, int nrows, const EqSpec& sp, hipStream_t s, double* y64) {
    SBV2_REQUIRE(nrows >= 0 && total >= 0 && (x || total == 0) && (nrows == 0 || rows), "internal: bad eq arguments");
    SBV2_REQUIRE(sp.n_bands >= 1 && sp.n_bands <= kEqMaxBands, "internal: an eq of " + std::to_string(sp.n_bands) + " bands has no kernel");
    // every address the kernels form is decided here: the rows inside the buffer
    int64_t tiles = 0;
    bool handoff = false;
    for (int64_t k = 0; k < nrows; ++k) {
        SBV2_REQUIRE(rows[k].n >= 0 && rows[k].off >= 0 && rows[k].off <= total - rows[k].n, "internal: row " + std::to_string(k) + " is outside the buffer");
        tiles += (rows[k].n + kTile - 1) / kTile;
        handoff = handoff || rows[k].n > kTile;
    }
    SBV2_REQUIRE(tiles < (1LL << 31), "internal: too many tiles");
    const int N = 2 * sp.n_bands;
    // rows | tile_row | coef | powers (uploaded) | tile_e | entry
    const size_t o_tile = up64(sizeof(RowDev) * (size_t)nrows), o_coef = o_tile + up64(4 * (size_t)tiles), o_pw = o_coef + up64(8 * 5 * (size_t)sp.n_bands);
    const size_t o_up = o_pw + up64(8 * 9 * (size_t)N * N), o_e = o_up, o_entry = o_e + up64(8 * (size_t)N * (size_t)tiles);
    const size_t bytes = o_entry + up64(8 * (size_t)N * (size_t)tiles) + 64;
    char* h = static_cast<char*>(host_.reserve(o_up, std::max<size_t>(o_up * 2, 4096), s));
    char* d = static_cast<char*>(dev_.reserve(bytes, std::max<size_t>(bytes * 2, 4096), s));
    float* y = static_cast<float*>(out_.reserve(sizeof(float) * (size_t)std::max<int64_t>(total, 4), s));
    RowDev* hrows = reinterpret_cast<RowDev*>(h);
    int32_t* tile_row = reinterpret_cast<int32_t*>(h + o_tile);
    for (int64_t k = 0, tile = 0; k < nrows; ++k) {
        hrows[k] = RowDev{rows[k].off, rows[k].n, tile};
        for (int64_t i = 0; i < (rows[k].n + kTile - 1) / kTile; ++i) tile_row[tile++] = (int32_t)k;
    }
    std::memcpy(h + o_coef, sp.coef, 8 * 5 * (size_t)sp.n_bands);
    eq_powers(sp, reinterpret_cast<double*>(h + o_pw));
    if (!tiles) return y;
    HIP_CHECK(hipMemcpyAsync(d, h, o_up, hipMemcpyHostToDevice, s));
    Tables a;
    a.rows = reinterpret_cast<const RowDev*>(d);
    a.tile_row = reinterpret_cast<const int32_t*>(d + o_tile);
    a.coef = reinterpret_cast<const double*>(d + o_coef);
    a.pw = reinterpret_cast<const double*>(d + o_pw);
    a.tile_e = reinterpret_cast<double*>(d + o_e);
    a.entry = reinterpret_cast<double*>(d + o_entry);
    switch (sp.n_bands) {
        case 1: launch_eq<1>(x, y, y64, a, tiles, nrows, handoff, s); break;
        case 2: launch_eq<2>(x, y, y64, a, tiles, nrows, handoff, s); break;
        case 3: launch_eq<3>(x, y, y64, a, tiles, nrows, handoff, s); break;
        case 4: launch_eq<4>(x, y, y64, a, tiles, nrows, handoff, s); break;
        case 5: launch_eq<5>(x, y, y64, a, tiles, nrows, handoff, s); break;
        case 6: launch_eq<6>(x, y, y64, a, tiles, nrows, handoff, s); break;
        case 7: launch_eq<7>(x, y, y64, a, tiles, nrows, handoff, s); break;
        default: launch_eq<8>(x, y, y64, a, tiles, nrows, handoff, s); break;
    }
    return y;
}

}  // namespace sbv2
