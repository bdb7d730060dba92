// The spectrum of a delivered signal on gfx950: a windowed DFT of every frame as ONE GEMM on the f16 matrix cores, and behind it the Slaney
// mel bank as a sparse sum.  include/sbv2_hip.h states the result above sbv2_spectrum; spectrum.h states the tile rule, and the stage fed
// replay by replay (StreamSpectrum, k_stream_spectrum: the same tile arithmetic over frames x groups of bin blocks, the window read from a
// carry of the last n_fft samples and from the replay).
//
// k_spectrum<T, FT, MEL>: a workgroup of four waves owns FT consecutive frames and writes all their bands; nothing is shared between
// workgroups, so there are no atomics and no second pass.
//   The product.  C [FT frames] x [cos | sin of a block of 32 bins] = A [FT][n_fft] B [n_fft][64] on v_mfma_f32_32x32x16_f16.  Both operands
//   are f16 pairs as in gemm_bfs.hip (hi = f16(x), lo' = f16((x - hi) 2^11): 22 mantissa bits), three MFMAs per product: hi hi into one
//   accumulator, lo' hi + hi lo' into a second one that the epilogue adds with 2^-11.  A wave owns one 32-frame x 32-bin block and its four
//   accumulators (cos / sin x main / cross = 64 registers); with FT = 32 the four waves take four neighbouring bin blocks of the same frames,
//   with FT = 128 four frame blocks of the same bins.  The outer loop runs over bin tiles (32 * WB bins), the inner one over K chunks of 32
//   samples of the window position (n_fft = 16 mod 32, the recogniser's 400: the last chunk is half zeros).  Every (frame, bin) sum is one
//   wave's MFMA chain over ascending K chunks, whatever FT: same bits.
//   Operand B, the basis: cos / sin(2 pi ((i k) mod n_fft) / n_fft) from an f64 table on the host, split and laid out in fragment order
//   [bin block][K chunk][k step 2][cos hi, cos lo', sin hi, sin lo'][64 lanes][8 f16], so a K chunk of a bin block is eight 1 KB pieces that a
//   wave's LDS-DMA (dma16) lands lane-linear; two stages, the DMA of chunk c + 1 issued behind the fragment reads of chunk c and in front of
//   its MFMAs.  Bins above n_fft / 2 in the last block are zeros.
//   Operand A is never in HBM: per K chunk the workgroup loads its frames' RAW samples (FT rows of 32, a row = 128 contiguous bytes of f32;
//   overlapping frames hit L2), positions outside [0, n) and the rows behind the last frame as zeros, into an LDS tile [FT][36] (two stages);
//   forming a fragment, a lane multiplies its eight samples by the window (LDS, whole) and splits them: about six VALU operations per
//   element against 768 MFMA flops per element and bin tile.
//   Epilogue per bin tile: P = re^2 + im^2 in f32 into an LDS tile [FT][32 WB + 1].  MEL = false: stored.  MEL = true: a mel triangle is
//   sparse (a bin feeds at most two bands), so this is no second GEMM: lane t owns the pairs (frame t mod FT, band (t + 256 q) / FT), q <
//   FT / 2, and adds W[m][k] P[k] over the bins of its band that lie in this tile, ascending k, compensated (Kahan), into f32 registers that
//   live across the bin-tile loop (P spans 120 dB: no f16 operand could hold it); the band sums are stored behind the last tile.
// LDS: window 8 KB + A 2 x FT x 144 B + B 2 x WB x 8 KB + P: 97 KB at FT = 32, 76.5 KB at FT = 128 (dynamic).
// Range: the f16 pair has f16's exponent range, and a[i] is split times 2^10.  Delivered samples are in [-1, 1] (every quantiser, and the f32
// sink behind a gain stage); an f32 value with |u w| beyond 63.97 is clamped there by the split (as gemm_bfs clamps), a NaN sample likewise.
#include "spectrum.h"
#include "device_prims.h"

#include <cmath>
#include <cstring>

namespace sbv2 {

namespace {

constexpr int kBlock = 256, kKc = 32, kAPitch = 36, kPiece = 1024, kBlockBytes = 8 * kPiece;   // a K chunk of one bin block: 8 KB
constexpr float kInvLo = 1.0f / kF16LoScale;
// a[i] enters the split times 2^10 (exact) and P leaves times 2^-20 (exact): f16 is subnormal below 6.1e-5, where hi loses bits (and the
// residual of a value below 0.12 lands there once scaled by 2^11), and a window's first samples or a quiet signal (-70 dBFS: 3e-4) are that
// small.  Scaled, the pair keeps its 22 bits for 1.2e-7 <= |a| < 64.
constexpr float kAScale = 1024.0f, kInvAScale2 = 1.0f / (1024.0f * 1024.0f);

struct SpecArgs {
    const void* x;
    int64_t n, hop, n_frames;
    int n_fft, n_bins, nbt, n_mels;   // nbt: 32-bin blocks
    const _Float16* table;
    const float* window;
    const float* W;           // [n_mels][n_bins]
    const int32_t* range;     // [n_mels][2]
    float* power;             // [n_frames][n_bands]
};

struct MulawCode {
    uint8_t c;
};
struct AlawCode {
    uint8_t c;
};
// u[j] of the definition: exact in f32 for the integer encodings
__device__ inline float spec_load(const float* x, int64_t i) { return x[i]; }
__device__ inline float spec_load(const int16_t* x, int64_t i) { return (float)x[i] * (1.0f / 32768.0f); }
__device__ inline float spec_load(const MulawCode* x, int64_t i) { return (float)mulaw_decode(x[i].c) * (1.0f / 32768.0f); }
__device__ inline float spec_load(const AlawCode* x, int64_t i) { return (float)alaw_decode(x[i].c) * (1.0f / 32768.0f); }

template <int FT>
constexpr size_t spec_lds_bytes() {
    return (size_t)kSpectrumMaxFft * 4 + 2 * (size_t)FT * kAPitch * 4 + 2 * (size_t)(128 / FT) * kBlockBytes + (size_t)FT * (32 * (128 / FT) + 1) * 4;
}

// What a workgroup owns of the product: the frames [f0, f0 + FT) below f_end, the 32-bin blocks [bb0, bb1) and, MEL, the bands [m0, m1);
// frame f goes to row f - row0 of out.  k_spectrum owns every block and band of its frames; k_stream_spectrum a group's share.
struct SpecShare {
    int64_t f0, f_end, row0;
    int bb0, bb1, m0, m1;
    float* out;
};

// The tile arithmetic of both kernels (stated at the top of the file): the K-chunk loop with the two-stage A tile and the LDS-DMA basis, the
// hi / lo' split and the six MFMAs, the P epilogue and the Kahan band sums.  at(pos) = u[pos] of the definition, 0 outside the signal.  A bin
// tile is the four blocks bb0 + 4 t ... of the share: whichever tile and wave hold a block, a (frame, bin) sum is one wave's MFMA chain over
// ascending K chunks, and a band's chain runs over ascending k in one lane, so the bits depend on neither the share nor the tile's first frame.
template <int FT, bool MEL, class At>
__device__ __forceinline__ void spectrum_share(const SpecArgs& a, const SpecShare& sh, const At& at) {
    constexpr int WF = FT / 32, WB = 4 / WF, BT = 32 * WB, PP = BT + 1;   // frame blocks, bin blocks per tile, bins per tile, P pitch
    constexpr int NA = FT * kKc / kBlock;                                  // raw samples a lane stages per K chunk
    constexpr int NQ = FT / 2;                                             // (frame, band) pairs a lane can own: FT * 128 / 256
    constexpr int NP = 8 * WB / 4;                                         // 1 KB pieces of the basis a wave requests per K chunk
    extern __shared__ __attribute__((aligned(1024))) char smem[];
    float* const win = reinterpret_cast<float*>(smem);
    float* const As = win + kSpectrumMaxFft;                               // [2][FT][kAPitch]
    char* const Bs = reinterpret_cast<char*>(As + 2 * FT * kAPitch);       // [2][WB][8 pieces][1 KB]
    float* const Pt = reinterpret_cast<float*>(Bs + 2 * WB * kBlockBytes); // [FT][PP]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lrow = lane & 31, lh = lane >> 5;
    const int fb = WF == 1 ? 0 : wave, wb = WB == 1 ? 0 : wave;
    const int64_t f0 = sh.f0;
    const int nkc = (a.n_fft + kKc - 1) / kKc;   // (n_fft = 16 mod 32: the last chunk's second half is zeros in A, in the window and in the basis)
    const int nbands = MEL ? sh.m1 - sh.m0 : 0;

    for (int i = tid; i < nkc * kKc; i += kBlock) win[i] = i < a.n_fft ? a.window[i] : 0.0f;

    // raw samples of K chunk c: element e = tid + 256 j is frame e / 32 of the tile, position e % 32 of the chunk
    const int64_t pos0 = (f0 + (tid >> 5)) * a.hop + a.hop / 2 - a.n_fft / 2 + (tid & 31);
    auto load_a = [&](int c, float (&r)[NA]) {
#pragma unroll
        for (int j = 0; j < NA; ++j) {
            const int64_t f = f0 + (tid >> 5) + 8 * j, s = pos0 + (int64_t)8 * j * a.hop + c * kKc;
            r[j] = (f < sh.f_end && c * kKc + (tid & 31) < a.n_fft) ? at(s) : 0.0f;
        }
    };
    auto store_a = [&](int buf, const float (&r)[NA]) {
#pragma unroll
        for (int j = 0; j < NA; ++j) As[(buf * FT + (tid >> 5) + 8 * j) * kAPitch + (tid & 31)] = r[j];
    };
    // the basis of K chunk c of bin tile bt: piece wave * NP + j of the stage = piece (..) % 8 of bin block bb0 + bt * WB + (..) / 8
    auto dma_b = [&](int bt, int c, int buf) {
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            const int pi = wave * NP + j, bb = sh.bb0 + bt * WB + pi / 8;
            if (bb < sh.bb1)   // (wave-uniform)
                dma16(a.table + (((int64_t)bb * nkc + c) * 8 + pi % 8) * (kPiece / 2) + lane * 8, lds_addr(Bs + (buf * WB * 8 + pi) * kPiece));
        }
    };

    float macc[MEL ? NQ : 1], mcmp[MEL ? NQ : 1];   // a band's sum and its compensation (Kahan: a band may span a thousand bins)
#pragma unroll
    for (int q = 0; q < (MEL ? NQ : 1); ++q) macc[q] = mcmp[q] = 0.0f;

    for (int bt = 0; sh.bb0 + bt * WB < sh.bb1; ++bt) {
        const bool active = sh.bb0 + bt * WB + wb < sh.bb1;   // (wave-uniform: this wave's bin block exists)
        f32x16 acc[4];                                        // cos main, cos cross, sin main, sin cross
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
        {   // (every wave has left the previous tile's K loop: the barrier of its epilogue)
            float r0[NA];
            load_a(0, r0);
            dma_b(bt, 0, 0);
            store_a(0, r0);
            wait_vm<0>();
            __syncthreads();
        }
        for (int c = 0; c < nkc; ++c) {
            const int buf = c & 1;
            f16x8 ah[2], al[2], bf[2][4];
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const int k0 = ks * 16 + 8 * lh;
                const float* ap = As + (buf * FT + fb * 32 + lrow) * kAPitch + k0;
                const float* wp = win + c * kKc + k0;
                const f32x4v u0 = *reinterpret_cast<const f32x4v*>(ap), u1 = *reinterpret_cast<const f32x4v*>(ap + 4);
                const f32x4v w0 = *reinterpret_cast<const f32x4v*>(wp), w1 = *reinterpret_cast<const f32x4v*>(wp + 4);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    // a[i] = u w, one rounding; 2^10 a[i], held within f16's range (a sample beyond 63.9 saturates instead of becoming inf)
                    const float v = fminf(fmaxf(((e < 4 ? u0[e & 3] : u1[e & 3]) * (e < 4 ? w0[e & 3] : w1[e & 3])) * kAScale, -65504.0f), 65504.0f);
                    const _Float16 h = (_Float16)v;
                    ah[ks][e] = h;
                    al[ks][e] = (_Float16)((v - (float)h) * kF16LoScale);
                }
                if (active) {
#pragma unroll
                    for (int pt = 0; pt < 4; ++pt)
                        bf[ks][pt] = *reinterpret_cast<const f16x8*>(Bs + ((buf * WB + wb) * 8 + ks * 4 + pt) * kPiece + lane * 16);
                }
            }
            __builtin_amdgcn_sched_barrier(0);   // the fragment reads stay in front of the requests for the next chunk
            float rn[NA];
            if (c + 1 < nkc) {
                load_a(c + 1, rn);
                dma_b(bt, c + 1, buf ^ 1);
            }
            if (active) {
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    acc[0] = mfma32(ah[ks], bf[ks][0], acc[0]);
                    acc[1] = mfma32(al[ks], bf[ks][0], acc[1]);
                    acc[1] = mfma32(ah[ks], bf[ks][1], acc[1]);
                    acc[2] = mfma32(ah[ks], bf[ks][2], acc[2]);
                    acc[3] = mfma32(al[ks], bf[ks][2], acc[3]);
                    acc[3] = mfma32(ah[ks], bf[ks][3], acc[3]);
                }
            }
            if (c + 1 < nkc) store_a(buf ^ 1, rn);
            wait_vm<0>();
            __syncthreads();
        }

        // ---- epilogue of the bin tile: P into LDS, then stored or summed into the bands
        if (active) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float re = acc[0][r] + acc[1][r] * kInvLo, im = acc[2][r] + acc[3][r] * kInvLo;
                Pt[(fb * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh) * PP + wb * 32 + lrow] = (re * re + im * im) * kInvAScale2;
            }
        }
        __syncthreads();
        const int bin0 = (sh.bb0 + bt * WB) * 32;
        if constexpr (!MEL) {
            const int bins_end = min(a.n_bins, sh.bb1 * 32);   // (the blocks of the tile behind the share hold nothing)
            for (int idx = tid; idx < FT * BT; idx += kBlock) {
                const int fl = idx / BT, bl = idx % BT;
                if (f0 + fl < sh.f_end && bin0 + bl < bins_end) sh.out[(f0 + fl - sh.row0) * a.n_bins + bin0 + bl] = Pt[fl * PP + bl];
            }
        } else {
            const int fl = tid % FT;
            static_for<0, NQ>([&](auto qc) {
                constexpr int q = decltype(qc)::value;
                if (q * kBlock < FT * nbands) {   // (uniform)
                    // (opaque: the band's range and row stay loads of this tile; traced, they were hoisted into 4 registers per pair)
                    const int m = sh.m0 + (int)opaque((unsigned)(tid + kBlock * q)) / FT;
                    if (m < sh.m1) {
                        // (a band's bins lie within the share's blocks: the host's group table, spectrum_groups)
                        const int lo = max(a.range[2 * m], bin0), hi = min(a.range[2 * m + 1], bin0 + BT);
                        const float* w = a.W + (int64_t)m * a.n_bins;
                        float s = macc[q], cmp = mcmp[q];
                        for (int k = lo; k < hi; ++k) {
                            const float y = w[k] * Pt[fl * PP + k - bin0] - cmp, t = s + y;
                            cmp = (t - s) - y;
                            s = t;
                        }
                        macc[q] = s;
                        mcmp[q] = cmp;
                    }
                }
            });
        }
        // (the next tile's P is written behind its K loop's barriers: every lane has read this one by then)
    }
    if constexpr (MEL) {
        const int fl = tid % FT;
        static_for<0, NQ>([&](auto qc) {
            constexpr int q = decltype(qc)::value;
            const int m = sh.m0 + (tid + kBlock * q) / FT;
            if (m < sh.m1 && f0 + fl < sh.f_end) sh.out[(f0 + fl - sh.row0) * a.n_mels + m] = macc[q];
        });
    }
}

template <class T, int FT, bool MEL>
__global__ __launch_bounds__(kBlock) void k_spectrum(const SpecArgs a) {
    const T* x = static_cast<const T*>(a.x);
    const int64_t n = a.n;
    const SpecShare sh{(int64_t)blockIdx.x * FT, a.n_frames, 0, 0, a.nbt, 0, a.n_mels, a.power};
    spectrum_share<FT, MEL>(a, sh, [x, n](int64_t s) -> float { return s >= 0 && s < n ? spec_load(x, s) : 0.0f; });
}

// The fed stage (StreamSpectrum, spectrum.h), one launch per push.  Workgroup (t, g), t < tiles: the frames first + 32 t ... of the push's
// count completed frames, group g's share of their blocks and bands (the table comes by value), into the push's result rows.  A frame's
// sample at pos comes from the carry when pos < d0 (the cl samples before d0, in the sample's own type), from x when d0 <= pos < d1, and
// is 0 outside [0, total): nothing outside carry_in[0, cl) and x[0, d1 - d0) is addressed, whatever the arguments.  The workgroups (t >=
// tiles, 0) write the next carry, the last cl_out fed samples, into the OTHER copy: no workgroup reads what one of the same launch writes.
struct SpecGroup {
    int32_t m0, m1, bb0, bb1;
};
struct SpecGroups {
    SpecGroup g[kSpectrumMaxGroups];
};
struct StreamSpecArgs {
    SpecArgs a;             // x = the sample at d0; n, n_frames, power unused
    const void* carry_in;   // positions [d0 - cl, d0)
    void* carry_out;        // positions [d1 - cl_out, d1)
    int64_t d0, d1, total, first;
    int32_t count, tiles, cl, cl_out;
    float* out;             // [count][n_bands]
    SpecGroups groups;
};

template <class T, bool MEL>
__global__ __launch_bounds__(kBlock) void k_stream_spectrum(const StreamSpecArgs p) {
    const T* x = static_cast<const T*>(p.a.x);
    const T* cin = static_cast<const T*>(p.carry_in);
    const int64_t d0 = p.d0, d1 = p.d1, c0 = p.d0 - p.cl, total = p.total;
    if ((int)blockIdx.x >= p.tiles) {   // the carry: a push shorter than it keeps the end of the old one in front of x (uniform: no barrier here)
        if (blockIdx.y) return;
        T* cout = static_cast<T*>(p.carry_out);
        const int j = ((int)blockIdx.x - p.tiles) * kBlock + (int)threadIdx.x;
        if (j >= p.cl_out) return;
        const int64_t i = d1 - p.cl_out + j;
        if (i >= d0) cout[j] = x[i - d0];
        else if (i >= c0) cout[j] = cin[i - c0];
        return;
    }
    const SpecGroup g = p.groups.g[blockIdx.y];
    const SpecShare sh{p.first + (int64_t)blockIdx.x * 32, p.first + p.count, p.first, g.bb0, g.bb1, g.m0, g.m1, p.out};
    spectrum_share<32, MEL>(p.a, sh, [x, cin, d0, d1, c0, total](int64_t s) -> float {
        if (s < 0 || s >= total) return 0.0f;
        if (s >= d0) return s < d1 ? spec_load(x, s - d0) : 0.0f;
        return s >= c0 ? spec_load(cin, s - c0) : 0.0f;
    });
}

template <class T, int FT, bool MEL>
void launch_one(const SpecArgs& a, hipStream_t s) {
    auto kern = k_spectrum<T, FT, MEL>;
    static std::atomic<uint64_t> lds_allowed{0};
    allow_full_lds(reinterpret_cast<const void*>(kern), lds_allowed);
    const int64_t grid = (a.n_frames + FT - 1) / FT;
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(kBlock), spec_lds_bytes<FT>(), s, a);
    HIP_CHECK(hipGetLastError());
}
template <class T>
void launch_enc(const SpecArgs& a, hipStream_t s) {
    const bool wide = spectrum_tile(a.n_frames) == 128;
    if (a.n_mels) wide ? launch_one<T, 128, true>(a, s) : launch_one<T, 32, true>(a, s);
    else wide ? launch_one<T, 128, false>(a, s) : launch_one<T, 32, false>(a, s);
}

template <class T, bool MEL>
void launch_stream_one(const StreamSpecArgs& p, dim3 grid, hipStream_t s) {
    auto kern = k_stream_spectrum<T, MEL>;
    static std::atomic<uint64_t> lds_allowed{0};
    allow_full_lds(reinterpret_cast<const void*>(kern), lds_allowed);
    hipLaunchKernelGGL(kern, grid, dim3(kBlock), spec_lds_bytes<32>(), s, p);
    HIP_CHECK(hipGetLastError());
}
template <class T>
void launch_stream_enc(const StreamSpecArgs& p, dim3 grid, hipStream_t s) {
    p.a.n_mels ? launch_stream_one<T, true>(p, grid, s) : launch_stream_one<T, false>(p, grid, s);
}

// ---- the host's tables -------------------------------------------------------------------------------------------------------------------
constexpr double kPi = 3.14159265358979323846;

// Slaney's mel scale: linear below 1000 Hz at 200 / 3 Hz per mel, logarithmic above with step log(6.4) / 27
double hz_to_mel(double f) { return f >= 1000.0 ? 15.0 + std::log(f / 1000.0) / (std::log(6.4) / 27.0) : f / (200.0 / 3.0); }
double mel_to_hz(double m) { return m >= 15.0 ? 1000.0 * std::exp((std::log(6.4) / 27.0) * (m - 15.0)) : (200.0 / 3.0) * m; }

int spec_blocks(int n_fft) { return (n_fft / 2 + 1 + 31) / 32; }
int spec_chunks(int n_fft) { return (n_fft + kKc - 1) / kKc; }
size_t spec_table_bytes(int n_fft) { return (size_t)spec_blocks(n_fft) * spec_chunks(n_fft) * kBlockBytes; }

// the basis in fragment order: lane l of a piece holds column (bin) 32 bb + (l & 31), k = 32 c + 16 ks + 8 (l >> 5) + j
void build_basis(int n_fft, _Float16* t) {
    std::vector<double> cs((size_t)n_fft), sn((size_t)n_fft);
    for (int r = 0; r < n_fft; ++r) {   // the argument is reduced in integers first
        cs[r] = std::cos(2.0 * kPi * (double)r / (double)n_fft);
        sn[r] = std::sin(2.0 * kPi * (double)r / (double)n_fft);
    }
    const int nbt = spec_blocks(n_fft), nkc = spec_chunks(n_fft);
    for (int bb = 0; bb < nbt; ++bb)
        for (int c = 0; c < nkc; ++c)
            for (int ks = 0; ks < 2; ++ks)
                for (int l = 0; l < 64; ++l)
                    for (int j = 0; j < 8; ++j) {
                        const int k = 32 * bb + (l & 31), i = kKc * c + 16 * ks + 8 * (l >> 5) + j;
                        const int r = (int)(((int64_t)(i % n_fft) * k) % n_fft);
                        _Float16* p = t + ((((size_t)bb * nkc + c) * 2 + ks) * 4 * 64 + l) * 8 + j;
                        for (int tr = 0; tr < 2; ++tr) {
                            const float v = k <= n_fft / 2 && i < n_fft ? (float)(tr ? sn[r] : cs[r]) : 0.0f;
                            const _Float16 h = (_Float16)v;
                            p[(size_t)(2 * tr) * 512] = h;
                            p[(size_t)(2 * tr + 1) * 512] = (_Float16)((v - (float)h) * kF16LoScale);
                        }
                    }
}

// The basis and the window of an n_fft, formed on the host in f64 and uploaded from pinned staging on s, which is synchronised (the staging is reused).
void upload_basis(int n_fft, DeviceBuffer* table, DeviceBuffer* window, PinnedBuffer* stage, hipStream_t s) {
    const size_t tb = spec_table_bytes(n_fft), wbytes = sizeof(float) * (size_t)n_fft;
    char* st = static_cast<char*>(stage->reserve(tb + wbytes, s));
    build_basis(n_fft, reinterpret_cast<_Float16*>(st));
    std::vector<float> w;
    spectrum_window(n_fft, &w);
    std::memcpy(st + tb, w.data(), wbytes);
    HIP_CHECK(hipMemcpyAsync(table->reserve(tb, s), st, tb, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(window->reserve(wbytes, s), st + tb, wbytes, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipStreamSynchronize(s));
}

// ... and the mel bank of a spec, W [n_mels][n_bins] f32 | range [n_mels][2] i32; range_host (may be null) receives the ranges.
void upload_bank(const SpectrumSpec& sp, DeviceBuffer* bank, PinnedBuffer* stage, hipStream_t s, std::vector<int32_t>* range_host = nullptr) {
    std::vector<float> W;
    std::vector<int32_t> range;
    spectrum_mel_bank(sp, &W, &range);
    const size_t wcount = (size_t)sp.n_mels * sp.n_bins(), bytes = 4 * wcount + 8 * (size_t)sp.n_mels;
    char* st = static_cast<char*>(stage->reserve(bytes, s));
    std::memcpy(st, W.data(), 4 * wcount);
    std::memcpy(st + 4 * wcount, range.data(), 8 * (size_t)sp.n_mels);
    HIP_CHECK(hipMemcpyAsync(bank->reserve(bytes, s), st, bytes, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipStreamSynchronize(s));
    if (range_host) *range_host = std::move(range);
}

// The group table of a spec at G groups (spectrum.h, above spectrum_stream_groups).  range == nullptr: bins, the nbt blocks cut into G
// contiguous runs.  Otherwise the bands go to groups by the block their triangle starts in, relative to the blocks [B0, B1) that the bank
// spans at all, so that the groups hold about as many blocks each (low bands are narrow: equal band counts would not); a band without a
// bin stays with its predecessor.  A group computes the blocks from its first band's first bin to its last band's last one; a group left
// without bands, or with empty triangles only, computes none and stores zeros for what it owns.
SpecGroups spectrum_groups(int nbt, int n_mels, const int32_t* range, int G) {
    SpecGroups t{};
    if (!range) {
        for (int g = 0; g < G; ++g) t.g[g] = SpecGroup{0, 0, nbt * g / G, nbt * (g + 1) / G};
        return t;
    }
    int B0 = nbt, B1 = 0;
    for (int m = 0; m < n_mels; ++m)
        if (range[2 * m] < range[2 * m + 1]) B0 = std::min(B0, range[2 * m] / 32), B1 = std::max(B1, (range[2 * m + 1] + 31) / 32);
    int m = 0, gid = 0;
    for (int g = 0; g < G; ++g) {
        SpecGroup& q = t.g[g];
        q.m0 = m;
        int lo = nbt, hi = 0;
        for (; m < n_mels; ++m) {
            const bool holds = range[2 * m] < range[2 * m + 1];
            if (holds) gid = std::max(gid, std::min(G - 1, (range[2 * m] / 32 - B0) * G / std::max(1, B1 - B0)));
            if (gid > g) break;
            if (holds) lo = std::min(lo, range[2 * m] / 32), hi = std::max(hi, (range[2 * m + 1] + 31) / 32);
        }
        q.m1 = g + 1 == G ? n_mels : m;
        q.bb0 = hi > lo ? lo : 0;
        q.bb1 = hi > lo ? hi : 0;
    }
    SBV2_REQUIRE(m == n_mels, "internal: mel bands left without a group");
    return t;
}

}  // namespace

SpectrumSpec spectrum_spec(int sample_rate, int n_fft, int64_t hop, int n_mels, double f_min, double f_max) {
    SBV2_REQUIRE(sample_rate > 0 && sample_rate <= kSpectrumMaxRate,
                 "spectrum: sample rate must be in [1, " + std::to_string(kSpectrumMaxRate) + "]: " + std::to_string(sample_rate));
    SBV2_REQUIRE(n_fft >= kSpectrumMinFft && n_fft <= kSpectrumMaxFft && n_fft % 16 == 0,
                 "spectrum: n_fft must be a multiple of 16 in [64, 2048]: " + std::to_string(n_fft));
    SBV2_REQUIRE(hop >= 1 && hop <= n_fft, "spectrum: hop must be in [1, n_fft]: " + std::to_string(hop));
    SBV2_REQUIRE(n_mels >= 0 && n_mels <= kSpectrumMaxMels, "spectrum: n_mels must be in [0, 128]: " + std::to_string(n_mels));
    SBV2_REQUIRE(f_min >= 0.0, "spectrum: f_min must be >= 0: " + std::to_string(f_min));
    SBV2_REQUIRE(f_min < f_max, "spectrum: f_min must be below f_max: " + std::to_string(f_min) + " >= " + std::to_string(f_max));
    SBV2_REQUIRE(f_max <= sample_rate / 2.0,
                 "spectrum: f_max must be <= sample_rate / 2 = " + std::to_string(sample_rate / 2.0) + ": " + std::to_string(f_max));
    SpectrumSpec sp;
    sp.sample_rate = sample_rate;
    sp.n_fft = n_fft;
    sp.hop = hop;
    sp.n_mels = n_mels;
    sp.f_min = f_min;
    sp.f_max = f_max;
    return sp;
}

void spectrum_window(int n_fft, std::vector<float>* w) {
    w->resize((size_t)n_fft);
    for (int i = 0; i < n_fft; ++i) (*w)[i] = (float)(0.5 - 0.5 * std::cos(2.0 * kPi * (double)i / (double)n_fft));
}

void spectrum_mel_bank(const SpectrumSpec& sp, std::vector<float>* W, std::vector<int32_t>* range) {
    const int nm = sp.n_mels, nb = sp.n_bins();
    SBV2_REQUIRE(nm > 0, "internal: a mel bank of no bands");
    std::vector<double> edge((size_t)nm + 2);
    const double m0 = hz_to_mel(sp.f_min), m1 = hz_to_mel(sp.f_max);
    for (int i = 0; i < nm + 2; ++i) edge[i] = mel_to_hz(m0 + (m1 - m0) * (double)i / (double)(nm + 1));
    W->assign((size_t)nm * nb, 0.0f);
    if (range) range->assign((size_t)2 * nm, 0);
    for (int m = 0; m < nm; ++m) {
        const double norm = 2.0 / (edge[m + 2] - edge[m]);
        int lo = 0, hi = 0;
        for (int k = 0; k < nb; ++k) {
            const double f = (double)k * (double)sp.sample_rate / (double)sp.n_fft;
            const double up = (f - edge[m]) / (edge[m + 1] - edge[m]), down = (edge[m + 2] - f) / (edge[m + 2] - edge[m + 1]);
            const float w = (float)(std::max(0.0, std::min(up, down)) * norm);
            (*W)[(size_t)m * nb + k] = w;
            if (w != 0.0f) {
                if (hi == 0) lo = k;
                hi = k + 1;
            }
        }
        if (range) (*range)[2 * m] = lo, (*range)[2 * m + 1] = hi;
    }
}

void Spectrum::run(const void* x, int encoding, int64_t n, const SpectrumSpec& sp, hipStream_t s) {
    SBV2_REQUIRE(pcm_encoding_known(encoding), "internal: spectrum of an unknown encoding");
    SBV2_REQUIRE(n >= 0 && sp.hop >= 1 && sp.hop <= sp.n_fft && sp.n_fft >= kSpectrumMinFft && sp.n_fft <= kSpectrumMaxFft && sp.n_fft % 16 == 0 &&
                     sp.n_mels >= 0 && sp.n_mels <= kSpectrumMaxMels,
                 "internal: bad spectrum spec");
    const int64_t nf = spectrum_frames(n, sp.hop);
    SBV2_REQUIRE(nf < (1 << 30), "too many spectrum frames: " + std::to_string(nf) + " >= 2^30");
    nf_ = nf;
    if (nf == 0) return;
    SBV2_REQUIRE(x, "internal: no samples");
    const int nb = sp.n_bins(), nbands = sp.n_bands();

    if (!basis_.count(sp.n_fft) && basis_.size() >= kMaxBases) {   // (nothing enqueued reads what is dropped)
        HIP_CHECK(hipStreamSynchronize(s));
        basis_.clear();
    }
    Basis& bs = basis_[sp.n_fft];
    if (!bs.table.get()) upload_basis(sp.n_fft, &bs.table, &bs.window, &stage_, s);   // once per n_fft and context
    const size_t wcount = (size_t)sp.n_mels * nb;
    const BankKey key{sp.n_fft, sp.n_mels, sp.sample_rate, sp.f_min, sp.f_max};
    if (sp.n_mels && !banks_.count(key) && banks_.size() >= kMaxBanks) {
        HIP_CHECK(hipStreamSynchronize(s));
        banks_.clear();
    }
    DeviceBuffer* const bank = sp.n_mels ? &banks_[key] : nullptr;
    if (bank && !bank->get()) upload_bank(sp, bank, &stage_, s);   // once per bank and context

    const size_t bytes = sizeof(float) * (size_t)nf * nbands;
    float* h = static_cast<float*>(host_.reserve(bytes, std::max<size_t>(bytes * 2, 4096), s));
    float* d = static_cast<float*>(dev_.reserve(bytes, std::max<size_t>(bytes * 2, 4096), s));
    SpecArgs a;
    a.x = x;
    a.n = n;
    a.hop = sp.hop;
    a.n_frames = nf;
    a.n_fft = sp.n_fft;
    a.n_bins = nb;
    a.nbt = spec_blocks(sp.n_fft);
    a.n_mels = sp.n_mels;
    a.table = bs.table.as<_Float16>();
    a.window = bs.window.as<float>();
    a.W = bank ? bank->as<float>() : nullptr;
    a.range = bank ? reinterpret_cast<const int32_t*>(bank->as<char>() + 4 * wcount) : nullptr;
    a.power = d;
    if (encoding == kEncS16) launch_enc<int16_t>(a, s);
    else if (encoding == kEncMulaw) launch_enc<MulawCode>(a, s);
    else if (encoding == kEncAlaw) launch_enc<AlawCode>(a, s);
    else launch_enc<float>(a, s);
    HIP_CHECK(hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, s));
}

// ---- the fed stage (StreamSpectrum, spectrum.h) ----
void StreamSpectrum::check(const SpectrumSpec& sp, int64_t total) {
    SBV2_REQUIRE(total >= 0 && sp.hop >= 1 && sp.hop <= sp.n_fft && sp.n_fft >= kSpectrumMinFft && sp.n_fft <= kSpectrumMaxFft && sp.n_fft % 16 == 0 &&
                     sp.n_mels >= 0 && sp.n_mels <= kSpectrumMaxMels,
                 "internal: bad spectrum spec");
    const int64_t nf = spectrum_frames(total, sp.hop);
    SBV2_REQUIRE(nf < (1 << 30), "too many spectrum frames: " + std::to_string(nf) + " >= 2^30");
}

int64_t spectrum_frames_complete(const SpectrumSpec& sp, int64_t total, int64_t D) {
    const int64_t nf = spectrum_frames(total, sp.hop);
    if (nf == 0 || D >= total) return nf;
    const int64_t r = D - sp.n_fft / 2 - sp.hop / 2;   // frame f: f hop + hop / 2 + n_fft / 2 <= D
    return r < 0 ? 0 : std::min(nf, r / sp.hop + 1);
}

int64_t StreamSpectrum::complete(int64_t D) const { return spectrum_frames_complete(sp_, total_, D); }

void StreamSpectrum::begin(const SpectrumSpec& sp, int encoding, int64_t total, int64_t most, hipStream_t s, int groups) {
    SBV2_REQUIRE(pcm_encoding_known(encoding), "internal: spectrum of an unknown encoding");
    SBV2_REQUIRE(most >= 0 && groups >= 0, "internal: bad spectrum stream");
    check(sp, total);
    sp_ = sp;
    encoding_ = encoding;
    total_ = total;
    nf_ = spectrum_frames(total, sp.hop);
    fed_ = done_ = 0;
    parity_ = 0;
    forced_ = groups;
    // the tables of this spec, kept from the previous stream of this context when they are the same
    if (basis_fft_ != sp.n_fft) {
        upload_basis(sp.n_fft, &table_, &window_, &stage_, s);
        basis_fft_ = sp.n_fft;
    }
    const BankKey key{sp.n_fft, sp.n_mels, sp.sample_rate, sp.f_min, sp.f_max};
    if (sp.n_mels && (!bank_.get() || key != bank_key_)) {
        upload_bank(sp, &bank_, &stage_, s, &range_);
        bank_key_ = key;
    }
    // the group tables at every G the rule can give: the blocks that count are the bank's own with mel bands
    const int nbt = spec_blocks(sp.n_fft);
    const int32_t* range = sp.n_mels ? range_.data() : nullptr;
    blocks_ = nbt;
    if (range) {
        const SpecGroup all = spectrum_groups(nbt, sp.n_mels, range, 1).g[0];
        blocks_ = all.bb1 - all.bb0;
    }
    static_assert(sizeof(groups_[0]) == sizeof(SpecGroups), "the group table by value");
    for (int G = 1; G <= spectrum_stream_groups_max(blocks_); ++G) {
        const SpecGroups t = spectrum_groups(nbt, sp.n_mels, range, G);
        std::memcpy(&groups_[G - 1], &t, sizeof t);
    }
    // device: the carry (two copies, each kSpectrumMaxFft elements of the widest sample type), the results of one push; pinned: every frame
    const size_t row = sizeof(float) * (size_t)sp.n_bands(), h_bytes = row * (size_t)nf_;
    const size_t push_bytes = row * (size_t)std::min(nf_, (most + sp.n_fft) / sp.hop + 2);
    carry_.reserve(2 * kCarryBytes, s);
    out_.reserve(std::max<size_t>(push_bytes, 4096), s);
    host_.reserve(std::max<size_t>(h_bytes, 64), std::max<size_t>(h_bytes, 4096), s);
    HIP_CHECK(hipStreamSynchronize(s));   // (an earlier stream's copies into the mirror are done)
}

int64_t StreamSpectrum::push(const void* x, int64_t D0, int64_t n, hipStream_t s) {
    SBV2_REQUIRE(n >= 0 && D0 == fed_ && D0 + n <= total_, "internal: a spectrum push of [" + std::to_string(D0) + ", " + std::to_string(D0 + n) +
                                                               ") out of stream order (" + std::to_string(fed_) + " of " + std::to_string(total_) + " fed)");
    const int64_t D1 = D0 + n, now = complete(D1), done = now - done_;
    fed_ = D1;
    if (n > 0) {
        SBV2_REQUIRE(x, "internal: no samples to push");
        const size_t row = sizeof(float) * (size_t)sp_.n_bands();
        float* out = static_cast<float*>(out_.reserve(std::max<size_t>(row * (size_t)done, 4096), s));   // (sized at begin for a push of up to `most`)
        const int gmax = spectrum_stream_groups_max(blocks_);
        const int G = done == 0 ? 1 : forced_ ? std::min(forced_, gmax) : spectrum_stream_groups(done, blocks_, device_cu_count());
        const size_t wcount = (size_t)sp_.n_mels * sp_.n_bins();
        StreamSpecArgs p{};
        p.a.x = x;
        p.a.hop = sp_.hop;
        p.a.n_fft = sp_.n_fft;
        p.a.n_bins = sp_.n_bins();
        p.a.nbt = spec_blocks(sp_.n_fft);
        p.a.n_mels = sp_.n_mels;
        p.a.table = table_.as<_Float16>();
        p.a.window = window_.as<float>();
        p.a.W = sp_.n_mels ? bank_.as<float>() : nullptr;
        p.a.range = sp_.n_mels ? reinterpret_cast<const int32_t*>(bank_.as<char>() + 4 * wcount) : nullptr;
        p.carry_in = carry_.as<char>() + (size_t)parity_ * kCarryBytes;
        p.carry_out = carry_.as<char>() + (size_t)(parity_ ^ 1) * kCarryBytes;
        p.d0 = D0;
        p.d1 = D1;
        p.total = total_;
        p.first = done_;
        p.count = (int32_t)done;
        p.tiles = (int32_t)((done + 31) / 32);
        p.cl = (int32_t)std::min<int64_t>(D0, sp_.n_fft);
        p.cl_out = (int32_t)std::min<int64_t>(D1, sp_.n_fft);
        p.out = out;
        std::memcpy(&p.groups, &groups_[G - 1], sizeof p.groups);
        const dim3 grid((unsigned)(p.tiles + (p.cl_out + kBlock - 1) / kBlock), (unsigned)G);
        if (encoding_ == kEncS16) launch_stream_enc<int16_t>(p, grid, s);
        else if (encoding_ == kEncMulaw) launch_stream_enc<MulawCode>(p, grid, s);
        else if (encoding_ == kEncAlaw) launch_stream_enc<AlawCode>(p, grid, s);
        else launch_stream_enc<float>(p, grid, s);
        parity_ ^= 1;
        if (done) HIP_CHECK(hipMemcpyAsync(host_.as<char>() + row * (size_t)done_, out, row * (size_t)done, hipMemcpyDeviceToHost, s));
    }
    done_ = now;
    return done;
}

}  // namespace sbv2
