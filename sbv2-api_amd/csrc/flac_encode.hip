// FLAC encoder on the device: mono, 16-bit, fixed 4096-sample blocks, one stream per signal (RFC 9639, streamable subset).
//
// Three launches per fetch, whatever the number of signals:
//   k_flac_analyse  one workgroup per frame (all frames of all signals): stage the block in LDS; CONSTANT when every sample is equal; else a
//                   Tukey(0.5)-windowed autocorrelation (lags 0..12, f64, fixed summation order), Levinson-Durbin (f64) and libFLAC's
//                   precision-15 quantiser give LPC orders 1..12; every predictor (FIXED 0..4 = LPC with fixed integer coefficients and
//                   shift 0, then LPC 1..12) is costed exactly for every valid Rice partition order p <= 8: each lane owns one finest
//                   partition (16 samples of a full block), sums u >> k for k = 0..14, and the sums are added up the partition tree (wave
//                   shuffles, then LDS).  The cheapest candidate (ties: CONSTANT, FIXED by order, LPC by order, VERBATIM; lower p first) goes
//                   into the frame's descriptor with its Rice parameters and the frame's byte size.
//   k_flac_scan     one workgroup: exclusive scan of the frame sizes (every frame's offset in the compacted output, signals back to back, 42
//                   header bytes before each signal's first frame), each signal's size and its min / max frame size (integer atomics).
//   k_flac_pack     one workgroup per frame: recompute the chosen residuals, scan their code lengths in LDS, OR each code's terminating one
//                   bit and low bits into a zeroed LDS bit buffer (the unary zeros need no write), header + CRC-8, CRC-16 as per-lane CRCs of
//                   byte spans combined over GF(2), store; the workgroups past the last frame write the STREAMINFO blocks.
// Every f64 reduction has a fixed order and every other reduction is over integers, so the bytes are a pure function of the samples.
#include <climits>
#include <cmath>
#include <cstring>

#include "flac_encode.h"

namespace sbv2 {

namespace {

constexpr int kT = 256;          // lanes per workgroup of the frame kernels: a lane per finest (p = 8) partition of a full block
constexpr int kMaxLpc = 12;
constexpr int kMaxRice = 14;     // 4-bit Rice parameters, 15 = escape (unused)
constexpr int kBitWords = 2056;  // LDS bit buffer: >= (kFlacMaxFrameHeader + 1 + 2 * kFlacBlock + 2) bytes
enum { kConstant = 0, kVerbatim = 1, kFixed = 2, kLpc = 3 };

struct FlacSig {
    int64_t x_off, n, f0;   // samples at x[x_off, x_off + n); frames [f0, f0 + ceil(n / 4096)) of the launch
    int64_t fno0;           // frame number of the signal's first frame (0 for a whole stream; a push of a fed stream continues its count)
    int64_t hoff;           // stream-header bytes in the output before the signal's first frame, its own included
    int64_t hdr;            // 1: the signal starts a stream (42-byte header, written by k_flac_pack), 0: frames only
};

struct FlacDesc {
    int64_t x;   // first sample of the frame in x
    int32_t sig, n, fno, method, order, shift, p, hdr, bytes, pad;
    int32_t coef[kMaxLpc];
    uint8_t k[kT];
};

__device__ __forceinline__ int find_sig(const FlacSig* sg, int nsig, int64_t f) {
    int lo = 0, hi = nsig - 1;   // last signal with f0 <= f (a signal without frames shares its f0 with the next one)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (sg[mid].f0 <= f) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__host__ __device__ __forceinline__ int utf8_len(uint32_t v) {
    return v < 0x80 ? 1 : v < 0x800 ? 2 : v < 0x10000 ? 3 : v < 0x200000 ? 4 : v < 0x4000000 ? 5 : 6;
}

__device__ __forceinline__ int header_bytes(int n, int fno) { return 4 + utf8_len((uint32_t)fno) + (n == kFlacBlock ? 0 : n <= 256 ? 1 : 2) + 1; }

// the fixed predictors as integer LPC with shift 0: coefficient j multiplies x[i - 1 - j]
__device__ __forceinline__ int fixed_coef(int order, int j) {
    constexpr int c[5][4] = {{0, 0, 0, 0}, {1, 0, 0, 0}, {2, -1, 0, 0}, {3, -3, 1, 0}, {4, -6, 4, -1}};
    return c[order][j];
}

// bits of a subframe before its residual codes: zero bit + type + wasted flag, warm-up, LPC precision / shift / coefficients, the residual's
// method and partition order, and partition 0's Rice parameter (the other partitions' parameters are counted with their partitions)
__device__ __forceinline__ int preamble_bits(int method, int order) {
    return 8 + 16 * order + (method == kLpc ? 4 + 5 + 15 * order : 0) + 2 + 4 + 4;
}

// ---- analyse ----

__global__ __launch_bounds__(kT) void k_flac_analyse(const short* __restrict__ x, const FlacSig* __restrict__ sg, int nsig, FlacDesc* __restrict__ dd) {
    __shared__ int xs[kFlacBlock];
    __shared__ double xw[kFlacBlock];
    __shared__ double red[kT / 64][kMaxLpc + 1];
    __shared__ double lpc[kMaxLpc][kMaxLpc];
    __shared__ int qc[kMaxLpc][kMaxLpc], qsh[kMaxLpc], nlpc;
    __shared__ unsigned long long wsum[kT / 64][kMaxRice + 1];
    __shared__ unsigned long long tot[9];
    __shared__ uint8_t kc[511], ksel[kT];
    __shared__ int upd_p, best_method_s, best_p_s;
    __shared__ int best_coef[kMaxLpc];

    const int f = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int s = find_sig(sg, nsig, f);
    const int fi = f - (int)sg[s].f0;   // frame of the signal; its number in the stream:
    const int fno = (int)sg[s].fno0 + fi;
    const int64_t x0 = sg[s].x_off + (int64_t)fi * kFlacBlock;
    const int n = (int)min((int64_t)kFlacBlock, sg[s].n - (int64_t)fi * kFlacBlock);
    const int hdr = header_bytes(n, fno);
    FlacDesc& d = dd[f];

    bool same = true;
    for (int i = t; i < n; i += kT) {
        xs[i] = x[x0 + i];
    }
    if (t < 9) tot[t] = 0;
    __syncthreads();
    for (int i = t; i < n; i += kT) same &= xs[i] == xs[0];
    const bool constant = __syncthreads_and(same);
    // a constant block of >= 7 samples: CONSTANT (24 bits) beats every other candidate (>= 18 + n bits); shorter ones are costed below
    int best_method = -1, best_order = 0, best_shift = 0, best_p = 0;
    long long best_bits = LLONG_MAX;
    if (constant) {
        best_method = kConstant;
        best_bits = 24;
    }
    if (!(constant && n >= 7)) {
        // windowed autocorrelation, lags 0..12: each lane sums its 16 contiguous samples in order, then a fixed butterfly and a fixed LDS order
        const int width = (n - 1) / 4;   // scipy.signal.windows.tukey(n, 0.5)
        for (int i = t; i < n; i += kT) {
            const int m = min(i, n - 1 - i);
            const double w = (n > 1 && m <= width) ? 0.5 * (1.0 - cos(4.0 * M_PI * m / (n - 1))) : 1.0;
            xw[i] = w * (double)xs[i];
        }
        __syncthreads();
        double r[16 + kMaxLpc];
#pragma unroll
        for (int j = 0; j < 16 + kMaxLpc; ++j) {
            const int i = 16 * t - kMaxLpc + j;
            r[j] = (i >= 0 && i < n) ? xw[i] : 0.0;
        }
        double ac[kMaxLpc + 1];
#pragma unroll
        for (int l = 0; l <= kMaxLpc; ++l) {
            double a = 0.0;
#pragma unroll
            for (int j = 0; j < 16; ++j) a = fma(r[kMaxLpc + j], r[kMaxLpc + j - l], a);
#pragma unroll
            for (int dl = 32; dl >= 1; dl >>= 1) a += __shfl_xor(a, dl);
            ac[l] = a;
        }
        if (lane == 0)
            for (int l = 0; l <= kMaxLpc; ++l) red[wave][l] = ac[l];
        __syncthreads();
        if (t == 0) {
            double R[kMaxLpc + 1];
            for (int l = 0; l <= kMaxLpc; ++l) R[l] = (red[0][l] + red[1][l]) + (red[2][l] + red[3][l]);
            // Levinson-Durbin: a[] = the error filter's coefficients, predictor coefficient j (of x[i - 1 - j]) = -a[j]
            double a[kMaxLpc], tmp[kMaxLpc], err = R[0];
            const int maxo = min(kMaxLpc, n - 1);
            int ok = 0;
            if (err > 0.0) {
                for (int o = 0; o < maxo; ++o) {
                    double k = -R[o + 1];
                    for (int j = 0; j < o; ++j) k -= a[j] * R[o - j];
                    k /= err;
                    for (int j = 0; j < o; ++j) tmp[j] = a[j] + k * a[o - 1 - j];
                    for (int j = 0; j < o; ++j) a[j] = tmp[j];
                    a[o] = k;
                    err *= 1.0 - k * k;
                    bool fin = isfinite(k);
                    for (int j = 0; j <= o; ++j) fin &= isfinite(a[j]);
                    if (!fin) break;
                    for (int j = 0; j <= o; ++j) lpc[o][j] = -a[j];
                    ok = o + 1;
                    if (!(err > 0.0)) break;
                }
            }
            nlpc = ok;
        }
        __syncthreads();
        if (t < nlpc) {   // libFLAC's quantiser at precision 15: the largest |coefficient| fills 15 signed bits, error feedback rounding
            const int order = t + 1;
            double cmax = 0.0;
            for (int j = 0; j < order; ++j) cmax = fmax(cmax, fabs(lpc[t][j]));
            int sh = 0;
            if (cmax > 0.0) {
                int e;
                frexp(cmax, &e);   // floor(log2 cmax) = e - 1
                sh = min(max(13 - (e - 1), 0), 15);
            }
            double acc = 0.0;
            for (int j = 0; j < order; ++j) {
                acc += lpc[t][j] * ldexp(1.0, sh);
                const int q = (int)fmin(fmax(round(acc), -16384.0), 16383.0);
                acc -= q;
                qc[t][j] = q;
            }
            qsh[t] = sh;
        }
        __syncthreads();

        // finest partitions: 2^pmax segments of z samples, r_ lanes each (a full block: 256 segments of 16 samples, one per lane)
        const int pmax = min(8, __builtin_ctz((unsigned)n));
        const int rl = kT >> pmax, z = n >> pmax;
        const int seg = t / rl, jl = t % rl;
        int xr[16 + kMaxLpc];
        if (rl == 1) {
#pragma unroll
            for (int j = 0; j < 16 + kMaxLpc; ++j) {
                const int i = t * z - kMaxLpc + j;
                xr[j] = (i >= 0 && i < n) ? xs[i] : 0;
            }
        }
        for (int c = 0; c < 5 + kMaxLpc; ++c) {
            const bool is_lpc = c >= 5;
            const int order = is_lpc ? c - 4 : c;
            if ((is_lpc && order > nlpc) || order >= n) continue;   // uniform
            const int sh = is_lpc ? qsh[order - 1] : 0;
            int q[kMaxLpc];
#pragma unroll
            for (int j = 0; j < kMaxLpc; ++j) q[j] = j < order ? (is_lpc ? qc[order - 1][j] : fixed_coef(order, j)) : 0;
            unsigned long long S[kMaxRice + 1];
#pragma unroll
            for (int k = 0; k <= kMaxRice; ++k) S[k] = 0;
            bool bad = false;
            auto add = [&](long long acc, int xi) {
                const long long e = (long long)xi - (acc >> sh);
                bad |= e < INT32_MIN || e > INT32_MAX;
                const int ei = (int)e;
                const unsigned u = ((unsigned)ei << 1) ^ (unsigned)(ei >> 31);
#pragma unroll
                for (int k = 0; k <= kMaxRice; ++k) S[k] += u >> k;
            };
            if (rl == 1) {
#pragma unroll
                for (int m = 0; m < 16; ++m) {
                    const int i = t * z + m;
                    if (m < z && i >= order) {
                        long long acc = 0;
#pragma unroll
                        for (int j = 0; j < kMaxLpc; ++j) acc += (long long)(q[j] * xr[kMaxLpc + m - 1 - j]);
                        add(acc, xr[kMaxLpc + m]);
                    }
                }
            } else {
                for (int i = seg * z + jl; i < (seg + 1) * z; i += rl) {
                    if (i < order) continue;
                    long long acc = 0;
                    for (int j = 0; j < order; ++j) acc += (long long)(q[j] * xs[i - 1 - j]);
                    add(acc, xs[i]);
                }
            }
            if (is_lpc && __syncthreads_or(bad)) continue;   // residuals outside int32: not a valid candidate
            // up the partition tree: groups of g lanes = the partitions of order p (g = 256 >> p)
            for (int p = 8; p >= 0; --p) {
                const int g = kT >> p;
                if (g >= 2 && g <= 64) {
#pragma unroll
                    for (int k = 0; k <= kMaxRice; ++k) S[k] += __shfl_xor(S[k], g >> 1);
                } else if (g == 128) {
                    if (lane == 0)
                        for (int k = 0; k <= kMaxRice; ++k) wsum[wave][k] = S[k];
                    __syncthreads();
                    for (int k = 0; k <= kMaxRice; ++k) S[k] = wsum[wave & ~1][k] + wsum[wave | 1][k];
                } else if (g == 256) {
                    for (int k = 0; k <= kMaxRice; ++k) S[k] = (wsum[0][k] + wsum[1][k]) + (wsum[2][k] + wsum[3][k]);
                }
                if (p > pmax || (n >> p) <= order) continue;
                const int part = t / g;
                if (t % g) continue;
                const long long np = (n >> p) - (part == 0 ? order : 0);
                unsigned long long bc = ~0ull;
                int bk = 0;
                for (int k = 0; k <= kMaxRice; ++k) {
                    const unsigned long long v = S[k] + (unsigned long long)np * (k + 1);
                    if (v < bc) {
                        bc = v;
                        bk = k;
                    }
                }
                atomicAdd(&tot[p], bc + 4);
                kc[(1 << p) - 1 + part] = (uint8_t)bk;
            }
            __syncthreads();
            if (t == 0) {
                int up = -1;
                for (int p = 0; p <= pmax; ++p) {
                    if ((n >> p) <= order) break;
                    const long long bits = preamble_bits(is_lpc ? kLpc : kFixed, order) - 4 + (long long)tot[p];   // tot counts partition 0's k
                    if (bits < best_bits) {
                        best_bits = bits;
                        best_method = is_lpc ? kLpc : kFixed;
                        best_order = order;
                        best_shift = sh;
                        best_p = p;
                        up = p;
                    }
                }
                for (int p = 0; p < 9; ++p) tot[p] = 0;
                if (up >= 0)
                    for (int j = 0; j < kMaxLpc; ++j) best_coef[j] = q[j];
                upd_p = up;
            }
            __syncthreads();
            const int up = upd_p;
            if (up >= 0 && t < (1 << up)) ksel[t] = kc[(1 << up) - 1 + t];
            __syncthreads();
        }
        if (t == 0 && 8 + 16LL * n < best_bits) {
            best_bits = 8 + 16LL * n;
            best_method = kVerbatim;
            best_order = best_p = best_shift = 0;
        }
    }
    if (t == 0) {
        d.x = x0;
        d.sig = s;
        d.n = n;
        d.fno = fno;
        d.method = best_method;
        d.order = best_order;
        d.shift = best_shift;
        d.p = best_p;
        d.hdr = hdr;
        d.bytes = hdr + (int)((best_bits + 7) / 8) + 2;
        d.pad = 0;
        for (int j = 0; j < kMaxLpc; ++j) d.coef[j] = best_method == kFixed || best_method == kLpc ? best_coef[j] : 0;
        best_method_s = best_method;
        best_p_s = best_p;
    }
    __syncthreads();
    const bool pred = best_method_s == kFixed || best_method_s == kLpc;
    d.k[t] = pred && t < (1 << best_p_s) ? ksel[t] : 0;
}

// ---- scan ----

constexpr int kScanT = 1024;

__global__ __launch_bounds__(kScanT) void k_flac_scan(const FlacDesc* __restrict__ dd, int nframes, const FlacSig* __restrict__ sg, int nsig,
                                                      int64_t* __restrict__ pre, int64_t* __restrict__ sig_bytes, int64_t* __restrict__ sig_off,
                                                      unsigned* __restrict__ smin, unsigned* __restrict__ smax) {
    __shared__ long long wt[kScanT / 64];
    __shared__ long long carry_s;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    if (t == 0) carry_s = 0;
    __syncthreads();
    for (int base = 0; base < nframes; base += kScanT) {
        const int f = base + t;
        const long long v = f < nframes ? dd[f].bytes : 0;
        if (f < nframes) {
            atomicMin(smin + dd[f].sig, (unsigned)v);
            atomicMax(smax + dd[f].sig, (unsigned)v);
        }
        long long inc = v;
        for (int dl = 1; dl < 64; dl <<= 1) {
            const long long o = __shfl_up(inc, dl);
            if (lane >= dl) inc += o;
        }
        if (lane == 63) wt[wave] = inc;
        __syncthreads();
        long long before = carry_s;
        for (int w = 0; w < wave; ++w) before += wt[w];
        if (f < nframes) pre[f] = before + inc - v;
        __syncthreads();
        if (t == 0) {
            long long sum = 0;
            for (int w = 0; w < kScanT / 64; ++w) sum += wt[w];
            carry_s += sum;
        }
        __syncthreads();
    }
    if (t == 0) pre[nframes] = carry_s;
    __syncthreads();
    for (int s = t; s < nsig; s += kScanT) {
        const int64_t f0 = sg[s].f0, f1 = f0 + (sg[s].n + kFlacBlock - 1) / kFlacBlock;
        const int64_t own = sg[s].hdr ? kFlacStreamHeader : 0;
        sig_off[s] = sg[s].hoff - own + pre[f0];
        sig_bytes[s] = own + pre[f1] - pre[f0];
    }
    if (t == 0) sig_bytes[nsig] = sg[nsig - 1].hoff + carry_s;
}

// ---- pack ----

// a field of w <= 16 bits at stream bit `pos` (MSB first); word i of b holds stream bytes 4i .. 4i + 3, the first one in bits 31..24
__device__ __forceinline__ void put_bits(unsigned* b, unsigned pos, unsigned v, int w) {
    v &= (1u << w) - 1;
    const int sh = 32 - (int)(pos & 31) - w;
    if (sh >= 0) {
        atomicOr(b + (pos >> 5), v << sh);
    } else {
        atomicOr(b + (pos >> 5), v >> -sh);
        atomicOr(b + (pos >> 5) + 1, v << (32 + sh));
    }
}

__device__ __forceinline__ unsigned get_byte(const unsigned* b, int i) { return (b[i >> 2] >> (24 - 8 * (i & 3))) & 0xFFu; }

// a * b mod x^16 + x^15 + x^2 + 1 over GF(2)
__device__ __forceinline__ unsigned gf_mulmod(unsigned a, unsigned b) {
    unsigned r = 0;
    for (int i = 15; i >= 0; --i) {
        r <<= 1;
        if (r & 0x10000u) r ^= 0x18005u;
        if ((b >> i) & 1u) r ^= a;
    }
    return r;
}

// x^(8 nbytes) mod the CRC-16 polynomial: crc(A || B) = crc(A) x^(8 |B|) + crc(B) for a CRC with init 0 and no final xor
__device__ __forceinline__ unsigned x8pow(unsigned nbytes) {
    unsigned r = 1, b = 0x100;
    while (nbytes) {
        if (nbytes & 1u) r = gf_mulmod(r, b);
        b = gf_mulmod(b, b);
        nbytes >>= 1;
    }
    return r;
}

__host__ __device__ void write_streaminfo(uint8_t* o, int64_t n, unsigned fmin, unsigned fmax, int rate) {
    const uint8_t head[12] = {'f', 'L', 'a', 'C', 0x80, 0, 0, 34, kFlacBlock >> 8, kFlacBlock & 0xFF, kFlacBlock >> 8, kFlacBlock & 0xFF};
    for (int i = 0; i < 12; ++i) o[i] = head[i];
    for (int i = 0; i < 3; ++i) {
        o[12 + i] = (uint8_t)(fmin >> (16 - 8 * i));
        o[15 + i] = (uint8_t)(fmax >> (16 - 8 * i));
    }
    const unsigned long long v = ((unsigned long long)rate << 44) | (15ull << 36) | (unsigned long long)n;   // rate, channels - 1 = 0, bps - 1, samples
    for (int i = 0; i < 8; ++i) o[18 + i] = (uint8_t)(v >> (56 - 8 * i));
    for (int i = 26; i < kFlacStreamHeader; ++i) o[i] = 0;   // MD5 not computed
}

__global__ __launch_bounds__(kT) void k_flac_pack(const short* __restrict__ x, const FlacSig* __restrict__ sg, int nsig, int rate, int rate_code,
                                                  const FlacDesc* __restrict__ dd, const int64_t* __restrict__ pre, int nframes,
                                                  const int64_t* __restrict__ sig_off, const unsigned* __restrict__ smin,
                                                  const unsigned* __restrict__ smax, uint8_t* __restrict__ out, int64_t cap, int64_t* err) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    if ((int)blockIdx.x >= nframes) {   // STREAMINFO of signals (blockIdx - nframes) * 256 + t
        const int s = ((int)blockIdx.x - nframes) * kT + t;
        if (s >= nsig || !sg[s].hdr) return;
        const bool any = sg[s].n > 0;
        if (sig_off[s] + kFlacStreamHeader > cap) {
            atomicOr((unsigned long long*)err, 2ull);
            return;
        }
        write_streaminfo(out + sig_off[s], sg[s].n, any ? smin[s] : 0, any ? smax[s] : 0, rate);
        return;
    }
    __shared__ int xs[kFlacBlock];
    __shared__ unsigned bits[kBitWords];
    __shared__ unsigned short crct[256];
    __shared__ unsigned wtot[kT / 64], wcrc[kT / 64];
    const int f = blockIdx.x;
    const FlacDesc& d = dd[f];
    const int n = d.n, method = d.method, order = d.order, sh = d.shift, p = d.p, hdr = d.hdr;
    for (int i = t; i < n; i += kT) xs[i] = x[d.x + i];
    for (int i = t; i < kBitWords; i += kT) bits[i] = 0;
    {
        unsigned c = (unsigned)t << 8;
        for (int b = 0; b < 8; ++b) c = (c & 0x8000u) ? (c << 1) ^ 0x8005u : c << 1;
        crct[t] = (unsigned short)(c & 0xFFFFu);
    }
    __syncthreads();
    const unsigned sub = 8u * hdr;   // first bit of the subframe
    const bool pred = method == kFixed || method == kLpc;
    // residual code lengths of the lane's 16 contiguous samples, then a block scan
    unsigned len[16], u[16];
    unsigned mine = 0;
    const int P = pred ? n >> p : 1;
    if (pred) {
        int q[kMaxLpc];
#pragma unroll
        for (int j = 0; j < kMaxLpc; ++j) q[j] = d.coef[j];
        int xr[16 + kMaxLpc];
#pragma unroll
        for (int j = 0; j < 16 + kMaxLpc; ++j) {
            const int i = 16 * t - kMaxLpc + j;
            xr[j] = (i >= 0 && i < n) ? xs[i] : 0;
        }
#pragma unroll
        for (int m = 0; m < 16; ++m) {
            const int i = 16 * t + m;
            len[m] = u[m] = 0;
            if (i < n && i >= order) {
                long long acc = 0;
#pragma unroll
                for (int j = 0; j < kMaxLpc; ++j) acc += (long long)(q[j] * xr[kMaxLpc + m - 1 - j]);
                const int e = (int)((long long)xr[kMaxLpc + m] - (acc >> sh));
                u[m] = ((unsigned)e << 1) ^ (unsigned)(e >> 31);
                const int part = i / P, k = d.k[part];
                len[m] = (u[m] >> k) + 1 + k + ((i % P == 0 && part > 0) ? 4 : 0);
            }
            mine += len[m];
        }
    }
    unsigned inc = mine;
    for (int dl = 1; dl < 64; dl <<= 1) {
        const unsigned o = __shfl_up(inc, dl);
        if (lane >= dl) inc += o;
    }
    if (lane == 63) wtot[wave] = inc;
    __syncthreads();
    unsigned before = inc - mine, all = 0;
    for (int w = 0; w < kT / 64; ++w) {
        if (w < wave) before += wtot[w];
        all += wtot[w];
    }
    const long long body = method == kConstant ? 8 + 16 : method == kVerbatim ? 8 + 16LL * n : preamble_bits(method, order) + (long long)all;
    const int F = hdr + (int)((body + 7) / 8);   // frame bytes before the CRC-16
    const int64_t off = sg[d.sig].hoff + pre[f];
    if (F + 2 != d.bytes || F + 2 > 4 * kBitWords || off + F + 2 > cap) {   // the analysis and the packing disagree, or no room: refuse
        if (t == 0) atomicOr((unsigned long long*)err, 1ull);
        return;
    }
    if (t == 0) {
        uint8_t hb[16];
        int nb = 0;
        hb[nb++] = 0xFF;
        hb[nb++] = 0xF8;
        const int bs_code = n == kFlacBlock ? 0xC : n <= 256 ? 0x6 : 0x7;
        hb[nb++] = (uint8_t)(bs_code << 4 | rate_code);
        hb[nb++] = 0x08;   // mono, 16 bits, reserved 0
        const unsigned fn = (unsigned)d.fno;
        const int ul = utf8_len(fn);
        if (ul == 1) {
            hb[nb++] = (uint8_t)fn;
        } else {
            hb[nb++] = (uint8_t)(((0xFF00u >> ul) & 0xFFu) | (fn >> (6 * (ul - 1))));
            for (int i = ul - 2; i >= 0; --i) hb[nb++] = (uint8_t)(0x80u | ((fn >> (6 * i)) & 0x3Fu));
        }
        if (n != kFlacBlock) {
            if (n <= 256) {
                hb[nb++] = (uint8_t)(n - 1);
            } else {
                hb[nb++] = (uint8_t)((n - 1) >> 8);
                hb[nb++] = (uint8_t)(n - 1);
            }
        }
        unsigned c8 = 0;
        for (int i = 0; i < nb; ++i) {
            c8 ^= hb[i];
            for (int b = 0; b < 8; ++b) c8 = (c8 & 0x80u) ? ((c8 << 1) ^ 0x07u) & 0xFFu : (c8 << 1) & 0xFFu;
        }
        hb[nb++] = (uint8_t)c8;
        for (int i = 0; i < nb; ++i) put_bits(bits, 8u * i, hb[i], 8);
        unsigned pos = sub;
        if (method == kConstant) {
            put_bits(bits, pos, 0x00, 8);
            put_bits(bits, pos + 8, (unsigned)xs[0], 16);
        } else if (method == kVerbatim) {
            put_bits(bits, pos, 0x02, 8);
        } else {
            put_bits(bits, pos, method == kFixed ? (0x08u | order) << 1 : (0x20u | (order - 1)) << 1, 8);
            pos += 8;
            for (int j = 0; j < order; ++j, pos += 16) put_bits(bits, pos, (unsigned)xs[j], 16);
            if (method == kLpc) {
                put_bits(bits, pos, 14, 4);   // precision - 1
                put_bits(bits, pos + 4, (unsigned)sh, 5);
                pos += 9;
                for (int j = 0; j < order; ++j, pos += 15) put_bits(bits, pos, (unsigned)d.coef[j], 15);
            }
            put_bits(bits, pos, 0, 2);   // Rice, 4-bit parameters
            put_bits(bits, pos + 2, (unsigned)p, 4);
            put_bits(bits, pos + 6, d.k[0], 4);
        }
    }
    if (method == kVerbatim) {
        for (int i = t; i < n; i += kT) put_bits(bits, sub + 8 + 16u * i, (unsigned)xs[i], 16);
    } else if (pred) {
        unsigned pos = sub + preamble_bits(method, order) + before;
#pragma unroll
        for (int m = 0; m < 16; ++m) {
            const int i = 16 * t + m;
            if (len[m]) {
                const int part = i / P, k = d.k[part];
                if (i % P == 0 && part > 0) {
                    put_bits(bits, pos, (unsigned)k, 4);
                    pos += 4;
                }
                put_bits(bits, pos + (u[m] >> k), (1u << k) | (u[m] & ((1u << k) - 1)), k + 1);
                pos += (u[m] >> k) + 1 + k;
            }
        }
    }
    __syncthreads();
    // CRC-16 of bytes [0, F): per-lane spans, each lane's CRC shifted past the bytes after its span, xor-combined
    const int span = (F + kT - 1) / kT, b0 = min(F, t * span), b1 = min(F, b0 + span);
    unsigned c = 0;
    for (int i = b0; i < b1; ++i) c = ((c << 8) ^ crct[((c >> 8) ^ get_byte(bits, i)) & 0xFFu]) & 0xFFFFu;
    if (b1 > b0) c = gf_mulmod(c, x8pow((unsigned)(F - b1)));
    for (int dl = 32; dl >= 1; dl >>= 1) c ^= __shfl_xor(c, dl);
    if (lane == 0) wcrc[wave] = c;
    __syncthreads();
    if (t == 0) put_bits(bits, 8u * F, wcrc[0] ^ wcrc[1] ^ wcrc[2] ^ wcrc[3], 16);
    __syncthreads();
    uint8_t* o = out + off;
    for (int i = t; i < F + 2; i += kT) o[i] = (uint8_t)get_byte(bits, i);
}

}  // namespace

int64_t flac_bound(int64_t n) {
    const int64_t frames = (n + kFlacBlock - 1) / kFlacBlock;
    return kFlacStreamHeader + frames * (kFlacMaxFrameHeader + 1 + 2) + 2 * n;
}

int flac_rate_code(int rate) {
    switch (rate) {
        case 8000: return 0x4;
        case 16000: return 0x5;
        case 22050: return 0x6;
        case 24000: return 0x7;
        case 32000: return 0x8;
        case 44100: return 0x9;
        case 48000: return 0xA;
    }
    throw std::runtime_error("unsupported sample rate " + std::to_string(rate) + " (8000 16000 22050 24000 32000 44100 48000)");
}

int64_t FlacEncoder::encode(const int16_t* x_dev, const std::vector<int64_t>& offs, const std::vector<int64_t>& lens, int rate, hipStream_t s,
                            std::vector<int64_t>* bytes) {
    const int rate_code = flac_rate_code(rate);
    const int nsig = (int)lens.size();
    SBV2_REQUIRE(nsig >= 1 && offs.size() == lens.size(), "FLAC: no signal to encode");
    std::vector<FlacSig> sig(nsig);
    int64_t nframes = 0, cap = 0;
    for (int i = 0; i < nsig; ++i) {
        SBV2_REQUIRE(lens[i] >= 0 && lens[i] < (1ll << 36), "FLAC: signal length out of range");
        sig[i] = FlacSig{offs[i], lens[i], nframes, 0, (int64_t)kFlacStreamHeader * (i + 1), 1};
        nframes += (lens[i] + kFlacBlock - 1) / kFlacBlock;
        cap += flac_bound(lens[i]);
    }
    SBV2_REQUIRE(nframes < (1ll << 31), "FLAC: too many frames in one call");
    // device: [signals][sizes: nsig + total + error word][offsets][min frame][max frame]; frames: [descriptors][prefix: nframes + 1]
    const size_t sig_b = round_up64(sizeof(FlacSig) * nsig, 64), sz_b = round_up64(8 * (nsig + 2), 64), off_b = round_up64(8 * nsig, 64),
                 mm_b = round_up64(4 * nsig, 64);
    const size_t desc_b = round_up64(sizeof(FlacDesc) * nframes, 64), pre_b = 8 * (nframes + 1);
    void* sig_host = sig_host_.reserve(sig_b, s);   // (the buffers are only used on this context's stream)
    const int64_t* sizes_host = static_cast<const int64_t*>(sizes_host_.reserve(sz_b, s));
    char* sd = static_cast<char*>(sig_.reserve(sig_b + sz_b + off_b + 2 * mm_b, s));
    char* fd = static_cast<char*>(frames_.reserve(desc_b + pre_b, s));
    uint8_t* out = static_cast<uint8_t*>(out_.reserve((size_t)std::max<int64_t>(cap, 1), s));
    FlacSig* d_sig = reinterpret_cast<FlacSig*>(sd);
    int64_t* d_sizes = reinterpret_cast<int64_t*>(sd + sig_b);
    int64_t* d_off = reinterpret_cast<int64_t*>(sd + sig_b + sz_b);
    unsigned* d_min = reinterpret_cast<unsigned*>(sd + sig_b + sz_b + off_b);
    unsigned* d_max = reinterpret_cast<unsigned*>(sd + sig_b + sz_b + off_b + mm_b);
    FlacDesc* d_desc = reinterpret_cast<FlacDesc*>(fd);
    int64_t* d_pre = reinterpret_cast<int64_t*>(fd + desc_b);

    std::memcpy(sig_host, sig.data(), sizeof(FlacSig) * nsig);
    HIP_CHECK(hipMemcpyAsync(d_sig, sig_host, sizeof(FlacSig) * nsig, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemsetAsync(d_sizes, 0, 8 * (nsig + 2), s));
    HIP_CHECK(hipMemsetAsync(d_min, 0xFF, 4 * nsig, s));
    HIP_CHECK(hipMemsetAsync(d_max, 0, 4 * nsig, s));
    const short* xs = reinterpret_cast<const short*>(x_dev);
    if (nframes) hipLaunchKernelGGL(k_flac_analyse, dim3((unsigned)nframes), dim3(kT), 0, s, xs, d_sig, nsig, d_desc);
    hipLaunchKernelGGL(k_flac_scan, dim3(1), dim3(kScanT), 0, s, d_desc, (int)nframes, d_sig, nsig, d_pre, d_sizes, d_off, d_min, d_max);
    hipLaunchKernelGGL(k_flac_pack, dim3((unsigned)(nframes + (nsig + kT - 1) / kT)), dim3(kT), 0, s, xs, d_sig, nsig, rate, rate_code, d_desc,
                       d_pre, (int)nframes, d_off, d_min, d_max, out, cap, d_sizes + nsig + 1);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(sizes_host_.get(), d_sizes, 8 * (nsig + 2), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    SBV2_REQUIRE(sizes_host[nsig + 1] == 0, "FLAC encoder: internal error " + std::to_string(sizes_host[nsig + 1]) + " (frame sizes disagree)");
    bytes->assign(sizes_host, sizes_host + nsig);
    SBV2_REQUIRE(sizes_host[nsig] <= cap, "FLAC encoder: stream larger than its bound");
    return sizes_host[nsig];
}

// ---- the encoder fed piece by piece ----
//
// One contiguous s16 buffer on the device: the carried tail (< 4096 samples) at its start, the push's samples written right behind it by the
// caller (dst()).  A push encodes the complete blocks of [tail | new samples] as ONE signal without a stream header whose first frame
// continues the count (FlacSig.fno0), with the three launches of FlacEncoder::encode, and moves the remainder to the front of the buffer (one
// device-to-device copy of < 8 KB; source and destination cannot overlap: the source starts at a block edge >= 4096).  The scan's prefix of
// the frame sizes and the error word lie in front of the packed bytes in one device region that ONE copy takes to the caller's pinned
// region: the frames' bound is copied, the host reads the sizes next to the bytes once the stream has passed the push.

namespace {
constexpr size_t kPushSig = 64;   // the push's FlacSig at the head of the pinned region (uploaded from there: the region lives until the push is delivered)
int64_t push_frames_max(int64_t max_push) { return (max_push + 2 * (kFlacBlock - 1)) / kFlacBlock; }   // ceil((4095 + n) / 4096), the short last frame included
size_t push_meta_bytes(int64_t max_push) { return round_up64(8 * (push_frames_max(max_push) + 2), 64); }   // error word + prefix[frames + 1], at most
}  // namespace

int64_t flac_stream_bound(int64_t n) { return kFlacStreamHeader + push_frames_max(n) * (kFlacMaxFrameHeader + 1 + 2) + 2 * (n + kFlacBlock - 1); }

size_t FlacStreamEncoder::host_bytes(int64_t max_push) {
    return kPushSig + push_meta_bytes(max_push) + (size_t)(flac_stream_bound(max_push) - kFlacStreamHeader);
}

void FlacStreamEncoder::begin(int rate, int64_t total_samples, int64_t max_push, hipStream_t s) {
    rate_code_ = flac_rate_code(rate);
    SBV2_REQUIRE(total_samples >= 0 && total_samples < (1ll << 36) && max_push >= 0, "FLAC: stream length out of range");
    static_assert(sizeof(FlacSig) <= kPushSig, "the push's signal entry outgrew its place");
    rate_ = rate;
    total_ = total_samples;
    max_push_ = max_push;
    fed_ = frames_ = tail_ = 0;
    done_ = false;
    const int64_t fmax = push_frames_max(max_push);
    buf_.reserve(sizeof(int16_t) * (size_t)(kFlacBlock + max_push), s);
    // [signal][sizes: 1 + total][offset][min frame][max frame] (what k_flac_scan writes per signal; a fed stream reads none of it back)
    tab_.reserve(kPushSig + 64 * 4, s);
    desc_.reserve(sizeof(FlacDesc) * (size_t)fmax, s);
    out_.reserve(push_meta_bytes(max_push) + (size_t)(flac_stream_bound(max_push) - kFlacStreamHeader), s);
}

int16_t* FlacStreamEncoder::dst() const { return buf_.as<int16_t>() + tail_; }

void FlacStreamEncoder::header(uint8_t* out) const { write_streaminfo(out, total_, 0, 0, rate_); }   // frame sizes unknown ahead: 0 (RFC 9639 8.2)

FlacStreamEncoder::Push FlacStreamEncoder::push(int64_t n, bool last, void* host, hipStream_t s) {
    SBV2_REQUIRE(rate_code_ >= 0 && !done_, "FLAC stream: push without begin, or after the last push");
    SBV2_REQUIRE(n >= 0 && n <= max_push_ && fed_ + n <= total_, "FLAC stream: push of " + std::to_string(n) + " samples outgrows what begin announced");
    SBV2_REQUIRE(!last || fed_ + n == total_, "FLAC stream: the last push ends " + std::to_string(total_ - fed_ - n) + " samples short of the announced length");
    const int64_t have = tail_ + n;
    const int64_t enc = last ? have : have / kFlacBlock * kFlacBlock;   // samples this push encodes
    const int nf = (int)((enc + kFlacBlock - 1) / kFlacBlock);
    SBV2_REQUIRE(frames_ + nf < (1ll << 31), "FLAC: too many frames in one stream");
    char* hb = static_cast<char*>(host);
    const size_t meta = round_up64(8 * (nf + 2), 64);   // the push's own error word + prefix[nf + 1]: a region sized for n samples holds a push of n
    Push r;
    r.first_frame = frames_;
    r.frames = nf;
    r.err = reinterpret_cast<const int64_t*>(hb + kPushSig);
    r.pre = r.err + 1;
    r.bytes = reinterpret_cast<const uint8_t*>(hb + kPushSig + meta);
    if (nf) {
        const FlacSig sig{0, enc, 0, frames_, 0, 0};
        std::memcpy(hb, &sig, sizeof sig);
        char* tab = tab_.as<char>();
        FlacSig* d_sig = reinterpret_cast<FlacSig*>(tab);
        int64_t* d_sizes = reinterpret_cast<int64_t*>(tab + kPushSig);
        int64_t* d_off = reinterpret_cast<int64_t*>(tab + kPushSig + 64);
        unsigned* d_min = reinterpret_cast<unsigned*>(tab + kPushSig + 128);
        unsigned* d_max = reinterpret_cast<unsigned*>(tab + kPushSig + 192);
        int64_t* d_err = out_.as<int64_t>();
        int64_t* d_pre = d_err + 1;
        uint8_t* d_bytes = out_.as<uint8_t>() + meta;
        const int64_t cap = (int64_t)nf * (kFlacMaxFrameHeader + 1 + 2) + 2 * enc;
        const short* xs = reinterpret_cast<const short*>(buf_.get());
        HIP_CHECK(hipMemcpyAsync(d_sig, hb, sizeof sig, hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemsetAsync(d_err, 0, 8, s));
        hipLaunchKernelGGL(k_flac_analyse, dim3((unsigned)nf), dim3(kT), 0, s, xs, d_sig, 1, desc_.as<FlacDesc>());
        // (d_min / d_max are not initialised here, unlike in FlacEncoder::encode: the scan's atomicMin / atomicMax need valid words only.  Their
        // results feed the STREAMINFO that k_flac_pack writes for a signal with a header; a push has none, and nothing reads them back.)
        hipLaunchKernelGGL(k_flac_scan, dim3(1), dim3(kScanT), 0, s, desc_.as<FlacDesc>(), nf, d_sig, 1, d_pre, d_sizes, d_off, d_min, d_max);
        hipLaunchKernelGGL(k_flac_pack, dim3((unsigned)nf), dim3(kT), 0, s, xs, d_sig, 1, rate_, rate_code_, desc_.as<FlacDesc>(), d_pre, nf, d_off,
                           d_min, d_max, d_bytes, cap, d_err);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(hb + kPushSig, d_err, meta + (size_t)cap, hipMemcpyDeviceToHost, s));
        const int64_t rest = have - enc;
        if (rest) HIP_CHECK(hipMemcpyAsync(buf_.get(), buf_.as<int16_t>() + enc, sizeof(int16_t) * (size_t)rest, hipMemcpyDeviceToDevice, s));
        tail_ = rest;
    } else {
        tail_ = have;
    }
    fed_ += n;
    frames_ += nf;
    done_ = last;
    return r;
}

int64_t FlacStreamEncoder::Push::size(int f0, int f1) const {
    if (f0 >= f1) return 0;
    SBV2_REQUIRE(f0 >= 0 && f1 <= frames, "FLAC stream: frame range outside its push");
    SBV2_REQUIRE(*err == 0, "FLAC encoder: internal error " + std::to_string(*err) + " (frame sizes disagree)");
    return pre[f1] - pre[f0];
}

}  // namespace sbv2
