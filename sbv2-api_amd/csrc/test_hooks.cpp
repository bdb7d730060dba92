// The test hooks of libsbv2_hip.so (the sbv2_debug_* entry points of include/sbv2_hip.h): one kernel or launcher at a time on host data, for the tests
// and the probe tools.  The decoder's kernels get their parameters from the decoder's own builders (decoder_cl.cpp: pack_decoder_conv, conv_cl_params,
// step_params, branch_params, clx_conv1_params, clx_conv2_params), so a test of a kernel also tests what the decoder launches.  The launchers of ops.h
// (LayerNorm, the duration flow's pieces, noise, the generator tail, the movers) have one hook per launcher or family, on planes at the library's pitches
// and layouts built by the models' own make_layout, with the attention hooks' poison / sentinel / stray-count convention (tests/test_ops_kernels.py).
#include <cstring>
#include <limits>
#include <memory>

#include "api_internal.h"

namespace {

// Device memory, freed on scope exit (at least 16 bytes, so that an empty operand is still a valid address)
struct DevMem {
    void* p = nullptr;
    explicit DevMem(size_t bytes) { HIP_CHECK(hipMalloc(&p, std::max<size_t>(bytes, 16))); }
    DevMem(const void* src, size_t bytes) : DevMem(bytes) {
        if (bytes) HIP_CHECK(hipMemcpy(p, src, bytes, hipMemcpyHostToDevice));
    }
    ~DevMem() { (void)hipFree(p); }
    DevMem(const DevMem&) = delete;
    DevMem& operator=(const DevMem&) = delete;
    float* f() const { return static_cast<float*>(p); }
    unsigned char* u8() const { return static_cast<unsigned char*>(p); }
};

Blob one_conv_blob(const float* w, const float* bias, std::vector<int64_t> dims, int64_t nbias) {
    Blob b;
    b.kind = 0;
    HostTensor t;
    t.dims = std::move(dims);
    t.data = w;
    b.tensors.emplace("c.weight", t);
    if (bias) {
        HostTensor tb;
        tb.dims = {nbias};
        tb.data = bias;
        b.tensors.emplace("c.bias", tb);
    }
    return b;
}

// Average milliseconds of one run() over `iters` back-to-back runs on the null stream
template <class F>
float time_ms(int64_t iters, F&& run) {
    struct Event {
        hipEvent_t e = nullptr;
        Event() { HIP_CHECK(hipEventCreate(&e)); }
        ~Event() { (void)hipEventDestroy(e); }
    } e0, e1;
    HIP_CHECK(hipEventRecord(e0.e, nullptr));
    for (int64_t i = 0; i < iters; ++i) run();
    HIP_CHECK(hipEventRecord(e1.e, nullptr));
    HIP_CHECK(hipEventSynchronize(e1.e));
    float t = 0.f;
    HIP_CHECK(hipEventElapsedTime(&t, e0.e, e1.e));
    return t / (float)iters;
}

// A channel-major host plane x [C][L] as a channels-last device plane [L][C], and back
DevMem upload_cl(const float* x, int64_t C, int64_t L) {
    std::vector<float> t((size_t)L * C);
    for (int64_t c = 0; c < C; ++c)
        for (int64_t n = 0; n < L; ++n) t[(size_t)n * C + c] = x[(size_t)c * L + n];
    return DevMem(t.data(), sizeof(float) * t.size());
}
void download_cl(const float* d, int64_t C, int64_t L, float* y) {
    std::vector<float> t((size_t)L * C);
    HIP_CHECK(hipMemcpy(t.data(), d, sizeof(float) * t.size(), hipMemcpyDeviceToHost));
    for (int64_t c = 0; c < C; ++c)
        for (int64_t n = 0; n < L; ++n) y[(size_t)c * L + n] = t[(size_t)n * C + c];
}

// hi + lo of the bf16 parts planes sp (conv_clx.hip's operand format) as a channel-major host plane [C][N]
void read_parts(const SplitClPlanes& sp, float* out) {
    const int64_t rows = sp.front + sp.N + sp.back;
    std::vector<uint16_t> h(split_cl_bytes(sp.C, sp.N) / 2);
    HIP_CHECK(hipMemcpy(h.data(), sp.p, h.size() * 2, hipMemcpyDeviceToHost));
    auto f = [](uint16_t v) {
        const uint32_t u = (uint32_t)v << 16;
        float o;
        std::memcpy(&o, &u, 4);
        return o;
    };
    for (int64_t c = 0; c < sp.C; ++c)
        for (int64_t n = 0; n < sp.N; ++n) {
            const size_t hi = ((size_t)(c >> 4) * 2 * rows + sp.front + n) * 16 + (c & 15);
            out[(size_t)c * sp.N + n] = f(h[hi]) + f(h[hi + (size_t)rows * 16]);
        }
}

// Packed planes of the attention hooks: host [R][sum lens] (utterances concatenated) <-> rows of a device plane at the layout's columns.  poison: every
// column outside an utterance, up to the pitch, holds NaN (all bits set) instead of zero.
void upload_packed(const float* x, const SegLayout& lay, Plane P, bool poison) {
    HIP_CHECK(hipMemset(P.p, poison ? 0xFF : 0, sizeof(float) * (size_t)P.C * P.ld));
    int64_t total = 0;
    for (int v : lay.len) total += v;
    int64_t e = 0;
    for (int u = 0; u < lay.n; ++u) {
        HIP_CHECK(hipMemcpy2D(P.p + lay.start[u], sizeof(float) * P.ld, x + e, sizeof(float) * total, sizeof(float) * lay.len[u], P.C, hipMemcpyHostToDevice));
        e += lay.len[u];
    }
}
// V token-major [N][ldvt] (the unfused path's V^T operand; linear_tokmajor in the model), same poison rule
DevMem upload_tokmajor(const float* x, const SegLayout& lay, int R, bool poison) {
    std::vector<float> t((size_t)lay.L * R, poison ? std::numeric_limits<float>::quiet_NaN() : 0.f);
    int64_t total = 0;
    for (int v : lay.len) total += v;
    int64_t e = 0;
    for (int u = 0; u < lay.n; ++u)
        for (int j = 0; j < lay.len[u]; ++j, ++e)
            for (int c = 0; c < R; ++c) t[(size_t)(lay.start[u] + j) * R + c] = x[(size_t)c * total + e];
    return DevMem(t.data(), sizeof(float) * t.size());
}
// ctx fill before the launch: the sentinel (poison) or zero (as the models clear it)
constexpr unsigned char kCtxSentinel = 0x5A;
void download_packed(Plane P, const SegLayout& lay, bool poison, float* y, int64_t* stray) {
    std::vector<float> h((size_t)P.C * P.ld);
    HIP_CHECK(hipMemcpy(h.data(), P.p, sizeof(float) * h.size(), hipMemcpyDeviceToHost));
    int64_t total = 0;
    for (int v : lay.len) total += v;
    std::vector<unsigned char> inside(P.ld, 0);
    int64_t e = 0;
    for (int u = 0; u < lay.n; ++u) {
        for (int c = 0; c < P.C; ++c) std::memcpy(y + (size_t)c * total + e, &h[(size_t)c * P.ld + lay.start[u]], sizeof(float) * lay.len[u]);
        std::memset(&inside[lay.start[u]], 1, lay.len[u]);
        e += lay.len[u];
    }
    if (!stray) return;
    *stray = 0;
    if (!poison) return;
    uint32_t sent;
    std::memset(&sent, kCtxSentinel, 4);
    for (int c = 0; c < P.C; ++c)
        for (int n = 0; n < P.ld; ++n) {
            uint32_t b;
            std::memcpy(&b, &h[(size_t)c * P.ld + n], 4);
            *stray += !inside[n] && b != sent;
        }
}

// the signals of the audio hooks: lens[i] samples each, back to back; *total = their sum
std::vector<FmtSignal> packed_signals(const int64_t* lens, int nsig, int64_t* total) {
    std::vector<FmtSignal> sig(nsig);
    *total = 0;
    for (int i = 0; i < nsig; ++i) {
        SBV2_REQUIRE(lens[i] >= 0, "negative signal length");
        sig[i] = FmtSignal{0, lens[i], *total, 0, 0};
        *total += lens[i];
    }
    return sig;
}

// Scratch of one audio hook call on `device`: a non-blocking stream and the hook's input uploaded on it (x stays null for an empty input
// unless min_bytes asks for an allocation anyway).  The stream is drained before the buffer and the stream go.
struct AudioScratch {
    hipStream_t s = nullptr;
    DeviceBuffer x;
    AudioScratch(int device, const void* src, size_t bytes, size_t min_bytes = 0) {
        HIP_CHECK(hipSetDevice(device));
        HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        try {
            if (std::max(bytes, min_bytes)) x.reserve(std::max(bytes, min_bytes), s);
            if (bytes) HIP_CHECK(hipMemcpyAsync(x.get(), src, bytes, hipMemcpyHostToDevice, s));
        } catch (...) {
            release();
            throw;
        }
    }
    ~AudioScratch() { release(); }
    void release() {
        (void)hipStreamSynchronize(s);
        x = DeviceBuffer();
        (void)hipStreamDestroy(s);
    }
    AudioScratch(const AudioScratch&) = delete;
    AudioScratch& operator=(const AudioScratch&) = delete;
};

// The packed f64 input of the *_parts hooks (tests/test_loudness_limiter_kernels.py): kPad NaN words (all bits set), the total samples, kPad NaN
// words.  The signal starts at words[kPad]; a read outside [0, total) poisons what it feeds.
struct PoisonedSignal {
    static constexpr size_t kPad = 64;
    std::vector<double> words;
    PoisonedSignal(const double* x, int64_t total) : words((size_t)total + 2 * kPad) {
        std::memset(words.data(), 0xFF, sizeof(double) * words.size());
        if (total) std::memcpy(words.data() + kPad, x, sizeof(double) * (size_t)total);
    }
};
// the words of [a, b) that no longer hold the sentinel fill (kCtxSentinel in every byte)
int64_t sentinel_strays(const double* a, const double* b) {
    uint64_t sent;
    std::memset(&sent, kCtxSentinel, 8);
    int64_t bad = 0;
    for (; a < b; ++a) {
        uint64_t v;
        std::memcpy(&v, a, 8);
        bad += v != sent;
    }
    return bad;
}

// ---- the hooks of ops.h's launchers (tests/test_ops_kernels.py) ----------------------------------------------------------------------------------------
// A host plane [C][L] on the device at the library's pitch (Arena::plane's rule: a multiple of 64 floats).  poison: the columns between L and the pitch,
// and every column where inside[n] == 0 (inside may be null), hold NaN (all bits set) instead of zero.  Outputs are pre-filled with the sentinel; after
// the launch get() counts the pad words (columns L .. pitch) that no longer hold what they held before it.
constexpr uint32_t kSentinelWord = 0x5A5A5A5Au, kNanWord = 0xFFFFFFFFu;
struct DevPlane {
    Plane P;
    DevMem m;
    DevPlane(int64_t C, int64_t L) : P{nullptr, (int)C, (int)L, round_up((int)L, 64)}, m(sizeof(float) * (size_t)C * round_up((int)L, 64)) {
        SBV2_REQUIRE(C >= 1 && L >= 1 && L < (1 << 28) && C < (1 << 20), "bad plane shape");
        P.p = m.f();
    }
    void put(const float* x, bool poison, const unsigned char* inside = nullptr) {
        std::vector<float> h((size_t)P.C * P.ld, poison ? std::numeric_limits<float>::quiet_NaN() : 0.f);
        if (poison) std::memset(h.data(), 0xFF, sizeof(float) * h.size());
        for (int c = 0; c < P.C; ++c)
            for (int n = 0; n < P.L; ++n)
                if (!poison || !inside || inside[n]) h[(size_t)c * P.ld + n] = x[(size_t)c * P.L + n];
        HIP_CHECK(hipMemcpy(P.p, h.data(), sizeof(float) * h.size(), hipMemcpyHostToDevice));
    }
    void fill(bool poison) { HIP_CHECK(hipMemset(P.p, poison ? kCtxSentinel : 0, sizeof(float) * (size_t)P.C * P.ld)); }
    // y [C][L] (any 4-byte element type); returns the number of pad words that are not `pad`
    int64_t get(void* y, uint32_t pad) const {
        std::vector<uint32_t> h((size_t)P.C * P.ld);
        HIP_CHECK(hipMemcpy(h.data(), P.p, 4 * h.size(), hipMemcpyDeviceToHost));
        int64_t stray = 0;
        for (int c = 0; c < P.C; ++c) {
            std::memcpy(static_cast<uint32_t*>(y) + (size_t)c * P.L, &h[(size_t)c * P.ld], 4 * (size_t)P.L);
            for (int n = P.L; n < P.ld; ++n) stray += h[(size_t)c * P.ld + n] != pad;
        }
        return stray;
    }
};
// the text encoder's layout (kind 0: kTextGap, columns rounded to 4) or the flow's / decoder's (kind 1: kFrameGap, rounded to 32), as VitsModel builds them
SegLayout hook_layout(const int64_t* lens, int nutt, int kind, Arena& ar, const unsigned char* extra_mask = nullptr) {
    SBV2_REQUIRE(lens && nutt >= 1 && (kind == 0 || kind == 1), "bad layout arguments");
    std::vector<int> L(nutt);
    for (int i = 0; i < nutt; ++i) {
        SBV2_REQUIRE(lens[i] >= 1 && lens[i] < (1 << 20), "bad sequence length");
        L[i] = (int)lens[i];
    }
    return kind ? make_layout(L, kFrameGap, ar, nullptr, extra_mask, 32) : make_layout(L, kTextGap, ar, nullptr, extra_mask);
}
// inside[n] = column n / div belongs to an utterance
std::vector<unsigned char> layout_inside(const SegLayout& lay, int div = 1) {
    std::vector<unsigned char> in((size_t)lay.L * div, 0);
    for (int u = 0; u < lay.n; ++u) std::memset(&in[(size_t)lay.start[u] * div], 1, (size_t)lay.len[u] * div);
    return in;
}
int* upload_ints(Arena& ar, const int32_t* v, size_t n) {
    int* d = ar.array<int>(std::max<size_t>(n, 1));
    if (n) HIP_CHECK(hipMemcpy(d, v, sizeof(int) * n, hipMemcpyHostToDevice));
    return d;
}

// the per-row option records of durations / noise_fill / expand_frames: null array = the scalar for every row (index null = the row number)
RowOpts* upload_rows(Arena& ar, int n, const uint64_t* seed, uint64_t seed1, const int32_t* index, const float* sdp_ratio, float sdp_ratio1,
                     const float* length_scale, float length_scale1, const float* noise_scale, float noise_scale1, const float* noise_scale_w,
                     float noise_scale_w1) {
    std::vector<RowOpts> r((size_t)std::max(n, 1));
    for (int u = 0; u < n; ++u)
        r[u] = RowOpts{seed ? seed[u] : seed1, index ? index[u] : u, sdp_ratio ? sdp_ratio[u] : sdp_ratio1, length_scale ? length_scale[u] : length_scale1,
                       noise_scale ? noise_scale[u] : noise_scale1, noise_scale_w ? noise_scale_w[u] : noise_scale_w1, 0};
    RowOpts* d = ar.array<RowOpts>(r.size());
    HIP_CHECK(hipMemcpy(d, r.data(), sizeof(RowOpts) * r.size(), hipMemcpyHostToDevice));
    return d;
}

// ---- the repeated-launch screen of the inline-asm MFMA kernels (tests/test_mfma_repeatability.py) -------------------------------------------------------
// One launch is enqueued `reps` times on one stream without a host synchronisation in between, alternately on two inputs (repetition i: input and output
// plane i % 2).  Before each repetition the output is restored by a device-to-device copy (the previous contents under accumulate, else NaN: every row must be
// written); after it a comparison kernel counts the 32-bit words that differ from the FIRST result of the same input.  These kernels have no floating-point
// atomics and no order-dependent reduction, so any difference is a defect.  Optionally a second stream receives one launch per repetition from
// the same host loop, alternately a LayerNorm over a plane that reaches every CU and one gemm_bfs f16x3 product of DeBERTa's batch shape class: nothing polls,
// nothing waits for a condition, no graphs.
__global__ __launch_bounds__(256) void k_rep_compare(const uint32_t* __restrict__ got, const uint32_t* __restrict__ ref, size_t n, unsigned long long word0,
                                                     unsigned long long* mismatch, unsigned long long* first_bad) {
    const size_t n4 = n / 4, stride = (size_t)gridDim.x * blockDim.x, t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long cnt = 0, first = ~0ull;
    auto note = [&](size_t i) {
        ++cnt;
        if (i < first) first = i;
    };
    for (size_t i = t; i < n4; i += stride) {
        const uint4 a = reinterpret_cast<const uint4*>(got)[i], b = reinterpret_cast<const uint4*>(ref)[i];
        if (a.x != b.x) note(4 * i);
        if (a.y != b.y) note(4 * i + 1);
        if (a.z != b.z) note(4 * i + 2);
        if (a.w != b.w) note(4 * i + 3);
    }
    for (size_t i = 4 * n4 + t; i < n; i += stride)
        if (got[i] != ref[i]) note(i);
    if (cnt) {
        atomicAdd(mismatch, cnt);
        atomicMin(first_bad, word0 + first);
    }
}
__global__ void k_rep_flip(uint32_t* p, size_t word) { p[word] ^= 0x1000u; }

struct RepRegion {          // one buffer a launch writes: the two output planes, the first result of each input, what a repetition starts from (null: nothing)
    void* out[2];
    void* ref[2];
    const void* init;
    size_t words;
};
struct RepOpts {
    int reps, neighbour, flip_at;
    int64_t flip_word;
};
struct HookStream {
    hipStream_t s = nullptr;
    HookStream() { HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking)); }
    ~HookStream() {
        (void)hipStreamSynchronize(s);
        (void)hipStreamDestroy(s);
    }
    HookStream(const HookStream&) = delete;
    HookStream& operator=(const HookStream&) = delete;
};
// the other execution context's work: LayerNorm [1024][8192] (8192 columns: waves on every CU; little LDS, few registers) and W[1024][1024] x X[1024][2048]
// in f16x3 (128 tiles of 128 x 128: the batch instantiation)
struct RepNeighbour {
    static constexpr int kC = 1024, kL = 8192, kN = 2048;
    std::vector<float> w, bias;
    Blob blob;
    WeightStore ws;
    PackedConv pc;
    DevMem x, y, g, b, xs_mem, sk_mem;
    Plane X, Y, GX, GY;
    SplitPlanes xs;
    BfsSplitK sk;
    static std::vector<float> noise(size_t n, float scale, uint32_t st) {
        std::vector<float> v(n);
        for (auto& e : v) {
            st = st * 1664525u + 1013904223u;
            e = ((st >> 8) * (1.0f / 16777216.0f) - 0.5f) * scale;
        }
        return v;
    }
    static constexpr size_t kWs = (size_t)48 << 20;
    RepNeighbour()
        : w(noise((size_t)kC * kC, 0.1f, 1u)), bias(noise(kC, 1.f, 2u)), blob(one_conv_blob(w.data(), bias.data(), {kC, kC, 1}, kC)), ws(blob),
          x(sizeof(float) * kC * kL), y(sizeof(float) * kC * kL), g(sizeof(float) * kC), b(sizeof(float) * kC), xs_mem((size_t)2 * kC * kN * 2 + 64),
          sk_mem(kWs + 1024 * sizeof(float)) {
        ws.set_bfs_parts(kPartsF16x3);
        pc = ws.conv("c");
        const std::vector<float> hx = noise((size_t)kC * kL, 2.f, 3u);
        HIP_CHECK(hipMemcpy(x.p, hx.data(), sizeof(float) * hx.size(), hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(g.p, bias.data(), sizeof(float) * kC, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(b.p, bias.data(), sizeof(float) * kC, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemset(sk_mem.p, 0, kWs + 1024 * sizeof(float)));
        X = Plane{x.f(), kC, kL, kL};
        Y = Plane{y.f(), kC, kL, kL};
        GX = Plane{x.f(), kC, kN, kL};   // the product reads the first 2048 columns of the same plane and writes the LayerNorm's output plane
        GY = Plane{y.f(), kC, kN, kL};
        xs.p = xs_mem.p;
        xs.parts = 2;
        xs.f16 = 1;
        xs.sat = f16x3_sat_counter();
        xs.C = kC;
        xs.L = kN;
        xs.ld = kN;
        xs.pstride = (int64_t)kC * kN;
        split_planes(GX, xs, nullptr);
        sk.ws = sk_mem.f();
        sk.ws_bytes = kWs;
        sk.counters = reinterpret_cast<unsigned*>(sk_mem.f() + kWs / sizeof(float));
        sk.ncounters = 1024;
    }
    void launch(int i, hipStream_t s) {
        if (i & 1) conv_bfs(pc, xs, &GY, nullptr, nullptr, 1, s, ACT_NONE, nullptr, 1.0f, 1.0f, -1, 0, &sk);
        else layernorm_ch(X, Y, g.f(), b.f(), 1e-5f, ACT_NONE, nullptr, 0, nullptr, s);
    }
};

// launch(which, stream) enqueues the launch under test on input / output plane `which`
template <class F>
void run_repeated(const std::vector<RepRegion>& regs, const RepOpts& o, F&& launch, int64_t* mismatch, int64_t* first_bad) {
    SBV2_REQUIRE(o.reps >= 2 && o.reps <= 4096 && mismatch && first_bad && o.flip_at >= -1 && o.flip_at < o.reps, "bad repetition arguments");
    size_t total = 0;
    for (const RepRegion& r : regs) total += r.words;
    SBV2_REQUIRE(o.flip_at < 0 || (o.flip_word >= 0 && (size_t)o.flip_word < total), "flip_word lies outside what the launch writes");
    std::unique_ptr<RepNeighbour> nb;
    if (o.neighbour) nb.reset(new RepNeighbour());
    std::vector<unsigned long long> h((size_t)2 * o.reps, 0);
    for (int i = 0; i < o.reps; ++i) h[(size_t)o.reps + i] = ~0ull;
    DevMem dc(h.data(), sizeof(unsigned long long) * h.size());
    unsigned long long* cnt = static_cast<unsigned long long*>(dc.p);
    HIP_CHECK(hipDeviceSynchronize());   // (the uploads ran on the null stream, which the two streams below do not wait for)
    {
        HookStream A, B;
        for (int i = 0; i < o.reps; ++i) {
            const int w = i & 1;
            for (const RepRegion& r : regs)
                if (r.init) HIP_CHECK(hipMemcpyAsync(r.out[w], r.init, r.words * 4, hipMemcpyDeviceToDevice, A.s));
            launch(w, A.s);
            if (i < 2)
                for (const RepRegion& r : regs) HIP_CHECK(hipMemcpyAsync(r.ref[w], r.out[w], r.words * 4, hipMemcpyDeviceToDevice, A.s));
            size_t word0 = 0;
            for (const RepRegion& r : regs) {
                if (i == o.flip_at && (size_t)o.flip_word >= word0 && (size_t)o.flip_word < word0 + r.words)
                    hipLaunchKernelGGL(k_rep_flip, dim3(1), dim3(1), 0, A.s, static_cast<uint32_t*>(r.out[w]), (size_t)o.flip_word - word0);
                const unsigned grid = (unsigned)std::min<size_t>((r.words / 4 + 255) / 256 + 1, 2048);
                hipLaunchKernelGGL(k_rep_compare, dim3(grid), dim3(256), 0, A.s, static_cast<const uint32_t*>(r.out[w]), static_cast<const uint32_t*>(r.ref[w]),
                                   r.words, (unsigned long long)word0, cnt + i, cnt + o.reps + i);
                HIP_CHECK(hipGetLastError());
                word0 += r.words;
            }
            if (nb) nb->launch(i, B.s);
        }
        HIP_CHECK(hipStreamSynchronize(A.s));
        HIP_CHECK(hipStreamSynchronize(B.s));
    }
    HIP_CHECK(hipMemcpy(h.data(), dc.p, sizeof(unsigned long long) * h.size(), hipMemcpyDeviceToHost));
    for (int i = 0; i < o.reps; ++i) {
        mismatch[i] = (int64_t)h[i];
        first_bad[i] = h[(size_t)o.reps + i] == ~0ull ? -1 : (int64_t)h[(size_t)o.reps + i];
    }
}

// 0xFF bytes: NaN as f32 and as bf16
void fill_nan(DevMem& m, size_t bytes) { HIP_CHECK(hipMemset(m.p, 0xFF, bytes)); }

// the two inputs of a conv_clx launch as bf16 parts of lrelu(x, pre_slope): x channel-major [cin][L] on the host
struct ClxInputs {
    DevMem ma, mb;
    SplitClPlanes xs[2];
    ClxInputs(const float* xa, const float* xb, int64_t cin, int64_t L, float pre_slope) : ma(split_cl_bytes((int)cin, L) + 16), mb(split_cl_bytes((int)cin, L) + 16) {
        const float* hx[2] = {xa, xb};
        void* mem[2] = {ma.p, mb.p};
        for (int i = 0; i < 2; ++i) {
            DevMem dx = upload_cl(hx[i], cin, L);
            xs[i] = make_split_cl(mem[i], (int)cin, L, nullptr);
            split_cl(dx.f(), (int)cin, L, (int)cin, pre_slope, xs[i], nullptr);
            HIP_CHECK(hipDeviceSynchronize());
        }
    }
};
// p0 (everything but X, Y, Ys) repeated on in.xs[which]: the f32 plane [rows][C] starts every repetition as NaN, the parts planes (want_ys) as NaN between
// zeroed halo rows (make_split_cl's contract); the parts are compared word by word, halo rows included, behind the f32 plane's rows * C words
void repeat_clx(ConvClxParams p0, const ClxInputs& in, int64_t C, int64_t rows, int want_ys, const RepOpts& o, float* ya, float* yb, float* ysa, float* ysb,
                int64_t* mismatch, int64_t* first_bad) {
    const size_t ybytes = sizeof(float) * rows * C, ysbytes = want_ys ? split_cl_bytes((int)C, rows) + 16 : 0;
    DevMem dya(ybytes), dyb(ybytes), ra(ybytes), rb(ybytes), nan(ybytes), dysa(ysbytes), dysb(ysbytes), rsa(ysbytes), rsb(ysbytes), ysinit(ysbytes);
    fill_nan(nan, ybytes);
    SplitClPlanes ys[2], ysr[2];
    if (want_ys) {
        DevMem* mem[2] = {&dysa, &dysb};
        void* rmem[2] = {rsa.p, rsb.p};
        fill_nan(ysinit, ysbytes);
        (void)make_split_cl(ysinit.p, (int)C, rows, nullptr);
        for (int i = 0; i < 2; ++i) {
            fill_nan(*mem[i], ysbytes);
            ys[i] = make_split_cl(mem[i]->p, (int)C, rows, nullptr);
            ysr[i] = ys[i];
            ysr[i].p = rmem[i];
        }
    }
    p0.X = in.xs[0];
    p0.Y = dya.f();
    p0.Ys = want_ys ? ys[0] : SplitClPlanes();
    SBV2_REQUIRE(p0.W && conv_clx_usable(p0), "shape not supported by conv_clx");
    std::vector<RepRegion> regs{{{dya.p, dyb.p}, {ra.p, rb.p}, nan.p, (size_t)rows * C}};
    if (want_ys) regs.push_back(RepRegion{{dysa.p, dysb.p}, {rsa.p, rsb.p}, ysinit.p, split_cl_bytes((int)C, rows) / 4});
    run_repeated(regs, o,
                 [&](int which, hipStream_t s) {
                     ConvClxParams p = p0;
                     p.X = in.xs[which];
                     p.Y = static_cast<float*>(regs[0].out[which]);
                     if (want_ys) p.Ys = ys[which];
                     launch_conv_clx(p, s);
                 },
                 mismatch, first_bad);
    download_cl(ra.f(), C, rows, ya);
    download_cl(rb.f(), C, rows, yb);
    if (want_ys) {
        read_parts(ysr[0], ysa);
        read_parts(ysr[1], ysb);
    }
}

}  // namespace

extern "C" {

int sbv2_debug_flac_encode(int device, const int16_t* x, const int64_t* lens, int nsig, int32_t sample_rate, uint8_t* dst, int64_t capacity,
                           int64_t* out_bytes) {
    API_BEGIN
    SBV2_REQUIRE(nsig >= 1 && lens && dst && out_bytes, "bad arguments");
    flac_rate_code(sample_rate);
    int64_t total = 0;
    const std::vector<FmtSignal> sig = packed_signals(lens, nsig, &total);
    std::vector<int64_t> ls(lens, lens + nsig), offs(nsig);
    for (int i = 0; i < nsig; ++i) offs[i] = sig[i].out_off;
    SBV2_REQUIRE(total == 0 || x, "bad arguments");
    AudioScratch r(device, x, sizeof(int16_t) * (size_t)total, sizeof(int16_t));
    FlacEncoder enc;
    std::vector<int64_t> bytes;
    const int64_t nbytes = enc.encode(r.x.as<int16_t>(), offs, ls, sample_rate, r.s, &bytes);
    SBV2_REQUIRE(capacity >= nbytes, "FLAC buffer too small: " + std::to_string(capacity) + " < " + std::to_string(nbytes) + " bytes");
    HIP_CHECK(hipMemcpyAsync(dst, enc.output(), (size_t)nbytes, hipMemcpyDeviceToHost, r.s));
    HIP_CHECK(hipStreamSynchronize(r.s));
    for (int i = 0; i < nsig; ++i) out_bytes[i] = bytes[i];
    API_END
}

int sbv2_debug_flac_stream_encode(int device, const int16_t* x, int64_t n, const int64_t* cuts, int ncuts, int32_t sample_rate, uint8_t* dst,
                                  int64_t capacity, int64_t* out_bytes_per_push) {
    API_BEGIN
    SBV2_REQUIRE(n >= 0 && ncuts >= 0 && (ncuts == 0 || cuts) && dst && out_bytes_per_push && (n == 0 || x), "bad arguments");
    flac_rate_code(sample_rate);
    // push i = samples [edge[i], edge[i + 1])
    std::vector<int64_t> edge(1, 0);
    for (int i = 0; i < ncuts; ++i) {
        SBV2_REQUIRE(cuts[i] >= edge.back() && cuts[i] <= n, "cuts must ascend within [0, n]");
        edge.push_back(cuts[i]);
    }
    edge.push_back(n);
    const int npush = ncuts + 1;
    int64_t longest = 0;
    for (int i = 0; i < npush; ++i) longest = std::max(longest, edge[i + 1] - edge[i]);
    AudioScratch r(device, x, sizeof(int16_t) * (size_t)n);
    // every push is enqueued before the host waits once: one pinned region per push
    const size_t region = round_up64((int64_t)FlacStreamEncoder::host_bytes(longest), 64);
    PinnedBuffer host;
    char* hb = static_cast<char*>(host.reserve(region * npush, r.s));
    FlacStreamEncoder enc;
    enc.begin(sample_rate, n, longest, r.s);
    std::vector<FlacStreamEncoder::Push> pushes;
    for (int i = 0; i < npush; ++i) {
        const int64_t len = edge[i + 1] - edge[i];
        if (len) HIP_CHECK(hipMemcpyAsync(enc.dst(), r.x.as<int16_t>() + edge[i], sizeof(int16_t) * (size_t)len, hipMemcpyDeviceToDevice, r.s));
        pushes.push_back(enc.push(len, i + 1 == npush, hb + region * i, r.s));
    }
    HIP_CHECK(hipStreamSynchronize(r.s));
    int64_t at = 0;
    for (int i = 0; i < npush; ++i) {
        const FlacStreamEncoder::Push& p = pushes[i];
        const int64_t head = i == 0 ? kFlacStreamHeader : 0, nb = p.size(0, p.frames);
        SBV2_REQUIRE(capacity >= at + head + nb, "FLAC buffer too small: " + std::to_string(capacity) + " < " + std::to_string(at + head + nb) + " bytes");
        if (head) enc.header(dst + at);
        if (nb) std::memcpy(dst + at + head, p.bytes + p.pre[0], (size_t)nb);
        out_bytes_per_push[i] = head + nb;
        at += head + nb;
    }
    API_END
}

int sbv2_debug_loudness(int device, const double* x, const int64_t* lens, int nsig, int32_t sample_rate, const sbv2_loudness* ln, double* stats) {
    API_BEGIN
    SBV2_REQUIRE(nsig >= 1 && lens && stats, "bad arguments");
    const LoudnessSpec spec = loudness_spec(ln);
    double coef[10];
    loudness_kweight(sample_rate, coef);   // refuses unsupported rates
    int64_t total = 0;
    const std::vector<FmtSignal> sig = packed_signals(lens, nsig, &total);
    SBV2_REQUIRE(total == 0 || x, "bad arguments");
    AudioScratch r(device, x, sizeof(double) * (size_t)total);
    LoudnessMeter meter;
    meter.measure(r.x.as<double>(), sig, sample_rate, spec, r.s);
    HIP_CHECK(hipStreamSynchronize(r.s));
    std::memcpy(stats, meter.stats_host(), sizeof(double) * 3 * nsig);
    API_END
}

int sbv2_debug_limiter(int device, const double* x, const int64_t* lens, int nsig, int32_t sample_rate, const sbv2_limiter* lim, double* out_x,
                       double* stats) {
    API_BEGIN
    SBV2_REQUIRE(nsig >= 1 && lens && stats, "bad arguments");
    const LimiterSpec spec = limiter_spec(lim);
    double coef[10];
    loudness_kweight(sample_rate, coef);   // refuses unsupported rates
    int64_t total = 0;
    const std::vector<FmtSignal> sig = packed_signals(lens, nsig, &total);
    SBV2_REQUIRE(total == 0 || (x && out_x), "bad arguments");
    AudioScratch r(device, x, sizeof(double) * (size_t)total);
    LoudnessMeter meter;
    Limiter limiter;
    const double* unit = nullptr;
    const double* lx = limiter.run(r.x.as<double>(), sig, sample_rate, spec, meter, r.s, &unit);
    if (total) HIP_CHECK(hipMemcpyAsync(out_x, lx, sizeof(double) * (size_t)total, hipMemcpyDeviceToHost, r.s));
    HIP_CHECK(hipStreamSynchronize(r.s));
    std::memcpy(stats, limiter.stats_host(), sizeof(double) * 6 * nsig);
    API_END
}

int sbv2_debug_dynamics(int device, const double* x, const int64_t* lens, int nsig, int32_t sample_rate, const sbv2_dynamics* dynamics,
                        double* e_out, int64_t* dq_out, int64_t* u_out, double* s_out, double* y_out, double* stats) {
    API_BEGIN
    SBV2_REQUIRE(nsig >= 1 && lens && stats, "bad arguments");
    const DynamicsSpec spec = dynamics_spec(dynamics);
    double coef[10];
    loudness_kweight(sample_rate, coef);   // refuses unsupported rates
    int64_t total = 0;
    const std::vector<FmtSignal> sig = packed_signals(lens, nsig, &total);
    SBV2_REQUIRE(total == 0 || x, "bad arguments");
    AudioScratch r(device, x, sizeof(double) * (size_t)total);
    LoudnessMeter meter;
    Dynamics dyn;
    dyn.run(r.x.as<double>(), sig, sample_rate, spec, meter, r.s, true);   // (the kernels run also at ratio == 1: d = 0 throughout)
    const Dynamics::Parts& pt = dyn.parts();
    const size_t bytes = sizeof(double) * (size_t)total;
    if (total) {
        if (e_out) HIP_CHECK(hipMemcpyAsync(e_out, pt.e, bytes, hipMemcpyDeviceToHost, r.s));
        if (dq_out) HIP_CHECK(hipMemcpyAsync(dq_out, pt.dq, bytes, hipMemcpyDeviceToHost, r.s));
        if (u_out) HIP_CHECK(hipMemcpyAsync(u_out, pt.u, bytes, hipMemcpyDeviceToHost, r.s));
        if (s_out) HIP_CHECK(hipMemcpyAsync(s_out, pt.s, bytes, hipMemcpyDeviceToHost, r.s));
        if (y_out) HIP_CHECK(hipMemcpyAsync(y_out, pt.yc, bytes, hipMemcpyDeviceToHost, r.s));
    }
    HIP_CHECK(hipStreamSynchronize(r.s));
    std::memcpy(stats, dyn.stats_host(), sizeof(double) * 3 * nsig);
    API_END
}

int sbv2_debug_limiter_fixed(int device, const double* x, const int64_t* lens, int nsig, int32_t sample_rate, const sbv2_stream_level* level,
                             double* out_x, double* stats) {
    API_BEGIN
    SBV2_REQUIRE(nsig >= 1 && lens && stats, "bad arguments");
    const StreamLevelSpec spec = stream_level_spec(level);
    double coef[10];
    loudness_kweight(sample_rate, coef);   // refuses unsupported rates
    int64_t total = 0;
    const std::vector<FmtSignal> sig = packed_signals(lens, nsig, &total);
    SBV2_REQUIRE(total == 0 || (x && out_x), "bad arguments");
    AudioScratch r(device, x, sizeof(double) * (size_t)total);
    Limiter limiter;
    const double* lx = limiter.run_fixed(r.x.as<double>(), sig, sample_rate, spec, r.s);
    if (total) HIP_CHECK(hipMemcpyAsync(out_x, lx, sizeof(double) * (size_t)total, hipMemcpyDeviceToHost, r.s));
    HIP_CHECK(hipStreamSynchronize(r.s));
    std::memcpy(stats, limiter.stats_host(), sizeof(double) * 2 * nsig);
    API_END
}

int sbv2_debug_loudness_parts(int device, const double* x, const int64_t* lens, int nsig, int32_t sample_rate, double* stats, int64_t cap_seg,
                              int64_t cap_blk, double* e, double* st, double* part, double* bmax, double* peak, double* taps, int64_t* counts) {
    API_BEGIN
    SBV2_REQUIRE(nsig >= 1 && lens && stats && e && st && part && bmax && peak && taps && counts, "bad arguments");
    double coef[10];
    loudness_kweight(sample_rate, coef);   // refuses unsupported rates
    int64_t total = 0;
    const std::vector<FmtSignal> sig = packed_signals(lens, nsig, &total);
    SBV2_REQUIRE(total == 0 || x, "bad arguments");
    SBV2_REQUIRE(cap_blk >= (total + 255) / 256, "bmax too small: " + std::to_string(cap_blk) + " < " + std::to_string((total + 255) / 256) + " workgroups");
    PoisonedSignal src(x, total);
    AudioScratch r(device, src.words.data(), sizeof(double) * src.words.size());
    const double* y = r.x.as<double>() + PoisonedSignal::kPad;
    const LoudnessSpec spec;
    LoudnessMeter meter;
    meter.measure(y, sig, sample_rate, spec, r.s);   // places the buffers; the run reported is the next one, at the same places
    const LoudnessMeter::Parts p = meter.parts();
    SBV2_REQUIRE(cap_seg >= p.nseg, "e / st / part too small: " + std::to_string(cap_seg) + " < " + std::to_string(p.nseg) + " segments");
    HIP_CHECK(hipMemsetAsync(const_cast<double*>(p.e), kCtxSentinel, sizeof(double) * (size_t)(p.end - p.e), r.s));
    meter.measure(y, sig, sample_rate, spec, r.s);
    const LoudnessMeter::Parts q = meter.parts();
    SBV2_REQUIRE(q.e == p.e && q.end == p.end && q.nseg == p.nseg && q.nblk == p.nblk, "internal: the meter moved its buffers between two equal runs");
    std::vector<double> h((size_t)(p.end - p.e));
    std::vector<unsigned long long> pk((size_t)nsig);
    HIP_CHECK(hipMemcpyAsync(h.data(), p.e, sizeof(double) * h.size(), hipMemcpyDeviceToHost, r.s));
    HIP_CHECK(hipMemcpyAsync(pk.data(), p.peak, 8 * (size_t)nsig, hipMemcpyDeviceToHost, r.s));
    HIP_CHECK(hipStreamSynchronize(r.s));
    const double *he = h.data(), *hst = he + (p.st - p.e), *hpart = he + (p.part - p.e), *hbmax = he + (p.bmax - p.e), *hend = he + h.size();
    std::memcpy(stats, meter.stats_host(), sizeof(double) * 3 * nsig);
    std::memcpy(e, he, sizeof(double) * 4 * (size_t)p.nseg);
    std::memcpy(st, hst, sizeof(double) * 4 * (size_t)p.nseg);
    std::memcpy(part, hpart, sizeof(double) * (size_t)p.nseg);
    std::memcpy(bmax, hbmax, sizeof(double) * (size_t)p.nblk);
    for (int i = 0; i < nsig; ++i) std::memcpy(peak + i, &pk[i], 8);
    loudness_true_peak_taps(reinterpret_cast<double(*)[kTruePeakTaps]>(taps));
    counts[0] = p.m;
    counts[1] = p.nseg;
    counts[2] = p.nblk;
    counts[3] = sentinel_strays(he + 4 * p.nseg, hst) + sentinel_strays(hst + 4 * p.nseg, hpart) + sentinel_strays(hpart + p.nseg, hbmax) +
                sentinel_strays(hbmax + p.nblk, hend);
    API_END
}

int sbv2_debug_limiter_parts(int device, const double* x, const int64_t* lens, int nsig, int32_t sample_rate, const sbv2_stream_level* level,
                             int64_t cap_tiles, double* out_t, double* out_x, double* smin, double* taps, double* hsum, int64_t* counts) {
    API_BEGIN
    SBV2_REQUIRE(nsig >= 1 && lens && out_t && out_x && smin && taps && hsum && counts, "bad arguments");
    const StreamLevelSpec spec = stream_level_spec(level);
    double coef[10];
    loudness_kweight(sample_rate, coef);   // refuses unsupported rates
    int64_t total = 0;
    const std::vector<FmtSignal> sig = packed_signals(lens, nsig, &total);
    SBV2_REQUIRE(total == 0 || x, "bad arguments");
    int64_t tiles = 0;
    for (int i = 0; i < nsig; ++i) tiles += (lens[i] + 1023) / 1024;
    SBV2_REQUIRE(cap_tiles >= tiles, "smin too small: " + std::to_string(cap_tiles) + " < " + std::to_string(tiles) + " tiles");
    PoisonedSignal src(x, total);
    AudioScratch r(device, src.words.data(), sizeof(double) * src.words.size());
    const double* y = r.x.as<double>() + PoisonedSignal::kPad;
    Limiter limiter;
    limiter.run_fixed(y, sig, sample_rate, spec, r.s);   // places the buffers; the run reported is the next one, at the same places
    const Limiter::Parts p = limiter.parts();
    SBV2_REQUIRE(p.tiles == tiles && p.total == total, "internal: the limiter's tile count");
    HIP_CHECK(hipMemsetAsync(const_cast<double*>(p.t), kCtxSentinel, sizeof(double) * (size_t)(p.end - p.t), r.s));
    limiter.run_fixed(y, sig, sample_rate, spec, r.s);
    const Limiter::Parts q = limiter.parts();
    SBV2_REQUIRE(q.t == p.t && q.end == p.end && q.h == p.h && q.K == p.K, "internal: the limiter moved its buffers between two equal runs");
    std::vector<double> h((size_t)(p.end - p.t)), hh((size_t)p.K);
    HIP_CHECK(hipMemcpyAsync(h.data(), p.t, sizeof(double) * h.size(), hipMemcpyDeviceToHost, r.s));
    HIP_CHECK(hipMemcpyAsync(hh.data(), p.h, sizeof(double) * hh.size(), hipMemcpyDeviceToHost, r.s));
    HIP_CHECK(hipStreamSynchronize(r.s));
    const double *ht = h.data(), *hx = ht + (p.x - p.t), *hsm = ht + (p.smin - p.t), *hend = ht + h.size();
    std::memcpy(out_t, ht, sizeof(double) * (size_t)total);
    std::memcpy(out_x, hx, sizeof(double) * (size_t)total);
    std::memcpy(smin, hsm, sizeof(double) * (size_t)tiles);
    std::memcpy(taps, hh.data(), sizeof(double) * hh.size());
    *hsum = q.hsum;
    counts[0] = p.K;
    counts[1] = tiles;
    counts[2] = sentinel_strays(ht + total, hx) + sentinel_strays(hx + total, hsm) + sentinel_strays(hsm + tiles, hend);
    API_END
}

int sbv2_debug_limiter_stream(int device, const double* x, int64_t n, const int64_t* cuts, int ncuts, int32_t sample_rate,
                              const sbv2_stream_level* level, double* out_x, int64_t* out_per_push, double* stats) {
    API_BEGIN
    SBV2_REQUIRE(n >= 0 && ncuts >= 0 && (ncuts == 0 || cuts) && out_per_push && stats && (n == 0 || (x && out_x)), "bad arguments");
    const StreamLevelSpec spec = stream_level_spec(level);
    double coef[10];
    loudness_kweight(sample_rate, coef);   // refuses unsupported rates
    // push i = samples [edge[i], edge[i + 1])
    std::vector<int64_t> edge(1, 0);
    for (int i = 0; i < ncuts; ++i) {
        SBV2_REQUIRE(cuts[i] >= edge.back() && cuts[i] <= n, "cuts must ascend within [0, n]");
        edge.push_back(cuts[i]);
    }
    edge.push_back(n);
    const int npush = ncuts + 1;
    int64_t longest = 0;
    for (int i = 0; i < npush; ++i) longest = std::max(longest, edge[i + 1] - edge[i]);
    AudioScratch r(device, x, sizeof(double) * (size_t)n);
    DeviceBuffer out;   // every push is enqueued before the host waits once: the pushes' samples back to back
    out.reserve(sizeof(double) * (size_t)std::max<int64_t>(n, 1), r.s);
    StreamLimiter lim;
    lim.begin(sample_rate, n, longest, spec, r.s);
    int64_t at = 0;
    for (int i = 0; i < npush; ++i) {
        const int64_t len = edge[i + 1] - edge[i];
        if (len) HIP_CHECK(hipMemcpyAsync(lim.dst(), r.x.as<double>() + edge[i], sizeof(double) * (size_t)len, hipMemcpyDeviceToDevice, r.s));
        out_per_push[i] = lim.push(len, i + 1 == npush, out.as<double>() + at, r.s);
        at += out_per_push[i];
    }
    SBV2_REQUIRE(at == n, "internal: the fed limiter emitted " + std::to_string(at) + " of " + std::to_string(n) + " samples");
    if (n) HIP_CHECK(hipMemcpyAsync(out_x, out.get(), sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, r.s));
    HIP_CHECK(hipStreamSynchronize(r.s));
    lim.stats(stats);
    API_END
}

// The fed leveler with the stream limiter behind it, as StreamOutput::push runs them: every push's samples are copied behind the limiter's
// carried tail, scaled there in place, then pushed.  The input lies between NaN words on the device.
int sbv2_debug_leveler_stream(int device, const double* x, int64_t n, const int64_t* cuts, int ncuts, int32_t sample_rate,
                              const sbv2_stream_level* level, const sbv2_stream_leveler* leveler, double* out_x, int64_t* out_per_push,
                              double* out_gain_db, int64_t gain_capacity, double* stats) {
    API_BEGIN
    SBV2_REQUIRE(n >= 0 && ncuts >= 0 && (ncuts == 0 || cuts) && out_per_push && out_gain_db && stats && (n == 0 || (x && out_x)), "bad arguments");
    const StreamLevelSpec spec = stream_level_spec(level);
    const StreamLevelerSpec lspec = stream_leveler_spec(leveler);
    double coef[10];
    loudness_kweight(sample_rate, coef);   // refuses unsupported rates
    const int64_t ngain = n / (sample_rate / 10) + 1;
    SBV2_REQUIRE(gain_capacity >= ngain, "out_gain_db too small: " + std::to_string(gain_capacity) + " < " + std::to_string(ngain) + " gains");
    std::vector<int64_t> edge(1, 0);   // push i = samples [edge[i], edge[i + 1])
    for (int i = 0; i < ncuts; ++i) {
        SBV2_REQUIRE(cuts[i] >= edge.back() && cuts[i] <= n, "cuts must ascend within [0, n]");
        edge.push_back(cuts[i]);
    }
    edge.push_back(n);
    const int npush = ncuts + 1;
    int64_t longest = 0;
    for (int i = 0; i < npush; ++i) longest = std::max(longest, edge[i + 1] - edge[i]);
    PoisonedSignal src(x, n);
    AudioScratch r(device, src.words.data(), sizeof(double) * src.words.size());
    const double* y = r.x.as<double>() + PoisonedSignal::kPad;
    DeviceBuffer out;   // every push is enqueued before the host waits once: the pushes' samples back to back
    out.reserve(sizeof(double) * (size_t)std::max<int64_t>(n, 1), r.s);
    StreamLevelSpec unity = spec;
    unity.gain_db = 0.0;
    StreamLimiter lim;
    StreamLeveler lev;
    lim.begin(sample_rate, n, longest, unity, r.s);
    lev.begin(sample_rate, n, longest, lspec, spec.gain_db, r.s);
    int64_t at = 0;
    for (int i = 0; i < npush; ++i) {
        const int64_t len = edge[i + 1] - edge[i];
        if (len) HIP_CHECK(hipMemcpyAsync(lim.dst(), y + edge[i], sizeof(double) * (size_t)len, hipMemcpyDeviceToDevice, r.s));
        lev.push(lim.dst(), len, i + 1 == npush, r.s);
        out_per_push[i] = lim.push(len, i + 1 == npush, out.as<double>() + at, r.s);
        at += out_per_push[i];
    }
    SBV2_REQUIRE(at == n, "internal: the fed limiter emitted " + std::to_string(at) + " of " + std::to_string(n) + " samples");
    if (n) HIP_CHECK(hipMemcpyAsync(out_x, out.get(), sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, r.s));
    HIP_CHECK(hipMemcpyAsync(out_gain_db, lev.gains_dev(), sizeof(double) * (size_t)ngain, hipMemcpyDeviceToHost, r.s));
    HIP_CHECK(hipStreamSynchronize(r.s));
    lev.stats(stats);
    lim.stats(stats + 4);
    API_END
}

int sbv2_debug_bucket_table(int64_t max_s, int64_t buckets, int64_t max_rel, int32_t* out) {
    API_BEGIN
    SBV2_REQUIRE(max_s >= 1 && out, "bad arguments");
    const std::vector<int> t = BertModel::bucket_table((int)max_s, (int)buckets, (int)max_rel);
    for (size_t i = 0; i < t.size(); ++i) out[i] = t[i];
    API_END
}

int sbv2_debug_conv1d(int device, const float* x, const float* w, const float* bias, int64_t cin, int64_t cout, int64_t k, int64_t L,
                      int64_t dilation, float pre_slope, float* y) {
    API_BEGIN
    HIP_CHECK(hipSetDevice(device));
    Blob b = one_conv_blob(w, bias, {cout, cin, k}, cout);
    WeightStore ws(b);
    PackedConv pc = ws.conv("c");
    Plane X{nullptr, (int)cin, (int)L, round_up((int)L, 64)}, Y{nullptr, (int)cout, (int)L, round_up((int)L, 64)};
    DevMem dx(sizeof(float) * cin * X.ld), dy(sizeof(float) * cout * Y.ld);
    X.p = dx.f();
    Y.p = dy.f();
    HIP_CHECK(hipMemcpy2D(X.p, sizeof(float) * X.ld, x, sizeof(float) * L, sizeof(float) * L, cin, hipMemcpyHostToDevice));
    conv_plain(pc, X, Y, (int)dilation, (int)(dilation * (k - 1) / 2), nullptr, 1, nullptr, ACT_NONE, pre_slope);
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy2D(y, sizeof(float) * L, Y.p, sizeof(float) * Y.ld, sizeof(float) * L, cout, hipMemcpyDeviceToHost));
    API_END
}

// ---- conv_plain / the encoders' FFN pair / linear_tokmajor with every argument the models pass (tests/test_gemm_conv_kernels.py): planes at the library's
// pitch, NaN behind L in every input, outputs pre-filled with the sentinel (or the caller's previous contents under `accumulate`, NaN behind L), *stray =
// the pad words of the outputs that the launch changed
int sbv2_debug_conv_plain(int device, const float* x, const float* w, const float* bias, int64_t cin, int64_t cout, int64_t k, int64_t L, int64_t dilation,
                          int64_t pad_l, int cl_parts, const uint8_t* mask, int64_t mask_div, int act, float pre_slope, const float* res, float alpha,
                          float beta, int accumulate, float* y_inout, int64_t* stray) {
    API_BEGIN
    HIP_CHECK(hipSetDevice(device));
    SBV2_REQUIRE(x && w && y_inout && cin >= 1 && cout >= 1 && k >= 1 && k <= kMaxTaps && dilation >= 1 && pad_l >= 0 && cl_parts >= 0 && cl_parts <= 3 &&
                     mask_div >= 1 && act >= ACT_NONE && act <= ACT_TANH,
                 "bad arguments");
    Blob b = one_conv_blob(w, bias, {cout, cin, k}, cout);
    WeightStore ws(b, cl_parts);
    PackedConv pc = ws.conv("c");
    DevPlane X(cin, L), Y(cout, L), R(res ? cout : 1, res ? L : 1);
    X.put(x, true);
    if (res) R.put(res, true);
    if (accumulate) Y.put(y_inout, true);
    else Y.fill(true);
    DevMem dm(mask, mask ? (size_t)((L + mask_div - 1) / mask_div) : 0);
    conv_plain(pc, X.P, Y.P, (int)dilation, (int)pad_l, mask ? dm.u8() : nullptr, (int)mask_div, nullptr, act, pre_slope, res ? &R.P : nullptr, alpha, beta,
               accumulate);
    HIP_CHECK(hipDeviceSynchronize());
    const int64_t bad = Y.get(y_inout, accumulate ? kNanWord : kSentinelWord);
    if (stray) *stray = bad;
    API_END
}

int sbv2_debug_conv_ffn_cl(int device, const float* x, const float* w1, const float* b1, const float* w2, const float* b2, int64_t H, int64_t F, int64_t k,
                           int64_t L, const uint8_t* mask, const float* res, float* y, float* mid, int64_t* stray) {
    API_BEGIN
    HIP_CHECK(hipSetDevice(device));
    SBV2_REQUIRE(x && w1 && w2 && y && mid && H >= 1 && F >= 1 && k >= 1 && k <= kMaxTaps && (k & 1) && L >= 1, "bad arguments");
    Blob bl1 = one_conv_blob(w1, b1, {F, H, k}, F), bl2 = one_conv_blob(w2, b2, {H, F, k}, H);
    WeightStore ws1(bl1, 2), ws2(bl2, 2);   // split-bf16 fragments, as the flow's encoder loads its FFN
    PackedConv c1 = ws1.conv("c"), c2 = ws2.conv("c");
    DevPlane X(H, L), Y(H, L), R(res ? H : 1, res ? L : 1);
    X.put(x, true);
    if (res) R.put(res, true);
    Y.fill(true);
    // the channels-last intermediate [L][F] (pitch F, as VitsModel::run_encoder allocates it) with guard words behind it
    constexpr int64_t kGuard = 256;
    const size_t nmid = (size_t)L * F;
    DevMem dmid(sizeof(float) * (nmid + kGuard)), dm(mask, mask ? (size_t)L : 0);
    HIP_CHECK(hipMemset(dmid.p, kCtxSentinel, sizeof(float) * (nmid + kGuard)));
    const unsigned char* m = mask ? dm.u8() : nullptr;
    SBV2_REQUIRE(conv_km_to_cl(c1, X.P, dmid.f(), (int)F, 1, (int)(k - 1) / 2, m, 1, nullptr),
                 "conv_km_to_cl refused the shape (k >= 3 and a multiple of 16 output channels)");
    SBV2_REQUIRE(conv_cl_to_km(c2, dmid.f(), (int)F, Y.P, 1, (int)(k - 1) / 2, m, 1, nullptr, 0.0f, res ? &R.P : nullptr),
                 "conv_cl_to_km refused the shape (k >= 3 and a multiple of 16 input channels)");
    HIP_CHECK(hipDeviceSynchronize());
    int64_t bad = Y.get(y, kSentinelWord);
    std::vector<uint32_t> h(nmid + kGuard);
    HIP_CHECK(hipMemcpy(h.data(), dmid.p, 4 * h.size(), hipMemcpyDeviceToHost));
    for (size_t e = nmid; e < nmid + kGuard; ++e) bad += h[e] != kSentinelWord;
    for (int64_t c = 0; c < F; ++c)   // returned channel-major [F][L] like every other plane of the hooks
        for (int64_t n = 0; n < L; ++n) std::memcpy(&mid[(size_t)c * L + n], &h[(size_t)n * F + c], 4);
    if (stray) *stray = bad;
    API_END
}

int sbv2_debug_linear_tokmajor(int device, const float* x, const float* w, const float* bias, int64_t cin, int64_t cout, int64_t L, int64_t ldy, float* y,
                               int64_t* stray) {
    API_BEGIN
    HIP_CHECK(hipSetDevice(device));
    SBV2_REQUIRE(x && w && y && cin >= 1 && cout >= 1 && L >= 1 && ldy >= cout && ldy < (1 << 20), "bad arguments");
    Blob b = one_conv_blob(w, bias, {cout, cin, 1}, cout);
    WeightStore ws(b);
    PackedConv pc = ws.conv("c");
    DevPlane X(cin, L);
    X.put(x, true);
    // y [L][ldy] token-major: columns cout .. ldy of every row and the guard words behind the last row must keep the sentinel
    constexpr int64_t kGuard = 256;
    const size_t ny = (size_t)L * ldy;
    DevMem dy(sizeof(float) * (ny + kGuard));
    HIP_CHECK(hipMemset(dy.p, kCtxSentinel, sizeof(float) * (ny + kGuard)));
    linear_tokmajor(pc, X.P, dy.f(), (int)ldy, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    std::vector<uint32_t> h(ny + kGuard);
    HIP_CHECK(hipMemcpy(h.data(), dy.p, 4 * h.size(), hipMemcpyDeviceToHost));
    int64_t bad = 0;
    for (int64_t n = 0; n < L; ++n) {
        std::memcpy(y + (size_t)n * cout, &h[(size_t)n * ldy], 4 * (size_t)cout);
        for (int64_t c = cout; c < ldy; ++c) bad += h[(size_t)n * ldy + c] != kSentinelWord;
    }
    for (size_t e = ny; e < ny + kGuard; ++e) bad += h[e] != kSentinelWord;
    if (stray) *stray = bad;
    API_END
}

int sbv2_debug_conv_transpose1d(int device, const float* x, const float* w, const float* bias, int64_t cin, int64_t cout, int64_t k,
                                int64_t L, int64_t stride, int64_t padding, float pre_slope, float* y) {
    API_BEGIN
    HIP_CHECK(hipSetDevice(device));
    SBV2_REQUIRE(bias, "bias required");
    Blob b = one_conv_blob(w, bias, {cin, cout, k}, cout);
    WeightStore ws(b);
    PackedUpsample up = ws.upsample("c", (int)stride, (int)padding);
    const int Lo = (int)(L * stride);
    Plane X{nullptr, (int)cin, (int)L, round_up((int)L, 64)}, Y{nullptr, (int)cout, Lo, round_up(Lo, 64)};
    DevMem dx(sizeof(float) * cin * X.ld), dy(sizeof(float) * cout * Y.ld);
    X.p = dx.f();
    Y.p = dy.f();
    HIP_CHECK(hipMemcpy2D(X.p, sizeof(float) * X.ld, x, sizeof(float) * L, sizeof(float) * L, cin, hipMemcpyHostToDevice));
    for (const auto& g : up.groups) {
        ConvParams p;
        p.A = g.w;
        p.lda = g.lda;
        p.a_tap_stride = (int64_t)up.cin * g.lda;
        p.B = X.p;
        p.ldb = X.ld;
        p.nb = X.L;
        p.C = Y.p;
        p.ldc = Y.ld;
        p.M = g.nph * up.cout;
        p.N = X.L;
        p.K = up.cin;
        p.ntaps = g.ntaps;
        for (int t = 0; t < g.ntaps; ++t) p.shift[t] = g.shift[t];
        p.bias = up.bias;
        p.bias_mode = BIAS_ROW;
        p.pre_slope = pre_slope;
        p.out_stride = (int)stride;
        p.phase_rows = up.cout;
        for (int q = 0; q < kMaxPhases; ++q) p.phase_off[q] = g.phase_off[q];
        launch_conv(p, nullptr);
    }
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy2D(y, sizeof(float) * Lo, Y.p, sizeof(float) * Y.ld, sizeof(float) * Lo, cout, hipMemcpyDeviceToHost));
    API_END
}

int sbv2_debug_set_upx(int on) { return set_upx(on); }
int sbv2_debug_conv_transpose1d_clx(int device, const float* x, const float* w, const float* bias, int64_t cin, int64_t cout, int64_t k, int64_t L,
                                    int64_t stride, float pre_slope, const uint8_t* mask, int64_t mask_div, int64_t iters, float* y, float* ys_sum, float* ms) {
    API_BEGIN
    HIP_CHECK(hipSetDevice(device));
    SBV2_REQUIRE(x && w && bias && y && mask_div >= 1 && (mask_div & (mask_div - 1)) == 0, "bad arguments");
    Blob b = one_conv_blob(w, bias, {cin, cout, k}, cout);
    WeightStore ws(b);
    ClUpX u = build_upx(ws, w, bias, (int)cin, (int)cout, (int)k, (int)stride, /*parts_out=*/ys_sum != nullptr);
    SBV2_REQUIRE(u.wx, "shape not supported by the phased conv_clx transposed convolution");
    const int64_t Lo = L * stride;
    DevMem dx = upload_cl(x, cin, L), dy(sizeof(float) * Lo * cout);
    HIP_CHECK(hipMemset(dy.p, 0xFF, sizeof(float) * Lo * cout));   // (NaN: every output row must be written)
    DevMem dxs(split_cl_bytes((int)cin, L) + 16), dys(split_cl_bytes((int)cout, Lo) + 16);
    SplitClPlanes xs = make_split_cl(dxs.p, (int)cin, L, nullptr), ysp = make_split_cl(dys.p, (int)cout, Lo, nullptr);
    split_cl(dx.f(), (int)cin, L, (int)cin, pre_slope, xs, nullptr);
    DevMem dm(mask, mask ? (size_t)((L + mask_div - 1) / mask_div) : 0);
    int shift = 0;
    while ((1 << shift) < mask_div) ++shift;
    ConvClxParams p;
    p.X = xs;
    p.W = u.wx;
    p.nmt = u.M / 32;
    p.M = u.M;
    p.N = (int)L;
    p.K = (int)cin;
    p.ntaps = u.ntaps;
    p.shift0 = u.shift0;
    p.shift_step = -1;
    p.Y = dy.f();
    p.ldy = (int)cout;
    if (ys_sum) {
        p.Ys = ysp;
        p.ys_slope = 0.1f;
    }
    p.bias = u.bias;
    p.mask = mask ? dm.u8() : nullptr;   // indexed by the INPUT position >> shift
    p.mask_shift = shift;
    p.out_stride = (int)stride;
    p.phase_rows = (int)cout;
    p.phase_group = u.group;
    for (int q = 0; q < kMaxPhases; ++q) {
        p.phase_off[q] = u.phase_off[q];
        p.phase_tap0[q] = u.phase_tap0[q];
    }
    SBV2_REQUIRE(conv_clx_usable(p), "shape not supported by conv_clx");
    launch_conv_clx(p, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    if (iters > 0 && ms) *ms = time_ms(iters, [&] { launch_conv_clx(p, nullptr); });
    download_cl(dy.f(), cout, Lo, y);
    if (ys_sum) read_parts(ysp, ys_sum);
    API_END
}

int sbv2_debug_conv1d_cl(int device, const float* x, const float* w, const float* bias, int64_t cin, int64_t cout, int64_t k, int64_t L,
                         int64_t dilation, float pre_slope, int mode, int64_t iters, float* y, float* ms) {
    API_BEGIN
    HIP_CHECK(hipSetDevice(device));
    SBV2_REQUIRE(mode >= 1 && mode <= 3, "mode: 1 = split-bf16, 2 = bf16, 3 = f16");
    Blob b = one_conv_blob(w, bias, {cout, cin, k}, cout);
    WeightStore ws(b);
    ClConv c = pack_decoder_conv(ws, w, (int)cout, (int)cin, (int)k, mode, bias);
    DevMem dx = upload_cl(x, cin, L), dy(sizeof(float) * L * cout);
    const ConvClParams p = conv_cl_params(c, dx.f(), (int)cin, (int)L, dy.f(), (int)cout, (int)L, (int)dilation, (int)(dilation * (k - 1) / 2), nullptr, 1,
                                          pre_slope, nullptr, 0, 1.0f, 0);
    launch_conv_cl(p, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    if (iters > 0 && ms) *ms = time_ms(iters, [&] { launch_conv_cl(p, nullptr); });
    download_cl(dy.f(), cout, L, y);
    API_END
}

int sbv2_debug_set_skinny_max(int workgroups) { return set_skinny_max(workgroups); }
int sbv2_debug_set_clx(int on) { return set_clx(on); }
int sbv2_debug_set_ksplit(int on) { return set_ksplit(on); }
int sbv2_debug_set_flash_parts(int on) { return set_flash_parts(on); }
int sbv2_debug_set_sdp_all(int on) { return set_sdp_all(on); }

int sbv2_debug_conv1d_clx(int device, const float* x, const float* w, const float* bias, const float* res, int64_t cin, int64_t cout, int64_t k,
                          int64_t L, int64_t dilation, float pre_slope, float beta, int64_t iters, float* y, float* ys_sum, float* ms) {
    API_BEGIN
    HIP_CHECK(hipSetDevice(device));
    SBV2_REQUIRE(x && w && y, "bad arguments");
    Blob b = one_conv_blob(w, bias, {cout, cin, k}, cout);
    WeightStore ws(b);
    ClConv c = pack_decoder_conv(ws, w, (int)cout, (int)cin, (int)k, 1, bias);
    DevMem dx = upload_cl(x, cin, L), dy(sizeof(float) * L * cout), dr = res ? upload_cl(res, cout, L) : DevMem(0);
    DevMem dxs(split_cl_bytes((int)cin, L) + 16), dys(split_cl_bytes((int)cout, L) + 16);
    SplitClPlanes xs = make_split_cl(dxs.p, (int)cin, L, nullptr), ysp = make_split_cl(dys.p, (int)cout, L, nullptr);
    split_cl(dx.f(), (int)cin, L, (int)cin, pre_slope, xs, nullptr);
    ConvClxParams p;
    p.X = xs;
    p.W = c.wx;
    p.nmt = c.nmt;
    p.M = (int)cout;
    p.N = (int)L;
    p.K = (int)cin;
    p.ntaps = (int)k;
    p.shift0 = (int)(-dilation * (k - 1) / 2);
    p.shift_step = (int)dilation;
    p.Y = dy.f();
    p.ldy = (int)cout;
    if (ys_sum) {
        p.Ys = ysp;
        p.ys_slope = 0.1f;
    }
    p.bias = c.bias;
    if (res) {
        p.R = dr.f();
        p.ldr = (int)cout;
    }
    p.beta = beta;
    SBV2_REQUIRE(conv_clx_usable(p), "shape not supported by conv_clx");
    launch_conv_clx(p, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    if (iters > 0 && ms) *ms = time_ms(iters, [&] { launch_conv_clx(p, nullptr); });
    download_cl(dy.f(), cout, L, y);
    if (ys_sum) read_parts(ysp, ys_sum);
    API_END
}

int sbv2_debug_f16x3_saturation(int device, int enable, uint64_t* count) {
    API_BEGIN
    HIP_CHECK(hipSetDevice(device));
    if (enable >= 0) f16x3_sat_enable(enable);
    if (count) *count = f16x3_sat_read(true);
    API_END
}

int sbv2_debug_set_respair_clx(int on) { return set_respair_clx(on); }

int sbv2_debug_respair(int device, const float* x, const float* w1, const float* w2, const float* b1, const float* b2, int64_t C, int64_t N, int64_t k,
                       int64_t dilation, const uint8_t* mask, int64_t mask_div, float beta, int accumulate, int variant, float* y) {
    API_BEGIN
    HIP_CHECK(hipSetDevice(device));
    SBV2_REQUIRE(x && w1 && w2 && b1 && b2 && y && (C == 16 || C == 32 || C == 64) && N >= 1 && k >= 1 && k <= kMaxTaps && (k & 1) && mask_div >= 1 &&
                     (mask_div & (mask_div - 1)) == 0, "bad arguments");
    Blob b = one_conv_blob(w1, b1, {C, C, k}, C);
    WeightStore ws(b);
    ClConv c1 = pack_decoder_conv(ws, w1, (int)C, (int)C, (int)k, 1, b1);
    ClConv c2 = pack_decoder_conv(ws, w2, (int)C, (int)C, (int)k, 1, b2);
    DevMem dx(x, sizeof(float) * N * C), dy(y, sizeof(float) * N * C);   // (the previous contents of y matter when accumulate is set)
    DevMem dm(mask, mask ? (size_t)((N + mask_div - 1) / mask_div) : 0);
    int shift = 0;
    while ((1 << shift) < mask_div) ++shift;
    ResPairParams rp = step_params(c1, c2, (int)k, (int)dilation, 1, (int)C, N, mask ? dm.u8() : nullptr, (int)mask_div, shift);
    rp.X = dx.f();
    rp.Y = dy.f();
    rp.beta = beta;
    rp.accumulate = accumulate;
    // 0 = respair_cl, 1 = the default dispatch's kernel, 2 = respair_clx
    launch_respair(rp, variant == 0 ? BranchKernel::respair_cl : (variant == 2 ? BranchKernel::respair_clx : respair_default(rp)), nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(y, dy.p, sizeof(float) * N * C, hipMemcpyDeviceToHost));
    API_END
}

// ys (variant 3 only, may be null): hi + lo of the bf16 parts of lrelu(y, 0.1) the last launch writes, [N][C] as y
// y_steps, ys_steps (variant 3 only, may be null): [2][N][C], the planes the first two steps' conv2 launches wrote, and hi + lo of the parts they wrote
static int debug_resbranch_impl(int device, const float* x, const float* w, const float* bias, int64_t C, int64_t N, int64_t k, const int64_t* dilations,
                                const uint8_t* mask, int64_t mask_div, float beta, int accumulate, int variant, int64_t iters, float* y, float* ms, float* ys,
                                float* y_steps, float* ys_steps) {
    API_BEGIN
    HIP_CHECK(hipSetDevice(device));
    SBV2_REQUIRE(x && w && bias && y && dilations && (C == 16 || C == 32 || C == 64 || C == 128 || C == 256) && N >= 1 && k >= 1 && k <= kMaxTaps && (k & 1) &&
                     mask_div >= 1 && (mask_div & (mask_div - 1)) == 0 && variant >= 0 && variant <= 3,
                 "bad arguments");
    SBV2_REQUIRE(variant != 0 || C <= 64, "the fused step exists for C <= 64 (variant 2 = the two-launch conv_cl path at any C)");
    SBV2_REQUIRE(variant != 3 || C >= 128, "the conv_clx step chain is the path of the >= 128-channel stages");
    SBV2_REQUIRE(variant == 3 || (!ys && !y_steps && !ys_steps), "only the conv_clx step chain returns parts and its steps' planes");
    const size_t wsz = (size_t)C * C * k;
    Blob b = one_conv_blob(w, bias, {C, C, k}, C);
    WeightStore ws(b);
    std::vector<ClConv> c1, c2;   // conv1 / conv2 of each step
    std::vector<int> dil;
    for (int q = 0; q < kResBranchSteps; ++q) {
        c1.push_back(pack_decoder_conv(ws, w + 2 * q * wsz, (int)C, (int)C, (int)k, 1, bias + (size_t)2 * q * C));
        c2.push_back(pack_decoder_conv(ws, w + (2 * q + 1) * wsz, (int)C, (int)C, (int)k, 1, bias + (size_t)(2 * q + 1) * C));
        dil.push_back((int)dilations[q]);
    }
    const size_t bytes = sizeof(float) * N * C;
    DevMem dx(x, bytes), dy(y, bytes), da(bytes), db(bytes), dt(bytes);   // (the previous contents of y matter when accumulate is set)
    DevMem dm(mask, mask ? (size_t)((N + mask_div - 1) / mask_div) : 0);
    const unsigned char* m = mask ? dm.u8() : nullptr;
    int shift = 0;
    while ((1 << shift) < mask_div) ++shift;
    // 3 = six launches of conv_clx.hip as run_decoder_cl's clx_steps arm makes them: the input's parts by one split_cl pass, conv1 writes parts only, conv2
    // reads them and adds the residual plane; the parts of the last result (ys) as the stage's last branch writes them for the next transposed convolution
    const size_t sb = variant == 3 ? split_cl_bytes((int)C, N) + 16 : 0;
    DevMem mxu(sb), mt1(sb), mya(sb), myb(sb), mys(ys ? sb : 0);
    SplitClPlanes XUs, T1s, YsA, YsB, YSs;
    if (variant == 3) {
        for (int q = 0; q < kResBranchSteps; ++q) SBV2_REQUIRE(c1[q].wx && c2[q].wx, "shape not supported by conv_clx");
        XUs = make_split_cl(mxu.p, (int)C, N, nullptr);
        T1s = make_split_cl(mt1.p, (int)C, N, nullptr);
        YsA = make_split_cl(mya.p, (int)C, N, nullptr);
        YsB = make_split_cl(myb.p, (int)C, N, nullptr);
        if (ys) YSs = make_split_cl(mys.p, (int)C, N, nullptr);
        split_cl(dx.f(), (int)C, N, (int)C, 0.1f, XUs, nullptr);
    }
    auto run = [&]() {
        if (variant == 3) {
            const float* cur = dx.f();
            const SplitClPlanes* cs = &XUs;   // bf16 parts of lrelu(cur)
            for (int q = 0; q < kResBranchSteps; ++q) {
                const bool last = q + 1 == kResBranchSteps;
                float* yn = last ? dy.f() : (q & 1 ? db.f() : da.f());
                const SplitClPlanes* yns = (cs == &YsA) ? &YsB : &YsA;
                launch_conv_clx(clx_conv1_params(c1[q], *cs, T1s, (int)C, N, (int)k, dil[q], m, shift), nullptr);
                launch_conv_clx(clx_conv2_params(c2[q], T1s, (int)C, N, (int)k, cur, yn, !last ? yns : (ys ? &YSs : nullptr), last ? beta : 1.0f,
                                                 last ? accumulate : 0, m, shift),
                                nullptr);
                cs = yns;
                cur = yn;
            }
            return;
        }
        if (variant == 1) {     // 1 = the fused branch (resbranch_clx.hip)
            ResBranchParams rb = branch_params(c1, c2, dil, (int)k, (int)C, N, m, shift);
            rb.X = dx.f();
            rb.Y = dy.f();
            rb.beta = beta;
            rb.accumulate = accumulate;
            launch_resbranch(rb, nullptr);
            return;
        }
        // 0 = three launches of the fused step (respair_clx.hip), 2 = six launches of conv_cl.hip (conv1 -> T, conv2 + residual): the unfused path, any C
        const float* cur = dx.f();
        for (int q = 0; q < kResBranchSteps; ++q) {
            const bool last = q + 1 == kResBranchSteps;
            float* yn = last ? dy.f() : (q & 1 ? db.f() : da.f());
            if (variant == 2) {
                launch_conv_cl(conv_cl_params(c1[q], cur, (int)C, (int)N, dt.f(), (int)C, (int)N, dil[q], dil[q] * (int)(k - 1) / 2, m, (int)mask_div, 0.1f,
                                              nullptr, (int)C, 1.0f, 0),
                               nullptr);
                launch_conv_cl(conv_cl_params(c2[q], dt.f(), (int)C, (int)N, yn, (int)C, (int)N, 1, (int)(k - 1) / 2, m, (int)mask_div, 0.1f, cur, (int)C,
                                              last ? beta : 1.0f, last ? accumulate : 0),
                               nullptr);
            } else {
                ResPairParams rp = step_params(c1[q], c2[q], (int)k, dil[q], 1, (int)C, N, m, (int)mask_div, shift);
                rp.X = cur;
                rp.Y = yn;
                rp.beta = last ? beta : 1.0f;
                rp.accumulate = last ? accumulate : 0;
                launch_respair(rp, respair_default(rp), nullptr);
            }
            cur = yn;
        }
    };
    run();
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(y, dy.p, bytes, hipMemcpyDeviceToHost));
    auto parts_cl = [&](const SplitClPlanes& s, float* out) {   // hi + lo of a parts plane, channels-last
        std::vector<float> t((size_t)N * C);
        read_parts(s, t.data());
        for (int64_t c = 0; c < C; ++c)
            for (int64_t n = 0; n < N; ++n) out[(size_t)n * C + c] = t[(size_t)c * N + n];
    };
    if (ys) parts_cl(YSs, ys);
    if (y_steps) {    // (step 0 wrote da and YsA, step 1 db and YsB)
        HIP_CHECK(hipMemcpy(y_steps, da.p, bytes, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(y_steps + (size_t)N * C, db.p, bytes, hipMemcpyDeviceToHost));
    }
    if (ys_steps) {
        parts_cl(YsA, ys_steps);
        parts_cl(YsB, ys_steps + (size_t)N * C);
    }
    if (iters > 0 && ms) *ms = time_ms(iters, run);
    API_END
}
int sbv2_debug_resbranch(int device, const float* x, const float* w, const float* bias, int64_t C, int64_t N, int64_t k, const int64_t* dilations,
                         const uint8_t* mask, int64_t mask_div, float beta, int accumulate, int variant, int64_t iters, float* y, float* ms) {
    return debug_resbranch_impl(device, x, w, bias, C, N, k, dilations, mask, mask_div, beta, accumulate, variant, iters, y, ms, nullptr, nullptr, nullptr);
}
int sbv2_debug_resbranch_ys(int device, const float* x, const float* w, const float* bias, int64_t C, int64_t N, int64_t k, const int64_t* dilations,
                            const uint8_t* mask, int64_t mask_div, float beta, int accumulate, int64_t iters, float* y, float* ys, float* y_steps, float* ys_steps,
                            float* ms) {
    return debug_resbranch_impl(device, x, w, bias, C, N, k, dilations, mask, mask_div, beta, accumulate, 3, iters, y, ms, ys, y_steps, ys_steps);
}
int sbv2_debug_set_resbranch(int on) { return set_resbranch(on); }

// x2 / y2 (sbv2_debug_gemm_bfs_alt): a second input; the launches alternate between the two on ONE scratch buffer that is never cleared in between, so a
// workgroup that read a stale partial sum (the other input's, left in its XCD's L2 by the previous launch) would show up in the result
// ex (sbv2_debug_gemm_bfs_ex): the rest of conv_bfs' arguments, and the poison / sentinel / stray-count convention of the ops.h hooks: x and res hold NaN
// in the columns N .. pitch (so do x's parts: split_planes converts the whole pitch), the f32 plane and the parts planes are pre-filled with the sentinel,
// y returns the f32 plane and ys the recombined parts separately, *stray = the pad words of either (columns N .. pitch, and one guard row behind row M
// of the plane and of every part) that the launch changed.
struct BfsHookEx {
    const uint8_t* mask = nullptr;
    int64_t mask_div = 1;
    float alpha = 1.0f, beta = 1.0f;
    int64_t y_rows = -1, ys_row0 = 0;
    int want_y = 1;
    float* ys = nullptr;
    int64_t* stray = nullptr;
};
static int debug_gemm_bfs_impl(int device, const float* x, const float* x2, const float* w, const float* bias, const float* res, int64_t M, int64_t N, int64_t K,
                               int parts, int act, int split_out, int64_t iters, float* y, float* y2, float* ms, const BfsHookEx* ex = nullptr) {
    API_BEGIN
    HIP_CHECK(hipSetDevice(device));
    SBV2_REQUIRE((parts == 2 || parts == 3 || parts == kPartsF16x3) && x && w && y && M >= 1 && N >= 4 && (N & 3) == 0 && (K & 15) == 0, "bad arguments");
    SBV2_REQUIRE(!ex || ((ex->want_y || split_out) && (!split_out || ex->ys) && ex->mask_div >= 1 && ex->y_rows >= -1 && ex->ys_row0 >= 0 && !x2), "bad arguments");
    const bool poison = ex != nullptr;
    Blob b = one_conv_blob(w, bias, {M, K, 1}, M);
    WeightStore ws(b);
    ws.set_bfs_parts(parts);
    PackedConv pc = ws.conv("c");
    const int ld = round_up((int)N, 64);
    Plane X{nullptr, (int)K, (int)N, ld}, Y{nullptr, (int)M, (int)N, ld}, R{nullptr, (int)M, (int)N, ld};
    const size_t xs_bytes = (size_t)split_nplanes(parts) * K * ld * 2 + 64;
    const int64_t Mg = M + (poison ? 1 : 0);   // poison: one guard row behind the f32 plane and behind EVERY part (a write one row past M lands there)
    const size_t ys_bytes = (size_t)3 * Mg * ld * 2 + 64;
    DevMem dx(sizeof(float) * K * ld), dy(sizeof(float) * Mg * ld), dr(sizeof(float) * M * ld), dxs(xs_bytes), dys(ys_bytes);
    X.p = dx.f();
    Y.p = dy.f();
    R.p = dr.f();
    HIP_CHECK(hipMemset(X.p, poison ? 0xFF : 0, sizeof(float) * (size_t)K * ld));
    HIP_CHECK(hipMemcpy2D(X.p, sizeof(float) * ld, x, sizeof(float) * N, sizeof(float) * N, K, hipMemcpyHostToDevice));
    if (poison) {
        HIP_CHECK(hipMemset(R.p, 0xFF, sizeof(float) * (size_t)M * ld));
        HIP_CHECK(hipMemset(Y.p, kCtxSentinel, sizeof(float) * (size_t)Mg * ld));
        HIP_CHECK(hipMemset(dys.p, kCtxSentinel, ys_bytes));
    }
    if (res) HIP_CHECK(hipMemcpy2D(R.p, sizeof(float) * ld, res, sizeof(float) * N, sizeof(float) * N, M, hipMemcpyHostToDevice));
    DevMem dmask(ex ? ex->mask : nullptr, ex && ex->mask ? (size_t)((N + ex->mask_div - 1) / ex->mask_div) : 0);
    SplitPlanes xs;
    xs.p = dxs.p;
    xs.parts = split_nplanes(parts);
    xs.f16 = parts == kPartsF16x3;
    xs.sat = xs.f16 ? f16x3_sat_counter() : nullptr;
    xs.C = (int)K;
    xs.L = (int)N;
    xs.ld = ld;
    xs.pstride = (int64_t)K * ld;
    split_planes(X, xs, nullptr);
    DevMem dx2(x2 ? sizeof(float) * K * ld : 0), dxs2(x2 ? xs_bytes : 0);
    SplitPlanes xs2 = xs;
    if (x2) {
        Plane X2{dx2.f(), (int)K, (int)N, ld};
        HIP_CHECK(hipMemset(X2.p, 0, sizeof(float) * (size_t)K * ld));
        HIP_CHECK(hipMemcpy2D(X2.p, sizeof(float) * ld, x2, sizeof(float) * N, sizeof(float) * N, K, hipMemcpyHostToDevice));
        xs2.p = dxs2.p;
        split_planes(X2, xs2, nullptr);
    }
    SplitPlanes ys;
    ys.p = dys.p;
    ys.parts = split_nplanes(split_out);
    ys.f16 = split_out == kPartsF16x3;
    ys.C = (int)M;
    ys.L = (int)N;
    ys.ld = ld;
    ys.pstride = (int64_t)Mg * ld;
    // split_out: 0 = f32 result only; 2 / 3 = the result is ALSO written as that many bf16 parts, and y returns their sum (what a consumer sees)
    // (scratch for the small-grid K split, as DeBERTa's forward provides it)
    constexpr size_t kWs = (size_t)48 << 20;   // (as BertModel::kSkWsBytes / kSkCounters)
    DevMem dsk(kWs + 1024 * sizeof(float));
    HIP_CHECK(hipMemset(dsk.p, 0, kWs + 1024 * sizeof(float)));
    BfsSplitK sk;
    sk.ws = dsk.f();
    sk.ws_bytes = kWs;
    sk.counters = reinterpret_cast<unsigned*>(dsk.f() + (kWs / sizeof(float)));
    sk.ncounters = 1024;
    int turn = 0;
    auto run = [&]() {
        if (ex)
            conv_bfs(pc, xs, ex->want_y ? &Y : nullptr, split_out ? &ys : nullptr, ex->mask ? dmask.u8() : nullptr, (int)ex->mask_div, nullptr, act,
                     res ? &R : nullptr, ex->alpha, ex->beta, (int)ex->y_rows, (int)ex->ys_row0, &sk);
        else
            conv_bfs(pc, (x2 && (turn++ & 1)) ? xs2 : xs, &Y, split_out ? &ys : nullptr, nullptr, 1, nullptr, act, res ? &R : nullptr, 1.0f, 1.0f, -1, 0, &sk);
    };
    run();
    HIP_CHECK(hipDeviceSynchronize());
    if (iters > 0 && ms) *ms = time_ms(iters, run);
    if (x2) {   // the last launch of each input, back to back on the used scratch
        turn = 1;
        run();
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipMemcpy2D(y2, sizeof(float) * N, Y.p, sizeof(float) * ld, sizeof(float) * N, M, hipMemcpyDeviceToHost));
        turn = 0;
        run();
        HIP_CHECK(hipDeviceSynchronize());
    }
    HIP_CHECK(hipMemcpy2D(y, sizeof(float) * N, Y.p, sizeof(float) * ld, sizeof(float) * N, M, hipMemcpyDeviceToHost));
    int64_t bad = 0;
    if (poison) {
        std::vector<uint32_t> hy((size_t)Mg * ld);
        HIP_CHECK(hipMemcpy(hy.data(), Y.p, 4 * hy.size(), hipMemcpyDeviceToHost));
        for (int64_t m = 0; m < Mg; ++m)
            for (int64_t n = m < M ? N : 0; n < ld; ++n) bad += hy[(size_t)m * ld + n] != kSentinelWord;
    }
    if (split_out) {
        const int np = ys.parts;
        std::vector<uint16_t> hs((size_t)np * Mg * ld);
        HIP_CHECK(hipMemcpy(hs.data(), ys.p, hs.size() * 2, hipMemcpyDeviceToHost));
        if (poison)
            for (int pp = 0; pp < np; ++pp)
                for (int64_t m = 0; m < Mg; ++m)
                    for (int64_t n = m < M ? N : 0; n < ld; ++n) bad += hs[((size_t)pp * Mg + m) * ld + n] != (uint16_t)(kSentinelWord & 0xFFFF);
        if (ex) y = ex->ys;   // (the f32 plane went to the caller's y above)
        for (int64_t m = 0; m < M; ++m)
            for (int64_t n = 0; n < N; ++n) {
                float acc = 0.f;
                if (ys.f16) {
                    _Float16 hi, lo;
                    memcpy(&hi, &hs[(size_t)m * ld + n], 2);
                    memcpy(&lo, &hs[((size_t)Mg + m) * ld + n], 2);
                    y[(size_t)m * N + n] = (float)hi + (float)lo * (1.0f / kF16LoScale);
                    continue;
                }
                for (int pp = np - 1; pp >= 0; --pp) {
                    const uint32_t u = (uint32_t)hs[((size_t)pp * Mg + m) * ld + n] << 16;
                    float f;
                    memcpy(&f, &u, 4);
                    acc += f;
                }
                y[(size_t)m * N + n] = acc;
            }
    }
    if (ex && ex->stray) *ex->stray = bad;
    API_END
}

int sbv2_debug_gemm_bfs_ex(int device, const float* x, const float* w, const float* bias, const float* res, int64_t M, int64_t N, int64_t K, int parts, int act,
                           int split_out, int64_t iters, const uint8_t* mask, int64_t mask_div, float alpha, float beta, int64_t y_rows, int64_t ys_row0,
                           int want_y, float* y, float* ys, float* ms, int64_t* stray) {
    BfsHookEx ex;
    ex.mask = mask;
    ex.mask_div = mask_div;
    ex.alpha = alpha;
    ex.beta = beta;
    ex.y_rows = y_rows;
    ex.ys_row0 = ys_row0;
    ex.want_y = want_y;
    ex.ys = ys;
    ex.stray = stray;
    return debug_gemm_bfs_impl(device, x, nullptr, w, bias, res, M, N, K, parts, act, split_out, iters, y, nullptr, ms, &ex);
}

int sbv2_debug_gemm_bfs(int device, const float* x, const float* w, const float* bias, const float* res, int64_t M, int64_t N, int64_t K,
                        int parts, int act, int split_out, int64_t iters, float* y, float* ms) {
    return debug_gemm_bfs_impl(device, x, nullptr, w, bias, res, M, N, K, parts, act, split_out, iters, y, nullptr, ms);
}
int sbv2_debug_gemm_bfs_alt(int device, const float* xa, const float* xb, const float* w, const float* bias, const float* res, int64_t M, int64_t N, int64_t K,
                            int parts, int64_t iters, float* ya, float* yb) {
    if (!xb || !yb) {
        set_last_error("bad arguments");
        return 1;
    }
    float ms = 0.f;
    return debug_gemm_bfs_impl(device, xa, xb, w, bias, res, M, N, K, parts, 0, 0, iters, ya, yb, &ms);
}

int sbv2_debug_time_conv1d(int device, int64_t cin, int64_t cout, int64_t k, int64_t L, int64_t dilation, int64_t iters, float* ms) {
    API_BEGIN
    HIP_CHECK(hipSetDevice(device));
    SBV2_REQUIRE(ms && iters >= 1, "bad arguments");
    std::vector<float> w((size_t)cout * cin * k), bias((size_t)cout, 0.1f);
    uint32_t st = 12345u;
    auto rnd = [&]() {
        st = st * 1664525u + 1013904223u;
        return ((st >> 8) * (1.0f / 16777216.0f) - 0.5f);
    };
    for (auto& v : w) v = rnd() * 0.1f;
    Blob b = one_conv_blob(w.data(), bias.data(), {cout, cin, k}, cout);
    WeightStore ws(b);
    PackedConv pc = ws.conv("c");
    Plane X{nullptr, (int)cin, (int)L, round_up((int)L, 64)}, Y{nullptr, (int)cout, (int)L, round_up((int)L, 64)};
    std::vector<float> hx((size_t)cin * X.ld);
    for (auto& v : hx) v = rnd() * 2.f;
    DevMem dx(hx.data(), sizeof(float) * hx.size()), dy(sizeof(float) * cout * Y.ld);
    X.p = dx.f();
    Y.p = dy.f();
    auto run = [&] { conv_plain(pc, X, Y, (int)dilation, (int)(dilation * (k - 1) / 2), nullptr, 1, nullptr, ACT_NONE, 1.0f); };
    for (int i = 0; i < 3; ++i) run();
    *ms = time_ms(iters, run);
    API_END
}

int sbv2_debug_vits_attention(int device, const float* q, const float* k, const float* v, const float* erk, const float* erv, const int64_t* lens, int nutt,
                              int64_t heads, int64_t dk, int64_t window, int layout, int variant, int poison, float* ctx, int64_t* stray) {
    API_BEGIN
    HIP_CHECK(hipSetDevice(device));
    SBV2_REQUIRE(q && k && v && erk && erv && lens && ctx && nutt >= 1 && heads >= 1 && dk >= 1 && window >= 0 && (layout == 0 || layout == 1) &&
                     variant >= -1 && variant <= 5,
                 "bad arguments");
    std::vector<int> L(nutt);
    for (int i = 0; i < nutt; ++i) {
        SBV2_REQUIRE(lens[i] >= 1 && lens[i] < (1 << 20), "bad sequence length");
        L[i] = (int)lens[i];
    }
    const int H = (int)(heads * dk), nw = 2 * (int)window + 1;
    Arena ar;
    // the text encoder's layout (kTextGap, columns rounded to 4) or the flow's (kFrameGap, rounded to 32), as VitsModel builds them
    const SegLayout lay = layout ? make_layout(L, kFrameGap, ar, nullptr, nullptr, 32) : make_layout(L, kTextGap, ar, nullptr);
    const int N = lay.L;
    Plane QKV = ar.plane(3 * H, N), C = ar.plane(H, N);
    Plane Q = QKV.rows(0, H), K = QKV.rows(H, H), V = QKV.rows(2 * H, H);
    upload_packed(q, lay, Q, poison);
    upload_packed(k, lay, K, poison);
    upload_packed(v, lay, V, poison);
    DevMem d_erk(erk, sizeof(float) * nw * dk), d_erv(erv, sizeof(float) * nw * dk);
    const AttnPlan pl = make_attn_plan(lay, H, (int)heads, QKV.ld, (int)window, ar, nullptr, variant == 0);
    HIP_CHECK(hipMemset(C.p, poison ? kCtxSentinel : 0, sizeof(float) * (size_t)H * C.ld));
    const float qscale = 1.0f / std::sqrt((float)dk);   // as run_encoder
    // keys / values as the bf16 parts the flow's q | k | v product writes next to the f32 plane (its epilogue: split_store4's bf16 split, the one
    // split_planes uses), in the same place: rows H .. 3 H of a [3 H][N] split plane
    auto kv_parts = [&]() {
        SplitPlanes s = alloc_split(ar, 2, 3 * H, N);
        HIP_CHECK(hipMemset(s.p, poison ? 0xFF : 0, (size_t)2 * s.pstride * 2));
        split_planes(QKV.rows(H, 2 * H), s.rows(H, 2 * H), nullptr);
        return s;
    };
    const bool split_attn = dk % 16 == 0;   // run_encoder: the flow's split-bf16 attention takes head dimensions of whole 16-row steps
    const int dki = (int)dk, w = (int)window;
    if (variant == -1) {
        const FlashChoice fc = flash_choice(pl, kPartsF16x3, split_attn, dki);   // the flow: its 1x1 products on pre-split operands
        if (fc.kv_parts) vits_flash_attention_parts(pl.d_ag, pl.ng, pl.maxT, Q.p, Q.ld, kv_parts(), H, 2 * H, C.p, C.ld, dki, d_erk.f(), d_erv.f(), w, qscale,
                                                    nullptr, fc.pipelined);
        else vits_flash_attention(pl.d_ag, pl.ng, pl.maxT, Q.p, K.p, V.p, Q.ld, C.p, C.ld, dki, d_erk.f(), d_erv.f(), w, qscale, split_attn, nullptr);
    } else if (variant == 0) {
        DevMem vt = upload_tokmajor(v, lay, H, poison);
        grouped_gemm(K.p, K.ld, Q.p, Q.ld, pl.S, pl.lds, pl.d_st, pl.ng, pl.maxT, pl.maxT, qscale, pl.flops, nullptr);
        vits_softmax(pl.d_ag, pl.ng, pl.maxT, pl.S, Q.p, Q.ld, dki, d_erk.f(), w, qscale, pl.PW, nullptr);
        grouped_gemm(vt.f(), H, pl.S, pl.lds, C.p, C.ld, pl.d_pv, pl.ng, dki, pl.maxT, 1.0f, pl.flops, nullptr);
        vits_relv_add(pl.d_ag, pl.ng, pl.maxT, C.p, C.ld, dki, d_erv.f(), w, pl.PW, nullptr);
        HIP_CHECK(hipDeviceSynchronize());
    } else if (variant <= 2) {
        vits_flash_attention(pl.d_ag, pl.ng, pl.maxT, Q.p, K.p, V.p, Q.ld, C.p, C.ld, dki, d_erk.f(), d_erv.f(), w, qscale, variant == 2, nullptr);
    } else {
        SBV2_REQUIRE(variant == 3 || flash_pipelined_usable(dki), "k_vits_flash_x3q does not take this head dimension");
        vits_flash_attention_parts(pl.d_ag, pl.ng, pl.maxT, Q.p, Q.ld, kv_parts(), H, 2 * H, C.p, C.ld, dki, d_erk.f(), d_erv.f(), w, qscale, nullptr,
                                   variant == 3 ? 0 : (variant == 4 ? 3 : 2));
    }
    HIP_CHECK(hipDeviceSynchronize());
    download_packed(C, lay, poison, ctx, stray);
    API_END
}

int sbv2_debug_deberta_attention(int device, const float* q, const float* k, const float* v, const float* pos_k, const float* pos_q, const int64_t* lens,
                                 int nutt, int64_t heads, int64_t d, int64_t buckets, int64_t max_rel, const uint8_t* tok_mask, int64_t gap, int variant,
                                 int poison, float* ctx, int64_t* stray) {
    API_BEGIN
    HIP_CHECK(hipSetDevice(device));
    SBV2_REQUIRE(q && k && v && pos_k && pos_q && lens && ctx && nutt >= 1 && heads >= 1 && d >= 1 && gap >= 0 && variant >= -1 && variant <= 3 &&
                     (buckets > 0 || max_rel > 0),
                 "bad arguments");
    std::vector<int> L(nutt);
    int64_t total = 0;
    for (int i = 0; i < nutt; ++i) {
        SBV2_REQUIRE(lens[i] >= 1 && lens[i] < (1 << 20), "bad sequence length");
        L[i] = (int)lens[i];
        total += lens[i];
    }
    const int H = (int)(heads * d), span = (int)(buckets > 0 ? buckets : max_rel);
    std::vector<unsigned char> am((size_t)total, 1);
    if (tok_mask)
        for (int64_t e = 0; e < total; ++e) am[e] = tok_mask[e] != 0;
    Arena ar;
    const SegLayout lay = make_layout(L, (int)gap, ar, nullptr, am.data());   // as BertModel::forward
    const int N = lay.L;
    Plane QKV = ar.plane(3 * H, N), C = ar.plane(H, N), PK = ar.plane(H, 2 * span), PQ = ar.plane(H, 2 * span);
    Plane Q = QKV.rows(0, H), K = QKV.rows(H, H), V = QKV.rows(2 * H, H);
    upload_packed(q, lay, Q, poison);
    upload_packed(k, lay, K, poison);
    upload_packed(v, lay, V, poison);
    for (Plane* P : {&PK, &PQ}) {
        HIP_CHECK(hipMemset(P->p, 0, sizeof(float) * (size_t)H * P->ld));
        HIP_CHECK(hipMemcpy2D(P->p, sizeof(float) * P->ld, P == &PK ? pos_k : pos_q, sizeof(float) * 2 * span, sizeof(float) * 2 * span, H,
                              hipMemcpyHostToDevice));
    }
    DebertaAttnPlan ap = make_deberta_attn_plan(lay, H, (int)heads, (int)buckets, (int)max_rel, QKV.ld, PK.ld, variant);
    ap.upload_table(ar, nullptr);
    ap.upload_groups(ar, nullptr, N, H);
    HIP_CHECK(hipMemset(C.p, poison ? kCtxSentinel : 0, sizeof(float) * (size_t)H * C.ld));
    const float inv_scale = 1.0f / std::sqrt((float)d * 3.0f);   // as BertModel::forward
    deberta_attention_fused(ap, Q.p, K.p, V.p, QKV.ld, PK.p, PQ.p, PK.ld, (int)d, inv_scale, lay.d_mask, C.p, C.ld, nullptr);
    if (ap.ngL()) {
        DevMem vt = upload_tokmajor(v, lay, H, poison);
        HIP_CHECK(hipMemcpy(ap.VT, vt.p, sizeof(float) * (size_t)N * H, hipMemcpyDeviceToDevice));
        deberta_attention_unfused(ap, Q.p, K.p, QKV.ld, ap.VT, H, PK.p, PQ.p, PK.ld, (int)d, inv_scale, lay.d_mask, C.p, C.ld, nullptr);
    }
    HIP_CHECK(hipDeviceSynchronize());
    download_packed(C, lay, poison, ctx, stray);
    API_END
}

int sbv2_debug_layout(const int64_t* lens, int nutt, int kind, int32_t* start, int64_t* L) {
    API_BEGIN
    SBV2_REQUIRE(start && L, "bad arguments");
    Arena ar;
    const SegLayout lay = hook_layout(lens, nutt, kind, ar);
    HIP_CHECK(hipDeviceSynchronize());
    for (int u = 0; u < nutt; ++u) start[u] = lay.start[u];
    *L = lay.L;
    API_END
}

int sbv2_debug_layernorm(int device, const float* x, const float* gamma, const float* beta, float eps, int act, const float* res, const uint8_t* mask,
                         const float* dw_w, const float* dw_b, int64_t dil, int64_t C, int64_t L, int inplace, int split_code, int poison, float* y,
                         float* ysplit, int64_t* stray) {
    API_BEGIN
    HIP_CHECK(hipSetDevice(device));
    SBV2_REQUIRE(x && gamma && beta && y && (act == ACT_NONE || act == ACT_GELU) && (split_code == 0 || split_code == 2 || split_code == kPartsF16x3) &&
                     (!split_code || ysplit) && (!dw_w || (dw_b && !res && !inplace && !split_code && dil >= 1)),
                 "bad arguments");
    Arena ar;
    DevPlane X(C, L), Yo(inplace ? 1 : C, inplace ? 1 : L), R(res ? C : 1, res ? L : 1);
    X.put(x, poison);
    if (res) R.put(res, poison);
    if (!inplace) Yo.fill(poison);
    const Plane Y = inplace ? X.P : Yo.P;
    DevMem dg(gamma, sizeof(float) * C), db(beta, sizeof(float) * C), dm(mask, mask ? (size_t)L : 0), dw(dw_w, dw_w ? sizeof(float) * 3 * C : 0),
        dwb(dw_b, dw_w ? sizeof(float) * C : 0);
    SplitPlanes sp;
    if (split_code) {
        sp = alloc_split(ar, split_code, (int)C, (int)L);
        HIP_CHECK(hipMemset(sp.p, kCtxSentinel, (size_t)sp.parts * sp.pstride * 2));
    }
    if (dw_w) dds_dw_ln_gelu(X.P, Y, dw.f(), dwb.f(), (int)dil, dg.f(), db.f(), mask ? dm.u8() : nullptr, nullptr);
    else layernorm_ch(X.P, Y, dg.f(), db.f(), eps, act, res ? R.P.p : nullptr, R.P.ld, mask ? dm.u8() : nullptr, nullptr, split_code ? &sp : nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    int64_t bad = (inplace ? X : Yo).get(y, inplace ? kNanWord : kSentinelWord);
    if (split_code) {   // hi + lo of the parts (the f16 pair: lo scaled back), and the pad columns of every part
        std::vector<uint16_t> hs((size_t)sp.parts * sp.pstride);
        HIP_CHECK(hipMemcpy(hs.data(), sp.p, hs.size() * 2, hipMemcpyDeviceToHost));
        for (int64_t c = 0; c < C; ++c)
            for (int64_t n = 0; n < sp.ld; ++n) {
                if (n >= L) {
                    for (int pp = 0; pp < sp.parts; ++pp) bad += hs[(size_t)pp * sp.pstride + c * sp.ld + n] != (uint16_t)(kSentinelWord & 0xFFFF);
                    continue;
                }
                if (sp.f16) {
                    _Float16 hi, lo;
                    memcpy(&hi, &hs[(size_t)c * sp.ld + n], 2);
                    memcpy(&lo, &hs[(size_t)sp.pstride + c * sp.ld + n], 2);
                    ysplit[(size_t)c * L + n] = (float)hi + (float)lo * (1.0f / kF16LoScale);
                    continue;
                }
                float acc = 0.f;
                for (int pp = sp.parts - 1; pp >= 0; --pp) {
                    const uint32_t u = (uint32_t)hs[(size_t)pp * sp.pstride + c * sp.ld + n] << 16;
                    float f;
                    memcpy(&f, &u, 4);
                    acc += f;
                }
                ysplit[(size_t)c * L + n] = acc;
            }
    }
    if (stray) *stray = poison ? bad : 0;
    API_END
}

int sbv2_debug_deberta_embed_ln(int device, const int32_t* ids, const float* emb, int64_t V, int64_t H, const float* gamma, const float* beta, float eps,
                                int64_t N, int poison, float* y, int64_t* stray) {
    API_BEGIN
    HIP_CHECK(hipSetDevice(device));
    SBV2_REQUIRE(ids && emb && gamma && beta && y && V >= 1 && H >= 1, "bad arguments");
    for (int64_t n = 0; n < N; ++n) SBV2_REQUIRE(ids[n] < V, "token id outside the table");
    DevPlane Y(H, N);
    Y.fill(poison);
    DevMem di(ids, sizeof(int) * N), de(emb, sizeof(float) * V * H), dg(gamma, sizeof(float) * H), db(beta, sizeof(float) * H);
    deberta_embed_ln(static_cast<const int*>(di.p), de.f(), (int)H, dg.f(), db.f(), eps, Y.P, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    const int64_t bad = Y.get(y, kSentinelWord);
    if (stray) *stray = poison ? bad : 0;
    API_END
}

int sbv2_debug_spline_inverse(int device, const float* params, const float* z, const uint8_t* mask, int64_t L, int64_t nbins, float tail, float inv_sqrt_f,
                              int poison, float* z_out, int64_t* stray) {
    API_BEGIN
    HIP_CHECK(hipSetDevice(device));
    SBV2_REQUIRE(params && z && mask && z_out && nbins >= 1, "bad arguments");
    DevPlane PR(3 * nbins - 1, L), Z(2, L);   // z0 | z1 as the two rows of one plane, as the duration flow keeps them
    PR.put(params, poison);
    Z.put(z, poison);
    DevMem dm(mask, (size_t)L);
    spline_inverse(PR.P, Z.P.p, Z.P.p + Z.P.ld, (int)nbins, tail, inv_sqrt_f, dm.u8(), (int)L, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    const int64_t bad = Z.get(z_out, kNanWord);
    if (stray) *stray = poison ? bad : 0;
    API_END
}

// durations over a text layout of nutt segments with each row's (ratio, length_scale); sdp, dp, mask, logw, dur: [L of the layout]
int sbv2_debug_durations_rows(int device, const float* sdp, const float* dp, const uint8_t* mask, const int64_t* lens, int nutt, const float* ratio,
                              const float* length_scale, float* logw, int32_t* dur, int64_t* stray) {
    API_BEGIN
    HIP_CHECK(hipSetDevice(device));
    SBV2_REQUIRE(sdp && dp && mask && ratio && length_scale && logw && dur, "bad arguments");
    Arena ar;
    const SegLayout lay = hook_layout(lens, nutt, 0, ar);
    const int64_t L = lay.L;
    DevPlane S(1, L), D(1, L), W(1, L), U(1, L);
    S.put(sdp, true);
    D.put(dp, true);
    W.fill(true);
    U.fill(true);
    DevMem dm(mask, (size_t)L);
    durations(S.P.p, D.P.p, lay.d_seg_of, upload_rows(ar, nutt, nullptr, 0, nullptr, ratio, 0.f, length_scale, 1.f, nullptr, 0.f, nullptr, 0.f), dm.u8(),
              (int)L, W.P.p, reinterpret_cast<int*>(U.P.p), nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    const int64_t bad = W.get(logw, kSentinelWord) + U.get(dur, kSentinelWord);
    if (stray) *stray = bad;
    API_END
}

// (one segment of L columns without gaps: the row's scalars are the call's)
int sbv2_debug_durations(int device, const float* sdp, const float* dp, const uint8_t* mask, int64_t L, float ratio, float length_scale, float* logw,
                         int32_t* dur, int64_t* stray) {
    API_BEGIN
    HIP_CHECK(hipSetDevice(device));
    SBV2_REQUIRE(sdp && dp && mask && logw && dur, "bad arguments");
    Arena ar;
    DevPlane S(1, L), D(1, L), W(1, L), U(1, L);
    S.put(sdp, true);
    D.put(dp, true);
    W.fill(true);
    U.fill(true);
    DevMem dm(mask, (size_t)L);
    const std::vector<int32_t> seg_of((size_t)std::max<int64_t>(L, 0), 0);
    durations(S.P.p, D.P.p, upload_ints(ar, seg_of.data(), (size_t)L),
              upload_rows(ar, 1, nullptr, 0, nullptr, nullptr, ratio, nullptr, length_scale, nullptr, 0.f, nullptr, 0.f), dm.u8(), (int)L, W.P.p,
              reinterpret_cast<int*>(U.P.p), nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    const int64_t bad = W.get(logw, kSentinelWord) + U.get(dur, kSentinelWord);
    if (stray) *stray = bad;
    API_END
}

int sbv2_debug_affine_reverse(int device, const float* z, const float* m, const float* logs, const float* scale, const uint8_t* mask, int64_t L,
                              float* z_out, int64_t* stray) {
    API_BEGIN
    HIP_CHECK(hipSetDevice(device));
    SBV2_REQUIRE(z && m && (logs || scale) && mask && z_out, "bad arguments");
    DevPlane Z(2, L);
    Z.put(z, true);
    DevMem dmn(m, 8), dl(logs, logs ? 8 : 0), ds(scale, scale ? 8 : 0), dm(mask, (size_t)L);
    affine_reverse(Z.P.p, Z.P.p + Z.P.ld, dmn.f(), logs ? dl.f() : nullptr, scale ? ds.f() : nullptr, dm.u8(), (int)L, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    const int64_t bad = Z.get(z_out, kNanWord);
    if (stray) *stray = bad;
    API_END
}

int sbv2_debug_convflow_pre(int device, const float* z0, const float* w, const float* b, const float* cond, const uint8_t* mask, int64_t C, int64_t L,
                            float* y, int64_t* stray) {
    API_BEGIN
    HIP_CHECK(hipSetDevice(device));
    SBV2_REQUIRE(z0 && w && b && cond && mask && y, "bad arguments");
    DevPlane Z(1, L), CO(C, L), Y(C, L);
    Z.put(z0, true);
    CO.put(cond, true);
    Y.fill(true);
    DevMem dw(w, sizeof(float) * C), db(b, sizeof(float) * C), dm(mask, (size_t)L);
    convflow_pre(Z.P.p, dw.f(), db.f(), CO.P, Y.P, dm.u8(), nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    const int64_t bad = Y.get(y, kSentinelWord);
    if (stray) *stray = bad;
    API_END
}

// noise_fill / expand_frames with each row's (seed, index, scale); the scalar hooks below are the same calls with one seed and scale for every row
int sbv2_debug_noise_fill_rows(int device, const int64_t* lens, int nutt, int kind, const uint64_t* seed, const int32_t* index, int stream_id,
                               const float* scale, int64_t rows, float* y, int64_t* stray) {
    API_BEGIN
    HIP_CHECK(hipSetDevice(device));
    SBV2_REQUIRE(seed && index && scale && y && rows >= 1, "bad arguments");
    Arena ar;
    const SegLayout lay = hook_layout(lens, nutt, kind, ar);
    DevPlane Y(rows, lay.L);
    Y.fill(true);
    noise_fill(Y.P.p, Y.P.ld, (int)rows, lay.d_seg_of, lay.d_start, lay.d_len,
               upload_rows(ar, nutt, seed, 0, index, nullptr, 0.f, nullptr, 1.f, nullptr, 0.f, scale, 0.f), lay.L, stream_id, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    const int64_t bad = Y.get(y, kSentinelWord);
    if (stray) *stray = bad;
    API_END
}

int sbv2_debug_noise_fill(int device, const int64_t* lens, int nutt, int kind, const int32_t* seg_utt, uint64_t seed, int stream_id, float scale,
                          int64_t rows, float* y, int64_t* stray) {
    const std::vector<uint64_t> seeds((size_t)std::max(nutt, 1), seed);   // (a null seg_utt and nutt < 1 are refused by the call below, as ever)
    const std::vector<float> scales((size_t)std::max(nutt, 1), scale);
    return sbv2_debug_noise_fill_rows(device, lens, nutt, kind, seeds.data(), seg_utt, stream_id, scales.data(), rows, y, stray);
}

int sbv2_debug_expand_frames_rows(int device, const float* m_p, const float* logs_p, int64_t C, int64_t Lt, const int32_t* tok_of_frame, const int64_t* lens,
                                  int nutt, const uint64_t* seed, const int32_t* index, const float* noise_scale, float* y, int64_t* stray) {
    API_BEGIN
    HIP_CHECK(hipSetDevice(device));
    SBV2_REQUIRE(m_p && logs_p && tok_of_frame && seed && index && noise_scale && y, "bad arguments");
    Arena ar;
    const SegLayout lay = hook_layout(lens, nutt, 1, ar);
    const std::vector<unsigned char> inside = layout_inside(lay);
    for (int n = 0; n < lay.L; ++n) SBV2_REQUIRE(tok_of_frame[n] < Lt && (inside[n] || tok_of_frame[n] < 0), "token map outside the text plane or in a gap");
    DevPlane M(C, Lt), S(C, Lt), Y(C, lay.L);
    M.put(m_p, true);
    S.put(logs_p, true);
    Y.fill(true);
    expand_frames(M.P, S.P, upload_ints(ar, tok_of_frame, lay.L), lay.d_seg_of, lay.d_start, lay.d_len,
                  upload_rows(ar, nutt, seed, 0, index, nullptr, 0.f, nullptr, 1.f, noise_scale, 0.f, nullptr, 0.f), Y.P, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    const int64_t bad = Y.get(y, kSentinelWord);
    if (stray) *stray = bad;
    API_END
}

int sbv2_debug_expand_frames(int device, const float* m_p, const float* logs_p, int64_t C, int64_t Lt, const int32_t* tok_of_frame, const int64_t* lens,
                             int nutt, const int32_t* seg_utt, uint64_t seed, float noise_scale, float* y, int64_t* stray) {
    const std::vector<uint64_t> seeds((size_t)std::max(nutt, 1), seed);   // (a null seg_utt and nutt < 1 are refused by the call below, as ever)
    const std::vector<float> scales((size_t)std::max(nutt, 1), noise_scale);
    return sbv2_debug_expand_frames_rows(device, m_p, logs_p, C, Lt, tok_of_frame, lens, nutt, seeds.data(), seg_utt, scales.data(), y, stray);
}

int sbv2_debug_conv_post_tanh(int device, const float* x, const float* w, int64_t C, int64_t k, const int64_t* lens, int nutt, int64_t up, int cl,
                              float* pcm, int64_t* stray) {
    API_BEGIN
    HIP_CHECK(hipSetDevice(device));
    SBV2_REQUIRE(x && w && pcm && C >= 1 && k >= 1 && up >= 1, "bad arguments");
    Arena ar;
    const SegLayout lay = hook_layout(lens, nutt, 1, ar);
    const int64_t L = (int64_t)lay.L * up;
    std::vector<int64_t> off(nutt);
    int64_t tot = 0, maxlen = 0;
    for (int u = 0; u < nutt; ++u) {   // compact PCM, one contiguous block per utterance (as the decoders)
        off[u] = tot;
        tot += (int64_t)lay.len[u] * up;
        maxlen = std::max(maxlen, (int64_t)lay.len[u] * up);
    }
    constexpr int64_t kGuard = 256;
    DevMem dp(sizeof(float) * (size_t)(tot + kGuard)), dw(w, sizeof(float) * C * k), doff(off.data(), sizeof(int64_t) * nutt);
    HIP_CHECK(hipMemset(dp.p, kCtxSentinel, sizeof(float) * (size_t)(tot + kGuard)));
    if (cl) {
        DevMem dx = upload_cl(x, C, L);
        conv_post_tanh_cl(dx.f(), (int)C, L, dw.f(), (int)k, 0.01f, lay.d_start, lay.d_len, static_cast<const int64_t*>(doff.p), nutt, (int)up, maxlen,
                          dp.f(), nullptr);
        HIP_CHECK(hipDeviceSynchronize());
    } else {
        DevPlane X(C, L);
        X.put(x, true);
        conv_post_tanh(X.P, dw.f(), (int)k, 0.01f, lay.d_start, lay.d_len, static_cast<const int64_t*>(doff.p), nutt, (int)up, maxlen, dp.f(), nullptr);
        HIP_CHECK(hipDeviceSynchronize());
    }
    std::vector<uint32_t> h((size_t)(tot + kGuard));
    HIP_CHECK(hipMemcpy(h.data(), dp.p, 4 * h.size(), hipMemcpyDeviceToHost));
    std::memcpy(pcm, h.data(), 4 * (size_t)tot);
    int64_t bad = 0;
    for (int64_t e = tot; e < tot + kGuard; ++e) bad += h[e] != kSentinelWord;
    if (stray) *stray = bad;
    API_END
}

int sbv2_debug_linear_vec(int device, const float* W, const float* bias, int64_t M, int64_t K, const float* v, int64_t B, float* y) {
    API_BEGIN
    HIP_CHECK(hipSetDevice(device));
    SBV2_REQUIRE(W && v && y && M >= 1 && K >= 1 && B >= 1, "bad arguments");
    DevMem dW(W, sizeof(float) * M * K), db(bias, bias ? sizeof(float) * M : 0), dv(v, sizeof(float) * B * K), dy(sizeof(float) * B * M);
    linear_vec(dW.f(), bias ? db.f() : nullptr, (int)M, (int)K, dv.f(), (int)K, dy.f(), (int)M, (int)B, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(y, dy.p, sizeof(float) * B * M, hipMemcpyDeviceToHost));
    API_END
}

int sbv2_debug_gather_rows(int device, const float* table, int64_t V, int64_t K, const int32_t* idx, int64_t B, float* y) {
    API_BEGIN
    HIP_CHECK(hipSetDevice(device));
    SBV2_REQUIRE(table && idx && y && V >= 1 && K >= 1 && B >= 1, "bad arguments");
    for (int64_t b = 0; b < B; ++b) SBV2_REQUIRE(idx[b] >= 0 && idx[b] < V, "row index outside the table");
    DevMem dt(table, sizeof(float) * V * K), di(idx, sizeof(int) * B), dy(sizeof(float) * B * K);
    gather_rows(dt.f(), (int)K, static_cast<const int*>(di.p), dy.f(), (int)B, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(y, dy.p, sizeof(float) * B * K, hipMemcpyDeviceToHost));
    API_END
}

int sbv2_debug_text_embed(int device, const int32_t* phones, const int32_t* tones, const int32_t* langs, const int64_t* lens, int nutt, const float* emb,
                          int64_t nph, const float* tone_emb, int64_t ntone, const float* lang_emb, int64_t nlang, const float* bertproj,
                          const float* styleproj, float scale, int64_t H, float* y, int64_t* stray) {
    API_BEGIN
    HIP_CHECK(hipSetDevice(device));
    SBV2_REQUIRE(phones && tones && langs && emb && tone_emb && lang_emb && bertproj && styleproj && y && H >= 1, "bad arguments");
    Arena ar;
    const SegLayout lay = hook_layout(lens, nutt, 0, ar);
    const std::vector<unsigned char> inside = layout_inside(lay);
    for (int n = 0; n < lay.L; ++n)
        SBV2_REQUIRE(!inside[n] || (phones[n] >= 0 && phones[n] < nph && tones[n] >= 0 && tones[n] < ntone && langs[n] >= 0 && langs[n] < nlang),
                     "symbol outside its table");
    DevPlane BP(H, lay.L), Y(H, lay.L);
    BP.put(bertproj, true, inside.data());
    Y.fill(true);
    DevMem de(emb, sizeof(float) * nph * H), dt(tone_emb, sizeof(float) * ntone * H), dl(lang_emb, sizeof(float) * nlang * H),
        ds(styleproj, sizeof(float) * nutt * H);
    text_embed(upload_ints(ar, phones, lay.L), upload_ints(ar, tones, lay.L), upload_ints(ar, langs, lay.L), lay.d_seg_of, de.f(), dt.f(), dl.f(), BP.P.p,
               BP.P.ld, ds.f(), (int)H, scale, Y.P, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    const int64_t bad = Y.get(y, kSentinelWord);
    if (stray) *stray = bad;
    API_END
}

int sbv2_debug_add_segvec(int device, const float* x, const float* vec, int64_t C, const int64_t* lens, int nutt, int kind, int64_t div,
                          const uint8_t* tok_mask, int use_mask, int cl, float* y, int64_t* stray) {
    API_BEGIN
    HIP_CHECK(hipSetDevice(device));
    SBV2_REQUIRE(x && vec && y && C >= 1 && div >= 1 && (!cl || (div == 1 && use_mask && (C & 3) == 0)), "bad arguments");
    Arena ar;
    const SegLayout lay = hook_layout(lens, nutt, kind, ar, tok_mask);
    const int64_t L = (int64_t)lay.L * div;
    DevMem dv(vec, sizeof(float) * nutt * C);
    int64_t bad = 0;
    if (cl) {
        DevMem dx = upload_cl(x, C, L);
        add_segvec_cl(dx.f(), (int)L, (int)C, dv.f(), (int)C, lay.d_seg_of, lay.d_mask, nullptr);
        HIP_CHECK(hipDeviceSynchronize());
        download_cl(dx.f(), C, L, y);
    } else {
        const std::vector<unsigned char> inside = layout_inside(lay, (int)div);
        DevPlane X(C, L);
        X.put(x, true, inside.data());
        add_segvec(X.P, dv.f(), (int)C, lay.d_seg_of, (int)div, use_mask ? lay.d_mask : nullptr, nullptr);
        HIP_CHECK(hipDeviceSynchronize());
        bad = X.get(y, kNanWord);
    }
    if (stray) *stray = bad;
    API_END
}

// The two kernels of assist.hip on a host plane at the caller's pitch, between NaN words; the row table is the one pipeline_run_one builds
int sbv2_debug_assist_blend(int device, const float* F, int64_t C, int64_t ld, const int32_t* map, const int32_t* row_of, int64_t L, int64_t A,
                            const int32_t* a_start, const int32_t* a_len, int64_t n_rows, const int32_t* text_of, const double* weight, float* mean,
                            float* out, int64_t* stray) {
    API_BEGIN
    SBV2_REQUIRE(F && map && row_of && a_start && a_len && text_of && weight && mean && out, "bad arguments");
    SBV2_REQUIRE(C >= 1 && C < (1 << 20) && ld >= 1 && ld < (1 << 28) && L >= 1 && L < (1 << 28) && A >= 1 && A < (1 << 20) && n_rows >= 1 && n_rows < (1 << 20),
                 "bad shapes");
    for (int64_t a = 0; a < A; ++a)
        SBV2_REQUIRE(a_len[a] >= 1 && a_start[a] >= 0 && (int64_t)a_start[a] + a_len[a] <= ld, "assist sequence " + std::to_string(a) + " outside the plane");
    for (int64_t t = 0; t < L; ++t) {
        SBV2_REQUIRE(map[t] < ld, "column map outside the plane");
        SBV2_REQUIRE(map[t] < 0 || (row_of[t] >= 0 && row_of[t] < n_rows), "row_of outside the rows at column " + std::to_string(t));
    }
    const std::vector<AssistRow> rows = assist_row_table(n_rows, (int)A, text_of, weight);
    HIP_CHECK(hipSetDevice(device));
    constexpr size_t kPad = 64;
    const size_t nF = (size_t)C * ld, nM = (size_t)A * C;
    std::vector<uint32_t> hF(nF + 2 * kPad, kNanWord);
    std::memcpy(hF.data() + kPad, F, sizeof(float) * nF);
    DevMem dF(hF.data(), 4 * hF.size()), dM(4 * (nM + 2 * kPad));
    HIP_CHECK(hipMemset(dM.p, kCtxSentinel, 4 * (nM + 2 * kPad)));
    DevPlane Y(C, L);
    Y.fill(true);
    DevMem dmap(map, sizeof(int) * L), drow(row_of, sizeof(int) * L), das(a_start, sizeof(int) * A), dal(a_len, sizeof(int) * A),
        drows(rows.data(), sizeof(AssistRow) * rows.size());
    const Plane P{dF.f() + kPad, (int)C, (int)ld, (int)ld};
    assist_mean(P, static_cast<const int*>(das.p), static_cast<const int*>(dal.p), (int)A, dM.f() + kPad, nullptr);
    gather_cols_assist(P, static_cast<const int*>(dmap.p), static_cast<const int*>(drow.p), static_cast<const AssistRow*>(drows.p), dM.f() + kPad, Y.P,
                       nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    int64_t bad = Y.get(out, kSentinelWord);
    std::vector<uint32_t> hM(nM + 2 * kPad);
    HIP_CHECK(hipMemcpy(hM.data(), dM.p, 4 * hM.size(), hipMemcpyDeviceToHost));
    std::memcpy(mean, hM.data() + kPad, 4 * nM);
    for (size_t e = 0; e < kPad; ++e) bad += (hM[e] != kSentinelWord) + (hM[kPad + nM + e] != kSentinelWord);
    if (stray) *stray = bad;
    API_END
}

int sbv2_debug_plane_op(int device, int op, const float* x, int64_t C, int64_t L, const int32_t* map, int64_t a, int64_t b, float* y, uint8_t* mask_out,
                        int64_t* stray) {
    API_BEGIN
    HIP_CHECK(hipSetDevice(device));
    SBV2_REQUIRE(x && y && op >= 0 && op <= 4, "bad arguments");
    DevPlane X(C, L);
    X.put(x, true);
    int64_t bad = 0;
    if (op == 0) {          // gather_cols: map [a], y [C][a]
        SBV2_REQUIRE(map && a >= 1, "bad arguments");
        for (int64_t n = 0; n < a; ++n) SBV2_REQUIRE(map[n] < L, "column map outside the plane");
        DevPlane Y(C, a);
        Y.fill(true);
        DevMem dmap(map, sizeof(int) * a);
        gather_cols(X.P, static_cast<const int*>(dmap.p), Y.P, nullptr);
        HIP_CHECK(hipDeviceSynchronize());
        bad = Y.get(y, kSentinelWord);
    } else if (op == 1) {   // transpose_out: col0 = a, T = b, y [T][C]
        SBV2_REQUIRE(a >= 0 && b >= 1 && a + b <= L, "bad arguments");
        constexpr int64_t kGuard = 64;
        DevMem dy(sizeof(float) * (size_t)(b * C + kGuard));
        HIP_CHECK(hipMemset(dy.p, kCtxSentinel, sizeof(float) * (size_t)(b * C + kGuard)));
        transpose_out(X.P, (int)a, (int)b, dy.f(), nullptr);
        HIP_CHECK(hipDeviceSynchronize());
        std::vector<uint32_t> h((size_t)(b * C + kGuard));
        HIP_CHECK(hipMemcpy(h.data(), dy.p, 4 * h.size(), hipMemcpyDeviceToHost));
        std::memcpy(y, h.data(), 4 * (size_t)(b * C));
        for (int64_t e = b * C; e < b * C + kGuard; ++e) bad += h[e] != kSentinelWord;
    } else if (op == 2) {   // one window of stream_windows over the whole plane: first column a (any sign), width = b, y [C][b], mask_out [b]
        SBV2_REQUIRE(b >= 1 && mask_out && a > -(1 << 28) && a < (1 << 28), "bad arguments");
        DevPlane Y(C, b);
        Y.fill(true);
        DevMem dm((size_t)round_up((int)b, 64)), d0(sizeof(int));
        HIP_CHECK(hipMemset(dm.p, kCtxSentinel, (size_t)round_up((int)b, 64)));
        HIP_CHECK(hipMemset(d0.p, 0, sizeof(int)));
        StreamWinTable tab{};
        tab.w[0] = StreamWin{0, (int)L, (int)a, 0};
        const int h0 = 0;
        stream_windows(X.P, tab, 1, (int)b, static_cast<const int*>(d0.p), &h0, Y.P, dm.u8(), nullptr, 0, nullptr, nullptr);
        HIP_CHECK(hipDeviceSynchronize());
        bad = Y.get(y, kSentinelWord);
        std::vector<unsigned char> hm((size_t)round_up((int)b, 64));
        HIP_CHECK(hipMemcpy(hm.data(), dm.p, hm.size(), hipMemcpyDeviceToHost));
        std::memcpy(mask_out, hm.data(), (size_t)b);
        for (size_t n = (size_t)b; n < hm.size(); ++n) bad += hm[n] != kCtxSentinel;
    } else if (op == 3) {   // flip_channels
        DevPlane Y(C, L);
        Y.fill(true);
        flip_channels(X.P, Y.P, nullptr);
        HIP_CHECK(hipDeviceSynchronize());
        bad = Y.get(y, kSentinelWord);
    } else {                // swap_rows: rows 0 and 1 of a two-row plane, in place
        SBV2_REQUIRE(C == 2, "swap_rows: two rows");
        swap_rows(X.P.p, X.P.p + X.P.ld, (int)L, nullptr);
        HIP_CHECK(hipDeviceSynchronize());
        bad = X.get(y, kNanWord);
    }
    if (stray) *stray = bad;
    API_END
}

int sbv2_debug_stream_windows(int device, const float* z, int64_t C, int64_t L, const int32_t* table, int64_t W, int64_t nwin, const float* cond_vecs,
                              int64_t n_rows, int64_t cond_dim, float* z_out, uint8_t* mask_out, float* cond_out) {
    API_BEGIN
    HIP_CHECK(hipSetDevice(device));
    SBV2_REQUIRE(z && table && cond_vecs && z_out && mask_out && cond_out, "bad arguments");
    SBV2_REQUIRE(nwin >= 1 && nwin <= kStreamWinMax && W >= 1 && W < (1 << 20) && n_rows >= 1 && cond_dim >= 1 && cond_dim < (1 << 16), "bad window plan");
    StreamWinTable tab{};
    for (int64_t w = 0; w < nwin; ++w) {   // every read the launch can make lies inside the plane and the cond table
        const int32_t *t = table + 4 * w, z0 = t[0], len = t[1], first = t[2], row = t[3];
        SBV2_REQUIRE(z0 >= 0 && len >= 0 && (int64_t)z0 + len <= L && first > -(1 << 28) && first < (1 << 28) && row >= 0 && row < n_rows,
                     "window " + std::to_string(w) + " of the table lies outside the plane");
        tab.w[w] = StreamWin{z0, len, first, row};
    }
    DevPlane X(C, L);
    X.put(z, true);
    // the windows lie kGuard columns apart in one output plane; everything else holds the sentinel and must still hold it afterwards
    constexpr int kGuard = 64;
    const int pitch = round_up((int)W, 4) + kGuard;
    const int64_t Lo = kGuard + (int64_t)nwin * pitch;
    std::vector<int> start((size_t)nwin);
    for (int64_t w = 0; w < nwin; ++w) start[w] = kGuard + (int)w * pitch;
    DevPlane Y(C, Lo);
    Y.fill(true);
    const size_t ncond = (size_t)(nwin * cond_dim);
    DevMem dstart(start.data(), sizeof(int) * (size_t)nwin), dm((size_t)Lo), dc(sizeof(float) * (ncond + 2 * kGuard)),
        dv(cond_vecs, sizeof(float) * (size_t)(n_rows * cond_dim));
    HIP_CHECK(hipMemset(dm.p, kCtxSentinel, (size_t)Lo));
    HIP_CHECK(hipMemset(dc.p, kCtxSentinel, sizeof(float) * (ncond + 2 * kGuard)));
    stream_windows(X.P, tab, (int)nwin, (int)W, static_cast<const int*>(dstart.p), start.data(), Y.P, dm.u8(), dv.f(), (int)cond_dim, dc.f() + kGuard, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    std::vector<uint32_t> hy((size_t)C * Lo), hc(ncond + 2 * kGuard);
    std::vector<unsigned char> hm((size_t)Lo);
    int64_t bad = Y.get(hy.data(), kSentinelWord);
    HIP_CHECK(hipMemcpy(hm.data(), dm.p, hm.size(), hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(hc.data(), dc.p, 4 * hc.size(), hipMemcpyDeviceToHost));
    std::vector<unsigned char> inside((size_t)Lo, 0);
    for (int64_t w = 0; w < nwin; ++w) std::memset(&inside[(size_t)start[w]], 1, (size_t)W);
    for (int64_t n = 0; n < Lo; ++n) {
        if (inside[n]) continue;
        bad += hm[n] != kCtxSentinel;
        for (int64_t c = 0; c < C; ++c) bad += hy[(size_t)c * Lo + n] != kSentinelWord;
    }
    for (int i = 0; i < kGuard; ++i) bad += (hc[i] != kSentinelWord) + (hc[kGuard + ncond + i] != kSentinelWord);
    SBV2_REQUIRE(bad == 0, "stream_windows wrote " + std::to_string(bad) + " words or bytes outside its output");
    for (int64_t w = 0; w < nwin; ++w) {
        for (int64_t c = 0; c < C; ++c) std::memcpy(z_out + (size_t)((w * C + c) * W), &hy[(size_t)c * Lo + start[w]], 4 * (size_t)W);
        std::memcpy(mask_out + (size_t)(w * W), &hm[(size_t)start[w]], (size_t)W);
    }
    std::memcpy(cond_out, hc.data() + kGuard, 4 * ncond);
    API_END
}

int sbv2_debug_copy_segments(int device, const float* src, int64_t nsrc, const int64_t* table, int nseg, float* dst, int64_t ndst) {
    API_BEGIN
    HIP_CHECK(hipSetDevice(device));
    SBV2_REQUIRE(src && table && dst && nsrc >= 1 && ndst >= 1 && nseg >= 0, "bad arguments");
    for (int i = 0; i < nseg; ++i)
        SBV2_REQUIRE(table[3 * i] >= 0 && table[3 * i + 1] >= 0 && table[3 * i + 2] >= 0 && table[3 * i] + table[3 * i + 2] <= nsrc &&
                         table[3 * i + 1] + table[3 * i + 2] <= ndst,
                     "segment outside its buffer");
    DevMem ds(src, sizeof(float) * nsrc), dd(dst, sizeof(float) * ndst), dt(table, sizeof(int64_t) * 3 * nseg);   // (dst keeps what no segment covers)
    copy_segments(ds.f(), dd.f(), static_cast<const int64_t*>(dt.p), nseg, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(dst, dd.p, sizeof(float) * ndst, hipMemcpyDeviceToHost));
    API_END
}

// The gain-stage kernel of the output chain (k_pcm_gain_sig, pcm_format.hip) on host f64 signals laid back to back, signal i times gains[i],
// delivered in `encoding` (0, 1, 7, 6) -> dst (host, total samples).  The device output lies between two guard bands; a byte written there
// fails the call.
int sbv2_debug_pcm_cast(int device, const double* x, const int64_t* lens, int nsig, const double* gains, int32_t encoding, void* dst) {
    API_BEGIN
    HIP_CHECK(hipSetDevice(device));
    SBV2_REQUIRE(nsig >= 1 && lens && gains, "bad arguments");
    SBV2_REQUIRE(pcm_encoding_known(encoding), "unsupported PCM encoding " + std::to_string(encoding) + " (0 = f32, 1 = s16, 7 = G.711 mu-law, 6 = G.711 A-law)");
    int64_t total = 0;
    const std::vector<FmtSignal> sig = packed_signals(lens, nsig, &total);
    SBV2_REQUIRE(total == 0 || (x && dst), "bad arguments");
    constexpr size_t kGuard = 64;
    constexpr unsigned char kFill = 0xA5;
    const size_t nb = (size_t)total * pcm_encoding_bytes(encoding);
    DevMem dx(x, sizeof(double) * (size_t)total), dsig(sig.data(), sizeof(FmtSignal) * sig.size()), dg(gains, sizeof(double) * (size_t)nsig),
        dout(nb + 2 * kGuard);
    HIP_CHECK(hipMemset(dout.p, kFill, nb + 2 * kGuard));
    pcm_gain_signals(static_cast<const double*>(dx.p), static_cast<const FmtSignal*>(dsig.p), nsig, static_cast<const double*>(dg.p), total, encoding,
                     dout.u8() + kGuard, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    std::vector<unsigned char> h(nb + 2 * kGuard);
    HIP_CHECK(hipMemcpy(h.data(), dout.p, h.size(), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < kGuard; ++i)
        SBV2_REQUIRE(h[i] == kFill && h[kGuard + nb + i] == kFill, "the cast wrote outside its " + std::to_string(nb) + " bytes");
    if (nb) std::memcpy(dst, h.data() + kGuard, nb);
    API_END
}

// The formatting launches of the output chain (PcmFormatter::run, pcm_format.hip: k_pcm_resample and, when fmt normalises, k_pcm_gain) on a host
// table of pieces and signals.  x = nx native samples; piece q = x[pieces[3q], + pieces[3q + 2]) lying at position pieces[3q + 1] of its signal's
// timeline; signal i = outputs [sigs[4i], sigs[4i + 1]) of the timeline whose pieces are [sigs[4i + 2], sigs[4i + 3]), written back to back in
// signal order (out_off = the running sum of j1 - j0, as format_layout and the streaming replay lay them).  expose_y: the run ends at the gain
// stage's input and dst receives f64.  The tables are checked before any device call.  On the device every piece is a copy of its own between
// NaN words (a read outside a piece poisons the output) and the output lies between two guard bands; a byte written there fails the call.
// peaks (may be NULL): max |y| of each signal when fmt normalises.
int sbv2_debug_pcm_format(int device, const float* x, int64_t nx, const int64_t* pieces, int npieces, const int64_t* sigs, int nsig,
                          const sbv2_pcm_format* fmt, int expose_y, void* dst, double* peaks) {
    API_BEGIN
    const PcmFmtSpec spec = pcm_format_spec(fmt);
    SBV2_REQUIRE(nx >= 0 && npieces >= 0 && nsig >= 1 && sigs && (x || nx == 0) && (pieces || npieces == 0), "bad arguments");
    SBV2_REQUIRE(expose_y == 0 || expose_y == 1, "expose_y must be 0 or 1");
    SBV2_REQUIRE(!(expose_y && spec.normalize), "expose_y with a peak-normalised format");
    constexpr int64_t kMaxPos = (int64_t)1 << 44, kMaxTotal = (int64_t)1 << 26;   // j M + half and t0 + len stay far inside int64
    constexpr size_t kPad = 64, kGuard = 64;
    constexpr unsigned char kFill = 0xA5;
    std::vector<size_t> at((size_t)npieces);   // piece q's first word in the poisoned source
    size_t words = kPad;
    for (int q = 0; q < npieces; ++q) {
        const int64_t off = pieces[3 * q], t0 = pieces[3 * q + 1], len = pieces[3 * q + 2];
        SBV2_REQUIRE(len >= 0 && off >= 0 && off <= nx && len <= nx - off, "piece " + std::to_string(q) + " lies outside the " + std::to_string(nx) + " samples");
        SBV2_REQUIRE(t0 >= 0 && t0 <= kMaxPos, "piece " + std::to_string(q) + " starts at a position outside [0, 2^44]");
        at[q] = words;
        words += (size_t)len + kPad;
    }
    std::vector<FmtSignal> sig((size_t)nsig);
    int64_t total = 0;
    for (int i = 0; i < nsig; ++i) {
        const int64_t j0 = sigs[4 * i], j1 = sigs[4 * i + 1], p0 = sigs[4 * i + 2], p1 = sigs[4 * i + 3];
        SBV2_REQUIRE(0 <= j0 && j0 <= j1 && j1 <= kMaxPos, "signal " + std::to_string(i) + ": outputs [" + std::to_string(j0) + ", " + std::to_string(j1) +
                                                               ") are no range within [0, 2^44]");
        SBV2_REQUIRE(0 <= p0 && p0 <= p1 && p1 <= npieces, "signal " + std::to_string(i) + ": pieces [" + std::to_string(p0) + ", " + std::to_string(p1) +
                                                               ") are no range of the table's " + std::to_string(npieces));
        for (int64_t q = p0; q + 1 < p1; ++q) {
            SBV2_REQUIRE(pieces[3 * q + 1] <= pieces[3 * q + 4], "signal " + std::to_string(i) + ": its pieces are not sorted by position");
            SBV2_REQUIRE(pieces[3 * q + 1] + pieces[3 * q + 2] <= pieces[3 * q + 4], "signal " + std::to_string(i) + ": pieces " + std::to_string(q) + " and " +
                                                                                        std::to_string(q + 1) + " overlap");
        }
        sig[i] = FmtSignal{j0, j1, total, (int32_t)p0, (int32_t)p1};
        total += j1 - j0;
        SBV2_REQUIRE(total <= kMaxTotal, "more than 2^26 output samples");
    }
    SBV2_REQUIRE(total == 0 || dst, "bad arguments");
    std::vector<uint32_t> src(words, kNanWord);
    for (int q = 0; q < npieces; ++q)
        if (pieces[3 * q + 2]) std::memcpy(&src[at[q]], x + pieces[3 * q], sizeof(float) * (size_t)pieces[3 * q + 2]);
    AudioScratch r(device, src.data(), sizeof(uint32_t) * words);
    std::vector<FmtPiece> pc((size_t)npieces);
    for (int q = 0; q < npieces; ++q) pc[q] = FmtPiece{r.x.as<float>() + at[q], pieces[3 * q + 1], pieces[3 * q + 2]};
    const size_t nb = (size_t)total * (expose_y ? sizeof(double) : (size_t)spec.bytes());
    DevMem dout(nb + 2 * kGuard);
    HIP_CHECK(hipMemsetAsync(dout.p, kFill, nb + 2 * kGuard, r.s));
    PcmFormatter f;
    if (expose_y) f.run(spec, pc, sig, total, nullptr, 0, r.s, GainStage(reinterpret_cast<double*>(dout.u8() + kGuard)));
    else f.run(spec, pc, sig, total, dout.u8() + kGuard, 0, r.s);
    std::vector<unsigned char> h(nb + 2 * kGuard);
    HIP_CHECK(hipMemcpyAsync(h.data(), dout.p, h.size(), hipMemcpyDeviceToHost, r.s));
    std::vector<double> pk;
    if (peaks && spec.normalize && total) {
        pk.resize((size_t)nsig);
        HIP_CHECK(hipMemcpyAsync(pk.data(), f.peaks_device(), sizeof(double) * (size_t)nsig, hipMemcpyDeviceToHost, r.s));
    }
    HIP_CHECK(hipStreamSynchronize(r.s));
    for (size_t i = 0; i < kGuard; ++i)
        SBV2_REQUIRE(h[i] == kFill && h[kGuard + nb + i] == kFill, "the formatter wrote outside its " + std::to_string(nb) + " bytes");
    if (nb) std::memcpy(dst, h.data() + kGuard, nb);
    if (peaks && spec.normalize)
        for (int i = 0; i < nsig; ++i) peaks[i] = pk.empty() ? 0.0 : pk[i];
    API_END
}

// The level reduction of the speech marks (marks.hip) on host samples: x = n samples (encoding 0 = f32, 1 = s16, 7 / 6 = G.711 codes), segments
// [starts[i], ends[i]).
int sbv2_debug_segment_levels(int device, const void* x, int encoding, int64_t n, const int64_t* starts, const int64_t* ends, int64_t nseg, double* sumsq,
                              double* peak) {
    API_BEGIN
    HIP_CHECK(hipSetDevice(device));
    SBV2_REQUIRE(pcm_encoding_known(encoding) && n >= 0 && nseg >= 0 && (x || n == 0), "bad arguments");
    SBV2_REQUIRE(nseg == 0 || (starts && ends && sumsq && peak), "bad arguments");
    std::vector<int64_t> seg((size_t)(2 * nseg));
    for (int64_t i = 0; i < nseg; ++i) seg[2 * i] = starts[i], seg[2 * i + 1] = ends[i];
    DevMem dx(x, (size_t)n * pcm_encoding_bytes(encoding));
    Marks m;
    m.run(dx.p, encoding, n, seg.data(), nseg, nullptr);
    HIP_CHECK(hipStreamSynchronize(nullptr));
    for (int64_t i = 0; i < nseg; ++i) sumsq[i] = m.sumsq_host()[i], peak[i] = m.peak_host()[i];
    API_END
}

// The pitch estimator (Pitch, marks.hip) on host samples, finished on the host as the fetch finishes it.  Parameters and capacity are checked
// before any device call; nothing is written when the call fails.
int sbv2_debug_pitch(int device, const void* x, int encoding, int64_t n, int32_t sample_rate, sbv2_pitch* pitch, double* cmnd3, int32_t* voiced) {
    API_BEGIN
    SBV2_REQUIRE(pitch && pcm_encoding_known(encoding) && n >= 0 && (x || n == 0), "bad arguments");
    SBV2_REQUIRE(pitch->reserved == 0, "sbv2_pitch.reserved must be 0");
    const PitchSpec sp = pitch_spec(sample_rate, pitch->hop, pitch->f0_min, pitch->f0_max, pitch->threshold);
    const int64_t nf = pitch_frames(n, sp.hop);
    SBV2_REQUIRE(pitch->capacity >= nf, "pitch arrays too small: " + std::to_string(pitch->capacity) + " < " + std::to_string(nf) + " frames");
    SBV2_REQUIRE(pitch->f0, "sbv2_pitch.f0 must not be NULL");
    HIP_CHECK(hipSetDevice(device));
    DevMem dx(x, (size_t)n * pcm_encoding_bytes(encoding));
    Pitch est;
    est.run(dx.p, encoding, n, sp, nullptr);
    HIP_CHECK(hipStreamSynchronize(nullptr));
    for (int64_t f = 0; f < nf; ++f) {
        const int32_t lag = est.lag_host()[f];
        pitch_finish(sp, lag, est.voiced_host()[f], est.c3_host() + 3 * f, pitch->f0 + f, pitch->ap ? pitch->ap + f : nullptr);
        if (pitch->lag) pitch->lag[f] = lag;
        if (cmnd3) std::memcpy(cmnd3 + 3 * f, est.c3_host() + 3 * f, 3 * sizeof(double));
        if (voiced) voiced[f] = est.voiced_host()[f];
    }
    pitch->n_frames = nf;
    API_END
}

// The tracker (Track, track.hip) on host samples, or on the caller's candidate table alone.  Everything is checked before any device call;
// nothing is written when the call fails.
int sbv2_debug_pitch_track(int device, const void* x, int encoding, int64_t n, int32_t sample_rate, sbv2_pitch* pitch, const sbv2_pitch_track* track,
                           const int32_t* cand_in, const double* c3_in, int64_t nf_in, int32_t* cand_out, double* c3_out, int32_t* state_out) {
    API_BEGIN
    (void)c3_in;   // (the path depends on tau and q alone)
    SBV2_REQUIRE(track, "bad arguments");
    SBV2_REQUIRE(track->reserved[0] == 0 && track->reserved[1] == 0, "sbv2_pitch_track.reserved must be 0");
    const TrackSpec ts = track_spec(track->cand_max, track->unvoiced_cost, track->switch_cost, track->jump_cost);
    if (cand_in) {   // the path alone
        SBV2_REQUIRE(nf_in >= 0 && nf_in < (1 << 30) && (state_out || nf_in == 0), "bad arguments");
        track_check_table(cand_in, nf_in);
        HIP_CHECK(hipSetDevice(device));
        if (nf_in == 0) return 0;
        DevMem dc(cand_in, sizeof(int32_t) * kTrackRec * (size_t)nf_in);
        Track tk;
        tk.run(static_cast<const int32_t*>(dc.p), nullptr, nf_in, ts, nullptr, nullptr, nullptr, nullptr);
        std::vector<int32_t> st((size_t)nf_in);
        HIP_CHECK(hipMemcpyAsync(st.data(), tk.state_device(), sizeof(int32_t) * (size_t)nf_in, hipMemcpyDeviceToHost, nullptr));
        HIP_CHECK(hipStreamSynchronize(nullptr));
        std::memcpy(state_out, st.data(), sizeof(int32_t) * (size_t)nf_in);
        return 0;
    }
    SBV2_REQUIRE(pitch && pcm_encoding_known(encoding) && n >= 0 && (x || n == 0), "bad arguments");
    SBV2_REQUIRE(pitch->reserved == 0, "sbv2_pitch.reserved must be 0");
    const PitchSpec sp = pitch_spec(sample_rate, pitch->hop, pitch->f0_min, pitch->f0_max, pitch->threshold);
    const int64_t nf = pitch_frames(n, sp.hop);
    SBV2_REQUIRE(nf < (1 << 30), "too many pitch frames: " + std::to_string(nf) + " >= 2^30");
    SBV2_REQUIRE(pitch->capacity >= nf, "pitch arrays too small: " + std::to_string(pitch->capacity) + " < " + std::to_string(nf) + " frames");
    SBV2_REQUIRE(pitch->f0, "sbv2_pitch.f0 must not be NULL");
    HIP_CHECK(hipSetDevice(device));
    if (nf > 0) {
        const size_t F = (size_t)nf;
        DevMem dx(x, (size_t)n * pcm_encoding_bytes(encoding));
        DevMem dc3(24 * F), dlag(8 * F), dcc3(24 * kTrackCand * F), dcand(4 * kTrackRec * F);
        double* c3 = static_cast<double*>(dc3.p);
        int32_t* lag = static_cast<int32_t*>(dlag.p);
        pitch_launch(dx.p, encoding, n, sp, c3, lag, lag + nf, nullptr, ts.cand_max, static_cast<int32_t*>(dcand.p), static_cast<double*>(dcc3.p));
        Track tk;
        tk.run(static_cast<const int32_t*>(dcand.p), static_cast<const double*>(dcc3.p), nf, ts, c3, lag, lag + nf, nullptr);
        std::vector<double> hc3(3 * F), hcc3(3 * kTrackCand * F);
        std::vector<int32_t> hlag(2 * F), hcand(kTrackRec * F), hst(F);
        HIP_CHECK(hipMemcpyAsync(hc3.data(), c3, 24 * F, hipMemcpyDeviceToHost, nullptr));
        HIP_CHECK(hipMemcpyAsync(hlag.data(), lag, 8 * F, hipMemcpyDeviceToHost, nullptr));
        HIP_CHECK(hipMemcpyAsync(hcc3.data(), dcc3.p, 24 * kTrackCand * F, hipMemcpyDeviceToHost, nullptr));
        HIP_CHECK(hipMemcpyAsync(hcand.data(), dcand.p, 4 * kTrackRec * F, hipMemcpyDeviceToHost, nullptr));
        HIP_CHECK(hipMemcpyAsync(hst.data(), tk.state_device(), 4 * F, hipMemcpyDeviceToHost, nullptr));
        HIP_CHECK(hipStreamSynchronize(nullptr));
        for (int64_t f = 0; f < nf; ++f) {
            pitch_finish(sp, hlag[f], hlag[F + f], hc3.data() + 3 * f, pitch->f0 + f, pitch->ap ? pitch->ap + f : nullptr);
            if (pitch->lag) pitch->lag[f] = hlag[f];
        }
        if (cand_out) std::memcpy(cand_out, hcand.data(), 4 * kTrackRec * F);
        if (c3_out) std::memcpy(c3_out, hcc3.data(), 24 * kTrackCand * F);
        if (state_out) std::memcpy(state_out, hst.data(), 4 * F);
    }
    pitch->n_frames = nf;
    API_END
}

// The shifter (Voice, voice.hip) on host rows laid back to back, always through its kernels; everything is checked before any device call.
// tp (with tok_counts / tok_ends): the per-token edits, through k_voice_marks_tok whatever the values are.
// fmnt: the formant scale, through k_voice_gather_fmt whatever the value is.
static int debug_voice(int device, const float* x, const int64_t* lens, int nrows, int32_t sample_rate, const sbv2_voice* voice,
                       const double* period_in, const int32_t* voiced_in, const int64_t* tok_counts, const int64_t* tok_ends,
                       const sbv2_token_pitch* tp, double* period_out, int32_t* voiced_out, int32_t* ta, int32_t* ts, int32_t* map, int64_t* n_marks,
                       float* y, double* ratio_out, const sbv2_formant* fmnt = nullptr) {
    API_BEGIN
    SBV2_REQUIRE(voice && nrows >= 0 && (nrows == 0 || lens), "bad arguments");
    SBV2_REQUIRE(voice->reserved == 0, "sbv2_voice.reserved must be 0");
    const VoiceSpec sp = voice_spec(sample_rate, voice->pitch_scale, voice->intonation_scale, voice->hop, voice->f0_min, voice->f0_max, voice->threshold);
    SBV2_REQUIRE(!period_in == !voiced_in, "period_in and voiced_in are given together or not at all");
    SBV2_REQUIRE((!ta == !ts) && (!ta == !map) && (!ta == !n_marks), "ta, ts, map and n_marks are given together or not at all");
    std::vector<VoiceRow> rows((size_t)nrows);
    int64_t total = 0;
    for (int i = 0; i < nrows; ++i) {
        SBV2_REQUIRE(lens[i] >= 0 && lens[i] < (1 << 30), "bad length of row " + std::to_string(i));
        rows[i] = VoiceRow{total, lens[i]};
        total += lens[i];
    }
    SBV2_REQUIRE(total == 0 || (x && y), "bad arguments");
    FormantSpec fs;
    if (fmnt) fs = formant_spec(fmnt->formant_scale, fmnt->reserved, sp);
    VoiceTokens vt{};
    if (tp) {
        SBV2_REQUIRE(nrows == 0 || tok_counts, "bad arguments");
        SBV2_REQUIRE(tp->reserved == 0, "sbv2_token_pitch.reserved must be 0");
        int64_t n_tok = 0;
        for (int i = 0; i < nrows; ++i) {
            SBV2_REQUIRE(tok_counts[i] >= 0 && tok_counts[i] < (1 << 30), "bad token count of row " + std::to_string(i));
            n_tok += tok_counts[i];
        }
        SBV2_REQUIRE(tp->n_tokens == n_tok, "sbv2_token_pitch.n_tokens is " + std::to_string(tp->n_tokens) + " but the listed rows have " +
                                                std::to_string(n_tok) + " tokens");
        SBV2_REQUIRE(n_tok == 0 || (tp->value && tok_ends), "sbv2_token_pitch.value must not be NULL");
        voice_tokens_check(tp->value, n_tok, tp->kind, tp->smooth, sp);
        for (int i = 0, e = 0; i < nrows; ++i)
            for (int64_t t = 0, prev = 0; t < tok_counts[i]; ++t, ++e) {
                SBV2_REQUIRE(tok_ends[e] >= prev, "the token ends of row " + std::to_string(i) + " must ascend from 0");
                prev = tok_ends[e];
            }
        vt = VoiceTokens{tok_counts, tok_ends, tp->value, tp->kind, tp->smooth};
    }
    HIP_CHECK(hipSetDevice(device));
    DevMem dx(x, sizeof(float) * (size_t)total);
    Voice v;
    const float* dy = v.run(dx.f(), total, rows.data(), nrows, sp, nullptr, period_in, voiced_in, nullptr, tp ? &vt : nullptr, fmnt ? &fs : nullptr);
    v.results_to_host(nullptr);
    HIP_CHECK(hipStreamSynchronize(nullptr));
    for (int i = 0; i < nrows; ++i) SBV2_REQUIRE(v.status(i) == 0, "internal: the shifter found more marks than it planned for in row " + std::to_string(i));
    if (total) HIP_CHECK(hipMemcpy(y, dy, sizeof(float) * (size_t)total, hipMemcpyDeviceToHost));
    if (period_out) std::memcpy(period_out, v.period_host(), sizeof(double) * (size_t)v.n_frames());
    if (voiced_out) std::memcpy(voiced_out, v.voiced_host(), sizeof(int32_t) * (size_t)v.n_frames());
    if (ta) {
        int64_t at = 0;   // row i's lists start at sum of (lens + 1) of the rows before it
        for (int i = 0; i < nrows; ++i) {
            const int64_t na = v.n_a(i), ns = v.n_s(i);
            SBV2_REQUIRE(na <= lens[i] + 1 && ns <= lens[i] + 1, "internal: more marks than samples");
            std::memcpy(ta + at, v.ta_host(i), sizeof(int32_t) * (size_t)na);
            std::memcpy(ts + at, v.ts_host(i), sizeof(int32_t) * (size_t)ns);
            std::memcpy(map + at, v.map_host(i), sizeof(int32_t) * (size_t)ns);
            n_marks[2 * i] = na;
            n_marks[2 * i + 1] = ns;
            at += lens[i] + 1;
        }
    }
    if (tp) {
        if (ratio_out) std::memcpy(ratio_out, v.ratio_host(), sizeof(double) * (size_t)v.n_frames());
        if (tp->applied) std::memcpy(tp->applied, v.applied_host(), sizeof(double) * (size_t)v.n_tokens());
        if (tp->src_f0) std::memcpy(tp->src_f0, v.src_f0_host(), sizeof(double) * (size_t)v.n_tokens());
    }
    API_END
}
int sbv2_debug_voice_shift(int device, const float* x, const int64_t* lens, int nrows, int32_t sample_rate, const sbv2_voice* voice,
                           const double* period_in, const int32_t* voiced_in, double* period_out, int32_t* voiced_out, int32_t* ta, int32_t* ts,
                           int32_t* map, int64_t* n_marks, float* y) {
    return debug_voice(device, x, lens, nrows, sample_rate, voice, period_in, voiced_in, nullptr, nullptr, nullptr, period_out, voiced_out, ta, ts, map,
                       n_marks, y, nullptr);
}
int sbv2_debug_voice_tokens(int device, const float* x, const int64_t* lens, int nrows, int32_t sample_rate, const sbv2_voice* voice,
                            const double* period_in, const int32_t* voiced_in, const int64_t* tok_counts, const int64_t* tok_ends,
                            const sbv2_token_pitch* token_pitch, double* period_out, int32_t* voiced_out, int32_t* ta, int32_t* ts, int32_t* map,
                            int64_t* n_marks, float* y, double* ratio_out) {
    if (!token_pitch) {
        set_last_error("bad arguments");
        return 1;
    }
    return debug_voice(device, x, lens, nrows, sample_rate, voice, period_in, voiced_in, tok_counts, tok_ends, token_pitch, period_out, voiced_out, ta,
                       ts, map, n_marks, y, ratio_out);
}
int sbv2_debug_voice_formant(int device, const float* x, const int64_t* lens, int nrows, int32_t sample_rate, const sbv2_voice* voice,
                             const sbv2_formant* formant, const double* period_in, const int32_t* voiced_in, double* period_out,
                             int32_t* voiced_out, int32_t* ta, int32_t* ts, int32_t* map, int64_t* n_marks, float* y) {
    if (!formant) {
        set_last_error("bad arguments");
        return 1;
    }
    return debug_voice(device, x, lens, nrows, sample_rate, voice, period_in, voiced_in, nullptr, nullptr, nullptr, period_out, voiced_out, ta, ts, map,
                       n_marks, y, nullptr, formant);
}

// The fed shifter (StreamVoice, voice.hip) on its own: one row x cut at cuts[ncuts] into ncuts + 1 pushes, each handed a COPY of its piece
// between two guards of a fill pattern (the stage keeps the fed samples itself; nothing in front of or behind a piece is its to read).  The
// shifted samples each push made final go to y back to back.  Everything is checked before any device call.
int sbv2_debug_voice_stream(int device, const float* x, int64_t n, const int64_t* cuts, int ncuts, int32_t sample_rate, const sbv2_stream_voice* v,
                            const double* period_in, const int32_t* voiced_in, float* y, int64_t* out_per_push) {
    API_BEGIN
    SBV2_REQUIRE(v && out_per_push && n >= 0 && n < (1 << 30) && ncuts >= 0 && (ncuts == 0 || cuts) && (n == 0 || (x && y)), "bad arguments");
    SBV2_REQUIRE(v->voice.reserved == 0, "sbv2_voice.reserved must be 0");
    SBV2_REQUIRE(!period_in == !voiced_in, "period_in and voiced_in are given together or not at all");
    const StreamVoiceSpec sp = stream_voice_spec(sample_rate, v->voice.pitch_scale, v->voice.intonation_scale, v->voice.hop, v->voice.f0_min,
                                                 v->voice.f0_max, v->voice.threshold, v->formant_scale, v->pivot_hz, 1, v->reserved[0], v->reserved[1]);
    std::vector<int64_t> edge(1, 0);
    int64_t longest = 0;
    for (int i = 0; i < ncuts; ++i) {
        SBV2_REQUIRE(cuts[i] >= edge.back() && cuts[i] <= n, "cuts must ascend within [0, n]");
        edge.push_back(cuts[i]);
    }
    edge.push_back(n);
    for (size_t i = 0; i + 1 < edge.size(); ++i) longest = std::max(longest, edge[i + 1] - edge[i]);
    const size_t guard = 4096;
    AudioScratch r(device, x, sizeof(float) * (size_t)n);
    DeviceBuffer piece;
    char* pc = static_cast<char*>(piece.reserve(sizeof(float) * (size_t)longest + 2 * guard, r.s));
    HIP_CHECK(hipMemsetAsync(pc, 0x5A, sizeof(float) * (size_t)longest + 2 * guard, r.s));
    const VoiceRow row{0, n};
    StreamVoice sv;
    sv.begin(sp, &row, 1, n, r.s, period_in, voiced_in);
    std::vector<float> out((size_t)std::max<int64_t>(n, 1));
    int64_t at = 0;
    for (int i = 0; i <= ncuts; ++i) {
        const int64_t len = edge[i + 1] - edge[i];
        // (stream order: the previous push has copied the piece before this copy overwrites it)
        if (len) HIP_CHECK(hipMemcpyAsync(pc + guard, r.x.as<float>() + edge[i], sizeof(float) * (size_t)len, hipMemcpyDeviceToDevice, r.s));
        const int64_t fin = sv.push(0, reinterpret_cast<const float*>(pc + guard), len, r.s);
        out_per_push[i] = fin - at;
        // the samples this push made final, read before a later push could write them again (it never does)
        if (fin > at) HIP_CHECK(hipMemcpyAsync(out.data() + at, sv.out(0) + at, sizeof(float) * (size_t)(fin - at), hipMemcpyDeviceToHost, r.s));
        at = fin;
    }
    sv.status_to_host(r.s);
    HIP_CHECK(hipStreamSynchronize(r.s));
    SBV2_REQUIRE(at == n, "internal: the fed shifter made " + std::to_string(at) + " of " + std::to_string(n) + " samples final");
    SBV2_REQUIRE(sv.status(0) == 0, "internal: the shifter found more marks than it planned for");
    if (n) std::memcpy(y, out.data(), sizeof(float) * (size_t)n);
    API_END
}

// The fed level reduction (StreamLevels, marks.hip) on its own: x cut at cuts[ncuts] into ncuts + 1 pushes, each handed the samples of its
// piece only.  Segments, envelope and cuts are checked before any device call.
int sbv2_debug_stream_levels(int device, const void* x, int encoding, int64_t n, const int64_t* cuts, int ncuts, const int64_t* starts,
                             const int64_t* ends, int64_t nseg, int32_t env_hop, double* seg_sumsq, double* seg_peak, double* env_sumsq,
                             double* env_peak, int64_t* seg_per_push, int64_t* env_per_push) {
    API_BEGIN
    SBV2_REQUIRE(pcm_encoding_known(encoding) && n >= 0 && nseg >= 0 && ncuts >= 0 && (x || n == 0) && (ncuts == 0 || cuts), "bad arguments");
    SBV2_REQUIRE(nseg == 0 || (starts && ends && seg_sumsq && seg_peak), "bad arguments");
    SBV2_REQUIRE(seg_per_push && env_per_push, "bad arguments");
    std::vector<int64_t> seg((size_t)(2 * nseg));
    for (int64_t i = 0; i < nseg; ++i) seg[2 * i] = starts[i], seg[2 * i + 1] = ends[i];
    StreamLevels::check(seg.data(), nseg, env_hop, n);
    const int64_t nenv = StreamLevels::env_frames(env_hop, n);
    SBV2_REQUIRE(nenv == 0 || (env_sumsq && env_peak), "bad arguments");
    std::vector<int64_t> edge(1, 0);
    for (int i = 0; i < ncuts; ++i) {
        SBV2_REQUIRE(cuts[i] >= edge.back() && cuts[i] <= n, "cuts must ascend within [0, n]");
        edge.push_back(cuts[i]);
    }
    edge.push_back(n);
    const size_t esz = pcm_encoding_bytes(encoding);
    AudioScratch r(device, x, (size_t)n * esz);
    StreamLevels lv;
    lv.begin(seg.data(), nseg, env_hop, n, r.s);
    for (int i = 0; i <= ncuts; ++i) {
        const StreamLevels::Done d = lv.push(r.x.as<char>() + (size_t)edge[i] * esz, encoding, edge[i], edge[i + 1] - edge[i], r.s);
        seg_per_push[i] = d.tok;
        env_per_push[i] = d.env;
    }
    HIP_CHECK(hipStreamSynchronize(r.s));
    for (int64_t i = 0; i < nseg; ++i) seg_sumsq[i] = lv.tok_host()[2 * i], seg_peak[i] = lv.tok_host()[2 * i + 1];
    for (int64_t i = 0; i < nenv; ++i) env_sumsq[i] = lv.env_host()[2 * i], env_peak[i] = lv.env_host()[2 * i + 1];
    API_END
}

// The fed pitch estimator (StreamPitch, marks.hip) on its own: x cut at cuts[ncuts] into ncuts + 1 pushes.  Each push is handed a COPY of its
// piece, between two guards of a fill pattern, never a pointer into the whole signal: a kernel that looked for earlier samples in front of x
// instead of in its carry would not find them.  Parameters, capacity and cuts are checked before any device call.
int sbv2_debug_stream_pitch(int device, const void* x, int encoding, int64_t n, const int64_t* cuts, int ncuts, int32_t sample_rate, sbv2_pitch* pitch,
                            double* cmnd3, int32_t* voiced, int64_t* per_push) {
    API_BEGIN
    SBV2_REQUIRE(pitch && per_push && pcm_encoding_known(encoding) && n >= 0 && ncuts >= 0 && (x || n == 0) && (ncuts == 0 || cuts), "bad arguments");
    SBV2_REQUIRE(pitch->reserved == 0, "sbv2_pitch.reserved must be 0");
    const PitchSpec sp = pitch_spec(sample_rate, pitch->hop, pitch->f0_min, pitch->f0_max, pitch->threshold);
    StreamPitch::check(sp, n);
    const int64_t nf = pitch_frames(n, sp.hop);
    SBV2_REQUIRE(pitch->capacity >= nf, "pitch arrays too small: " + std::to_string(pitch->capacity) + " < " + std::to_string(nf) + " frames");
    SBV2_REQUIRE(pitch->f0, "sbv2_pitch.f0 must not be NULL");
    std::vector<int64_t> edge(1, 0);
    int64_t longest = 0;
    for (int i = 0; i < ncuts; ++i) {
        SBV2_REQUIRE(cuts[i] >= edge.back() && cuts[i] <= n, "cuts must ascend within [0, n]");
        edge.push_back(cuts[i]);
    }
    edge.push_back(n);
    for (size_t i = 0; i + 1 < edge.size(); ++i) longest = std::max(longest, edge[i + 1] - edge[i]);
    const size_t esz = pcm_encoding_bytes(encoding), guard = 4096;
    AudioScratch r(device, x, (size_t)n * esz);
    DeviceBuffer piece;
    char* pc = static_cast<char*>(piece.reserve((size_t)longest * esz + 2 * guard, (size_t)longest * esz + 2 * guard, r.s));
    HIP_CHECK(hipMemsetAsync(pc, 0x5A, (size_t)longest * esz + 2 * guard, r.s));
    StreamPitch est;
    est.begin(sp, encoding, n, r.s);
    for (int i = 0; i <= ncuts; ++i) {
        const int64_t len = edge[i + 1] - edge[i];
        // (stream order: the previous push's launch has read the piece before this copy overwrites it)
        if (len) HIP_CHECK(hipMemcpyAsync(pc + guard, r.x.as<char>() + (size_t)edge[i] * esz, (size_t)len * esz, hipMemcpyDeviceToDevice, r.s));
        per_push[i] = est.push(pc + guard, edge[i], len, r.s);
    }
    HIP_CHECK(hipStreamSynchronize(r.s));
    SBV2_REQUIRE(est.complete(est.fed()) == nf, "internal: frames left incomplete after the last push");
    for (int64_t f = 0; f < nf; ++f) {
        const int32_t lag = est.lag_host(f);
        pitch_finish(sp, lag, est.voiced_host(f), est.c3_host(f), pitch->f0 + f, pitch->ap ? pitch->ap + f : nullptr);
        if (pitch->lag) pitch->lag[f] = lag;
        if (cmnd3) std::memcpy(cmnd3 + 3 * f, est.c3_host(f), 3 * sizeof(double));
        if (voiced) voiced[f] = est.voiced_host(f);
    }
    pitch->n_frames = nf;
    API_END
}

// ---- the repeated-launch hooks (run_repeated above): operands as in the one-launch hook of the same kernel, two inputs xa / xb, ya / yb = the first result of
// each; prev (may be null) = what every repetition accumulates onto
int sbv2_debug_repeat_respair(int device, const float* xa, const float* xb, const float* w1, const float* w2, const float* b1, const float* b2, int64_t C,
                              int64_t N, int64_t k, int64_t dilation, const uint8_t* mask, int64_t mask_div, float beta, const float* prev, int variant,
                              int reps, int neighbour, int flip_at, int64_t flip_word, float* ya, float* yb, int64_t* mismatch, int64_t* first_bad) {
    API_BEGIN
    HIP_CHECK(hipSetDevice(device));
    SBV2_REQUIRE(xa && xb && w1 && w2 && b1 && b2 && ya && yb && (C == 16 || C == 32 || C == 64) && N >= 1 && N * C < ((int64_t)1 << 31) && k >= 1 &&
                     k <= kMaxTaps && (k & 1) && mask_div >= 1 && (mask_div & (mask_div - 1)) == 0 && variant >= 1 && variant <= 3,
                 "bad arguments");
    Blob b = one_conv_blob(w1, b1, {C, C, k}, C);
    WeightStore ws(b);
    ClConv c1 = pack_decoder_conv(ws, w1, (int)C, (int)C, (int)k, 1, b1);
    ClConv c2 = pack_decoder_conv(ws, w2, (int)C, (int)C, (int)k, 1, b2);
    const size_t bytes = sizeof(float) * N * C;
    DevMem dxa(xa, bytes), dxb(xb, bytes), dya(bytes), dyb(bytes), ra(bytes), rb(bytes), init(prev, prev ? bytes : 0), nan(prev ? 0 : bytes);
    if (!prev) fill_nan(nan, bytes);
    DevMem dm(mask, mask ? (size_t)((N + mask_div - 1) / mask_div) : 0);
    int shift = 0;
    while ((1 << shift) < mask_div) ++shift;
    ResPairParams rp = step_params(c1, c2, (int)k, (int)dilation, 1, (int)C, N, mask ? dm.u8() : nullptr, (int)mask_div, shift);
    rp.beta = beta;
    rp.accumulate = prev != nullptr;
    // 1 = the default dispatch's kernel, 2 = respair_clx, 3 = respair_x16 (launch_respair_x16 refuses what that kernel does not take: no silent fall-back)
    const BranchKernel kern = variant == 3 ? BranchKernel::respair_x16 : (variant == 2 ? BranchKernel::respair_clx : respair_default(rp));
    const float* X[2] = {dxa.f(), dxb.f()};
    const std::vector<RepRegion> regs{{{dya.p, dyb.p}, {ra.p, rb.p}, prev ? init.p : nan.p, (size_t)N * C}};
    run_repeated(regs, RepOpts{reps, neighbour, flip_at, flip_word},
                 [&](int which, hipStream_t s) {
                     ResPairParams p = rp;
                     p.X = X[which];
                     p.Y = static_cast<float*>(regs[0].out[which]);
                     launch_respair(p, kern, s);
                 },
                 mismatch, first_bad);
    HIP_CHECK(hipMemcpy(ya, ra.p, bytes, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(yb, rb.p, bytes, hipMemcpyDeviceToHost));
    API_END
}

int sbv2_debug_repeat_resbranch(int device, const float* xa, const float* xb, const float* w, const float* bias, int64_t C, int64_t N, int64_t k,
                                const int64_t* dilations, const uint8_t* mask, int64_t mask_div, float beta, const float* prev, int reps, int neighbour,
                                int flip_at, int64_t flip_word, float* ya, float* yb, int64_t* mismatch, int64_t* first_bad) {
    API_BEGIN
    HIP_CHECK(hipSetDevice(device));
    SBV2_REQUIRE(xa && xb && w && bias && ya && yb && dilations && (C == 16 || C == 32 || C == 64 || C == 128) && N >= 1 && N * C < ((int64_t)1 << 31) &&
                     k >= 1 && k <= kMaxTaps && (k & 1) && mask_div >= 1 && (mask_div & (mask_div - 1)) == 0,
                 "bad arguments");
    const size_t wsz = (size_t)C * C * k;
    Blob b = one_conv_blob(w, bias, {C, C, k}, C);
    WeightStore ws(b);
    std::vector<ClConv> c1, c2;   // conv1 / conv2 of each step
    std::vector<int> dil;
    for (int q = 0; q < kResBranchSteps; ++q) {
        c1.push_back(pack_decoder_conv(ws, w + 2 * q * wsz, (int)C, (int)C, (int)k, 1, bias + (size_t)2 * q * C));
        c2.push_back(pack_decoder_conv(ws, w + (2 * q + 1) * wsz, (int)C, (int)C, (int)k, 1, bias + (size_t)(2 * q + 1) * C));
        dil.push_back((int)dilations[q]);
    }
    const size_t bytes = sizeof(float) * N * C;
    DevMem dxa(xa, bytes), dxb(xb, bytes), dya(bytes), dyb(bytes), ra(bytes), rb(bytes), init(prev, prev ? bytes : 0), nan(prev ? 0 : bytes);
    if (!prev) fill_nan(nan, bytes);
    DevMem dm(mask, mask ? (size_t)((N + mask_div - 1) / mask_div) : 0);
    int shift = 0;
    while ((1 << shift) < mask_div) ++shift;
    ResBranchParams rb0 = branch_params(c1, c2, dil, (int)k, (int)C, N, mask ? dm.u8() : nullptr, shift);
    rb0.beta = beta;
    rb0.accumulate = prev != nullptr;
    const float* X[2] = {dxa.f(), dxb.f()};
    const std::vector<RepRegion> regs{{{dya.p, dyb.p}, {ra.p, rb.p}, prev ? init.p : nan.p, (size_t)N * C}};
    run_repeated(regs, RepOpts{reps, neighbour, flip_at, flip_word},
                 [&](int which, hipStream_t s) {
                     ResBranchParams p = rb0;
                     p.X = X[which];
                     p.Y = static_cast<float*>(regs[0].out[which]);
                     launch_resbranch(p, s);
                 },
                 mismatch, first_bad);
    HIP_CHECK(hipMemcpy(ya, ra.p, bytes, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(yb, rb.p, bytes, hipMemcpyDeviceToHost));
    API_END
}

// x / res / y channel-major [C][L] as sbv2_debug_conv1d_clx; want_ys: the launch also writes the bf16 parts of lrelu(y, 0.1), which are compared word by word
// (halo rows included) behind the f32 plane's L * cout words, and ysa / ysb return hi + lo of the first results
int sbv2_debug_repeat_conv1d_clx(int device, const float* xa, const float* xb, const float* w, const float* bias, const float* res, int64_t cin, int64_t cout,
                                 int64_t k, int64_t L, int64_t dilation, float pre_slope, float beta, int want_ys, int reps, int neighbour, int flip_at,
                                 int64_t flip_word, float* ya, float* yb, float* ysa, float* ysb, int64_t* mismatch, int64_t* first_bad) {
    API_BEGIN
    HIP_CHECK(hipSetDevice(device));
    SBV2_REQUIRE(xa && xb && w && ya && yb && (!want_ys || (ysa && ysb)) && L >= 1 && L * std::max(cin, cout) < ((int64_t)1 << 31), "bad arguments");
    Blob b = one_conv_blob(w, bias, {cout, cin, k}, cout);
    WeightStore ws(b);
    ClConv c = pack_decoder_conv(ws, w, (int)cout, (int)cin, (int)k, 1, bias);
    DevMem dr = res ? upload_cl(res, cout, L) : DevMem(0);
    ClxInputs in(xa, xb, cin, L, pre_slope);
    ConvClxParams p;
    p.W = c.wx;
    p.nmt = c.nmt;
    p.M = (int)cout;
    p.N = (int)L;
    p.K = (int)cin;
    p.ntaps = (int)k;
    p.shift0 = (int)(-dilation * (k - 1) / 2);
    p.shift_step = (int)dilation;
    p.ldy = (int)cout;
    p.ys_slope = 0.1f;
    p.bias = c.bias;
    if (res) {
        p.R = dr.f();
        p.ldr = (int)cout;
    }
    p.beta = beta;
    repeat_clx(p, in, cout, L, want_ys, RepOpts{reps, neighbour, flip_at, flip_word}, ya, yb, ysa, ysb, mismatch, first_bad);
    API_END
}

// the phased transposed convolution of the wide decoder stages, operands as sbv2_debug_conv_transpose1d_clx; y [cout][L * stride]
int sbv2_debug_repeat_conv_transpose1d_clx(int device, const float* xa, const float* xb, const float* w, const float* bias, int64_t cin, int64_t cout, int64_t k,
                                           int64_t L, int64_t stride, float pre_slope, const uint8_t* mask, int64_t mask_div, int want_ys, int reps,
                                           int neighbour, int flip_at, int64_t flip_word, float* ya, float* yb, float* ysa, float* ysb, int64_t* mismatch,
                                           int64_t* first_bad) {
    API_BEGIN
    HIP_CHECK(hipSetDevice(device));
    SBV2_REQUIRE(xa && xb && w && bias && ya && yb && (!want_ys || (ysa && ysb)) && mask_div >= 1 && (mask_div & (mask_div - 1)) == 0 && L >= 1 && stride >= 1 &&
                     L * stride * cout < ((int64_t)1 << 31) && L * cin < ((int64_t)1 << 31),
                 "bad arguments");
    Blob b = one_conv_blob(w, bias, {cin, cout, k}, cout);
    WeightStore ws(b);
    ClUpX u = build_upx(ws, w, bias, (int)cin, (int)cout, (int)k, (int)stride, /*parts_out=*/want_ys != 0);
    SBV2_REQUIRE(u.wx, "shape not supported by the phased conv_clx transposed convolution");
    ClxInputs in(xa, xb, cin, L, pre_slope);
    DevMem dm(mask, mask ? (size_t)((L + mask_div - 1) / mask_div) : 0);
    int shift = 0;
    while ((1 << shift) < mask_div) ++shift;
    ConvClxParams p;
    p.W = u.wx;
    p.nmt = u.M / 32;
    p.M = u.M;
    p.N = (int)L;
    p.K = (int)cin;
    p.ntaps = u.ntaps;
    p.shift0 = u.shift0;
    p.shift_step = -1;
    p.ldy = (int)cout;
    p.ys_slope = 0.1f;
    p.bias = u.bias;
    p.mask = mask ? dm.u8() : nullptr;   // indexed by the INPUT position >> shift
    p.mask_shift = shift;
    p.out_stride = (int)stride;
    p.phase_rows = (int)cout;
    p.phase_group = u.group;
    for (int q = 0; q < kMaxPhases; ++q) {
        p.phase_off[q] = u.phase_off[q];
        p.phase_tap0[q] = u.phase_tap0[q];
    }
    repeat_clx(p, in, cout, L * stride, want_ys, RepOpts{reps, neighbour, flip_at, flip_word}, ya, yb, ysa, ysb, mismatch, first_bad);
    API_END
}

// y[M][N] = w[M][K] x[K][N] + bias (+ res) through gemm_bfs.hip as conv_bfs launches it (parts code as sbv2_debug_gemm_bfs), with the K-split scratch of the
// other gemm_bfs hooks; split_out: the parts copy is written and compared too (ysa / ysb = the parts' sum).  Words: the f32 plane [M][round_up(N, 64)], pad
// columns included, then the parts planes.
int sbv2_debug_repeat_gemm_bfs(int device, const float* xa, const float* xb, const float* w, const float* bias, const float* res, int64_t M, int64_t N, int64_t K,
                               int parts, int split_out, int reps, int neighbour, int flip_at, int64_t flip_word, float* ya, float* yb, float* ysa, float* ysb,
                               int64_t* mismatch, int64_t* first_bad) {
    API_BEGIN
    HIP_CHECK(hipSetDevice(device));
    SBV2_REQUIRE((parts == 2 || parts == 3 || parts == kPartsF16x3) && (split_out == 0 || split_out == parts) && xa && xb && w && ya && yb &&
                     (!split_out || (ysa && ysb)) && M >= 1 && N >= 4 && (N & 3) == 0 && (K & 15) == 0 && M * (N + 64) < ((int64_t)1 << 30),
                 "bad arguments");
    Blob b = one_conv_blob(w, bias, {M, K, 1}, M);
    WeightStore ws(b);
    ws.set_bfs_parts(parts);
    PackedConv pc = ws.conv("c");
    const int ld = round_up((int)N, 64), np_ = split_nplanes(parts);
    const size_t ybytes = sizeof(float) * M * ld, xbytes = sizeof(float) * K * ld, xs_bytes = (size_t)np_ * K * ld * 2 + 64,
                 ys_bytes = split_out ? (size_t)np_ * M * ld * 2 : 0;
    DevMem dx(xbytes), dr(res ? ybytes : 0), dxsa(xs_bytes), dxsb(xs_bytes), dya(ybytes), dyb(ybytes), ra(ybytes), rb(ybytes), nan(ybytes), dysa(ys_bytes),
        dysb(ys_bytes), rsa(ys_bytes), rsb(ys_bytes), ysnan(ys_bytes);
    fill_nan(nan, ybytes);
    if (split_out) fill_nan(ysnan, ys_bytes);
    Plane X{dx.f(), (int)K, (int)N, ld}, R{dr.f(), (int)M, (int)N, ld};
    if (res) {
        HIP_CHECK(hipMemset(R.p, 0, ybytes));
        HIP_CHECK(hipMemcpy2D(R.p, sizeof(float) * ld, res, sizeof(float) * N, sizeof(float) * N, M, hipMemcpyHostToDevice));
    }
    SplitPlanes xs[2], ys[2];
    for (int i = 0; i < 2; ++i) {
        HIP_CHECK(hipMemset(X.p, 0, xbytes));
        HIP_CHECK(hipMemcpy2D(X.p, sizeof(float) * ld, i ? xb : xa, sizeof(float) * N, sizeof(float) * N, K, hipMemcpyHostToDevice));
        xs[i].p = i ? dxsb.p : dxsa.p;
        xs[i].parts = np_;
        xs[i].f16 = parts == kPartsF16x3;
        xs[i].sat = xs[i].f16 ? f16x3_sat_counter() : nullptr;
        xs[i].C = (int)K;
        xs[i].L = (int)N;
        xs[i].ld = ld;
        xs[i].pstride = (int64_t)K * ld;
        split_planes(X, xs[i], nullptr);
        HIP_CHECK(hipDeviceSynchronize());
        ys[i] = xs[i];
        ys[i].p = i ? dysb.p : dysa.p;
        ys[i].sat = nullptr;
        ys[i].C = (int)M;
        ys[i].pstride = (int64_t)M * ld;
    }
    constexpr size_t kWs = (size_t)48 << 20;   // (as BertModel::kSkWsBytes / kSkCounters)
    DevMem dsk(kWs + 1024 * sizeof(float));
    HIP_CHECK(hipMemset(dsk.p, 0, kWs + 1024 * sizeof(float)));
    BfsSplitK sk;
    sk.ws = dsk.f();
    sk.ws_bytes = kWs;
    sk.counters = reinterpret_cast<unsigned*>(dsk.f() + (kWs / sizeof(float)));
    sk.ncounters = 1024;
    std::vector<RepRegion> regs{{{dya.p, dyb.p}, {ra.p, rb.p}, nan.p, (size_t)M * ld}};
    if (split_out) regs.push_back(RepRegion{{dysa.p, dysb.p}, {rsa.p, rsb.p}, ysnan.p, ys_bytes / 4});
    run_repeated(regs, RepOpts{reps, neighbour, flip_at, flip_word},
                 [&](int which, hipStream_t s) {
                     Plane Y{static_cast<float*>(regs[0].out[which]), (int)M, (int)N, ld};
                     conv_bfs(pc, xs[which], &Y, split_out ? &ys[which] : nullptr, nullptr, 1, s, ACT_NONE, res ? &R : nullptr, 1.0f, 1.0f, -1, 0, &sk);
                 },
                 mismatch, first_bad);
    for (int i = 0; i < 2; ++i) {
        HIP_CHECK(hipMemcpy2D(i ? yb : ya, sizeof(float) * N, i ? rb.p : ra.p, sizeof(float) * ld, sizeof(float) * N, M, hipMemcpyDeviceToHost));
        if (!split_out) continue;
        std::vector<uint16_t> hs(ys_bytes / 2);
        HIP_CHECK(hipMemcpy(hs.data(), i ? rsb.p : rsa.p, ys_bytes, hipMemcpyDeviceToHost));
        float* out = i ? ysb : ysa;
        for (int64_t m = 0; m < M; ++m)
            for (int64_t n = 0; n < N; ++n) {
                if (parts == kPartsF16x3) {
                    _Float16 hi, lo;
                    memcpy(&hi, &hs[(size_t)m * ld + n], 2);
                    memcpy(&lo, &hs[((size_t)M + m) * ld + n], 2);
                    out[(size_t)m * N + n] = (float)hi + (float)lo * (1.0f / kF16LoScale);
                    continue;
                }
                float acc = 0.f;
                for (int pp = np_ - 1; pp >= 0; --pp) {
                    const uint32_t u = (uint32_t)hs[((size_t)pp * M + m) * ld + n] << 16;
                    float f;
                    memcpy(&f, &u, 4);
                    acc += f;
                }
                out[(size_t)m * N + n] = acc;
            }
    }
    API_END
}

// k_vits_flash_x3q on the flow's frame layout as sbv2_debug_vits_attention (variant 4 / 5) builds it, the launcher choosing the 4- or 8-wave shape by the grid
// as in the model; q / k / v packed [heads * dk][sum lens], two sets; ctx starts every repetition as zeros (as the models clear it).  Words: the ctx plane at
// its device pitch [heads * dk][ld], gaps and pad columns included.
int sbv2_debug_repeat_vits_attention(int device, const float* qa, const float* ka, const float* va, const float* qb, const float* kb, const float* vb,
                                     const float* erk, const float* erv, const int64_t* lens, int nutt, int64_t heads, int64_t dk, int64_t window, int reps,
                                     int neighbour, int flip_at, int64_t flip_word, float* ctxa, float* ctxb, int64_t* ld_out, int64_t* mismatch,
                                     int64_t* first_bad) {
    API_BEGIN
    HIP_CHECK(hipSetDevice(device));
    SBV2_REQUIRE(qa && ka && va && qb && kb && vb && erk && erv && lens && ctxa && ctxb && nutt >= 1 && heads >= 1 && window >= 0 && flash_pipelined_usable((int)dk),
                 "bad arguments");
    std::vector<int> L(nutt);
    for (int i = 0; i < nutt; ++i) {
        SBV2_REQUIRE(lens[i] >= 1 && lens[i] < (1 << 20), "bad sequence length");
        L[i] = (int)lens[i];
    }
    const int H = (int)(heads * dk), nw = 2 * (int)window + 1;
    Arena ar;
    const SegLayout lay = make_layout(L, kFrameGap, ar, nullptr, nullptr, 32);
    const int N = lay.L;
    Plane QKV[2] = {ar.plane(3 * H, N), ar.plane(3 * H, N)}, Cx[4] = {ar.plane(H, N), ar.plane(H, N), ar.plane(H, N), ar.plane(H, N)}, Z = ar.plane(H, N);
    SplitPlanes kv[2];
    const float* hq[2][3] = {{qa, ka, va}, {qb, kb, vb}};
    for (int i = 0; i < 2; ++i) {
        for (int j = 0; j < 3; ++j) upload_packed(hq[i][j], lay, QKV[i].rows(j * H, H), false);
        kv[i] = alloc_split(ar, 2, 3 * H, N);
        HIP_CHECK(hipMemset(kv[i].p, 0, (size_t)2 * kv[i].pstride * 2));
        split_planes(QKV[i].rows(H, 2 * H), kv[i].rows(H, 2 * H), nullptr);
    }
    DevMem d_erk(erk, sizeof(float) * nw * dk), d_erv(erv, sizeof(float) * nw * dk);
    const AttnPlan pl = make_attn_plan(lay, H, (int)heads, QKV[0].ld, (int)window, ar, nullptr, false);
    const size_t words = (size_t)H * Cx[0].ld;
    HIP_CHECK(hipMemset(Z.p, 0, words * 4));
    const float qscale = 1.0f / std::sqrt((float)dk);   // as run_encoder
    const std::vector<RepRegion> regs{{{Cx[0].p, Cx[1].p}, {Cx[2].p, Cx[3].p}, Z.p, words}};
    run_repeated(regs, RepOpts{reps, neighbour, flip_at, flip_word},
                 [&](int which, hipStream_t s) {
                     vits_flash_attention_parts(pl.d_ag, pl.ng, pl.maxT, QKV[which].p, QKV[which].ld, kv[which], H, 2 * H, Cx[which].p, Cx[which].ld, (int)dk,
                                                d_erk.f(), d_erv.f(), (int)window, qscale, s, 1);
                 },
                 mismatch, first_bad);
    download_packed(Cx[2], lay, false, ctxa, nullptr);
    download_packed(Cx[3], lay, false, ctxb, nullptr);
    if (ld_out) *ld_out = Cx[0].ld;
    API_END
}

// The flow FFN pair as VitsModel::run_encoder launches it on conv_clx.hip (weights through the builders of sbv2_debug_conv_ffn_cl: split-bf16 fragments):
// conv_1 reads the parts of x (split_cl_km, once per input) and writes relu(.) as conv_2's operand parts, conv_2 writes the k-major plane y = conv + b + x;
// mask [L] at both.  One repetition = both launches.  Words: the intermediate's parts planes (halo rows included), then y at its pitch [H][round_up(L, 64)].
int sbv2_debug_repeat_conv_ffn_clx(int device, const float* xa, const float* xb, const float* w1, const float* b1, const float* w2, const float* b2, int64_t H,
                                   int64_t F, int64_t k, int64_t L, const uint8_t* mask, int reps, int neighbour, int flip_at, int64_t flip_word, float* ya,
                                   float* yb, int64_t* mismatch, int64_t* first_bad) {
    API_BEGIN
    HIP_CHECK(hipSetDevice(device));
    SBV2_REQUIRE(xa && xb && w1 && w2 && ya && yb && H >= 1 && F >= 1 && k >= 1 && k <= kMaxTaps && (k & 1) && L >= 1 && L * F < ((int64_t)1 << 31), "bad arguments");
    Blob bl1 = one_conv_blob(w1, b1, {F, H, k}, F), bl2 = one_conv_blob(w2, b2, {H, F, k}, H);
    WeightStore ws1(bl1, 2), ws2(bl2, 2);
    PackedConv c1 = ws1.conv("c"), c2 = ws2.conv("c");
    SBV2_REQUIRE(c1.cl.wx && c2.cl.wx, "shape not supported by conv_clx");
    DevPlane Xa(H, L), Xb(H, L), Ya(H, L), Yb(H, L), Ra(H, L), Rb(H, L), Yn(H, L);
    Xa.put(xa, false);
    Xb.put(xb, false);
    const size_t ywords = (size_t)H * Xa.P.ld, xsb = split_cl_bytes((int)H, L) + 16, fsb = split_cl_bytes((int)F, L) + 16;
    HIP_CHECK(hipMemset(Yn.P.p, 0xFF, ywords * 4));
    DevMem mxa(xsb), mxb(xsb), mfa(fsb), mfb(fsb), rfa(fsb), rfb(fsb), finit(fsb), dm(mask, mask ? (size_t)L : 0);
    SplitClPlanes xs[2], fs[2];
    DevMem* fm[2] = {&mfa, &mfb};
    fill_nan(finit, fsb);
    (void)make_split_cl(finit.p, (int)F, L, nullptr);
    for (int i = 0; i < 2; ++i) {
        xs[i] = make_split_cl(i ? mxb.p : mxa.p, (int)H, L, nullptr);
        split_cl_km(i ? Xb.P : Xa.P, 1.0f, xs[i], nullptr);
        fill_nan(*fm[i], fsb);
        fs[i] = make_split_cl(fm[i]->p, (int)F, L, nullptr);
    }
    const Plane X[2] = {Xa.P, Xb.P};
    const std::vector<RepRegion> regs{{{mfa.p, mfb.p}, {rfa.p, rfb.p}, finit.p, split_cl_bytes((int)F, L) / 4}, {{Ya.P.p, Yb.P.p}, {Ra.P.p, Rb.P.p}, Yn.P.p, ywords}};
    run_repeated(regs, RepOpts{reps, neighbour, flip_at, flip_word},
                 [&](int which, hipStream_t s) {
                     ConvClxParams p1;
                     p1.X = xs[which];
                     p1.W = c1.cl.wx;
                     p1.nmt = c1.cl.nmt;
                     p1.M = (int)F;
                     p1.N = (int)L;
                     p1.K = (int)H;
                     p1.ntaps = (int)k;
                     p1.shift0 = -(int)(k - 1) / 2;
                     p1.shift_step = 1;
                     p1.Ys = fs[which];
                     p1.ys_slope = 0.0f;     // ReLU
                     p1.bias = c1.cl.bias;
                     p1.mask = mask ? dm.u8() : nullptr;
                     p1.mask_shift = mask ? 0 : -1;
                     launch_conv_clx(p1, s);
                     ConvClxParams p2;
                     p2.X = fs[which];
                     p2.W = c2.cl.wx;
                     p2.nmt = c2.cl.nmt;
                     p2.M = (int)H;
                     p2.N = (int)L;
                     p2.K = (int)F;
                     p2.ntaps = (int)k;
                     p2.shift0 = -(int)(k - 1) / 2;
                     p2.shift_step = 1;
                     p2.Ykm = static_cast<float*>(regs[1].out[which]);
                     p2.ldykm = X[which].ld;
                     p2.Rkm = X[which].p;
                     p2.ldrkm = X[which].ld;
                     p2.bias = c2.cl.bias;
                     p2.mask = p1.mask;
                     p2.mask_shift = p1.mask_shift;
                     launch_conv_clx(p2, s);
                 },
                 mismatch, first_bad);
    (void)Ra.get(ya, kNanWord);
    (void)Rb.get(yb, kNanWord);
    API_END
}

}  // extern "C"
