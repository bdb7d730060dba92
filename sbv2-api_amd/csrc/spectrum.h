// The spectrum of a delivered signal (spectrum.hip): power per STFT bin, or per Slaney mel band, of every frame of the samples a formatted
// fetch leaves in HBM, as include/sbv2_hip.h states it above sbv2_spectrum.  The time axis is that of the pitch contour and of the envelope
// (marks.h).  Used by sbv2_pipeline_fetch_request_spectrum (fetch.cpp) and the test hook sbv2_debug_spectrum.
#pragma once
#include <tuple>

#include "common.h"
#include "pcm_format.h"

namespace sbv2 {

constexpr int kSpectrumMinFft = 64, kSpectrumMaxFft = 2048, kSpectrumMaxMels = 128, kSpectrumMaxRate = 48000;

// Checked parameters and what follows from them.
struct SpectrumSpec {
    int sample_rate = 0;
    int n_fft = 0, n_mels = 0;
    int64_t hop = 0;
    double f_min = 0.0, f_max = 0.0;
    int n_bins() const { return n_fft / 2 + 1; }
    int n_bands() const { return n_mels ? n_mels : n_bins(); }
};
// throws: n_fft a multiple of 16 in [64, 2048], 1 <= hop <= n_fft, 0 <= n_mels <= 128, 0 <= f_min < f_max <= sr / 2, 0 < sr <= 48000
// (NaNs fail every comparison and are refused)
SpectrumSpec spectrum_spec(int sample_rate, int n_fft, int64_t hop, int n_mels, double f_min, double f_max);
inline int64_t spectrum_frames(int64_t n, int64_t hop) { return n > 0 ? (n + hop - 1) / hop : 0; }
// The Slaney mel bank of a spec with n_mels > 0, W [n_mels][n_bins], formed in f64 and rounded to f32; range [2 m], [2 m + 1] = the bins
// [lo, hi) outside which row m is zero (lo = hi: a triangle that holds no bin).
void spectrum_mel_bank(const SpectrumSpec& sp, std::vector<float>* W, std::vector<int32_t>* range);
// The periodic Hann window, 0.5 - 0.5 cos(2 pi i / n_fft) in f64, rounded to f32.
void spectrum_window(int n_fft, std::vector<float>* w);

// Frames per workgroup.  A workgroup of four waves owns FT consecutive frames and all their bands, so the launch has ceil(n_frames / FT)
// workgroups and FT trades the chip's fill against the bytes of the basis each frame pulls through LDS:
//   FT = 32:  the four waves take four 32-bin blocks of the same 32 frames; a workgroup streams the whole basis for 32 frames.
//   FT = 128: the four waves take four 32-frame blocks and share one 32-bin block; a quarter of the bytes per frame.
// The rule: FT = 128 once its tiles alone give every compute unit of an MI355X (256) a workgroup, n_frames > 128 * 256; below that FT = 32
// spreads what there is (a single utterance of 1000 frames: 32 workgroups instead of 8).  Every (frame, bin) sum runs in one wave in the
// same order either way: the two give identical bits.
constexpr int64_t kSpectrumWideFrames = 128 * 256;
inline int spectrum_tile(int64_t n_frames) { return n_frames > kSpectrumWideFrames ? 128 : 32; }

// Device state of the spectrum stage of one execution context: per n_fft the basis in MFMA fragment order and the window, per (n_fft, n_mels,
// rate, f_min, f_max) the mel bank, the results on the device and their pinned mirror, grown on demand; nothing is allocated before the first
// run.  One launch per run (k_spectrum), no atomics.
// What the FIRST run with an n_fft or a bank costs, inside the fetch: the table is formed on the host in f64 (4.3 M splits and 17.3 MB at n_fft
// = 2048; 0.75 MB at 400), uploaded from pinned staging, and the stream is synchronised once for it (so that fetch has two synchronisations
// more than its one).  Later runs find both cached and add one launch.  The caches are bounded: kMaxBases tables (at most 69 MB per context)
// and kMaxBanks banks (at most 4.2 MB); a run that needs one more drops them all after a synchronisation and starts again.
class Spectrum {
  public:
    Spectrum() = default;
    Spectrum(const Spectrum&) = delete;
    Spectrum& operator=(const Spectrum&) = delete;
    // Enqueues on s the stage over x = n delivered samples on the device (encoding 0 = f32, 1 = s16, 7 / 6 = G.711 codes, as Marks::run) and
    // the copy of its results to the host: power_host()[f n_bands + m] holds frame f < n_frames() once s has been synchronised.  n = 0
    // enqueues nothing.  A new n_fft or a new bank is built and uploaded from pinned staging on s first (the costs are stated above).
    void run(const void* x, int encoding, int64_t n, const SpectrumSpec& sp, hipStream_t s);
    int64_t n_frames() const { return nf_; }
    const float* power_host() const { return host_.as<float>(); }

  private:
    struct Basis {
        DeviceBuffer table, window;   // [bin block][K chunk][k step][cos hi, cos lo, sin hi, sin lo][64 lanes][8] f16; [n_fft] f32
    };
    using BankKey = std::tuple<int, int, int, double, double>;   // n_fft, n_mels, rate, f_min, f_max
    static constexpr size_t kMaxBases = 4, kMaxBanks = 8;
    std::map<int, Basis> basis_;            // by n_fft
    std::map<BankKey, DeviceBuffer> banks_; // W [n_mels][n_bins] f32 | range [n_mels][2] i32
    PinnedBuffer stage_;                    // upload staging (a basis, or a bank)
    DeviceBuffer dev_;                      // power [n_frames][n_bands]
    PinnedBuffer host_;
    int64_t nf_ = 0;
};

}  // namespace sbv2
