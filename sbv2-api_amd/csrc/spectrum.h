// The spectrum of a delivered signal (spectrum.hip): power per STFT bin, or per Slaney mel band, of every frame of the samples a formatted
// fetch leaves in HBM, as include/sbv2_hip.h states it above sbv2_spectrum.  The time axis is that of the pitch contour and of the envelope
// (marks.h).  Used by sbv2_pipeline_fetch_request_spectrum (fetch.cpp) and the test hook sbv2_debug_spectrum; fed replay by replay
// (StreamSpectrum below) by sbv2_stream_begin_request_spectrum (stream_output.cpp) and the test hook sbv2_debug_stream_spectrum.
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

// The same stage FED piece by piece (a stream's replays), by sbv2_spectrum's convention unchanged: frame f has its centre at f hop + hop / 2,
// its window is [centre - n_fft / 2, centre + n_fft / 2), positions outside [0, total) read as 0, n_frames = ceil(total / hop).
// The completion rule: frame f is complete once min(f hop + hop / 2 + n_fft / 2, total) <= D, D the samples fed (or, for what a stream hands
// out, delivered) so far.  Frames complete in order; after the last push everything is complete.
// The carry: the last min(D, n_fft) fed samples, in the sample's own type, on the device.  That is enough: the first incomplete frame has
// centre + n_fft / 2 > D, so its window starts after D - n_fft.  Sized once for kSpectrumMaxFft elements and held twice (a push reads one copy
// and writes the other: a push shorter than the carry keeps part of the old one, and no workgroup reads what another one of the same launch
// overwrites) = 16 KB whatever the stream's length.
// A push is ONE launch (k_stream_spectrum) and one copy of the frames it completed from the push's device rows to the pinned mirror, which
// holds every frame of the stream (n_frames x n_bands f32) until the next begin; a push that completes no frame still updates the carry,
// n = 0 enqueues nothing.  Basis, window, bank and group tables are formed and uploaded in begin.  No atomics.
//
// The work split of a push: frame tiles x G groups.  A tile is 32 frames from the first pending one on; a push completes a few hundred
// frames at most, ten tiles, and k_spectrum's split (a workgroup = all blocks of its frames) would leave most of the chip idle while every
// workgroup streams the whole basis (17.3 MB at n_fft = 2048).  So the 32-bin blocks are cut into G contiguous groups, the grid's second
// dimension: without mel bands group g stores the P of its blocks; with mel bands it owns the bands [m0, m1), computes only the blocks their
// triangles touch (neighbours recompute the few blocks where their triangles overlap; blocks outside [f_min, f_max] belong to nobody) and
// runs each band's compensated sum from its first bin to its last.  Every P[k] is one wave's MFMA chain and every band's chain lies in one
// lane over ascending k: the bits do not depend on G, and equal Spectrum::run over the whole signal for every encoding, whatever the pushes.
// The rule for G: as many groups as it takes for tiles x G workgroups to reach the compute units of the device, but never so many that a
// group holds fewer than one bin tile of four blocks (below that a workgroup's four waves no longer all have a block): G <= blocks / 4, the
// blocks being those the bank spans with mel bands, n_bins / 32 rounded up without.  n_fft = 400 (7 blocks) has G = 1, n_fft = 2048 up to 8.
constexpr int kSpectrumMaxGroups = 8;   // (33 blocks at n_fft = 2048) / 4
inline int spectrum_stream_groups_max(int blocks) { return std::max(1, std::min(kSpectrumMaxGroups, blocks / 4)); }
inline int spectrum_stream_groups(int64_t frames, int blocks, int cus) {
    const int64_t tiles = (frames + 31) / 32;
    int G = 1;
    while (tiles * G < cus && G < spectrum_stream_groups_max(blocks)) ++G;
    return G;
}
// the completion rule on its own: the frames of a signal of `total` samples that are complete once D of them are in
int64_t spectrum_frames_complete(const SpectrumSpec& sp, int64_t total, int64_t D);
class StreamSpectrum {
  public:
    StreamSpectrum() = default;
    StreamSpectrum(const StreamSpectrum&) = delete;
    StreamSpectrum& operator=(const StreamSpectrum&) = delete;
    // Host only, throws: the spec within the stage's limits, fewer than 2^30 frames
    static void check(const SpectrumSpec& sp, int64_t total);
    // Forms and uploads the tables the previous stream did not leave, sizes the push's rows for pushes of up to `most` samples (a longer one
    // grows them, which waits for s) and waits for s once.  groups: 0 = the rule; otherwise that G for every push, at most the rule's largest.
    void begin(const SpectrumSpec& sp, int encoding, int64_t total, int64_t most, hipStream_t s, int groups = 0);
    // x = the sample at delivered position D0 (device), D0 = fed(); returns the frames this push completed; n = 0 enqueues nothing
    int64_t push(const void* x, int64_t D0, int64_t n, hipStream_t s);
    int64_t fed() const { return fed_; }
    int64_t total() const { return total_; }
    int64_t n_frames() const { return nf_; }
    const SpectrumSpec& spec() const { return sp_; }
    int64_t complete(int64_t D) const;   // the completion rule: frames complete once D samples are in
    // frame f (n_bands values) is valid once the push that completed it has run on s
    const float* power_host(int64_t f) const { return host_.as<float>() + f * sp_.n_bands(); }

  private:
    static constexpr size_t kCarryBytes = (size_t)kSpectrumMaxFft * sizeof(float);   // one copy, in the widest sample type
    using BankKey = std::tuple<int, int, int, double, double>;
    struct Groups { int32_t v[4 * kSpectrumMaxGroups]; };   // {m0, m1, bb0, bb1} per group, as the launch takes it
    PinnedBuffer host_, stage_;   // the results' mirror; upload staging
    DeviceBuffer table_, window_, bank_, carry_, out_;
    std::vector<int32_t> range_;  // the bank's ranges on the host
    Groups groups_[kSpectrumMaxGroups];   // the table at G = 1 ... spectrum_stream_groups_max
    BankKey bank_key_;
    SpectrumSpec sp_;
    int64_t total_ = 0, nf_ = 0, fed_ = 0, done_ = 0;
    int encoding_ = 0, parity_ = 0, forced_ = 0, blocks_ = 0, basis_fft_ = 0;
};

}  // namespace sbv2
