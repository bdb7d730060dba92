// FLAC encoder on the device (flac_encode.hip): mono 16-bit streams of the s16 samples PcmFormatter::run leaves in HBM, encoded before the
// copy to the host.  Used by sbv2_pipeline_fetch_flac and sbv2_debug_flac_encode (api.cpp).
#pragma once
#include "common.h"

namespace sbv2 {

constexpr int kFlacBlock = 4096;          // samples per frame (the last frame of a signal may be shorter)
constexpr int kFlacStreamHeader = 42;     // "fLaC" + STREAMINFO block header + 34-byte STREAMINFO
constexpr int kFlacMaxFrameHeader = 13;   // sync + 2 code bytes + 6-byte frame number + 16-bit block size + CRC-8

// bytes one signal of n s16 samples can take at most: the stream header, then per frame the largest header, a VERBATIM subframe (1 + 2 n_f
// bytes) and the CRC-16.  The encoder never exceeds it: VERBATIM is always a candidate.
int64_t flac_bound(int64_t n);
// the frame-header code of a supported rate (throws for any other rate)
int flac_rate_code(int rate);

// Device state of the encoding launches of one execution context: the signal table (pinned + device), the per-frame descriptors, the scan's
// offsets and per-signal sizes, and the output buffer of the streams (all grown on demand; growing synchronises the stream).
class FlacEncoder {
  public:
    explicit FlacEncoder(int device) : device_(device) {}
    ~FlacEncoder();
    FlacEncoder(const FlacEncoder&) = delete;
    FlacEncoder& operator=(const FlacEncoder&) = delete;
    // Encodes signal i = x_dev[offs[i], offs[i] + lens[i]) (device s16) as one FLAC stream at `rate`; the streams lie back to back in output().
    // Enqueues three launches on s, then reads back the per-signal sizes (synchronises s): bytes[i] = stream i's size, returns the total.
    int64_t encode(const int16_t* x_dev, const std::vector<int64_t>& offs, const std::vector<int64_t>& lens, int rate, hipStream_t s,
                   std::vector<int64_t>* bytes);
    const void* output() const { return out_; }

  private:
    template <typename T>
    T* grow(T*& p, size_t& cap, size_t n, hipStream_t s);
    int device_;
    void* sig_host_ = nullptr;   // pinned signal table
    size_t sig_host_cap_ = 0;
    void* sig_ = nullptr;        // device: signal table, then per-signal outputs
    size_t sig_cap_ = 0;
    void* frames_ = nullptr;     // device: per-frame descriptors and the scan's prefix
    size_t frames_cap_ = 0;
    int64_t* sizes_host_ = nullptr;   // pinned: per-signal stream sizes + total + error word
    size_t sizes_host_cap_ = 0;
    uint8_t* out_ = nullptr;
    size_t out_cap_ = 0;
};

}  // namespace sbv2
