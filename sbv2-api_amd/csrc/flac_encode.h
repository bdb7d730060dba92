// FLAC encoder on the device (flac_encode.hip): mono 16-bit streams of the s16 samples PcmFormatter::run leaves in HBM, encoded before the
// copy to the host.  Used by the FLAC sink of the formatted fetches (fetch_formatted, api.cpp) and sbv2_debug_flac_encode (test_hooks.cpp).
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
    FlacEncoder() = default;
    FlacEncoder(const FlacEncoder&) = delete;
    FlacEncoder& operator=(const FlacEncoder&) = delete;
    // Encodes signal i = x_dev[offs[i], offs[i] + lens[i]) (device s16) as one FLAC stream at `rate`; the streams lie back to back in output().
    // Enqueues three launches on s, then reads back the per-signal sizes (synchronises s): bytes[i] = stream i's size, returns the total.
    int64_t encode(const int16_t* x_dev, const std::vector<int64_t>& offs, const std::vector<int64_t>& lens, int rate, hipStream_t s,
                   std::vector<int64_t>* bytes);
    const void* output() const { return out_.get(); }

  private:
    PinnedBuffer sig_host_;     // signal table
    DeviceBuffer sig_;          // signal table, then per-signal outputs
    DeviceBuffer frames_;       // per-frame descriptors and the scan's prefix
    PinnedBuffer sizes_host_;   // per-signal stream sizes + total + error word
    DeviceBuffer out_;
};

}  // namespace sbv2
