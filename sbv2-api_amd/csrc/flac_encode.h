// FLAC encoder on the device (flac_encode.hip): mono 16-bit streams of the s16 samples PcmFormatter::run leaves in HBM, encoded before the
// copy to the host.  Used by the FLAC sink of the formatted fetches (fetch_formatted, fetch.cpp), the FLAC stream (StreamOutput::push, stream_output.cpp) and the
// sbv2_debug_flac_* hooks (test_hooks.cpp).
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

// bytes one push of n samples into a fed stream can deliver at most: the stream header (first push), then the frames that a carried tail of
// up to 4095 samples and the n new ones complete, each at its VERBATIM bound
int64_t flac_stream_bound(int64_t n);

// The same encoder fed piece by piece (a synthesis stream's replays): begin, then pushes in stream order.  The frames are the frames
// FlacEncoder::encode gives the whole signal (the bytes are a function of the samples, the frame number and the rate); the 42-byte stream
// header is written on the host (header()), with min / max frame size 0 = unknown.  Nothing here waits for the GPU after begin (which may
// grow the buffers): which frames a push completes follows from the sample counts, their sizes arrive in the pinned region with the bytes.
class FlacStreamEncoder {
  public:
    // What a push enqueued.  The pointers lie in the push's pinned region and hold its result once the stream has passed the push.
    struct Push {
        int64_t first_frame = 0;        // stream number of the push's first frame
        int frames = 0;                 // frames it completed (0: nothing was launched, nothing may be read)
        const int64_t* err = nullptr;   // 0, or the packing kernel's refusal
        const int64_t* pre = nullptr;   // frame i of the push = bytes[pre[i], pre[i + 1])
        const uint8_t* bytes = nullptr;
        int64_t size(int f0, int f1) const;   // bytes of frames [f0, f1) of the push (checks err)
    };
    FlacStreamEncoder() = default;
    FlacStreamEncoder(const FlacStreamEncoder&) = delete;
    FlacStreamEncoder& operator=(const FlacStreamEncoder&) = delete;
    // pinned bytes the region of one push of up to max_push samples needs
    static size_t host_bytes(int64_t max_push);
    // a stream of total_samples at `rate`, fed in pushes of up to max_push samples: frame counter 0, tail empty
    void begin(int rate, int64_t total_samples, int64_t max_push, hipStream_t s);
    // where the next push's samples go (device): right behind the carried tail
    int16_t* dst() const;
    // the n samples at dst() join the stream; `last`: the remainder becomes the short final frame.  `host`: pinned, host_bytes(max_push)
    // bytes, left alone until the push is delivered.
    Push push(int64_t n, bool last, void* host, hipStream_t s);
    void header(uint8_t* out) const;   // the stream's first kFlacStreamHeader bytes
    int64_t tail() const { return tail_; }

  private:
    DeviceBuffer buf_;    // [tail | new samples]
    DeviceBuffer tab_;    // the push's signal entry and the scan's per-signal outputs
    DeviceBuffer desc_;   // per-frame descriptors
    DeviceBuffer out_;    // [error word | prefix | packed frames]
    int rate_ = 0, rate_code_ = -1;
    int64_t total_ = 0, max_push_ = 0, fed_ = 0, frames_ = 0, tail_ = 0;
    bool done_ = false;
};

}  // namespace sbv2
