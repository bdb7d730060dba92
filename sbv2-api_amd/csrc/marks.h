// Speech marks (marks.hip): where each token lies in a delivered signal (host arithmetic, marks_spans) and how loud it is there (one
// segmented reduction over the samples a formatted fetch leaves in HBM: sum of squares and peak per [start, end) segment).  Used by
// sbv2_pipeline_fetch_request_marks (fetch_formatted, api.cpp), sbv2_stream_marks (stream.cpp) and the test hook sbv2_debug_segment_levels.
#pragma once
#include "common.h"
#include "pcm_format.h"

namespace sbv2 {

// Delivered index of native position a at rate L / M: ceil(a L / M), the rule of pcm_format_out_len.
inline int64_t marks_delivered(const PcmFmtSpec& s, int64_t a) { return (a * s.L + s.M - 1) / s.M; }
// Token t of a row with durations d (frames, >= 0), placed at native sample `place` of its timeline, hop samples per frame:
// [start[t], end[t]) = [J(place + hop c[t]), J(place + hop c[t + 1])), c the exclusive prefix sum of d.  Throws for a negative duration,
// hop < 1, place < 0 and positions that leave the int64 range of a L.
void marks_spans(const int64_t* d, int64_t n, int64_t hop, int64_t place, const PcmFmtSpec& s, int64_t* start, int64_t* end);

// Device state of the level reduction of one execution context: the segment table (pinned + device) and the results (device + pinned), grown
// on demand; nothing is allocated before the first run.  One launch per run, no atomics: a segment's sum is formed in an order that depends
// on its length only, so equal samples give equal bits.
class Marks {
  public:
    Marks() = default;
    Marks(const Marks&) = delete;
    Marks& operator=(const Marks&) = delete;
    // segments longer than this take a whole workgroup (256 lanes) instead of one wave
    static constexpr int64_t kLongSegment = 4096;
    // Enqueues on s: sumsq / peak of x[seg[2 i], seg[2 i + 1]) for i < nseg, x = n delivered samples on the device (encoding 0 = f32,
    // 1 = s16, taken as integers, 7 / 6 = G.711 codes, taken as the integers they decode to), and the copy of the results to the host: sumsq_host()[i] / peak_host()[i] hold them once s has been
    // synchronised.  Every segment is checked against [0, n] before anything is enqueued (throws); nseg = 0 enqueues nothing.
    void run(const void* x, int encoding, int64_t n, const int64_t* seg, int64_t nseg, hipStream_t s);
    const double* sumsq_host() const { return res_host_; }
    const double* peak_host() const { return res_host_ + nseg_; }

  private:
    PinnedBuffer host_;   // segment table | order, then the results
    DeviceBuffer dev_;    // the same
    double* res_host_ = nullptr;
    int64_t nseg_ = 0;
};

}  // namespace sbv2
