// The pitch tracker (track.hip): one best path through the per-frame candidates of the YIN contour, as include/sbv2_hip.h states it above
// sbv2_pitch_track.  Used by sbv2_pipeline_fetch_request_tracked (the delivered contour through Pitch::run, the shifter's own contour through
// Voice::run) and the test hook sbv2_debug_pitch_track.  The candidates come from k_pitch_yin_cand (marks.hip, pitch_launch with cand).
// Everything here is integer arithmetic: the path does not depend on any order of evaluation.
#pragma once
#include "common.h"
#include "marks.h"

namespace sbv2 {

// Checked parameters: the three costs in 1 / 65536 units (llrint(value * 65536), formed once on the host) and the candidates' ceiling.
struct TrackSpec {
    double cand_max = 0.0;
    int64_t U = 0, Sw = 0, J = 0;
};
// throws: cand_max in (0, 1], unvoiced_cost and switch_cost in [0, 4], jump_cost in [0, 16] (NaNs fail every comparison and are refused)
TrackSpec track_spec(double cand_max, double unvoiced_cost, double switch_cost, double jump_cost);
// throws unless every record of cand [nf][kTrackRec] has ncand in [0, 7], its tau ascending within [1, kPitchMaxTau] and its q in [0, 65536]
void track_check_table(const int32_t* cand, int64_t nf);

constexpr int kTrackStates = kTrackCand + 1;   // the candidates and, last, unvoiced
constexpr int kTrackGrid = 1024;               // workgroups (of one wave) of k_track_path at most: a run list longer than that is strided over

// Device state of the tracker of one execution context: the run list, the back-pointers and the path, grown on demand; nothing is allocated
// before the first run.  Two launches per run, no atomics, no host round trip:
//   * k_track_runs (one workgroup): the frames without a candidate ("cuts") and the first frames of the rows, flagged and scanned into the
//     list of runs.  A cut has the single state "unvoiced", so the frames before and after it do not influence each other's choices.
//   * k_track_path: one wavefront per run, workgroup i takes the runs i, i + grid, ...; it walks its run forward (64 lanes = 8 x 8 state
//     pairs), writes one back-pointer byte per (frame, state), backtraces 64 frames at a time and writes state [nf] and, where given, the
//     tracked lag / voiced / c3 over the plain contour's.
class Track {
  public:
    Track() = default;
    Track(const Track&) = delete;
    Track& operator=(const Track&) = delete;
    // Enqueues on s.  cand [nf][kTrackRec] on the device (trusted: the extraction's, or checked by track_check_table); rows: nrows > 0 device
    // int64 values at row_off[i * row_stride], the first frame of row i (rows are tracked apart from each other), nrows = 0: one signal.
    // lag / voiced / c3 [nf] (with cand_c3 [nf][7][3]; all four or none): the plain contour in, the tracked one out.  nf = 0 enqueues nothing.
    void run(const int32_t* cand, const double* cand_c3, int64_t nf, const TrackSpec& sp, double* c3, int32_t* lag, int32_t* voiced, hipStream_t s,
             const int64_t* row_off = nullptr, int row_stride = 0, int nrows = 0);
    const int32_t* state_device() const { return d_state_; }   // [nf]: 0 .. 6 the candidate, 7 unvoiced

  private:
    DeviceBuffer dev_;   // runs [nf + 1] | nruns | state [nf] | back-pointers [nf][8]
    int32_t* d_state_ = nullptr;
};

}  // namespace sbv2
