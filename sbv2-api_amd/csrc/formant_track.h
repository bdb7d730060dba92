// The formant tracker (formant_track.hip): one best path through the kept roots of the formant contour, as include/sbv2_hip.h states it above
// sbv2_formant_track.  The stage of formants.h runs unchanged with n_formants = K candidates per frame; a state of a frame is an assignment of
// the T tracks to its m candidates in ascending order, and one path is chosen through the states of every run of frames between cuts (frames
// with m < T).  Used by sbv2_pipeline_fetch_request_formant_track (fetch.cpp) and the test hook sbv2_debug_formant_track.  Everything after the
// candidates' f64 values is integer arithmetic: the path does not depend on any order of evaluation.
#pragma once
#include "common.h"
#include "formants.h"

namespace sbv2 {

constexpr int kFtMaxTracks = 5, kFtMaxCand = 7, kFtMaxStates = 35;   // C(7, 3) = C(7, 4) = 35
constexpr int kFtBpStride = 40;                                       // back-pointer bytes per frame (>= kFtMaxStates, a multiple of 8)
constexpr int kFtGrid = 1024;                                         // workgroups (of one wave) of k_ftrack_path at most, as kTrackGrid
constexpr double kFtMaxF = 32768.0, kFtMaxB = 16777216.0;             // what a candidate table may hold (Hz); B above kFtMaxB counts as kFtMaxB

// Checked parameters: the three costs in 1 / 65536 units and the references in Hz, integers formed once on the host.
struct FormantTrackSpec {
    int T = 0, K = 0;
    int64_t Wf = 0, Wb = 0, Wj = 0;
    int64_t Rq[kFtMaxTracks] = {0, 0, 0, 0, 0};
};
// THE check; throws on anything outside the ranges include/sbv2_hip.h states (NaNs fail every comparison and are refused): n_tracks in [1, 5],
// candidates in [n_tracks, min(7, order / 2)], ref_hz[0 .. n_tracks) strictly ascending within (0, sample_rate / 2), the costs in [0, 16],
// reserved = 0.
FormantTrackSpec formant_track_spec(int n_tracks, int candidates, const double* ref_hz, double freq_cost, double bw_cost, double jump_cost, int reserved,
                                    int sample_rate, int order);
// throws unless every row of cand_f / cand_b [nf][K] holds its positive F first, in non-descending order and at most kFtMaxF, zeros behind them,
// and every B in [0, kFtMaxB]
void formant_track_check_table(const double* cand_f, const double* cand_b, int64_t nf, int K);

// Device state of the tracker of one execution context: the results and their pinned mirror, the run list, the frames' candidate counts and
// the back-pointers, grown on demand; nothing is allocated before the first run.  Two launches per run, no atomics, no host round trip:
//   * k_ftrack_runs (one workgroup): every frame's m is counted once; a cut is delivered on the spot (its first m candidates, zeros, state -1);
//     the first frame of every run and the cut behind its last one are flagged and scanned into a list of pairs.
//   * k_ftrack_path: one wavefront per run, workgroup i takes the runs i, i + grid, ...; the lanes are the states of the current frame.
class FormantTrack {
  public:
    FormantTrack() = default;
    FormantTrack(const FormantTrack&) = delete;
    FormantTrack& operator=(const FormantTrack&) = delete;
    // Enqueues on s the path over cand_f / cand_b [nf][sp.K] on the device (the stage's F and B, or a table that formant_track_check_table has
    // passed) and the copy of its results to the host: f_host()[f T + t], bw_host() likewise and state_host()[f] hold frame f < nf once s has
    // been synchronised.  nf = 0 enqueues nothing.
    void run(const double* cand_f, const double* cand_b, int64_t nf, const FormantTrackSpec& sp, hipStream_t s);
    const double* f_host() const { return host_.as<double>(); }
    const double* bw_host() const { return host_.as<double>() + nf_ * T_; }
    const int32_t* state_host() const { return reinterpret_cast<const int32_t*>(host_.as<double>() + 2 * nf_ * T_); }

  private:
    DeviceBuffer dev_;   // F [nf][T] | B [nf][T] | state [nf] (mirrored) | runs [nf + 2] | nruns | m [nf] | back-pointers [nf][kFtBpStride]
    PinnedBuffer host_;
    int64_t nf_ = 0, T_ = 0;
};

}  // namespace sbv2
