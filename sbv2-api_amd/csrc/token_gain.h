// Per-token volume targets (token_gain.hip): the gain stage of a request fetch that edits loudness token by token, as include/sbv2_hip.h
// states it above sbv2_token_gain.  It sits behind the shifter (voice.h) and in front of the formatter: it reads the rows where the formatter
// would have read them (the run's packed PCM, or the shifter's output), writes the edited rows into its own buffer laid out like the packed
// PCM, and the formatter's pieces are re-pointed.  Three launches on the fetch's stream, no atomics, no host round trip:
//   k_tgain_level    the f64 sum of squares of every token's span: one wave per span of <= kLongSpan samples, one workgroup per longer one;
//   k_tgain_factors  lanes take tokens: M_t, src_rms, the factor and its clamp, the ramp length at the token's end -> one record per token;
//   k_tgain_apply    y[n] = float(double(x[n]) g(n)), the hot path: every native sample of the listed rows is read once and written once.
// The tile rule of k_tgain_apply.  A workgroup of 256 lanes owns kTile = 2048 consecutive samples of ONE row, counted from the row's head: a
// whole number of hops (the model's hop is 512 native samples and token ends are multiples of it), so a token boundary falls on a tile edge or
// inside a tile, never between the rows' coordinates and the tiles'.  2048 and not 1024: a tile stages at most kStage records whatever its
// size, and the bisection and the staging (a dependent chain of scalar loads ahead of the first sample) are paid once per tile; at 2048
// every lane moves two 16-byte groups.  profiles/token_gain_probe.txt holds the trace at 2048: the kernel is bound by that prologue, not
// by HBM; 1024 was not traced.  A tile meets at most 4 non-empty tokens of >= 1 hop plus one
// neighbour to each side; kStage = 16 leaves room for zero-duration tokens between them.  A tile that would need more records (a run of more
// than ten zero-duration tokens) reads the table in HBM by a bisection per group instead: slower, same bits.
#pragma once
#include "common.h"

namespace sbv2 {

// A row of the packed buffer: its first sample and its length.
struct TokenGainRow {
    int64_t off, n;
};

// Checked parameters of a call (token_gain_spec).  HOST arrays: value [n_tokens], the rows' tokens back to back.
struct TokenGainSpec {
    const double* value = nullptr;
    int64_t n_tokens = 0;
    int kind = 0;
    int64_t ramp = 0;
    double max_ratio = 1.0;
    bool edits = false;   // some token's factor can differ from 1: the stage has something to do
};
// throws: n_tokens >= 0, value given, kind in {0, 1}, ramp >= 0, max_ratio >= 1 and finite, every value finite and >= 0, reserved == 0
// (a NaN fails every comparison and is refused)
TokenGainSpec token_gain_spec(const double* value, int64_t n_tokens, int kind, int64_t ramp, double max_ratio, int64_t reserved);

// Device state of the stage of one execution context, grown on demand; nothing is allocated before the first run.
class TokenGain {
  public:
    TokenGain() = default;
    TokenGain(const TokenGain&) = delete;
    TokenGain& operator=(const TokenGain&) = delete;
    static constexpr int kTile = 2048;          // samples of one row per workgroup of k_tgain_apply
    static constexpr int kStage = 16;           // records a tile stages in LDS
    static constexpr int64_t kLongSpan = 4096;  // spans longer than this take a whole workgroup of k_tgain_level
    // Enqueues on s the three launches over the rows rows[nrows] of x (a packed buffer of `total` floats on the device, only read) and the copy
    // of applied / src_rms to the host.  tok_counts [nrows]: tokens of every row; tok_ends [sum]: the sample of its row every token ends at,
    // ascending within [0, rows[k].n] (checked before anything is enqueued; throws).  -> the edited rows, laid out as x (what lies between
    // and outside the rows is not written and must not be read).  applied_host() / src_rms_host() hold the tokens' results once s has been
    // synchronised.
    const float* run(const float* x, int64_t total, const TokenGainRow* rows, int nrows, const int64_t* tok_counts, const int64_t* tok_ends,
                     const TokenGainSpec& sp, hipStream_t s);
    int64_t n_tokens() const { return nt_; }
    const double* applied_host() const { return res_host_; }
    const double* src_rms_host() const { return res_host_ + nt_; }

  private:
    PinnedBuffer host_;   // the tables for their upload, then the results' mirror
    DeviceBuffer dev_;    // the same tables | sums of squares | records | results
    DeviceBuffer out_;    // the edited rows
    double* res_host_ = nullptr;
    int64_t nt_ = 0;
};

}  // namespace sbv2
