// Parametric EQ (eq.hip): the filter stage of a request fetch, a cascade of up to 8 biquads in f64, as include/sbv2_hip.h states it above
// sbv2_eq.  It sits behind the shifter (voice.h) and the token gain (token_gain.h) and in front of the formatter: it reads the rows where the
// formatter would have read them, writes the filtered rows into its own buffer laid out like the packed PCM, and the formatter's pieces are
// re-pointed.  Three launches on the fetch's stream, no atomics, no host round trip:
//   k_eq_tiles   every tile that has a successor: the cascade's state at the tile's end from zero state at its head;
//   k_eq_carry   one wavefront per row walks its tiles: entry_{i+1} = M_T entry_i + e_i, the state every tile is entered with;
//   k_eq_apply   the hot path: every native sample of the listed rows is read once and written once, filtered from its tile's entry state.
// The split.  The cascade of S sections is a linear recurrence on N = 2 S doubles: over m samples, s_end = M_m s_start + e, with M_m the
// zero-input transition (formed on the host by repeated squaring, eq_powers) and e the end state from zero.  A workgroup of 256 lanes owns a
// tile of kTile = 256 kLane consecutive samples of ONE row, counted from the row's head; lane t walks the kLane samples [t kLane, (t + 1)
// kLane) serially.  kLane is FIXED, so the matrix half of every map in the scan over the lanes is known ahead (M_{kLane 2^k}, k = 0 .. 7) and
// only the vector half is scanned: 8 Kogge-Stone steps of one N x N matrix-vector product per lane.  Only full tiles hand a state on, so one
// more power, M_T = M_{256 kLane}, serves across tiles.
// LDS of a workgroup: the tile as f32 words at a row stride of kLane + 1 (lane t reads word t (kLane + 1) + n: 64 different banks), 66560
// bytes; the 8 matrices, 64 N^2 bytes; the scan's exchange buffer [N][256] doubles, 2048 N bytes.  S = 8: 115712 bytes, one workgroup per
// CU; S <= 3: two.
#pragma once
#include "common.h"

namespace sbv2 {

// A row of the packed buffer: its first sample and its length.
struct EqRow {
    int64_t off, n;
};

constexpr int kEqMaxBands = 8;

// Checked parameters of a call (eq_spec): the sections' coefficients b0 b1 b2 a1 a2 (a0 = 1), band by band.
struct EqSpec {
    int n_bands = 0;
    double coef[5 * kEqMaxBands] = {0};
    bool filters = false;   // some band is not the identity (a shelf or peak at 0 dB is): the stage has something to do
};
// THE check and the design (Audio-EQ-Cookbook biquads at `rate`, f64); throws, naming the field, on n_bands outside [0, 8], a kind outside
// 0 .. 4, f0_hz outside [10, 0.45 rate], gain_db outside [-24, 24] or non-zero on a high-pass / low-pass, q outside [0.1, 20], reserved != 0
// (a NaN fails every comparison and is refused).
EqSpec eq_spec(int n_bands, const int32_t* kind, const double* f0_hz, const double* gain_db, const double* q, int reserved, int rate);

// The zero-input transition of the cascade over kLane 2^k samples, k = 0 .. 8 (the last one is M_T): pw [9][N N], row-major, N = 2 n_bands.
// Host: the one-sample transition from the section step on unit vectors, then squarings, in long double, each power rounded to f64 once
// (eq.hip says why f64 squarings are not enough).  Every power keeps the cascade's block lower triangle: entry (i, j) with j > 2 (i / 2) + 1
// is exactly 0, and the kernels skip those.
void eq_powers(const EqSpec& sp, double* pw);

// Device state of the stage of one execution context, grown on demand; nothing is allocated before the first run.
class Eq {
  public:
    Eq() = default;
    Eq(const Eq&) = delete;
    Eq& operator=(const Eq&) = delete;
    static constexpr int kLane = 64;             // samples a lane walks serially
    static constexpr int kTile = 256 * kLane;    // samples of one row per workgroup
    // Enqueues on s the three launches over the rows rows[nrows] of x (a packed buffer of `total` floats on the device, only read); sp.n_bands
    // >= 1.  -> the filtered rows, laid out as x (what lies between and outside the rows is not written and must not be read).  y64 (a
    // DEVICE buffer laid out as x, or NULL): besides, every sample's f64 value before the cast.  Rows are checked before anything is enqueued.
    const float* run(const float* x, int64_t total, const EqRow* rows, int nrows, const EqSpec& sp, hipStream_t s, double* y64 = nullptr);

  private:
    PinnedBuffer host_;   // the tables for their upload
    DeviceBuffer dev_;    // the same tables | the tiles' end states | the tiles' entry states
    DeviceBuffer out_;    // the filtered rows
};

}  // namespace sbv2
