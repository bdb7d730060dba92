// What a running stream does to decoded PCM after the decoder (stream_output.cpp): the formatter, the optional level control, level reduction,
// pitch estimator and FLAC encoder, and the sink.  One object per execution context, behind VitsModel::stream_* as OutputChain (api_internal.h)
// is behind the formatted fetches; the decoder's replays, their pinned slots and the prefetch stay in VitsModel.
#pragma once
#include "flac_encode.h"
#include "leveler.h"
#include "limiter.h"
#include "marks.h"
#include "pcm_format.h"
#include "voice.h"

#include <memory>

namespace sbv2 {

// levels on a stream (sbv2_stream_levels, include/sbv2_hip.h)
struct StreamMarksSpec {
    bool tokens = false;
    int64_t env_hop = 0;
    // the pitch contour of the delivered samples (sbv2_stream_pitch): on or off independently of the levels; the spec at the stream's delivered rate
    bool pitch = false;
    PitchSpec pitch_spec;
};

// One window of a replay as the voice stage is fed it (sbv2_stream_voice): the window's central native samples clipped to its row, the
// samples [s0, s1) of row `row`, at src on the device.
struct StreamVoiceFeed {
    int row;
    int64_t s0, s1;
    const float* src;
};

class StreamOutput {
  public:
    // What one replay left in its pinned slot (`host`), per window: the delivered samples [off, off + n) of the slot, the samples the window
    // fed (n without a level: delivery then runs A behind), and with FLAC the frames [fr0, fr1) of the slot's push that it completed.
    struct Slot {
        struct Win { int64_t off, n, fed; int fr0, fr1; };
        std::vector<Win> win;
        FlacStreamEncoder::Push flac;
        const char* host = nullptr;
    };
    // what one call handed out: samples delivered, bytes written to the caller's buffer, samples of the chunk taken
    struct Taken {
        int64_t samples = 0, bytes = 0, fed = 0;
    };
    // Host only, throws: the frame counts of the envelope and of the contour over the `joined` native samples of the timeline, then the
    // look-ahead A of the level (0 without one), which it returns.  Called before a stream sets up anything.
    static int64_t check(const PcmFmtSpec& spec, const StreamLevelSpec* level, const StreamMarksSpec* marks, int64_t joined);
    // A voice stream (sbv2_stream_voice) over rows of len[i] native samples at place[i] of the timeline, begun right after begin(): the
    // shifter's stage is made on first use; upto = the calls' cumulative delivered samples (stream_voice_upto, models.h).  From then on push()
    // is given the windows' feeds and formats the SHIFTED rows.
    void begin_voice(const StreamVoiceSpec& voice, const std::vector<int64_t>& place, const std::vector<int64_t>& len, std::vector<int64_t> upto,
                     hipStream_t s);
    bool voice() const { return voice_on_; }
    // pinned bytes of a slot whose replays deliver up to cap samples (A included)
    static size_t slot_bytes(const PcmFmtSpec& spec, bool flac, int64_t cap) { return flac ? FlacStreamEncoder::host_bytes(cap) : (size_t)cap * spec.bytes(); }
    // A stream of `joined` native samples whose largest replay delivers cap samples (A included).  Each optional stage is made on first use
    // and reused by later streams; a stage's begin may grow its buffers (synchronises s).  used / offs / place / hop: the rows' token
    // durations and places (marks_spans_rows), read for token levels only.  leveler (needs level): the loudness follower (StreamLeveler,
    // leveler.h) works on y in place between the formatter and the limiter, which then runs at 0 dB under the level's ceiling.
    void begin(const PcmFmtSpec& spec, bool flac, const StreamLevelSpec* level, const StreamMarksSpec* marks, const std::vector<int64_t>& used,
               const std::vector<int64_t>& offs, const int64_t* place, int hop, int64_t joined, int64_t cap, hipStream_t s,
               const StreamLevelerSpec* leveler = nullptr);
    // One replay, enqueued on s: the formatter over its windows (sig[w] = window w), with a level the limiter's push and the cast, the levels
    // and pitch pushes on the delivered samples, then the sink: the encoder's push into `host` or the copy there.  fmt_slot: the formatter's
    // table slot; cap: what `host` was sized for; rec: filled for deliver.
    // A voice stream: feed[w] = window w's native samples and c0 = the replay's first call; the pieces and signals are then made here, from
    // the shifted rows and the delivery rule, and the caller's are not looked at (sig[w].j1 - sig[w].j0 stays what window w fed).
    void push(const std::vector<FmtPiece>& pieces, const std::vector<FmtSignal>& sig, int64_t total, bool last, int fmt_slot, void* host,
              int64_t cap, Slot& rec, hipStream_t s, const std::vector<StreamVoiceFeed>* feed = nullptr, int64_t c0 = 0);
    // Why this stream delivers in order only (something is carried from replay to replay), or nullptr: replays may be enqueued again
    const char* ordered() const;
    // Window w of a replay that has completed -> dst, the stream header in front for call ci = 0 of a FLAC stream.  Too small a buffer is
    // refused before anything is written or counted as delivered: the call can be repeated.
    Taken deliver(const Slot& rec, int64_t w, int64_t ci, void* dst, int64_t capacity_bytes);
    int64_t call_bound(int64_t most) const;   // bytes that suffice for a call of up to `most` fed samples
    void level_stats(double* out, hipStream_t s) const;   // level stream, after its last chunk: 20 log10 min s and max |x| (synchronises s)
    // levelled stream, after its last chunk: L_in, the last / min / max g in dB, then the two of level_stats (synchronises s)
    void leveler_stats(double* out, hipStream_t s) const;
    bool leveler() const { return leveler_on_; }
    bool flac() const { return flac_on_; }
    bool level() const { return level_on_; }
    // the reductions of a stream begun with marks (nullptr otherwise) and the samples the taken calls handed out
    const StreamLevels* levels() const { return levels_on_ ? levels_.get() : nullptr; }
    const StreamPitch* pitch() const { return pitch_on_ ? pitch_.get() : nullptr; }
    int64_t delivered() const { return delivered_; }

  private:
    PcmFmtSpec spec_;
    PcmFormatter fmtr_;   // its table slots: 0 / 1 = the single-window plan's, 2 / 3 = the burst plan's
    std::unique_ptr<FlacStreamEncoder> flac_;
    std::unique_ptr<StreamLimiter> lim_;
    std::unique_ptr<StreamLeveler> lev_;
    std::unique_ptr<StreamLevels> levels_;
    std::unique_ptr<StreamPitch> pitch_;
    std::unique_ptr<StreamVoice> voice_;
    std::vector<FmtPiece> vpieces_;   // a voice stream's pieces: every row's shifted samples at its place
    std::vector<int64_t> vupto_;      // ... and its calls' cumulative delivered samples
    bool voice_on_ = false;
    bool flac_on_ = false, level_on_ = false, leveler_on_ = false, levels_on_ = false, pitch_on_ = false;   // what the running stream uses of them
    int64_t A_ = 0;           // the level's look-ahead in delivered samples (0 without a level)
    int64_t delivered_ = 0;
};

}  // namespace sbv2
