// StreamOutput (stream_output.h): the output side of a running stream, one sequence per replay whatever the stream's kind.
#include "stream_output.h"

#include <cstring>

namespace sbv2 {

int64_t StreamOutput::check(const PcmFmtSpec& spec, const StreamLevelSpec* level, const StreamMarksSpec* marks, int64_t joined) {
    if (marks) StreamLevels::check(nullptr, 0, marks->env_hop, pcm_format_out_len(spec, joined));
    if (marks && marks->pitch) StreamPitch::check(marks->pitch_spec, pcm_format_out_len(spec, joined));
    return level ? stream_level_lookahead(spec.rate) : 0;   // (sizes the slots: a replay may hand back A samples more than it fed)
}

void StreamOutput::begin(const PcmFmtSpec& spec, bool flac, const StreamLevelSpec* level, const StreamMarksSpec* marks, const std::vector<int64_t>& used,
                         const std::vector<int64_t>& offs, const int64_t* place, int hop, int64_t joined, int64_t cap, hipStream_t s,
                         const StreamLevelerSpec* leveler) {
    flac_on_ = level_on_ = leveler_on_ = levels_on_ = pitch_on_ = voice_on_ = false;
    SBV2_REQUIRE(!leveler || level, "a stream leveler needs a level: its ceiling and its starting gain");
    spec_ = spec;
    A_ = level ? stream_level_lookahead(spec.rate) : 0;
    delivered_ = 0;
    const int64_t total_out = pcm_format_out_len(spec_, joined);
    if (flac) {   // the replays' s16 samples go straight behind the encoder's carried tail (push)
        if (!flac_) flac_.reset(new FlacStreamEncoder);
        flac_->begin(spec_.rate, total_out, cap, s);
        flac_on_ = true;
    } else {
        fmtr_.out_buffer((size_t)cap * spec_.bytes(), s);
    }
    if (level) {   // the formatter's y goes behind the limiter's carried tail, what the limiter emits to one of the two sinks above
        if (!lim_) lim_.reset(new StreamLimiter);
        StreamLevelSpec lv = *level;
        if (leveler) {   // the follower starts at the level's gain and owns it from there: the limiter behind it runs at 0 dB under the same ceiling
            if (!lev_) lev_.reset(new StreamLeveler);
            lev_->begin(spec_.rate, total_out, cap, *leveler, level->gain_db, s);
            leveler_on_ = true;
            lv.gain_db = 0.0;
        }
        lim_->begin(spec_.rate, total_out, cap, lv, s);
        level_on_ = true;
    }
    if (marks && (marks->tokens || marks->env_hop > 0)) {
        // the token spans of all rows on the delivered timeline (what sbv2_stream_marks answers) and the frames, fixed before the first replay
        std::vector<int64_t> seg;
        if (marks->tokens) {
            const int64_t ntok = (int64_t)used.size();
            std::vector<int64_t> st((size_t)ntok), en((size_t)ntok);
            marks_spans_rows(used, offs, nullptr, (int64_t)offs.size() - 1, place, hop, spec_, st.data(), en.data());
            seg.resize((size_t)(2 * ntok));
            for (int64_t i = 0; i < ntok; ++i) seg[2 * i] = st[i], seg[2 * i + 1] = en[i];
        }
        if (!levels_) levels_.reset(new StreamLevels);
        levels_->begin(seg.data(), (int64_t)seg.size() / 2, marks->env_hop, total_out, s);
        levels_on_ = true;
    }
    if (marks && marks->pitch) {   // the contour of the same delivered samples: the format's rate (in the spec) and encoding
        if (!pitch_) pitch_.reset(new StreamPitch);
        pitch_->begin(marks->pitch_spec, spec_.encoding, total_out, s);
        pitch_on_ = true;
    }
}

void StreamOutput::begin_voice(const StreamVoiceSpec& voice, const std::vector<int64_t>& place, const std::vector<int64_t>& len,
                               std::vector<int64_t> upto, hipStream_t s) {
    // the rows back to back in the stage's two buffers; the formatter finds row i's shifted samples at place[i] of the timeline
    const int nrows = (int)place.size();
    std::vector<VoiceRow> rows((size_t)nrows);
    int64_t span = 0;
    for (int i = 0; i < nrows; ++i) {
        rows[(size_t)i] = VoiceRow{span, len[(size_t)i]};
        span += len[(size_t)i];
    }
    if (!voice_) voice_.reset(new StreamVoice);
    voice_->begin(voice, rows.data(), nrows, span, s);
    vpieces_.clear();
    for (int i = 0; i < nrows; ++i) vpieces_.push_back(FmtPiece{voice_->out(i), place[(size_t)i], len[(size_t)i]});
    vupto_ = std::move(upto);
    voice_on_ = true;
}

void StreamOutput::push(const std::vector<FmtPiece>& pieces_in, const std::vector<FmtSignal>& sig_in, int64_t total, bool last, int fmt_slot,
                        void* host, int64_t cap, Slot& rec, hipStream_t s, const std::vector<StreamVoiceFeed>* feed, int64_t c0) {
    std::vector<FmtSignal> vsig;
    if (voice_on_) {
        // every window's native samples go through the shifter first; the window then delivers the outputs the delivery rule makes final
        // (vupto_, worked out at begin: nothing here waits for the device), read from the shifted rows
        SBV2_REQUIRE(feed && feed->size() == sig_in.size() && c0 >= 0 && c0 + (int64_t)feed->size() <= (int64_t)vupto_.size(),
                     "internal: a voice stream's replay without its windows' samples");
        total = 0;
        for (size_t w = 0; w < feed->size(); ++w) {
            const StreamVoiceFeed& f = (*feed)[w];
            SBV2_REQUIRE(f.s0 == voice_->fed(f.row), "internal: a voice replay out of stream order (row " + std::to_string(f.row) + ": sample " +
                                                         std::to_string(f.s0) + " after " + std::to_string(voice_->fed(f.row)) + " fed)");
            voice_->push(f.row, f.src, f.s1 - f.s0, s);
            const int64_t c = c0 + (int64_t)w, j0 = c ? vupto_[(size_t)(c - 1)] : 0, j1 = vupto_[(size_t)c];
            vsig.push_back(FmtSignal{j0, j1, total, 0, (int32_t)vpieces_.size()});
            total += j1 - j0;
        }
    }
    const std::vector<FmtPiece>& pieces = voice_on_ ? vpieces_ : pieces_in;
    const std::vector<FmtSignal>& sig = voice_on_ ? vsig : sig_in;
    SBV2_REQUIRE(total + A_ <= cap, "internal: a replay of " + std::to_string(total) + " samples exceeds the slot sized for " + std::to_string(cap));
    rec.host = static_cast<const char*>(host);
    rec.win.clear();
    for (size_t w = 0; w < sig.size(); ++w) rec.win.push_back(Slot::Win{sig[w].out_off, sig[w].j1 - sig[w].j0, sig_in[w].j1 - sig_in[w].j0, 0, 0});
    // the replay's delivered samples are [d0, d0 + n) of the stream; on the device they lie behind the encoder's carried tail or in the formatter's buffer
    void* dev = flac_on_ ? static_cast<void*>(flac_->dst()) : fmtr_.out_buffer((size_t)cap * spec_.bytes(), s);
    const int64_t fed0 = sig.empty() ? 0 : sig[0].j0;
    int64_t d0 = fed0, n = total;
    if (level_on_) {
        // ONE level push per replay: y (f64) behind the limiter's carried tail, then the samples the push completes through the cast /
        // quantiser.  With S samples fed up to a window's end the stream has emitted max(0, S - A), the request's last window
        // everything: window w is handed the samples between its predecessor's count and its own.
        SBV2_REQUIRE(fed0 == lim_->fed(), "internal: a level replay out of stream order (" + std::to_string(fed0) + " samples before it, " +
                                              std::to_string(lim_->fed()) + " fed)");
        d0 = lim_->emitted_after(fed0, false);
        fmtr_.run(spec_, pieces, sig, total, nullptr, fmt_slot, s, GainStage(lim_->dst()));
        if (leveler_on_) lev_->push(lim_->dst(), total, last, s);   // in place, before the limiter reads it
        n = lim_->push(total, last, lim_->out_buffer(), s);
        int64_t at = d0;
        for (size_t w = 0; w < sig.size(); ++w) {
            const int64_t upto = lim_->emitted_after(sig[w].j1, last && w + 1 == sig.size());
            rec.win[w].off = at - d0;
            rec.win[w].n = upto - at;
            at = upto;
        }
        SBV2_REQUIRE(at - d0 == n, "internal: the level stream's counts disagree");
        pcm_cast(lim_->out_buffer(), n, lim_->unit(), spec_.encoding, dev, s);
    } else {
        fmtr_.run(spec_, pieces, sig, total, dev, fmt_slot, s);
    }
    // the reductions read the delivered samples where the sink finds them: pushed BEFORE the encoder's push moves its tail
    if (levels_on_) levels_->push(dev, spec_.encoding, d0, n, s);
    if (pitch_on_) pitch_->push(dev, d0, n, s);
    if (flac_on_) {
        // ONE push per replay: the encoder packs every block that completes (with the request's last chunk also the short final frame);
        // window w completes the frames of the push up to the block its last sample lies in
        const int64_t t0 = flac_->tail();
        rec.flac = flac_->push(n, last, host, s);
        for (size_t w = 0; w < rec.win.size(); ++w) {
            Slot::Win& k = rec.win[w];
            k.fr0 = w ? rec.win[w - 1].fr1 : 0;
            k.fr1 = w + 1 == rec.win.size() ? rec.flac.frames : (int)((t0 + k.off + k.n) / kFlacBlock);
        }
    } else if (n) {
        HIP_CHECK(hipMemcpyAsync(host, dev, (size_t)n * spec_.bytes(), hipMemcpyDeviceToHost, s));
    }
}

const char* StreamOutput::ordered() const {
    return voice_on_    ? "a voice stream delivers its chunks in order only: the shifter carries its phases and marks from chunk to chunk"
           : leveler_on_ ? "a levelled stream delivers its chunks in order only: the leveler carries its meter and its gain from chunk to chunk"
           : level_on_  ? "a level stream delivers its chunks in order only: the limiter carries a tail from chunk to chunk"
           : flac_on_   ? "a FLAC stream delivers its chunks in order only: the encoder carries a tail from chunk to chunk"
           : levels_on_ ? "a stream with levels delivers its chunks in order only: the reduction carries partial sums from chunk to chunk"
           : pitch_on_  ? "a stream with pitch delivers its chunks in order only: the estimator carries the last samples from chunk to chunk"
                        : nullptr;
}

StreamOutput::Taken StreamOutput::deliver(const Slot& rec, int64_t w, int64_t ci, void* dst, int64_t capacity_bytes) {
    SBV2_REQUIRE(w < (int64_t)rec.win.size(), "formatted chunk missing from its replay");
    const Slot::Win& k = rec.win[w];
    const int64_t esz = spec_.bytes();
    Taken t{k.n, k.n * esz, k.fed};
    if (flac_on_) {   // the frames this window completed, the stream header in front of the request's first ones
        const int64_t head = ci == 0 ? kFlacStreamHeader : 0, nb = rec.flac.size(k.fr0, k.fr1);
        SBV2_REQUIRE(capacity_bytes >= head + nb, "FLAC buffer too small for the chunk: " + std::to_string(capacity_bytes) + " < " +
                                                      std::to_string(head + nb) + " bytes (sbv2_flac_stream_bound always suffices)");
        uint8_t* o = static_cast<uint8_t*>(dst);
        if (head) flac_->header(o);
        if (nb) std::memcpy(o + head, rec.flac.bytes + rec.flac.pre[k.fr0], (size_t)nb);
        t.bytes = head + nb;
    } else {
        SBV2_REQUIRE(capacity_bytes >= t.bytes, "PCM buffer too small for the chunk: " + std::to_string(capacity_bytes) + " < " + std::to_string(t.bytes) + " bytes");
        if (k.n) std::memcpy(dst, rec.host + (size_t)k.off * esz, (size_t)t.bytes);
    }
    delivered_ += k.n;
    return t;
}

int64_t StreamOutput::call_bound(int64_t most) const { return flac_on_ ? flac_stream_bound(most + A_) : (most + A_) * spec_.bytes(); }

void StreamOutput::level_stats(double* out, hipStream_t s) const {
    SBV2_REQUIRE(level_on_ && lim_, "this stream was not begun with a level");
    HIP_CHECK(hipStreamSynchronize(s));
    lim_->stats(out);
}

void StreamOutput::leveler_stats(double* out, hipStream_t s) const {
    SBV2_REQUIRE(leveler_on_ && lev_ && lim_, "this stream was not begun with a leveler");
    HIP_CHECK(hipStreamSynchronize(s));
    lev_->stats(out);
    lim_->stats(out + 4);
}

}  // namespace sbv2
