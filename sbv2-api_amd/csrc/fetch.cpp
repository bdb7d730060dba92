// The formatted fetches of a pipeline: output formats (pcm_format.hip), FLAC (flac_encode.hip), loudness (loudness.hip), limiter (limiter.hip) and the
// stages of a request (marks, voice, track, dynamics).  One routine, fetch_formatted, in three phases: plan, enqueue, deliver.
#include <algorithm>
#include <cstring>

#include "api_internal.h"

namespace {   // (nothing here is exported; the entry points are at the end)

// A formatted fetch = a gain stage and a sink.  The gain stage: none (peak-normalise or not, as fmt->normalize says), a loudness gain
// (ln; NULL = measure only) or the look-ahead limiter (lim).  The sink: PCM bytes in fmt's encoding, or one FLAC stream per signal.
struct FetchGain {
    enum Kind { kNone, kLoudness, kLimiter } kind = kNone;
    const sbv2_loudness* ln = nullptr;
    const sbv2_limiter* lim = nullptr;
    int stats_per_signal() const { return kind == kLimiter ? 6 : kind == kLoudness ? 3 : 0; }
};
enum class Sink { kPcm, kFlac };

// What every formatted fetch is given.  place NULL: one signal per utterance; else the run's utterances (or the stages' rows) on one joined
// timeline.  out_counts: samples (PCM) or bytes (FLAC) of each signal; stats (may be NULL): the gain stage's 3 or 6 doubles per signal.
struct FetchArgs {
    sbv2_pipeline* p;
    int64_t ticket;
    const sbv2_pcm_format* fmt;
    FetchGain gain;
    const int64_t* place;
    int64_t joined_len;
    Sink sink;
    void* dst;
    int64_t capacity_bytes;
    int64_t* out_counts;
    double* stats;
};

// The optional stages of a request fetch as the caller gave them (NULL: not asked for); all of them need the request's rows.
// marks, pitch: the speech marks and the pitch contour (marks.h) of the delivered samples, read in HBM on the same stream before the one synchronisation.
// voice (the identity: nothing): the listed rows are shifted first (Voice, voice.h) into the chain's scratch buffer, laid out like the run's packed
// PCM, and the pieces point there; the run's PCM is only read.  token_pitch (all zeros: nothing), formant (scale 1: nothing): the shifter runs whatever
// the voice is, editing the rows' tokens (its token phase) and reading every grain at the scaled offset.
// track (with pitch, or with a shifter that runs): both contours are tracked (Track, track.h) before they are used.
// dynamics (with a loudness or limiter stage; ratio 1: nothing): the compressor runs on y first (dynamics.h); dyn_stats (may be NULL): its 3 doubles.
struct FetchStages {
    const int32_t* utts = nullptr;   // the rows of the one signal (with place[k] belonging to row utts[k]); NULL: no request, all of the run
    int n_utts = 0;
    const sbv2_voice* voice = nullptr;
    const sbv2_pitch_track* track = nullptr;
    const sbv2_dynamics* dynamics = nullptr;
    double* dyn_stats = nullptr;
    const sbv2_token_pitch* token_pitch = nullptr;
    const sbv2_formant* formant = nullptr;
    sbv2_marks* marks = nullptr;
    sbv2_pitch* pitch = nullptr;
};
// ... and once everything about them that needs no run has been checked (check_stages).  Default: no stage.
struct CheckedStages : FetchStages {
    DynamicsSpec dyn;
    VoiceSpec vs;
    FormantSpec fs;
    TrackSpec ts;
    PitchSpec ps;
    bool edit = false, scale = false, compress = false;   // a token is edited; the formants move; the compressor is not the identity
    bool shifts() const { return (voice && !vs.identity()) || edit || scale; }   // the shifter has something to do
};

PcmFmtSpec fetch_spec(const sbv2_pcm_format* fmt, bool gain_stage, Sink sink) {
    const PcmFmtSpec spec = pcm_format_spec(fmt);
    if (gain_stage) SBV2_REQUIRE(!spec.normalize, "loudness normalisation replaces peak normalisation: fmt->normalize must be 0");
    if (sink == Sink::kFlac) SBV2_REQUIRE(spec.encoding == kEncS16, "FLAC needs encoding = 1 (s16): f32 samples and G.711 codes have no FLAC form");
    return spec;
}

// the checks of sbv2_marks that need no run
void check_marks_static(const sbv2_marks* m) {
    SBV2_REQUIRE(m->reserved == 0, "sbv2_marks.reserved must be 0");
    SBV2_REQUIRE(m->env_hop >= 0, "sbv2_marks.env_hop must be >= 0: " + std::to_string(m->env_hop));
    SBV2_REQUIRE(m->env_hop == 0 || (m->env_sumsq && m->env_peak), "sbv2_marks.env_hop > 0 needs env_sumsq and env_peak");
    SBV2_REQUIRE(!m->tok_sumsq == !m->tok_peak, "sbv2_marks.tok_sumsq and tok_peak are given together or not at all");
    SBV2_REQUIRE(m->tok_capacity >= 0 && m->env_capacity >= 0, "negative sbv2_marks capacity");
}

// The checks of sbv2_pitch that need no run: the parameters at the delivered rate (marks.h states the bounds), the arrays.
PitchSpec check_pitch_static(const sbv2_pitch* q, int rate) {
    SBV2_REQUIRE(q->reserved == 0, "sbv2_pitch.reserved must be 0");
    const PitchSpec sp = pitch_spec(rate, q->hop, q->f0_min, q->f0_max, q->threshold);
    SBV2_REQUIRE(q->capacity >= 0, "negative sbv2_pitch capacity");
    SBV2_REQUIRE(q->f0, "sbv2_pitch.f0 must not be NULL");
    return sp;
}

// The checks of sbv2_voice that need no run: the parameters at the rate of the rows (voice.h states the bounds).
VoiceSpec check_voice_static(const sbv2_voice* v, int rate) {
    SBV2_REQUIRE(v->reserved == 0, "sbv2_voice.reserved must be 0");
    return voice_spec(rate, v->pitch_scale, v->intonation_scale, v->hop, v->f0_min, v->f0_max, v->threshold);
}

// The checks of sbv2_token_pitch that need no run (voice.h states the bounds; vs: the voice's checked parameters, the defaults without a voice)
// -> whether any token is edited.
bool check_token_pitch_static(const sbv2_token_pitch* t, const VoiceSpec& vs) {
    SBV2_REQUIRE(t->reserved == 0, "sbv2_token_pitch.reserved must be 0");
    SBV2_REQUIRE(t->n_tokens >= 0, "sbv2_token_pitch.n_tokens must be >= 0: " + std::to_string(t->n_tokens));
    SBV2_REQUIRE(t->value || t->n_tokens == 0, "sbv2_token_pitch.value must not be NULL");
    voice_tokens_check(t->value, t->n_tokens, t->kind, t->smooth, vs);
    for (int64_t i = 0; i < t->n_tokens; ++i)
        if (t->value[i] != 0.0) return true;
    return false;
}

// The checks of sbv2_formant that need no run (formant_spec of voice.h holds them; vs as above) -> the scale and the gather's widened range.
FormantSpec check_formant_static(const sbv2_formant* f, const VoiceSpec& vs) { return formant_spec(f->formant_scale, f->reserved, vs); }

// The checks of sbv2_pitch_track (track.h states the bounds).
TrackSpec check_track_static(const sbv2_pitch_track* t) {
    SBV2_REQUIRE(t->reserved[0] == 0 && t->reserved[1] == 0, "sbv2_pitch_track.reserved must be 0");
    return track_spec(t->cand_max, t->unvoiced_cost, t->switch_cost, t->jump_cost);
}

// Everything about a request and its stages that needs no run, refused in this order before the handle is looked at: the stages' parameters, the
// request itself, then marks and pitch with the format they are delivered in.  The one place these checks run.
CheckedStages check_stages(const sbv2_fetch_request* req, const FetchStages& st) {
    CheckedStages cs{st};
    if (st.dynamics) cs.dyn = dynamics_spec(st.dynamics);
    cs.compress = st.dynamics && !cs.dyn.identity();
    cs.vs = st.voice ? check_voice_static(st.voice, kNativeRate) : voice_spec(kNativeRate, 1.0, 1.0, 0, 0.0, 0.0, 0.0);   // (or the defaults)
    cs.edit = st.token_pitch && check_token_pitch_static(st.token_pitch, cs.vs);
    if (st.formant) cs.fs = check_formant_static(st.formant, cs.vs);
    cs.scale = st.formant && !cs.fs.identity();
    if (st.track) {
        cs.ts = check_track_static(st.track);
        SBV2_REQUIRE(st.pitch || cs.shifts(), "pitch tracking needs a pitch contour or a voice that is not the identity");
    }
    SBV2_REQUIRE(req && req->n_utts >= 0 && (req->n_utts == 0 || (req->utts && req->place)), "bad fetch request");
    SBV2_REQUIRE(!(req->loudness && req->limiter), "a fetch request takes a loudness target or a limiter, not both");
    if (cs.compress)   // (fmt->normalize is then refused with the gain stage it needs)
        SBV2_REQUIRE(req->loudness || req->limiter,
                     "a compressor needs a loudness target or a limiter behind it: without make-up it only makes the signal quieter");
    if (st.marks) {
        check_marks_static(st.marks);
        (void)pcm_format_spec(req->fmt);
    }
    if (st.pitch) cs.ps = check_pitch_static(st.pitch, pcm_format_spec(req->fmt).rate);
    return cs;
}

// The signals of a formatted fetch: one per utterance (place == NULL), or the run's utterances on one joined timeline.  outs = output samples
// of each signal; the result is `total` samples.
// utts != NULL: the joined timeline holds those n_utts rows only, place[k] belonging to row utts[k] (sbv2_pipeline_fetch_request).
void format_layout(const PcmFmtSpec& spec, VitsModel& vm, const int32_t* utts, int n_utts, const int64_t* place, int64_t joined_len,
                          std::vector<FmtPiece>* pieces, std::vector<FmtSignal>* sig, std::vector<int64_t>* outs, int64_t* total) {
    const std::vector<int64_t>& lens = vm.pcm_lens();
    const std::vector<int64_t>& offs = vm.pcm_offs();
    const int n = (int)lens.size();
    const float* pcm = vm.pcm_device();
    *total = 0;
    if (!place) {
        for (int i = 0; i < n; ++i) {
            const int64_t j1 = pcm_format_out_len(spec, lens[i]);
            pieces->push_back(FmtPiece{pcm + offs[i], 0, lens[i]});
            sig->push_back(FmtSignal{0, j1, *total, i, i + 1});
            outs->push_back(j1);
            *total += j1;
        }
        return;
    }
    SBV2_REQUIRE(joined_len >= 0, "joined_len must be >= 0");
    const int m = utts ? n_utts : n;   // entry k of place belongs to row row(k)
    const auto row = [&](int k) { return utts ? (int)utts[k] : k; };
    if (utts) {
        std::vector<char> seen(n, 0);
        for (int k = 0; k < m; ++k) {
            SBV2_REQUIRE(utts[k] >= 0 && utts[k] < n, "row " + std::to_string(utts[k]) + " is outside the run's " + std::to_string(n) + " utterances");
            SBV2_REQUIRE(!seen[utts[k]], "row " + std::to_string(utts[k]) + " is listed twice");
            seen[utts[k]] = 1;
        }
    }
    std::vector<int> order(m);
    for (int k = 0; k < m; ++k) {
        order[k] = k;
        SBV2_REQUIRE(place[k] >= 0 && place[k] + lens[row(k)] <= joined_len,
                     "placement of utterance " + std::to_string(row(k)) + " (" + std::to_string(place[k]) + " + " + std::to_string(lens[row(k)]) +
                         " samples) is outside the joined timeline of " + std::to_string(joined_len) + " samples");
    }
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return place[a] < place[b]; });
    for (int r = 0; r < m; ++r) {
        const int k = order[r], i = row(k);
        if (r) SBV2_REQUIRE(place[order[r - 1]] + lens[row(order[r - 1])] <= place[k], "placements of utterances overlap on the joined timeline");
        if (lens[i]) pieces->push_back(FmtPiece{pcm + offs[i], place[k], lens[i]});
    }
    *total = pcm_format_out_len(spec, joined_len);
    sig->push_back(FmtSignal{0, *total, 0, 0, (int32_t)pieces->size()});
    outs->push_back(*total);
}

// The speech marks of a request fetch (marks.h), planned on the host before anything is enqueued: the listed rows' token spans on the delivered
// timeline and the segment table of the level reduction (the token spans when levels are asked for, then the envelope frames).
struct MarksPlan {
    std::vector<int64_t> start, end;   // per token, in the order of the request's rows
    std::vector<int64_t> seg;          // [levels ? n_tok : 0][2], then [n_env][2]
    int64_t n_tok = 0, n_env = 0;
    bool levels = false, reduce = false;   // reduce: the level reduction runs: there are segments and samples (else every level is 0, without a launch)
};
MarksPlan plan_marks(const sbv2_marks* m, const PcmFmtSpec& spec, const VitsModel& vm, const int32_t* utts, int n_utts, const int64_t* place,
                            int64_t n_tok, int64_t total) {
    MarksPlan mp;
    mp.n_tok = n_tok;
    SBV2_REQUIRE(m->tok_capacity >= mp.n_tok,
                 "token arrays too small: " + std::to_string(m->tok_capacity) + " < " + std::to_string(mp.n_tok) + " tokens");
    SBV2_REQUIRE(mp.n_tok == 0 || (m->tok_start && m->tok_end), "sbv2_marks.tok_start and tok_end must not be NULL");
    if (m->env_hop > 0) {
        mp.n_env = (total + m->env_hop - 1) / m->env_hop;
        SBV2_REQUIRE(m->env_capacity >= mp.n_env,
                     "envelope arrays too small: " + std::to_string(m->env_capacity) + " < " + std::to_string(mp.n_env) + " frames");
    }
    mp.levels = m->tok_sumsq != nullptr;
    mp.start.resize((size_t)mp.n_tok);
    mp.end.resize((size_t)mp.n_tok);
    marks_spans_rows(vm.used_durations(), vm.used_offs(), utts, n_utts, place, vm.cfg().hop(), spec, mp.start.data(), mp.end.data());
    mp.seg.reserve((size_t)(2 * ((mp.levels ? mp.n_tok : 0) + mp.n_env)));
    if (mp.levels)
        for (int64_t t = 0; t < mp.n_tok; ++t) mp.seg.push_back(mp.start[t]), mp.seg.push_back(mp.end[t]);
    for (int64_t f = 0; f < mp.n_env; ++f) mp.seg.push_back(f * m->env_hop), mp.seg.push_back(std::min((f + 1) * (int64_t)m->env_hop, total));
    mp.reduce = !mp.seg.empty() && total > 0;
    return mp;
}

// Phase 1 of a fetch, host only: what will run, on what, into how many bytes.  Every refusal that needs the run is here (the format against the
// gain stage and the sink, the gain's parameters, the ticket, the layout, PCM capacity, the marks' and the contour's capacity, the token count), so
// nothing is enqueued before every check has passed.  (The FLAC sink alone checks its capacity after encoding, when the sizes are known.)
struct FetchPlan {
    PcmFmtSpec spec;
    LoudnessSpec ln;
    LimiterSpec lim;
    int ctx = 0;
    std::vector<FmtPiece> pieces;
    std::vector<FmtSignal> sig;
    std::vector<int64_t> outs;   // per signal: samples
    int64_t total = 0, pcm_bytes = 0, n_pitch = 0;   // delivered samples and their bytes; frames of the contour
    MarksPlan marks;
    std::vector<int64_t> tok_counts, tok_ends;   // (an edit only) per listed row: its tokens; per token: the native sample it ends at
    bool shift = false;                          // the shifter runs
};
FetchPlan plan_fetch(const FetchArgs& a, const CheckedStages& cs) {
    FetchPlan pl;
    pl.spec = fetch_spec(a.fmt, a.gain.kind != FetchGain::kNone, a.sink);
    if (a.gain.kind == FetchGain::kLoudness) pl.ln = loudness_spec(a.gain.ln);
    if (a.gain.kind == FetchGain::kLimiter) pl.lim = limiter_spec(a.gain.lim);
    pl.ctx = a.p->ctx_of(a.ticket);
    VitsModel& vm = a.p->vm(pl.ctx);
    format_layout(pl.spec, vm, cs.utts, cs.n_utts, a.place, a.joined_len, &pl.pieces, &pl.sig, &pl.outs, &pl.total);
    pl.pcm_bytes = pl.total * pl.spec.bytes();
    if (a.sink == Sink::kPcm)
        SBV2_REQUIRE(a.capacity_bytes >= pl.pcm_bytes,
                     "PCM buffer too small: " + std::to_string(a.capacity_bytes) + " < " + std::to_string(pl.pcm_bytes) + " bytes");
    const std::vector<int64_t>& offs = vm.used_offs();
    int64_t n_tok = 0;   // the tokens of the listed rows, for marks and token pitch alike
    if (cs.marks || cs.token_pitch) {
        SBV2_REQUIRE(offs.size() == vm.pcm_lens().size() + 1, "internal: the run kept no durations");
        for (int k = 0; k < cs.n_utts; ++k) n_tok += offs[cs.utts[k] + 1] - offs[cs.utts[k]];
    }
    if (cs.marks) pl.marks = plan_marks(cs.marks, pl.spec, vm, cs.utts, cs.n_utts, a.place, n_tok, pl.total);
    if (cs.pitch) {
        pl.n_pitch = pitch_frames(pl.total, cs.ps.hop);
        SBV2_REQUIRE(cs.pitch->capacity >= pl.n_pitch,
                     "pitch arrays too small: " + std::to_string(cs.pitch->capacity) + " < " + std::to_string(pl.n_pitch) + " frames");
    }
    if (cs.token_pitch)
        SBV2_REQUIRE(cs.token_pitch->n_tokens == n_tok, "sbv2_token_pitch.n_tokens is " + std::to_string(cs.token_pitch->n_tokens) +
                                                            " but the listed rows have " + std::to_string(n_tok) + " tokens");
    if (cs.edit) {   // token t of a row ends at hop c[t + 1]
        pl.tok_ends.reserve((size_t)n_tok);
        for (int k = 0; k < cs.n_utts; ++k) {
            pl.tok_counts.push_back(offs[cs.utts[k] + 1] - offs[cs.utts[k]]);
            int64_t c = 0;
            for (int64_t e = offs[cs.utts[k]]; e < offs[cs.utts[k] + 1]; ++e)
                pl.tok_ends.push_back((c += vm.used_durations()[(size_t)e]) * vm.cfg().hop());
        }
    }
    pl.shift = cs.shifts() && cs.n_utts > 0;
    return pl;
}

// Phase 2: the run's packed PCM (pcm_device + pcm_offs / pcm_lens) is formatted on the run's own stream and crosses PCIe in the format: the shifter,
// the formatter's launches with the gain stage between the resampler and the quantiser, marks and pitch on the delivered samples, the sink's copy,
// and the one synchronisation of the fetch.  Writes dst and nothing else of the caller's.  -> per signal, the bytes of its FLAC stream (that sink only)
std::vector<int64_t> enqueue_fetch(const FetchArgs& a, const CheckedStages& cs, FetchPlan& pl) {
    const PcmFmtSpec& spec = pl.spec;
    VitsModel& vm = a.p->vm(pl.ctx);
    std::vector<int64_t> flac_bytes;
    HIP_CHECK(hipSetDevice(vm.device()));
    OutputChain& c = a.p->chains[pl.ctx];
    const hipStream_t s = vm.stream();
    const TrackSpec* const ts = cs.track ? &cs.ts : nullptr;
    if (pl.shift) {   // the listed rows, shifted, where the formatter will read them
        std::vector<VoiceRow> rows((size_t)cs.n_utts);
        for (int k = 0; k < cs.n_utts; ++k) rows[k] = VoiceRow{vm.pcm_offs()[cs.utts[k]], vm.pcm_lens()[cs.utts[k]]};
        const float* pcm = vm.pcm_device();
        const sbv2_token_pitch* tp = cs.token_pitch;
        const VoiceTokens vt{pl.tok_counts.data(), pl.tok_ends.data(), cs.edit ? tp->value : nullptr, cs.edit ? tp->kind : 0, cs.edit ? tp->smooth : 0};
        const float* shifted = c.voice.run(pcm, vm.pcm_total(), rows.data(), cs.n_utts, cs.vs, s, nullptr, nullptr, ts, cs.edit ? &vt : nullptr,
                                           cs.scale ? &cs.fs : nullptr);
        for (FmtPiece& pc : pl.pieces) pc.src = shifted + (pc.src - pcm);
    }
    if (a.sink == Sink::kPcm && a.gain.kind == FetchGain::kNone && spec.identity() && !a.place) {   // the bytes of sbv2_pipeline_fetch_pcm_ticket
        HIP_CHECK(hipMemcpyAsync(a.dst, vm.pcm_device(), sizeof(float) * (size_t)vm.pcm_total(), hipMemcpyDeviceToHost, s));
    } else if (pl.total > 0 || a.gain.kind != FetchGain::kNone || a.sink == Sink::kFlac) {   // a gain stage and the encoder run on empty signals too
        void* dev = c.formatter.out_buffer((size_t)std::max<int64_t>(pl.pcm_bytes, spec.bytes()), s);
        Dynamics* const dy = cs.compress ? &c.dynamics : nullptr;
        const GainStage stage = a.gain.kind == FetchGain::kLimiter    ? GainStage(c.meter, c.limiter, pl.lim, dy, &cs.dyn)
                                : a.gain.kind == FetchGain::kLoudness ? GainStage(c.meter, pl.ln, dy, &cs.dyn)
                                                                      : GainStage();
        c.formatter.run(spec, pl.pieces, pl.sig, pl.total, dev, 0, s, stage);
        // marks and pitch read the delivered samples, as they cross PCIe or enter the encoder
        if (pl.marks.reduce) c.marks.run(dev, spec.encoding, pl.total, pl.marks.seg.data(), (int64_t)pl.marks.seg.size() / 2, s);
        if (pl.n_pitch > 0) c.pitch.run(dev, spec.encoding, pl.total, cs.ps, s, ts, cs.track ? &c.track : nullptr);
        if (a.sink == Sink::kFlac) {   // the signals stay in HBM; the encoder reads the stream sizes back, then exactly the encoded bytes cross PCIe
            std::vector<int64_t> offs(pl.outs.size());
            for (size_t i = 1; i < pl.outs.size(); ++i) offs[i] = offs[i - 1] + pl.outs[i - 1];
            const int64_t nbytes = c.flac.encode(static_cast<const int16_t*>(dev), offs, pl.outs, spec.rate, s, &flac_bytes);
            SBV2_REQUIRE(a.capacity_bytes >= nbytes,
                         "FLAC buffer too small: " + std::to_string(a.capacity_bytes) + " < " + std::to_string(nbytes) + " bytes");
            HIP_CHECK(hipMemcpyAsync(a.dst, c.flac.output(), (size_t)nbytes, hipMemcpyDeviceToHost, s));
        } else if (pl.total > 0) {
            HIP_CHECK(hipMemcpyAsync(a.dst, dev, (size_t)pl.pcm_bytes, hipMemcpyDeviceToHost, s));
        }
    }
    HIP_CHECK(hipStreamSynchronize(s));
    if (pl.shift)
        for (int k = 0; k < cs.n_utts; ++k) SBV2_REQUIRE(c.voice.status(k) == 0, "internal: the shifter found more marks than it planned for");
    return flac_bytes;
}

// Phase 3, once everything else has succeeded: the counts, the stats, and the caller's marks, pitch and token-pitch arrays, from the chain's pinned
// buffers.  Nothing here can fail.
void deliver_fetch(const FetchArgs& a, const CheckedStages& cs, const FetchPlan& pl, const std::vector<int64_t>& flac_bytes) {
    OutputChain& c = a.p->chains[pl.ctx];
    for (size_t i = 0; i < pl.outs.size(); ++i) a.out_counts[i] = a.sink == Sink::kFlac ? flac_bytes[i] : pl.outs[i];
    if (a.stats) {   // written by the stage's last copy on the stream
        const double* from = a.gain.kind == FetchGain::kLimiter ? c.limiter.stats_host() : c.meter.stats_host();
        std::memcpy(a.stats, from, sizeof(double) * a.gain.stats_per_signal() * pl.sig.size());
    }
    if (cs.dyn_stats && cs.compress) std::memcpy(cs.dyn_stats, c.dynamics.stats_host(), sizeof(double) * 3 * pl.sig.size());
    if (sbv2_marks* marks = cs.marks) {
        const MarksPlan& mp = pl.marks;
        std::copy(mp.start.begin(), mp.start.end(), marks->tok_start);
        std::copy(mp.end.begin(), mp.end.end(), marks->tok_end);
        const int64_t nt = mp.levels ? mp.n_tok : 0;
        const auto level = [&](bool peak, int64_t i) { return !mp.reduce ? 0.0 : (peak ? c.marks.peak_host() : c.marks.sumsq_host())[i]; };
        for (int64_t t = 0; t < nt; ++t) marks->tok_sumsq[t] = level(false, t), marks->tok_peak[t] = level(true, t);
        for (int64_t f = 0; f < mp.n_env; ++f) marks->env_sumsq[f] = level(false, nt + f), marks->env_peak[f] = level(true, nt + f);
        marks->n_tokens = mp.n_tok;
        marks->n_env = mp.n_env;
    }
    if (const sbv2_token_pitch* tp = cs.token_pitch) {   // (all zeros: nothing was measured)
        const bool ran = cs.edit && pl.shift;
        for (int64_t t = 0; t < tp->n_tokens; ++t) {
            if (tp->applied) tp->applied[t] = ran ? c.voice.applied_host()[t] : 1.0;
            if (tp->src_f0) tp->src_f0[t] = ran ? c.voice.src_f0_host()[t] : 0.0;
        }
    }
    if (sbv2_pitch* pitch = cs.pitch) {   // (an empty signal has no frames and ran nothing)
        for (int64_t f = 0; f < pl.n_pitch; ++f) {
            const int32_t lag = c.pitch.lag_host()[f];
            pitch_finish(cs.ps, lag, c.pitch.voiced_host()[f], c.pitch.c3_host() + 3 * f, pitch->f0 + f, pitch->ap ? pitch->ap + f : nullptr);
            if (pitch->lag) pitch->lag[f] = lag;
        }
        pitch->n_frames = pl.n_pitch;
    }
}

void fetch_formatted(const FetchArgs& a, const CheckedStages& cs) {
    SBV2_REQUIRE(a.p && a.dst && a.out_counts, "bad arguments");
    FetchPlan pl = plan_fetch(a, cs);
    deliver_fetch(a, cs, pl, enqueue_fetch(a, cs, pl));
}

// The fetches of a whole run: no request, no stage.
int fetch_run(sbv2_pipeline* p, int64_t ticket, const sbv2_pcm_format* fmt, FetchGain gain, const int64_t* place, int64_t joined_len, Sink sink, void* dst,
              int64_t capacity_bytes, int64_t* out_counts, double* stats) {
    API_BEGIN
    fetch_formatted({p, ticket, fmt, gain, place, joined_len, sink, dst, capacity_bytes, out_counts, stats}, CheckedStages());
    API_END
}

}  // namespace

extern "C" {

int sbv2_pipeline_fetch_pcm_format(sbv2_pipeline* p, int64_t ticket, const sbv2_pcm_format* fmt, const int64_t* place, int64_t joined_len,
                                   void* dst, int64_t capacity_bytes, int64_t* out_lens) {
    return fetch_run(p, ticket, fmt, FetchGain(), place, joined_len, Sink::kPcm, dst, capacity_bytes, out_lens, nullptr);
}

int64_t sbv2_flac_bound(const sbv2_pcm_format* fmt, int64_t n_native) {
    try {
        const PcmFmtSpec spec = fetch_spec(fmt, false, Sink::kFlac);
        SBV2_REQUIRE(n_native >= 0, "negative sample count");
        return flac_bound(pcm_format_out_len(spec, n_native));
    } catch (const std::exception& e) {
        set_last_error(e.what());
        return -1;
    }
}

int sbv2_pipeline_fetch_flac(sbv2_pipeline* p, int64_t ticket, const sbv2_pcm_format* fmt, const int64_t* place, int64_t joined_len, uint8_t* dst,
                             int64_t capacity_bytes, int64_t* out_bytes) {
    return fetch_run(p, ticket, fmt, FetchGain(), place, joined_len, Sink::kFlac, dst, capacity_bytes, out_bytes, nullptr);
}

int sbv2_pipeline_fetch_pcm_loudness(sbv2_pipeline* p, int64_t ticket, const sbv2_pcm_format* fmt, const sbv2_loudness* ln, const int64_t* place,
                                     int64_t joined_len, void* dst, int64_t capacity_bytes, int64_t* out_lens, double* stats) {
    return fetch_run(p, ticket, fmt, {FetchGain::kLoudness, ln, nullptr}, place, joined_len, Sink::kPcm, dst, capacity_bytes, out_lens, stats);
}

int sbv2_pipeline_fetch_flac_loudness(sbv2_pipeline* p, int64_t ticket, const sbv2_pcm_format* fmt, const sbv2_loudness* ln, const int64_t* place,
                                      int64_t joined_len, uint8_t* dst, int64_t capacity_bytes, int64_t* out_bytes, double* stats) {
    return fetch_run(p, ticket, fmt, {FetchGain::kLoudness, ln, nullptr}, place, joined_len, Sink::kFlac, dst, capacity_bytes, out_bytes, stats);
}

int sbv2_pipeline_fetch_pcm_limited(sbv2_pipeline* p, int64_t ticket, const sbv2_pcm_format* fmt, const sbv2_limiter* lim, const int64_t* place,
                                    int64_t joined_len, void* dst, int64_t capacity_bytes, int64_t* out_lens, double* stats) {
    return fetch_run(p, ticket, fmt, {FetchGain::kLimiter, nullptr, lim}, place, joined_len, Sink::kPcm, dst, capacity_bytes, out_lens, stats);
}

int sbv2_pipeline_fetch_flac_limited(sbv2_pipeline* p, int64_t ticket, const sbv2_pcm_format* fmt, const sbv2_limiter* lim, const int64_t* place,
                                     int64_t joined_len, uint8_t* dst, int64_t capacity_bytes, int64_t* out_bytes, double* stats) {
    return fetch_run(p, ticket, fmt, {FetchGain::kLimiter, nullptr, lim}, place, joined_len, Sink::kFlac, dst, capacity_bytes, out_bytes, stats);
}

// The widest request fetch; each narrower symbol below is exactly this call with NULL for what it lacks.
int sbv2_pipeline_fetch_request_formant(sbv2_pipeline* p, int64_t ticket, const sbv2_fetch_request* req, const sbv2_voice* voice,
                                        const sbv2_pitch_track* track, const sbv2_dynamics* dynamics, const sbv2_token_pitch* token_pitch,
                                        const sbv2_formant* formant, void* dst, int64_t capacity_bytes, int64_t* out_count, double* stats,
                                        double* dyn_stats, sbv2_marks* marks, sbv2_pitch* pitch) {
    API_BEGIN
    static const int32_t no_rows[1] = {0};   // (a request of no rows is still a request: one empty joined signal)
    static const int64_t no_place[1] = {0};
    const bool rows = req && req->n_utts > 0;   // (what is wrong with req is refused in its turn, by check_stages)
    const CheckedStages cs = check_stages(
        req, FetchStages{rows ? req->utts : no_rows, rows ? req->n_utts : 0, voice, track, dynamics, dyn_stats, token_pitch, formant, marks, pitch});
    const FetchGain gain = req->limiter    ? FetchGain{FetchGain::kLimiter, nullptr, req->limiter}
                           : req->loudness ? FetchGain{FetchGain::kLoudness, req->loudness, nullptr}
                                           : FetchGain();
    const Sink sink = req->flac ? Sink::kFlac : Sink::kPcm;
    fetch_formatted({p, ticket, req->fmt, gain, rows ? req->place : no_place, req->joined_len, sink, dst, capacity_bytes, out_count, stats}, cs);
    API_END
}
int sbv2_pipeline_fetch_request_token_pitch(sbv2_pipeline* p, int64_t ticket, const sbv2_fetch_request* req, const sbv2_voice* voice,
                                            const sbv2_pitch_track* track, const sbv2_dynamics* dynamics, const sbv2_token_pitch* token_pitch,
                                            void* dst, int64_t capacity_bytes, int64_t* out_count, double* stats, double* dyn_stats,
                                            sbv2_marks* marks, sbv2_pitch* pitch) {
    return sbv2_pipeline_fetch_request_formant(p, ticket, req, voice, track, dynamics, token_pitch, nullptr, dst, capacity_bytes, out_count, stats,
                                               dyn_stats, marks, pitch);
}
int sbv2_pipeline_fetch_request_dynamics(sbv2_pipeline* p, int64_t ticket, const sbv2_fetch_request* req, const sbv2_voice* voice,
                                         const sbv2_pitch_track* track, const sbv2_dynamics* dynamics, void* dst, int64_t capacity_bytes,
                                         int64_t* out_count, double* stats, double* dyn_stats, sbv2_marks* marks, sbv2_pitch* pitch) {
    return sbv2_pipeline_fetch_request_token_pitch(p, ticket, req, voice, track, dynamics, nullptr, dst, capacity_bytes, out_count, stats, dyn_stats,
                                                   marks, pitch);
}
int sbv2_pipeline_fetch_request_tracked(sbv2_pipeline* p, int64_t ticket, const sbv2_fetch_request* req, const sbv2_voice* voice,
                                        const sbv2_pitch_track* track, void* dst, int64_t capacity_bytes, int64_t* out_count, double* stats,
                                        sbv2_marks* marks, sbv2_pitch* pitch) {
    return sbv2_pipeline_fetch_request_dynamics(p, ticket, req, voice, track, nullptr, dst, capacity_bytes, out_count, stats, nullptr, marks, pitch);
}
int sbv2_pipeline_fetch_request_voice(sbv2_pipeline* p, int64_t ticket, const sbv2_fetch_request* req, const sbv2_voice* voice, void* dst,
                                      int64_t capacity_bytes, int64_t* out_count, double* stats, sbv2_marks* marks, sbv2_pitch* pitch) {
    return sbv2_pipeline_fetch_request_tracked(p, ticket, req, voice, nullptr, dst, capacity_bytes, out_count, stats, marks, pitch);
}
int sbv2_pipeline_fetch_request_pitch(sbv2_pipeline* p, int64_t ticket, const sbv2_fetch_request* req, void* dst, int64_t capacity_bytes,
                                      int64_t* out_count, double* stats, sbv2_marks* marks, sbv2_pitch* pitch) {
    return sbv2_pipeline_fetch_request_voice(p, ticket, req, nullptr, dst, capacity_bytes, out_count, stats, marks, pitch);
}
int sbv2_pipeline_fetch_request_marks(sbv2_pipeline* p, int64_t ticket, const sbv2_fetch_request* req, void* dst, int64_t capacity_bytes,
                                      int64_t* out_count, double* stats, sbv2_marks* marks) {
    return sbv2_pipeline_fetch_request_pitch(p, ticket, req, dst, capacity_bytes, out_count, stats, marks, nullptr);
}
int sbv2_pipeline_fetch_request(sbv2_pipeline* p, int64_t ticket, const sbv2_fetch_request* req, void* dst, int64_t capacity_bytes, int64_t* out_count,
                                double* stats) {
    return sbv2_pipeline_fetch_request_marks(p, ticket, req, dst, capacity_bytes, out_count, stats, nullptr);
}

}  // extern "C"
