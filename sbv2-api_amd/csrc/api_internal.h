// Shared by the translation units behind the C ABI (api.cpp, fetch.cpp, test_hooks.cpp, node.cpp, stream.cpp): handle structs and the exception -> return-code
// convention.  Not installed; include/sbv2_hip.h is the public contract.
#pragma once
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>

#include "../../include/sbv2_hip.h"
#include "dynamics.h"
#include "flac_encode.h"
#include "limiter.h"
#include "loudness.h"
#include "marks.h"
#include "models.h"
#include "pcm_format.h"
#include "track.h"
#include "voice.h"

namespace sbv2 {
const char* last_error_cstr();
}
using namespace sbv2;

struct sbv2_bert {
    std::unique_ptr<BertModel> m;
};
struct sbv2_vits {
    std::unique_ptr<VitsModel> m;
};
// The output chain of one execution context: what the formatted fetches (fetch_formatted, fetch.cpp) launch on that context's stream.  Every
// member grows its device and pinned buffers on first use and holds none before: a pipeline that never asks for FLAC or a limiter pays
// nothing for them, and creating the pipeline allocates nothing here.
struct OutputChain {
    PcmFormatter formatter;
    FlacEncoder flac;
    LoudnessMeter meter;
    Limiter limiter;   // (owns a second meter, for its evaluations)
    Dynamics dynamics; // the speech compressor in front of the loudness gain or the limiter (fetch_request_dynamics only)
    Marks marks;       // speech marks: levels of token spans and envelope frames (fetch_request_marks only)
    Pitch pitch;       // ... and the pitch contour of the same samples (fetch_request_pitch only)
    Voice voice;       // pitch / intonation scale of the listed rows, in front of the formatter (fetch_request_voice only)
    Track track;       // the best path through the delivered contour's candidates (fetch_request_tracked only; the shifter has its own)
};
struct sbv2_pipeline {
    sbv2_bert* bert;
    sbv2_vits* vits;
    // execution contexts: context 0 is the caller's pair of handles, the others are clones (shared weights, own stream + arena)
    std::vector<std::unique_ptr<BertModel>> bclones;
    std::vector<std::unique_ptr<VitsModel>> vclones;
    std::vector<OutputChain> chains;   // one per context
    int64_t calls = 0;   // tickets are call numbers 1, 2, ...: ticket t ran on context (t - 1) % depth and is valid until that context is reused
    BertModel& bm(int i) { return i == 0 ? *bert->m : *bclones[i - 1]; }
    VitsModel& vm(int i) { return i == 0 ? *vits->m : *vclones[i - 1]; }
    int contexts() const { return 1 + (int)vclones.size(); }
    // context of a ticket; throws for tickets never issued or already overwritten by a later run on the same context
    int ctx_of(int64_t ticket) const {
        SBV2_REQUIRE(ticket >= 1 && ticket <= calls, "unknown pipeline ticket");
        SBV2_REQUIRE(ticket > calls - contexts(), "stale pipeline ticket: its execution context has been reused by a later run");
        return (int)((ticket - 1) % contexts());
    }
};

#define API_BEGIN try {
#define API_END                                   \
    return 0;                                     \
    }                                             \
    catch (const std::exception& e) {             \
        set_last_error(e.what());                 \
        return 1;                                 \
    }                                             \
    catch (...) {                                 \
        set_last_error("unknown error");          \
        return 1;                                 \
    }

VitsBatch to_batch(const sbv2_batch* b);
// The per-row arrays of sbv2_utt_options onto the batch (NULL: nothing); throws for an option out of range, before any GPU work
void apply_utt_options(sbv2::VitsBatch* v, const sbv2_utt_options* o);
// One batch on one execution context: bert::predict -> word2ph repeat (tts_util.rs:129-154) -> model::synthesize; returns once enqueued
// What a run carries of an sbv2_assist (the contract above the struct, include/sbv2_hip.h): A = 0 when there is none or no row names a text
struct AssistSpec {
    int A = 0;
    const int64_t* ids = nullptr;    // the A sequences back to back, `total` ids
    const int64_t* lens = nullptr;   // [A]
    int64_t total = 0;
    std::vector<sbv2::AssistRow> rows;   // [n]: the row's text and f32 weights (mean_row -1: none, or a weight of 0)
};
// every check of the struct's fields, the row or text named; throws before any GPU work
AssistSpec assist_spec(const sbv2_assist* a, int64_t n);
std::vector<sbv2::AssistRow> assist_row_table(int64_t n, int A, const int32_t* text_of, const double* weight);
// ... assist (may be null): its sequences ride behind the batch's in the one DeBERTa forward and the gather blends their means in
void pipeline_run_one(sbv2::BertModel& bm, sbv2::VitsModel& vm, sbv2::VitsBatch v, const int64_t* token_ids, const int64_t* s_lens,
                      const int64_t* word2ph, const AssistSpec* assist = nullptr);
