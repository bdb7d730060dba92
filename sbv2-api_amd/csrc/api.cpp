// extern "C" boundary of libsbv2_hip.so (see include/sbv2_hip.h for what each entry point replaces).
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>


#include "api_internal.h"

VitsBatch to_batch(const sbv2_batch* b) {
    SBV2_REQUIRE(b && b->n >= 1 && b->t_lens && b->x_tst && b->tones && b->lang_ids && b->sids && b->style_vectors,
                 "sbv2_batch has null fields");
    VitsBatch v;
    v.n = (int)b->n;
    v.t_lens = b->t_lens;
    v.phones = b->x_tst;
    v.tones = b->tones;
    v.langs = b->lang_ids;
    v.sids = b->sids;
    v.styles = b->style_vectors;
    v.bert_host = b->bert;
    v.sdp_ratio = b->sdp_ratio;
    v.length_scale = b->length_scale;
    v.noise_scale = b->noise_scale;
    v.noise_scale_w = b->noise_scale_w;
    v.seed = b->noise_seed;
    v.forced_durations = b->forced_durations;
    return v;
}

// The per-row arrays of sbv2_utt_options onto the batch (host pointers, read by forward()); every check here, before any GPU work.
void apply_utt_options(VitsBatch* v, const sbv2_utt_options* o) {
    if (!o) return;
    const auto row = [](int u) { return " of row " + std::to_string(u); };
    for (int u = 0; u < v->n; ++u) {
        if (o->length_scale)
            SBV2_REQUIRE(std::isfinite(o->length_scale[u]) && o->length_scale[u] > 0.f,
                         "length_scale" + row(u) + " must be finite and > 0: " + std::to_string(o->length_scale[u]));
        if (o->sdp_ratio)
            SBV2_REQUIRE(o->sdp_ratio[u] >= 0.f && o->sdp_ratio[u] <= 1.f, "sdp_ratio" + row(u) + " must be in [0, 1]: " + std::to_string(o->sdp_ratio[u]));
        if (o->noise_scale)
            SBV2_REQUIRE(std::isfinite(o->noise_scale[u]) && o->noise_scale[u] >= 0.f,
                         "noise_scale" + row(u) + " must be finite and >= 0: " + std::to_string(o->noise_scale[u]));
        if (o->noise_scale_w)
            SBV2_REQUIRE(std::isfinite(o->noise_scale_w[u]) && o->noise_scale_w[u] >= 0.f,
                         "noise_scale_w" + row(u) + " must be finite and >= 0: " + std::to_string(o->noise_scale_w[u]));
        if (o->noise_index)
            SBV2_REQUIRE(o->noise_index[u] >= 0 && o->noise_index[u] < (1 << 30),
                         "noise_index" + row(u) + " must be in [0, 2^30): " + std::to_string(o->noise_index[u]));
    }
    v->row_sdp_ratio = o->sdp_ratio;
    v->row_length_scale = o->length_scale;
    v->row_noise_scale = o->noise_scale;
    v->row_noise_scale_w = o->noise_scale_w;
    v->row_seed = o->noise_seed;
    v->row_index = o->noise_index;
}

extern "C" {

const char* sbv2_last_error(void) { return last_error_cstr(); }

int sbv2_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int sbv2_bert_create(const uint8_t* model, size_t model_len, int device, sbv2_bert** out) {
    API_BEGIN
    SBV2_REQUIRE(out, "null output handle");
    Blob blob = load_model_bytes(model, model_len, 1);
    std::unique_ptr<sbv2_bert> h(new sbv2_bert);
    h->m.reset(new BertModel(blob, device));
    *out = h.release();
    API_END
}
void sbv2_bert_destroy(sbv2_bert* h) { delete h; }
int64_t sbv2_bert_hidden(const sbv2_bert* h) { return h ? h->m->cfg().hidden : 0; }
int sbv2_bert_gemm_parts(const sbv2_bert* h) { return h ? h->m->gemm_parts() : -1; }

int sbv2_bert_predict_batch(sbv2_bert* h, int64_t n, const int64_t* token_ids, const int64_t* attention_mask, const int64_t* lens,
                            float* out) {
    API_BEGIN
    SBV2_REQUIRE(h && token_ids && lens && out && n >= 1, "bad arguments");
    h->m->forward((int)n, token_ids, attention_mask, lens);
    h->m->copy_out(out);
    API_END
}
int sbv2_bert_predict(sbv2_bert* h, const int64_t* token_ids, const int64_t* attention_mask, int64_t S, float* out) {
    return sbv2_bert_predict_batch(h, 1, token_ids, attention_mask, &S, out);
}

int sbv2_vits_create(const uint8_t* model, size_t model_len, int device, sbv2_vits** out) {
    API_BEGIN
    SBV2_REQUIRE(out, "null output handle");
    Blob blob = load_model_bytes(model, model_len, 2);
    std::unique_ptr<sbv2_vits> h(new sbv2_vits);
    h->m.reset(new VitsModel(blob, device));
    *out = h.release();
    API_END
}
void sbv2_vits_destroy(sbv2_vits* h) { delete h; }
int64_t sbv2_vits_hop(const sbv2_vits* h) { return h ? h->m->cfg().hop() : 0; }
int64_t sbv2_vits_bert_dim(const sbv2_vits* h) { return h ? h->m->cfg().bert_dim : 0; }
int64_t sbv2_vits_style_dim(const sbv2_vits* h) { return h ? h->m->cfg().style_dim : 0; }
int sbv2_vits_decoder_mode(const sbv2_vits* h) { return h ? h->m->decoder_mode() : -1; }
int64_t sbv2_vits_workspace_bytes(const sbv2_vits* h) { return h ? (int64_t)h->m->workspace_bytes() : -1; }

int sbv2_vits_synthesize_batch_opts(sbv2_vits* h, const sbv2_batch* batch, const sbv2_utt_options* opts, int64_t* pcm_lens) {
    API_BEGIN
    VitsBatch v = to_batch(batch);
    apply_utt_options(&v, opts);
    SBV2_REQUIRE(h && pcm_lens, "bad arguments");
    SBV2_REQUIRE(v.bert_host, "sbv2_batch.bert is required here");
    h->m->forward(v);
    for (int i = 0; i < v.n; ++i) pcm_lens[i] = h->m->pcm_lens()[i];
    API_END
}
int sbv2_vits_synthesize_batch(sbv2_vits* h, const sbv2_batch* batch, int64_t* pcm_lens) {
    if (!h || !pcm_lens) {   // (checked before the batch, as ever)
        set_last_error("bad arguments");
        return 1;
    }
    return sbv2_vits_synthesize_batch_opts(h, batch, nullptr, pcm_lens);
}
int sbv2_vits_fetch_pcm(sbv2_vits* h, float* pcm, int64_t capacity) {
    API_BEGIN
    SBV2_REQUIRE(h && pcm, "bad arguments");
    SBV2_REQUIRE(capacity >= h->m->pcm_total(), "PCM buffer too small: " + std::to_string(capacity) + " < " + std::to_string(h->m->pcm_total()));
    h->m->copy_pcm(pcm);
    API_END
}
const float* sbv2_vits_pcm_device(sbv2_vits* h, int64_t* total) {
    if (!h) return nullptr;
    if (total) *total = h->m->pcm_total();
    return h->m->pcm_device();
}
int sbv2_vits_copy_pcm_device(sbv2_vits* h, void* dst_device, int64_t capacity) {
    API_BEGIN
    SBV2_REQUIRE(h && dst_device, "bad arguments");
    SBV2_REQUIRE(capacity >= h->m->pcm_total(), "PCM buffer too small");
    HIP_CHECK(hipSetDevice(h->m->device()));
    HIP_CHECK(hipMemcpyAsync(dst_device, h->m->pcm_device(), sizeof(float) * (size_t)h->m->pcm_total(), hipMemcpyDeviceToDevice,
                             h->m->stream()));
    HIP_CHECK(hipStreamSynchronize(h->m->stream()));
    API_END
}
int sbv2_sync(sbv2_vits* h) {
    API_BEGIN
    SBV2_REQUIRE(h, "bad arguments");
    HIP_CHECK(hipSetDevice(h->m->device()));
    HIP_CHECK(hipStreamSynchronize(h->m->stream()));
    API_END
}
int sbv2_prof_begin(void) {
    API_BEGIN
    conv_prof_begin();
    API_END
}
int sbv2_prof_end(char* json, int64_t cap) {
    API_BEGIN
    const std::string s = conv_prof_end();
    SBV2_REQUIRE(json && (int64_t)s.size() + 1 <= cap, "profile buffer too small");
    std::memcpy(json, s.c_str(), s.size() + 1);
    API_END
}
int sbv2_vits_fetch_durations(sbv2_vits* h, int64_t* durations, float* logw, int64_t capacity) {
    API_BEGIN
    SBV2_REQUIRE(h, "bad arguments");
    const auto& d = h->m->durations();
    const auto& l = h->m->logw();
    SBV2_REQUIRE(capacity >= (int64_t)d.size(), "duration buffer too small");
    if (durations)
        for (size_t i = 0; i < d.size(); ++i) durations[i] = d[i];
    if (logw) std::memcpy(logw, l.data(), sizeof(float) * l.size());
    API_END
}
int sbv2_vits_set_trace(sbv2_vits* h, int on) {
    API_BEGIN
    SBV2_REQUIRE(h, "bad arguments");
    h->m->set_trace(on != 0);
    API_END
}
int sbv2_vits_get_trace(sbv2_vits* h, const char* name, int64_t utt, float* out, int64_t cap, int64_t* rows, int64_t* cols) {
    API_BEGIN
    SBV2_REQUIRE(h && name && rows && cols, "bad arguments");
    std::vector<float> v;
    int r = 0, c = 0;
    SBV2_REQUIRE(h->m->get_trace(name, (int)utt, v, r, c), std::string("no trace named ") + name);
    *rows = r;
    *cols = c;
    if (out) {
        SBV2_REQUIRE((int64_t)v.size() <= cap, "trace buffer too small");
        std::memcpy(out, v.data(), sizeof(float) * v.size());
    }
    API_END
}

int sbv2_vits_synthesize(sbv2_vits* h, const float* bert, const int64_t* x_tst, const int64_t* tones, const int64_t* lang_ids, int64_t T,
                         int64_t sid, const float* style_vector, float sdp_ratio, float length_scale, float noise_scale,
                         float noise_scale_w, uint64_t noise_seed, float** pcm, int64_t* pcm_len) {
    API_BEGIN
    SBV2_REQUIRE(h && bert && pcm && pcm_len, "bad arguments");
    sbv2_batch b;
    std::memset(&b, 0, sizeof(b));
    b.n = 1;
    b.t_lens = &T;
    b.x_tst = x_tst;
    b.tones = tones;
    b.lang_ids = lang_ids;
    b.sids = &sid;
    b.style_vectors = style_vector;
    b.bert = bert;
    b.sdp_ratio = sdp_ratio;
    b.length_scale = length_scale;
    b.noise_scale = noise_scale;
    b.noise_scale_w = noise_scale_w;
    b.noise_seed = noise_seed;
    h->m->forward(to_batch(&b));
    const int64_t n = h->m->pcm_total();
    float* buf = static_cast<float*>(std::malloc(sizeof(float) * (size_t)std::max<int64_t>(n, 1)));
    SBV2_REQUIRE(buf, "out of host memory");
    try {
        h->m->copy_pcm(buf);
    } catch (...) {
        std::free(buf);
        throw;
    }
    *pcm = buf;
    *pcm_len = n;
    API_END
}
void sbv2_pcm_free(float* pcm) { std::free(pcm); }

int sbv2_pipeline_create(sbv2_bert* bert, sbv2_vits* vits, sbv2_pipeline** out) {
    API_BEGIN
    SBV2_REQUIRE(bert && vits && out, "bad arguments");
    SBV2_REQUIRE(bert->m->device() == vits->m->device(), "bert and vits handles live on different devices");
    SBV2_REQUIRE(bert->m->cfg().hidden == vits->m->cfg().bert_dim, "DeBERTa hidden size does not match the VITS bert_proj input");
    std::unique_ptr<sbv2_pipeline> p(new sbv2_pipeline);
    p->bert = bert;
    p->vits = vits;
    // execution contexts = pipeline depth across calls (SBV2_PIPELINE_DEPTH, default 2).  (Cutting ONE batch into micro-batches was
    // measured too: the latency-bound chains then repeat per micro-batch and the step gets slower, 220 vs 186 ms with 4 cuts.)
    int k = 2;
    if (const char* e = getenv("SBV2_PIPELINE_DEPTH")) k = std::max(1, std::min(8, atoi(e)));
    for (int i = 1; i < k; ++i) {
        p->bclones.emplace_back(bert->m->clone());
        p->vclones.emplace_back(vits->m->clone());
    }
    p->chains = std::vector<OutputChain>(k);
    *out = p.release();
    API_END
}
void sbv2_pipeline_destroy(sbv2_pipeline* p) { delete p; }

}  // extern "C"

// One micro-batch on one context: bert::predict -> word2ph repeat (tts_util.rs:129-154) -> model::synthesize
void pipeline_run_one(BertModel& bm, VitsModel& vm, VitsBatch v, const int64_t* token_ids, const int64_t* s_lens,
                      const int64_t* word2ph) {
    HIP_CHECK(hipStreamSynchronize(vm.stream()));  // this context's previous batch may still be reading the DeBERTa output plane
    bm.forward(v.n, token_ids, nullptr, s_lens);
    const SegLayout& bl = bm.layout();
    std::vector<int> map;
    int64_t e = 0;
    for (int u = 0; u < v.n; ++u) {
        SBV2_REQUIRE(s_lens[u] == bl.len[u], "internal: layout mismatch");
        int64_t cnt = 0;
        for (int64_t i = 0; i < s_lens[u]; ++i, ++e) {
            SBV2_REQUIRE(word2ph[e] >= 0, "negative word2ph");
            for (int64_t r = 0; r < word2ph[e]; ++r) map.push_back(bl.start[u] + (int)i);
            cnt += word2ph[e];
        }
        SBV2_REQUIRE(cnt == v.t_lens[u], "sum(word2ph) must equal the text length (tts_util.rs:122-127)");
    }
    v.bert_host = nullptr;
    v.bert_dev = &bm.out();
    v.bert_map = map.data();
    // the two models run on their own streams: an event dependency inside forward(), not a host wait
    v.after_stream = bm.stream();
    vm.forward(v);
}

extern "C" {

// Batches are PIPELINED ACROSS CALLS: call n runs on execution context n % depth (own HIP stream + workspace, shared weights), so the
// latency-bound part of batch n+1 (DeBERTa, text encoder, duration predictors, flow: ~1300 small launches, ~55 ms whatever the
// batch size) executes beside the throughput-bound HiFi-GAN kernels of batch n.  A call returns once its kernels are enqueued (the
// host only waits for the batch's own integer durations); results are collected with sbv2_pipeline_wait / _fetch_pcm by ticket.
int sbv2_pipeline_run_opts(sbv2_pipeline* p, const sbv2_batch* batch, const sbv2_utt_options* opts, const int64_t* token_ids, const int64_t* s_lens,
                           const int64_t* word2ph, int64_t* pcm_lens) {
    API_BEGIN
    VitsBatch v = to_batch(batch);
    apply_utt_options(&v, opts);
    SBV2_REQUIRE(p && token_ids && s_lens && word2ph && pcm_lens, "bad arguments");
    const int ctx = (int)(p->calls % p->contexts());
    ++p->calls;
    pipeline_run_one(p->bm(ctx), p->vm(ctx), v, token_ids, s_lens, word2ph);
    for (int i = 0; i < v.n; ++i) pcm_lens[i] = p->vm(ctx).pcm_lens()[i];
    API_END
}
int sbv2_pipeline_run(sbv2_pipeline* p, const sbv2_batch* batch, const int64_t* token_ids, const int64_t* s_lens, const int64_t* word2ph,
                      int64_t* pcm_lens) {
    if (!p || !token_ids || !s_lens || !word2ph || !pcm_lens) {   // (checked before the batch, as ever)
        set_last_error("bad arguments");
        return 1;
    }
    return sbv2_pipeline_run_opts(p, batch, nullptr, token_ids, s_lens, word2ph, pcm_lens);
}

int64_t sbv2_pipeline_last_ticket(sbv2_pipeline* p) { return p ? p->calls : -1; }

int sbv2_pipeline_wait(sbv2_pipeline* p, int64_t ticket) {
    API_BEGIN
    SBV2_REQUIRE(p, "bad arguments");
    const int ctx = p->ctx_of(ticket);
    HIP_CHECK(hipSetDevice(p->vits->m->device()));
    HIP_CHECK(hipStreamSynchronize(p->vm(ctx).stream()));
    API_END
}

int sbv2_pipeline_sync(sbv2_pipeline* p) {
    API_BEGIN
    SBV2_REQUIRE(p, "bad arguments");
    HIP_CHECK(hipSetDevice(p->vits->m->device()));
    for (int j = 0; j < p->contexts(); ++j) HIP_CHECK(hipStreamSynchronize(p->vm(j).stream()));
    API_END
}

// Concatenated PCM of the run with this ticket (utterance order); dst_is_device != 0: dst is device memory (the RCCL send buffer).
// capacity = samples dst can hold: a run whose PCM is longer is refused instead of overflowing the buffer.
int sbv2_pipeline_fetch_pcm_ticket(sbv2_pipeline* p, int64_t ticket, float* dst, int64_t capacity, int dst_is_device) {
    API_BEGIN
    SBV2_REQUIRE(p && dst, "bad arguments");
    VitsModel& vm = p->vm(p->ctx_of(ticket));
    SBV2_REQUIRE(capacity >= vm.pcm_total(), "PCM buffer too small: " + std::to_string(capacity) + " < " + std::to_string(vm.pcm_total()));
    HIP_CHECK(hipSetDevice(vm.device()));
    HIP_CHECK(hipMemcpyAsync(dst, vm.pcm_device(), sizeof(float) * (size_t)vm.pcm_total(),
                             dst_is_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, vm.stream()));
    HIP_CHECK(hipStreamSynchronize(vm.stream()));
    API_END
}
int sbv2_pipeline_fetch_pcm(sbv2_pipeline* p, float* dst, int64_t capacity, int dst_is_device) {
    return sbv2_pipeline_fetch_pcm_ticket(p, p ? p->calls : -1, dst, capacity, dst_is_device);
}

// ---- output formats (pcm_format.hip) ----
int64_t sbv2_pcm_format_length(const sbv2_pcm_format* fmt, int64_t n_native) {
    try {
        const PcmFmtSpec spec = pcm_format_spec(fmt);
        SBV2_REQUIRE(n_native >= 0, "negative sample count");
        return pcm_format_out_len(spec, n_native);
    } catch (const std::exception& e) {
        set_last_error(e.what());
        return -1;
    }
}

// Host only: the two G.711 laws on s16 integers, the very lines the device quantisers and the level reduction run (pcm_format.h)
int sbv2_g711_encode(int32_t encoding, const int16_t* q, int64_t n, uint8_t* codes) {
    API_BEGIN
    SBV2_REQUIRE(pcm_encoding_g711(encoding), "unsupported G.711 encoding " + std::to_string(encoding) + " (7 = mu-law, 6 = A-law)");
    SBV2_REQUIRE(n >= 0 && (n == 0 || (q && codes)), "bad arguments");
    for (int64_t i = 0; i < n; ++i) {
        const int v = std::max<int>(q[i], -32767);   // (the quantiser never delivers -32768)
        codes[i] = encoding == kEncMulaw ? mulaw_encode(v) : alaw_encode(v);
    }
    API_END
}
int sbv2_g711_decode(int32_t encoding, const uint8_t* codes, int64_t n, int16_t* q) {
    API_BEGIN
    SBV2_REQUIRE(pcm_encoding_g711(encoding), "unsupported G.711 encoding " + std::to_string(encoding) + " (7 = mu-law, 6 = A-law)");
    SBV2_REQUIRE(n >= 0 && (n == 0 || (q && codes)), "bad arguments");
    for (int64_t i = 0; i < n; ++i) q[i] = (int16_t)(encoding == kEncMulaw ? mulaw_decode(codes[i]) : alaw_decode(codes[i]));
    API_END
}

int sbv2_pcm_format_taps(int32_t sample_rate, float* h, int64_t cap, int64_t* len, int32_t* L, int32_t* M) {
    API_BEGIN
    SBV2_REQUIRE(len, "bad arguments");
    int l, m, half;
    const std::vector<double> proto = pcm_format_prototype(sample_rate, &l, &m, &half);
    SBV2_REQUIRE(!h || cap >= (int64_t)proto.size(), "tap buffer too small: " + std::to_string(cap) + " < " + std::to_string(proto.size()));
    *len = (int64_t)proto.size();
    if (L) *L = l;
    if (M) *M = m;
    if (h)
        for (size_t i = 0; i < proto.size(); ++i) h[i] = (float)proto[i];
    API_END
}

// The signals of a formatted fetch: one per utterance (place == NULL), or the run's utterances on one joined timeline.  outs = output samples
// of each signal; the result is `total` samples.
// utts != NULL: the joined timeline holds those n_utts rows only, place[k] belonging to row utts[k] (sbv2_pipeline_fetch_request).
static void format_layout(const PcmFmtSpec& spec, VitsModel& vm, const int32_t* utts, int n_utts, const int64_t* place, int64_t joined_len,
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

}  // extern "C"

// ---- the formatted fetches: output formats (pcm_format.hip), FLAC (flac_encode.hip), loudness (loudness.hip), limiter (limiter.hip) ----
// A formatted fetch = a gain stage and a sink.  The gain stage: none (peak-normalise or not, as fmt->normalize says), a loudness gain
// (ln; NULL = measure only) or the look-ahead limiter (lim).  The sink: PCM bytes in fmt's encoding, or one FLAC stream per signal.
struct FetchGain {
    enum Kind { kNone, kLoudness, kLimiter } kind = kNone;
    const sbv2_loudness* ln = nullptr;
    const sbv2_limiter* lim = nullptr;
    const sbv2_dynamics* dyn = nullptr;   // the compressor in front of either stage (NULL or ratio == 1: none)
    int stats_per_signal() const { return kind == kLimiter ? 6 : kind == kLoudness ? 3 : 0; }
};
enum class Sink { kPcm, kFlac };

static PcmFmtSpec fetch_spec(const sbv2_pcm_format* fmt, bool gain_stage, Sink sink) {
    const PcmFmtSpec spec = pcm_format_spec(fmt);
    if (gain_stage) SBV2_REQUIRE(!spec.normalize, "loudness normalisation replaces peak normalisation: fmt->normalize must be 0");
    if (sink == Sink::kFlac) SBV2_REQUIRE(spec.encoding == kEncS16, "FLAC needs encoding = 1 (s16): f32 samples and G.711 codes have no FLAC form");
    return spec;
}

// The speech marks of a request fetch (marks.h), planned on the host before anything is enqueued: the listed rows' token spans on the delivered
// timeline and the segment table of the level reduction (the token spans when levels are asked for, then the envelope frames).
struct MarksPlan {
    std::vector<int64_t> start, end;   // per token, in the order of the request's rows
    std::vector<int64_t> seg;          // [levels ? n_tok : 0][2], then [n_env][2]
    int64_t n_tok = 0, n_env = 0;
    bool levels = false;
};
// the checks of sbv2_marks that need no run
static void check_marks_static(const sbv2_marks* m) {
    SBV2_REQUIRE(m->reserved == 0, "sbv2_marks.reserved must be 0");
    SBV2_REQUIRE(m->env_hop >= 0, "sbv2_marks.env_hop must be >= 0: " + std::to_string(m->env_hop));
    SBV2_REQUIRE(m->env_hop == 0 || (m->env_sumsq && m->env_peak), "sbv2_marks.env_hop > 0 needs env_sumsq and env_peak");
    SBV2_REQUIRE(!m->tok_sumsq == !m->tok_peak, "sbv2_marks.tok_sumsq and tok_peak are given together or not at all");
    SBV2_REQUIRE(m->tok_capacity >= 0 && m->env_capacity >= 0, "negative sbv2_marks capacity");
}
static MarksPlan plan_marks(const sbv2_marks* m, const PcmFmtSpec& spec, const VitsModel& vm, const int32_t* utts, int n_utts, const int64_t* place,
                            int64_t total) {
    check_marks_static(m);
    SBV2_REQUIRE(utts && place, "internal: marks need a request's rows");
    const std::vector<int64_t>& offs = vm.used_offs();
    const std::vector<int64_t>& used = vm.used_durations();
    SBV2_REQUIRE(offs.size() == vm.pcm_lens().size() + 1, "internal: the run kept no durations");
    MarksPlan mp;
    for (int k = 0; k < n_utts; ++k) mp.n_tok += offs[utts[k] + 1] - offs[utts[k]];
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
    marks_spans_rows(used, offs, utts, n_utts, place, vm.cfg().hop(), spec, mp.start.data(), mp.end.data());
    mp.seg.reserve((size_t)(2 * ((mp.levels ? mp.n_tok : 0) + mp.n_env)));
    if (mp.levels)
        for (int64_t t = 0; t < mp.n_tok; ++t) mp.seg.push_back(mp.start[t]), mp.seg.push_back(mp.end[t]);
    for (int64_t f = 0; f < mp.n_env; ++f) mp.seg.push_back(f * m->env_hop), mp.seg.push_back(std::min((f + 1) * (int64_t)m->env_hop, total));
    return mp;
}

// The checks of sbv2_pitch that need no run: the parameters at the delivered rate (marks.h states the bounds), the arrays.
static PitchSpec check_pitch_static(const sbv2_pitch* q, int rate) {
    SBV2_REQUIRE(q->reserved == 0, "sbv2_pitch.reserved must be 0");
    const PitchSpec sp = pitch_spec(rate, q->hop, q->f0_min, q->f0_max, q->threshold);
    SBV2_REQUIRE(q->capacity >= 0, "negative sbv2_pitch capacity");
    SBV2_REQUIRE(q->f0, "sbv2_pitch.f0 must not be NULL");
    return sp;
}

// The checks of sbv2_voice that need no run: the parameters at the rate of the rows (voice.h states the bounds).
static VoiceSpec check_voice_static(const sbv2_voice* v, int rate) {
    SBV2_REQUIRE(v->reserved == 0, "sbv2_voice.reserved must be 0");
    return voice_spec(rate, v->pitch_scale, v->intonation_scale, v->hop, v->f0_min, v->f0_max, v->threshold);
}

// The checks of sbv2_token_pitch that need no run (voice.h states the bounds; vs: the voice's checked parameters, the defaults without a voice)
// -> whether any token is edited.
static VoiceSpec default_voice_spec() { return voice_spec(kNativeRate, 1.0, 1.0, 0, 0.0, 0.0, 0.0); }
static bool check_token_pitch_static(const sbv2_token_pitch* t, const VoiceSpec& vs) {
    SBV2_REQUIRE(t->reserved == 0, "sbv2_token_pitch.reserved must be 0");
    SBV2_REQUIRE(t->n_tokens >= 0, "sbv2_token_pitch.n_tokens must be >= 0: " + std::to_string(t->n_tokens));
    SBV2_REQUIRE(t->value || t->n_tokens == 0, "sbv2_token_pitch.value must not be NULL");
    voice_tokens_check(t->value, t->n_tokens, t->kind, t->smooth, vs);
    for (int64_t i = 0; i < t->n_tokens; ++i)
        if (t->value[i] != 0.0) return true;
    return false;
}

// The checks of sbv2_formant that need no run (formant_spec of voice.h holds them; vs as above) -> the scale and the gather's widened range.
static FormantSpec check_formant_static(const sbv2_formant* f, const VoiceSpec& vs) { return formant_spec(f->formant_scale, f->reserved, vs); }

// The checks of sbv2_pitch_track (track.h states the bounds).
static TrackSpec check_track_static(const sbv2_pitch_track* t) {
    SBV2_REQUIRE(t->reserved[0] == 0 && t->reserved[1] == 0, "sbv2_pitch_track.reserved must be 0");
    return track_spec(t->cand_max, t->unvoiced_cost, t->switch_cost, t->jump_cost);
}

// The run's packed PCM (pcm_device + pcm_offs / pcm_lens) is formatted on the run's own stream and crosses PCIe in the format: every
// check first (format, gain options, ticket, placement, PCM capacity), then the formatter's launches with the gain stage between the
// resampler and the quantiser, then the sink.  out_counts: samples (PCM) or bytes (FLAC) of each signal; stats (may be NULL): the gain
// stage's 3 or 6 doubles per signal.
// utts (with place): the one signal of those rows only.
// marks (with utts): the speech marks of that signal; their reduction reads the delivered samples in HBM, on the same stream, before the one
// synchronisation of the fetch, and the caller's arrays are written only once everything else has succeeded.
// pitch (with utts): the pitch contour of the same delivered samples (Pitch, marks.h), enqueued and written under the same two rules.
// voice (with utts; NULL or the identity: nothing): the listed rows are shifted first (Voice, voice.h) into the chain's scratch buffer, laid out
// like the run's packed PCM, and the pieces point there; the run's PCM is only read.
// track (with pitch, or with a voice that shifts): both contours are tracked (Track, track.h) before they are used.
// gain.dyn (with a loudness or limiter stage): the compressor runs on y first (Dynamics, dynamics.h); dyn_stats (may be NULL): its 3 doubles.
// tp (with utts; NULL or all zeros: nothing): the listed rows' tokens are edited in the shifter (its token phase, voice.h), which then runs
// whatever the voice is; applied / src_f0 reach the caller's arrays only once everything else has succeeded.
// fmnt (with utts; NULL or scale 1: nothing): the shifter runs whatever the voice is, its gather reading every grain at the scaled offset.
static void fetch_formatted(sbv2_pipeline* p, int64_t ticket, const sbv2_pcm_format* fmt, const FetchGain& gain, const int64_t* place,
                            int64_t joined_len, Sink sink, void* dst, int64_t capacity_bytes, int64_t* out_counts, double* stats,
                            const int32_t* utts = nullptr, int n_utts = 0, sbv2_marks* marks = nullptr, sbv2_pitch* pitch = nullptr,
                            const sbv2_voice* voice = nullptr, const sbv2_pitch_track* track = nullptr, double* dyn_stats = nullptr,
                            const sbv2_token_pitch* tp = nullptr, const sbv2_formant* fmnt = nullptr) {
    const DynamicsSpec dyn = gain.dyn ? dynamics_spec(gain.dyn) : DynamicsSpec();
    const bool compress = gain.dyn && !dyn.identity();
    const PcmFmtSpec spec = fetch_spec(fmt, gain.kind != FetchGain::kNone, sink);
    const LoudnessSpec ln = gain.kind == FetchGain::kLoudness ? loudness_spec(gain.ln) : LoudnessSpec();
    const LimiterSpec lim = gain.kind == FetchGain::kLimiter ? limiter_spec(gain.lim) : LimiterSpec();
    const int ctx = p->ctx_of(ticket);
    VitsModel& vm = p->vm(ctx);
    std::vector<FmtPiece> pieces;
    std::vector<FmtSignal> sig;
    std::vector<int64_t> outs, flac_bytes;   // per signal: samples, bytes of its FLAC stream
    int64_t total = 0;
    format_layout(spec, vm, utts, n_utts, place, joined_len, &pieces, &sig, &outs, &total);
    const int64_t pcm_bytes = total * spec.bytes();
    if (sink == Sink::kPcm)   // (the FLAC sink checks its capacity after encoding, when the sizes are known)
        SBV2_REQUIRE(capacity_bytes >= pcm_bytes,
                     "PCM buffer too small: " + std::to_string(capacity_bytes) + " < " + std::to_string(pcm_bytes) + " bytes");
    const MarksPlan mp = marks ? plan_marks(marks, spec, vm, utts, n_utts, place, total) : MarksPlan();
    const int64_t nseg = (int64_t)mp.seg.size() / 2;
    bool marks_ran = false;
    PitchSpec ps;
    int64_t n_pitch = 0;
    if (pitch) {
        SBV2_REQUIRE(utts && place, "internal: pitch needs a request's rows");
        ps = check_pitch_static(pitch, spec.rate);
        n_pitch = pitch_frames(total, ps.hop);
        SBV2_REQUIRE(pitch->capacity >= n_pitch,
                     "pitch arrays too small: " + std::to_string(pitch->capacity) + " < " + std::to_string(n_pitch) + " frames");
    }
    VoiceSpec vs;
    if (voice) {
        SBV2_REQUIRE(utts && place, "internal: voice needs a request's rows");
        vs = check_voice_static(voice, kNativeRate);
    } else if (tp || fmnt) {
        vs = default_voice_spec();
    }
    FormantSpec fs;
    if (fmnt) {
        SBV2_REQUIRE(utts && place, "internal: formant needs a request's rows");
        fs = check_formant_static(fmnt, vs);
    }
    const bool scale = fmnt && !fs.identity();
    bool edit = false;
    std::vector<int64_t> tok_counts, tok_ends;
    if (tp) {
        SBV2_REQUIRE(utts && place, "internal: token pitch needs a request's rows");
        edit = check_token_pitch_static(tp, vs);
        const std::vector<int64_t>& offs = vm.used_offs();
        const std::vector<int64_t>& used = vm.used_durations();
        SBV2_REQUIRE(offs.size() == vm.pcm_lens().size() + 1, "internal: the run kept no durations");
        int64_t n_tok = 0;
        for (int k = 0; k < n_utts; ++k) n_tok += offs[utts[k] + 1] - offs[utts[k]];
        SBV2_REQUIRE(tp->n_tokens == n_tok, "sbv2_token_pitch.n_tokens is " + std::to_string(tp->n_tokens) + " but the listed rows have " +
                                                std::to_string(n_tok) + " tokens");
        if (edit) {   // token t of a row ends at hop c[t + 1]
            tok_ends.reserve((size_t)n_tok);
            for (int k = 0; k < n_utts; ++k) {
                tok_counts.push_back(offs[utts[k] + 1] - offs[utts[k]]);
                int64_t c = 0;
                for (int64_t e = offs[utts[k]]; e < offs[utts[k] + 1]; ++e) tok_ends.push_back((c += used[(size_t)e]) * vm.cfg().hop());
            }
        }
    }
    const bool shift = ((voice && !vs.identity()) || edit || scale) && n_utts > 0;
    TrackSpec ts;
    if (track) {
        ts = check_track_static(track);
        SBV2_REQUIRE(pitch || (voice && !vs.identity()) || edit || scale,
                     "pitch tracking needs a pitch contour or a voice that is not the identity");
    }
    HIP_CHECK(hipSetDevice(vm.device()));
    OutputChain& c = p->chains[ctx];
    const hipStream_t s = vm.stream();
    if (shift) {   // the listed rows, shifted, where the formatter will read them
        std::vector<VoiceRow> rows((size_t)n_utts);
        for (int k = 0; k < n_utts; ++k) rows[k] = VoiceRow{vm.pcm_offs()[utts[k]], vm.pcm_lens()[utts[k]]};
        const float* pcm = vm.pcm_device();
        const VoiceTokens vt{tok_counts.data(), tok_ends.data(), edit ? tp->value : nullptr, edit ? tp->kind : 0, edit ? tp->smooth : 0};
        const float* shifted = c.voice.run(pcm, vm.pcm_total(), rows.data(), n_utts, vs, s, nullptr, nullptr, track ? &ts : nullptr, edit ? &vt : nullptr,
                                           scale ? &fs : nullptr);
        for (FmtPiece& pc : pieces) pc.src = shifted + (pc.src - pcm);
    }
    if (sink == Sink::kPcm && gain.kind == FetchGain::kNone && spec.identity() && !place) {   // the bytes of sbv2_pipeline_fetch_pcm_ticket
        HIP_CHECK(hipMemcpyAsync(dst, vm.pcm_device(), sizeof(float) * (size_t)vm.pcm_total(), hipMemcpyDeviceToHost, s));
    } else if (total > 0 || gain.kind != FetchGain::kNone || sink == Sink::kFlac) {   // a gain stage and the encoder run on empty signals too
        void* dev = c.formatter.out_buffer((size_t)std::max<int64_t>(pcm_bytes, spec.bytes()), s);
        Dynamics* const dy = compress ? &c.dynamics : nullptr;
        const GainStage stage = gain.kind == FetchGain::kLimiter    ? GainStage(c.meter, c.limiter, lim, dy, &dyn)
                                : gain.kind == FetchGain::kLoudness ? GainStage(c.meter, ln, dy, &dyn)
                                                                    : GainStage();
        c.formatter.run(spec, pieces, sig, total, dev, 0, s, stage);
        if (nseg > 0 && total > 0) {   // the delivered samples, as they cross PCIe or enter the encoder
            c.marks.run(dev, spec.encoding, total, mp.seg.data(), nseg, s);
            marks_ran = true;
        }
        if (n_pitch > 0) c.pitch.run(dev, spec.encoding, total, ps, s, track ? &ts : nullptr, track ? &c.track : nullptr);
        if (sink == Sink::kFlac) {   // the signals stay in HBM; the encoder reads the stream sizes back, then exactly the encoded bytes cross PCIe
            std::vector<int64_t> offs(outs.size());
            for (size_t i = 1; i < outs.size(); ++i) offs[i] = offs[i - 1] + outs[i - 1];
            const int64_t nbytes = c.flac.encode(static_cast<const int16_t*>(dev), offs, outs, spec.rate, s, &flac_bytes);
            SBV2_REQUIRE(capacity_bytes >= nbytes,
                         "FLAC buffer too small: " + std::to_string(capacity_bytes) + " < " + std::to_string(nbytes) + " bytes");
            HIP_CHECK(hipMemcpyAsync(dst, c.flac.output(), (size_t)nbytes, hipMemcpyDeviceToHost, s));
        } else if (total > 0) {
            HIP_CHECK(hipMemcpyAsync(dst, dev, (size_t)pcm_bytes, hipMemcpyDeviceToHost, s));
        }
    }
    HIP_CHECK(hipStreamSynchronize(s));
    if (shift)
        for (int k = 0; k < n_utts; ++k) SBV2_REQUIRE(c.voice.status(k) == 0, "internal: the shifter found more marks than it planned for");
    for (size_t i = 0; i < outs.size(); ++i) out_counts[i] = sink == Sink::kFlac ? flac_bytes[i] : outs[i];
    if (stats) {   // written by the stage's last copy on s
        const double* from = gain.kind == FetchGain::kLimiter ? c.limiter.stats_host() : c.meter.stats_host();
        std::memcpy(stats, from, sizeof(double) * gain.stats_per_signal() * sig.size());
    }
    if (dyn_stats && compress) std::memcpy(dyn_stats, c.dynamics.stats_host(), sizeof(double) * 3 * sig.size());
    if (marks) {
        std::copy(mp.start.begin(), mp.start.end(), marks->tok_start);
        std::copy(mp.end.begin(), mp.end.end(), marks->tok_end);
        // (an empty signal has only empty segments: 0, without a launch)
        const int64_t nt = mp.levels ? mp.n_tok : 0;
        for (int64_t t = 0; t < nt; ++t) {
            marks->tok_sumsq[t] = marks_ran ? c.marks.sumsq_host()[t] : 0.0;
            marks->tok_peak[t] = marks_ran ? c.marks.peak_host()[t] : 0.0;
        }
        for (int64_t f = 0; f < mp.n_env; ++f) {
            marks->env_sumsq[f] = marks_ran ? c.marks.sumsq_host()[nt + f] : 0.0;
            marks->env_peak[f] = marks_ran ? c.marks.peak_host()[nt + f] : 0.0;
        }
        marks->n_tokens = mp.n_tok;
        marks->n_env = mp.n_env;
    }
    if (tp) {   // (all zeros: nothing was measured)
        for (int64_t t = 0; t < tp->n_tokens; ++t) {
            if (tp->applied) tp->applied[t] = edit && shift ? c.voice.applied_host()[t] : 1.0;
            if (tp->src_f0) tp->src_f0[t] = edit && shift ? c.voice.src_f0_host()[t] : 0.0;
        }
    }
    if (pitch) {   // (an empty signal has no frames and ran nothing)
        for (int64_t f = 0; f < n_pitch; ++f) {
            const int32_t lag = c.pitch.lag_host()[f];
            pitch_finish(ps, lag, c.pitch.voiced_host()[f], c.pitch.c3_host() + 3 * f, pitch->f0 + f, pitch->ap ? pitch->ap + f : nullptr);
            if (pitch->lag) pitch->lag[f] = lag;
        }
        pitch->n_frames = n_pitch;
    }
}

extern "C" {

int sbv2_pipeline_fetch_pcm_format(sbv2_pipeline* p, int64_t ticket, const sbv2_pcm_format* fmt, const int64_t* place, int64_t joined_len,
                                   void* dst, int64_t capacity_bytes, int64_t* out_lens) {
    API_BEGIN
    SBV2_REQUIRE(p && dst && out_lens, "bad arguments");
    fetch_formatted(p, ticket, fmt, FetchGain(), place, joined_len, Sink::kPcm, dst, capacity_bytes, out_lens, nullptr);
    API_END
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
    API_BEGIN
    SBV2_REQUIRE(p && dst && out_bytes, "bad arguments");
    fetch_formatted(p, ticket, fmt, FetchGain(), place, joined_len, Sink::kFlac, dst, capacity_bytes, out_bytes, nullptr);
    API_END
}

int sbv2_loudness_kweight(int32_t sample_rate, double* coef) {
    API_BEGIN
    SBV2_REQUIRE(coef, "bad arguments");
    loudness_kweight(sample_rate, coef);
    API_END
}

int sbv2_pipeline_fetch_pcm_loudness(sbv2_pipeline* p, int64_t ticket, const sbv2_pcm_format* fmt, const sbv2_loudness* ln, const int64_t* place,
                                     int64_t joined_len, void* dst, int64_t capacity_bytes, int64_t* out_lens, double* stats) {
    API_BEGIN
    SBV2_REQUIRE(p && dst && out_lens, "bad arguments");
    fetch_formatted(p, ticket, fmt, FetchGain{FetchGain::kLoudness, ln, nullptr}, place, joined_len, Sink::kPcm, dst, capacity_bytes, out_lens, stats);
    API_END
}

int sbv2_pipeline_fetch_flac_loudness(sbv2_pipeline* p, int64_t ticket, const sbv2_pcm_format* fmt, const sbv2_loudness* ln, const int64_t* place,
                                      int64_t joined_len, uint8_t* dst, int64_t capacity_bytes, int64_t* out_bytes, double* stats) {
    API_BEGIN
    SBV2_REQUIRE(p && dst && out_bytes, "bad arguments");
    fetch_formatted(p, ticket, fmt, FetchGain{FetchGain::kLoudness, ln, nullptr}, place, joined_len, Sink::kFlac, dst, capacity_bytes, out_bytes, stats);
    API_END
}

int sbv2_pipeline_fetch_pcm_limited(sbv2_pipeline* p, int64_t ticket, const sbv2_pcm_format* fmt, const sbv2_limiter* lim, const int64_t* place,
                                    int64_t joined_len, void* dst, int64_t capacity_bytes, int64_t* out_lens, double* stats) {
    API_BEGIN
    SBV2_REQUIRE(p && dst && out_lens, "bad arguments");
    fetch_formatted(p, ticket, fmt, FetchGain{FetchGain::kLimiter, nullptr, lim}, place, joined_len, Sink::kPcm, dst, capacity_bytes, out_lens, stats);
    API_END
}

int sbv2_pipeline_fetch_flac_limited(sbv2_pipeline* p, int64_t ticket, const sbv2_pcm_format* fmt, const sbv2_limiter* lim, const int64_t* place,
                                     int64_t joined_len, uint8_t* dst, int64_t capacity_bytes, int64_t* out_bytes, double* stats) {
    API_BEGIN
    SBV2_REQUIRE(p && dst && out_bytes, "bad arguments");
    fetch_formatted(p, ticket, fmt, FetchGain{FetchGain::kLimiter, nullptr, lim}, place, joined_len, Sink::kFlac, dst, capacity_bytes, out_bytes, stats);
    API_END
}

int32_t sbv2_voice_tile(void) { return Voice::kTile; }

int32_t sbv2_dynamics_tile(void) { return Dynamics::kTile; }

int sbv2_pipeline_fetch_request_formant(sbv2_pipeline* p, int64_t ticket, const sbv2_fetch_request* req, const sbv2_voice* voice,
                                        const sbv2_pitch_track* track, const sbv2_dynamics* dynamics, const sbv2_token_pitch* token_pitch,
                                        const sbv2_formant* formant, void* dst, int64_t capacity_bytes, int64_t* out_count, double* stats,
                                        double* dyn_stats, sbv2_marks* marks, sbv2_pitch* pitch) {
    API_BEGIN
    DynamicsSpec ds;
    if (dynamics) ds = dynamics_spec(dynamics);   // what needs no run is refused before the handle is looked at
    VoiceSpec vs;
    if (voice) vs = check_voice_static(voice, kNativeRate);   // what needs no run is refused before the handle is looked at
    const bool edit = token_pitch && check_token_pitch_static(token_pitch, voice ? vs : default_voice_spec());
    const bool scale = formant && !check_formant_static(formant, voice ? vs : default_voice_spec()).identity();
    if (track) {
        (void)check_track_static(track);
        SBV2_REQUIRE(pitch || (voice && !vs.identity()) || edit || scale, "pitch tracking needs a pitch contour or a voice that is not the identity");
    }
    SBV2_REQUIRE(req && req->n_utts >= 0 && (req->n_utts == 0 || (req->utts && req->place)), "bad fetch request");
    SBV2_REQUIRE(!(req->loudness && req->limiter), "a fetch request takes a loudness target or a limiter, not both");
    if (dynamics && !ds.identity())   // (fmt->normalize is then refused with the gain stage it needs)
        SBV2_REQUIRE(req->loudness || req->limiter,
                     "a compressor needs a loudness target or a limiter behind it: without make-up it only makes the signal quieter");
    if (marks) {   // what needs no run is refused before the handle is looked at
        check_marks_static(marks);
        (void)pcm_format_spec(req->fmt);
    }
    if (pitch) (void)check_pitch_static(pitch, pcm_format_spec(req->fmt).rate);
    SBV2_REQUIRE(p && dst && out_count, "bad arguments");
    const FetchGain gain = req->limiter    ? FetchGain{FetchGain::kLimiter, nullptr, req->limiter, dynamics}
                           : req->loudness ? FetchGain{FetchGain::kLoudness, req->loudness, nullptr, dynamics}
                                           : FetchGain{FetchGain::kNone, nullptr, nullptr, dynamics};
    static const int32_t no_rows[1] = {0};
    static const int64_t no_place[1] = {0};
    fetch_formatted(p, ticket, req->fmt, gain, req->n_utts ? req->place : no_place, req->joined_len, req->flac ? Sink::kFlac : Sink::kPcm, dst,
                    capacity_bytes, out_count, stats, req->n_utts ? req->utts : no_rows, req->n_utts, marks, pitch, voice, track, dyn_stats,
                    token_pitch, formant);
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

int sbv2_pitch_lags(int32_t sample_rate, double f0_min, double f0_max, int32_t* tau_min, int32_t* tau_max) {
    API_BEGIN
    SBV2_REQUIRE(tau_min && tau_max, "bad arguments");
    const PitchSpec sp = pitch_spec(sample_rate, 1, f0_min, f0_max, 0.5);   // (hop and threshold have no part in the lags)
    *tau_min = sp.tau_min;
    *tau_max = sp.tau_max;
    API_END
}

int sbv2_marks_spans(const int64_t* durations, int64_t n_tokens, int32_t hop, int64_t place, const sbv2_pcm_format* fmt, int64_t* start, int64_t* end) {
    API_BEGIN
    const PcmFmtSpec spec = pcm_format_spec(fmt);
    marks_spans(durations, n_tokens, hop, place, spec, start, end);
    API_END
}

// Pinned host memory for PCM destinations: a device -> host copy into pageable memory is staged by the runtime at a fraction of the
// PCIe rate; into these buffers it is one DMA that overlaps the other execution context's kernels.
void* sbv2_host_alloc(size_t bytes) {
    void* p = nullptr;
    if (hipHostMalloc(&p, std::max<size_t>(bytes, 64), hipHostMallocDefault) != hipSuccess) {
        set_last_error("hipHostMalloc failed");
        return nullptr;
    }
    return p;
}
void sbv2_host_free(void* p) {
    if (p) (void)hipHostFree(p);
}
}  // extern "C"
