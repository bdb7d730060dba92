// extern "C" boundary of libsbv2_hip.so (see include/sbv2_hip.h for what each entry point replaces); the formatted fetches are in fetch.cpp.
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

// sbv2_assist onto the run's tables (the contract above the struct, include/sbv2_hip.h); every check here, before any GPU work
AssistSpec assist_spec(const sbv2_assist* a, int64_t n) {
    AssistSpec s;
    if (!a) return s;
    SBV2_REQUIRE(a->reserved == 0, "sbv2_assist.reserved must be 0");
    SBV2_REQUIRE(a->n_texts >= 1 && a->n_texts < (1 << 20), "sbv2_assist.n_texts must be >= 1: " + std::to_string(a->n_texts));
    SBV2_REQUIRE(a->token_ids && a->s_lens && a->text_of && a->weight, "sbv2_assist has null fields (token_ids, s_lens, text_of, weight)");
    const int A = (int)a->n_texts;
    for (int t = 0; t < A; ++t) {
        SBV2_REQUIRE(a->s_lens[t] >= 1 && a->s_lens[t] < (1 << 20),
                     "s_lens of assist text " + std::to_string(t) + " must be in [1, 2^20): " + std::to_string(a->s_lens[t]));
        s.total += a->s_lens[t];
    }
    s.rows = assist_row_table(n, A, a->text_of, a->weight);
    bool used = false;
    for (int64_t u = 0; u < n; ++u) used = used || a->text_of[u] >= 0;
    if (!used) return AssistSpec();   // every text_of is -1: the run without an assist
    s.A = A;
    s.ids = a->token_ids;
    s.lens = a->s_lens;
    return s;
}
std::vector<AssistRow> assist_row_table(int64_t n, int A, const int32_t* text_of, const double* weight) {
    std::vector<AssistRow> rows((size_t)n, AssistRow{-1, 0.f, 1.f, 0});
    for (int64_t u = 0; u < n; ++u) {
        const int32_t t = text_of[u];
        SBV2_REQUIRE(t >= -1 && t < A, "text_of of row " + std::to_string(u) + " must be in [-1, " + std::to_string(A) + "): " + std::to_string(t));
        if (t < 0) continue;
        const double w = weight[u];
        SBV2_REQUIRE(w >= 0.0 && w <= 1.0, "assist weight of row " + std::to_string(u) + " must be in [0, 1]: " + std::to_string(w));   // (a NaN fails both)
        if (w == 0.0) continue;   // the plain gather, bit for bit
        rows[u] = AssistRow{t, (float)w, (float)(1.0 - w), 0};
    }
    return rows;
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
                      const int64_t* word2ph, const AssistSpec* assist) {
    HIP_CHECK(hipStreamSynchronize(vm.stream()));  // this context's previous batch may still be reading the DeBERTa output plane
    std::vector<int> a_start, a_len;
    if (assist && assist->A > 0) {
        // the assist sequences ride behind the batch's in ONE forward: the batch's rows lie where they lie without them
        int64_t total = 0;
        for (int u = 0; u < v.n; ++u) {
            SBV2_REQUIRE(s_lens[u] >= 1 && s_lens[u] < (1 << 20), "bad sequence length");
            total += s_lens[u];
        }
        std::vector<int64_t> ids(token_ids, token_ids + total), lens(s_lens, s_lens + v.n);
        ids.insert(ids.end(), assist->ids, assist->ids + assist->total);
        lens.insert(lens.end(), assist->lens, assist->lens + assist->A);
        bm.forward(v.n + assist->A, ids.data(), nullptr, lens.data());
        for (int a = 0; a < assist->A; ++a) {
            a_start.push_back(bm.layout().start[v.n + a]);
            a_len.push_back(bm.layout().len[v.n + a]);
        }
        v.assist_n = assist->A;
        v.assist_start = a_start.data();
        v.assist_len = a_len.data();
        v.assist_rows = assist->rows.data();
    } else {
        bm.forward(v.n, token_ids, nullptr, s_lens);
    }
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
// (assist == NULL, or an assist no row names: sbv2_pipeline_run_opts itself, launch for launch)
int sbv2_pipeline_run_assist(sbv2_pipeline* p, const sbv2_batch* batch, const sbv2_utt_options* opts, const sbv2_assist* assist, const int64_t* token_ids,
                             const int64_t* s_lens, const int64_t* word2ph, int64_t* pcm_lens) {
    API_BEGIN
    VitsBatch v = to_batch(batch);
    apply_utt_options(&v, opts);
    const AssistSpec as = assist_spec(assist, v.n);
    SBV2_REQUIRE(p && token_ids && s_lens && word2ph && pcm_lens, "bad arguments");
    const int ctx = (int)(p->calls % p->contexts());
    ++p->calls;
    pipeline_run_one(p->bm(ctx), p->vm(ctx), v, token_ids, s_lens, word2ph, &as);
    for (int i = 0; i < v.n; ++i) pcm_lens[i] = p->vm(ctx).pcm_lens()[i];
    API_END
}
int sbv2_pipeline_run_opts(sbv2_pipeline* p, const sbv2_batch* batch, const sbv2_utt_options* opts, const int64_t* token_ids, const int64_t* s_lens,
                           const int64_t* word2ph, int64_t* pcm_lens) {
    return sbv2_pipeline_run_assist(p, batch, opts, nullptr, token_ids, s_lens, word2ph, pcm_lens);
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

int sbv2_loudness_kweight(int32_t sample_rate, double* coef) {
    API_BEGIN
    SBV2_REQUIRE(coef, "bad arguments");
    loudness_kweight(sample_rate, coef);
    API_END
}

int32_t sbv2_voice_tile(void) { return Voice::kTile; }

int32_t sbv2_dynamics_tile(void) { return Dynamics::kTile; }

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
