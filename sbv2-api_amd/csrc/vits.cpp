// Style-Bert-VITS2 JP-Extra synthesizer (the graph behind `model::synthesize`, crates/sbv2_core/src/model.rs:53-111,
// exported from SynthesizerTrn.infer by scripts/convert/convert_model.py:89-113).
//
// A batch of utterances is PACKED along the time axis (SegLayout): text-rate planes [C][sum T_text + gaps] and frame-rate
// planes [C][sum T_frames + gaps]; the zero gaps play the role of every convolution's zero padding, every kernel re-zeroes
// them through its column mask, and attention is grouped per (utterance, head).  So each utterance's result is the
// reference's batch-1 result (the reference cannot batch: model.rs:66-79) while every launch covers the whole batch.
// Stage by stage this follows oracle/sbv2_oracle.py::vits_forward.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>

#include <atomic>
#include "models.h"

namespace sbv2 {

// keys / values of the flow's attention as pre-split bf16 planes (sbv2_debug_set_flash_parts, for the test that holds the attention kernels to each other:
// 1 = the default policy below, 2: at every length, 3: at every length on the un-pipelined kernel k_vits_flash_x3p, 4: at every length on k_vits_flash_x3q's
// 8-wave shape, 0: never = converted per key tile inside the attention kernel; bit-identical)
static std::atomic<int> g_flash_parts{1};
bool flash_parts_enabled() { return g_flash_parts.load(std::memory_order_relaxed) != 0; }
static int flash_parts_mode() { return g_flash_parts.load(std::memory_order_relaxed); }
int set_flash_parts(int on) { return g_flash_parts.exchange(on); }

// sbv2_debug_set_sdp_all: 1 = every row of every call goes through the stochastic duration predictor on the full text layout, whatever its sdp_ratio
// (what the exported graph does); 0 (default) = only the rows whose ratio is not 0 (VitsModel::forward).  For tests and same-process A/B.
static std::atomic<int> g_sdp_all{0};
bool sdp_all() { return g_sdp_all.load(std::memory_order_relaxed) != 0; }
int set_sdp_all(int on) { return g_sdp_all.exchange(on != 0); }

AttnPlan make_attn_plan(const SegLayout& lay, int H, int heads, int ld, int window, Arena& ar, hipStream_t stream, bool scores) {
    AttnPlan pl;
    const int dk = H / heads;
    pl.ng = lay.n * heads;
    pl.maxT = lay.max_len();
    pl.lds = round_up(pl.maxT, 4);
    std::vector<AttnGroup> ag(pl.ng);
    std::vector<GemmGroup> st(pl.ng), pv(pl.ng);
    int64_t s_off = 0, w_off = 0;
    for (int u = 0; u < lay.n; ++u)
        for (int h = 0; h < heads; ++h) {
            const int gi = u * heads + h;
            const int T = lay.len[u];
            AttnGroup& a = ag[gi];
            a.qk_off = (int64_t)h * dk * ld + lay.start[u];
            a.s_off = s_off;
            a.aux_off = w_off;
            a.aux2_off = 0;
            a.T = T;
            a.lds = pl.lds;
            a.col0 = lay.start[u];
            a.head = h;
            st[gi] = GemmGroup{a.qk_off, a.qk_off, s_off, 0, T, T, dk, T};                        // S^T = K^T Q
            pv[gi] = GemmGroup{(int64_t)lay.start[u] * H + h * dk, s_off, a.qk_off, 0, dk, T, T, T};  // ctx = V P^T
            pl.flops += 2.0 * (double)T * T * dk;
            s_off += (int64_t)T * pl.lds;
            w_off += (int64_t)(2 * window + 1) * pl.lds;
        }
    if (scores) {   // the unfused path materialises the T x T score block and the band of probabilities
        pl.S = ar.array<float>((size_t)s_off);
        pl.PW = ar.array<float>((size_t)w_off);
    }
    pl.d_ag = ar.array<AttnGroup>(pl.ng);
    pl.d_st = ar.array<GemmGroup>(pl.ng);
    pl.d_pv = ar.array<GemmGroup>(pl.ng);
    {
        UploadBatch ub(ar);
        ar.upload(pl.d_ag, ag.data(), sizeof(AttnGroup) * pl.ng, stream);
        ar.upload(pl.d_st, st.data(), sizeof(GemmGroup) * pl.ng, stream);
        ar.upload(pl.d_pv, pv.data(), sizeof(GemmGroup) * pl.ng, stream);
    }
    return pl;
}

void grouped_gemm(const float* A, int lda, const float* B, int ldb, float* C, int ldc, const GemmGroup* grp, int ng, int maxM, int maxN,
                  float alpha, double flops, hipStream_t s) {
    ConvParams p;
    p.A = A;
    p.lda = lda;
    p.B = B;
    p.ldb = ldb;
    p.C = C;
    p.ldc = ldc;
    p.alpha = alpha;
    p.groups = grp;
    p.ngroups = ng;
    p.maxM = maxM;
    p.maxN = maxN;
    p.flops_hint = flops;
    launch_conv(p, s);
}

// The split-bf16 attention reads its keys / values as bf16 hi / lo planes written by the q | k | v product's epilogue next to the f32
// plane (attn_flash.hip, k_vits_flash_x3p: no conversion per key tile; the same bits as converting while staging).
// Which kernel (same bits, so the choice is free).  The software-pipelined kernel on pre-split tiles (k_vits_flash_x3q, attn_flash.hip) at every size when
// the head dimension fits its DMA blocks: 4-wave workgroups while they leave at most one per CU (a single utterance: 58 us per launch at 897 frames
// against 84 for k_vits_flash_x3p and ~80 for the converting kernel), 8-wave workgroups beyond (32 x 897 frames: 84 us against 113; the q | k | v product
// then writes q as f32 and k / v as parts only: the same bytes).  Otherwise the un-pipelined pre-split kernel from 4096 frames (at 897
// frames x 32 it is slower than converting, 138 against 124 us; at 14 001 it wins) and for launches of <= 64 workgroups; the converting kernel for the rest.
// set_flash_parts: 2 = parts at every length, 3 = ... on the un-pipelined kernel, 4 = ... on the 8-wave shape, 0 = never (the tests).
FlashChoice flash_choice(const AttnPlan& pl, int SP, bool split_attn, int dk) {
    constexpr int parts_min_t = 4096, parts_max_wgs = 64;
    const int64_t attn_wgs = (int64_t)((pl.maxT + 127) / 128) * pl.ng;
    FlashChoice c;
    c.kv_parts = SP && split_attn && flash_parts_enabled() &&
                 ((flash_parts_mode() != 3 && flash_pipelined_usable(dk)) || pl.maxT >= parts_min_t || attn_wgs <= parts_max_wgs || flash_parts_mode() >= 2);
    c.pipelined = flash_parts_mode() == 3 ? 0 : (flash_parts_mode() == 4 ? 2 : 1);
    return c;
}

VitsModel::Encoder VitsModel::load_encoder(const std::string& p, int n_layers) {
    Encoder e;
    const int Hh = cfg_.hidden, dkk = cfg_.hidden / cfg_.heads, nwin = 2 * cfg_.window + 1;
    e.spk_w = ws_->tensor(p + "spk_emb_linear.weight", {Hh, cfg_.gin});
    e.spk_b = ws_->tensor(p + "spk_emb_linear.bias", {Hh});
    e.layers.resize(n_layers);
    for (int i = 0; i < n_layers; ++i) {
        EncLayer& L = e.layers[i];
        const std::string a = p + "attn_layers." + std::to_string(i) + ".";
        L.attn.q = ws_->conv(a + "conv_q");
        L.attn.k = ws_->conv(a + "conv_k");
        L.attn.v = ws_->conv(a + "conv_v");
        L.attn.o = ws_->conv(a + "conv_o");
        L.attn.qkv = ws_->conv_cat({a + "conv_q", a + "conv_k", a + "conv_v"});
        L.attn.erk = ws_->tensor(a + "emb_rel_k", {nwin, dkk});     // [1][2w+1][dk]: shared by the heads
        L.attn.erv = ws_->tensor(a + "emb_rel_v", {nwin, dkk});
        L.n1g = ws_->tensor(p + "norm_layers_1." + std::to_string(i) + ".gamma", {Hh});
        L.n1b = ws_->tensor(p + "norm_layers_1." + std::to_string(i) + ".beta", {Hh});
        L.n2g = ws_->tensor(p + "norm_layers_2." + std::to_string(i) + ".gamma", {Hh});
        L.n2b = ws_->tensor(p + "norm_layers_2." + std::to_string(i) + ".beta", {Hh});
        L.ffn1 = ws_->conv(p + "ffn_layers." + std::to_string(i) + ".conv_1");
        L.ffn2 = ws_->conv(p + "ffn_layers." + std::to_string(i) + ".conv_2");
        for (const PackedConv* c : {&L.attn.q, &L.attn.k, &L.attn.v, &L.attn.o}) ws_->expect(*c, a + "conv_*", Hh, Hh, 1);
        ws_->expect(L.ffn1, p + "ffn_layers.conv_1", cfg_.filter, Hh, L.ffn1.k);
        ws_->expect(L.ffn2, p + "ffn_layers.conv_2", Hh, cfg_.filter, L.ffn1.k);
    }
    return e;
}

VitsModel::DDS VitsModel::load_dds(const std::string& p, int) {
    DDS d;
    for (int i = 0; i < cfg_.sdp_dds_layers; ++i) {
        const std::string s = std::to_string(i);
        const HostTensor& w = ws_->blob().get(p + "convs_sep." + s + ".weight");
        SBV2_REQUIRE(w.dims.size() == 3 && w.dims[2] == 3, "DDSConv depthwise kernel must be 3");
        const int Hd = cfg_.hidden;
        d.sep_w.push_back(ws_->tensor(p + "convs_sep." + s + ".weight", {Hd, 3}));
        d.sep_b.push_back(ws_->tensor(p + "convs_sep." + s + ".bias", {Hd}));
        d.pw.push_back(ws_->conv(p + "convs_1x1." + s));
        ws_->expect(d.pw.back(), p + "convs_1x1." + s, Hd, Hd, 1);
        d.n1g.push_back(ws_->tensor(p + "norms_1." + s + ".gamma", {Hd}));
        d.n1b.push_back(ws_->tensor(p + "norms_1." + s + ".beta", {Hd}));
        d.n2g.push_back(ws_->tensor(p + "norms_2." + s + ".gamma", {Hd}));
        d.n2b.push_back(ws_->tensor(p + "norms_2." + s + ".beta", {Hd}));
    }
    return d;
}

VitsModel::VitsModel(const Blob& blob, int device) : device_(device) {
    SBV2_REQUIRE(blob.kind == 2, "weight container is not a VITS (kind 2) model");
    HIP_CHECK(hipSetDevice(device));
    HIP_CHECK(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));  // never serialised against the NULL stream (e.g. RCCL launched by the caller)
    f16x3_sat_prepare();
    sat_watch_.baseline();
    const std::string& js = blob.config_json;
    auto I = [&](const char* k) { return (int)json_number(js, k); };
    cfg_.n_vocab = I("n_vocab"); cfg_.n_tones = I("n_tones"); cfg_.n_langs = I("n_langs"); cfg_.n_speakers = I("n_speakers");
    cfg_.hidden = I("hidden"); cfg_.inter = I("inter"); cfg_.filter = I("filter"); cfg_.heads = I("heads");
    cfg_.enc_layers = I("enc_layers"); cfg_.enc_kernel = I("enc_kernel"); cfg_.window = I("window"); cfg_.gin = I("gin");
    cfg_.style_dim = I("style_dim"); cfg_.bert_dim = I("bert_dim"); cfg_.cond_layer_idx = I("cond_layer_idx");
    cfg_.flow_n = I("flow_n"); cfg_.flow_layers = I("flow_layers"); cfg_.flow_kernel = I("flow_kernel");
    cfg_.dp_filter = I("dp_filter"); cfg_.dp_kernel = I("dp_kernel"); cfg_.sdp_kernel = I("sdp_kernel");
    cfg_.sdp_flows = I("sdp_flows"); cfg_.sdp_bins = I("sdp_bins"); cfg_.sdp_dds_layers = I("sdp_dds_layers");
    cfg_.sdp_tail = (float)json_number(js, "sdp_tail");
    cfg_.up_rates = json_int_array(js, "up_rates");
    cfg_.up_kernels = json_int_array(js, "up_kernels");
    cfg_.res_kernels = json_int_array(js, "res_kernels");
    cfg_.res_dilations = json_int_array2(js, "res_dilations");
    cfg_.up_initial = I("up_initial");
    SBV2_REQUIRE(cfg_.sdp_kernel == 3, "DDSConv kernel must be 3");
    SBV2_REQUIRE(cfg_.hidden % cfg_.heads == 0 && (cfg_.hidden / cfg_.heads) % 4 == 0, "head size must be a multiple of 4");
    SBV2_REQUIRE(cfg_.inter % 8 == 0, "flow channels must be a multiple of 8");
    SBV2_REQUIRE(cfg_.res_dilations.size() == cfg_.res_kernels.size(), "resblock config mismatch");

    // Arithmetic of the k >= 3 convolutions outside the decoder, i.e. the flow's k = 5 FFN convs (SBV2_GEMM): split-bf16 through the
    // k-major variant of conv_cl.hip by default (203 TFLOP/s algorithmic against ~60 for the f32 MFMA kernel on those shapes), or
    // f32 | bf16 | f16.  1x1 products always stay on the f32 MFMA kernel: the k-major variant transposes while staging and a 1x1 has too
    // few MFMAs per chunk to pay for it (~48 TFLOP/s measured).
    int gemm_parts = 2;
    if (const char* m = getenv("SBV2_GEMM")) {
        const std::string v(m);
        if (v == "f32") gemm_parts = 0;
        else if (v == "bf16") gemm_parts = 1;
        else if (v == "f16") gemm_parts = 3;
        else SBV2_REQUIRE(v == "bf16x3" || v.empty(), "SBV2_GEMM must be f32, bf16x3, bf16 or f16");
    }
    ws_.reset(new WeightStore(blob, gemm_parts));
    WeightStore& w = *ws_;
    // The text side decides the INTEGER durations (ceil(exp(logw) * length_scale)): text encoder and both duration predictors run on
    // the exact-f32 kernels whatever SBV2_GEMM says.  (Round 2 measured their k = 3 convolutions on the split-bf16 matrix cores behind a knob: one flipped
    // duration per 102 800 symbols, profiles/r02_flip_rate.json; the knob and its script are gone, the text side is exact f32.)
    w.set_cl_parts(0);
    // every tensor's shape is checked against the config before a kernel indexes it (a container / imported ONNX whose config and
    // weights disagree is refused here)
    const int Hc = cfg_.hidden, Gc = cfg_.gin, Ic = cfg_.inter, Fd = cfg_.dp_filter;
    SBV2_REQUIRE(cfg_.n_vocab >= 1 && cfg_.n_tones >= 1 && cfg_.n_langs >= 1 && cfg_.n_speakers >= 1 && Hc >= 4 && Gc >= 1 && Ic >= 2 && Fd >= 1 &&
                     cfg_.enc_layers >= 1 && cfg_.flow_n >= 1 && cfg_.flow_layers >= 1 && cfg_.sdp_bins >= 2 && cfg_.sdp_bins <= 16 && cfg_.window >= 0,
                 "bad VITS config");
    emb_g_ = w.tensor("emb_g.weight", {cfg_.n_speakers, Gc});
    emb_ = w.tensor("enc_p.emb.weight", {cfg_.n_vocab, Hc});
    tone_emb_ = w.tensor("enc_p.tone_emb.weight", {cfg_.n_tones, Hc});
    lang_emb_ = w.tensor("enc_p.language_emb.weight", {cfg_.n_langs, Hc});
    bert_proj_ = w.conv("enc_p.bert_proj");
    w.expect(bert_proj_, "enc_p.bert_proj", Hc, cfg_.bert_dim, 1);
    style_w_ = w.tensor("enc_p.style_proj.weight", {Hc, cfg_.style_dim});
    style_b_ = w.tensor("enc_p.style_proj.bias", {Hc});
    enc_p_ = load_encoder("enc_p.encoder.", cfg_.enc_layers);
    enc_proj_ = w.conv("enc_p.proj");
    w.expect(enc_proj_, "enc_p.proj", 2 * Ic, Hc, 1);
    dp_c1_ = w.conv("dp.conv_1");
    dp_c2_ = w.conv("dp.conv_2");
    dp_proj_ = w.conv("dp.proj");
    w.expect(dp_c1_, "dp.conv_1", Fd, Hc, cfg_.dp_kernel);
    w.expect(dp_c2_, "dp.conv_2", Fd, Fd, cfg_.dp_kernel);
    w.expect(dp_proj_, "dp.proj", 1, Fd, 1);
    dp_n1g_ = w.tensor("dp.norm_1.gamma", {Fd}); dp_n1b_ = w.tensor("dp.norm_1.beta", {Fd});
    dp_n2g_ = w.tensor("dp.norm_2.gamma", {Fd}); dp_n2b_ = w.tensor("dp.norm_2.beta", {Fd});
    dp_cond_w_ = w.tensor("dp.cond.weight", {Hc, Gc}); dp_cond_b_ = w.tensor("dp.cond.bias", {Hc});
    sdp_pre_ = w.conv("sdp.pre");
    sdp_proj_ = w.conv("sdp.proj");
    w.expect(sdp_pre_, "sdp.pre", Hc, Hc, 1);
    w.expect(sdp_proj_, "sdp.proj", Hc, Hc, 1);
    sdp_cond_w_ = w.tensor("sdp.cond.weight", {Hc, Gc}); sdp_cond_b_ = w.tensor("sdp.cond.bias", {Hc});
    sdp_ea_m_ = w.tensor("sdp.flows.0.m", {2});
    // (an onnxsim-processed export has exp(-logs) folded into a constant: import.cpp rule 7 stores it as flows.0.exp_neg_logs)
    if (blob.has("sdp.flows.0.logs") || !blob.has("sdp.flows.0.exp_neg_logs")) sdp_ea_logs_ = w.tensor("sdp.flows.0.logs", {2});
    else sdp_ea_scale_ = w.tensor("sdp.flows.0.exp_neg_logs", {2});
    sdp_dds_ = load_dds("sdp.convs.", cfg_.hidden);
    for (int i = 2; i <= cfg_.sdp_flows; ++i) {  // ConvFlow 1 is the "useless vflow" dropped in reverse mode
        const std::string p = "sdp.flows." + std::to_string(2 * i - 1) + ".";
        ConvFlow cf;
        cf.pre_w = w.tensor(p + "pre.weight", {Hc});
        cf.pre_b = w.tensor(p + "pre.bias", {Hc});
        cf.dds = load_dds(p + "convs.", cfg_.hidden);
        cf.proj = w.conv(p + "proj");
        SBV2_REQUIRE(cf.proj.cout == 3 * cfg_.sdp_bins - 1, "ConvFlow projection size");
        sdp_cf_.push_back(cf);
    }
    w.set_cl_parts(gemm_parts);   // the flow only shapes the (continuous) latent: split-bf16 for its k = 5 FFN convs
    // ... and for the 1x1 products of its attention layers (q | k | v and the output projection: 48 launches of a batch-32 step) through
    // gemm_bfs.hip with pre-split operands.  SBV2_FLOW_1X1=f32 keeps them on
    // the exact-f32 kernel; SBV2_GEMM=f32 does as well.
    // Operand format: f16x3 (f16 hi + scaled f16 lo: 22 mantissa bits, common.h) costs the same three MFMAs per product as bf16x3 and is
    // 20x closer to the f32 product on these shapes (tools/bfs_probe.py), so it is the default; SBV2_FLOW_1X1=bf16x3 keeps the two-bf16 split.
    int flow_bfs = gemm_parts == 2 && (Hc & 15) == 0 ? kPartsF16x3 : 0;
    if (const char* m = getenv("SBV2_FLOW_1X1")) {
        const std::string v(m);
        SBV2_REQUIRE(v == "f16x3" || v == "bf16x3" || v == "f32" || v.empty(), "SBV2_FLOW_1X1 must be f32, bf16x3 or f16x3");
        if (v == "f32") flow_bfs = 0;
        else if (v == "bf16x3" && flow_bfs) flow_bfs = 2;
    }
    w.set_bfs_parts(flow_bfs);
    for (int i = 0; i < cfg_.flow_n; ++i) {
        const std::string p = "flow.flows." + std::to_string(2 * i) + ".";
        Coupling c;
        c.pre = w.conv(p + "pre");
        c.post = w.conv(p + "post");
        w.expect(c.pre, p + "pre", Hc, Ic / 2, 1);
        w.expect(c.post, p + "post", Ic / 2, Hc, 1);
        c.enc = load_encoder(p + "enc.", cfg_.flow_layers);
        flows_.push_back(c);
    }
    // the k-major decoder weights stay exact f32 (SBV2_DECODER=f32 is the exact reference path); the bf16 decoder has its own packing
    w.set_cl_parts(0);
    w.set_bfs_parts(0);
    dec_pre_ = w.conv("dec.conv_pre");
    w.expect(dec_pre_, "dec.conv_pre", cfg_.up_initial, Ic, dec_pre_.k);
    dec_cond_w_ = w.tensor("dec.cond.weight", {cfg_.up_initial, Gc});
    dec_cond_b_ = w.tensor("dec.cond.bias", {cfg_.up_initial});
    {
        const HostTensor& pw = blob.get("dec.conv_post.weight");
        SBV2_REQUIRE(pw.dims.size() == 3 && pw.dims[0] == 1 && pw.dims[2] >= 1 && pw.dims[2] <= 15 && (pw.dims[2] & 1), "dec.conv_post.weight must be [1][C][odd k]");
        int cl = cfg_.up_initial;
        for (size_t i = 0; i < cfg_.up_rates.size(); ++i) cl /= 2;
        dec_post_w_ = w.tensor("dec.conv_post.weight", {cl, pw.dims[2]});
        dec_post_k_ = (int)pw.dims[2];
    }
    SBV2_REQUIRE(cfg_.up_rates.size() == cfg_.up_kernels.size() && !cfg_.up_rates.empty(), "upsampling config mismatch");
    int C = cfg_.up_initial;
    const int nk = (int)cfg_.res_kernels.size();
    for (size_t i = 0; i < cfg_.up_rates.size(); ++i) {
        Stage st;
        st.rate = cfg_.up_rates[i];
        st.up = w.upsample("dec.ups." + std::to_string(i), st.rate, (cfg_.up_kernels[i] - st.rate) / 2);
        SBV2_REQUIRE(st.up.cin == C && st.up.cout == C / 2, "dec.ups." + std::to_string(i) + ": channel counts do not follow up_initial / 2^i");
        C /= 2;
        st.ch = C;
        for (int j = 0; j < nk; ++j) {
            ResBranch rb;
            rb.k = cfg_.res_kernels[j];
            rb.dil = cfg_.res_dilations[j];
            const std::string p = "dec.resblocks." + std::to_string(i * nk + j) + ".";
            for (size_t n = 0; n < rb.dil.size(); ++n) {
                rb.c1.push_back(w.conv(p + "convs1." + std::to_string(n)));
                rb.c2.push_back(w.conv(p + "convs2." + std::to_string(n)));
                w.expect(rb.c1.back(), p + "convs1", C, C, rb.k);
                w.expect(rb.c2.back(), p + "convs2", C, C, rb.k);
            }
            st.branches.push_back(rb);
        }
        stages_.push_back(st);
    }
    // decoder arithmetic: exact f32 MFMA (default) | split-bf16 MFMA, f32-grade | plain bf16 MFMA
    //   bf16x3 (default when every decoder channel count is a multiple of 16): split-bf16 MFMA, waveform within ~2e-6 of the f32 path
    //   f32: exact f32 MFMA on k-major planes;  bf16: plain bf16 operands (~9e-4 waveform error at a 0.1 peak);
    //   f16: fp16 operands, same speed as bf16, 1.3e-4 (relative to the signal that is ~1e-3: opt-in, not the default)
    bool cl_ok = cfg_.inter % 16 == 0;
    for (const Stage& st : stages_) cl_ok = cl_ok && st.ch % 16 == 0;
    dec_mode_ = cl_ok ? 1 : 0;
    if (const char* m = getenv("SBV2_DECODER")) {
        const std::string v(m);
        if (v == "bf16x3") dec_mode_ = 1;
        else if (v == "bf16") dec_mode_ = 2;
        else if (v == "f16") dec_mode_ = 3;
        else if (v == "f32") dec_mode_ = 0;
        else SBV2_REQUIRE(v.empty(), "SBV2_DECODER must be f32, bf16x3, bf16 or f16");
        SBV2_REQUIRE(dec_mode_ == 0 || cl_ok, "SBV2_DECODER: the bf16 MFMA decoder needs channel counts that are multiples of 16");
    }
    if (dec_mode_) load_decoder_cl(blob);
}

VitsModel* VitsModel::clone() const {
    HIP_CHECK(hipSetDevice(device_));
    VitsModel* c = new VitsModel(*this);   // shares ws_ (device weights); Arena copies are empty
    c->stream_ = nullptr;
    HIP_CHECK(hipStreamCreateWithFlags(&c->stream_, hipStreamNonBlocking));
    c->after_ev_ = nullptr;   // created on first use PER CONTEXT: a copied handle would be destroyed twice (and waited on after its first destruction)
    c->pcm_ = nullptr;
    c->pcm_total_ = 0;
    c->pcm_lens_.clear();
    c->pcm_offs_.clear();
    c->traces_.clear();
    c->chunk_.reset();
    c->burst_.reset();
    c->sout_.reset();   // (with it the carried limiter, encoder tail and reductions: a clone's stream shares none of them)
    c->sformatted_ = false;
    c->z_ = Plane{};
    c->trace_ = false;
    return c;
}

VitsModel::~VitsModel() {
    (void)hipSetDevice(device_);
    if (after_ev_) (void)hipEventDestroy(after_ev_);
    if (stream_) (void)hipStreamDestroy(stream_);
}

void VitsModel::trace(const std::string& name, Plane p, const SegLayout& lay, int div) {
    if (!trace_) return;
    Plane c = keep_.plane(p.C, p.L);
    HIP_CHECK(hipMemcpy2DAsync(c.p, sizeof(float) * c.ld, p.p, sizeof(float) * p.ld, sizeof(float) * p.L, p.C, hipMemcpyDeviceToDevice, stream_));
    traces_[name] = TraceEntry{c, &lay, div};
}

bool VitsModel::get_trace(const std::string& name, int utt, std::vector<float>& out, int& rows, int& cols) {
    auto it = traces_.find(name);
    if (it == traces_.end()) return false;
    const TraceEntry& t = it->second;
    if (utt < 0 || utt >= t.lay->n) return false;
    HIP_CHECK(hipSetDevice(device_));
    rows = t.p.C;
    cols = t.lay->len[utt] * t.div;
    out.resize((size_t)rows * cols);
    HIP_CHECK(hipStreamSynchronize(stream_));
    HIP_CHECK(hipMemcpy2D(out.data(), sizeof(float) * cols, t.p.p + (size_t)t.lay->start[utt] * t.div, sizeof(float) * t.p.ld,
                          sizeof(float) * cols, rows, hipMemcpyDeviceToHost));
    return true;
}

// attentions.Encoder (post-LN, window-relative attention, FFN with 'same' convolutions, speaker vector before layer 2)
void VitsModel::run_encoder(const Encoder& e, Plane x, const SegLayout& lay, const float* spk_vec, Arena& ar) {
    const int H = x.C, heads = cfg_.heads, dk = H / heads, N = lay.L;
    const Arena::Mark mk = ar.mark();
    // SBV2_ATTN=unfused keeps the four-launch attention (grouped GEMM, softmax, grouped GEMM, relative-value add) for A/B runs
    static const bool fused = !(getenv("SBV2_ATTN") && std::string(getenv("SBV2_ATTN")) == "unfused");
    // SBV2_ATTN=f32 keeps the fused kernel on the exact-f32 MFMA everywhere; by default an encoder whose convs run on the split-bf16
    // matrix cores (the flow: nothing there feeds the integer durations) takes the split-bf16 attention as well
    static const bool attn_f32 = getenv("SBV2_ATTN") && std::string(getenv("SBV2_ATTN")) == "f32";
    const bool split_attn = !attn_f32 && e.layers[0].ffn1.cl.parts == 2 && (H / heads) % 16 == 0;
    const AttnPlan pl = make_attn_plan(lay, H, heads, x.ld, cfg_.window, ar, stream_, !fused);
    Plane QKV = ar.plane(3 * H, N);
    Plane Q = QKV.rows(0, H), K = QKV.rows(H, H), ctx = ar.plane(H, N), Y = ar.plane(H, N);
    SBV2_REQUIRE(Q.ld == x.ld, "plane pitch mismatch");
    Plane F = ar.plane(e.layers[0].ffn1.cout, N);
    constexpr bool cl_ffn = true;
    const PackedConv& f1 = e.layers[0].ffn1;
    const PackedConv& f2 = e.layers[0].ffn2;
    float* Fcl = (cl_ffn && f1.cl.parts && f2.cl.parts && f1.k >= 3 && f2.k >= 3 && (f1.cout & 15) == 0) ? ar.array<float>((size_t)N * f1.cout) : nullptr;
    float* VT = fused ? nullptr : ar.array<float>((size_t)N * H);
    Plane Vp = QKV.rows(2 * H, H);
    fill_zero(ctx.p, sizeof(float) * (size_t)H * ctx.ld, stream_);
    const float qscale = 1.0f / std::sqrt((float)dk);
    // 1x1 products on pre-split operands (gemm_bfs.hip; the flow by default): the parts of x are written by the LayerNorm that produces x
    // (by split_planes for the encoder's input and after the speaker vector is added), the parts of the attention output by split_planes
    const int SP = !fused ? 0 : (e.layers[0].attn.qkv.bfs.f16 ? kPartsF16x3 : e.layers[0].attn.qkv.bfs.parts);   // parts code
    SplitPlanes Xs, Cs, QKVs;
    if (SP) {
        Xs = alloc_split(ar, SP, H, N);
        Cs = alloc_split(ar, SP, H, N);
        split_planes(x, Xs, stream_);
    }
    const FlashChoice fc = flash_choice(pl, SP, split_attn, dk);
    const bool kv_parts = fc.kv_parts;
    if (kv_parts) QKVs = alloc_split(ar, 2, 3 * H, N);
    // Large batches: the FFN pair on conv_clx.hip (pre-split chunk-major operands by LDS-DMA instead of conv_cl's transposing register staging):
    // x is split once per layer from its k-major plane (split_cl_km), conv_1's epilogue writes relu(.) as conv_2's operand parts, conv_2 writes
    // the k-major result + residual.  Small launches (a single utterance) stay on conv_cl: since round 5 conv_clx multiplies on 16 x 16 x 32 MFMAs in another
    // summation order, so the two agree to f32 rounding (1e-5 kernel against kernel), not bit for bit.
    const bool clx_ffn = Fcl && f1.cl.parts == 2 && f2.cl.parts == 2 && f1.k == 5 && f2.k == 5 && (H & 63) == 0 && (f1.cout & 63) == 0 &&
                         clx_wanted((int64_t)(N / 256) * (H / 64), 192);
    SplitClPlanes XsC, FsC;
    if (clx_ffn) {
        XsC = make_split_cl(ar.alloc(split_cl_bytes(H, N)), H, N, stream_);
        FsC = make_split_cl(ar.alloc(split_cl_bytes(f1.cout, N)), f1.cout, N, stream_);
    }
    for (size_t i = 0; i < e.layers.size(); ++i) {
        const EncLayer& L = e.layers[i];
        if ((int)i == cfg_.cond_layer_idx && spk_vec) {
            add_segvec(x, spk_vec, H, lay.d_seg_of, 1, lay.d_mask, stream_);
            if (SP) split_planes(x, Xs, stream_);
        }
        if (fused) {
            // (keys / values as parts: q goes to the f32 plane, k and v to the parts only: the bytes of the one-format product)
            if (SP && kv_parts) conv_bfs(L.attn.qkv, Xs, &QKV, &QKVs, nullptr, 1, stream_, ACT_NONE, nullptr, 1.0f, 1.0f, H, H);
            else if (SP) conv_bfs(L.attn.qkv, Xs, &QKV, nullptr, nullptr, 1, stream_);
            else conv_plain(L.attn.qkv, x, QKV, 1, 0, nullptr, 1, stream_);
            if (kv_parts)
                vits_flash_attention_parts(pl.d_ag, pl.ng, pl.maxT, Q.p, Q.ld, QKVs, H, 2 * H, ctx.p, ctx.ld, dk, L.attn.erk, L.attn.erv, cfg_.window,
                                           qscale, stream_, fc.pipelined);
            else
                vits_flash_attention(pl.d_ag, pl.ng, pl.maxT, Q.p, K.p, Vp.p, Q.ld, ctx.p, ctx.ld, dk, L.attn.erk, L.attn.erv, cfg_.window, qscale,
                                     split_attn, stream_);
        } else {
            conv_plain(L.attn.q, x, Q, 1, 0, nullptr, 1, stream_);
            conv_plain(L.attn.k, x, K, 1, 0, nullptr, 1, stream_);
            linear_tokmajor(L.attn.v, x, VT, H, stream_);
            grouped_gemm(K.p, K.ld, Q.p, Q.ld, pl.S, pl.lds, pl.d_st, pl.ng, pl.maxT, pl.maxT, qscale, pl.flops, stream_);
            vits_softmax(pl.d_ag, pl.ng, pl.maxT, pl.S, Q.p, Q.ld, dk, L.attn.erk, cfg_.window, qscale, pl.PW, stream_);
            grouped_gemm(VT, H, pl.S, pl.lds, ctx.p, ctx.ld, pl.d_pv, pl.ng, dk, pl.maxT, 1.0f, pl.flops, stream_);
            vits_relv_add(pl.d_ag, pl.ng, pl.maxT, ctx.p, ctx.ld, dk, L.attn.erv, cfg_.window, pl.PW, stream_);
        }
        if (SP) {
            split_planes(ctx, Cs, stream_);
            conv_bfs(L.attn.o, Cs, &Y, nullptr, nullptr, 1, stream_, ACT_NONE, &x);
        } else {
            conv_plain(L.attn.o, ctx, Y, 1, 0, nullptr, 1, stream_, ACT_NONE, 1.0f, &x);
        }
        layernorm_ch(Y, x, L.n1g, L.n1b, 1e-5f, ACT_NONE, nullptr, 0, lay.d_mask, stream_);
        const int k = L.ffn1.k;
        // FFN: conv_1 -> ReLU -> conv_2 (+ x).  On the matrix-core path the 768-channel intermediate stays channels-last and the ReLU is
        // conv_2's pre-activation (leaky slope 0); otherwise (exact-f32 text side) both convs run on k-major planes.
        const int Fc = L.ffn1.cout;
        if (clx_ffn) {
            split_cl_km(x, 1.0f, XsC, stream_);
            ConvClxParams p1;
            p1.X = XsC;
            p1.W = L.ffn1.cl.wx;
            p1.nmt = L.ffn1.cl.nmt;
            p1.M = Fc;
            p1.N = N;
            p1.K = H;
            p1.ntaps = k;
            p1.shift0 = -(k - 1) / 2;
            p1.shift_step = 1;
            p1.Ys = FsC;
            p1.ys_slope = 0.0f;     // ReLU
            p1.bias = L.ffn1.bias;
            p1.mask = lay.d_mask;
            p1.mask_shift = 0;
            launch_conv_clx(p1, stream_);
            ConvClxParams p2;
            p2.X = FsC;
            p2.W = L.ffn2.cl.wx;
            p2.nmt = L.ffn2.cl.nmt;
            p2.M = H;
            p2.N = N;
            p2.K = Fc;
            p2.ntaps = k;
            p2.shift0 = -(k - 1) / 2;
            p2.shift_step = 1;
            p2.Ykm = Y.p;
            p2.ldykm = Y.ld;
            p2.Rkm = x.p;
            p2.ldrkm = x.ld;
            p2.bias = L.ffn2.bias;
            p2.mask = lay.d_mask;
            p2.mask_shift = 0;
            launch_conv_clx(p2, stream_);
        } else if (Fcl && conv_km_to_cl(L.ffn1, x, Fcl, Fc, 1, (k - 1) / 2, lay.d_mask, 1, stream_)) {
            SBV2_REQUIRE(conv_cl_to_km(L.ffn2, Fcl, Fc, Y, 1, (k - 1) / 2, lay.d_mask, 1, stream_, 0.0f, &x), "FFN: conv_2 has no matrix-core path");
        } else {
            conv_plain(L.ffn1, x, F, 1, (k - 1) / 2, lay.d_mask, 1, stream_, ACT_RELU);
            conv_plain(L.ffn2, F, Y, 1, (k - 1) / 2, lay.d_mask, 1, stream_, ACT_NONE, 1.0f, &x);
        }
        layernorm_ch(Y, x, L.n2g, L.n2b, 1e-5f, ACT_NONE, nullptr, 0, lay.d_mask, stream_, (SP && i + 1 < e.layers.size()) ? &Xs : nullptr);
    }
    ar.rewind(mk);
}

// modules.DDSConv: x += gelu(LN(1x1(gelu(LN(depthwise(x * mask))))))  x 3, dilation 3^i
// (shape_L: the column count the LayerNorm kernels are chosen for, see layernorm_ch; 0 = the plane's own)
void VitsModel::run_dds(const DDS& d, Plane x, const SegLayout& lay, Arena& ar, int shape_L) {
    const Arena::Mark mk = ar.mark();
    Plane a = ar.plane(x.C, x.L), b = ar.plane(x.C, x.L);
    int dil = 1;
    for (size_t i = 0; i < d.pw.size(); ++i) {
        dds_dw_ln_gelu(x, a, d.sep_w[i], d.sep_b[i], dil, d.n1g[i], d.n1b[i], lay.d_mask, stream_, shape_L);
        conv_plain(d.pw[i], a, b, 1, 0, nullptr, 1, stream_);
        layernorm_ch(b, x, d.n2g[i], d.n2b[i], 1e-5f, ACT_GELU, x.p, x.ld, lay.d_mask, stream_, nullptr, shape_L);
        dil *= cfg_.sdp_kernel;
    }
    ar.rewind(mk);
}

// models_jp_extra.Generator
void VitsModel::run_decoder(Arena& ar, Plane z, const SegLayout& fl, const float* cond_vec) {
    const int n = fl.n;
    const int Lf = fl.L;
    Plane cur = ar.plane(cfg_.up_initial, Lf);
    conv_plain(dec_pre_, z, cur, 1, dec_pre_.k / 2, fl.d_mask, 1, stream_);
    add_segvec(cur, cond_vec, cfg_.up_initial, fl.d_seg_of, 1, fl.d_mask, stream_);
    trace("dec_pre", cur, fl, 1);
    int U = 1;
    const int nk = (int)cfg_.res_kernels.size();
    for (size_t si = 0; si < stages_.size(); ++si) {
        const Stage& st = stages_[si];
        U *= st.rate;
        const int Lo = Lf * U;
        Plane XS = ar.plane(st.ch, Lo);
        const Arena::Mark mk = ar.mark();
        Plane XU = ar.plane(st.ch, Lo), T1 = ar.plane(st.ch, Lo), YA = ar.plane(st.ch, Lo), YB = ar.plane(st.ch, Lo);
        for (const auto& g : st.up.groups) {
            ConvParams p;
            p.A = g.w;
            p.lda = g.lda;
            p.a_tap_stride = (int64_t)st.up.cin * g.lda;
            p.B = cur.p;
            p.ldb = cur.ld;
            p.nb = cur.L;
            p.C = XU.p;
            p.ldc = XU.ld;
            p.M = g.nph * st.up.cout;
            p.N = cur.L;
            p.K = st.up.cin;
            p.ntaps = g.ntaps;
            for (int t = 0; t < g.ntaps; ++t) p.shift[t] = g.shift[t];
            p.bias = st.up.bias;
            p.bias_mode = BIAS_ROW;
            p.pre_slope = 0.1f;
            p.mask = fl.d_mask;
            p.mask_div = U;
            p.out_stride = st.rate;
            p.phase_rows = st.up.cout;
            for (int q = 0; q < kMaxPhases; ++q) p.phase_off[q] = g.phase_off[q];
            launch_conv(p, stream_);
        }
        for (int j = 0; j < nk; ++j) {
            const ResBranch& rb = st.branches[j];
            Plane y = XU;
            const int nd = (int)rb.dil.size();
            for (int q = 0; q < nd; ++q) {
                const int d = rb.dil[q];
                conv_plain(rb.c1[q], y, T1, d, d * (rb.k - 1) / 2, fl.d_mask, U, stream_, ACT_NONE, 0.1f);
                if (q + 1 < nd) {
                    Plane yn = (y.p == YA.p) ? YB : YA;
                    conv_plain(rb.c2[q], T1, yn, 1, (rb.k - 1) / 2, fl.d_mask, U, stream_, ACT_NONE, 0.1f, &y);
                    y = yn;
                } else {
                    conv_plain(rb.c2[q], T1, XS, 1, (rb.k - 1) / 2, fl.d_mask, U, stream_, ACT_NONE, 0.1f, &y, 1.0f, 1.0f / nk, j > 0);
                }
            }
        }
        ar.rewind(mk);
        cur = XS;
        trace("dec_stage" + std::to_string(si), cur, fl, U);
    }
    // compact PCM, one contiguous block per utterance
    pcm_lens_.assign(n, 0);
    pcm_offs_.assign(n, 0);
    int64_t tot = 0, maxlen = 0;
    for (int u = 0; u < n; ++u) {
        pcm_offs_[u] = tot;
        pcm_lens_[u] = (int64_t)fl.len[u] * U;
        tot += pcm_lens_[u];
        maxlen = std::max(maxlen, pcm_lens_[u]);
    }
    pcm_total_ = tot;
    pcm_ = ar.array<float>((size_t)tot);
    int64_t* d_off = ar.array<int64_t>(n);
    ar.upload(d_off, pcm_offs_.data(), sizeof(int64_t) * n, stream_);
    conv_post_tanh(cur, dec_post_w_, dec_post_k_, 0.01f, fl.d_start, fl.d_len, d_off, n, U, maxlen, pcm_, stream_);
}

void VitsModel::forward(const VitsBatch& b) {
    HIP_CHECK(hipSetDevice(device_));
    SBV2_REQUIRE(b.n >= 1, "empty batch");
    HIP_CHECK(hipStreamSynchronize(stream_));  // pinned staging of the previous call must be drained before reuse
    arena_.reset();
    keep_.reset();
    traces_.clear();
    if (b.after_stream) {
        if (!after_ev_) HIP_CHECK(hipEventCreateWithFlags(&after_ev_, hipEventDisableTiming));
        HIP_CHECK(hipEventRecord(after_ev_, b.after_stream));
        HIP_CHECK(hipStreamWaitEvent(stream_, after_ev_, 0));
    }
    Arena& ar = arena_;
    const int n = b.n, H = cfg_.hidden, I = cfg_.inter;
    std::vector<int> T(n);
    int64_t total_t = 0;
    for (int u = 0; u < n; ++u) {
        SBV2_REQUIRE(b.t_lens[u] >= 1 && b.t_lens[u] < (1 << 20), "bad text length");
        T[u] = (int)b.t_lens[u];
        total_t += T[u];
    }
    tl_ = make_layout(T, kTextGap, ar, stream_);
    const SegLayout& tl = tl_;
    const int Lt = tl.L;

    // ---- inputs -------------------------------------------------------------------------------------
    std::vector<int> ph(Lt, 0), tn(Lt, 0), lg(Lt, 0), sid(n);
    {
        int64_t e = 0;
        for (int u = 0; u < n; ++u) {
            SBV2_REQUIRE(b.sids[u] >= 0 && b.sids[u] < cfg_.n_speakers, "speaker id out of range");
            sid[u] = (int)b.sids[u];
            for (int t = 0; t < T[u]; ++t, ++e) {
                SBV2_REQUIRE(b.phones[e] >= 0 && b.phones[e] < cfg_.n_vocab && b.tones[e] >= 0 && b.tones[e] < cfg_.n_tones &&
                                 b.langs[e] >= 0 && b.langs[e] < cfg_.n_langs,
                             "phone / tone / language id out of range");
                ph[tl.start[u] + t] = (int)b.phones[e];
                tn[tl.start[u] + t] = (int)b.tones[e];
                lg[tl.start[u] + t] = (int)b.langs[e];
            }
        }
    }
    int* d_ph = ar.array<int>(Lt);
    int* d_tn = ar.array<int>(Lt);
    int* d_lg = ar.array<int>(Lt);
    int* d_sid = ar.array<int>(n);
    RowOpts* d_rows = ar.array<RowOpts>(n);   // every row's options and noise key (seed, index of the utterance in the caller's batch)
    float* d_style = ar.array<float>((size_t)n * cfg_.style_dim);
    std::vector<RowOpts> rows(n);
    for (int u = 0; u < n; ++u) {
        RowOpts& r = rows[u];
        r.seed = b.row_seed ? b.row_seed[u] : b.seed;
        r.index = b.row_index ? (int)b.row_index[u] : b.utt_ids ? (int)b.utt_ids[u] : b.utt0 + u;
        r.sdp_ratio = b.row_sdp_ratio ? b.row_sdp_ratio[u] : b.sdp_ratio;
        r.length_scale = b.row_length_scale ? b.row_length_scale[u] : b.length_scale;
        r.noise_scale = b.row_noise_scale ? b.row_noise_scale[u] : b.noise_scale;
        r.noise_scale_w = b.row_noise_scale_w ? b.row_noise_scale_w[u] : b.noise_scale_w;
        r.pad_ = 0;
    }
    // The stochastic duration predictor's only consumer is k_durations, which multiplies its value by the row's sdp_ratio: a row needs it iff that
    // ratio is not exactly 0 (a denormal ratio counts as needing it).  Decided here, on the host, before anything is enqueued: no row -> the
    // predictor is not run at all; every row -> it runs on the text layout; some rows -> it runs on a second text layout over those rows only, in
    // batch order (sl), fed by gathers, and k_durations reads its plane through a column map.  (sbv2_debug_set_sdp_all(1): every row, always.)
    std::vector<int> sdp_rows;   // the batch rows that go through the predictor
    for (int u = 0; u < n; ++u)
        if (rows[u].sdp_ratio != 0.0f || sdp_all()) sdp_rows.push_back(u);
    const int n_sdp = (int)sdp_rows.size();
    const bool sdp_sub = n_sdp > 0 && n_sdp < n;
    SegLayout sl;                  // the sub-layout (sdp_sub only)
    RowOpts* d_sub_rows = nullptr; // its rows' options, compacted: noise_fill keys by (seed, index, position within the segment), so a row draws its own noise
    int* d_sub_idx = nullptr;      // [n_sdp] batch row of each of its rows
    int* d_sub_src = nullptr;      // [sl.L] column of tl behind each of its columns, -1 in its gaps
    int* d_sdp_col = nullptr;      // [Lt] its column for each column of tl, -1 for none
    {
        // six neighbours in the arena, uploaded in allocation order: one copy (Arena::begin_uploads); the sub-layout's tables ride along
        UploadBatch ub(ar);
        ar.upload(d_ph, ph.data(), sizeof(int) * Lt, stream_);
        ar.upload(d_tn, tn.data(), sizeof(int) * Lt, stream_);
        ar.upload(d_lg, lg.data(), sizeof(int) * Lt, stream_);
        ar.upload(d_sid, sid.data(), sizeof(int) * n, stream_);
        ar.upload(d_rows, rows.data(), sizeof(RowOpts) * n, stream_);
        ar.upload(d_style, b.styles, sizeof(float) * (size_t)n * cfg_.style_dim, stream_);
        if (sdp_sub) {
            std::vector<int> T_sub(n_sdp);
            std::vector<RowOpts> sub_rows(n_sdp);
            for (int j = 0; j < n_sdp; ++j) {
                T_sub[j] = T[sdp_rows[j]];
                sub_rows[j] = rows[sdp_rows[j]];
            }
            sl = make_layout(T_sub, kTextGap, ar, stream_);
            std::vector<int> src(sl.L, -1), col(Lt, -1);
            for (int j = 0; j < n_sdp; ++j)
                for (int t = 0; t < T_sub[j]; ++t) {
                    src[sl.start[j] + t] = tl.start[sdp_rows[j]] + t;
                    col[tl.start[sdp_rows[j]] + t] = sl.start[j] + t;
                }
            d_sub_rows = ar.array<RowOpts>(n_sdp);
            d_sub_idx = ar.array<int>(n_sdp);
            d_sub_src = ar.array<int>(sl.L);
            d_sdp_col = ar.array<int>(Lt);
            ar.upload(d_sub_rows, sub_rows.data(), sizeof(RowOpts) * n_sdp, stream_);
            ar.upload(d_sub_idx, sdp_rows.data(), sizeof(int) * n_sdp, stream_);
            ar.upload(d_sub_src, src.data(), sizeof(int) * sl.L, stream_);
            ar.upload(d_sdp_col, col.data(), sizeof(int) * Lt, stream_);
        }
    }

    // Device-resident features without an assist text: bert_proj is a 1x1 product, so it commutes with the word2ph column gather.  It runs over
    // DeBERTa's own token columns and the gather then moves H rows; the [bert_dim x Lt] plane is never built (see the TextEncoder block).
    const bool proj_first = !b.bert_host && b.bert_dev && b.assist_n == 0;
    Plane bert = proj_first ? Plane() : ar.plane(cfg_.bert_dim, Lt);
    Plane BP = ar.plane(H, Lt);   // bert_proj's output on the text layout
    int* d_map = nullptr;         // [Lt] DeBERTa's column behind each text column, -1 for none (device-resident features)
    if (b.bert_host) {
        fill_zero(bert.p, sizeof(float) * (size_t)bert.C * bert.ld, stream_);
        HIP_CHECK(hipStreamSynchronize(stream_));
        int64_t off = 0;
        for (int u = 0; u < n; ++u) {
            HIP_CHECK(hipMemcpy2D(bert.p + tl.start[u], sizeof(float) * bert.ld, b.bert_host + off, sizeof(float) * T[u],
                                  sizeof(float) * T[u], cfg_.bert_dim, hipMemcpyHostToDevice));
            off += (int64_t)cfg_.bert_dim * T[u];
        }
    } else {
        SBV2_REQUIRE(b.bert_dev && b.bert_map, "no BERT features given");
        std::vector<int> map(Lt, -1);
        int64_t e = 0;
        for (int u = 0; u < n; ++u)
            for (int t = 0; t < T[u]; ++t, ++e) {
                SBV2_REQUIRE(b.bert_map[e] < b.bert_dev->L, "internal: feature map outside the feature plane");
                map[tl.start[u] + t] = b.bert_map[e];
            }
        d_map = ar.array<int>(Lt);
        ar.upload(d_map, map.data(), sizeof(int) * Lt, stream_);
        if (b.assist_n > 0) {
            // assist text: every sequence's mean over its own columns, then the gather with the rows' blends (assist.hip)
            SBV2_REQUIRE(b.assist_start && b.assist_len && b.assist_rows, "internal: assist tables missing");
            const int A = b.assist_n;
            for (int a = 0; a < A; ++a)
                SBV2_REQUIRE(b.assist_len[a] >= 1 && b.assist_start[a] >= 0 && b.assist_start[a] + b.assist_len[a] <= b.bert_dev->L,
                             "internal: assist sequence outside the feature plane");
            for (int u = 0; u < n; ++u) SBV2_REQUIRE(b.assist_rows[u].mean_row < A, "internal: assist row outside the table");
            int* d_as = ar.array<int>(A);
            int* d_al = ar.array<int>(A);
            AssistRow* d_ar = ar.array<AssistRow>(n);
            float* d_mean = ar.array<float>((size_t)A * cfg_.bert_dim);
            ar.upload(d_as, b.assist_start, sizeof(int) * A, stream_);
            ar.upload(d_al, b.assist_len, sizeof(int) * A, stream_);
            ar.upload(d_ar, b.assist_rows, sizeof(AssistRow) * n, stream_);
            assist_mean(*b.bert_dev, d_as, d_al, A, d_mean, stream_);
            gather_cols_assist(*b.bert_dev, d_map, tl.d_seg_of, d_ar, d_mean, bert, stream_);
        }
    }

    // ---- per-utterance vectors: g = emb_g(sid) and every Linear / 1x1 conv applied to it ---------------
    float* G = ar.array<float>((size_t)n * cfg_.gin);
    gather_rows(emb_g_, cfg_.gin, d_sid, G, n, stream_);
    auto gvec = [&](const float* w, const float* bias, int M) {
        float* out = ar.array<float>((size_t)n * M);
        linear_vec(w, bias, M, cfg_.gin, G, cfg_.gin, out, M, n, stream_);
        return out;
    };
    float* v_style = ar.array<float>((size_t)n * H);
    linear_vec(style_w_, style_b_, H, cfg_.style_dim, d_style, cfg_.style_dim, v_style, H, n, stream_);
    float* v_encp = gvec(enc_p_.spk_w, enc_p_.spk_b, H);
    float* v_dp = gvec(dp_cond_w_, dp_cond_b_, H);
    float* v_sdp = n_sdp > 0 ? gvec(sdp_cond_w_, sdp_cond_b_, H) : nullptr;
    if (sdp_sub) {   // the sub-layout's segments are numbered 0 .. n_sdp - 1: its rows' vectors, compacted
        float* v_sub = ar.array<float>((size_t)n_sdp * H);
        gather_rows(v_sdp, H, d_sub_idx, v_sub, n_sdp, stream_);
        v_sdp = v_sub;
    }
    dec_cond_vec_ = gvec(dec_cond_w_, dec_cond_b_, cfg_.up_initial);
    std::vector<float*> v_flow;
    for (auto& c : flows_) v_flow.push_back(gvec(c.enc.spk_w, c.enc.spk_b, H));

    // ---- TextEncoder ----------------------------------------------------------------------------------
    std::unique_ptr<TraceRange> tr(new TraceRange("text_encoder"));
    if (proj_first) {
        // Same bits as gather-then-project: the exact-f32 product is one fma chain per column whatever the launch shape, the bias is per row, and
        // a column with no source gets 0 + bias, what the product gave the gather's zero column.
        SBV2_REQUIRE(b.bert_dev->C >= cfg_.bert_dim, "internal: feature plane narrower than bert_dim");
        Plane P = ar.plane(H, b.bert_dev->L);
        conv_plain(bert_proj_, b.bert_dev->rows(0, cfg_.bert_dim), P, 1, 0, nullptr, 1, stream_);
        gather_cols(P, d_map, BP, stream_, bert_proj_.bias);
    } else {
        conv_plain(bert_proj_, bert, BP, 1, 0, nullptr, 1, stream_);
    }
    Plane X = ar.plane(H, Lt);
    text_embed(d_ph, d_tn, d_lg, tl.d_seg_of, emb_, tone_emb_, lang_emb_, BP.p, BP.ld, v_style, H, std::sqrt((float)H), X, stream_);
    trace("x_emb", X, tl);
    run_encoder(enc_p_, X, tl, v_encp, ar);
    trace("x", X, tl);
    Plane ST = ar.plane(2 * I, Lt);
    conv_plain(enc_proj_, X, ST, 1, 0, tl.d_mask, 1, stream_);
    Plane m_p = ST.rows(0, I), logs_p = ST.rows(I, I);
    trace("stats", ST, tl);

    // ---- DurationPredictor -----------------------------------------------------------------------------
    tr.reset();
    tr.reset(new TraceRange("durations"));
    Plane XD = ar.plane(H, Lt);
    add_segvec(XD, v_dp, H, tl.d_seg_of, 1, tl.d_mask, stream_, &X);   // XD = X + v_dp, out of place: no copy of X first
    Plane D1 = ar.plane(cfg_.dp_filter, Lt), D2 = ar.plane(cfg_.dp_filter, Lt), DPO = ar.plane(1, Lt);
    conv_plain(dp_c1_, XD, D1, 1, cfg_.dp_kernel / 2, tl.d_mask, 1, stream_, ACT_RELU);
    layernorm_ch(D1, D1, dp_n1g_, dp_n1b_, 1e-5f, ACT_NONE, nullptr, 0, tl.d_mask, stream_);
    conv_plain(dp_c2_, D1, D2, 1, cfg_.dp_kernel / 2, tl.d_mask, 1, stream_, ACT_RELU);
    layernorm_ch(D2, D2, dp_n2g_, dp_n2b_, 1e-5f, ACT_NONE, nullptr, 0, tl.d_mask, stream_);
    conv_plain(dp_proj_, D2, DPO, 1, 0, tl.d_mask, 1, stream_);

    // ---- StochasticDurationPredictor, reverse: only for the rows whose sdp_ratio is not 0 (decided above).  The exported graph runs it for every row
    // and multiplies by the ratio; no row at a non-zero ratio is the default of every server path, and then nothing of it is launched or allocated. ----
    // Every kernel of the chain is column-local or segment-local (the exact-f32 products are one fma chain per column whatever the launch shape,
    // the depthwise convolutions see their own segment and the zero gap), so a row gets the same bits on sl as on tl.  LayerNorm is per column too, but
    // its kernels differ in the order of the per-column sums and are chosen by column count: on sl they are chosen for Lt columns, as on tl.
    float* z0 = nullptr;   // the predictor's output row, on sl when sdp_sub, else on tl; null: no row uses it
    if (n_sdp > 0) {
        const SegLayout& pl = sdp_sub ? sl : tl;
        const int Lp = pl.L;
        Plane XS = X;
        if (sdp_sub) {
            XS = ar.plane(H, Lp);
            gather_cols(X, d_sub_src, XS, stream_);
        }
        Plane XSd = ar.plane(H, Lp), COND = ar.plane(H, Lp), HH = ar.plane(H, Lp);
        Plane PR = ar.plane(3 * cfg_.sdp_bins - 1, Lp), Z = ar.plane(2, Lp);
        conv_plain(sdp_pre_, XS, XSd, 1, 0, nullptr, 1, stream_);
        add_segvec(XSd, v_sdp, H, pl.d_seg_of, 1, pl.d_mask, stream_);
        run_dds(sdp_dds_, XSd, pl, ar, Lt);
        conv_plain(sdp_proj_, XSd, COND, 1, 0, pl.d_mask, 1, stream_);
        z0 = Z.p;
        float* z1 = Z.p + Z.ld;
        noise_fill(Z.p, Z.ld, 2, pl.d_seg_of, pl.d_start, pl.d_len, sdp_sub ? d_sub_rows : d_rows, Lp, 0, stream_);
        const float inv_sqrt_f = 1.0f / std::sqrt((float)H);
        for (int i = (int)sdp_cf_.size() - 1; i >= 0; --i) {
            const ConvFlow& cf = sdp_cf_[i];
            swap_rows(z0, z1, Lp, stream_);  // Flip
            convflow_pre(z0, cf.pre_w, cf.pre_b, COND, HH, pl.d_mask, stream_);
            run_dds(cf.dds, HH, pl, ar, Lt);
            conv_plain(cf.proj, HH, PR, 1, 0, pl.d_mask, 1, stream_);
            spline_inverse(PR, z0, z1, cfg_.sdp_bins, cfg_.sdp_tail, inv_sqrt_f, pl.d_mask, Lp, stream_);
        }
        swap_rows(z0, z1, Lp, stream_);
        affine_reverse(z0, z1, sdp_ea_m_, sdp_ea_logs_, sdp_ea_scale_, pl.d_mask, Lp, stream_);
    }

    // ---- durations (the one device -> host sync of the batch: T_frames is data dependent) ----------------
    float* d_logw = ar.array<float>(Lt);
    int* d_dur = ar.array<int>(Lt);
    sbv2::durations(z0, DPO.p, tl.d_seg_of, d_rows, tl.d_mask, Lt, d_logw, d_dur, stream_, sdp_sub ? d_sdp_col : nullptr);
    std::vector<int> dur_p(Lt);
    std::vector<float> logw_p(Lt);
    HIP_CHECK(hipMemcpyAsync(dur_p.data(), d_dur, sizeof(int) * Lt, hipMemcpyDeviceToHost, stream_));
    HIP_CHECK(hipMemcpyAsync(logw_p.data(), d_logw, sizeof(float) * Lt, hipMemcpyDeviceToHost, stream_));
    // (the f16x3 clamp count of everything queued so far: DeBERTa's products when a pipeline run feeds this call on the same device, the previous call's
    // flow; the one host sync of the batch is here anyway)
    sat_watch_.enqueue(stream_);
    HIP_CHECK(hipStreamSynchronize(stream_));
    sat_watch_.check("DeBERTa / flow products seen by the VITS call");
    dur_host_.assign((size_t)total_t, 0);
    logw_host_.assign((size_t)total_t, 0.f);
    std::vector<int> Tf(n);
    std::vector<std::vector<int>> used(n);
    used_host_.assign((size_t)total_t, 0);
    used_offs_.assign((size_t)n + 1, 0);
    {
        int64_t e = 0;
        for (int u = 0; u < n; ++u) {
            int64_t sum = 0;
            used[u].resize(T[u]);
            used_offs_[u + 1] = used_offs_[u] + T[u];
            for (int t = 0; t < T[u]; ++t, ++e) {
                dur_host_[e] = dur_p[tl.start[u] + t];
                logw_host_[e] = logw_p[tl.start[u] + t];
                const int64_t dv = b.forced_durations ? b.forced_durations[e] : dur_host_[e];
                SBV2_REQUIRE(dv >= 0 && dv < (1 << 20), "duration out of range");
                used[u][t] = (int)dv;
                used_host_[e] = dv;
                sum += dv;
            }
            SBV2_REQUIRE(sum < (1 << 24), "utterance too long");
            Tf[u] = (int)std::max<int64_t>(sum, 1);  // torch.clamp_min(sum, 1)
        }
    }
    // (frame count rounded to 32: every plane of the decoder's wide stages - 8 and 64 positions per frame - is then a whole number of conv_clx's 256-position
    // tiles, and the kernel instance without the guarded last-tile epilogue applies)
    ar.begin_uploads();   // the layout's four arrays and the token map: neighbours, one copy
    fl_ = make_layout(Tf, kFrameGap, ar, stream_, nullptr, 32);
    const SegLayout& fl = fl_;
    const int Lf = fl.L;
    std::vector<int> tok(Lf, -1);
    for (int u = 0; u < n; ++u) {
        int y = fl.start[u];
        for (int t = 0; t < T[u]; ++t)
            for (int q = 0; q < used[u][t]; ++q) tok[y++] = tl.start[u] + t;
    }
    int* d_tok = ar.array<int>(Lf);
    ar.upload(d_tok, tok.data(), sizeof(int) * Lf, stream_);
    ar.end_uploads();

    // ---- alignment expansion + prior sample ---------------------------------------------------------------
    tr.reset();
    tr.reset(new TraceRange("flow"));
    Plane ZA = ar.plane(I, Lf), ZB = ar.plane(I, Lf);
    expand_frames(m_p, logs_p, d_tok, fl.d_seg_of, fl.d_start, fl.d_len, d_rows, ZA, stream_);
    trace("z_p", ZA, fl);

    // ---- TransformerCouplingBlock, reverse ----------------------------------------------------------------
    const int half = I / 2;
    Plane Hf = ar.plane(H, Lf);
    for (int i = cfg_.flow_n - 1; i >= 0; --i) {
        const Coupling& c = flows_[i];
        flip_channels(ZA, ZB, stream_);
        std::swap(ZA, ZB);
        conv_plain(c.pre, ZA.rows(0, half), Hf, 1, 0, fl.d_mask, 1, stream_);
        run_encoder(c.enc, Hf, fl, v_flow[i], ar);
        Plane x1 = ZA.rows(half, half);
        conv_plain(c.post, Hf, x1, 1, 0, fl.d_mask, 1, stream_, ACT_NONE, 1.0f, &x1, -1.0f);  // x1 = (x1 - m) * mask
    }
    trace("z", ZA, fl);
    tr.reset();
    z_ = ZA;
    if (b.skip_decoder) {   // streaming: the caller decodes chunk by chunk (stream_begin / stream_next)
        pcm_ = nullptr;
        pcm_total_ = 0;
        pcm_lens_.assign(n, 0);
        pcm_offs_.assign(n, 0);
        return;
    }
    TraceRange td("decoder");
    if (dec_mode_) run_decoder_cl(ar, ZA, fl, dec_cond_vec_);
    else run_decoder(ar, ZA, fl, dec_cond_vec_);
    log_line("vits forward: " + std::to_string(n) + " utterance(s), " + std::to_string(Lt) + " text columns, " + std::to_string(Lf) + " frame columns");
}

// ---- streaming long-form decode ---------------------------------------------------------------------------------------------------
// The generator is purely convolutional: frames [f0, f0 + chunk) depend on z[f0 - 13.4, f0 + chunk + 13.4) only, so a window with a
// 16-frame halo on both sides reproduces the whole-sequence result on its centre.  The window's column mask marks which of its frames
// exist (the sequence ends are zero padding at EVERY layer, exactly like the gaps of a packed batch), interior window edges only
// contaminate the halo, which is discarded.  The window shape is fixed, so the ~90 launches of the decoder are captured once into a
// hipGraph and replayed per chunk; all device pointers of the captured launches live in the plan's own arena.
// Receptive field of the generator per side, in frames: conv_pre + per stage {transposed-conv taps at the input rate, the widest MRF branch
// sum_d (d + 1)(k - 1) / 2 at the output rate} + conv_post; + 1 frame of margin, rounded up to a multiple of 4.
double VitsModel::stream_receptive_field() const {
    double rf = (dec_pre_.k - 1) / 2.0;
    double rate = 1.0;
    for (size_t i = 0; i < stages_.size(); ++i) {
        int tmax = 0;
        for (const auto& g : stages_[i].up.groups)
            for (int t = 0; t < g.ntaps; ++t) tmax = std::max(tmax, std::abs(g.shift[t]));
        rf += tmax / rate;
        rate *= stages_[i].rate;
        int mrf = 0;
        for (const auto& rb : stages_[i].branches) {
            int h = 0;
            for (int d : rb.dil) h += (d + 1) * (rb.k - 1) / 2;
            mrf = std::max(mrf, h);
        }
        rf += mrf / rate;
    }
    rf += (dec_post_k_ - 1) / 2.0 / rate;
    return rf;
}
int VitsModel::stream_halo() const { return round_up((int)std::ceil(stream_receptive_field()) + 1, 4); }

// A decode plan = nwin windows of chunk + 2 * halo frames packed into one batch (the packed-batch layout: the gaps between the windows are
// the zero padding of every convolution), its persistent input / conditioning buffers, its own arena and the graph captured for that shape.
// chunk_ (one window) decodes the first chunk of an utterance: time to first PCM; burst_ (kStreamBurst windows per replay) every later
// one: a 288-frame window is ~90 launches of mostly < 100 workgroups, i.e. launch-latency bound, and four windows per replay cost little
// more than one (profiles/r03_longform_*.json).
void VitsModel::ensure_plan(std::shared_ptr<ChunkPlan>& slot, int chunk_frames, int nwin) {
    static const bool no_graph = getenv("SBV2_STREAM_GRAPH") && atoi(getenv("SBV2_STREAM_GRAPH")) == 0;   // A/B knob
    if (!slot || slot->chunk != chunk_frames || slot->nwin != nwin) {
        slot.reset(new ChunkPlan);
        ChunkPlan& c = *slot;
        c.chunk = chunk_frames;
        c.nwin = nwin;
        c.W = chunk_frames + 2 * stream_halo();
        c.lay = make_layout(std::vector<int>(nwin, c.W), kFrameGap, c.ar, stream_);
        c.zin = c.ar.plane(cfg_.inter, c.lay.L);
        fill_zero(c.zin.p, sizeof(float) * (size_t)c.zin.C * c.zin.ld, stream_);
        c.cond = c.ar.array<float>((size_t)cfg_.up_initial * nwin);
        fill_zero(c.cond, sizeof(float) * (size_t)cfg_.up_initial * nwin, stream_);
        c.mark = c.ar.mark();
        for (int i = 0; i < 2; ++i) {
            HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&c.host[i]), sizeof(float) * (size_t)nwin * chunk_frames * cfg_.hop(), hipHostMallocDefault));
            c.host_bytes = sizeof(float) * (size_t)nwin * chunk_frames * cfg_.hop();
            HIP_CHECK(hipEventCreateWithFlags(&c.ev[i], hipEventDisableTiming));
        }
    }
    ChunkPlan& c = *slot;
    // (the conditioning vectors of the windows' rows reach c.cond with every replay's stream_windows launch: the captured launches read them there;
    // the warm-up and the capture below run on whatever the buffers hold, their output is never used)
    if (!c.exec && !no_graph) {
        // warm-up pass (sizes the arena: no hipMalloc may happen under capture), then the same launch sequence under capture
        auto decode = [&]() {
            c.ar.rewind(c.mark);
            if (dec_mode_) run_decoder_cl(c.ar, c.zin, c.lay, c.cond);
            else run_decoder(c.ar, c.zin, c.lay, c.cond);
            c.pcm = pcm_;
        };
        const bool tr = trace_;
        trace_ = false;
        decode();
        HIP_CHECK(hipStreamSynchronize(stream_));
        HIP_CHECK(hipStreamBeginCapture(stream_, hipStreamCaptureModeThreadLocal));
        try {
            decode();
        } catch (...) {
            hipGraph_t g = nullptr;
            (void)hipStreamEndCapture(stream_, &g);
            if (g) (void)hipGraphDestroy(g);
            trace_ = tr;
            throw;
        }
        HIP_CHECK(hipStreamEndCapture(stream_, &c.graph));
        HIP_CHECK(hipGraphInstantiate(&c.exec, c.graph, nullptr, nullptr, 0));
        trace_ = tr;
    }
    if (!c.exec) {   // eager path: the plan's pinned staging is recycled once per stream
        HIP_CHECK(hipStreamSynchronize(stream_));
        c.ar.reset_pinned();
    }
    c.slot_ci[0] = c.slot_ci[1] = -1;
}

// ---- the timeline of a stream over the n rows of one forward (sbv2_stream_timeline, include/sbv2_hip.h) ----
int64_t stream_min_gap(const PcmFmtSpec& spec) { return 2 * (((int64_t)spec.half + spec.L - 1) / spec.L); }

void stream_check_gaps(const int64_t* gap_after, int64_t n, const PcmFmtSpec& spec) {
    SBV2_REQUIRE(gap_after, "no gap_after given (one entry per row, the last one = trailing silence)");
    SBV2_REQUIRE(n >= 1, "a stream needs at least one row");
    const int64_t need = stream_min_gap(spec);
    for (int64_t i = 0; i < n; ++i) {
        SBV2_REQUIRE(gap_after[i] >= 0 && gap_after[i] <= kStreamMaxGap, "gap_after[" + std::to_string(i) + "] = " + std::to_string(gap_after[i]) +
                                                                              " is outside [0, " + std::to_string(kStreamMaxGap) + "] native samples");
        SBV2_REQUIRE(i == n - 1 || gap_after[i] >= need, "gap_after[" + std::to_string(i) + "] = " + std::to_string(gap_after[i]) +
                                                             " is below the minimum gap of " + std::to_string(need) + " native samples at " +
                                                             std::to_string(spec.rate) + " Hz (the resampling filter must not reach across a cut)");
    }
}

StreamTimeline stream_timeline(const int64_t* frames, const int64_t* gap_after, int64_t n, int hop, int64_t chunk_frames, const PcmFmtSpec& spec) {
    stream_check_gaps(gap_after, n, spec);
    SBV2_REQUIRE(frames && hop >= 1 && chunk_frames >= 1 && n < (1 << 20), "bad timeline arguments");
    StreamTimeline t;
    int64_t pos = 0;
    for (int64_t i = 0; i < n; ++i) {
        SBV2_REQUIRE(frames[i] >= 1 && frames[i] < (1 << 28), "row " + std::to_string(i) + " has " + std::to_string(frames[i]) + " frames");
        t.place.push_back(pos);
        t.len.push_back(frames[i] * hop);
        pos += frames[i] * hop + gap_after[i];
    }
    t.joined = pos;
    int64_t cut = 0;   // m_{i-1}: where the previous row's last call ended
    for (int64_t i = 0; i < n; ++i) {
        const int64_t end = i == n - 1 ? t.joined : t.place[i] + t.len[i] + gap_after[i] / 2;
        for (int64_t f0 = 0; f0 < frames[i]; f0 += chunk_frames) {
            const bool last = f0 + chunk_frames >= frames[i];
            const int64_t a = f0 == 0 ? cut : t.place[i] + f0 * hop, b = last ? end : t.place[i] + (f0 + chunk_frames) * hop;
            t.calls.push_back(StreamCall{(int)i, f0, pcm_format_out_len(spec, a), pcm_format_out_len(spec, b)});
        }
        cut = end;
    }
    return t;
}

std::vector<int64_t> stream_voice_upto(const StreamTimeline& t, int hop, int64_t chunk_frames, const PcmFmtSpec& spec, int64_t lookahead) {
    SBV2_REQUIRE(hop >= 1 && chunk_frames >= 1 && lookahead >= 0, "bad timeline arguments");
    std::vector<int64_t> upto;
    int64_t prev = 0;
    for (const StreamCall& k : t.calls) {
        const int64_t len = t.len[(size_t)k.row], S = std::min((k.f0 + chunk_frames) * (int64_t)hop, len);
        int64_t now = prev;
        if (S >= len) {
            now = k.j1;   // the row's last call: where it always ended
        } else if (S > lookahead) {
            // the outputs j whose newest tap, floor((j M + half) / L), lies below P = place + final: j M + half <= P L - 1
            const int64_t P = t.place[(size_t)k.row] + (S - lookahead), top = P * spec.L - 1 - spec.half;
            if (top >= 0) now = std::max(prev, std::min(top / spec.M + 1, k.j1));
        }
        upto.push_back(now);
        prev = now;
    }
    return upto;
}

int64_t VitsModel::stream_begin(int chunk_frames, const PcmFmtSpec* fmt, bool flac, const StreamLevelSpec* level, const int64_t* gap_after,
                                const StreamMarksSpec* marks, const StreamVoiceSpec* voice, const StreamLevelerSpec* leveler) {
    HIP_CHECK(hipSetDevice(device_));
    SBV2_REQUIRE(!leveler || level, "a stream leveler needs a level: its ceiling and its starting gain");
    SBV2_REQUIRE(fl_.n >= 1 && z_.p, "stream_begin needs a preceding forward with skip_decoder");
    SBV2_REQUIRE(gap_after || fl_.n == 1, "stream_begin without gaps needs a preceding forward of ONE utterance");
    SBV2_REQUIRE(!gap_after || fmt, "a stream over several rows is a formatted stream");
    SBV2_REQUIRE(chunk_frames >= 16 && chunk_frames <= (1 << 20), "chunk_frames must be in [16, 2^20]");
    sformatted_ = false;
    SBV2_REQUIRE(!marks || fmt, "levels and pitch on a stream need an output format: begin it with the identity format (44100 Hz f32) instead of none");
    SBV2_REQUIRE(!flac || (fmt && fmt->encoding == kEncS16), "a FLAC stream needs encoding = 1 (s16): f32 samples and G.711 codes have no FLAC form");
    SBV2_REQUIRE(!level || fmt, "a level stream needs an output format");
    if (fmt) SBV2_REQUIRE(!fmt->normalize, "a formatted stream cannot normalise: the peak of the utterance is not known ahead");
    if (fmt && !voice) {   // (a voice stream formats the shifted rows, whole on the device: no filter tap reads a window's halo)
        // the filter of an output sample at a chunk edge reaches ceil(half / L) native samples past the window centre; they must lie in the
        // part of the halo that the decoder computes exactly (halo minus the generator's receptive field)
        const int64_t reach = (fmt->half + fmt->L - 1) / fmt->L;
        const double exact = (stream_halo() - stream_receptive_field()) * cfg_.hop();
        SBV2_REQUIRE((double)reach <= exact, "the " + std::to_string(fmt->rate) + " Hz filter reaches " + std::to_string(reach) +
                                                 " samples past a chunk edge, the stream halo holds only " + std::to_string((int64_t)exact) + " exact samples");
    }
    // the global chunk list: every row cut on its own frame grid, the calls in row order then chunk order (a single utterance: one row, no gap)
    const int64_t no_gap = 0;
    const std::vector<int64_t> frames(fl_.len.begin(), fl_.len.end());
    stl_ = stream_timeline(frames.data(), gap_after ? gap_after : &no_gap, fl_.n, cfg_.hop(), chunk_frames, fmt ? *fmt : PcmFmtSpec());
    // (the envelope's and the contour's frame counts are refused here, before the stream has set up anything of its own)
    const int64_t A = fmt ? StreamOutput::check(*fmt, level, marks, stl_.joined) : 0;
    SBV2_REQUIRE(!voice || fmt, "a voice stream needs an output format: begin it with the identity format (44100 Hz f32) instead of none");
    SBV2_REQUIRE(!voice || (int64_t)voice->pivot.size() == fl_.n, "a voice stream needs one pivot per row");
    svoice_upto_.clear();
    if (voice) svoice_upto_ = stream_voice_upto(stl_, cfg_.hop(), chunk_frames, *fmt, voice->lookahead);
    constexpr int burst = kStreamBurst;   // (1 / 2 / 4 / 8 / 12 / 16 windows per replay measured in round 3: 2.62 / 1.88 / 1.64 / 1.41 / 1.39 / 1.47 ms per chunk)
    static_assert(kStreamBurst <= kStreamWinMax, "a replay's window table holds kStreamWinMax windows");
    const int64_t ncalls = (int64_t)stl_.calls.size();
    ensure_plan(chunk_, chunk_frames, 1);
    const bool want_burst = burst > 1 && ncalls > 1;   // a request of one chunk never needs it
    if (want_burst) {
        // windows per replay: no more than the chunks that follow the first one (a 2-chunk utterance does not decode 7 all-zero windows, nor pay
        // their workspace: 256 MiB per window at 256-frame chunks), from {2, 4, 8, 16} so that utterances of different lengths share few captures;
        // a larger plan of the same chunk size that this handle already holds is reused as it is
        const int64_t rest = ncalls - 1;
        int nw = 2;
        while (nw < burst && nw < rest) nw *= 2;
        nw = std::min(nw, burst);
        if (burst_ && burst_->chunk == chunk_frames && burst_->nwin >= nw) nw = burst_->nwin;
        ensure_plan(burst_, chunk_frames, nw);
    }
    stream_bursts_ = want_burst;
    if (fmt) {   // pinned slots and the device output sized from the timeline: the largest replay of each plan, gaps included (+ A with a level)
        int64_t cap = 0;
        for (ChunkPlan* c : {chunk_.get(), want_burst ? burst_.get() : nullptr}) {
            if (!c) continue;
            const bool is_burst = want_burst && c == burst_.get();   // (with bursts the single-window plan decodes call 0 only)
            int64_t most = 0;
            for (int64_t c0 = is_burst ? 1 : 0; c0 < (want_burst && !is_burst ? 1 : ncalls); c0 += c->nwin) {
                const int64_t ce = std::min<int64_t>(c0 + c->nwin, ncalls) - 1;
                if (voice) most = std::max(most, svoice_upto_[(size_t)ce] - (c0 ? svoice_upto_[(size_t)(c0 - 1)] : 0));   // (what the replay delivers)
                else most = std::max(most, stl_.calls[ce].j1 - stl_.calls[c0].j0);
            }
            c->fmt_cap = most + A;
            const size_t need = StreamOutput::slot_bytes(*fmt, flac, c->fmt_cap);
            cap = std::max(cap, c->fmt_cap);
            if (need > c->host_bytes) {
                HIP_CHECK(hipStreamSynchronize(stream_));
                for (int i = 0; i < 2; ++i) {
                    HIP_CHECK(hipHostFree(c->host[i]));
                    c->host[i] = nullptr;
                }
                c->host_bytes = 0;
                for (int i = 0; i < 2; ++i) HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&c->host[i]), need, hipHostMallocDefault));
                c->host_bytes = need;
            }
        }
        if (!sout_) sout_ = std::make_shared<StreamOutput>();
        sout_->begin(*fmt, flac, level, marks, used_host_, used_offs_, stl_.place.data(), cfg_.hop(), stl_.joined, cap, stream_, leveler);
        if (voice) sout_->begin_voice(*voice, stl_.place, stl_.len, svoice_upto_, stream_);
        sformatted_ = true;
    }
    stream_enqueue(*chunk_, 0, 0);                 // the first chunk starts right behind the flow ...
    if (want_burst) stream_enqueue(*burst_, 1, 0); // ... and the first burst right behind it
    return ncalls;
}

// windows + decoder (graph replay) + device -> pinned-host copies of the windows' centres, all asynchronous on the model's stream.
// The plan's windows are the calls c0, c0 + 1, ... of the global chunk list, whatever rows they belong to (windows past the end of the
// request decode zeros and are not copied).
void VitsModel::stream_enqueue(ChunkPlan& c, int64_t c0, int slot) {
    const int hop = cfg_.hop(), halo = stream_halo();
    const int64_t ncalls = (int64_t)stl_.calls.size();
    const int live = (int)std::min<int64_t>(c.nwin, ncalls - c0);
    // window w = frames [f0 - halo, f0 - halo + W) of its call's row (fl_.start[row] is the row's first column in the packed plane); ONE launch
    // writes every window's z columns, column mask and conditioning vector, from a table passed by value
    StreamWinTable tab{};
    for (int w = 0; w < live; ++w) {
        const StreamCall& k = stl_.calls[c0 + w];
        tab.w[w] = StreamWin{fl_.start[k.row], fl_.len[k.row], (int)(k.f0 - halo), k.row};
    }
    SBV2_REQUIRE((int)c.lay.start.size() >= c.nwin, "stream plan: fewer windows in the layout than in the plan");
    stream_windows(z_, tab, c.nwin, c.W, c.lay.d_start, c.lay.start.data(), c.zin, c.lay.d_mask, dec_cond_vec_, cfg_.up_initial, c.cond, stream_);
    if (c.exec) {
        HIP_CHECK(hipGraphLaunch(c.exec, stream_));
    } else {
        c.ar.rewind(c.mark);
        if (dec_mode_) run_decoder_cl(c.ar, c.zin, c.lay, c.cond);
        else run_decoder(c.ar, c.zin, c.lay, c.cond);
        c.pcm = pcm_;
    }
    if (sformatted_) {
        // ONE formatting launch over the replay's windows: window w holds native samples [(f0 - halo) hop, (f0 - halo + W) hop) of its row, which
        // lies at place[row] of the joined timeline; the piece is that PCM clipped to the row (the decoder's output outside a row is not silence);
        // the call emits the output samples [j0, j1) of the timeline (stream_timeline: its chunk, and with a row's first / last chunk the half gaps)
        std::vector<FmtPiece> pieces;
        std::vector<FmtSignal> sig;
        int64_t total = 0;
        for (int w = 0; w < live; ++w) {
            const StreamCall& k = stl_.calls[c0 + w];
            const int64_t r0 = stl_.place[k.row], r1 = r0 + stl_.len[k.row];
            const int64_t ws = r0 + (k.f0 - halo) * hop, lo = std::max<int64_t>(r0, ws), hi = std::min<int64_t>(r1, ws + (int64_t)c.W * hop);
            pieces.push_back(FmtPiece{c.pcm + (size_t)w * c.W * hop + (lo - ws), lo, hi - lo});
            sig.push_back(FmtSignal{k.j0, k.j1, total, w, w + 1});
            total += k.j1 - k.j0;
        }
        // a voice stream: the shifter is fed every window's central samples clipped to the row, the samples the fetch's packed PCM holds
        std::vector<StreamVoiceFeed> feed;
        if (sout_->voice())
            for (int w = 0; w < live; ++w) {
                const StreamCall& k = stl_.calls[c0 + w];
                const int64_t s0 = k.f0 * hop, s1 = std::min<int64_t>((k.f0 + c.chunk) * hop, stl_.len[k.row]);
                feed.push_back(StreamVoiceFeed{k.row, s0, s1, c.pcm + ((size_t)w * c.W + halo) * hop});
            }
        // ... and everything behind it, sink included (StreamOutput::push); the formatter's table slots: 0 / 1 = chunk_'s, 2 / 3 = burst_'s
        sout_->push(pieces, sig, total, c0 + c.nwin >= ncalls, (&c == burst_.get() ? 2 : 0) + slot, c.host[slot], c.fmt_cap, c.out[slot], stream_,
                    sout_->voice() ? &feed : nullptr, c0);
    } else {
        for (int w = 0; w < live; ++w) {   // a plain stream: one row at place 0, the windows' centres as they are
            const StreamCall& k = stl_.calls[c0 + w];
            HIP_CHECK(hipMemcpyAsync(c.host[slot] + (size_t)w * c.chunk * hop, c.pcm + ((size_t)w * c.W + halo) * hop, sizeof(float) * (size_t)(k.j1 - k.j0),
                                     hipMemcpyDeviceToHost, stream_));
        }
    }
    HIP_CHECK(hipEventRecord(c.ev[slot], stream_));
    c.slot_ci[slot] = c0;
}

int64_t VitsModel::stream_call_bound() const {
    int64_t most = 0;
    for (const StreamCall& k : stl_.calls) most = std::max(most, k.j1 - k.j0);
    for (size_t c = 0; c < svoice_upto_.size(); ++c)   // (a voice stream: a row's last call also delivers what the look-ahead held back)
        most = std::max(most, svoice_upto_[c] - (c ? svoice_upto_[c - 1] : 0));
    return sformatted_ ? sout_->call_bound(most) : most * (int64_t)sizeof(float);
}

StreamOutput::Taken VitsModel::stream_next(int64_t ci, void* dst, int64_t capacity_bytes) {
    HIP_CHECK(hipSetDevice(device_));
    const int64_t ncalls = (int64_t)stl_.calls.size();
    SBV2_REQUIRE(chunk_ && z_.p && ncalls > 0, "stream_chunk without stream_begin");
    SBV2_REQUIRE(ci >= 0 && ci < ncalls, "chunk out of range");
    const int64_t nsamp = stl_.calls[ci].j1 - stl_.calls[ci].j0, nbytes = nsamp * (int64_t)sizeof(float);
    SBV2_REQUIRE(sformatted_ || capacity_bytes >= nbytes, "PCM buffer too small for the chunk");
    // The replay that holds call ci: window w of the replay of calls c0 .. on plan c.  The single-window plan has the request's first chunk
    // (and everything when bursts are off) and runs the next chunk while this one is delivered; the burst plan has every later chunk and
    // decodes the following burst while the first window of this one is delivered (that burst's slot was drained one burst ago).
    const bool bursts = stream_bursts_ && burst_ && burst_->chunk == chunk_->chunk;
    const bool single = ci == 0 || !bursts;
    ChunkPlan& c = single ? *chunk_ : *burst_;
    const int64_t w = single ? 0 : (ci - 1) % c.nwin, c0 = ci - w, next = c0 + c.nwin;
    const int slot = (int)((c0 / c.nwin) & 1);
    if (c.slot_ci[slot] != c0) {   // random access, not the streaming order: refused where anything is carried from replay to replay
        const char* carried = sformatted_ ? sout_->ordered() : nullptr;
        SBV2_REQUIRE(!carried, carried);
        stream_enqueue(c, c0, slot);
    }
    if ((single ? !bursts : w == 0) && next < ncalls && c.slot_ci[slot ^ 1] != next) stream_enqueue(c, next, slot ^ 1);
    HIP_CHECK(hipEventSynchronize(c.ev[slot]));
    StreamOutput::Taken t{nsamp, nbytes, nsamp};
    if (sformatted_) t = sout_->deliver(c.out[slot], w, ci, dst, capacity_bytes);
    else std::memcpy(dst, c.host[slot] + (size_t)w * c.chunk * cfg_.hop(), (size_t)nbytes);
    if (single) c.slot_ci[slot] = -1;
    return t;
}

void VitsModel::copy_pcm(float* host) {
    HIP_CHECK(hipSetDevice(device_));
    HIP_CHECK(hipMemcpyAsync(host, pcm_, sizeof(float) * (size_t)pcm_total_, hipMemcpyDeviceToHost, stream_));
    HIP_CHECK(hipStreamSynchronize(stream_));
}

}  // namespace sbv2
