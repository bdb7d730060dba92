// Host-side model objects behind the C ABI: weights resident in HBM, per-call workspace arena,
// batched forward passes expressed as sequences of kernel launches on one HIP stream.
#pragma once
#include "common.h"
#include "flac_encode.h"
#include "limiter.h"
#include "marks.h"
#include "ops.h"
#include "pcm_format.h"
#include "stream_output.h"

#include <memory>

namespace sbv2 {

// A convolution packed for conv_cl.hip (bf16 MFMA fragment blocks); parts = 2 keeps a bf16 hi and a bf16 lo copy.
struct ClConv {
    void* w = nullptr;
    void* wxp = nullptr;   // split-bf16, M == K in {32, 64}: the same weights as step-pair fragments of the 16x16x32 MFMA (pack_step_pairs; respair_x16.hip), else null
    void* wx = nullptr;    // split-bf16, M % 64 == 0, K % 32 == 0: the same weights as [hi | lo] fragments of the 16x16x32 MFMA (pack_clx16; conv_clx.hip), else null
    void* wp = nullptr;    // 16 x 16 convolutions of the fused ResBlock step: tap-pair fragments [pair][part][64 lanes][8] (pack_cl_pairs), else null
    float* bias = nullptr;
    int M = 0, K = 0, k = 1, nmt = 0, tm = 1, parts = 0;
};

// Weights in the layout gemm_conv expects: [tap][Cin][lda] (k-major, Cout contiguous), plus (optionally) the bf16 fragment
// packing of the same weights: when `cl.parts != 0` conv_plain / linear_tokmajor run on the bf16 matrix cores.
struct PackedConv {
    float* w = nullptr;
    float* bias = nullptr;
    int cout = 0, cin = 0, k = 1, lda = 0;
    ClConv cl;
    BfsWeights bfs;   // 1x1 products only: pre-split bf16 fragments for gemm_bfs.hip (parts = 0: not packed)
    int64_t tap_stride() const { return (int64_t)cin * lda; }
};
// One ConvTranspose1d split into groups of output phases that share the same input taps.
struct PackedUpsample {
    struct Grp {
        float* w = nullptr;
        int lda = 0, ntaps = 0, nph = 0;
        int shift[kMaxTaps];
        int phase_off[kMaxPhases];
    };
    std::vector<Grp> groups;
    float* bias = nullptr;
    int cin = 0, cout = 0, stride = 1;
};

// Packed segments along the time axis: utterance i occupies columns [start[i], start[i]+len[i]); every start is a
// multiple of 4 and at least `gap` zero columns separate neighbours (the zero padding of every 'same' convolution).
struct SegLayout {
    int n = 0, L = 0;
    std::vector<int> start, len;
    int* d_seg_of = nullptr;
    unsigned char* d_mask = nullptr;
    int* d_start = nullptr;
    int* d_len = nullptr;
    int max_len() const {
        int m = 0;
        for (int v : len) m = std::max(m, v);
        return m;
    }
};
SegLayout make_layout(const std::vector<int>& lens, int gap, Arena& arena, hipStream_t stream, const unsigned char* extra_mask = nullptr, int round_to = 4);

class WeightStore;
// w is [M][K][k] (Conv1d layout); K is zero-padded to a multiple of 16
ClConv pack_cl(WeightStore& ws, const float* w, int M, int K, int k, int parts, const float* bias);
void* pack_clx16(WeightStore& ws, const float* w, int M, int K, int k);
// A ConvTranspose1d (weight [cin][cout][k], stride s, padding (k - s) / 2) as ONE phased product for conv_clx.hip (round 6): rows (phase, cout), taps = the
// union of the phases' input taps (zero weights where a phase has none; 2 .. 5 taps); tap t
// reads input position n + shift0 - t.  wx == nullptr: the shape does not fit (decoder_cl.cpp falls back to conv_cl.hip's phase groups).
struct ClUpX {
    void* wx = nullptr;
    float* bias = nullptr;      // per row (phase, cout)
    int M = 0, K = 0, ntaps = 0, shift0 = 0, nph = 0, cout = 0;
    int group = 1;              // ConvClxParams::phase_group of the row order the weights and the bias were packed in
    double alg_macs_per_pos = 0;   // multiply-adds per input position that are not padding (the launch's algorithmic FLOP for the profile)
    int phase_off[kMaxPhases] = {0};
    int phase_tap0[kMaxPhases] = {0};   // ConvClxParams::phase_tap0: where each phase's own taps start in the union of all phases' taps
};
ClUpX build_upx(WeightStore& ws, const float* wt, const float* ub, int cin, int cout, int k, int s, bool parts_out);
void* pack_step_pairs(WeightStore& ws, const float* w, int C, int k);   // w [C][C][k], C in {32, 64} -> step-pair fragments (split-bf16) for respair_x16.hip
void* pack_cl_pairs(WeightStore& ws, const float* w, int k);   // w [16][16][k] -> tap-pair fragments (split-bf16) for respair_clx's 16-channel kernel
// One convolution of the channels-last decoder in decoder arithmetic `mode` (1 = bf16x3, 2 = bf16, 3 = f16): pack_cl, plus pack_cl_pairs for a 16 x 16 split-bf16 conv
ClConv pack_decoder_conv(WeightStore& ws, const float* w, int M, int K, int k, int mode, const float* bias);
// The decoder's launch parameters (decoder_cl.cpp), shared with the test hooks.  A conv_cl launch of c: tap t reads position n + t * dil - pad_l
ConvClParams conv_cl_params(const ClConv& c, const float* X, int ldx, int NB, float* Y, int ldy, int N, int dil, int pad_l, const unsigned char* mask,
                            int mask_div, float pre_slope, const float* R, int ldr, float beta, int accumulate);
// The operands of one fused ResBlock step (respair_*.hip); X, Y, beta and accumulate are the caller's
ResPairParams step_params(const ClConv& c1, const ClConv& c2, int k, int dil, int mode, int C, int64_t N, const unsigned char* mask, int U, int ushift);
// The operands of a fused ResBlock branch (resbranch_clx.hip); X, Y, beta and accumulate are the caller's
ResBranchParams branch_params(const std::vector<ClConv>& c1, const std::vector<ClConv>& c2, const std::vector<int>& dil, int k, int C, int64_t N,
                              const unsigned char* mask, int mask_shift);
// The two conv_clx launches of one ResBlock step of the wide stages (run_decoder_cl's clx_steps arm): conv1 reads the parts X of lrelu(y) and writes ONLY the
// parts T of lrelu(its result); conv2 reads T, adds the residual plane R = y and writes the f32 plane Y and, when Ys is given, the parts of lrelu(Y)
ConvClxParams clx_conv1_params(const ClConv& c1, const SplitClPlanes& X, const SplitClPlanes& T, int C, int64_t N, int k, int dil, const unsigned char* mask,
                               int mask_shift);
ConvClxParams clx_conv2_params(const ClConv& c2, const SplitClPlanes& T, int C, int64_t N, int k, const float* R, float* Y, const SplitClPlanes* Ys, float beta,
                               int accumulate, const unsigned char* mask, int mask_shift);
// w is [M][K] (Linear / 1x1 conv): bf16 parts (2 = hi + lo, 3 = hi + mid + lo) as MFMA A fragments; K must be a multiple of 16
BfsWeights pack_bfs(WeightStore& ws, const float* w, int M, int K, int parts);

class WeightStore {
  public:
    // cl_parts: 0 = f32 MFMA only, 1 = also pack plain-bf16 fragments, 2 = also pack split-bf16 (hi/lo) fragments, 3 = fp16 fragments
    explicit WeightStore(const Blob& b, int cl_parts = 0) : blob_(b), cl_parts_(cl_parts) {}
    int cl_parts() const { return cl_parts_; }
    void set_cl_parts(int parts) { cl_parts_ = parts; }
    // 1x1 products loaded from now on also get their pre-split fragments for gemm_bfs.hip (0 = none, 2 = bf16x3, 3 = bf16x6)
    int bfs_parts() const { return bfs_parts_; }
    void set_bfs_parts(int parts) { bfs_parts_ = parts; }
    ~WeightStore();
    float* upload(const float* host, size_t n);
    float* tensor(const std::string& name);                      // raw copy
    // raw copy of a tensor whose shape is fixed by the config: a container whose tensor has another shape is rejected here, before
    // any kernel indexes the weights (trailing / leading 1-dims are ignored: [C] == [C, 1] == [1, C])
    float* tensor(const std::string& name, std::initializer_list<int64_t> dims);
    void expect(const PackedConv& c, const std::string& prefix, int cout, int cin, int k) const;
    PackedConv conv(const std::string& prefix, bool bias = true);  // <prefix>.weight [Cout][Cin][k] (+ .bias)
    PackedConv conv_cat(const std::vector<std::string>& prefixes);  // 1x1 convs of one input stacked along Cout
    PackedConv linear(const std::string& prefix);                // <prefix>.weight [Cout][Cin] + .bias
    PackedUpsample upsample(const std::string& prefix, int stride, int padding);  // weight [Cin][Cout][k]
    size_t bytes() const { return bytes_; }
    const Blob& blob() const { return blob_; }

  private:
    const Blob& blob_;
    int cl_parts_ = 0, bfs_parts_ = 0;
    std::vector<void*> allocs_;
    size_t bytes_ = 0;
};

// helpers shared by both models
void conv_plain(const PackedConv& w, Plane x, Plane y, int dil, int pad_l, const unsigned char* mask, int mask_div, hipStream_t s,
                int act = ACT_NONE, float pre_slope = 1.0f, const Plane* res = nullptr, float alpha = 1.0f, float beta = 1.0f,
                int accumulate = 0);
// 1x1 product with pre-split bf16 operands (gemm_bfs.hip): y (f32 plane) and / or ys (bf16 parts) receive act(W x + b) * alpha (+ res) * beta
void conv_bfs(const PackedConv& w, const SplitPlanes& xs, const Plane* y, const SplitPlanes* ys, const unsigned char* mask, int mask_div,
              hipStream_t s, int act = ACT_NONE, const Plane* res = nullptr, float alpha = 1.0f, float beta = 1.0f, int y_rows = -1, int ys_row0 = 0,
              const BfsSplitK* sk = nullptr);
// (y_rows >= 0: only rows < y_rows go to y; ys_row0: only rows >= ys_row0 go to ys)
// y[n][m] (token-major) = x^T W + b : the "weights as B operand" form used for V^T
bool conv_km_to_cl(const PackedConv& w, Plane x, float* y, int ldy, int dil, int pad_l, const unsigned char* mask, int mask_div,
                   hipStream_t s);
bool conv_cl_to_km(const PackedConv& w, const float* x, int ldx, Plane y, int dil, int pad_l, const unsigned char* mask, int mask_div,
                   hipStream_t s, float pre_slope, const Plane* res);
void linear_tokmajor(const PackedConv& w, Plane x, float* y, int ldy, hipStream_t s);

// the library-wide default arithmetic of DeBERTa's 1x1 products (bert.cpp documents the choice): bf16 parts per operand, 0 = exact f32
int default_bert_bfs_parts();
bool flash_parts_enabled();   // vits.cpp: the flow's attention reads pre-split keys / values
int set_flash_parts(int on);
bool sdp_all();               // vits.cpp: every row goes through the stochastic duration predictor (sbv2_debug_set_sdp_all)
int set_sdp_all(int on);      // returns the previous value

// The VITS encoders' attention (vits.cpp; built here for run_encoder and sbv2_debug_vits_attention alike)
constexpr int kTextGap = 16;   // >= 9: DDSConv depthwise dilation 3^2 with k=3
constexpr int kFrameGap = 4;   // >= 25/8 frames: widest decoder tap offset (k=11, d=5) at the first upsampled rate
struct AttnPlan {
    int ng = 0, maxT = 0, lds = 0;
    AttnGroup* d_ag = nullptr;
    GemmGroup* d_st = nullptr;
    GemmGroup* d_pv = nullptr;
    float* S = nullptr;
    float* PW = nullptr;
    double flops = 0;  // algorithmic FLOP of one grouped product over all (utterance, head) problems
};
// one group per (utterance, head) of the packed layout; scores: the unfused path's T x T score blocks and probability bands are allocated as well
AttnPlan make_attn_plan(const SegLayout& lay, int H, int heads, int ld, int window, Arena& ar, hipStream_t stream, bool scores);
// C[groups] = alpha A^T B per GemmGroup (gemm_conv.hip): the unfused attention's S^T = K^T Q and ctx = V P^T
void grouped_gemm(const float* A, int lda, const float* B, int ldb, float* C, int ldc, const GemmGroup* grp, int ng, int maxM, int maxN,
                  float alpha, double flops, hipStream_t s);
// Which fused kernel an encoder's attention takes (same bits whichever it is): kv_parts = keys / values read as bf16 parts written by the q | k | v
// product (vits_flash_attention_parts with `pipelined`), otherwise vits_flash_attention (split-bf16 when split_attn).  SP: the encoder's 1x1 parts code.
struct FlashChoice {
    bool kv_parts = false;
    int pipelined = 1;
};
FlashChoice flash_choice(const AttnPlan& pl, int SP, bool split_attn, int dk);

// DeBERTa's disentangled attention (bert.cpp; built here for BertModel::forward and sbv2_debug_deberta_attention alike).  Each utterance takes one class:
// short (deberta_attention, <= 64 tokens), mid (deberta_attention128), long (deberta_attention_long) or the unfused grouped-GEMM + deberta_softmax path.
enum DebertaAttnMode {
    kDbAuto = -1,      // the model's per-utterance dispatch
    kDbUnfused = 0,    // every utterance on the unfused path (SBV2_BERT_ATTN=unfused)
    kDbShort = 1,      // every utterance on one fused kernel: an utterance it does not fit is an error
    kDbMid = 2,
    kDbLong = 3,
    kDbNoLong = 4,     // the model's dispatch without the long kernel (SBV2_BERT_ATTN=nolong)
};
struct DebertaAttnPlan {
    int span = 0, maxT = 0, lds = 0;
    std::vector<int> tab;            // bucket(i - j) at tab[maxT - 1 + i - j]
    int win_lo = 0, wlen = 0, win_ld = 0;        // bucket window reachable by the batch (long kernel, unfused path)
    int win_lo_s = 0, wlen_s = 1;                // ... by |i - j| <= 63 (short kernel)
    int win_lo_m = 0, wlen_m = 1;                // ... by |i - j| <= 127 (mid kernel)
    std::vector<AttnGroup> ag_s, ag_m, ag_f, ag_l;   // short / mid / long fused, grouped-GEMM path
    std::vector<GemmGroup> g_st, g_c2p, g_p2c, g_pv;
    int64_t s_off = 0, c_off = 0, p_off = 0;
    int maxTL = 0, maxTF = 0;
    double fl_tt = 0, fl_tw = 0;     // algorithmic FLOP of the grouped products (profiling only)
    // device side (upload_table, then upload_groups)
    int* d_tab = nullptr;
    AttnGroup *d_agS = nullptr, *d_agM = nullptr, *d_agF = nullptr, *d_agL = nullptr;
    GemmGroup* d_g = nullptr;        // [4][ngL]: S^T, c2p, p2c, PV
    float *S = nullptr, *C2P = nullptr, *P2C = nullptr, *VT = nullptr;
    int ngS() const { return (int)ag_s.size(); }
    int ngM() const { return (int)ag_m.size(); }
    int ngF() const { return (int)ag_f.size(); }
    int ngL() const { return (int)ag_l.size(); }
    void upload_table(Arena& ar, hipStream_t stream);
    void upload_groups(Arena& ar, hipStream_t stream, int N, int H);   // also allocates the unfused path's score blocks and V^T
};
// lay: the packed batch; ld: pitch of the q / k / v planes; ldp: pitch of the position planes [H][2 span]
DebertaAttnPlan make_deberta_attn_plan(const SegLayout& lay, int H, int heads, int buckets, int max_rel, int ld, int ldp, int mode);
// the fused kernels' launches of a plan (short, mid, long), then the unfused path's (VT: V token-major [N][ldvt], filled by the caller)
void deberta_attention_fused(const DebertaAttnPlan& ap, const float* Q, const float* K, const float* V, int ld, const float* posk, const float* posq,
                             int ldp, int d, float inv_scale, const unsigned char* tok_mask, float* ctx, int ldc, hipStream_t s);
void deberta_attention_unfused(const DebertaAttnPlan& ap, const float* Q, const float* K, int ld, const float* VT, int ldvt, const float* posk,
                               const float* posq, int ldp, int d, float inv_scale, const unsigned char* tok_mask, float* ctx, int ldc, hipStream_t s);
struct BertConfig {
    int vocab, hidden, layers, heads, inter, buckets, max_rel;
    float eps;
    int conv_k = 0;          // DebertaV2Encoder.conv (ConvLayer after layer 0) when conv_kernel_size > 0
    int conv_act = ACT_TANH; // ConvLayer's default activation is tanh (modeling_deberta_v2.py:453)
};

class BertModel {
  public:
    BertModel(const Blob& blob, int device);
    ~BertModel();
    // A second execution context on the same weights: own stream and workspace (micro-batch pipelining)
    BertModel* clone() const;
    int device() const { return device_; }
    const BertConfig& cfg() const { return cfg_; }
    int gemm_parts() const { return bfs_parts_; }   // 0 = exact-f32 products, 2 = bf16x3, 3 = bf16x6, 4 = f16x3
    // ids/mask concatenated over utterances; result stays on the device (out_, layout_)
    void forward(int n, const int64_t* ids, const int64_t* mask, const int64_t* lens);
    void copy_out(float* host);  // [sum S][hidden], utterances concatenated
    const Plane& out() const { return out_; }
    const SegLayout& layout() const { return layout_; }
    hipStream_t stream() const { return stream_; }
    static std::vector<int> bucket_table(int maxS, int buckets, int max_rel);  // bucket(rel) for rel in [-(maxS-1), maxS-1]

  private:
    struct Layer {
        PackedConv q, k, v, o, ffn1, ffn2;
        PackedConv qkv;   // rows q | k | v: one product for the fused-attention path (k-major V)
        float *ln1_g, *ln1_b, *ln2_g, *ln2_b;
        Plane pos_k, pos_q;  // key_proj / query_proj of the LayerNorm'ed relative embeddings: [H][2*span]
    };
    int device_;
    BertConfig cfg_;
    int bfs_parts_ = 0;   // parts code: 0 = exact-f32 products, 2 = bf16x3, 3 = bf16x6, 4 = f16x3 (gemm_bfs.hip)
    std::shared_ptr<WeightStore> ws_;
    float *emb_, *emb_g_, *emb_b_;
    PackedConv conv_;                       // encoder.conv.conv (k = conv_k)
    float *conv_g_ = nullptr, *conv_b_ = nullptr;   // encoder.conv.LayerNorm
    std::vector<Layer> layers_;
    Arena arena_;
    hipStream_t stream_ = nullptr;
    unsigned* sk_counters_ = nullptr;   // this context's arrival counters for gemm_bfs' small-grid K split (kSkCounters, zero between launches)
    static constexpr int kSkCounters = 1024;
    static constexpr size_t kSkWsBytes = (size_t)48 << 20;   // (round 6: the batch's K = 4096 product: 272 tiles x 2 groups x 64 KB)
    SatWatch sat_watch_;                // f16x3 clamp warning of this handle (common.h)
    Plane out_;
    SegLayout layout_;
};

struct VitsConfig {
    int n_vocab, n_tones, n_langs, n_speakers, hidden, inter, filter, heads, enc_layers, enc_kernel, window, gin, style_dim,
        bert_dim, cond_layer_idx, flow_n, flow_layers, flow_kernel, dp_filter, dp_kernel, sdp_kernel, sdp_flows, sdp_bins,
        sdp_dds_layers;
    float sdp_tail;
    std::vector<int> up_rates, up_kernels, res_kernels;
    std::vector<std::vector<int>> res_dilations;
    int up_initial;
    int hop() const {
        int h = 1;
        for (int r : up_rates) h *= r;
        return h;
    }
};

constexpr int kStreamBurst = 8;   // windows per graph replay of the streaming decoder after an utterance's first chunk
// The timeline of a stream over the n rows of one forward (the contract above sbv2_stream_begin_request, include/sbv2_hip.h): row i of
// len[i] = frames[i] * hop native samples lies at place[i] of a silent timeline of `joined` samples; the calls are the rows' chunks in row
// order, then chunk order, call c delivering the output samples [j0, j1) of the timeline.  The library's one place for this arithmetic
// (sbv2_stream_timeline and VitsModel::stream_begin both call it); every check before any device call, refusals as exceptions.
constexpr int64_t kStreamMaxGap = 441000;   // 10 s of silence after a row
struct StreamCall {
    int row;
    int64_t f0;       // the chunk's first frame within its row
    int64_t j0, j1;
};
struct StreamTimeline {
    std::vector<int64_t> place, len;
    int64_t joined = 0;
    std::vector<StreamCall> calls;
};
int64_t stream_min_gap(const PcmFmtSpec& spec);   // 2 ceil(half / L): no output sample on one side of a cut has a filter tap on the other side's row
void stream_check_gaps(const int64_t* gap_after, int64_t n, const PcmFmtSpec& spec);
StreamTimeline stream_timeline(const int64_t* frames, const int64_t* gap_after, int64_t n, int hop, int64_t chunk_frames, const PcmFmtSpec& spec);
// The delivery rule of a voice stream (above sbv2_stream_voice, include/sbv2_hip.h) over timeline t: entry c = the output samples delivered
// once call c has been taken, without a level; `lookahead` = A_v.  Host only; the stream's pushes and sbv2_stream_voice_timeline both read it here.
std::vector<int64_t> stream_voice_upto(const StreamTimeline& t, int hop, int64_t chunk_frames, const PcmFmtSpec& spec, int64_t lookahead);
struct VitsBatch {
    int n = 0;
    const int64_t* t_lens = nullptr;   // [n]
    const int64_t* phones = nullptr;   // concatenated
    const int64_t* tones = nullptr;
    const int64_t* langs = nullptr;
    const int64_t* sids = nullptr;     // [n]
    const float* styles = nullptr;     // [n][style_dim]
    const float* bert_host = nullptr;  // concatenated [bert_dim][T_i] blocks, or null when bert_dev is given
    const Plane* bert_dev = nullptr;   // device plane [bert_dim][*] ...
    const int* bert_map = nullptr;     // ... with HOST map: text column (packed, no gaps, utterance-major) -> source column
    // Assist text (bert_dev only; the contract above sbv2_assist, include/sbv2_hip.h): assist_n > 0 sequences lie in bert_dev at the columns
    // [assist_start[a], assist_start[a] + assist_len[a]) (host arrays); assist_rows [n] (host) names each row's mean and weights.  assist_n == 0:
    // the plain gather, the launches of a batch without an assist.
    int assist_n = 0;
    const int* assist_start = nullptr;
    const int* assist_len = nullptr;
    const AssistRow* assist_rows = nullptr;
    float sdp_ratio = 0.f, length_scale = 1.f, noise_scale = 0.f, noise_scale_w = 0.f;
    uint64_t seed = 0;
    const int64_t* forced_durations = nullptr;  // concatenated, optional
    int utt0 = 0;                               // index of the first utterance in the caller's batch (noise stream keys) ...
    const int64_t* utt_ids = nullptr;           // ... or, for an arbitrary subset (a shard dealt to this GPU), every utterance's index
    // Optional per-row options, host arrays [n]; a null array = the scalar above for every row (row_index null = utt_ids / utt0 + u).
    // forward() broadcasts the scalars into one RowOpts record per row either way: the kernels know rows only.
    const float* row_sdp_ratio = nullptr;
    const float* row_length_scale = nullptr;
    const float* row_noise_scale = nullptr;
    const float* row_noise_scale_w = nullptr;
    const uint64_t* row_seed = nullptr;
    const int64_t* row_index = nullptr;
    hipStream_t after_stream = nullptr;         // when set, the forward's kernels wait for the work queued on this stream
    bool skip_decoder = false;                  // stop after the flow (streaming: the decoder then runs chunk by chunk, stream_*)
};

class VitsModel {
  public:
    VitsModel(const Blob& blob, int device);
    ~VitsModel();
    // A second execution context on the same weights: own stream and workspace (micro-batch pipelining)
    VitsModel* clone() const;
    int device() const { return device_; }
    const VitsConfig& cfg() const { return cfg_; }
    void forward(const VitsBatch& b);
    // Streaming decode (BASELINE configs[4]) of the rows of the last forward(skip_decoder = true): the HiFi-GAN decoder runs on windows of
    // chunk_frames + 2 * stream_halo() frames, ONE hipGraph captured for that fixed shape and replayed per burst of windows; the workspace is
    // bounded by the window.  The stream's state is a global chunk list (stream_layout().calls): every row cut on its own frame grid, row after
    // row; a replay takes the next windows of that list whatever rows they belong to.  stream_begin returns the number of calls; stream_next
    // delivers call ci (in order) into dst (host).  gap_after == nullptr: ONE row without gaps (the single-utterance streams).
    // halo frames per side = the generator's receptive field (from the config: 13.4 frames -> 16 for JP-Extra, SURVEY.md §5 "Long-context")
    int stream_halo() const;
    double stream_receptive_field() const;   // frames per side, before the margin and rounding of stream_halo
    // fmt (optional): the chunks leave the device in that output format (pcm_format.h; normalize must be 0): chunk [a, b) of native samples
    // emits output samples [ceil(a L / M), ceil(b L / M)), computed from the window's exact samples beyond the centre
    // flac (fmt must be s16): the chunks' samples are not delivered but pushed into a FlacStreamEncoder (flac_encode.h) behind each replay
    // level (needs fmt): the formatter stops at y (f64), a StreamLimiter (limiter.h) takes it replay by replay at the fixed gain and holds the
    // ceiling; what it emits is cast / quantised and delivered (or, with flac, pushed into the encoder): delivery runs A samples behind
    // leveler (needs level): a StreamLeveler (leveler.h) scales y in place ahead of the limiter, from the level's gain towards its loudness target
    // gap_after (needs fmt): [n] native samples of silence after each row of the forward, the rows joined as stream_timeline lays them out
    // marks (needs fmt): levels per token and / or per envelope frame of the DELIVERED samples, reduced replay by replay (StreamLevels, marks.h):
    // one push per replay on what crosses PCIe or enters the FLAC encoder; such a stream delivers in order only.  marks->pitch: the pitch contour
    // of the same samples, fed by the same pushes (StreamPitch, marks.h), with or without the levels; in order only as well
    // voice (needs fmt; its pivots one per row): every window's central samples pass the fed shifter (StreamVoice, voice.h) ahead of the
    // formatter, which then reads the shifted rows; delivery runs A_v native samples behind within a row (stream_voice_upto); in order only
    int64_t stream_begin(int chunk_frames, const PcmFmtSpec* fmt = nullptr, bool flac = false, const StreamLevelSpec* level = nullptr,
                         const int64_t* gap_after = nullptr, const StreamMarksSpec* marks = nullptr, const StreamVoiceSpec* voice = nullptr,
                         const StreamLevelerSpec* leveler = nullptr);
    // the output side of the running stream when it is formatted (stream_output.h: its kind, reductions, delivered count), else nullptr
    const StreamOutput* stream_output() const { return sformatted_ ? sout_.get() : nullptr; }
    const StreamTimeline& stream_layout() const { return stl_; }
    int64_t stream_call_bound() const;   // bytes that suffice for any one call of the running stream
    // What call ci completes -> dst_host: the chunk's f32 samples (plain), its output samples (formatted), what the limiter hands back
    // (level: possibly nothing; `fed` = the samples of the chunk taken) or the bytes of the FLAC frames those samples complete (the stream
    // header before the first; possibly none).  A stream that carries state from replay to replay delivers in order only.
    StreamOutput::Taken stream_next(int64_t ci, void* dst_host, int64_t capacity_bytes);
    bool stream_graph_captured() const { return chunk_ && chunk_->exec != nullptr; }
    size_t stream_workspace_bytes() const { return (chunk_ ? chunk_->ar.capacity() : 0) + (burst_ ? burst_->ar.capacity() : 0); }
    // results of the last forward
    const std::vector<int64_t>& pcm_lens() const { return pcm_lens_; }
    const std::vector<int64_t>& pcm_offs() const { return pcm_offs_; }
    const float* pcm_device() const { return pcm_; }
    int64_t pcm_total() const { return pcm_total_; }
    void copy_pcm(float* host);  // concatenated
    const std::vector<int>& durations() const { return dur_host_; }   // concatenated predicted w_ceil
    const std::vector<float>& logw() const { return logw_host_; }
    // the durations the last forward expanded (forced where the batch gave them, predicted otherwise), concatenated; row u's tokens are
    // [used_offs()[u], used_offs()[u + 1]).  On the host once forward() has returned (speech marks, marks.h).
    const std::vector<int64_t>& used_durations() const { return used_host_; }
    const std::vector<int64_t>& used_offs() const { return used_offs_; }
    hipStream_t stream() const { return stream_; }
    void set_trace(bool on) { trace_ = on; }
    int decoder_mode() const { return dec_mode_; }
    size_t workspace_bytes() const { return arena_.capacity() + keep_.capacity(); }
    // copies a traced plane of the last forward for utterance `utt`: returns rows/cols
    bool get_trace(const std::string& name, int utt, std::vector<float>& out, int& rows, int& cols);

  private:
    struct Attn {
        PackedConv q, k, v, o;
        PackedConv qkv;   // rows q | k | v: one launch for the three projections (fused attention path)
        float *erk, *erv;
    };
    struct EncLayer {
        Attn attn;
        float *n1g, *n1b, *n2g, *n2b;
        PackedConv ffn1, ffn2;
    };
    struct Encoder {
        float *spk_w = nullptr, *spk_b = nullptr;  // [hidden][gin] row-major (linear_vec)
        std::vector<EncLayer> layers;
    };
    struct DDS {
        std::vector<float*> sep_w, sep_b, n1g, n1b, n2g, n2b;
        std::vector<PackedConv> pw;
    };
    struct ConvFlow {
        float *pre_w, *pre_b;
        DDS dds;
        PackedConv proj;
    };
    struct Coupling {
        PackedConv pre, post;
        Encoder enc;
    };
    struct ResBranch {
        std::vector<PackedConv> c1, c2;
        std::vector<int> dil;
        int k;
    };
    struct Stage {
        PackedUpsample up;
        std::vector<ResBranch> branches;
        int ch, rate;
    };
    struct TraceEntry {
        Plane p;
        const SegLayout* lay;
        int div;  // columns per layout unit (upsampling factor)
    };

    Encoder load_encoder(const std::string& prefix, int n_layers);
    DDS load_dds(const std::string& prefix, int channels);
    void run_encoder(const Encoder& e, Plane x, const SegLayout& lay, const float* spk_vec, Arena& ar);
    void run_dds(const DDS& d, Plane x, const SegLayout& lay, Arena& ar, int shape_L = 0);
    void run_decoder(Arena& ar, Plane z, const SegLayout& fl, const float* cond_vec);
    // channels-last bf16 / split-bf16 MFMA decoder (decoder_cl.cpp)
    struct ClUpGroup {
        ClConv c;
        int ntaps = 0, nph = 0;
        int shift[kMaxTaps];
        int phase_off[kMaxPhases];
    };
    struct ClBranch {
        std::vector<ClConv> c1, c2;
        std::vector<int> dil;
        int k;
    };
    struct ClStage {
        std::vector<ClUpGroup> up;
        ClUpX upx;              // the same transposed convolution as one phased conv_clx launch (large batches of the wide stages; else conv_cl's groups)
        std::vector<ClBranch> branches;
        int cin, ch, rate;
        int mode = 1;   // the stage's arithmetic (dec_mode_ codes 1 .. 3; SBV2_DECODER_STAGES)
    };
    struct ClStagePlan;
    void load_decoder_cl(const Blob& blob);
    std::vector<ClStagePlan> plan_decoder_cl(int64_t Lf, const unsigned char* mask) const;
    void run_decoder_cl(Arena& ar, Plane z, const SegLayout& fl, const float* cond_vec);
    void conv_cl(const ClConv& c, const float* X, int ldx, int NB, float* Y, int ldy, int N, int dil, int pad_l, const unsigned char* mask,
                 int mask_div, float pre_slope, const float* R, int ldr, float beta, int accumulate);
    void trace(const std::string& name, Plane p, const SegLayout& lay, int div = 1);
    // fixed-shape decoder of the streaming path: own arena (never reset while the plan lives), persistent input / conditioning buffers
    // and the captured graph
    struct ChunkPlan {
        int chunk = 0, W = 0, nwin = 1;   // nwin windows of W frames per replay
        Arena ar;
        SegLayout lay;
        Plane zin;
        float* cond = nullptr;
        Arena::Mark mark{0, 0};
        hipGraph_t graph = nullptr;
        hipGraphExec_t exec = nullptr;
        float* pcm = nullptr;       // window PCM (W * hop samples), valid after a replay
        // chunk c + 1 is enqueued before the host waits for chunk c: two pinned host slots + events
        float* host[2] = {nullptr, nullptr};
        hipEvent_t ev[2] = {nullptr, nullptr};
        int64_t slot_ci[2] = {-1, -1};              // the first call of the replay a slot holds (-1: none)
        size_t host_bytes = 0;                      // capacity of each pinned slot
        int64_t fmt_cap = 0;                        // formatted stream: samples the running stream's largest replay of this plan delivers (+ A)
        StreamOutput::Slot out[2];                  // formatted stream: what each slot's replay left there, window by window
        ~ChunkPlan() {
            if (exec) (void)hipGraphExecDestroy(exec);
            if (graph) (void)hipGraphDestroy(graph);
            for (int i = 0; i < 2; ++i) {
                if (host[i]) (void)hipHostFree(host[i]);
                if (ev[i]) (void)hipEventDestroy(ev[i]);
            }
        }
    };
    void ensure_plan(std::shared_ptr<ChunkPlan>& slot, int chunk_frames, int nwin);
    void stream_enqueue(ChunkPlan& c, int64_t c0, int slot);   // the replay of calls c0 .. c0 + nwin - 1
    StreamTimeline stl_;                         // rows, placement and calls of the running stream
    std::vector<int64_t> svoice_upto_;           // a voice stream: the calls' cumulative delivered samples (empty otherwise)
    bool sformatted_ = false;                    // the running stream is formatted (stream_begin with fmt) ...
    std::shared_ptr<StreamOutput> sout_;         // ... and this is everything behind its decoder (made by the first such stream; a clone makes its own)
    bool stream_bursts_ = false;                 // the running stream uses burst_ behind its first chunk
    std::shared_ptr<ChunkPlan> chunk_, burst_;   // one window (an utterance's first chunk) / kStreamBurst windows per replay (every later one)
    Plane z_{};              // flow output of the last forward (frame-rate plane, packed layout fl_)

    int device_;
    VitsConfig cfg_;
    std::shared_ptr<WeightStore> ws_;
    hipStream_t stream_ = nullptr;
    SatWatch sat_watch_;                // f16x3 clamp warning of this handle (common.h)
    hipEvent_t after_ev_ = nullptr;   // orders this context after the producer stream of its DeBERTa features (created on first use)
    Arena arena_, keep_;
    // weights
    float *emb_g_, *emb_, *tone_emb_, *lang_emb_, *style_w_, *style_b_;
    PackedConv bert_proj_, enc_proj_;
    Encoder enc_p_;
    PackedConv dp_c1_, dp_c2_, dp_proj_;
    float *dp_n1g_, *dp_n1b_, *dp_n2g_, *dp_n2b_, *dp_cond_w_, *dp_cond_b_;
    PackedConv sdp_pre_, sdp_proj_;
    float *sdp_cond_w_, *sdp_cond_b_, *sdp_ea_m_, *sdp_ea_logs_ = nullptr, *sdp_ea_scale_ = nullptr;
    DDS sdp_dds_;
    std::vector<ConvFlow> sdp_cf_;  // ConvFlow 2..n (index 0 = flows.3)
    std::vector<Coupling> flows_;
    PackedConv dec_pre_;
    float *dec_cond_w_, *dec_cond_b_, *dec_post_w_;
    float* dec_cond_vec_ = nullptr;  // cond(g) per utterance of the running forward
    int dec_post_k_ = 7;
    std::vector<Stage> stages_;
    int dec_mode_ = 0;  // 0 = exact f32 MFMA (k-major), 1 = split-bf16 (f32-grade), 2 = plain bf16, 3 = fp16 operands
    ClConv cl_pre_;
    std::vector<ClStage> cl_stages_;
    // last-forward results
    float* pcm_ = nullptr;
    int64_t pcm_total_ = 0;
    std::vector<int64_t> pcm_lens_, pcm_offs_;
    std::vector<int> dur_host_;
    std::vector<float> logw_host_;
    std::vector<int64_t> used_host_, used_offs_;
    bool trace_ = false;
    std::map<std::string, TraceEntry> traces_;
    SegLayout tl_, fl_;
};

}  // namespace sbv2
