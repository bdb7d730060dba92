// Launchers for the non-GEMM kernels of the hot path (ops.hip).  All activations are channel-major planes.
#pragma once
#include "common.h"

namespace sbv2 {

// one attention problem = (utterance, head)
struct AttnGroup {
    int64_t qk_off;  // element offset of this head's first row / this utterance's first column in Q, K, ctx planes
    int64_t s_off;   // offset of the [T][lds] score block
    int64_t aux_off; // offset of the per-group auxiliary block (DeBERTa: c2p^T; VITS: P window [2w+1][T])
    int64_t aux2_off;  // DeBERTa: p2c block
    int T;           // sequence length of the utterance
    int lds;         // pitch of the score block
    int col0;        // first column of the utterance in the packed plane (for masks)
    int head;
};

void deberta_embed_ln(const int* ids, const float* emb, int H, const float* gamma, const float* beta, float eps,
                      Plane out, hipStream_t s);
// out = mask * ( act(LN_c(in)) + res )   (act: ACT_NONE / ACT_GELU; res optional; in == out allowed)
// split != null: the result is also written as bf16 parts (the operand format of gemm_bfs.hip)
// shape_L > 0: the kernel is chosen as for a plane of shape_L columns (the choice fixes the order of the per-column sums, i.e. the f32 rounding)
void layernorm_ch(Plane in, Plane out, const float* gamma, const float* beta, float eps, int act, const float* res,
                  int ldr, const unsigned char* mask, hipStream_t s, const SplitPlanes* split = nullptr, int shape_L = 0);
// out = mask * gelu(LN_c(depthwise_conv_k3(in, dilation) + b))
void dds_dw_ln_gelu(Plane in, Plane out, const float* w, const float* b, int dil, const float* gamma,
                    const float* beta, const unsigned char* mask, hipStream_t s, int shape_L = 0);

// fused disentangled attention for short sequences (attn_deberta.hip); deberta_attention_fits says whether a batch qualifies
bool deberta_attention_fits(int maxT, int wlen, int dh);
// the tiled variant for 65 .. 128 tokens (same arguments; the window is the one reachable by the longest sequence of the batch)
bool deberta_attention_long_fits(int T, int dh);   // > 128 tokens: key-tile loop with an online softmax, one workgroup per 32-query tile
void deberta_attention_long(const AttnGroup* groups, int ngroups, int maxT, const float* Q, const float* K, int ld, const float* V,
                            const float* posk, const float* posq, int ldp, int win_lo, int wlen, const int* tab, int tab_center, int span,
                            float inv_scale, const unsigned char* tok_mask, int dh, float* ctx, int ldc, hipStream_t s);
bool deberta_attention128_fits(int T, int dh);
void deberta_attention128(const AttnGroup* groups, int ngroups, const float* Q, const float* K, int ld, const float* V, const float* posk,
                          const float* posq, int ldp, int win_lo, int wlen, const int* tab, int tab_center, int span, float inv_scale,
                          const unsigned char* tok_mask, int dh, float* ctx, int ldc, hipStream_t s);
void deberta_attention(const AttnGroup* groups, int ngroups, const float* Q, const float* K, int ld, const float* V, const float* posk,
                       const float* posq, int ldp, int win_lo, int wlen, const int* tab, int tab_center, int span, float inv_scale,
                       const unsigned char* tok_mask, int dh, float* ctx, int ldc, hipStream_t s);
void deberta_softmax(const AttnGroup* groups, int ngroups, int maxT, float* S, const float* c2pT, const float* p2c,
                     const int* bucket_tab, int tab_center, int span, int win_lo, int win_ld, float inv_scale,
                     const unsigned char* tok_mask, hipStream_t s);
void vits_softmax(const AttnGroup* groups, int ngroups, int maxT, float* S, const float* Q, int ldq, int dk,
                  const float* erk, int window, float qscale, float* pwin, hipStream_t s);
// fused QK^T + relative-key term + online softmax + PV + relative-value term (attn_flash.hip); Q, K, V, ctx: k-major planes
bool flash_pipelined_usable(int dk);   // attn_flash.hip: k_vits_flash_x3q takes this head dimension 
void vits_flash_attention_parts(const AttnGroup* groups, int ngroups, int maxT, const float* Q, int ld, const SplitPlanes& kv, int k_row0,
                                int v_row0, float* ctx, int ldc, int dk, const float* erk, const float* erv, int window, float qscale,
                                hipStream_t s, int pipelined = 1);   // keys / values pre-split into two bf16 parts (rows of kv); same bits as the split variant below
// (pipelined: 0 = k_vits_flash_x3p, 1 = k_vits_flash_x3q with the shape chosen by the grid, 2 = ... its 8-wave shape, 3 = ... its 4-wave shape)
void vits_flash_attention(const AttnGroup* groups, int ngroups, int maxT, const float* Q, const float* K, const float* V, int ld, float* ctx,
                          int ldc, int dk, const float* erk, const float* erv, int window, float qscale, bool split_bf16, hipStream_t s);
void vits_relv_add(const AttnGroup* groups, int ngroups, int maxT, float* ctx, int ldc, int dk, const float* erv,
                   int window, const float* pwin, hipStream_t s);

void add_segvec(Plane x, const float* vec, int vec_ld, const int* seg_of, int div, const unsigned char* mask,
                hipStream_t s, const Plane* src = nullptr);   // x = (src ? *src : x) + vec of the column's segment, 0 outside the mask
void linear_vec(const float* W, const float* bias, int M, int K, const float* v, int ldv, float* out, int ldo, int B,
                hipStream_t s);
void gather_rows(const float* table, int K, const int* idx, float* out, int B, hipStream_t s);
void text_embed(const int* phones, const int* tones, const int* langs, const int* seg_of, const float* emb,
                const float* tone_emb, const float* lang_emb, const float* bertproj, int ldb, const float* styleproj,
                int lds_, float scale, Plane out, hipStream_t s);
void convflow_pre(const float* z0, const float* w, const float* b, Plane cond, Plane out, const unsigned char* mask,
                  hipStream_t s);
void spline_inverse(Plane params, float* z0, float* z1, int nbins, float tail, float inv_sqrt_f,
                    const unsigned char* mask, int L, hipStream_t s);
void swap_rows(float* a, float* b, int L, hipStream_t s);
void flip_channels(Plane in, Plane out, hipStream_t s);
void affine_reverse(float* z0, float* z1, const float* m, const float* logs, const float* scale, const unsigned char* mask, int L,
                    hipStream_t s);   // (x - m) * exp(-logs), or * scale when logs is null (exp(-logs) folded into the weight file)
// The synthesis options of one row (utterance) of a batch, [n] on the device; the kernels below reach a column's record through seg_of.
// (seed, index) key the row's two noise streams: noise_key(seed, index, stream).
struct RowOpts {
    uint64_t seed;
    int index;
    float sdp_ratio, length_scale, noise_scale, noise_scale_w;
    int pad_;
};
static_assert(sizeof(RowOpts) == 32, "RowOpts is one 32-byte record");
// sdp: the stochastic predictor's plane, or null when no row of the batch uses it; sdp_col (may be null: column n of sdp is column n): the column of sdp
// that holds column n's value, -1 where it has none (a row whose sdp_ratio is 0 when only some rows went through the predictor).
void durations(const float* sdp, const float* dp, const int* seg_of, const RowOpts* rows, const unsigned char* mask, int L,
               float* logw, int* dur, hipStream_t s, const int* sdp_col = nullptr);
void noise_fill(float* out, int ld, int rows, const int* seg_of, const int* seg_start, const int* seg_len, const RowOpts* opts, int L,
                int stream_id, hipStream_t s);   // scaled by the row's noise_scale_w
void expand_frames(Plane m_p, Plane logs_p, const int* tok_of_frame, const int* seg_of, const int* seg_start,
                   const int* seg_len, const RowOpts* opts, Plane out, hipStream_t s);   // prior noise scaled by the row's noise_scale
// The windows of one replay of the streaming decoder, ONE launch.  Window w < nwin is described by tab.w[w]: its row's first column z0 in the
// plane z, the row's length len in frames, the window's first frame `first` within the row (negative, or past the end, where the window
// overhangs the row) and the row's index.  For j < W: out[c][out_start[w] + j] = z[c][z0 + first + j] where 0 <= first + j < len, else 0;
// mask[out_start[w] + j] = that condition; cond[w][i] = cond_vec[row][i] for i < cond_dim (cond may be null: nothing is gathered).  A window
// with len == 0 (past the end of the request) is all-zero with mask 0 and a zero cond.  The table travels BY VALUE as a kernel argument: no
// pinned table is rewritten while an earlier replay may still read it.  out_start: device array [nwin] (the plan layout's d_start).
constexpr int kStreamWinMax = 16;
struct StreamWin {
    int z0, len, first, row;
};
struct StreamWinTable {
    StreamWin w[kStreamWinMax];
};
static_assert(sizeof(StreamWinTable) == 256, "the window table is a 256-byte kernel argument");
// h_start: the same [nwin] starts on the host; every window must lie inside out (h_start[w] + W <= out.L, checked before the launch).
void stream_windows(Plane z, const StreamWinTable& tab, int nwin, int W, const int* out_start, const int* h_start, Plane out, unsigned char* mask,
                    const float* cond_vec, int cond_dim, float* cond, hipStream_t s);
// dst[tab[3i + 1] + e] = src[tab[3i] + e] for e < tab[3i + 2], i < n (device table)
void copy_segments(const float* src, float* dst, const int64_t* d_table, int n, hipStream_t s);
void conv_post_tanh(Plane x, const float* w, int k, float slope, const int* seg_start, const int* seg_len,
                    const int64_t* pcm_off, int nseg, int up, int64_t max_samples, float* pcm, hipStream_t s);
void transpose_out(Plane in, int col0, int T, float* out, hipStream_t s);  // out[t][c] = in[c][col0+t]
void gather_cols(Plane in, const int* map, Plane out, hipStream_t s, const float* fill = nullptr);   // out[c][n] = map[n]>=0 ? in[c][map[n]] : fill ? 0 + fill[c] : 0
// Assist text (assist.hip; the contract above sbv2_assist, include/sbv2_hip.h).  One record per row of the batch, [n] on the device: the row of
// `mean` blended into the row's columns (-1: none, the plain gather) and the two f32 weights wf = float(w), omw = float(1.0 - w).
struct AssistRow {
    int mean_row;
    float wf, omw;
    int pad_;
};
static_assert(sizeof(AssistRow) == 16, "AssistRow is one 16-byte record");
// mean[a][c] = float(sum_i double(F[c][a_start[a] + i]) / a_len[a]) in the header's order; a_start / a_len: device arrays [A], mean [A][F.C]
void assist_mean(Plane F, const int* a_start, const int* a_len, int A, float* mean, hipStream_t s);
// gather_cols with out[c][n] = in[c][map[n]] * omw + mean[mean_row][c] * wf for the columns of a row that has an assist (rows[seg_of[n]])
void gather_cols_assist(Plane in, const int* map, const int* seg_of, const AssistRow* rows, const float* mean, Plane out, hipStream_t s);
void fill_zero(void* p, size_t bytes, hipStream_t s);
// channels-last helpers: x[L][C]
void add_segvec_cl(float* x, int L, int C, const float* vec, int vec_ld, const int* seg_of, const unsigned char* mask, hipStream_t s);
void conv_post_tanh_cl(const float* x, int C, int64_t L, const float* w, int k, float slope, const int* seg_start, const int* seg_len,
                       const int64_t* pcm_off, int nseg, int up, int64_t max_samples, float* pcm, hipStream_t s);

}  // namespace sbv2
