/* sbv2_hip.h — C ABI of libsbv2_hip.so: the MI355X-native replacement for the two ONNX Runtime sessions of sbv2_core.
 *
 * Drop-in boundary.  Every entry point cites the reference interface it replaces; paths are relative
 * to the reference repository (tuna2134/sbv2-api @ 2025-03-07).
 *
 * Conventions
 *   - return value 0 = ok; non-zero = error, message via sbv2_last_error() (thread local).  The Rust shim maps this to
 *     sbv2_core::error::Error::OtherError(String) (crates/sbv2_core/src/error.rs:29-30); nothing panics across the FFI.
 *   - inputs are borrowed for the duration of the call (the reference passes views: model.rs:68-90, bert.rs:13-14);
 *     outputs are either caller-allocated or owned buffers released with sbv2_pcm_free (the reference returns owned
 *     arrays: model.rs:108, bert.rs:21).
 *   - a handle is used by one caller at a time (`&mut Session` in the reference: bert.rs:7, model.rs:54).
 *   - model bytes: what the reference hands to load_model, i.e. an ONNX ModelProto (deberta.onnx / model_<name>.onnx: the initializers are
 *     read, the graph itself is replaced by the HIP path), or a whole `.sbv2` file (zstd(tar{model.onnx, style_vectors.json})) for the VITS
 *     handle; also the synthetic weight container "SBV2W001" (sbv2-api_amd/synth.py) used by tests and bench.py.  The bytes need not
 *     outlive *_create (the reference drops them unless max_loaded_models is set: tts.rs:171-175).
 */
#ifndef SBV2_HIP_H
#define SBV2_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sbv2_bert sbv2_bert;         /* replaces the `Session` held in TTSModelHolder.bert (tts.rs:40-46) */
typedef struct sbv2_vits sbv2_vits;         /* replaces the `Session` held in TTSModel.vits2 (tts.rs:32-38) */
typedef struct sbv2_pipeline sbv2_pipeline; /* new: batched, device-resident bert -> vits path */

/* Message of the last failing call on this thread (never NULL). */
const char* sbv2_last_error(void);
/* Number of visible HIP devices (0 when no GPU / no driver). */
int sbv2_device_count(void);

/* ---- load_model(model_file, bert = true)  crates/sbv2_core/src/model.rs:6-50 ---------------------------------- */
int sbv2_bert_create(const uint8_t* model, size_t model_len, int device, sbv2_bert** out);
void sbv2_bert_destroy(sbv2_bert* h);
int64_t sbv2_bert_hidden(const sbv2_bert* h); /* 1024 for deberta-v2-large */
/* arithmetic of the handle's Linear products: 0 = exact f32 MFMA, 2 = bf16x3 (two bf16 parts per operand), 3 = bf16x6 (three parts: f32-grade),
   4 = f16x3 (f16 hi + scaled f16 lo: 22 mantissa bits, three MFMAs per product; the default, SBV2_BERT_GEMM=f32|bf16x3|bf16x6|f16x3) */
int sbv2_bert_gemm_parts(const sbv2_bert* h);

/* ---- bert::predict(session, token_ids, attention_masks) -> Array2<f32>[S, 1024]  crates/sbv2_core/src/bert.rs:6-24
 * out: caller-allocated S * hidden floats, row-major [S][hidden]. */
int sbv2_bert_predict(sbv2_bert* h, const int64_t* token_ids, const int64_t* attention_mask, int64_t S, float* out);
/* new: n utterances at once; ids / mask concatenated, lens[n]; out = concatenated [sum S][hidden].
 * Row block i equals what sbv2_bert_predict returns for utterance i alone. */
int sbv2_bert_predict_batch(sbv2_bert* h, int64_t n, const int64_t* token_ids, const int64_t* attention_mask,
                            const int64_t* lens, float* out);

/* ---- load_model(model_file, bert = false)  crates/sbv2_core/src/model.rs:6-50 --------------------------------- */
int sbv2_vits_create(const uint8_t* model, size_t model_len, int device, sbv2_vits** out);
void sbv2_vits_destroy(sbv2_vits* h);
int64_t sbv2_vits_hop(const sbv2_vits* h);       /* samples per frame (512) */
int64_t sbv2_vits_bert_dim(const sbv2_vits* h);  /* 1024 */
int64_t sbv2_vits_style_dim(const sbv2_vits* h); /* 256 */
/* Decoder arithmetic chosen at create time (env SBV2_DECODER = f32 | bf16x3 | bf16 | f16): 0 = exact f32 MFMA, 1 = split-bf16 MFMA
 * (hi/lo operands, f32-grade, default), 2 = plain bf16 MFMA, 3 = fp16 MFMA operands. */
int sbv2_vits_decoder_mode(const sbv2_vits* h);
/* Device workspace (activation arena) the handle currently holds, in bytes.  It is sized by the largest recent batch: after a dozen
 * calls with much smaller batches it is released and re-grown on demand (a long-running server does not accumulate one arena per shape). */
int64_t sbv2_vits_workspace_bytes(const sbv2_vits* h);

/* ---- model::synthesize(session, bert_ori, x_tst, sid, tones, lang_ids, style_vector, sdp_ratio, length_scale,
 *                        noise_scale, noise_scale_w) -> Array3<f32>[1, 1, L]      crates/sbv2_core/src/model.rs:53-111
 * bert: [bert_dim][T] row-major (Array2 [1024, T], model.rs:56); x_tst/tones/lang: i64[T]; style: f32[style_dim].
 * *pcm: owned buffer of *pcm_len samples (release with sbv2_pcm_free).  noise_seed selects the counter-based noise
 * stream that replaces the graph's RandomNormalLike nodes (irrelevant when both noise scales are 0). */
int sbv2_vits_synthesize(sbv2_vits* h, const float* bert, const int64_t* x_tst, const int64_t* tones,
                         const int64_t* lang_ids, int64_t T, int64_t sid, const float* style_vector, float sdp_ratio,
                         float length_scale, float noise_scale, float noise_scale_w, uint64_t noise_seed, float** pcm,
                         int64_t* pcm_len);
void sbv2_pcm_free(float* pcm);

/* new: a batch of utterances in one call.  All per-token arrays are concatenated over utterances (utterance-major). */
typedef struct sbv2_batch {
    int64_t n;                       /* utterances */
    const int64_t* t_lens;           /* [n] T_text of each utterance */
    const int64_t* x_tst;            /* [sum T] phone ids */
    const int64_t* tones;            /* [sum T] */
    const int64_t* lang_ids;         /* [sum T] */
    const int64_t* sids;             /* [n] */
    const float* style_vectors;      /* [n][style_dim] */
    const float* bert;               /* concatenated [bert_dim][T_i] blocks; NULL in sbv2_pipeline_* (features come from DeBERTa) */
    float sdp_ratio, length_scale, noise_scale, noise_scale_w;
    uint64_t noise_seed;
    const int64_t* forced_durations; /* optional [sum T]: teacher-forced w_ceil (benchmark / parity mode), else NULL */
} sbv2_batch;

/* Runs the batch; results stay on the device until fetched.  pcm_lens: caller-allocated [n]. */
int sbv2_vits_synthesize_batch(sbv2_vits* h, const sbv2_batch* batch, int64_t* pcm_lens);
/* Concatenated PCM of the last batch (sum of pcm_lens samples) -> host.  capacity = samples `pcm` can hold; a batch that does not
 * fit is refused (no write). */
int sbv2_vits_fetch_pcm(sbv2_vits* h, float* pcm, int64_t capacity);
/* Device pointer to the concatenated PCM of the last batch (valid until the next call on the handle). */
const float* sbv2_vits_pcm_device(sbv2_vits* h, int64_t* total);
/* Copies the concatenated PCM of the last batch into caller-owned DEVICE memory (e.g. the send buffer of the RCCL gather). */
int sbv2_vits_copy_pcm_device(sbv2_vits* h, void* dst_device, int64_t capacity);
/* Blocks until every kernel the handle has launched is complete (the batch calls are asynchronous up to the PCM). */
int sbv2_sync(sbv2_vits* h);
/* Predicted integer durations w_ceil (before any forcing) and log-durations of the last batch, concatenated [sum T];
 * capacity = entries each non-NULL output can hold. */
int sbv2_vits_fetch_durations(sbv2_vits* h, int64_t* durations, float* logw, int64_t capacity);
/* Debug/parity: keep named intermediates of the next calls (x_emb, x, stats, z_p, z, dec_pre, dec_stage<i>). */
int sbv2_vits_set_trace(sbv2_vits* h, int on);
int sbv2_vits_get_trace(sbv2_vits* h, const char* name, int64_t utt, float* out, int64_t cap, int64_t* rows, int64_t* cols);

/* ---- new: the whole hot path for a batch, device resident:
 *   bert::predict per utterance (tts.rs:210-212) -> feature repeat by word2ph (tts_util.rs:129-154) -> model::synthesize.
 * token_ids / word2ph are concatenated over utterances; s_lens[n] gives S_i; sum(word2ph of utterance i) must equal t_lens[i]. */
int sbv2_pipeline_create(sbv2_bert* bert, sbv2_vits* vits, sbv2_pipeline** out);
void sbv2_pipeline_destroy(sbv2_pipeline* p);
int sbv2_pipeline_run(sbv2_pipeline* p, const sbv2_batch* batch, const int64_t* token_ids, const int64_t* s_lens,
                      const int64_t* word2ph, int64_t* pcm_lens);

/* ---- new: options per utterance.  Every array is [n] of the batch; a NULL array = the batch's scalar for every row.  Row u's two noise streams
 * are keyed by (noise_seed[u], noise_index[u]): a request's sentence j that is given the request's seed and index j draws the noise it draws
 * when the request runs alone, whatever shares the run with it.  noise_index NULL = the row number.  Refused before any GPU work, with the
 * row named in sbv2_last_error: a non-finite or <= 0 length_scale, an sdp_ratio outside [0, 1], a negative or non-finite noise scale, a
 * negative noise_index (or one >= 2^30). */
typedef struct sbv2_utt_options {
    const float* sdp_ratio;
    const float* length_scale;
    const float* noise_scale;
    const float* noise_scale_w;
    const uint64_t* noise_seed;
    const int64_t* noise_index;
} sbv2_utt_options;
/* sbv2_vits_synthesize_batch / sbv2_pipeline_run with per-utterance options; opts == NULL is exactly the call without them. */
int sbv2_vits_synthesize_batch_opts(sbv2_vits* h, const sbv2_batch* batch, const sbv2_utt_options* opts, int64_t* pcm_lens);
int sbv2_pipeline_run_opts(sbv2_pipeline* p, const sbv2_batch* batch, const sbv2_utt_options* opts, const int64_t* token_ids,
                           const int64_t* s_lens, const int64_t* word2ph, int64_t* pcm_lens);

/* Calls are pipelined: call n runs on execution context n % SBV2_PIPELINE_DEPTH (default 2; own stream + workspace, shared
 * weights) and returns once its kernels are enqueued, so the latency-bound DeBERTa / text / flow part of the next batch overlaps
 * the HiFi-GAN kernels of this one.  Every run gets a TICKET (1, 2, 3, ...: the call number); its results stay available until the
 * run `depth` calls later reuses its context, after which the ticket is stale and every call with it fails. */
int64_t sbv2_pipeline_last_ticket(sbv2_pipeline* p);
int sbv2_pipeline_wait(sbv2_pipeline* p, int64_t ticket);   /* blocks until that run is complete */
int sbv2_pipeline_sync(sbv2_pipeline* p);                   /* ... until every run is complete */
/* Concatenated PCM of a run in utterance order (waits for it); capacity = samples dst can hold (a longer result is refused);
 * dst_is_device != 0: dst is device memory. */
int sbv2_pipeline_fetch_pcm_ticket(sbv2_pipeline* p, int64_t ticket, float* dst, int64_t capacity, int dst_is_device);
int sbv2_pipeline_fetch_pcm(sbv2_pipeline* p, float* dst, int64_t capacity, int dst_is_device);   /* the most recent run */
/* Pinned (page-locked) host memory for PCM destinations: device -> host copies into it run at the full PCIe rate and overlap compute. */
void* sbv2_host_alloc(size_t bytes);
void sbv2_host_free(void* p);

/* ---- new: output formats (the reference returns 44.1 kHz mono f32 only: tts_util.rs:163-180).  The PCM of a run is resampled to a common rate
 * (rational polyphase, L / M = rate / 44100 in lowest terms), optionally peak-normalised per output signal and quantised to 16 bits ON THE DEVICE,
 * before it crosses PCIe.  Convention: y[j] = sum_k h[j M - k L + half] x[k], j < ceil(N L / M), x = 0 outside [0, N); h = a Kaiser-windowed sinc
 * (cutoff 0.45 min(44100, rate), beta 8.6, half = 32 max(L, M)), every polyphase branch summing to 1; i.e. scipy.signal.resample_poly(x, L, M,
 * window = h / L).  s16 = clamp(rint(y g 32767), -32767, 32767), little-endian; g = 1 / max|y| of the signal when normalising (1 for silence).
 *
 * G.711 (telephony: PCMU / PCMA), encoded ON THE DEVICE.  encoding 7 = mu-law, 6 = A-law: the WAVE format tags of the two laws, so the number
 * a caller writes into a WAV header is the number it passes here (2, 3, 4 and 5 stay refused).  Each delivered sample is ONE byte: the G.711
 * code of q, the s16 integer that encoding 1 delivers for the same sample (q = clamp(rint(v 32767), -32767, 32767) after the gain stage).  A
 * mu-law or A-law fetch is therefore byte for byte enc(the s16 fetch) with the same format fields; capacities and out_lens are in samples,
 * and samples equal bytes.  With >> an arithmetic shift and lg = floor(log2):
 *   mu-law encode:  s = q < 0;  m = min(|q|, 32635) + 132;  e = lg(m) - 7 (0..7);  mant = (m >> (e + 3)) & 15;
 *                   code = ~(s * 0x80 | e << 4 | mant) & 0xFF
 *   mu-law decode:  u = ~code & 0xFF;  t = (((u & 15) << 3) + 132) << ((u >> 4) & 7);  value = u & 0x80 ? 132 - t : t - 132
 *   A-law encode:   p = q >= 0;  m = (p ? q : -q - 1) >> 3;  e = m < 32 ? 0 : lg(m) - 4;  mant = e == 0 ? (m >> 1) & 15 : (m >> e) & 15;
 *                   code = (p * 0x80 | e << 4 | mant) ^ 0x55
 *   A-law decode:   a = code ^ 0x55;  e = (a >> 4) & 7;  t = ((a & 15) << 4) + 8;  if e >= 1: t = (t + 256) << (e - 1);
 *                   value = a & 0x80 ? t : -t
 * The decoders are the tables of ITU-T G.711 scaled to 16 bits; the mu-law encoder is the common 16-bit form (bias 132, clip 32635), the
 * A-law encoder the common 13-bit form on q >> 3.  Anchors: mu-law enc(0) = 0xFF, enc(-1) = 0x7F ("minus zero": decodes to 0, re-encodes to
 * 0xFF, the one code of 256 that does not round-trip), enc(32767) = 0x80, enc(-32767) = 0x00, decoded range +-32124; A-law enc(0) = 0xD5,
 * enc(-1) = 0x55, enc(32767) = 0xAA, enc(-32767) = 0x2A, decoded range +-32256, every code round-trips.  dec(enc(q)) is non-decreasing in q
 * and |dec(enc(q)) - q| is at most half the segment's step (mu-law 1 << (e + 3), A-law 16 for e = 0, else 8 << e).  Saturation: mu-law
 * clips |q| above 32635 (-0.035 dBFS) to its top level 32124 (an error of at most 643, never a wrap); A-law's top level 32256 stands for
 * every q >= 31744 or q <= -31745.  normalize, the loudness gain and the limiter come before the quantiser and compose unchanged: their
 * stats are those of the s16 fetch bit for bit.  FLAC takes s16 only: 7 / 6 are refused by everything FLAC. */
typedef struct sbv2_pcm_format {
    int32_t sample_rate;   /* 8000 16000 22050 24000 32000 44100 48000; anything else is refused */
    int32_t encoding;      /* 0 = f32, 1 = s16 little-endian, 7 = G.711 mu-law, 6 = G.711 A-law (one byte per sample) */
    int32_t normalize;     /* 0 = none, 1 = peak of each output signal -> full scale */
    int32_t reserved;      /* must be 0 */
} sbv2_pcm_format;
/* Host only: samples of a signal of n_native samples at 44.1 kHz in that format, ceil(n L / M); -1 (message in sbv2_last_error) when fmt is bad. */
int64_t sbv2_pcm_format_length(const sbv2_pcm_format* fmt, int64_t n_native);
/* Host only: the G.711 laws above on n s16 integers (-32768 is taken as -32767) / n codes; encoding 7 = mu-law, 6 = A-law, anything else is
 * refused with a message.  What a client needs to play, mix or check the delivered bytes. */
int sbv2_g711_encode(int32_t encoding, const int16_t* q, int64_t n, uint8_t* codes);
int sbv2_g711_decode(int32_t encoding, const uint8_t* codes, int64_t n, int16_t* q);
/* Test hook: the gain-stage kernel of the output chain on host f64 signals (nsig >= 1 signals of lens[i] samples, back to back in x), signal i
 * times gains[i], delivered in `encoding` (0, 1, 7, 6) -> dst (host; sum of lens samples, back to back as well: a G.711 signal starts at any
 * byte offset).  The device output lies between guard bands; a byte written outside it fails the call. */
int sbv2_debug_pcm_cast(int device, const double* x, const int64_t* lens, int nsig, const double* gains, int32_t encoding, void* dst);
/* Test hook: the formatting launches themselves (resampler, and peak normalisation when fmt asks for it) on a host table of pieces and signals.
 * x = nx native samples.  pieces [npieces][3] = offset into x, t0, len: x[offset, offset + len) lies at [t0, t0 + len) of a silent timeline.
 * sigs [nsig][4] = j0, j1, p0, p1: the output samples [j0, j1) of the timeline whose pieces are [p0, p1) (sorted by t0, disjoint; pieces of
 * different signals may overlap), delivered back to back in signal order -> dst (host; sum of j1 - j0 samples in fmt's encoding).
 * expose_y != 0: the run ends before the gain stage and dst receives the resampler's f64 samples (fmt->normalize must be 0).  peaks (may be
 * NULL): when fmt normalises, max |y| of each signal, the value whose reciprocal is the gain.  Refused with a message before any device call,
 * nothing written: a bad fmt, ranges that are no ranges (j1 < j0, p1 < p0, outside the table or x), unsorted or overlapping pieces of a
 * signal.  On the device every piece is a copy of its own between NaN words and the output lies between guard bands; a byte written outside
 * it fails the call. */
int sbv2_debug_pcm_format(int device, const float* x, int64_t nx, const int64_t* pieces, int npieces, const int64_t* sigs, int nsig,
                          const sbv2_pcm_format* fmt, int expose_y, void* dst, double* peaks);
/* Host-only test hook: the prototype h of a rate (*len = 2 half + 1 taps at 44100 L Hz) and L, M.  h may be NULL (query); else cap >= *len. */
int sbv2_pcm_format_taps(int32_t sample_rate, float* h, int64_t cap, int64_t* len, int32_t* L, int32_t* M);
/* Formats run `ticket` on its context's stream (waits for it) and copies the result into HOST memory dst (capacity_bytes; a longer result is refused
 * and nothing is written).
 *   place == NULL: one signal per utterance, concatenated in utterance order; out_lens[n] = samples of each.
 *   place != NULL: ONE signal: the run's utterances laid on a silent timeline of joined_len native samples, utterance i starting at place[i]
 *                  (in bounds and non-overlapping, else refused); out_lens[0] = its samples.
 * f32 at 44100 without normalisation and place == NULL returns exactly the bytes of sbv2_pipeline_fetch_pcm_ticket. */
int sbv2_pipeline_fetch_pcm_format(sbv2_pipeline* p, int64_t ticket, const sbv2_pcm_format* fmt, const int64_t* place, int64_t joined_len,
                                   void* dst, int64_t capacity_bytes, int64_t* out_lens);

/* ---- new: FLAC output (RFC 9639), encoded ON THE DEVICE from the s16 samples of sbv2_pipeline_fetch_pcm_format.  One stream per signal: mono,
 * 16 bits, fMT->sample_rate, fixed 4096-sample blocks (the last may be shorter), STREAMINFO with min / max frame size and total samples, MD5
 * zero ("not computed"); each block is the cheapest of CONSTANT, FIXED 0-4, LPC 1-12 (Tukey(0.5) window, precision 15) and VERBATIM, with
 * Rice partition orders <= 8; streamable subset.  The bytes are a pure function of the samples: two fetches of one ticket are identical. */
/* Host only: an upper bound on the bytes of one signal's stream, n = sbv2_pcm_format_length(fmt, n_native) samples in frames of 4096:
 * 42 + 16 ceil(n / 4096) + 2 n (per frame the largest header, a VERBATIM subframe and the CRC-16).  -1 (message in sbv2_last_error) when
 * fmt is bad or its encoding is not 1 (s16; G.711 codes have no FLAC form either). */
int64_t sbv2_flac_bound(const sbv2_pcm_format* fmt, int64_t n_native);
/* The signals of sbv2_pipeline_fetch_pcm_format (same place / joined_len rules; fmt->encoding must be 1 = s16, fmt->normalize as there),
 * each encoded as one FLAC stream; the streams are written back to back into HOST memory dst, out_bytes[i] = stream i's size (one entry
 * per utterance, or one for the joined timeline).  Waits for the run.  A result longer than capacity_bytes is refused and nothing is
 * written (sbv2_flac_bound sums give a capacity that always suffices). */
int sbv2_pipeline_fetch_flac(sbv2_pipeline* p, int64_t ticket, const sbv2_pcm_format* fmt, const int64_t* place, int64_t joined_len,
                             uint8_t* dst, int64_t capacity_bytes, int64_t* out_bytes);
/* Test hook: the same device encoder on host s16 signals (nsig >= 1 signals of lens[i] samples, back to back in x) on `device`, at
 * sample_rate (a rate of sbv2_pcm_format).  Output as sbv2_pipeline_fetch_flac. */
int sbv2_debug_flac_encode(int device, const int16_t* x, const int64_t* lens, int nsig, int32_t sample_rate, uint8_t* dst, int64_t capacity,
                           int64_t* out_bytes);

/* ---- new: loudness normalisation (ITU-R BS.1770-4 integrated loudness, EBU R128 / ATSC A/85 style targets) ON THE DEVICE.  Measured in f64
 * on each output signal y of sbv2_pipeline_fetch_pcm_format (resampled to fs, before any gain or quantisation; mono, channel weight 1):
 *   K-weighting: shelf (f0 1681.974450955533 Hz, G 3.999843853973347 dB, Q 0.7071752369554196) then high-pass (f0 38.13547087602444 Hz,
 *     Q 0.5003270373238773), biquads derived at fs in the libebur128 form, transposed direct form II from zero state -> w;
 *   S = fs / 10; quarter q = sum w^2 over [q S, (q + 1) S) (complete quarters only); block j = quarters j..j+3, z_j = sum / (4 S),
 *     l_j = -0.691 + 10 log10 z_j; blocks with l_j > -70 pass the absolute gate; Gr = -0.691 + 10 log10(mean z of those) - 10; blocks with
 *     l_j > Gr pass as well; L = -0.691 + 10 log10(mean z of the blocks passing both) LUFS, -inf when none does.  A signal shorter than 4 S
 *     samples is one block over its whole length; an empty one gives -inf.
 *   True peak: TP = 20 log10 max |z| dBTP, z = scipy.signal.resample_poly(y, 4, 1, window = h4 / 4), h4[n] = sinc(n / 4) I0(8.6 sqrt(1 -
 *     (n / 48)^2)) / I0(8.6), n in [-48, 48], each phase (n mod 4) scaled to sum to 1; -inf for silence.  TP >= the sample peak.
 *   Gain: G = min(target - L, ceiling - TP) dB when L is finite, else 0 (G may be positive); output y 10^(G / 20), then the f32 cast or the
 *     s16 quantiser of sbv2_pcm_format.  With ceiling <= 0 s16 never clips.
 * The sbv2_stream_* and sbv2_node_* paths have no loudness: integrated loudness needs the whole signal (as peak normalisation does). */
typedef struct sbv2_loudness {
    double target_lufs;          /* [-70, -5] */
    double true_peak_max_dbtp;   /* [-20, 0] */
} sbv2_loudness;
/* The signals of sbv2_pipeline_fetch_pcm_format (same place / joined_len rules; fmt->normalize must be 0), each measured and scaled as above;
 * out-of-range or non-finite ln fields are refused.  ln == NULL: measure only (the bytes equal sbv2_pipeline_fetch_pcm_format's).
 * stats (NULL or 3 doubles per signal): L before the gain (LUFS), TP before the gain (dBTP), the applied G (dB).  Two fetches of one run give
 * identical bytes and stats. */
int sbv2_pipeline_fetch_pcm_loudness(sbv2_pipeline* p, int64_t ticket, const sbv2_pcm_format* fmt, const sbv2_loudness* ln,
                                     const int64_t* place, int64_t joined_len, void* dst, int64_t capacity_bytes, int64_t* out_lens,
                                     double* stats);
/* The same signals as FLAC streams (fmt->encoding must be 1), exactly as sbv2_pipeline_fetch_flac encodes them; stats as above. */
int sbv2_pipeline_fetch_flac_loudness(sbv2_pipeline* p, int64_t ticket, const sbv2_pcm_format* fmt, const sbv2_loudness* ln,
                                      const int64_t* place, int64_t joined_len, uint8_t* dst, int64_t capacity_bytes, int64_t* out_bytes,
                                      double* stats);
/* Host only: the K-weighting at a supported rate: coef[10] = shelf b0 b1 b2 a1 a2, then high-pass b0 b1 b2 a1 a2 (a0 = 1). */
int sbv2_loudness_kweight(int32_t sample_rate, double* coef);
/* Test hook: the device meter on host f64 signals (nsig >= 1 signals of lens[i] samples, back to back in x) on `device` at sample_rate (a rate
 * of sbv2_pcm_format; no resampling); stats (3 doubles per signal) as above, G from ln (NULL: 0). */
int sbv2_debug_loudness(int device, const double* x, const int64_t* lens, int nsig, int32_t sample_rate, const sbv2_loudness* ln,
                        double* stats);

/* ---- new: look-ahead true-peak limiter ON THE DEVICE, for loudness targets the gain above cannot reach.  G = min(target - L, ceiling - TP)
 * is peak-bound whenever the signal's peak-to-loudness ratio TP - L exceeds ceiling - target (speech: near 20 dB, so under -1 dBTP every
 * target above about -21 LUFS is missed).  The limiter takes the peaks down by at most max_reduction_db and raises the rest.  In f64 on each
 * output signal y at fs (before any gain), with L and TP as above, c = 10^(ceiling / 20), D = max_reduction_db, K = fs div 100 (10 ms):
 *   1. Envelope, once per signal: z = the 4x interpolation of y defined for TP (h4); e[n] = max |z[4 n + d]| for d in -3..3, z = 0 outside
 *      the signal.  So e[n] >= |y[n]|, and every z sample is seen by both neighbours.
 *   2. For a pre-gain G dB, g0 = 10^(G / 20):
 *        r[n] = min(1, c / (g0 e[n])), 1 where e[n] = 0;
 *        m[n] = min r[n .. n + K - 1], with r = 1 past the end;
 *        s[n] = sum_{k < K} h[k] m[n - k], with m = m[0] before the start, h[k] = sin^2(pi (k + 0.5) / K) scaled to sum to 1;
 *        x[n] = y[n] g0 s[n].
 *      Every m[n - k] is a minimum over a window that contains n (m[0] = min r[0 .. K - 1] stands in before the start, and contains every
 *      n < K - 1), and s[n] is a convex combination of them, so s[n] <= r[n] and |x[n]| <= c for every sample: with ceiling <= 0 s16 cannot
 *      clip.  In floating point the bounds hold up to a few ulp (the taps sum to 1 within rounding); s[n] is therefore taken as
 *      min(sum, r[n]) and x[n] is clamped to [-c, c], which moves a value by rounding errors only.  A signal whose first 10 ms hold a peak
 *      starts at that peak's gain instead of fading down from 1: with m = 1 before the start the sum would stay near 1 over the first
 *      K - 1 samples whatever r is, and only a per-sample min could hold a loud onset, in steps of up to D dB between neighbours.
 *      Windows never cross a signal edge.
 *   3. Make-up, three evaluations: Gcap = ceiling - TP + D; G_0 = min(target - L, Gcap); for i = 0, 1: L_i = the integrated loudness of x
 *      at G_i, G_{i+1} = min(G_i + target - L_i, Gcap) (G_i when L_i = -inf).  The output is x at G_2.  Gcap bounds the depth: no sample is
 *      reduced by more than D dB, and an unreachable target cannot run away.
 *   4. Idle rule: when G_0 <= ceiling - TP (g0 max e <= c: the scale alone fits under the ceiling, or D = 0) or L = -inf, the signal takes
 *      the gain path above: the delivered bytes and the first three stats equal those of sbv2_pipeline_fetch_pcm_loudness /
 *      _fetch_flac_loudness with the same target and ceiling, bit for bit.
 *   stats, 6 doubles per signal: L and TP before (as above), G_2, L_out and TP_out of the delivered x (before the cast or quantiser), and
 *      the deepest reduction 20 log10 min s (<= 0; 0 when idle).  Step 2 bounds the samples, not the interpolated peak of the
 *      gain-modulated signal: TP_out is reported, not bounded.  Measured at most 1e-5 dB above the ceiling, on speech-like
 *      signals and on dense noise-like audio limited at the full depth alike (s moves slowly against the interpolator's 24 samples).
 * The sbv2_stream_* and sbv2_node_* paths have no limiter, as they have no loudness; a stream can take step 2 alone at a gain fixed ahead:
 * struct sbv2_stream_level. */
typedef struct sbv2_limiter {
    double target_lufs;          /* [-70, -5] */
    double true_peak_max_dbtp;   /* [-20, 0] */
    double max_reduction_db;     /* [0, 12] */
    double reserved;             /* must be 0 */
} sbv2_limiter;
/* The signals of sbv2_pipeline_fetch_pcm_loudness (same place / joined_len rules; fmt->normalize must be 0) through the limiter; lim must
 * not be NULL, out-of-range or non-finite fields and a non-zero reserved are refused.  stats: NULL or 6 doubles per signal.  Two fetches of
 * one run give identical bytes and stats. */
int sbv2_pipeline_fetch_pcm_limited(sbv2_pipeline* p, int64_t ticket, const sbv2_pcm_format* fmt, const sbv2_limiter* lim,
                                    const int64_t* place, int64_t joined_len, void* dst, int64_t capacity_bytes, int64_t* out_lens,
                                    double* stats);
/* The same signals as FLAC streams (fmt->encoding must be 1), exactly as sbv2_pipeline_fetch_flac encodes them; stats as above. */
int sbv2_pipeline_fetch_flac_limited(sbv2_pipeline* p, int64_t ticket, const sbv2_pcm_format* fmt, const sbv2_limiter* lim,
                                     const int64_t* place, int64_t joined_len, uint8_t* dst, int64_t capacity_bytes, int64_t* out_bytes,
                                     double* stats);
/* ---- new: ONE signal from a subset of a run's rows, through the same output chain as the six formatted fetches above: a run that holds
 * several requests hands each of them its own joined, resampled, gain-staged and encoded signal.  The listed rows are laid on a silent timeline
 * of joined_len native samples, row utts[i] starting at place[i].  Refused (nothing written): a row outside [0, n) or listed twice, a placement
 * out of bounds or overlapping, both loudness and limiter given, a stale ticket, a result longer than capacity_bytes, and whatever the
 * corresponding joined fetch refuses in fmt / loudness / limiter.  out_count: samples (flac = 0) or bytes (flac = 1); stats: NULL, or 3
 * (loudness) / 6 (limiter) doubles.  The run's PCM is only read: any number of requests may be fetched from one ticket, in any order. */
typedef struct sbv2_fetch_request {
    const int32_t* utts;         /* [n_utts] rows of the run that form this signal */
    int32_t n_utts;
    const int64_t* place;        /* [n_utts] */
    int64_t joined_len;
    const sbv2_pcm_format* fmt;
    const sbv2_loudness* loudness;   /* at most one of loudness / limiter non-NULL */
    const sbv2_limiter* limiter;
    int32_t flac;                /* 0 = PCM bytes (or G.711 codes) in fmt's encoding, 1 = one FLAC stream (fmt->encoding must be 1) */
} sbv2_fetch_request;
int sbv2_pipeline_fetch_request(sbv2_pipeline* p, int64_t ticket, const sbv2_fetch_request* req, void* dst, int64_t capacity_bytes,
                                int64_t* out_count, double* stats);

/* ---- new: speech marks.  When each token (phone id, blanks included) is spoken in a delivered signal, and how loud it is there.
 * Token spans.  Row u of a run has tokens t < t_lens[u]; token t has the duration d[t] in frames as the run expanded it: the batch's
 *   forced_durations where given, the predicted ones otherwise.  With c the exclusive prefix sum of d and hop = sbv2_vits_hop, token t occupies
 *   native samples [hop c[t], hop c[t + 1]) of its row.  A row placed at native position `place` of a joined timeline and delivered at the rate
 *   L / M of a sbv2_pcm_format maps native position a to the delivered index J(a) = ceil(a L / M), the rule of sbv2_pcm_format_length, so the
 *   delivered span of token t is [J(place + hop c[t]), J(place + hop c[t + 1])).  Hence: the spans of a row are contiguous and monotone
 *   (end[t] == start[t + 1]); the first starts at J(place); where the row's durations sum to >= 1 the last ends at J(place + pcm_len); a
 *   zero-duration token has an empty span; a row whose durations sum to 0 still synthesises one frame (clamp_min(sum, 1)), all its spans are
 *   empty at J(place) and that frame belongs to no token.  The silence between the rows of a joined timeline belongs to no token either.
 * Levels.  For a span [s, e) of the DELIVERED samples v: sumsq = sum v[j]^2 and peak = max |v[j]| as f64, both 0 for an empty span.  The
 *   delivered samples are the f32 values, or the s16 integers as integers (full scale 32767), after the resampler, the gain stage and the
 *   quantiser: exactly what crosses PCIe or enters the FLAC encoder.  For s16 sumsq is exact (integers below 2^53); for f32 every square is
 *   exact in f64 and only the order of the sum is the library's (within len 2^-52 relative of any other order).  The order is fixed: two
 *   fetches of one ticket give identical bits.  dBFS = 10 log10(sumsq / n) (s16: divided by 32767^2) is the caller's arithmetic.
 *   G.711 (encoding 7 / 6): v[j] is the integer the delivered byte decodes to (the decode rules of sbv2_pcm_format), so sumsq and peak are
 *   exact as for s16 and full scale stays 32767.
 * Envelope (optional, env_hop > 0 delivered samples): frame f = [f env_hop, min((f + 1) env_hop, out_len)), n_env = ceil(out_len / env_hop)
 *   frames, each with the same sumsq and peak; out_len = the delivered samples of the signal.
 * The levels are ONE segmented reduction over the samples in HBM (marks.hip), enqueued before the fetch's only synchronisation; timing alone
 *   (tok_sumsq == tok_peak == NULL, env_hop == 0) launches nothing, and a fetch without marks does nothing new at all. */
typedef struct sbv2_marks {
    int64_t tok_capacity;                 /* in: entries each token array holds */
    int64_t* tok_start; int64_t* tok_end; /* out: delivered-sample spans */
    double* tok_sumsq; double* tok_peak;  /* out; either may be NULL with the other: timing only, no kernel launch */
    int64_t n_tokens;                     /* out: sum of t_lens over the listed rows */
    int32_t env_hop; int32_t reserved;    /* in: 0 = no envelope; reserved must be 0 */
    int64_t env_capacity; double* env_sumsq; double* env_peak; int64_t n_env;
} sbv2_marks;
/* sbv2_pipeline_fetch_request that also fills *marks: the tokens of the rows in the order of req->utts, then token order within each row.
 * marks == NULL is exactly sbv2_pipeline_fetch_request; with marks the audio bytes, out_count and stats are those of the same fetch without.
 * All six gain / sink combinations are supported, FLAC included.  Refused with nothing written, besides everything that call refuses: a
 * tok_capacity below the rows' token count, an env_capacity below n_env, a negative env_hop, a non-zero reserved, env_hop > 0 with NULL
 * envelope arrays, one of tok_sumsq / tok_peak NULL without the other. */
int sbv2_pipeline_fetch_request_marks(sbv2_pipeline* p, int64_t ticket, const sbv2_fetch_request* req, void* dst, int64_t capacity_bytes,
                                      int64_t* out_count, double* stats, sbv2_marks* marks);
/* Host only: the span arithmetic above in one place (the fetch and the stream both call it): start[t], end[t] for n_tokens durations (>= 0)
 * of one row at `place`, at fmt's rate (its encoding and normalize do not matter).  Refused: a bad fmt, a negative duration or place, hop < 1. */
int sbv2_marks_spans(const int64_t* durations, int64_t n_tokens, int32_t hop, int64_t place, const sbv2_pcm_format* fmt, int64_t* start,
                     int64_t* end);
/* Test hook: the level reduction on host samples x[n] (encoding 0 = f32, 1 = s16, 7 / 6 = G.711 codes, one byte each) over the segments [starts[i], ends[i]) within [0, n]. */
int sbv2_debug_segment_levels(int device, const void* x, int encoding, int64_t n, const int64_t* starts, const int64_t* ends, int64_t nseg,
                              double* sumsq, double* peak);

/* ---- new: the pitch contour of a delivered signal.  How high the voice is, frame by frame, estimated on the device from the samples the
 * speech marks are taken of: YIN (de Cheveigne & Kawahara 2002, steps 2 - 5), stated so that it is reproducible.
 * Input.  The delivered samples v[0 .. n) of ONE signal at rate sr, read as the levels read them (f32 values, s16 integers, or the integers
 *   that G.711 codes decode to); positions outside [0, n) read as 0.  Parameters hop >= 1, f0_min, f0_max, threshold with
 *   40 <= f0_min < f0_max <= sr / 4 and 0 < threshold < 1 (everything else is refused).
 * Frames.  tau_min = floor(sr / f0_max), tau_max = ceil(sr / f0_min), W = tau_max; n_frames = ceil(n / hop) (0 for n = 0); frame f has its
 *   centre at f hop + hop / 2 (integer division) and its window starts at b = centre - tau_max.
 * Per frame.  d(tau) = sum_{j < W} (v[b + j] - v[b + j + tau])^2 for tau = 1 .. tau_max; S(tau) = sum_{k <= tau} d(k);
 *   c(tau) = double(d(tau)) double(tau) / double(S(tau)), and c(tau) = 1 where S(tau) = 0.
 * Decision.  The smallest tau in [tau_min, tau_max] with c(tau) < threshold, then tau is increased while tau + 1 <= tau_max and
 *   c(tau + 1) < c(tau): that is the lag, and the frame is voiced.  If no tau qualifies the frame is unvoiced and its lag is the smallest tau
 *   in range that attains min c.
 * Result.  The device gives lag, voiced and c- = c(lag - 1), c0 = c(lag), c+ = c(lag + 1) (a neighbour outside [1, tau_max] is replaced by
 *   c0); the HOST computes in plain f64 arithmetic, never contracted: den = c- - 2 c0 + c+; delta = 0.5 (c- - c+) / den if den > 0 and both
 *   neighbours exist, else 0; f0 = voiced ? sr / (lag + delta) : 0; ap = c0 (the aperiodicity: near 0 for a clean periodic frame).
 * Bits.  For the integer encodings d and S are formed in 64-bit integers.  With |v| <= 32768 and tau_max <= 1200 (the 40 Hz floor at 48 kHz)
 *   d tau and S stay below 2^53 (6.2e15 < 9.0e15), so c has exactly one rounding, its division: lag, voiced and the three c values do not
 *   depend on the order of any sum and equal a restatement in int64 / f64 bit for bit.  For f32 samples differences and squares are taken in
 *   f64 in an order the library fixes; only that order is its own (f32 samples that are s16 integers / 32768 still give the s16 bits).
 * On a stream the same contour comes frame by frame: sbv2_stream_begin_request_pitch / sbv2_stream_next_pitch below.
 * Not done here: anything across frames.  Octave-error repair is sbv2_pitch_track below (one best path through the frames' candidates, opt-in);
 *   smoothing of the f0 values is not built. */
typedef struct sbv2_pitch {
    int32_t hop; int32_t reserved;        /* in: delivered samples per frame (>= 1); reserved must be 0 */
    double f0_min, f0_max, threshold;     /* in: Hz, Hz, (0, 1); usual values 70, 600, 0.15 */
    int64_t capacity;                     /* in: entries each given array holds */
    double* f0;                           /* out: Hz, 0 for an unvoiced frame; must not be NULL */
    double* ap;                           /* out, may be NULL: c(lag) */
    int32_t* lag;                         /* out, may be NULL */
    int64_t n_frames;                     /* out: ceil(out_len / hop) */
} sbv2_pitch;
/* sbv2_pipeline_fetch_request_marks that also fills *pitch: the contour of the delivered signal of the request (every gain / sink combination,
 * FLAC included), one more launch before the fetch's only synchronisation.  pitch == NULL is exactly sbv2_pipeline_fetch_request_marks (marks
 * may be NULL either way); with pitch the audio bytes, out_count, stats and marks are those of the same call without, and two fetches of one
 * ticket give identical bits.  The caller's arrays are written only after everything else has succeeded.  Refused with nothing written,
 * besides everything that call refuses: parameters outside the ranges above, capacity < n_frames, a NULL f0, a non-zero reserved. */
int sbv2_pipeline_fetch_request_pitch(sbv2_pipeline* p, int64_t ticket, const sbv2_fetch_request* req, void* dst, int64_t capacity_bytes,
                                      int64_t* out_count, double* stats, sbv2_marks* marks, sbv2_pitch* pitch);
/* Host only: tau_min and tau_max of a rate and a range, under the checks above (0 < sample_rate <= 48000). */
int sbv2_pitch_lags(int32_t sample_rate, double f0_min, double f0_max, int32_t* tau_min, int32_t* tau_max);
/* Test hook: the estimator on host samples x[n] (encoding as sbv2_debug_segment_levels).  pitch: parameters in, f0 / ap / lag / n_frames out as
 * in the fetch; cmnd3 [n_frames][3] (c-, c0, c+) and voiced [n_frames] may be NULL. */
int sbv2_debug_pitch(int device, const void* x, int encoding, int64_t n, int32_t sample_rate, sbv2_pitch* pitch, double* cmnd3, int32_t* voiced);

/* ---- new: pitch and intonation scale.  Raise or lower a voice (pitch_scale) and flatten or exaggerate its melody (intonation_scale).  The model
 * gives no handle on f0, so both are a transform of the synthesized signal: a length-preserving pitch-synchronous overlap-add (TD-PSOLA) of the
 * run's native f32 rows, on the device, BEFORE the formatter.  Every row keeps its length, so placement, delivered lengths, token spans and every
 * later stage (resampler, gain stage, quantiser, FLAC, the marks' levels and their own pitch contour) work unchanged on the shifted voice.
 * Input.  One row x[0 .. n) of f32 at rate sr (the model's rate in the pipeline; the hook takes 1000 <= sr <= 48000); reads outside [0, n) are 0.
 * Parameters (anything else is refused): pitch_scale p in [0.5, 2]; intonation_scale s in [0, 2]; hop H in [sr / 1000, sr / 50] (integer
 *   divisions), 0 = sr / 200; f0_min, f0_max, threshold under the rules of sbv2_pitch, 0 = 70, 600, 0.15.
 * Contour.  YIN exactly as sbv2_pitch states it on x (encoding f32) with hop H, and the parabolic refinement on the device, the same f64
 *   expression as there, never contracted: delta = 0.5 (c- - c+) / den if den > 0 and both neighbours exist, else 0, here limited to [-1, 1] (a
 *   parabola whose vertex lies farther off has not been fitted to a minimum; the limit is what bounds the windows below).  Per frame
 *   T_f = lag + delta (f64) and voiced_f; frame f owns the samples [f H, min((f + 1) H, n)).
 * Target.  f0_f = sr / T_f for voiced frames; their mean m = double(sum llrint(f0_f 65536)) / (65536.0 count), an integer sum, so any order of
 *   reduction gives the same bits; g_f = p (m + s (f0_f - m)) clamped to [f0_min / 2, 2 f0_max]; T'_f = sr / g_f.
 * Phase increments (Q32, int64).  inc_a(f) = llrint(4294967296.0 / T_f) and inc_s(f) = llrint(4294967296.0 / T'_f) for voiced frames; both are
 *   inc_u = llrint(4294967296.0 / (sr / 200)) (integer division) for unvoiced frames.
 * Analysis marks.  phi_a(k) = sum_{i <= k} inc_a(frame(i)), phi_a(-1) = 0; sample k is an analysis mark iff phi_a(k) >> 32 != phi_a(k - 1) >> 32.
 * Synthesis marks.  In an unvoiced frame k is a synthesis mark iff it is an analysis mark.  A voiced run starts at the first sample k0 of a
 *   voiced frame whose predecessor is unvoiced or absent; there phi_s(k0 - 1) = phi_a(k0 - 1); inside the run phi_s(k) = phi_s(k - 1) +
 *   inc_s(frame(k)) and k is a mark iff the integer part changes.  (The increment is constant within a frame: the marks of a frame follow from a
 *   prefix sum over FRAMES and a division, nothing walks the samples.)
 * Mapping.  With the ascending lists ta[0 .. Na) and ts[0 .. Ns): synthesis mark j uses the analysis mark m(j) nearest to ts_j, a tie going to
 *   the earlier one.
 * Window of analysis mark m.  L = ta_m - ta_{m-1} (ta_0 + 1 for m = 0), R = ta_{m+1} - ta_m (n - ta_m for the last).  For integer offsets
 *   -L < u < R: v = double(|u|) / double(u < 0 ? L : R), S = (v v) (3.0 - 2.0 v), w(u) = 1.0 - S, except w = 1 on the left side of mark 0 and on
 *   the right side of the last mark.  Adjacent windows are complementary: the analysis grains partition the row.
 * Output.  In ascending j, in f64, never contracted: num(k) = sum_j w_{m(j)}(k - ts_j) double(x[ta_{m(j)} + k - ts_j]),
 *   den(k) = sum_j w_{m(j)}(k - ts_j); y[k] = float(num / max(den, 1.0)).  A row with no analysis mark is copied.
 * Hence: the length is unchanged; |y[k]| <= max |x| (where den >= 1 y is a convex combination of input samples, elsewhere a sub-unit one), so
 *   the stage cannot create clipping; with p = 1 and s = 1 the two mark lists coincide and y == x bit for bit, and the same holds in any stretch
 *   of unvoiced frames farther than tau_max + H + 2 samples from a voiced one; no half-width exceeds max(tau_max + 1, sr / 200) + 2, which bounds
 *   the gather.  Dividing by den trades level for the peak bound; the loudness stage downstream restores level.
 * Not built: epoch (glottal) alignment of the marks, contour smoothing, energy compensation (octave-error repair of the
 *   contour is opt-in: sbv2_pitch_track and sbv2_pipeline_fetch_request_tracked below; a target per token instead of one pair of scales is
 *   sbv2_token_pitch and sbv2_pipeline_fetch_request_token_pitch below; moving the formants is sbv2_formant and
 *   sbv2_pipeline_fetch_request_formant below).  On a
 *   request stream the same shifter runs chunk by chunk about a pivot the caller names: sbv2_stream_voice and
 *   sbv2_stream_begin_request_voice below; sbv2_node_* and the plain sbv2_stream_begin* entries do not take a sbv2_voice. */
typedef struct sbv2_voice {
    double pitch_scale;          /* [0.5, 2] */
    double intonation_scale;     /* [0, 2] */
    double f0_min, f0_max;       /* Hz; 0 = 70, 600 */
    double threshold;            /* (0, 1); 0 = 0.15 */
    int32_t hop; int32_t reserved;   /* native samples per contour frame, 0 = rate / 200; reserved must be 0 */
} sbv2_voice;
/* sbv2_pipeline_fetch_request_pitch of the listed rows SHIFTED.  voice == NULL, or pitch_scale == 1 and intonation_scale == 1, is exactly that
 * call: no launch, the same bytes.  Otherwise the listed rows are shifted into a scratch buffer laid out like the run's packed PCM and the
 * formatter reads them there; everything else (gain stage, sink, stats, marks, pitch: all of the delivered, shifted signal) is that call.  The
 * run's PCM is only read: a ticket can be fetched any number of times, with and without voice, and two equal fetches give identical bytes.
 * Refused with nothing written: a non-zero reserved, parameters outside the ranges above, and everything that call refuses. */
int sbv2_pipeline_fetch_request_voice(sbv2_pipeline* p, int64_t ticket, const sbv2_fetch_request* req, const sbv2_voice* voice, void* dst,
                                      int64_t capacity_bytes, int64_t* out_count, double* stats, sbv2_marks* marks, sbv2_pitch* pitch);
/* Output samples per workgroup of the overlap-add gather (tests place row lengths around it). */
int32_t sbv2_voice_tile(void);
/* Test hook: the shifter on host rows x laid back to back (lens[nrows] samples each, f32), always through the kernels (p = s = 1 included).
 * period_in / voiced_in (both or neither; one entry per frame, ceil(len / hop) frames per row, rows back to back): the contour to use instead of
 * the estimated one; a voiced period outside [tau_min - 1, tau_max + 1] is refused.  Outputs: y laid out as x; period_out / voiced_out per
 * frame (may be NULL); ta, ts, map [sum(lens) + nrows] each, row i's lists starting at entry sum_{r < i} (lens[r] + 1), and n_marks
 * [nrows][2] = (Na, Ns) per row (all four may be NULL together). */
int sbv2_debug_voice_shift(int device, const float* x, const int64_t* lens, int nrows, int32_t sample_rate, const sbv2_voice* voice,
                           const double* period_in, const int32_t* voiced_in, double* period_out, int32_t* voiced_out, int32_t* ta, int32_t* ts,
                           int32_t* map, int64_t* n_marks, float* y);

/* ---- new: the pitch contour TRACKED across frames (octave-error repair).  sbv2_pitch decides every frame on its own, and "the first lag under
 * the threshold" answers T / 2 or 2 T on single frames whenever a harmonic or subharmonic dips under the threshold first.  Here every frame
 * keeps its candidates and ONE path is chosen through them (the last step of pYIN, RAPT and Praat).  Everything after the c values is integer
 * arithmetic, so the path does not depend on any order of evaluation and equals a sequential restatement bit for bit.
 * Parameters (anything else, a NaN included, is refused; 0 never means "default"): cand_max in (0, 1]; unvoiced_cost and switch_cost in [0, 4];
 *   jump_cost in [0, 16]; reserved = {0, 0}.  The host forms U, Sw, J = llrint(value * 65536) once.  Usual values 0.5, 0.30, 0.20, 1.0.
 * Candidates of a frame.  c(1 .. tau_max) exactly as sbv2_pitch defines it.  tau in [tau_min, tau_max] is a dip iff c(tau) < c(tau - 1) and
 *   c(tau) <= c(tau + 1) (c(tau_max + 1) read as +infinity) and c(tau) < cand_max.  The candidates are the 7 dips with the smallest c (ties: the
 *   smaller tau), or all dips when there are fewer, listed in ascending tau; each carries tau, q = llrint(c(tau) * 65536) and c-, c0, c+ under
 *   the neighbour rule of sbv2_pitch.  A frame may have no candidate (digital silence: S = 0, c = 1).
 * States.  0 .. 6 are the frame's candidates, 7 is "unvoiced" and is always present; absent candidate slots take no part in any minimum.
 * Costs (int64).  local(k) = q_k for a candidate, local(7) = U.  trans(j -> k) = (J |tau_k - tau_j|) / max(tau_k, tau_j) (integer division)
 *   between two candidates, Sw between a candidate and state 7 either way, 0 from 7 to 7.  cost(0, k) = local(k);
 *   cost(f, k) = local(k) + min_j (cost(f - 1, j) + trans(j -> k)), bp(f, k) = the smallest j that attains the minimum.  The last frame takes
 *   the smallest k that attains min cost; the path is the backtrace.  With n_frames < 2^30 the costs stay below 2^52.
 * Result per frame.  On a candidate the frame is voiced, lag = tau and c-, c0, c+ are the candidate's; on state 7 voiced = 0 and lag and the
 *   three c values stay what sbv2_pitch gives for that frame.  f0, ap and the refinement are sbv2_pitch's, unchanged.
 * Hence: a frame with no candidate (a "cut") has a single state, so the frames before and after it do not influence each other's choices and
 *   the path of a signal is the concatenation of the paths of the runs between cuts; the last state before a cut is the smallest j attaining
 *   min (cost_j + trans(j -> 7)).  The library walks those runs side by side on the device.
 * Not built: smoothing of the f0 values (a median and the like), tracking on streams (a best path needs the future; a fixed-lag variant would
 *   be another definition) and on sbv2_node_*, probabilistic voicing (pYIN's several thresholds). */
typedef struct sbv2_pitch_track {
    double cand_max;              /* (0, 1]: a dip at or above it is no candidate */
    double unvoiced_cost;         /* [0, 4]: a frame on state 7 */
    double switch_cost;           /* [0, 4]: between a candidate and state 7 */
    double jump_cost;             /* [0, 16]: times the relative change of the lag between two candidates */
    int32_t reserved[2];          /* must be 0 */
} sbv2_pitch_track;
/* sbv2_pipeline_fetch_request_voice with the contours tracked.  track == NULL is exactly that call.  With track and pitch the delivered contour
 * is the tracked one; with track and a voice that is not the identity the shifter's own contour (native f32, per row, hop H) is tracked with
 * the same parameters before the marks are placed.  The audio bytes of a tracked fetch without a shifting voice are those of the untracked
 * fetch; two fetches of one ticket give identical bits.  Refused with nothing written: track with neither a pitch nor a non-identity voice,
 * parameters outside the ranges above, a non-zero reserved, and everything that call refuses. */
int sbv2_pipeline_fetch_request_tracked(sbv2_pipeline* p, int64_t ticket, const sbv2_fetch_request* req, const sbv2_voice* voice,
                                        const sbv2_pitch_track* track, void* dst, int64_t capacity_bytes, int64_t* out_count, double* stats,
                                        sbv2_marks* marks, sbv2_pitch* pitch);
/* Test hook: the tracker on host samples x[n] (as sbv2_debug_pitch): pitch receives the TRACKED f0 / ap / lag; cand_out [n_frames][15] (ncand,
 * 7 tau, 7 q; 0 in absent slots), c3_out [n_frames][7][3] and state_out [n_frames] (0 .. 6 the candidate, 7 unvoiced) may each be NULL.
 * With cand_in [nf_in][15] the extraction is skipped and the path alone is found on the caller's table: x and pitch may be NULL, c3_in is not
 * read (the path depends on tau and q alone) and only state_out [nf_in], which must be given, is written.  Refused besides everything
 * sbv2_debug_pitch refuses: a table with ncand outside [0, 7], tau not ascending or outside [1, 1200], q outside [0, 65536]. */
int sbv2_debug_pitch_track(int device, const void* x, int encoding, int64_t n, int32_t sample_rate, sbv2_pitch* pitch, const sbv2_pitch_track* track,
                           const int32_t* cand_in, const double* c3_in, int64_t nf_in, int32_t* cand_out, double* c3_out, int32_t* state_out);

/* ---- new: a speech compressor in front of the loudness stage.  Speech cannot always reach the loudness target it is asked for: its
 * peak-to-loudness ratio is near 20 dB, and the limiter's depth is used up before a loud target is met.  The compressor evens out the level
 * differences between syllables and between the sentences of a joined request, so that the limiter behind it is left with the crest only.
 * Per output signal y[0 .. N) at fs, all in f64: the formatter's y before any gain, the array the limiter reads.
 *   L = the integrated loudness of y (the meter of sbv2_loudness).  If L = -inf, N = 0 or ratio == 1 the signal is idle: yc = y bit for bit.
 *   e[n] = the envelope of sbv2_limiter step 1 (computed by the limiter's own code).
 *   Static curve.  T = L + threshold_lu, k = 1 - 1 / ratio; d[n] = k (20 log10 e[n] - T) where e[n] > 0 and that value is > 0, else 0;
 *     dq[n] = llrint(65536 d[n]) (int64; the unit is 1 / 65536 dB, as in sbv2_pitch_track).
 *   Ballistics, in integers, so that no order of evaluation matters.  rho = max(1, llrint(65536 release_db_per_s / fs)),
 *     alpha = max(1, llrint(65536 attack_db_per_s / fs));
 *     p[n] = max_{i <= n} (dq[i] - rho (n - i)): hold, then a release that is linear in dB (sequentially p[n] = max(dq[n], p[n - 1] - rho));
 *     a[n] = max_{i >= n} (dq[i] - alpha (i - n)): the attack ramp AHEAD of a peak (the whole signal is at hand: the stage is not causal);
 *     u[n] = max(p[n], a[n]).  Hence p[n] = prefixmax(dq[i] + rho i)[n] - rho n and a[n] = suffixmax(dq[i] - alpha i)[n] + alpha n: two
 *     plain maximum scans of int64 keys below 2^46.
 *   Smoothing with the limiter's window.  K = fs div 100, h[k] = sin^2(pi (k + 0.5) / K) scaled to sum to 1, c0 = K - 1 - K div 2;
 *     ut[n] = sum_{k < K} h[k] double(u[clamp(n + c0 - k, 0, N - 1)]) / 65536, summed in ascending k and never contracted;
 *     s[n] = 10^(-ut[n] / 20); yc[n] = y[n] s[n].
 *   Hence: 0 < s <= 1, so |yc| <= |y| and the stage cannot create clipping; scans and windows never cross a signal edge; the smoothed
 *   curve may sit below d at an isolated peak, by about alpha K / 4 units: the stage LEVELS the signal, it does not bound it (the limiter
 *   behind it bounds); the knee is hard and the detector reads peaks (the envelope), not a mean square.  The crest factor stays: on
 *   speech-like signals the peak-to-loudness ratio falls from about 21 to about 17 dB, not further.
 *   stats, 3 doubles per signal: L of y, T, and -max ut (the deepest compression in dB; <= 0, 0 when idle).  The 3 or 6 stats of the
 *   loudness or limiter stage behind are then those of yc: everything behind the stage (meter, gain, limiter, cast, quantisers, FLAC, the
 *   marks' levels and pitch) runs unchanged on the compressed signal.
 * Parameters: 0 never means "default" and a NaN is refused.  Usual values 8, 4, 600, 60.
 * Not built: the stage on streams (the threshold needs the whole signal's loudness and the attack looks ahead without bound), on sbv2_node_*
 *   and on the six older formatted fetches; a soft knee, an RMS detector, several bands. */
typedef struct sbv2_dynamics {
    double threshold_lu;        /* [0, 30]: dB above the signal's own integrated loudness */
    double ratio;               /* [1, 20]; 1 = identity */
    double attack_db_per_s;     /* [10, 10000] */
    double release_db_per_s;    /* [1, 1000] */
    double reserved;            /* must be 0 */
} sbv2_dynamics;
/* sbv2_pipeline_fetch_request_tracked with the compressor in front of req's loudness gain or limiter.  dynamics == NULL or ratio == 1 is
 * exactly that call: no launch, the same bytes, and dyn_stats is not written.  Otherwise dyn_stats (may be NULL) receives the 3 doubles above
 * and stats (NULL, or 3 / 6 doubles) those of the stage behind, of yc.  The run's PCM is only read: two fetches of one ticket give identical
 * bytes and stats.  Refused with nothing written: a compressing dynamics with neither req->loudness nor req->limiter (without make-up the
 * stage only makes the signal quieter) or with fmt->normalize, fields out of range or non-finite (ratio == 1 included), a non-zero
 * reserved, and everything that call refuses. */
int sbv2_pipeline_fetch_request_dynamics(sbv2_pipeline* p, int64_t ticket, const sbv2_fetch_request* req, const sbv2_voice* voice,
                                         const sbv2_pitch_track* track, const sbv2_dynamics* dynamics, void* dst, int64_t capacity_bytes,
                                         int64_t* out_count, double* stats, double* dyn_stats, sbv2_marks* marks, sbv2_pitch* pitch);
/* Samples per workgroup of the compressor's scans (tests place signal lengths around it). */
int32_t sbv2_dynamics_tile(void);
/* Test hook: the compressor on host f64 signals laid back to back (as sbv2_debug_limiter), always through the kernels (ratio == 1
 * included).  Outputs, each laid out as the input and each may be NULL: e_out, dq_out (int64), u_out (int64), s_out, y_out (yc); stats 3
 * doubles per signal. */
int sbv2_debug_dynamics(int device, const double* x, const int64_t* lens, int nsig, int32_t sample_rate, const sbv2_dynamics* dynamics,
                        double* e_out, int64_t* dq_out, int64_t* u_out, double* s_out, double* y_out, double* stats);

/* ---- new: per-token pitch targets.  The speech marks say that token 17 sits at 212 Hz; this says "make it 180": query, edit the pitch per
 * token, fetch again.  It is the shifter of sbv2_voice with ONE more factor in the target f0 of a frame; everything not named here is that
 * section, unchanged.  Targets are per token and not per time, so they survive a re-run whose predicted durations differ.
 * Tokens of a frame.  Token t of a row owns the native samples [hop c[t], hop c[t + 1]) (c = the running sum of the row's used durations: the
 *   span rule of sbv2_marks).  Contour frame f (H samples, the voice's hop) belongs to the token whose span holds its centre sample
 *   min(f H + H / 2, n - 1).  A zero-duration token owns no frame; a row whose durations sum to 0 has one frame that belongs to no token; a
 *   frame without a token has rho = 65536 (ratio 1).  The frames of a token are consecutive.
 * Measured mean.  Over the voiced frames of token t: M_t = double(sum llrint(f0_f 65536)) / (65536.0 count_t), an integer sum as the row mean m
 *   is; f0_f = sr / T_f of the contour the marks are placed by (the tracked one when a sbv2_pitch_track is given).  src_f0_t = M_t, 0 where
 *   count_t = 0.
 * Token ratio.  kind 0: r_t = value_t.  kind 1: G_t = p (m + s (M_t - m)) (where the two scales alone would put the token's mean) and
 *   r_t = min(max(value_t / G_t, 0.5), 2.0), f64, never contracted.  Both: rho_t = llrint(r_t 65536) (int64), and rho_t = 65536 where
 *   value_t == 0 or (kind 1) count_t == 0; applied_t = double(rho_t) / 65536.0.
 * Frame ratio.  rho(f) = the rho of the frame's token; with K = smooth and nf the row's frames
 *   R_f = double(sum_{i = max(f - K, 0)}^{min(f + K, nf - 1)} rho(i)) / (65536.0 double(count)), an integer sum inside the row: nothing crosses
 *   rows, and any order of summation gives the same bits.  K is taken as given, 0 = steps at the token boundaries.
 * Target.  g_f = R_f (p (m + s (f0_f - m))), then the clamp to [f0_min / 2, 2 f0_max].  Everything behind g_f is sbv2_voice: T'_f, the
 *   increments, the marks, the mapping, the windows and the gather.
 * Hence: the length is unchanged and |y[k]| <= max |x|; where every rho is 65536, R_f = 1.0 exactly, the product is exact and the result is the
 *   call without the struct, bit for bit; a kind 1 target is honoured in the token's MEAN, before the clamp of g_f and before smoothing (both
 *   move it: a smoothed edge shares the ratio with the neighbours); what the clamp of r_t did is visible in applied.
 * Why Q16 ratios averaged linearly and not in the log domain: an integer sum has no order, so R_f has the same bits on any device and in the
 *   restatement; the arithmetic and the geometric mean of two neighbouring ratios a, b differ by the factor (a + b) / (2 sqrt(a b)), 0.9 % for
 *   1 next to 1.3 and 6 % for 1 next to 2, and only on the K frames of an edge.  Why the centre rule: a frame is decided by the samples about its centre, and it gives every frame at most one token.
 * Not built: token pitch on streams (sbv2_stream_*) and on sbv2_node_*, a per-token intonation scale, per-token duration edits, energy
 *   compensation. */
typedef struct sbv2_token_pitch {
    const double* value;      /* [n_tokens]: tokens of the rows in the order of req->utts, token order within a row (the order of sbv2_marks); 0 = token not edited */
    int64_t n_tokens;         /* must equal the sum of t_lens over the listed rows */
    int32_t kind;             /* 0 = value is a ratio in [0.5, 2]; 1 = value is the token's target mean f0 in Hz, in [f0_min / 2, 2 f0_max] */
    int32_t smooth;           /* K in [0, 20] contour frames to each side; taken as given, 0 = steps */
    double* applied;          /* out, NULL or [n_tokens]: the ratio used for the token (1.0 where not edited) */
    double* src_f0;           /* out, NULL or [n_tokens]: the token's measured mean f0 before any shift, 0 where it has no voiced frame */
    int64_t reserved;         /* must be 0 */
} sbv2_token_pitch;
/* sbv2_pipeline_fetch_request_dynamics with the listed rows' tokens edited.  token_pitch == NULL, or a value array of all zeros, is exactly that
 * call: no new launch, the same bytes (with all zeros applied is 1.0 and src_f0 is 0 throughout: nothing was measured).  Otherwise the rows
 * are shifted as sbv2_voice shifts them, with R_f in the target, also when voice is NULL or the identity (voice == NULL: p = s = 1 and the
 * voice's defaults); track then tracks the shifter's contour.  The token stage is one phase of the marks kernel: no further launch, no
 * atomics, no synchronisation beyond the fetch's one; applied and src_f0 reach pinned memory before it and the caller's arrays only after
 * everything else has succeeded.  The run's PCM is only read: two equal fetches give identical bytes and identical applied / src_f0.
 * Refused with nothing written: n_tokens different from the rows' token count, a NULL value (with n_tokens > 0), kind outside {0, 1}, smooth
 * outside [0, 20], a value that is negative, non-finite or outside the kind's range (0 excepted), a non-zero reserved, and everything that
 * call refuses. */
int sbv2_pipeline_fetch_request_token_pitch(sbv2_pipeline* p, int64_t ticket, const sbv2_fetch_request* req, const sbv2_voice* voice,
                                            const sbv2_pitch_track* track, const sbv2_dynamics* dynamics, const sbv2_token_pitch* token_pitch,
                                            void* dst, int64_t capacity_bytes, int64_t* out_count, double* stats, double* dyn_stats,
                                            sbv2_marks* marks, sbv2_pitch* pitch);
/* Test hook: sbv2_debug_voice_shift with a token table, always through the kernels (all zeros included).  tok_counts [nrows]: tokens of every
 * row; tok_ends [sum tok_counts]: the end position of every token in samples of its row, ascending within a row from 0 (token t owns
 * [end[t - 1], end[t]), the first from 0; arbitrary positions, also beyond the row: the hook needs no model); token_pitch as in the fetch, its
 * n_tokens = sum tok_counts.  Outputs besides sbv2_debug_voice_shift's: ratio_out [frames] = R_f (may be NULL), token_pitch->applied and
 * ->src_f0. */
int sbv2_debug_voice_tokens(int device, const float* x, const int64_t* lens, int nrows, int32_t sample_rate, const sbv2_voice* voice,
                            const double* period_in, const int32_t* voiced_in, const int64_t* tok_counts, const int64_t* tok_ends,
                            const sbv2_token_pitch* token_pitch, double* period_out, int32_t* voiced_out, int32_t* ta, int32_t* ts, int32_t* map,
                            int64_t* n_marks, float* y, double* ratio_out);

/* ---- new: formant scale.  TD-PSOLA keeps the spectral envelope: a voice raised by 1.3 is the same vocal tract at a higher pitch.  The perceived
 * size, age and character of a speaker sit in the formants; this moves them, by the factor q, and leaves f0 alone.  It is the shifter of
 * sbv2_voice with every grain READ at a scaled offset; everything up to and including the mapping m(j) is that section, unchanged.
 * Parameter: q = formant_scale in [0.5, 2]; 1 is the identity; anything else, a NaN included, is refused.
 * Voiced marks.  Analysis mark m is voiced iff frame ta_m / H (integer division) of the contour the marks were placed by (the given, the
 *   estimated or the tracked one) is voiced.
 * Output.  For synthesis mark j with a = ta_{m(j)}, L, R and the edge rule of sbv2_voice, every integer offset u = k - ts_j, in f64, never
 *   contracted: the read position p = q double(u); the window argument pw = p for a voiced mark and pw = double(u) for an unvoiced one; the
 *   grain contributes iff -L < pw < R; v = |pw| / (pw < 0 ? L : R), w = 1.0 - (v v) (3.0 - 2.0 v), and w = 1 on the left side of mark 0 and
 *   on the right side of the last mark, the side decided by the sign of pw; i0 = floor(p), fr = p - i0,
 *   val = (1.0 - fr) X(a + i0) + fr X(a + i0 + 1) with X = x inside [0, n) and 0 outside (64-bit indices); num += w val, den += w in
 *   ascending j; y[k] = float(num / max(den, 1.0)).  A row without an analysis mark is copied.
 * Why two window rules.  A voiced grain is the vocal tract's response to one pulse: compressing it together with its window is the classical
 *   grain resampling.  Unvoiced marks sit sr / 200 samples apart; compressed windows would no longer sum to 1 between them (den falls to 0.70
 *   at q = 1.2: a 200 Hz amplitude dip on every fricative), so an unvoiced grain keeps its complementary output-domain window (den = 1) and
 *   only its read index is scaled.
 * Hence: the length is unchanged; |y[k]| <= max |x| still holds, because val is a convex combination of two samples (or of a sample and 0):
 *   that is why the interpolation is linear and not cubic, the stage must stay unable to create clipping; with q = 1, fr = 0 and the result
 *   equals sbv2_voice's gather bit for bit; the marks, the contour, and applied / src_f0 of a token table are those of the call without; a
 *   voiced grain reaches |u| < max(L, R) / q, so the gather looks ceil(half / min(q, 1)) + 1 samples to each side of a tile for marks
 *   (half = max(tau_max + 1, sr / 200) + 2).
 * The level drops (RMS ratio 0.73 .. 0.91 on the synthetic vowel of tests/test_formant.py for q in 0.8 .. 1.3; the overlapping grains of noise
 *   are incoherent and lose level too): energy compensation stays not built, and the loudness stage behind restores level, as it does for pitch.
 * Not built: formant scale on streams (sbv2_stream_*) and on sbv2_node_*, a per-token or time-varying scale, energy compensation, an
 *   envelope-based (LPC / cepstral) shifter that would move single formants. */
typedef struct sbv2_formant {
    double formant_scale;     /* [0.5, 2]; 1 = the identity */
    double reserved;          /* must be 0 */
} sbv2_formant;
/* sbv2_pipeline_fetch_request_token_pitch with the listed rows' formants scaled.  formant == NULL, or formant_scale == 1, is exactly that call:
 * no new launch, the same bytes.  Otherwise the listed rows go through the shifter with k_voice_gather_fmt in place of its gather, also when
 * voice is NULL or the identity and no token is edited (voice == NULL: p = s = 1 and the voice's defaults); track then tracks the shifter's
 * contour.  Everything else (token table, compressor, gain stage, sink, stats, marks, pitch: all of the delivered signal) is that call, and
 * token_pitch's applied / src_f0 are those of the call without formant.  The run's PCM is only read: two equal fetches give identical bytes.
 * Refused with nothing written: a formant_scale outside [0.5, 2] or NaN, a non-zero reserved, and everything that call refuses. */
int sbv2_pipeline_fetch_request_formant(sbv2_pipeline* p, int64_t ticket, const sbv2_fetch_request* req, const sbv2_voice* voice,
                                        const sbv2_pitch_track* track, const sbv2_dynamics* dynamics, const sbv2_token_pitch* token_pitch,
                                        const sbv2_formant* formant, void* dst, int64_t capacity_bytes, int64_t* out_count, double* stats,
                                        double* dyn_stats, sbv2_marks* marks, sbv2_pitch* pitch);
/* Test hook: sbv2_debug_voice_shift with a formant scale, always through k_voice_gather_fmt (formant_scale = 1 included). */
int sbv2_debug_voice_formant(int device, const float* x, const int64_t* lens, int nrows, int32_t sample_rate, const sbv2_voice* voice,
                             const sbv2_formant* formant, const double* period_in, const int32_t* voiced_in, double* period_out,
                             int32_t* voiced_out, int32_t* ta, int32_t* ts, int32_t* map, int64_t* n_marks, float* y);

/* Test hook: the device limiter on host f64 signals (as sbv2_debug_loudness): out_x receives x (f64, laid out as the input), stats 6
 * doubles per signal. */
int sbv2_debug_limiter(int device, const double* x, const int64_t* lens, int nsig, int32_t sample_rate, const sbv2_limiter* lim,
                       double* out_x, double* stats);

/* ---- sbv2file.rs:15-37 `parse_sbv2file(bytes) -> (style_vectors, vits2)`: a .sbv2 file is zstd(tar{version.txt, model.onnx,
 * style_vectors.json}) (writer: scripts/convert/convert_model.py:156-175).  Both outputs are owned copies (sbv2_bytes_free).
 * Errors: "model not found: style_vectors" / "model not found: vits2" (Error::ModelNotFoundError, sbv2file.rs:31-36). ------------------- */
int sbv2_parse_sbv2file(const uint8_t* sbv2_bytes, size_t len, uint8_t** style_vectors, size_t* style_len, uint8_t** vits2, size_t* vits2_len);
void sbv2_bytes_free(uint8_t* p);
/* style.rs:11-17 `load_style`: {"shape": [n, dim], "data": [[..], ..]} -> owned f32 [n][dim] (release with sbv2_bytes_free) */
int sbv2_style_load(const uint8_t* json, size_t len, float** data, int64_t* n, int64_t* dim);
/* tts.rs:84-124 `load_aivmx` (cargo feature "aivmx"): the bytes are the VITS ONNX model itself (hand them to sbv2_vits_create); the style
 * table is ModelProto.metadata_props["aivm_style_vectors"] = base64(.npy, 2-D float32, C or Fortran order) -> owned f32 [n][dim]
 * (sbv2_bytes_free).  Errors: key absent; not 2-D ("expected 2D array", the reference's panic); not float32. */
int sbv2_aivmx_style_vectors(const uint8_t* aivmx_bytes, size_t len, float** data, int64_t* n, int64_t* dim);
/* style.rs:19-28 `get_style_vector`: out[dim] = mean + (style_vectors[style_id] - mean) * weight, mean = row 0 */
int sbv2_style_vector(const float* style_vectors, int64_t n, int64_t dim, int64_t style_id, float weight, float* out);

/* ---- new: multi-GPU.  The reference is one process, one device, batch 1; a batch of independent utterances is
 * sharded over the GPUs of a node (sorted by cost, longest-processing-time-first deal, a full weight replica per GPU, no data-path
 * collective) and the PCM is gathered to rank 0 over RCCL / xGMI (one all-gather of the sample counts + grouped send / recv).
 * RCCL is dlopen'ed on first use: single-GPU callers never load it. ------------------------------------------------------------------ */
/* rank_of[i] = rank that synthesises utterance i (host only, deterministic on every rank). */
int sbv2_deal(int64_t n, const int64_t* costs, int world, int32_t* rank_of);
/* Host only: the gather of a dealt batch.  Rank r's message is the PCM of its utterances in ascending caller index; the messages sit in
   rank order in the root's staging buffer.  counts[world] = samples per rank, table[3 n] = {offset in the staging buffer, offset in the
   caller's utterance order, samples} per utterance (the permutation sbv2_node_synthesize applies on the device). */
int sbv2_gather_plan(int64_t n, const int64_t* pcm_lens, const int32_t* rank_of, int world, int64_t* counts, int64_t* table);

/* (a) one process per GPU: rank 0 obtains a 128-byte id (ncclGetUniqueId) and hands it to the other ranks by any side channel. */
typedef struct sbv2_comm sbv2_comm;
int sbv2_comm_unique_id(uint8_t* id128);
int sbv2_comm_create(const uint8_t* id128, int rank, int world, int device, sbv2_comm** out);
void sbv2_comm_destroy(sbv2_comm* c);
int sbv2_comm_rank(const sbv2_comm* c);
int sbv2_comm_world(const sbv2_comm* c);
int sbv2_comm_barrier(sbv2_comm* c);
int sbv2_comm_max_f64(sbv2_comm* c, double* v);   /* in place: max over ranks (also a barrier) */
/* PCM of the run `ticket` of this rank's pipeline -> root: counts[world] = samples per rank (filled on every rank); on the root
 * dst_host (capacity samples; may be sbv2_host_alloc memory) receives the ranks' PCM concatenated in rank order. */
int sbv2_comm_gather_pcm(sbv2_comm* c, sbv2_pipeline* p, int64_t ticket, int root, float* dst_host, int64_t capacity, int64_t* counts);

/* (b) one process, N devices: the batched multi-GPU entry SURVEY.md §8b calls `sbv2_synthesize_batch`.  devices[ndev] are HIP ordinals (the model bytes are
 * the ones sbv2_bert_create / sbv2_vits_create take); one host thread + stream set per device, ncclCommInitAll when ndev > 1. */
typedef struct sbv2_node sbv2_node;
int sbv2_node_create(const uint8_t* bert_model, size_t bert_len, const uint8_t* vits_model, size_t vits_len, const int* devices, int ndev,
                     sbv2_node** out);
void sbv2_node_destroy(sbv2_node* nd);
int sbv2_node_devices(const sbv2_node* nd);
int sbv2_node_uses_rccl(const sbv2_node* nd);
/* Same inputs as sbv2_pipeline_run.  Outputs: pcm_lens[n]; pcm_host = the batch's PCM concatenated in the CALLER's utterance order
 * (capacity samples).  Utterance i's samples equal what a one-GPU call of the whole batch returns for it, bit for bit. */
int sbv2_node_synthesize(sbv2_node* nd, const sbv2_batch* batch, const int64_t* token_ids, const int64_t* s_lens, const int64_t* word2ph,
                         int64_t* pcm_lens, float* pcm_host, int64_t capacity);
int sbv2_node_last_deal(const sbv2_node* nd, int32_t* rank_of, int64_t n);   /* which device ran which utterance in the last call */

/* ---- new: streaming long-form synthesis (BASELINE configs[4]).  The reference synthesises one sentence per session.run and only splits
 * long text on '\n' (tts.rs:290-321).  Here DeBERTa / text encoder / durations / flow run whole-sequence (global attention) and the HiFi-GAN
 * decoder runs on fixed windows of chunk_frames + 2 x 16 halo frames, ONE hipGraph captured per window shape and replayed per chunk;
 * chunked output equals the whole-sequence output (the halo covers the generator's 13.4-frame receptive field per side). ------------- */
typedef struct sbv2_stream sbv2_stream;
/* batch->n must be 1; inputs as for sbv2_pipeline_run.  *total_samples = samples of the whole utterance.  The handles are busy until _end. */
int sbv2_stream_begin(sbv2_bert* bert, sbv2_vits* vits, const sbv2_batch* batch, const int64_t* token_ids, const int64_t* s_lens,
                      const int64_t* word2ph, int64_t chunk_frames, sbv2_stream** out, int64_t* total_samples);
/* next chunk -> dst (host; capacity samples, chunk_frames * hop always suffices); *n = samples written, 0 at the end */
int sbv2_stream_next(sbv2_stream* s, float* dst, int64_t capacity, int64_t* n);
/* Streaming with an output format (see sbv2_pcm_format): inputs as sbv2_stream_begin; *total_samples at fmt->sample_rate; fmt->normalize must be 0
 * (a stream cannot know the peak ahead).  Chunk c of native samples [a, b) emits output samples [ceil(a L / M), ceil(b L / M)), so the chunks
 * concatenate to the formatted whole utterance.  sbv2_stream_next is refused on such a stream, sbv2_stream_next_format on any other.  There is
 * no loudness (sbv2_loudness) on a stream either: integrated loudness needs the whole signal. */
int sbv2_stream_begin_format(sbv2_bert* bert, sbv2_vits* vits, const sbv2_batch* batch, const int64_t* token_ids, const int64_t* s_lens,
                             const int64_t* word2ph, int64_t chunk_frames, const sbv2_pcm_format* fmt, sbv2_stream** out, int64_t* total_samples);
/* next chunk -> dst (host; capacity_bytes); *n = samples written, 0 at the end */
int sbv2_stream_next_format(sbv2_stream* s, void* dst, int64_t capacity_bytes, int64_t* n);
/* ---- new: the stream as FLAC.  Inputs as sbv2_stream_begin_format; fmt->encoding must be 1 (s16), fmt->normalize 0; *total_samples at
 * fmt->sample_rate.  The s16 samples that sbv2_stream_next_format would deliver are encoded on the device instead, replay by replay, as ONE
 * FLAC stream in the convention of sbv2_pipeline_fetch_flac (mono, 16 bits, fixed 4096-sample blocks, frames numbered from 0); the samples
 * that do not fill a block yet are carried on the device to the next chunk.  Call c of sbv2_stream_next_flac consumes the samples of chunk c
 * (*n_samples; 0 once the utterance is complete) and writes into HOST memory dst the bytes of every frame those samples complete (*n_bytes,
 * which may be 0 while *n_samples > 0); the first call starts with the 42-byte stream header, whose STREAMINFO names total_samples and
 * min / max frame size 0 (unknown, RFC 9639 8.2), the last one that consumes samples ends with the short final frame.  The concatenated
 * output equals sbv2_debug_flac_encode of the stream's samples in every byte except stream bytes 12..17 (min / max frame size).  A
 * capacity_bytes that does not hold the call's bytes is refused with nothing written and nothing consumed: repeat the call with more room.
 * sbv2_stream_next and sbv2_stream_next_format are refused on such a stream, sbv2_stream_next_flac on any other. */
/* Host only: a capacity that always suffices for one call, 42 + 16 ceil((n + 4095) / 4096) + 2 (n + 4095) with
 * n = sbv2_pcm_format_length(fmt, chunk_native_samples), chunk_native_samples = chunk_frames * sbv2_vits_hop; -1 for a bad fmt. */
int64_t sbv2_flac_stream_bound(const sbv2_pcm_format* fmt, int64_t chunk_native_samples);
int sbv2_stream_begin_flac(sbv2_bert* bert, sbv2_vits* vits, const sbv2_batch* batch, const int64_t* token_ids, const int64_t* s_lens,
                           const int64_t* word2ph, int64_t chunk_frames, const sbv2_pcm_format* fmt, sbv2_stream** out, int64_t* total_samples);
int sbv2_stream_next_flac(sbv2_stream* s, uint8_t* dst, int64_t capacity_bytes, int64_t* n_bytes, int64_t* n_samples);
/* Test hook: the fed encoder on its own.  x[n] (host s16) is cut at the ascending sample positions cuts[ncuts] into ncuts + 1 pushes (empty
 * ones allowed, the last one ends the stream); dst receives the pushes' bytes back to back, out_bytes_per_push[ncuts + 1] their sizes. */
int sbv2_debug_flac_stream_encode(int device, const int16_t* x, int64_t n, const int64_t* cuts, int ncuts, int32_t sample_rate, uint8_t* dst,
                                  int64_t capacity, int64_t* out_bytes_per_push);
/* ---- new: level control on a stream: a fixed gain and the look-ahead limiter of sbv2_limiter, carried from chunk to chunk ON THE DEVICE.
 * Step 3 of sbv2_limiter, the make-up loop, needs the whole signal; step 2, its gain curve for a pre-gain named ahead, does not.  For the whole
 * delivered signal y of the stream (resampled to fs, f64, before any cast or quantiser), g0 = 10^(gain_db / 20), c = 10^(ceiling / 20),
 * K = fs div 100:  x = y g0 s, with e, r, m and s exactly those of sbv2_limiter step 2 at that g0, the onset rule (m = m[0] before the start),
 * the end rule (r = 1 past the end), s = min(sum, r) and the clamp of x to [-c, c] included.  So |x[n]| <= c for every sample and s16 cannot
 * clip, whatever the gain.  There is no make-up loop and no max_reduction: the depth is whatever the signal needs at that gain, and it is
 * reported (sbv2_stream_level_stats), not bounded.  There is no idle rule either: a stream whose r is 1 throughout still delivers
 * y g0 min(sum of the K taps over ones, 1), which may differ from y g0 in the last bit.  The gain is the caller's: for a consistent level,
 * target - L from the loudness stats of any /synthesize answer of the same voice.
 * Look-ahead: t[o], the interpolated magnitude behind e, reads y[o - 11 .. o + 12]; r[p] reads t[p - 1 .. p]; m[j] reads r[j .. j + K - 1];
 * s[n] reads m[n - K + 1 .. n].  Sample n of x therefore depends on y[n - K - 11 .. n + K + 11] and on nothing else, and is final once
 * A = K - 1 + 12 samples follow it (91 at 8 kHz, 452 at 44.1 kHz, 491 at 48 kHz).
 * Delivery rule: after chunks of S samples in all have been taken and the utterance has not ended, exactly max(0, S - A) samples of x have
 * been delivered; the call that takes the last chunk delivers all the rest.  Time is not shifted: sample j of the output is sample j of the
 * utterance (sbv2_stream_marks stays valid as it is); only delivery runs A samples late.  x does not depend on the chunk size: bit for bit
 * the samples sbv2_debug_limiter_fixed gives for the whole y. */
typedef struct sbv2_stream_level {
    double gain_db;              /* [-40, 40]; g0 = 10^(gain_db / 20) */
    double true_peak_max_dbtp;   /* [-20, 0];  c = 10^(ceiling / 20) */
    double reserved[2];          /* must be 0 */
} sbv2_stream_level;
/* Host only: A at fmt->sample_rate; -1 for a bad fmt.  A depends on the rate alone and this query takes encodings 0 and 1 only, as it
 * always did: for a G.711 level stream ask with either at the same rate. */
int64_t sbv2_stream_level_lookahead(const sbv2_pcm_format* fmt);
/* Host only: bytes that always suffice for one sbv2_stream_next_level call of a stream with chunks of chunk_native_samples (chunk_frames * hop):
 * n = sbv2_pcm_format_length of the chunk + A samples, as n * bytes per sample, or with flac != 0 (fmt s16) the bound of sbv2_flac_stream_bound
 * for a push of n samples.  -1 for a bad fmt. */
int64_t sbv2_stream_level_bound(const sbv2_pcm_format* fmt, int64_t chunk_native_samples, int flac);
/* Inputs as sbv2_stream_begin_format; fmt must not be NULL, fmt->normalize must be 0, any encoding; flac != 0 needs s16 and encodes the delivered
 * s16 samples as ONE FLAC stream, as sbv2_stream_begin_flac does.  A NULL level, out-of-range or non-finite fields and non-zero reserved
 * fields are refused.  *total_samples at fmt->sample_rate: the same total as without a level.
 * G.711 (encoding 7 / 6): the guarantee holds BEFORE the quantiser: no sample of x above the ceiling, and the codes are enc(the s16 level
 * stream's samples).  The laws then saturate on their own: mu-law above 32635 / 32767 (-0.035 dBFS), A-law at its top level (q >= 31744 or
 * q <= -31745). */
int sbv2_stream_begin_level(sbv2_bert* bert, sbv2_vits* vits, const sbv2_batch* batch, const int64_t* token_ids, const int64_t* s_lens,
                            const int64_t* word2ph, int64_t chunk_frames, const sbv2_pcm_format* fmt, const sbv2_stream_level* level, int flac,
                            sbv2_stream** out, int64_t* total_samples);
/* Takes the next chunk.  *n_consumed = the chunk's samples at fmt->sample_rate (those sbv2_stream_next_format would have written), 0 once the
 * utterance is complete: the end signal.  *n_out = samples of x written to dst in fmt's encoding by the delivery rule, or for a FLAC stream
 * the bytes of the frames those samples complete (the 42-byte header in front on the first call); *n_out may be 0 while *n_consumed > 0 (a
 * 16-frame chunk of a decoder with hop 16 is 256 samples at 44.1 kHz, A is 452).  Too small a capacity is refused with nothing written and
 * nothing consumed: the call can be repeated (sbv2_stream_level_bound always suffices).  The other three sbv2_stream_next* calls are refused on
 * a level stream, this one on any other stream. */
int sbv2_stream_next_level(sbv2_stream* s, void* dst, int64_t capacity_bytes, int64_t* n_out, int64_t* n_consumed);
/* stats[0] = 20 log10 min s, the deepest reduction over the utterance in dB (<= 0); stats[1] = max |x| before the cast / quantiser (<= c).
 * Kept on the device across the chunks (min and max are exact: the values do not depend on the chunk size), read once here.  Refused before
 * the stream is complete (sbv2_stream_next_level has answered *n_consumed = 0, or has taken the last chunk). */
int sbv2_stream_level_stats(sbv2_stream* s, double* stats);
/* Test hook: step 2 at the fixed gain of `level`, in one shot, on host f64 signals (layout as sbv2_debug_limiter) -> out_x, stats 2 doubles per
 * signal as sbv2_stream_level_stats.  The yardstick of the streamed path. */
int sbv2_debug_limiter_fixed(int device, const double* x, const int64_t* lens, int nsig, int32_t sample_rate, const sbv2_stream_level* level,
                             double* out_x, double* stats);
/* Test hook: the same limiter fed piece by piece: the n samples of x cut at the ascending positions cuts[ncuts] into ncuts + 1 pushes (empty
 * ones allowed, the last one ends the stream); out_x receives the pushes' samples back to back (n in all), out_per_push[ncuts + 1] their
 * counts (the delivery rule), stats the 2 doubles.  level, rate and cuts are checked before any device call. */
int sbv2_debug_limiter_stream(int device, const double* x, int64_t n, const int64_t* cuts, int ncuts, int32_t sample_rate,
                              const sbv2_stream_level* level, double* out_x, int64_t* out_per_push, double* stats);
/* Test hooks: what every launch of the meter / of the fixed-gain limiter leaves on the device, on host f64 signals laid out as for
 * sbv2_debug_loudness.  On the device the packed input lies between NaN words (a read outside [0, total) poisons a result) and every array
 * returned is pre-filled with the byte 0x5A (a slot no launch wrote still holds 0x5A5A5A5A5A5A5A5A); the meter / limiter runs as it is.
 * Refused without writing anything: an unsupported rate, a bad level, a negative length, a NULL output, too small a capacity.
 * sbv2_debug_loudness_parts (measure only): stats [nsig][3]; e and st [nseg][4] (zero-start end state and true start state of every
 * K-weighting segment), part [nseg] (its sum of w^2), nseg <= cap_seg; bmax [ceil(total / 256)] <= cap_blk (the true-peak workgroups' maxima,
 * 0 for one that straddles signals); peak [nsig] (the atomic maxima of the straddling workgroups, as doubles); taps [3][24] (the
 * interpolator's phases 1..3 as the kernels get them); counts[4] = the segment length m, nseg, workgroups, pad words behind the arrays that a
 * launch changed.
 * sbv2_debug_limiter_parts: out_t and out_x [total] (the interpolated magnitudes and the limited signal), smin [tiles] <= cap_tiles (min s of
 * every 1024-sample tile), taps [K] and *hsum (the Hann taps and their sum as uploaded); counts[3] = K, tiles, pad words changed. */
int sbv2_debug_loudness_parts(int device, const double* x, const int64_t* lens, int nsig, int32_t sample_rate, double* stats, int64_t cap_seg,
                              int64_t cap_blk, double* e, double* st, double* part, double* bmax, double* peak, double* taps, int64_t* counts);
int sbv2_debug_limiter_parts(int device, const double* x, const int64_t* lens, int nsig, int32_t sample_rate, const sbv2_stream_level* level,
                             int64_t cap_tiles, double* out_t, double* out_x, double* smin, double* taps, double* hsum, int64_t* counts);
/* ---- new: speech marks of a stream.  Host only, valid from sbv2_stream_begin* onwards: the token spans (see sbv2_marks) of the stream's one
 * utterance at place 0 (a request stream, sbv2_stream_begin_request: of all its rows, row i at place[i], row order then token order) and at
 * the stream's delivered rate (native for sbv2_stream_begin).  Every duration is known before the first replay, so
 * the client has the full timing before the first audio byte; the samples of all chunks sum to the last token's end (durations summing to >= 1).
 * Levels and the envelope of a stream come from sbv2_stream_begin_request_levels / sbv2_stream_next_marks below (partial sums carried across
 * the chunks on the device); this call stays host arithmetic and is the same on every stream.  Refused: capacity below the token count. */
int sbv2_stream_marks(sbv2_stream* s, int64_t* tok_start, int64_t* tok_end, int64_t capacity, int64_t* n_tokens);
/* ---- new: a stream over the n rows of ONE batched forward: a multi-sentence request as one signal, sentence by sentence.
 * Forward.  batch->n >= 1 rows run through one forward with the decoder left out: the forward sbv2_pipeline_run_opts runs for that batch and
 *   opts (which may be NULL), so durations and noise keys are those of the run.
 * Timeline.  With len[i] the native (44.1 kHz) samples of row i: place[0] = 0, place[i + 1] = place[i] + len[i] + gap_after[i],
 *   joined_len = place[n - 1] + len[n - 1] + gap_after[n - 1]; *total_samples = J(joined_len), J(a) = ceil(a L / M) at the stream's rate.
 * Output.  The concatenation of everything the stream delivers is the signal sbv2_pipeline_fetch_pcm_format(..., place, joined_len, ...)
 *   delivers for a pipeline run of the same batch and options in the same format; with flac its s16 samples as one FLAC stream in the
 *   convention of sbv2_stream_begin_flac; with level the x of sbv2_stream_level for the whole joined y.
 * Calls.  Row i is cut on its own frame grid into ceil(frames[i] / chunk_frames) chunks (a gap is no multiple of the hop: there is no joined
 *   frame grid); the stream's calls are those chunks in row order, then chunk order.  With m_i = place[i] + len[i] + gap_after[i] / 2 (integer
 *   division) for i < n - 1, m_{-1} = 0 and m_{n-1} = joined_len, the call for chunk [a, b) (native positions of the timeline) of row i delivers
 *   the output samples [J(a'), J(b')): a' = m_{i-1} for the row's first chunk, else a; b' = m_i for its last chunk, else b.  The calls tile
 *   [0, J(joined_len)): each gap leaves half with the sentence before it and half with the one after it, trailing silence with the last call.
 * Minimum gap.  For i < n - 1, gap_after[i] >= 2 ceil(half / L) of the format (sbv2_stream_min_gap): 354 at 8 kHz, 178 at 16 kHz, 128 at
 *   22.05 kHz, 118 at 24 kHz, 90 at 32 kHz, 64 at 48 kHz, 0 at 44.1 kHz (sentences may abut).  Then no output sample on one side of m_i has a
 *   filter tap on the other side's sentence, and every call needs its own window's PCM only.  A shorter gap is refused with the minimum named;
 *   every gap_after[i] must lie in [0, 441000] (10 s).  The halo check of sbv2_stream_begin_format (reach <= exact) stays as it is: the
 *   exact part of the halo grows with the hop, so the full-size model (hop 512) streams 16 kHz and 8 kHz, and only a model with a small hop
 *   (the tiny test models, hop 16) is refused 16 kHz by it.
 * Taking chunks.  A request stream is always a formatted stream, also at the identity format: sbv2_stream_next_format, or sbv2_stream_next_flac
 *   with flac, or sbv2_stream_next_level with level; sbv2_stream_next is refused.  n_consumed / n_samples of call c = call_samples[c] of
 *   sbv2_stream_timeline; the end marker and "too small a buffer: nothing written, nothing consumed, repeat" are those of the single-utterance
 *   streams.  sbv2_stream_marks gives the tokens of all rows, row order then token order, row i at place[i]: the spans of
 *   sbv2_pipeline_fetch_request_marks for the joined fetch; the silence belongs to no token.
 * Refused before any GPU work: NULL rq or gap_after, n < 1, a gap out of range or below the minimum, a non-zero reserved, normalize, flac without
 *   s16, and whatever the options, the format and the level are refused for elsewhere.
 * Not built: gaps below the minimum at resampled rates (they would need a call to see two windows), sbv2_node_*.  Levels and an envelope:
 *   sbv2_stream_begin_request_levels below; a loudness target: sbv2_stream_begin_request_leveler below.  The four calls above are the n = 1,
 *   gap_after = {0} case of the same code and keep their bytes. */
typedef struct sbv2_stream_request {
    const int64_t* gap_after;         /* [batch->n] native (44.1 kHz) samples of silence after row i; the last entry is trailing silence */
    const sbv2_pcm_format* fmt;       /* NULL = 44100 Hz f32, not normalised (the identity format) */
    const sbv2_stream_level* level;   /* NULL = none */
    int32_t flac;                     /* 1 = one FLAC stream (fmt s16) */
    int32_t reserved;                 /* must be 0 */
} sbv2_stream_request;
int sbv2_stream_begin_request(sbv2_bert* bert, sbv2_vits* vits, const sbv2_batch* batch, const sbv2_utt_options* opts /* may be NULL */,
                              const int64_t* token_ids, const int64_t* s_lens, const int64_t* word2ph, int64_t chunk_frames,
                              const sbv2_stream_request* rq, sbv2_stream** out, int64_t* total_samples);
/* ---- new: the levels and the envelope of a stream's marks, reduced chunk by chunk ON THE DEVICE.
 * sbv2_stream_begin_request with, besides, a level reduction of the DELIVERED samples behind every decoder replay: sumsq / peak (see sbv2_marks:
 *   the same values of the same samples, "exactly what crosses PCIe or enters the FLAC encoder", G.711 codes as the integers they decode to) per
 *   token span of sbv2_stream_marks (tokens = 1) and / or per envelope frame [f env_hop, min((f + 1) env_hop, total_samples)) (env_hop > 0,
 *   *n_env = ceil(total_samples / env_hop) frames).  On a level stream (rq->level) the samples are those the limiter emits, at their own
 *   positions: time is not shifted, delivery only runs A samples late.
 * Bits.  A segment's sum is formed in the order of the one-shot reduction (sbv2_debug_segment_levels, sbv2_pipeline_fetch_request_marks): lane
 *   o mod stride adds offset o, stride by the segment's total length; a segment open at a replay's end keeps its lanes' partial sums on the
 *   device (16 KB in all, whatever the stream's length).  So the values do not depend on chunk_frames, and where the stream's bytes equal a
 *   fetch's (sbv2_stream_begin_request, "Output") they equal the fetch's marks bit for bit.  No sample is read more often than in the fetch.
 * lv == NULL, or tokens == 0 and env_hop == 0: exactly sbv2_stream_begin_request (*n_tokens = *n_env = 0, no new launch, sbv2_stream_next_marks
 *   refused).  Otherwise the stream is taken with the sbv2_stream_next_* call of its kind, unchanged, its audio bytes are those of the same
 *   stream without levels, and it delivers in order only.  The single-utterance streams are the n = 1, gap_after = {0} case.
 * Refused before any GPU work: a non-zero reserved, tokens outside {0, 1}, a negative env_hop (these three before the handles are looked at),
 *   and everything sbv2_stream_begin_request refuses.  n_env >= 2^30 is refused once the forward has named the length
 *   (with predicted durations nothing names it earlier), before the stream has set up anything: no replay, no buffer, no level work.
 * Not built: levels on the plain sbv2_stream_begin stream (begin a request stream with fmt NULL, the identity format, instead), sbv2_node_*. */
typedef struct sbv2_stream_levels {
    int32_t tokens;        /* 0 / 1: levels per token */
    int32_t env_hop;       /* 0 = no envelope, else delivered samples per frame */
    int32_t reserved[2];   /* must be 0 */
} sbv2_stream_levels;
int sbv2_stream_begin_request_levels(sbv2_bert* bert, sbv2_vits* vits, const sbv2_batch* batch, const sbv2_utt_options* opts /* may be NULL */,
                                     const int64_t* token_ids, const int64_t* s_lens, const int64_t* word2ph, int64_t chunk_frames,
                                     const sbv2_stream_request* rq, const sbv2_stream_levels* lv, sbv2_stream** out, int64_t* total_samples,
                                     int64_t* n_tokens, int64_t* n_env);
/* Host only: the entries completed since the previous call.  With D the samples the stream has delivered or consumed so far (the sum of *n of
 * sbv2_stream_next_format, of *n_samples of sbv2_stream_next_flac; on a level stream the samples EMITTED by its delivery rule, max(0, S - A),
 * and everything with the last chunk): token t is complete once end[t] <= D, frame f once min((f + 1) env_hop, total) <= D; after the last
 * chunk everything is.  A call hands out the contiguous ranges [tok_first, tok_first + n_tok) (numbering of sbv2_stream_marks) and
 * [env_first, env_first + n_env) that became complete since the previous call, and delivered = D.  A capacity below the pending entries, or
 * NULL arrays with entries pending, is refused with nothing handed out: repeat with more room.  Not calling it loses nothing: the next call
 * returns everything pending.  Refused on a stream begun without levels. */
typedef struct sbv2_stream_marks_part {
    int64_t tok_capacity; double* tok_sumsq; double* tok_peak; int64_t tok_first, n_tok;
    int64_t env_capacity; double* env_sumsq; double* env_peak; int64_t env_first, n_env;
    int64_t delivered;
} sbv2_stream_marks_part;
int sbv2_stream_next_marks(sbv2_stream* s, sbv2_stream_marks_part* part);
/* ---- new: the pitch contour of a stream, estimated chunk by chunk ON THE DEVICE.
 * sbv2_stream_begin_request_levels with, besides, the contour of sbv2_pitch over the DELIVERED samples of the stream (the samples the levels
 *   are taken of; on a level stream those the limiter emits), by sbv2_pitch's convention unchanged: the rate is the format's (fmt NULL = the
 *   identity format, 44100 Hz), frame f has its centre at f hop + hop / 2 and its window [centre - tau_max, centre + tau_max), positions outside
 *   [0, total_samples) read as 0, *n_pitch = ceil(total_samples / hop).
 * Completion.  Frame f is complete once min(f hop + hop / 2 + tau_max, total_samples) <= D, D as for sbv2_stream_next_marks (delivered or
 *   consumed samples; emitted ones on a level stream): frames complete in order and about tau_max samples late, everything with the last chunk.
 * Bits.  The device keeps the last 2 tau_max delivered samples from replay to replay (19 KB in all, whatever the stream's length); a frame's
 *   window is staged from them and from the replay's samples and then takes the one-shot kernel's own per-frame arithmetic.  So lag, ap and f0
 *   equal sbv2_debug_pitch / sbv2_pipeline_fetch_request_pitch over the same samples bit for bit, for every encoding, f32 included, whatever
 *   chunk_frames is.  One launch and one device-to-host copy more per replay.
 * sp == NULL: exactly sbv2_stream_begin_request_levels (*n_pitch = 0, sbv2_stream_next_pitch refused).  Pitch may be on without levels (lv NULL)
 *   and levels without pitch.  With pitch the audio bytes, sbv2_stream_marks and sbv2_stream_next_marks are those of the same stream without,
 *   and the stream delivers in order only.
 * Refused before the handles are looked at: a non-zero reserved and everything sbv2_pitch's parameters refuse at the format's rate (so rates
 *   above 48000 Hz); besides, everything sbv2_stream_begin_request_levels refuses.  n_pitch >= 2^30 is refused where n_env >= 2^30 is.
 * Not built: pitch on the plain sbv2_stream_begin stream (begin a request stream with fmt NULL instead), sbv2_node_*, smoothing across frames. */
typedef struct sbv2_stream_pitch {
    int32_t hop; int32_t reserved;        /* delivered samples per frame (>= 1); reserved must be 0 */
    double f0_min, f0_max, threshold;     /* Hz, Hz, (0, 1); usual values 70, 600, 0.15 */
} sbv2_stream_pitch;
int sbv2_stream_begin_request_pitch(sbv2_bert* bert, sbv2_vits* vits, const sbv2_batch* batch, const sbv2_utt_options* opts /* may be NULL */,
                                    const int64_t* token_ids, const int64_t* s_lens, const int64_t* word2ph, int64_t chunk_frames,
                                    const sbv2_stream_request* rq, const sbv2_stream_levels* lv /* may be NULL */,
                                    const sbv2_stream_pitch* sp /* may be NULL */, sbv2_stream** out, int64_t* total_samples, int64_t* n_tokens,
                                    int64_t* n_env, int64_t* n_pitch);
/* Host only: the frames [first, first + n) that became complete since the previous call, f0 / ap / lag as sbv2_pitch gives them (ap and lag may
 * be NULL), and delivered = D.  A capacity below the pending frames, or a NULL f0 with frames pending, is refused with nothing written and
 * nothing lost: repeat with more room.  Not calling it loses nothing.  Refused on a stream begun without pitch. */
typedef struct sbv2_stream_pitch_part {
    int64_t capacity; double* f0; double* ap; int32_t* lag; int64_t first, n;
    int64_t delivered;
} sbv2_stream_pitch_part;
int sbv2_stream_next_pitch(sbv2_stream* s, sbv2_stream_pitch_part* part);
/* Test hook: the fed estimator on its own.  x[n] (host; encoding and pitch as sbv2_debug_pitch) is cut at the ascending positions cuts[ncuts]
 * into ncuts + 1 pushes (empty ones allowed), each handed a copy of its own samples only; outputs as sbv2_debug_pitch, and per_push [ncuts + 1]
 * the frames each push completed.  Parameters, capacity and cuts are checked before any device call. */
int sbv2_debug_stream_pitch(int device, const void* x, int encoding, int64_t n, const int64_t* cuts, int ncuts, int32_t sample_rate, sbv2_pitch* pitch,
                            double* cmnd3, int32_t* voiced, int64_t* per_push);
/* Test hook: the fed reduction on its own.  x[n] (host; encoding as sbv2_debug_segment_levels) is cut at the ascending positions cuts[ncuts] into
 * ncuts + 1 pushes (empty ones allowed); segments [starts[i], ends[i]) must be monotone and disjoint within [0, n] (empty ones and holes allowed),
 * env_hop as above (0 = none).  seg_* [nseg] and env_* [ceil(n / env_hop)] receive the results, seg_per_push / env_per_push [ncuts + 1] the
 * entries each push completed.  Segments, env_hop and cuts are checked before any device call. */
int sbv2_debug_stream_levels(int device, const void* x, int encoding, int64_t n, const int64_t* cuts, int ncuts, const int64_t* starts,
                             const int64_t* ends, int64_t nseg, int32_t env_hop, double* seg_sumsq, double* seg_peak, double* env_sumsq,
                             double* env_peak, int64_t* seg_per_push, int64_t* env_per_push);
/* Host only: the minimum gap above in native samples (fmt NULL = the identity format = 0); -1 for a bad fmt. */
int64_t sbv2_stream_min_gap(const sbv2_pcm_format* fmt);
/* Host only: the arithmetic above in one place (the library calls it itself).  frames[n] = the rows' lengths in frames (>= 1), hop =
 * sbv2_vits_hop, fmt NULL = the identity format.  Outputs (each may be NULL): place[n], *joined_len, call_samples[c] = the samples call c covers
 * (a level stream DELIVERS them by its delivery rule, A samples late), *n_calls (also written when capacity is refused).  Refused: what
 * sbv2_stream_begin_request refuses in the gaps, n < 1, a row without frames, hop or chunk_frames < 1, capacity < n_calls with call_samples given. */
int sbv2_stream_timeline(const int64_t* frames, const int64_t* gap_after, int64_t n, int32_t hop, int64_t chunk_frames, const sbv2_pcm_format* fmt,
                         int64_t* place, int64_t* joined_len, int64_t* call_samples, int64_t capacity, int64_t* n_calls);
/* Host only, valid from any sbv2_stream_begin* onwards: the rows' placement and native lengths (capacity entries each; either may be NULL), *n
 * rows, *joined_len. */
int sbv2_stream_layout(const sbv2_stream* s, int64_t* place, int64_t* pcm_lens, int64_t capacity, int64_t* n, int64_t* joined_len);
/* Host only: bytes that suffice for any sbv2_stream_next* call of THIS stream: its largest call, plus A samples with a level, or the FLAC push
 * bound of that many samples.  (sbv2_flac_stream_bound / sbv2_stream_level_bound bound a plain chunk, not a call that carries half a gap.) */
int64_t sbv2_stream_call_bound(const sbv2_stream* s);
int sbv2_stream_uses_graph(const sbv2_stream* s);
int64_t sbv2_stream_workspace_bytes(const sbv2_stream* s);
void sbv2_stream_end(sbv2_stream* s);

/* ---- new: assist text.  Steer HOW a sentence is spoken with a second text ("I am so happy!"): upstream Style-Bert-VITS2's assist_text /
 * assist_text_weight.  The second text goes through the same DeBERTa; the mean of its hidden states over its tokens is mixed into every
 * token's feature of the spoken text before the word2ph repeat: res[i] * (1 - w) + style_res_mean * w.  It is the one inference knob that acts
 * BEFORE the model; durations, PCM, every fetch, sink, mark, voice edit and stream work unchanged on what an assisted run produces.
 * A run of n rows also carries A >= 1 assist sequences of token ids, each of its own length S_a >= 1 with the limits of a sequence of
 *   sbv2_pipeline_run (1 <= S_a < 2^20, ids inside the vocabulary).  Row u names one of them, text_of[u] in [0, A), or none (-1), and carries a
 *   weight w_u, a double in [0, 1].  An assist text that no row names is allowed (a caller may hand in a deduplicated table); it is still run.
 * Forward.  ONE DeBERTa forward over the n sequences of the batch followed by the A assist sequences (n + A rows); the packed layout puts the
 *   batch's rows where they are without an assist.  F[c][q] below is that forward's output plane (channel-major), s_a the first column of
 *   assist sequence a in it.
 * Mean of assist sequence a (k_assist_mean, one 64-lane wavefront per (a, channel c), no atomics), over ALL S_a columns, [CLS] and [SEP]
 *   included, as upstream's mean(0): lane l adds double(F[c][s_a + i]) for i = l, l + 64, l + 128, ... < S_a in ascending i, in f64, starting
 *   from 0.0; then the lanes are folded pairwise, for h = 32, 16, 8, 4, 2, 1 in that order: acc[l] = acc[l] + acc[l + h] for every l < h;
 *   mean_a[c] = float(acc[0] / double(S_a)).  The result depends on nothing but that sequence's own columns.
 * Blend, fused into the word2ph gather (k_gather_cols_assist in place of the plain gather).  For text column t of row u with source column
 *   q = map[t]: wf = float(w_u), omw = float(1.0 - w_u) (the subtraction in f64: what torch does with a Python scalar), and
 *   out[c][t] = F[c][q] * omw + mean[c] * wf, two f32 products and one f32 sum, never contracted into a fused multiply-add.  A row with
 *   text_of = -1 or w_u == 0 is gathered plainly, out[c][t] = F[c][q], the expression and the bits of a run without an assist.  A padding
 *   column (map < 0) stays 0 whatever the row's weight.  The text encoder reads the blended plane where it read the gathered one; nothing
 *   else changes.
 * assist == NULL, or every text_of[u] == -1: exactly sbv2_pipeline_run_opts / sbv2_stream_begin_request_pitch: no assist sequence is run, the
 *   same launches, the same bytes.  (sbv2_utt_options is not extended: it is passed by pointer and older callers hand in the shorter struct.)
 * Co-batching.  Appended sequences change the forward's column count, and DeBERTa's small-grid summation order moves with it: a row keeps its
 *   integer durations and its PCM to f32 rounding (2e-4 on the tiny models), and bit for bit under sbv2_debug_set_ksplit(0).
 * Refused before any GPU work and before the handles are looked at, with the row or text named in sbv2_last_error: n_texts < 1, a NULL array,
 *   an s_lens entry below 1 or >= 2^20, a text_of outside [-1, A), a weight that is NaN or outside [0, 1] (not read where text_of is -1), a
 *   non-zero reserved.
 * Not built: an assist on sbv2_node_*; on the plain single-utterance sbv2_stream_begin* entries (a request stream with one row serves them);
 *   a per-token weight; caching an assist text's mean across runs; sbv2_bert_predict / sbv2_vits_synthesize, where the host has the features
 *   and can blend them itself; a text front end for the assist text (the caller parses it as it parses the spoken text). */
typedef struct sbv2_assist {
    int64_t n_texts;            /* A >= 1 */
    const int64_t* token_ids;   /* the A sequences back to back */
    const int64_t* s_lens;      /* [A] */
    const int32_t* text_of;     /* [batch->n], -1 = none */
    const double* weight;       /* [batch->n], in [0, 1]; not read where text_of is -1 */
    int64_t reserved;           /* must be 0 */
} sbv2_assist;
int sbv2_pipeline_run_assist(sbv2_pipeline* p, const sbv2_batch* batch, const sbv2_utt_options* opts /* may be NULL */,
                             const sbv2_assist* assist /* may be NULL */, const int64_t* token_ids, const int64_t* s_lens, const int64_t* word2ph,
                             int64_t* pcm_lens);
int sbv2_stream_begin_request_assist(sbv2_bert* bert, sbv2_vits* vits, const sbv2_batch* batch, const sbv2_utt_options* opts /* may be NULL */,
                                     const sbv2_assist* assist /* may be NULL */, const int64_t* token_ids, const int64_t* s_lens,
                                     const int64_t* word2ph, int64_t chunk_frames, const sbv2_stream_request* rq,
                                     const sbv2_stream_levels* lv /* may be NULL */, const sbv2_stream_pitch* sp /* may be NULL */, sbv2_stream** out,
                                     int64_t* total_samples, int64_t* n_tokens, int64_t* n_env, int64_t* n_pitch);
/* ---- new: pitch, intonation and formant scale on a request stream.  Nothing in sbv2_voice / sbv2_formant needs the whole signal except ONE
 * number, the mean f0 m that the intonation scale pivots about; the contour, the Q32 phases (a prefix sum over frames), the mapping and the
 * windows (one mark ahead) and the gather (a bounded half-width) are local.  A stream cannot know m ahead, as it cannot know its loudness, so
 * the caller names the pivot (as sbv2_stream_level's caller names the gain) and everything else is carried from chunk to chunk ON THE DEVICE.
 * Signal.  Row i of the stream is transformed exactly as sbv2_voice and sbv2_formant state it, with m := pivot_hz[i] and nothing else changed:
 *   the contour on the row's native f32 samples at hop H, the increments, both mark lists, the mapping, the windows with their edge rules (the
 *   row's length n is known at begin), the gather in f64 in ascending j, y = float(num / max(den, 1)).  formant_scale == 1 is the plain gather.
 *   Hence: if pivot_hz[i] holds the bits of the row's own m, the shifted row equals the one-shot shifter's bit for bit whatever the chunk size;
 *   |y| <= max |x| and the unchanged length come with it.
 * Pivot.  Required for every stream voice, s == 1 included (ONE formula for the target): finite and in [f0_min, f0_max] after the 0-defaults.
 *   Read it from any /synthesize_marks answer of the same voice (the mean f0_hz of its pitch block) or from src_f0.
 * Look-ahead.  With W = max(tau_max + 1, sr / 200) + 2 (no half-width and no distance of two neighbouring analysis marks exceeds it),
 *   G = ceil(W / min(q, 1)) + 1 and X = ceil((max(q, 1) - 1) W):  output k sums over the synthesis marks t within G of it, t <= k + G - 1; t
 *   needs the first analysis mark at or after it, which lies before t + W; the nearer of that mark and its predecessor needs ITS successor
 *   for its right half-width, before t + 2 W; an unvoiced grain is read up to q times as far as its window reaches, X samples more (samples,
 *   not marks).  So marks are needed at positions below k + G - 1 + 2 W and samples at or below k + G - 1 + 2 W + X.  The marks below
 *   position F H are known once the contour frames 0 .. F - 1 are, and frame f is complete where sbv2_pitch says: once f H + H div 2 + tau_max
 *   samples are in.  With S samples fed the complete frames reach beyond S - tau_max - H div 2.  Output k is therefore final once
 *       A_v = G + 2 W + X + tau_max + H div 2
 *   native samples of the row follow it: 2640 at 44.1 kHz, 70 Hz, H = 220, q = 1 (60 ms); 3273 at q = 0.5, 3273 at q = 2.  A higher f0_min
 *   shortens it (tau_max = ceil(sr / f0_min) enters four times).
 * Delivery rule (deterministic, no host wait): after S native samples of a row have been fed and the row has not ended, max(0, S - A_v) of
 *   its shifted samples are final; the window that feeds the row's last sample makes all n final.  A call then delivers the timeline's
 *   output samples j whose filter reads final samples only (floor((j M + half) / L) below place + final), never fewer than the calls
 *   before it delivered and nothing while no sample of the row is final; a row's last call delivers up to where it always ended (the
 *   row's end and half its gap).  Time is not shifted: sbv2_stream_marks and sbv2_stream_timeline stay valid, only delivery runs late.
 *   sbv2_stream_voice_timeline gives every call's delivered count ahead.  A level's own A adds behind.
 * Taking the chunks: with sbv2_stream_next_level, whatever else the stream carries: *n_consumed = the chunk's samples (0 = the end),
 *   *n_out = what the call delivers (bytes for FLAC), possibly 0.  The other sbv2_stream_next* calls are refused on a voice stream.
 * Composition: every encoding, FLAC, sbv2_stream_level, levels / env_hop / stream pitch (all of the delivered, shifted samples), assist,
 *   n rows with gaps.  voice == NULL is exactly sbv2_stream_begin_request_assist: the same launches, the same bytes.
 * Refused before any GPU work: a NULL or non-finite pivot or one outside [f0_min, f0_max], the identity (p = s = q = 1: begin the stream
 *   without the struct), non-zero reserved fields, everything sbv2_voice and sbv2_formant refuse.
 * Not built: pitch_track and token_pitch on a stream (Viterbi and token means need unbounded look-ahead), the plain sbv2_stream_begin*
 *   entries (a request stream of one row serves them), sbv2_node_*, estimating the pivot on the fly. */
typedef struct sbv2_stream_voice {
    sbv2_voice voice;            /* p, s, f0_min, f0_max, threshold, hop: the rules of sbv2_voice */
    double formant_scale;        /* [0.5, 2], the rules of sbv2_formant; 1 = plain gather */
    const double* pivot_hz;      /* [batch->n]: replaces the row mean m in g_f = p (m + s (f0_f - m)) */
    double reserved[2];          /* must be 0 */
} sbv2_stream_voice;
int sbv2_stream_begin_request_voice(sbv2_bert* bert, sbv2_vits* vits, const sbv2_batch* batch, const sbv2_utt_options* opts /* may be NULL */,
                                    const sbv2_assist* assist /* may be NULL */, const int64_t* token_ids, const int64_t* s_lens,
                                    const int64_t* word2ph, int64_t chunk_frames, const sbv2_stream_request* rq,
                                    const sbv2_stream_levels* lv /* may be NULL */, const sbv2_stream_pitch* sp /* may be NULL */,
                                    const sbv2_stream_voice* voice /* may be NULL */, sbv2_stream** out, int64_t* total_samples,
                                    int64_t* n_tokens, int64_t* n_env, int64_t* n_pitch);
/* Host only: A_v at sample_rate (v->pivot_hz is not looked at); -1 for parameters the begin call refuses. */
int64_t sbv2_stream_voice_lookahead(const sbv2_stream_voice* v, int32_t sample_rate);
/* Host only: sbv2_stream_timeline's arguments and the voice (pivot_hz not looked at; the rate is the model's, 44100) -> call_delivered[c] = the
 * samples call c of a voice stream WITHOUT a level delivers by the delivery rule (they sum to the stream's total), *n_calls. */
int sbv2_stream_voice_timeline(const int64_t* frames, const int64_t* gap_after, int64_t n, int32_t hop, int64_t chunk_frames,
                               const sbv2_pcm_format* fmt, const sbv2_stream_voice* v, int64_t* call_delivered, int64_t capacity, int64_t* n_calls);
/* Test hook: the fed shifter on one host row x[n] at sample_rate, cut at the ascending positions cuts[ncuts] into ncuts + 1 pushes (empty ones
 * allowed, the last one ends the row); v carries ONE pivot.  period_in / voiced_in as sbv2_debug_voice_shift takes them.  y receives the
 * pushes' final samples back to back (n in all), out_per_push[ncuts + 1] their counts (the delivery rule). */
int sbv2_debug_voice_stream(int device, const float* x, int64_t n, const int64_t* cuts, int ncuts, int32_t sample_rate, const sbv2_stream_voice* v,
                            const double* period_in, const int32_t* voiced_in, float* y, int64_t* out_per_push);

/* ---- new: a loudness target on a request stream: a gated leveler carried from chunk to chunk ON THE DEVICE.
 * An exact integrated-loudness target needs the end of the signal; a follower does not.  The BS.1770 meter of sbv2_loudness is a linear
 * recurrence over segments and its gated mean can be kept as a running quantity, so a gain that tracks "target - loudness of everything heard so
 * far" needs no look-ahead beyond the limiter's own A samples.  The leveler starts from the caller's gain_db (sbv2_stream_level: the guess),
 * walks to the right gain at a bounded rate, ends at target - L_in and reports L_in, so the next request of the same voice can start right.
 * Signal.  y = the stream's delivered signal: f64, at the format's rate fs, before any cast: the signal the limiter of a level stream reads.
 *   S = fs div 10.  m = the K-weighting segment length of the meter at that rate: 200 at 8 / 16 / 32 kHz, 245 at 22.05 / 44.1 kHz, 240 at 24 /
 *   48 kHz (m divides S).
 * Meter.  w = y through the K-weighting cascade of sbv2_loudness: the same coefficients, transposed direct form II, zero state at the stream's
 *   start.  Segment s covers samples [s m, (s + 1) m); its start state is st_{s+1} = A^m st_s + e_s with st_0 = 0, A the cascade's transition
 *   over one sample of zero input and e_s the segment's end state from a zero start, folded in ascending segment order (a sequential fold, not
 *   a scan tree: each row of A^m st is 4 fused multiply-adds in ascending column order onto e_s); its partial p_s = the sum of w^2 in sample
 *   order from st_s (acc = fma(w, w, acc)).  Quarter k = samples [k S, (k + 1) S), complete quarters only; E_k = the sum of its S / m partials
 *   in ascending order.  Block j >= 3: z_j = (((E_{j-3} + E_{j-2}) + E_{j-1}) + E_j) / (4 S), l_j = -0.691 + 10 log10 z_j.
 * Running gated loudness.  Once quarter k is complete, Lambda_k = the BS.1770-4 integrated loudness over the blocks 3 .. k: absolute gate
 *   l_j > -70, relative gate l_j > (-0.691 + 10 log10 of the mean z of the blocks that passed the absolute gate) - 10, Lambda_k = -0.691 +
 *   10 log10 of the mean z of the blocks that pass both; -inf when no block passes (always for k < 3).  n_k = the number of blocks that pass the
 *   absolute gate.  Every mean over blocks runs in an order that depends on the block indices alone (block j - 3 is added by lane (j - 3) mod
 *   256 in ascending order, the lanes by a fixed tree), so the values agree with a sequential float64 sum to its rounding, not bit for bit.
 * Gain schedule, in dB.  g_k = the gain reached at the end of quarter k, decided from quarters < k only.  g_0 = gain_db of the stream's
 *   sbv2_stream_level.  For k >= 1: if n_{k-1} >= hold_blocks and Lambda_{k-1} is finite, want = clamp(target_lufs - Lambda_{k-1},
 *   gain_db - range_db, gain_db + range_db) and g_k = g_{k-1} + clamp(want - g_{k-1}, -slew_db_per_s / 10, +slew_db_per_s / 10); otherwise
 *   g_k = g_{k-1}.
 * Gain applied.  a_k = 10^(g_k / 20).  Sample i (0 <= i < S) of quarter k becomes v = y (a_{k-1} + (a_k - a_{k-1}) (i + 1) / S), a_{-1} = a_0;
 *   the trailing partial quarter is ramped like a whole one.
 * Behind the leveler.  v goes through the stream limiter of sbv2_stream_level begun at gain 0 dB under the level's ceiling: x = v s, |x| <= c as
 *   on any level stream.  Delivery runs A samples late and not one more: the gain of a sample depends only on quarters that end before that
 *   sample's quarter begins.  The delivery rule, sbv2_stream_level_lookahead, sbv2_stream_call_bound, the timelines, sbv2_stream_marks, the
 *   stream levels and the stream pitch (all of the delivered x) stay as they are; such a stream is taken with sbv2_stream_next_level.
 * Chunk invariance.  x, the schedule g_k and the stats do not depend on how the stream is cut into chunks.
 * Carried on the device: the 4-double filter state, the < m samples of the unfinished segment, the < S / m partials of the unfinished quarter,
 *   the last three E, the block history z_j and g_k, a_k (ceil(total / S) doubles each), the running stats.  Five launches per replay.
 * leveler == NULL: exactly sbv2_stream_begin_request_voice: the same launches, the same bytes.
 * Refused before any GPU work and before the handles are looked at: non-finite or out-of-range fields, a non-zero reserved, a leveler without
 *   rq->level (it needs the ceiling and the starting gain).
 * Not built: a bound on the limiter's depth on a stream (reported, as on any level stream), the compressor on a stream, the plain
 *   sbv2_stream_begin_level entry (a request stream of one row serves it), sbv2_node_*, a short-term (per-sentence) leveler. */
typedef struct sbv2_stream_leveler {
    double target_lufs;      /* [-70, -5], as sbv2_loudness.target_lufs */
    double range_db;         /* [0, 20]: g stays within gain_db +- range_db; usual value 12 */
    double slew_db_per_s;    /* (0, 20]: g moves at most slew / 10 dB per quarter; usual value 3 */
    int32_t hold_blocks;     /* [1, 100]: blocks above the absolute gate before g moves; usual value 10 */
    int32_t reserved;        /* must be 0 */
} sbv2_stream_leveler;
int sbv2_stream_begin_request_leveler(sbv2_bert* bert, sbv2_vits* vits, const sbv2_batch* batch, const sbv2_utt_options* opts /* may be NULL */,
                                      const sbv2_assist* assist /* may be NULL */, const int64_t* token_ids, const int64_t* s_lens,
                                      const int64_t* word2ph, int64_t chunk_frames, const sbv2_stream_request* rq,
                                      const sbv2_stream_levels* lv /* may be NULL */, const sbv2_stream_pitch* sp /* may be NULL */,
                                      const sbv2_stream_voice* voice /* may be NULL */, const sbv2_stream_leveler* leveler /* may be NULL */,
                                      sbv2_stream** out, int64_t* total_samples, int64_t* n_tokens, int64_t* n_env, int64_t* n_pitch);
/* stats[0] = L_in = Lambda of the last complete quarter (-inf when none passed the gates), stats[1] = the last g (g_K, K = the complete
 * quarters: the gain to begin the next request of the voice with), stats[2] / stats[3] = the lowest / highest g_k, k = 0 .. K, stats[4] /
 * stats[5] = the two of sbv2_stream_level_stats (20 log10 min s, max |x|).  Refused before the stream is complete, as that call is. */
int sbv2_stream_leveler_stats(sbv2_stream* s, double* stats /* [6] */);
/* Test hook: the fed leveler and the stream limiter behind it on a host f64 signal, as StreamOutput runs them.  On the device the input lies
 * between NaN words (a read outside [0, n) poisons a result).  x[n] is cut at the ascending positions cuts[ncuts] into ncuts + 1 pushes (empty
 * ones allowed, the last one ends the stream; ncuts = 0 is the one shot); out_x receives the pushes' samples back to back (n in all),
 * out_per_push[ncuts + 1] their counts (the delivery rule), out_gain_db[k] = g_k for k = 0 .. n div S (gain_capacity must hold them), stats the
 * 6 doubles.  level, leveler, rate, cuts and the capacity are checked before any device call. */
int sbv2_debug_leveler_stream(int device, const double* x, int64_t n, const int64_t* cuts, int ncuts, int32_t sample_rate,
                              const sbv2_stream_level* level, const sbv2_stream_leveler* leveler, double* out_x, int64_t* out_per_push,
                              double* out_gain_db, int64_t gain_capacity, double* stats);

/* Test hook: the two kernels on a host plane F [C][ld] (pitch ld, any value >= 1; on the device it lies between NaN words).  Assist sequence a
 * is the columns [a_start[a], a_start[a] + a_len[a]) of F; text column t < L reads source column map[t] (< 0: padding) and belongs to row
 * row_of[t] in [0, n_rows) (read where map[t] >= 0); text_of / weight [n_rows] as in sbv2_assist, checked the same way.  mean [A][C] and
 * out [C][L] are pre-filled with 0x5A on the device and lie between guard words; *stray = the guard and pitch-pad words no longer 0x5A. */
int sbv2_debug_assist_blend(int device, const float* F, int64_t C, int64_t ld, const int32_t* map, const int32_t* row_of, int64_t L, int64_t A,
                            const int32_t* a_start, const int32_t* a_len, int64_t n_rows, const int32_t* text_of, const double* weight, float* mean,
                            float* out, int64_t* stray);

/* ---- test hooks (no reference counterpart) ------------------------------------------------------------------------ */
/* bucket(rel) for rel in [-(max_s-1), max_s-1] (transformers modeling_deberta_v2.py:57-69); host only, no GPU needed. */
int sbv2_debug_bucket_table(int64_t max_s, int64_t buckets, int64_t max_rel, int32_t* out);
/* y[Cout][L] = conv1d(x[Cin][L], w[Cout][Cin][k], bias, dilation, 'same' padding) with optional leaky-ReLU on the input,
 * through the production implicit-GEMM kernel; host buffers. */
int sbv2_debug_conv1d(int device, const float* x, const float* w, const float* bias, int64_t cin, int64_t cout, int64_t k,
                      int64_t L, int64_t dilation, float pre_slope, float* y);
/* y[Cout][L*stride] = conv_transpose1d(x[Cin][L], w[Cin][Cout][k], bias, stride, padding) via the polyphase path. */
int sbv2_debug_conv_transpose1d(int device, const float* x, const float* w, const float* bias, int64_t cin, int64_t cout,
                                int64_t k, int64_t L, int64_t stride, int64_t padding, float pre_slope, float* y);
/* Same contract as sbv2_debug_conv1d but through the channels-last bf16 MFMA kernel (mode 1 = split-bf16, 2 = plain bf16);
 * when iters > 0 also returns the mean time of `iters` further launches in *ms. */
int sbv2_debug_conv1d_cl(int device, const float* x, const float* w, const float* bias, int64_t cin, int64_t cout, int64_t k,
                         int64_t L, int64_t dilation, float pre_slope, int mode, int64_t iters, float* y, float* ms);
/* The named-tensor table an import of `model` (ONNX / .sbv2 / container; kind 1 = DeBERTa, 2 = VITS) produces, written back as an SBV2W001
 * container (owned, sbv2_bytes_free): tests compare it with the container the same weights were packed into.  Host only. */
int sbv2_debug_import_to_container(const uint8_t* model, size_t len, int kind, uint8_t** out, size_t* out_len);
/* Per-launch HIP-event timing of the implicit-GEMM kernel family between begin and end; end writes a JSON array
 * [{"kernel", "launches", "ms", "flop"}] (one entry per tile configuration) into json[cap]. */
int sbv2_prof_begin(void);
int sbv2_prof_end(char* json, int64_t cap);
/* Times `iters` launches of one dilated conv (device buffers, random data) and returns the mean kernel time in ms. */
int sbv2_debug_time_conv1d(int device, int64_t cin, int64_t cout, int64_t k, int64_t L, int64_t dilation, int64_t iters,
                           float* ms);
/* Small-grid threshold of the f32 GEMM (workgroups of the 64 x 64 tiling below which the one-wave 16 x 16 kernel runs; 0 = never; default
 * 128).  Returns the previous value; tests use it to compare both kernels bit for bit in one process. */
int sbv2_debug_set_skinny_max(int workgroups);
/* 1 (default): the ResBlocks of the wide decoder stages run on conv_clx.hip when the launch has >= 128 tiles; 2: always; 0: on conv_cl.hip.
   The two kernels sum in different orders (round 5: conv_clx on 16 x 16 x 32 MFMAs) and agree to f32 rounding; with 0 (and sbv2_debug_set_ksplit(0)) every
   launch size takes the same kernels and a batch row equals its single-utterance call bit for bit.  Returns the previous value, or -1 for any other value
   (the setting stays). */
int sbv2_debug_set_clx(int on);
/* 1 (default): the small-grid dispatch of a single utterance's launches: gemm_bfs products with a long K loop split it over workgroups (K >= 2048) or over the
   four waves of a 32 x 32 tile (the 1024 x 1024 products) and add the partial sums in group order, and LayerNorm runs few columns per workgroup; other
   summation orders than the batch's launch shapes, so a single call and its batch row agree to f32 rounding; 0: the batch's launch shapes at every size (batch
   row == single call bit for bit; the bit-equality tests run on it).  Returns the previous value. */
int sbv2_debug_set_ksplit(int on);
/* the flow's attention on keys / values pre-split by the q | k | v product: 1 (default) for sequences of >= 4096 frames and launches of <= 64
   workgroups, 2 at every length, 3 at every length on the un-pipelined kernel (k_vits_flash_x3p, the fallback for head dimensions that are no multiple
   of 8), 4 at every length on the pipelined kernel's 8-wave shape (the batch shape, forced for the test), 0 never (converted per key tile inside the
   attention kernel); bit-identical; returns the previous setting */
int sbv2_debug_set_flash_parts(int on);
/* 0 (default): the stochastic duration predictor runs only for the rows of a call whose sdp_ratio is not exactly 0: not at all when there is none, on a
   second text layout over those rows when there are some, on the text layout when all need it.  1: for every row of every call on the text layout, as the
   exported graph does.  The two agree bit for bit in durations, logw (up to the sign of an exact zero at ratio 0) and PCM wherever the predictor's value is
   finite (on the second layout the predictor's LayerNorm launches take the kernels the text layout's column count selects, so this holds whichever side of
   the small-grid threshold of sbv2_debug_set_ksplit either layout falls on); the tests compare them in one process.  Process-wide, atomic; returns the
   previous value. */
int sbv2_debug_set_sdp_all(int on);
/* Same contract as sbv2_debug_conv1d_cl (mode 1) through conv_clx.hip: x is split into bf16 parts of lrelu(x, pre_slope) first (split_cl), the
   convolution reads the parts; y = (conv + bias + res) * beta; ys_sum (optional) = hi + lo of the parts of lrelu(y, 0.1) the epilogue emits. */
int sbv2_debug_conv1d_clx(int device, const float* x, const float* w, const float* bias, const float* res, int64_t cin, int64_t cout, int64_t k,
                          int64_t L, int64_t dilation, float pre_slope, float beta, int64_t iters, float* y, float* ys_sum, float* ms);
/* Diagnostics for the f16x3 operand format (DeBERTa's and the flow's 1x1 products): the split of an activation into the f16 hi / scaled-lo pair clamps
   finite values beyond +-65504 (NaN and infinities propagate).  enable = 1 / 0 switches the device-side counter of clamped values on / off for planes
   allocated from then on (-1: leave as is; the SBV2_F16X3_SATCOUNT=1 environment variable switches it on from the start); *count (optional) receives the
   number of clamped values since the last call, on `device`.  A non-zero count on a real checkpoint means: run with SBV2_BERT_GEMM=bf16x6. */
int sbv2_debug_f16x3_saturation(int device, int enable, uint64_t* count);
/* 1 (default): the fused ResBlock steps of the <= 64-channel decoder stages run on respair_x16.hip where it exists (C = 32 / 64, k = 7 / 11: 16x16x32 MFMAs,
   step pairs in the K dimension; f32 rounding apart) and on respair_clx.hip (split-bf16, k in {3, 7, 11}) otherwise; 0: respair_cl.hip (respair_clx.hip's
   bits at C = 32 / 64).  Returns the previous value, or -1 for any other value (the setting stays). */
int sbv2_debug_set_respair_clx(int on);
/* One fused ResBlock1 step y' = beta (conv2(lrelu(conv1(lrelu(x), dilation) + b1)) + b2 + x) [+ y when accumulate], masked by mask[n / mask_div] (may be
   null; mask_div a power of two), channels-last x / y [N][C], w [C][C][k], split-bf16, through respair_cl.hip (variant 0), the default dispatch's kernel
   (variant 1: respair_x16.hip where it exists, else respair_clx.hip) or respair_clx.hip (variant 2).  Test hook. */
int sbv2_debug_respair(int device, const float* x, const float* w1, const float* w2, const float* b1, const float* b2, int64_t C, int64_t N, int64_t k,
                       int64_t dilation, const uint8_t* mask, int64_t mask_div, float beta, int accumulate, int variant, float* y);
/* 1 (default; SBV2_RESBRANCH): the k = 3 branches of the 128- / 64- / 32- / 16-channel decoder stages and the k = 7 / 11 branches of the 16-channel stage
   run their three steps in ONE launch (resbranch_clx.hip: y_1, y_2 stay on the chip, 2 plane passes through HBM per branch instead of 6); 0: three fused-step
   launches (same bits; at 128 channels six conv_clx launches: f32 rounding apart).  Returns the previous value, or -1 for any other value (the setting
   stays). */
int sbv2_debug_set_resbranch(int on);
/* 1 (default; SBV2_UPX): the ConvTranspose1d of the wide decoder stages (large launches) runs as ONE phased conv_clx.hip launch on pre-split operands
   (rows = (phase, cout), every phase on its own input taps); 0: conv_cl.hip's phase groups (f32 rounding apart).  Returns the previous value, or -1 for any
   other value (the setting stays). */
int sbv2_debug_set_upx(int on);
/* ConvTranspose1d(lrelu(x, pre_slope)) [cin][L] -> y [cout][L * stride] (weight [cin][cout][k], padding (k - stride) / 2) through the phased conv_clx launch;
   mask (may be null): input position n and its `stride` outputs are kept iff mask[n / mask_div]; ys_sum (may be null): hi + lo of the bf16 parts of
   lrelu(y, 0.1) the launch writes for the ResBlocks.  iters > 0: *ms = average duration.  Test / measurement hook (scripts/convert/convert_model.py:97-110's
   `ups` layers). */
int sbv2_debug_conv_transpose1d_clx(int device, const float* x, const float* w, const float* bias, int64_t cin, int64_t cout, int64_t k, int64_t L,
                                    int64_t stride, float pre_slope, const uint8_t* mask, int64_t mask_div, int64_t iters, float* y, float* ys_sum, float* ms);
/* A whole ResBlock1 branch (HifiGanResidualBlock.forward, modeling_vits.py:455-463; the graph of scripts/convert/convert_model.py:97-110): three steps
   y_q = conv2_q(lrelu(conv1_q(lrelu(y_{q-1}), dilations[q]) + b1_q)) + b2_q + y_{q-1}, result beta * y_3 [+ y when accumulate], masked by mask[n / mask_div]
   (a power of two; mask may be null) at every layer; channels-last x / y [N][C], w [6][C][C][k] and bias [6][C] in the order conv1_0, conv2_0, conv1_1, ...,
   split-bf16, C in {16, 32, 64, 128, 256}; variant 0 = three launches of the fused step (respair_clx.hip, C <= 64), 1 = one launch (resbranch_clx.hip,
   C <= 128), 2 = six launches of conv_cl.hip (any C), 3 = six launches of conv_clx.hip as the decoder's wide stages make them (C >= 128: the input's bf16
   parts by one split_cl pass, conv1 writes parts only, conv2 reads them and adds the residual plane; beta and accumulate on the last launch).
   iters > 0: *ms = average duration of `iters` further runs.  Test / measurement hook. */
int sbv2_debug_resbranch(int device, const float* x, const float* w, const float* bias, int64_t C, int64_t N, int64_t k, const int64_t* dilations,
                         const uint8_t* mask, int64_t mask_div, float beta, int accumulate, int variant, int64_t iters, float* y, float* ms);
/* Variant 3 of sbv2_debug_resbranch whose last launch also writes the bf16 parts of lrelu(y, 0.1), as the last branch of a stage does for the next
   transposed convolution: ys (may be null) [N][C] = hi + lo of those parts.  y_steps, ys_steps (may be null) [2][N][C]: the planes the first two steps
   returned and hi + lo of the parts their conv2 launches wrote for the next step's conv1, so a test can hold the chain step by step. */
int sbv2_debug_resbranch_ys(int device, const float* x, const float* w, const float* bias, int64_t C, int64_t N, int64_t k, const int64_t* dilations,
                            const uint8_t* mask, int64_t mask_div, float beta, int accumulate, int64_t iters, float* y, float* ys, float* y_steps, float* ys_steps,
                            float* ms);
/* y[M][N] = act(w[M][K] x[K][N] + bias) (+ res) through the split-bf16 1x1 GEMM (gemm_bfs.hip; parts 2 = bf16x3, 3 = bf16x6).  split_out != 0:
   the result is also emitted as that many bf16 parts and y returns their sum.  iters > 0: average launch time in *ms.  Test hook. */
int sbv2_debug_gemm_bfs(int device, const float* x, const float* w, const float* bias, const float* res, int64_t M, int64_t N, int64_t K,
                        int parts, int act, int split_out, int64_t iters, float* y, float* ms);
/* The same product for TWO inputs xa, xb [K][N] launched alternately (iters + 2 launches) on ONE K-split scratch buffer that is never cleared in between;
   ya / yb = the last result of each.  A workgroup that summed a stale partial sum (the other input's, left in its XCD's L2 by the previous launch) shows up as a
   wrong result: the race screen of gemm_bfs.hip's cross-workgroup K split.  parts as above. */
int sbv2_debug_gemm_bfs_alt(int device, const float* xa, const float* xb, const float* w, const float* bias, const float* res, int64_t M, int64_t N, int64_t K,
                            int parts, int64_t iters, float* ya, float* yb);
/* ---- the repeated-launch screen of the inline-asm MFMA kernels (tests/test_mfma_repeatability.py) ----
   One launch of the named kernel is enqueued `reps` (2 .. 4096) times on one stream with no host synchronisation in between, alternately on the two inputs
   xa / xb (repetition i: input and output plane i % 2).  Before each repetition a device-to-device copy restores the output (prev when it is given: the launch
   accumulates onto it; NaN otherwise: every row must be written), after it a comparison kernel counts the 32-bit words of everything the launch writes that
   differ from the FIRST result of the same input: mismatch[i] = that count, first_bad[i] = the index of the first such word (-1: none), both [reps].
   ya / yb = the first result of each input.  neighbour != 0: a second stream receives one launch per repetition from the same host loop, alternately a
   LayerNorm [1024][8192] and a gemm_bfs f16x3 product 1024 x 1024 x 2048 (nothing polls or waits; no graphs).  flip_at >= 0: one bit of word flip_word of
   repetition flip_at's output is flipped before its comparison (the screen's self-check; -1: off).  A HIP error of any launch is returned; nothing is
   retried.  Operands as in sbv2_debug_respair (variant 1 / 2; 3 = respair_x16.hip or an error), sbv2_debug_resbranch (variant 1) and sbv2_debug_conv1d_clx; the latter's words are the f32
   plane [L][cout] and, with want_ys, the bf16 parts planes behind it (ysa / ysb = hi + lo of the first results). */
int sbv2_debug_repeat_respair(int device, const float* xa, const float* xb, const float* w1, const float* w2, const float* b1, const float* b2, int64_t C,
                              int64_t N, int64_t k, int64_t dilation, const uint8_t* mask, int64_t mask_div, float beta, const float* prev, int variant,
                              int reps, int neighbour, int flip_at, int64_t flip_word, float* ya, float* yb, int64_t* mismatch, int64_t* first_bad);
int sbv2_debug_repeat_resbranch(int device, const float* xa, const float* xb, const float* w, const float* bias, int64_t C, int64_t N, int64_t k,
                                const int64_t* dilations, const uint8_t* mask, int64_t mask_div, float beta, const float* prev, int reps, int neighbour,
                                int flip_at, int64_t flip_word, float* ya, float* yb, int64_t* mismatch, int64_t* first_bad);
int sbv2_debug_repeat_conv1d_clx(int device, const float* xa, const float* xb, const float* w, const float* bias, const float* res, int64_t cin, int64_t cout,
                                 int64_t k, int64_t L, int64_t dilation, float pre_slope, float beta, int want_ys, int reps, int neighbour, int flip_at,
                                 int64_t flip_word, float* ya, float* yb, float* ysa, float* ysb, int64_t* mismatch, int64_t* first_bad);
/* ... the phased transposed convolution of the wide decoder stages (operands as sbv2_debug_conv_transpose1d_clx; y [cout][L * stride], the mask on input
   positions), and y[M][N] = w[M][K] x[K][N] + bias (+ res) through gemm_bfs.hip as conv_bfs launches it (parts code 2 / 3 / 4 as sbv2_debug_gemm_bfs, with the
   K-split scratch DeBERTa's forward provides; split_out = parts: the parts copy is written and compared as well).  gemm_bfs' words are the f32 plane at its
   device pitch [M][round_up(N, 64)], then the parts planes. */
int sbv2_debug_repeat_conv_transpose1d_clx(int device, const float* xa, const float* xb, const float* w, const float* bias, int64_t cin, int64_t cout, int64_t k,
                                           int64_t L, int64_t stride, float pre_slope, const uint8_t* mask, int64_t mask_div, int want_ys, int reps,
                                           int neighbour, int flip_at, int64_t flip_word, float* ya, float* yb, float* ysa, float* ysb, int64_t* mismatch,
                                           int64_t* first_bad);
int sbv2_debug_repeat_gemm_bfs(int device, const float* xa, const float* xb, const float* w, const float* bias, const float* res, int64_t M, int64_t N, int64_t K,
                               int parts, int split_out, int reps, int neighbour, int flip_at, int64_t flip_word, float* ya, float* yb, float* ysa, float* ysb,
                               int64_t* mismatch, int64_t* first_bad);
/* ... and k_vits_flash_x3q (attn_flash.hip) on the flow's frame layout as sbv2_debug_vits_attention's variants 4 / 5 build it, the launcher choosing the 4- or
   8-wave shape by the grid as in the model: q / k / v packed [heads * dk][sum lens] in two sets, ctx cleared before every repetition.  The words are the ctx
   plane at its device pitch [heads * dk][*ld], gaps and pad columns included. */
int sbv2_debug_repeat_vits_attention(int device, const float* qa, const float* ka, const float* va, const float* qb, const float* kb, const float* vb,
                                     const float* erk, const float* erv, const int64_t* lens, int nutt, int64_t heads, int64_t dk, int64_t window, int reps,
                                     int neighbour, int flip_at, int64_t flip_word, float* ctxa, float* ctxb, int64_t* ld, int64_t* mismatch,
                                     int64_t* first_bad);
/* ... and the flow FFN pair as VitsModel::run_encoder launches it on conv_clx.hip (weights through sbv2_debug_conv_ffn_cl's builders): conv_1 writes relu(.) as
   conv_2's operand parts, conv_2 the k-major plane y = conv + b + x, mask [L] at both; one repetition = both launches; x / y [H][L].  The words are the
   intermediate's parts planes, then y at its device pitch [H][round_up(L, 64)]. */
int sbv2_debug_repeat_conv_ffn_clx(int device, const float* xa, const float* xb, const float* w1, const float* b1, const float* w2, const float* b2, int64_t H,
                                   int64_t F, int64_t k, int64_t L, const uint8_t* mask, int reps, int neighbour, int flip_at, int64_t flip_word, float* ya,
                                   float* yb, int64_t* mismatch, int64_t* first_bad);
/* ---- conv_plain, conv_bfs, the encoders' FFN pair and linear_tokmajor with every argument the models pass (tests/test_gemm_conv_kernels.py) ----
   Host planes [C][L] without pitch; on the device every plane sits at the library's pitch, every input holds NaN in the columns L .. pitch, outputs are
   pre-filled with a sentinel (0x5A bytes) and *stray (optional) = the number of pad words of the outputs that the launch changed.
   Epilogue order of all of them: bias, act (0 none, 1 ReLU, 2 erf-GELU, 3 tanh), * alpha, + res, * beta, + previous contents (accumulate), mask.
   sbv2_debug_conv_plain: exactly conv_plain on a WeightStore(blob, cl_parts): y[co][n] = epi(sum_ci sum_j w[co][ci][j] lrelu(x, pre_slope)[ci][n + j dilation -
   pad_l]); cl_parts 0 = launch_conv (f32 MFMA, the skinny kernels under sbv2_debug_set_skinny_max), 2 / 1 / 3 = split-bf16 / bf16 / f16 fragments, which k >= 3
   takes through the k-major launch_conv_cl.  bias, mask, res may be null; output column n is kept iff mask[n / mask_div]; y_inout is read when accumulate. */
int sbv2_debug_conv_plain(int device, const float* x, const float* w, const float* bias, int64_t cin, int64_t cout, int64_t k, int64_t L, int64_t dilation,
                          int64_t pad_l, int cl_parts, const uint8_t* mask, int64_t mask_div, int act, float pre_slope, const float* res, float alpha,
                          float beta, int accumulate, float* y_inout, int64_t* stray);
/* The encoder FFN as VitsModel runs it on the matrix cores (split-bf16): mid = mask * (conv(x, w1 [F][H][k]) + b1) kept channels-last on the device
   (conv_km_to_cl; returned as [F][L]), y = mask * (conv(relu(mid), w2 [H][F][k]) + b2 + res) (conv_cl_to_km with pre_slope 0); 'same' padding (k - 1) / 2.
   Fails where either function refuses the shape. */
int sbv2_debug_conv_ffn_cl(int device, const float* x, const float* w1, const float* b1, const float* w2, const float* b2, int64_t H, int64_t F, int64_t k,
                           int64_t L, const uint8_t* mask, const float* res, float* y, float* mid, int64_t* stray);
/* sbv2_debug_gemm_bfs with the rest of conv_bfs' arguments: the result is act(w x + bias) * alpha (+ res) * beta, column n kept iff mask[n / mask_div]; the
   f32 plane y receives rows < y_rows (-1: all; want_y = 0: no f32 plane is passed), the parts rows >= ys_row0; ys = the recombined parts, separately from
   y.  Rows a plane does not receive still hold the sentinel (ys: the recombination of sentinel halves). */
int sbv2_debug_gemm_bfs_ex(int device, const float* x, const float* w, const float* bias, const float* res, int64_t M, int64_t N, int64_t K, int parts, int act,
                           int split_out, int64_t iters, const uint8_t* mask, int64_t mask_div, float alpha, float beta, int64_t y_rows, int64_t ys_row0,
                           int want_y, float* y, float* ys, float* ms, int64_t* stray);
/* linear_tokmajor: y [L][cout] = x^T w^T + bias from x [cin][L], w [cout][cin]; on the device y has the row pitch ldy >= cout (columns cout .. ldy and the
   words behind the last row are counted in *stray) */
int sbv2_debug_linear_tokmajor(int device, const float* x, const float* w, const float* bias, int64_t cin, int64_t cout, int64_t L, int64_t ldy, float* y,
                               int64_t* stray);
/* One window-relative attention of the VITS encoders (attn_flash.hip / ops.hip) on a packed batch, laid out and planned by the model's own builders
   (make_layout, make_attn_plan, flash_choice).  q, k, v, ctx: [heads * dk][sum lens] (utterances concatenated, head h = rows h dk .. + dk); erk, erv:
   [2 window + 1][dk]; layout: 0 = text-rate layout, 1 = frame-rate layout (the flow's); qscale = 1 / sqrt(dk).  variant: -1 = the flow's own choice for
   this batch, 0 = unfused (grouped GEMMs, k_vits_softmax, k_vits_relv_add), 1 = k_vits_flash (exact f32), 2 = k_vits_flash_x3, 3 = k_vits_flash_x3p,
   4 / 5 = k_vits_flash_x3q on its 4- / 8-wave shape (3 .. 5 read k and v as the bf16 parts the q | k | v product's epilogue writes).  poison != 0: every
   column of q, k, v and their parts outside an utterance (layout gaps and the tail up to the pitch) holds NaN and ctx is filled with a sentinel first;
   *stray (optional) = the number of ctx elements outside an utterance that no longer hold it. */
int sbv2_debug_vits_attention(int device, const float* q, const float* k, const float* v, const float* erk, const float* erv, const int64_t* lens, int nutt,
                              int64_t heads, int64_t dk, int64_t window, int layout, int variant, int poison, float* ctx, int64_t* stray);
/* One disentangled attention of DeBERTa (attn_deberta.hip / ops.hip) on a packed batch, planned by the model's own builder (make_deberta_attn_plan).
   q, k, v, ctx: [heads * d][sum lens]; pos_k, pos_q: [heads * d][2 span] (the model's position planes, span = buckets > 0 ? buckets : max_rel);
   tok_mask: [sum lens] attention mask per token (null: all ones); gap: zero columns between utterances.  variant: -1 = the model's per-utterance dispatch,
   0 = unfused (grouped GEMMs + deberta_softmax), 1 / 2 / 3 = every utterance on the short / 128-token / long kernel (an error, and no launch, when one
   does not fit).  poison: as sbv2_debug_vits_attention. */
int sbv2_debug_deberta_attention(int device, const float* q, const float* k, const float* v, const float* pos_k, const float* pos_q, const int64_t* lens,
                                 int nutt, int64_t heads, int64_t d, int64_t buckets, int64_t max_rel, const uint8_t* tok_mask, int64_t gap, int variant,
                                 int poison, float* ctx, int64_t* stray);

/* ---- One launcher of ops.h at a time on host data (test hooks; tests/test_ops_kernels.py) ----
   Planes are host arrays [C][L] (row-major, no pitch); on the device they get the library's pitch (a multiple of 64 floats).  poison (where it is a
   parameter; the other hooks always do it): the columns between L and the pitch of every input hold NaN, outputs are pre-filled with a sentinel, and *stray
   (optional) = the number of words outside the valid region (pad columns, guard words behind a compact output) that the launch changed.  Packed-utterance
   layouts are built by the models' own make_layout: kind 0 = the text encoder's (16-column gaps, columns rounded to 4), 1 = the flow's / decoder's
   (4-column gaps, rounded to 32); sbv2_debug_layout returns the first column of every utterance and the column count L of that layout. */
int sbv2_debug_layout(const int64_t* lens, int nutt, int kind, int32_t* start, int64_t* L);
/* layernorm_ch: y = mask * (act(LN_c(x)) + res) (act 0 / 2 = none / GELU; res, mask may be null; inplace: out == in); split_code 2 / 4: the
   result is also written as two bf16 parts / the f16 hi + scaled-lo pair, and ysplit = hi + lo (the lo scale undone).  dw_w != null: dds_dw_ln_gelu instead
   (depthwise k = 3 conv with dilation dil and bias dw_b, LayerNorm eps 1e-5, GELU; eps / act ignored).  Which kernel runs is launch_layernorm's choice
   (sbv2_debug_set_ksplit is honoured). */
int sbv2_debug_layernorm(int device, const float* x, const float* gamma, const float* beta, float eps, int act, const float* res, const uint8_t* mask,
                         const float* dw_w, const float* dw_b, int64_t dil, int64_t C, int64_t L, int inplace, int split_code, int poison, float* y,
                         float* ysplit, int64_t* stray);
/* deberta_embed_ln: y [H][N] = LN(emb[ids[n]]) per column; ids < 0 give a zero column */
int sbv2_debug_deberta_embed_ln(int device, const int32_t* ids, const float* emb, int64_t V, int64_t H, const float* gamma, const float* beta, float eps,
                                int64_t N, int poison, float* y, int64_t* stray);
/* spline_inverse on z [2][L] (row 0 = z0, row 1 = z1, in place) with params [3 nbins - 1][L] */
int sbv2_debug_spline_inverse(int device, const float* params, const float* z, const uint8_t* mask, int64_t L, int64_t nbins, float tail, float inv_sqrt_f,
                              int poison, float* z_out, int64_t* stray);
int sbv2_debug_durations(int device, const float* sdp, const float* dp, const uint8_t* mask, int64_t L, float ratio, float length_scale, float* logw,
                         int32_t* dur, int64_t* stray);
/* affine_reverse on z [2][L] in place: (z - m) * exp(-logs), or * scale when logs is null */
/* durations over a TEXT layout of nutt segments, row u with ratio[u] / length_scale[u]; sdp, dp, mask, logw, dur: [L of that layout] */
int sbv2_debug_durations_rows(int device, const float* sdp, const float* dp, const uint8_t* mask, const int64_t* lens, int nutt, const float* ratio,
                              const float* length_scale, float* logw, int32_t* dur, int64_t* stray);
int sbv2_debug_affine_reverse(int device, const float* z, const float* m, const float* logs, const float* scale, const uint8_t* mask, int64_t L,
                              float* z_out, int64_t* stray);
int sbv2_debug_convflow_pre(int device, const float* z0, const float* w, const float* b, const float* cond, const uint8_t* mask, int64_t C, int64_t L,
                            float* y, int64_t* stray);
/* noise_fill: y [rows][L of the layout]; seg_utt [nutt] = the caller-batch index of every utterance (the noise key) */
int sbv2_debug_noise_fill(int device, const int64_t* lens, int nutt, int kind, const int32_t* seg_utt, uint64_t seed, int stream_id, float scale,
                          int64_t rows, float* y, int64_t* stray);
/* expand_frames: m_p, logs_p [C][Lt]; tok_of_frame [L of the frame layout of lens] (text column or -1); y [C][L] */
int sbv2_debug_expand_frames(int device, const float* m_p, const float* logs_p, int64_t C, int64_t Lt, const int32_t* tok_of_frame, const int64_t* lens,
                             int nutt, const int32_t* seg_utt, uint64_t seed, float noise_scale, float* y, int64_t* stray);
/* noise_fill / expand_frames with row u's own (seed[u], index[u], scale[u]); the two hooks above are these with one seed and scale for every row */
int sbv2_debug_noise_fill_rows(int device, const int64_t* lens, int nutt, int kind, const uint64_t* seed, const int32_t* index, int stream_id,
                               const float* scale, int64_t rows, float* y, int64_t* stray);
int sbv2_debug_expand_frames_rows(int device, const float* m_p, const float* logs_p, int64_t C, int64_t Lt, const int32_t* tok_of_frame, const int64_t* lens,
                                  int nutt, const uint64_t* seed, const int32_t* index, const float* noise_scale, float* y, int64_t* stray);
/* conv_post_tanh (cl = 0) / conv_post_tanh_cl (cl = 1): x [C][L up] = the whole gapped plane of the frame layout of lens at `up` samples per frame,
   w [C][k], slope 0.01; pcm = the utterances' samples back to back (lens[i] up each) */
int sbv2_debug_conv_post_tanh(int device, const float* x, const float* w, int64_t C, int64_t k, const int64_t* lens, int nutt, int64_t up, int cl,
                              float* pcm, int64_t* stray);
int sbv2_debug_linear_vec(int device, const float* W, const float* bias, int64_t M, int64_t K, const float* v, int64_t B, float* y);
int sbv2_debug_gather_rows(int device, const float* table, int64_t V, int64_t K, const int32_t* idx, int64_t B, float* y);
/* text_embed on the text layout of lens: phones / tones / langs [L], bertproj [H][L], styleproj [nutt][H], y [H][L] */
int sbv2_debug_text_embed(int device, const int32_t* phones, const int32_t* tones, const int32_t* langs, const int64_t* lens, int nutt, const float* emb,
                          int64_t nph, const float* tone_emb, int64_t ntone, const float* lang_emb, int64_t nlang, const float* bertproj,
                          const float* styleproj, float scale, int64_t H, float* y, int64_t* stray);
/* add_segvec (cl = 0; x [C][L div], column n belongs to layout column n / div) / add_segvec_cl (cl = 1: the plane is transposed to [L][C] for the launch);
   tok_mask [sum lens] (may be null) is the layout's extra mask; use_mask = 0 passes no mask to the kernel */
int sbv2_debug_add_segvec(int device, const float* x, const float* vec, int64_t C, const int64_t* lens, int nutt, int kind, int64_t div,
                          const uint8_t* tok_mask, int use_mask, int cl, float* y, int64_t* stray);
/* op 0 = gather_cols (map [a], y [C][a]); 1 = transpose_out (col0 = a, T = b, y [T][C]); 2 = one window of stream_windows over the whole plane
   (first column a, width b, y [C][b], mask_out [b]); 3 = flip_channels; 4 = swap_rows (C = 2) */
int sbv2_debug_plane_op(int device, int op, const float* x, int64_t C, int64_t L, const int32_t* map, int64_t a, int64_t b, float* y, uint8_t* mask_out,
                        int64_t* stray);
/* stream_windows (ops.h), the one launch in front of a replay of the streaming decoder: z [C][L] = a plane holding several rows (the caller
   puts NaN between and around them), table [nwin][4] = {first z column of the window's row, row length in frames, first frame of the window
   within the row (any sign), row index}, cond_vecs [n_rows][cond_dim].  Outputs: z_out [nwin][C][W], mask_out [nwin][W], cond_out
   [nwin][cond_dim].  On the device the three outputs lie between guard bands; a byte written outside them fails the call.  nwin <= 16. */
int sbv2_debug_stream_windows(int device, const float* z, int64_t C, int64_t L, const int32_t* table, int64_t W, int64_t nwin, const float* cond_vecs,
                              int64_t n_rows, int64_t cond_dim, float* z_out, uint8_t* mask_out, float* cond_out);
/* copy_segments: table [nseg][3] = (source offset, destination offset, length); dst is read and written (what no segment covers stays) */
int sbv2_debug_copy_segments(int device, const float* src, int64_t nsrc, const int64_t* table, int nseg, float* dst, int64_t ndst);

#ifdef __cplusplus
}
#endif
#endif /* SBV2_HIP_H */
