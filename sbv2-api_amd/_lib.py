"""ctypes binding of libsbv2_hip.so (include/sbv2_hip.h).  Fails loudly: there is no CPU fallback."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libsbv2_hip.so")

i64p = C.POINTER(C.c_int64)
f32p = C.POINTER(C.c_float)


class Sbv2Batch(C.Structure):
    """struct sbv2_batch (include/sbv2_hip.h)."""
    _fields_ = [
        ("n", C.c_int64), ("t_lens", i64p), ("x_tst", i64p), ("tones", i64p), ("lang_ids", i64p), ("sids", i64p),
        ("style_vectors", f32p), ("bert", f32p),
        ("sdp_ratio", C.c_float), ("length_scale", C.c_float), ("noise_scale", C.c_float), ("noise_scale_w", C.c_float),
        ("noise_seed", C.c_uint64), ("forced_durations", i64p),
    ]


class Sbv2PcmFormat(C.Structure):
    """struct sbv2_pcm_format (include/sbv2_hip.h)."""
    _fields_ = [("sample_rate", C.c_int32), ("encoding", C.c_int32), ("normalize", C.c_int32), ("reserved", C.c_int32)]


class Sbv2Loudness(C.Structure):
    """struct sbv2_loudness (include/sbv2_hip.h)."""
    _fields_ = [("target_lufs", C.c_double), ("true_peak_max_dbtp", C.c_double)]


class Sbv2Limiter(C.Structure):
    """struct sbv2_limiter (include/sbv2_hip.h)."""
    _fields_ = [("target_lufs", C.c_double), ("true_peak_max_dbtp", C.c_double), ("max_reduction_db", C.c_double), ("reserved", C.c_double)]


class Sbv2Dynamics(C.Structure):
    """struct sbv2_dynamics (include/sbv2_hip.h)."""
    _fields_ = [("threshold_lu", C.c_double), ("ratio", C.c_double), ("attack_db_per_s", C.c_double), ("release_db_per_s", C.c_double),
                ("reserved", C.c_double)]


class Sbv2StreamLevel(C.Structure):
    """struct sbv2_stream_level (include/sbv2_hip.h)."""
    _fields_ = [("gain_db", C.c_double), ("true_peak_max_dbtp", C.c_double), ("reserved", C.c_double * 2)]


class Sbv2StreamLeveler(C.Structure):
    """struct sbv2_stream_leveler (include/sbv2_hip.h)."""
    _fields_ = [("target_lufs", C.c_double), ("range_db", C.c_double), ("slew_db_per_s", C.c_double), ("hold_blocks", C.c_int32),
                ("reserved", C.c_int32)]


class Sbv2StreamRequest(C.Structure):
    """struct sbv2_stream_request (include/sbv2_hip.h)."""
    _fields_ = [("gap_after", i64p), ("fmt", C.POINTER(Sbv2PcmFormat)), ("level", C.POINTER(Sbv2StreamLevel)), ("flac", C.c_int32),
                ("reserved", C.c_int32)]


class Sbv2StreamLevels(C.Structure):
    """struct sbv2_stream_levels (include/sbv2_hip.h)."""
    _fields_ = [("tokens", C.c_int32), ("env_hop", C.c_int32), ("reserved", C.c_int32 * 2)]


class Sbv2StreamMarksPart(C.Structure):
    """struct sbv2_stream_marks_part (include/sbv2_hip.h)."""
    _fields_ = [("tok_capacity", C.c_int64), ("tok_sumsq", C.POINTER(C.c_double)), ("tok_peak", C.POINTER(C.c_double)), ("tok_first", C.c_int64),
                ("n_tok", C.c_int64), ("env_capacity", C.c_int64), ("env_sumsq", C.POINTER(C.c_double)), ("env_peak", C.POINTER(C.c_double)),
                ("env_first", C.c_int64), ("n_env", C.c_int64), ("delivered", C.c_int64)]


class Sbv2StreamPitch(C.Structure):
    """struct sbv2_stream_pitch (include/sbv2_hip.h)."""
    _fields_ = [("hop", C.c_int32), ("reserved", C.c_int32), ("f0_min", C.c_double), ("f0_max", C.c_double), ("threshold", C.c_double)]


class Sbv2StreamPitchPart(C.Structure):
    """struct sbv2_stream_pitch_part (include/sbv2_hip.h)."""
    _fields_ = [("capacity", C.c_int64), ("f0", C.POINTER(C.c_double)), ("ap", C.POINTER(C.c_double)), ("lag", C.POINTER(C.c_int32)),
                ("first", C.c_int64), ("n", C.c_int64), ("delivered", C.c_int64)]


class Sbv2UttOptions(C.Structure):
    """struct sbv2_utt_options (include/sbv2_hip.h)."""
    _fields_ = [("sdp_ratio", f32p), ("length_scale", f32p), ("noise_scale", f32p), ("noise_scale_w", f32p),
                ("noise_seed", C.POINTER(C.c_uint64)), ("noise_index", i64p)]


class Sbv2FetchRequest(C.Structure):
    """struct sbv2_fetch_request (include/sbv2_hip.h)."""
    _fields_ = [("utts", C.POINTER(C.c_int32)), ("n_utts", C.c_int32), ("place", i64p), ("joined_len", C.c_int64),
                ("fmt", C.POINTER(Sbv2PcmFormat)), ("loudness", C.POINTER(Sbv2Loudness)), ("limiter", C.POINTER(Sbv2Limiter)), ("flac", C.c_int32)]


class Sbv2Marks(C.Structure):
    """struct sbv2_marks (include/sbv2_hip.h)."""
    _fields_ = [("tok_capacity", C.c_int64), ("tok_start", i64p), ("tok_end", i64p), ("tok_sumsq", C.POINTER(C.c_double)),
                ("tok_peak", C.POINTER(C.c_double)), ("n_tokens", C.c_int64), ("env_hop", C.c_int32), ("reserved", C.c_int32),
                ("env_capacity", C.c_int64), ("env_sumsq", C.POINTER(C.c_double)), ("env_peak", C.POINTER(C.c_double)), ("n_env", C.c_int64)]


class Sbv2Pitch(C.Structure):
    """struct sbv2_pitch (include/sbv2_hip.h)."""
    _fields_ = [("hop", C.c_int32), ("reserved", C.c_int32), ("f0_min", C.c_double), ("f0_max", C.c_double), ("threshold", C.c_double),
                ("capacity", C.c_int64), ("f0", C.POINTER(C.c_double)), ("ap", C.POINTER(C.c_double)), ("lag", C.POINTER(C.c_int32)),
                ("n_frames", C.c_int64)]


class Sbv2Voice(C.Structure):
    """struct sbv2_voice (include/sbv2_hip.h)."""
    _fields_ = [("pitch_scale", C.c_double), ("intonation_scale", C.c_double), ("f0_min", C.c_double), ("f0_max", C.c_double),
                ("threshold", C.c_double), ("hop", C.c_int32), ("reserved", C.c_int32)]


class Sbv2PitchTrack(C.Structure):
    """struct sbv2_pitch_track (include/sbv2_hip.h)."""
    _fields_ = [("cand_max", C.c_double), ("unvoiced_cost", C.c_double), ("switch_cost", C.c_double), ("jump_cost", C.c_double),
                ("reserved", C.c_int32 * 2)]


class Sbv2TokenPitch(C.Structure):
    """struct sbv2_token_pitch (include/sbv2_hip.h)."""
    _fields_ = [("value", C.POINTER(C.c_double)), ("n_tokens", C.c_int64), ("kind", C.c_int32), ("smooth", C.c_int32),
                ("applied", C.POINTER(C.c_double)), ("src_f0", C.POINTER(C.c_double)), ("reserved", C.c_int64)]


class Sbv2Formant(C.Structure):
    """struct sbv2_formant (include/sbv2_hip.h)."""
    _fields_ = [("formant_scale", C.c_double), ("reserved", C.c_double)]


class Sbv2StreamVoice(C.Structure):
    """struct sbv2_stream_voice (include/sbv2_hip.h)."""
    _fields_ = [("voice", Sbv2Voice), ("formant_scale", C.c_double), ("pivot_hz", C.POINTER(C.c_double)), ("reserved", C.c_double * 2)]


class Sbv2Assist(C.Structure):
    """struct sbv2_assist (include/sbv2_hip.h)."""
    _fields_ = [("n_texts", C.c_int64), ("token_ids", i64p), ("s_lens", i64p), ("text_of", C.POINTER(C.c_int32)), ("weight", C.POINTER(C.c_double)),
                ("reserved", C.c_int64)]


#: every symbol include/sbv2_hip.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "sbv2_last_error": (C.c_char_p, []),
    "sbv2_device_count": (C.c_int, []),
    "sbv2_bert_create": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_void_p)]),
    "sbv2_bert_destroy": (None, [C.c_void_p]),
    "sbv2_bert_hidden": (C.c_int64, [C.c_void_p]),
    "sbv2_bert_gemm_parts": (C.c_int, [C.c_void_p]),
    "sbv2_bert_predict": (C.c_int, [C.c_void_p, i64p, i64p, C.c_int64, f32p]),
    "sbv2_bert_predict_batch": (C.c_int, [C.c_void_p, C.c_int64, i64p, i64p, i64p, f32p]),
    "sbv2_vits_create": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_void_p)]),
    "sbv2_vits_destroy": (None, [C.c_void_p]),
    "sbv2_vits_hop": (C.c_int64, [C.c_void_p]),
    "sbv2_vits_bert_dim": (C.c_int64, [C.c_void_p]),
    "sbv2_vits_style_dim": (C.c_int64, [C.c_void_p]),
    "sbv2_vits_decoder_mode": (C.c_int, [C.c_void_p]),
    "sbv2_vits_workspace_bytes": (C.c_int64, [C.c_void_p]),
    "sbv2_vits_synthesize": (C.c_int, [C.c_void_p, f32p, i64p, i64p, i64p, C.c_int64, C.c_int64, f32p, C.c_float, C.c_float,
                                       C.c_float, C.c_float, C.c_uint64, C.POINTER(f32p), i64p]),
    "sbv2_pcm_free": (None, [f32p]),
    "sbv2_vits_synthesize_batch": (C.c_int, [C.c_void_p, C.POINTER(Sbv2Batch), i64p]),
    "sbv2_vits_fetch_pcm": (C.c_int, [C.c_void_p, f32p, C.c_int64]),
    "sbv2_vits_pcm_device": (C.c_void_p, [C.c_void_p, i64p]),
    "sbv2_vits_copy_pcm_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    "sbv2_sync": (C.c_int, [C.c_void_p]),
    "sbv2_prof_begin": (C.c_int, []),
    "sbv2_prof_end": (C.c_int, [C.c_char_p, C.c_int64]),
    "sbv2_vits_fetch_durations": (C.c_int, [C.c_void_p, i64p, f32p, C.c_int64]),
    "sbv2_vits_set_trace": (C.c_int, [C.c_void_p, C.c_int]),
    "sbv2_vits_get_trace": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int64, f32p, C.c_int64, i64p, i64p]),
    "sbv2_pipeline_create": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]),
    "sbv2_pipeline_destroy": (None, [C.c_void_p]),
    "sbv2_pipeline_run": (C.c_int, [C.c_void_p, C.POINTER(Sbv2Batch), i64p, i64p, i64p, i64p]),
    "sbv2_vits_synthesize_batch_opts": (C.c_int, [C.c_void_p, C.POINTER(Sbv2Batch), C.POINTER(Sbv2UttOptions), i64p]),
    "sbv2_pipeline_run_opts": (C.c_int, [C.c_void_p, C.POINTER(Sbv2Batch), C.POINTER(Sbv2UttOptions), i64p, i64p, i64p, i64p]),
    "sbv2_pipeline_fetch_request": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(Sbv2FetchRequest), C.c_void_p, C.c_int64, i64p, C.POINTER(C.c_double)]),
    "sbv2_pipeline_fetch_request_marks": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(Sbv2FetchRequest), C.c_void_p, C.c_int64, i64p,
                                                    C.POINTER(C.c_double), C.POINTER(Sbv2Marks)]),
    "sbv2_pipeline_fetch_request_pitch": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(Sbv2FetchRequest), C.c_void_p, C.c_int64, i64p,
                                                    C.POINTER(C.c_double), C.POINTER(Sbv2Marks), C.POINTER(Sbv2Pitch)]),
    "sbv2_pitch_lags": (C.c_int, [C.c_int32, C.c_double, C.c_double, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "sbv2_pipeline_fetch_request_voice": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(Sbv2FetchRequest), C.POINTER(Sbv2Voice), C.c_void_p, C.c_int64, i64p,
                                                    C.POINTER(C.c_double), C.POINTER(Sbv2Marks), C.POINTER(Sbv2Pitch)]),
    "sbv2_pipeline_fetch_request_tracked": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(Sbv2FetchRequest), C.POINTER(Sbv2Voice),
                                                      C.POINTER(Sbv2PitchTrack), C.c_void_p, C.c_int64, i64p, C.POINTER(C.c_double),
                                                      C.POINTER(Sbv2Marks), C.POINTER(Sbv2Pitch)]),
    "sbv2_pipeline_fetch_request_dynamics": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(Sbv2FetchRequest), C.POINTER(Sbv2Voice),
                                                       C.POINTER(Sbv2PitchTrack), C.POINTER(Sbv2Dynamics), C.c_void_p, C.c_int64, i64p,
                                                       C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(Sbv2Marks), C.POINTER(Sbv2Pitch)]),
    "sbv2_pipeline_fetch_request_token_pitch": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(Sbv2FetchRequest), C.POINTER(Sbv2Voice),
                                                          C.POINTER(Sbv2PitchTrack), C.POINTER(Sbv2Dynamics), C.POINTER(Sbv2TokenPitch), C.c_void_p,
                                                          C.c_int64, i64p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(Sbv2Marks),
                                                          C.POINTER(Sbv2Pitch)]),
    "sbv2_pipeline_fetch_request_formant": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(Sbv2FetchRequest), C.POINTER(Sbv2Voice),
                                                      C.POINTER(Sbv2PitchTrack), C.POINTER(Sbv2Dynamics), C.POINTER(Sbv2TokenPitch),
                                                      C.POINTER(Sbv2Formant), C.c_void_p, C.c_int64, i64p, C.POINTER(C.c_double),
                                                      C.POINTER(C.c_double), C.POINTER(Sbv2Marks), C.POINTER(Sbv2Pitch)]),
    "sbv2_debug_voice_formant": (C.c_int, [C.c_int, f32p, i64p, C.c_int, C.c_int32, C.POINTER(Sbv2Voice), C.POINTER(Sbv2Formant),
                                           C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_int32),
                                           C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), i64p, f32p]),
    "sbv2_debug_voice_tokens": (C.c_int, [C.c_int, f32p, i64p, C.c_int, C.c_int32, C.POINTER(Sbv2Voice), C.POINTER(C.c_double), C.POINTER(C.c_int32),
                                          i64p, i64p, C.POINTER(Sbv2TokenPitch), C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                          C.POINTER(C.c_int32), C.POINTER(C.c_int32), i64p, f32p, C.POINTER(C.c_double)]),
    "sbv2_dynamics_tile": (C.c_int32, []),
    "sbv2_debug_dynamics": (C.c_int, [C.c_int, C.c_void_p, i64p, C.c_int, C.c_int32, C.POINTER(Sbv2Dynamics), C.POINTER(C.c_double), i64p, i64p,
                                      C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "sbv2_debug_pitch_track": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int64, C.c_int32, C.POINTER(Sbv2Pitch), C.POINTER(Sbv2PitchTrack),
                                         C.POINTER(C.c_int32), C.POINTER(C.c_double), C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_double),
                                         C.POINTER(C.c_int32)]),
    "sbv2_voice_tile": (C.c_int32, []),
    "sbv2_debug_voice_shift": (C.c_int, [C.c_int, f32p, i64p, C.c_int, C.c_int32, C.POINTER(Sbv2Voice), C.POINTER(C.c_double), C.POINTER(C.c_int32),
                                         C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                         C.POINTER(C.c_int32), i64p, f32p]),
    "sbv2_debug_pitch": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int64, C.c_int32, C.POINTER(Sbv2Pitch), C.POINTER(C.c_double),
                                   C.POINTER(C.c_int32)]),
    "sbv2_marks_spans": (C.c_int, [i64p, C.c_int64, C.c_int32, C.c_int64, C.POINTER(Sbv2PcmFormat), i64p, i64p]),
    "sbv2_debug_segment_levels": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int64, i64p, i64p, C.c_int64, C.POINTER(C.c_double),
                                            C.POINTER(C.c_double)]),
    "sbv2_stream_marks": (C.c_int, [C.c_void_p, i64p, i64p, C.c_int64, i64p]),
    "sbv2_pipeline_sync": (C.c_int, [C.c_void_p]),
    "sbv2_pipeline_fetch_pcm": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int]),
    "sbv2_pipeline_fetch_pcm_ticket": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int]),
    "sbv2_pipeline_last_ticket": (C.c_int64, [C.c_void_p]),
    "sbv2_pipeline_wait": (C.c_int, [C.c_void_p, C.c_int64]),
    "sbv2_pcm_format_length": (C.c_int64, [C.POINTER(Sbv2PcmFormat), C.c_int64]),
    "sbv2_g711_encode": (C.c_int, [C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]),
    "sbv2_g711_decode": (C.c_int, [C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]),
    "sbv2_debug_pcm_cast": (C.c_int, [C.c_int, C.c_void_p, i64p, C.c_int, C.POINTER(C.c_double), C.c_int32, C.c_void_p]),
    "sbv2_debug_pcm_format": (C.c_int, [C.c_int, f32p, C.c_int64, i64p, C.c_int, i64p, C.c_int, C.POINTER(Sbv2PcmFormat), C.c_int, C.c_void_p,
                                        C.POINTER(C.c_double)]),
    "sbv2_pcm_format_taps": (C.c_int, [C.c_int32, f32p, C.c_int64, i64p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "sbv2_pipeline_fetch_pcm_format": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(Sbv2PcmFormat), i64p, C.c_int64, C.c_void_p, C.c_int64, i64p]),
    "sbv2_flac_bound": (C.c_int64, [C.POINTER(Sbv2PcmFormat), C.c_int64]),
    "sbv2_pipeline_fetch_flac": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(Sbv2PcmFormat), i64p, C.c_int64, C.c_void_p, C.c_int64, i64p]),
    "sbv2_debug_flac_encode": (C.c_int, [C.c_int, C.c_void_p, i64p, C.c_int, C.c_int32, C.c_void_p, C.c_int64, i64p]),
    "sbv2_pipeline_fetch_pcm_loudness": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(Sbv2PcmFormat), C.POINTER(Sbv2Loudness), i64p, C.c_int64,
                                                   C.c_void_p, C.c_int64, i64p, C.POINTER(C.c_double)]),
    "sbv2_pipeline_fetch_flac_loudness": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(Sbv2PcmFormat), C.POINTER(Sbv2Loudness), i64p, C.c_int64,
                                                    C.c_void_p, C.c_int64, i64p, C.POINTER(C.c_double)]),
    "sbv2_loudness_kweight": (C.c_int, [C.c_int32, C.POINTER(C.c_double)]),
    "sbv2_debug_loudness": (C.c_int, [C.c_int, C.c_void_p, i64p, C.c_int, C.c_int32, C.POINTER(Sbv2Loudness), C.POINTER(C.c_double)]),
    "sbv2_pipeline_fetch_pcm_limited": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(Sbv2PcmFormat), C.POINTER(Sbv2Limiter), i64p, C.c_int64,
                                                  C.c_void_p, C.c_int64, i64p, C.POINTER(C.c_double)]),
    "sbv2_pipeline_fetch_flac_limited": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(Sbv2PcmFormat), C.POINTER(Sbv2Limiter), i64p, C.c_int64,
                                                   C.c_void_p, C.c_int64, i64p, C.POINTER(C.c_double)]),
    "sbv2_debug_limiter": (C.c_int, [C.c_int, C.c_void_p, i64p, C.c_int, C.c_int32, C.POINTER(Sbv2Limiter), C.c_void_p, C.POINTER(C.c_double)]),
    "sbv2_host_alloc": (C.c_void_p, [C.c_size_t]),
    "sbv2_host_free": (None, [C.c_void_p]),
    "sbv2_deal": (C.c_int, [C.c_int64, i64p, C.c_int, C.POINTER(C.c_int32)]),
    "sbv2_gather_plan": (C.c_int, [C.c_int64, i64p, C.POINTER(C.c_int32), C.c_int, i64p, i64p]),
    "sbv2_comm_unique_id": (C.c_int, [C.c_char_p]),
    "sbv2_comm_create": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "sbv2_comm_destroy": (None, [C.c_void_p]),
    "sbv2_comm_rank": (C.c_int, [C.c_void_p]),
    "sbv2_comm_world": (C.c_int, [C.c_void_p]),
    "sbv2_comm_barrier": (C.c_int, [C.c_void_p]),
    "sbv2_comm_max_f64": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "sbv2_comm_gather_pcm": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int64, i64p]),
    "sbv2_node_create": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_void_p)]),
    "sbv2_node_destroy": (None, [C.c_void_p]),
    "sbv2_node_devices": (C.c_int, [C.c_void_p]),
    "sbv2_node_uses_rccl": (C.c_int, [C.c_void_p]),
    "sbv2_node_synthesize": (C.c_int, [C.c_void_p, C.POINTER(Sbv2Batch), i64p, i64p, i64p, i64p, C.c_void_p, C.c_int64]),
    "sbv2_node_last_deal": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_int64]),
    "sbv2_stream_begin": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(Sbv2Batch), i64p, i64p, i64p, C.c_int64, C.POINTER(C.c_void_p), i64p]),
    "sbv2_stream_next": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, i64p]),
    "sbv2_stream_begin_format": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(Sbv2Batch), i64p, i64p, i64p, C.c_int64, C.POINTER(Sbv2PcmFormat),
                                           C.POINTER(C.c_void_p), i64p]),
    "sbv2_stream_next_format": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, i64p]),
    "sbv2_flac_stream_bound": (C.c_int64, [C.POINTER(Sbv2PcmFormat), C.c_int64]),
    "sbv2_stream_begin_flac": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(Sbv2Batch), i64p, i64p, i64p, C.c_int64, C.POINTER(Sbv2PcmFormat),
                                         C.POINTER(C.c_void_p), i64p]),
    "sbv2_stream_next_flac": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, i64p, i64p]),
    "sbv2_debug_flac_stream_encode": (C.c_int, [C.c_int, C.c_void_p, C.c_int64, i64p, C.c_int, C.c_int32, C.c_void_p, C.c_int64, i64p]),
    "sbv2_stream_level_lookahead": (C.c_int64, [C.POINTER(Sbv2PcmFormat)]),
    "sbv2_stream_level_bound": (C.c_int64, [C.POINTER(Sbv2PcmFormat), C.c_int64, C.c_int]),
    "sbv2_stream_begin_level": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(Sbv2Batch), i64p, i64p, i64p, C.c_int64, C.POINTER(Sbv2PcmFormat),
                                          C.POINTER(Sbv2StreamLevel), C.c_int, C.POINTER(C.c_void_p), i64p]),
    "sbv2_stream_next_level": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, i64p, i64p]),
    "sbv2_stream_level_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "sbv2_debug_limiter_fixed": (C.c_int, [C.c_int, C.c_void_p, i64p, C.c_int, C.c_int32, C.POINTER(Sbv2StreamLevel), C.c_void_p,
                                           C.POINTER(C.c_double)]),
    "sbv2_debug_limiter_stream": (C.c_int, [C.c_int, C.c_void_p, C.c_int64, i64p, C.c_int, C.c_int32, C.POINTER(Sbv2StreamLevel), C.c_void_p, i64p,
                                            C.POINTER(C.c_double)]),
    "sbv2_debug_loudness_parts": (C.c_int, [C.c_int, C.c_void_p, i64p, C.c_int, C.c_int32, C.POINTER(C.c_double), C.c_int64, C.c_int64] +
                                  [C.POINTER(C.c_double)] * 6 + [i64p]),
    "sbv2_debug_limiter_parts": (C.c_int, [C.c_int, C.c_void_p, i64p, C.c_int, C.c_int32, C.POINTER(Sbv2StreamLevel), C.c_int64] +
                                 [C.POINTER(C.c_double)] * 5 + [i64p]),
    "sbv2_stream_begin_request": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(Sbv2Batch), C.POINTER(Sbv2UttOptions), i64p, i64p, i64p, C.c_int64,
                                            C.POINTER(Sbv2StreamRequest), C.POINTER(C.c_void_p), i64p]),
    "sbv2_stream_begin_request_levels": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(Sbv2Batch), C.POINTER(Sbv2UttOptions), i64p, i64p, i64p, C.c_int64,
                                                   C.POINTER(Sbv2StreamRequest), C.POINTER(Sbv2StreamLevels), C.POINTER(C.c_void_p), i64p, i64p, i64p]),
    "sbv2_stream_next_marks": (C.c_int, [C.c_void_p, C.POINTER(Sbv2StreamMarksPart)]),
    "sbv2_debug_stream_levels": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int64, i64p, C.c_int, i64p, i64p, C.c_int64, C.c_int32,
                                           C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), i64p, i64p]),
    "sbv2_stream_begin_request_pitch": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(Sbv2Batch), C.POINTER(Sbv2UttOptions), i64p, i64p, i64p, C.c_int64,
                                                  C.POINTER(Sbv2StreamRequest), C.POINTER(Sbv2StreamLevels), C.POINTER(Sbv2StreamPitch),
                                                  C.POINTER(C.c_void_p), i64p, i64p, i64p, i64p]),
    "sbv2_pipeline_run_assist": (C.c_int, [C.c_void_p, C.POINTER(Sbv2Batch), C.POINTER(Sbv2UttOptions), C.POINTER(Sbv2Assist), i64p, i64p, i64p, i64p]),
    "sbv2_stream_begin_request_assist": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(Sbv2Batch), C.POINTER(Sbv2UttOptions), C.POINTER(Sbv2Assist), i64p, i64p,
                                                   i64p, C.c_int64, C.POINTER(Sbv2StreamRequest), C.POINTER(Sbv2StreamLevels), C.POINTER(Sbv2StreamPitch),
                                                   C.POINTER(C.c_void_p), i64p, i64p, i64p, i64p]),
    "sbv2_stream_begin_request_voice": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(Sbv2Batch), C.POINTER(Sbv2UttOptions), C.POINTER(Sbv2Assist), i64p, i64p,
                                                  i64p, C.c_int64, C.POINTER(Sbv2StreamRequest), C.POINTER(Sbv2StreamLevels), C.POINTER(Sbv2StreamPitch),
                                                  C.POINTER(Sbv2StreamVoice), C.POINTER(C.c_void_p), i64p, i64p, i64p, i64p]),
    "sbv2_stream_begin_request_leveler": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(Sbv2Batch), C.POINTER(Sbv2UttOptions), C.POINTER(Sbv2Assist), i64p,
                                                    i64p, i64p, C.c_int64, C.POINTER(Sbv2StreamRequest), C.POINTER(Sbv2StreamLevels),
                                                    C.POINTER(Sbv2StreamPitch), C.POINTER(Sbv2StreamVoice), C.POINTER(Sbv2StreamLeveler),
                                                    C.POINTER(C.c_void_p), i64p, i64p, i64p, i64p]),
    "sbv2_stream_leveler_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "sbv2_debug_leveler_stream": (C.c_int, [C.c_int, C.c_void_p, C.c_int64, i64p, C.c_int, C.c_int32, C.POINTER(Sbv2StreamLevel),
                                            C.POINTER(Sbv2StreamLeveler), C.c_void_p, i64p, C.POINTER(C.c_double), C.c_int64, C.POINTER(C.c_double)]),
    "sbv2_stream_voice_lookahead": (C.c_int64, [C.POINTER(Sbv2StreamVoice), C.c_int32]),
    "sbv2_stream_voice_timeline": (C.c_int, [i64p, i64p, C.c_int64, C.c_int32, C.c_int64, C.POINTER(Sbv2PcmFormat), C.POINTER(Sbv2StreamVoice), i64p,
                                             C.c_int64, i64p]),
    "sbv2_debug_voice_stream": (C.c_int, [C.c_int, f32p, C.c_int64, i64p, C.c_int, C.c_int32, C.POINTER(Sbv2StreamVoice), C.POINTER(C.c_double),
                                          C.POINTER(C.c_int32), f32p, i64p]),
    "sbv2_debug_assist_blend": (C.c_int, [C.c_int, f32p, C.c_int64, C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int64, C.c_int64,
                                          C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_double), f32p, f32p,
                                          i64p]),
    "sbv2_stream_next_pitch": (C.c_int, [C.c_void_p, C.POINTER(Sbv2StreamPitchPart)]),
    "sbv2_debug_stream_pitch": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int64, i64p, C.c_int, C.c_int32, C.POINTER(Sbv2Pitch),
                                          C.POINTER(C.c_double), C.POINTER(C.c_int32), i64p]),
    "sbv2_stream_min_gap": (C.c_int64, [C.POINTER(Sbv2PcmFormat)]),
    "sbv2_stream_timeline": (C.c_int, [i64p, i64p, C.c_int64, C.c_int32, C.c_int64, C.POINTER(Sbv2PcmFormat), i64p, i64p, i64p, C.c_int64, i64p]),
    "sbv2_stream_layout": (C.c_int, [C.c_void_p, i64p, i64p, C.c_int64, i64p, i64p]),
    "sbv2_stream_call_bound": (C.c_int64, [C.c_void_p]),
    "sbv2_debug_stream_windows": (C.c_int, [C.c_int, f32p, C.c_int64, C.c_int64, C.POINTER(C.c_int32), C.c_int64, C.c_int64, f32p, C.c_int64, C.c_int64,
                                            f32p, C.c_void_p, f32p]),
    "sbv2_stream_uses_graph": (C.c_int, [C.c_void_p]),
    "sbv2_stream_workspace_bytes": (C.c_int64, [C.c_void_p]),
    "sbv2_stream_end": (None, [C.c_void_p]),
    "sbv2_parse_sbv2file": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "sbv2_bytes_free": (None, [C.c_void_p]),
    "sbv2_style_load": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p), i64p, i64p]),
    "sbv2_aivmx_style_vectors": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p), i64p, i64p]),
    "sbv2_style_vector": (C.c_int, [f32p, C.c_int64, C.c_int64, C.c_int64, C.c_float, f32p]),
    "sbv2_debug_import_to_container": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "sbv2_debug_bucket_table": (C.c_int, [C.c_int64, C.c_int64, C.c_int64, C.POINTER(C.c_int32)]),
    "sbv2_debug_conv1d": (C.c_int, [C.c_int, f32p, f32p, f32p, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_float, f32p]),
    "sbv2_debug_conv_transpose1d": (C.c_int, [C.c_int, f32p, f32p, f32p, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64,
                                              C.c_int64, C.c_float, f32p]),
    "sbv2_debug_conv1d_cl": (C.c_int, [C.c_int, f32p, f32p, f32p, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_float, C.c_int,
                                       C.c_int64, f32p, f32p]),
    "sbv2_debug_time_conv1d": (C.c_int, [C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, f32p]),
    "sbv2_debug_set_skinny_max": (C.c_int, [C.c_int]),
    "sbv2_debug_set_clx": (C.c_int, [C.c_int]),
    "sbv2_debug_set_ksplit": (C.c_int, [C.c_int]),
    "sbv2_debug_set_flash_parts": (C.c_int, [C.c_int]),
    "sbv2_debug_set_sdp_all": (C.c_int, [C.c_int]),
    "sbv2_debug_conv1d_clx": (C.c_int, [C.c_int, f32p, f32p, f32p, f32p, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_float, C.c_float,
                                        C.c_int64, f32p, f32p, f32p]),
    "sbv2_debug_set_respair_clx": (C.c_int, [C.c_int]),
    "sbv2_debug_f16x3_saturation": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_uint64)]),
    "sbv2_debug_respair": (C.c_int, [C.c_int, f32p, f32p, f32p, f32p, f32p, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_float, C.c_int,
                                     C.c_int, f32p]),
    "sbv2_debug_set_resbranch": (C.c_int, [C.c_int]),
    "sbv2_debug_set_upx": (C.c_int, [C.c_int]),
    "sbv2_debug_conv_transpose1d_clx": (C.c_int, [C.c_int, f32p, f32p, f32p, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_float, C.c_void_p,
                                                  C.c_int64, C.c_int64, f32p, f32p, f32p]),
    "sbv2_debug_resbranch": (C.c_int, [C.c_int, f32p, f32p, f32p, C.c_int64, C.c_int64, C.c_int64, i64p, C.c_void_p, C.c_int64, C.c_float, C.c_int, C.c_int,
                                       C.c_int64, f32p, f32p]),
    "sbv2_debug_resbranch_ys": (C.c_int, [C.c_int, f32p, f32p, f32p, C.c_int64, C.c_int64, C.c_int64, i64p, C.c_void_p, C.c_int64, C.c_float, C.c_int,
                                          C.c_int64, f32p, f32p, f32p, f32p, f32p]),
    "sbv2_debug_gemm_bfs_alt": (C.c_int, [C.c_int, f32p, f32p, f32p, f32p, f32p, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_int64, f32p, f32p]),
    "sbv2_debug_repeat_respair": (C.c_int, [C.c_int, f32p, f32p, f32p, f32p, f32p, f32p, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_int64,
                                            C.c_float, f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, f32p, f32p, i64p, i64p]),
    "sbv2_debug_repeat_resbranch": (C.c_int, [C.c_int, f32p, f32p, f32p, f32p, C.c_int64, C.c_int64, C.c_int64, i64p, C.c_void_p, C.c_int64, C.c_float, f32p,
                                              C.c_int, C.c_int, C.c_int, C.c_int64, f32p, f32p, i64p, i64p]),
    "sbv2_debug_repeat_conv1d_clx": (C.c_int, [C.c_int, f32p, f32p, f32p, f32p, f32p, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_float,
                                               C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, f32p, f32p, f32p, f32p, i64p, i64p]),
    "sbv2_debug_repeat_conv_transpose1d_clx": (C.c_int, [C.c_int, f32p, f32p, f32p, f32p, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_float,
                                                         C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, f32p, f32p, f32p, f32p, i64p,
                                                         i64p]),
    "sbv2_debug_repeat_gemm_bfs": (C.c_int, [C.c_int, f32p, f32p, f32p, f32p, f32p, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int,
                                             C.c_int, C.c_int64, f32p, f32p, f32p, f32p, i64p, i64p]),
    "sbv2_debug_repeat_vits_attention": (C.c_int, [C.c_int, f32p, f32p, f32p, f32p, f32p, f32p, f32p, f32p, i64p, C.c_int, C.c_int64, C.c_int64, C.c_int64,
                                                   C.c_int, C.c_int, C.c_int, C.c_int64, f32p, f32p, i64p, i64p, i64p]),
    "sbv2_debug_repeat_conv_ffn_clx": (C.c_int, [C.c_int, f32p, f32p, f32p, f32p, f32p, f32p, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_int,
                                                 C.c_int, C.c_int, C.c_int64, f32p, f32p, i64p, i64p]),
    "sbv2_debug_gemm_bfs": (C.c_int, [C.c_int, f32p, f32p, f32p, f32p, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int64,
                                      f32p, f32p]),
    "sbv2_debug_conv_plain": (C.c_int, [C.c_int, f32p, f32p, f32p, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_void_p,
                                        C.c_int64, C.c_int, C.c_float, f32p, C.c_float, C.c_float, C.c_int, f32p, i64p]),
    "sbv2_debug_conv_ffn_cl": (C.c_int, [C.c_int, f32p, f32p, f32p, f32p, f32p, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, f32p, f32p, f32p,
                                         i64p]),
    "sbv2_debug_gemm_bfs_ex": (C.c_int, [C.c_int, f32p, f32p, f32p, f32p, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_void_p,
                                         C.c_int64, C.c_float, C.c_float, C.c_int64, C.c_int64, C.c_int, f32p, f32p, f32p, i64p]),
    "sbv2_debug_linear_tokmajor": (C.c_int, [C.c_int, f32p, f32p, f32p, C.c_int64, C.c_int64, C.c_int64, C.c_int64, f32p, i64p]),
    "sbv2_debug_vits_attention": (C.c_int, [C.c_int, f32p, f32p, f32p, f32p, f32p, i64p, C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_int,
                                            C.c_int, f32p, i64p]),
    "sbv2_debug_deberta_attention": (C.c_int, [C.c_int, f32p, f32p, f32p, f32p, f32p, i64p, C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_int64,
                                               C.c_void_p, C.c_int64, C.c_int, C.c_int, f32p, i64p]),
    "sbv2_debug_layout": (C.c_int, [i64p, C.c_int, C.c_int, C.POINTER(C.c_int32), i64p]),
    "sbv2_debug_layernorm": (C.c_int, [C.c_int, f32p, f32p, f32p, C.c_float, C.c_int, f32p, C.c_void_p, f32p, f32p, C.c_int64, C.c_int64, C.c_int64, C.c_int,
                                       C.c_int, C.c_int, f32p, f32p, i64p]),
    "sbv2_debug_deberta_embed_ln": (C.c_int, [C.c_int, C.POINTER(C.c_int32), f32p, C.c_int64, C.c_int64, f32p, f32p, C.c_float, C.c_int64, C.c_int, f32p,
                                              i64p]),
    "sbv2_debug_spline_inverse": (C.c_int, [C.c_int, f32p, f32p, C.c_void_p, C.c_int64, C.c_int64, C.c_float, C.c_float, C.c_int, f32p, i64p]),
    "sbv2_debug_durations": (C.c_int, [C.c_int, f32p, f32p, C.c_void_p, C.c_int64, C.c_float, C.c_float, f32p, C.POINTER(C.c_int32), i64p]),
    "sbv2_debug_durations_rows": (C.c_int, [C.c_int, f32p, f32p, C.c_void_p, i64p, C.c_int, f32p, f32p, f32p, C.POINTER(C.c_int32), i64p]),
    "sbv2_debug_affine_reverse": (C.c_int, [C.c_int, f32p, f32p, f32p, f32p, C.c_void_p, C.c_int64, f32p, i64p]),
    "sbv2_debug_convflow_pre": (C.c_int, [C.c_int, f32p, f32p, f32p, f32p, C.c_void_p, C.c_int64, C.c_int64, f32p, i64p]),
    "sbv2_debug_noise_fill": (C.c_int, [C.c_int, i64p, C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_uint64, C.c_int, C.c_float, C.c_int64, f32p, i64p]),
    "sbv2_debug_expand_frames": (C.c_int, [C.c_int, f32p, f32p, C.c_int64, C.c_int64, C.POINTER(C.c_int32), i64p, C.c_int, C.POINTER(C.c_int32), C.c_uint64,
                                           C.c_float, f32p, i64p]),
    "sbv2_debug_noise_fill_rows": (C.c_int, [C.c_int, i64p, C.c_int, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_int32), C.c_int, f32p, C.c_int64, f32p,
                                             i64p]),
    "sbv2_debug_expand_frames_rows": (C.c_int, [C.c_int, f32p, f32p, C.c_int64, C.c_int64, C.POINTER(C.c_int32), i64p, C.c_int, C.POINTER(C.c_uint64),
                                                C.POINTER(C.c_int32), f32p, f32p, i64p]),
    "sbv2_debug_conv_post_tanh": (C.c_int, [C.c_int, f32p, f32p, C.c_int64, C.c_int64, i64p, C.c_int, C.c_int64, C.c_int, f32p, i64p]),
    "sbv2_debug_linear_vec": (C.c_int, [C.c_int, f32p, f32p, C.c_int64, C.c_int64, f32p, C.c_int64, f32p]),
    "sbv2_debug_gather_rows": (C.c_int, [C.c_int, f32p, C.c_int64, C.c_int64, C.POINTER(C.c_int32), C.c_int64, f32p]),
    "sbv2_debug_text_embed": (C.c_int, [C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), i64p, C.c_int, f32p, C.c_int64, f32p,
                                        C.c_int64, f32p, C.c_int64, f32p, f32p, C.c_float, C.c_int64, f32p, i64p]),
    "sbv2_debug_add_segvec": (C.c_int, [C.c_int, f32p, f32p, C.c_int64, i64p, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_int, C.c_int, f32p, i64p]),
    "sbv2_debug_plane_op": (C.c_int, [C.c_int, C.c_int, f32p, C.c_int64, C.c_int64, C.POINTER(C.c_int32), C.c_int64, C.c_int64, f32p, C.c_void_p, i64p]),
    "sbv2_debug_copy_segments": (C.c_int, [C.c_int, f32p, C.c_int64, i64p, C.c_int, f32p, C.c_int64]),
}

_lib = None


class Sbv2Error(RuntimeError):
    """Mirror of sbv2_core::error::Error::OtherError (crates/sbv2_core/src/error.rs:29-30)."""


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise Sbv2Error(f"{LIB_PATH} is missing: build it with __graft_entry__.build() (there is no CPU fallback)")
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(l, name)   # AttributeError here = the library does not export what the header declares
            fn.restype = res
            fn.argtypes = args
        _lib = l
    return _lib


def check(rc):
    if rc != 0:
        raise Sbv2Error(lib().sbv2_last_error().decode(errors="replace"))
