"""ctypes binding of libqasr.so (the C ABI in include/qasr.h).  No torch types cross it."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), "lib", "libqasr.so")


class QasrConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("enc_d_model", "enc_heads", "enc_ffn", "enc_layers", "n_mels",
                                         "enc_out_dim", "conv_channels", "n_window", "n_window_infer")] + \
               [("ln_eps", C.c_float)] + \
               [(n, C.c_int32) for n in ("vocab", "hidden", "dec_layers", "heads", "kv_heads", "head_dim", "inter")] + \
               [("rms_eps", C.c_float), ("rope_theta", C.c_float), ("group_size", C.c_int32), ("bits", C.c_int32)] + \
               [(n, C.c_int32) for n in ("tok_im_start", "tok_im_end", "tok_audio_start", "tok_audio_end",
                                         "tok_audio_pad", "tok_asr_text", "tok_newline", "tok_system",
                                         "tok_user", "tok_assistant")] + \
               [("fft_scale", C.c_float)] + \
               [(n, C.c_int32) for n in ("device", "max_batch", "max_audio_seconds", "max_new_tokens",
                                         "max_prompt_extra", "classify_num", "tok_timestamp")] + \
               [("timestamp_segment_time", C.c_float)]


class QasrCtcConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("model_dim", "layers", "heads", "ffn_dim", "feature_dim", "pos_kernel", "pos_groups",
                                         "vocab", "group_size", "bits")] + \
               [("ln_eps", C.c_float)] + \
               [(n, C.c_int32) for n in ("device", "max_batch", "max_audio_seconds")]


class QasrOptions(C.Structure):
    _fields_ = [("max_tokens", C.c_int32), ("ignore_eos", C.c_int32),
                ("context_ids", C.POINTER(C.c_int32)), ("n_context", C.c_int32),
                ("language_ids", C.POINTER(C.c_int32)), ("n_language", C.c_int32),
                ("repetition_penalty", C.c_float), ("no_repeat_ngram_size", C.c_int32),
                ("temperature", C.c_float), ("seed", C.c_uint64)]


class QasrResult(C.Structure):
    _fields_ = [("text", C.c_char_p), ("tokens", C.POINTER(C.c_int32)), ("n_tokens", C.c_int32)]


class ScTranscriptionResult(C.Structure):
    _fields_ = [("text", C.c_char_p), ("language", C.c_char_p), ("confidence", C.c_float),
                ("start_time", C.c_float), ("end_time", C.c_float)]


class QasrAlignedWord(C.Structure):
    _fields_ = [("text", C.c_char_p), ("start_time", C.c_float), ("end_time", C.c_float)]


class QasrAlignment(C.Structure):
    _fields_ = [("words", C.POINTER(QasrAlignedWord)), ("n_words", C.c_size_t),
                ("raw_indices", C.POINTER(C.c_int32)), ("n_indices", C.c_size_t), ("passes", C.c_int32)]


class QasrTransducerConfig(C.Structure):
    _fields_ = [("vocab_size", C.c_int32), ("blank_id", C.c_int32), ("eou_id", C.c_int32), ("n_durations", C.c_int32),
                ("durations", C.c_int32 * 8), ("first_text_id", C.c_int32), ("max_symbols", C.c_int32)]


TD_DECODER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int32)
TD_JOINT_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_float))


class QasrTransducerCallbacks(C.Structure):
    _fields_ = [("ctx", C.c_void_p), ("decoder_step", TD_DECODER_FN), ("joint", TD_JOINT_FN)]


class QasrTtsConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("hidden", "layers", "heads", "kv_heads", "head_dim", "inter", "text_vocab", "text_hidden",
                                         "codec_vocab", "cp_hidden", "cp_embedding_dim", "cp_layers", "cp_heads", "cp_kv_heads",
                                         "cp_head_dim", "cp_inter", "cp_vocab")] + \
               [(n, C.c_float) for n in ("rms_eps", "rope_theta", "cp_rms_eps", "cp_rope_theta")] + \
               [(n, C.c_int32) for n in ("bits", "group_size", "codec_pad", "codec_bos", "codec_eos", "codec_think", "codec_nothink",
                                         "codec_think_bos", "codec_think_eos", "suppress_lo", "suppress_hi", "tts_pad", "tts_bos",
                                         "tts_eos", "max_batch", "max_frames", "max_text", "max_instruct", "device")]


class QasrTtsSampling(C.Structure):
    _fields_ = [("temperature", C.c_float), ("top_k", C.c_int32), ("top_p", C.c_float), ("repetition_penalty", C.c_float),
                ("max_tokens", C.c_int32), ("eos_logit_bias", C.c_float)]


class QasrTtsRequest(C.Structure):
    _fields_ = [("B", C.c_size_t), ("text", C.POINTER(C.POINTER(C.c_int32))), ("text_len", C.POINTER(C.c_int32)),
                ("language", C.POINTER(C.c_int32)), ("speaker", C.POINTER(C.c_int32)),
                ("xvector", C.POINTER(C.POINTER(C.c_float))), ("instruct", C.POINTER(C.POINTER(C.c_int32))),
                ("instruct_len", C.POINTER(C.c_int32)), ("row_index", C.POINTER(C.c_int64))]


class QasrCvlmConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("hidden", "layers", "heads", "kv_heads", "head_dim", "inter", "text_vocab", "speech_tokens",
                                         "speech_extra")] + \
               [(n, C.c_float) for n in ("rms_eps", "rope_theta")] + \
               [(n, C.c_int32) for n in ("bits", "group_size", "device", "max_batch", "max_text", "max_prompt_tokens", "max_tokens")]


class QasrCvlmSampling(C.Structure):
    _fields_ = [("top_k", C.c_int32), ("top_p", C.c_float), ("win_size", C.c_int32), ("tau_r", C.c_float), ("min_ratio", C.c_float)]


class QasrCvlmRequest(C.Structure):
    _fields_ = [("B", C.c_size_t), ("text", C.POINTER(C.POINTER(C.c_int32))), ("text_len", C.POINTER(C.c_int32)),
                ("prompt", C.POINTER(C.POINTER(C.c_int32))), ("prompt_len", C.POINTER(C.c_int32)),
                ("content_len", C.POINTER(C.c_int32)), ("max_tokens", C.POINTER(C.c_int32)), ("row_index", C.POINTER(C.c_int64))]


class QasrTtsIcl(C.Structure):
    _fields_ = [("ref_text", C.POINTER(C.POINTER(C.c_int32))), ("ref_text_len", C.POINTER(C.c_int32)),
                ("ref_codes", C.POINTER(C.POINTER(C.c_int32))), ("ref_frames", C.POINTER(C.c_int32))]


class QasrTtsStreamConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("first_chunk_frames", "chunk_frames", "decoder_left_context")]


class QasrTtsChunk(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("stream", "frame_index", "n_frames", "is_final")] + \
               [("samples", C.POINTER(C.c_float)), ("n_samples", C.c_size_t), ("codes", C.POINTER(C.c_int32))]


SC_TRANSCRIBE_FN = C.CFUNCTYPE(ScTranscriptionResult, C.c_void_p, C.POINTER(C.c_float), C.c_size_t, C.c_int)
SC_RATE_FN = C.CFUNCTYPE(C.c_int32, C.c_void_p)


class ScSttVtable(C.Structure):
    _fields_ = [("context", C.c_void_p), ("transcribe", SC_TRANSCRIBE_FN), ("input_sample_rate", SC_RATE_FN),
                ("begin_stream", C.c_void_p), ("push_chunk", C.c_void_p), ("flush_stream", C.c_void_p),
                ("end_stream", C.c_void_p), ("cancel_stream", C.c_void_p)]


class QasrVadConfig(C.Structure):
    _fields_ = [("onset", C.c_float), ("offset", C.c_float), ("min_speech_duration", C.c_float), ("min_silence_duration", C.c_float)]


class QasrSegVadConfig(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("onset", "offset", "min_speech_duration", "min_silence_duration", "window_duration", "step_ratio")]


class QasrSepConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("wiener", "wiener_iterations", "wiener_window")]


class QasrDiarConfig(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("onset", "offset", "min_speech_duration", "min_silence_duration", "clustering_threshold")]


class QasrDiarSegment(C.Structure):
    _fields_ = [("start_time", C.c_float), ("end_time", C.c_float), ("speaker_id", C.c_int32)]


VAD_PROCESS_FN = C.CFUNCTYPE(C.c_float, C.c_void_p, C.POINTER(C.c_float), C.c_size_t)
VAD_RESET_FN = C.CFUNCTYPE(None, C.c_void_p)
VAD_CHUNK_FN = C.CFUNCTYPE(C.c_size_t, C.c_void_p)


class ScVadVtable(C.Structure):
    _fields_ = [("context", C.c_void_p), ("process_chunk", VAD_PROCESS_FN), ("reset", VAD_RESET_FN),
                ("input_sample_rate", SC_RATE_FN), ("chunk_size", VAD_CHUNK_FN)]


class QasrGemmCase(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("M", "N", "K", "ld", "out_rows", "n_img", "H", "W", "C", "wide", "hw_major", "level", "a_len",
                                         "KP", "cpg", "groups", "n_t")]


class QasrAttnCase(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("n_slots", "heads", "kv_heads", "hd", "max_ctx", "n_pos", "n_clips", "route", "hidden")] + \
               [("eps", C.c_float), ("rope_theta", C.c_float)]


class QasrSynAttnCase(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("heads", "kv_heads", "rows", "out_rows", "n_slots", "max_ctx", "pos", "S", "n_seq", "n_table")] + \
               [(n, C.c_int64) for n in ("qkv_elems", "cache_elems", "out_elems", "table_elems")] + [("eps", C.c_float)]


class QasrCodecCase(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("rows_kind", "snake", "epi", "M", "a_rows", "out_extra", "Cin", "taps", "dil", "K", "N", "bmod", "ldc",
                                         "rate", "stride", "lead", "n_clips", "n_loc", "in_place", "C", "Q", "S0", "S1", "clip", "heads", "hd", "n_table")] + [("eps", C.c_float)]


class QasrEncCase(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("rows", "n_clips", "in_extra", "out_extra", "heads", "hd", "max_len", "D", "ld", "n_in", "n_mels",
                                         "mel_stride", "H1", "W1", "stride")] + [("eps", C.c_float)]


class QasrDecCase(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("B", "N", "K", "epi", "generic", "bits", "sb_f32", "in_extra", "out_extra", "part_cap")] + \
               [("eps", C.c_float)] + [(n, C.c_int32) for n in ("n_parts", "route", "max_new", "max_tokens", "eos", "ignore_eos", "advance_ctx",
                                                                "clear_words", "n_rope", "half", "n_audio", "r0")]


class QasrVlocGeometry(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("patch_size", "feat_dim", "lm_hidden", "enc_hidden", "dit_hidden", "enc_layers", "dit_layers", "mu_dim",
                                         "kv_heads")] + [("stored_bytes", C.c_size_t)]


_P = C.POINTER
_F = _P(C.c_float)
_I = _P(C.c_int32)
_E = C.c_void_p

# name -> (restype, argtypes); mirrors include/qasr.h one to one
SIGNATURES = {
    "qasr_default_config": (C.c_int, [C.c_char_p, _P(QasrConfig)]),
    "qasr_create": (C.c_int, [C.c_char_p, _P(QasrConfig), _P(_E)]),
    "qasr_set_tensor": (C.c_int, [_E, C.c_char_p, C.c_void_p, C.c_int, _P(C.c_int64), C.c_int]),
    "qasr_finalize": (C.c_int, [_E]),
    "qasr_set_vocab": (C.c_int, [_E, _I, _P(C.c_char_p), C.c_size_t]),
    "qasr_is_loaded": (C.c_int, [_E]),
    "qasr_unload": (C.c_int, [_E]),
    "qasr_memory_footprint": (C.c_size_t, [_E]),
    "qasr_destroy": (None, [_E]),
    "qasr_last_error": (C.c_char_p, [_E]),
    "qasr_input_sample_rate": (C.c_int, [_E]),
    "qasr_load_wav": (C.c_int, [C.c_char_p, _P(_F), _P(C.c_size_t), _P(C.c_int)]),
    "qasr_free": (None, [C.c_void_p]),
    "qasr_transcribe": (C.c_int, [_E, _F, C.c_size_t, C.c_int, _P(QasrOptions), _P(QasrResult)]),
    "qasr_transcribe_batch": (C.c_int, [_E, _P(_F), _P(C.c_size_t), C.c_size_t, C.c_int, _P(QasrOptions), _I, _I]),
    "qasr_detokenize": (C.c_int, [_E, _I, C.c_int32, C.c_char_p, C.c_size_t]),
    "qasr_stt_vtable": (C.c_int, [_E, _P(ScSttVtable)]),
    "qasr_encode_text": (C.c_int, [_E, C.c_char_p, _I, C.c_int32]),
    "qasr_set_merges": (C.c_int, [_E, C.c_char_p]),
    "qasr_pick_next_token": (C.c_int32, [_F, C.c_int32, _I, C.c_int32, C.c_float, C.c_int32, C.c_float, _P(C.c_uint64)]),
    "qasr_batch_begin": (C.c_int, [_E, _P(_F), _P(C.c_size_t), C.c_size_t, _P(QasrOptions)]),
    "qasr_batch_stage": (C.c_int, [_E, _P(_F), _P(C.c_size_t), C.c_size_t]),
    "qasr_batch_begin_staged": (C.c_int, [_E, _P(QasrOptions)]),
    "qasr_batch_run": (C.c_int, [_E]),
    "qasr_batch_rewind": (C.c_int, [_E]),
    "qasr_batch_sync": (C.c_int, [_E]),
    "qasr_batch_tokens": (C.c_int, [_E, _I, _I]),
    "qasr_batch_timings": (C.c_int, [_E, _F, _I]),
    "qasr_kernel_probe": (C.c_int, [_E, C.c_int, C.c_int, _F, _P(C.c_double)]),
    "qasr_gemm_probe": (C.c_int, [_E, _P(C.c_uint16), _P(C.c_uint16), _F, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _F, _F]),
    "qasr_gemm_case_probe": (C.c_int, [_E, C.c_int, C.c_int, _P(QasrGemmCase), _P(C.c_uint16), _P(C.c_uint16), C.c_void_p, _I, _P(C.c_int64),
                                       _F, C.c_void_p]),
    "qasr_attn_case_probe": (C.c_int, [_E, C.c_int, _P(QasrAttnCase)] + [_P(C.c_uint16)] * 3 + [_I] * 4 + [_P(C.c_uint16)] * 7),
    "qasr_syn_attn_case_probe": (C.c_int, [_E, C.c_int, _P(QasrSynAttnCase), C.c_void_p, _I, _I, _P(C.c_uint16), _P(C.c_uint16), _F, _F] +
                                 [_P(C.c_uint16)] * 3 + [C.c_void_p]),
    "qasr_codec_case_probe": (C.c_int, [_E, C.c_int, _P(QasrCodecCase)] + [_F] * 7 + [_I, _I, _F]),
    "qasr_enc_case_probe": (C.c_int, [_E, C.c_int, _P(QasrEncCase), C.c_void_p, _I, _P(C.c_int64), _F, _P(C.c_uint16), C.c_void_p]),
    "qasr_dec_case_probe": (C.c_int, [_E, C.c_int, _P(QasrDecCase), _P(C.c_uint16)] + [C.c_void_p] * 3 + [_P(C.c_uint16)] * 2 + [_F, _F, _I, _I, _F, _F]),
    "qasr_set_shared_device": (C.c_int, [_E, C.c_int]),
    "qasr_decode_structure": (C.c_int, [_E, _P(C.c_int), _P(C.c_int), _P(C.c_int)]),
    "qasr_set_tuning": (C.c_int, [C.c_char_p, C.c_int]),
    "qasr_get_tuning": (C.c_int, [C.c_char_p, _P(C.c_int)]),
    "qasr_num_mel_frames": (C.c_int, [C.c_size_t]),
    "qasr_num_audio_tokens": (C.c_int, [_E, C.c_int]),
    "qasr_mel": (C.c_int, [_E, _F, C.c_size_t, _F]),
    "qasr_encode": (C.c_int, [_E, _F, C.c_int, _F]),
    "qasr_prefill_logits": (C.c_int, [_E, _F, C.c_int, _P(QasrOptions), _F]),
    "qasr_decode_forced": (C.c_int, [_E, _I, C.c_int, _F]),
    "qasr_batch_prefill_logits": (C.c_int, [_E, _F]),
    "qasr_batch_decode_forced": (C.c_int, [_E, _I, _F]),
    "qasr_split_words": (C.c_int, [C.c_char_p, C.c_char_p, _P(C.c_void_p), _P(C.c_void_p)]),
    "qasr_lis_positions": (C.c_int, [_I, C.c_size_t, _I]),
    "qasr_enforce_monotonicity": (C.c_int, [_I, C.c_size_t, _I]),
    "qasr_find_trailing_plateau": (C.c_int, [_F, C.c_size_t, C.c_float, C.c_int32]),
    "qasr_align_prepare": (C.c_int, [_E, C.c_char_p, C.c_char_p, _I, C.c_int32, _I, C.c_int32, _I, _I]),
    "qasr_align_raw": (C.c_int, [_E, _F, C.c_size_t, _I, C.c_int32, _I, C.c_int32, _I, _F]),
    "qasr_align": (C.c_int, [_E, _F, C.c_size_t, C.c_int, C.c_char_p, C.c_char_p, _P(QasrAlignment)]),
    "qasr_align_words": (C.c_int, [_E, _F, C.c_size_t, C.c_int, _P(C.c_char_p), _P(C.c_char_p), C.c_size_t, _P(QasrAlignment)]),
    "qasr_align_batch": (C.c_int, [_E, _P(_F), _P(C.c_size_t), C.c_size_t, C.c_int, _P(C.c_char_p), C.c_char_p, _P(QasrAlignment)]),
    "qasr_align_long": (C.c_int, [_E, _F, C.c_size_t, C.c_int, C.c_char_p, C.c_char_p, _P(QasrAlignment)]),
    "qasr_ctc_default_config": (C.c_int, [C.c_char_p, _P(QasrCtcConfig)]),
    "qasr_ctc_create": (C.c_int, [C.c_char_p, _P(QasrCtcConfig), _P(_E)]),
    "qasr_ctc_set_tensor": (C.c_int, [_E, C.c_char_p, C.c_void_p, C.c_int, _P(C.c_int64), C.c_int]),
    "qasr_ctc_finalize": (C.c_int, [_E]),
    "qasr_ctc_set_pieces": (C.c_int, [_E, _P(C.c_char_p), _I, C.c_size_t]),
    "qasr_ctc_is_loaded": (C.c_int, [_E]),
    "qasr_ctc_unload": (C.c_int, [_E]),
    "qasr_ctc_memory_footprint": (C.c_size_t, [_E]),
    "qasr_ctc_destroy": (None, [_E]),
    "qasr_ctc_last_error": (C.c_char_p, [_E]),
    "qasr_ctc_num_frames": (C.c_int, [C.c_size_t]),
    "qasr_ctc_transcribe_batch": (C.c_int, [_E, _P(_F), _P(C.c_size_t), C.c_size_t, C.c_int, _I, C.c_size_t, _I]),
    "qasr_ctc_transcribe": (C.c_int, [_E, _F, C.c_size_t, C.c_int, _P(C.c_char_p)]),
    "qasr_ctc_logits": (C.c_int, [_E, _F, C.c_size_t, _F]),
    "qasr_ctc_detokenize": (C.c_int, [_E, _I, C.c_int32, C.c_char_p, C.c_size_t]),
    "qasr_ctc_timings": (C.c_int, [_E, _F]),
    "qasr_ctc_greedy": (C.c_int, [_F, C.c_int32, C.c_int32, C.c_int32, _I]),
    "qasr_layer_normalize": (C.c_int, [_F, C.c_size_t, C.c_float, _F]),
    "qasr_dp_create": (C.c_int, [C.c_char_p, _P(QasrConfig), _I, C.c_int32, _P(_E)]),
    "qasr_dp_destroy": (None, [_E]),
    "qasr_dp_n_devices": (C.c_int, [_E]),
    "qasr_dp_engine": (_E, [_E, C.c_int32]),
    "qasr_dp_last_error": (C.c_char_p, [_E]),
    "qasr_dp_set_tensor": (C.c_int, [_E, C.c_char_p, C.c_void_p, C.c_int, _P(C.c_int64), C.c_int]),
    "qasr_dp_finalize": (C.c_int, [_E]),
    "qasr_dp_transcribe_batch": (C.c_int, [_E, _P(_F), _P(C.c_size_t), C.c_size_t, C.c_int, _P(QasrOptions), _I, _I]),
    "qasr_dp_timings": (C.c_int, [_E, _F, C.c_int32]),
    "qasr_dp_submit": (C.c_int, [_E, _P(_F), _P(C.c_size_t), C.c_size_t, C.c_int, _P(QasrOptions), _P(C.c_int64)]),
    "qasr_dp_collect": (C.c_int, [_E, C.c_int64, _I, _I]),
    "qasr_nemo_mel_create": (C.c_int, [C.c_int, C.c_int, C.c_size_t, C.c_float, _P(_E)]),
    "qasr_nemo_mel_destroy": (None, [_E]),
    "qasr_nemo_mel_last_error": (C.c_char_p, [_E]),
    "qasr_nemo_mel_num_frames": (C.c_int, [C.c_size_t]),
    "qasr_nemo_mel_length": (C.c_int, [C.c_size_t]),
    "qasr_nemo_mel_extract": (C.c_int, [_E, C.c_int, _P(_F), _P(C.c_size_t), C.c_size_t, _I, _F, C.c_size_t, _I, C.c_int]),
    "qasr_nemo_mel_reset_stats": (C.c_int, [_E, C.c_int]),
    "qasr_nemo_mel_timing": (C.c_int, [_E, _F, _P(C.c_int)]),
    "qasr_vad_default_config": (C.c_int, [_P(QasrVadConfig)]),
    "qasr_vad_create": (C.c_int, [C.c_int, C.c_char_p, C.c_int, _E, _P(_E)]),
    "qasr_vad_destroy": (None, [_E]),
    "qasr_vad_last_error": (C.c_char_p, [_E]),
    "qasr_vad_reset": (C.c_int, [_E, C.c_int]),
    "qasr_vad_process": (C.c_int, [_E, _F, _I, C.c_size_t, _F]),
    "qasr_vad_probs": (C.c_int, [_E, _P(_F), _P(C.c_size_t), C.c_size_t, _I, _F, C.c_size_t, _I]),
    "qasr_vad_binarize": (C.c_int, [_F, C.c_size_t, _P(QasrVadConfig), _F, C.c_size_t]),
    "qasr_vad_detect_speech": (C.c_int, [_E, _F, C.c_size_t, C.c_int, _P(QasrVadConfig), _F, C.c_size_t]),
    "qasr_vad_vtable": (C.c_int, [_E, C.c_int, _P(ScVadVtable)]),
    "qasr_vad_timing": (C.c_int, [_E, _F, _P(C.c_int)]),
    "qasr_vad_state": (C.c_int, [_E, C.c_int, _F, _F, _F]),
    "qasr_spk_create": (C.c_int, [C.c_int, C.c_char_p, C.c_size_t, _E, _P(_E)]),
    "qasr_spk_destroy": (None, [_E]),
    "qasr_spk_last_error": (C.c_char_p, [_E]),
    "qasr_spk_is_loaded": (C.c_int, [_E]),
    "qasr_spk_unload": (C.c_int, [_E]),
    "qasr_spk_memory_footprint": (C.c_size_t, [_E]),
    "qasr_spk_embedding_dim": (C.c_int, []),
    "qasr_spk_input_sample_rate": (C.c_int, []),
    "qasr_spk_embed": (C.c_int, [_E, _F, C.c_size_t, C.c_int, _F]),
    "qasr_spk_embed_batch": (C.c_int, [_E, _P(_F), _P(C.c_size_t), C.c_size_t, _F]),
    "qasr_spk_fbank": (C.c_int, [_E, _P(_F), _P(C.c_size_t), C.c_size_t, _F, C.c_size_t, _I]),
    "qasr_spk_num_frames": (C.c_int, [C.c_size_t]),
    "qasr_spk_cosine_similarity": (C.c_float, [_F, _F, C.c_size_t]),
    "qasr_spk_timing": (C.c_int, [_E, _F]),
    "qasr_seg_vad_default_config": (C.c_int, [_P(QasrSegVadConfig)]),
    "qasr_seg_create": (C.c_int, [C.c_int, C.c_char_p, C.c_int, _E, _P(_E)]),
    "qasr_seg_destroy": (None, [_E]),
    "qasr_seg_last_error": (C.c_char_p, [_E]),
    "qasr_seg_is_loaded": (C.c_int, [_E]),
    "qasr_seg_unload": (C.c_int, [_E]),
    "qasr_seg_memory_footprint": (C.c_size_t, [_E]),
    "qasr_seg_num_frames": (C.c_int, [C.c_size_t]),
    "qasr_seg_timing": (C.c_int, [_E, _F]),
    "qasr_seg_forward": (C.c_int, [_E, _F, C.c_size_t, C.c_size_t, _F, _F, _F]),
    "qasr_seg_window_positions": (C.c_int, [C.c_size_t, C.c_size_t, C.c_size_t, _P(C.c_int64), _P(C.c_int64), C.c_size_t]),
    "qasr_seg_windows": (C.c_int, [_E, _F, C.c_size_t, C.c_size_t, C.c_size_t, _F, _F, _F, _P(C.c_int64), _P(C.c_int64), C.c_size_t]),
    "qasr_seg_aggregate_frames": (C.c_int, [_F, C.c_size_t, C.c_size_t, _P(C.c_int64), C.c_size_t, C.c_int, C.c_float, _F, C.c_size_t]),
    "qasr_seg_binarize": (C.c_int, [_F, C.c_size_t, C.c_float, _P(QasrVadConfig), C.c_int, _F, C.c_size_t]),
    "qasr_seg_detect_speech": (C.c_int, [_E, _F, C.c_size_t, C.c_int, _P(QasrSegVadConfig), _F, C.c_size_t]),
    "qasr_diar_default_config": (C.c_int, [_P(QasrDiarConfig)]),
    "qasr_diar_cosine_distance": (C.c_float, [_F, _F, C.c_size_t]),
    "qasr_diar_cluster": (C.c_int, [_F, _I, C.c_size_t, C.c_size_t, C.c_float, _I, _F]),
    "qasr_diar_merge_segments": (C.c_int, [_P(QasrDiarSegment), C.c_size_t, C.c_float, _P(QasrDiarSegment)]),
    "qasr_diar_compact_speaker_ids": (C.c_int, [_P(QasrDiarSegment), C.c_size_t]),
    "qasr_diarize": (C.c_int, [_E, _E, _E, _F, C.c_size_t, C.c_int, _P(QasrDiarConfig), _P(_E)]),
    "qasr_diar_result_segments": (_P(QasrDiarSegment), [_E, _P(C.c_size_t)]),
    "qasr_diar_result_num_speakers": (C.c_int, [_E]),
    "qasr_diar_result_embeddings": (_F, [_E]),
    "qasr_diar_result_free": (None, [_E]),
    "qasr_diar_extract_speaker": (C.c_int, [_E, _F, _F, C.c_size_t]),
    "qasr_sep_default_config": (C.c_int, [_P(QasrSepConfig)]),
    "qasr_sep_create": (C.c_int, [C.c_int, C.c_char_p, C.c_size_t, _E, _P(_E)]),
    "qasr_sep_destroy": (None, [_E]),
    "qasr_sep_last_error": (C.c_char_p, [_E]),
    "qasr_sep_is_loaded": (C.c_int, [_E]),
    "qasr_sep_unload": (C.c_int, [_E]),
    "qasr_sep_memory_footprint": (C.c_size_t, [_E]),
    "qasr_sep_hidden_size": (C.c_int, [_E]),
    "qasr_sep_sample_rate": (C.c_int, []),
    "qasr_sep_num_frames": (C.c_int64, [C.c_size_t]),
    "qasr_sep_timing": (C.c_int, [_E, _F]),
    "qasr_sep_set_recurrence_form": (C.c_int, [_E, C.c_int]),
    "qasr_sep_separate_batch": (C.c_int, [_E, _P(_F), _P(_F), _P(C.c_size_t), C.c_size_t, C.c_int, C.c_uint, _P(QasrSepConfig), _P(_F)]),
    "qasr_sep_separate": (C.c_int, [_E, _F, _F, C.c_size_t, C.c_int, C.c_uint, _P(QasrSepConfig), _F]),
    "qasr_sep_stft": (C.c_int, [_E, _F, _F, C.c_size_t, _F, _F, _F]),
    "qasr_sep_masks": (C.c_int, [_E, _F, _P(C.c_size_t), C.c_size_t, _F]),
    "qasr_sep_wiener": (C.c_int, [_E, _F, C.c_int, _F, _F, C.c_size_t, _P(QasrSepConfig), _F, _F]),
    "qasr_sep_istft": (C.c_int, [_E, _F, _F, C.c_int, C.c_size_t, C.c_size_t, _F]),
    "qasr_codec_create": (C.c_int, [C.c_int, C.c_char_p, C.c_int, _E, _P(_E)]),
    "qasr_codec_destroy": (None, [_E]),
    "qasr_codec_last_error": (C.c_char_p, [_E]),
    "qasr_codec_is_loaded": (C.c_int, [_E]),
    "qasr_codec_unload": (C.c_int, [_E]),
    "qasr_codec_memory_footprint": (C.c_size_t, [_E]),
    "qasr_codec_sample_rate": (C.c_int, []),
    "qasr_codec_samples_per_frame": (C.c_int, []),
    "qasr_codec_num_quantizers": (C.c_int, [_E]),
    "qasr_codec_hidden_size": (C.c_int, [_E]),
    "qasr_codec_latent_dim": (C.c_int, [_E]),
    "qasr_codec_forward": (C.c_int, [_E, _I, C.c_size_t, C.c_size_t, C.c_int, _F]),
    "qasr_codec_forward_tail": (C.c_int, [_E, _I, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, _F]),
    "qasr_codec_tail_leads": (C.c_int, [_I, _I]),
    "qasr_codec_window_positions": (C.c_int64, [C.c_size_t, _I, _I, _I, C.c_size_t]),
    "qasr_codec_decode": (C.c_int, [_E, _I, C.c_size_t, _F]),
    "qasr_codec_decode_batch": (C.c_int, [_E, _P(_I), _P(C.c_size_t), C.c_size_t, _P(_F)]),
    "qasr_codec_quantizer_decode": (C.c_int, [_E, _I, C.c_size_t, C.c_size_t, _F]),
    "qasr_codec_pre_transformer": (C.c_int, [_E, _F, C.c_size_t, C.c_size_t, _F]),
    "qasr_codec_timing": (C.c_int, [_E, _F]),
    "qasr_codec_enc_create": (C.c_int, [C.c_int, C.c_char_p, C.c_size_t, _E, _P(_E)]),
    "qasr_codec_enc_destroy": (None, [_E]),
    "qasr_codec_enc_last_error": (C.c_char_p, [_E]),
    "qasr_codec_enc_is_loaded": (C.c_int, [_E]),
    "qasr_codec_enc_unload": (C.c_int, [_E]),
    "qasr_codec_enc_memory_footprint": (C.c_size_t, [_E]),
    "qasr_codec_enc_num_quantizers": (C.c_int, [_E]),
    "qasr_codec_enc_hidden_size": (C.c_int, [_E]),
    "qasr_codec_enc_latent_dim": (C.c_int, [_E]),
    "qasr_codec_enc_num_frames": (C.c_size_t, [C.c_size_t]),
    "qasr_codec_enc_encode": (C.c_int, [_E, _F, C.c_size_t, _I]),
    "qasr_codec_enc_encode_batch": (C.c_int, [_E, _P(_F), _P(C.c_size_t), C.c_size_t, _P(_I)]),
    "qasr_codec_enc_conv": (C.c_int, [_E, _F, C.c_size_t, _F]),
    "qasr_codec_enc_conv_batch": (C.c_int, [_E, _P(_F), _P(C.c_size_t), C.c_size_t, _P(_F)]),
    "qasr_codec_enc_latent": (C.c_int, [_E, _F, C.c_size_t, _F]),
    "qasr_codec_enc_latent_batch": (C.c_int, [_E, _P(_F), _P(C.c_size_t), C.c_size_t, _P(_F)]),
    "qasr_codec_enc_quantize": (C.c_int, [_E, _F, C.c_size_t, _I]),
    "qasr_codec_enc_timing": (C.c_int, [_E, _F]),
    "qasr_xvec_create": (C.c_int, [C.c_int, C.c_char_p, C.c_size_t, _E, _P(_E)]),
    "qasr_xvec_destroy": (None, [_E]),
    "qasr_xvec_last_error": (C.c_char_p, [_E]),
    "qasr_xvec_is_loaded": (C.c_int, [_E]),
    "qasr_xvec_unload": (C.c_int, [_E]),
    "qasr_xvec_memory_footprint": (C.c_size_t, [_E]),
    "qasr_xvec_embedding_dim": (C.c_int, [_E]),
    "qasr_xvec_input_sample_rate": (C.c_int, []),
    "qasr_xvec_num_frames": (C.c_size_t, [C.c_size_t]),
    "qasr_xvec_embed": (C.c_int, [_E, _F, C.c_size_t, C.c_int, _F]),
    "qasr_xvec_embed_batch": (C.c_int, [_E, _P(_F), _P(C.c_size_t), C.c_size_t, _F]),
    "qasr_xvec_mel": (C.c_int, [_E, _P(_F), _P(C.c_size_t), C.c_size_t, _P(_F)]),
    "qasr_xvec_embed_mel": (C.c_int, [_E, _F, C.c_size_t, _F]),
    "qasr_xvec_timing": (C.c_int, [_E, _F]),
    "qasr_hift_create": (C.c_int, [C.c_int, C.c_char_p, C.c_size_t, _E, _P(_E)]),
    "qasr_hift_destroy": (None, [_E]),
    "qasr_hift_last_error": (C.c_char_p, [_E]),
    "qasr_hift_is_loaded": (C.c_int, [_E]),
    "qasr_hift_unload": (C.c_int, [_E]),
    "qasr_hift_memory_footprint": (C.c_size_t, [_E]),
    "qasr_hift_sample_rate": (C.c_int, []),
    "qasr_hift_num_samples": (C.c_size_t, [C.c_size_t]),
    "qasr_hift_noise": (C.c_int, [C.c_uint64, _P(C.c_uint64), C.c_size_t, _F, _F]),
    "qasr_hift_f0": (C.c_int, [_E, _F, C.c_size_t, _F]),
    "qasr_hift_source": (C.c_int, [_E, _F, C.c_size_t, C.c_uint64, _F]),
    "qasr_hift_decode_source": (C.c_int, [_E, _F, C.c_size_t, _F, _F]),
    "qasr_hift_decode": (C.c_int, [_E, _F, C.c_size_t, C.c_uint64, _F]),
    "qasr_hift_decode_batch": (C.c_int, [_E, _P(_F), _P(C.c_size_t), _P(C.c_uint64), C.c_size_t, _P(_F)]),
    "qasr_hift_timing": (C.c_int, [_E, _F]),
    "qasr_avae_create": (C.c_int, [C.c_int, C.c_char_p, C.c_size_t, _E, _P(_E)]),
    "qasr_avae_destroy": (None, [_E]),
    "qasr_avae_last_error": (C.c_char_p, [_E]),
    "qasr_avae_is_loaded": (C.c_int, [_E]),
    "qasr_avae_unload": (C.c_int, [_E]),
    "qasr_avae_memory_footprint": (C.c_size_t, [_E]),
    "qasr_avae_latent_dim": (C.c_int, [_E]),
    "qasr_avae_in_sample_rate": (C.c_int, [_E]),
    "qasr_avae_out_sample_rate": (C.c_int, [_E]),
    "qasr_avae_hop": (C.c_int, [_E]),
    "qasr_avae_samples_per_frame": (C.c_int, [_E]),
    "qasr_avae_num_frames": (C.c_size_t, [_E, C.c_size_t]),
    "qasr_avae_num_blocks": (C.c_int, [_E, C.c_int]),
    "qasr_avae_stage_shape": (C.c_int, [_E, C.c_int, C.c_int, _I, _I]),
    "qasr_avae_encode": (C.c_int, [_E, _F, C.c_size_t, _F]),
    "qasr_avae_decode": (C.c_int, [_E, _F, C.c_size_t, C.c_int, _F]),
    "qasr_avae_encode_batch": (C.c_int, [_E, _P(_F), _P(C.c_size_t), C.c_size_t, _P(_F)]),
    "qasr_avae_decode_batch": (C.c_int, [_E, _P(_F), _P(C.c_size_t), C.c_size_t, C.c_int, _P(_F)]),
    "qasr_avae_enc_stage": (C.c_int, [_E, _F, C.c_size_t, C.c_int, _F]),
    "qasr_avae_dec_stage": (C.c_int, [_E, _F, C.c_size_t, C.c_int, C.c_int, _F]),
    "qasr_avae_dec_output": (C.c_int, [_E, _F, C.c_size_t, _F]),
    "qasr_avae_timing": (C.c_int, [_E, _F]),
    "qasr_tts_default_config": (C.c_int, [C.c_char_p, C.c_int, _P(QasrTtsConfig)]),
    "qasr_tts_default_sampling": (None, [C.c_int, _P(QasrTtsSampling)]),
    "qasr_tts_poll_interval": (C.c_int, []),
    "qasr_tts_create": (C.c_int, [C.c_char_p, _P(QasrTtsConfig), _P(_E)]),
    "qasr_tts_free": (None, [_E]),
    "qasr_tts_last_error": (C.c_char_p, [_E]),
    "qasr_tts_memory_footprint": (C.c_size_t, [_E]),
    "qasr_tts_device_bytes": (C.c_size_t, [_E]),
    "qasr_tts_generate": (C.c_int, [_E, _P(QasrTtsRequest), _P(QasrTtsSampling), C.c_uint64, _I, _I]),
    "qasr_tts_forced": (C.c_int, [_E, _P(QasrTtsRequest), _I, C.c_size_t, _F, _F, _F]),
    "qasr_tts_sample_host": (C.c_int, [_P(QasrTtsConfig), _F, C.c_int32, C.c_int, _P(QasrTtsSampling), _I, C.c_int32, C.c_uint64,
                                       C.c_int64, C.c_int32, C.c_int32]),
    "qasr_tts_synthesize": (C.c_int, [_E, _E, _P(QasrTtsRequest), _P(QasrTtsSampling), C.c_uint64, _P(_F), _P(C.c_size_t), _I, _I]),
    "qasr_tts_create_icl": (C.c_int, [C.c_char_p, _P(QasrTtsConfig), C.c_int32, C.c_int32, _P(_E)]),
    "qasr_tts_icl_capacity": (C.c_int, [_E, _I, _I]),
    "qasr_tts_generate_icl": (C.c_int, [_E, _P(QasrTtsRequest), _P(QasrTtsIcl), _P(QasrTtsSampling), C.c_uint64, _I, _I]),
    "qasr_tts_forced_icl": (C.c_int, [_E, _P(QasrTtsRequest), _P(QasrTtsIcl), _I, C.c_size_t, _F, _F, _F]),
    "qasr_tts_synthesize_icl": (C.c_int, [_E, _E, _P(QasrTtsRequest), _P(QasrTtsIcl), _P(QasrTtsSampling), C.c_uint64, _P(_F),
                                          _P(C.c_size_t), _I, _I]),
    "qasr_tts_icl_prompt": (C.c_int, [_E, _P(QasrTtsRequest), _P(QasrTtsIcl), _F, _I]),
    "qasr_tts_clone": (C.c_int, [_E, _E, _E, _E, _P(QasrTtsRequest), _P(_I), _I, _P(_F), _P(C.c_size_t), _P(QasrTtsSampling), C.c_uint64,
                                 _P(_F), _P(C.c_size_t), _I, _I]),
    "qasr_tts_default_stream_config": (None, [C.c_int, _P(QasrTtsStreamConfig)]),
    "qasr_tts_pool_create": (C.c_int, [_E, _E, _P(QasrTtsSampling), C.c_uint64, _P(_E)]),
    "qasr_tts_pool_open": (C.c_int, [_E, _P(QasrTtsRequest), _P(QasrTtsStreamConfig), _I]),
    "qasr_tts_pool_step": (C.c_int, [_E, _P(QasrTtsChunk), C.c_size_t, _P(C.c_size_t)]),
    "qasr_tts_pool_timing": (C.c_int, [_E, _F]),
    "qasr_tts_pool_close": (C.c_int, [_E, C.c_int32]),
    "qasr_tts_pool_live": (C.c_int, [_E]),
    "qasr_tts_pool_destroy": (None, [_E]),
    "qasr_tts_pool_last_error": (C.c_char_p, [_E]),
    "qasr_tts_stream_chunks": (C.c_int64, [C.c_int32, C.c_int, _P(QasrTtsStreamConfig), _I, _I, _I, C.c_size_t]),
    "qasr_transducer_default_config": (C.c_int, [C.c_char_p, _P(QasrTransducerConfig)]),
    "qasr_tdt_greedy_decode": (C.c_int, [_P(QasrTransducerConfig), _P(QasrTransducerCallbacks), C.c_int32, _I, _F, C.c_int32, _F]),
    "qasr_rnnt_greedy_decode": (C.c_int, [_P(QasrTransducerConfig), _P(QasrTransducerCallbacks), C.c_int32, C.c_int32, _I, _F, C.c_int32, _I]),
    "qasr_log_softmax_at": (C.c_float, [_F, C.c_int32, C.c_int32]),
    "qasr_transducer_confidence": (C.c_float, [_F, C.c_int32]),
    "qasr_sp_vocab_create": (C.c_int, [_I, _P(C.c_char_p), C.c_size_t, C.c_int, _P(_E)]),
    "qasr_sp_vocab_load": (C.c_int, [C.c_char_p, C.c_int, _P(_E)]),
    "qasr_sp_vocab_destroy": (None, [_E]),
    "qasr_sp_vocab_count": (C.c_int, [_E]),
    "qasr_sp_vocab_decode": (C.c_int, [_E, _I, C.c_int32, C.c_char_p, C.c_size_t]),
    "qasr_sp_vocab_decode_words": (C.c_int, [_E, _I, C.c_int32, _F, C.c_int32, C.c_char_p, C.c_size_t, _F, C.c_int32]),
    "qasr_stream_chunker_create": (C.c_int, [C.c_int32, C.c_int32, _P(_E)]),
    "qasr_stream_chunker_destroy": (None, [_E]),
    "qasr_stream_chunker_push": (C.c_int, [_E, _F, C.c_size_t]),
    "qasr_stream_chunker_pop": (C.c_int, [_E, _F]),
    "qasr_stream_chunker_flush": (C.c_int, [_E, _F]),
    "qasr_stream_chunker_buffered": (C.c_size_t, [_E]),
    "qasr_flow_create": (C.c_int, [C.c_int, C.c_char_p, C.c_size_t, _E, _P(_E)]),
    "qasr_flow_destroy": (None, [_E]),
    "qasr_flow_last_error": (C.c_char_p, [_E]),
    "qasr_flow_is_loaded": (C.c_int, [_E]),
    "qasr_flow_unload": (C.c_int, [_E]),
    "qasr_flow_memory_footprint": (C.c_size_t, [_E]),
    "qasr_flow_depth": (C.c_int, [_E]),
    "qasr_flow_mel_frames": (C.c_size_t, [C.c_size_t]),
    "qasr_flow_schedule": (C.c_int, [C.c_int, _F]),
    "qasr_flow_check_clip": (C.c_int, [_I, C.c_size_t, _I, C.c_size_t, C.c_size_t, C.c_int, C.c_size_t]),
    "qasr_flow_mu": (C.c_int, [_E, _I, C.c_size_t, _F]),
    "qasr_flow_spks": (C.c_int, [_E, _F, _F]),
    "qasr_flow_velocity": (C.c_int, [_E, _F, _F, _F, _F, C.c_size_t, C.c_float, _F]),
    "qasr_flow_solve": (C.c_int, [_E, _F, _F, _F, C.c_size_t, _F, C.c_int, _F, _F]),
    "qasr_flow_generate": (C.c_int, [_E, _I, C.c_size_t, _I, C.c_size_t, _F, C.c_size_t, _F, C.c_int, C.c_float, C.c_uint64, _F, _F]),
    "qasr_flow_generate_batch": (C.c_int, [_E, _P(_I), _P(C.c_size_t), _P(_I), _P(C.c_size_t), _P(_F), _P(C.c_size_t), _P(_F), C.c_int, C.c_float,
                                           _P(C.c_uint64), C.c_size_t, _P(_F), _P(_F)]),
    "qasr_flow_timing": (C.c_int, [_E, _F]),
    "qasr_cvlm_default_config": (C.c_int, [C.c_int, _P(QasrCvlmConfig)]),
    "qasr_cvlm_default_sampling": (None, [_P(QasrCvlmSampling)]),
    "qasr_cvlm_create": (C.c_int, [C.c_char_p, _P(QasrCvlmConfig), _P(_E)]),
    "qasr_cvlm_check": (C.c_int, [C.c_char_p, _P(QasrCvlmConfig)]),
    "qasr_cvlm_free": (None, [_E]),
    "qasr_cvlm_last_error": (C.c_char_p, [_E]),
    "qasr_cvlm_memory_footprint": (C.c_size_t, [_E]),
    "qasr_cvlm_device_bytes": (C.c_size_t, [_E]),
    "qasr_cvlm_poll_interval": (C.c_int, []),
    "qasr_cvlm_context": (C.c_int, [_P(QasrCvlmConfig)]),
    "qasr_cvlm_plan_prefix": (C.c_int, [_P(QasrCvlmConfig), _I, C.c_int32, _I, C.c_int32, _I]),
    "qasr_cvlm_generate": (C.c_int, [_E, _P(QasrCvlmRequest), _P(QasrCvlmSampling), C.c_uint64, _I, _I]),
    "qasr_cvlm_forced": (C.c_int, [_E, _P(QasrCvlmRequest), _I, C.c_size_t, _F, _F]),
    "qasr_cvlm_sample": (C.c_int, [_E, _F, _P(_I), _I, _I, _I, C.c_size_t, _P(QasrCvlmSampling), C.c_uint64, _P(C.c_int64), _I]),
    "qasr_cvlm_sample_host": (C.c_int, [_P(QasrCvlmConfig), _F, _I, C.c_int32, C.c_int32, C.c_int, _P(QasrCvlmSampling), C.c_uint64,
                                        C.c_int64]),
    "qasr_cvlm_linear_probe": (C.c_int, [_E, C.c_int32, C.c_int32, _F, _F, C.c_size_t, _F]),
    "qasr_cvlm_synthesize": (C.c_int, [_E, _E, _E, _P(QasrCvlmRequest), _P(QasrCvlmSampling), C.c_uint64, _P(_F), _P(_F), _P(C.c_size_t),
                                       _P(_F), _P(C.c_size_t), _I, _I]),
    "qasr_s3tok_create": (C.c_int, [C.c_int, C.c_char_p, C.c_size_t, _E, _P(_E)]),
    "qasr_s3tok_destroy": (None, [_E]),
    "qasr_s3tok_last_error": (C.c_char_p, [_E]),
    "qasr_s3tok_is_loaded": (C.c_int, [_E]),
    "qasr_s3tok_unload": (C.c_int, [_E]),
    "qasr_s3tok_memory_footprint": (C.c_size_t, [_E]),
    "qasr_s3tok_depth": (C.c_int, [_E]),
    "qasr_s3tok_max_tokens": (C.c_size_t, [_E]),
    "qasr_s3tok_whisper_frames": (C.c_size_t, [C.c_size_t]),
    "qasr_s3tok_tokens": (C.c_size_t, [C.c_size_t]),
    "qasr_s3tok_flow_frames": (C.c_size_t, [C.c_size_t]),
    "qasr_s3tok_resampled_length": (C.c_size_t, [C.c_size_t, C.c_int, C.c_int]),
    "qasr_s3tok_profile_cut": (C.c_size_t, [C.c_size_t, C.c_size_t]),
    "qasr_s3tok_resample": (C.c_int, [_F, C.c_size_t, C.c_int, C.c_int, _F]),
    "qasr_s3tok_fsq_host": (C.c_int, [_F, C.c_size_t, _I]),
    "qasr_s3tok_whisper_mel": (C.c_int, [_E, _F, C.c_size_t, _F]),
    "qasr_s3tok_flow_mel": (C.c_int, [_E, _F, C.c_size_t, _F]),
    "qasr_s3tok_hidden": (C.c_int, [_E, _F, C.c_size_t, _F]),
    "qasr_s3tok_project": (C.c_int, [_E, _F, C.c_size_t, _F]),
    "qasr_s3tok_encode": (C.c_int, [_E, _F, C.c_size_t, _I]),
    "qasr_s3tok_encode_batch": (C.c_int, [_E, _P(_F), _P(C.c_size_t), C.c_size_t, _P(_I)]),
    "qasr_s3tok_profile": (C.c_int, [_E, _F, C.c_size_t, C.c_int, _I, _P(C.c_size_t), _F, _P(C.c_size_t), _P(C.c_size_t), _P(C.c_size_t)]),
    "qasr_s3tok_profile_batch": (C.c_int, [_E, _P(_F), _P(C.c_size_t), _P(C.c_int), C.c_size_t, _P(_I), _P(C.c_size_t), _P(_F), _P(C.c_size_t),
                                           _P(C.c_size_t), _P(C.c_size_t)]),
    "qasr_s3tok_timing": (C.c_int, [_E, _F]),
    "qasr_vloc_check": (C.c_int, [C.c_char_p, _P(QasrVlocGeometry)]),
    "qasr_vloc_create": (C.c_int, [C.c_int, C.c_char_p, C.c_size_t, _E, _P(_E)]),
    "qasr_vloc_destroy": (None, [_E]),
    "qasr_vloc_last_error": (C.c_char_p, [_E]),
    "qasr_vloc_is_loaded": (C.c_int, [_E]),
    "qasr_vloc_unload": (C.c_int, [_E]),
    "qasr_vloc_memory_footprint": (C.c_size_t, [_E]),
    "qasr_vloc_patch_size": (C.c_int, [_E]),
    "qasr_vloc_feat_dim": (C.c_int, [_E]),
    "qasr_vloc_lm_hidden": (C.c_int, [_E]),
    "qasr_vloc_mu_dim": (C.c_int, [_E]),
    "qasr_vloc_hidden": (C.c_int, [_E, C.c_int]),
    "qasr_vloc_depth": (C.c_int, [_E, C.c_int]),
    "qasr_vloc_max_seqs": (C.c_size_t, [_E]),
    "qasr_vloc_schedule": (C.c_int, [C.c_int, _F]),
    "qasr_vloc_zero_steps": (C.c_int, [C.c_int]),
    "qasr_vloc_rope_table": (C.c_int, [C.c_char_p, C.c_int, C.c_int, _F, _F]),
    "qasr_vloc_encode": (C.c_int, [_E, _F, C.c_size_t, _F, _F]),
    "qasr_vloc_mu": (C.c_int, [_E, _F, _F, C.c_size_t, _F]),
    "qasr_vloc_velocity": (C.c_int, [_E, _F, _F, _F, C.c_size_t, C.c_float, _F]),
    "qasr_vloc_solve": (C.c_int, [_E, _F, _F, _F, C.c_size_t, C.c_int, C.c_float, _F, _F]),
    "qasr_vloc_sample": (C.c_int, [_E, _F, _F, C.c_size_t, C.c_int, C.c_float, C.c_float, C.c_uint64, _P(C.c_uint64), _F, _F]),
    "qasr_vloc_stack": (C.c_int, [_E, C.c_int, _F, C.c_size_t, C.c_int, C.c_int, _F]),
    "qasr_vloc_timing": (C.c_int, [_E, _F]),
}

_lib = None


def load(strict=True):
    """dlopen libqasr.so; raises (never falls back) when the HIP extension is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"libqasr.so not built ({LIB_PATH}); run `python -c 'import __graft_entry__ as g; g.build()'`")
    lib = C.CDLL(LIB_PATH)
    missing = []
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            missing.append(name)
            continue
        fn.restype = res
        fn.argtypes = args
    if missing and strict:
        raise RuntimeError(f"libqasr.so lacks symbols declared in include/qasr.h: {missing}")
    _lib = lib
    return lib
