/* qasr.h -- C ABI of libqasr.so: MI355X-native (gfx950) Qwen3-ASR transcribe() hot path.
 *
 * Drop-in boundary for ivan-digital/qwen3-asr-swift.  Every entry point names the reference
 * interface it replaces (file:line under the reference tree).  Plain pointers and sizes only.
 *
 *   Qwen3ASRModel.fromPretrained(modelId:cacheDir:...)   Sources/Qwen3ASR/Qwen3ASR.swift:608-668
 *        -> qasr_default_config + qasr_create (+ qasr_set_tensor / qasr_finalize for in-memory weights)
 *   Qwen3ASRModel.transcribe(audio:sampleRate:language:maxTokens:context:)   Qwen3ASR.swift:131-164
 *   SpeechRecognitionModel.transcribe / inputSampleRate   Sources/AudioCommon/Protocols.swift:151-165,
 *                                                         Sources/Qwen3ASR/Qwen3ASR+Protocols.swift:5-11
 *        -> qasr_transcribe, qasr_input_sample_rate
 *   sc_stt_vtable_t.transcribe callback                   Sources/SpeechCore/VoicePipeline.swift:374-410
 *        -> qasr_stt_vtable (same field order / ownership rules)
 *   ModelMemoryManageable isLoaded/unload/memoryFootprint Sources/Qwen3ASR/Qwen3ASR+Memory.swift:3-18
 *        -> qasr_is_loaded, qasr_unload, qasr_memory_footprint
 *   TranscribeBatchCommand (sequential loop in the reference; batched here)
 *                                                         Sources/AudioCLILib/TranscribeBatchCommand.swift:69-133
 *        -> qasr_batch_begin / qasr_batch_run / qasr_batch_tokens, qasr_transcribe_batch
 *   Parakeet-TDT / Nemotron / Parakeet-EOU (BASELINE configs[4]; networks are opaque CoreML there): MelPreprocessor.extract,
 *   StreamingMelPreprocessor.extract / extractRaw / extractStreaming, TDTGreedyDecoder.decode, RNNTGreedyDecoder.decode,
 *   ParakeetVocabulary / NemotronVocabulary, StreamingSession.pushAudio   (file:line at each declaration)
 *        -> qasr_nemo_mel_*, qasr_tdt_greedy_decode, qasr_rnnt_greedy_decode, qasr_sp_vocab_*, qasr_stream_chunker_*
 *   SileroVADModel (Sources/SpeechVAD/SileroVAD.swift, SileroModel.swift) and the speech-core VAD vtable (VoicePipeline.swift:470-492)
 *        -> qasr_vad_* (file:line at the declarations)
 *   WeSpeakerModel / SpeakerEmbeddingModel (Sources/SpeechVAD/WeSpeaker.swift, WeSpeakerModel.swift, MelFeatureExtractor.swift;
 *   Sources/AudioCommon/Protocols.swift:249-256)  -> qasr_spk_* (file:line at the declarations)
 *   Stage entry points (no reference counterpart; they expose R1-R8 of SURVEY.md section 8a so
 *   each kernel can be diffed against the oracle in isolation): qasr_mel, qasr_encode,
 *   qasr_prefill_logits, qasr_decode_forced.
 *
 * Threading: like the reference ("not thread-safe", Qwen3ASR.swift:67) one engine = one HIP
 * device + one stream, not re-entrant; use one engine per GPU.
 * Errors: integer status (0 = ok) + qasr_last_error(engine).  transcribe() in the reference never
 * throws (Qwen3ASR.swift:151-154); shims convert a non-zero status to "[qasr error: ...]".
 */
#ifndef QASR_H
#define QASR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QASR_OK 0
#define QASR_ERR_INVALID 1      /* bad argument / shape */
#define QASR_ERR_HIP 2          /* HIP runtime failure (message in qasr_last_error) */
#define QASR_ERR_NOT_LOADED 3   /* weights missing / engine unloaded */
#define QASR_ERR_IO 4           /* checkpoint directory / file problem */
#define QASR_ERR_CAPACITY 5     /* batch or clip exceeds the engine's configured capacity */
#define QASR_ERR_EMPTY_AUDIO 6  /* zero-length clip (the reference traps on it) */
#define QASR_ERR_UNSUPPORTED 7  /* input the reference handles with a closed-source dependency (see qasr_split_words) */

#define QASR_DTYPE_F32 0
#define QASR_DTYPE_BF16 1
#define QASR_DTYPE_F16 2
#define QASR_DTYPE_U32 3

typedef struct qasr_engine qasr_engine;

/* Compile-time presets of the reference (Sources/Qwen3ASR/AudioEncoder.swift:28-88,
 * Configuration.swift:47-108) plus engine capacity knobs. */
typedef struct qasr_config {
    /* audio encoder */
    int32_t enc_d_model, enc_heads, enc_ffn, enc_layers, n_mels, enc_out_dim, conv_channels;
    int32_t n_window, n_window_infer;
    float ln_eps;
    /* text decoder */
    int32_t vocab, hidden, dec_layers, heads, kv_heads, head_dim, inter;
    float rms_eps, rope_theta;
    int32_t group_size, bits;          /* MLX affine quantisation of the checkpoint (4 / 8); 16 = bf16 */
    /* special token ids (Qwen3ASR.swift:54-63,181-193) */
    int32_t tok_im_start, tok_im_end, tok_audio_start, tok_audio_end, tok_audio_pad, tok_asr_text;
    int32_t tok_newline, tok_system, tok_user, tok_assistant;
    /* front-end: 2.0 reproduces vDSP_fft_zrip's documented 2x scaling */
    float fft_scale;
    /* engine capacity */
    int32_t device;                    /* HIP device ordinal */
    int32_t max_batch;                 /* clips per batch */
    int32_t max_audio_seconds;         /* longest clip, seconds at 16 kHz (reference cap: 1200) */
    int32_t max_new_tokens;            /* decoder output cap (reference default 448) */
    int32_t max_prompt_extra;          /* room for context / language hint tokens (aligner: the slotted text) in the prompt */
    /* forced aligner head (Qwen3ForcedAligner, ForcedAligner.swift:63-83; Configuration.swift:132-133).
     * classify_num == 0: an ASR engine (tied LM head).  > 0: the checkpoint's `lm_head.{weight,bias}` is a
     * Linear(hidden, classify_num) over timestamp classes and only the qasr_align* entry points run. */
    int32_t classify_num;              /* 5000 for Qwen3-ForcedAligner-0.6B */
    int32_t tok_timestamp;             /* <|timestamp|> = 151705 (Qwen3ASR.swift:62) */
    float timestamp_segment_time;      /* seconds per class, 0.08 */
} qasr_config;

typedef struct qasr_options {
    int32_t max_tokens;                /* <= config.max_new_tokens; 0 -> 448 */
    int32_t ignore_eos;                /* 1: always emit max_tokens tokens (fixed-work benchmarking) */
    const int32_t* context_ids;        /* tokenised context (Qwen3ASR.swift:203-206) or NULL */
    int32_t n_context;
    const int32_t* language_ids;       /* tokenised "language XX" hint (:228-232) or NULL */
    int32_t n_language;
    /* Qwen3DecodingOptions (Qwen3ASR.swift:13-51).  All zero = greedy fast path (isGreedyFastPath, :300-304).
     * Any non-default value selects the reference's slow path (generateSlow): the f32 logits of every row are written each
     * step and pickNextToken (:449-520) runs on them -- on the device by default, on the host (qasr_pick_next_token) with the
     * tuning knob device_sampler = 0; same tokens at temperature 0, same uniform stream (seed) otherwise. */
    float repetition_penalty;          /* 0 or 1.0 = off; HF sign-aware penalty on already generated ids */
    int32_t no_repeat_ngram_size;      /* 0 = off */
    float temperature;                 /* 0 = argmax; > 0 = Gumbel-max sampling */
    uint64_t seed;                     /* sampler seed (the reference uses the system RNG) */
} qasr_options;

typedef struct qasr_result {
    const char* text;                  /* owned by the engine, valid until the next call on it */
    const int32_t* tokens;             /* generated ids incl. the EOS that stopped the loop */
    int32_t n_tokens;
} qasr_result;

/* speech-core STT vtable shapes, field order as built at VoicePipeline.swift:376-409 */
typedef struct sc_transcription_result_t {
    const char* text;
    const char* language;
    float confidence;
    float start_time;
    float end_time;
} sc_transcription_result_t;

typedef struct sc_stt_vtable_t {
    void* context;
    sc_transcription_result_t (*transcribe)(void* ctx, const float* audio, size_t length, int sample_rate);
    int32_t (*input_sample_rate)(void* ctx);
    void* begin_stream;
    void* push_chunk;
    void* flush_stream;
    void* end_stream;
    void* cancel_stream;
} sc_stt_vtable_t;

/* ---- lifecycle ---------------------------------------------------------------------------- */
/* preset: "0.6B" | "1.7B" | a model id such as "aufklarer/Qwen3-ASR-0.6B-MLX-4bit"
 * (size/bits detection of Qwen3ASR.swift:581-601) | "tiny" (test geometry). */
int qasr_default_config(const char* preset, qasr_config* out);
/* model_dir: directory with *.safetensors (+ vocab.json, tokenizer_config.json); NULL = create an
 * empty engine whose tensors arrive through qasr_set_tensor. */
int qasr_create(const char* model_dir, const qasr_config* cfg, qasr_engine** out);
int qasr_set_tensor(qasr_engine* e, const char* name, const void* host_data, int dtype,
                    const int64_t* shape, int ndim);
int qasr_finalize(qasr_engine* e);                      /* checks completeness, builds fused layouts */
int qasr_set_vocab(qasr_engine* e, const int32_t* ids, const char* const* tokens, size_t n);
int qasr_is_loaded(const qasr_engine* e);
int qasr_unload(qasr_engine* e);
/* Weight bytes resident in HBM: the uploaded tensors plus everything qasr_finalize derives from them (fused q|k|v / gate|up,
 * fragment-major decode-step images; for an MLX 4 / 8-bit checkpoint the packed decode images and ONE layer-sized bf16 scratch the
 * prompt pass dequantises into -- no bf16 expansion of the decoder stays resident).  KV caches / workspaces are not counted. */
size_t qasr_memory_footprint(const qasr_engine* e);
void qasr_destroy(qasr_engine* e);
const char* qasr_last_error(const qasr_engine* e);      /* e may be NULL: last create() failure */
int qasr_input_sample_rate(const qasr_engine* e);       /* 16000 */

/* ---- harness input ---------------------------------------------------------------------------- */
/* PCM16 WAV reader (AudioFileLoader.loadWAV, Sources/AudioCommon/AudioFileLoader.swift:70-157, with the bounds
 * checks pinned by Tests/Qwen3ASRTests/SecurityHardeningTests.swift:83-196): first channel, int16 / 32768.
 * *samples is malloc'ed, release with qasr_free.  Pure CPU; malformed files return QASR_ERR_IO. */
int qasr_load_wav(const char* path, float** samples, size_t* n_samples, int* sample_rate);
void qasr_free(void* p);

/* ---- transcribe --------------------------------------------------------------------------- */
int qasr_transcribe(qasr_engine* e, const float* pcm, size_t n, int sample_rate,
                    const qasr_options* opt, qasr_result* out);
/* tokens: [B, max_new_tokens + 1] row-major, row b = lens[b] ids then padding (-1). */
int qasr_transcribe_batch(qasr_engine* e, const float* const* pcm, const size_t* n, size_t B,
                          int sample_rate, const qasr_options* opt, int32_t* tokens, int32_t* lens);
/* detokenise + "<asr_text>" post-strip (Tokenizer.swift:111-142, Qwen3ASR.swift:283-289);
 * returns bytes written (excluding NUL) or -1. */
int qasr_detokenize(qasr_engine* e, const int32_t* tokens, int32_t n, char* buf, size_t cap);
int qasr_stt_vtable(qasr_engine* e, sc_stt_vtable_t* out);
/* BPE encode of a UTF-8 string with the engine's vocab + merges (Qwen3Tokenizer.encode, Tokenizer.swift:195-289):
 * the reference encodes `context` and "language XX" with it (Qwen3ASR.swift:203-206,228-232).  Returns the
 * number of ids written or -1.  qasr_set_merges installs merges.txt content for engines built in memory. */
int qasr_encode_text(qasr_engine* e, const char* utf8, int32_t* ids, int32_t cap);
int qasr_set_merges(qasr_engine* e, const char* merges_txt);
/* pickNextToken (Qwen3ASR.swift:449-520) on a host logits vector; pure CPU function, no engine needed.
 * rng_state: in/out sampler state (only used when temperature > 0), may be NULL. */
int32_t qasr_pick_next_token(const float* logits, int32_t vocab, const int32_t* generated, int32_t n_generated,
                             float repetition_penalty, int32_t no_repeat_ngram_size, float temperature,
                             uint64_t* rng_state);

/* ---- split batch API: H2D / compute / D2H separately timed -------------------------------- */
int qasr_batch_begin(qasr_engine* e, const float* const* pcm, const size_t* n, size_t B,
                     const qasr_options* opt);          /* host -> HBM, builds the batch plan */
int qasr_batch_run(qasr_engine* e);                     /* mel + encoder + prefill + greedy decode, async */
/* Software pipeline over consecutive batches (a serving loop; no reference counterpart -- it loads and transcribes one file at a time):
 * qasr_batch_stage copies the NEXT batch's clips into a second pinned buffer and queues their host -> HBM copy on a copy stream behind
 * the current batch's log-mel (the only reader of the device PCM buffer), so that staging + PCIe run under the current batch's encoder /
 * prompt pass / decode.  Call it after qasr_batch_run of the current batch (QASR_ERR_INVALID before that); qasr_batch_begin_staged then
 * adopts the staged batch (planning only) once the current batch's tokens have been read.  Same results as qasr_batch_begin.  Once its
 * successor is staged a batch cannot be run again (qasr_batch_rewind + qasr_batch_run: QASR_ERR_INVALID): its samples have left the device. */
int qasr_batch_stage(qasr_engine* e, const float* const* pcm, const size_t* n, size_t B);
int qasr_batch_begin_staged(qasr_engine* e, const qasr_options* opt);
/* Re-arm the resident batch (PCM + plans stay in HBM, greedy state is reset on the device) so that
 * qasr_batch_run can be timed repeatedly without host->device traffic.  No reference counterpart. */
int qasr_batch_rewind(qasr_engine* e);
int qasr_batch_sync(qasr_engine* e);                    /* wait for the engine stream */
int qasr_batch_tokens(qasr_engine* e, int32_t* tokens, int32_t* lens);   /* HBM -> host */
/* per-stage device time of the last qasr_batch_run, milliseconds (HIP events on the engine stream):
 * [0] mel [1] encoder [2] prefill [3] decode [4] total; n_steps = decode steps executed. */
int qasr_batch_timings(qasr_engine* e, float ms[5], int32_t* n_steps);
/* Dominant-kernel probe used by bench.py's roofline object: average duration (ms) of kernel
 * `which` over the last run measured with HIP events on the engine stream, plus its launch count
 * and algorithmic bytes per launch.  which: 0 = decode-step weight-streaming GEMV group,
 * 1 = decode attention, 2 = LM head; 3 / 4 = prompt-pass QKV / gate-up GEMM, 5 = prompt attention of one layer (bytes_per_launch
 * then holds FLOPs; causal count for 5).  The probes time what the step launches: where the step runs the q|k|v projection and the attention
 * of a layer as ONE launch (qasr_decode_structure), 1 is that launch (K / V rows + the q|k|v weights) and 0 the three linears left. 
 * 6 / 7: diagnostic phase stamps of the persistent launches (stderr). */
int qasr_kernel_probe(qasr_engine* e, int which, int reps, float* avg_ms, double* bytes_per_launch);
/* How the decode step of the CURRENT batch is launched (csrc/decoder.hip run_decode_step): *fused_qa = 1 when a layer's q|k|v projection and
 * attention are one launch (csrc/dec_qa.hip), *chain = the `chain` knob where it applies, else 0; *launches_per_layer = dependent launches per
 * decoder layer (5 when neither applies).  No reference counterpart. */
int qasr_decode_structure(qasr_engine* e, int* fused_qa, int* chain, int* launches_per_layer);
/* Diagnostic: the MFMA GEMM the encoder / prompt pass / wav2vec2 path are built on, by itself.  out[M][N] (f32, host) =
 * A[M][K] . W[N][K]^T + bias[N] with bf16 operands (host arrays of bf16 bit patterns), f32 accumulation, f32 bias (may be
 * NULL).  form: 0 = 128x128 double-buffered, 1 = 128x128 single LDS buffer, 2 = 256x256 ping-pong (csrc/gemm_p8.h),
 * -1 = whatever the engine would pick for this shape.  K % 8 == 0 and N % 4 == 0 like every caller.  Needs no weights;
 * no reference counterpart (MLX supplies the matmul there) -- used by tests/test_gpu_gemm.py to compare the forms with
 * each other bit for bit and with a float64 product on ragged shapes.  *avg_ms (may be NULL): mean of `reps` launches. */
int qasr_gemm_probe(qasr_engine* e, const uint16_t* A, const uint16_t* W, const float* bias, int M, int N, int K, int form,
                    int reps, float* out, float* avg_ms);
/* Diagnostic: ONE operand gather + fused epilogue pair of that GEMM as the product launches it (same functor types, same launch entry),
 * on host data: upload, one launch, download.  Needs no weights; no reference counterpart.  tests/test_gpu_gemm_cases.py holds every pair
 * against a float64 restatement (tests/gemm_cases.py) and the gathers bit for bit against qasr_gemm_probe on the materialised operand.
 *   which                    operand A (bf16 bit patterns)         epilogue -> out                                     launch
 *   CONV                     NHWC image [n_img][H][W][C], 3x3 /    bf16 gelu(acc + bias_f32[n]), +0 where ow >=         gemm_nt
 *                            stride 2 / pad 1, K index (kh*3+kw)   aux_i[img] (the image's valid output width; the
 *                            *C+ci; wide = 1: the per-K-tile tap   engine's level 2 / 3 width field carries it)
 *                            decomposition (C >= 64)
 *   CONV_PLAIN               the same gathers                      f32 acc + bias_f32[n]                               gemm_nt
 *   ROWTABLE                 a_len elements, row m = A + aux_l[m]  f32 acc + bias_f32[n]                               gemm_nt
 *   GROUPCONV                frames [M][groups*cpg]; aux_i = per   f32 gelu(acc + bias_f32[col]) + aux_f[m][col],      gemm_nt_groups
 *                            frame (t, L) of its clip; kernel KP,  col = g * cpg + n
 *                            padding KP / 2, K index tap*cpg+ci;
 *                            W [groups][cpg][KP*cpg]
 *   GROUPCONV_PLAIN          the same gather                       f32 acc + bias_f32[col]                             gemm_nt_groups
 *   BIAS_BF16 / _GELU        dense [M][K]                          bf16 act(acc + bias_bf16[n]), bias may be NULL      gemm_nt
 *   BIASF_BF16 / _GELU       dense                                 bf16 act(acc + bias_f32[n])                         gemm_nt
 *   STORE_BF16               dense                                 bf16 acc                                            gemm_nt
 *   RESID_F32 / RESID_F32F   dense                                 f32 out += acc + bias (bf16 / f32)                  gemm_nt
 *   RESID_BF16               dense                                 bf16 out = bf16(out + bf16(acc))                    gemm_nt
 *   POS_F32                  dense                                 f32 acc + aux_f[aux_i[m]][n]  (aux_f: [n_t][ld])    gemm_nt
 *   SWIGLU                   dense; W rows in blocks of 16 gate +  bf16(bf16(silu(bf16 g)) * bf16 u), [M][N / 2]       gemm_nt_swiglu
 *                            16 up rows
 * out is [out_rows][ld] (f32 or bf16 by the table; ld = 0: tight, out_rows = 0: M); it is uploaded before the launch, so the residual
 * forms read it and rows >= M come back as they went in.  form as for qasr_gemm_probe; the grouped launch has the single-buffer form only
 * (-1 or 1).  Refused with QASR_ERR_INVALID before anything is launched: C % 8 != 0, wide with C < 64, N % 4 != 0, a SWIGLU N that is not
 * a multiple of 32, form 2 for the grouped launch, M / N / K that contradict the geometry, ld % 4 != 0 or smaller than the written width,
 * a row offset / frame record / position index that would read outside the given arrays. */
enum {
    QASR_GEMM_CASE_CONV = 0, QASR_GEMM_CASE_CONV_PLAIN = 1, QASR_GEMM_CASE_ROWTABLE = 2, QASR_GEMM_CASE_GROUPCONV = 3,
    QASR_GEMM_CASE_GROUPCONV_PLAIN = 4, QASR_GEMM_CASE_BIAS_BF16 = 5, QASR_GEMM_CASE_BIAS_BF16_GELU = 6, QASR_GEMM_CASE_BIASF_BF16 = 7,
    QASR_GEMM_CASE_BIASF_BF16_GELU = 8, QASR_GEMM_CASE_STORE_BF16 = 9, QASR_GEMM_CASE_RESID_F32 = 10, QASR_GEMM_CASE_RESID_F32F = 11,
    QASR_GEMM_CASE_RESID_BF16 = 12, QASR_GEMM_CASE_POS_F32 = 13, QASR_GEMM_CASE_SWIGLU = 14
};
typedef struct qasr_gemm_case {
    int32_t M, N, K;                  /* output rows, weight rows, reduction length (conv: n_img*OH*OW, any, 9*C; groupconv: frames, cpg, KP*cpg) */
    int32_t ld, out_rows;             /* out's row stride in elements and its row count; 0 = tight / M */
    int32_t n_img, H, W, C;           /* conv */
    int32_t wide, hw_major, level;    /* conv: AConv3x3s2W | pixel order m = (img*OH+oh)*OW+ow (1) or (img*OW+ow)*OH+oh (0) | 2 or 3 */
    int32_t a_len;                    /* rowtable: elements of A */
    int32_t KP, cpg, groups;          /* groupconv */
    int32_t n_t;                      /* pos: rows of aux_f */
} qasr_gemm_case;
int qasr_gemm_case_probe(qasr_engine* e, int which, int form, const qasr_gemm_case* g, const uint16_t* A, const uint16_t* W,
                         const void* bias, const int32_t* aux_i, const int64_t* aux_l, const float* aux_f, void* out);

/* Diagnostic: the text decoder's attention and the kernels that write its K / V cache, by themselves, on host data and a scratch cache of ONE
 * layer whose geometry is the struct's (free of the engine's preset; needs no weights).  Nothing is restated: the product's launch entries
 * run (csrc/dec_kernels.h), with rope tables from the product's table builder at rope_theta.  All tensors are bf16 bit patterns.
 *   QASR_ATTN_PROMPT  qkv [n_pos][(heads + 2 kv_heads) * hd] (q | k | v), clip c = packed rows [cu[c], cu[c + 1]) in slot slot_of_clip[c];
 *                     pos[p] / slot[p] = position and slot of packed row p.  qk_norm_rope_launch, then prefill_attention_launch.
 *                     route 1: qkv = x[n_pos][hidden] . W[(heads + 2 kv_heads) * hd][hidden]^T first (gemm_nt, EpiStoreBf16);
 *                     route 2: that product as the head-tile GEMM with EpiQkHeads, then qk_norm_rope_launch(v_only) (hd 128 and
 *                     (heads + kv_heads) % 8 == 0; only the v third of qkv is meaningful then).  qkv comes back in every route.
 *                     -> qr [n_pos][heads * hd], out [n_pos][heads * hd]
 *   QASR_ATTN_DECODE  qkv [n_pos][...], one new token per row; row b lives in slot b at position pos[b] (its context length); cu,
 *                     slot_of_clip, slot, qr unused (may be NULL).  refresh of the rope rows, then decode_attention_launch.
 *                     -> out [n_pos][heads * hd]
 * kcache [n_slots][kv_heads][max_ctx][hd] and vfrag (same size, fragment-major per (slot, kv head): csrc/dec_attention.hip vfrag_index) are
 * uploaded before and downloaded after the launches, vt [n_slots][kv_heads][hd][max_ctx] (the prompt pass's V^T scratch, PROMPT only) is
 * uploaded.  Knobs: qasr_set_tuning.  Refused with QASR_ERR_INVALID before anything is launched: hd other than 32 / 128, max_ctx % 32 != 0
 * (PROMPT: % 64), DECODE with heads != 2 * kv_heads or n_pos > n_slots or a pos outside [0, max_ctx - 1], PROMPT with a head count the
 * writers do not take, a cu that does not start at 0 / increase / end at n_pos, a clip longer than max_ctx, a slot outside n_slots or used
 * by two clips, pos / slot that contradict cu, route 2 where it does not apply.  tests/test_gpu_attn_cases.py. */
enum { QASR_ATTN_PROMPT = 0, QASR_ATTN_DECODE = 1 };
typedef struct qasr_attn_case {
    int32_t n_slots, heads, kv_heads, hd, max_ctx;
    int32_t n_pos, n_clips;           /* packed rows (DECODE: batch rows); PROMPT: clips */
    int32_t route, hidden;            /* PROMPT: 0 = qkv given | 1 | 2 (see above), width of x */
    float eps, rope_theta;
} qasr_attn_case;
int qasr_attn_case_probe(qasr_engine* e, int op, const qasr_attn_case* g, uint16_t* qkv, const uint16_t* x, const uint16_t* W,
                         const int32_t* cu, const int32_t* slot_of_clip, const int32_t* pos, const int32_t* slot, const uint16_t* qn_w,
                         const uint16_t* kn_w, uint16_t* kcache, uint16_t* vfrag, const uint16_t* vt, uint16_t* qr, uint16_t* out);

/* Diagnostic: the attention kernels of the speech-synthesis stacks, by themselves, on host data; needs no weights.  Nothing is restated: one
 * call of the product's launch entry, the one its owning class calls.  The RoPE tables are data: cos / sin f32 [n_table][...].
 *   QASR_SYN_CVLM  cvlm_rope_append_launch, then cvlm_attention_launch (csrc/llm_cosyvoice.h; head_dim 64).  qkv bf16 [rows][(heads + 2 kv_heads)
 *                  * 64]; row r sits at (slot[r], pos[r]); tables [n_table][32]; kcache / vcache bf16 [n_slots][kv_heads][max_ctx][64];
 *                  qr and out bf16 [out_rows][heads * 64].
 *   QASR_SYN_CP    tts_cp_attn_launch at position `pos` (csrc/tts_talker.h; head_dim 128).  qkv bf16 [rows][(heads + 2 kv_heads) * 128]; qn_w /
 *                  kn_w bf16 [128]; tables [n_table][64]; kcache / vcache bf16 [n_slots][kv_heads][16][128] (n_slots >= rows cache rows, max_ctx
 *                  = 16); out bf16 [out_rows][heads * 128].
 *   QASR_SYN_VL    vl_attention_launch (csrc/loc_voxcpm.h; head_dim 128, f32).  qkv f32 [rows][(heads + 2 kv_heads) * 128], rows = n_seq * S;
 *                  tables [n_table][128]; out f32 [out_rows][heads * 128].
 * kcache, vcache, qr and out are uploaded before the launch and downloaded after it, so an untouched byte comes back as it went in; out_rows >=
 * rows.  qkv_elems, cache_elems, out_elems and table_elems are the element counts of the caller's arrays.  Refused with QASR_ERR_INVALID before
 * anything is launched: an unknown op, a missing array, heads / kv_heads above 16 (CVLM) or not integral, pos outside 0 .. 15 (CP), S outside
 * 1 .. 32 or heads x 128 no multiple of 512 (VL), a slot or position outside the cache or the tables, two rows on one cache row, an element
 * count that contradicts the geometry.  tests/test_gpu_syn_attn_cases.py. */
enum { QASR_SYN_CVLM = 0, QASR_SYN_CP = 1, QASR_SYN_VL = 2 };
typedef struct qasr_syn_attn_case {
    int32_t heads, kv_heads;
    int32_t rows, out_rows;           /* rows the launch is told about (VL: n_seq * S); rows of qr / out */
    int32_t n_slots, max_ctx;         /* CVLM: the cache; CP: cache rows (>= rows) and 16 */
    int32_t pos;                      /* CP */
    int32_t S, n_seq;                 /* VL */
    int32_t n_table;                  /* positions of cos / sin */
    int64_t qkv_elems, cache_elems, out_elems, table_elems;
    float eps;                        /* CP */
} qasr_syn_attn_case;
int qasr_syn_attn_case_probe(qasr_engine* e, int op, const qasr_syn_attn_case* g, const void* qkv, const int32_t* slot, const int32_t* pos,
                             const uint16_t* qn_w, const uint16_t* kn_w, const float* cos, const float* sin, uint16_t* kcache, uint16_t* vcache,
                             uint16_t* qr, void* out);

/* Diagnostic: the f32 kernels the waveform codecs share or keep outside their GEMM, by themselves, on host data; needs no weights.  Nothing
 * is restated: one call of the launch entry the three codec classes call (csrc/codec_launch.h).  All arrays are f32 but loc_a / loc_b.
 * `A` holds a_rows rows, which is everything a locator may reach; `out` (and R) hold M + out_extra rows, of which the launch is told
 * about M; the caller fills what lies beyond with NaN patterns / a sentinel.  `out` is uploaded before the launch and downloaded after
 * it, so an untouched byte comes back as it went in.
 *   TILE     codec_tile_launch(rows, snake, epi).  A [a_rows][Cin]; Wt [K][N], K = taps * Cin; bias [bmod] under WINDOW / TAIL
 *            (bias[n % bmod]), [N] under CLIP / VAE_STRIDE, or null; sa / sb [Cin] under snake, [N] under E_RESMAP; ls [N] under E_LSRES,
 *            [2 N] or null under E_RESMAP; R and out [M + out_extra][ldc] (R: E_RES, E_LSRES; optional under E_RESMAP), or in_place = 1:
 *            R is out itself, as the product runs E_RES / E_LSRES.  E_SWIGLU writes N / 2 columns.  Locators (csrc/codec_shared.h):
 *              WINDOW      loc_a = fstart [ceil(M / rate)]: fstart[f] is f or fstart[f - 1]; input row = output row
 *              TAIL        WINDOW, and loc_b = kept [as fstart]: a frame row of its own window, one value per window; lead >= 0
 *              CLIP        loc_a = ostart, loc_b = istart [n_clips + 1]: ostart from 0 to M, strictly increasing; istart not decreasing;
 *                          output row t of a clip reads input row istart + t * stride.  Both null (taps 1): row m reads row m
 *              VAE_STRIDE  loc_a = fstart [ceil(M / rate)] as WINDOW; output row m reads input rows up to (m + 1) * stride - 1
 *   RMS      codec_rms_launch.  A = x [a_rows >= M][C], Wt = w [C], eps; out [M + out_extra][C].
 *   DWLN     codec_dwln_launch under WINDOW or CLIP (loc_b = loc_a, stride 1).  A = x [a_rows >= M][C], Wt = w [7][C], bias = b [C], sa / sb
 *            = the LayerNorm's weight / bias [C]; out [M + out_extra][C].
 *   GATHER   codec_gather_launch.  loc_a = codes [M][Q] (n_loc = M Q), Wt = codebook 0 [S0][C], then Q - 1 codebooks [S1][C]; out
 *            [M + out_extra][2 C].  A is not used.
 *   OUT      codec_out_launch, TAIL under rows_kind TAIL (loc_b = kept), else WINDOW.  A = x [a_rows >= M][C], sa / sb [C], Wt = w [7][C],
 *            bias = b [1], clip 0 / 1; out [M + out_extra].
 *   CENC_IN  cenc_in_launch.  A = pcm [a_rows >= M], loc_a = clip starts [n_clips + 1] from 0 to M, Wt = w [7][C], bias = b [C]; out
 *            [M + out_extra][C].
 *   VQ       cenc_vq_launch.  out = r [M + out_extra][2 C] (read and written), loc_b = codes [M + out_extra][Q] (written; uploaded first, so
 *            rows past M come back as they went in), Wt / bias / sa = cb0 [S0][C], its transpose [C][S0] and |c|^2 [S0]; sb / ls / R = cb1
 *            [Q - 1][S1][C], the transposes [Q - 1][C][S1] and |c|^2 [Q - 1][S1] (null for Q = 1).  A is not used.
 *   ATTN_DEC codec_attn_launch.  A = qkv [a_rows >= M][3 heads 64], loc_a = n_clips windows (frames, first row) back to back from row 0 to M
 *            (n_loc = 2 n_clips), Wt = rope [n_table][32] pairs (cos, sin); out [M + out_extra][heads 64].
 *   ATTN_ENC cenc_attn_launch.  As ATTN_DEC with loc_a = n_clips tiles (the clip's first row, its frames, the tile's first query, 0): one per
 *            32 queries of each clip, clips back to back (n_loc = 4 n_clips).
 *   VAE_DW   vae_dw_launch under WINDOW (loc_a = fstart), both snakes (snake = 1: sa / sb = a1, 1 / a1, ls / R = a2, 1 / a2, each [C]) or
 *            neither.  A = x [a_rows >= M][C], Wt = w [7][C], bias = b [C], dil; out [M + out_extra][C].
 *   VAE_UNIT vae_unit_launch under WINDOW (loc_a = fstart), RPT by the product's rule.  A = x [a_rows >= M][C]; Wt = the unit's parameters packed
 *            as w1 [7][C] | b1 | a1 | 1 / a1 | a2 | 1 / a2 [C each] | conv2's Wt [C][C] | b2 [C]; sa / sb = the reader's map a, 1 / a [C] (both
 *            null: none), ls = its affine [2 C] or null; out [M + out_extra][C].  bias and R are not used.
 * Refused with QASR_ERR_INVALID before anything is launched: an unknown op; a missing array; a (rows, snake, epi) outside
 * CODEC_TILE_COMBOS (csrc/codec_launch.h); another locator than WINDOW / CLIP for DWLN, than WINDOW / TAIL for OUT; M outside 1 .. 2^20,
 * a_rows or out_extra above 2^20, Cin, N, C outside 1 .. 65536 (RMS too: codec_rms_kernel holds no row in LDS; DWLN, GATHER, VQ: C above
 * 4096; VAE_UNIT: C above AV_FUSE_MAX = 128 or no multiple of 4, dil above 9, a map with one array, an affine without the map), taps outside 1 .. 64, dil, rate, stride
 * outside 1 .. 64, Q outside 1 .. 64, S0 / S1 outside 1 .. 65536; K != taps * Cin; an odd N under E_SWIGLU; ldc below the columns written;
 * bmod outside 1 .. N; n_loc that is not the count stated above; an fstart, kept, ostart, istart or clip start that is not monotone as
 * stated above or points outside; a code outside its codebook (GATHER); any output row whose `last` input row is not inside
 * 0 .. a_rows - 1 or whose `first` is negative; a_rows below M where input and output rows are the same; in_place without a residual
 * epilogue, or with R; a residual epilogue without either; hd other than 64, heads outside 1 .. 64, a window above CODEC_MAX_T frames or
 * the rope table, windows, clips or tiles that do not lie back to back from row 0 to M (attention); dil above 27 or another locator than
 * WINDOW (VAE_DW).  tests/test_gpu_codec_cases.py. */
enum { QASR_CODEC_TILE = 0, QASR_CODEC_RMS = 1, QASR_CODEC_DWLN = 2, QASR_CODEC_GATHER = 3, QASR_CODEC_OUT = 4, QASR_CODEC_CENC_IN = 5,
       QASR_CODEC_VQ = 6, QASR_CODEC_ATTN_DEC = 7, QASR_CODEC_ATTN_ENC = 8, QASR_CODEC_VAE_DW = 9,
       QASR_CODEC_VAE_UNIT = 10 };
enum { QASR_CODEC_ROWS_WINDOW = 0, QASR_CODEC_ROWS_TAIL = 1, QASR_CODEC_ROWS_CLIP = 2, QASR_CODEC_ROWS_VAE_STRIDE = 3 };
typedef struct qasr_codec_case {
    int32_t rows_kind, snake, epi;    /* TILE: QASR_CODEC_ROWS_*, 0 / 1, 0 .. 5 = E_LIN, E_GELU, E_RES, E_LSRES, E_SWIGLU, E_RESMAP */
    int32_t M, a_rows, out_extra;
    int32_t Cin, taps, dil, K, N, bmod, ldc;
    int32_t rate, stride, lead, n_clips, n_loc;
    int32_t in_place;
    int32_t C;                        /* RMS, DWLN, GATHER (D), OUT, CENC_IN */
    int32_t Q, S0, S1;                /* GATHER, VQ */
    int32_t clip;                     /* OUT */
    int32_t heads, hd, n_table;       /* ATTN_DEC, ATTN_ENC: hd must be 64; rope positions */
    float eps;                        /* RMS */
} qasr_codec_case;
int qasr_codec_case_probe(qasr_engine* e, int op, const qasr_codec_case* g, const float* A, const float* Wt, const float* bias, const float* sa,
                          const float* sb, const float* ls, const float* R, const int32_t* loc_a, int32_t* loc_b, float* out);

/* Diagnostic: the encoder-side kernels that are not the GEMM, one launch of the product's own entry (csrc/enc_kernels.h, csrc/ctc_kernels.h)
 * on host data; needs no weights.  Nothing is restated.  `in` and `out` hold in_extra / out_extra ROWS beyond what the launch is told about
 * (the caller fills them with NaN patterns / a sentinel); `out` is uploaded before the launch and downloaded after it, so an untouched byte
 * comes back as it went in.  pf = f32 parameters, pw = bf16 parameters, idx / off = the launch's int32 / int64 index arrays.
 *   MHA, WINDOW     in bf16 [rows + in_extra][3 * heads * hd] (q | k | v), idx = cu [n_clips + 1]; out bf16 [rows + out_extra][heads * hd].
 *                   mha_attention_launch(max_len) under the mha_form knob / window_attention_launch.
 *   LN_BF16, LN_GELU_BF16, LN_GELU_F32   in f32 [rows + in_extra][D], pf = gamma [D] | beta [D]; out bf16 / bf16 / f32 [rows + out_extra][D].
 *   CONV0           in = pcm f32 [n_in], off = pcm_off [n_clips], idx = frame_off [n_clips] | n_out [n_clips], pf = stats [2 n_clips] |
 *                   w [D][10] | bias [D] | ln_g [D] | ln_b [D], max_len = max_out; out bf16 [rows + out_extra][D] (D = channels).
 *   WAVE_STATS      in = pcm f32 [n_in], off = pcm_off [rows], idx = n_samples [rows]; out f32 [rows + out_extra][2].
 *   CONV1           in = mel f32 [n_in], idx = ChunkMeta records, 9 int32 per image (clip, t0, clen, w0, w1, w2, w3, tok_off, n_tok),
 *                   rows = images, pf = bias [D], pw = w bf16 [D][9]; out bf16 [rows + out_extra][H1][W1][D].
 *   ARGMAX          in f32 [(rows + in_extra) * ld], n = D; out int32 [rows + out_extra] ids, then ONE int32 error word.
 *   CAST            in f32 [rows + in_extra] ELEMENTS; out bf16 [rows + out_extra].
 *   CONV_ROWS       idx = in_off | out_off | n_out [n_clips each], rows = total_out, stride, D = C; out int64 [rows + out_extra].
 *   FRAME_INFO      idx = frame_off | n_frames [n_clips each], rows = total; out int32 [rows + out_extra][2].
 * Refused with QASR_ERR_INVALID before anything is launched: a cu that does not start at 0 / increase / end at rows, max_len below a clip,
 * head_dim other than 32 / 64, mha_form 1 / 2 at head_dim 32 (the launcher would run form 0 there: the probe runs only the form that was
 * asked for), a WINDOW clip above 128 rows, D % 4 != 0 or D > 2048 for the norms, more than 1024 CONV0 channels, CONV1 channels that are no
 * multiple of 8, a ChunkMeta that reads outside mel, a CAST count that is no multiple of 4, a pcm offset or frame range outside its array.
 * tests/test_gpu_enc_cases.py. */
enum { QASR_ENC_MHA = 0, QASR_ENC_WINDOW, QASR_ENC_LN_BF16, QASR_ENC_LN_GELU_BF16, QASR_ENC_LN_GELU_F32, QASR_ENC_CONV0, QASR_ENC_WAVE_STATS,
       QASR_ENC_CONV1, QASR_ENC_ARGMAX, QASR_ENC_CAST, QASR_ENC_CONV_ROWS, QASR_ENC_FRAME_INFO };
typedef struct qasr_enc_case {
    int32_t rows, n_clips;            /* rows the launch is told about; clips / windows */
    int32_t in_extra, out_extra;      /* rows allocated beyond `rows` in `in` / `out` */
    int32_t heads, hd, max_len;       /* attention; CONV0: max_out */
    int32_t D, ld;                    /* width | channels | argmax n; ARGMAX row pitch */
    int32_t n_in;                     /* elements of pcm / mel */
    int32_t n_mels, mel_stride, H1, W1;   /* CONV1 */
    int32_t stride;                   /* CONV_ROWS */
    float eps;
} qasr_enc_case;
int qasr_enc_case_probe(qasr_engine* e, int op, const qasr_enc_case* g, const void* in, const int32_t* idx, const int64_t* off,
                        const float* pf, const uint16_t* pw, void* out);

/* Diagnostic: the kernels that stream the weights of a decode step, by themselves, on host data; needs no weights.  Nothing is restated: the
 * probe uploads, repacks the weight with the product's packer (pack_mfma_a_launch / quant_pack_launch) unless `generic` is set, calls the
 * product's launch entry ONCE (csrc/dec_kernels.h, csrc/dec_quant.h, csrc/dec_gemv_wide.h) and downloads.
 *   GEMV           X bf16 [B + in_extra][K], W bf16 [N][K] row-major, norm_w bf16 [K] or NULL (the fused RMSNorm prologue).  The dispatch of a
 *                  float checkpoint's decode-step linear: decode_gemv_wide_launch at K = 6144 under the gemv_wide knob, else
 *                  decode_gemv_fused_launch.  epi BF16 / RESID: out bf16 [B + out_extra][N] (RESID reads it); SWIGLU: out [..][N / 2], weight
 *                  rows in blocks of 16 gate + 16 up; LOGITS: logits f32 [B + out_extra][N] and the argmax partials.
 *   GEMVQ          the same on an MLX affine-quantised matrix: W = uint32 [N][K * bits / 32], scales / biases [N][K / 64] bf16 (sb_f32 0) or
 *                  f32 (1).  decode_gemv_q_launch; epi BF16 / RESID / SWIGLU.
 *   LMHEAD         lm_head_launch: final RMSNorm (norm_w required) + tied head on W bf16 [N][K] -> logits f32 [B + out_extra][N], partials.
 *   LMHEADQ        lm_head_q_launch on a quantised table.
 *   RMSNORM_ROWS   rmsnorm_rows_launch: X [B + in_extra][K], norm_w -> out bf16 [B + out_extra][K].
 *   FINALIZE       greedy_finalize_launch on given partials part_val / part_idx [B][n_parts] (n_parts is an INPUT here) and a given state.  With
 *                  R = B + out_extra: state int32 = tokens [R][max_new + 1] | lens [R] | finished [R] | ctx_len [R] | n_active [1] | err [1] |
 *                  clear [clear_words + 33] (absent at clear_words 0: the word 32 behind the cleared ones is the step sequence word);
 *                  rope f32 = cos [n_rope][half] | sin [n_rope][half]; rope_rows f32 = cos_rows [R][half] | sin_rows [R][half]; the embedding
 *                  table W = bf16 [N][K] (bits 0) or a quantised triplet (N = vocab, K = hidden) -> out bf16 [R][K] = the next input rows.
 *                  state, rope_rows and out are uploaded before and downloaded after the launch: everything it may write comes back.
 *   EMBED          epi 0: embed_splice_launch / embed_splice_q_launch, state = ids [B] | audio_src [B], X = audio rows bf16 [n_audio][K];
 *                  epi 1: gather_rows_launch / gather_rows_q_launch, state = row ids [B]; epi 2: quant_dequant_rows_launch of rows
 *                  [r0, r0 + B).  W as for FINALIZE -> out bf16 [B + out_extra][K].
 * out, logits and the partials are uploaded before the launch and downloaded after it, so an untouched byte comes back as it went in.
 * part_val / part_idx hold part_cap elements each; the launch writes [B][n_parts] at their start.  On return g->n_parts = partials per row
 * (0 without an argmax) and g->route = 1 where a tuned instantiation ran, 0 for the generic kernel (-1: RMSNORM_ROWS, FINALIZE, EMBED).  Knobs: qasr_set_tuning.
 * Refused with QASR_ERR_INVALID before anything is launched: B outside 1 .. 64, N that is no multiple of the epilogue's row tile (16; SWIGLU
 * 32), K % 32 != 0 (bf16) or K % 64 != 0 (quantised; % 128 unless generic: the packer's block), K above 8192, a norm above K = 2048, bits
 * other than 4 / 8, an epilogue the launch does not have (GEMVQ LOGITS), an LM-head B above lm_head_rows, a persistent LM head with fewer
 * than 8 tiles per workgroup of its grid, part_cap below B * n_parts, a missing array, more than 2^28 weight elements; FINALIZE / EMBED: a
 * hidden size that is no multiple of 8 (quantised: 64), a row id, audio row or dequantised row range outside its table, lens outside
 * [0, max_new], a context length whose next position lies outside the rope table, half above 256, n_parts outside [1, 4096], part_cap
 * below B * n_parts, n_audio outside [0, 65536].  A partial
 * INDEX outside the vocabulary is not refused: the kernel clamps it and sets err.
 * tests/test_gpu_dec_cases.py. */
enum { QASR_DEC_GEMV = 0, QASR_DEC_GEMVQ = 1, QASR_DEC_LMHEAD = 2, QASR_DEC_LMHEADQ = 3, QASR_DEC_RMSNORM_ROWS = 4, QASR_DEC_FINALIZE = 5,
       QASR_DEC_EMBED = 6 };
enum { QASR_DEC_EPI_BF16 = 0, QASR_DEC_EPI_RESID = 1, QASR_DEC_EPI_SWIGLU = 2, QASR_DEC_EPI_LOGITS = 3 };
typedef struct qasr_dec_case {
    int32_t B, N, K;                  /* batch rows, weight rows, reduction length */
    int32_t epi;                      /* GEMV / GEMVQ: QASR_DEC_EPI_*; else 0 */
    int32_t generic;                  /* 1: no packed image is handed to the launch, so its generic kernel runs */
    int32_t bits, sb_f32;             /* quantised forms */
    int32_t in_extra, out_extra;      /* rows allocated beyond B in X / in out and logits */
    int32_t part_cap;                 /* elements of part_val and of part_idx */
    float eps;
    int32_t n_parts, route;           /* written by the probe (FINALIZE: n_parts is given) */
    int32_t max_new, max_tokens, eos, ignore_eos, advance_ctx, clear_words;   /* FINALIZE: GreedyState and the launch's flag */
    int32_t n_rope, half;             /* FINALIZE: rows and width of the rope tables */
    int32_t n_audio, r0;              /* EMBED: audio rows in X; first row of epi 2 */
} qasr_dec_case;
int qasr_dec_case_probe(qasr_engine* e, int op, qasr_dec_case* g, const uint16_t* X, const void* W, const void* scales, const void* biases,
                        const uint16_t* norm_w, uint16_t* out, float* logits, float* part_val, int32_t* part_idx, int32_t* state,
                        const float* rope, float* rope_rows);

/* ---- utterance-batch data parallelism inside one process ----------------------------------------------------------------------
 * Replaces the sequential file loop of `speech transcribe-batch` (Sources/AudioCLILib/TranscribeBatchCommand.swift:82-93) for a caller
 * that owns several GPUs: one engine (= one HIP device + one stream, weights replicated) and one host thread per listed device; clips
 * are independent (Qwen3ASR.swift:131-164), so device i takes the contiguous block [lo_i, hi_i) of the list (the first B % n devices one
 * clip more) and there is no data-path exchange.  The gather of the decoded token streams is each engine's device -> host copy of its
 * [rows, max_new_tokens + 1] int32 block straight into the caller's buffer.  (The one-process-per-GPU form of the same partition, with
 * the RCCL all_gather of that block over xGMI, is bench.py / qasr/dist.py.)  A device may be listed twice (two engines on one GPU). */
typedef struct qasr_dp qasr_dp;
/* cfg->device is ignored (devices[i] is used); model_dir as for qasr_create (NULL: fill with qasr_dp_set_tensor + qasr_dp_finalize). */
int qasr_dp_create(const char* model_dir, const qasr_config* cfg, const int32_t* devices, int32_t n_devices, qasr_dp** out);
void qasr_dp_destroy(qasr_dp* dp);
int qasr_dp_n_devices(const qasr_dp* dp);
qasr_engine* qasr_dp_engine(qasr_dp* dp, int32_t i);               /* borrowed: engine i (vocabulary, options, stage entry points) */
const char* qasr_dp_last_error(const qasr_dp* dp);                 /* dp may be NULL: last create() failure */
int qasr_dp_set_tensor(qasr_dp* dp, const char* name, const void* host_data, int dtype, const int64_t* shape, int ndim);   /* every engine */
int qasr_dp_finalize(qasr_dp* dp);
/* tokens [B, max_new_tokens + 1], lens [B] as for qasr_transcribe_batch; B may exceed n_devices x max_batch (blocks go through an
 * engine in slices of its capacity).  Results are identical to qasr_transcribe_batch on one engine (batch invariance). */
int qasr_dp_transcribe_batch(qasr_dp* dp, const float* const* pcm, const size_t* n, size_t B, int sample_rate, const qasr_options* opt,
                             int32_t* tokens, int32_t* lens);
int qasr_dp_timings(const qasr_dp* dp, float* ms_per_engine, int32_t cap);    /* wall time of each engine's share of the last call */
/* Whole batches in flight, one per engine: batch k runs on engine k % n_devices as ONE pass (the reference's loop body,
 * TranscribeBatchCommand.swift:82-93, without its "one after the other"); submit returns at once with a ticket, collect waits for that
 * batch and copies tokens [B, max_new_tokens + 1] / lens [B] out.  List a device twice in qasr_dp_create to keep two passes in flight on
 * one GPU: the decode stage is bound by launch latency, so the second pass runs in the first one's gaps (+30 % audio-seconds/sec at
 * 32 x 30 s on one MI355X).  The pcm / n arrays, the samples and the id arrays *opt points to must stay valid until the
 * ticket is collected (*opt itself is copied).  At most one uncollected ticket per engine: a submit whose engine still holds one, a
 * collect of a ticket that is not in flight, and qasr_dp_transcribe_batch while any ticket is in flight return QASR_ERR_INVALID.
 * Tokens are identical to qasr_transcribe_batch's.  submit / collect / destroy are for ONE caller thread (the engines' host threads
 * are the library's own). */
int qasr_dp_submit(qasr_dp* dp, const float* const* pcm, const size_t* n, size_t B, int sample_rate, const qasr_options* opt, int64_t* ticket);
int qasr_dp_collect(qasr_dp* dp, int64_t ticket, int32_t* tokens, int32_t* lens);

/* ---- tuning / diagnostic knobs ----------------------------------------------------------------
 * Process-wide A/B switches between kept kernel variants (csrc/tuning.h lists them with their measurements: "gemm_nbuf",
 * "gemv_splitb", "use_graph", ...).  Defaults are the measured winners; every value passes the parity tests.  Each knob
 * is also seeded once from the environment variable QASR_<KEY IN UPPER CASE>.  No reference counterpart.
 * QASR_ERR_INVALID: unknown key. */
int qasr_set_tuning(const char* key, int value);
/* An engine normally has its GPU to itself while a call runs, and its decode step may then use launches whose workgroups wait for each
 * other inside the launch (csrc/dec_qa.hip: q|k|v projection + attention in one launch; every wait is bounded and ends in QASR_ERR_HIP,
 * never in a hang).  Such a launch needs its whole grid resident at once: an engine that runs concurrently with OTHER engines on the same
 * GPU (qasr_dp_* with a device listed more than once sets this itself) must be marked shared = 1 and then keeps to ordinary launches.
 * A Silero VAD created with order_with = this engine (qasr_vad_create) runs on the engine's stream, between its launches, and needs no
 * mark; a VAD with a stream of its own on the same GPU is another user like a second engine.  The same holds for a WeSpeaker model
 * (qasr_spk_create): ordered on this engine it needs no mark, with a stream of its own it is another user of the GPU.
 * No reference counterpart (the reference runs one model instance per process). */
int qasr_set_shared_device(qasr_engine* engine, int shared);
int qasr_get_tuning(const char* key, int* value);

/* ---- stage entry points (oracle diffing) -------------------------------------------------- */
int qasr_num_mel_frames(size_t n_samples);              /* frames handed to the encoder */
int qasr_num_audio_tokens(const qasr_engine* e, int n_frames);
/* out: [n_mels, T] float32 row-major, T = qasr_num_mel_frames(n) (AudioPreprocessing.swift:315-316) */
int qasr_mel(qasr_engine* e, const float* pcm, size_t n, float* out);
/* mel: [n_mels, T] f32 -> out [tokens, enc_out_dim] f32 (bf16 values widened) */
int qasr_encode(qasr_engine* e, const float* mel, int n_frames, float* out);
/* audio_embeds [n_audio, hidden] f32 -> logits [vocab] f32 of the prompt's last position; keeps the
 * KV cache of slot 0 for qasr_decode_forced. */
int qasr_prefill_logits(qasr_engine* e, const float* audio_embeds, int n_audio,
                        const qasr_options* opt, float* logits);
/* teacher-forced steps on slot 0: feeds tokens[i], returns logits [n, vocab]. */
int qasr_decode_forced(qasr_engine* e, const int32_t* tokens, int n, float* logits);
/* The same two stages for a whole batch (no reference counterpart, used by tests).
 * After qasr_batch_begin (or qasr_batch_begin_staged): mel + encoder + prompt pass of the prepared batch with the logits kept.
 * logits [B][vocab] f32 = each row's last prompt position.  Leaves every row's KV cache and ctx_len ready for qasr_batch_decode_forced. */
int qasr_batch_prefill_logits(qasr_engine* e, float* logits);
/* One teacher-forced decode step for ALL rows of that batch: row b is fed tokens[b]; logits [B][vocab] f32 of the next position.
 * The step is the one qasr_batch_run captures into its graph, launched eagerly.  QASR_ERR_CAPACITY when a row's cache is full,
 * QASR_ERR_INVALID for an id outside the vocabulary or without a preceding qasr_batch_prefill_logits of the prepared batch. */
int qasr_batch_decode_forced(qasr_engine* e, const int32_t* tokens, float* logits);

/* ---- forced aligner ----------------------------------------------------------------------
 * Replaces Qwen3ForcedAligner.align / alignLong (Sources/Qwen3ASR/ForcedAligner.swift:226-331, :97-180):
 * mel -> audio encoder -> ONE decoder pass over [chat template + audio + text with <timestamp> slots] (no cache,
 * no autoregression) -> Linear(hidden, classify_num) at the slots -> argmax -> LIS monotonicity fix-up -> seconds.
 * Engines are created from the "aligner-0.6B" preset (encoder = the reference's `.forcedAligner` config); its default
 * capacity max_audio_seconds = 1200 is the reference's own mel cap (AudioPreprocessing.swift:299-313), longer clips
 * return QASR_ERR_CAPACITY. */
typedef struct qasr_aligned_word {     /* AlignedWord (Sources/AudioCommon/Protocols.swift) */
    const char* text;                  /* surface form: the word with its adjacent punctuation */
    float start_time, end_time;        /* seconds */
} qasr_aligned_word;

typedef struct qasr_alignment {        /* owned by the engine, valid until its next align call */
    const qasr_aligned_word* words;
    size_t n_words;
    const int32_t* raw_indices;        /* argmax class per timestamp slot before the fix-up (last pass), 2 per word */
    size_t n_indices;
    int32_t passes;                    /* align passes run (qasr_align: 1; qasr_align_long: 1 + re-alignments) */
} qasr_alignment;

/* TextPreprocessor.splitIntoWordPairs (TextPreprocessing.swift:103-263), default path: whitespace split, one word
 * per Han ideograph, cleaned form keeps Unicode letters / numbers / marks and the ASCII apostrophe.  *surfaces and
 * *cleaned receive '\n'-joined UTF-8 (malloc'ed, release with qasr_free); returns the word count, or
 * -QASR_ERR_UNSUPPORTED for the languages the reference hands to Apple's NLTokenizer (Japanese, Korean, Thai, Lao,
 * Khmer, Burmese, Tibetan: not reproducible) -- pass pre-split words to qasr_align_words for those.  Pure CPU. */
int qasr_split_words(const char* text, const char* language, char** surfaces, char** cleaned);
/* TimestampCorrection.longestIncreasingSubsequencePositions (TimestampCorrection.swift:102-144); returns the count. */
int qasr_lis_positions(const int32_t* values, size_t n, int32_t* positions);
/* TimestampCorrection.enforceMonotonicity (TimestampCorrection.swift:15-99); out has n entries.  Pure CPU. */
int qasr_enforce_monotonicity(const int32_t* raw, size_t n, int32_t* out);
/* Qwen3ForcedAligner.findTrailingPlateauStart (ForcedAligner.swift:196-215) on the words' start times. */
int qasr_find_trailing_plateau(const float* start_times, size_t n, float tolerance, int32_t min_size);
/* TextPreprocessor.prepareForAlignment (TextPreprocessing.swift:48-93) with the engine's tokenizer: token ids with
 * <timestamp> slots around every word, the slot positions inside ids, and the number of words kept.
 * Returns the id count or -1 (capacity / unsupported language / no tokenizer). */
int qasr_align_prepare(qasr_engine* e, const char* text, const char* language, int32_t* ids, int32_t ids_cap,
                       int32_t* ts_positions, int32_t ts_cap, int32_t* n_ts, int32_t* n_words);
/* Stage entry point (oracle diffing): forward for already slotted ids -> raw argmax class per slot; logits
 * (optional) receives [n_ts, classify_num] f32 (bf16 values widened). */
int qasr_align_raw(qasr_engine* e, const float* pcm, size_t n, const int32_t* slotted_ids, int32_t n_ids,
                   const int32_t* ts_positions, int32_t n_ts, int32_t* raw_indices, float* logits);
/* align(audio:text:sampleRate:language:) -- single pass.  16 kHz input (no resampler, as for transcribe). */
int qasr_align(qasr_engine* e, const float* pcm, size_t n, int sample_rate, const char* text, const char* language,
               qasr_alignment* out);
/* the same with caller-split words (surface + cleaned form per word): the NLTokenizer languages. */
int qasr_align_words(qasr_engine* e, const float* pcm, size_t n, int sample_rate, const char* const* surfaces,
                     const char* const* cleaned, size_t n_words, qasr_alignment* out);
/* Batched single-pass align (new: the reference aligns one utterance at a time): B clips with one text each, one
 * mel / encoder / decoder pass over the packed batch; out[b] as for qasr_align (all owned by the engine). */
int qasr_align_batch(qasr_engine* e, const float* const* pcm, const size_t* n, size_t B, int sample_rate,
                     const char* const* texts, const char* language, qasr_alignment* out);
/* alignLong: re-aligns the remainder while a trailing plateau (>= 5 words within 0.1 s) is detected on audio longer
 * than 240 s, at most 10 passes (ForcedAligner.swift:97-180). */
int qasr_align_long(qasr_engine* e, const float* pcm, size_t n, int sample_rate, const char* text,
                    const char* language, qasr_alignment* out);

/* ---- Omnilingual ASR: wav2vec2 encoder + CTC head (BASELINE configs[3]) --------------------------------------------
 * Replaces OmnilingualASRMLXModel (Sources/OmnilingualASR/MLX/OmnilingualMLXModel.swift:20-210) behind the same
 * SpeechRecognitionModel surface (MLX/OmnilingualASRMLXModel+Protocols.swift:3-15): raw 16 kHz samples -> utterance
 * layer-norm -> conv feature extractor -> positional encoder -> N pre-norm transformer layers -> CTC head -> per-frame argmax
 * -> duplicate collapse -> SentencePiece text.  Language-agnostic (the `language` hint is ignored by the reference too);
 * 40 s cap like the reference (:154-159): longer clips return QASR_ERR_CAPACITY.  Batched: clips of a call are independent. */
typedef struct qasr_ctc_engine qasr_ctc_engine;
typedef struct qasr_ctc_config {       /* OmnilingualMLXConfig (MLX/OmnilingualMLXConfig.swift:11-103) + engine capacity */
    int32_t model_dim, layers, heads, ffn_dim;
    int32_t feature_dim;               /* 512: conv feature extractor width; kernels [10,3,3,3,3,2,2], strides [5,2,2,2,2,2,2] */
    int32_t pos_kernel, pos_groups;    /* 128, 16 */
    int32_t vocab;                     /* 10288 */
    int32_t group_size, bits;          /* MLX quantisation of the encoder / head linears: 64, 4 | 8 */
    float ln_eps;                      /* 1e-5 */
    int32_t device, max_batch;
    int32_t max_audio_seconds;         /* <= 40 (the reference's cap) */
} qasr_ctc_config;
/* variant: "300M" | "1B" | "3B" | "7B", a model id such as "aufklarer/Omnilingual-ASR-CTC-1B-MLX-8bit" (detectVariant /
 * detectBits, OmnilingualMLXModel.swift:121-133), or "tiny" (test geometry). */
int qasr_ctc_default_config(const char* variant, qasr_ctc_config* out);
/* model_dir: model.safetensors (+ tokenizer.model) as published (OmnilingualMLXWeightLoader.swift:12-37); NULL = empty
 * engine filled through qasr_ctc_set_tensor (fairseq2 tensor names, PyTorch Conv1d layout, weight_g / weight_v). */
int qasr_ctc_create(const char* model_dir, const qasr_ctc_config* cfg, qasr_ctc_engine** out);
int qasr_ctc_set_tensor(qasr_ctc_engine* e, const char* name, const void* host_data, int dtype, const int64_t* shape, int ndim);
int qasr_ctc_finalize(qasr_ctc_engine* e);
/* SentencePiece vocabulary: piece texts + types (1 normal, 2 unknown, 3 control, 4 user, 5 unused, 6 byte) */
int qasr_ctc_set_pieces(qasr_ctc_engine* e, const char* const* texts, const int32_t* types, size_t n);
int qasr_ctc_is_loaded(const qasr_ctc_engine* e);
int qasr_ctc_unload(qasr_ctc_engine* e);
size_t qasr_ctc_memory_footprint(const qasr_ctc_engine* e);
void qasr_ctc_destroy(qasr_ctc_engine* e);
const char* qasr_ctc_last_error(const qasr_ctc_engine* e);
/* encoder frames for n samples (Wav2Vec2FeatureExtractor.outputLength, Wav2Vec2Frontend.swift:47-54): 160000 -> 499 */
int qasr_ctc_num_frames(size_t n_samples);
/* ids: [B][stride] collapsed token ids of every clip (argmax per frame, consecutive duplicates removed, blank kept:
 * OmnilingualMLXModel.swift:183-188), lens[b] = count; stride >= qasr_ctc_num_frames(longest clip). */
int qasr_ctc_transcribe_batch(qasr_ctc_engine* e, const float* const* pcm, const size_t* n, size_t B, int sample_rate,
                              int32_t* ids, size_t stride, int32_t* lens);
/* transcribe(audio:sampleRate:language:) -> text owned by the engine until its next call; "" for an empty clip */
int qasr_ctc_transcribe(qasr_ctc_engine* e, const float* pcm, size_t n, int sample_rate, const char** text);
/* stage entry point (oracle diffing): logits [frames][vocab] f32 of one clip */
int qasr_ctc_logits(qasr_ctc_engine* e, const float* pcm, size_t n, float* logits);
int qasr_ctc_detokenize(qasr_ctc_engine* e, const int32_t* ids, int32_t n, char* buf, size_t cap);
/* device time of the last call, ms: [0] feature extractor + positional encoder [1] transformer [2] head + argmax [3] total */
int qasr_ctc_timings(qasr_ctc_engine* e, float ms[4]);
/* pure CPU: CTCGreedyDecoder.decode (CTCGreedyDecoder.swift:28-55) -> count; OmnilingualASRModel.layerNormalize
 * (OmnilingualASR.swift:305-325) */
int qasr_ctc_greedy(const float* logits, int32_t T, int32_t V, int32_t valid_frames, int32_t* out);
int qasr_layer_normalize(const float* x, size_t n, float eps, float* out);

/* ---- Parakeet-TDT / Nemotron streaming / Parakeet-EOU (BASELINE configs[4]): the restatable slice ------------------------------
 * In the reference the FastConformer encoder, the LSTM prediction network and the joint of these models are opaque CoreML bundles
 * (`encoder.mlmodelc`, `decoder.mlmodelc`, `joint.mlmodelc`): their arithmetic is not in its tree and is NOT rebuilt here.  What the
 * reference does in Swift around them is: the log-mel front-end (CPU, Accelerate), the greedy transducer loops, vocabulary decode and
 * the streaming session's chunk cutting.  Those are the entry points below; the networks are caller-supplied callbacks. */

/* log-mel front-ends, batched on the device (csrc/nemo_mel.hip).  One launch serves every stream's chunk (64 concurrent streams x one
 * 160 ms chunk replay one captured hipGraph: H2D, three kernels, D2H) where the reference makes one Accelerate call per chunk. */
#define QASR_NEMO_MEL_TDT 0            /* MelPreprocessor.extract, Sources/ParakeetASR/MelPreprocessor.swift:52-202 (float16 values) */
#define QASR_NEMO_MEL_EOU 1            /* StreamingMelPreprocessor.extract, Sources/ParakeetStreamingASR/StreamingMelPreprocessor.swift:62-186 */
#define QASR_NEMO_MEL_RAW 2            /* extractRaw, Sources/NemotronStreamingASR/StreamingMelPreprocessor.swift:55-129 (= ParakeetStreamingASR :193-273) */
#define QASR_NEMO_MEL_EOU_STREAMING 3  /* extractStreaming (running mean / std per stream), ParakeetStreamingASR/StreamingMelPreprocessor.swift:280-393 */
typedef struct qasr_nemo_mel qasr_nemo_mel;
/* fft_scale: 2.0 = vDSP_fft_zrip's scaling as the reference states it (NemotronStreamingASR/StreamingMelPreprocessor.swift:100); only
 * the normalised variants depend on it (through the 2^-24 log guard), RAW divides it out. */
int qasr_nemo_mel_create(int device, int max_streams, size_t max_samples, float fft_scale, qasr_nemo_mel** out);
void qasr_nemo_mel_destroy(qasr_nemo_mel* m);
const char* qasr_nemo_mel_last_error(const qasr_nemo_mel* m);      /* m may be NULL: last create() failure */
int qasr_nemo_mel_num_frames(size_t n_samples);                     /* n / 160 + 1 */
int qasr_nemo_mel_length(size_t n_samples);                         /* melLength = n / 160 */
/* B clips or chunks -> out [B][128][stride] float32 (host), mel_len[b].  fit > 0: every row is cut / zero-padded to `fit` frames
 * (StreamingSession.truncateMel / padMel, Sources/NemotronStreamingASR/StreamingSession.swift:245-274); fit <= 0: nFrames of the
 * longest row.  A zero-length row gives zeros and mel_len 0 (the streaming variants' `guard !audio.isEmpty`); the reflect-padded
 * variants need more than 256 samples (the Swift code indexes out of bounds below that): QASR_ERR_INVALID.  stream_ids: the running-
 * statistics slot of each row for EOU_STREAMING (NULL = row index), ignored otherwise. */
int qasr_nemo_mel_extract(qasr_nemo_mel* m, int variant, const float* const* pcm, const size_t* n, size_t B, const int32_t* stream_ids,
                          float* out, size_t stride, int32_t* mel_len, int fit);
int qasr_nemo_mel_reset_stats(qasr_nemo_mel* m, int stream);        /* resetRunningStats; stream < 0: every stream */
/* device time of the last extract in ms (HIP events: H2D + kernels + D2H) and whether it replayed the captured graph */
int qasr_nemo_mel_timing(const qasr_nemo_mel* m, float* ms, int* was_graph);

/* ---- Silero VAD v5 (csrc/vad_silero.hip, csrc/api_vad.cpp) ------------------------------------------------------------------
 * SileroVADModel (Sources/SpeechVAD/SileroVAD.swift:39-321) with its MLX network (SileroModel.swift:1-186), rebuilt as two HIP launches
 * per call: a parallel front end (STFT magnitudes, four convolutions, LSTM input projection) and a per-stream recurrence.  One object
 * holds max_streams independent streams (LSTM h, c and the 64-sample context in HBM), each one the state of one reference instance.
 *   SileroVADModel.fromPretrained (:229-305, MLX engine; SileroWeightLoading.swift)  -> qasr_vad_create (model_dir/model.safetensors)
 *   processChunk (:108-130) / resetState (:148-157)                                   -> qasr_vad_process (B streams at once) / qasr_vad_reset
 *   detectSpeech (:168-220)                                                            -> qasr_vad_detect_speech (stream 0), qasr_vad_probs
 *   VADPipeline.binarize + filterDurations (Sources/SpeechVAD/VADPipeline.swift:117-181) -> qasr_vad_binarize
 *   StreamingVADProvider / VoiceActivityDetectionModel conformances (:308-321)        -> sc_vad_vtable_t via qasr_vad_vtable
 * Sharing a GPU with an engine: pass it as order_with and every VAD call is issued on that engine's stream, so it never runs while the
 * engine's fused decode launch needs all its workgroups resident (see qasr_set_shared_device).  The engine must outlive the VAD, and the
 * two are driven from one thread at a time, like the engine itself.  Without order_with the VAD has a stream of its own and then counts
 * as another user of the GPU for qasr_set_shared_device.  The same threading rule as the engine: one object, one thread at a time. */
typedef struct qasr_vad qasr_vad;
/* VADConfig.sileroDefault (Sources/SpeechVAD/Configuration.swift:84-91); windowDuration / stepRatio are set by detectSpeech itself */
typedef struct qasr_vad_config {
    float onset, offset, min_speech_duration, min_silence_duration;
} qasr_vad_config;
/* speech-core VAD vtable, field order as built at Sources/SpeechCore/VoicePipeline.swift:470-492 (its C header is not in the reference
 * tree; the types follow the Swift closures).  process_chunk takes exactly 512 samples at 16 kHz; on any failure it answers 0 (the
 * reference's CoreML path: `(try? ...) ?? 0.0`) with the message in qasr_vad_last_error. */
typedef struct sc_vad_vtable_t {
    void* context;
    float (*process_chunk)(void* ctx, const float* samples, size_t length);
    void (*reset)(void* ctx);
    int32_t (*input_sample_rate)(void* ctx);
    size_t (*chunk_size)(void* ctx);
} sc_vad_vtable_t;
int qasr_vad_default_config(qasr_vad_config* out);
/* Loads and checks every key and shape of model_dir/model.safetensors (f32, f16 or bf16 on disk, widened to f32) before any HIP call:
 * missing file or key -> QASR_ERR_IO, wrong shape or dtype -> QASR_ERR_INVALID, the key named in qasr_vad_last_error(NULL).
 * order_with: an engine on `device` whose stream orders the VAD's work, or NULL. */
int qasr_vad_create(int device, const char* model_dir, int max_streams, qasr_engine* order_with, qasr_vad** out);
void qasr_vad_destroy(qasr_vad* v);
const char* qasr_vad_last_error(const qasr_vad* v);                 /* v may be NULL: last create() failure */
int qasr_vad_reset(qasr_vad* v, int stream);                        /* resetState; stream < 0: every stream */
/* processChunk of B distinct streams at once: chunks [B][512] -> probs [B], each stream's state advanced.  stream_ids NULL = row index.
 * Replays one captured graph per B (H2D, two kernels, D2H). */
int qasr_vad_process(qasr_vad* v, const float* chunks, const int32_t* stream_ids, size_t B, float* probs);
/* detectSpeech's probability loop for B whole buffers (distinct streams, B <= max_streams): each row's stream is reset, walked in
 * 512-sample chunks (the last one zero-padded) and keeps its final state.  probs [B][stride] (zero past a row's chunks),
 * n_chunks[b] = ceil(n[b] / 512) (may be NULL).  Bit-identical to feeding the same chunks through qasr_vad_process. */
int qasr_vad_probs(qasr_vad* v, const float* const* pcm, const size_t* n, size_t B, const int32_t* stream_ids, float* probs, size_t stride,
                   int32_t* n_chunks);
/* VADPipeline.binarize with detectSpeech's frame duration (f32: (n * 0.032) / n per frame).  Pure CPU.  segments [cap][2] = start, end
 * in seconds; returns the segment count (only the first cap written) or -status.  cfg NULL = sileroDefault. */
int qasr_vad_binarize(const float* probs, size_t n, const qasr_vad_config* cfg, float* segments, size_t cap);
/* detectSpeech on stream 0: count of segments (as qasr_vad_binarize) or -status; sample_rate != 16000 -> -QASR_ERR_UNSUPPORTED
 * (the reference resamples with AVAudioConverter). */
int qasr_vad_detect_speech(qasr_vad* v, const float* pcm, size_t n, int sample_rate, const qasr_vad_config* cfg, float* segments,
                           size_t cap);
int qasr_vad_vtable(qasr_vad* v, int stream, sc_vad_vtable_t* out);  /* context owned by v, valid until qasr_vad_destroy */
/* device time of the last process / probs call in ms (HIP events on the work stream: H2D + kernels + D2H) and whether it was a graph */
int qasr_vad_timing(const qasr_vad* v, float* ms, int* was_graph);
/* a stream's LSTM h [128], c [128] and context [64] (any pointer may be NULL); no reference counterpart (tests) */
int qasr_vad_state(qasr_vad* v, int stream, float* h, float* c, float* context);

/* ---- WeSpeaker ResNet34 speaker embeddings (csrc/spk_wespeaker.hip, csrc/spk_conv.h, csrc/api_spk.cpp) ----------------------
 * WeSpeakerModel (Sources/SpeechVAD/WeSpeaker.swift:37-231, MLX engine) with its network (WeSpeakerModel.swift:67-170) and front end
 * (MelFeatureExtractor.swift:120-214), rebuilt as HIP launches over a ragged batch packed along the time axis:
 *   WeSpeakerModel.fromPretrained (:97-171, MLX; WeSpeakerWeightLoading.swift:15-33) -> qasr_spk_create (model_dir/model.safetensors)
 *   embed(audio:sampleRate:) (:178-213; SpeakerEmbeddingModel, Protocols.swift:249-256)   -> qasr_spk_embed, qasr_spk_embed_batch
 *   cosineSimilarity (:217-229)                                                           -> qasr_spk_cosine_similarity
 *   isLoaded / unload / memoryFootprint (WeSpeaker+Memory.swift:3-19)                     -> qasr_spk_is_loaded / _unload / _memory_footprint
 *   embeddingDimension / inputSampleRate (:62, :65)                                      -> qasr_spk_embedding_dim / _input_sample_rate
 * Sharing a GPU with an engine: as for the VAD, pass it as order_with and every call is issued on that engine's stream; without
 * order_with the model has a stream of its own and counts as another user of the GPU for qasr_set_shared_device.  The engine must
 * outlive the model.  One object, one thread at a time.
 * Precision: bf16 MFMA operands (3x3 / shortcut weights, stored activations), f32 accumulation, epilogues, front end, pooling, linear
 * and normalisation.  A clip's embedding is bit-identical alone or in any batch, and run to run. */
typedef struct qasr_spk qasr_spk;
/* fromPretrained from a local directory.  Every key, shape and dtype is checked before any HIP call: missing file or key ->
 * QASR_ERR_IO, wrong shape or dtype or an unknown key (the reference loads with verify: .noUnusedKeys) -> QASR_ERR_INVALID, the key
 * named in qasr_spk_last_error(NULL).  max_batch_samples: PCM samples one device pass holds (0 = 64 x 10 s); the workspace is sized
 * from it.  order_with: an engine on `device` whose stream orders the model's work, or NULL. */
int qasr_spk_create(int device, const char* model_dir, size_t max_batch_samples, qasr_engine* order_with, qasr_spk** out);
void qasr_spk_destroy(qasr_spk* s);
const char* qasr_spk_last_error(const qasr_spk* s);                 /* s may be NULL: last create() failure */
int qasr_spk_is_loaded(const qasr_spk* s);                          /* isLoaded (WeSpeaker+Memory.swift:4) */
int qasr_spk_unload(qasr_spk* s);                                   /* unload (:6-13): later calls return QASR_ERR_NOT_LOADED */
size_t qasr_spk_memory_footprint(const qasr_spk* s);                /* memoryFootprint (:15-18): parameter bytes as stored, 0 unloaded */
int qasr_spk_embedding_dim(void);                                   /* 256 (WeSpeaker.swift:62) */
int qasr_spk_input_sample_rate(void);                               /* 16000 (WeSpeaker.swift:65) */
/* embed(audio:sampleRate:) (WeSpeaker.swift:178-213): out[256], L2-normalised.  sample_rate != 16000 -> QASR_ERR_UNSUPPORTED (the
 * reference resamples with AVAudioConverter); n == 0 -> QASR_ERR_EMPTY_AUDIO (the reference traps on an empty array). */
int qasr_spk_embed(qasr_spk* s, const float* pcm, size_t n, int sample_rate, float* out);
/* B clips of 16 kHz PCM in one call (DiarizationPipeline.swift:369-430 calls embed once per window and speaker): out [B][256].  A call
 * larger than the workspace runs as several device passes; a single clip longer than max_batch_samples -> QASR_ERR_CAPACITY; an empty
 * clip -> QASR_ERR_EMPTY_AUDIO.  Each row is bit-identical to qasr_spk_embed of the same clip. */
int qasr_spk_embed_batch(qasr_spk* s, const float* const* pcm, const size_t* n, size_t B, float* out);
/* stage entry point, no reference counterpart: MelFeatureExtractor.extractRaw (:120-214) after CMN, [T_b][80] per clip at
 * feats + b * stride (stride >= 80 * T_b floats); n_frames[b] = T_b (may be NULL). */
int qasr_spk_fbank(qasr_spk* s, const float* const* pcm, const size_t* n, size_t B, float* feats, size_t stride, int32_t* n_frames);
int qasr_spk_num_frames(size_t n);                                  /* T = n / 160 + 1 (extractRaw's frame count) */
/* cosineSimilarity (WeSpeaker.swift:217-229), pure CPU: 0 for empty input or a zero denominator */
float qasr_spk_cosine_similarity(const float* a, const float* b, size_t n);
/* device time of the last embed / fbank call in ms (HIP events on the work stream: H2D + kernels + D2H of every pass) */
int qasr_spk_timing(const qasr_spk* s, float* ms);

/* ---- pyannote segmentation and diarization (csrc/seg_pyannote.hip, csrc/api_seg.cpp, csrc/diarize.cpp) ------------------------
 * The PyanNet segmentation network (Sources/SpeechVAD/Segmentation.swift:17-97, SincNet.swift:15-129, BiLSTM.swift:9-100,
 * PowersetDecoder.swift:23-72) and the two public things built on it, rebuilt as HIP launches over all windows of a file at once:
 *   SegmentationModel.callAsFunction (Segmentation.swift:63-84) + speakerProbabilities (PowersetDecoder.swift:23-31)
 *        + speechProbability (Segmentation.swift:93-96)                                -> qasr_seg_forward, qasr_seg_windows
 *   SegmentationWeightLoader / fromPretrained (SpeechVAD.swift:51-81)                   -> qasr_seg_create (model_dir/model.safetensors)
 *   isLoaded / unload / memoryFootprint (PyannoteVAD+Memory.swift)                      -> qasr_seg_is_loaded / _unload / _memory_footprint
 *   PyannoteVADModel.detectSpeech (SpeechVAD.swift:89-140)                              -> qasr_seg_detect_speech
 *   VADPipeline.windowPositions / aggregateFrames / binarize (VADPipeline.swift:37-181) -> qasr_seg_window_positions / _aggregate_frames / _binarize
 *   PyannoteDiarizationPipeline.diarize / extractSpeaker (DiarizationPipeline.swift:187-537) -> qasr_diarize, qasr_diar_extract_speaker
 *   DiarizationHelpers (DiarizationHelpers.swift:11-182)                                -> qasr_diar_merge_segments / _compact_speaker_ids / _cluster / _cosine_distance
 * The reference's progress / cancel callback is not carried over.  Sharing a GPU with an engine: as for the VAD and
 * WeSpeaker, pass it as order_with.  One object, one thread at a time.
 * Precision: f32 throughout.  A window's outputs are bit-identical alone, in any batch, under any max_windows, and run to run
 * (DESIGN.md section 13). */
typedef struct qasr_seg qasr_seg;
typedef struct qasr_seg_vad_config {   /* VADConfig (Configuration.swift:52-82) */
    float onset, offset, min_speech_duration, min_silence_duration, window_duration, step_ratio;
} qasr_seg_vad_config;
int qasr_seg_vad_default_config(qasr_seg_vad_config* out);         /* VADConfig.default: 0.767, 0.377, 0.136, 0.067, 10 s, 0.1 */
/* fromPretrained from a local directory.  Every key, shape and dtype (F32 / F16 / BF16, widened to f32) is checked before any HIP call:
 * missing file or required key -> QASR_ERR_IO, wrong shape or dtype or an unknown key (verify: .noUnusedKeys) -> QASR_ERR_INVALID, the
 * key named in qasr_seg_last_error(NULL).  A missing sincnet conv bias (0), norm weight (1) or norm bias (0) keeps the module's initial
 * value, as in the reference.  max_windows: windows one device pass holds (0 = 64); larger calls run as several passes with identical
 * results.  order_with: an engine on `device` whose stream orders the model's work, or NULL. */
int qasr_seg_create(int device, const char* model_dir, int max_windows, qasr_engine* order_with, qasr_seg** out);
void qasr_seg_destroy(qasr_seg* s);
const char* qasr_seg_last_error(const qasr_seg* s);                 /* s may be NULL: last create() failure */
int qasr_seg_is_loaded(const qasr_seg* s);
int qasr_seg_unload(qasr_seg* s);                                   /* later device calls return QASR_ERR_NOT_LOADED */
size_t qasr_seg_memory_footprint(const qasr_seg* s);                /* parameter bytes as stored, 0 unloaded */
/* frames for n samples: L0 = (n - 251) / 10 + 1, then /3, -4, /3, -4, /3 (all floored); 589 for 160 000; -1 below 991.  Pure CPU. */
int qasr_seg_num_frames(size_t n);
int qasr_seg_timing(const qasr_seg* s, float* ms);                  /* device time of the last call in ms (H2D + kernels + D2H) */
/* SegmentationModel.callAsFunction on pcm [B][n] (any n >= 991, else QASR_ERR_INVALID) with both decoders; F = qasr_seg_num_frames(n):
 * posteriors [B][F][7] (softmax), speaker_probs [B][F][3], speech_probs [B][F]; any of them may be NULL. */
int qasr_seg_forward(qasr_seg* s, const float* pcm, size_t B, size_t n, float* posteriors, float* speaker_probs, float* speech_probs);
/* windowPositions (VADPipeline.swift:37-60 = DiarizationPipeline.swift:319-332), pure CPU: the window count; the first min(count, cap)
 * (start, end) sample pairs are written (starts / ends may be NULL). */
int qasr_seg_window_positions(size_t n_samples, size_t window_samples, size_t step_samples, int64_t* starts, int64_t* ends, size_t cap);
/* every window of a buffer in one call: the buffer is uploaded once, each window reads it at its start (its tail past the buffer reads
 * as zero) and is bit-identical to qasr_seg_forward of the sliced, zero-padded copy.  Outputs as qasr_seg_forward with B = the count
 * and n = window_samples.  Returns the window count or -status (-QASR_ERR_CAPACITY when count > cap; nothing is run then). */
int qasr_seg_windows(qasr_seg* s, const float* pcm, size_t n_samples, size_t window_samples, size_t step_samples, float* posteriors,
                     float* speaker_probs, float* speech_probs, int64_t* starts, int64_t* ends, size_t cap);
/* VADPipeline.aggregateFrames (VADPipeline.swift:74-106) with frameDuration = window_duration / frames_per_window and its f32
 * Int(frameTime / frameDuration) indexing, pure CPU: window_probs [n_windows][frames_per_window]; the frame count (first cap written). */
int qasr_seg_aggregate_frames(const float* window_probs, size_t n_windows, size_t frames_per_window, const int64_t* starts, size_t n_samples,
                              int sample_rate, float window_duration, float* out, size_t cap);
/* hysteresis binarisation, pure CPU: filter_durations = 0 is PowersetDecoder.binarize (PowersetDecoder.swift:44-72, no duration filter),
 * 1 is VADPipeline.binarize (VADPipeline.swift:117-181, with filterDurations).  (start, end) pairs; the count or -status. */
int qasr_seg_binarize(const float* probs, size_t n, float frame_duration, const qasr_vad_config* cfg, int filter_durations, float* segments,
                      size_t cap);
/* PyannoteVADModel.detectSpeech (SpeechVAD.swift:89-140): windows of cfg->window_duration at cfg->step_ratio, aggregated and binarised
 * with the 589-frame duration.  cfg NULL = VADConfig.default.  The segment count or -status; sample_rate != 16000 -> -QASR_ERR_UNSUPPORTED. */
int qasr_seg_detect_speech(qasr_seg* s, const float* pcm, size_t n, int sample_rate, const qasr_seg_vad_config* cfg, float* segments,
                           size_t cap);

typedef struct qasr_diar_config {      /* DiarizationConfig (DiarizationPipeline.swift:11-39) */
    float onset, offset, min_speech_duration, min_silence_duration, clustering_threshold;
} qasr_diar_config;
typedef struct qasr_diar_segment {     /* DiarizedSegment */
    float start_time, end_time;
    int32_t speaker_id;
} qasr_diar_segment;
typedef struct qasr_diar_result qasr_diar_result;
int qasr_diar_default_config(qasr_diar_config* out);                /* 0.5, 0.3, 0.3, 0.15, 0.715 */
/* cosineDistance (DiarizationHelpers.swift:168-182), pure CPU: 2 for empty input or a denominator <= 1e-10 */
float qasr_diar_cosine_distance(const float* a, const float* b, size_t n);
/* constrainedAgglomerativeClustering (DiarizationHelpers.swift:83-164), pure CPU: centroid linkage, items of one window never merge,
 * first-found minimum over the sorted active list, size-weighted centroids, compact ids.  embeddings [n][dim]; assignment [n];
 * centroids [n][dim] capacity (may be NULL).  The cluster count or -status. */
int qasr_diar_cluster(const float* embeddings, const int32_t* window_index, size_t n, size_t dim, float threshold, int32_t* assignment,
                      float* centroids);
/* mergeSegments (DiarizationHelpers.swift:11-45), pure CPU: out has room for n; the count.  Speakers in ascending id, stable sorts. */
int qasr_diar_merge_segments(const qasr_diar_segment* in, size_t n, float min_silence, qasr_diar_segment* out);
int qasr_diar_compact_speaker_ids(qasr_diar_segment* segments, size_t n);    /* compactSpeakerIds (:48-58), in place */
/* PyannoteDiarizationPipeline.diarize (DiarizationPipeline.swift:209-537) behind one call: optional Silero pre-filter on vad's stream 0
 * (vad NULL = none; an empty mask gives an empty result), 10 s windows at a 5 s step, the solo-speaker clip of every (window, local
 * speaker) with at least 0.5 s, ALL clips in one qasr_spk_embed_batch, clustering, centre-zone ownership, trimToSpeechMask, sort,
 * compact, merge.  cfg NULL = the default.  *out is released with qasr_diar_result_free.  Errors are reported on seg. */
int qasr_diarize(qasr_seg* seg, qasr_spk* spk, qasr_vad* vad, const float* pcm, size_t n, int sample_rate, const qasr_diar_config* cfg,
                 qasr_diar_result** out);
const qasr_diar_segment* qasr_diar_result_segments(const qasr_diar_result* r, size_t* count);
int qasr_diar_result_num_speakers(const qasr_diar_result* r);
const float* qasr_diar_result_embeddings(const qasr_diar_result* r);         /* [num_speakers][256]; truncated / zero-padded as :519-530 */
void qasr_diar_result_free(qasr_diar_result* r);
/* the cosine argmax half of extractSpeaker (DiarizationPipeline.swift:259-275): (start, end) pairs of the speaker whose centroid is
 * most similar to target[256]; the count (first cap written) or -status */
int qasr_diar_extract_speaker(const qasr_diar_result* r, const float* target, float* segments, size_t cap);

/* ---- Open-Unmix music source separation (csrc/sep_openunmix.hip, csrc/api_sep.cpp) ----------------------------------------------------
 * Reference: Sources/SourceSeparation.  What each entry replaces:
 *   SourceSeparator.fromPretrained (SourceSeparation.swift:178-240), from a local directory        -> qasr_sep_create
 *   SourceSeparator.separate(audio:sampleRate:targets:wiener:) (:45-175), one file or many         -> qasr_sep_separate / _separate_batch
 *   STFTProcessor.forward + magnitude (STFT.swift:40-102)                                           -> qasr_sep_stft
 *   OpenUnmixStemModel.callAsFunction of the four stems (OpenUnmixModel.swift:91-127, 175-301)      -> qasr_sep_masks
 *   WienerFilterMLX.applyMLX (WienerFilterMLX.swift:26-84, 139-261)                                 -> qasr_sep_wiener
 *   STFTProcessor.inverseMLX (STFT.swift:183-231)                                                   -> qasr_sep_istft
 * Stems are numbered vocals 0, drums 1, bass 2, other 3; a target mask has bit s set for stem s; outputs keep that order.
 * Precision: f32 throughout, as the reference.  A file's stems are bit-identical alone, in any batch and position, under any
 * max_batch_samples, and run to run.  One object, one thread at a time. */
typedef struct qasr_sep qasr_sep;
typedef struct qasr_sep_config {
    int32_t wiener;                    /* 1: Wiener EM when more than one target is asked (SourceSeparation.swift:127) */
    int32_t wiener_iterations;         /* EM rounds, 1 as separate passes (1..16) */
    int32_t wiener_window;             /* frames per EM window, 300 (WienerFilterMLX.swift:34) */
} qasr_sep_config;
int qasr_sep_default_config(qasr_sep_config* out);                  /* 1, 1, 300 */
/* model_dir holds {vocals,drums,bass,other}.safetensors in the reference's keys.  The preset (hidden 512 umxhq | 1024 umxl,
 * OpenUnmixConfig.swift:24-46) is read from the shape of fc1.weight.  Every file, key, shape and dtype (F32 / F16 / BF16, widened to
 * f32) is checked before any HIP call: missing file or key -> QASR_ERR_IO, wrong shape or dtype or an unknown key -> QASR_ERR_INVALID,
 * file and key named in qasr_sep_last_error(NULL).  max_batch_samples: samples per channel one device pass holds (0 = 64 x 10 s);
 * larger calls run as several passes, split between files, with identical results.  order_with: as for qasr_seg_create. */
int qasr_sep_create(int device, const char* model_dir, size_t max_batch_samples, qasr_engine* order_with, qasr_sep** out);
void qasr_sep_destroy(qasr_sep* s);
const char* qasr_sep_last_error(const qasr_sep* s);                 /* s may be NULL: last create() failure */
int qasr_sep_is_loaded(const qasr_sep* s);
int qasr_sep_unload(qasr_sep* s);                                   /* later device calls return QASR_ERR_NOT_LOADED */
size_t qasr_sep_memory_footprint(const qasr_sep* s);                /* parameter bytes of the four stems as stored, 0 unloaded */
int qasr_sep_hidden_size(const qasr_sep* s);                        /* 512 | 1024 */
int qasr_sep_sample_rate(void);                                     /* 44100 */
int64_t qasr_sep_num_frames(size_t n);                              /* T = n / 1024 + 1 (STFT.swift:60).  Pure CPU. */
int qasr_sep_timing(const qasr_sep* s, float* ms);                  /* ms[4]: device time of the last call's stft, network, wiener, istft */
/* the recurrence kernel's form: 0 (default) W_hh streamed from L2 every step | 1 its first columns resident in registers.  Both
 * sum in the same order and give the same bits. */
int qasr_sep_set_recurrence_form(qasr_sep* s, int form);
/* separate: left[b] / right[b] hold n[b] samples at 44.1 kHz (any other rate: QASR_ERR_UNSUPPORTED; separate() does not resample either,
 * whatever its comment says); right[b] == NULL duplicates the mono channel (:52-58).  out[b] receives [targets asked, in stem order][2][n[b]].
 * cfg NULL = the default.  An empty file: QASR_ERR_EMPTY_AUDIO; a file over max_batch_samples: QASR_ERR_CAPACITY. */
int qasr_sep_separate_batch(qasr_sep* s, const float* const* left, const float* const* right, const size_t* n, size_t B, int sample_rate,
                            unsigned target_mask, const qasr_sep_config* cfg, float* const* out);
int qasr_sep_separate(qasr_sep* s, const float* left, const float* right, size_t n, int sample_rate, unsigned target_mask,
                      const qasr_sep_config* cfg, float* out);
/* stage entry points.  stft: re, im, magnitude [T][2][2049] each (any may be NULL), T = qasr_sep_num_frames(n). */
int qasr_sep_stft(qasr_sep* s, const float* left, const float* right, size_t n, float* re, float* im, float* magnitude);
/* the four stem networks on B files' magnitudes [sum T][2][2049] (file b has T[b] frames): masked magnitudes [4][sum T][2][2049] */
int qasr_sep_masks(qasr_sep* s, const float* magnitude, const size_t* T, size_t B, float* out);
/* Wiener EM of one file: masked [n_sources][T][2][2049], mixture STFT re / im [T][2][2049] -> out_re / out_im [n_sources][T][2][2049];
 * cfg gives the rounds and the window (cfg->wiener is not read) */
int qasr_sep_wiener(qasr_sep* s, const float* masked, int n_sources, const float* re, const float* im, size_t T, const qasr_sep_config* cfg,
                    float* out_re, float* out_im);
/* inverse STFT of n_spectra (1..4) spectra [n_spectra][T][2][2049] with T = length / 1024 + 1 -> out [n_spectra][2][length] */
int qasr_sep_istft(qasr_sep* s, const float* re, const float* im, int n_spectra, size_t T, size_t length, float* out);

/* ---- Qwen3-TTS 12.5 Hz speech tokenizer decoder (csrc/codec_qwen3tts.hip, csrc/api_codec.cpp) -----------------------------------------
 * Reference: Sources/Qwen3TTS/SpeechTokenizerDecoder.swift.  16 code streams at 12.5 Hz -> a 24 kHz waveform.  What each entry replaces:
 *   TTSWeightLoader.loadSpeechTokenizerDecoderWeights (TTSWeightLoading.swift:190-247), local directory -> qasr_codec_create
 *   SpeechTokenizerDecoder.callAsFunction (:658-688)                                                      -> qasr_codec_forward
 *   chunkedDecode's window loop (:696-733)                                                                -> qasr_codec_window_positions
 *   decode(codes:) (:739-744) and decodeBatch (:750-752)                                                  -> qasr_codec_decode / _decode_batch
 *   SplitResidualVectorQuantizer.decode (:513-521)                                                        -> qasr_codec_quantizer_decode
 *   DecoderTransformer.callAsFunction (:368-391)                                                          -> qasr_codec_pre_transformer
 * Codes are int32, one utterance [num_quantizers][T] with quantizer 0 the semantic stream.  Precision: f32 throughout, as the reference.
 * The chunking is part of the result (windows of 25 frames after 10 frames of context, one pass up to 35 frames).  A window's samples are
 * bit-identical alone, in any batch and place, under any max_windows, and run to run.  One object, one thread
 * at a time.  Not covered: the tokenizer's encoder, the Talker, the code predictor, bf16 or quantised forms.  Streamed chunks (qasr_tts_pool_step) are
 * windows decoded for their tail: qasr_codec_forward_tail. */
typedef struct qasr_codec qasr_codec;
/* model_dir holds model.safetensors with the decoder.* keys in the PyTorch layouts (conv [out][in][k], transposed conv [in][out][k]); a
 * codebook is read from `..._codebook.embed`, else from embedding_sum / max(cluster_usage, 1e-7) (TTSWeightLoading.swift:280-301).  The
 * geometry is SpeechTokenizerDecoderConfig's defaults (Configuration.swift:128-148) unless model_dir/config.json carries a "decoder_config"
 * object (latent_dim, decoder_dim, hidden_size, num_heads | num_attention_heads, head_dim, num_layers | num_hidden_layers, upsample_rates,
 * upsampling_ratios, num_quantizers, codebook_size | semantic_codebook_size + acoustic_codebook_size, codebook_dim, rms_norm_eps);
 * head_dim must be 64, with four upsample rates and two upsampling ratios whose product is 1920, the samples per frame every output
 * buffer here is sized by (any other geometry: QASR_ERR_INVALID at create).  Every key, shape and dtype (F32 / F16 / BF16, widened to f32)
 * is checked before any HIP call: missing file or key -> QASR_ERR_IO, wrong shape, dtype or geometry -> QASR_ERR_INVALID, the tensor named
 * in qasr_codec_last_error(NULL).  max_windows: windows one device pass holds (0 = 16, at most 512); longer inputs run in several
 * passes with identical results.  order_with: as for qasr_seg_create. */
int qasr_codec_create(int device, const char* model_dir, int max_windows, qasr_engine* order_with, qasr_codec** out);
void qasr_codec_destroy(qasr_codec* c);
const char* qasr_codec_last_error(const qasr_codec* c);             /* c may be NULL: last create() failure */
int qasr_codec_is_loaded(const qasr_codec* c);
int qasr_codec_unload(qasr_codec* c);                               /* later device calls return QASR_ERR_NOT_LOADED */
size_t qasr_codec_memory_footprint(const qasr_codec* c);            /* parameter bytes as stored, 0 unloaded */
int qasr_codec_sample_rate(void);                                   /* 24000 (Configuration.swift:143) */
int qasr_codec_samples_per_frame(void);                             /* 1920 (SpeechTokenizerDecoder.swift:698) */
int qasr_codec_num_quantizers(const qasr_codec* c);                 /* 16 (Configuration.swift:138) */
int qasr_codec_hidden_size(const qasr_codec* c);                    /* 512: row width of qasr_codec_quantizer_decode */
int qasr_codec_latent_dim(const qasr_codec* c);                     /* 1024: row width of qasr_codec_pre_transformer */
/* callAsFunction (:658-688) on B windows of T <= 35 frames each: codes [B][Q][T] -> out [B][samples_per_frame T].  clip = 0 returns the
 * signal before the clip to [-1, 1] (:685).  A code outside its codebook is QASR_ERR_INVALID, found on the host before anything is
 * uploaded; T = 0, T > 35 and a NULL buffer are QASR_ERR_INVALID too. */
int qasr_codec_forward(qasr_codec* c, const int32_t* codes, size_t B, size_t T, int clip, float* out);
/* chunkedDecode's windows for T frames (:696-733): window i decodes frames starts[i] .. ends[i] and drops its first context[i] frames.
 * Returns the window count or -status (-QASR_ERR_CAPACITY when it exceeds cap; nothing is written then).  Pure CPU. */
/* a window decoded for its tail: out [B][(T - context) x 1920], bit-identical to the last (T - context) x 1920 samples of each row of
 * qasr_codec_forward; 0 <= context < T <= 35, else QASR_ERR_INVALID.  From decoder.decoder.0 on, no launch of the vocoder does work before
 * the first row of a window that a kept sample depends on (qasr_codec_tail_leads; at T 35 / context 10 that skips 27 % of the vocoder's
 * rows), and only the kept samples are copied back.  Tuning knob codec_tail_rows: 1 skips, 0 runs whole windows; the same bits.
 * qasr_codec_forward, _decode and _decode_batch always run whole windows. */
int qasr_codec_forward_tail(qasr_codec* c, const int32_t* codes, size_t B, size_t T, size_t context, int clip, float* out);
/* pure CPU: input rows before the first kept one that each stage of the vocoder needs, from the geometry: leads[0] decoder.decoder.0 and
 * leads[1..4] blocks 1..4 (each at its input's rate), leads[5] the output conv.  upsample_rates 8 5 4 3 -> 20 14 23 28 29 6. */
int qasr_codec_tail_leads(const int32_t upsample_rates[4], int32_t leads[6]);
int64_t qasr_codec_window_positions(size_t T, int32_t* starts, int32_t* context, int32_t* ends, size_t cap);
/* decode(codes:) (:739-744): codes [Q][T], any T >= 1 -> out [samples_per_frame T], chunked as above */
int qasr_codec_decode(qasr_codec* c, const int32_t* codes, size_t T, float* out);
/* decodeBatch (:750-752) with every window of every item in one batch, max_windows per pass: codes[b] [Q][T[b]] -> out[b] */
int qasr_codec_decode_batch(qasr_codec* c, const int32_t* const* codes, const size_t* T, size_t B, float* const* out);
/* stage entry points on B windows of T <= 35 frames: codes [B][Q][T] -> out [B][T][hidden_size]; x [B][T][latent_dim] -> out the same */
int qasr_codec_quantizer_decode(qasr_codec* c, const int32_t* codes, size_t B, size_t T, float* out);
int qasr_codec_pre_transformer(qasr_codec* c, const float* x, size_t B, size_t T, float* out);
/* ms[8]: device time of the last call: quantizer + pre_conv, pre-transformer, the two upsampling stages, decoder blocks 1..4
 * (decoder.decoder.0 counted with block 1), output conv */
int qasr_codec_timing(const qasr_codec* c, float* ms);

/* ---- Qwen3-TTS 12.5 Hz speech tokenizer encoder (csrc/codec_enc_qwen3tts.hip, csrc/api_codec_enc.cpp) -------------------------------
 * Reference: Sources/Qwen3TTS/SpeechTokenizerEncoder.swift.  24 kHz mono PCM -> 16 code streams at 12.5 Hz, the other direction of
 * qasr_codec_*.  What each entry replaces:
 *   TTSWeightLoader.loadSpeechTokenizerEncoderWeights (TTSWeightLoading+Encoder.swift:14-86), local directory -> qasr_codec_enc_create
 *   SpeechTokenizerEncoder.callAsFunction (:223-241) and encode(samples:) (:246-249)                          -> qasr_codec_enc_encode / _encode_batch
 *   callAsFunction up to postConv (:224-237)                                                                  -> qasr_codec_enc_conv
 *   ... and EncoderTransformer.callAsFunction (:94-102)                                                       -> qasr_codec_enc_latent
 *   EncoderRVQ.encode (:130-134) over ResidualVectorQuantizer.encode (SpeechTokenizerDecoder.swift:467-485)   -> qasr_codec_enc_quantize
 * A clip of n >= 1 samples gives ceil(n / 1920) frames (every CausalConv1d pads on the left only; a stride-s conv gives ceil(T / s)
 * rows).  Attention has no mask: every frame of a clip attends to every frame of that clip, so a clip is never chunked and one longer
 * than max_samples is refused.  Both quantizers encode the same latent (:131-132).  Precision: f32 throughout.  A clip's rows and codes
 * are bit-identical alone, in any batch and place, under any max_samples that holds it, and run to run.  One
 * object, one thread at a time.  Not covered: the Talker, the code predictor, bf16 or quantised forms, streaming encode. */
typedef struct qasr_codec_enc qasr_codec_enc;
/* model_dir holds model.safetensors with the encoder.* keys in the PyTorch layouts (conv [out][in][k]); it may hold the decoder.* keys
 * too, as the real checkpoint does.  encoder.quantizer.rvq_{first,rest}.input_proj.weight is [hidden_size][codebook_dim][1], the matrix
 * ResidualVectorQuantizer.encode multiplies by; encoder.pre_transformer.output_proj must be present and is not applied (:100).
 * Codebooks, geometry (config.json's "decoder_config"; the channel schedule is decoder_dim / 16, / 8, .. , decoder_dim), checks and
 * statuses: as qasr_codec_create, the tensor named in qasr_codec_enc_last_error(NULL).  max_samples: samples one device pass holds
 * (0 = 720000, 30 s; at most 2^24); every buffer is sized from it at create.  order_with: as for qasr_seg_create. */
int qasr_codec_enc_create(int device, const char* model_dir, size_t max_samples, qasr_engine* order_with, qasr_codec_enc** out);
void qasr_codec_enc_destroy(qasr_codec_enc* c);
const char* qasr_codec_enc_last_error(const qasr_codec_enc* c);     /* c may be NULL: last create() failure */
int qasr_codec_enc_is_loaded(const qasr_codec_enc* c);
int qasr_codec_enc_unload(qasr_codec_enc* c);                       /* later device calls return QASR_ERR_NOT_LOADED */
size_t qasr_codec_enc_memory_footprint(const qasr_codec_enc* c);    /* parameter bytes as stored, 0 unloaded */
int qasr_codec_enc_num_quantizers(const qasr_codec_enc* c);         /* 16 (Configuration.swift:138) */
int qasr_codec_enc_hidden_size(const qasr_codec_enc* c);            /* 512: row width of qasr_codec_enc_latent and _quantize */
int qasr_codec_enc_latent_dim(const qasr_codec_enc* c);             /* 1024: row width of qasr_codec_enc_conv */
size_t qasr_codec_enc_num_frames(size_t n);                         /* ceil(n / 1920), 0 for 0.  Pure CPU. */
/* encode(samples:) (:246-249): pcm [n] -> codes [Q][frames].  n = 0, n > max_samples and a NULL buffer are QASR_ERR_INVALID. */
int qasr_codec_enc_encode(qasr_codec_enc* c, const float* pcm, size_t n, int32_t* codes);
/* B clips of any lengths, cut into passes of at most max_samples samples at clip boundaries: pcm[b] [n[b]] -> codes[b] [Q][frames] */
int qasr_codec_enc_encode_batch(qasr_codec_enc* c, const float* const* pcm, const size_t* n, size_t B, int32_t* const* codes);
/* stage entry points: out [frames][latent_dim] after post_conv (:237); out [frames][hidden_size] after the transformer's norm (:99) */
int qasr_codec_enc_conv(qasr_codec_enc* c, const float* pcm, size_t n, float* out);
int qasr_codec_enc_conv_batch(qasr_codec_enc* c, const float* const* pcm, const size_t* n, size_t B, float* const* out);
int qasr_codec_enc_latent(qasr_codec_enc* c, const float* pcm, size_t n, float* out);
int qasr_codec_enc_latent_batch(qasr_codec_enc* c, const float* const* pcm, const size_t* n, size_t B, float* const* out);
/* EncoderRVQ.encode (:130-134) of caller-supplied rows: h [F][hidden_size] -> codes [Q][F]; frames are independent */
int qasr_codec_enc_quantize(qasr_codec_enc* c, const float* h, size_t F, int32_t* codes);
/* ms[8]: device time of the last call: input conv, encoder blocks 1..4, encoder.5 + the two downsampling stages + post_conv,
 * pre-transformer, quantizer */
int qasr_codec_enc_timing(const qasr_codec_enc* c, float* ms);

/* ---- Qwen3-TTS ECAPA-TDNN speaker encoder (csrc/xvec_qwen3tts.hip, csrc/api_xvec.cpp) -----------------------------------------------
 * Reference: Sources/Qwen3TTS/SpeakerEncoder.swift.  24 kHz mono PCM of a voice-cloning reference clip -> one x-vector, what
 * Qwen3TTS.swift:222-223 and Qwen3TTS+ICL.swift:93-94 compute from the clip beside its codes (qasr_codec_enc_*).  What each entry
 * replaces:
 *   TTSWeightLoader.loadSpeakerEncoderWeights (TTSWeightLoading.swift:385-453), local directory -> qasr_xvec_create
 *   SpeakerMel.compute (SpeakerEncoder.swift:245-388)                                            -> qasr_xvec_mel
 *   SpeakerEncoder.callAsFunction (:214-238)                                                     -> qasr_xvec_embed_mel
 *   speakerEncoder(SpeakerMel.compute(audio:))                                                   -> qasr_xvec_embed / _embed_batch
 * A clip of n >= 1 samples gives n / 256 + 1 frames of 128 log-mel bins (reflect pad 512 with the reference's clamped indices, periodic
 * Hann 1024, DFT magnitudes, unnormalised HTK triangles 0 .. 12 kHz, log(max(., 1e-5))).  Every Conv1d pads with zeros inside its clip.
 * The embedding is not normalised (the reference does not).  Precision: f32 throughout.  A clip's log-mel and embedding are
 * bit-identical alone, in any batch and place, under any split into passes, and run to run.  One object, one
 * thread at a time.  Not covered: the Talker, the code predictor, resampling, bf16 forms. */
typedef struct qasr_xvec qasr_xvec;
/* model_dir: every *.safetensors file of it is searched for the speaker_encoder.* keys (:389-397: blocks.0.conv, blocks.{1,2,3}.{tdnn1.conv,
 * tdnn2.conv, res2net_block.blocks.{0..6}.conv, se_block.conv1, se_block.conv2}, mfa.conv, asp.tdnn.conv, asp.conv, fc; .weight
 * [out][k][in] as stored (:436-437), .bias); F32, F16 or BF16, widened at upload.  Other keys are neither read nor an error.  The
 * embedding width is fc.weight's first dimension.  Everything is checked before any HIP call: a missing key, or no speaker_encoder.
 * key at all -> QASR_ERR_IO, a wrong shape or dtype -> QASR_ERR_INVALID, the key named in qasr_xvec_last_error(NULL).  max_samples:
 * samples one device pass holds (0 = 64 x 10 s; at most 2^28); every buffer is sized from it at create: about 82 bytes of device
 * memory per sample (4864 f32 per frame of activations, the PCM, the tile partials) plus 0.1 GB that does not depend on it (f32
 * weights, room for 1024 clips), so 1.4 GB at the default and 0.12 GB for one 10 s clip (max_samples = 240000).  order_with: as for
 * qasr_seg_create. */
int qasr_xvec_create(int device, const char* model_dir, size_t max_samples, qasr_engine* order_with, qasr_xvec** out);
void qasr_xvec_destroy(qasr_xvec* x);
const char* qasr_xvec_last_error(const qasr_xvec* x);               /* x may be NULL: last create() failure */
int qasr_xvec_is_loaded(const qasr_xvec* x);
int qasr_xvec_unload(qasr_xvec* x);                                 /* later device calls return QASR_ERR_NOT_LOADED */
size_t qasr_xvec_memory_footprint(const qasr_xvec* x);              /* parameter bytes as stored, 0 unloaded */
int qasr_xvec_embedding_dim(const qasr_xvec* x);                    /* fc.weight's rows: 1024 in the reference (:204-206) */
int qasr_xvec_input_sample_rate(void);                              /* 24000 (:259) */
size_t qasr_xvec_num_frames(size_t n);                              /* n / 256 + 1 (:305), 0 for 0.  Pure CPU. */
/* Qwen3TTS.swift:222-223: pcm [n] -> out [E].  sample_rate != 24000 -> QASR_ERR_UNSUPPORTED (the reference resamples with
 * AVAudioConverter, :249-251); n == 0 -> QASR_ERR_EMPTY_AUDIO; n > max_samples -> QASR_ERR_CAPACITY; NULL -> QASR_ERR_INVALID;
 * after qasr_xvec_unload every argument gives QASR_ERR_NOT_LOADED. */
int qasr_xvec_embed(qasr_xvec* x, const float* pcm, size_t n, int sample_rate, float* out);
/* B clips of any lengths at 24 kHz, cut into passes of at most max_samples samples at clip boundaries: out [B][E]; each row is
 * bit-identical to qasr_xvec_embed of that clip */
int qasr_xvec_embed_batch(qasr_xvec* x, const float* const* pcm, const size_t* n, size_t B, float* out);
/* stage entry points: SpeakerMel.compute (:247-278), out[b] [n[b] / 256 + 1][128]; the network alone (:214-238) on mel [T][128] */
int qasr_xvec_mel(qasr_xvec* x, const float* const* pcm, const size_t* n, size_t B, float* const* out);
int qasr_xvec_embed_mel(qasr_xvec* x, const float* mel, size_t T, float* out);
/* ms[6]: device time of the last call, HIP events on the work stream: front end, initial conv, blocks 1..3, MFA + pooling + fc */
int qasr_xvec_timing(const qasr_xvec* x, float* ms);

/* ---- CosyVoice3 HiFT vocoder (csrc/voc_cosyvoice.hip, csrc/api_voc.cpp) ----------------------------------------------------------------
 * Reference: Sources/CosyVoiceTTS/HiFiGAN.swift.  80-bin mel frames (20 ms each) -> 24 kHz mono PCM, what HiFiGANGenerator.decode(mel:)
 * computes for CosyVoiceTTS.  What each entry replaces:
 *   CosyVoiceWeightLoader.loadHiFiGAN (WeightLoading.swift:214-331), local directory           -> qasr_hift_create
 *   F0Predictor.callAsFunction (HiFiGAN.swift:361-373)                                           -> qasr_hift_f0
 *   interpolateF0 + SourceModuleHnNSF.callAsFunction (:383-395, :253-289, :323-328)              -> qasr_hift_source
 *   stft, conv_pre, the three stages, conv_post, istft, clip (:777-857) on a given source       -> qasr_hift_decode_source
 *   HiFiGANGenerator.decode(mel:) (:755-868)                                                     -> qasr_hift_decode / _decode_batch
 * A clip of T >= 1 frames gives 480 T source samples, 120 T + 1 STFT frames (n_fft 16, hop 4, periodic Hann, reflect padding 8) and
 * 480 T + 16 PCM samples: the inverse STFT's centre padding is not trimmed (:566-568).  Snake is x + 1 / (alpha + 1e-9) sin^2(alpha x)
 * with alpha as stored; the phase channels of conv_post go through sin, the last LeakyReLU has slope 0.01 (:838-849).
 * Noise.  MLX's random stream cannot be restated; the distribution and the three places noise enters are the reference's, the
 * generator is this library's: draw c of a clip is splitmix64(seed + (c + 1) 0x9e3779b97f4a7c15) (the counter form of the sampler's
 * generator); with r the draw, u1 = ((r >> 40) + 1) 2^-24, u2 = ((r >> 16) & 0xFFFFFF) 2^-24, uniform = u2, normal = sqrt(-2 ln u1)
 * cos(2 pi u2).  Counter h = 0 .. 8: initPhase of harmonic h + 1 = 2 pi uniform; counter 16 + 10 n + h: the unvoiced noise of sample n,
 * harmonic h + 1; counter 16 + 10 n + 9: the noise added to sample n after the merge.
 * Precision: f32 throughout; the source's running phase is kept in cycles in f64 and reduced mod 1 before the sine.  A clip's output
 * is bit-identical alone, in any batch and place, under any split into passes, and run to run; qasr_hift_decode is bit-identical to
 * the three stage entries chained.  One object, one thread at a time.  Not covered: the LLM, the flow model,
 * CAM++, the speech tokenizer, chunked / streaming vocoding. */
typedef struct qasr_hift qasr_hift;
/* model_dir/hifigan.safetensors: conv_pre, ups.{0..2}, source_downs.{0..2}, conv_post, f0_predictor.condnet.{0,2,4,6,8} (.weight
 * [out][k][in] as stored, .bias), f0_predictor.classifier and m_source.l_linear (.weight [out][in], .bias), and for resblocks.{0..8}
 * (3 stage + kernel) and source_resblocks.{0..2}: convs1.{0..2}, convs2.{0..2}, activations1.{0..2}.alpha, activations2.{0..2}.alpha;
 * F32, F16 or BF16, widened at upload.  The file's beta, up_activations.* and final_activation.* are not read, as in the reference.
 * Everything is checked before any HIP call: a missing file or key -> QASR_ERR_IO, a wrong shape or dtype -> QASR_ERR_INVALID, the
 * key named in qasr_hift_last_error(NULL).  max_frames: mel frames one device pass holds (0 = 4096, about 82 s; at most 2^17); every
 * buffer is sized from it at create: about 160 KB of device memory per frame (five activation buffers of 120 x 64 f32, the source,
 * its STFT, the PCM) plus 0.1 GB that does not depend on it, so 0.75 GB at the default.  order_with: as for qasr_seg_create. */
int qasr_hift_create(int device, const char* model_dir, size_t max_frames, qasr_engine* order_with, qasr_hift** out);
void qasr_hift_destroy(qasr_hift* h);
const char* qasr_hift_last_error(const qasr_hift* h);               /* h may be NULL: last create() failure */
int qasr_hift_is_loaded(const qasr_hift* h);
int qasr_hift_unload(qasr_hift* h);                                 /* later device calls return QASR_ERR_NOT_LOADED */
size_t qasr_hift_memory_footprint(const qasr_hift* h);              /* bytes as stored of the tensors read, 0 unloaded */
int qasr_hift_sample_rate(void);                                    /* 24000 */
size_t qasr_hift_num_samples(size_t T);                             /* 480 T + 16, 0 for 0.  Pure CPU. */
/* The noise stream on the host, the twin of the device code (the same lines, csrc/voc_cosyvoice.h): for draw counters[i] of the stream
 * `seed`, uniform[i] = u2 and normal[i] = sqrt(-2 ln u1) cos(2 pi u2) in f32; either output may be NULL.  Pure CPU. */
int qasr_hift_noise(uint64_t seed, const uint64_t* counters, size_t n, float* uniform, float* normal);
/* Stage entries.  mel [T][80], f0 [T] (Hz, >= 0), src [480 T], pcm [480 T + 16].  T == 0, T > max_frames or NULL -> QASR_ERR_INVALID;
 * after qasr_hift_unload every argument gives QASR_ERR_NOT_LOADED. */
int qasr_hift_f0(qasr_hift* h, const float* mel, size_t T, float* f0);
int qasr_hift_source(qasr_hift* h, const float* f0, size_t T, uint64_t seed, float* src);
int qasr_hift_decode_source(qasr_hift* h, const float* mel, size_t T, const float* src, float* pcm);
/* the whole generator: bit-identical to qasr_hift_decode_source(mel, qasr_hift_source(qasr_hift_f0(mel), seed)) */
int qasr_hift_decode(qasr_hift* h, const float* mel, size_t T, uint64_t seed, float* pcm);
/* B clips of any lengths, cut into passes of at most max_frames frames at clip boundaries; pcm[b] [480 T[b] + 16] is bit-identical to
 * qasr_hift_decode of that clip with seeds[b] */
int qasr_hift_decode_batch(qasr_hift* h, const float* const* mel, const size_t* T, const uint64_t* seeds, size_t B, float* const* pcm);
/* ms[7]: device time of the last call, HIP events on the work stream: F0 predictor, source, STFT, conv_pre, stage 0, stage 1, stage 2 +
 * conv_post + inverse STFT; a stage the entry does not run is 0 */
int qasr_hift_timing(const qasr_hift* h, float* ms);

/* ---- VoxCPM2 AudioVAE (csrc/vae_voxcpm.hip, csrc/api_avae.cpp) ---------------------------------------------------------------------------
 * Reference: Sources/VoxCPM2TTS/AudioVAE.swift.  16 kHz mono PCM -> latent frames [F][latent_dim] at 25 frames per second (hop 640), and
 * latent frames -> 48 kHz PCM, 1920 samples per frame.  What each entry replaces:
 *   AudioVAEConfig.init(from:) (Configuration.swift:171-186), AudioVAE.sanitize (AudioVAE.swift:646-686) and the loaders of
 *   VoxCPM2TTS.swift:450-511, :743-850, local directory                                          -> qasr_avae_create
 *   AudioVAE.preprocess + CausalEncoder.callAsFunction (:636-644, :456-460)                      -> qasr_avae_encode / _encode_batch
 *   AudioVAE.decode / CausalDecoder.callAsFunction (:630-634, :536-561)                          -> qasr_avae_decode / _decode_batch
 *   CausalEncoder.conv_in / blocks[k - 1], CausalDecoder.conv_in / blocks[k - 1]                 -> qasr_avae_enc_stage / _dec_stage
 *   snake_out, conv_out, tanh (:558-560)                                                         -> qasr_avae_dec_output
 * Every conv is causal: zeros go in front of the already-Snaked input only, so decode(z[:k]) is the first 1920 k samples of decode(z).
 * Snake is x + 1 / (alpha + 1e-9) sin^2(alpha x) with alpha as stored.  A clip of n samples is padded with zero samples to a whole
 * frame (real rows: conv_in has a bias) and gives ceil(n / hop) frames.  sr_cond picks the row of the decoder's scale / bias tables:
 * the number of sr_bin_boundaries it has reached; 0 means out_sample_rate.
 * Precision: f32 throughout, as the reference runs this model.  A clip's output is bit-identical alone, in any batch and place, under
 * any split into passes, and run to run.  The tuning knob vae_fuse_c picks, per width, between two forms of a residual unit that sum in
 * different orders; both are held to the same bounds.  One object, one thread at a time.  Not covered: the
 * VoxCPM2 LM, feature encoder, DiT and FSQ, streaming decode, resampling (input other than sample_rate is the caller's to convert), the
 * noise block, bf16 operands. */
typedef struct qasr_avae qasr_avae;
/* model_dir/config.json's audio_vae_config is optional, every field of it defaults as in the reference.  The tensors are looked up in all
 * *.safetensors of the directory under audio_vae.{encoder,decoder}.* or the bare encoder.* / decoder.*; a conv's .weight may be stored as
 * a .weight_g [out][1][1] / .weight_v pair, fused to g v / (|v| + 1e-9) (formed in f64, rounded once); fc_logvar is not read; a
 * 64-wide sr_cond_layers table may be [n][8][8] or [n][64].  F32, F16 or BF16, widened at upload.  Everything is checked before any HIP
 * call, the field or tensor named in qasr_avae_last_error(NULL): use_noise_block true, depthwise false, a cond_type other than
 * scale_bias / scale_bias_init, rates or widths outside the ranges held, a wrong shape or dtype -> QASR_ERR_INVALID; a missing tensor
 * (every decoder block needs its sr_cond_layers entry: the reference would keep a random table) -> QASR_ERR_IO.
 * max_frames: latent frames one device pass holds (0 = 1024, 41 s; at most 2^14); the buffers are sized from it at create: three
 * activation buffers of 81,920 f32 per frame at the default geometry plus PCM and latents, about 1 MB per frame.  order_with: as for
 * qasr_seg_create. */
int qasr_avae_create(int device, const char* model_dir, size_t max_frames, qasr_engine* order_with, qasr_avae** out);
void qasr_avae_destroy(qasr_avae* h);
const char* qasr_avae_last_error(const qasr_avae* h);               /* h may be NULL: last create() failure */
int qasr_avae_is_loaded(const qasr_avae* h);
int qasr_avae_unload(qasr_avae* h);                                 /* later device calls return QASR_ERR_NOT_LOADED */
size_t qasr_avae_memory_footprint(const qasr_avae* h);              /* bytes as stored of the tensors read, 0 unloaded */
int qasr_avae_latent_dim(const qasr_avae* h);                       /* 64 */
int qasr_avae_in_sample_rate(const qasr_avae* h);                   /* 16000 */
int qasr_avae_out_sample_rate(const qasr_avae* h);                  /* 48000 */
int qasr_avae_hop(const qasr_avae* h);                              /* 640: the product of encoder_rates */
int qasr_avae_samples_per_frame(const qasr_avae* h);                /* 1920: the product of decoder_rates */
size_t qasr_avae_num_frames(const qasr_avae* h, size_t n);          /* ceil(n / hop); h NULL: the default hop 640.  Pure CPU. */
int qasr_avae_num_blocks(const qasr_avae* h, int decoder);          /* encoder (0) or decoder (1) blocks: stages run 0 .. this */
/* rows per latent frame and width of stage k's output (k = 0: after conv_in, k >= 1: after block k - 1); k out of range -> QASR_ERR_INVALID */
int qasr_avae_stage_shape(const qasr_avae* h, int decoder, int k, int* rows_per_frame, int* width);
/* pcm [n] at in_sample_rate -> z [ceil(n / hop)][latent_dim].  n == 0, more frames than max_frames or NULL -> QASR_ERR_INVALID */
int qasr_avae_encode(qasr_avae* h, const float* pcm, size_t n, float* z);
/* z [T][latent_dim] -> pcm [samples_per_frame T].  T == 0, T > max_frames, sr_cond < 0 or NULL -> QASR_ERR_INVALID */
int qasr_avae_decode(qasr_avae* h, const float* z, size_t T, int sr_cond, float* pcm);
/* B clips of any lengths, cut into passes of at most max_frames frames at clip boundaries; each output is bit-identical to the single entry */
int qasr_avae_encode_batch(qasr_avae* h, const float* const* pcm, const size_t* n, size_t B, float* const* z);
int qasr_avae_decode_batch(qasr_avae* h, const float* const* z, const size_t* T, size_t B, int sr_cond, float* const* pcm);
/* Stage entries: out [frames x rows_per_frame][width] of qasr_avae_stage_shape, the rows as the reference holds them at that point
 * (a decoder stage before the next block's scale / bias and Snake) */
int qasr_avae_enc_stage(qasr_avae* h, const float* pcm, size_t n, int k, float* out);
int qasr_avae_dec_stage(qasr_avae* h, const float* z, size_t T, int sr_cond, int k, float* out);
/* rows [samples_per_frame T][width of the last decoder stage] as qasr_avae_dec_stage returns them -> pcm; chained they are qasr_avae_decode's bits */
int qasr_avae_dec_output(qasr_avae* h, const float* rows, size_t T, float* pcm);
/* ms[20]: device time of the last call, HIP events on the work stream.  ms[0] encoder conv_in, ms[1 ..] its blocks, then fc_mu;
 * ms[10] decoder conv_in, ms[11 ..] its blocks, then conv_out + tanh; a stage the entry does not run is 0 */
int qasr_avae_timing(const qasr_avae* h, float* ms);

/* ---- Qwen3-TTS Talker + code predictor (Sources/Qwen3TTS/Talker.swift, CodePredictor.swift, Sampling.swift, Qwen3TTS.swift) -------------
 * Text ids (the chat template of prepareTextTokens around them), a language id, optionally a speaker token id or an x-vector (qasr_xvec_*)
 * and an instruct prefix -> 16 code streams at 12.5 Hz, which qasr_codec_decode turns into 24 kHz audio.  MLX affine 4 / 8 bit
 * checkpoints only (keys talker.* and talker.code_predictor.* in any *.safetensors of the directory); a float checkpoint is refused.
 * Rows of a call are independent: own prompt length, position, trailing text, history and finished flag; a row's codes are the same
 * bits alone, in any batch, at any slot and under any max_batch.  One object, one thread at a time.
 * HBM: the packed weights (0.6B 4-bit: about 0.5 GB with the bf16 embedding tables) plus the Talker KV cache, 2 images x layers x
 * kv_heads x head_dim x 2 bytes x positions per row: 28 x 8 x 128 x 2 x 2 = 114,688 bytes per position; positions = max_instruct + 11
 * prompt + max_frames + 1, rounded up to 32 (544 by default; the 510 a row can reach are 3.8 GB of it at max_batch 64, the allocation 4.0 GB).
 * ICL voice cloning (Qwen3TTS+ICL.swift: synthesizeWithVoiceCloneICL) is qasr_tts_*_icl / qasr_tts_clone below, on a handle from
 * qasr_tts_create_icl; streaming synthesis (synthesizeStream) is the stream pool qasr_tts_pool_* further below.  Not covered: top_p < 1,
 * the text tokenizer, host resampling, ReferenceAudioCache. */
typedef struct qasr_tts qasr_tts;
typedef struct qasr_tts_config {
    int32_t hidden, layers, heads, kv_heads, head_dim, inter;          /* Talker: 1024 28 16 8 128 3072 (1.7B: 2048 .. 6144) */
    int32_t text_vocab, text_hidden, codec_vocab;                      /* 151936 2048 3072 */
    int32_t cp_hidden, cp_embedding_dim, cp_layers, cp_heads, cp_kv_heads, cp_head_dim, cp_inter, cp_vocab;   /* 1024 1024 5 16 8 128 3072 2048 */
    float rms_eps, rope_theta, cp_rms_eps, cp_rope_theta;              /* 1e-6 1e6 1e-6 1e6 */
    int32_t bits, group_size;                                          /* 4 | 8, 64 */
    int32_t codec_pad, codec_bos, codec_eos, codec_think, codec_nothink, codec_think_bos, codec_think_eos;   /* 2148 2149 2150 2154 2155 2156 2157 */
    int32_t suppress_lo, suppress_hi;                                  /* [2048, 3072): never sampled, except codec_eos */
    int32_t tts_pad, tts_bos, tts_eos;                                 /* text side: 151671 151672 151673 */
    int32_t max_batch;                                                 /* rows of one call, 1 .. 64 (default 8) */
    int32_t max_frames;                                                /* 1 .. 500 (default and cap: the reference's safeMaxTokens) */
    int32_t max_text, max_instruct;                                    /* ids per row (defaults 512, 0) */
    int32_t device;
} qasr_tts_config;
typedef struct qasr_tts_sampling {          /* SamplingConfig (Sampling.swift:5-30); minP is declared and never read there: no field */
    float temperature;                      /* 0.9; <= 0: greedy (the first maximum) */
    int32_t top_k;                          /* 50; <= 0 or >= vocabulary: off */
    float top_p;                            /* 1.0; < 1 is refused (QASR_ERR_UNSUPPORTED): the reference's branch masks the likeliest tokens */
    float repetition_penalty;               /* 1.05; 1.0 = the reference's batch path */
    int32_t max_tokens;                     /* frames, capped by the handle's max_frames; <= 0: max_frames */
    float eos_logit_bias;                   /* 0 */
} qasr_tts_sampling;
typedef struct qasr_tts_request {
    size_t B;
    const int32_t* const* text; const int32_t* text_len;        /* [B]: templated ids, at least 9 */
    const int32_t* language;                                    /* [B]: codec language ids */
    const int32_t* speaker;                                     /* [B] or NULL; < 0: none */
    const float* const* xvector;                                /* [B] or NULL; NULL entry: none; `hidden` floats each */
    const int32_t* const* instruct; const int32_t* instruct_len;/* [B] or NULL; prepareInstructTokens' ids */
    const int64_t* row_index;                                   /* [B] or NULL (0 .. B-1): the caller's index of the row, which keys its random stream */
} qasr_tts_request;
/* model: "0.6B" | "1.7B" (or a model id containing "1.7B"), bits 4 | 8: Qwen3TTSConfig.config(for:bits:) with the CodecTokens ids */
int qasr_tts_default_config(const char* model, int bits, qasr_tts_config* out);
void qasr_tts_default_sampling(int greedy, qasr_tts_sampling* out);
/* missing file or key -> QASR_ERR_IO; wrong shape / dtype, a float checkpoint, a geometry the kernels do not serve (widths not multiples
 * of 64, head_dim != 128, heads != 2 kv_heads, cp_embedding_dim != hidden, vocabularies over 4096 codes) -> QASR_ERR_INVALID */
int qasr_tts_create(const char* model_dir, const qasr_tts_config* cfg, qasr_tts** out);
void qasr_tts_free(qasr_tts* t);
const char* qasr_tts_last_error(const qasr_tts* t);                /* t may be NULL: last create() failure */
size_t qasr_tts_memory_footprint(const qasr_tts* t);               /* parameter bytes as stored */
size_t qasr_tts_device_bytes(const qasr_tts* t);                   /* every device allocation of the handle */
int qasr_tts_poll_interval(void);                                  /* frames between two host reads of the finished flags (8) */
/* codes [B][16][max_frames] int32 (max_frames = the handle's; entries past n_frames[b] are -1), n_frames [B].  A row whose first token
 * is EOS has 0 frames.  B > max_batch -> QASR_ERR_CAPACITY; a text shorter than 9 ids, an id outside its vocabulary, a NULL buffer ->
 * QASR_ERR_INVALID; too many text / instruct ids -> QASR_ERR_CAPACITY; top_p < 1 -> QASR_ERR_UNSUPPORTED. */
int qasr_tts_generate(qasr_tts* t, const qasr_tts_request* rq, const qasr_tts_sampling* s, uint64_t seed, int32_t* codes, int32_t* n_frames);
/* teacher-forced pass: forced codes [B][16][T], T <= max_frames -> talker_logits [B][T][codec_vocab], cp_logits [B][T][15][cp_vocab],
 * hidden [B][T][hidden] (post-norm), any of them NULL.  No sampling decides what is fed. */
int qasr_tts_forced(qasr_tts* t, const qasr_tts_request* rq, const int32_t* codes, size_t T, float* talker_logits, float* cp_logits,
                    float* hidden);
/* the host twin of the device sampler on one row of logits [V]: talker != 0 applies the suppress range, the penalty over history[n_history]
 * and the EOS rules with cfg's ids (cfg NULL: the defaults), else sampleTokenLazy.  Returns the token or -status.  Pure CPU. */
int qasr_tts_sample_host(const qasr_tts_config* cfg, const float* logits, int32_t V, int talker, const qasr_tts_sampling* s,
                         const int32_t* history, int32_t n_history, uint64_t seed, int64_t row_index, int32_t frame, int32_t group);
/* generate, then the caller's codec handle: pcm[b] holds 1920 x max_frames floats, n_samples[b] = 1920 x n_frames[b] of them are written.
 * codes / n_frames as qasr_tts_generate, may be NULL. */
int qasr_tts_synthesize(qasr_tts* t, qasr_codec* codec, const qasr_tts_request* rq, const qasr_tts_sampling* s, uint64_t seed,
                        float* const* pcm, size_t* n_samples, int32_t* codes, int32_t* n_frames);

/* ---- ICL voice cloning (Sources/Qwen3TTS/Qwen3TTS+ICL.swift) ---------------------------------------------------
 * The reference clip's codes (qasr_codec_enc_encode) and transcript go into the Talker's context beside the x-vector.  A row's prompt has
 * P = 11 + ref_text_len + target ids + ref_frames positions (buildICLPrefillEmbeddings): role 3 | tts_pad x 5 + tts_bos over think,
 * think_bos, language, think_eos, x-vector, codec_pad | reference-text ids, then target ids, then tts_eos, each over codec_pad | tts_pad
 * over codec_bos | tts_pad over the summed 16 code embeddings of every reference frame.  No trailing text: every generated frame adds tts_pad.
 * rq->text stays templated (role = text[0..3), target ids = text[3 .. n-5)); rq->xvector[b] is required; a speaker token or an instruct
 * prefix -> QASR_ERR_INVALID; a reference code outside its table (stream 0: codec_vocab, streams 1..15: cp_vocab) -> QASR_ERR_INVALID (not
 * clamped); ref_frames / ref_text_len over the handle's capacity -> QASR_ERR_CAPACITY (a handle from qasr_tts_create has capacity 0).
 * Every refusal names the row in qasr_tts_last_error.
 * qasr_tts_create_icl is qasr_tts_create with the Talker cache, the RoPE tables and the prompt buffers sized for 11 + max_ref_text +
 * max_text + max_ref_frames + max_frames + 1 positions, rounded up to 64 (the prompt pass moves the V images in blocks of 64 keys), at most
 * 32768; over that, max_ref_frames < 1 or max_ref_text < 0 -> QASR_ERR_INVALID before any device call.  It also allocates the packed
 * prompt pass's scratch: one layer of bf16 weights (0.6B: 31 MB) and, per prompt position and batch row, 2 x hidden + 3 x heads x
 * head_dim + 2 x kv_heads x head_dim + inter bf16 values plus one V^T column (0.6B: 26,624 + 2,048 bytes) next to the 114,688 bytes
 * of the cache.  qasr_tts_device_bytes counts all of it.  Tuning knob tts_packed_prompt: 1 = ICL prompts take one packed pass, 0 = one
 * decode step per position; calls without ICL always take the step path. */
typedef struct qasr_tts_icl {                                     /* accompanies a qasr_tts_request, one entry per row */
    const int32_t* const* ref_text;  const int32_t* ref_text_len;  /* [B] tokenizer.encode(referenceText), no template; length >= 0 */
    const int32_t* const* ref_codes; const int32_t* ref_frames;    /* [B] [16][ref_frames[b]] as qasr_codec_enc_encode writes them; >= 1 frame */
} qasr_tts_icl;
int qasr_tts_create_icl(const char* model_dir, const qasr_tts_config* cfg, int32_t max_ref_frames, int32_t max_ref_text, qasr_tts** out);
int qasr_tts_icl_capacity(const qasr_tts* t, int32_t* max_ref_frames, int32_t* max_ref_text);     /* 0, 0 on a plain handle */
/* as qasr_tts_generate / _forced / _synthesize with the ICL prompt */
int qasr_tts_generate_icl(qasr_tts* t, const qasr_tts_request* rq, const qasr_tts_icl* icl, const qasr_tts_sampling* s, uint64_t seed,
                          int32_t* codes, int32_t* n_frames);
int qasr_tts_forced_icl(qasr_tts* t, const qasr_tts_request* rq, const qasr_tts_icl* icl, const int32_t* codes, size_t T, float* talker_logits,
                        float* cp_logits, float* hidden);
int qasr_tts_synthesize_icl(qasr_tts* t, qasr_codec* codec, const qasr_tts_request* rq, const qasr_tts_icl* icl, const qasr_tts_sampling* s,
                            uint64_t seed, float* const* pcm, size_t* n_samples, int32_t* codes, int32_t* n_frames);
/* the prompt rows as the Talker reads them: rows [B][P_max][hidden] (bf16 values widened, zeros past a row's P; P_max = the call's longest,
 * at most 11 + max_ref_text + max_text + max_ref_frames), P [B] */
int qasr_tts_icl_prompt(qasr_tts* t, const qasr_tts_request* rq, const qasr_tts_icl* icl, float* rows, int32_t* P);
/* synthesizeWithVoiceCloneICL end to end for B rows: qasr_codec_enc_encode_batch -> qasr_xvec_embed_batch -> qasr_tts_synthesize_icl.
 * rq->xvector is ignored; ref_pcm[b] [ref_n[b]] is 24 kHz mono (the reference resamples on the host: not rebuilt, nor its
 * ReferenceAudioCache -- a caller who wants the cache keeps codes and x-vector and calls qasr_tts_synthesize_icl).  A speaker encoder
 * whose embedding dimension is not the Talker's hidden size -> QASR_ERR_INVALID. */
int qasr_tts_clone(qasr_tts* t, qasr_codec_enc* codec_enc, qasr_xvec* xvec, qasr_codec* codec, const qasr_tts_request* rq,
                   const int32_t* const* ref_text, const int32_t* ref_text_len, const float* const* ref_pcm, const size_t* ref_n,
                   const qasr_tts_sampling* s, uint64_t seed, float* const* pcm, size_t* n_samples, int32_t* codes, int32_t* n_frames);

/* ---- streaming synthesis: a pool of concurrent streams (Qwen3TTS.swift:297-608 synthesizeStream, runStreamingGeneration,
 * decodeAndEmitChunk) -------------------------------------------------------------------------------------------
 * A pool borrows a Talker handle and a codec handle and holds up to max_batch streams, one per batch row (slot) of the frame step.  A
 * stream joins at any frame and leaves at any frame without changing a bit of any other: its codes equal qasr_tts_generate of the same
 * request (B = 1, the pool's sampling and seed, rq->row_index[0] keying its random numbers), its chunks are those qasr_tts_stream_chunks
 * names, and a chunk's samples are the last 1920 x n_frames samples of qasr_codec_forward (clip = 1) on the frames
 * max(frame_index - decoder_left_context, 0) .. frame_index + n_frames, all-zero frames prepended while they are fewer than 4.
 * Chunk boundaries: a chunk when the stream's frame count reaches first_chunk_frames, then every chunk_frames; at EOS the remaining frames
 * as the final chunk, or a final chunk without samples when nothing remains (EOS as the first token: one empty final chunk at frame 0);
 * a stream that stops at max_tokens (capped by max_frames) ends with its last chunk marked final, no empty chunk behind it.  (The
 * reference's loop agrees but for max_tokens = 1 with first_chunk_frames = 1, where it sends that frame as a non-final chunk and an empty
 * final one behind it.)
 * While a pool exists on a Talker handle, qasr_tts_generate / _forced / _synthesize, the ICL calls and a second qasr_tts_pool_create on it
 * return QASR_ERR_INVALID: the pool owns the handle's rows.  After qasr_tts_pool_destroy they work as before.  Destroy the pool before
 * the handles it borrows.  One thread at a time for the pool and both handles.
 * Not covered: ICL streams (no entry takes a qasr_tts_icl; plain streams run on an ICL handle too), the sc_tts_vtable_t bridge (it takes a text string; the text tokenizer stays with the
 * caller), warmUp, a packed prompt pass for admission (a stream's prompt runs one position per step while the other streams wait), the
 * noChunking preset (decoder_left_context + chunk_frames > 35: use qasr_tts_synthesize). */
typedef struct qasr_tts_pool qasr_tts_pool;
typedef struct qasr_tts_stream_config { int32_t first_chunk_frames, chunk_frames, decoder_left_context; } qasr_tts_stream_config; /* 3, 25, 10 */
typedef struct qasr_tts_chunk {
    int32_t stream, frame_index, n_frames, is_final;   /* AudioChunk: frameIndex, isFinal */
    const float* samples; size_t n_samples;            /* 1920 x n_frames, pool-owned, valid until the next step / close / destroy */
    const int32_t* codes;                              /* [16][n_frames] of this chunk, same lifetime */
} qasr_tts_chunk;
void qasr_tts_default_stream_config(int preset, qasr_tts_stream_config* out);   /* 0 default (3, 25, 10), 1 lowLatency (1, 15, 10) */
/* top_p < 1 -> QASR_ERR_UNSUPPORTED; a handle that already has a pool, a NULL argument -> QASR_ERR_INVALID (message: qasr_tts_last_error(t)) */
int qasr_tts_pool_create(qasr_tts* t, qasr_codec* codec, const qasr_tts_sampling* s, uint64_t seed, qasr_tts_pool** out);
/* queues one stream (rq->B == 1; the request is copied) for the next step and names it in *stream: the slot index, 0 .. max_batch - 1,
 * free again after the stream's final chunk or qasr_tts_pool_close.  first_chunk_frames < 1, chunk_frames < 1, decoder_left_context < 0,
 * B != 1 -> QASR_ERR_INVALID; first_chunk_frames > 35, decoder_left_context + chunk_frames > 35 -> QASR_ERR_UNSUPPORTED;
 * whatever qasr_tts_generate refuses -> its status; no free slot -> QASR_ERR_CAPACITY.  The pool stays usable. */
int qasr_tts_pool_open(qasr_tts_pool* p, const qasr_tts_request* rq, const qasr_tts_stream_config* sc, int32_t* stream);
/* admits the queued streams (one prompt pass each), runs frames for all live streams until a chunk is due -- never past the nearest
 * boundary of any stream, reading counts and finished flags every qasr_tts_poll_interval() frames -- and decodes every due chunk in one
 * codec call.  *n chunks are written (at most one per stream); *n == 0 only when no stream is live.  cap below the number of live
 * streams -> QASR_ERR_CAPACITY before anything runs. */
int qasr_tts_pool_step(qasr_tts_pool* p, qasr_tts_chunk* chunks, size_t cap, size_t* n);
/* ms[3]: host time of the last step: admission | frames, with the polls and the code reads | the codec call */
int qasr_tts_pool_timing(const qasr_tts_pool* p, float* ms);
int qasr_tts_pool_close(qasr_tts_pool* p, int32_t stream);                       /* cancel (TTSBridge.cancel): the slot is free at once */
int qasr_tts_pool_live(const qasr_tts_pool* p);                                 /* streams queued or running */
void qasr_tts_pool_destroy(qasr_tts_pool* p);
const char* qasr_tts_pool_last_error(const qasr_tts_pool* p);
/* pure CPU: the chunks a stream of n_frames frames is cut into; ended_by_eos = 0: it stopped at max_tokens (then n_frames >= 1).  Writes
 * frame_index / frames / is_final (any may be NULL) and returns the number of chunks, or -status (cap too small: -QASR_ERR_CAPACITY). */
int64_t qasr_tts_stream_chunks(int32_t n_frames, int ended_by_eos, const qasr_tts_stream_config* sc,
                               int32_t* frame_index, int32_t* frames, int32_t* is_final, size_t cap);

/* transducer greedy loops (pure CPU).  The caller owns the networks and their state:
 *   decoder_step(ctx, token)  advance the prediction network with `token` (the loops prime it with the blank id where the reference does)
 *   joint(ctx, frame, token_logits[vocab_size + 1], duration_logits[n_durations] or NULL)  logits for encoder frame `frame` and the
 *        current prediction-network output (the CoreML outputs are float16; pass them widened)
 * Both return 0 on success; any other value aborts the decode with QASR_ERR_INVALID. */
typedef struct qasr_transducer_config {
    int32_t vocab_size;                /* 8192 Parakeet-TDT | 1024 Nemotron | 1026 Parakeet-EOU (Configuration.swift of each target) */
    int32_t blank_id;                  /* = vocab_size */
    int32_t eou_id;                    /* 1024 for Parakeet-EOU, -1 otherwise */
    int32_t n_durations;               /* TDT: 5; RNNT: 0 */
    int32_t durations[8];              /* TDT: 0 1 2 3 4 */
    int32_t first_text_id;             /* TDT: 274 (ids below are fed to the network but not reported, TDTGreedyDecoder.swift:91-94) */
    int32_t max_symbols;               /* RNNT: 10 symbols per encoder frame (RNNTGreedyDecoder.swift:35) */
} qasr_transducer_config;
typedef struct qasr_transducer_callbacks {
    void* ctx;
    int (*decoder_step)(void* ctx, int32_t token);
    int (*joint)(void* ctx, int32_t frame, float* token_logits, float* duration_logits);
} qasr_transducer_callbacks;
/* model: "parakeet-tdt" | "nemotron-streaming" | "parakeet-eou" (or the reference's model ids containing those families' names) */
int qasr_transducer_default_config(const char* model, qasr_transducer_config* out);
/* TDTGreedyDecoder.decode (Sources/ParakeetASR/TDTGreedyDecoder.swift:45-143) -> number of tokens (<= cap) or -status.
 * log_probs / confidence may be NULL. */
int qasr_tdt_greedy_decode(const qasr_transducer_config* cfg, const qasr_transducer_callbacks* cb, int32_t encoded_length,
                           int32_t* tokens, float* log_probs, int32_t cap, float* confidence);
/* RNNTGreedyDecoder.decode (Sources/NemotronStreamingASR/RNNTGreedyDecoder.swift:38-90; with cfg->eou_id >= 0:
 * Sources/ParakeetStreamingASR/RNNTGreedyDecoder.swift:58-126).  The prediction network is NOT primed here: a session primes it once
 * (StreamingSession.swift:93-99) and its state persists across chunks. */
int qasr_rnnt_greedy_decode(const qasr_transducer_config* cfg, const qasr_transducer_callbacks* cb, int32_t encoded_length,
                            int32_t frame_offset, int32_t* tokens, float* log_probs, int32_t cap, int32_t* eou_detected);
float qasr_log_softmax_at(const float* logits, int32_t n, int32_t id);          /* TDTGreedyDecoder.logSoftmax (:149-172) */
float qasr_transducer_confidence(const float* log_probs, int32_t n);           /* min(1, exp(mean log-prob)), 0 when n == 0 */

/* SentencePiece-style vocabularies of these models (vocab.json: {"0": "\u2581the", ...}).  style 0: ParakeetVocabulary
 * (Sources/ParakeetASR/Vocabulary.swift:42-96); style 1: NemotronVocabulary = ParakeetEOUVocabulary
 * (Sources/NemotronStreamingASR/Vocabulary.swift:31-77).  Pure CPU. */
typedef struct qasr_sp_vocab qasr_sp_vocab;
int qasr_sp_vocab_create(const int32_t* ids, const char* const* pieces, size_t n, int style, qasr_sp_vocab** out);
int qasr_sp_vocab_load(const char* vocab_json_path, int style, qasr_sp_vocab** out);
void qasr_sp_vocab_destroy(qasr_sp_vocab* v);
int qasr_sp_vocab_count(const qasr_sp_vocab* v);
int qasr_sp_vocab_decode(const qasr_sp_vocab* v, const int32_t* ids, int32_t n, char* buf, size_t cap);        /* bytes written or -1 */
/* decodeWords: words '\n'-joined into buf, one confidence per word; returns the word count or -1 (buffer / conf_cap too small) */
int qasr_sp_vocab_decode_words(const qasr_sp_vocab* v, const int32_t* ids, int32_t n_ids, const float* log_probs, int32_t n_log_probs,
                               char* buf, size_t cap, float* confidences, int32_t conf_cap);

/* sample bookkeeping of a streaming session (StreamingSession.pushAudio / finalize, Sources/NemotronStreamingASR/StreamingSession.swift:
 * 110-139): whenever samples_per_chunk samples are buffered one chunk is cut and the buffer advances by `shift` samples
 * (Nemotron 160 ms: 17 x 160 = 2720 and 2 x 8 x 160 = 2560; Parakeet-EOU 320 ms: 33 x 160 = 5280 and 4 x 8 x 160 = 5120).  Pure CPU. */
typedef struct qasr_stream_chunker qasr_stream_chunker;
int qasr_stream_chunker_create(int32_t samples_per_chunk, int32_t shift, qasr_stream_chunker** out);
void qasr_stream_chunker_destroy(qasr_stream_chunker* c);
int qasr_stream_chunker_push(qasr_stream_chunker* c, const float* samples, size_t n);
int qasr_stream_chunker_pop(qasr_stream_chunker* c, float* chunk);       /* 1: chunk[samples_per_chunk] filled; 0: not enough samples */
int qasr_stream_chunker_flush(qasr_stream_chunker* c, float* chunk);     /* finalize: 1: the zero-padded remainder; 0: buffer was empty */
size_t qasr_stream_chunker_buffered(const qasr_stream_chunker* c);

/* ---- CosyVoice3 flow-matching mel decoder (csrc/flow_cosyvoice.hip, csrc/api_flow.cpp) --------------------------------------------------
 * Reference: Sources/CosyVoiceTTS/FlowMatching.swift, DiT.swift.  Speech tokens at 25 Hz (prompt tokens then new tokens), optionally a
 * prompt mel and a 192-d speaker vector -> an 80-bin mel at 50 Hz, the input of qasr_hift_decode.  What each entry replaces:
 *   CosyVoiceWeightLoader.loadFlow / loadDiT (WeightLoading.swift:126-212), local directory       -> qasr_flow_create
 *   inputEmbedding, PreLookaheadLayer, RepeatInterleaveUpsampler (FlowMatching.swift:204-227, :315-321, :23-33) -> qasr_flow_mu
 *   the L2 norm and spk_embed_affine_layer (FlowMatching.swift:332-336)                            -> qasr_flow_spks
 *   DiT.callAsFunction (DiT.swift:430-473) on one branch as given                                  -> qasr_flow_velocity
 *   ConditionalFlowMatching.forward (FlowMatching.swift:127-196) from a given x0                   -> qasr_flow_solve
 *   CosyVoiceFlowModel.callAsFunction (FlowMatching.swift:293-376)                                 -> qasr_flow_generate / _generate_batch
 * DiT: dim 1024, 16 heads x 64, ff 2048, any depth (22 as published); time embedding = sinusoid (half 128, angles 1000 t f, [sin | cos],
 * DiT.swift:22-32) -> Linear -> SiLU -> Linear; rows [x | cond | mu | spks] -> proj -> h + conv_pos_embed(h) (two grouped causal convs
 * k = 31 with Mish, DiT.swift:283-322); per block AdaLN chunks shift / scale / gate (attention) then shift / scale / gate (MLP)
 * (DiT.swift:88-101), RoPE on features 0 .. 63 of the 1024-wide q and k only, i.e. head 0 (DiT.swift:161-171), GELU-tanh; norm_out's
 * chunks are scale then shift (DiT.swift:121-125); proj_out is a float Linear.  Solver: t_i = 1 - cos(i / n pi / 2) in Float, both CFG
 * branches per step on the same x and t, v = (1 + 0.7) v_c - 0.7 v_u, x += (t_{i+1} - t_i) v (FlowMatching.swift:141-189).
 * Noise: x0 is this library's counter stream, not MLX's: element (frame t, bin m) of a clip = temperature * the `normal` of draw
 * 80 t + m of the clip's seed (qasr_hift_noise).
 * Precision: x, the residual stream, modulation, LayerNorm statistics and the solver are f32; GEMM operands are bf16, accumulation f32;
 * MLX 4 / 8 bit Linears are dequantised once at load, except the time MLP and the AdaLN linears, which stay packed (DESIGN.md section
 * 22).  A clip's result is bit-identical alone, in any batch and place, under any split into passes, and run to run.  One object, one
 * thread at a time.  Not covered: the LLM, CAM++, the speech tokenizer, FlowMelExtractor, chunked / streaming flow, float checkpoints. */
typedef struct qasr_flow qasr_flow;
/* model_dir/flow.safetensors with the reference's keys (WeightLoading.swift:126-212).  Depth = the number of
 * decoder.transformer_blocks.N present; bits (4 or 8) at group 64 from the weight / scales shapes; every other dimension is checked:
 * a missing file or key -> QASR_ERR_IO, a wrong shape or dtype or an unexpected key -> QASR_ERR_INVALID, the key named in
 * qasr_flow_last_error(NULL); all before any HIP call.  max_frames: mel frames (sum over clips) one device pass holds, 0 = 4096, at
 * most 2^15; about 33 KB of device memory per frame.  order_with: as for qasr_seg_create. */
int qasr_flow_create(int device, const char* model_dir, size_t max_frames, qasr_engine* order_with, qasr_flow** out);
void qasr_flow_destroy(qasr_flow* h);
const char* qasr_flow_last_error(const qasr_flow* h);               /* h may be NULL: last create() or check_clip failure */
int qasr_flow_is_loaded(const qasr_flow* h);
int qasr_flow_unload(qasr_flow* h);                                 /* later device calls return QASR_ERR_NOT_LOADED */
size_t qasr_flow_memory_footprint(const qasr_flow* h);              /* bytes as stored of the tensors read, 0 unloaded */
int qasr_flow_depth(const qasr_flow* h);
size_t qasr_flow_mel_frames(size_t n_tokens);                       /* 2 n (tokenMelRatio, Configuration.swift:74).  Pure CPU. */
/* t[n_steps + 1], the solver's time steps (FlowMatching.swift:141-144); n_steps in 1 .. 64.  Pure CPU. */
int qasr_flow_schedule(int n_steps, float* t);
/* what qasr_flow_generate checks of a clip before any device work: n >= 1, every id in [0, vocab) (refused, not clamped),
 * prompt_frames == 2 n_prompt and <= 2 (n + n_prompt) <= max_frames (0 = 4096).  Pure CPU. */
int qasr_flow_check_clip(const int32_t* tokens, size_t n, const int32_t* prompt_tokens, size_t n_prompt, size_t prompt_frames, int vocab,
                         size_t max_frames);
/* Stage entries; rows are frames: x, mu, cond, v, z, mel [T][80], spks [80]; spks and cond may be NULL (zeros, DiT.swift:357-362, :443-447) */
int qasr_flow_mu(qasr_flow* h, const int32_t* tokens, size_t n, float* mu /* [2 n][80] */);
int qasr_flow_spks(qasr_flow* h, const float* emb192 /* NULL: 80 zeros */, float* spks80);
int qasr_flow_velocity(qasr_flow* h, const float* x, const float* mu, const float* spks, const float* cond, size_t T, float t, float* v);
/* n_steps Euler steps from z (0 = 10, at most 64); v_out NULL or [2][T][80]: the last step's conditioned, then unconditioned velocity.
 * Bit-identical to a loop over qasr_flow_velocity (conditioned; then mu zero, spks and cond NULL) with the Euler line in f32. */
int qasr_flow_solve(qasr_flow* h, const float* mu, const float* spks, const float* cond, size_t T, const float* z, int n_steps, float* v_out,
                    float* mel);
/* The whole model.  prompt_tokens / prompt_feat [80][prompt_frames] / spk_emb [192] may be NULL; z_out NULL or, like mel,
 * [80][2 (n + n_prompt)] as the reference returns it (the caller slices off the first prompt_frames columns).  Bit-identical to
 * qasr_flow_solve on z_out with qasr_flow_mu / qasr_flow_spks and cond = the prompt mel followed by zeros. */
int qasr_flow_generate(qasr_flow* h, const int32_t* tokens, size_t n, const int32_t* prompt_tokens, size_t n_prompt, const float* prompt_feat,
                       size_t prompt_frames, const float* spk_emb, int n_steps, float temperature, uint64_t seed, float* z_out, float* mel);
/* B clips of any lengths in passes of at most max_frames frames cut at clip boundaries; one clip above max_frames -> QASR_ERR_INVALID.
 * The per-clip arrays prompt_tokens, n_prompt, prompt_feat, prompt_frames, spk_emb and z_out may be NULL, and so may their entries. */
int qasr_flow_generate_batch(qasr_flow* h, const int32_t* const* tokens, const size_t* n, const int32_t* const* prompt_tokens,
                             const size_t* n_prompt, const float* const* prompt_feat, const size_t* prompt_frames,
                             const float* const* spk_emb, int n_steps, float temperature, const uint64_t* seeds, size_t B,
                             float* const* z_out, float* const* mel);
/* ms[5]: device time of the solver passes of the last call, HIP events on the work stream: modulation table (0 when the cached table
 * of this n_steps was reused), input_embed, blocks, norm_out + proj_out, Euler */
int qasr_flow_timing(const qasr_flow* h, float* ms);

/* ---- CosyVoice3 speech-token LLM (csrc/llm_cosyvoice.hip, csrc/cvlm_sampler.cpp, csrc/api_cvlm.cpp) ------------------------------------
 * Reference: Sources/CosyVoiceTTS/LLM.swift, Configuration.swift:5-41,124-133, WeightLoading.swift:18-110, CosyVoiceTTS.swift:194-322.
 * Text ids (the caller's tokenizer; instruction + <|endofprompt|> + content) and optionally the prompt speech tokens of a reference clip
 * -> speech tokens at 25 Hz, which qasr_flow_generate turns into a mel and qasr_hift_decode into 24 kHz audio.  What each entry replaces:
 *   CosyVoiceWeightLoader.loadLLM (WeightLoading.swift:35-110), llm.safetensors of a local directory   -> qasr_cvlm_create
 *   CosyVoiceLLM.generate (LLM.swift:479-560) for B rows                                              -> qasr_cvlm_generate
 *   forwardStep on given tokens (:425-468)                                                            -> qasr_cvlm_forced
 *   sampleToken (:56-123)                                                                             -> qasr_cvlm_sample / _sample_host
 *   CosyVoiceTTSModel.synthesize behind the tokenizer (CosyVoiceTTS.swift:236-322)                     -> qasr_cvlm_synthesize
 * A Qwen2.5-0.5B shaped decoder (hidden 896, 24 layers, 14 heads over 2 kv heads, head_dim 64, no q/k norm, a Linear bias on q, k, v,
 * RoPE theta 1e6 split-half, SwiGLU 4864), float text and speech embeddings, a quantised speech head.  MLX affine 4 / 8 bit checkpoints
 * only.  The prefix of a row is [speech_emb(sos), text_emb(ids), speech_emb(task_id), speech_emb(prompt tokens)]; position prefix - 1
 * yields token 0; the stop set is speech_tokens + {0, 1, 2}; a stop token ends the row and is not stored.  Random numbers are the
 * library's counter stream keyed by (seed, row_index, step, draw), not MLX's.  Rows of a call are independent: a row's tokens and forced
 * logits are the same bits alone, in any batch, at any slot, under any max_batch and under either prompt chunking (tuning knob
 * cvlm_prompt_chunk: 64 | 1).  One object, one thread at a time.  HBM: the packed weights plus the KV cache, 2 x layers x kv_heads x 64
 * x 2 bytes = 12,288 bytes per position and row; positions = 2 + max_text + max_prompt_tokens + max_tokens rounded up to 64.
 * Not covered: the text tokenizer, CAM++, the speech tokenizer, float checkpoints, a streaming pool. */
typedef struct qasr_cvlm qasr_cvlm;
typedef struct qasr_cvlm_config {
    int32_t hidden, layers, heads, kv_heads, head_dim, inter;          /* 896 24 14 2 64 4864 */
    int32_t text_vocab, speech_tokens, speech_extra;                   /* 151936 6561 200: sos = 6561, eos = 6562, task_id = 6563 */
    float rms_eps, rope_theta;                                         /* 1e-6 1e6 */
    int32_t bits, group_size;                                          /* 4 | 8, 64 */
    int32_t device;
    int32_t max_batch;                                                 /* rows of one call, 1 .. 64 (default 8) */
    int32_t max_text, max_prompt_tokens, max_tokens;                   /* per row (defaults 512, 0, 1000) */
} qasr_cvlm_config;
typedef struct qasr_cvlm_sampling {         /* CosyVoiceSamplingConfig (Configuration.swift:124-133); maxTokenTextRatio is never read there: no field */
    int32_t top_k;                          /* 25; <= 0 or >= vocabulary: off */
    float top_p;                            /* 0.8; >= 1: off */
    int32_t win_size;                       /* 10; 0: no repetition-aware resample; at most 64 */
    float tau_r;                            /* 0.1 */
    float min_ratio;                        /* 2.0: min_len = Int(Float(content_len) * min_ratio) */
} qasr_cvlm_sampling;
typedef struct qasr_cvlm_request {
    size_t B;
    const int32_t* const* text; const int32_t* text_len;        /* [B]: at least 1 id */
    const int32_t* const* prompt; const int32_t* prompt_len;    /* [B] or NULL; NULL entry or 0: none; ids in [0, speech_tokens) */
    const int32_t* content_len;                                 /* [B] or NULL; < 0: the text length */
    const int32_t* max_tokens;                                  /* [B] or NULL; <= 0: the handle's */
    const int64_t* row_index;                                   /* [B] or NULL (0 .. B-1): keys the row's random stream */
} qasr_cvlm_request;
int qasr_cvlm_default_config(int bits, qasr_cvlm_config* out);
void qasr_cvlm_default_sampling(qasr_cvlm_sampling* out);
/* reads model_dir/llm.safetensors.  Every key, shape and dtype is checked on the host before any HIP call: a missing file or key ->
 * QASR_ERR_IO; a wrong shape or dtype, a float checkpoint, a key the reference does not name (layers.N.self_attn.q_norm / k_norm.weight,
 * which its loader names and never loads, are ignored) -> QASR_ERR_INVALID; so is a geometry the kernels do not serve: head_dim != 64,
 * hidden != heads x 64, heads % kv_heads != 0, heads / kv_heads > 16, hidden or inter not a multiple of 128, group_size != 64, a
 * vocabulary over 8192, inter over 10240 (4 bit) | 5120 (8 bit) -- there is no fallback kernel.  The key is named in
 * qasr_cvlm_last_error(NULL).  qasr_cvlm_check runs the host checks alone: no device is touched, no handle is made. */
int qasr_cvlm_create(const char* model_dir, const qasr_cvlm_config* cfg, qasr_cvlm** out);
int qasr_cvlm_check(const char* model_dir, const qasr_cvlm_config* cfg);
void qasr_cvlm_free(qasr_cvlm* h);
const char* qasr_cvlm_last_error(const qasr_cvlm* h);              /* h may be NULL: last create() / check() failure */
size_t qasr_cvlm_memory_footprint(const qasr_cvlm* h);             /* parameter bytes as stored */
size_t qasr_cvlm_device_bytes(const qasr_cvlm* h);                 /* every device allocation of the handle */
int qasr_cvlm_poll_interval(void);                                 /* steps between two host reads of the finished flags (8) */
int qasr_cvlm_context(const qasr_cvlm_config* cfg);                /* positions of a row's cache, or -status.  Pure CPU. */
/* the prefix of one row as the prompt pass reads it: a text id as it is, a speech id as -1 - id; out [2 + text_len + prompt_len].
 * Returns the prefix length or -status.  Pure CPU. */
int qasr_cvlm_plan_prefix(const qasr_cvlm_config* cfg, const int32_t* text, int32_t text_len, const int32_t* prompt, int32_t prompt_len,
                          int32_t* out);
/* tokens [B][max_tokens] int32 (the handle's max_tokens; entries past n_tokens[b] are -1), n_tokens [B].  B > max_batch, a text or prompt
 * or max_tokens over the handle's -> QASR_ERR_CAPACITY; an id outside its vocabulary (refused, not clamped), an empty text, a NULL buffer,
 * win_size over 64 -> QASR_ERR_INVALID.  Every refusal names the row. */
int qasr_cvlm_generate(qasr_cvlm* h, const qasr_cvlm_request* rq, const qasr_cvlm_sampling* s, uint64_t seed, int32_t* tokens, int32_t* n_tokens);
/* teacher-forced pass: tokens [B][T], T <= max_tokens, ids in [0, vocabulary) -> logits [B][T][V] f32 (V = speech_tokens + speech_extra),
 * hidden [B][T][hidden] (post-norm, bf16 values); logits[f] is read at position prefix - 1 + f after feeding tokens 0 .. f - 1.  Either
 * output may be NULL. */
int qasr_cvlm_forced(qasr_cvlm* h, const qasr_cvlm_request* rq, const int32_t* tokens, size_t T, float* logits, float* hidden);
/* the device sampler alone on the caller's logits [B][V]: history[b] [n_history[b]] (n_history <= max_tokens), step[b] keys the random
 * stream and step 0 masks the stops, below_min[b] != 0 masks them too; row_index NULL: 0 .. B-1.  out [B]. */
int qasr_cvlm_sample(qasr_cvlm* h, const float* logits, const int32_t* const* history, const int32_t* n_history, const int32_t* step,
                     const int32_t* below_min, size_t B, const qasr_cvlm_sampling* s, uint64_t seed, const int64_t* row_index, int32_t* out);
/* the host twin of the device sampler on one row.  cfg NULL: the default geometry.  Returns the token or -status.  Pure CPU. */
int qasr_cvlm_sample_host(const qasr_cvlm_config* cfg, const float* logits, const int32_t* history, int32_t n_history, int32_t step,
                          int below_min, const qasr_cvlm_sampling* s, uint64_t seed, int64_t row_index);
/* one linear of the loaded handle alone, as the step runs it: kind 0 q|k|v (input_layernorm prologue, bias; y [B][(heads + 2 kv) x 64]),
 * 1 o (y = resid + o(x), [B][hidden]), 2 gate|up (post_attention_layernorm prologue, SwiGLU; y [B][inter]), 3 down (y = resid + down(x)),
 * 4 head (final norm prologue; y [B][V] f32; layer ignored).  x [B][K], resid [B][N]: f32 holding bf16 values.  1 <= B <= 64. */
int qasr_cvlm_linear_probe(qasr_cvlm* h, int32_t layer, int32_t kind, const float* x, const float* resid, size_t B, float* y);
/* generate, then per row qasr_flow_generate_batch (the row's prompt tokens, prompt_feat[b] [80][prompt_frames[b]] and spk_emb[b] [192],
 * any NULL; 10 steps, temperature 1, flow and vocoder seed = seed + row_index[b]) and qasr_hift_decode_batch on the full mel; the first
 * 480 x prompt_frames[b] samples are dropped afterwards (CosyVoiceTTS.swift:276-322).  pcm[b] holds qasr_hift_num_samples(2 x max_tokens)
 * floats, n_samples[b] of them are written; a row with no tokens returns 0 samples.  tokens / n_tokens as qasr_cvlm_generate, may be NULL. */
int qasr_cvlm_synthesize(qasr_cvlm* h, qasr_flow* flow, qasr_hift* hift, const qasr_cvlm_request* rq, const qasr_cvlm_sampling* s,
                         uint64_t seed, const float* const* spk_emb, const float* const* prompt_feat, const size_t* prompt_frames,
                         float* const* pcm, size_t* n_samples, int32_t* tokens, int32_t* n_tokens);

/* ---- CosyVoice3 speech tokenizer and voice profiles (csrc/s3tok_cosyvoice.hip, csrc/api_s3tok.cpp) ---------------------------------------
 * Reference: Sources/CosyVoiceTTS/SpeechTokenizer.swift, WhisperMelExtractor.swift, FlowMelExtractor.swift, VoiceCloning.swift:69-158,
 * :329-345, WeightLoading.swift:350-398.  A reference clip -> the prompt speech tokens (25 Hz, [0, 6561)) and the prompt mel ([80][frames],
 * 50 Hz) that qasr_cvlm_synthesize / qasr_flow_generate take for zero-shot cloning.  The CAM++ speaker vector stays a caller input.
 * What each entry replaces:
 *   CosyVoiceWeightLoader.loadSpeechTokenizer (WeightLoading.swift:350-398), speech_tokenizer.safetensors -> qasr_s3tok_create
 *   resample (VoiceCloning.swift:329-345)                                                                -> qasr_s3tok_resample
 *   WhisperMelExtractor.extract (WhisperMelExtractor.swift:132-225)                                      -> qasr_s3tok_whisper_mel
 *   FlowMelExtractor.extract (FlowMelExtractor.swift:142-229)                                            -> qasr_s3tok_flow_mel
 *   AudioEncoderV3.callAsFunction (SpeechTokenizer.swift:279-288)                                        -> qasr_s3tok_hidden
 *   FSQCodebook.encode up to project_down (:77), and from tanh on (:78-93)                              -> qasr_s3tok_project, qasr_s3tok_fsq_host
 *   SpeechTokenizerModel.encode on the Whisper mel of a clip (:312-315)                                  -> qasr_s3tok_encode / _encode_batch
 *   extractVoiceProfile (VoiceCloning.swift:69-158) without camppSpeaker                                 -> qasr_s3tok_profile / _profile_batch
 * One deviation: the reference hands tokens and prompt mel over with whatever lengths they have; qasr_flow_generate takes a prompt mel of
 * exactly 2 frames per prompt token, so the profile entries cut both to L = min(tokens, frames / 2) as upstream CosyVoice's zero-shot front
 * end does, and report the uncut lengths.  The stage entries return uncut results.  A clip gives the same bits alone, at any place of a
 * batch and under any max_tokens.  One handle, one thread at a time. */
typedef struct qasr_s3tok qasr_s3tok;
/* model_dir holds speech_tokenizer.safetensors (F32 / F16 / BF16).  A missing file or key is QASR_ERR_IO; a wrong shape or dtype, an unknown
 * key (a bias on `key` is one) or an argument out of range is QASR_ERR_INVALID, the message names the key: qasr_s3tok_last_error(NULL);
 * all before any HIP call.  max_tokens: hidden rows (tokens, summed over clips) one device pass holds, 0 = 768 (30 s), at most 2^14. */
int qasr_s3tok_create(int device, const char* model_dir, size_t max_tokens, qasr_engine* order_with, qasr_s3tok** out);
void qasr_s3tok_destroy(qasr_s3tok* h);
const char* qasr_s3tok_last_error(const qasr_s3tok* h);             /* h may be NULL: last create() failure */
int qasr_s3tok_is_loaded(const qasr_s3tok* h);
int qasr_s3tok_unload(qasr_s3tok* h);                               /* later device calls return QASR_ERR_NOT_LOADED */
size_t qasr_s3tok_memory_footprint(const qasr_s3tok* h);            /* bytes as stored of the tensors read, 0 unloaded */
int qasr_s3tok_depth(const qasr_s3tok* h);
size_t qasr_s3tok_max_tokens(const qasr_s3tok* h);
/* Pure CPU.  Whisper mel frames of n samples at 16 kHz: n / 160 (the last frame is dropped); tokens of T mel frames: two k 3, stride 2,
 * pad 1 convs; flow mel frames of n samples at 24 kHz: n / 480 for n >= 480, else 0; the resampler's output length floor(n dst / src);
 * the profile's common length min(tokens, frames / 2). */
size_t qasr_s3tok_whisper_frames(size_t n_samples_16k);
size_t qasr_s3tok_tokens(size_t mel_frames);
size_t qasr_s3tok_flow_frames(size_t n_samples_24k);
size_t qasr_s3tok_resampled_length(size_t n, int src_rate, int dst_rate);
size_t qasr_s3tok_profile_cut(size_t n_tokens, size_t frames);
/* The reference's linear resampler on the host, bit for bit; out holds qasr_s3tok_resampled_length values. */
int qasr_s3tok_resample(const float* x, size_t n, int src_rate, int dst_rate, float* out);
/* projections [rows][8] -> codes: tanh, x Float(0.999), round half to even, + 1, sum digit[k] 3^k.  Pure CPU, the twin of the device's lines. */
int qasr_s3tok_fsq_host(const float* proj, size_t rows, int32_t* codes);
int qasr_s3tok_whisper_mel(qasr_s3tok* h, const float* pcm16k, size_t n, float* mel /* [128][n / 160] */);
int qasr_s3tok_flow_mel(qasr_s3tok* h, const float* pcm24k, size_t n, float* mel /* [80][n / 480] */);
int qasr_s3tok_hidden(qasr_s3tok* h, const float* mel /* [128][T] */, size_t T, float* hidden /* [tokens][1280], after the last block */);
int qasr_s3tok_project(qasr_s3tok* h, const float* mel /* [128][T] */, size_t T, float* proj /* [tokens][8], before tanh */);
int qasr_s3tok_encode(qasr_s3tok* h, const float* pcm16k, size_t n, int32_t* codes /* [tokens of n / 160 frames] */);
/* ragged clips packed back to back, in passes of at most max_tokens rows; a clip alone over max_tokens is refused */
int qasr_s3tok_encode_batch(qasr_s3tok* h, const float* const* pcm16k, const size_t* n, size_t B, int32_t* const* codes);
/* tokens holds the uncut token count, prompt_feat 80 x the uncut frame count (both from the length functions on the resampled lengths);
 * written: tokens[0 .. L), prompt_feat as [80][2 L].  n_tokens = L, prompt_frames = 2 L; uncut_* may be NULL.  L = 0 is QASR_ERR_INVALID. */
int qasr_s3tok_profile(qasr_s3tok* h, const float* pcm, size_t n, int sample_rate, int32_t* tokens, size_t* n_tokens, float* prompt_feat,
                       size_t* prompt_frames, size_t* uncut_tokens, size_t* uncut_frames);
int qasr_s3tok_profile_batch(qasr_s3tok* h, const float* const* pcm, const size_t* n, const int* sample_rate, size_t B, int32_t* const* tokens,
                             size_t* n_tokens, float* const* prompt_feat, size_t* prompt_frames, size_t* uncut_tokens, size_t* uncut_frames);
/* ms[4] of the last encode / hidden / project / profile call, summed over passes: mel, stems, blocks, FSQ */
int qasr_s3tok_timing(const qasr_s3tok* h, float* ms);

/* ---- VoxCPM2 local networks: LocEnc and the LocDiT patch decoder (csrc/loc_voxcpm.hip, csrc/api_vloc.cpp) ------------------------------
 * Reference: Sources/VoxCPM2TTS/MiniCPM4.swift, Configuration.swift:3-136, VoxCPM2TTS.swift:81-124, :377-449.  A patch is P latent frames
 * [P][feat_dim], the layout qasr_avae_* reads and writes.  What each entry replaces:
 *   the feat_encoder / feat_decoder / *_proj part of loadWeights (VoxCPM2TTS.swift:383-440)              -> qasr_vloc_create, qasr_vloc_check
 *   makeUnifiedCFMTimeSpan (MiniCPM4.swift:152-166), zeroInitSteps (:687)                                -> qasr_vloc_schedule, _zero_steps
 *   MiniCPMLongRoPE.init + callAsFunction (:43-89)                                                       -> qasr_vloc_rope_table
 *   enc_to_lm_proj(feat_encoder(feat)) (:480-539, VoxCPM2TTS.swift:1312, :1388)                          -> qasr_vloc_encode
 *   lm_to_dit_proj(lm hidden) || res_to_dit_proj(residual hidden) (VoxCPM2TTS.swift:1368-1371)           -> qasr_vloc_mu
 *   VoxCPMLocDiTV2.callAsFunction with dt = 0 (:611-651)                                                 -> qasr_vloc_velocity
 *   UnifiedCFM.solveEuler with CFG-zero-star (:674-727)                                                  -> qasr_vloc_solve
 *   UnifiedCFM.sample (:729-745)                                                                         -> qasr_vloc_sample
 *   MiniCPMModel.callAsFunction(inputsEmbeds:, isCausal: false) (:430-475)                               -> qasr_vloc_stack
 * Deviations: MLXRandom is not reproduced, qasr_vloc_sample draws from the project's counter stream (see below); mean_mode true and a head
 * width other than 128 are refused at create.  4-bit / 8-bit MLX checkpoints are dequantised to bf16 once at load.  A sequence gives the same bits alone, at any place of a
 * batch and in a second run (as long as both launches lie on the same side of the tuning knob vloc_skinny_rows).  One handle, one thread at a time. */
typedef struct qasr_vloc qasr_vloc;
typedef struct qasr_vloc_geometry {
    int32_t patch_size, feat_dim, lm_hidden, enc_hidden, dit_hidden, enc_layers, dit_layers, mu_dim, kv_heads;
    size_t stored_bytes;
} qasr_vloc_geometry;
/* config.json and every tensor the handle reads, checked on the host alone (no HIP call): what qasr_vloc_create does first.  g may be NULL. */
int qasr_vloc_check(const char* model_dir, qasr_vloc_geometry* g);
/* model_dir holds config.json (optional, every key optional: the reference's defaults) and *.safetensors (F32 / F16 / BF16, or MLX 4-bit / 8-bit
 * triplets weight U32 / scales / biases in groups of 64 for any Linear) with feat_encoder.*, feat_decoder.estimator.*, enc_to_lm_proj.*, lm_to_dit_proj.*, res_to_dit_proj.*.  A missing file or tensor is QASR_ERR_IO;
 * a wrong shape or dtype, or a configuration value the kernels do not serve, is QASR_ERR_INVALID with the field named:
 * qasr_vloc_last_error(NULL); all before any HIP call.  max_seqs: patches one device pass holds, 0 = 32, at most 1024. */
int qasr_vloc_create(int device, const char* model_dir, size_t max_seqs, qasr_engine* order_with, qasr_vloc** out);
void qasr_vloc_destroy(qasr_vloc* h);
const char* qasr_vloc_last_error(const qasr_vloc* h);               /* h may be NULL: last create() / check() failure */
int qasr_vloc_is_loaded(const qasr_vloc* h);
int qasr_vloc_unload(qasr_vloc* h);                                 /* later device calls return QASR_ERR_NOT_LOADED */
size_t qasr_vloc_memory_footprint(const qasr_vloc* h);              /* bytes as stored of the tensors read, 0 unloaded */
int qasr_vloc_patch_size(const qasr_vloc* h);
int qasr_vloc_feat_dim(const qasr_vloc* h);
int qasr_vloc_lm_hidden(const qasr_vloc* h);
int qasr_vloc_mu_dim(const qasr_vloc* h);                           /* mu tokens x the LocDiT's width */
int qasr_vloc_hidden(const qasr_vloc* h, int which);                /* which: 0 LocEnc, 1 LocDiT */
int qasr_vloc_depth(const qasr_vloc* h, int which);
size_t qasr_vloc_max_seqs(const qasr_vloc* h);
/* Pure CPU.  t[0 .. n_steps]: u + (cos(pi / 2 u) - 1 + u), u = 1 - i / n, in double, rounded to float; n_steps in 1..64. */
int qasr_vloc_schedule(int n_steps, float* t);
int qasr_vloc_zero_steps(int n_steps);                              /* max(1, Int((n + 1) 0.04)) leading steps with a zero derivative */
/* Pure CPU.  The LongRoPE tables of model_dir's config.json for a head of head_dim values, positions 0 .. n_pos - 1: cos, sin
 * [n_pos][head_dim], formed in double.  The attention scaling reads LMConfig.originalMaxPositionEmbeddings, which has no coding key and
 * is therefore 32768 whatever rope_scaling says. */
int qasr_vloc_rope_table(const char* model_dir, int head_dim, int n_pos, float* cos, float* sin);
/* feats [n][P][feat_dim] -> cls [n][enc hidden] (token 0 after the final norm) and / or embed [n][lm_hidden]; one of them may be NULL.
 * n over max_seqs runs in passes with identical results. */
int qasr_vloc_encode(qasr_vloc* h, const float* feats, size_t n, float* cls, float* embed);
/* B over max_seqs is QASR_ERR_CAPACITY in the four entries below. */
int qasr_vloc_mu(qasr_vloc* h, const float* lm_hidden /* [B][lm_hidden] */, const float* res_hidden, size_t B, float* mu /* [B][mu_dim] */);
/* one estimator call, mu as given: x, cond, v [B][P][feat_dim] */
int qasr_vloc_velocity(qasr_vloc* h, const float* x, const float* mu, const float* cond, size_t B, float t, float* v);
/* the Euler solve from the caller's noise z [B][P][feat_dim]: x_out the patch, v_out (may be NULL) the last step's guided derivative.
 * The first solve of a (B, n_steps) runs its launches one by one, the second captures them into one graph, later ones replay it; at most
 * 16 such graphs are kept, one more pair drops them all. */
int qasr_vloc_solve(qasr_vloc* h, const float* mu, const float* cond, const float* z, size_t B, int n_steps, float cfg, float* x_out, float* v_out);
/* qasr_vloc_solve from z[b][i] = temperature x the normal of draw row_index[b] P feat_dim + i of the counter stream `seed`
 * (csrc/voc_cosyvoice.h: the stream of qasr_flow_generate); row_index NULL: b.  z_out (may be NULL) receives z. */
int qasr_vloc_sample(qasr_vloc* h, const float* mu, const float* cond, size_t B, int n_steps, float cfg, float temperature, uint64_t seed,
                     const uint64_t* row_index, float* z_out, float* x_out);
/* stage entry: the first n_layers layers of a stack on embeddings x [n_seq][S][hidden], S in 1..32, n_seq up to 2 max_seqs; n_layers =
 * depth adds the final norm */
int qasr_vloc_stack(qasr_vloc* h, int which, const float* x, size_t n_seq, int S, int n_layers, float* out);
/* ms[4] of the last encode (summed over passes) | mu | velocity or stack | solve, copies included */
int qasr_vloc_timing(const qasr_vloc* h, float* ms);

#ifdef __cplusplus
}
#endif
#endif /* QASR_H */
