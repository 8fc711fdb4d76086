// tts_talker.h -- the Qwen3-TTS Talker and code predictor on the device (kernels and host object in tts_talker.hip, host sampler twin in
// tts_sampler.cpp, C ABI in api_tts.cpp): text ids + language (+ speaker token | x-vector, + instruct ids) -> 16 code streams at 12.5 Hz.
//
// Reference: Sources/Qwen3TTS/Talker.swift, CodePredictor.swift, Sampling.swift, Qwen3TTS.swift (buildCodecPrefix, buildPrefillEmbeddings,
// generateWithCodePredictor, predictCodebooksForTimestep), TTSWeightLoading.swift:24-158 (keys).  MLX affine 4 / 8 bit Linears stay packed
// (dec_quant.h); bf16 activations between layers, f32 accumulation, f32 norms / softmax / logits.  Nothing here is shared with the Engine
// class: the layer GEMVs and the Talker's attention are the decode step's launch functions (decode_gemv_q_launch,
// decode_attention_launch), and for ICL prompts the engine's prompt-pass launch functions (quant_dequant_multi_launch, gemm_nt*,
// qk_norm_rope_launch, prefill_attention_launch).  Shared with the CosyVoice3 LLM (llm_cosyvoice.h): the checked
// weight loader and its arena (qlm_weights.h), the per-batch-size graph cache (StepGraphs, engine.h), the RoPE tables (rope_tables_host)
// and the samplers' two reduction helpers (sample_dev.h); every other kernel of the frame is in tts_talker.hip.  DESIGN.md section 18.
#pragma once
#include "engine.h"
#include "qlm_weights.h"
#include "qasr.h"
#include <memory>
#include <string>
#include <vector>

namespace qasr {

constexpr int TTS_GROUPS = 16;          // code streams of a frame: code 0 from the Talker, 1 .. 15 from the code predictor
constexpr int TTS_MAX_FRAMES = 500;     // the reference's safeMaxTokens (Qwen3TTS.swift:1407)
constexpr int TTS_POLL = 8;             // frames between two host reads of the finished flags
constexpr int TTS_MAX_VOCAB = 4096;     // logits of one sampler workgroup (LDS image)
constexpr int TTS_TEMPLATE = 9;         // <|im_start|>assistant\n ... <|im_end|>\n<|im_start|>assistant\n
constexpr int TTS_ICL_FIXED = 11;       // positions of an ICL prompt beside its texts and frames: role 3, codec prefix 6, tts_eos, codec_bos
constexpr int TTS_MAX_CTX = 32768;      // positions of a row: the Talker's max_position_embeddings (Configuration.swift), which is also what
                                        // the prompt kernels were checked for (32-bit byte offsets inside one V^T row block: 128 x stride x 2)

// ---- the sampler, stated once for the device kernel and the host twin (tts_sampler.cpp) ------------------------------------------
struct TtsSampleParams {
    float temperature, repetition_penalty, eos_logit_bias;
    int top_k;
    int suppress_lo, suppress_hi, eos;   // Talker mode only (eos < 0: code-predictor mode, steps 1, 2, 5, 7 are skipped)
    unsigned long long seed;
};
// the random stream: counter-based splitmix64; the counter depends on (seed, caller row, frame, group, vocabulary index) only
__host__ __device__ inline unsigned long long tts_splitmix64(unsigned long long z) {
    z += 0x9e3779b97f4a7c15ull;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
__host__ __device__ inline unsigned long long tts_stream_key(unsigned long long seed, long long row, int frame, int group) {
    const unsigned long long a = tts_splitmix64(seed ^ 0x5174735454533031ull);
    const unsigned long long b = tts_splitmix64(a + (unsigned long long)row);
    return tts_splitmix64(b + (((unsigned long long)(unsigned)frame) << 8) + (unsigned long long)group);
}
// u in [1e-6, 1] as dec_sampler.hip draws it
__host__ __device__ inline float tts_uniform(unsigned long long key, int i) {
    const double r = (double)(tts_splitmix64(key + (unsigned long long)i) >> 11) * (1.0 / 9007199254740992.0);
    return (float)(1e-6 + r * (1.0 - 1e-6));
}
// sampleToken / sampleTokenLazy (Sampling.swift:36-160) on one row of f32 logits; `seen` [V] marks the row's distinct code-0 history (may be
// null); returns the token.  Pure host code.
int tts_sample_host(const float* logits, int V, const TtsSampleParams& p, const unsigned char* seen, long long row, int frame, int group);

// The launch entry of the code predictor's attention (kernel in tts_talker.hip; head_dim 128): position pos (0 .. 15) of the frame for B
// rows of qkv [B][(heads + 2 kv_heads) * 128].  q/k RMSNorm (qn / kn [128]) + RoPE (row pos of cos_t / sin_t [16][64]); k and v go to entry
// pos of the caches [B][kv_heads][16][128], the row attends entries 0 .. pos -> out [B][heads * 128].  std::invalid_argument for a pos
// outside 0 .. 15 or heads no multiple of kv_heads.
void tts_cp_attn_launch(const bf16_t* qkv, int pos, int B, int heads, int kv_heads, const bf16_t* qn, const bf16_t* kn, float eps,
                        const float* cos_t, const float* sin_t, bf16_t* kc, bf16_t* vc, bf16_t* out, hipStream_t s);

struct TtsRow {                         // one row of a request, checked by the C ABI
    const int32_t* text; int n_text;
    int language, speaker;              // speaker < 0: none
    const float* xvector;               // [hidden] or null
    const int32_t* instruct; int n_instruct;
    long long index;                    // the caller's row index (random stream)
    // ICL voice cloning (Qwen3TTS+ICL.swift): the reference clip's transcript ids and its codes [16][ref_frames]; ref_codes null: a plain row
    const int32_t* ref_text = nullptr; int n_ref_text = 0;
    const int32_t* ref_codes = nullptr; int ref_frames = 0;
};

struct TtsForcedOut {                   // qasr_tts_forced: any pointer may be null
    const int32_t* codes; int T;        // [B][16][T]
    float* talker_logits;               // [B][T][codec_vocab]
    float* cp_logits;                   // [B][T][15][cp_vocab]
    float* hidden;                      // [B][T][hidden]
};

class TtsTalker {
  public:
    // every key, shape and dtype is checked on the host before any HIP call (WeightLoadError); `cfg` is complete (api_tts.cpp)
    // max_ref_frames > 0: an ICL handle (context, prompt buffers and the packed prompt pass's scratch sized for reference clips)
    TtsTalker(const qasr_tts_config& cfg, const SafeTensorsDir& st, int max_ref_frames = 0, int max_ref_text = 0);
    ~TtsTalker();
    const qasr_tts_config& config() const { return cfg_; }
    size_t footprint() const { return wl_->param_bytes(); }
    size_t device_bytes() const { return wl_->device_bytes(); }
    // codes [B][16][max_frames] (row stride 16 * max_frames), n_frames [B]
    void generate(const std::vector<TtsRow>& rows, const qasr_tts_sampling& s, unsigned long long seed, int max_frames, int32_t* codes,
                  int32_t* n_frames);
    void forced(const std::vector<TtsRow>& rows, const TtsForcedOut& f);
    // the prompt rows of an ICL call as the Talker would read them: rows [B][P_max][hidden] (bf16 values widened, zeros past a row's P), P [B]
    void icl_prompt(const std::vector<TtsRow>& rows, float* out, int32_t* P);
    int max_ref_frames() const { return max_ref_frames_; }
    int max_ref_text() const { return max_ref_text_; }
    static void check_geometry(const qasr_tts_config& c);      // std::invalid_argument for what the kernels do not serve
    static int icl_context(const qasr_tts_config& c, int max_ref_frames, int max_ref_text);   // positions of an ICL handle; throws over TTS_MAX_CTX
    // ---- the stream pool's view (api_tts.cpp, qasr_tts_pool_*): a batch row is a slot that a stream joins and
    // leaves at any frame.  Everything a row owns is per slot; a free slot carries finished = 1, is computed and writes nothing.
    void pool_begin(const qasr_tts_sampling& s, unsigned long long seed);     // the pool's Knobs, every slot free, table rows 0 1 2
    void pool_admit(int slot, const TtsRow& r);                                // the slot's state and its prompt but the last position
    void pool_frames(int B, int n);                                            // n frames of slots 0 .. B - 1, no host read
    void pool_poll(int B, int* n_frames, int* finished);                       // [B] each, synchronises
    void pool_finish(int slot);                                                // finished = 1 (max_tokens reached, close)
    void pool_codes(int slot, int f0, int n, int32_t* out);                    // frames f0 .. f0 + n - 1 of the slot -> out [16][n]
    struct Knobs;                        // device-side per-call values (tts_talker.hip)

  private:
    struct Layer : QlmLayer { const bf16_t *qn = nullptr, *kn = nullptr; };
    struct Net { std::vector<Layer> layers; const bf16_t* norm = nullptr; int H, heads, kv, hd, I; float eps; };
    void load_net(const SafeTensorsDir& st, QlmLoader& wl, const std::string& prefix, Net& n, int layers);
    void load_all(const SafeTensorsDir& st, QlmLoader& wl);
    void prefill(const std::vector<TtsRow>& rows, bool build_only = false);
    int plan_row(const TtsRow& r, std::vector<int>& tp_ids, int tp_row0, int* pt, int* pc, int* tr, int& nt, float* xv, int* ref) const;
    void packed_prompt(int B, int Pmax);
    void layer_steps(const Net& n, bf16_t* x, int B, bool talker, int cp_pos, bool kv_only_last, int row0 = 0);
    void issue_frame(int B, bool forced_mode);
    void run_frame(int B);
    void set_knobs(const qasr_tts_sampling& s, unsigned long long seed);

    qasr_tts_config cfg_;
    hipStream_t stream_ = nullptr;
    std::unique_ptr<QlmLoader> wl_;      // the weights' and workspaces' arena
    Net tk_, cp_;
    QLin head_, fc1_, fc2_, proj_, lm_[TTS_GROUPS - 1];
    const bf16_t *codec_emb_ = nullptr, *text_emb_ = nullptr, *cp_emb_[TTS_GROUPS - 1] = {};
    const bf16_t** d_cp_emb_ = nullptr;
    int max_ctx_ = 0, max_prefill_ = 0, max_tp_ = 0;
    int max_ref_frames_ = 0, max_ref_text_ = 0;
    // ICL handles: the reference codes of a call, and the packed prompt pass's scratch (one layer of bf16 weights, activations of every
    // packed position, the V^T image, the per-position slot / position and per-row offsets)
    int* d_ref_codes_ = nullptr;
    int max_pos_ = 0, vt_stride_ = 0;
    bf16_t *d_w_ = nullptr, *d_vt_ = nullptr, *d_px_ = nullptr, *d_ph_ = nullptr, *d_pqkv_ = nullptr, *d_pqr_ = nullptr, *d_pattn_ = nullptr,
           *d_pact_ = nullptr;
    int* d_pmeta_ = nullptr;
    std::vector<int> pf_len_;                                  // prompt length of every row of the last prefill
    float *d_rope_cos_ = nullptr, *d_rope_sin_ = nullptr, *d_cp_cos_ = nullptr, *d_cp_sin_ = nullptr, *d_rope_rows_ = nullptr;
    bf16_t *d_k_ = nullptr, *d_vf_ = nullptr, *d_cpk_ = nullptr, *d_cpv_ = nullptr;
    bf16_t *d_x_ = nullptr, *d_hn_ = nullptr, *d_qkv_ = nullptr, *d_attn_ = nullptr, *d_act_ = nullptr, *d_scratch_ = nullptr;
    bf16_t *d_cpa_ = nullptr, *d_cpb_ = nullptr, *d_cx_ = nullptr, *d_chn_ = nullptr;
    bf16_t *d_tp_in_ = nullptr, *d_tp_mid_ = nullptr, *d_tp_ = nullptr, *d_pf_ = nullptr;
    float *d_logits_ = nullptr, *d_cp_logits_ = nullptr, *d_xvec_ = nullptr;
    int *d_state_ = nullptr, *d_codes_ = nullptr, *d_tp_ids_ = nullptr, *d_pf_text_ = nullptr, *d_pf_codec_ = nullptr, *d_trail_ = nullptr;
    long long* d_row_index_ = nullptr;
    unsigned char* d_seen_ = nullptr;
    Knobs* d_knobs_ = nullptr;
    float *d_f_tlog_ = nullptr, *d_f_cplog_ = nullptr, *d_f_hid_ = nullptr;    // forced-pass outputs (sized per call)
    int* d_f_codes_ = nullptr;
    int forced_T_host_ = 0;
    std::unique_ptr<DevBuf> forced_buf_[4];
    StepGraphs graphs_;                                        // the frame's launch sequence per batch size
};

}  // namespace qasr
