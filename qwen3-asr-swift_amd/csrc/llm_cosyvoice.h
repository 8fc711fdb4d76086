// llm_cosyvoice.h -- the CosyVoice3 speech-token LLM on the device (kernels and host object in llm_cosyvoice.hip, host sampler twin in
// cvlm_sampler.cpp, C ABI in api_cvlm.cpp): text ids (+ prompt speech tokens) -> speech tokens at 25 Hz, the input of qasr_flow_*.
//
// Reference: Sources/CosyVoiceTTS/LLM.swift (sampleToken :12-123, CosyVoiceAttention :131-216, CosyVoiceBlock :219-262, buildInputSequence
// :387-417, generate :479-560), Configuration.swift:5-41,124-133, WeightLoading.swift:18-110 (keys of llm.safetensors).  A Qwen2.5-0.5B
// shaped decoder: head_dim 64, no q/k norm, a Linear bias on q, k and v, separate text and speech embeddings, a quantised speech head.
// MLX affine 4 / 8 bit Linears stay packed (the images of dec_quant.h); bf16 activations between ops, f32 accumulation, f32 norms,
// softmax and logits.  Every kernel of the step is in llm_cosyvoice.hip.  Shared with the Talker (tts_talker.h): the checked weight
// loader and its arena (qlm_weights.h, which builds the images with quant_pack_launch), the per-batch-size graph cache (StepGraphs,
// engine.h), the RoPE tables (rope_tables_host), the counter random stream of tts_talker.h and the samplers' two reduction helpers
// (sample_dev.h).  DESIGN.md section 23.
#pragma once
#include "qlm_weights.h"
#include "tts_talker.h"      // tts_stream_key, tts_uniform
#include "qasr.h"
#include <memory>
#include <string>
#include <vector>

namespace qasr {

constexpr int CVLM_POLL = 8;             // steps between two host reads of the finished flags
constexpr int CVLM_MAX_VOCAB = 8192;     // logits of one sampler workgroup (four LDS arrays of this many words)
constexpr int CVLM_MAX_WIN = 64;         // history window of the repetition-aware resample (LDS)
constexpr int CVLM_ATT_CHUNK = 64;       // keys of one wave in one round of the attention sweep
constexpr int CVLM_ATT_ROUND = 256;      // keys of one round (4 waves): the online-softmax merge happens once per round, in key order
constexpr int CVLM_PASS_ROWS = 64;       // rows of one launch sequence: batch rows of a step, packed (slot, position) pairs of a prompt pass
constexpr int CVLM_MAX_CTX = 32768;      // positions of a row
constexpr int CVLM_GEMV_PHASE = 1024;    // activation columns of the GEMV's LDS image
constexpr int CVLM_GEMV_MAXB = 10;       // k-blocks one wave may own: K <= 8 * 10 * 128 (4 bit) | 8 * 10 * 64 (8 bit)
constexpr int CVLM_STOPS = 3;            // speech_tokens + 0 .. 2 end a row (Configuration.swift:33-35)

// ---- the sampler, stated once for the device kernel and the host twin (cvlm_sampler.cpp) ------------------------------------------
struct CvlmSampleParams {
    int top_k; float top_p; int win_size; float tau_r;
    int V, speech_tokens;                // suppress [speech_tokens, V) except the stops speech_tokens + 0 .. 2
    unsigned long long seed;
};
// repetitions of the pick in the window that trigger the resample (LLM.swift:106-108)
__host__ __device__ inline int cvlm_ras_threshold(int win_size, float tau_r) {
    const int t = (int)((float)win_size * tau_r);
    return t > 1 ? t : 1;
}
// sampleToken on one row of f32 logits; history [n_history] are the row's tokens so far, step keys the random stream, mask_stops is
// "below min_len or token 0".  Pure host code.
int cvlm_sample_host(const float* logits, const CvlmSampleParams& p, const int32_t* history, int n_history, int step, bool mask_stops,
                     long long row);

struct CvlmRow {                         // one row of a request, checked by the C ABI
    const int32_t* text; int n_text;
    const int32_t* prompt; int n_prompt; // prompt speech tokens, may be null / 0
    int content_len;                     // ids of `text` that are content (min_len = Int(Float(content_len) * min_ratio))
    int max_tokens;                      // 1 .. the handle's
    long long index;                     // the caller's row index (random stream)
};

// The launch entries of the attention path (kernels in llm_cosyvoice.hip; head_dim 64).  Row r sits at (slot[r], pos[r]), device arrays.
// append: split-half RoPE at pos[r] on the q and k thirds of qkv [rows][(heads + 2 kv_heads) * 64] (cos_t / sin_t [positions][32]),
// q -> qr [rows][heads * 64], k and v -> row pos[r] of the caches [slots][kv_heads][max_ctx][64].  attention: row r over keys 0 .. pos[r] of
// its slot -> out [rows][heads * 64]; std::invalid_argument unless heads / kv_heads is integral and at most 16.
void cvlm_rope_append_launch(const bf16_t* qkv, const int* slot, const int* pos, int rows, int heads, int kv_heads, const float* cos_t,
                             const float* sin_t, bf16_t* qr, bf16_t* kc, bf16_t* vc, int max_ctx, hipStream_t s);
void cvlm_attention_launch(const bf16_t* qr, const int* slot, const int* pos, int rows, int heads, int kv_heads, const bf16_t* kc,
                           const bf16_t* vc, int max_ctx, bf16_t* out, hipStream_t s);

enum CvlmLinear { CVLM_LIN_QKV = 0, CVLM_LIN_O = 1, CVLM_LIN_GATE_UP = 2, CVLM_LIN_DOWN = 3, CVLM_LIN_HEAD = 4 };

class CosyLlm {
  public:
    // every key, shape and dtype is checked on the host before any HIP call (WeightLoadError); host_only: stop there (no device is touched)
    CosyLlm(const qasr_cvlm_config& cfg, const SafeTensorsDir& st, bool host_only = false);
    ~CosyLlm();
    const qasr_cvlm_config& config() const { return cfg_; }
    int vocab() const { return cfg_.speech_tokens + cfg_.speech_extra; }
    size_t footprint() const { return wl_ ? wl_->param_bytes() : 0; }      // a host_only object holds nothing
    size_t device_bytes() const { return wl_ ? wl_->device_bytes() : 0; }
    static void check_geometry(const qasr_cvlm_config& c);      // std::invalid_argument for what the kernels do not serve
    static int context(const qasr_cvlm_config& c);              // positions of a row's cache
    // the prefix of a row as the prompt pass reads it: text ids as they are, speech ids as -1 - id (buildInputSequence)
    static std::vector<int> plan_prefix(const qasr_cvlm_config& c, const CvlmRow& r);
    // tokens [B][max_tokens] (the handle's; -1 past a row's count), n_tokens [B]
    void generate(const std::vector<CvlmRow>& rows, const qasr_cvlm_sampling& s, unsigned long long seed, int32_t* tokens, int32_t* n_tokens);
    // teacher-forced: tokens [B][T] -> logits [B][T][V], hidden [B][T][hidden] (post-norm), either may be null
    void forced(const std::vector<CvlmRow>& rows, const int32_t* tokens, int T, float* logits, float* hidden);
    // the device sampler alone: logits [B][V], history[b] [n_history[b]]
    void sample(int B, const float* logits, const int32_t* const* history, const int32_t* n_history, const int32_t* step,
                const int32_t* below_min, const qasr_cvlm_sampling& s, unsigned long long seed, const int64_t* row_index, int32_t* out);
    // one linear of the handle alone: x [B][K] (bf16 values), resid [B][N] for o / down, y [B][N] (gate_up: [B][inter])
    void linear_probe(int layer, int kind, int B, const float* x, const float* resid, float* y);
    static void linear_shape(const qasr_cvlm_config& c, int kind, int& K, int& N_out);
    struct State;                        // per-row device state (llm_cosyvoice.hip)

  private:
    using Layer = QlmLayer;
    void load_all(const SafeTensorsDir& st, QlmLoader& wl);
    void gemv(int epi, const QLin& w, const bf16_t* X, int B, const bf16_t* norm_w, bf16_t* out, float* logits);
    void layers(int rows, const int* slot, const int* pos, bool last_kv_only);
    void prefill(const std::vector<CvlmRow>& rows, const qasr_cvlm_sampling* s, int forced_T);
    void issue_step(int B, bool forced_mode);
    void run_step(int B);
    void set_knobs(const qasr_cvlm_sampling& s, unsigned long long seed);
    State state() const;

    qasr_cvlm_config cfg_;
    hipStream_t stream_ = nullptr;
    std::unique_ptr<QlmLoader> wl_;      // the weights' and workspaces' arena; null in a host_only object
    std::vector<Layer> layers_;
    QLin head_;
    const bf16_t *text_emb_ = nullptr, *speech_emb_ = nullptr, *norm_ = nullptr;
    int max_ctx_ = 0, max_prefix_ = 0;
    float *d_cos_ = nullptr, *d_sin_ = nullptr;
    bf16_t *d_k_ = nullptr, *d_v_ = nullptr;
    bf16_t *d_x_ = nullptr, *d_hn_ = nullptr, *d_qkv_ = nullptr, *d_qr_ = nullptr, *d_attn_ = nullptr, *d_act_ = nullptr, *d_res_ = nullptr;
    float* d_logits_ = nullptr;
    int *d_state_ = nullptr, *d_tokens_ = nullptr, *d_pick_ = nullptr, *d_prefix_ = nullptr, *d_pairs_ = nullptr, *d_iota_ = nullptr,
        *d_probe_ = nullptr;
    long long* d_row_index_ = nullptr;
    CvlmSampleParams* d_knobs_ = nullptr;
    float *d_f_log_ = nullptr, *d_f_hid_ = nullptr;             // forced-pass outputs (sized per call)
    int* d_f_tok_ = nullptr;
    int forced_T_ = 0;
    std::unique_ptr<DevBuf> forced_buf_[3];
    StepGraphs graphs_;                                         // the step's launch sequence per batch size
};

}  // namespace qasr
