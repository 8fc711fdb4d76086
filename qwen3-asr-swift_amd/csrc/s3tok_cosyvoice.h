// s3tok_cosyvoice.h -- the CosyVoice3 speech tokenizer (S3-Tokenizer-v3) and the two mel front ends of a voice profile on the device
// (kernels and host object in s3tok_cosyvoice.hip, C ABI in api_s3tok.cpp): a reference clip -> the prompt speech tokens at 25 Hz and
// the 80-bin prompt mel at 50 Hz that the flow decoder (flow_cosyvoice.h) and the LLM (llm_cosyvoice.h) take for zero-shot cloning.
//
// Reference: Sources/CosyVoiceTTS/SpeechTokenizer.swift:40-95 (FSQ), :105-200 (FSMN attention), :213-235 (block), :243-289 (encoder);
// WhisperMelExtractor.swift:31-225; FlowMelExtractor.swift:40-229; VoiceCloning.swift:69-158 (extractVoiceProfile), :329-345 (resample);
// WeightLoading.swift:350-398 (keys of speech_tokenizer.safetensors).  DESIGN.md section 24.
//
// Precision (section 22's plan): the residual stream, LayerNorm statistics, the FSMN sum, project_down and the FSQ are f32; GEMM operands
// are bf16 with f32 accumulation, from bf16 Wt[n][k] images made once at load; q and k are rounded once after RoPE, v once.
#pragma once
#include "engine.h"
#include "mel.h"
#include "safetensors.h"
#include <cstdint>
#include <string>
#include <vector>

namespace qasr {

constexpr int S3_MELS = 128, S3_DIM = 1280, S3_HEADS = 20, S3_HD = 64, S3_FF = 5120, S3_FSMN_K = 31, S3_FSMN_PAD = 15, S3_FSQ = 8;
constexpr int S3_MAX_DEPTH = 64, S3_STAGES = 4;
constexpr long S3_DEFAULT_TOKENS = 768, S3_MAX_TOKENS = 1L << 14, S3_MAX_SAMPLES = 1L << 24;     // 768 tokens: 30.7 s
constexpr int FM_MELS = 80, FM_NFFT = 1920, FM_HOP = 480, FM_PAD = 720, FM_PADDED = 2048, FM_BINS = 1025, FM_SR = 24000;
constexpr float S3_FSQ_SCALE = 0.9990000128746033f;                                             // SpeechTokenizer.swift:79

// ---- lengths (host) ----
inline size_t s3_whisper_frames(size_t n) { return n / MEL_HOP; }                               // last frame dropped (WhisperMelExtractor.swift:154-155)
inline size_t s3_tokens(size_t T) { return T ? ((T - 1) / 2 + 1 - 1) / 2 + 1 : 0; }            // two convs k 3, stride 2, pad 1
inline size_t s3_flow_frames(size_t n) { return n >= (size_t)FM_HOP ? n / FM_HOP : 0; }         // (n + 1440 - 1920) / 480 + 1 (FlowMelExtractor.swift:164-165)
size_t s3_resampled_length(size_t n, int src, int dst);                                         // VoiceCloning.swift:331-332
// out holds s3_resampled_length values (VoiceCloning.swift:329-345)
void s3_resample(const float* x, size_t n, int src, int dst, float* out);
// projections [rows][8] -> codes (SpeechTokenizer.swift:78-93), the host twin of the device's lines
void s3_fsq_host(const float* proj, size_t rows, int32_t* codes);

struct S3Weights {
    int depth = 0;
    CheckedWeights f;
};
// speech_tokenizer.safetensors checked on the host: depth and every key, shape and dtype; throws WeightLoadError naming the key
S3Weights s3_load_weights(const std::string& dir);

// one clip of a run: pcm (16 kHz) or mel ([128][T], T frames); any of the outputs may be null
struct S3Clip {
    const float* pcm = nullptr;
    long n = 0;
    const float* mel = nullptr;
    long T = 0;
    float* hidden = nullptr;           // [tokens][1280]
    float* proj = nullptr;             // [tokens][8]
    int32_t* codes = nullptr;          // [tokens]
};

class S3Tokenizer {
  public:
    S3Tokenizer(int device, const S3Weights& w, long max_tokens, hipStream_t work);
    ~S3Tokenizer();
    int depth() const { return depth_; }
    long max_tokens() const { return max_tokens_; }
    void whisper_mel(const float* pcm, long n, float* out /* [128][n / 160] */);
    void flow_mel(const float* const* pcm, const long* n, int B, float* const* out /* [80][n / 480] each */);
    // any number of clips, cut into passes of at most max_tokens rows at clip boundaries; a clip alone over max_tokens is refused
    void run(const std::vector<S3Clip>& clips);
    void unload();
    bool loaded() const { return loaded_; }
    size_t footprint() const { return loaded_ ? param_bytes_ : 0; }
    const float* timing() const { return timing_; }             // ms of the last run: mel, stems, blocks, fsq
    hipStream_t stream() const { return work_; }

  private:
    struct Dense { size_t w = 0, bias = 0; int N = 0, K = 0; };
    struct Block { Dense qkv, o, fc1, fc2; size_t fsmn = 0, ln1_g = 0, ln1_b = 0, ln2_g = 0, ln2_b = 0; };
    void check_loaded() const;
    void pass(const S3Clip* c, int n);
    void front_end(const S3Clip* c, int n, const std::vector<int>& frame_off);     // whisper mel of pcm clips -> d_melf_
    void grow(DevBuf& b, size_t bytes);
    const bf16_t* W(size_t off) const { return d_w_.as<bf16_t>() + off; }
    const float* F(size_t off) const { return d_f_.as<float>() + off; }
    int device_, depth_ = 0;
    long max_tokens_;
    size_t param_bytes_ = 0;
    bool loaded_ = true;
    hipStream_t own_ = nullptr, work_ = nullptr;
    hipEvent_t ev_[S3_STAGES + 1] = {};
    float timing_[S3_STAGES] = {};
    MelTables mel_tab_;
    Dense conv1_, conv2_;
    std::vector<Block> blocks_;
    size_t proj_w_ = 0, proj_b_ = 0, rope_cos_ = 0, rope_sin_ = 0, fm_hann_ = 0, fm_tw1024_ = 0, fm_tw2048_ = 0, fm_fbw_ = 0, fm_fbi_ = 0;
    DevBuf d_w_, d_f_, d_i_, d_cu_, d_pos_, d_info_, d_stem1_, d_stem2_, d_melb_, d_h1_, d_xs_, d_a_, d_attn_, d_qkv_, d_u_, d_proj_, d_codes_;
    DevBuf d_pcm_, d_tab_, d_raw_, d_gmax_, d_melf_, d_fm_out_, d_rows_;                     // front ends: grown on demand
};

}  // namespace qasr
