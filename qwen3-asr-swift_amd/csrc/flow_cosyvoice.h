// flow_cosyvoice.h -- the CosyVoice3 flow-matching mel decoder on the device (kernels and host object in flow_cosyvoice.hip, C ABI in
// api_flow.cpp): speech tokens at 25 Hz (+ prompt tokens, prompt mel, a 192-d speaker vector) -> an 80-bin mel at 50 Hz, the input of the
// HiFT vocoder (voc_cosyvoice.h).
//
// Reference: Sources/CosyVoiceTTS/FlowMatching.swift:46-197 (ConditionalFlowMatching: schedule, CFG, Euler), :204-227 (PreLookaheadLayer),
// :241-377 (CosyVoiceFlowModel); DiT.swift:10-33 (sinusoid), :39-59 (time MLP), :69-127 (AdaLN), :133-218 (attention, feed-forward),
// :224-268 (block), :283-327 (conv position embedding, Mish), :333-379 (input embedding), :387-483 (DiT); Configuration.swift:45-80;
// WeightLoading.swift:126-212 (keys of flow.safetensors); HiFiGAN.swift:35-84 (CausalDilatedConv1d).  DESIGN.md section 22.
//
// Precision: x, the residual stream, the modulation vectors, LayerNorm statistics and the solver are f32; GEMM operands are bf16 with f32
// accumulation.  q|k|v, to_out, ff, proj, the position convs and proj_out are bf16 images made once at load; the time MLP and the AdaLN
// linears stay packed and run as f32 GEMVs on one row per time step (they never see a mel row).
#pragma once
#include "engine.h"
#include "safetensors.h"
#include "voc_cosyvoice.h"
#include <cstdint>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

namespace qasr {

constexpr int FL_MEL = 80, FL_DIM = 1024, FL_HEADS = 16, FL_HD = 64, FL_FF = 2048, FL_SPK = 192, FL_IN = 320, FL_FREQ = 256;
constexpr int FL_CONV_K = 31, FL_CONV_GROUPS = 16, FL_LOOK_K = 4, FL_LOOK2_K = 3, FL_RATIO = 2, FL_GROUP = 64;
constexpr int FL_MAX_STEPS = 64, FL_DEFAULT_STEPS = 10, FL_MAX_CLIPS = 1024, FL_STAGES = 5, FL_MAX_DEPTH = 64;
constexpr long FL_DEFAULT_FRAMES = 4096, FL_MAX_FRAMES = 1L << 15;
constexpr float FL_CFG = 0.7f;

inline size_t flow_mel_frames(size_t n_tokens) { return (size_t)FL_RATIO * n_tokens; }
// t_i = 1 - cos(i / n * pi / 2) in Float (FlowMatching.swift:141-144); t holds n + 1 values
void flow_schedule(int n_steps, float* t);

// flow.safetensors checked on the host: depth, bits and every shape; throws WeightLoadError naming the key
struct FlowWeights {
    int depth = 0, bits = 0, vocab = 0;
    CheckedWeights f;                                          // every float tensor (scales and biases of the packed ones too)
    std::map<std::string, std::vector<uint32_t>> packed;       // `weight` of every quantised Linear
};
FlowWeights flow_load_weights(const std::string& dir);

// one clip of a call: whichever pointers the mode reads and writes (row-major [T][80] unless said otherwise)
struct FlowClip {
    long T = 0;
    const float *x = nullptr, *mu = nullptr, *spks = nullptr, *cond = nullptr;   // spks [80]; spks / cond may be null (zeros)
    unsigned long long seed = 0;
    float temperature = 1.0f;
    bool noise = false;                // x0 = temperature * the counter stream instead of x
    float *z_out = nullptr, *v_out = nullptr, *mel = nullptr;   // z_out [T][80]; v_out [2][T][80] (last step: conditioned, unconditioned); mel [T][80]
};

class FlowCosyVoice {
  public:
    FlowCosyVoice(int device, const FlowWeights& w, long max_frames, hipStream_t work);
    ~FlowCosyVoice();
    int vocab() const { return vocab_; }
    int depth() const { return depth_; }
    void mu(const int32_t* tokens, long n, float* out /* [2 n][80] */);
    void spks(const float* emb192, float* out80) const;       // host arithmetic in f32: 192 x 80 multiply-adds
    void velocity(const float* x, const float* mu, const float* spks, const float* cond, long T, float t, float* v);
    // any number of clips, cut into passes of at most max_frames frames at clip boundaries
    void solve(const std::vector<FlowClip>& clips, int n_steps);
    void unload();
    bool loaded() const { return loaded_; }
    size_t footprint() const { return loaded_ ? param_bytes_ : 0; }
    long max_frames() const { return max_frames_; }
    const float* timing() const { return timing_; }            // ms of the last call: modulation table, input_embed, blocks, output, Euler
    hipStream_t stream() const { return work_; }

  private:
    struct QLin { size_t w = 0, s = 0, b = 0, bias = 0; int N = 0, K = 0; };       // packed: offsets into d_q_ (words) and d_f_ (floats)
    struct Dense { size_t w = 0, bias = 0; int N = 0, K = 0; };                    // bf16 image: offset into d_w_ (elements), bias in d_f_
    struct Block { QLin ada; Dense qkv, o, ff1, ff2; };
    void check_loaded() const;
    void qgemv(const QLin& l, const float* x, int rows, long ldx, float* out, float* out_silu, long ldo);
    void modulation(const float* d_t, int rows, float* table);
    void set_pass(const FlowClip* c, int n, bool doubled);
    void forward(const float* mod);                            // rows_ rows of the pass -> d_v_
    void pass(const FlowClip* c, int n, int n_steps);
    const bf16_t* W(size_t off) const { return d_w_.as<bf16_t>() + off; }
    const float* F(size_t off) const { return d_f_.as<float>() + off; }
    int device_, depth_ = 0, bits_ = 0, vocab_ = 0;
    long max_frames_;
    size_t param_bytes_ = 0, mod_stride_ = 0;
    bool loaded_ = true;
    hipStream_t own_ = nullptr, work_ = nullptr;
    std::vector<hipEvent_t> ev_;
    int ev_used_ = 0;
    float timing_[FL_STAGES] = {};
    std::vector<float> h_spk_w_, h_spk_b_;
    QLin time1_, time2_, norm_out_;
    Dense proj_, conv_[2], out_;
    std::vector<Block> blocks_;
    size_t emb_ = 0, look1_w_ = 0, look1_b_ = 0, look2_w_ = 0, look2_b_ = 0, rope_cos_ = 0, rope_sin_ = 0;
    // the pass
    int n_seq_ = 0, max_len_ = 0, table_steps_ = 0;
    long src_rows_ = 0, cond_rows_ = 0, rows_ = 0;            // rows of x; rows whose conditioning is read; rows of the forward
    DevBuf d_w_, d_q_, d_f_, d_cu_, d_pos_, d_clip_, d_seed_, d_t_, d_sin_, d_emb_, d_mod_, d_mod1_, d_x_, d_xb_, d_condb_, d_mub_, d_spkb_, d_stage_,
        d_h0_, d_xs_, d_a_, d_attn_, d_qkv_, d_u_, d_v_, d_tok_, d_look_;
};

}  // namespace qasr
