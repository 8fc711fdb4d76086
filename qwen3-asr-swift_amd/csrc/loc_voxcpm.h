// loc_voxcpm.h -- the two "local" networks of VoxCPM2 on the device (kernels and host object in loc_voxcpm.hip, C ABI in api_vloc.cpp):
// VoxCPMLocEnc, a patch of P latent frames -> one embedding for the language model, and VoxCPMLocDiTV2 under UnifiedCFM, the language
// model's two hidden vectors and the previous patch -> the next patch by an Euler solve under classifier-free guidance.
//
// Reference: Sources/VoxCPM2TTS/MiniCPM4.swift:10-31 (RMSNorm), :35-113 (LongRoPE, rotate-half), :152-166 (the time span), :226-476
// (MiniCPM attention, MLP, layer, model), :480-539 (LocEnc), :543-652 (sinusoid, TimestepEmbedding, LocDiT), :654-746 (UnifiedCFM);
// Configuration.swift:3-136; VoxCPM2TTS.swift:81-124 (how lm_config, encoder_config and dit_config combine), :377-449 (the keys),
// :1312, :1368-1371, :1388 (enc_to_lm_proj, lm_to_dit_proj | res_to_dit_proj).
//   layer    h = x + s attn(n1(x)),  h + s down(silu(gate(n2(h))) up(n2(h))),  s = scale_depth / sqrt(depth of the stack) under use_mup
//   LocEnc   [special_token ; in_proj(patch rows)] -> stack -> final norm -> token 0 -> enc_to_lm_proj
//   LocDiT   [mu tokens ; time token ; cond_proj(cond rows) ; in_proj(x rows)] -> stack -> final norm -> out_proj on the last P tokens
// Rows are [P][feat_dim] everywhere (the reference's layout after its transposes; what qasr_avae_* reads and writes).
// Precision: the residual stream, norms, RoPE, attention, softmax, time token, st and the Euler line are f32; every Linear multiplies
// bf16 weights by activations rounded to bf16 at the load and accumulates in f32.  Layouts and summation orders: DESIGN.md section 26.
// The CFG-zero-star sums: prod[i] = pos[i] neg[i] and sq[i] = neg[i] neg[i], i over the patch's P feat_dim values in row order, each array
// padded with zeros to the next power of two n and reduced by  for (s = n / 2; s > 0; s /= 2) a[i] += a[i + s], i < s;  then
// st = dot / (sq + 1e-8), a = neg st, d = a + cfg (pos - a), x = x - dt d, one rounding per operation.
#pragma once
#include "engine.h"
#include "safetensors.h"
#include <map>
#include <string>
#include <vector>

namespace qasr {

constexpr int VL_HEAD_DIM = 128;       // the only head width the attention launch serves
constexpr int VL_MAX_S = 32;           // keys of a sequence; they live in LDS
constexpr int VL_MAX_STEPS = 64;
constexpr int VL_KC = 512;             // K chunk of the skinny GEMM: every Linear's K is a multiple of it (or K <= 256 for the feature inputs)
constexpr long VL_DEFAULT_SEQS = 32, VL_MAX_SEQS = 1024;
constexpr int VL_MAX_SOLVES = 16;       // captured solves kept per handle; one more (batch, steps) pair drops them all
constexpr int VL_TIMING = 4;           // ms of the last encode | mu | velocity | solve

struct VlocStack { int hidden = 1024, ffn = 4096, heads = 16, layers = 12, head_dim = 128; };

struct VlocConfig {                    // ModelArgs / LMConfig / EncoderConfig / DiTConfig defaults
    VlocStack enc, dit;
    int patch_size = 4, feat_dim = 64, lm_hidden = 2048, kv_heads = 2, mu_tokens = 2;
    float rms_eps = 1e-5f, rope_theta = 10000.0f, scale_depth = 1.4f;
    bool use_mup = false;
    int max_pos = 32768, rope_orig = 32768;            // lm_config.max_position_embeddings, rope_scaling.original_max_position_embeddings
    std::vector<float> short_factor, long_factor;
    int mu_dim() const { return mu_tokens * dit.hidden; }
    int dit_tokens() const { return mu_tokens + 1 + 2 * patch_size; }
    float resid_scale(const VlocStack& s) const;       // Float(scale_depth) / sqrt(Float(depth)), or 1
};
// model_dir/config.json (the file and every key optional); throws std::invalid_argument "<who>: <field> ..." for what this port refuses
VlocConfig vloc_read_config(const std::string& model_dir, const char* who);
// an MLX affine-quantised Linear as stored: 4 or 8 bits, groups of 64 along K; scales and biases widened to f32 (exact)
struct VlocQuant { std::vector<uint32_t> wq; std::vector<float> scales, biases; int N = 0, K = 0, bits = 0; };
struct VlocWeights { CheckedWeights f; std::map<std::string, VlocQuant> q; };   // q: by the Linear's stem
// every tensor of the two networks and the three projections out of the directory's *.safetensors, each checked for presence, shape and
// dtype: floats F32 / F16 / BF16; a Linear with .scales as the U32 / scales / biases triplet of an MLX 4-bit or 8-bit checkpoint.
// f.disk_bytes counts all of them as stored.  Sets cfg.mu_tokens from the rows of lm_to_dit_proj and res_to_dit_proj.  Throws
// WeightLoadError naming the tensor.  Host work only.
VlocWeights vloc_load_weights(const std::string& model_dir, const char* who, VlocConfig& cfg);

// makeUnifiedCFMTimeSpan: t[0 .. n], in double, rounded to float
void vloc_schedule(int n_steps, float* t);
// max(1, Int(Double(n + 1) 0.04)): the leading steps whose derivative is zero
int vloc_zero_steps(int n_steps);
// MiniCPMLongRoPE's tables for positions 0 .. n_pos - 1, [n_pos][head_dim], in f64 rounded to f32; std::invalid_argument for a factor list
// whose length is neither 0, 1 nor head_dim / 2
void vloc_rope_table(const VlocConfig& cfg, int head_dim, int n_pos, float* cos, float* sin);

// The launch entry of the stacks' attention (kernel in loc_voxcpm.hip; head_dim 128, f32, no mask): qkv [n_seq * S][(heads + 2 kv_heads) *
// 128], RoPE from rows 0 .. S - 1 of rcos / rsin [positions][128] -> out [n_seq * S][heads * 128].  Query head h reads K/V head
// h / (heads / kv_heads).  std::invalid_argument for S outside 1 .. 32 or heads no multiple of kv_heads.
void vl_attention_launch(const float* qkv, long n_seq, int S, int heads, int kv_heads, const float* rcos, const float* rsin, float* out,
                         hipStream_t s);

class LocVoxcpm {
  public:
    LocVoxcpm(int device, const VlocConfig& cfg, const VlocWeights& w, long max_seqs, hipStream_t work);
    ~LocVoxcpm();
    // feats [n][P][feat_dim] -> cls [n][enc.hidden] and / or embed [n][lm_hidden], in passes of at most max_seqs patches
    void encode(const float* feats, long n, float* cls, float* embed);
    void mu(const float* lm_hidden, const float* res_hidden, long B, float* mu);
    // one estimator call, mu as given: x, cond [B][P][feat_dim], mu [B][mu_dim] -> v [B][P][feat_dim]
    void velocity(const float* x, const float* mu, const float* cond, long B, float t, float* v);
    // the Euler solve from z; v_out: the last step's guided derivative
    void solve(const float* mu, const float* cond, const float* z, long B, int n_steps, float cfg, float* x_out, float* v_out);
    // the first n_layers layers of a stack (which: 0 LocEnc, 1 LocDiT) on embeddings x [n_seq][S][hidden]; the final norm with all of them
    void stack(int which, const float* x, long n_seq, int S, int n_layers, float* out);
    void unload();
    bool loaded() const { return loaded_; }
    size_t footprint() const { return loaded_ ? param_bytes_ : 0; }
    long max_seqs() const { return max_seqs_; }
    const VlocConfig& config() const { return cfg_; }
    const float* timing() const { return timing_; }
    hipStream_t stream() const { return work_; }

  private:
    struct Lin { size_t w = 0, bias = 0; int K = 0, N = 0; bool has_bias = false; };   // w in bf16 elements, bias in floats
    struct Layer { size_t n1 = 0, n2 = 0; Lin qkv, o, gu, down; };
    struct Net { VlocStack g; std::vector<Layer> layers; size_t norm = 0; float s = 1.0f; };
    struct Solve { hipGraphExec_t exec = nullptr; DevBuf ttok; };
    void check_loaded() const;
    void gemm(const Lin& l, const float* A, long lda, int a_group, int a_stride, int a_off, const float* norm_w, const float* resid, long ldr,
              float s, int act, bool swiglu, float* out, long ldo, long M);
    void run_stack(const Net& net, long n_seq, int S, int n_layers);
    void final_norm(const Net& net, long rows, int group, int stride, int off, float* out);
    void time_tokens(const float* t, int n, float* out);
    void small_linear(const Lin& l, const float* x, long rows, float* out);
    void assemble_dit(long n_seq, long mu_seqs, long B, const float* ttok);
    void issue_solve(long B, int n_steps, const float* ttok);
    void drop_solves();
    void begin(int slot);
    void end(int slot);
    const bf16_t* Wb(size_t off) const { return d_wb_.as<bf16_t>() + off; }
    const float* Wf(size_t off) const { return d_wf_.as<float>() + off; }
    int device_;
    VlocConfig cfg_;
    long max_seqs_;
    size_t param_bytes_ = 0;
    bool loaded_ = true;
    hipStream_t own_ = nullptr, work_ = nullptr;
    hipEvent_t ev_[2] = {};
    float timing_[VL_TIMING] = {};
    Net enc_, dit_;
    Lin enc_in_, dit_in_, dit_cond_, dit_out_, t1_, t2_, dt1_, dt2_, enc_to_lm_, lm_to_dit_, res_to_dit_;
    size_t special_ = 0, rope_cos_ = 0, rope_sin_ = 0;
    std::map<std::pair<long, int>, Solve> solves_;     // one captured solve per (B, n_steps), at most VL_MAX_SOLVES
    // weights: matrices as bf16, vectors and tables as f32
    DevBuf d_wb_, d_wf_;
    // the pass: token rows [2 max_seqs][32][hidden], q|k|v, attention output, SwiGLU output, the normed rows out_proj / enc_to_lm_proj read
    DevBuf d_h_, d_qkv_, d_attn_, d_act_, d_norm_, d_ab_;   // d_ab_: the rows of a wide-pass Linear as bf16
    unsigned knob_epoch_ = 0;
    std::vector<float> h_sin_;                         // host staging that outlives the call that fills it
    float h_cfg_ = 0.0f;
    DevBuf d_x_, d_mu_, d_cond_, d_condp_, d_v_, d_d_, d_cfg_, d_sin_, d_t1_, d_ttok_, d_dconst_, d_lm_, d_embed_;
};

}  // namespace qasr
