// vae_voxcpm.h -- the VoxCPM2 AudioVAE on the device (kernels and host object in vae_voxcpm.hip, C ABI in api_avae.cpp): 16 kHz PCM ->
// latent frames [F][latent_dim] at 25 frames per second, latent frames -> 48 kHz PCM, 1920 samples per frame.
//
// Reference: Sources/VoxCPM2TTS/AudioVAE.swift:10-25 (Snake1d), :63-158 (the causal conv wrappers), :240-351 (residual unit, encoder and
// decoder blocks), :355-411 (sample-rate condition), :431-562 (CausalEncoder, CausalDecoder), :618-686 (encode, decode, preprocess,
// sanitize); Configuration.swift:138-204; VoxCPM2TTS.swift:450-511, :743-850 (the keys).  Activations are channel-last rows; every conv
// pads on the left only, with zeros put in front of the already-Snaked input, so a row before a clip's first row adds an exact zero.
//   encoder  conv_in 1 -> D k 7 | per rate s: three residual units (dilation 1, 3, 9), Snake, conv k 2 s stride s to twice the width |
//            fc_mu k 3 to latent_dim
//   decoder  conv_in depthwise k 7 + 1x1 to D | per rate s: h scale[idx] + bias[idx], Snake, transposed conv k 2 s stride s to half the
//            width with its last s rows trimmed, three residual units | Snake, conv_out k 7 to one channel, tanh
//   unit     x + conv2(snake2(conv1(snake1(x)))), conv1 depthwise k 7 dilated, conv2 1x1
// f32 throughout, as the reference runs it (VoxCPM2TTS.swift:225).  Summation orders: DESIGN.md section 25.
#pragma once
#include "engine.h"
#include "safetensors.h"
#include <string>
#include <vector>

namespace qasr {

constexpr long AV_DEFAULT_FRAMES = 1024, AV_MAX_FRAMES = 1L << 14;
constexpr int AV_MAX_RATES = 8, AV_STAGES = 2 * (AV_MAX_RATES + 2);   // timing slots: encoder conv_in, blocks, fc_mu | decoder conv_in, blocks, conv_out
constexpr int AV_SLAB = 64;            // rows of a workgroup of the depthwise and the fused unit launches
constexpr int AV_FUSE_MAX = 128;       // the widest unit the fused launch holds in LDS (conv2's weights are 64 KB there)

struct AvaeConfig {                    // AudioVAEConfig.init(from:) defaults
    int encoder_dim = 128, latent_dim = 64, decoder_dim = 2048, sample_rate = 16000, out_sample_rate = 48000;
    std::vector<int> encoder_rates{2, 5, 8, 8}, decoder_rates{8, 6, 5, 2, 2, 2}, sr_bin_boundaries{20000, 30000, 40000};
    bool depthwise = true, use_noise_block = false;
    std::string cond_type = "scale_bias";
    int hop() const { int h = 1; for (int r : encoder_rates) h *= r; return h; }
    int samples_per_frame() const { int h = 1; for (int r : decoder_rates) h *= r; return h; }
};
// model_dir/config.json's audio_vae_config (the file and the object are optional); throws std::invalid_argument "<who>: <field> ..."
// for a value this port refuses
AvaeConfig avae_read_config(const std::string& model_dir, const char* who);
// every tensor of the AudioVAE out of the directory's *.safetensors, under the names and shapes the reference's modules hold after
// AudioVAE.sanitize (:646-686): weight_g / weight_v pairs fused, a bare encoder. / decoder. prefix completed, fc_logvar left out, an
// embedding table [n][8][8] flattened.  Throws WeightLoadError naming the tensor.  Host work only.
CheckedWeights avae_load_weights(const std::string& model_dir, const char* who, const AvaeConfig& cfg);

// one clip of a call: encode reads pcm [n] and writes out, decode reads z [T][latent_dim] and writes out
struct AvaeClip { const float* in; long n; float* out; };

class AudioVaeVoxcpm {
  public:
    AudioVaeVoxcpm(int device, const AvaeConfig& cfg, const CheckedWeights& w, long max_frames, hipStream_t work);
    ~AudioVaeVoxcpm();
    // stage < 0: the whole direction (z, or PCM).  stage k >= 0: the rows after conv_in (0) or after block k - 1, as the reference holds
    // them (before the next block's affine and Snake).  Clips are cut into passes of at most max_frames frames at clip boundaries.
    void encode(const std::vector<AvaeClip>& clips, int stage);
    void decode(const std::vector<AvaeClip>& clips, int sr_cond, int stage);
    // the decoder's last step alone: rows [1920 T][C_last] as _dec_stage(last) returns them -> PCM (Snake at the load, the same sums)
    void output(const std::vector<AvaeClip>& clips);
    void unload();
    bool loaded() const { return loaded_; }
    size_t footprint() const { return loaded_ ? param_bytes_ : 0; }
    long max_frames() const { return max_frames_; }
    const AvaeConfig& config() const { return cfg_; }
    long frames_of(long samples) const { return (samples + cfg_.hop() - 1) / cfg_.hop(); }
    // rows per latent frame and width of a stage's output; false when k is out of range
    bool stage_shape(bool decoder, int k, int* rows_per_frame, int* width) const;
    const float* timing() const { return timing_; }
    hipStream_t stream() const { return work_; }

  private:
    struct Gemm { size_t wt = 0, bias = 0; int K = 0, N = 0, Cin = 0, taps = 1, bmod = 0; };
    struct Snake { size_t a = 0, inv = 0; };
    struct Unit { Snake s1, s2; size_t w1 = 0, b1 = 0; Gemm c2; int C = 0, dil = 1; };
    struct Map { const float *a = nullptr, *inv = nullptr, *affine = nullptr; };   // what a block's last launch applies for its reader
    void check_loaded() const;
    template <class F> void passes(const std::vector<AvaeClip>& clips, bool samples, F&& run);
    void begin_pass(const AvaeClip* c, int n, bool samples);
    void unit(const Unit& u, long rows, int rate, const float* x, float* t, float* y, const Map& map);
    void gemm(const Gemm& g, int epi, long rows, int rate, int stride, const float* A, const float* R, float* C, const Map& map);
    void run_encoder(int stage);
    void run_decoder(int idx, int stage);
    void finish(int first, int last);
    const float* W(size_t off) const { return d_w_.as<float>() + off; }
    int device_;
    AvaeConfig cfg_;
    long max_frames_;
    size_t param_bytes_ = 0;
    bool loaded_ = true;
    hipStream_t own_ = nullptr, work_ = nullptr;
    hipEvent_t ev_[AV_STAGES + 1] = {};
    float timing_[AV_STAGES] = {};
    // weights (offsets in floats into d_w_)
    size_t enc_in_w_ = 0, enc_in_b_ = 0, dec_in_w_ = 0, dec_in_b_ = 0, out_w_ = 0, out_b_ = 0;
    std::vector<Unit> enc_units_, dec_units_;          // three per block
    std::vector<Snake> enc_snake_, dec_snake_;         // of each block; dec_snake_ ends with snake_out
    std::vector<Gemm> enc_down_, dec_up_;
    std::vector<size_t> affine_;                       // per decoder block: [buckets][2][C] scale | bias
    Gemm fc_mu_, dec_in1_;
    // the pass
    long frames_ = 0;
    std::vector<int> h_fstart_;                        // per frame row: the first frame row of its clip
    std::vector<long> clip_first_;                     // first frame row of each clip of the pass
    DevBuf d_w_, d_fstart_, d_pcm_, d_z_, d_b_[3];
};

}  // namespace qasr
