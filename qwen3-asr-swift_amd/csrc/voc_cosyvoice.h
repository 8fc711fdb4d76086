// voc_cosyvoice.h -- the CosyVoice3 HiFT vocoder on the device (kernels and host object in voc_cosyvoice.hip, C ABI in api_voc.cpp):
// 80-bin mel frames of 20 ms -> 24 kHz PCM, 480 T + 16 samples for T frames.
//
// Reference: Sources/CosyVoiceTTS/HiFiGAN.swift:635-858 (HiFiGANGenerator), :336-374 (F0Predictor), :229-329 (SineGenerator,
// SourceModuleHnNSF), :410-486 (stft), :502-620 (istft), :176-222 (ResBlock), :10-26 (SnakeActivation), :35-169 (the three conv
// wrappers); Configuration.swift:84-107; WeightLoading.swift:214-331 (keys of hifigan.safetensors).  Per clip of T frames:
//   f0      5 convs 80 -> 512 -> .. -> 512 with ELU (the first k = 4 reading t .. t + 3, the others k = 3 reading t - 2 .. t), |Linear 512 -> 1|
//   source  9 harmonics of the F0 held for 480 samples each, running phase, 0.1 sin where f0 > 10 and 0.003 N(0, 1) where not,
//           tanh(Linear 9 -> 1) + 0.003 N(0, 1): 480 T samples; then a 16-point STFT at hop 4 with reflect padding 8: 120 T + 1 frames
//           of 9 real | 9 imaginary
//   decode  conv_pre k = 5 reading t .. t + 4 | three stages (LeakyReLU 0.1, nearest upsample x 8 / 5 / 3 + causal conv 512 -> 256 ->
//           128 -> 64, on the last stage one reflected row in front, + source_resblocks(source_downs(STFT)), mean of three ResBlocks
//           k = 3, 7, 11) | LeakyReLU 0.01, conv_post 64 -> 18, exp | sin, inverse STFT without trimming, clip to 0.99
// f32 throughout, except the source's running phase, which is kept in cycles in f64.
#pragma once
#include "engine.h"
#include "safetensors.h"
#include <string>
#include <vector>

namespace qasr {

constexpr int HF_RATE = 24000, HF_NMELS = 80, HF_C = 512, HF_HARM = 9, HF_NFFT = 16, HF_HOP = 4, HF_BINS = 9, HF_SPEC = 18;
constexpr int HF_SAMPLES_PER_FRAME = 480, HF_ROWS_PER_FRAME = 120, HF_STAGES = 7, HF_MAX_CLIPS = 1024;
constexpr int HF_TILE = 64;            // rows of a GEMM tile; the tile grid runs over the rows of the pass, whatever clips they belong to
constexpr int HF_TAIL_FRAMES = 64;     // inverse-STFT frames (4 samples each) a workgroup of the tail launch owns
constexpr long HF_DEFAULT_FRAMES = 4096, HF_MAX_FRAMES = 1L << 17;
constexpr int HF_RATES[3] = {8, 5, 3}, HF_UP_K[3] = {16, 11, 7}, HF_CH[4] = {512, 256, 128, 64};
constexpr int HF_DOWN_STRIDE[3] = {15, 3, 1}, HF_DOWN_K[3] = {30, 6, 1}, HF_SRC_K[3] = {7, 7, 11}, HF_RES_K[3] = {3, 7, 11};
constexpr int HF_DIL[3] = {1, 3, 5};

// The generator's noise (include/qasr.h): draw `counter` of a clip's stream is splitmix64 of seed + (counter + 1) gamma, the counter form of
// csrc/sampler.cpp's generator.  One draw gives one value: u1 = ((r >> 40) + 1) 2^-24 in (0, 1], u2 = ((r >> 16) & 0xFFFFFF) 2^-24 in [0, 1);
// uniform = u2, normal = sqrt(-2 ln u1) cos(2 pi u2).  Host and device run these same lines; tests/hift_oracle.py restates them in f64.
__host__ __device__ inline unsigned long long hift_draw(unsigned long long seed, unsigned long long counter) {
    unsigned long long z = seed + (counter + 1ull) * 0x9e3779b97f4a7c15ull;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
__host__ __device__ inline float hift_uniform(unsigned long long r) { return (float)((r >> 16) & 0xFFFFFFull) * (1.0f / 16777216.0f); }
__host__ __device__ inline float hift_normal(unsigned long long r) {
    const float u1 = (float)((r >> 40) + 1ull) * (1.0f / 16777216.0f);
    return sqrtf(-2.0f * logf(u1)) * cosf(6.28318530717958647692f * hift_uniform(r));
}

inline size_t hift_num_samples(size_t T) { return T ? (size_t)HF_SAMPLES_PER_FRAME * T + HF_NFFT : 0; }
// key -> shape of every tensor read from hifigan.safetensors
std::vector<std::pair<std::string, std::vector<int64_t>>> hift_tensor_shapes();

// mel [T][80]; f0 [T]; src [480 T]; pcm [480 T + 16].  Which pointers a mode reads and writes: see HiftCosyVoice::run.
struct HiftClip { const float* mel; long T; unsigned long long seed; const float* f0_in; float* f0_out; const float* src_in; float* src_out; float* pcm; };

class HiftCosyVoice {
  public:
    enum Mode { F0, SOURCE, DECODE_SOURCE, DECODE };
    HiftCosyVoice(int device, const CheckedWeights& w, long max_frames, hipStream_t work);
    ~HiftCosyVoice();
    // any number of clips, cut into passes of at most max_frames frames at clip boundaries; a clip over max_frames is std::invalid_argument
    //   F0             mel -> f0_out
    //   SOURCE         f0_in, seed -> src_out
    //   DECODE_SOURCE  mel, src_in -> pcm
    //   DECODE         mel, seed -> pcm: the three above chained on the device, the same bits
    void run(const std::vector<HiftClip>& clips, Mode mode);
    void unload();
    bool loaded() const { return loaded_; }
    size_t footprint() const { return loaded_ ? param_bytes_ : 0; }
    long max_frames() const { return max_frames_; }
    const float* timing() const { return timing_; }    // ms per stage of the last call (HF_STAGES): f0, source, stft, conv_pre, stage 0..2 + tail
    hipStream_t stream() const { return work_; }

  private:
    struct Conv { size_t wt = 0, bias = 0; int K = 0, N = 0, Cin = 0, taps = 1; };
    struct Snake { size_t a = 0, inv = 0; };
    struct ResBlock { Conv c1[3], c2[3]; Snake s1[3], s2[3]; int k = 0; };
    struct Level { const int* start; long rows; };     // first rows of the clips at one rate, and the rows of the pass
    void check_loaded() const;
    void pass(const HiftClip* c, int n, Mode mode);
    void dev_f0();
    void dev_source();
    void dev_decode();
    void finish(bool f0, bool source, bool decode);
    void resblock(const ResBlock& rb, const Level& lv, const float* x, float* h, float* t1, float* out, int acc_mode);
    const float* W(size_t off) const { return d_w_.as<float>() + off; }
    int device_;
    long max_frames_;
    size_t param_bytes_ = 0;
    bool loaded_ = true;
    hipStream_t own_ = nullptr, work_ = nullptr;
    hipEvent_t ev_[HF_STAGES + 1] = {};
    float timing_[HF_STAGES] = {};
    // weights and tables (offsets in floats into d_w_)
    Conv cond_[5], cls_, pre_, ups_[3], down_[3], post_;
    ResBlock src_rb_[3], rb_[3][3];
    size_t merge_w_ = 0, merge_b_ = 0, hann_ = 0, dft_cos_ = 0, dft_sin_ = 0, idft_cos_ = 0, idft_sin_ = 0;
    // the pass: start tables of the six levels (frames, 8 T, 40 T, 120 T + 1, samples 480 T, PCM 480 T + 16), HF_MAX_CLIPS + 1 ints each
    int n_clips_ = 0;
    long frames_ = 0;
    std::vector<int> h_start_;
    std::vector<unsigned long long> h_seed_;
    std::vector<int> h_tiles_;                         // of the tail launch: (first row, rows, first hop, first PCM sample) per tile
    DevBuf d_w_, d_start_, d_seed_, d_mel_, d_f0_, d_base_, d_src_, d_stft_, d_pcm_, d_tiles_, d_b_[5];
};

}  // namespace qasr
