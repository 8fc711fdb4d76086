// sep_openunmix.h -- Open-Unmix (UMX-HQ / UMX-L) music source separation on the device (kernels and host object in sep_openunmix.hip,
// C ABI in api_sep.cpp).
//
// Reference: Sources/SourceSeparation/STFT.swift:40-102 (forward, magnitude), :183-231 (inverseMLX), :240-260 (applyMaskAndInvert),
// OpenUnmixModel.swift:91-127 (stem network), :175-301 (BiLSTMLayer, LSTMCell), OpenUnmixConfig.swift:24-46 (presets),
// WienerFilterMLX.swift:139-261 (emWienerWindow), SourceSeparation.swift:45-175 (separate).
// Per file of n stereo samples at 44.1 kHz: STFT (4096 / 1024, centre pad 2048 by the reference's index rule) -> magnitude [T][2][2049]
// -> per stem: crop 1487 bins, (x + mean) * scale | fc1 BN tanh | 3 x BiLSTM(hidden / 2 per direction) | [skip | lstm] fc2 BN ReLU |
// fc3 BN | * scale + mean, ReLU, x magnitude -> Wiener EM over windows of frames (or the mixture's phase) -> inverse STFT.
// f32 throughout.
#pragma once
#include "engine.h"
#include "safetensors.h"
#include <string>
#include <vector>

namespace qasr {

constexpr int SEP_RATE = 44100, SEP_NFFT = 4096, SEP_HOP = 1024, SEP_BINS = 2049, SEP_MAXBIN = 1487, SEP_STEMS = 4, SEP_LAYERS = 3;
constexpr int SEP_IN = 2 * SEP_MAXBIN, SEP_OUT = 2 * SEP_BINS;      // 2974 network inputs, 4098 outputs per frame
extern const char* const SEP_STEM_NAMES[SEP_STEMS];                 // vocals, drums, bass, other: the file names and the output order

inline long sep_num_frames(size_t n) { return (long)(n / SEP_HOP) + 1; }    // (n + 4096 - 4096) / 1024 + 1 (STFT.swift:60)

// key -> shape of every tensor of one stem file at `hidden` (512 umxhq | 1024 umxl)
std::vector<std::pair<std::string, std::vector<int64_t>>> sep_tensor_shapes(int hidden);

struct SepTiming { float stft = 0, network = 0, wiener = 0, istft = 0; };

class SepOpenUnmix {
  public:
    // w: the four stems' checked tensors in SEP_STEM_NAMES order.  work: the stream the model's work is ordered on, nullptr = its own.
    SepOpenUnmix(int device, const CheckedWeights* w, int hidden, size_t max_batch_samples, hipStream_t work);
    ~SepOpenUnmix();
    // B files; right[b] == nullptr: mono (duplicated).  targets: bit s = stem s.  out[b]: [targets asked][2][n_b].
    void separate(const float* const* left, const float* const* right, const size_t* n, size_t B, unsigned targets, bool wiener,
                  int iterations, int window, float* const* out);
    // stage entry points on one file
    void stft(const float* left, const float* right, size_t n, float* re, float* im, float* mag);               // each [T][2][2049]
    void masks(const float* mag, const size_t* T, size_t B, float* out);                 // mag [sum T][2][2049] -> [4][sum T][2][2049]
    void wiener(const float* masked, int J, const float* re, const float* im, size_t T, int iterations, int window, float* out_re,
                float* out_im);                                                          // [J][T][2][2049]
    void istft(const float* re, const float* im, int J, size_t T, size_t length, float* out);                   // -> [J][2][length]
    void unload();
    bool loaded() const { return loaded_; }
    size_t footprint() const { return loaded_ ? param_bytes_ : 0; }
    int hidden() const { return hidden_; }
    size_t max_batch_samples() const { return max_samples_; }
    const SepTiming& timing() const { return timing_; }
    void set_recurrence_form(int form) { recur_form_ = form; }      // 0 all of W_hh streamed | 1 its first columns resident in registers
    hipStream_t stream() const { return work_; }

  private:
    struct Plan { int B = 0; long M = 0, total = 0; std::vector<long> n, off; std::vector<int> T, row0; };
    void check_loaded() const;
    void plan(const size_t* n, const size_t* T, size_t B);          // geometry of a pass: uploads the per-file tables
    void ensure_rows(long M, bool net, bool cplx);
    void ensure_samples(long total, int J);
    void plan_windows(int window);
    void dev_stft();
    void dev_masks(unsigned targets);
    void dev_wiener(int J, int iterations);
    void dev_phase(int J);
    void dev_istft(int J);
    float elapsed(int a, int b);
    int device_, hidden_;
    size_t max_samples_, param_bytes_ = 0, stem_stride_ = 0;
    bool loaded_ = true;
    int recur_form_ = 0;
    hipStream_t own_ = nullptr, work_ = nullptr;
    hipEvent_t ev_[5] = {};
    Plan p_;
    int n_win_ = 0;
    DevBuf d_w_, d_tab_;                            // the four stems' weights (device layouts), window + twiddles
    DevBuf d_meta_, d_rowfile_, d_win_;             // per-file n | off | T | row0 (long), row -> file, windows (row0, len) + row -> window
    DevBuf d_pcm_, d_re_, d_im_, d_mag_, d_mask_, d_yre_, d_yim_, d_x1_, d_pre_, d_h_[2], d_f2_, d_cov_, d_scale_, d_audio_;
    long cap_rows_ = 0, cap_net_ = 0, cap_cplx_ = 0, cap_samples_ = 0, cap_audio_ = 0, cap_win_ = 0, cap_files_ = 0, cap_mask_ = 0, cap_nwin_ = 0;
    SepTiming timing_;
};

}  // namespace qasr
