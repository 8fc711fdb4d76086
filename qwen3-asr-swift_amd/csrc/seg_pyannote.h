// seg_pyannote.h -- pyannote PyanNet segmentation on the device (kernels and host object in seg_pyannote.hip, C ABI in api_seg.cpp,
// the pipelines' host logic in diarize.cpp).
//
// Reference: Sources/SpeechVAD/Segmentation.swift:17-97 (SegmentationModel), SincNet.swift:15-129 (front end, InstanceNorm, maxPool1d,
// leakyRelu), BiLSTM.swift:9-100 (LSTMLayer, runBiLSTM), PowersetDecoder.swift:23-31, PyannoteVAD+Memory.swift.
// Per window of n samples: InstanceNorm(1) | Conv1d(1->80, k 251, s 10) |.| MaxPool 3 InstanceNorm LeakyReLU | Conv1d(80->60, k 5) pool
// norm leaky | Conv1d(60->60, k 5) pool norm leaky | 4 x BiLSTM(H 128) | Linear 256->128 leaky | Linear 128->128 leaky | Linear 128->7 |
// softmax | speaker probabilities, speech probability.  f32 throughout.
#pragma once
#include "engine.h"
#include "safetensors.h"
#include <string>
#include <vector>

namespace qasr {

constexpr int SEG_RATE = 16000, SEG_H = 128, SEG_G = 512, SEG_LAYERS = 4, SEG_CLASSES = 7, SEG_SPK = 3;
constexpr int SEG_C0 = 80, SEG_C1 = 60, SEG_K0 = 251, SEG_S0 = 10, SEG_K1 = 5, SEG_MIN_SAMPLES = 991;

// frame counts of every stage for n samples (all divisions floored); F < 1 below 991 samples
struct SegGeom { int L0, P0, L1, P1, L2, F; };
inline SegGeom seg_geom(long n) {
    SegGeom g{0, 0, 0, 0, 0, 0};
    if (n < SEG_K0) return g;
    g.L0 = (int)((n - SEG_K0) / SEG_S0) + 1;
    g.P0 = g.L0 / 3;
    g.L1 = g.P0 - 4;
    g.P1 = g.L1 > 0 ? g.L1 / 3 : 0;
    g.L2 = g.P1 - 4;
    g.F = g.L2 > 0 ? g.L2 / 3 : 0;
    return g;
}
inline int seg_num_frames(size_t n) { return n < (size_t)SEG_MIN_SAMPLES || n > ((size_t)1 << 30) ? -1 : seg_geom((long)n).F; }

// key -> shape of every tensor the network reads (MLX layouts: conv [out][k][in]); the keys of `seg_optional_keys` may be absent and
// then take the reference's deterministic initial value (Conv1d bias 0 is never reached: MLX initialises it to zeros; InstanceNorm
// weight ones, bias zeros: SincNet.swift:85-86)
const std::vector<std::pair<std::string, std::vector<int64_t>>>& seg_tensor_shapes();
// value a missing optional key takes, or a negative number when the key is required
float seg_optional_default(const std::string& key);

class SegPyannote {
  public:
    // work: the stream the model's work is ordered on (an engine's stream), nullptr = a stream of its own
    SegPyannote(int device, const CheckedWeights& w, int max_windows, hipStream_t work);
    ~SegPyannote();
    // W windows of n samples each, window w reading pcm[starts[w] .. starts[w] + n) with samples at or past `total` read as zero.
    // The buffer is uploaded once; more than max_windows windows run as several passes.  Any output may be NULL.
    void run(const float* pcm, size_t total, const long* starts, size_t W, size_t n, float* posteriors, float* speaker_probs,
             float* speech_probs);
    void unload();
    bool loaded() const { return loaded_; }
    size_t footprint() const { return loaded_ ? param_bytes_ : 0; }
    float last_ms() const { return last_ms_; }
    int max_windows() const { return max_windows_; }
    hipStream_t stream() const { return work_; }
    int device() const { return device_; }

  private:
    void ensure(size_t total, size_t n);
    void pass(int B, const SegGeom& g, int n, long total, hipStream_t s);
    int device_, max_windows_;
    size_t param_bytes_;
    bool loaded_ = true;
    hipStream_t own_ = nullptr, work_ = nullptr;
    hipEvent_t ev_[2] = {};
    DevBuf d_w_;                                    // every weight, device layouts (offsets in seg_pyannote.hip)
    DevBuf d_pcm_, d_off_, d_stat_, d_p0_, d_p1_, d_p2_, d_pre_, d_h_[2], d_out_;
    HostBuf h_off_, h_out_;
    size_t cap_total_ = 0, cap_n_ = 0;
    float last_ms_ = 0.f;
};

}  // namespace qasr
