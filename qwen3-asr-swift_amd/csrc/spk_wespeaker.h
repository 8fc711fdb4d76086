// spk_wespeaker.h -- WeSpeaker ResNet34 speaker embeddings on the device (kernels and host object in spk_wespeaker.hip, the convolution
// family in spk_conv.h, C ABI in api_spk.cpp).
//
// Reference: Sources/SpeechVAD/WeSpeaker.swift (embed, cosineSimilarity), WeSpeakerModel.swift (BN-fused ResNet34),
// MelFeatureExtractor.swift (80-bin fbank + CMN), WeSpeakerWeightLoading.swift (model.safetensors, MLX layouts, .noUnusedKeys),
// WeSpeaker+Memory.swift (isLoaded / unload / memoryFootprint).
// Per clip: pre-emphasis 0.97 | reflect pad 200 | 400-sample symmetric Hamming frames, hop 160, 512-point power x 4 | HTK mel 80 (20 Hz ..
// 8 kHz, slaney-normalised) | log(max(x, 1e-10)) | CMN | conv1 1->32 + 16 BasicBlocks (32, 64, 128, 256 channels; F 80 -> 40 -> 20 -> 10)
// | mean ++ std over time (C*F order) | Linear 5120 -> 256 | L2 normalise.
#pragma once
#include "engine.h"
#include "safetensors.h"
#include <map>
#include <string>
#include <vector>

namespace qasr {

constexpr int SPK_RATE = 16000, SPK_NMELS = 80, SPK_HOP = 160, SPK_WIN = 400, SPK_DIM = 256, SPK_POOL = 5120;
constexpr int SPK_COL_ALIGN = 8;        // clips sit at multiples of 8 time columns with >= 8 zero guard columns between them (level 0)

__host__ __device__ inline int spk_num_frames(size_t n) { return (int)(n / SPK_HOP) + 1; }

// key -> shape of every tensor the network reads (WeSpeakerModel.swift)
// (MLX layouts); load_checked_f32 checks a checkpoint against it, unknown keys refused, with no HIP call
const std::vector<std::pair<std::string, std::vector<int64_t>>>& spk_tensor_shapes();

class WeSpeaker {
  public:
    // work: the stream the model's work is ordered on (an engine's stream), nullptr = a stream of its own.
    // max_samples: PCM samples one device pass holds (the workspace is sized from it).
    WeSpeaker(int device, const CheckedWeights& w, size_t max_samples, hipStream_t work);
    ~WeSpeaker();
    // B clips -> out [B][256]; calls larger than the workspace run as several passes; a clip longer than max_samples: std::length_error
    void embed(const float* const* pcm, const size_t* n, size_t B, float* out);
    // front end only: post-CMN [T_b][80] per clip at feats + b * stride
    void fbank(const float* const* pcm, const size_t* n, size_t B, float* feats, size_t stride, int32_t* n_frames);
    void unload();
    bool loaded() const { return loaded_; }
    size_t footprint() const { return loaded_ ? param_bytes_ : 0; }
    float last_ms() const { return last_ms_; }

  private:
    struct Pass { size_t first, count, samples; int frames, cols; };
    std::vector<Pass> plan(const size_t* n, size_t B) const;
    void stage(const float* const* pcm, const size_t* n, const Pass& p);
    void front(const Pass& p, hipStream_t s);
    void network(const Pass& p, hipStream_t s);
    int device_;
    size_t max_samples_, cap_frames_, cap_cols_, cap_clips_;
    size_t param_bytes_;
    bool loaded_ = true;
    hipStream_t own_ = nullptr, work_ = nullptr;
    hipEvent_t ev_[2] = {};
    DevBuf d_tab_, d_wconv_, d_wstem_, d_bias_, d_wlin_;
    DevBuf d_pcm_, d_meta_, d_raw_, d_feat_, d_act_[3], d_emb_;
    HostBuf h_pcm_, h_meta_, h_out_;
    float last_ms_ = 0.f;
};

}  // namespace qasr
