// vad_silero.h -- Silero VAD v5 on the device (kernels and host object in vad_silero.hip, C ABI in api_vad.cpp).
//
// Reference: Sources/SpeechVAD/SileroModel.swift:1-186 (network), SileroVAD.swift:1-321 (processChunk / resetState / detectSpeech),
// SileroWeightLoading.swift (model.safetensors, MLX layouts), VADPipeline.swift:117-181 (binarize + filterDurations).
// Per stream and 512-sample chunk: 64 context samples ++ 512 | right reflection pad 64 | STFT conv (258 x 256, stride 128) -> 4 x 129
// magnitudes | 4 x (Conv1d k3 + ReLU): 129->128 s1, 128->64 s2, 64->64 s2, 64->128 s1 | LSTM cell H=128 (i, f, g, o) | sigmoid(decoder(relu h)).
#pragma once
#include "engine.h"
#include "safetensors.h"
#include <map>
#include <string>
#include <vector>

namespace qasr {

constexpr int VAD_CHUNK = 512, VAD_CTX = 64, VAD_H = 128, VAD_G = 512, VAD_RATE = 16000;

// key -> shape of every tensor the network reads (SileroModel.swift:22-28,44-66)
// (conv weights [out, k, in], lstm.Wx / Wh [512, 128]); load_checked_f32 checks a checkpoint against it with no HIP call
const std::vector<std::pair<std::string, std::vector<int64_t>>>& silero_tensor_shapes();

struct VadConfig { float onset, offset, min_speech, min_silence; };
struct VadSegment { float start, end; };
// VADPipeline.binarize with the frame duration detectSpeech sets up (windowDuration = n * 0.032, frameDuration = windowDuration / n, f32)
std::vector<VadSegment> silero_binarize(const float* probs, size_t n, const VadConfig& cfg);

class SileroVad {
  public:
    // work: the stream the VAD's work is ordered on (an engine's stream), nullptr = a stream of its own
    SileroVad(int device, const CheckedWeights& w, int max_streams, hipStream_t work);
    ~SileroVad();
    void reset(int stream);                                                     // stream < 0: every stream
    // processChunk for B distinct streams: chunks [B][512] -> probs [B]
    void process(const float* chunks, const int32_t* stream_ids, size_t B, float* probs);
    // detectSpeech's probability loop for B buffers (row stream reset first, final state left there); probs [B][stride]
    void probs(const float* const* pcm, const size_t* n, size_t B, const int32_t* stream_ids, float* probs, size_t stride, int32_t* n_chunks);
    void state(int stream, float* h, float* c, float* ctx);
    int device() const { return device_; }
    int max_streams() const { return max_streams_; }
    float last_ms() const { return last_ms_; }
    bool last_was_graph() const { return last_graph_; }

  private:
    void ensure(size_t B, size_t samples, size_t chunks);
    void issue(int B, int total_chunks, size_t samples, hipStream_t s);
    void run(int B, int total_chunks, size_t samples, bool tick);
    void drop_graphs();
    int device_, max_streams_;
    hipStream_t own_ = nullptr, work_ = nullptr;
    hipEvent_t ev_[2] = {};
    DevBuf d_w_;                                    // every weight, device layouts (offsets in vad_silero.hip)
    DevBuf d_h_, d_c_, d_ctx_;                      // per-stream state [S][128], [S][128], [S][64]
    DevBuf d_pcm_, d_meta_, d_pre_, d_prob_;
    HostBuf h_pcm_, h_meta_, h_prob_;
    size_t cap_rows_ = 0, cap_samples_ = 0, cap_chunks_ = 0;
    float dec_b_ = 0.f;
    float last_ms_ = 0.f;
    bool last_graph_ = false;
    std::map<int, hipGraphExec_t> graphs_;          // tick graphs per B
};

}  // namespace qasr
