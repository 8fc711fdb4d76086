// xvec_qwen3tts.h -- the Qwen3-TTS ECAPA-TDNN speaker encoder on the device (kernels and host object in xvec_qwen3tts.hip, C ABI in
// api_xvec.cpp): 24 kHz mono PCM of a voice-cloning reference clip -> one x-vector of E floats (E = fc.weight's rows, 1024 in the reference).
//
// Reference: Sources/Qwen3TTS/SpeakerEncoder.swift:245-388 (SpeakerMel.compute: reflect pad 512 with clamped indices, periodic Hann 1024,
// 1024-point DFT magnitudes at hop 256, 128 unnormalised HTK triangles 0 .. 12 kHz, log(max(., 1e-5))), :176-238 (SpeakerEncoder), :72-100
// (ECAPABlock), :34-68 (Res2NetBlock), :10-30 (SEBlock), :107-149 (AttentiveStatisticsPooling); TTSWeightLoading.swift:385-453 (keys).
// Per clip of T = n / 256 + 1 frames: conv k5 128 -> 512, ReLU | 3 x (1 x 1 ReLU, Res2Net of seven k3 dilated 64 -> 64 convs, 1 x 1 ReLU,
// squeeze-excitation over the clip's mean, + input) with dilation 2 3 4 | 1 x 1 over the three outputs side by side, ReLU | attentive
// statistics pooling | Linear 3072 -> E.  Every conv pads with zeros inside its clip.  f32 throughout.
#pragma once
#include "engine.h"
#include "safetensors.h"
#include <string>
#include <vector>

namespace qasr {

constexpr int XV_RATE = 24000, XV_NFFT = 1024, XV_HOP = 256, XV_NMELS = 128, XV_NBINS = 513;
constexpr int XV_C = 512, XV_W = 64, XV_SE = 128, XV_ATT = 128, XV_CAT = 1536, XV_STAGES = 6, XV_MAX_CLIPS = 1024;
constexpr int XV_TILE = 64;            // rows of a GEMM / reduction tile; the grid of tiles starts at every clip's first row
constexpr int XV_RES_TILE = 64;        // rows a Res2Net workgroup owns (plus 7 x dilation rows of halo per side)
constexpr long XV_DEFAULT_SAMPLES = 64L * 10 * XV_RATE, XV_MAX_SAMPLES = 1L << 28;

inline long xvec_num_frames(long n) { return n > 0 ? n / XV_HOP + 1 : 0; }
// key -> shape of every tensor read, with the speaker_encoder. prefix; E: the embedding width
std::vector<std::pair<std::string, std::vector<int64_t>>> xvec_tensor_shapes(int64_t E);
// [513][128] as SpeakerEncoder.swift:354-387 builds it (Float arithmetic)
std::vector<float> xvec_filterbank();

struct XvecClip { const float* pcm; long n; float* mel; float* out; };     // mel [T][128] (MEL mode) or out [E] (EMBED mode)

class XvecQwen3TTS {
  public:
    enum Mode { EMBED, MEL };
    XvecQwen3TTS(int device, const CheckedWeights& w, int E, long max_samples, hipStream_t work);
    ~XvecQwen3TTS();
    // any number of clips, cut into passes at clip boundaries; a clip over max_samples is std::length_error
    void run(const std::vector<XvecClip>& clips, Mode mode);
    void embed_mel(const float* mel, long T, float* out);                           // the network alone on caller-supplied rows
    void unload();
    bool loaded() const { return loaded_; }
    size_t footprint() const { return loaded_ ? param_bytes_ : 0; }
    int embedding_dim() const { return E_; }
    long max_samples() const { return max_samples_; }
    const float* timing() const { return timing_; }                                 // ms per stage of the last call (XV_STAGES)
    hipStream_t stream() const { return work_; }

  private:
    struct Gemm { size_t wt = 0, bias = 0; int K = 0, N = 0, Cin = 0, taps = 1; };
    struct Block { Gemm tdnn1, tdnn2, se1, se2; size_t res_w = 0, res_b = 0; };
    void check_loaded() const;
    void pass(const XvecClip* c, int n, Mode mode);
    void plan(const long* frames, int n);
    void dev_mel();
    void dev_network();
    void finish(int last);
    template <int ACT, int STAT>
    void gemm(const Gemm& g, const float* A, int lda, float* C, int ldc, const float* ctx, float* part);
    const float* W(size_t off) const { return d_w_.as<float>() + off; }
    int device_, E_;
    long max_samples_, rows_cap_ = 0, tiles_cap_ = 0;
    size_t param_bytes_ = 0;
    bool loaded_ = true;
    hipStream_t own_ = nullptr, work_ = nullptr;
    hipEvent_t ev_[XV_STAGES + 1] = {};
    float timing_[XV_STAGES] = {};
    // weights and tables (offsets in floats into d_w_)
    size_t hann_ = 0, tw512_ = 0, tw1024_ = 0, fb_w_ = 0, ctx_w_ = 0;
    Gemm init_, mfa_, att1_, att2_, fc_;
    Block blocks_[3];
    // the pass
    int n_clips_ = 0, n_tiles_ = 0, n_res_tiles_ = 0;
    long M_ = 0;
    std::vector<int> h_start_, h_tiles_, h_tstart_, h_res_tiles_, h_n_;
    std::vector<long> h_off_;
    std::vector<float> h_pcm_;
    DevBuf d_w_, d_fb_, d_start_, d_tiles_, d_tstart_, d_res_tiles_, d_n_, d_off_, d_pcm_, d_mel_, d_h0_, d_t1_, d_r_, d_cat_, d_mfa_,
        d_att_, d_part_[6], d_ctx_, d_out_;                                          // d_fb_: the filterbank's start | len | off tables (int)
};

}  // namespace qasr
