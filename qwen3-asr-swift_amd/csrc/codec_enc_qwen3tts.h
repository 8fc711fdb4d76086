// codec_enc_qwen3tts.h -- the Qwen3-TTS 12.5 Hz speech tokenizer encoder on the device (kernels and host object in codec_enc_qwen3tts.hip,
// C ABI in api_codec_enc.cpp): 24 kHz mono PCM -> 16 code streams, the other direction of codec_qwen3tts.h.
//
// Reference: Sources/Qwen3TTS/SpeechTokenizerEncoder.swift:223-241 (callAsFunction), :12-70 (residual unit, encoder block), :77-103
// (EncoderTransformer: no mask, output_proj not applied), :109-135 (EncoderRVQ.encode: both quantizers see the same latent);
// SpeechTokenizerDecoder.swift:414-424 (nearest code in the expanded form), :467-485 (ResidualVectorQuantizer.encode), :11-47
// (CausalConv1d); TTSWeightLoading+Encoder.swift (the encoder.* keys).
// Per clip of n samples: conv k7 1 -> C/16 -> 4 x (3 residual units of dilation 1 3 9, SnakeBeta, strided conv k = 2 s, s = 3 4 5 8)
// -> conv k7 to latent -> 2 x (ConvNeXt, strided conv k4 s2) -> conv k3 -> Linear | layers x (RMSNorm, RoPE attention over the whole
// clip, layer scale, SwiGLU, layer scale) | RMSNorm -> per quantizer: projection, then per codebook nearest code and residual update.
// Every conv is causal inside its clip; lengths are ceilings at every rate.  f32 throughout.
#pragma once
#include "codec_qwen3tts.h"

namespace qasr {

constexpr int CENC_LEVELS = 7, CENC_STAGES = 8, CENC_MAX_CLIPS = 1024;
constexpr long CENC_DEFAULT_SAMPLES = 720000, CENC_MAX_SAMPLES = 1L << 24;

// key -> shape of every tensor the encoder reads (encoder.*); embed_stored as for codec_tensor_shapes
CodecShapes codec_enc_tensor_shapes(const CodecGeom& g, const std::vector<bool>& embed_stored);
// the six strides in the order they are applied: upsample_rates reversed, then upsampling_ratios reversed
void codec_enc_strides(const CodecGeom& g, int s[6]);
// rows of a clip of n samples at every rate: len[0] = n, len[l + 1] = ceil(len[l] / stride[l]); len[6] = frames
void codec_enc_lengths(const CodecGeom& g, long n, long len[CENC_LEVELS]);

struct CodecEncClip { const float* pcm; long n; int32_t* codes; float* out; };   // codes [Q][frames] or out [frames][width], by mode

class CodecEncQwen3TTS {
  public:
    enum Mode { ENCODE, CONV, LATENT };
    CodecEncQwen3TTS(int device, const CheckedWeights& w, const CodecGeom& g, const std::vector<bool>& embed_stored, long max_samples,
                     hipStream_t work);
    ~CodecEncQwen3TTS();
    // any number of clips, cut into passes at clip boundaries; a clip over max_samples is std::invalid_argument
    void run(const std::vector<CodecEncClip>& clips, Mode mode);
    void quantize(const float* h, long F, int32_t* codes);                           // [F][hidden] -> [Q][F]
    void unload();
    bool loaded() const { return loaded_; }
    size_t footprint() const { return loaded_ ? param_bytes_ : 0; }
    const CodecGeom& geom() const { return g_; }
    long max_samples() const { return max_samples_; }
    const float* timing() const { return timing_; }                                 // ms per stage of the last call (CENC_STAGES)
    hipStream_t stream() const { return work_; }

  private:
    using Gemm = CodecGemm;
    using Snake = CodecSnake;
    struct Down { Gemm pw1, pw2, sconv; size_t dw, dwb, lnw, lnb, gamma; };
    struct Block { CodecUnit u[3]; Snake s; Gemm sconv; };
    void check_loaded() const;
    void pass(const CodecEncClip* c, int n, Mode mode);
    void plan(const CodecEncClip* c, int n);
    void dev_convs();
    void dev_transformer();
    void dev_rvq(long F);
    void fetch_codes(long F, long row0, long frames, int32_t* codes);
    // level: the rate of the output rows; in_level: that of the input rows (a strided conv reads the level above it); -1: rows are independent
    template <bool SNAKE, int EPI>
    void gemm(const Gemm& g, const float* A, long M, int dil, int stride, int level, int in_level, const Snake* sn, const float* ls,
              const float* R, float* C, int ldc);
    const float* W(size_t off) const { return d_w_.as<float>() + off; }
    const int* starts(int level) const { return d_start_.as<int>() + (size_t)level * (CENC_MAX_CLIPS + 1); }
    int device_;
    CodecGeom g_;
    long max_samples_;
    int stride_[6], width_[CENC_LEVELS];
    long rows_cap_[CENC_LEVELS];
    size_t param_bytes_ = 0;
    bool loaded_ = true;
    hipStream_t own_ = nullptr, work_ = nullptr;
    hipEvent_t ev_[CENC_STAGES + 1] = {};
    float timing_[CENC_STAGES] = {};
    // weights (offsets in floats into d_w_)
    size_t in_w_ = 0, in_b_ = 0, norm_ = 0, rope_ = 0, cb_[2] = {}, cbt_[2] = {}, csq_[2] = {};
    Gemm enc5_, post_conv_, in_proj_, rvq_;
    Block blocks_[4];
    Down down_[2];
    std::vector<CodecLayer> layers_;
    // the pass
    int n_clips_ = 0, n_tiles_ = 0;
    long M_[CENC_LEVELS] = {};
    std::vector<int> h_start_, h_tiles_;
    std::vector<float> h_pcm_;
    std::vector<int32_t> h_codes_;
    DevBuf d_w_, d_start_, d_tiles_, d_pcm_, d_big_[3], d_x_, d_h_, d_qkv_, d_att_, d_g_, d_r_, d_codes_;
    float* conv_out_ = nullptr;                                                     // post_conv's output inside d_big_
};

}  // namespace qasr
