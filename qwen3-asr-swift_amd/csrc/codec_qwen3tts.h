// codec_qwen3tts.h -- the Qwen3-TTS 12.5 Hz speech tokenizer decoder on the device (kernels and host object in codec_qwen3tts.hip, C ABI
// in api_codec.cpp): 16 code streams -> 24 kHz waveform.
//
// Reference: Sources/Qwen3TTS/SpeechTokenizerDecoder.swift:658-688 (callAsFunction), :696-736 (chunkedDecode), :739-752 (decode,
// decodeBatch), :513-521 (split RVQ decode), :368-391 (DecoderTransformer), :156-165 (ConvNeXtBlock), :190-228 (residual unit, decoder
// block), :92-111 (SnakeBeta); Configuration.swift:128-148 (SpeechTokenizerDecoderConfig); TTSWeightLoading.swift:190-301, :347-381,
// :458-480 (checkpoint keys, codebook from embedding_sum / cluster_usage).
// Per window of T <= 35 frames: RVQ gather-sum + projections -> pre_conv k3 -> Linear | layers x (RMSNorm, RoPE causal attention, layer
// scale, SwiGLU, layer scale) | RMSNorm, Linear -> 2 x (transposed conv x2, ConvNeXt) -> conv k7 -> 4 x (SnakeBeta, transposed conv
// x8 x5 x4 x3, 3 residual units of dilation 1 3 9) -> SnakeBeta, conv k7 to one channel, clip.  Every conv is causal inside its window.
// f32 throughout.
#pragma once
#include "codec_shared.h"

namespace qasr {

constexpr int CODEC_RATE = 24000, CODEC_MAX_T = 35, CODEC_CHUNK = 25, CODEC_CONTEXT = 10, CODEC_STAGES = 8;

// model_dir/config.json's "decoder_config" over the defaults (api_codec.cpp); throws WeightLoadError with messages starting "<who>: "
CodecGeom codec_read_geometry(const std::string& dir, const char* who);
// key -> shape of every tensor the decoder reads; embed_stored[q]: codebook q (0 = rvq_first) is stored under `embed`, else under
// embedding_sum + cluster_usage
CodecShapes codec_tensor_shapes(const CodecGeom& g, const std::vector<bool>& embed_stored);
// chunkedDecode's windows (:696-733): frames starts[i] .. ends[i] are decoded, the first context[i] of them dropped
struct CodecSpan { int start, context, end; };
std::vector<CodecSpan> codec_window_positions(long T);

struct CodecWin { const int32_t* codes; long ld; int start, frames, context; float* out; };   // codes [Q][ld]; out: (frames - context) x spf

class CodecQwen3TTS {
  public:
    CodecQwen3TTS(int device, const CheckedWeights& w, const CodecGeom& g, const std::vector<bool>& embed_stored, int max_windows,
                  hipStream_t work);
    ~CodecQwen3TTS();
    // any number of windows, max_windows per pass.  tail: the windows are decoded for what they keep -- under the knob codec_tail_rows the
    // vocoder skips the rows only the dropped context needs (the same bits)
    void run(const std::vector<CodecWin>& wins, bool clip, bool tail = false);
    void quantizer_decode(const int32_t* codes, int B, int T, float* out);          // codes [B][Q][T] -> [B][T][hidden]
    void pre_transformer(const float* x, int B, int T, float* out);                 // [B][T][latent] -> [B][T][latent]
    void unload();
    bool loaded() const { return loaded_; }
    size_t footprint() const { return loaded_ ? param_bytes_ : 0; }
    const CodecGeom& geom() const { return g_; }
    const float* timing() const { return timing_; }                                 // ms per stage of the last call (CODEC_STAGES)
    hipStream_t stream() const { return work_; }

  private:
    using Gemm = CodecGemm;
    using Snake = CodecSnake;
    struct Up { Gemm tconv, pw1, pw2; size_t dw, dwb, lnw, lnb, gamma; };
    struct Block { Snake s; Gemm tconv; CodecUnit u[3]; };
    enum Mode { FULL, RVQ, PT };
    void check_loaded() const;
    void ensure(long M1, Mode mode);
    void pass(const CodecWin* w, int n, Mode mode, bool clip, const float* xin, float* xout, bool tail = false);
    void plan(const CodecWin* w, int n, bool with_codes);
    void dev_rvq();
    void dev_pre_transformer();
    void dev_vocoder(bool clip, bool tail);
    template <bool SNAKE, int EPI>
    void gemm(const Gemm& g, const float* A, long M, int dil, int rate, const Snake* sn, const float* ls, const float* R, float* C, int ldc, int bmod,
              int lead = -1);                                                       // lead >= 0: TailRows with that lead
    const float* W(size_t off) const { return d_w_.as<float>() + off; }
    int device_;
    CodecGeom g_;
    int max_windows_, spf_;
    size_t param_bytes_ = 0, big_per_frame_ = 0;
    bool loaded_ = true;
    hipStream_t own_ = nullptr, work_ = nullptr;
    hipEvent_t ev_[CODEC_STAGES + 1] = {};
    float timing_[CODEC_STAGES] = {};
    // weights (offsets in floats into d_w_)
    size_t cb_first_ = 0, rope_ = 0, final_w_ = 0, final_b_ = 0, norm_ = 0;
    Gemm rvq_, pre_conv_, in_proj_, out_proj_, dec0_;
    std::vector<CodecLayer> layers_;
    Up up_[2];
    Block blocks_[4];
    Snake final_snake_;
    // the pass
    long M1_ = 0;
    int n_win_ = 0;
    DevBuf d_w_, d_codes_, d_fstart_, d_kept_, d_win_, d_emb_, d_q_, d_lat_[2], d_x_, d_h_, d_qkv_, d_att_, d_g_, d_big_[3], d_wave_;
    long cap_small_ = 0, cap_big_ = 0, cap_win_ = 0;
    std::vector<int32_t> h_codes_;
};

// How many input rows before the first kept one each stage of the vocoder needs so that every kept sample is what the whole window gives:
// leads[0] the input of decoder.decoder.0, leads[1 .. 4] the inputs of blocks 1 .. 4, leads[5] the input of the output conv, each at its own
// rate.  From the output backwards: 6 for the k = 7 output conv; a block of stride s whose output needs `out` rows needs
// ceil((out + 6 (1 + 3 + 9)) / s) + 1 (three k = 7 units of dilation 1 3 9, then the transposed conv's previous-row tap); decoder.decoder.0
// adds its own 6.  The real rates 8 5 4 3 give 20 14 23 28 29 6.  Pure host.
void codec_tail_leads(const int rates[4], int leads[6]);

// windows handed over by another handle kind of this library (the TTS stream pool, api_tts.cpp): the checks of qasr_codec_forward on
// every window (loaded, 1 .. 35 frames, every code inside its codebook), then one run(); status and message as the C ABI (api_codec.cpp)
int codec_run_windows(qasr_codec* c, const std::vector<CodecWin>& wins, bool clip);

}  // namespace qasr
