// codec_launch.h -- the launch entries of the kernels in codec_shared.h (defined in codec_launch.hip): the f32 tile behind its four row
// locators, RMSNorm, and the depthwise conv + LayerNorm; and of the decoder's code gather and output conv and the encoder's input conv and quantiser
// (defined beside those kernels).  CodecQwen3TTS, CodecEncQwen3TTS, AudioVaeVoxcpm and qasr_codec_case_probe
// (codec_cases.hip) all launch through these, so the probe runs exactly the instantiations the product runs.  Device pointers and a
// stream only; nothing here knows a model.
#pragma once
#include <hip/hip_runtime.h>

namespace qasr {

enum { E_LIN = 0, E_GELU = 1, E_RES = 2, E_LSRES = 3, E_SWIGLU = 4, E_RESMAP = 5 };
enum { CODEC_ROWS_WINDOW = 0, CODEC_ROWS_TAIL = 1, CODEC_ROWS_CLIP = 2, CODEC_ROWS_VAE_STRIDE = 3 };

// Every (Rows, SNAKE, EPI) of codec_gemm_kernel that exists.  codec_tile_launch instantiates these and refuses any other;
// tests/test_codec_cases_cpu.py reads this list and asserts that each one is launched by a case of tests/codec_cases.py.
//   decoder: WindowRows and, from decoder.decoder.0 on in a streamed pass, TailRows; encoder: ClipRows; AudioVAE: WindowRows, VaeStrideRows
#define CODEC_TILE_COMBOS(X)          \
    X(WindowRows, false, E_LIN)       \
    X(WindowRows, false, E_GELU)      \
    X(WindowRows, false, E_RES)       \
    X(WindowRows, false, E_LSRES)     \
    X(WindowRows, false, E_SWIGLU)    \
    X(WindowRows, false, E_RESMAP)    \
    X(WindowRows, true, E_LIN)        \
    X(WindowRows, true, E_RES)        \
    X(TailRows, false, E_LIN)         \
    X(TailRows, true, E_LIN)          \
    X(TailRows, true, E_RES)          \
    X(ClipRows, false, E_LIN)         \
    X(ClipRows, false, E_GELU)        \
    X(ClipRows, false, E_LSRES)       \
    X(ClipRows, false, E_SWIGLU)      \
    X(ClipRows, true, E_LIN)          \
    X(ClipRows, true, E_RES)          \
    X(VaeStrideRows, false, E_LIN)

// what a row locator is built from (codec_shared.h).  a | b: WindowRows fstart | -; TailRows fstart | kept; ClipRows ostart | istart (both
// null: independent rows); VaeStrideRows fstart | -.  rate: Window, Tail, VaeStride; lead: Tail; n_clips: Clip; stride: Clip, VaeStride.
struct CodecRowsArg {
    int kind = CODEC_ROWS_WINDOW;
    const int *a = nullptr, *b = nullptr;
    int rate = 1, lead = 0, n_clips = 0, stride = 1;
};

// whether CODEC_TILE_COMBOS holds (rows kind, snake, epi)
bool codec_tile_served(int kind, bool snake, int epi);

// one launch of codec_gemm_kernel<Rows, SNAKE, EPI> on a grid of (M / 64, N / 64) tiles, rounded up; the arguments are the kernel's.
// throws std::invalid_argument for a combination outside CODEC_TILE_COMBOS
void codec_tile_launch(const CodecRowsArg& rows, bool snake, int epi, const float* A, long M, int Cin, int taps, int dil, const float* Wt, int K,
                       int N, const float* bias, int bmod, const float* sa, const float* sb, const float* ls, const float* R, float* C, int ldc,
                       hipStream_t s);

// codec_rms_kernel over rows 0 .. M - 1
void codec_rms_launch(const float* x, long M, int C, const float* w, float eps, float* y, hipStream_t s);

// codec_dwln_kernel<WindowRows | ClipRows> over rows 0 .. M - 1; C <= 4096.  throws std::invalid_argument for another locator or a wider C
void codec_dwln_launch(const CodecRowsArg& rows, const float* x, long M, int C, const float* w, const float* b, const float* lnw, const float* lnb,
                       float* y, hipStream_t s);

// codec_gather_kernel (codec_qwen3tts.hip): codes [M][Q], every code inside its codebook; cb = codebook 0 [S0][D], then Q - 1 of [S1][D];
// out [M][2 D]
void codec_gather_launch(const int* codes, long M, int Q, int D, long S0, long S1, const float* cb, float* out, hipStream_t s);

// codec_out_kernel<tail> (codec_qwen3tts.hip): x [M][C] -> wave [M]; fstart / kept [M / rate] as WindowRows / TailRows; w [7][C], b [1]
void codec_out_launch(bool tail, const float* x, long M, int C, int rate, const int* fstart, const int* kept, const float* sa, const float* sb,
                      const float* w, const float* b, int clip, float* wave, hipStream_t s);

// cenc_in_kernel (codec_enc_qwen3tts.hip): pcm [M] -> y [M][C]; start [nclips + 1] from 0 to M, strictly increasing; w [7][C], b [C]
void cenc_in_launch(const float* pcm, long M, int C, const int* start, int nclips, const float* w, const float* b, float* y, hipStream_t s);

// cenc_vq_kernel (codec_enc_qwen3tts.hip): r [M][ldr] read and written (chain 0 in columns 0 .. D - 1, chain 1 in D .. 2 D - 1); cb [stage][S][D],
// cbt [stage][D][S], csq [stage][S] (chain 0: one stage of S0; chain 1: Q - 1 stages of S1); codes [M][Q]
void cenc_vq_launch(float* r, long M, int ldr, int D, int Q, const float* cb0, const float* cbt0, const float* csq0, int S0, const float* cb1,
                    const float* cbt1, const float* csq1, int S1, int* codes, hipStream_t s);

// codec_attn_kernel (codec_qwen3tts.hip): causal attention inside each window, head_dim 64.  qkv [M][3 heads 64]; win [n_win] pairs (frames <=
// CODEC_MAX_T, first row); rope [>= frames][32] pairs (cos, sin); out [M][heads 64]
void codec_attn_launch(const float* qkv, const int* win, int n_win, const float* rope, int heads, float* out, hipStream_t s);

// cenc_attn_kernel (codec_enc_qwen3tts.hip): full attention inside each clip, head_dim 64.  tiles [n_tiles] quadruples (the clip's first row, its
// frames, the tile's first query, unused): one per 32 queries of a clip; rope [>= frames][32] pairs (cos, sin)
void cenc_attn_launch(const float* qkv, const int* tiles, int n_tiles, const float* rope, int heads, float* out, hipStream_t s);

// vae_dw_kernel<snakes, snakes> (vae_voxcpm.hip): x, y [M][C]; fstart [M / rate] as WindowRows; w [7][C], b [C]; a1, i1, a2, i2 [C] under snakes;
// dynamic LDS (64 + 6 dil) x 64 floats
void vae_dw_launch(bool snakes, const float* x, long M, int C, int dil, const int* fstart, int rate, const float* w, const float* b, const float* a1,
                   const float* i1, const float* a2, const float* i2, float* y, hipStream_t s);

// vae_unit_kernel<RPT> (vae_voxcpm.hip), RPT by the rule of the entry: a whole residual unit.  x, y [M][C] (y is not x), C a multiple of 4 up to
// AV_FUSE_MAX, dil <= 9; w1 [7][C], b1, a1, i1, a2, i2 [C]; Wt [C][C], b2 [C]; the reader's map ma, mi [C] (null: none) and aff [2 C] (null: no
// affine); every pointer 16-byte aligned.  throws std::invalid_argument for another C or dil
void vae_unit_launch(const float* x, long M, int C, int dil, const int* fstart, int rate, const float* w1, const float* b1, const float* a1,
                     const float* i1, const float* a2, const float* i2, const float* Wt, const float* b2, const float* ma, const float* mi,
                     const float* aff, float* y, hipStream_t s);

}  // namespace qasr
