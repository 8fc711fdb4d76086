// codec_launch.hip -- the launch entries of codec_launch.h: the one place codec_gemm_kernel, codec_rms_kernel and codec_dwln_kernel
// (codec_shared.h) are instantiated and launched.
#include "codec_shared.h"
#include <stdexcept>

namespace qasr {

namespace {

template <class Rows> struct RowsKind;
template <> struct RowsKind<WindowRows> {
    static constexpr int kind = CODEC_ROWS_WINDOW;
    static WindowRows make(const CodecRowsArg& r) { return WindowRows{r.a, r.rate}; }
};
template <> struct RowsKind<TailRows> {
    static constexpr int kind = CODEC_ROWS_TAIL;
    static TailRows make(const CodecRowsArg& r) { return TailRows{r.a, r.b, r.rate, r.lead}; }
};
template <> struct RowsKind<ClipRows> {
    static constexpr int kind = CODEC_ROWS_CLIP;
    static ClipRows make(const CodecRowsArg& r) { return ClipRows{r.a, r.b, r.n_clips, r.stride}; }
};
template <> struct RowsKind<VaeStrideRows> {
    static constexpr int kind = CODEC_ROWS_VAE_STRIDE;
    static VaeStrideRows make(const CodecRowsArg& r) { return VaeStrideRows{r.a, r.rate, r.stride}; }
};

}  // namespace

bool codec_tile_served(int kind, bool snake, int epi) {
#define CODEC_SERVED(ROWS, SNAKE, EPI) \
    if (kind == RowsKind<ROWS>::kind && snake == SNAKE && epi == EPI) return true;
    CODEC_TILE_COMBOS(CODEC_SERVED)
#undef CODEC_SERVED
    return false;
}

void codec_tile_launch(const CodecRowsArg& rows, bool snake, int epi, const float* A, long M, int Cin, int taps, int dil, const float* Wt, int K,
                       int N, const float* bias, int bmod, const float* sa, const float* sb, const float* ls, const float* R, float* C, int ldc,
                       hipStream_t s) {
    const dim3 grid((unsigned)cdiv(M, (long)CG_T), (unsigned)cdiv(N, CG_T));
#define CODEC_LAUNCH(ROWS, SNAKE, EPI)                                                                                                       \
    if (rows.kind == RowsKind<ROWS>::kind && snake == SNAKE && epi == EPI) {                                                                 \
        hipLaunchKernelGGL((codec_gemm_kernel<ROWS, SNAKE, EPI>), grid, dim3(CG_THREADS), 0, s, A, M, Cin, taps, dil, RowsKind<ROWS>::make(rows), \
                           Wt, K, N, bias, bmod, sa, sb, ls, R, C, ldc);                                                                     \
        return;                                                                                                                              \
    }
    CODEC_TILE_COMBOS(CODEC_LAUNCH)
#undef CODEC_LAUNCH
    throw std::invalid_argument("codec_tile_launch: no codec_gemm_kernel for this (row locator, snake, epilogue)");
}

void codec_rms_launch(const float* x, long M, int C, const float* w, float eps, float* y, hipStream_t s) {
    hipLaunchKernelGGL(codec_rms_kernel<>, dim3((unsigned)M), dim3(ROW_THREADS), 0, s, x, C, w, eps, y);
}

void codec_dwln_launch(const CodecRowsArg& rows, const float* x, long M, int C, const float* w, const float* b, const float* lnw, const float* lnb,
                       float* y, hipStream_t s) {
    if (C < 1 || C > 4096) throw std::invalid_argument("codec_dwln_launch: C in [1, 4096]");
    if (rows.kind == CODEC_ROWS_WINDOW)
        hipLaunchKernelGGL(codec_dwln_kernel<WindowRows>, dim3((unsigned)M), dim3(ROW_THREADS), 0, s, x, C, RowsKind<WindowRows>::make(rows), w, b,
                           lnw, lnb, y);
    else if (rows.kind == CODEC_ROWS_CLIP)
        hipLaunchKernelGGL(codec_dwln_kernel<ClipRows>, dim3((unsigned)M), dim3(ROW_THREADS), 0, s, x, C, RowsKind<ClipRows>::make(rows), w, b, lnw,
                           lnb, y);
    else
        throw std::invalid_argument("codec_dwln_launch: the depthwise conv runs under WindowRows or ClipRows");
}

}  // namespace qasr
