// spk_conv.h -- implicit-GEMM 3x3 convolutions of the WeSpeaker ResNet34 (spk_wespeaker.hip) on v_mfma_f32_16x16x32_bf16.
//
// Activations are NHWC bf16 with one image per call: [F][W][C], H = frequency, W = the packed time axis of every clip of the batch.
// GEMM shape: M = F_out * W_out output pixels, N = CO output channels, K = 9 * CA (+ CX).  K index = (kh * 3 + kw) * CA + ci, which is
// the MLX weight layout [out][kh][kw][in] flattened; weights are [CO][K] bf16.  A downsampling block's conv2 appends the 1x1 stride-2
// shortcut as CX extra K columns (K = 9 * CA + CX, the shortcut weight [CO][CX] after the 3x3 taps) so the block ends in this one launch.
//
// One wave owns 64 pixels x NT * 16 channels (4 x NT MFMA tiles) and needs nothing from any other wave: no LDS, no barrier.  Every
// 32-deep K step lies inside one tap, so a lane's A fragment is 8 consecutive channels of one input pixel (one 16-byte load, zero
// outside the image) and its B fragment 8 consecutive K of one weight row.  The K order is fixed (taps 0..8, channels ascending, then
// the shortcut), so an output depends only on its own pixel's receptive field: where the pixel sits in the batch never enters.
// Epilogue in f32: + bias (+ the bf16-stored residual), ReLU, then every column outside a clip's valid range is written as 0, which
// keeps the guard columns between clips the zero padding a lone clip sees.  The residual may alias the output (it is read at the
// output's own element by the lane that writes it).
#pragma once
#include "common.h"

namespace qasr {

struct SpkConvArgs {
    const bf16_t* in;          // [F_in][W_in][CA]
    const bf16_t* sc;          // shortcut input = the block input [2 F_in][2 W_in][CX] (CX > 0), read at (2 fo, 2 wo)
    const bf16_t* w;           // [CO][K]
    const float* bias;         // [CO]
    const bf16_t* res;         // identity residual [F_out][W_out][CO] (RES)
    bf16_t* out;               // [F_out][W_out][CO]
    const unsigned char* colvalid;   // [W_out]
    int F_in, W_in, F_out, W_out;
};

constexpr int SPK_CONV_THREADS = 256;

typedef __attribute__((ext_vector_type(8))) __bf16 spk_bf16x8;      // the builtin's operand type (bit pattern, not a value conversion)

__device__ __forceinline__ spk_bf16x8 spk_ld8(const bf16_t* p) {
    return __builtin_bit_cast(spk_bf16x8, *reinterpret_cast<const uint4*>(p));
}

template <int CA, int S, int CX, bool RES, int CO>
__global__ __launch_bounds__(SPK_CONV_THREADS) void spk_conv_kernel(SpkConvArgs a) {
    constexpr int NT = CO < 64 ? CO / 16 : 4;            // N tiles of 16 per wave
    constexpr int K = 9 * CA + CX;
    static_assert(CA % 32 == 0 && CX % 32 == 0 && CO % 16 == 0, "channel multiples");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int M = a.F_out * a.W_out;
    const int m0 = (blockIdx.x * (SPK_CONV_THREADS / 64) + wave) * 64;
    if (m0 >= M) return;                                   // whole wave past the end (no barrier in this kernel)
    const int n0 = blockIdx.y * NT * 16;
    const int kq = (lane >> 4) * 8;
    const int col = lane & 15;

    int fo[4], wo[4];
    bool live[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = m0 + i * 16 + col;
        live[i] = m < M;
        fo[i] = live[i] ? m / a.W_out : 0;
        wo[i] = live[i] ? m - fo[i] * a.W_out : 0;
    }
    const bf16_t* wrow[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) wrow[j] = a.w + (long)(n0 + j * 16 + col) * K + kq;

    f32x4 acc[4][NT];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const spk_bf16x8 zero8 = __builtin_bit_cast(spk_bf16x8, make_uint4(0, 0, 0, 0));

    for (int tap = 0; tap < 9; ++tap) {
        const int kh = tap / 3, kw = tap - kh * 3;
        const bf16_t* src[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int fi = fo[i] * S + kh - 1, wi = wo[i] * S + kw - 1;
            const bool in = live[i] && fi >= 0 && fi < a.F_in && wi >= 0 && wi < a.W_in;
            src[i] = in ? a.in + ((long)fi * a.W_in + wi) * CA + kq : nullptr;
        }
#pragma unroll 2
        for (int c0 = 0; c0 < CA; c0 += 32) {
            spk_bf16x8 av[4], bv[NT];
#pragma unroll
            for (int i = 0; i < 4; ++i) av[i] = src[i] ? spk_ld8(src[i] + c0) : zero8;
#pragma unroll
            for (int j = 0; j < NT; ++j) bv[j] = spk_ld8(wrow[j] + tap * CA + c0);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[i], bv[j], acc[i][j], 0, 0, 0);
        }
    }
    if constexpr (CX > 0) {                                // 1x1 stride-2 shortcut: input pixel (2 fo, 2 wo), always inside the image
        const bf16_t* src[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) src[i] = live[i] ? a.sc + ((long)(2 * fo[i]) * a.W_in * 2 + 2 * wo[i]) * CX + kq : nullptr;
#pragma unroll
        for (int c0 = 0; c0 < CX; c0 += 32) {
            spk_bf16x8 av[4], bv[NT];
#pragma unroll
            for (int i = 0; i < 4; ++i) av[i] = src[i] ? spk_ld8(src[i] + c0) : zero8;
#pragma unroll
            for (int j = 0; j < NT; ++j) bv[j] = spk_ld8(wrow[j] + 9 * CA + c0);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[i], bv[j], acc[i][j], 0, 0, 0);
        }
    }

    // epilogue: C/D element (row (lane >> 4) * 4 + r, column lane & 15) of each 16 x 16 tile
    float bias[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) bias[j] = a.bias[n0 + j * 16 + col];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = m0 + i * 16 + (lane >> 4) * 4 + r;
            if (m >= M) continue;
            const int w_out = m % a.W_out;
            const bool valid = a.colvalid[w_out] != 0;
            const long base = (long)m * CO + n0 + col;
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                float v = acc[i][j][r] + bias[j];
                if constexpr (RES) v = v + bf16_to_f32(a.res[base + j * 16]);
                v = fmaxf(v, 0.0f);
                a.out[base + j * 16] = f32_to_bf16(valid ? v : 0.0f);
            }
        }
}

}  // namespace qasr
