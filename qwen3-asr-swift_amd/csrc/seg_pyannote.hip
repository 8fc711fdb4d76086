// seg_pyannote.hip -- pyannote PyanNet segmentation for gfx950 (seg_pyannote.h).  f32 throughout, accurate expf / tanhf / sqrtf.
//
// Launches per pass of B windows (all windows of a pass are independent workgroups over ONE uploaded copy of the audio):
//   seg_wav_stats_kernel   one workgroup per window: mean and population variance of its n samples (the zero tail of a short window is
//                          part of them), fixed tree.
//   seg_sinc_kernel        Conv1d(1->80, k 251, s 10) + bias -> |.| -> MaxPool(3, 3), fused: the 80 x 251 filters (80 KB) sit in LDS once
//                          per workgroup, next to the 3121 normalised samples its 96 pooled frames need; a thread owns 4 channels x 9 conv
//                          outputs (3 pooled frames), one LDS float4 of weights and 9 broadcast samples per 36 FMAs.  VALU: K = 251 with a
//                          stride-10 window has no dense operand for the 16x16x4 f32 MFMA without an im2col copy through LDS.
//   seg_chan_stats_kernel  InstanceNorm statistics per (window, channel) over time, two passes (mean, then centred squares), fixed order.
//                          Only mean and 1/sqrt(var + eps) are stored: the normalisation, its affine and the LeakyReLU are applied by the
//                          next consumer when it loads, so only pooled activations go through HBM.
//   seg_conv5_kernel<CIN>  Conv1d(CIN->60, k 5) + bias -> MaxPool(3, 3) on the normalised input: weights [CIN][5][60] in LDS (96 / 72 KB),
//                          a thread owns 4 channels x 6 conv outputs (2 pooled frames): 15 LDS reads per 120 FMAs.  VALU, as above: small.
//   seg_proj_kernel        LSTM input projection of both directions, [B F][in] x [in][1024] + bias: a 64 x 64 tiled f32 GEMM on the VALU
//                          (4 x 4 per thread, k in LDS steps of 16); layer 0 applies the last InstanceNorm + LeakyReLU at its load.
//   seg_recur_kernel       grid (window, direction), 1024 threads, in the form of vad_recur_kernel: Wh in VGPRs (thread = gate row x half
//                          of h), h broadcast through LDS, the next step's pre-gate loaded one step ahead; the backward workgroup walks
//                          time in reverse and writes h at the original index.  Four dependent (proj, recur) launch pairs; no workgroup
//                          waits for another.
//   seg_head_kernel        16 frames per workgroup: Linear + LeakyReLU twice, classifier, softmax, speaker and speech probabilities.
// Summation order (the bit-identity argument): every output is ONE thread's sequential fmaf chain in an order fixed
// by the layer (sinc: tap 0..250, + bias; conv5: input channel, then tap, + bias; projection: input 0..in-1, + bias; head: input in
// order, + bias), the recurrent dot is two fixed 64-term halves as in the VAD, and the statistics are a per-thread strided chain followed
// by a fixed tree / fixed serial combine.  The batch size, a window's place in the batch, the pass split and the grid never enter.
#include "seg_pyannote.h"
#include <algorithm>
#include <cstring>

namespace qasr {

// ---- device weight block (floats; every offset a multiple of 4) --------------------------------------------------------------------
constexpr int SW_WAVN = 0;                                   // weight, bias, 0, 0
constexpr int SW_C0 = 4;                                     // [251 k][80 co]
constexpr int SB_C0 = SW_C0 + SEG_K0 * SEG_C0;               // 20084
constexpr int SN_0 = SB_C0 + SEG_C0;                         // norm.0 weight [80] | bias [80]
constexpr int SW_C1 = SN_0 + 2 * SEG_C0;                     // [80 ci][5 k][60 co]
constexpr int SB_C1 = SW_C1 + SEG_C0 * SEG_K1 * SEG_C1;
constexpr int SN_1 = SB_C1 + SEG_C1;
constexpr int SW_C2 = SN_1 + 2 * SEG_C1;                     // [60 ci][5 k][60 co]
constexpr int SB_C2 = SW_C2 + SEG_C1 * SEG_K1 * SEG_C1;
constexpr int SN_2 = SB_C2 + SEG_C1;
constexpr int SW_LSTM = SN_2 + 2 * SEG_C1;
constexpr int SEG_N = 2 * SEG_G;                             // 1024 pre-gates per frame: fwd | bwd
// per layer: Wx [in][1024] | bias [1024] | Wh [2][512][128] (reference layout)
__host__ __device__ constexpr int seg_lstm_in(int l) { return l == 0 ? SEG_C1 : 2 * SEG_H; }
__host__ __device__ constexpr int seg_lstm_size(int l) { return seg_lstm_in(l) * SEG_N + SEG_N + 2 * SEG_G * SEG_H; }
__host__ __device__ constexpr int seg_lstm_off(int l) { return l == 0 ? SW_LSTM : seg_lstm_off(l - 1) + seg_lstm_size(l - 1); }
constexpr int SW_L0 = seg_lstm_off(SEG_LAYERS);              // [256 in][128 out]
constexpr int SB_L0 = SW_L0 + 256 * 128;
constexpr int SW_L1 = SB_L0 + 128;                           // [128][128]
constexpr int SB_L1 = SW_L1 + 128 * 128;
constexpr int SW_CL = SB_L1 + 128;                           // [128][8] (7 used)
constexpr int SB_CL = SW_CL + 128 * 8;                       // [8]
constexpr int SW_TOTAL = SB_CL + 8;
static_assert(SW_C1 % 4 == 0 && SW_C2 % 4 == 0 && SW_LSTM % 4 == 0 && SW_L0 % 4 == 0 && SW_CL % 4 == 0, "alignment");

__device__ __forceinline__ float seg_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ float seg_leaky(float x) { return fmaxf(x, 0.01f * x); }       // SincNet.swift:127-129

// ---- wav_norm statistics (SincNet.swift:50, 89-97) ------------------------------------------------------------------------------------
constexpr int ST_THREADS = 1024;

// sum over the block in a fixed tree (pairs tid, tid + s for s = 512 .. 1); every thread gets the result
__device__ __forceinline__ float block_sum_fixed(float v, float* red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int s = ST_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    const float r = red[0];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(ST_THREADS) void seg_wav_stats_kernel(const float* __restrict__ pcm, const long* __restrict__ off, long total,
                                                                   int n, float* __restrict__ stat) {
    __shared__ float red[ST_THREADS];
    const int b = blockIdx.x, tid = threadIdx.x;
    const long o = off[b];
    float s = 0.0f;
    for (int i = tid; i < n; i += ST_THREADS) s += (o + i < total) ? pcm[o + i] : 0.0f;
    const float mean = block_sum_fixed(s, red) / (float)n;
    float q = 0.0f;
    for (int i = tid; i < n; i += ST_THREADS) {
        const float d = ((o + i < total) ? pcm[o + i] : 0.0f) - mean;
        q = fmaf(d, d, q);
    }
    const float var = block_sum_fixed(q, red) / (float)n;
    if (tid == 0) { stat[2 * b] = mean; stat[2 * b + 1] = 1.0f / sqrtf(var + 1e-5f); }
}

// ---- layer 0: Conv1d(1->80, k 251, s 10) + bias -> abs -> MaxPool(3, 3)  (SincNet.swift:52-62) -------------------------------------
constexpr int S0_THREADS = 640, S0_TG = 32, S0_POOL = 3 * S0_TG;          // 96 pooled frames = 288 conv outputs per workgroup
constexpr int S0_CONV = 3 * S0_POOL, S0_X = (S0_CONV - 1) * SEG_S0 + SEG_K0;   // 3121 samples
constexpr int S0_XPAD = (S0_X + 3) & ~3;
constexpr size_t S0_LDS = (size_t)(SEG_K0 * SEG_C0 + S0_XPAD) * sizeof(float);

__global__ __launch_bounds__(S0_THREADS) void seg_sinc_kernel(const float* __restrict__ W, const float* __restrict__ pcm,
                                                              const long* __restrict__ off, long total, int n, int P0,
                                                              const float* __restrict__ wstat, float* __restrict__ p0) {
    extern __shared__ float lds[];
    float* ws = lds;                                   // [251][80]
    float* xs = lds + SEG_K0 * SEG_C0;                 // [3121]
    const int b = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x;
    for (int i = tid * 4; i < SEG_K0 * SEG_C0; i += S0_THREADS * 4)
        *reinterpret_cast<float4*>(&ws[i]) = *reinterpret_cast<const float4*>(&W[SW_C0 + i]);
    {
        const float mean = wstat[2 * b], rstd = wstat[2 * b + 1], nw = W[SW_WAVN], nb = W[SW_WAVN + 1];
        const long o = off[b];
        const int s0 = tile * S0_CONV * SEG_S0;
        for (int i = tid; i < S0_XPAD; i += S0_THREADS) {
            const int s = s0 + i;
            float v = 0.0f;
            if (s < n) {                               // the window's own zero tail is normalised like any sample
                const float x = (o + s < total) ? pcm[o + s] : 0.0f;
                v = ((x - mean) * rstd) * nw + nb;
            }
            xs[i] = v;
        }
    }
    __syncthreads();
    const int q = tid % 20, tg = tid / 20;
    float acc[9][4];
#pragma unroll
    for (int j = 0; j < 9; ++j)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[j][c] = 0.0f;
    const float* xb = xs + tg * 9 * SEG_S0;
#pragma unroll 2
    for (int k = 0; k < SEG_K0; ++k) {
        const float4 w = lds_read_f4(&ws[k * SEG_C0 + 4 * q]);
#pragma unroll
        for (int j = 0; j < 9; ++j) {
            const float x = xb[j * SEG_S0 + k];
            acc[j][0] = fmaf(w.x, x, acc[j][0]);
            acc[j][1] = fmaf(w.y, x, acc[j][1]);
            acc[j][2] = fmaf(w.z, x, acc[j][2]);
            acc[j][3] = fmaf(w.w, x, acc[j][3]);
        }
    }
    const float4 bias = *reinterpret_cast<const float4*>(&W[SB_C0 + 4 * q]);
    const float bb[4] = {bias.x, bias.y, bias.z, bias.w};
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        const int p = tile * S0_POOL + tg * 3 + m;
        if (p < P0) {
            float r[4];
#pragma unroll
            for (int c = 0; c < 4; ++c)
                r[c] = fmaxf(fmaxf(fabsf(acc[3 * m][c] + bb[c]), fabsf(acc[3 * m + 1][c] + bb[c])), fabsf(acc[3 * m + 2][c] + bb[c]));
            *reinterpret_cast<float4*>(&p0[((long)b * P0 + p) * SEG_C0 + 4 * q]) = make_float4(r[0], r[1], r[2], r[3]);
        }
    }
}

// ---- InstanceNorm statistics over time of a channels-last [B][P][C] tensor (SincNet.swift:89-97) -------------------------------------
constexpr int CS_CG = 20, CS_SL = 48, CS_THREADS = CS_CG * CS_SL;

__global__ __launch_bounds__(CS_THREADS) void seg_chan_stats_kernel(const float* __restrict__ x, int P, int C, float* __restrict__ stat) {
    __shared__ float red[CS_SL][CS_CG];
    __shared__ float s_mean[CS_CG];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int cl = tid % CS_CG, sl = tid / CS_CG, c = blockIdx.x * CS_CG + cl;
    const float* xp = x + (long)b * P * C + c;
    float s = 0.0f;
    for (int p = sl; p < P; p += CS_SL) s += xp[(long)p * C];
    red[sl][cl] = s;
    __syncthreads();
    if (sl == 0) {
        float t = 0.0f;
        for (int i = 0; i < CS_SL; ++i) t += red[i][cl];
        s_mean[cl] = t / (float)P;
    }
    __syncthreads();
    const float mean = s_mean[cl];
    float qv = 0.0f;
    for (int p = sl; p < P; p += CS_SL) {
        const float d = xp[(long)p * C] - mean;
        qv = fmaf(d, d, qv);
    }
    red[sl][cl] = qv;
    __syncthreads();
    if (sl == 0) {
        float t = 0.0f;
        for (int i = 0; i < CS_SL; ++i) t += red[i][cl];
        stat[((long)b * C + c) * 2] = mean;
        stat[((long)b * C + c) * 2 + 1] = 1.0f / sqrtf(t / (float)P + 1e-5f);
    }
}

// ---- layers 1, 2: InstanceNorm + LeakyReLU at the load, Conv1d(CIN->60, k 5) + bias -> MaxPool(3, 3) ---------------------------------
constexpr int C5_THREADS = 240, C5_TG = 16, C5_POOL = 2 * C5_TG, C5_ROWS = 3 * C5_POOL + SEG_K1 - 1;       // 32 pooled, 100 input rows
template <int CIN> constexpr size_t c5_lds() { return (size_t)(CIN * SEG_K1 * SEG_C1 + C5_ROWS * CIN) * sizeof(float); }

template <int CIN>
__global__ __launch_bounds__(C5_THREADS) void seg_conv5_kernel(const float* __restrict__ Wc, const float* __restrict__ bias,
                                                               const float* __restrict__ nwb, const float* __restrict__ xin,
                                                               const float* __restrict__ stat, int Pin, int Pout,
                                                               float* __restrict__ out) {
    extern __shared__ float lds[];
    float* ws = lds;                                   // [CIN][5][60]
    float* xs = lds + CIN * SEG_K1 * SEG_C1;           // [100][CIN]
    const int b = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x;
    for (int i = tid * 4; i < CIN * SEG_K1 * SEG_C1; i += C5_THREADS * 4)
        *reinterpret_cast<float4*>(&ws[i]) = *reinterpret_cast<const float4*>(&Wc[i]);
    const int r0 = tile * 3 * C5_POOL;
    for (int i = tid; i < C5_ROWS * CIN; i += C5_THREADS) {
        const int r = i / CIN, ci = i - r * CIN, row = r0 + r;
        float v = 0.0f;
        if (row < Pin) {
            const float mean = stat[((long)b * CIN + ci) * 2], rstd = stat[((long)b * CIN + ci) * 2 + 1];
            v = seg_leaky(((xin[((long)b * Pin + row) * CIN + ci] - mean) * rstd) * nwb[ci] + nwb[CIN + ci]);
        }
        xs[i] = v;
    }
    __syncthreads();
    const int q = tid % 15, tg = tid / 15;
    float acc[6][4];
#pragma unroll
    for (int j = 0; j < 6; ++j)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[j][c] = 0.0f;
    const float* xb = xs + tg * 6 * CIN;
    for (int ci = 0; ci < CIN; ++ci) {
        float x[10];
#pragma unroll
        for (int j = 0; j < 10; ++j) x[j] = xb[j * CIN + ci];
#pragma unroll
        for (int k = 0; k < SEG_K1; ++k) {
            const float4 w = lds_read_f4(&ws[(ci * SEG_K1 + k) * SEG_C1 + 4 * q]);
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                acc[j][0] = fmaf(w.x, x[j + k], acc[j][0]);
                acc[j][1] = fmaf(w.y, x[j + k], acc[j][1]);
                acc[j][2] = fmaf(w.z, x[j + k], acc[j][2]);
                acc[j][3] = fmaf(w.w, x[j + k], acc[j][3]);
            }
        }
    }
    const float4 bv = *reinterpret_cast<const float4*>(&bias[4 * q]);
    const float bb[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        const int p = tile * C5_POOL + tg * 2 + m;
        if (p < Pout) {
            float r[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) r[c] = fmaxf(fmaxf(acc[3 * m][c] + bb[c], acc[3 * m + 1][c] + bb[c]), acc[3 * m + 2][c] + bb[c]);
            *reinterpret_cast<float4*>(&out[((long)b * Pout + p) * SEG_C1 + 4 * q]) = make_float4(r[0], r[1], r[2], r[3]);
        }
    }
}

// ---- LSTM input projection: pre[m][0..1023] = bias + x[m] . Wx^T, both directions (BiLSTM.swift:29) ----------------------------------
constexpr int PJ_THREADS = 256, PJ_T = 64, PJ_K = 16;

// NORM: x is the raw pooled layer-2 output [M][60]; InstanceNorm (statistics of window m / F) + LeakyReLU are applied at the load
template <bool NORM>
__global__ __launch_bounds__(PJ_THREADS) void seg_proj_kernel(const float* __restrict__ A, int M, int K, const float* __restrict__ Wx,
                                                              const float* __restrict__ bias, const float* __restrict__ stat,
                                                              const float* __restrict__ nwb, int F, float* __restrict__ pre) {
    __shared__ __attribute__((aligned(16))) float As[PJ_K][PJ_T + 4];
    __shared__ __attribute__((aligned(16))) float Bs[PJ_K][PJ_T];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int m0 = blockIdx.x * PJ_T, n0 = blockIdx.y * PJ_T;
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.0f;
    for (int k0 = 0; k0 < K; k0 += PJ_K) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int idx = tid + r * PJ_THREADS, row = idx >> 4, kk = idx & 15, m = m0 + row, k = k0 + kk;
            float v = 0.0f;                            // rows past M and inputs past K add exact zeros
            if (m < M && k < K) {
                v = A[(long)m * K + k];
                if (NORM) {
                    const long sb = ((long)(m / F) * K + k) * 2;
                    v = seg_leaky(((v - stat[sb]) * stat[sb + 1]) * nwb[k] + nwb[K + k]);
                }
            }
            As[kk][row] = v;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int idx = tid + r * PJ_THREADS, kk = idx >> 6, col = idx & 63, k = k0 + kk;
            Bs[kk][col] = k < K ? Wx[(long)k * SEG_N + n0 + col] : 0.0f;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < PJ_K; ++kk) {
            const float4 a = lds_read_f4(&As[kk][ty * 4]);
            const float4 bq = lds_read_f4(&Bs[kk][tx * 4]);
            const float av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {bq.x, bq.y, bq.z, bq.w};
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(av[i], bv[j], acc[i][j]);
        }
        __syncthreads();
    }
    const float4 bb = *reinterpret_cast<const float4*>(&bias[n0 + tx * 4]);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = m0 + ty * 4 + i;
        if (m < M)
            *reinterpret_cast<float4*>(&pre[(long)m * SEG_N + n0 + tx * 4]) =
                make_float4(bb.x + acc[i][0], bb.y + acc[i][1], bb.z + acc[i][2], bb.w + acc[i][3]);
    }
}

// ---- LSTM recurrence: grid (window, direction) (BiLSTM.swift:36-58, 81-97) ---------------------------------------------------------
constexpr int RC_THREADS = 1024;

__global__ __launch_bounds__(RC_THREADS) void seg_recur_kernel(const float* __restrict__ Wh, const float* __restrict__ pre, int F,
                                                               float* __restrict__ hout) {
    __shared__ __attribute__((aligned(16))) float s_h[SEG_H];
    __shared__ float s_gate[SEG_G];
    const int b = blockIdx.x, dir = blockIdx.y, tid = threadIdx.x;
    const int g = tid >> 1, half = tid & 1;
    float w[64];                                       // Wh[dir][g][64 half .. 64 half + 63]
#pragma unroll
    for (int k = 0; k < 64; k += 4) {
        const float4 v = *reinterpret_cast<const float4*>(&Wh[((long)dir * SEG_G + g) * SEG_H + half * 64 + k]);
        w[k] = v.x; w[k + 1] = v.y; w[k + 2] = v.z; w[k + 3] = v.w;
    }
    float h = 0.0f, c = 0.0f;                          // the reference's nil initial state is the zero state
    if (tid < SEG_H) s_h[tid] = 0.0f;
    __syncthreads();
    const long base = (long)b * F;
    const int step = dir ? -1 : 1, t0 = dir ? F - 1 : 0;      // the backward direction walks the frames in reverse
    const float* pp = pre + dir * SEG_G + g;
    float pnext = half == 0 ? pp[(base + t0) * SEG_N] : 0.0f;
    for (int t = 0; t < F; ++t) {
        const int tt = t0 + step * t;
        const float pcur = pnext;
        if (half == 0 && t + 1 < F) pnext = pp[(base + tt + step) * SEG_N];
        float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
#pragma unroll
        for (int k = 0; k < 64; k += 4) {
            const float4 hv = lds_read_f4(&s_h[half * 64 + k]);
            a0 = fmaf(w[k], hv.x, a0); a1 = fmaf(w[k + 1], hv.y, a1); a2 = fmaf(w[k + 2], hv.z, a2); a3 = fmaf(w[k + 3], hv.w, a3);
        }
        const float part = (a0 + a1) + (a2 + a3);
        const float other = dpp_mov_f32<0xB1>(part);  // the partner half (lane ^ 1)
        if (half == 0) s_gate[g] = pcur + (part + other);
        __syncthreads();
        if (tid < SEG_H) {                             // i, f, g, o (BiLSTM.swift:42-46)
            const float ig = seg_sigmoid(s_gate[tid]), fg = seg_sigmoid(s_gate[SEG_H + tid]);
            const float gg = tanhf(s_gate[2 * SEG_H + tid]), og = seg_sigmoid(s_gate[3 * SEG_H + tid]);
            c = fg * c + ig * gg;
            h = og * tanhf(c);
            s_h[tid] = h;
            hout[(base + tt) * (2 * SEG_H) + dir * SEG_H + tid] = h;
        }
        __syncthreads();
    }
}

// ---- head: Linear + LeakyReLU x 2, classifier, softmax, powerset decoders (Segmentation.swift:73-96, PowersetDecoder.swift:23-31) ----
constexpr int HD_THREADS = 128, HD_F = 16;

__global__ __launch_bounds__(HD_THREADS) void seg_head_kernel(const float* __restrict__ W, const float* __restrict__ x, int M,
                                                              float* __restrict__ post, float* __restrict__ spk,
                                                              float* __restrict__ speech) {
    __shared__ __attribute__((aligned(16))) float xs[HD_F][256];
    __shared__ __attribute__((aligned(16))) float h1[HD_F][128];
    __shared__ __attribute__((aligned(16))) float h2[HD_F][128];
    __shared__ float lg[HD_F][8];
    const int tid = threadIdx.x, m0 = blockIdx.x * HD_F;
    for (int i = tid; i < HD_F * 256; i += HD_THREADS) {
        const int f = i >> 8, m = m0 + f;
        xs[f][i & 255] = m < M ? x[(long)m * 256 + (i & 255)] : 0.0f;
    }
    __syncthreads();
    float acc[HD_F];
#pragma unroll
    for (int f = 0; f < HD_F; ++f) acc[f] = 0.0f;
    for (int i = 0; i < 256; i += 4) {
        const float w0 = W[SW_L0 + (i + 0) * 128 + tid], w1 = W[SW_L0 + (i + 1) * 128 + tid];
        const float w2 = W[SW_L0 + (i + 2) * 128 + tid], w3 = W[SW_L0 + (i + 3) * 128 + tid];
#pragma unroll
        for (int f = 0; f < HD_F; ++f) {
            const float4 v = lds_read_f4(&xs[f][i]);
            float a = acc[f];
            a = fmaf(w0, v.x, a); a = fmaf(w1, v.y, a); a = fmaf(w2, v.z, a); a = fmaf(w3, v.w, a);
            acc[f] = a;
        }
    }
    {
        const float bb = W[SB_L0 + tid];
#pragma unroll
        for (int f = 0; f < HD_F; ++f) { h1[f][tid] = seg_leaky(acc[f] + bb); acc[f] = 0.0f; }
    }
    __syncthreads();
    for (int i = 0; i < 128; i += 4) {
        const float w0 = W[SW_L1 + (i + 0) * 128 + tid], w1 = W[SW_L1 + (i + 1) * 128 + tid];
        const float w2 = W[SW_L1 + (i + 2) * 128 + tid], w3 = W[SW_L1 + (i + 3) * 128 + tid];
#pragma unroll
        for (int f = 0; f < HD_F; ++f) {
            const float4 v = lds_read_f4(&h1[f][i]);
            float a = acc[f];
            a = fmaf(w0, v.x, a); a = fmaf(w1, v.y, a); a = fmaf(w2, v.z, a); a = fmaf(w3, v.w, a);
            acc[f] = a;
        }
    }
    {
        const float bb = W[SB_L1 + tid];
#pragma unroll
        for (int f = 0; f < HD_F; ++f) h2[f][tid] = seg_leaky(acc[f] + bb);
    }
    __syncthreads();
    if (tid < HD_F * SEG_CLASSES) {
        const int f = tid / SEG_CLASSES, c = tid - f * SEG_CLASSES;
        float a = 0.0f;
        for (int i = 0; i < 128; ++i) a = fmaf(W[SW_CL + i * 8 + c], h2[f][i], a);
        lg[f][c] = a + W[SB_CL + c];
    }
    __syncthreads();
    if (tid < HD_F && m0 + tid < M) {
        const long m = m0 + tid;
        float p[SEG_CLASSES], mx = lg[tid][0];
#pragma unroll
        for (int c = 1; c < SEG_CLASSES; ++c) mx = fmaxf(mx, lg[tid][c]);
        float sum = 0.0f;
#pragma unroll
        for (int c = 0; c < SEG_CLASSES; ++c) { p[c] = expf(lg[tid][c] - mx); sum += p[c]; }
#pragma unroll
        for (int c = 0; c < SEG_CLASSES; ++c) { p[c] = p[c] / sum; post[m * SEG_CLASSES + c] = p[c]; }
        spk[m * 3 + 0] = (p[1] + p[4]) + p[5];         // PowersetDecoder.swift:25-29, in that order of addition
        spk[m * 3 + 1] = (p[2] + p[4]) + p[6];
        spk[m * 3 + 2] = (p[3] + p[5]) + p[6];
        speech[m] = 1.0f - p[0];                       // Segmentation.swift:93-96
    }
}

// ---- weights ------------------------------------------------------------------------------------------------------------------------
const std::vector<std::pair<std::string, std::vector<int64_t>>>& seg_tensor_shapes() {
    static const std::vector<std::pair<std::string, std::vector<int64_t>>> s = [] {
        std::vector<std::pair<std::string, std::vector<int64_t>>> v = {
            {"sincnet.wav_norm.weight", {1}}, {"sincnet.wav_norm.bias", {1}},
            {"sincnet.conv.0.weight", {SEG_C0, SEG_K0, 1}}, {"sincnet.conv.0.bias", {SEG_C0}},
            {"sincnet.conv.1.weight", {SEG_C1, SEG_K1, SEG_C0}}, {"sincnet.conv.1.bias", {SEG_C1}},
            {"sincnet.conv.2.weight", {SEG_C1, SEG_K1, SEG_C1}}, {"sincnet.conv.2.bias", {SEG_C1}},
            {"sincnet.norm.0.weight", {SEG_C0}}, {"sincnet.norm.0.bias", {SEG_C0}},
            {"sincnet.norm.1.weight", {SEG_C1}}, {"sincnet.norm.1.bias", {SEG_C1}},
            {"sincnet.norm.2.weight", {SEG_C1}}, {"sincnet.norm.2.bias", {SEG_C1}},
        };
        for (const char* d : {"lstm_fwd", "lstm_bwd"})
            for (int l = 0; l < SEG_LAYERS; ++l) {
                const std::string p = std::string(d) + ".layers." + std::to_string(l) + ".";
                v.push_back({p + "Wx", {SEG_G, seg_lstm_in(l)}});
                v.push_back({p + "Wh", {SEG_G, SEG_H}});
                v.push_back({p + "bias", {SEG_G}});
            }
        v.push_back({"linear.0.weight", {128, 256}}); v.push_back({"linear.0.bias", {128}});
        v.push_back({"linear.1.weight", {128, 128}}); v.push_back({"linear.1.bias", {128}});
        v.push_back({"classifier.weight", {SEG_CLASSES, 128}}); v.push_back({"classifier.bias", {SEG_CLASSES}});
        return v;
    }();
    return s;
}

float seg_optional_default(const std::string& key) {
    if (key.compare(0, 13, "sincnet.conv.") == 0 && key.size() > 5 && key.compare(key.size() - 5, 5, ".bias") == 0) return 0.0f;
    const bool norm = key.compare(0, 13, "sincnet.norm.") == 0 || key.compare(0, 17, "sincnet.wav_norm.") == 0;
    if (norm && key.compare(key.size() - 7, 7, ".weight") == 0) return 1.0f;
    if (norm && key.compare(key.size() - 5, 5, ".bias") == 0) return 0.0f;
    return -1.0f;
}

// ---- host object --------------------------------------------------------------------------------------------------------------------
constexpr size_t SEG_MAX_N = (size_t)300 * SEG_RATE;         // one window: at most 300 s (the workspace is max_windows of them)

SegPyannote::SegPyannote(int device, const CheckedWeights& w, int max_windows, hipStream_t work)
    : device_(device), max_windows_(max_windows), param_bytes_(w.disk_bytes) {
    if (max_windows <= 0 || max_windows > 4096) throw std::invalid_argument("pyannote segmentation: max_windows in 1..4096");
    std::vector<float> h(SW_TOTAL, 0.0f);
    h[SW_WAVN] = w.t.at("sincnet.wav_norm.weight")[0];
    h[SW_WAVN + 1] = w.t.at("sincnet.wav_norm.bias")[0];
    {   // conv.0 [80][251][1] -> [251][80]
        const auto& c0 = w.t.at("sincnet.conv.0.weight");
        for (int co = 0; co < SEG_C0; ++co)
            for (int k = 0; k < SEG_K0; ++k) h[SW_C0 + k * SEG_C0 + co] = c0[(size_t)co * SEG_K0 + k];
    }
    const int wo[3] = {SW_C0, SW_C1, SW_C2}, bo[3] = {SB_C0, SB_C1, SB_C2}, no[3] = {SN_0, SN_1, SN_2};
    const int cout[3] = {SEG_C0, SEG_C1, SEG_C1}, cin[3] = {1, SEG_C0, SEG_C1};
    for (int l = 0; l < 3; ++l) {
        const std::string p = "sincnet.conv." + std::to_string(l), q = "sincnet.norm." + std::to_string(l);
        if (l > 0) {   // [out][k][in] -> [in][k][out]
            const auto& cw = w.t.at(p + ".weight");
            for (int o = 0; o < cout[l]; ++o)
                for (int k = 0; k < SEG_K1; ++k)
                    for (int i = 0; i < cin[l]; ++i)
                        h[wo[l] + (i * SEG_K1 + k) * cout[l] + o] = cw[((size_t)o * SEG_K1 + k) * cin[l] + i];
        }
        for (int o = 0; o < cout[l]; ++o) {
            h[bo[l] + o] = w.t.at(p + ".bias")[o];
            h[no[l] + o] = w.t.at(q + ".weight")[o];
            h[no[l] + cout[l] + o] = w.t.at(q + ".bias")[o];
        }
    }
    for (int l = 0; l < SEG_LAYERS; ++l) {
        const int in = seg_lstm_in(l), base = seg_lstm_off(l);
        for (int d = 0; d < 2; ++d) {
            const std::string p = std::string(d ? "lstm_bwd" : "lstm_fwd") + ".layers." + std::to_string(l) + ".";
            const auto &wx = w.t.at(p + "Wx"), &wh = w.t.at(p + "Wh"), &bx = w.t.at(p + "bias");
            for (int g = 0; g < SEG_G; ++g) {
                for (int i = 0; i < in; ++i) h[base + i * SEG_N + d * SEG_G + g] = wx[(size_t)g * in + i];
                h[base + in * SEG_N + d * SEG_G + g] = bx[g];
                for (int i = 0; i < SEG_H; ++i) h[base + in * SEG_N + SEG_N + (d * SEG_G + g) * SEG_H + i] = wh[(size_t)g * SEG_H + i];
            }
        }
    }
    {
        const auto &l0 = w.t.at("linear.0.weight"), &l1 = w.t.at("linear.1.weight"), &cl = w.t.at("classifier.weight");
        for (int o = 0; o < 128; ++o) {
            for (int i = 0; i < 256; ++i) h[SW_L0 + i * 128 + o] = l0[(size_t)o * 256 + i];
            for (int i = 0; i < 128; ++i) h[SW_L1 + i * 128 + o] = l1[(size_t)o * 128 + i];
            h[SB_L0 + o] = w.t.at("linear.0.bias")[o];
            h[SB_L1 + o] = w.t.at("linear.1.bias")[o];
        }
        for (int c = 0; c < SEG_CLASSES; ++c) {
            for (int i = 0; i < 128; ++i) h[SW_CL + i * 8 + c] = cl[(size_t)c * 128 + i];
            h[SB_CL + c] = w.t.at("classifier.bias")[c];
        }
    }
    QASR_HIP(hipSetDevice(device_));
    QASR_HIP(hipStreamCreateWithFlags(&own_, hipStreamNonBlocking));
    work_ = work ? work : own_;
    for (auto& e : ev_) QASR_HIP(hipEventCreate(&e));
    d_w_.alloc((size_t)SW_TOTAL * sizeof(float));
    QASR_HIP(hipMemcpy(d_w_.p, h.data(), (size_t)SW_TOTAL * sizeof(float), hipMemcpyHostToDevice));
    ensure_dynamic_lds(reinterpret_cast<const void*>(&seg_sinc_kernel), (int)S0_LDS);
    ensure_dynamic_lds(reinterpret_cast<const void*>(&seg_conv5_kernel<SEG_C0>), (int)c5_lds<SEG_C0>());
    ensure_dynamic_lds(reinterpret_cast<const void*>(&seg_conv5_kernel<SEG_C1>), (int)c5_lds<SEG_C1>());
    ensure((size_t)10 * SEG_RATE, (size_t)10 * SEG_RATE);
}

SegPyannote::~SegPyannote() {
    if (work_) (void)hipStreamSynchronize(work_);
    for (auto& e : ev_) if (e) (void)hipEventDestroy(e);
    if (own_) (void)hipStreamDestroy(own_);
}

void SegPyannote::unload() {
    if (!loaded_) return;
    QASR_HIP(hipSetDevice(device_));
    QASR_HIP(hipStreamSynchronize(work_));
    for (DevBuf* b : {&d_w_, &d_pcm_, &d_off_, &d_stat_, &d_p0_, &d_p1_, &d_p2_, &d_pre_, &d_h_[0], &d_h_[1], &d_out_}) b->release();
    cap_total_ = cap_n_ = 0;
    loaded_ = false;
}

constexpr int SEG_STAT = 2 + 2 * (SEG_C0 + SEG_C1 + SEG_C1);    // floats of statistics per window: wav | norm.0 | norm.1 | norm.2
constexpr int SEG_OUTF = SEG_CLASSES + SEG_SPK + 1;              // output floats per frame

void SegPyannote::ensure(size_t total, size_t n) {
    if (total > cap_total_) {
        QASR_HIP(hipStreamSynchronize(work_));
        cap_total_ = total;
        d_pcm_.alloc(cap_total_ * sizeof(float));
    }
    if (n <= cap_n_) return;
    QASR_HIP(hipStreamSynchronize(work_));
    cap_n_ = n;
    const SegGeom g = seg_geom((long)n);
    const size_t B = (size_t)max_windows_, F = (size_t)g.F;
    d_off_.alloc(B * sizeof(long));
    h_off_.alloc(B * sizeof(long));
    d_stat_.alloc(B * SEG_STAT * sizeof(float));
    d_p0_.alloc(B * g.P0 * SEG_C0 * sizeof(float));
    d_p1_.alloc(B * g.P1 * SEG_C1 * sizeof(float));
    d_p2_.alloc(B * F * SEG_C1 * sizeof(float));
    d_pre_.alloc(B * F * SEG_N * sizeof(float));
    d_h_[0].alloc(B * F * 2 * SEG_H * sizeof(float));
    d_h_[1].alloc(B * F * 2 * SEG_H * sizeof(float));
    d_out_.alloc(B * F * SEG_OUTF * sizeof(float));
    h_out_.alloc(B * F * SEG_OUTF * sizeof(float));
}

// every launch of one pass of B windows, in stream order (a linear chain)
void SegPyannote::pass(int B, const SegGeom& g, int n, long total, hipStream_t s) {
    const float* W = d_w_.as<float>();
    const float* pcm = d_pcm_.as<float>();
    const long* off = d_off_.as<long>();
    float* st_wav = d_stat_.as<float>();
    float* st0 = st_wav + (size_t)max_windows_ * 2;
    float* st1 = st0 + (size_t)max_windows_ * 2 * SEG_C0;
    float* st2 = st1 + (size_t)max_windows_ * 2 * SEG_C1;
    float *p0 = d_p0_.as<float>(), *p1 = d_p1_.as<float>(), *p2 = d_p2_.as<float>(), *pre = d_pre_.as<float>();
    const int M = B * g.F;
    hipLaunchKernelGGL(seg_wav_stats_kernel, dim3(B), dim3(ST_THREADS), 0, s, pcm, off, total, n, st_wav);
    hipLaunchKernelGGL(seg_sinc_kernel, dim3(cdiv(g.P0, S0_POOL), B), dim3(S0_THREADS), S0_LDS, s, W, pcm, off, total, n, g.P0, st_wav, p0);
    hipLaunchKernelGGL(seg_chan_stats_kernel, dim3(SEG_C0 / CS_CG, B), dim3(CS_THREADS), 0, s, p0, g.P0, SEG_C0, st0);
    hipLaunchKernelGGL(seg_conv5_kernel<SEG_C0>, dim3(cdiv(g.P1, C5_POOL), B), dim3(C5_THREADS), c5_lds<SEG_C0>(), s, W + SW_C1, W + SB_C1,
                       W + SN_0, p0, st0, g.P0, g.P1, p1);
    hipLaunchKernelGGL(seg_chan_stats_kernel, dim3(SEG_C1 / CS_CG, B), dim3(CS_THREADS), 0, s, p1, g.P1, SEG_C1, st1);
    hipLaunchKernelGGL(seg_conv5_kernel<SEG_C1>, dim3(cdiv(g.F, C5_POOL), B), dim3(C5_THREADS), c5_lds<SEG_C1>(), s, W + SW_C2, W + SB_C2,
                       W + SN_1, p1, st1, g.P1, g.F, p2);
    hipLaunchKernelGGL(seg_chan_stats_kernel, dim3(SEG_C1 / CS_CG, B), dim3(CS_THREADS), 0, s, p2, g.F, SEG_C1, st2);
    const float* x = p2;
    for (int l = 0; l < SEG_LAYERS; ++l) {
        const int in = seg_lstm_in(l);
        const float* Wl = W + seg_lstm_off(l);
        float* hout = d_h_[l & 1].as<float>();
        const dim3 grid(cdiv(M, PJ_T), SEG_N / PJ_T);
        if (l == 0)
            hipLaunchKernelGGL(seg_proj_kernel<true>, grid, dim3(PJ_THREADS), 0, s, x, M, in, Wl, Wl + in * SEG_N, st2, W + SN_2, g.F, pre);
        else
            hipLaunchKernelGGL(seg_proj_kernel<false>, grid, dim3(PJ_THREADS), 0, s, x, M, in, Wl, Wl + in * SEG_N, (const float*)nullptr,
                               (const float*)nullptr, g.F, pre);
        hipLaunchKernelGGL(seg_recur_kernel, dim3(B, 2), dim3(RC_THREADS), 0, s, Wl + in * SEG_N + SEG_N, pre, g.F, hout);
        x = hout;
    }
    float* out = d_out_.as<float>();
    hipLaunchKernelGGL(seg_head_kernel, dim3(cdiv(M, HD_F)), dim3(HD_THREADS), 0, s, W, x, M, out, out + (size_t)M * SEG_CLASSES,
                       out + (size_t)M * (SEG_CLASSES + SEG_SPK));
    QASR_HIP(hipGetLastError());
    QASR_HIP(hipMemcpyAsync(h_out_.p, d_out_.p, (size_t)M * SEG_OUTF * sizeof(float), hipMemcpyDeviceToHost, s));
}

void SegPyannote::run(const float* pcm, size_t total, const long* starts, size_t W, size_t n, float* posteriors, float* speaker_probs,
                      float* speech_probs) {
    if (!loaded_) throw NotLoaded("pyannote segmentation: model unloaded");
    if (n < (size_t)SEG_MIN_SAMPLES) throw std::invalid_argument("pyannote segmentation: a window needs at least 991 samples");
    if (n > SEG_MAX_N) throw std::length_error("pyannote segmentation: window longer than 300 s");
    if (total > ((size_t)1 << 32)) throw std::length_error("pyannote segmentation: buffer longer than 2^32 samples");
    if (W == 0) return;
    for (size_t w = 0; w < W; ++w)
        if (starts[w] < 0 || (size_t)starts[w] > total) throw std::invalid_argument("pyannote segmentation: window start outside the buffer");
    QASR_HIP(hipSetDevice(device_));
    ensure(total, n);
    const SegGeom g = seg_geom((long)n);
    const size_t F = (size_t)g.F;
    QASR_HIP(hipEventRecord(ev_[0], work_));
    if (total) QASR_HIP(hipMemcpyAsync(d_pcm_.p, pcm, total * sizeof(float), hipMemcpyHostToDevice, work_));
    for (size_t w0 = 0; w0 < W; w0 += (size_t)max_windows_) {
        const size_t B = std::min(W - w0, (size_t)max_windows_), M = B * F;
        std::memcpy(h_off_.p, starts + w0, B * sizeof(long));
        QASR_HIP(hipMemcpyAsync(d_off_.p, h_off_.p, B * sizeof(long), hipMemcpyHostToDevice, work_));
        pass((int)B, g, (int)n, (long)total, work_);
        QASR_HIP(hipStreamSynchronize(work_));         // the staging buffers are reused by the next pass
        const float* o = h_out_.as<float>();
        if (posteriors) std::memcpy(posteriors + w0 * F * SEG_CLASSES, o, M * SEG_CLASSES * sizeof(float));
        if (speaker_probs) std::memcpy(speaker_probs + w0 * F * SEG_SPK, o + M * SEG_CLASSES, M * SEG_SPK * sizeof(float));
        if (speech_probs) std::memcpy(speech_probs + w0 * F, o + M * (SEG_CLASSES + SEG_SPK), M * sizeof(float));
    }
    QASR_HIP(hipEventRecord(ev_[1], work_));
    QASR_HIP(hipStreamSynchronize(work_));
    QASR_HIP(hipGetLastError());
    QASR_HIP(hipEventElapsedTime(&last_ms_, ev_[0], ev_[1]));
}

}  // namespace qasr
