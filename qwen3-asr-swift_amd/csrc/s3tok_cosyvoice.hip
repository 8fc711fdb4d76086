// s3tok_cosyvoice.hip -- kernels and host object of the CosyVoice3 speech tokenizer and voice-profile front ends (s3tok_cosyvoice.h;
// DESIGN.md section 24).  Heavy launches are the bf16 MFMA GEMM of gemm.h with the stem gather and the epilogues below, and
// mha_attention_launch as it stands; the Whisper-style mel runs on mel_core.h's 512-point frame transform and tables.
#include "s3tok_cosyvoice.h"
#include "ctc_kernels.h"
#include "gemm.h"
#include "mel_core.h"
#include "qasr.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>

namespace qasr {

// =====================================================================================================================================
// host arithmetic: resampler, FSQ twin
// =====================================================================================================================================
size_t s3_resampled_length(size_t n, int src, int dst) {
    if (src == dst) return n;
    const double ratio = (double)dst / (double)src;                        // VoiceCloning.swift:331-332
    return (size_t)std::floor((double)n * ratio);
}

void s3_resample(const float* x, size_t n, int src, int dst, float* out) {
    if (src == dst) { std::memcpy(out, x, n * sizeof(float)); return; }    // :330
    const double ratio = (double)dst / (double)src;
    const size_t out_len = (size_t)std::floor((double)n * ratio);
    const double step = 1.0 / ratio;                                       // :335
    for (size_t i = 0; i < out_len; ++i) {
        const double pos = (double)i * step;                               // position in Double, fraction in Float (:337-339)
        const size_t idx = (size_t)pos;
        const float frac = (float)(pos - (double)idx);
        const float a = x[idx], b = idx + 1 < n ? x[idx + 1] : a;
        out[i] = a * (1.0f - frac) + b * frac;
    }
}

void s3_fsq_host(const float* proj, size_t rows, int32_t* codes) {
    for (size_t r = 0; r < rows; ++r) {
        int32_t code = 0, p = 1;
        for (int k = 0; k < S3_FSQ; ++k) {                                 // SpeechTokenizer.swift:78-91
            const float h = tanhf(proj[r * S3_FSQ + k]) * S3_FSQ_SCALE;
            code += (int32_t)(nearbyintf(h) + 1.0f) * p;
            p *= 3;
        }
        codes[r] = code;
    }
}

// =====================================================================================================================================
// kernels: Whisper-style mel at 16 kHz (WhisperMelExtractor.swift:132-225)
// =====================================================================================================================================
__device__ __forceinline__ unsigned s3_ordered(float f) {                  // order-preserving float <-> uint: atomicMax on signed floats
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float s3_unordered(unsigned u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u); }

constexpr int S3M_WAVES = 4, S3M_FPW = 8;

// mel.hip's frame kernel with this extractor's frame set: only the T = n / 160 kept frames are computed, so the clip maximum that the
// range clip reads is taken over them (WhisperMelExtractor.swift:155, :209-212), not over the dropped last frame as well.  One wave per
// frame, mel_core.h's transform and filterbank.  Reads of pcm are clamped to [0, n).  raw [frames][128] = log10(max(mel, 1e-10)).
__global__ __launch_bounds__(S3M_WAVES * 64) void s3_whisper_frames_kernel(const float* __restrict__ tab, const float* __restrict__ pcm,
                                                                           const long* __restrict__ pcm_off, const int* __restrict__ n_samples,
                                                                           const int* __restrict__ frame_off, float* __restrict__ raw,
                                                                           unsigned* __restrict__ gmax) {
    __shared__ float s_tab[T_TOTAL];
    __shared__ float2 s_buf[S3M_WAVES][2][256];
    __shared__ float s_pow[S3M_WAVES][260];
    __shared__ float s_max[S3M_WAVES];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < T_TOTAL; i += S3M_WAVES * 64) s_tab[i] = tab[i];
    __syncthreads();
    const int n = n_samples[b], nf = n / MEL_HOP;
    const float* x = pcm + pcm_off[b];
    float* out = raw + (long)frame_off[b] * MEL_NMELS;
    const float2* tw256 = reinterpret_cast<const float2*>(&s_tab[T_TW256]);
    const float2* tw512 = reinterpret_cast<const float2*>(&s_tab[T_TW512]);
    const float scale2 = s_tab[T_SCALE2];
    float vmax = -INFINITY;
    const int frame0 = blockIdx.x * (S3M_WAVES * S3M_FPW) + wave * S3M_FPW;
    for (int fi = 0; fi < S3M_FPW; ++fi) {
        const int frame = frame0 + fi;
        const bool live = frame < nf;                                     // the barriers below stay uniform
        cplx v[4];
        const long start = (long)frame * MEL_HOP - MEL_NFFT / 2;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int p = lane + 64 * r;
            float a0 = 0.0f, a1 = 0.0f;
            if (live && p < MEL_NFFT / 2) {
                const long i0 = start + 2 * p, i1 = i0 + 1;             // reflect pad with the reference's clamps (:138-150)
                long j0 = i0 < 0 ? -i0 : (i0 >= n ? 2L * n - 2 - i0 : i0);
                long j1 = i1 < 0 ? -i1 : (i1 >= n ? 2L * n - 2 - i1 : i1);
                j0 = j0 < 0 ? 0 : (j0 > n - 1 ? n - 1 : j0);
                j1 = j1 < 0 ? 0 : (j1 > n - 1 ? n - 1 : j1);
                a0 = x[j0] * s_tab[T_HANN + 2 * p];
                a1 = x[j1] * s_tab[T_HANN + 2 * p + 1];
            }
            v[r] = {a0, a1};
        }
        melc_frame_power(v, lane, s_buf[wave][0], s_buf[wave][1], s_pow[wave], tw256, tw512, scale2);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int m = lane + 64 * h;
            const float lg = log10f(fmaxf(melc_filter(s_tab, s_pow[wave], m), 1e-10f));
            if (live) {
                out[(long)frame * MEL_NMELS + m] = lg;
                vmax = fmaxf(vmax, lg);
            }
        }
        __syncthreads();
    }
    vmax = wave_max(vmax);
    if (lane == 0) s_max[wave] = vmax;
    __syncthreads();
    if (tid == 0) {
        const float m = fmaxf(fmaxf(s_max[0], s_max[1]), fmaxf(s_max[2], s_max[3]));
        if (m > -INFINITY) atomicMax(&gmax[b], s3_ordered(m));
    }
}

// raw [frames][128] -> melf: clip b's [128][T] at 128 frame_off[b]; max(x, clip max - 8), (x + 4) / 4 (:209-218)
__global__ __launch_bounds__(256) void s3_whisper_finalize_kernel(const float* __restrict__ raw, const unsigned* __restrict__ gmax,
                                                                  const int* __restrict__ n_samples, const int* __restrict__ frame_off,
                                                                  float* __restrict__ melf) {
    __shared__ float tile[64][MEL_NMELS + 1];
    const int b = blockIdx.y, T = n_samples[b] / MEL_HOP, t0 = blockIdx.x * 64, tid = threadIdx.x;
    if (t0 >= T) return;
    const float floor_v = s3_unordered(gmax[b]) - 8.0f;
    const float* src = raw + (long)frame_off[b] * MEL_NMELS;
    for (int i = tid; i < 64 * MEL_NMELS; i += 256) {
        const int tt = i >> 7, m = i & 127;
        const float v = (t0 + tt < T) ? src[(long)(t0 + tt) * MEL_NMELS + m] : 0.0f;
        tile[tt][m] = (fmaxf(v, floor_v) + 4.0f) * 0.25f;
    }
    __syncthreads();
    float* dst = melf + (long)frame_off[b] * MEL_NMELS;
    for (int i = tid; i < 64 * MEL_NMELS; i += 256) {
        const int m = i >> 6, tt = i & 63;
        if (t0 + tt < T) dst[(long)m * T + t0 + tt] = tile[tt][m];
    }
}

// melf (per clip [128][T]) -> time-major bf16 rows [frame][128], the first stem's operand (SpeechTokenizer.swift:281)
__global__ __launch_bounds__(256) void s3_mel_rows_kernel(const float* __restrict__ melf, const int* __restrict__ frame_off,
                                                          const int* __restrict__ n_frames, bf16_t* __restrict__ melb) {
    __shared__ float tile[64][MEL_NMELS + 1];
    const int b = blockIdx.y, T = n_frames[b], t0 = blockIdx.x * 64, tid = threadIdx.x;
    if (t0 >= T) return;
    const float* src = melf + (long)frame_off[b] * MEL_NMELS;
    for (int i = tid; i < 64 * MEL_NMELS; i += 256) {
        const int m = i >> 6, tt = i & 63;
        tile[tt][m] = (t0 + tt < T) ? src[(long)m * T + t0 + tt] : 0.0f;
    }
    __syncthreads();
    bf16_t* dst = melb + (long)frame_off[b] * MEL_NMELS;
    for (int i = tid; i < 64 * MEL_NMELS; i += 256) {
        const int tt = i >> 7, m = i & 127;
        if (t0 + tt < T) dst[(long)(t0 + tt) * MEL_NMELS + m] = f32_to_bf16(tile[tt][m]);
    }
}

// =====================================================================================================================================
// kernel: flow mel at 24 kHz (FlowMelExtractor.swift:142-229)
// =====================================================================================================================================
constexpr int FM_FPB = 4;                  // frames per workgroup, one after the other

// One workgroup of 256 threads per frame: the 2048-point real FFT of the windowed, zero-padded frame as a 1024-point complex Stockham
// radix-4 transform (five passes, Ns = 1 .. 256, ping-pong between two LDS images, 4 points per thread: mel_core.h's form at N = 1024),
// the even / odd split, magnitude sqrt(re^2 + im^2 + 1e-9), the sparse 80-row filterbank (ascending bins), ln(max(., 1e-5)).
// out: clip b's [80][T] at out_off[b].  Reads of pcm are clamped to [0, n); a clip under 480 samples has no frame.  LDS 20 KiB.
__global__ __launch_bounds__(256) void s3_flow_mel_kernel(const float* __restrict__ pcm, const long* __restrict__ pcm_off,
                                                          const int* __restrict__ n_samples, const long* __restrict__ out_off,
                                                          const float* __restrict__ hann, const float2* __restrict__ tw1024,
                                                          const float2* __restrict__ tw2048, const int* __restrict__ fbi,
                                                          const float* __restrict__ fbw, float* __restrict__ out) {
    __shared__ float2 s_buf[2][1024];
    __shared__ float s_mag[FM_BINS + 3];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int n = n_samples[b], T = n >= FM_HOP ? n / FM_HOP : 0;
    const float* x = pcm + pcm_off[b];
    float* o = out + out_off[b];
    for (int fi = 0; fi < FM_FPB; ++fi) {
        const int frame = blockIdx.x * FM_FPB + fi;
        if (frame >= T) break;                                            // uniform over the workgroup
        cplx v[4];
        const long start = (long)frame * FM_HOP - FM_PAD;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int p = tid + 256 * r;                                  // packed point: samples 2 p, 2 p + 1 of the 2048-sample frame
            float a0 = 0.0f, a1 = 0.0f;
            if (p < FM_NFFT / 2) {
                const long i0 = start + 2 * p, i1 = i0 + 1;             // reflect pre-pad 720 with the reference's clamps (:148-160)
                long j0 = i0 < 0 ? -i0 : (i0 >= n ? 2L * n - 2 - i0 : i0);
                long j1 = i1 < 0 ? -i1 : (i1 >= n ? 2L * n - 2 - i1 : i1);
                j0 = j0 < 0 ? 0 : (j0 > n - 1 ? n - 1 : j0);
                j1 = j1 < 0 ? 0 : (j1 > n - 1 ? n - 1 : j1);
                a0 = x[j0] * hann[2 * p];
                a1 = x[j1] * hann[2 * p + 1];
            }
            v[r] = {a0, a1};
        }
        float2* src = s_buf[0];
        float2* dst = s_buf[1];
#pragma unroll
        for (int pass = 0; pass < 5; ++pass) {
            const int Ns = 1 << (2 * pass);
            if (pass > 0) {
#pragma unroll
                for (int r = 0; r < 4; ++r) { const float2 t = src[tid + 256 * r]; v[r] = {t.x, t.y}; }
            }
            const int k = tid & (Ns - 1);
            const int tstep = k * (256 / Ns);                             // twiddle w1024^(tstep r)
#pragma unroll
            for (int r = 1; r < 4; ++r) {
                const float2 t = tw1024[(tstep * r) & 1023];
                v[r] = cmul(v[r], {t.x, t.y});
            }
            const cplx t0 = {v[0].re + v[2].re, v[0].im + v[2].im};
            const cplx t1 = {v[0].re - v[2].re, v[0].im - v[2].im};
            const cplx t2 = {v[1].re + v[3].re, v[1].im + v[3].im};
            const cplx t3 = {v[1].im - v[3].im, -(v[1].re - v[3].re)};    // (v1 - v3) (-i)
            const int base = (tid / Ns) * Ns * 4 + k;
            dst[base] = make_float2(t0.re + t2.re, t0.im + t2.im);
            dst[base + Ns] = make_float2(t1.re + t3.re, t1.im + t3.im);
            dst[base + 2 * Ns] = make_float2(t0.re - t2.re, t0.im - t2.im);
            dst[base + 3 * Ns] = make_float2(t1.re - t3.re, t1.im - t3.im);
            __syncthreads();
            float2* tmp = src; src = dst; dst = tmp;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {                                     // src holds Z[0 .. 1023]
            const int k = tid + 256 * r;
            const float2 zk = src[k], zn = src[(1024 - k) & 1023];
            const float er = 0.5f * (zk.x + zn.x), ei = 0.5f * (zk.y - zn.y);
            const float orr = 0.5f * (zk.y + zn.y), oi = -0.5f * (zk.x - zn.x);
            const float2 w = tw2048[k];
            const float xr = er + (orr * w.x - oi * w.y), xi = ei + (orr * w.y + oi * w.x);
            s_mag[k] = sqrtf(xr * xr + xi * xi + 1e-9f);                  // magnitude, not power (:199-205)
            if (k == 0) {
                const float nr = er - orr;                                // Nyquist: E[0] - O[0]
                s_mag[1024] = sqrtf(nr * nr + 1e-9f);
            }
        }
        __syncthreads();
        if (tid < FM_MELS) {
            const int s0 = fbi[tid], len = fbi[FM_MELS + tid], wo = fbi[2 * FM_MELS + tid];
            float acc = 0.0f;
            for (int i = 0; i < len; ++i) acc += s_mag[s0 + i] * fbw[wo + i];
            o[(long)tid * T + frame] = logf(fmaxf(acc, 1e-5f));           // :216-222
        }
        __syncthreads();
    }
}

// =====================================================================================================================================
// kernels and GEMM functors of the tokenizer (SpeechTokenizer.swift)
// =====================================================================================================================================
// Conv1d k = 3, stride 2, pad 1 over time-major bf16 rows of ragged clips as an implicit GEMM (:255-262, :282-283): K index = tap C + ci,
// which is the stored [out][k][in] weight row.  info[m] = (input row of tap 0 = clip's first row + 2 t - 1, mask of the taps inside the
// clip): the three taps are 3 C contiguous elements from there, a tap outside the clip is a zero chunk.  C is a multiple of 8.
struct AS3Stem {
    const bf16_t* x;
    const int2* info;
    int C, M;
    static constexpr bool no_p8 = true;
    struct Row { const bf16_t* base; unsigned mask; };
    __device__ __forceinline__ Row row_init(int m) const {
        if (m >= M) return {nullptr, 0u};
        const int2 i = info[m];
        return {x + (long)i.x * C, (unsigned)i.y};
    }
    __device__ __forceinline__ const bf16_t* addr(const Row& r, int k) const {
        if (!r.base || k >= 3 * C) return nullptr;
        const int tap = (k >= C) + (k >= 2 * C);
        if (!((r.mask >> tap) & 1u)) return nullptr;
        return r.base + k;
    }
    __device__ __forceinline__ uint4 load(const Row& r, int k) const {
        const bf16_t* p = addr(r, k);
        return p ? *reinterpret_cast<const uint4*>(p) : make_uint4(0, 0, 0, 0);
    }
    struct KT { int k; };
    __device__ __forceinline__ KT ktile(int k0, int c8) const { return {k0 + c8}; }
    __device__ __forceinline__ const bf16_t* addr_kt(const Row& r, const KT& t) const { return addr(r, t.k); }
};

__device__ __forceinline__ float4 s3_add4(float4 v, const float* b) {
    const float4 c = *reinterpret_cast<const float4*>(b);
    return make_float4(v.x + c.x, v.y + c.y, v.z + c.z, v.w + c.w);
}
// conv2: gelu(acc + bias) starts the f32 residual stream (:283)
struct EpiS3Stem2 {
    float* x; const float* bias;
    __device__ __forceinline__ void operator()(int m, int n, float4 v) const {
        v = s3_add4(v, bias + n);
        v = make_float4(gelu_erf(v.x), gelu_erf(v.y), gelu_erf(v.z), gelu_erf(v.w));
        *reinterpret_cast<float4*>(x + (long)m * S3_DIM + n) = v;
    }
};
// q|k|v: acc + bias (key's is zero), RoPE on every head of q and of k (:172-185), -> bf16.  The rows of W_q and W_k are permuted at load
// inside each head so that the split-half pair (i, i + 32) sits in columns (2 i, 2 i + 1): the rotation below is the adjacent-pair form.
struct EpiS3QkvRope {
    bf16_t* out; const float* bias; const int* pos; const float *cs, *sn;
    __device__ __forceinline__ void operator()(int m, int n, float4 v) const {
        v = s3_add4(v, bias + n);
        if (n < 2 * S3_DIM) {
            const int i = (n & (S3_HD - 1)) >> 1;
            const float* c = cs + (long)pos[m] * (S3_HD / 2) + i;
            const float* s = sn + (long)pos[m] * (S3_HD / 2) + i;
            v = make_float4(v.x * c[0] - v.y * s[0], v.x * s[0] + v.y * c[0], v.z * c[1] - v.w * s[1], v.z * s[1] + v.w * c[1]);
        }
        *reinterpret_cast<uint2*>(out + (long)m * (3 * S3_DIM) + n) = pack_bf16x4(v);
    }
};

// FSMN memory (:162-170): x[m][c] += v[m][c] + sum_j w[c][j] v[m - 15 + j][c] over the taps inside the clip, v = the bf16 v third of
// q|k|v (un-rotated, before the head split), f32 sums, taps ascending.  A workgroup takes 32 rows x 128 channels and stages the 62 rows
// it reads in LDS (15.5 KiB); rows outside [0, rows) are zeros, rows of a neighbouring clip are masked by info[m] = (position, length).
// Runs ahead of the o-projection, whose epilogue adds its product into the same stream.
constexpr int FS_ROWS = 32, FS_CH = 128;
__global__ __launch_bounds__(256) void s3_fsmn_kernel(const bf16_t* __restrict__ qkv, const int2* __restrict__ info, const float* __restrict__ w,
                                                      int rows, float* __restrict__ xs) {
    __shared__ __attribute__((aligned(16))) bf16_t tile[FS_ROWS + S3_FSMN_K - 1][FS_CH];
    const int tid = threadIdx.x, m0 = blockIdx.x * FS_ROWS, c0 = blockIdx.y * FS_CH;
    for (int i = tid; i < (FS_ROWS + S3_FSMN_K - 1) * (FS_CH / 8); i += 256) {
        const int r = i / (FS_CH / 8), ch = (i % (FS_CH / 8)) * 8, g = m0 - S3_FSMN_PAD + r;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (g >= 0 && g < rows) v = *reinterpret_cast<const uint4*>(qkv + (long)g * (3 * S3_DIM) + 2 * S3_DIM + c0 + ch);
        *reinterpret_cast<uint4*>(&tile[r][ch]) = v;
    }
    __syncthreads();
    const int c = tid & (FS_CH - 1), r0 = (tid >> 7) * (FS_ROWS / 2);
    float wt[S3_FSMN_K], v[FS_ROWS / 2 + S3_FSMN_K - 1];                  // a thread's channel over its 16 rows: 46 values, read once
#pragma unroll
    for (int j = 0; j < S3_FSMN_K; ++j) wt[j] = w[(long)(c0 + c) * S3_FSMN_K + j];
#pragma unroll
    for (int i = 0; i < FS_ROWS / 2 + S3_FSMN_K - 1; ++i) v[i] = bf16_to_f32(tile[r0 + i][c]);
#pragma unroll
    for (int rr = 0; rr < FS_ROWS / 2; ++rr) {
        const int m = m0 + r0 + rr;
        if (m < rows) {
            const int2 tl = info[m];
            const int jlo = S3_FSMN_PAD - tl.x, jhi = tl.y - tl.x + S3_FSMN_PAD;  // 0 <= t - 15 + j < L
            float acc = 0.0f;
#pragma unroll
            for (int j = 0; j < S3_FSMN_K; ++j)
                if (j >= jlo && j < jhi) acc += wt[j] * v[rr + j];
            const float mem = acc + v[rr + S3_FSMN_PAD];
            xs[(long)m * S3_DIM + c0 + c] += mem;
        }
    }
}

// FSQ (:70-94), one wave per row: the 8 f32 dot products of K = 1280 (a lane sums its 20 terms in ascending k, then the wave's xor tree),
// bias, tanh, x 0.999, round to nearest even, + 1, base-3 pack.  Writes the projections [row][8] and the code.
__global__ __launch_bounds__(256) void s3_fsq_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                     int rows, float* __restrict__ proj, int* __restrict__ codes) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float4* xr = reinterpret_cast<const float4*>(x + (long)row * S3_DIM);
    float acc[S3_FSQ];
#pragma unroll
    for (int o = 0; o < S3_FSQ; ++o) acc[o] = 0.0f;
#pragma unroll
    for (int i = 0; i < S3_DIM / 256; ++i) {
        const float4 v = xr[lane + 64 * i];
#pragma unroll
        for (int o = 0; o < S3_FSQ; ++o) {
            const float4 u = reinterpret_cast<const float4*>(w + (long)o * S3_DIM)[lane + 64 * i];
            acc[o] += v.x * u.x;
            acc[o] += v.y * u.y;
            acc[o] += v.z * u.z;
            acc[o] += v.w * u.w;
        }
    }
    int code = 0, p = 1;
#pragma unroll
    for (int o = 0; o < S3_FSQ; ++o) {
        const float y = wave_sum(acc[o]) + bias[o];
        if (lane == 0) proj[(long)row * S3_FSQ + o] = y;
        code += (int)(rintf(tanhf(y) * S3_FSQ_SCALE) + 1.0f) * p;
        p *= 3;
    }
    if (lane == 0) codes[row] = code;
}

// =====================================================================================================================================
// loader (host only)
// =====================================================================================================================================
namespace {
const char* const WHO = "speech tokenizer";
[[noreturn]] void refuse(int code, const std::string& m) { throw WeightLoadError(code, std::string(WHO) + ": " + m); }
}  // namespace

S3Weights s3_load_weights(const std::string& dir) {
    std::unique_ptr<SafeTensorsDir> st;
    try { st = std::make_unique<SafeTensorsDir>(dir, "speech_tokenizer.safetensors"); }
    catch (const std::exception& ex) { refuse(QASR_ERR_IO, ex.what()); }
    S3Weights sw;
    const std::string B = "encoder.blocks.";
    while (sw.depth <= S3_MAX_DEPTH && st->entries.count(B + std::to_string(sw.depth) + ".attn.query.weight")) ++sw.depth;
    if (sw.depth < 1 || sw.depth > S3_MAX_DEPTH) refuse(QASR_ERR_IO, "missing key " + B + "0.attn.query.weight (depth 1.." + std::to_string(S3_MAX_DEPTH) + ")");
    std::vector<std::pair<std::string, std::vector<int64_t>>> shapes = {                       // WeightLoading.swift:350-398
        {"encoder.conv1.weight", {S3_DIM, 3, S3_MELS}}, {"encoder.conv1.bias", {S3_DIM}},
        {"encoder.conv2.weight", {S3_DIM, 3, S3_DIM}}, {"encoder.conv2.bias", {S3_DIM}},
        {"quantizer._codebook.project_down.weight", {S3_FSQ, S3_DIM}}, {"quantizer._codebook.project_down.bias", {S3_FSQ}}};
    for (int i = 0; i < sw.depth; ++i) {
        const std::string p = B + std::to_string(i) + ".";
        for (const char* n : {"attn.query", "attn.key", "attn.value", "attn.out"}) {
            shapes.push_back({p + n + ".weight", {S3_DIM, S3_DIM}});
            if (std::string(n) != "attn.key") shapes.push_back({p + n + ".bias", {S3_DIM}});   // key has no bias: one in the file is an unknown key
        }
        shapes.push_back({p + "attn.fsmn_block.weight", {S3_DIM, S3_FSMN_K, 1}});
        for (const char* n : {"attn_ln", "mlp_ln"}) {
            shapes.push_back({p + n + ".weight", {S3_DIM}});
            shapes.push_back({p + n + ".bias", {S3_DIM}});
        }
        shapes.push_back({p + "mlp.0.weight", {S3_FF, S3_DIM}});
        shapes.push_back({p + "mlp.0.bias", {S3_FF}});
        shapes.push_back({p + "mlp.2.weight", {S3_DIM, S3_FF}});
        shapes.push_back({p + "mlp.2.bias", {S3_DIM}});
    }
    sw.f = load_checked_f32(*st, WHO, shapes, true);
    return sw;
}

// =====================================================================================================================================
// host object
// =====================================================================================================================================
namespace {
struct Pack {
    std::vector<bf16_t> w;
    std::vector<float> f;
    std::vector<int> i;
    size_t put_f(const std::vector<float>& v) {
        const size_t o = f.size();
        f.insert(f.end(), v.begin(), v.end());
        while (f.size() % 4) f.push_back(0.0f);
        return o;
    }
    size_t put_w(const std::vector<float>& v) {
        const size_t o = w.size();
        for (float x : v) w.push_back(f32_to_bf16_host(x));
        while (w.size() % 8) w.push_back(0);
        return o;
    }
};
// Slaney mel <-> Hz in Float as FlowMelExtractor.swift:58-81 writes them
float fm_hz_to_mel(float hz) {
    const float f_sp = 200.0f / 3.0f, min_log_hz = 1000.0f, min_log_mel = min_log_hz / f_sp, log_step = logf(6.4f) / 27.0f;
    return hz < min_log_hz ? hz / f_sp : min_log_mel + logf(hz / min_log_hz) / log_step;
}
float fm_mel_to_hz(float mel) {
    const float f_sp = 200.0f / 3.0f, min_log_hz = 1000.0f, min_log_mel = min_log_hz / f_sp, log_step = logf(6.4f) / 27.0f;
    return mel < min_log_mel ? f_sp * mel : min_log_hz * expf(log_step * (mel - min_log_mel));
}
}  // namespace

S3Tokenizer::S3Tokenizer(int device, const S3Weights& sw, long max_tokens, hipStream_t work) : device_(device), depth_(sw.depth), max_tokens_(max_tokens) {
    Pack b;
    const auto& T = sw.f.t;
    auto vec = [&](const std::string& k) -> const std::vector<float>& { return T.at(k); };
    auto dense = [&](const std::string& stem, int N, int K) {
        Dense d;
        d.w = b.put_w(vec(stem + ".weight"));
        d.bias = b.put_f(vec(stem + ".bias"));
        d.N = N; d.K = K;
        return d;
    };
    conv1_ = dense("encoder.conv1", S3_DIM, 3 * S3_MELS);                  // [1280][3][C]: row n is K = 3 C values, tap-major: the Wt image as stored
    conv2_ = dense("encoder.conv2", S3_DIM, 3 * S3_DIM);
    blocks_.resize(depth_);
    for (int i = 0; i < depth_; ++i) {
        const std::string p = "encoder.blocks." + std::to_string(i) + ".";
        Block& k = blocks_[i];
        // q | k | v with the rows of q and k permuted inside each head: new column 2 i <- i, 2 i + 1 <- i + 32
        std::vector<float> w((size_t)3 * S3_DIM * S3_DIM), bias((size_t)3 * S3_DIM, 0.0f);
        const std::vector<float>*src[3] = {&vec(p + "attn.query.weight"), &vec(p + "attn.key.weight"), &vec(p + "attn.value.weight")};
        const std::vector<float>*sb[3] = {&vec(p + "attn.query.bias"), nullptr, &vec(p + "attn.value.bias")};
        for (int part = 0; part < 3; ++part)
            for (int n = 0; n < S3_DIM; ++n) {
                const int j = n & (S3_HD - 1);
                const int from = part < 2 ? (n - j) + (j >> 1) + (j & 1) * (S3_HD / 2) : n;
                std::memcpy(&w[((size_t)part * S3_DIM + n) * S3_DIM], &(*src[part])[(size_t)from * S3_DIM], S3_DIM * sizeof(float));
                if (sb[part]) bias[(size_t)part * S3_DIM + n] = (*sb[part])[from];
            }
        k.qkv.w = b.put_w(w);
        k.qkv.bias = b.put_f(bias);
        k.qkv.N = 3 * S3_DIM; k.qkv.K = S3_DIM;
        k.o = dense(p + "attn.out", S3_DIM, S3_DIM);
        k.fc1 = dense(p + "mlp.0", S3_FF, S3_DIM);
        k.fc2 = dense(p + "mlp.2", S3_DIM, S3_FF);
        k.fsmn = b.put_f(vec(p + "attn.fsmn_block.weight"));               // [1280][31][1]
        k.ln1_g = b.put_f(vec(p + "attn_ln.weight"));
        k.ln1_b = b.put_f(vec(p + "attn_ln.bias"));
        k.ln2_g = b.put_f(vec(p + "mlp_ln.weight"));
        k.ln2_b = b.put_f(vec(p + "mlp_ln.bias"));
    }
    proj_w_ = b.put_f(vec("quantizer._codebook.project_down.weight"));
    proj_b_ = b.put_f(vec("quantizer._codebook.project_down.bias"));
    {   // RoPE base 10000 over 64 dims (:271-272): angle = position 10000^(-i / 32), Float of the f64 value
        std::vector<float> cs((size_t)max_tokens * (S3_HD / 2)), sn(cs.size());
        for (long p = 0; p < max_tokens; ++p)
            for (int i = 0; i < S3_HD / 2; ++i) {
                const double a = (double)p * std::pow(10000.0, -(double)i / (double)(S3_HD / 2));
                cs[(size_t)p * (S3_HD / 2) + i] = (float)std::cos(a);
                sn[(size_t)p * (S3_HD / 2) + i] = (float)std::sin(a);
            }
        rope_cos_ = b.put_f(cs);
        rope_sin_ = b.put_f(sn);
    }
    {   // flow mel tables: periodic Hann 1920 in Float (FlowMelExtractor.swift:41-44), twiddles, the sparse 80 x 1025 filterbank (:83-136)
        std::vector<float> hann(FM_NFFT), tw1(2 * 1024), tw2(2 * 1024);
        for (int i = 0; i < FM_NFFT; ++i) hann[i] = 0.5f * (1.0f - cosf(2.0f * (float)M_PI * (float)i / (float)FM_NFFT));
        for (int k = 0; k < 1024; ++k) {
            const double a1 = -2.0 * M_PI * k / 1024.0, a2 = -2.0 * M_PI * k / 2048.0;
            tw1[2 * k] = (float)std::cos(a1); tw1[2 * k + 1] = (float)std::sin(a1);
            tw2[2 * k] = (float)std::cos(a2); tw2[2 * k + 1] = (float)std::sin(a2);
        }
        const int npts = FM_MELS + 2;
        const float mel_min = fm_hz_to_mel(0.0f), mel_max = fm_hz_to_mel((float)FM_SR / 2.0f);
        std::vector<float> pts(npts), fbw;
        for (int i = 0; i < npts; ++i) pts[i] = fm_mel_to_hz(mel_min + (mel_max - mel_min) * ((float)i / (float)(npts - 1)));
        std::vector<int> fbi(3 * FM_MELS, 0);
        for (int m = 0; m < FM_MELS; ++m) {
            const float left = pts[m], center = pts[m + 1], right = pts[m + 2], enorm = 2.0f / std::max(right - left, 1e-12f);
            std::vector<float> row(FM_BINS, 0.0f);
            int first = -1, last = -1;
            for (int k = 0; k < FM_BINS; ++k) {
                const float hz = (float)k * (float)FM_SR / (float)FM_PADDED;
                float v = 0.0f;
                if (hz >= left && hz <= center) v = (hz - left) / std::max(center - left, 1e-12f);
                else if (hz > center && hz <= right) v = (right - hz) / std::max(right - center, 1e-12f);
                row[k] = v * enorm;
                if (row[k] != 0.0f) { if (first < 0) first = k; last = k; }
            }
            fbi[m] = first < 0 ? 0 : first;
            fbi[FM_MELS + m] = first < 0 ? 0 : last - first + 1;
            fbi[2 * FM_MELS + m] = (int)fbw.size();
            for (int k = fbi[m]; k < fbi[m] + fbi[FM_MELS + m]; ++k) fbw.push_back(row[k]);
        }
        fm_hann_ = b.put_f(hann);
        fm_tw1024_ = b.put_f(tw1);
        fm_tw2048_ = b.put_f(tw2);
        fm_fbw_ = b.put_f(fbw);
        fm_fbi_ = b.i.size();
        b.i.insert(b.i.end(), fbi.begin(), fbi.end());
    }
    QASR_HIP(hipSetDevice(device_));
    QASR_HIP(hipStreamCreateWithFlags(&own_, hipStreamNonBlocking));
    work_ = work ? work : own_;
    for (auto& e : ev_) QASR_HIP(hipEventCreate(&e));
    auto up = [&](DevBuf& d, const void* src, size_t bytes) {
        d.alloc(bytes);
        if (bytes) QASR_HIP(hipMemcpy(d.p, src, bytes, hipMemcpyHostToDevice));
    };
    param_bytes_ = sw.f.disk_bytes;
    up(d_w_, b.w.data(), b.w.size() * sizeof(bf16_t));
    up(d_f_, b.f.data(), b.f.size() * sizeof(float));
    up(d_i_, b.i.data(), b.i.size() * sizeof(int));
    mel_tab_.build(1.0f);                                                  // the reference undoes vDSP's factor (WhisperMelExtractor.swift:181-189): true DFT power
    const size_t M = (size_t)max_tokens, H2 = sizeof(bf16_t), F4 = sizeof(float);
    d_cu_.alloc((M + 1) * sizeof(int));
    d_pos_.alloc(M * sizeof(int));
    d_info_.alloc(M * sizeof(int2));
    d_stem1_.alloc(2 * M * sizeof(int2));
    d_stem2_.alloc(M * sizeof(int2));
    d_melb_.alloc(4 * M * S3_MELS * H2);                                   // T <= 4 tokens, T1 <= 2 tokens per clip
    d_h1_.alloc(2 * M * S3_DIM * H2);
    d_xs_.alloc(M * S3_DIM * F4);
    d_a_.alloc(M * S3_DIM * H2);
    d_attn_.alloc(M * S3_DIM * H2);
    d_qkv_.alloc(M * 3 * S3_DIM * H2);
    d_u_.alloc(M * S3_FF * H2);
    d_proj_.alloc(M * S3_FSQ * F4);
    d_codes_.alloc(M * sizeof(int));
}

S3Tokenizer::~S3Tokenizer() {
    if (work_) (void)hipStreamSynchronize(work_);
    for (auto& e : ev_) if (e) (void)hipEventDestroy(e);
    mel_tab_.release();
    if (own_) (void)hipStreamDestroy(own_);
}

void S3Tokenizer::unload() {
    if (!loaded_) return;
    QASR_HIP(hipSetDevice(device_));
    QASR_HIP(hipStreamSynchronize(work_));
    for (DevBuf* b : {&d_w_, &d_f_, &d_i_, &d_cu_, &d_pos_, &d_info_, &d_stem1_, &d_stem2_, &d_melb_, &d_h1_, &d_xs_, &d_a_, &d_attn_, &d_qkv_, &d_u_, &d_proj_,
                      &d_codes_, &d_pcm_, &d_tab_, &d_raw_, &d_gmax_, &d_melf_, &d_fm_out_, &d_rows_})
        b->release();
    mel_tab_.release();
    loaded_ = false;
}

void S3Tokenizer::check_loaded() const {
    if (!loaded_) throw NotLoaded("speech tokenizer: model unloaded");
}

void S3Tokenizer::grow(DevBuf& b, size_t bytes) {
    if (b.bytes < bytes) b.alloc(bytes + bytes / 4);
}

// ---- front ends ----------------------------------------------------------------------------------------------------------------------
// the Whisper-style mel of n pcm clips into d_melf_ (clip i's [128][T] at 128 frame_off[i]); the stream is idle on entry
void S3Tokenizer::front_end(const S3Clip* c, int n, const std::vector<int>& frame_off) {
    std::vector<long> off(n);
    std::vector<int> ns(n);
    long total = 0;
    int max_T = 0;
    for (int i = 0; i < n; ++i) {
        off[i] = total;
        ns[i] = (int)c[i].n;
        total += (c[i].n + 3) / 4 * 4;
        max_T = std::max<int>(max_T, (int)s3_whisper_frames((size_t)c[i].n));
    }
    std::vector<float> pcm((size_t)total, 0.0f);
    for (int i = 0; i < n; ++i) std::memcpy(&pcm[(size_t)off[i]], c[i].pcm, (size_t)c[i].n * sizeof(float));
    const size_t frames = (size_t)frame_off[n];
    grow(d_pcm_, pcm.size() * sizeof(float));
    grow(d_tab_, (size_t)n * (sizeof(long) + 2 * sizeof(int)));
    grow(d_raw_, frames * MEL_NMELS * sizeof(float));
    grow(d_melf_, frames * MEL_NMELS * sizeof(float));
    grow(d_gmax_, (size_t)n * sizeof(unsigned));
    long* d_off = d_tab_.as<long>();
    int* d_ns = reinterpret_cast<int*>(d_off + n);
    int* d_fo = d_ns + n;
    QASR_HIP(hipMemcpy(d_pcm_.p, pcm.data(), pcm.size() * sizeof(float), hipMemcpyHostToDevice));
    QASR_HIP(hipMemcpy(d_off, off.data(), (size_t)n * sizeof(long), hipMemcpyHostToDevice));
    QASR_HIP(hipMemcpy(d_ns, ns.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice));
    QASR_HIP(hipMemcpy(d_fo, frame_off.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice));
    QASR_HIP(hipMemsetAsync(d_gmax_.p, 0, (size_t)n * sizeof(unsigned), work_));
    hipLaunchKernelGGL(s3_whisper_frames_kernel, dim3((unsigned)cdiv(max_T, S3M_WAVES * S3M_FPW), (unsigned)n), dim3(S3M_WAVES * 64), 0, work_, mel_tab_.dev,
                       d_pcm_.as<float>(), d_off, d_ns, d_fo, d_raw_.as<float>(), d_gmax_.as<unsigned>());
    hipLaunchKernelGGL(s3_whisper_finalize_kernel, dim3((unsigned)cdiv(max_T, 64), (unsigned)n), dim3(256), 0, work_, d_raw_.as<float>(),
                       d_gmax_.as<unsigned>(), d_ns, d_fo, d_melf_.as<float>());
    QASR_HIP(hipGetLastError());
}

void S3Tokenizer::whisper_mel(const float* pcm, long n, float* out) {
    check_loaded();
    if (n < MEL_HOP || n > S3_MAX_SAMPLES) throw std::invalid_argument("speech tokenizer: a 16 kHz clip holds 160.." + std::to_string(S3_MAX_SAMPLES) + " samples");
    QASR_HIP(hipSetDevice(device_));
    QASR_HIP(hipStreamSynchronize(work_));
    S3Clip c;
    c.pcm = pcm; c.n = n;
    const int T = (int)s3_whisper_frames((size_t)n);
    front_end(&c, 1, {0, T});
    QASR_HIP(hipMemcpyAsync(out, d_melf_.p, (size_t)T * MEL_NMELS * sizeof(float), hipMemcpyDeviceToHost, work_));
    QASR_HIP(hipStreamSynchronize(work_));
}

void S3Tokenizer::flow_mel(const float* const* pcm, const long* n, int B, float* const* out) {
    check_loaded();
    for (int i = 0; i < B; ++i)
        if (n[i] < FM_HOP || n[i] > S3_MAX_SAMPLES)
            throw std::invalid_argument("speech tokenizer: a 24 kHz clip holds 480.." + std::to_string(S3_MAX_SAMPLES) + " samples");
    if (B <= 0) return;
    QASR_HIP(hipSetDevice(device_));
    QASR_HIP(hipStreamSynchronize(work_));
    std::vector<long> off(B), ooff(B + 1, 0);
    std::vector<int> ns(B);
    long total = 0;
    int max_T = 0;
    for (int i = 0; i < B; ++i) {
        off[i] = total;
        ns[i] = (int)n[i];
        total += (n[i] + 3) / 4 * 4;
        const long T = (long)s3_flow_frames((size_t)n[i]);
        ooff[i + 1] = ooff[i] + T * FM_MELS;
        max_T = std::max<int>(max_T, (int)T);
    }
    std::vector<float> h((size_t)total, 0.0f);
    for (int i = 0; i < B; ++i) std::memcpy(&h[(size_t)off[i]], pcm[i], (size_t)n[i] * sizeof(float));
    grow(d_pcm_, h.size() * sizeof(float));
    grow(d_tab_, (size_t)B * (2 * sizeof(long) + sizeof(int)));
    grow(d_fm_out_, (size_t)ooff[B] * sizeof(float));
    long* d_off = d_tab_.as<long>();
    long* d_ooff = d_off + B;
    int* d_ns = reinterpret_cast<int*>(d_ooff + B);
    QASR_HIP(hipMemcpy(d_pcm_.p, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
    QASR_HIP(hipMemcpy(d_off, off.data(), (size_t)B * sizeof(long), hipMemcpyHostToDevice));
    QASR_HIP(hipMemcpy(d_ooff, ooff.data(), (size_t)B * sizeof(long), hipMemcpyHostToDevice));
    QASR_HIP(hipMemcpy(d_ns, ns.data(), (size_t)B * sizeof(int), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(s3_flow_mel_kernel, dim3((unsigned)cdiv(max_T, FM_FPB), (unsigned)B), dim3(256), 0, work_, d_pcm_.as<float>(), d_off, d_ns, d_ooff,
                       F(fm_hann_), reinterpret_cast<const float2*>(F(fm_tw1024_)), reinterpret_cast<const float2*>(F(fm_tw2048_)),
                       d_i_.as<int>() + fm_fbi_, F(fm_fbw_), d_fm_out_.as<float>());
    QASR_HIP(hipGetLastError());
    for (int i = 0; i < B; ++i)
        QASR_HIP(hipMemcpyAsync(out[i], d_fm_out_.as<float>() + ooff[i], (size_t)(ooff[i + 1] - ooff[i]) * sizeof(float), hipMemcpyDeviceToHost, work_));
    QASR_HIP(hipStreamSynchronize(work_));
}

// ---- a pass --------------------------------------------------------------------------------------------------------------------------
void S3Tokenizer::pass(const S3Clip* c, int n) {
    QASR_HIP(hipSetDevice(device_));
    QASR_HIP(hipStreamSynchronize(work_));
    hipStream_t s = work_;
    const bool from_pcm = c[0].pcm != nullptr;
    std::vector<int> off0(n + 1, 0), off1(n + 1, 0), cu(n + 1, 0), len0(n);
    int max_len = 0, max_T = 0;
    for (int i = 0; i < n; ++i) {
        const int T = (int)c[i].T, T1 = (T - 1) / 2 + 1, T2 = (T1 - 1) / 2 + 1;
        len0[i] = T;
        off0[i + 1] = off0[i] + T;
        off1[i + 1] = off1[i] + T1;
        cu[i + 1] = cu[i] + T2;
        max_len = std::max(max_len, T2);
        max_T = std::max(max_T, T);
    }
    const int R0 = off0[n], R1 = off1[n], R = cu[n];
    if (R > max_tokens_) throw std::length_error("speech tokenizer: a pass exceeds its buffers");
    std::vector<int2> st1((size_t)R1), st2((size_t)R), info((size_t)R);
    std::vector<int> pos((size_t)R);
    auto taps = [](int t, int L) { unsigned m = 0; for (int k = 0; k < 3; ++k) if (2 * t - 1 + k >= 0 && 2 * t - 1 + k < L) m |= 1u << k; return (int)m; };
    for (int i = 0; i < n; ++i) {
        const int T = len0[i], T1 = off1[i + 1] - off1[i], T2 = cu[i + 1] - cu[i];
        for (int t = 0; t < T1; ++t) st1[(size_t)off1[i] + t] = make_int2(off0[i] + 2 * t - 1, taps(t, T));
        for (int t = 0; t < T2; ++t) {
            st2[(size_t)cu[i] + t] = make_int2(off1[i] + 2 * t - 1, taps(t, T1));
            info[(size_t)cu[i] + t] = make_int2(t, T2);
            pos[(size_t)cu[i] + t] = t;
        }
    }
    QASR_HIP(hipMemcpy(d_cu_.p, cu.data(), cu.size() * sizeof(int), hipMemcpyHostToDevice));
    QASR_HIP(hipMemcpy(d_pos_.p, pos.data(), pos.size() * sizeof(int), hipMemcpyHostToDevice));
    QASR_HIP(hipMemcpy(d_info_.p, info.data(), info.size() * sizeof(int2), hipMemcpyHostToDevice));
    QASR_HIP(hipMemcpy(d_stem1_.p, st1.data(), st1.size() * sizeof(int2), hipMemcpyHostToDevice));
    QASR_HIP(hipMemcpy(d_stem2_.p, st2.data(), st2.size() * sizeof(int2), hipMemcpyHostToDevice));
    QASR_HIP(hipEventRecord(ev_[0], s));
    if (from_pcm) {
        front_end(c, n, off0);
    } else {
        std::vector<float> m((size_t)R0 * S3_MELS);
        for (int i = 0; i < n; ++i) std::memcpy(&m[(size_t)off0[i] * S3_MELS], c[i].mel, (size_t)len0[i] * S3_MELS * sizeof(float));
        grow(d_melf_, m.size() * sizeof(float));
        QASR_HIP(hipMemcpy(d_melf_.p, m.data(), m.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    // frame offsets and lengths of the clips for the row kernel
    DevBuf& rows_tab = d_rows_;
    grow(rows_tab, (size_t)2 * n * sizeof(int));
    QASR_HIP(hipMemcpy(rows_tab.p, off0.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice));
    QASR_HIP(hipMemcpy(rows_tab.as<int>() + n, len0.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(s3_mel_rows_kernel, dim3((unsigned)cdiv(max_T, 64), (unsigned)n), dim3(256), 0, s, d_melf_.as<float>(), rows_tab.as<int>(),
                       rows_tab.as<int>() + n, d_melb_.as<bf16_t>());
    QASR_HIP(hipEventRecord(ev_[1], s));
    float* xs = d_xs_.as<float>();
    bf16_t *a = d_a_.as<bf16_t>(), *attn = d_attn_.as<bf16_t>(), *qkv = d_qkv_.as<bf16_t>(), *u = d_u_.as<bf16_t>(), *h1 = d_h1_.as<bf16_t>();
    // stems (SpeechTokenizer.swift:281-283)
    gemm_nt(AS3Stem{d_melb_.as<bf16_t>(), d_stem1_.as<int2>(), S3_MELS, R1}, W(conv1_.w), conv1_.K, R1, S3_DIM, conv1_.K,
            EpiBiasActBf16F<1>{h1, S3_DIM, F(conv1_.bias)}, s);
    gemm_nt(AS3Stem{h1, d_stem2_.as<int2>(), S3_DIM, R}, W(conv2_.w), conv2_.K, R, S3_DIM, conv2_.K, EpiS3Stem2{xs, F(conv2_.bias)}, s);
    QASR_HIP(hipEventRecord(ev_[2], s));
    for (int i = 0; i < depth_; ++i) {                                     // :230-234
        const Block& b = blocks_[i];
        layernorm_f32p_launch(xs, F(b.ln1_g), F(b.ln1_b), a, R, S3_DIM, 1e-5f, 0, s);
        gemm_nt(ADense{a, S3_DIM, R, S3_DIM}, W(b.qkv.w), S3_DIM, R, 3 * S3_DIM, S3_DIM,
                EpiS3QkvRope{qkv, F(b.qkv.bias), d_pos_.as<int>(), F(rope_cos_), F(rope_sin_)}, s);
        hipLaunchKernelGGL(s3_fsmn_kernel, dim3((unsigned)cdiv(R, FS_ROWS), S3_DIM / FS_CH), dim3(256), 0, s, qkv, d_info_.as<int2>(), F(b.fsmn), R, xs);
        mha_attention_launch(qkv, d_cu_.as<int>(), n, max_len, S3_HEADS, S3_HD, attn, s);
        gemm_nt(ADense{attn, S3_DIM, R, S3_DIM}, W(b.o.w), S3_DIM, R, S3_DIM, S3_DIM, EpiResidF32F{xs, S3_DIM, F(b.o.bias)}, s);
        layernorm_f32p_launch(xs, F(b.ln2_g), F(b.ln2_b), a, R, S3_DIM, 1e-5f, 0, s);
        gemm_nt(ADense{a, S3_DIM, R, S3_DIM}, W(b.fc1.w), S3_DIM, R, S3_FF, S3_DIM, EpiBiasActBf16F<1>{u, S3_FF, F(b.fc1.bias)}, s);
        gemm_nt(ADense{u, S3_FF, R, S3_FF}, W(b.fc2.w), S3_FF, R, S3_DIM, S3_FF, EpiResidF32F{xs, S3_DIM, F(b.fc2.bias)}, s);
    }
    QASR_HIP(hipEventRecord(ev_[3], s));
    hipLaunchKernelGGL(s3_fsq_kernel, dim3((unsigned)cdiv(R, 4)), dim3(256), 0, s, xs, F(proj_w_), F(proj_b_), R, d_proj_.as<float>(), d_codes_.as<int>());
    QASR_HIP(hipEventRecord(ev_[4], s));
    QASR_HIP(hipGetLastError());
    for (int i = 0; i < n; ++i) {
        const size_t r0 = (size_t)cu[i], rows = (size_t)(cu[i + 1] - cu[i]);
        if (c[i].hidden) QASR_HIP(hipMemcpyAsync(c[i].hidden, xs + r0 * S3_DIM, rows * S3_DIM * sizeof(float), hipMemcpyDeviceToHost, s));
        if (c[i].proj) QASR_HIP(hipMemcpyAsync(c[i].proj, d_proj_.as<float>() + r0 * S3_FSQ, rows * S3_FSQ * sizeof(float), hipMemcpyDeviceToHost, s));
        if (c[i].codes) QASR_HIP(hipMemcpyAsync(c[i].codes, d_codes_.as<int>() + r0, rows * sizeof(int), hipMemcpyDeviceToHost, s));
    }
    QASR_HIP(hipStreamSynchronize(s));
    QASR_HIP(hipGetLastError());
    for (int k = 0; k < S3_STAGES; ++k) {
        float ms = 0.0f;
        QASR_HIP(hipEventElapsedTime(&ms, ev_[k], ev_[k + 1]));
        timing_[k] += ms;
    }
}

void S3Tokenizer::run(const std::vector<S3Clip>& clips) {
    check_loaded();
    for (float& t : timing_) t = 0.0f;
    std::vector<S3Clip> c = clips;
    for (size_t i = 0; i < c.size(); ++i) {
        const std::string who = "speech tokenizer: clip " + std::to_string(i);
        if ((c[i].pcm != nullptr) != (c[0].pcm != nullptr) || (!c[i].pcm && !c[i].mel)) throw std::invalid_argument(who + ": every clip of a call is pcm, or every clip is a mel");
        if (c[i].pcm) {
            if (c[i].n > S3_MAX_SAMPLES) throw std::invalid_argument(who + " is too long");
            c[i].T = c[i].n > 0 ? (long)s3_whisper_frames((size_t)c[i].n) : 0;
        }
        if (c[i].T < 1) throw std::invalid_argument(who + " is empty (a clip holds at least one mel frame: 160 samples)");
        const long tok = (long)s3_tokens((size_t)c[i].T);
        if (tok > max_tokens_)
            throw std::invalid_argument(who + " holds " + std::to_string(tok) + " tokens, more than max_tokens = " + std::to_string(max_tokens_));
    }
    for (size_t i = 0; i < c.size();) {                                    // passes end at clip boundaries
        size_t j = i;
        long total = 0;
        while (j < c.size() && total + (long)s3_tokens((size_t)c[j].T) <= max_tokens_) total += (long)s3_tokens((size_t)c[j++].T);
        pass(c.data() + i, (int)(j - i));
        i = j;
    }
}

}  // namespace qasr
