// xvec_qwen3tts.hip -- the Qwen3-TTS ECAPA-TDNN speaker encoder for gfx950 (xvec_qwen3tts.h).  f32 throughout, accurate logf / expf /
// tanhf / sqrtf, no atomics, no vendor BLAS or FFT.
//
// A pass holds clips back to back, channel-last: a clip of n samples owns T = n / 256 + 1 rows of every activation, start[clip] is its
// first row.  Two tile grids are laid over the rows, both starting again at every clip's first row, so a tile never spans two clips and
// a clip's tiles are the same wherever the clip sits: tiles of XV_TILE rows for the GEMMs and the reductions, tiles of XV_RES_TILE rows
// for the Res2Net chain.  Row and element indices are 64-bit.  The 22 launches of a pass, whatever it holds:
//   xv_mel_kernel       one workgroup per frame of any clip: the reflect pad by clamped index, Hann, a 1024-point real DFT in LDS (512-point
//                       complex Stockham radix 2 + even/odd split), magnitudes, the sparse HTK filterbank, log
//   xv_gemm_kernel      the house 64 x 64 f32 tile (16-deep k steps, one fmaf chain per output over k = tap-major, channel-minor), here on
//                       the clip-aligned tile grid: taps of a k > 1 conv outside the clip read exact zeros.  Epilogues: bias, ReLU or
//                       (+ per-clip context, tanh); optionally the tile's column sums or column maxima, rows added in order
//   xv_res2net_kernel   the seven chained k = 3 dilated 64 -> 64 convs of a block in one launch: a workgroup owns XV_RES_TILE rows of one
//                       clip plus 7 x dilation rows of halo per side, keeps the running 64-wide output in LDS and streams each stage's
//                       192 x 64 weights through LDS; stage s computes the rows still needed (the halo shrinks by one dilation per stage)
//   xv_se_apply_kernel  per tile: the clip's column means from the tile partials, 512 -> 128 ReLU -> 512 sigmoid, out = gate x + input
//   xv_asp_*_kernel     global variance partials | per-clip [mean | std] context of the attention's first layer | softmax sums and
//                       weighted sums | weighted variance partials
//   xv_fc_kernel        pooled [mean | std] of a clip from the partials, then fc
// Summation order: every GEMM / conv output is one thread's fmaf chain over k; every per-clip reduction is first summed over the rows of
// a tile in row order, then over the clip's tiles in tile order.  Nothing depends on a clip's place in the pass.
#include "xvec_qwen3tts.h"
#include "codec_shared.h"
#include <algorithm>
#include <cmath>
#include <cstring>

namespace qasr {

// ---- keys, tables (host) ------------------------------------------------------------------------------------------------------------
std::vector<std::pair<std::string, std::vector<int64_t>>> xvec_tensor_shapes(int64_t E) {
    std::vector<std::pair<std::string, std::vector<int64_t>>> s;
    const std::string P = "speaker_encoder.";
    auto conv = [&](const std::string& k, int64_t out, int64_t taps, int64_t in) {
        s.emplace_back(P + k + ".weight", std::vector<int64_t>{out, taps, in});
        s.emplace_back(P + k + ".bias", std::vector<int64_t>{out});
    };
    conv("blocks.0.conv", XV_C, 5, XV_NMELS);
    for (int b = 1; b <= 3; ++b) {
        const std::string p = "blocks." + std::to_string(b) + ".";
        conv(p + "tdnn1.conv", XV_C, 1, XV_C);
        for (int j = 0; j < 7; ++j) conv(p + "res2net_block.blocks." + std::to_string(j) + ".conv", XV_W, 3, XV_W);
        conv(p + "tdnn2.conv", XV_C, 1, XV_C);
        conv(p + "se_block.conv1", XV_SE, 1, XV_C);
        conv(p + "se_block.conv2", XV_C, 1, XV_SE);
    }
    conv("mfa.conv", XV_CAT, 1, XV_CAT);
    conv("asp.tdnn.conv", XV_ATT, 1, 3 * XV_CAT);
    conv("asp.conv", XV_CAT, 1, XV_ATT);
    conv("fc", E, 1, 2 * XV_CAT);
    return s;
}

std::vector<float> xvec_filterbank() {
    auto hz_to_mel = [](float hz) { return 2595.0f * log10f(1.0f + hz / 700.0f); };
    auto mel_to_hz = [](float mel) { return 700.0f * (powf(10.0f, mel / 2595.0f) - 1.0f); };
    const float mel_min = hz_to_mel(0.0f), mel_max = hz_to_mel(12000.0f);
    std::vector<float> pts(XV_NMELS + 2), fb((size_t)XV_NBINS * XV_NMELS, 0.0f);
    for (int i = 0; i < XV_NMELS + 2; ++i) pts[i] = mel_to_hz(mel_min + (float)i * (mel_max - mel_min) / (float)(XV_NMELS + 1));
    for (int m = 0; m < XV_NMELS; ++m) {
        const float lo = pts[m], ce = pts[m + 1], hi = pts[m + 2];
        for (int k = 0; k < XV_NBINS; ++k) {
            const float f = (float)k * (float)XV_RATE / (float)XV_NFFT;
            if (f >= lo && f <= ce && ce > lo) fb[(size_t)k * XV_NMELS + m] = (f - lo) / (ce - lo);
            else if (f > ce && f <= hi && hi > ce) fb[(size_t)k * XV_NMELS + m] = (hi - f) / (hi - ce);
        }
    }
    return fb;
}

// ---- kernels ------------------------------------------------------------------------------------------------------------------------
constexpr int XG_THREADS = 256, XG_T = XV_TILE, XG_K = 16;
constexpr int RS_HALO = 28, RS_ROWS = XV_RES_TILE + 2 * RS_HALO, RS_RP = RS_ROWS + 1;
enum { A_LIN = 0, A_RELU = 1, A_TANH_CTX = 2 };
enum { S_NONE = 0, S_SUM = 1, S_MAX = 2 };

// column c of the partials of tiles tb .. te - 1, in tile order
__device__ __forceinline__ float xv_tiles_sum(const float* __restrict__ part, int ld, int tb, int te, int c) {
    float s = 0.0f;
    for (int t = tb; t < te; ++t) s = s + part[(size_t)t * ld + c];
    return s;
}
__device__ __forceinline__ float xv_tiles_max(const float* __restrict__ part, int ld, int tb, int te, int c) {
    float s = -INFINITY;
    for (int t = tb; t < te; ++t) s = fmaxf(s, part[(size_t)t * ld + c]);
    return s;
}

struct xv_c { float re, im; };
__device__ __forceinline__ xv_c xv_cmul(xv_c a, float2 b) { return {a.re * b.x - a.im * b.y, a.re * b.y + a.im * b.x}; }

// SpeakerMel.compute for row m of the pass (frame m - start[clip] of its clip).  tw512 [256], tw1024 [512]: exp(-2 pi i k / 512), / 1024;
// filter f reads magnitudes fb_start[f] .. + fb_len[f] with weights fb_w[fb_off[f] ..].  mel [M][128].
__global__ __launch_bounds__(256) void xv_mel_kernel(const float* __restrict__ pcm, const long* __restrict__ off, const int* __restrict__ nsamp,
                                                     const int* __restrict__ start, int nclips, const float* __restrict__ hann,
                                                     const float2* __restrict__ tw512, const float2* __restrict__ tw1024,
                                                     const int* __restrict__ fb_start, const int* __restrict__ fb_len,
                                                     const int* __restrict__ fb_off, const float* __restrict__ fb_w, float* __restrict__ mel) {
    __shared__ float2 buf[2][512];
    __shared__ float mag[XV_NBINS + 3];
    const int tid = threadIdx.x;
    const long m = blockIdx.x;
    const int clip = clip_of(start, nclips, m);
    const long frame = m - start[clip], n = nsamp[clip];
    const float* x = pcm + off[clip];
#pragma unroll
    for (int r = 0; r < 2; ++r) {                      // complex point p = samples 2 p, 2 p + 1 of the windowed frame
        const int p = tid + 256 * r;
        float v[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int i = 2 * p + e;
            const long pos = frame * XV_HOP + i - XV_NFFT / 2;     // index into the clip; the pad mirrors with clamps (:296, :302)
            long idx = pos;
            if (pos < 0) idx = -pos < n - 1 ? -pos : n - 1;
            else if (pos >= n) idx = 2 * n - 2 - pos > 0 ? 2 * n - 2 - pos : 0;
            v[e] = x[idx] * hann[i];
        }
        buf[0][p] = make_float2(v[0], v[1]);
    }
    __syncthreads();
    int src = 0;
#pragma unroll
    for (int Ns = 1; Ns < 512; Ns <<= 1) {             // Stockham radix 2: nine passes, one butterfly per thread
        const int k = tid & (Ns - 1), j0 = ((tid - k) << 1) + k;
        const float2 a = buf[src][tid], bq = buf[src][tid + 256];
        const xv_c b = xv_cmul({bq.x, bq.y}, tw512[k * (256 / Ns)]);
        buf[src ^ 1][j0] = make_float2(a.x + b.re, a.y + b.im);
        buf[src ^ 1][j0 + Ns] = make_float2(a.x - b.re, a.y - b.im);
        __syncthreads();
        src ^= 1;
    }
#pragma unroll
    for (int r = 0; r < 2; ++r) {                      // X[k] = E[k] + w^k O[k], E / O the transforms of the even / odd samples
        const int k = tid + 256 * r;
        const float2 zk = buf[src][k], zn = buf[src][(512 - k) & 511];
        const float er = 0.5f * (zk.x + zn.x), ei = 0.5f * (zk.y - zn.y);
        const float orr = 0.5f * (zk.y + zn.y), oi = -0.5f * (zk.x - zn.x);
        const float2 w = tw1024[k];
        const float xr = er + (orr * w.x - oi * w.y), xi = ei + (orr * w.y + oi * w.x);
        mag[k] = k == 0 ? fabsf(xr) : sqrtf(xr * xr + xi * xi);
        if (k == 0) mag[512] = fabsf(er - orr);
    }
    __syncthreads();
    if (tid < XV_NMELS) {
        const int s0 = fb_start[tid], len = fb_len[tid], wo = fb_off[tid];
        float acc = 0.0f;
        for (int i = 0; i < len; ++i) acc = fmaf(mag[s0 + i], fb_w[wo + i], acc);
        mel[m * XV_NMELS + tid] = logf(fmaxf(acc, 1e-5f));
    }
}

// C = act(sum_k A(m, k) Wt[k][n] + bias) on tile blockIdx.x = (first row of the clip, its rows T, the tile's first row t0 inside it,
// clip).  k = j C_in + c <-> A[first + t + j - taps / 2][c], exact zero outside rows 0 .. T - 1 of the clip.  A rows are lda apart, C
// rows ldc.  A_TANH_CTX: tanh(. + ctx[clip][n]), ctx [clips][N].  S_SUM / S_MAX: part[tile][n] = the tile's column sum / maximum of C,
// rows taken in order.
template <int ACT, int STAT>
__global__ __launch_bounds__(XG_THREADS) void xv_gemm_kernel(const float* __restrict__ A, int lda, int Cin, int taps,
                                                             const int4* __restrict__ tiles, const float* __restrict__ Wt, int K, int N,
                                                             const float* __restrict__ bias, const float* __restrict__ ctx,
                                                             float* __restrict__ C, int ldc, float* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float As[XG_K][XG_T + 4];
    __shared__ __attribute__((aligned(16))) float Bs[XG_K][XG_T];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int4 tile = tiles[blockIdx.x];
    const long first = tile.x;
    const int T = tile.y, t0 = tile.z, clip = tile.w, nrows = min(XG_T, T - t0), n0 = blockIdx.y * XG_T, half = taps / 2;
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[i][q] = 0.0f;
    for (int k0 = 0; k0 < K; k0 += XG_K) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int idx = tid + r * XG_THREADS, row = idx >> 4, kk = idx & 15, k = k0 + kk;
            float v = 0.0f;                            // rows past the tile, inputs past K and taps outside the clip add exact zeros
            if (row < nrows && k < K) {
                const int j = k / Cin, c = k - j * Cin, t = t0 + row + j - half;
                if (t >= 0 && t < T) v = A[(first + t) * lda + c];
            }
            As[kk][row] = v;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int idx = tid + r * XG_THREADS, kk = idx >> 6, col = idx & 63, k = k0 + kk, n = n0 + col;
            Bs[kk][col] = (k < K && n < N) ? Wt[(size_t)k * N + n] : 0.0f;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < XG_K; ++kk) {
            const float4 a = lds_read_f4(&As[kk][ty * 4]);
            const float4 bq = lds_read_f4(&Bs[kk][tx * 4]);
            const float av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {bq.x, bq.y, bq.z, bq.w};
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[i][q] = fmaf(av[i], bv[q], acc[i][q]);
        }
        __syncthreads();
    }
    __shared__ float sT[STAT == S_NONE ? 1 : XG_T][XG_T + 1];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = ty * 4 + i;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int n = n0 + tx * 4 + q;
            float v = acc[i][q];
            if (n < N) {
                if (bias) v = v + bias[n];
                if (ACT == A_RELU) v = fmaxf(v, 0.0f);
                if (ACT == A_TANH_CTX) v = tanhf(v + ctx[(size_t)clip * N + n]);
                if (row < nrows) C[(first + t0 + row) * ldc + n] = v;
            }
            if constexpr (STAT != S_NONE) sT[row][tx * 4 + q] = v;
        }
    }
    if constexpr (STAT != S_NONE) {
        __syncthreads();
        if (tid < XG_T && n0 + tid < N) {
            float s = STAT == S_SUM ? 0.0f : -INFINITY;
            for (int r = 0; r < nrows; ++r) s = STAT == S_SUM ? s + sT[r][tid] : fmaxf(s, sT[r][tid]);
            part[(size_t)blockIdx.x * N + n0 + tid] = s;
        }
    }
}

// Res2NetBlock (:50-67) of one block: x, y [M][512]; chunk 0 passes through, chunk 1 goes through conv 0, chunk i >= 2 plus the previous
// output through conv i - 1; every conv k = 3, dilation dil, zeros outside the clip, ReLU.  w [7][192][64] (k = tap-major), b [7][64].
// tiles[blockIdx.x] = (first row of the clip, its rows T, the tile's first row t0).  Window row r <-> clip row t0 - 7 dil + r.  Stage s
// forms its input in place over the previous output (rows outside the clip: zero, the conv's own padding), then computes rows
// (s + 1) dil .. window - (s + 1) dil: exactly those whose three taps hold right values, and after the last stage exactly the tile.
// A row's value is the same fmaf chain over k whichever workgroup computes it, so the tiling leaves no trace in the result.
__global__ __launch_bounds__(XG_THREADS) void xv_res2net_kernel(const float* __restrict__ x, const int4* __restrict__ tiles,
                                                                const float* __restrict__ w, const float* __restrict__ b, int dil,
                                                                float* __restrict__ y) {
    __shared__ float sU[2][XV_W][RS_RP];               // [buffer][channel][window row]
    __shared__ __attribute__((aligned(16))) float sW[3 * XV_W][XV_W];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int4 tile = tiles[blockIdx.x];
    const long first = tile.x;
    const int T = tile.y, t0 = tile.z, H = 7 * dil, win = XV_RES_TILE + 2 * H, nown = min(XV_RES_TILE, T - t0);
    for (int idx = tid; idx < nown * XV_W; idx += XG_THREADS) {
        const long e = (first + t0 + (idx >> 6)) * XV_C + (idx & 63);
        y[e] = x[e];
    }
    int cur = 0;
    for (int s = 0; s < 7; ++s) {
        const int u_lo = s * dil, u_n = win - 2 * u_lo;
        for (int idx = tid; idx < u_n * XV_W; idx += XG_THREADS) {
            const int r = u_lo + (idx >> 6), c = idx & 63, t = t0 - H + r;
            float v = 0.0f;
            if (t >= 0 && t < T) {
                v = x[(first + t) * XV_C + XV_W * (s + 1) + c];
                if (s > 0) v = v + sU[cur][c][r];
            }
            sU[cur][c][r] = v;
        }
        for (int idx = tid; idx < 3 * XV_W * XV_W / 4; idx += XG_THREADS)
            reinterpret_cast<f32x4*>(&sW[0][0])[idx] = reinterpret_cast<const f32x4*>(w + (size_t)s * 3 * XV_W * XV_W)[idx];
        __syncthreads();
        const int r_lo = (s + 1) * dil, r_n = win - 2 * r_lo, nxt = cur ^ 1;
        for (int rb = 0; rb * 64 < r_n; ++rb) {
            const int r0 = r_lo + rb * 64 + ty * 4;
            int rr[4];                                 // rows past the range recompute its last row and store nothing
#pragma unroll
            for (int i = 0; i < 4; ++i) rr[i] = min(r0 + i, r_lo + r_n - 1);
            float acc[4][4];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[i][q] = 0.0f;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const int sh = (j - 1) * dil;
#pragma unroll 8
                for (int c = 0; c < XV_W; ++c) {
                    const float4 bq = lds_read_f4(&sW[j * XV_W + c][tx * 4]);
                    const float bv[4] = {bq.x, bq.y, bq.z, bq.w};
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float a = sU[cur][c][rr[i] + sh];
#pragma unroll
                        for (int q = 0; q < 4; ++q) acc[i][q] = fmaf(a, bv[q], acc[i][q]);
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int r = r0 + i;
                if (r >= r_lo + r_n) continue;
                float v[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    v[q] = fmaxf(acc[i][q] + b[s * XV_W + tx * 4 + q], 0.0f);
                    sU[nxt][tx * 4 + q][r] = v[q];
                }
                if (r >= H && r < H + nown) {
                    float* dst = y + (first + t0 + (r - H)) * XV_C + XV_W * (s + 1) + tx * 4;
#pragma unroll
                    for (int q = 0; q < 4; ++q) dst[q] = v[q];
                }
            }
        }
        __syncthreads();
        cur = nxt;
    }
}

// SEBlock (:24-29) and the block's residual (:98) on one tile: the clip's column means from psum [tiles][512] (tile order), 512 -> 128
// ReLU -> 512 sigmoid, out = h gate + res.  w1 [512][128], w2 [128][512] (k-major).  h [M][512]; res rows ldr apart, out rows ldo.
__global__ __launch_bounds__(XG_THREADS) void xv_se_apply_kernel(const float* __restrict__ h, const int4* __restrict__ tiles,
                                                                 const int* __restrict__ tstart, const float* __restrict__ psum,
                                                                 const float* __restrict__ w1, const float* __restrict__ b1,
                                                                 const float* __restrict__ w2, const float* __restrict__ b2,
                                                                 const float* __restrict__ res, int ldr, float* __restrict__ out, int ldo) {
    __shared__ float s_mean[XV_C], s_hid[XV_SE], s_gate[XV_C];
    const int tid = threadIdx.x;
    const int4 tile = tiles[blockIdx.x];
    const long first = tile.x;
    const int T = tile.y, t0 = tile.z, clip = tile.w, nrows = min(XG_T, T - t0), tb = tstart[clip], te = tstart[clip + 1];
    for (int c = tid; c < XV_C; c += XG_THREADS) s_mean[c] = xv_tiles_sum(psum, XV_C, tb, te, c) / (float)T;
    __syncthreads();
    if (tid < XV_SE) {
        float acc = 0.0f;
        for (int k = 0; k < XV_C; ++k) acc = fmaf(s_mean[k], w1[k * XV_SE + tid], acc);
        s_hid[tid] = fmaxf(acc + b1[tid], 0.0f);
    }
    __syncthreads();
    for (int c = tid; c < XV_C; c += XG_THREADS) {
        float acc = 0.0f;
        for (int k = 0; k < XV_SE; ++k) acc = fmaf(s_hid[k], w2[k * XV_C + c], acc);
        s_gate[c] = 1.0f / (1.0f + expf(-(acc + b2[c])));
    }
    __syncthreads();
    for (int idx = tid; idx < nrows * XV_C; idx += XG_THREADS) {
        const long m = first + t0 + (idx >> 9);
        const int c = idx & (XV_C - 1);
        out[m * ldo + c] = h[m * XV_C + c] * s_gate[c] + res[m * ldr + c];
    }
}

// pvar[tile][c] = sum over the tile's rows of (x - mean)^2, mean from psum [tiles][1536] (:127-128); x [M][1536]
__global__ __launch_bounds__(XG_THREADS) void xv_asp_var_kernel(const float* __restrict__ x, const int4* __restrict__ tiles,
                                                                const int* __restrict__ tstart, const float* __restrict__ psum,
                                                                float* __restrict__ pvar) {
    const int4 tile = tiles[blockIdx.x];
    const long first = tile.x;
    const int T = tile.y, t0 = tile.z, clip = tile.w, nrows = min(XG_T, T - t0), tb = tstart[clip], te = tstart[clip + 1];
    for (int c = threadIdx.x; c < XV_CAT; c += XG_THREADS) {
        const float mean = xv_tiles_sum(psum, XV_CAT, tb, te, c) / (float)T;
        float s = 0.0f;
        for (int r = 0; r < nrows; ++r) { const float d = x[(first + t0 + r) * XV_CAT + c] - mean; s = s + d * d; }
        pvar[(size_t)blockIdx.x * XV_CAT + c] = s;
    }
}

// ctx[clip][n] = bias[n] + sum_k [mean | std][k] wc[k][n]: the part of asp.tdnn's input that is constant over the clip (:132-136).
// wc [3072][128]; one workgroup per clip, two k halves per output added in order.
__global__ __launch_bounds__(XG_THREADS) void xv_asp_ctx_kernel(const int* __restrict__ start, const int* __restrict__ tstart,
                                                                const float* __restrict__ psum, const float* __restrict__ pvar,
                                                                const float* __restrict__ wc, const float* __restrict__ bias,
                                                                float* __restrict__ ctx) {
    __shared__ float s_ms[2 * XV_CAT], s_acc[2][XV_ATT];
    const int tid = threadIdx.x, clip = blockIdx.x, tb = tstart[clip], te = tstart[clip + 1];
    const float T = (float)(start[clip + 1] - start[clip]);
    for (int c = tid; c < XV_CAT; c += XG_THREADS) {
        s_ms[c] = xv_tiles_sum(psum, XV_CAT, tb, te, c) / T;
        s_ms[XV_CAT + c] = sqrtf(fmaxf(xv_tiles_sum(pvar, XV_CAT, tb, te, c) / T, 1e-12f));
    }
    __syncthreads();
    const int n = tid & (XV_ATT - 1), hf = tid >> 7;
    float acc = 0.0f;
    for (int k = hf * XV_CAT; k < (hf + 1) * XV_CAT; ++k) acc = fmaf(s_ms[k], wc[(size_t)k * XV_ATT + n], acc);
    s_acc[hf][n] = acc;
    __syncthreads();
    if (tid < XV_ATT) ctx[(size_t)clip * XV_ATT + tid] = (s_acc[0][tid] + s_acc[1][tid]) + bias[tid];
}

// softmax over the clip's rows, per channel (:139): with the clip's maximum from pmax, pexp[tile][c] = sum exp(e - max) and
// pwx[tile][c] = sum exp(e - max) x over the tile's rows.  e, x [M][1536].
__global__ __launch_bounds__(XG_THREADS) void xv_asp_sum_kernel(const float* __restrict__ e, const float* __restrict__ x,
                                                                const int4* __restrict__ tiles, const int* __restrict__ tstart,
                                                                const float* __restrict__ pmax, float* __restrict__ pexp,
                                                                float* __restrict__ pwx) {
    const int4 tile = tiles[blockIdx.x];
    const long first = tile.x;
    const int T = tile.y, t0 = tile.z, clip = tile.w, nrows = min(XG_T, T - t0), tb = tstart[clip], te = tstart[clip + 1];
    for (int c = threadIdx.x; c < XV_CAT; c += XG_THREADS) {
        const float mx = xv_tiles_max(pmax, XV_CAT, tb, te, c);
        float s = 0.0f, sx = 0.0f;
        for (int r = 0; r < nrows; ++r) {
            const long at = (first + t0 + r) * XV_CAT + c;
            const float p = expf(e[at] - mx);
            s = s + p;
            sx = sx + p * x[at];
        }
        pexp[(size_t)blockIdx.x * XV_CAT + c] = s;
        pwx[(size_t)blockIdx.x * XV_CAT + c] = sx;
    }
}

// pwv[tile][c] = sum over the tile's rows of alpha (x - wm) (x - wm), alpha = exp(e - max) / S, wm = (sum pwx) / S (:142-143)
__global__ __launch_bounds__(XG_THREADS) void xv_asp_wvar_kernel(const float* __restrict__ e, const float* __restrict__ x,
                                                                 const int4* __restrict__ tiles, const int* __restrict__ tstart,
                                                                 const float* __restrict__ pmax, const float* __restrict__ pexp,
                                                                 const float* __restrict__ pwx, float* __restrict__ pwv) {
    const int4 tile = tiles[blockIdx.x];
    const long first = tile.x;
    const int T = tile.y, t0 = tile.z, clip = tile.w, nrows = min(XG_T, T - t0), tb = tstart[clip], te = tstart[clip + 1];
    for (int c = threadIdx.x; c < XV_CAT; c += XG_THREADS) {
        const float mx = xv_tiles_max(pmax, XV_CAT, tb, te, c), S = xv_tiles_sum(pexp, XV_CAT, tb, te, c);
        const float wm = xv_tiles_sum(pwx, XV_CAT, tb, te, c) / S;
        float s = 0.0f;
        for (int r = 0; r < nrows; ++r) {
            const long at = (first + t0 + r) * XV_CAT + c;
            const float a = expf(e[at] - mx) / S, d = x[at] - wm;
            s = s + (a * d) * d;
        }
        pwv[(size_t)blockIdx.x * XV_CAT + c] = s;
    }
}

// out[clip][n] = bias[n] + sum_k [wm | wstd][k] wt[k][n] (:144-147, :233-235).  grid (clips, ceil(E / 64)); an output is four k
// quarters added as ((q0 + q1) + (q2 + q3)).
__global__ __launch_bounds__(XG_THREADS) void xv_fc_kernel(const int* __restrict__ tstart, const float* __restrict__ pexp,
                                                           const float* __restrict__ pwx, const float* __restrict__ pwv,
                                                           const float* __restrict__ wt, const float* __restrict__ bias, int E,
                                                           float* __restrict__ out) {
    __shared__ float s_pool[2 * XV_CAT], s_acc[4][64];
    const int tid = threadIdx.x, clip = blockIdx.x, tb = tstart[clip], te = tstart[clip + 1];
    for (int c = tid; c < XV_CAT; c += XG_THREADS) {
        const float S = xv_tiles_sum(pexp, XV_CAT, tb, te, c);
        s_pool[c] = xv_tiles_sum(pwx, XV_CAT, tb, te, c) / S;
        s_pool[XV_CAT + c] = sqrtf(fmaxf(xv_tiles_sum(pwv, XV_CAT, tb, te, c), 1e-12f));
    }
    __syncthreads();
    const int col = tid & 63, qt = tid >> 6, n = blockIdx.y * 64 + col, kq = 2 * XV_CAT / 4;
    float acc = 0.0f;
    if (n < E)
        for (int k = qt * kq; k < (qt + 1) * kq; ++k) acc = fmaf(s_pool[k], wt[(size_t)k * E + n], acc);
    s_acc[qt][col] = acc;
    __syncthreads();
    if (tid < 64 && n < E) out[(size_t)clip * E + n] = ((s_acc[0][tid] + s_acc[1][tid]) + (s_acc[2][tid] + s_acc[3][tid])) + bias[n];
}

// ---- weights ------------------------------------------------------------------------------------------------------------------------
XvecQwen3TTS::XvecQwen3TTS(int device, const CheckedWeights& cw, int E, long max_samples, hipStream_t work)
    : device_(device), E_(E), max_samples_(max_samples) {
    if (max_samples < 1 || max_samples > XV_MAX_SAMPLES) throw std::invalid_argument("speaker encoder: max_samples in 1..2^28");
    if (E < 1 || E > 65536) throw std::invalid_argument("speaker encoder: fc.weight has " + std::to_string(E) + " rows, 1..65536 supported");
    param_bytes_ = cw.disk_bytes;
    Builder b(cw, "speaker_encoder.");
    // Wt[j C_in + c][n] = W[n][j][c] of a conv stored [out][k][in] (:436-437)
    auto conv = [&](const std::string& key, int Cout, int k, int Cin, int c0, int c1) {
        Gemm gm; gm.K = k * (c1 - c0); gm.N = Cout; gm.Cin = c1 - c0; gm.taps = k;
        const auto& W = b.t(key + ".weight");
        gm.wt = b.take((size_t)gm.K * gm.N);
        for (int n = 0; n < Cout; ++n)
            for (int j = 0; j < k; ++j)
                for (int c = c0; c < c1; ++c) b.h[gm.wt + ((size_t)j * gm.Cin + (c - c0)) * Cout + n] = W[((size_t)n * k + j) * Cin + c];
        gm.bias = b.vec(key + ".bias");
        return gm;
    };
    init_ = conv("blocks.0.conv", XV_C, 5, XV_NMELS, 0, XV_NMELS);
    for (int i = 0; i < 3; ++i) {
        const std::string p = "blocks." + std::to_string(i + 1) + ".";
        Block& bl = blocks_[i];
        bl.tdnn1 = conv(p + "tdnn1.conv", XV_C, 1, XV_C, 0, XV_C);
        bl.tdnn2 = conv(p + "tdnn2.conv", XV_C, 1, XV_C, 0, XV_C);
        bl.se1 = conv(p + "se_block.conv1", XV_SE, 1, XV_C, 0, XV_C);
        bl.se2 = conv(p + "se_block.conv2", XV_C, 1, XV_SE, 0, XV_SE);
        bl.res_w = b.take((size_t)7 * 3 * XV_W * XV_W);
        bl.res_b = b.take((size_t)7 * XV_W);
        for (int s = 0; s < 7; ++s) {
            const std::string key = p + "res2net_block.blocks." + std::to_string(s) + ".conv";
            const auto &W = b.t(key + ".weight"), &B = b.t(key + ".bias");
            for (int n = 0; n < XV_W; ++n) {
                for (int j = 0; j < 3; ++j)
                    for (int c = 0; c < XV_W; ++c)
                        b.h[bl.res_w + ((size_t)s * 3 * XV_W + j * XV_W + c) * XV_W + n] = W[((size_t)n * 3 + j) * XV_W + c];
                b.h[bl.res_b + (size_t)s * XV_W + n] = B[n];
            }
        }
    }
    mfa_ = conv("mfa.conv", XV_CAT, 1, XV_CAT, 0, XV_CAT);
    att1_ = conv("asp.tdnn.conv", XV_ATT, 1, 3 * XV_CAT, 0, XV_CAT);                // the x third; [mean | std] go through ctx_w_
    {
        const auto& W = b.t("asp.tdnn.conv.weight");
        ctx_w_ = b.take((size_t)2 * XV_CAT * XV_ATT);
        for (int n = 0; n < XV_ATT; ++n)
            for (int k = 0; k < 2 * XV_CAT; ++k) b.h[ctx_w_ + (size_t)k * XV_ATT + n] = W[(size_t)n * 3 * XV_CAT + XV_CAT + k];
    }
    att2_ = conv("asp.conv", XV_CAT, 1, XV_ATT, 0, XV_ATT);
    fc_ = conv("fc", E, 1, 2 * XV_CAT, 0, 2 * XV_CAT);
    // the front end's tables: window (:282-286, Float), twiddles, the filterbank's non-zero runs
    hann_ = b.take(XV_NFFT);
    for (int i = 0; i < XV_NFFT; ++i) b.h[hann_ + i] = 0.5f * (1.0f - cosf(2.0f * (float)M_PI * (float)i / (float)XV_NFFT));
    tw512_ = b.take(512);
    for (int k = 0; k < 256; ++k) {
        const double a = -2.0 * M_PI * k / 512.0;
        b.h[tw512_ + 2 * k] = (float)cos(a); b.h[tw512_ + 2 * k + 1] = (float)sin(a);
    }
    tw1024_ = b.take(1024);
    for (int k = 0; k < 512; ++k) {
        const double a = -2.0 * M_PI * k / 1024.0;
        b.h[tw1024_ + 2 * k] = (float)cos(a); b.h[tw1024_ + 2 * k + 1] = (float)sin(a);
    }
    std::vector<int> h_fb;
    {
        const std::vector<float> fb = xvec_filterbank();
        std::vector<int> st(XV_NMELS, 0), len(XV_NMELS, 0), offs(XV_NMELS, 0);
        std::vector<float> packed;
        for (int m = 0; m < XV_NMELS; ++m) {
            int lo = -1, hi = -1;
            for (int k = 0; k < XV_NBINS; ++k)
                if (fb[(size_t)k * XV_NMELS + m] != 0.0f) { if (lo < 0) lo = k; hi = k; }
            offs[m] = (int)packed.size();
            if (lo >= 0) {
                st[m] = lo; len[m] = hi - lo + 1;
                for (int k = lo; k <= hi; ++k) packed.push_back(fb[(size_t)k * XV_NMELS + m]);
            }
        }
        h_fb.insert(h_fb.end(), st.begin(), st.end());     // d_fb_: start [128] | len [128] | off [128]
        h_fb.insert(h_fb.end(), len.begin(), len.end());
        h_fb.insert(h_fb.end(), offs.begin(), offs.end());
        fb_w_ = b.take(packed.size());
        std::copy(packed.begin(), packed.end(), b.h.begin() + fb_w_);
    }
    // rows and tiles a pass can hold: a clip of n samples has n / 256 + 1 rows and at most rows / 64 + 1 tiles
    const long clips_cap = std::min<long>(XV_MAX_CLIPS, max_samples);
    rows_cap_ = max_samples / XV_HOP + clips_cap;
    tiles_cap_ = rows_cap_ / XV_TILE + clips_cap;
    QASR_HIP(hipSetDevice(device_));
    QASR_HIP(hipStreamCreateWithFlags(&own_, hipStreamNonBlocking));
    work_ = work ? work : own_;
    for (auto& e : ev_) QASR_HIP(hipEventCreate(&e));
    d_w_.alloc(b.h.size() * sizeof(float));
    QASR_HIP(hipMemcpy(d_w_.p, b.h.data(), b.h.size() * sizeof(float), hipMemcpyHostToDevice));
    d_fb_.alloc(h_fb.size() * sizeof(int));
    QASR_HIP(hipMemcpy(d_fb_.p, h_fb.data(), h_fb.size() * sizeof(int), hipMemcpyHostToDevice));
    const size_t F = sizeof(float), R = (size_t)rows_cap_;
    d_start_.alloc((XV_MAX_CLIPS + 1) * sizeof(int)); d_tstart_.alloc((XV_MAX_CLIPS + 1) * sizeof(int));
    d_n_.alloc(XV_MAX_CLIPS * sizeof(int)); d_off_.alloc(XV_MAX_CLIPS * sizeof(long));
    d_tiles_.alloc((size_t)tiles_cap_ * 4 * sizeof(int)); d_res_tiles_.alloc((size_t)tiles_cap_ * 4 * sizeof(int));
    d_pcm_.alloc((size_t)max_samples * F);
    d_mel_.alloc(R * XV_NMELS * F);
    // 4864 floats per row.  tdnn2's output goes where tdnn1's was (dead once the Res2Net launch has read it), the attention's logits
    // where the three blocks' outputs were (dead once the MFA has read them).
    d_h0_.alloc(R * XV_C * F); d_t1_.alloc(R * XV_C * F); d_r_.alloc(R * XV_C * F);
    d_cat_.alloc(R * XV_CAT * F); d_mfa_.alloc(R * XV_CAT * F); d_att_.alloc(R * XV_ATT * F);
    for (auto& p : d_part_) p.alloc((size_t)tiles_cap_ * XV_CAT * F);
    d_ctx_.alloc((size_t)XV_MAX_CLIPS * XV_ATT * F);
    d_out_.alloc((size_t)XV_MAX_CLIPS * E * F);
}

XvecQwen3TTS::~XvecQwen3TTS() {
    if (work_) (void)hipStreamSynchronize(work_);
    for (auto& e : ev_) if (e) (void)hipEventDestroy(e);
    if (own_) (void)hipStreamDestroy(own_);
}

void XvecQwen3TTS::unload() {
    if (!loaded_) return;
    QASR_HIP(hipSetDevice(device_));
    QASR_HIP(hipStreamSynchronize(work_));
    for (DevBuf* b : {&d_w_, &d_fb_, &d_start_, &d_tiles_, &d_tstart_, &d_res_tiles_, &d_n_, &d_off_, &d_pcm_, &d_mel_, &d_h0_, &d_t1_, &d_r_,
                      &d_cat_, &d_mfa_, &d_att_, &d_part_[0], &d_part_[1], &d_part_[2], &d_part_[3], &d_part_[4], &d_part_[5], &d_ctx_,
                      &d_out_})
        b->release();
    loaded_ = false;
}

void XvecQwen3TTS::check_loaded() const {
    if (!loaded_) throw NotLoaded("speaker encoder: model unloaded");
}

// ---- a pass -------------------------------------------------------------------------------------------------------------------------
// uploads the pass's tables: start[clip], the two tile grids (each starts again at every clip's first row), tstart[clip]
void XvecQwen3TTS::plan(const long* frames, int n) {
    QASR_HIP(hipStreamSynchronize(work_));             // the tables are rewritten
    n_clips_ = n;
    h_start_.assign(XV_MAX_CLIPS + 1, 0);
    h_tstart_.assign(XV_MAX_CLIPS + 1, 0);
    h_tiles_.clear();
    h_res_tiles_.clear();
    long at = 0;
    for (int i = 0; i < n; ++i) {
        h_start_[i] = (int)at;
        h_tstart_[i] = (int)(h_tiles_.size() / 4);
        for (long t0 = 0; t0 < frames[i]; t0 += XV_TILE)
            for (int v : {(int)at, (int)frames[i], (int)t0, i}) h_tiles_.push_back(v);
        for (long t0 = 0; t0 < frames[i]; t0 += XV_RES_TILE)
            for (int v : {(int)at, (int)frames[i], (int)t0, i}) h_res_tiles_.push_back(v);
        at += frames[i];
    }
    h_start_[n] = (int)at;
    h_tstart_[n] = (int)(h_tiles_.size() / 4);
    M_ = at;
    n_tiles_ = (int)(h_tiles_.size() / 4);
    n_res_tiles_ = (int)(h_res_tiles_.size() / 4);
    if (M_ > rows_cap_ || n_tiles_ > tiles_cap_ || n_res_tiles_ > tiles_cap_) throw std::length_error("speaker encoder: a pass exceeds its buffers");
    QASR_HIP(hipMemcpy(d_start_.p, h_start_.data(), h_start_.size() * sizeof(int), hipMemcpyHostToDevice));
    QASR_HIP(hipMemcpy(d_tstart_.p, h_tstart_.data(), h_tstart_.size() * sizeof(int), hipMemcpyHostToDevice));
    QASR_HIP(hipMemcpy(d_tiles_.p, h_tiles_.data(), h_tiles_.size() * sizeof(int), hipMemcpyHostToDevice));
    QASR_HIP(hipMemcpy(d_res_tiles_.p, h_res_tiles_.data(), h_res_tiles_.size() * sizeof(int), hipMemcpyHostToDevice));
}

template <int ACT, int STAT>
void XvecQwen3TTS::gemm(const Gemm& gm, const float* A, int lda, float* C, int ldc, const float* ctx, float* part) {
    const dim3 grid((unsigned)n_tiles_, (unsigned)cdiv(gm.N, XG_T));
    hipLaunchKernelGGL((xv_gemm_kernel<ACT, STAT>), grid, dim3(XG_THREADS), 0, work_, A, lda, gm.Cin, gm.taps, d_tiles_.as<int4>(), W(gm.wt),
                       gm.K, gm.N, ACT == A_TANH_CTX ? (const float*)nullptr : W(gm.bias), ctx, C, ldc, part);
}

// d_pcm_ -> d_mel_; records ev_[1]
void XvecQwen3TTS::dev_mel() {
    hipLaunchKernelGGL(xv_mel_kernel, dim3((unsigned)M_), dim3(256), 0, work_, d_pcm_.as<float>(), d_off_.as<long>(), d_n_.as<int>(),
                       d_start_.as<int>(), n_clips_, W(hann_), reinterpret_cast<const float2*>(W(tw512_)),
                       reinterpret_cast<const float2*>(W(tw1024_)), d_fb_.as<int>(), d_fb_.as<int>() + XV_NMELS,
                       d_fb_.as<int>() + 2 * XV_NMELS, W(fb_w_), d_mel_.as<float>());
    QASR_HIP(hipEventRecord(ev_[1], work_));
    QASR_HIP(hipGetLastError());
}

// d_mel_ -> d_out_ [clips][E]; records ev_[2] .. ev_[6]
void XvecQwen3TTS::dev_network() {
    float *h0 = d_h0_.as<float>(), *t1 = d_t1_.as<float>(), *r = d_r_.as<float>(), *t2 = t1, *cat = d_cat_.as<float>();
    float *mfa = d_mfa_.as<float>(), *att = d_att_.as<float>(), *e = cat, *ctx = d_ctx_.as<float>();
    float *psum = d_part_[0].as<float>(), *pvar = d_part_[1].as<float>(), *pmax = d_part_[2].as<float>(), *pexp = d_part_[3].as<float>();
    float *pwx = d_part_[4].as<float>(), *pwv = d_part_[5].as<float>();
    const int4* tiles = d_tiles_.as<int4>();
    const int* tstart = d_tstart_.as<int>();
    const dim3 th(XG_THREADS);
    gemm<A_RELU, S_NONE>(init_, d_mel_.as<float>(), XV_NMELS, h0, XV_C, nullptr, nullptr);
    QASR_HIP(hipEventRecord(ev_[2], work_));
    const int dil[3] = {2, 3, 4};
    for (int i = 0; i < 3; ++i) {                      // ECAPABlock (:91-99); block i's output is columns 512 i .. of cat
        const Block& bl = blocks_[i];
        const float* in = i == 0 ? h0 : cat + (size_t)(i - 1) * XV_C;
        const int ldin = i == 0 ? XV_C : XV_CAT;
        gemm<A_RELU, S_NONE>(bl.tdnn1, in, ldin, t1, XV_C, nullptr, nullptr);
        hipLaunchKernelGGL(xv_res2net_kernel, dim3((unsigned)n_res_tiles_), th, 0, work_, t1, d_res_tiles_.as<int4>(), W(bl.res_w), W(bl.res_b),
                           dil[i], r);
        gemm<A_RELU, S_SUM>(bl.tdnn2, r, XV_C, t2, XV_C, nullptr, psum);
        hipLaunchKernelGGL(xv_se_apply_kernel, dim3((unsigned)n_tiles_), th, 0, work_, t2, tiles, tstart, psum, W(bl.se1.wt), W(bl.se1.bias),
                           W(bl.se2.wt), W(bl.se2.bias), in, ldin, cat + (size_t)i * XV_C, XV_CAT);
        QASR_HIP(hipEventRecord(ev_[3 + i], work_));
    }
    gemm<A_RELU, S_SUM>(mfa_, cat, XV_CAT, mfa, XV_CAT, nullptr, psum);
    hipLaunchKernelGGL(xv_asp_var_kernel, dim3((unsigned)n_tiles_), th, 0, work_, mfa, tiles, tstart, psum, pvar);
    hipLaunchKernelGGL(xv_asp_ctx_kernel, dim3((unsigned)n_clips_), th, 0, work_, d_start_.as<int>(), tstart, psum, pvar, W(ctx_w_),
                       W(att1_.bias), ctx);
    gemm<A_TANH_CTX, S_NONE>(att1_, mfa, XV_CAT, att, XV_ATT, ctx, nullptr);
    gemm<A_LIN, S_MAX>(att2_, att, XV_ATT, e, XV_CAT, nullptr, pmax);
    hipLaunchKernelGGL(xv_asp_sum_kernel, dim3((unsigned)n_tiles_), th, 0, work_, e, mfa, tiles, tstart, pmax, pexp, pwx);
    hipLaunchKernelGGL(xv_asp_wvar_kernel, dim3((unsigned)n_tiles_), th, 0, work_, e, mfa, tiles, tstart, pmax, pexp, pwx, pwv);
    hipLaunchKernelGGL(xv_fc_kernel, dim3((unsigned)n_clips_, (unsigned)cdiv(E_, 64)), th, 0, work_, tstart, pexp, pwx, pwv, W(fc_.wt),
                       W(fc_.bias), E_, d_out_.as<float>());
    QASR_HIP(hipEventRecord(ev_[6], work_));
    QASR_HIP(hipGetLastError());
}

// waits for the pass and adds its stage times; stages past `last` did not run
void XvecQwen3TTS::finish(int last) {
    QASR_HIP(hipStreamSynchronize(work_));
    QASR_HIP(hipGetLastError());
    for (int s = 0; s < last; ++s) {
        float ms = 0;
        QASR_HIP(hipEventElapsedTime(&ms, ev_[s], ev_[s + 1]));
        timing_[s] += ms;
    }
}

void XvecQwen3TTS::pass(const XvecClip* c, int n, Mode mode) {
    QASR_HIP(hipSetDevice(device_));
    std::vector<long> frames(n);
    h_n_.resize(n); h_off_.resize(n);
    long total = 0;
    for (int i = 0; i < n; ++i) { frames[i] = xvec_num_frames(c[i].n); h_n_[i] = (int)c[i].n; h_off_[i] = total; total += c[i].n; }
    plan(frames.data(), n);
    h_pcm_.resize((size_t)total);
    for (int i = 0; i < n; ++i) std::memcpy(h_pcm_.data() + h_off_[i], c[i].pcm, (size_t)c[i].n * sizeof(float));
    QASR_HIP(hipMemcpy(d_n_.p, h_n_.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice));
    QASR_HIP(hipMemcpy(d_off_.p, h_off_.data(), (size_t)n * sizeof(long), hipMemcpyHostToDevice));
    QASR_HIP(hipMemcpy(d_pcm_.p, h_pcm_.data(), h_pcm_.size() * sizeof(float), hipMemcpyHostToDevice));
    QASR_HIP(hipEventRecord(ev_[0], work_));
    dev_mel();
    if (mode == MEL) {
        for (int i = 0; i < n; ++i)
            QASR_HIP(hipMemcpyAsync(c[i].mel, d_mel_.as<float>() + (size_t)h_start_[i] * XV_NMELS, (size_t)frames[i] * XV_NMELS * sizeof(float),
                                    hipMemcpyDeviceToHost, work_));
        finish(1);
        return;
    }
    dev_network();
    for (int i = 0; i < n; ++i)
        QASR_HIP(hipMemcpyAsync(c[i].out, d_out_.as<float>() + (size_t)i * E_, (size_t)E_ * sizeof(float), hipMemcpyDeviceToHost, work_));
    finish(XV_STAGES);
}

// ---- entry points -------------------------------------------------------------------------------------------------------------------
void XvecQwen3TTS::run(const std::vector<XvecClip>& clips, Mode mode) {
    check_loaded();
    for (float& t : timing_) t = 0.0f;
    for (size_t i = 0; i < clips.size(); ++i)
        if (clips[i].n < 1 || clips[i].n > max_samples_)
            throw std::length_error("speaker encoder: item " + std::to_string(i) + " holds " + std::to_string(clips[i].n) +
                                    " samples, a clip holds 1.." + std::to_string(max_samples_) + " (max_samples)");
    for (size_t i = 0; i < clips.size();) {            // passes end at clip boundaries
        size_t j = i;
        long total = 0;
        while (j < clips.size() && j - i < (size_t)XV_MAX_CLIPS && total + clips[j].n <= max_samples_) total += clips[j++].n;
        pass(clips.data() + i, (int)(j - i), mode);
        i = j;
    }
}

void XvecQwen3TTS::embed_mel(const float* mel, long T, float* out) {
    check_loaded();
    for (float& t : timing_) t = 0.0f;
    if (T < 1 || T > max_samples_ / XV_HOP + 1)
        throw std::length_error("speaker encoder: " + std::to_string(T) + " frames, a clip holds 1.." + std::to_string(max_samples_ / XV_HOP + 1) +
                                " (max_samples / 256 + 1)");
    QASR_HIP(hipSetDevice(device_));
    plan(&T, 1);
    QASR_HIP(hipMemcpy(d_mel_.p, mel, (size_t)T * XV_NMELS * sizeof(float), hipMemcpyHostToDevice));
    QASR_HIP(hipEventRecord(ev_[0], work_));
    QASR_HIP(hipEventRecord(ev_[1], work_));
    dev_network();
    QASR_HIP(hipMemcpyAsync(out, d_out_.p, (size_t)E_ * sizeof(float), hipMemcpyDeviceToHost, work_));
    finish(XV_STAGES);
}

}  // namespace qasr
