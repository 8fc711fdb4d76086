// voc_cosyvoice.hip -- the CosyVoice3 HiFT vocoder for gfx950 (voc_cosyvoice.h).  f32 throughout (the source's running phase: f64, in
// cycles), accurate expf / sinf / cosf / tanhf / logf, no atomics, no vendor BLAS or FFT.
//
// A pass holds clips back to back, channel-last, at five rates: a clip of T frames owns T rows of the mel and of the F0 stack, 8 T and
// 40 T rows of the first two stages, 120 T + 1 rows of the last stage and of the source's STFT, 480 T source samples and 480 T + 16 PCM
// samples.  start[level][clip] is the clip's first row at a level.  The launches of a pass:
//   hf_conv_kernel   the house 64 x 64 f32 tile (16-deep k steps, one fmaf chain per output over k = tap-major, channel-minor) with one
//                    row locator for every conv of the network: output row t of a clip reads, under tap j, position t stride + j dil -
//                    lpad of the clip's input *after* nearest upsampling by `up` (row position / up); positions outside the clip add
//                    exact zeros.  lpad = (k - 1) dil: causal; lpad = 0: look-ahead; up > 1: the upsample stages; stride > 1: source_downs.
//                    `reflect`: the output has one more row in front, a copy of row 1 (row t is the conv's row t - 1, row 0 its row 1).
//                    At the load: nothing, LeakyReLU or Snake.  Epilogues: bias, then nothing | ELU | abs | + R | the resblock mean.
//   hf_phase_kernel  per clip and harmonic, the phase at the start of every frame: a scan over T values
//   hf_source_kernel sines, noise, merge, tanh, noise: one thread per sample
//   hf_stft_kernel   one thread per (frame, bin) of the source's STFT
//   hf_tail_kernel   LeakyReLU 0.01, conv_post, exp | sin, the 16-point inverse DFT, the window, and per output sample the gather of its
//                    at most four frames and the division by the window sum
// Every output is one thread's chain in a fixed order, so a clip's rows are the same bits alone, in any batch and in any pass.
#include "voc_cosyvoice.h"
#include "codec_shared.h"
#include <algorithm>
#include <cmath>
#include <cstring>

namespace qasr {

// ---- keys (host) --------------------------------------------------------------------------------------------------------------------
std::vector<std::pair<std::string, std::vector<int64_t>>> hift_tensor_shapes() {
    std::vector<std::pair<std::string, std::vector<int64_t>>> s;
    auto conv = [&](const std::string& k, int64_t out, int64_t taps, int64_t in) {
        s.emplace_back(k + ".weight", std::vector<int64_t>{out, taps, in});
        s.emplace_back(k + ".bias", std::vector<int64_t>{out});
    };
    auto resblock = [&](const std::string& p, int64_t C, int64_t k) {
        for (int d = 0; d < 3; ++d) {
            const std::string i = std::to_string(d);
            conv(p + ".convs1." + i, C, k, C);
            conv(p + ".convs2." + i, C, k, C);
            s.emplace_back(p + ".activations1." + i + ".alpha", std::vector<int64_t>{C});
            s.emplace_back(p + ".activations2." + i + ".alpha", std::vector<int64_t>{C});
        }
    };
    for (int i = 0; i < 5; ++i) conv("f0_predictor.condnet." + std::to_string(2 * i), HF_C, i == 0 ? 4 : 3, i == 0 ? HF_NMELS : HF_C);
    s.emplace_back("f0_predictor.classifier.weight", std::vector<int64_t>{1, HF_C});
    s.emplace_back("f0_predictor.classifier.bias", std::vector<int64_t>{1});
    s.emplace_back("m_source.l_linear.weight", std::vector<int64_t>{1, HF_HARM});
    s.emplace_back("m_source.l_linear.bias", std::vector<int64_t>{1});
    conv("conv_pre", HF_C, 5, HF_NMELS);
    for (int i = 0; i < 3; ++i) {
        const std::string n = std::to_string(i);
        conv("ups." + n, HF_CH[i + 1], HF_UP_K[i], HF_CH[i]);
        conv("source_downs." + n, HF_CH[i + 1], HF_DOWN_K[i], HF_SPEC);
        resblock("source_resblocks." + n, HF_CH[i + 1], HF_SRC_K[i]);
        for (int j = 0; j < 3; ++j) resblock("resblocks." + std::to_string(3 * i + j), HF_CH[i + 1], HF_RES_K[j]);
    }
    conv("conv_post", HF_SPEC, 7, HF_CH[3]);
    return s;
}

// ---- kernels ------------------------------------------------------------------------------------------------------------------------
constexpr int HG_THREADS = 256, HG_T = HF_TILE, HG_K = 16;
enum { L_NONE = 0, L_LEAKY = 1, L_SNAKE = 2 };
enum { P_LIN = 0, P_ELU = 1, P_ABS = 2, P_RES = 3, P_MEAN = 4 };

// where the rows of a conv lie: ostart / istart the clips' first rows at the output / input level (nclips + 1 entries)
struct HfRows {
    const int *ostart, *istart;
    int nclips, stride, dil, lpad, up, reflect;
};

// x + 1 / (alpha + 1e-9) sin^2(alpha x), inv = 1 / (alpha + 1e-9) formed on the host in f32 (HiFiGAN.swift:22-24)
__device__ __forceinline__ float hf_snake(float x, float a, float inv) {
    const float s = sinf(a * x);
    return x + inv * (s * s);
}

// C[m][n] = epilogue(bias[n] + sum_k A(m, k) Wt[k][n]), k = j C_in + c; A [input rows][C_in], Wt [K][N], C and R [M][N].
// P_MEAN (the last conv of a ResBlock of the three whose mean a stage takes, HiFiGAN.swift:831-835): v = R + (. + bias) is the block's
// output; acc_mode 0: C = v; 1: C = C + v; 2: C = (C + v) / 3 -- blocks k = 3, 7, 11 in this order, as the reference adds them.
template <int LOAD, int EPI>
__global__ __launch_bounds__(HG_THREADS) void hf_conv_kernel(const float* __restrict__ A, long M, int Cin, HfRows rows,
                                                             const float* __restrict__ Wt, int K, int N, const float* __restrict__ bias,
                                                             float slope, const float* __restrict__ sa, const float* __restrict__ sinv,
                                                             const float* R, float* C, int acc_mode) {
    __shared__ __attribute__((aligned(16))) float As[HG_K][HG_T + 4];
    __shared__ __attribute__((aligned(16))) float Bs[HG_K][HG_T];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const long m0 = (long)blockIdx.x * HG_T;
    const int n0 = blockIdx.y * HG_T;
    int ibase[4], p0[4], vlen[4];                      // of each A row this thread loads: the clip's first input row, the position under
#pragma unroll                                         // tap 0, the clip's input length after upsampling (0: a row past M)
    for (int r = 0; r < 4; ++r) {
        const long m = m0 + ((tid + r * HG_THREADS) >> 4);
        ibase[r] = 0; p0[r] = 0; vlen[r] = 0;
        if (m < M) {
            const int clip = clip_of(rows.ostart, rows.nclips, m);
            int t = (int)(m - rows.ostart[clip]);
            if (rows.reflect) t = t == 0 ? 1 : t - 1;
            ibase[r] = rows.istart[clip];
            vlen[r] = (rows.istart[clip + 1] - rows.istart[clip]) * rows.up;
            p0[r] = t * rows.stride - rows.lpad;
        }
    }
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[i][q] = 0.0f;
    for (int k0 = 0; k0 < K; k0 += HG_K) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int idx = tid + r * HG_THREADS, row = idx >> 4, kk = idx & 15, k = k0 + kk;
            float v = 0.0f;                            // rows past M, inputs past K and positions outside the clip add exact zeros
            if (k < K) {
                const int j = k / Cin, c = k - j * Cin;
                const int p = p0[r] + j * rows.dil;
                if (p >= 0 && p < vlen[r]) {
                    v = A[(size_t)(ibase[r] + p / rows.up) * Cin + c];
                    if (LOAD == L_LEAKY) v = fmaxf(v, slope * v);      // maximum(x, slope x) (:794)
                    if (LOAD == L_SNAKE) v = hf_snake(v, sa[c], sinv[c]);
                }
            }
            As[kk][row] = v;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int idx = tid + r * HG_THREADS, kk = idx >> 6, col = idx & 63, k = k0 + kk, n = n0 + col;
            Bs[kk][col] = (k < K && n < N) ? Wt[(size_t)k * N + n] : 0.0f;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < HG_K; ++kk) {
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
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const long m = m0 + ty * 4 + i;
        if (m >= M) continue;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int n = n0 + tx * 4 + q;
            if (n >= N) continue;
            const size_t at = (size_t)m * N + n;
            float v = acc[i][q] + bias[n];
            if (EPI == P_ELU) v = v > 0.0f ? v : expf(v) - 1.0f;       // where(h > 0, h, exp(h) - 1) (:366)
            if (EPI == P_ABS) v = fabsf(v);
            if (EPI == P_RES) v = v + R[at];
            if (EPI == P_MEAN) {
                v = R[at] + v;
                if (acc_mode >= 1) v = C[at] + v;
                if (acc_mode == 2) v = v / 3.0f;
            }
            C[at] = v;
        }
    }
}

// base[(first + t) 9 + h] = the phase in cycles, reduced to [0, 1), at the start of frame t of clip blockIdx.x for harmonic h + 1:
// initPhase / 2 pi + the sum over earlier frames of 480 f0 (h + 1) / 24000 where f0 > 10 (:261-280; the cumsum runs over samples, F0
// is constant over a frame's 480).  f64, reduced after every frame: the sum over a long clip keeps its fraction.
__global__ void hf_phase_kernel(const float* __restrict__ f0, const int* __restrict__ start, const unsigned long long* __restrict__ seed,
                                double* __restrict__ base) {
    const int clip = blockIdx.x, h = threadIdx.x;
    if (h >= HF_HARM) return;
    const long first = start[clip], T = start[clip + 1] - first;
    double ph = (double)hift_uniform(hift_draw(seed[clip], (unsigned long long)h));
    for (long t = 0; t < T; ++t) {
        base[(first + t) * HF_HARM + h] = ph;
        const float f = f0[first + t];
        if (f > 10.0f) {
            ph += (double)HF_SAMPLES_PER_FRAME * ((double)f * (double)(h + 1) / (double)HF_RATE);
            ph -= floor(ph);
        }
    }
}

// src[n] of the pass (:253-289, :323-328): sample r of frame t has phase base + (r + 1) f0 (h + 1) / 24000 cycles.  sstart: the clips'
// first samples, fstart: their first frames.
__global__ __launch_bounds__(256) void hf_source_kernel(const float* __restrict__ f0, const double* __restrict__ base,
                                                        const int* __restrict__ sstart, const int* __restrict__ fstart, int nclips,
                                                        const unsigned long long* __restrict__ seed, const float* __restrict__ mw,
                                                        const float* __restrict__ mb, long total, float* __restrict__ src) {
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    if (g >= total) return;
    const int clip = clip_of(sstart, nclips, g);
    const long n = g - sstart[clip], t = n / HF_SAMPLES_PER_FRAME, frame = fstart[clip] + t;
    const int r = (int)(n - t * HF_SAMPLES_PER_FRAME);
    const unsigned long long s0 = seed[clip], ctr = 16ull + 10ull * (unsigned long long)n;
    const float f = f0[frame];
    const bool voiced = f > 10.0f;
    float acc = 0.0f;
#pragma unroll
    for (int h = 0; h < HF_HARM; ++h) {
        float v;
        if (voiced) {
            double ph = base[frame * HF_HARM + h] + (double)(r + 1) * ((double)f * (double)(h + 1) / (double)HF_RATE);
            ph -= floor(ph);
            v = 0.1f * sinf(6.28318530717958647692f * (float)ph);
        } else {
            v = 0.003f * hift_normal(hift_draw(s0, ctr + (unsigned long long)h));
        }
        acc = fmaf(v, mw[h], acc);
    }
    src[g] = tanhf(acc + mb[0]) + 0.003f * hift_normal(hift_draw(s0, ctr + 9ull));
}

// spec[frame][b] = sum_i hann[i] x[4 f + i - 8] cos(2 pi b i / 16), [9 + b]: - sin (:410-486); x reflects at the clip's ends (:441-447).
// fstart: the clips' first STFT frames (120 T + 1 each), sstart: their first samples; dcos, dsin [9][16].
__global__ __launch_bounds__(256) void hf_stft_kernel(const float* __restrict__ src, const int* __restrict__ fstart,
                                                      const int* __restrict__ sstart, int nclips, const float* __restrict__ hann,
                                                      const float* __restrict__ dcos, const float* __restrict__ dsin, long total,
                                                      float* __restrict__ spec) {
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    if (g >= total * HF_SPEC) return;
    const long row = g / HF_SPEC;
    const int ch = (int)(g - row * HF_SPEC), b = ch < HF_BINS ? ch : ch - HF_BINS;
    const int clip = clip_of(fstart, nclips, row);
    const long f = row - fstart[clip], N = sstart[clip + 1] - sstart[clip];
    const float* x = src + sstart[clip];
    const float* w = (ch < HF_BINS ? dcos : dsin) + b * HF_NFFT;
    float acc = 0.0f;
#pragma unroll
    for (int i = 0; i < HF_NFFT; ++i) {
        long p = f * HF_HOP + i - HF_NFFT / 2;
        if (p < 0) p = -p;
        else if (p >= N) p = 2 * N - 2 - p;
        acc = fmaf(x[p] * hann[i], w[i], acc);
    }
    spec[g] = acc;
}

// The tail (:838-857) for HF_TAIL_FRAMES hops of one clip: tiles[blockIdx.x] = (the clip's first row, its rows F = 120 T + 1, the tile's
// first hop q0, the clip's first PCM sample).  Hop q (samples 4 q .. 4 q + 3) gathers frames q, q - 1, q - 2, q - 3 in this order
// (the reference adds segment 0, 1, 2, 3 of them, :578-599); the window sum adds the frames in ascending order (:603-610).
// x [rows][64]; wt [448][18] (k = tap-major), cw, sw [16][16] the inverse DFT's cos / sin with the 1 / 16, hann [16].
constexpr int HT_FR = HF_TAIL_FRAMES + 3, HT_XR = HT_FR + 6;
__global__ __launch_bounds__(256) void hf_tail_kernel(const float* __restrict__ x, const int4* __restrict__ tiles, const float* __restrict__ wt,
                                                      const float* __restrict__ bias, const float* __restrict__ cw, const float* __restrict__ sw,
                                                      const float* __restrict__ hann, float* __restrict__ pcm) {
    __shared__ float sX[HT_XR][64 + 1];                // LeakyReLU(x) of rows q0 - 9 .. q0 + 63, zero before the clip (the conv's padding)
    __shared__ float sS[HT_FR][HF_SPEC + 1];           // conv_post of frames q0 - 3 .. q0 + 63
    __shared__ float sP[HT_FR][HF_SPEC + 1];           // their spectra, real | imaginary
    __shared__ float sT[HT_FR][HF_NFFT + 1];           // the windowed time frames
    const int tid = threadIdx.x;
    const int4 tile = tiles[blockIdx.x];
    const long first = tile.x, out0 = tile.w;
    const int F = tile.y, q0 = tile.z;
    for (int idx = tid; idx < HT_XR * 64; idx += 256) {
        const int r = idx >> 6, c = idx & 63, row = q0 - 9 + r;
        float v = 0.0f;
        if (row >= 0 && row < F) {
            v = x[(first + row) * 64 + c];
            v = fmaxf(v, 0.01f * v);
        }
        sX[r][c] = v;
    }
    __syncthreads();
    for (int idx = tid; idx < HT_FR * HF_SPEC; idx += 256) {
        const int fr = idx / HF_SPEC, ch = idx - fr * HF_SPEC;          // frame q0 - 3 + fr reads rows fr .. fr + 6 of sX
        float acc = 0.0f;
        for (int j = 0; j < 7; ++j)
            for (int c = 0; c < 64; ++c) acc = fmaf(sX[fr + j][c], wt[(j * 64 + c) * HF_SPEC + ch], acc);
        sS[fr][ch] = acc + bias[ch];
    }
    __syncthreads();
    for (int idx = tid; idx < HT_FR * HF_BINS; idx += 256) {
        const int fr = idx / HF_BINS, b = idx - fr * HF_BINS;
        const float mag = expf(sS[fr][b]), ph = sinf(sS[fr][HF_BINS + b]);             // yes, sin of the phase channels (:848-849)
        sP[fr][b] = mag * cosf(ph);
        sP[fr][HF_BINS + b] = mag * sinf(ph);
    }
    __syncthreads();
    for (int idx = tid; idx < HT_FR * HF_NFFT; idx += 256) {
        const int fr = idx >> 4, n = idx & 15;
        float re = 0.0f, im = 0.0f;
#pragma unroll
        for (int k = 0; k < HF_NFFT; ++k) {            // bins 9 .. 15 mirror 7 .. 1 with the imaginary part negated (:523-531)
            const int b = k < HF_BINS ? k : HF_NFFT - k;
            const float xr = sP[fr][b], xi = k < HF_BINS ? sP[fr][HF_BINS + b] : -sP[fr][HF_BINS + b];
            re = fmaf(xr, cw[n * HF_NFFT + k], re);
            im = fmaf(xi, sw[n * HF_NFFT + k], im);
        }
        sT[fr][n] = (re - im) * hann[n];
    }
    __syncthreads();
    {
        const int q = q0 + (tid >> 2), i = tid & 3, hops = F + 3;       // one thread per sample of the tile's 64 hops
        if (q < hops) {
            float acc = 0.0f, ws = 0.0f;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int f = q - s;
                if (f >= 0 && f < F) acc = acc + sT[f - (q0 - 3)][4 * s + i];
            }
#pragma unroll
            for (int s = 3; s >= 0; --s) {
                const int f = q - s;
                if (f >= 0 && f < F) ws = ws + hann[4 * s + i] * hann[4 * s + i];
            }
            const float v = acc / fmaxf(ws, 1e-8f);
            pcm[out0 + 4L * q + i] = fminf(fmaxf(v, -0.99f), 0.99f);
        }
    }
}

// ---- weights ------------------------------------------------------------------------------------------------------------------------
HiftCosyVoice::HiftCosyVoice(int device, const CheckedWeights& cw, long max_frames, hipStream_t work) : device_(device), max_frames_(max_frames) {
    if (max_frames < 1 || max_frames > HF_MAX_FRAMES) throw std::invalid_argument("HiFT vocoder: max_frames in 1..2^17");
    param_bytes_ = cw.disk_bytes;
    Builder b(cw);
    // Wt[j C_in + c][n] = W[n][j][c] of a conv stored [out][k][in] (WeightLoading.swift:234); a Linear [out][in] is k = 1
    auto conv = [&](const std::string& key, int Cout, int k, int Cin) {
        Conv cv; cv.K = k * Cin; cv.N = Cout; cv.Cin = Cin; cv.taps = k;
        const auto& Wm = b.t(key + ".weight");
        cv.wt = b.take((size_t)cv.K * cv.N);
        for (int n = 0; n < Cout; ++n)
            for (int kk = 0; kk < cv.K; ++kk) b.h[cv.wt + (size_t)kk * Cout + n] = Wm[(size_t)n * cv.K + kk];
        cv.bias = b.vec(key + ".bias");
        return cv;
    };
    auto snake = [&](const std::string& key, int C) {
        Snake s; s.a = b.vec(key + ".alpha"); s.inv = b.take(C);
        for (int c = 0; c < C; ++c) b.h[s.inv + c] = 1.0f / (b.h[s.a + c] + 1e-9f);
        return s;
    };
    auto resblock = [&](const std::string& p, int C, int k) {
        ResBlock rb; rb.k = k;
        for (int d = 0; d < 3; ++d) {
            const std::string i = std::to_string(d);
            rb.c1[d] = conv(p + ".convs1." + i, C, k, C);
            rb.c2[d] = conv(p + ".convs2." + i, C, k, C);
            rb.s1[d] = snake(p + ".activations1." + i, C);
            rb.s2[d] = snake(p + ".activations2." + i, C);
        }
        return rb;
    };
    for (int i = 0; i < 5; ++i) cond_[i] = conv("f0_predictor.condnet." + std::to_string(2 * i), HF_C, i == 0 ? 4 : 3, i == 0 ? HF_NMELS : HF_C);
    cls_ = conv("f0_predictor.classifier", 1, 1, HF_C);
    merge_w_ = b.vec("m_source.l_linear.weight");
    merge_b_ = b.vec("m_source.l_linear.bias");
    pre_ = conv("conv_pre", HF_C, 5, HF_NMELS);
    for (int i = 0; i < 3; ++i) {
        const std::string n = std::to_string(i);
        ups_[i] = conv("ups." + n, HF_CH[i + 1], HF_UP_K[i], HF_CH[i]);
        down_[i] = conv("source_downs." + n, HF_CH[i + 1], HF_DOWN_K[i], HF_SPEC);
        src_rb_[i] = resblock("source_resblocks." + n, HF_CH[i + 1], HF_SRC_K[i]);
        for (int j = 0; j < 3; ++j) rb_[i][j] = resblock("resblocks." + std::to_string(3 * i + j), HF_CH[i + 1], HF_RES_K[j]);
    }
    post_ = conv("conv_post", HF_SPEC, 7, HF_CH[3]);
    // the transforms' tables, Float of the f64 value as the reference forms them (:417-433, :539-559)
    hann_ = b.take(HF_NFFT);
    for (int n = 0; n < HF_NFFT; ++n) b.h[hann_ + n] = (float)(0.5 * (1.0 - cos(2.0 * M_PI * (double)n / (double)HF_NFFT)));
    dft_cos_ = b.take(HF_BINS * HF_NFFT); dft_sin_ = b.take(HF_BINS * HF_NFFT);
    for (int k = 0; k < HF_BINS; ++k)
        for (int n = 0; n < HF_NFFT; ++n) {
            const double a = 2.0 * M_PI * (double)k * (double)n / (double)HF_NFFT;
            b.h[dft_cos_ + k * HF_NFFT + n] = (float)cos(a);
            b.h[dft_sin_ + k * HF_NFFT + n] = (float)(-sin(a));
        }
    idft_cos_ = b.take(HF_NFFT * HF_NFFT); idft_sin_ = b.take(HF_NFFT * HF_NFFT);
    for (int n = 0; n < HF_NFFT; ++n)
        for (int k = 0; k < HF_NFFT; ++k) {
            const double a = 2.0 * M_PI * (double)n * (double)k / (double)HF_NFFT;
            b.h[idft_cos_ + n * HF_NFFT + k] = (float)(cos(a) * (1.0 / (double)HF_NFFT));
            b.h[idft_sin_ + n * HF_NFFT + k] = (float)(sin(a) * (1.0 / (double)HF_NFFT));
        }
    QASR_HIP(hipSetDevice(device_));
    QASR_HIP(hipStreamCreateWithFlags(&own_, hipStreamNonBlocking));
    work_ = work ? work : own_;
    for (auto& e : ev_) QASR_HIP(hipEventCreate(&e));
    d_w_.alloc(b.h.size() * sizeof(float));
    QASR_HIP(hipMemcpy(d_w_.p, b.h.data(), b.h.size() * sizeof(float), hipMemcpyHostToDevice));
    // a pass holds at most max_frames frames in at most min(HF_MAX_CLIPS, max_frames) clips; the widest level is 120 T + 1 rows of 64
    const size_t F = sizeof(float), T = (size_t)max_frames, clips = (size_t)std::min<long>(HF_MAX_CLIPS, max_frames);
    const size_t rows3 = HF_ROWS_PER_FRAME * T + clips;
    d_start_.alloc((size_t)6 * (HF_MAX_CLIPS + 1) * sizeof(int));
    d_seed_.alloc((size_t)HF_MAX_CLIPS * sizeof(unsigned long long));
    d_mel_.alloc(T * HF_NMELS * F);
    d_f0_.alloc(T * F);
    d_base_.alloc(T * HF_HARM * sizeof(double));
    d_src_.alloc(T * HF_SAMPLES_PER_FRAME * F);
    d_stft_.alloc(rows3 * HF_SPEC * F);
    d_pcm_.alloc((T * HF_SAMPLES_PER_FRAME + clips * HF_NFFT) * F);
    d_tiles_.alloc((rows3 / HF_TAIL_FRAMES + 2 * clips) * 4 * sizeof(int));      // a clip has (120 T + 4) / 64 + 1 tiles at most
    for (auto& buf : d_b_) buf.alloc(rows3 * 64 * F);  // 120 x 64 >= 40 x 128 >= 8 x 256 >= 512 floats per frame
}

HiftCosyVoice::~HiftCosyVoice() {
    if (work_) (void)hipStreamSynchronize(work_);
    for (auto& e : ev_) if (e) (void)hipEventDestroy(e);
    if (own_) (void)hipStreamDestroy(own_);
}

void HiftCosyVoice::unload() {
    if (!loaded_) return;
    QASR_HIP(hipSetDevice(device_));
    QASR_HIP(hipStreamSynchronize(work_));
    for (DevBuf* b : {&d_w_, &d_start_, &d_seed_, &d_mel_, &d_f0_, &d_base_, &d_src_, &d_stft_, &d_pcm_, &d_tiles_, &d_b_[0], &d_b_[1], &d_b_[2], &d_b_[3], &d_b_[4]})
        b->release();
    loaded_ = false;
}

void HiftCosyVoice::check_loaded() const {
    if (!loaded_) throw NotLoaded("HiFT vocoder: model unloaded");
}

// ---- a pass -------------------------------------------------------------------------------------------------------------------------
// levels of d_start_: 0 frames, 1 rows 8 T, 2 rows 40 T, 3 rows 120 T + 1, 4 samples 480 T, 5 PCM samples 480 T + 16
enum { LV_T = 0, LV_8 = 1, LV_40 = 2, LV_120 = 3, LV_SRC = 4, LV_PCM = 5 };
static long level_rows(int lv, long T) {
    switch (lv) {
        case LV_T: return T;
        case LV_8: return 8 * T;
        case LV_40: return 40 * T;
        case LV_120: return HF_ROWS_PER_FRAME * T + 1;
        case LV_SRC: return HF_SAMPLES_PER_FRAME * T;
        default: return HF_SAMPLES_PER_FRAME * T + HF_NFFT;
    }
}

template <int LOAD, int EPI>
static void launch_conv(hipStream_t st, const float* A, long M, const HfRows& rows, const float* Wt, int K, int N, int Cin, const float* bias,
                        float slope, const float* sa, const float* sinv, const float* R, float* C, int acc_mode) {
    const dim3 grid((unsigned)cdiv(M, HG_T), (unsigned)cdiv(N, HG_T));
    hipLaunchKernelGGL((hf_conv_kernel<LOAD, EPI>), grid, dim3(HG_THREADS), 0, st, A, M, Cin, rows, Wt, K, N, bias, slope, sa, sinv, R, C, acc_mode);
}

// d_mel_ -> d_f0_ (:361-373); records ev_[1]
void HiftCosyVoice::dev_f0() {
    const int* st = d_start_.as<int>() + LV_T * (HF_MAX_CLIPS + 1);
    float* pp[2] = {d_b_[0].as<float>(), d_b_[1].as<float>()};
    const float* in = d_mel_.as<float>();
    for (int i = 0; i < 5; ++i) {
        const Conv& c = cond_[i];
        const HfRows rows{st, st, n_clips_, 1, 1, i == 0 ? 0 : c.taps - 1, 1, 0};
        launch_conv<L_NONE, P_ELU>(work_, in, frames_, rows, W(c.wt), c.K, c.N, c.Cin, W(c.bias), 0.0f, nullptr, nullptr, nullptr, pp[i & 1], 0);
        in = pp[i & 1];
    }
    const HfRows rows{st, st, n_clips_, 1, 1, 0, 1, 0};
    launch_conv<L_NONE, P_ABS>(work_, in, frames_, rows, W(cls_.wt), cls_.K, 1, cls_.Cin, W(cls_.bias), 0.0f, nullptr, nullptr, nullptr,
                               d_f0_.as<float>(), 0);
    QASR_HIP(hipEventRecord(ev_[1], work_));
    QASR_HIP(hipGetLastError());
}

// d_f0_ -> d_src_ (:765-775); records ev_[2]
void HiftCosyVoice::dev_source() {
    const int *fst = d_start_.as<int>() + LV_T * (HF_MAX_CLIPS + 1), *sst = d_start_.as<int>() + LV_SRC * (HF_MAX_CLIPS + 1);
    const long total = frames_ * HF_SAMPLES_PER_FRAME;
    hipLaunchKernelGGL(hf_phase_kernel, dim3((unsigned)n_clips_), dim3(64), 0, work_, d_f0_.as<float>(), fst, d_seed_.as<unsigned long long>(),
                       d_base_.as<double>());
    hipLaunchKernelGGL(hf_source_kernel, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, work_, d_f0_.as<float>(), d_base_.as<double>(), sst, fst,
                       n_clips_, d_seed_.as<unsigned long long>(), W(merge_w_), W(merge_b_), total, d_src_.as<float>());
    QASR_HIP(hipEventRecord(ev_[2], work_));
    QASR_HIP(hipGetLastError());
}

// ResBlock (:211-221): h = x; three times h = h + convs2(snake(convs1(snake(h)))).  x is left alone, h and t1 are scratch; the last
// sum goes to `out`: acc_mode < 0 as it is (out may be h), else through the mean epilogue.
void HiftCosyVoice::resblock(const ResBlock& rb, const Level& lv, const float* x, float* h, float* t1, float* out, int acc_mode) {
    for (int d = 0; d < 3; ++d) {
        const Conv &c1 = rb.c1[d], &c2 = rb.c2[d];
        const float* in = d == 0 ? x : h;
        const HfRows r1{lv.start, lv.start, n_clips_, 1, HF_DIL[d], (rb.k - 1) * HF_DIL[d], 1, 0};
        const HfRows r2{lv.start, lv.start, n_clips_, 1, 1, rb.k - 1, 1, 0};
        launch_conv<L_SNAKE, P_LIN>(work_, in, lv.rows, r1, W(c1.wt), c1.K, c1.N, c1.Cin, W(c1.bias), 0.0f, W(rb.s1[d].a), W(rb.s1[d].inv), nullptr,
                                    t1, 0);
        if (d == 2 && acc_mode >= 0)
            launch_conv<L_SNAKE, P_MEAN>(work_, t1, lv.rows, r2, W(c2.wt), c2.K, c2.N, c2.Cin, W(c2.bias), 0.0f, W(rb.s2[d].a), W(rb.s2[d].inv), in,
                                         out, acc_mode);
        else
            launch_conv<L_SNAKE, P_RES>(work_, t1, lv.rows, r2, W(c2.wt), c2.K, c2.N, c2.Cin, W(c2.bias), 0.0f, W(rb.s2[d].a), W(rb.s2[d].inv), in,
                                        d == 2 ? out : h, 0);
    }
}

// d_mel_, d_src_ -> d_pcm_ (:777-857); records ev_[3] .. ev_[7]
void HiftCosyVoice::dev_decode() {
    const int* S = d_start_.as<int>();
    auto level = [&](int lv) { return Level{S + lv * (HF_MAX_CLIPS + 1), (long)h_start_[(size_t)lv * (HF_MAX_CLIPS + 1) + n_clips_]}; };
    const Level l0 = level(LV_T), l3 = level(LV_120), ls = level(LV_SRC);
    hipLaunchKernelGGL(hf_stft_kernel, dim3((unsigned)cdiv(l3.rows * HF_SPEC, 256)), dim3(256), 0, work_, d_src_.as<float>(), l3.start, ls.start,
                       n_clips_, W(hann_), W(dft_cos_), W(dft_sin_), l3.rows, d_stft_.as<float>());
    QASR_HIP(hipEventRecord(ev_[3], work_));
    float* B[5];
    for (int i = 0; i < 5; ++i) B[i] = d_b_[i].as<float>();
    float *cur = B[0], *sres = B[1], *t1 = B[2], *x = B[3], *mean = B[4];
    {
        const HfRows rows{l0.start, l0.start, n_clips_, 1, 1, 0, 1, 0};
        launch_conv<L_NONE, P_LIN>(work_, d_mel_.as<float>(), l0.rows, rows, W(pre_.wt), pre_.K, pre_.N, pre_.Cin, W(pre_.bias), 0.0f, nullptr, nullptr,
                                   nullptr, cur, 0);
    }
    QASR_HIP(hipEventRecord(ev_[4], work_));
    Level prev = l0;
    for (int i = 0; i < 3; ++i) {
        const Level lv = level(LV_8 + i);
        const int reflect = i == 2 ? 1 : 0;
        {                                              // source_downs[i](sourceSTFT) (:808-816), then source_resblocks[i] in place
            const Conv& c = down_[i];
            const HfRows rows{lv.start, l3.start, n_clips_, HF_DOWN_STRIDE[i], 1, HF_DOWN_STRIDE[i] - 1, 1, 0};
            launch_conv<L_NONE, P_LIN>(work_, d_stft_.as<float>(), lv.rows, rows, W(c.wt), c.K, c.N, c.Cin, W(c.bias), 0.0f, nullptr, nullptr, nullptr,
                                       sres, 0);
            resblock(src_rb_[i], lv, sres, sres, t1, sres, -1);
        }
        {                                              // LeakyReLU, upsample + conv, the reflected row, + the source branch (:794-827)
            const Conv& c = ups_[i];
            const HfRows rows{lv.start, prev.start, n_clips_, 1, 1, c.taps - 1, HF_RATES[i], reflect};
            launch_conv<L_LEAKY, P_RES>(work_, cur, lv.rows, rows, W(c.wt), c.K, c.N, c.Cin, W(c.bias), 0.1f, nullptr, nullptr, sres, x, 0);
        }
        for (int j = 0; j < 3; ++j) resblock(rb_[i][j], lv, x, sres, t1, mean, j);     // sres is free again: the blocks' running h
        std::swap(cur, mean);
        prev = lv;
        if (i < 2) QASR_HIP(hipEventRecord(ev_[5 + i], work_));
    }
    hipLaunchKernelGGL(hf_tail_kernel, dim3((unsigned)(h_tiles_.size() / 4)), dim3(256), 0, work_, cur, d_tiles_.as<int4>(), W(post_.wt), W(post_.bias), W(idft_cos_), W(idft_sin_), W(hann_),
                       d_pcm_.as<float>());
    QASR_HIP(hipEventRecord(ev_[7], work_));
    QASR_HIP(hipGetLastError());
}

// waits for the pass and adds the times of the stages that ran: 0 the F0 predictor, 1 the source, 2 .. 6 the decode
void HiftCosyVoice::finish(bool f0, bool source, bool decode) {
    QASR_HIP(hipStreamSynchronize(work_));
    QASR_HIP(hipGetLastError());
    for (int s = 0; s < HF_STAGES; ++s) {
        if (!(s == 0 ? f0 : s == 1 ? source : decode)) continue;
        float ms = 0;
        QASR_HIP(hipEventElapsedTime(&ms, ev_[s], ev_[s + 1]));
        timing_[s] += ms;
    }
}

void HiftCosyVoice::pass(const HiftClip* c, int n, Mode mode) {
    QASR_HIP(hipSetDevice(device_));
    QASR_HIP(hipStreamSynchronize(work_));             // the tables are rewritten
    n_clips_ = n;
    const size_t L = HF_MAX_CLIPS + 1;
    h_start_.assign(6 * L, 0);
    h_seed_.assign(HF_MAX_CLIPS, 0);
    frames_ = 0;
    for (int i = 0; i < n; ++i) {
        for (int lv = 0; lv < 6; ++lv) h_start_[lv * L + i + 1] = h_start_[lv * L + i] + (int)level_rows(lv, c[i].T);
        h_seed_[i] = c[i].seed;
        frames_ += c[i].T;
    }
    QASR_HIP(hipMemcpy(d_start_.p, h_start_.data(), h_start_.size() * sizeof(int), hipMemcpyHostToDevice));
    QASR_HIP(hipMemcpy(d_seed_.p, h_seed_.data(), h_seed_.size() * sizeof(unsigned long long), hipMemcpyHostToDevice));
    auto at = [&](int lv, int i) { return (size_t)h_start_[lv * L + i]; };
    if (mode != SOURCE)
        for (int i = 0; i < n; ++i)
            QASR_HIP(hipMemcpy(d_mel_.as<float>() + at(LV_T, i) * HF_NMELS, c[i].mel, (size_t)c[i].T * HF_NMELS * sizeof(float), hipMemcpyHostToDevice));
    if (mode == SOURCE)
        for (int i = 0; i < n; ++i)
            QASR_HIP(hipMemcpy(d_f0_.as<float>() + at(LV_T, i), c[i].f0_in, (size_t)c[i].T * sizeof(float), hipMemcpyHostToDevice));
    if (mode == DECODE_SOURCE)
        for (int i = 0; i < n; ++i)
            QASR_HIP(hipMemcpy(d_src_.as<float>() + at(LV_SRC, i), c[i].src_in, (size_t)level_rows(LV_SRC, c[i].T) * sizeof(float),
                               hipMemcpyHostToDevice));
    h_tiles_.clear();
    for (int i = 0; i < n; ++i) {
        const int F = (int)level_rows(LV_120, c[i].T);
        for (int q0 = 0; q0 < F + 3; q0 += HF_TAIL_FRAMES)
            for (int v : {(int)at(LV_120, i), F, q0, (int)at(LV_PCM, i)}) h_tiles_.push_back(v);
    }
    if (h_tiles_.size() * sizeof(int) > d_tiles_.bytes) throw std::length_error("HiFT vocoder: a pass exceeds its buffers");
    QASR_HIP(hipMemcpy(d_tiles_.p, h_tiles_.data(), h_tiles_.size() * sizeof(int), hipMemcpyHostToDevice));
    const bool run_f0 = mode == F0 || mode == DECODE, run_src = mode == SOURCE || mode == DECODE, run_dec = mode == DECODE_SOURCE || mode == DECODE;
    QASR_HIP(hipEventRecord(ev_[0], work_));           // every event is recorded in order; finish() counts the stages that ran
    if (run_f0) dev_f0(); else QASR_HIP(hipEventRecord(ev_[1], work_));
    if (run_src) dev_source(); else QASR_HIP(hipEventRecord(ev_[2], work_));
    if (run_dec) dev_decode();
    else for (int s = 3; s <= HF_STAGES; ++s) QASR_HIP(hipEventRecord(ev_[s], work_));
    for (int i = 0; i < n; ++i) {
        if (mode == F0)
            QASR_HIP(hipMemcpyAsync(c[i].f0_out, d_f0_.as<float>() + at(LV_T, i), (size_t)c[i].T * sizeof(float), hipMemcpyDeviceToHost, work_));
        else if (mode == SOURCE)
            QASR_HIP(hipMemcpyAsync(c[i].src_out, d_src_.as<float>() + at(LV_SRC, i), (size_t)level_rows(LV_SRC, c[i].T) * sizeof(float),
                                    hipMemcpyDeviceToHost, work_));
        else
            QASR_HIP(hipMemcpyAsync(c[i].pcm, d_pcm_.as<float>() + at(LV_PCM, i), (size_t)level_rows(LV_PCM, c[i].T) * sizeof(float),
                                    hipMemcpyDeviceToHost, work_));
    }
    finish(run_f0, run_src, run_dec);
}

// ---- entry points -------------------------------------------------------------------------------------------------------------------
void HiftCosyVoice::run(const std::vector<HiftClip>& clips, Mode mode) {
    check_loaded();
    for (float& t : timing_) t = 0.0f;
    for (size_t i = 0; i < clips.size(); ++i)
        if (clips[i].T < 1 || clips[i].T > max_frames_)
            throw std::invalid_argument("HiFT vocoder: clip " + std::to_string(i) + " holds " + std::to_string(clips[i].T) +
                                        " frames, a clip holds 1.." + std::to_string(max_frames_) + " (max_frames)");
    for (size_t i = 0; i < clips.size();) {            // passes end at clip boundaries
        size_t j = i;
        long total = 0;
        while (j < clips.size() && j - i < (size_t)HF_MAX_CLIPS && total + clips[j].T <= max_frames_) total += clips[j++].T;
        pass(clips.data() + i, (int)(j - i), mode);
        i = j;
    }
}

}  // namespace qasr
