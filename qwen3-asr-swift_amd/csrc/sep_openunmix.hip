// sep_openunmix.hip -- Open-Unmix source separation for gfx950 (sep_openunmix.h).  f32 throughout, accurate expf / tanhf / sqrtf, no
// float atomics, no vendor FFT or BLAS.
//
// Launches of one pass over B files (M = sum of their frame counts T_b; the four stems are one grid dimension of every network launch):
//   sep_stft_kernel        one workgroup per (frame, channel): the reference's centre-pad index rule at the load, periodic Hann, a 4096-point
//                          complex Stockham radix-4 FFT in LDS (six passes, the form of mel_core.h's 256-point one), bins 0..2048 and
//                          their magnitude written together.
//   sep_gemm_kernel        the 64 x 64 tiled f32 GEMM of seg_proj_kernel, generalised over how A is read and what the epilogue does:
//                          fc1 (crop + input affine at the load; BN + tanh), the LSTM input projections of both directions (+ b_ih),
//                          fc2 ([skip | lstm] at the load; BN + ReLU), fc3 (BN, output affine, ReLU, x mixture magnitude).
//   sep_recur_kernel       grid (stem x direction, group of 4 files), 1024 threads: a thread owns one (hidden 512) or two (hidden 1024)
//                          gate rows of W_hh for the group's 4 files; W_hh streams from L2 each step as coalesced rows of the
//                          transposed matrix (a kept alternative holds the first KRES columns of its rows in registers: at 1024
//                          threads the 128 registers go to the accumulators and the loads in flight, so it spills; DESIGN.md
//                          section 14 has the measurement); h of the 4 files is broadcast from LDS;
//                          the next step's pre-gates are loaded one step ahead.  No workgroup waits for another.
//   sep_wmax / sep_cov / sep_gain   Wiener EM per window of frames: window maximum (fixed tree), one pass that forms y, v and the five
//                          covariance sums per (source, bin) as a sequential chain over the window's frames, one pass that applies the gain.
//   sep_phase_kernel       without Wiener: masked magnitude on the mixture's unit phasor.
//   sep_istft_kernel       a workgroup owns 16 output segments of 1024 samples of one (stem, file, channel): it walks the frames that
//                          touch them in frame order (Hermitian extension, inverse FFT, 1 / N, window), adds each into a four-slot ring of
//                          segments in LDS and retires a segment once its last frame is in: every sample is the sum of its <= 4 frames in
//                          frame order, whatever the chunking, divided by max(sum w^2, 1e-8).
// Summation order: every GEMM output is one thread's fmaf chain over k = 0..K-1; a gate's recurrent dot is four
// interleaved chains (k mod 4) over k = 0..Hd-1 combined as (a0 + a1) + (a2 + a3), the same for the resident and the streamed columns; the
// FFT butterflies are fixed; the covariance sums run over a window's frames in order.  The batch size, a file's place in it and the pass
// split never enter, so a file's stems are bit-identical alone, in any batch and under any max_batch_samples.
#include "sep_openunmix.h"
#include <algorithm>
#include <cmath>
#include <cstring>

namespace qasr {

const char* const SEP_STEM_NAMES[SEP_STEMS] = {"vocals", "drums", "bass", "other"};

constexpr int SEP_NP = 4160;                                  // fc3 outputs padded to a multiple of the GEMM tile
constexpr int SEP_BINP = 2052, SEP_MBP = 1488;                // padded vector lengths

// ---- device weight block of one stem (floats; every offset a multiple of 4) ----------------------------------------------------------
struct SepLayout {
    int H, in_mean, in_scale, fc1, bn1, wx[SEP_LAYERS], bih[SEP_LAYERS], bhh[SEP_LAYERS], wh[SEP_LAYERS], fc2, bn2, fc3, bn3, oscale, omean, total;
};
static SepLayout sep_layout(int H) {
    SepLayout L;
    int o = 0;
    auto take = [&](int n) { const int at = o; o += (n + 3) & ~3; return at; };
    L.H = H;
    L.in_mean = take(SEP_MBP); L.in_scale = take(SEP_MBP);
    L.fc1 = take(SEP_IN * H); L.bn1 = take(4 * H);
    for (int l = 0; l < SEP_LAYERS; ++l) {
        L.wx[l] = take(H * 4 * H); L.bih[l] = take(4 * H); L.bhh[l] = take(4 * H);
        L.wh[l] = take(2 * (H / 2) * 2 * H);                 // [dir][Hd k][4 Hd rows]
    }
    L.fc2 = take(2 * H * H); L.bn2 = take(4 * H);
    L.fc3 = take(H * SEP_NP); L.bn3 = take(4 * SEP_NP);
    L.oscale = take(SEP_BINP); L.omean = take(SEP_BINP);
    L.total = o;
    return L;
}

struct SepStems { int n; int id[SEP_STEMS]; };

__device__ __forceinline__ float sep_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// ---- table: Hann window [4096] | twiddles [4096][2] = cos, sin(-2 pi k / 4096) ----------------------------------------------------
constexpr int TB_WIN = 0, TB_TW = SEP_NFFT, TB_TOTAL = 3 * SEP_NFFT;
constexpr int FFT_THREADS = 1024;
constexpr size_t FFT_LDS = (size_t)2 * SEP_NFFT * sizeof(float2);        // two ping-pong buffers, 64 KB

// 4096-point complex FFT of a[0..4095] by 1024 threads (Stockham radix-4, Ns = 1, 4, .., 1024); the result is back in `a` after the six
// passes.  INV: conjugate twiddles and the +i rotation, unscaled.  Ends with a barrier.
template <bool INV>
__device__ __forceinline__ void sep_fft4096(float2* a, float2* b, const float2* __restrict__ tw, int tid) {
    float2* src = a;
    float2* dst = b;
#pragma unroll
    for (int pass = 0; pass < 6; ++pass) {
        const int Ns = 1 << (2 * pass);
        float2 v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = src[tid + 1024 * r];
        const int k = tid & (Ns - 1);
        const int tstep = k * (1024 / Ns);            // w4096^(tstep r), tstep r < 3072
        if (pass > 0) {
#pragma unroll
            for (int r = 1; r < 4; ++r) {
                float2 t = tw[tstep * r];
                if (INV) t.y = -t.y;
                v[r] = make_float2(v[r].x * t.x - v[r].y * t.y, v[r].x * t.y + v[r].y * t.x);
            }
        }
        const float2 t0 = make_float2(v[0].x + v[2].x, v[0].y + v[2].y);
        const float2 t1 = make_float2(v[0].x - v[2].x, v[0].y - v[2].y);
        const float2 t2 = make_float2(v[1].x + v[3].x, v[1].y + v[3].y);
        const float2 d = make_float2(v[1].x - v[3].x, v[1].y - v[3].y);
        const float2 t3 = INV ? make_float2(-d.y, d.x) : make_float2(d.y, -d.x);     // (v1 - v3) x (+i | -i)
        const int base = (tid / Ns) * Ns * 4 + k;
        dst[base] = make_float2(t0.x + t2.x, t0.y + t2.y);
        dst[base + Ns] = make_float2(t1.x + t3.x, t1.y + t3.y);
        dst[base + 2 * Ns] = make_float2(t0.x - t2.x, t0.y - t2.y);
        dst[base + 3 * Ns] = make_float2(t1.x - t3.x, t1.y - t3.y);
        __syncthreads();
        float2* tmp = src; src = dst; dst = tmp;
    }
}

// per-file tables, all long: n[B] | off[B] | T[B] | row0[B]
__global__ __launch_bounds__(FFT_THREADS) void sep_stft_kernel(const float* __restrict__ pcm, long total, const long* __restrict__ meta, int B,
                                                               const int* __restrict__ rowfile, const float* __restrict__ tab,
                                                               float* __restrict__ re, float* __restrict__ im, float* __restrict__ mag) {
    extern __shared__ float2 fft_lds[];
    float2* a = fft_lds;
    float2* b = fft_lds + SEP_NFFT;
    const long m = blockIdx.x;
    const int c = blockIdx.y, tid = threadIdx.x;
    const int f = rowfile[m];
    const long n = meta[f], off = meta[B + f], t = m - meta[3 * B + f];
    const float* x = pcm + (long)c * total + off;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = tid + 1024 * r;
        const long p = t * SEP_HOP + i;                // position in the padded signal (STFT.swift:43-58)
        long src;
        if (p < SEP_NFFT / 2) src = max(0L, min((long)(SEP_NFFT / 2) - p, n - 1));
        else if (p < SEP_NFFT / 2 + n) src = p - SEP_NFFT / 2;
        else src = max(0L, n - 2 - (p - SEP_NFFT / 2 - n));
        a[i] = make_float2(x[src] * tab[TB_WIN + i], 0.0f);
    }
    __syncthreads();
    sep_fft4096<false>(a, b, reinterpret_cast<const float2*>(tab + TB_TW), tid);
    const long o = (m * 2 + c) * SEP_BINS;
    for (int k = tid; k < SEP_BINS; k += FFT_THREADS) {
        const float2 z = a[k];
        re[o + k] = z.x;
        im[o + k] = z.y;
        mag[o + k] = sqrtf(z.x * z.x + z.y * z.y);     // STFT.swift:98
    }
}

// ---- inverse STFT (STFT.swift:183-231) ---------------------------------------------------------------------------------------------
constexpr int IS_SEGS = 16;
constexpr size_t IS_LDS = FFT_LDS + (size_t)SEP_NFFT * sizeof(float);

// yre / yim [J][M][2][2049]; out: file f at J * 2 * off_f, [J][2][n_f]
__global__ __launch_bounds__(FFT_THREADS) void sep_istft_kernel(const float* __restrict__ yre, const float* __restrict__ yim, long M,
                                                                const long* __restrict__ meta, int B, int J,
                                                                const float* __restrict__ tab, float* __restrict__ out) {
    extern __shared__ float2 fft_lds[];
    float2* a = fft_lds;
    float2* b = fft_lds + SEP_NFFT;
    float* ring = reinterpret_cast<float*>(fft_lds + 2 * SEP_NFFT);     // [4][1024]
    const int chunk = blockIdx.x, c = blockIdx.y, tid = threadIdx.x;
    const int j = blockIdx.z / B, f = blockIdx.z - j * B;
    const long n = meta[f], off = meta[B + f], T = meta[2 * B + f], row0 = meta[3 * B + f];
    const long last_seg = (SEP_NFFT / 2 + n - 1) / SEP_HOP;            // padded segment of the last kept sample
    const long s_first = 2 + (long)chunk * IS_SEGS;
    if (s_first > last_seg) return;
    const long s_last = min(s_first + IS_SEGS - 1, last_seg);
    const float* win = tab + TB_WIN;
    const float2* tw = reinterpret_cast<const float2*>(tab + TB_TW);
    float* o = out + (long)J * 2 * off + ((long)j * 2 + c) * n;
#pragma unroll
    for (int r = 0; r < 4; ++r) ring[tid + 1024 * r] = 0.0f;
    for (long fr = max(0L, s_first - 3); fr <= s_last; ++fr) {
        if (fr < T) {
            const long src = (((long)j * M + row0 + fr) * 2 + c) * SEP_BINS;
            __syncthreads();
            for (int k = tid; k < SEP_BINS; k += FFT_THREADS) {         // mirror the one-sided spectrum (STFT.swift:137-144)
                const float xr = yre[src + k], xi = yim[src + k];
                a[k] = make_float2(xr, xi);
                if (k >= 1 && k < SEP_NFFT / 2) a[SEP_NFFT - k] = make_float2(xr, -xi);
            }
            __syncthreads();
            sep_fft4096<true>(a, b, tw, tid);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = tid + 1024 * r;
                ring[((fr + r) & 3) * 1024 + tid] += (a[i].x * (1.0f / SEP_NFFT)) * win[i];
            }
        }
        // segment fr has all its frames (fr - 3 .. fr): write it and free its slot (each thread owns its ring entries: no barrier)
        const int slot = (int)(fr & 3) * 1024 + tid;
        if (fr >= s_first) {
            const long p = fr * SEP_HOP + tid, i = p - SEP_NFFT / 2;
            if (i >= 0 && i < n) {
                float ws = 0.0f;
                for (long g = max(0L, fr - 3); g <= min(fr, T - 1); ++g) {
                    const float w = win[p - g * SEP_HOP];
                    ws += w * w;
                }
                o[i] = ring[slot] / fmaxf(ws, 1e-8f);
            }
        }
        ring[slot] = 0.0f;
    }
}

// ---- tiled f32 GEMM with fused loads and epilogues ---------------------------------------------------------------------------------
constexpr int GM_THREADS = 256, GM_T = 64, GM_K = 16;
enum { A_FC1 = 0, A_PLAIN = 1, A_CAT = 2 };
enum { E_BN_TANH = 0, E_BIAS = 1, E_BN_RELU = 2, E_MASK = 3 };

// C[j][m][0..N) = epilogue(sum_k A_j[m][k] Wt_j[k][n]).  Wt is [K][ldb] (ldb a multiple of 64, columns past N zero).  BN vectors at
// offE: running_mean | 1 / sqrt(running_var + eps) | weight | bias, each ldb long.
template <int AMODE, int EPI>
__global__ __launch_bounds__(GM_THREADS) void sep_gemm_kernel(const float* __restrict__ A, const float* __restrict__ A2, long M, int K,
                                                              const float* __restrict__ W, size_t wstride, int offB, int ldb, int offE,
                                                              int offA, int N, SepStems st, float* __restrict__ C, int ldc,
                                                              const float* __restrict__ mag) {
    __shared__ __attribute__((aligned(16))) float As[GM_K][GM_T + 4];
    __shared__ __attribute__((aligned(16))) float Bs[GM_K][GM_T];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4, j = blockIdx.z;
    const long m0 = (long)blockIdx.x * GM_T;
    const int n0 = blockIdx.y * GM_T;
    const float* Ws = W + (size_t)st.id[j] * wstride;
    const float* Bt = Ws + offB;
    const int split = K / 2;
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[i][q] = 0.0f;
    for (int k0 = 0; k0 < K; k0 += GM_K) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int idx = tid + r * GM_THREADS, row = idx >> 4, kk = idx & 15, k = k0 + kk;
            const long m = m0 + row;
            float v = 0.0f;                            // rows past M and inputs past K add exact zeros
            if (m < M && k < K) {
                if (AMODE == A_FC1) {                  // crop to 1487 bins, (x + input_mean) * input_scale (OpenUnmixModel.swift:96-101)
                    const int c = k / SEP_MAXBIN, bin = k - c * SEP_MAXBIN;
                    v = (A[(m * 2 + c) * SEP_BINS + bin] + Ws[offA + bin]) * Ws[offA + SEP_MBP + bin];
                } else if (AMODE == A_PLAIN) {
                    v = A[((long)j * M + m) * K + k];
                } else {                               // [skip | lstm] (:111)
                    v = k < split ? A[((long)j * M + m) * split + k] : A2[((long)j * M + m) * split + (k - split)];
                }
            }
            As[kk][row] = v;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int idx = tid + r * GM_THREADS, kk = idx >> 6, col = idx & 63, k = k0 + kk;
            Bs[kk][col] = k < K ? Bt[(size_t)k * ldb + n0 + col] : 0.0f;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < GM_K; ++kk) {
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
    const float* E = Ws + offE;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int n = n0 + tx * 4 + q;
        if (n >= N) continue;
        float e0 = E[n], e1 = 0.0f, e2 = 0.0f, e3 = 0.0f, os = 0.0f, om = 0.0f;
        if (EPI != E_BIAS) { e1 = E[ldb + n]; e2 = E[2 * ldb + n]; e3 = E[3 * ldb + n]; }
        if (EPI == E_MASK) {
            const int bin = n >= SEP_BINS ? n - SEP_BINS : n;
            os = E[4 * ldb + bin];
            om = E[4 * ldb + SEP_BINP + bin];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const long m = m0 + ty * 4 + i;
            if (m >= M) continue;
            float v = acc[i][q];
            if (EPI == E_BIAS) v = v + e0;
            else v = ((v - e0) * e1) * e2 + e3;        // BatchNorm on running statistics (MLXNN BatchNorm in eval mode, eps 1e-5)
            if (EPI == E_BN_TANH) v = tanhf(v);
            if (EPI == E_BN_RELU) v = fmaxf(v, 0.0f);
            if (EPI == E_MASK) v = fmaxf(v * os + om, 0.0f) * mag[m * SEP_OUT + n];      // :120-126
            C[((long)j * M + m) * ldc + n] = v;
        }
    }
}

// ---- LSTM recurrence (OpenUnmixModel.swift:175-301) --------------------------------------------------------------------------------
constexpr int RC_THREADS = 1024, RC_FILES = 4;

// pre [J][M][2][4 HD] (x W_ih^T + b_ih), Wt [dir][HD k][4 HD rows], bhh [2][4 HD], hout [J][M][2 HD].  grid (J x 2, file groups).
template <int HD, int KRES>
__global__ __launch_bounds__(RC_THREADS) void sep_recur_kernel(const float* __restrict__ W, size_t wstride, int offWh, int offBhh,
                                                               SepStems st, const float* __restrict__ pre, long M,
                                                               const long* __restrict__ meta, int B, float* __restrict__ hout) {
    constexpr int G4 = 4 * HD, ROWS = G4 / RC_THREADS, CELLS = RC_FILES * HD / RC_THREADS;
    __shared__ __attribute__((aligned(16))) float s_h[RC_FILES][HD];
    __shared__ float s_gate[RC_FILES][G4];
    const int tid = threadIdx.x, j = blockIdx.x >> 1, dir = blockIdx.x & 1, f0 = blockIdx.y * RC_FILES;
    const float* Ws = W + (size_t)st.id[j] * wstride;
    const float* Wt = Ws + offWh + (size_t)dir * HD * G4;
    long T[RC_FILES], row0[RC_FILES];
    long Tmax = 0;
#pragma unroll
    for (int f = 0; f < RC_FILES; ++f) {
        const bool in = f0 + f < B;
        T[f] = in ? meta[2 * B + f0 + f] : 0;
        row0[f] = in ? meta[3 * B + f0 + f] : 0;
        Tmax = max(Tmax, T[f]);
    }
    float bh[ROWS], wres[ROWS][KRES > 0 ? KRES : 1];
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        bh[r] = Ws[offBhh + dir * G4 + tid + r * RC_THREADS];
#pragma unroll
        for (int k = 0; k < KRES; ++k) wres[r][k] = Wt[(size_t)k * G4 + tid + r * RC_THREADS];
    }
    float cst[CELLS];
#pragma unroll
    for (int i = 0; i < CELLS; ++i) cst[i] = 0.0f;    // h0 = c0 = 0 (:180-181)
    for (int i = tid; i < RC_FILES * HD; i += RC_THREADS) (&s_h[0][0])[i] = 0.0f;
    __syncthreads();
    // frame of file f at step s: forward s, backward T_f - 1 - s (:192); a file takes part while s < T_f
    const float* pj = pre + (long)j * M * (2 * G4) + dir * G4;
    float pnext[ROWS][RC_FILES];
#pragma unroll
    for (int f = 0; f < RC_FILES; ++f)
#pragma unroll
        for (int r = 0; r < ROWS; ++r)
            pnext[r][f] = T[f] > 0 ? pj[(row0[f] + (dir ? T[f] - 1 : 0)) * (2 * G4) + tid + r * RC_THREADS] : 0.0f;
    for (long s = 0; s < Tmax; ++s) {
        float pcur[ROWS][RC_FILES];
#pragma unroll
        for (int f = 0; f < RC_FILES; ++f)
#pragma unroll
            for (int r = 0; r < ROWS; ++r) {
                pcur[r][f] = pnext[r][f];
                if (s + 1 < T[f]) pnext[r][f] = pj[(row0[f] + (dir ? T[f] - 2 - s : s + 1)) * (2 * G4) + tid + r * RC_THREADS];
            }
        float acc[ROWS][RC_FILES][4];
#pragma unroll
        for (int r = 0; r < ROWS; ++r)
#pragma unroll
            for (int f = 0; f < RC_FILES; ++f)
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[r][f][q] = 0.0f;
#pragma unroll
        for (int k = 0; k < KRES; k += 4) {
#pragma unroll
            for (int f = 0; f < RC_FILES; ++f) {
                const float4 hv = lds_read_f4(&s_h[f][k]);
#pragma unroll
                for (int r = 0; r < ROWS; ++r) {
                    acc[r][f][0] = fmaf(wres[r][k], hv.x, acc[r][f][0]);
                    acc[r][f][1] = fmaf(wres[r][k + 1], hv.y, acc[r][f][1]);
                    acc[r][f][2] = fmaf(wres[r][k + 2], hv.z, acc[r][f][2]);
                    acc[r][f][3] = fmaf(wres[r][k + 3], hv.w, acc[r][f][3]);
                }
            }
        }
#pragma unroll 4
        for (int k = KRES; k < HD; k += 4) {
            float w[ROWS][4];
#pragma unroll
            for (int r = 0; r < ROWS; ++r)
#pragma unroll
                for (int q = 0; q < 4; ++q) w[r][q] = Wt[(size_t)(k + q) * G4 + tid + r * RC_THREADS];
#pragma unroll
            for (int f = 0; f < RC_FILES; ++f) {
                const float4 hv = lds_read_f4(&s_h[f][k]);
#pragma unroll
                for (int r = 0; r < ROWS; ++r) {
                    acc[r][f][0] = fmaf(w[r][0], hv.x, acc[r][f][0]);
                    acc[r][f][1] = fmaf(w[r][1], hv.y, acc[r][f][1]);
                    acc[r][f][2] = fmaf(w[r][2], hv.z, acc[r][f][2]);
                    acc[r][f][3] = fmaf(w[r][3], hv.w, acc[r][f][3]);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < ROWS; ++r)
#pragma unroll
            for (int f = 0; f < RC_FILES; ++f)         // x W_ih^T + b_ih + h W_hh^T + b_hh (:289)
                s_gate[f][tid + r * RC_THREADS] = (pcur[r][f] + ((acc[r][f][0] + acc[r][f][1]) + (acc[r][f][2] + acc[r][f][3]))) + bh[r];
        __syncthreads();
#pragma unroll
        for (int i = 0; i < CELLS; ++i) {
            const int cell = tid + i * RC_THREADS, f = cell / HD, u = cell - f * HD;
            if (s < T[f]) {                            // i, f, g, o (:293-300)
                const float ig = sep_sigmoid(s_gate[f][u]), fg = sep_sigmoid(s_gate[f][HD + u]);
                const float gg = tanhf(s_gate[f][2 * HD + u]), og = sep_sigmoid(s_gate[f][3 * HD + u]);
                cst[i] = fg * cst[i] + ig * gg;
                const float h = og * tanhf(cst[i]);
                s_h[f][u] = h;
                const long t = dir ? T[f] - 1 - s : s;
                hout[((long)j * M + row0[f] + t) * (2 * HD) + dir * HD + u] = h;
            }
        }
        __syncthreads();
    }
}

// ---- Wiener EM (WienerFilterMLX.swift:139-261) ---------------------------------------------------------------------------------------
constexpr int WN_THREADS = 1024, WV_THREADS = 256;
constexpr float WN_EPS = 1e-10f;

// win: (row0, len) per window.  scale[w] = max(1, max |mix| / 10) over both channels of the window (:147-150); max is exact in any order.
__global__ __launch_bounds__(WN_THREADS) void sep_wmax_kernel(const float* __restrict__ re, const float* __restrict__ im,
                                                              const long* __restrict__ win, float* __restrict__ scale) {
    __shared__ float red[WN_THREADS];
    const int w = blockIdx.x, tid = threadIdx.x;
    const long base = win[2 * w] * SEP_OUT, cnt = win[2 * w + 1] * SEP_OUT;
    float mx = 0.0f;
    for (long i = tid; i < cnt; i += WN_THREADS) {
        const float a = re[base + i], b = im[base + i];
        mx = fmaxf(mx, sqrtf(a * a + b * b));
    }
    red[tid] = mx;
    __syncthreads();
    for (int s = WN_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] = fmaxf(red[tid], red[tid + s]);
        __syncthreads();
    }
    if (tid == 0) scale[w] = fmaxf(1.0f, red[0] / 10.0f);
}

// thread = (bin, source, window).  FIRST: y = masked magnitude x unit phasor of the mixture / scale, written to yre / yim (:154-167).
// cov [window][J][4][2049]: R00, R01re, R01im, R11 = frame sums / (sum v + eps) (:175-193), the sums taken in frame order.
template <bool FIRST>
__global__ __launch_bounds__(WV_THREADS) void sep_cov_kernel(const float* __restrict__ mask, const float* __restrict__ re,
                                                             const float* __restrict__ im, long M, int J, const long* __restrict__ win,
                                                             const float* __restrict__ scale, float* __restrict__ yre,
                                                             float* __restrict__ yim, float* __restrict__ cov) {
    const int bin = blockIdx.x * WV_THREADS + threadIdx.x, j = blockIdx.y, w = blockIdx.z;
    if (bin >= SEP_BINS) return;
    const long r0 = win[2 * w], len = win[2 * w + 1];
    const float s = 1.0f / scale[w];
    float s00 = 0.0f, sre = 0.0f, sim = 0.0f, s11 = 0.0f, sv = 0.0f;
    for (long t = 0; t < len; ++t) {
        const long xl = (r0 + t) * SEP_OUT + bin, xr = xl + SEP_BINS;
        const long yl = ((long)j * M + r0 + t) * SEP_OUT + bin, yr = yl + SEP_BINS;
        float aRe, aIm, bRe, bIm;
        if (FIRST) {
            const float lr = re[xl], li = im[xl], rr = re[xr], ri = im[xr];
            const float ml = fmaxf(sqrtf(lr * lr + li * li), WN_EPS), mr = fmaxf(sqrtf(rr * rr + ri * ri), WN_EPS);
            const float tl = mask[yl], tr = mask[yr];
            aRe = tl * (lr / ml) * s; aIm = tl * (li / ml) * s;
            bRe = tr * (rr / mr) * s; bIm = tr * (ri / mr) * s;
            yre[yl] = aRe; yim[yl] = aIm; yre[yr] = bRe; yim[yr] = bIm;
        } else {
            aRe = yre[yl]; aIm = yim[yl]; bRe = yre[yr]; bIm = yim[yr];
        }
        const float v = 0.5f * (aRe * aRe + aIm * aIm + bRe * bRe + bIm * bIm);
        s00 += aRe * aRe + aIm * aIm;
        sre += aRe * bRe + aIm * bIm;
        sim += aIm * bRe - aRe * bIm;
        s11 += bRe * bRe + bIm * bIm;
        sv += v;
    }
    sv += WN_EPS;
    float* c = cov + ((long)w * J + j) * 4 * SEP_BINS + bin;
    c[0] = s00 / sv; c[SEP_BINS] = sre / sv; c[2 * SEP_BINS] = sim / sv; c[3 * SEP_BINS] = s11 / sv;
}

// thread = (bin, frame): mixture covariance over the sources in source order, its 2x2 complex inverse, W_j = G_j C^-1, y_j = W_j x
// (:195-252).  The products with the reference's all-zero imaginary parts of G's diagonal (g0iZ, g3iZ) are left out: they add +-0.
// LAST: the result is scaled back by the window's scale (:256-260).
template <int J, bool LAST>
__global__ __launch_bounds__(WV_THREADS) void sep_gain_kernel(const float* __restrict__ re, const float* __restrict__ im, long M,
                                                              const int* __restrict__ rowwin, const float* __restrict__ scale,
                                                              const float* __restrict__ cov, float* __restrict__ yre,
                                                              float* __restrict__ yim) {
    const int bin = blockIdx.x * WV_THREADS + threadIdx.x;
    const long m = blockIdx.y;
    if (bin >= SEP_BINS) return;
    const int w = rowwin[m];
    const float sd = scale[w], s = 1.0f / sd;
    const long xl = m * SEP_OUT + bin, xr = xl + SEP_BINS;
    const float xLR = re[xl] * s, xLI = im[xl] * s, xRR = re[xr] * s, xRI = im[xr] * s;
    float g0r[J], g1r[J], g1i[J], g3r[J];
    float c00 = 0.0f, c01re = 0.0f, c01im = 0.0f, c11 = 0.0f;
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const long yl = ((long)j * M + m) * SEP_OUT + bin, yr = yl + SEP_BINS;
        const float aRe = yre[yl], aIm = yim[yl], bRe = yre[yr], bIm = yim[yr];
        const float v = 0.5f * (aRe * aRe + aIm * aIm + bRe * bRe + bIm * bIm);
        const float* c = cov + ((long)w * J + j) * 4 * SEP_BINS + bin;
        g0r[j] = v * c[0]; g1r[j] = v * c[SEP_BINS]; g1i[j] = v * c[2 * SEP_BINS]; g3r[j] = v * c[3 * SEP_BINS];
        c00 += g0r[j]; c01re += g1r[j]; c01im += g1i[j]; c11 += g3r[j];
    }
    c00 += WN_EPS; c11 += WN_EPS;
    const float c10re = c01re, c10im = -c01im;
    const float detRe = (c00 * c11) - (c01re * c10re - c01im * c10im);
    const float detIm = -(c01re * c10im + c01im * c10re);
    const float detMag2 = detRe * detRe + detIm * detIm + WN_EPS * WN_EPS;
    const float idR = detRe / detMag2, idI = -detIm / detMag2;
    const float i0r = c11 * idR, i0i = c11 * idI;
    const float i1r = -(c01re * idR - c01im * idI), i1i = -(c01re * idI + c01im * idR);
    const float i2r = -(c10re * idR - c10im * idI), i2i = -(c10re * idI + c10im * idR);
    const float i3r = c00 * idR, i3i = c00 * idI;
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const float g2r = g1r[j], g2i = -g1i[j];
        const float w0r = (g0r[j] * i0r) + (g1r[j] * i2r - g1i[j] * i2i);
        const float w0i = (g0r[j] * i0i) + (g1r[j] * i2i + g1i[j] * i2r);
        const float w1r = (g0r[j] * i1r) + (g1r[j] * i3r - g1i[j] * i3i);
        const float w1i = (g0r[j] * i1i) + (g1r[j] * i3i + g1i[j] * i3r);
        const float w2r = (g2r * i0r - g2i * i0i) + (g3r[j] * i2r);
        const float w2i = (g2r * i0i + g2i * i0r) + (g3r[j] * i2i);
        const float w3r = (g2r * i1r - g2i * i1i) + (g3r[j] * i3r);
        const float w3i = (g2r * i1i + g2i * i1r) + (g3r[j] * i3i);
        float yLR = w0r * xLR - w0i * xLI + w1r * xRR - w1i * xRI;
        float yLI = w0r * xLI + w0i * xLR + w1r * xRI + w1i * xRR;
        float yRR = w2r * xLR - w2i * xLI + w3r * xRR - w3i * xRI;
        float yRI = w2r * xLI + w2i * xLR + w3r * xRI + w3i * xRR;
        if (LAST) { yLR *= sd; yLI *= sd; yRR *= sd; yRI *= sd; }
        const long yl = ((long)j * M + m) * SEP_OUT + bin, yr = yl + SEP_BINS;
        yre[yl] = yLR; yim[yl] = yLI; yre[yr] = yRR; yim[yr] = yRI;
    }
}

// without Wiener (STFT.swift:240-260): mag cos / sin(atan2(im, re)) stated as mag re / |x|, mag im / |x|, and (mag, 0) at |x| = 0
__global__ __launch_bounds__(WV_THREADS) void sep_phase_kernel(const float* __restrict__ mask, const float* __restrict__ re,
                                                               const float* __restrict__ im, long M, float* __restrict__ yre,
                                                               float* __restrict__ yim) {
    const long i = (long)blockIdx.x * WV_THREADS + threadIdx.x, cnt = M * SEP_OUT;
    if (i >= cnt) return;
    const float a = re[i], b = im[i], r = sqrtf(a * a + b * b);
    const float t = mask[(long)blockIdx.y * cnt + i];
    yre[(long)blockIdx.y * cnt + i] = r > 0.0f ? t * (a / r) : t;
    yim[(long)blockIdx.y * cnt + i] = r > 0.0f ? t * (b / r) : 0.0f;
}

// ---- weights ------------------------------------------------------------------------------------------------------------------------
std::vector<std::pair<std::string, std::vector<int64_t>>> sep_tensor_shapes(int H) {
    std::vector<std::pair<std::string, std::vector<int64_t>>> v = {
        {"input_mean", {SEP_MAXBIN}}, {"input_scale", {SEP_MAXBIN}}, {"output_mean", {SEP_BINS}}, {"output_scale", {SEP_BINS}},
        {"fc1.weight", {H, SEP_IN}}, {"fc2.weight", {H, 2 * H}}, {"fc3.weight", {SEP_OUT, H}},
    };
    const int feat[3] = {H, H, SEP_OUT};
    for (int i = 0; i < 3; ++i)
        for (const char* k : {"weight", "bias", "running_mean", "running_var"})
            v.push_back({"bn" + std::to_string(i + 1) + "." + k, {feat[i]}});
    for (int l = 0; l < SEP_LAYERS; ++l)
        for (const char* d : {"forward", "backward"}) {
            const std::string p = "lstm.layers." + std::to_string(l) + "." + d + ".";
            v.push_back({p + "weight_ih", {2 * H, H}});      // 4 x hidden / 2 gates; the input is hidden wide in every layer
            v.push_back({p + "weight_hh", {2 * H, H / 2}});
            v.push_back({p + "bias_ih", {2 * H}});
            v.push_back({p + "bias_hh", {2 * H}});
        }
    return v;
}

// BatchNorm vectors: running_mean | 1 / sqrt(running_var + 1e-5) | weight | bias, stride ld.  eps is MLXNN.BatchNorm's default: the
// reference tree does not hold mlx-swift, and OpenUnmixModel.swift:71 passes none.
static void put_bn(std::vector<float>& h, size_t at, int ld, int n, const CheckedWeights& w, const std::string& p) {
    const auto &g = w.t.at(p + ".weight"), &b = w.t.at(p + ".bias"), &rm = w.t.at(p + ".running_mean"), &rv = w.t.at(p + ".running_var");
    for (int i = 0; i < n; ++i) {
        h[at + i] = rm[i];
        h[at + ld + i] = 1.0f / sqrtf(rv[i] + 1e-5f);
        h[at + 2 * ld + i] = g[i];
        h[at + 3 * ld + i] = b[i];
    }
}

SepOpenUnmix::SepOpenUnmix(int device, const CheckedWeights* w, int hidden, size_t max_batch_samples, hipStream_t work)
    : device_(device), hidden_(hidden), max_samples_(max_batch_samples) {
    if (hidden != 512 && hidden != 1024) throw std::invalid_argument("open-unmix: hidden size 512 (umxhq) or 1024 (umxl)");
    const int H = hidden, Hd = H / 2, G4 = 2 * H;
    const SepLayout L = sep_layout(H);
    stem_stride_ = (size_t)L.total;
    std::vector<float> h((size_t)SEP_STEMS * L.total, 0.0f);
    for (int s = 0; s < SEP_STEMS; ++s) {
        const CheckedWeights& cw = w[s];
        param_bytes_ += cw.disk_bytes;
        const size_t b = (size_t)s * L.total;
        for (int i = 0; i < SEP_MAXBIN; ++i) { h[b + L.in_mean + i] = cw.t.at("input_mean")[i]; h[b + L.in_scale + i] = cw.t.at("input_scale")[i]; }
        for (int i = 0; i < SEP_BINS; ++i) { h[b + L.oscale + i] = cw.t.at("output_scale")[i]; h[b + L.omean + i] = cw.t.at("output_mean")[i]; }
        const auto &f1 = cw.t.at("fc1.weight"), &f2 = cw.t.at("fc2.weight"), &f3 = cw.t.at("fc3.weight");
        for (int o = 0; o < H; ++o) {
            for (int i = 0; i < SEP_IN; ++i) h[b + L.fc1 + (size_t)i * H + o] = f1[(size_t)o * SEP_IN + i];
            for (int i = 0; i < 2 * H; ++i) h[b + L.fc2 + (size_t)i * H + o] = f2[(size_t)o * 2 * H + i];
        }
        for (int o = 0; o < SEP_OUT; ++o)
            for (int i = 0; i < H; ++i) h[b + L.fc3 + (size_t)i * SEP_NP + o] = f3[(size_t)o * H + i];
        put_bn(h, b + L.bn1, H, H, cw, "bn1");
        put_bn(h, b + L.bn2, H, H, cw, "bn2");
        put_bn(h, b + L.bn3, SEP_NP, SEP_OUT, cw, "bn3");
        for (int l = 0; l < SEP_LAYERS; ++l)
            for (int d = 0; d < 2; ++d) {
                const std::string p = "lstm.layers." + std::to_string(l) + (d ? ".backward." : ".forward.");
                const auto &wi = cw.t.at(p + "weight_ih"), &wh = cw.t.at(p + "weight_hh"), &bi = cw.t.at(p + "bias_ih"), &bhh = cw.t.at(p + "bias_hh");
                for (int g = 0; g < G4; ++g) {
                    for (int i = 0; i < H; ++i) h[b + L.wx[l] + (size_t)i * 4 * H + d * G4 + g] = wi[(size_t)g * H + i];
                    for (int k = 0; k < Hd; ++k) h[b + L.wh[l] + ((size_t)d * Hd + k) * G4 + g] = wh[(size_t)g * Hd + k];
                    h[b + L.bih[l] + d * G4 + g] = bi[g];
                    h[b + L.bhh[l] + d * G4 + g] = bhh[g];
                }
            }
    }
    std::vector<float> tab(TB_TOTAL);
    for (int i = 0; i < SEP_NFFT; ++i) {
        tab[TB_WIN + i] = 0.5f * (1.0f - cosf(2.0f * (float)M_PI * (float)i / (float)SEP_NFFT));      // STFT.swift:25-27, in f32
        const double a = -2.0 * M_PI * i / (double)SEP_NFFT;
        tab[TB_TW + 2 * i] = (float)cos(a);
        tab[TB_TW + 2 * i + 1] = (float)sin(a);
    }
    QASR_HIP(hipSetDevice(device_));
    QASR_HIP(hipStreamCreateWithFlags(&own_, hipStreamNonBlocking));
    work_ = work ? work : own_;
    for (auto& e : ev_) QASR_HIP(hipEventCreate(&e));
    d_w_.alloc(h.size() * sizeof(float));
    QASR_HIP(hipMemcpy(d_w_.p, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
    d_tab_.alloc(tab.size() * sizeof(float));
    QASR_HIP(hipMemcpy(d_tab_.p, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice));
    ensure_dynamic_lds(reinterpret_cast<const void*>(&sep_stft_kernel), (int)FFT_LDS);
    ensure_dynamic_lds(reinterpret_cast<const void*>(&sep_istft_kernel), (int)IS_LDS);
}

SepOpenUnmix::~SepOpenUnmix() {
    if (work_) (void)hipStreamSynchronize(work_);
    for (auto& e : ev_) if (e) (void)hipEventDestroy(e);
    if (own_) (void)hipStreamDestroy(own_);
}

void SepOpenUnmix::unload() {
    if (!loaded_) return;
    QASR_HIP(hipSetDevice(device_));
    QASR_HIP(hipStreamSynchronize(work_));
    for (DevBuf* b : {&d_w_, &d_tab_, &d_meta_, &d_rowfile_, &d_win_, &d_pcm_, &d_re_, &d_im_, &d_mag_, &d_mask_, &d_yre_, &d_yim_, &d_x1_,
                      &d_pre_, &d_h_[0], &d_h_[1], &d_f2_, &d_cov_, &d_scale_, &d_audio_})
        b->release();
    cap_rows_ = cap_net_ = cap_cplx_ = cap_samples_ = cap_audio_ = cap_win_ = cap_files_ = cap_mask_ = cap_nwin_ = 0;
    loaded_ = false;
}

void SepOpenUnmix::check_loaded() const {
    if (!loaded_) throw NotLoaded("open-unmix: model unloaded");
}

// ---- geometry and workspace ---------------------------------------------------------------------------------------------------------
void SepOpenUnmix::plan(const size_t* n, const size_t* T, size_t B) {
    QASR_HIP(hipSetDevice(device_));
    QASR_HIP(hipStreamSynchronize(work_));             // the tables are rewritten
    p_ = Plan();
    p_.B = (int)B;
    for (size_t b = 0; b < B; ++b) {
        const long nb = n ? (long)n[b] : 0, Tb = T ? (long)T[b] : sep_num_frames((size_t)nb);
        if (Tb <= 0 || Tb > (1L << 30)) throw std::invalid_argument("open-unmix: frame count out of range");
        p_.n.push_back(nb); p_.off.push_back(p_.total); p_.T.push_back((int)Tb); p_.row0.push_back((int)p_.M);
        p_.total += nb; p_.M += Tb;
    }
    if (p_.M > (1L << 30)) throw std::length_error("open-unmix: more than 2^30 frames in one pass");
    std::vector<long> meta(4 * B);
    std::vector<int> rowfile((size_t)p_.M);
    for (size_t b = 0; b < B; ++b) {
        meta[b] = p_.n[b]; meta[B + b] = p_.off[b]; meta[2 * B + b] = p_.T[b]; meta[3 * B + b] = p_.row0[b];
        std::fill(rowfile.begin() + p_.row0[b], rowfile.begin() + p_.row0[b] + p_.T[b], (int)b);
    }
    if ((long)B > cap_files_) { cap_files_ = (long)B; d_meta_.alloc(4 * B * sizeof(long)); }
    QASR_HIP(hipMemcpy(d_meta_.p, meta.data(), meta.size() * sizeof(long), hipMemcpyHostToDevice));
    ensure_rows(p_.M, false, false);
    QASR_HIP(hipMemcpy(d_rowfile_.p, rowfile.data(), rowfile.size() * sizeof(int), hipMemcpyHostToDevice));
}

// window table of the pass: (row0, len) per window | row -> window, uploaded to d_win_
void SepOpenUnmix::plan_windows(int window) {
    std::vector<long> win;
    std::vector<int> rowwin((size_t)p_.M);
    n_win_ = 0;
    for (int b = 0; b < p_.B; ++b)
        for (long pos = 0; pos < p_.T[b]; pos += window) {             // WienerFilterMLX.swift:54-75: the last window is shorter
            const long len = std::min((long)window, (long)p_.T[b] - pos);
            win.push_back(p_.row0[b] + pos); win.push_back(len);
            std::fill(rowwin.begin() + p_.row0[b] + pos, rowwin.begin() + p_.row0[b] + pos + len, n_win_);
            ++n_win_;
        }
    const size_t need = win.size() * sizeof(long) + rowwin.size() * sizeof(int);
    QASR_HIP(hipStreamSynchronize(work_));
    if ((long)need > cap_win_) { cap_win_ = (long)need; d_win_.alloc(need); }
    if (n_win_ > cap_nwin_) {
        cap_nwin_ = n_win_;
        d_scale_.alloc((size_t)n_win_ * sizeof(float));
        d_cov_.alloc((size_t)n_win_ * SEP_STEMS * 4 * SEP_BINS * sizeof(float));
    }
    QASR_HIP(hipMemcpy(d_win_.p, win.data(), win.size() * sizeof(long), hipMemcpyHostToDevice));
    QASR_HIP(hipMemcpy(d_win_.as<char>() + win.size() * sizeof(long), rowwin.data(), rowwin.size() * sizeof(int), hipMemcpyHostToDevice));
}

void SepOpenUnmix::ensure_rows(long M, bool net, bool cplx) {
    const size_t row = (size_t)SEP_OUT * sizeof(float), H = (size_t)hidden_;
    if (M > cap_rows_) {
        QASR_HIP(hipStreamSynchronize(work_));
        cap_rows_ = M;
        d_rowfile_.alloc((size_t)M * sizeof(int));
        d_re_.alloc(M * row); d_im_.alloc(M * row); d_mag_.alloc(M * row);
    }
    if ((net || cplx) && M > cap_mask_) {
        QASR_HIP(hipStreamSynchronize(work_));
        cap_mask_ = M;
        d_mask_.alloc(SEP_STEMS * M * row);
    }
    if (net && M > cap_net_) {
        QASR_HIP(hipStreamSynchronize(work_));
        cap_net_ = M;
        d_x1_.alloc(SEP_STEMS * M * H * sizeof(float));
        d_pre_.alloc(SEP_STEMS * M * 4 * H * sizeof(float));
        d_h_[0].alloc(SEP_STEMS * M * H * sizeof(float));
        d_h_[1].alloc(SEP_STEMS * M * H * sizeof(float));
        d_f2_.alloc(SEP_STEMS * M * H * sizeof(float));
    }
    if (cplx && M > cap_cplx_) {
        QASR_HIP(hipStreamSynchronize(work_));
        cap_cplx_ = M;
        d_yre_.alloc(SEP_STEMS * M * row);
        d_yim_.alloc(SEP_STEMS * M * row);
    }
}

void SepOpenUnmix::ensure_samples(long total, int J) {
    if (total > cap_samples_) {
        QASR_HIP(hipStreamSynchronize(work_));
        cap_samples_ = total;
        d_pcm_.alloc((size_t)2 * total * sizeof(float));
    }
    if ((long)J * 2 * total > cap_audio_) {
        QASR_HIP(hipStreamSynchronize(work_));
        cap_audio_ = (long)J * 2 * total;
        d_audio_.alloc((size_t)cap_audio_ * sizeof(float));
    }
}

float SepOpenUnmix::elapsed(int a, int b) {
    float ms = 0.0f;
    QASR_HIP(hipEventElapsedTime(&ms, ev_[a], ev_[b]));
    return ms;
}

// ---- the stages on device buffers, in stream order ----------------------------------------------------------------------------------
void SepOpenUnmix::dev_stft() {
    hipLaunchKernelGGL(sep_stft_kernel, dim3((unsigned)p_.M, 2), dim3(FFT_THREADS), FFT_LDS, work_, d_pcm_.as<float>(), p_.total,
                       d_meta_.as<long>(), p_.B, d_rowfile_.as<int>(), d_tab_.as<float>(), d_re_.as<float>(), d_im_.as<float>(),
                       d_mag_.as<float>());
    QASR_HIP(hipGetLastError());
}

void SepOpenUnmix::dev_masks(unsigned targets) {
    SepStems st{0, {0, 0, 0, 0}};
    for (int s = 0; s < SEP_STEMS; ++s)
        if (targets & (1u << s)) st.id[st.n++] = s;
    const int H = hidden_, J = st.n;
    const long M = p_.M;
    const SepLayout L = sep_layout(H);
    const float* W = d_w_.as<float>();
    const float* none = nullptr;
    const unsigned mt = (unsigned)cdiv(M, GM_T);
    hipStream_t s = work_;
    float *x1 = d_x1_.as<float>(), *pre = d_pre_.as<float>(), *f2 = d_f2_.as<float>();
    hipLaunchKernelGGL((sep_gemm_kernel<A_FC1, E_BN_TANH>), dim3(mt, H / GM_T, J), dim3(GM_THREADS), 0, s, d_mag_.as<float>(), none, M, SEP_IN,
                       W, stem_stride_, L.fc1, H, L.bn1, L.in_mean, H, st, x1, H, none);
    const float* x = x1;
    for (int l = 0; l < SEP_LAYERS; ++l) {
        float* hout = d_h_[l & 1].as<float>();
        hipLaunchKernelGGL((sep_gemm_kernel<A_PLAIN, E_BIAS>), dim3(mt, 4 * H / GM_T, J), dim3(GM_THREADS), 0, s, x, none, M, H, W,
                           stem_stride_, L.wx[l], 4 * H, L.bih[l], 0, 4 * H, st, pre, 4 * H, none);
        const dim3 grid(2 * J, cdiv(p_.B, RC_FILES));
#define SEP_RECUR(HD, KRES)                                                                                                          \
    hipLaunchKernelGGL((sep_recur_kernel<HD, KRES>), grid, dim3(RC_THREADS), 0, s, W, stem_stride_, L.wh[l], L.bhh[l], st, pre, M, \
                       d_meta_.as<long>(), p_.B, hout)
        if (H == 512) { if (recur_form_ == 1) SEP_RECUR(256, 64); else SEP_RECUR(256, 0); }
        else { if (recur_form_ == 1) SEP_RECUR(512, 32); else SEP_RECUR(512, 0); }
#undef SEP_RECUR
        x = hout;
    }
    hipLaunchKernelGGL((sep_gemm_kernel<A_CAT, E_BN_RELU>), dim3(mt, H / GM_T, J), dim3(GM_THREADS), 0, s, x1, x, M, 2 * H, W, stem_stride_,
                       L.fc2, H, L.bn2, 0, H, st, f2, H, none);
    hipLaunchKernelGGL((sep_gemm_kernel<A_PLAIN, E_MASK>), dim3(mt, SEP_NP / GM_T, J), dim3(GM_THREADS), 0, s, f2, none, M, H, W, stem_stride_,
                       L.fc3, SEP_NP, L.bn3, 0, SEP_OUT, st, d_mask_.as<float>(), SEP_OUT, d_mag_.as<float>());
    QASR_HIP(hipGetLastError());
}

void SepOpenUnmix::dev_wiener(int J, int iterations) {
    const long M = p_.M;
    const long* win = d_win_.as<long>();
    const int* rowwin = reinterpret_cast<const int*>(d_win_.as<char>() + (size_t)n_win_ * 2 * sizeof(long));
    float *yre = d_yre_.as<float>(), *yim = d_yim_.as<float>(), *cov = d_cov_.as<float>(), *scale = d_scale_.as<float>();
    const float *re = d_re_.as<float>(), *im = d_im_.as<float>(), *mask = d_mask_.as<float>();
    hipStream_t s = work_;
    hipLaunchKernelGGL(sep_wmax_kernel, dim3(n_win_), dim3(WN_THREADS), 0, s, re, im, win, scale);
    const dim3 cgrid(cdiv(SEP_BINS, WV_THREADS), J, n_win_), ggrid(cdiv(SEP_BINS, WV_THREADS), (unsigned)M);
    for (int it = 0; it < iterations; ++it) {
        if (it == 0) hipLaunchKernelGGL(sep_cov_kernel<true>, cgrid, dim3(WV_THREADS), 0, s, mask, re, im, M, J, win, scale, yre, yim, cov);
        else hipLaunchKernelGGL(sep_cov_kernel<false>, cgrid, dim3(WV_THREADS), 0, s, mask, re, im, M, J, win, scale, yre, yim, cov);
        const bool last = it + 1 == iterations;
#define SEP_GAIN(JJ)                                                                                                                 \
    if (last) hipLaunchKernelGGL((sep_gain_kernel<JJ, true>), ggrid, dim3(WV_THREADS), 0, s, re, im, M, rowwin, scale, cov, yre, yim); \
    else hipLaunchKernelGGL((sep_gain_kernel<JJ, false>), ggrid, dim3(WV_THREADS), 0, s, re, im, M, rowwin, scale, cov, yre, yim)
        if (J == 1) { SEP_GAIN(1); } else if (J == 2) { SEP_GAIN(2); } else if (J == 3) { SEP_GAIN(3); } else { SEP_GAIN(4); }
#undef SEP_GAIN
    }
    QASR_HIP(hipGetLastError());
}

void SepOpenUnmix::dev_phase(int J) {
    hipLaunchKernelGGL(sep_phase_kernel, dim3(cdiv(p_.M * SEP_OUT, WV_THREADS), J), dim3(WV_THREADS), 0, work_, d_mask_.as<float>(),
                       d_re_.as<float>(), d_im_.as<float>(), p_.M, d_yre_.as<float>(), d_yim_.as<float>());
    QASR_HIP(hipGetLastError());
}

void SepOpenUnmix::dev_istft(int J) {
    long nmax = 0;
    for (long n : p_.n) nmax = std::max(nmax, n);
    const long last_seg = (SEP_NFFT / 2 + nmax - 1) / SEP_HOP;
    const dim3 grid(cdiv(last_seg - 1, IS_SEGS), 2, (unsigned)(J * p_.B));
    hipLaunchKernelGGL(sep_istft_kernel, grid, dim3(FFT_THREADS), IS_LDS, work_, d_yre_.as<float>(), d_yim_.as<float>(), p_.M,
                       d_meta_.as<long>(), p_.B, J, d_tab_.as<float>(), d_audio_.as<float>());
    QASR_HIP(hipGetLastError());
}

// ---- entry points -------------------------------------------------------------------------------------------------------------------
static int popcount4(unsigned t) { return (int)((t & 1) + ((t >> 1) & 1) + ((t >> 2) & 1) + ((t >> 3) & 1)); }

void SepOpenUnmix::separate(const float* const* left, const float* const* right, const size_t* n, size_t B, unsigned targets, bool wiener,
                            int iterations, int window, float* const* out) {
    check_loaded();
    const int J = popcount4(targets);
    if (J == 0 || (targets & ~0xFu)) throw std::invalid_argument("open-unmix: target mask names no stem or an unknown one");
    if (iterations < 1 || iterations > 16 || window < 1) throw std::invalid_argument("open-unmix: wiener_iterations in 1..16, wiener_window >= 1");
    for (size_t b = 0; b < B; ++b)
        if (n[b] > max_samples_)
            throw std::length_error("open-unmix: file " + std::to_string(b) + " has " + std::to_string(n[b]) + " samples, more than max_batch_samples " +
                                    std::to_string(max_samples_));
    const bool em = wiener && J > 1;                   // SourceSeparation.swift:127
    timing_ = SepTiming();
    for (size_t b0 = 0; b0 < B;) {
        size_t b1 = b0, sum = 0;
        while (b1 < B && (b1 == b0 || sum + n[b1] <= max_samples_)) sum += n[b1++];
        plan(n + b0, nullptr, b1 - b0);
        ensure_rows(p_.M, true, true);
        ensure_samples(p_.total, J);
        if (em) plan_windows(window);
        for (size_t b = b0; b < b1; ++b) {             // mono is duplicated (SourceSeparation.swift:52-58)
            const long off = p_.off[b - b0];
            QASR_HIP(hipMemcpyAsync(d_pcm_.as<float>() + off, left[b], n[b] * sizeof(float), hipMemcpyHostToDevice, work_));
            QASR_HIP(hipMemcpyAsync(d_pcm_.as<float>() + p_.total + off, right[b] ? right[b] : left[b], n[b] * sizeof(float),
                                    hipMemcpyHostToDevice, work_));
        }
        QASR_HIP(hipEventRecord(ev_[0], work_));
        dev_stft();
        QASR_HIP(hipEventRecord(ev_[1], work_));
        dev_masks(targets);
        QASR_HIP(hipEventRecord(ev_[2], work_));
        if (em) dev_wiener(J, iterations); else dev_phase(J);
        QASR_HIP(hipEventRecord(ev_[3], work_));
        dev_istft(J);
        QASR_HIP(hipEventRecord(ev_[4], work_));
        for (size_t b = b0; b < b1; ++b)
            QASR_HIP(hipMemcpyAsync(out[b], d_audio_.as<float>() + (size_t)J * 2 * p_.off[b - b0], (size_t)J * 2 * n[b] * sizeof(float),
                                    hipMemcpyDeviceToHost, work_));
        QASR_HIP(hipStreamSynchronize(work_));
        QASR_HIP(hipGetLastError());
        timing_.stft += elapsed(0, 1); timing_.network += elapsed(1, 2); timing_.wiener += elapsed(2, 3); timing_.istft += elapsed(3, 4);
        b0 = b1;
    }
}

void SepOpenUnmix::stft(const float* left, const float* right, size_t n, float* re, float* im, float* mag) {
    check_loaded();
    plan(&n, nullptr, 1);
    ensure_samples(p_.total, 1);
    QASR_HIP(hipMemcpyAsync(d_pcm_.as<float>(), left, n * sizeof(float), hipMemcpyHostToDevice, work_));
    QASR_HIP(hipMemcpyAsync(d_pcm_.as<float>() + n, right ? right : left, n * sizeof(float), hipMemcpyHostToDevice, work_));
    QASR_HIP(hipEventRecord(ev_[0], work_));
    dev_stft();
    QASR_HIP(hipEventRecord(ev_[1], work_));
    const size_t bytes = (size_t)p_.M * SEP_OUT * sizeof(float);
    if (re) QASR_HIP(hipMemcpyAsync(re, d_re_.p, bytes, hipMemcpyDeviceToHost, work_));
    if (im) QASR_HIP(hipMemcpyAsync(im, d_im_.p, bytes, hipMemcpyDeviceToHost, work_));
    if (mag) QASR_HIP(hipMemcpyAsync(mag, d_mag_.p, bytes, hipMemcpyDeviceToHost, work_));
    QASR_HIP(hipStreamSynchronize(work_));
    timing_ = SepTiming();
    timing_.stft = elapsed(0, 1);
}

void SepOpenUnmix::masks(const float* mag, const size_t* T, size_t B, float* out) {
    check_loaded();
    plan(nullptr, T, B);
    ensure_rows(p_.M, true, false);
    const size_t bytes = (size_t)p_.M * SEP_OUT * sizeof(float);
    QASR_HIP(hipMemcpyAsync(d_mag_.p, mag, bytes, hipMemcpyHostToDevice, work_));
    QASR_HIP(hipEventRecord(ev_[0], work_));
    dev_masks(0xFu);
    QASR_HIP(hipEventRecord(ev_[1], work_));
    QASR_HIP(hipMemcpyAsync(out, d_mask_.p, SEP_STEMS * bytes, hipMemcpyDeviceToHost, work_));
    QASR_HIP(hipStreamSynchronize(work_));
    timing_ = SepTiming();
    timing_.network = elapsed(0, 1);
}

void SepOpenUnmix::wiener(const float* masked, int J, const float* re, const float* im, size_t T, int iterations, int window, float* out_re,
                          float* out_im) {
    check_loaded();
    if (J < 1 || J > SEP_STEMS) throw std::invalid_argument("open-unmix: 1..4 sources");
    if (iterations < 1 || iterations > 16 || window < 1) throw std::invalid_argument("open-unmix: wiener_iterations in 1..16, wiener_window >= 1");
    plan(nullptr, &T, 1);
    ensure_rows(p_.M, false, true);
    plan_windows(window);
    const size_t bytes = (size_t)p_.M * SEP_OUT * sizeof(float);
    QASR_HIP(hipMemcpyAsync(d_mask_.p, masked, J * bytes, hipMemcpyHostToDevice, work_));
    QASR_HIP(hipMemcpyAsync(d_re_.p, re, bytes, hipMemcpyHostToDevice, work_));
    QASR_HIP(hipMemcpyAsync(d_im_.p, im, bytes, hipMemcpyHostToDevice, work_));
    QASR_HIP(hipEventRecord(ev_[0], work_));
    dev_wiener(J, iterations);
    QASR_HIP(hipEventRecord(ev_[1], work_));
    QASR_HIP(hipMemcpyAsync(out_re, d_yre_.p, J * bytes, hipMemcpyDeviceToHost, work_));
    QASR_HIP(hipMemcpyAsync(out_im, d_yim_.p, J * bytes, hipMemcpyDeviceToHost, work_));
    QASR_HIP(hipStreamSynchronize(work_));
    timing_ = SepTiming();
    timing_.wiener = elapsed(0, 1);
}

void SepOpenUnmix::istft(const float* re, const float* im, int J, size_t T, size_t length, float* out) {
    check_loaded();
    if (J < 1 || J > SEP_STEMS) throw std::invalid_argument("open-unmix: 1..4 spectra");
    if (length == 0 || (size_t)sep_num_frames(length) != T) throw std::invalid_argument("open-unmix: T must be length / 1024 + 1");
    plan(&length, nullptr, 1);
    ensure_rows(p_.M, false, true);
    ensure_samples(p_.total, J);
    const size_t bytes = (size_t)p_.M * SEP_OUT * sizeof(float);
    QASR_HIP(hipMemcpyAsync(d_yre_.p, re, J * bytes, hipMemcpyHostToDevice, work_));
    QASR_HIP(hipMemcpyAsync(d_yim_.p, im, J * bytes, hipMemcpyHostToDevice, work_));
    QASR_HIP(hipEventRecord(ev_[0], work_));
    dev_istft(J);
    QASR_HIP(hipEventRecord(ev_[1], work_));
    QASR_HIP(hipMemcpyAsync(out, d_audio_.p, (size_t)J * 2 * length * sizeof(float), hipMemcpyDeviceToHost, work_));
    QASR_HIP(hipStreamSynchronize(work_));
    timing_ = SepTiming();
    timing_.istft = elapsed(0, 1);
}

}  // namespace qasr
