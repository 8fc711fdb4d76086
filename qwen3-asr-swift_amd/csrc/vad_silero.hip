// vad_silero.hip -- Silero VAD v5 for gfx950 (vad_silero.h).  f32 throughout, accurate expf / tanhf / sqrtf.
//
// Two launches per call, because only the LSTM recurrence is sequential:
//   vad_front_kernel  parallel over chunks (CPW chunks of any rows per workgroup): padded input -> STFT magnitudes -> four convolutions
//                     with ReLU -> LSTM input projection x Wx^T + bias: 512 pre-gates per chunk to HBM.  Every weight is read once per
//                     workgroup (coalesced, k-major device layouts) and used for all of its chunks; activations live in LDS.
//   vad_recur_kernel  one workgroup per row (1024 threads), steps t = 0 .. n_chunks - 1: gates = pre[t] + h Wh^T, cell update,
//                     prob[t] = sigmoid(w_d . relu(h) + b_d).  Wh stays in VGPRs (thread = gate row x half of h: 64 floats), h is
//                     broadcast through LDS; two barriers per step.  At the end the row's h, c and 64-sample context go to its slot.
// Summation order (the bit-identity argument): every output is ONE thread's sequential fmaf chain in an order fixed
// by the layer (STFT: k = 0..255; conv: tap, then input channel, padded taps skipped; Wx: input 0..127; then + bias), and the recurrent
// dot is two fixed 64-term halves (four interleaved partial sums each, combined in a fixed tree) added as lo + hi.  Which workgroup,
// which slot of it, how many chunks it holds, the batch size and the grid size never enter the arithmetic, so a stream fed tick by tick
// and the same audio fed as one buffer give bit-identical probabilities and state.  No workgroup waits for another.
#include "vad_silero.h"
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>

namespace qasr {

// device weight block (floats; every offset a multiple of 4)
constexpr int W_STFT = 0;                              // [256 k][258 co]
constexpr int W_E1 = W_STFT + 256 * 258;               // [3][129 ci][128 co]
constexpr int B_E1 = W_E1 + 3 * 129 * 128;
constexpr int W_E2 = B_E1 + 128;                       // [3][128][64]
constexpr int B_E2 = W_E2 + 3 * 128 * 64;
constexpr int W_E3 = B_E2 + 64;                        // [3][64][64]
constexpr int B_E3 = W_E3 + 3 * 64 * 64;
constexpr int W_E4 = B_E3 + 64;                        // [3][64][128]
constexpr int B_E4 = W_E4 + 3 * 64 * 128;
constexpr int W_X = B_E4 + 128;                        // [128 in][512 gate]
constexpr int B_X = W_X + 128 * 512;
constexpr int W_HH = B_X + 512;                        // [512 gate][128 h] (reference layout)
constexpr int W_D = W_HH + 512 * 128;                  // [128]
constexpr int W_TOTAL = W_D + 128;
static_assert(W_E1 % 4 == 0 && W_HH % 4 == 0 && W_X % 4 == 0, "alignment");

struct VadMeta {
    const long* pcm_off;       // [rows]
    const int* n;              // samples of the row
    const int* base;           // first chunk of the row (pre / prob index)
    const int* n_chunks;
    const int* sid;            // stream slot
    const int* zero;           // 1: start from the zero state (resetState), 0: from the slot
    const int* chunk_row;      // [chunks]
};

__device__ __forceinline__ float vad_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

constexpr int FR_THREADS = 256;
constexpr int X_LEN = 640, ST_LEN = 4 * 258, MG_LEN = 129 * 4;

template <int CPW>
__global__ __launch_bounds__(FR_THREADS) void vad_front_kernel(const float* __restrict__ W, const float* __restrict__ pcm,
                                                               const float* __restrict__ st_ctx, VadMeta meta, int total,
                                                               float* __restrict__ pre) {
    extern __shared__ float lds[];
    float* xs = lds;                                   // [CPW][640]            later e2 [CPW][64][2]
    float* st = xs + CPW * X_LEN;                      // [CPW][4][258]         later e1 [CPW][128][4], e4 [CPW][128]
    float* mg = st + CPW * ST_LEN;                     // [CPW][129][4]         later e3 [CPW][64]
    const int tid = threadIdx.x;
    const int q0 = blockIdx.x * CPW;

    // ---- 640-sample padded input (SileroVAD.swift processChunk: context ++ chunk; SileroModel.swift reflectionPadRight: x[576 + m] = x[574 - m])
    for (int idx = tid; idx < CPW * X_LEN; idx += FR_THREADS) {
        const int j = idx / X_LEN, i = idx - j * X_LEN, q = q0 + j;
        float v = 0.0f;
        if (q < total) {
            const int row = meta.chunk_row[q];
            const int c = q - meta.base[row], n = meta.n[row];
            const float* src = pcm + meta.pcm_off[row];
            if (i < VAD_CTX) {
                if (c > 0) v = src[c * VAD_CHUNK - VAD_CTX + i];          // previous chunk of the row: always whole
                else if (!meta.zero[row]) v = st_ctx[(long)meta.sid[row] * VAD_CTX + i];
            } else {
                const int s = i < 576 ? i - VAD_CTX : 1086 - i;            // 1086 - i = (1150 - i) - 64
                const int g = c * VAD_CHUNK + s;
                if (g < n) v = src[g];                                      // detectSpeech zero-pads the last chunk
            }
        }
        xs[idx] = v;
    }
    __syncthreads();

    // ---- STFT conv: st[j][f][co] = sum_k W[co][k] x[128 f + k], k = 0..255 in order
    {
        const int co = tid;
        float acc[CPW][4];
#pragma unroll
        for (int j = 0; j < CPW; ++j)
#pragma unroll
            for (int f = 0; f < 4; ++f) acc[j][f] = 0.0f;
        for (int k = 0; k < 256; k += 4) {
            const float w0 = W[W_STFT + (k + 0) * 258 + co], w1 = W[W_STFT + (k + 1) * 258 + co];
            const float w2 = W[W_STFT + (k + 2) * 258 + co], w3 = W[W_STFT + (k + 3) * 258 + co];
#pragma unroll
            for (int j = 0; j < CPW; ++j)
#pragma unroll
                for (int f = 0; f < 4; ++f) {
                    const float4 x = lds_read_f4(&xs[j * X_LEN + f * 128 + k]);
                    float a = acc[j][f];
                    a = fmaf(w0, x.x, a); a = fmaf(w1, x.y, a); a = fmaf(w2, x.z, a); a = fmaf(w3, x.w, a);
                    acc[j][f] = a;
                }
        }
#pragma unroll
        for (int j = 0; j < CPW; ++j)
#pragma unroll
            for (int f = 0; f < 4; ++f) st[j * ST_LEN + f * 258 + co] = acc[j][f];
        // channels 256 and 257 (imaginary parts of bins 127, 128): one (channel, chunk) item per thread of the last wave's tail
        const int item = tid - (FR_THREADS - 2 * CPW);
        if (item >= 0) {
            const int c2 = 256 + (item & 1), j = item >> 1;
            float a2[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            for (int k = 0; k < 256; k += 4) {
                const float w0 = W[W_STFT + (k + 0) * 258 + c2], w1 = W[W_STFT + (k + 1) * 258 + c2];
                const float w2 = W[W_STFT + (k + 2) * 258 + c2], w3 = W[W_STFT + (k + 3) * 258 + c2];
#pragma unroll
                for (int f = 0; f < 4; ++f) {
                    const float4 x = lds_read_f4(&xs[j * X_LEN + f * 128 + k]);
                    float a = a2[f];
                    a = fmaf(w0, x.x, a); a = fmaf(w1, x.y, a); a = fmaf(w2, x.z, a); a = fmaf(w3, x.w, a);
                    a2[f] = a;
                }
            }
#pragma unroll
            for (int f = 0; f < 4; ++f) st[j * ST_LEN + f * 258 + c2] = a2[f];
        }
    }
    __syncthreads();

    // ---- magnitude sqrt(re^2 + im^2) -> mg[j][bin][f]
    for (int idx = tid; idx < CPW * 4 * 129; idx += FR_THREADS) {
        const int j = idx / (4 * 129), r = idx - j * 4 * 129, f = r / 129, b = r - f * 129;
        const float re = st[j * ST_LEN + f * 258 + b], im = st[j * ST_LEN + f * 258 + 129 + b];
        mg[j * MG_LEN + b * 4 + f] = sqrtf(re * re + im * im);
    }
    __syncthreads();

    // ---- encoder.0: 129 -> 128, k3 s1 p1, 4 frames -> e1[j][co][f] (in st)
    constexpr int NJ1 = (CPW + 1) / 2, NJ2 = (CPW + 3) / 4;
    float* e1 = st;
    {
        const int co = tid & 127, grp = tid >> 7;
        float acc[NJ1][4];
#pragma unroll
        for (int m = 0; m < NJ1; ++m)
#pragma unroll
            for (int f = 0; f < 4; ++f) acc[m][f] = 0.0f;
#pragma unroll
        for (int k = 0; k < 3; ++k)
            for (int ci = 0; ci < 129; ++ci) {
                const float w = W[W_E1 + (k * 129 + ci) * 128 + co];
#pragma unroll
                for (int m = 0; m < NJ1; ++m) {
                    const int j = grp + 2 * m;
                    if (j < CPW) {
                        const float4 v = lds_read_f4(&mg[j * MG_LEN + ci * 4]);
                        const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                        for (int f = 0; f < 4; ++f) {
                            const int fi = f + k - 1;
                            if (fi >= 0 && fi < 4) acc[m][f] = fmaf(w, vv[fi], acc[m][f]);
                        }
                    }
                }
            }
        const float b = W[B_E1 + co];                  // st (the STFT output) was last read by the magnitude pass: e1 may overwrite it
#pragma unroll
        for (int m = 0; m < NJ1; ++m) {
            const int j = grp + 2 * m;
            if (j < CPW)
#pragma unroll
                for (int f = 0; f < 4; ++f) e1[j * 512 + co * 4 + f] = fmaxf(acc[m][f] + b, 0.0f);
        }
    }
    __syncthreads();

    // ---- encoder.1: 128 -> 64, k3 s2 p1, 4 -> 2 frames -> e2[j][co][f] (in xs)
    float* e2 = xs;
    {
        const int co = tid & 63, grp = tid >> 6;
        float acc[NJ2][2];
#pragma unroll
        for (int m = 0; m < NJ2; ++m) acc[m][0] = acc[m][1] = 0.0f;
#pragma unroll
        for (int k = 0; k < 3; ++k)
            for (int ci = 0; ci < 128; ++ci) {
                const float w = W[W_E2 + (k * 128 + ci) * 64 + co];
#pragma unroll
                for (int m = 0; m < NJ2; ++m) {
                    const int j = grp + 4 * m;
                    if (j < CPW) {
                        const float4 v = lds_read_f4(&e1[j * 512 + ci * 4]);
                        const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                        for (int f = 0; f < 2; ++f) {
                            const int fi = 2 * f + k - 1;
                            if (fi >= 0 && fi < 4) acc[m][f] = fmaf(w, vv[fi], acc[m][f]);
                        }
                    }
                }
            }
        const float b = W[B_E2 + co];
#pragma unroll
        for (int m = 0; m < NJ2; ++m) {
            const int j = grp + 4 * m;
            if (j < CPW) { e2[j * 128 + co * 2] = fmaxf(acc[m][0] + b, 0.0f); e2[j * 128 + co * 2 + 1] = fmaxf(acc[m][1] + b, 0.0f); }
        }
    }
    __syncthreads();

    // ---- encoder.2: 64 -> 64, k3 s2 p1, 2 -> 1 frame (taps 1, 2 see frames 0, 1) -> e3[j][co] (in mg)
    float* e3 = mg;
    {
        const int co = tid & 63, grp = tid >> 6;
        float acc[NJ2];
#pragma unroll
        for (int m = 0; m < NJ2; ++m) acc[m] = 0.0f;
#pragma unroll
        for (int k = 1; k < 3; ++k)
            for (int ci = 0; ci < 64; ++ci) {
                const float w = W[W_E3 + (k * 64 + ci) * 64 + co];
#pragma unroll
                for (int m = 0; m < NJ2; ++m) {
                    const int j = grp + 4 * m;
                    if (j < CPW) acc[m] = fmaf(w, e2[j * 128 + ci * 2 + (k - 1)], acc[m]);
                }
            }
        const float b = W[B_E3 + co];
#pragma unroll
        for (int m = 0; m < NJ2; ++m) {
            const int j = grp + 4 * m;
            if (j < CPW) e3[j * 64 + co] = fmaxf(acc[m] + b, 0.0f);
        }
    }
    __syncthreads();

    // ---- encoder.3: 64 -> 128, k3 s1 p1 on one frame (only the centre tap sees data) -> e4[j][co] (in st)
    float* e4 = st;
    {
        const int co = tid & 127, grp = tid >> 7;
        float acc[NJ1];
#pragma unroll
        for (int m = 0; m < NJ1; ++m) acc[m] = 0.0f;
        for (int ci = 0; ci < 64; ++ci) {
            const float w = W[W_E4 + (64 + ci) * 128 + co];
#pragma unroll
            for (int m = 0; m < NJ1; ++m) {
                const int j = grp + 2 * m;
                if (j < CPW) acc[m] = fmaf(w, e3[j * 64 + ci], acc[m]);
            }
        }
        const float b = W[B_E4 + co];
#pragma unroll
        for (int m = 0; m < NJ1; ++m) {
            const int j = grp + 2 * m;
            if (j < CPW) e4[j * 128 + co] = fmaxf(acc[m] + b, 0.0f);
        }
    }
    __syncthreads();

    // ---- LSTM input projection: pre[q][g] = sum_i x[i] Wx[g][i] (i = 0..127) + bias[g]   (SileroModel.swift lstmForward addMM)
    {
        float acc[CPW][2];
#pragma unroll
        for (int j = 0; j < CPW; ++j) acc[j][0] = acc[j][1] = 0.0f;
        for (int i = 0; i < 128; ++i) {
            const float w0 = W[W_X + i * 512 + tid], w1 = W[W_X + i * 512 + 256 + tid];
#pragma unroll
            for (int j = 0; j < CPW; ++j) {
                const float x = e4[j * 128 + i];
                acc[j][0] = fmaf(w0, x, acc[j][0]);
                acc[j][1] = fmaf(w1, x, acc[j][1]);
            }
        }
        const float b0 = W[B_X + tid], b1 = W[B_X + 256 + tid];
#pragma unroll
        for (int j = 0; j < CPW; ++j) {
            const int q = q0 + j;
            if (q < total) {
                pre[(long)q * VAD_G + tid] = acc[j][0] + b0;
                pre[(long)q * VAD_G + 256 + tid] = acc[j][1] + b1;
            }
        }
    }
}

constexpr int RC_THREADS = 1024;

__global__ __launch_bounds__(RC_THREADS) void vad_recur_kernel(const float* __restrict__ W, const float* __restrict__ pre,
                                                               const float* __restrict__ pcm, VadMeta meta, float dec_b,
                                                               float* __restrict__ prob, float* __restrict__ st_h,
                                                               float* __restrict__ st_c, float* __restrict__ st_ctx) {
    __shared__ float s_h[VAD_H];
    __shared__ float s_gate[VAD_G];
    __shared__ float s_dec[2][2];
    const int row = blockIdx.x, tid = threadIdx.x;
    const int g = tid >> 1, half = tid & 1;
    const int nc = meta.n_chunks[row], base = meta.base[row], sid = meta.sid[row], zero = meta.zero[row];

    float w[64];                                       // Wh[g][64 half .. 64 half + 63]
#pragma unroll
    for (int k = 0; k < 64; k += 4) {
        const float4 v = *reinterpret_cast<const float4*>(&W[W_HH + g * VAD_H + half * 64 + k]);
        w[k] = v.x; w[k + 1] = v.y; w[k + 2] = v.z; w[k + 3] = v.w;
    }
    float h = 0.0f, c = 0.0f;
    if (tid < VAD_H) {
        if (!zero) { h = st_h[(long)sid * VAD_H + tid]; c = st_c[(long)sid * VAD_H + tid]; }
        s_h[tid] = h;
    }
    const float wd = tid < VAD_H ? W[W_D + tid] : 0.0f;
    __syncthreads();

    float pnext = (nc > 0 && half == 0) ? pre[(long)base * VAD_G + g] : 0.0f;
    for (int t = 0; t < nc; ++t) {
        const float pcur = pnext;
        if (half == 0 && t + 1 < nc) pnext = pre[(long)(base + t + 1) * VAD_G + g];
        // h Wh^T: this thread's 64-term half, four interleaved partial sums
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
        if (tid < VAD_H) {                             // i, f, g, o (SileroModel.swift lstmForward split order)
            const float ig = vad_sigmoid(s_gate[tid]), fg = vad_sigmoid(s_gate[VAD_H + tid]);
            const float gg = tanhf(s_gate[2 * VAD_H + tid]), og = vad_sigmoid(s_gate[3 * VAD_H + tid]);
            c = fg * c + ig * gg;
            h = og * tanhf(c);
            s_h[tid] = h;
            const float d = lane_sum<64>(fmaxf(h, 0.0f) * wd);
            if ((tid & 63) == 0) s_dec[t & 1][tid >> 6] = d;
        }
        __syncthreads();
        if (tid == 0) prob[base + t] = vad_sigmoid((s_dec[t & 1][0] + s_dec[t & 1][1]) + dec_b);
    }
    // the row's stream keeps h, c and the last 64 samples of its last (zero-padded) chunk; an empty row only resets (zero = 1)
    if (nc > 0 || zero) {
        if (tid < VAD_H) { st_h[(long)sid * VAD_H + tid] = h; st_c[(long)sid * VAD_H + tid] = c; }
        if (tid < VAD_CTX) {
            float v = 0.0f;
            if (nc > 0) {
                const long gi = (long)nc * VAD_CHUNK - VAD_CTX + tid;
                if (gi < meta.n[row]) v = pcm[meta.pcm_off[row] + gi];
            }
            st_ctx[(long)sid * VAD_CTX + tid] = v;
        }
    }
}

// ---- weights ------------------------------------------------------------------------------------------------------------
const std::vector<std::pair<std::string, std::vector<int64_t>>>& silero_tensor_shapes() {
    static const std::vector<std::pair<std::string, std::vector<int64_t>>> s = {
        {"stft.weight", {258, 256, 1}},
        {"encoder.0.weight", {128, 3, 129}}, {"encoder.0.bias", {128}},
        {"encoder.1.weight", {64, 3, 128}}, {"encoder.1.bias", {64}},
        {"encoder.2.weight", {64, 3, 64}}, {"encoder.2.bias", {64}},
        {"encoder.3.weight", {128, 3, 64}}, {"encoder.3.bias", {128}},
        {"lstm.Wx", {512, 128}}, {"lstm.Wh", {512, 128}}, {"lstm.bias", {512}},
        {"decoder.weight", {1, 1, 128}}, {"decoder.bias", {1}},
    };
    return s;
}

// ---- binarize (VADPipeline.swift:117-181 with SileroVAD.swift detectSpeech's frame duration) ---------------------------------------
std::vector<VadSegment> silero_binarize(const float* probs, size_t n, const VadConfig& cfg) {
    std::vector<VadSegment> segs;
    if (n == 0) return segs;
    const float chunk = (float)VAD_CHUNK / (float)VAD_RATE;
    const float window = (float)n * chunk;
    const float frame = window / (float)n;
    bool in = false;
    float start = 0.0f;
    for (size_t i = 0; i < n; ++i) {
        const float time = (float)i * frame;
        if (!in && probs[i] >= cfg.onset) { in = true; start = time; }
        else if (in && probs[i] < cfg.offset) { in = false; segs.push_back({start, time}); }
    }
    if (in) segs.push_back({start, (float)n * frame});
    std::vector<VadSegment> kept;                              // filterDurations
    for (const auto& s : segs) if (s.end - s.start >= cfg.min_speech) kept.push_back(s);
    std::vector<VadSegment> merged;
    if (kept.empty()) return merged;
    VadSegment cur = kept[0];
    for (size_t i = 1; i < kept.size(); ++i) {
        if (kept[i].start - cur.end < cfg.min_silence) cur.end = kept[i].end;
        else { merged.push_back(cur); cur = kept[i]; }
    }
    merged.push_back(cur);
    return merged;
}

// ---- host object --------------------------------------------------------------------------------------------------------
constexpr int FR_CPW_BIG = 8;

static size_t front_lds(int cpw) { return (size_t)cpw * (X_LEN + ST_LEN + MG_LEN) * sizeof(float); }

SileroVad::SileroVad(int device, const CheckedWeights& w, int max_streams, hipStream_t work)
    : device_(device), max_streams_(max_streams) {
    if (max_streams <= 0 || max_streams > 4096) throw std::invalid_argument("silero vad: max_streams in 1..4096");
    // device layouts: conv weights [out, k, in] -> [k, in, out], STFT [258, 256, 1] -> [256, 258], Wx [512, 128] -> [128, 512]
    std::vector<float> h(W_TOTAL, 0.0f);
    const auto& stft = w.t.at("stft.weight");
    for (int co = 0; co < 258; ++co)
        for (int k = 0; k < 256; ++k) h[W_STFT + k * 258 + co] = stft[co * 256 + k];
    const int wo[4] = {W_E1, W_E2, W_E3, W_E4}, bo[4] = {B_E1, B_E2, B_E3, B_E4};
    const int cout[4] = {128, 64, 64, 128}, cin[4] = {129, 128, 64, 64};
    for (int l = 0; l < 4; ++l) {
        const auto& wt = w.t.at("encoder." + std::to_string(l) + ".weight");
        const auto& bt = w.t.at("encoder." + std::to_string(l) + ".bias");
        for (int o = 0; o < cout[l]; ++o) {
            for (int k = 0; k < 3; ++k)
                for (int i = 0; i < cin[l]; ++i) h[wo[l] + (k * cin[l] + i) * cout[l] + o] = wt[((size_t)o * 3 + k) * cin[l] + i];
            h[bo[l] + o] = bt[o];
        }
    }
    const auto &wx = w.t.at("lstm.Wx"), &wh = w.t.at("lstm.Wh"), &bx = w.t.at("lstm.bias");
    for (int g = 0; g < VAD_G; ++g) {
        for (int i = 0; i < VAD_H; ++i) { h[W_X + i * VAD_G + g] = wx[g * VAD_H + i]; h[W_HH + g * VAD_H + i] = wh[g * VAD_H + i]; }
        h[B_X + g] = bx[g];
    }
    for (int i = 0; i < VAD_H; ++i) h[W_D + i] = w.t.at("decoder.weight")[i];
    dec_b_ = w.t.at("decoder.bias")[0];

    QASR_HIP(hipSetDevice(device_));
    QASR_HIP(hipStreamCreateWithFlags(&own_, hipStreamNonBlocking));
    work_ = work ? work : own_;
    for (auto& e : ev_) QASR_HIP(hipEventCreate(&e));
    d_w_.alloc((size_t)W_TOTAL * sizeof(float));
    QASR_HIP(hipMemcpy(d_w_.p, h.data(), (size_t)W_TOTAL * sizeof(float), hipMemcpyHostToDevice));
    const size_t S = (size_t)max_streams_;
    d_h_.alloc(S * VAD_H * sizeof(float));
    d_c_.alloc(S * VAD_H * sizeof(float));
    d_ctx_.alloc(S * VAD_CTX * sizeof(float));
    QASR_HIP(hipMemset(d_h_.p, 0, d_h_.bytes));
    QASR_HIP(hipMemset(d_c_.p, 0, d_c_.bytes));
    QASR_HIP(hipMemset(d_ctx_.p, 0, d_ctx_.bytes));
    ensure(S, S * VAD_CHUNK, S);                       // a tick of every stream never reallocates (its graphs stay valid)
    ensure_dynamic_lds(reinterpret_cast<const void*>(&vad_front_kernel<FR_CPW_BIG>), (int)front_lds(FR_CPW_BIG));
    ensure_dynamic_lds(reinterpret_cast<const void*>(&vad_front_kernel<1>), (int)front_lds(1));
}

SileroVad::~SileroVad() {
    if (work_) (void)hipStreamSynchronize(work_);
    drop_graphs();
    for (auto& e : ev_) if (e) (void)hipEventDestroy(e);
    if (own_) (void)hipStreamDestroy(own_);
}

void SileroVad::drop_graphs() {
    for (auto& kv : graphs_) (void)hipGraphExecDestroy(kv.second);
    graphs_.clear();
}

// meta block: long pcm_off[cap_rows] | int n, base, n_chunks, sid, zero [cap_rows each] | int chunk_row[cap_chunks]
static size_t meta_bytes(size_t rows, size_t chunks) { return rows * (sizeof(long) + 5 * sizeof(int)) + chunks * sizeof(int); }

void SileroVad::ensure(size_t B, size_t samples, size_t chunks) {
    if (B <= cap_rows_ && samples <= cap_samples_ && chunks <= cap_chunks_) return;
    QASR_HIP(hipStreamSynchronize(work_));
    drop_graphs();
    cap_rows_ = std::max(cap_rows_, B);
    cap_samples_ = std::max(cap_samples_, samples);
    cap_chunks_ = std::max(cap_chunks_, chunks);
    h_pcm_.alloc(cap_samples_ * sizeof(float));
    d_pcm_.alloc(cap_samples_ * sizeof(float));
    h_meta_.alloc(meta_bytes(cap_rows_, cap_chunks_));
    d_meta_.alloc(meta_bytes(cap_rows_, cap_chunks_));
    d_pre_.alloc(cap_chunks_ * VAD_G * sizeof(float));
    d_prob_.alloc(cap_chunks_ * sizeof(float));
    h_prob_.alloc(cap_chunks_ * sizeof(float));
}

static VadMeta meta_ptrs(char* base, size_t rows) {
    VadMeta m;
    m.pcm_off = reinterpret_cast<const long*>(base);
    const int* p = reinterpret_cast<const int*>(base + rows * sizeof(long));
    m.n = p; m.base = p + rows; m.n_chunks = p + 2 * rows; m.sid = p + 3 * rows; m.zero = p + 4 * rows; m.chunk_row = p + 5 * rows;
    return m;
}

// everything of one call that touches the device, in stream order: meta + PCM up, two kernels, probabilities down
void SileroVad::issue(int B, int total_chunks, size_t samples, hipStream_t s) {
    QASR_HIP(hipMemcpyAsync(d_meta_.p, h_meta_.p, meta_bytes(cap_rows_, (size_t)total_chunks), hipMemcpyHostToDevice, s));
    if (samples) QASR_HIP(hipMemcpyAsync(d_pcm_.p, h_pcm_.p, samples * sizeof(float), hipMemcpyHostToDevice, s));
    const VadMeta m = meta_ptrs(d_meta_.as<char>(), cap_rows_);
    if (total_chunks > 0) {
        // eight chunks per workgroup once there are enough chunks to fill the GPU that way; ticks of few streams: one per workgroup
        if (total_chunks >= 256 * FR_CPW_BIG / 2)
            hipLaunchKernelGGL(vad_front_kernel<FR_CPW_BIG>, dim3(cdiv(total_chunks, FR_CPW_BIG)), dim3(FR_THREADS), front_lds(FR_CPW_BIG), s,
                               d_w_.as<float>(), d_pcm_.as<float>(), d_ctx_.as<float>(), m, total_chunks, d_pre_.as<float>());
        else
            hipLaunchKernelGGL(vad_front_kernel<1>, dim3(total_chunks), dim3(FR_THREADS), front_lds(1), s, d_w_.as<float>(), d_pcm_.as<float>(),
                               d_ctx_.as<float>(), m, total_chunks, d_pre_.as<float>());
    }
    hipLaunchKernelGGL(vad_recur_kernel, dim3(B), dim3(RC_THREADS), 0, s, d_w_.as<float>(), d_pre_.as<float>(), d_pcm_.as<float>(), m, dec_b_,
                       d_prob_.as<float>(), d_h_.as<float>(), d_c_.as<float>(), d_ctx_.as<float>());
    if (total_chunks > 0)
        QASR_HIP(hipMemcpyAsync(h_prob_.p, d_prob_.p, (size_t)total_chunks * sizeof(float), hipMemcpyDeviceToHost, s));
}

void SileroVad::run(int B, int total_chunks, size_t samples, bool tick) {
    QASR_HIP(hipSetDevice(device_));
    QASR_HIP(hipEventRecord(ev_[0], work_));
    last_graph_ = false;
    if (tick) {
        // a tick of B streams: same addresses, sizes and launches every time, only the staged samples / stream ids differ -> one graph per B
        auto it = graphs_.find(B);
        if (it == graphs_.end()) it = graphs_.emplace(B, capture_graph(own_, [&] { issue(B, total_chunks, samples, own_); })).first;
        QASR_HIP(hipGraphLaunch(it->second, work_));
        last_graph_ = true;
    } else {
        issue(B, total_chunks, samples, work_);
    }
    QASR_HIP(hipEventRecord(ev_[1], work_));
    QASR_HIP(hipStreamSynchronize(work_));
    QASR_HIP(hipGetLastError());
    QASR_HIP(hipEventElapsedTime(&last_ms_, ev_[0], ev_[1]));
}

void SileroVad::reset(int stream) {
    if (stream >= max_streams_) throw std::invalid_argument("silero vad: stream outside [0, max_streams)");
    QASR_HIP(hipSetDevice(device_));
    const size_t off = stream < 0 ? 0 : (size_t)stream, cnt = stream < 0 ? (size_t)max_streams_ : 1;
    QASR_HIP(hipMemsetAsync(d_h_.as<float>() + off * VAD_H, 0, cnt * VAD_H * sizeof(float), work_));
    QASR_HIP(hipMemsetAsync(d_c_.as<float>() + off * VAD_H, 0, cnt * VAD_H * sizeof(float), work_));
    QASR_HIP(hipMemsetAsync(d_ctx_.as<float>() + off * VAD_CTX, 0, cnt * VAD_CTX * sizeof(float), work_));
    QASR_HIP(hipStreamSynchronize(work_));
}

static void check_ids(const int32_t* ids, size_t B, int max_streams) {
    if (B > (size_t)max_streams) throw std::length_error("silero vad: more rows than max_streams");
    std::vector<char> seen((size_t)max_streams, 0);
    for (size_t b = 0; b < B; ++b) {
        const int s = ids ? ids[b] : (int)b;
        if (s < 0 || s >= max_streams) throw std::invalid_argument("silero vad: stream id outside [0, max_streams)");
        if (seen[(size_t)s]) throw std::invalid_argument("silero vad: a stream appears twice in one call (its chunks are sequential)");
        seen[(size_t)s] = 1;
    }
}

void SileroVad::process(const float* chunks, const int32_t* stream_ids, size_t B, float* probs) {
    if (B == 0) return;
    check_ids(stream_ids, B, max_streams_);
    const VadMeta m = meta_ptrs(h_meta_.as<char>(), cap_rows_);
    long* off = const_cast<long*>(m.pcm_off);
    int *n = const_cast<int*>(m.n), *base = const_cast<int*>(m.base), *nc = const_cast<int*>(m.n_chunks);
    int *sid = const_cast<int*>(m.sid), *zero = const_cast<int*>(m.zero), *crow = const_cast<int*>(m.chunk_row);
    for (size_t b = 0; b < B; ++b) {
        off[b] = (long)b * VAD_CHUNK; n[b] = VAD_CHUNK; base[b] = (int)b; nc[b] = 1;
        sid[b] = stream_ids ? stream_ids[b] : (int)b; zero[b] = 0; crow[b] = (int)b;
    }
    std::memcpy(h_pcm_.p, chunks, B * VAD_CHUNK * sizeof(float));
    run((int)B, (int)B, B * VAD_CHUNK, true);
    std::memcpy(probs, h_prob_.p, B * sizeof(float));
}

void SileroVad::probs(const float* const* pcm, const size_t* n, size_t B, const int32_t* stream_ids, float* probs, size_t stride,
                      int32_t* n_chunks) {
    if (B == 0) return;
    check_ids(stream_ids, B, max_streams_);
    size_t samples = 0, chunks = 0, maxc = 0;
    for (size_t b = 0; b < B; ++b) {
        if (n[b] && !pcm[b]) throw std::invalid_argument("silero vad: null buffer");
        if (n[b] > (size_t)1 << 30) throw std::length_error("silero vad: buffer longer than 2^30 samples");
        const size_t c = (n[b] + VAD_CHUNK - 1) / VAD_CHUNK;
        samples += n[b]; chunks += c; maxc = std::max(maxc, c);
    }
    if (stride < maxc) throw std::invalid_argument("silero vad: stride smaller than the longest row's chunk count");
    if (chunks > (size_t)1 << 30) throw std::length_error("silero vad: too many chunks in one call");
    ensure(B, samples, chunks);
    const VadMeta m = meta_ptrs(h_meta_.as<char>(), cap_rows_);
    long* off = const_cast<long*>(m.pcm_off);
    int *nn = const_cast<int*>(m.n), *base = const_cast<int*>(m.base), *nc = const_cast<int*>(m.n_chunks);
    int *sid = const_cast<int*>(m.sid), *zero = const_cast<int*>(m.zero), *crow = const_cast<int*>(m.chunk_row);
    size_t so = 0, co = 0;
    for (size_t b = 0; b < B; ++b) {
        const size_t c = (n[b] + VAD_CHUNK - 1) / VAD_CHUNK;
        off[b] = (long)so; nn[b] = (int)n[b]; base[b] = (int)co; nc[b] = (int)c;
        sid[b] = stream_ids ? stream_ids[b] : (int)b; zero[b] = 1;
        for (size_t i = 0; i < c; ++i) crow[co + i] = (int)b;
        if (n[b]) std::memcpy(h_pcm_.as<float>() + so, pcm[b], n[b] * sizeof(float));
        so += n[b]; co += c;
        if (n_chunks) n_chunks[b] = (int32_t)c;
    }
    run((int)B, (int)chunks, samples, false);
    for (size_t b = 0; b < B; ++b) {
        float* dst = probs + b * stride;
        std::memcpy(dst, h_prob_.as<float>() + base[b], (size_t)nc[b] * sizeof(float));
        std::fill(dst + nc[b], dst + stride, 0.0f);
    }
}

void SileroVad::state(int stream, float* h, float* c, float* ctx) {
    if (stream < 0 || stream >= max_streams_) throw std::invalid_argument("silero vad: stream outside [0, max_streams)");
    QASR_HIP(hipSetDevice(device_));
    QASR_HIP(hipStreamSynchronize(work_));
    if (h) QASR_HIP(hipMemcpy(h, d_h_.as<float>() + (size_t)stream * VAD_H, VAD_H * sizeof(float), hipMemcpyDeviceToHost));
    if (c) QASR_HIP(hipMemcpy(c, d_c_.as<float>() + (size_t)stream * VAD_H, VAD_H * sizeof(float), hipMemcpyDeviceToHost));
    if (ctx) QASR_HIP(hipMemcpy(ctx, d_ctx_.as<float>() + (size_t)stream * VAD_CTX, VAD_CTX * sizeof(float), hipMemcpyDeviceToHost));
}

}  // namespace qasr
