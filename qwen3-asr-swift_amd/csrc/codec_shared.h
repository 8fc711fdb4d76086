// codec_shared.h -- what the two directions of the Qwen3-TTS speech tokenizer (codec_qwen3tts.hip, codec_enc_qwen3tts.hip) have in
// common: the geometry, the f32 tile GEMM with its SnakeBeta load and its epilogues, RMSNorm, the depthwise conv + LayerNorm, and the
// packing of the weights both read (host functions in codec_shared.cpp).  xvec_qwen3tts.hip takes Builder and clip_of from here.
// vae_voxcpm.hip (the VoxCPM2 AudioVAE) takes Builder, WindowRows and the tile, with its one epilogue of that model's own, E_RESMAP.
//
// The two models differ in how a pass lays utterances out in rows, so a kernel that reads across rows takes a row locator (WindowRows,
// ClipRows): for an output row it names the input row under the conv's last tap and the first input row the row may read.  Everything
// after that is one body, so both directions keep one summation order (DESIGN.md sections 15, 16): a GEMM output is one thread's fmaf
// chain over k = 0..K-1 (taps outer, channels inner; rows before `first` add exact zeros), a norm's row reduction is a thread's
// sequential partial over c = tid, tid + 256, .. then a fixed tree.
#pragma once
#include "engine.h"
#include "codec_launch.h"
#include "safetensors.h"
#include <algorithm>
#include <string>
#include <vector>

namespace qasr {

constexpr int CODEC_SAMPLES_PER_FRAME = 1920;

struct CodecGeom {                     // SpeechTokenizerDecoderConfig's defaults
    int latent = 1024, decoder_dim = 1536, hidden = 512, heads = 16, head_dim = 64, layers = 8;
    int rates[4] = {8, 5, 4, 3}, ratios[2] = {2, 2};
    int quantizers = 16, semantic_size = 2048, acoustic_size = 2048, codebook_dim = 256;
    float eps = 1e-8f;
    int samples_per_frame() const { return ratios[0] * ratios[1] * rates[0] * rates[1] * rates[2] * rates[3]; }
};
// throws std::invalid_argument "<who>: <the offending field>"
void codec_check_geometry(const CodecGeom& g, const char* who);
// side: "decoder" or "encoder"; q = 0 is rvq_first's codebook
std::string codec_codebook_prefix(const char* side, int q);
// per codebook of model_dir/model.safetensors: stored under `embed` (true) or under embedding_sum + cluster_usage
// (TTSWeightLoading.swift:286-300); throws WeightLoadError with messages starting "<who>: "
std::vector<bool> codec_codebooks_stored(const std::string& model_dir, const char* who, const char* side, int quantizers);

using CodecShapes = std::vector<std::pair<std::string, std::vector<int64_t>>>;
// appends the keys under P = "<side>.pre_transformer."
void codec_pre_transformer_shapes(CodecShapes& s, const std::string& P, const CodecGeom& g);

// ---- weights (host) -----------------------------------------------------------------------------------------------------------------
// offsets are in floats into the one device array a model's weights are packed into
struct CodecGemm { size_t wt = 0, bias = 0; int K = 0, N = 0, Cin = 0, taps = 1; bool has_bias = false; };
struct CodecSnake { size_t a = 0, b = 0; };
struct CodecLayer { size_t n1, n2, ls1, ls2; CodecGemm qkv, o, gu, down; };
struct CodecUnit { CodecSnake s1, s2; CodecGemm c1, c2; };

struct Builder {                       // the host image of that array; every take is padded to 4 floats
    std::vector<float> h;
    const CheckedWeights& w;
    const std::string prefix;          // of every key
    explicit Builder(const CheckedWeights& cw, std::string key_prefix = "") : w(cw), prefix(std::move(key_prefix)) {}
    const std::vector<float>& t(const std::string& k) const { return w.t.at(prefix + k); }
    size_t take(size_t n) { const size_t at = h.size(); h.resize(at + ((n + 3) & ~(size_t)3), 0.0f); return at; }
    size_t vec(const std::string& k) { const auto& v = t(k); const size_t at = take(v.size()); std::copy(v.begin(), v.end(), h.begin() + at); return at; }
};

// Wt[j C_in + c][n] = W[n][c][j] of a conv [out][in][k] (k = 1: a Linear [out][in])
CodecGemm codec_pack_conv(Builder& b, const std::string& key, int Cout, int Cin, int k, bool bias);
// a depthwise or one-channel k = 7 conv [C][1][7] or [1][C][7] -> [7][C]
size_t codec_pack_taps7(Builder& b, const std::string& key, int C);
// exp(alpha) | 1 / exp(beta), in f32 as the reference forms them
CodecSnake codec_pack_snake(Builder& b, const std::string& key);
// codebook [n][D] at b.h[at ..]: `embed`, or embedding_sum / max(cluster_usage, 1e-7)
void codec_pack_codebook(Builder& b, size_t at, const std::string& prefix, bool embed_stored, int n, int D);
// p = "<side>.pre_transformer.layers.<l>."; q | k | v side by side, gate and up interleaved (columns 2 i, 2 i + 1)
CodecLayer codec_pack_layer(Builder& b, const std::string& p, int H, int A);
// MLXNN.RoPE base 10000 over all 64 dimensions: [n][32] (cos, sin) for positions 0 .. n - 1
size_t codec_pack_rope(Builder& b, long n);

// ---- kernels ------------------------------------------------------------------------------------------------------------------------
constexpr int CG_THREADS = 256, CG_T = 64, CG_K = 16, ROW_THREADS = 256;      // the epilogues E_* are in codec_launch.h

// x + (1 / exp(beta)) sin^2(exp(alpha) x) with a = exp(alpha), b = 1 / exp(beta) formed at load (SpeechTokenizerDecoder.swift:105-110)
__device__ __forceinline__ float codec_snake(float x, float a, float b) {
    const float s = sinf(a * x);
    return x + b * (s * s);
}

// sum over the workgroup's 256 values in a fixed tree; every thread gets it.  Ends with a barrier that also frees `red`.
__device__ __forceinline__ float codec_block_sum(float v, float* red, int tid) {
    red[tid] = v;
    __syncthreads();
    for (int s = ROW_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] = red[tid] + red[tid + s];
        __syncthreads();
    }
    const float r = red[0];
    __syncthreads();
    return r;
}

// the clip that owns row m: start[0] = 0 < start[1] < .. < start[n] = rows, every clip holds at least one row
__device__ __forceinline__ int clip_of(const int* __restrict__ start, int n, long m) {
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((long)start[mid] <= m) lo = mid; else hi = mid;
    }
    return lo;
}

// what a causal conv reads for one output row: `last` is the input row under its last tap, `first` the first input row it may read
struct RowSpan { long last, first; };

// the decoder's rows: windows back to back, a window's rows at rate r are r times its frame rows; fstart[frame row] = the window's
// first frame row.  Input and output are at the same rate.
struct WindowRows {
    static constexpr bool BIAS_REPEATS = true;         // a transposed conv's N = s C_out columns share C_out biases: bias[n % bmod]
    static constexpr bool SKIPS = false;               // every row is computed
    const int* fstart;
    int rate;
    __device__ __forceinline__ RowSpan operator()(long m) const { return {m, (long)fstart[m / rate] * rate}; }
};

// WindowRows for windows of which only the tail is kept (streamed chunks behind their left context): kept[frame row] = the window's
// first kept frame row, lead = how many rows at this launch's rate before the first kept one a later launch still reads
// (codec_tail_leads).  A row before live(m) is dead: nothing kept depends on it, a tile of dead rows is not computed and keeps whatever
// an earlier pass left there, which a correct lead never reads.  Rows are located as in WindowRows, so a live row is the same bits.
struct TailRows {
    static constexpr bool BIAS_REPEATS = true;
    static constexpr bool SKIPS = true;
    const int *fstart, *kept;
    int rate, lead;
    __device__ __forceinline__ RowSpan operator()(long m) const { return {m, (long)fstart[m / rate] * rate}; }
    __device__ __forceinline__ long live(long m) const {               // the first live row of m's window, clamped to the window's first row
        const long f = m / rate, a = (long)kept[f] * rate - lead, b = (long)fstart[f] * rate;
        return a > b ? a : b;
    }
};

// the encoder's rows: ostart / istart are the first rows of the clips at the output / input level, output row t of a clip reads input
// row t stride of the same clip.  ostart = nullptr: rows are independent (taps = 1).
struct ClipRows {
    static constexpr bool BIAS_REPEATS = false;        // bias[n]
    static constexpr bool SKIPS = false;
    const int *ostart, *istart;
    int nclips, stride;
    __device__ __forceinline__ RowSpan operator()(long m) const {
        if (!ostart) return {m, 0};
        const int clip = clip_of(ostart, nclips, m);
        const long first = istart[clip];
        return {first + (m - ostart[clip]) * stride, first};
    }
};

// the AudioVAE's strided conv (k = 2 s, stride s): output row m (rate rows per frame) reads input rows (m - 1) s .. (m + 1) s - 1 of its
// own clip
struct VaeStrideRows {
    static constexpr bool BIAS_REPEATS = false;
    static constexpr bool SKIPS = false;
    const int* fstart;
    int rate, stride;
    __device__ __forceinline__ RowSpan operator()(long m) const {
        return {(m + 1) * stride - 1, (long)fstart[m / rate] * rate * stride};
    }
};

// C = epilogue(sum_k A(m, k) Wt[k][n]), k = j C_in + c <-> x[rows(m).last - (taps - 1 - j) dil][c], zero before rows(m).first.
// A [input rows][C_in], Wt [K][N].  bias[n], or bias[n % bmod] where Rows::BIAS_REPEATS (nullptr: none).  E_SWIGLU: columns 2 i,
// 2 i + 1 are gate i, up i; C [M][N / 2].  Rows::SKIPS: tiles of dead rows return at once (block-uniform, before any barrier).
// E_RESMAP: (+ R where given), then the map the one reader of C would apply at its load, snake(v ls[n] + ls[N + n]) with a = sa[n],
// b = sb[n] (ls = nullptr: no affine), so that reader loads plain values (vae_voxcpm.hip).
template <class Rows, bool SNAKE, int EPI>
__global__ __launch_bounds__(CG_THREADS) void codec_gemm_kernel(const float* __restrict__ A, long M, int Cin, int taps, int dil, Rows rows,
                                                                const float* __restrict__ Wt, int K, int N, const float* __restrict__ bias,
                                                                int bmod, const float* __restrict__ sa, const float* __restrict__ sb,
                                                                const float* __restrict__ ls, const float* R, float* C, int ldc) {
    __shared__ __attribute__((aligned(16))) float As[CG_K][CG_T + 4];
    __shared__ __attribute__((aligned(16))) float Bs[CG_K][CG_T];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const long m0 = (long)blockIdx.x * CG_T;
    const int n0 = blockIdx.y * CG_T;
    if constexpr (Rows::SKIPS) {                       // a tile wholly before the live rows of its last row's window, and wholly inside that
        const long ml = (m0 + CG_T < M ? m0 + CG_T : M) - 1;           // window (the end of an earlier window is always live): nothing to do
        if (ml < rows.live(ml) && m0 >= rows(ml).first) return;
    }
    RowSpan span[4];                                   // of each A row this thread loads
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const long m = m0 + ((tid + r * CG_THREADS) >> 4);
        span[r] = m < M ? rows(m) : RowSpan{m, 0};
    }
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[i][q] = 0.0f;
    for (int k0 = 0; k0 < K; k0 += CG_K) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int idx = tid + r * CG_THREADS, row = idx >> 4, kk = idx & 15, k = k0 + kk;
            float v = 0.0f;                            // rows past M, inputs past K and rows before `first` add exact zeros
            if (m0 + row < M && k < K) {
                const int j = k / Cin, c = k - j * Cin;
                const long src = span[r].last - (long)(taps - 1 - j) * dil;
                if (src >= span[r].first) {
                    v = A[src * Cin + c];
                    if (SNAKE) v = codec_snake(v, sa[c], sb[c]);
                }
            }
            As[kk][row] = v;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int idx = tid + r * CG_THREADS, kk = idx >> 6, col = idx & 63, k = k0 + kk, n = n0 + col;
            Bs[kk][col] = (k < K && n < N) ? Wt[(size_t)k * N + n] : 0.0f;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < CG_K; ++kk) {
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
        if (EPI == E_SWIGLU) {                         // silu(gate) * up (SpeechTokenizerDecoder.swift:340)
#pragma unroll
            for (int q = 0; q < 4; q += 2) {
                const int n = n0 + tx * 4 + q;
                if (n + 1 >= N) continue;
                const float g = acc[i][q];
                C[m * ldc + (n >> 1)] = (g / (1.0f + expf(-g))) * acc[i][q + 1];
            }
            continue;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int n = n0 + tx * 4 + q;
            if (n >= N) continue;
            float v = acc[i][q];
            if (bias) v = v + bias[Rows::BIAS_REPEATS ? n % bmod : n];
            if (EPI == E_GELU) v = 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f));
            if (EPI == E_RES) v = v + R[m * ldc + n];
            if (EPI == E_LSRES) v = v * ls[n] + R[m * ldc + n];
            if (EPI == E_RESMAP) {
                if (R) v = v + R[m * ldc + n];
                if (ls) v = v * ls[n] + ls[N + n];
                v = codec_snake(v, sa[n], sb[n]);
            }
            C[m * ldc + n] = v;
        }
    }
}

// y = x / sqrt(mean(x^2) + eps) * w, one workgroup per row.  A template only so that this header can define it: launch codec_rms_kernel<>.
template <class = void>
__global__ __launch_bounds__(ROW_THREADS) void codec_rms_kernel(const float* __restrict__ x, int C, const float* __restrict__ w, float eps,
                                                                float* __restrict__ y) {
    __shared__ float red[ROW_THREADS];
    const long m = blockIdx.x;
    const int tid = threadIdx.x;
    float p = 0.0f;
    for (int c = tid; c < C; c += ROW_THREADS) { const float v = x[m * C + c]; p = p + v * v; }
    const float inv = 1.0f / sqrtf(codec_block_sum(p, red, tid) / (float)C + eps);
    for (int c = tid; c < C; c += ROW_THREADS) y[m * C + c] = (x[m * C + c] * inv) * w[c];
}

// depthwise causal conv k = 7 (w [7][C], + bias) then LayerNorm eps 1e-5, one workgroup per row; C <= 4096
// (SpeechTokenizerDecoder.swift:156-160).  Input and output rows are the same: only rows(m).first is used.
template <class Rows>
__global__ __launch_bounds__(ROW_THREADS) void codec_dwln_kernel(const float* __restrict__ x, int C, Rows rows, const float* __restrict__ w,
                                                                 const float* __restrict__ b, const float* __restrict__ lnw,
                                                                 const float* __restrict__ lnb, float* __restrict__ y) {
    __shared__ float red[ROW_THREADS];
    __shared__ float val[4096];
    const long m = blockIdx.x, first = rows(m).first;
    const int tid = threadIdx.x;
    float p = 0.0f;
    for (int c = tid; c < C; c += ROW_THREADS) {
        float acc = 0.0f;
#pragma unroll
        for (int j = 0; j < 7; ++j) {
            const long src = m - (6 - j);
            if (src >= first) acc = acc + x[src * C + c] * w[j * C + c];
        }
        acc = acc + b[c];
        val[c] = acc;
        p = p + acc;
    }
    const float mu = codec_block_sum(p, red, tid) / (float)C;
    float q = 0.0f;
    for (int c = tid; c < C; c += ROW_THREADS) { const float d = val[c] - mu; q = q + d * d; }
    const float inv = 1.0f / sqrtf(codec_block_sum(q, red, tid) / (float)C + 1e-5f);
    for (int c = tid; c < C; c += ROW_THREADS) y[m * C + c] = ((val[c] - mu) * inv) * lnw[c] + lnb[c];
}

}  // namespace qasr
