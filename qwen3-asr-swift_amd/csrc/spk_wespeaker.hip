// spk_wespeaker.hip -- WeSpeaker ResNet34 speaker embeddings for gfx950 (spk_wespeaker.h).
//
// One device pass embeds a ragged batch.  Clips are packed along the time axis of ONE image: clip b's level-0 frames sit at columns
// col0[b] .. col0[b] + T_b - 1, col0 a multiple of 8, with at least 8 zero guard columns before and after it.  At level l (F = 80 >> l,
// time / 2^l after each stride-2 stage) the clip starts at col0 / 2^l and keeps >= 1 zero column on each side, and every epilogue writes
// 0 to the columns outside the clips' valid ranges, so each edge sees exactly the zero padding a lone clip sees.  Cost follows the
// total frame count, not B x the longest clip.
//   spk_frames_kernel   one wavefront per frame of any clip: pre-emphasis, reflect pad, Hamming, 512-point power (melc_frame_power, x 4
//                       as vDSP_fft_zrip's 2x scaled spectrum), sparse HTK mel bank, log(max(x, 1e-10)) -> raw [frames][80] f32
//   spk_cmn_kernel      one workgroup per clip: per-bin mean over the clip's frames (4 fixed strided partial sums combined in a fixed
//                       tree), subtracted; writes the packed [80][W0] f32 feature image (guard columns stay zero)
//   spk_stem_kernel     conv1 1 -> 32 on VALU (9 taps in order, f32), + bias, ReLU, masked -> bf16 [80][W0][32]
//   spk_conv_kernel     (spk_conv.h) 32 MFMA launches: two per BasicBlock, the downsampling shortcut folded into conv2
//   spk_pool_kernel     one workgroup per clip: mean, then the two-pass population variance over the clip's T' columns (sequential
//                       f32 sums), Linear 5120 -> 256 (one sequential fmaf chain per output), L2 normalisation (DPP tree, fixed order)
// Precision: MFMA operands (3x3 / shortcut weights, stored activations) bf16, f32 accumulation and epilogues,
// front end, stem, pooling, linear and normalisation f32.  No workgroup waits for another and no sum uses atomics: results are
// deterministic, and a clip's embedding is bit-identical alone or in any batch.
#include "spk_wespeaker.h"
#include "spk_conv.h"
#include "mel_core.h"
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>

namespace qasr {

constexpr int SPK_BLOCKS[4] = {3, 4, 6, 3};

// meta block (one pass): long pcm_off[cap] | int n[cap] | int frame_off[cap + 1] | int col0[cap] | uchar colvalid[W0 + W0/2 + W0/4 + W0/8]
struct SpkMeta {
    const long* pcm_off;
    const int* n;
    const int* frame_off;
    const int* col0;
    const unsigned char* colvalid;
};

static size_t spk_meta_bytes(size_t clips, size_t cols) {
    return clips * sizeof(long) + (3 * clips + 1) * sizeof(int) + 2 * cols + 16;
}
static SpkMeta spk_meta_ptrs(char* base, size_t clips) {
    SpkMeta m;
    m.pcm_off = reinterpret_cast<const long*>(base);
    const int* p = reinterpret_cast<const int*>(base + clips * sizeof(long));
    m.n = p; m.frame_off = p + clips; m.col0 = p + 2 * clips + 1;
    m.colvalid = reinterpret_cast<const unsigned char*>(p + 3 * clips + 1);
    return m;
}

// ---- front end ----------------------------------------------------------------------------------------------------------
constexpr int FE_WAVES = 4;

// emphasised sample of the reflect-padded signal at padded index q (MelFeatureExtractor.extractRaw: left min(200 - i, n - 1),
// right max(0, n - 2 - i), pre-emphasis y[0] = x[0], y[i] = x[i] - 0.97 x[i - 1])
__device__ __forceinline__ float spk_padded(const float* x, long n, long q) {
    const long pad = SPK_WIN / 2;
    long i;
    if (q < pad) { i = pad - q < n - 1 ? pad - q : n - 1; i = i < 0 ? 0 : i; }
    else if (q < pad + n) i = q - pad;
    else { i = n - 2 - (q - pad - n); i = i < 0 ? 0 : i; }
    return i == 0 ? x[0] : x[i] - 0.97f * x[i - 1];
}

__global__ __launch_bounds__(FE_WAVES * 64) void spk_frames_kernel(const float* __restrict__ tab, const float* __restrict__ pcm, SpkMeta meta,
                                                                   int B, int total, float* __restrict__ raw) {
    __shared__ float s_tab[T_TOTAL];
    __shared__ float2 s_buf[FE_WAVES][2][256];
    __shared__ float s_pow[FE_WAVES][260];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < T_TOTAL; i += FE_WAVES * 64) s_tab[i] = tab[i];
    __syncthreads();
    const int g = blockIdx.x * FE_WAVES + wave;
    const bool live = g < total;                           // barriers inside melc_frame_power stay uniform
    int b = 0;
    if (live) {                                            // last clip whose first frame is <= g
        int lo = 0, hi = B - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (meta.frame_off[mid] <= g) lo = mid; else hi = mid - 1;
        }
        b = lo;
    }
    const long n = meta.n[b];
    const float* x = pcm + meta.pcm_off[b];
    const long start = (long)(g - meta.frame_off[b]) * SPK_HOP;
    cplx v[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int p = lane + 64 * r;
        float a0 = 0.0f, a1 = 0.0f;
        if (live && 2 * p < SPK_WIN) {                     // 400 is even: both samples of the pair are inside the window
            a0 = spk_padded(x, n, start + 2 * p) * s_tab[T_HANN + 2 * p];
            a1 = spk_padded(x, n, start + 2 * p + 1) * s_tab[T_HANN + 2 * p + 1];
        }
        v[r] = {a0, a1};
    }
    const float2* tw256 = reinterpret_cast<const float2*>(&s_tab[T_TW256]);
    const float2* tw512 = reinterpret_cast<const float2*>(&s_tab[T_TW512]);
    float* pw = s_pow[wave];
    melc_frame_power(v, lane, s_buf[wave][0], s_buf[wave][1], pw, tw256, tw512, s_tab[T_SCALE2]);
    if (live) {
        for (int m = lane; m < SPK_NMELS; m += 64) raw[(long)g * SPK_NMELS + m] = logf(fmaxf(melc_filter(s_tab, pw, m), 1e-10f));
    }
}

constexpr int CMN_PARTS = 4;

__global__ __launch_bounds__(SPK_NMELS * CMN_PARTS) void spk_cmn_kernel(const float* __restrict__ raw, SpkMeta meta, int W0,
                                                                        float* __restrict__ feat) {
    __shared__ float s_part[CMN_PARTS][SPK_NMELS];
    const int b = blockIdx.x, bin = threadIdx.x % SPK_NMELS, part = threadIdx.x / SPK_NMELS;
    const int T = spk_num_frames((size_t)meta.n[b]);
    const float* src = raw + (long)meta.frame_off[b] * SPK_NMELS + bin;
    float s = 0.0f;
    for (int t = part; t < T; t += CMN_PARTS) s += src[(long)t * SPK_NMELS];
    s_part[part][bin] = s;
    __syncthreads();
    const float mean = ((s_part[0][bin] + s_part[1][bin]) + (s_part[2][bin] + s_part[3][bin])) * (1.0f / (float)T);
    float* dst = feat + (long)bin * W0 + meta.col0[b];
    for (int t = part; t < T; t += CMN_PARTS) dst[t] = src[(long)t * SPK_NMELS] - mean;
}

// conv1 (1 -> 32, 3x3, pad 1) + bias + ReLU on VALU; thread = output pixel of the [80][W0] image
__global__ __launch_bounds__(256) void spk_stem_kernel(const float* __restrict__ feat, const float* __restrict__ w, const float* __restrict__ bias,
                                                       const unsigned char* __restrict__ colvalid, int W0, bf16_t* __restrict__ out) {
    __shared__ float s_w[32 * 9 + 32];
    for (int i = threadIdx.x; i < 32 * 9; i += 256) s_w[i] = w[i];
    if (threadIdx.x < 32) s_w[32 * 9 + threadIdx.x] = bias[threadIdx.x];
    __syncthreads();
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= (long)SPK_NMELS * W0) return;
    const int f = (int)(p / W0), t = (int)(p - (long)f * W0);
    float v[9];
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
        const int fi = f + tap / 3 - 1, ti = t + tap % 3 - 1;
        v[tap] = (fi >= 0 && fi < SPK_NMELS && ti >= 0 && ti < W0) ? feat[(long)fi * W0 + ti] : 0.0f;
    }
    const bool valid = colvalid[t] != 0;
    unsigned packed[16];
#pragma unroll
    for (int c = 0; c < 32; c += 2) {
        float a0 = 0.0f, a1 = 0.0f;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) { a0 = fmaf(s_w[c * 9 + tap], v[tap], a0); a1 = fmaf(s_w[(c + 1) * 9 + tap], v[tap], a1); }
        a0 = fmaxf(a0 + s_w[288 + c], 0.0f);
        a1 = fmaxf(a1 + s_w[288 + c + 1], 0.0f);
        packed[c / 2] = valid ? pack_bf16x2(a0, a1) : 0u;
    }
    uint4* dst = reinterpret_cast<uint4*>(out + p * 32);
#pragma unroll
    for (int q = 0; q < 4; ++q) dst[q] = make_uint4(packed[4 * q], packed[4 * q + 1], packed[4 * q + 2], packed[4 * q + 3]);
}

// statistics pooling + embedding + L2 normalisation, one workgroup per clip (thread = channel for the pooling, output for the linear)
__global__ __launch_bounds__(256) void spk_pool_kernel(const bf16_t* __restrict__ act, SpkMeta meta, int W3, const float* __restrict__ wl,
                                                       const float* __restrict__ bl, float* __restrict__ emb) {
    __shared__ float s_pool[SPK_POOL];
    __shared__ float s_red[4];
    const int b = blockIdx.x, c = threadIdx.x, lane = c & 63, wave = c >> 6;
    int T = spk_num_frames((size_t)meta.n[b]);
    T = (T + 1) >> 1; T = (T + 1) >> 1; T = (T + 1) >> 1;
    const int col3 = meta.col0[b] >> 3;
    const float inv = 1.0f / (float)T;
    for (int f = 0; f < 10; ++f) {
        const bf16_t* p = act + ((long)f * W3 + col3) * 256 + c;
        float s = 0.0f;
        for (int t = 0; t < T; ++t) s += bf16_to_f32(p[(long)t * 256]);
        const float mean = s * inv;
        float q = 0.0f;
        for (int t = 0; t < T; ++t) { const float d = bf16_to_f32(p[(long)t * 256]) - mean; q = fmaf(d, d, q); }
        s_pool[c * 10 + f] = mean;                         // C*F order: feature c * 10 + f
        s_pool[2560 + c * 10 + f] = sqrtf(q * inv + 1e-10f);
    }
    __syncthreads();
    float e = 0.0f;
    for (int k = 0; k < SPK_POOL; ++k) e = fmaf(s_pool[k], wl[(long)k * SPK_DIM + c], e);
    e += bl[c];
    const float ss = lane_sum<64>(e * e);
    if (lane == 0) s_red[wave] = ss;
    __syncthreads();
    const float tot = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
    emb[(long)b * SPK_DIM + c] = e / sqrtf(tot + 1e-10f);
}

// ---- weights ------------------------------------------------------------------------------------------------------------
static std::string blk(int s, int i) { return "layer" + std::to_string(s + 1) + "." + std::to_string(i) + "."; }

const std::vector<std::pair<std::string, std::vector<int64_t>>>& spk_tensor_shapes() {
    static const std::vector<std::pair<std::string, std::vector<int64_t>>> s = [] {
        std::vector<std::pair<std::string, std::vector<int64_t>>> v;
        v.push_back({"conv1.weight", {32, 3, 3, 1}});
        v.push_back({"conv1.bias", {32}});
        for (int st = 0; st < 4; ++st) {
            const int64_t C = 32 << st, Cp = st ? 16 << st : 32;
            for (int i = 0; i < SPK_BLOCKS[st]; ++i) {
                const int64_t cin = i == 0 ? Cp : C;
                v.push_back({blk(st, i) + "conv1.weight", {C, 3, 3, cin}});
                v.push_back({blk(st, i) + "conv1.bias", {C}});
                v.push_back({blk(st, i) + "conv2.weight", {C, 3, 3, C}});
                v.push_back({blk(st, i) + "conv2.bias", {C}});
                if (st > 0 && i == 0) {
                    v.push_back({blk(st, i) + "shortcut.weight", {C, 1, 1, Cp}});
                    v.push_back({blk(st, i) + "shortcut.bias", {C}});
                }
            }
        }
        v.push_back({"embedding.weight", {SPK_DIM, SPK_POOL}});
        v.push_back({"embedding.bias", {SPK_DIM}});
        return v;
    }();
    return s;
}

// HTK mel bank of MelFeatureExtractor.setupMelFilterbank (f32, the reference's formulas) in mel_core.h's sparse table slots
static void spk_fill_tables(std::vector<float>& t) {
    melc_fill_tables(t, 4.0f);                             // twiddles + power scale (|2X|^2); the Whisper bank it writes is replaced below
    for (int i = 0; i < 512; ++i) t[T_HANN + i] = i < SPK_WIN ? 0.54f - 0.46f * cosf(2.0f * (float)M_PI * (float)i / 399.0f) : 0.0f;
    auto hz2mel = [](float hz) { return 2595.0f * log10f(1.0f + hz / 700.0f); };
    auto mel2hz = [](float mel) { return 700.0f * (powf(10.0f, mel / 2595.0f) - 1.0f); };
    const int npts = SPK_NMELS + 2;
    const float mmin = hz2mel(20.0f), mmax = hz2mel(8000.0f);
    std::vector<float> ff(npts), diff(npts - 1);
    for (int i = 0; i < npts; ++i) ff[i] = mel2hz(mmin + (float)i * (mmax - mmin) / (float)(npts - 1));
    for (int i = 0; i < npts - 1; ++i) diff[i] = ff[i + 1] - ff[i];
    int* fb_start = reinterpret_cast<int*>(&t[T_FBSTART]);
    int* fb_len = reinterpret_cast<int*>(&t[T_FBLEN]);
    int* fb_woff = reinterpret_cast<int*>(&t[T_FBWOFF]);
    for (int m = 0; m < MELC_NMELS; ++m) fb_start[m] = fb_len[m] = fb_woff[m] = 0;
    int w = 0;
    for (int m = 0; m < SPK_NMELS; ++m) {
        const float enorm = 2.0f / (ff[m + 2] - ff[m]);
        int first = -1, last = -1;
        std::vector<float> row(MELC_NBINS);
        for (int k = 0; k < MELC_NBINS; ++k) {
            const float f = (float)k * 16000.0f / 512.0f;
            const float down = (f - ff[m]) / diff[m], up = (ff[m + 2] - f) / diff[m + 1];
            row[k] = std::max(0.0f, std::min(down, up)) * enorm;
            if (row[k] != 0.0f) { if (first < 0) first = k; last = k; }
        }
        fb_start[m] = first < 0 ? 0 : first;
        fb_len[m] = first < 0 ? 0 : last - first + 1;
        fb_woff[m] = w;
        for (int k = fb_start[m]; k < fb_start[m] + fb_len[m]; ++k) {
            if (w >= FBW_CAP) throw std::runtime_error("wespeaker: mel filterbank exceeds FBW_CAP");
            t[T_FBW + w++] = row[k];
        }
    }
}

// ---- host object --------------------------------------------------------------------------------------------------------
WeSpeaker::WeSpeaker(int device, const CheckedWeights& w, size_t max_samples, hipStream_t work)
    : device_(device), max_samples_(max_samples) {
    if (max_samples_ < (size_t)SPK_WIN) throw std::invalid_argument("wespeaker: max_batch_samples below 400");
    cap_clips_ = 1024;
    cap_frames_ = max_samples_ / SPK_HOP + cap_clips_;
    const size_t t_max = max_samples_ / SPK_HOP + 1;
    cap_cols_ = SPK_COL_ALIGN + SPK_COL_ALIGN * ((t_max + 7) / 8 + 1) + 64 * 2 * SPK_COL_ALIGN;
    if (cap_cols_ * SPK_NMELS > (size_t)1 << 30) throw std::length_error("wespeaker: max_batch_samples too large");

    // device weights: 3x3 convs bf16 [CO][9 CA (+ CX)] in layer order (conv1, conv2 per block), biases f32 (conv2 + shortcut folded)
    std::vector<bf16_t> wc;
    std::vector<float> bias;
    param_bytes_ = w.disk_bytes;
    for (int st = 0; st < 4; ++st) {
        const int C = 32 << st, Cp = st ? 16 << st : 32;
        for (int i = 0; i < SPK_BLOCKS[st]; ++i) {
            const int cin = i == 0 ? Cp : C;
            const bool ds = st > 0 && i == 0;
            const auto& w1 = w.t.at(blk(st, i) + "conv1.weight");
            for (float x : w1) wc.push_back(f32_to_bf16_host(x));
            const auto& b1 = w.t.at(blk(st, i) + "conv1.bias");
            bias.insert(bias.end(), b1.begin(), b1.end());
            const auto& w2 = w.t.at(blk(st, i) + "conv2.weight");
            const auto& b2 = w.t.at(blk(st, i) + "conv2.bias");
            for (int o = 0; o < C; ++o) {
                for (int k = 0; k < 9 * C; ++k) wc.push_back(f32_to_bf16_host(w2[(size_t)o * 9 * C + k]));
                if (ds) {
                    const auto& ws = w.t.at(blk(st, i) + "shortcut.weight");
                    for (int k = 0; k < cin; ++k) wc.push_back(f32_to_bf16_host(ws[(size_t)o * cin + k]));
                }
            }
            for (int o = 0; o < C; ++o) bias.push_back(ds ? b2[o] + w.t.at(blk(st, i) + "shortcut.bias")[o] : b2[o]);
        }
    }
    std::vector<float> stem(32 * 9 + 32);
    for (int i = 0; i < 32 * 9; ++i) stem[i] = w.t.at("conv1.weight")[i];     // [32][3][3][1] = [o][tap]
    for (int o = 0; o < 32; ++o) stem[288 + o] = w.t.at("conv1.bias")[o];
    std::vector<float> lin((size_t)SPK_POOL * SPK_DIM + SPK_DIM);
    const auto& we = w.t.at("embedding.weight");
    for (int o = 0; o < SPK_DIM; ++o)
        for (int k = 0; k < SPK_POOL; ++k) lin[(size_t)k * SPK_DIM + o] = we[(size_t)o * SPK_POOL + k];
    for (int o = 0; o < SPK_DIM; ++o) lin[(size_t)SPK_POOL * SPK_DIM + o] = w.t.at("embedding.bias")[o];
    std::vector<float> tab(T_TOTAL, 0.0f);
    spk_fill_tables(tab);

    QASR_HIP(hipSetDevice(device_));
    QASR_HIP(hipStreamCreateWithFlags(&own_, hipStreamNonBlocking));
    work_ = work ? work : own_;
    for (auto& e : ev_) QASR_HIP(hipEventCreate(&e));
    auto up = [](DevBuf& d, const void* src, size_t bytes) {
        d.alloc(bytes);
        QASR_HIP(hipMemcpy(d.p, src, bytes, hipMemcpyHostToDevice));
    };
    up(d_wconv_, wc.data(), wc.size() * sizeof(bf16_t));
    up(d_bias_, bias.data(), bias.size() * sizeof(float));
    up(d_wstem_, stem.data(), stem.size() * sizeof(float));
    up(d_wlin_, lin.data(), lin.size() * sizeof(float));
    up(d_tab_, tab.data(), tab.size() * sizeof(float));

    h_pcm_.alloc(max_samples_ * sizeof(float));
    d_pcm_.alloc(max_samples_ * sizeof(float));
    h_meta_.alloc(spk_meta_bytes(cap_clips_, cap_cols_));
    d_meta_.alloc(spk_meta_bytes(cap_clips_, cap_cols_));
    d_raw_.alloc(cap_frames_ * SPK_NMELS * sizeof(float));
    d_feat_.alloc(cap_cols_ * SPK_NMELS * sizeof(float));
    const size_t lvl0 = cap_cols_ * SPK_NMELS * 32;        // elements of the level-0 image; every later level holds half of the previous
    d_act_[0].alloc(lvl0 * sizeof(bf16_t));
    d_act_[1].alloc(lvl0 * sizeof(bf16_t));
    d_act_[2].alloc(lvl0 / 2 * sizeof(bf16_t));
    d_emb_.alloc(cap_clips_ * SPK_DIM * sizeof(float));
    h_out_.alloc(std::max(cap_clips_ * SPK_DIM, cap_cols_ * SPK_NMELS) * sizeof(float));
}

WeSpeaker::~WeSpeaker() {
    if (work_) (void)hipStreamSynchronize(work_);
    for (auto& e : ev_) if (e) (void)hipEventDestroy(e);
    if (own_) (void)hipStreamDestroy(own_);
}

void WeSpeaker::unload() {
    if (!loaded_) return;
    QASR_HIP(hipSetDevice(device_));
    QASR_HIP(hipStreamSynchronize(work_));
    d_wconv_.release(); d_bias_.release(); d_wstem_.release(); d_wlin_.release();
    d_pcm_.release(); d_raw_.release(); d_feat_.release(); d_emb_.release();
    for (auto& a : d_act_) a.release();
    loaded_ = false;
}

static size_t spk_clip_cols(size_t n) { return SPK_COL_ALIGN * (((size_t)spk_num_frames(n) + 7) / 8 + 1); }

std::vector<WeSpeaker::Pass> WeSpeaker::plan(const size_t* n, size_t B) const {
    std::vector<Pass> ps;
    Pass cur{0, 0, 0, 0, SPK_COL_ALIGN};
    for (size_t b = 0; b < B; ++b) {
        if (n[b] == 0) throw std::invalid_argument("wespeaker: empty clip");
        if (n[b] > max_samples_) throw std::length_error("wespeaker: clip of " + std::to_string(n[b]) + " samples exceeds the workspace (" +
                                                         std::to_string(max_samples_) + ")");
        const size_t cols = spk_clip_cols(n[b]), fr = (size_t)spk_num_frames(n[b]);
        if (cur.count && (cur.samples + n[b] > max_samples_ || cur.cols + cols > cap_cols_ || cur.count + 1 > cap_clips_ ||
                          cur.frames + fr > cap_frames_)) {
            ps.push_back(cur);
            cur = Pass{b, 0, 0, 0, SPK_COL_ALIGN};
        }
        cur.count++; cur.samples += n[b]; cur.cols += (int)cols; cur.frames += (int)fr;
    }
    if (cur.count) ps.push_back(cur);
    return ps;
}

void WeSpeaker::stage(const float* const* pcm, const size_t* n, const Pass& p) {
    char* base = h_meta_.as<char>();
    SpkMeta m = spk_meta_ptrs(base, cap_clips_);
    long* off = const_cast<long*>(m.pcm_off);
    int *nn = const_cast<int*>(m.n), *fo = const_cast<int*>(m.frame_off), *c0 = const_cast<int*>(m.col0);
    unsigned char* cv = const_cast<unsigned char*>(m.colvalid);
    const size_t W0 = (size_t)p.cols;
    std::memset(cv, 0, W0 + W0 / 2 + W0 / 4 + W0 / 8);
    size_t so = 0;
    int fr = 0, col = SPK_COL_ALIGN;
    for (size_t k = 0; k < p.count; ++k) {
        const size_t b = p.first + k;
        if (!pcm[b]) throw std::invalid_argument("wespeaker: null clip");
        off[k] = (long)so; nn[k] = (int)n[b]; fo[k] = fr; c0[k] = col;
        std::memcpy(h_pcm_.as<float>() + so, pcm[b], n[b] * sizeof(float));
        int T = spk_num_frames(n[b]);
        size_t lvl = 0;
        for (int l = 0; l < 4; ++l) {                      // valid columns of the clip at every level
            std::memset(cv + lvl + (col >> l), 1, (size_t)T);
            lvl += W0 >> l;
            T = (T + 1) / 2;
        }
        so += n[b]; fr += spk_num_frames(n[b]); col += (int)spk_clip_cols(n[b]);
    }
    fo[p.count] = fr;
}

void WeSpeaker::front(const Pass& p, hipStream_t s) {
    QASR_HIP(hipMemcpyAsync(d_meta_.p, h_meta_.p, spk_meta_bytes(cap_clips_, cap_cols_), hipMemcpyHostToDevice, s));
    QASR_HIP(hipMemcpyAsync(d_pcm_.p, h_pcm_.p, p.samples * sizeof(float), hipMemcpyHostToDevice, s));
    QASR_HIP(hipMemsetAsync(d_feat_.p, 0, (size_t)p.cols * SPK_NMELS * sizeof(float), s));
    const SpkMeta m = spk_meta_ptrs(d_meta_.as<char>(), cap_clips_);
    hipLaunchKernelGGL(spk_frames_kernel, dim3(cdiv(p.frames, FE_WAVES)), dim3(FE_WAVES * 64), 0, s, d_tab_.as<float>(), d_pcm_.as<float>(), m,
                       (int)p.count, p.frames, d_raw_.as<float>());
    hipLaunchKernelGGL(spk_cmn_kernel, dim3((unsigned)p.count), dim3(SPK_NMELS * CMN_PARTS), 0, s, d_raw_.as<float>(), m, p.cols,
                       d_feat_.as<float>());
}

template <int CA, int S, int CX, bool RES, int CO>
static void spk_conv(const SpkConvArgs& a, hipStream_t s) {
    constexpr int NCOL = CO < 64 ? CO : 64;
    const int M = a.F_out * a.W_out;
    hipLaunchKernelGGL((spk_conv_kernel<CA, S, CX, RES, CO>), dim3(cdiv(M, SPK_CONV_THREADS), CO / NCOL), dim3(SPK_CONV_THREADS), 0, s, a);
}

// the 3x3 convolutions of stage st (C = 32 << st channels); downsampling first block when st > 0
template <int C>
static void spk_stage(int nblocks, const bf16_t* wc, size_t& woff, const float* bias, int& boff, bf16_t* act[3], int& x, int& y, int& z,
                      int F, int W, const unsigned char* cv, hipStream_t s) {
    constexpr int Cp = C == 32 ? 32 : C / 2;
    for (int i = 0; i < nblocks; ++i) {
        SpkConvArgs a{};
        a.F_out = F; a.W_out = W; a.colvalid = cv;
        if (C != 32 && i == 0) {
            a.in = act[x]; a.F_in = 2 * F; a.W_in = 2 * W; a.w = wc + woff; a.bias = bias + boff; a.out = act[y];
            spk_conv<Cp, 2, 0, false, C>(a, s);
            woff += (size_t)C * 9 * Cp; boff += C;
            a.in = act[y]; a.F_in = F; a.W_in = W; a.sc = act[x]; a.w = wc + woff; a.bias = bias + boff; a.out = act[z];
            spk_conv<C, 1, Cp, false, C>(a, s);
            woff += (size_t)C * (9 * C + Cp); boff += C;
            std::swap(x, z);
        } else {
            a.in = act[x]; a.F_in = F; a.W_in = W; a.w = wc + woff; a.bias = bias + boff; a.out = act[y];
            spk_conv<C, 1, 0, false, C>(a, s);
            woff += (size_t)C * 9 * C; boff += C;
            a.in = act[y]; a.res = act[x]; a.w = wc + woff; a.bias = bias + boff; a.out = act[x];
            spk_conv<C, 1, 0, true, C>(a, s);
            woff += (size_t)C * 9 * C; boff += C;
        }
    }
}

void WeSpeaker::network(const Pass& p, hipStream_t s) {
    const SpkMeta m = spk_meta_ptrs(d_meta_.as<char>(), cap_clips_);
    const int W0 = p.cols;
    const unsigned char* cv = m.colvalid;
    bf16_t* act[3] = {d_act_[0].as<bf16_t>(), d_act_[1].as<bf16_t>(), d_act_[2].as<bf16_t>()};
    hipLaunchKernelGGL(spk_stem_kernel, dim3(cdiv((long)SPK_NMELS * W0, 256)), dim3(256), 0, s, d_feat_.as<float>(), d_wstem_.as<float>(),
                       d_wstem_.as<float>() + 288, cv, W0, act[0]);
    int x = 0, y = 1, z = 2;
    size_t woff = 0;
    int boff = 0;
    const bf16_t* wc = d_wconv_.as<bf16_t>();
    const float* bias = d_bias_.as<float>();
    spk_stage<32>(SPK_BLOCKS[0], wc, woff, bias, boff, act, x, y, z, 80, W0, cv, s);
    spk_stage<64>(SPK_BLOCKS[1], wc, woff, bias, boff, act, x, y, z, 40, W0 / 2, cv + W0, s);
    spk_stage<128>(SPK_BLOCKS[2], wc, woff, bias, boff, act, x, y, z, 20, W0 / 4, cv + W0 + W0 / 2, s);
    spk_stage<256>(SPK_BLOCKS[3], wc, woff, bias, boff, act, x, y, z, 10, W0 / 8, cv + W0 + W0 / 2 + W0 / 4, s);
    hipLaunchKernelGGL(spk_pool_kernel, dim3((unsigned)p.count), dim3(256), 0, s, act[x], m, W0 / 8, d_wlin_.as<float>(),
                       d_wlin_.as<float>() + (size_t)SPK_POOL * SPK_DIM, d_emb_.as<float>());
}

void WeSpeaker::embed(const float* const* pcm, const size_t* n, size_t B, float* out) {
    if (!loaded_) throw NotLoaded("wespeaker: model unloaded");
    if (B == 0) return;
    const auto passes = plan(n, B);
    QASR_HIP(hipSetDevice(device_));
    QASR_HIP(hipEventRecord(ev_[0], work_));
    for (const Pass& p : passes) {
        stage(pcm, n, p);
        front(p, work_);
        network(p, work_);
        QASR_HIP(hipMemcpyAsync(h_out_.p, d_emb_.p, p.count * SPK_DIM * sizeof(float), hipMemcpyDeviceToHost, work_));
        QASR_HIP(hipStreamSynchronize(work_));            // the host staging buffers are reused by the next pass
        QASR_HIP(hipGetLastError());
        std::memcpy(out + p.first * SPK_DIM, h_out_.p, p.count * SPK_DIM * sizeof(float));
    }
    QASR_HIP(hipEventRecord(ev_[1], work_));
    QASR_HIP(hipEventSynchronize(ev_[1]));
    QASR_HIP(hipEventElapsedTime(&last_ms_, ev_[0], ev_[1]));
}

void WeSpeaker::fbank(const float* const* pcm, const size_t* n, size_t B, float* feats, size_t stride, int32_t* n_frames) {
    if (!loaded_) throw NotLoaded("wespeaker: model unloaded");
    if (B == 0) return;
    for (size_t b = 0; b < B; ++b)
        if (n[b] && (size_t)spk_num_frames(n[b]) * SPK_NMELS > stride) throw std::invalid_argument("wespeaker: stride below T * 80");
    const auto passes = plan(n, B);
    QASR_HIP(hipSetDevice(device_));
    QASR_HIP(hipEventRecord(ev_[0], work_));
    for (const Pass& p : passes) {
        stage(pcm, n, p);
        front(p, work_);
        QASR_HIP(hipMemcpyAsync(h_out_.p, d_feat_.p, (size_t)p.cols * SPK_NMELS * sizeof(float), hipMemcpyDeviceToHost, work_));
        QASR_HIP(hipStreamSynchronize(work_));
        QASR_HIP(hipGetLastError());
        const SpkMeta m = spk_meta_ptrs(h_meta_.as<char>(), cap_clips_);
        const float* img = h_out_.as<float>();
        for (size_t k = 0; k < p.count; ++k) {
            const int T = spk_num_frames(n[p.first + k]);
            float* dst = feats + (p.first + k) * stride;
            for (int t = 0; t < T; ++t)
                for (int f = 0; f < SPK_NMELS; ++f) dst[(size_t)t * SPK_NMELS + f] = img[(size_t)f * p.cols + m.col0[k] + t];
            if (n_frames) n_frames[p.first + k] = T;
        }
    }
    QASR_HIP(hipEventRecord(ev_[1], work_));
    QASR_HIP(hipEventSynchronize(ev_[1]));
    QASR_HIP(hipEventElapsedTime(&last_ms_, ev_[0], ev_[1]));
}

}  // namespace qasr
