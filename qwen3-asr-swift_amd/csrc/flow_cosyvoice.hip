// flow_cosyvoice.hip -- kernels and host object of the CosyVoice3 flow-matching mel decoder (flow_cosyvoice.h).
// Heavy launches are the bf16 MFMA GEMM of gemm.h with the operand gathers and epilogues below, and mha_attention_launch as it stands.
#include "flow_cosyvoice.h"
#include "ctc_kernels.h"
#include "gemm.h"
#include "qasr.h"
#include <algorithm>
#include <cmath>
#include <set>

namespace qasr {

// =====================================================================================================================================
// kernels
// =====================================================================================================================================
__device__ __forceinline__ float fl_silu(float x) { return x / (1.0f + expf(-x)); }
__device__ __forceinline__ float fl_mish(float x) { return x * tanhf(log1pf(expf(x))); }                     // DiT.swift:325-327
__device__ __forceinline__ float fl_gelu_tanh(float x) {                                                      // geluApproximate
    return 0.5f * x * (1.0f + tanhf(0.7978845608028654f * (x + 0.044715f * x * x * x)));
}

// sinusoid of a time step (DiT.swift:22-32): half = 128, out [rows][256] = [sin | cos] of 1000 t f_i.  Bound: nothing, 256 values per row.
__global__ void fl_sinusoid_kernel(const float* __restrict__ t, int rows, float* __restrict__ out) {
    const int i = threadIdx.x, r = blockIdx.x;
    if (r >= rows || i >= FL_FREQ / 2) return;
    const float log_factor = 9.210340371976184f / (float)(FL_FREQ / 2 - 1);
    const float a = (1000.0f * t[r]) * expf((float)i * (-log_factor));
    out[(long)r * FL_FREQ + i] = sinf(a);
    out[(long)r * FL_FREQ + FL_FREQ / 2 + i] = cosf(a);
}

// y[row][n] = bias[n] + sum_k x[row][k] (scale q + zero)[n][k] on a packed MLX 4 / 8 bit matrix, one wave per (n, row), f32 throughout.
// A lane takes whole words (8 or 4 elements of one group) at stride 64 words, then the wave sums: the order depends on (n, K, bits) only,
// so a row of an n_steps-row table equals the same row computed alone.  Bound: the packed weight read (L2 resident after the first row).
__global__ __launch_bounds__(256) void fl_qgemv_kernel(const uint32_t* __restrict__ W, const float* __restrict__ S, const float* __restrict__ Z,
                                                       const float* __restrict__ bias, int N, int K, int bits, const float* __restrict__ x,
                                                       long ldx, float* __restrict__ out, float* __restrict__ out_silu, long ldo) {
    const int lane = threadIdx.x & 63, n = blockIdx.x * 4 + (threadIdx.x >> 6), row = blockIdx.y;
    if (n >= N) return;
    const int per = 32 / bits, wpr = K / per, gpr = K / FL_GROUP;
    const uint32_t mask = (1u << bits) - 1u;
    const float* xr = x + (long)row * ldx;
    float acc = 0.0f;
    for (int w = lane; w < wpr; w += 64) {
        const uint32_t word = W[(long)n * wpr + w];
        const int k0 = w * per, g = k0 / FL_GROUP;
        const float s = S[(long)n * gpr + g], z = Z[(long)n * gpr + g];
        for (int e = 0; e < per; ++e) acc += xr[k0 + e] * (s * (float)((word >> (e * bits)) & mask) + z);
    }
    acc = wave_sum(acc);
    if (lane == 0) {
        const float y = acc + bias[n];
        if (out) out[(long)row * ldo + n] = y;
        if (out_silu) out_silu[(long)row * ldo + n] = fl_silu(y);
    }
}

// x0 of a clip: element (frame t, bin m) = temperature * hift_normal of draw 80 t + m of the clip's stream
__global__ void fl_noise_kernel(const int* __restrict__ cu, int n_clips, const unsigned long long* __restrict__ seed, const float* __restrict__ temp,
                                long total, float* __restrict__ x, bf16_t* __restrict__ xb) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int row = (int)(i / FL_MEL);
    int c = 0;
    while (c + 1 < n_clips && cu[c + 1] <= row) ++c;
    const unsigned long long counter = (unsigned long long)(i - (long)cu[c] * FL_MEL);
    const float v = __fmul_rn(temp[c], hift_normal(hift_draw(seed[c], counter)));
    x[i] = v;
    xb[i] = f32_to_bf16(v);
}

__global__ void fl_cast_kernel(const float* __restrict__ x, bf16_t* __restrict__ y, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = f32_to_bf16(x[i]);
}

// x += dt ((1 + cfg) v_c - cfg v_u) (FlowMatching.swift:186-189), each product and sum rounded once, in this order; also the bf16 image of x
__global__ void fl_euler_kernel(float* __restrict__ x, bf16_t* __restrict__ xb, const float* __restrict__ vc, const float* __restrict__ vu, float dt,
                                float cfg, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float a = __fmul_rn(__fadd_rn(1.0f, cfg), vc[i]);
    const float b = __fmul_rn(cfg, vu[i]);
    const float v = __fsub_rn(a, b);
    const float r = __fadd_rn(x[i], __fmul_rn(dt, v));
    x[i] = r;
    xb[i] = f32_to_bf16(r);
}

// the mu path (FlowMatching.swift:204-227, :315-321), f32, one clip per launch; under 1 % of the work
// h[r][c] = relu(b[c] + sum_{j < 4, r + j < n} sum_i w1[c][j][i] E[tok[r + j]][i]): the look-ahead conv pads on the right
__global__ __launch_bounds__(256) void fl_look1_kernel(const int* __restrict__ tok, int n, const float* __restrict__ E, const float* __restrict__ w1,
                                                       const float* __restrict__ b1, float* __restrict__ h) {
    __shared__ float e[FL_LOOK_K * FL_MEL];
    const int r = blockIdx.x;
    for (int i = threadIdx.x; i < FL_LOOK_K * FL_MEL; i += 256) {
        const int j = i / FL_MEL;
        e[i] = r + j < n ? E[(long)tok[r + j] * FL_MEL + (i - j * FL_MEL)] : 0.0f;
    }
    __syncthreads();
    for (int c = threadIdx.x; c < FL_DIM; c += 256) {
        const float* w = w1 + (long)c * (FL_LOOK_K * FL_MEL);
        float acc = 0.0f;
        for (int i = 0; i < FL_LOOK_K * FL_MEL; ++i) acc += w[i] * e[i];
        acc += b1[c];
        h[(long)r * FL_DIM + c] = acc > 0.0f ? acc : 0.0f;
    }
}
// mu[2 r][c] = mu[2 r + 1][c] = b[c] + sum_{j < 3, r - 2 + j >= 0} sum_i w2[c][j][i] h[r - 2 + j][i]; one wave per (r, c)
__global__ __launch_bounds__(256) void fl_look2_kernel(const float* __restrict__ h, int n, const float* __restrict__ w2, const float* __restrict__ b2,
                                                       float* __restrict__ mu) {
    const int lane = threadIdx.x & 63, o = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (o >= n * FL_MEL) return;
    const int r = o / FL_MEL, c = o - r * FL_MEL;
    float acc = 0.0f;
    for (int j = 0; j < FL_LOOK2_K; ++j) {
        const int s = r - (FL_LOOK2_K - 1) + j;
        if (s < 0) continue;
        const float* w = w2 + ((long)c * FL_LOOK2_K + j) * FL_DIM;
        const float* hr = h + (long)s * FL_DIM;
        for (int i = lane; i < FL_DIM; i += 64) acc += w[i] * hr[i];
    }
    acc = wave_sum(acc);
    if (lane == 0) {
        const float y = acc + b2[c];
        mu[(long)(2 * r) * FL_MEL + c] = y;
        mu[(long)(2 * r + 1) * FL_MEL + c] = y;
    }
}

// y_bf16[row] = LN(x[row]) (1 + scale) + shift, LN without affine, eps 1e-6, two-pass statistics in f32 (DiT.swift:112, :125, :262).
// One wave per row of 1024: a lane holds 2 x 8 consecutive values (16-byte loads, 16-byte stores).  Bound: HBM, 4 KiB in and 2 KiB out per row.
__global__ __launch_bounds__(256) void fl_ln_mod_kernel(const float* __restrict__ x, const float* __restrict__ scale, const float* __restrict__ shift,
                                                        bf16_t* __restrict__ y, int rows) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* p = x + (long)row * FL_DIM;
    float v[16];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const float4 a = *reinterpret_cast<const float4*>(p + j * 512 + lane * 8), b = *reinterpret_cast<const float4*>(p + j * 512 + lane * 8 + 4);
        v[8 * j + 0] = a.x; v[8 * j + 1] = a.y; v[8 * j + 2] = a.z; v[8 * j + 3] = a.w;
        v[8 * j + 4] = b.x; v[8 * j + 5] = b.y; v[8 * j + 6] = b.z; v[8 * j + 7] = b.w;
    }
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < 16; ++i) s += v[i];
    const float mean = wave_sum(s) * (1.0f / (float)FL_DIM);
    float ss = 0.0f;
#pragma unroll
    for (int i = 0; i < 16; ++i) { v[i] -= mean; ss += v[i] * v[i]; }
    const float inv = 1.0f / sqrtf(wave_sum(ss) * (1.0f / (float)FL_DIM) + 1e-6f);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int c = j * 512 + lane * 8;
        float o[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] = (v[8 * j + i] * inv) * (1.0f + scale[c + i]) + shift[c + i];
        uint4 u;
        u.x = pack_bf16x2(o[0], o[1]); u.y = pack_bf16x2(o[2], o[3]); u.z = pack_bf16x2(o[4], o[5]); u.w = pack_bf16x2(o[6], o[7]);
        *reinterpret_cast<uint4*>(y + (long)row * FL_DIM + c) = u;
    }
}

// ---- GEMM operand gathers (gemm.h) ---------------------------------------------------------------------------------------------------
// Row m of [x | cond | mu | spks] (DiT.swift:364-371) from four bf16 images, never stored: rows [0, S) read x row m, rows [S, M) are the
// unconditioned branch and read x row m - S; rows at or past Sc read zeros for columns 80 .. 319.  80 is a multiple of the 8-element chunk.
struct AFlowIn {
    const bf16_t *xb, *condb, *mub, *spkb;
    const int* clip_of;
    int S, Sc, M;
    static constexpr bool no_p8 = true;
    struct Row { int src, clip; };
    __device__ __forceinline__ Row row_init(int m) const {
        if (m >= M) return {-1, -1};
        const int src = m < S ? m : m - S;
        return {src, m < Sc ? clip_of[src] : -1};
    }
    __device__ __forceinline__ const bf16_t* addr(const Row& r, int k) const {
        if (r.src < 0 || k >= FL_IN) return nullptr;
        if (k < FL_MEL) return xb + (long)r.src * FL_MEL + k;
        if (r.clip < 0) return nullptr;
        if (k < 2 * FL_MEL) return condb + (long)r.src * FL_MEL + (k - FL_MEL);
        if (k < 3 * FL_MEL) return mub + (long)r.src * FL_MEL + (k - 2 * FL_MEL);
        return spkb + (long)r.clip * FL_MEL + (k - 3 * FL_MEL);
    }
    __device__ __forceinline__ uint4 load(const Row& r, int k) const {
        const bf16_t* p = addr(r, k);
        return p ? *reinterpret_cast<const uint4*>(p) : make_uint4(0, 0, 0, 0);
    }
    struct KT { int k; };
    __device__ __forceinline__ KT ktile(int k0, int c8) const { return {k0 + c8}; }
    __device__ __forceinline__ const bf16_t* addr_kt(const Row& r, const KT& t) const { return addr(r, t.k); }
};

// Grouped causal Conv1d k = 31 (DiT.swift:283-322) as an implicit GEMM per group: K index = tap * 64 + ci, tap j of the row at in-clip
// position t reads row t - 30 + j; taps that would read in front of the clip are exact zeros.  A 64-wide K-tile is one tap.
struct AFlowConv {
    const bf16_t* x;        // [rows][1024]
    const int* pos;         // in-clip position of every row
    int g, M;
    static constexpr bool no_p8 = true;
    struct Row { const bf16_t* base; int kmin; };
    __device__ __forceinline__ AFlowConv for_group(int grp) const { AFlowConv a = *this; a.g = grp; return a; }
    __device__ __forceinline__ Row row_init(int m) const {
        if (m >= M) return {nullptr, 0};
        const int t = pos[m];
        return {x + ((long)m - (FL_CONV_K - 1)) * FL_DIM + g * FL_GROUP, t >= FL_CONV_K - 1 ? 0 : FL_CONV_K - 1 - t};
    }
    __device__ __forceinline__ const bf16_t* addr(const Row& r, int k) const {
        if (!r.base || k >= FL_CONV_K * FL_GROUP) return nullptr;
        const int tap = k >> 6;
        if (tap < r.kmin) return nullptr;
        return r.base + (long)tap * FL_DIM + (k & 63);
    }
    __device__ __forceinline__ uint4 load(const Row& r, int k) const {
        const bf16_t* p = addr(r, k);
        return p ? *reinterpret_cast<const uint4*>(p) : make_uint4(0, 0, 0, 0);
    }
    struct KT { int k; };
    __device__ __forceinline__ KT ktile(int k0, int c8) const { return {k0 + c8}; }
    __device__ __forceinline__ const bf16_t* addr_kt(const Row& r, const KT& t) const { return addr(r, t.k); }
};

// ---- epilogues -------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float4 fl_add4(float4 v, const float* b) {
    const float4 c = *reinterpret_cast<const float4*>(b);
    return make_float4(v.x + c.x, v.y + c.y, v.z + c.z, v.w + c.w);
}
// proj: h = acc + bias as f32 (the residual of the position embedding) and as bf16 (the first conv's operand)
struct EpiFlowProj {
    float* h; bf16_t* hb; const float* bias;
    __device__ __forceinline__ void operator()(int m, int n, float4 v) const {
        v = fl_add4(v, bias + n);
        *reinterpret_cast<float4*>(h + (long)m * FL_DIM + n) = v;
        *reinterpret_cast<uint2*>(hb + (long)m * FL_DIM + n) = pack_bf16x4(v);
    }
};
// first conv: bf16(mish(acc + bias)) into the group's 64 columns
struct EpiFlowMishBf16 {
    bf16_t* out; const float* bias; int col0;
    __device__ __forceinline__ EpiFlowMishBf16 for_group(int grp) const { EpiFlowMishBf16 e = *this; e.col0 = grp * FL_GROUP; return e; }
    __device__ __forceinline__ void operator()(int m, int n, float4 v) const {
        v = fl_add4(v, bias + col0 + n);
        v = make_float4(fl_mish(v.x), fl_mish(v.y), fl_mish(v.z), fl_mish(v.w));
        *reinterpret_cast<uint2*>(out + (long)m * FL_DIM + col0 + n) = pack_bf16x4(v);
    }
};
// second conv: x = h + mish(acc + bias), the start of the f32 residual stream (DiT.swift:375-376)
struct EpiFlowMishAdd {
    float* x; const float* h; const float* bias; int col0;
    __device__ __forceinline__ EpiFlowMishAdd for_group(int grp) const { EpiFlowMishAdd e = *this; e.col0 = grp * FL_GROUP; return e; }
    __device__ __forceinline__ void operator()(int m, int n, float4 v) const {
        v = fl_add4(v, bias + col0 + n);
        const float4 r = *reinterpret_cast<const float4*>(h + (long)m * FL_DIM + col0 + n);
        v = make_float4(r.x + fl_mish(v.x), r.y + fl_mish(v.y), r.z + fl_mish(v.z), r.w + fl_mish(v.w));
        *reinterpret_cast<float4*>(x + (long)m * FL_DIM + col0 + n) = v;
    }
};
// q|k|v: acc + bias, RoPE on features 0 .. 63 of q and of k (head 0 only: DiT.swift:161-171), traditional pairs (2 i, 2 i + 1), -> bf16
struct EpiFlowQkvRope {
    bf16_t* out; const float* bias; const int* pos; const float *cs, *sn;
    __device__ __forceinline__ void operator()(int m, int n, float4 v) const {
        v = fl_add4(v, bias + n);
        if (n < 2 * FL_DIM && (n & (FL_DIM - 1)) < FL_HD) {
            const int i = (n & (FL_DIM - 1)) >> 1;
            const float* c = cs + (long)pos[m] * (FL_HD / 2) + i;
            const float* s = sn + (long)pos[m] * (FL_HD / 2) + i;
            v = make_float4(v.x * c[0] - v.y * s[0], v.x * s[0] + v.y * c[0], v.z * c[1] - v.w * s[1], v.z * s[1] + v.w * c[1]);
        }
        *reinterpret_cast<uint2*>(out + (long)m * (3 * FL_DIM) + n) = pack_bf16x4(v);
    }
};
// to_out and ff.ff.2: x += gate[n] (acc + bias[n]) on the f32 stream (DiT.swift:256, :265)
struct EpiFlowGate {
    float* x; const float *gate, *bias;
    __device__ __forceinline__ void operator()(int m, int n, float4 v) const {
        v = fl_add4(v, bias + n);
        const float4 g = *reinterpret_cast<const float4*>(gate + n);
        float4 r = *reinterpret_cast<const float4*>(x + (long)m * FL_DIM + n);
        r = make_float4(r.x + g.x * v.x, r.y + g.y * v.y, r.z + g.z * v.z, r.w + g.w * v.w);
        *reinterpret_cast<float4*>(x + (long)m * FL_DIM + n) = r;
    }
};
// ff.ff.0.0: bf16(gelu_tanh(acc + bias))
struct EpiFlowGelu {
    bf16_t* out; const float* bias;
    __device__ __forceinline__ void operator()(int m, int n, float4 v) const {
        v = fl_add4(v, bias + n);
        v = make_float4(fl_gelu_tanh(v.x), fl_gelu_tanh(v.y), fl_gelu_tanh(v.z), fl_gelu_tanh(v.w));
        *reinterpret_cast<uint2*>(out + (long)m * FL_FF + n) = pack_bf16x4(v);
    }
};

// =====================================================================================================================================
// loader (host only)
// =====================================================================================================================================
void flow_schedule(int n_steps, float* t) {
    for (int i = 0; i <= n_steps; ++i) t[i] = 1.0f - cosf((float)i / (float)n_steps * 0.5f * 3.14159265358979323846f);
}

namespace {
const char* const WHO = "flow decoder";
[[noreturn]] void refuse(int code, const std::string& m) { throw WeightLoadError(code, std::string(WHO) + ": " + m); }
std::string shape_str(const std::vector<int64_t>& s) {
    std::string o = "[";
    for (size_t i = 0; i < s.size(); ++i) o += (i ? ", " : "") + std::to_string(s[i]);
    return o + "]";
}
struct QSpec { std::string stem; int N, K; };
std::vector<QSpec> flow_quantised(int depth) {
    const std::string D = "decoder.";
    std::vector<QSpec> q = {{D + "time_embed.time_mlp.0", FL_DIM, FL_FREQ}, {D + "time_embed.time_mlp.2", FL_DIM, FL_DIM},
                            {D + "input_embed.proj", FL_DIM, FL_IN}, {D + "norm_out.linear", 2 * FL_DIM, FL_DIM}};
    for (int i = 0; i < depth; ++i) {
        const std::string b = D + "transformer_blocks." + std::to_string(i) + ".";
        q.push_back({b + "attn_norm.linear", 6 * FL_DIM, FL_DIM});
        for (const char* n : {"attn.to_q", "attn.to_k", "attn.to_v", "attn.to_out.0"}) q.push_back({b + n, FL_DIM, FL_DIM});
        q.push_back({b + "ff.ff.0.0", FL_FF, FL_DIM});
        q.push_back({b + "ff.ff.2", FL_DIM, FL_FF});
    }
    return q;
}
}  // namespace

FlowWeights flow_load_weights(const std::string& dir) {
    std::unique_ptr<SafeTensorsDir> st;
    try { st = std::make_unique<SafeTensorsDir>(dir, "flow.safetensors"); }
    catch (const std::exception& ex) { refuse(QASR_ERR_IO, ex.what()); }
    const auto& E = st->entries;
    FlowWeights fw;
    const std::string D = "decoder.";
    while (fw.depth <= FL_MAX_DEPTH && E.count(D + "transformer_blocks." + std::to_string(fw.depth) + ".attn.to_q.weight")) ++fw.depth;
    if (fw.depth < 1 || fw.depth > FL_MAX_DEPTH) refuse(QASR_ERR_IO, "no key " + D + "transformer_blocks.0.attn.to_q.weight (depth 1.." + std::to_string(FL_MAX_DEPTH) + ")");
    {   // bits and group from the first quantised Linear, as stored (K = 256)
        const std::string stem = D + "time_embed.time_mlp.0";
        auto w = E.find(stem + ".weight"), s = E.find(stem + ".scales");
        if (w == E.end()) refuse(QASR_ERR_IO, "missing key " + stem + ".weight");
        if (s == E.end()) refuse(QASR_ERR_IO, "missing key " + stem + ".scales");
        if (w->second.shape.size() != 2 || s->second.shape.size() != 2 || s->second.shape[1] != FL_FREQ / FL_GROUP)
            refuse(QASR_ERR_INVALID, "key " + stem + ".scales has shape " + shape_str(s->second.shape) + ": the group size must be 64");
        fw.bits = (int)(w->second.shape[1] * 32 / FL_FREQ);
        if ((fw.bits != 4 && fw.bits != 8) || w->second.shape[1] * 32 != (int64_t)FL_FREQ * fw.bits)
            refuse(QASR_ERR_INVALID, "key " + stem + ".weight has shape " + shape_str(w->second.shape) + ": 4 or 8 bits");
    }
    {
        auto e = E.find("input_embedding.weight");
        if (e == E.end()) refuse(QASR_ERR_IO, "missing key input_embedding.weight");
        if (e->second.shape.size() != 2 || e->second.shape[0] < 1 || e->second.shape[1] != FL_MEL)
            refuse(QASR_ERR_INVALID, "key input_embedding.weight has shape " + shape_str(e->second.shape) + ", expected [vocab, 80]");
        fw.vocab = (int)e->second.shape[0];
    }
    std::vector<std::pair<std::string, std::vector<int64_t>>> shapes = {
        {"input_embedding.weight", {fw.vocab, FL_MEL}},
        {"spk_embed_affine_layer.weight", {FL_MEL, FL_SPK}}, {"spk_embed_affine_layer.bias", {FL_MEL}},
        {"pre_lookahead_layer.conv1.weight", {FL_DIM, FL_LOOK_K, FL_MEL}}, {"pre_lookahead_layer.conv1.bias", {FL_DIM}},
        {"pre_lookahead_layer.conv2.weight", {FL_MEL, FL_LOOK2_K, FL_DIM}}, {"pre_lookahead_layer.conv2.bias", {FL_MEL}},
        {D + "input_embed.conv_pos_embed.conv1.0.weight", {FL_DIM, FL_CONV_K, FL_GROUP}}, {D + "input_embed.conv_pos_embed.conv1.0.bias", {FL_DIM}},
        {D + "input_embed.conv_pos_embed.conv2.0.weight", {FL_DIM, FL_CONV_K, FL_GROUP}}, {D + "input_embed.conv_pos_embed.conv2.0.bias", {FL_DIM}},
        {D + "proj_out.weight", {FL_MEL, FL_DIM}}, {D + "proj_out.bias", {FL_MEL}}};
    const std::vector<QSpec> qs = flow_quantised(fw.depth);
    std::set<std::string> known;
    for (const QSpec& q : qs) {
        shapes.push_back({q.stem + ".scales", {q.N, q.K / FL_GROUP}});
        shapes.push_back({q.stem + ".biases", {q.N, q.K / FL_GROUP}});
        shapes.push_back({q.stem + ".bias", {q.N}});
        known.insert(q.stem + ".weight");
    }
    for (const auto& s : shapes) known.insert(s.first);
    for (const auto& kv : E)
        if (!known.count(kv.first)) refuse(QASR_ERR_INVALID, "unexpected key " + kv.first);
    fw.f = load_checked_f32(*st, WHO, shapes, false);
    for (const QSpec& q : qs) {
        const std::string key = q.stem + ".weight";
        auto e = E.find(key);
        if (e == E.end()) refuse(QASR_ERR_IO, "missing key " + key);
        const std::vector<int64_t> want = {q.N, (int64_t)q.K * fw.bits / 32};
        if (e->second.dtype != "U32") refuse(QASR_ERR_INVALID, "key " + key + " has dtype " + e->second.dtype + ", expected U32 (a float checkpoint is not served)");
        if (e->second.shape != want) refuse(QASR_ERR_INVALID, "key " + key + " has shape " + shape_str(e->second.shape) + ", expected " + shape_str(want));
        std::vector<uint32_t> w(e->second.numel());
        std::memcpy(w.data(), e->second.data, w.size() * sizeof(uint32_t));
        fw.f.disk_bytes += w.size() * sizeof(uint32_t);
        fw.packed.emplace(key, std::move(w));
    }
    return fw;
}

// =====================================================================================================================================
// host object
// =====================================================================================================================================
namespace {
struct Pack {
    std::vector<bf16_t> w;
    std::vector<uint32_t> q;
    std::vector<float> f;
    size_t put_f(const std::vector<float>& v) {
        const size_t o = f.size();
        f.insert(f.end(), v.begin(), v.end());
        while (f.size() % 4) f.push_back(0.0f);            // float4 reads start at multiples of 16 bytes
        return o;
    }
    size_t put_w(const std::vector<float>& v) {
        const size_t o = w.size();
        for (float x : v) w.push_back(f32_to_bf16_host(x));
        while (w.size() % 8) w.push_back(0);
        return o;
    }
};
}  // namespace

FlowCosyVoice::FlowCosyVoice(int device, const FlowWeights& fw, long max_frames, hipStream_t work)
    : device_(device), depth_(fw.depth), bits_(fw.bits), vocab_(fw.vocab), max_frames_(max_frames) {
    Pack b;
    const auto& T = fw.f.t;
    auto vec = [&](const std::string& k) -> const std::vector<float>& { return T.at(k); };
    // w[n][k] = Float(scale q + bias) of a packed Linear, as the bf16 image is rounded from
    auto dequant = [&](const std::string& stem, int N, int K, std::vector<float>& out) {
        const std::vector<uint32_t>& wq = fw.packed.at(stem + ".weight");
        const std::vector<float>&s = vec(stem + ".scales"), &z = vec(stem + ".biases");
        const int per = 32 / bits_, wpr = K / per, gpr = K / FL_GROUP;
        const uint32_t mask = (1u << bits_) - 1u;
        for (int n = 0; n < N; ++n)
            for (int k = 0; k < K; ++k) {
                const uint32_t q = (wq[(size_t)n * wpr + k / per] >> ((k % per) * bits_)) & mask;
                out.push_back((float)((double)s[(size_t)n * gpr + k / FL_GROUP] * (double)q + (double)z[(size_t)n * gpr + k / FL_GROUP]));
            }
    };
    auto dense = [&](const std::vector<std::string>& stems, int N, int K) {
        Dense d;
        std::vector<float> w, bias;
        for (const std::string& s : stems) {
            dequant(s, N, K, w);
            bias.insert(bias.end(), vec(s + ".bias").begin(), vec(s + ".bias").end());
        }
        d.w = b.put_w(w);
        d.bias = b.put_f(bias);
        d.N = N * (int)stems.size();
        d.K = K;
        return d;
    };
    auto packed = [&](const std::string& stem, int N, int K) {
        QLin l;
        const std::vector<uint32_t>& wq = fw.packed.at(stem + ".weight");
        l.w = b.q.size();
        b.q.insert(b.q.end(), wq.begin(), wq.end());
        l.s = b.put_f(vec(stem + ".scales"));
        l.b = b.put_f(vec(stem + ".biases"));
        l.bias = b.put_f(vec(stem + ".bias"));
        l.N = N;
        l.K = K;
        return l;
    };
    const std::string D = "decoder.";
    time1_ = packed(D + "time_embed.time_mlp.0", FL_DIM, FL_FREQ);
    time2_ = packed(D + "time_embed.time_mlp.2", FL_DIM, FL_DIM);
    norm_out_ = packed(D + "norm_out.linear", 2 * FL_DIM, FL_DIM);
    proj_ = dense({D + "input_embed.proj"}, FL_DIM, FL_IN);
    for (int i = 0; i < 2; ++i) {
        const std::string p = D + "input_embed.conv_pos_embed.conv" + std::to_string(i + 1) + ".0";
        conv_[i].w = b.put_w(vec(p + ".weight"));           // [1024][31][64]: row n of a group is K = 1984 contiguous values, tap-major
        conv_[i].bias = b.put_f(vec(p + ".bias"));
        conv_[i].N = FL_DIM;
        conv_[i].K = FL_CONV_K * FL_GROUP;
    }
    out_.w = b.put_w(vec(D + "proj_out.weight"));
    out_.bias = b.put_f(vec(D + "proj_out.bias"));
    out_.N = FL_MEL;
    out_.K = FL_DIM;
    blocks_.resize(depth_);
    for (int i = 0; i < depth_; ++i) {
        const std::string p = D + "transformer_blocks." + std::to_string(i) + ".";
        Block& k = blocks_[i];
        k.ada = packed(p + "attn_norm.linear", 6 * FL_DIM, FL_DIM);
        k.qkv = dense({p + "attn.to_q", p + "attn.to_k", p + "attn.to_v"}, FL_DIM, FL_DIM);
        k.o = dense({p + "attn.to_out.0"}, FL_DIM, FL_DIM);
        k.ff1 = dense({p + "ff.ff.0.0"}, FL_FF, FL_DIM);
        k.ff2 = dense({p + "ff.ff.2"}, FL_DIM, FL_FF);
    }
    emb_ = b.put_f(vec("input_embedding.weight"));
    look1_w_ = b.put_f(vec("pre_lookahead_layer.conv1.weight"));
    look1_b_ = b.put_f(vec("pre_lookahead_layer.conv1.bias"));
    look2_w_ = b.put_f(vec("pre_lookahead_layer.conv2.weight"));
    look2_b_ = b.put_f(vec("pre_lookahead_layer.conv2.bias"));
    h_spk_w_ = vec("spk_embed_affine_layer.weight");
    h_spk_b_ = vec("spk_embed_affine_layer.bias");
    {   // RoPE, traditional, base 10000, dims 64 (DiT.swift:404-405): angle = position * 10000^(-i / 32), Float of the f64 value
        std::vector<float> cs((size_t)max_frames * (FL_HD / 2)), sn(cs.size());
        for (long p = 0; p < max_frames; ++p)
            for (int i = 0; i < FL_HD / 2; ++i) {
                const double a = (double)p * std::pow(10000.0, -(double)i / (double)(FL_HD / 2));
                cs[(size_t)p * (FL_HD / 2) + i] = (float)std::cos(a);
                sn[(size_t)p * (FL_HD / 2) + i] = (float)std::sin(a);
            }
        rope_cos_ = b.put_f(cs);
        rope_sin_ = b.put_f(sn);
    }
    QASR_HIP(hipSetDevice(device_));
    QASR_HIP(hipStreamCreateWithFlags(&own_, hipStreamNonBlocking));
    work_ = work ? work : own_;
    auto up = [&](DevBuf& d, const void* src, size_t bytes) {
        d.alloc(bytes);
        if (bytes) QASR_HIP(hipMemcpy(d.p, src, bytes, hipMemcpyHostToDevice));
    };
    param_bytes_ = fw.f.disk_bytes;
    up(d_w_, b.w.data(), b.w.size() * sizeof(bf16_t));
    up(d_q_, b.q.data(), b.q.size() * sizeof(uint32_t));
    up(d_f_, b.f.data(), b.f.size() * sizeof(float));
    const size_t S = (size_t)max_frames, R = 2 * S, F4 = sizeof(float), H2 = sizeof(bf16_t);
    mod_stride_ = (size_t)depth_ * 6 * FL_DIM + 2 * FL_DIM;
    d_cu_.alloc((2 * FL_MAX_CLIPS + 1) * sizeof(int));
    d_pos_.alloc(R * sizeof(int));
    d_clip_.alloc(S * sizeof(int));
    d_seed_.alloc(FL_MAX_CLIPS * (sizeof(unsigned long long) + F4));
    d_t_.alloc((FL_MAX_STEPS + 1) * F4);
    d_sin_.alloc((size_t)FL_MAX_STEPS * FL_FREQ * F4);
    d_emb_.alloc((size_t)FL_MAX_STEPS * FL_DIM * F4 * 2);
    d_mod_.alloc((size_t)FL_MAX_STEPS * mod_stride_ * F4);
    d_mod1_.alloc(mod_stride_ * F4);
    d_x_.alloc(S * FL_MEL * F4);
    d_xb_.alloc(S * FL_MEL * H2);
    d_condb_.alloc(S * FL_MEL * H2);
    d_mub_.alloc(S * FL_MEL * H2);
    d_spkb_.alloc((size_t)FL_MAX_CLIPS * FL_MEL * H2);
    d_stage_.alloc((2 * S + FL_MAX_CLIPS) * FL_MEL * F4);
    d_h0_.alloc(R * FL_DIM * F4);
    d_xs_.alloc(R * FL_DIM * F4);
    d_a_.alloc(R * FL_DIM * H2);
    d_attn_.alloc(R * FL_DIM * H2);
    d_qkv_.alloc(R * 3 * FL_DIM * H2);
    d_u_.alloc(R * FL_FF * H2);
    d_v_.alloc(R * FL_MEL * F4);
    d_tok_.alloc((S / 2 + 1) * sizeof(int));
    d_look_.alloc((S / 2 + 1) * FL_DIM * F4);
}

FlowCosyVoice::~FlowCosyVoice() {
    if (work_) (void)hipStreamSynchronize(work_);
    for (auto& e : ev_) if (e) (void)hipEventDestroy(e);
    if (own_) (void)hipStreamDestroy(own_);
}

void FlowCosyVoice::unload() {
    if (!loaded_) return;
    QASR_HIP(hipSetDevice(device_));
    QASR_HIP(hipStreamSynchronize(work_));
    for (DevBuf* b : {&d_w_, &d_q_, &d_f_, &d_cu_, &d_pos_, &d_clip_, &d_seed_, &d_t_, &d_sin_, &d_emb_, &d_mod_, &d_mod1_, &d_x_, &d_xb_, &d_condb_, &d_mub_,
                      &d_spkb_, &d_stage_, &d_h0_, &d_xs_, &d_a_, &d_attn_, &d_qkv_, &d_u_, &d_v_, &d_tok_, &d_look_})
        b->release();
    loaded_ = false;
    table_steps_ = 0;
}

void FlowCosyVoice::check_loaded() const {
    if (!loaded_) throw NotLoaded("flow decoder: model unloaded");
}

// ---- stage entries -------------------------------------------------------------------------------------------------------------------
void FlowCosyVoice::spks(const float* emb, float* out) const {
    check_loaded();
    if (!emb) { for (int c = 0; c < FL_MEL; ++c) out[c] = 0.0f; return; }        // a missing speaker is 80 zeros (DiT.swift:357-362)
    float ss = 0.0f;                                                               // FlowMatching.swift:332-336
    for (int i = 0; i < FL_SPK; ++i) ss += emb[i] * emb[i];
    const float norm = sqrtf(ss) + 1e-8f;
    for (int c = 0; c < FL_MEL; ++c) {
        float acc = 0.0f;
        for (int i = 0; i < FL_SPK; ++i) acc += h_spk_w_[(size_t)c * FL_SPK + i] * (emb[i] / norm);
        out[c] = acc + h_spk_b_[c];
    }
}

void FlowCosyVoice::mu(const int32_t* tokens, long n, float* out) {
    check_loaded();
    if (n < 1 || 2 * n > max_frames_) throw std::invalid_argument("flow decoder: a clip holds 1.." + std::to_string(max_frames_ / 2) + " tokens (max_frames / 2)");
    for (long i = 0; i < n; ++i)
        if (tokens[i] < 0 || tokens[i] >= vocab_)
            throw std::invalid_argument("flow decoder: token " + std::to_string(i) + " is " + std::to_string(tokens[i]) + ", outside [0, " + std::to_string(vocab_) + ")");
    QASR_HIP(hipSetDevice(device_));
    QASR_HIP(hipStreamSynchronize(work_));
    QASR_HIP(hipMemcpy(d_tok_.p, tokens, (size_t)n * sizeof(int), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(fl_look1_kernel, dim3((unsigned)n), dim3(256), 0, work_, d_tok_.as<int>(), (int)n, F(emb_), F(look1_w_), F(look1_b_), d_look_.as<float>());
    hipLaunchKernelGGL(fl_look2_kernel, dim3((unsigned)cdiv(n * FL_MEL, 4)), dim3(256), 0, work_, d_look_.as<float>(), (int)n, F(look2_w_), F(look2_b_),
                       d_stage_.as<float>());
    QASR_HIP(hipGetLastError());
    QASR_HIP(hipMemcpyAsync(out, d_stage_.p, (size_t)2 * n * FL_MEL * sizeof(float), hipMemcpyDeviceToHost, work_));
    QASR_HIP(hipStreamSynchronize(work_));
}

void FlowCosyVoice::qgemv(const QLin& l, const float* x, int rows, long ldx, float* out, float* out_silu, long ldo) {
    hipLaunchKernelGGL(fl_qgemv_kernel, dim3((unsigned)cdiv(l.N, 4), (unsigned)rows), dim3(256), 0, work_, d_q_.as<uint32_t>() + l.w, F(l.s), F(l.b), F(l.bias),
                       l.N, l.K, bits_, x, ldx, out, out_silu, ldo);
}

// table[row] = [depth][shift | scale | gate | shift | scale | gate] then norm_out's [scale | shift], from the time steps d_t[rows]
void FlowCosyVoice::modulation(const float* d_t, int rows, float* table) {
    float* hid = d_emb_.as<float>();
    float* act = hid + (size_t)FL_MAX_STEPS * FL_DIM;
    hipLaunchKernelGGL(fl_sinusoid_kernel, dim3((unsigned)rows), dim3(FL_FREQ / 2), 0, work_, d_t, rows, d_sin_.as<float>());
    qgemv(time1_, d_sin_.as<float>(), rows, FL_FREQ, nullptr, hid, FL_DIM);                 // SiLU(linear1)
    qgemv(time2_, hid, rows, FL_DIM, nullptr, act, FL_DIM);                                 // SiLU(emb): every AdaLN linear reads it
    for (int i = 0; i < depth_; ++i) qgemv(blocks_[i].ada, act, rows, FL_DIM, table + (size_t)i * 6 * FL_DIM, nullptr, (long)mod_stride_);
    qgemv(norm_out_, act, rows, FL_DIM, table + (size_t)depth_ * 6 * FL_DIM, nullptr, (long)mod_stride_);
    QASR_HIP(hipGetLastError());
}

// ---- a pass --------------------------------------------------------------------------------------------------------------------------
void FlowCosyVoice::set_pass(const FlowClip* c, int n, bool doubled) {
    QASR_HIP(hipSetDevice(device_));
    QASR_HIP(hipStreamSynchronize(work_));
    long S = 0;
    max_len_ = 0;
    for (int i = 0; i < n; ++i) { S += c[i].T; max_len_ = std::max<int>(max_len_, (int)c[i].T); }
    if (n > FL_MAX_CLIPS || S > max_frames_) throw std::length_error("flow decoder: a pass exceeds its buffers");
    src_rows_ = cond_rows_ = S;
    rows_ = doubled ? 2 * S : S;
    n_seq_ = doubled ? 2 * n : n;
    std::vector<int> cu(n_seq_ + 1, 0), pos((size_t)rows_), clip((size_t)S);
    for (int q = 0; q < n_seq_; ++q) {
        const long T = c[q % n].T;
        cu[q + 1] = cu[q] + (int)T;
        for (long t = 0; t < T; ++t) pos[(size_t)cu[q] + t] = (int)t;
        if (q < n) for (long t = 0; t < T; ++t) clip[(size_t)cu[q] + t] = q;
    }
    QASR_HIP(hipMemcpy(d_cu_.p, cu.data(), cu.size() * sizeof(int), hipMemcpyHostToDevice));
    QASR_HIP(hipMemcpy(d_pos_.p, pos.data(), pos.size() * sizeof(int), hipMemcpyHostToDevice));
    QASR_HIP(hipMemcpy(d_clip_.p, clip.data(), clip.size() * sizeof(int), hipMemcpyHostToDevice));
    // mu | cond | spks of the pass, f32 in the staging buffer, then one cast each
    std::vector<float> st((size_t)(2 * S + n) * FL_MEL, 0.0f);
    for (int i = 0; i < n; ++i) {
        const size_t r0 = (size_t)cu[i] * FL_MEL, len = (size_t)c[i].T * FL_MEL;
        std::memcpy(&st[r0], c[i].mu, len * sizeof(float));
        if (c[i].cond) std::memcpy(&st[(size_t)S * FL_MEL + r0], c[i].cond, len * sizeof(float));
        if (c[i].spks) std::memcpy(&st[(size_t)(2 * S + i) * FL_MEL], c[i].spks, FL_MEL * sizeof(float));
    }
    QASR_HIP(hipMemcpy(d_stage_.p, st.data(), st.size() * sizeof(float), hipMemcpyHostToDevice));
    auto cast = [&](const float* src, bf16_t* dst, long cnt) {
        hipLaunchKernelGGL(fl_cast_kernel, dim3((unsigned)cdiv(cnt, 256)), dim3(256), 0, work_, src, dst, cnt);
    };
    cast(d_stage_.as<float>(), d_mub_.as<bf16_t>(), S * FL_MEL);
    cast(d_stage_.as<float>() + S * FL_MEL, d_condb_.as<bf16_t>(), S * FL_MEL);
    cast(d_stage_.as<float>() + 2 * S * FL_MEL, d_spkb_.as<bf16_t>(), (long)n * FL_MEL);
    bool any_x = false;
    for (int i = 0; i < n; ++i) any_x = any_x || !c[i].noise;
    if (any_x) {
        std::vector<float> hx((size_t)S * FL_MEL, 0.0f);
        for (int i = 0; i < n; ++i)
            if (!c[i].noise) std::memcpy(&hx[(size_t)cu[i] * FL_MEL], c[i].x, (size_t)c[i].T * FL_MEL * sizeof(float));
        QASR_HIP(hipMemcpy(d_x_.p, hx.data(), hx.size() * sizeof(float), hipMemcpyHostToDevice));
        cast(d_x_.as<float>(), d_xb_.as<bf16_t>(), S * FL_MEL);
    } else {
        std::vector<unsigned long long> seeds((size_t)n);
        std::vector<float> temps((size_t)n);
        for (int i = 0; i < n; ++i) { seeds[i] = c[i].seed; temps[i] = c[i].temperature; }
        float* d_temp = reinterpret_cast<float*>(d_seed_.as<unsigned long long>() + FL_MAX_CLIPS);
        QASR_HIP(hipMemcpy(d_seed_.p, seeds.data(), seeds.size() * sizeof(unsigned long long), hipMemcpyHostToDevice));
        QASR_HIP(hipMemcpy(d_temp, temps.data(), temps.size() * sizeof(float), hipMemcpyHostToDevice));
        hipLaunchKernelGGL(fl_noise_kernel, dim3((unsigned)cdiv(S * FL_MEL, 256)), dim3(256), 0, work_, d_cu_.as<int>(), n, d_seed_.as<unsigned long long>(), d_temp,
                           S * FL_MEL, d_x_.as<float>(), d_xb_.as<bf16_t>());
    }
    QASR_HIP(hipGetLastError());
}

// one DiT forward on the rows of the pass (DiT.swift:430-473): d_xb_, d_condb_, d_mub_, d_spkb_ and the modulation row `mod` -> d_v_
void FlowCosyVoice::forward(const float* mod) {
    const int R = (int)rows_;
    hipStream_t s = work_;
    auto mark = [&](int stage) {
        if ((size_t)ev_used_ == ev_.size()) { hipEvent_t e; QASR_HIP(hipEventCreate(&e)); ev_.push_back(e); }
        QASR_HIP(hipEventRecord(ev_[ev_used_], s));
        ev_used_++;
        (void)stage;
    };
    float *h0 = d_h0_.as<float>(), *xs = d_xs_.as<float>();
    bf16_t *a = d_a_.as<bf16_t>(), *attn = d_attn_.as<bf16_t>(), *qkv = d_qkv_.as<bf16_t>(), *u = d_u_.as<bf16_t>();
    const int* pos = d_pos_.as<int>();
    auto ln = [&](const float* scale, const float* shift) {
        hipLaunchKernelGGL(fl_ln_mod_kernel, dim3((unsigned)cdiv(R, 4)), dim3(256), 0, s, xs, scale, shift, a, R);
    };
    mark(-1);
    // input_embed (DiT.swift:352-378)
    gemm_nt(AFlowIn{d_xb_.as<bf16_t>(), d_condb_.as<bf16_t>(), d_mub_.as<bf16_t>(), d_spkb_.as<bf16_t>(), d_clip_.as<int>(), (int)src_rows_, (int)cond_rows_, R},
            W(proj_.w), FL_IN, R, FL_DIM, FL_IN, EpiFlowProj{h0, a, F(proj_.bias)}, s);
    const long gs = (long)FL_GROUP * conv_[0].K;
    gemm_nt_groups(AFlowConv{a, pos, 0, R}, W(conv_[0].w), conv_[0].K, gs, FL_CONV_GROUPS, R, FL_GROUP, conv_[0].K, EpiFlowMishBf16{attn, F(conv_[0].bias), 0}, s);
    gemm_nt_groups(AFlowConv{attn, pos, 0, R}, W(conv_[1].w), conv_[1].K, gs, FL_CONV_GROUPS, R, FL_GROUP, conv_[1].K, EpiFlowMishAdd{xs, h0, F(conv_[1].bias), 0}, s);
    mark(1);
    for (int i = 0; i < depth_; ++i) {                     // DiT.swift:241-267; chunks: shift, scale, gate (attention), shift, scale, gate (MLP)
        const Block& b = blocks_[i];
        const float* m = mod + (size_t)i * 6 * FL_DIM;
        ln(m + FL_DIM, m);
        gemm_nt(ADense{a, FL_DIM, R, FL_DIM}, W(b.qkv.w), FL_DIM, R, 3 * FL_DIM, FL_DIM, EpiFlowQkvRope{qkv, F(b.qkv.bias), pos, F(rope_cos_), F(rope_sin_)}, s);
        mha_attention_launch(qkv, d_cu_.as<int>(), n_seq_, max_len_, FL_HEADS, FL_HD, attn, s);
        gemm_nt(ADense{attn, FL_DIM, R, FL_DIM}, W(b.o.w), FL_DIM, R, FL_DIM, FL_DIM, EpiFlowGate{xs, m + 2 * FL_DIM, F(b.o.bias)}, s);
        ln(m + 4 * FL_DIM, m + 3 * FL_DIM);
        gemm_nt(ADense{a, FL_DIM, R, FL_DIM}, W(b.ff1.w), FL_DIM, R, FL_FF, FL_DIM, EpiFlowGelu{u, F(b.ff1.bias)}, s);
        gemm_nt(ADense{u, FL_FF, R, FL_FF}, W(b.ff2.w), FL_FF, R, FL_DIM, FL_FF, EpiFlowGate{xs, m + 5 * FL_DIM, F(b.ff2.bias)}, s);
    }
    mark(2);
    const float* fin = mod + (size_t)depth_ * 6 * FL_DIM;  // norm_out: scale then shift (DiT.swift:121-125)
    ln(fin, fin + FL_DIM);
    gemm_nt(ADense{a, FL_DIM, R, FL_DIM}, W(out_.w), FL_DIM, R, FL_MEL, FL_DIM, EpiBiasF32{d_v_.as<float>(), FL_MEL, F(out_.bias)}, s);
    mark(3);
    QASR_HIP(hipGetLastError());
}

void FlowCosyVoice::velocity(const float* x, const float* mu, const float* spks, const float* cond, long T, float t, float* v) {
    check_loaded();
    if (T < 1 || T > max_frames_) throw std::invalid_argument("flow decoder: a clip holds 1.." + std::to_string(max_frames_) + " frames (max_frames)");
    for (float& q : timing_) q = 0.0f;
    FlowClip c;
    c.T = T; c.x = x; c.mu = mu; c.spks = spks; c.cond = cond;
    set_pass(&c, 1, false);
    QASR_HIP(hipMemcpy(d_t_.p, &t, sizeof(float), hipMemcpyHostToDevice));
    modulation(d_t_.as<float>(), 1, d_mod1_.as<float>());
    ev_used_ = 0;
    forward(d_mod1_.as<float>());
    QASR_HIP(hipMemcpyAsync(v, d_v_.p, (size_t)T * FL_MEL * sizeof(float), hipMemcpyDeviceToHost, work_));
    QASR_HIP(hipStreamSynchronize(work_));
    QASR_HIP(hipGetLastError());
}

void FlowCosyVoice::pass(const FlowClip* c, int n, int n_steps) {
    set_pass(c, n, true);
    const long S = src_rows_, cnt = S * FL_MEL;
    float tt[FL_MAX_STEPS + 1];
    flow_schedule(n_steps, tt);
    std::vector<int> off(n + 1, 0);
    for (int i = 0; i < n; ++i) off[i + 1] = off[i] + (int)c[i].T;
    for (int i = 0; i < n; ++i)
        if (c[i].z_out)
            QASR_HIP(hipMemcpyAsync(c[i].z_out, d_x_.as<float>() + (size_t)off[i] * FL_MEL, (size_t)c[i].T * FL_MEL * sizeof(float), hipMemcpyDeviceToHost, work_));
    ev_used_ = 0;
    std::vector<int> first(n_steps, 0);
    int ev_table0 = -1;
    if (table_steps_ != n_steps) {                         // the whole modulation table of a solve, once per n_steps
        QASR_HIP(hipStreamSynchronize(work_));
        QASR_HIP(hipMemcpy(d_t_.p, tt, (size_t)n_steps * sizeof(float), hipMemcpyHostToDevice));
        if (ev_.size() < 2) { ev_.resize(2); for (auto& e : ev_) QASR_HIP(hipEventCreate(&e)); }
        QASR_HIP(hipEventRecord(ev_[0], work_));
        modulation(d_t_.as<float>(), n_steps, d_mod_.as<float>());
        QASR_HIP(hipEventRecord(ev_[1], work_));
        ev_table0 = 0;
        ev_used_ = 2;
        table_steps_ = n_steps;
    }
    for (int i = 0; i < n_steps; ++i) {
        first[i] = ev_used_;
        forward(d_mod_.as<float>() + (size_t)i * mod_stride_);
        hipLaunchKernelGGL(fl_euler_kernel, dim3((unsigned)cdiv(cnt, 256)), dim3(256), 0, work_, d_x_.as<float>(), d_xb_.as<bf16_t>(), d_v_.as<float>(),
                           d_v_.as<float>() + cnt, tt[i + 1] - tt[i], FL_CFG, cnt);
        if ((size_t)ev_used_ == ev_.size()) { hipEvent_t e; QASR_HIP(hipEventCreate(&e)); ev_.push_back(e); }
        QASR_HIP(hipEventRecord(ev_[ev_used_++], work_));
    }
    for (int i = 0; i < n; ++i) {
        const size_t r0 = (size_t)off[i] * FL_MEL, len = (size_t)c[i].T * FL_MEL * sizeof(float);
        if (c[i].v_out) {
            QASR_HIP(hipMemcpyAsync(c[i].v_out, d_v_.as<float>() + r0, len, hipMemcpyDeviceToHost, work_));
            QASR_HIP(hipMemcpyAsync(c[i].v_out + (size_t)c[i].T * FL_MEL, d_v_.as<float>() + cnt + r0, len, hipMemcpyDeviceToHost, work_));
        }
        QASR_HIP(hipMemcpyAsync(c[i].mel, d_x_.as<float>() + r0, len, hipMemcpyDeviceToHost, work_));
    }
    QASR_HIP(hipStreamSynchronize(work_));
    QASR_HIP(hipGetLastError());
    float ms = 0;
    if (ev_table0 >= 0) { QASR_HIP(hipEventElapsedTime(&ms, ev_[0], ev_[1])); timing_[0] += ms; }
    for (int i = 0; i < n_steps; ++i)                      // a step's events: start, input_embed, blocks, output, Euler
        for (int k = 0; k < 4; ++k) {
            QASR_HIP(hipEventElapsedTime(&ms, ev_[first[i] + k], ev_[first[i] + k + 1]));
            timing_[1 + k] += ms;
        }
}

void FlowCosyVoice::solve(const std::vector<FlowClip>& clips, int n_steps) {
    check_loaded();
    if (n_steps < 1 || n_steps > FL_MAX_STEPS) throw std::invalid_argument("flow decoder: n_steps in 1.." + std::to_string(FL_MAX_STEPS));
    for (float& t : timing_) t = 0.0f;
    for (size_t i = 0; i < clips.size(); ++i)
        if (clips[i].T < 1 || clips[i].T > max_frames_)
            throw std::invalid_argument("flow decoder: clip " + std::to_string(i) + " holds " + std::to_string(clips[i].T) + " frames, a clip holds 1.." +
                                        std::to_string(max_frames_) + " (max_frames)");
    for (size_t i = 0; i < clips.size();) {                // passes end at clip boundaries
        size_t j = i;
        long total = 0;
        while (j < clips.size() && j - i < (size_t)FL_MAX_CLIPS && total + clips[j].T <= max_frames_) total += clips[j++].T;
        pass(clips.data() + i, (int)(j - i), n_steps);
        i = j;
    }
}

}  // namespace qasr
