// loc_voxcpm.hip -- VoxCPM2's LocEnc and LocDiT (loc_voxcpm.h).  Launches of one MiniCPM layer:
//   q|k|v     vl_gemm_kernel, RMSNorm at the activation load, N = (heads + 2 kv_heads) 128, f32 out
//   attention vl_attention_kernel, one workgroup per (sequence, query head): RoPE at the load of K and of each query, the S <= 32 keys and
//             values of its K/V head in LDS
//   o         vl_gemm_kernel, epilogue x + s y in place
//   gate|up   vl_gemm_kernel, RMSNorm at the load, two weight tiles per wave (gate rows n, up rows ffn + n), epilogue silu(g) u
//   down      vl_gemm_kernel, epilogue x + s y in place
// vl_gemm_kernel is the skinny bf16 GEMM: a workgroup of 8 waves owns 16 output columns and up to 64 rows; the K axis goes in chunks of
// 512, wave w taking k = 64 w .. 64 w + 63 of each chunk (two v_mfma_f32_16x16x32_bf16 per row block and tile), so a weight byte is read
// once per 64 rows, straight from global memory into the B fragment.  The activations of a chunk are rounded to bf16 into LDS.  An output
// is  sum over waves 0..7 in order of (the wave's MFMA chain over the chunks in order): the order depends on nothing but K, so a row's
// bits do not depend on how many rows the launch holds.
#include "loc_voxcpm.h"
#include "gemm.h"
#include "json.h"
#include <cmath>
#include <cstdio>
#include <cstring>

namespace qasr {

// ---- kernels ------------------------------------------------------------------------------------------------------------------------
typedef __attribute__((ext_vector_type(8))) __bf16 vl_bf16x8;   // one operand fragment of v_mfma_f32_16x16x32_bf16
constexpr int VL_GEMM_THREADS = 512, VL_LDA = VL_KC + 8;   // LDS row of a chunk in bf16: 1040 bytes, 16 rows fall on 16 different 16-byte slots

struct VlGemmArgs {
    const float* A; long lda;                  // row m of the launch reads row (m / a_group) a_stride + a_off + m % a_group of A
    int a_group, a_stride, a_off;
    const float* norm_w; float eps;            // norm_w: RMSNorm over K at the load
    const bf16_t* W;                           // [N][K]; SWIGLU: [2 N][K], gate rows then up rows
    const float* bias;                         // [N] or null
    const float* resid; long ldr;              // null, or rows (ldr = 0: one row for every m): out = resid + s v
    float s; int act;                          // act 1: silu
    float* out; long ldo;
    int M, N, K;
};

__device__ __forceinline__ float vl_silu(float v) { return v / (1.0f + expf(-v)); }

template <int MB, bool SWIGLU>
__global__ __launch_bounds__(VL_GEMM_THREADS) void vl_gemm_kernel(VlGemmArgs a) {
    constexpr int NT = SWIGLU ? 2 : 1, ROWS = 16 * MB;
    extern __shared__ __attribute__((aligned(16))) unsigned char vl_lds[];
    __shared__ float rstd[64];
    bf16_t* As = reinterpret_cast<bf16_t*>(vl_lds);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fc = lane >> 4;
    const int n0 = blockIdx.x * 16, m0 = blockIdx.y * ROWS;
    const int rows = min(ROWS, a.M - m0);
    const int nchunk = a.K / VL_KC;
    const bf16_t* wrow[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) wrow[t] = a.W + ((long)t * a.N + n0 + fr) * a.K + wave * 64 + fc * 8;
    uint4 bcur[2][NT], bnext[2][NT];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int t = 0; t < NT; ++t) bcur[s][t] = *reinterpret_cast<const uint4*>(wrow[t] + s * 32);
    __shared__ const float* rowp[64];             // the gathered source rows, resolved once
    if (tid < rows) { const int m = m0 + tid; rowp[tid] = a.A + ((long)(m / a.a_group) * a.a_stride + a.a_off + m % a.a_group) * a.lda; }
    __syncthreads();
    auto src = [&](int r) { return rowp[r]; };
    if (a.norm_w) {                            // rows r = wave, wave + 8, ..: lane-strided squares in k order, then the xor butterfly
        for (int r = wave; r < rows; r += 8) {
            const float* x = src(r);
            float ss = 0.0f;
            for (int k = lane * 4; k < a.K; k += 256) {
                const float4 v = *reinterpret_cast<const float4*>(x + k);
                ss = fmaf(v.x, v.x, ss); ss = fmaf(v.y, v.y, ss); ss = fmaf(v.z, v.z, ss); ss = fmaf(v.w, v.w, ss);
            }
            ss = wave_sum(ss);
            if (lane == 0) rstd[r] = 1.0f / sqrtf(ss / (float)a.K + a.eps);
        }
        __syncthreads();
    }
    f32x4 acc[MB][NT];
#pragma unroll
    for (int i = 0; i < MB; ++i)
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[i][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int c = 0; c < nchunk; ++c) {
        for (int i = tid; i < ROWS * (VL_KC / 4); i += VL_GEMM_THREADS) {
            const int r = i / (VL_KC / 4), k = (i % (VL_KC / 4)) * 4;
            uint2 p = make_uint2(0u, 0u);
            if (r < rows) {
                float4 v = *reinterpret_cast<const float4*>(src(r) + c * VL_KC + k);
                if (a.norm_w) {
                    const float4 w = *reinterpret_cast<const float4*>(a.norm_w + c * VL_KC + k);
                    const float q = rstd[r];
                    v.x = (v.x * q) * w.x; v.y = (v.y * q) * w.y; v.z = (v.z * q) * w.z; v.w = (v.w * q) * w.w;
                }
                p.x = pack_bf16x2(v.x, v.y);
                p.y = pack_bf16x2(v.z, v.w);
            }
            *reinterpret_cast<uint2*>(As + r * VL_LDA + k) = p;
        }
        if (c + 1 < nchunk) {
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int t = 0; t < NT; ++t) bnext[s][t] = *reinterpret_cast<const uint4*>(wrow[t] + (c + 1) * VL_KC + s * 32);
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int i = 0; i < MB; ++i) {
                const vl_bf16x8 af = *reinterpret_cast<const vl_bf16x8*>(As + (i * 16 + fr) * VL_LDA + wave * 64 + s * 32 + fc * 8);
#pragma unroll
                for (int t = 0; t < NT; ++t)
                    acc[i][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, __builtin_bit_cast(vl_bf16x8, bcur[s][t]), acc[i][t], 0, 0, 0);
            }
        __syncthreads();
        if (c + 1 < nchunk) {
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int t = 0; t < NT; ++t) bcur[s][t] = bnext[s][t];
        }
    }
    // the eight waves' partial tiles through LDS (the chunk image is dead after the loop's last barrier), summed in wave order
    f32x4* red = reinterpret_cast<f32x4*>(vl_lds);
#pragma unroll
    for (int i = 0; i < MB; ++i)
#pragma unroll
        for (int t = 0; t < NT; ++t) red[((wave * MB + i) * NT + t) * 64 + lane] = acc[i][t];
    __syncthreads();
    for (int e = tid; e < MB * 64; e += VL_GEMM_THREADS) {
        const int i = e >> 6, l = e & 63, col = n0 + (l & 15);
        f32x4 v[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            v[t] = red[((0 * MB + i) * NT + t) * 64 + l];
            for (int w = 1; w < 8; ++w) {
                const f32x4 p = red[((w * MB + i) * NT + t) * 64 + l];
                v[t][0] += p[0]; v[t][1] += p[1]; v[t][2] += p[2]; v[t][3] += p[3];
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = m0 + i * 16 + (l >> 4) * 4 + r;
            if (m >= a.M) continue;
            float y = v[0][r];
            if constexpr (SWIGLU) {
                y = vl_silu(y) * v[1][r];
            } else {
                if (a.bias) y += a.bias[col];
                if (a.act == 1) y = vl_silu(y);
                if (a.resid) y = a.resid[(long)m * a.ldr + col] + a.s * y;
            }
            a.out[(long)m * a.ldo + col] = y;
        }
    }
}

// ---- the wide pass: the shared 128 x 128 tile of gemm.h on the rows as a bf16 image ------------------------------------------------------
// the gathered rows as the skinny kernel stages them, (x rstd) w rounded to bf16, once per launch: one wave per row, the squares in the same order
__global__ __launch_bounds__(64) void vl_rows_bf16_kernel(const float* __restrict__ A, long lda, int a_group, int a_stride, int a_off, int K,
                                                          const float* __restrict__ norm_w, float eps, bf16_t* __restrict__ out) {
    const long m = blockIdx.x;
    const float* x = A + ((m / a_group) * a_stride + a_off + m % a_group) * lda;
    const int lane = threadIdx.x;
    float q = 1.0f;
    if (norm_w) {
        float ss = 0.0f;
        for (int k = lane * 4; k < K; k += 256) {
            const float4 v = *reinterpret_cast<const float4*>(x + k);
            ss = fmaf(v.x, v.x, ss); ss = fmaf(v.y, v.y, ss); ss = fmaf(v.z, v.z, ss); ss = fmaf(v.w, v.w, ss);
        }
        ss = wave_sum(ss);
        q = 1.0f / sqrtf(ss / (float)K + eps);
    }
    for (int k = lane * 4; k < K; k += 256) {
        float4 v = *reinterpret_cast<const float4*>(x + k);
        if (norm_w) {
            const float4 w = *reinterpret_cast<const float4*>(norm_w + k);
            v.x = (v.x * q) * w.x; v.y = (v.y * q) * w.y; v.z = (v.z * q) * w.z; v.w = (v.w * q) * w.w;
        }
        *reinterpret_cast<uint2*>(out + m * K + k) = make_uint2(pack_bf16x2(v.x, v.y), pack_bf16x2(v.z, v.w));
    }
}

// the skinny kernel's epilogues on the tile's four columns; gate: y = silu(out[m][n]) acc, where out holds the gate product (SwiGLU in two launches)
struct EpiVl {
    const float* bias; const float* resid; long ldr; float s; int act; int gate; float* out; long ldo;
    __device__ __forceinline__ float one(int m, int n, float y) const {
        if (gate) return vl_silu(out[(long)m * ldo + n]) * y;
        if (bias) y += bias[n];
        if (act == 1) y = vl_silu(y);
        if (resid) y = resid[(long)m * ldr + n] + s * y;
        return y;
    }
    __device__ __forceinline__ void operator()(int m, int n, float4 v) const {
        float4 r;
        r.x = one(m, n, v.x); r.y = one(m, n + 1, v.y); r.z = one(m, n + 2, v.z); r.w = one(m, n + 3, v.w);
        *reinterpret_cast<float4*>(out + (long)m * ldo + n) = r;
    }
};

// y[n] = bias[n] + sum_k bf16(x[k]) W[n][k], k in order: the K <= 256 inputs (in_proj, cond_proj); xs holds the row's rounded values
__device__ __forceinline__ float vl_small_dot(const float* xs, const bf16_t* __restrict__ w, int K, float bias) {
    float acc = 0.0f;
    for (int k = 0; k < K; k += 8) {
        const uint4 p = *reinterpret_cast<const uint4*>(w + k);
        acc = fmaf(xs[k + 0], bf16_lo(p.x), acc); acc = fmaf(xs[k + 1], bf16_hi(p.x), acc);
        acc = fmaf(xs[k + 2], bf16_lo(p.y), acc); acc = fmaf(xs[k + 3], bf16_hi(p.y), acc);
        acc = fmaf(xs[k + 4], bf16_lo(p.z), acc); acc = fmaf(xs[k + 5], bf16_hi(p.z), acc);
        acc = fmaf(xs[k + 6], bf16_lo(p.w), acc); acc = fmaf(xs[k + 7], bf16_hi(p.w), acc);
    }
    return acc + bias;
}

// out[row][:] = Linear(x[row][:]), one workgroup per row
__global__ __launch_bounds__(256) void vl_small_linear_kernel(const float* __restrict__ x, int K, const bf16_t* __restrict__ W, const float* __restrict__ bias,
                                                              int N, float* __restrict__ out) {
    __shared__ float xs[256];
    const long row = blockIdx.x;
    for (int k = threadIdx.x; k < K; k += 256) xs[k] = bf16_round(x[row * K + k]);
    __syncthreads();
    for (int n = threadIdx.x; n < N; n += 256) out[row * N + n] = vl_small_dot(xs, W + (long)n * K, K, bias[n]);
}

struct VlAssembleArgs {
    float* h; int H, S;                        // token rows [n_seq][S][H]
    int n_lead, n_mu, has_time, n_cond, P, F;  // n_lead: 1 for LocEnc's special token
    const float* lead;                         // [H]
    const float* mu; long mu_seqs, B;          // [B][n_mu H]; sequences >= mu_seqs take zeros; sequence q reads row q % B of mu, cond and x
    const float* ttok;                         // [H]
    const float* condp;                        // [B][P][H]
    const float* x;                            // [B][P][F], through in_proj here
    const bf16_t* Win; const float* bin;
};

// one workgroup per token row
__global__ __launch_bounds__(256) void vl_assemble_kernel(VlAssembleArgs a) {
    __shared__ float xs[256];
    const long q = blockIdx.x / a.S, b = q % a.B;
    int tok = blockIdx.x % a.S;
    float* out = a.h + (long)blockIdx.x * a.H;
    const int tid = threadIdx.x;
    if (tok < a.n_lead) { for (int n = tid; n < a.H; n += 256) out[n] = a.lead[n]; return; }
    tok -= a.n_lead;
    if (tok < a.n_mu) {
        for (int n = tid; n < a.H; n += 256) out[n] = q < a.mu_seqs ? a.mu[(b * a.n_mu + tok) * a.H + n] : 0.0f;
        return;
    }
    tok -= a.n_mu;
    if (tok < a.has_time) { for (int n = tid; n < a.H; n += 256) out[n] = a.ttok[n]; return; }
    tok -= a.has_time;
    if (tok < a.n_cond) { for (int n = tid; n < a.H; n += 256) out[n] = a.condp[(b * a.P + tok) * a.H + n]; return; }
    tok -= a.n_cond;
    for (int k = tid; k < a.F; k += 256) xs[k] = bf16_round(a.x[(b * a.P + tok) * a.F + k]);
    __syncthreads();
    for (int n = tid; n < a.H; n += 256) out[n] = vl_small_dot(xs, a.Win + (long)n * a.F, a.F, a.bin[n]);
}

// RMSNorm of gathered rows, f32 out: one wave per row, the squares as in vl_gemm_kernel
__global__ __launch_bounds__(64) void vl_norm_rows_kernel(const float* __restrict__ x, int H, int group, int stride, int off, const float* __restrict__ w,
                                                          float eps, float* __restrict__ out) {
    const long m = blockIdx.x;
    const float* xr = x + ((m / group) * stride + off + m % group) * H;
    const int lane = threadIdx.x;
    float ss = 0.0f;
    for (int k = lane * 4; k < H; k += 256) {
        const float4 v = *reinterpret_cast<const float4*>(xr + k);
        ss = fmaf(v.x, v.x, ss); ss = fmaf(v.y, v.y, ss); ss = fmaf(v.z, v.z, ss); ss = fmaf(v.w, v.w, ss);
    }
    ss = wave_sum(ss);
    const float q = 1.0f / sqrtf(ss / (float)H + eps);
    for (int k = lane; k < H; k += 64) out[m * H + k] = (xr[k] * q) * w[k];
}

// softmax(q k^T / sqrt 128) v without a mask.  grid (sequences, query heads), 4 waves; the workgroup holds its K/V head's S <= 32 keys
// (rotated at the load) and values in LDS, a wave takes one token per round.  A score is one lane's fmaf chain over d = 0 .. 127, an
// output element one lane's chain over the keys in order.  Why per query head and not per K/V head: DESIGN.md section 26.2.
__global__ __launch_bounds__(256) void vl_attention_kernel(const float* __restrict__ qkv, int S, int heads, int kv_heads, const float* __restrict__ rcos,
                                                           const float* __restrict__ rsin, float* __restrict__ out) {
    constexpr int D = VL_HEAD_DIM, HALF = D / 2, KP = D + 4;   // key rows 16 bytes apart in the banks: 16-byte reads of 16 lanes do not collide
    __shared__ __attribute__((aligned(16))) float Ks[VL_MAX_S][KP], Vs[VL_MAX_S][D], qs[4][D], ps[4][VL_MAX_S];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int head = blockIdx.y, kvh = head / (heads / kv_heads), ld = (heads + 2 * kv_heads) * D;
    const long row0 = (long)blockIdx.x * S;
    const int koff = heads * D + kvh * D, voff = (heads + kv_heads) * D + kvh * D;
    for (int i = tid; i < S * HALF; i += 256) {
        const int j = i / HALF, d = i % HALF;
        const float* r = qkv + (row0 + j) * ld;
        const float k1 = r[koff + d], k2 = r[koff + HALF + d], c = rcos[j * D + d], sn = rsin[j * D + d];
        Ks[j][d] = k1 * c - k2 * sn;
        Ks[j][HALF + d] = k2 * c + k1 * sn;
        Vs[j][d] = r[voff + d];
        Vs[j][HALF + d] = r[voff + HALF + d];
    }
    __syncthreads();
    const float scale = 1.0f / sqrtf((float)D);
    for (int base = 0; base < S; base += 4) {
        const int i = base + wave;
        const bool valid = i < S;
        if (valid) {
            const float* r = qkv + (row0 + i) * ld + head * D;
            const float q1 = r[lane], q2 = r[HALF + lane], c = rcos[i * D + lane], sn = rsin[i * D + lane];
            qs[wave][lane] = q1 * c - q2 * sn;
            qs[wave][HALF + lane] = q2 * c + q1 * sn;
        }
        __syncthreads();
        if (valid) {
            float sc = -INFINITY;
            if (lane < S) {
                float acc = 0.0f;
#pragma unroll 8
                for (int d = 0; d < D; d += 4) {
                    const float4 q = lds_read_f4(&qs[wave][d]), k = lds_read_f4(&Ks[lane][d]);
                    acc = fmaf(q.x, k.x, acc); acc = fmaf(q.y, k.y, acc); acc = fmaf(q.z, k.z, acc); acc = fmaf(q.w, k.w, acc);
                }
                sc = acc * scale;
            }
            const float mx = wave_max(sc);
            const float e = lane < S ? expf(sc - mx) : 0.0f;
            const float sum = wave_sum(e);
            if (lane < S) ps[wave][lane] = e / sum;
        }
        __syncthreads();
        if (valid) {
            float o1 = 0.0f, o2 = 0.0f;
            for (int j = 0; j < S; ++j) {
                const float p = ps[wave][j];
                o1 = fmaf(p, Vs[j][lane], o1);
                o2 = fmaf(p, Vs[j][HALF + lane], o2);
            }
            float* o = out + (row0 + i) * (long)(heads * D) + head * D;
            o[lane] = o1;
            o[HALF + lane] = o2;
        }
        __syncthreads();
    }
}

// the kernel's launch entry (loc_voxcpm.h): LocVoxcpm::run_stack and qasr_syn_attn_case_probe call this
void vl_attention_launch(const float* qkv, long n_seq, int S, int heads, int kv_heads, const float* rcos, const float* rsin, float* out,
                         hipStream_t s) {
    if (S < 1 || S > VL_MAX_S) throw std::invalid_argument("voxcpm2 local networks: attention serves sequences of 1 .. 32 tokens");
    if (heads < 1 || kv_heads < 1 || heads % kv_heads != 0)
        throw std::invalid_argument("voxcpm2 local networks: heads must be a multiple of kv_heads");
    if (n_seq <= 0) return;
    hipLaunchKernelGGL(vl_attention_kernel, dim3((unsigned)n_seq, (unsigned)heads), dim3(256), 0, s, qkv, S, heads, kv_heads, rcos, rsin, out);
}

// CFG-zero-star and the Euler line for one patch per workgroup (the order: loc_voxcpm.h).  v [2 B][n]: positive rows, then negative rows.
__global__ __launch_bounds__(256) void vl_euler_kernel(const float* __restrict__ v, long B, int n, int n2, const float* __restrict__ cfg, float dt,
                                                       float* __restrict__ x, float* __restrict__ d_out) {
    extern __shared__ __attribute__((aligned(16))) float vl_e[];
    float *pa = vl_e, *pb = vl_e + n2;
    const long b = blockIdx.x;
    const float *pos = v + b * n, *neg = v + (B + b) * n;
    for (int i = threadIdx.x; i < n2; i += 256) {
        const float p = i < n ? pos[i] : 0.0f, q = i < n ? neg[i] : 0.0f;
        pa[i] = __fmul_rn(p, q);
        pb[i] = __fmul_rn(q, q);
    }
    __syncthreads();
    for (int s = n2 / 2; s > 0; s >>= 1) {
        for (int i = threadIdx.x; i < s; i += 256) {
            pa[i] = __fadd_rn(pa[i], pa[i + s]);
            pb[i] = __fadd_rn(pb[i], pb[i + s]);
        }
        __syncthreads();
    }
    const float st = __fdiv_rn(pa[0], __fadd_rn(pb[0], 1e-8f)), c = cfg[0];
    for (int i = threadIdx.x; i < n; i += 256) {
        const float a = __fmul_rn(neg[i], st);
        const float d = __fadd_rn(a, __fmul_rn(c, __fsub_rn(pos[i], a)));
        d_out[b * n + i] = d;
        x[b * n + i] = __fsub_rn(x[b * n + i], __fmul_rn(dt, d));
    }
}

// ---- configuration, schedule and tables (host) ---------------------------------------------------------------------------------------
float VlocConfig::resid_scale(const VlocStack& s) const { return use_mup ? scale_depth / std::sqrt((float)s.layers) : 1.0f; }

void vloc_schedule(int n_steps, float* t) {
    const int n = n_steps < 1 ? 1 : n_steps;
    for (int i = 0; i <= n; ++i) {
        const double u = 1.0 - (double)i / (double)n;
        t[i] = (float)(u + (std::cos(M_PI / 2.0 * u) - 1.0 + u));
    }
}

int vloc_zero_steps(int n_steps) {
    const int z = (int)((double)(n_steps + 1) * 0.04);
    return z < 1 ? 1 : z;
}

void vloc_rope_table(const VlocConfig& c, int head_dim, int n_pos, float* cs, float* sn) {
    const int half = head_dim / 2;
    const bool use_long = std::max(1, c.max_pos) > std::max(1, c.rope_orig);
    const std::vector<float>& f = use_long ? c.long_factor : c.short_factor;
    if (!(f.empty() || f.size() == 1 || (int)f.size() == half))
        throw std::invalid_argument(std::string("rope_scaling.") + (use_long ? "long_factor" : "short_factor") + " holds " + std::to_string(f.size()) +
                                    " values, neither 0, 1 nor head_dim / 2 = " + std::to_string(half));
    // LMConfig.originalMaxPositionEmbeddings has no coding key: 32768 whatever config.json says (MiniCPM4.swift:66-69)
    const double ratio = (double)std::max(c.max_pos, 1) / 32768.0;
    const double scale = std::sqrt(1.0 + std::log(std::max(ratio, 1.0)) / std::log(32768.0));
    for (int p = 0; p < n_pos; ++p)
        for (int i = 0; i < half; ++i) {
            const double inv = std::exp((double)i / (double)half * -std::log((double)c.rope_theta));
            const double fac = f.empty() ? 1.0 : (double)f[f.size() == 1 ? 0 : i];
            const double ang = (double)p * (1.0 / fac) * inv;
            cs[(size_t)p * head_dim + i] = cs[(size_t)p * head_dim + half + i] = (float)(std::cos(ang) * scale);
            sn[(size_t)p * head_dim + i] = sn[(size_t)p * head_dim + half + i] = (float)(std::sin(ang) * scale);
        }
}

static void read_stack(const Json* j, VlocStack& s) {
    if (!j) return;
    auto num = [&](const char* k, int& v) { if (const Json* e = j->get(k)) if (e->type == Json::Num) v = (int)e->num; };
    num("hidden_dim", s.hidden); num("ffn_dim", s.ffn); num("num_heads", s.heads); num("num_layers", s.layers);
    s.head_dim = 128;                                   // kv_channels ?? hidden / heads, the default 128
    if (const Json* e = j->get("kv_channels")) {
        if (e->type == Json::Num) s.head_dim = (int)e->num;
        else if (e->type == Json::Null) s.head_dim = s.heads > 0 ? s.hidden / s.heads : 0;
    }
}

VlocConfig vloc_read_config(const std::string& model_dir, const char* who_c) {
    const std::string who = std::string(who_c) + ": ";
    VlocConfig c;
    std::string text;
    if (FILE* f = fopen((model_dir + "/config.json").c_str(), "rb")) {
        char buf[4096];
        size_t n;
        while ((n = fread(buf, 1, sizeof buf, f)) > 0) text.append(buf, n);
        fclose(f);
    }
    bool mean_mode = false;
    if (!text.empty()) {
        Json root;
        try { root = JsonParser(text.data(), text.size()).parse(); }
        catch (const std::exception& ex) { throw std::invalid_argument(who + "config.json: " + ex.what()); }
        auto num = [](const Json* o, const char* k, int& v) { if (o) if (const Json* e = o->get(k)) if (e->type == Json::Num) v = (int)e->num; };
        auto real = [](const Json* o, const char* k, float& v) { if (o) if (const Json* e = o->get(k)) if (e->type == Json::Num) v = (float)e->num; };
        auto flag = [](const Json* o, const char* k, bool& v) { if (o) if (const Json* e = o->get(k)) if (e->type == Json::Bool) v = e->b; };
        auto list = [&](const Json* o, const char* k, std::vector<float>& v) {
            const Json* e = o ? o->get(k) : nullptr;
            if (!e || e->type == Json::Null) return;
            if (e->type != Json::Arr) throw std::invalid_argument(who + "rope_scaling." + k + " is not a list");
            v.clear();
            for (const Json& x : e->arr) {
                if (x.type != Json::Num) throw std::invalid_argument(who + "rope_scaling." + k + " holds a non-number");
                v.push_back((float)x.num);
            }
        };
        num(&root, "patch_size", c.patch_size); num(&root, "feat_dim", c.feat_dim);
        const Json* lm = root.get("lm_config");
        num(lm, "hidden_size", c.lm_hidden); num(lm, "num_key_value_heads", c.kv_heads); num(lm, "max_position_embeddings", c.max_pos);
        real(lm, "rms_norm_eps", c.rms_eps); real(lm, "rope_theta", c.rope_theta); real(lm, "scale_depth", c.scale_depth);
        flag(lm, "use_mup", c.use_mup);
        if (const Json* rs = lm ? lm->get("rope_scaling") : nullptr) {
            if (rs->type == Json::Obj) {
                list(rs, "short_factor", c.short_factor); list(rs, "long_factor", c.long_factor);
                num(rs, "original_max_position_embeddings", c.rope_orig);
            }
        }
        read_stack(root.get("encoder_config"), c.enc);
        read_stack(root.get("dit_config"), c.dit);
        flag(root.get("dit_config"), "mean_mode", mean_mode);
    }
    if (mean_mode) throw std::invalid_argument(who + "dit_config.mean_mode is true: only the dt = 0 estimator is built");
    if (c.patch_size < 1 || c.patch_size > 8) throw std::invalid_argument(who + "patch_size outside 1..8");
    if (c.feat_dim < 16 || c.feat_dim > 256 || c.feat_dim % 16) throw std::invalid_argument(who + "feat_dim is not a multiple of 16 in 16..256");
    if (c.lm_hidden < VL_KC || c.lm_hidden > 16384 || c.lm_hidden % VL_KC) throw std::invalid_argument(who + "lm_config.hidden_size is not a multiple of 512 in 512..16384");
    if (!(c.rms_eps > 0.0f)) throw std::invalid_argument(who + "lm_config.rms_norm_eps must be positive");
    if (!(c.rope_theta > 1.0f)) throw std::invalid_argument(who + "lm_config.rope_theta must exceed 1");
    auto stack = [&](const VlocStack& s, const std::string& f) {
        if (s.head_dim != VL_HEAD_DIM) throw std::invalid_argument(who + f + ".kv_channels (head_dim) is " + std::to_string(s.head_dim) + ": the attention launch serves 128 only");
        if (s.hidden < VL_KC || s.hidden > 8192 || s.hidden % VL_KC) throw std::invalid_argument(who + f + ".hidden_dim is not a multiple of 512 in 512..8192");
        if (s.ffn < VL_KC || s.ffn > 32768 || s.ffn % VL_KC) throw std::invalid_argument(who + f + ".ffn_dim is not a multiple of 512 in 512..32768");
        if (s.heads < 1 || s.heads > 64 || (s.heads * VL_HEAD_DIM) % VL_KC) throw std::invalid_argument(who + f + ".num_heads outside 1..64 or heads x 128 no multiple of 512");
        if (s.layers < 1 || s.layers > 64) throw std::invalid_argument(who + f + ".num_layers outside 1..64");
        if (c.kv_heads < 1 || s.heads % c.kv_heads) throw std::invalid_argument(who + "lm_config.num_key_value_heads does not divide " + f + ".num_heads");
    };
    stack(c.enc, "encoder_config");
    stack(c.dit, "dit_config");
    std::vector<float> t((size_t)2 * VL_HEAD_DIM);
    try { vloc_rope_table(c, VL_HEAD_DIM, 1, t.data(), t.data() + VL_HEAD_DIM); }
    catch (const std::invalid_argument& ex) { throw std::invalid_argument(who + "lm_config." + ex.what()); }
    return c;
}

using Shapes = std::vector<std::pair<std::string, std::vector<int64_t>>>;

static void stack_shapes(Shapes& s, const std::string& p, const VlocStack& g, int kv_heads) {
    const int qd = g.heads * g.head_dim, kd = kv_heads * g.head_dim;
    for (int l = 0; l < g.layers; ++l) {
        const std::string q = p + ".layers." + std::to_string(l);
        s.push_back({q + ".self_attn.q_proj.weight", {qd, g.hidden}});
        s.push_back({q + ".self_attn.k_proj.weight", {kd, g.hidden}});
        s.push_back({q + ".self_attn.v_proj.weight", {kd, g.hidden}});
        s.push_back({q + ".self_attn.o_proj.weight", {g.hidden, qd}});
        s.push_back({q + ".mlp.gate_proj.weight", {g.ffn, g.hidden}});
        s.push_back({q + ".mlp.up_proj.weight", {g.ffn, g.hidden}});
        s.push_back({q + ".mlp.down_proj.weight", {g.hidden, g.ffn}});
        s.push_back({q + ".input_layernorm.weight", {g.hidden}});
        s.push_back({q + ".post_attention_layernorm.weight", {g.hidden}});
    }
    s.push_back({p + ".norm.weight", {g.hidden}});
}

// an MLX affine-quantised Linear of the checkpoint: `weight` U32 [N][K bits / 32], `scales` and `biases` [N][K / 64]
static VlocQuant read_quant(const SafeTensorsDir& st, const std::string& pre, const std::string& stem, long N, long K, size_t& bytes) {
    const SafeEntry &w = st.entries.at(stem + ".weight"), &sc = st.entries.at(stem + ".scales");
    auto bi_it = st.entries.find(stem + ".biases");
    if (bi_it == st.entries.end()) throw WeightLoadError(QASR_ERR_IO, pre + "tensor " + stem + ".biases is missing");
    const SafeEntry& bi = bi_it->second;
    if (K % 64) throw WeightLoadError(QASR_ERR_INVALID, pre + "tensor " + stem + ".weight is quantised over K = " + std::to_string(K) + ", no multiple of the group 64");
    const std::vector<int64_t> gs{N, K / 64};
    if (sc.shape != gs || bi.shape != gs || sc.dtype != bi.dtype || (sc.dtype != "F32" && sc.dtype != "F16" && sc.dtype != "BF16"))
        throw WeightLoadError(QASR_ERR_INVALID, pre + "tensor " + stem + ".scales / .biases are not [" + std::to_string(N) + "][" + std::to_string(K / 64) + "] of one float dtype (group size 64)");
    VlocQuant q;
    q.N = (int)N; q.K = (int)K;
    if (w.dtype == "U32" && w.shape == std::vector<int64_t>{N, K / 8}) q.bits = 4;
    else if (w.dtype == "U32" && w.shape == std::vector<int64_t>{N, K / 4}) q.bits = 8;
    else throw WeightLoadError(QASR_ERR_INVALID, pre + "tensor " + stem + ".weight is not U32 [" + std::to_string(N) + "][K / 8] (4 bit) or [..][K / 4] (8 bit)");
    q.wq.resize(w.bytes / 4);
    std::memcpy(q.wq.data(), w.data, q.wq.size() * 4);
    q.scales.resize(sc.numel()); q.biases.resize(bi.numel());
    for (size_t i = 0; i < q.scales.size(); ++i) { q.scales[i] = safe_elem_f32(sc, i); q.biases[i] = safe_elem_f32(bi, i); }
    bytes += w.bytes + sc.bytes + bi.bytes;
    return q;
}

VlocWeights vloc_load_weights(const std::string& model_dir, const char* who, VlocConfig& c) {
    const std::string pre = std::string(who) + ": ";
    std::unique_ptr<SafeTensorsDir> st;
    try { st = std::make_unique<SafeTensorsDir>(model_dir); }
    catch (const std::exception& ex) { throw WeightLoadError(QASR_ERR_IO, pre + ex.what()); }
    auto quantised = [&](const std::string& stem) { return st->entries.count(stem + ".scales") != 0; };
    // mu = lm_to_dit_proj(lm hidden) || res_to_dit_proj(residual hidden), cut into tokens of dit.hidden values: the token count follows the rows
    long mu_rows = 0;
    for (const char* stem : {"lm_to_dit_proj", "res_to_dit_proj"}) {
        const std::string k = std::string(stem) + ".weight";
        auto it = st->entries.find(k);
        if (it == st->entries.end()) throw WeightLoadError(QASR_ERR_IO, pre + "tensor " + k + " is missing");
        if (it->second.shape.size() != 2 || (!quantised(stem) && it->second.shape[1] != c.lm_hidden) || it->second.shape[0] < 16 || it->second.shape[0] % 16)
            throw WeightLoadError(QASR_ERR_INVALID, pre + "tensor " + k + " is not [16 n][" + std::to_string(c.lm_hidden) + "]");
        mu_rows += it->second.shape[0];
    }
    if (mu_rows % c.dit.hidden || mu_rows / c.dit.hidden < 1 || mu_rows / c.dit.hidden > 4)
        throw WeightLoadError(QASR_ERR_INVALID, pre + "lm_to_dit_proj.weight and res_to_dit_proj.weight hold " + std::to_string(mu_rows) +
                                                    " rows together, not 1..4 tokens of dit_config.hidden_dim = " + std::to_string(c.dit.hidden));
    c.mu_tokens = (int)(mu_rows / c.dit.hidden);
    Shapes s;
    auto lin = [&](const std::string& k, long out, long in) { s.push_back({k + ".weight", {out, in}}); s.push_back({k + ".bias", {out}}); };
    const int He = c.enc.hidden, Hd = c.dit.hidden, F = c.feat_dim;
    s.push_back({"feat_encoder.special_token", {1, 1, 1, He}});
    lin("feat_encoder.in_proj", He, F);
    stack_shapes(s, "feat_encoder.encoder", c.enc, c.kv_heads);
    lin("feat_decoder.estimator.in_proj", Hd, F);
    lin("feat_decoder.estimator.cond_proj", Hd, F);
    lin("feat_decoder.estimator.out_proj", F, Hd);
    for (const char* m : {"time_mlp", "delta_time_mlp"})
        for (const char* l : {".linear_1", ".linear_2"}) lin(std::string("feat_decoder.estimator.") + m + l, Hd, Hd);
    stack_shapes(s, "feat_decoder.estimator.decoder", c.dit, c.kv_heads);
    lin("enc_to_lm_proj", c.lm_hidden, He);
    lin("lm_to_dit_proj", st->entries.at("lm_to_dit_proj.weight").shape[0], c.lm_hidden);
    lin("res_to_dit_proj", st->entries.at("res_to_dit_proj.weight").shape[0], c.lm_hidden);
    // a Linear whose stem has .scales is an MLX 4-bit / 8-bit triplet (swapQuantizedLinears, VoxCPM2TTS.swift:380): read as stored, the rest as floats
    VlocWeights out;
    Shapes floats;
    size_t qbytes = 0;
    for (const auto& ks : s) {
        const std::string& k = ks.first;
        const bool is_w = ks.second.size() == 2 && k.size() > 7 && k.compare(k.size() - 7, 7, ".weight") == 0;
        const std::string stem = is_w ? k.substr(0, k.size() - 7) : "";
        if (is_w && st->entries.count(k) && quantised(stem)) out.q[stem] = read_quant(*st, pre, stem, ks.second[0], ks.second[1], qbytes);
        else floats.push_back(ks);
    }
    out.f = load_checked_f32(*st, who, floats, false);
    out.f.disk_bytes += qbytes;
    return out;
}

// ---- the host object ----------------------------------------------------------------------------------------------------------------
static const char* const WHO = "VoxCPM2 local networks";

static size_t gemm_lds(int mb) { return (size_t)16 * mb * VL_LDA * sizeof(bf16_t); }

LocVoxcpm::LocVoxcpm(int device, const VlocConfig& cfg, const VlocWeights& vw, long max_seqs, hipStream_t work)
    : device_(device), cfg_(cfg), max_seqs_(max_seqs) {
    if (max_seqs < 1 || max_seqs > VL_MAX_SEQS) throw std::invalid_argument(std::string(WHO) + ": max_seqs in 1..1024");
    if (cfg.dit_tokens() > VL_MAX_S || cfg.patch_size + 1 > VL_MAX_S) throw std::invalid_argument(std::string(WHO) + ": a sequence exceeds 32 tokens");
    const CheckedWeights& cw = vw.f;
    param_bytes_ = cw.disk_bytes;
    struct Dequant { const VlocQuant* q; size_t at; };
    std::vector<Dequant> dequant;                       // quantised matrices: their rows of the bf16 image are written on the device
    std::vector<bf16_t> hb;
    std::vector<float> hf;
    auto mat = [&](const std::vector<std::string>& keys, int K) {       // the keys' rows one under the other
        Lin l; l.K = K; l.w = hb.size();
        for (const auto& k : keys) {
            auto qi = vw.q.find(k);
            if (qi != vw.q.end()) {
                dequant.push_back({&qi->second, hb.size()});
                hb.resize(hb.size() + (size_t)qi->second.N * K, 0);
                l.N += qi->second.N;
                continue;
            }
            const auto& v = cw.t.at(k + ".weight");
            for (float x : v) hb.push_back(f32_to_bf16_host(x));
            l.N += (int)(v.size() / (size_t)K);
        }
        hb.resize((hb.size() + 7) & ~(size_t)7);
        return l;
    };
    auto vec = [&](const std::string& k) {
        const auto& v = cw.t.at(k);
        const size_t at = hf.size();
        hf.insert(hf.end(), v.begin(), v.end());
        hf.resize((hf.size() + 3) & ~(size_t)3);
        return at;
    };
    auto lin = [&](const std::string& k, int K) { Lin l = mat({k}, K); l.bias = vec(k + ".bias"); l.has_bias = true; return l; };
    auto net = [&](const std::string& p, const VlocStack& g) {
        Net n; n.g = g; n.s = cfg.resid_scale(g);
        for (int i = 0; i < g.layers; ++i) {
            const std::string q = p + ".layers." + std::to_string(i);
            Layer L;
            L.n1 = vec(q + ".input_layernorm.weight"); L.n2 = vec(q + ".post_attention_layernorm.weight");
            L.qkv = mat({q + ".self_attn.q_proj", q + ".self_attn.k_proj", q + ".self_attn.v_proj"}, g.hidden);
            L.o = mat({q + ".self_attn.o_proj"}, g.heads * g.head_dim);
            L.gu = mat({q + ".mlp.gate_proj", q + ".mlp.up_proj"}, g.hidden);
            L.gu.N = g.ffn;                            // the fused width; the up rows lie N rows below the gate rows
            L.down = mat({q + ".mlp.down_proj"}, g.ffn);
            n.layers.push_back(L);
        }
        n.norm = vec(p + ".norm.weight");
        return n;
    };
    const int He = cfg.enc.hidden, Hd = cfg.dit.hidden, F = cfg.feat_dim, P = cfg.patch_size;
    special_ = vec("feat_encoder.special_token");
    enc_in_ = lin("feat_encoder.in_proj", F);
    enc_ = net("feat_encoder.encoder", cfg.enc);
    dit_in_ = lin("feat_decoder.estimator.in_proj", F);
    dit_cond_ = lin("feat_decoder.estimator.cond_proj", F);
    dit_out_ = lin("feat_decoder.estimator.out_proj", Hd);
    t1_ = lin("feat_decoder.estimator.time_mlp.linear_1", Hd); t2_ = lin("feat_decoder.estimator.time_mlp.linear_2", Hd);
    dt1_ = lin("feat_decoder.estimator.delta_time_mlp.linear_1", Hd); dt2_ = lin("feat_decoder.estimator.delta_time_mlp.linear_2", Hd);
    dit_ = net("feat_decoder.estimator.decoder", cfg.dit);
    enc_to_lm_ = lin("enc_to_lm_proj", He);
    lm_to_dit_ = lin("lm_to_dit_proj", cfg.lm_hidden);
    res_to_dit_ = lin("res_to_dit_proj", cfg.lm_hidden);
    rope_cos_ = hf.size(); hf.resize(hf.size() + (size_t)VL_MAX_S * VL_HEAD_DIM);
    rope_sin_ = hf.size(); hf.resize(hf.size() + (size_t)VL_MAX_S * VL_HEAD_DIM);
    vloc_rope_table(cfg, VL_HEAD_DIM, VL_MAX_S, &hf[rope_cos_], &hf[rope_sin_]);

    QASR_HIP(hipSetDevice(device_));
    ensure_dynamic_lds(reinterpret_cast<const void*>(&vl_gemm_kernel<1, false>), (int)gemm_lds(1));
    ensure_dynamic_lds(reinterpret_cast<const void*>(&vl_gemm_kernel<2, false>), (int)gemm_lds(2));
    ensure_dynamic_lds(reinterpret_cast<const void*>(&vl_gemm_kernel<4, false>), (int)gemm_lds(4));
    ensure_dynamic_lds(reinterpret_cast<const void*>(&vl_gemm_kernel<1, true>), (int)gemm_lds(1));
    ensure_dynamic_lds(reinterpret_cast<const void*>(&vl_gemm_kernel<2, true>), (int)gemm_lds(2));
    ensure_dynamic_lds(reinterpret_cast<const void*>(&vl_gemm_kernel<4, true>), (int)gemm_lds(4));
    QASR_HIP(hipStreamCreateWithFlags(&own_, hipStreamNonBlocking));
    work_ = work ? work : own_;
    for (auto& e : ev_) QASR_HIP(hipEventCreate(&e));
    d_wb_.alloc(hb.size() * sizeof(bf16_t));
    QASR_HIP(hipMemcpy(d_wb_.p, hb.data(), hb.size() * sizeof(bf16_t), hipMemcpyHostToDevice));
    // bf16(scale q + bias), once: the image the reference's multi-row kernel multiplies by (dec_quant.h)
    for (const Dequant& d : dequant) {
        DevBuf w, sc, bi;
        w.alloc(d.q->wq.size() * 4); sc.alloc(d.q->scales.size() * 4); bi.alloc(d.q->biases.size() * 4);
        QASR_HIP(hipMemcpy(w.p, d.q->wq.data(), d.q->wq.size() * 4, hipMemcpyHostToDevice));
        QASR_HIP(hipMemcpy(sc.p, d.q->scales.data(), d.q->scales.size() * 4, hipMemcpyHostToDevice));
        QASR_HIP(hipMemcpy(bi.p, d.q->biases.data(), d.q->biases.size() * 4, hipMemcpyHostToDevice));
        QuantRaw raw;
        raw.wq = w.as<uint32_t>(); raw.scales = sc.p; raw.biases = bi.p; raw.sb_f32 = 1; raw.N = d.q->N; raw.K = d.q->K; raw.bits = d.q->bits;
        quant_dequant_rows_launch(raw, 0, raw.N, d_wb_.as<bf16_t>() + d.at, work_);
        QASR_HIP(hipGetLastError());
        QASR_HIP(hipStreamSynchronize(work_));
    }
    d_wf_.alloc(hf.size() * sizeof(float));
    QASR_HIP(hipMemcpy(d_wf_.p, hf.data(), hf.size() * sizeof(float), hipMemcpyHostToDevice));
    const size_t f4 = sizeof(float), Q = 2 * (size_t)max_seqs, rows = Q * VL_MAX_S;
    const size_t H = std::max(He, Hd), qkvw = (size_t)(std::max(cfg.enc.heads, cfg.dit.heads) + 2 * cfg.kv_heads) * VL_HEAD_DIM;
    d_h_.alloc(rows * H * f4);
    d_qkv_.alloc(rows * qkvw * f4);
    d_attn_.alloc(rows * (size_t)std::max(cfg.enc.heads, cfg.dit.heads) * VL_HEAD_DIM * f4);
    d_act_.alloc(rows * (size_t)std::max(cfg.enc.ffn, cfg.dit.ffn) * f4);
    d_norm_.alloc(Q * (size_t)std::max(P, 1) * H * f4);
    d_ab_.alloc(rows * (size_t)std::max({cfg.enc.hidden, cfg.dit.hidden, cfg.enc.ffn, cfg.dit.ffn, cfg.enc.heads * VL_HEAD_DIM, cfg.dit.heads * VL_HEAD_DIM, cfg.lm_hidden}) * sizeof(bf16_t));
    (void)gemm_zero_block();                           // allocated here, not inside a capture
    d_x_.alloc((size_t)max_seqs * P * F * f4);
    d_mu_.alloc((size_t)max_seqs * cfg.mu_dim() * f4);
    d_cond_.alloc((size_t)max_seqs * P * F * f4);
    d_condp_.alloc((size_t)max_seqs * P * Hd * f4);
    d_v_.alloc(Q * P * F * f4);
    d_d_.alloc((size_t)max_seqs * P * F * f4);
    d_cfg_.alloc(f4);
    d_sin_.alloc((size_t)VL_MAX_STEPS * Hd * f4);
    d_t1_.alloc((size_t)VL_MAX_STEPS * Hd * f4);
    d_ttok_.alloc((size_t)Hd * f4);
    d_dconst_.alloc((size_t)Hd * f4);
    d_lm_.alloc((size_t)2 * max_seqs * cfg.lm_hidden * f4);
    d_embed_.alloc((size_t)max_seqs * cfg.lm_hidden * f4);
    // mean_mode false: dt = 0 in every call, so delta_time_mlp(sinusoid(0)) is one vector per model
    std::vector<float> s0((size_t)Hd, 0.0f);
    for (int i = Hd / 2; i < Hd; ++i) s0[i] = 1.0f;
    QASR_HIP(hipMemcpyAsync(d_sin_.p, s0.data(), s0.size() * f4, hipMemcpyHostToDevice, work_));
    gemm(dt1_, d_sin_.as<float>(), Hd, 1, 1, 0, nullptr, nullptr, 0, 1.0f, 1, false, d_t1_.as<float>(), Hd, 1);
    gemm(dt2_, d_t1_.as<float>(), Hd, 1, 1, 0, nullptr, nullptr, 0, 1.0f, 0, false, d_dconst_.as<float>(), Hd, 1);
    QASR_HIP(hipStreamSynchronize(work_));
}

LocVoxcpm::~LocVoxcpm() {
    if (work_) (void)hipStreamSynchronize(work_);
    for (auto& kv : solves_) if (kv.second.exec) (void)hipGraphExecDestroy(kv.second.exec);
    for (auto& e : ev_) if (e) (void)hipEventDestroy(e);
    if (own_) (void)hipStreamDestroy(own_);
}

void LocVoxcpm::drop_solves() {
    QASR_HIP(hipStreamSynchronize(work_));
    for (auto& kv : solves_) if (kv.second.exec) (void)hipGraphExecDestroy(kv.second.exec);
    solves_.clear();
}

void LocVoxcpm::unload() {
    if (!loaded_) return;
    QASR_HIP(hipSetDevice(device_));
    QASR_HIP(hipStreamSynchronize(work_));
    for (auto& kv : solves_) if (kv.second.exec) (void)hipGraphExecDestroy(kv.second.exec);
    solves_.clear();
    for (DevBuf* b : {&d_wb_, &d_wf_, &d_h_, &d_qkv_, &d_attn_, &d_act_, &d_norm_, &d_ab_, &d_x_, &d_mu_, &d_cond_, &d_condp_, &d_v_, &d_d_, &d_cfg_, &d_sin_,
                      &d_t1_, &d_ttok_, &d_dconst_, &d_lm_, &d_embed_})
        b->release();
    loaded_ = false;
}

void LocVoxcpm::check_loaded() const {
    if (!loaded_) throw NotLoaded(std::string(WHO) + ": model unloaded");
}

void LocVoxcpm::begin(int) {
    check_loaded();
    QASR_HIP(hipSetDevice(device_));
    QASR_HIP(hipEventRecord(ev_[0], work_));
}

void LocVoxcpm::end(int slot) {
    QASR_HIP(hipEventRecord(ev_[1], work_));
    QASR_HIP(hipStreamSynchronize(work_));
    QASR_HIP(hipEventElapsedTime(&timing_[slot], ev_[0], ev_[1]));
}

// ---- launches -----------------------------------------------------------------------------------------------------------------------
void LocVoxcpm::gemm(const Lin& l, const float* A, long lda, int a_group, int a_stride, int a_off, const float* norm_w, const float* resid, long ldr,
                     float s, int act, bool swiglu, float* out, long ldo, long M) {
    if (M <= 0) return;
    if (l.K % VL_KC || l.N % 16) throw std::invalid_argument(std::string(WHO) + ": a Linear of K = " + std::to_string(l.K) + ", N = " + std::to_string(l.N) +
                                                             " is outside the skinny GEMM's shapes (K a multiple of 512, N of 16)");
    if (M > tuning().vloc_skinny_rows) {               // the wide pass (knob vloc_skinny_rows; 0 = always)
        bf16_t* ab = d_ab_.as<bf16_t>();
        hipLaunchKernelGGL(vl_rows_bf16_kernel, dim3((unsigned)M), dim3(64), 0, work_, A, lda, a_group, a_stride, a_off, l.K, norm_w, cfg_.rms_eps, ab);
        QASR_HIP(hipGetLastError());
        const ADense rows{ab, (long)l.K, (int)M, l.K};
        if (swiglu) {                                  // gate into out, then up with silu(gate) up in the epilogue
            gemm_nt(rows, Wb(l.w), l.K, (int)M, l.N, l.K, EpiVl{nullptr, nullptr, 0, 1.0f, 0, 0, out, ldo}, work_);
            gemm_nt(rows, Wb(l.w) + (size_t)l.N * l.K, l.K, (int)M, l.N, l.K, EpiVl{nullptr, nullptr, 0, 1.0f, 0, 1, out, ldo}, work_);
        } else {
            gemm_nt(rows, Wb(l.w), l.K, (int)M, l.N, l.K, EpiVl{l.has_bias ? Wf(l.bias) : nullptr, resid, ldr, s, act, 0, out, ldo}, work_);
        }
        QASR_HIP(hipGetLastError());
        return;
    }
    VlGemmArgs a{A, lda, a_group, a_stride, a_off, norm_w, cfg_.rms_eps, Wb(l.w), l.has_bias ? Wf(l.bias) : nullptr, resid, ldr, s, act, out, ldo,
                 (int)M, l.N, l.K};
    const int mb = M <= 16 ? 1 : M <= 32 ? 2 : 4;
    const dim3 grid((unsigned)(l.N / 16), (unsigned)cdiv(M, 16 * mb)), block(VL_GEMM_THREADS);
    const size_t lds = gemm_lds(mb);
#define VL_GO(MB, SW) hipLaunchKernelGGL((vl_gemm_kernel<MB, SW>), grid, block, lds, work_, a)
    if (swiglu) { if (mb == 1) VL_GO(1, true); else if (mb == 2) VL_GO(2, true); else VL_GO(4, true); }
    else { if (mb == 1) VL_GO(1, false); else if (mb == 2) VL_GO(2, false); else VL_GO(4, false); }
#undef VL_GO
    QASR_HIP(hipGetLastError());
}

void LocVoxcpm::run_stack(const Net& net, long n_seq, int S, int n_layers) {
    const VlocStack& g = net.g;
    const long rows = n_seq * S;
    const int H = g.hidden, qd = g.heads * g.head_dim, qkvw = (g.heads + 2 * cfg_.kv_heads) * g.head_dim;
    float *h = d_h_.as<float>(), *qkv = d_qkv_.as<float>(), *attn = d_attn_.as<float>(), *act = d_act_.as<float>();
    for (int l = 0; l < n_layers; ++l) {
        const Layer& L = net.layers[l];
        gemm(L.qkv, h, H, 1, 1, 0, Wf(L.n1), nullptr, 0, 1.0f, 0, false, qkv, qkvw, rows);
        vl_attention_launch(qkv, n_seq, S, g.heads, cfg_.kv_heads, Wf(rope_cos_), Wf(rope_sin_), attn, work_);
        QASR_HIP(hipGetLastError());
        gemm(L.o, attn, qd, 1, 1, 0, nullptr, h, H, net.s, 0, false, h, H, rows);
        gemm(L.gu, h, H, 1, 1, 0, Wf(L.n2), nullptr, 0, 1.0f, 0, true, act, g.ffn, rows);
        gemm(L.down, act, g.ffn, 1, 1, 0, nullptr, h, H, net.s, 0, false, h, H, rows);
    }
}

void LocVoxcpm::final_norm(const Net& net, long rows, int group, int stride, int off, float* out) {
    hipLaunchKernelGGL(vl_norm_rows_kernel, dim3((unsigned)rows), dim3(64), 0, work_, d_h_.as<float>(), net.g.hidden, group, stride, off, Wf(net.norm),
                       cfg_.rms_eps, out);
    QASR_HIP(hipGetLastError());
}

void LocVoxcpm::small_linear(const Lin& l, const float* x, long rows, float* out) {
    hipLaunchKernelGGL(vl_small_linear_kernel, dim3((unsigned)rows), dim3(256), 0, work_, x, l.K, Wb(l.w), Wf(l.bias), l.N, out);
    QASR_HIP(hipGetLastError());
}

// time_mlp(sinusoid(t)) + delta_time_mlp(sinusoid(0)) for n values of t: the sinusoid [sin ; cos] of 1000 t exp(-i ln 10000 / (half - 1)) in
// f32 on the host, the two Linears on the device
void LocVoxcpm::time_tokens(const float* t, int n, float* out) {
    const int H = cfg_.dit.hidden, half = H / 2;
    std::vector<float>& s = h_sin_;                    // a member: the copy below may still read it when this returns
    s.resize((size_t)n * H);
    const float es = std::log(10000.0f) / (float)(half - 1);
    for (int r = 0; r < n; ++r)
        for (int i = 0; i < half; ++i) {
            const float e = 1000.0f * t[r] * std::exp((float)i * -es);
            s[(size_t)r * H + i] = std::sin(e);
            s[(size_t)r * H + half + i] = std::cos(e);
        }
    QASR_HIP(hipMemcpyAsync(d_sin_.p, s.data(), s.size() * sizeof(float), hipMemcpyHostToDevice, work_));
    gemm(t1_, d_sin_.as<float>(), H, 1, 1, 0, nullptr, nullptr, 0, 1.0f, 1, false, d_t1_.as<float>(), H, n);
    gemm(t2_, d_t1_.as<float>(), H, 1, 1, 0, nullptr, d_dconst_.as<float>(), 0, 1.0f, 0, false, out, H, n);
}

void LocVoxcpm::assemble_dit(long n_seq, long mu_seqs, long B, const float* ttok) {
    VlAssembleArgs a{};
    a.h = d_h_.as<float>(); a.H = cfg_.dit.hidden; a.S = cfg_.dit_tokens();
    a.n_lead = 0; a.n_mu = cfg_.mu_tokens; a.has_time = 1; a.n_cond = cfg_.patch_size; a.P = cfg_.patch_size; a.F = cfg_.feat_dim;
    a.mu = d_mu_.as<float>(); a.mu_seqs = mu_seqs; a.B = B; a.ttok = ttok; a.condp = d_condp_.as<float>(); a.x = d_x_.as<float>();
    a.Win = Wb(dit_in_.w); a.bin = Wf(dit_in_.bias);
    hipLaunchKernelGGL(vl_assemble_kernel, dim3((unsigned)(n_seq * a.S)), dim3(256), 0, work_, a);
    QASR_HIP(hipGetLastError());
}

// ---- entries ------------------------------------------------------------------------------------------------------------------------
void LocVoxcpm::encode(const float* feats, long n, float* cls, float* embed) {
    begin(0);
    const int P = cfg_.patch_size, F = cfg_.feat_dim, H = cfg_.enc.hidden, S = P + 1;
    float ms = 0.0f;
    for (long at = 0; at < n; at += max_seqs_) {
        const long q = std::min(max_seqs_, n - at);
        QASR_HIP(hipEventRecord(ev_[0], work_));
        QASR_HIP(hipMemcpyAsync(d_x_.p, feats + at * P * F, (size_t)q * P * F * sizeof(float), hipMemcpyHostToDevice, work_));
        VlAssembleArgs a{};
        a.h = d_h_.as<float>(); a.H = H; a.S = S; a.n_lead = 1; a.lead = Wf(special_); a.P = P; a.F = F; a.B = q; a.x = d_x_.as<float>();
        a.Win = Wb(enc_in_.w); a.bin = Wf(enc_in_.bias);
        hipLaunchKernelGGL(vl_assemble_kernel, dim3((unsigned)(q * S)), dim3(256), 0, work_, a);
        QASR_HIP(hipGetLastError());
        run_stack(enc_, q, S, cfg_.enc.layers);
        final_norm(enc_, q, 1, S, 0, d_norm_.as<float>());
        if (embed) gemm(enc_to_lm_, d_norm_.as<float>(), H, 1, 1, 0, nullptr, nullptr, 0, 1.0f, 0, false, d_embed_.as<float>(), cfg_.lm_hidden, q);
        if (cls) QASR_HIP(hipMemcpyAsync(cls + at * H, d_norm_.p, (size_t)q * H * sizeof(float), hipMemcpyDeviceToHost, work_));
        if (embed) QASR_HIP(hipMemcpyAsync(embed + at * cfg_.lm_hidden, d_embed_.p, (size_t)q * cfg_.lm_hidden * sizeof(float), hipMemcpyDeviceToHost, work_));
        end(0);
        ms += timing_[0];
    }
    timing_[0] = ms;
}

void LocVoxcpm::mu(const float* lm_hidden, const float* res_hidden, long B, float* mu) {
    begin(1);
    if (B > max_seqs_) throw std::length_error(std::string(WHO) + ": B = " + std::to_string(B) + " exceeds max_seqs = " + std::to_string(max_seqs_));
    const size_t bytes = (size_t)B * cfg_.lm_hidden * sizeof(float);
    float* lm = d_lm_.as<float>();
    float* rs = lm + (size_t)max_seqs_ * cfg_.lm_hidden;
    QASR_HIP(hipMemcpyAsync(lm, lm_hidden, bytes, hipMemcpyHostToDevice, work_));
    QASR_HIP(hipMemcpyAsync(rs, res_hidden, bytes, hipMemcpyHostToDevice, work_));
    const int md = cfg_.mu_dim();
    gemm(lm_to_dit_, lm, cfg_.lm_hidden, 1, 1, 0, nullptr, nullptr, 0, 1.0f, 0, false, d_mu_.as<float>(), md, B);
    gemm(res_to_dit_, rs, cfg_.lm_hidden, 1, 1, 0, nullptr, nullptr, 0, 1.0f, 0, false, d_mu_.as<float>() + lm_to_dit_.N, md, B);
    QASR_HIP(hipMemcpyAsync(mu, d_mu_.p, (size_t)B * md * sizeof(float), hipMemcpyDeviceToHost, work_));
    end(1);
}

void LocVoxcpm::velocity(const float* x, const float* mu, const float* cond, long B, float t, float* v) {
    begin(2);
    if (B > max_seqs_) throw std::length_error(std::string(WHO) + ": B = " + std::to_string(B) + " exceeds max_seqs = " + std::to_string(max_seqs_));
    const int P = cfg_.patch_size, F = cfg_.feat_dim, S = cfg_.dit_tokens();
    const size_t pb = (size_t)B * P * F * sizeof(float);
    QASR_HIP(hipMemcpyAsync(d_x_.p, x, pb, hipMemcpyHostToDevice, work_));
    QASR_HIP(hipMemcpyAsync(d_cond_.p, cond, pb, hipMemcpyHostToDevice, work_));
    QASR_HIP(hipMemcpyAsync(d_mu_.p, mu, (size_t)B * cfg_.mu_dim() * sizeof(float), hipMemcpyHostToDevice, work_));
    time_tokens(&t, 1, d_ttok_.as<float>());
    small_linear(dit_cond_, d_cond_.as<float>(), B * P, d_condp_.as<float>());
    assemble_dit(B, B, B, d_ttok_.as<float>());
    run_stack(dit_, B, S, cfg_.dit.layers);
    final_norm(dit_, B * P, P, S, S - P, d_norm_.as<float>());
    gemm(dit_out_, d_norm_.as<float>(), cfg_.dit.hidden, 1, 1, 0, nullptr, nullptr, 0, 1.0f, 0, false, d_v_.as<float>(), F, B * P);
    QASR_HIP(hipMemcpyAsync(v, d_v_.p, pb, hipMemcpyDeviceToHost, work_));
    end(2);
}

// cond_proj once, then per step past the zero steps: token rows of 2 B sequences (mu given | mu zero), the stack, out_proj, the guided step
void LocVoxcpm::issue_solve(long B, int n_steps, const float* ttok) {
    const int P = cfg_.patch_size, F = cfg_.feat_dim, S = cfg_.dit_tokens(), H = cfg_.dit.hidden, n = P * F;
    int n2 = 1;
    while (n2 < n) n2 *= 2;
    std::vector<float> t((size_t)n_steps + 1);
    vloc_schedule(n_steps, t.data());
    small_linear(dit_cond_, d_cond_.as<float>(), B * P, d_condp_.as<float>());
    for (int step = vloc_zero_steps(n_steps) + 1; step <= n_steps; ++step) {
        const float dt = t[step - 1] - t[step];
        assemble_dit(2 * B, B, B, ttok + (size_t)(step - 1) * H);
        run_stack(dit_, 2 * B, S, cfg_.dit.layers);
        final_norm(dit_, 2 * B * P, P, S, S - P, d_norm_.as<float>());
        gemm(dit_out_, d_norm_.as<float>(), H, 1, 1, 0, nullptr, nullptr, 0, 1.0f, 0, false, d_v_.as<float>(), F, 2 * B * P);
        hipLaunchKernelGGL(vl_euler_kernel, dim3((unsigned)B), dim3(256), (size_t)2 * n2 * sizeof(float), work_, d_v_.as<float>(), B, n, n2,
                           d_cfg_.as<float>(), dt, d_x_.as<float>(), d_d_.as<float>());
        QASR_HIP(hipGetLastError());
    }
}

void LocVoxcpm::solve(const float* mu, const float* cond, const float* z, long B, int n_steps, float cfg, float* x_out, float* v_out) {
    begin(3);
    if (B > max_seqs_) throw std::length_error(std::string(WHO) + ": B = " + std::to_string(B) + " exceeds max_seqs = " + std::to_string(max_seqs_));
    if (n_steps < 1 || n_steps > VL_MAX_STEPS) throw std::invalid_argument(std::string(WHO) + ": n_steps in 1..64");
    const int P = cfg_.patch_size, F = cfg_.feat_dim, H = cfg_.dit.hidden;
    const size_t pb = (size_t)B * P * F * sizeof(float);
    if (knob_epoch_ != tuning().epoch) { drop_solves(); knob_epoch_ = tuning().epoch; }   // graphs and time tokens hold the old routing
    if (solves_.size() >= (size_t)VL_MAX_SOLVES && !solves_.count({B, n_steps})) drop_solves();
    auto it = solves_.find({B, n_steps});
    const bool fresh = it == solves_.end();
    if (fresh) {                                       // the steps' time tokens depend on n_steps alone: computed once, kept with the graph
        it = solves_.emplace(std::piecewise_construct, std::forward_as_tuple(B, n_steps), std::forward_as_tuple()).first;
        it->second.ttok.alloc((size_t)n_steps * H * sizeof(float));
        std::vector<float> t((size_t)n_steps + 1);
        vloc_schedule(n_steps, t.data());
        time_tokens(t.data(), n_steps, it->second.ttok.as<float>());
        QASR_HIP(hipEventRecord(ev_[0], work_));
    }
    QASR_HIP(hipMemcpyAsync(d_x_.p, z, pb, hipMemcpyHostToDevice, work_));
    QASR_HIP(hipMemcpyAsync(d_cond_.p, cond, pb, hipMemcpyHostToDevice, work_));
    QASR_HIP(hipMemcpyAsync(d_mu_.p, mu, (size_t)B * cfg_.mu_dim() * sizeof(float), hipMemcpyHostToDevice, work_));
    h_cfg_ = cfg;
    QASR_HIP(hipMemcpyAsync(d_cfg_.p, &h_cfg_, sizeof(float), hipMemcpyHostToDevice, work_));
    QASR_HIP(hipMemsetAsync(d_d_.p, 0, pb, work_));    // every step a zero step: the derivative reported is zero
    Solve& sv = it->second;
    if (fresh) {                                       // the first solve of a shape runs eagerly: code objects load outside a capture
        issue_solve(B, n_steps, sv.ttok.as<float>());
    } else if (!sv.exec && vloc_zero_steps(n_steps) < n_steps) {
        sv.exec = capture_graph(work_, [&] { issue_solve(B, n_steps, sv.ttok.as<float>()); });
    }
    if (!fresh && sv.exec) QASR_HIP(hipGraphLaunch(sv.exec, work_));
    QASR_HIP(hipMemcpyAsync(x_out, d_x_.p, pb, hipMemcpyDeviceToHost, work_));
    if (v_out) QASR_HIP(hipMemcpyAsync(v_out, d_d_.p, pb, hipMemcpyDeviceToHost, work_));
    end(3);
}

void LocVoxcpm::stack(int which, const float* x, long n_seq, int S, int n_layers, float* out) {
    begin(2);
    const Net& net = which ? dit_ : enc_;
    if (n_seq < 1 || n_seq > 2 * max_seqs_) throw std::length_error(std::string(WHO) + ": n_seq outside 1..2 max_seqs");
    if (S < 1 || S > VL_MAX_S) throw std::invalid_argument(std::string(WHO) + ": S in 1..32");
    if (n_layers < 0 || n_layers > net.g.layers) throw std::invalid_argument(std::string(WHO) + ": n_layers outside 0..depth");
    const size_t bytes = (size_t)n_seq * S * net.g.hidden * sizeof(float);
    QASR_HIP(hipMemcpyAsync(d_h_.p, x, bytes, hipMemcpyHostToDevice, work_));
    run_stack(net, n_seq, S, n_layers);
    if (n_layers == net.g.layers) {
        final_norm(net, n_seq * S, 1, 1, 0, d_act_.as<float>());
        QASR_HIP(hipMemcpyAsync(out, d_act_.p, bytes, hipMemcpyDeviceToHost, work_));
    } else {
        QASR_HIP(hipMemcpyAsync(out, d_h_.p, bytes, hipMemcpyDeviceToHost, work_));
    }
    end(2);
}

}  // namespace qasr
