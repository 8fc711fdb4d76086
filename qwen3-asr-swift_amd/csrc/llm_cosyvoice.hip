// llm_cosyvoice.hip -- the CosyVoice3 speech-token LLM (declarations and references: llm_cosyvoice.h).
//
// A step for all rows is one linear sequence of launches on one stream (per layer: q|k|v GEMV, RoPE + cache append, attention, o GEMV,
// gate|up GEMV, down GEMV; then head, sampler, next input), captured once per batch size and replayed per token; what changes between
// calls (sampling values, seed) lives in a device-side record, what changes between steps (position, count, finished) in per-row device
// state.  The prompt pass is the same sequence with rows = packed (slot, position) pairs.  No launch waits on another workgroup.
#include "llm_cosyvoice.h"
#include "dec_quant_dev.h"
#include "sample_dev.h"
#include "tuning.h"
#include <algorithm>
#include <cmath>
#include <cstring>

namespace qasr {

struct CosyLlm::State { int *pos, *count, *finished, *min_len, *max_tok; };

// ------------------------------------------------------------------------------------------------
// cvlm_gemvq_kernel: weight-streaming GEMV on the packed images of dec_quant.h for any K that is a multiple of 128.  A workgroup = NT
// 16-row weight tiles x 16 batch rows, 8 waves.  The arithmetic is decode_gemvq_kernel's: A = activations, B = weights, per 64-column
// group two 16x16x32 MFMAs from a zero accumulator, then tot += scale * acc + bias * xsum on the vector unit.  What differs is the
// geometry: K is a run-time value, the activation rows pass through an LDS image of CVLM_GEMV_PHASE columns per phase, and k-block
// `blk` of a row tile belongs to wave blk % 8 (7 or 38 blocks leave some waves a block short: they add nothing).  A wave adds its
// blocks in ascending order, the eight partials are added in wave order: the order is fixed by K alone.
// ------------------------------------------------------------------------------------------------
enum { CV_EPI_BF16 = 0, CV_EPI_RESID = 1, CV_EPI_SWIGLU = 2, CV_EPI_LOGITS = 3 };

struct CvGemvArgs {
    const uint32_t* qp; const void* sb;
    const bf16_t* X;                     // [B][K]
    int B, N, K;                         // N: rows of the image (a multiple of 16 NT)
    const bf16_t* norm_w; float eps;     // NORM
    const float* bias;                   // BF16: the Linear bias (bf16 values) or null
    bf16_t* out;                         // BF16 [B][N] | RESID in place [B][N] | SWIGLU [B][N / 2]
    float* logits; int ldl, n_valid;     // LOGITS: [B][ldl], rows n < n_valid
};

template <int BITS, bool SBF32, int NT, bool NORM, int EPI, int MAXB>
__global__ __launch_bounds__(512) void cvlm_gemvq_kernel(CvGemvArgs a) {
    constexpr int BLK = BITS == 4 ? 128 : 64, GPB = BLK / 64, PH = CVLM_GEMV_PHASE, XSTRIDE = 2 * PH + 16;
    constexpr int BPP = PH / BLK / 8;                                          // blocks of a wave per phase: 1 | 2
    constexpr int MAXP = MAXB / BPP;
    static_assert(MAXB % BPP == 0, "a wave's blocks fill whole phases");
    __shared__ __attribute__((aligned(16))) char s_x[16 * XSTRIDE];           // [16 rows][PH] bf16
    __shared__ __attribute__((aligned(16))) float s_xs[(PH / 64) * 16];       // [group][row] sums of the staged values
    __shared__ __attribute__((aligned(16))) float s_red[8 * NT * 256];        // [wave][tile][batch 16][n 16]
    const int K = a.K, G = K / 64, nblk = K / BLK, nch = K / 8, nph = (K + PH - 1) / PH;
    const int r0 = blockIdx.y * 16;
    const bf16_t* X = a.X + (long)r0 * K;
    const int Bt = a.B - r0 < 16 ? a.B - r0 : 16;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fc = lane >> 4;
    const int n0 = blockIdx.x * 16 * NT;
    const int srow = tid >> 5, scol = tid & 31;
    const bf16_t* xrow = X + (long)(srow < Bt ? srow : 0) * K;
    // ---- every packed block of this wave with the scales / biases of its groups ----------------------------------------------
    uint4 wq[NT][MAXB];
    float sc[NT][MAXB][GPB], bi[NT][MAXB][GPB];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const long tile = n0 / 16 + t;
        const uint32_t* qp = a.qp + (tile * nblk * 64 + lane) * 4;
#pragma unroll
        for (int i = 0; i < MAXB; ++i) {
            const int blk = wave + 8 * i;
            wq[t][i] = make_uint4(0, 0, 0, 0);
#pragma unroll
            for (int h = 0; h < GPB; ++h) { sc[t][i][h] = 0.0f; bi[t][i][h] = 0.0f; }
            if (blk < nblk) {
                wq[t][i] = *reinterpret_cast<const uint4*>(qp + (long)blk * 256);
                sb_load<SBF32, GPB>(a.sb, ((tile * 16 + fr) * G + blk * GPB) * 2, sc[t][i], bi[t][i]);
#pragma unroll
                for (int h = 0; h < GPB; ++h) bi[t][i][h] = eff_bias<BITS>(sc[t][i][h], bi[t][i][h]);
            }
        }
    }
    // ---- the activation rows: the first NPRE phases are requested here, behind the weights; a later phase takes the slot of the phase
    // NPRE before it as soon as that one is staged -----------------------------------------------------------------------------------
    constexpr int NPRE = MAXP < 5 ? MAXP : 5;
    uint4 xr[NPRE][4];
    auto load_phase = [&](int kp, uint4 (&dst)[4]) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = kp * (PH / 8) + scol + 32 * i;
            dst[i] = make_uint4(0, 0, 0, 0);
            if (c < nch && srow < Bt) dst[i] = *reinterpret_cast<const uint4*>(xrow + (long)c * 8);
        }
    };
#pragma unroll
    for (int kp = 0; kp < NPRE; ++kp)
        if (kp < nph) load_phase(kp, xr[kp]);
    // ---- the row statistic of the RMSNorm prologue: chunks scol, scol + 32, ... of the row in ascending order (from the registers when
    // the row is one phase: the same chunks in the same order), then the 32 partials ---------------------------------------------------
    float inv = 0.0f;
    if constexpr (NORM) {
        float ss = 0.0f;
        if (nph == 1) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const bf16_t* e = reinterpret_cast<const bf16_t*>(&xr[0][i]);
#pragma unroll
                for (int j = 0; j < 8; ++j) { const float f = bf16_to_f32(e[j]); ss = fmaf(f, f, ss); }
            }
        } else {
            for (int c = scol; c < nch; c += 32) {
                const uint4 v = *reinterpret_cast<const uint4*>(xrow + (long)c * 8);
                const bf16_t* e = reinterpret_cast<const bf16_t*>(&v);
#pragma unroll
                for (int j = 0; j < 8; ++j) { const float f = bf16_to_f32(e[j]); ss = fmaf(f, f, ss); }
            }
        }
        ss = lane_sum<32>(ss);
        inv = rsqrtf(ss / (float)K + a.eps);
    }
    const int erow = lane >> 2, eq = lane & 3;                                // epilogue lane map: batch row, four consecutive n
    f32x4 tot[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) tot[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    uint2 rsd[NT];                                                            // RESID: the residual, requested before the sweep
    if constexpr (EPI == CV_EPI_RESID) {
        if (wave == 0) {
#pragma unroll
            for (int t = 0; t < NT; ++t)
                rsd[t] = *reinterpret_cast<const uint2*>(a.out + (long)(r0 + (erow < Bt ? erow : 0)) * a.N + n0 + t * 16 + eq * 4);
        }
    }
#pragma unroll
    for (int kp = 0; kp < MAXP; ++kp) {
        if (kp < nph) {                                                        // workgroup-uniform
            if (kp > 0) __syncthreads();                                       // the previous phase's LDS reads are done
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int cl = scol + 32 * i, c = kp * (PH / 8) + cl;          // chunk within the phase, within the row
                uint4 o = xr[kp % NPRE][i];
                if constexpr (NORM) {
                    if (c < nch) {
                        const uint4 nw = reinterpret_cast<const uint4*>(a.norm_w)[c];
                        o = make_uint4(rmsnorm_pair_bf16(o.x, nw.x, inv), rmsnorm_pair_bf16(o.y, nw.y, inv),
                                       rmsnorm_pair_bf16(o.z, nw.z, inv), rmsnorm_pair_bf16(o.w, nw.w, inv));
                    }
                }
                *reinterpret_cast<uint4*>(s_x + (size_t)srow * XSTRIDE + cl * 16) = o;
                const bf16_t* oe = reinterpret_cast<const bf16_t*>(&o);
                float p = 0.0f;
#pragma unroll
                for (int j = 0; j < 8; ++j) p += bf16_to_f32(oe[j]);
                p = lane_sum8(p);                                              // the 8 chunks of a group sit on 8 adjacent lanes
                if ((scol & 7) == 0) s_xs[(cl >> 3) * 16 + srow] = p;
            }
            if (kp + NPRE < MAXP && kp + NPRE < nph) load_phase(kp + NPRE, xr[kp % NPRE]);
            __syncthreads();
#pragma unroll
            for (int ii = 0; ii < BPP; ++ii) {
                const int i = kp * BPP + ii;
                if (wave + 8 * i < nblk) {                         // wave-uniform
                    const int lb = wave + 8 * ii;                              // block within the phase
#pragma unroll
                    for (int h = 0; h < GPB; ++h) {
                        const int g = lb * GPB + h;                            // group within the phase
                        const f32x4 xs = *reinterpret_cast<const f32x4*>(s_xs + g * 16 + fc * 4);
                        const uint4 x0 = *reinterpret_cast<const uint4*>(s_x + (size_t)fr * XSTRIDE + ((g * 2 + 0) * 32 + fc * 8) * 2);
                        const uint4 x1 = *reinterpret_cast<const uint4*>(s_x + (size_t)fr * XSTRIDE + ((g * 2 + 1) * 32 + fc * 8) * 2);
#pragma unroll
                        for (int t = 0; t < NT; ++t) {
                            f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
                            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(mfma_bf16x8, x0), frag_of<BITS>(wq[t][i], 2 * h + 0), acc, 0, 0, 0);
                            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(mfma_bf16x8, x1), frag_of<BITS>(wq[t][i], 2 * h + 1), acc, 0, 0, 0);
#pragma unroll
                            for (int j = 0; j < 4; ++j) tot[t][j] += sc[t][i][h] * acc[j] + bi[t][i][h] * xs[j];
                        }
                    }
                }
            }
        }
    }
    // ---- cross-wave reduction in wave order through a [batch][n] image, epilogue on wave 0 ---------------------------------------
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) s_red[((size_t)(wave * NT + t) * 16 + fc * 4 + j) * 16 + fr] = tot[t][j];
    __syncthreads();
    if (wave != 0 || erow >= Bt) return;
    f32x4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int wv = 0; wv < 8; ++wv) acc[t] += *reinterpret_cast<const f32x4*>(s_red + ((size_t)(wv * NT + t) * 16 + erow) * 16 + eq * 4);
    }
    const long row = r0 + erow;
    if constexpr (EPI == CV_EPI_SWIGLU) {
        // rows come in blocks of 32: 16 gate rows then the 16 matching up rows -> tile pairs (2i, 2i + 1)
#pragma unroll
        for (int t = 0; t + 1 < NT; t += 2) {
            float4 v;
            v.x = gemm_swiglu(acc[t][0], acc[t + 1][0]); v.y = gemm_swiglu(acc[t][1], acc[t + 1][1]);
            v.z = gemm_swiglu(acc[t][2], acc[t + 1][2]); v.w = gemm_swiglu(acc[t][3], acc[t + 1][3]);
            *reinterpret_cast<uint2*>(a.out + row * (a.N / 2) + (n0 + t * 16) / 2 + eq * 4) = pack_bf16x4(v);
        }
    } else {
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int n = n0 + t * 16 + eq * 4;
            float4 v = make_float4(acc[t][0], acc[t][1], acc[t][2], acc[t][3]);
            if constexpr (EPI == CV_EPI_LOGITS) {
                const float ve[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (n + j < a.n_valid) a.logits[row * a.ldl + n + j] = ve[j];
            } else {
                bf16_t* p = a.out + row * a.N + n;
                if constexpr (EPI == CV_EPI_RESID) {
                    const float4 r = unpack_bf16x4(rsd[t]);
                    v.x = r.x + bf16_round(v.x); v.y = r.y + bf16_round(v.y); v.z = r.z + bf16_round(v.z); v.w = r.w + bf16_round(v.w);
                } else if (a.bias) {                                           // the reference's two roundings: bf16(bf16(acc) + bias)
                    const float4 b = *reinterpret_cast<const float4*>(a.bias + n);
                    v.x = bf16_round(v.x) + b.x; v.y = bf16_round(v.y) + b.y; v.z = bf16_round(v.z) + b.z; v.w = bf16_round(v.w) + b.w;
                }
                *reinterpret_cast<uint2*>(p) = pack_bf16x4(v);
            }
        }
    }
}

template <int BITS, bool SBF32, int NT, bool NORM, int EPI>
static void cvlm_gemv_go(const CvGemvArgs& a, hipStream_t s) {
    constexpr int BLK = BITS == 4 ? 128 : 64;
    const dim3 grid(a.N / (16 * NT), (a.B + 15) / 16);
    const int per_wave = (a.K / BLK + 7) / 8;
    if (per_wave <= 2) hipLaunchKernelGGL((cvlm_gemvq_kernel<BITS, SBF32, NT, NORM, EPI, 2>), grid, dim3(512), 0, s, a);
    else hipLaunchKernelGGL((cvlm_gemvq_kernel<BITS, SBF32, NT, NORM, EPI, CVLM_GEMV_MAXB>), grid, dim3(512), 0, s, a);
}

template <int BITS, bool SBF32>
static void cvlm_gemv_epi(int epi, const CvGemvArgs& a, hipStream_t s) {
    const bool norm = a.norm_w != nullptr;
    if (epi == CV_EPI_BF16 && norm) cvlm_gemv_go<BITS, SBF32, 1, true, CV_EPI_BF16>(a, s);
    else if (epi == CV_EPI_SWIGLU && norm) cvlm_gemv_go<BITS, SBF32, 2, true, CV_EPI_SWIGLU>(a, s);
    else if (epi == CV_EPI_RESID && !norm) cvlm_gemv_go<BITS, SBF32, 1, false, CV_EPI_RESID>(a, s);
    else if (epi == CV_EPI_LOGITS && norm) cvlm_gemv_go<BITS, SBF32, 1, true, CV_EPI_LOGITS>(a, s);
    else throw std::invalid_argument("cosyvoice llm: no GEMV form for this epilogue");
}

// what cvlm_gemvq_kernel serves; checked at create for every linear of the geometry
static void cvlm_gemv_check(int N, int K, int bits, int nt) {
    const int blk = bits == 4 ? 128 : 64;
    if (K < 128 || K % 128 != 0 || N % (16 * nt) != 0 || (K / blk + 7) / 8 > CVLM_GEMV_MAXB)
        throw std::invalid_argument("cosyvoice llm: a " + std::to_string(N) + " x " + std::to_string(K) + " linear at " + std::to_string(bits) +
                                    " bit is not served (K a multiple of 128, at most " + std::to_string(8 * CVLM_GEMV_MAXB * blk) +
                                    "; N a multiple of " + std::to_string(16 * nt) + ")");
}

// ------------------------------------------------------------------------------------------------
// cvlm_rope_append_kernel: row r at (slot[r], pos[r]): split-half RoPE on q and k at the rounding points of dec_rope.h (no q/k norm here),
// q -> qr [rows][heads][64], k and v -> the cache [slot][kv head][max_ctx][64].
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cvlm_rope_append_kernel(const bf16_t* __restrict__ qkv, const int* __restrict__ slot,
                                                               const int* __restrict__ pos, int heads, int kv_heads,
                                                               const float* __restrict__ cos_t, const float* __restrict__ sin_t,
                                                               bf16_t* __restrict__ qr, bf16_t* __restrict__ kc, bf16_t* __restrict__ vc,
                                                               int max_ctx) {
    constexpr int HD = 64, HALF = 32;
    const int r = blockIdx.x, sl = slot[r], ps = pos[r], nh = heads + 2 * kv_heads;
    const bf16_t* row = qkv + (long)r * nh * HD;
    for (int i = threadIdx.x; i < (heads + kv_heads) * HALF; i += 256) {
        const int h = i / HALF, d = i % HALF;
        const float x1 = bf16_to_f32(row[h * HD + d]), x2 = bf16_to_f32(row[h * HD + d + HALF]);
        const float c = cos_t[(long)ps * HALF + d], sn = sin_t[(long)ps * HALF + d];
        const bf16_t o1 = f32_to_bf16(x1 * c - x2 * sn), o2 = f32_to_bf16(x1 * sn + x2 * c);
        bf16_t* dst = h < heads ? qr + ((long)r * heads + h) * HD : kc + (((long)sl * kv_heads + (h - heads)) * max_ctx + ps) * HD;
        dst[d] = o1;
        dst[d + HALF] = o2;
    }
    for (int i = threadIdx.x; i < kv_heads * HD; i += 256) {
        const int h = i / HD, d = i % HD;
        vc[(((long)sl * kv_heads + h) * max_ctx + ps) * HD + d] = row[(heads + kv_heads + h) * HD + d];
    }
}

// ------------------------------------------------------------------------------------------------
// cvlm_attention_kernel: row r attends keys 0 .. pos[r] of slot[r]; one workgroup per (kv head, row) serves the rep <= 16 query heads
// of the kv head.  Keys go by rounds of CVLM_ATT_ROUND = 256: key j0 + t belongs to thread t (wave t / 64 owns a chunk of
// CVLM_ATT_CHUNK keys), which computes the rep scores of its key in f32 (d ascending).  Per round and head: the round's maximum, the
// online-softmax rescale, p = exp(s - m), the sum of the 256 p (4 per lane, then over the wave), then o += p V over the round's keys in
// key order, lane = d.  Head h is merged by wave h % 4.  Nothing here depends on the batch or on the context beyond pos[r].
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cvlm_attention_kernel(const bf16_t* __restrict__ qr, const int* __restrict__ slot,
                                                             const int* __restrict__ pos, int heads, int kv_heads,
                                                             const bf16_t* __restrict__ kc, const bf16_t* __restrict__ vc, int max_ctx,
                                                             bf16_t* __restrict__ out, float scale) {
    constexpr int HD = 64, RND = CVLM_ATT_ROUND, MAXREP = 16;
    __shared__ __attribute__((aligned(16))) float s_q[MAXREP][HD];
    __shared__ __attribute__((aligned(16))) float s_p[MAXREP][RND];
    __shared__ __attribute__((aligned(16))) bf16_t s_v[RND][HD];
    const int kvh = blockIdx.x, r = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rep = heads / kv_heads, sl = slot[r], ps = pos[r];
    const long base = ((long)sl * kv_heads + kvh) * max_ctx * HD;
    for (int i = tid; i < rep * HD; i += 256) s_q[i / HD][i % HD] = bf16_to_f32(qr[((long)r * heads + kvh * rep) * HD + i]);
    float o[4] = {0.f, 0.f, 0.f, 0.f}, m_run[4], l_run[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 4; ++i) m_run[i] = -INFINITY;
    __syncthreads();
    for (int j0 = 0; j0 <= ps; j0 += RND) {
        const int j = j0 + tid;
        const bool valid = j <= ps;
        uint4 kr[8], vr[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) { kr[c] = make_uint4(0, 0, 0, 0); vr[c] = make_uint4(0, 0, 0, 0); }
        if (valid) {
            const uint4* kp = reinterpret_cast<const uint4*>(kc + base + (long)j * HD);
            const uint4* vp = reinterpret_cast<const uint4*>(vc + base + (long)j * HD);
#pragma unroll
            for (int c = 0; c < 8; ++c) { kr[c] = kp[c]; vr[c] = vp[c]; }
        }
#pragma unroll
        for (int c = 0; c < 8; ++c) reinterpret_cast<uint4*>(&s_v[tid][0])[c] = vr[c];
        for (int h = 0; h < rep; ++h) {
            float s = 0.0f;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const bf16_t* ke = reinterpret_cast<const bf16_t*>(&kr[c]);
                const f32x4 q0 = *reinterpret_cast<const f32x4*>(&s_q[h][c * 8]), q1 = *reinterpret_cast<const f32x4*>(&s_q[h][c * 8 + 4]);
#pragma unroll
                for (int e = 0; e < 4; ++e) s += q0[e] * bf16_to_f32(ke[e]);
#pragma unroll
                for (int e = 0; e < 4; ++e) s += q1[e] * bf16_to_f32(ke[4 + e]);
            }
            s_p[h][tid] = valid ? s * scale : -INFINITY;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int h = wave + 4 * i;
            if (h < rep) {                                                     // wave-uniform
                const float a0 = s_p[h][lane], a1 = s_p[h][lane + 64], a2 = s_p[h][lane + 128], a3 = s_p[h][lane + 192];
                const float m_new = fmaxf(m_run[i], wave_max(fmaxf(fmaxf(a0, a1), fmaxf(a2, a3))));
                const float p0 = expf(a0 - m_new), p1 = expf(a1 - m_new), p2 = expf(a2 - m_new), p3 = expf(a3 - m_new);
                s_p[h][lane] = p0; s_p[h][lane + 64] = p1; s_p[h][lane + 128] = p2; s_p[h][lane + 192] = p3;
                const float alpha = expf(m_run[i] - m_new);                    // first round: exp(-inf) = 0
                l_run[i] = l_run[i] * alpha + wave_sum((p0 + p1) + (p2 + p3));
                o[i] *= alpha;
                m_run[i] = m_new;
            }
        }
        __syncthreads();
        const int nk = ps - j0 + 1 < RND ? ps - j0 + 1 : RND;
#pragma unroll 8
        for (int jj = 0; jj < nk; ++jj) {
            const float vv = bf16_to_f32(s_v[jj][lane]);
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (wave + 4 * i < rep) o[i] += s_p[wave + 4 * i][jj] * vv;
        }
        __syncthreads();                                                       // before the next round overwrites s_p / s_v
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int h = wave + 4 * i;
        if (h < rep) out[((long)r * heads + kvh * rep + h) * HD + lane] = f32_to_bf16(o[i] / l_run[i]);
    }
}

// the launch entries of the two kernels above (llm_cosyvoice.h): CosyLlm::layers and qasr_syn_attn_case_probe call these
void cvlm_rope_append_launch(const bf16_t* qkv, const int* slot, const int* pos, int rows, int heads, int kv_heads, const float* cos_t,
                             const float* sin_t, bf16_t* qr, bf16_t* kc, bf16_t* vc, int max_ctx, hipStream_t s) {
    if (rows <= 0) return;
    hipLaunchKernelGGL(cvlm_rope_append_kernel, dim3(rows), dim3(256), 0, s, qkv, slot, pos, heads, kv_heads, cos_t, sin_t, qr, kc, vc, max_ctx);
}

void cvlm_attention_launch(const bf16_t* qr, const int* slot, const int* pos, int rows, int heads, int kv_heads, const bf16_t* kc,
                           const bf16_t* vc, int max_ctx, bf16_t* out, hipStream_t s) {
    if (heads < 1 || kv_heads < 1 || heads % kv_heads != 0 || heads / kv_heads > 16)    // s_q[16][64]
        throw std::invalid_argument("cosyvoice llm: the attention kernel serves 1 .. 16 query heads per kv head, heads a multiple of kv_heads");
    if (rows <= 0) return;
    hipLaunchKernelGGL(cvlm_attention_kernel, dim3(kv_heads, rows), dim3(256), 0, s, qr, slot, pos, heads, kv_heads, kc, vc, max_ctx, out,
                       1.0f / sqrtf(64.0f));
}

// ------------------------------------------------------------------------------------------------
// The sampler: one workgroup per row, the row's logits and history window in LDS.  Steps as cvlm_sampler.cpp (the host twin) numbers
// them.  Top-k's threshold, the k-th largest value, is found exactly by bisection over an order-preserving integer key.  Top-p: the
// survivors (values above -1e9) are gathered, ranked by (value descending, index ascending) by counting, and thread 0 adds the
// exponentials one by one in that order -- the same route for 25 survivors and for 6761.
// ------------------------------------------------------------------------------------------------
struct CvlmSampleArgs {
    const float* logits;                 // [B][V]
    const CvlmSampleParams* knobs;
    const int* history; int hist_ld;     // [B][hist_ld]
    const int* n_history;                // [B]
    const int* step;                     // [B] or null: n_history
    const int* below;                    // [B] or null: n_history < min_len
    const int* min_len;
    const long long* row_index;
    int* out;                            // [B]
};

__device__ __forceinline__ bool cvlm_is_stop(int i, int st) { return i >= st && i < st + CVLM_STOPS; }

// logit i after steps 1 and 2
__device__ __forceinline__ float cvlm_masked(float v, int i, int st, int V, bool mask_stops) {
    if (i >= st && i < V && !cvlm_is_stop(i, st)) v = -1e9f;                                                            // 1
    if (mask_stops && cvlm_is_stop(i, st)) v = -1e9f;                                                                   // 2
    return v;
}

__global__ __launch_bounds__(1024) void cvlm_sample_kernel(CvlmSampleArgs a) {
    extern __shared__ __attribute__((aligned(16))) char dsm[];
    __shared__ float r_v[16];
    __shared__ int r_i[16], s_cnt[2][16], s_hist[CVLM_MAX_WIN], s_n;
    const int b = blockIdx.x, tid = threadIdx.x;
    const CvlmSampleParams p = *a.knobs;
    const int V = p.V, ST = p.speech_tokens;
    float* s_v = reinterpret_cast<float*>(dsm);                               // [V] the logits as masked so far
    float* s_sv = s_v + V;                                                    // [V] survivors in order: values
    int* s_si = reinterpret_cast<int*>(s_sv + V);                             // [V] ... indices
    int* s_ui = s_si + V;                                                     // [V] survivors as gathered
    const int nh = a.n_history[b];
    const int step = a.step ? a.step[b] : nh;
    const bool mask_stops = (a.below ? a.below[b] != 0 : nh < a.min_len[b]) || step == 0;
    const int win = p.win_size < nh ? p.win_size : nh;
    const float* row = a.logits + (long)b * V;
    for (int i = tid; i < V; i += 1024) s_v[i] = cvlm_masked(row[i], i, ST, V, mask_stops);
    if (tid < win) s_hist[tid] = a.history[(long)b * a.hist_ld + nh - win + tid];
    if (tid == 0) s_n = 0;
    __syncthreads();
    if (p.top_k > 0 && p.top_k < V) {                                                                                   // 3
        unsigned prefix = 0u;
        for (int bit = 31; bit >= 0; --bit) {
            const unsigned cand = prefix | (1u << bit);
            int c = 0;
            for (int i = tid; i < V; i += 1024) c += sample_order_key(s_v[i]) >= cand ? 1 : 0;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
            if ((tid & 63) == 0) s_cnt[bit & 1][tid >> 6] = c;
            __syncthreads();
            int total = 0;
            for (int w = 0; w < 16; ++w) total += s_cnt[bit & 1][w];
            if (total >= p.top_k) prefix = cand;
        }
        for (int i = tid; i < V; i += 1024)
            if (sample_order_key(s_v[i]) < prefix) s_v[i] = -1e9f;
        __syncthreads();
    }
    if (p.top_p < 1.0f) {                                                                                               // 4
        for (int i = tid; i < V; i += 1024)
            if (s_v[i] > -1e9f) s_ui[atomicAdd(&s_n, 1)] = i;
        __syncthreads();
        const int n = s_n;
        for (int e = tid; e < n; e += 1024) {
            const int i = s_ui[e];
            const float v = s_v[i];
            int rank = 0;
            for (int f = 0; f < n; ++f) {
                const int k = s_ui[f];
                const float w = s_v[k];
                rank += (w > v || (w == v && k < i)) ? 1 : 0;
            }
            s_sv[rank] = v;
            s_si[rank] = i;
        }
        __syncthreads();
        if (tid == 0 && n > 0) {
            const float mx = s_sv[0];
            float S = 0.0f;
            for (int e = 0; e < n; ++e) S += expf(s_sv[e] - mx);
            float cum = 0.0f;
            for (int e = 0; e < n; ++e) {
                const float pr = expf(s_sv[e] - mx) / S;
                cum += pr;
                if (cum - pr > p.top_p) s_v[s_si[e]] = -1e9f;
            }
        }
        __syncthreads();
    }
    int tok;
    {                                                                                                                   // 5
        const unsigned long long key = tts_stream_key(p.seed, a.row_index[b], step, 0);
        float bv = -INFINITY;
        int bi = 0x7fffffff;
        for (int i = tid; i < V; i += 1024) {
            const float v = s_v[i] - logf(-logf(tts_uniform(key, i)));
            if (v > bv || bi == 0x7fffffff) { bv = v; bi = i; }
        }
        tok = sample_block_argmax(bv, bi, r_v, r_i);
    }
    if (tok < 0 || tok >= V) tok = 0;                                         // all-NaN logits: keep the gather inside its table
    if (p.win_size > 0 && nh > 0) {                                                                                     // 6
        int cnt = 0;
        for (int i = 0; i < win; ++i) cnt += s_hist[i] == tok ? 1 : 0;
        if (cnt >= cvlm_ras_threshold(p.win_size, p.tau_r)) {                  // workgroup-uniform
            const unsigned long long key = tts_stream_key(p.seed, a.row_index[b], step, 1);
            float bv = -INFINITY;
            int bi = 0x7fffffff;
            for (int i = tid; i < V; i += 1024) {
                float v = cvlm_masked(row[i], i, ST, V, mask_stops);
                if (i == tok) v = -1e9f;
                v = v - logf(-logf(tts_uniform(key, i)));
                if (v > bv || bi == 0x7fffffff) { bv = v; bi = i; }
            }
            tok = sample_block_argmax(bv, bi, r_v, r_i);
            if (tok < 0 || tok >= V) tok = 0;
        }
    }
    if (tid == 0) a.out[b] = tok;
}

// ------------------------------------------------------------------------------------------------
// The next step of a row: the picked (or forced) token is stored unless it is a stop token, which finishes the row; the state moves on
// (position and count unless the row is finished or has reached its max_tokens); the token's speech embedding is the next input.
// ------------------------------------------------------------------------------------------------
struct CvlmNextArgs {
    CosyLlm::State st;
    const int* pick;
    const int* forced; int forced_T;     // [B][T] or null
    int* tokens; int ld;                 // [B][ld]
    const bf16_t* speech_emb; int H, V, speech_tokens;
    bf16_t* x;
};

__global__ __launch_bounds__(128) void cvlm_next_kernel(CvlmNextArgs a) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int cnt = a.st.count[b];
    const bool fin = a.st.finished[b] != 0;
    int tok = a.forced ? a.forced[(long)b * a.forced_T + (cnt < a.forced_T ? cnt : a.forced_T - 1)] : a.pick[b];
    if (tok < 0 || tok >= a.V) tok = 0;
    __syncthreads();                                                           // every thread has read the state
    if (tid == 0 && !fin) {
        if (!a.forced && cvlm_is_stop(tok, a.speech_tokens)) {
            a.st.finished[b] = 1;
        } else {
            if (cnt < a.ld) a.tokens[(long)b * a.ld + cnt] = tok;
            a.st.count[b] = cnt + 1;
            if (cnt + 1 >= a.st.max_tok[b]) a.st.finished[b] = 1;
            else a.st.pos[b] = a.st.pos[b] + 1;
        }
    }
    const uint4* src = reinterpret_cast<const uint4*>(a.speech_emb + (long)tok * a.H);
    uint4* dst = reinterpret_cast<uint4*>(a.x + (long)b * a.H);
    for (int i = tid; i < a.H / 8; i += 128) dst[i] = src[i];
}

// x[r] = the embedding of prefix[slot[r]][pos[r]]: a text id as it is, a speech id stored as -1 - id
__global__ __launch_bounds__(128) void cvlm_embed_kernel(const int* __restrict__ prefix, int ld, const int* __restrict__ slot,
                                                         const int* __restrict__ pos, const bf16_t* __restrict__ text_emb,
                                                         const bf16_t* __restrict__ speech_emb, int H, bf16_t* __restrict__ x) {
    const int r = blockIdx.x, id = prefix[(long)slot[r] * ld + pos[r]];
    const uint4* src = reinterpret_cast<const uint4*>(id >= 0 ? text_emb + (long)id * H : speech_emb + (long)(-1 - id) * H);
    uint4* dst = reinterpret_cast<uint4*>(x + (long)r * H);
    for (int i = threadIdx.x; i < H / 8; i += 128) dst[i] = src[i];
}

// forced pass: src [B][W] (f32 or bf16) -> dst[b][count[b]] rows of a [B][T][W] f32 array
__global__ __launch_bounds__(256) void cvlm_copy_out_kernel(const float* __restrict__ srcf, const bf16_t* __restrict__ srcb, int W,
                                                            const int* __restrict__ count, int T, float* __restrict__ dst) {
    const int b = blockIdx.x, f = count[b];
    if (f >= T) return;
    const long o = ((long)b * T + f) * W;
    for (int i = threadIdx.x; i < W; i += 256) dst[o + i] = srcf ? srcf[(long)b * W + i] : bf16_to_f32(srcb[(long)b * W + i]);
}

// ================================================================================================
// host
// ================================================================================================
static const char* const WHO = "cosyvoice llm";

int CosyLlm::context(const qasr_cvlm_config& c) {
    const long ctx = (2L + c.max_text + c.max_prompt_tokens + c.max_tokens + CVLM_ATT_CHUNK - 1) / CVLM_ATT_CHUNK * CVLM_ATT_CHUNK;
    return (int)std::min<long>(ctx, (long)CVLM_MAX_CTX + CVLM_ATT_CHUNK);
}

void CosyLlm::linear_shape(const qasr_cvlm_config& c, int kind, int& K, int& N) {
    const int nq = c.heads * c.head_dim, nkv = c.kv_heads * c.head_dim;
    switch (kind) {
        case CVLM_LIN_QKV: K = c.hidden; N = nq + 2 * nkv; break;
        case CVLM_LIN_O: K = nq; N = c.hidden; break;
        case CVLM_LIN_GATE_UP: K = c.hidden; N = c.inter; break;
        case CVLM_LIN_DOWN: K = c.inter; N = c.hidden; break;
        case CVLM_LIN_HEAD: K = c.hidden; N = c.speech_tokens + c.speech_extra; break;
        default: throw std::invalid_argument(std::string(WHO) + ": linear kind in 0..4 (qkv, o, gate_up, down, head)");
    }
}

void CosyLlm::check_geometry(const qasr_cvlm_config& c) {
    auto bad = [](const std::string& m) { throw std::invalid_argument(std::string(WHO) + ": " + m); };
    if (c.bits != 4 && c.bits != 8) bad("bits must be 4 or 8 (a float checkpoint is not served)");
    if (c.group_size != 64) bad("only group size 64 is supported");
    if (c.head_dim != 64) bad("head_dim must be 64 (the attention kernel is built for it)");
    if (c.heads < 1 || c.kv_heads < 1 || c.hidden != c.heads * 64) bad("hidden must equal heads * 64");
    if (c.heads % c.kv_heads != 0) bad("heads must be a multiple of kv_heads");
    if (c.heads / c.kv_heads > 16) bad("at most 16 query heads per kv head");
    if (c.hidden % 128 != 0 || c.inter < 128 || c.inter % 128 != 0) bad("hidden and inter must be multiples of 128");
    if (c.layers < 1) bad("layers must be positive");
    if (c.text_vocab < 1) bad("text_vocab must be positive");
    if (c.speech_tokens < 1 || c.speech_extra < CVLM_STOPS) bad("speech_tokens must be positive and speech_extra at least 3 (sos, eos, task_id)");
    if (c.speech_tokens + c.speech_extra > CVLM_MAX_VOCAB) bad("speech_tokens + speech_extra over " + std::to_string(CVLM_MAX_VOCAB));
    if (!(c.rms_eps > 0.0f) || !(c.rope_theta > 0.0f)) bad("rms_eps and rope_theta must be positive");
    if (c.max_batch < 1 || c.max_batch > CVLM_PASS_ROWS) bad("max_batch in 1..64");
    if (c.max_text < 1 || c.max_prompt_tokens < 0 || c.max_tokens < 1) bad("max_text and max_tokens at least 1, max_prompt_tokens not negative");
    if (2L + c.max_text + c.max_prompt_tokens + c.max_tokens > CVLM_MAX_CTX)
        bad("a context of 2 + max_text + max_prompt_tokens + max_tokens positions is over the limit of " + std::to_string(CVLM_MAX_CTX));
    // every linear of the step: there is no other GEMV kernel to fall to
    const int nq = c.heads * 64, nkv = c.kv_heads * 64, vpad = (c.speech_tokens + c.speech_extra + 15) / 16 * 16;
    cvlm_gemv_check(nq + 2 * nkv, c.hidden, c.bits, 1);
    cvlm_gemv_check(c.hidden, nq, c.bits, 1);
    cvlm_gemv_check(2 * c.inter, c.hidden, c.bits, 2);
    cvlm_gemv_check(c.hidden, c.inter, c.bits, 1);
    cvlm_gemv_check(vpad, c.hidden, c.bits, 1);
}

std::vector<int> CosyLlm::plan_prefix(const qasr_cvlm_config& c, const CvlmRow& r) {
    std::vector<int> p;
    p.reserve((size_t)2 + r.n_text + r.n_prompt);
    p.push_back(-1 - c.speech_tokens);                                         // sos
    for (int i = 0; i < r.n_text; ++i) p.push_back(r.text[i]);
    p.push_back(-1 - (c.speech_tokens + 2));                                   // task_id
    for (int i = 0; i < r.n_prompt; ++i) p.push_back(-1 - r.prompt[i]);
    return p;
}

// every tensor of llm.safetensors; a dry loader: the host checks alone (presence, shape, dtype of every key, no unexpected key)
void CosyLlm::load_all(const SafeTensorsDir& st, QlmLoader& wl) {
    const auto& c = cfg_;
    const int H = c.hidden, V = vocab();
    const QlmLayerGeom g{H, c.heads * c.head_dim, c.kv_heads * c.head_dim, c.inter, c.bits};
    layers_.clear();
    text_emb_ = wl.bf16(st, "text_embedding.weight", {c.text_vocab, H});
    speech_emb_ = wl.bf16(st, "speech_embedding.weight", {V, H});
    for (int l = 0; l < c.layers; ++l) {
        const std::string p = "layers." + std::to_string(l) + ".";
        Layer L = qlm_load_layer(wl, st, p, g, QlmBias::BF16);               // q, k and v carry a bias; float tensors are kept as bf16
        for (QLin* q : {&L.qkv, &L.o, &L.gu, &L.down}) wl.pack(*q);
        // named by the reference loader's comment and never loaded (WeightLoading.swift:28-29): present or not, they are not read
        wl.mark_seen(p + "self_attn.q_norm.weight");
        wl.mark_seen(p + "self_attn.k_norm.weight");
        layers_.push_back(L);
    }
    norm_ = wl.bf16(st, "norm.weight", {H});
    head_ = wl.qlin(st, {"speech_head"}, H, c.bits, QlmBias::NONE, 0, (V + 15) / 16 * 16);   // zero rows up to the GEMV's 16-row tiles
    if (head_.N != V) wl.refuse("speech_head holds " + std::to_string(head_.N) + " rows, expected " + std::to_string(V));
    wl.pack(head_);
    wl.refuse_unexpected(st);
}

CosyLlm::CosyLlm(const qasr_cvlm_config& cfg, const SafeTensorsDir& st, bool host_only) : cfg_(cfg) {
    check_geometry(cfg_);
    const auto& c = cfg_;
    {
        QlmLoader dry(WHO, nullptr, true);
        load_all(st, dry);                                                 // throws before any HIP call
    }
    if (host_only) return;
    QASR_HIP(hipSetDevice(c.device));
    QASR_HIP(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
    try {
        wl_ = std::make_unique<QlmLoader>(WHO, stream_, false);
        load_all(st, *wl_);
        const int MB = c.max_batch, R = CVLM_PASS_ROWS, H = c.hidden, half = c.head_dim / 2, V = vocab();
        const int nq = c.heads * c.head_dim, nkv = c.kv_heads * c.head_dim;
        max_ctx_ = context(c);
        max_prefix_ = 2 + c.max_text + c.max_prompt_tokens;
        std::vector<float> rc, rs;
        rope_tables_host(c.rope_theta, half, max_ctx_, rc, rs);
        d_cos_ = (float*)wl_->upload(rc.data(), rc.size() * 4);
        d_sin_ = (float*)wl_->upload(rs.data(), rs.size() * 4);
        const size_t kv_bytes = (size_t)c.layers * MB * c.kv_heads * max_ctx_ * c.head_dim * 2;
        d_k_ = (bf16_t*)wl_->upload(nullptr, kv_bytes);                      // the sweep reads keys 0 .. pos only: no zero fill
        d_v_ = (bf16_t*)wl_->upload(nullptr, kv_bytes);
        d_x_ = (bf16_t*)wl_->upload(nullptr, (size_t)R * H * 2);
        d_hn_ = (bf16_t*)wl_->upload(nullptr, (size_t)R * H * 2);
        d_qkv_ = (bf16_t*)wl_->upload(nullptr, (size_t)R * (nq + 2 * nkv) * 2);
        d_qr_ = (bf16_t*)wl_->upload(nullptr, (size_t)R * nq * 2);
        d_attn_ = (bf16_t*)wl_->upload(nullptr, (size_t)R * nq * 2);
        d_act_ = (bf16_t*)wl_->upload(nullptr, (size_t)R * c.inter * 2);
        d_res_ = (bf16_t*)wl_->upload(nullptr, (size_t)R * std::max({H, c.inter, nq + 2 * nkv}) * 2);
        d_logits_ = (float*)wl_->upload(nullptr, (size_t)R * V * 4);
        d_state_ = (int*)wl_->upload(nullptr, (size_t)5 * MB * 4);
        d_tokens_ = (int*)wl_->upload(nullptr, (size_t)R * c.max_tokens * 4);
        d_pick_ = (int*)wl_->upload(nullptr, (size_t)R * 4);
        d_prefix_ = (int*)wl_->upload(nullptr, (size_t)MB * max_prefix_ * 4);
        d_pairs_ = (int*)wl_->upload(nullptr, (size_t)2 * MB * max_prefix_ * 4);
        d_probe_ = (int*)wl_->upload(nullptr, (size_t)3 * R * 4);
        d_row_index_ = (long long*)wl_->upload(nullptr, (size_t)R * 8);
        d_knobs_ = (CvlmSampleParams*)wl_->upload(nullptr, sizeof(CvlmSampleParams));
        std::vector<int> iota(R);
        for (int i = 0; i < R; ++i) iota[i] = i;
        d_iota_ = (int*)wl_->upload(iota.data(), iota.size() * 4);
        ensure_dynamic_lds(reinterpret_cast<const void*>(cvlm_sample_kernel), 4 * CVLM_MAX_VOCAB * 4);
        QASR_HIP(hipStreamSynchronize(stream_));
    } catch (...) {
        wl_.reset();
        (void)hipStreamDestroy(stream_);
        stream_ = nullptr;
        throw;
    }
}

CosyLlm::~CosyLlm() {
    if (stream_) (void)hipStreamSynchronize(stream_);
    graphs_.drop();
    wl_.reset();
    for (auto& f : forced_buf_) f.reset();
    if (stream_) (void)hipStreamDestroy(stream_);
}

CosyLlm::State CosyLlm::state() const {
    const int MB = cfg_.max_batch;
    return State{d_state_, d_state_ + MB, d_state_ + 2 * MB, d_state_ + 3 * MB, d_state_ + 4 * MB};
}

void CosyLlm::gemv(int epi, const QLin& w, const bf16_t* X, int B, const bf16_t* norm_w, bf16_t* out, float* logits) {
    CvGemvArgs a{};
    a.qp = w.img.qp; a.sb = w.img.sb; a.X = X; a.B = B; a.N = w.img.raw.N; a.K = w.K;
    a.norm_w = norm_w; a.eps = cfg_.rms_eps; a.bias = w.bias; a.out = out; a.logits = logits; a.ldl = w.N; a.n_valid = w.N;
    if (B < 1 || B > CVLM_PASS_ROWS) throw std::length_error(std::string(WHO) + ": more than 64 rows in one launch");
    if (w.img.bits == 4) { if (w.img.sb_f32) cvlm_gemv_epi<4, true>(epi, a, stream_); else cvlm_gemv_epi<4, false>(epi, a, stream_); }
    else { if (w.img.sb_f32) cvlm_gemv_epi<8, true>(epi, a, stream_); else cvlm_gemv_epi<8, false>(epi, a, stream_); }
}

// `rows` rows of d_x_ through every layer, in place; row r sits at (slot[r], pos[r]) (device arrays).  last_kv_only: the last layer stops
// behind its cache append (a prompt position that is not a row's last needs nothing more of it).
void CosyLlm::layers(int rows, const int* slot, const int* pos, bool last_kv_only) {
    const auto& c = cfg_;
    const int MB = c.max_batch;
    const size_t per = (size_t)MB * c.kv_heads * max_ctx_ * c.head_dim;
    for (size_t l = 0; l < layers_.size(); ++l) {
        const Layer& L = layers_[l];
        bf16_t *kc = d_k_ + l * per, *vc = d_v_ + l * per;
        gemv(CV_EPI_BF16, L.qkv, d_x_, rows, L.ln1, d_qkv_, nullptr);
        cvlm_rope_append_launch(d_qkv_, slot, pos, rows, c.heads, c.kv_heads, d_cos_, d_sin_, d_qr_, kc, vc, max_ctx_, stream_);
        if (last_kv_only && l + 1 == layers_.size()) break;
        cvlm_attention_launch(d_qr_, slot, pos, rows, c.heads, c.kv_heads, kc, vc, max_ctx_, d_attn_, stream_);
        gemv(CV_EPI_RESID, L.o, d_attn_, rows, nullptr, d_x_, nullptr);
        gemv(CV_EPI_SWIGLU, L.gu, d_x_, rows, L.ln2, d_act_, nullptr);
        gemv(CV_EPI_RESID, L.down, d_act_, rows, nullptr, d_x_, nullptr);
    }
}

// One step of every row: the layers at the rows' positions, the head, the sampler (or the forced token), the next input.
void CosyLlm::issue_step(int B, bool forced_mode) {
    const auto& c = cfg_;
    State st = state();
    const int V = vocab();
    layers(B, d_iota_, st.pos, false);
    gemv(CV_EPI_LOGITS, head_, d_x_, B, norm_, nullptr, d_logits_);
    if (forced_mode) {
        if (d_f_log_) hipLaunchKernelGGL(cvlm_copy_out_kernel, dim3(B), dim3(256), 0, stream_, (const float*)d_logits_, (const bf16_t*)nullptr, V, (const int*)st.count, forced_T_, d_f_log_);
        if (d_f_hid_) {
            rmsnorm_rows_launch(d_x_, norm_, d_hn_, B, c.hidden, c.rms_eps, stream_);
            hipLaunchKernelGGL(cvlm_copy_out_kernel, dim3(B), dim3(256), 0, stream_, (const float*)nullptr, (const bf16_t*)d_hn_, c.hidden, (const int*)st.count, forced_T_, d_f_hid_);
        }
    } else {
        CvlmSampleArgs sa{};
        sa.logits = d_logits_; sa.knobs = d_knobs_; sa.history = d_tokens_; sa.hist_ld = c.max_tokens; sa.n_history = st.count;
        sa.step = nullptr; sa.below = nullptr; sa.min_len = st.min_len; sa.row_index = d_row_index_; sa.out = d_pick_;
        hipLaunchKernelGGL(cvlm_sample_kernel, dim3(B), dim3(1024), (size_t)4 * V * 4, stream_, sa);
    }
    CvlmNextArgs na{};
    na.st = st; na.pick = d_pick_; na.forced = forced_mode ? d_f_tok_ : nullptr; na.forced_T = forced_T_;
    na.tokens = d_tokens_; na.ld = c.max_tokens; na.speech_emb = speech_emb_; na.H = c.hidden; na.V = V; na.speech_tokens = c.speech_tokens;
    na.x = d_x_;
    hipLaunchKernelGGL(cvlm_next_kernel, dim3(B), dim3(128), 0, stream_, na);
    QASR_HIP(hipGetLastError());
}

void CosyLlm::run_step(int B) {
    graphs_.run(B, stream_, [&] { issue_step(B, false); });
}

// buildInputSequence for every row, the rows' state, then every prefix position but a row's last through the layers: packed (slot,
// position) pairs, CVLM_PASS_ROWS per pass (knob cvlm_prompt_chunk = 64), or one position of every row per pass (= 1).  A row's last
// prefix position is the input of its step 0.
void CosyLlm::prefill(const std::vector<CvlmRow>& rows, const qasr_cvlm_sampling* s, int forced_T) {
    const auto& c = cfg_;
    const int B = (int)rows.size(), MB = c.max_batch, P = max_prefix_;
    std::vector<int> prefix((size_t)B * P, 0), st((size_t)5 * MB, 0), len(B);
    std::vector<long long> ridx(CVLM_PASS_ROWS, 0);
    int Pmax = 0;
    for (int b = 0; b < B; ++b) {
        const std::vector<int> p = plan_prefix(c, rows[b]);
        if ((int)p.size() > P) throw std::length_error(std::string(WHO) + ": a prefix over the handle's capacity");
        std::copy(p.begin(), p.end(), prefix.begin() + (size_t)b * P);
        len[b] = (int)p.size();
        Pmax = std::max(Pmax, len[b]);
        ridx[b] = rows[b].index;
        st[(size_t)0 * MB + b] = len[b] - 1;                                   // position of step 0
        st[(size_t)3 * MB + b] = s ? (int)((float)rows[b].content_len * s->min_ratio) : 0;
        st[(size_t)4 * MB + b] = forced_T > 0 ? forced_T + 1 : rows[b].max_tokens;
    }
    for (int b = B; b < MB; ++b) st[(size_t)2 * MB + b] = 1;
    std::vector<int> pslot, ppos;
    std::vector<std::pair<int, int>> passes;                                   // (first pair, rows)
    if (tuning().cvlm_prompt_chunk == 1) {
        for (int i = 0; i + 1 < Pmax; ++i) {
            const int first = (int)pslot.size();
            for (int b = 0; b < B; ++b)
                if (i + 1 < len[b]) { pslot.push_back(b); ppos.push_back(i); }
            passes.push_back({first, (int)pslot.size() - first});
        }
    } else {
        for (int b = 0; b < B; ++b)
            for (int i = 0; i + 1 < len[b]; ++i) { pslot.push_back(b); ppos.push_back(i); }
        for (int first = 0; first < (int)pslot.size(); first += CVLM_PASS_ROWS)
            passes.push_back({first, std::min(CVLM_PASS_ROWS, (int)pslot.size() - first)});
    }
    const int n = (int)pslot.size();
    if (n > MB * P) throw std::length_error(std::string(WHO) + ": packed prompt over the handle's capacity");
    QASR_HIP(hipMemcpyAsync(d_prefix_, prefix.data(), prefix.size() * 4, hipMemcpyHostToDevice, stream_));
    QASR_HIP(hipMemcpyAsync(d_state_, st.data(), st.size() * 4, hipMemcpyHostToDevice, stream_));
    QASR_HIP(hipMemcpyAsync(d_row_index_, ridx.data(), ridx.size() * 8, hipMemcpyHostToDevice, stream_));
    QASR_HIP(hipMemsetAsync(d_tokens_, 0xff, (size_t)CVLM_PASS_ROWS * c.max_tokens * 4, stream_));
    int *d_slot = d_pairs_, *d_pos = d_pairs_ + (size_t)MB * P;
    if (n) {
        QASR_HIP(hipMemcpyAsync(d_slot, pslot.data(), (size_t)n * 4, hipMemcpyHostToDevice, stream_));
        QASR_HIP(hipMemcpyAsync(d_pos, ppos.data(), (size_t)n * 4, hipMemcpyHostToDevice, stream_));
    }
    for (const auto& ps : passes) {
        if (ps.second == 0) continue;
        hipLaunchKernelGGL(cvlm_embed_kernel, dim3(ps.second), dim3(128), 0, stream_, (const int*)d_prefix_, P, (const int*)(d_slot + ps.first),
                           (const int*)(d_pos + ps.first), text_emb_, speech_emb_, c.hidden, d_x_);
        layers(ps.second, d_slot + ps.first, d_pos + ps.first, true);
    }
    State sd = state();
    hipLaunchKernelGGL(cvlm_embed_kernel, dim3(B), dim3(128), 0, stream_, (const int*)d_prefix_, P, (const int*)d_iota_, (const int*)sd.pos,
                       text_emb_, speech_emb_, c.hidden, d_x_);
    QASR_HIP(hipGetLastError());
    QASR_HIP(hipStreamSynchronize(stream_));                                // the host vectors above go out of scope
}

void CosyLlm::set_knobs(const qasr_cvlm_sampling& s, unsigned long long seed) {
    const CvlmSampleParams k{s.top_k, s.top_p, s.win_size, s.tau_r, vocab(), cfg_.speech_tokens, seed};
    QASR_HIP(hipMemcpyAsync(d_knobs_, &k, sizeof(k), hipMemcpyHostToDevice, stream_));
    QASR_HIP(hipStreamSynchronize(stream_));
}

void CosyLlm::generate(const std::vector<CvlmRow>& rows, const qasr_cvlm_sampling& s, unsigned long long seed, int32_t* tokens, int32_t* n_tokens) {
    const int B = (int)rows.size(), F = cfg_.max_tokens;
    if (B == 0) return;
    QASR_HIP(hipSetDevice(cfg_.device));
    set_knobs(s, seed);
    prefill(rows, &s, 0);
    int steps = 0;
    for (const CvlmRow& r : rows) steps = std::max(steps, r.max_tokens);
    std::vector<int> fin(B);
    State st = state();
    for (int f = 0; f < steps; ++f) {
        run_step(B);
        if ((f + 1) % CVLM_POLL == 0 && f + 1 < steps) {                     // the finished flags, every CVLM_POLL steps
            QASR_HIP(hipMemcpyAsync(fin.data(), st.finished, (size_t)B * 4, hipMemcpyDeviceToHost, stream_));
            QASR_HIP(hipStreamSynchronize(stream_));
            if (std::all_of(fin.begin(), fin.end(), [](int v) { return v != 0; })) break;
        }
    }
    // steps computed behind a row's end (up to the next poll) stored nothing: a finished row writes no token
    std::vector<int> h((size_t)B * F);
    QASR_HIP(hipMemcpyAsync(h.data(), d_tokens_, h.size() * 4, hipMemcpyDeviceToHost, stream_));
    QASR_HIP(hipMemcpyAsync(n_tokens, st.count, (size_t)B * 4, hipMemcpyDeviceToHost, stream_));
    QASR_HIP(hipStreamSynchronize(stream_));
    for (int b = 0; b < B; ++b)
        for (int t = 0; t < F; ++t) tokens[(size_t)b * F + t] = t < n_tokens[b] ? h[(size_t)b * F + t] : -1;
}

void CosyLlm::forced(const std::vector<CvlmRow>& rows, const int32_t* tokens, int T, float* logits, float* hidden) {
    const int B = (int)rows.size(), V = vocab(), H = cfg_.hidden;
    if (B == 0 || T == 0) return;
    QASR_HIP(hipSetDevice(cfg_.device));
    const size_t n_tok = (size_t)B * T, n_l = (size_t)B * T * V, n_h = (size_t)B * T * H;
    for (auto& fb : forced_buf_) fb = std::make_unique<DevBuf>();
    forced_buf_[0]->alloc(n_tok * 4);
    d_f_tok_ = forced_buf_[0]->as<int>();
    d_f_log_ = d_f_hid_ = nullptr;
    if (logits) { forced_buf_[1]->alloc(n_l * 4); d_f_log_ = forced_buf_[1]->as<float>(); }
    if (hidden) { forced_buf_[2]->alloc(n_h * 4); d_f_hid_ = forced_buf_[2]->as<float>(); }
    forced_T_ = T;
    QASR_HIP(hipMemcpyAsync(d_f_tok_, tokens, n_tok * 4, hipMemcpyHostToDevice, stream_));
    prefill(rows, nullptr, T);
    for (int t = 0; t < T; ++t) issue_step(B, true);
    if (logits) QASR_HIP(hipMemcpyAsync(logits, d_f_log_, n_l * 4, hipMemcpyDeviceToHost, stream_));
    if (hidden) QASR_HIP(hipMemcpyAsync(hidden, d_f_hid_, n_h * 4, hipMemcpyDeviceToHost, stream_));
    QASR_HIP(hipStreamSynchronize(stream_));
    for (auto& fb : forced_buf_) fb.reset();
    d_f_tok_ = nullptr; d_f_log_ = d_f_hid_ = nullptr;
}

void CosyLlm::sample(int B, const float* logits, const int32_t* const* history, const int32_t* n_history, const int32_t* step,
                     const int32_t* below_min, const qasr_cvlm_sampling& s, unsigned long long seed, const int64_t* row_index, int32_t* out) {
    const int V = vocab(), F = cfg_.max_tokens;
    if (B == 0) return;
    QASR_HIP(hipSetDevice(cfg_.device));
    set_knobs(s, seed);
    std::vector<int> hist((size_t)B * F, -1), meta((size_t)3 * CVLM_PASS_ROWS, 0);
    std::vector<long long> ridx(CVLM_PASS_ROWS, 0);
    for (int b = 0; b < B; ++b) {
        for (int i = 0; i < n_history[b]; ++i) hist[(size_t)b * F + i] = history[b][i];
        meta[b] = n_history[b];
        meta[CVLM_PASS_ROWS + b] = step[b];
        meta[2 * CVLM_PASS_ROWS + b] = below_min[b];
        ridx[b] = row_index ? row_index[b] : b;
    }
    QASR_HIP(hipMemcpyAsync(d_logits_, logits, (size_t)B * V * 4, hipMemcpyHostToDevice, stream_));
    QASR_HIP(hipMemcpyAsync(d_tokens_, hist.data(), hist.size() * 4, hipMemcpyHostToDevice, stream_));
    QASR_HIP(hipMemcpyAsync(d_probe_, meta.data(), meta.size() * 4, hipMemcpyHostToDevice, stream_));
    QASR_HIP(hipMemcpyAsync(d_row_index_, ridx.data(), ridx.size() * 8, hipMemcpyHostToDevice, stream_));
    CvlmSampleArgs sa{};
    sa.logits = d_logits_; sa.knobs = d_knobs_; sa.history = d_tokens_; sa.hist_ld = F; sa.n_history = d_probe_;
    sa.step = d_probe_ + CVLM_PASS_ROWS; sa.below = d_probe_ + 2 * CVLM_PASS_ROWS; sa.min_len = nullptr; sa.row_index = d_row_index_;
    sa.out = d_pick_;
    hipLaunchKernelGGL(cvlm_sample_kernel, dim3(B), dim3(1024), (size_t)4 * V * 4, stream_, sa);
    QASR_HIP(hipGetLastError());
    QASR_HIP(hipMemcpyAsync(out, d_pick_, (size_t)B * 4, hipMemcpyDeviceToHost, stream_));
    QASR_HIP(hipStreamSynchronize(stream_));
}

void CosyLlm::linear_probe(int layer, int kind, int B, const float* x, const float* resid, float* y) {
    const auto& c = cfg_;
    int K = 0, N = 0;
    linear_shape(c, kind, K, N);
    if (kind != CVLM_LIN_HEAD && (layer < 0 || layer >= c.layers)) throw std::invalid_argument(std::string(WHO) + ": layer outside the model");
    QASR_HIP(hipSetDevice(c.device));
    const bool res = kind == CVLM_LIN_O || kind == CVLM_LIN_DOWN;
    if (res && !resid) throw std::invalid_argument(std::string(WHO) + ": the o and down linears add to a residual: resid is NULL");
    bf16_t* in = kind == CVLM_LIN_O ? d_attn_ : kind == CVLM_LIN_DOWN ? d_act_ : d_x_;
    std::vector<bf16_t> hx((size_t)B * K), hr;
    for (size_t i = 0; i < hx.size(); ++i) hx[i] = f32_to_bf16_host(x[i]);
    QASR_HIP(hipMemcpyAsync(in, hx.data(), hx.size() * 2, hipMemcpyHostToDevice, stream_));
    if (res) {
        hr.resize((size_t)B * N);
        for (size_t i = 0; i < hr.size(); ++i) hr[i] = f32_to_bf16_host(resid[i]);
        QASR_HIP(hipMemcpyAsync(d_res_, hr.data(), hr.size() * 2, hipMemcpyHostToDevice, stream_));
    }
    const Layer* L = kind == CVLM_LIN_HEAD ? nullptr : &layers_[layer];
    switch (kind) {
        case CVLM_LIN_QKV: gemv(CV_EPI_BF16, L->qkv, in, B, L->ln1, d_res_, nullptr); break;
        case CVLM_LIN_O: gemv(CV_EPI_RESID, L->o, in, B, nullptr, d_res_, nullptr); break;
        case CVLM_LIN_GATE_UP: gemv(CV_EPI_SWIGLU, L->gu, in, B, L->ln2, d_res_, nullptr); break;
        case CVLM_LIN_DOWN: gemv(CV_EPI_RESID, L->down, in, B, nullptr, d_res_, nullptr); break;
        default: gemv(CV_EPI_LOGITS, head_, in, B, norm_, nullptr, d_logits_); break;
    }
    QASR_HIP(hipGetLastError());
    if (kind == CVLM_LIN_HEAD) {
        QASR_HIP(hipMemcpyAsync(y, d_logits_, (size_t)B * N * 4, hipMemcpyDeviceToHost, stream_));
        QASR_HIP(hipStreamSynchronize(stream_));
        return;
    }
    std::vector<bf16_t> hy((size_t)B * N);
    QASR_HIP(hipMemcpyAsync(hy.data(), d_res_, hy.size() * 2, hipMemcpyDeviceToHost, stream_));
    QASR_HIP(hipStreamSynchronize(stream_));
    for (size_t i = 0; i < hy.size(); ++i) y[i] = bf16_to_f32_host(hy[i]);
}

}  // namespace qasr
