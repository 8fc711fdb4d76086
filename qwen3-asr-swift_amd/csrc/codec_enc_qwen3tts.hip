// codec_enc_qwen3tts.hip -- the Qwen3-TTS speech tokenizer encoder for gfx950 (codec_enc_qwen3tts.h).  f32 throughout, accurate sinf /
// expf / erff / sqrtf, no atomics, no vendor BLAS.
//
// A pass holds clips back to back.  A clip of n samples owns len[l] = ceil(n / rate[l]) rows of the tensors at level l (rates 1, 3, 12,
// 60, 480, 960, 1920): the lengths are ceilings, not multiples of one another, so every level has its own table start[l][clip] of first
// rows (start[l][clips] = the level's row count) and a kernel finds a row's clip by bisection.  Row and element indices are 64-bit.
// Launches of a pass:
//   cenc_in_kernel      the 1 -> C k = 7 conv as a 7-term dot, one thread per output element, 96-wide rows stored coalesced
//   codec_gemm_kernel   the decoder's GEMM (codec_shared.h: 64 x 64 f32 tile, k = taps outer, channels inner, one fmaf chain per output,
//                       the same epilogues) with the row locator ClipRows, which adds a stride: the A element of (output row t of a
//                       clip, tap j, channel c) is x[t s - (taps - 1 - j) dilation][c] of the same clip one level up, exact zero before
//                       the clip's first row, SnakeBeta optionally applied as it is loaded.  Runs every conv but the first, every
//                       Linear and the RVQ projections.
//   codec_rms_kernel, codec_dwln_kernel   (codec_shared.h) RMSNorm; depthwise k = 7 causal conv + LayerNorm; one workgroup per row
//   cenc_attn_kernel    unmasked attention over a whole clip, flash-style: a workgroup owns 32 queries of one clip and one head, streams
//                       the clip's K / V in tiles of 32 through LDS (RoPE on the way in, rotate-halves, positions from 0) with a running
//                       max and sum
//   cenc_vq_kernel      ResidualVectorQuantizer.encode: a workgroup owns 64 frames of one quantizer and walks its codebooks in order;
//                       per codebook the [64][size] score GEMM in the same tile, the distance in the reference's expanded form, a
//                       (value, index) argmin, then the residual update in place
// Summation order: every GEMM output is one thread's fmaf chain over k = 0..K-1; the norms are the decoder's
// kernels; an attention output row is accumulated over the clip's keys in order, tile after tile from the clip's first frame.  No
// reduction crosses a clip and nothing depends on a clip's place, so a clip's latent and codes are the same bits alone, in any batch and
// under any split into passes.
#include "codec_enc_qwen3tts.h"
#include <algorithm>
#include <cmath>
#include <cstring>

namespace qasr {

// ---- geometry, keys, lengths (host) -------------------------------------------------------------------------------------------------
void codec_enc_strides(const CodecGeom& g, int s[6]) {
    for (int i = 0; i < 4; ++i) s[i] = g.rates[3 - i];
    s[4] = g.ratios[1]; s[5] = g.ratios[0];
}

void codec_enc_lengths(const CodecGeom& g, long n, long len[CENC_LEVELS]) {
    int s[6];
    codec_enc_strides(g, s);
    len[0] = n;
    for (int l = 0; l < 6; ++l) len[l + 1] = (len[l] + s[l] - 1) / s[l];
}

CodecShapes codec_enc_tensor_shapes(const CodecGeom& g, const std::vector<bool>& embed_stored) {
    CodecShapes s;
    auto add = [&](const std::string& k, std::vector<int64_t> sh) { s.emplace_back(k, std::move(sh)); };
    const int64_t L = g.latent, H = g.hidden, Dd = g.decoder_dim, D = g.codebook_dim;
    int st[6];
    codec_enc_strides(g, st);
    for (int q = 0; q < g.quantizers; ++q) {
        const int64_t n = q == 0 ? g.semantic_size : g.acoustic_size;
        const std::string p = codec_codebook_prefix("encoder", q);
        if (embed_stored[q]) add(p + ".embed", {n, D});
        else { add(p + ".embedding_sum", {n, D}); add(p + ".cluster_usage", {n}); }
    }
    // the [hidden][codebook_dim] matrix ResidualVectorQuantizer.encode multiplies by (:472-475), stored as the module holds it
    add("encoder.quantizer.rvq_first.input_proj.weight", {H, D, 1});
    add("encoder.quantizer.rvq_rest.input_proj.weight", {H, D, 1});
    int64_t c = Dd / 16;
    add("encoder.encoder.0.conv.weight", {c, 1, 7}); add("encoder.encoder.0.conv.bias", {c});
    for (int b = 0; b < 4; ++b) {
        const std::string p = "encoder.encoder." + std::to_string(b + 1) + ".block.";
        for (int j = 0; j < 3; ++j) {
            const std::string u = p + std::to_string(j) + ".";
            for (const char* a : {"act1", "act2"}) { add(u + a + ".alpha", {c}); add(u + a + ".beta", {c}); }
            add(u + "conv1.conv.weight", {c, c, 7}); add(u + "conv1.conv.bias", {c});
            add(u + "conv2.conv.weight", {c, c, 1}); add(u + "conv2.conv.bias", {c});
        }
        add(p + "3.alpha", {c}); add(p + "3.beta", {c});
        add(p + "4.conv.weight", {2 * c, c, 2 * st[b]}); add(p + "4.conv.bias", {2 * c});
        c *= 2;
    }
    add("encoder.encoder.5.conv.weight", {L, Dd, 7}); add("encoder.encoder.5.conv.bias", {L});
    for (int i = 0; i < 2; ++i) {
        const std::string p = "encoder.downsample." + std::to_string(i) + ".";
        add(p + "0.dwconv.conv.weight", {L, 1, 7}); add(p + "0.dwconv.conv.bias", {L});
        add(p + "0.norm.weight", {L}); add(p + "0.norm.bias", {L});
        add(p + "0.pwconv1.weight", {4 * L, L}); add(p + "0.pwconv1.bias", {4 * L});
        add(p + "0.pwconv2.weight", {L, 4 * L}); add(p + "0.pwconv2.bias", {L});
        add(p + "0.gamma", {L});
        add(p + "1.conv.weight", {L, L, 2 * st[4 + i]}); add(p + "1.conv.bias", {L});
    }
    add("encoder.post_conv.conv.weight", {L, L, 3}); add("encoder.post_conv.conv.bias", {L});
    // output_proj is read by the reference's loader, never applied (:100)
    codec_pre_transformer_shapes(s, "encoder.pre_transformer.", g);
    return s;
}

// ---- kernels ------------------------------------------------------------------------------------------------------------------------
constexpr int AT_Q = 32, AT_K = 32;

// y[m][c] = b[c] + sum_j w[j][c] x[m - (6 - j)] inside the clip (:224); x [M], w [7][C], y [M][C]; one thread per (m, c)
__global__ __launch_bounds__(ROW_THREADS) void cenc_in_kernel(const float* __restrict__ x, long M, int C, const int* __restrict__ start,
                                                              int nclips, const float* __restrict__ w, const float* __restrict__ b,
                                                              float* __restrict__ y) {
    const long e = (long)blockIdx.x * ROW_THREADS + threadIdx.x;
    if (e >= M * C) return;
    const long m = e / C;
    const int c = (int)(e - m * C);
    const long first = start[clip_of(start, nclips, m)];
    float acc = 0.0f;
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        const long src = m - (6 - j);
        acc = fmaf(src >= first ? x[src] : 0.0f, w[j * C + c], acc);
    }
    y[e] = acc + b[c];
}

// the kernel's launch entry (codec_launch.h): CodecEncQwen3TTS::dev_convs and qasr_codec_case_probe call this
void cenc_in_launch(const float* pcm, long M, int C, const int* start, int nclips, const float* w, const float* b, float* y, hipStream_t s) {
    hipLaunchKernelGGL(cenc_in_kernel, dim3((unsigned)cdiv(M * C, ROW_THREADS)), dim3(ROW_THREADS), 0, s, pcm, M, C, start, nclips, w, b, y);
}

// qkv [M][3 A] (A = heads x 64); tiles[b] = (the clip's first row, its frames, the tile's first query); rope [positions][32] (cos, sin);
// out [M][A].  grid (query tiles, heads).  Thread (i = tid / 8, g = tid % 8) owns outputs 8 g .. 8 g + 7 of query i: per K / V tile the
// 32 x 32 scores go through LDS, then the row's running max m, sum l and accumulators are updated over the tile's keys in order (the
// eight threads of a row compute the same m and l).  Keys past the clip's last frame are never read.
__global__ __launch_bounds__(ROW_THREADS) void cenc_attn_kernel(const float* __restrict__ qkv, const int4* __restrict__ tiles,
                                                                const float2* __restrict__ rope, int heads, float* __restrict__ out) {
    __shared__ float sq[AT_Q][64], sk[AT_K][65], sv[AT_K][64], sp[AT_Q][AT_K + 1];
    const int tid = threadIdx.x, h = blockIdx.y, A = heads * 64;
    const int4 tile = tiles[blockIdx.x];
    const long row0 = tile.x;
    const int F = tile.y, q0 = tile.z, nq = min(AT_Q, F - q0);
    for (int i = tid; i < AT_Q * 32; i += ROW_THREADS) {               // MLXNN.RoPE traditional: false: element d pairs with d + 32
        const int t = i >> 5, d = i & 31;
        float a = 0.0f, b = 0.0f;
        if (t < nq) {
            const float* base = qkv + (row0 + q0 + t) * 3 * A + h * 64;
            const float2 cs = rope[(q0 + t) * 32 + d];
            const float q1 = base[d], q2 = base[d + 32];
            a = q1 * cs.x - q2 * cs.y; b = q1 * cs.y + q2 * cs.x;
        }
        sq[t][d] = a; sq[t][d + 32] = b;
    }
    const int qi = tid >> 3, dg = (tid & 7) * 8;
    float mx = -INFINITY, sum = 0.0f, acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.0f;
    for (int k0 = 0; k0 < F; k0 += AT_K) {
        const int nk = min(AT_K, F - k0);
        __syncthreads();                                               // the previous tile is consumed (and sq is written)
        for (int i = tid; i < nk * 32; i += ROW_THREADS) {
            const int t = i >> 5, d = i & 31;
            const float* base = qkv + (row0 + k0 + t) * 3 * A + A + h * 64;
            const float2 cs = rope[(k0 + t) * 32 + d];
            const float k1 = base[d], k2 = base[d + 32];
            sk[t][d] = k1 * cs.x - k2 * cs.y; sk[t][d + 32] = k1 * cs.y + k2 * cs.x;
        }
        for (int i = tid; i < nk * 64; i += ROW_THREADS) sv[i >> 6][i & 63] = qkv[(row0 + k0 + (i >> 6)) * 3 * A + 2 * A + h * 64 + (i & 63)];
        __syncthreads();
#pragma unroll
        for (int r = 0; r < AT_K / 8; ++r) {
            const int j = (tid & 7) + 8 * r;
            if (j >= nk) continue;
            float s = 0.0f;
#pragma unroll 8
            for (int d = 0; d < 64; ++d) s = fmaf(sq[qi][d], sk[j][d], s);
            sp[qi][j] = s * 0.125f;
        }
        __syncthreads();
        float tmax = sp[qi][0];
        for (int j = 1; j < nk; ++j) tmax = fmaxf(tmax, sp[qi][j]);
        const float nmx = fmaxf(mx, tmax), scale = expf(mx - nmx);     // first tile: exp(-inf) = 0 on zero accumulators
        sum = sum * scale;
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = acc[e] * scale;
        for (int j = 0; j < nk; ++j) {
            const float p = expf(sp[qi][j] - nmx);
            sum = sum + p;
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] = fmaf(p, sv[j][dg + e], acc[e]);
        }
        mx = nmx;
    }
    if (qi < nq) {
#pragma unroll
        for (int e = 0; e < 8; ++e) out[(row0 + q0 + qi) * A + h * 64 + dg + e] = acc[e] / sum;
    }
}

// ResidualVectorQuantizer.encode (:467-485) after the projection.  r [M][ldr]: the residual of chain 0 (rvq_first, 1 codebook) in
// columns 0 .. D - 1, of chain 1 (rvq_rest, Q - 1 codebooks) in columns D .. 2 D - 1.  cb [stage][S][D], cbt [stage][D][S], csq
// [stage][S] = |c|^2.  Per stage: code = argmin_n (|r|^2 - 2 r.c_n) + |c_n|^2 (:417-423), the lowest n among equal values, then
// r -= cb[code].  codes [M][Q].  grid (frame tiles of 64, 2); a workgroup reads and writes only its own rows of r.
__global__ __launch_bounds__(CG_THREADS) void cenc_vq_kernel(float* r, long M, int ldr, int D, int Q, const float* __restrict__ cb0,
                                                             const float* __restrict__ cbt0, const float* __restrict__ csq0, int S0,
                                                             const float* __restrict__ cb1, const float* __restrict__ cbt1,
                                                             const float* __restrict__ csq1, int S1, int* __restrict__ codes) {
    __shared__ __attribute__((aligned(16))) float As[CG_K][CG_T + 4];
    __shared__ __attribute__((aligned(16))) float Bs[CG_K][CG_T];
    __shared__ float rv[CG_T][17], part[CG_T][4], xsq[CG_T];
    __shared__ int ri[CG_T][17], best[CG_T];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4, chain = blockIdx.y;
    const long m0 = (long)blockIdx.x * CG_T;
    const int stages = chain ? Q - 1 : 1, S = chain ? S1 : S0, col = chain ? D : 0;
    for (int st = 0; st < stages; ++st) {
        const float* cb = (chain ? cb1 : cb0) + (size_t)st * S * D;
        const float* cbt = (chain ? cbt1 : cbt0) + (size_t)st * S * D;
        const float* csq = (chain ? csq1 : csq0) + (size_t)st * S;
        {   // |r|^2 per frame: four strided partials, then ((p0 + p1) + (p2 + p3))
            const int f = tid >> 2, pt = tid & 3;
            float p = 0.0f;
            if (m0 + f < M)
                for (int d = pt; d < D; d += 4) { const float v = r[(m0 + f) * ldr + col + d]; p = fmaf(v, v, p); }
            part[f][pt] = p;
            __syncthreads();
            if (tid < CG_T) xsq[tid] = (part[tid][0] + part[tid][1]) + (part[tid][2] + part[tid][3]);
        }
        float bv[4];
        int bi[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) { bv[i] = INFINITY; bi[i] = 0; }
        for (int n0 = 0; n0 < S; n0 += CG_T) {
            float acc[4][4];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[i][q] = 0.0f;
            for (int k0 = 0; k0 < D; k0 += CG_K) {
                __syncthreads();                                       // the previous step's tiles are consumed; xsq is written
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) {
                    const int idx = tid + rr * CG_THREADS, row = idx >> 4, kk = idx & 15, k = k0 + kk;
                    As[kk][row] = (m0 + row < M && k < D) ? r[(m0 + row) * ldr + col + k] : 0.0f;
                }
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) {
                    const int idx = tid + rr * CG_THREADS, kk = idx >> 6, c = idx & 63, k = k0 + kk, n = n0 + c;
                    Bs[kk][c] = (k < D && n < S) ? cbt[(size_t)k * S + n] : 0.0f;
                }
                __syncthreads();
#pragma unroll
                for (int kk = 0; kk < CG_K; ++kk) {
                    const float4 a = lds_read_f4(&As[kk][ty * 4]);
                    const float4 bq = lds_read_f4(&Bs[kk][tx * 4]);
                    const float av[4] = {a.x, a.y, a.z, a.w}, bw[4] = {bq.x, bq.y, bq.z, bq.w};
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int q = 0; q < 4; ++q) acc[i][q] = fmaf(av[i], bw[q], acc[i][q]);
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {                              // ascending n: a thread keeps the lowest index among equals
                const int n = n0 + tx * 4 + q;
                if (n >= S) continue;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float v = (xsq[ty * 4 + i] - 2.0f * acc[i][q]) + csq[n];
                    if (v < bv[i]) { bv[i] = v; bi[i] = n; }
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) { rv[ty * 4 + i][tx] = bv[i]; ri[ty * 4 + i][tx] = bi[i]; }
        __syncthreads();
        if (tid < CG_T) {                                              // (value, index) pairs: the smaller value, then the smaller index
            float v = rv[tid][0];
            int n = ri[tid][0];
            for (int t = 1; t < 16; ++t) {
                const float v2 = rv[tid][t];
                const int n2 = ri[tid][t];
                if (v2 < v || (v2 == v && n2 < n)) { v = v2; n = n2; }
            }
            best[tid] = n;
            if (m0 + tid < M) codes[(m0 + tid) * Q + chain + st] = n;
        }
        __syncthreads();
        for (int idx = tid; idx < CG_T * D; idx += CG_THREADS) {
            const int f = idx / D, d = idx - f * D;
            if (m0 + f < M) r[(m0 + f) * ldr + col + d] = r[(m0 + f) * ldr + col + d] - cb[(size_t)best[f] * D + d];
        }
        __threadfence_block();
        __syncthreads();
    }
}

// the kernel's launch entry (codec_launch.h): CodecEncQwen3TTS::dev_transformer and qasr_codec_case_probe call this
void cenc_attn_launch(const float* qkv, const int* tiles, int n_tiles, const float* rope, int heads, float* out, hipStream_t s) {
    hipLaunchKernelGGL(cenc_attn_kernel, dim3((unsigned)n_tiles, (unsigned)heads), dim3(ROW_THREADS), 0, s, qkv, reinterpret_cast<const int4*>(tiles),
                       reinterpret_cast<const float2*>(rope), heads, out);
}

// the kernel's launch entry (codec_launch.h): CodecEncQwen3TTS::dev_rvq and qasr_codec_case_probe call this
void cenc_vq_launch(float* r, long M, int ldr, int D, int Q, const float* cb0, const float* cbt0, const float* csq0, int S0, const float* cb1,
                    const float* cbt1, const float* csq1, int S1, int* codes, hipStream_t s) {
    hipLaunchKernelGGL(cenc_vq_kernel, dim3((unsigned)cdiv(M, CG_T), 2), dim3(CG_THREADS), 0, s, r, M, ldr, D, Q, cb0, cbt0, csq0, S0, cb1, cbt1,
                       csq1, S1, codes);
}

// ---- weights ------------------------------------------------------------------------------------------------------------------------
CodecEncQwen3TTS::CodecEncQwen3TTS(int device, const CheckedWeights& cw, const CodecGeom& g, const std::vector<bool>& embed_stored,
                                   long max_samples, hipStream_t work)
    : device_(device), g_(g), max_samples_(max_samples) {
    codec_check_geometry(g, "speech tokenizer encoder");
    if (max_samples < 1 || max_samples > CENC_MAX_SAMPLES) throw std::invalid_argument("speech tokenizer encoder: max_samples in 1..2^24");
    param_bytes_ = cw.disk_bytes;
    Builder b(cw);
    const int L = g.latent, H = g.hidden, Dd = g.decoder_dim, D = g.codebook_dim, A = g.heads * g.head_dim, I = 2 * H, Q = g.quantizers;
    codec_enc_strides(g, stride_);
    auto conv = [&](const std::string& key, int Cout, int Cin, int k, bool bias) { return codec_pack_conv(b, key, Cout, Cin, k, bias); };
    auto snake = [&](const std::string& key) { return codec_pack_snake(b, key); };
    // codebooks (TTSWeightLoading+Encoder.swift:121-139) as [S][D], transposed [D][S] for the score GEMM, and |c|^2 in f32
    for (int chain = 0; chain < 2; ++chain) {
        const int n = chain ? g.acoustic_size : g.semantic_size, stages = chain ? Q - 1 : 1;
        cb_[chain] = b.take((size_t)stages * n * D);
        cbt_[chain] = b.take((size_t)stages * n * D);
        csq_[chain] = b.take((size_t)stages * n);
        for (int st = 0; st < stages; ++st) {
            const int q = chain + st;
            codec_pack_codebook(b, cb_[chain] + (size_t)st * n * D, codec_codebook_prefix("encoder", q), embed_stored[q], n, D);
            const float* e = b.h.data() + cb_[chain] + (size_t)st * n * D;
            float* et = b.h.data() + cbt_[chain] + (size_t)st * n * D;
            float* sq = b.h.data() + csq_[chain] + (size_t)st * n;
            for (int i = 0; i < n; ++i) {
                float s = 0.0f;
                for (int d = 0; d < D; ++d) { const float v = e[(size_t)i * D + d]; et[(size_t)d * n + i] = v; s = s + v * v; }
                sq[i] = s;
            }
        }
    }
    {   // both input projections as one GEMM: columns [first | rest]
        rvq_.K = H; rvq_.N = 2 * D; rvq_.Cin = H; rvq_.taps = 1;
        rvq_.wt = b.take((size_t)H * 2 * D);
        const auto &w1 = b.t("encoder.quantizer.rvq_first.input_proj.weight"), &w2 = b.t("encoder.quantizer.rvq_rest.input_proj.weight");
        for (int c = 0; c < H; ++c)
            for (int d = 0; d < D; ++d) {
                b.h[rvq_.wt + (size_t)c * 2 * D + d] = w1[(size_t)c * D + d];
                b.h[rvq_.wt + (size_t)c * 2 * D + D + d] = w2[(size_t)c * D + d];
            }
    }
    int c = Dd / 16;
    in_w_ = codec_pack_taps7(b, "encoder.encoder.0.conv.weight", c);
    in_b_ = b.vec("encoder.encoder.0.conv.bias");
    width_[0] = c;
    for (int k = 0; k < 4; ++k) {
        const std::string p = "encoder.encoder." + std::to_string(k + 1) + ".block.";
        Block& bl = blocks_[k];
        for (int j = 0; j < 3; ++j) {
            const std::string u = p + std::to_string(j) + ".";
            bl.u[j].s1 = snake(u + "act1"); bl.u[j].s2 = snake(u + "act2");
            bl.u[j].c1 = conv(u + "conv1.conv", c, c, 7, true);
            bl.u[j].c2 = conv(u + "conv2.conv", c, c, 1, true);
        }
        bl.s = snake(p + "3");
        bl.sconv = conv(p + "4.conv", 2 * c, c, 2 * stride_[k], true);
        c *= 2;
        width_[k + 1] = c;
    }
    width_[4] = std::max(c, 4 * L); width_[5] = 4 * L; width_[6] = L;
    enc5_ = conv("encoder.encoder.5.conv", L, Dd, 7, true);
    for (int i = 0; i < 2; ++i) {
        const std::string p = "encoder.downsample." + std::to_string(i) + ".";
        Down& u = down_[i];
        u.dw = codec_pack_taps7(b, p + "0.dwconv.conv.weight", L);
        u.dwb = b.vec(p + "0.dwconv.conv.bias");
        u.lnw = b.vec(p + "0.norm.weight"); u.lnb = b.vec(p + "0.norm.bias");
        u.pw1 = conv(p + "0.pwconv1", 4 * L, L, 1, true);
        u.pw2 = conv(p + "0.pwconv2", L, 4 * L, 1, true);
        u.gamma = b.vec(p + "0.gamma");
        u.sconv = conv(p + "1.conv", L, L, 2 * stride_[4 + i], true);
    }
    post_conv_ = conv("encoder.post_conv.conv", L, L, 3, true);
    const std::string P = "encoder.pre_transformer.";
    in_proj_ = conv(P + "input_proj", H, L, 1, true);
    norm_ = b.vec(P + "norm.weight");
    for (int l = 0; l < g.layers; ++l)
        layers_.push_back(codec_pack_layer(b, P + "layers." + std::to_string(l) + ".", H, A));
    // rows a pass can hold at every level: a clip of n samples has ceil(n / rate) rows, so max_samples / rate + one per clip
    long rate = 1;
    size_t big = 0;
    for (int l = 0; l < CENC_LEVELS; ++l) {
        rows_cap_[l] = (max_samples + rate - 1) / rate + CENC_MAX_CLIPS;
        if (l == 0) rows_cap_[l] = max_samples;
        big = std::max(big, (size_t)rows_cap_[l] * width_[l]);
        if (l < 6) rate *= stride_[l];
    }
    const long max_frames = (max_samples + rate - 1) / rate;
    rope_ = codec_pack_rope(b, max_frames);            // positions 0 .. a clip's last frame
    QASR_HIP(hipSetDevice(device_));
    QASR_HIP(hipStreamCreateWithFlags(&own_, hipStreamNonBlocking));
    work_ = work ? work : own_;
    for (auto& e : ev_) QASR_HIP(hipEventCreate(&e));
    d_w_.alloc(b.h.size() * sizeof(float));
    QASR_HIP(hipMemcpy(d_w_.p, b.h.data(), b.h.size() * sizeof(float), hipMemcpyHostToDevice));
    // every buffer of a pass, sized once
    const size_t F = sizeof(float), R6 = (size_t)rows_cap_[6];
    d_start_.alloc((size_t)CENC_LEVELS * (CENC_MAX_CLIPS + 1) * sizeof(int));
    d_tiles_.alloc((R6 / AT_Q + CENC_MAX_CLIPS + 1) * 4 * sizeof(int));
    d_pcm_.alloc((size_t)max_samples * F);
    for (auto& buf : d_big_) buf.alloc(big * F);
    d_x_.alloc(R6 * H * F); d_h_.alloc(R6 * H * F); d_qkv_.alloc(R6 * 3 * A * F); d_att_.alloc(R6 * A * F); d_g_.alloc(R6 * I * F);
    d_r_.alloc(R6 * 2 * D * F); d_codes_.alloc(R6 * Q * sizeof(int));
}

CodecEncQwen3TTS::~CodecEncQwen3TTS() {
    if (work_) (void)hipStreamSynchronize(work_);
    for (auto& e : ev_) if (e) (void)hipEventDestroy(e);
    if (own_) (void)hipStreamDestroy(own_);
}

void CodecEncQwen3TTS::unload() {
    if (!loaded_) return;
    QASR_HIP(hipSetDevice(device_));
    QASR_HIP(hipStreamSynchronize(work_));
    for (DevBuf* b : {&d_w_, &d_start_, &d_tiles_, &d_pcm_, &d_big_[0], &d_big_[1], &d_big_[2], &d_x_, &d_h_, &d_qkv_, &d_att_, &d_g_, &d_r_,
                      &d_codes_})
        b->release();
    loaded_ = false;
}

void CodecEncQwen3TTS::check_loaded() const {
    if (!loaded_) throw NotLoaded("speech tokenizer encoder: model unloaded");
}

// ---- a pass -------------------------------------------------------------------------------------------------------------------------
// uploads the pass's tables and samples: start[level][clip], the attention's query tiles, pcm back to back
void CodecEncQwen3TTS::plan(const CodecEncClip* c, int n) {
    QASR_HIP(hipStreamSynchronize(work_));             // the tables are rewritten
    n_clips_ = n;
    h_start_.assign((size_t)CENC_LEVELS * (CENC_MAX_CLIPS + 1), 0);
    h_tiles_.clear();
    long at[CENC_LEVELS] = {};
    for (int i = 0; i < n; ++i) {
        long len[CENC_LEVELS];
        codec_enc_lengths(g_, c[i].n, len);
        for (int l = 0; l < CENC_LEVELS; ++l) h_start_[(size_t)l * (CENC_MAX_CLIPS + 1) + i] = (int)at[l];
        for (long q0 = 0; q0 < len[6]; q0 += AT_Q) {
            h_tiles_.push_back((int)at[6]); h_tiles_.push_back((int)len[6]); h_tiles_.push_back((int)q0); h_tiles_.push_back(0);
        }
        for (int l = 0; l < CENC_LEVELS; ++l) at[l] += len[l];
    }
    for (int l = 0; l < CENC_LEVELS; ++l) {
        h_start_[(size_t)l * (CENC_MAX_CLIPS + 1) + n] = (int)at[l];
        M_[l] = at[l];
        if (at[l] > rows_cap_[l]) throw std::length_error("speech tokenizer encoder: a pass exceeds its buffers");
    }
    n_tiles_ = (int)(h_tiles_.size() / 4);
    if (h_tiles_.size() * sizeof(int) > d_tiles_.bytes) throw std::length_error("speech tokenizer encoder: a pass exceeds its tile table");
    h_pcm_.resize((size_t)at[0]);
    long off = 0;
    for (int i = 0; i < n; ++i) { std::memcpy(h_pcm_.data() + off, c[i].pcm, (size_t)c[i].n * sizeof(float)); off += c[i].n; }
    QASR_HIP(hipMemcpy(d_start_.p, h_start_.data(), h_start_.size() * sizeof(int), hipMemcpyHostToDevice));
    QASR_HIP(hipMemcpy(d_tiles_.p, h_tiles_.data(), h_tiles_.size() * sizeof(int), hipMemcpyHostToDevice));
    QASR_HIP(hipMemcpy(d_pcm_.p, h_pcm_.data(), h_pcm_.size() * sizeof(float), hipMemcpyHostToDevice));
}

template <bool SNAKE, int EPI>
void CodecEncQwen3TTS::gemm(const Gemm& gm, const float* A, long M, int dil, int stride, int level, int in_level, const Snake* sn,
                            const float* ls, const float* R, float* C, int ldc) {
    CodecRowsArg rows;
    rows.kind = CODEC_ROWS_CLIP;
    rows.a = level < 0 ? nullptr : starts(level);
    rows.b = level < 0 ? nullptr : starts(in_level);
    rows.n_clips = n_clips_;
    rows.stride = stride;
    codec_tile_launch(rows, SNAKE, EPI, A, M, gm.Cin, gm.taps, dil, W(gm.wt), gm.K, gm.N, gm.has_bias ? W(gm.bias) : (const float*)nullptr, gm.N,
                      sn ? W(sn->a) : (const float*)nullptr, sn ? W(sn->b) : (const float*)nullptr, ls, R, C, ldc, work_);
}

// d_pcm_ -> conv_out_ [frames][latent]; records ev_[1] .. ev_[6]
void CodecEncQwen3TTS::dev_convs() {
    const int L = g_.latent;
    float *a = d_big_[0].as<float>(), *t = d_big_[1].as<float>(), *o = d_big_[2].as<float>();
    int C = width_[0];
    cenc_in_launch(d_pcm_.as<float>(), M_[0], C, starts(0), n_clips_, W(in_w_), W(in_b_), a, work_);
    QASR_HIP(hipEventRecord(ev_[1], work_));
    const int dil[3] = {1, 3, 9};
    for (int k = 0; k < 4; ++k) {                      // three residual units, SnakeBeta, strided conv (:63-70)
        const Block& bl = blocks_[k];
        for (int j = 0; j < 3; ++j) {
            gemm<true, E_LIN>(bl.u[j].c1, a, M_[k], dil[j], 1, k, k, &bl.u[j].s1, nullptr, nullptr, t, C);
            gemm<true, E_RES>(bl.u[j].c2, t, M_[k], 1, 1, k, k, &bl.u[j].s2, nullptr, a, a, C);
        }
        gemm<true, E_LIN>(bl.sconv, a, M_[k + 1], 1, stride_[k], k + 1, k, &bl.s, nullptr, nullptr, o, 2 * C);
        std::swap(a, o);
        C *= 2;
        QASR_HIP(hipEventRecord(ev_[2 + k], work_));
    }
    gemm<false, E_LIN>(enc5_, a, M_[4], 1, 1, 4, 4, nullptr, nullptr, nullptr, t, L);
    std::swap(a, t);
    for (int i = 0; i < 2; ++i) {                      // ConvNeXt, strided conv (:233-236)
        const Down& u = down_[i];
        const int lv = 4 + i;
        CodecRowsArg rows;
        rows.kind = CODEC_ROWS_CLIP;
        rows.a = rows.b = starts(lv);
        rows.n_clips = n_clips_;
        codec_dwln_launch(rows, a, M_[lv], L, W(u.dw), W(u.dwb), W(u.lnw), W(u.lnb), t, work_);
        gemm<false, E_GELU>(u.pw1, t, M_[lv], 1, 1, -1, -1, nullptr, nullptr, nullptr, o, 4 * L);
        gemm<false, E_LSRES>(u.pw2, o, M_[lv], 1, 1, -1, -1, nullptr, W(u.gamma), a, a, L);
        gemm<false, E_LIN>(u.sconv, a, M_[lv + 1], 1, stride_[lv], lv + 1, lv, nullptr, nullptr, nullptr, t, L);
        std::swap(a, t);
    }
    gemm<false, E_LIN>(post_conv_, a, M_[6], 1, 1, 6, 6, nullptr, nullptr, nullptr, t, L);
    conv_out_ = t;
    QASR_HIP(hipEventRecord(ev_[6], work_));
    QASR_HIP(hipGetLastError());
}

// conv_out_ -> d_h_ [frames][hidden]; records ev_[7]
void CodecEncQwen3TTS::dev_transformer() {
    const int H = g_.hidden, A = g_.heads * g_.head_dim;
    const long M = M_[6];
    float *x = d_x_.as<float>(), *h = d_h_.as<float>(), *qkv = d_qkv_.as<float>(), *att = d_att_.as<float>(), *gg = d_g_.as<float>();
    gemm<false, E_LIN>(in_proj_, conv_out_, M, 1, 1, -1, -1, nullptr, nullptr, nullptr, x, H);
    for (const CodecLayer& ly : layers_) {
        codec_rms_launch(x, M, H, W(ly.n1), g_.eps, h, work_);
        gemm<false, E_LIN>(ly.qkv, h, M, 1, 1, -1, -1, nullptr, nullptr, nullptr, qkv, 3 * A);
        cenc_attn_launch(qkv, d_tiles_.as<int>(), n_tiles_, W(rope_), g_.heads, att, work_);
        gemm<false, E_LSRES>(ly.o, att, M, 1, 1, -1, -1, nullptr, W(ly.ls1), x, x, H);
        codec_rms_launch(x, M, H, W(ly.n2), g_.eps, h, work_);
        gemm<false, E_SWIGLU>(ly.gu, h, M, 1, 1, -1, -1, nullptr, nullptr, nullptr, gg, 2 * H);
        gemm<false, E_LSRES>(ly.down, gg, M, 1, 1, -1, -1, nullptr, W(ly.ls2), x, x, H);
    }
    codec_rms_launch(x, M, H, W(norm_), g_.eps, h, work_);
    QASR_HIP(hipEventRecord(ev_[7], work_));
    QASR_HIP(hipGetLastError());
}

// d_h_ [F][hidden] -> d_codes_ [F][Q]; records ev_[8]
void CodecEncQwen3TTS::dev_rvq(long F) {
    const int D = g_.codebook_dim;
    gemm<false, E_LIN>(rvq_, d_h_.as<float>(), F, 1, 1, -1, -1, nullptr, nullptr, nullptr, d_r_.as<float>(), 2 * D);
    cenc_vq_launch(d_r_.as<float>(), F, 2 * D, D, g_.quantizers, W(cb_[0]), W(cbt_[0]), W(csq_[0]), g_.semantic_size, W(cb_[1]), W(cbt_[1]),
                   W(csq_[1]), g_.acoustic_size, d_codes_.as<int>(), work_);
    QASR_HIP(hipEventRecord(ev_[8], work_));
    QASR_HIP(hipGetLastError());
}

// d_codes_ rows row0 .. row0 + frames of F -> codes [Q][frames]
void CodecEncQwen3TTS::fetch_codes(long F, long row0, long frames, int32_t* codes) {
    const int Q = g_.quantizers;
    if (row0 == 0) {
        h_codes_.resize((size_t)F * Q);
        QASR_HIP(hipMemcpyAsync(h_codes_.data(), d_codes_.p, h_codes_.size() * sizeof(int32_t), hipMemcpyDeviceToHost, work_));
        QASR_HIP(hipStreamSynchronize(work_));
    }
    for (long t = 0; t < frames; ++t)
        for (int q = 0; q < Q; ++q) codes[(size_t)q * frames + t] = h_codes_[(size_t)(row0 + t) * Q + q];
}

void CodecEncQwen3TTS::pass(const CodecEncClip* c, int n, Mode mode) {
    QASR_HIP(hipSetDevice(device_));
    plan(c, n);
    const size_t F = sizeof(float);
    QASR_HIP(hipEventRecord(ev_[0], work_));
    dev_convs();
    int last = 6;
    if (mode != CONV) { dev_transformer(); last = 7; }
    if (mode == ENCODE) { dev_rvq(M_[6]); last = 8; }
    const int* fs = h_start_.data() + (size_t)6 * (CENC_MAX_CLIPS + 1);
    if (mode == ENCODE) {
        for (int i = 0; i < n; ++i) fetch_codes(M_[6], fs[i], fs[i + 1] - fs[i], c[i].codes);
    } else {
        const int width = mode == CONV ? g_.latent : g_.hidden;
        const float* src = mode == CONV ? conv_out_ : d_h_.as<float>();
        for (int i = 0; i < n; ++i)
            QASR_HIP(hipMemcpyAsync(c[i].out, src + (size_t)fs[i] * width, (size_t)(fs[i + 1] - fs[i]) * width * F, hipMemcpyDeviceToHost, work_));
        QASR_HIP(hipStreamSynchronize(work_));
    }
    QASR_HIP(hipGetLastError());
    for (int s = 0; s < last; ++s) {
        float ms = 0;
        QASR_HIP(hipEventElapsedTime(&ms, ev_[s], ev_[s + 1]));
        timing_[s] += ms;
    }
}

// ---- entry points -------------------------------------------------------------------------------------------------------------------
void CodecEncQwen3TTS::run(const std::vector<CodecEncClip>& clips, Mode mode) {
    check_loaded();
    for (float& t : timing_) t = 0.0f;
    for (size_t i = 0; i < clips.size(); ++i)
        if (clips[i].n < 1 || clips[i].n > max_samples_)
            throw std::invalid_argument("speech tokenizer encoder: item " + std::to_string(i) + " holds " + std::to_string(clips[i].n) +
                                        " samples, a clip holds 1.." + std::to_string(max_samples_) + " (max_samples; the encoder is not chunked)");
    for (size_t i = 0; i < clips.size();) {            // passes end at clip boundaries
        size_t j = i;
        long total = 0;
        while (j < clips.size() && j - i < (size_t)CENC_MAX_CLIPS && total + clips[j].n <= max_samples_) total += clips[j++].n;
        pass(clips.data() + i, (int)(j - i), mode);
        i = j;
    }
}

void CodecEncQwen3TTS::quantize(const float* h, long F, int32_t* codes) {
    check_loaded();
    for (float& t : timing_) t = 0.0f;
    QASR_HIP(hipSetDevice(device_));
    const int H = g_.hidden, Q = g_.quantizers;
    std::vector<int32_t> part;
    for (long f0 = 0; f0 < F; f0 += rows_cap_[6]) {    // frames are independent: any split gives the same codes
        const long n = std::min(F - f0, rows_cap_[6]);
        QASR_HIP(hipStreamSynchronize(work_));
        QASR_HIP(hipMemcpyAsync(d_h_.p, h + (size_t)f0 * H, (size_t)n * H * sizeof(float), hipMemcpyHostToDevice, work_));
        QASR_HIP(hipEventRecord(ev_[7], work_));
        dev_rvq(n);
        part.resize((size_t)n * Q);
        fetch_codes(n, 0, n, part.data());
        for (int q = 0; q < Q; ++q) std::memcpy(codes + (size_t)q * F + f0, part.data() + (size_t)q * n, (size_t)n * sizeof(int32_t));
        float ms = 0;
        QASR_HIP(hipEventElapsedTime(&ms, ev_[7], ev_[8]));
        timing_[7] += ms;
    }
}

}  // namespace qasr
