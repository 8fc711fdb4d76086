// codec_qwen3tts.hip -- the Qwen3-TTS speech tokenizer decoder for gfx950 (codec_qwen3tts.h).  f32 throughout, accurate sinf / expf /
// erff / sqrtf, no atomics, no vendor BLAS.
//
// A pass runs W windows (of any utterances, 1..35 frames each).  Activations are [window rows back to back][C]; a window of F frames
// whose first frame is row `off` of the 1x tensors owns rows off * r .. (off + F) * r of the tensors at rate r (2, 4, 32, 160, 640,
// 1920), so one table fstart[frame row] = off serves every rate; row indices are 64-bit.
// Launches of a pass:
//   codec_gather_kernel    per frame: codebook 0's vector | the 15 acoustic vectors summed in codebook order -> [M][2 D]
//   codec_gemm_kernel      (codec_shared.h, with the row locator WindowRows) the 64 x 64 tiled f32 GEMM of sep_gemm_kernel as an
//                          implicit-GEMM causal conv: K = taps x C_in, the A element of (row t, tap j, channel c) is
//                          x[t - (taps - 1 - j) dilation][c], zero before the window's first row, SnakeBeta
//                          optionally applied as it is loaded; the epilogue is bias | bias + GELU | bias + residual | layer scale +
//                          residual | SiLU(gate) x up over interleaved columns.  It runs the two RVQ projections (one GEMM, K = 2 D),
//                          pre_conv, every Linear, decoder.decoder.0, the k = 7 and k = 1 convs of the residual units, and every
//                          transposed conv: with k = 2 s, output row t s + j is x[t] W[:, :, j] + x[t - 1] W[:, :, j + s], a two-tap GEMM
//                          with N = s C_out whose output row [s][C_out] IS rows t s .. t s + s - 1 of the upsampled tensor; the trim
//                          falls out.  Edge tiles are guarded, not padded.
//   codec_rms_kernel       (codec_shared.h) RMSNorm, one workgroup per row
//   codec_attn_kernel      one workgroup per (window, head): q, k (RoPE on the way in, rotate-halves, positions from 0) and v in LDS,
//                          causal scores, softmax, P V
//   codec_dwln_kernel      (codec_shared.h, WindowRows) depthwise k = 7 causal conv + LayerNorm, one workgroup per row
//   codec_out_kernel       final SnakeBeta, the C -> 1 k = 7 conv as one dot of 7 C terms per sample, clip
// Summation order: every GEMM output is one thread's fmaf chain over k = 0..K-1 (taps outer, channels inner;
// rows before the window add exact zeros); the row reductions of the norms are a thread's sequential partial over c = tid, tid + 256, ..
// then a fixed tree; attention sums over d, then over j, in order.  No reduction crosses a window and nothing depends on a window's
// place, so a window's samples are the same bits alone, in any batch, at any place in it and under any split into passes.
#include "codec_qwen3tts.h"
#include "tuning.h"
#include <algorithm>
#include <cmath>
#include <cstring>

namespace qasr {

// ---- geometry, keys, windows (host) -------------------------------------------------------------------------------------------------
CodecShapes codec_tensor_shapes(const CodecGeom& g, const std::vector<bool>& embed_stored) {
    CodecShapes s;
    auto add = [&](const std::string& k, std::vector<int64_t> sh) { s.emplace_back(k, std::move(sh)); };
    const int64_t L = g.latent, H = g.hidden, Dd = g.decoder_dim, D = g.codebook_dim;
    for (int q = 0; q < g.quantizers; ++q) {
        const int64_t n = q == 0 ? g.semantic_size : g.acoustic_size;
        const std::string p = codec_codebook_prefix("decoder", q);
        if (embed_stored[q]) add(p + ".embed", {n, D});
        else { add(p + ".embedding_sum", {n, D}); add(p + ".cluster_usage", {n}); }
    }
    add("decoder.quantizer.rvq_first.output_proj.weight", {H, D, 1});
    add("decoder.quantizer.rvq_rest.output_proj.weight", {H, D, 1});
    add("decoder.pre_conv.conv.weight", {L, H, 3}); add("decoder.pre_conv.conv.bias", {L});
    codec_pre_transformer_shapes(s, "decoder.pre_transformer.", g);
    for (int i = 0; i < 2; ++i) {
        const std::string p = "decoder.upsample." + std::to_string(i) + ".";
        add(p + "0.conv.weight", {L, L, 2 * g.ratios[i]}); add(p + "0.conv.bias", {L});
        add(p + "1.dwconv.conv.weight", {L, 1, 7}); add(p + "1.dwconv.conv.bias", {L});
        add(p + "1.norm.weight", {L}); add(p + "1.norm.bias", {L});
        add(p + "1.pwconv1.weight", {4 * L, L}); add(p + "1.pwconv1.bias", {4 * L});
        add(p + "1.pwconv2.weight", {L, 4 * L}); add(p + "1.pwconv2.bias", {L});
        add(p + "1.gamma", {L});
    }
    add("decoder.decoder.0.conv.weight", {Dd, L, 7}); add("decoder.decoder.0.conv.bias", {Dd});
    int64_t c = Dd;
    for (int b = 0; b < 4; ++b) {
        const std::string p = "decoder.decoder." + std::to_string(b + 1) + ".block.";
        const int64_t co = c / 2;
        add(p + "0.alpha", {c}); add(p + "0.beta", {c});
        add(p + "1.conv.weight", {c, co, 2 * g.rates[b]}); add(p + "1.conv.bias", {co});
        for (int j = 2; j <= 4; ++j) {
            const std::string u = p + std::to_string(j) + ".";
            for (const char* a : {"act1", "act2"}) { add(u + a + ".alpha", {co}); add(u + a + ".beta", {co}); }
            add(u + "conv1.conv.weight", {co, co, 7}); add(u + "conv1.conv.bias", {co});
            add(u + "conv2.conv.weight", {co, co, 1}); add(u + "conv2.conv.bias", {co});
        }
        c = co;
    }
    add("decoder.decoder.5.alpha", {c}); add("decoder.decoder.5.beta", {c});
    add("decoder.decoder.6.conv.weight", {1, c, 7}); add("decoder.decoder.6.conv.bias", {1});
    return s;
}

std::vector<CodecSpan> codec_window_positions(long T) {
    std::vector<CodecSpan> out;
    if (T <= CODEC_CHUNK + CODEC_CONTEXT) { out.push_back({0, 0, (int)T}); return out; }
    for (long offset = 0; offset < T;) {
        const long end = std::min(offset + CODEC_CHUNK, T), start = std::max(offset - CODEC_CONTEXT, 0L);
        out.push_back({(int)start, (int)(offset - start), (int)end});
        offset = end;
    }
    return out;
}

constexpr int UNIT_DIL[3] = {1, 3, 9};                 // the residual units of a block, k = 7 each

void codec_tail_leads(const int rates[4], int leads[6]) {
    const int units = 6 * (UNIT_DIL[0] + UNIT_DIL[1] + UNIT_DIL[2]);
    leads[5] = 6;
    for (int k = 3; k >= 0; --k) leads[k + 1] = cdiv(leads[k + 2] + units, rates[k]) + 1;
    leads[0] = leads[1] + 6;
}

// ---- kernels ------------------------------------------------------------------------------------------------------------------------
// codes [M][Q]; cb: codebook 0 [S0][D], then Q - 1 codebooks [S1][D]; out [M][2 D] = first | rest summed in codebook order (:449-462)
__global__ __launch_bounds__(ROW_THREADS) void codec_gather_kernel(const int* __restrict__ codes, int Q, int D, long S0, long S1,
                                                                   const float* __restrict__ cb, float* __restrict__ out) {
    const long m = blockIdx.x;
    const int* c = codes + m * Q;
    for (int d = threadIdx.x; d < D; d += ROW_THREADS) {
        out[m * 2 * D + d] = cb[(long)c[0] * D + d];
        float acc = 0.0f;
        for (int q = 1; q < Q; ++q) {
            const float e = cb[(S0 + (long)(q - 1) * S1 + c[q]) * D + d];
            acc = q == 1 ? e : acc + e;
        }
        out[m * 2 * D + D + d] = acc;
    }
}

// qkv [M][3 A] (A = heads x 64), win[w] = (frames, first row), rope [35][32] (cos, sin); out [M][A].  grid (windows, heads).
__global__ __launch_bounds__(ROW_THREADS) void codec_attn_kernel(const float* __restrict__ qkv, const int2* __restrict__ win,
                                                                 const float2* __restrict__ rope, int heads, float* __restrict__ out) {
    __shared__ float sq[CODEC_MAX_T][64], sk[CODEC_MAX_T][65], sv[CODEC_MAX_T][64], sp[CODEC_MAX_T][CODEC_MAX_T + 1];
    const int tid = threadIdx.x, h = blockIdx.y, A = heads * 64;
    const int T = min(win[blockIdx.x].x, CODEC_MAX_T);
    const long off = win[blockIdx.x].y;
    for (int i = tid; i < T * 32; i += ROW_THREADS) {                  // MLXNN.RoPE traditional: false: element d pairs with d + 32
        const int t = i >> 5, d = i & 31;
        const float* base = qkv + (off + t) * 3 * A + h * 64;
        const float2 cs = rope[t * 32 + d];
        const float q1 = base[d], q2 = base[d + 32], k1 = base[A + d], k2 = base[A + d + 32];
        sq[t][d] = q1 * cs.x - q2 * cs.y; sq[t][d + 32] = q1 * cs.y + q2 * cs.x;
        sk[t][d] = k1 * cs.x - k2 * cs.y; sk[t][d + 32] = k1 * cs.y + k2 * cs.x;
    }
    for (int i = tid; i < T * 64; i += ROW_THREADS) sv[i >> 6][i & 63] = qkv[(off + (i >> 6)) * 3 * A + 2 * A + h * 64 + (i & 63)];
    __syncthreads();
    for (int p = tid; p < T * T; p += ROW_THREADS) {                   // the additive -1e9 mask leaves exact zeros after the softmax
        const int i = p / T, j = p - i * T;
        if (j > i) continue;
        float acc = 0.0f;
#pragma unroll 8
        for (int d = 0; d < 64; ++d) acc = fmaf(sq[i][d], sk[j][d], acc);
        sp[i][j] = acc * 0.125f;
    }
    __syncthreads();
    if (tid < T) {
        const int i = tid;
        float mx = sp[i][0];
        for (int j = 1; j <= i; ++j) mx = fmaxf(mx, sp[i][j]);
        float sum = 0.0f;
        for (int j = 0; j <= i; ++j) { const float e = expf(sp[i][j] - mx); sp[i][j] = e; sum = sum + e; }
        for (int j = 0; j <= i; ++j) sp[i][j] = sp[i][j] / sum;
    }
    __syncthreads();
    for (int p = tid; p < T * 64; p += ROW_THREADS) {
        const int i = p >> 6, d = p & 63;
        float acc = 0.0f;
        for (int j = 0; j <= i; ++j) acc = fmaf(sp[i][j], sv[j][d], acc);
        out[(off + i) * A + h * 64 + d] = acc;
    }
}

// wave[m] = clip(bias + sum_j sum_c snake(x[m - (6 - j)][c]) w[j][c]) (:683-685); x [M][C], one thread per sample.  TAIL: only the samples
// from the window's first kept frame (kept[frame row]) on are computed.
template <bool TAIL>
__global__ __launch_bounds__(ROW_THREADS) void codec_out_kernel(const float* __restrict__ x, long M, int C, int rate, const int* __restrict__ fstart,
                                                                const int* __restrict__ kept, const float* __restrict__ sa,
                                                                const float* __restrict__ sb, const float* __restrict__ w,
                                                                const float* __restrict__ b, int clip, float* __restrict__ wave) {
    const long m = (long)blockIdx.x * ROW_THREADS + threadIdx.x;
    if (m >= M) return;
    if (TAIL && m < (long)kept[m / rate] * rate) return;
    const long start = (long)fstart[m / rate] * rate;
    float acc = 0.0f;
    for (int j = 0; j < 7; ++j) {
        const long src = m - (6 - j);
        if (src < start) continue;
        for (int c = 0; c < C; ++c) acc = fmaf(codec_snake(x[src * C + c], sa[c], sb[c]), w[j * C + c], acc);
    }
    acc = acc + b[0];
    if (clip) acc = fminf(fmaxf(acc, -1.0f), 1.0f);
    wave[m] = acc;
}

// the launch entries of the kernels above (codec_launch.h): CodecQwen3TTS and qasr_codec_case_probe call these
void codec_attn_launch(const float* qkv, const int* win, int n_win, const float* rope, int heads, float* out, hipStream_t s) {
    hipLaunchKernelGGL(codec_attn_kernel, dim3((unsigned)n_win, (unsigned)heads), dim3(ROW_THREADS), 0, s, qkv, reinterpret_cast<const int2*>(win),
                       reinterpret_cast<const float2*>(rope), heads, out);
}

void codec_gather_launch(const int* codes, long M, int Q, int D, long S0, long S1, const float* cb, float* out, hipStream_t s) {
    hipLaunchKernelGGL(codec_gather_kernel, dim3((unsigned)M), dim3(ROW_THREADS), 0, s, codes, Q, D, S0, S1, cb, out);
}

void codec_out_launch(bool tail, const float* x, long M, int C, int rate, const int* fstart, const int* kept, const float* sa, const float* sb,
                      const float* w, const float* b, int clip, float* wave, hipStream_t s) {
    const dim3 grid((unsigned)cdiv(M, ROW_THREADS));
    if (tail) hipLaunchKernelGGL(codec_out_kernel<true>, grid, dim3(ROW_THREADS), 0, s, x, M, C, rate, fstart, kept, sa, sb, w, b, clip, wave);
    else hipLaunchKernelGGL(codec_out_kernel<false>, grid, dim3(ROW_THREADS), 0, s, x, M, C, rate, fstart, kept, sa, sb, w, b, clip, wave);
}

// ---- weights ------------------------------------------------------------------------------------------------------------------------
CodecQwen3TTS::CodecQwen3TTS(int device, const CheckedWeights& cw, const CodecGeom& g, const std::vector<bool>& embed_stored,
                             int max_windows, hipStream_t work)
    : device_(device), g_(g), max_windows_(max_windows), spf_(g.samples_per_frame()) {
    codec_check_geometry(g, "speech tokenizer decoder");
    if (max_windows < 1 || max_windows > 512) throw std::invalid_argument("speech tokenizer decoder: max_windows in 1..512");
    param_bytes_ = cw.disk_bytes;
    Builder b(cw);
    const int L = g.latent, H = g.hidden, Dd = g.decoder_dim, D = g.codebook_dim, A = g.heads * g.head_dim;
    auto conv = [&](const std::string& key, int Cout, int Cin, int k, bool bias) { return codec_pack_conv(b, key, Cout, Cin, k, bias); };
    auto snake = [&](const std::string& key) { return codec_pack_snake(b, key); };
    // transposed conv [in][out][2 s] as two taps: tap 0 (x[t - 1]) holds W[:, :, ph + s], tap 1 (x[t]) holds W[:, :, ph]; n = ph C_out + co
    auto tconv = [&](const std::string& key, int Cin, int Cout, int s) {
        Gemm gm; gm.K = 2 * Cin; gm.N = s * Cout; gm.Cin = Cin; gm.taps = 2;
        const auto& W = b.t(key + ".weight");
        gm.wt = b.take((size_t)gm.K * gm.N);
        for (int c = 0; c < Cin; ++c)
            for (int co = 0; co < Cout; ++co)
                for (int ph = 0; ph < s; ++ph) {
                    const size_t src = ((size_t)c * Cout + co) * 2 * s;
                    b.h[gm.wt + (size_t)c * gm.N + ph * Cout + co] = W[src + ph + s];
                    b.h[gm.wt + ((size_t)Cin + c) * gm.N + ph * Cout + co] = W[src + ph];
                }
        gm.has_bias = true;
        gm.bias = b.vec(key + ".bias");
        return gm;
    };
    // codebooks (TTSWeightLoading.swift:280-301)
    for (int q = 0; q < g.quantizers; ++q) {
        const int n = q == 0 ? g.semantic_size : g.acoustic_size;
        // codec_gather_kernel indexes all codebooks from cb_first_ as one array: take() pads to 4 floats, and codec_check_geometry
        // requires size x dim to be a multiple of 4, so consecutive takes are contiguous
        const size_t at = b.take((size_t)n * D);
        if (q == 0) cb_first_ = at;
        codec_pack_codebook(b, at, codec_codebook_prefix("decoder", q), embed_stored[q], n, D);
    }
    {   // both output projections as one GEMM over [first | rest]
        rvq_.K = 2 * D; rvq_.N = H; rvq_.Cin = 2 * D; rvq_.taps = 1;
        rvq_.wt = b.take((size_t)2 * D * H);
        const auto &w1 = b.t("decoder.quantizer.rvq_first.output_proj.weight"), &w2 = b.t("decoder.quantizer.rvq_rest.output_proj.weight");
        for (int n = 0; n < H; ++n)
            for (int c = 0; c < D; ++c) {
                b.h[rvq_.wt + (size_t)c * H + n] = w1[(size_t)n * D + c];
                b.h[rvq_.wt + ((size_t)D + c) * H + n] = w2[(size_t)n * D + c];
            }
    }
    pre_conv_ = conv("decoder.pre_conv.conv", L, H, 3, true);
    const std::string P = "decoder.pre_transformer.";
    in_proj_ = conv(P + "input_proj", H, L, 1, true);
    out_proj_ = conv(P + "output_proj", L, H, 1, true);
    norm_ = b.vec(P + "norm.weight");
    for (int l = 0; l < g.layers; ++l)
        layers_.push_back(codec_pack_layer(b, P + "layers." + std::to_string(l) + ".", H, A));
    for (int i = 0; i < 2; ++i) {
        const std::string p = "decoder.upsample." + std::to_string(i) + ".";
        Up& u = up_[i];
        u.tconv = tconv(p + "0.conv", L, L, g.ratios[i]);
        u.dw = codec_pack_taps7(b, p + "1.dwconv.conv.weight", L);
        u.dwb = b.vec(p + "1.dwconv.conv.bias");
        u.lnw = b.vec(p + "1.norm.weight"); u.lnb = b.vec(p + "1.norm.bias");
        u.pw1 = conv(p + "1.pwconv1", 4 * L, L, 1, true);
        u.pw2 = conv(p + "1.pwconv2", L, 4 * L, 1, true);
        u.gamma = b.vec(p + "1.gamma");
    }
    dec0_ = conv("decoder.decoder.0.conv", Dd, L, 7, true);
    size_t big = std::max((size_t)g.ratios[0] * g.ratios[1] * 4 * L, (size_t)g.ratios[0] * g.ratios[1] * Dd);
    int c = Dd, rate = g.ratios[0] * g.ratios[1];
    for (int k = 0; k < 4; ++k) {
        const std::string p = "decoder.decoder." + std::to_string(k + 1) + ".block.";
        const int co = c / 2;
        Block& bl = blocks_[k];
        bl.s = snake(p + "0");
        bl.tconv = tconv(p + "1.conv", c, co, g.rates[k]);
        for (int j = 0; j < 3; ++j) {
            const std::string u = p + std::to_string(j + 2) + ".";
            bl.u[j].s1 = snake(u + "act1"); bl.u[j].s2 = snake(u + "act2");
            bl.u[j].c1 = conv(u + "conv1.conv", co, co, 7, true);
            bl.u[j].c2 = conv(u + "conv2.conv", co, co, 1, true);
        }
        c = co; rate *= g.rates[k];
        big = std::max(big, (size_t)rate * c);
    }
    big_per_frame_ = big;
    final_snake_ = snake("decoder.decoder.5");
    final_w_ = codec_pack_taps7(b, "decoder.decoder.6.conv.weight", c);
    final_b_ = b.vec("decoder.decoder.6.conv.bias");
    rope_ = codec_pack_rope(b, CODEC_MAX_T);           // positions 0..34
    QASR_HIP(hipSetDevice(device_));
    QASR_HIP(hipStreamCreateWithFlags(&own_, hipStreamNonBlocking));
    work_ = work ? work : own_;
    for (auto& e : ev_) QASR_HIP(hipEventCreate(&e));
    d_w_.alloc(b.h.size() * sizeof(float));
    QASR_HIP(hipMemcpy(d_w_.p, b.h.data(), b.h.size() * sizeof(float), hipMemcpyHostToDevice));
}

CodecQwen3TTS::~CodecQwen3TTS() {
    if (work_) (void)hipStreamSynchronize(work_);
    for (auto& e : ev_) if (e) (void)hipEventDestroy(e);
    if (own_) (void)hipStreamDestroy(own_);
}

void CodecQwen3TTS::unload() {
    if (!loaded_) return;
    QASR_HIP(hipSetDevice(device_));
    QASR_HIP(hipStreamSynchronize(work_));
    for (DevBuf* b : {&d_w_, &d_codes_, &d_fstart_, &d_win_, &d_emb_, &d_q_, &d_lat_[0], &d_lat_[1], &d_x_, &d_h_, &d_qkv_, &d_att_, &d_g_,
                      &d_big_[0], &d_big_[1], &d_big_[2], &d_wave_, &d_kept_})
        b->release();
    cap_small_ = cap_big_ = cap_win_ = 0;
    loaded_ = false;
}

void CodecQwen3TTS::check_loaded() const {
    if (!loaded_) throw NotLoaded("speech tokenizer decoder: model unloaded");
}

// ---- a pass -------------------------------------------------------------------------------------------------------------------------
void CodecQwen3TTS::ensure(long M1, Mode mode) {
    const size_t F = sizeof(float), A = (size_t)g_.heads * g_.head_dim;
    // a capacity is recorded only once every buffer behind it exists: a failed allocation leaves it 0, so the next call allocates again
    if (M1 > cap_small_) {
        QASR_HIP(hipStreamSynchronize(work_));
        cap_small_ = 0;
        d_codes_.alloc(M1 * g_.quantizers * sizeof(int));
        d_fstart_.alloc(M1 * sizeof(int));
        d_kept_.alloc(M1 * sizeof(int));
        d_emb_.alloc(M1 * 2 * g_.codebook_dim * F);
        d_q_.alloc(M1 * g_.hidden * F);
        d_lat_[0].alloc(M1 * g_.latent * F); d_lat_[1].alloc(M1 * g_.latent * F);
        d_x_.alloc(M1 * g_.hidden * F); d_h_.alloc(M1 * g_.hidden * F);
        d_qkv_.alloc(M1 * 3 * A * F); d_att_.alloc(M1 * A * F); d_g_.alloc(M1 * 2 * g_.hidden * F);
        cap_small_ = M1;
    }
    if (mode == FULL && M1 > cap_big_) {
        QASR_HIP(hipStreamSynchronize(work_));
        cap_big_ = 0;
        for (auto& b : d_big_) b.alloc((size_t)M1 * big_per_frame_ * F);
        d_wave_.alloc((size_t)M1 * spf_ * F);
        cap_big_ = M1;
    }
}

// uploads the pass's tables: fstart[frame row] = its window's first row, kept[frame row] = its window's first kept row,
// win[w] = (frames, first row), codes [M1][Q]
void CodecQwen3TTS::plan(const CodecWin* w, int n, bool with_codes) {
    QASR_HIP(hipStreamSynchronize(work_));             // the tables are rewritten
    long M1 = 0;
    for (int i = 0; i < n; ++i) M1 += w[i].frames;
    M1_ = M1; n_win_ = n;
    std::vector<int> fstart((size_t)M1), kept((size_t)M1), win((size_t)2 * n);
    const int Q = g_.quantizers;
    if (with_codes) h_codes_.resize((size_t)M1 * Q);
    long off = 0;
    for (int i = 0; i < n; ++i) {
        win[2 * i] = w[i].frames; win[2 * i + 1] = (int)off;
        for (int t = 0; t < w[i].frames; ++t) {
            fstart[off + t] = (int)off;
            kept[off + t] = (int)off + w[i].context;
            if (with_codes)
                for (int q = 0; q < Q; ++q) h_codes_[(size_t)(off + t) * Q + q] = w[i].codes[(size_t)q * w[i].ld + w[i].start + t];
        }
        off += w[i].frames;
    }
    if (n > cap_win_) { cap_win_ = 0; d_win_.alloc((size_t)2 * n * sizeof(int)); cap_win_ = n; }
    QASR_HIP(hipMemcpy(d_win_.p, win.data(), win.size() * sizeof(int), hipMemcpyHostToDevice));
    QASR_HIP(hipMemcpy(d_fstart_.p, fstart.data(), fstart.size() * sizeof(int), hipMemcpyHostToDevice));
    QASR_HIP(hipMemcpy(d_kept_.p, kept.data(), kept.size() * sizeof(int), hipMemcpyHostToDevice));
    if (with_codes) QASR_HIP(hipMemcpy(d_codes_.p, h_codes_.data(), h_codes_.size() * sizeof(int), hipMemcpyHostToDevice));
}

template <bool SNAKE, int EPI>
void CodecQwen3TTS::gemm(const Gemm& gm, const float* A, long M, int dil, int rate, const Snake* sn, const float* ls, const float* R, float* C,
                         int ldc, int bmod, int lead) {
    CodecRowsArg rows;
    rows.a = d_fstart_.as<int>();
    rows.rate = rate;
    if constexpr (EPI == E_LIN || (SNAKE && EPI == E_RES)) {           // the vocoder's launches from decoder.decoder.0 on
        if (lead >= 0) {
            rows.kind = CODEC_ROWS_TAIL;
            rows.b = d_kept_.as<int>();
            rows.lead = lead;
        }
    }
    codec_tile_launch(rows, SNAKE, EPI, A, M, gm.Cin, gm.taps, dil, W(gm.wt), gm.K, gm.N, gm.has_bias ? W(gm.bias) : (const float*)nullptr, bmod,
                      sn ? W(sn->a) : (const float*)nullptr, sn ? W(sn->b) : (const float*)nullptr, ls, R, C, ldc, work_);
}

void CodecQwen3TTS::dev_rvq() {
    codec_gather_launch(d_codes_.as<int>(), M1_, g_.quantizers, g_.codebook_dim, (long)g_.semantic_size, (long)g_.acoustic_size, W(cb_first_),
                        d_emb_.as<float>(), work_);
    gemm<false, E_LIN>(rvq_, d_emb_.as<float>(), M1_, 1, 1, nullptr, nullptr, nullptr, d_q_.as<float>(), g_.hidden, g_.hidden);
    QASR_HIP(hipGetLastError());
}

// d_lat_[0] -> d_lat_[1]
void CodecQwen3TTS::dev_pre_transformer() {
    const int H = g_.hidden, L = g_.latent, A = g_.heads * g_.head_dim;
    const long M = M1_;
    float *x = d_x_.as<float>(), *h = d_h_.as<float>(), *qkv = d_qkv_.as<float>(), *att = d_att_.as<float>(), *gg = d_g_.as<float>();
    gemm<false, E_LIN>(in_proj_, d_lat_[0].as<float>(), M, 1, 1, nullptr, nullptr, nullptr, x, H, H);
    for (const CodecLayer& ly : layers_) {
        codec_rms_launch(x, M, H, W(ly.n1), g_.eps, h, work_);
        gemm<false, E_LIN>(ly.qkv, h, M, 1, 1, nullptr, nullptr, nullptr, qkv, 3 * A, 3 * A);
        codec_attn_launch(qkv, d_win_.as<int>(), n_win_, W(rope_), g_.heads, att, work_);
        gemm<false, E_LSRES>(ly.o, att, M, 1, 1, nullptr, W(ly.ls1), x, x, H, H);
        codec_rms_launch(x, M, H, W(ly.n2), g_.eps, h, work_);
        gemm<false, E_SWIGLU>(ly.gu, h, M, 1, 1, nullptr, nullptr, nullptr, gg, 2 * H, 2 * H);
        gemm<false, E_LSRES>(ly.down, gg, M, 1, 1, nullptr, W(ly.ls2), x, x, H, H);
    }
    codec_rms_launch(x, M, H, W(norm_), g_.eps, h, work_);
    gemm<false, E_LIN>(out_proj_, h, M, 1, 1, nullptr, nullptr, nullptr, d_lat_[1].as<float>(), L, L);
    QASR_HIP(hipGetLastError());
}

// d_lat_[1] -> d_wave_; records ev_[2] .. ev_[8].  tail: every launch from decoder.decoder.0 on starts each window at the first row a
// kept sample depends on (codec_tail_leads; inside a block, from its output backwards: unit j adds 6 x its dilation to the lead of the
// launches before it, and a transposed conv's row covers `stride` output rows).  The two upsampling stages run whole windows.
void CodecQwen3TTS::dev_vocoder(bool clip, bool tail) {
    const int L = g_.latent;
    int leads[6];
    codec_tail_leads(g_.rates, leads);
    float* buf[3] = {d_big_[0].as<float>(), d_big_[1].as<float>(), d_big_[2].as<float>()};
    const float* x = d_lat_[1].as<float>();
    int rate = 1;
    for (int i = 0; i < 2; ++i) {                      // transposed conv, ConvNeXt (:669-672)
        const Up& u = up_[i];
        float *y = buf[i == 0 ? 0 : 1], *h = buf[i == 0 ? 1 : 0], *mid = buf[2];
        gemm<false, E_LIN>(u.tconv, x, M1_ * rate, 1, rate, nullptr, nullptr, nullptr, y, u.tconv.N, L);
        rate *= g_.ratios[i];
        const long M = M1_ * rate;
        CodecRowsArg rows;
        rows.a = d_fstart_.as<int>();
        rows.rate = rate;
        codec_dwln_launch(rows, y, M, L, W(u.dw), W(u.dwb), W(u.lnw), W(u.lnb), h, work_);
        gemm<false, E_GELU>(u.pw1, h, M, 1, rate, nullptr, nullptr, nullptr, mid, 4 * L, 4 * L);
        gemm<false, E_LSRES>(u.pw2, mid, M, 1, rate, nullptr, W(u.gamma), y, y, L, L);
        x = y;
    }
    QASR_HIP(hipEventRecord(ev_[3], work_));
    // x is buf[1]
    int cur = 1;
    {
        const int nxt = 0;
        gemm<false, E_LIN>(dec0_, buf[cur], M1_ * rate, 1, rate, nullptr, nullptr, nullptr, buf[nxt], g_.decoder_dim, g_.decoder_dim,
                           tail ? leads[1] : -1);
        cur = nxt;
    }
    int C = g_.decoder_dim;
    for (int k = 0; k < 4; ++k) {                      // SnakeBeta, transposed conv, three residual units (:221-228)
        const Block& bl = blocks_[k];
        const int nxt = (cur + 1) % 3, tmp = (cur + 2) % 3, co = C / 2;
        int lead[3];                                   // of unit j's two launches: what the units behind it read before the block's output lead
        lead[2] = leads[k + 2];
        for (int j = 1; j >= 0; --j) lead[j] = lead[j + 1] + 6 * UNIT_DIL[j + 1];
        gemm<true, E_LIN>(bl.tconv, buf[cur], M1_ * rate, 1, rate, &bl.s, nullptr, nullptr, buf[nxt], bl.tconv.N, co,
                          tail ? cdiv(lead[0] + 6 * UNIT_DIL[0], g_.rates[k]) : -1);
        rate *= g_.rates[k];
        const long M = M1_ * rate;
        for (int j = 0; j < 3; ++j) {
            gemm<true, E_LIN>(bl.u[j].c1, buf[nxt], M, UNIT_DIL[j], rate, &bl.u[j].s1, nullptr, nullptr, buf[tmp], co, co, tail ? lead[j] : -1);
            gemm<true, E_RES>(bl.u[j].c2, buf[tmp], M, 1, rate, &bl.u[j].s2, nullptr, buf[nxt], buf[nxt], co, co, tail ? lead[j] : -1);
        }
        cur = nxt; C = co;
        QASR_HIP(hipEventRecord(ev_[4 + k], work_));
    }
    const long M = M1_ * rate;
    codec_out_launch(tail, buf[cur], M, C, rate, d_fstart_.as<int>(), d_kept_.as<int>(), W(final_snake_.a), W(final_snake_.b), W(final_w_),
                     W(final_b_), clip ? 1 : 0, d_wave_.as<float>(), work_);
    QASR_HIP(hipEventRecord(ev_[8], work_));
    QASR_HIP(hipGetLastError());
}

void CodecQwen3TTS::pass(const CodecWin* w, int n, Mode mode, bool clip, const float* xin, float* xout, bool tail) {
    QASR_HIP(hipSetDevice(device_));
    long M1 = 0;
    for (int i = 0; i < n; ++i) {
        if (w[i].frames < 1 || w[i].frames > CODEC_MAX_T || w[i].context < 0 || w[i].context >= w[i].frames)
            throw std::invalid_argument("speech tokenizer decoder: a window holds 1..35 frames");
        M1 += w[i].frames;
    }
    ensure(M1, mode);
    plan(w, n, mode != PT);
    const size_t F = sizeof(float);
    QASR_HIP(hipEventRecord(ev_[0], work_));
    if (mode != PT) dev_rvq();
    if (mode == RVQ) {
        QASR_HIP(hipEventRecord(ev_[1], work_));
        QASR_HIP(hipMemcpyAsync(xout, d_q_.p, (size_t)M1_ * g_.hidden * F, hipMemcpyDeviceToHost, work_));
        QASR_HIP(hipStreamSynchronize(work_));
        float ms = 0; QASR_HIP(hipEventElapsedTime(&ms, ev_[0], ev_[1])); timing_[0] += ms;
        return;
    }
    if (mode == PT) QASR_HIP(hipMemcpyAsync(d_lat_[0].p, xin, (size_t)M1_ * g_.latent * F, hipMemcpyHostToDevice, work_));
    else gemm<false, E_LIN>(pre_conv_, d_q_.as<float>(), M1_, 1, 1, nullptr, nullptr, nullptr, d_lat_[0].as<float>(), g_.latent, g_.latent);
    QASR_HIP(hipEventRecord(ev_[1], work_));
    dev_pre_transformer();
    QASR_HIP(hipEventRecord(ev_[2], work_));
    if (mode == PT) {
        QASR_HIP(hipMemcpyAsync(xout, d_lat_[1].p, (size_t)M1_ * g_.latent * F, hipMemcpyDeviceToHost, work_));
        QASR_HIP(hipStreamSynchronize(work_));
        float ms = 0; QASR_HIP(hipEventElapsedTime(&ms, ev_[1], ev_[2])); timing_[1] += ms;
        return;
    }
    dev_vocoder(clip, tail && tuning().codec_tail_rows != 0);
    for (int i = 0, off = 0; i < n; off += w[i].frames, ++i)
        QASR_HIP(hipMemcpyAsync(w[i].out, d_wave_.as<float>() + (size_t)(off + w[i].context) * spf_,
                                (size_t)(w[i].frames - w[i].context) * spf_ * F, hipMemcpyDeviceToHost, work_));
    QASR_HIP(hipStreamSynchronize(work_));
    QASR_HIP(hipGetLastError());
    for (int s = 0; s < CODEC_STAGES; ++s) {
        float ms = 0;
        QASR_HIP(hipEventElapsedTime(&ms, ev_[s], ev_[s + 1]));
        timing_[s] += ms;
    }
}

// ---- entry points -------------------------------------------------------------------------------------------------------------------
void CodecQwen3TTS::run(const std::vector<CodecWin>& wins, bool clip, bool tail) {
    check_loaded();
    for (float& t : timing_) t = 0.0f;
    for (size_t i = 0; i < wins.size(); i += (size_t)max_windows_)
        pass(wins.data() + i, (int)std::min(wins.size() - i, (size_t)max_windows_), FULL, clip, nullptr, nullptr, tail);
}

void CodecQwen3TTS::quantizer_decode(const int32_t* codes, int B, int T, float* out) {
    check_loaded();
    for (float& t : timing_) t = 0.0f;
    for (int b0 = 0; b0 < B; b0 += max_windows_) {
        const int n = std::min(B - b0, max_windows_);
        std::vector<CodecWin> w;
        for (int b = b0; b < b0 + n; ++b) w.push_back({codes + (size_t)b * g_.quantizers * T, T, 0, T, 0, nullptr});
        pass(w.data(), n, RVQ, false, nullptr, out + (size_t)b0 * T * g_.hidden);
    }
}

void CodecQwen3TTS::pre_transformer(const float* x, int B, int T, float* out) {
    check_loaded();
    for (float& t : timing_) t = 0.0f;
    for (int b0 = 0; b0 < B; b0 += max_windows_) {
        const int n = std::min(B - b0, max_windows_);
        std::vector<CodecWin> w((size_t)n, CodecWin{nullptr, T, 0, T, 0, nullptr});
        pass(w.data(), n, PT, false, x + (size_t)b0 * T * g_.latent, out + (size_t)b0 * T * g_.latent);
    }
}

}  // namespace qasr
