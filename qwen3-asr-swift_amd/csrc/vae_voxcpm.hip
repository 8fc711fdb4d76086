// vae_voxcpm.hip -- the VoxCPM2 AudioVAE (vae_voxcpm.h).  Launches per direction:
//   a residual unit of width C <= vae_fuse_c   vae_unit_kernel: 64 rows x C with their 6 dil halo in LDS through snake1, the depthwise taps, bias and
//                                              snake2 back to LDS, the C x C pointwise from LDS against conv2's weights held in LDS, + bias + x
//   a wider unit                               vae_dw_kernel (snake1 once per element on the way into LDS, taps, bias, snake2) + the shared f32
//                                              tile with taps = 1 and a plain load (codec_shared.h)
//   transposed conv k 2 s stride s             the tile in the two-tap form: row t -> s output rows, N = s C_out columns sharing C_out biases
//   strided conv k 2 s stride s                the tile behind VaeStrideRows
//   a block's last unit                        applies its one reader's map in the epilogue (snake(v scale + bias), or snake(v)), so no GEMM of
//                                              this model evaluates sinf at an operand load
// A clip's rows lie back to back at every rate: fstart[frame row] = the first frame row of its clip, a row m at `rate` rows per frame may read
// rows >= fstart[m / rate] rate.  Every output is one thread's fmaf chain in an order that does not depend on where its row lies.
#include "vae_voxcpm.h"
#include "codec_shared.h"
#include "json.h"
#include "tuning.h"
#include <cmath>
#include <cstdio>
#include <cstring>

namespace qasr {

// ---- kernels ------------------------------------------------------------------------------------------------------------------------
// y = [snake2](b + sum_j w[j][c] [snake1](x[m - (6 - j) dil][c])), j = 0..6 in order.  grid (row slabs of 64, channel tiles of 64),
// LDS (64 + 6 dil) x 64 floats.
template <bool SIN, bool SOUT>
__global__ __launch_bounds__(256) void vae_dw_kernel(const float* __restrict__ x, long M, int C, int dil, const int* __restrict__ fstart, int rate,
                                                     const float* __restrict__ w, const float* __restrict__ b, const float* __restrict__ a1,
                                                     const float* __restrict__ i1, const float* __restrict__ a2, const float* __restrict__ i2,
                                                     float* __restrict__ y) {
    extern __shared__ __attribute__((aligned(16))) float av_lds[];
    float* xs = av_lds;
    const int tid = threadIdx.x, cl = tid & 63, rg = tid >> 6, halo = 6 * dil, c = blockIdx.y * 64 + cl;
    const long m0 = (long)blockIdx.x * AV_SLAB;
    const bool live = c < C;
    const float sa = SIN && live ? a1[c] : 0.0f, si = SIN && live ? i1[c] : 0.0f;
    for (int i = rg; i < AV_SLAB + halo; i += 4) {
        const long g = m0 - halo + i;
        float v = 0.0f;
        if (live && g >= 0 && g < M) {
            v = x[g * C + c];
            if (SIN) v = codec_snake(v, sa, si);
        }
        xs[i * 64 + cl] = v;
    }
    __syncthreads();
    if (!live) return;
    float wj[7];
#pragma unroll
    for (int j = 0; j < 7; ++j) wj[j] = w[j * C + c];
    const float bias = b[c], oa = SOUT ? a2[c] : 0.0f, oi = SOUT ? i2[c] : 0.0f;
    for (int r = rg; r < AV_SLAB; r += 4) {
        const long m = m0 + r;
        if (m >= M) break;
        const long first = (long)fstart[m / rate] * rate;
        float acc = 0.0f;
#pragma unroll
        for (int j = 0; j < 7; ++j)
            if (m - (long)(6 - j) * dil >= first) acc = fmaf(xs[(r + j * dil) * 64 + cl], wj[j], acc);
        acc = acc + bias;
        if (SOUT) acc = codec_snake(acc, oa, oi);
        y[m * C + c] = acc;
    }
}

__host__ __device__ inline size_t vae_unit_lds(int C, int dil) {
    return ((size_t)(AV_SLAB + 6 * dil) * C + (size_t)C * C + (size_t)AV_SLAB * (C + 4) + AV_SLAB) * sizeof(float);
}

// A whole residual unit for 64 rows x C channels (C a multiple of 4, at most AV_FUSE_MAX): y = map(x + b2 + sum_c h[c] Wt[c][n]), c = 0..C-1
// in order, h = snake2(b1 + sum_j w1[j][c] snake1(x[m - (6 - j) dil][c])).  A thread owns RPT rows x 4 columns; C / 4 column groups.
template <int RPT>
__global__ __launch_bounds__(256) void vae_unit_kernel(const float* __restrict__ x, long M, int C, int dil, const int* __restrict__ fstart, int rate,
                                                       const float* __restrict__ w1, const float* __restrict__ b1, const float* __restrict__ a1,
                                                       const float* __restrict__ i1, const float* __restrict__ a2, const float* __restrict__ i2,
                                                       const float* __restrict__ Wt, const float* __restrict__ b2, const float* __restrict__ ma,
                                                       const float* __restrict__ mi, const float* __restrict__ aff, float* __restrict__ y) {
    extern __shared__ __attribute__((aligned(16))) float av_lds[];
    const int halo = 6 * dil, C4 = C >> 2, ldh = C + 4, tid = threadIdx.x;
    float* xs = av_lds;                                // [64 + halo][C] through snake1
    float* ws = xs + (size_t)(AV_SLAB + halo) * C;     // [C][C]
    float* hs = ws + (size_t)C * C;                    // [64][C + 4]
    int* firsts = reinterpret_cast<int*>(hs + (size_t)AV_SLAB * ldh);
    const long m0 = (long)blockIdx.x * AV_SLAB;
    for (int i = tid; i < C * C4; i += 256) *reinterpret_cast<float4*>(ws + 4 * i) = *reinterpret_cast<const float4*>(Wt + 4 * i);
    for (int i = tid; i < (AV_SLAB + halo) * C4; i += 256) {
        const int row = i / C4, q = i - row * C4;
        const long g = m0 - halo + row;
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (g >= 0 && g < M) {
            v = *reinterpret_cast<const float4*>(x + g * C + 4 * q);
            const float4 a = *reinterpret_cast<const float4*>(a1 + 4 * q), iv = *reinterpret_cast<const float4*>(i1 + 4 * q);
            v.x = codec_snake(v.x, a.x, iv.x); v.y = codec_snake(v.y, a.y, iv.y);
            v.z = codec_snake(v.z, a.z, iv.z); v.w = codec_snake(v.w, a.w, iv.w);
        }
        *reinterpret_cast<float4*>(xs + (size_t)row * C + 4 * q) = v;
    }
    if (tid < AV_SLAB) {
        const long m = m0 + tid;
        firsts[tid] = m < M ? fstart[m / rate] * rate : 0;
    }
    __syncthreads();
    for (int i = tid; i < AV_SLAB * C4; i += 256) {
        const int r = i / C4, q = i - r * C4;
        const long m = m0 + r;
        float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (m < M) {
            const long first = firsts[r];
#pragma unroll
            for (int j = 0; j < 7; ++j) {
                if (m - (long)(6 - j) * dil < first) continue;
                const float4 v = lds_read_f4(xs + (size_t)(r + j * dil) * C + 4 * q);
                const float4 wv = *reinterpret_cast<const float4*>(w1 + j * C + 4 * q);
                acc.x = fmaf(v.x, wv.x, acc.x); acc.y = fmaf(v.y, wv.y, acc.y);
                acc.z = fmaf(v.z, wv.z, acc.z); acc.w = fmaf(v.w, wv.w, acc.w);
            }
            const float4 bb = *reinterpret_cast<const float4*>(b1 + 4 * q), a = *reinterpret_cast<const float4*>(a2 + 4 * q),
                         iv = *reinterpret_cast<const float4*>(i2 + 4 * q);
            acc.x = codec_snake(acc.x + bb.x, a.x, iv.x); acc.y = codec_snake(acc.y + bb.y, a.y, iv.y);
            acc.z = codec_snake(acc.z + bb.z, a.z, iv.z); acc.w = codec_snake(acc.w + bb.w, a.w, iv.w);
        }
        *reinterpret_cast<float4*>(hs + (size_t)r * ldh + 4 * q) = acc;
    }
    __syncthreads();
    const int cg = tid % C4, r0 = (tid / C4) * RPT;
    if (r0 >= AV_SLAB) return;
    float acc[RPT][4];
#pragma unroll
    for (int i = 0; i < RPT; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[i][q] = 0.0f;
    for (int c0 = 0; c0 < C; c0 += 4) {
        float hv[RPT][4];
#pragma unroll
        for (int i = 0; i < RPT; ++i) {
            const float4 h = r0 + i < AV_SLAB ? lds_read_f4(hs + (size_t)(r0 + i) * ldh + c0) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            hv[i][0] = h.x; hv[i][1] = h.y; hv[i][2] = h.z; hv[i][3] = h.w;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float4 wv = lds_read_f4(ws + (size_t)(c0 + k) * C + 4 * cg);
#pragma unroll
            for (int i = 0; i < RPT; ++i) {
                acc[i][0] = fmaf(hv[i][k], wv.x, acc[i][0]); acc[i][1] = fmaf(hv[i][k], wv.y, acc[i][1]);
                acc[i][2] = fmaf(hv[i][k], wv.z, acc[i][2]); acc[i][3] = fmaf(hv[i][k], wv.w, acc[i][3]);
            }
        }
    }
    const int n = 4 * cg;
    const float4 bb = *reinterpret_cast<const float4*>(b2 + n);
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
        const long m = m0 + r0 + i;
        if (r0 + i >= AV_SLAB || m >= M) continue;
        const float4 res = *reinterpret_cast<const float4*>(x + m * C + n);
        float v[4] = {(acc[i][0] + bb.x) + res.x, (acc[i][1] + bb.y) + res.y, (acc[i][2] + bb.z) + res.z, (acc[i][3] + bb.w) + res.w};
        if (ma) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (aff) v[q] = v[q] * aff[n + q] + aff[C + n + q];
                v[q] = codec_snake(v[q], ma[n + q], mi[n + q]);
            }
        }
        *reinterpret_cast<float4*>(y + m * C + n) = make_float4(v[0], v[1], v[2], v[3]);
    }
}

// the encoder's conv_in: y[m][n] = b[n] + sum_j pcm[m - (6 - j)] w[j][n]
__global__ __launch_bounds__(256) void vae_convin_kernel(const float* __restrict__ pcm, long M, int D, const int* __restrict__ fstart, int rate,
                                                         const float* __restrict__ w, const float* __restrict__ b, float* __restrict__ y) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= M * D) return;
    const long m = i / D;
    const int n = (int)(i - m * D);
    const long first = (long)fstart[m / rate] * rate;
    float acc = 0.0f;
#pragma unroll
    for (int j = 0; j < 7; ++j)
        if (m - (6 - j) >= first) acc = fmaf(pcm[m - (6 - j)], w[j * D + n], acc);
    y[i] = acc + b[n];
}

// conv_out + tanh: pcm[m] = tanh(b + sum_j sum_c x[m - (6 - j)][c] w[j][c]), j then c in order; x already through snake_out
// (SNAKE: applied here at the load, for the stage entry that starts from the raw rows).  LDS: w [7][C] | alpha [C] | 1 / alpha [C].
template <bool SNAKE>
__global__ __launch_bounds__(256) void vae_out_kernel(const float* __restrict__ x, long M, int C, const int* __restrict__ fstart, int rate,
                                                      const float* __restrict__ w, const float* __restrict__ b, const float* __restrict__ a,
                                                      const float* __restrict__ inv, float* __restrict__ pcm) {
    extern __shared__ __attribute__((aligned(16))) float av_lds[];
    float *ws = av_lds, *as = ws + 7 * C, *is = as + C;
    for (int i = threadIdx.x; i < 7 * C; i += 256) ws[i] = w[i];
    if (SNAKE)
        for (int i = threadIdx.x; i < C; i += 256) { as[i] = a[i]; is[i] = inv[i]; }
    __syncthreads();
    const long m = (long)blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    const long first = (long)fstart[m / rate] * rate;
    float acc = 0.0f;
    for (int j = 0; j < 7; ++j) {
        const long src = m - (6 - j);
        if (src < first) continue;
        const float* row = x + src * C;
        if ((C & 3) == 0) {
            for (int c = 0; c < C; c += 4) {
                float4 v = *reinterpret_cast<const float4*>(row + c);
                if (SNAKE) {
                    v.x = codec_snake(v.x, as[c], is[c]); v.y = codec_snake(v.y, as[c + 1], is[c + 1]);
                    v.z = codec_snake(v.z, as[c + 2], is[c + 2]); v.w = codec_snake(v.w, as[c + 3], is[c + 3]);
                }
                const float* wr = ws + j * C + c;
                acc = fmaf(v.x, wr[0], acc); acc = fmaf(v.y, wr[1], acc); acc = fmaf(v.z, wr[2], acc); acc = fmaf(v.w, wr[3], acc);
            }
        } else {
            for (int c = 0; c < C; ++c) {
                float v = row[c];
                if (SNAKE) v = codec_snake(v, as[c], is[c]);
                acc = fmaf(v, ws[j * C + c], acc);
            }
        }
    }
    pcm[m] = tanhf(acc + b[0]);
}

// ---- configuration and weights (host) -----------------------------------------------------------------------------------------------
static std::vector<int> json_ints(const Json* j, std::vector<int> dflt, const std::string& who, const char* field) {
    if (!j || j->type == Json::Null) return dflt;
    if (j->type != Json::Arr) throw std::invalid_argument(who + field + " is not a list");
    std::vector<int> v;
    for (const Json& e : j->arr) {
        if (e.type != Json::Num) throw std::invalid_argument(who + field + " holds a non-number");
        v.push_back((int)e.num);
    }
    return v;
}

AvaeConfig avae_read_config(const std::string& model_dir, const char* who_c) {
    const std::string who = std::string(who_c) + ": ";
    AvaeConfig c;
    std::string text;
    if (FILE* f = fopen((model_dir + "/config.json").c_str(), "rb")) {
        char buf[4096];
        size_t n;
        while ((n = fread(buf, 1, sizeof buf, f)) > 0) text.append(buf, n);
        fclose(f);
    }
    if (!text.empty()) {
        Json root;
        try { root = JsonParser(text.data(), text.size()).parse(); }
        catch (const std::exception& ex) { throw std::invalid_argument(who + "config.json: " + ex.what()); }
        if (const Json* a = root.get("audio_vae_config")) {
            auto num = [&](const char* k, int& v) { if (const Json* j = a->get(k)) if (j->type == Json::Num) v = (int)j->num; };
            auto flag = [&](const char* k, bool& v) { if (const Json* j = a->get(k)) if (j->type == Json::Bool) v = j->b; };
            num("encoder_dim", c.encoder_dim); num("latent_dim", c.latent_dim); num("decoder_dim", c.decoder_dim);
            num("sample_rate", c.sample_rate); num("out_sample_rate", c.out_sample_rate);
            flag("depthwise", c.depthwise); flag("use_noise_block", c.use_noise_block);
            c.encoder_rates = json_ints(a->get("encoder_rates"), c.encoder_rates, who, "encoder_rates");
            c.decoder_rates = json_ints(a->get("decoder_rates"), c.decoder_rates, who, "decoder_rates");
            c.sr_bin_boundaries = json_ints(a->get("sr_bin_boundaries"), c.sr_bin_boundaries, who, "sr_bin_boundaries");
            if (const Json* j = a->get("cond_type")) if (j->type == Json::Str) c.cond_type = j->str;
        }
    }
    if (c.use_noise_block) throw std::invalid_argument(who + "use_noise_block is true: the noise block draws MLXRandom noise, which is not reproduced");
    if (!c.depthwise) throw std::invalid_argument(who + "depthwise is false: only the depthwise residual units are built");
    if (c.cond_type != "scale_bias" && c.cond_type != "scale_bias_init") throw std::invalid_argument(who + "cond_type \"" + c.cond_type + "\" is not scale_bias or scale_bias_init");
    auto rates = [&](const std::vector<int>& r, const char* f) {
        if (r.empty() || r.size() > (size_t)AV_MAX_RATES) throw std::invalid_argument(who + f + " holds 1.." + std::to_string(AV_MAX_RATES) + " rates");
        for (int s : r) if (s < 1 || s > 16) throw std::invalid_argument(who + f + " holds a rate outside 1..16");
    };
    rates(c.encoder_rates, "encoder_rates");
    rates(c.decoder_rates, "decoder_rates");
    if (c.encoder_dim < 1 || c.encoder_dim > 4096) throw std::invalid_argument(who + "encoder_dim outside 1..4096");
    if (c.latent_dim < 1 || c.latent_dim > 4096) throw std::invalid_argument(who + "latent_dim outside 1..4096");
    if (c.decoder_dim < 1 || c.decoder_dim > 8192 || c.decoder_dim % (1 << c.decoder_rates.size()))
        throw std::invalid_argument(who + "decoder_dim is not a multiple of 2^(number of decoder_rates) in 1..8192");
    if (c.sample_rate < 1 || c.out_sample_rate < 1) throw std::invalid_argument(who + "sample_rate / out_sample_rate must be positive");
    if (c.sr_bin_boundaries.size() > 64) throw std::invalid_argument(who + "sr_bin_boundaries holds more than 64 values");
    return c;
}

using Shapes = std::vector<std::pair<std::string, std::vector<int64_t>>>;

// the names (without the audio_vae. prefix) and shapes the reference's modules hold
static Shapes avae_shapes(const AvaeConfig& c) {
    Shapes s;
    auto conv = [&](const std::string& k, int out, int kk, int in) { s.push_back({k + ".weight", {out, kk, in}}); s.push_back({k + ".bias", {out}}); };
    auto snake = [&](const std::string& k, int C) { s.push_back({k + ".alpha", {1, 1, C}}); };
    auto unit = [&](const std::string& p, int C) {
        snake(p + ".snake1", C); conv(p + ".conv1", C, 7, 1); snake(p + ".snake2", C); conv(p + ".conv2", C, 1, C);
    };
    conv("encoder.conv_in", c.encoder_dim, 7, 1);
    int C = c.encoder_dim;
    for (size_t i = 0; i < c.encoder_rates.size(); ++i, C *= 2) {
        const std::string p = "encoder.blocks.layers." + std::to_string(i);
        for (int u = 1; u <= 3; ++u) unit(p + ".res" + std::to_string(u), C);
        snake(p + ".snake", C);
        conv(p + ".conv", 2 * C, 2 * c.encoder_rates[i], C);
    }
    conv("encoder.fc_mu", c.latent_dim, 3, C);
    conv("decoder.conv_in.layers.0", c.latent_dim, 7, 1);
    conv("decoder.conv_in.layers.1", c.decoder_dim, 1, c.latent_dim);
    C = c.decoder_dim;
    const int buckets = (int)c.sr_bin_boundaries.size() + 1;
    for (size_t i = 0; i < c.decoder_rates.size(); ++i, C /= 2) {
        const std::string p = "decoder.blocks.layers." + std::to_string(i), q = "decoder.sr_cond_layers." + std::to_string(i);
        s.push_back({q + ".scale_embed.weight", {buckets, C}});
        s.push_back({q + ".bias_embed.weight", {buckets, C}});
        snake(p + ".snake", C);
        conv(p + ".conv_t", C / 2, 2 * c.decoder_rates[i], C);
        for (int u = 1; u <= 3; ++u) unit(p + ".res" + std::to_string(u), C / 2);
    }
    snake("decoder.snake_out", C);
    conv("decoder.conv_out", 1, 7, C);
    return s;
}

CheckedWeights avae_load_weights(const std::string& model_dir, const char* who, const AvaeConfig& cfg) {
    const std::string pre = std::string(who) + ": ";
    std::unique_ptr<SafeTensorsDir> st;
    try { st = std::make_unique<SafeTensorsDir>(model_dir); }
    catch (const std::exception& ex) { throw WeightLoadError(QASR_ERR_IO, pre + ex.what()); }
    auto stored = [&](const std::string& k) -> std::string {      // the spelling the checkpoint uses, "" when it has neither
        if (st->entries.count("audio_vae." + k)) return "audio_vae." + k;
        if (st->entries.count(k)) return k;
        return "";
    };
    const Shapes want = avae_shapes(cfg);
    Shapes ask;                                        // what is read, in the checkpoint's spelling; a missing tensor is named in full
    std::vector<int> kind(want.size(), 0);             // 0 as stored | 1 weight_g + weight_v
    for (size_t i = 0; i < want.size(); ++i) {
        const std::string& k = want[i].first;
        std::vector<int64_t> shape = want[i].second;
        std::string at = stored(k);
        const bool is_weight = k.size() > 7 && k.compare(k.size() - 7, 7, ".weight") == 0;
        if (at.empty() && is_weight && shape.size() == 3) {
            const std::string g = stored(k + "_g"), v = stored(k + "_v");
            if (!g.empty() && !v.empty()) {
                kind[i] = 1;
                ask.push_back({g, {shape[0], 1, 1}});
                ask.push_back({v, shape});
                continue;
            }
        }
        if (!at.empty() && shape.size() == 2 && shape[1] == 64 && st->entries.at(at).shape.size() == 3) shape = {shape[0], 8, 8};   // TableEmbedding
        ask.push_back({at.empty() ? "audio_vae." + k : at, shape});
    }
    const CheckedWeights raw = load_checked_f32(*st, who, ask, false);
    CheckedWeights out;
    out.disk_bytes = raw.disk_bytes;
    size_t a = 0;
    for (size_t i = 0; i < want.size(); ++i) {
        if (kind[i] == 0) { out.t[want[i].first] = raw.t.at(ask[a++].first); continue; }
        const std::vector<float>&g = raw.t.at(ask[a].first), &v = raw.t.at(ask[a + 1].first);
        a += 2;
        // g v / (|v| + 1e-9), the norm over everything but the first axis (:656-667); formed in f64 and rounded once
        const size_t rows = g.size(), per = v.size() / rows;
        std::vector<float> w(v.size());
        for (size_t r = 0; r < rows; ++r) {
            double ss = 0.0;
            for (size_t e = 0; e < per; ++e) ss += (double)v[r * per + e] * (double)v[r * per + e];
            const double nrm = std::sqrt(ss) + 1e-9;
            for (size_t e = 0; e < per; ++e) w[r * per + e] = (float)((double)g[r] * ((double)v[r * per + e] / nrm));
        }
        out.t[want[i].first] = std::move(w);
    }
    return out;
}

// ---- the host object ----------------------------------------------------------------------------------------------------------------
static const char* const WHO = "AudioVAE";

template <int RPT> static void unit_lds_limit() {
    ensure_dynamic_lds(reinterpret_cast<const void*>(&vae_unit_kernel<RPT>), (int)vae_unit_lds(AV_FUSE_MAX, 9));
}

AudioVaeVoxcpm::AudioVaeVoxcpm(int device, const AvaeConfig& cfg, const CheckedWeights& cw, long max_frames, hipStream_t work)
    : device_(device), cfg_(cfg), max_frames_(max_frames) {
    if (max_frames < 1 || max_frames > AV_MAX_FRAMES) throw std::invalid_argument(std::string(WHO) + ": max_frames in 1..2^14");
    param_bytes_ = cw.disk_bytes;
    Builder b(cw);
    // Wt[j C_in + c][n] = W[n][j][c] of a conv stored [out][k][in]
    auto conv = [&](const std::string& key, int Cout, int k, int Cin) {
        Gemm g; g.K = k * Cin; g.N = Cout; g.Cin = Cin; g.taps = k; g.bmod = Cout;
        const auto& Wm = b.t(key + ".weight");
        g.wt = b.take((size_t)g.K * g.N);
        for (int n = 0; n < Cout; ++n)
            for (int kk = 0; kk < g.K; ++kk) b.h[g.wt + (size_t)kk * Cout + n] = Wm[(size_t)n * g.K + kk];
        g.bias = b.vec(key + ".bias");
        return g;
    };
    // the trimmed transposed conv as two taps on the input rows: column r C_out + o of row t is output row t s + r,
    // Wt[c][..] = W[o][r + s][c] under x[t - 1] (tap 0), Wt[C_in + c][..] = W[o][r][c] under x[t] (tap 1)
    auto conv_t = [&](const std::string& key, int Cout, int s, int Cin) {
        Gemm g; g.K = 2 * Cin; g.N = s * Cout; g.Cin = Cin; g.taps = 2; g.bmod = Cout;
        const auto& Wm = b.t(key + ".weight");           // [out][2 s][in]
        g.wt = b.take((size_t)g.K * g.N);
        for (int o = 0; o < Cout; ++o)
            for (int r = 0; r < s; ++r)
                for (int c = 0; c < Cin; ++c) {
                    b.h[g.wt + (size_t)c * g.N + r * Cout + o] = Wm[((size_t)o * 2 * s + r + s) * Cin + c];
                    b.h[g.wt + (size_t)(Cin + c) * g.N + r * Cout + o] = Wm[((size_t)o * 2 * s + r) * Cin + c];
                }
        g.bias = b.vec(key + ".bias");
        return g;
    };
    auto taps7 = [&](const std::string& key, int C, bool per_out = true) {   // [C][7][1], or (conv_out) [1][7][C], -> [7][C]
        const auto& Wm = b.t(key + ".weight");
        const size_t at = b.take((size_t)7 * C);
        for (int c = 0; c < C; ++c)
            for (int j = 0; j < 7; ++j) b.h[at + (size_t)j * C + c] = per_out ? Wm[(size_t)c * 7 + j] : Wm[(size_t)j * C + c];
        return at;
    };
    auto snake = [&](const std::string& key, int C) {
        Snake s; s.a = b.vec(key + ".alpha"); s.inv = b.take(C);
        for (int c = 0; c < C; ++c) b.h[s.inv + c] = 1.0f / (b.h[s.a + c] + 1e-9f);
        return s;
    };
    auto unit = [&](const std::string& p, int C, int dil) {
        Unit u; u.C = C; u.dil = dil;
        u.s1 = snake(p + ".snake1", C); u.w1 = taps7(p + ".conv1", C); u.b1 = b.vec(p + ".conv1.bias");
        u.s2 = snake(p + ".snake2", C); u.c2 = conv(p + ".conv2", C, 1, C);
        return u;
    };
    static const int DIL[3] = {1, 3, 9};
    enc_in_w_ = taps7("encoder.conv_in", cfg.encoder_dim); enc_in_b_ = b.vec("encoder.conv_in.bias");
    int C = cfg.encoder_dim;
    for (size_t i = 0; i < cfg.encoder_rates.size(); ++i, C *= 2) {
        const std::string p = "encoder.blocks.layers." + std::to_string(i);
        for (int u = 0; u < 3; ++u) enc_units_.push_back(unit(p + ".res" + std::to_string(u + 1), C, DIL[u]));
        enc_snake_.push_back(snake(p + ".snake", C));
        enc_down_.push_back(conv(p + ".conv", 2 * C, 2 * cfg.encoder_rates[i], C));
    }
    fc_mu_ = conv("encoder.fc_mu", cfg.latent_dim, 3, C);
    size_t widest = (size_t)cfg.hop() * cfg.encoder_dim;   // floats per latent frame of the widest level: rows x width is the same
    {                                                      // at every encoder level but the first, and grows with the decoder's
        long rows = cfg.hop(); int w = cfg.encoder_dim;
        for (int s : cfg.encoder_rates) { rows /= s; w *= 2; widest = std::max(widest, (size_t)rows * w); }
    }
    dec_in_w_ = taps7("decoder.conv_in.layers.0", cfg.latent_dim); dec_in_b_ = b.vec("decoder.conv_in.layers.0.bias");
    dec_in1_ = conv("decoder.conv_in.layers.1", cfg.decoder_dim, 1, cfg.latent_dim);
    C = cfg.decoder_dim;
    const int buckets = (int)cfg.sr_bin_boundaries.size() + 1;
    long rows = 1;
    widest = std::max(widest, (size_t)C);
    for (size_t i = 0; i < cfg.decoder_rates.size(); ++i, C /= 2) {
        const std::string p = "decoder.blocks.layers." + std::to_string(i), q = "decoder.sr_cond_layers." + std::to_string(i);
        const auto &sc = b.t(q + ".scale_embed.weight"), &bi = b.t(q + ".bias_embed.weight");
        const size_t at = b.take((size_t)buckets * 2 * C);
        for (int k = 0; k < buckets; ++k)
            for (int c = 0; c < C; ++c) {
                b.h[at + ((size_t)k * 2) * C + c] = sc[(size_t)k * C + c];
                b.h[at + ((size_t)k * 2 + 1) * C + c] = bi[(size_t)k * C + c];
            }
        affine_.push_back(at);
        dec_snake_.push_back(snake(p + ".snake", C));
        dec_up_.push_back(conv_t(p + ".conv_t", C / 2, cfg.decoder_rates[i], C));
        for (int u = 0; u < 3; ++u) dec_units_.push_back(unit(p + ".res" + std::to_string(u + 1), C / 2, DIL[u]));
        rows *= cfg.decoder_rates[i];
        widest = std::max(widest, (size_t)rows * (C / 2));
    }
    dec_snake_.push_back(snake("decoder.snake_out", C));
    out_w_ = taps7("decoder.conv_out", C, false); out_b_ = b.vec("decoder.conv_out.bias");
    if ((size_t)max_frames * std::max(cfg.hop(), cfg.samples_per_frame()) > (size_t)1 << 30)
        throw std::invalid_argument(std::string(WHO) + ": max_frames x the rows of a frame exceeds 2^30");
    QASR_HIP(hipSetDevice(device_));
    unit_lds_limit<1>(); unit_lds_limit<2>(); unit_lds_limit<4>(); unit_lds_limit<8>();
    QASR_HIP(hipStreamCreateWithFlags(&own_, hipStreamNonBlocking));
    work_ = work ? work : own_;
    for (auto& e : ev_) QASR_HIP(hipEventCreate(&e));
    d_w_.alloc(b.h.size() * sizeof(float));
    QASR_HIP(hipMemcpy(d_w_.p, b.h.data(), b.h.size() * sizeof(float), hipMemcpyHostToDevice));
    const size_t F = sizeof(float), T = (size_t)max_frames;
    d_fstart_.alloc(T * sizeof(int));
    d_pcm_.alloc(T * std::max(cfg.hop(), cfg.samples_per_frame()) * F);
    d_z_.alloc(T * cfg.latent_dim * F);
    for (auto& buf : d_b_) buf.alloc(T * widest * F);
}

AudioVaeVoxcpm::~AudioVaeVoxcpm() {
    if (work_) (void)hipStreamSynchronize(work_);
    for (auto& e : ev_) if (e) (void)hipEventDestroy(e);
    if (own_) (void)hipStreamDestroy(own_);
}

void AudioVaeVoxcpm::unload() {
    if (!loaded_) return;
    QASR_HIP(hipSetDevice(device_));
    QASR_HIP(hipStreamSynchronize(work_));
    for (DevBuf* b : {&d_w_, &d_fstart_, &d_pcm_, &d_z_, &d_b_[0], &d_b_[1], &d_b_[2]}) b->release();
    loaded_ = false;
}

void AudioVaeVoxcpm::check_loaded() const {
    if (!loaded_) throw NotLoaded(std::string(WHO) + ": model unloaded");
}

bool AudioVaeVoxcpm::stage_shape(bool decoder, int k, int* rows_per_frame, int* width) const {
    const std::vector<int>& r = decoder ? cfg_.decoder_rates : cfg_.encoder_rates;
    if (k < 0 || k > (int)r.size()) return false;
    long rows = decoder ? 1 : cfg_.hop();
    int w = decoder ? cfg_.decoder_dim : cfg_.encoder_dim;
    for (int i = 0; i < k; ++i) {
        if (decoder) { rows *= r[i]; w /= 2; } else { rows /= r[i]; w *= 2; }
    }
    *rows_per_frame = (int)rows;
    *width = w;
    return true;
}

// ---- launches -----------------------------------------------------------------------------------------------------------------------
// vae_dw_kernel's launch entry (codec_launch.h): AudioVaeVoxcpm and qasr_codec_case_probe call this.  The two forms the model has: both
// snakes (a residual unit's depthwise conv) or neither (the decoder's conv_in)
void vae_dw_launch(bool snakes, const float* x, long M, int C, int dil, const int* fstart, int rate, const float* w, const float* b, const float* a1,
                   const float* i1, const float* a2, const float* i2, float* y, hipStream_t s) {
    const dim3 grid((unsigned)cdiv(M, (long)AV_SLAB), (unsigned)cdiv(C, 64));
    const size_t lds = (size_t)(AV_SLAB + 6 * dil) * 64 * sizeof(float);
    if (snakes) hipLaunchKernelGGL((vae_dw_kernel<true, true>), grid, dim3(256), lds, s, x, M, C, dil, fstart, rate, w, b, a1, i1, a2, i2, y);
    else hipLaunchKernelGGL((vae_dw_kernel<false, false>), grid, dim3(256), lds, s, x, M, C, dil, fstart, rate, w, b, a1, i1, a2, i2, y);
}

// vae_unit_kernel's launch entry (codec_launch.h): AudioVaeVoxcpm::unit and qasr_codec_case_probe call this.  A thread owns RPT rows x 4
// columns: 256 / (C / 4) threads share a column group, RPT is the power of two that lets them cover the slab's 64 rows
void vae_unit_launch(const float* x, long M, int C, int dil, const int* fstart, int rate, const float* w1, const float* b1, const float* a1,
                     const float* i1, const float* a2, const float* i2, const float* Wt, const float* b2, const float* ma, const float* mi,
                     const float* aff, float* y, hipStream_t s) {
    if (C < 4 || C > AV_FUSE_MAX || (C & 3) || dil < 1 || dil > 9)
        throw std::invalid_argument("vae_unit_launch: C a multiple of 4 in [4, AV_FUSE_MAX], dil in [1, 9]");
    const dim3 slabs((unsigned)cdiv(M, (long)AV_SLAB));
    const int per = 256 / (C / 4), need = (AV_SLAB + per - 1) / per, rpt = need <= 1 ? 1 : need <= 2 ? 2 : need <= 4 ? 4 : 8;
    const size_t lds = vae_unit_lds(C, dil);
#define AV_UNIT(R)                                                                                                                    \
    do {                                                                                                                              \
        unit_lds_limit<R>();                                                                                                          \
        hipLaunchKernelGGL((vae_unit_kernel<R>), slabs, dim3(256), lds, s, x, M, C, dil, fstart, rate, w1, b1, a1, i1, a2, i2, Wt, b2, ma, mi, \
                           aff, y);                                                                                                   \
    } while (0)
    if (rpt == 1) AV_UNIT(1); else if (rpt == 2) AV_UNIT(2); else if (rpt == 4) AV_UNIT(4); else AV_UNIT(8);
#undef AV_UNIT
}

void AudioVaeVoxcpm::gemm(const Gemm& g, int epi, long rows, int rate, int stride, const float* A, const float* R, float* C, const Map& map) {
    CodecRowsArg ra;
    ra.a = d_fstart_.as<int>();
    ra.rate = rate;
    const float* none = nullptr;
    if (stride > 0) {
        ra.kind = CODEC_ROWS_VAE_STRIDE;
        ra.stride = stride;
        codec_tile_launch(ra, false, E_LIN, A, rows, g.Cin, g.taps, 1, W(g.wt), g.K, g.N, W(g.bias), g.bmod, none, none, none, none, C, g.N, work_);
        return;
    }
    if (epi == E_LIN)
        codec_tile_launch(ra, false, E_LIN, A, rows, g.Cin, g.taps, 1, W(g.wt), g.K, g.N, W(g.bias), g.bmod, none, none, none, none, C, g.N, work_);
    else if (epi == E_RES)
        codec_tile_launch(ra, false, E_RES, A, rows, g.Cin, g.taps, 1, W(g.wt), g.K, g.N, W(g.bias), g.bmod, none, none, none, R, C, g.N, work_);
    else
        codec_tile_launch(ra, false, E_RESMAP, A, rows, g.Cin, g.taps, 1, W(g.wt), g.K, g.N, W(g.bias), g.bmod, map.a, map.inv, map.affine, R, C, g.N,
                          work_);
}

// y = map(x + conv2(snake2(conv1(snake1(x))))); t is scratch of the wide path; y is not x
void AudioVaeVoxcpm::unit(const Unit& u, long rows, int rate, const float* x, float* t, float* y, const Map& map) {
    const int* fs = d_fstart_.as<int>();
    const int fuse = tuning().vae_fuse_c, C = u.C;
    if (C <= fuse && C <= AV_FUSE_MAX && (C & 3) == 0) {
        vae_unit_launch(x, rows, C, u.dil, fs, rate, W(u.w1), W(u.b1), W(u.s1.a), W(u.s1.inv), W(u.s2.a), W(u.s2.inv), W(u.c2.wt), W(u.c2.bias), map.a,
                        map.inv, map.affine, y, work_);
        return;
    }
    vae_dw_launch(true, x, rows, C, u.dil, fs, rate, W(u.w1), W(u.b1), W(u.s1.a), W(u.s1.inv), W(u.s2.a), W(u.s2.inv), t, work_);
    gemm(u.c2, map.a ? E_RESMAP : E_RES, rows, rate, 0, t, x, y, map);
}

void AudioVaeVoxcpm::finish(int first, int count) {
    QASR_HIP(hipStreamSynchronize(work_));
    QASR_HIP(hipGetLastError());
    for (int s = 0; s < count; ++s) {
        float ms = 0;
        QASR_HIP(hipEventElapsedTime(&ms, ev_[s], ev_[s + 1]));
        timing_[first + s] += ms;
    }
}

// d_pcm_ -> d_z_, or a stage's rows in d_b_[0].  Records ev_[0 ..]; returns through finish() in the callers.
void AudioVaeVoxcpm::run_encoder(int stage) {
    const int* fs = d_fstart_.as<int>();
    float *A = d_b_[0].as<float>(), *B = d_b_[1].as<float>(), *T = d_b_[2].as<float>();
    const int nb = (int)cfg_.encoder_rates.size();
    long rpf = cfg_.hop();
    int C = cfg_.encoder_dim, e = 0;
    QASR_HIP(hipEventRecord(ev_[e++], work_));
    hipLaunchKernelGGL(vae_convin_kernel, dim3((unsigned)cdiv(frames_ * rpf * C, 256L)), dim3(256), 0, work_, d_pcm_.as<float>(), frames_ * rpf, C, fs,
                       (int)rpf, W(enc_in_w_), W(enc_in_b_), A);
    QASR_HIP(hipEventRecord(ev_[e++], work_));
    for (int i = 0; i < nb && stage != i; ++i, C *= 2) {
        const long rows = frames_ * rpf;
        const Map snake{W(enc_snake_[i].a), W(enc_snake_[i].inv), nullptr};
        unit(enc_units_[3 * i], rows, (int)rpf, A, T, B, Map{});
        unit(enc_units_[3 * i + 1], rows, (int)rpf, B, T, A, Map{});
        unit(enc_units_[3 * i + 2], rows, (int)rpf, A, T, B, snake);
        const int s = cfg_.encoder_rates[i];
        rpf /= s;
        gemm(enc_down_[i], E_LIN, frames_ * rpf, (int)rpf, s, B, nullptr, A, Map{});
        QASR_HIP(hipEventRecord(ev_[e++], work_));
    }
    if (stage < 0) gemm(fc_mu_, E_LIN, frames_, 1, 0, A, nullptr, d_z_.as<float>(), Map{});
    for (; e <= nb + 2; ++e) QASR_HIP(hipEventRecord(ev_[e], work_));
    QASR_HIP(hipGetLastError());
}

// d_z_ -> d_pcm_, or a stage's rows in d_b_[0]
void AudioVaeVoxcpm::run_decoder(int idx, int stage) {
    const int* fs = d_fstart_.as<int>();
    float *A = d_b_[0].as<float>(), *B = d_b_[1].as<float>(), *T = d_b_[2].as<float>();
    const int nb = (int)cfg_.decoder_rates.size();
    auto reader = [&](int i) {                         // what reads block i - 1's output: block i's affine and Snake, or snake_out
        Map m{W(dec_snake_[i].a), W(dec_snake_[i].inv), nullptr};
        if (i < nb) m.affine = W(affine_[i]) + (size_t)idx * 2 * (cfg_.decoder_dim >> i);
        return m;
    };
    int C = cfg_.decoder_dim, e = 0;
    long rpf = 1;
    QASR_HIP(hipEventRecord(ev_[e++], work_));
    vae_dw_launch(false, d_z_.as<float>(), frames_, cfg_.latent_dim, 1, fs, 1, W(dec_in_w_), W(dec_in_b_), nullptr, nullptr, nullptr, nullptr, T, work_);
    gemm(dec_in1_, stage == 0 ? E_LIN : E_RESMAP, frames_, 1, 0, T, nullptr, A, reader(0));
    QASR_HIP(hipEventRecord(ev_[e++], work_));
    for (int i = 0; i < nb && stage != i; ++i, C /= 2) {
        gemm(dec_up_[i], E_LIN, frames_ * rpf, (int)rpf, 0, A, nullptr, B, Map{});
        rpf *= cfg_.decoder_rates[i];
        const long rows = frames_ * rpf;
        unit(dec_units_[3 * i], rows, (int)rpf, B, T, A, Map{});
        unit(dec_units_[3 * i + 1], rows, (int)rpf, A, T, B, Map{});
        unit(dec_units_[3 * i + 2], rows, (int)rpf, B, T, A, stage == i + 1 ? Map{} : reader(i + 1));
        QASR_HIP(hipEventRecord(ev_[e++], work_));
    }
    if (stage < 0)
        hipLaunchKernelGGL((vae_out_kernel<false>), dim3((unsigned)cdiv(frames_ * rpf, 256L)), dim3(256), (size_t)9 * C * sizeof(float), work_, A, frames_ * rpf,
                           C, fs, (int)rpf, W(out_w_), W(out_b_), (const float*)nullptr, (const float*)nullptr, d_pcm_.as<float>());
    for (; e <= nb + 2; ++e) QASR_HIP(hipEventRecord(ev_[e], work_));
    QASR_HIP(hipGetLastError());
}

// ---- passes -------------------------------------------------------------------------------------------------------------------------
void AudioVaeVoxcpm::begin_pass(const AvaeClip* c, int n, bool samples) {
    QASR_HIP(hipSetDevice(device_));
    QASR_HIP(hipStreamSynchronize(work_));             // the table is rewritten
    h_fstart_.clear();
    clip_first_.assign(1, 0);
    for (int i = 0; i < n; ++i) {
        const long T = samples ? frames_of(c[i].n) : c[i].n, first = clip_first_.back();
        h_fstart_.insert(h_fstart_.end(), (size_t)T, (int)first);
        clip_first_.push_back(first + T);
    }
    frames_ = clip_first_.back();
    QASR_HIP(hipMemcpy(d_fstart_.p, h_fstart_.data(), h_fstart_.size() * sizeof(int), hipMemcpyHostToDevice));
}

template <class F> void AudioVaeVoxcpm::passes(const std::vector<AvaeClip>& clips, bool samples, F&& run) {
    check_loaded();
    for (float& t : timing_) t = 0.0f;
    auto frames = [&](const AvaeClip& c) { return samples ? frames_of(c.n) : c.n; };
    for (size_t i = 0; i < clips.size(); ++i)
        if (clips[i].n < 1 || frames(clips[i]) > max_frames_)
            throw std::invalid_argument(std::string(WHO) + ": clip " + std::to_string(i) + " holds " + std::to_string(frames(clips[i])) +
                                        " frames, a clip holds 1.." + std::to_string(max_frames_) + " (max_frames)");
    for (size_t i = 0; i < clips.size();) {            // passes end at clip boundaries
        size_t j = i;
        long total = 0;
        while (j < clips.size() && total + frames(clips[j]) <= max_frames_) total += frames(clips[j++]);
        begin_pass(clips.data() + i, (int)(j - i), samples);
        run(clips.data() + i, (int)(j - i));
        i = j;
    }
}

void AudioVaeVoxcpm::encode(const std::vector<AvaeClip>& clips, int stage) {
    const int nb = (int)cfg_.encoder_rates.size(), hop = cfg_.hop();
    if (stage > nb) throw std::invalid_argument(std::string(WHO) + ": encoder stage outside 0.." + std::to_string(nb));
    passes(clips, true, [&](const AvaeClip* c, int n) {
        // preprocess (:636-644): zero samples up to a whole frame are real rows
        QASR_HIP(hipMemsetAsync(d_pcm_.p, 0, (size_t)frames_ * hop * sizeof(float), work_));
        for (int i = 0; i < n; ++i)
            QASR_HIP(hipMemcpyAsync(d_pcm_.as<float>() + clip_first_[i] * hop, c[i].in, (size_t)c[i].n * sizeof(float), hipMemcpyHostToDevice, work_));
        run_encoder(stage);
        int rpf = 1, w = cfg_.latent_dim;
        if (stage >= 0) stage_shape(false, stage, &rpf, &w);
        const float* src = stage < 0 ? d_z_.as<float>() : d_b_[0].as<float>();
        const size_t per = (size_t)rpf * w;
        for (int i = 0; i < n; ++i)
            QASR_HIP(hipMemcpyAsync(c[i].out, src + clip_first_[i] * per, (size_t)(clip_first_[i + 1] - clip_first_[i]) * per * sizeof(float),
                                    hipMemcpyDeviceToHost, work_));
        finish(0, nb + 2);
    });
}

void AudioVaeVoxcpm::decode(const std::vector<AvaeClip>& clips, int sr_cond, int stage) {
    const int nb = (int)cfg_.decoder_rates.size(), L = cfg_.latent_dim;
    if (stage > nb) throw std::invalid_argument(std::string(WHO) + ": decoder stage outside 0.." + std::to_string(nb));
    if (sr_cond == 0) sr_cond = cfg_.out_sample_rate;
    int idx = 0;                                       // getSrIdx (:385-393): how many boundaries sr_cond has reached
    for (int bnd : cfg_.sr_bin_boundaries) idx += sr_cond >= bnd ? 1 : 0;
    passes(clips, false, [&](const AvaeClip* c, int n) {
        for (int i = 0; i < n; ++i)
            QASR_HIP(hipMemcpyAsync(d_z_.as<float>() + clip_first_[i] * L, c[i].in, (size_t)c[i].n * L * sizeof(float), hipMemcpyHostToDevice, work_));
        run_decoder(idx, stage);
        int rpf = cfg_.samples_per_frame(), w = 1;
        if (stage >= 0) stage_shape(true, stage, &rpf, &w);
        const float* src = stage < 0 ? d_pcm_.as<float>() : d_b_[0].as<float>();
        const size_t per = (size_t)rpf * w;
        for (int i = 0; i < n; ++i)
            QASR_HIP(hipMemcpyAsync(c[i].out, src + clip_first_[i] * per, (size_t)c[i].n * per * sizeof(float), hipMemcpyDeviceToHost, work_));
        finish(AV_MAX_RATES + 2, nb + 2);
    });
}

void AudioVaeVoxcpm::output(const std::vector<AvaeClip>& clips) {
    const int nb = (int)cfg_.decoder_rates.size(), C = cfg_.decoder_dim >> nb, spf = cfg_.samples_per_frame();
    passes(clips, false, [&](const AvaeClip* c, int n) {
        float* A = d_b_[0].as<float>();
        const size_t per = (size_t)spf * C;
        for (int i = 0; i < n; ++i)
            QASR_HIP(hipMemcpyAsync(A + clip_first_[i] * per, c[i].in, (size_t)c[i].n * per * sizeof(float), hipMemcpyHostToDevice, work_));
        hipLaunchKernelGGL((vae_out_kernel<true>), dim3((unsigned)cdiv(frames_ * spf, 256L)), dim3(256), (size_t)9 * C * sizeof(float), work_, A, frames_ * spf, C,
                           d_fstart_.as<int>(), spf, W(out_w_), W(out_b_), W(dec_snake_[nb].a), W(dec_snake_[nb].inv), d_pcm_.as<float>());
        QASR_HIP(hipGetLastError());
        for (int i = 0; i < n; ++i)
            QASR_HIP(hipMemcpyAsync(c[i].out, d_pcm_.as<float>() + clip_first_[i] * spf, (size_t)c[i].n * spf * sizeof(float), hipMemcpyDeviceToHost, work_));
        QASR_HIP(hipStreamSynchronize(work_));
    });
}

}  // namespace qasr
