// codec_shared.cpp -- the host half of codec_shared.h: geometry, checkpoint keys and weight packing of the Qwen3-TTS speech tokenizer,
// the same for its decoder and its encoder.
#include "codec_shared.h"
#include <algorithm>
#include <cmath>

namespace qasr {

void codec_check_geometry(const CodecGeom& g, const char* who) {
    auto bad = [who](const std::string& m) { throw std::invalid_argument(std::string(who) + ": " + m); };
    if (g.head_dim != 64) bad("head_dim must be 64");
    if (g.heads < 1 || g.heads > 64) bad("num_heads in 1..64");
    if (g.layers < 1 || g.layers > 64) bad("num_layers in 1..64");
    if (g.hidden < 1 || g.hidden > 4096 || g.latent < 1 || g.latent > 4096) bad("hidden_size and latent_dim in 1..4096");
    if (g.decoder_dim < 16 || g.decoder_dim > 8192 || g.decoder_dim % 16) bad("decoder_dim a multiple of 16 in 16..8192");
    for (int r : g.rates) if (r < 1 || r > 16) bad("four upsample_rates in 1..16");
    for (int r : g.ratios) if (r < 1 || r > 16) bad("two upsampling_ratios in 1..16");
    if (g.quantizers < 2 || g.quantizers > 64) bad("num_quantizers in 2..64");
    if (g.semantic_size < 1 || g.acoustic_size < 1 || g.semantic_size > (1 << 20) || g.acoustic_size > (1 << 20)) bad("codebook sizes in 1..2^20");
    if (g.codebook_dim < 1 || g.codebook_dim > 4096) bad("codebook_dim in 1..4096");
    if (((long)g.semantic_size * g.codebook_dim) % 4 || ((long)g.acoustic_size * g.codebook_dim) % 4) bad("codebook size x codebook_dim a multiple of 4");
    if (!(g.eps > 0.0f)) bad("rms_norm_eps > 0");
    // every output buffer of the C ABI is [1920 T] (qasr_codec_samples_per_frame, SpeechTokenizerDecoder.swift:698 fixes it too)
    if (g.samples_per_frame() != CODEC_SAMPLES_PER_FRAME)
        bad("upsampling_ratios x upsample_rates multiply to " + std::to_string(g.samples_per_frame()) + " samples per frame, must be 1920");
}

std::string codec_codebook_prefix(const char* side, int q) {
    const std::string p = std::string(side) + ".quantizer.";
    return q == 0 ? p + "rvq_first.vq.layers.0._codebook" : p + "rvq_rest.vq.layers." + std::to_string(q - 1) + "._codebook";
}

std::vector<bool> codec_codebooks_stored(const std::string& model_dir, const char* who, const char* side, int quantizers) {
    std::unique_ptr<SafeTensorsDir> st;
    try { st = std::make_unique<SafeTensorsDir>(model_dir, "model.safetensors"); }
    catch (const std::exception& ex) { throw WeightLoadError(QASR_ERR_IO, std::string(who) + ": " + ex.what()); }
    std::vector<bool> embed_stored;
    for (int q = 0; q < quantizers; ++q) {
        const std::string p = codec_codebook_prefix(side, q);
        const bool e = st->entries.count(p + ".embed") > 0;
        if (!e && !st->entries.count(p + ".embedding_sum") && !st->entries.count(p + ".cluster_usage"))
            throw WeightLoadError(QASR_ERR_IO, std::string(who) + ": missing tensor " + p + ".embed");
        embed_stored.push_back(e);
    }
    return embed_stored;
}

void codec_pre_transformer_shapes(CodecShapes& s, const std::string& P, const CodecGeom& g) {
    auto add = [&](const std::string& k, std::vector<int64_t> sh) { s.emplace_back(k, std::move(sh)); };
    const int64_t L = g.latent, H = g.hidden, A = (int64_t)g.heads * g.head_dim;
    add(P + "input_proj.weight", {H, L}); add(P + "input_proj.bias", {H});
    add(P + "output_proj.weight", {L, H}); add(P + "output_proj.bias", {L});
    add(P + "norm.weight", {H});
    for (int l = 0; l < g.layers; ++l) {
        const std::string p = P + "layers." + std::to_string(l) + ".";
        for (const char* k : {"q_proj", "k_proj", "v_proj"}) add(p + "self_attn." + k + ".weight", {A, H});
        add(p + "self_attn.o_proj.weight", {H, A});
        add(p + "input_layernorm.weight", {H}); add(p + "post_attention_layernorm.weight", {H});
        add(p + "mlp.gate_proj.weight", {2 * H, H}); add(p + "mlp.up_proj.weight", {2 * H, H}); add(p + "mlp.down_proj.weight", {H, 2 * H});
        add(p + "self_attn_layer_scale.scale", {H}); add(p + "mlp_layer_scale.scale", {H});
    }
}

CodecGemm codec_pack_conv(Builder& b, const std::string& key, int Cout, int Cin, int k, bool bias) {
    CodecGemm gm; gm.K = k * Cin; gm.N = Cout; gm.Cin = Cin; gm.taps = k;
    const auto& W = b.t(key + ".weight");
    gm.wt = b.take((size_t)gm.K * gm.N);
    for (int n = 0; n < Cout; ++n)
        for (int c = 0; c < Cin; ++c)
            for (int j = 0; j < k; ++j) b.h[gm.wt + ((size_t)j * Cin + c) * Cout + n] = W[((size_t)n * Cin + c) * k + j];
    gm.has_bias = bias;
    if (bias) gm.bias = b.vec(key + ".bias");
    return gm;
}

size_t codec_pack_taps7(Builder& b, const std::string& key, int C) {
    const auto& W = b.t(key);
    const size_t at = b.take((size_t)7 * C);
    for (int c = 0; c < C; ++c)
        for (int j = 0; j < 7; ++j) b.h[at + (size_t)j * C + c] = W[(size_t)c * 7 + j];
    return at;
}

CodecSnake codec_pack_snake(Builder& b, const std::string& key) {
    CodecSnake s;
    const auto &al = b.t(key + ".alpha"), &be = b.t(key + ".beta");
    s.a = b.take(al.size()); s.b = b.take(be.size());
    for (size_t i = 0; i < al.size(); ++i) { b.h[s.a + i] = expf(al[i]); b.h[s.b + i] = 1.0f / expf(be[i]); }
    return s;
}

void codec_pack_codebook(Builder& b, size_t at, const std::string& prefix, bool embed_stored, int n, int D) {
    if (embed_stored) { std::copy(b.t(prefix + ".embed").begin(), b.t(prefix + ".embed").end(), b.h.begin() + at); return; }
    const auto &sum = b.t(prefix + ".embedding_sum"), &use = b.t(prefix + ".cluster_usage");
    for (int i = 0; i < n; ++i)
        for (int d = 0; d < D; ++d) b.h[at + (size_t)i * D + d] = sum[(size_t)i * D + d] / std::max(use[i], 1e-7f);
}

CodecLayer codec_pack_layer(Builder& b, const std::string& p, int H, int A) {
    const int I = 2 * H;
    CodecLayer ly;
    ly.n1 = b.vec(p + "input_layernorm.weight"); ly.n2 = b.vec(p + "post_attention_layernorm.weight");
    ly.ls1 = b.vec(p + "self_attn_layer_scale.scale"); ly.ls2 = b.vec(p + "mlp_layer_scale.scale");
    ly.qkv.K = H; ly.qkv.N = 3 * A; ly.qkv.Cin = H;
    ly.qkv.wt = b.take((size_t)H * 3 * A);
    int part = 0;
    for (const char* k : {"q_proj", "k_proj", "v_proj"}) {
        const auto& W = b.t(p + "self_attn." + k + ".weight");
        for (int n = 0; n < A; ++n)
            for (int c = 0; c < H; ++c) b.h[ly.qkv.wt + (size_t)c * 3 * A + part * A + n] = W[(size_t)n * H + c];
        ++part;
    }
    ly.o = codec_pack_conv(b, p + "self_attn.o_proj", H, A, 1, false);
    ly.gu.K = H; ly.gu.N = 2 * I; ly.gu.Cin = H;
    ly.gu.wt = b.take((size_t)H * 2 * I);
    const auto &Wg = b.t(p + "mlp.gate_proj.weight"), &Wu = b.t(p + "mlp.up_proj.weight");
    for (int n = 0; n < I; ++n)
        for (int c = 0; c < H; ++c) {
            b.h[ly.gu.wt + (size_t)c * 2 * I + 2 * n] = Wg[(size_t)n * H + c];
            b.h[ly.gu.wt + (size_t)c * 2 * I + 2 * n + 1] = Wu[(size_t)n * H + c];
        }
    ly.down = codec_pack_conv(b, p + "mlp.down_proj", H, I, 1, false);
    return ly;
}

size_t codec_pack_rope(Builder& b, long n) {
    const size_t at = b.take((size_t)n * 32 * 2);
    for (long t = 0; t < n; ++t)
        for (int d = 0; d < 32; ++d) {
            const float inv = (float)pow(10000.0, -(double)d / 32.0), ang = (float)t * inv;
            b.h[at + ((size_t)t * 32 + d) * 2] = (float)cos((double)ang);
            b.h[at + ((size_t)t * 32 + d) * 2 + 1] = (float)sin((double)ang);
        }
    return at;
}

}  // namespace qasr
