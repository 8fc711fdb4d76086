// api_codec.cpp -- extern "C" boundary of the Qwen3-TTS speech tokenizer decoder (include/qasr.h, qasr_codec_*).  Exceptions never cross it.
#include "api_guard.h"
#include "codec_qwen3tts.h"
#include "json.h"
#include <fstream>
#include <memory>
#include <sstream>

struct qasr_codec {
    std::unique_ptr<qasr::CodecQwen3TTS> impl;
    mutable std::string last_error;
};
static std::string& error_slot(const qasr_codec* c) { return c ? c->last_error : create_error<qasr_codec>(); }

using namespace qasr;

static const char* const WHO = "speech tokenizer decoder";

// model_dir/config.json's "decoder_config" (or the object itself when it carries the decoder's fields) over the reference's defaults
CodecGeom qasr::codec_read_geometry(const std::string& dir, const char* WHO) {
    CodecGeom g;
    std::ifstream f(dir + "/config.json", std::ios::binary);
    if (!f) return g;
    std::stringstream ss;
    ss << f.rdbuf();
    const std::string text = ss.str();
    Json root;
    try { root = JsonParser(text.data(), text.size()).parse(); }
    catch (const std::exception& ex) { throw WeightLoadError(QASR_ERR_INVALID, std::string(WHO) + ": config.json: " + ex.what()); }
    const Json* d = root.get("decoder_config");
    if (!d && root.get("upsample_rates") && root.get("latent_dim")) d = &root;
    if (!d) return g;
    if (d->type != Json::Obj) throw WeightLoadError(QASR_ERR_INVALID, std::string(WHO) + ": config.json: decoder_config is not an object");
    auto bad = [WHO](const std::string& k) { throw WeightLoadError(QASR_ERR_INVALID, std::string(WHO) + ": config.json: " + k); };
    auto num = [&](const char* k, int* out) {
        const Json* v = d->get(k);
        if (!v) return;
        if (v->type != Json::Num || v->num < 0 || v->num > (1 << 24) || v->num != (double)(int)v->num) bad(std::string(k) + " is not a small integer");
        *out = (int)v->num;
    };
    auto list = [&](const char* k, int* out, size_t n) {
        const Json* v = d->get(k);
        if (!v) return;
        if (v->type != Json::Arr || v->arr.size() != n) bad(std::string(k) + " must hold " + std::to_string(n) + " integers");
        for (size_t i = 0; i < n; ++i) {
            const Json& e = v->arr[i];
            if (e.type != Json::Num || e.num < 1 || e.num > 64 || e.num != (double)(int)e.num) bad(std::string(k) + " must hold " + std::to_string(n) + " integers");
            out[i] = (int)e.num;
        }
    };
    num("latent_dim", &g.latent); num("decoder_dim", &g.decoder_dim); num("hidden_size", &g.hidden);
    num("num_attention_heads", &g.heads); num("num_heads", &g.heads); num("head_dim", &g.head_dim);
    num("num_hidden_layers", &g.layers); num("num_layers", &g.layers); num("num_quantizers", &g.quantizers);
    int cb = -1;
    num("codebook_size", &cb);
    if (cb >= 0) g.semantic_size = g.acoustic_size = cb;
    num("semantic_codebook_size", &g.semantic_size); num("acoustic_codebook_size", &g.acoustic_size); num("codebook_dim", &g.codebook_dim);
    list("upsample_rates", g.rates, 4); list("upsampling_ratios", g.ratios, 2);
    if (const Json* e = d->get("rms_norm_eps")) {
        if (e->type != Json::Num) bad("rms_norm_eps is not a number");
        g.eps = (float)e->num;
    }
    return g;
}

// every code inside its codebook, before anything reaches the device
static int check_codes(qasr_codec* c, const int32_t* codes, size_t T, size_t item) {
    const CodecGeom& g = c->impl->geom();
    for (int q = 0; q < g.quantizers; ++q) {
        const int32_t lim = q == 0 ? g.semantic_size : g.acoustic_size;
        for (size_t t = 0; t < T; ++t) {
            const int32_t v = codes[(size_t)q * T + t];
            if (v < 0 || v >= lim)
                return fail(c, QASR_ERR_INVALID, std::string(WHO) + ": item " + std::to_string(item) + ": code " + std::to_string(v) + " of quantizer " +
                                                     std::to_string(q) + " at frame " + std::to_string(t) + " is outside [0, " + std::to_string(lim) + ")");
        }
    }
    return QASR_OK;
}

static int ready(qasr_codec* c) {
    if (!c || !c->impl) return QASR_ERR_INVALID;
    if (!c->impl->loaded()) return fail(c, QASR_ERR_NOT_LOADED, std::string(WHO) + ": model unloaded");
    return QASR_OK;
}

int qasr::codec_run_windows(qasr_codec* c, const std::vector<CodecWin>& wins, bool clip) {
    if (int rc = ready(c)) return rc;
    for (size_t i = 0; i < wins.size(); ++i) {
        const CodecWin& w = wins[i];
        if (!w.codes || !w.out || w.start != 0 || w.frames < 1 || w.frames > CODEC_MAX_T || w.ld != w.frames || w.context < 0 || w.context >= w.frames)
            return fail(c, QASR_ERR_INVALID, std::string(WHO) + ": window " + std::to_string(i) + " is not 1..35 whole frames with a shorter context");
        if (int rc = check_codes(c, w.codes, (size_t)w.frames, i)) return rc;
    }
    if (wins.empty()) return QASR_OK;
    return guarded(c, [&] { c->impl->run(wins, clip, true); });
}

extern "C" {

int qasr_codec_create(int device, const char* model_dir, int max_windows, qasr_engine* order_with, qasr_codec** out) {
    if (!out) return QASR_ERR_INVALID;
    *out = nullptr;
    if (!model_dir) return fail<qasr_codec>(nullptr, QASR_ERR_INVALID, std::string(WHO) + ": model_dir is NULL");
    if (max_windows == 0) max_windows = 16;
    if (max_windows < 1 || max_windows > 512) return fail<qasr_codec>(nullptr, QASR_ERR_INVALID, std::string(WHO) + ": max_windows in 1..512 (0 = 16)");
    if (order_with && (!order_with->impl || order_with->impl->config().device != device))
        return fail<qasr_codec>(nullptr, QASR_ERR_INVALID, std::string(WHO) + ": order_with must be an engine on the same device");
    CheckedWeights w;
    CodecGeom g;
    std::vector<bool> embed_stored;
    try {                                              // geometry, every key, shape and dtype before any HIP call
        g = codec_read_geometry(model_dir, WHO);
        try { codec_check_geometry(g, WHO); }
        catch (const std::exception& ex) { throw WeightLoadError(QASR_ERR_INVALID, ex.what()); }
        embed_stored = codec_codebooks_stored(model_dir, WHO, "decoder", g.quantizers);
        w = load_checked_f32(model_dir, WHO, codec_tensor_shapes(g, embed_stored), false);
    } catch (const WeightLoadError& ex) { return fail<qasr_codec>(nullptr, ex.code, ex.what()); }
    catch (const std::exception& ex) { return fail<qasr_codec>(nullptr, QASR_ERR_IO, ex.what()); }
    return guarded_create(out, QASR_ERR_INVALID, [&](qasr_codec* c) {
        c->impl = std::make_unique<CodecQwen3TTS>(device, w, g, embed_stored, max_windows, order_with ? order_with->impl->stream() : nullptr);
    });
}

void qasr_codec_destroy(qasr_codec* c) { delete c; }
const char* qasr_codec_last_error(const qasr_codec* c) { return error_slot(c).c_str(); }
int qasr_codec_is_loaded(const qasr_codec* c) { return c && c->impl && c->impl->loaded() ? 1 : 0; }
int qasr_codec_unload(qasr_codec* c) {
    if (!c || !c->impl) return QASR_ERR_INVALID;
    return guarded(c, [&] { c->impl->unload(); });
}
size_t qasr_codec_memory_footprint(const qasr_codec* c) { return c && c->impl ? c->impl->footprint() : 0; }
int qasr_codec_sample_rate(void) { return CODEC_RATE; }
int qasr_codec_samples_per_frame(void) { return CODEC_SAMPLES_PER_FRAME; }
int qasr_codec_num_quantizers(const qasr_codec* c) { return c && c->impl ? c->impl->geom().quantizers : 0; }
int qasr_codec_hidden_size(const qasr_codec* c) { return c && c->impl ? c->impl->geom().hidden : 0; }
int qasr_codec_latent_dim(const qasr_codec* c) { return c && c->impl ? c->impl->geom().latent : 0; }
int qasr_codec_timing(const qasr_codec* c, float* ms) {
    if (!c || !c->impl) return QASR_ERR_INVALID;
    if (ms) std::memcpy(ms, c->impl->timing(), CODEC_STAGES * sizeof(float));
    return QASR_OK;
}

int64_t qasr_codec_window_positions(size_t T, int32_t* starts, int32_t* context, int32_t* ends, size_t cap) {
    if (T == 0 || T > ((size_t)1 << 30)) return -QASR_ERR_INVALID;
    const auto spans = codec_window_positions((long)T);
    if (spans.size() > cap) return -QASR_ERR_CAPACITY;
    for (size_t i = 0; i < spans.size(); ++i) {
        if (starts) starts[i] = spans[i].start;
        if (context) context[i] = spans[i].context;
        if (ends) ends[i] = spans[i].end;
    }
    return (int64_t)spans.size();
}

int qasr_codec_forward(qasr_codec* c, const int32_t* codes, size_t B, size_t T, int clip, float* out) {
    if (int rc = ready(c)) return rc;
    if (!codes || !out) return fail(c, QASR_ERR_INVALID, std::string(WHO) + ": null argument");
    if (B == 0 || B > ((size_t)1 << 20)) return fail(c, QASR_ERR_INVALID, std::string(WHO) + ": 1..2^20 windows");
    if (T == 0 || T > (size_t)CODEC_MAX_T) return fail(c, QASR_ERR_INVALID, std::string(WHO) + ": forward takes 1..35 frames (decode chunks longer inputs)");
    const CodecGeom& g = c->impl->geom();
    const size_t spf = (size_t)g.samples_per_frame();
    std::vector<CodecWin> wins;
    for (size_t b = 0; b < B; ++b) {
        const int32_t* cb = codes + b * g.quantizers * T;
        if (int rc = check_codes(c, cb, T, b)) return rc;
        wins.push_back({cb, (long)T, 0, (int)T, 0, out + b * spf * T});
    }
    return guarded(c, [&] { c->impl->run(wins, clip != 0); });
}

int qasr_codec_forward_tail(qasr_codec* c, const int32_t* codes, size_t B, size_t T, size_t context, int clip, float* out) {
    if (int rc = ready(c)) return rc;
    if (!codes || !out) return fail(c, QASR_ERR_INVALID, std::string(WHO) + ": null argument");
    if (B == 0 || B > ((size_t)1 << 20)) return fail(c, QASR_ERR_INVALID, std::string(WHO) + ": 1..2^20 windows");
    if (T == 0 || T > (size_t)CODEC_MAX_T || context >= T)
        return fail(c, QASR_ERR_INVALID, std::string(WHO) + ": forward_tail takes 1..35 frames and a context shorter than the window");
    const CodecGeom& g = c->impl->geom();
    const size_t kept = (size_t)g.samples_per_frame() * (T - context);
    std::vector<CodecWin> wins;
    for (size_t b = 0; b < B; ++b) wins.push_back({codes + b * g.quantizers * T, (long)T, 0, (int)T, (int)context, out + b * kept});
    return codec_run_windows(c, wins, clip != 0);
}

int qasr_codec_tail_leads(const int32_t upsample_rates[4], int32_t leads[6]) {
    if (!upsample_rates || !leads) return QASR_ERR_INVALID;
    int r[4], l[6];
    for (int i = 0; i < 4; ++i) {
        if (upsample_rates[i] < 1 || upsample_rates[i] > 64) return QASR_ERR_INVALID;
        r[i] = upsample_rates[i];
    }
    codec_tail_leads(r, l);
    for (int i = 0; i < 6; ++i) leads[i] = l[i];
    return QASR_OK;
}

int qasr_codec_decode_batch(qasr_codec* c, const int32_t* const* codes, const size_t* T, size_t B, float* const* out) {
    if (int rc = ready(c)) return rc;
    if (B == 0) return QASR_OK;
    if (!codes || !T || !out) return fail(c, QASR_ERR_INVALID, std::string(WHO) + ": null argument");
    const size_t spf = (size_t)c->impl->geom().samples_per_frame();
    std::vector<CodecWin> wins;
    for (size_t b = 0; b < B; ++b) {
        if (!codes[b] || !out[b]) return fail(c, QASR_ERR_INVALID, std::string(WHO) + ": null item or output");
        if (T[b] == 0 || T[b] > ((size_t)1 << 24)) return fail(c, QASR_ERR_INVALID, std::string(WHO) + ": item " + std::to_string(b) + " holds no frame (or more than 2^24)");
        if (int rc = check_codes(c, codes[b], T[b], b)) return rc;
        for (const CodecSpan& s : codec_window_positions((long)T[b]))
            wins.push_back({codes[b], (long)T[b], s.start, s.end - s.start, s.context, out[b] + (size_t)(s.start + s.context) * spf});
    }
    return guarded(c, [&] { c->impl->run(wins, true); });
}

int qasr_codec_decode(qasr_codec* c, const int32_t* codes, size_t T, float* out) {
    const int32_t* cp[1] = {codes};
    float* op[1] = {out};
    return qasr_codec_decode_batch(c, cp, &T, 1, op);
}

int qasr_codec_quantizer_decode(qasr_codec* c, const int32_t* codes, size_t B, size_t T, float* out) {
    if (int rc = ready(c)) return rc;
    if (!codes || !out) return fail(c, QASR_ERR_INVALID, std::string(WHO) + ": null argument");
    if (B == 0 || B > ((size_t)1 << 20) || T == 0 || T > (size_t)CODEC_MAX_T) return fail(c, QASR_ERR_INVALID, std::string(WHO) + ": 1..2^20 windows of 1..35 frames");
    for (size_t b = 0; b < B; ++b)
        if (int rc = check_codes(c, codes + b * c->impl->geom().quantizers * T, T, b)) return rc;
    return guarded(c, [&] { c->impl->quantizer_decode(codes, (int)B, (int)T, out); });
}

int qasr_codec_pre_transformer(qasr_codec* c, const float* x, size_t B, size_t T, float* out) {
    if (int rc = ready(c)) return rc;
    if (!x || !out) return fail(c, QASR_ERR_INVALID, std::string(WHO) + ": null argument");
    if (B == 0 || B > ((size_t)1 << 20) || T == 0 || T > (size_t)CODEC_MAX_T) return fail(c, QASR_ERR_INVALID, std::string(WHO) + ": 1..2^20 windows of 1..35 frames");
    return guarded(c, [&] { c->impl->pre_transformer(x, (int)B, (int)T, out); });
}

}  // extern "C"
