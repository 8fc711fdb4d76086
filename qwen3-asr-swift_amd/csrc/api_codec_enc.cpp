// api_codec_enc.cpp -- extern "C" boundary of the Qwen3-TTS speech tokenizer encoder (include/qasr.h, qasr_codec_enc_*).  Exceptions never
// cross it.
#include "api_guard.h"
#include "codec_enc_qwen3tts.h"
#include <memory>

struct qasr_codec_enc {
    std::unique_ptr<qasr::CodecEncQwen3TTS> impl;
    mutable std::string last_error;
};
static std::string& error_slot(const qasr_codec_enc* c) { return c ? c->last_error : create_error<qasr_codec_enc>(); }

using namespace qasr;

static const char* const WHO = "speech tokenizer encoder";

static int ready(qasr_codec_enc* c) {
    if (!c || !c->impl) return QASR_ERR_INVALID;
    if (!c->impl->loaded()) return fail(c, QASR_ERR_NOT_LOADED, std::string(WHO) + ": model unloaded");
    return QASR_OK;
}

// the clips of one call, checked on the host; out[b]: codes [Q][frames] (ENCODE) or rows [frames][width]
static int run_batch(qasr_codec_enc* c, const float* const* pcm, const size_t* n, size_t B, void* const* out, CodecEncQwen3TTS::Mode mode) {
    if (int rc = ready(c)) return rc;
    if (B == 0) return QASR_OK;
    if (!pcm || !n || !out) return fail(c, QASR_ERR_INVALID, std::string(WHO) + ": null argument");
    std::vector<CodecEncClip> clips;
    for (size_t b = 0; b < B; ++b) {
        if (!pcm[b] || !out[b]) return fail(c, QASR_ERR_INVALID, std::string(WHO) + ": null item or output");
        if (n[b] == 0) return fail(c, QASR_ERR_INVALID, std::string(WHO) + ": item " + std::to_string(b) + " holds no sample");
        if (n[b] > (size_t)c->impl->max_samples())
            return fail(c, QASR_ERR_INVALID, std::string(WHO) + ": item " + std::to_string(b) + " holds " + std::to_string(n[b]) +
                                                 " samples, more than max_samples = " + std::to_string(c->impl->max_samples()) +
                                                 " (the encoder attends over the whole clip and is not chunked)");
        clips.push_back({pcm[b], (long)n[b], mode == CodecEncQwen3TTS::ENCODE ? (int32_t*)out[b] : nullptr,
                         mode == CodecEncQwen3TTS::ENCODE ? nullptr : (float*)out[b]});
    }
    return guarded(c, [&] { c->impl->run(clips, mode); });
}

extern "C" {

int qasr_codec_enc_create(int device, const char* model_dir, size_t max_samples, qasr_engine* order_with, qasr_codec_enc** out) {
    if (!out) return QASR_ERR_INVALID;
    *out = nullptr;
    if (!model_dir) return fail<qasr_codec_enc>(nullptr, QASR_ERR_INVALID, std::string(WHO) + ": model_dir is NULL");
    if (max_samples == 0) max_samples = (size_t)CENC_DEFAULT_SAMPLES;
    if (max_samples > (size_t)CENC_MAX_SAMPLES)
        return fail<qasr_codec_enc>(nullptr, QASR_ERR_INVALID, std::string(WHO) + ": max_samples in 1..2^24 (0 = 720000)");
    if (order_with && (!order_with->impl || order_with->impl->config().device != device))
        return fail<qasr_codec_enc>(nullptr, QASR_ERR_INVALID, std::string(WHO) + ": order_with must be an engine on the same device");
    CheckedWeights w;
    CodecGeom g;
    std::vector<bool> embed_stored;
    try {                                              // geometry, every key, shape and dtype before any HIP call
        g = codec_read_geometry(model_dir, WHO);
        try { codec_check_geometry(g, WHO); }
        catch (const std::exception& ex) { throw WeightLoadError(QASR_ERR_INVALID, ex.what()); }
        embed_stored = codec_codebooks_stored(model_dir, WHO, "encoder", g.quantizers);
        w = load_checked_f32(model_dir, WHO, codec_enc_tensor_shapes(g, embed_stored), false);
    } catch (const WeightLoadError& ex) { return fail<qasr_codec_enc>(nullptr, ex.code, ex.what()); }
    catch (const std::exception& ex) { return fail<qasr_codec_enc>(nullptr, QASR_ERR_IO, ex.what()); }
    return guarded_create(out, QASR_ERR_INVALID, [&](qasr_codec_enc* c) {
        c->impl = std::make_unique<CodecEncQwen3TTS>(device, w, g, embed_stored, (long)max_samples,
                                                     order_with ? order_with->impl->stream() : nullptr);
    });
}

void qasr_codec_enc_destroy(qasr_codec_enc* c) { delete c; }
const char* qasr_codec_enc_last_error(const qasr_codec_enc* c) { return error_slot(c).c_str(); }
int qasr_codec_enc_is_loaded(const qasr_codec_enc* c) { return c && c->impl && c->impl->loaded() ? 1 : 0; }
int qasr_codec_enc_unload(qasr_codec_enc* c) {
    if (!c || !c->impl) return QASR_ERR_INVALID;
    return guarded(c, [&] { c->impl->unload(); });
}
size_t qasr_codec_enc_memory_footprint(const qasr_codec_enc* c) { return c && c->impl ? c->impl->footprint() : 0; }
int qasr_codec_enc_num_quantizers(const qasr_codec_enc* c) { return c && c->impl ? c->impl->geom().quantizers : 0; }
int qasr_codec_enc_hidden_size(const qasr_codec_enc* c) { return c && c->impl ? c->impl->geom().hidden : 0; }
int qasr_codec_enc_latent_dim(const qasr_codec_enc* c) { return c && c->impl ? c->impl->geom().latent : 0; }
int qasr_codec_enc_timing(const qasr_codec_enc* c, float* ms) {
    if (!c || !c->impl) return QASR_ERR_INVALID;
    if (ms) std::memcpy(ms, c->impl->timing(), CENC_STAGES * sizeof(float));
    return QASR_OK;
}

size_t qasr_codec_enc_num_frames(size_t n) { return (n + CODEC_SAMPLES_PER_FRAME - 1) / CODEC_SAMPLES_PER_FRAME; }

int qasr_codec_enc_encode_batch(qasr_codec_enc* c, const float* const* pcm, const size_t* n, size_t B, int32_t* const* codes) {
    return run_batch(c, pcm, n, B, (void* const*)codes, CodecEncQwen3TTS::ENCODE);
}

int qasr_codec_enc_encode(qasr_codec_enc* c, const float* pcm, size_t n, int32_t* codes) {
    return qasr_codec_enc_encode_batch(c, &pcm, &n, 1, &codes);
}

int qasr_codec_enc_conv_batch(qasr_codec_enc* c, const float* const* pcm, const size_t* n, size_t B, float* const* out) {
    return run_batch(c, pcm, n, B, (void* const*)out, CodecEncQwen3TTS::CONV);
}

int qasr_codec_enc_conv(qasr_codec_enc* c, const float* pcm, size_t n, float* out) { return qasr_codec_enc_conv_batch(c, &pcm, &n, 1, &out); }

int qasr_codec_enc_latent_batch(qasr_codec_enc* c, const float* const* pcm, const size_t* n, size_t B, float* const* out) {
    return run_batch(c, pcm, n, B, (void* const*)out, CodecEncQwen3TTS::LATENT);
}

int qasr_codec_enc_latent(qasr_codec_enc* c, const float* pcm, size_t n, float* out) { return qasr_codec_enc_latent_batch(c, &pcm, &n, 1, &out); }

int qasr_codec_enc_quantize(qasr_codec_enc* c, const float* h, size_t F, int32_t* codes) {
    if (int rc = ready(c)) return rc;
    if (!h || !codes) return fail(c, QASR_ERR_INVALID, std::string(WHO) + ": null argument");
    if (F == 0 || F > ((size_t)1 << 24)) return fail(c, QASR_ERR_INVALID, std::string(WHO) + ": quantize takes 1..2^24 frames");
    return guarded(c, [&] { c->impl->quantize(h, (long)F, codes); });
}

}  // extern "C"
