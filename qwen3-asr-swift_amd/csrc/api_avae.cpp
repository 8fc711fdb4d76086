// api_avae.cpp -- extern "C" boundary of the VoxCPM2 AudioVAE (include/qasr.h, qasr_avae_*).  Exceptions never cross it.
#include "api_guard.h"
#include "vae_voxcpm.h"
#include <memory>

struct qasr_avae {
    std::unique_ptr<qasr::AudioVaeVoxcpm> impl;
    mutable std::string last_error;
};
static std::string& error_slot(const qasr_avae* h) { return h ? h->last_error : create_error<qasr_avae>(); }

using namespace qasr;

static const char* const WHO = "AudioVAE";

// NOT_LOADED comes before every other refusal
static int ready(qasr_avae* h) {
    if (!h || !h->impl) return QASR_ERR_INVALID;
    if (!h->impl->loaded()) return fail(h, QASR_ERR_NOT_LOADED, std::string(WHO) + ": model unloaded");
    return QASR_OK;
}

static int null_argument(qasr_avae* h) { return fail(h, QASR_ERR_INVALID, std::string(WHO) + ": null argument"); }

// B clips of a batch entry -> AvaeClip, with the checks both directions share; n[b] counts samples (encode) or frames (decode)
static int clips_of(qasr_avae* h, const float* const* in, const size_t* n, size_t B, float* const* out, bool samples, std::vector<AvaeClip>& c) {
    if (!in || !n || !out) return null_argument(h);
    for (size_t b = 0; b < B; ++b) {
        if (!in[b] || !out[b]) return null_argument(h);
        const char* unit = samples ? " samples" : " frames";
        if (n[b] == 0) return fail(h, QASR_ERR_INVALID, std::string(WHO) + ": clip " + std::to_string(b) + " has no" + unit);
        const size_t cap = (size_t)h->impl->max_frames() * (samples ? (size_t)h->impl->config().hop() : 1);
        if (n[b] > cap)
            return fail(h, QASR_ERR_INVALID, std::string(WHO) + ": clip " + std::to_string(b) + " holds " + std::to_string(n[b]) + unit +
                                                 ", more than max_frames = " + std::to_string(h->impl->max_frames()) + " allows");
        c.push_back({in[b], (long)n[b], out[b]});
    }
    return QASR_OK;
}

extern "C" {

int qasr_avae_create(int device, const char* model_dir, size_t max_frames, qasr_engine* order_with, qasr_avae** out) {
    if (!out) return QASR_ERR_INVALID;
    *out = nullptr;
    if (!model_dir) return fail<qasr_avae>(nullptr, QASR_ERR_INVALID, std::string(WHO) + ": model_dir is NULL");
    if (max_frames == 0) max_frames = (size_t)AV_DEFAULT_FRAMES;
    if (max_frames > (size_t)AV_MAX_FRAMES)
        return fail<qasr_avae>(nullptr, QASR_ERR_INVALID, std::string(WHO) + ": max_frames in 1..2^14 (0 = 1024)");
    if (order_with && (!order_with->impl || order_with->impl->config().device != device))
        return fail<qasr_avae>(nullptr, QASR_ERR_INVALID, std::string(WHO) + ": order_with must be an engine on the same device");
    AvaeConfig cfg;
    CheckedWeights w;
    try {                                              // the configuration, then every key, shape and dtype, before any HIP call
        cfg = avae_read_config(model_dir, WHO);
        w = avae_load_weights(model_dir, WHO, cfg);
    } catch (const WeightLoadError& ex) { return fail<qasr_avae>(nullptr, ex.code, ex.what()); }
    catch (const std::invalid_argument& ex) { return fail<qasr_avae>(nullptr, QASR_ERR_INVALID, ex.what()); }
    catch (const std::exception& ex) { return fail<qasr_avae>(nullptr, QASR_ERR_IO, ex.what()); }
    return guarded_create(out, QASR_ERR_INVALID, [&](qasr_avae* h) {
        h->impl = std::make_unique<AudioVaeVoxcpm>(device, cfg, w, (long)max_frames, order_with ? order_with->impl->stream() : nullptr);
    });
}

void qasr_avae_destroy(qasr_avae* h) { delete h; }
const char* qasr_avae_last_error(const qasr_avae* h) { return error_slot(h).c_str(); }
int qasr_avae_is_loaded(const qasr_avae* h) { return h && h->impl && h->impl->loaded() ? 1 : 0; }
int qasr_avae_unload(qasr_avae* h) {
    if (!h || !h->impl) return QASR_ERR_INVALID;
    return guarded(h, [&] { h->impl->unload(); });
}
size_t qasr_avae_memory_footprint(const qasr_avae* h) { return h && h->impl ? h->impl->footprint() : 0; }
int qasr_avae_latent_dim(const qasr_avae* h) { return h && h->impl ? h->impl->config().latent_dim : 0; }
int qasr_avae_in_sample_rate(const qasr_avae* h) { return h && h->impl ? h->impl->config().sample_rate : 0; }
int qasr_avae_out_sample_rate(const qasr_avae* h) { return h && h->impl ? h->impl->config().out_sample_rate : 0; }
int qasr_avae_hop(const qasr_avae* h) { return h && h->impl ? h->impl->config().hop() : 0; }
int qasr_avae_samples_per_frame(const qasr_avae* h) { return h && h->impl ? h->impl->config().samples_per_frame() : 0; }
size_t qasr_avae_num_frames(const qasr_avae* h, size_t n) { return h && h->impl ? (size_t)h->impl->frames_of((long)n) : (n + 639) / 640; }
int qasr_avae_num_blocks(const qasr_avae* h, int decoder) {
    if (!h || !h->impl) return 0;
    return (int)(decoder ? h->impl->config().decoder_rates.size() : h->impl->config().encoder_rates.size());
}
int qasr_avae_stage_shape(const qasr_avae* h, int decoder, int k, int* rows_per_frame, int* width) {
    if (!h || !h->impl || !rows_per_frame || !width) return QASR_ERR_INVALID;
    return h->impl->stage_shape(decoder != 0, k, rows_per_frame, width) ? QASR_OK : QASR_ERR_INVALID;
}

int qasr_avae_encode_batch(qasr_avae* h, const float* const* pcm, const size_t* n, size_t B, float* const* z) {
    if (const int rc = ready(h)) return rc;
    if (B == 0) return QASR_OK;
    std::vector<AvaeClip> c;
    if (const int rc = clips_of(h, pcm, n, B, z, true, c)) return rc;
    return guarded(h, [&] { h->impl->encode(c, -1); });
}

int qasr_avae_encode(qasr_avae* h, const float* pcm, size_t n, float* z) { return qasr_avae_encode_batch(h, &pcm, &n, 1, &z); }

int qasr_avae_decode_batch(qasr_avae* h, const float* const* z, const size_t* T, size_t B, int sr_cond, float* const* pcm) {
    if (const int rc = ready(h)) return rc;
    if (sr_cond < 0) return fail(h, QASR_ERR_INVALID, std::string(WHO) + ": sr_cond is negative");
    if (B == 0) return QASR_OK;
    std::vector<AvaeClip> c;
    if (const int rc = clips_of(h, z, T, B, pcm, false, c)) return rc;
    return guarded(h, [&] { h->impl->decode(c, sr_cond, -1); });
}

int qasr_avae_decode(qasr_avae* h, const float* z, size_t T, int sr_cond, float* pcm) { return qasr_avae_decode_batch(h, &z, &T, 1, sr_cond, &pcm); }

int qasr_avae_enc_stage(qasr_avae* h, const float* pcm, size_t n, int k, float* out) {
    if (const int rc = ready(h)) return rc;
    if (k < 0) return fail(h, QASR_ERR_INVALID, std::string(WHO) + ": stage is negative");
    std::vector<AvaeClip> c;
    if (const int rc = clips_of(h, &pcm, &n, 1, &out, true, c)) return rc;
    return guarded(h, [&] { h->impl->encode(c, k); });
}

int qasr_avae_dec_stage(qasr_avae* h, const float* z, size_t T, int sr_cond, int k, float* out) {
    if (const int rc = ready(h)) return rc;
    if (k < 0 || sr_cond < 0) return fail(h, QASR_ERR_INVALID, std::string(WHO) + ": stage or sr_cond is negative");
    std::vector<AvaeClip> c;
    if (const int rc = clips_of(h, &z, &T, 1, &out, false, c)) return rc;
    return guarded(h, [&] { h->impl->decode(c, sr_cond, k); });
}

int qasr_avae_dec_output(qasr_avae* h, const float* rows, size_t T, float* pcm) {
    if (const int rc = ready(h)) return rc;
    std::vector<AvaeClip> c;
    if (const int rc = clips_of(h, &rows, &T, 1, &pcm, false, c)) return rc;
    return guarded(h, [&] { h->impl->output(c); });
}

int qasr_avae_timing(const qasr_avae* h, float* ms) {
    if (!h || !h->impl) return QASR_ERR_INVALID;
    if (ms) std::memcpy(ms, h->impl->timing(), AV_STAGES * sizeof(float));
    return QASR_OK;
}

}  // extern "C"
