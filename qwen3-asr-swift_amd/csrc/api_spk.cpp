// api_spk.cpp -- extern "C" boundary of the WeSpeaker speaker embedding model (include/qasr.h, qasr_spk_*).  Exceptions never cross it.
#include "api_guard.h"
#include "spk_wespeaker.h"
#include <cmath>
#include <memory>
#include <string>

struct qasr_spk {
    std::unique_ptr<qasr::WeSpeaker> impl;
    mutable std::string last_error;
};
static std::string& error_slot(const qasr_spk* s) { return s ? s->last_error : create_error<qasr_spk>(); }

static constexpr size_t SPK_DEFAULT_SAMPLES = (size_t)64 * 10 * qasr::SPK_RATE;

// what embed_batch and fbank ask of their clips: a loaded model, no empty clip, no null clip
static int check_clips(qasr_spk* s, const float* const* pcm, const size_t* n, size_t B) {
    if (!s->impl->loaded()) return fail(s, QASR_ERR_NOT_LOADED, "wespeaker: model unloaded");
    for (size_t b = 0; b < B; ++b) {
        if (n[b] == 0) return fail(s, QASR_ERR_EMPTY_AUDIO, "wespeaker: clip " + std::to_string(b) + " is empty");
        if (!pcm[b]) return fail(s, QASR_ERR_INVALID, "wespeaker: null clip");
    }
    return QASR_OK;
}

extern "C" {

int qasr_spk_create(int device, const char* model_dir, size_t max_batch_samples, qasr_engine* order_with, qasr_spk** out) {
    if (!out) return QASR_ERR_INVALID;
    *out = nullptr;
    if (!model_dir) return fail<qasr_spk>(nullptr, QASR_ERR_INVALID, "wespeaker: model_dir is NULL");
    if (max_batch_samples == 0) max_batch_samples = SPK_DEFAULT_SAMPLES;
    if (max_batch_samples < (size_t)qasr::SPK_WIN || max_batch_samples > ((size_t)1 << 31))
        return fail<qasr_spk>(nullptr, QASR_ERR_INVALID, "wespeaker: max_batch_samples in 400 .. 2^31 (0 = 64 x 10 s)");
    if (order_with && (!order_with->impl || order_with->impl->config().device != device))
        return fail<qasr_spk>(nullptr, QASR_ERR_INVALID, "wespeaker: order_with must be an engine on the same device");
    qasr::CheckedWeights w;
    try { w = qasr::load_checked_f32(model_dir, "wespeaker", qasr::spk_tensor_shapes(), true); }          // all checked before any HIP call
    catch (const qasr::WeightLoadError& ex) { return fail<qasr_spk>(nullptr, ex.code, ex.what()); }
    catch (const std::exception& ex) { return fail<qasr_spk>(nullptr, QASR_ERR_IO, ex.what()); }
    return guarded_create(out, QASR_ERR_INVALID, [&](qasr_spk* s) {
        s->impl = std::make_unique<qasr::WeSpeaker>(device, w, max_batch_samples, order_with ? order_with->impl->stream() : nullptr);
    });
}

void qasr_spk_destroy(qasr_spk* s) { delete s; }
const char* qasr_spk_last_error(const qasr_spk* s) { return error_slot(s).c_str(); }

int qasr_spk_is_loaded(const qasr_spk* s) { return s && s->impl && s->impl->loaded() ? 1 : 0; }

int qasr_spk_unload(qasr_spk* s) {
    if (!s || !s->impl) return QASR_ERR_INVALID;
    return guarded(s, [&] { s->impl->unload(); });
}

size_t qasr_spk_memory_footprint(const qasr_spk* s) { return s && s->impl ? s->impl->footprint() : 0; }
int qasr_spk_embedding_dim(void) { return qasr::SPK_DIM; }
int qasr_spk_input_sample_rate(void) { return qasr::SPK_RATE; }
int qasr_spk_num_frames(size_t n) { return qasr::spk_num_frames(n); }

int qasr_spk_embed_batch(qasr_spk* s, const float* const* pcm, const size_t* n, size_t B, float* out) {
    if (!s || !s->impl) return QASR_ERR_INVALID;
    if (B == 0) return QASR_OK;
    if (!pcm || !n || !out) return fail(s, QASR_ERR_INVALID, "wespeaker: null argument");
    if (int rc = check_clips(s, pcm, n, B)) return rc;
    return guarded(s, [&] { s->impl->embed(pcm, n, B, out); });
}

int qasr_spk_embed(qasr_spk* s, const float* pcm, size_t n, int sample_rate, float* out) {
    if (!s || !s->impl) return QASR_ERR_INVALID;
    if (sample_rate != qasr::SPK_RATE)
        return fail(s, QASR_ERR_UNSUPPORTED, "wespeaker: 16 kHz input only (the reference resamples with AVAudioConverter)");
    if (n == 0) return fail(s, QASR_ERR_EMPTY_AUDIO, "wespeaker: empty audio");
    const float* rows[1] = {pcm};
    return qasr_spk_embed_batch(s, rows, &n, 1, out);
}

int qasr_spk_fbank(qasr_spk* s, const float* const* pcm, const size_t* n, size_t B, float* feats, size_t stride, int32_t* n_frames) {
    if (!s || !s->impl) return QASR_ERR_INVALID;
    if (B == 0) return QASR_OK;
    if (!pcm || !n || !feats) return fail(s, QASR_ERR_INVALID, "wespeaker: null argument");
    if (int rc = check_clips(s, pcm, n, B)) return rc;
    return guarded(s, [&] { s->impl->fbank(pcm, n, B, feats, stride, n_frames); });
}

float qasr_spk_cosine_similarity(const float* a, const float* b, size_t n) {
    if (!a || !b || n == 0) return 0.0f;                   // WeSpeaker.swift cosineSimilarity: f32 sums in index order
    float dot = 0.0f, na = 0.0f, nb = 0.0f;
    for (size_t i = 0; i < n; ++i) {
        dot += a[i] * b[i];
        na += a[i] * a[i];
        nb += b[i] * b[i];
    }
    const float den = std::sqrt(na) * std::sqrt(nb);
    return den > 0.0f ? dot / den : 0.0f;
}

int qasr_spk_timing(const qasr_spk* s, float* ms) {
    if (!s || !s->impl) return QASR_ERR_INVALID;
    if (ms) *ms = s->impl->last_ms();
    return QASR_OK;
}

}  // extern "C"
