// api_vad.cpp -- extern "C" boundary of the Silero VAD (include/qasr.h, qasr_vad_*).  Exceptions never cross it.
#include "api_guard.h"
#include "vad_silero.h"
#include <cstring>
#include <memory>
#include <string>
#include <vector>

struct qasr_vad_vt_ctx;
struct qasr_vad {
    std::unique_ptr<qasr::SileroVad> impl;
    mutable std::string last_error;
    std::vector<std::unique_ptr<qasr_vad_vt_ctx>> vt;       // one vtable context per stream, made on demand
};
struct qasr_vad_vt_ctx {
    qasr_vad* v;
    int stream;
};

static std::string& error_slot(const qasr_vad* v) { return v ? v->last_error : create_error<qasr_vad>(); }

static qasr::VadConfig vad_cfg(const qasr_vad_config* c) {
    qasr_vad_config d;
    qasr_vad_default_config(&d);
    if (!c) c = &d;
    return {c->onset, c->offset, c->min_speech_duration, c->min_silence_duration};
}

static int write_segments(const std::vector<qasr::VadSegment>& s, float* out, size_t cap) {
    for (size_t i = 0; i < s.size() && i < cap; ++i) { out[2 * i] = s[i].start; out[2 * i + 1] = s[i].end; }
    return (int)s.size();
}

// vtable callbacks (sc_vad_vtable_t): a failed call answers 0 and leaves the message in qasr_vad_last_error, as the reference's CoreML
// path answers `(try? ...) ?? 0.0` (SileroVAD.swift processChunk)
static float vt_process_chunk(void* ctx, const float* samples, size_t length) {
    auto* c = static_cast<qasr_vad_vt_ctx*>(ctx);
    if (length != (size_t)qasr::VAD_CHUNK || !samples) {
        c->v->last_error = "silero vad: process_chunk needs exactly 512 samples";
        return 0.0f;
    }
    const int32_t sid = c->stream;
    float p = 0.0f;
    return qasr_vad_process(c->v, samples, &sid, 1, &p) == QASR_OK ? p : 0.0f;
}
static void vt_reset(void* ctx) {
    auto* c = static_cast<qasr_vad_vt_ctx*>(ctx);
    (void)qasr_vad_reset(c->v, c->stream);
}
static int32_t vt_rate(void*) { return qasr::VAD_RATE; }
static size_t vt_chunk(void*) { return (size_t)qasr::VAD_CHUNK; }

extern "C" {

int qasr_vad_default_config(qasr_vad_config* out) {
    if (!out) return QASR_ERR_INVALID;
    out->onset = 0.5f; out->offset = 0.35f; out->min_speech_duration = 0.25f; out->min_silence_duration = 0.1f;
    return QASR_OK;
}

int qasr_vad_create(int device, const char* model_dir, int max_streams, qasr_engine* order_with, qasr_vad** out) {
    if (!out) return QASR_ERR_INVALID;
    *out = nullptr;
    if (!model_dir) return fail<qasr_vad>(nullptr, QASR_ERR_INVALID, "silero vad: model_dir is NULL");
    if (max_streams <= 0 || max_streams > 4096) return fail<qasr_vad>(nullptr, QASR_ERR_INVALID, "silero vad: max_streams in 1..4096");
    if (order_with && (!order_with->impl || order_with->impl->config().device != device))
        return fail<qasr_vad>(nullptr, QASR_ERR_INVALID, "silero vad: order_with must be an engine on the same device");
    qasr::CheckedWeights w;
    try { w = qasr::load_checked_f32(model_dir, "silero vad", qasr::silero_tensor_shapes(), false); }     // all checked before any HIP call
    catch (const qasr::WeightLoadError& ex) { return fail<qasr_vad>(nullptr, ex.code, ex.what()); }
    catch (const std::exception& ex) { return fail<qasr_vad>(nullptr, QASR_ERR_IO, ex.what()); }
    return guarded_create(out, QASR_ERR_INVALID, [&](qasr_vad* v) {
        v->impl = std::make_unique<qasr::SileroVad>(device, w, max_streams, order_with ? order_with->impl->stream() : nullptr);
    });
}

void qasr_vad_destroy(qasr_vad* v) { delete v; }
const char* qasr_vad_last_error(const qasr_vad* v) { return error_slot(v).c_str(); }

int qasr_vad_reset(qasr_vad* v, int stream) {
    if (!v || !v->impl) return QASR_ERR_INVALID;
    return guarded(v, [&] { v->impl->reset(stream); });
}

int qasr_vad_process(qasr_vad* v, const float* chunks, const int32_t* stream_ids, size_t B, float* probs) {
    if (!v || !v->impl) return QASR_ERR_INVALID;
    if (B == 0) return QASR_OK;
    if (!chunks || !probs) return fail(v, QASR_ERR_INVALID, "silero vad: null argument");
    return guarded(v, [&] { v->impl->process(chunks, stream_ids, B, probs); });
}

int qasr_vad_probs(qasr_vad* v, const float* const* pcm, const size_t* n, size_t B, const int32_t* stream_ids, float* probs, size_t stride,
                   int32_t* n_chunks) {
    if (!v || !v->impl) return QASR_ERR_INVALID;
    if (B == 0) return QASR_OK;
    if (!pcm || !n || !probs) return fail(v, QASR_ERR_INVALID, "silero vad: null argument");
    return guarded(v, [&] { v->impl->probs(pcm, n, B, stream_ids, probs, stride, n_chunks); });
}

int qasr_vad_binarize(const float* probs, size_t n, const qasr_vad_config* cfg, float* segments, size_t cap) {
    if ((!probs && n) || (!segments && cap)) return -QASR_ERR_INVALID;
    return write_segments(qasr::silero_binarize(probs, n, vad_cfg(cfg)), segments, cap);
}

int qasr_vad_detect_speech(qasr_vad* v, const float* pcm, size_t n, int sample_rate, const qasr_vad_config* cfg, float* segments, size_t cap) {
    if (!v || !v->impl) return -QASR_ERR_INVALID;
    if (sample_rate != qasr::VAD_RATE) {
        fail(v, QASR_ERR_UNSUPPORTED, "silero vad: 16 kHz input only (the reference resamples with AVAudioConverter)");
        return -QASR_ERR_UNSUPPORTED;
    }
    if ((!pcm && n) || (!segments && cap)) return -fail(v, QASR_ERR_INVALID, "silero vad: null argument");
    const size_t nc = (n + qasr::VAD_CHUNK - 1) / qasr::VAD_CHUNK;
    std::vector<float> p(nc ? nc : 1);
    const float* rows[1] = {pcm};
    const int32_t sid = 0;
    if (n) {
        const int st = qasr_vad_probs(v, rows, &n, 1, &sid, p.data(), nc, nullptr);
        if (st != QASR_OK) return -st;
    } else {
        const int st = qasr_vad_reset(v, 0);                           // detectSpeech resets first, then finds no chunk
        if (st != QASR_OK) return -st;
    }
    return write_segments(qasr::silero_binarize(p.data(), nc, vad_cfg(cfg)), segments, cap);
}

int qasr_vad_vtable(qasr_vad* v, int stream, sc_vad_vtable_t* out) {
    if (!v || !v->impl || !out) return QASR_ERR_INVALID;
    if (stream < 0 || stream >= v->impl->max_streams()) return fail(v, QASR_ERR_INVALID, "silero vad: stream outside [0, max_streams)");
    qasr_vad_vt_ctx* c = nullptr;
    for (auto& p : v->vt) if (p->stream == stream) c = p.get();
    if (!c) { v->vt.push_back(std::make_unique<qasr_vad_vt_ctx>(qasr_vad_vt_ctx{v, stream})); c = v->vt.back().get(); }
    out->context = c;
    out->process_chunk = vt_process_chunk;
    out->reset = vt_reset;
    out->input_sample_rate = vt_rate;
    out->chunk_size = vt_chunk;
    return QASR_OK;
}

int qasr_vad_timing(const qasr_vad* v, float* ms, int* was_graph) {
    if (!v || !v->impl) return QASR_ERR_INVALID;
    if (ms) *ms = v->impl->last_ms();
    if (was_graph) *was_graph = v->impl->last_was_graph() ? 1 : 0;
    return QASR_OK;
}

int qasr_vad_state(qasr_vad* v, int stream, float* h, float* c, float* context) {
    if (!v || !v->impl) return QASR_ERR_INVALID;
    return guarded(v, [&] { v->impl->state(stream, h, c, context); });
}

}  // extern "C"
