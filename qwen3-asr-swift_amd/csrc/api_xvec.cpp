// api_xvec.cpp -- extern "C" boundary of the Qwen3-TTS speaker encoder (include/qasr.h, qasr_xvec_*).  Exceptions never cross it.
#include "api_guard.h"
#include "xvec_qwen3tts.h"
#include <memory>

struct qasr_xvec {
    std::unique_ptr<qasr::XvecQwen3TTS> impl;
    mutable std::string last_error;
};
static std::string& error_slot(const qasr_xvec* x) { return x ? x->last_error : create_error<qasr_xvec>(); }

using namespace qasr;

static const char* const WHO = "speaker encoder";

// the clips of one call, checked on the host
static int run_batch(qasr_xvec* x, const float* const* pcm, const size_t* n, size_t B, float* const* mel, float* out) {
    if (!x || !x->impl) return QASR_ERR_INVALID;
    if (!x->impl->loaded()) return fail(x, QASR_ERR_NOT_LOADED, std::string(WHO) + ": model unloaded");
    if (B == 0) return QASR_OK;
    if (!pcm || !n || (!mel && !out)) return fail(x, QASR_ERR_INVALID, std::string(WHO) + ": null argument");
    std::vector<XvecClip> clips;
    for (size_t b = 0; b < B; ++b) {
        if (n[b] == 0) return fail(x, QASR_ERR_EMPTY_AUDIO, std::string(WHO) + ": clip " + std::to_string(b) + " is empty");
        if (!pcm[b] || (mel && !mel[b])) return fail(x, QASR_ERR_INVALID, std::string(WHO) + ": null clip or output");
        if (n[b] > (size_t)x->impl->max_samples())
            return fail(x, QASR_ERR_CAPACITY, std::string(WHO) + ": clip " + std::to_string(b) + " holds " + std::to_string(n[b]) +
                                                  " samples, more than max_samples = " + std::to_string(x->impl->max_samples()));
        clips.push_back({pcm[b], (long)n[b], mel ? mel[b] : nullptr, out ? out + b * (size_t)x->impl->embedding_dim() : nullptr});
    }
    return guarded(x, [&] { x->impl->run(clips, mel ? XvecQwen3TTS::MEL : XvecQwen3TTS::EMBED); });
}

extern "C" {

int qasr_xvec_create(int device, const char* model_dir, size_t max_samples, qasr_engine* order_with, qasr_xvec** out) {
    if (!out) return QASR_ERR_INVALID;
    *out = nullptr;
    if (!model_dir) return fail<qasr_xvec>(nullptr, QASR_ERR_INVALID, std::string(WHO) + ": model_dir is NULL");
    if (max_samples == 0) max_samples = (size_t)XV_DEFAULT_SAMPLES;
    if (max_samples > (size_t)XV_MAX_SAMPLES)
        return fail<qasr_xvec>(nullptr, QASR_ERR_INVALID, std::string(WHO) + ": max_samples in 1..2^28 (0 = 64 x 10 s)");
    if (order_with && (!order_with->impl || order_with->impl->config().device != device))
        return fail<qasr_xvec>(nullptr, QASR_ERR_INVALID, std::string(WHO) + ": order_with must be an engine on the same device");
    CheckedWeights w;
    int64_t E = 0;
    try {                                              // every key, shape and dtype before any HIP call
        std::unique_ptr<SafeTensorsDir> st;            // all *.safetensors of the directory (TTSWeightLoading.swift:389); other keys are not read
        try { st = std::make_unique<SafeTensorsDir>(model_dir); }
        catch (const std::exception& ex) { throw WeightLoadError(QASR_ERR_IO, std::string(WHO) + ": " + ex.what()); }
        const std::string fcw = "speaker_encoder.fc.weight";
        auto it = st->entries.find(fcw);
        if (it == st->entries.end()) {
            bool any = false;
            for (const auto& kv : st->entries) any = any || kv.first.compare(0, 16, "speaker_encoder.") == 0;
            throw WeightLoadError(QASR_ERR_IO, std::string(WHO) + (any ? ": missing tensor " + fcw
                                                                       : ": no speaker_encoder. tensor in " + std::string(model_dir) +
                                                                             " (missing tensor " + fcw + ")"));
        }
        if (it->second.shape.size() != 3 || it->second.shape[0] < 1 || it->second.shape[0] > 65536)
            throw WeightLoadError(QASR_ERR_INVALID, std::string(WHO) + ": tensor " + fcw + " is not [E][1][3072] with E in 1..65536");
        E = it->second.shape[0];                       // the embedding width is the checkpoint's (1024; 2048 in the 1.7B Base model)
        w = load_checked_f32(*st, WHO, xvec_tensor_shapes(E), false);
    } catch (const WeightLoadError& ex) { return fail<qasr_xvec>(nullptr, ex.code, ex.what()); }
    catch (const std::exception& ex) { return fail<qasr_xvec>(nullptr, QASR_ERR_IO, ex.what()); }
    return guarded_create(out, QASR_ERR_INVALID, [&](qasr_xvec* x) {
        x->impl = std::make_unique<XvecQwen3TTS>(device, w, (int)E, (long)max_samples, order_with ? order_with->impl->stream() : nullptr);
    });
}

void qasr_xvec_destroy(qasr_xvec* x) { delete x; }
const char* qasr_xvec_last_error(const qasr_xvec* x) { return error_slot(x).c_str(); }
int qasr_xvec_is_loaded(const qasr_xvec* x) { return x && x->impl && x->impl->loaded() ? 1 : 0; }
int qasr_xvec_unload(qasr_xvec* x) {
    if (!x || !x->impl) return QASR_ERR_INVALID;
    return guarded(x, [&] { x->impl->unload(); });
}
size_t qasr_xvec_memory_footprint(const qasr_xvec* x) { return x && x->impl ? x->impl->footprint() : 0; }
int qasr_xvec_embedding_dim(const qasr_xvec* x) { return x && x->impl ? x->impl->embedding_dim() : 0; }
int qasr_xvec_input_sample_rate(void) { return XV_RATE; }
size_t qasr_xvec_num_frames(size_t n) { return (size_t)xvec_num_frames((long)n); }

int qasr_xvec_embed_batch(qasr_xvec* x, const float* const* pcm, const size_t* n, size_t B, float* out) {
    return run_batch(x, pcm, n, B, nullptr, out);
}

int qasr_xvec_embed(qasr_xvec* x, const float* pcm, size_t n, int sample_rate, float* out) {
    if (!x || !x->impl) return QASR_ERR_INVALID;
    if (!x->impl->loaded()) return fail(x, QASR_ERR_NOT_LOADED, std::string(WHO) + ": model unloaded");
    if (sample_rate != XV_RATE)
        return fail(x, QASR_ERR_UNSUPPORTED, std::string(WHO) + ": 24 kHz input only (the reference resamples with AVAudioConverter)");
    const float* rows[1] = {pcm};
    return run_batch(x, rows, &n, 1, nullptr, out);
}

int qasr_xvec_mel(qasr_xvec* x, const float* const* pcm, const size_t* n, size_t B, float* const* out) {
    return run_batch(x, pcm, n, B, out, nullptr);
}

int qasr_xvec_embed_mel(qasr_xvec* x, const float* mel, size_t T, float* out) {
    if (!x || !x->impl) return QASR_ERR_INVALID;
    if (!x->impl->loaded()) return fail(x, QASR_ERR_NOT_LOADED, std::string(WHO) + ": model unloaded");
    if (!mel || !out) return fail(x, QASR_ERR_INVALID, std::string(WHO) + ": null argument");
    if (T == 0) return fail(x, QASR_ERR_EMPTY_AUDIO, std::string(WHO) + ": no frames");
    if (T > ((size_t)1 << 30)) return fail(x, QASR_ERR_CAPACITY, std::string(WHO) + ": too many frames");
    return guarded(x, [&] { x->impl->embed_mel(mel, (long)T, out); });
}

int qasr_xvec_timing(const qasr_xvec* x, float* ms) {
    if (!x || !x->impl) return QASR_ERR_INVALID;
    if (ms) std::memcpy(ms, x->impl->timing(), XV_STAGES * sizeof(float));
    return QASR_OK;
}

}  // extern "C"
