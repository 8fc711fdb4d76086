// api_voc.cpp -- extern "C" boundary of the CosyVoice3 HiFT vocoder (include/qasr.h, qasr_hift_*).  Exceptions never cross it.
#include "api_guard.h"
#include "voc_cosyvoice.h"
#include <memory>

struct qasr_hift {
    std::unique_ptr<qasr::HiftCosyVoice> impl;
    mutable std::string last_error;
};
static std::string& error_slot(const qasr_hift* h) { return h ? h->last_error : create_error<qasr_hift>(); }

using namespace qasr;

static const char* const WHO = "HiFT vocoder";

// the checks every device entry shares; clips holds B clips with T set
static int run(qasr_hift* h, std::vector<HiftClip>& clips, HiftCosyVoice::Mode mode) {
    for (size_t b = 0; b < clips.size(); ++b) {
        if (clips[b].T == 0) return fail(h, QASR_ERR_INVALID, std::string(WHO) + ": clip " + std::to_string(b) + " has no frames");
        if ((size_t)clips[b].T > (size_t)h->impl->max_frames())
            return fail(h, QASR_ERR_INVALID, std::string(WHO) + ": clip " + std::to_string(b) + " holds " + std::to_string(clips[b].T) +
                                                 " frames, more than max_frames = " + std::to_string(h->impl->max_frames()));
    }
    return guarded(h, [&] { h->impl->run(clips, mode); });
}

// NOT_LOADED comes before every other refusal
static int ready(qasr_hift* h) {
    if (!h || !h->impl) return QASR_ERR_INVALID;
    if (!h->impl->loaded()) return fail(h, QASR_ERR_NOT_LOADED, std::string(WHO) + ": model unloaded");
    return QASR_OK;
}

static int null_argument(qasr_hift* h) { return fail(h, QASR_ERR_INVALID, std::string(WHO) + ": null argument"); }

extern "C" {

int qasr_hift_create(int device, const char* model_dir, size_t max_frames, qasr_engine* order_with, qasr_hift** out) {
    if (!out) return QASR_ERR_INVALID;
    *out = nullptr;
    if (!model_dir) return fail<qasr_hift>(nullptr, QASR_ERR_INVALID, std::string(WHO) + ": model_dir is NULL");
    if (max_frames == 0) max_frames = (size_t)HF_DEFAULT_FRAMES;
    if (max_frames > (size_t)HF_MAX_FRAMES)
        return fail<qasr_hift>(nullptr, QASR_ERR_INVALID, std::string(WHO) + ": max_frames in 1..2^17 (0 = 4096)");
    if (order_with && (!order_with->impl || order_with->impl->config().device != device))
        return fail<qasr_hift>(nullptr, QASR_ERR_INVALID, std::string(WHO) + ": order_with must be an engine on the same device");
    CheckedWeights w;
    try {                                              // every key, shape and dtype before any HIP call; beta, up_activations.* and
        w = load_checked_f32(model_dir, WHO, hift_tensor_shapes(), false, nullptr, "hifigan.safetensors");     // final_activation.* are not read
    } catch (const WeightLoadError& ex) { return fail<qasr_hift>(nullptr, ex.code, ex.what()); }
    catch (const std::exception& ex) { return fail<qasr_hift>(nullptr, QASR_ERR_IO, ex.what()); }
    return guarded_create(out, QASR_ERR_INVALID, [&](qasr_hift* h) {
        h->impl = std::make_unique<HiftCosyVoice>(device, w, (long)max_frames, order_with ? order_with->impl->stream() : nullptr);
    });
}

void qasr_hift_destroy(qasr_hift* h) { delete h; }
const char* qasr_hift_last_error(const qasr_hift* h) { return error_slot(h).c_str(); }
int qasr_hift_is_loaded(const qasr_hift* h) { return h && h->impl && h->impl->loaded() ? 1 : 0; }
int qasr_hift_unload(qasr_hift* h) {
    if (!h || !h->impl) return QASR_ERR_INVALID;
    return guarded(h, [&] { h->impl->unload(); });
}
size_t qasr_hift_memory_footprint(const qasr_hift* h) { return h && h->impl ? h->impl->footprint() : 0; }
int qasr_hift_sample_rate(void) { return HF_RATE; }
size_t qasr_hift_num_samples(size_t T) { return hift_num_samples(T); }

int qasr_hift_noise(uint64_t seed, const uint64_t* counters, size_t n, float* uniform, float* normal) {
    if (n && (!counters || (!uniform && !normal))) return QASR_ERR_INVALID;
    for (size_t i = 0; i < n; ++i) {                   // the lines the kernels run (voc_cosyvoice.h), on the host
        const unsigned long long r = hift_draw(seed, counters[i]);
        if (uniform) uniform[i] = hift_uniform(r);
        if (normal) normal[i] = hift_normal(r);
    }
    return QASR_OK;
}

int qasr_hift_f0(qasr_hift* h, const float* mel, size_t T, float* f0) {
    if (const int rc = ready(h)) return rc;
    if (!mel || !f0) return null_argument(h);
    std::vector<HiftClip> c{{mel, (long)T, 0, nullptr, f0, nullptr, nullptr, nullptr}};
    return run(h, c, HiftCosyVoice::F0);
}

int qasr_hift_source(qasr_hift* h, const float* f0, size_t T, uint64_t seed, float* src) {
    if (const int rc = ready(h)) return rc;
    if (!f0 || !src) return null_argument(h);
    std::vector<HiftClip> c{{nullptr, (long)T, seed, f0, nullptr, nullptr, src, nullptr}};
    return run(h, c, HiftCosyVoice::SOURCE);
}

int qasr_hift_decode_source(qasr_hift* h, const float* mel, size_t T, const float* src, float* pcm) {
    if (const int rc = ready(h)) return rc;
    if (!mel || !src || !pcm) return null_argument(h);
    std::vector<HiftClip> c{{mel, (long)T, 0, nullptr, nullptr, src, nullptr, pcm}};
    return run(h, c, HiftCosyVoice::DECODE_SOURCE);
}

int qasr_hift_decode_batch(qasr_hift* h, const float* const* mel, const size_t* T, const uint64_t* seeds, size_t B, float* const* pcm) {
    if (const int rc = ready(h)) return rc;
    if (B == 0) return QASR_OK;
    if (!mel || !T || !seeds || !pcm) return null_argument(h);
    std::vector<HiftClip> c;
    for (size_t b = 0; b < B; ++b) {
        if (!mel[b] || !pcm[b]) return null_argument(h);
        if (T[b] > (size_t)HF_MAX_FRAMES) return fail(h, QASR_ERR_INVALID, std::string(WHO) + ": clip " + std::to_string(b) + " is too long");
        c.push_back({mel[b], (long)T[b], seeds[b], nullptr, nullptr, nullptr, nullptr, pcm[b]});
    }
    return run(h, c, HiftCosyVoice::DECODE);
}

int qasr_hift_decode(qasr_hift* h, const float* mel, size_t T, uint64_t seed, float* pcm) {
    return qasr_hift_decode_batch(h, &mel, &T, &seed, 1, &pcm);
}

int qasr_hift_timing(const qasr_hift* h, float* ms) {
    if (!h || !h->impl) return QASR_ERR_INVALID;
    if (ms) std::memcpy(ms, h->impl->timing(), HF_STAGES * sizeof(float));
    return QASR_OK;
}

}  // extern "C"
