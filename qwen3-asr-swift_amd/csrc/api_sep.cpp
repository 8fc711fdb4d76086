// api_sep.cpp -- extern "C" boundary of the Open-Unmix source separator (include/qasr.h, qasr_sep_*).  Exceptions never cross it.
#include "api_guard.h"
#include "sep_openunmix.h"
#include <memory>

struct qasr_sep {
    std::unique_ptr<qasr::SepOpenUnmix> impl;
    mutable std::string last_error;
};
static std::string& error_slot(const qasr_sep* s) { return s ? s->last_error : create_error<qasr_sep>(); }

using namespace qasr;

static constexpr size_t SEP_DEFAULT_SAMPLES = (size_t)64 * 10 * SEP_RATE;

static int check_cfg(qasr_sep* s, const qasr_sep_config* cfg, qasr_sep_config* c) {
    qasr_sep_default_config(c);
    if (cfg) *c = *cfg;
    if (c->wiener_iterations < 1 || c->wiener_iterations > 16 || c->wiener_window < 1)
        return fail(s, QASR_ERR_INVALID, "open-unmix: wiener_iterations in 1..16 and wiener_window >= 1");
    return QASR_OK;
}

extern "C" {

int qasr_sep_default_config(qasr_sep_config* out) {
    if (!out) return QASR_ERR_INVALID;
    out->wiener = 1; out->wiener_iterations = 1; out->wiener_window = 300;
    return QASR_OK;
}

int qasr_sep_create(int device, const char* model_dir, size_t max_batch_samples, qasr_engine* order_with, qasr_sep** out) {
    if (!out) return QASR_ERR_INVALID;
    *out = nullptr;
    if (!model_dir) return fail<qasr_sep>(nullptr, QASR_ERR_INVALID, "open-unmix: model_dir is NULL");
    if (max_batch_samples == 0) max_batch_samples = SEP_DEFAULT_SAMPLES;
    if (max_batch_samples > ((size_t)1 << 36)) return fail<qasr_sep>(nullptr, QASR_ERR_INVALID, "open-unmix: max_batch_samples up to 2^36 (0 = 64 x 10 s)");
    if (order_with && (!order_with->impl || order_with->impl->config().device != device))
        return fail<qasr_sep>(nullptr, QASR_ERR_INVALID, "open-unmix: order_with must be an engine on the same device");
    CheckedWeights w[SEP_STEMS];
    int hidden = 0;
    try {                                              // every file, key, shape and dtype before any HIP call
        const std::string first = std::string(SEP_STEM_NAMES[0]) + ".safetensors";
        {   // the preset is the checkpoint's (OpenUnmixConfig.swift:24-46): fc1.weight is [hidden][2974]
            std::unique_ptr<SafeTensorsDir> st;
            try { st = std::make_unique<SafeTensorsDir>(model_dir, first); }
            catch (const std::exception& ex) { throw WeightLoadError(QASR_ERR_IO, std::string("open-unmix: ") + ex.what()); }
            auto it = st->entries.find("fc1.weight");
            if (it == st->entries.end()) throw WeightLoadError(QASR_ERR_IO, "open-unmix: " + first + ": missing tensor fc1.weight");
            const auto& sh = it->second.shape;
            if (sh.size() != 2 || (sh[0] != 512 && sh[0] != 1024))
                throw WeightLoadError(QASR_ERR_INVALID, "open-unmix: " + first + ": tensor fc1.weight names no preset (hidden 512 umxhq | 1024 umxl)");
            hidden = (int)sh[0];
        }
        const auto shapes = sep_tensor_shapes(hidden);
        for (int i = 0; i < SEP_STEMS; ++i) {
            const std::string file = std::string(SEP_STEM_NAMES[i]) + ".safetensors", who = "open-unmix: " + file;
            w[i] = load_checked_f32(model_dir, who.c_str(), shapes, true, nullptr, file.c_str());
        }
    } catch (const WeightLoadError& ex) { return fail<qasr_sep>(nullptr, ex.code, ex.what()); }
    catch (const std::exception& ex) { return fail<qasr_sep>(nullptr, QASR_ERR_IO, ex.what()); }
    return guarded_create(out, QASR_ERR_INVALID, [&](qasr_sep* s) {
        s->impl = std::make_unique<SepOpenUnmix>(device, w, hidden, max_batch_samples, order_with ? order_with->impl->stream() : nullptr);
    });
}

void qasr_sep_destroy(qasr_sep* s) { delete s; }
const char* qasr_sep_last_error(const qasr_sep* s) { return error_slot(s).c_str(); }
int qasr_sep_is_loaded(const qasr_sep* s) { return s && s->impl && s->impl->loaded() ? 1 : 0; }
int qasr_sep_unload(qasr_sep* s) {
    if (!s || !s->impl) return QASR_ERR_INVALID;
    return guarded(s, [&] { s->impl->unload(); });
}
size_t qasr_sep_memory_footprint(const qasr_sep* s) { return s && s->impl ? s->impl->footprint() : 0; }
int qasr_sep_hidden_size(const qasr_sep* s) { return s && s->impl ? s->impl->hidden() : 0; }
int qasr_sep_sample_rate(void) { return SEP_RATE; }
int64_t qasr_sep_num_frames(size_t n) { return n > ((size_t)1 << 40) ? -1 : (int64_t)sep_num_frames(n); }
int qasr_sep_timing(const qasr_sep* s, float* ms) {
    if (!s || !s->impl) return QASR_ERR_INVALID;
    const SepTiming& t = s->impl->timing();
    if (ms) { ms[0] = t.stft; ms[1] = t.network; ms[2] = t.wiener; ms[3] = t.istft; }
    return QASR_OK;
}
int qasr_sep_set_recurrence_form(qasr_sep* s, int form) {
    if (!s || !s->impl) return QASR_ERR_INVALID;
    if (form != 0 && form != 1) return fail(s, QASR_ERR_INVALID, "open-unmix: recurrence form 0 (streamed) | 1 (resident + streamed)");
    s->impl->set_recurrence_form(form);
    return QASR_OK;
}

int qasr_sep_separate_batch(qasr_sep* s, const float* const* left, const float* const* right, const size_t* n, size_t B, int sample_rate,
                            unsigned target_mask, const qasr_sep_config* cfg, float* const* out) {
    if (!s || !s->impl) return QASR_ERR_INVALID;
    if (!s->impl->loaded()) return fail(s, QASR_ERR_NOT_LOADED, "open-unmix: model unloaded");
    if (sample_rate != SEP_RATE)
        return fail(s, QASR_ERR_UNSUPPORTED, "open-unmix: 44.1 kHz input only (SourceSeparator.separate does not resample either)");
    if (target_mask == 0 || (target_mask & ~0xFu)) return fail(s, QASR_ERR_INVALID, "open-unmix: target_mask is a non-empty set of bits 0..3");
    qasr_sep_config c;
    if (int rc = check_cfg(s, cfg, &c)) return rc;
    if (B == 0) return QASR_OK;
    if (!left || !right || !n || !out) return fail(s, QASR_ERR_INVALID, "open-unmix: null argument");
    for (size_t b = 0; b < B; ++b) {
        if (n[b] == 0) return fail(s, QASR_ERR_EMPTY_AUDIO, "open-unmix: file " + std::to_string(b) + " is empty");
        if (!left[b] || !out[b]) return fail(s, QASR_ERR_INVALID, "open-unmix: null file or output");
    }
    return guarded(s, [&] { s->impl->separate(left, right, n, B, target_mask, c.wiener != 0, c.wiener_iterations, c.wiener_window, out); });
}

int qasr_sep_separate(qasr_sep* s, const float* left, const float* right, size_t n, int sample_rate, unsigned target_mask,
                      const qasr_sep_config* cfg, float* out) {
    const float* l[1] = {left};
    const float* r[1] = {right};
    float* o[1] = {out};
    return qasr_sep_separate_batch(s, l, r, &n, 1, sample_rate, target_mask, cfg, o);
}

int qasr_sep_stft(qasr_sep* s, const float* left, const float* right, size_t n, float* re, float* im, float* magnitude) {
    if (!s || !s->impl) return QASR_ERR_INVALID;
    if (!s->impl->loaded()) return fail(s, QASR_ERR_NOT_LOADED, "open-unmix: model unloaded");
    if (n == 0) return fail(s, QASR_ERR_EMPTY_AUDIO, "open-unmix: empty audio");
    if (!left) return fail(s, QASR_ERR_INVALID, "open-unmix: null argument");
    if (n > s->impl->max_batch_samples()) return fail(s, QASR_ERR_CAPACITY, "open-unmix: more samples than max_batch_samples");
    return guarded(s, [&] { s->impl->stft(left, right, n, re, im, magnitude); });
}

int qasr_sep_masks(qasr_sep* s, const float* magnitude, const size_t* T, size_t B, float* out) {
    if (!s || !s->impl) return QASR_ERR_INVALID;
    if (!s->impl->loaded()) return fail(s, QASR_ERR_NOT_LOADED, "open-unmix: model unloaded");
    if (B == 0) return QASR_OK;
    if (!magnitude || !T || !out) return fail(s, QASR_ERR_INVALID, "open-unmix: null argument");
    for (size_t b = 0; b < B; ++b)
        if (T[b] == 0) return fail(s, QASR_ERR_INVALID, "open-unmix: a file without frames");
    return guarded(s, [&] { s->impl->masks(magnitude, T, B, out); });
}

int qasr_sep_wiener(qasr_sep* s, const float* masked, int n_sources, const float* re, const float* im, size_t T, const qasr_sep_config* cfg,
                    float* out_re, float* out_im) {
    if (!s || !s->impl) return QASR_ERR_INVALID;
    if (!s->impl->loaded()) return fail(s, QASR_ERR_NOT_LOADED, "open-unmix: model unloaded");
    qasr_sep_config c;
    if (int rc = check_cfg(s, cfg, &c)) return rc;
    if (!masked || !re || !im || !out_re || !out_im || T == 0) return fail(s, QASR_ERR_INVALID, "open-unmix: null argument or no frame");
    return guarded(s, [&] { s->impl->wiener(masked, n_sources, re, im, T, c.wiener_iterations, c.wiener_window, out_re, out_im); });
}

int qasr_sep_istft(qasr_sep* s, const float* re, const float* im, int n_spectra, size_t T, size_t length, float* out) {
    if (!s || !s->impl) return QASR_ERR_INVALID;
    if (!s->impl->loaded()) return fail(s, QASR_ERR_NOT_LOADED, "open-unmix: model unloaded");
    if (!re || !im || !out) return fail(s, QASR_ERR_INVALID, "open-unmix: null argument");
    return guarded(s, [&] { s->impl->istft(re, im, n_spectra, T, length, out); });
}

}  // extern "C"
