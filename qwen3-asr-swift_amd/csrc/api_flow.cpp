// api_flow.cpp -- extern "C" boundary of the CosyVoice3 flow-matching mel decoder (include/qasr.h, qasr_flow_*).  Exceptions never cross it.
#include "api_guard.h"
#include "flow_cosyvoice.h"
#include <memory>

struct qasr_flow {
    std::unique_ptr<qasr::FlowCosyVoice> impl;
    mutable std::string last_error;
};
static std::string& error_slot(const qasr_flow* h) { return h ? h->last_error : create_error<qasr_flow>(); }

using namespace qasr;

static const char* const WHO = "flow decoder";

// NOT_LOADED comes before every other refusal
static int ready(qasr_flow* h) {
    if (!h || !h->impl) return QASR_ERR_INVALID;
    if (!h->impl->loaded()) return fail(h, QASR_ERR_NOT_LOADED, std::string(WHO) + ": model unloaded");
    return QASR_OK;
}
static int null_argument(qasr_flow* h) { return fail(h, QASR_ERR_INVALID, std::string(WHO) + ": null argument"); }
static int invalid(qasr_flow* h, const std::string& m) { return fail(h, QASR_ERR_INVALID, std::string(WHO) + ": " + m); }

// what a clip of a generate call must satisfy, host only (h may be null: the message then goes to the create slot)
static int check_clip(const qasr_flow* h, const std::string& who, const int32_t* tokens, size_t n, const int32_t* prompt_tokens, size_t np, size_t tp, int vocab,
                      size_t max_frames) {
    auto bad = [&](const std::string& m) { return fail(h, QASR_ERR_INVALID, std::string(WHO) + ": " + who + m); };
    if (!tokens || (np && !prompt_tokens)) return bad(": null argument");
    if (n == 0) return bad(" has no tokens");
    if (n > (size_t)FL_MAX_FRAMES || np > (size_t)FL_MAX_FRAMES) return bad(" is too long");
    const size_t T = flow_mel_frames(n + np);
    if (T > max_frames) return bad(" holds " + std::to_string(T) + " frames, more than max_frames = " + std::to_string(max_frames));
    if (tp != flow_mel_frames(np) || tp > T)                // FlowMatching.swift:288-289, :350-351
        return bad(": the prompt mel holds " + std::to_string(tp) + " frames, " + std::to_string(np) + " prompt tokens need " + std::to_string(flow_mel_frames(np)));
    for (size_t i = 0; i < np + n; ++i) {                   // refused, not clamped
        const int32_t id = i < np ? prompt_tokens[i] : tokens[i - np];
        if (id < 0 || id >= vocab) return bad(": token " + std::to_string(i) + " is " + std::to_string(id) + ", outside [0, " + std::to_string(vocab) + ")");
    }
    return QASR_OK;
}

extern "C" {

int qasr_flow_create(int device, const char* model_dir, size_t max_frames, qasr_engine* order_with, qasr_flow** out) {
    if (!out) return QASR_ERR_INVALID;
    *out = nullptr;
    if (!model_dir) return fail<qasr_flow>(nullptr, QASR_ERR_INVALID, std::string(WHO) + ": model_dir is NULL");
    if (max_frames == 0) max_frames = (size_t)FL_DEFAULT_FRAMES;
    if (max_frames > (size_t)FL_MAX_FRAMES || max_frames < 2)
        return fail<qasr_flow>(nullptr, QASR_ERR_INVALID, std::string(WHO) + ": max_frames in 2..2^15 (0 = 4096)");
    if (order_with && (!order_with->impl || order_with->impl->config().device != device))
        return fail<qasr_flow>(nullptr, QASR_ERR_INVALID, std::string(WHO) + ": order_with must be an engine on the same device");
    FlowWeights w;
    try { w = flow_load_weights(model_dir); }              // every key, shape and dtype before any HIP call
    catch (const WeightLoadError& ex) { return fail<qasr_flow>(nullptr, ex.code, ex.what()); }
    catch (const std::exception& ex) { return fail<qasr_flow>(nullptr, QASR_ERR_IO, ex.what()); }
    return guarded_create(out, QASR_ERR_INVALID, [&](qasr_flow* h) {
        h->impl = std::make_unique<FlowCosyVoice>(device, w, (long)max_frames, order_with ? order_with->impl->stream() : nullptr);
    });
}

void qasr_flow_destroy(qasr_flow* h) { delete h; }
const char* qasr_flow_last_error(const qasr_flow* h) { return error_slot(h).c_str(); }
int qasr_flow_is_loaded(const qasr_flow* h) { return h && h->impl && h->impl->loaded() ? 1 : 0; }
int qasr_flow_unload(qasr_flow* h) {
    if (!h || !h->impl) return QASR_ERR_INVALID;
    return guarded(h, [&] { h->impl->unload(); });
}
size_t qasr_flow_memory_footprint(const qasr_flow* h) { return h && h->impl ? h->impl->footprint() : 0; }
size_t qasr_flow_mel_frames(size_t n_tokens) { return flow_mel_frames(n_tokens); }
int qasr_flow_depth(const qasr_flow* h) { return h && h->impl ? h->impl->depth() : 0; }

int qasr_flow_check_clip(const int32_t* tokens, size_t n, const int32_t* prompt_tokens, size_t n_prompt, size_t prompt_frames, int vocab, size_t max_frames) {
    if (max_frames == 0) max_frames = (size_t)FL_DEFAULT_FRAMES;
    return check_clip(nullptr, "clip", tokens, n, prompt_tokens, n_prompt, prompt_frames, vocab, max_frames);
}

int qasr_flow_schedule(int n_steps, float* t) {
    if (!t || n_steps < 1 || n_steps > FL_MAX_STEPS) return QASR_ERR_INVALID;
    flow_schedule(n_steps, t);
    return QASR_OK;
}

int qasr_flow_mu(qasr_flow* h, const int32_t* tokens, size_t n, float* mu) {
    if (const int rc = ready(h)) return rc;
    if (!tokens || !mu) return null_argument(h);
    if (n == 0) return invalid(h, "no tokens");
    if (n > (size_t)FL_MAX_FRAMES) return invalid(h, "too many tokens");
    return guarded(h, [&] { h->impl->mu(tokens, (long)n, mu); });
}

int qasr_flow_spks(qasr_flow* h, const float* emb192, float* spks80) {
    if (const int rc = ready(h)) return rc;
    if (!spks80) return null_argument(h);
    return guarded(h, [&] { h->impl->spks(emb192, spks80); });
}

int qasr_flow_velocity(qasr_flow* h, const float* x, const float* mu, const float* spks, const float* cond, size_t T, float t, float* v) {
    if (const int rc = ready(h)) return rc;
    if (!x || !mu || !v) return null_argument(h);
    if (T == 0) return invalid(h, "no frames");
    if (T > (size_t)FL_MAX_FRAMES) return invalid(h, "the clip is too long");
    return guarded(h, [&] { h->impl->velocity(x, mu, spks, cond, (long)T, t, v); });
}

int qasr_flow_solve(qasr_flow* h, const float* mu, const float* spks, const float* cond, size_t T, const float* z, int n_steps, float* v_out, float* mel) {
    if (const int rc = ready(h)) return rc;
    if (!mu || !z || !mel) return null_argument(h);
    if (T == 0) return invalid(h, "no frames");
    if (T > (size_t)FL_MAX_FRAMES) return invalid(h, "the clip is too long");
    if (n_steps == 0) n_steps = FL_DEFAULT_STEPS;
    FlowClip c;
    c.T = (long)T; c.x = z; c.mu = mu; c.spks = spks; c.cond = cond; c.v_out = v_out; c.mel = mel;
    return guarded(h, [&] { h->impl->solve({c}, n_steps); });
}

// tokens: prompt tokens then new tokens (FlowMatching.swift:306-312); prompt_feat [80][prompt_frames]; mel and z_out [80][2 (n + n_prompt)]
int qasr_flow_generate_batch(qasr_flow* h, const int32_t* const* tokens, const size_t* n, const int32_t* const* prompt_tokens, const size_t* n_prompt,
                             const float* const* prompt_feat, const size_t* prompt_frames, const float* const* spk_emb, int n_steps, float temperature,
                             const uint64_t* seeds, size_t B, float* const* z_out, float* const* mel) {
    if (const int rc = ready(h)) return rc;
    if (B == 0) return QASR_OK;
    if (!tokens || !n || !seeds || !mel) return null_argument(h);
    if (n_steps == 0) n_steps = FL_DEFAULT_STEPS;
    if (n_steps < 1 || n_steps > FL_MAX_STEPS) return invalid(h, "n_steps in 1..64 (0 = 10)");
    if (!(temperature >= 0.0f) || !std::isfinite(temperature)) return invalid(h, "temperature must be finite and not negative");
    struct Work { std::vector<int32_t> tok; std::vector<float> mu, cond, spk, z, mel; bool has_cond = false, has_spk = false; };
    std::vector<Work> w(B);
    for (size_t b = 0; b < B; ++b) {
        const std::string who = "clip " + std::to_string(b);
        if (!tokens[b] || !mel[b]) return null_argument(h);
        const size_t np = (prompt_tokens && n_prompt && prompt_tokens[b]) ? n_prompt[b] : 0;
        const size_t tp = (prompt_feat && prompt_frames && prompt_feat[b]) ? prompt_frames[b] : 0;
        if (const int rc = check_clip(h, who, tokens[b], n[b], np ? prompt_tokens[b] : nullptr, np, tp, h->impl->vocab(), (size_t)h->impl->max_frames())) return rc;
        const size_t T = flow_mel_frames(n[b] + np);
        Work& k = w[b];
        if (np) k.tok.assign(prompt_tokens[b], prompt_tokens[b] + np);
        k.tok.insert(k.tok.end(), tokens[b], tokens[b] + n[b]);
        k.mu.resize(T * FL_MEL);
        k.mel.resize(T * FL_MEL);
        if (z_out && z_out[b]) k.z.resize(T * FL_MEL);
        if (tp) {                                          // conds[:, :, :Tp] = prompt_feat, zeros after (FlowMatching.swift:343-360)
            k.has_cond = true;
            k.cond.assign(T * FL_MEL, 0.0f);
            for (size_t t = 0; t < tp; ++t)
                for (int m = 0; m < FL_MEL; ++m) k.cond[t * FL_MEL + m] = prompt_feat[b][(size_t)m * tp + t];
        }
        k.has_spk = spk_emb && spk_emb[b];
        k.spk.assign(FL_MEL, 0.0f);
    }
    const int rc = guarded(h, [&] {
        std::vector<FlowClip> clips(B);
        for (size_t b = 0; b < B; ++b) {
            Work& k = w[b];
            h->impl->mu(k.tok.data(), (long)k.tok.size(), k.mu.data());
            if (k.has_spk) h->impl->spks(spk_emb[b], k.spk.data());
            FlowClip& c = clips[b];
            c.T = (long)(k.mu.size() / FL_MEL);
            c.mu = k.mu.data();
            c.spks = k.has_spk ? k.spk.data() : nullptr;
            c.cond = k.has_cond ? k.cond.data() : nullptr;
            c.noise = true;
            c.seed = seeds[b];
            c.temperature = temperature;
            c.z_out = k.z.empty() ? nullptr : k.z.data();
            c.mel = k.mel.data();
        }
        h->impl->solve(clips, n_steps);
    });
    if (rc != QASR_OK) return rc;
    for (size_t b = 0; b < B; ++b) {                       // [T][80] -> [80][T], as the reference returns it (FlowMatching.swift:375)
        const size_t T = w[b].mel.size() / FL_MEL;
        for (size_t t = 0; t < T; ++t)
            for (int m = 0; m < FL_MEL; ++m) {
                mel[b][(size_t)m * T + t] = w[b].mel[t * FL_MEL + m];
                if (!w[b].z.empty()) z_out[b][(size_t)m * T + t] = w[b].z[t * FL_MEL + m];
            }
    }
    return QASR_OK;
}

int qasr_flow_generate(qasr_flow* h, const int32_t* tokens, size_t n, const int32_t* prompt_tokens, size_t n_prompt, const float* prompt_feat,
                       size_t prompt_frames, const float* spk_emb, int n_steps, float temperature, uint64_t seed, float* z_out, float* mel) {
    if (const int rc = ready(h)) return rc;
    if (!tokens || !mel) return null_argument(h);
    return qasr_flow_generate_batch(h, &tokens, &n, &prompt_tokens, &n_prompt, &prompt_feat, &prompt_frames, &spk_emb, n_steps, temperature, &seed, 1,
                                    z_out ? &z_out : nullptr, &mel);
}

int qasr_flow_timing(const qasr_flow* h, float* ms) {
    if (!h || !h->impl) return QASR_ERR_INVALID;
    if (ms) std::memcpy(ms, h->impl->timing(), FL_STAGES * sizeof(float));
    return QASR_OK;
}

}  // extern "C"
