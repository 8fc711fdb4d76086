// api_s3tok.cpp -- extern "C" boundary of the CosyVoice3 speech tokenizer and voice profiles (include/qasr.h, qasr_s3tok_*).  Exceptions
// never cross it.
#include "api_guard.h"
#include "s3tok_cosyvoice.h"
#include <memory>

struct qasr_s3tok {
    std::unique_ptr<qasr::S3Tokenizer> impl;
    mutable std::string last_error;
};
static std::string& error_slot(const qasr_s3tok* h) { return h ? h->last_error : create_error<qasr_s3tok>(); }

using namespace qasr;

static const char* const WHO = "speech tokenizer";

// NOT_LOADED comes before every other refusal
static int ready(qasr_s3tok* h) {
    if (!h || !h->impl) return QASR_ERR_INVALID;
    if (!h->impl->loaded()) return fail(h, QASR_ERR_NOT_LOADED, std::string(WHO) + ": model unloaded");
    return QASR_OK;
}
static int null_argument(qasr_s3tok* h) { return fail(h, QASR_ERR_INVALID, std::string(WHO) + ": null argument"); }
static int invalid(qasr_s3tok* h, const std::string& m) { return fail(h, QASR_ERR_INVALID, std::string(WHO) + ": " + m); }

extern "C" {

int qasr_s3tok_create(int device, const char* model_dir, size_t max_tokens, qasr_engine* order_with, qasr_s3tok** out) {
    if (!out) return QASR_ERR_INVALID;
    *out = nullptr;
    if (!model_dir) return fail<qasr_s3tok>(nullptr, QASR_ERR_INVALID, std::string(WHO) + ": model_dir is NULL");
    if (max_tokens == 0) max_tokens = (size_t)S3_DEFAULT_TOKENS;
    if (max_tokens > (size_t)S3_MAX_TOKENS)
        return fail<qasr_s3tok>(nullptr, QASR_ERR_INVALID, std::string(WHO) + ": max_tokens in 1..2^14 (0 = 768)");
    if (order_with && (!order_with->impl || order_with->impl->config().device != device))
        return fail<qasr_s3tok>(nullptr, QASR_ERR_INVALID, std::string(WHO) + ": order_with must be an engine on the same device");
    S3Weights w;
    try { w = s3_load_weights(model_dir); }                // every key, shape and dtype before any HIP call
    catch (const WeightLoadError& ex) { return fail<qasr_s3tok>(nullptr, ex.code, ex.what()); }
    catch (const std::exception& ex) { return fail<qasr_s3tok>(nullptr, QASR_ERR_IO, ex.what()); }
    return guarded_create(out, QASR_ERR_INVALID, [&](qasr_s3tok* h) {
        h->impl = std::make_unique<S3Tokenizer>(device, w, (long)max_tokens, order_with ? order_with->impl->stream() : nullptr);
    });
}

void qasr_s3tok_destroy(qasr_s3tok* h) { delete h; }
const char* qasr_s3tok_last_error(const qasr_s3tok* h) { return error_slot(h).c_str(); }
int qasr_s3tok_is_loaded(const qasr_s3tok* h) { return h && h->impl && h->impl->loaded() ? 1 : 0; }
int qasr_s3tok_unload(qasr_s3tok* h) {
    if (!h || !h->impl) return QASR_ERR_INVALID;
    return guarded(h, [&] { h->impl->unload(); });
}
size_t qasr_s3tok_memory_footprint(const qasr_s3tok* h) { return h && h->impl ? h->impl->footprint() : 0; }
int qasr_s3tok_depth(const qasr_s3tok* h) { return h && h->impl ? h->impl->depth() : 0; }
size_t qasr_s3tok_max_tokens(const qasr_s3tok* h) { return h && h->impl ? (size_t)h->impl->max_tokens() : 0; }

// lengths, pure CPU (WhisperMelExtractor.swift:154-155; SpeechTokenizer.swift:255-262; FlowMelExtractor.swift:164-165; VoiceCloning.swift:331-332)
size_t qasr_s3tok_whisper_frames(size_t n_samples_16k) { return s3_whisper_frames(n_samples_16k); }
size_t qasr_s3tok_tokens(size_t mel_frames) { return s3_tokens(mel_frames); }
size_t qasr_s3tok_flow_frames(size_t n_samples_24k) { return s3_flow_frames(n_samples_24k); }
size_t qasr_s3tok_resampled_length(size_t n, int src_rate, int dst_rate) {
    return src_rate > 0 && dst_rate > 0 ? s3_resampled_length(n, src_rate, dst_rate) : 0;
}
size_t qasr_s3tok_profile_cut(size_t n_tokens, size_t frames) { return std::min(n_tokens, frames / 2); }

// resample (VoiceCloning.swift:329-345), host
int qasr_s3tok_resample(const float* x, size_t n, int src_rate, int dst_rate, float* out) {
    if (src_rate <= 0 || dst_rate <= 0 || (n && (!x || !out))) return QASR_ERR_INVALID;
    s3_resample(x, n, src_rate, dst_rate, out);
    return QASR_OK;
}

// FSQCodebook.encode from tanh on (SpeechTokenizer.swift:78-93), host
int qasr_s3tok_fsq_host(const float* proj, size_t rows, int32_t* codes) {
    if (rows && (!proj || !codes)) return QASR_ERR_INVALID;
    s3_fsq_host(proj, rows, codes);
    return QASR_OK;
}

// WhisperMelExtractor.extract (WhisperMelExtractor.swift:132-225): [128][n / 160]
int qasr_s3tok_whisper_mel(qasr_s3tok* h, const float* pcm16k, size_t n, float* mel) {
    if (const int rc = ready(h)) return rc;
    if (!pcm16k || !mel) return null_argument(h);
    if (s3_whisper_frames(n) == 0) return invalid(h, "the clip is empty (under 160 samples)");
    if (n > (size_t)S3_MAX_SAMPLES) return invalid(h, "the clip is too long");
    return guarded(h, [&] { h->impl->whisper_mel(pcm16k, (long)n, mel); });
}

// FlowMelExtractor.extract (FlowMelExtractor.swift:142-229): [80][n / 480]
int qasr_s3tok_flow_mel(qasr_s3tok* h, const float* pcm24k, size_t n, float* mel) {
    if (const int rc = ready(h)) return rc;
    if (!pcm24k || !mel) return null_argument(h);
    if (s3_flow_frames(n) == 0) return invalid(h, "the clip is empty (under 480 samples)");
    if (n > (size_t)S3_MAX_SAMPLES) return invalid(h, "the clip is too long");
    const long ln = (long)n;
    return guarded(h, [&] { h->impl->flow_mel(&pcm24k, &ln, 1, &mel); });
}

// AudioEncoderV3.callAsFunction (SpeechTokenizer.swift:279-288) and project_down (:77):
// mel [128][T] -> the residual stream after the last block and / or the projections before tanh (either may be NULL)
static int from_mel(qasr_s3tok* h, const float* mel, size_t T, float* hidden, float* proj) {
    if (const int rc = ready(h)) return rc;
    if (!mel || (!hidden && !proj)) return null_argument(h);
    if (T == 0) return invalid(h, "the clip is empty (no mel frame)");
    if (T > (size_t)S3_MAX_SAMPLES / 160) return invalid(h, "the clip is too long");
    S3Clip c;
    c.mel = mel; c.T = (long)T; c.hidden = hidden; c.proj = proj;
    return guarded(h, [&] { h->impl->run({c}); });
}
int qasr_s3tok_hidden(qasr_s3tok* h, const float* mel, size_t T, float* hidden) { return from_mel(h, mel, T, hidden, nullptr); }
int qasr_s3tok_project(qasr_s3tok* h, const float* mel, size_t T, float* proj) { return from_mel(h, mel, T, nullptr, proj); }

// SpeechTokenizerModel.encode (SpeechTokenizer.swift:312-315) on the Whisper mel of each clip (VoiceCloning.swift:82-84)
int qasr_s3tok_encode_batch(qasr_s3tok* h, const float* const* pcm16k, const size_t* n, size_t B, int32_t* const* codes) {
    if (const int rc = ready(h)) return rc;
    if (B == 0) return QASR_OK;
    if (!pcm16k || !n || !codes) return null_argument(h);
    std::vector<S3Clip> c(B);
    for (size_t b = 0; b < B; ++b) {
        if (!pcm16k[b] || !codes[b]) return null_argument(h);
        if (s3_whisper_frames(n[b]) == 0) return invalid(h, "clip " + std::to_string(b) + " is empty (under 160 samples)");
        if (n[b] > (size_t)S3_MAX_SAMPLES) return invalid(h, "clip " + std::to_string(b) + " is too long");
        c[b].pcm = pcm16k[b]; c[b].n = (long)n[b]; c[b].codes = codes[b];
    }
    return guarded(h, [&] { h->impl->run(c); });
}

int qasr_s3tok_encode(qasr_s3tok* h, const float* pcm16k, size_t n, int32_t* codes) {
    if (const int rc = ready(h)) return rc;
    if (!pcm16k || !codes) return null_argument(h);
    return qasr_s3tok_encode_batch(h, &pcm16k, &n, 1, &codes);
}

// extractVoiceProfile (VoiceCloning.swift:69-158) without the CAM++ vector, with the cut to the common length
int qasr_s3tok_profile_batch(qasr_s3tok* h, const float* const* pcm, const size_t* n, const int* sample_rate, size_t B, int32_t* const* tokens,
                             size_t* n_tokens, float* const* prompt_feat, size_t* prompt_frames, size_t* uncut_tokens, size_t* uncut_frames) {
    if (const int rc = ready(h)) return rc;
    if (B == 0) return QASR_OK;
    if (!pcm || !n || !sample_rate || !tokens || !n_tokens || !prompt_feat || !prompt_frames) return null_argument(h);
    std::vector<std::vector<float>> a16(B), a24(B), feat(B);
    std::vector<std::vector<int32_t>> tok(B);
    std::vector<S3Clip> c(B);
    for (size_t b = 0; b < B; ++b) {
        const std::string who = "clip " + std::to_string(b);
        if (!pcm[b] || !tokens[b] || !prompt_feat[b]) return null_argument(h);
        if (sample_rate[b] < 1000 || sample_rate[b] > 768000) return invalid(h, who + ": sample rate in 1000..768000");
        if (n[b] > (size_t)S3_MAX_SAMPLES) return invalid(h, who + " is too long");
        a16[b].resize(s3_resampled_length(n[b], sample_rate[b], MEL_SR));
        a24[b].resize(s3_resampled_length(n[b], sample_rate[b], FM_SR));
        const size_t nt = s3_tokens(s3_whisper_frames(a16[b].size())), nf = s3_flow_frames(a24[b].size());
        if (std::min(nt, nf / 2) == 0) return invalid(h, who + " is empty (no token or no pair of mel frames)");
        if (nt > (size_t)h->impl->max_tokens())                        // refused, not cut
            return invalid(h, who + " holds " + std::to_string(nt) + " tokens, more than max_tokens = " + std::to_string(h->impl->max_tokens()));
        if (a24[b].size() > (size_t)S3_MAX_SAMPLES) return invalid(h, who + " is too long");
        s3_resample(pcm[b], n[b], sample_rate[b], MEL_SR, a16[b].data());
        s3_resample(pcm[b], n[b], sample_rate[b], FM_SR, a24[b].data());
        tok[b].resize(nt);
        feat[b].resize(nf * FM_MELS);
        c[b].pcm = a16[b].data(); c[b].n = (long)a16[b].size(); c[b].codes = tok[b].data();
    }
    const int rc = guarded(h, [&] {
        h->impl->run(c);
        std::vector<const float*> p(B);
        std::vector<long> ln(B);
        std::vector<float*> o(B);
        for (size_t b = 0; b < B; ++b) { p[b] = a24[b].data(); ln[b] = (long)a24[b].size(); o[b] = feat[b].data(); }
        h->impl->flow_mel(p.data(), ln.data(), (int)B, o.data());
    });
    if (rc != QASR_OK) return rc;
    for (size_t b = 0; b < B; ++b) {
        const size_t nt = tok[b].size(), nf = feat[b].size() / FM_MELS, L = std::min(nt, nf / 2);
        std::memcpy(tokens[b], tok[b].data(), L * sizeof(int32_t));
        for (int m = 0; m < FM_MELS; ++m) std::memcpy(prompt_feat[b] + (size_t)m * 2 * L, feat[b].data() + (size_t)m * nf, 2 * L * sizeof(float));
        n_tokens[b] = L;
        prompt_frames[b] = 2 * L;
        if (uncut_tokens) uncut_tokens[b] = nt;
        if (uncut_frames) uncut_frames[b] = nf;
    }
    return QASR_OK;
}

int qasr_s3tok_profile(qasr_s3tok* h, const float* pcm, size_t n, int sample_rate, int32_t* tokens, size_t* n_tokens, float* prompt_feat,
                       size_t* prompt_frames, size_t* uncut_tokens, size_t* uncut_frames) {
    if (const int rc = ready(h)) return rc;
    if (!pcm || !tokens || !n_tokens || !prompt_feat || !prompt_frames) return null_argument(h);
    return qasr_s3tok_profile_batch(h, &pcm, &n, &sample_rate, 1, &tokens, n_tokens, &prompt_feat, prompt_frames, uncut_tokens, uncut_frames);
}

int qasr_s3tok_timing(const qasr_s3tok* h, float* ms) {
    if (!h || !h->impl) return QASR_ERR_INVALID;
    if (ms) std::memcpy(ms, h->impl->timing(), S3_STAGES * sizeof(float));
    return QASR_OK;
}

}  // extern "C"
