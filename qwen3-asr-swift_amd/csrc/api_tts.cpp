// api_tts.cpp -- extern "C" boundary of the Qwen3-TTS Talker + code predictor (include/qasr.h, qasr_tts_*).  Exceptions never cross it.
#include "api_guard.h"
#include "tts_talker.h"
#include <memory>

struct qasr_tts {
    std::unique_ptr<qasr::TtsTalker> impl;
    mutable std::string last_error;
};
static std::string& error_slot(const qasr_tts* t) { return t ? t->last_error : create_error<qasr_tts>(); }

using namespace qasr;

static const std::string WHO = "talker";

// the rows of one request, checked on the host before anything is uploaded
static int check_request(qasr_tts* t, const qasr_tts_request* rq, std::vector<TtsRow>& rows) {
    if (!t || !t->impl) return QASR_ERR_INVALID;
    const qasr_tts_config& c = t->impl->config();
    if (!rq) return fail(t, QASR_ERR_INVALID, WHO + ": null request");
    if (rq->B > (size_t)c.max_batch)
        return fail(t, QASR_ERR_CAPACITY, WHO + ": " + std::to_string(rq->B) + " rows, more than max_batch = " + std::to_string(c.max_batch));
    if (rq->B == 0) return QASR_OK;
    if (!rq->text || !rq->text_len || !rq->language) return fail(t, QASR_ERR_INVALID, WHO + ": null argument");
    for (size_t b = 0; b < rq->B; ++b) {
        const std::string row = WHO + ": row " + std::to_string(b) + ": ";
        TtsRow r{};
        r.text = rq->text[b]; r.n_text = rq->text_len[b];
        if (!r.text) return fail(t, QASR_ERR_INVALID, row + "null text");
        if (r.n_text < TTS_TEMPLATE)
            return fail(t, QASR_ERR_INVALID, row + "text of " + std::to_string(r.n_text) + " ids is shorter than the 9 template tokens");
        if (r.n_text > c.max_text)
            return fail(t, QASR_ERR_CAPACITY, row + "text of " + std::to_string(r.n_text) + " ids, more than max_text = " + std::to_string(c.max_text));
        for (int i = 0; i < r.n_text; ++i)
            if (r.text[i] < 0 || r.text[i] >= c.text_vocab)
                return fail(t, QASR_ERR_INVALID, row + "text id " + std::to_string(r.text[i]) + " outside the text vocabulary");
        r.language = rq->language[b];
        if (r.language < 0 || r.language >= c.codec_vocab)
            return fail(t, QASR_ERR_INVALID, row + "language id " + std::to_string(r.language) + " outside the codec vocabulary");
        r.speaker = rq->speaker ? rq->speaker[b] : -1;
        if (r.speaker >= c.codec_vocab)
            return fail(t, QASR_ERR_INVALID, row + "speaker id " + std::to_string(r.speaker) + " outside the codec vocabulary");
        r.xvector = rq->xvector ? rq->xvector[b] : nullptr;
        r.instruct = rq->instruct ? rq->instruct[b] : nullptr;
        r.n_instruct = r.instruct && rq->instruct_len ? rq->instruct_len[b] : 0;
        if (r.n_instruct < 0) return fail(t, QASR_ERR_INVALID, row + "negative instruct length");
        if (r.n_instruct > c.max_instruct)
            return fail(t, QASR_ERR_CAPACITY, row + "instruct of " + std::to_string(r.n_instruct) + " ids, more than max_instruct = " + std::to_string(c.max_instruct));
        for (int i = 0; i < r.n_instruct; ++i)
            if (r.instruct[i] < 0 || r.instruct[i] >= c.text_vocab)
                return fail(t, QASR_ERR_INVALID, row + "instruct id " + std::to_string(r.instruct[i]) + " outside the text vocabulary");
        r.index = rq->row_index ? rq->row_index[b] : (long long)b;
        rows.push_back(r);
    }
    return QASR_OK;
}

static int check_sampling(qasr_tts* t, const qasr_tts_sampling* s) {
    if (!s) return fail(t, QASR_ERR_INVALID, WHO + ": null sampling");
    if (s->top_p < 1.0f)
        return fail(t, QASR_ERR_UNSUPPORTED, WHO + ": top_p < 1 is not served (the reference's branch masks the likeliest tokens; DESIGN.md section 18)");
    if (!(s->repetition_penalty > 0.0f)) return fail(t, QASR_ERR_INVALID, WHO + ": repetition_penalty must be positive");
    return QASR_OK;
}

extern "C" {

int qasr_tts_default_config(const char* model, int bits, qasr_tts_config* out) {
    if (!out) return QASR_ERR_INVALID;
    const std::string m = model ? model : "0.6B";
    const bool large = m.find("1.7B") != std::string::npos || m.find("1.7b") != std::string::npos;
    if (bits == 0) bits = 4;
    if (bits != 4 && bits != 8) return QASR_ERR_INVALID;
    qasr_tts_config c{};
    c.hidden = large ? 2048 : 1024; c.layers = 28; c.heads = 16; c.kv_heads = 8; c.head_dim = 128; c.inter = large ? 6144 : 3072;
    c.text_vocab = 151936; c.text_hidden = 2048; c.codec_vocab = 3072;
    c.cp_hidden = 1024; c.cp_embedding_dim = large ? 2048 : 1024; c.cp_layers = 5; c.cp_heads = 16; c.cp_kv_heads = 8; c.cp_head_dim = 128;
    c.cp_inter = 3072; c.cp_vocab = 2048;
    c.rms_eps = 1e-6f; c.rope_theta = 1e6f; c.cp_rms_eps = 1e-6f; c.cp_rope_theta = 1e6f;
    c.bits = bits; c.group_size = 64;
    c.codec_pad = 2148; c.codec_bos = 2149; c.codec_eos = 2150; c.codec_think = 2154; c.codec_nothink = 2155; c.codec_think_bos = 2156;
    c.codec_think_eos = 2157;
    c.suppress_lo = 2048; c.suppress_hi = 3072;
    c.tts_pad = 151671; c.tts_bos = 151672; c.tts_eos = 151673;
    c.max_batch = 8; c.max_frames = TTS_MAX_FRAMES; c.max_text = 512; c.max_instruct = 0; c.device = 0;
    *out = c;
    return QASR_OK;
}

void qasr_tts_default_sampling(int greedy, qasr_tts_sampling* out) {
    if (!out) return;
    *out = qasr_tts_sampling{greedy ? 0.0f : 0.9f, greedy ? 1 : 50, 1.0f, 1.05f, 4096, 0.0f};
}

int qasr_tts_poll_interval(void) { return TTS_POLL; }

int qasr_tts_create(const char* model_dir, const qasr_tts_config* cfg, qasr_tts** out) {
    if (!out) return QASR_ERR_INVALID;
    *out = nullptr;
    if (!model_dir || !cfg) return fail<qasr_tts>(nullptr, QASR_ERR_INVALID, WHO + ": model_dir or cfg is NULL");
    try { TtsTalker::check_geometry(*cfg); }
    catch (const std::exception& ex) { return fail<qasr_tts>(nullptr, QASR_ERR_INVALID, ex.what()); }
    std::unique_ptr<SafeTensorsDir> st;            // all *.safetensors of the directory (TTSWeightLoading.swift:24-30); other keys are not read
    try { st = std::make_unique<SafeTensorsDir>(model_dir); }
    catch (const std::exception& ex) { return fail<qasr_tts>(nullptr, QASR_ERR_IO, WHO + ": " + ex.what()); }
    qasr_tts* h = new qasr_tts();
    try { h->impl = std::make_unique<TtsTalker>(*cfg, *st); }
    catch (const WeightLoadError& ex) { delete h; return fail<qasr_tts>(nullptr, ex.code, ex.what()); }
    catch (const HipError& ex) { delete h; return fail<qasr_tts>(nullptr, QASR_ERR_HIP, ex.what()); }
    catch (const std::exception& ex) { delete h; return fail<qasr_tts>(nullptr, QASR_ERR_INVALID, ex.what()); }
    *out = h;
    return QASR_OK;
}

void qasr_tts_free(qasr_tts* t) { delete t; }
const char* qasr_tts_last_error(const qasr_tts* t) { return error_slot(t).c_str(); }
size_t qasr_tts_memory_footprint(const qasr_tts* t) { return t && t->impl ? t->impl->footprint() : 0; }
size_t qasr_tts_device_bytes(const qasr_tts* t) { return t && t->impl ? t->impl->device_bytes() : 0; }

int qasr_tts_generate(qasr_tts* t, const qasr_tts_request* rq, const qasr_tts_sampling* s, uint64_t seed, int32_t* codes, int32_t* n_frames) {
    std::vector<TtsRow> rows;
    if (int rc = check_request(t, rq, rows)) return rc;
    if (int rc = check_sampling(t, s)) return rc;
    if (rows.empty()) return QASR_OK;
    if (!codes || !n_frames) return fail(t, QASR_ERR_INVALID, WHO + ": null output");
    const int cap = t->impl->config().max_frames;
    const int frames = s->max_tokens > 0 && s->max_tokens < cap ? s->max_tokens : cap;
    return guarded(t, [&] { t->impl->generate(rows, *s, seed, frames, codes, n_frames); });
}

int qasr_tts_forced(qasr_tts* t, const qasr_tts_request* rq, const int32_t* codes, size_t T, float* talker_logits, float* cp_logits,
                    float* hidden) {
    std::vector<TtsRow> rows;
    if (int rc = check_request(t, rq, rows)) return rc;
    if (rows.empty() || T == 0) return QASR_OK;
    const qasr_tts_config& c = t->impl->config();
    if (!codes) return fail(t, QASR_ERR_INVALID, WHO + ": null codes");
    if (T > (size_t)c.max_frames) return fail(t, QASR_ERR_CAPACITY, WHO + ": " + std::to_string(T) + " forced frames, more than max_frames");
    for (size_t b = 0; b < rows.size(); ++b)
        for (int g = 0; g < TTS_GROUPS; ++g)
            for (size_t i = 0; i < T; ++i) {
                const int v = codes[(b * TTS_GROUPS + g) * T + i];
                if (v < 0 || v >= (g == 0 ? c.codec_vocab : c.cp_vocab))
                    return fail(t, QASR_ERR_INVALID, WHO + ": forced code " + std::to_string(v) + " of stream " + std::to_string(g) + " outside its vocabulary");
            }
    TtsForcedOut f{codes, (int)T, talker_logits, cp_logits, hidden};
    return guarded(t, [&] { t->impl->forced(rows, f); });
}

int qasr_tts_sample_host(const qasr_tts_config* cfg, const float* logits, int32_t V, int talker, const qasr_tts_sampling* s,
                         const int32_t* history, int32_t n_history, uint64_t seed, int64_t row_index, int32_t frame, int32_t group) {
    if (!logits || !s || V < 1 || n_history < 0 || (n_history > 0 && !history)) return -QASR_ERR_INVALID;
    if (s->top_p < 1.0f) return -QASR_ERR_UNSUPPORTED;
    qasr_tts_config c;
    if (cfg) c = *cfg;
    else qasr_tts_default_config(nullptr, 4, &c);
    TtsSampleParams p{s->temperature, talker ? s->repetition_penalty : 1.0f, talker ? s->eos_logit_bias : 0.0f, s->top_k,
                      c.suppress_lo, c.suppress_hi, talker ? c.codec_eos : -1, seed};
    std::vector<unsigned char> seen(V, 0);
    for (int i = 0; i < n_history; ++i)
        if (history[i] >= 0 && history[i] < V) seen[history[i]] = 1;
    try { return tts_sample_host(logits, V, p, seen.data(), row_index, frame, group); }
    catch (...) { return -QASR_ERR_INVALID; }
}

int qasr_tts_synthesize(qasr_tts* t, qasr_codec* codec, const qasr_tts_request* rq, const qasr_tts_sampling* s, uint64_t seed,
                        float* const* pcm, size_t* n_samples, int32_t* codes, int32_t* n_frames) {
    if (!t || !t->impl) return QASR_ERR_INVALID;
    if (!codec || !rq || !pcm || !n_samples) return fail(t, QASR_ERR_INVALID, WHO + ": null argument");
    const size_t B = rq->B, F = (size_t)t->impl->config().max_frames;
    std::vector<int32_t> own_codes, own_frames;
    if (!codes) { own_codes.resize(B * TTS_GROUPS * F); codes = own_codes.data(); }
    if (!n_frames) { own_frames.resize(B); n_frames = own_frames.data(); }
    if (int rc = qasr_tts_generate(t, rq, s, seed, codes, n_frames)) return rc;
    const size_t spf = (size_t)qasr_codec_samples_per_frame();
    std::vector<int32_t> row;
    for (size_t b = 0; b < B; ++b) {
        const size_t T = (size_t)n_frames[b];
        n_samples[b] = spf * T;
        if (T == 0) continue;                                            // EOS first: an empty waveform
        if (!pcm[b]) return fail(t, QASR_ERR_INVALID, WHO + ": null pcm buffer");
        row.resize(TTS_GROUPS * T);                                      // [16][T] of the row's [16][max_frames]
        for (int g = 0; g < TTS_GROUPS; ++g)
            for (size_t i = 0; i < T; ++i) row[g * T + i] = codes[(b * TTS_GROUPS + g) * F + i];
        if (int rc = qasr_codec_decode(codec, row.data(), T, pcm[b]))
            return fail(t, rc, WHO + ": codec: " + qasr_codec_last_error(codec));
    }
    return QASR_OK;
}

}  // extern "C"
