// api_cvlm.cpp -- extern "C" boundary of the CosyVoice3 speech-token LLM (include/qasr.h, qasr_cvlm_*).  Exceptions never cross it.
#include "api_guard.h"
#include "llm_cosyvoice.h"
#include <memory>

struct qasr_cvlm {
    std::unique_ptr<qasr::CosyLlm> impl;
    mutable std::string last_error;
};
static std::string& error_slot(const qasr_cvlm* h) { return h ? h->last_error : create_error<qasr_cvlm>(); }

using namespace qasr;

static const std::string WHO = "cosyvoice llm";

static void default_config(int bits, qasr_cvlm_config* c) {
    *c = qasr_cvlm_config{};
    c->hidden = 896; c->layers = 24; c->heads = 14; c->kv_heads = 2; c->head_dim = 64; c->inter = 4864;
    c->text_vocab = 151936; c->speech_tokens = 6561; c->speech_extra = 200;
    c->rms_eps = 1e-6f; c->rope_theta = 1e6f;
    c->bits = bits; c->group_size = 64;
    c->device = 0; c->max_batch = 8; c->max_text = 512; c->max_prompt_tokens = 0; c->max_tokens = 1000;
}

// the rows of one request, checked on the host before anything is uploaded
static int check_request(qasr_cvlm* h, const qasr_cvlm_request* rq, std::vector<CvlmRow>& rows) {
    if (!h || !h->impl) return QASR_ERR_INVALID;
    const qasr_cvlm_config& c = h->impl->config();
    if (!rq) return fail(h, QASR_ERR_INVALID, WHO + ": null request");
    if (rq->B > (size_t)c.max_batch)
        return fail(h, QASR_ERR_CAPACITY, WHO + ": " + std::to_string(rq->B) + " rows, more than max_batch = " + std::to_string(c.max_batch));
    if (rq->B == 0) return QASR_OK;
    if (!rq->text || !rq->text_len) return fail(h, QASR_ERR_INVALID, WHO + ": null argument");
    for (size_t b = 0; b < rq->B; ++b) {
        const std::string row = WHO + ": row " + std::to_string(b) + ": ";
        CvlmRow r{};
        r.text = rq->text[b]; r.n_text = rq->text_len[b];
        if (!r.text) return fail(h, QASR_ERR_INVALID, row + "null text");
        if (r.n_text < 1) return fail(h, QASR_ERR_INVALID, row + "an empty text");
        if (r.n_text > c.max_text)
            return fail(h, QASR_ERR_CAPACITY, row + "text of " + std::to_string(r.n_text) + " ids, more than max_text = " + std::to_string(c.max_text));
        for (int i = 0; i < r.n_text; ++i)
            if (r.text[i] < 0 || r.text[i] >= c.text_vocab)
                return fail(h, QASR_ERR_INVALID, row + "text id " + std::to_string(r.text[i]) + " outside the text vocabulary");
        r.prompt = rq->prompt ? rq->prompt[b] : nullptr;
        r.n_prompt = r.prompt && rq->prompt_len ? rq->prompt_len[b] : 0;
        if (r.n_prompt < 0) return fail(h, QASR_ERR_INVALID, row + "negative prompt length");
        if (r.n_prompt == 0) r.prompt = nullptr;
        if (r.n_prompt > c.max_prompt_tokens)
            return fail(h, QASR_ERR_CAPACITY, row + std::to_string(r.n_prompt) + " prompt speech tokens, more than max_prompt_tokens = " + std::to_string(c.max_prompt_tokens));
        for (int i = 0; i < r.n_prompt; ++i)
            if (r.prompt[i] < 0 || r.prompt[i] >= c.speech_tokens)
                return fail(h, QASR_ERR_INVALID, row + "prompt speech token " + std::to_string(r.prompt[i]) + " outside [0, " + std::to_string(c.speech_tokens) + ")");
        r.content_len = rq->content_len && rq->content_len[b] >= 0 ? rq->content_len[b] : r.n_text;
        r.max_tokens = rq->max_tokens && rq->max_tokens[b] > 0 ? rq->max_tokens[b] : c.max_tokens;
        if (r.max_tokens > c.max_tokens)
            return fail(h, QASR_ERR_CAPACITY, row + "max_tokens " + std::to_string(r.max_tokens) + ", more than the handle's " + std::to_string(c.max_tokens));
        r.index = rq->row_index ? rq->row_index[b] : (long long)b;
        rows.push_back(r);
    }
    return QASR_OK;
}

template <class H> static int check_sampling(const H* h, const qasr_cvlm_sampling* s) {
    if (!s) return fail(h, QASR_ERR_INVALID, WHO + ": null sampling");
    if (s->win_size < 0 || s->win_size > CVLM_MAX_WIN) return fail(h, QASR_ERR_INVALID, WHO + ": win_size in 0..64");
    if (!(s->top_p > 0.0f)) return fail(h, QASR_ERR_INVALID, WHO + ": top_p must be positive");
    if (!(s->tau_r >= 0.0f) || !(s->min_ratio >= 0.0f)) return fail(h, QASR_ERR_INVALID, WHO + ": tau_r and min_ratio must not be negative");
    return QASR_OK;
}

static int open_checkpoint(const char* model_dir, const qasr_cvlm_config* cfg, std::unique_ptr<SafeTensorsDir>& st) {
    if (!model_dir || !cfg) return fail<qasr_cvlm>(nullptr, QASR_ERR_INVALID, WHO + ": model_dir or cfg is NULL");
    try { CosyLlm::check_geometry(*cfg); }
    catch (const std::exception& ex) { return fail<qasr_cvlm>(nullptr, QASR_ERR_INVALID, ex.what()); }
    try { st = std::make_unique<SafeTensorsDir>(model_dir, "llm.safetensors"); }
    catch (const std::exception& ex) { return fail<qasr_cvlm>(nullptr, QASR_ERR_IO, WHO + ": " + ex.what()); }
    return QASR_OK;
}

static int create_handle(const char* model_dir, const qasr_cvlm_config* cfg, bool host_only, qasr_cvlm** out) {
    std::unique_ptr<SafeTensorsDir> st;
    if (const int rc = open_checkpoint(model_dir, cfg, st)) return rc;
    qasr_cvlm* h = new qasr_cvlm();
    try { h->impl = std::make_unique<CosyLlm>(*cfg, *st, host_only); }
    catch (const WeightLoadError& ex) { delete h; return fail<qasr_cvlm>(nullptr, ex.code, ex.what()); }
    catch (const HipError& ex) { delete h; return fail<qasr_cvlm>(nullptr, QASR_ERR_HIP, ex.what()); }
    catch (const std::exception& ex) { delete h; return fail<qasr_cvlm>(nullptr, QASR_ERR_INVALID, ex.what()); }
    if (host_only) delete h;
    else *out = h;
    return QASR_OK;
}

extern "C" {

int qasr_cvlm_default_config(int bits, qasr_cvlm_config* out) {
    if (!out || (bits != 4 && bits != 8)) return QASR_ERR_INVALID;
    default_config(bits, out);
    return QASR_OK;
}

void qasr_cvlm_default_sampling(qasr_cvlm_sampling* out) {
    if (out) *out = qasr_cvlm_sampling{25, 0.8f, 10, 0.1f, 2.0f};
}

int qasr_cvlm_create(const char* model_dir, const qasr_cvlm_config* cfg, qasr_cvlm** out) {
    if (!out) return QASR_ERR_INVALID;
    *out = nullptr;
    return create_handle(model_dir, cfg, false, out);
}

int qasr_cvlm_check(const char* model_dir, const qasr_cvlm_config* cfg) { return create_handle(model_dir, cfg, true, nullptr); }

void qasr_cvlm_free(qasr_cvlm* h) { delete h; }
const char* qasr_cvlm_last_error(const qasr_cvlm* h) { return error_slot(h).c_str(); }
size_t qasr_cvlm_memory_footprint(const qasr_cvlm* h) { return h && h->impl ? h->impl->footprint() : 0; }
size_t qasr_cvlm_device_bytes(const qasr_cvlm* h) { return h && h->impl ? h->impl->device_bytes() : 0; }
int qasr_cvlm_poll_interval(void) { return CVLM_POLL; }

int qasr_cvlm_context(const qasr_cvlm_config* cfg) {
    if (!cfg) return -QASR_ERR_INVALID;
    try { CosyLlm::check_geometry(*cfg); }
    catch (const std::exception& ex) { return -fail<qasr_cvlm>(nullptr, QASR_ERR_INVALID, ex.what()); }
    return CosyLlm::context(*cfg);
}

int qasr_cvlm_plan_prefix(const qasr_cvlm_config* cfg, const int32_t* text, int32_t text_len, const int32_t* prompt, int32_t prompt_len,
                          int32_t* out) {
    if (!cfg || !text || !out || text_len < 1 || prompt_len < 0 || (prompt_len > 0 && !prompt)) return -QASR_ERR_INVALID;
    CvlmRow r{};
    r.text = text; r.n_text = text_len; r.prompt = prompt; r.n_prompt = prompt_len;
    const std::vector<int> p = CosyLlm::plan_prefix(*cfg, r);
    std::copy(p.begin(), p.end(), out);
    return (int)p.size();
}

int qasr_cvlm_generate(qasr_cvlm* h, const qasr_cvlm_request* rq, const qasr_cvlm_sampling* s, uint64_t seed, int32_t* tokens, int32_t* n_tokens) {
    std::vector<CvlmRow> rows;
    if (const int rc = check_request(h, rq, rows)) return rc;
    if (const int rc = check_sampling(h, s)) return rc;
    if (rows.empty()) return QASR_OK;
    if (!tokens || !n_tokens) return fail(h, QASR_ERR_INVALID, WHO + ": null argument");
    return guarded(h, [&] { h->impl->generate(rows, *s, seed, tokens, n_tokens); });
}

int qasr_cvlm_forced(qasr_cvlm* h, const qasr_cvlm_request* rq, const int32_t* tokens, size_t T, float* logits, float* hidden) {
    std::vector<CvlmRow> rows;
    if (const int rc = check_request(h, rq, rows)) return rc;
    if (rows.empty() || T == 0) return QASR_OK;
    const qasr_cvlm_config& c = h->impl->config();
    if (!tokens) return fail(h, QASR_ERR_INVALID, WHO + ": null tokens");
    if (T > (size_t)c.max_tokens) return fail(h, QASR_ERR_CAPACITY, WHO + ": " + std::to_string(T) + " forced tokens, more than max_tokens");
    const int V = h->impl->vocab();
    for (size_t b = 0; b < rows.size(); ++b)
        for (size_t i = 0; i < T; ++i) {
            const int v = tokens[b * T + i];
            if (v < 0 || v >= V)
                return fail(h, QASR_ERR_INVALID, WHO + ": row " + std::to_string(b) + ": forced token " + std::to_string(v) + " outside the speech vocabulary");
        }
    return guarded(h, [&] { h->impl->forced(rows, tokens, (int)T, logits, hidden); });
}

int qasr_cvlm_sample(qasr_cvlm* h, const float* logits, const int32_t* const* history, const int32_t* n_history, const int32_t* step,
                     const int32_t* below_min, size_t B, const qasr_cvlm_sampling* s, uint64_t seed, const int64_t* row_index, int32_t* out) {
    if (!h || !h->impl) return QASR_ERR_INVALID;
    if (const int rc = check_sampling(h, s)) return rc;
    if (B == 0) return QASR_OK;
    const qasr_cvlm_config& c = h->impl->config();
    if (B > (size_t)CVLM_PASS_ROWS) return fail(h, QASR_ERR_CAPACITY, WHO + ": " + std::to_string(B) + " rows, more than 64");
    if (!logits || !n_history || !step || !below_min || !out) return fail(h, QASR_ERR_INVALID, WHO + ": null argument");
    for (size_t b = 0; b < B; ++b) {
        const std::string row = WHO + ": row " + std::to_string(b) + ": ";
        if (n_history[b] < 0 || step[b] < 0) return fail(h, QASR_ERR_INVALID, row + "negative history length or step");
        if (n_history[b] > c.max_tokens) return fail(h, QASR_ERR_CAPACITY, row + "a history over max_tokens");
        if (n_history[b] > 0 && (!history || !history[b])) return fail(h, QASR_ERR_INVALID, row + "null history");
    }
    return guarded(h, [&] { h->impl->sample((int)B, logits, history, n_history, step, below_min, *s, seed, row_index, out); });
}

int qasr_cvlm_sample_host(const qasr_cvlm_config* cfg, const float* logits, const int32_t* history, int32_t n_history, int32_t step,
                          int below_min, const qasr_cvlm_sampling* s, uint64_t seed, int64_t row_index) {
    qasr_cvlm_config d;
    default_config(4, &d);
    const qasr_cvlm_config& c = cfg ? *cfg : d;
    if (!logits || n_history < 0 || step < 0 || (n_history > 0 && !history)) return -QASR_ERR_INVALID;
    if (c.speech_tokens < 1 || c.speech_extra < CVLM_STOPS) return -QASR_ERR_INVALID;
    if (const int rc = check_sampling<qasr_cvlm>(nullptr, s)) return -rc;
    const CvlmSampleParams p{s->top_k, s->top_p, s->win_size, s->tau_r, c.speech_tokens + c.speech_extra, c.speech_tokens, seed};
    return cvlm_sample_host(logits, p, history, n_history, step, below_min != 0, row_index);
}

int qasr_cvlm_linear_probe(qasr_cvlm* h, int32_t layer, int32_t kind, const float* x, const float* resid, size_t B, float* y) {
    if (!h || !h->impl) return QASR_ERR_INVALID;
    if (!x || !y) return fail(h, QASR_ERR_INVALID, WHO + ": null argument");
    if (B < 1 || B > (size_t)CVLM_PASS_ROWS) return fail(h, QASR_ERR_INVALID, WHO + ": B in 1..64");
    return guarded(h, [&] { h->impl->linear_probe(layer, kind, (int)B, x, resid, y); });
}

int qasr_cvlm_synthesize(qasr_cvlm* h, qasr_flow* flow, qasr_hift* hift, const qasr_cvlm_request* rq, const qasr_cvlm_sampling* s,
                         uint64_t seed, const float* const* spk_emb, const float* const* prompt_feat, const size_t* prompt_frames,
                         float* const* pcm, size_t* n_samples, int32_t* tokens, int32_t* n_tokens) {
    if (!h || !h->impl) return QASR_ERR_INVALID;
    if (!flow || !hift || !rq || !pcm || !n_samples) return fail(h, QASR_ERR_INVALID, WHO + ": null argument");
    const size_t B = rq->B, F = (size_t)h->impl->config().max_tokens;
    std::vector<int32_t> tk, nt;
    if (!tokens) { tk.resize(B * F); tokens = tk.data(); }
    if (!n_tokens) { nt.resize(B); n_tokens = nt.data(); }
    if (const int rc = qasr_cvlm_generate(h, rq, s, seed, tokens, n_tokens)) return rc;
    // the rows that have tokens, as one flow call and one vocoder call
    std::vector<size_t> live;
    for (size_t b = 0; b < B; ++b) {
        n_samples[b] = 0;
        if (n_tokens[b] > 0) live.push_back(b);
    }
    if (live.empty()) return QASR_OK;
    const size_t L = live.size();
    std::vector<const int32_t*> tp(L), pp(L);
    std::vector<size_t> tn(L), pn(L), pf_n(L), T(L);
    std::vector<const float*> pf(L), se(L), melp(L);
    std::vector<uint64_t> seeds(L);
    std::vector<std::vector<float>> mel(L), rows(L), wav(L);
    std::vector<float*> melw(L), wavw(L);
    for (size_t i = 0; i < L; ++i) {
        const size_t b = live[i];
        if (!pcm[b]) return fail(h, QASR_ERR_INVALID, WHO + ": row " + std::to_string(b) + ": null pcm buffer");
        tp[i] = tokens + b * F; tn[i] = (size_t)n_tokens[b];
        pp[i] = rq->prompt ? rq->prompt[b] : nullptr;
        pn[i] = pp[i] && rq->prompt_len ? (size_t)rq->prompt_len[b] : 0;
        if (pn[i] == 0) pp[i] = nullptr;
        pf[i] = prompt_feat ? prompt_feat[b] : nullptr;
        pf_n[i] = pf[i] && prompt_frames ? prompt_frames[b] : 0;
        if (pf_n[i] == 0) pf[i] = nullptr;
        se[i] = spk_emb ? spk_emb[b] : nullptr;
        seeds[i] = seed + (uint64_t)(rq->row_index ? rq->row_index[b] : (int64_t)b);
        T[i] = qasr_flow_mel_frames(tn[i] + pn[i]);
        mel[i].resize(80 * T[i]);
        melw[i] = mel[i].data();
    }
    if (const int rc = qasr_flow_generate_batch(flow, tp.data(), tn.data(), pp.data(), pn.data(), pf.data(), pf_n.data(), se.data(), 0, 1.0f,
                                                seeds.data(), L, nullptr, melw.data()))
        return fail(h, rc, WHO + ": flow: " + qasr_flow_last_error(flow));
    for (size_t i = 0; i < L; ++i) {                       // [80][T] -> the [T][80] the vocoder takes
        rows[i].resize(T[i] * 80);
        for (size_t t = 0; t < T[i]; ++t)
            for (size_t m = 0; m < 80; ++m) rows[i][t * 80 + m] = mel[i][m * T[i] + t];
        melp[i] = rows[i].data();
        wav[i].resize(qasr_hift_num_samples(T[i]));
        wavw[i] = wav[i].data();
    }
    if (const int rc = qasr_hift_decode_batch(hift, melp.data(), T.data(), seeds.data(), L, wavw.data()))
        return fail(h, rc, WHO + ": vocoder: " + qasr_hift_last_error(hift));
    for (size_t i = 0; i < L; ++i) {
        const size_t b = live[i], cut = 480 * pf_n[i];    // the prompt region is rendered and then dropped (CosyVoiceTTS.swift:311-318)
        const size_t from = cut > 0 && cut < wav[i].size() ? cut : 0;
        n_samples[b] = wav[i].size() - from;
        std::memcpy(pcm[b], wav[i].data() + from, n_samples[b] * sizeof(float));
    }
    return QASR_OK;
}

}  // extern "C"
