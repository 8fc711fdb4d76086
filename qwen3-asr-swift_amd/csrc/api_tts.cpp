// api_tts.cpp -- extern "C" boundary of the Qwen3-TTS Talker + code predictor (include/qasr.h, qasr_tts_*).  Exceptions never cross it.
#include "api_guard.h"
#include "codec_qwen3tts.h"
#include "tts_talker.h"
#include <chrono>
#include <climits>
#include <memory>

struct qasr_tts {
    std::unique_ptr<qasr::TtsTalker> impl;
    mutable std::string last_error;
    qasr_tts_pool* pool = nullptr;       // the stream pool that owns the handle's rows, if any
};
static std::string& error_slot(const qasr_tts* t) { return t ? t->last_error : create_error<qasr_tts>(); }

// One stream of a pool = one batch row (slot) of the Talker.  frames: what the device has stored, emitted: what went out in chunks.
struct TtsStream {
    enum { FREE, QUEUED, RUNNING } state = FREE;
    qasr_tts_stream_config sc{};
    int frames = 0, emitted = 0, cap = 0;
    qasr::TtsRow row{};                  // points into the copies below
    std::vector<int32_t> text, instruct;
    std::vector<float> xvector;
};
struct qasr_tts_pool {
    qasr_tts* t = nullptr;
    qasr_codec* codec = nullptr;
    int max_tokens = 0;
    std::vector<TtsStream> streams;      // [max_batch]
    std::vector<float> pcm;              // the chunks of the last step
    std::vector<int32_t> chunk_codes, window_codes;
    float timing[3] = {0, 0, 0};         // host ms of the last step: admission, frames (with the polls and code reads), codec
    mutable std::string last_error;
};
static std::string& error_slot(const qasr_tts_pool* p) { return p ? p->last_error : create_error<qasr_tts_pool>(); }

using namespace qasr;

static const std::string WHO = "talker";

// the rows of one request, checked on the host before anything is uploaded
static int check_request(qasr_tts* t, const qasr_tts_request* rq, std::vector<TtsRow>& rows, bool one_shot = true) {
    if (!t || !t->impl) return QASR_ERR_INVALID;
    if (one_shot && t->pool)
        return fail(t, QASR_ERR_INVALID, WHO + ": a stream pool owns this handle's rows (qasr_tts_pool_destroy it before a one-shot call)");
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

// the ICL side of a request (qasr_tts_icl), checked against the handle's capacity and the code tables; fills the rows' ICL fields
static int check_icl(qasr_tts* t, const qasr_tts_icl* icl, std::vector<TtsRow>& rows) {
    if (rows.empty()) return QASR_OK;
    const qasr_tts_config& c = t->impl->config();
    const int cap_f = t->impl->max_ref_frames(), cap_t = t->impl->max_ref_text();
    if (!icl || !icl->ref_codes || !icl->ref_frames || !icl->ref_text_len) return fail(t, QASR_ERR_INVALID, WHO + ": null ICL argument");
    for (size_t b = 0; b < rows.size(); ++b) {
        const std::string row = WHO + ": row " + std::to_string(b) + ": ";
        TtsRow& r = rows[b];
        if (!r.xvector) return fail(t, QASR_ERR_INVALID, row + "an ICL row needs an x-vector");
        if (r.speaker >= 0) return fail(t, QASR_ERR_INVALID, row + "a speaker token on an ICL call");
        if (r.n_instruct > 0) return fail(t, QASR_ERR_INVALID, row + "an instruct prefix on an ICL call");
        r.n_ref_text = icl->ref_text_len[b];
        r.ref_text = icl->ref_text ? icl->ref_text[b] : nullptr;
        r.ref_frames = icl->ref_frames[b];
        r.ref_codes = icl->ref_codes[b];
        if (r.n_ref_text < 0) return fail(t, QASR_ERR_INVALID, row + "negative reference text length");
        if (r.ref_frames < 1) return fail(t, QASR_ERR_INVALID, row + "an ICL row needs at least 1 reference frame");
        if (r.ref_frames > cap_f)
            return fail(t, QASR_ERR_CAPACITY, row + std::to_string(r.ref_frames) + " reference frames, more than max_ref_frames = " + std::to_string(cap_f));
        if (r.n_ref_text > cap_t)
            return fail(t, QASR_ERR_CAPACITY, row + "reference text of " + std::to_string(r.n_ref_text) + " ids, more than max_ref_text = " + std::to_string(cap_t));
        if (!r.ref_codes || (r.n_ref_text > 0 && !r.ref_text)) return fail(t, QASR_ERR_INVALID, row + "null reference codes or text");
        for (int i = 0; i < r.n_ref_text; ++i)
            if (r.ref_text[i] < 0 || r.ref_text[i] >= c.text_vocab)
                return fail(t, QASR_ERR_INVALID, row + "reference text id " + std::to_string(r.ref_text[i]) + " outside the text vocabulary");
        for (int g = 0; g < TTS_GROUPS; ++g)
            for (int f = 0; f < r.ref_frames; ++f) {
                const int v = r.ref_codes[(size_t)g * r.ref_frames + f];
                if (v < 0 || v >= (g == 0 ? c.codec_vocab : c.cp_vocab))
                    return fail(t, QASR_ERR_INVALID, row + "reference code " + std::to_string(v) + " of stream " + std::to_string(g) + " outside its table");
            }
    }
    return QASR_OK;
}

static int check_forced_codes(qasr_tts* t, size_t B, const int32_t* codes, size_t T) {
    const qasr_tts_config& c = t->impl->config();
    if (!codes) return fail(t, QASR_ERR_INVALID, WHO + ": null codes");
    if (T > (size_t)c.max_frames) return fail(t, QASR_ERR_CAPACITY, WHO + ": " + std::to_string(T) + " forced frames, more than max_frames");
    for (size_t b = 0; b < B; ++b)
        for (int g = 0; g < TTS_GROUPS; ++g)
            for (size_t i = 0; i < T; ++i) {
                const int v = codes[(b * TTS_GROUPS + g) * T + i];
                if (v < 0 || v >= (g == 0 ? c.codec_vocab : c.cp_vocab))
                    return fail(t, QASR_ERR_INVALID, WHO + ": forced code " + std::to_string(v) + " of stream " + std::to_string(g) + " outside its vocabulary");
            }
    return QASR_OK;
}

static int create_handle(const char* model_dir, const qasr_tts_config* cfg, bool icl, int max_ref_frames, int max_ref_text, qasr_tts** out) {
    if (!out) return QASR_ERR_INVALID;
    *out = nullptr;
    if (!model_dir || !cfg) return fail<qasr_tts>(nullptr, QASR_ERR_INVALID, WHO + ": model_dir or cfg is NULL");
    try {
        TtsTalker::check_geometry(*cfg);
        if (icl) (void)TtsTalker::icl_context(*cfg, max_ref_frames, max_ref_text);
    } catch (const std::exception& ex) { return fail<qasr_tts>(nullptr, QASR_ERR_INVALID, ex.what()); }
    std::unique_ptr<SafeTensorsDir> st;            // all *.safetensors of the directory (TTSWeightLoading.swift:24-30); other keys are not read
    try { st = std::make_unique<SafeTensorsDir>(model_dir); }
    catch (const std::exception& ex) { return fail<qasr_tts>(nullptr, QASR_ERR_IO, WHO + ": " + ex.what()); }
    qasr_tts* h = new qasr_tts();
    try { h->impl = std::make_unique<TtsTalker>(*cfg, *st, icl ? max_ref_frames : 0, icl ? max_ref_text : 0); }
    catch (const WeightLoadError& ex) { delete h; return fail<qasr_tts>(nullptr, ex.code, ex.what()); }
    catch (const HipError& ex) { delete h; return fail<qasr_tts>(nullptr, QASR_ERR_HIP, ex.what()); }
    catch (const std::exception& ex) { delete h; return fail<qasr_tts>(nullptr, QASR_ERR_INVALID, ex.what()); }
    *out = h;
    return QASR_OK;
}

// codes [B][16][max_frames] of a generate call -> pcm through the caller's codec handle
static int decode_rows(qasr_tts* t, qasr_codec* codec, size_t B, const int32_t* codes, const int32_t* n_frames, float* const* pcm, size_t* n_samples) {
    const size_t F = (size_t)t->impl->config().max_frames, spf = (size_t)qasr_codec_samples_per_frame();
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

static int check_sampling(qasr_tts* t, const qasr_tts_sampling* s) {
    if (!s) return fail(t, QASR_ERR_INVALID, WHO + ": null sampling");
    if (s->top_p < 1.0f)
        return fail(t, QASR_ERR_UNSUPPORTED, WHO + ": top_p < 1 is not served (the reference's branch masks the likeliest tokens; DESIGN.md section 18)");
    if (!(s->repetition_penalty > 0.0f)) return fail(t, QASR_ERR_INVALID, WHO + ": repetition_penalty must be positive");
    return QASR_OK;
}


// ---- the stream pool ------------------------------------------------------------------------------------------
// the chunks of a stream, stated once: the pool cuts by next_boundary() and the final rules of stream_chunks()
static int next_boundary(const qasr_tts_stream_config& sc, int emitted) { return emitted == 0 ? sc.first_chunk_frames : emitted + sc.chunk_frames; }

struct ChunkSpan { int frame_index, frames, is_final; };
static std::vector<ChunkSpan> stream_chunks(int n, bool eos, const qasr_tts_stream_config& sc) {
    std::vector<ChunkSpan> out;
    int emitted = 0;
    // a boundary the stream reached and went on from; the one it stopped on at max_tokens is its final chunk
    for (int b = next_boundary(sc, 0); b < n || (b == n && eos); b = next_boundary(sc, emitted)) {
        out.push_back({emitted, b - emitted, 0});
        emitted = b;
    }
    if (eos || n > emitted) out.push_back({emitted, n - emitted, 1});       // at EOS with nothing left: the empty final chunk
    return out;
}

static int check_stream_config(qasr_tts_pool* p, const qasr_tts_stream_config* sc) {
    if (!sc) return fail(p, QASR_ERR_INVALID, WHO + ": null stream config");
    if (sc->first_chunk_frames < 1) return fail(p, QASR_ERR_INVALID, WHO + ": first_chunk_frames must be at least 1");
    if (sc->chunk_frames < 1) return fail(p, QASR_ERR_INVALID, WHO + ": chunk_frames must be at least 1");
    if (sc->decoder_left_context < 0) return fail(p, QASR_ERR_INVALID, WHO + ": decoder_left_context must not be negative");
    if (sc->first_chunk_frames > CODEC_MAX_T)
        return fail(p, QASR_ERR_UNSUPPORTED, WHO + ": first_chunk_frames over the codec's window of " + std::to_string(CODEC_MAX_T) + " frames");
    if ((long)sc->decoder_left_context + sc->chunk_frames > CODEC_MAX_T)
        return fail(p, QASR_ERR_UNSUPPORTED, WHO + ": decoder_left_context + chunk_frames over the codec's window of " + std::to_string(CODEC_MAX_T) +
                                                 " frames (the noChunking preset: use qasr_tts_synthesize)");
    return QASR_OK;
}

// one chunk of slot `slot`: its codes through the host, its window queued for the codec pass
struct DueChunk { int slot, frame_index, frames, is_final; size_t codes_at, pcm_at, win_at; int win_frames; };

static int pool_step(qasr_tts_pool* p, qasr_tts_chunk* chunks, size_t cap, size_t* n_out) {
    TtsTalker& tk = *p->t->impl;
    const int MB = (int)p->streams.size(), spf = qasr_codec_samples_per_frame();
    if ((size_t)qasr_tts_pool_live(p) > cap)
        return fail(p, QASR_ERR_CAPACITY, WHO + ": " + std::to_string(qasr_tts_pool_live(p)) + " live streams may each send a chunk, cap is " + std::to_string(cap));
    std::vector<DueChunk> due;
    std::vector<int> frames(MB), fin(MB);
    using Clock = std::chrono::steady_clock;
    auto ms_since = [](Clock::time_point t0) { return std::chrono::duration<float, std::milli>(Clock::now() - t0).count(); };
    Clock::time_point t0 = Clock::now();
    p->timing[0] = p->timing[1] = p->timing[2] = 0.0f;
    int rc = guarded(p, [&] {
        for (int b = 0; b < MB; ++b) {                                       // 1. admission
            TtsStream& st = p->streams[b];
            if (st.state != TtsStream::QUEUED) continue;
            tk.pool_admit(b, st.row);
            st.state = TtsStream::RUNNING;
        }
        p->timing[0] = ms_since(t0);
        t0 = Clock::now();
        while (due.empty()) {
            int B = 0, run = INT_MAX;                                      // 2. 3. frames up to the nearest boundary of any stream
            for (int b = 0; b < MB; ++b) {
                const TtsStream& st = p->streams[b];
                if (st.state != TtsStream::RUNNING) continue;
                B = b + 1;
                run = std::min(run, std::min(next_boundary(st.sc, st.emitted), st.cap) - st.frames);
            }
            if (B == 0) return;
            bool stop = false;
            for (int f = 0; f < run && !stop; f += TTS_POLL) {              // 4. the counts and flags every TTS_POLL frames
                tk.pool_frames(B, std::min(TTS_POLL, run - f));
                tk.pool_poll(B, frames.data(), fin.data());
                for (int b = 0; b < B; ++b) stop = stop || (p->streams[b].state == TtsStream::RUNNING && fin[b]);
            }
            // a stream already on its boundary: the step before failed behind its frames (a codec or HIP error) and its chunk is still owed
            if (run <= 0) tk.pool_poll(B, frames.data(), fin.data());
            for (int b = 0; b < B; ++b) {
                TtsStream& st = p->streams[b];
                if (st.state != TtsStream::RUNNING) continue;
                st.frames = frames[b];
                const bool eos = fin[b] != 0, capped = !eos && st.frames >= st.cap;
                if (!eos && !capped && st.frames < next_boundary(st.sc, st.emitted)) continue;
                due.push_back({b, st.emitted, st.frames - st.emitted, eos || capped ? 1 : 0, 0, 0, 0, 0});
                if (capped) tk.pool_finish(b);                                // before another frame runs
            }
        }
        // 5. the codes of every due chunk and of its left context, [zero pad | context | chunk] per window
        size_t n_codes = 0, n_pcm = 0, n_win = 0;
        for (DueChunk& d : due) {
            const int ctx = std::min(p->streams[d.slot].sc.decoder_left_context, d.frame_index);
            d.win_frames = d.frames > 0 ? std::max(ctx + d.frames, 4) : 0;
            d.codes_at = n_codes; d.pcm_at = n_pcm; d.win_at = n_win;
            n_codes += (size_t)TTS_GROUPS * d.frames; n_pcm += (size_t)spf * d.frames; n_win += (size_t)TTS_GROUPS * d.win_frames;
        }
        p->chunk_codes.assign(n_codes, 0); p->pcm.assign(n_pcm, 0.0f); p->window_codes.assign(n_win, 0);
        for (const DueChunk& d : due) {
            if (d.frames == 0) continue;
            const int real = std::min(p->streams[d.slot].sc.decoder_left_context, d.frame_index) + d.frames, W = d.win_frames;
            std::vector<int32_t> got((size_t)TTS_GROUPS * real);
            tk.pool_codes(d.slot, d.frame_index + d.frames - real, real, got.data());
            for (int g = 0; g < TTS_GROUPS; ++g) {
                std::copy_n(&got[(size_t)g * real], real, &p->window_codes[d.win_at + (size_t)g * W + (W - real)]);
                std::copy_n(&got[(size_t)g * real + (real - d.frames)], d.frames, &p->chunk_codes[d.codes_at + (size_t)g * d.frames]);
            }
        }
        p->timing[1] = ms_since(t0);
    });
    if (rc) return rc;
    t0 = Clock::now();
    std::vector<CodecWin> wins;
    for (const DueChunk& d : due)
        if (d.frames > 0)
            wins.push_back({&p->window_codes[d.win_at], (long)d.win_frames, 0, d.win_frames, d.win_frames - d.frames, &p->pcm[d.pcm_at]});
    if (int crc = codec_run_windows(p->codec, wins, true)) return fail(p, crc, WHO + ": codec: " + qasr_codec_last_error(p->codec));
    p->timing[2] = ms_since(t0);
    for (size_t i = 0; i < due.size(); ++i) {
        const DueChunk& d = due[i];
        chunks[i] = qasr_tts_chunk{d.slot, d.frame_index, d.frames, d.is_final, d.frames ? &p->pcm[d.pcm_at] : nullptr, (size_t)spf * d.frames,
                                   d.frames ? &p->chunk_codes[d.codes_at] : nullptr};
        TtsStream& st = p->streams[d.slot];
        st.emitted += d.frames;
        if (d.is_final) st = TtsStream{};                                    // the slot is free for the next open
    }
    *n_out = due.size();
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

void qasr_tts_default_stream_config(int preset, qasr_tts_stream_config* out) {
    if (out) *out = preset == 1 ? qasr_tts_stream_config{1, 15, 10} : qasr_tts_stream_config{3, 25, 10};     // StreamingConfig.lowLatency | .default
}

int64_t qasr_tts_stream_chunks(int32_t n_frames, int ended_by_eos, const qasr_tts_stream_config* sc, int32_t* frame_index, int32_t* frames,
                               int32_t* is_final, size_t cap) {
    if (!sc || sc->first_chunk_frames < 1 || sc->chunk_frames < 1 || n_frames < 0 || (!ended_by_eos && n_frames < 1)) return -QASR_ERR_INVALID;
    const auto spans = stream_chunks(n_frames, ended_by_eos != 0, *sc);
    if (spans.size() > cap) return -QASR_ERR_CAPACITY;
    for (size_t i = 0; i < spans.size(); ++i) {
        if (frame_index) frame_index[i] = spans[i].frame_index;
        if (frames) frames[i] = spans[i].frames;
        if (is_final) is_final[i] = spans[i].is_final;
    }
    return (int64_t)spans.size();
}

int qasr_tts_pool_create(qasr_tts* t, qasr_codec* codec, const qasr_tts_sampling* s, uint64_t seed, qasr_tts_pool** out) {
    if (!t || !t->impl) return QASR_ERR_INVALID;
    if (!out) return fail(t, QASR_ERR_INVALID, WHO + ": null argument");
    *out = nullptr;
    if (!codec) return fail(t, QASR_ERR_INVALID, WHO + ": null argument");
    if (t->pool) return fail(t, QASR_ERR_INVALID, WHO + ": the handle already has a stream pool");
    if (int rc = check_sampling(t, s)) return rc;
    if (int rc = guarded(t, [&] { t->impl->pool_begin(*s, seed); })) return rc;
    qasr_tts_pool* p = new qasr_tts_pool();
    p->t = t; p->codec = codec; p->max_tokens = s->max_tokens;
    p->streams.resize(t->impl->config().max_batch);
    t->pool = p;
    *out = p;
    return QASR_OK;
}

void qasr_tts_pool_destroy(qasr_tts_pool* p) {
    if (!p) return;
    for (size_t b = 0; b < p->streams.size(); ++b) (void)qasr_tts_pool_close(p, (int32_t)b);
    p->t->pool = nullptr;
    delete p;
}

const char* qasr_tts_pool_last_error(const qasr_tts_pool* p) { return error_slot(p).c_str(); }

int qasr_tts_pool_live(const qasr_tts_pool* p) {
    int n = 0;
    if (p) for (const TtsStream& st : p->streams) n += st.state != TtsStream::FREE;
    return n;
}

int qasr_tts_pool_open(qasr_tts_pool* p, const qasr_tts_request* rq, const qasr_tts_stream_config* sc, int32_t* stream) {
    if (!p) return QASR_ERR_INVALID;
    if (!stream) return fail(p, QASR_ERR_INVALID, WHO + ": null argument");
    if (int rc = check_stream_config(p, sc)) return rc;
    if (rq && rq->B != 1) return fail(p, QASR_ERR_INVALID, WHO + ": a stream is one row: B must be 1, got " + std::to_string(rq->B));
    std::vector<TtsRow> rows;
    if (int rc = check_request(p->t, rq, rows, false)) return fail(p, rc, qasr_tts_last_error(p->t));
    size_t slot = 0;
    while (slot < p->streams.size() && p->streams[slot].state != TtsStream::FREE) ++slot;
    if (slot == p->streams.size())
        return fail(p, QASR_ERR_CAPACITY, WHO + ": no free slot: all " + std::to_string(slot) + " streams (max_batch) are live");
    const int H = p->t->impl->config().hidden, F = p->t->impl->config().max_frames;
    TtsStream& st = p->streams[slot];
    st = TtsStream{};
    st.state = TtsStream::QUEUED;
    st.sc = *sc;
    st.cap = p->max_tokens > 0 && p->max_tokens < F ? p->max_tokens : F;
    st.row = rows[0];
    st.text.assign(st.row.text, st.row.text + st.row.n_text);
    st.row.text = st.text.data();
    if (st.row.n_instruct > 0) { st.instruct.assign(st.row.instruct, st.row.instruct + st.row.n_instruct); st.row.instruct = st.instruct.data(); }
    if (st.row.xvector) { st.xvector.assign(st.row.xvector, st.row.xvector + H); st.row.xvector = st.xvector.data(); }
    *stream = (int32_t)slot;
    return QASR_OK;
}

int qasr_tts_pool_step(qasr_tts_pool* p, qasr_tts_chunk* chunks, size_t cap, size_t* n) {
    if (!p) return QASR_ERR_INVALID;
    if (!n || (cap > 0 && !chunks)) return fail(p, QASR_ERR_INVALID, WHO + ": null argument");
    *n = 0;
    return pool_step(p, chunks, cap, n);
}

int qasr_tts_pool_timing(const qasr_tts_pool* p, float* ms) {
    if (!p || !ms) return QASR_ERR_INVALID;
    std::memcpy(ms, p->timing, sizeof(p->timing));
    return QASR_OK;
}

int qasr_tts_pool_close(qasr_tts_pool* p, int32_t stream) {
    if (!p) return QASR_ERR_INVALID;
    if (stream < 0 || (size_t)stream >= p->streams.size()) return fail(p, QASR_ERR_INVALID, WHO + ": stream " + std::to_string(stream) + " outside the pool");
    TtsStream& st = p->streams[stream];
    int rc = QASR_OK;
    if (st.state == TtsStream::RUNNING) rc = guarded(p, [&] { p->t->impl->pool_finish(stream); });
    st = TtsStream{};
    return rc;
}

int qasr_tts_create(const char* model_dir, const qasr_tts_config* cfg, qasr_tts** out) {
    return create_handle(model_dir, cfg, false, 0, 0, out);
}

int qasr_tts_create_icl(const char* model_dir, const qasr_tts_config* cfg, int32_t max_ref_frames, int32_t max_ref_text, qasr_tts** out) {
    return create_handle(model_dir, cfg, true, max_ref_frames, max_ref_text, out);
}

int qasr_tts_icl_capacity(const qasr_tts* t, int32_t* max_ref_frames, int32_t* max_ref_text) {
    if (!t || !t->impl) return QASR_ERR_INVALID;
    if (max_ref_frames) *max_ref_frames = t->impl->max_ref_frames();
    if (max_ref_text) *max_ref_text = t->impl->max_ref_text();
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
    if (int rc = check_forced_codes(t, rows.size(), codes, T)) return rc;
    TtsForcedOut f{codes, (int)T, talker_logits, cp_logits, hidden};
    return guarded(t, [&] { t->impl->forced(rows, f); });
}

int qasr_tts_generate_icl(qasr_tts* t, const qasr_tts_request* rq, const qasr_tts_icl* icl, const qasr_tts_sampling* s, uint64_t seed,
                          int32_t* codes, int32_t* n_frames) {
    std::vector<TtsRow> rows;
    if (int rc = check_request(t, rq, rows)) return rc;
    if (int rc = check_icl(t, icl, rows)) return rc;
    if (int rc = check_sampling(t, s)) return rc;
    if (rows.empty()) return QASR_OK;
    if (!codes || !n_frames) return fail(t, QASR_ERR_INVALID, WHO + ": null output");
    const int cap = t->impl->config().max_frames;
    const int frames = s->max_tokens > 0 && s->max_tokens < cap ? s->max_tokens : cap;
    return guarded(t, [&] { t->impl->generate(rows, *s, seed, frames, codes, n_frames); });
}

int qasr_tts_forced_icl(qasr_tts* t, const qasr_tts_request* rq, const qasr_tts_icl* icl, const int32_t* codes, size_t T, float* talker_logits,
                        float* cp_logits, float* hidden) {
    std::vector<TtsRow> rows;
    if (int rc = check_request(t, rq, rows)) return rc;
    if (int rc = check_icl(t, icl, rows)) return rc;
    if (rows.empty() || T == 0) return QASR_OK;
    if (int rc = check_forced_codes(t, rows.size(), codes, T)) return rc;
    TtsForcedOut f{codes, (int)T, talker_logits, cp_logits, hidden};
    return guarded(t, [&] { t->impl->forced(rows, f); });
}

int qasr_tts_icl_prompt(qasr_tts* t, const qasr_tts_request* rq, const qasr_tts_icl* icl, float* rows_out, int32_t* P) {
    std::vector<TtsRow> rows;
    if (int rc = check_request(t, rq, rows)) return rc;
    if (int rc = check_icl(t, icl, rows)) return rc;
    if (rows.empty()) return QASR_OK;
    if (!rows_out || !P) return fail(t, QASR_ERR_INVALID, WHO + ": null output");
    return guarded(t, [&] { t->impl->icl_prompt(rows, rows_out, P); });
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
    return decode_rows(t, codec, B, codes, n_frames, pcm, n_samples);
}

int qasr_tts_synthesize_icl(qasr_tts* t, qasr_codec* codec, const qasr_tts_request* rq, const qasr_tts_icl* icl, const qasr_tts_sampling* s,
                            uint64_t seed, float* const* pcm, size_t* n_samples, int32_t* codes, int32_t* n_frames) {
    if (!t || !t->impl) return QASR_ERR_INVALID;
    if (!codec || !rq || !pcm || !n_samples) return fail(t, QASR_ERR_INVALID, WHO + ": null argument");
    const size_t B = rq->B, F = (size_t)t->impl->config().max_frames;
    std::vector<int32_t> own_codes, own_frames;
    if (!codes) { own_codes.resize(B * TTS_GROUPS * F); codes = own_codes.data(); }
    if (!n_frames) { own_frames.resize(B); n_frames = own_frames.data(); }
    if (int rc = qasr_tts_generate_icl(t, rq, icl, s, seed, codes, n_frames)) return rc;
    return decode_rows(t, codec, B, codes, n_frames, pcm, n_samples);
}

// synthesizeWithVoiceCloneICL (Qwen3TTS+ICL.swift:49-145) for B rows: codes and x-vector of every reference clip, then the ICL call
int qasr_tts_clone(qasr_tts* t, qasr_codec_enc* codec_enc, qasr_xvec* xvec, qasr_codec* codec, const qasr_tts_request* rq,
                   const int32_t* const* ref_text, const int32_t* ref_text_len, const float* const* ref_pcm, const size_t* ref_n,
                   const qasr_tts_sampling* s, uint64_t seed, float* const* pcm, size_t* n_samples, int32_t* codes, int32_t* n_frames) {
    if (!t || !t->impl) return QASR_ERR_INVALID;
    if (!codec_enc || !xvec || !codec || !rq || !ref_pcm || !ref_n || !ref_text_len) return fail(t, QASR_ERR_INVALID, WHO + ": null argument");
    const size_t B = rq->B;
    const int H = t->impl->config().hidden, E = qasr_xvec_embedding_dim(xvec);
    if (E != H)
        return fail(t, QASR_ERR_INVALID, WHO + ": the speaker encoder's embedding holds " + std::to_string(E) + " floats, the Talker's hidden size is " + std::to_string(H));
    if (B > (size_t)t->impl->config().max_batch)
        return fail(t, QASR_ERR_CAPACITY, WHO + ": " + std::to_string(B) + " rows, more than max_batch = " + std::to_string(t->impl->config().max_batch));
    if (B == 0) return QASR_OK;
    std::vector<std::vector<int32_t>> rc_store(B);
    std::vector<int32_t*> rc_ptr(B);
    std::vector<const int32_t*> rc_cptr(B);
    std::vector<int32_t> frames(B);
    for (size_t b = 0; b < B; ++b) {
        const std::string row = WHO + ": row " + std::to_string(b) + ": ";
        if (!ref_pcm[b] || ref_n[b] == 0) return fail(t, QASR_ERR_INVALID, row + "empty reference clip");
        const size_t f = qasr_codec_enc_num_frames(ref_n[b]);
        if (f > (size_t)t->impl->max_ref_frames())
            return fail(t, QASR_ERR_CAPACITY, row + std::to_string(f) + " reference frames, more than max_ref_frames = " + std::to_string(t->impl->max_ref_frames()));
        frames[b] = (int32_t)f;
        rc_store[b].resize(TTS_GROUPS * f);
        rc_ptr[b] = rc_store[b].data();
        rc_cptr[b] = rc_store[b].data();
    }
    if (qasr_codec_enc_num_quantizers(codec_enc) != TTS_GROUPS) return fail(t, QASR_ERR_INVALID, WHO + ": the speech tokenizer encoder does not write 16 code streams");
    if (int rc = qasr_codec_enc_encode_batch(codec_enc, ref_pcm, ref_n, B, rc_ptr.data()))
        return fail(t, rc, WHO + ": codec encoder: " + qasr_codec_enc_last_error(codec_enc));
    std::vector<float> xv(B * (size_t)H);
    if (int rc = qasr_xvec_embed_batch(xvec, ref_pcm, ref_n, B, xv.data())) return fail(t, rc, WHO + ": speaker encoder: " + qasr_xvec_last_error(xvec));
    std::vector<const float*> xp(B);
    for (size_t b = 0; b < B; ++b) xp[b] = xv.data() + b * (size_t)H;
    qasr_tts_request q = *rq;
    q.xvector = xp.data();
    qasr_tts_icl icl{ref_text, ref_text_len, rc_cptr.data(), frames.data()};
    return qasr_tts_synthesize_icl(t, codec, &q, &icl, s, seed, pcm, n_samples, codes, n_frames);
}

}  // extern "C"
