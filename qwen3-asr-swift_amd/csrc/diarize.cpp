// diarize.cpp -- PyannoteDiarizationPipeline.diarize / extractSpeaker (Sources/SpeechVAD/DiarizationPipeline.swift) and the helpers of
// DiarizationHelpers.swift, VADPipeline.swift and PowersetDecoder.swift on the host, behind the C ABI (include/qasr.h).  Every time and
// index expression is computed in float in the reference's order.  The device work goes through qasr_seg_windows (every window of the
// file in one call) and ONE qasr_spk_embed_batch (every solo-speaker clip of the file).  Exceptions never cross the boundary.
#include "api_guard.h"
#include "diarize.h"
#include <algorithm>
#include <cmath>
#include <map>
#include <set>

namespace qasr {

std::vector<std::pair<long, long>> seg_window_positions(size_t n_samples, size_t window, size_t step) {
    std::vector<std::pair<long, long>> pos;
    if (n_samples == 0) return pos;
    if (n_samples <= window) { pos.push_back({0, (long)n_samples}); return pos; }      // one zero-padded window
    for (size_t start = 0; start + window <= n_samples; start += step) pos.push_back({(long)start, (long)(start + window)});
    if (pos.empty() || (size_t)pos.back().second < n_samples) pos.push_back({(long)(n_samples - window), (long)n_samples});
    return pos;
}

std::vector<float> seg_aggregate_frames(const float* probs, size_t W, size_t frames, const long* starts, size_t n_samples, int sample_rate,
                                        float frame_duration) {
    const float total = (float)n_samples / (float)sample_rate;
    const long num = (long)std::ceil(total / frame_duration);
    std::vector<float> out;
    if (num <= 0) return out;
    std::vector<float> sum((size_t)num, 0.0f), cnt((size_t)num, 0.0f);
    for (size_t w = 0; w < W; ++w) {
        const float t0 = (float)starts[w] / (float)sample_rate;
        for (size_t f = 0; f < frames; ++f) {
            const float time = t0 + (float)f * frame_duration;
            const long gf = (long)(time / frame_duration);             // Int(frameTime / frameDuration), f32
            if (gf >= 0 && gf < num) { sum[(size_t)gf] += probs[w * frames + f]; cnt[(size_t)gf] += 1.0f; }
        }
    }
    out.resize((size_t)num);
    for (long i = 0; i < num; ++i) out[(size_t)i] = cnt[(size_t)i] > 0.0f ? sum[(size_t)i] / cnt[(size_t)i] : 0.0f;
    return out;
}

std::vector<SegSpan> seg_binarize(const float* probs, size_t n, size_t stride, float onset, float offset, float frame_duration) {
    std::vector<SegSpan> segs;
    bool in = false;
    float start = 0.0f;
    for (size_t i = 0; i < n; ++i) {
        const float time = (float)i * frame_duration, p = probs[i * stride];
        if (!in && p >= onset) { in = true; start = time; }
        else if (in && p < offset) { in = false; segs.push_back({start, time}); }
    }
    if (in) segs.push_back({start, (float)n * frame_duration});
    return segs;
}

std::vector<SegSpan> seg_filter_durations(const std::vector<SegSpan>& s, float min_speech, float min_silence) {
    std::vector<SegSpan> kept, merged;
    for (const auto& x : s) if (x.end - x.start >= min_speech) kept.push_back(x);
    if (kept.empty()) return merged;
    SegSpan cur = kept[0];
    for (size_t i = 1; i < kept.size(); ++i) {
        if (kept[i].start - cur.end < min_silence) cur.end = kept[i].end;
        else { merged.push_back(cur); cur = kept[i]; }
    }
    merged.push_back(cur);
    return merged;
}

float diar_cosine_distance(const float* a, const float* b, size_t n) {
    if (n == 0) return 2.0f;
    float dot = 0.0f, na = 0.0f, nb = 0.0f;
    for (size_t i = 0; i < n; ++i) { dot += a[i] * b[i]; na += a[i] * a[i]; nb += b[i] * b[i]; }
    const float den = std::sqrt(na) * std::sqrt(nb);
    if (!(den > 1e-10f)) return 2.0f;
    return 1.0f - dot / den;
}

int diar_cluster(const float* emb, const int32_t* window, size_t n, size_t dim, float threshold, int32_t* assignment,
                 std::vector<float>& centroids) {
    centroids.clear();
    if (n == 0) return 0;
    std::vector<std::vector<float>> cen(n);
    for (size_t i = 0; i < n; ++i) cen[i].assign(emb + i * dim, emb + (i + 1) * dim);
    std::vector<int> of(n);
    std::vector<std::vector<int>> members(n);
    std::vector<std::set<int32_t>> wins(n);
    std::set<int> active;
    for (size_t i = 0; i < n; ++i) { of[i] = (int)i; members[i] = {(int)i}; wins[i] = {window[i]}; active.insert((int)i); }
    while (n > 1 && active.size() > 1) {
        float best = 3.402823466e+38f;
        int bi = -1, bj = -1;
        const std::vector<int> list(active.begin(), active.end());      // sorted
        for (size_t ai = 0; ai < list.size(); ++ai)
            for (size_t aj = ai + 1; aj < list.size(); ++aj) {
                const int ci = list[ai], cj = list[aj];
                bool shared = false;                                        // same-window constraint
                for (int32_t x : wins[cj]) if (wins[ci].count(x)) { shared = true; break; }
                if (shared) continue;
                const float d = diar_cosine_distance(cen[ci].data(), cen[cj].data(), dim);
                if (d < best) { best = d; bi = ci; bj = cj; }             // first-found minimum
            }
        if (!(best < threshold) || bi < 0) break;
        const float si = (float)members[bi].size(), sj = (float)members[bj].size(), tot = (float)(members[bi].size() + members[bj].size());
        for (size_t d = 0; d < dim; ++d) cen[bi][d] = (cen[bi][d] * si + cen[bj][d] * sj) / tot;
        for (int m : members[bj]) of[m] = bi;
        members[bi].insert(members[bi].end(), members[bj].begin(), members[bj].end());
        wins[bi].insert(wins[bj].begin(), wins[bj].end());
        active.erase(bj);
    }
    std::map<int, int> compact;
    for (int old : active) { const int id = (int)compact.size(); compact[old] = id; }
    for (size_t i = 0; i < n; ++i) assignment[i] = compact[of[i]];
    for (int old : active) centroids.insert(centroids.end(), cen[old].begin(), cen[old].end());
    return (int)active.size();
}

// Swift's sort is not specified as stable and bySpeaker is a Dictionary: here speakers are visited in ascending id and every sort is
// stable, which fixes the order of segments that start at the same time.
static bool by_start(const qasr_diar_segment& a, const qasr_diar_segment& b) { return a.start_time < b.start_time; }

std::vector<qasr_diar_segment> diar_merge_segments(const std::vector<qasr_diar_segment>& s, float min_silence) {
    std::vector<qasr_diar_segment> merged;
    if (s.empty()) return merged;
    std::map<int32_t, std::vector<qasr_diar_segment>> by;
    for (const auto& x : s) by[x.speaker_id].push_back(x);
    for (auto& kv : by) {
        auto& v = kv.second;
        std::stable_sort(v.begin(), v.end(), by_start);
        qasr_diar_segment cur = v[0];
        for (size_t i = 1; i < v.size(); ++i) {
            if (v[i].start_time - cur.end_time < min_silence) cur.end_time = v[i].end_time;
            else { merged.push_back(cur); cur = v[i]; }
        }
        merged.push_back(cur);
    }
    std::stable_sort(merged.begin(), merged.end(), by_start);
    return merged;
}

void diar_compact_speaker_ids(qasr_diar_segment* s, size_t n) {
    std::set<int32_t> used;
    for (size_t i = 0; i < n; ++i) used.insert(s[i].speaker_id);
    std::map<int32_t, int32_t> m;
    for (int32_t id : used) { const int32_t k = (int32_t)m.size(); m[id] = k; }
    for (size_t i = 0; i < n; ++i) s[i].speaker_id = m[s[i].speaker_id];
}

// trimToSpeechMask (DiarizationPipeline.swift:540-565)
static bool trim_to_mask(float start, float end, const std::vector<SegSpan>& mask, float min_duration, SegSpan* out) {
    const float dur = end - start;
    if (!(dur > 0.0f)) return false;
    float overlap = 0.0f, ts = end, te = start;
    for (const auto& v : mask) {
        const float os = std::max(start, v.start), oe = std::min(end, v.end);
        if (os < oe) { overlap += oe - os; ts = std::min(ts, os); te = std::max(te, oe); }
    }
    if (!(overlap / dur >= 0.5f) || !(te - ts >= min_duration)) return false;
    *out = {ts, te};
    return true;
}

}  // namespace qasr

struct qasr_diar_result {
    std::vector<qasr_diar_segment> segments;
    int num_speakers = 0;
    std::vector<float> embeddings;                     // [num_speakers][256]
};

using namespace qasr;

static qasr_diar_config diar_cfg(const qasr_diar_config* c) {
    qasr_diar_config d;
    qasr_diar_default_config(&d);
    return c ? *c : d;
}

// runEmbeddingClusteredDiarization (DiarizationPipeline.swift:301-537)
static int diarize_impl(qasr_seg* seg, qasr_spk* spk, qasr_vad* vad, const float* pcm, size_t n, const qasr_diar_config& cfg,
                        qasr_diar_result* res) {
    const int rate = SEG_RATE;
    std::vector<SegSpan> mask;
    if (vad) {                                         // stage 0: Silero pre-filter on stream 0 (:218-232)
        std::vector<float> buf(2 * (n / 512 + 2));
        const int c = qasr_vad_detect_speech(vad, pcm, n, rate, nullptr, buf.data(), buf.size() / 2);
        if (c < 0) return fail(seg, -c, std::string("diarize: silero pre-filter: ") + qasr_vad_last_error(vad));
        if (c == 0) return QASR_OK;
        for (int i = 0; i < c; ++i) mask.push_back({buf[2 * i], buf[2 * i + 1]});
    }
    if (n == 0) return QASR_OK;
    const float window_duration = 10.0f;
    const long window_samples = (long)(window_duration * (float)rate);
    const int frames = SEG_FRAMES;
    const float frame_duration = window_duration / (float)frames;
    const auto pos = seg_window_positions(n, (size_t)window_samples, (size_t)(window_samples / 2));
    const size_t W = pos.size();
    std::vector<float> sp(W * frames * SEG_SPK);
    std::vector<int64_t> st(W), en(W);
    const int wc = qasr_seg_windows(seg, pcm, n, (size_t)window_samples, (size_t)(window_samples / 2), nullptr, sp.data(), nullptr, st.data(),
                                    en.data(), W);
    if (wc < 0) return -wc;
    if ((size_t)wc != W) return fail(seg, QASR_ERR_INVALID, "diarize: window count mismatch");

    // step 2: per (window, local speaker) the audio of the frames where only that speaker is at or above `offset` (:369-428)
    const size_t min_clip = (size_t)(rate / 2);
    std::vector<float> audio;
    std::vector<size_t> clip_off, clip_len;
    std::vector<int32_t> clip_win, clip_spk;
    std::vector<std::vector<SegSpan>> binar(W * SEG_SPK);
    for (size_t w = 0; w < W; ++w) {
        const float* tr = sp.data() + w * frames * SEG_SPK;
        for (int ls = 0; ls < SEG_SPK; ++ls) {
            auto& bs = binar[w * SEG_SPK + ls];
            bs = seg_binarize(tr + ls, frames, SEG_SPK, cfg.onset, cfg.offset, frame_duration);
            if (bs.empty()) continue;
            const size_t begin = audio.size();
            for (const auto& s : bs) {
                const long f0 = (long)(s.start / frame_duration), f1 = std::min((long)(s.end / frame_duration), (long)frames);
                for (long f = f0; f < f1; ++f) {
                    bool other = false;
                    for (int os = 0; os < SEG_SPK; ++os)
                        if (os != ls && tr[f * SEG_SPK + os] >= cfg.offset) { other = true; break; }
                    if (other) continue;
                    const long a = pos[w].first + (long)((float)f * frame_duration * (float)rate);
                    const long b = std::min(pos[w].first + (long)((float)(f + 1) * frame_duration * (float)rate), (long)n);
                    if (b > a) audio.insert(audio.end(), pcm + a, pcm + b);
                }
            }
            const size_t len = audio.size() - begin;
            if (len < min_clip) { audio.resize(begin); continue; }
            clip_off.push_back(begin); clip_len.push_back(len); clip_win.push_back((int32_t)w); clip_spk.push_back(ls);
        }
    }
    const size_t C = clip_off.size();
    if (C == 0) return QASR_OK;
    const int dim = qasr_spk_embedding_dim();
    std::vector<float> emb(C * dim);
    {
        std::vector<const float*> ptr(C);
        for (size_t i = 0; i < C; ++i) ptr[i] = audio.data() + clip_off[i];
        const int rc = qasr_spk_embed_batch(spk, ptr.data(), clip_len.data(), C, emb.data());      // every clip of the file in one call
        if (rc != QASR_OK) return fail(seg, rc, std::string("diarize: speaker embedding: ") + qasr_spk_last_error(spk));
    }
    // step 3: constrained clustering (:435-450)
    std::vector<int32_t> assign(C);
    std::vector<float> centroids;
    const int n_clusters = diar_cluster(emb.data(), clip_win.data(), C, (size_t)dim, cfg.clustering_threshold, assign.data(), centroids);
    std::map<std::pair<int32_t, int32_t>, int32_t> local_to_global;
    for (size_t i = 0; i < C; ++i) local_to_global[{clip_win[i], clip_spk[i]}] = assign[i];

    // step 4: segments with global ids, centre-zone ownership, optional mask (:452-509)
    std::vector<qasr_diar_segment> segs;
    for (size_t w = 0; w < W; ++w) {
        const float ws = (float)pos[w].first / (float)rate, we = (float)pos[w].second / (float)rate;
        const float prev_end = w > 0 ? (float)pos[w - 1].second / (float)rate : 0.0f;
        const float next_start = w + 1 < W ? (float)pos[w + 1].first / (float)rate : (float)n / (float)rate;
        const float own_start = w > 0 ? (ws + prev_end) / 2.0f : 0.0f;
        const float own_end = w + 1 < W ? (we + next_start) / 2.0f : (float)n / (float)rate;
        for (int ls = 0; ls < SEG_SPK; ++ls) {
            auto it = local_to_global.find({(int32_t)w, ls});
            if (it == local_to_global.end()) continue;
            for (const auto& s : binar[w * SEG_SPK + ls]) {
                const float abs_start = ws + s.start, abs_end = std::min(ws + s.end, we);
                const float cs = std::max(abs_start, own_start), ce = std::min(abs_end, own_end);
                if (!(ce - cs >= cfg.min_speech_duration)) continue;
                if (vad) {
                    SegSpan t;
                    if (trim_to_mask(cs, ce, mask, cfg.min_speech_duration, &t)) segs.push_back({t.start, t.end, it->second});
                } else {
                    segs.push_back({cs, ce, it->second});
                }
            }
        }
    }
    std::stable_sort(segs.begin(), segs.end(), by_start);
    diar_compact_speaker_ids(segs.data(), segs.size());
    res->segments = diar_merge_segments(segs, cfg.min_silence_duration);
    std::set<int32_t> ids;
    for (const auto& s : res->segments) ids.insert(s.speaker_id);
    res->num_speakers = (int)ids.size();
    // centroids truncated or zero-padded to num_speakers (:519-530)
    res->embeddings.assign((size_t)res->num_speakers * dim, 0.0f);
    const size_t keep = (size_t)std::min(res->num_speakers, n_clusters) * dim;
    std::copy(centroids.begin(), centroids.begin() + keep, res->embeddings.begin());
    return QASR_OK;
}

extern "C" {

int qasr_diar_default_config(qasr_diar_config* out) {
    if (!out) return QASR_ERR_INVALID;
    out->onset = 0.5f; out->offset = 0.3f; out->min_speech_duration = 0.3f; out->min_silence_duration = 0.15f;
    out->clustering_threshold = 0.715f;
    return QASR_OK;
}

float qasr_diar_cosine_distance(const float* a, const float* b, size_t n) {
    if (!a || !b) return 2.0f;
    return diar_cosine_distance(a, b, n);
}

int qasr_diar_cluster(const float* embeddings, const int32_t* window_index, size_t n, size_t dim, float threshold, int32_t* assignment,
                      float* centroids) {
    if (n == 0) return 0;
    if (!embeddings || !window_index || !assignment || dim == 0) return -QASR_ERR_INVALID;
    try {
        std::vector<float> cen;
        const int k = diar_cluster(embeddings, window_index, n, dim, threshold, assignment, cen);
        if (centroids) std::copy(cen.begin(), cen.end(), centroids);
        return k;
    } catch (...) { return -QASR_ERR_INVALID; }
}

int qasr_diar_merge_segments(const qasr_diar_segment* in, size_t n, float min_silence, qasr_diar_segment* out) {
    if (n == 0) return 0;
    if (!in || !out) return -QASR_ERR_INVALID;
    try {
        const auto m = diar_merge_segments(std::vector<qasr_diar_segment>(in, in + n), min_silence);
        std::copy(m.begin(), m.end(), out);
        return (int)m.size();
    } catch (...) { return -QASR_ERR_INVALID; }
}

int qasr_diar_compact_speaker_ids(qasr_diar_segment* segments, size_t n) {
    if (n == 0) return QASR_OK;
    if (!segments) return QASR_ERR_INVALID;
    try { diar_compact_speaker_ids(segments, n); return QASR_OK; } catch (...) { return QASR_ERR_INVALID; }
}

int qasr_diarize(qasr_seg* seg, qasr_spk* spk, qasr_vad* vad, const float* pcm, size_t n, int sample_rate, const qasr_diar_config* cfg,
                 qasr_diar_result** out) {
    if (!seg || !seg->impl) return QASR_ERR_INVALID;
    if (!out) return fail(seg, QASR_ERR_INVALID, "diarize: null result pointer");
    *out = nullptr;
    if (!spk) return fail(seg, QASR_ERR_INVALID, "diarize: a speaker embedding model is required");
    if (sample_rate != SEG_RATE)
        return fail(seg, QASR_ERR_UNSUPPORTED, "diarize: 16 kHz input only (the reference resamples with AVAudioConverter)");
    if (!pcm && n) return fail(seg, QASR_ERR_INVALID, "diarize: null audio");
    if (n > ((size_t)1 << 31)) return fail(seg, QASR_ERR_CAPACITY, "diarize: more than 2^31 samples");
    auto res = std::make_unique<qasr_diar_result>();
    int rc = QASR_OK;
    const int g = guarded(seg, [&] { rc = diarize_impl(seg, spk, vad, pcm, n, diar_cfg(cfg), res.get()); });
    if (g != QASR_OK) return g;
    if (rc != QASR_OK) return rc;
    *out = res.release();
    return QASR_OK;
}

const qasr_diar_segment* qasr_diar_result_segments(const qasr_diar_result* r, size_t* count) {
    if (count) *count = r ? r->segments.size() : 0;
    return r ? r->segments.data() : nullptr;
}
int qasr_diar_result_num_speakers(const qasr_diar_result* r) { return r ? r->num_speakers : 0; }
const float* qasr_diar_result_embeddings(const qasr_diar_result* r) { return r ? r->embeddings.data() : nullptr; }
void qasr_diar_result_free(qasr_diar_result* r) { delete r; }

int qasr_diar_extract_speaker(const qasr_diar_result* r, const float* target, float* segments, size_t cap) {
    if (!r || !target || (!segments && cap)) return -QASR_ERR_INVALID;
    if (r->num_speakers <= 0) return 0;
    const size_t dim = (size_t)qasr_spk_embedding_dim();
    int best = 0;
    float best_sim = -1.0f;                            // DiarizationPipeline.swift:261-271
    for (int i = 0; i < r->num_speakers; ++i) {
        const float sim = qasr_spk_cosine_similarity(r->embeddings.data() + (size_t)i * dim, target, dim);
        if (sim > best_sim) { best_sim = sim; best = i; }
    }
    size_t c = 0;
    for (const auto& s : r->segments)
        if (s.speaker_id == best) {
            if (c < cap) { segments[2 * c] = s.start_time; segments[2 * c + 1] = s.end_time; }
            ++c;
        }
    return (int)c;
}

}  // extern "C"
