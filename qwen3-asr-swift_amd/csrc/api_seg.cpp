// api_seg.cpp -- extern "C" boundary of the pyannote segmentation model and the pyannote VAD (include/qasr.h, qasr_seg_*).  Exceptions
// never cross it.  The diarization pipeline over it is in diarize.cpp.
#include "api_guard.h"
#include "diarize.h"
#include <cmath>

std::string& error_slot(const qasr_seg* s) { return s ? s->last_error : create_error<qasr_seg>(); }

using namespace qasr;

static int write_spans(const std::vector<SegSpan>& s, float* out, size_t cap) {
    for (size_t i = 0; i < s.size() && i < cap; ++i) { out[2 * i] = s[i].start; out[2 * i + 1] = s[i].end; }
    return (int)s.size();
}

extern "C" {

int qasr_seg_vad_default_config(qasr_seg_vad_config* out) {
    if (!out) return QASR_ERR_INVALID;
    out->onset = 0.767f; out->offset = 0.377f; out->min_speech_duration = 0.136f; out->min_silence_duration = 0.067f;
    out->window_duration = 10.0f; out->step_ratio = 0.1f;
    return QASR_OK;
}

int qasr_seg_create(int device, const char* model_dir, int max_windows, qasr_engine* order_with, qasr_seg** out) {
    if (!out) return QASR_ERR_INVALID;
    *out = nullptr;
    if (!model_dir) return fail<qasr_seg>(nullptr, QASR_ERR_INVALID, "pyannote segmentation: model_dir is NULL");
    if (max_windows == 0) max_windows = 64;
    if (max_windows < 0 || max_windows > 4096) return fail<qasr_seg>(nullptr, QASR_ERR_INVALID, "pyannote segmentation: max_windows in 1..4096 (0 = 64)");
    if (order_with && (!order_with->impl || order_with->impl->config().device != device))
        return fail<qasr_seg>(nullptr, QASR_ERR_INVALID, "pyannote segmentation: order_with must be an engine on the same device");
    CheckedWeights w;
    try { w = load_checked_f32(model_dir, "pyannote segmentation", seg_tensor_shapes(), true, seg_optional_default); }   // no HIP call yet
    catch (const WeightLoadError& ex) { return fail<qasr_seg>(nullptr, ex.code, ex.what()); }
    catch (const std::exception& ex) { return fail<qasr_seg>(nullptr, QASR_ERR_IO, ex.what()); }
    return guarded_create(out, QASR_ERR_INVALID, [&](qasr_seg* s) {
        s->impl = std::make_unique<SegPyannote>(device, w, max_windows, order_with ? order_with->impl->stream() : nullptr);
    });
}

void qasr_seg_destroy(qasr_seg* s) { delete s; }
const char* qasr_seg_last_error(const qasr_seg* s) { return error_slot(s).c_str(); }
int qasr_seg_is_loaded(const qasr_seg* s) { return s && s->impl && s->impl->loaded() ? 1 : 0; }
int qasr_seg_unload(qasr_seg* s) {
    if (!s || !s->impl) return QASR_ERR_INVALID;
    return guarded(s, [&] { s->impl->unload(); });
}
size_t qasr_seg_memory_footprint(const qasr_seg* s) { return s && s->impl ? s->impl->footprint() : 0; }
int qasr_seg_num_frames(size_t n) { return seg_num_frames(n); }
int qasr_seg_timing(const qasr_seg* s, float* ms) {
    if (!s || !s->impl) return QASR_ERR_INVALID;
    if (ms) *ms = s->impl->last_ms();
    return QASR_OK;
}

int qasr_seg_forward(qasr_seg* s, const float* pcm, size_t B, size_t n, float* posteriors, float* speaker_probs, float* speech_probs) {
    if (!s || !s->impl) return QASR_ERR_INVALID;
    if (!s->impl->loaded()) return fail(s, QASR_ERR_NOT_LOADED, "pyannote segmentation: model unloaded");
    if (n < (size_t)SEG_MIN_SAMPLES) return fail(s, QASR_ERR_INVALID, "pyannote segmentation: fewer than 991 samples give no frame");
    if (B == 0) return QASR_OK;
    if (!pcm) return fail(s, QASR_ERR_INVALID, "pyannote segmentation: null argument");
    return guarded(s, [&] {
        std::vector<long> starts(B);
        for (size_t b = 0; b < B; ++b) starts[b] = (long)(b * n);
        s->impl->run(pcm, B * n, starts.data(), B, n, posteriors, speaker_probs, speech_probs);
    });
}

int qasr_seg_window_positions(size_t n_samples, size_t window_samples, size_t step_samples, int64_t* starts, int64_t* ends, size_t cap) {
    if (window_samples == 0 || step_samples == 0) return -QASR_ERR_INVALID;
    try {
        const auto pos = seg_window_positions(n_samples, window_samples, step_samples);
        for (size_t i = 0; i < pos.size() && i < cap; ++i) {
            if (starts) starts[i] = pos[i].first;
            if (ends) ends[i] = pos[i].second;
        }
        return (int)pos.size();
    } catch (...) { return -QASR_ERR_INVALID; }
}

int qasr_seg_windows(qasr_seg* s, const float* pcm, size_t n_samples, size_t window_samples, size_t step_samples, float* posteriors,
                     float* speaker_probs, float* speech_probs, int64_t* starts, int64_t* ends, size_t cap) {
    if (!s || !s->impl) return -QASR_ERR_INVALID;
    if (!s->impl->loaded()) return -fail(s, QASR_ERR_NOT_LOADED, "pyannote segmentation: model unloaded");
    if (step_samples == 0 || window_samples < (size_t)SEG_MIN_SAMPLES)
        return -fail(s, QASR_ERR_INVALID, "pyannote segmentation: window of at least 991 samples and a positive step");
    if (!pcm && n_samples) return -fail(s, QASR_ERR_INVALID, "pyannote segmentation: null argument");
    int count = 0;
    const int rc = guarded(s, [&] {
        const auto pos = seg_window_positions(n_samples, window_samples, step_samples);
        count = (int)pos.size();
        if (pos.size() > cap) throw std::length_error("pyannote segmentation: more windows than the caller's capacity");
        std::vector<long> st(pos.size());
        for (size_t i = 0; i < pos.size(); ++i) {
            st[i] = pos[i].first;
            if (starts) starts[i] = pos[i].first;
            if (ends) ends[i] = pos[i].second;
        }
        s->impl->run(pcm, n_samples, st.data(), pos.size(), window_samples, posteriors, speaker_probs, speech_probs);
    });
    return rc == QASR_OK ? count : -rc;
}

int qasr_seg_aggregate_frames(const float* window_probs, size_t n_windows, size_t frames_per_window, const int64_t* starts, size_t n_samples,
                              int sample_rate, float window_duration, float* out, size_t cap) {
    if (sample_rate <= 0 || frames_per_window == 0 || (n_windows && (!window_probs || !starts)) || (!out && cap)) return -QASR_ERR_INVALID;
    try {
        std::vector<long> st(starts, starts + n_windows);
        const auto a = seg_aggregate_frames(window_probs, n_windows, frames_per_window, st.data(), n_samples, sample_rate,
                                            window_duration / (float)frames_per_window);
        for (size_t i = 0; i < a.size() && i < cap; ++i) out[i] = a[i];
        return (int)a.size();
    } catch (...) { return -QASR_ERR_INVALID; }
}

int qasr_seg_binarize(const float* probs, size_t n, float frame_duration, const qasr_vad_config* cfg, int filter_durations, float* segments,
                      size_t cap) {
    if ((!probs && n) || (!segments && cap) || !cfg) return -QASR_ERR_INVALID;
    try {
        auto s = seg_binarize(probs, n, 1, cfg->onset, cfg->offset, frame_duration);
        if (filter_durations) s = seg_filter_durations(s, cfg->min_speech_duration, cfg->min_silence_duration);
        return write_spans(s, segments, cap);
    } catch (...) { return -QASR_ERR_INVALID; }
}

int qasr_seg_detect_speech(qasr_seg* s, const float* pcm, size_t n, int sample_rate, const qasr_seg_vad_config* cfg, float* segments,
                           size_t cap) {
    if (!s || !s->impl) return -QASR_ERR_INVALID;
    if (sample_rate != SEG_RATE)
        return -fail(s, QASR_ERR_UNSUPPORTED, "pyannote vad: 16 kHz input only (the reference resamples with AVAudioConverter)");
    if ((!pcm && n) || (!segments && cap)) return -fail(s, QASR_ERR_INVALID, "pyannote vad: null argument");
    qasr_seg_vad_config c;
    qasr_seg_vad_default_config(&c);
    if (cfg) c = *cfg;
    // VADPipeline.windowPositions (VADPipeline.swift:38-39) in f32
    const long window = (long)(c.window_duration * (float)SEG_RATE), step = (long)(c.window_duration * c.step_ratio * (float)SEG_RATE);
    if (window < SEG_MIN_SAMPLES || step <= 0) return -fail(s, QASR_ERR_INVALID, "pyannote vad: window or step too small");
    if (n == 0) return 0;
    int out = 0;
    const int rc = guarded(s, [&] {
        const auto pos = seg_window_positions(n, (size_t)window, (size_t)step);
        std::vector<long> st(pos.size());
        for (size_t i = 0; i < pos.size(); ++i) st[i] = pos[i].first;
        const int frames = seg_num_frames((size_t)window);
        std::vector<float> speech(pos.size() * (size_t)frames);
        s->impl->run(pcm, n, st.data(), pos.size(), (size_t)window, nullptr, nullptr, speech.data());
        // SpeechVAD.swift:97-101 fixes framesPerChunk = 589 for the frame duration, whatever the window gives
        const float frame_duration = c.window_duration / (float)SEG_FRAMES;
        const auto agg = seg_aggregate_frames(speech.data(), pos.size(), (size_t)frames, st.data(), n, SEG_RATE, frame_duration);
        auto sp = seg_binarize(agg.data(), agg.size(), 1, c.onset, c.offset, frame_duration);
        out = write_spans(seg_filter_durations(sp, c.min_speech_duration, c.min_silence_duration), segments, cap);
    });
    return rc == QASR_OK ? out : -rc;
}

}  // extern "C"
