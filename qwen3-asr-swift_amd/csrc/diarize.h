// diarize.h -- host logic of the pyannote VAD and diarization pipelines (diarize.cpp), in f32 and in the reference's operation order:
// sample ranges and threshold decisions depend on it.  Pure CPU; the C ABI over it is in api_seg.cpp and diarize.cpp.
#pragma once
#include "qasr.h"
#include "seg_pyannote.h"
#include <memory>
#include <string>
#include <utility>
#include <vector>

struct qasr_seg {
    std::unique_ptr<qasr::SegPyannote> impl;
    mutable std::string last_error;
};
std::string& error_slot(const qasr_seg* s);

namespace qasr {

constexpr int SEG_WINDOW = 160000, SEG_FRAMES = 589;        // the pipelines' 10 s window and its frame count

struct SegSpan { float start, end; };
// VADPipeline.windowPositions (VADPipeline.swift:37-60) = DiarizationPipeline.swift:319-332
std::vector<std::pair<long, long>> seg_window_positions(size_t n_samples, size_t window, size_t step);
// VADPipeline.aggregateFrames (:74-106)
std::vector<float> seg_aggregate_frames(const float* probs, size_t W, size_t frames, const long* starts, size_t n_samples, int sample_rate,
                                        float frame_duration);
// PowersetDecoder.binarize (PowersetDecoder.swift:44-72); filter: VADPipeline.binarize's filterDurations (VADPipeline.swift:150-180)
std::vector<SegSpan> seg_binarize(const float* probs, size_t n, size_t stride, float onset, float offset, float frame_duration);
std::vector<SegSpan> seg_filter_durations(const std::vector<SegSpan>& s, float min_speech, float min_silence);

float diar_cosine_distance(const float* a, const float* b, size_t n);
// constrainedAgglomerativeClustering (DiarizationHelpers.swift:83-164): the number of clusters; centroids [clusters][dim]
int diar_cluster(const float* emb, const int32_t* window, size_t n, size_t dim, float threshold, int32_t* assignment,
                 std::vector<float>& centroids);
std::vector<qasr_diar_segment> diar_merge_segments(const std::vector<qasr_diar_segment>& s, float min_silence);
void diar_compact_speaker_ids(qasr_diar_segment* s, size_t n);

}  // namespace qasr
