// tts_sampler.cpp -- host twin of the Qwen3-TTS device sampler (tts_talker.hip: tts_sample_kernel), the same arithmetic step by step:
// sampleToken / sampleTokenLazy of Sources/Qwen3TTS/Sampling.swift:36-160 with the project's counter-based splitmix64 stream in place of
// MLX's generator.  tests/test_talker_cpu.py holds it against a numpy restatement, tests/test_gpu_talker.py against the device.
#include "tts_talker.h"
#include <algorithm>
#include <cmath>
#include <functional>

namespace qasr {

int tts_sample_host(const float* logits, int V, const TtsSampleParams& p, const unsigned char* seen, long long row, int frame, int group) {
    std::vector<float> v(logits, logits + V);
    const bool talker = p.eos >= 0;
    if (talker) {
        // 1. the suppress range to -1e9, except EOS
        for (int i = std::max(p.suppress_lo, 0); i < std::min(p.suppress_hi, V); ++i)
            if (i != p.eos) v[i] = -1e9f;
        // 2. sign-aware repetition penalty over the distinct history
        if (p.repetition_penalty != 1.0f && seen)
            for (int i = 0; i < V; ++i)
                if (seen[i]) v[i] = v[i] < 0.0f ? v[i] * p.repetition_penalty : v[i] / p.repetition_penalty;
    }
    auto first_max = [&](const std::vector<float>& a) {
        int best = 0;
        for (int i = 1; i < V; ++i)
            if (a[i] > a[best]) best = i;
        return best;
    };
    // 3. greedy
    if (p.temperature <= 0.0f) return first_max(v);
    // 4. temperature
    for (int i = 0; i < V; ++i) v[i] = v[i] / p.temperature;
    // 5. the EOS logit is kept aside
    const bool eos_ok = talker && p.eos < V;
    const float eos_saved = eos_ok ? v[p.eos] : 0.0f;
    // 6. top-k: the threshold is the k-th largest value, ties with it survive
    if (p.top_k > 0 && p.top_k < V) {
        std::vector<float> s(v);
        std::nth_element(s.begin(), s.begin() + (p.top_k - 1), s.end(), std::greater<float>());
        const float thr = s[p.top_k - 1];
        for (int i = 0; i < V; ++i)
            if (v[i] < thr) v[i] = -1e9f;
    }
    // 7. EOS back, with its bias
    if (eos_ok) v[p.eos] = p.eos_logit_bias != 0.0f ? eos_saved + p.eos_logit_bias : eos_saved;
    // 8. Gumbel-max
    const unsigned long long key = tts_stream_key(p.seed, row, frame, group);
    for (int i = 0; i < V; ++i) v[i] = v[i] - logf(-logf(tts_uniform(key, i)));
    return first_max(v);
}

}  // namespace qasr
