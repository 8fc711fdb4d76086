// cvlm_sampler.cpp -- host twin of the CosyVoice3 LLM's device sampler (llm_cosyvoice.hip: cvlm_sample_kernel), the same arithmetic step
// by step: sampleToken / nucleusSample of Sources/CosyVoiceTTS/LLM.swift:12-123 with the project's counter-based splitmix64 stream
// (tts_talker.h) in place of MLX's generator.  tests/test_cvlm_cpu.py holds it against a numpy restatement, tests/test_gpu_cvlm.py
// against the device.
#include "llm_cosyvoice.h"
#include <algorithm>
#include <cmath>
#include <functional>

namespace qasr {

static bool is_stop(int i, int st) { return i >= st && i < st + CVLM_STOPS; }

// logit i after steps 1 and 2
static float masked(float v, int i, int st, int V, bool mask_stops) {
    if (i >= st && i < V && !is_stop(i, st)) v = -1e9f;                                                                 // 1
    if (mask_stops && is_stop(i, st)) v = -1e9f;                                                                        // 2
    return v;
}

static int first_max(const std::vector<float>& a) {
    int best = 0;
    for (int i = 1; i < (int)a.size(); ++i)
        if (a[i] > a[best]) best = i;
    return best;
}

int cvlm_sample_host(const float* logits, const CvlmSampleParams& p, const int32_t* history, int n_history, int step, bool below_min,
                     long long row) {
    const int V = p.V, ST = p.speech_tokens;
    const bool mask_stops = below_min || step == 0;
    std::vector<float> v(V);
    for (int i = 0; i < V; ++i) v[i] = masked(logits[i], i, ST, V, mask_stops);
    // 3. top-k: the threshold is the k-th largest value, ties with it survive
    if (p.top_k > 0 && p.top_k < V) {
        std::vector<float> s(v);
        std::nth_element(s.begin(), s.begin() + (p.top_k - 1), s.end(), std::greater<float>());
        const float thr = s[p.top_k - 1];
        for (int i = 0; i < V; ++i)
            if (v[i] < thr) v[i] = -1e9f;
    }
    // 4. top-p over the survivors in (value descending, index ascending) order, the sums added one by one in f32
    if (p.top_p < 1.0f) {
        std::vector<int> idx;
        for (int i = 0; i < V; ++i)
            if (v[i] > -1e9f) idx.push_back(i);
        std::sort(idx.begin(), idx.end(), [&](int a, int b) { return v[a] > v[b] || (v[a] == v[b] && a < b); });
        const int n = (int)idx.size();
        if (n > 0) {
            const float mx = v[idx[0]];
            float S = 0.0f;
            for (int e = 0; e < n; ++e) S += expf(v[idx[e]] - mx);
            float cum = 0.0f;
            std::vector<int> drop;
            for (int e = 0; e < n; ++e) {
                const float pr = expf(v[idx[e]] - mx) / S;
                cum += pr;
                if (cum - pr > p.top_p) drop.push_back(idx[e]);
            }
            for (int i : drop) v[i] = -1e9f;
        }
    }
    // 5. Gumbel-max, draw 0
    int tok;
    {
        const unsigned long long key = tts_stream_key(p.seed, row, step, 0);
        std::vector<float> g(V);
        for (int i = 0; i < V; ++i) g[i] = v[i] - logf(-logf(tts_uniform(key, i)));
        tok = first_max(g);
    }
    // 6. repetition-aware resample, draw 1: the logits as they were after steps 1 and 2, the pick masked
    if (p.win_size > 0 && n_history > 0) {
        const int win = std::min(p.win_size, n_history);
        int cnt = 0;
        for (int i = 0; i < win; ++i) cnt += history[n_history - win + i] == tok ? 1 : 0;
        if (cnt >= cvlm_ras_threshold(p.win_size, p.tau_r)) {
            const unsigned long long key = tts_stream_key(p.seed, row, step, 1);
            std::vector<float> g(V);
            for (int i = 0; i < V; ++i) {
                float x = masked(logits[i], i, ST, V, mask_stops);
                if (i == tok) x = -1e9f;
                g[i] = x - logf(-logf(tts_uniform(key, i)));
            }
            tok = first_max(g);
        }
    }
    return tok;
}

}  // namespace qasr
