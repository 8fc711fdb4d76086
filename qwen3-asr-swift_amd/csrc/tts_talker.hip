// tts_talker.hip -- the Qwen3-TTS Talker and code predictor (declarations and references: tts_talker.h).
//
// A frame for all rows is one linear sequence of launches on one stream, captured once per batch size and replayed per frame; what
// changes between calls (sampling values, seed) lives in a device-side Knobs record, what changes between frames (position, frame
// index, finished flags) in per-row device state.  New kernels of this file: the code predictor's attention over its <= 16 cached
// positions (the frame's K / V of a head staged in LDS), the sampler (with the gather of the next code-predictor input fused behind
// the pick), the embedding sum that builds the next Talker input, the prefill embedding builder, and a wave-per-column quantised
// GEMV with f32 output for the heads and the biased projections.  The layer GEMVs and the Talker's attention are the decode step's.
#include "tts_talker.h"
#include "sample_dev.h"
#include <algorithm>
#include <cmath>
#include <cstring>

namespace qasr {

struct TtsState { int *ctx_len, *finished, *n_frames, *frame_of, *trail_len, *pf_len; };
struct TtsTalker::Knobs { TtsSampleParams talker, cp; };

// ------------------------------------------------------------------------------------------------
// y[r][n] = act(sum_g (scale * sum q x + bias * sum x) + b[n]): one wave per output column, eight batch rows per workgroup share the
// decoded weights.  A lane owns the 8-element chunks lane, lane + 64, ... of the row (chunk c lies in group c / 8) and adds
// scale * dot + bias * xsum of each to its f32 partial; the 64 partials are summed by wave_sum.  The order does not depend on R.
// ------------------------------------------------------------------------------------------------
template <bool SILU>
__global__ __launch_bounds__(256) void tts_gemv_rows_kernel(QuantRaw q, const bf16_t* __restrict__ X, int R, const float* __restrict__ bias,
                                                            float* __restrict__ outf, bf16_t* __restrict__ outb, long ldo) {
    const int lane = threadIdx.x & 63, n = blockIdx.x * 4 + (threadIdx.x >> 6), r0 = blockIdx.y * 8;
    if (n >= q.N) return;
    const int nch = q.K / 8, G = q.K / 64;
    float acc[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) acc[r] = 0.0f;
    for (int c = lane; c < nch; c += 64) {
        unsigned e[8];
        if (q.bits == 4) {
            const uint32_t w = q.wq[(long)n * nch + c];
#pragma unroll
            for (int j = 0; j < 8; ++j) e[j] = (w >> (4 * j)) & 0xFu;
        } else {
            const uint2 w = *reinterpret_cast<const uint2*>(q.wq + (long)n * (q.K / 4) + 2 * c);
#pragma unroll
            for (int j = 0; j < 4; ++j) { e[j] = (w.x >> (8 * j)) & 0xFFu; e[4 + j] = (w.y >> (8 * j)) & 0xFFu; }
        }
        const long gi = (long)n * G + (c >> 3);
        const float s = q.sb_f32 ? reinterpret_cast<const float*>(q.scales)[gi] : bf16_to_f32(reinterpret_cast<const bf16_t*>(q.scales)[gi]);
        const float b = q.sb_f32 ? reinterpret_cast<const float*>(q.biases)[gi] : bf16_to_f32(reinterpret_cast<const bf16_t*>(q.biases)[gi]);
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            if (r0 + r >= R) break;
            const uint4 xv = *reinterpret_cast<const uint4*>(X + (long)(r0 + r) * q.K + (long)c * 8);
            const bf16_t* xe = reinterpret_cast<const bf16_t*>(&xv);
            float dot = 0.0f, xs = 0.0f;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float x = bf16_to_f32(xe[j]);
                dot = fmaf((float)e[j], x, dot);
                xs += x;
            }
            acc[r] += s * dot + b * xs;
        }
    }
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        if (r0 + r >= R) break;
        float v = wave_sum(acc[r]);
        if (lane == 0) {
            if (bias) v += bias[n];
            if (SILU) v = v / (1.0f + expf(-v));
            if (outf) outf[(long)(r0 + r) * ldo + n] = v;
            else outb[(long)(r0 + r) * ldo + n] = f32_to_bf16(v);
        }
    }
}

static void gemv_rows(const QuantRaw& q, const bf16_t* X, int R, const float* bias, float* outf, bf16_t* outb, long ldo, bool silu,
                      hipStream_t s) {
    if (R <= 0) return;
    const dim3 grid(cdiv(q.N, 4), cdiv(R, 8));
    if (silu) hipLaunchKernelGGL(tts_gemv_rows_kernel<true>, grid, dim3(256), 0, s, q, X, R, bias, outf, outb, ldo);
    else hipLaunchKernelGGL(tts_gemv_rows_kernel<false>, grid, dim3(256), 0, s, q, X, R, bias, outf, outb, ldo);
}

// ------------------------------------------------------------------------------------------------
// Code-predictor attention at position pos (0 .. 15) of the frame: one wave per (kv head, batch row).  The head's cached keys and values
// of positions < pos go to LDS (at most 2 x 16 x 128 bf16 = 8 KiB), the token's own k (q/k RMSNorm + RoPE at the rounding points of
// dec_rope.h) and v are appended to LDS and to the cache, then every query head of the kv head: scores in f32 (lane d owns the pair
// d, d + 64; sum over the wave), f32 softmax, p . V in f32 in ascending key order, one rounding to bf16.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void tts_cp_attn_kernel(const bf16_t* __restrict__ qkv, int pos, int heads, int kv_heads,
                                                         const bf16_t* __restrict__ qn, const bf16_t* __restrict__ kn, float eps,
                                                         const float* __restrict__ cos_t, const float* __restrict__ sin_t,
                                                         bf16_t* __restrict__ kc, bf16_t* __restrict__ vc, bf16_t* __restrict__ out, float scale) {
    constexpr int HD = 128, HALF = 64, MAXP = TTS_GROUPS;
    __shared__ bf16_t s_k[MAXP][HD], s_v[MAXP][HD];
    const int kvh = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
    const int rep = heads / kv_heads, nh = heads + 2 * kv_heads;
    const bf16_t* row = qkv + (long)b * nh * HD;
    bf16_t* kb = kc + ((long)b * kv_heads + kvh) * MAXP * HD;
    bf16_t* vb = vc + ((long)b * kv_heads + kvh) * MAXP * HD;
    for (int j = 0; j < pos; ++j) {
        s_k[j][lane] = kb[j * HD + lane];
        s_k[j][lane + HALF] = kb[j * HD + lane + HALF];
        s_v[j][lane] = vb[j * HD + lane];
        s_v[j][lane + HALF] = vb[j * HD + lane + HALF];
    }
    const float c = cos_t[pos * HALF + lane], sn = sin_t[pos * HALF + lane];
    {
        const bf16_t* src = row + (long)(heads + kvh) * HD;
        const float x1 = bf16_to_f32(src[lane]), x2 = bf16_to_f32(src[lane + HALF]);
        const float inv = rsqrtf(lane_sum<64>(x1 * x1 + x2 * x2) / (float)HD + eps);
        float o1, o2;
        norm_rope_pair(x1, x2, bf16_to_f32(kn[lane]), bf16_to_f32(kn[lane + HALF]), inv, c, sn, o1, o2);
        const bf16_t k1 = f32_to_bf16(o1), k2 = f32_to_bf16(o2);
        s_k[pos][lane] = k1; s_k[pos][lane + HALF] = k2;
        kb[pos * HD + lane] = k1; kb[pos * HD + lane + HALF] = k2;
        const bf16_t* vs = row + (long)(heads + kv_heads + kvh) * HD;
        const bf16_t v1 = vs[lane], v2 = vs[lane + HALF];
        s_v[pos][lane] = v1; s_v[pos][lane + HALF] = v2;
        vb[pos * HD + lane] = v1; vb[pos * HD + lane + HALF] = v2;
    }
    __syncthreads();
    for (int r = 0; r < rep; ++r) {
        const int h = kvh * rep + r;
        const bf16_t* src = row + (long)h * HD;
        const float x1 = bf16_to_f32(src[lane]), x2 = bf16_to_f32(src[lane + HALF]);
        const float inv = rsqrtf(lane_sum<64>(x1 * x1 + x2 * x2) / (float)HD + eps);
        float q1, q2;
        norm_rope_pair(x1, x2, bf16_to_f32(qn[lane]), bf16_to_f32(qn[lane + HALF]), inv, c, sn, q1, q2);
        float sc[MAXP], m = -INFINITY;
#pragma unroll
        for (int j = 0; j < MAXP; ++j) {
            sc[j] = -INFINITY;
            if (j <= pos) {
                sc[j] = lane_sum<64>(q1 * bf16_to_f32(s_k[j][lane]) + q2 * bf16_to_f32(s_k[j][lane + HALF])) * scale;
                m = fmaxf(m, sc[j]);
            }
        }
        float l = 0.0f, o1 = 0.0f, o2 = 0.0f;
#pragma unroll
        for (int j = 0; j < MAXP; ++j) {
            if (j <= pos) {
                const float p = expf(sc[j] - m);
                l += p;
                o1 += p * bf16_to_f32(s_v[j][lane]);
                o2 += p * bf16_to_f32(s_v[j][lane + HALF]);
            }
        }
        bf16_t* dst = out + ((long)b * heads + h) * HD;
        dst[lane] = f32_to_bf16(o1 / l);
        dst[lane + HALF] = f32_to_bf16(o2 / l);
    }
}

// the kernel's launch entry (tts_talker.h): TtsTalker::layer_steps and qasr_syn_attn_case_probe call this
void tts_cp_attn_launch(const bf16_t* qkv, int pos, int B, int heads, int kv_heads, const bf16_t* qn, const bf16_t* kn, float eps,
                        const float* cos_t, const float* sin_t, bf16_t* kc, bf16_t* vc, bf16_t* out, hipStream_t s) {
    if (pos < 0 || pos >= TTS_GROUPS)                                            // s_k[16][128]
        throw std::invalid_argument("qwen3-tts code predictor: attention position outside 0 .. 15");
    if (heads < 1 || kv_heads < 1 || heads % kv_heads != 0)
        throw std::invalid_argument("qwen3-tts code predictor: heads must be a multiple of kv_heads");
    if (B <= 0) return;
    hipLaunchKernelGGL(tts_cp_attn_kernel, dim3(kv_heads, B), dim3(64), 0, s, qkv, pos, heads, kv_heads, qn, kn, eps, cos_t, sin_t, kc, vc, out,
                       1.0f / sqrtf(128.0f));
}

// ------------------------------------------------------------------------------------------------
// The sampler: one workgroup per batch row, the row's logits in LDS.  Steps as tts_sampler.cpp (the host twin) numbers them.  Top-k's
// threshold, the k-th largest value, is found exactly by bisection over the 32 bits of an order-preserving integer key (count of
// keys >= candidate, one barrier per bit).  Behind the pick: the code is stored (Talker: EOS finishes the row instead), and the
// embedding row of the picked token is gathered as the next code-predictor input (Talker: the hidden state is copied next to it).
// ------------------------------------------------------------------------------------------------
struct TtsSampleArgs {
    const float* logits; int V;
    int group;                          // code stream 0 .. 15; 0 = the Talker's
    const TtsTalker::Knobs* knobs;
    TtsState st;
    unsigned char* seen;                // [B][V], Talker only
    const long long* row_index;
    int* codes; int stride;             // [B][16][stride]
    const int* forced; int forced_T;    // [B][16][T] or null
    const bf16_t* emb; int E;           // [V][E]
    bf16_t* emb_out;                    // [B][E]
    const bf16_t* hn; bf16_t* hn_out;   // [B][E] or null
};

__global__ __launch_bounds__(1024) void tts_sample_kernel(TtsSampleArgs a) {
    __shared__ float s_v[TTS_MAX_VOCAB];
    __shared__ float r_v[16];
    __shared__ int r_i[16], s_cnt[2][16];
    const int b = blockIdx.x, tid = threadIdx.x, V = a.V;
    const bool talker = a.group == 0;
    const TtsSampleParams p = talker ? a.knobs->talker : a.knobs->cp;
    const int frame = a.st.frame_of[b];
    const bool fin = a.st.finished[b] != 0;
    const float* row = a.logits + (long)b * V;
    for (int i = tid; i < V; i += 1024) {
        float v = row[i];
        if (talker) {
            if (i >= p.suppress_lo && i < p.suppress_hi && i != p.eos) v = -1e9f;                                      // 1
            if (p.repetition_penalty != 1.0f && a.seen[(long)b * V + i])                                                // 2
                v = v < 0.0f ? v * p.repetition_penalty : v / p.repetition_penalty;
        }
        s_v[i] = v;
    }
    __syncthreads();
    int tok;
    if (a.forced) {
        tok = a.forced[((long)b * TTS_GROUPS + a.group) * a.forced_T + frame];
    } else if (p.temperature <= 0.0f) {                                                                                 // 3
        float bv = -INFINITY;
        int bi = 0x7fffffff;
        for (int i = tid; i < V; i += 1024)
            if (s_v[i] > bv || bi == 0x7fffffff) { bv = s_v[i]; bi = i; }
        tok = sample_block_argmax(bv, bi, r_v, r_i);
    } else {
        float val[TTS_MAX_VOCAB / 1024];
        unsigned key[TTS_MAX_VOCAB / 1024];
#pragma unroll
        for (int e = 0; e < TTS_MAX_VOCAB / 1024; ++e) {
            const int i = tid + e * 1024;
            val[e] = i < V ? s_v[i] / p.temperature : 0.0f;                                                            // 4
            key[e] = i < V ? sample_order_key(val[e]) : 0u;                // 0 is below every real key
        }
        const bool eos_ok = talker && p.eos < V;
        const float eos_saved = eos_ok ? s_v[p.eos] / p.temperature : 0.0f;                                            // 5
        if (p.top_k > 0 && p.top_k < V) {                                                                               // 6
            unsigned prefix = 0u;
            for (int bit = 31; bit >= 0; --bit) {
                const unsigned cand = prefix | (1u << bit);
                int c = 0;
#pragma unroll
                for (int e = 0; e < TTS_MAX_VOCAB / 1024; ++e) c += key[e] >= cand ? 1 : 0;
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
                if ((tid & 63) == 0) s_cnt[bit & 1][tid >> 6] = c;
                __syncthreads();
                int total = 0;
                for (int w = 0; w < 16; ++w) total += s_cnt[bit & 1][w];
                if (total >= p.top_k) prefix = cand;
            }
#pragma unroll
            for (int e = 0; e < TTS_MAX_VOCAB / 1024; ++e)
                if (key[e] < prefix) val[e] = -1e9f;
        }
        const unsigned long long skey = tts_stream_key(p.seed, a.row_index[b], frame, a.group);
        float bv = -INFINITY;
        int bi = 0x7fffffff;
#pragma unroll
        for (int e = 0; e < TTS_MAX_VOCAB / 1024; ++e) {
            const int i = tid + e * 1024;
            if (i >= V) continue;
            float v = val[e];
            if (eos_ok && i == p.eos) v = p.eos_logit_bias != 0.0f ? eos_saved + p.eos_logit_bias : eos_saved;          // 7
            v = v - logf(-logf(tts_uniform(skey, i)));                                                                 // 8
            if (v > bv || bi == 0x7fffffff) { bv = v; bi = i; }
        }
        tok = sample_block_argmax(bv, bi, r_v, r_i);
    }
    if (tok < 0 || tok >= V) tok = 0;                                   // all-NaN logits: keep the gather inside its table
    if (tid == 0 && !fin) {
        if (talker && !a.forced && tok == p.eos) {
            a.st.finished[b] = 1;
            a.st.n_frames[b] = frame;
        } else {
            a.codes[((long)b * TTS_GROUPS + a.group) * a.stride + frame] = tok;
            if (talker) a.seen[(long)b * V + tok] = 1;
        }
    }
    for (int i = tid; i < a.E; i += 1024) {
        a.emb_out[(long)b * a.E + i] = a.emb[(long)tok * a.E + i];
        if (a.hn_out) a.hn_out[(long)b * a.E + i] = a.hn[(long)b * a.E + i];
    }
}

// ------------------------------------------------------------------------------------------------
// The next Talker input of a row: text side (the row's next trailing text embedding, tts_pad once they ran out) + codec_embedding(code 0)
// + the 15 code-predictor embeddings, added in that order in f32, rounded once to bf16.  Then the row's state moves on: position and
// frame count unless it is finished, the frame index always, and the RoPE row of the new position for the Talker's attention.
// ------------------------------------------------------------------------------------------------
struct TtsNextArgs {
    TtsState st;
    const int* codes; int stride;
    const int* forced; int forced_T;
    const bf16_t* tp; const int* trail; int max_trail;
    const bf16_t* codec_emb; const bf16_t* const* cp_emb;
    int H, codec_vocab, cp_vocab;
    bf16_t* x;
    const float *cos_t, *sin_t;
    float *cos_rows, *sin_rows;
    int half;
};

__global__ __launch_bounds__(256) void tts_next_input_kernel(TtsNextArgs a) {
    __shared__ int s_c[TTS_GROUPS];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int frame = a.st.frame_of[b], ctx = a.st.ctx_len[b];
    const bool fin = a.st.finished[b] != 0;
    if (tid < TTS_GROUPS) {
        int c = 0;                                                      // a finished row computes on, its values are never read; in a stream
        if (!fin)                                                       // pool its frame index runs on past the code rows: no load there
            c = a.forced ? a.forced[((long)b * TTS_GROUPS + tid) * a.forced_T + frame] : a.codes[((long)b * TTS_GROUPS + tid) * a.stride + frame];
        const int lim = tid == 0 ? a.codec_vocab : a.cp_vocab;
        s_c[tid] = (c < 0 || c >= lim) ? 0 : c;
    }
    __syncthreads();
    const int ti = frame < a.st.trail_len[b] ? a.trail[(long)b * a.max_trail + frame] : 0;      // row 0 of tp: tts_pad
    for (int i = tid; i < a.H; i += 256) {
        float s = bf16_to_f32(a.tp[(long)ti * a.H + i]);
        s += bf16_to_f32(a.codec_emb[(long)s_c[0] * a.H + i]);
        for (int g = 0; g < TTS_GROUPS - 1; ++g) s += bf16_to_f32(a.cp_emb[g][(long)s_c[g + 1] * a.H + i]);
        a.x[(long)b * a.H + i] = f32_to_bf16(s);
    }
    const int nctx = fin ? ctx : ctx + 1;
    for (int t = tid; t < a.half; t += 256) {
        a.cos_rows[(long)b * a.half + t] = a.cos_t[(long)nctx * a.half + t];
        a.sin_rows[(long)b * a.half + t] = a.sin_t[(long)nctx * a.half + t];
    }
    if (tid == 0) {
        if (!fin) { a.st.ctx_len[b] = nctx; a.st.n_frames[b] = frame + 1; }
        a.st.frame_of[b] = frame + 1;
    }
}

// ---- prefill: text rows gathered for the text projection, the prompt assembled, one prompt position fed per step ------------------
__global__ __launch_bounds__(256) void tts_gather_rows_kernel(const bf16_t* __restrict__ table, const int* __restrict__ ids, int W,
                                                              bf16_t* __restrict__ out) {
    const long r = blockIdx.x;
    for (int i = threadIdx.x; i < W; i += 256) out[r * W + i] = table[(long)ids[r] * W + i];
}

// pf[b][p] = bf16(text side + codec side): text side = tp[pf_text] (or nothing), codec side = codec_embedding[pf_codec] | the x-vector (-2) |
// frame f = -3 - pf_codec of the row's ICL reference codes ref[b][16][ref_ld]: codec_embedding[c0] + the 15 code-predictor embeddings, added
// in the order of tts_next_input_kernel (text, code 0, streams 1 .. 15) in f32 and rounded once.  The codes were checked by the C ABI.
__global__ __launch_bounds__(256) void tts_prefill_build_kernel(const int* __restrict__ pf_text, const int* __restrict__ pf_codec, int P,
                                                                const bf16_t* __restrict__ tp, const bf16_t* __restrict__ codec_emb,
                                                                const float* __restrict__ xvec, int H, bf16_t* __restrict__ pf,
                                                                const int* __restrict__ ref, int ref_ld, const bf16_t* const* __restrict__ cp_emb) {
    __shared__ int s_c[TTS_GROUPS];
    const int p = blockIdx.x, b = blockIdx.y;
    const int ti = pf_text[(long)b * P + p], ci = pf_codec[(long)b * P + p];
    if (ci <= -3) {                                                     // block-uniform
        if (threadIdx.x < TTS_GROUPS) s_c[threadIdx.x] = ref[((long)b * TTS_GROUPS + threadIdx.x) * ref_ld + (-3 - ci)];
        __syncthreads();
    }
    for (int i = threadIdx.x; i < H; i += 256) {
        float s = ti >= 0 ? bf16_to_f32(tp[(long)ti * H + i]) : 0.0f;
        if (ci >= 0) s += bf16_to_f32(codec_emb[(long)ci * H + i]);
        else if (ci == -2) s += xvec[(long)b * H + i];
        else if (ci <= -3) {
            s += bf16_to_f32(codec_emb[(long)s_c[0] * H + i]);
            for (int g = 0; g < TTS_GROUPS - 1; ++g) s += bf16_to_f32(cp_emb[g][(long)s_c[g + 1] * H + i]);
        }
        pf[((long)b * P + p) * H + i] = f32_to_bf16(s);
    }
}

// packed prompt pass: x[p] = pf[slot[p]][pos[p]] for the packed positions (every prompt position of a row but its last)
__global__ __launch_bounds__(128) void tts_pack_rows_kernel(const bf16_t* __restrict__ pf, int pf_ld, const int* __restrict__ slot,
                                                            const int* __restrict__ pos, int H, bf16_t* __restrict__ x) {
    const long p = blockIdx.x;
    const uint4* src = reinterpret_cast<const uint4*>(pf + ((long)slot[p] * pf_ld + pos[p]) * H);
    uint4* dst = reinterpret_cast<uint4*>(x + p * H);
    for (int i = threadIdx.x; i < H / 8; i += 128) dst[i] = src[i];
}

// step s of the prompt pass over prompts that END together: row b feeds its position s - (P - len[b]); before its first position it
// recomputes position 0, which its real first step then overwrites
__global__ __launch_bounds__(256) void tts_prefill_feed_kernel(TtsState st, int s, int P, const bf16_t* __restrict__ pf, int pf_ld, int H,
                                                               bf16_t* __restrict__ x, const float* __restrict__ cos_t,
                                                               const float* __restrict__ sin_t, float* __restrict__ cos_rows,
                                                               float* __restrict__ sin_rows, int half) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int p = max(s - (P - st.pf_len[b]), 0);
    for (int i = tid; i < H; i += 256) x[(long)b * H + i] = pf[((long)b * pf_ld + p) * H + i];
    for (int t = tid; t < half; t += 256) {
        cos_rows[(long)b * half + t] = cos_t[(long)p * half + t];
        sin_rows[(long)b * half + t] = sin_t[(long)p * half + t];
    }
    if (tid == 0) st.ctx_len[b] = p;
}

// forced pass: src [B][W] (f32 or bf16) -> dst[b][frame_of[b]][slot] rows of a [B][T][slots][W] f32 array
__global__ __launch_bounds__(256) void tts_copy_out_kernel(const float* __restrict__ srcf, const bf16_t* __restrict__ srcb, int W,
                                                           const int* __restrict__ frame_of, int T, int slots, int slot,
                                                           float* __restrict__ dst) {
    const int b = blockIdx.x;
    const long o = (((long)b * T + frame_of[b]) * slots + slot) * W;
    for (int i = threadIdx.x; i < W; i += 256) dst[o + i] = srcf ? srcf[(long)b * W + i] : bf16_to_f32(srcb[(long)b * W + i]);
}

// ================================================================================================
// host
// ================================================================================================
static const char* const WHO = "talker";

void TtsTalker::check_geometry(const qasr_tts_config& c) {
    auto bad = [](const std::string& m) { throw std::invalid_argument(std::string(WHO) + ": " + m); };
    if (c.bits != 4 && c.bits != 8) bad("bits must be 4 or 8 (a float checkpoint is not served)");
    if (c.group_size != 64) bad("only group size 64 is supported");
    if (c.head_dim != 128 || c.cp_head_dim != 128) bad("head_dim must be 128 (the attention kernels are built for it)");
    if (c.heads != 2 * c.kv_heads || c.kv_heads < 1) bad("the Talker needs 2 query heads per kv head");
    if (c.cp_kv_heads < 1 || c.cp_heads % c.cp_kv_heads != 0) bad("cp_heads must be a multiple of cp_kv_heads");
    for (int k : {c.hidden, c.inter, c.text_hidden, c.cp_hidden, c.cp_inter, c.cp_embedding_dim})
        if (k < 64 || k % 64 != 0) bad("every GEMV width (K) must be a multiple of 64");
    if (c.inter % 16 != 0 || c.cp_inter % 16 != 0) bad("intermediate sizes must be multiples of 16");
    if (c.cp_embedding_dim != c.hidden) bad("cp_embedding_dim must equal the Talker's hidden size");
    if (c.layers < 1 || c.cp_layers < 1) bad("layer counts must be positive");
    if (c.codec_vocab < 1 || c.codec_vocab > TTS_MAX_VOCAB || c.cp_vocab < 1 || c.cp_vocab > TTS_MAX_VOCAB)
        bad("codec_vocab and cp_vocab in 1..4096");
    if (c.text_vocab < 1) bad("text_vocab must be positive");
    for (int id : {c.codec_pad, c.codec_bos, c.codec_eos, c.codec_think, c.codec_nothink, c.codec_think_bos, c.codec_think_eos})
        if (id < 0 || id >= c.codec_vocab) bad("a codec special id lies outside codec_vocab");
    for (int id : {c.tts_pad, c.tts_bos, c.tts_eos})
        if (id < 0 || id >= c.text_vocab) bad("a text-side special id lies outside text_vocab");
    if (c.suppress_lo < 0 || c.suppress_hi > c.codec_vocab || c.suppress_lo > c.suppress_hi) bad("suppress range outside codec_vocab");
    if (c.max_batch < 1 || c.max_batch > 64) bad("max_batch in 1..64");
    if (c.max_frames < 1 || c.max_frames > TTS_MAX_FRAMES) bad("max_frames in 1..500");
    if (c.max_text < TTS_TEMPLATE || c.max_text > 8192) bad("max_text in 9..8192");
    if (c.max_instruct < 0 || c.max_instruct > 8192) bad("max_instruct in 0..8192");
}

void TtsTalker::load_net(const SafeTensorsDir& st, QlmLoader& wl, const std::string& prefix, Net& n, int layers) {
    const QlmLayerGeom g{n.H, n.heads * n.hd, n.kv * n.hd, n.I, cfg_.bits};
    for (int l = 0; l < layers; ++l) {
        const std::string p = prefix + "model.layers." + std::to_string(l) + ".";
        Layer L{qlm_load_layer(wl, st, p, g, QlmBias::NONE)};
        L.qn = wl.bf16(st, p + "self_attn.q_norm.weight", {n.hd});
        L.kn = wl.bf16(st, p + "self_attn.k_norm.weight", {n.hd});
        // the packed images of the tuned decode GEMVs (dec_quant.h) next to the triplets the generic kernel reads
        for (QLin* q : {&L.qkv, &L.o, &L.gu, &L.down})
            if (q->N % 16 == 0 && q->K % 128 == 0) wl.pack(*q);
        n.layers.push_back(L);
    }
    n.norm = wl.bf16(st, prefix + "model.norm.weight", {n.H});
}

// every tensor of both networks; a dry loader: the host checks alone (presence, shape, dtype of every key), no HIP call.  Keys the two
// networks do not name are not refused: the checkpoint holds other sub-models.
void TtsTalker::load_all(const SafeTensorsDir& st, QlmLoader& wl) {
    const auto& c = cfg_;
    const int bits = c.bits;
    tk_ = Net{}; cp_ = Net{};
    tk_.H = c.hidden; tk_.heads = c.heads; tk_.kv = c.kv_heads; tk_.hd = c.head_dim; tk_.I = c.inter; tk_.eps = c.rms_eps;
    cp_.H = c.cp_hidden; cp_.heads = c.cp_heads; cp_.kv = c.cp_kv_heads; cp_.hd = c.cp_head_dim; cp_.I = c.cp_inter; cp_.eps = c.cp_rms_eps;
    const std::string T = "talker.", P = "talker.code_predictor.";
    codec_emb_ = wl.bf16(st, T + "model.codec_embedding.weight", {c.codec_vocab, c.hidden});
    text_emb_ = wl.bf16(st, T + "model.text_embedding.weight", {c.text_vocab, c.text_hidden});
    // the heads and the biased projections stay raw triplets (tts_gemv_rows_kernel); their bias is read as plain f32
    fc1_ = wl.qlin(st, {T + "text_projection.linear_fc1"}, c.text_hidden, bits, QlmBias::F32);
    fc2_ = wl.qlin(st, {T + "text_projection.linear_fc2"}, c.text_hidden, bits, QlmBias::F32);
    head_ = wl.qlin(st, {T + "codec_head"}, c.hidden, bits);
    if (fc1_.N != c.text_hidden || fc2_.N != c.hidden || head_.N != c.codec_vocab)
        wl.refuse("text_projection / codec_head row counts do not match the geometry");
    load_net(st, wl, T, tk_, c.layers);
    load_net(st, wl, P, cp_, c.cp_layers);
    std::vector<const bf16_t*> tables;
    for (int g = 0; g < TTS_GROUPS - 1; ++g) {
        cp_emb_[g] = wl.bf16(st, P + "model.codec_embedding." + std::to_string(g) + ".weight", {c.cp_vocab, c.cp_embedding_dim});
        tables.push_back(cp_emb_[g]);
        lm_[g] = wl.qlin(st, {P + "lm_head." + std::to_string(g)}, c.cp_hidden, bits);
        if (lm_[g].N != c.cp_vocab) wl.refuse("lm_head." + std::to_string(g) + " does not hold cp_vocab rows");
    }
    if (!wl.dry()) d_cp_emb_ = (const bf16_t**)wl.upload(tables.data(), tables.size() * sizeof(void*));
    if (c.cp_embedding_dim != c.cp_hidden) {
        proj_ = wl.qlin(st, {P + "small_to_mtp_projection"}, c.cp_embedding_dim, bits, QlmBias::F32);
        if (proj_.N != c.cp_hidden) wl.refuse("small_to_mtp_projection does not hold cp_hidden rows");
    }
}

int TtsTalker::icl_context(const qasr_tts_config& c, int max_ref_frames, int max_ref_text) {
    auto bad = [](const std::string& m) { throw std::invalid_argument(std::string(WHO) + ": " + m); };
    if (max_ref_frames < 1) bad("max_ref_frames must be at least 1 for an ICL handle");
    if (max_ref_text < 0) bad("max_ref_text must not be negative");
    // 64: the prompt pass writes and reads the V images in blocks of 64 keys (v_transpose_kernel, prefill_attention2_kernel)
    const long prompt = std::max<long>((long)c.max_instruct + 11, (long)TTS_ICL_FIXED + max_ref_text + c.max_text + max_ref_frames);
    const long ctx = (prompt + c.max_frames + 1 + 63) / 64 * 64;
    if (ctx > TTS_MAX_CTX)
        bad("an ICL context of " + std::to_string(ctx) + " positions (11 + max_ref_text + max_text + max_ref_frames + max_frames + 1) is over the limit of " +
            std::to_string(TTS_MAX_CTX) + " positions");
    return (int)ctx;
}

TtsTalker::TtsTalker(const qasr_tts_config& cfg, const SafeTensorsDir& st, int max_ref_frames, int max_ref_text)
    : cfg_(cfg), max_ref_frames_(max_ref_frames), max_ref_text_(max_ref_frames > 0 ? max_ref_text : 0) {
    check_geometry(cfg_);
    const auto& c = cfg_;
    const bool icl = max_ref_frames_ > 0;
    const int icl_ctx = icl ? icl_context(c, max_ref_frames_, max_ref_text_) : 0;
    {
        QlmLoader dry(WHO, nullptr, true);
        load_all(st, dry);                                                 // throws before any HIP call
    }
    QASR_HIP(hipSetDevice(c.device));
    QASR_HIP(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
    try {
        wl_ = std::make_unique<QlmLoader>(WHO, stream_, false);
        load_all(st, *wl_);
        // ---- tables, caches, workspaces -------------------------------------------------------------------------------------
        const int B = c.max_batch, H = c.hidden, half = c.head_dim / 2;
        max_prefill_ = c.max_instruct + 11;                                 // instruct + role 3 + codec prefix (<= 8) - 1 + first text
        if (icl) max_prefill_ = std::max(max_prefill_, TTS_ICL_FIXED + max_ref_text_ + c.max_text + max_ref_frames_);
        max_ctx_ = icl ? icl_ctx : ((max_prefill_ + c.max_frames + 1 + 31) / 32) * 32;
        max_tp_ = 3 + B * (c.max_text + c.max_instruct + max_ref_text_);
        std::vector<float> rc, rs;
        rope_tables_host(c.rope_theta, half, max_ctx_, rc, rs);
        d_rope_cos_ = (float*)wl_->upload(rc.data(), rc.size() * 4);
        d_rope_sin_ = (float*)wl_->upload(rs.data(), rs.size() * 4);
        rope_tables_host(c.cp_rope_theta, c.cp_head_dim / 2, TTS_GROUPS, rc, rs);
        d_cp_cos_ = (float*)wl_->upload(rc.data(), rc.size() * 4);
        d_cp_sin_ = (float*)wl_->upload(rs.data(), rs.size() * 4);
        d_rope_rows_ = (float*)wl_->upload(nullptr, (size_t)2 * B * half * 4);
        const size_t kv_bytes = (size_t)c.layers * B * c.kv_heads * max_ctx_ * c.head_dim * 2;
        d_k_ = (bf16_t*)wl_->upload(nullptr, kv_bytes);
        d_vf_ = (bf16_t*)wl_->upload(nullptr, kv_bytes);
        QASR_HIP(hipMemsetAsync(d_k_, 0, kv_bytes, stream_));               // the attention sweep reads whole 32-key chunks and masks: finite values
        QASR_HIP(hipMemsetAsync(d_vf_, 0, kv_bytes, stream_));
        const size_t cpkv = (size_t)c.cp_layers * B * c.cp_kv_heads * TTS_GROUPS * c.cp_head_dim * 2;
        d_cpk_ = (bf16_t*)wl_->upload(nullptr, cpkv);
        d_cpv_ = (bf16_t*)wl_->upload(nullptr, cpkv);
        const int nqkv = std::max((c.heads + 2 * c.kv_heads) * c.head_dim, (c.cp_heads + 2 * c.cp_kv_heads) * c.cp_head_dim);
        const int nattn = std::max(c.heads * c.head_dim, c.cp_heads * c.cp_head_dim);
        const int wmax = std::max({H, c.cp_hidden, c.inter, c.cp_inter, nattn});
        d_x_ = (bf16_t*)wl_->upload(nullptr, (size_t)B * H * 2);
        d_hn_ = (bf16_t*)wl_->upload(nullptr, (size_t)B * H * 2);
        d_qkv_ = (bf16_t*)wl_->upload(nullptr, (size_t)B * nqkv * 2);
        d_attn_ = (bf16_t*)wl_->upload(nullptr, (size_t)B * nattn * 2);
        d_act_ = (bf16_t*)wl_->upload(nullptr, (size_t)B * std::max(c.inter, c.cp_inter) * 2);
        d_scratch_ = (bf16_t*)wl_->upload(nullptr, (size_t)B * wmax * 2);
        d_cpa_ = (bf16_t*)wl_->upload(nullptr, (size_t)B * H * 2);
        d_cpb_ = (bf16_t*)wl_->upload(nullptr, (size_t)B * H * 2);
        d_cx_ = (bf16_t*)wl_->upload(nullptr, (size_t)B * c.cp_hidden * 2);
        d_chn_ = (bf16_t*)wl_->upload(nullptr, (size_t)B * c.cp_hidden * 2);
        d_tp_in_ = (bf16_t*)wl_->upload(nullptr, (size_t)max_tp_ * c.text_hidden * 2);
        d_tp_mid_ = (bf16_t*)wl_->upload(nullptr, (size_t)max_tp_ * c.text_hidden * 2);
        d_tp_ = (bf16_t*)wl_->upload(nullptr, (size_t)max_tp_ * H * 2);
        d_pf_ = (bf16_t*)wl_->upload(nullptr, (size_t)B * max_prefill_ * H * 2);
        d_logits_ = (float*)wl_->upload(nullptr, (size_t)B * c.codec_vocab * 4);
        d_cp_logits_ = (float*)wl_->upload(nullptr, (size_t)B * c.cp_vocab * 4);
        d_xvec_ = (float*)wl_->upload(nullptr, (size_t)B * H * 4);
        d_state_ = (int*)wl_->upload(nullptr, (size_t)6 * B * 4);
        d_codes_ = (int*)wl_->upload(nullptr, (size_t)B * TTS_GROUPS * c.max_frames * 4);
        d_tp_ids_ = (int*)wl_->upload(nullptr, (size_t)max_tp_ * 4);
        d_pf_text_ = (int*)wl_->upload(nullptr, (size_t)B * max_prefill_ * 4);
        d_pf_codec_ = (int*)wl_->upload(nullptr, (size_t)B * max_prefill_ * 4);
        d_trail_ = (int*)wl_->upload(nullptr, (size_t)B * c.max_text * 4);
        d_row_index_ = (long long*)wl_->upload(nullptr, (size_t)B * 8);
        d_seen_ = (unsigned char*)wl_->upload(nullptr, (size_t)B * c.codec_vocab);
        d_knobs_ = (Knobs*)wl_->upload(nullptr, sizeof(Knobs));
        if (icl) {
            const int nq = c.heads * c.head_dim, nkv = c.kv_heads * c.head_dim, I = c.inter;
            d_ref_codes_ = (int*)wl_->upload(nullptr, (size_t)B * TTS_GROUPS * max_ref_frames_ * 4);
            max_pos_ = B * (max_prefill_ - 1);
            vt_stride_ = (max_prefill_ + 63) / 64 * 64;
            d_w_ = (bf16_t*)wl_->upload(nullptr, ((size_t)(nq + 2 * nkv) * H + (size_t)H * nq + (size_t)2 * I * H + (size_t)H * I) * 2);
            const size_t vt_bytes = (size_t)B * c.kv_heads * c.head_dim * vt_stride_ * 2;
            d_vt_ = (bf16_t*)wl_->upload(nullptr, vt_bytes);
            QASR_HIP(hipMemsetAsync(d_vt_, 0, vt_bytes, stream_));          // masked keys multiply stale bytes by P = 0
            d_px_ = (bf16_t*)wl_->upload(nullptr, (size_t)max_pos_ * H * 2);
            d_ph_ = (bf16_t*)wl_->upload(nullptr, (size_t)max_pos_ * H * 2);
            d_pqkv_ = (bf16_t*)wl_->upload(nullptr, (size_t)max_pos_ * (nq + 2 * nkv) * 2);
            d_pqr_ = (bf16_t*)wl_->upload(nullptr, (size_t)max_pos_ * nq * 2);
            d_pattn_ = (bf16_t*)wl_->upload(nullptr, (size_t)max_pos_ * nq * 2);
            d_pact_ = (bf16_t*)wl_->upload(nullptr, (size_t)max_pos_ * I * 2);
            d_pmeta_ = (int*)wl_->upload(nullptr, ((size_t)2 * max_pos_ + 2 * B + 1) * 4);
        }
        QASR_HIP(hipStreamSynchronize(stream_));
    } catch (...) {
        wl_.reset();
        (void)hipStreamDestroy(stream_);
        throw;
    }
}

TtsTalker::~TtsTalker() {
    if (stream_) (void)hipStreamSynchronize(stream_);
    graphs_.drop();
    wl_.reset();
    for (auto& f : forced_buf_) f.reset();
    if (stream_) (void)hipStreamDestroy(stream_);
}

static TtsState state_of(int* base, int B) { return TtsState{base, base + B, base + 2 * B, base + 3 * B, base + 4 * B, base + 5 * B}; }

// one token per row through every layer of a network, in place on x.  talker: attention over the row's cache at ctx_len[b];
// else the code predictor's attention at position cp_pos of the frame.  kv_only_last: the last layer stops behind its attention
// (its K / V are all a later position needs of it).  row0 (Talker only): x holds the rows of slots row0 .. row0 + B - 1, whose state, RoPE
// rows and cache blocks are read at their own slots (the pool admits one slot while the others stand still).
void TtsTalker::layer_steps(const Net& n, bf16_t* x, int B, bool talker, int cp_pos, bool kv_only_last, int row0) {
    const int nq = n.heads * n.hd, nkv = n.kv * n.hd, half = n.hd / 2;
    const int MB = cfg_.max_batch;
    TtsState st = state_of(d_state_, MB);
    for (size_t l = 0; l < n.layers.size(); ++l) {
        const Layer& L = n.layers[l];
        DecGemvArgs a{};
        a.X = x; a.B = B; a.N = nq + 2 * nkv; a.K = n.H; a.out = d_qkv_;
        decode_gemv_q_launch(DEC_EPI_BF16, a, L.qkv.img, L.ln1, n.eps, d_scratch_, stream_);
        if (talker) {
            const size_t per = (size_t)MB * n.kv * max_ctx_ * n.hd;
            const size_t slot0 = (size_t)row0 * n.kv * max_ctx_ * n.hd;      // KVLayout::off(slot, 0, 0)
            KVLayout kv{d_k_ + l * per + slot0, nullptr, max_ctx_, n.kv, n.hd, d_vf_ + l * per + slot0};
            decode_attention_launch(d_qkv_, st.ctx_len + row0, B, n.heads, n.kv, n.hd, L.qn, L.kn, n.eps, d_rope_rows_ + (size_t)row0 * half,
                                    d_rope_rows_ + (size_t)(MB + row0) * half, kv, d_attn_, stream_);
        } else {
            const size_t per = (size_t)MB * n.kv * TTS_GROUPS * n.hd;
            tts_cp_attn_launch(d_qkv_, cp_pos, B, n.heads, n.kv, L.qn, L.kn, n.eps, d_cp_cos_, d_cp_sin_, d_cpk_ + l * per, d_cpv_ + l * per,
                               d_attn_, stream_);
        }
        if (kv_only_last && l + 1 == n.layers.size()) break;
        a.X = d_attn_; a.N = n.H; a.K = nq; a.out = x;
        decode_gemv_q_launch(DEC_EPI_RESID, a, L.o.img, nullptr, n.eps, d_scratch_, stream_);
        a.X = x; a.N = 2 * n.I; a.K = n.H; a.out = d_act_;
        decode_gemv_q_launch(DEC_EPI_SWIGLU, a, L.gu.img, L.ln2, n.eps, d_scratch_, stream_);
        a.X = d_act_; a.N = n.H; a.K = n.I; a.out = x;
        decode_gemv_q_launch(DEC_EPI_RESID, a, L.down.img, nullptr, n.eps, d_scratch_, stream_);
    }
}

// One frame of every row (tts_talker.h): Talker step, code 0, the code predictor's 16 positions, next input.
void TtsTalker::issue_frame(int B, bool forced_mode) {
    const auto& c = cfg_;
    const int MB = c.max_batch, H = c.hidden, Hc = c.cp_hidden;
    TtsState st = state_of(d_state_, MB);
    const bool proj = c.cp_embedding_dim != c.cp_hidden;
    layer_steps(tk_, d_x_, B, true, 0, false);
    rmsnorm_rows_launch(d_x_, tk_.norm, d_hn_, B, H, c.rms_eps, stream_);
    gemv_rows(head_.img.raw, d_hn_, B, nullptr, d_logits_, nullptr, c.codec_vocab, false, stream_);
    if (forced_mode) {
        if (d_f_tlog_) hipLaunchKernelGGL(tts_copy_out_kernel, dim3(B), dim3(256), 0, stream_, (const float*)d_logits_, (const bf16_t*)nullptr, c.codec_vocab, (const int*)st.frame_of, forced_T_host_, 1, 0, d_f_tlog_);
        if (d_f_hid_) hipLaunchKernelGGL(tts_copy_out_kernel, dim3(B), dim3(256), 0, stream_, (const float*)nullptr, (const bf16_t*)d_hn_, H, (const int*)st.frame_of, forced_T_host_, 1, 0, d_f_hid_);
    }
    TtsSampleArgs sa{};
    sa.knobs = d_knobs_; sa.st = st; sa.seen = d_seen_; sa.row_index = d_row_index_;
    sa.codes = d_codes_; sa.stride = c.max_frames;
    sa.forced = forced_mode ? d_f_codes_ : nullptr; sa.forced_T = forced_T_host_;
    sa.logits = d_logits_; sa.V = c.codec_vocab; sa.group = 0;
    sa.emb = codec_emb_; sa.E = H; sa.emb_out = d_cpb_; sa.hn = d_hn_; sa.hn_out = d_cpa_;
    hipLaunchKernelGGL(tts_sample_kernel, dim3(B), dim3(1024), 0, stream_, sa);
    // the code predictor: positions 0 (hidden state) and 1 (code 0) give code 1; position g + 1 holds code g and gives code g + 1
    for (int pos = 0; pos < TTS_GROUPS; ++pos) {
        bf16_t* in = pos == 0 ? d_cpa_ : d_cpb_;
        bf16_t* x = in;
        if (proj) {
            gemv_rows(proj_.img.raw, in, B, proj_.bias, nullptr, d_cx_, Hc, false, stream_);
            x = d_cx_;
        }
        layer_steps(cp_, x, B, false, pos, pos == 0);
        if (pos == 0) continue;
        const int g = pos - 1;                                             // lm_head.g -> code g + 1
        rmsnorm_rows_launch(x, cp_.norm, d_chn_, B, Hc, c.cp_rms_eps, stream_);
        gemv_rows(lm_[g].img.raw, d_chn_, B, nullptr, d_cp_logits_, nullptr, c.cp_vocab, false, stream_);
        if (forced_mode && d_f_cplog_)
            hipLaunchKernelGGL(tts_copy_out_kernel, dim3(B), dim3(256), 0, stream_, (const float*)d_cp_logits_, (const bf16_t*)nullptr, c.cp_vocab, (const int*)st.frame_of, forced_T_host_, TTS_GROUPS - 1, g, d_f_cplog_);
        sa.logits = d_cp_logits_; sa.V = c.cp_vocab; sa.group = g + 1;
        sa.emb = cp_emb_[g]; sa.E = c.cp_embedding_dim; sa.emb_out = d_cpb_; sa.hn = nullptr; sa.hn_out = nullptr;
        hipLaunchKernelGGL(tts_sample_kernel, dim3(B), dim3(1024), 0, stream_, sa);
    }
    TtsNextArgs na{};
    na.st = st; na.codes = d_codes_; na.stride = c.max_frames; na.forced = sa.forced; na.forced_T = forced_T_host_;
    na.tp = d_tp_; na.trail = d_trail_; na.max_trail = c.max_text;
    na.codec_emb = codec_emb_; na.cp_emb = d_cp_emb_; na.H = H; na.codec_vocab = c.codec_vocab; na.cp_vocab = c.cp_vocab;
    na.x = d_x_; na.cos_t = d_rope_cos_; na.sin_t = d_rope_sin_;
    na.cos_rows = d_rope_rows_; na.sin_rows = d_rope_rows_ + (size_t)MB * (c.head_dim / 2); na.half = c.head_dim / 2;
    hipLaunchKernelGGL(tts_next_input_kernel, dim3(B), dim3(256), 0, stream_, na);
    QASR_HIP(hipGetLastError());
}

void TtsTalker::run_frame(int B) {
    graphs_.run(B, stream_, [&] { issue_frame(B, false); });
}

// The prompt plan of one row: buildPrefillEmbeddings (Qwen3TTS.swift:1313-1390), for an ICL row buildICLPrefillEmbeddings.  pt / pc
// [max_prefill_] (preset to -1): the text-side and codec-side entry of every position; tr [max_text]: the trailing text rows, nt of them.
// A text id is appended to tp_ids and named by its row of the projected text table, tp_row0 + its place in tp_ids (rows 0 1 2 of the
// table are tts_pad, tts_bos, tts_eos).  xv [hidden], ref [16][max_ref_frames_] (ICL rows).  Returns the prompt length.
int TtsTalker::plan_row(const TtsRow& r, std::vector<int>& tp_ids, int tp_row0, int* pt, int* pc, int* tr, int& nt, float* xv, int* ref) const {
    const auto& c = cfg_;
    int n = 0;
    nt = 0;
    auto text_row = [&](int id) { tp_ids.push_back(id); return tp_row0 + (int)tp_ids.size() - 1; };
    for (int i = 0; i < r.n_instruct; ++i) pt[n++] = text_row(r.instruct[i]);                  // instruct in front
    for (int i = 0; i < 3; ++i) pt[n++] = text_row(r.text[i]);                                 // role
    std::vector<int> codec = {c.codec_think, c.codec_think_bos, r.language, c.codec_think_eos};
    if (r.xvector) { codec.push_back(-2); std::memcpy(xv, r.xvector, (size_t)c.hidden * 4); }
    if (r.speaker >= 0) codec.push_back(r.speaker);
    codec.push_back(c.codec_pad);
    codec.push_back(c.codec_bos);
    const int L = (int)codec.size();
    for (int i = 0; i < L - 1; ++i) { pt[n] = i < L - 2 ? 0 : 1; pc[n++] = codec[i]; }        // tts_pad ... tts_bos over the prefix
    if (r.ref_codes) {
        // buildICLPrefillEmbeddings (Qwen3TTS+ICL.swift:158-242): the prefix's own codec_bos is dropped; every text id over codec_pad,
        // tts_eos over codec_pad, tts_pad over codec_bos, tts_pad over every reference frame; no trailing text
        for (int i = 0; i < r.n_ref_text; ++i) { pt[n] = text_row(r.ref_text[i]); pc[n++] = c.codec_pad; }
        for (int i = 3; i < r.n_text - 5; ++i) { pt[n] = text_row(r.text[i]); pc[n++] = c.codec_pad; }
        pt[n] = 2; pc[n++] = c.codec_pad;
        pt[n] = 0; pc[n++] = c.codec_bos;
        for (int f = 0; f < r.ref_frames; ++f) { pt[n] = 0; pc[n++] = -3 - f; }
        for (int g = 0; g < TTS_GROUPS; ++g)
            std::memcpy(&ref[(size_t)g * max_ref_frames_], r.ref_codes + (size_t)g * r.ref_frames, (size_t)r.ref_frames * 4);
    } else {
        pt[n] = text_row(r.text[3]); pc[n++] = codec[L - 1];                                   // first text + codec_bos
        for (int i = 4; i < r.n_text - 5; ++i) tr[nt++] = text_row(r.text[i]);
        tr[nt++] = 2;                                                                          // tts_eos
    }
    return n;
}

// buildPrefillEmbeddings (Qwen3TTS.swift:1313-1390) for every row, then the prompt positions but the last through the Talker's layers.
void TtsTalker::prefill(const std::vector<TtsRow>& rows, bool build_only) {
    const auto& c = cfg_;
    const int B = (int)rows.size(), MB = c.max_batch, H = c.hidden, P = max_prefill_, half = c.head_dim / 2;
    std::vector<int> tp_ids = {c.tts_pad, c.tts_bos, c.tts_eos};          // rows 0 1 2 of the projected text table
    std::vector<int> pf_text((size_t)B * P, -1), pf_codec((size_t)B * P, -1), trail((size_t)B * c.max_text, 0), state((size_t)6 * MB, 0);
    std::vector<float> xv((size_t)B * H, 0.0f);
    std::vector<long long> ridx(MB, 0);
    std::vector<int> ref;
    bool icl = false;
    for (const TtsRow& r : rows) icl = icl || r.ref_codes;
    if (icl) ref.assign((size_t)B * TTS_GROUPS * max_ref_frames_, 0);
    pf_len_.assign(B, 0);
    int Pmax = 0;
    for (int b = 0; b < B; ++b) {
        ridx[b] = rows[b].index;
        int nt = 0;
        const int n = plan_row(rows[b], tp_ids, 0, &pf_text[(size_t)b * P], &pf_codec[(size_t)b * P], &trail[(size_t)b * c.max_text], nt,
                               &xv[(size_t)b * H], icl ? &ref[(size_t)b * TTS_GROUPS * max_ref_frames_] : nullptr);
        pf_len_[b] = n;
        state[(size_t)4 * MB + b] = nt;
        state[(size_t)5 * MB + b] = n;
        Pmax = std::max(Pmax, n);
    }
    for (int b = B; b < MB; ++b) state[(size_t)1 * MB + b] = 1;
    const int ntp = (int)tp_ids.size();
    QASR_HIP(hipMemcpyAsync(d_tp_ids_, tp_ids.data(), (size_t)ntp * 4, hipMemcpyHostToDevice, stream_));
    QASR_HIP(hipMemcpyAsync(d_pf_text_, pf_text.data(), pf_text.size() * 4, hipMemcpyHostToDevice, stream_));
    QASR_HIP(hipMemcpyAsync(d_pf_codec_, pf_codec.data(), pf_codec.size() * 4, hipMemcpyHostToDevice, stream_));
    QASR_HIP(hipMemcpyAsync(d_trail_, trail.data(), trail.size() * 4, hipMemcpyHostToDevice, stream_));
    QASR_HIP(hipMemcpyAsync(d_state_, state.data(), state.size() * 4, hipMemcpyHostToDevice, stream_));
    QASR_HIP(hipMemcpyAsync(d_xvec_, xv.data(), xv.size() * 4, hipMemcpyHostToDevice, stream_));
    if (icl) QASR_HIP(hipMemcpyAsync(d_ref_codes_, ref.data(), ref.size() * 4, hipMemcpyHostToDevice, stream_));
    QASR_HIP(hipMemcpyAsync(d_row_index_, ridx.data(), ridx.size() * 8, hipMemcpyHostToDevice, stream_));
    QASR_HIP(hipMemsetAsync(d_seen_, 0, (size_t)MB * c.codec_vocab, stream_));
    QASR_HIP(hipMemsetAsync(d_codes_, 0xff, (size_t)MB * TTS_GROUPS * c.max_frames * 4, stream_));
    // text_projection(text_embedding(id)) of every text-side id of the call
    hipLaunchKernelGGL(tts_gather_rows_kernel, dim3(ntp), dim3(256), 0, stream_, text_emb_, (const int*)d_tp_ids_, c.text_hidden, d_tp_in_);
    gemv_rows(fc1_.img.raw, d_tp_in_, ntp, fc1_.bias, nullptr, d_tp_mid_, c.text_hidden, true, stream_);
    gemv_rows(fc2_.img.raw, d_tp_mid_, ntp, fc2_.bias, nullptr, d_tp_, H, false, stream_);
    hipLaunchKernelGGL(tts_prefill_build_kernel, dim3(P, B), dim3(256), 0, stream_, (const int*)d_pf_text_, (const int*)d_pf_codec_, P,
                       (const bf16_t*)d_tp_, codec_emb_, (const float*)d_xvec_, H, d_pf_, (const int*)d_ref_codes_, max_ref_frames_,
                       (const bf16_t* const*)d_cp_emb_);
    TtsState st = state_of(d_state_, MB);
    // ICL calls under tts_packed_prompt: every prompt position but the last of every row as one packed sequence, then the rows' state
    const bool packed = icl && tuning().tts_packed_prompt != 0;
    if (packed && !build_only) packed_prompt(B, Pmax);
    for (int s = packed ? Pmax - 1 : 0; s < Pmax && !build_only; ++s) {
        hipLaunchKernelGGL(tts_prefill_feed_kernel, dim3(B), dim3(256), 0, stream_, st, s, Pmax, (const bf16_t*)d_pf_, P, H, d_x_,
                           (const float*)d_rope_cos_, (const float*)d_rope_sin_, d_rope_rows_, d_rope_rows_ + (size_t)MB * half, half);
        if (s + 1 < Pmax) layer_steps(tk_, d_x_, B, true, 0, false);      // the last position is the Talker step of frame 0
    }
    QASR_HIP(hipGetLastError());
    QASR_HIP(hipStreamSynchronize(stream_));                              // the host vectors above go out of scope
}

// The prompt pass of the ASR engine (Engine::run_prefill) on the Talker's layers: per layer one dequantisation of its four matrices to
// bf16 (q|k|v and gate|up are kept fused by the loader, gate|up already in the 16-row interleave the SwiGLU GEMM reads), then the
// engine's launch functions.  K rows and the V fragments land in the Talker's cache at slot = row, where the frame step reads them.
void TtsTalker::packed_prompt(int B, int Pmax) {
    const auto& c = cfg_;
    const int H = c.hidden, hd = c.head_dim, nq = c.heads * hd, nkv = c.kv_heads * hd, nh = c.heads + 2 * c.kv_heads, I = c.inter;
    const int MB = c.max_batch;
    std::vector<int> meta((size_t)2 * max_pos_ + 2 * MB + 1, 0);
    int *slot = meta.data(), *pos = slot + max_pos_, *cu = pos + max_pos_, *clip = cu + MB + 1;
    int n = 0, max_len = 0;
    for (int b = 0; b < B; ++b) {
        cu[b] = n;
        clip[b] = b;
        for (int i = 0; i + 1 < pf_len_[b]; ++i) { slot[n] = b; pos[n++] = i; }
        max_len = std::max(max_len, pf_len_[b] - 1);
    }
    cu[B] = n;
    if (n == 0 || n > max_pos_ || max_len > vt_stride_ || Pmax > max_prefill_) throw std::length_error("talker: packed prompt over the handle's capacity");
    QASR_HIP(hipMemcpyAsync(d_pmeta_, meta.data(), meta.size() * 4, hipMemcpyHostToDevice, stream_));
    const int *d_slot = d_pmeta_, *d_pos = d_pmeta_ + max_pos_, *d_cu = d_pmeta_ + 2 * (size_t)max_pos_, *d_clip = d_cu + MB + 1;
    hipStream_t s = stream_;
    hipLaunchKernelGGL(tts_pack_rows_kernel, dim3(n), dim3(128), 0, s, (const bf16_t*)d_pf_, max_prefill_, d_slot, d_pos, H, d_px_);
    bf16_t *wqkv = d_w_, *wo = wqkv + (size_t)(nq + 2 * nkv) * H, *wgu = wo + (size_t)H * nq, *wdown = wgu + (size_t)2 * I * H;
    const size_t per = (size_t)MB * c.kv_heads * max_ctx_ * hd;
    for (size_t l = 0; l < tk_.layers.size(); ++l) {
        const Layer& L = tk_.layers[l];
        KVLayout kv{d_k_ + l * per, nullptr, max_ctx_, c.kv_heads, hd, d_vf_ + l * per};
        const DequantJob jobs[4] = {{L.qkv.img.raw, 0, nq + 2 * nkv, wqkv}, {L.o.img.raw, 0, H, wo}, {L.gu.img.raw, 0, 2 * I, wgu},
                                    {L.down.img.raw, 0, H, wdown}};
        quant_dequant_multi_launch(jobs, 4, s);
        rmsnorm_rows_launch(d_px_, L.ln1, d_ph_, n, H, c.rms_eps, s);
        const bool fuse_qk = qk_norm_rope_fusable(c.heads, c.kv_heads, hd);
        if (fuse_qk)
            gemm_nt_headtiles(ADense{d_ph_, H, n, H}, wqkv, H, n, nh * hd, H,
                              EpiQkHeads{d_pqkv_, (long)nh * hd, d_pqr_, kv, d_slot, d_pos, L.qn, L.kn, c.rms_eps, d_rope_cos_, d_rope_sin_,
                                         c.heads, c.kv_heads}, s);
        else
            gemm_nt(ADense{d_ph_, H, n, H}, wqkv, H, n, nh * hd, H, EpiStoreBf16{d_pqkv_, (long)nh * hd}, s);
        qk_norm_rope_launch(d_pqkv_, d_slot, d_pos, n, c.heads, c.kv_heads, hd, L.qn, L.kn, c.rms_eps, d_rope_cos_, d_rope_sin_, d_pqr_, kv,
                            d_vt_, vt_stride_, d_cu, d_clip, B, max_len, s, fuse_qk);
        prefill_attention_launch(d_pqr_, kv, d_vt_, vt_stride_, d_cu, d_clip, B, max_len, c.heads, d_pattn_, s);
        gemm_nt(ADense{d_pattn_, nq, n, nq}, wo, nq, n, H, nq, EpiResidBf16{d_px_, H}, s);
        rmsnorm_rows_launch(d_px_, L.ln2, d_ph_, n, H, c.rms_eps, s);
        gemm_nt_swiglu(ADense{d_ph_, H, n, H}, wgu, H, n, 2 * I, H, EpiStoreBf16{d_pact_, I}, s);
        gemm_nt(ADense{d_pact_, I, n, I}, wdown, I, n, H, I, EpiResidBf16{d_px_, H}, s);
    }
    QASR_HIP(hipGetLastError());
    QASR_HIP(hipStreamSynchronize(s));                                     // `meta` goes out of scope
}

void TtsTalker::icl_prompt(const std::vector<TtsRow>& rows, float* out, int32_t* P) {
    const int B = (int)rows.size(), H = cfg_.hidden;
    if (B == 0) return;
    QASR_HIP(hipSetDevice(cfg_.device));
    prefill(rows, true);
    int Pmax = 0;
    for (int b = 0; b < B; ++b) { P[b] = pf_len_[b]; Pmax = std::max(Pmax, pf_len_[b]); }
    std::vector<bf16_t> h((size_t)B * max_prefill_ * H);
    QASR_HIP(hipMemcpyAsync(h.data(), d_pf_, h.size() * 2, hipMemcpyDeviceToHost, stream_));
    QASR_HIP(hipStreamSynchronize(stream_));
    for (int b = 0; b < B; ++b)
        for (int p = 0; p < Pmax; ++p)
            for (int i = 0; i < H; ++i)
                out[((size_t)b * Pmax + p) * H + i] = p < pf_len_[b] ? bf16_to_f32_host(h[((size_t)b * max_prefill_ + p) * H + i]) : 0.0f;
}

void TtsTalker::set_knobs(const qasr_tts_sampling& s, unsigned long long seed) {
    Knobs k{};
    k.talker = TtsSampleParams{s.temperature, s.repetition_penalty, s.eos_logit_bias, s.top_k, cfg_.suppress_lo, cfg_.suppress_hi,
                               cfg_.codec_eos, seed};
    k.cp = TtsSampleParams{s.temperature, 1.0f, 0.0f, s.top_k, 0, 0, -1, seed};
    QASR_HIP(hipMemcpyAsync(d_knobs_, &k, sizeof(k), hipMemcpyHostToDevice, stream_));
    QASR_HIP(hipStreamSynchronize(stream_));
}

void TtsTalker::generate(const std::vector<TtsRow>& rows, const qasr_tts_sampling& s, unsigned long long seed, int max_frames,
                         int32_t* codes, int32_t* n_frames) {
    const int B = (int)rows.size(), MB = cfg_.max_batch, F = cfg_.max_frames;
    if (B == 0) return;
    QASR_HIP(hipSetDevice(cfg_.device));
    max_frames = std::min(std::max(max_frames, 1), F);
    set_knobs(s, seed);
    prefill(rows);
    std::vector<int> fin(MB);
    TtsState st = state_of(d_state_, MB);
    for (int f = 0; f < max_frames; ++f) {
        run_frame(B);
        if ((f + 1) % TTS_POLL == 0 && f + 1 < max_frames) {              // the finished flags, every TTS_POLL frames
            QASR_HIP(hipMemcpyAsync(fin.data(), st.finished, (size_t)B * 4, hipMemcpyDeviceToHost, stream_));
            QASR_HIP(hipStreamSynchronize(stream_));
            if (std::all_of(fin.begin(), fin.begin() + B, [](int v) { return v != 0; })) break;
        }
    }
    // frames computed behind a row's EOS (up to the next poll) were never stored: a finished row writes no code
    std::vector<int> h((size_t)B * TTS_GROUPS * F);
    QASR_HIP(hipMemcpyAsync(h.data(), d_codes_, h.size() * 4, hipMemcpyDeviceToHost, stream_));
    QASR_HIP(hipMemcpyAsync(n_frames, st.n_frames, (size_t)B * 4, hipMemcpyDeviceToHost, stream_));
    QASR_HIP(hipStreamSynchronize(stream_));
    for (int b = 0; b < B; ++b) {
        n_frames[b] = std::min(n_frames[b], max_frames);
        for (int g = 0; g < TTS_GROUPS; ++g)
            for (int t = 0; t < F; ++t) {
                const size_t i = ((size_t)b * TTS_GROUPS + g) * F + t;
                codes[i] = t < n_frames[b] ? h[i] : -1;
            }
    }
}

void TtsTalker::forced(const std::vector<TtsRow>& rows, const TtsForcedOut& f) {
    const int B = (int)rows.size(), T = f.T;
    const auto& c = cfg_;
    if (B == 0 || T == 0) return;
    QASR_HIP(hipSetDevice(c.device));
    qasr_tts_sampling s{0.0f, 1, 1.0f, 1.0f, T, 0.0f};
    set_knobs(s, 0);
    const size_t n_codes = (size_t)B * TTS_GROUPS * T, n_tl = (size_t)B * T * c.codec_vocab,
                 n_cl = (size_t)B * T * (TTS_GROUPS - 1) * c.cp_vocab, n_h = (size_t)B * T * c.hidden;
    for (auto& fb : forced_buf_) fb = std::make_unique<DevBuf>();
    forced_buf_[0]->alloc(n_codes * 4);
    d_f_codes_ = forced_buf_[0]->as<int>();
    d_f_tlog_ = d_f_cplog_ = d_f_hid_ = nullptr;
    if (f.talker_logits) { forced_buf_[1]->alloc(n_tl * 4); d_f_tlog_ = forced_buf_[1]->as<float>(); }
    if (f.cp_logits) { forced_buf_[2]->alloc(n_cl * 4); d_f_cplog_ = forced_buf_[2]->as<float>(); }
    if (f.hidden) { forced_buf_[3]->alloc(n_h * 4); d_f_hid_ = forced_buf_[3]->as<float>(); }
    forced_T_host_ = T;
    QASR_HIP(hipMemcpyAsync(d_f_codes_, f.codes, n_codes * 4, hipMemcpyHostToDevice, stream_));
    prefill(rows);
    for (int t = 0; t < T; ++t) issue_frame(B, true);
    if (f.talker_logits) QASR_HIP(hipMemcpyAsync(f.talker_logits, d_f_tlog_, n_tl * 4, hipMemcpyDeviceToHost, stream_));
    if (f.cp_logits) QASR_HIP(hipMemcpyAsync(f.cp_logits, d_f_cplog_, n_cl * 4, hipMemcpyDeviceToHost, stream_));
    if (f.hidden) QASR_HIP(hipMemcpyAsync(f.hidden, d_f_hid_, n_h * 4, hipMemcpyDeviceToHost, stream_));
    QASR_HIP(hipStreamSynchronize(stream_));
    for (auto& fb : forced_buf_) fb.reset();
    d_f_codes_ = nullptr; d_f_tlog_ = d_f_cplog_ = d_f_hid_ = nullptr;
}

// ================================================================================================
// The stream pool's view (qasr_tts_pool_*, api_tts.cpp).  What prefill() builds for a whole call is built here for
// one slot: the slot's rows of the projected text table are rows 3 + slot * per_slot .. of d_tp_ (max_tp_ holds max_batch such blocks),
// its plan, trailing indices, x-vector, history bits, code rows and six state words are its rows of the call-wide arrays.
// ================================================================================================
void TtsTalker::pool_begin(const qasr_tts_sampling& s, unsigned long long seed) {
    const auto& c = cfg_;
    const int MB = c.max_batch;
    QASR_HIP(hipSetDevice(c.device));
    set_knobs(s, seed);
    std::vector<int> state((size_t)6 * MB, 0);
    for (int b = 0; b < MB; ++b) state[(size_t)MB + b] = 1;                 // every slot free
    const int ids[3] = {c.tts_pad, c.tts_bos, c.tts_eos};
    QASR_HIP(hipMemcpyAsync(d_state_, state.data(), state.size() * 4, hipMemcpyHostToDevice, stream_));
    QASR_HIP(hipMemcpyAsync(d_tp_ids_, ids, sizeof(ids), hipMemcpyHostToDevice, stream_));
    hipLaunchKernelGGL(tts_gather_rows_kernel, dim3(3), dim3(256), 0, stream_, text_emb_, (const int*)d_tp_ids_, c.text_hidden, d_tp_in_);
    gemv_rows(fc1_.img.raw, d_tp_in_, 3, fc1_.bias, nullptr, d_tp_mid_, c.text_hidden, true, stream_);
    gemv_rows(fc2_.img.raw, d_tp_mid_, 3, fc2_.bias, nullptr, d_tp_, c.hidden, false, stream_);
    QASR_HIP(hipGetLastError());
    QASR_HIP(hipStreamSynchronize(stream_));
}

void TtsTalker::pool_admit(int slot, const TtsRow& r) {
    const auto& c = cfg_;
    const int MB = c.max_batch, H = c.hidden, P = max_prefill_, half = c.head_dim / 2, TH = c.text_hidden;
    if (slot < 0 || slot >= MB || r.ref_codes) throw std::invalid_argument("talker: pool_admit: slot outside the handle or an ICL row");
    QASR_HIP(hipSetDevice(c.device));
    const int tp0 = 3 + slot * (c.max_text + c.max_instruct + max_ref_text_);
    std::vector<int> tp_ids, pt(P, -1), pc(P, -1), tr(c.max_text, 0);
    std::vector<float> xv(H, 0.0f);
    int nt = 0;
    const int n = plan_row(r, tp_ids, tp0, pt.data(), pc.data(), tr.data(), nt, xv.data(), nullptr);
    const int ntp = (int)tp_ids.size();
    const int words[6] = {0, 0, 0, 0, nt, n};                               // ctx_len finished n_frames frame_of trail_len pf_len
    const long long ridx = r.index;
    QASR_HIP(hipMemcpyAsync(d_tp_ids_ + tp0, tp_ids.data(), (size_t)ntp * 4, hipMemcpyHostToDevice, stream_));
    QASR_HIP(hipMemcpyAsync(d_pf_text_ + (size_t)slot * P, pt.data(), (size_t)P * 4, hipMemcpyHostToDevice, stream_));
    QASR_HIP(hipMemcpyAsync(d_pf_codec_ + (size_t)slot * P, pc.data(), (size_t)P * 4, hipMemcpyHostToDevice, stream_));
    QASR_HIP(hipMemcpyAsync(d_trail_ + (size_t)slot * c.max_text, tr.data(), (size_t)c.max_text * 4, hipMemcpyHostToDevice, stream_));
    QASR_HIP(hipMemcpyAsync(d_xvec_ + (size_t)slot * H, xv.data(), (size_t)H * 4, hipMemcpyHostToDevice, stream_));
    QASR_HIP(hipMemcpyAsync(d_row_index_ + slot, &ridx, 8, hipMemcpyHostToDevice, stream_));
    for (int w = 0; w < 6; ++w) QASR_HIP(hipMemcpyAsync(d_state_ + (size_t)w * MB + slot, &words[w], 4, hipMemcpyHostToDevice, stream_));
    QASR_HIP(hipMemsetAsync(d_seen_ + (size_t)slot * c.codec_vocab, 0, (size_t)c.codec_vocab, stream_));
    QASR_HIP(hipMemsetAsync(d_codes_ + (size_t)slot * TTS_GROUPS * c.max_frames, 0xff, (size_t)TTS_GROUPS * c.max_frames * 4, stream_));
    hipLaunchKernelGGL(tts_gather_rows_kernel, dim3(ntp), dim3(256), 0, stream_, text_emb_, (const int*)(d_tp_ids_ + tp0), TH,
                       d_tp_in_ + (size_t)tp0 * TH);
    gemv_rows(fc1_.img.raw, d_tp_in_ + (size_t)tp0 * TH, ntp, fc1_.bias, nullptr, d_tp_mid_ + (size_t)tp0 * TH, TH, true, stream_);
    gemv_rows(fc2_.img.raw, d_tp_mid_ + (size_t)tp0 * TH, ntp, fc2_.bias, nullptr, d_tp_ + (size_t)tp0 * H, H, false, stream_);
    // the one-row view: every pointer at the slot's row, the table (d_tp_) whole since the plan names its rows
    bf16_t* pf = d_pf_ + (size_t)slot * P * H;
    hipLaunchKernelGGL(tts_prefill_build_kernel, dim3(P, 1), dim3(256), 0, stream_, (const int*)(d_pf_text_ + (size_t)slot * P),
                       (const int*)(d_pf_codec_ + (size_t)slot * P), P, (const bf16_t*)d_tp_, codec_emb_, (const float*)(d_xvec_ + (size_t)slot * H),
                       H, pf, (const int*)nullptr, 0, (const bf16_t* const*)d_cp_emb_);
    TtsState st = state_of(d_state_ + slot, MB);
    bf16_t* x = d_x_ + (size_t)slot * H;
    for (int s = 0; s < n; ++s) {
        hipLaunchKernelGGL(tts_prefill_feed_kernel, dim3(1), dim3(256), 0, stream_, st, s, n, (const bf16_t*)pf, P, H, x,
                           (const float*)d_rope_cos_, (const float*)d_rope_sin_, d_rope_rows_ + (size_t)slot * half,
                           d_rope_rows_ + (size_t)(MB + slot) * half, half);
        if (s + 1 < n) layer_steps(tk_, x, 1, true, 0, false, slot);       // the last position is the Talker step of the slot's frame 0
    }
    QASR_HIP(hipGetLastError());
    QASR_HIP(hipStreamSynchronize(stream_));                              // the host vectors above go out of scope
}

void TtsTalker::pool_frames(int B, int n) {
    QASR_HIP(hipSetDevice(cfg_.device));
    for (int f = 0; f < n; ++f) run_frame(B);
}

void TtsTalker::pool_poll(int B, int* n_frames, int* finished) {
    TtsState st = state_of(d_state_, cfg_.max_batch);
    QASR_HIP(hipMemcpyAsync(n_frames, st.n_frames, (size_t)B * 4, hipMemcpyDeviceToHost, stream_));
    QASR_HIP(hipMemcpyAsync(finished, st.finished, (size_t)B * 4, hipMemcpyDeviceToHost, stream_));
    QASR_HIP(hipStreamSynchronize(stream_));
}

void TtsTalker::pool_finish(int slot) {
    const int one = 1;
    QASR_HIP(hipMemcpyAsync(state_of(d_state_, cfg_.max_batch).finished + slot, &one, 4, hipMemcpyHostToDevice, stream_));
    QASR_HIP(hipStreamSynchronize(stream_));
}

void TtsTalker::pool_codes(int slot, int f0, int n, int32_t* out) {
    const int F = cfg_.max_frames;
    if (n <= 0) return;
    if (f0 < 0 || f0 + n > F) throw std::invalid_argument("talker: pool_codes: frames outside the slot's rows");
    QASR_HIP(hipMemcpy2DAsync(out, (size_t)n * 4, d_codes_ + (size_t)slot * TTS_GROUPS * F + f0, (size_t)F * 4, (size_t)n * 4, TTS_GROUPS,
                              hipMemcpyDeviceToHost, stream_));
    QASR_HIP(hipStreamSynchronize(stream_));
}

}  // namespace qasr
