// api.cpp -- extern "C" boundary (include/qasr.h).  Exceptions never cross it.
#include "api_guard.h"
#include "engine.h"
#include "ctc_engine.h"
#include "tuning.h"
#include "codec_launch.h"
#include "codec_qwen3tts.h"
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using qasr::Engine;

// engine and Omnilingual handles keep their message in impl->last_error (api_dp.cpp and the bindings read it through qasr_last_error)
// and share one create-error slot
static std::string& error_slot(const qasr_engine* e) { return e && e->impl ? e->impl->last_error : create_error<qasr_engine>(); }

// a guarded engine entry first makes the engine's device current for the calling thread (the HIP current device is per thread: an engine
// per GPU may be driven from any thread, e.g. the worker threads of qasr_dp_*)
template <class F> static int on_device(qasr_engine* e, F&& f) {
    return guarded(e, [&] { e->impl->bind_device(); f(); });
}

static bool contains(const std::string& s, const char* sub) { return s.find(sub) != std::string::npos; }

// qasr_gemm_case_probe: why the arguments are refused, or null.  Everything a launch would index with is checked here, on the host.
static const char* gemm_case_refusal(int which, int form, const qasr_gemm_case& g, const void* bias, const int32_t* aux_i,
                                     const int64_t* aux_l, const float* aux_f) {
    if (which < QASR_GEMM_CASE_CONV || which > QASR_GEMM_CASE_SWIGLU) return "gemm case: unknown case id";
    if (form < -1 || form > 2) return "gemm case: form must be -1, 0, 1 or 2";
    if (g.M <= 0 || g.N <= 0 || g.K <= 0) return "gemm case: M, N, K must be positive";
    if (g.K % 8) return "gemm case: K must be a multiple of 8";
    if (g.N % 4) return "gemm case: N must be a multiple of 4";
    const bool grouped = which == QASR_GEMM_CASE_GROUPCONV || which == QASR_GEMM_CASE_GROUPCONV_PLAIN;
    int width = g.N;                                   // columns written per row
    if (which == QASR_GEMM_CASE_SWIGLU) {
        if (g.N % 32) return "gemm case: the swiglu width must be a multiple of 32";
        width = g.N / 2;
    }
    if (grouped) {
        if (form == 2 || form == 0) return "gemm case: the grouped launch has the single-buffer 128 x 128 form only (AGroupConv1d: no_p8)";
        if (g.KP <= 0 || g.cpg <= 0 || g.groups <= 0 || g.cpg % 8) return "gemm case: groupconv needs KP, groups > 0 and cpg a positive multiple of 8";
        if (g.N != g.cpg || (long)g.K != (long)g.KP * g.cpg) return "gemm case: groupconv needs N = cpg and K = KP * cpg";
        width = g.groups * g.cpg;
        if (!aux_i || !bias || (which == QASR_GEMM_CASE_GROUPCONV && !aux_f)) return "gemm case: groupconv needs frame records, a bias and (EpiPosConv) the residual";
        for (int m = 0; m < g.M; ++m) {                // frame m is frame t of a clip of L frames that lies inside [0, M)
            const long t = aux_i[2 * m], L = aux_i[2 * m + 1];
            if (t < 0 || t >= L || m - t < 0 || m - t + L > g.M) return "gemm case: a frame record points outside the packed frames";
        }
    }
    if (which == QASR_GEMM_CASE_CONV || which == QASR_GEMM_CASE_CONV_PLAIN) {
        if (g.n_img <= 0 || g.H <= 0 || g.W <= 0 || g.C <= 0 || g.C % 8) return "gemm case: conv needs n_img, H, W > 0 and C a positive multiple of 8";
        if (g.wide && g.C < 64) return "gemm case: the per-K-tile conv gather needs C >= 64";
        const long OH = (g.H - 1) / 2 + 1, OW = (g.W - 1) / 2 + 1;
        if ((long)g.M != g.n_img * OH * OW || (long)g.K != 9L * g.C) return "gemm case: conv needs M = n_img * OH * OW and K = 9 * C";
        if (!bias) return "gemm case: conv needs a bias";
        if (which == QASR_GEMM_CASE_CONV && (!aux_i || (g.level != 2 && g.level != 3))) return "gemm case: conv needs valid widths and level 2 or 3";
    }
    if (which == QASR_GEMM_CASE_ROWTABLE) {
        if (!aux_l || !bias || g.a_len <= 0) return "gemm case: rowtable needs offsets, a bias and a_len";
        for (int m = 0; m < g.M; ++m)
            if (aux_l[m] < 0 || aux_l[m] % 8 || aux_l[m] + g.K > g.a_len) return "gemm case: a row offset is misaligned or outside A";
    }
    if (which == QASR_GEMM_CASE_POS_F32) {
        if (!aux_i || !aux_f || g.n_t <= 0) return "gemm case: pos needs tok_t, the table and n_t";
        for (int m = 0; m < g.M; ++m)
            if (aux_i[m] < 0 || aux_i[m] >= g.n_t) return "gemm case: a position index is outside the table";
    }
    if ((which == QASR_GEMM_CASE_BIASF_BF16 || which == QASR_GEMM_CASE_BIASF_BF16_GELU || which == QASR_GEMM_CASE_RESID_F32 ||
         which == QASR_GEMM_CASE_RESID_F32F) && !bias) return "gemm case: this epilogue needs a bias";
    if (g.ld < 0 || g.out_rows < 0 || (g.ld && (g.ld % 4 || g.ld < width)) || (g.out_rows && g.out_rows < g.M))
        return "gemm case: ld must be 0 or a multiple of 4 that holds the written width, out_rows 0 or >= M";
    if (grouped && g.ld && g.ld != width) return "gemm case: groupconv output is tight ([M][groups * cpg])";
    return nullptr;
}

// qasr_attn_case_probe: why the arguments are refused, or null.  Everything a launch would index with is checked here, on the host.
static const char* attn_case_refusal(int op, const qasr_attn_case& g, const uint16_t* x, const uint16_t* W, const int32_t* cu,
                                     const int32_t* slot_of_clip, const int32_t* pos, const int32_t* slot, const uint16_t* vt,
                                     const uint16_t* qr) {
    if (op != QASR_ATTN_PROMPT && op != QASR_ATTN_DECODE) return "attn case: unknown operation";
    if (g.hd != 32 && g.hd != 128) return "attn case: head_dim must be 32 or 128";
    if (g.n_slots <= 0 || g.heads <= 0 || g.kv_heads <= 0 || g.n_pos <= 0) return "attn case: n_slots, heads, kv_heads, n_pos must be positive";
    if (g.max_ctx <= 0 || g.max_ctx % 32) return "attn case: max_ctx must be a positive multiple of 32";
    if (g.heads > 64 || g.kv_heads > 64 || g.n_pos > 65536 || (double)g.n_slots * g.kv_heads * g.max_ctx * g.hd > 64.0 * 1024 * 1024)
        return "attn case: geometry above the probe's limits (64 heads, 65536 rows, 64 Mi cache elements)";
    if (!(g.eps > 0.0f) || !(g.eps < 1.0f) || !(g.rope_theta >= 1.0f) || !(g.rope_theta <= 1e9f)) return "attn case: eps in (0, 1) and rope_theta in [1, 1e9]";
    if (!pos) return "attn case: positions are missing";
    if (op == QASR_ATTN_DECODE) {
        if (g.heads != 2 * g.kv_heads) return "attn case: decode attention is built for 2 query heads per kv head";
        if (g.n_pos > g.n_slots) return "attn case: more batch rows than slots";
        if (g.route != 0) return "attn case: decode has no route";
        for (int b = 0; b < g.n_pos; ++b)
            if (pos[b] < 0 || pos[b] >= g.max_ctx) return "attn case: a context length is outside [0, max_ctx - 1]";
        return nullptr;
    }
    if (!cu || !slot_of_clip || !slot || !vt || !qr) return "attn case: prompt needs cu, slot_of_clip, slot, vt and qr";
    if (g.max_ctx % 64) return "attn case: the prompt pass moves 64-key tiles, max_ctx must be a multiple of 64";
    if (g.heads % g.kv_heads) return "attn case: heads must be a multiple of kv_heads";
    const int nh = g.heads + 2 * g.kv_heads;
    if (g.hd == 128 ? nh % 2 != 0 : nh % 8 != 0) return "attn case: head count the q/k norm + rope kernels do not take";
    if (g.route < 0 || g.route > 2) return "attn case: route must be 0, 1 or 2";
    if (g.route) {
        if (!x || !W || g.hidden <= 0 || g.hidden % 8 || g.hidden > 8192) return "attn case: routes 1 and 2 need x, W and hidden a multiple of 8 up to 8192";
        if (g.route == 2 && (g.hd != 128 || (g.heads + g.kv_heads) % 8)) return "attn case: the head-tile route needs head_dim 128 and (heads + kv_heads) % 8 == 0";
    }
    if (g.n_clips <= 0 || g.n_clips > g.n_slots) return "attn case: n_clips must be in [1, n_slots]";
    if (cu[0] != 0) return "attn case: cu must start at 0";
    for (int c = 0; c < g.n_clips; ++c) {
        if (cu[c + 1] <= cu[c]) return "attn case: cu must increase";
        if (cu[c + 1] > g.n_pos) return "attn case: cu runs past n_pos";
        if (cu[c + 1] - cu[c] > g.max_ctx) return "attn case: a clip is longer than max_ctx";
        if (slot_of_clip[c] < 0 || slot_of_clip[c] >= g.n_slots) return "attn case: a clip's slot is outside n_slots";
        for (int d = 0; d < c; ++d)
            if (slot_of_clip[d] == slot_of_clip[c]) return "attn case: two clips share a slot";
        for (int p = cu[c]; p < cu[c + 1]; ++p)
            if (slot[p] != slot_of_clip[c] || pos[p] != p - cu[c]) return "attn case: pos / slot contradict cu";
    }
    if (cu[g.n_clips] != g.n_pos) return "attn case: cu must end at n_pos";
    return nullptr;
}

// qasr_syn_attn_case_probe: why the arguments are refused, or null.  Everything a launch would index with is checked here, on the host, and
// the element counts the caller states for its arrays must be the geometry's.
static const char* syn_attn_case_refusal(int op, const qasr_syn_attn_case& g, const void* qkv, const int32_t* slot, const int32_t* pos,
                                         const uint16_t* qn_w, const uint16_t* kn_w, const float* cos, const float* sin, const uint16_t* kcache,
                                         const uint16_t* vcache, const uint16_t* qr, const void* out) {
    if (op != QASR_SYN_CVLM && op != QASR_SYN_CP && op != QASR_SYN_VL) return "syn attn case: unknown operation";
    if (!qkv || !cos || !sin || !out) return "syn attn case: qkv, cos, sin or out is missing";
    if (g.heads < 1 || g.kv_heads < 1 || g.heads > 64) return "syn attn case: heads in [1, 64], kv_heads positive";
    if (g.heads % g.kv_heads) return "syn attn case: heads must be a multiple of kv_heads";
    if (g.rows < 1 || g.out_rows < g.rows || g.out_rows > 65536) return "syn attn case: rows positive, out_rows in [rows, 65536]";
    if (g.n_table < 1 || g.n_table > 32768) return "syn attn case: n_table in [1, 32768]";
    const int64_t nh = g.heads + 2 * g.kv_heads;
    if (op == QASR_SYN_CVLM) {
        if (g.heads / g.kv_heads > 16) return "syn attn case: the CosyVoice attention serves at most 16 query heads per kv head";
        if (!slot || !pos || !kcache || !vcache || !qr) return "syn attn case: slot, pos, the caches or qr is missing";
        if (g.n_slots < 1 || g.max_ctx < 1 || g.rows > 4096 || (double)g.n_slots * g.kv_heads * g.max_ctx * 64 > 64.0 * 1024 * 1024)
            return "syn attn case: geometry above the probe's limits (4096 rows, 64 Mi cache elements)";
        for (int r = 0; r < g.rows; ++r) {
            if (slot[r] < 0 || slot[r] >= g.n_slots) return "syn attn case: a slot is outside the cache";
            if (pos[r] < 0 || pos[r] >= g.max_ctx || pos[r] >= g.n_table) return "syn attn case: a position is outside the cache or the rope tables";
            for (int q = 0; q < r; ++q)
                if (slot[q] == slot[r] && pos[q] == pos[r]) return "syn attn case: two rows share a cache row";
        }
        if (g.qkv_elems != g.rows * nh * 64 || g.cache_elems != (int64_t)g.n_slots * g.kv_heads * g.max_ctx * 64 ||
            g.out_elems != (int64_t)g.out_rows * g.heads * 64 || g.table_elems != (int64_t)g.n_table * 32)
            return "syn attn case: an array's size contradicts the geometry";
        return nullptr;
    }
    if (op == QASR_SYN_CP) {
        if (!qn_w || !kn_w || !kcache || !vcache) return "syn attn case: the norm weights or the caches are missing";
        if (g.pos < 0 || g.pos >= 16 || g.pos >= g.n_table) return "syn attn case: the code predictor's position is outside 0 .. 15 or the rope tables";
        if (g.max_ctx != 16 || g.n_slots < g.rows || g.n_slots > 65536) return "syn attn case: the code predictor's cache holds 16 entries for each of n_slots >= rows rows";
        if (!(g.eps > 0.0f) || !(g.eps < 1.0f)) return "syn attn case: eps in (0, 1)";
        if (g.qkv_elems != g.rows * nh * 128 || g.cache_elems != (int64_t)g.n_slots * g.kv_heads * 16 * 128 ||
            g.out_elems != (int64_t)g.out_rows * g.heads * 128 || g.table_elems != (int64_t)g.n_table * 64)
            return "syn attn case: an array's size contradicts the geometry";
        return nullptr;
    }
    if (g.S < 1 || g.S > 32 || g.S > g.n_table) return "syn attn case: S outside 1 .. 32 or the rope tables";
    if ((g.heads * 128) % 512) return "syn attn case: heads x 128 must be a multiple of 512";
    if (g.n_seq < 1 || (int64_t)g.n_seq * g.S != g.rows) return "syn attn case: rows must equal n_seq * S";
    if (g.qkv_elems != g.rows * nh * 128 || g.out_elems != (int64_t)g.out_rows * g.heads * 128 || g.table_elems != (int64_t)g.n_table * 128)
        return "syn attn case: an array's size contradicts the geometry";
    return nullptr;
}

// qasr_codec_case_probe: why the arguments are refused, or null.  The locator arrays are held to their contracts (codec_shared.h), then every
// output row's span is formed as the locator forms it and must lie inside A.
static const char* codec_case_refusal(int op, const qasr_codec_case& g, const float* A, const float* Wt, const float* bias, const float* sa,
                                      const float* sb, const float* ls, const float* R, const int32_t* la, const int32_t* lb, const float* out) {
    if (op < QASR_CODEC_TILE || op > QASR_CODEC_VAE_UNIT) return "codec case: unknown operation";
    if ((!A && op != QASR_CODEC_GATHER && op != QASR_CODEC_VQ) || !Wt || !out) return "codec case: A, Wt or out is missing";
    const int lim = 1 << 20;
    if (g.M < 1 || g.M > lim || g.a_rows < 1 || g.a_rows > lim || g.out_extra < 0 || g.out_extra > lim)
        return "codec case: M, a_rows in [1, 2^20], out_extra in [0, 2^20]";
    const int kind = g.rows_kind;
    if (op == QASR_CODEC_RMS) {
        if (g.C < 1 || g.C > 65536 || g.a_rows < g.M) return "codec case: rms needs C in [1, 65536] and a_rows >= M";
        if (!(g.eps > 0.0f) || !(g.eps < 1.0f)) return "codec case: eps in (0, 1)";
        return nullptr;
    }
    if (op == QASR_CODEC_GATHER) {
        if (g.Q < 1 || g.Q > 64 || g.C < 1 || g.C > 4096 || g.S0 < 1 || g.S0 > 65536 || g.S1 < 1 || g.S1 > 65536)
            return "codec case: gather needs Q in [1, 64], C in [1, 4096], S0 and S1 in [1, 65536]";
        if (!la || (long)g.n_loc != (long)g.M * g.Q) return "codec case: gather needs codes [M][Q]";
        for (long m = 0; m < g.M; ++m)
            for (int q = 0; q < g.Q; ++q) {
                const int code = la[m * g.Q + q];
                if (code < 0 || code >= (q == 0 ? g.S0 : g.S1)) return "codec case: a code is outside its codebook";
            }
        return nullptr;
    }
    if (op == QASR_CODEC_ATTN_DEC || op == QASR_CODEC_ATTN_ENC) {
        if (g.hd != 64) return "codec case: the codec attention kernels serve head_dim 64";
        if (g.heads < 1 || g.heads > 64 || g.n_table < 1 || g.n_table > 65536 || g.a_rows < g.M) return "codec case: heads in [1, 64], n_table in [1, 65536], a_rows >= M";
        const int per = op == QASR_CODEC_ATTN_DEC ? 2 : 4;
        if (!la || g.n_clips < 1 || g.n_clips > g.M || g.n_loc != per * g.n_clips) return "codec case: attention needs its windows / tiles";
        long row = 0;                                  // windows / clips lie back to back from row 0 to M
        if (op == QASR_CODEC_ATTN_DEC) {
            for (int w = 0; w < g.n_clips; ++w) {
                const int T = la[2 * w], off = la[2 * w + 1];
                if (T < 1 || T > qasr::CODEC_MAX_T || T > g.n_table) return "codec case: a window holds 1 .. CODEC_MAX_T frames inside the rope table";
                if (off != row) return "codec case: windows must lie back to back from row 0";
                row += T;
            }
        } else {
            int w = 0;
            while (w < g.n_clips) {                    // a clip's tiles: first query 0, 32, .. below its frames
                const int row0 = la[4 * w], F = la[4 * w + 1];
                if (row0 != row || F < 1 || F > g.n_table || row + F > g.M) return "codec case: clips must lie back to back from row 0, inside M and the rope table";
                for (int q0 = 0; q0 < F; q0 += 32, ++w)
                    if (w >= g.n_clips || la[4 * w] != row0 || la[4 * w + 1] != F || la[4 * w + 2] != q0)
                        return "codec case: a clip needs one tile per 32 queries, in order";
                row += F;
            }
        }
        if (row != g.M) return "codec case: the windows / clips must end at M";
        return nullptr;
    }
    if (op == QASR_CODEC_VQ) {
        if (g.Q < 1 || g.Q > 64 || g.C < 1 || g.C > 4096 || g.S0 < 1 || g.S0 > 65536 || g.S1 < 1 || g.S1 > 65536)
            return "codec case: the quantiser needs Q in [1, 64], C in [1, 4096], S0 and S1 in [1, 65536]";
        if (!bias || !sa || !lb) return "codec case: the quantiser needs the first codebook's transpose and norms, and codes";
        if (g.Q > 1 && (!sb || !ls || !R)) return "codec case: the quantiser needs the later codebooks, their transposes and norms";
        if ((long)g.n_loc != ((long)g.M + g.out_extra) * g.Q) return "codec case: codes must hold [M + out_extra][Q]";
        return nullptr;
    }
    if (op == QASR_CODEC_CENC_IN) {
        if (g.C < 1 || g.C > 65536 || g.a_rows < g.M) return "codec case: the input conv needs C in [1, 65536] and a_rows >= M";
        if (!la || !bias || g.n_clips < 1 || g.n_clips > g.M || g.n_loc != g.n_clips + 1) return "codec case: the input conv needs its bias and n_clips + 1 clip starts";
        if (la[0] != 0 || la[g.n_clips] != g.M) return "codec case: the clip starts must run from 0 to M";
        for (int c = 0; c < g.n_clips; ++c)
            if (la[c + 1] <= la[c]) return "codec case: the clip starts must increase";
        return nullptr;
    }
    if (kind < QASR_CODEC_ROWS_WINDOW || kind > QASR_CODEC_ROWS_VAE_STRIDE) return "codec case: unknown row locator";
    if (op == QASR_CODEC_OUT) {
        if (kind != QASR_CODEC_ROWS_WINDOW && kind != QASR_CODEC_ROWS_TAIL) return "codec case: the output conv runs under WindowRows or TailRows";
        if (g.C < 1 || g.C > 65536 || g.a_rows < g.M || (g.clip != 0 && g.clip != 1)) return "codec case: the output conv needs C in [1, 65536], a_rows >= M, clip 0 or 1";
        if (!bias || !sa || !sb) return "codec case: the output conv needs its bias and snake";
    }
    if (g.rate < 1 || g.rate > 64 || g.stride < 1 || g.stride > 64) return "codec case: rate and stride in [1, 64]";
    // the locator's arrays
    const bool frames = kind != QASR_CODEC_ROWS_CLIP;
    if (frames) {
        const int nf = (g.M + g.rate - 1) / g.rate;
        if (!la || g.n_loc != nf) return "codec case: fstart must hold ceil(M / rate) entries";
        for (int f = 0; f < nf; ++f)
            if (la[f] != f && (f == 0 || la[f] != la[f - 1])) return "codec case: fstart[f] must be f or fstart[f - 1]";
        if (kind == QASR_CODEC_ROWS_TAIL) {
            if (!lb || g.lead < 0 || g.lead > lim) return "codec case: TailRows needs kept and lead in [0, 2^20]";
            int end = nf - 1;                          // the last frame row of f's window, walking backwards
            for (int f = nf - 1; f >= 0; --f) {
                if (f + 1 < nf && la[f + 1] != la[f]) end = f;
                if (lb[f] < la[f] || lb[f] > end) return "codec case: kept must lie inside its window's frame rows";
                if (f > 0 && la[f] == la[f - 1] && lb[f] != lb[f - 1]) return "codec case: kept must be one value per window";
            }
        }
    } else if (la || lb) {
        if (!la || !lb || g.n_clips < 1 || g.n_clips > g.M || g.n_loc != g.n_clips + 1) return "codec case: ClipRows needs ostart, istart and n_loc = n_clips + 1";
        if (la[0] != 0 || la[g.n_clips] != g.M) return "codec case: ostart must run from 0 to M";
        if (lb[0] < 0) return "codec case: istart points outside";
        for (int c = 0; c < g.n_clips; ++c) {
            if (la[c + 1] <= la[c]) return "codec case: ostart must increase";
            if (lb[c + 1] < lb[c] || lb[c + 1] > g.a_rows) return "codec case: istart must not decrease and must stay inside A";
        }
    } else if (g.n_loc != 0) {
        return "codec case: n_loc without locator arrays";
    }
    // every output row's span, as the locator forms it
    auto span_ok = [&](long m) {
        long last, first;
        if (kind == QASR_CODEC_ROWS_WINDOW || kind == QASR_CODEC_ROWS_TAIL) { last = m; first = (long)la[m / g.rate] * g.rate; }
        else if (kind == QASR_CODEC_ROWS_VAE_STRIDE) { last = (m + 1) * g.stride - 1; first = (long)la[m / g.rate] * g.rate * g.stride; }
        else if (!la) { last = m; first = 0; }
        else {
            int c = 0;
            while (c + 1 < g.n_clips && la[c + 1] <= m) ++c;
            first = lb[c];
            last = first + (m - la[c]) * g.stride;
        }
        return first >= 0 && last >= 0 && last < g.a_rows;
    };
    for (long m = 0; m < g.M; ++m)
        if (!span_ok(m)) return "codec case: an output row would read outside A";
    if (op == QASR_CODEC_OUT) return nullptr;
    if (op == QASR_CODEC_VAE_UNIT) {
        if (kind != QASR_CODEC_ROWS_WINDOW) return "codec case: the AudioVAE's fused unit runs under WindowRows";
        if (g.C < 4 || g.C > 128 || (g.C & 3)) return "codec case: the fused unit holds C a multiple of 4 up to AV_FUSE_MAX";
        if (g.dil < 1 || g.dil > 9 || g.a_rows < g.M) return "codec case: the fused unit needs dil in [1, 9] and a_rows >= M";
        if ((sa == nullptr) != (sb == nullptr)) return "codec case: the map needs both a and 1 / a";
        if (ls && !sa) return "codec case: an affine without the map";
        if (bias || R) return "codec case: the fused unit takes its parameters packed in Wt";
        return nullptr;
    }
    if (op == QASR_CODEC_VAE_DW) {
        if (kind != QASR_CODEC_ROWS_WINDOW) return "codec case: the AudioVAE's depthwise conv runs under WindowRows";
        if (g.C < 1 || g.C > 65536 || g.dil < 1 || g.dil > 27 || g.a_rows < g.M) return "codec case: the AudioVAE's depthwise conv needs C in [1, 65536], dil in [1, 27], a_rows >= M";
        if (!bias || (g.snake != 0 && g.snake != 1)) return "codec case: the AudioVAE's depthwise conv needs its bias; snake is 0 or 1";
        if (g.snake && (!sa || !sb || !ls || !R)) return "codec case: the snakes need a1, 1 / a1, a2, 1 / a2";
        return nullptr;
    }
    if (op == QASR_CODEC_DWLN) {
        if (kind != QASR_CODEC_ROWS_WINDOW && kind != QASR_CODEC_ROWS_CLIP) return "codec case: the depthwise conv runs under WindowRows or ClipRows";
        if (kind == QASR_CODEC_ROWS_CLIP && (!la || g.stride != 1)) return "codec case: the depthwise conv under ClipRows needs clip starts and stride 1";
        if (kind == QASR_CODEC_ROWS_CLIP)
            for (int c = 0; c <= g.n_clips; ++c)
                if (la[c] != lb[c]) return "codec case: the depthwise conv's input and output rows are the same";
        if (g.C < 1 || g.C > 4096) return "codec case: the depthwise conv holds a row of at most 4096 channels";
        if (!bias || !sa || !sb) return "codec case: the depthwise conv needs its bias and the LayerNorm's weight and bias";
        return nullptr;
    }
    if (!qasr::codec_tile_served(kind, g.snake != 0, g.epi) || (g.snake != 0 && g.snake != 1))
        return "codec case: no codec_gemm_kernel for this (row locator, snake, epilogue)";
    if (g.Cin < 1 || g.Cin > 65536 || g.N < 1 || g.N > 65536 || g.taps < 1 || g.taps > 64 || g.dil < 1 || g.dil > 64)
        return "codec case: Cin, N in [1, 65536], taps, dil in [1, 64]";
    if ((long)g.K != (long)g.taps * g.Cin) return "codec case: K must be taps * Cin";
    if (kind == QASR_CODEC_ROWS_CLIP && !la && g.taps != 1) return "codec case: independent rows take one tap";
    const int epi = g.epi;
    if (epi == qasr::E_SWIGLU && (g.N & 1)) return "codec case: E_SWIGLU needs an even N";
    if (g.ldc < (epi == qasr::E_SWIGLU ? g.N / 2 : g.N) || g.ldc > 65536) return "codec case: ldc below the columns written";
    if (bias && (g.bmod < 1 || g.bmod > g.N)) return "codec case: bmod in [1, N]";
    if (g.snake && (!sa || !sb)) return "codec case: the snake load needs its a and b";
    if (epi == qasr::E_RESMAP && (!sa || !sb)) return "codec case: E_RESMAP needs the map's a and b";
    if (epi == qasr::E_LSRES && !ls) return "codec case: E_LSRES needs ls";
    const bool residual = epi == qasr::E_RES || epi == qasr::E_LSRES || epi == qasr::E_RESMAP;
    if (g.in_place != 0 && g.in_place != 1) return "codec case: in_place is 0 or 1";
    if (g.in_place && (!residual || R)) return "codec case: in_place needs a residual epilogue and no R";
    if ((epi == qasr::E_RES || epi == qasr::E_LSRES) && !g.in_place && !R) return "codec case: a residual epilogue needs R or in_place";
    if (!residual && R) return "codec case: R without a residual epilogue";
    return nullptr;
}

// qasr_enc_case_probe: why the arguments are refused, or null.  Everything a launch would index with is checked here, on the host.
static const char* enc_case_refusal(int op, const qasr_enc_case& g, const void* in, const int32_t* idx, const int64_t* off, const float* pf,
                                    const uint16_t* pw) {
    if (op < QASR_ENC_MHA || op > QASR_ENC_FRAME_INFO) return "enc case: unknown operation";
    if (g.rows < 0 || g.rows > (1 << 22) || g.in_extra < 0 || g.in_extra > 4096 || g.out_extra < 0 || g.out_extra > 4096)
        return "enc case: rows in [0, 2^22], in_extra / out_extra in [0, 4096]";
    const bool attn = op == QASR_ENC_MHA || op == QASR_ENC_WINDOW;
    const bool norm = op == QASR_ENC_LN_BF16 || op == QASR_ENC_LN_GELU_BF16 || op == QASR_ENC_LN_GELU_F32;
    const bool clips = attn || op == QASR_ENC_CONV0 || op == QASR_ENC_CONV_ROWS || op == QASR_ENC_FRAME_INFO;
    if (clips && (g.n_clips <= 0 || g.n_clips > 4096 || !idx)) return "enc case: n_clips in [1, 4096] and the index array";
    if (op != QASR_ENC_CONV_ROWS && op != QASR_ENC_FRAME_INFO && !in) return "enc case: the input array is missing";
    if (attn) {
        if (g.hd != 32 && g.hd != 64) return "enc case: head_dim must be 32 or 64";
        if (g.heads <= 0 || g.heads > 64) return "enc case: heads in [1, 64]";
        if (op == QASR_ENC_MHA && g.hd == 32 && qasr::tuning().mha_form != 0)
            return "enc case: head_dim 32 has the 16x16x32 form only: set mha_form 0 (the launcher would run it whatever the knob says)";
        if (idx[0] != 0) return "enc case: cu must start at 0";
        for (int c = 0; c < g.n_clips; ++c) {
            if (idx[c + 1] <= idx[c]) return "enc case: cu must increase";
            if (idx[c + 1] > g.rows) return "enc case: cu runs past rows";
            if (op == QASR_ENC_MHA && idx[c + 1] - idx[c] > g.max_len) return "enc case: max_len is smaller than a clip";
            if (op == QASR_ENC_WINDOW && idx[c + 1] - idx[c] > 128) return "enc case: a window is longer than 128 rows";
        }
        if (idx[g.n_clips] != g.rows) return "enc case: cu must end at rows";
        if (op == QASR_ENC_MHA && (g.max_len <= 0 || g.max_len > (1 << 20))) return "enc case: max_len in [1, 2^20]";
    }
    if (norm) {
        if (g.D <= 0 || g.D % 4 || g.D > 2048) return "enc case: the norms take a width that is a multiple of 4 up to 2048";
        if (!pf || !(g.eps > 0.0f) || !(g.eps < 1.0f)) return "enc case: the norms need gamma | beta and eps in (0, 1)";
    }
    if (op == QASR_ENC_CONV0 || op == QASR_ENC_WAVE_STATS) {
        const int B = op == QASR_ENC_CONV0 ? g.n_clips : g.rows;
        if (g.n_in <= 0 || !off || !idx || !(g.eps > 0.0f) || !(g.eps < 1.0f)) return "enc case: pcm, pcm_off, the lengths and eps in (0, 1)";
        if (B > 4096) return "enc case: at most 4096 clips";
        for (int b = 0; b < B; ++b) {
            // CONV0 reads the 5 n_out + 5 samples of its frames (kernel 10, stride 5); WAVE_STATS its n samples
            const long n = op == QASR_ENC_CONV0 ? 5L * idx[g.n_clips + b] + 5 : idx[b];
            const long cnt = op == QASR_ENC_CONV0 ? idx[g.n_clips + b] : idx[b];
            if (cnt < 0) return "enc case: a negative length";
            if (off[b] < 0 || off[b] > g.n_in || (cnt > 0 && off[b] + n > g.n_in)) return "enc case: a pcm offset or range lies outside the pcm array";
        }
    }
    if (op == QASR_ENC_CONV0) {
        if (g.D <= 0 || g.D > 1024) return "enc case: conv0 takes 1 to 1024 channels";
        if (!pf || g.max_len <= 0) return "enc case: conv0 needs its parameters and max_out > 0";
        for (int b = 0; b < g.n_clips; ++b) {
            const long f0 = idx[b], nf = idx[g.n_clips + b];
            if (nf > g.max_len) return "enc case: max_out is smaller than a clip's frames";
            if (f0 < 0 || f0 + nf > g.rows) return "enc case: a clip's frames lie outside the output rows";
        }
    }
    if (op == QASR_ENC_CONV1) {
        if (g.D <= 0 || g.D % 8 || g.D > 1024) return "enc case: conv1 takes a channel count that is a multiple of 8 up to 1024";
        if (!pf || !pw || !idx || g.rows <= 0) return "enc case: conv1 needs bias, weights and chunk records";
        if (g.n_mels <= 0 || g.n_mels > 256 || g.mel_stride <= 0 || g.H1 <= 0 || g.H1 > 256 || g.W1 <= 0 || g.W1 > 256 || g.n_in <= 0)
            return "enc case: conv1 geometry (n_mels, H1, W1 in [1, 256], mel_stride, n_in > 0)";
        if ((3L * (2 * g.W1 + 2) + 10L * g.D) * 4 > 64 * 1024) return "enc case: conv1 shared memory above 64 KiB";
        if ((double)g.rows * g.H1 * g.W1 * g.D > 64.0 * 1024 * 1024) return "enc case: conv1 output above 64 Mi elements";
        for (int i = 0; i < g.rows; ++i) {
            const long clip = idx[9 * i], t0 = idx[9 * i + 1], clen = idx[9 * i + 2];
            if (clip < 0 || t0 < 0 || clen < 0 || clip > 4096) return "enc case: a chunk record is negative";
            const long cols = clen < 2L * g.W1 + 1 ? clen : 2L * g.W1 + 1;      // columns iw < min(clen, 2 W1 + 1) are read
            if (t0 + cols > g.mel_stride || ((clip + 1) * g.n_mels - 1) * g.mel_stride + t0 + cols > g.n_in)
                return "enc case: a chunk record reads outside the mel array";
        }
    }
    if (op == QASR_ENC_ARGMAX && (g.D <= 0 || g.ld < g.D || (double)g.ld * (g.rows + g.in_extra) > 64.0 * 1024 * 1024))
        return "enc case: argmax needs n > 0, ld >= n and at most 64 Mi elements";
    if (op == QASR_ENC_CAST && g.rows % 4) return "enc case: the cast takes an element count that is a multiple of 4";
    if (op == QASR_ENC_CONV_ROWS && (g.stride <= 0 || g.D <= 0)) return "enc case: conv rows need stride and C > 0";
    return nullptr;
}

// qasr_dec_case_probe: why the arguments are refused, or null.  Everything a launch would index with is checked here, on the host.
static const char* dec_case_refusal(int op, const qasr_dec_case& g, const uint16_t* X, const void* W, const void* scales, const void* biases,
                                    const uint16_t* norm_w, const uint16_t* out, const float* logits, const float* part_val,
                                    const int32_t* part_idx, const int32_t* state, const float* rope, const float* rope_rows) {
    if (op < QASR_DEC_GEMV || op > QASR_DEC_EMBED) return "dec case: unknown operation";
    if (op == QASR_DEC_FINALIZE || op == QASR_DEC_EMBED) {
        if (g.B < 1 || g.B > 64 || g.out_extra < 0 || g.out_extra > 64) return "dec case: B must be in [1, 64], out_extra in [0, 64]";
        if (!W || !out || !state) return "dec case: the table, out and the int32 array are missing";
        if (g.N <= 0 || g.K <= 0 || g.K % 8 || g.K > 8192 || (double)g.N * g.K > 268435456.0) return "dec case: table rows > 0, hidden a multiple of 8 up to 8192";
        if (g.bits != 0) {
            if (g.bits != 4 && g.bits != 8) return "dec case: bits must be 0 (bf16 table), 4 or 8";
            if (g.sb_f32 != 0 && g.sb_f32 != 1) return "dec case: sb_f32 must be 0 or 1";
            if (g.K % 64 || !scales || !biases) return "dec case: a quantised table needs hidden % 64 == 0, scales and biases";
        }
        const int R = g.B + g.out_extra;
        if (op == QASR_DEC_EMBED) {
            if (g.epi < 0 || g.epi > 2) return "dec case: EMBED epi 0 splice, 1 gather, 2 dequantise rows";
            if (g.n_audio < 0 || g.n_audio > 65536) return "dec case: n_audio in [0, 65536]";
            if (g.epi == 2) {
                if (!g.bits) return "dec case: dequantised rows need a quantised table";
                return g.r0 < 0 || (long)g.r0 + g.B > g.N ? "dec case: the dequantised rows lie outside the table" : nullptr;
            }
            for (int p = 0; p < g.B; ++p) {
                const int a = g.epi == 0 ? state[g.B + p] : -1;
                if (a >= 0 && (!X || a >= g.n_audio)) return "dec case: an audio row outside the audio rows";
                if (a < 0 && (state[p] < 0 || state[p] >= g.N)) return "dec case: a row id outside the table";
            }
            return nullptr;
        }
        if (!part_val || !part_idx || !rope || !rope_rows) return "dec case: partials and rope arrays are missing";
        if (g.n_parts < 1 || g.n_parts > 4096) return "dec case: n_parts in [1, 4096]";
        if ((long)g.part_cap < (long)g.B * g.n_parts) return "dec case: part_cap is below B * n_parts";
        if (g.max_new < 1 || g.max_new > 4096 || g.clear_words < 0 || g.clear_words > 4096) return "dec case: max_new in [1, 4096], clear_words in [0, 4096]";
        if (g.half < 1 || g.half > 256 || g.n_rope < 1 || g.n_rope > 65536) return "dec case: half in [1, 256], n_rope in [1, 65536]";
        if (g.advance_ctx != 0 && g.advance_ctx != 1) return "dec case: advance_ctx must be 0 or 1";
        const int32_t* lens = state + (long)R * (g.max_new + 1);
        for (int b = 0; b < g.B; ++b) {
            if (lens[b] < 0 || lens[b] > g.max_new) return "dec case: a row's length outside [0, max_new]";
            const long next = (long)lens[2 * R + b] + g.advance_ctx;
            if (lens[2 * R + b] < 0 || next >= g.n_rope) return "dec case: a row's next position lies outside the rope table";
        }
        return nullptr;
    }
    const bool quant = op == QASR_DEC_GEMVQ || op == QASR_DEC_LMHEADQ, head = op == QASR_DEC_LMHEAD || op == QASR_DEC_LMHEADQ;
    const bool gemv = op == QASR_DEC_GEMV || op == QASR_DEC_GEMVQ;
    if (g.B < 1 || g.B > 64) return "dec case: B must be in [1, 64]";
    if (g.in_extra < 0 || g.in_extra > 64 || g.out_extra < 0 || g.out_extra > 64) return "dec case: in_extra / out_extra in [0, 64]";
    if (!X) return "dec case: the activation rows are missing";
    if (g.K <= 0 || g.K > 8192) return "dec case: K in [1, 8192]";
    if (!(g.eps > 0.0f) || !(g.eps < 1.0f)) return "dec case: eps in (0, 1)";
    if (op == QASR_DEC_RMSNORM_ROWS) {
        if (g.K % 8 || g.K > 2048) return "dec case: rmsnorm rows take a width that is a multiple of 8 up to 2048";
        if (!norm_w || !out) return "dec case: rmsnorm rows need the weight and out";
        if (g.epi != 0) return "dec case: rmsnorm rows have no epilogue";
        return nullptr;
    }
    if (!W) return "dec case: the weight is missing";
    if (g.generic != 0 && g.generic != 1) return "dec case: generic must be 0 or 1";
    if (g.N <= 0 || (double)g.N * g.K > 268435456.0) return "dec case: N > 0 and at most 2^28 weight elements";
    if (quant) {
        if (g.bits != 4 && g.bits != 8) return "dec case: bits must be 4 or 8";
        if (g.sb_f32 != 0 && g.sb_f32 != 1) return "dec case: sb_f32 must be 0 or 1";
        if (g.K % 64) return "dec case: a quantised K must be a multiple of the group size 64";
        if (!g.generic && g.K % 128) return "dec case: the packed quantised image needs K % 128 == 0 (set generic)";
        if (!scales || !biases) return "dec case: scales / biases are missing";
    } else if (g.K % 32) return "dec case: K must be a multiple of 32";
    if (norm_w && (g.K % 8 || g.K > 2048)) return "dec case: the norm takes K up to 2048";
    const int epi = head ? QASR_DEC_EPI_LOGITS : g.epi;
    if (gemv && (g.epi < QASR_DEC_EPI_BF16 || g.epi > QASR_DEC_EPI_LOGITS)) return "dec case: unknown epilogue";
    if (head && g.epi != 0) return "dec case: the LM heads have no epilogue choice";
    if (op == QASR_DEC_GEMVQ && epi == QASR_DEC_EPI_LOGITS) return "dec case: the quantised linear has no LOGITS epilogue (LMHEADQ is the head)";
    if (g.N % (epi == QASR_DEC_EPI_SWIGLU ? 32 : 16)) return "dec case: N must be a multiple of the epilogue's row tile (16; SWIGLU 32)";
    if (epi != QASR_DEC_EPI_LOGITS) return out ? nullptr : "dec case: out is missing";
    if (!logits || !part_val || !part_idx) return "dec case: logits and the partial arrays are missing";
    int parts;
    if (head) {
        if (!norm_w) return "dec case: the LM heads need the final norm's weight";
        const int rows = quant ? qasr::lm_head_q_rows(g.N, g.K, g.bits) : qasr::lm_head_rows(g.N, g.K);
        parts = quant ? qasr::lm_head_q_parts(g.N, g.K, g.bits) : qasr::lm_head_parts(g.N, g.K);
        const bool persistent = !g.generic && rows < (1 << 30);
        if (persistent && g.B > rows) return "dec case: more batch rows than one LM-head launch holds at this hidden size";
        if (persistent && g.N / 16 < 8 * parts) return "dec case: the persistent LM head needs a tile for every wave of its grid";
        if (!persistent) parts = quant ? 1 : qasr::decode_gemv_blocks(qasr::DEC_EPI_LOGITS, g.N);
    } else parts = qasr::decode_gemv_blocks(qasr::DEC_EPI_LOGITS, g.N);
    if (g.part_cap < 0 || (long)g.part_cap < (long)g.B * parts) return "dec case: part_cap is below B * partials per row";
    return nullptr;
}

extern "C" {

int qasr_default_config(const char* preset, qasr_config* c) {
    if (!c) return QASR_ERR_INVALID;
    std::string p = preset ? preset : "0.6B";
    std::memset(c, 0, sizeof(*c));
    // Qwen3AudioEncoderConfig.small (AudioEncoder.swift:28-45), TextDecoderConfig.small (Configuration.swift:68-79)
    c->enc_d_model = 896; c->enc_heads = 14; c->enc_ffn = 3584; c->enc_layers = 18; c->n_mels = 128;
    c->enc_out_dim = 1024; c->conv_channels = 480; c->n_window = 50; c->n_window_infer = 800; c->ln_eps = 1e-5f;
    c->vocab = 151936; c->hidden = 1024; c->dec_layers = 28; c->heads = 16; c->kv_heads = 8; c->head_dim = 128;
    c->inter = 3072; c->rms_eps = 1e-6f; c->rope_theta = 1000000.0f; c->group_size = 64; c->bits = 4;
    c->tok_im_start = 151644; c->tok_im_end = 151645; c->tok_audio_start = 151669; c->tok_audio_end = 151670;
    c->tok_audio_pad = 151676; c->tok_asr_text = 151704; c->tok_newline = 198; c->tok_system = 8948;
    c->tok_user = 872; c->tok_assistant = 77091;
    c->fft_scale = 2.0f;
    c->device = 0; c->max_batch = 32; c->max_audio_seconds = 30; c->max_new_tokens = 448; c->max_prompt_extra = 64;
    c->classify_num = 0; c->tok_timestamp = 151705; c->timestamp_segment_time = 0.08f;
    if (p == "tiny" || p == "tiny-aligner") {   // test geometry (oracle/config.py AUDIO_TINY / TEXT_TINY / TOKENS_TINY)
        c->enc_d_model = 64; c->enc_heads = 2; c->enc_ffn = 128; c->enc_layers = 2; c->enc_out_dim = 64;
        c->conv_channels = 32; c->n_window_infer = 200;
        c->vocab = 512; c->hidden = 64; c->dec_layers = 2; c->heads = 4; c->kv_heads = 2; c->head_dim = 32; c->inter = 128;
        c->tok_im_start = 500; c->tok_im_end = 501; c->tok_audio_start = 502; c->tok_audio_end = 503;
        c->tok_audio_pad = 504; c->tok_asr_text = 505; c->tok_newline = 198; c->tok_system = 300;
        c->tok_user = 301; c->tok_assistant = 302;
        c->bits = 16; c->max_batch = 8;
        if (p == "tiny-aligner") { c->classify_num = 40; c->tok_timestamp = 506; c->max_prompt_extra = 256; c->max_new_tokens = 1; }
        return QASR_OK;
    }
    std::string lower_p = p;
    for (auto& ch : lower_p) ch = (char)tolower(ch);
    if (contains(lower_p, "aligner")) {
        // Qwen3ForcedAligner (ForcedAligner.swift:63-83): encoder = Qwen3AudioEncoderConfig.forcedAligner
        // (AudioEncoder.swift:71-88: the large encoder projecting to 1024), text decoder = .small, 5000 classes
        c->enc_d_model = 1024; c->enc_heads = 16; c->enc_ffn = 4096; c->enc_layers = 24; c->enc_out_dim = 1024;
        c->classify_num = 5000;
        c->bits = contains(lower_p, "bf16") || contains(lower_p, "float") ? 16 : contains(lower_p, "8bit") ? 8 : 4;   // ForcedAlignerVariant.detect :17-26
        c->max_batch = 1; c->max_audio_seconds = 1200; c->max_new_tokens = 1; c->max_prompt_extra = 4096;
        return QASR_OK;
    }
    // ASRModelSize.detect / detectBits (Qwen3ASR.swift:581-601)
    bool large = contains(p, "1.7B") || contains(p, "1.7b");
    std::string lower = p;
    for (auto& ch : lower) ch = (char)tolower(ch);
    int bits = (contains(lower, "8bit") || contains(lower, "8-bit")) ? 8
             : (contains(lower, "4bit") || contains(lower, "4-bit")) ? 4 : (large ? 8 : 4);
    c->bits = bits;
    if (large) {         // .large presets (AudioEncoder.swift:51-68, Configuration.swift:89-100)
        c->enc_d_model = 1024; c->enc_heads = 16; c->enc_ffn = 4096; c->enc_layers = 24; c->enc_out_dim = 2048;
        c->hidden = 2048; c->inter = 6144;
    }
    return QASR_OK;
}

int qasr_create(const char* model_dir, const qasr_config* cfg, qasr_engine** out) {
    if (!cfg || !out) return QASR_ERR_INVALID;
    *out = nullptr;
    return guarded_create(out, model_dir ? QASR_ERR_IO : QASR_ERR_INVALID, [&](qasr_engine* e) {
        e->impl.reset(new Engine(*cfg));
        if (model_dir) { e->impl->load_directory(model_dir); e->impl->finalize(); }
    });
}

int qasr_set_tensor(qasr_engine* e, const char* name, const void* host, int dtype, const int64_t* shape, int ndim) {
    if (!e || !name || !host || !shape || ndim <= 0) return QASR_ERR_INVALID;
    return on_device(e, [&] { e->impl->set_tensor(name, host, dtype, shape, ndim); });
}
int qasr_finalize(qasr_engine* e) { if (!e) return QASR_ERR_INVALID; return on_device(e, [&] { e->impl->finalize(); }); }
int qasr_is_loaded(const qasr_engine* e) { return e && e->impl->loaded(); }
int qasr_unload(qasr_engine* e) { if (!e) return QASR_ERR_INVALID; return on_device(e, [&] { e->impl->unload(); }); }
size_t qasr_memory_footprint(const qasr_engine* e) { return e ? e->impl->memory_footprint() : 0; }
void qasr_destroy(qasr_engine* e) { delete e; }
const char* qasr_last_error(const qasr_engine* e) { return error_slot(e).c_str(); }
int qasr_input_sample_rate(const qasr_engine*) { return 16000; }

int qasr_num_mel_frames(size_t n) { return qasr::mel_num_frames((long)n); }

int qasr_mel(qasr_engine* e, const float* pcm, size_t n, float* out) {
    if (!e || !pcm || !out) return QASR_ERR_INVALID;
    if (n == 0) return fail(e, QASR_ERR_EMPTY_AUDIO, "empty clip");
    return on_device(e, [&] { e->impl->mel_host(pcm, n, out); });
}

int qasr_num_audio_tokens(const qasr_engine* e, int n_frames) { return e ? e->impl->num_audio_tokens(n_frames) : -1; }

int qasr_encode(qasr_engine* e, const float* mel, int n_frames, float* out) {
    if (!e || !mel || !out) return QASR_ERR_INVALID;
    if (!e->impl->loaded()) return fail(e, QASR_ERR_NOT_LOADED, "weights not finalized");
    return on_device(e, [&] { e->impl->encode_host(mel, n_frames, out); });
}

int qasr_set_vocab(qasr_engine* e, const int32_t* ids, const char* const* tokens, size_t n) {
    if (!e || !ids || !tokens) return QASR_ERR_INVALID;
    return on_device(e, [&] { e->impl->set_vocab(ids, tokens, n); });
}

int qasr_set_merges(qasr_engine* e, const char* merges_txt) {
    if (!e || !merges_txt) return QASR_ERR_INVALID;
    return on_device(e, [&] { e->impl->set_merges(merges_txt); });
}

int qasr_encode_text(qasr_engine* e, const char* utf8, int32_t* ids, int32_t cap) {
    if (!e || !utf8 || !ids || cap < 0) return -1;
    try {
        std::vector<int32_t> v = e->impl->encode_text(utf8);
        if ((int32_t)v.size() > cap) { fail(e, QASR_ERR_CAPACITY, "encode_text: buffer too small"); return -1; }
        std::memcpy(ids, v.data(), v.size() * sizeof(int32_t));
        return (int32_t)v.size();
    } catch (const std::exception& ex) { fail(e, QASR_ERR_INVALID, ex.what()); return -1; }
}

int qasr_detokenize(qasr_engine* e, const int32_t* tokens, int32_t n, char* buf, size_t cap) {
    if (!e || !tokens || !buf || cap == 0 || n < 0) return -1;
    int len = -1;
    if (guarded(e, [&] { len = copy_out(e->impl->detokenize(tokens, n, true), buf, cap); })) return -1;
    if (len < 0) fail(e, QASR_ERR_CAPACITY, "detokenize: buffer too small");
    return len;
}

int qasr_batch_begin(qasr_engine* e, const float* const* pcm, const size_t* n, size_t B, const qasr_options* opt) {
    if (!e || !pcm || !n) return QASR_ERR_INVALID;
    if (!e->impl->loaded()) return fail(e, QASR_ERR_NOT_LOADED, "weights not finalized");
    for (size_t b = 0; b < B; ++b) if (n[b] == 0 || !pcm[b]) return fail(e, QASR_ERR_EMPTY_AUDIO, "empty clip in batch");
    return on_device(e, [&] { e->impl->batch_begin(pcm, n, B, opt); });
}
int qasr_batch_stage(qasr_engine* e, const float* const* pcm, const size_t* n, size_t B) {
    if (!e || !pcm || !n) return QASR_ERR_INVALID;
    return on_device(e, [&] { e->impl->batch_stage(pcm, n, B); });
}
int qasr_batch_begin_staged(qasr_engine* e, const qasr_options* opt) {
    if (!e) return QASR_ERR_INVALID;
    return on_device(e, [&] { e->impl->batch_begin_staged(opt); });
}
int qasr_batch_run(qasr_engine* e) { if (!e) return QASR_ERR_INVALID; return on_device(e, [&] { e->impl->batch_run(); }); }
int qasr_batch_rewind(qasr_engine* e) { if (!e) return QASR_ERR_INVALID; return on_device(e, [&] { e->impl->batch_rewind(); }); }
int qasr_batch_sync(qasr_engine* e) { if (!e) return QASR_ERR_INVALID; return on_device(e, [&] { e->impl->batch_sync(); }); }
int qasr_batch_tokens(qasr_engine* e, int32_t* tokens, int32_t* lens) {
    if (!e || !tokens || !lens) return QASR_ERR_INVALID;
    if (!e->impl->loaded()) return fail(e, QASR_ERR_NOT_LOADED, "weights not finalized");
    return on_device(e, [&] { e->impl->batch_tokens(tokens, lens); });
}
int qasr_batch_timings(qasr_engine* e, float ms[5], int32_t* n_steps) {
    if (!e || !ms) return QASR_ERR_INVALID;
    return on_device(e, [&] { e->impl->batch_timings(ms, n_steps); });
}
int qasr_kernel_probe(qasr_engine* e, int which, int reps, float* avg_ms, double* bytes_per_launch) {
    if (!e || !avg_ms || !bytes_per_launch || reps <= 0 || which < 0 || which > 7) return QASR_ERR_INVALID;
    return on_device(e, [&] { e->impl->kernel_probe(which, reps, avg_ms, bytes_per_launch); });
}

int qasr_gemm_probe(qasr_engine* e, const uint16_t* A, const uint16_t* W, const float* bias, int M, int N, int K, int form,
                    int reps, float* out, float* avg_ms) {
    if (!e || !A || !W || !out || M <= 0 || N <= 0 || K <= 0 || K % 8 || N % 4 || form < -1 || form > 2 || reps <= 0)
        return QASR_ERR_INVALID;
    return on_device(e, [&] { e->impl->gemm_probe(A, W, bias, M, N, K, form, reps, out, avg_ms); });
}

int qasr_gemm_case_probe(qasr_engine* e, int which, int form, const qasr_gemm_case* g, const uint16_t* A, const uint16_t* W,
                         const void* bias, const int32_t* aux_i, const int64_t* aux_l, const float* aux_f, void* out) {
    if (!e || !g || !A || !W || !out) return QASR_ERR_INVALID;
    if (const char* why = gemm_case_refusal(which, form, *g, bias, aux_i, aux_l, aux_f)) return fail(e, QASR_ERR_INVALID, why);
    return on_device(e, [&] { e->impl->gemm_case_probe(which, form, *g, A, W, bias, aux_i, aux_l, aux_f, out); });
}

int qasr_attn_case_probe(qasr_engine* e, int op, const qasr_attn_case* g, uint16_t* qkv, const uint16_t* x, const uint16_t* W,
                         const int32_t* cu, const int32_t* slot_of_clip, const int32_t* pos, const int32_t* slot, const uint16_t* qn_w,
                         const uint16_t* kn_w, uint16_t* kcache, uint16_t* vfrag, const uint16_t* vt, uint16_t* qr, uint16_t* out) {
    if (!e || !g || !qkv || !qn_w || !kn_w || !kcache || !vfrag || !out) return QASR_ERR_INVALID;
    if (const char* why = attn_case_refusal(op, *g, x, W, cu, slot_of_clip, pos, slot, vt, qr)) return fail(e, QASR_ERR_INVALID, why);
    return on_device(e, [&] { e->impl->attn_case_probe(op, *g, qkv, x, W, cu, slot_of_clip, pos, slot, qn_w, kn_w, kcache, vfrag, vt, qr, out); });
}

int qasr_syn_attn_case_probe(qasr_engine* e, int op, const qasr_syn_attn_case* g, const void* qkv, const int32_t* slot, const int32_t* pos,
                             const uint16_t* qn_w, const uint16_t* kn_w, const float* cos, const float* sin, uint16_t* kcache, uint16_t* vcache,
                             uint16_t* qr, void* out) {
    if (!e || !g) return QASR_ERR_INVALID;
    if (const char* why = syn_attn_case_refusal(op, *g, qkv, slot, pos, qn_w, kn_w, cos, sin, kcache, vcache, qr, out))
        return fail(e, QASR_ERR_INVALID, why);
    return on_device(e, [&] { e->impl->syn_attn_case_probe(op, *g, qkv, slot, pos, qn_w, kn_w, cos, sin, kcache, vcache, qr, out); });
}

int qasr_codec_case_probe(qasr_engine* e, int op, const qasr_codec_case* g, const float* A, const float* Wt, const float* bias, const float* sa,
                          const float* sb, const float* ls, const float* R, const int32_t* loc_a, int32_t* loc_b, float* out) {
    if (!e || !g) return QASR_ERR_INVALID;
    if (const char* why = codec_case_refusal(op, *g, A, Wt, bias, sa, sb, ls, R, loc_a, loc_b, out)) return fail(e, QASR_ERR_INVALID, why);
    return on_device(e, [&] { e->impl->codec_case_probe(op, *g, A, Wt, bias, sa, sb, ls, R, loc_a, loc_b, out); });
}

int qasr_enc_case_probe(qasr_engine* e, int op, const qasr_enc_case* g, const void* in, const int32_t* idx, const int64_t* off, const float* pf,
                        const uint16_t* pw, void* out) {
    if (!e || !g || !out) return QASR_ERR_INVALID;
    if (const char* why = enc_case_refusal(op, *g, in, idx, off, pf, pw)) return fail(e, QASR_ERR_INVALID, why);
    return on_device(e, [&] { e->impl->enc_case_probe(op, *g, in, idx, off, pf, pw, out); });
}

int qasr_dec_case_probe(qasr_engine* e, int op, qasr_dec_case* g, const uint16_t* X, const void* W, const void* scales, const void* biases,
                        const uint16_t* norm_w, uint16_t* out, float* logits, float* part_val, int32_t* part_idx, int32_t* state,
                        const float* rope, float* rope_rows) {
    if (!e || !g) return QASR_ERR_INVALID;
    if (const char* why = dec_case_refusal(op, *g, X, W, scales, biases, norm_w, out, logits, part_val, part_idx, state, rope, rope_rows))
        return fail(e, QASR_ERR_INVALID, why);
    return on_device(e, [&] { e->impl->dec_case_probe(op, *g, X, W, scales, biases, norm_w, out, logits, part_val, part_idx, state, rope, rope_rows); });
}

int qasr_transcribe_batch(qasr_engine* e, const float* const* pcm, const size_t* n, size_t B, int sample_rate,
                          const qasr_options* opt, int32_t* tokens, int32_t* lens) {
    if (!e || !tokens || !lens) return QASR_ERR_INVALID;
    // AudioPreprocessing.swift:327-329 resamples with AVAudioConverter (closed source); inputs must be 16 kHz here
    if (sample_rate != 16000) return fail(e, QASR_ERR_INVALID, "only 16 kHz input is supported (resampler is out of scope)");
    int rc = qasr_batch_begin(e, pcm, n, B, opt);
    if (rc) return rc;
    if ((rc = qasr_batch_run(e))) return rc;
    return qasr_batch_tokens(e, tokens, lens);
}

int qasr_transcribe(qasr_engine* e, const float* pcm, size_t n, int sample_rate, const qasr_options* opt, qasr_result* out) {
    if (!e || !out) return QASR_ERR_INVALID;
    const int stride = e->impl->config().max_new_tokens + 1;
    std::vector<int32_t> toks((size_t)stride);
    int32_t len = 0;
    const float* ptrs[1] = {pcm};
    size_t ns[1] = {n};
    int rc = qasr_transcribe_batch(e, ptrs, ns, 1, sample_rate, opt, toks.data(), &len);
    if (rc) return rc;
    try {
        e->impl->result_tokens.assign(toks.begin(), toks.begin() + len);
        e->impl->result_text = e->impl->detokenize(toks.data(), len, true);
    } catch (const std::exception& ex) { return fail(e, QASR_ERR_INVALID, ex.what()); }
    out->text = e->impl->result_text.c_str();
    out->tokens = e->impl->result_tokens.data();
    out->n_tokens = len;
    return QASR_OK;
}

// ---- forced aligner ---------------------------------------------------------------------------------
static char* dup_joined(const std::vector<std::string>& v) {
    size_t n = 1;
    for (auto& s : v) n += s.size() + 1;
    char* out = (char*)malloc(n);
    if (!out) return nullptr;
    char* q = out;
    for (size_t i = 0; i < v.size(); ++i) {
        if (i) *q++ = '\n';
        std::memcpy(q, v[i].data(), v[i].size());
        q += v[i].size();
    }
    *q = 0;
    return out;
}

int qasr_split_words(const char* text, const char* language, char** surfaces, char** cleaned) {
    if (!text) return -QASR_ERR_INVALID;
    if (surfaces) *surfaces = nullptr;
    if (cleaned) *cleaned = nullptr;
    try {
        if (qasr::aligner_needs_nl_tokenizer(language ? language : "English")) return -QASR_ERR_UNSUPPORTED;
        auto pairs = qasr::aligner_split_word_pairs(text);
        std::vector<std::string> a, b;
        for (auto& p : pairs) { a.push_back(p.first); b.push_back(p.second); }
        if (surfaces && !(*surfaces = dup_joined(a))) return -QASR_ERR_INVALID;
        if (cleaned && !(*cleaned = dup_joined(b))) return -QASR_ERR_INVALID;
        return (int)pairs.size();
    } catch (const std::exception&) { return -QASR_ERR_INVALID; }
}

int qasr_lis_positions(const int32_t* values, size_t n, int32_t* positions) {
    if ((!values && n) || !positions) return -QASR_ERR_INVALID;
    try {
        auto p = qasr::aligner_lis_positions(values, n);
        std::memcpy(positions, p.data(), p.size() * sizeof(int32_t));
        return (int)p.size();
    } catch (const std::exception&) { return -QASR_ERR_INVALID; }
}

int qasr_enforce_monotonicity(const int32_t* raw, size_t n, int32_t* out) {
    if ((!raw || !out) && n) return QASR_ERR_INVALID;
    try {
        auto v = qasr::aligner_enforce_monotonicity(raw, n);
        std::memcpy(out, v.data(), v.size() * sizeof(int32_t));
        return QASR_OK;
    } catch (const std::exception&) { return QASR_ERR_INVALID; }
}

int qasr_find_trailing_plateau(const float* start_times, size_t n, float tolerance, int32_t min_size) {
    if (!start_times && n) return -QASR_ERR_INVALID;
    return qasr::aligner_find_trailing_plateau(start_times, n, tolerance, min_size);
}

static int split_for(qasr_engine* e, const char* text, const char* language, std::vector<std::pair<std::string, std::string>>& pairs) {
    try {
        if (qasr::aligner_needs_nl_tokenizer(language ? language : "English"))
            return fail(e, QASR_ERR_UNSUPPORTED, "the reference splits this language with Apple's NLTokenizer: pass words to qasr_align_words");
        pairs = qasr::aligner_split_word_pairs(text);
        return QASR_OK;
    } catch (const std::exception& ex) { return fail(e, QASR_ERR_INVALID, ex.what()); }
}

int qasr_align_prepare(qasr_engine* e, const char* text, const char* language, int32_t* ids, int32_t ids_cap,
                       int32_t* ts_positions, int32_t ts_cap, int32_t* n_ts, int32_t* n_words) {
    if (!e || !text || !ids || !ts_positions) return -1;
    try {
        std::vector<std::pair<std::string, std::string>> pairs;
        if (split_for(e, text, language, pairs)) return -1;
        auto st = e->impl->prepare_alignment(pairs);
        if ((int32_t)st.ids.size() > ids_cap || (int32_t)st.ts_pos.size() > ts_cap) { fail(e, QASR_ERR_CAPACITY, "align_prepare: buffer too small"); return -1; }
        std::memcpy(ids, st.ids.data(), st.ids.size() * sizeof(int32_t));
        std::memcpy(ts_positions, st.ts_pos.data(), st.ts_pos.size() * sizeof(int32_t));
        if (n_ts) *n_ts = (int32_t)st.ts_pos.size();
        if (n_words) *n_words = (int32_t)st.words.size();
        return (int)st.ids.size();
    } catch (const std::exception& ex) { fail(e, QASR_ERR_INVALID, ex.what()); return -1; }
}

int qasr_align_raw(qasr_engine* e, const float* pcm, size_t n, const int32_t* slotted_ids, int32_t n_ids,
                   const int32_t* ts_positions, int32_t n_ts, int32_t* raw_indices, float* logits) {
    if (!e || !pcm || !slotted_ids || !ts_positions || !raw_indices || n_ids < 0 || n_ts < 0) return QASR_ERR_INVALID;
    if (n == 0) return fail(e, QASR_ERR_EMPTY_AUDIO, "empty clip");
    if (!e->impl->loaded()) return fail(e, QASR_ERR_NOT_LOADED, "weights not finalized");
    return on_device(e, [&] {
        std::vector<std::vector<int32_t>> raw;
        e->impl->align_forward(&pcm, &n, 1, {std::vector<int32_t>(slotted_ids, slotted_ids + n_ids)},
                               {std::vector<int32_t>(ts_positions, ts_positions + n_ts)}, raw, logits);
        if (!raw.empty()) std::memcpy(raw_indices, raw[0].data(), raw[0].size() * sizeof(int32_t));
    });
}

static int align_common(qasr_engine* e, const float* pcm, size_t n, int sample_rate,
                        const std::vector<std::pair<std::string, std::string>>& pairs, bool long_form, qasr_alignment* out,
                        const char* long_text = nullptr) {
    if (sample_rate != 16000) return fail(e, QASR_ERR_INVALID, "input must be 16 kHz mono (no resampler: AVAudioConverter is not reproducible)");
    if (n == 0) return fail(e, QASR_ERR_EMPTY_AUDIO, "empty clip");
    if (!e->impl->loaded()) return fail(e, QASR_ERR_NOT_LOADED, "weights not finalized");
    return on_device(e, [&] {
        const std::string text = long_text ? long_text : "";
        const int passes = e->impl->align_words(pcm, n, pairs, long_form, long_text ? &text : nullptr);
        out->words = e->impl->al_view.data();
        out->n_words = e->impl->al_view.size();
        out->raw_indices = e->impl->al_raw.data();
        out->n_indices = e->impl->al_raw.size();
        out->passes = passes;
    });
}

int qasr_align(qasr_engine* e, const float* pcm, size_t n, int sample_rate, const char* text, const char* language,
               qasr_alignment* out) {
    if (!e || !pcm || !text || !out) return QASR_ERR_INVALID;
    std::vector<std::pair<std::string, std::string>> pairs;
    if (int rc = split_for(e, text, language, pairs)) return rc;
    return align_common(e, pcm, n, sample_rate, pairs, false, out);
}

int qasr_align_long(qasr_engine* e, const float* pcm, size_t n, int sample_rate, const char* text, const char* language,
                    qasr_alignment* out) {
    if (!e || !pcm || !text || !out) return QASR_ERR_INVALID;
    std::vector<std::pair<std::string, std::string>> pairs;
    if (int rc = split_for(e, text, language, pairs)) return rc;
    return align_common(e, pcm, n, sample_rate, pairs, true, out, text);
}

int qasr_align_batch(qasr_engine* e, const float* const* pcm, const size_t* n, size_t B, int sample_rate,
                     const char* const* texts, const char* language, qasr_alignment* out) {
    if (!e || !pcm || !n || !texts || !out || B == 0) return QASR_ERR_INVALID;
    if (sample_rate != 16000) return fail(e, QASR_ERR_INVALID, "input must be 16 kHz mono (no resampler: AVAudioConverter is not reproducible)");
    if (!e->impl->loaded()) return fail(e, QASR_ERR_NOT_LOADED, "weights not finalized");
    std::vector<std::vector<std::pair<std::string, std::string>>> pairs(B);
    for (size_t b = 0; b < B; ++b) {
        if (!pcm[b] || !texts[b]) return fail(e, QASR_ERR_INVALID, "align_batch: null clip or text");
        if (n[b] == 0) return fail(e, QASR_ERR_EMPTY_AUDIO, "empty clip");
        if (int rc = split_for(e, texts[b], language, pairs[b])) return rc;
    }
    return on_device(e, [&] {
        e->impl->align_batch(pcm, n, B, pairs);
        for (size_t b = 0; b < B; ++b) {
            auto& r = e->impl->al_batch[b];
            out[b].words = r.view.data();
            out[b].n_words = r.view.size();
            out[b].raw_indices = r.raw.data();
            out[b].n_indices = r.raw.size();
            out[b].passes = 1;
        }
    });
}

int qasr_align_words(qasr_engine* e, const float* pcm, size_t n, int sample_rate, const char* const* surfaces,
                     const char* const* cleaned, size_t n_words, qasr_alignment* out) {
    if (!e || !pcm || !surfaces || !cleaned || !out) return QASR_ERR_INVALID;
    std::vector<std::pair<std::string, std::string>> pairs;
    for (size_t i = 0; i < n_words; ++i) {
        if (!surfaces[i] || !cleaned[i]) return fail(e, QASR_ERR_INVALID, "align_words: null word");
        pairs.push_back({surfaces[i], cleaned[i]});
    }
    return align_common(e, pcm, n, sample_rate, pairs, false, out);
}

// speech-core bridge (VoicePipeline.swift:374-410): strings stay valid until the next transcribe
static sc_transcription_result_t vt_transcribe(void* ctx, const float* audio, size_t length, int sample_rate) {
    qasr_engine* e = static_cast<qasr_engine*>(ctx);
    qasr_result r{};
    sc_transcription_result_t out{};
    int rc = qasr_transcribe(e, audio, length, sample_rate, nullptr, &r);
    if (rc != QASR_OK) {
        e->impl->result_text = std::string("[qasr error: ") + e->impl->last_error + "]";
        out.text = e->impl->result_text.c_str();
    } else {
        out.text = r.text;
    }
    out.language = "";
    out.confidence = 0.0f;      // TranscriptionResult default (Protocols.swift:141)
    out.start_time = 0.0f;
    out.end_time = 0.0f;
    return out;
}
static int32_t vt_rate(void*) { return 16000; }

int qasr_stt_vtable(qasr_engine* e, sc_stt_vtable_t* out) {
    if (!e || !out) return QASR_ERR_INVALID;
    std::memset(out, 0, sizeof(*out));
    out->context = e;
    out->transcribe = vt_transcribe;
    out->input_sample_rate = vt_rate;
    return QASR_OK;
}

int qasr_decode_structure(qasr_engine* e, int* fused_qa, int* chain, int* launches_per_layer) {
    if (!e || !fused_qa || !chain || !launches_per_layer) return QASR_ERR_INVALID;
    return on_device(e, [&] { e->impl->decode_structure(fused_qa, chain, launches_per_layer); });
}

int qasr_set_shared_device(qasr_engine* e, int shared) {
    if (!e) return QASR_ERR_INVALID;
    return on_device(e, [&] { e->impl->set_shared_device(shared != 0); });
}

int qasr_set_tuning(const char* key, int value) {
    if (!key) return QASR_ERR_INVALID;
    return qasr::tuning_set(key, value) ? QASR_OK : QASR_ERR_INVALID;
}
int qasr_get_tuning(const char* key, int* value) {
    if (!key || !value) return QASR_ERR_INVALID;
    return qasr::tuning_get(key, value) ? QASR_OK : QASR_ERR_INVALID;
}

int qasr_prefill_logits(qasr_engine* e, const float* audio_embeds, int n_audio, const qasr_options* opt, float* logits) {
    if (!e || !logits || (n_audio > 0 && !audio_embeds)) return QASR_ERR_INVALID;
    if (!e->impl->loaded()) return fail(e, QASR_ERR_NOT_LOADED, "weights not finalized");
    return on_device(e, [&] { e->impl->prefill_logits_host(audio_embeds, n_audio, opt, logits); });
}

int qasr_decode_forced(qasr_engine* e, const int32_t* tokens, int n, float* logits) {
    if (!e || !tokens || !logits || n < 0) return QASR_ERR_INVALID;
    return on_device(e, [&] { e->impl->decode_forced_host(tokens, n, logits); });
}

int qasr_batch_prefill_logits(qasr_engine* e, float* logits) {
    if (!e || !logits) return QASR_ERR_INVALID;
    return on_device(e, [&] { e->impl->batch_prefill_logits(logits); });
}

int qasr_batch_decode_forced(qasr_engine* e, const int32_t* tokens, float* logits) {
    if (!e || !tokens || !logits) return QASR_ERR_INVALID;
    return on_device(e, [&] { e->impl->batch_decode_forced(tokens, logits); });
}

// ---- Omnilingual ASR (wav2vec2 + CTC) -------------------------------------------------------------------
}  // extern "C"

struct qasr_ctc_engine {
    std::unique_ptr<qasr::CtcEngine> impl;
};
static std::string& error_slot(const qasr_ctc_engine* e) { return e && e->impl ? e->impl->last_error : create_error<qasr_engine>(); }

extern "C" {

int qasr_ctc_default_config(const char* variant, qasr_ctc_config* c) {
    if (!c) return QASR_ERR_INVALID;
    const std::string v = variant ? variant : "300M";
    std::memset(c, 0, sizeof(*c));
    c->feature_dim = 512; c->pos_kernel = 128; c->pos_groups = 16; c->vocab = 10288; c->group_size = 64; c->bits = 4;
    c->ln_eps = 1e-5f; c->device = 0; c->max_batch = 32; c->max_audio_seconds = 40;
    if (v == "tiny") {               // oracle/omnilingual.py OMNI_TINY
        c->model_dim = 64; c->layers = 2; c->heads = 2; c->ffn_dim = 128; c->feature_dim = 32; c->pos_kernel = 16; c->pos_groups = 4;
        c->vocab = 40; c->bits = 16; c->max_batch = 8; c->max_audio_seconds = 10;
        return QASR_OK;
    }
    // OmnilingualMLXConfig.variant (:88-103); detectVariant looks for "CTC-<size>-" in a model id (OmnilingualMLXModel.swift:121-126)
    struct V { const char* name; int d, l, h, f; };
    static const V table[] = {{"300M", 1024, 24, 16, 4096}, {"1B", 1280, 48, 20, 5120}, {"3B", 2048, 60, 32, 8192}, {"7B", 2048, 128, 32, 8192}};
    const V* pick = nullptr;
    for (const V& t : table)
        if (v == t.name || contains(v, (std::string("CTC-") + t.name + "-").c_str())) pick = &t;
    if (!pick) return QASR_ERR_INVALID;
    c->model_dim = pick->d; c->layers = pick->l; c->heads = pick->h; c->ffn_dim = pick->f;
    if (contains(v, "8bit")) c->bits = 8;      // detectBits (:128-132)
    return QASR_OK;
}

int qasr_ctc_create(const char* model_dir, const qasr_ctc_config* cfg, qasr_ctc_engine** out) {
    if (!cfg || !out) return QASR_ERR_INVALID;
    *out = nullptr;
    if (cfg->max_audio_seconds > 40 || cfg->max_audio_seconds <= 0 || cfg->max_batch <= 0)
        return fail<qasr_ctc_engine>(nullptr, QASR_ERR_INVALID, "omnilingual: max_audio_seconds must be in 1..40 (the reference's cap), max_batch positive");
    return guarded_create(out, model_dir ? QASR_ERR_IO : QASR_ERR_INVALID, [&](qasr_ctc_engine* e) {
        e->impl.reset(new qasr::CtcEngine(*cfg));
        if (model_dir) { e->impl->load_directory(model_dir); e->impl->finalize(); }
    });
}
int qasr_ctc_set_tensor(qasr_ctc_engine* e, const char* name, const void* host, int dtype, const int64_t* shape, int ndim) {
    if (!e || !name || !host || !shape || ndim <= 0) return QASR_ERR_INVALID;
    return guarded(e, [&] { e->impl->set_tensor(name, host, dtype, shape, ndim); });
}
int qasr_ctc_finalize(qasr_ctc_engine* e) { if (!e) return QASR_ERR_INVALID; return guarded(e, [&] { e->impl->finalize(); }); }
int qasr_ctc_set_pieces(qasr_ctc_engine* e, const char* const* texts, const int32_t* types, size_t n) {
    if (!e || (!texts && n)) return QASR_ERR_INVALID;
    return guarded(e, [&] { e->impl->set_pieces(texts, types, n); });
}
int qasr_ctc_is_loaded(const qasr_ctc_engine* e) { return e && e->impl->loaded(); }
int qasr_ctc_unload(qasr_ctc_engine* e) { if (!e) return QASR_ERR_INVALID; return guarded(e, [&] { e->impl->unload(); }); }
size_t qasr_ctc_memory_footprint(const qasr_ctc_engine* e) { return e ? e->impl->memory_footprint() : 0; }
void qasr_ctc_destroy(qasr_ctc_engine* e) { delete e; }
const char* qasr_ctc_last_error(const qasr_ctc_engine* e) { return error_slot(e).c_str(); }
int qasr_ctc_num_frames(size_t n) { return qasr::CtcEngine::num_frames((long)n); }

static int ctc_run(qasr_ctc_engine* e, const float* const* pcm, const size_t* n, size_t B, int sample_rate,
                   std::vector<std::vector<int32_t>>& collapsed, float* logits) {
    if (sample_rate != 16000) return fail(e, QASR_ERR_INVALID, "only 16 kHz input is supported (resampler is out of scope)");
    if (!e->impl->loaded()) return fail(e, QASR_ERR_NOT_LOADED, "weights not finalized");
    for (size_t b = 0; b < B; ++b) {
        if (!pcm[b] || n[b] == 0) return fail(e, QASR_ERR_EMPTY_AUDIO, "empty clip in batch");
        // OmnilingualMLXModel.swift:154-159: the 40 s cap is an error, not a truncation
        if ((double)n[b] / 16000.0 > 40.0) return fail(e, QASR_ERR_CAPACITY, "input exceeds the Omnilingual cap of 40 s");
    }
    return guarded(e, [&] {
        std::vector<std::vector<int32_t>> frames;
        e->impl->forward(pcm, n, B, frames, logits);
        collapsed.assign(B, {});
        for (size_t b = 0; b < B; ++b) {                    // collapseConsecutiveDuplicates (:195-209)
            int prev = -1;
            for (int32_t id : frames[b]) if (id != prev) { collapsed[b].push_back(id); prev = id; }
        }
    });
}

int qasr_ctc_transcribe_batch(qasr_ctc_engine* e, const float* const* pcm, const size_t* n, size_t B, int sample_rate,
                              int32_t* ids, size_t stride, int32_t* lens) {
    if (!e || !pcm || !n || !ids || !lens || B == 0) return QASR_ERR_INVALID;
    std::vector<std::vector<int32_t>> col;
    if (int rc = ctc_run(e, pcm, n, B, sample_rate, col, nullptr)) return rc;
    for (size_t b = 0; b < B; ++b) {
        if (col[b].size() > stride) return fail(e, QASR_ERR_CAPACITY, "ctc_transcribe_batch: id buffer stride too small");
        std::memcpy(ids + b * stride, col[b].data(), col[b].size() * sizeof(int32_t));
        lens[b] = (int32_t)col[b].size();
    }
    return QASR_OK;
}

int qasr_ctc_transcribe(qasr_ctc_engine* e, const float* pcm, size_t n, int sample_rate, const char** text) {
    if (!e || !text) return QASR_ERR_INVALID;
    if (n == 0) { e->impl->result_text.clear(); *text = e->impl->result_text.c_str(); return QASR_OK; }     // :160-162
    if (!pcm) return QASR_ERR_INVALID;
    std::vector<std::vector<int32_t>> col;
    if (int rc = ctc_run(e, &pcm, &n, 1, sample_rate, col, nullptr)) return rc;
    // no SentencePiece vocabulary: an error, not "" for every clip (the reference cannot exist without one, OmnilingualMLXModel.swift:86-98)
    if (!e->impl->has_pieces()) return fail(e, QASR_ERR_NOT_LOADED, "no SentencePiece vocabulary: load tokenizer.model or call qasr_ctc_set_pieces");
    try { e->impl->result_text = e->impl->detokenize(col[0].data(), (int)col[0].size()); }
    catch (const std::exception& ex) { return fail(e, QASR_ERR_INVALID, ex.what()); }
    *text = e->impl->result_text.c_str();
    return QASR_OK;
}

int qasr_ctc_logits(qasr_ctc_engine* e, const float* pcm, size_t n, float* logits) {
    if (!e || !pcm || !logits) return QASR_ERR_INVALID;
    std::vector<std::vector<int32_t>> col;
    return ctc_run(e, &pcm, &n, 1, 16000, col, logits);
}

int qasr_ctc_detokenize(qasr_ctc_engine* e, const int32_t* ids, int32_t n, char* buf, size_t cap) {
    if (!e || (!ids && n) || !buf || cap == 0 || n < 0) return -1;
    if (!e->impl->has_pieces()) { fail(e, QASR_ERR_NOT_LOADED, "no SentencePiece vocabulary"); return -1; }
    int len = -1;
    if (guarded(e, [&] { len = copy_out(e->impl->detokenize(ids, n), buf, cap); })) return -1;
    if (len < 0) fail(e, QASR_ERR_CAPACITY, "detokenize: buffer too small");
    return len;
}

int qasr_ctc_timings(qasr_ctc_engine* e, float ms[4]) {
    if (!e || !ms) return QASR_ERR_INVALID;
    return guarded(e, [&] { e->impl->timings(ms); });
}

int qasr_ctc_greedy(const float* logits, int32_t T, int32_t V, int32_t valid_frames, int32_t* out) {
    if (T < 0 || V <= 0 || (T > 0 && (!logits || !out))) return -QASR_ERR_INVALID;
    return qasr::ctc_greedy_decode(logits, T, V, valid_frames, out);
}

int qasr_layer_normalize(const float* x, size_t n, float eps, float* out) {
    if ((!x || !out) && n) return QASR_ERR_INVALID;
    qasr::layer_normalize_host(x, n, eps, out);
    return QASR_OK;
}

}  // extern "C"
