// dec_cases.hip -- qasr_dec_case_probe: the decode-step linears (bf16 and MLX-quantised), the LM heads, rmsnorm_rows, the greedy tail and the
// embedding lookups by themselves, on host
// data.  Only plumbing lives here: uploads, the product's weight repack (pack_mfma_a_launch / quant_pack_launch), ONE call of the product's
// launch entry (dec_kernels.h, dec_quant.h, dec_gemv_wide.h) the way Engine::decode_gemv / run_lm_head call it, downloads.  The arguments were
// checked by the C ABI (api.cpp, dec_case_refusal): every index a launch forms from them stays inside the buffers allocated below.  X carries
// in_extra rows beyond B, out / logits out_extra rows; out, logits and the partials are uploaded first, so bytes no kernel wrote come back as
// given.
#include "engine.h"
#include "dec_gemv_wide.h"

namespace qasr {

// FINALIZE / EMBED: the greedy tail and the embedding lookups; state layout in include/qasr.h
void Engine::dec_case_tail(int op, qasr_dec_case& g, const uint16_t* X, const void* W, const void* scales, const void* biases, uint16_t* out,
                           const float* part_val, const int32_t* part_idx, int32_t* state, const float* rope, float* rope_rows) {
    hipStream_t s = stream_;
    const size_t B = (size_t)g.B, R = B + g.out_extra, V = (size_t)g.N, H = (size_t)g.K;
    DevBuf dW, dS, dBi, dOut, dX, dPv, dPi, dSt, dRope, dRows;
    auto up = [&](DevBuf& d, const void* h, size_t n) {
        d.alloc(n);
        if (n && h) QASR_HIP(hipMemcpyAsync(d.p, h, n, hipMemcpyHostToDevice, s));
    };
    QuantRaw q{};
    if (g.bits) {
        const size_t G = H / 64, esz = g.sb_f32 ? 4 : 2;
        up(dW, W, V * H * g.bits / 8); up(dS, scales, V * G * esz); up(dBi, biases, V * G * esz);
        q = QuantRaw{dW.as<uint32_t>(), dS.p, dBi.p, g.sb_f32, g.N, g.K, g.bits};
    } else up(dW, W, V * H * sizeof(bf16_t));
    const size_t out_bytes = R * H * sizeof(bf16_t);
    up(dOut, out, out_bytes);
    g.route = -1;
    if (op == QASR_DEC_EMBED) {
        const size_t st_bytes = (g.epi == 0 ? 2 : g.epi == 1 ? 1 : 0) * B * sizeof(int32_t);
        up(dSt, state, st_bytes);
        up(dX, X, g.epi == 0 ? (size_t)g.n_audio * H * sizeof(bf16_t) : 0);
        const int* ids = dSt.as<int>();
        if (g.epi == 0) {
            if (g.bits) embed_splice_q_launch(ids, ids + B, q, dX.as<bf16_t>(), dOut.as<bf16_t>(), g.B, g.K, s);
            else embed_splice_launch(ids, ids + B, dW.as<bf16_t>(), dX.as<bf16_t>(), dOut.as<bf16_t>(), g.B, g.K, s);
        } else if (g.epi == 1) {
            if (g.bits) gather_rows_q_launch(q, ids, dOut.as<bf16_t>(), g.B, s);
            else gather_rows_launch(dW.as<bf16_t>(), ids, dOut.as<bf16_t>(), g.B, g.K, s);
        } else quant_dequant_rows_launch(q, g.r0, g.B, dOut.as<bf16_t>(), s);
    } else {
        const size_t stride = (size_t)g.max_new + 1, clear_n = g.clear_words ? (size_t)g.clear_words + 33 : 0;
        const size_t st_n = R * stride + 3 * R + 2 + clear_n, half = (size_t)g.half;
        up(dSt, state, st_n * sizeof(int32_t));
        up(dPv, part_val, B * g.n_parts * sizeof(float)); up(dPi, part_idx, B * g.n_parts * sizeof(int32_t));
        up(dRope, rope, 2 * (size_t)g.n_rope * half * sizeof(float)); up(dRows, rope_rows, 2 * R * half * sizeof(float));
        int* st = dSt.as<int>();
        GreedyState gs{};
        gs.tokens = st; gs.lens = st + R * stride; gs.finished = gs.lens + R; gs.ctx_len = gs.finished + R; gs.n_active = gs.ctx_len + R;
        gs.err = gs.n_active + 1;
        gs.max_new = g.max_new; gs.max_tokens = g.max_tokens; gs.eos = g.eos; gs.ignore_eos = g.ignore_eos; gs.vocab = g.N;
        gs.clear = clear_n ? reinterpret_cast<unsigned*>(gs.err + 1) : nullptr; gs.clear_words = g.clear_words;
        RopeRows rr{dRope.as<float>(), dRope.as<float>() + (size_t)g.n_rope * half, dRows.as<float>(), dRows.as<float>() + R * half, g.half};
        greedy_finalize_launch(dPv.as<float>(), dPi.as<int>(), g.n_parts, gs, g.B, g.advance_ctx, g.bits ? nullptr : dW.as<bf16_t>(),
                               dOut.as<bf16_t>(), g.K, rr, s, g.bits ? &q : nullptr);
        QASR_HIP(hipGetLastError());
        QASR_HIP(hipMemcpyAsync(state, dSt.p, st_n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        QASR_HIP(hipMemcpyAsync(rope_rows, dRows.p, 2 * R * half * sizeof(float), hipMemcpyDeviceToHost, s));
    }
    QASR_HIP(hipGetLastError());
    QASR_HIP(hipMemcpyAsync(out, dOut.p, out_bytes, hipMemcpyDeviceToHost, s));
    QASR_HIP(hipStreamSynchronize(s));
}

void Engine::dec_case_probe(int op, qasr_dec_case& g, const uint16_t* X, const void* W, const void* scales, const void* biases,
                            const uint16_t* norm_w, uint16_t* out, float* logits, float* part_val, int32_t* part_idx, int32_t* state,
                            const float* rope, float* rope_rows) {
    if (op == QASR_DEC_FINALIZE || op == QASR_DEC_EMBED) return dec_case_tail(op, g, X, W, scales, biases, out, part_val, part_idx, state, rope, rope_rows);
    hipStream_t s = stream_;
    const size_t B = (size_t)g.B, N = (size_t)g.N, K = (size_t)g.K;
    const bool quant = op == QASR_DEC_GEMVQ || op == QASR_DEC_LMHEADQ;
    const bool head = op == QASR_DEC_LMHEAD || op == QASR_DEC_LMHEADQ;
    const bool wants_logits = head || (op == QASR_DEC_GEMV && g.epi == DEC_EPI_LOGITS);
    DevBuf dX, dW, dWp, dS, dBi, dSb, dNw, dOut, dLg, dPv, dPi, dScratch;
    auto up = [&](DevBuf& d, const void* h, size_t n) {
        d.alloc(n);
        if (n && h) QASR_HIP(hipMemcpyAsync(d.p, h, n, hipMemcpyHostToDevice, s));
    };
    const size_t out_cols = op == QASR_DEC_RMSNORM_ROWS ? K : g.epi == DEC_EPI_SWIGLU ? N / 2 : N;      // RMSNORM_ROWS: epi is 0 (refusal)
    const size_t out_bytes = out && !wants_logits ? (B + g.out_extra) * out_cols * sizeof(bf16_t) : 0;
    const size_t lg_bytes = wants_logits && logits ? (B + g.out_extra) * N * sizeof(float) : 0;
    const size_t part_bytes = wants_logits ? (size_t)g.part_cap * 4 : 0;
    up(dX, X, (B + g.in_extra) * K * sizeof(bf16_t));
    up(dNw, norm_w, norm_w ? K * sizeof(bf16_t) : 0);
    up(dOut, out, out_bytes); up(dLg, logits, lg_bytes); up(dPv, part_val, part_bytes); up(dPi, part_idx, part_bytes);
    dScratch.alloc(B * K * sizeof(bf16_t));                       // norm_scratch of the generic fallbacks
    const bf16_t* nw = norm_w ? dNw.as<bf16_t>() : nullptr;
    QuantImg qi;
    if (op != QASR_DEC_RMSNORM_ROWS) {
        if (quant) {
            const size_t G = K / 64, esz = g.sb_f32 ? 4 : 2;
            up(dW, W, N * K * g.bits / 8); up(dS, scales, N * G * esz); up(dBi, biases, N * G * esz);
            qi.raw = QuantRaw{dW.as<uint32_t>(), dS.p, dBi.p, g.sb_f32, g.N, g.K, g.bits};
            qi.sb_f32 = g.sb_f32; qi.bits = g.bits;
            if (!g.generic) {
                dWp.alloc(quant_q_bytes(g.N, g.K, g.bits)); dSb.alloc(quant_sb_bytes(g.N, g.K, g.sb_f32));
                quant_pack_launch(qi.raw, dWp.as<uint32_t>(), dSb.p, s);
                qi.qp = dWp.as<uint32_t>(); qi.sb = dSb.p;
            }
        } else {
            up(dW, W, N * K * sizeof(bf16_t));
            if (!g.generic) {
                dWp.alloc(N * K * sizeof(bf16_t));
                pack_mfma_a_launch(dW.as<bf16_t>(), dWp.as<bf16_t>(), g.N, g.K, s);
            }
        }
    }
    DecGemvArgs a{};
    a.W = dW.as<bf16_t>(); a.Wp = !quant && !g.generic ? dWp.as<bf16_t>() : nullptr; a.X = dX.as<bf16_t>();
    a.B = g.B; a.N = g.N; a.K = g.K; a.out = dOut.as<bf16_t>();
    a.logits = lg_bytes ? dLg.as<float>() : nullptr; a.part_val = dPv.as<float>(); a.part_idx = dPi.as<int>();
    const DecEpi epi = (DecEpi)g.epi;
    decode_gemv_note_route(-1);
    g.n_parts = 0;
    switch (op) {
    case QASR_DEC_GEMV:            // Engine::decode_gemv of a float checkpoint
        g.n_parts = decode_gemv_dense_launch(epi, a, nw, g.eps, dScratch.as<bf16_t>(), s); break;
    case QASR_DEC_GEMVQ: decode_gemv_q_launch(epi, a, qi, nw, g.eps, dScratch.as<bf16_t>(), s); break;
    case QASR_DEC_LMHEAD:
        g.n_parts = lm_head_launch(a.W, a.Wp, a.X, nw, g.eps, g.B, g.N, g.K, a.logits, a.part_val, a.part_idx, dScratch.as<bf16_t>(), s);
        break;
    case QASR_DEC_LMHEADQ:
        g.n_parts = lm_head_q_launch(qi, a.X, nw, g.eps, g.B, g.N, g.K, a.logits, a.part_val, a.part_idx, dScratch.as<bf16_t>(), s);
        break;
    case QASR_DEC_RMSNORM_ROWS: rmsnorm_rows_launch(a.X, nw, a.out, g.B, g.K, g.eps, s); break;
    }
    if (!wants_logits) g.n_parts = 0;
    g.route = decode_gemv_last_route();
    QASR_HIP(hipGetLastError());
    if (out_bytes) QASR_HIP(hipMemcpyAsync(out, dOut.p, out_bytes, hipMemcpyDeviceToHost, s));
    if (lg_bytes) QASR_HIP(hipMemcpyAsync(logits, dLg.p, lg_bytes, hipMemcpyDeviceToHost, s));
    if (part_bytes) {
        QASR_HIP(hipMemcpyAsync(part_val, dPv.p, part_bytes, hipMemcpyDeviceToHost, s));
        QASR_HIP(hipMemcpyAsync(part_idx, dPi.p, part_bytes, hipMemcpyDeviceToHost, s));
    }
    QASR_HIP(hipStreamSynchronize(s));
}

}  // namespace qasr
