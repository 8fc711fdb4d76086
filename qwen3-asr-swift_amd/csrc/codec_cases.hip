// codec_cases.hip -- qasr_codec_case_probe: the f32 kernels of the waveform codecs by themselves, on host data: the tile behind each row
// locator, RMSNorm, the depthwise conv + LayerNorm, the decoder's code gather, attention and output conv, the encoder's input conv,
// attention and quantiser, the AudioVAE's depthwise conv and fused unit.  Only plumbing lives here: uploads, ONE call of a launch entry of
// codec_launch.h (the one the three codec classes call), downloads.  The arguments were checked by the C ABI (api.cpp,
// codec_case_refusal): every index a launch forms from them stays inside the buffers allocated below, whose sizes are the ones
// include/qasr.h states for the caller's arrays.
#include "engine.h"
#include "codec_launch.h"

namespace qasr {

void Engine::codec_case_probe(int op, const qasr_codec_case& g, const float* A, const float* Wt, const float* bias, const float* sa, const float* sb,
                              const float* ls, const float* R, const int32_t* loc_a, int32_t* loc_b, float* out) {
    hipStream_t s = stream_;
    const bool tile = op == QASR_CODEC_TILE;
    const bool attn = op == QASR_CODEC_ATTN_DEC || op == QASR_CODEC_ATTN_ENC;
    const size_t F = sizeof(float), in_w = tile ? g.Cin : op == QASR_CODEC_CENC_IN ? 1 : attn ? (size_t)3 * g.heads * 64 : g.C;
    const size_t out_w = tile ? g.ldc : op == QASR_CODEC_GATHER || op == QASR_CODEC_VQ ? 2 * g.C : op == QASR_CODEC_OUT ? 1
                         : attn ? (size_t)g.heads * 64 : g.C;
    const size_t a_bytes = (size_t)g.a_rows * in_w * F, out_bytes = ((size_t)g.M + g.out_extra) * out_w * F;
    const bool repeats = g.rows_kind == QASR_CODEC_ROWS_WINDOW || g.rows_kind == QASR_CODEC_ROWS_TAIL;
    const size_t n_w = tile ? (size_t)g.K * g.N : op == QASR_CODEC_RMS ? (size_t)g.C
                     : op == QASR_CODEC_GATHER ? ((size_t)g.S0 + (size_t)(g.Q - 1) * g.S1) * g.C
                     : op == QASR_CODEC_VQ ? (size_t)g.S0 * g.C : attn ? (size_t)g.n_table * 64
                     : op == QASR_CODEC_VAE_UNIT ? (size_t)g.C * g.C + (size_t)13 * g.C : (size_t)7 * g.C;
    const size_t n_bias = tile ? (size_t)(repeats ? g.bmod : g.N) : op == QASR_CODEC_OUT ? 1 : (size_t)g.C;
    const size_t n_s = tile ? (size_t)(g.epi == E_RESMAP ? g.N : g.Cin) : (size_t)g.C;
    DevBuf dA, dW, dBias, dSa, dSb, dLs, dR, dLa, dLb, dOut;
    auto up = [&](DevBuf& d, const void* h, size_t n) -> const float* {
        if (!h) return nullptr;
        d.alloc(n);
        QASR_HIP(hipMemcpyAsync(d.p, h, n, hipMemcpyHostToDevice, s));
        return d.as<float>();
    };
    const float *pA = up(dA, A, a_bytes), *pW = up(dW, Wt, n_w * F);
    up(dOut, out, out_bytes);
    CodecRowsArg rows;
    rows.kind = g.rows_kind;
    rows.a = reinterpret_cast<const int*>(up(dLa, loc_a, (size_t)g.n_loc * sizeof(int)));
    rows.b = reinterpret_cast<const int*>(up(dLb, loc_b, (size_t)g.n_loc * sizeof(int)));
    rows.rate = g.rate; rows.lead = g.lead; rows.n_clips = g.n_clips; rows.stride = g.stride;
    if (op == QASR_CODEC_VQ) {                         // Wt | bias | sa = codebook 0, its transpose, its norms; sb | ls | R = those of codebooks 1 .. Q - 1
        const size_t n0 = (size_t)g.S0 * g.C, n1 = (size_t)(g.Q - 1) * g.S1 * g.C;
        const float *cb0 = pW, *cbt0 = up(dBias, bias, n0 * F), *csq0 = up(dSa, sa, (size_t)g.S0 * F);
        const float *cb1 = up(dSb, sb, n1 * F), *cbt1 = up(dLs, ls, n1 * F), *csq1 = up(dR, R, (size_t)(g.Q - 1) * g.S1 * F);
        cenc_vq_launch(dOut.as<float>(), g.M, 2 * g.C, g.C, g.Q, cb0, cbt0, csq0, g.S0, cb1, cbt1, csq1, g.S1, const_cast<int*>(rows.b), s);
        QASR_HIP(hipGetLastError());
        QASR_HIP(hipMemcpyAsync(loc_b, dLb.p, (size_t)g.n_loc * sizeof(int), hipMemcpyDeviceToHost, s));
        QASR_HIP(hipMemcpyAsync(out, dOut.p, out_bytes, hipMemcpyDeviceToHost, s));
        QASR_HIP(hipStreamSynchronize(s));
        return;
    }
    if (op == QASR_CODEC_ATTN_DEC) {
        codec_attn_launch(pA, rows.a, g.n_clips, pW, g.heads, dOut.as<float>(), s);
    } else if (op == QASR_CODEC_ATTN_ENC) {
        cenc_attn_launch(pA, rows.a, g.n_clips, pW, g.heads, dOut.as<float>(), s);
    } else if (op == QASR_CODEC_VAE_UNIT) {            // Wt = w1 [7][C] | b1 | a1 | 1 / a1 | a2 | 1 / a2 | conv2's Wt [C][C] | b2; sa | sb | ls = the map
        const size_t C = (size_t)g.C;
        const float *ma = up(dSa, sa, C * F), *mi = up(dSb, sb, C * F), *aff = up(dLs, ls, 2 * C * F);
        vae_unit_launch(pA, g.M, g.C, g.dil, rows.a, g.rate, pW, pW + 7 * C, pW + 8 * C, pW + 9 * C, pW + 10 * C, pW + 11 * C, pW + 12 * C,
                        pW + 12 * C + C * C, ma, mi, aff, dOut.as<float>(), s);
    } else if (op == QASR_CODEC_VAE_DW) {              // sa | sb = a1, 1 / a1; ls | R = a2, 1 / a2
        const size_t c = (size_t)g.C * F;
        const float *pB = up(dBias, bias, c), *a1 = up(dSa, sa, c), *i1 = up(dSb, sb, c), *a2 = up(dLs, ls, c), *i2 = up(dR, R, c);
        vae_dw_launch(g.snake != 0, pA, g.M, g.C, g.dil, rows.a, g.rate, pW, pB, a1, i1, a2, i2, dOut.as<float>(), s);
    } else if (op == QASR_CODEC_RMS) {
        codec_rms_launch(pA, g.M, g.C, pW, g.eps, dOut.as<float>(), s);
    } else if (op == QASR_CODEC_GATHER) {
        codec_gather_launch(rows.a, g.M, g.Q, g.C, g.S0, g.S1, pW, dOut.as<float>(), s);
    } else if (op == QASR_CODEC_OUT) {
        const float *pB = up(dBias, bias, n_bias * F), *pSa = up(dSa, sa, n_s * F), *pSb = up(dSb, sb, n_s * F);
        codec_out_launch(g.rows_kind == QASR_CODEC_ROWS_TAIL, pA, g.M, g.C, g.rate, rows.a, rows.b, pSa, pSb, pW, pB, g.clip, dOut.as<float>(), s);
    } else if (op == QASR_CODEC_CENC_IN) {
        const float* pB = up(dBias, bias, n_bias * F);
        cenc_in_launch(pA, g.M, g.C, rows.a, g.n_clips, pW, pB, dOut.as<float>(), s);
    } else if (op == QASR_CODEC_DWLN) {
        const float *pB = up(dBias, bias, n_bias * F), *pLw = up(dSa, sa, n_s * F), *pLb = up(dSb, sb, n_s * F);
        codec_dwln_launch(rows, pA, g.M, g.C, pW, pB, pLw, pLb, dOut.as<float>(), s);
    } else {
        const float *pB = up(dBias, bias, n_bias * F), *pSa = up(dSa, sa, n_s * F), *pSb = up(dSb, sb, n_s * F), *pLs = up(dLs, ls, (size_t)(g.epi == E_RESMAP ? 2 * g.N : g.N) * F);
        const float* pR = g.in_place ? dOut.as<float>() : up(dR, R, out_bytes);
        codec_tile_launch(rows, g.snake != 0, g.epi, pA, g.M, g.Cin, g.taps, g.dil, pW, g.K, g.N, pB, g.bmod, pSa, pSb, pLs, pR, dOut.as<float>(),
                          g.ldc, s);
    }
    QASR_HIP(hipGetLastError());
    QASR_HIP(hipMemcpyAsync(out, dOut.p, out_bytes, hipMemcpyDeviceToHost, s));
    QASR_HIP(hipStreamSynchronize(s));
}

}  // namespace qasr
