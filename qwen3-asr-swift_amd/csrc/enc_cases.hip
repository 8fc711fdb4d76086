// enc_cases.hip -- qasr_enc_case_probe: the encoder-side kernels that are not the GEMM by themselves, on host data.  Only plumbing lives
// here: uploads, ONE call of the product's launch entry (enc_kernels.h, ctc_kernels.h), downloads.  The arguments were checked by the C ABI
// (api.cpp, enc_case_refusal): every index a launch forms from them stays inside the buffers allocated below.  `in` and `out` carry
// in_extra / out_extra rows beyond what the launch is told about; `out` is uploaded first, so bytes no kernel wrote come back as given.
#include "engine.h"
#include "enc_kernels.h"
#include "ctc_kernels.h"

namespace qasr {

static_assert(sizeof(ChunkMeta) == 9 * sizeof(int32_t), "ChunkMeta is passed as 9 int32 per image");

// bytes of one row of `in` / `out` and the elements of idx / off / pf / pw, per operation
struct EncCaseSizes { size_t in_row, in_bytes, out_row, out_tail, out_bytes, idx, off, pf, pw; };

static EncCaseSizes enc_case_sizes(int op, const qasr_enc_case& g) {
    EncCaseSizes z{};
    const size_t D = (size_t)g.D, B = (size_t)g.n_clips, rows = (size_t)g.rows;
    switch (op) {
    case QASR_ENC_MHA: case QASR_ENC_WINDOW:
        z.in_row = 3 * (size_t)g.heads * g.hd * sizeof(bf16_t); z.out_row = (size_t)g.heads * g.hd * sizeof(bf16_t); z.idx = B + 1; break;
    case QASR_ENC_LN_BF16: case QASR_ENC_LN_GELU_BF16: z.in_row = D * 4; z.out_row = D * 2; z.pf = 2 * D; break;
    case QASR_ENC_LN_GELU_F32: z.in_row = D * 4; z.out_row = D * 4; z.pf = 2 * D; break;
    case QASR_ENC_CONV0: z.in_bytes = (size_t)g.n_in * 4; z.off = B; z.idx = 2 * B; z.pf = 2 * B + 13 * D; z.out_row = D * 2; break;
    case QASR_ENC_WAVE_STATS: z.in_bytes = (size_t)g.n_in * 4; z.off = rows; z.idx = rows; z.out_row = 8; break;
    case QASR_ENC_CONV1:
        z.in_bytes = (size_t)g.n_in * 4; z.idx = 9 * rows; z.pf = D; z.pw = 9 * D; z.out_row = (size_t)g.H1 * g.W1 * D * 2; break;
    case QASR_ENC_ARGMAX: z.in_row = (size_t)g.ld * 4; z.out_row = 4; z.out_tail = 4; break;
    case QASR_ENC_CAST: z.in_row = 4; z.out_row = 2; break;
    case QASR_ENC_CONV_ROWS: z.idx = 3 * B; z.out_row = 8; break;
    case QASR_ENC_FRAME_INFO: z.idx = 2 * B; z.out_row = 8; break;
    }
    if (z.in_row) z.in_bytes = z.in_row * (rows + (size_t)g.in_extra);
    z.out_bytes = z.out_row * (rows + (size_t)g.out_extra) + z.out_tail;
    return z;
}

void Engine::enc_case_probe(int op, const qasr_enc_case& g, const void* in, const int32_t* idx, const int64_t* off, const float* pf,
                            const uint16_t* pw, void* out) {
    const EncCaseSizes z = enc_case_sizes(op, g);
    hipStream_t s = stream_;
    DevBuf dIn, dIdx, dOff, dPf, dPw, dOut;
    auto up = [&](DevBuf& d, const void* h, size_t n) {
        d.alloc(n);
        if (n) QASR_HIP(hipMemcpyAsync(d.p, h, n, hipMemcpyHostToDevice, s));
    };
    up(dIn, in, z.in_bytes); up(dIdx, idx, z.idx * sizeof(int32_t)); up(dOff, off, z.off * sizeof(int64_t));
    up(dPf, pf, z.pf * sizeof(float)); up(dPw, pw, z.pw * sizeof(bf16_t)); up(dOut, out, z.out_bytes);
    const int B = g.n_clips, D = g.D, rows = g.rows;
    const int* di = dIdx.as<int>();
    const float* dp = dPf.as<float>();
    switch (op) {
    case QASR_ENC_MHA: mha_attention_launch(dIn.as<bf16_t>(), di, B, g.max_len, g.heads, g.hd, dOut.as<bf16_t>(), s); break;
    case QASR_ENC_WINDOW: window_attention_launch(dIn.as<bf16_t>(), di, B, g.heads, g.hd, dOut.as<bf16_t>(), s); break;
    case QASR_ENC_LN_BF16: case QASR_ENC_LN_GELU_BF16:
        layernorm_f32p_launch(dIn.as<float>(), dp, dp + D, dOut.as<bf16_t>(), rows, D, g.eps, op == QASR_ENC_LN_GELU_BF16, s); break;
    case QASR_ENC_LN_GELU_F32: layernorm_gelu_f32_launch(dIn.as<float>(), dp, dp + D, dOut.as<float>(), rows, D, g.eps, s); break;
    case QASR_ENC_CONV0:
        w2v_conv0_launch(dIn.as<float>(), dOff.as<long>(), dp, di, di + B, B, g.max_len, dp + 2 * B, dp + 2 * B + 10 * D, dp + 2 * B + 11 * D,
                         dp + 2 * B + 12 * D, g.eps, dOut.as<bf16_t>(), D, s);
        break;
    case QASR_ENC_WAVE_STATS: wave_stats_launch(dIn.as<float>(), dOff.as<long>(), di, rows, g.eps, dOut.as<float>(), s); break;
    case QASR_ENC_CONV1:
        conv1_launch(dIn.as<float>(), g.mel_stride, g.n_mels, dIdx.as<ChunkMeta>(), rows, dPw.as<bf16_t>(), dp, dOut.as<bf16_t>(), g.H1, g.W1,
                     D, s);
        break;
    case QASR_ENC_ARGMAX:
        argmax_f32_launch(dIn.as<float>(), g.ld, rows, D, dOut.as<int>(), dOut.as<int>() + rows + g.out_extra, s); break;
    case QASR_ENC_CAST: cast_f32_bf16_launch(dIn.as<float>(), dOut.as<bf16_t>(), rows, s); break;
    case QASR_ENC_CONV_ROWS: w2v_conv_rows_launch(di, di + B, di + 2 * B, B, rows, g.stride, D, dOut.as<long>(), s); break;
    case QASR_ENC_FRAME_INFO: w2v_frame_info_launch(di, di + B, B, rows, dOut.as<int2>(), s); break;
    }
    QASR_HIP(hipGetLastError());
    if (z.out_bytes) QASR_HIP(hipMemcpyAsync(out, dOut.p, z.out_bytes, hipMemcpyDeviceToHost, s));
    QASR_HIP(hipStreamSynchronize(s));
}

}  // namespace qasr
