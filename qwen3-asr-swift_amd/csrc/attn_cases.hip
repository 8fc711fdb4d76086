// attn_cases.hip -- qasr_attn_case_probe: the text decoder's attention and the kernels that write its K / V cache by themselves, on host
// data and a scratch cache of one layer.  Only plumbing lives here: uploads, the product's launch entries (dec_kernels.h) in the order
// run_prefill / the decode step call them, downloads.  The arguments were checked by the C ABI (api.cpp, attn_case_refusal): every index a
// launch forms from them stays inside the buffers allocated below.
#include "engine.h"
#include "dec_kernels.h"
#include <algorithm>
#include <vector>

namespace qasr {

void Engine::attn_case_probe(int op, const qasr_attn_case& g, uint16_t* qkv, const uint16_t* x, const uint16_t* W, const int32_t* cu,
                             const int32_t* slot_of_clip, const int32_t* pos, const int32_t* slot, const uint16_t* qn_w, const uint16_t* kn_w,
                             uint16_t* kcache, uint16_t* vfrag, const uint16_t* vt, uint16_t* qr, uint16_t* out) {
    const bool prompt = op == QASR_ATTN_PROMPT;
    const int hd = g.hd, half = hd / 2, nh = g.heads + 2 * g.kv_heads, P = g.n_pos;
    const size_t cache_bytes = (size_t)g.n_slots * g.kv_heads * g.max_ctx * hd * sizeof(bf16_t);
    const size_t qkv_bytes = (size_t)P * nh * hd * sizeof(bf16_t), q_bytes = (size_t)P * g.heads * hd * sizeof(bf16_t);
    hipStream_t s = stream_;
    std::vector<float> c, sn;
    rope_tables_host(g.rope_theta, half, g.max_ctx, c, sn);

    DevBuf dQkv, dK, dVf, dVt, dQr, dOut, dQn, dKn, dCos, dSin, dRows, dPos, dCu, dSoc, dSlot, dX, dW;
    dQkv.alloc(qkv_bytes); dK.alloc(cache_bytes); dVf.alloc(cache_bytes); dOut.alloc(q_bytes);
    dQn.alloc(hd * sizeof(bf16_t)); dKn.alloc(hd * sizeof(bf16_t));
    dCos.alloc(c.size() * sizeof(float)); dSin.alloc(sn.size() * sizeof(float));
    dPos.alloc((size_t)P * sizeof(int));
    auto up = [&](DevBuf& d, const void* h, size_t n) { QASR_HIP(hipMemcpyAsync(d.p, h, n, hipMemcpyHostToDevice, s)); };
    up(dQkv, qkv, qkv_bytes); up(dK, kcache, cache_bytes); up(dVf, vfrag, cache_bytes);
    up(dQn, qn_w, hd * sizeof(bf16_t)); up(dKn, kn_w, hd * sizeof(bf16_t));
    up(dCos, c.data(), c.size() * sizeof(float)); up(dSin, sn.data(), sn.size() * sizeof(float));
    up(dPos, pos, (size_t)P * sizeof(int));
    QASR_HIP(hipMemsetAsync(dOut.p, 0, q_bytes, s));
    KVLayout kv{dK.as<bf16_t>(), nullptr, g.max_ctx, g.kv_heads, hd, dVf.as<bf16_t>()};
    const bf16_t *qn = dQn.as<bf16_t>(), *kn = dKn.as<bf16_t>();

    if (prompt) {
        const int vt_stride = g.max_ctx;                       // a multiple of 64 that holds every clip
        int max_len = 0;
        for (int i = 0; i < g.n_clips; ++i) max_len = std::max(max_len, cu[i + 1] - cu[i]);
        dVt.alloc(cache_bytes); dQr.alloc(q_bytes);
        dCu.alloc((size_t)(g.n_clips + 1) * sizeof(int)); dSoc.alloc((size_t)g.n_clips * sizeof(int)); dSlot.alloc((size_t)P * sizeof(int));
        up(dVt, vt, cache_bytes); up(dQr, qr, q_bytes);
        up(dCu, cu, (size_t)(g.n_clips + 1) * sizeof(int)); up(dSoc, slot_of_clip, (size_t)g.n_clips * sizeof(int));
        up(dSlot, slot, (size_t)P * sizeof(int));
        bf16_t *dq = dQkv.as<bf16_t>(), *dqr = dQr.as<bf16_t>();
        if (g.route) {
            const int H = g.hidden;
            dX.alloc((size_t)P * H * sizeof(bf16_t)); dW.alloc((size_t)nh * hd * H * sizeof(bf16_t));
            up(dX, x, (size_t)P * H * sizeof(bf16_t)); up(dW, W, (size_t)nh * hd * H * sizeof(bf16_t));
            const ADense a{dX.as<bf16_t>(), H, P, H};
            if (g.route == 2)
                gemm_nt_headtiles(a, dW.as<bf16_t>(), H, P, nh * hd, H,
                                  EpiQkHeads{dq, (long)nh * hd, dqr, kv, dSlot.as<int>(), dPos.as<int>(), qn, kn, g.eps, dCos.as<float>(),
                                             dSin.as<float>(), g.heads, g.kv_heads}, s);
            else
                gemm_nt(a, dW.as<bf16_t>(), H, P, nh * hd, H, EpiStoreBf16{dq, (long)nh * hd}, s);
        }
        qk_norm_rope_launch(dq, dSlot.as<int>(), dPos.as<int>(), P, g.heads, g.kv_heads, hd, qn, kn, g.eps, dCos.as<float>(), dSin.as<float>(),
                            dqr, kv, dVt.as<bf16_t>(), vt_stride, dCu.as<int>(), dSoc.as<int>(), g.n_clips, max_len, s, g.route == 2);
        prefill_attention_launch(dqr, kv, dVt.as<bf16_t>(), vt_stride, dCu.as<int>(), dSoc.as<int>(), g.n_clips, max_len, g.heads,
                                 dOut.as<bf16_t>(), s);
    } else {
        dRows.alloc((size_t)2 * P * half * sizeof(float));
        const RopeRows rr{dCos.as<float>(), dSin.as<float>(), dRows.as<float>(), dRows.as<float>() + (size_t)P * half, half};
        refresh_rope_rows_launch(dPos.as<int>(), rr, P, s);
        decode_attention_launch(dQkv.as<bf16_t>(), dPos.as<int>(), P, g.heads, g.kv_heads, hd, qn, kn, g.eps, rr.cos_rows, rr.sin_rows, kv,
                                dOut.as<bf16_t>(), s);
    }
    QASR_HIP(hipGetLastError());
    auto down = [&](void* h, const DevBuf& d, size_t n) { QASR_HIP(hipMemcpyAsync(h, d.p, n, hipMemcpyDeviceToHost, s)); };
    down(out, dOut, q_bytes); down(kcache, dK, cache_bytes); down(vfrag, dVf, cache_bytes); down(qkv, dQkv, qkv_bytes);
    if (prompt) down(qr, dQr, q_bytes);
    QASR_HIP(hipStreamSynchronize(s));
}

}  // namespace qasr
