// syn_attn_cases.hip -- qasr_syn_attn_case_probe: the attention kernels of the speech-synthesis stacks by themselves, on host data.  Only
// plumbing lives here: uploads, ONE call of the product's launch entry (two for the CosyVoice pair, in the order CosyLlm::layers calls
// them), downloads.  The arguments were checked by the C ABI (api.cpp, syn_attn_case_refusal): every index a launch forms from them stays
// inside the buffers allocated below, whose sizes are the caller's arrays'.
#include "engine.h"
#include "llm_cosyvoice.h"
#include "loc_voxcpm.h"
#include "tts_talker.h"

namespace qasr {

void Engine::syn_attn_case_probe(int op, const qasr_syn_attn_case& g, const void* qkv, const int32_t* slot, const int32_t* pos,
                                 const uint16_t* qn_w, const uint16_t* kn_w, const float* cos, const float* sin, uint16_t* kcache,
                                 uint16_t* vcache, uint16_t* qr, void* out) {
    hipStream_t s = stream_;
    const size_t esz = op == QASR_SYN_VL ? sizeof(float) : sizeof(bf16_t);
    const size_t qkv_bytes = (size_t)g.qkv_elems * esz, out_bytes = (size_t)g.out_elems * esz, tab_bytes = (size_t)g.table_elems * sizeof(float);
    const size_t cache_bytes = (size_t)g.cache_elems * sizeof(bf16_t);
    DevBuf dQkv, dOut, dCos, dSin, dK, dV, dQr, dSlot, dPos, dQn, dKn;
    auto up = [&](DevBuf& d, const void* h, size_t n) { d.alloc(n); QASR_HIP(hipMemcpyAsync(d.p, h, n, hipMemcpyHostToDevice, s)); };
    auto down = [&](void* h, const DevBuf& d, size_t n) { QASR_HIP(hipMemcpyAsync(h, d.p, n, hipMemcpyDeviceToHost, s)); };
    up(dQkv, qkv, qkv_bytes); up(dOut, out, out_bytes); up(dCos, cos, tab_bytes); up(dSin, sin, tab_bytes);
    if (op != QASR_SYN_VL) { up(dK, kcache, cache_bytes); up(dV, vcache, cache_bytes); }
    if (op == QASR_SYN_CVLM) {
        up(dQr, qr, out_bytes); up(dSlot, slot, (size_t)g.rows * sizeof(int)); up(dPos, pos, (size_t)g.rows * sizeof(int));
        cvlm_rope_append_launch(dQkv.as<bf16_t>(), dSlot.as<int>(), dPos.as<int>(), g.rows, g.heads, g.kv_heads, dCos.as<float>(), dSin.as<float>(),
                                dQr.as<bf16_t>(), dK.as<bf16_t>(), dV.as<bf16_t>(), g.max_ctx, s);
        cvlm_attention_launch(dQr.as<bf16_t>(), dSlot.as<int>(), dPos.as<int>(), g.rows, g.heads, g.kv_heads, dK.as<bf16_t>(), dV.as<bf16_t>(),
                              g.max_ctx, dOut.as<bf16_t>(), s);
    } else if (op == QASR_SYN_CP) {
        up(dQn, qn_w, 128 * sizeof(bf16_t)); up(dKn, kn_w, 128 * sizeof(bf16_t));
        tts_cp_attn_launch(dQkv.as<bf16_t>(), g.pos, g.rows, g.heads, g.kv_heads, dQn.as<bf16_t>(), dKn.as<bf16_t>(), g.eps, dCos.as<float>(),
                           dSin.as<float>(), dK.as<bf16_t>(), dV.as<bf16_t>(), dOut.as<bf16_t>(), s);
    } else {
        vl_attention_launch(dQkv.as<float>(), g.n_seq, g.S, g.heads, g.kv_heads, dCos.as<float>(), dSin.as<float>(), dOut.as<float>(), s);
    }
    QASR_HIP(hipGetLastError());
    down(out, dOut, out_bytes);
    if (op != QASR_SYN_VL) { down(kcache, dK, cache_bytes); down(vcache, dV, cache_bytes); }
    if (op == QASR_SYN_CVLM) down(qr, dQr, out_bytes);
    QASR_HIP(hipStreamSynchronize(s));
}

}  // namespace qasr
