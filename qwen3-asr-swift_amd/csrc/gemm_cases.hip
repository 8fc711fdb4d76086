// gemm_cases.hip -- qasr_gemm_case_probe: one operand gather + fused epilogue pair of the product's GEMM (gemm.h) by itself, on host data.
// Every case builds the functor types the product builds and goes through the product's launch entry (gemm_nt / gemm_nt_groups /
// gemm_nt_swiglu); nothing of a gather or an epilogue is restated here.  The arguments were checked by the C ABI (api.cpp,
// gemm_case_refusal): every index a launch forms from them stays inside the uploaded arrays.  The dense cases live in gemm_cases_dense.hip
// (a second translation unit only so that the two compile side by side).
#include "engine.h"
#include "ctc_kernels.h"
#include "enc_kernels.h"
#include "gemm_cases.h"
#include <vector>

namespace qasr {

// EpiBiasF32 per group of the grouped launch: group g writes columns [g * cpg, (g + 1) * cpg) of out with that slice of the bias
struct EpiBiasF32Group : EpiBiasF32 {
    int cpg;
    __device__ __forceinline__ EpiBiasF32Group for_group(int grp) const {
        EpiBiasF32Group e = *this;
        e.out += grp * cpg;
        e.bias += grp * cpg;
        return e;
    }
};

template <class A>
static void conv_case(int which, int form, const qasr_gemm_case& g, const A& a, const bf16_t* W, const float* bias, const ChunkMeta* chunks,
                      int OH, int OW, void* out, long ld, hipStream_t s) {
    if (which == QASR_GEMM_CASE_CONV)
        gemm_nt(a, W, g.K, g.M, g.N, g.K, EpiConvGelu{(bf16_t*)out, ld, bias, chunks, OH, OW, g.hw_major != 0, g.level}, s, form);
    else
        gemm_nt(a, W, g.K, g.M, g.N, g.K, EpiBiasF32{(float*)out, ld, bias}, s, form);
}

void Engine::gemm_case_probe(int which, int form, const qasr_gemm_case& g, const uint16_t* A, const uint16_t* W, const void* bias,
                             const int32_t* aux_i, const int64_t* aux_l, const float* aux_f, void* out) {
    const bool conv = which == QASR_GEMM_CASE_CONV || which == QASR_GEMM_CASE_CONV_PLAIN;
    const bool grouped = which == QASR_GEMM_CASE_GROUPCONV || which == QASR_GEMM_CASE_GROUPCONV_PLAIN;
    const bool swiglu = which == QASR_GEMM_CASE_SWIGLU;
    const int D = g.groups * g.cpg;
    const long width = grouped ? D : swiglu ? g.N / 2 : g.N;
    const long ld = g.ld ? g.ld : width, rows = g.out_rows ? g.out_rows : g.M;
    const bool out_bf16 = which == QASR_GEMM_CASE_CONV || which == QASR_GEMM_CASE_BIAS_BF16 || which == QASR_GEMM_CASE_BIAS_BF16_GELU ||
                          which == QASR_GEMM_CASE_BIASF_BF16 || which == QASR_GEMM_CASE_BIASF_BF16_GELU ||
                          which == QASR_GEMM_CASE_STORE_BF16 || which == QASR_GEMM_CASE_RESID_BF16 || swiglu;
    const bool bias_bf16 = which == QASR_GEMM_CASE_BIAS_BF16 || which == QASR_GEMM_CASE_BIAS_BF16_GELU || which == QASR_GEMM_CASE_RESID_F32;
    const size_t a_elems = conv ? (size_t)g.n_img * g.H * g.W * g.C : which == QASR_GEMM_CASE_ROWTABLE ? (size_t)g.a_len
                         : grouped ? (size_t)g.M * D : (size_t)g.M * g.K;
    const size_t w_elems = (grouped ? (size_t)g.groups : 1) * g.N * g.K;
    const size_t out_bytes = (size_t)rows * ld * (out_bf16 ? 2 : 4);
    const size_t bias_bytes = (size_t)width * (bias_bf16 ? 2 : 4);
    // int records: conv valid widths (as ChunkMeta) | frame (t, L) | tok_t;  float rows: the positional conv's residual | the pe table
    std::vector<ChunkMeta> chunks;
    if (which == QASR_GEMM_CASE_CONV) {
        chunks.resize(g.n_img);
        for (int i = 0; i < g.n_img; ++i) {
            chunks[i] = ChunkMeta{};
            chunks[i].w2 = chunks[i].w3 = aux_i[i];
        }
    }
    const size_t ai_bytes = which == QASR_GEMM_CASE_CONV ? chunks.size() * sizeof(ChunkMeta) : grouped ? (size_t)g.M * 8
                          : which == QASR_GEMM_CASE_POS_F32 ? (size_t)g.M * 4 : 0;
    const void* ai_src = which == QASR_GEMM_CASE_CONV ? (const void*)chunks.data() : (const void*)aux_i;
    const size_t af_bytes = which == QASR_GEMM_CASE_GROUPCONV ? (size_t)g.M * D * 4 : which == QASR_GEMM_CASE_POS_F32 ? (size_t)g.n_t * ld * 4 : 0;
    const size_t al_bytes = which == QASR_GEMM_CASE_ROWTABLE ? (size_t)g.M * sizeof(long) : 0;
    static_assert(sizeof(long) == sizeof(int64_t), "row offsets are 64-bit");

    DevBuf dA, dW, dB, dO, dI, dL, dF;
    dA.alloc(a_elems * 2); dW.alloc(w_elems * 2); dB.alloc(bias_bytes); dO.alloc(out_bytes);
    dI.alloc(ai_bytes); dL.alloc(al_bytes); dF.alloc(af_bytes);
    hipStream_t s = stream_;
    QASR_HIP(hipMemcpyAsync(dA.p, A, a_elems * 2, hipMemcpyHostToDevice, s));
    QASR_HIP(hipMemcpyAsync(dW.p, W, w_elems * 2, hipMemcpyHostToDevice, s));
    if (bias) QASR_HIP(hipMemcpyAsync(dB.p, bias, bias_bytes, hipMemcpyHostToDevice, s));
    QASR_HIP(hipMemcpyAsync(dO.p, out, out_bytes, hipMemcpyHostToDevice, s));
    if (ai_bytes) QASR_HIP(hipMemcpyAsync(dI.p, ai_src, ai_bytes, hipMemcpyHostToDevice, s));
    if (al_bytes) QASR_HIP(hipMemcpyAsync(dL.p, aux_l, al_bytes, hipMemcpyHostToDevice, s));
    if (af_bytes) QASR_HIP(hipMemcpyAsync(dF.p, aux_f, af_bytes, hipMemcpyHostToDevice, s));
    QASR_HIP(hipStreamSynchronize(s));                      // `chunks` is pageable host memory of this frame

    const bf16_t *a = dA.as<bf16_t>(), *w = dW.as<bf16_t>();
    if (conv) {
        const int OH = (g.H - 1) / 2 + 1, OW = (g.W - 1) / 2 + 1;
        const AConv3x3s2 ac{a, g.H, g.W, g.C, OH, OW, g.M, g.K, g.hw_major != 0};
        if (g.wide) conv_case(which, form, g, AConv3x3s2W{ac}, w, dB.as<float>(), dI.as<ChunkMeta>(), OH, OW, dO.p, ld, s);
        else conv_case(which, form, g, ac, w, dB.as<float>(), dI.as<ChunkMeta>(), OH, OW, dO.p, ld, s);
    } else if (which == QASR_GEMM_CASE_ROWTABLE) {
        gemm_nt(ARowTable{a, dL.as<long>(), g.M, g.K}, w, g.K, g.M, g.N, g.K, EpiBiasF32{dO.as<float>(), ld, dB.as<float>()}, s, form);
    } else if (grouped) {
        const AGroupConv1d ag{a, dI.as<int2>(), D, g.cpg, g.KP, 0, g.M};
        const long ldw = (long)g.KP * g.cpg, wgs = (long)g.cpg * g.KP * g.cpg;
        if (which == QASR_GEMM_CASE_GROUPCONV)
            gemm_nt_groups(ag, w, ldw, wgs, g.groups, g.M, g.cpg, g.K, EpiPosConv{dO.as<float>(), dF.as<float>(), D, dB.as<float>(), 0, g.cpg}, s);
        else
            gemm_nt_groups(ag, w, ldw, wgs, g.groups, g.M, g.cpg, g.K, EpiBiasF32Group{{dO.as<float>(), D, dB.as<float>()}, g.cpg}, s);
    } else {
        gemm_case_dense_launch(which, form, g, a, w, bias ? dB.p : nullptr, dI.as<int>(), dF.as<float>(), dO.p, ld, s);
    }
    QASR_HIP(hipGetLastError());
    QASR_HIP(hipMemcpyAsync(out, dO.p, out_bytes, hipMemcpyDeviceToHost, s));
    QASR_HIP(hipStreamSynchronize(s));
}

}  // namespace qasr
