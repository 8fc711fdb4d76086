// gemm_cases_dense.hip -- see gemm_cases.h
#include "gemm_cases.h"
#include "ctc_kernels.h"
#include "enc_kernels.h"
#include "dec_kernels.h"

namespace qasr {

void gemm_case_dense_launch(int which, int form, const qasr_gemm_case& g, const bf16_t* A, const bf16_t* W, const void* bias,
                            const int* tok_t, const float* pe, void* out, long ld, hipStream_t s) {
    const ADense a{A, g.K, g.M, g.K};
    const int M = g.M, N = g.N, K = g.K;
    bf16_t* ob = (bf16_t*)out;
    float* of = (float*)out;
    const bf16_t* bb = (const bf16_t*)bias;
    const float* bf = (const float*)bias;
    switch (which) {
    case QASR_GEMM_CASE_BIAS_BF16: gemm_nt(a, W, K, M, N, K, EpiBiasActBf16<0>{ob, ld, bb}, s, form); break;
    case QASR_GEMM_CASE_BIAS_BF16_GELU: gemm_nt(a, W, K, M, N, K, EpiBiasActBf16<1>{ob, ld, bb}, s, form); break;
    case QASR_GEMM_CASE_BIASF_BF16: gemm_nt(a, W, K, M, N, K, EpiBiasActBf16F<0>{ob, ld, bf}, s, form); break;
    case QASR_GEMM_CASE_BIASF_BF16_GELU: gemm_nt(a, W, K, M, N, K, EpiBiasActBf16F<1>{ob, ld, bf}, s, form); break;
    case QASR_GEMM_CASE_STORE_BF16: gemm_nt(a, W, K, M, N, K, EpiStoreBf16{ob, ld}, s, form); break;
    case QASR_GEMM_CASE_RESID_F32: gemm_nt(a, W, K, M, N, K, EpiResidF32{of, ld, bb}, s, form); break;
    case QASR_GEMM_CASE_RESID_F32F: gemm_nt(a, W, K, M, N, K, EpiResidF32F{of, ld, bf}, s, form); break;
    case QASR_GEMM_CASE_RESID_BF16: gemm_nt(a, W, K, M, N, K, EpiResidBf16{ob, ld}, s, form); break;
    case QASR_GEMM_CASE_POS_F32: gemm_nt(a, W, K, M, N, K, EpiPosF32{of, ld, pe, tok_t}, s, form); break;
    case QASR_GEMM_CASE_SWIGLU: gemm_nt_swiglu(a, W, K, M, N, K, EpiStoreBf16{ob, ld}, s, form); break;
    default: throw std::invalid_argument("gemm case: not a dense case");
    }
}

}  // namespace qasr
