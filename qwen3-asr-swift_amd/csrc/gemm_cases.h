// gemm_cases.h -- the dense half of qasr_gemm_case_probe (gemm_cases.hip): ADense with each fused epilogue, and the SwiGLU launch
#pragma once
#include "common.h"
#include "qasr.h"

namespace qasr {

// device pointers; bias is bf16 or f32 as the case's epilogue takes it (null: EpiBiasActBf16 without a bias); out is [rows][ld]
void gemm_case_dense_launch(int which, int form, const qasr_gemm_case& g, const bf16_t* A, const bf16_t* W, const void* bias,
                            const int* tok_t, const float* pe, void* out, long ld, hipStream_t s);

}  // namespace qasr
