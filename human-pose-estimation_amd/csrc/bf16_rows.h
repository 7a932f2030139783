// bf16_rows.h -- slab geometry of the bf16 LDS-DMA GEMM kernels (conv_gemm_bf16.hip, conv_gemm_bf16_p8.hip).
// The per-lane source addressing is make_row<MODE, 8> of conv_gemm_common.h (8 bf16 per 16-byte chunk); the waits are lds_dma.h's.
#pragma once

#define BKE 64  // bf16 elements per k-slab (128 B)
#define RF 32   // floats per staged LDS row (128 B)
