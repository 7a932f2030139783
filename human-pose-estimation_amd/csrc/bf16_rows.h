// bf16_rows.h -- slab geometry and counted waits of the bf16 LDS-DMA kernels (conv_gemm_bf16.hip, conv_gemm_bf16_p8.hip, conv_chain_bf16.hip).
// The per-lane source addressing is make_row<MODE, 8> of conv_gemm_common.h (8 bf16 per 16-byte chunk).
#pragma once
#include <hip/hip_runtime.h>

#include "hpe_internal.h"

#define BKE 64  // bf16 elements per k-slab (128 B)
#define RF 32   // floats per staged LDS row (128 B)

// s_waitcnt vmcnt(n), n <= 63, everything else unconstrained (gfx9 encoding: vmcnt = bits 3:0 and 15:14, expcnt 6:4, lgkmcnt 11:8)
#define HPE_WAIT_VMCNT(n) __builtin_amdgcn_s_waitcnt(0x0F70 | ((n) & 15) | (((n) >> 4) << 14))
// s_waitcnt lgkmcnt(0), vmcnt / expcnt unconstrained
#define HPE_WAIT_LGKM0() __builtin_amdgcn_s_waitcnt(0xC07F)
