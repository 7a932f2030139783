// lds_dma.h -- the LDS-DMA, wait and barrier idioms of the conv kernels, stated once (device code only): conv_gemm.hip,
// conv_gemm_f32s.hip, conv_stream_f32s.hip, conv_stream_chain_f32s.hip, conv_gemm_bf16.hip, conv_gemm_bf16_p8.hip, conv_chain_bf16.hip, conv_chain_f32.hip, conv3_halo_bf16.hip,
// conv_wino.hip and conv_wino4.hip.  The kernels say at each site only what is specific to it (which slab has landed, what stays in flight).
//
// The rules behind every primitive here:
//   * global_load_lds_dwordx4 writes LDS asynchronously and is tracked by vmcnt ONLY.  vmcnt is per wave and counts LDS-DMA, loads and
//     stores together, in issue order: "s_waitcnt vmcnt(n)" means all but the wave's n youngest vector-memory operations are done
//     (loads and DMA complete in order; a skipped store makes a count inexact).
//   * A barrier that publishes DMA'd data needs that wait in front of it, and it is WRITTEN OUT: __syncthreads() is a workgroup fence +
//     s_barrier, and what hipcc puts in front of it depends on the control flow around the DMA issue -- vmcnt(0) behind some patterns
//     (which drains a ring that was meant to stay in flight), lgkmcnt(0) alone behind others (round 3: conv_wino4.hip raced, whole
//     tile blocks wrong once >= 200 workgroups stretched the DMA latency).  So behind pending DMA the kernels use bare_barrier() /
//     lds_barrier() with their own wait; where a __syncthreads() stays, a written-out wait stands in front of it.
//   * tools/isa_lint.py (tests/test_isa_lint.py) walks the disassembly of every kernel: no path from a global_load_lds to an s_barrier
//     without an s_waitcnt that names vmcnt.  That is why some waits are spelled out where the queue is known to be empty.  Whether a
//     count is right is what the GPU parity tests check.
#pragma once
#include <hip/hip_runtime.h>

#include "hpe_internal.h"  // f32x4, f32x16

typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
// Per-channel scale / shift are read through the CONSTANT address space: the address is wave-uniform, so the loads become s_load (a
// kernel that also stores to global memory makes hipcc fall back to per-lane global_load for plain pointers -- those would queue
// behind the LDS-DMA in flight)
typedef const __attribute__((address_space(4))) float* cfloat_p;
typedef const __attribute__((address_space(4))) f32x4* cf32x4_p;

// ---- s_waitcnt immediates (gfx9 encoding: vmcnt = bits 3:0 and 15:14, expcnt = 6:4, left at 7 = unconstrained, lgkmcnt = 11:8)
constexpr int WAIT_NONE = -1;  // this counter is unconstrained
constexpr unsigned waitcnt_imm(int vm, int lgkm) {
    const unsigned v = vm == WAIT_NONE ? 63u : (unsigned)vm, l = lgkm == WAIT_NONE ? 15u : (unsigned)lgkm;
    return (v & 15u) | ((v >> 4) << 14) | (7u << 4) | (l << 8);
}
static_assert(waitcnt_imm(0, WAIT_NONE) == 0x0F70 && waitcnt_imm(8, WAIT_NONE) == 0x0F78 && waitcnt_imm(16, WAIT_NONE) == 0x4F70, "vmcnt field");
static_assert(waitcnt_imm(0, 0) == 0x0070 && waitcnt_imm(2, 0) == 0x0072 && waitcnt_imm(WAIT_NONE, 0) == 0xC07F, "lgkmcnt field");

// s_waitcnt vmcnt(VM) lgkmcnt(LGKM) through the builtin: no compiler fence of its own (the barrier or sched_barrier behind it is one)
template <int VM, int LGKM = WAIT_NONE>
__device__ __forceinline__ void wait_counts() {
    static_assert(VM >= WAIT_NONE && VM <= 63 && LGKM >= WAIT_NONE && LGKM <= 15, "counter range");
    __builtin_amdgcn_s_waitcnt(waitcnt_imm(VM, LGKM));
}

// The same vmcnt wait as inline asm with a "memory" clobber: also a compiler fence, which the chain and halo kernels rely on (their LDS
// accesses may not move across it).  n is a compile-time constant after unrolling (inline asm needs an immediate); a count nobody
// provided for stops the build instead of quietly draining the queue.  (conv_chain_bf16.hip keeps a switch of its own, see there.)
__device__ void wait_dma_leaving_unprovided() __attribute__((error("wait_dma_leaving: the count is not a compile-time constant in 0..16")));
#define HPE_VMCNT_CASE(N) \
    case N: asm volatile("s_waitcnt vmcnt(" #N ")" ::: "memory"); break
__device__ __forceinline__ void wait_dma_leaving(int n) {
    switch (n) {
        HPE_VMCNT_CASE(1); HPE_VMCNT_CASE(2); HPE_VMCNT_CASE(3); HPE_VMCNT_CASE(4); HPE_VMCNT_CASE(5); HPE_VMCNT_CASE(6);
        HPE_VMCNT_CASE(7); HPE_VMCNT_CASE(8); HPE_VMCNT_CASE(9); HPE_VMCNT_CASE(10); HPE_VMCNT_CASE(11); HPE_VMCNT_CASE(12);
        HPE_VMCNT_CASE(13); HPE_VMCNT_CASE(14); HPE_VMCNT_CASE(15); HPE_VMCNT_CASE(16);
        HPE_VMCNT_CASE(0);  // last on purpose: the order of the cases decides the block layout the kernels compile to
        default: wait_dma_leaving_unprovided();
    }
}
#undef HPE_VMCNT_CASE

// ---- 16 bytes per lane from global memory straight into LDS (a wave-instruction fills 1 KiB at lds_dst, lane l at + 16 l)
__device__ __forceinline__ void dma16(const void* src, void* lds_dst) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src, (__attribute__((address_space(3))) void*)lds_dst, 16, 0, 0);
}
// ... with the non-temporal cache policy (aux bit 1): data that is read exactly once
__device__ __forceinline__ void dma16_nt(const void* src, void* lds_dst) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src, (__attribute__((address_space(3))) void*)lds_dst, 16, 0, 2);
}

// ---- barriers that bring no wait of the compiler's
// this wave's LDS traffic is done, its DMAs stay in flight; the caller adds wait_dma_leaving() where the barrier publishes DMA'd data
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
// s_barrier alone between two compiler fences (no LDS access may be scheduled across it); every wait is the caller's wait_counts()
__device__ __forceinline__ void bare_barrier() {
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}
