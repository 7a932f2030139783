// gemm_contract.h -- the tile table and the host-side shape contract of the four implicit-GEMM launchers (conv_gemm.hip, conv_gemm_f32s.hip,
// conv_gemm_bf16.hip, conv_gemm_bf16_p8.hip), stated once.  Checked before every launch so that a bad plan cannot fault on the device.
// Host code only, no HIP runtime call; tests/gemm_ref.py restates the clauses by the same names (DESIGN.md section 4 has the table).
#pragma once
#include <stdint.h>

#include "hpe_internal.h"

enum GemmKernel { GEMM_K_F32 = 0, GEMM_K_F32S = 1, GEMM_K_BF16 = 2, GEMM_K_BF16_P8 = 3 };

// workgroup tile bm x bn as a wm x wn grid of waves; bm == 0: this kernel has no such tile
struct TileShape {
    int bm, bn, wm, wn;
};

constexpr TileShape tile_shape(GemmKernel k, int tile) {
    if (k == GEMM_K_F32 || k == GEMM_K_BF16) {
        switch (tile) {
            case TILE_128x128: return {128, 128, 2, 2};
            case TILE_128x64: return {128, 64, 2, 2};
            case TILE_64x64: return {64, 64, 2, 2};
            case TILE_64x128: return {64, 128, 2, 2};
            case TILE_128x128_W8: return {128, 128, 2, 4};
            case TILE_128x64_W8: return {128, 64, 4, 2};
            case TILE_256x128_W8: return {256, 128, 4, 2};
        }
    } else if (k == GEMM_K_F32S) {  // WN = 1 on the 4-wave tile: every A element is split by exactly one wave
        switch (tile) {
            case TILE_128x128: return {128, 128, 4, 1};
            case TILE_128x128_W8: return {128, 128, 4, 2};
            case TILE_256x128_W8: return {256, 128, 8, 1};
        }
    } else if (tile == TILE_P8_256x256) {
        return {256, 256, 2, 4};
    }
    return {0, 0, 0, 0};
}

// what the clauses are parametrised by: elements per 16-B vector of the activations / of the weights, elements per k-slab, the modes
struct GemmRules {
    int gran, wgran, slab;
    bool conv3, stem;
};

constexpr GemmRules gemm_rules(GemmKernel k) {
    return k == GEMM_K_F32 ? GemmRules{4, 4, 32, true, true}
         : k == GEMM_K_F32S ? GemmRules{4, 8, 32, false, false}
         : k == GEMM_K_BF16 ? GemmRules{8, 8, 64, true, true}
                            : GemmRules{8, 8, 64, true, false};
}

// nullptr: the launch is inside the contract of kernel k; else the name of the first clause it breaks
inline const char* gemm_contract(const GemmArgs& p, int mode, int tile, GemmKernel k) {
    const GemmRules r = gemm_rules(k);
    const int BK_ = r.slab;
    const bool g4 = r.gran == 4, s32 = BK_ == 32;
    auto misaligned = [](const void* q) { return ((uintptr_t)q & 15) != 0; };
#define HPE_CLAUSE(broken, name) \
    if (broken) return name
    HPE_CLAUSE(p.M <= 0, "M > 0");
    HPE_CLAUSE(p.N <= 0, "N > 0");
    HPE_CLAUSE(p.K <= 0, "K > 0");
    HPE_CLAUSE(p.K % BK_ != 0, s32 ? "K % 32 == 0" : "K % 64 == 0");
    HPE_CLAUSE(p.ldw % r.wgran != 0, r.wgran == 4 ? "ldw % 4 == 0" : "ldw % 8 == 0");
    if (k == GEMM_K_F32S) {  // three bf16 pieces per weight row, w_piece elements apart
        HPE_CLAUSE(p.w_piece % 8 != 0, "w_piece % 8 == 0");
        HPE_CLAUSE(p.w_piece < p.K, "w_piece >= K");
        HPE_CLAUSE(p.ldw < p.K + 2 * p.w_piece, "ldw >= K + 2 * w_piece");
    } else {
        HPE_CLAUSE(p.ldw < p.K, "ldw >= K");
    }
    HPE_CLAUSE(!p.x, "x != NULL");
    HPE_CLAUSE(!p.w, "wt != NULL");
    HPE_CLAUSE(!p.y, "y != NULL");
    HPE_CLAUSE(!p.scale, "scale != NULL");
    HPE_CLAUSE(!p.shift, "shift != NULL");
    HPE_CLAUSE(k != GEMM_K_F32S && !p.zero, "zero != NULL");  // f32s has no 3x3 mode and no tail k-tiles: it never reads the zero page
    // vector epilogue: 16-B aligned rows of y / residual
    HPE_CLAUSE(p.ldy % r.gran != 0, g4 ? "ldy % 4 == 0" : "ldy % 8 == 0");
    HPE_CLAUSE(misaligned(p.y), "y aligned");
    HPE_CLAUSE(g4 && p.y_slab8 && p.N % 8 != 0, "y_slab8 needs N % 8 == 0");  // the bf16 kernels have no slab-major output
    HPE_CLAUSE(p.res && p.ldres % r.gran != 0, g4 ? "ldres % 4 == 0" : "ldres % 8 == 0");
    HPE_CLAUSE(p.res && misaligned(p.res), "residual aligned");
    HPE_CLAUSE(misaligned(p.x), "x aligned");
    HPE_CLAUSE(misaligned(p.w), "wt aligned");
    const TileShape ts = tile_shape(k, tile);
    HPE_CLAUSE(ts.bm == 0, k == GEMM_K_F32 || k == GEMM_K_BF16 ? "tile in 0..6" : k == GEMM_K_F32S ? "tile in {0, 4, 6}" : "tile == 7");
    if (k == GEMM_K_BF16_P8) {  // weight rows past w_rows are clamped, not read; DMAs past K come from the zero page; split-K stores 16 B per lane
        HPE_CLAUSE(p.w_rows < 1, "w_rows >= 1");
        HPE_CLAUSE(misaligned(p.zero), "zero aligned");
        HPE_CLAUSE(p.partial && misaligned(p.partial), "partial aligned");
    } else {
        HPE_CLAUSE((p.N + ts.bn - 1) / ts.bn * ts.bn > p.w_rows, "w_rows covers the padded N");
    }
    const bool strided = mode == GEMM_STRIDED || mode == GEMM_DUAL;
    HPE_CLAUSE(!(mode == GEMM_DENSE || strided || (mode == GEMM_CONV3 && r.conv3) || (mode == GEMM_STEM && r.stem)), "mode");
    if (mode == GEMM_DENSE) HPE_CLAUSE(p.lda < p.K, "lda >= K");
    if (mode == GEMM_DUAL) {
        HPE_CLAUSE(!p.x2, "x2 != NULL");
        HPE_CLAUSE(misaligned(p.x2), "x2 aligned");
        HPE_CLAUSE(p.k1_slabs < 1, "k1_slabs >= 1");
        HPE_CLAUSE(p.k1_slabs * BK_ >= p.K, s32 ? "k1_slabs * 32 < K" : "k1_slabs * 64 < K");
        HPE_CLAUSE(p.lda < p.k1_slabs * BK_, s32 ? "lda >= k1_slabs * 32" : "lda >= k1_slabs * 64");
    }
    if (mode == GEMM_DENSE || mode == GEMM_DUAL) HPE_CLAUSE(p.lda % r.gran != 0, g4 ? "lda % 4 == 0" : "lda % 8 == 0");
    if (strided) {
        HPE_CLAUSE(p.Cin != (mode == GEMM_DUAL ? p.K - p.k1_slabs * BK_ : p.K),
                   mode != GEMM_DUAL ? "Cin == K" : s32 ? "Cin == K - k1_slabs * 32" : "Cin == K - k1_slabs * 64");
        HPE_CLAUSE(p.Cin % r.gran != 0, g4 ? "Cin % 4 == 0" : "Cin % 8 == 0");
        HPE_CLAUSE(p.Ho < 1 || p.Wo < 1 || p.stride < 1, "Ho, Wo, stride >= 1");  // host and kernel divide by Ho * Wo and by Wo
        HPE_CLAUSE(mode == GEMM_DUAL && p.M % (p.Ho * p.Wo) != 0, "M % (Ho * Wo) == 0");
        HPE_CLAUSE((p.Ho - 1) * p.stride >= p.Hi, "(Ho - 1) * stride < Hi");
        HPE_CLAUSE((p.Wo - 1) * p.stride >= p.Wi, "(Wo - 1) * stride < Wi");
    } else if (mode == GEMM_CONV3) {
        HPE_CLAUSE(p.Cin % BK_ != 0, s32 ? "Cin % 32 == 0" : "Cin % 64 == 0");
        HPE_CLAUSE(p.K != 9 * p.Cin, "K == 9 * Cin");
        HPE_CLAUSE(p.cin_slabs != p.Cin / BK_, s32 ? "cin_slabs == Cin / 32" : "cin_slabs == Cin / 64");
        HPE_CLAUSE(k == GEMM_K_BF16_P8 && (p.cin_slabs & (p.cin_slabs - 1)) != 0, "cin_slabs a power of two");  // p8 finds the tap by a shift
        HPE_CLAUSE(p.Ho != p.Hi, "Ho == Hi");
        HPE_CLAUSE(p.Wo != p.Wi, "Wo == Wi");
        HPE_CLAUSE(p.Hi < 1 || p.Wi < 1, "Hi, Wi >= 1");  // the kernel divides by Ho * Wo and by Wo
    } else if (mode == GEMM_STEM) {  // padded input [B,Hi,Wi,4]: fp32 one kernel row (8 px) per slab, 7 slabs; bf16 two rows per slab, 4 slabs
        HPE_CLAUSE(p.K != (s32 ? 7 : 4) * BK_, s32 ? "K == 7 * 32" : "K == 4 * 64");
        HPE_CLAUSE(p.Hi < 2 * (p.Ho - 1) + (s32 ? 7 : 8), s32 ? "Hi >= 2 * (Ho - 1) + 7" : "Hi >= 2 * (Ho - 1) + 8");
        HPE_CLAUSE(p.Wi < 2 * (p.Wo - 1) + 8, "Wi >= 2 * (Wo - 1) + 8");
    }
#undef HPE_CLAUSE
    return nullptr;
}
