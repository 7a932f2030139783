// hpe_plan.h -- the launch plan of one context: every option that decides which kernel runs and how it is launched, resolved ONCE
// (hpe_finalize, or the first loss call of a loss-only context) by hpe_resolve_plan() from the table in hpe_plan.hip, and the dispatch over
// it: layer_packs() says which packings a layer holds, route_conv() / route_block() which kernel, tile and layouts a launch takes.  All of
// it is pure host logic of (plan, dtype, layer, query): no pointer, no HIP call.  hpe_plan.hip is the only file of the library that reads the
// environment; the launchers are pure functions of their arguments.
#pragma once
#include "../../include/hpe.h"
#include "hpe_internal.h"

struct HpePlan {
    // ---- options with an HpeConfig field (HpeConfig field if >= 0, else the environment variable, else the default; see include/hpe.h)
    int n_streams = 2;          // batch-chunk streams of the encoder, 1..4
    int dual_gemm = 1;          // conv_block: branch2c + branch1 in one launch (0: two launches through the shortcut buffer)
    int stem_fused = 1;         // conv1 + BN + ReLU + max-pool as one kernel reading the raw images (0: pad / im2col GEMM / pool)
    int wino_min_c = 128;       // 3x3 layers with at least this many channels take the Winograd path (0 disables it)
    int wino_min_items = 128;   // ... when the launch has at least this many workgroups
    int wino_fused = 1;         // 56x56 / 28x28 maps: input transform inside the GEMM kernel, fed by a slab-major 1x1 producer
    int wino_fused_min_hw = 28; // smallest map side on the fused path
    int mesh_a2b = 0;           // pixel -> vertex search of the mesh loss: 0 cell grid, 1 VALU full search, 2 matrix-core full search
    int wino_f4 = 7;            // map sizes whose 3x3 layers run as Winograd F(4x4,3x3): bit 0: 7x7, 1: 14x14, 2: 28x28, 3: 56x56
    int wino4_fused = 0;        // map sizes (bits as wino_f4: 4 = 28x28, 8 = 56x56) whose F(4x4) layers take the fused-transform kernel
    int bf16_p8 = 0;            // layer kinds that take the 256 x 256 phase-interleaved kernel (bit mask, see pick_bf16)
    int wino4_ksplit = 1;       // F(4x4) launches with few workgroups cut their C axis
    int chain_fuse = 0;         // bf16: stages (bit 0: stage 2, 1: stage 3, 2: the conv_block of stage 2, 4: stage 4) whose identity blocks run
                                // branch2c + the next block's branch2a as one launch (conv_chain_bf16.hip); fp32: bit 3 (conv_chain_f32.hip)
    int halo3 = 0;              // bf16 only: map sizes (1 = 7x7, 2 = 14x14, 4 = 28x28, 8 = 56x56) whose 3x3 layers run on conv3_halo_bf16.hip
    int f32_split = 0;          // fp32 only: stages (1 = stage 2 ... 8 = stage 5) whose 1x1 / strided / dual layers run on conv_gemm_f32s.hip
    // ---- options of the environment only (tests and tools)
    int chunk_images = 0;       // HPE_CHUNK: images per batch chunk (0: one chunk per stream)
    int min_chunk = 32;         // HPE_MIN_CHUNK: smallest batch chunk that still gets its own stream
    int halo3_two = 4;          // HPE_HALO3_TWO: map sizes of halo3 on the two-workgroups-per-CU form of that kernel (default: 28x28)
    int f32s_min_tiles = 128;   // HPE_F32S_MIN_TILES: launches with fewer tiles than this keep the fp32 kernel (and its split-K)
    int stream1x1 = 15;         // HPE_STREAM1X1: forms on conv_stream_f32s.hip (1: identity-block expand layers with K <= 128; 2: the dual-source
                                // launch of res2a) and its chained forms on conv_stream_chain_f32s.hip (4: res2b_branch2c + res2c_branch2a instead of
                                // conv_chain_f32.hip; 8: the dual-source launch of res2a + res2b_branch2a); needs f32_split != 0 (= 0 is the fp32-MFMA plan)
    int stream1x1_min_m = 25088;  // HPE_STREAM1X1_MIN_M: launches with fewer rows keep the fp32 GEMM (default: 8 images of 56x56, 32 of 28x28)
    int stream1x1_walkers = 0;  // HPE_STREAM1X1_WALKERS: cap on the workgroups per 128-cout slice of such a launch (0: two workgroups per CU)
    int wino_streamk = 0;       // HPE_WINO_STREAMK: persistent stream-K scheduling of the F(2x2) Winograd GEMM
    int concurrent_tiles = 0;   // HPE_CONCURRENT_TILES=1: the tile rule of concurrent chunk launches on every launch (profiling passes with HPE_STREAMS=1)
    int bf16_w8_min_tiles = 128;  // HPE_BF16_W8_MIN_TILES: N > 64 bf16 launches with >= this many 128 x 128 tiles use the 8-wave tile (0 = never)
    int wide128_min_tiles = 384;  // HPE_WIDE128_MIN_TILES: 1.5 tiles per CU (0 = the round-1 rule everywhere)
    int force_wide = -1;        // HPE_TILE_WIDE: fp32 tile of every N > 64 launch that is not an expand layer (-1: per-layer rule)
    int splitk_min_slabs = 4;   // HPE_SPLITK_SLABS: k-slabs per split-K slice of the fp32 GEMM, >= 2
    int wino4_min_items = 64;   // HPE_WINO4_MIN_ITEMS: F(4x4) launches need at least this many 32-cout workgroups, else F(2x2) / direct by their rules
    int wino4_n32 = 256;        // HPE_WINO4_N32: F(4x4) launches with fewer 64-cout workgroups on the device take the 32-cout GEMM (0 = never)
    int w4_abl = 0;             // HPE_W4_ABL: ablation mask of the F(4x4) GEMM (diagnostics builds with -DHPE_ABLATION only; results wrong)
};

// Values that were sweep knobs of the environment while they were being measured and are fixed now (DESIGN.md has the measurements)
constexpr int PLAN_BF16_128_MIN_TILES = 192;  // concurrent bf16 chunk launches take 128x128 from 0.75 tiles per CU on
constexpr int PLAN_BF16_P8_MIN_N = 256;       // smallest N / K of a launch on the bf16_p8 kernel
constexpr int PLAN_BF16_P8_MIN_K = 512;
constexpr int PLAN_EXPAND_SMALL_GRID = 128;   // fp32 expand layers with fewer 128x64 tiles than this take the 64x64 split-K tile
constexpr int PLAN_SHORTK_TILE = TILE_128x64_W8;        // fp32 tile of the K <= 128 layers on the huge-M maps
constexpr int PLAN_F32S_TILE = TILE_128x128;            // tile of the split-bf16 fp32 kernel
constexpr int PLAN_F32S_EXPAND_TILE = TILE_128x128_W8;  // ... of the identity-block expand layers (+ residual)
constexpr int PLAN_F32S_EXPAND_MIN_K = 256;   // expand layers with a shorter k axis keep the fp32 kernel (stage 3: all epilogue)

// cfg.encoder_dtype decides the dtype-dependent defaults and masks
HpePlan hpe_resolve_plan(const HpeConfig& cfg);

// bit of a layer's ResNet stage in the f32_split mask, by its output map: 56x56 stage 2 (1), 28x28 stage 3 (2), 14x14 stage 4 (4), 7x7 stage 5 (8)
inline int stage_bit(int hout) { return hout >= 56 ? 1 : (hout >= 28 ? 2 : (hout >= 14 ? 4 : 8)); }
// bit of a 3x3 layer's map size in wino_f4 / wino4_fused / halo3
inline int f4_bit(int hin) { return hin <= 7 ? 1 : (hin <= 14 ? 2 : (hin <= 28 ? 4 : 8)); }

// ---- the dispatch ("The conv dispatch").  Packings of a layer: bit 1 << HPE_PACK_* of include/hpe.h
constexpr unsigned PACK_W_SPLIT = 1u << HPE_PACK_W_SPLIT, PACK_WINO_U = 1u << HPE_PACK_WINO_U, PACK_WINO4_U = 1u << HPE_PACK_WINO4_U,
                   PACK_STEM_W = 1u << HPE_PACK_STEM_W, PACK_W_DUAL = 1u << HPE_PACK_W_DUAL, PACK_W_DUAL_SPLIT = 1u << HPE_PACK_W_DUAL_SPLIT;
// which of them hpe_finalize packs for layer idx: the rule, not its side effect
unsigned layer_packs(const HpePlan& pl, bool bf16, int idx);
// layer idx is one conv_stream_f32s.hip takes at some batch: hpe_finalize then keeps its split weights ([n_pad][3][k], ConvLayer::w_stream)
bool stream1x1_layer(const HpePlan& pl, bool bf16, int idx);

// one launcher each; the first four are GemmKernel's (gemm_contract.h)
enum ConvKernel { CONV_K_F32 = 0, CONV_K_F32S, CONV_K_BF16, CONV_K_BF16_P8, CONV_K_HALO3, CONV_K_WINO, CONV_K_WINO_FUSED, CONV_K_WINO4, CONV_K_WINO4_FUSED };
// what a launch is asked with: images, a batch chunk running beside others, a residual operand, a slice of the Winograd V workspace
struct ConvQuery { int B; bool concurrent, residual, workspace; };
struct ConvRoute {
    int kernel, mode, tile;  // ConvKernel, GemmMode, GemmTile (-1: the kernel has none)
    bool in_slab8;           // the kernel reads its input channel-slab major (the fused Winograd kernels)
    bool out_slab8;          // ... and so must its producer write it (route_block sets it on branch2a)
    bool concurrent;         // of the query: such a launch never takes the context's one split-K workspace
    bool stream;             // the launch runs on conv_stream_f32s.hip instead; kernel / tile name the GEMM it takes with HPE_STREAM1X1=0
};
enum BlockJoin { JOIN_SEPARATE = 0, JOIN_DUAL, JOIN_CHAIN };  // branch2c (+ branch1) as launches of their own / the dual-source GEMM / chained with the next branch2a
struct BlockRoute {
    ConvRoute r2a, r2b, r2c, r1;  // r2c: the dual-source launch when join == JOIN_DUAL; r1 only when a conv_block joins separately
    int join;
    bool u1_slab8;  // JOIN_CHAIN: the next block's branch2a output is written channel-slab major
    // the inference walk runs the block's join AND the next block's branch2a as one launch of conv_stream_chain_f32s.hip (bits 4 / 8 of
    // stream1x1, from stream1x1_min_m rows on).  Beside the route, as ConvRoute::stream: join / r2c name what runs without it, and the next
    // block's r2a the GEMM its branch2a takes when launched alone
    bool stream_chain;
    bool stream_u1_slab8;  // ... and writes the next block's branch2a output channel-slab major (u1_slab8 itself stays what it was: JOIN_CHAIN's)
};
struct ResBlock;
bool stream1x1_dual(const HpePlan& pl, bool bf16, const ResBlock& blk);  // the conv_block whose dual-source launch conv_stream_f32s.hip takes (ConvLayer::w_dual_stream of blk.i2c)
ConvRoute route_conv(const HpePlan& pl, bool bf16, int idx, const ConvQuery& q);
BlockRoute route_block(const HpePlan& pl, bool bf16, const ResBlock& blk, ConvQuery q);  // q.residual is ignored: the block says which layer has one
// fp32 tile of a launch outside the table (the data-gradient GEMMs of encoder_train.hip)
int pick_tile(const HpePlan& pl, int M, int N, int K, bool residual_expand = false, bool concurrent = false);
// ... and the bf16 tile of one (the data-gradient GEMMs of the mixed-precision walk): the rule of the bf16 routes, alone on the device
int pick_tile_bf16(const HpePlan& pl, int M, int N, int K, int mode);
