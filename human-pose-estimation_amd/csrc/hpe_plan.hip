// hpe_plan.hip -- the layer table, the option table and its resolver (the one place of the library that reads the environment), and the
// dispatch: which packings a layer holds (layer_packs) and which kernel, tile and layouts a launch takes (route_conv, route_block).  Host
// logic only: no pointer, no HIP call.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "gemm_contract.h"
#include "hpe_ctx.h"

namespace {

struct Network {
    std::vector<ConvSpec> specs;
    std::vector<ResBlock> blocks;
};

// ResNet-50 v1 layer table, Keras names / order [2a, 2b, 2c, (1)] per block, and the block table over it: the
// one loop that numbers the layers also says which of them form a block
Network build_network() {
    Network net;
    std::vector<ConvSpec>& v = net.specs;
    auto add = [&](const std::string& n, const std::string& b, int kh, int cin, int cout, int s, int hin, int hout) {
        ConvSpec c;
        snprintf(c.name, sizeof c.name, "%s", n.c_str());
        snprintf(c.bn, sizeof c.bn, "%s", b.c_str());
        c.kh = c.kw = kh;
        c.cin = cin;
        c.cout = cout;
        c.stride = s;
        c.hin = hin;
        c.hout = hout;
        v.push_back(c);
    };
    add("conv1", "bn_conv1", 7, 3, 64, 2, 224, 112);
    const int nblk[4] = {3, 4, 6, 3};
    const int filt[4][3] = {{64, 64, 256}, {128, 128, 512}, {256, 256, 1024}, {512, 512, 2048}};
    int cin = 64, h = 56;
    int in = -1;  // the layer that feeds the next block: the previous block's branch2c; the max-pooled map for the first
    for (int st = 0; st < 4; ++st) {
        for (int b = 0; b < nblk[st]; ++b) {
            const bool first = b == 0;
            const int s = (first && st > 0) ? 2 : 1;
            const int hout = h / s;
            const int i2a = (int)v.size();
            net.blocks.push_back(ResBlock{st, first, b == nblk[st] - 1, i2a, i2a + 1, i2a + 2, first ? i2a + 3 : -1, in});
            in = i2a + 2;
            char base[24], bn[24];
            snprintf(base, sizeof base, "res%d%c_branch", st + 2, 'a' + b);
            snprintf(bn, sizeof bn, "bn%d%c_branch", st + 2, 'a' + b);
            add(std::string(base) + "2a", std::string(bn) + "2a", 1, cin, filt[st][0], s, h, hout);
            add(std::string(base) + "2b", std::string(bn) + "2b", 3, filt[st][0], filt[st][1], 1, hout, hout);
            add(std::string(base) + "2c", std::string(bn) + "2c", 1, filt[st][1], filt[st][2], 1, hout, hout);
            if (first) add(std::string(base) + "1", std::string(bn) + "1", 1, cin, filt[st][2], s, h, hout);
            cin = filt[st][2];
            h = hout;
        }
    }
    return net;
}

const Network& network() {
    static const Network n = build_network();
    return n;
}

}  // namespace

const std::vector<ConvSpec>& specs() { return network().specs; }
const std::vector<ResBlock>& blocks() { return network().blocks; }

// ---- the option table.  One row per HpePlan member that can be set from outside; precedence as documented in include/hpe.h: the HpeConfig
// field if it is >= 0, else the environment variable, else the built-in default.  dflt / mask are {fp32 encoder, bf16 encoder}; the resolved
// value is ANDed with the mask (-1 keeps every bit, 0 switches the option off for that dtype), then clamped to [lo, hi].
struct PlanOption {
    int HpePlan::*member;
    int HpeConfig::*cfg;  // nullptr: no HpeConfig field
    const char* env;
    int dflt[2];
    int mask[2];
    int lo, hi;
};

constexpr int ANY = -1, NO_LO = INT_MIN, NO_HI = INT_MAX;

const PlanOption kPlanOptions[] = {
    // Two chunk streams by default: with the tail stream of the pipelined forward that makes 3 busy queues per process, and a 4th for RCCL.
    // A 5th concurrently busy queue is expensive on this part whatever GPU_MAX_HW_QUEUES says -- with a process group alive 3 chunk streams
    // cost 6 % in fp32 and 24 % in bf16 (profiles/r02/streams_vs_rccl.txt) -- while 2 and 3 chunk streams are equal without one.
    {&HpePlan::n_streams, &HpeConfig::n_streams, "HPE_STREAMS", {2, 2}, {ANY, ANY}, 1, 4},
    {&HpePlan::dual_gemm, &HpeConfig::dual_gemm, "HPE_DUAL", {1, 1}, {ANY, ANY}, NO_LO, NO_HI},
    {&HpePlan::stem_fused, &HpeConfig::stem_fused, "HPE_STEM_FUSED", {1, 1}, {ANY, ANY}, NO_LO, NO_HI},
    {&HpePlan::wino_min_c, &HpeConfig::wino_min_c, "HPE_WINO_MINC", {128, 128}, {ANY, ANY}, NO_LO, NO_HI},
    {&HpePlan::wino_min_items, &HpeConfig::wino_min_items, "HPE_WINO_MIN_ITEMS", {128, 128}, {ANY, ANY}, NO_LO, NO_HI},
    {&HpePlan::wino_fused, &HpeConfig::wino_fused, "HPE_WINO_FUSED", {1, 1}, {ANY, ANY}, NO_LO, NO_HI},
    {&HpePlan::wino_fused_min_hw, &HpeConfig::wino_fused_min_hw, "HPE_WINO_FUSED_MINHW", {28, 28}, {ANY, ANY}, NO_LO, NO_HI},
    // HPE_MESH_A2B is a word: "grid" (default), "valu", "mfma" (the full searches, for A/B comparisons)
    {&HpePlan::mesh_a2b, &HpeConfig::mesh_a2b, "HPE_MESH_A2B", {0, 0}, {ANY, ANY}, NO_LO, NO_HI},
    // F(4x4,3x3) on the 28x28 / 14x14 / 7x7 maps by default (A/B on one box: 17,720 -> 18,790 img/s; with the 7x7 and 14x14 maps only
    // 18,540; the 56x56 maps lose: their V round trip costs more than the direct kernel's extra multiplies)
    {&HpePlan::wino_f4, &HpeConfig::wino_f4, "HPE_WINO_F4", {7, 7}, {ANY, ANY}, NO_LO, NO_HI},
    {&HpePlan::wino4_fused, &HpeConfig::wino4_fused, "HPE_WINO4_FUSED", {0, 0}, {12, 12}, NO_LO, NO_HI},
    {&HpePlan::bf16_p8, &HpeConfig::bf16_p8, "HPE_BF16_P8", {0, 0}, {ANY, ANY}, NO_LO, NO_HI},
    {&HpePlan::wino4_ksplit, &HpeConfig::wino4_ksplit, "HPE_WINO4_KSPLIT", {1, 1}, {ANY, ANY}, NO_LO, NO_HI},
    {&HpePlan::chain_fuse, &HpeConfig::chain_fuse, "HPE_CHAIN", {8, 7}, {8, 23}, NO_LO, NO_HI},
    {&HpePlan::halo3, &HpeConfig::halo3, "HPE_HALO3", {15, 15}, {0, 15}, NO_LO, NO_HI},
    {&HpePlan::f32_split, &HpeConfig::f32_split, "HPE_F32_SPLIT", {14, 14}, {15, 0}, NO_LO, NO_HI},
    {&HpePlan::chunk_images, nullptr, "HPE_CHUNK", {0, 0}, {ANY, ANY}, NO_LO, NO_HI},
    // bf16 launches are short enough to leave CUs idle at small batches: two chunks pay from 2 x 24 images on (B = 48 / 64 / 80:
    // 38.5 / 44.8 / 48.9 k img/s against 34.7 / 39.2 / 44.5 k as one chunk); fp32 from 2 x 32 (see encoder_impl).  Values below 8 are ignored.
    {&HpePlan::min_chunk, nullptr, "HPE_MIN_CHUNK", {32, 24}, {ANY, ANY}, NO_LO, NO_HI},
    {&HpePlan::halo3_two, nullptr, "HPE_HALO3_TWO", {4, 4}, {7, 7}, NO_LO, NO_HI},
    {&HpePlan::f32s_min_tiles, nullptr, "HPE_F32S_MIN_TILES", {128, 128}, {ANY, ANY}, NO_LO, NO_HI},
    // conv_stream_f32s.hip: form mask (1: the K <= 128 identity-block expand layers; 2: the dual-source launch of res2a; 4 / 8: the chained
    // forms of conv_stream_chain_f32s.hip, res2b -> res2c and res2a -> res2b), fp32 only; the smallest launch it takes; a cap on its grid
    // (the walk tests)
    {&HpePlan::stream1x1, nullptr, "HPE_STREAM1X1", {15, 0}, {15, 0}, 0, 15},
    {&HpePlan::stream1x1_min_m, nullptr, "HPE_STREAM1X1_MIN_M", {25088, 25088}, {ANY, ANY}, 1, NO_HI},
    {&HpePlan::stream1x1_walkers, nullptr, "HPE_STREAM1X1_WALKERS", {0, 0}, {ANY, ANY}, 0, NO_HI},
    // persistent stream-K scheduling of the Winograd GEMM: opt-in.  It removes the partial last round of workgroups (-7 % on a res4 layer,
    // -2 % on the step with HPE_STREAMS=1) but with the default batch-chunk streams, whose kernels already fill those idle CUs, the step
    // time is unchanged within noise (profiles/r01/g_wino_streamk.txt)
    {&HpePlan::wino_streamk, nullptr, "HPE_WINO_STREAMK", {0, 0}, {ANY, ANY}, NO_LO, NO_HI},
    {&HpePlan::concurrent_tiles, nullptr, "HPE_CONCURRENT_TILES", {0, 0}, {ANY, ANY}, NO_LO, NO_HI},
    {&HpePlan::bf16_w8_min_tiles, nullptr, "HPE_BF16_W8_MIN_TILES", {128, 128}, {ANY, ANY}, NO_LO, NO_HI},
    {&HpePlan::wide128_min_tiles, nullptr, "HPE_WIDE128_MIN_TILES", {384, 384}, {ANY, ANY}, NO_LO, NO_HI},
    {&HpePlan::force_wide, nullptr, "HPE_TILE_WIDE", {-1, -1}, {ANY, ANY}, NO_LO, NO_HI},
    // slabs per split-K slice: a slice shorter than 4 is all launch ramp.  Every split layer pays a second, dependent launch (the fix-up),
    // which costs a single frame about what 6-8 more slabs in the main loop cost.
    {&HpePlan::splitk_min_slabs, nullptr, "HPE_SPLITK_SLABS", {4, 4}, {ANY, ANY}, 2, NO_HI},
    {&HpePlan::wino4_min_items, nullptr, "HPE_WINO4_MIN_ITEMS", {64, 64}, {ANY, ANY}, NO_LO, NO_HI},
    // from 256 workgroups = one per CU on, the 64-cout F(4x4) GEMM is the faster one (profiles/r03/w4_n32_ab.txt)
    {&HpePlan::wino4_n32, nullptr, "HPE_WINO4_N32", {256, 256}, {ANY, ANY}, NO_LO, NO_HI},
    {&HpePlan::w4_abl, nullptr, "HPE_W4_ABL", {0, 0}, {ANY, ANY}, NO_LO, NO_HI},
};

HpePlan hpe_resolve_plan(const HpeConfig& cfg) {
    const int dt = cfg.encoder_dtype == 1 ? 1 : 0;
    HpePlan pl;
    for (const PlanOption& o : kPlanOptions) {
        int v = o.dflt[dt];
        const char* e = getenv(o.env);
        if (o.cfg && cfg.*o.cfg >= 0) v = cfg.*o.cfg;
        else if (e && o.member == &HpePlan::mesh_a2b) v = e[0] == 'v' ? 1 : (e[0] == 'm' ? 2 : 0);
        else if (e) v = atoi(e);
        v &= o.mask[dt];
        pl.*o.member = v < o.lo ? o.lo : (v > o.hi ? o.hi : v);
    }
    if (pl.min_chunk < 8) pl.min_chunk = dt ? 24 : 32;
    // wino_min_c == 0 disables every Winograd path
    pl.wino_fused = pl.wino_fused && pl.wino_min_c > 0;
    if (pl.wino_min_c <= 0) pl.wino_f4 = pl.wino4_fused = 0;
    return pl;
}

// tile of conv_gemm_f32s.hip for this launch, -1 = the launch keeps the fp32 kernel.  Split weights are packed (fp32 encoder, stage in f32_split),
// N > 64, the grid is whole tiles of a useful size.  Measured at B = 256 (profiles/r05): the 4-wave 128 x 128 tile (each A element
// split by one wave) everywhere but on the identity-block expand layers, which are mostly epilogue: there 8 waves (128 x 128, 4 x 2), and on
// stage 3 (K = 128) the fp32 kernel's 128 x 64 8-wave tile stays ahead.
static int pick_f32s(const HpePlan& pl, bool split_packed, int M, int N, int K, bool residual_expand) {
    if (!split_packed || N <= 64) return -1;
    if (residual_expand && K < PLAN_F32S_EXPAND_MIN_K) return -1;
    const int tile = residual_expand ? PLAN_F32S_EXPAND_TILE : PLAN_F32S_TILE;
    const TileShape ts = tile_shape(GEMM_K_F32S, tile);
    return (long)((M + ts.bm - 1) / ts.bm) * ((N + ts.bn - 1) / ts.bn) >= pl.f32s_min_tiles ? tile : -1;
}

int pick_tile(const HpePlan& pl, int M, int N, int K, bool residual_expand, bool concurrent) {
    // prefer the largest tile that still gives >= 2 workgroups per CU; N == 64 layers use 64-wide tiles
    const bool wide = N > 64;
    // identity-block expand layers: 8 waves (see below) -- unless the grid is so small that the launch is DMA latency: then the 4-wave
    // 64x64 tile, which the launcher cuts along K (single frames: res5*_branch2c 21 -> 9 us)
    if (wide && residual_expand) return (long)((M + 127) / 128) * ((N + 63) / 64) < PLAN_EXPAND_SMALL_GRID ? TILE_64x64 : TILE_128x64_W8;
    if (wide && pl.force_wide >= 0) return pl.force_wide;
    // Measured on MI355X (profiles/r01/d_tile_sweep.txt): with LDS-DMA staging the small tiles with 3-5 workgroups
    // per CU beat 128x128 at 2 per CU except on the huge-M layers of stages 2-3.
    if (!wide) return TILE_128x64;
    // Identity-block expand layers (above) and K <= 128 on the huge-M maps (the C -> 4C expand / projection layers of stages 2 and
    // 3): the launch is mostly epilogue -> 8 waves to issue the row stores and residual loads win; 128x64 beats 128x128
    // (profiles/r01/h_tile_128x64w8.txt: res2*_branch2c 0.41-0.43 -> 0.37-0.38 ms, res3*_branch2c 0.31 -> 0.28 ms; stages 4-5:
    // equal to the 64x64 tile within 1 %, profiles/r02/fp32_expand_tile.txt)
    if (K <= 128 && M >= 150000) return PLAN_SHORTK_TILE;
    // Launches of concurrent batch chunks: 128x128 wherever it still leaves >= 1.5 tiles per CU (round 2, pipelined steps + two chunk
    // streams at B = 256: 17,440 -> 17,830 img/s, B = 128: +0.7 %, although most of these layers are 5-10 % SLOWER with it when they
    // run alone -- fewer, longer workgroups leave the co-running chunk's kernels more room).  A single-chunk batch keeps the
    // round-1 rule (B = 64: -0.6 ... -1.2 % with 128x128).  Thresholds 300 / 390 / 700 tiles: 17,805 / 17,843 / 17,806 img/s.
    if ((concurrent || pl.concurrent_tiles) && pl.wide128_min_tiles > 0 && (long)((M + 127) / 128) * ((N + 127) / 128) >= pl.wide128_min_tiles) return TILE_128x128;
    if (M >= 150000) return TILE_64x128;
    return TILE_64x64;
}

// bf16 tile per layer kind, from the per-layer sweeps in profiles/r02 (B = 256):
//  * identity-block expand layers (1x1, K = C, N = 4C, + residual): all epilogue -> 128x64 with 8 waves issuing the row stores
//    and residual loads (res2b_branch2c 0.273 -> 0.182 ms = 5.1 TB/s, res3* 0.157 -> 0.108, res4* 0.079 -> 0.062, res5* 0.061 -> 0.048)
//  * everything with a long k axis on the small maps (stage 5: M = 49 B): 256x128, 8 waves (res5*_branch2b 0.112 -> 0.083 ms)
//  * otherwise 128x128 while that still gives >= 512 workgroups, else 64x128
// (the LDS ring is two slabs deep everywhere: a 3-deep ring lost on every layer it was measured on)
static int pick_bf16(const HpePlan& pl, int M, int N, int K, bool residual_expand, bool concurrent, int mode) {
    // 256 x 256 phase-interleaved kernel (conv_gemm_bf16_p8.hip), per layer kind -- bits of bf16_p8:
    //   1: 3x3 layers with N == 256 (stage 4), 2: 3x3 layers with N >= 512 (stage 5), 4: 1x1 / strided layers,
    //   8: dual-source launches with N >= 2048 (res5a), 16: the other dual-source launches
    if (pl.bf16_p8 && N >= PLAN_BF16_P8_MIN_N && N % 256 == 0 && K >= PLAN_BF16_P8_MIN_K && !residual_expand) {
        const int bit = mode == GEMM_CONV3 ? (N == 256 ? 1 : 2) : (mode == GEMM_DUAL ? (N >= 2048 ? 8 : 16) : 4);
        if (pl.bf16_p8 & bit) return TILE_P8_256x256;
    }
    if (N <= 64) return TILE_128x64;
    const long t128 = (long)((M + 127) / 128) * ((N + 127) / 128);
    int tile = t128 >= ((concurrent || pl.concurrent_tiles) ? PLAN_BF16_128_MIN_TILES : 512) ? TILE_128x128 : TILE_64x128;
    if (residual_expand) tile = TILE_128x64_W8;
    else if (M <= 16384 && M >= 8192 && K >= 1024 && N >= 256) tile = TILE_256x128_W8;
    // Round 4: these launches are paced by the ISSUE of their LDS-DMA instructions (60-180 cycles each for the issuing wave),
    // not by the matrix pipe (without any multiplies the 1x1 layers take 0.96-0.99 of their time; a deeper ring is slower):
    // the 128 x 128 tile with EIGHT waves halves the DMA instructions per wave and slab.  Every N > 64 layer of the B = 256
    // step is equal or faster with it (serial pass 3.59 -> 3.50 ms, step 75.1 -> 76.7 k img/s); small grids keep the old rules.
    if (pl.bf16_w8_min_tiles > 0 && t128 >= pl.bf16_w8_min_tiles) tile = TILE_128x128_W8;
    return tile;
}

int pick_tile_bf16(const HpePlan& pl, int M, int N, int K, int mode) { return pick_bf16(pl, M, N, K, false, false, mode); }

// ---- the dispatch.  layer_packs() is the rule hpe_finalize packs by and the routes ask; the order of the tests in route_conv() is the
// precedence of the kernels.
unsigned layer_packs(const HpePlan& pl, bool bf16, int idx) {
    const ConvSpec& s = specs()[idx];
    // fused stem: the conv1 weights in the k enumeration of stem_fused.hip
    unsigned m = idx == 0 ? PACK_STEM_W : 0;
    // conv_block: branch2c + branch1 as one GEMM over the concatenated k axis, both k axes whole slabs (32 floats / 64 bf16)
    const int slab = bf16 ? 64 : 32;
    const ResBlock* blk = nullptr;
    for (const ResBlock& b : blocks())
        if (b.first && b.i2c == idx) blk = &b;
    if (pl.dual_gemm && blk && s.cin % slab == 0 && specs()[blk->i1].cin % slab == 0) {
        m |= PACK_W_DUAL;
        // f32_split: the folded weight is split (the BN scales are inside the pieces)
        if (!bf16 && (pl.f32_split & stage_bit(s.hout))) m |= PACK_W_DUAL_SPLIT;
    }
    if (bf16) return m;
    if (idx != 0 && s.kh == 1 && (pl.f32_split & stage_bit(s.hout))) m |= PACK_W_SPLIT;
    const bool wino = s.kh == 3 && s.stride == 1 && s.cin % 32 == 0 && s.cout % 64 == 0;
    if (wino && pl.wino_min_c > 0 && (s.cin >= pl.wino_min_c || (pl.wino_fused && s.hin >= pl.wino_fused_min_hw))) m |= PACK_WINO_U;
    if (wino && ((pl.wino_f4 | pl.wino4_fused) & f4_bit(s.hin))) m |= PACK_WINO4_U;
    return m;
}

// the identity-block expand layers with K <= 128 that run as launches of their own (stage 2: the last block, the others are chained; stage 3:
// all three): conv_stream_f32s.hip takes them from stream1x1_min_m rows on.  Part of the split-bf16 family: f32_split = 0 keeps the fp32-MFMA plan
static bool use_chain(const HpePlan& pl, bool bf16, const ResBlock& blk);
bool stream1x1_layer(const HpePlan& pl, bool bf16, int idx) {
    if (bf16 || !(pl.stream1x1 & 1) || !pl.f32_split) return false;
    const ConvSpec& s = specs()[idx];
    for (const ResBlock& b : blocks())
        if (b.i2c == idx && !b.first && !use_chain(pl, bf16, b))
            return s.kh == 1 && s.stride == 1 && s.cout == 4 * s.cin && hpe_stream_f32s_supported(1, s.cout, conv_k_pad(idx, bf16));
    return false;
}

// the conv_block whose dual-source launch conv_stream_f32s.hip takes (form 2): two sources of 64 channels on one map -- res2a
bool stream1x1_dual(const HpePlan& pl, bool bf16, const ResBlock& blk) {
    if (bf16 || !(pl.stream1x1 & 2) || !pl.f32_split || !blk.first || use_chain(pl, bf16, blk) || !(layer_packs(pl, bf16, blk.i2c) & PACK_W_DUAL)) return false;
    const ConvSpec& s2 = specs()[blk.i2c];
    const ConvSpec& s1 = specs()[blk.i1];
    return hpe_stream_f32s_dual_supported(1, s2.cout, s2.cin, s1.cin, s1.stride, s1.hin, s1.hout);
}

// steps 6-8 of route_conv, and the dual-source launch: the implicit-GEMM kernel and tile of an M x N x K launch; stream_layer: the launch is
// one of stream1x1_layer's (then step 5a: conv_stream_f32s.hip from stream1x1_min_m rows on, noted beside the GEMM route)
static ConvRoute route_gemm(const HpePlan& pl, bool bf16, int mode, int M, int N, int K, bool expand, bool split_packed, bool concurrent,
                            bool stream_layer = false) {
    ConvRoute r{CONV_K_F32, mode, -1, false, false, concurrent, stream_layer && expand && M >= pl.stream1x1_min_m};
    if (bf16) {  // 6. bf16 / bf16_p8
        r.tile = pick_bf16(pl, M, N, K, expand, concurrent, mode);
        r.kernel = r.tile == TILE_P8_256x256 ? CONV_K_BF16_P8 : CONV_K_BF16;
    } else if ((r.tile = pick_f32s(pl, split_packed, M, N, K, expand)) >= 0) {  // 7. f32s
        r.kernel = CONV_K_F32S;
    } else {  // 8. fp32
        r.tile = pick_tile(pl, M, N, K, expand, concurrent);
    }
    return r;
}

ConvRoute route_conv(const HpePlan& pl, bool bf16, int idx, const ConvQuery& q) {
    const ConvSpec& s = specs()[idx];
    const unsigned packs = layer_packs(pl, bf16, idx);
    const int B = q.B, H = s.hin;
    const int mode = idx == 0 ? GEMM_STEM : s.kh == 3 ? GEMM_CONV3 : s.stride == 1 ? GEMM_DENSE : GEMM_STRIDED;
    // every kernel but the implicit GEMMs is a plain 3x3 / stride 1 convolution: no residual operand
    const bool plain3 = mode == GEMM_CONV3 && s.stride == 1 && !q.residual;
    auto special = [&](int kernel) { return ConvRoute{kernel, mode, -1, kernel == CONV_K_WINO_FUSED || kernel == CONV_K_WINO4_FUSED, false, q.concurrent}; };
    const int min4 = pl.wino_min_items < pl.wino4_min_items ? pl.wino_min_items : pl.wino4_min_items;
    // 1. F(4x4) with the input transform inside the GEMM kernel (its 1x1 producer then writes channel-slab major); before F(4x4)
    if (plain3 && (packs & PACK_WINO4_U) && (pl.wino4_fused & f4_bit(H)) && hpe_wino4_fused_items(B, H, H, s.cout) >= min4) return special(CONV_K_WINO4_FUSED);
    // the layer runs as F(4x4,3x3) for this batch (blocked V through the workspace) -- where it would, F(2x2) fused stands back even in a
    // chunk that has no workspace slice
    const bool f4 = plain3 && (packs & PACK_WINO4_U) && (pl.wino_f4 & f4_bit(H)) && hpe_wino4_items(B, H, H, s.cout) >= min4;
    // 2. the fused F(2x2) kernel (its 1x1 producer then writes channel-slab major)
    if (plain3 && !f4 && pl.wino_fused && (packs & PACK_WINO_U) && H >= pl.wino_fused_min_hw && hpe_wino_fused_items(B, H, H, s.cout) >= pl.wino_min_items)
        return special(CONV_K_WINO_FUSED);
    // 3. F(4x4)
    if (f4 && q.workspace) return special(CONV_K_WINO4);
    // 4. F(2x2).  Winograd needs enough (64-tile x 64-cout) work items to occupy the 256 CUs (one 8-wave workgroup each); below that
    // the direct kernel with split-K is faster (measured crossover: batch ~32, profiles/r01/g_wino_small_batch.txt)
    if (plain3 && (packs & PACK_WINO_U) && q.workspace && s.cin >= pl.wino_min_c &&
        (long)((B * ((H + 1) / 2) * ((H + 1) / 2) + 63) / 64) * (s.cout / 64) >= pl.wino_min_items)
        return special(CONV_K_WINO);
    // 5. halo3 (bf16): before bf16_p8, whose bits 1-2 name the same 3x3 layers -- clear halo3 to reach them
    if (bf16 && plain3 && (pl.halo3 & f4_bit(H)) && hpe_halo3_bf16_supported(H, s.cin, s.cout)) return special(CONV_K_HALO3);
    // 6.-8. the implicit GEMMs; expand: an identity block's C -> 4C layer with its residual
    return route_gemm(pl, bf16, mode, B * s.hout * s.hout, s.cout, conv_k_pad(idx, bf16), mode == GEMM_DENSE && q.residual && s.cout == 4 * s.cin,
                      (packs & PACK_W_SPLIT) != 0, q.concurrent, stream1x1_layer(pl, bf16, idx));
}

// the pair branch2c (+ residual + ReLU) -> next block's branch2a as one launch.  The last block of a stage has no partner.
static bool use_chain(const HpePlan& pl, bool bf16, const ResBlock& blk) {
    if (blk.last) return false;
    const int stg = blk.stage, i2c = blk.i2c;
    const ConvSpec& s2 = specs()[i2c];
    const ConvSpec& sn = specs()[i2c + (blk.first ? 2 : 1)];  // the next block's branch2a
    if (sn.kh != 1 || sn.stride != 1 || sn.cin != s2.cout) return false;
    // fp32: identity blocks of stage 2 only (conv_chain_f32.hip; bit 3 of chain_fuse, on by default: A/B on two boxes +0.3 ... +1.4 % at
    // B = 256, +1.6 % at B = 64)
    if (!bf16) return !blk.first && stg == 0 && (pl.chain_fuse & 8) && hpe_chain_f32_supported(s2.cin, s2.cout, sn.cout);
    // blk.first: the conv_block form -- branch2c + the projection shortcut branch1 (stride 1: stage 2 only) as the dual-source GEMM, chained
    // with the next block's branch2a; bit 2 of chain_fuse
    if (blk.first) {
        const ConvSpec& s1 = specs()[blk.i1];
        return stg == 0 && (pl.chain_fuse & 4) && (layer_packs(pl, bf16, i2c) & PACK_W_DUAL) && s1.stride == 1 && s1.hin == s2.hin &&
               hpe_chain_bf16_supported(s2.cin, s2.cout, sn.cout, s1.cin);
    }
    // identity blocks: bit 0 = stage 2, bit 1 = stage 3, bit 4 (value 16) = stage 4 (128-pixel workgroups, one per CU)
    const int bit = stg == 0 ? 1 : stg == 1 ? 2 : stg == 2 ? 16 : 0;
    return (pl.chain_fuse & bit) && hpe_chain_bf16_supported(s2.cin, s2.cout, sn.cout, 0);
}

// the chained streaming launch of a stage-2 block and the next block's branch2a: form 3 (bit 4) where the plan chains the pair anyway (res2b),
// form 4 (bit 8) on the dual-source conv_block (res2a).  Part of the split-bf16 family, as stream1x1_layer
static bool stream_chain(const HpePlan& pl, bool bf16, const ResBlock& blk, int join, int M) {
    if (bf16 || !pl.f32_split || blk.last || M < pl.stream1x1_min_m) return false;
    if (!(pl.stream1x1 & (join == JOIN_CHAIN ? 4 : join == JOIN_DUAL ? 8 : 0))) return false;
    const ConvSpec& s2 = specs()[blk.i2c];
    const ConvSpec& sn = specs()[blk.i2c + (blk.first ? 2 : 1)];  // the next block's branch2a
    if (sn.kh != 1 || sn.stride != 1 || sn.cin != s2.cout || s2.hout != s2.hin) return false;
    if (blk.first && (specs()[blk.i1].stride != 1 || specs()[blk.i1].hin != s2.hin)) return false;
    return hpe_stream_chain_f32s_supported(M, s2.cin, s2.cout, sn.cout, blk.first ? specs()[blk.i1].cin : 0);
}

BlockRoute route_block(const HpePlan& pl, bool bf16, const ResBlock& blk, ConvQuery q) {
    BlockRoute b{};
    q.residual = false;
    b.r2a = route_conv(pl, bf16, blk.i2a, q);
    b.r2b = route_conv(pl, bf16, blk.i2b, q);
    b.r2a.out_slab8 = b.r2b.in_slab8;  // then branch2a's output never leaves this pair of launches
    const ConvSpec& s2 = specs()[blk.i2c];
    if (use_chain(pl, bf16, blk)) {
        b.join = JOIN_CHAIN;
        // (fp32: the next block's 3x3 layer may be a fused Winograd kernel, which reads its input channel-slab major)
        b.u1_slab8 = route_conv(pl, bf16, blk.i2c + (blk.first ? 3 : 2), q).in_slab8;
    } else if (blk.first && (layer_packs(pl, bf16, blk.i2c) & PACK_W_DUAL)) {
        b.join = JOIN_DUAL;
        b.r2c = route_gemm(pl, bf16, GEMM_DUAL, q.B * s2.hout * s2.hout, s2.cout, s2.cin + specs()[blk.i1].cin, false,
                           (layer_packs(pl, bf16, blk.i2c) & PACK_W_DUAL_SPLIT) != 0, q.concurrent);
        b.r2c.stream = stream1x1_dual(pl, bf16, blk) && q.B * s2.hout * s2.hout >= pl.stream1x1_min_m;
    } else {
        if (blk.first) b.r1 = route_conv(pl, bf16, blk.i1, q);
        q.residual = true;
        b.r2c = route_conv(pl, bf16, blk.i2c, q);
    }
    b.stream_chain = stream_chain(pl, bf16, blk, b.join, q.B * s2.hout * s2.hout);
    if (b.stream_chain) b.stream_u1_slab8 = route_conv(pl, bf16, blk.i2c + (blk.first ? 3 : 2), q).in_slab8;
    return b;
}
