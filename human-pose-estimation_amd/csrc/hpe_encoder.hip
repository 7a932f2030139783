// hpe_encoder.hip -- the launch sequences: one conv layer / dual-source block / chained pair through the kernel its route names, the
// encoder over batch chunks, the regressor steps and the forward tail.  Host logic only.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "hpe_ctx.h"

// the implicit GEMM a route names, p filled but for the workspace; w_split: the three-bf16-piece form of p.w (rows of p.ldw elements)
static hipError_t launch_gemm(hpe_ctx* c, GemmArgs& p, const ConvRoute& r, const void* w_split, hipStream_t st) {
    // The ctx has ONE split-K workspace: only a launch that is alone on the device may use it.  Batch chunks running on
    // concurrent streams never split K, whatever their size (their grids overlap each other instead).
    if (!r.concurrent) p.partial = c->partial, p.partial_floats = c->partial_floats;
    if (r.kernel == CONV_K_BF16 || r.kernel == CONV_K_BF16_P8) return hpe_launch_gemm_bf16(p, r.mode, r.tile, st);
    if (r.kernel != CONV_K_F32S) return hpe_launch_gemm(p, r.mode, r.tile, c->plan.splitk_min_slabs, st);
    if (!w_split) return hipErrorInvalidValue;
    p.w = static_cast<const float*>(w_split);
    p.w_piece = p.ldw;
    p.ldw *= 3;
    return hpe_launch_gemm_f32s(p, r.mode, r.tile, st);
}

// one conv layer (+BN fold, +residual, +ReLU) through the kernel of its route (hpe_plan.hip).  A route whose packing or workspace this
// context does not hold, or a residual on a kernel that takes none, is refused: nothing is launched
hipError_t run_conv(hpe_ctx* c, int idx, const ConvRoute& r, const float* x, int B, const float* res, int relu, float* y, hipStream_t st,
                    float* wino_v, int slot, const float* scale, const float* shift) {
    const ConvSpec& s = specs()[idx];
    const ConvLayer& L = c->conv[idx];
    if (!scale) scale = L.scale;
    if (!shift) shift = L.shift;
    const int H = s.hin;
    const bool f2 = r.kernel == CONV_K_WINO || r.kernel == CONV_K_WINO_FUSED, f4 = r.kernel == CONV_K_WINO4 || r.kernel == CONV_K_WINO4_FUSED;
    if ((r.kernel >= CONV_K_HALO3 && res) || (f2 && !L.wino_u) || (f4 && !L.wino4_u) || ((f2 || f4) && !r.in_slab8 && !wino_v)) return hipErrorInvalidValue;
    switch (r.kernel) {
        case CONV_K_WINO4_FUSED: return hpe_launch_wino4_fused_conv3(x, L.wino4_u, scale, shift, c->zeros, y, s.cout, B, H, H, s.cin, s.cout, relu, st);
        case CONV_K_WINO_FUSED: return hpe_launch_wino_fused_conv3(x, L.wino_u_split, scale, shift, c->zeros, y, s.cout, B, H, H, s.cin, s.cout, relu, st);
        case CONV_K_WINO4:
            return hpe_launch_wino4_conv3(x, s.cin, L.wino4_u, scale, shift, y, s.cout, B, H, H, s.cin, s.cout, relu, wino_v, st, r.concurrent ? c->co_running : 1,
                                          c->w4_split && slot >= 0 && slot < 4 ? c->w4_split + (size_t)slot * hpe_wino4_split_ws_floats() : nullptr, c->plan.wino4_n32,
                                          c->plan.w4_abl);
        case CONV_K_WINO: {
            WinoStreamK sk{};
            if (c->wino_ws && slot >= 0 && slot < 4) {
                sk.ws = c->wino_ws + (size_t)slot * c->n_cu * HPE_WINO_WS_FLOATS;
                sk.flags = c->wino_flags + (size_t)slot * c->n_cu;
                sk.epoch = ++c->wino_epoch;
                if (sk.epoch == 0) sk.epoch = ++c->wino_epoch;
                sk.n_wg = c->n_cu;
                sk.err = c->dev_err;
            }
            return hpe_launch_wino_conv3(x, s.cin, L.wino_u, scale, shift, y, s.cout, B, H, H, s.cin, s.cout, relu, wino_v, c->wino_ws ? &sk : nullptr, st);
        }
        case CONV_K_HALO3: {
            Halo3Args h{};
            h.x = reinterpret_cast<const __bf16*>(x), h.w = reinterpret_cast<const __bf16*>(L.w), h.y = reinterpret_cast<__bf16*>(y);
            h.scale = scale, h.shift = shift;
            h.M = B * s.hout * s.hout, h.N = s.cout, h.ldw = L.k_pad;
            h.relu = relu, h.two = c->plan.halo3_two;
            return hpe_launch_halo3_bf16(h, H, s.cin, st);
        }
    }
    GemmArgs p{};
    p.x = x, p.w = L.w, p.scale = scale, p.shift = shift, p.res = res, p.y = y, p.zero = c->zeros;
    p.M = B * s.hout * s.hout, p.N = s.cout, p.K = L.k_pad;
    p.lda = s.cin, p.ldw = L.k_pad, p.w_rows = L.n_pad, p.ldy = p.ldres = s.cout;
    p.Hi = p.Wi = H, p.Cin = s.cin, p.Ho = p.Wo = s.hout, p.stride = s.stride;
    p.cin_slabs = s.cin / (c->bf16 ? 64 : 32);
    p.relu = relu, p.y_slab8 = r.out_slab8 ? 1 : 0;
    if (r.mode == GEMM_STEM) p.Hi = STEM_HP, p.Wi = STEM_WP, p.Cin = 4;
    if (r.stream) {  // conv_stream_f32s.hip: a missing weight image is an error, not a reason for another kernel
        if (!L.w_stream || !res) return hipErrorInvalidValue;
        p.w = reinterpret_cast<const float*>(L.w_stream);
        p.w_piece = p.ldw;
        p.ldw *= 3;
        return hpe_launch_stream_f32s(p, GEMM_DENSE, c->plan.stream1x1_walkers, st);
    }
    return launch_gemm(c, p, r, L.w_split, st);
}

hipError_t run_conv_nhwc(hpe_ctx* c, int idx, const float* x, int B, const float* res, int relu, float* y, hipStream_t st, const float* scale,
                         const float* shift) {
    const ConvRoute r = route_conv(c->plan, c->bf16, idx, ConvQuery{B, false, res != nullptr, c->wino_v != nullptr});
    if (r.in_slab8) {
        // the fused Winograd kernels read channel-slab major input; in the network their 1x1 producer writes that directly
        const ConvSpec& s = specs()[idx];
        HIPE(hpe_launch_nhwc_to_slab8(x, c->T1, (long)B * s.hin * s.hin, s.cin, st));
        x = c->T1;
    }
    return run_conv(c, idx, r, x, B, res, relu, y, st, c->wino_v, 0, scale, shift);
}

// branch2c (+BN) + branch1 (+BN) + add + ReLU of a conv_block as one dual-source GEMM: t2 [M, K1] dense, x NHWC strided
hipError_t run_dual(hpe_ctx* c, int i2c, int i1, const ConvRoute& r, const float* t2, const float* x, int B, float* y, hipStream_t st) {
    const ConvSpec& s2 = specs()[i2c];
    const ConvSpec& s1 = specs()[i1];
    const ConvLayer& L = c->conv[i2c];
    GemmArgs p{};
    p.x = t2, p.x2 = x, p.w = L.w_dual, p.scale = c->ones, p.shift = L.shift_dual, p.y = y, p.zero = c->zeros;
    p.M = B * s2.hout * s2.hout, p.N = s2.cout, p.K = L.k_dual;
    p.k1_slabs = L.k1_dual / (c->bf16 ? 64 : 32), p.relu = 1;
    p.lda = s2.cin, p.ldw = L.k_dual, p.w_rows = round_up(s2.cout, 128), p.ldy = s2.cout;
    p.Hi = p.Wi = s1.hin, p.Cin = s1.cin, p.Ho = p.Wo = s1.hout, p.stride = s1.stride;
    if (r.stream) {  // conv_stream_f32s.hip, the dual-source form
        if (!L.w_dual_stream) return hipErrorInvalidValue;
        p.w = reinterpret_cast<const float*>(L.w_dual_stream);
        p.w_piece = p.ldw;
        p.ldw *= 3;
        return hpe_launch_stream_f32s(p, GEMM_DUAL, c->plan.stream1x1_walkers, st);
    }
    return launch_gemm(c, p, r, L.w_dual_split, st);
}

// res: the block input -- the residual of an identity block, the second A source of a conv_block
hipError_t run_chain(hpe_ctx* c, int i2c, bool first, const float* t2, const float* res, int B, float* t3, float* u1, hipStream_t st,
                     bool u1_slab8) {
    const ConvSpec& s2 = specs()[i2c];
    const int inext = i2c + (first ? 2 : 1);
    const ConvSpec& sn = specs()[inext];
    const ConvLayer& L2 = c->conv[i2c];
    const ConvLayer& Ln = c->conv[inext];
    if (!c->bf16) {
        ChainArgsF32 q{};
        q.t2 = t2;
        q.res = res;
        q.w2c = L2.w;
        q.w2a = Ln.w;
        q.scaleA = L2.scale;
        q.shiftA = L2.shift;
        q.scaleB = Ln.scale;
        q.shiftB = Ln.shift;
        q.t3 = t3;
        q.u1 = u1;
        q.M = B * s2.hout * s2.hout;
        q.ldw2c = L2.k_pad;
        q.ldw2a = Ln.k_pad;
        q.u1_slab8 = u1_slab8 ? 1 : 0;
        return hpe_launch_chain_f32(q, s2.cin, s2.cout, sn.cout, st);
    }
    ChainArgs p{};
    p.t2 = reinterpret_cast<const __bf16*>(t2);
    if (first) {
        p.x2 = reinterpret_cast<const __bf16*>(res);
        p.w2c = reinterpret_cast<const __bf16*>(L2.w_dual);
        p.scaleA = c->ones;
        p.shiftA = L2.shift_dual;
        p.ldw2c = L2.k_dual;
    } else {
        p.res = reinterpret_cast<const __bf16*>(res);
        p.w2c = reinterpret_cast<const __bf16*>(L2.w);
        p.scaleA = L2.scale;
        p.shiftA = L2.shift;
        p.ldw2c = L2.k_pad;
    }
    p.w2a = reinterpret_cast<const __bf16*>(Ln.w);
    p.scaleB = Ln.scale;
    p.shiftB = Ln.shift;
    p.t3 = reinterpret_cast<__bf16*>(t3);
    p.u1 = reinterpret_cast<__bf16*>(u1);
    p.M = B * s2.hout * s2.hout;
    p.ldw2a = Ln.k_pad;
    return hpe_launch_chain_bf16(p, s2.cin, s2.cout, sn.cout, first ? specs()[i2c + 1].cin : 0, st);
}

// the chained streaming launch (BlockRoute::stream_chain): x is the block input -- the residual of an identity block, the second A source of a
// conv_block.  The kernel reads the fp32 weights of both layers; a conv_block without its folded dual weights is an error
hipError_t run_stream_chain(hpe_ctx* c, int i2c, bool first, const float* t2, const float* x, int B, float* t3, float* u1, hipStream_t st,
                            bool u1_slab8, int rows) {
    const ConvSpec& s2 = specs()[i2c];
    const int inext = i2c + (first ? 2 : 1);
    const ConvSpec& sn = specs()[inext];
    const ConvLayer& L2 = c->conv[i2c];
    const ConvLayer& Ln = c->conv[inext];
    if (c->bf16 || (first && (!L2.w_dual || !L2.shift_dual))) return hipErrorInvalidValue;
    StreamChainArgs q{};
    q.t2 = t2, q.x = x, q.t3 = t3, q.u1 = u1;
    q.wA = first ? L2.w_dual : L2.w, q.ldwA = first ? L2.k_dual : L2.k_pad;
    q.scaleA = first ? c->ones : L2.scale, q.shiftA = first ? L2.shift_dual : L2.shift;
    q.wB = Ln.w, q.ldwB = Ln.k_pad, q.scaleB = Ln.scale, q.shiftB = Ln.shift;
    q.M = rows ? rows : B * s2.hout * s2.hout;  // (rows: hpe_debug_stream_chain's, the first rows of the batch)
    q.u1_slab8 = u1_slab8 ? 1 : 0;
    return hpe_launch_stream_chain_f32s(q, s2.cin, s2.cout, sn.cout, first ? specs()[i2c + 1].cin : 0, c->plan.stream1x1_walkers, st);
}

hipError_t run_dense(hpe_ctx* c, const float* x, int lda, int M, int K, const float* w, int w_rows, int N, const float* scale,
                     const float* shift, const float* res, int ldres, int relu, float* y, int ldy, hipStream_t st, float* partial,
                     size_t partial_floats) {
    // single frames and very small batches: one launch per layer (the implicit-GEMM kernel would need split-K + a fix-up launch)
    if (M <= 4) return hpe_launch_dense_gemv(x, lda, M, K, w, N, scale, shift, res, ldres, relu, y, ldy, st);
    GemmArgs p{};
    p.zero = shift;  // any readable 16 B: dense mode never takes the zero-page path
    // the Dense layers run after the chunk streams have joined; in the pipelined forward they overlap the NEXT batch's encoder,
    // whose unchunked launches may split K too -> separate workspace
    p.partial = partial ? partial : c->dense_on_tail ? c->partial_tail : c->partial;
    p.partial_floats = partial ? partial_floats : c->dense_on_tail ? c->partial_tail_floats : c->partial_floats;
    p.x = x;
    p.w = w;
    p.scale = scale;
    p.shift = shift;
    p.res = res;
    p.y = y;
    p.M = M;
    p.N = N;
    p.K = K;
    p.lda = lda;
    p.ldw = K;
    p.w_rows = w_rows;
    p.ldy = ldy;
    p.ldres = ldres;
    p.relu = relu;
    return hpe_launch_gemm(p, GEMM_DENSE, TILE_64x64, c->plan.splitk_min_slabs, st);
}

static hipError_t timed_conv(hpe_ctx* c, int idx, const ConvRoute& r, const float* x, int B, const float* res, int relu, float* y, hipStream_t st,
                             float* wino_v = nullptr, int slot = 0) {
    const bool t2 = c->timing >= 2;
    if (t2) HIPE(hipEventRecord(c->cev0[idx], st));
    HIPE(run_conv(c, idx, r, x, B, res, relu, y, st, wino_v, slot));
    if (t2) HIPE(hipEventRecord(c->cev1[idx], st));
    return hipSuccess;
}

// the encoder on images [i0, i0+B) of the batch (all workspace buffers are image-major)
static hipError_t encoder_chunk(hpe_ctx* c, const float* images, int i0, int B, float* features, int ldfeat, hipStream_t st, int slot = 0,
                         bool concurrent = false) {
    // all workspace buffers are image-major; in bf16 mode the same allocations hold bf16 elements (half the bytes)
    const int esz = c->bf16 ? 2 : 4;
    auto at = [&](float* base, size_t elems) { return reinterpret_cast<float*>(reinterpret_cast<char*>(base) + elems * esz); };
    const size_t o_img = (size_t)i0 * HPE_IMG_SIZE * HPE_IMG_SIZE * 3;
    const size_t o_pad = (size_t)i0 * STEM_HP * STEM_WP * 4;
    const size_t o_big = (size_t)i0 * 802816;
    const size_t o_mid = (size_t)i0 * 200704;
    float* padded = at(c->padded, o_pad);
    float* SC = at(c->SC, o_big);
    float* T1 = at(c->T1, o_mid);
    float* T2 = at(c->T2, o_mid);
    float* cur = at(c->X0, o_big);
    float* nxt = at(c->X1, o_big);
    // the chunk's slice of the Winograd workspace (chunks of < 32 images only occur unchunked, i0 == 0: the slack at the end covers them)
    float* wv = (c->wino_v && (i0 == 0 || B >= 32)) ? c->wino_v + (size_t)i0 * WINO_V_PITCH : nullptr;
    const ConvQuery q{B, concurrent, false, wv != nullptr};
    // the fused stem stages whole 16-byte chunks of the caller's rows; an images pointer that is only float-aligned (e.g. a
    // tensor view at an odd offset) takes the pad / im2col / pool path, which reads the images with scalar loads
    if (c->plan.stem_fused && (reinterpret_cast<uintptr_t>(images + o_img) & 15) == 0) {
        // conv1_pad .. pool1 in one kernel straight from the caller's images (stem_fused.hip); timed as conv layer 0
        const bool t2 = c->timing >= 2;
        if (t2) HIPE(hipEventRecord(c->cev0[0], st));
        HIPE(hpe_launch_stem_fused(images + o_img, c->conv[0].stem_w, c->conv[0].scale, c->conv[0].shift, cur, B, hpe_stem_fused_pick_rows(B),
                                   c->bf16 ? 1 : 0, st));
        if (t2) HIPE(hipEventRecord(c->cev1[0], st));
    } else if (c->bf16) {
        HIPE(hpe_launch_pad_input_bf16(images + o_img, padded, B, HPE_IMG_SIZE, HPE_IMG_SIZE, STEM_HP, STEM_WP, st));
        HIPE(timed_conv(c, 0, route_conv(c->plan, true, 0, q), padded, B, nullptr, 1, SC, st));
        HIPE(hpe_launch_maxpool_bf16(SC, cur, B, 112, 64, st));
    } else {
        HIPE(hpe_launch_pad_input(images + o_img, padded, B, HPE_IMG_SIZE, HPE_IMG_SIZE, STEM_HP, STEM_WP, st));
        HIPE(timed_conv(c, 0, route_conv(c->plan, false, 0, q), padded, B, nullptr, 1, SC, st));
        HIPE(hpe_launch_maxpool(SC, cur, B, 112, 64, st));
    }
    bool have_2a = false;  // the previous block's chained launch has already written this block's branch2a output to T1
    for (const ResBlock& blk : blocks()) {
        const bool first = blk.first;
        const int i2a = blk.i2a, i2b = blk.i2b, i2c = blk.i2c, i1 = blk.i1;
        const BlockRoute br = route_block(c->plan, c->bf16, blk, q);  // (r2a.out_slab8: T1 is channel-slab major between branch2a and branch2b)
        if (have_2a) {
            if (c->timing >= 2) {
                HIPE(hipEventRecord(c->cev0[i2a], st));
                HIPE(hipEventRecord(c->cev1[i2a], st));
            }
        } else {
            HIPE(timed_conv(c, i2a, br.r2a, cur, B, nullptr, 1, T1, st));
        }
        have_2a = false;
        HIPE(timed_conv(c, i2b, br.r2b, T1, B, nullptr, 1, T2, st, wv, slot));
        const float* res = cur;
        if (br.stream_chain) {
            // the block's join and the next block's branch2a as one launch of conv_stream_chain_f32s.hip (timed as layer i2c; the projection
            // shortcut and the next branch2a then show 0)
            const bool t2 = c->timing >= 2;
            if (t2) HIPE(hipEventRecord(c->cev0[i2c], st));
            HIPE(run_stream_chain(c, i2c, first, T2, cur, B, nxt, T1, st, br.stream_u1_slab8));
            if (t2) {
                HIPE(hipEventRecord(c->cev1[i2c], st));
                if (first) {
                    HIPE(hipEventRecord(c->cev0[i1], st));
                    HIPE(hipEventRecord(c->cev1[i1], st));
                }
            }
            have_2a = true;
        } else if (br.join == JOIN_CHAIN) {
            // identity block followed by an identity block (bf16): relu(bn(W2c t2) + x) and the next block's relu(bn(W2a' .)) in one
            // launch; the 4C-wide sum is written once and not read back (timed as layer i2c; the next branch2a then shows 0)
            const bool t2 = c->timing >= 2;
            if (t2) HIPE(hipEventRecord(c->cev0[i2c], st));
            HIPE(run_chain(c, i2c, first, T2, cur, B, nxt, T1, st, br.u1_slab8));
            if (t2) {
                HIPE(hipEventRecord(c->cev1[i2c], st));
                if (first) {  // the projection shortcut is inside the launch
                    HIPE(hipEventRecord(c->cev0[i1], st));
                    HIPE(hipEventRecord(c->cev1[i1], st));
                }
            }
            have_2a = true;
        } else if (br.join == JOIN_DUAL) {
            // conv_block: expand convolution + projection shortcut + add + ReLU as one dual-source GEMM (timed as layer i2c)
            const bool t2 = c->timing >= 2;
            if (t2) HIPE(hipEventRecord(c->cev0[i2c], st));
            HIPE(run_dual(c, i2c, i1, br.r2c, T2, cur, B, nxt, st));
            if (t2) {
                HIPE(hipEventRecord(c->cev1[i2c], st));
                HIPE(hipEventRecord(c->cev0[i1], st));
                HIPE(hipEventRecord(c->cev1[i1], st));
            }
        } else {
            if (first) {
                // projection shortcut (conv_block), no ReLU before the add
                HIPE(timed_conv(c, i1, br.r1, cur, B, nullptr, 0, SC, st));
                res = SC;
            }
            HIPE(timed_conv(c, i2c, br.r2c, T2, B, res, 1, nxt, st));
        }
        float* t = cur;
        cur = nxt;
        nxt = t;
    }
    if (c->bf16) return hpe_launch_avgpool_bf16(cur, features + (size_t)i0 * ldfeat, B, 49, HPE_FEATURE_DIM, ldfeat, st);
    return hpe_launch_avgpool(cur, features + (size_t)i0 * ldfeat, B, 49, HPE_FEATURE_DIM, ldfeat, st);
}

// Batch chunks run on separate HIP streams (fork/join with events around the caller's stream): images are
// independent, so while one chunk's launch drains its last partial round of workgroups (49*2^k tiles never fill
// 256 CUs x 2 evenly) the other chunk's kernels fill the idle CUs.  Per-conv event timing (level 2) needs
// back-to-back launches on one stream and therefore runs unchunked.
hipError_t encoder_impl(hpe_ctx* c, const float* images, int B, float* features, int ldfeat, hipStream_t st) {
    int nstream = c->plan.n_streams;
    // a chunk needs >= 32 images to keep its own launches efficient.  Rounds 1-2 had 44 (B = 64 was 7 % faster unchunked,
    // profiles/r01/g_wino_chunk_rule.txt); with the 32-cout / C-split F(4x4) launches of round 3 two chunks of 32-40 win: B = 64 / 72 / 80
    // 15.0 / 15.1 / 15.8 k img/s in two chunks against 14.1 / 13.4 / 14.1 k unchunked, B = 56 13.3 against 13.6 k, B = 40 12.5 against
    // 12.8 k (profiles/r03/chunk_rule.txt); B = 128 best with 2 chunks, B = 256 equal for 2-3, 4 chunks of 64 lose 5 %
    if (nstream > B / c->plan.min_chunk) nstream = B / c->plan.min_chunk;
    if (c->timing >= 2 || nstream < 2) nstream = 1;
    if (nstream == 1) return encoder_chunk(c, images, 0, B, features, ldfeat, st);
    // chunk size: about HPE_CHUNK images (default: one chunk per stream), never below min_chunk -- smaller chunks are launch bound
    //  -- and all chunks of equal size +-1; chunks go round-robin over the streams
    int nchunk = nstream;
    if (c->plan.chunk_images > 0) {
        const int want = c->plan.chunk_images < c->plan.min_chunk ? c->plan.min_chunk : c->plan.chunk_images;
        nchunk = B / want;
        if (nchunk < nstream) nchunk = nstream;
    }
    const int per = (B + nchunk - 1) / nchunk;
    nchunk = (B + per - 1) / per;
    HIPE(hipEventRecord(c->ev_fork, st));
    for (int k = 1; k < nstream; ++k) HIPE(hipStreamWaitEvent(c->aux[k - 1], c->ev_fork, 0));
    c->co_running = nstream;
    for (int k = 0; k < nchunk; ++k) {
        const int i0 = k * per;
        const int n = (i0 + per <= B) ? per : (B - i0);
        const int sid = k % nstream;
        hipStream_t s = (sid == 0) ? st : c->aux[sid - 1];
        const hipError_t ec = encoder_chunk(c, images, i0, n, features, ldfeat, s, sid, true);
        if (ec != hipSuccess) {
            c->co_running = 1;
            return ec;
        }
    }
    c->co_running = 1;
    // The join: an event behind the last launch of every chunk stream, waited for on the caller's stream.  Whatever is enqueued on `st`
    // after this call therefore runs after every launch of it; hpe_encoder_set_params_dev relies on that to rewrite the weights in
    // stream order without a wait of its own.
    for (int k = 1; k < nstream; ++k) {
        HIPE(hipEventRecord(c->ev_join[k - 1], c->aux[k - 1]));
        HIPE(hipStreamWaitEvent(st, c->ev_join[k - 1], 0));
    }
    return hipSuccess;
}

// one IEF step on padded theta rows [B, THETA_LD]; P1 = features . W1[:2048] must be current
hipError_t regress_impl(hpe_ctx* c, const float* th_prev, float* th_next, int B, hipStream_t st) {
    HIPE(run_dense(c, th_prev, THETA_LD, B, THETA_LD, c->w1t, 1024, 1024, c->ones, c->b1, c->P1, 1024, 1, c->H1, 1024, st));
    HIPE(run_dense(c, c->H1, 1024, B, 1024, c->w2, 1024, 1024, c->ones, c->b2, nullptr, 0, 1, c->H2, 1024, st));
    return run_dense(c, c->H2, 1024, B, 1024, c->w3, 128, HPE_THETA_DIM, c->ones, c->b3, th_prev, THETA_LD, 0, th_next, THETA_LD, st);
}

hipError_t features_proj(hpe_ctx* c, const float* features, int B, hipStream_t st) {
    return run_dense(c, features, HPE_FEATURE_DIM, B, HPE_FEATURE_DIM, c->w1f, 1024, 1024, c->ones, c->zeros, nullptr, 0, 0, c->P1,
                     1024, st);
}

// features [B,2048] -> feature projection (hoisted W1 block), then num_stage x (regressor step, SMPL of the stages that are returned);
// feat_free (optional) is recorded once the features have been consumed
hipError_t tail_impl(hpe_ctx* c, const float* feat, int B, const HpeOutputs* stage_outs, int n_outs, hipStream_t ts, hipEvent_t feat_free) {
    hipError_t e = features_proj(c, feat, B, ts);
    if (e == hipSuccess && feat_free) e = hipEventRecord(feat_free, ts);
    if (e == hipSuccess) e = hpe_launch_tile_theta(c->mean_dev, c->thA, B, THETA_LD, ts);
    float* prev = c->thA;
    float* next = c->thB;
    const int first_out = c->cfg.num_stage - n_outs;
    for (int s = 0; e == hipSuccess && s < c->cfg.num_stage; ++s) {
        e = regress_impl(c, prev, next, B, ts);
        if (e == hipSuccess && s >= first_out) e = hpe_launch_smpl(c->smpl, c->work, next, THETA_LD, B, &stage_outs[s - first_out], ts);
        float* t = prev;
        prev = next;
        next = t;
    }
    return e;
}

// What runs on `st` from here on reads or writes buffers the tail of a pipelined call uses (regressor weights and activations, SMPL
// work buffers): order it behind a tail that may still be running
hipError_t join_tail(hpe_ctx* c, hipStream_t st) {
    if (!c->tail_pending) return hipSuccess;
    HIPE(hipStreamWaitEvent(st, c->ev_tail, 0));
    c->tail_pending = false;
    return hipSuccess;
}

// encoder on `st`; regressor + SMPL stages on `st` (pipelined == false) or on the ctx's tail stream behind an event (true)
int forward_impl(hpe_ctx* c, const float* images, int B, const HpeOutputs* stage_outs, int n_outs, hipStream_t st, bool pipelined) {
    int rc = check_ready(c, B, NEED_ENC | NEED_REG | NEED_SMPL);
    if (rc) return rc;
    if (!images || !stage_outs) return fail(HPE_ERR_INVALID, "null pointer");
    if (n_outs < 1 || n_outs > c->cfg.num_stage) return fail(HPE_ERR_INVALID, "n_outs must be in [1, num_stage]");
    DeviceGuard g(c->cfg.device);
    const bool tm = c->timing != 0;
    if (c->timing >= 2) pipelined = false;  // per-launch event timing wants one serial stream
    float* feat = c->feat;
    hipStream_t ts = st;
    if (pipelined) {
        // features alternate between two buffers: the tail of batch k reads one while the encoder of batch k+1 fills the other;
        // the buffer used now was last read by the feature projection of two calls ago (long finished: the wait is a formality)
        const unsigned slot = c->pipe_idx & 1u;
        feat = slot ? c->feat_alt : c->feat;
        if (c->feat_free_valid[slot]) HIP_TRY(hipStreamWaitEvent(st, c->ev_feat_free[slot], 0));
        ts = c->tail_st;
    } else {
        HIP_TRY(join_tail(c, st));  // a serial call after pipelined ones
    }
    if (tm) {
        HIP_TRY(hipEventRecord(c->ev[0], st));
        HIP_TRY(hipEventRecord(c->span0[c->span_n % hpe_ctx::SPAN_RING], st));
    }
    HIP_TRY(encoder_impl(c, images, B, feat, HPE_FEATURE_DIM, st));
    if (tm) {
        HIP_TRY(hipEventRecord(c->ev[1], st));
        HIP_TRY(hipEventRecord(c->span1[c->span_n % hpe_ctx::SPAN_RING], st));
        ++c->span_n;
    }
    if (pipelined) {
        HIP_TRY(hipEventRecord(c->ev_enc, st));
        HIP_TRY(hipStreamWaitEvent(ts, c->ev_enc, 0));
        c->dense_on_tail = true;
    }
    hipEvent_t feat_free = nullptr;
    if (pipelined) {
        const unsigned slot = c->pipe_idx & 1u;
        feat_free = c->ev_feat_free[slot];
        c->feat_free_valid[slot] = true;
    }
    hipError_t e = tail_impl(c, feat, B, stage_outs, n_outs, ts, feat_free);
    c->dense_on_tail = false;
    if (e != hipSuccess) return fail(HPE_ERR_HIP, std::string("forward tail: ") + hipGetErrorString(e));
    if (pipelined) {
        HIP_TRY(hipEventRecord(c->ev_tail, ts));
        c->tail_pending = true;
        ++c->pipe_idx;
    }
    if (tm) {
        HIP_TRY(hipEventRecord(c->ev[4], ts));
        c->timed_valid = true;
        c->conv_timed_valid = c->timing >= 2;
    }
    return HPE_OK;
}

