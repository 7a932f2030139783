// encoder_train.hip -- fine-tuning the ResNet-50 encoder with the BatchNorm statistics held fixed (Keras' frozen-BN mode; the generator
// update of src/trainer.py:481 puts image_feature_extractor.trainable_variables into the Adam step): the layer-by-layer training forward
// that keeps every activation, the backward to the flat parameters, and the flat <-> live parameter copies.
//
// Per conv layer, with s = gamma / sqrt(var + eps):   y = act(s * (conv(x, W) + b - mean) + beta (+ residual))
//
//   dz = dy * [y > 0]          (enc_gate_kernel; TensorFlow's ReLU gradient, zero at 0; also writes dz * s, the data-gradient operand)
//   G  = A^T dz                (conv_wg_gemm_kernel + conv_wg_fixup_kernel; A = the gathered im2col of x)
//   dW = s * G    dshift = sum_m dz    dbeta = dshift    db = s * dshift    dgamma = (<W[:,n], G[:,n]> + (b - mean) * dshift) / sqrt(var + eps)
//   dx = (dz * s) . W^T        (the implicit-GEMM launcher of the forward: dense for 1x1, CONV3 with the flipped, channel-transposed kernel for
//                               3x3; a 1x1 / stride 2 layer runs the dense GEMM on the low-resolution map, enc_scatter2_kernel spreads it)
//
// sum_m dz * conv_raw = sum_k W[k][n] G[k][n] exactly, so the BatchNorm gradient needs neither the pre-BN tensor nor a division by s.
//
// The kernels and their launchers are in encoder_grad.hip, those of BatchNorm with batch statistics in encoder_bn.hip, those of the
// mixed-precision walks (bf16 activations and cotangents on this fp32 context) in encoder_grad_bf16.hip and, for their BatchNorm with
// batch statistics, encoder_bn_bf16.hip; this file holds the layout, the reserves, the two walks (one forward, one backward, each taking
// the BatchNorm mode and the precision as per-layer choices) and the C ABI.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "hpe_ctx.h"

constexpr int POOL_FLOATS = 56 * 56 * 64;  // the max-pooled map, per image
constexpr int BIG = 802816, MID = 200704;  // the largest layer output / the largest bottleneck (and low-resolution) map, per image

const EncLayout& layout() {
    static const EncLayout L = [] {
        EncLayout l{};
        int o = 0, ch = 0;
        size_t so = 0;
        for (int i = 0; i < HPE_NUM_CONV; ++i) {
            const ConvSpec& s = specs()[i];
            l.off[i][0] = o;
            o += s.kh * s.kw * s.cin * s.cout;
            for (int w = 1; w < 4; ++w) {
                l.off[i][w] = o;
                o += s.cout;
            }
            l.stat[i] = ch;
            ch += s.cout;
            l.stash[i] = so;
            so += (size_t)s.hout * s.hout * s.cout;
        }
        l.stash_pool = so;
        l.stash_per_image = so + POOL_FLOATS;
        l.total = o;
        l.channels = ch;
        return l;
    }();
    return L;
}

namespace {

// Every buffer of hpe_encoder_train_reserve at batch B, in allocation order, as f(member, floats, zero-filled): the reserve allocates
// through this and hpe_encoder_train_ws_floats adds it up
template <class F>
void train_buffers(EncTrainWork& w, int B, F&& f) {
    const EncLayout& l = layout();
    const size_t nb = (size_t)B;
    f(w.stash, nb * l.stash_per_image, false);
    f(w.g0, nb * BIG, false);
    f(w.g1, nb * BIG, false);
    f(w.sbig, nb * BIG, false);
    f(w.t0, nb * MID, false);
    f(w.t1, nb * MID, false);
    f(w.ssmall, nb * MID, false);
    f(w.partial, wg_partial_floats(B), false);
    f(w.dsh, (size_t)WG_MAX_SLICES * 2048, false);
    f(w.wgp, (size_t)WG_WGP_FLOATS, false);
    f(w.zeros, 2048, true);
    f(w.feat, nb * HPE_FEATURE_DIM, false);
    f(w.flat, l.total, false);
    f(w.mean, l.channels, false);
    f(w.istd, l.channels, false);
    f(w.sd, 2 * (size_t)l.channels, false);  // `channels` doubles
    for (int i = 1; i < HPE_NUM_CONV; ++i) f(w.dxw[i], conv_dxw_floats(i), false);
}

// ... and what hpe_encoder_train_reserve_batchnorm adds
template <class F>
void train_buffers_bn(EncTrainWork& w, int B, F&& f) {
    const EncLayout& l = layout();
    f(w.zstash, (size_t)B * l.stash_pool, false);
    f(w.bn_batch, 3 * (size_t)l.channels + 3 * 2048, true);
    f(w.bn_stats, 2 * (size_t)l.channels, false);
    f(w.bn_part, 4 * (size_t)BN_PART_COLS, false);  // 2 * BN_PART_COLS doubles
    f(w.bn_hw, l.channels, false);
}

// ... and what hpe_encoder_train_reserve_mixed adds: bf16 elements, two to a float (every count is even).  The weight operands are zeroed:
// the cast that opens a mixed call never writes their k padding
constexpr size_t PADDED16 = (size_t)STEM_HP * STEM_WP * 4;  // the padded bf16 input, per image
template <class F>
void train_buffers_mixed(EncTrainWork& w, int B, F&& f) {
    const EncLayout& l = layout();
    const size_t nb = (size_t)B;
    f(w.mx_stash, nb * l.stash_per_image / 2, false);
    f(w.mx_g0, nb * BIG / 2, false);
    f(w.mx_g1, nb * BIG / 2, false);
    f(w.mx_sbig, nb * BIG / 2, false);
    f(w.mx_t0, nb * MID / 2, false);
    f(w.mx_t1, nb * MID / 2, false);
    f(w.mx_ssmall, nb * MID / 2, false);
    f(w.mx_padded, nb * PADDED16 / 2, false);
    for (int i = 0; i < HPE_NUM_CONV; ++i) f(w.mx_w[i], (size_t)round_up(specs()[i].cout, 128) * conv_k_pad(i, true) / 2, true);
    for (int i = 1; i < HPE_NUM_CONV; ++i) f(w.mx_dxw[i], conv_dxw_floats(i) / 2, false);
    f(w.mx_cast, (size_t)MX_CAST_SEGS * sizeof(MxCastSeg) / sizeof(float), false);
}

// ... and what hpe_encoder_train_reserve_batchnorm_mixed adds to those two: the bf16 raw-output stash
template <class F>
void train_buffers_bn_mixed(EncTrainWork& w, int B, F&& f) {
    f(w.mx_zstash, (size_t)B * layout().stash_pool / 2, false);
}

struct TrainAlloc {  // rc keeps the first failure, which ends the allocations
    hpe_ctx* c;
    int rc = HPE_OK;
    template <class T>
    void operator()(T*& member, size_t floats, bool zero) {
        float* p = nullptr;
        if (rc == HPE_OK && (rc = dev_alloc(c, &p, floats, zero)) == HPE_OK) member = reinterpret_cast<T*>(p);
    }
};

size_t ws_floats(int B, bool bn, bool mixed = false, bool bn_mixed = false) {
    EncTrainWork w;
    size_t n = encoder_repack_reserve_floats();  // the layer table of hpe_encoder_set_params_dev, allocated by encoder_repack_reserve
    auto add = [&n](auto&, size_t floats, bool) { n += floats; };
    train_buffers(w, B, add);
    if (bn) train_buffers_bn(w, B, add);
    if (mixed) train_buffers_mixed(w, B, add);
    if (bn_mixed) train_buffers_bn_mixed(w, B, add);
    return n;
}

// the walks: frozen statistics in fp32, batch statistics in fp32, frozen statistics in mixed precision, batch statistics in mixed
// precision.  A mixed walk keeps bf16 elements behind the float pointers of its activations and cotangents (as a bf16 context does
// behind ConvLayer::w)
enum Walk { WALK_FROZEN, WALK_BATCH, WALK_MIXED, WALK_MIXED_BATCH };
bool walk_bn(Walk wk) { return wk == WALK_BATCH || wk == WALK_MIXED_BATCH; }
bool walk_mx(Walk wk) { return wk == WALK_MIXED || wk == WALK_MIXED_BATCH; }
cmx16 h16(const float* p) { return reinterpret_cast<cmx16>(p); }
mx16 h16(float* p) { return reinterpret_cast<mx16>(p); }
float* f16(mx16 p) { return reinterpret_cast<float*>(p); }

// the data-gradient operand of layer idx in the forward GEMM's Wt[n][k] form: rows = input channels (zero padded to 128), k = output channels
// (1x1: the HWIO matrix itself) or (tap', output channel) with the taps flipped (3x3)
void pack_dx_weights(int idx, const float* kernel, std::vector<float>& out) {
    const ConvSpec& s = specs()[idx];
    const int taps = s.kh * s.kw, K = taps * s.cout;
    out.assign(conv_dxw_floats(idx), 0.f);
    for (int t = 0; t < taps; ++t)
        for (int ci = 0; ci < s.cin; ++ci) {
            const float* src = kernel + ((size_t)t * s.cin + ci) * s.cout;
            std::copy(src, src + s.cout, out.begin() + (size_t)ci * K + (size_t)(taps - 1 - t) * s.cout);
        }
}

float* stash_of(hpe_ctx* c, int idx, int B) {
    const EncLayout& l = layout();
    return c->et.stash + (size_t)B * (idx < 0 ? l.stash_pool : l.stash[idx]);
}

// ... of the walk's own stash: the mixed one has the same layout in bf16 elements
float* stash_of(hpe_ctx* c, Walk wk, int idx, int B) {
    if (!walk_mx(wk)) return stash_of(c, idx, B);
    const EncLayout& l = layout();
    return f16(c->et.mx_stash + (size_t)B * (idx < 0 ? l.stash_pool : l.stash[idx]));
}

// ---- BatchNorm with batch statistics (encoder_bn.hip holds the kernels): z kept beside y, the layer's statistics in its slots

float* zstash_of(hpe_ctx* c, int idx, int B) { return c->et.zstash + (size_t)B * layout().stash[idx]; }
mx16 mx_zstash_of(hpe_ctx* c, int idx, int B) { return c->et.mx_zstash + (size_t)B * layout().stash[idx]; }

struct BnSlots {
    float *mu, *var, *r;
};

// layer idx's slots of the batch statistics; scratch: the three 2048-float slots behind them, for the one-layer debug calls
BnSlots bn_slots(hpe_ctx* c, int idx, bool scratch) {
    const EncLayout& l = layout();
    float* b = c->et.bn_batch;
    if (scratch) return {b + 3 * l.channels, b + 3 * l.channels + 2048, b + 3 * l.channels + 4096};
    return {b + l.stat[idx], b + l.channels + l.stat[idx], b + 2 * l.channels + l.stat[idx]};
}

// the reduce buffers of data-parallel training, in the weight gradient's scratch (hpe_ctx.h): the sums [2][N] doubles that cross the
// ranks, and behind them the reduced dbeta | dgamma [2][N] floats
double* reduce_sums(hpe_ctx* c) { return reinterpret_cast<double*>(c->et.wgp); }
float* reduce_grads(hpe_ctx* c) { return c->et.wgp + 2 * 2 * 2048; }

// the rows of layer idx over the batch of all ranks
double rows_all(hpe_ctx* c, int idx) { return (double)c->et.reduce_G * specs()[idx].hout * specs()[idx].hout; }

// the hook on `count` doubles of the reduce buffer; a failure is kept for the entry point, which names the layer
hipError_t reduce_call(hpe_ctx* c, int idx, long long count, hipStream_t st) {
    if (c->et.reduce(c->et.reduce_user, reduce_sums(c), count, st) == 0) return hipSuccess;
    c->et.reduce_failed = idx;
    return hipErrorUnknown;
}

// z = conv(x, W) + b (the layer's own route, unit scale, the bias of the flat copy as shift), its statistics, y = act(BN(z) (+ res)).
// reduce: the statistics of all ranks' rows (the hook is set)
hipError_t layer_forward_bn(hpe_ctx* c, int idx, const float* x, int B, const float* res, int relu, float* z, float* y, const BnSlots& s, hipStream_t st,
                            bool reduce = false) {
    const ConvSpec& sp = specs()[idx];
    const EncLayout& l = layout();
    const float* flat = c->et.flat;
    const int M = B * sp.hout * sp.hout;
    HIPE(run_conv_nhwc(c, idx, x, B, nullptr, 0, z, st, c->ones, flat + l.off[idx][1]));
    if (reduce) {
        HIPE(bn_launch_stats_sums(z, M, sp.cout, c->et.bn_part, reduce_sums(c), st));
        HIPE(reduce_call(c, idx, 2LL * sp.cout, st));
        HIPE(bn_launch_stats_from_sums(reduce_sums(c), rows_all(c, idx), sp.cout, c->cfg.bn_eps, s.mu, s.var, s.r, st));
    } else {
        HIPE(bn_launch_stats(z, M, sp.cout, c->cfg.bn_eps, c->et.bn_part, s.mu, s.var, s.r, st));
    }
    return bn_launch_apply(z, s.mu, s.r, flat + l.off[idx][2], flat + l.off[idx][3], res, relu, y, M, sp.cout, st);
}

// the gate and the BatchNorm backward of layer idx: db (= 0), dgamma, dbeta into grad_layer; dz (may be nullptr, may alias dy) and dzraw
// reduce: grad_layer keeps this rank's partial sums, dzraw is that of the batch of all ranks (the hook is set)
hipError_t layer_gate_bn(hpe_ctx* c, int idx, const float* dy, const float* y, const float* z, int B, const BnSlots& s, float* grad_layer, float* dz,
                         float* dzraw, hipStream_t st, bool reduce = false) {
    const ConvSpec& sp = specs()[idx];
    const int M = B * sp.hout * sp.hout, N = sp.cout, kn = sp.kh * sp.kw * sp.cin * N;
    float *db = grad_layer + kn, *dgamma = db + N, *dbeta = dgamma + N;
    const float* gamma = c->et.flat + layout().off[idx][2];
    if (!reduce) {
        HIPE(bn_launch_bwd_reduce(dy, y, z, s.mu, s.r, M, N, c->et.bn_part, db, dgamma, dbeta, st));
        return bn_launch_bwd_apply(dy, y, z, s.mu, s.r, gamma, dgamma, dbeta, M, N, dz, dzraw, st);
    }
    float* red = reduce_grads(c);
    HIPE(bn_launch_bwd_sums(dy, y, z, s.mu, s.r, M, N, c->et.bn_part, reduce_sums(c), db, dgamma, dbeta, st));
    HIPE(reduce_call(c, idx, 2LL * N, st));
    HIPE(bn_launch_bwd_from_sums(reduce_sums(c), N, red, st));
    return bn_launch_bwd_apply(dy, y, z, s.mu, s.r, gamma, red + N, red, M, N, dz, dzraw, st, rows_all(c, idx));
}

// layer_forward_bn in mixed precision: z16 = RNE(conv(x16, W16) + b) through the layer's bf16 route, the statistics OF z16 into the same
// slots, y16 = RNE(act(BN(z16) (+ res16))).  Only the first-stage kernels differ: the hook sees the same sums at the same place
hipError_t layer_forward_bn16(hpe_ctx* c, int idx, cmx16 x, int B, cmx16 res, int relu, mx16 z, mx16 y, const BnSlots& s, hipStream_t st,
                              bool reduce = false) {
    const ConvSpec& sp = specs()[idx];
    const EncLayout& l = layout();
    const float* flat = c->et.flat;
    const int M = B * sp.hout * sp.hout;
    HIPE(mx_conv_forward(c, idx, x, B, nullptr, 0, z, st, c->ones, flat + l.off[idx][1]));
    if (reduce) {
        HIPE(bn16_launch_stats_sums(z, M, sp.cout, c->et.bn_part, reduce_sums(c), st));
        HIPE(reduce_call(c, idx, 2LL * sp.cout, st));
        HIPE(bn_launch_stats_from_sums(reduce_sums(c), rows_all(c, idx), sp.cout, c->cfg.bn_eps, s.mu, s.var, s.r, st));
    } else {
        HIPE(bn16_launch_stats(z, M, sp.cout, c->cfg.bn_eps, c->et.bn_part, s.mu, s.var, s.r, st));
    }
    return bn16_launch_apply(z, s.mu, s.r, flat + l.off[idx][2], flat + l.off[idx][3], res, relu, y, M, sp.cout, st);
}

// ... and layer_gate_bn: db (= 0), dgamma, dbeta (fp32) into grad_layer; dz (bf16, exact; may be nullptr, may alias dy) and dzraw16
hipError_t layer_gate_bn16(hpe_ctx* c, int idx, cmx16 dy, cmx16 y, cmx16 z, int B, const BnSlots& s, float* grad_layer, mx16 dz, mx16 dzraw,
                           hipStream_t st, bool reduce = false) {
    const ConvSpec& sp = specs()[idx];
    const int M = B * sp.hout * sp.hout, N = sp.cout, kn = sp.kh * sp.kw * sp.cin * N;
    float *db = grad_layer + kn, *dgamma = db + N, *dbeta = dgamma + N;
    const float* gamma = c->et.flat + layout().off[idx][2];
    if (!reduce) {
        HIPE(bn16_launch_bwd_reduce(dy, y, z, s.mu, s.r, M, N, c->et.bn_part, db, dgamma, dbeta, st));
        return bn16_launch_bwd_apply(dy, y, z, s.mu, s.r, gamma, dgamma, dbeta, M, N, dz, dzraw, st);
    }
    float* red = reduce_grads(c);
    HIPE(bn16_launch_bwd_sums(dy, y, z, s.mu, s.r, M, N, c->et.bn_part, reduce_sums(c), db, dgamma, dbeta, st));
    HIPE(reduce_call(c, idx, 2LL * N, st));
    HIPE(bn_launch_bwd_from_sums(reduce_sums(c), N, red, st));
    return bn16_launch_bwd_apply(dy, y, z, s.mu, s.r, gamma, red + N, red, M, N, dz, dzraw, st, rows_all(c, idx));
}

// The training forward, every activation kept in the stash.  bn (batch statistics): z kept beside y, the statistics in the layers' slots
//                       mixed: the weight operands are cast from the live fp32 weights first, every layer runs on the bf16 GEMMs
hipError_t forward_train(hpe_ctx* c, Walk wk, const float* images, int B, float* features, hipStream_t st) {
    const bool bn = walk_bn(wk), mx = walk_mx(wk);
    const bool reduce = bn && c->et.reduce != nullptr;
    auto stash = [&](int idx) { return stash_of(c, wk, idx, B); };
    auto layer = [&](int idx, const float* x, const float* res, int relu) {
        float* y = stash(idx);
        if (mx && bn) return layer_forward_bn16(c, idx, h16(x), B, h16(res), relu, mx_zstash_of(c, idx, B), h16(y), bn_slots(c, idx, false), st, reduce);
        if (mx) return mx_conv_forward(c, idx, h16(x), B, h16(res), relu, h16(y), st);
        return bn ? layer_forward_bn(c, idx, x, B, res, relu, zstash_of(c, idx, B), y, bn_slots(c, idx, false), st, reduce)
                  : run_conv_nhwc(c, idx, x, B, res, relu, y, st);
    };
    if (mx) {
        HIPE(mx_cast_launch(c, 0, MX_CAST_SEGS, st));
        HIPE(hpe_launch_pad_input_bf16(images, c->et.mx_padded, B, HPE_IMG_SIZE, HPE_IMG_SIZE, STEM_HP, STEM_WP, st));
        HIPE(layer(0, f16(c->et.mx_padded), nullptr, 1));
        HIPE(hpe_launch_maxpool_bf16(stash(0), stash(-1), B, 112, 64, st));
    } else {
        HIPE(hpe_launch_pad_input(images, c->padded, B, HPE_IMG_SIZE, HPE_IMG_SIZE, STEM_HP, STEM_WP, st));
        HIPE(layer(0, c->padded, nullptr, 1));
        HIPE(hpe_launch_maxpool(stash(0), stash(-1), B, 112, 64, st));
    }
    for (const ResBlock& blk : blocks()) {
        const float* cur = stash(blk.in);
        HIPE(layer(blk.i2a, cur, nullptr, 1));
        HIPE(layer(blk.i2b, stash(blk.i2a), nullptr, 1));
        const float* res = cur;
        if (blk.first) {
            HIPE(layer(blk.i1, cur, nullptr, 0));
            res = stash(blk.i1);
        }
        HIPE(layer(blk.i2c, stash(blk.i2b), res, 1));
    }
    const float* last = stash(blocks().back().i2c);
    if (mx) return hpe_launch_avgpool_bf16(last, features, B, 49, HPE_FEATURE_DIM, HPE_FEATURE_DIM, st);
    return hpe_launch_avgpool(last, features, B, 49, HPE_FEATURE_DIM, HPE_FEATURE_DIM, st);
}

struct GateOut {
    const float *wg, *dg;  // what the layer's weight gradient and its data gradient read
};

// The cotangent dy of layer idx's output -> that of its convolution.  gated: the layer has a ReLU; keep: dy's buffer must hold dz
// afterwards (branch2c: it is the shortcut's cotangent too); copy: receives the data-gradient operand.
//   frozen  dz in place where there is a ReLU (without one dz is dy), copy = dz * s (none for conv1, which has no data gradient); the
//           weight gradient reads dz
//   batch   the bias / gamma / beta gradients go into grad_flat, copy = dzraw, which both gradients read; dz is written only if kept
//   mixed   as frozen on bf16 elements; copy = RNE(dz * s)
//   mixed batch   as batch on bf16 elements; copy = dzraw16, the bias / gamma / beta gradients stay fp32
hipError_t layer_gate(hpe_ctx* c, Walk wk, int idx, float* dy, bool gated, bool keep, float* copy, int B, float* grad_flat, hipStream_t st,
                      GateOut* o) {
    const ConvSpec& s = specs()[idx];
    const float* y = gated ? stash_of(c, wk, idx, B) : nullptr;
    if (wk == WALK_MIXED_BATCH) {
        *o = {copy, copy};
        return layer_gate_bn16(c, idx, h16(dy), h16(y), mx_zstash_of(c, idx, B), B, bn_slots(c, idx, false), grad_flat + layout().off[idx][0],
                               keep ? h16(dy) : nullptr, h16(copy), st, c->et.reduce != nullptr);
    }
    if (wk == WALK_MIXED) {
        float* dzs = idx == 0 ? nullptr : copy;
        mx_gate(h16(dy), h16(y), dzs ? c->conv[idx].scale : nullptr, gated ? h16(dy) : nullptr, h16(dzs), (long)B * s.hout * s.hout * s.cout, s.cout, st);
        *o = {dy, dzs};
        return hipSuccess;
    }
    if (wk == WALK_BATCH) {
        *o = {copy, copy};
        return layer_gate_bn(c, idx, dy, y, zstash_of(c, idx, B), B, bn_slots(c, idx, false), grad_flat + layout().off[idx][0], keep ? dy : nullptr,
                             copy, st, c->et.reduce != nullptr);
    }
    float* dzs = idx == 0 ? nullptr : copy;
    gate(dy, y, dzs ? c->conv[idx].scale : nullptr, gated ? dy : nullptr, dzs, (long)B * s.hout * s.hout * s.cout, s.cout, st);
    *o = {dy, dzs};
    return hipSuccess;
}

hipError_t backward(hpe_ctx* c, Walk wk, const float* images, int B, const float* grad_features, float* grad_flat, hipStream_t st) {
    EncTrainWork& w = c->et;
    const bool bn = walk_bn(wk), mx = walk_mx(wk);
    HIPE(forward_train(c, wk, images, B, w.feat, st));
    auto stash = [&](int idx) { return stash_of(c, wk, idx, B); };
    auto lgate = [&](int idx, float* dy, bool gated, bool keep, float* copy, GateOut* o) {
        return layer_gate(c, wk, idx, dy, gated, keep, copy, B, grad_flat, st, o);
    };
    auto wgrad = [&](int idx, const float* x, const float* dz) {
        float* grad_layer = grad_flat + layout().off[idx][0];
        return mx ? mx_weight_grad(c, idx, h16(x), h16(dz), B, grad_layer, st, bn) : weight_grad(c, idx, x, dz, B, grad_layer, st, bn);
    };
    auto dgrad = [&](int idx, const float* dzs, const float* res, float* out) {
        return mx ? mx_data_grad(c, idx, h16(dzs), B, h16(res), h16(out), st) : data_grad(c, idx, dzs, B, res, out, st);
    };
    GateOut o2c, o2b, o2a, o1, o0;
    // the cotangent and operand buffers of the walk's precision
    float *g = mx ? f16(w.mx_g0) : w.g0, *go = mx ? f16(w.mx_g1) : w.g1, *sbig = mx ? f16(w.mx_sbig) : w.sbig;
    float *t0 = mx ? f16(w.mx_t0) : w.t0, *t1 = mx ? f16(w.mx_t1) : w.t1, *ssmall = mx ? f16(w.mx_ssmall) : w.ssmall;
    if (mx) {
        mx_avgpool_bwd(grad_features, h16(g), B, 49, HPE_FEATURE_DIM, st);
    } else {
        avgpool_bwd(grad_features, g, B, 49, HPE_FEATURE_DIM, st);
    }
    for (auto it = blocks().rbegin(); it != blocks().rend(); ++it) {
        const int i2a = it->i2a, i2b = it->i2b, i2c = it->i2c, i1 = it->i1;
        const ConvSpec& sa = specs()[i2a];
        const float* xin = stash(it->in);  // the block's input: the previous block's branch2c output
        // branch2c: g becomes dz (the cotangent of the shortcut too)
        HIPE(lgate(i2c, g, true, true, sbig, &o2c));
        HIPE(wgrad(i2c, stash(i2b), o2c.wg));
        HIPE(dgrad(i2c, o2c.dg, nullptr, t0));
        HIPE(lgate(i2b, t0, true, false, ssmall, &o2b));
        HIPE(wgrad(i2b, stash(i2a), o2b.wg));
        HIPE(dgrad(i2b, o2b.dg, nullptr, t1));
        HIPE(lgate(i2a, t1, true, false, ssmall, &o2a));
        HIPE(wgrad(i2a, xin, o2a.wg));
        if (!it->first) {
            HIPE(dgrad(i2a, o2a.dg, g, go));
            std::swap(g, go);
            continue;
        }
        // projection shortcut: no activation of its own, its dz is the block's
        HIPE(lgate(i1, g, false, false, sbig, &o1));
        HIPE(wgrad(i1, xin, o1.wg));
        if (sa.stride == 1) {
            HIPE(dgrad(i2a, o2a.dg, nullptr, go));
            HIPE(dgrad(i1, o1.dg, go, g));
        } else {
            HIPE(dgrad(i2a, o2a.dg, nullptr, t0));
            HIPE(dgrad(i1, o1.dg, t0, t1));
            if (mx) {
                mx_scatter2(h16(t1), h16(go), B, sa.hout, sa.cin, st);
            } else {
                scatter2(t1, go, B, sa.hout, sa.cin, st);
            }
            std::swap(g, go);
        }
    }
    if (mx) {
        mx_maxpool_bwd(h16(stash(0)), h16(g), h16(go), B, 112, 64, st);
    } else {
        maxpool_bwd(stash(0), g, go, B, 112, 64, st);
    }
    HIPE(lgate(0, go, true, false, sbig, &o0));
    return wgrad(0, mx ? f16(w.mx_padded) : images, o0.wg);  // conv1's weight gradient reads the images; mixed: the padded bf16 input
}

// dx of layer idx from its data-gradient operand, for the one-layer debug calls: a stride-2 layer's comes on the low-resolution map
int debug_data_grad(hpe_ctx* c, int idx, const float* dzs, int B, float* dx, hipStream_t st) {
    const ConvSpec& s = specs()[idx];
    if (s.stride == 1) {
        HIP_TRY(data_grad(c, idx, dzs, B, nullptr, dx, st));
    } else {
        HIP_TRY(data_grad(c, idx, dzs, B, nullptr, c->et.t0, st));
        scatter2(c->et.t0, dx, B, s.hout, s.cin, st);
        HIP_TRY(hipGetLastError());
    }
    return HPE_OK;
}

// what a call needs: nothing reserved yet, hpe_encoder_train_reserve, or hpe_encoder_train_reserve_batchnorm as well
enum Reserve { RESERVE_NONE, RESERVE_FROZEN, RESERVE_BN, RESERVE_MIXED, RESERVE_BN_MIXED };

int check_train(hpe_ctx* c, int B, Reserve need = RESERVE_FROZEN) {
    if (!c) return fail(HPE_ERR_INVALID, "null ctx");
    if (c->dead) return fail(HPE_ERR_STATE, "hpe_finalize failed on this ctx: destroy it and create a new one");
    if (!c->finalized) return fail(HPE_ERR_STATE, "hpe_finalize() has not been called");
    if (!c->have_encoder) return fail(HPE_ERR_STATE, "encoder weights were not loaded before hpe_finalize");
    if (c->bf16) return fail(HPE_ERR_STATE, "encoder training needs an fp32 context");
    if (need != RESERVE_NONE && c->et.B == 0) return fail(HPE_ERR_STATE, "hpe_encoder_train_reserve() has not been called");
    if (need == RESERVE_BN && c->et.bn_B == 0) return fail(HPE_ERR_STATE, "hpe_encoder_train_reserve_batchnorm() has not been called");
    if (need == RESERVE_MIXED && c->et.mx_B == 0) return fail(HPE_ERR_STATE, "hpe_encoder_train_reserve_mixed() has not been called");
    if (need == RESERVE_BN_MIXED && c->et.mxbn_B == 0)
        return fail(HPE_ERR_STATE, "hpe_encoder_train_reserve_batchnorm_mixed() has not been called");
    static const char* const range[] = {"max_batch", "reserved batch", "batch of the batch-norm reserve", "batch of the mixed-precision reserve",
                                        "batch of the mixed-precision batch-norm reserve"};
    const int top = need == RESERVE_NONE     ? c->cfg.max_batch
                    : need == RESERVE_FROZEN ? c->et.B
                    : need == RESERVE_BN     ? c->et.bn_B
                    : need == RESERVE_MIXED  ? c->et.mx_B
                                             : c->et.mxbn_B;
    if (B < 1 || B > top) return fail(HPE_ERR_INVALID, "batch " + std::to_string(B) + " outside [1, " + range[need] + "]");
    return HPE_OK;
}

// before a walk's first launch: no hook failure on record and, with the reduce hook set, what a batch-statistics walk needs: B within
// the batch of all ranks, no capture
int check_reduce(hpe_ctx* c, bool bn, int B, hipStream_t st) {
    c->et.reduce_failed = -1;
    if (!bn || !c->et.reduce) return HPE_OK;
    if (B > c->et.reduce_G)
        return fail(HPE_ERR_INVALID, "batch " + std::to_string(B) + " above the global batch " + std::to_string(c->et.reduce_G) + " of hpe_encoder_set_reduce");
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    HIP_TRY(hipStreamIsCapturing(st, &cap));
    if (cap != hipStreamCaptureStatusNone) return fail(HPE_ERR_STATE, "the stream is being captured and a reduce hook is set: the hook is host code");
    return HPE_OK;
}

// the result of a walk: a hook failure (named by its layer) before any HIP error
int walk_result(hpe_ctx* c, hipError_t e, const char* what) {
    if (c->et.reduce_failed >= 0)
        return fail(HPE_ERR_REDUCE, std::string("the reduce hook failed in the ") + what + " at layer " + std::to_string(c->et.reduce_failed) + " (" +
                                        specs()[c->et.reduce_failed].name + ")");
    HIP_TRY(e);
    return HPE_OK;
}

void walk_done(hpe_ctx* c, Walk wk, int B) {
    if (walk_mx(wk)) {  // the mixed stash has its own batch counter: the fp32 stash is as it was
        c->et.mx_stash_B = B;
        if (wk == WALK_MIXED) return;
        c->et.mx_zstash_B = B;
    } else {
        c->et.stash_B = B;
        if (wk != WALK_BATCH) return;
    }
    // the statistics in bn_batch are those of the last batch-statistics walk of either precision
    c->et.bn_stat_mixed = walk_mx(wk);
    c->et.bn_stat_B = B;
    c->et.bn_stat_G = c->et.reduce ? c->et.reduce_G : B;
}

Reserve reserve_of(Walk wk) {
    return wk == WALK_BATCH ? RESERVE_BN : wk == WALK_MIXED ? RESERVE_MIXED : wk == WALK_MIXED_BATCH ? RESERVE_BN_MIXED : RESERVE_FROZEN;
}

// hpe_encoder_forward_train / _batchnorm / _mixed / _batchnorm_mixed and hpe_encoder_backward / _batchnorm / _mixed / _batchnorm_mixed
int forward_entry(hpe_ctx* c, Walk wk, const float* images, int B, float* features, void* stream) {
    int rc = check_train(c, B, reserve_of(wk));
    if (rc) return rc;
    if (!images || !features) return fail(HPE_ERR_INVALID, "null pointer");
    DeviceGuard g(c->cfg.device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if ((rc = check_reduce(c, walk_bn(wk), B, st))) return rc;
    if ((rc = walk_result(c, forward_train(c, wk, images, B, features, st), "forward"))) return rc;
    walk_done(c, wk, B);
    return HPE_OK;
}

int backward_entry(hpe_ctx* c, Walk wk, const float* images, int B, const float* grad_features, float* grad_flat, void* stream) {
    int rc = check_train(c, B, reserve_of(wk));
    if (rc) return rc;
    if (!images || !grad_features || !grad_flat) return fail(HPE_ERR_INVALID, "null pointer");
    DeviceGuard g(c->cfg.device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if ((rc = check_reduce(c, walk_bn(wk), B, st))) return rc;
    if ((rc = walk_result(c, backward(c, wk, images, B, grad_features, grad_flat, st), "backward"))) return rc;
    walk_done(c, wk, B);
    return HPE_OK;
}

// host flat -> the data-gradient packings and the flat device copy (buffers exist)
int upload_train_params(hpe_ctx* c, const float* flat) {
    const EncLayout& l = layout();
    std::vector<float> dx;
    for (int i = 1; i < HPE_NUM_CONV; ++i) {
        pack_dx_weights(i, flat + l.off[i][0], dx);
        HIP_TRY(hipMemcpy(c->et.dxw[i], dx.data(), dx.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    HIP_TRY(hipMemcpy(c->et.flat, flat, (size_t)l.total * sizeof(float), hipMemcpyHostToDevice));
    return HPE_OK;
}

// what the four half-layer debug calls check: M, where they take one, is the rows of all parts
int debug_bn_check(hpe_ctx* c, int idx, int B, long long M, bool with_m) {
    int rc = check_train(c, B, RESERVE_BN);
    if (rc) return rc;
    if (idx < 0 || idx >= HPE_NUM_CONV) return fail(HPE_ERR_INVALID, "bad argument");
    const long long local = (long long)B * specs()[idx].hout * specs()[idx].hout;
    if (with_m && (M < local || M > 0x7fffffffLL / 2)) return fail(HPE_ERR_INVALID, "M below the rows given, or too large");
    return HPE_OK;
}

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

int hpe_encoder_param_floats(void) { return layout().total; }

int hpe_encoder_param_offset(int idx, int which) {
    if (idx < 0 || idx >= HPE_NUM_CONV || which < 0 || which > 3) return -1;
    return layout().off[idx][which];
}

long long hpe_encoder_train_ws_floats(int B) { return B < 1 ? 0 : (long long)ws_floats(B, false); }

int hpe_encoder_wg_slices(int idx, int B) {
    if (idx < 0 || idx >= HPE_NUM_CONV || B < 1) return -1;
    int P, sl;
    wg_slicing(idx, B, &P, &sl);
    return sl;
}

int hpe_encoder_train_reserve(hpe_ctx* c, int B) {
    int rc = check_train(c, B, RESERVE_NONE);
    if (rc) return rc;
    EncTrainWork& w = c->et;
    if (w.B != 0) return B <= w.B ? HPE_OK : fail(HPE_ERR_STATE, "hpe_encoder_train_reserve: already reserved for a smaller batch");
    DeviceGuard g(c->cfg.device);
    const EncLayout& l = layout();
    TrainAlloc alloc{c};
    train_buffers(w, B, alloc);
    if (alloc.rc) return alloc.rc;
    w.partial_floats = wg_partial_floats(B);
    // the flat parameters: hpe_finalize released the host kernels, so they come back from the packed device weights Wt[n][k] (fp32: exact)
    std::vector<float> flat(l.total), mean(l.channels), istd(l.channels), wt;
    std::vector<double> sd(l.channels);
    HIP_TRY(hipDeviceSynchronize());
    for (int i = 0; i < HPE_NUM_CONV; ++i) {
        const ConvSpec& s = specs()[i];
        const ConvLayer& L = c->conv[i];
        wt.resize((size_t)L.n_pad * L.k_pad);
        HIP_TRY(hipMemcpy(wt.data(), L.w, wt.size() * sizeof(float), hipMemcpyDeviceToHost));
        for (int kh = 0; kh < s.kh; ++kh)
            for (int kw = 0; kw < s.kw; ++kw)
                for (int ci = 0; ci < s.cin; ++ci) {
                    const int k = conv_wt_k(i, kh, kw, ci);
                    float* dst = &flat[l.off[i][0] + (((size_t)kh * s.kw + kw) * s.cin + ci) * s.cout];
                    for (int n = 0; n < s.cout; ++n) dst[n] = wt[(size_t)n * L.k_pad + k];
                }
        for (int n = 0; n < s.cout; ++n) {
            flat[l.off[i][1] + n] = L.bias[n];
            flat[l.off[i][2] + n] = L.gamma[n];
            flat[l.off[i][3] + n] = L.beta[n];
            mean[l.stat[i] + n] = L.mean[n];
            istd[l.stat[i] + n] = bn_istd(L, n, c->cfg.bn_eps);
            sd[l.stat[i] + n] = bn_sd(L, n, c->cfg.bn_eps);
        }
    }
    HIP_TRY(hipMemcpy(w.mean, mean.data(), mean.size() * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(w.istd, istd.data(), istd.size() * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(w.sd, sd.data(), sd.size() * sizeof(double), hipMemcpyHostToDevice));
    if ((rc = upload_train_params(c, flat.data()))) return rc;
    if ((rc = encoder_repack_reserve(c))) return rc;
    w.B = B;
    return HPE_OK;
}

int hpe_encoder_forward_train(hpe_ctx* c, const float* images, int B, float* features, void* stream) {
    return forward_entry(c, WALK_FROZEN, images, B, features, stream);
}

int hpe_encoder_backward(hpe_ctx* c, const float* images, int B, const float* grad_features, float* grad_flat, void* stream) {
    return backward_entry(c, WALK_FROZEN, images, B, grad_features, grad_flat, stream);
}

int hpe_encoder_get_params(hpe_ctx* c, float* flat, void* stream) {
    int rc = check_train(c, 1);
    if (rc) return rc;
    if (!flat) return fail(HPE_ERR_INVALID, "null flat_dev");
    DeviceGuard g(c->cfg.device);
    HIP_TRY(hipMemcpyAsync(flat, c->et.flat, (size_t)layout().total * sizeof(float), hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream)));
    return HPE_OK;
}

int hpe_encoder_set_params(hpe_ctx* c, const float* flat) {
    int rc = check_train(c, 1);
    if (rc) return rc;
    if (!flat) return fail(HPE_ERR_INVALID, "null flat_host");
    DeviceGuard g(c->cfg.device);
    const EncLayout& l = layout();
    HIP_TRY(hipDeviceSynchronize());  // launches still reading the weights
    if (c->et.bn_B) {  // hpe_encoder_set_stats_dev may have moved the statistics: the host packers fold what is installed
        std::vector<float> stats(2 * (size_t)l.channels);
        HIP_TRY(hipMemcpy(stats.data(), c->et.bn_stats, stats.size() * sizeof(float), hipMemcpyDeviceToHost));
        for (int i = 0; i < HPE_NUM_CONV; ++i) {
            const int n = specs()[i].cout;
            c->conv[i].mean.assign(stats.begin() + l.stat[i], stats.begin() + l.stat[i] + n);
            c->conv[i].var.assign(stats.begin() + l.channels + l.stat[i], stats.begin() + l.channels + l.stat[i] + n);
        }
    }
    for (int i = 0; i < HPE_NUM_CONV; ++i) {
        const ConvSpec& s = specs()[i];
        ConvLayer& L = c->conv[i];
        L.kernel.assign(flat + l.off[i][0], flat + l.off[i][1]);
        L.bias.assign(flat + l.off[i][1], flat + l.off[i][1] + s.cout);
        L.gamma.assign(flat + l.off[i][2], flat + l.off[i][2] + s.cout);
        L.beta.assign(flat + l.off[i][3], flat + l.off[i][3] + s.cout);
    }
    if ((rc = repack_encoder(c))) return rc;
    if ((rc = upload_train_params(c, flat))) return rc;
    HIP_TRY(hipDeviceSynchronize());
    return HPE_OK;
}

int hpe_encoder_set_params_dev(hpe_ctx* c, const float* flat, void* stream) {
    int rc = check_train(c, 1);
    if (rc) return rc;
    if (!flat) return fail(HPE_ERR_INVALID, "null flat_dev");
    DeviceGuard g(c->cfg.device);
    // Nothing to wait for here: encoder_impl has made the caller's stream wait for every chunk stream before it returned (the ev_join
    // loop at its end), so launches of earlier calls on `stream` are ordered before these; a pipelined tail reads no encoder weight.
    HIP_TRY(encoder_repack_launch(c, flat, static_cast<hipStream_t>(stream)));
    return HPE_OK;
}

int hpe_debug_conv_backward(hpe_ctx* c, int idx, const float* x, const float* y, const float* dy, int B, float* dx, float* grad_layer,
                            void* stream) {
    int rc = check_train(c, B);
    if (rc) return rc;
    if (idx < 0 || idx >= HPE_NUM_CONV || !x || !dy || !grad_layer) return fail(HPE_ERR_INVALID, "bad argument");
    if (idx == 0 && dx) return fail(HPE_ERR_INVALID, "hpe_debug_conv_backward: conv1 has no data gradient, dx_dev must be NULL");
    DeviceGuard g(c->cfg.device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const ConvSpec& s = specs()[idx];
    EncTrainWork& w = c->et;
    const long n = (long)B * s.hout * s.hout * s.cout;
    gate(dy, y, c->conv[idx].scale, w.g0, dx ? w.sbig : nullptr, n, s.cout, st);
    HIP_TRY(weight_grad(c, idx, x, w.g0, B, grad_layer, st));
    return dx ? debug_data_grad(c, idx, w.sbig, B, dx, st) : HPE_OK;
}

int hpe_debug_maxpool_backward(const float* x, const float* dy, int B, int H, int C, float* dx, void* stream) {
    if (!x || !dy || !dx || B < 1 || H < 2 || (H & 1) || C < 1) return fail(HPE_ERR_INVALID, "bad argument");
    maxpool_bwd(x, dy, dx, B, H, C, static_cast<hipStream_t>(stream));
    HIP_TRY(hipGetLastError());
    return HPE_OK;
}

int hpe_debug_avgpool_backward(const float* dy, int B, int HW, int C, float* dx, void* stream) {
    if (!dy || !dx || B < 1 || HW < 1 || C < 1) return fail(HPE_ERR_INVALID, "bad argument");
    avgpool_bwd(dy, dx, B, HW, C, static_cast<hipStream_t>(stream));
    HIP_TRY(hipGetLastError());
    return HPE_OK;
}

int hpe_debug_encoder_stash_batch(hpe_ctx* c) { return (c && c->finalized && !c->dead) ? c->et.stash_B : 0; }

int hpe_debug_encoder_stash(hpe_ctx* c, int idx, float* out, void* stream) {
    int rc = check_train(c, 1);
    if (rc) return rc;
    if (idx < -1 || idx >= HPE_NUM_CONV || !out) return fail(HPE_ERR_INVALID, "bad argument");
    const int B = c->et.stash_B;
    if (B == 0) return fail(HPE_ERR_STATE, "hpe_debug_encoder_stash: no training forward has run");
    DeviceGuard g(c->cfg.device);
    const size_t n = idx < 0 ? (size_t)POOL_FLOATS : (size_t)specs()[idx].hout * specs()[idx].hout * specs()[idx].cout;
    HIP_TRY(hipMemcpyAsync(out, stash_of(c, idx, B), (size_t)B * n * sizeof(float), hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream)));
    return HPE_OK;
}

// ---- BatchNorm with batch statistics

int hpe_encoder_stat_floats(void) { return 2 * layout().channels; }

int hpe_encoder_stat_offset(int idx, int which) {
    if (idx < 0 || idx >= HPE_NUM_CONV || which < 0 || which > 1) return -1;
    return which * layout().channels + layout().stat[idx];
}

long long hpe_encoder_train_ws_floats_batchnorm(int B) { return B < 1 ? 0 : (long long)ws_floats(B, true); }

int hpe_debug_encoder_bn_slices(int idx, int B) {
    if (idx < 0 || idx >= HPE_NUM_CONV || B < 1) return -1;
    return bn_slices(B * specs()[idx].hout * specs()[idx].hout, specs()[idx].cout);
}

int hpe_encoder_train_reserve_batchnorm(hpe_ctx* c, int B) {
    int rc = hpe_encoder_train_reserve(c, B);
    if (rc) return rc;
    EncTrainWork& w = c->et;
    if (w.bn_B != 0) return B <= w.bn_B ? HPE_OK : fail(HPE_ERR_STATE, "hpe_encoder_train_reserve_batchnorm: already reserved for a smaller batch");
    DeviceGuard g(c->cfg.device);
    const EncLayout& l = layout();
    TrainAlloc alloc{c};
    train_buffers_bn(w, B, alloc);
    if (alloc.rc) return alloc.rc;
    // the statistics as loaded (nothing can have moved them: hpe_encoder_set_stats_dev needs this reserve) and every channel's map size
    std::vector<float> stats(2 * (size_t)l.channels);
    std::vector<int> hw(l.channels);
    for (int i = 0; i < HPE_NUM_CONV; ++i) {
        const ConvSpec& s = specs()[i];
        for (int n = 0; n < s.cout; ++n) {
            stats[l.stat[i] + n] = c->conv[i].mean[n];
            stats[l.channels + l.stat[i] + n] = c->conv[i].var[n];
            hw[l.stat[i] + n] = s.hout * s.hout;
        }
    }
    HIP_TRY(hipMemcpy(w.bn_stats, stats.data(), stats.size() * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(w.bn_hw, hw.data(), hw.size() * sizeof(int), hipMemcpyHostToDevice));
    w.bn_B = B;
    return HPE_OK;
}

int hpe_encoder_forward_batchnorm(hpe_ctx* c, const float* images, int B, float* features, void* stream) {
    return forward_entry(c, WALK_BATCH, images, B, features, stream);
}

int hpe_encoder_backward_batchnorm(hpe_ctx* c, const float* images, int B, const float* grad_features, float* grad_flat, void* stream) {
    return backward_entry(c, WALK_BATCH, images, B, grad_features, grad_flat, stream);
}

int hpe_encoder_get_stats(hpe_ctx* c, float* stats, void* stream) {
    int rc = check_train(c, 1, RESERVE_BN);
    if (rc) return rc;
    if (!stats) return fail(HPE_ERR_INVALID, "null stats_dev");
    DeviceGuard g(c->cfg.device);
    HIP_TRY(hipMemcpyAsync(stats, c->et.bn_stats, 2 * (size_t)layout().channels * sizeof(float), hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream)));
    return HPE_OK;
}

int hpe_encoder_update_stats(hpe_ctx* c, float* stats, double momentum, int unbiased, void* stream) {
    int rc = check_train(c, 1, RESERVE_BN);
    if (rc) return rc;
    if (!stats) return fail(HPE_ERR_INVALID, "null stats_dev");
    if (!(momentum >= 0.0 && momentum <= 1.0)) return fail(HPE_ERR_INVALID, "momentum outside [0, 1]");
    if (c->et.bn_stat_B == 0) return fail(HPE_ERR_STATE, "hpe_encoder_update_stats: no batch-statistics forward has run");
    DeviceGuard g(c->cfg.device);
    HIP_TRY(bn_launch_momentum(stats, c->et.bn_batch, c->et.bn_hw, c->et.bn_stat_G, layout().channels, momentum, unbiased != 0,
                               static_cast<hipStream_t>(stream)));
    return HPE_OK;
}

int hpe_encoder_set_stats_dev(hpe_ctx* c, const float* stats, void* stream) {
    int rc = check_train(c, 1, RESERVE_BN);
    if (rc) return rc;
    if (!stats) return fail(HPE_ERR_INVALID, "null stats_dev");
    DeviceGuard g(c->cfg.device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    EncTrainWork& w = c->et;
    HIP_TRY(bn_launch_install(stats, layout().channels, c->cfg.bn_eps, w.bn_stats, w.mean, w.istd, w.sd, st));
    HIP_TRY(encoder_repack_stats_launch(c, st));
    return HPE_OK;
}

int hpe_debug_conv_batchnorm(hpe_ctx* c, int idx, const float* x, int B, const float* residual, int relu, float* y, float* z_out, float* stats_out,
                             void* stream) {
    int rc = check_train(c, B, RESERVE_BN);
    if (rc) return rc;
    if (idx < 0 || idx >= HPE_NUM_CONV || !x || !y || !z_out || !stats_out) return fail(HPE_ERR_INVALID, "bad argument");
    DeviceGuard g(c->cfg.device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const float* in = x;
    if (idx == 0) {
        HIP_TRY(hpe_launch_pad_input(x, c->padded, B, HPE_IMG_SIZE, HPE_IMG_SIZE, STEM_HP, STEM_WP, st));
        in = c->padded;
    }
    const BnSlots s = bn_slots(c, idx, true);
    HIP_TRY(layer_forward_bn(c, idx, in, B, residual, relu, z_out, y, s, st));
    const size_t n = (size_t)specs()[idx].cout * sizeof(float);
    HIP_TRY(hipMemcpyAsync(stats_out, s.mu, n, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(stats_out + specs()[idx].cout, s.var, n, hipMemcpyDeviceToDevice, st));
    return HPE_OK;
}

int hpe_debug_conv_backward_batchnorm(hpe_ctx* c, int idx, const float* x, const float* z, const float* y, const float* dy, int B, float* dx,
                                      float* grad_layer, void* stream) {
    int rc = check_train(c, B, RESERVE_BN);
    if (rc) return rc;
    if (idx < 0 || idx >= HPE_NUM_CONV || !x || !z || !dy || !grad_layer) return fail(HPE_ERR_INVALID, "bad argument");
    if (idx == 0 && dx) return fail(HPE_ERR_INVALID, "hpe_debug_conv_backward_batchnorm: conv1 has no data gradient, dx_dev must be NULL");
    DeviceGuard g(c->cfg.device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const ConvSpec& s = specs()[idx];
    EncTrainWork& w = c->et;
    const BnSlots sl = bn_slots(c, idx, true);
    HIP_TRY(bn_launch_stats(z, B * s.hout * s.hout, s.cout, c->cfg.bn_eps, w.bn_part, sl.mu, sl.var, sl.r, st));
    HIP_TRY(layer_gate_bn(c, idx, dy, y, z, B, sl, grad_layer, nullptr, w.sbig, st));
    HIP_TRY(weight_grad(c, idx, x, w.sbig, B, grad_layer, st, true));
    return dx ? debug_data_grad(c, idx, w.sbig, B, dx, st) : HPE_OK;
}

int hpe_debug_encoder_stash_raw(hpe_ctx* c, int idx, float* out, void* stream) {
    int rc = check_train(c, 1, RESERVE_BN);
    if (rc) return rc;
    if (idx < 0 || idx >= HPE_NUM_CONV || !out) return fail(HPE_ERR_INVALID, "bad argument");
    const int B = c->et.bn_stat_B;
    if (B == 0) return fail(HPE_ERR_STATE, "hpe_debug_encoder_stash_raw: no batch-statistics forward has run");
    if (c->et.bn_stat_mixed) return fail(HPE_ERR_STATE, "hpe_debug_encoder_stash_raw: the last batch-statistics forward was a mixed-precision one");
    if (c->et.stash_B != B) return fail(HPE_ERR_STATE, "hpe_debug_encoder_stash_raw: a frozen-statistics forward of another batch has refilled the stash since");
    DeviceGuard g(c->cfg.device);
    const size_t n = (size_t)specs()[idx].hout * specs()[idx].hout * specs()[idx].cout;
    HIP_TRY(hipMemcpyAsync(out, zstash_of(c, idx, B), (size_t)B * n * sizeof(float), hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream)));
    return HPE_OK;
}

int hpe_debug_encoder_batch_stats(hpe_ctx* c, float* out, void* stream) {
    int rc = check_train(c, 1, RESERVE_BN);
    if (rc) return rc;
    if (!out) return fail(HPE_ERR_INVALID, "null out_dev");
    if (c->et.bn_stat_B == 0) return fail(HPE_ERR_STATE, "hpe_debug_encoder_batch_stats: no batch-statistics forward has run");
    DeviceGuard g(c->cfg.device);
    HIP_TRY(hipMemcpyAsync(out, c->et.bn_batch, 2 * (size_t)layout().channels * sizeof(float), hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream)));
    return HPE_OK;
}

// ---- data-parallel training: the statistics over the batch of all ranks

int hpe_encoder_set_reduce(hpe_ctx* c, hpe_reduce_fn fn, void* user, int global_batch) {
    int rc = check_train(c, 1, RESERVE_BN);
    if (rc) return rc;
    if (fn && (global_batch < 1 || global_batch > 65536)) return fail(HPE_ERR_INVALID, "hpe_encoder_set_reduce: global batch outside [1, 65536]");
    c->et.reduce = fn;
    c->et.reduce_user = fn ? user : nullptr;
    c->et.reduce_G = fn ? global_batch : 0;
    return HPE_OK;
}

int hpe_debug_bn_sums(hpe_ctx* c, int idx, const float* z, int B, double* sums_out, void* stream) {
    int rc = debug_bn_check(c, idx, B, 0, false);
    if (rc) return rc;
    if (!z || !sums_out) return fail(HPE_ERR_INVALID, "null pointer");
    DeviceGuard g(c->cfg.device);
    const ConvSpec& s = specs()[idx];
    HIP_TRY(bn_launch_stats_sums(z, B * s.hout * s.hout, s.cout, c->et.bn_part, sums_out, static_cast<hipStream_t>(stream)));
    return HPE_OK;
}

int hpe_debug_bn_finish(hpe_ctx* c, int idx, const double* sums, long long M, const float* z, int B, const float* residual, int relu, float* y,
                        float* stats_out, void* stream) {
    int rc = debug_bn_check(c, idx, B, M, true);
    if (rc) return rc;
    if (!sums || !z || !y || !stats_out) return fail(HPE_ERR_INVALID, "null pointer");
    DeviceGuard g(c->cfg.device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const ConvSpec& s = specs()[idx];
    const EncLayout& l = layout();
    const BnSlots sl = bn_slots(c, idx, true);
    HIP_TRY(bn_launch_stats_from_sums(sums, (double)M, s.cout, c->cfg.bn_eps, sl.mu, sl.var, sl.r, st));
    HIP_TRY(bn_launch_apply(z, sl.mu, sl.r, c->et.flat + l.off[idx][2], c->et.flat + l.off[idx][3], residual, relu, y, B * s.hout * s.hout, s.cout, st));
    HIP_TRY(hipMemcpyAsync(stats_out, sl.mu, (size_t)s.cout * sizeof(float), hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(stats_out + s.cout, sl.var, (size_t)s.cout * sizeof(float), hipMemcpyDeviceToDevice, st));
    return HPE_OK;
}

int hpe_debug_bn_backward_sums(hpe_ctx* c, int idx, const float* z, const float* y, const float* dy, int B, const double* sums, long long M,
                               double* sums_out, void* stream) {
    int rc = debug_bn_check(c, idx, B, M, true);
    if (rc) return rc;
    if (!z || !dy || !sums || !sums_out) return fail(HPE_ERR_INVALID, "null pointer");
    DeviceGuard g(c->cfg.device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const ConvSpec& s = specs()[idx];
    const BnSlots sl = bn_slots(c, idx, true);
    float* local = reduce_grads(c);  // the rounded local sums, which nobody reads here: [db | dgamma | dbeta]
    HIP_TRY(bn_launch_stats_from_sums(sums, (double)M, s.cout, c->cfg.bn_eps, sl.mu, sl.var, sl.r, st));
    HIP_TRY(bn_launch_bwd_sums(dy, y, z, sl.mu, sl.r, B * s.hout * s.hout, s.cout, c->et.bn_part, sums_out, local, local + s.cout, local + 2 * s.cout, st));
    return HPE_OK;
}

int hpe_debug_bn_backward_finish(hpe_ctx* c, int idx, const float* x, const float* z, const float* y, const float* dy, int B, const double* sums,
                                 const double* bwd_sums, long long M, float* dx, float* grad_layer, void* stream) {
    int rc = debug_bn_check(c, idx, B, M, true);
    if (rc) return rc;
    if (!x || !z || !dy || !sums || !bwd_sums || !grad_layer) return fail(HPE_ERR_INVALID, "null pointer");
    if (idx == 0 && dx) return fail(HPE_ERR_INVALID, "hpe_debug_bn_backward_finish: conv1 has no data gradient, dx_dev must be NULL");
    DeviceGuard g(c->cfg.device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const ConvSpec& s = specs()[idx];
    EncTrainWork& w = c->et;
    const int rows = B * s.hout * s.hout, N = s.cout, kn = s.kh * s.kw * s.cin * N;
    const BnSlots sl = bn_slots(c, idx, true);
    float *db = grad_layer + kn, *dgamma = db + N, *dbeta = dgamma + N, *red = reduce_grads(c);
    HIP_TRY(bn_launch_stats_from_sums(sums, (double)M, N, c->cfg.bn_eps, sl.mu, sl.var, sl.r, st));
    HIP_TRY(bn_launch_bwd_sums(dy, y, z, sl.mu, sl.r, rows, N, w.bn_part, reduce_sums(c), db, dgamma, dbeta, st));
    HIP_TRY(bn_launch_bwd_from_sums(bwd_sums, N, red, st));
    HIP_TRY(bn_launch_bwd_apply(dy, y, z, sl.mu, sl.r, w.flat + layout().off[idx][2], red + N, red, rows, N, nullptr, w.sbig, st, (double)M));
    HIP_TRY(weight_grad(c, idx, x, w.sbig, B, grad_layer, st, true));
    return dx ? debug_data_grad(c, idx, w.sbig, B, dx, st) : HPE_OK;
}

// ---- mixed precision: bf16 walks on an fp32 context.  The bf16 weight operands are cast from the context's live fp32 weights
// (ConvLayer::w and dxw, which both setters keep current) by one launch at the start of every mixed call: no setter knows of them

long long hpe_encoder_train_ws_floats_mixed(int B) { return B < 1 ? 0 : (long long)ws_floats(B, false, true); }

int hpe_encoder_train_reserve_mixed(hpe_ctx* c, int B) {
    int rc = hpe_encoder_train_reserve(c, B);
    if (rc) return rc;
    EncTrainWork& w = c->et;
    if (w.mx_B != 0) return B <= w.mx_B ? HPE_OK : fail(HPE_ERR_STATE, "hpe_encoder_train_reserve_mixed: already reserved for a smaller batch");
    DeviceGuard g(c->cfg.device);
    TrainAlloc alloc{c};
    train_buffers_mixed(w, B, alloc);
    if (alloc.rc) return alloc.rc;
    std::vector<MxCastSeg> table(MX_CAST_SEGS);
    for (int i = 0; i < HPE_NUM_CONV; ++i) {
        const ConvLayer& L = c->conv[i];
        table[i] = {L.w, w.mx_w[i], L.k_pad, conv_k_pad(i, true), (long)L.n_pad * L.k_pad / 4};
        if (i == 0) continue;
        const int kd = specs()[i].kh * specs()[i].kw * specs()[i].cout;
        table[HPE_NUM_CONV - 1 + i] = {w.dxw[i], w.mx_dxw[i], kd, kd, (long)(conv_dxw_floats(i) / 4)};
    }
    HIP_TRY(hipMemcpy(w.mx_cast, table.data(), table.size() * sizeof(MxCastSeg), hipMemcpyHostToDevice));
    w.mx_B = B;
    return HPE_OK;
}

int hpe_encoder_forward_train_mixed(hpe_ctx* c, const float* images, int B, float* features, void* stream) {
    return forward_entry(c, WALK_MIXED, images, B, features, stream);
}

int hpe_encoder_backward_mixed(hpe_ctx* c, const float* images, int B, const float* grad_features, float* grad_flat, void* stream) {
    return backward_entry(c, WALK_MIXED, images, B, grad_features, grad_flat, stream);
}

int hpe_debug_conv_backward_mixed(hpe_ctx* c, int idx, const void* x, const void* y, const void* dy, int B, void* dx, float* grad_layer,
                                  void* stream) {
    int rc = check_train(c, B, RESERVE_MIXED);
    if (rc) return rc;
    if (idx < 0 || idx >= HPE_NUM_CONV || !x || !dy || !grad_layer) return fail(HPE_ERR_INVALID, "bad argument");
    if (idx == 0 && dx) return fail(HPE_ERR_INVALID, "hpe_debug_conv_backward_mixed: conv1 has no data gradient, dx_dev must be NULL");
    DeviceGuard g(c->cfg.device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const ConvSpec& s = specs()[idx];
    EncTrainWork& w = c->et;
    HIP_TRY(mx_cast_launch(c, idx, 1, st));
    if (idx > 0) HIP_TRY(mx_cast_launch(c, HPE_NUM_CONV - 1 + idx, 1, st));
    cmx16 in = static_cast<cmx16>(x);
    if (idx == 0) {  // x is the fp32 image tensor
        HIP_TRY(hpe_launch_pad_input_bf16(static_cast<const float*>(x), w.mx_padded, B, HPE_IMG_SIZE, HPE_IMG_SIZE, STEM_HP, STEM_WP, st));
        in = w.mx_padded;
    }
    const long n = (long)B * s.hout * s.hout * s.cout;
    mx_gate(static_cast<cmx16>(dy), static_cast<cmx16>(y), c->conv[idx].scale, w.mx_g0, dx ? w.mx_sbig : nullptr, n, s.cout, st);
    HIP_TRY(mx_weight_grad(c, idx, in, w.mx_g0, B, grad_layer, st));
    if (!dx) return HPE_OK;
    if (s.stride == 1) {
        HIP_TRY(mx_data_grad(c, idx, w.mx_sbig, B, nullptr, static_cast<mx16>(dx), st));
    } else {  // a stride-2 layer's data gradient comes on the low-resolution map
        HIP_TRY(mx_data_grad(c, idx, w.mx_sbig, B, nullptr, w.mx_t0, st));
        mx_scatter2(w.mx_t0, static_cast<mx16>(dx), B, s.hout, s.cin, st);
        HIP_TRY(hipGetLastError());
    }
    return HPE_OK;
}

int hpe_debug_maxpool_backward_mixed(const void* x, const void* dy, int B, int H, int C, void* dx, void* stream) {
    if (!x || !dy || !dx || B < 1 || H < 2 || (H & 1) || C < 8 || (C & 7)) return fail(HPE_ERR_INVALID, "bad argument");
    mx_maxpool_bwd(static_cast<cmx16>(x), static_cast<cmx16>(dy), static_cast<mx16>(dx), B, H, C, static_cast<hipStream_t>(stream));
    HIP_TRY(hipGetLastError());
    return HPE_OK;
}

int hpe_debug_avgpool_backward_mixed(const float* dy, int B, int HW, int C, void* dx, void* stream) {
    if (!dy || !dx || B < 1 || HW < 1 || C < 8 || (C & 7)) return fail(HPE_ERR_INVALID, "bad argument");
    mx_avgpool_bwd(dy, static_cast<mx16>(dx), B, HW, C, static_cast<hipStream_t>(stream));
    HIP_TRY(hipGetLastError());
    return HPE_OK;
}

int hpe_debug_encoder_stash_batch_mixed(hpe_ctx* c) { return (c && c->finalized && !c->dead) ? c->et.mx_stash_B : 0; }

int hpe_debug_encoder_stash_mixed(hpe_ctx* c, int idx, void* out, void* stream) {
    int rc = check_train(c, 1, RESERVE_MIXED);
    if (rc) return rc;
    if (idx < -1 || idx >= HPE_NUM_CONV || !out) return fail(HPE_ERR_INVALID, "bad argument");
    const int B = c->et.mx_stash_B;
    if (B == 0) return fail(HPE_ERR_STATE, "hpe_debug_encoder_stash_mixed: no mixed-precision forward has run");
    DeviceGuard g(c->cfg.device);
    const size_t n = idx < 0 ? (size_t)POOL_FLOATS : (size_t)specs()[idx].hout * specs()[idx].hout * specs()[idx].cout;
    HIP_TRY(hipMemcpyAsync(out, stash_of(c, WALK_MIXED, idx, B), (size_t)B * n * sizeof(unsigned short), hipMemcpyDeviceToDevice,
                           static_cast<hipStream_t>(stream)));
    return HPE_OK;
}

// ---- mixed precision with batch statistics (encoder_bn_bf16.hip holds the kernels): both reserves and a bf16 raw-output stash

long long hpe_encoder_train_ws_floats_batchnorm_mixed(int B) { return B < 1 ? 0 : (long long)ws_floats(B, true, true, true); }

int hpe_encoder_train_reserve_batchnorm_mixed(hpe_ctx* c, int B) {
    int rc = hpe_encoder_train_reserve_mixed(c, B);
    if (rc) return rc;
    if ((rc = hpe_encoder_train_reserve_batchnorm(c, B))) return rc;
    EncTrainWork& w = c->et;
    if (w.mxbn_B != 0)
        return B <= w.mxbn_B ? HPE_OK : fail(HPE_ERR_STATE, "hpe_encoder_train_reserve_batchnorm_mixed: already reserved for a smaller batch");
    DeviceGuard g(c->cfg.device);
    TrainAlloc alloc{c};
    train_buffers_bn_mixed(w, B, alloc);
    if (alloc.rc) return alloc.rc;
    w.mxbn_B = B;
    return HPE_OK;
}

int hpe_encoder_forward_batchnorm_mixed(hpe_ctx* c, const float* images, int B, float* features, void* stream) {
    return forward_entry(c, WALK_MIXED_BATCH, images, B, features, stream);
}

int hpe_encoder_backward_batchnorm_mixed(hpe_ctx* c, const float* images, int B, const float* grad_features, float* grad_flat, void* stream) {
    return backward_entry(c, WALK_MIXED_BATCH, images, B, grad_features, grad_flat, stream);
}

int hpe_debug_conv_batchnorm_mixed(hpe_ctx* c, int idx, const void* x, int B, const void* residual, int relu, void* y, void* z_out, float* stats_out,
                                   void* stream) {
    int rc = check_train(c, B, RESERVE_BN_MIXED);
    if (rc) return rc;
    if (idx < 0 || idx >= HPE_NUM_CONV || !x || !y || !z_out || !stats_out) return fail(HPE_ERR_INVALID, "bad argument");
    DeviceGuard g(c->cfg.device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    EncTrainWork& w = c->et;
    HIP_TRY(mx_cast_launch(c, idx, 1, st));
    cmx16 in = static_cast<cmx16>(x);
    if (idx == 0) {  // x is the fp32 image tensor
        HIP_TRY(hpe_launch_pad_input_bf16(static_cast<const float*>(x), w.mx_padded, B, HPE_IMG_SIZE, HPE_IMG_SIZE, STEM_HP, STEM_WP, st));
        in = w.mx_padded;
    }
    const BnSlots s = bn_slots(c, idx, true);
    HIP_TRY(layer_forward_bn16(c, idx, in, B, static_cast<cmx16>(residual), relu, static_cast<mx16>(z_out), static_cast<mx16>(y), s, st));
    const size_t n = (size_t)specs()[idx].cout * sizeof(float);
    HIP_TRY(hipMemcpyAsync(stats_out, s.mu, n, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(stats_out + specs()[idx].cout, s.var, n, hipMemcpyDeviceToDevice, st));
    return HPE_OK;
}

int hpe_debug_conv_backward_batchnorm_mixed(hpe_ctx* c, int idx, const void* x, const void* z, const void* y, const void* dy, int B, void* dx,
                                            float* grad_layer, void* stream) {
    int rc = check_train(c, B, RESERVE_BN_MIXED);
    if (rc) return rc;
    if (idx < 0 || idx >= HPE_NUM_CONV || !x || !z || !dy || !grad_layer) return fail(HPE_ERR_INVALID, "bad argument");
    if (idx == 0 && dx) return fail(HPE_ERR_INVALID, "hpe_debug_conv_backward_batchnorm_mixed: conv1 has no data gradient, dx_dev must be NULL");
    DeviceGuard g(c->cfg.device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const ConvSpec& s = specs()[idx];
    EncTrainWork& w = c->et;
    HIP_TRY(mx_cast_launch(c, idx, 1, st));
    if (idx > 0) HIP_TRY(mx_cast_launch(c, HPE_NUM_CONV - 1 + idx, 1, st));
    cmx16 in = static_cast<cmx16>(x);
    if (idx == 0) {  // x is the fp32 image tensor
        HIP_TRY(hpe_launch_pad_input_bf16(static_cast<const float*>(x), w.mx_padded, B, HPE_IMG_SIZE, HPE_IMG_SIZE, STEM_HP, STEM_WP, st));
        in = w.mx_padded;
    }
    const BnSlots sl = bn_slots(c, idx, true);
    cmx16 z16 = static_cast<cmx16>(z);
    HIP_TRY(bn16_launch_stats(z16, B * s.hout * s.hout, s.cout, c->cfg.bn_eps, w.bn_part, sl.mu, sl.var, sl.r, st));
    HIP_TRY(layer_gate_bn16(c, idx, static_cast<cmx16>(dy), static_cast<cmx16>(y), z16, B, sl, grad_layer, nullptr, w.mx_sbig, st));
    HIP_TRY(mx_weight_grad(c, idx, in, w.mx_sbig, B, grad_layer, st, true));
    if (!dx) return HPE_OK;
    if (s.stride == 1) {
        HIP_TRY(mx_data_grad(c, idx, w.mx_sbig, B, nullptr, static_cast<mx16>(dx), st));
    } else {  // a stride-2 layer's data gradient comes on the low-resolution map
        HIP_TRY(mx_data_grad(c, idx, w.mx_sbig, B, nullptr, w.mx_t0, st));
        mx_scatter2(w.mx_t0, static_cast<mx16>(dx), B, s.hout, s.cin, st);
        HIP_TRY(hipGetLastError());
    }
    return HPE_OK;
}

int hpe_debug_encoder_stash_raw_mixed(hpe_ctx* c, int idx, void* out, void* stream) {
    int rc = check_train(c, 1, RESERVE_BN_MIXED);
    if (rc) return rc;
    if (idx < 0 || idx >= HPE_NUM_CONV || !out) return fail(HPE_ERR_INVALID, "bad argument");
    const int B = c->et.mx_zstash_B;
    if (B == 0) return fail(HPE_ERR_STATE, "hpe_debug_encoder_stash_raw_mixed: no mixed-precision batch-statistics forward has run");
    if (c->et.mx_stash_B != B)
        return fail(HPE_ERR_STATE, "hpe_debug_encoder_stash_raw_mixed: a frozen-statistics mixed forward of another batch has refilled the stash since");
    DeviceGuard g(c->cfg.device);
    const size_t n = (size_t)specs()[idx].hout * specs()[idx].hout * specs()[idx].cout;
    HIP_TRY(hipMemcpyAsync(out, mx_zstash_of(c, idx, B), (size_t)B * n * sizeof(unsigned short), hipMemcpyDeviceToDevice,
                           static_cast<hipStream_t>(stream)));
    return HPE_OK;
}

}  // extern "C"
#pragma GCC visibility pop
