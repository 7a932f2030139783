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
// batch statistics, encoder_bn_bf16.hip; each launcher is an overload on the element type of its tensors (float, or bf16e for bf16).
// This file holds the layout, the reserves, the two walks and the C ABI.  The walks (one forward, one backward) are templates on that
// element type and take the BatchNorm mode as a per-layer choice; Prec<T> states the few steps in which the precisions really differ.
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

// The activation buffers of one precision at batch B, in allocation order, as f(member, floats, zero-filled); a bf16 element is half a
// float (every count is even).  zstash is not among them: the batch-statistics reserves add it
template <class T, class F>
void act_buffers(EncActs<T>& a, int B, F&& f) {
    const size_t nb = (size_t)B * sizeof(T);
    f(a.stash, nb * layout().stash_per_image / sizeof(float), false);
    f(a.g0, nb * BIG / sizeof(float), false);
    f(a.g1, nb * BIG / sizeof(float), false);
    f(a.sbig, nb * BIG / sizeof(float), false);
    f(a.t0, nb * MID / sizeof(float), false);
    f(a.t1, nb * MID / sizeof(float), false);
    f(a.ssmall, nb * MID / sizeof(float), false);
}
template <class T, class F>
void zstash_buffer(EncActs<T>& a, int B, F&& f) {
    f(a.zstash, (size_t)B * sizeof(T) * layout().stash_pool / sizeof(float), false);
}

// Every buffer of a reserve at batch B, in allocation order, through the same f: the reserve allocates through this and
// hpe_encoder_train_ws_floats* add it up.  RESERVE_BN and RESERVE_MIXED build on RESERVE_FROZEN, RESERVE_BN_MIXED on both
enum Reserve { RESERVE_NONE, RESERVE_FROZEN, RESERVE_BN, RESERVE_MIXED, RESERVE_BN_MIXED };
constexpr size_t PADDED16 = (size_t)STEM_HP * STEM_WP * 4;  // the padded bf16 input, per image
template <class F>
void train_buffers(EncTrainWork& w, Reserve r, int B, F&& f) {
    const EncLayout& l = layout();
    const size_t nb = (size_t)B;
    switch (r) {
    case RESERVE_NONE:
        break;
    case RESERVE_FROZEN:
        act_buffers(w.f32, B, f);
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
        break;
    case RESERVE_BN:
        zstash_buffer(w.f32, B, f);
        f(w.bn_batch, 3 * (size_t)l.channels + 3 * 2048, true);
        f(w.bn_stats, 2 * (size_t)l.channels, false);
        f(w.bn_part, 4 * (size_t)BN_PART_COLS, false);  // 2 * BN_PART_COLS doubles
        f(w.bn_hw, l.channels, false);
        break;
    case RESERVE_MIXED:  // the weight operands are zeroed: the cast that opens a mixed call never writes their k padding
        act_buffers(w.b16, B, f);
        f(w.mx_padded, nb * PADDED16 / 2, false);
        for (int i = 0; i < HPE_NUM_CONV; ++i) f(w.mx_w[i], (size_t)round_up(specs()[i].cout, 128) * conv_k_pad(i, true) / 2, true);
        for (int i = 1; i < HPE_NUM_CONV; ++i) f(w.mx_dxw[i], conv_dxw_floats(i) / 2, false);
        f(w.mx_cast, (size_t)MX_CAST_SEGS * sizeof(MxCastSeg) / sizeof(float), false);
        break;
    case RESERVE_BN_MIXED:
        zstash_buffer(w.b16, B, f);
        break;
    }
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
    train_buffers(w, RESERVE_FROZEN, B, add);
    if (bn) train_buffers(w, RESERVE_BN, B, add);
    if (mixed) train_buffers(w, RESERVE_MIXED, B, add);
    if (bn_mixed) train_buffers(w, RESERVE_BN_MIXED, B, add);
    return n;
}

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

// What differs between the two precisions of a walk, each stated once.  T = float: the fp32 walks; T = bf16e: the mixed ones, whose
// weight operands are cast from the live fp32 weights by the launch that opens every mixed call
template <class T>
struct Prec;
template <>
struct Prec<float> {
    static constexpr bool mixed = false;
    static constexpr const char* suffix = "";
    static constexpr Reserve reserve(bool bn) { return bn ? RESERVE_BN : RESERVE_FROZEN; }
    static hipError_t cast(hpe_ctx*, int, int, hipStream_t) { return hipSuccess; }  // the fp32 weights are the operands
    static float* padded(hpe_ctx* c) { return c->padded; }                          // conv1's input
    // what conv1's weight gradient reads: the images themselves, with pad = (kh - 1) / 2
    static constexpr bool wg0_padded = false;
    static const float* wg0_input(hpe_ctx*, const float* images) { return images; }
    static void done(EncTrainWork& w, int B, bool) { w.stash_B = B; }
    // the batch whose activations / raw outputs the stash / zstash holds for the debug calls, or 0 and why not
    static int stash_batch(const EncTrainWork& w, const char** why) {
        *why = "no training forward has run";
        return w.stash_B;
    }
    static int zstash_batch(const EncTrainWork& w, const char** why) {
        *why = w.bn_stat_B == 0   ? "no batch-statistics forward has run"
               : w.bn_stat_mixed ? "the last batch-statistics forward was a mixed-precision one"
                                 : "a frozen-statistics forward of another batch has refilled the stash since";
        return w.bn_stat_mixed || w.stash_B != w.bn_stat_B ? 0 : w.bn_stat_B;
    }
};
template <>
struct Prec<bf16e> {
    static constexpr bool mixed = true;
    static constexpr const char* suffix = "_mixed";
    static constexpr Reserve reserve(bool bn) { return bn ? RESERVE_BN_MIXED : RESERVE_MIXED; }
    static hipError_t cast(hpe_ctx* c, int first, int segs, hipStream_t st) { return mx_cast_launch(c, first, segs, st); }
    static bf16e* padded(hpe_ctx* c) { return c->et.mx_padded; }
    // ... the padded bf16 input
    static constexpr bool wg0_padded = true;
    static const bf16e* wg0_input(hpe_ctx* c, const float*) { return c->et.mx_padded; }
    // the mixed stash has its own batch counters: the fp32 stash is as it was
    static void done(EncTrainWork& w, int B, bool bn) {
        w.mx_stash_B = B;
        if (bn) w.mx_zstash_B = B;
    }
    static int stash_batch(const EncTrainWork& w, const char** why) {
        *why = "no mixed-precision forward has run";
        return w.mx_stash_B;
    }
    static int zstash_batch(const EncTrainWork& w, const char** why) {
        *why = w.mx_zstash_B == 0 ? "no mixed-precision batch-statistics forward has run"
                                  : "a frozen-statistics mixed forward of another batch has refilled the stash since";
        return w.mx_stash_B != w.mx_zstash_B ? 0 : w.mx_zstash_B;
    }
};

template <class T>
T* stash_of(hpe_ctx* c, int idx, int B) {
    const EncLayout& l = layout();
    return c->et.acts<T>().stash + (size_t)B * (idx < 0 ? l.stash_pool : l.stash[idx]);
}

template <class T>
hipError_t pad_images(hpe_ctx* c, const float* images, int B, hipStream_t st) {
    return enc_pad_input(images, Prec<T>::padded(c), B, HPE_IMG_SIZE, HPE_IMG_SIZE, STEM_HP, STEM_WP, st);
}

// ---- BatchNorm with batch statistics (encoder_bn.hip / encoder_bn_bf16.hip hold the kernels): z kept beside y, the layer's statistics
// in its slots

template <class T>
T* zstash_of(hpe_ctx* c, int idx, int B) {
    return c->et.acts<T>().zstash + (size_t)B * layout().stash[idx];
}

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
// Mixed: z and y are rounded to bf16 where they are written, and the statistics are those OF the rounded z.
// reduce: the statistics of all ranks' rows (the hook is set).  Only the first-stage kernels differ between the precisions: the hook
// sees the same sums at the same place
template <class T>
hipError_t layer_forward_bn(hpe_ctx* c, int idx, const T* x, int B, const T* res, int relu, T* z, T* y, const BnSlots& s, hipStream_t st,
                            bool reduce = false) {
    const ConvSpec& sp = specs()[idx];
    const EncLayout& l = layout();
    const float* flat = c->et.flat;
    const int M = B * sp.hout * sp.hout;
    HIPE(layer_conv(c, idx, x, B, nullptr, 0, z, st, c->ones, flat + l.off[idx][1]));
    if (reduce) {
        HIPE(bn_launch_stats_sums(z, M, sp.cout, c->et.bn_part, reduce_sums(c), st));
        HIPE(reduce_call(c, idx, 2LL * sp.cout, st));
        HIPE(bn_launch_stats_from_sums(reduce_sums(c), rows_all(c, idx), sp.cout, c->cfg.bn_eps, s.mu, s.var, s.r, st));
    } else {
        HIPE(bn_launch_stats(z, M, sp.cout, c->cfg.bn_eps, c->et.bn_part, s.mu, s.var, s.r, st));
    }
    return bn_launch_apply(z, s.mu, s.r, flat + l.off[idx][2], flat + l.off[idx][3], res, relu, y, M, sp.cout, st);
}

// the gate and the BatchNorm backward of layer idx: db (= 0), dgamma, dbeta (fp32) into grad_layer; dz (exact in bf16 too; may be nullptr,
// may alias dy) and dzraw.  reduce: grad_layer keeps this rank's partial sums, dzraw is that of the batch of all ranks (the hook is set)
template <class T>
hipError_t layer_gate_bn(hpe_ctx* c, int idx, const T* dy, const T* y, const T* z, int B, const BnSlots& s, float* grad_layer, T* dz, T* dzraw,
                         hipStream_t st, bool reduce = false) {
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

// The training forward at the precision T, every activation kept in the stash.  bn (batch statistics): z kept beside y, the statistics
// in the layers' slots
template <class T>
hipError_t forward_train(hpe_ctx* c, bool bn, const float* images, int B, float* features, hipStream_t st) {
    const bool reduce = bn && c->et.reduce != nullptr;
    auto stash = [&](int idx) { return stash_of<T>(c, idx, B); };
    auto layer = [&](int idx, const T* x, const T* res, int relu) {
        T* y = stash(idx);
        return bn ? layer_forward_bn<T>(c, idx, x, B, res, relu, zstash_of<T>(c, idx, B), y, bn_slots(c, idx, false), st, reduce)
                  : layer_conv(c, idx, x, B, res, relu, y, st);
    };
    HIPE(Prec<T>::cast(c, 0, MX_CAST_SEGS, st));
    HIPE(pad_images<T>(c, images, B, st));
    HIPE(layer(0, Prec<T>::padded(c), nullptr, 1));
    HIPE(enc_maxpool(stash(0), stash(-1), B, 112, 64, st));
    for (const ResBlock& blk : blocks()) {
        const T* cur = stash(blk.in);
        HIPE(layer(blk.i2a, cur, nullptr, 1));
        HIPE(layer(blk.i2b, stash(blk.i2a), nullptr, 1));
        const T* res = cur;
        if (blk.first) {
            HIPE(layer(blk.i1, cur, nullptr, 0));
            res = stash(blk.i1);
        }
        HIPE(layer(blk.i2c, stash(blk.i2b), res, 1));
    }
    return enc_avgpool(stash(blocks().back().i2c), features, B, 49, HPE_FEATURE_DIM, HPE_FEATURE_DIM, st);
}

template <class T>
struct GateOut {
    const T *wg, *dg;  // what the layer's weight gradient and its data gradient read
};

// The cotangent dy of layer idx's output -> that of its convolution.  gated: the layer has a ReLU; keep: dy's buffer must hold dz
// afterwards (branch2c: it is the shortcut's cotangent too); copy: receives the data-gradient operand.
//   frozen  dz in place where there is a ReLU (without one dz is dy), copy = dz * s (none for conv1, which has no data gradient; bf16:
//           rounded to nearest even); the weight gradient reads dz
//   batch   the bias / gamma / beta gradients (fp32) go into grad_flat, copy = dzraw, which both gradients read; dz is written only if kept
template <class T>
hipError_t layer_gate(hpe_ctx* c, bool bn, int idx, T* dy, bool gated, bool keep, T* copy, int B, float* grad_flat, hipStream_t st, GateOut<T>* o) {
    const ConvSpec& s = specs()[idx];
    const T* y = gated ? stash_of<T>(c, idx, B) : nullptr;
    if (bn) {
        *o = {copy, copy};
        return layer_gate_bn<T>(c, idx, dy, y, zstash_of<T>(c, idx, B), B, bn_slots(c, idx, false), grad_flat + layout().off[idx][0],
                                keep ? dy : nullptr, copy, st, c->et.reduce != nullptr);
    }
    T* dzs = idx == 0 ? nullptr : copy;
    gate(dy, y, dzs ? c->conv[idx].scale : nullptr, gated ? dy : nullptr, dzs, (long)B * s.hout * s.hout * s.cout, s.cout, st);
    *o = {dy, dzs};
    return hipSuccess;
}

template <class T>
hipError_t backward(hpe_ctx* c, bool bn, const float* images, int B, const float* grad_features, float* grad_flat, hipStream_t st) {
    EncActs<T>& a = c->et.acts<T>();
    HIPE(forward_train<T>(c, bn, images, B, c->et.feat, st));
    auto stash = [&](int idx) { return stash_of<T>(c, idx, B); };
    auto lgate = [&](int idx, T* dy, bool gated, bool keep, T* copy, GateOut<T>* o) {
        return layer_gate<T>(c, bn, idx, dy, gated, keep, copy, B, grad_flat, st, o);
    };
    auto wgrad = [&](int idx, const T* x, const T* dz) { return weight_grad(c, idx, x, dz, B, grad_flat + layout().off[idx][0], st, bn); };
    auto dgrad = [&](int idx, const T* dzs, const T* res, T* out) { return data_grad(c, idx, dzs, B, res, out, st); };
    GateOut<T> o2c, o2b, o2a, o1, o0;
    T *g = a.g0, *go = a.g1;
    avgpool_bwd(grad_features, g, B, 49, HPE_FEATURE_DIM, st);
    for (auto it = blocks().rbegin(); it != blocks().rend(); ++it) {
        const int i2a = it->i2a, i2b = it->i2b, i2c = it->i2c, i1 = it->i1;
        const ConvSpec& sa = specs()[i2a];
        const T* xin = stash(it->in);  // the block's input: the previous block's branch2c output
        // branch2c: g becomes dz (the cotangent of the shortcut too)
        HIPE(lgate(i2c, g, true, true, a.sbig, &o2c));
        HIPE(wgrad(i2c, stash(i2b), o2c.wg));
        HIPE(dgrad(i2c, o2c.dg, nullptr, a.t0));
        HIPE(lgate(i2b, a.t0, true, false, a.ssmall, &o2b));
        HIPE(wgrad(i2b, stash(i2a), o2b.wg));
        HIPE(dgrad(i2b, o2b.dg, nullptr, a.t1));
        HIPE(lgate(i2a, a.t1, true, false, a.ssmall, &o2a));
        HIPE(wgrad(i2a, xin, o2a.wg));
        if (!it->first) {
            HIPE(dgrad(i2a, o2a.dg, g, go));
            std::swap(g, go);
            continue;
        }
        // projection shortcut: no activation of its own, its dz is the block's
        HIPE(lgate(i1, g, false, false, a.sbig, &o1));
        HIPE(wgrad(i1, xin, o1.wg));
        if (sa.stride == 1) {
            HIPE(dgrad(i2a, o2a.dg, nullptr, go));
            HIPE(dgrad(i1, o1.dg, go, g));
        } else {
            HIPE(dgrad(i2a, o2a.dg, nullptr, a.t0));
            HIPE(dgrad(i1, o1.dg, a.t0, a.t1));
            scatter2(a.t1, go, B, sa.hout, sa.cin, st);
            std::swap(g, go);
        }
    }
    maxpool_bwd(stash(0), g, go, B, 112, 64, st);
    HIPE(lgate(0, go, true, false, a.sbig, &o0));
    return wgrad(0, Prec<T>::wg0_input(c, images), o0.wg);
}

// dx of layer idx from its data-gradient operand, for the one-layer debug calls: a stride-2 layer's comes on the low-resolution map
template <class T>
int debug_data_grad(hpe_ctx* c, int idx, const T* dzs, int B, T* dx, hipStream_t st) {
    const ConvSpec& s = specs()[idx];
    T* t0 = c->et.acts<T>().t0;
    if (s.stride == 1) {
        HIP_TRY(data_grad(c, idx, dzs, B, nullptr, dx, st));
    } else {
        HIP_TRY(data_grad(c, idx, dzs, B, nullptr, t0, st));
        scatter2(t0, dx, B, s.hout, s.cin, st);
        HIP_TRY(hipGetLastError());
    }
    return HPE_OK;
}

// what a call needs reserved (nothing yet, or one of the four reserves): the reserve's batch, its entry point, the name of its range
const struct {
    int EncTrainWork::*batch;
    const char *call, *range;
} reserves[] = {{nullptr, nullptr, "max_batch"},
                {&EncTrainWork::B, "hpe_encoder_train_reserve", "reserved batch"},
                {&EncTrainWork::bn_B, "hpe_encoder_train_reserve_batchnorm", "batch of the batch-norm reserve"},
                {&EncTrainWork::mx_B, "hpe_encoder_train_reserve_mixed", "batch of the mixed-precision reserve"},
                {&EncTrainWork::mxbn_B, "hpe_encoder_train_reserve_batchnorm_mixed", "batch of the mixed-precision batch-norm reserve"}};

int check_train(hpe_ctx* c, int B, Reserve need = RESERVE_FROZEN) {
    if (!c) return fail(HPE_ERR_INVALID, "null ctx");
    if (c->dead) return fail(HPE_ERR_STATE, "hpe_finalize failed on this ctx: destroy it and create a new one");
    if (!c->finalized) return fail(HPE_ERR_STATE, "hpe_finalize() has not been called");
    if (!c->have_encoder) return fail(HPE_ERR_STATE, "encoder weights were not loaded before hpe_finalize");
    if (c->bf16) return fail(HPE_ERR_STATE, "encoder training needs an fp32 context");
    if (need != RESERVE_NONE)  // the frozen reserve, which every other one builds on, then the call's own
        for (Reserve r : {RESERVE_FROZEN, need})
            if (c->et.*reserves[r].batch == 0) return fail(HPE_ERR_STATE, std::string(reserves[r].call) + "() has not been called");
    const int top = need == RESERVE_NONE ? c->cfg.max_batch : c->et.*reserves[need].batch;
    if (B < 1 || B > top) return fail(HPE_ERR_INVALID, "batch " + std::to_string(B) + " outside [1, " + reserves[need].range + "]");
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

template <class T>
void walk_done(hpe_ctx* c, bool bn, int B) {
    Prec<T>::done(c->et, B, bn);
    if (!bn) return;
    // the statistics in bn_batch are those of the last batch-statistics walk of either precision
    c->et.bn_stat_mixed = Prec<T>::mixed;
    c->et.bn_stat_B = B;
    c->et.bn_stat_G = c->et.reduce ? c->et.reduce_G : B;
}

// hpe_encoder_forward_train / _batchnorm / _mixed / _batchnorm_mixed and hpe_encoder_backward / _batchnorm / _mixed / _batchnorm_mixed
template <class T>
int forward_entry(hpe_ctx* c, bool bn, const float* images, int B, float* features, void* stream) {
    int rc = check_train(c, B, Prec<T>::reserve(bn));
    if (rc) return rc;
    if (!images || !features) return fail(HPE_ERR_INVALID, "null pointer");
    DeviceGuard g(c->cfg.device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if ((rc = check_reduce(c, bn, B, st))) return rc;
    if ((rc = walk_result(c, forward_train<T>(c, bn, images, B, features, st), "forward"))) return rc;
    walk_done<T>(c, bn, B);
    return HPE_OK;
}

template <class T>
int backward_entry(hpe_ctx* c, bool bn, const float* images, int B, const float* grad_features, float* grad_flat, void* stream) {
    int rc = check_train(c, B, Prec<T>::reserve(bn));
    if (rc) return rc;
    if (!images || !grad_features || !grad_flat) return fail(HPE_ERR_INVALID, "null pointer");
    DeviceGuard g(c->cfg.device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if ((rc = check_reduce(c, bn, B, st))) return rc;
    if ((rc = walk_result(c, backward<T>(c, bn, images, B, grad_features, grad_flat, st), "backward"))) return rc;
    walk_done<T>(c, bn, B);
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

// ---- the one-layer and stash debug calls, one body for both precisions.  T = bf16e: the tensors are bf16 and the call is the _mixed one

// What opens a one-layer debug call: mixed, the cast of the layer's weight operand (backward: and of its data-gradient operand).  *in:
// the layer's input x, or for conv1, where x is the fp32 images, what the precision reads in their place -- the padded input of the
// convolution, or (backward) what Prec<T> says conv1's weight gradient reads
template <class T>
hipError_t debug_open(hpe_ctx* c, int idx, const void* x, int B, bool backward, hipStream_t st, const T** in) {
    HIPE(Prec<T>::cast(c, idx, 1, st));
    if (backward && idx > 0) HIPE(Prec<T>::cast(c, HPE_NUM_CONV - 1 + idx, 1, st));
    *in = static_cast<const T*>(x);
    if (idx != 0) return hipSuccess;
    const float* images = static_cast<const float*>(x);
    if (!backward || Prec<T>::wg0_padded) HIPE(pad_images<T>(c, images, B, st));
    *in = backward ? Prec<T>::wg0_input(c, images) : Prec<T>::padded(c);
    return hipSuccess;
}

// hpe_debug_conv_backward / _mixed
template <class T>
int debug_conv_backward(hpe_ctx* c, int idx, const void* x, const T* y, const T* dy, int B, T* dx, float* grad_layer, void* stream) {
    int rc = check_train(c, B, Prec<T>::reserve(false));
    if (rc) return rc;
    if (idx < 0 || idx >= HPE_NUM_CONV || !x || !dy || !grad_layer) return fail(HPE_ERR_INVALID, "bad argument");
    if (idx == 0 && dx)
        return fail(HPE_ERR_INVALID, std::string("hpe_debug_conv_backward") + Prec<T>::suffix + ": conv1 has no data gradient, dx_dev must be NULL");
    DeviceGuard g(c->cfg.device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const ConvSpec& s = specs()[idx];
    EncActs<T>& a = c->et.acts<T>();
    const T* in;
    HIP_TRY(debug_open<T>(c, idx, x, B, true, st, &in));
    const long n = (long)B * s.hout * s.hout * s.cout;
    gate(dy, y, c->conv[idx].scale, a.g0, dx ? a.sbig : nullptr, n, s.cout, st);
    HIP_TRY(weight_grad(c, idx, in, a.g0, B, grad_layer, st));
    return dx ? debug_data_grad<T>(c, idx, a.sbig, B, dx, st) : HPE_OK;
}

// hpe_debug_conv_batchnorm / _mixed
template <class T>
int debug_conv_batchnorm(hpe_ctx* c, int idx, const void* x, int B, const T* residual, int relu, T* y, T* z_out, float* stats_out, void* stream) {
    int rc = check_train(c, B, Prec<T>::reserve(true));
    if (rc) return rc;
    if (idx < 0 || idx >= HPE_NUM_CONV || !x || !y || !z_out || !stats_out) return fail(HPE_ERR_INVALID, "bad argument");
    DeviceGuard g(c->cfg.device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const T* in;
    HIP_TRY(debug_open<T>(c, idx, x, B, false, st, &in));
    const BnSlots s = bn_slots(c, idx, true);
    HIP_TRY(layer_forward_bn<T>(c, idx, in, B, residual, relu, z_out, y, s, st));
    const size_t n = (size_t)specs()[idx].cout * sizeof(float);
    HIP_TRY(hipMemcpyAsync(stats_out, s.mu, n, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(stats_out + specs()[idx].cout, s.var, n, hipMemcpyDeviceToDevice, st));
    return HPE_OK;
}

// hpe_debug_conv_backward_batchnorm / _mixed
template <class T>
int debug_conv_backward_batchnorm(hpe_ctx* c, int idx, const void* x, const T* z, const T* y, const T* dy, int B, T* dx, float* grad_layer,
                                  void* stream) {
    int rc = check_train(c, B, Prec<T>::reserve(true));
    if (rc) return rc;
    if (idx < 0 || idx >= HPE_NUM_CONV || !x || !z || !dy || !grad_layer) return fail(HPE_ERR_INVALID, "bad argument");
    if (idx == 0 && dx)
        return fail(HPE_ERR_INVALID,
                    std::string("hpe_debug_conv_backward_batchnorm") + Prec<T>::suffix + ": conv1 has no data gradient, dx_dev must be NULL");
    DeviceGuard g(c->cfg.device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const ConvSpec& s = specs()[idx];
    EncTrainWork& w = c->et;
    T* sbig = w.acts<T>().sbig;
    const T* in;
    HIP_TRY(debug_open<T>(c, idx, x, B, true, st, &in));
    const BnSlots sl = bn_slots(c, idx, true);
    HIP_TRY(bn_launch_stats(z, B * s.hout * s.hout, s.cout, c->cfg.bn_eps, w.bn_part, sl.mu, sl.var, sl.r, st));
    HIP_TRY(layer_gate_bn<T>(c, idx, dy, y, z, B, sl, grad_layer, nullptr, sbig, st));
    HIP_TRY(weight_grad(c, idx, in, sbig, B, grad_layer, st, true));
    return dx ? debug_data_grad<T>(c, idx, sbig, B, dx, st) : HPE_OK;
}

// hpe_debug_encoder_stash / _mixed (idx -1: the pooled map) and hpe_debug_encoder_stash_raw / _raw_mixed
template <class T>
int debug_stash(hpe_ctx* c, bool raw, int idx, T* out, void* stream) {
    int rc = check_train(c, 1, Prec<T>::reserve(raw));
    if (rc) return rc;
    if (idx < (raw ? 0 : -1) || idx >= HPE_NUM_CONV || !out) return fail(HPE_ERR_INVALID, "bad argument");
    const char* why;
    const int B = raw ? Prec<T>::zstash_batch(c->et, &why) : Prec<T>::stash_batch(c->et, &why);
    if (B == 0) return fail(HPE_ERR_STATE, std::string("hpe_debug_encoder_stash") + (raw ? "_raw" : "") + Prec<T>::suffix + ": " + why);
    DeviceGuard g(c->cfg.device);
    const size_t n = idx < 0 ? (size_t)POOL_FLOATS : (size_t)specs()[idx].hout * specs()[idx].hout * specs()[idx].cout;
    const T* src = raw ? zstash_of<T>(c, idx, B) : stash_of<T>(c, idx, B);
    HIP_TRY(hipMemcpyAsync(out, src, (size_t)B * n * sizeof(T), hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream)));
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
    wg_slicing(idx, B, 8, &P, &sl);
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
    train_buffers(w, RESERVE_FROZEN, B, alloc);
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
    return forward_entry<float>(c, false, images, B, features, stream);
}

int hpe_encoder_backward(hpe_ctx* c, const float* images, int B, const float* grad_features, float* grad_flat, void* stream) {
    return backward_entry<float>(c, false, images, B, grad_features, grad_flat, stream);
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
    return debug_conv_backward<float>(c, idx, x, y, dy, B, dx, grad_layer, stream);
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
    return debug_stash<float>(c, false, idx, out, stream);
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
    train_buffers(w, RESERVE_BN, B, alloc);
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
    return forward_entry<float>(c, true, images, B, features, stream);
}

int hpe_encoder_backward_batchnorm(hpe_ctx* c, const float* images, int B, const float* grad_features, float* grad_flat, void* stream) {
    return backward_entry<float>(c, true, images, B, grad_features, grad_flat, stream);
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
    return debug_conv_batchnorm<float>(c, idx, x, B, residual, relu, y, z_out, stats_out, stream);
}

int hpe_debug_conv_backward_batchnorm(hpe_ctx* c, int idx, const float* x, const float* z, const float* y, const float* dy, int B, float* dx,
                                      float* grad_layer, void* stream) {
    return debug_conv_backward_batchnorm<float>(c, idx, x, z, y, dy, B, dx, grad_layer, stream);
}

int hpe_debug_encoder_stash_raw(hpe_ctx* c, int idx, float* out, void* stream) {
    return debug_stash<float>(c, true, idx, out, stream);
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
    HIP_TRY(bn_launch_bwd_apply(dy, y, z, sl.mu, sl.r, w.flat + layout().off[idx][2], red + N, red, rows, N, nullptr, w.f32.sbig, st, (double)M));
    HIP_TRY(weight_grad(c, idx, x, w.f32.sbig, B, grad_layer, st, true));
    return dx ? debug_data_grad<float>(c, idx, w.f32.sbig, B, dx, st) : HPE_OK;
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
    train_buffers(w, RESERVE_MIXED, B, alloc);
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
    return forward_entry<bf16e>(c, false, images, B, features, stream);
}

int hpe_encoder_backward_mixed(hpe_ctx* c, const float* images, int B, const float* grad_features, float* grad_flat, void* stream) {
    return backward_entry<bf16e>(c, false, images, B, grad_features, grad_flat, stream);
}

int hpe_debug_conv_backward_mixed(hpe_ctx* c, int idx, const void* x, const void* y, const void* dy, int B, void* dx, float* grad_layer,
                                  void* stream) {
    return debug_conv_backward<bf16e>(c, idx, x, static_cast<cmx16>(y), static_cast<cmx16>(dy), B, static_cast<mx16>(dx), grad_layer, stream);
}

int hpe_debug_maxpool_backward_mixed(const void* x, const void* dy, int B, int H, int C, void* dx, void* stream) {
    if (!x || !dy || !dx || B < 1 || H < 2 || (H & 1) || C < 8 || (C & 7)) return fail(HPE_ERR_INVALID, "bad argument");
    maxpool_bwd(static_cast<cmx16>(x), static_cast<cmx16>(dy), static_cast<mx16>(dx), B, H, C, static_cast<hipStream_t>(stream));
    HIP_TRY(hipGetLastError());
    return HPE_OK;
}

int hpe_debug_avgpool_backward_mixed(const float* dy, int B, int HW, int C, void* dx, void* stream) {
    if (!dy || !dx || B < 1 || HW < 1 || C < 8 || (C & 7)) return fail(HPE_ERR_INVALID, "bad argument");
    avgpool_bwd(dy, static_cast<mx16>(dx), B, HW, C, static_cast<hipStream_t>(stream));
    HIP_TRY(hipGetLastError());
    return HPE_OK;
}

int hpe_debug_encoder_stash_batch_mixed(hpe_ctx* c) { return (c && c->finalized && !c->dead) ? c->et.mx_stash_B : 0; }

int hpe_debug_encoder_stash_mixed(hpe_ctx* c, int idx, void* out, void* stream) {
    return debug_stash<bf16e>(c, false, idx, static_cast<mx16>(out), stream);
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
    train_buffers(w, RESERVE_BN_MIXED, B, alloc);
    if (alloc.rc) return alloc.rc;
    w.mxbn_B = B;
    return HPE_OK;
}

int hpe_encoder_forward_batchnorm_mixed(hpe_ctx* c, const float* images, int B, float* features, void* stream) {
    return forward_entry<bf16e>(c, true, images, B, features, stream);
}

int hpe_encoder_backward_batchnorm_mixed(hpe_ctx* c, const float* images, int B, const float* grad_features, float* grad_flat, void* stream) {
    return backward_entry<bf16e>(c, true, images, B, grad_features, grad_flat, stream);
}

int hpe_debug_conv_batchnorm_mixed(hpe_ctx* c, int idx, const void* x, int B, const void* residual, int relu, void* y, void* z_out, float* stats_out,
                                   void* stream) {
    return debug_conv_batchnorm<bf16e>(c, idx, x, B, static_cast<cmx16>(residual), relu, static_cast<mx16>(y), static_cast<mx16>(z_out), stats_out, stream);
}

int hpe_debug_conv_backward_batchnorm_mixed(hpe_ctx* c, int idx, const void* x, const void* z, const void* y, const void* dy, int B, void* dx,
                                            float* grad_layer, void* stream) {
    return debug_conv_backward_batchnorm<bf16e>(c, idx, x, static_cast<cmx16>(z), static_cast<cmx16>(y), static_cast<cmx16>(dy), B, static_cast<mx16>(dx), grad_layer,
                                                stream);
}

int hpe_debug_encoder_stash_raw_mixed(hpe_ctx* c, int idx, void* out, void* stream) {
    return debug_stash<bf16e>(c, true, idx, static_cast<mx16>(out), stream);
}

}  // extern "C"
#pragma GCC visibility pop
