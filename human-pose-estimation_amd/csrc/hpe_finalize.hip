// hpe_finalize.hip -- weight ingestion (Keras layouts) and hpe_finalize: BN folding, weight packing for every kernel family the plan
// selects, workspace sizing, streams and events.  Host logic only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "hpe_ctx.h"

int dev_alloc(hpe_ctx* c, float** p, size_t n_floats, bool zero) {
    void* q = nullptr;
    HIP_TRY(hipMalloc(&q, n_floats * sizeof(float)));
    c->allocs.push_back(q);
    if (zero) HIP_TRY(hipMemset(q, 0, n_floats * sizeof(float)));
    *p = static_cast<float*>(q);
    return HPE_OK;
}

int upload(hpe_ctx* c, float** p, const std::vector<float>& h) {
    int rc = dev_alloc(c, p, h.size(), false);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(*p, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
    return HPE_OK;
}

// upload(), or a copy into the buffer *p already names (repack_encoder: the pointers of a finalized context never change)
static int upload_to(hpe_ctx* c, float** p, const std::vector<float>& h) {
    if (!*p) return upload(c, p, h);
    HIP_TRY(hipMemcpy(*p, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
    return HPE_OK;
}

// bf16 elements into a new buffer, or into the buffer *p already names (as upload_to)
static int upload_bf16(hpe_ctx* c, void** p, const std::vector<unsigned short>& h) {
    if (!*p) {
        HIP_TRY(hipMalloc(p, h.size() * 2));
        c->allocs.push_back(*p);
    }
    HIP_TRY(hipMemcpy(*p, h.data(), h.size() * 2, hipMemcpyHostToDevice));
    return HPE_OK;
}

// (bf16 contexts keep bf16 elements behind the float* members of ConvLayer)
static int upload_bf16(hpe_ctx* c, float** p, const std::vector<unsigned short>& h) {
    void* q = *p;
    const int rc = upload_bf16(c, &q, h);
    *p = static_cast<float*>(q);
    return rc;
}

static std::vector<unsigned short> to_bf16(const std::vector<float>& v) {
    std::vector<unsigned short> h(v.size());
    for (size_t q = 0; q < v.size(); ++q) h[q] = f2bf(v[q]);
    return h;
}

// fp32 Wt[rows][K] -> bf16 [rows][3][K]: w = w0 + w1 + w2 exactly (finite weights), each piece rounded to nearest even (conv_gemm_f32s.hip)
int upload_split(hpe_ctx* c, void** p, const std::vector<float>& wt, int rows, int K) {
    std::vector<unsigned short> ws((size_t)rows * 3 * K);
    for (int n = 0; n < rows; ++n)
        for (int k = 0; k < K; ++k) {
            unsigned short h[3];
            bf16_split3(wt[(size_t)n * K + k], h);
            unsigned short* d = &ws[(size_t)n * 3 * K + k];
            d[0] = h[0];
            d[K] = h[1];
            d[2 * K] = h[2];
        }
    return upload_bf16(c, p, ws);
}

// the split image conv_stream_f32s.hip reads, [rows][3][K] bf16, appended behind the rows * K floats of wt (a layer without the split
// packing keeps it in the allocation of its fp32 weights: w_stream_of)
static void append_split(std::vector<float>& wt, int rows, int K) {
    const size_t nw = (size_t)rows * K;
    std::vector<unsigned short> ws(nw * 3);
    for (int n = 0; n < rows; ++n)
        for (int k = 0; k < K; ++k) {
            unsigned short h[3];
            bf16_split3(wt[(size_t)n * K + k], h);
            for (int j = 0; j < 3; ++j) ws[((size_t)n * 3 + j) * K + k] = h[j];
        }
    wt.resize(nw + nw * 3 / 2);
    memcpy(wt.data() + nw, ws.data(), ws.size() * 2);
}

#pragma GCC visibility push(default)
extern "C" {

int hpe_load_smpl(hpe_ctx* c, const HpeSmplModel* m) {
    if (!c || !m) return fail(HPE_ERR_INVALID, "null argument");
    if (c->finalized) return fail(HPE_ERR_STATE, "already finalized");
    if (!m->v_template || !m->shapedirs || !m->posedirs || !m->J_regressor || !m->weights || !m->kp_regressor || !m->parents)
        return fail(HPE_ERR_INVALID, "null SMPL array");
    if (m->num_kp < 1 || m->num_kp > HPE_MAX_KP) return fail(HPE_ERR_INVALID, "num_kp must be in [1,24]");
    if (m->parents[0] >= 0) return fail(HPE_ERR_INVALID, "parents[0] must be negative (root)");
    for (int i = 1; i < 24; ++i)
        if (m->parents[i] < 0 || m->parents[i] >= i) return fail(HPE_ERR_INVALID, "parents[i] must satisfy 0 <= parents[i] < i");
    const int V = HPE_NUM_VERTS;
    c->h_vt.assign(m->v_template, m->v_template + V * 3);
    c->h_sd.assign(m->shapedirs, m->shapedirs + (size_t)V * 3 * 10);
    c->h_pd.assign(m->posedirs, m->posedirs + (size_t)V * 3 * 207);
    c->h_jreg.assign(m->J_regressor, m->J_regressor + (size_t)24 * V);
    c->h_w.assign(m->weights, m->weights + (size_t)V * 24);
    c->h_kreg.assign(m->kp_regressor, m->kp_regressor + (size_t)m->num_kp * V);
    c->h_par.assign(m->parents, m->parents + 24);
    c->num_kp = m->num_kp;
    c->smpl_loaded = true;
    return HPE_OK;
}

int hpe_load_conv(hpe_ctx* c, int idx, const float* kernel, const float* bias, const float* gamma, const float* beta,
                  const float* mean, const float* var) {
    if (!c || idx < 0 || idx >= HPE_NUM_CONV) return fail(HPE_ERR_INVALID, "bad conv index");
    if (c->finalized) return fail(HPE_ERR_STATE, "already finalized");
    if (!kernel || !bias || !gamma || !beta || !mean || !var) return fail(HPE_ERR_INVALID, "null conv array");
    const ConvSpec& s = specs()[idx];
    ConvLayer& L = c->conv[idx];
    L.kernel.assign(kernel, kernel + (size_t)s.kh * s.kw * s.cin * s.cout);
    L.bias.assign(bias, bias + s.cout);
    L.gamma.assign(gamma, gamma + s.cout);
    L.beta.assign(beta, beta + s.cout);
    L.mean.assign(mean, mean + s.cout);
    L.var.assign(var, var + s.cout);
    L.loaded = true;
    return HPE_OK;
}

int hpe_load_dense(hpe_ctx* c, int idx, const float* kernel, const float* bias) {
    if (!c || idx < 0 || idx >= HPE_NUM_DENSE) return fail(HPE_ERR_INVALID, "bad dense index");
    if (c->finalized) return fail(HPE_ERR_STATE, "already finalized");
    if (!kernel || !bias) return fail(HPE_ERR_INVALID, "null dense array");
    const int din[3] = {2133, 1024, 1024}, dout[3] = {1024, 1024, 85};
    c->dense[idx].kernel.assign(kernel, kernel + (size_t)din[idx] * dout[idx]);
    c->dense[idx].bias.assign(bias, bias + dout[idx]);
    c->dense[idx].loaded = true;
    return HPE_OK;
}

int hpe_load_mean_theta(hpe_ctx* c, const float* mean85) {
    if (!c || !mean85) return fail(HPE_ERR_INVALID, "null argument");
    if (c->finalized) return fail(HPE_ERR_STATE, "already finalized");
    memcpy(c->h_mean, mean85, sizeof(float) * HPE_THETA_DIM);
    c->mean_loaded = true;
    return HPE_OK;
}

}  // extern "C"
#pragma GCC visibility pop

// release everything a (possibly partial) hpe_finalize created
void release_device_state(hpe_ctx* c) {
    for (void* p : c->allocs) (void)hipFree(p);
    c->allocs.clear();
    c->rt = RegTrainWork{};
    c->et = EncTrainWork{};
    if (c->critic_buf) {
        (void)hipFree(c->critic_buf);
        c->critic_buf = nullptr;
        c->critic = CriticW{};
        c->have_critic = false;
    }
    if (c->critic_ws) {
        (void)hipFree(c->critic_ws);
        c->critic_ws = nullptr;
        c->critic_ws_floats = 0;
    }
    for (auto& a : c->aux)
        if (a) {
            (void)hipStreamDestroy(a);
            a = nullptr;
        }
    auto kill = [](hipEvent_t& e) {
        if (e) {
            (void)hipEventDestroy(e);
            e = nullptr;
        }
    };
    kill(c->ev_fork);
    kill(c->ev_enc);
    kill(c->ev_tail);
    for (auto& e : c->ev_feat_free) kill(e);
    if (c->tail_st) {
        (void)hipStreamDestroy(c->tail_st);
        c->tail_st = nullptr;
    }
    for (auto& e : c->ev_join) kill(e);
    for (auto& e : c->ev) kill(e);
    for (auto& e : c->span0) kill(e);
    for (auto& e : c->span1) kill(e);
    for (auto& e : c->cev0) kill(e);
    for (auto& e : c->cev1) kill(e);
    for (auto& e : c->lev0) kill(e);
    for (auto& e : c->lev1) kill(e);
    for (auto& e : c->lev_all) kill(e);
    c->ev_ok = false;
}

// every part is either loaded completely or not at all
static int check_loaded(hpe_ctx* c) {
    int nconv = 0, ndense = 0;
    for (int i = 0; i < HPE_NUM_CONV; ++i) nconv += c->conv[i].loaded ? 1 : 0;
    for (int i = 0; i < HPE_NUM_DENSE; ++i) ndense += c->dense[i].loaded ? 1 : 0;
    if (nconv != 0 && nconv != HPE_NUM_CONV) {
        for (int i = 0; i < HPE_NUM_CONV; ++i)
            if (!c->conv[i].loaded) return fail(HPE_ERR_STATE, std::string("conv layer not loaded: ") + specs()[i].name);
    }
    if (ndense != 0 && (ndense != HPE_NUM_DENSE || !c->mean_loaded))
        return fail(HPE_ERR_STATE, "regressor needs all 3 dense layers and the mean theta");
    c->have_encoder = nconv == HPE_NUM_CONV;
    c->have_regressor = ndense == HPE_NUM_DENSE && c->mean_loaded;
    c->have_smpl = c->smpl_loaded;
    if (!c->have_encoder && !c->have_regressor && !c->have_smpl) return fail(HPE_ERR_STATE, "nothing was loaded");
    return HPE_OK;
}

// ---- conv_block (first block of a stage): out = relu(bn2c(W2c . t2) + bn1(W1 . x_strided)).  Both convolutions are 1x1,
//      so they are ONE GEMM over the concatenated k axis once each BN scale is folded into its weights:
//      out = relu([s2c W2c | s1 W1] . [t2 ; x] + (shift2c + shift1))   -- no shortcut tensor in HBM, one launch instead of two
static int pack_dual_weights(hpe_ctx* c) {
    int rc;
    for (const ResBlock& blk : blocks()) {
        const unsigned packs = layer_packs(c->plan, c->bf16, blk.i2c);
        if (!(packs & PACK_W_DUAL)) continue;
        const ConvSpec& s2 = specs()[blk.i2c];
        const ConvSpec& s1 = specs()[blk.i1];
        ConvLayer& L2 = c->conv[blk.i2c];
        const ConvLayer& L1 = c->conv[blk.i1];
        const int K1 = s2.cin, K2 = s1.cin, N = s2.cout;
        const int n_pad = round_up(N, 128), K = K1 + K2;
        std::vector<float> wt((size_t)n_pad * K, 0.f), sh(N);
        for (int n = 0; n < N; ++n) {
            double inv2, inv1, shift2, shift1;
            bn_fold(L2, n, c->cfg.bn_eps, &inv2, &shift2);
            bn_fold(L1, n, c->cfg.bn_eps, &inv1, &shift1);
            for (int k = 0; k < K1; ++k) wt[(size_t)n * K + k] = (float)(inv2 * (double)L2.kernel[(size_t)k * N + n]);
            for (int k = 0; k < K2; ++k) wt[(size_t)n * K + K1 + k] = (float)(inv1 * (double)L1.kernel[(size_t)k * N + n]);
            sh[n] = (float)(shift2 + shift1);
        }
        if (c->bf16) {
            if ((rc = upload_bf16(c, &L2.w_dual, to_bf16(wt)))) return rc;
        } else {
            const bool stream = stream1x1_dual(c->plan, c->bf16, blk), derived = stream && !(packs & PACK_W_DUAL_SPLIT);
            if (derived) append_split(wt, n_pad, K);
            if ((rc = upload_to(c, &L2.w_dual, wt))) return rc;
            if ((packs & PACK_W_DUAL_SPLIT) && (rc = upload_split(c, &L2.w_dual_split, wt, n_pad, K))) return rc;
            if (stream) L2.w_dual_stream = derived ? w_stream_of(L2.w_dual, n_pad, K) : static_cast<unsigned short*>(L2.w_dual_split);
        }
        if ((rc = upload_to(c, &L2.shift_dual, sh))) return rc;
        L2.k_dual = K;
        L2.k1_dual = K1;
    }
    return HPE_OK;
}

// the F(2x2,3x3) Winograd weights of one 3x3 layer (conv_wino.hip)
static int pack_wino_weights(hpe_ctx* c, const ConvSpec& s, ConvLayer& L) {
    int rc;
    // U = G g G^T in double (wino_elem); layout [cout/64][cin/8][16][2][64][4] (wino_u_base)
    std::vector<float> U((size_t)16 * s.cin * s.cout);
    for (int ci = 0; ci < s.cin; ++ci)
        for (int n = 0; n < s.cout; ++n) {
            double g[3][3];
            for (int a = 0; a < 3; ++a)
                for (int b = 0; b < 3; ++b) g[a][b] = L.kernel[(((size_t)a * 3 + b) * s.cin + ci) * s.cout + n];
            const size_t base = wino_u_base(n, ci, s.cin);
            for (int xi = 0; xi < 4; ++xi)
                for (int nu = 0; nu < 4; ++nu) {
                    const double gx[3] = {wino_g(xi, 0), wino_g(xi, 1), wino_g(xi, 2)}, gn[3] = {wino_g(nu, 0), wino_g(nu, 1), wino_g(nu, 2)};
                    U[base + (size_t)(xi * 4 + nu) * 512] = wino_elem(gx, gn, g);
                }
        }
    if (!(c->plan.wino_fused && s.hin >= c->plan.wino_fused_min_hw)) return upload_to(c, &L.wino_u, U);
    // the fused kernel of the large maps reads U as three bf16 pieces (wino_us_base): kept behind wino_u in the same allocation
    const size_t nu = U.size();
    std::vector<unsigned short> Us((size_t)3 * nu);
    for (int ci = 0; ci < s.cin; ++ci)
        for (int n = 0; n < s.cout; ++n)
            for (int e = 0; e < 16; ++e) {
                unsigned short h[3];
                bf16_split3(U[wino_u_base(n, ci, s.cin) + (size_t)e * 512], h);
                for (int j = 0; j < 3; ++j) Us[wino_us_base(n, ci, s.cin) + j * WINO_US_PIECE + (size_t)e * 512] = h[j];
            }
    U.resize(nu + Us.size() / 2);
    memcpy(U.data() + nu, Us.data(), Us.size() * 2);
    if ((rc = upload_to(c, &L.wino_u, U))) return rc;
    L.wino_u_split = wino_u_split_of(L.wino_u, s.cin, s.cout);
    return HPE_OK;
}

// the F(4x4,3x3) Winograd weights of one 3x3 layer (conv_wino4.hip)
static int pack_wino4_weights(hpe_ctx* c, const ConvSpec& s, ConvLayer& L) {
    int rc;
    // F(4x4,3x3): U = G g G^T in double (wino_elem, rows of wino4_g); layout [cout/64][cin/4][36][64][4] (wino4_u_base)
    std::vector<float> U((size_t)36 * s.cin * s.cout);
    for (int ci = 0; ci < s.cin; ++ci)
        for (int n = 0; n < s.cout; ++n) {
            double g[3][3];
            for (int a = 0; a < 3; ++a)
                for (int b = 0; b < 3; ++b) g[a][b] = L.kernel[(((size_t)a * 3 + b) * s.cin + ci) * s.cout + n];
            const size_t base = wino4_u_base(n, ci, s.cin);
            for (int xi = 0; xi < 6; ++xi)
                for (int nu = 0; nu < 6; ++nu) {
                    const double gx[3] = {wino4_g(xi, 0), wino4_g(xi, 1), wino4_g(xi, 2)}, gn[3] = {wino4_g(nu, 0), wino4_g(nu, 1), wino4_g(nu, 2)};
                    U[base + (size_t)(xi * 6 + nu) * 256] = wino_elem(gx, gn, g);
                }
        }
    if ((rc = upload_to(c, &L.wino4_u, U))) return rc;
    return HPE_OK;
}

// fused stem: the conv1 weights in the k enumeration of stem_fused.hip
static int pack_stem_weights(hpe_ctx* c, ConvLayer& L) {
    // [64][7][32], k as in Wt[n][k]: rounded to bf16 (bf16 contexts), or its three exact bf16 pieces [3][64][7][32] (fp32 contexts)
    const size_t ld = 7 * 32;
    std::vector<float> wp(64 * ld, 0.f);
    for (int kh = 0; kh < 7; ++kh)
        for (int kw = 0; kw < 7; ++kw)
            for (int ci = 0; ci < 3; ++ci) {
                const int k = conv_wt_k(0, kh, kw, ci);
                for (int n = 0; n < 64; ++n) wp[n * ld + k] = L.kernel[(((size_t)kh * 7 + kw) * 3 + ci) * 64 + n];
            }
    if (c->bf16) return upload_bf16(c, &L.stem_w, to_bf16(wp));
    std::vector<unsigned short> ws(3 * wp.size());
    for (size_t o = 0; o < wp.size(); ++o) {
        unsigned short h[3];
        bf16_split3(wp[o], h);
        for (int j = 0; j < 3; ++j) ws[j * wp.size() + o] = h[j];
    }
    return upload_bf16(c, &L.stem_w, ws);
}

// ---- encoder weights: HWIO -> Wt[n][k] (k = (kh,kw,cin), cin fastest), zero padded; BN -> scale/shift; and the packings layer_packs names
static int pack_conv_weights(hpe_ctx* c) {
    int rc;
    for (int i = 0; i < HPE_NUM_CONV; ++i) {
        const ConvSpec& s = specs()[i];
        ConvLayer& L = c->conv[i];
        const unsigned packs = layer_packs(c->plan, c->bf16, i);
        L.n_pad = round_up(s.cout, 128);
        L.k_pad = conv_k_pad(i, c->bf16);
        std::vector<float> wt((size_t)L.n_pad * L.k_pad, 0.f);
        for (int kh = 0; kh < s.kh; ++kh)
            for (int kw = 0; kw < s.kw; ++kw)
                for (int ci = 0; ci < s.cin; ++ci) {
                    const int k = conv_wt_k(i, kh, kw, ci);
                    const float* src = &L.kernel[(((size_t)kh * s.kw + kw) * s.cin + ci) * s.cout];
                    for (int n = 0; n < s.cout; ++n) wt[(size_t)n * L.k_pad + k] = src[n];
                }
        if (c->bf16) {
            if ((rc = upload_bf16(c, &L.w, to_bf16(wt)))) return rc;
        } else {
            const bool stream = stream1x1_layer(c->plan, c->bf16, i), derived = stream && !(packs & PACK_W_SPLIT);
            if (derived) append_split(wt, L.n_pad, L.k_pad);
            if ((rc = upload_to(c, &L.w, wt))) return rc;
            if ((packs & PACK_W_SPLIT) && (rc = upload_split(c, &L.w_split, wt, L.n_pad, L.k_pad))) return rc;
            if (stream) L.w_stream = derived ? w_stream_of(L.w, L.n_pad, L.k_pad) : static_cast<unsigned short*>(L.w_split);
            if ((packs & PACK_WINO_U) && (rc = pack_wino_weights(c, s, L))) return rc;
            if ((packs & PACK_WINO4_U) && (rc = pack_wino4_weights(c, s, L))) return rc;
        }
        if ((packs & PACK_STEM_W) && (rc = pack_stem_weights(c, L))) return rc;
        std::vector<float> sc(s.cout), sh(s.cout);
        for (int n = 0; n < s.cout; ++n) {
            double scale, shift;
            bn_fold(L, n, c->cfg.bn_eps, &scale, &shift);
            sc[n] = (float)scale;
            sh[n] = (float)shift;
        }
        if ((rc = upload_to(c, &L.scale, sc))) return rc;
        if ((rc = upload_to(c, &L.shift, sh))) return rc;
        std::vector<float>().swap(L.kernel);
    }
    return HPE_OK;
}

// ---- regressor: Dense kernels [in,out] -> [out_pad][in_pad], W1 split into features / theta parts, and the Keras-major operands of the
//      backward.  The layouts are stated once, by the set kernels of regressor_train.hip: finalize runs them on the loaded parameters.
static int pack_regressor(hpe_ctx* c) {
    int rc;
    // Zero-filled: the set kernels write the live elements only, so this fill is what keeps the padding rows and columns zero.  They are
    // read: the theta GEMM feeds columns 85..95 of a theta row back as a K = 96 operand, and garbage there would reach the output.
    const struct {
        float** p;
        size_t n;
    } live[] = {
        {&c->w1f, (size_t)1024 * 2048},
        {&c->w1t, (size_t)1024 * THETA_LD},
        {&c->w2, (size_t)1024 * 1024},
        {&c->w3, (size_t)128 * 1024},
        {&c->b1, 1024},
        {&c->b2, 1024},
        {&c->b3, 128},
        {&c->mean_dev, HPE_THETA_DIM},
        {&c->rt.w1k, (size_t)(2048 + 128) * 1024},
        {&c->rt.w2k, (size_t)1024 * 1024},
        {&c->rt.w3k, (size_t)1024 * THETA_LD},
    };
    for (const auto& b : live)
        if ((rc = dev_alloc(c, b.p, b.n, true))) return rc;
    // the flat layout (regressor_spec.flat_layout): kernel and bias of the three layers as loaded, then mean theta
    std::vector<float> flat((size_t)regressor_param_offset(4, false));
    for (int i = 0; i < HPE_NUM_DENSE; ++i) {
        std::copy(c->dense[i].kernel.begin(), c->dense[i].kernel.end(), flat.begin() + regressor_param_offset(i, false));
        std::copy(c->dense[i].bias.begin(), c->dense[i].bias.end(), flat.begin() + regressor_param_offset(i, true));
    }
    std::copy(c->h_mean, c->h_mean + HPE_THETA_DIM, flat.begin() + regressor_param_offset(3, false));
    float* tmp = nullptr;  // in c->allocs while it lives: a failure below leaves it to release_device_state
    if ((rc = upload(c, &tmp, flat))) return rc;
    HIP_TRY(regressor_params_copy(c, tmp, true, nullptr));
    HIP_TRY(hipDeviceSynchronize());
    c->allocs.pop_back();
    HIP_TRY(hipFree(tmp));
    return HPE_OK;
}

// ---- SMPL constants in kernel layouts
static int pack_smpl(hpe_ctx* c) {
    int rc;
    const int V = HPE_NUM_VERTS, V3 = V * 3;
    // basis source [11][V*3]: row 0 v_template, rows 1..10 shapedirs^T  (shapedirs [V,3,10] -> [10][V*3])
    std::vector<float> src((size_t)11 * V3);
    memcpy(src.data(), c->h_vt.data(), sizeof(float) * V3);
    for (int i = 0; i < V3; ++i)
        for (int k = 0; k < 10; ++k) src[(size_t)(1 + k) * V3 + i] = c->h_sd[(size_t)i * 10 + k];
    if ((rc = upload(c, &c->smpl_basis_src, src))) return rc;
    c->smpl.v_template = c->smpl_basis_src;
    c->smpl.shapedirs = c->smpl_basis_src + V3;
    // posedirs [V,3,207] -> [207][V*3]
    std::vector<float> pd((size_t)207 * V3);
    for (int i = 0; i < V3; ++i)
        for (int k = 0; k < 207; ++k) pd[(size_t)k * V3 + i] = c->h_pd[(size_t)i * 207 + k];
    float* p = nullptr;
    if ((rc = upload(c, &p, pd))) return rc;
    c->smpl.posedirs = p;
    if ((rc = upload(c, &p, c->h_w))) return rc;
    c->smpl.weights = p;
    // regressors [K,V] -> [V][24] zero padded
    std::vector<float> jr((size_t)V * SMPL_KP_PITCH, 0.f), kr((size_t)V * SMPL_KP_PITCH, 0.f);
    for (int j = 0; j < 24; ++j)
        for (int v = 0; v < V; ++v) jr[(size_t)v * SMPL_KP_PITCH + j] = c->h_jreg[(size_t)j * V + v];
    for (int j = 0; j < c->num_kp; ++j)
        for (int v = 0; v < V; ++v) kr[(size_t)v * SMPL_KP_PITCH + j] = c->h_kreg[(size_t)j * V + v];
    if ((rc = upload(c, &p, jr))) return rc;
    c->smpl.j_reg = p;
    if ((rc = upload(c, &p, kr))) return rc;
    c->smpl.kp_reg = p;
    int depth[24], maxd = 0;
    for (int j = 0; j < 24; ++j) {
        depth[j] = c->h_par[j] < 0 ? 0 : depth[c->h_par[j]] + 1;
        if (depth[j] > maxd) maxd = depth[j];
    }
    void* ip = nullptr;
    HIP_TRY(hipMalloc(&ip, sizeof(int) * 48));
    c->allocs.push_back(ip);
    HIP_TRY(hipMemcpy(ip, c->h_par.data(), sizeof(int) * 24, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(static_cast<int*>(ip) + 24, depth, sizeof(int) * 24, hipMemcpyHostToDevice));
    c->smpl.parents = static_cast<int*>(ip);
    c->smpl.depth = static_cast<int*>(ip) + 24;
    c->smpl.max_depth = maxd;
    c->smpl.num_kp = c->num_kp;
    // 24-joint basis through the 6890 -> 24 joint-regressor kernel
    float* jb = nullptr;
    if ((rc = dev_alloc(c, &jb, 11 * 24 * 3, true))) return rc;
    HIP_TRY(hpe_launch_joint_regress(c->smpl_basis_src, c->smpl.j_reg, 11, 24, jb, nullptr, nullptr, nullptr));
    HIP_TRY(hipDeviceSynchronize());
    c->smpl.j_basis = jb;
    return HPE_OK;
}

// ---- workspaces for max_batch images
static int size_workspaces(hpe_ctx* c) {
    int rc;
    const size_t B = (size_t)c->cfg.max_batch;
    const size_t Bpad = (size_t)round_up(c->cfg.max_batch, SMPL_IMG_TILE);
    if (c->have_encoder) {
        if ((rc = dev_alloc(c, &c->padded, B * STEM_HP * STEM_WP * 4 + 64, true))) return rc;
        if ((rc = dev_alloc(c, &c->X0, B * 802816, false))) return rc;
        if ((rc = dev_alloc(c, &c->X1, B * 802816, false))) return rc;
        if ((rc = dev_alloc(c, &c->SC, B * 802816, false))) return rc;
        if ((rc = dev_alloc(c, &c->T1, B * 200704, false))) return rc;
        if ((rc = dev_alloc(c, &c->T2, B * 200704, false))) return rc;
        if ((rc = dev_alloc(c, &c->feat, B * HPE_FEATURE_DIM, true))) return rc;
        if ((rc = dev_alloc(c, &c->feat_alt, B * HPE_FEATURE_DIM, true))) return rc;
    }
    if (c->have_encoder && !c->bf16 && c->plan.wino_min_c > 0) {
        if ((rc = dev_alloc(c, &c->wino_v, B * WINO_V_PITCH + WINO_V_SLACK, false))) return rc;
        if (c->plan.wino_f4 && c->plan.wino4_ksplit) {
            // one workspace per chunk-stream slot (16 MB each), block counters zeroed
            const size_t nws = hpe_wino4_split_ws_floats();
            if ((rc = dev_alloc(c, &c->w4_split, 4 * nws, false))) return rc;
            for (int k = 0; k < 4; ++k) HIP_TRY(hipMemset(c->w4_split + (k + 1) * nws - 256, 0, 256 * sizeof(unsigned)));
        }
        // persistent stream-K scheduling of the Winograd GEMM (opt-in): parking space and flags, one slot per chunk stream
        if (c->plan.wino_streamk) {
            hipDeviceProp_t prop;
            HIP_TRY(hipGetDeviceProperties(&prop, c->cfg.device));
            c->n_cu = prop.multiProcessorCount;
            if ((rc = dev_alloc(c, &c->wino_ws, (size_t)4 * c->n_cu * HPE_WINO_WS_FLOATS, false))) return rc;
            float* fl = nullptr;
            if ((rc = dev_alloc(c, &fl, (size_t)4 * c->n_cu + 4, true))) return rc;
            c->wino_flags = reinterpret_cast<unsigned*>(fl);
            c->dev_err = c->wino_flags + (size_t)4 * c->n_cu;
        }
    }
    {
        c->partial_floats = (size_t)512 * 128 * 128;  // 512 slices of the largest tile (32 MB)
        if ((rc = dev_alloc(c, &c->partial, c->partial_floats, false))) return rc;
        c->partial_tail_floats = (size_t)64 * 128 * 128;  // Dense layers: <= 16 slices of <= 64 tiles of 64 x 64 (4 MB)
        if ((rc = dev_alloc(c, &c->partial_tail, c->partial_tail_floats, false))) return rc;
    }
    if (c->have_regressor) {
        if ((rc = dev_alloc(c, &c->P1, B * 1024, true))) return rc;
        if ((rc = dev_alloc(c, &c->H1, B * 1024, true))) return rc;
        if ((rc = dev_alloc(c, &c->H2, B * 1024, true))) return rc;
        if ((rc = dev_alloc(c, &c->thA, B * THETA_LD, true))) return rc;
        if ((rc = dev_alloc(c, &c->thB, B * THETA_LD, true))) return rc;
        // hpe_regressor_forward_train / hpe_regressor_backward: their own workspace, split-K slices included
        const size_t S = (size_t)c->cfg.num_stage;
        RegTrainWork& t = c->rt;
        if ((rc = dev_alloc(c, &t.p1, B * 1024, true))) return rc;
        if ((rc = dev_alloc(c, &t.a1, S * B * 1024, true))) return rc;
        if ((rc = dev_alloc(c, &t.a2, S * B * 1024, true))) return rc;
        if ((rc = dev_alloc(c, &t.th, (S + 1) * B * THETA_LD, true))) return rc;
        if ((rc = dev_alloc(c, &t.g, (S + 1) * B * THETA_LD, true))) return rc;
        if ((rc = dev_alloc(c, &t.r, B * THETA_LD, true))) return rc;
        if ((rc = dev_alloc(c, &t.da, B * 1024, true))) return rc;
        if ((rc = dev_alloc(c, &t.dz1, S * B * 1024, true))) return rc;
        if ((rc = dev_alloc(c, &t.dz2, S * B * 1024, true))) return rc;
        if ((rc = dev_alloc(c, &t.sum1, B * 1024, true))) return rc;
        if ((rc = dev_alloc(c, &t.zeros, 2048, true))) return rc;
        t.partial_floats = c->partial_tail_floats;
        if ((rc = dev_alloc(c, &t.partial, t.partial_floats, false))) return rc;
    }
    if (c->have_smpl) {
        if ((rc = dev_alloc(c, &c->work.pfT, 207 * Bpad, true))) return rc;
        if ((rc = dev_alloc(c, &c->work.betaT, 10 * Bpad, true))) return rc;
        if ((rc = dev_alloc(c, &c->work.A, Bpad * 288, true))) return rc;
        if ((rc = dev_alloc(c, &c->work.cams, Bpad * 4, true))) return rc;
        if ((rc = dev_alloc(c, &c->work.verts_tmp, B * HPE_NUM_VERTS * 3, false))) return rc;
        if ((rc = dev_alloc(c, &c->work.kp_part, (size_t)SMPL_SMALL_B * ((HPE_NUM_VERTS + 63) / 64) * 72, true))) return rc;
        // hpe_smpl_backward recomputes the forward's per-image operands into buffers of its own
        if ((rc = dev_alloc(c, &c->bwd.pfT, 207 * Bpad, true))) return rc;
        if ((rc = dev_alloc(c, &c->bwd.betaT, 10 * Bpad, true))) return rc;
        if ((rc = dev_alloc(c, &c->bwd.A, Bpad * 288, true))) return rc;
        if ((rc = dev_alloc(c, &c->bwd.cams, Bpad * 4, true))) return rc;
        if ((rc = dev_alloc(c, &c->bwd.rjg, Bpad * 576, true))) return rc;
        if ((rc = dev_alloc(c, &c->bwd.gj, Bpad * 120, true))) return rc;
        if ((rc = dev_alloc(c, &c->bwd.part, hpe_smpl_bwd_part_floats((int)Bpad), true))) return rc;
        // reprojection-loss workspace for the geometry the path itself produces (config 5); other sizes grow it on demand
        c->loss_ws_floats = hpe_mesh_loss_ws_floats(c->cfg.max_batch, HPE_IMG_SIZE, HPE_IMG_SIZE, HPE_NUM_VERTS);
        if ((rc = dev_alloc(c, &c->loss_ws, c->loss_ws_floats, true))) return rc;
    }
    c->work.Bpad = (int)Bpad;
    c->bwd.Bpad = (int)Bpad;
    return HPE_OK;
}

// ---- chunk streams, the tail stream and the events of the fork / join, the software pipeline and the timing hooks
static int create_streams_and_events(hpe_ctx* c) {
    for (int i = 0; i < c->plan.n_streams - 1; ++i) HIP_TRY(hipStreamCreateWithFlags(&c->aux[i], hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
    HIP_TRY(hipStreamCreateWithFlags(&c->tail_st, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&c->ev_enc, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&c->ev_tail, hipEventDisableTiming));
    for (auto& ev : c->ev_feat_free) HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    for (auto& ev : c->ev_join) HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    for (auto& e : c->ev) HIP_TRY(hipEventCreate(&e));
    for (auto& e : c->span0) HIP_TRY(hipEventCreate(&e));
    for (auto& e : c->span1) HIP_TRY(hipEventCreate(&e));
    for (auto& e : c->cev0) HIP_TRY(hipEventCreate(&e));
    for (auto& e : c->cev1) HIP_TRY(hipEventCreate(&e));
    for (auto& e : c->lev0) HIP_TRY(hipEventCreate(&e));
    for (auto& e : c->lev1) HIP_TRY(hipEventCreate(&e));
    for (auto& e : c->lev_all) HIP_TRY(hipEventCreate(&e));
    c->ev_ok = true;
    return HPE_OK;
}

int repack_encoder(hpe_ctx* c) {
    int rc;
    if ((rc = pack_dual_weights(c))) return rc;
    return pack_conv_weights(c);
}

int finalize_impl(hpe_ctx* c) {
    int rc = check_loaded(c);
    if (rc) return rc;
    DeviceGuard g(c->cfg.device);
    c->plan = hpe_resolve_plan(c->cfg);
    // per-device function attributes (dynamic LDS above 64 KB) of the Winograd, stem and loss kernels
    HIP_TRY(hpe_wino_init_device());
    HIP_TRY(hpe_wino4_init_device());
    HIP_TRY(hpe_stem_fused_init_device());
    HIP_TRY(hpe_losses_init_device());
    c->loss_attr_done = true;
    if (c->have_encoder && (rc = pack_dual_weights(c))) return rc;
    if (c->have_encoder && (rc = pack_conv_weights(c))) return rc;
    // constants every part uses: the zero page is the LDS-DMA source of out-of-image taps / halo pixels
    if ((rc = upload(c, &c->ones, std::vector<float>(2048, 1.f)))) return rc;
    if ((rc = upload(c, &c->zeros, std::vector<float>(1024, 0.f)))) return rc;
    if (c->have_regressor && (rc = pack_regressor(c))) return rc;
    if (c->have_smpl && (rc = pack_smpl(c))) return rc;
    if ((rc = size_workspaces(c))) return rc;
    if ((rc = create_streams_and_events(c))) return rc;
    HIP_TRY(hipDeviceSynchronize());
    c->finalized = true;
    return HPE_OK;
}
