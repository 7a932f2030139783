// hpe_api.hip -- the extern "C" entry points of include/hpe.h: argument checks, then a call into hpe_finalize.hip / hpe_encoder.hip / the
// launchers; debug and timing hooks.  The renderer's entry points are in hpe_render_api.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
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
thread_local std::string g_err;
}

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

int check_ready(hpe_ctx* c, int B, int need) {
    if (!c) return fail(HPE_ERR_INVALID, "null ctx");
    if (c->dead) return fail(HPE_ERR_STATE, "hpe_finalize failed on this ctx: destroy it and create a new one");
    if (!c->finalized) return fail(HPE_ERR_STATE, "hpe_finalize() has not been called");
    if (B < 1 || B > c->cfg.max_batch) return fail(HPE_ERR_INVALID, "batch " + std::to_string(B) + " outside [1, max_batch]");
    if ((need & NEED_ENC) && !c->have_encoder) return fail(HPE_ERR_STATE, "encoder weights were not loaded before hpe_finalize");
    if ((need & NEED_REG) && !c->have_regressor) return fail(HPE_ERR_STATE, "regressor weights / mean theta were not loaded");
    if ((need & NEED_SMPL) && !c->have_smpl) return fail(HPE_ERR_STATE, "SMPL model was not loaded before hpe_finalize");
    return HPE_OK;
}

#pragma GCC visibility push(default)
extern "C" {


const char* hpe_last_error(void) { return g_err.c_str(); }
const char* hpe_version(void) { return "hpe_hip 0.1 (gfx950)"; }

const char* hpe_conv_layer_name(int idx) { return (idx >= 0 && idx < HPE_NUM_CONV) ? specs()[idx].name : nullptr; }
const char* hpe_bn_layer_name(int idx) { return (idx >= 0 && idx < HPE_NUM_CONV) ? specs()[idx].bn : nullptr; }

int hpe_conv_layer_geometry(int idx, int out[7]) {
    if (idx < 0 || idx >= HPE_NUM_CONV || !out) return fail(HPE_ERR_INVALID, "bad conv index");
    const ConvSpec& s = specs()[idx];
    out[0] = s.kh;
    out[1] = s.kw;
    out[2] = s.cin;
    out[3] = s.cout;
    out[4] = s.stride;
    out[5] = s.hin;
    out[6] = s.hout;
    return HPE_OK;
}

void hpe_config_init(HpeConfig* cfg) {
    if (!cfg) return;
    cfg->struct_size = (int)sizeof(HpeConfig);
    cfg->device = 0;
    cfg->max_batch = 8;
    cfg->num_stage = 3;
    cfg->bn_eps = 1e-3f;
    cfg->encoder_dtype = 0;
    cfg->n_streams = cfg->dual_gemm = cfg->stem_fused = cfg->wino_min_c = cfg->wino_min_items = cfg->wino_fused = -1;
    cfg->wino_fused_min_hw = cfg->mesh_a2b = cfg->wino_f4 = cfg->wino4_fused = cfg->bf16_p8 = cfg->wino4_ksplit = cfg->chain_fuse = cfg->halo3 = cfg->f32_split = -1;
}

int hpe_create(const HpeConfig* cfg, hpe_ctx** out) {
    if (!cfg || !out) return fail(HPE_ERR_INVALID, "null argument");
    // The struct has grown every round: a caller built against another header (or one that zero-initialised the struct instead of
    // calling hpe_config_init) is refused here instead of having plan options read from past the end of its struct.
    if (cfg->struct_size != (int)sizeof(HpeConfig))
        return fail(HPE_ERR_INVALID, "HpeConfig.struct_size is " + std::to_string(cfg->struct_size) + ", this library expects " +
                                         std::to_string(sizeof(HpeConfig)) + ": fill the struct with hpe_config_init() of the same header");
    if (cfg->n_streams > 4 || cfg->n_streams == 0) return fail(HPE_ERR_INVALID, "n_streams must be -1 (default) or 1..4");
    if (cfg->mesh_a2b > 2) return fail(HPE_ERR_INVALID, "mesh_a2b must be -1 (default), 0 (grid), 1 (valu) or 2 (mfma)");
    if (cfg->max_batch < 1 || cfg->max_batch > 1024) return fail(HPE_ERR_INVALID, "max_batch must be in [1,1024]");
    if (cfg->num_stage < 1 || cfg->num_stage > 16) return fail(HPE_ERR_INVALID, "num_stage must be in [1,16]");
    if (cfg->encoder_dtype != 0 && cfg->encoder_dtype != 1) return fail(HPE_ERR_INVALID, "encoder_dtype must be 0 (fp32) or 1 (bf16)");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(HPE_ERR_NO_DEVICE, "no HIP device visible");
    if (cfg->device < 0 || cfg->device >= ndev) return fail(HPE_ERR_INVALID, "device ordinal out of range");
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, cfg->device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(HPE_ERR_NO_DEVICE, std::string("device is ") + prop.gcnArchName + ", kernels are built for gfx950 only");
    hpe_ctx* c = new hpe_ctx();
    c->cfg = *cfg;
    c->bf16 = cfg->encoder_dtype == 1;
    if (c->cfg.bn_eps <= 0.f) c->cfg.bn_eps = 1e-3f;
    *out = c;
    return HPE_OK;
}

int hpe_destroy(hpe_ctx* c) {
    if (!c) return HPE_OK;
    DeviceGuard g(c->cfg.device);
    (void)hipDeviceSynchronize();
    release_device_state(c);
    delete c;
    return HPE_OK;
}

int hpe_finalize(hpe_ctx* c) {
    if (!c) return fail(HPE_ERR_INVALID, "null ctx");
    if (c->dead) return fail(HPE_ERR_STATE, "an earlier hpe_finalize failed: destroy this ctx and create a new one");
    if (c->finalized) return fail(HPE_ERR_STATE, "already finalized");
    const int rc = finalize_impl(c);
    if (rc != HPE_OK && rc != HPE_ERR_STATE) {
        // a device-side failure part-way (out of memory, ...): nothing of the half-built state survives, so a retry cannot
        // leak it or double-allocate (the thread-local error message of the failing call is kept)
        const std::string keep = g_err;
        DeviceGuard g(c->cfg.device);
        (void)hipDeviceSynchronize();
        release_device_state(c);
        c->dead = true;
        g_err = keep;
    }
    return rc;
}

int hpe_encoder(hpe_ctx* c, const float* images, int B, float* features, void* stream) {
    int rc = check_ready(c, B, NEED_ENC);
    if (rc) return rc;
    if (!images || !features) return fail(HPE_ERR_INVALID, "null pointer");
    DeviceGuard g(c->cfg.device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (c->timing) {
        HIP_TRY(hipEventRecord(c->ev[0], st));
        HIP_TRY(hipEventRecord(c->span0[c->span_n % hpe_ctx::SPAN_RING], st));
    }
    HIP_TRY(encoder_impl(c, images, B, features, HPE_FEATURE_DIM, st));
    if (c->timing) {
        HIP_TRY(hipEventRecord(c->span1[c->span_n % hpe_ctx::SPAN_RING], st));
        ++c->span_n;
        HIP_TRY(hipEventRecord(c->ev[1], st));
        HIP_TRY(hipEventRecord(c->ev[4], st));
        c->timed_valid = true;
        c->conv_timed_valid = c->timing >= 2;
    }
    return HPE_OK;
}

int hpe_regress_stage(hpe_ctx* c, const float* features, const float* theta_prev, int B, float* theta_out, void* stream) {
    int rc = check_ready(c, B, NEED_REG);
    if (rc) return rc;
    if (!features || !theta_out) return fail(HPE_ERR_INVALID, "null pointer");
    DeviceGuard g(c->cfg.device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIP_TRY(join_tail(c, st));  // shares the regressor buffers with a pipelined call's tail
    HIP_TRY(features_proj(c, features, B, st));
    if (theta_prev)
        HIP_TRY(hpe_launch_copy_theta(theta_prev, HPE_THETA_DIM, c->thA, THETA_LD, B, HPE_THETA_DIM, st));
    else
        HIP_TRY(hpe_launch_tile_theta(c->mean_dev, c->thA, B, THETA_LD, st));
    HIP_TRY(regress_impl(c, c->thA, c->thB, B, st));
    HIP_TRY(hpe_launch_copy_theta(c->thB, THETA_LD, theta_out, HPE_THETA_DIM, B, HPE_THETA_DIM, st));
    return HPE_OK;
}

int hpe_smpl(hpe_ctx* c, const float* theta, int B, const HpeOutputs* outs, void* stream) {
    int rc = check_ready(c, B, NEED_SMPL);
    if (rc) return rc;
    if (!theta || !outs) return fail(HPE_ERR_INVALID, "null pointer");
    DeviceGuard g(c->cfg.device);
    HIP_TRY(join_tail(c, static_cast<hipStream_t>(stream)));  // shares the SMPL work buffers with a pipelined call's tail
    HIP_TRY(hpe_launch_smpl(c->smpl, c->work, theta, HPE_THETA_DIM, B, outs, static_cast<hipStream_t>(stream)));
    return HPE_OK;
}

int hpe_smpl_backward(hpe_ctx* c, const float* theta, int B, const HpeOutputs* grad_outs, float* grad_theta, void* stream) {
    int rc = check_ready(c, B, NEED_SMPL);
    if (rc) return rc;
    if (!theta || !grad_outs || !grad_theta) return fail(HPE_ERR_INVALID, "null pointer");
    DeviceGuard g(c->cfg.device);
    HIP_TRY(hpe_launch_smpl_backward(c->smpl, c->bwd, theta, B, grad_outs, grad_theta, static_cast<hipStream_t>(stream)));
    return HPE_OK;
}

int hpe_forward(hpe_ctx* c, const float* images, int B, const HpeOutputs* stage_outs, int n_outs, void* stream) {
    return forward_impl(c, images, B, stage_outs, n_outs, static_cast<hipStream_t>(stream), false);
}

int hpe_forward_pipelined(hpe_ctx* c, const float* images, int B, const HpeOutputs* stage_outs, int n_outs, void* stream) {
    return forward_impl(c, images, B, stage_outs, n_outs, static_cast<hipStream_t>(stream), true);
}

int hpe_tail(hpe_ctx* c, const float* features, int B, const HpeOutputs* stage_outs, int n_outs, void* stream) {
    int rc = check_ready(c, B, NEED_REG | NEED_SMPL);
    if (rc) return rc;
    if (!features || !stage_outs) return fail(HPE_ERR_INVALID, "null pointer");
    if (n_outs < 1 || n_outs > c->cfg.num_stage) return fail(HPE_ERR_INVALID, "n_outs must be in [1, num_stage]");
    DeviceGuard g(c->cfg.device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIP_TRY(join_tail(c, st));  // shares the regressor / SMPL buffers with a pipelined call's tail
    c->dense_on_tail = true;  // its own split-K workspace: may overlap hpe_encoder of the next batch
    const hipError_t e = tail_impl(c, features, B, stage_outs, n_outs, st, nullptr);
    c->dense_on_tail = false;
    if (e != hipSuccess) return fail(HPE_ERR_HIP, std::string("hpe_tail: ") + hipGetErrorString(e));
    return HPE_OK;
}

int hpe_join(hpe_ctx* c, void* stream) {
    if (!c || !c->finalized) return fail(HPE_ERR_STATE, "needs a finalized ctx");
    DeviceGuard g(c->cfg.device);
    if (c->tail_pending) HIP_TRY(hipStreamWaitEvent(static_cast<hipStream_t>(stream), c->ev_tail, 0));
    return HPE_OK;
}

void* hpe_tail_stream(hpe_ctx* c) { return (c && c->finalized) ? static_cast<void*>(c->tail_st) : nullptr; }

int hpe_orth_proj(const float* X, const float* cam, int B, int P, float* out, void* stream) {
    if (!X || !cam || !out || B < 1 || P < 1) return fail(HPE_ERR_INVALID, "bad argument");
    HIP_TRY(hpe_launch_orth_proj(X, cam, B, P, 0.f, 0.f, 0, out, static_cast<hipStream_t>(stream)));
    return HPE_OK;
}

int hpe_reproject_vertices(const float* verts, const float* cam, int B, int P, float im_w, float im_h, float* out, void* stream) {
    if (!verts || !cam || !out || B < 1 || P < 1) return fail(HPE_ERR_INVALID, "bad argument");
    HIP_TRY(hpe_launch_orth_proj(verts, cam, B, P, im_w, im_h, 1, out, static_cast<hipStream_t>(stream)));
    return HPE_OK;
}

// preview.py:22-29 / image.py:7-15,17-39 -- all index arithmetic in double like numpy; false if the frame is too thin
static bool preprocess_geometry(int H, int W, PreprocFrame* f, int proc_param[5]) {
    const int S = HPE_IMG_SIZE;
    const int mx = H > W ? H : W;
    const double scale = (mx != S) ? ((double)S / (double)mx) : 1.0;
    const int newH = (int)std::floor(H * scale), newW = (int)std::floor(W * scale);
    if (newH < 1 || newW < 1) return false;
    const double fy = (double)newH / (double)H, fx = (double)newW / (double)W;  // actual_factor [y, x]
    const double cy = std::nearbyint(H / 2.0), cx = std::nearbyint(W / 2.0);     // np.round: half to even
    const int csx = (int)std::nearbyint(cx * fx), csy = (int)std::nearbyint(cy * fy);
    const int margin = S / 2;
    const int start_x = csx + margin - margin, start_y = csy + margin - margin;  // center_pad - margin
    proc_param[0] = start_x;
    proc_param[1] = start_y;
    proc_param[2] = start_x + 2 * margin;
    proc_param[3] = start_y + 2 * margin;
    proc_param[4] = S;
    f->H = H;
    f->W = W;
    f->newH = newH;
    f->newW = newW;
    f->start_x = start_x;
    f->start_y = start_y;
    return true;
}

int hpe_preprocess_u8(const unsigned char* img, int H, int W, int C, float* out224, int proc_param[5], void* stream) {
    if (!img || !out224 || !proc_param || H < 1 || W < 1 || (C != 3 && C != 4)) return fail(HPE_ERR_INVALID, "bad argument");
    PreprocFrame f{};
    if (!preprocess_geometry(H, W, &f, proc_param)) return fail(HPE_ERR_INVALID, "image too thin");
    HIP_TRY(hpe_launch_preprocess_u8(img, H, W, C, f.newH, f.newW, f.start_x, f.start_y, HPE_IMG_SIZE / 2, out224, HPE_IMG_SIZE,
                                     static_cast<hipStream_t>(stream)));
    return HPE_OK;
}

int hpe_preprocess_u8_batch(const unsigned char* frames, const long long* offsets, const int* sizes_hw, int B, int C, float* out,
                            int* proc_params, void* table_dev, void* stream) {
    if (!frames || !sizes_hw || !out || !proc_params || B < 1 || (C != 3 && C != 4)) return fail(HPE_ERR_INVALID, "bad argument");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (!offsets) {
        PreprocFrame f{};
        if (sizes_hw[0] < 1 || sizes_hw[1] < 1 || !preprocess_geometry(sizes_hw[0], sizes_hw[1], &f, proc_params))
            return fail(HPE_ERR_INVALID, "bad frame size");
        for (int b = 1; b < B; ++b) memcpy(proc_params + 5 * b, proc_params, 5 * sizeof(int));
        HIP_TRY(hpe_launch_preprocess_u8_batch(frames, nullptr, f, B, C, HPE_IMG_SIZE / 2, out, HPE_IMG_SIZE, st));
        return HPE_OK;
    }
    if (!table_dev) return fail(HPE_ERR_INVALID, "per-image sizes need table_dev (32 * B bytes of device scratch)");
    static_assert(sizeof(PreprocFrame) == 32, "table_dev is documented as 32 bytes per frame");
    std::vector<PreprocFrame> tab((size_t)B);
    for (int b = 0; b < B; ++b) {
        if (offsets[b] < 0 || sizes_hw[2 * b] < 1 || sizes_hw[2 * b + 1] < 1 ||
            !preprocess_geometry(sizes_hw[2 * b], sizes_hw[2 * b + 1], &tab[b], proc_params + 5 * b))
            return fail(HPE_ERR_INVALID, "bad frame " + std::to_string(b));
        tab[b].offset = offsets[b];
    }
    // pageable source: the runtime stages the bytes before it returns, so `tab` may die at the end of this call
    // The table lives on this call's stack: the copy must have READ it before the call returns.  hipMemcpyAsync from pageable memory
    // happens to stage the bytes before returning on this runtime, but that is not a contract of the API -- so: wait for the work already
    // on `st` (the scratch may still be read by an earlier launch), then a synchronous copy.  This path (frames of different sizes) is
    // host-blocking and cannot be captured; the uniform-size path above needs no table at all.
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipMemcpy(table_dev, tab.data(), tab.size() * sizeof(PreprocFrame), hipMemcpyHostToDevice));
    HIP_TRY(hpe_launch_preprocess_u8_batch(frames, static_cast<const PreprocFrame*>(table_dev), PreprocFrame{}, B, C, HPE_IMG_SIZE / 2, out,
                                           HPE_IMG_SIZE, st));
    return HPE_OK;
}

int hpe_get_original(const float* verts, const float* cam, int B, int P, int K, const int start_pt[2], float scale, int img_size,
                     float* vert_shifted, float cam_for_render[3], float* kp_original_host, const float* joints2d_host,
                     void* stream) {
    if (!verts || !cam || !vert_shifted || !cam_for_render || !start_pt || B < 1 || P < 1 || scale <= 0.f || img_size < 1)
        return fail(HPE_ERR_INVALID, "bad argument");
    const float flength = 500.f;
    const float undo = 1.f / scale;
    HIP_TRY(hpe_launch_shift_verts(verts, cam, B, P, flength, (float)img_size, vert_shifted, static_cast<hipStream_t>(stream)));
    // renderer.py:273-276
    const float pp = img_size / 2.f;
    cam_for_render[0] = flength * undo;
    cam_for_render[1] = (pp + (start_pt[0] - 0.5f * img_size)) * undo;
    cam_for_render[2] = (pp + (start_pt[1] - 0.5f * img_size)) * undo;
    // renderer.py:281-282: kp_original = (joints + start_pt - margin) * undo_scale (host arrays, K x 2 per image)
    if (kp_original_host && joints2d_host) {
        const int margin = img_size / 2;
        for (int i = 0; i < B * K; ++i) {
            kp_original_host[2 * i] = (joints2d_host[2 * i] + start_pt[0] - margin) * undo;
            kp_original_host[2 * i + 1] = (joints2d_host[2 * i + 1] + start_pt[1] - margin) * undo;
        }
    }
    return HPE_OK;
}

int hpe_kp_loss(const float* kp_gt, const float* kp_pred, int B, int K, float* out, void* stream) {
    if (!kp_gt || !kp_pred || !out || B < 1 || K < 1) return fail(HPE_ERR_INVALID, "bad argument");
    HIP_TRY(hpe_launch_kp_loss(kp_gt, kp_pred, B * K, out, static_cast<hipStream_t>(stream)));
    return HPE_OK;
}

int hpe_kp_loss_backward(const float* kp_gt, const float* kp_pred, int B, int K, const float* grad_loss, float* grad_kp_pred, void* stream) {
    if (!kp_gt || !kp_pred || !grad_kp_pred || B < 1 || K < 1) return fail(HPE_ERR_INVALID, "bad argument");
    HIP_TRY(hpe_launch_kp_loss_backward(kp_gt, kp_pred, B * K, grad_loss, grad_kp_pred, static_cast<hipStream_t>(stream)));
    return HPE_OK;
}

// Loss workspace: sized in hpe_finalize for max_batch images of 224 x 224 and 6890 vertices (what the path produces); any
// other geometry grows it here -- the one case in which a compute call synchronises (documented in hpe.h).
static int ensure_loss_ws(hpe_ctx* c, int B, int H, int W, int P) {
    if (!c->loss_attr_done) {
        // a ctx that was never finalized (loss operators only): the search kernel's dynamic-LDS attribute is set here
        HIP_TRY(hpe_losses_init_device());
        c->plan = hpe_resolve_plan(c->cfg);
        c->loss_attr_done = true;
    }
    const size_t need = hpe_mesh_loss_ws_floats(B, H, W, P);
    if (need <= c->loss_ws_floats) return HPE_OK;
    HIP_TRY(hipDeviceSynchronize());
    if (c->loss_ws) {
        for (auto it = c->allocs.begin(); it != c->allocs.end(); ++it)
            if (*it == c->loss_ws) {
                c->allocs.erase(it);
                break;
            }
        (void)hipFree(c->loss_ws);
        c->loss_ws = nullptr;
        c->loss_ws_floats = 0;
    }
    float* p = nullptr;
    int rc = dev_alloc(c, &p, need, true);
    if (rc) return rc;
    c->loss_ws = p;
    c->loss_ws_floats = need;
    return HPE_OK;
}

int hpe_mesh_loss(hpe_ctx* c, const float* seg, const float* verts2d, int B, int H, int W, int P, float* out, void* stream) {
    if (!c) return fail(HPE_ERR_INVALID, "null ctx");
    if (!seg || !verts2d || !out || B < 1 || H < 1 || W < 1 || P < 1) return fail(HPE_ERR_INVALID, "bad argument");
    DeviceGuard g(c->cfg.device);
    int rc = ensure_loss_ws(c, B, H, W, P);
    if (rc) return rc;
    HIP_TRY(hpe_launch_mesh_loss(seg, verts2d, B, H, W, P, c->loss_ws, out, static_cast<hipStream_t>(stream), c->plan.mesh_a2b, c->loss_counter));
    return HPE_OK;
}

int hpe_mesh_loss_grad(hpe_ctx* c, const float* seg, const float* verts2d, int B, int H, int W, int P, float* out, float* grad_verts2d,
                       int* nn_pix, int* nn_vert, void* stream) {
    if (!c) return fail(HPE_ERR_INVALID, "null ctx");
    if (!seg || !verts2d || !out || B < 1 || H < 1 || W < 1 || P < 1) return fail(HPE_ERR_INVALID, "bad argument");
    if (!grad_verts2d) return fail(HPE_ERR_INVALID, "hpe_mesh_loss_grad needs grad_verts2d_dev (hpe_mesh_loss is the loss-only call)");
    DeviceGuard g(c->cfg.device);
    int rc = ensure_loss_ws(c, B, H, W, P);
    if (rc) return rc;
    HIP_TRY(hpe_launch_mesh_loss_grad(seg, verts2d, B, H, W, P, c->loss_ws, out, grad_verts2d, nn_pix, nn_vert, static_cast<hipStream_t>(stream),
                                      c->plan.mesh_a2b, c->loss_counter));
    return HPE_OK;
}

int hpe_val_losses(hpe_ctx* c, const float* seg, const float* kp_gt, const float* const* kp2d, const float* const* verts2d, int n_stage,
                   int B, int K, int H, int W, int P, float* out, void* stream) {
    if (!c) return fail(HPE_ERR_INVALID, "null ctx");
    if (!kp_gt || !kp2d || !out || n_stage < 1 || n_stage > 16 || B < 1 || K < 1) return fail(HPE_ERR_INVALID, "bad argument");
    const bool mesh = seg && verts2d;
    if (mesh && (H < 1 || W < 1 || P < 1)) return fail(HPE_ERR_INVALID, "bad silhouette / vertex geometry");
    for (int s = 0; s < n_stage; ++s)
        if (!kp2d[s] || (mesh && !verts2d[s])) return fail(HPE_ERR_INVALID, "null stage pointer");
    DeviceGuard g(c->cfg.device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool tm = c->timing != 0 && c->ev_ok;
    c->loss_timed_stages = 0;
    if (tm) HIP_TRY(hipEventRecord(c->lev_all[0], st));
    if (mesh) {
        int rc = ensure_loss_ws(c, B, H, W, P);
        if (rc) return rc;
        HIP_TRY(hpe_launch_mesh_loss_prepare(seg, B, H, W, P, c->loss_ws, st));
    }
    for (int s = 0; s < n_stage; ++s) {
        HIP_TRY(hpe_launch_kp_loss(kp_gt, kp2d[s], B * K, out + 4 * s, st));  // writes out[4s .. 4s+2]
        if (mesh)
            HIP_TRY(hpe_launch_mesh_loss_search(verts2d[s], B, H, W, P, c->loss_ws, out + 4 * s + 3, st, tm ? c->lev0[s] : nullptr,
                                                tm ? c->lev1[s] : nullptr, c->plan.mesh_a2b, c->loss_counter));
        else
            HIP_TRY(hipMemsetAsync(out + 4 * s + 3, 0, sizeof(float), st));
    }
    if (tm) {
        HIP_TRY(hipEventRecord(c->lev_all[1], st));
        c->loss_timed_stages = mesh ? n_stage : -1;
    }
    return HPE_OK;
}

const char* hpe_critic_layer_name(int idx) { return (idx >= 0 && idx < HPE_NUM_CRITIC_DENSE) ? hpe_critic_layers()[idx].name : nullptr; }

int hpe_critic_layer_shape(int idx, int out[2]) {
    if (idx < 0 || idx >= HPE_NUM_CRITIC_DENSE || !out) return fail(HPE_ERR_INVALID, "bad critic layer index");
    out[0] = hpe_critic_layers()[idx].in;
    out[1] = hpe_critic_layers()[idx].out;
    return HPE_OK;
}

int hpe_load_critic(hpe_ctx* c, const HpeCriticModel* m) {
    if (!c || !m) return fail(HPE_ERR_INVALID, "null argument");
    if (c->dead) return fail(HPE_ERR_STATE, "hpe_finalize failed on this ctx: destroy it and create a new one");
    for (int i = 0; i < HPE_NUM_CRITIC_DENSE; ++i)
        if (!m->kernel[i] || !m->bias[i])
            return fail(HPE_ERR_INVALID, std::string("critic layer ") + hpe_critic_layers()[i].name + ": null kernel or bias");
    // the flat layout (kernel 0 | bias 0 | kernel 1 | ...); the live layout is written from it by the one kernel that states it
    std::vector<float> flat((size_t)CRITIC_PARAM_FLOATS);
    for (int l = 0; l < HPE_NUM_CRITIC_DENSE; ++l) {
        const int kn = hpe_critic_layers()[l].in * hpe_critic_layers()[l].out;
        std::copy(m->kernel[l], m->kernel[l] + kn, flat.begin() + hpe_critic_flat_offset(l, false));
        std::copy(m->bias[l], m->bias[l] + hpe_critic_layers()[l].out, flat.begin() + hpe_critic_flat_offset(l, true));
    }
    DeviceGuard g(c->cfg.device);
    HIP_TRY(hipDeviceSynchronize());  // a call still running may read the weights that are about to be replaced
    if (!c->critic_buf) {
        void* q = nullptr;
        HIP_TRY(hipMalloc(&q, hpe_critic_live_floats() * sizeof(float)));
        c->critic_buf = static_cast<float*>(q);
        c->critic = hpe_critic_live_view(c->critic_buf);
    }
    // the set kernel writes the live elements only: the padding between the 16-byte aligned blocks is zero from here
    HIP_TRY(hipMemset(c->critic_buf, 0, hpe_critic_live_floats() * sizeof(float)));
    void* tmp = nullptr;
    HIP_TRY(hipMalloc(&tmp, flat.size() * sizeof(float)));
    hipError_t e = hipMemcpy(tmp, flat.data(), flat.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hpe_launch_critic_params(c->critic, static_cast<float*>(tmp), true, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    (void)hipFree(tmp);
    HIP_TRY(e);
    c->have_critic = true;
    return HPE_OK;
}

// what every critic entry point checks first; loaded: the call needs the weights
static int check_critic_ctx(hpe_ctx* c, bool loaded) {
    if (!c) return fail(HPE_ERR_INVALID, "null ctx");
    if (c->dead) return fail(HPE_ERR_STATE, "hpe_finalize failed on this ctx: destroy it and create a new one");
    if (loaded && !c->have_critic) return fail(HPE_ERR_STATE, "no critic loaded (hpe_load_critic)");
    return HPE_OK;
}

static int check_critic(hpe_ctx* c, const float* joints, int K, const float* betas, int betas_stride, const float* Rs, int N) {
    int rc = check_critic_ctx(c, true);
    if (rc) return rc;
    if (!joints || !betas || !Rs) return fail(HPE_ERR_INVALID, "null pointer");
    if (K < 14 || K > HPE_MAX_KP) return fail(HPE_ERR_INVALID, "joints must be [N,K,3] with 14 <= K <= " + std::to_string(HPE_MAX_KP));
    if (betas_stride < HPE_NUM_BETAS) return fail(HPE_ERR_INVALID, "betas_stride must be >= 10");
    if (N < 1) return fail(HPE_ERR_INVALID, "N must be >= 1");
    return HPE_OK;
}

int hpe_critic(hpe_ctx* c, const float* joints, int K, const float* betas, int betas_stride, const float* Rs, int N, float* scores,
               float* kcs, void* stream) {
    int rc = check_critic(c, joints, K, betas, betas_stride, Rs, N);
    if (rc) return rc;
    if (!scores) return fail(HPE_ERR_INVALID, "null scores_dev");
    DeviceGuard g(c->cfg.device);
    HIP_TRY(hpe_launch_critic(c->critic, joints, K, betas, betas_stride, Rs, N, scores, kcs, static_cast<hipStream_t>(stream)));
    return HPE_OK;
}

int hpe_critic_backward(hpe_ctx* c, const float* joints, int K, const float* betas, int betas_stride, const float* Rs, int N,
                        const float* grad_scores, float* grad_joints, float* grad_betas, float* grad_Rs, float* grad_kcs, void* stream) {
    int rc = check_critic(c, joints, K, betas, betas_stride, Rs, N);
    if (rc) return rc;
    if (!grad_joints && !grad_betas && !grad_Rs && !grad_kcs) return fail(HPE_ERR_INVALID, "hpe_critic_backward: every output is NULL");
    DeviceGuard g(c->cfg.device);
    HIP_TRY(hpe_launch_critic_backward(c->critic, joints, K, betas, betas_stride, Rs, N, grad_scores, grad_joints, grad_betas, grad_Rs,
                                       grad_kcs, static_cast<hipStream_t>(stream)));
    return HPE_OK;
}

int hpe_critic_param_floats(void) { return CRITIC_PARAM_FLOATS; }

int hpe_critic_param_offset(int idx, int is_bias) {
    if (idx < 0 || idx >= HPE_NUM_CRITIC_DENSE) return -1;
    return hpe_critic_flat_offset(idx, is_bias != 0);
}

long long hpe_critic_weight_grad_ws_floats(int N) { return N < 1 ? 0 : (long long)hpe_critic_wg_ws_floats(N); }

// Workspace of hpe_critic_weight_grad: grown here, with a device synchronisation, when a call needs more than the ctx holds
static int ensure_critic_ws(hpe_ctx* c, int N) {
    const size_t need = hpe_critic_wg_ws_floats(N);
    if (need <= c->critic_ws_floats) return HPE_OK;
    HIP_TRY(hipDeviceSynchronize());
    if (c->critic_ws) {
        (void)hipFree(c->critic_ws);
        c->critic_ws = nullptr;
        c->critic_ws_floats = 0;
    }
    void* q = nullptr;
    HIP_TRY(hipMalloc(&q, need * sizeof(float)));
    c->critic_ws = static_cast<float*>(q);
    c->critic_ws_floats = need;
    return HPE_OK;
}

int hpe_critic_reserve(hpe_ctx* c, int N) {
    int rc = check_critic_ctx(c, false);
    if (rc) return rc;
    if (N < 1) return fail(HPE_ERR_INVALID, "N must be >= 1");
    DeviceGuard g(c->cfg.device);
    return ensure_critic_ws(c, N);
}

int hpe_critic_weight_grad(hpe_ctx* c, const float* joints, int K, const float* betas, int betas_stride, const float* Rs, int N,
                           const float* grad_scores, const float* tangent_kcs, const float* tangent_joints, const float* tangent_betas,
                           const float* tangent_Rs, int tangent_per_row, float* grad_params, void* stream) {
    int rc = check_critic(c, joints, K, betas, betas_stride, Rs, N);
    if (rc) return rc;
    if (!grad_params) return fail(HPE_ERR_INVALID, "null grad_params_dev");
    if (!grad_scores && !tangent_kcs && !tangent_joints && !tangent_betas && !tangent_Rs)
        return fail(HPE_ERR_INVALID, "hpe_critic_weight_grad: grad_scores and every tangent are NULL");
    DeviceGuard g(c->cfg.device);
    rc = ensure_critic_ws(c, N);
    if (rc) return rc;
    HIP_TRY(hpe_launch_critic_weight_grad(c->critic, joints, K, betas, betas_stride, Rs, N, grad_scores, tangent_kcs, tangent_joints,
                                          tangent_betas, tangent_Rs, tangent_per_row, c->critic_ws, grad_params,
                                          static_cast<hipStream_t>(stream)));
    return HPE_OK;
}

static int check_critic_params(hpe_ctx* c, const void* flat) {
    int rc = check_critic_ctx(c, true);
    if (rc) return rc;
    if (!flat) return fail(HPE_ERR_INVALID, "null flat_dev");
    return HPE_OK;
}

int hpe_critic_get_params(hpe_ctx* c, float* flat, void* stream) {
    int rc = check_critic_params(c, flat);
    if (rc) return rc;
    DeviceGuard g(c->cfg.device);
    HIP_TRY(hpe_launch_critic_params(c->critic, flat, false, static_cast<hipStream_t>(stream)));
    return HPE_OK;
}

int hpe_critic_set_params_dev(hpe_ctx* c, const float* flat, void* stream) {
    int rc = check_critic_params(c, flat);
    if (rc) return rc;
    DeviceGuard g(c->cfg.device);
    HIP_TRY(hpe_launch_critic_params(c->critic, const_cast<float*>(flat), true, static_cast<hipStream_t>(stream)));
    return HPE_OK;
}

int hpe_regressor_param_floats(void) { return regressor_param_offset(4, false); }

int hpe_regressor_param_offset(int idx, int is_bias) {
    if (idx < 0 || idx > 3 || (idx == 3 && is_bias)) return -1;
    return regressor_param_offset(idx, is_bias != 0);
}

static int check_regressor_params(hpe_ctx* c, const void* flat) {
    if (!c) return fail(HPE_ERR_INVALID, "null ctx");
    if (c->dead) return fail(HPE_ERR_STATE, "hpe_finalize failed on this ctx: destroy it and create a new one");
    if (!c->finalized) return fail(HPE_ERR_STATE, "hpe_finalize() has not been called");
    if (!c->have_regressor) return fail(HPE_ERR_STATE, "regressor weights / mean theta were not loaded");
    if (!flat) return fail(HPE_ERR_INVALID, "null flat_dev");
    return HPE_OK;
}

int hpe_regressor_get_params(hpe_ctx* c, float* flat, void* stream) {
    int rc = check_regressor_params(c, flat);
    if (rc) return rc;
    DeviceGuard g(c->cfg.device);
    HIP_TRY(regressor_params_copy(c, flat, false, static_cast<hipStream_t>(stream)));
    return HPE_OK;
}

int hpe_regressor_set_params_dev(hpe_ctx* c, const float* flat, void* stream) {
    int rc = check_regressor_params(c, flat);
    if (rc) return rc;
    DeviceGuard g(c->cfg.device);
    HIP_TRY(join_tail(c, static_cast<hipStream_t>(stream)));  // a pipelined call's tail may still read the weights this rewrites
    HIP_TRY(regressor_params_copy(c, const_cast<float*>(flat), true, static_cast<hipStream_t>(stream)));
    return HPE_OK;
}

int hpe_regressor_forward_train(hpe_ctx* c, const float* features, int B, const float* drop, float* thetas, void* stream) {
    int rc = check_ready(c, B, NEED_REG);
    if (rc) return rc;
    if (!features || !thetas) return fail(HPE_ERR_INVALID, "null pointer");
    DeviceGuard g(c->cfg.device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIP_TRY(regressor_train_forward(c, features, B, drop, st));
    // rows [S * B] of pitch THETA_LD, stage-major, behind the tiled mean
    HIP_TRY(hpe_launch_copy_theta(c->rt.th + (size_t)B * THETA_LD, THETA_LD, thetas, HPE_THETA_DIM, c->cfg.num_stage * B, HPE_THETA_DIM, st));
    return HPE_OK;
}

int hpe_regressor_backward(hpe_ctx* c, const float* features, int B, const float* drop, const float* grad_thetas, float* grad_flat,
                           float* grad_features, void* stream) {
    int rc = check_ready(c, B, NEED_REG);
    if (rc) return rc;
    if (!features || !grad_flat) return fail(HPE_ERR_INVALID, "null pointer");
    DeviceGuard g(c->cfg.device);
    HIP_TRY(regressor_train_backward(c, features, B, drop, grad_thetas, grad_flat, grad_features, static_cast<hipStream_t>(stream)));
    return HPE_OK;
}

int hpe_debug_conv(hpe_ctx* c, int idx, const float* x, int B, const float* residual, int relu, float* y, void* stream) {
    int rc = check_ready(c, B, NEED_ENC);
    if (rc) return rc;
    if (idx < 0 || idx >= HPE_NUM_CONV || !x || !y) return fail(HPE_ERR_INVALID, "bad argument");
    DeviceGuard g(c->cfg.device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (c->bf16) {
        if (idx == 0) return fail(HPE_ERR_STATE, "hpe_debug_conv: conv1 of a bf16 context runs inside the fused stem only");
        const ConvSpec& s = specs()[idx];
        const long nin = (long)B * s.hin * s.hin * s.cin, nout = (long)B * s.hout * s.hout * s.cout;
        HIP_TRY(hpe_launch_f32_to_bf16(x, c->X0, nin, st));
        if (residual) HIP_TRY(hpe_launch_f32_to_bf16(residual, c->SC, nout, st));
        HIP_TRY(run_conv_nhwc(c, idx, c->X0, B, residual ? c->SC : nullptr, relu, c->X1, st));
        HIP_TRY(hpe_launch_bf16_to_f32(c->X1, y, nout, st));
        return HPE_OK;
    }
    const float* in = x;
    if (idx == 0) {
        HIP_TRY(hpe_launch_pad_input(x, c->padded, B, HPE_IMG_SIZE, HPE_IMG_SIZE, STEM_HP, STEM_WP, st));
        in = c->padded;
    }
    HIP_TRY(run_conv_nhwc(c, idx, in, B, residual, relu, y, st));
    return HPE_OK;
}

int hpe_debug_chain(hpe_ctx* c, int idx2c, const float* t2, const float* residual, int B, float* t3, float* u1, int* occupancy, void* stream) {
    int rc = check_ready(c, B, NEED_ENC);
    if (rc) return rc;
    if (idx2c < 1 || idx2c + 2 >= HPE_NUM_CONV || !t2 || !residual || !t3 || !u1) return fail(HPE_ERR_INVALID, "bad argument");
    const ConvSpec& s2 = specs()[idx2c];
    if (!c->bf16) {
        // fp32 contexts: the identity blocks of stage 2 (conv_chain_f32.hip); operands used in place, u1 row-major
        const ConvSpec& sn1 = specs()[idx2c + 1];
        if (s2.kh != 1 || sn1.kh != 1 || sn1.stride != 1 || sn1.cin != s2.cout || !hpe_chain_f32_supported(s2.cin, s2.cout, sn1.cout))
            return fail(HPE_ERR_INVALID, "hpe_debug_chain (fp32): idx2c must be res2b_branch2c (an identity block of stage 2 followed by an identity block)");
        DeviceGuard g32(c->cfg.device);
        HIP_TRY(run_chain(c, idx2c, false, t2, residual, B, t3, u1, static_cast<hipStream_t>(stream), false));
        if (occupancy) {
            occupancy[0] = occupancy[1] = occupancy[2] = 0;
            HIP_TRY(hpe_chain_f32_occupancy(&occupancy[0]));
        }
        return HPE_OK;
    }
    // the conv_block form when idx2c is the branch2c of a block's first unit (its branch1 follows in the layer table)
    const bool first = specs()[idx2c + 1].kh == 1 && specs()[idx2c + 1].cout == s2.cout && strstr(specs()[idx2c + 1].name, "branch1") != nullptr;
    const ConvSpec& sn = specs()[idx2c + (first ? 2 : 1)];
    const int C2 = first ? specs()[idx2c + 1].cin : 0;
    if (s2.kh != 1 || s2.cout != 4 * s2.cin || sn.kh != 1 || sn.stride != 1 || sn.cin != s2.cout || !hpe_chain_bf16_supported(s2.cin, s2.cout, sn.cout, C2) ||
        (first && (!c->conv[idx2c].w_dual || specs()[idx2c + 1].stride != 1)))
        return fail(HPE_ERR_INVALID, "hpe_debug_chain: idx2c must be the branch2c of a stage-2 / stage-3 block that is followed by an identity block");
    DeviceGuard g(c->cfg.device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long M = (long)B * s2.hout * s2.hout;
    HIP_TRY(hpe_launch_f32_to_bf16(t2, c->T2, M * s2.cin, st));
    HIP_TRY(hpe_launch_f32_to_bf16(residual, c->X0, M * (first ? C2 : s2.cout), st));
    HIP_TRY(run_chain(c, idx2c, first, c->T2, c->X0, B, c->X1, c->T1, st));
    HIP_TRY(hpe_launch_bf16_to_f32(c->X1, t3, M * s2.cout, st));
    HIP_TRY(hpe_launch_bf16_to_f32(c->T1, u1, M * sn.cout, st));
    if (occupancy) HIP_TRY(hpe_chain_bf16_occupancy(occupancy));
    return HPE_OK;
}

int hpe_debug_stem(hpe_ctx* c, const float* images, int B, int rows_per_strip, float* y, void* stream) {
    int rc = check_ready(c, B, NEED_ENC);
    if (rc) return rc;
    if (!images || !y) return fail(HPE_ERR_INVALID, "null pointer");
    if (c->bf16) return fail(HPE_ERR_STATE, "hpe_debug_stem works on fp32 contexts only");
    DeviceGuard g(c->cfg.device);
    const int R = rows_per_strip > 0 ? rows_per_strip : hpe_stem_fused_pick_rows(B);
    HIP_TRY(hpe_launch_stem_fused(images, c->conv[0].stem_w, c->conv[0].scale, c->conv[0].shift, y, B, R, 0, static_cast<hipStream_t>(stream)));
    return HPE_OK;
}

// HpeDebugGemm -> the launcher's arguments (slab: elements per k-slab of the kernel asked for); scale, shift and the zero page stay with the caller
static GemmArgs debug_gemm_args(const HpeDebugGemm* g, int slab) {
    static_assert(HPE_GEMM_DENSE == GEMM_DENSE && HPE_GEMM_STRIDED == GEMM_STRIDED && HPE_GEMM_CONV3 == GEMM_CONV3 && HPE_GEMM_DUAL == GEMM_DUAL,
                  "include/hpe.h numbers the modes as GemmMode does");
    GemmArgs p{};
    p.x = g->x, p.x2 = g->x2, p.w = g->wt, p.res = g->residual, p.y = g->y;
    p.M = g->M, p.N = g->N, p.K = g->K;
    p.lda = g->lda, p.ldw = g->ldw, p.ldy = g->ldy, p.ldres = g->ldres, p.w_rows = g->w_rows;
    p.Hi = g->Hi, p.Wi = g->Wi, p.Cin = g->Cin, p.Ho = g->Ho, p.Wo = g->Wo, p.stride = g->stride;
    p.cin_slabs = g->Cin / slab;
    p.k1_slabs = g->k1_slabs;
    p.relu = g->relu;
    p.y_slab8 = g->y_slab8;
    return p;
}

// the guards both hooks share; empty: g can be read and its mode is one the hooks take
static std::string debug_gemm_refusal(const HpeDebugGemm* g) {
    if (!g) return "null HpeDebugGemm";
    if (g->struct_size != (int)sizeof(HpeDebugGemm))
        return "HpeDebugGemm.struct_size is " + std::to_string(g->struct_size) + ", this library's is " + std::to_string(sizeof(HpeDebugGemm)) +
               " (other revision of include/hpe.h?)";
    if (g->mode != HPE_GEMM_DENSE && g->mode != HPE_GEMM_STRIDED && g->mode != HPE_GEMM_CONV3 && g->mode != HPE_GEMM_DUAL)
        return "HpeDebugGemm.mode must be dense, strided, conv3 or dual";
    return "";
}

static std::string debug_gemm_rejected(const HpeDebugGemm* g, const char* clause) {
    return "mode " + std::to_string(g->mode) + " tile " + std::to_string(g->tile) + " M " + std::to_string(g->M) + " N " + std::to_string(g->N) + " K " +
           std::to_string(g->K) + " is outside the launcher's contract (gemm_contract.h), clause \"" + clause + "\": nothing was launched";
}

int hpe_debug_gemm_ex(hpe_ctx* c, const HpeDebugGemm* g, void* stream) {
    if (g && g->split_k) *g->split_k = 0;
    if (!c || !c->finalized) return fail(HPE_ERR_STATE, "needs a finalized ctx");
    const std::string why = debug_gemm_refusal(g);
    if (!why.empty()) return fail(HPE_ERR_INVALID, why);
    if ((!g->scale || !g->shift) && g->N > 1024) return fail(HPE_ERR_INVALID, "hpe_debug_gemm_ex: N <= 1024 without scale / shift");
    DeviceGuard guard(c->cfg.device);
    GemmArgs p = debug_gemm_args(g, 32);
    p.scale = g->scale ? g->scale : c->ones;
    p.shift = g->shift ? g->shift : c->zeros;
    p.zero = c->zeros;
    if (g->use_splitk) {
        p.partial = c->partial;
        p.partial_floats = c->partial_floats;
    }
    if (const char* clause = gemm_contract(p, g->mode, g->tile, GEMM_K_F32)) return fail(HPE_ERR_INVALID, "hpe_debug_gemm_ex: " + debug_gemm_rejected(g, clause));
    int split_k = 0;
    const hipError_t e = hpe_launch_gemm(p, g->mode, g->tile, c->plan.splitk_min_slabs, static_cast<hipStream_t>(stream), &split_k);
    if (g->split_k) *g->split_k = split_k;
    if (e == hipErrorInvalidValue && split_k == 0) return fail(HPE_ERR_INVALID, "hpe_debug_gemm_ex: the launcher refused the plan's splitk_min_slabs, nothing was launched");
    HIP_TRY(e);
    return HPE_OK;
}

int hpe_debug_gemm_check(const HpeDebugGemm* g, int kernel, int w_piece) {
    const std::string why = debug_gemm_refusal(g);
    if (!why.empty()) return fail(HPE_ERR_INVALID, why);
    if (kernel < GEMM_K_F32 || kernel > GEMM_K_BF16_P8) return fail(HPE_ERR_INVALID, "hpe_debug_gemm_check: kernel must be 0 (fp32), 1 (f32s), 2 (bf16) or 3 (bf16_p8)");
    const GemmKernel k = static_cast<GemmKernel>(kernel);
    GemmArgs p = debug_gemm_args(g, gemm_rules(k).slab);
    alignas(16) static const float present[4] = {};  // scale, shift and the zero page count as present (never read)
    p.scale = p.shift = p.zero = present;
    if (k == GEMM_K_F32S) p.w_piece = w_piece;
    if (const char* clause = gemm_contract(p, g->mode, g->tile, k)) return fail(HPE_ERR_INVALID, "hpe_debug_gemm_check: " + debug_gemm_rejected(g, clause));
    return HPE_OK;
}

// The launching twin of hpe_debug_gemm_check.  Kernel 0 is hpe_debug_gemm_ex.  Kernels 1..3: the contract is checked FIRST, with what the
// context owns (scale / shift when NULL, the zero page) counted as present, so a broken clause is named with no context at all; then
// the context is required, its buffers are filled in and the launcher (which runs the contract again on the real pointers) is called.
// The zero page: conv_gemm_bf16.hip (3x3 taps outside the image) and conv_gemm_bf16_p8.hip (those, and k-tiles past the end of K)
// fetch 16 bytes from p.zero -- every lane of a global_load_lds the same 16 -- and f32s never reads it; c->zeros is 1024 floats = 4096
// zero bytes from hipMalloc (256-byte aligned), which covers both.  The split-K workspace is c->partial (partial_floats floats; the
// 256x256 launcher shrinks its split until tiles * split_k * 256 * 256 floats fit).
int hpe_debug_gemm_launch(hpe_ctx* c, const HpeDebugGemm* g, int kernel, int w_piece, void* stream) {
    if (kernel == GEMM_K_F32) return hpe_debug_gemm_ex(c, g, stream);
    if (g && g->split_k) *g->split_k = 0;
    const std::string why = debug_gemm_refusal(g);
    if (!why.empty()) return fail(HPE_ERR_INVALID, why);
    if (kernel < GEMM_K_F32 || kernel > GEMM_K_BF16_P8) return fail(HPE_ERR_INVALID, "hpe_debug_gemm_launch: kernel must be 0 (fp32), 1 (f32s), 2 (bf16) or 3 (bf16_p8)");
    if ((!g->scale || !g->shift) && g->N > 1024) return fail(HPE_ERR_INVALID, "hpe_debug_gemm_launch: N <= 1024 without scale / shift");
    const GemmKernel k = static_cast<GemmKernel>(kernel);
    GemmArgs p = debug_gemm_args(g, gemm_rules(k).slab);
    if (k == GEMM_K_F32S) p.w_piece = w_piece;
    alignas(16) static const float present[4] = {};
    p.scale = g->scale ? g->scale : present;
    p.shift = g->shift ? g->shift : present;
    p.zero = present;
    if (const char* clause = gemm_contract(p, g->mode, g->tile, k)) return fail(HPE_ERR_INVALID, "hpe_debug_gemm_launch: " + debug_gemm_rejected(g, clause));
    if (!c || !c->finalized) return fail(HPE_ERR_STATE, "needs a finalized ctx");
    DeviceGuard guard(c->cfg.device);
    p.scale = g->scale ? g->scale : c->ones;
    p.shift = g->shift ? g->shift : c->zeros;
    p.zero = c->zeros;
    if (g->use_splitk) {
        p.partial = c->partial;
        p.partial_floats = c->partial_floats;
    }
    if (const char* clause = gemm_contract(p, g->mode, g->tile, k)) return fail(HPE_ERR_INVALID, "hpe_debug_gemm_launch: " + debug_gemm_rejected(g, clause));
    int split_k = 1;  // f32s and the bf16 tiles 0..6 never split
    hipStream_t st = static_cast<hipStream_t>(stream);
    const hipError_t e = k == GEMM_K_F32S ? hpe_launch_gemm_f32s(p, g->mode, g->tile, st)
                       : k == GEMM_K_BF16 ? hpe_launch_gemm_bf16(p, g->mode, g->tile, st)
                                          : hpe_launch_gemm_bf16_p8(p, g->mode, st, &split_k);
    if (g->split_k) *g->split_k = split_k;
    HIP_TRY(e);
    return HPE_OK;
}

int hpe_debug_conv_route(const HpeConfig* cfg, int idx, int B, int concurrent, int residual, int workspace, HpeConvRoute* out) {
    static_assert(HPE_CONV_K_F32 == CONV_K_F32 && HPE_CONV_K_HALO3 == CONV_K_HALO3 && HPE_CONV_K_WINO4_FUSED == CONV_K_WINO4_FUSED && HPE_CONV_K_COUNT == CONV_K_WINO4_FUSED + 1,
                  "include/hpe.h numbers the kernels as ConvKernel does");
    if (!cfg || !out) return fail(HPE_ERR_INVALID, "null argument");
    if (cfg->struct_size != (int)sizeof(HpeConfig) || out->struct_size != (int)sizeof(HpeConvRoute))
        return fail(HPE_ERR_INVALID, "hpe_debug_conv_route: HpeConfig.struct_size / HpeConvRoute.struct_size are " + std::to_string(cfg->struct_size) + " / " +
                                         std::to_string(out->struct_size) + ", this library's are " + std::to_string(sizeof(HpeConfig)) + " / " + std::to_string(sizeof(HpeConvRoute)));
    if (idx < 0 || idx >= HPE_NUM_CONV || B < 1) return fail(HPE_ERR_INVALID, "hpe_debug_conv_route: idx must be in [0, HPE_NUM_CONV) and B >= 1");
    const HpePlan pl = hpe_resolve_plan(*cfg);
    const bool bf16 = cfg->encoder_dtype == 1;
    const ConvQuery q{B, concurrent != 0, residual != 0, workspace != 0};
    const ConvRoute r = route_conv(pl, bf16, idx, q);
    *out = HpeConvRoute{(int)sizeof(HpeConvRoute), r.kernel, r.mode, r.tile, r.in_slab8, 0, 0, -1, -1, 0, layer_packs(pl, bf16, idx), 0};
    for (const ResBlock& blk : blocks()) {
        if (idx != blk.i2a && idx != blk.i2c) continue;
        const BlockRoute b = route_block(pl, bf16, blk, q);
        if (idx == blk.i2a) out->out_slab8 = b.r2a.out_slab8;
        if (idx == blk.i2c) out->join = b.join, out->next_slab8 = b.u1_slab8;
        if (idx == blk.i2c && b.join == JOIN_DUAL) out->join_kernel = b.r2c.kernel, out->join_tile = b.r2c.tile;
    }
    return HPE_OK;
}

int hpe_debug_conv_stream1x1(const HpeConfig* cfg, int idx, int B, int concurrent, int residual) {
    if (!cfg || cfg->struct_size != (int)sizeof(HpeConfig) || idx < 0 || idx >= HPE_NUM_CONV || B < 1) {
        fail(HPE_ERR_INVALID, "hpe_debug_conv_stream1x1: cfg (struct_size), idx in [0, HPE_NUM_CONV) and B >= 1");
        return -1;
    }
    const HpePlan pl = hpe_resolve_plan(*cfg);
    const bool bf16 = cfg->encoder_dtype == 1;
    const ConvQuery q{B, concurrent != 0, residual != 0, true};
    for (const ResBlock& blk : blocks())  // the branch2c of a conv_block: the block's dual-source launch
        if (blk.first && blk.i2c == idx) {
            const BlockRoute b = route_block(pl, bf16, blk, q);
            return (stream1x1_dual(pl, bf16, blk) ? 2 : 0) | (b.join == JOIN_DUAL && b.r2c.stream ? 1 : 0);
        }
    return (stream1x1_layer(pl, bf16, idx) ? 2 : 0) | (route_conv(pl, bf16, idx, q).stream ? 1 : 0);
}

int hpe_debug_dual(hpe_ctx* c, int idx2c, const float* t2, const float* x, int B, float* y, void* stream) {
    int rc = check_ready(c, B, NEED_ENC);
    if (rc) return rc;
    if (!t2 || !x || !y || c->bf16) return fail(HPE_ERR_INVALID, "hpe_debug_dual: null pointer, or a bf16 context");
    for (const ResBlock& blk : blocks()) {
        if (!blk.first || blk.i2c != idx2c) continue;
        const BlockRoute b = route_block(c->plan, false, blk, ConvQuery{B, false, false, c->wino_v != nullptr});
        if (b.join != JOIN_DUAL) break;
        DeviceGuard g(c->cfg.device);
        HIP_TRY(run_dual(c, blk.i2c, blk.i1, b.r2c, t2, x, B, y, static_cast<hipStream_t>(stream)));
        return HPE_OK;
    }
    return fail(HPE_ERR_INVALID, "hpe_debug_dual: idx2c must be the branch2c of a conv_block that this plan runs as the dual-source launch");
}

int hpe_debug_stream_chain(hpe_ctx* c, int idx2c, const float* t2, const float* x, int B, float* t3, float* u1, int slab8, int rows, void* stream) {
    int rc = check_ready(c, B, NEED_ENC);
    if (rc) return rc;
    if (!t2 || !x || !t3 || !u1 || c->bf16 || rows < 0) return fail(HPE_ERR_INVALID, "hpe_debug_stream_chain: null pointer, negative rows, or a bf16 context");
    for (const ResBlock& blk : blocks()) {
        if (blk.i2c != idx2c || blk.last) continue;
        const ConvSpec& s2 = specs()[blk.i2c];
        const ConvSpec& sn = specs()[blk.i2c + (blk.first ? 2 : 1)];
        // (the geometry is the launcher's to refuse: only what would read past the caller's buffers is stopped here)
        if (rows > B * s2.hout * s2.hout || sn.cin != s2.cout || (blk.first && specs()[blk.i1].stride != 1)) break;
        DeviceGuard g(c->cfg.device);
        if (run_stream_chain(c, blk.i2c, blk.first, t2, x, B, t3, u1, static_cast<hipStream_t>(stream), slab8 != 0, rows) != hipSuccess) break;
        return HPE_OK;
    }
    return fail(HPE_ERR_INVALID, "hpe_debug_stream_chain: refused (idx2c must be res2a_branch2c or res2b_branch2c, rows a multiple of 32 inside the batch); nothing was launched");
}

int hpe_debug_gemm(hpe_ctx* c, const float* x, const float* wt, int M, int N, int K, int w_rows, int tile, const float* residual,
                   int relu, float* y, void* stream) {
    if (!c || !c->finalized || !c->have_regressor) return fail(HPE_ERR_STATE, "needs a finalized ctx with the regressor loaded");
    if (!x || !wt || !y || N > 1024) return fail(HPE_ERR_INVALID, "bad argument (N <= 1024)");
    HpeDebugGemm g{};
    g.struct_size = (int)sizeof(HpeDebugGemm);
    g.mode = HPE_GEMM_DENSE;
    g.tile = tile;
    g.x = x;
    g.wt = wt;
    g.residual = residual;
    g.y = y;
    g.M = M;
    g.N = N;
    g.K = K;
    g.lda = K;
    g.ldw = K;
    g.w_rows = w_rows;
    g.ldy = N;
    g.ldres = N;
    g.relu = relu;
    g.use_splitk = 0;
    return hpe_debug_gemm_ex(c, &g, stream);
}

int hpe_debug_maxpool(const float* x, int B, int H, int C, float* y, void* stream) {
    if (!x || !y || B < 1) return fail(HPE_ERR_INVALID, "bad argument");
    HIP_TRY(hpe_launch_maxpool(x, y, B, H, C, static_cast<hipStream_t>(stream)));
    return HPE_OK;
}

int hpe_debug_avgpool(const float* x, int B, int HW, int C, float* y, void* stream) {
    if (!x || !y || B < 1) return fail(HPE_ERR_INVALID, "bad argument");
    HIP_TRY(hpe_launch_avgpool(x, y, B, HW, C, C, static_cast<hipStream_t>(stream)));
    return HPE_OK;
}

int hpe_debug_joint_regress(hpe_ctx* c, const float* X, int n, int use_kp, float* out, void* stream) {
    if (!c || !c->finalized || !c->have_smpl) return fail(HPE_ERR_STATE, "SMPL not finalized");
    if (!X || !out || n < 1) return fail(HPE_ERR_INVALID, "bad argument");
    DeviceGuard g(c->cfg.device);
    HIP_TRY(hpe_launch_joint_regress(X, use_kp ? c->smpl.kp_reg : c->smpl.j_reg, n, use_kp ? c->num_kp : 24, out, nullptr, nullptr,
                                     static_cast<hipStream_t>(stream)));
    return HPE_OK;
}

int hpe_device_status(hpe_ctx* c, void* stream) {
    if (!c || !c->finalized) return fail(HPE_ERR_STATE, "needs a finalized ctx");
    DeviceGuard g(c->cfg.device);
    HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    if (c->dev_err) {
        unsigned w = 0;
        HIP_TRY(hipMemcpy(&w, c->dev_err, sizeof w, hipMemcpyDeviceToHost));
        if (w) {
            (void)hipMemset(c->dev_err, 0, sizeof w);
            return fail(HPE_ERR_HIP, "device error word " + std::to_string(w) +
                                         ": a stream-K wait of the Winograd GEMM timed out, outputs since the last check are invalid");
        }
    }
    return HPE_OK;
}

int hpe_enable_timing(hpe_ctx* c, int enable) {
    if (!c) return fail(HPE_ERR_INVALID, "null ctx");
    c->timing = enable;
    c->span_n = 0;
    c->timed_valid = false;
    c->conv_timed_valid = false;
    return HPE_OK;
}

int hpe_get_timings(hpe_ctx* c, float ms[5]) {
    if (!c || !ms) return fail(HPE_ERR_INVALID, "null argument");
    if (!c->timed_valid) return fail(HPE_ERR_STATE, "no timed call recorded (hpe_enable_timing first)");
    DeviceGuard g(c->cfg.device);
    HIP_TRY(hipEventSynchronize(c->ev[4]));
    for (int i = 0; i < 5; ++i) ms[i] = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms[0], c->ev[0], c->ev[1]));
    HIP_TRY(hipEventElapsedTime(&ms[4], c->ev[0], c->ev[4]));
    if (c->conv_timed_valid) {
        for (int i = 0; i < HPE_NUM_CONV; ++i) {
            float t = 0.f;
            HIP_TRY(hipEventElapsedTime(&t, c->cev0[i], c->cev1[i]));
            ms[1] += t;
        }
    }
    ms[2] = ms[4] - ms[0];  // regressor + SMPL stages
    return HPE_OK;
}

int hpe_get_span_stats(hpe_ctx* c, float ms[3], int* n_calls) {
    if (!c || !ms || !n_calls) return fail(HPE_ERR_INVALID, "null argument");
    if (c->span_n == 0) return fail(HPE_ERR_STATE, "no timed call recorded (hpe_enable_timing first)");
    DeviceGuard g(c->cfg.device);
    const unsigned n = c->span_n < (unsigned)hpe_ctx::SPAN_RING ? c->span_n : (unsigned)hpe_ctx::SPAN_RING;
    double sum = 0.0;
    float lo = 1e30f, hi = 0.f;
    for (unsigned i = 0; i < n; ++i) {
        float t = 0.f;
        HIP_TRY(hipEventSynchronize(c->span1[i]));
        HIP_TRY(hipEventElapsedTime(&t, c->span0[i], c->span1[i]));
        sum += t;
        lo = t < lo ? t : lo;
        hi = t > hi ? t : hi;
    }
    ms[0] = (float)(sum / n);
    ms[1] = lo;
    ms[2] = hi;
    *n_calls = (int)n;
    return HPE_OK;
}

int hpe_get_loss_timings(hpe_ctx* c, float ms[2]) {
    if (!c || !ms) return fail(HPE_ERR_INVALID, "null argument");
    if (c->loss_timed_stages == 0) return fail(HPE_ERR_STATE, "no timed hpe_val_losses call recorded (hpe_enable_timing first)");
    DeviceGuard g(c->cfg.device);
    HIP_TRY(hipEventSynchronize(c->lev_all[1]));
    HIP_TRY(hipEventElapsedTime(&ms[0], c->lev_all[0], c->lev_all[1]));
    ms[1] = 0.f;
    for (int s = 0; s < c->loss_timed_stages; ++s) {
        float t = 0.f;
        HIP_TRY(hipEventElapsedTime(&t, c->lev0[s], c->lev1[s]));
        ms[1] += t;
    }
    return HPE_OK;
}

int hpe_debug_set_loss_counter(hpe_ctx* c, void* counter_dev) {
    if (!c) return fail(HPE_ERR_INVALID, "null ctx");
    c->loss_counter = static_cast<unsigned long long*>(counter_dev);
    return HPE_OK;
}

int hpe_get_conv_timings(hpe_ctx* c, float* ms) {
    if (!c || !ms) return fail(HPE_ERR_INVALID, "null argument");
    if (!c->conv_timed_valid) return fail(HPE_ERR_STATE, "no level-2 timed call recorded");
    DeviceGuard g(c->cfg.device);
    HIP_TRY(hipEventSynchronize(c->ev[4]));
    for (int i = 0; i < HPE_NUM_CONV; ++i) HIP_TRY(hipEventElapsedTime(&ms[i], c->cev0[i], c->cev1[i]));
    return HPE_OK;
}

}  // extern "C"
#pragma GCC visibility pop
