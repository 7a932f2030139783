// hpe_render_api.hip -- the mesh renderer of the C ABI (render.hip; DESIGN.md "Renderer"): hpe_renderer and the render entry points.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "hpe_ctx.h"

#pragma GCC visibility push(default)
extern "C" {

struct hpe_renderer {
    int device = 0, P = 0, Fn = 0, max_batch = 0;
    int* faces = nullptr;     // [Fn,3]
    int* adj_off = nullptr;   // [P+1]
    int* adj_face = nullptr;  // [3 Fn]
    RenderVert* rec = nullptr;
    uint2* box = nullptr;
    float* center = nullptr;
};

void hpe_render_params_init(HpeRenderParams* p) {
    if (!p) return;
    p->struct_size = (int)sizeof(HpeRenderParams);
    p->color_id = 0;
    p->do_alpha = 0;
    p->rot_axis = 0;
    p->rot_deg = 0.f;
    p->near = -1.f;
    p->far = -1.f;
}

int hpe_renderer_destroy(hpe_renderer* r) {
    if (!r) return HPE_OK;
    {
        DeviceGuard g(r->device);
        (void)hipDeviceSynchronize();
        for (void* q : {(void*)r->faces, (void*)r->adj_off, (void*)r->adj_face, (void*)r->rec, (void*)r->box, (void*)r->center})
            if (q) (void)hipFree(q);
    }
    delete r;
    return HPE_OK;
}

int hpe_renderer_create(int device, const int* faces, int Fn, int P, int max_batch, hpe_renderer** out) {
    if (!out) return fail(HPE_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!faces || Fn < 1 || Fn > (1 << 28) || P < 3 || P > (1 << 26))
        return fail(HPE_ERR_INVALID, "faces must be [Fn,3] with 1 <= Fn <= 2^28 over 3 <= P <= 2^26 vertices");
    if (max_batch < 1 || max_batch > 1024) return fail(HPE_ERR_INVALID, "max_batch must be in [1, 1024]");
    for (long i = 0; i < 3L * Fn; ++i)
        if (faces[i] < 0 || faces[i] >= P)
            return fail(HPE_ERR_INVALID, "face " + std::to_string(i / 3) + " has vertex index " + std::to_string(faces[i]) +
                                             " outside [0, " + std::to_string(P) + ")");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(HPE_ERR_NO_DEVICE, "no HIP device visible");
    if (device < 0 || device >= ndev) return fail(HPE_ERR_INVALID, "device " + std::to_string(device) + " out of range");
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(HPE_ERR_NO_DEVICE, std::string("device is ") + prop.gcnArchName + ", kernels are built for gfx950 only");
    // vertex -> face CSR, faces in index order per vertex (the normal sum runs in this fixed order)
    std::vector<int> off((size_t)P + 1, 0), adj((size_t)3 * Fn);
    for (long i = 0; i < 3L * Fn; ++i) ++off[(size_t)faces[i] + 1];
    for (int v = 0; v < P; ++v) off[(size_t)v + 1] += off[v];
    std::vector<int> cur(off.begin(), off.end() - 1);
    for (int f = 0; f < Fn; ++f)
        for (int k = 0; k < 3; ++k) adj[(size_t)cur[faces[3L * f + k]]++] = f;
    hpe_renderer* r = new hpe_renderer();
    r->device = device;
    r->P = P;
    r->Fn = Fn;
    r->max_batch = max_batch;
    int rc = HPE_OK;
    {
        DeviceGuard g(device);
        auto alloc = [&](void** q, size_t bytes) -> bool {
            hipError_t e = hipMalloc(q, bytes);
            if (e != hipSuccess) rc = fail(HPE_ERR_HIP, std::string("hipMalloc: ") + hipGetErrorString(e));
            return e == hipSuccess;
        };
        if (alloc((void**)&r->faces, sizeof(int) * 3 * (size_t)Fn) && alloc((void**)&r->adj_off, sizeof(int) * off.size()) &&
            alloc((void**)&r->adj_face, sizeof(int) * adj.size()) && alloc((void**)&r->rec, sizeof(RenderVert) * (size_t)max_batch * P) &&
            alloc((void**)&r->box, sizeof(uint2) * (size_t)max_batch * Fn) && alloc((void**)&r->center, sizeof(float) * 4 * (size_t)max_batch)) {
            hipError_t e = hipMemcpy(r->faces, faces, sizeof(int) * 3 * (size_t)Fn, hipMemcpyHostToDevice);
            if (e == hipSuccess) e = hipMemcpy(r->adj_off, off.data(), sizeof(int) * off.size(), hipMemcpyHostToDevice);
            if (e == hipSuccess) e = hipMemcpy(r->adj_face, adj.data(), sizeof(int) * adj.size(), hipMemcpyHostToDevice);
            if (e != hipSuccess) rc = fail(HPE_ERR_HIP, std::string("hipMemcpy: ") + hipGetErrorString(e));
        }
    }
    if (rc != HPE_OK) {
        hpe_renderer_destroy(r);
        return rc;
    }
    *out = r;
    return HPE_OK;
}

// argument checks and the per-call constants shared by hpe_render and its test hooks
static int render_args(hpe_renderer* r, const float* verts, const float* cam, int B, int H, int W, const HpeRenderParams* p,
                       RenderArgs* a) {
    if (!r) return fail(HPE_ERR_INVALID, "renderer is NULL");
    HpeRenderParams d;
    hpe_render_params_init(&d);
    if (p && p->struct_size != (int)sizeof(HpeRenderParams))
        return fail(HPE_ERR_INVALID, "HpeRenderParams.struct_size is " + std::to_string(p->struct_size) + ", this library expects " +
                                         std::to_string(sizeof(HpeRenderParams)) + " (fill the struct with hpe_render_params_init)");
    if (!p) p = &d;
    if (!verts) return fail(HPE_ERR_INVALID, "verts is NULL");
    if (B < 1 || B > r->max_batch)
        return fail(HPE_ERR_INVALID, "B = " + std::to_string(B) + " outside [1, max_batch = " + std::to_string(r->max_batch) + "]");
    if (H < 1 || H > 4096 || W < 1 || W > 4096)
        return fail(HPE_ERR_INVALID, "image size " + std::to_string(H) + " x " + std::to_string(W) + " outside [1, 4096]");
    if (p->rot_axis < 0 || p->rot_axis > 3) return fail(HPE_ERR_INVALID, "rot_axis must be 0 (none), 1 (x), 2 (y) or 3 (z)");
    if (p->rot_axis && !std::isfinite(p->rot_deg)) return fail(HPE_ERR_INVALID, "rot_deg is not finite");
    *a = RenderArgs{};
    a->verts = verts;
    a->cam = cam;
    a->faces = r->faces;
    a->adj_off = r->adj_off;
    a->adj_face = r->adj_face;
    a->rec = r->rec;
    a->box = r->box;
    a->center = r->center;
    a->B = B;
    a->P = r->P;
    a->Fn = r->Fn;
    a->H = H;
    a->W = W;
    a->C = p->do_alpha ? 4 : 3;
    // the reference's defaults never reject a vertex that near = 0.1 / far = +inf would keep (renderer.py:65-68)
    a->znear = p->near >= 0.f ? p->near : 0.1f;
    a->zfar = p->far >= 0.f ? p->far : INFINITY;
    a->rotate = p->rot_axis != 0;
    if (a->rotate) {  // cv2.Rodrigues of radians(deg) about one axis (renderer.py:95-100)
        const double t = p->rot_deg * M_PI / 180.0, c = cos(t), s = sin(t);
        const double Rx[9] = {1, 0, 0, 0, c, -s, 0, s, c}, Ry[9] = {c, 0, s, 0, 1, 0, -s, 0, c}, Rz[9] = {c, -s, 0, s, c, 0, 0, 0, 1};
        const double* R = p->rot_axis == 1 ? Rx : p->rot_axis == 2 ? Ry : Rz;
        for (int k = 0; k < 9; ++k) a->R[k] = (float)R[k];
    }
    // simple_renderer (renderer.py:157-196): albedo by color_id parity (Python's % on negatives: -1 is odd), three point lights at
    // _rotateY(pos, radians(120)) = pos . [[cos, 0, sin], [0, 1, 0], [-sin, 0, cos]]
    static const float kBlue[3] = {0.65098039f, 0.74117647f, 0.85882353f}, kPink[3] = {0.9f, 0.7f, 0.7f};
    const float* alb = (p->color_id & 1) ? kPink : kBlue;
    static const double kLight[3][3] = {{-200, -100, -100}, {800, 10, 300}, {-500, 500, 1000}};
    static const float kLightColor[3] = {1.f, 1.f, 0.7f};
    const double ang = 120.0 * M_PI / 180.0, ca = cos(ang), sa = sin(ang);
    for (int k = 0; k < 3; ++k) {
        a->albedo[k] = alb[k];
        a->light_color[k] = kLightColor[k];
        const double x = kLight[k][0], y = kLight[k][1], z = kLight[k][2];
        a->light[3 * k] = (float)(x * ca - z * sa);
        a->light[3 * k + 1] = (float)y;
        a->light[3 * k + 2] = (float)(x * sa + z * ca);
    }
    return HPE_OK;
}

int hpe_render(hpe_renderer* r, const float* verts, const float* cam, int B, int H, int W, const unsigned char* bg,
               const HpeRenderParams* p, unsigned char* out, void* stream) {
    RenderArgs a;
    int rc = render_args(r, verts, cam, B, H, W, p, &a);
    if (rc) return rc;
    if (!out) return fail(HPE_ERR_INVALID, "out is NULL");
    a.bg = bg;
    a.out = out;
    DeviceGuard g(r->device);
    HIP_TRY(hpe_launch_render(a, 1, static_cast<hipStream_t>(stream)));
    return HPE_OK;
}

int hpe_debug_render_ids(hpe_renderer* r, const float* verts, const float* cam, int B, int H, int W, const HpeRenderParams* p,
                         int* face, float* z, void* stream) {
    RenderArgs a;
    int rc = render_args(r, verts, cam, B, H, W, p, &a);
    if (rc) return rc;
    if (!face || !z) return fail(HPE_ERR_INVALID, "face / z is NULL");
    a.out_face = face;
    a.out_z = z;
    DeviceGuard g(r->device);
    HIP_TRY(hpe_launch_render(a, 1, static_cast<hipStream_t>(stream)));
    return HPE_OK;
}

int hpe_debug_render_vertices(hpe_renderer* r, const float* verts, const float* cam, int B, int H, int W, const HpeRenderParams* p,
                              void* rec, void* stream) {
    RenderArgs a;
    int rc = render_args(r, verts, cam, B, H, W, p, &a);
    if (rc) return rc;
    if (!rec) return fail(HPE_ERR_INVALID, "rec is NULL");
    a.rec = static_cast<RenderVert*>(rec);
    DeviceGuard g(r->device);
    HIP_TRY(hpe_launch_render(a, 0, static_cast<hipStream_t>(stream)));
    return HPE_OK;
}

}  // extern "C"
#pragma GCC visibility pop
