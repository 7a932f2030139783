// render.hip -- batched mesh rasteriser with Lambertian shading: the reference's SMPLRenderer (src/util/renderer.py:23-112,
// simple_renderer :157-196) without OpenDR.  The output is defined in DESIGN.md "Renderer"; in short:
//   vertex kernel  one thread per (image, vertex): optional view rotation about the mesh centre, pinhole projection snapped to
//                  fixed point with 8 fractional bits, area-weighted vertex normal over a vertex -> face CSR (fixed order, no atomics),
//                  three point lights -> one RenderVert record.
//   face kernel    one thread per (image, face): rejection (non-finite / outside [near, far] / outside the guard band / zero area)
//                  and a packed pixel bounding box (empty for a dropped face).
//   raster kernel  one workgroup per (image, 64 x 64 tile): a tile of 64-bit keys (float bits of the depth << 32 | face) in LDS,
//                  min-reduced with LDS atomics; small faces one thread each, large ones by the whole workgroup; then every pixel is
//                  resolved in place (barycentrics of the winning face, perspective-correct colour, composite) and written as uint8.
// Coverage is integer arithmetic (int64 edge functions, top-left tie rule), so it does not depend on the order of the faces.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "hpe_internal.h"

namespace {

constexpr int kTile = 64;          // raster tile side (pixels)
constexpr int kThreads = 256;      // raster workgroup
constexpr int kChunk = 1024;       // faces scanned per pass of the raster loop (4 per thread)
constexpr int kLargeArea = 64;     // faces covering more tile pixels than this are rasterised by the whole workgroup
constexpr unsigned long long kEmptyKey = ~0ull;

// edge function of the directed edge a -> b at p, all in 1/256 px; |coordinates| <= 2^22 + 2^20, so products stay below 2^47
__device__ __forceinline__ long long edge_fn(int ax, int ay, int bx, int by, long long px, long long py) {
    return (long long)(bx - ax) * (py - ay) - (long long)(by - ay) * (px - ax);
}

// tie rule for a sample exactly on an edge of a positively oriented triangle: the edge owns it when it points down (+y), or along -x
// when horizontal.  A shared edge is traversed in opposite directions by its two triangles, so exactly one of them owns the sample
// (the rule is a fixed infinitesimal shift of the sample, which also settles samples on shared vertices).
__device__ __forceinline__ bool edge_owns(int ax, int ay, int bx, int by) { return (by > ay) || (by == ay && bx < ax); }

struct FaceSetup {
    int x[3], y[3];
    float iz[3];
    int vi[3];  // vertex indices in the (positively oriented) order used for x / y / iz
    long long A;
    bool own[3];
};

__device__ __forceinline__ void face_setup(const RenderArgs& a, int b, int f, FaceSetup& s) {
    const int* fv = a.faces + (size_t)f * 3;
    int i0 = fv[0], i1 = fv[1], i2 = fv[2];
    const RenderVert* rec = a.rec + (size_t)b * a.P;
    long long A = edge_fn(rec[i0].U, rec[i0].V, rec[i1].U, rec[i1].V, rec[i2].U, rec[i2].V);
    if (A < 0) {  // both windings are drawn: swap to a positive orientation
        const int t = i1;
        i1 = i2;
        i2 = t;
        A = -A;
    }
    s.vi[0] = i0;
    s.vi[1] = i1;
    s.vi[2] = i2;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const RenderVert r = rec[s.vi[k]];
        s.x[k] = r.U;
        s.y[k] = r.V;
        s.iz[k] = r.iz;
    }
    s.A = A;
    // edge k is opposite vertex k: v1 -> v2, v2 -> v0, v0 -> v1
    s.own[0] = edge_owns(s.x[1], s.y[1], s.x[2], s.y[2]);
    s.own[1] = edge_owns(s.x[2], s.y[2], s.x[0], s.y[0]);
    s.own[2] = edge_owns(s.x[0], s.y[0], s.x[1], s.y[1]);
}

__device__ __forceinline__ void edges_at(const FaceSetup& s, long long px, long long py, long long E[3]) {
    E[0] = edge_fn(s.x[1], s.y[1], s.x[2], s.y[2], px, py);
    E[1] = edge_fn(s.x[2], s.y[2], s.x[0], s.y[0], px, py);
    E[2] = edge_fn(s.x[0], s.y[0], s.x[1], s.y[1], px, py);
}

__device__ __forceinline__ bool inside(const FaceSetup& s, const long long E[3]) {
    return (E[0] > 0 || (E[0] == 0 && s.own[0])) && (E[1] > 0 || (E[1] == 0 && s.own[1])) && (E[2] > 0 || (E[2] == 0 && s.own[2]));
}

// z_pix = 1 / sum_k lambda_k / z_k with lambda_k = E_k / A; explicit fmas so that every call site rounds alike
__device__ __forceinline__ float pix_depth(const FaceSetup& s, const long long E[3], float l[3]) {
    const float rA = 1.0f / (float)s.A;
#pragma unroll
    for (int k = 0; k < 3; ++k) l[k] = (float)E[k] * rA;
    const float w = __fmaf_rn(l[2], s.iz[2], __fmaf_rn(l[1], s.iz[1], l[0] * s.iz[0]));
    return 1.0f / w;
}

__device__ __forceinline__ void depth_test(unsigned long long* key, int i, float z, int f) {
    const unsigned long long k = ((unsigned long long)__float_as_uint(z) << 32) | (unsigned)f;
    if (k < key[i]) atomicMin(&key[i], k);  // ds_min_u64
}

// mesh centre per image (only when rotating): one workgroup per image, fixed-order double sums, so bitwise repeatable
__global__ __launch_bounds__(256) void render_center_kernel(RenderArgs a) {
    __shared__ double red[3][256];
    const int b = blockIdx.x, t = threadIdx.x;
    const float* v = a.verts + (size_t)b * a.P * 3;
    double s0 = 0, s1 = 0, s2 = 0;
    for (int p = t; p < a.P; p += 256) {
        s0 += v[(size_t)p * 3];
        s1 += v[(size_t)p * 3 + 1];
        s2 += v[(size_t)p * 3 + 2];
    }
    red[0][t] = s0;
    red[1][t] = s1;
    red[2][t] = s2;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (t < h)
            for (int k = 0; k < 3; ++k) red[k][t] += red[k][t + h];
        __syncthreads();
    }
    if (t < 3) a.center[b * 4 + t] = (float)(red[t][0] / a.P);
}

// one thread per (vertex, image): grid (ceil(P / 256), B)
__global__ __launch_bounds__(256) void render_vertex_kernel(RenderArgs a) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    const int b = blockIdx.y;
    if (p >= a.P) return;
    const float* vb = a.verts + (size_t)b * a.P * 3;
    float x = vb[(size_t)p * 3], y = vb[(size_t)p * 3 + 1], z = vb[(size_t)p * 3 + 2];
    // area-weighted normal on the input vertices: differences of nearby float32 coordinates are exact there, and the normal of the
    // rotated mesh is this one times R (rotations commute with the cross product)
    float nx = 0.f, ny = 0.f, nz = 0.f;
    for (int k = a.adj_off[p], e = a.adj_off[p + 1]; k < e; ++k) {
        const int* fv = a.faces + (size_t)a.adj_face[k] * 3;
        const float* v0 = vb + (size_t)fv[0] * 3;
        const float* v1 = vb + (size_t)fv[1] * 3;
        const float* v2 = vb + (size_t)fv[2] * 3;
        const float e1x = v1[0] - v0[0], e1y = v1[1] - v0[1], e1z = v1[2] - v0[2];
        const float e2x = v2[0] - v0[0], e2y = v2[1] - v0[1], e2z = v2[2] - v0[2];
        nx += e1y * e2z - e1z * e2y;
        ny += e1z * e2x - e1x * e2z;
        nz += e1x * e2y - e1y * e2x;
    }
    if (a.rotate) {  // row vectors times R: V' = (V - c) R + c
        const float cx = a.center[b * 4], cy = a.center[b * 4 + 1], cz = a.center[b * 4 + 2];
        const float dx = x - cx, dy = y - cy, dz = z - cz;
        x = dx * a.R[0] + dy * a.R[3] + dz * a.R[6] + cx;
        y = dx * a.R[1] + dy * a.R[4] + dz * a.R[7] + cy;
        z = dx * a.R[2] + dy * a.R[5] + dz * a.R[8] + cz;
        const float mx = nx * a.R[0] + ny * a.R[3] + nz * a.R[6];
        const float my = nx * a.R[1] + ny * a.R[4] + nz * a.R[7];
        const float mz = nx * a.R[2] + ny * a.R[5] + nz * a.R[8];
        nx = mx;
        ny = my;
        nz = mz;
    }
    const float nl = sqrtf(nx * nx + ny * ny + nz * nz);
    if (nl > 0.f) {
        nx /= nl;
        ny /= nl;
        nz /= nl;
    }  // else: a vertex of no face (or of degenerate faces only) is unlit
    float shade = 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float lx = a.light[3 * k] - x, ly = a.light[3 * k + 1] - y, lz = a.light[3 * k + 2] - z;
        const float ll = sqrtf(lx * lx + ly * ly + lz * lz);
        const float d = (nx * lx + ny * ly + nz * lz) / ll;
        shade += a.light_color[k] * fmaxf(d, 0.f);
    }
    float f = 500.f, ppx = 0.5f * a.W, ppy = 0.5f * a.H;
    if (a.cam) {
        f = a.cam[b * 3];
        ppx = a.cam[b * 3 + 1];
        ppy = a.cam[b * 3 + 2];
    }
    RenderVert r;
    const float u = f * x / z + ppx, v = f * y / z + ppy;
    const bool ok = isfinite(x) && isfinite(y) && isfinite(z) && z >= a.znear && z <= a.zfar && fabsf(u) <= 16384.f && fabsf(v) <= 16384.f;
    r.U = ok ? (int)rintf(256.f * u) : 0;
    r.V = ok ? (int)rintf(256.f * v) : 0;
    r.valid = ok ? 1 : 0;
    r.pad = 0;
    r.iz = ok ? 1.0f / z : 0.f;
    r.r = a.albedo[0] * shade;
    r.g = a.albedo[1] * shade;
    r.b = a.albedo[2] * shade;
    a.rec[(size_t)b * a.P + p] = r;
}

// one thread per (face, image): grid (ceil(Fn / 256), B).  box = {x0 | y0 << 16, x1 | y1 << 16}, inclusive pixel bounds of the
// samples (256 j + 128, 256 i + 128) inside the face's snapped bounding box, clipped to the image; {0xffffffff, 0} when dropped
__global__ __launch_bounds__(256) void render_face_kernel(RenderArgs a) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    const int b = blockIdx.y;
    if (f >= a.Fn) return;
    const int* fv = a.faces + (size_t)f * 3;
    const RenderVert* rec = a.rec + (size_t)b * a.P;
    const RenderVert r0 = rec[fv[0]], r1 = rec[fv[1]], r2 = rec[fv[2]];
    uint2 box = make_uint2(0xffffffffu, 0u);
    if (r0.valid && r1.valid && r2.valid && edge_fn(r0.U, r0.V, r1.U, r1.V, r2.U, r2.V) != 0) {
        const int minU = min(r0.U, min(r1.U, r2.U)), maxU = max(r0.U, max(r1.U, r2.U));
        const int minV = min(r0.V, min(r1.V, r2.V)), maxV = max(r0.V, max(r1.V, r2.V));
        // first / last pixel whose sample lies in [min, max]: ceil((min - 128) / 256), floor((max - 128) / 256)
        const int x0 = max(-((128 - minU) >> 8), 0), x1 = min((maxU - 128) >> 8, a.W - 1);
        const int y0 = max(-((128 - minV) >> 8), 0), y1 = min((maxV - 128) >> 8, a.H - 1);
        if (x0 <= x1 && y0 <= y1) box = make_uint2((unsigned)x0 | ((unsigned)y0 << 16), (unsigned)x1 | ((unsigned)y1 << 16));
    }
    a.box[(size_t)b * a.Fn + f] = box;
}

// one thread rasterises face f over the pixels [cx0, cx1] x [cy0, cy1] of the tile at (X0, Y0); edge functions stepped incrementally
__device__ void raster_serial(const RenderArgs& a, int b, int f, int X0, int Y0, int cx0, int cx1, int cy0, int cy1,
                              unsigned long long* key) {
    FaceSetup s;
    face_setup(a, b, f, s);
    long long Er[3];
    edges_at(s, 256LL * cx0 + 128, 256LL * cy0 + 128, Er);
    // stepping one pixel in x / y changes edge (a -> b) by -(by - ay) * 256 / +(bx - ax) * 256
    const long long sx[3] = {-256LL * (s.y[2] - s.y[1]), -256LL * (s.y[0] - s.y[2]), -256LL * (s.y[1] - s.y[0])};
    const long long sy[3] = {256LL * (s.x[2] - s.x[1]), 256LL * (s.x[0] - s.x[2]), 256LL * (s.x[1] - s.x[0])};
    for (int py = cy0; py <= cy1; ++py) {
        long long E[3] = {Er[0], Er[1], Er[2]};
        for (int px = cx0; px <= cx1; ++px) {
            if (inside(s, E)) {
                float l[3];
                depth_test(key, (py - Y0) * kTile + (px - X0), pix_depth(s, E, l), f);
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) E[k] += sx[k];
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) Er[k] += sy[k];
    }
}

// the whole workgroup rasterises face f, one pixel per thread
__device__ void raster_coop(const RenderArgs& a, int b, int f, int X0, int Y0, int cx0, int cx1, int cy0, int cy1, unsigned long long* key) {
    FaceSetup s;
    face_setup(a, b, f, s);
    const int cw = cx1 - cx0 + 1, n = cw * (cy1 - cy0 + 1);
    for (int i = threadIdx.x; i < n; i += kThreads) {
        const int py = cy0 + i / cw, px = cx0 + i % cw;
        long long E[3];
        edges_at(s, 256LL * px + 128, 256LL * py + 128, E);
        if (inside(s, E)) {
            float l[3];
            depth_test(key, (py - Y0) * kTile + (px - X0), pix_depth(s, E, l), f);
        }
    }
}

__device__ __forceinline__ unsigned char to_byte(float c) {
    c = fminf(fmaxf(c, 0.f), 1.f);
    return (unsigned char)(int)floorf(255.f * c + 0.5f);
}

// one workgroup per (tile, image): grid (tiles_x * tiles_y, B)
__global__ __launch_bounds__(kThreads) void render_raster_kernel(RenderArgs a) {
    __shared__ unsigned long long key[kTile * kTile];
    __shared__ int small_list[kChunk];
    __shared__ int large_list[kChunk];
    __shared__ int counts[2];
    const int b = blockIdx.y;
    const int tiles_x = (a.W + kTile - 1) / kTile;
    const int X0 = (blockIdx.x % tiles_x) * kTile, Y0 = (blockIdx.x / tiles_x) * kTile;
    const int X1 = min(X0 + kTile, a.W) - 1, Y1 = min(Y0 + kTile, a.H) - 1;
    const int t = threadIdx.x;
    for (int i = t; i < kTile * kTile; i += kThreads) key[i] = kEmptyKey;
    const uint2* boxes = a.box + (size_t)b * a.Fn;
    for (int base = 0; base < a.Fn; base += kChunk) {
        if (t < 2) counts[t] = 0;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kChunk / kThreads; ++k) {
            const int f = base + k * kThreads + t;
            if (f < a.Fn) {
                const uint2 bx = boxes[f];
                const int cx0 = max((int)(bx.x & 0xffffu), X0), cy0 = max((int)(bx.x >> 16), Y0);
                const int cx1 = min((int)(bx.y & 0xffffu), X1), cy1 = min((int)(bx.y >> 16), Y1);
                if (cx0 <= cx1 && cy0 <= cy1) {
                    if ((cx1 - cx0 + 1) * (cy1 - cy0 + 1) > kLargeArea)
                        large_list[atomicAdd(&counts[1], 1)] = f;
                    else
                        small_list[atomicAdd(&counts[0], 1)] = f;
                }
            }
        }
        __syncthreads();
        const int ns = counts[0], nl = counts[1];
        for (int i = t; i < ns; i += kThreads) {
            const int f = small_list[i];
            const uint2 bx = boxes[f];
            raster_serial(a, b, f, X0, Y0, max((int)(bx.x & 0xffffu), X0), min((int)(bx.y & 0xffffu), X1), max((int)(bx.x >> 16), Y0),
                          min((int)(bx.y >> 16), Y1), key);
        }
        for (int j = 0; j < nl; ++j) {
            const int f = large_list[j];
            const uint2 bx = boxes[f];
            raster_coop(a, b, f, X0, Y0, max((int)(bx.x & 0xffffu), X0), min((int)(bx.y & 0xffffu), X1), max((int)(bx.x >> 16), Y0),
                        min((int)(bx.y >> 16), Y1), key);
        }
        __syncthreads();
    }
    __syncthreads();
    // resolve in place
    for (int i = t; i < kTile * kTile; i += kThreads) {
        const int px = X0 + (i & (kTile - 1)), py = Y0 + i / kTile;
        if (px > X1 || py > Y1) continue;
        const size_t pix = ((size_t)b * a.H + py) * a.W + px;
        const unsigned long long k = key[i];
        if (a.out_face) {  // test hook: winning face and its depth
            if (k == kEmptyKey) {
                a.out_face[pix] = -1;
                a.out_z[pix] = 0.f;
            } else {
                a.out_face[pix] = (int)(unsigned)(k & 0xffffffffu);
                a.out_z[pix] = __uint_as_float((unsigned)(k >> 32));
            }
            continue;
        }
        unsigned char* o = a.out + pix * a.C;
        if (k == kEmptyKey) {
            if (a.bg) {
                const unsigned char* g = a.bg + pix * 3;
                o[0] = g[0];
                o[1] = g[1];
                o[2] = g[2];
            } else {
                o[0] = o[1] = o[2] = 255;
            }
            if (a.C == 4) o[3] = a.bg ? 255 : 0;
            continue;
        }
        const int f = (int)(unsigned)(k & 0xffffffffu);
        FaceSetup s;
        face_setup(a, b, f, s);
        long long E[3];
        edges_at(s, 256LL * px + 128, 256LL * py + 128, E);
        float l[3];
        const float z = pix_depth(s, E, l);
        const RenderVert* rec = a.rec + (size_t)b * a.P;
        const RenderVert v0 = rec[s.vi[0]], v1 = rec[s.vi[1]], v2 = rec[s.vi[2]];
        const float w0 = l[0] * v0.iz, w1 = l[1] * v1.iz, w2 = l[2] * v2.iz;
        o[0] = to_byte(z * (w0 * v0.r + w1 * v1.r + w2 * v2.r));
        o[1] = to_byte(z * (w0 * v0.g + w1 * v1.g + w2 * v2.g));
        o[2] = to_byte(z * (w0 * v0.b + w1 * v1.b + w2 * v2.b));
        if (a.C == 4) o[3] = 255;
    }
}

}  // namespace

hipError_t hpe_launch_render(const RenderArgs& a, int stage, hipStream_t st) {
    if (a.rotate) {
        hipLaunchKernelGGL(render_center_kernel, dim3(a.B), dim3(256), 0, st, a);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(render_vertex_kernel, dim3((a.P + 255) / 256, a.B), dim3(256), 0, st, a);
    if (stage == 0) return hipGetLastError();  // vertex records only (test hook)
    hipLaunchKernelGGL(render_face_kernel, dim3((a.Fn + 255) / 256, a.B), dim3(256), 0, st, a);
    const int tiles = ((a.W + kTile - 1) / kTile) * ((a.H + kTile - 1) / kTile);
    hipLaunchKernelGGL(render_raster_kernel, dim3(tiles, a.B), dim3(kThreads), 0, st, a);
    return hipGetLastError();
}
