// smpl_bwd.hip -- gradient of the SMPL layer + orthographic projection of smpl.hip with respect to theta rows
// [ s, tx, ty | 72 axis-angle | 10 betas ] for gfx950 (DESIGN.md "SMPL backward").
//
// Stateless: the call takes theta and recomputes what it needs into its own workspace; it does not read what a forward call left.
// Three launches, all fp32 VALU, no atomics:
//   smpl_bwd_prep_kernel    one wave per image: the arithmetic of smpl_pose_kernel again (Rs, J, G, A, pose feature), kept in
//                           the workspace, and the keypoint cotangents gathered as  gJ = g_joints + s * [g_kp2d | 0]
//   smpl_bwd_vertex_kernel  (vertex tile NT) x (image tile NI), thread = one vertex x NI images: v_posed and T recomputed as in
//                           smpl_skin_kernel, g_v = g_verts + kp_reg . gJ + verts2d chain, dv_posed = T_R^T g_v.  The reductions
//                           over the tile's vertices are small matrix products taken from LDS: thread k walks ITS basis row
//                           (posedirs / shapedirs) over the tile against dv_posed broadcast from LDS -> d pose_feature (207) and
//                           d beta (10); thread (j, e) walks weights[:, j] against g_v (x) [v_posed; 1] -> dA (288).  Every sum
//                           runs in vertex order inside one thread: per (tile, image) partials, no cross-lane reduction except
//                           the three camera sums.  <256, 8> for batches, <64, 1> (108 workgroups per image) for B <= 8.
//   smpl_bwd_finish_kernel  one workgroup per image: the tile partials added in tile order, then one wave walks the kinematic
//                           tree backwards (children -> parent through LDS, adds ordered by joint index), dJ -> d beta through
//                           j_basis, and the Rodrigues backward in the form R = cos a I + f(a) th th^T + g(a) [th]x.
#include <hip/hip_runtime.h>

#include "../../include/hpe.h"
#include "hpe_internal.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

#define V SMPL_V
#define V3 (SMPL_V * 3)
#define PART SMPL_BWD_PART
// slots of one (tile, image) partial / of the per-image sums: dA [24][12] | d pose_feature [207] | d beta [10] | camera sums [3]
#define OFF_DPF 288
#define OFF_DBETA 495
#define OFF_CAM 505
#define N_SUMS 508
#define N_BASIS 217  // 207 posedirs rows + 10 shapedirs rows

namespace {

// ---------------------------------------------------------------------------------------------
// one wave per image.  Same expressions as smpl_pose_kernel (smpl.hip) so that backward differentiates what forward computed.
__global__ __launch_bounds__(64) void smpl_bwd_prep_kernel(SmplDev d, SmplBwdWork w, const float* __restrict__ theta, int B,
                                                           const float* __restrict__ g_joints, const float* __restrict__ g_kp2d) {
    __shared__ float sR[24][9];
    __shared__ float sJ[24][3];
    __shared__ float sG[24][12];
    __shared__ float sTh[85];
    const int b = blockIdx.x;
    const int j = threadIdx.x;
    const bool live = b < B;
    const int Bpad = w.Bpad;

    for (int k = j; k < 85; k += 64) sTh[k] = live ? theta[(size_t)b * 85 + k] : 0.f;
    __syncthreads();
    if (j < 4) w.cams[b * 4 + j] = j < 3 ? sTh[j] : 0.f;
    if (j < 10) w.betaT[j * Bpad + b] = sTh[75 + j];
    if (j < 24) {
        // keypoint cotangents: [0:3] what reaches joints (the kp2d cotangent pushed back through s * (joints_xy + t)), [3:5] g_kp2d itself
        float* gj = w.gj + ((size_t)b * 24 + j) * 5;
        const bool on = live && j < d.num_kp;
        const float q0 = (on && g_kp2d) ? g_kp2d[((size_t)b * d.num_kp + j) * 2] : 0.f;
        const float q1 = (on && g_kp2d) ? g_kp2d[((size_t)b * d.num_kp + j) * 2 + 1] : 0.f;
        const float* gjo = g_joints + ((size_t)b * d.num_kp + j) * 3;
        gj[0] = ((on && g_joints) ? gjo[0] : 0.f) + sTh[0] * q0;
        gj[1] = ((on && g_joints) ? gjo[1] : 0.f) + sTh[0] * q1;
        gj[2] = (on && g_joints) ? gjo[2] : 0.f;
        gj[3] = q0;
        gj[4] = q1;

        const float x = sTh[3 + 3 * j], y = sTh[4 + 3 * j], z = sTh[5 + 3 * j];
        const float ex = x + 1e-8f, ey = y + 1e-8f, ez = z + 1e-8f;
        const float angle = sqrtf(ex * ex + ey * ey + ez * ez);
        const float rx = x / angle, ry = y / angle, rz = z / angle;
        const float c = cosf(angle), s = sinf(angle), oc = 1.0f - c;
        float R[9];
        R[0] = c + oc * (rx * rx);
        R[1] = oc * (rx * ry) + s * (-rz);
        R[2] = oc * (rx * rz) + s * ry;
        R[3] = oc * (ry * rx) + s * rz;
        R[4] = c + oc * (ry * ry);
        R[5] = oc * (ry * rz) + s * (-rx);
        R[6] = oc * (rz * rx) + s * (-ry);
        R[7] = oc * (rz * ry) + s * rx;
        R[8] = c + oc * (rz * rz);
#pragma unroll
        for (int e = 0; e < 9; ++e) sR[j][e] = R[e];
        if (j >= 1) {
#pragma unroll
            for (int e = 0; e < 9; ++e) w.pfT[((j - 1) * 9 + e) * Bpad + b] = R[e] - ((e == 0 || e == 4 || e == 8) ? 1.0f : 0.0f);
        }
#pragma unroll
        for (int cc = 0; cc < 3; ++cc) {
            float acc = 0.f;
#pragma unroll
            for (int k = 0; k < 10; ++k) acc += sTh[75 + k] * d.j_basis[((1 + k) * 24 + j) * 3 + cc];
            sJ[j][cc] = acc + d.j_basis[j * 3 + cc];
        }
    }
    __syncthreads();

    const int par = (j < 24) ? d.parents[j] : -1;
    const int dep = (j < 24) ? d.depth[j] : -1;
    for (int lvl = 0; lvl <= d.max_depth; ++lvl) {
        if (j < 24 && dep == lvl) {
            if (par < 0) {
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    sG[j][r * 4 + 0] = sR[j][r * 3 + 0];
                    sG[j][r * 4 + 1] = sR[j][r * 3 + 1];
                    sG[j][r * 4 + 2] = sR[j][r * 3 + 2];
                    sG[j][r * 4 + 3] = sJ[j][r];
                }
            } else {
                const float tx = sJ[j][0] - sJ[par][0], ty = sJ[j][1] - sJ[par][1], tz = sJ[j][2] - sJ[par][2];
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    const float p0 = sG[par][r * 4 + 0], p1 = sG[par][r * 4 + 1], p2 = sG[par][r * 4 + 2], p3 = sG[par][r * 4 + 3];
#pragma unroll
                    for (int cc = 0; cc < 3; ++cc) sG[j][r * 4 + cc] = p0 * sR[j][cc] + p1 * sR[j][3 + cc] + p2 * sR[j][6 + cc];
                    sG[j][r * 4 + 3] = p0 * tx + p1 * ty + p2 * tz + p3;
                }
            }
        }
        __syncthreads();
    }
    if (j < 24) {
        float* a = w.A + ((size_t)b * 24 + j) * 12;
        float* keep = w.rjg + ((size_t)b * 24 + j) * 24;  // R (9) | J (3) | G (12)
#pragma unroll
        for (int e = 0; e < 9; ++e) keep[e] = sR[j][e];
#pragma unroll
        for (int e = 0; e < 3; ++e) keep[9 + e] = sJ[j][e];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const float g0 = sG[j][r * 4 + 0], g1 = sG[j][r * 4 + 1], g2 = sG[j][r * 4 + 2], g3 = sG[j][r * 4 + 3];
            a[r * 4 + 0] = g0;
            a[r * 4 + 1] = g1;
            a[r * 4 + 2] = g2;
            a[r * 4 + 3] = g3 - (g0 * sJ[j][0] + g1 * sJ[j][1] + g2 * sJ[j][2]);
            keep[12 + r * 4 + 0] = g0;
            keep[12 + r * 4 + 1] = g1;
            keep[12 + r * 4 + 2] = g2;
            keep[12 + r * 4 + 3] = g3;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// grid (ceil(V / NT), images / NI); thread = one vertex x NI images in phase 1, one output row in phases 2 and 3.
// part[(img * n_tiles + tile) * PART + slot]: the sums over this tile's vertices.
template <int NT, int NI>
__global__ __launch_bounds__(NT) void smpl_bwd_vertex_kernel(SmplDev d, SmplBwdWork w, int B, const float* __restrict__ g_verts,
                                                             const float* __restrict__ g_v2d, int has_kp, int has_q, float half_w,
                                                             float half_h, int n_tiles) {
    // phase 2 reads sBuf as dvp[NT * 3][NI]; phase 3 as [NT][6][NI] = g_v (3) | v_posed (3)
    __shared__ __attribute__((aligned(16))) float sBuf[NT * 6 * NI];
    __shared__ float sCam[NT / 64][NI * 3];
    const int t = threadIdx.x;
    const int v0 = blockIdx.x * NT;
    const int vraw = v0 + t;
    const bool vok = vraw < V;
    const int v = vok ? vraw : V - 1;
    const int img0 = blockIdx.y * NI;
    const int Bpad = w.Bpad;

    // ---- phase 1: forward values of this vertex (the arithmetic of smpl_skin_kernel), then g_v and dv_posed
    float vp[NI][3];
    {
        float vs[NI][3];
#pragma unroll
        for (int i = 0; i < NI; ++i) vs[i][0] = vs[i][1] = vs[i][2] = 0.f;
#pragma unroll 2
        for (int k = 0; k < 10; ++k) {
            const float* sd = d.shapedirs + (size_t)k * V3 + 3 * v;
            const float s0 = sd[0], s1 = sd[1], s2 = sd[2];
            const float* bt = w.betaT + k * Bpad + img0;
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                const float bb = bt[i];
                vs[i][0] += bb * s0;
                vs[i][1] += bb * s1;
                vs[i][2] += bb * s2;
            }
        }
        const float t0 = d.v_template[3 * v], t1 = d.v_template[3 * v + 1], t2 = d.v_template[3 * v + 2];
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            vs[i][0] += t0;
            vs[i][1] += t1;
            vs[i][2] += t2;
            vp[i][0] = vp[i][1] = vp[i][2] = 0.f;
        }
#pragma unroll(NI == 1 ? 23 : 6)
        for (int k = 0; k < 207; ++k) {
            const float* pd = d.posedirs + (size_t)k * V3 + 3 * v;
            const float p0 = pd[0], p1 = pd[1], p2 = pd[2];
            const float* pf = w.pfT + k * Bpad + img0;
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                const float f = pf[i];
                vp[i][0] += f * p0;
                vp[i][1] += f * p1;
                vp[i][2] += f * p2;
            }
        }
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            vp[i][0] += vs[i][0];
            vp[i][1] += vs[i][1];
            vp[i][2] += vs[i][2];
        }
    }
    float wgt[24], reg[24];
    {
        const f32x4* wp = reinterpret_cast<const f32x4*>(d.weights + (size_t)v * 24);
        const f32x4* rp = reinterpret_cast<const f32x4*>(d.kp_reg + (size_t)v * 24);
#pragma unroll
        for (int q = 0; q < 6; ++q) {
            const f32x4 a = wp[q];
            wgt[4 * q] = a.x, wgt[4 * q + 1] = a.y, wgt[4 * q + 2] = a.z, wgt[4 * q + 3] = a.w;
            if (has_kp) {
                const f32x4 r = rp[q];
                reg[4 * q] = r.x, reg[4 * q + 1] = r.y, reg[4 * q + 2] = r.z, reg[4 * q + 3] = r.w;
            } else {
                reg[4 * q] = reg[4 * q + 1] = reg[4 * q + 2] = reg[4 * q + 3] = 0.f;
            }
        }
    }
    float gv[NI][3];
    float cam_s[NI][3];  // h . verts_xy | g_verts2d x | g_verts2d y  (this vertex)
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int img = img0 + i;
        const bool on = vok && img < B;
        const float* Ai = w.A + (size_t)img * 288;
        float T[12];
#pragma unroll
        for (int e = 0; e < 12; ++e) T[e] = 0.f;
#pragma unroll
        for (int jj = 0; jj < 24; ++jj) {
#pragma unroll
            for (int e = 0; e < 12; ++e) T[e] += wgt[jj] * Ai[jj * 12 + e];
        }
        float g0 = 0.f, g1 = 0.f, g2 = 0.f, h0 = 0.f, h1 = 0.f;
        if (has_kp) {
            const float* gj = w.gj + (size_t)img * 120;
#pragma unroll
            for (int k = 0; k < 24; ++k) {
                g0 += reg[k] * gj[k * 5 + 0];
                g1 += reg[k] * gj[k * 5 + 1];
                g2 += reg[k] * gj[k * 5 + 2];
            }
            if (has_q) {
#pragma unroll
                for (int k = 0; k < 24; ++k) {
                    h0 += reg[k] * gj[k * 5 + 3];
                    h1 += reg[k] * gj[k * 5 + 4];
                }
            }
        }
        if (g_verts && on) {
            const float* gp = g_verts + ((size_t)img * V + v) * 3;
            g0 += gp[0];
            g1 += gp[1];
            g2 += gp[2];
        }
        float e0 = 0.f, e1 = 0.f;
        if (g_v2d && on) {
            // verts2d = (s * (x + t) + 1) * 0.5 * size
            const float* gp = g_v2d + ((size_t)img * V + v) * 2;
            e0 = gp[0] * half_w;
            e1 = gp[1] * half_h;
            const float s = w.cams[img * 4];
            g0 += s * e0;
            g1 += s * e1;
            h0 += e0;
            h1 += e1;
        }
        if (!on) g0 = g1 = g2 = h0 = h1 = 0.f;
        gv[i][0] = g0;
        gv[i][1] = g1;
        gv[i][2] = g2;
        const float px = vp[i][0], py = vp[i][1], pz = vp[i][2];
        const float ox = T[0] * px + T[1] * py + T[2] * pz + T[3];
        const float oy = T[4] * px + T[5] * py + T[6] * pz + T[7];
        cam_s[i][0] = h0 * ox + h1 * oy;
        cam_s[i][1] = e0;
        cam_s[i][2] = e1;
        // dv_posed = T_R^T g_v
        sBuf[(3 * t + 0) * NI + i] = T[0] * g0 + T[4] * g1 + T[8] * g2;
        sBuf[(3 * t + 1) * NI + i] = T[1] * g0 + T[5] * g1 + T[9] * g2;
        sBuf[(3 * t + 2) * NI + i] = T[2] * g0 + T[6] * g1 + T[10] * g2;
    }
    // the three camera sums: wave shuffle tree (fixed), then the waves in order
    {
        const int lane = t & 63, wave = t >> 6;
#pragma unroll
        for (int i = 0; i < NI; ++i)
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                float s = cam_s[i][e];
#pragma unroll
                for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
                if (lane == 0) sCam[wave][i * 3 + e] = s;
            }
    }
    __syncthreads();
    if (t < NI * 3) {
        float s = sCam[0][t];
#pragma unroll
        for (int wv = 1; wv < NT / 64; ++wv) s += sCam[wv][t];
        const int img = img0 + t / 3;
        w.part[((size_t)img * n_tiles + blockIdx.x) * PART + OFF_CAM + t % 3] = s;
    }

    // ---- phase 2: d pose_feature[k] / d beta[k] = sum over the tile of basis_k[v, c] * dv_posed[v, c]
    const int nv = (V - v0) < NT ? (V - v0) : NT;  // vertices of this tile (even times 3: the float2 walk below stays inside the row)
    for (int o = t; o < N_BASIS; o += NT) {
        const float* row = (o < 207 ? d.posedirs + (size_t)o * V3 : d.shapedirs + (size_t)(o - 207) * V3) + 3 * v0;
        float acc[NI];
#pragma unroll
        for (int i = 0; i < NI; ++i) acc[i] = 0.f;
#pragma unroll 4
        for (int vc = 0; vc < 3 * nv; vc += 2) {
            const f32x2 p = *reinterpret_cast<const f32x2*>(row + vc);
#pragma unroll
            for (int i = 0; i < NI; ++i) acc[i] += p.x * sBuf[vc * NI + i];
#pragma unroll
            for (int i = 0; i < NI; ++i) acc[i] += p.y * sBuf[(vc + 1) * NI + i];
        }
#pragma unroll
        for (int i = 0; i < NI; ++i) w.part[((size_t)(img0 + i) * n_tiles + blockIdx.x) * PART + OFF_DPF + o] = acc[i];
    }
    __syncthreads();
    // ---- phase 3: dA[j][r][c] = sum over the tile of weights[v, j] * g_v[r] * [v_posed; 1][c]
#pragma unroll
    for (int i = 0; i < NI; ++i) {
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            sBuf[(t * 6 + e) * NI + i] = gv[i][e];
            sBuf[(t * 6 + 3 + e) * NI + i] = vp[i][e];
        }
    }
    __syncthreads();
    for (int o = t; o < 288; o += NT) {
        const int j = o / 12, r = (o % 12) >> 2, c = o & 3;
        const float* wj = d.weights + (size_t)v0 * 24 + j;
        float acc[NI];
#pragma unroll
        for (int i = 0; i < NI; ++i) acc[i] = 0.f;
#pragma unroll 4
        for (int vv = 0; vv < nv; ++vv) {
            const float ww = wj[vv * 24];
            const float* gr = sBuf + (vv * 6 + r) * NI;
            const float* pc = sBuf + (vv * 6 + 3 + (c < 3 ? c : 0)) * NI;
#pragma unroll
            for (int i = 0; i < NI; ++i) acc[i] += ww * (gr[i] * (c < 3 ? pc[i] : 1.0f));
        }
#pragma unroll
        for (int i = 0; i < NI; ++i) w.part[((size_t)(img0 + i) * n_tiles + blockIdx.x) * PART + o] = acc[i];
    }
}

// ---------------------------------------------------------------------------------------------
// d theta_j (3) from the cotangent M of R_j.  R = cos a I + f th th^T + g [th]x with a = ||th + 1e-8||, f = (1 - cos a) / a^2,
// g = sin a / a (what batch_rodrigues computes as r = th / a).  With e = th + 1e-8 (da/dth_i = e_i / a):
//   dR/dth_i = e_i (-g I + (f'/a) th th^T + (g'/a) [th]x) + f (u_i th^T + th u_i^T) + g [u_i]x
// f, g, f'/a, g'/a are even in a: series below a = 1 (no 0/0 and no cancellation at the 23 zero joints of the mean pose).
__device__ __forceinline__ void rodrigues_bwd(float x, float y, float z, const float* M, float* out) {
    const float ex = x + 1e-8f, ey = y + 1e-8f, ez = z + 1e-8f;
    const float a2 = ex * ex + ey * ey + ez * ez;
    float f, g, fp, gp;
    if (a2 < 1.0f) {
        g = 1.0f + a2 * (-1.0f / 6 + a2 * (1.0f / 120 + a2 * (-1.0f / 5040 + a2 * (1.0f / 362880 + a2 * (-1.0f / 39916800)))));
        f = 0.5f + a2 * (-1.0f / 24 + a2 * (1.0f / 720 + a2 * (-1.0f / 40320 + a2 * (1.0f / 3628800 + a2 * (-1.0f / 479001600)))));
        gp = -1.0f / 3 + a2 * (1.0f / 30 + a2 * (-1.0f / 840 + a2 * (1.0f / 45360 + a2 * (-1.0f / 3991680 + a2 * (1.0f / 518918400)))));
        fp = -1.0f / 12 + a2 * (1.0f / 180 + a2 * (-1.0f / 6720 + a2 * (1.0f / 453600 + a2 * (-1.0f / 47900160 + a2 * (1.0f / 7264857600.0f)))));
    } else {
        const float a = sqrtf(a2);
        const float s = sinf(a), c = cosf(a);
        g = s / a;
        f = (1.0f - c) / a2;
        gp = (a * c - s) / (a * a2);
        fp = (a * s - 2.0f * (1.0f - c)) / (a2 * a2);
    }
    const float m0 = M[0] * x + M[1] * y + M[2] * z, m1 = M[3] * x + M[4] * y + M[5] * z, m2 = M[6] * x + M[7] * y + M[8] * z;  // M th
    const float n0 = M[0] * x + M[3] * y + M[6] * z, n1 = M[1] * x + M[4] * y + M[7] * z, n2 = M[2] * x + M[5] * y + M[8] * z;  // M^T th
    const float k0 = M[7] - M[5], k1 = M[2] - M[6], k2 = M[3] - M[1];  // <M, [u_i]x>
    const float common = -g * (M[0] + M[4] + M[8]) + fp * (x * m0 + y * m1 + z * m2) + gp * (x * k0 + y * k1 + z * k2);
    out[0] = ex * common + f * (m0 + n0) + g * k0;
    out[1] = ey * common + f * (m1 + n1) + g * k1;
    out[2] = ez * common + f * (m2 + n2) + g * k2;
}

// one workgroup per image
__global__ __launch_bounds__(512) void smpl_bwd_finish_kernel(SmplDev d, SmplBwdWork w, const float* __restrict__ theta, int n_tiles,
                                                              HpeOutputs g, float half_w, float half_h,
                                                              float* __restrict__ grad_theta) {
    __shared__ float sSum[512];
    __shared__ float sK[24][24];   // R (9) | J (3) | G (12) of the forward
    __shared__ float sdG[24][12];  // cotangent of G
    __shared__ float sdJ[24][3];
    __shared__ float sC[24][15];   // what joint j hands to its parent: dG (12) | dJ (3)
    __shared__ int sPar[24];
    const int b = blockIdx.x;
    const int t = threadIdx.x;
    {
        // the tile partials in tile order: four interleaved chains, then the chains (as smpl_kp_finish_kernel)
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
        if (t < N_SUMS) {
            const float* p = w.part + (size_t)b * n_tiles * PART + t;
            int i = 0;
            for (; i + 3 < n_tiles; i += 4) {
                s0 += p[(size_t)i * PART];
                s1 += p[(size_t)(i + 1) * PART];
                s2 += p[(size_t)(i + 2) * PART];
                s3 += p[(size_t)(i + 3) * PART];
            }
            for (; i < n_tiles; ++i) s0 += p[(size_t)i * PART];
        }
        sSum[t] = (s0 + s1) + (s2 + s3);
    }
    for (int k = t; k < 576; k += 512) sK[k / 24][k % 24] = w.rjg[(size_t)b * 576 + k];
    if (t < 24) sPar[t] = d.parents[t];
    __syncthreads();

    const int j = t;
    const bool act = t < 24;
    const int par = act ? sPar[j] : -1;
    const int dep = act ? d.depth[j] : -1;
    if (act) {
        // A = [G_R | G_t - G_R J];  J_transformed = G_t
        const float* dA = sSum + j * 12;
        float dj[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const float at = dA[r * 4 + 3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                sdG[j][r * 4 + c] = dA[r * 4 + c] - at * sK[j][9 + c];
                dj[c] -= sK[j][12 + r * 4 + c] * at;
            }
            sdG[j][r * 4 + 3] = at + (g.J_transformed ? g.J_transformed[((size_t)b * 24 + j) * 3 + r] : 0.f);
        }
        sdJ[j][0] = dj[0], sdJ[j][1] = dj[1], sdJ[j][2] = dj[2];
    }
    __syncthreads();
    float dR[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) dR[e] = 0.f;
    // G_j = G_p . [R_j | J_j - J_p]: children of a level hand their share to the parent, which adds them by joint index
    for (int lvl = d.max_depth; lvl >= 1; --lvl) {
        if (act && dep == lvl) {
            const float* Gp = &sK[par][12];
            const float* Rj = &sK[j][0];
            const float tj[3] = {sK[j][9] - sK[par][9], sK[j][10] - sK[par][10], sK[j][11] - sK[par][11]};
            float dG[12];
#pragma unroll
            for (int e = 0; e < 12; ++e) dG[e] = sdG[j][e];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
#pragma unroll
                for (int c = 0; c < 3; ++c) dR[a * 3 + c] = Gp[a] * dG[c] + Gp[4 + a] * dG[4 + c] + Gp[8 + a] * dG[8 + c];
                const float dt = Gp[a] * dG[3] + Gp[4 + a] * dG[7] + Gp[8 + a] * dG[11];
                sdJ[j][a] += dt;
                sC[j][12 + a] = -dt;
            }
#pragma unroll
            for (int r = 0; r < 3; ++r) {
#pragma unroll
                for (int a = 0; a < 3; ++a)
                    sC[j][r * 4 + a] = dG[r * 4 + 0] * Rj[a * 3 + 0] + dG[r * 4 + 1] * Rj[a * 3 + 1] + dG[r * 4 + 2] * Rj[a * 3 + 2] + dG[r * 4 + 3] * tj[a];
                sC[j][r * 4 + 3] = dG[r * 4 + 3];
            }
        }
        __syncthreads();
        if (act && dep == lvl - 1) {
            for (int k = 0; k < 24; ++k) {
                if (sPar[k] != j) continue;
#pragma unroll
                for (int e = 0; e < 12; ++e) sdG[j][e] += sC[k][e];
#pragma unroll
                for (int e = 0; e < 3; ++e) sdJ[j][e] += sC[k][12 + e];
            }
        }
        __syncthreads();
    }
    if (act) {
        if (par < 0) {
            // G_0 = [R_0 | J_0]
#pragma unroll
            for (int r = 0; r < 3; ++r) {
#pragma unroll
                for (int c = 0; c < 3; ++c) dR[r * 3 + c] = sdG[j][r * 4 + c];
                sdJ[j][r] += sdG[j][r * 4 + 3];
            }
        }
        // pose_feature = R - I (joints 1..23), and the cotangent of the Rs output
#pragma unroll
        for (int e = 0; e < 9; ++e) {
            if (j >= 1) dR[e] += sSum[OFF_DPF + (j - 1) * 9 + e];
            if (g.Rs) dR[e] += g.Rs[((size_t)b * 24 + j) * 9 + e];
        }
        const float* th = theta + (size_t)b * 85 + 3 + 3 * j;
        float o[3];
        rodrigues_bwd(th[0], th[1], th[2], dR, o);
#pragma unroll
        for (int e = 0; e < 3; ++e)
            grad_theta[(size_t)b * 85 + 3 + 3 * j + e] = o[e] + (g.theta ? g.theta[(size_t)b * 85 + 3 + 3 * j + e] : 0.f);
    }
    __syncthreads();
    if (t < 10) {
        // J = j_basis[0] + sum_k beta_k j_basis[1 + k]; v_shaped = v_template + sum_k beta_k shapedirs[k]
        float acc = sSum[OFF_DBETA + t];
        for (int jj = 0; jj < 24; ++jj) {
            const float* jb = d.j_basis + ((1 + t) * 24 + jj) * 3;
            acc += sdJ[jj][0] * jb[0] + sdJ[jj][1] * jb[1] + sdJ[jj][2] * jb[2];
        }
        grad_theta[(size_t)b * 85 + 75 + t] = acc + (g.theta ? g.theta[(size_t)b * 85 + 75 + t] : 0.f);
    } else if (t >= 64 && t < 67) {
        // kp2d = s (joints_xy + t); verts2d = (s (verts_xy + t) + 1) * 0.5 * size
        const int e = t - 64;
        const float s = w.cams[b * 4], tx = w.cams[b * 4 + 1], ty = w.cams[b * 4 + 2];
        float q0 = 0.f, q1 = 0.f;
        const float* gj = w.gj + (size_t)b * 120;
        for (int k = 0; k < 24; ++k) {
            q0 += gj[k * 5 + 3];
            q1 += gj[k * 5 + 4];
        }
        q0 += sSum[OFF_CAM + 1];
        q1 += sSum[OFF_CAM + 2];
        float r = e == 0 ? sSum[OFF_CAM] + (tx * q0 + ty * q1) : s * (e == 1 ? q0 : q1);
        if (g.cams) r += g.cams[(size_t)b * 3 + e];
        if (g.theta) r += g.theta[(size_t)b * 85 + e];
        grad_theta[(size_t)b * 85 + e] = r;
    }
}

}  // namespace

size_t hpe_smpl_bwd_part_floats(int Bpad) {
    const size_t big = (size_t)Bpad * ((V + 255) / 256), small = (size_t)SMPL_SMALL_B * ((V + 63) / 64);
    return (big > small ? big : small) * PART;
}

hipError_t hpe_launch_smpl_backward(const SmplDev& d, const SmplBwdWork& w, const float* theta, int B, const HpeOutputs* g,
                                    float* grad_theta, hipStream_t st) {
    const int Bpad = ((B + SMPL_IMG_TILE - 1) / SMPL_IMG_TILE) * SMPL_IMG_TILE;
    if (Bpad > w.Bpad) return hipErrorInvalidValue;
    const bool vertex_side = g->verts || g->joints || g->kp2d || g->verts2d;
    if (!vertex_side && !g->J_transformed && !g->Rs && !g->cams && !g->theta)
        return hipMemsetAsync(grad_theta, 0, (size_t)B * 85 * sizeof(float), st);
    const float half = 0.5f * (float)HPE_IMG_SIZE;
    hipLaunchKernelGGL(smpl_bwd_prep_kernel, dim3(Bpad), dim3(64), 0, st, d, w, theta, B, g->joints, g->kp2d);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    int n_tiles = 0;
    if (vertex_side) {
        const int has_kp = (g->joints || g->kp2d) ? 1 : 0, has_q = g->kp2d ? 1 : 0;
        if (B <= SMPL_SMALL_B) {
            n_tiles = (V + 63) / 64;
            hipLaunchKernelGGL((smpl_bwd_vertex_kernel<64, 1>), dim3(n_tiles, B), dim3(64), 0, st, d, w, B, g->verts, g->verts2d, has_kp,
                               has_q, half, half, n_tiles);
        } else {
            n_tiles = (V + 255) / 256;
            hipLaunchKernelGGL((smpl_bwd_vertex_kernel<256, SMPL_IMG_TILE>), dim3(n_tiles, Bpad / SMPL_IMG_TILE), dim3(256), 0, st, d, w, B,
                               g->verts, g->verts2d, has_kp, has_q, half, half, n_tiles);
        }
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(smpl_bwd_finish_kernel, dim3(B), dim3(512), 0, st, d, w, theta, n_tiles, *g, half, half, grad_theta);
    return hipGetLastError();
}
