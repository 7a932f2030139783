// encoder_grad_bf16.hip -- the kernels of the mixed-precision encoder walks and their launchers: bf16 activations, bf16 cotangents, bf16
// matrix products with fp32 accumulation, fp32 gradients of fp32 master weights (encoder_train.hip holds the walks; DESIGN.md section 4,
// "Mixed-precision encoder training", states the rounding points).  The launchers are the cmx16 / mx16 overloads of those of
// encoder_grad.hip (gate, weight_grad, data_grad, scatter2, avgpool_bwd, maxpool_bwd), plus the weight cast and the layer's bf16 convolution.
//
// conv_wg_gemm_bf16_kernel: G[k][n] = sum_m A[m][k] dz[m][n] on v_mfma_f32_32x32x16_bf16.  The reduction index is the pixel, and the MFMA
// wants eight reduction elements per lane, while NHWC memory has the channels contiguous: the operands are transposed in registers.  For
// each of its eight pixels a lane loads ONE dword = channels (2r, 2r + 1) of x (r = lane & 31: 32 lanes read one 128-byte line), and one
// dword = columns (2r, 2r + 1) of dz; the low halves of the eight dwords are the even-channel fragment, the high halves the odd-channel
// one.  Two operands per side feed four MFMAs on a 64 x 64 tile per 16 pixels (the fp32 kernel: 16 loads and 16 MFMAs per 8 pixels).
// Accumulator row i of the even (odd) fragment is channel 2i (2i + 1), column c of the even (odd) one is column 2c (2c + 1): the store
// undoes both, and writes the column pair as one 8-byte word.  The two lane halves take the even and the odd pixels of a group of 16 (a
// sum does not care which pixel sits at which reduction index, as long as both operands agree), so the pixel walk is the fp32 kernel's.
// Every layer has an even Cin (conv1 reads the padded bf16 input, 4 channels a pixel, the 4th zero), so a channel pair never straddles a
// tap.  Grid (tile, slice), one wave a workgroup, the partials [slices][K][N] and the column sums of dz per slice as in encoder_grad.hip;
// no atomics, every sum in a fixed ascending order.  Rows past M, taps outside the map and columns past K / N are masked, never read.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "hpe_ctx.h"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

struct WgArgs16 {
    const unsigned short* x;   // the layer's input, NHWC [B][Hi][Wi][Cin] bf16
    const unsigned short* dz;  // [M][N] bf16
    float* part;               // [slices][K][N]
    float* dsh;                // [slices][N] column sums of dz
    int M, K, N;               // K = taps * Cin, even; N even
    int Hi, Wi, Cin, Ho, Wo, kw, stride, pad;
    int P;     // pixels per slice, a multiple of 16
    int n_nt;  // tiles along N
};

__device__ __forceinline__ float bf16_lo(unsigned d) { return __uint_as_float(d << 16); }
__device__ __forceinline__ float bf16_hi(unsigned d) { return __uint_as_float(d & 0xffff0000u); }

__global__ __launch_bounds__(64) void conv_wg_gemm_bf16_kernel(WgArgs16 a) {
    const int lane = threadIdx.x, hi = lane >> 5, l31 = lane & 31;
    const int kt = blockIdx.x / a.n_nt, nt = blockIdx.x - kt * a.n_nt, slice = blockIdx.y;
    const int k0 = kt * 64, n0 = nt * 64;
    // lane l loads channels (k, k + 1) and columns (col, col + 1) of pixel m, m + 2, ..., m + 14; the lane halves take m = even / odd
    const int k = k0 + 2 * l31, col = n0 + 2 * l31;
    const bool kok = k < a.K, nok = col < a.N;
    const int tap = k / a.Cin, ch = k - tap * a.Cin;
    const int kh = tap / a.kw, kwi = tap - kh * a.kw;
    const long koff = ((long)kh * a.Wi + kwi) * a.Cin + ch;
    const int m_end = min(a.M, (slice + 1) * a.P);
    int m = slice * a.P + hi;
    int b = m / (a.Ho * a.Wo);
    int r = m - b * (a.Ho * a.Wo);
    int ho = r / a.Wo, wo = r - ho * a.Wo;
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
    float bs[2] = {0.f, 0.f};
    for (int it = 0; it < a.P; it += 16) {  // eight steps of two pixels, all 16 loads issued before the first MFMA
        unsigned av[8], bv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const bool live = m < m_end;
            const int h0 = ho * a.stride - a.pad, w0 = wo * a.stride - a.pad;
            const long base = (((long)b * a.Hi + h0) * a.Wi + w0) * a.Cin;
            const bool in = live && kok && (unsigned)(h0 + kh) < (unsigned)a.Hi && (unsigned)(w0 + kwi) < (unsigned)a.Wi;
            av[u] = in ? *reinterpret_cast<const unsigned*>(a.x + base + koff) : 0u;
            bv[u] = (live && nok) ? *reinterpret_cast<const unsigned*>(a.dz + (long)m * a.N + col) : 0u;
            m += 2;
            wo += 2;
            if (wo >= a.Wo) {  // Wo >= 2 (weight_grad refuses anything else): one wrap per step
                wo -= a.Wo;
                if (++ho >= a.Ho) {
                    ho = 0;
                    ++b;
                }
            }
        }
        u32x4 ae, ao, be, bo;  // element j of a fragment: pixel 2j + hi of the group
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            ae[q] = (av[2 * q] & 0xffffu) | (av[2 * q + 1] << 16);
            ao[q] = (av[2 * q] >> 16) | (av[2 * q + 1] & 0xffff0000u);
            be[q] = (bv[2 * q] & 0xffffu) | (bv[2 * q + 1] << 16);
            bo[q] = (bv[2 * q] >> 16) | (bv[2 * q + 1] & 0xffff0000u);
        }
        const bf16x8 fae = __builtin_bit_cast(bf16x8, ae), fao = __builtin_bit_cast(bf16x8, ao);
        const bf16x8 fbe = __builtin_bit_cast(bf16x8, be), fbo = __builtin_bit_cast(bf16x8, bo);
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fae, fbe, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fae, fbo, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fao, fbe, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fao, fbo, acc[1][1], 0, 0, 0);
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            bs[0] += bf16_lo(bv[u]);
            bs[1] += bf16_hi(bv[u]);
        }
    }
    // accumulator element e of lane l: row i = (e & 3) + 8 (e >> 2) + 4 (l >> 5) = channel k0 + 2 i + (0 even, 1 odd fragment); column
    // l & 31 = column n0 + 2 (l & 31) + (0 even, 1 odd)
    float* part = a.part + (size_t)slice * a.K * a.N;
    if (nok) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = k0 + 2 * ((e & 3) + 8 * (e >> 2) + 4 * hi) + i;
                if (row < a.K) *reinterpret_cast<float2*>(part + (size_t)row * a.N + col) = make_float2(acc[i][0][e], acc[i][1][e]);
            }
    }
    if (kt == 0) {  // workgroup-uniform: the first tile row also owns the column sums of dz (even + odd pixels)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const float other = __shfl_xor(bs[j], 32, 64);
            if (hi == 0 && nok) a.dsh[(size_t)slice * a.N + col + j] = bs[j] + other;
        }
    }
}

// conv_wg_fixup_kernel of encoder_grad.hip with the weight read as the forward read it: G = sum over the slices (ascending, four loads in
// flight); dW = s * G; wgp[kc][n] = sum over the 4 rows of chunk kc of W16 * G.  k runs over the HWIO rows of dW.
//   stem 0: partial row k;              W16(k, n) = w16[(k % cin) * wrow + (taps - 1 - k / cin) * N + n]   (the data-gradient operand)
//   stem 1: partial row 4 (k / 3) + k % 3; W16(k, n) = w16[n * wrow + (t / 7) * 32 + (t % 7) * 4 + k % 3], t = k / 3   (conv1: Wt[n][k])
// kp: rows of one slice's partial
__global__ __launch_bounds__(256) void conv_wg_fixup_bf16_kernel(const float* __restrict__ part, int slices, int K, int kp, int N,
                                                                 const unsigned short* __restrict__ w16, int stem, int cin, int taps, int wrow,
                                                                 const float* __restrict__ s, float* __restrict__ dW, float* __restrict__ wgp) {
    __shared__ float red[4][64];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int n = blockIdx.x * 64 + tx, k = blockIdx.y * 4 + ty;
    float acc = 0.f;
    if (n < N && k < K) {
        const int t = k / cin, ci = k - t * cin;
        const size_t o = (size_t)(stem ? 4 * t + ci : k) * N + n, kn = (size_t)kp * N;
        float g = 0.f;
        int sl = 0;
        for (; sl + 4 <= slices; sl += 4) {
            const float p0 = part[(size_t)sl * kn + o], p1 = part[(size_t)(sl + 1) * kn + o], p2 = part[(size_t)(sl + 2) * kn + o],
                        p3 = part[(size_t)(sl + 3) * kn + o];
            g = (((g + p0) + p1) + p2) + p3;
        }
        for (; sl < slices; ++sl) g += part[(size_t)sl * kn + o];
        dW[(size_t)k * N + n] = s[n] * g;
        const size_t wo = stem ? (size_t)n * wrow + (t / 7) * 32 + (t % 7) * 4 + ci : (size_t)ci * wrow + (size_t)(taps - 1 - t) * N + n;
        acc = __uint_as_float((unsigned)w16[wo] << 16) * g;
    }
    red[ty][tx] = acc;
    __syncthreads();
    if (ty == 0 && n < N) wgp[(size_t)blockIdx.y * N + n] = ((red[0][tx] + red[1][tx]) + red[2][tx]) + red[3][tx];
}

// W16 = RNE(W) of every segment of the table, four elements a thread: grid (x, segments)
__global__ __launch_bounds__(256) void enc_cast_weights_kernel(const MxCastSeg* __restrict__ table) {
    const MxCastSeg sg = table[blockIdx.y];
    for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < sg.quads; q += (long)gridDim.x * 256) {
        const f32x4 v = reinterpret_cast<const f32x4*>(sg.src)[q];
        const long e = q * 4, row = e / sg.src_pitch;
        const int cl = (int)(e - row * sg.src_pitch);
        __bf16 o[4] = {(__bf16)v.x, (__bf16)v.y, (__bf16)v.z, (__bf16)v.w};
        *reinterpret_cast<uint2*>(sg.dst + row * sg.dst_pitch + cl) = *reinterpret_cast<const uint2*>(o);
    }
}

// dz = dy * [y > 0] (y == nullptr: no activation, dz = dy), exact; dzs = RNE(dz * s[n]): one fp32 multiply, one rounding.  dz / dzs may be
// nullptr; dz may alias dy.  n8 groups of eight, N % 8 == 0
__global__ __launch_bounds__(256) void enc_gate_bf16_kernel(const bf16x8* dy, const bf16x8* __restrict__ y, const float* __restrict__ s, bf16x8* dz,
                                                            bf16x8* __restrict__ dzs, long n8, int N8) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n8) return;
    bf16x8 v = dy[i];
    if (y) {
        const bf16x8 a = y[i];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = (float)a[u] > 0.f ? v[u] : (__bf16)0.f;
    }
    if (dz) dz[i] = v;
    if (dzs) {
        const float* sc = s + (i % N8) * 8;
        bf16x8 o;
#pragma unroll
        for (int u = 0; u < 8; ++u) o[u] = (__bf16)((float)v[u] * sc[u]);
        dzs[i] = o;
    }
}

// dx [B][HW][C] = RNE(dy [B][C] / HW), dy fp32; eight channels a thread
__global__ __launch_bounds__(256) void enc_avgpool_bwd_bf16_kernel(const float* __restrict__ dy, bf16x8* __restrict__ dx, int B, int HW, int C8) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)B * HW * C8) return;
    const int c = (int)(i % C8), b = (int)(i / ((long)HW * C8));
    const float* src = dy + ((long)b * C8 + c) * 8;
    bf16x8 o;
#pragma unroll
    for (int u = 0; u < 8; ++u) o[u] = (__bf16)(src[u] / (float)HW);
    dx[i] = o;
}

// enc_maxpool_bwd_kernel on bf16 maps, eight channels a thread: every cotangent goes to the first maximum of its window in row-major
// order, the pad (value 0) taking part; the (at most four) cotangents of a pixel are summed in fp32, in row-major window order, and
// rounded once
__global__ __launch_bounds__(256) void enc_maxpool_bwd_bf16_kernel(const bf16x8* __restrict__ x, const bf16x8* __restrict__ dy, bf16x8* __restrict__ dx,
                                                                   int B, int H, int C8) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)B * H * H * C8) return;
    const int Ho = H / 2;
    const int c = (int)(i % C8);
    long r = i / C8;
    const int w = (int)(r % H);
    r /= H;
    const int h = (int)(r % H), b = (int)(r / H);
    float g[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) g[u] = 0.f;
    for (int ho = h / 2; ho <= (h + 1) / 2; ++ho) {
        if (ho >= Ho) continue;
        for (int wo = w / 2; wo <= (w + 1) / 2; ++wo) {
            if (wo >= Ho) continue;
            float best[8];
            int by[8], bx[8];
            for (int dy_ = 0; dy_ < 3; ++dy_)
                for (int dx_ = 0; dx_ < 3; ++dx_) {
                    const int yy = 2 * ho - 1 + dy_, xx = 2 * wo - 1 + dx_;
                    const bool in = (unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)H;
                    bf16x8 v;
                    if (in) v = x[(((long)b * H + yy) * H + xx) * C8 + c];
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const float f = in ? (float)v[u] : 0.f;
                        if ((dy_ == 0 && dx_ == 0) || f > best[u]) {
                            best[u] = f;
                            by[u] = in ? yy : -2;
                            bx[u] = xx;
                        }
                    }
                }
            const bf16x8 d = dy[(((long)b * Ho + ho) * Ho + wo) * C8 + c];
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (by[u] == h && bx[u] == w) g[u] += (float)d[u];
        }
    }
    bf16x8 o;
#pragma unroll
    for (int u = 0; u < 8; ++u) o[u] = (__bf16)g[u];
    dx[i] = o;
}

const float* as_f(const unsigned short* p) { return reinterpret_cast<const float*>(p); }
float* as_f(unsigned short* p) { return reinterpret_cast<float*>(p); }

}  // namespace

hipError_t mx_cast_launch(hpe_ctx* c, int first, int segs, hipStream_t st) {
    if (first < 0 || segs < 1 || first + segs > MX_CAST_SEGS) return hipErrorInvalidValue;
    hipLaunchKernelGGL(enc_cast_weights_kernel, dim3(64, segs), dim3(256), 0, st, static_cast<const MxCastSeg*>(c->et.mx_cast) + first);
    return hipGetLastError();
}

hipError_t mx_conv_forward(hpe_ctx* c, int idx, cmx16 x, int B, cmx16 res, int relu, mx16 y, hipStream_t st, const float* scale, const float* shift) {
    const ConvSpec& s = specs()[idx];
    const ConvLayer& L = c->conv[idx];
    if (!scale) scale = L.scale, shift = L.shift;
    const int kp = conv_k_pad(idx, true);
    // the kernel and tile a bf16 context would take for this layer alone on the device (a bf16 route never asks for a Winograd workspace)
    const ConvRoute r = route_conv(c->plan, true, idx, ConvQuery{B, false, res != nullptr, false});
    if (r.kernel == CONV_K_HALO3) {
        Halo3Args h{};
        h.x = reinterpret_cast<const __bf16*>(x), h.w = reinterpret_cast<const __bf16*>(c->et.mx_w[idx]), h.y = reinterpret_cast<__bf16*>(y);
        h.scale = scale, h.shift = shift;
        h.M = B * s.hout * s.hout, h.N = s.cout, h.ldw = kp;
        h.relu = relu, h.two = c->plan.halo3_two;
        return hpe_launch_halo3_bf16(h, s.hin, s.cin, st);
    }
    if (r.kernel != CONV_K_BF16 && r.kernel != CONV_K_BF16_P8) return hipErrorInvalidValue;
    GemmArgs p{};
    p.x = as_f(x), p.w = as_f(c->et.mx_w[idx]), p.scale = scale, p.shift = shift, p.res = as_f(res), p.y = as_f(y), p.zero = c->zeros;
    p.M = B * s.hout * s.hout, p.N = s.cout, p.K = kp;
    p.lda = s.cin, p.ldw = kp, p.w_rows = L.n_pad, p.ldy = p.ldres = s.cout;
    p.Hi = p.Wi = s.hin, p.Cin = s.cin, p.Ho = p.Wo = s.hout, p.stride = s.stride;
    p.cin_slabs = s.cin / 64;
    p.relu = relu;
    if (r.mode == GEMM_STEM) p.Hi = STEM_HP, p.Wi = STEM_WP, p.Cin = 4;
    p.partial = c->partial, p.partial_floats = c->partial_floats;
    return hpe_launch_gemm_bf16(p, r.mode, r.tile, st);
}

void gate(cmx16 dy, cmx16 y, const float* s, mx16 dz, mx16 dzs, long n, int N, hipStream_t st) {
    hipLaunchKernelGGL(enc_gate_bf16_kernel, grid1(n / 8), dim3(256), 0, st, reinterpret_cast<const bf16x8*>(dy), reinterpret_cast<const bf16x8*>(y), s,
                       reinterpret_cast<bf16x8*>(dz), reinterpret_cast<bf16x8*>(dzs), n / 8, N / 8);
}

hipError_t weight_grad(hpe_ctx* c, int idx, cmx16 x, cmx16 dz, int B, float* grad_layer, hipStream_t st, bool bn) {
    const ConvSpec& s = specs()[idx];
    EncTrainWork& w = c->et;
    const bool stem = idx == 0;
    WgArgs16 a{};
    a.x = x;
    a.dz = dz;
    a.part = w.partial;
    a.dsh = w.dsh;
    a.M = B * s.hout * s.hout;
    a.N = s.cout;
    a.Ho = a.Wo = s.hout;
    a.kw = s.kw;
    a.stride = s.stride;
    if (stem) {  // the padded input: 4 channels a pixel, no tap outside the map
        a.Hi = STEM_HP, a.Wi = STEM_WP, a.Cin = 4, a.pad = 0;
    } else {
        a.Hi = a.Wi = s.hin, a.Cin = s.cin, a.pad = (s.kh - 1) / 2;
    }
    a.K = s.kh * s.kw * a.Cin;
    int slices;
    wg_slicing(idx, B, 16, &a.P, &slices);
    a.n_nt = (a.N + 63) / 64;
    const int K = s.kh * s.kw * s.cin;  // rows of dW
    const int n_kt = (a.K + 63) / 64, n_kc = (K + 3) / 4;
    if ((size_t)slices * a.K * a.N > w.partial_floats || slices > WG_MAX_SLICES || (size_t)n_kc * a.N > WG_WGP_FLOATS) return hipErrorInvalidValue;
    // the kernel loads channel and column pairs, steps two pixels with at most one row wrap, and a slice is whole groups of 16 pixels
    if (a.Wo < 2 || a.P < 16 || a.P % 16 != 0 || a.Cin % 2 != 0 || a.N % 2 != 0) return hipErrorInvalidValue;
    if (stem && (s.kh != 7 || s.cin != 3 || 2 * (s.hout - 1) + 7 > STEM_HP || 2 * (s.hout - 1) + 7 > STEM_WP)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(conv_wg_gemm_bf16_kernel, dim3(n_kt * a.n_nt, slices), dim3(64), 0, st, a);
    cmx16 w16 = stem ? w.mx_w[0] : w.mx_dxw[idx];
    const int wrow = stem ? conv_k_pad(0, true) : s.kh * s.kw * s.cout;
    hipLaunchKernelGGL(conv_wg_fixup_bf16_kernel, dim3(a.n_nt, n_kc), dim3(256), 0, st, w.partial, slices, K, a.K, a.N, w16, stem ? 1 : 0, s.cin,
                       s.kh * s.kw, wrow, bn ? c->ones : c->conv[idx].scale, grad_layer, w.wgp);
    if (bn) return hipGetLastError();
    return wg_finish(c, idx, n_kc, slices, grad_layer, st);
}

hipError_t data_grad(hpe_ctx* c, int idx, cmx16 dzs, int B, cmx16 res, mx16 out, hipStream_t st) {
    const ConvSpec& s = specs()[idx];
    GemmArgs p{};
    p.x = as_f(dzs);
    p.w = as_f(c->et.mx_dxw[idx]);
    p.scale = c->ones;
    p.shift = c->et.zeros;
    p.res = as_f(res);
    p.y = as_f(out);
    p.M = B * s.hout * s.hout;
    p.N = s.cin;
    p.K = s.kh * s.kw * s.cout;
    p.lda = s.cout;
    p.ldw = p.K;
    p.w_rows = round_up(s.cin, 128);
    p.ldy = p.ldres = s.cin;
    p.Hi = p.Wi = p.Ho = p.Wo = s.hout;
    p.Cin = s.cout;
    p.stride = 1;
    p.cin_slabs = s.cout / 64;
    p.zero = c->zeros;
    p.partial = c->partial;
    p.partial_floats = c->partial_floats;
    const int mode = s.kh == 3 ? GEMM_CONV3 : GEMM_DENSE;
    return hpe_launch_gemm_bf16(p, mode, pick_tile_bf16(c->plan, p.M, p.N, p.K, mode), st);
}

// a move of 16-byte words, whatever they hold: the fp32 launch on C / 2 floats a pixel (C % 8 == 0)
void scatter2(cmx16 lo, mx16 hi, int B, int H, int C, hipStream_t st) { scatter2(as_f(lo), as_f(hi), B, H, C / 2, st); }

void avgpool_bwd(const float* dy, mx16 dx, int B, int HW, int C, hipStream_t st) {
    hipLaunchKernelGGL(enc_avgpool_bwd_bf16_kernel, grid1((long)B * HW * (C / 8)), dim3(256), 0, st, dy, reinterpret_cast<bf16x8*>(dx), B, HW, C / 8);
}

void maxpool_bwd(cmx16 x, cmx16 dy, mx16 dx, int B, int H, int C, hipStream_t st) {
    hipLaunchKernelGGL(enc_maxpool_bwd_bf16_kernel, grid1((long)B * H * H * (C / 8)), dim3(256), 0, st, reinterpret_cast<const bf16x8*>(x),
                       reinterpret_cast<const bf16x8*>(dy), reinterpret_cast<bf16x8*>(dx), B, H, C / 8);
}
