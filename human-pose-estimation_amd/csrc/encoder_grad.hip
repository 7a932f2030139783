// encoder_grad.hip -- the kernels of the encoder's backward (encoder_train.hip holds the walks and states the mathematics) and their launchers.
//
// conv_wg_gemm_kernel: G[k][n] = sum_m A[m][k] dz[m][n] on v_mfma_f32_32x32x2_f32.  For a fixed pixel m both A[m][.] (channels of one tap,
// NHWC) and dz[m][.] are contiguous, so every lane reads its operand straight from global memory in one coalesced dword load per pixel --
// no LDS, no transposed copy.  One wave per workgroup owns a 64 x 64 tile of G (four accumulators: two A and two B loads feed four MFMAs)
// over one slice of the pixel axis; the grid is (tile, slice), so a 64 x 64 output over B * 56 * 56 pixels still fills the device.  Each
// slice writes its partial tile; conv_wg_fixup_kernel adds the slices in ascending order, writes dW and the per-64-row partial sums of
// <W, G>; conv_wg_finish_kernel adds those and the per-slice column sums of dz in ascending order.  No atomics anywhere: the same inputs
// give the same bits.  Rows past M, taps outside the map and columns past K / N are masked to zero and never read.
// The launchers here take float tensors; encoder_grad_bf16.hip holds their overloads on bf16 ones, and shares wg_slicing and wg_finish.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "hpe_ctx.h"

namespace {

struct WgArgs {
    const float* x;   // the layer's input, NHWC [B][Hi][Wi][Cin]
    const float* dz;  // [M][N]
    float* part;      // [slices][K][N]
    float* dsh;       // [slices][N] column sums of dz
    int M, K, N;
    int Hi, Wi, Cin, Ho, Wo, kw, stride, pad;
    int P;     // pixels per slice, a multiple of 8
    int n_nt;  // tiles along N
};

__global__ __launch_bounds__(64) void conv_wg_gemm_kernel(WgArgs a) {
    const int lane = threadIdx.x, hi = lane >> 5, l31 = lane & 31;
    const int kt = blockIdx.x / a.n_nt, nt = blockIdx.x - kt * a.n_nt, slice = blockIdx.y;
    const int k0 = kt * 64, n0 = nt * 64;
    // lane l feeds A[row = l & 31][k = l >> 5] and B[k = l >> 5][col = l & 31]: pixel m + hi of x and of dz
    int kh[2], kwi[2];
    long koff[2];
    bool kok[2], nok[2];
    int col[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int k = k0 + 32 * i + l31;
        kok[i] = k < a.K;
        const int tap = k / a.Cin, c = k - tap * a.Cin;
        kh[i] = tap / a.kw;
        kwi[i] = tap - kh[i] * a.kw;
        koff[i] = ((long)kh[i] * a.Wi + kwi[i]) * a.Cin + c;
        col[i] = n0 + 32 * i + l31;
        nok[i] = col[i] < a.N;
    }
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
    for (int it = 0; it < a.P; it += 8) {  // four steps of two pixels, all 16 loads issued before the first MFMA
        float av[4][2], bv[4][2];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const bool live = m < m_end;
            const int h0 = ho * a.stride - a.pad, w0 = wo * a.stride - a.pad;
            const long base = (((long)b * a.Hi + h0) * a.Wi + w0) * a.Cin;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const bool in = live && kok[i] && (unsigned)(h0 + kh[i]) < (unsigned)a.Hi && (unsigned)(w0 + kwi[i]) < (unsigned)a.Wi;
                av[u][i] = in ? a.x[base + koff[i]] : 0.f;
                bv[u][i] = (live && nok[i]) ? a.dz[(long)m * a.N + col[i]] : 0.f;
            }
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
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u][i], bv[u][j], acc[i][j], 0, 0, 0);
            bs[0] += bv[u][0];
            bs[1] += bv[u][1];
        }
    }
    // accumulator element e of lane l: row (e & 3) + 8 (e >> 2) + 4 (l >> 5), column l & 31
    float* part = a.part + (size_t)slice * a.K * a.N;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (!nok[j]) continue;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = k0 + 32 * i + (e & 3) + 8 * (e >> 2) + 4 * hi;
                if (row < a.K) part[(size_t)row * a.N + col[j]] = acc[i][j][e];
            }
        }
    if (kt == 0) {  // workgroup-uniform: the first tile row also owns the column sums of dz (even + odd pixels)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const float other = __shfl_xor(bs[j], 32, 64);
            if (hi == 0 && nok[j]) a.dsh[(size_t)slice * a.N + col[j]] = bs[j] + other;
        }
    }
}

// G = sum over the slices (ascending, four loads in flight); dW = s * G; wgp[kc][n] = sum over the 4 rows of chunk kc of W * G (row
// 0 + 1 + 2 + 3).  One thread per element of G: grid (N / 64, K / 4) rounded up, 256 threads = 64 columns x 4 rows
__global__ __launch_bounds__(256) void conv_wg_fixup_kernel(const float* __restrict__ part, int slices, int K, int N, const float* __restrict__ W,
                                                            const float* __restrict__ s, float* __restrict__ dW, float* __restrict__ wgp) {
    __shared__ float red[4][64];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int n = blockIdx.x * 64 + tx, k = blockIdx.y * 4 + ty;
    float acc = 0.f;
    if (n < N && k < K) {
        const size_t o = (size_t)k * N + n, kn = (size_t)K * N;
        float g = 0.f;
        int sl = 0;
        for (; sl + 4 <= slices; sl += 4) {
            const float p0 = part[(size_t)sl * kn + o], p1 = part[(size_t)(sl + 1) * kn + o], p2 = part[(size_t)(sl + 2) * kn + o],
                        p3 = part[(size_t)(sl + 3) * kn + o];
            g = (((g + p0) + p1) + p2) + p3;
        }
        for (; sl < slices; ++sl) g += part[(size_t)sl * kn + o];
        dW[o] = s[n] * g;
        acc = W[o] * g;
    }
    red[ty][tx] = acc;
    __syncthreads();
    if (ty == 0 && n < N) wgp[(size_t)blockIdx.y * N + n] = ((red[0][tx] + red[1][tx]) + red[2][tx]) + red[3][tx];
}

// <W, G> = sum over the kc chunks, dshift = sum over the slices: four interleaved partial sums per column, each ascending, then
// 0 + 1 + 2 + 3.  grid N / 64 rounded up, 256 threads = 64 columns x 4 groups
__global__ __launch_bounds__(256) void conv_wg_finish_kernel(const float* __restrict__ wgp, int kc, const float* __restrict__ dsh, int slices, int N,
                                                             const float* __restrict__ bias, const float* __restrict__ mean,
                                                             const float* __restrict__ istd, const float* __restrict__ s, float* __restrict__ db,
                                                             float* __restrict__ dgamma, float* __restrict__ dbeta) {
    __shared__ float rw[4][64], rd[4][64];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int n = blockIdx.x * 64 + tx;
    float wg = 0.f, d = 0.f;
    if (n < N) {
        for (int i = ty; i < kc; i += 4) wg += wgp[(size_t)i * N + n];
        for (int i = ty; i < slices; i += 4) d += dsh[(size_t)i * N + n];
    }
    rw[ty][tx] = wg;
    rd[ty][tx] = d;
    __syncthreads();
    if (ty != 0 || n >= N) return;
    wg = ((rw[0][tx] + rw[1][tx]) + rw[2][tx]) + rw[3][tx];
    d = ((rd[0][tx] + rd[1][tx]) + rd[2][tx]) + rd[3][tx];
    dbeta[n] = d;
    db[n] = s[n] * d;
    dgamma[n] = (wg + (bias[n] - mean[n]) * d) * istd[n];
}

// dz = dy * [y > 0] (y == nullptr: no activation, dz = dy); dzs = dz * s[n].  dz / dzs may be nullptr; dz may alias dy.  n4 quads, N % 4 == 0
__global__ __launch_bounds__(256) void enc_gate_kernel(const f32x4* dy, const f32x4* __restrict__ y, const float* __restrict__ s, f32x4* dz,
                                                       f32x4* __restrict__ dzs, long n4, int N4) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    f32x4 v = dy[i];
    if (y) {
        const f32x4 a = y[i];
        v.x = a.x > 0.f ? v.x : 0.f;
        v.y = a.y > 0.f ? v.y : 0.f;
        v.z = a.z > 0.f ? v.z : 0.f;
        v.w = a.w > 0.f ? v.w : 0.f;
    }
    if (dz) dz[i] = v;
    if (dzs) dzs[i] = v * reinterpret_cast<const f32x4*>(s)[i % N4];
}

// lo [B][H][H][C] -> hi [B][2H][2H][C]: the even pixels, zero elsewhere (the data gradient of a 1x1 / stride 2 convolution)
__global__ __launch_bounds__(256) void enc_scatter2_kernel(const f32x4* __restrict__ lo, f32x4* __restrict__ hi, int B, int H, int C4) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)B * 4 * H * H * C4) return;
    const int c = (int)(i % C4);
    long r = i / C4;
    const int w = (int)(r % (2 * H));
    r /= 2 * H;
    const int h = (int)(r % (2 * H)), b = (int)(r / (2 * H));
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (!(h & 1) && !(w & 1)) v = lo[(((long)b * H + (h >> 1)) * H + (w >> 1)) * C4 + c];
    hi[i] = v;
}

// dx [B][HW][C] = dy [B][C] / HW
__global__ __launch_bounds__(256) void enc_avgpool_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx, int B, int HW, int C) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)B * HW * C) return;
    const int c = (int)(i % C), b = (int)(i / ((long)HW * C));
    dx[i] = dy[(long)b * C + c] / (float)HW;
}

// MaxPooling2D(3, 2) over the zero-padded map: every cotangent goes to the first maximum of its window in row-major order, the pad
// (value 0) taking part.  Gather form, no atomics: each input pixel looks at the (up to four) windows that hold it, in row-major order.
__global__ __launch_bounds__(256) void enc_maxpool_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ dx, int B,
                                                              int H, int C) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)B * H * H * C) return;
    const int Ho = H / 2;
    const int c = (int)(i % C);
    long r = i / C;
    const int w = (int)(r % H);
    r /= H;
    const int h = (int)(r % H), b = (int)(r / H);
    float g = 0.f;
    for (int ho = h / 2; ho <= (h + 1) / 2; ++ho) {
        if (ho >= Ho) continue;
        for (int wo = w / 2; wo <= (w + 1) / 2; ++wo) {
            if (wo >= Ho) continue;
            float best = 0.f;
            int by = -2, bx = -2;
            for (int dy_ = 0; dy_ < 3; ++dy_)
                for (int dx_ = 0; dx_ < 3; ++dx_) {
                    const int yy = 2 * ho - 1 + dy_, xx = 2 * wo - 1 + dx_;
                    const bool in = (unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)H;
                    const float v = in ? x[(((long)b * H + yy) * H + xx) * C + c] : 0.f;
                    if ((dy_ == 0 && dx_ == 0) || v > best) {
                        best = v;
                        by = in ? yy : -2;
                        bx = xx;
                    }
                }
            if (by == h && bx == w) g += dy[(((long)b * Ho + ho) * Ho + wo) * C + c];
        }
    }
    dx[i] = g;
}

// the slice count of layer idx at batch B before the pixels per slice are rounded: about 2048 single-wave workgroups on the device, at
// least 256 pixels a slice
int wg_slices_unrounded(int idx, int B) {
    const ConvSpec& s = specs()[idx];
    const int K = s.kh * s.kw * s.cin, M = B * s.hout * s.hout;
    const int tiles = ((K + 63) / 64) * ((s.cout + 63) / 64);
    return std::min(std::min((M + 255) / 256, std::max(1, 2048 / tiles)), WG_MAX_SLICES);
}

}  // namespace

// a slice is whole groups of `group` pixels: 8 for conv_wg_gemm_kernel, 16 for conv_wg_gemm_bf16_kernel (encoder_grad_bf16.hip)
void wg_slicing(int idx, int B, int group, int* P, int* slices) {
    const int M = B * specs()[idx].hout * specs()[idx].hout, sl = wg_slices_unrounded(idx, B);
    *P = round_up((M + sl - 1) / sl, group);
    *slices = (M + *P - 1) / *P;
}

// sized from the slice count before P is rounded to whole groups, which is monotone in the batch and never below the count wg_slicing
// ends with (the rounded count is not monotone in the batch: a larger P can leave fewer slices)
size_t wg_partial_floats(int B) {
    size_t need = 0;
    for (int i = 0; i < HPE_NUM_CONV; ++i) {
        const ConvSpec& s = specs()[i];
        need = std::max(need, (size_t)wg_slices_unrounded(i, B) * s.kh * s.kw * s.cin * s.cout);
    }
    return need;
}

void gate(const float* dy, const float* y, const float* s, float* dz, float* dzs, long n, int N, hipStream_t st) {
    hipLaunchKernelGGL(enc_gate_kernel, grid1(n / 4), dim3(256), 0, st, reinterpret_cast<const f32x4*>(dy), reinterpret_cast<const f32x4*>(y), s,
                       reinterpret_cast<f32x4*>(dz), reinterpret_cast<f32x4*>(dzs), n / 4, N / 4);
}

hipError_t weight_grad(hpe_ctx* c, int idx, const float* x, const float* dz, int B, float* grad_layer, hipStream_t st, bool bn) {
    const ConvSpec& s = specs()[idx];
    EncTrainWork& w = c->et;
    const EncLayout& l = layout();
    WgArgs a{};
    a.x = x;
    a.dz = dz;
    a.part = w.partial;
    a.dsh = w.dsh;
    a.M = B * s.hout * s.hout;
    a.K = s.kh * s.kw * s.cin;
    a.N = s.cout;
    a.Hi = a.Wi = s.hin;
    a.Cin = s.cin;
    a.Ho = a.Wo = s.hout;
    a.kw = s.kw;
    a.stride = s.stride;
    a.pad = (s.kh - 1) / 2;
    int slices;
    wg_slicing(idx, B, 8, &a.P, &slices);
    a.n_nt = (a.N + 63) / 64;
    const int n_kt = (a.K + 63) / 64, n_kc = (a.K + 3) / 4;
    if ((size_t)slices * a.K * a.N > w.partial_floats || slices > WG_MAX_SLICES || (size_t)n_kc * a.N > WG_WGP_FLOATS) return hipErrorInvalidValue;
    // the kernel's pixel walk steps two pixels with at most one row wrap, and a slice is whole groups of eight pixels
    if (a.Wo < 2 || a.P < 8 || a.P % 8 != 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(conv_wg_gemm_kernel, dim3(n_kt * a.n_nt, slices), dim3(64), 0, st, a);
    const float* flat = w.flat;
    const int kn = a.K * a.N;
    hipLaunchKernelGGL(conv_wg_fixup_kernel, dim3(a.n_nt, n_kc), dim3(256), 0, st, w.partial, slices, a.K, a.N, flat + l.off[idx][0],
                       bn ? c->ones : c->conv[idx].scale, grad_layer, w.wgp);
    if (bn) return hipGetLastError();
    return wg_finish(c, idx, n_kc, slices, grad_layer, st);
}

hipError_t wg_finish(hpe_ctx* c, int idx, int n_kc, int slices, float* grad_layer, hipStream_t st) {
    const ConvSpec& s = specs()[idx];
    EncTrainWork& w = c->et;
    const EncLayout& l = layout();
    const int N = s.cout, kn = s.kh * s.kw * s.cin * N;
    hipLaunchKernelGGL(conv_wg_finish_kernel, dim3((N + 63) / 64), dim3(256), 0, st, w.wgp, n_kc, w.dsh, slices, N, w.flat + l.off[idx][1],
                       w.mean + l.stat[idx], w.istd + l.stat[idx], c->conv[idx].scale, grad_layer + kn, grad_layer + kn + N, grad_layer + kn + 2 * N);
    return hipGetLastError();
}

hipError_t data_grad(hpe_ctx* c, int idx, const float* dzs, int B, const float* res, float* out, hipStream_t st) {
    const ConvSpec& s = specs()[idx];
    GemmArgs p{};
    p.x = dzs;
    p.w = c->et.dxw[idx];
    p.scale = c->ones;
    p.shift = c->et.zeros;
    p.res = res;
    p.y = out;
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
    p.cin_slabs = s.cout / 32;
    p.zero = c->zeros;
    p.partial = c->partial;
    p.partial_floats = c->partial_floats;
    return hpe_launch_gemm(p, s.kh == 3 ? GEMM_CONV3 : GEMM_DENSE, pick_tile(c->plan, p.M, p.N, p.K), c->plan.splitk_min_slabs, st);
}

void scatter2(const float* lo, float* hi, int B, int H, int C, hipStream_t st) {
    hipLaunchKernelGGL(enc_scatter2_kernel, grid1((long)B * 4 * H * H * (C / 4)), dim3(256), 0, st, reinterpret_cast<const f32x4*>(lo),
                       reinterpret_cast<f32x4*>(hi), B, H, C / 4);
}

void avgpool_bwd(const float* dy, float* dx, int B, int HW, int C, hipStream_t st) {
    hipLaunchKernelGGL(enc_avgpool_bwd_kernel, grid1((long)B * HW * C), dim3(256), 0, st, dy, dx, B, HW, C);
}

void maxpool_bwd(const float* x, const float* dy, float* dx, int B, int H, int C, hipStream_t st) {
    hipLaunchKernelGGL(enc_maxpool_bwd_kernel, grid1((long)B * H * H * C), dim3(256), 0, st, x, dy, dx, B, H, C);
}
