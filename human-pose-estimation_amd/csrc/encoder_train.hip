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
// conv_wg_gemm_kernel: G[k][n] = sum_m A[m][k] dz[m][n] on v_mfma_f32_32x32x2_f32.  For a fixed pixel m both A[m][.] (channels of one tap,
// NHWC) and dz[m][.] are contiguous, so every lane reads its operand straight from global memory in one coalesced dword load per pixel --
// no LDS, no transposed copy.  One wave per workgroup owns a 64 x 64 tile of G (four accumulators: two A and two B loads feed four MFMAs)
// over one slice of the pixel axis; the grid is (tile, slice), so a 64 x 64 output over B * 56 * 56 pixels still fills the device.  Each
// slice writes its partial tile; conv_wg_fixup_kernel adds the slices in ascending order, writes dW and the per-64-row partial sums of
// <W, G>; conv_wg_finish_kernel adds those and the per-slice column sums of dz in ascending order.  No atomics anywhere: the same inputs
// give the same bits.  Rows past M, taps outside the map and columns past K / N are masked to zero and never read.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "hpe_ctx.h"

namespace {

constexpr int POOL_FLOATS = 56 * 56 * 64;  // the max-pooled map, per image
constexpr int MAX_SLICES = 128;            // pixel slices of one weight gradient (what the fix-up adds per element)
constexpr int WGP_FLOATS = 1152 * 512;     // <W, G> per 4-row chunk: K / 4 x N of the largest kernel (3x3, 512 -> 512)
constexpr int BIG = 802816, MID = 200704;  // the largest layer output / the largest bottleneck (and low-resolution) map, per image

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

struct Layout {
    int off[HPE_NUM_CONV][4];
    int stat[HPE_NUM_CONV];      // offset into the per-channel statistics arrays
    size_t stash[HPE_NUM_CONV];  // per-image offset of the layer's output in the stash
    size_t stash_pool, stash_per_image;
    int total, channels;
};

const Layout& layout() {
    static const Layout L = [] {
        Layout l{};
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

// pixels per slice and the slice count of layer idx at batch B: about 2048 single-wave workgroups on the device, at least 256 pixels a slice
void wg_slicing(int idx, int B, int* P, int* slices) {
    const ConvSpec& s = specs()[idx];
    const int K = s.kh * s.kw * s.cin, M = B * s.hout * s.hout;
    const int tiles = ((K + 63) / 64) * ((s.cout + 63) / 64);
    int sl = std::min((M + 255) / 256, std::max(1, 2048 / tiles));
    sl = std::min(sl, MAX_SLICES);
    *P = round_up((M + sl - 1) / sl, 8);
    *slices = (M + *P - 1) / *P;
}

// the partial buffer for every batch up to B: sized from the slice count before P is rounded to a multiple of 8, which is monotone in the
// batch and never below the count wg_slicing ends with (the rounded count is not monotone in the batch: a larger P can leave fewer slices)
size_t partial_floats(int B) {
    size_t need = 0;
    for (int i = 0; i < HPE_NUM_CONV; ++i) {
        const ConvSpec& s = specs()[i];
        const int K = s.kh * s.kw * s.cin, M = B * s.hout * s.hout;
        const int tiles = ((K + 63) / 64) * ((s.cout + 63) / 64);
        const int sl = std::min(std::min((M + 255) / 256, std::max(1, 2048 / tiles)), MAX_SLICES);
        need = std::max(need, (size_t)sl * K * s.cout);
    }
    return need;
}

size_t dxw_floats(int idx) { return conv_dxw_floats(idx); }

size_t ws_floats(int B) {
    size_t n = (size_t)B * layout().stash_per_image + (size_t)B * (3 * (size_t)BIG + 3 * (size_t)MID) + partial_floats(B);
    n += (size_t)MAX_SLICES * 2048 + (size_t)WGP_FLOATS;  // column sums of dz per slice, <W, G> per 64-row chunk
    for (int i = 0; i < HPE_NUM_CONV; ++i) n += dxw_floats(i);
    n += 2 * (size_t)layout().channels + encoder_repack_reserve_floats();  // hpe_encoder_set_params_dev: sqrt(var + eps) in double, the layer table
    return n + layout().total + 2 * layout().channels + 2048 + (size_t)B * HPE_FEATURE_DIM;
}

// the data-gradient operand of layer idx in the forward GEMM's Wt[n][k] form: rows = input channels (zero padded to 128), k = output channels
// (1x1: the HWIO matrix itself) or (tap', output channel) with the taps flipped (3x3)
void pack_dx_weights(int idx, const float* kernel, std::vector<float>& out) {
    const ConvSpec& s = specs()[idx];
    const int taps = s.kh * s.kw, K = taps * s.cout;
    out.assign(dxw_floats(idx), 0.f);
    for (int t = 0; t < taps; ++t)
        for (int ci = 0; ci < s.cin; ++ci) {
            const float* src = kernel + ((size_t)t * s.cin + ci) * s.cout;
            std::copy(src, src + s.cout, out.begin() + (size_t)ci * K + (size_t)(taps - 1 - t) * s.cout);
        }
}

void gate(const float* dy, const float* y, const float* s, float* dz, float* dzs, long n, int N, hipStream_t st) {
    hipLaunchKernelGGL(enc_gate_kernel, grid1(n / 4), dim3(256), 0, st, reinterpret_cast<const f32x4*>(dy), reinterpret_cast<const f32x4*>(y), s,
                       reinterpret_cast<f32x4*>(dz), reinterpret_cast<f32x4*>(dzs), n / 4, N / 4);
}

// the weight gradient of layer idx and what hangs on it, into grad_layer = [kernel | bias | gamma | beta]: three launches.  bn (batch
// statistics): dz is dzraw, dW = G with a unit scale, and the finish is not launched -- bias, gamma and beta come from bn_launch_bwd_reduce
hipError_t weight_grad(hpe_ctx* c, int idx, const float* x, const float* dz, int B, float* grad_layer, hipStream_t st, bool bn = false) {
    const ConvSpec& s = specs()[idx];
    EncTrainWork& w = c->et;
    const Layout& l = layout();
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
    wg_slicing(idx, B, &a.P, &slices);
    a.n_nt = (a.N + 63) / 64;
    const int n_kt = (a.K + 63) / 64, n_kc = (a.K + 3) / 4;
    if ((size_t)slices * a.K * a.N > w.partial_floats || slices > MAX_SLICES || (size_t)n_kc * a.N > WGP_FLOATS) return hipErrorInvalidValue;
    // the kernel's pixel walk steps two pixels with at most one row wrap, and a slice is whole groups of eight pixels
    if (a.Wo < 2 || a.P < 8 || a.P % 8 != 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(conv_wg_gemm_kernel, dim3(n_kt * a.n_nt, slices), dim3(64), 0, st, a);
    const float* flat = w.flat;
    const int kn = a.K * a.N;
    hipLaunchKernelGGL(conv_wg_fixup_kernel, dim3(a.n_nt, n_kc), dim3(256), 0, st, w.partial, slices, a.K, a.N, flat + l.off[idx][0],
                       bn ? c->ones : c->conv[idx].scale, grad_layer, w.wgp);
    if (bn) return hipGetLastError();
    hipLaunchKernelGGL(conv_wg_finish_kernel, dim3(a.n_nt), dim3(256), 0, st, w.wgp, n_kc, w.dsh, slices, a.N, flat + l.off[idx][1],
                       w.mean + l.stat[idx], w.istd + l.stat[idx], c->conv[idx].scale, grad_layer + kn, grad_layer + kn + a.N,
                       grad_layer + kn + 2 * a.N);
    return hipGetLastError();
}

// out [M][cin] = dzs [M][cout] . W^T (+ res) on the map of the layer's OUTPUT (a stride-2 layer: the low-resolution map)
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

float* stash_of(hpe_ctx* c, int idx, int B) {
    const Layout& l = layout();
    return c->et.stash + (size_t)B * (idx < 0 ? l.stash_pool : l.stash[idx]);
}

hipError_t forward_train(hpe_ctx* c, const float* images, int B, float* features, hipStream_t st) {
    HIPE(hpe_launch_pad_input(images, c->padded, B, HPE_IMG_SIZE, HPE_IMG_SIZE, STEM_HP, STEM_WP, st));
    HIPE(run_conv_nhwc(c, 0, c->padded, B, nullptr, 1, stash_of(c, 0, B), st));
    HIPE(hpe_launch_maxpool(stash_of(c, 0, B), stash_of(c, -1, B), B, 112, 64, st));
    for (const ResBlock& blk : blocks()) {
        const float* cur = stash_of(c, blk.in, B);
        HIPE(run_conv_nhwc(c, blk.i2a, cur, B, nullptr, 1, stash_of(c, blk.i2a, B), st));
        HIPE(run_conv_nhwc(c, blk.i2b, stash_of(c, blk.i2a, B), B, nullptr, 1, stash_of(c, blk.i2b, B), st));
        const float* res = cur;
        if (blk.first) {
            HIPE(run_conv_nhwc(c, blk.i1, cur, B, nullptr, 0, stash_of(c, blk.i1, B), st));
            res = stash_of(c, blk.i1, B);
        }
        HIPE(run_conv_nhwc(c, blk.i2c, stash_of(c, blk.i2b, B), B, res, 1, stash_of(c, blk.i2c, B), st));
    }
    return hpe_launch_avgpool(stash_of(c, blocks().back().i2c, B), features, B, 49, HPE_FEATURE_DIM, HPE_FEATURE_DIM, st);
}

hipError_t backward(hpe_ctx* c, const float* images, int B, const float* grad_features, float* grad_flat, hipStream_t st) {
    EncTrainWork& w = c->et;
    const Layout& l = layout();
    HIPE(forward_train(c, images, B, w.feat, st));
    float *g = w.g0, *go = w.g1;
    hipLaunchKernelGGL(enc_avgpool_bwd_kernel, grid1((long)B * 49 * HPE_FEATURE_DIM), dim3(256), 0, st, grad_features, g, B, 49, HPE_FEATURE_DIM);
    for (auto it = blocks().rbegin(); it != blocks().rend(); ++it) {
        const int i2a = it->i2a, i2b = it->i2b, i2c = it->i2c, i1 = it->i1;
        const bool first = it->first;
        const ConvSpec &sa = specs()[i2a], &sb = specs()[i2b], &sc = specs()[i2c];
        const float* xin = stash_of(c, it->in, B);  // the block's input: the previous block's branch2c output
        const long Mo = (long)B * sc.hout * sc.hout;
        // branch2c: g becomes dz (the cotangent of the shortcut too)
        gate(g, stash_of(c, i2c, B), c->conv[i2c].scale, g, w.sbig, Mo * sc.cout, sc.cout, st);
        HIPE(weight_grad(c, i2c, stash_of(c, i2b, B), g, B, grad_flat + l.off[i2c][0], st));
        HIPE(data_grad(c, i2c, w.sbig, B, nullptr, w.t0, st));
        gate(w.t0, stash_of(c, i2b, B), c->conv[i2b].scale, w.t0, w.ssmall, Mo * sb.cout, sb.cout, st);
        HIPE(weight_grad(c, i2b, stash_of(c, i2a, B), w.t0, B, grad_flat + l.off[i2b][0], st));
        HIPE(data_grad(c, i2b, w.ssmall, B, nullptr, w.t1, st));
        gate(w.t1, stash_of(c, i2a, B), c->conv[i2a].scale, w.t1, w.ssmall, Mo * sa.cout, sa.cout, st);
        HIPE(weight_grad(c, i2a, xin, w.t1, B, grad_flat + l.off[i2a][0], st));
        if (!first) {
            HIPE(data_grad(c, i2a, w.ssmall, B, g, go, st));
            std::swap(g, go);
            continue;
        }
        // projection shortcut: no activation of its own, its dz is the block's
        gate(g, nullptr, c->conv[i1].scale, nullptr, w.sbig, Mo * sc.cout, sc.cout, st);
        HIPE(weight_grad(c, i1, xin, g, B, grad_flat + l.off[i1][0], st));
        if (sa.stride == 1) {
            HIPE(data_grad(c, i2a, w.ssmall, B, nullptr, go, st));
            HIPE(data_grad(c, i1, w.sbig, B, go, g, st));
        } else {
            HIPE(data_grad(c, i2a, w.ssmall, B, nullptr, w.t0, st));
            HIPE(data_grad(c, i1, w.sbig, B, w.t0, w.t1, st));
            scatter2(w.t1, go, B, sa.hout, sa.cin, st);
            std::swap(g, go);
        }
    }
    hipLaunchKernelGGL(enc_maxpool_bwd_kernel, grid1((long)B * 112 * 112 * 64), dim3(256), 0, st, stash_of(c, 0, B), g, go, B, 112, 64);
    gate(go, stash_of(c, 0, B), nullptr, go, nullptr, (long)B * BIG, 64, st);
    return weight_grad(c, 0, images, go, B, grad_flat + l.off[0][0], st);
}

// ---- BatchNorm with batch statistics (encoder_bn.hip holds the kernels): the same walks with z kept beside y

float* zstash_of(hpe_ctx* c, int idx, int B) { return c->et.zstash + (size_t)B * layout().stash[idx]; }

struct BnSlots {
    float *mu, *var, *r;
};

// layer idx's slots of the batch statistics; scratch: the three 2048-float slots behind them, for the one-layer debug calls
BnSlots bn_slots(hpe_ctx* c, int idx, bool scratch) {
    const Layout& l = layout();
    float* b = c->et.bn_batch;
    if (scratch) return {b + 3 * l.channels, b + 3 * l.channels + 2048, b + 3 * l.channels + 4096};
    return {b + l.stat[idx], b + l.channels + l.stat[idx], b + 2 * l.channels + l.stat[idx]};
}

// z = conv(x, W) + b (the layer's own route, unit scale, the bias of the flat copy as shift), its statistics, y = act(BN(z) (+ res))
hipError_t layer_forward_bn(hpe_ctx* c, int idx, const float* x, int B, const float* res, int relu, float* z, float* y, const BnSlots& s, hipStream_t st) {
    const ConvSpec& sp = specs()[idx];
    const Layout& l = layout();
    const float* flat = c->et.flat;
    const int M = B * sp.hout * sp.hout;
    HIPE(run_conv_nhwc(c, idx, x, B, nullptr, 0, z, st, c->ones, flat + l.off[idx][1]));
    HIPE(bn_launch_stats(z, M, sp.cout, c->cfg.bn_eps, c->et.bn_part, s.mu, s.var, s.r, st));
    return bn_launch_apply(z, s.mu, s.r, flat + l.off[idx][2], flat + l.off[idx][3], res, relu, y, M, sp.cout, st);
}

// the gate and the BatchNorm backward of layer idx: db (= 0), dgamma, dbeta into grad_layer; dz (may be nullptr, may alias dy) and dzraw
hipError_t layer_gate_bn(hpe_ctx* c, int idx, const float* dy, const float* y, const float* z, int B, const BnSlots& s, float* grad_layer, float* dz,
                         float* dzraw, hipStream_t st) {
    const ConvSpec& sp = specs()[idx];
    const int M = B * sp.hout * sp.hout, N = sp.cout, kn = sp.kh * sp.kw * sp.cin * N;
    float *db = grad_layer + kn, *dgamma = db + N, *dbeta = dgamma + N;
    HIPE(bn_launch_bwd_reduce(dy, y, z, s.mu, s.r, M, N, c->et.bn_part, db, dgamma, dbeta, st));
    return bn_launch_bwd_apply(dy, y, z, s.mu, s.r, c->et.flat + layout().off[idx][2], dgamma, dbeta, M, N, dz, dzraw, st);
}

hipError_t forward_bn(hpe_ctx* c, const float* images, int B, float* features, hipStream_t st) {
    auto layer = [&](int idx, const float* x, const float* res, int relu) {
        return layer_forward_bn(c, idx, x, B, res, relu, zstash_of(c, idx, B), stash_of(c, idx, B), bn_slots(c, idx, false), st);
    };
    HIPE(hpe_launch_pad_input(images, c->padded, B, HPE_IMG_SIZE, HPE_IMG_SIZE, STEM_HP, STEM_WP, st));
    HIPE(layer(0, c->padded, nullptr, 1));
    HIPE(hpe_launch_maxpool(stash_of(c, 0, B), stash_of(c, -1, B), B, 112, 64, st));
    for (const ResBlock& blk : blocks()) {
        const float* cur = stash_of(c, blk.in, B);
        HIPE(layer(blk.i2a, cur, nullptr, 1));
        HIPE(layer(blk.i2b, stash_of(c, blk.i2a, B), nullptr, 1));
        const float* res = cur;
        if (blk.first) {
            HIPE(layer(blk.i1, cur, nullptr, 0));
            res = stash_of(c, blk.i1, B);
        }
        HIPE(layer(blk.i2c, stash_of(c, blk.i2b, B), res, 1));
    }
    return hpe_launch_avgpool(stash_of(c, blocks().back().i2c, B), features, B, 49, HPE_FEATURE_DIM, HPE_FEATURE_DIM, st);
}

hipError_t backward_bn(hpe_ctx* c, const float* images, int B, const float* grad_features, float* grad_flat, hipStream_t st) {
    EncTrainWork& w = c->et;
    const Layout& l = layout();
    HIPE(forward_bn(c, images, B, w.feat, st));
    // dy -> layer idx's bias / gamma / beta gradients, dz (nullptr: not kept) and dzraw
    auto gate_bn = [&](int idx, const float* dy, bool gated, float* dz, float* dzraw) {
        return layer_gate_bn(c, idx, dy, gated ? stash_of(c, idx, B) : nullptr, zstash_of(c, idx, B), B, bn_slots(c, idx, false),
                             grad_flat + l.off[idx][0], dz, dzraw, st);
    };
    auto wgrad = [&](int idx, const float* x, const float* dzraw) { return weight_grad(c, idx, x, dzraw, B, grad_flat + l.off[idx][0], st, true); };
    float *g = w.g0, *go = w.g1;
    hipLaunchKernelGGL(enc_avgpool_bwd_kernel, grid1((long)B * 49 * HPE_FEATURE_DIM), dim3(256), 0, st, grad_features, g, B, 49, HPE_FEATURE_DIM);
    for (auto it = blocks().rbegin(); it != blocks().rend(); ++it) {
        const int i2a = it->i2a, i2b = it->i2b, i2c = it->i2c, i1 = it->i1;
        const ConvSpec& sa = specs()[i2a];
        const float* xin = stash_of(c, it->in, B);
        // branch2c: g becomes dz (the cotangent of the shortcut too)
        HIPE(gate_bn(i2c, g, true, g, w.sbig));
        HIPE(wgrad(i2c, stash_of(c, i2b, B), w.sbig));
        HIPE(data_grad(c, i2c, w.sbig, B, nullptr, w.t0, st));
        HIPE(gate_bn(i2b, w.t0, true, nullptr, w.ssmall));
        HIPE(wgrad(i2b, stash_of(c, i2a, B), w.ssmall));
        HIPE(data_grad(c, i2b, w.ssmall, B, nullptr, w.t1, st));
        HIPE(gate_bn(i2a, w.t1, true, nullptr, w.ssmall));
        HIPE(wgrad(i2a, xin, w.ssmall));
        if (!it->first) {
            HIPE(data_grad(c, i2a, w.ssmall, B, g, go, st));
            std::swap(g, go);
            continue;
        }
        // projection shortcut: no activation of its own, its dz is the block's
        HIPE(gate_bn(i1, g, false, nullptr, w.sbig));
        HIPE(wgrad(i1, xin, w.sbig));
        if (sa.stride == 1) {
            HIPE(data_grad(c, i2a, w.ssmall, B, nullptr, go, st));
            HIPE(data_grad(c, i1, w.sbig, B, go, g, st));
        } else {
            HIPE(data_grad(c, i2a, w.ssmall, B, nullptr, w.t0, st));
            HIPE(data_grad(c, i1, w.sbig, B, w.t0, w.t1, st));
            scatter2(w.t1, go, B, sa.hout, sa.cin, st);
            std::swap(g, go);
        }
    }
    hipLaunchKernelGGL(enc_maxpool_bwd_kernel, grid1((long)B * 112 * 112 * 64), dim3(256), 0, st, stash_of(c, 0, B), g, go, B, 112, 64);
    HIPE(gate_bn(0, go, true, nullptr, w.sbig));
    return wgrad(0, images, w.sbig);
}

size_t bn_batch_floats() { return 3 * (size_t)layout().channels + 3 * 2048; }

size_t ws_floats_bn(int B) {
    return (size_t)B * layout().stash_pool + bn_batch_floats() + 2 * (size_t)layout().channels + 4 * (size_t)BN_PART_COLS + layout().channels;
}

int check_train(hpe_ctx* c, int B, bool need_reserve = true) {
    if (!c) return fail(HPE_ERR_INVALID, "null ctx");
    if (c->dead) return fail(HPE_ERR_STATE, "hpe_finalize failed on this ctx: destroy it and create a new one");
    if (!c->finalized) return fail(HPE_ERR_STATE, "hpe_finalize() has not been called");
    if (!c->have_encoder) return fail(HPE_ERR_STATE, "encoder weights were not loaded before hpe_finalize");
    if (c->bf16) return fail(HPE_ERR_STATE, "encoder training needs an fp32 context");
    if (need_reserve && c->et.B == 0) return fail(HPE_ERR_STATE, "hpe_encoder_train_reserve() has not been called");
    if (B < 1 || B > (need_reserve ? c->et.B : c->cfg.max_batch))
        return fail(HPE_ERR_INVALID, "batch " + std::to_string(B) + (need_reserve ? " outside [1, reserved batch]" : " outside [1, max_batch]"));
    return HPE_OK;
}

// ... and for the calls that need hpe_encoder_train_reserve_batchnorm
int check_train_bn(hpe_ctx* c, int B) {
    int rc = check_train(c, 1);
    if (rc) return rc;
    if (c->et.bn_B == 0) return fail(HPE_ERR_STATE, "hpe_encoder_train_reserve_batchnorm() has not been called");
    if (B < 1 || B > c->et.bn_B) return fail(HPE_ERR_INVALID, "batch " + std::to_string(B) + " outside [1, batch of the batch-norm reserve]");
    return HPE_OK;
}

// host flat -> the data-gradient packings and the flat device copy (buffers exist)
int upload_train_params(hpe_ctx* c, const float* flat) {
    const Layout& l = layout();
    std::vector<float> dx;
    for (int i = 1; i < HPE_NUM_CONV; ++i) {
        pack_dx_weights(i, flat + l.off[i][0], dx);
        HIP_TRY(hipMemcpy(c->et.dxw[i], dx.data(), dx.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    HIP_TRY(hipMemcpy(c->et.flat, flat, (size_t)l.total * sizeof(float), hipMemcpyHostToDevice));
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

long long hpe_encoder_train_ws_floats(int B) { return B < 1 ? 0 : (long long)ws_floats(B); }

int hpe_encoder_wg_slices(int idx, int B) {
    if (idx < 0 || idx >= HPE_NUM_CONV || B < 1) return -1;
    int P, sl;
    wg_slicing(idx, B, &P, &sl);
    return sl;
}

int hpe_encoder_train_reserve(hpe_ctx* c, int B) {
    int rc = check_train(c, B, false);
    if (rc) return rc;
    EncTrainWork& w = c->et;
    if (w.B != 0) return B <= w.B ? HPE_OK : fail(HPE_ERR_STATE, "hpe_encoder_train_reserve: already reserved for a smaller batch");
    DeviceGuard g(c->cfg.device);
    const Layout& l = layout();
    const size_t nb = (size_t)B;
    if ((rc = dev_alloc(c, &w.stash, nb * l.stash_per_image, false))) return rc;
    if ((rc = dev_alloc(c, &w.g0, nb * BIG, false))) return rc;
    if ((rc = dev_alloc(c, &w.g1, nb * BIG, false))) return rc;
    if ((rc = dev_alloc(c, &w.sbig, nb * BIG, false))) return rc;
    if ((rc = dev_alloc(c, &w.t0, nb * MID, false))) return rc;
    if ((rc = dev_alloc(c, &w.t1, nb * MID, false))) return rc;
    if ((rc = dev_alloc(c, &w.ssmall, nb * MID, false))) return rc;
    w.partial_floats = partial_floats(B);
    if ((rc = dev_alloc(c, &w.partial, w.partial_floats, false))) return rc;
    if ((rc = dev_alloc(c, &w.dsh, (size_t)MAX_SLICES * 2048, false))) return rc;
    if ((rc = dev_alloc(c, &w.wgp, (size_t)WGP_FLOATS, false))) return rc;
    if ((rc = dev_alloc(c, &w.zeros, 2048, true))) return rc;
    if ((rc = dev_alloc(c, &w.feat, nb * HPE_FEATURE_DIM, false))) return rc;
    if ((rc = dev_alloc(c, &w.flat, l.total, false))) return rc;
    if ((rc = dev_alloc(c, &w.mean, l.channels, false))) return rc;
    if ((rc = dev_alloc(c, &w.istd, l.channels, false))) return rc;
    float* sdp = nullptr;
    if ((rc = dev_alloc(c, &sdp, 2 * (size_t)l.channels, false))) return rc;
    w.sd = reinterpret_cast<double*>(sdp);
    for (int i = 1; i < HPE_NUM_CONV; ++i)
        if ((rc = dev_alloc(c, &w.dxw[i], dxw_floats(i), false))) return rc;
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
    int rc = check_train(c, B);
    if (rc) return rc;
    if (!images || !features) return fail(HPE_ERR_INVALID, "null pointer");
    DeviceGuard g(c->cfg.device);
    HIP_TRY(forward_train(c, images, B, features, static_cast<hipStream_t>(stream)));
    c->et.stash_B = B;
    return HPE_OK;
}

int hpe_encoder_backward(hpe_ctx* c, const float* images, int B, const float* grad_features, float* grad_flat, void* stream) {
    int rc = check_train(c, B);
    if (rc) return rc;
    if (!images || !grad_features || !grad_flat) return fail(HPE_ERR_INVALID, "null pointer");
    DeviceGuard g(c->cfg.device);
    HIP_TRY(backward(c, images, B, grad_features, grad_flat, static_cast<hipStream_t>(stream)));
    c->et.stash_B = B;
    return HPE_OK;
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
    const Layout& l = layout();
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
    if (!dx) return HPE_OK;
    if (s.stride == 1) {
        HIP_TRY(data_grad(c, idx, w.sbig, B, nullptr, dx, st));
    } else {
        HIP_TRY(data_grad(c, idx, w.sbig, B, nullptr, w.t0, st));
        scatter2(w.t0, dx, B, s.hout, s.cin, st);
        HIP_TRY(hipGetLastError());
    }
    return HPE_OK;
}

int hpe_debug_maxpool_backward(const float* x, const float* dy, int B, int H, int C, float* dx, void* stream) {
    if (!x || !dy || !dx || B < 1 || H < 2 || (H & 1) || C < 1) return fail(HPE_ERR_INVALID, "bad argument");
    hipLaunchKernelGGL(enc_maxpool_bwd_kernel, grid1((long)B * H * H * C), dim3(256), 0, static_cast<hipStream_t>(stream), x, dy, dx, B, H, C);
    HIP_TRY(hipGetLastError());
    return HPE_OK;
}

int hpe_debug_avgpool_backward(const float* dy, int B, int HW, int C, float* dx, void* stream) {
    if (!dy || !dx || B < 1 || HW < 1 || C < 1) return fail(HPE_ERR_INVALID, "bad argument");
    hipLaunchKernelGGL(enc_avgpool_bwd_kernel, grid1((long)B * HW * C), dim3(256), 0, static_cast<hipStream_t>(stream), dy, dx, B, HW, C);
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

long long hpe_encoder_train_ws_floats_batchnorm(int B) { return B < 1 ? 0 : (long long)(ws_floats(B) + ws_floats_bn(B)); }

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
    const Layout& l = layout();
    float* p = nullptr;
    if ((rc = dev_alloc(c, &w.zstash, (size_t)B * l.stash_pool, false))) return rc;
    if ((rc = dev_alloc(c, &w.bn_batch, bn_batch_floats(), true))) return rc;
    if ((rc = dev_alloc(c, &w.bn_stats, 2 * (size_t)l.channels, false))) return rc;
    if ((rc = dev_alloc(c, &p, 4 * (size_t)BN_PART_COLS, false))) return rc;
    w.bn_part = reinterpret_cast<double*>(p);
    p = nullptr;
    if ((rc = dev_alloc(c, &p, l.channels, false))) return rc;
    w.bn_hw = reinterpret_cast<int*>(p);
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
    int rc = check_train_bn(c, B);
    if (rc) return rc;
    if (!images || !features) return fail(HPE_ERR_INVALID, "null pointer");
    DeviceGuard g(c->cfg.device);
    HIP_TRY(forward_bn(c, images, B, features, static_cast<hipStream_t>(stream)));
    c->et.stash_B = c->et.bn_stat_B = B;
    return HPE_OK;
}

int hpe_encoder_backward_batchnorm(hpe_ctx* c, const float* images, int B, const float* grad_features, float* grad_flat, void* stream) {
    int rc = check_train_bn(c, B);
    if (rc) return rc;
    if (!images || !grad_features || !grad_flat) return fail(HPE_ERR_INVALID, "null pointer");
    DeviceGuard g(c->cfg.device);
    HIP_TRY(backward_bn(c, images, B, grad_features, grad_flat, static_cast<hipStream_t>(stream)));
    c->et.stash_B = c->et.bn_stat_B = B;
    return HPE_OK;
}

int hpe_encoder_get_stats(hpe_ctx* c, float* stats, void* stream) {
    int rc = check_train_bn(c, 1);
    if (rc) return rc;
    if (!stats) return fail(HPE_ERR_INVALID, "null stats_dev");
    DeviceGuard g(c->cfg.device);
    HIP_TRY(hipMemcpyAsync(stats, c->et.bn_stats, 2 * (size_t)layout().channels * sizeof(float), hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream)));
    return HPE_OK;
}

int hpe_encoder_update_stats(hpe_ctx* c, float* stats, double momentum, int unbiased, void* stream) {
    int rc = check_train_bn(c, 1);
    if (rc) return rc;
    if (!stats) return fail(HPE_ERR_INVALID, "null stats_dev");
    if (!(momentum >= 0.0 && momentum <= 1.0)) return fail(HPE_ERR_INVALID, "momentum outside [0, 1]");
    if (c->et.bn_stat_B == 0) return fail(HPE_ERR_STATE, "hpe_encoder_update_stats: no batch-statistics forward has run");
    DeviceGuard g(c->cfg.device);
    HIP_TRY(bn_launch_momentum(stats, c->et.bn_batch, c->et.bn_hw, c->et.bn_stat_B, layout().channels, momentum, unbiased != 0,
                               static_cast<hipStream_t>(stream)));
    return HPE_OK;
}

int hpe_encoder_set_stats_dev(hpe_ctx* c, const float* stats, void* stream) {
    int rc = check_train_bn(c, 1);
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
    int rc = check_train_bn(c, B);
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
    int rc = check_train_bn(c, B);
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
    if (!dx) return HPE_OK;
    if (s.stride == 1) {
        HIP_TRY(data_grad(c, idx, w.sbig, B, nullptr, dx, st));
    } else {
        HIP_TRY(data_grad(c, idx, w.sbig, B, nullptr, w.t0, st));
        scatter2(w.t0, dx, B, s.hout, s.cin, st);
        HIP_TRY(hipGetLastError());
    }
    return HPE_OK;
}

int hpe_debug_encoder_stash_raw(hpe_ctx* c, int idx, float* out, void* stream) {
    int rc = check_train_bn(c, 1);
    if (rc) return rc;
    if (idx < 0 || idx >= HPE_NUM_CONV || !out) return fail(HPE_ERR_INVALID, "bad argument");
    const int B = c->et.bn_stat_B;
    if (B == 0) return fail(HPE_ERR_STATE, "hpe_debug_encoder_stash_raw: no batch-statistics forward has run");
    if (c->et.stash_B != B) return fail(HPE_ERR_STATE, "hpe_debug_encoder_stash_raw: a frozen-statistics forward of another batch has refilled the stash since");
    DeviceGuard g(c->cfg.device);
    const size_t n = (size_t)specs()[idx].hout * specs()[idx].hout * specs()[idx].cout;
    HIP_TRY(hipMemcpyAsync(out, zstash_of(c, idx, B), (size_t)B * n * sizeof(float), hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream)));
    return HPE_OK;
}

int hpe_debug_encoder_batch_stats(hpe_ctx* c, float* out, void* stream) {
    int rc = check_train_bn(c, 1);
    if (rc) return rc;
    if (!out) return fail(HPE_ERR_INVALID, "null out_dev");
    if (c->et.bn_stat_B == 0) return fail(HPE_ERR_STATE, "hpe_debug_encoder_batch_stats: no batch-statistics forward has run");
    DeviceGuard g(c->cfg.device);
    HIP_TRY(hipMemcpyAsync(out, c->et.bn_batch, 2 * (size_t)layout().channels * sizeof(float), hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream)));
    return HPE_OK;
}

}  // extern "C"
#pragma GCC visibility pop
