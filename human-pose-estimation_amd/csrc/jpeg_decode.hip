// jpeg_decode.hip -- the data-parallel half of the JPEG decoder (DESIGN.md "Training records and JPEG decode"): dequantisation, 8x8
// inverse DCT, chroma upsampling, colour conversion and the store, for a whole batch of mixed sizes and samplings in two launches, plus
// the C ABI of the host half (jpeg_entropy.hip).  The definition is libjpeg's default decode -- jidctint.c (JDCT_ISLOW), jdsample.c
// (fancy upsampling), jdcolor.c -- and the contract is bit-exactness, so everything is 32-bit integer arithmetic: products and sums in
// unsigned (a corrupt stream wraps), arithmetic shifts of the reinterpreted signed value.
//
// Launch one: 8 threads per block -- one per column (pass 1), then one per row (pass 2), the 8x8 transpose through LDS -- 32 blocks per
// workgroup; a row of 8 samples leaves as one 8-byte store into the component's uint8 plane in the workspace.
// Launch two: 4 adjacent output BYTES per thread, one aligned dword store; each byte is one channel of one pixel and needs Y and at
// most two upsampled chroma samples, read from the planes (L2-resident at these sizes).  A frame's last partial dword is stored byte
// by byte: nothing between the frames is written.
// Both grids are the concatenation of the images' workgroups; a workgroup finds its image by a search of the workgroup-uniform table.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "batch_table.h"
#include "hpe_ctx.h"
#include "jpeg.h"

namespace {

constexpr int JPEG_THREADS = 256;
static_assert(jpeg::IDCT_BLOCKS_PER_GROUP * 8 == JPEG_THREADS, "8 threads per block");
static_assert(jpeg::STORE_BYTES_PER_GROUP == JPEG_THREADS * 4, "4 output bytes per thread");
static_assert(sizeof(HpeJpegImage) == 304 && sizeof(HpeJpegInfo) == 72, "the table entries of include/hpe.h and jpeg.py");

typedef unsigned int u32;

// jidctint.c's 1-D kernel on in[0..7]; out[i] = (x + (1 << (SHIFT - 1))) >> SHIFT
template <int SHIFT>
__device__ __forceinline__ void idct8(const int* in, int* out) {
    const u32 i0 = (u32)in[0], i1 = (u32)in[1], i2 = (u32)in[2], i3 = (u32)in[3], i4 = (u32)in[4], i5 = (u32)in[5], i6 = (u32)in[6], i7 = (u32)in[7];
    u32 z1 = (i2 + i6) * 4433u;
    const u32 tmp2 = z1 - i6 * 15137u, tmp3 = z1 + i2 * 6270u;
    const u32 tmp0 = (i0 + i4) << 13, tmp1 = (i0 - i4) << 13;
    const u32 tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    u32 t0 = i7, t1 = i5, t2 = i3, t3 = i1;
    z1 = t0 + t3;
    u32 z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
    const u32 z5 = (z3 + z4) * 9633u;
    t0 *= 2446u;
    t1 *= 16819u;
    t2 *= 25172u;
    t3 *= 12299u;
    z1 *= (u32)-7373;
    z2 *= (u32)-20995;
    z3 = z3 * (u32)-16069 + z5;
    z4 = z4 * (u32)-3196 + z5;
    t0 += z1 + z3;
    t1 += z2 + z4;
    t2 += z2 + z3;
    t3 += z1 + z4;
    const u32 r = 1u << (SHIFT - 1);
    out[0] = (int)(tmp10 + t3 + r) >> SHIFT;
    out[7] = (int)(tmp10 - t3 + r) >> SHIFT;
    out[1] = (int)(tmp11 + t2 + r) >> SHIFT;
    out[6] = (int)(tmp11 - t2 + r) >> SHIFT;
    out[2] = (int)(tmp12 + t1 + r) >> SHIFT;
    out[5] = (int)(tmp12 - t1 + r) >> SHIFT;
    out[3] = (int)(tmp13 + t0 + r) >> SHIFT;
    out[4] = (int)(tmp13 - t0 + r) >> SHIFT;
}

__global__ __launch_bounds__(JPEG_THREADS) void jpeg_idct_kernel(const HpeJpegImage* __restrict__ table, int B, const short* __restrict__ coef,
                                                                 unsigned char* __restrict__ workspace) {
    __shared__ int ws[jpeg::IDCT_BLOCKS_PER_GROUP][8][9];  // [block][row][column], rows padded against bank conflicts in pass 2
    const int b = find_image<&HpeJpegImage::idct_group0>(table, B, (int)blockIdx.x);
    const HpeJpegImage* e = table + b;
    const int slot = threadIdx.x >> 3, j = threadIdx.x & 7;
    int k = (blockIdx.x - e->idct_group0) * jpeg::IDCT_BLOCKS_PER_GROUP + slot;  // block of the image, components back to back
    int c = 0;
    const int ncomp = e->ncomp;
    while (c < ncomp && k >= e->blocks_w[c] * e->blocks_h[c]) {
        k -= e->blocks_w[c] * e->blocks_h[c];
        ++c;
    }
    const bool active = c < ncomp;
    if (active) {  // pass 1: column j of coef * quant
        const short* src = coef + e->coef_offset[c] + (long long)k * 64;
        const unsigned char* q = e->quant[c];
        int in[8], out[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) in[r] = (int)src[r * 8 + j] * (int)q[r * 8 + j];
        idct8<11>(in, out);
#pragma unroll
        for (int r = 0; r < 8; ++r) ws[slot][r][j] = out[r];
    }
    __syncthreads();
    if (active) {  // pass 2: row j
        int in[8], out[8];
#pragma unroll
        for (int x = 0; x < 8; ++x) in[x] = ws[slot][j][x];
        idct8<18>(in, out);
        u32 lo = 0, hi = 0;
#pragma unroll
        for (int x = 0; x < 4; ++x) {
            lo |= (u32)min(max(out[x] + 128, 0), 255) << (8 * x);
            hi |= (u32)min(max(out[x + 4] + 128, 0), 255) << (8 * x);
        }
        const int bw = e->blocks_w[c], by = k / bw, bx = k - by * bw;
        unsigned char* dst = workspace + e->plane_offset[c] + ((long long)(by * 8 + j) * bw + bx) * 8;
        *reinterpret_cast<uint2*>(dst) = make_uint2(lo, hi);
    }
}

// jdsample.c: the chroma sample at output pixel (y, x) from plane P (row stride pw), whose real extent is n columns and m rows
__device__ __forceinline__ int chroma_at(const unsigned char* __restrict__ P, int pw, int n, int m, int hmax, int vmax, int y, int x) {
    if (hmax == 1) return P[(long long)y * pw + x];
    const int i = x >> 1;
    if (n <= 2) return P[(long long)(vmax == 2 ? y >> 1 : y) * pw + i];  // libjpeg takes the fancy filters only above 2 columns
    if (vmax == 1) {
        const unsigned char* row = P + (long long)y * pw;
        if (x & 1) return i == n - 1 ? row[i] : (3 * row[i] + row[i + 1] + 2) >> 2;
        return i == 0 ? row[0] : (3 * row[i] + row[i - 1] + 1) >> 2;
    }
    const int r = y >> 1;
    const int fr = (y & 1) ? min(r + 1, m - 1) : max(r - 1, 0);
    const unsigned char* near = P + (long long)r * pw;
    const unsigned char* far = P + (long long)fr * pw;
    const int s = 3 * near[i] + far[i];
    if (x & 1) return i == n - 1 ? (4 * s + 7) >> 4 : (3 * s + 3 * near[i + 1] + far[i + 1] + 7) >> 4;
    return i == 0 ? (4 * s + 8) >> 4 : (3 * s + 3 * near[i - 1] + far[i - 1] + 8) >> 4;
}

__device__ __forceinline__ int clamp_u8(int v) { return min(max(v, 0), 255); }

__global__ __launch_bounds__(JPEG_THREADS) void jpeg_store_kernel(const HpeJpegImage* __restrict__ table, int B, const unsigned char* __restrict__ workspace,
                                                                  unsigned char* __restrict__ frames) {
    const int b = find_image<&HpeJpegImage::store_group0>(table, B, (int)blockIdx.x);
    const HpeJpegImage* e = table + b;
    const int H = e->H, W = e->W, ch = e->channels, ncomp = e->ncomp;
    const int total = H * W * ch;  // < 2^31 by HPE_JPEG_MAX_SIDE
    const int first = ((blockIdx.x - e->store_group0) * JPEG_THREADS + threadIdx.x) * 4;
    if (first >= total) return;
    const unsigned char* Y = workspace + e->plane_offset[0];
    const int yw = e->blocks_w[0] * 8;
    const unsigned char* Cb = nullptr;
    const unsigned char* Cr = nullptr;
    int cw = 0, n = 0, m = 0;
    const int hmax = e->hmax, vmax = e->vmax;
    if (ncomp == 3) {
        Cb = workspace + e->plane_offset[1];
        Cr = workspace + e->plane_offset[2];
        cw = e->blocks_w[1] * 8;
        n = (W + hmax - 1) / hmax;
        m = (H + vmax - 1) / vmax;
    }
    int p = first / ch, c = first - p * ch;
    int y = p / W, x = p - y * W;
    const int count = min(4, total - first);
    u32 word = 0;
    for (int i = 0; i < count; ++i) {
        int v = Y[(long long)y * yw + x];
        if (ncomp == 3) {  // jdcolor.c
            if (c == 0) {
                const int cr = chroma_at(Cr, cw, n, m, hmax, vmax, y, x) - 128;
                v = clamp_u8(v + ((91881 * cr + 32768) >> 16));
            } else if (c == 1) {
                const int cb = chroma_at(Cb, cw, n, m, hmax, vmax, y, x) - 128, cr = chroma_at(Cr, cw, n, m, hmax, vmax, y, x) - 128;
                v = clamp_u8(v + ((-22554 * cb - 46802 * cr + 32768) >> 16));
            } else {
                const int cb = chroma_at(Cb, cw, n, m, hmax, vmax, y, x) - 128;
                v = clamp_u8(v + ((116130 * cb + 32768) >> 16));
            }
        }
        word |= (u32)v << (8 * i);
        if (++c == ch) {
            c = 0;
            if (++x == W) {
                x = 0;
                ++y;
            }
        }
    }
    unsigned char* dst = frames + e->out_offset + first;
    if (count == 4) {
        *reinterpret_cast<u32*>(dst) = word;
    } else {
        for (int i = 0; i < count; ++i) dst[i] = (unsigned char)(word >> (8 * i));
    }
}

// what hpe_jpeg_backend holds a table entry against; "" = fine.  g1 / g2: the workgroup bases the entry must carry.
const char* entry_fault(const HpeJpegImage& e, long long coef_count, long long workspace_bytes, long long frames_bytes, long long g1, long long g2) {
    if (e.H < 1 || e.W < 1 || e.H > HPE_JPEG_MAX_SIDE || e.W > HPE_JPEG_MAX_SIDE) return "H and W must be in [1, 16384]";
    if ((e.ncomp != 1 && e.ncomp != 3) || (e.channels != 1 && e.channels != 3) || (e.ncomp == 3 && e.channels != 3))
        return "ncomp and channels must be 1 or 3, and 3 components need 3 channels";
    const bool samp_ok = (e.hmax == 1 || e.hmax == 2) && (e.vmax == 1 || e.vmax == 2) && e.vmax <= e.hmax;
    if (!samp_ok) return "sampling must be 1x1, 2x1 or 2x2";
    for (int c = 0; c < e.ncomp; ++c) {
        if (e.blocks_w[c] != jpeg::blocks_for(e.W, e.hmax, c ? 1 : e.hmax) || e.blocks_h[c] != jpeg::blocks_for(e.H, e.vmax, c ? 1 : e.vmax))
            return "the block grid is not that of H, W and the sampling";
        const long long n = 64LL * e.blocks_w[c] * e.blocks_h[c];
        if (e.coef_offset[c] < 0 || e.coef_offset[c] > coef_count - n) return "coefficients outside the coefficient buffer";
        if (e.plane_offset[c] < 0 || (e.plane_offset[c] & 7) || e.plane_offset[c] > workspace_bytes - n) return "a plane outside the workspace or off an 8-byte boundary";
    }
    const long long bytes = (long long)e.H * e.W * e.channels;
    if (e.out_offset < 0 || (e.out_offset & 15) || e.out_offset > frames_bytes - bytes) return "the frame lies outside the frame buffer or off a 16-byte boundary";
    if (e.idct_group0 != g1 || e.store_group0 != g2) return "the workgroup bases are not the prefix sums of the images before";
    return "";
}

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

int hpe_jpeg_info(int B, const unsigned char* const* streams, const long long* lengths, HpeJpegInfo* info_out) {
    std::string why;
    const int rc = jpeg::info_batch(B, streams, lengths, info_out, &why);
    return rc == HPE_OK ? HPE_OK : fail(rc, why);
}

int hpe_jpeg_decode(int B, const unsigned char* const* streams, const long long* lengths, const int* channels, int threads, short* coef_out,
                    long long coef_capacity, HpeJpegImage* table_out, int* status_out, long long* totals_out) {
    std::string why;
    const int rc = jpeg::decode_batch(B, streams, lengths, channels, threads, coef_out, coef_capacity, table_out, status_out, totals_out, &why);
    return rc == HPE_OK ? HPE_OK : fail(rc, why);
}

int hpe_jpeg_backend(const HpeJpegImage* table_host, const HpeJpegImage* table_dev, int B, const short* coef_dev, long long coef_count,
                     unsigned char* workspace_dev, long long workspace_bytes, unsigned char* frames_dev, long long frames_bytes, void* stream) {
    if (!table_host || !table_dev || !coef_dev || !workspace_dev || !frames_dev) return fail(HPE_ERR_INVALID, "null argument");
    if (B < 1) return fail(HPE_ERR_INVALID, "B must be >= 1");
    if (coef_count < 0 || workspace_bytes < 0 || frames_bytes < 0) return fail(HPE_ERR_INVALID, "negative buffer size");
    if (((uintptr_t)workspace_dev | (uintptr_t)frames_dev | (uintptr_t)table_dev) & 15)
        return fail(HPE_ERR_INVALID, "table_dev, workspace_dev and frames_dev must be 16-byte aligned");
    if ((uintptr_t)coef_dev & 1) return fail(HPE_ERR_INVALID, "coef_dev must be 2-byte aligned");
    long long g1 = 0, g2 = 0;
    for (int b = 0; b < B; ++b) {
        const HpeJpegImage& e = table_host[b];
        const char* fault = entry_fault(e, coef_count, workspace_bytes, frames_bytes, g1, g2);
        if (fault[0]) return fail(HPE_ERR_INVALID, "table entry " + std::to_string(b) + ": " + fault);
        long long blocks = 0;
        for (int c = 0; c < e.ncomp; ++c) blocks += (long long)e.blocks_w[c] * e.blocks_h[c];
        g1 += (blocks + jpeg::IDCT_BLOCKS_PER_GROUP - 1) / jpeg::IDCT_BLOCKS_PER_GROUP;
        g2 += ((long long)e.H * e.W * e.channels + jpeg::STORE_BYTES_PER_GROUP - 1) / jpeg::STORE_BYTES_PER_GROUP;
        if (g1 > 0x7fffffffLL || g2 > 0x7fffffffLL) return fail(HPE_ERR_INVALID, "the batch needs more than 2^31 workgroups");
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)g1), dim3(JPEG_THREADS), 0, st, table_dev, B, coef_dev, workspace_dev);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(jpeg_store_kernel, dim3((unsigned)g2), dim3(JPEG_THREADS), 0, st, table_dev, B, static_cast<const unsigned char*>(workspace_dev), frames_dev);
    HIP_TRY(hipGetLastError());
    return HPE_OK;
}

}  // extern "C"
#pragma GCC visibility pop
