// jpeg_encode.hip -- the data-parallel half of the JPEG encoder (DESIGN.md "Dataset writers and JPEG encode"): colour conversion, chroma
// downsampling, 8x8 forward DCT and quantisation for a whole batch of mixed sizes in one launch, plus the C ABI of the host half
// (jpeg_huffman_enc.hip).  The definition is libjpeg's default compressor -- jccolor.c, jcsample.c without smoothing, the edge rules
// of jcprepct.c / jccoefct.c, jfdctint.c (JDCT_ISLOW) -- and the contract is bit-exactness, so everything is 32-bit integer arithmetic
// (8-bit samples keep every intermediate inside int32).
//
// The mirror of jpeg_idct_kernel: 8 threads per block -- one per row (pass 1), then one per column (pass 2 and the quantiser), then one
// per row again for the store, each 8x8 transpose through LDS -- 32 blocks per workgroup; the grid is the concatenation of the images'
// workgroups and a workgroup finds its image by a search of the workgroup-uniform table.  A thread gathers its 8 samples straight from
// the packed uint8 frame with clamped coordinates (the edge rules), a chroma sample converting and averaging its own 2 or 4 pixels, so no
// sample plane is ever written.  A dummy block (outside the component's real grid, inside its MCU grid) transforms the block whose DC it
// repeats and keeps the DC alone.  A natural-order row of 8 int16 leaves as one 16-byte store.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "batch_table.h"
#include "hpe_ctx.h"
#include "jpeg.h"

namespace {

constexpr int ENC_THREADS = 256;
static_assert(jpeg::IDCT_BLOCKS_PER_GROUP * 8 == ENC_THREADS, "8 threads per block");
static_assert(sizeof(HpeJpegEncImage) == 232, "the table entry of include/hpe.h and jpeg_encode.py");

// jfdctint.c's 1-D kernel on d[0..7] (level-shifted samples, or pass 1's outputs).  FIRST: the even outputs are << 2 and the others
// descaled by 11 bits; otherwise the even outputs are descaled by 2 bits and the others by 15.
template <bool FIRST>
__device__ __forceinline__ void fdct8(const int* d, int* out) {
    const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
    const int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    constexpr int SHIFT = FIRST ? 11 : 15, R = 1 << (SHIFT - 1);
    if (FIRST) {
        out[0] = (t10 + t11) << 2;
        out[4] = (t10 - t11) << 2;
    } else {
        out[0] = (t10 + t11 + 2) >> 2;
        out[4] = (t10 - t11 + 2) >> 2;
    }
    int z1 = (t12 + t13) * 4433;
    out[2] = (z1 + t13 * 6270 + R) >> SHIFT;
    out[6] = (z1 - t12 * 15137 + R) >> SHIFT;
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * 9633;
    const int m4 = t4 * 2446, m5 = t5 * 16819, m6 = t6 * 25172, m7 = t7 * 12299;
    z1 *= -7373;
    z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    out[7] = (m4 + z1 + z3 + R) >> SHIFT;
    out[5] = (m5 + z2 + z4 + R) >> SHIFT;
    out[3] = (m6 + z2 + z3 + R) >> SHIFT;
    out[1] = (m7 + z1 + z4 + R) >> SHIFT;
}

// jccolor.c on one RGB pixel: component c of (Y, Cb, Cr)
__device__ __forceinline__ int ycc(const unsigned char* __restrict__ px, int c) {
    const int r = px[0], g = px[1], b = px[2];
    if (c == 0) return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
    if (c == 1) return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
    return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

__global__ __launch_bounds__(ENC_THREADS) void jpeg_forward_kernel(const HpeJpegEncImage* __restrict__ table, int B,
                                                                   const unsigned char* __restrict__ frames, short* __restrict__ coef) {
    __shared__ int ws[jpeg::IDCT_BLOCKS_PER_GROUP][8][9];  // [block][row][column], rows padded against bank conflicts in the column pass
    const int b = find_image<&HpeJpegEncImage::group0>(table, B, (int)blockIdx.x);
    const HpeJpegEncImage* e = table + b;
    const int slot = threadIdx.x >> 3, j = threadIdx.x & 7;
    int k = (blockIdx.x - e->group0) * jpeg::IDCT_BLOCKS_PER_GROUP + slot;  // block of the image, components back to back
    int c = 0;
    const int C = e->C;
    while (c < C && k >= e->blocks_w[c] * e->blocks_h[c]) {
        k -= e->blocks_w[c] * e->blocks_h[c];
        ++c;
    }
    const bool active = c < C;
    bool dummy = false;
    if (active) {  // pass 1: row j of the block's samples
        const int H = e->H, W = e->W, bw = e->blocks_w[c], rw = e->real_w[c], rh = e->real_h[c];
        const int by = k / bw, bx = k - by * bw;
        int sy = by, sx = bx;  // the block whose samples are transformed: a dummy block takes the one whose DC it repeats
        if (by >= rh) {        // a bottom dummy row repeats the last block of the MCU's row above, itself possibly a right dummy
            const int h = c ? 1 : e->hmax;
            sy = rh - 1;
            sx = min(bx / h * h + h - 1, rw - 1);
            dummy = true;
        } else if (bx >= rw) {
            sx = rw - 1;
            dummy = true;
        }
        const unsigned char* frame = frames + e->frame_offset;
        const int r = sy * 8 + j;
        int d[8], out[8];
        if (C == 1) {
            const unsigned char* row = frame + (long long)min(r, H - 1) * W;
#pragma unroll
            for (int x = 0; x < 8; ++x) d[x] = (int)row[min(sx * 8 + x, W - 1)] - 128;
        } else if (c == 0 || (e->hmax == 1 && e->vmax == 1)) {  // full resolution: the source replicated to the right and downwards
            const unsigned char* row = frame + (long long)min(r, H - 1) * W * 3;
#pragma unroll
            for (int x = 0; x < 8; ++x) d[x] = ycc(row + min(sx * 8 + x, W - 1) * 3, c) - 128;
        } else if (e->vmax == 1) {  // 2x1: bias 0, 1, 0, 1, ... along the output row
            const unsigned char* row = frame + (long long)min(r, H - 1) * W * 3;
#pragma unroll
            for (int x = 0; x < 8; ++x) {
                const int cc = sx * 8 + x;
                const int s = ycc(row + min(2 * cc, W - 1) * 3, c) + ycc(row + min(2 * cc + 1, W - 1) * 3, c);
                d[x] = ((s + (cc & 1)) >> 1) - 128;
            }
        } else {  // 2x2: the source rows are replicated to an even count only; below that the last DOWNSAMPLED row repeats
            const int rr = min(r, (H + 1) / 2 - 1);
            const unsigned char* row0 = frame + (long long)(2 * rr) * W * 3;
            const unsigned char* row1 = frame + (long long)min(2 * rr + 1, H - 1) * W * 3;
#pragma unroll
            for (int x = 0; x < 8; ++x) {
                const int cc = sx * 8 + x;
                const int x0 = min(2 * cc, W - 1) * 3, x1 = min(2 * cc + 1, W - 1) * 3;
                const int s = ycc(row0 + x0, c) + ycc(row0 + x1, c) + ycc(row1 + x0, c) + ycc(row1 + x1, c);
                d[x] = ((s + 1 + (cc & 1)) >> 2) - 128;  // bias 1, 2, 1, 2, ...
            }
        }
        fdct8<true>(d, out);
#pragma unroll
        for (int x = 0; x < 8; ++x) ws[slot][j][x] = out[x];
    }
    __syncthreads();
    if (active) {  // pass 2 and the quantiser: column j, which this thread alone reads and writes back
        const unsigned char* q = e->quant[c ? 1 : 0];
        int d[8], out[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) d[r] = ws[slot][r][j];
        fdct8<false>(d, out);
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int div = 8 * (int)q[r * 8 + j];
            const int v = out[r], a = (abs(v) + (div >> 1)) / div;
            ws[slot][r][j] = v < 0 ? -a : a;
        }
    }
    __syncthreads();
    if (active) {  // row j in natural order: 8 int16, one 16-byte store
        uint32_t w[4];
#pragma unroll
        for (int x = 0; x < 4; ++x) {
            int lo = ws[slot][j][2 * x], hi = ws[slot][j][2 * x + 1];
            if (dummy) {
                lo = (j == 0 && x == 0) ? lo : 0;
                hi = 0;
            }
            w[x] = ((uint32_t)lo & 0xFFFFu) | ((uint32_t)hi << 16);
        }
        short* dst = coef + e->coef_offset[c] + (long long)k * 64 + j * 8;
        *reinterpret_cast<uint4*>(dst) = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

int hpe_jpeg_encode_layout(int B, const int* shapes, const long long* frame_offsets, int hmax, int vmax, int quality,
                           HpeJpegEncImage* table_out, long long* totals_out) {
    std::string why;
    const int rc = jpeg::encode_layout(B, shapes, frame_offsets, hmax, vmax, quality, table_out, totals_out, &why);
    return rc == HPE_OK ? HPE_OK : fail(rc, why);
}

int hpe_jpeg_entropy_encode(const HpeJpegEncImage* table, int B, const short* coef, long long coef_count, int units, int xdensity,
                            int ydensity, int threads, unsigned char* out, long long out_capacity, long long* offsets_out,
                            long long* lengths_out) {
    std::string why;
    const int rc = jpeg::entropy_encode(table, B, coef, coef_count, units, xdensity, ydensity, threads, out, out_capacity, offsets_out, lengths_out, &why);
    return rc == HPE_OK ? HPE_OK : fail(rc, why);
}

int hpe_jpeg_forward(const HpeJpegEncImage* table_host, const HpeJpegEncImage* table_dev, int B, const unsigned char* frames_dev,
                     long long frames_bytes, short* coef_dev, long long coef_count, void* stream) {
    if (!table_host) return fail(HPE_ERR_INVALID, "null argument");
    if (B < 1) return fail(HPE_ERR_INVALID, "B must be >= 1");
    if (frames_bytes < 0 || coef_count < 0) return fail(HPE_ERR_INVALID, "negative buffer size");
    long long groups = 0;
    for (int b = 0; b < B; ++b) {
        const HpeJpegEncImage& e = table_host[b];
        const char* fault = jpeg::enc_entry_fault(e);
        if (!fault[0] && (e.frame_offset < 0 || e.frame_offset > frames_bytes - (long long)e.H * e.W * e.C)) fault = "the frame lies outside the frame buffer";
        for (int c = 0; !fault[0] && c < e.C; ++c)
            if (e.coef_offset[c] > coef_count - 64LL * e.blocks_w[c] * e.blocks_h[c]) fault = "coefficients outside the coefficient buffer";
        if (!fault[0] && e.group0 != groups) fault = "the workgroup base is not the prefix sum of the images before";
        if (fault[0]) return fail(HPE_ERR_INVALID, "table entry " + std::to_string(b) + ": " + fault);
        groups += (jpeg::enc_blocks(e) + jpeg::IDCT_BLOCKS_PER_GROUP - 1) / jpeg::IDCT_BLOCKS_PER_GROUP;
        if (groups > 0x7fffffffLL) return fail(HPE_ERR_INVALID, "the batch needs more than 2^31 workgroups");
    }
    if (!table_dev || !frames_dev || !coef_dev) return fail(HPE_ERR_INVALID, "null argument");
    if ((uintptr_t)table_dev & 7) return fail(HPE_ERR_INVALID, "table_dev must be 8-byte aligned");
    if ((uintptr_t)coef_dev & 15) return fail(HPE_ERR_INVALID, "coef_dev must be 16-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(jpeg_forward_kernel, dim3((unsigned)groups), dim3(ENC_THREADS), 0, st, table_dev, B, frames_dev, coef_dev);
    HIP_TRY(hipGetLastError());
    return HPE_OK;
}

}  // extern "C"
#pragma GCC visibility pop
