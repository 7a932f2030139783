// png_decode.hip -- the per-byte half of the PNG decoder (DESIGN.md "PNG streams in the records"): the PNG unfilter and the store, for a
// whole batch of mixed sizes, colour types and depths in two launches.  The chunk walk and inflate are host code (hpe_amd/png.py); the
// table check every loop bound below rests on is png.h.  Lossless, so the contract is bit-exactness.
//
// Launch one, the unfilter: Recon(x) = Filt(x) + pred(a, b, c) mod 256 with a = Recon(x - bpp), b = Prior(x), c = Prior(x - bpp) is a
// true 2-D recurrence (Average and Paeth are no prefix sums), so all five filters share one schedule, a skewed wavefront.  One workgroup
// of one wave64 per image; the lanes are the 64 rows of a strip; at step s lane r handles group s - r of its row, a group being 4 bytes
// of the row (12 when bpp = 3: four whole pixels, three dwords), loaded and stored as dwords; the loads run four steps ahead of
// the recurrence, which they do not depend on.  b of the whole group is what the lane
// above produced one step earlier and arrives by one cross-lane move per dword; c of its first pixel is the tail of the b group before,
// a the tail of the lane's own group before: both stay in registers.  The filter is selected per byte by masks, without a branch, so
// rows of different filters do not diverge; a strip without a Paeth row (one wave-uniform vote) runs a body without Paeth's arithmetic.  The last row of a strip reaches lane 0 of the next strip through one row buffer in LDS: lane 63
// writes group s - 63 at the step lane 0 reads group s, so one buffer serves both strips, and LDS operations of one wave retire in
// order.  No barrier per step, no atomics, no waiting on another workgroup.
// Launch two, the store: 4 adjacent output BYTES per thread and one aligned dword store, as jpeg_store_kernel; each byte is one channel
// of one pixel: unpack (depths 1, 2, 4), palette, alpha dropped, grey <-> colour.  Direct images (8-bit grey to 1 channel, 8-bit RGB
// to 3) were unfiltered straight into the frame buffer and have no workgroup here.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "batch_table.h"
#include "hpe_ctx.h"
#include "png.h"

namespace {

constexpr int PNG_WAVE = 64;
constexpr int PNG_STORE_THREADS = 256;
static_assert(png::STORE_BYTES_PER_GROUP == PNG_STORE_THREADS * 4, "4 output bytes per thread");
static_assert(sizeof(HpePngImage) == 64, "the table entry of include/hpe.h and png.py");

typedef unsigned int u32;

// One byte of the recurrence.  The row's filter arrives as four byte masks (Sub, Up, Average, Paeth: one is 255, or none for None), so
// the predictor is picked with AND / OR and rows of different filters run the same instructions: written with ?: on the filter type
// the compiler turns every byte into five divergent branches.  Paeth's ties go to a, then b, then c.  PAETH false: no row of the strip
// uses Paeth and its arithmetic is left out.
template <bool PAETH>
__device__ __forceinline__ u32 recon_byte(u32 msub, u32 mup, u32 mavg, u32 mpaeth, u32 f, u32 a, u32 b, u32 c) {
    u32 pred = (a & msub) | (b & mup) | (((a + b) >> 1) & mavg);  // (a + b) is a 9-bit sum
    if (PAETH) {
        const int pa = abs((int)b - (int)c), pb = abs((int)a - (int)c), pc = abs((int)a + (int)b - 2 * (int)c);
        const u32 bc = pb <= pc ? b : c;
        const u32 paeth = (pa <= pb && pa <= pc) ? a : bc;
        pred |= paeth & mpaeth;
    }
    return (f + pred) & 255u;
}

constexpr int PNG_AHEAD = 4;  // steps whose filtered bytes are in flight while a step computes

// the filtered bytes of group m of the row at src, n of them real (the row's last group may be short): zero where there are none
template <int GB>
__device__ __forceinline__ void load_group(const unsigned char* __restrict__ src, int m, int n, u32* f) {
    const unsigned char* p = src + (long long)m * GB;
    if (n == GB) {
        __builtin_memcpy(f, p, GB);
    } else {
#pragma unroll
        for (int d = 0; d < GB / 4; ++d) f[d] = 0u;
#pragma unroll 1
        for (int i = 0; i < n; ++i) {  // rolled: once per row; the dword is picked by selects, so the group stays in registers
            const u32 v = (u32)p[i] << (8 * (i & 3));
#pragma unroll
            for (int d = 0; d < GB / 4; ++d) f[d] |= (i >> 2) == d ? v : 0u;
        }
    }
}

// one strip of `rows` rows (this lane's: src -> out, filter type ft); first: nothing above it; feeds_next: this lane is the last row of
// a strip that has a successor
template <int BPP, bool PAETH>
__device__ __forceinline__ void unfilter_strip(const unsigned char* __restrict__ src, unsigned char* __restrict__ out, u32* row, u32 ft, int rows,
                                               int rowbytes, bool live, bool first, bool feeds_next) {
    constexpr int GB = BPP == 3 ? 12 : 4, ND = GB / 4;  // bytes and dwords of a group: whole pixels
    const int lane = threadIdx.x;
    const int ngroups = (rowbytes + GB - 1) / GB;
    const u32 msub = ft == 1u ? 255u : 0u, mup = ft == 2u ? 255u : 0u, mavg = ft == 3u ? 255u : 0u, mpaeth = ft == 4u ? 255u : 0u;
    u32 mine[ND], above[ND];  // the group this lane reconstructed last, and the b group it had: a and c of the next first pixel
#pragma unroll
    for (int d = 0; d < ND; ++d) mine[d] = above[d] = 0u;  // left of the row reads zero
    // the filtered bytes do not depend on the recurrence: those of the next PNG_AHEAD steps are loaded while these compute, so a step
    // does not wait for memory.  No lane is active at a step >= ngroups + rows - 1, so the padded steps do nothing.
    const int steps = (ngroups + rows - 1 + PNG_AHEAD - 1) / PNG_AHEAD * PNG_AHEAD;
    u32 f[PNG_AHEAD][ND];
#pragma unroll
    for (int k = 0; k < PNG_AHEAD; ++k) {
        const int m = k - lane;
#pragma unroll
        for (int d = 0; d < ND; ++d) f[k][d] = 0u;
        if (live && m >= 0 && m < ngroups) load_group<GB>(src, m, min(GB, rowbytes - m * GB), f[k]);
    }
    for (int s0 = 0; s0 < steps; s0 += PNG_AHEAD) {
        u32 fn[PNG_AHEAD][ND];
#pragma unroll
        for (int k = 0; k < PNG_AHEAD; ++k) {
            const int m = s0 + PNG_AHEAD + k - lane;
#pragma unroll
            for (int d = 0; d < ND; ++d) fn[k][d] = 0u;
            if (live && m >= 0 && m < ngroups) load_group<GB>(src, m, min(GB, rowbytes - m * GB), fn[k]);
        }
#pragma unroll
        for (int k = 0; k < PNG_AHEAD; ++k) {
            const int s = s0 + k;
            u32 up[ND];
#pragma unroll
            for (int d = 0; d < ND; ++d) up[d] = __shfl_up(mine[d], 1);  // every lane, every step: lane r - 1 handled this group one step ago
            const int m = s - lane;
            const bool active = live && m >= 0 && m < ngroups;
            if (lane == 0) {  // the row above the strip: the strip before left it in LDS; above row 0 reads zero
#pragma unroll
                for (int d = 0; d < ND; ++d) up[d] = 0u;
                if (!first && active) {
#pragma unroll
                    for (int d = 0; d < ND; ++d) up[d] = row[m * ND + d];
                }
            }
            if (active) {
                const int n = min(GB, rowbytes - m * GB);
                u32 r[GB];
#pragma unroll
                for (int i = 0; i < GB; ++i) {
                    const int j = i - BPP, t = GB + j;  // the byte one pixel to the left: in this group, or the tail of the one before
                    const u32 a = j >= 0 ? r[j] : (mine[t >> 2] >> (8 * (t & 3))) & 255u;
                    const u32 c = j >= 0 ? (up[j >> 2] >> (8 * (j & 3))) & 255u : (above[t >> 2] >> (8 * (t & 3))) & 255u;
                    const u32 b = (up[i >> 2] >> (8 * (i & 3))) & 255u;
                    r[i] = recon_byte<PAETH>(msub, mup, mavg, mpaeth, (f[k][i >> 2] >> (8 * (i & 3))) & 255u, a, b, c);
                }
#pragma unroll
                for (int d = 0; d < ND; ++d) {
                    mine[d] = r[4 * d] | r[4 * d + 1] << 8 | r[4 * d + 2] << 16 | r[4 * d + 3] << 24;
                    above[d] = up[d];
                }
                unsigned char* q = out + (long long)m * GB;
                if (n == GB) {
                    __builtin_memcpy(q, mine, GB);
                } else {
#pragma unroll 1
                    for (int i = 0; i < n; ++i) {
                        u32 w = mine[0];
#pragma unroll
                        for (int d = 1; d < ND; ++d) w = (i >> 2) == d ? mine[d] : w;
                        q[i] = (unsigned char)(w >> (8 * (i & 3)));
                    }
                }
                if (feeds_next) {  // bytes past the row's end in the last group are never read as pixels
#pragma unroll
                    for (int d = 0; d < ND; ++d) row[m * ND + d] = mine[d];
                }
            }
        }
#pragma unroll
        for (int k = 0; k < PNG_AHEAD; ++k)
#pragma unroll
            for (int d = 0; d < ND; ++d) f[k][d] = fn[k][d];
    }
}

template <int BPP>
__device__ __forceinline__ void unfilter_image(const unsigned char* __restrict__ raw, unsigned char* __restrict__ dst, u32* row, int H, int rowbytes) {
    const int lane = threadIdx.x;
    for (int y0 = 0; y0 < H; y0 += PNG_WAVE) {
        const int rows = min(PNG_WAVE, H - y0);
        const bool live = lane < rows;
        const unsigned char* src = raw + (long long)(y0 + (live ? lane : 0)) * (rowbytes + 1LL);
        u32 ft = live ? (u32)src[0] : 0u;
        if (ft > 4u) ft = 0u;  // the host refused such a row; never an index here
        unsigned char* out = dst + (long long)(y0 + (live ? lane : 0)) * rowbytes;
        const bool feeds_next = lane == PNG_WAVE - 1 && y0 + PNG_WAVE < H;
        if (__any(ft == 4u))  // wave-uniform
            unfilter_strip<BPP, true>(src + 1, out, row, ft, rows, rowbytes, live, y0 == 0, feeds_next);
        else
            unfilter_strip<BPP, false>(src + 1, out, row, ft, rows, rowbytes, live, y0 == 0, feeds_next);
        // one wave: its LDS operations retire in order; this only keeps the compiler from moving them across the strips
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
}

__global__ __launch_bounds__(PNG_WAVE) void png_unfilter_kernel(const HpePngImage* __restrict__ table, const unsigned char* __restrict__ raw,
                                                                unsigned char* __restrict__ workspace, unsigned char* __restrict__ frames) {
    extern __shared__ u32 png_row[];
    const HpePngImage* e = table + blockIdx.x;
    const int H = e->H, rowbytes = e->rowbytes, bpp = e->bpp;
    const unsigned char* src = raw + e->raw_offset;
    unsigned char* dst = e->work_offset < 0 ? frames + e->out_offset : workspace + e->work_offset;
    if (bpp == 1)
        unfilter_image<1>(src, dst, png_row, H, rowbytes);
    else if (bpp == 2)
        unfilter_image<2>(src, dst, png_row, H, rowbytes);
    else if (bpp == 3)
        unfilter_image<3>(src, dst, png_row, H, rowbytes);
    else
        unfilter_image<4>(src, dst, png_row, H, rowbytes);
}

// Colour to grey: libpng's png_set_rgb_to_gray without gamma, coefficients 9797 / 19234 / 3737 of 32768 (they sum to 32768, so a grey
// pixel keeps its value).  TRUNCATING, as libpng 1.6's png_do_rgb_to_gray does without a gamma table ("the historical approach which
// simply truncates"); the rounding variant would add 16384.  DESIGN.md states what this rests on.
__device__ __forceinline__ u32 png_rgb_to_gray(u32 r, u32 g, u32 b) { return (9797u * r + 19234u * g + 3737u * b) >> 15; }

// sample x of a row at depth 1, 2, 4 or 8 with `samples` per pixel (below 8 bits: one sample per pixel, leftmost pixel in the high bits)
__device__ __forceinline__ u32 sample_at(const unsigned char* __restrict__ row, int x, int depth) {
    if (depth == 8) return row[x];
    const int bit = x * depth;
    return ((u32)row[bit >> 3] >> (8 - depth - (bit & 7))) & ((1u << depth) - 1u);
}

__global__ __launch_bounds__(PNG_STORE_THREADS) void png_store_kernel(const HpePngImage* __restrict__ table, int B, const unsigned char* __restrict__ raw,
                                                                      const unsigned char* __restrict__ workspace, unsigned char* __restrict__ frames) {
    const int b = find_image<&HpePngImage::store_group0>(table, B, (int)blockIdx.x);
    const HpePngImage* e = table + b;
    if (e->work_offset < 0) return;  // a direct image has no workgroup: not reached with a checked table
    const int H = e->H, W = e->W, ch = e->channels, ct = e->color_type, depth = e->depth, rowbytes = e->rowbytes;
    const int total = H * W * ch;  // < 2^31 by HPE_PNG_MAX_SIDE
    const int first = ((blockIdx.x - e->store_group0) * PNG_STORE_THREADS + threadIdx.x) * 4;
    if (first >= total) return;
    const unsigned char* rows = workspace + e->work_offset;
    const u32* pal = ct == 3 ? reinterpret_cast<const u32*>(raw + e->pal_offset) : nullptr;
    const u32 scale = depth == 1 ? 255u : depth == 2 ? 85u : depth == 4 ? 17u : 1u;
    int p = first / ch, c = first - p * ch;
    int y = p / W, x = p - y * W;
    const int count = min(4, total - first);
    u32 word = 0;
    for (int i = 0; i < count; ++i) {
        const unsigned char* row = rows + (long long)y * rowbytes;
        u32 v;
        if (ct == 0) {
            v = sample_at(row, x, depth) * scale;
        } else if (ct == 4) {
            v = row[2 * x];  // alpha is dropped, not blended
        } else {
            u32 r, g, bl;
            if (ct == 3) {
                const u32 rgb = pal[sample_at(row, x, depth)];  // 256 entries whatever PLTE held: an index beyond it reads black
                r = rgb & 255u, g = (rgb >> 8) & 255u, bl = (rgb >> 16) & 255u;
            } else {
                const unsigned char* px = row + x * (ct == 2 ? 3 : 4);
                r = px[0], g = px[1], bl = px[2];
            }
            v = ch == 1 ? png_rgb_to_gray(r, g, bl) : c == 0 ? r : c == 1 ? g : bl;
        }
        word |= v << (8 * i);
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

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

int hpe_png_backend(const HpePngImage* table_host, const HpePngImage* table_dev, int B, const unsigned char* raw_dev, long long raw_bytes,
                    unsigned char* workspace_dev, long long workspace_bytes, unsigned char* frames_dev, long long frames_bytes, void* stream) {
    std::string why;
    long long groups = 0;
    int lds = 0;
    if (png::check_table(table_host, B, raw_bytes, workspace_bytes, frames_bytes, &groups, &lds, &why) != HPE_OK) return fail(HPE_ERR_INVALID, why);
    if (!table_dev || !raw_dev || !frames_dev || (!workspace_dev && workspace_bytes > 0)) return fail(HPE_ERR_INVALID, "null argument");
    if (((uintptr_t)workspace_dev | (uintptr_t)frames_dev | (uintptr_t)table_dev | (uintptr_t)raw_dev) & 15)
        return fail(HPE_ERR_INVALID, "table_dev, raw_dev, workspace_dev and frames_dev must be 16-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(png_unfilter_kernel, dim3((unsigned)B), dim3(PNG_WAVE), (size_t)lds, st, table_dev, raw_dev, workspace_dev, frames_dev);
    HIP_TRY(hipGetLastError());
    if (groups > 0) {
        hipLaunchKernelGGL(png_store_kernel, dim3((unsigned)groups), dim3(PNG_STORE_THREADS), 0, st, table_dev, B, raw_dev,
                           static_cast<const unsigned char*>(workspace_dev), frames_dev);
        HIP_TRY(hipGetLastError());
    }
    return HPE_OK;
}

}  // extern "C"
#pragma GCC visibility pop
