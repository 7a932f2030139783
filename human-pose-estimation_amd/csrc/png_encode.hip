// png_encode.hip -- the per-byte half of the PNG encoder (DESIGN.md "Training summaries"), the mirror of png_decode.hip: packed uint8
// frames -> PNG scanlines (one filter byte and W * C filtered bytes per row) for a whole batch of mixed sizes in ONE launch.  Deflate
// and the chunk wrapping are host code (hpe_amd/png_encode.py: zlib).  Lossless, so the contract is bit-exactness against the rule
// stated here and restated in tests/png_encode_ref.py.
//
// Filter choice per row is libpng's minimum-sum rule: all five candidates (None, Sub, Up, Average, Paeth) of a byte come from RAW
// neighbours only -- a the byte bpp = C to the left, b the byte above, c the byte above a; zero left of the first pixel and above the
// first row --, each candidate is scored by the sum over its bytes of (v < 128 ? v : 256 - v), the smallest score wins and equal
// scores go to the lowest filter number.  Because nothing depends on a filtered byte, rows are independent (unlike the unfilter's 2-D
// recurrence): the grid runs over all rows of the batch, one wave64 per row, lanes striding the row.  Pass one accumulates the five
// sums per lane (a row has at most 65536 bytes of at most 128 each: 2^23, exact in 32 bits) and reduces them across the wave by a
// fixed butterfly; pass two writes the filter byte and the chosen candidate.  No atomics, no LDS, no waiting on another workgroup.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "batch_table.h"
#include "hpe_ctx.h"

namespace {

constexpr int ENC_WAVE = 64;
constexpr int ENC_ROWS_PER_GROUP = 4;  // waves of a workgroup, one row each
static_assert(sizeof(HpePngFilterImage) == 32, "the table entry of include/hpe.h and png_encode.py");

typedef unsigned int u32;

__device__ __forceinline__ u32 paeth_pred(u32 a, u32 b, u32 c) {  // ties in the order a, b, c
    const int pa = abs((int)b - (int)c), pb = abs((int)a - (int)c), pc = abs((int)a + (int)b - 2 * (int)c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

__device__ __forceinline__ u32 filter_score(u32 v) { return v < 128u ? v : 256u - v; }

// candidate f of raw byte x with raw neighbours a, b, c
__device__ __forceinline__ u32 filter_byte(u32 f, u32 x, u32 a, u32 b, u32 c) {
    const u32 pred = f == 0u ? 0u : f == 1u ? a : f == 2u ? b : f == 3u ? ((a + b) >> 1) : paeth_pred(a, b, c);
    return (x - pred) & 255u;
}

__device__ __forceinline__ u32 wave_sum(u32 v) {  // the same butterfly in every lane: all lanes end with the total
#pragma unroll
    for (int off = ENC_WAVE / 2; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

__global__ __launch_bounds__(ENC_WAVE* ENC_ROWS_PER_GROUP) void png_filter_kernel(const HpePngFilterImage* __restrict__ table, int B, long long rows,
                                                                                   const unsigned char* __restrict__ frames,
                                                                                   unsigned char* __restrict__ scan) {
    const int lane = threadIdx.x & (ENC_WAVE - 1);
    const long long row = (long long)blockIdx.x * ENC_ROWS_PER_GROUP + (threadIdx.x / ENC_WAVE);  // wave-uniform
    if (row >= rows) return;
    const HpePngFilterImage* e = table + find_image<&HpePngFilterImage::row0>(table, B, row);
    const int y = (int)(row - e->row0), bpp = e->C, rb = e->W * e->C;  // rb <= 16384 * 4
    const unsigned char* cur = frames + e->frame_offset + (long long)y * rb;
    const unsigned char* prev = cur - rb;  // read only when y > 0
    const bool has_prev = y > 0;
    u32 s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0;
    for (int i = lane; i < rb; i += ENC_WAVE) {
        const bool left = i >= bpp;
        const u32 x = cur[i], a = left ? cur[i - bpp] : 0u, b = has_prev ? prev[i] : 0u, c = (left && has_prev) ? prev[i - bpp] : 0u;
        s0 += filter_score(x);
        s1 += filter_score((x - a) & 255u);
        s2 += filter_score((x - b) & 255u);
        s3 += filter_score((x - ((a + b) >> 1)) & 255u);
        s4 += filter_score((x - paeth_pred(a, b, c)) & 255u);
    }
    s0 = wave_sum(s0), s1 = wave_sum(s1), s2 = wave_sum(s2), s3 = wave_sum(s3), s4 = wave_sum(s4);
    u32 best = s0, ft = 0u;  // strict <: equal scores keep the lowest filter number
    if (s1 < best) best = s1, ft = 1u;
    if (s2 < best) best = s2, ft = 2u;
    if (s3 < best) best = s3, ft = 3u;
    if (s4 < best) best = s4, ft = 4u;
    unsigned char* out = scan + e->scan_offset + (long long)y * (rb + 1LL);
    if (lane == 0) out[0] = (unsigned char)ft;
    for (int i = lane; i < rb; i += ENC_WAVE) {
        const bool left = i >= bpp;
        const u32 x = cur[i], a = left ? cur[i - bpp] : 0u, b = has_prev ? prev[i] : 0u, c = (left && has_prev) ? prev[i - bpp] : 0u;
        out[1 + i] = (unsigned char)filter_byte(ft, x, a, b, c);
    }
}

// "" = fine.  row0: the row base the entry must carry
const char* filter_entry_fault(const HpePngFilterImage& e, long long frames_bytes, long long scan_bytes, long long row0) {
    if (e.C != 1 && e.C != 3 && e.C != 4) return "C must be 1, 3 or 4";
    if (e.H < 1 || e.W < 1 || e.H > HPE_PNG_MAX_SIDE || e.W > HPE_PNG_MAX_SIDE) return "H and W must be in [1, 16384]";
    const long long rb = (long long)e.W * e.C, bytes = (long long)e.H * rb, lines = (long long)e.H * (rb + 1);
    if (e.frame_offset < 0 || e.frame_offset > frames_bytes - bytes) return "the frame lies outside the frame buffer";
    if (e.scan_offset < 0 || e.scan_offset > scan_bytes - lines) return "the scanlines lie outside the scanline buffer";
    if (e.row0 != row0) return "the row base is not the prefix sum of the images before";
    return "";
}

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

int hpe_png_filter(const HpePngFilterImage* table_host, const HpePngFilterImage* table_dev, int B, const unsigned char* frames_dev,
                   long long frames_bytes, unsigned char* scan_dev, long long scan_bytes, void* stream) {
    if (!table_host) return fail(HPE_ERR_INVALID, "null argument");
    if (B < 1) return fail(HPE_ERR_INVALID, "B must be >= 1");
    if (frames_bytes < 0 || scan_bytes < 0) return fail(HPE_ERR_INVALID, "negative buffer size");
    long long rows = 0;
    for (int b = 0; b < B; ++b) {
        const char* fault = filter_entry_fault(table_host[b], frames_bytes, scan_bytes, rows);
        if (fault[0]) return fail(HPE_ERR_INVALID, "table entry " + std::to_string(b) + ": " + fault);
        rows += table_host[b].H;
    }
    const long long groups = (rows + ENC_ROWS_PER_GROUP - 1) / ENC_ROWS_PER_GROUP;
    if (groups > 0x7fffffffLL) return fail(HPE_ERR_INVALID, "the batch needs more than 2^31 workgroups");
    if (!table_dev || !frames_dev || !scan_dev) return fail(HPE_ERR_INVALID, "null argument");
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(png_filter_kernel, dim3((unsigned)groups), dim3(ENC_WAVE * ENC_ROWS_PER_GROUP), 0, st, table_dev, B, rows, frames_dev,
                       scan_dev);
    HIP_TRY(hipGetLastError());
    return HPE_OK;
}

}  // extern "C"
#pragma GCC visibility pop
