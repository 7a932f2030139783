// png.h -- what hpe_png_backend (png_decode.hip) holds a table against before it launches: plain C++17 with nothing of HIP, so
// tools/png_host_check.cpp compiles it with a host compiler under the sanitizers.  The kernels take every loop bound from a table
// that passed this check (DESIGN.md "PNG streams in the records").
#pragma once

#include <string>

#include "../../include/hpe.h"

namespace png {

constexpr int STORE_BYTES_PER_GROUP = HPE_PNG_STORE_BYTES_PER_GROUP;
constexpr long long PALETTE_BYTES = 256 * 4;

// samples per pixel of a colour type; 0 = not a colour type
inline int samples_of(int color_type) {
    switch (color_type) {
        case 0: return 1;
        case 2: return 3;
        case 3: return 1;
        case 4: return 2;
        case 6: return 4;
        default: return 0;
    }
}

inline bool depth_allowed(int color_type, int depth) {
    if (depth == 8) return samples_of(color_type) != 0;
    return (depth == 1 || depth == 2 || depth == 4) && (color_type == 0 || color_type == 3);
}

// the unfiltered rows of such an image are its frame, byte for byte: launch one writes them into the frame buffer, launch two skips it
inline bool is_direct(int color_type, int depth, int channels) {
    return depth == 8 && ((color_type == 0 && channels == 1) || (color_type == 2 && channels == 3));
}

inline long long store_groups(const HpePngImage& e) {
    if (is_direct(e.color_type, e.depth, e.channels)) return 0;
    return ((long long)e.H * e.W * e.channels + STORE_BYTES_PER_GROUP - 1) / STORE_BYTES_PER_GROUP;
}

// "" = fine.  g2: the workgroup base the entry must carry.
inline const char* entry_fault(const HpePngImage& e, long long raw_bytes, long long workspace_bytes, long long frames_bytes, long long g2) {
    if (e.H < 1 || e.W < 1 || e.H > HPE_PNG_MAX_SIDE || e.W > HPE_PNG_MAX_SIDE) return "H and W must be in [1, 16384]";
    const int samples = samples_of(e.color_type);
    if (!samples) return "the colour type must be 0, 2, 3, 4 or 6";
    if (!depth_allowed(e.color_type, e.depth)) return "the depth must be 8, or 1, 2 or 4 for colour types 0 and 3";
    if (e.channels != 1 && e.channels != 3) return "channels must be 1 or 3";
    const long long bits = (long long)e.W * samples * e.depth;
    if (e.rowbytes != (bits + 7) / 8) return "rowbytes is not that of W, the colour type and the depth";
    const int bpp = samples * e.depth / 8;
    if (e.bpp != (bpp < 1 ? 1 : bpp)) return "bpp is not that of the colour type and the depth";
    const long long raw = (long long)e.H * (e.rowbytes + 1LL);
    if (e.raw_offset < 0 || (e.raw_offset & 15) || e.raw_offset > raw_bytes - raw) return "the scanlines lie outside the raw buffer or off a 16-byte boundary";
    if (e.color_type == 3) {
        if (e.pal_offset < 0 || (e.pal_offset & 15) || e.pal_offset > raw_bytes - PALETTE_BYTES)
            return "the palette lies outside the raw buffer or off a 16-byte boundary";
    } else if (e.pal_offset != -1) {
        return "pal_offset must be -1 without a palette";
    }
    if (is_direct(e.color_type, e.depth, e.channels)) {
        if (e.work_offset != -1) return "work_offset must be -1 for a direct image";
    } else {
        const long long rows = (long long)e.H * e.rowbytes;
        if (e.work_offset < 0 || (e.work_offset & 15) || e.work_offset > workspace_bytes - rows)
            return "the unfiltered rows lie outside the workspace or off a 16-byte boundary";
    }
    const long long bytes = (long long)e.H * e.W * e.channels;
    if (e.out_offset < 0 || (e.out_offset & 15) || e.out_offset > frames_bytes - bytes) return "the frame lies outside the frame buffer or off a 16-byte boundary";
    if (e.store_group0 != g2) return "the workgroup base is not the prefix sum of the images before";
    return "";
}

// The whole table: HPE_OK and *groups = the workgroups of launch two, *lds = the bytes of one row buffer for launch one; or
// HPE_ERR_INVALID with the message in *why.
inline int check_table(const HpePngImage* table, int B, long long raw_bytes, long long workspace_bytes, long long frames_bytes, long long* groups,
                       int* lds, std::string* why) {
    if (!table) return *why = "null argument", HPE_ERR_INVALID;
    if (B < 1) return *why = "B must be >= 1", HPE_ERR_INVALID;
    if (raw_bytes < 0 || workspace_bytes < 0 || frames_bytes < 0) return *why = "negative buffer size", HPE_ERR_INVALID;
    long long g2 = 0;
    int widest = 0;
    for (int b = 0; b < B; ++b) {
        const HpePngImage& e = table[b];
        const char* fault = entry_fault(e, raw_bytes, workspace_bytes, frames_bytes, g2);
        if (fault[0]) return *why = "table entry " + std::to_string(b) + ": " + fault, HPE_ERR_INVALID;
        g2 += store_groups(e);
        if (g2 > 0x7fffffffLL) return *why = "the batch needs more than 2^31 workgroups", HPE_ERR_INVALID;
        const int group = e.bpp == 3 ? 12 : 4;  // launch one moves whole groups of this many bytes through the row buffer
        const int need = (e.rowbytes + group - 1) / group * group;
        if (e.H > 64 && need > widest) widest = need;  // the row buffer joins the 64-row strips: one strip needs none
    }
    *groups = g2;
    *lds = (widest + 15) / 16 * 16;  // <= 16384 * 4 = 64 KB
    return HPE_OK;
}

}  // namespace png
