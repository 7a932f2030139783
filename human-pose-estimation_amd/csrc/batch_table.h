// batch_table.h -- what the batched image kernels (jpeg_decode, jpeg_encode, png_decode, png_encode) share on the device: every launch
// runs over the workgroups (or rows) of a whole batch, and every table entry carries the prefix sum of the units before its image.
#pragma once

#include <hip/hip_runtime.h>

// The last image whose base `Member` is <= unit, e.g. find_image<&HpeJpegImage::store_group0>(table, B, (int)blockIdx.x).  The host
// checked that the bases are the prefix sums in batch order; images without a unit share their base with the next image and are
// stepped over.
template <auto Member, class Entry, class Unit>
__device__ __forceinline__ int find_image(const Entry* __restrict__ table, int B, Unit unit) {
    int lo = 0, hi = B - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[mid].*Member <= unit)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}
