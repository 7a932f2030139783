// jpeg.h -- the host half of the JPEG decoder (jpeg_entropy.hip): marker parser, Huffman decoder and the packed layout of a batch.
// Plain C++17 with nothing of HIP, so jpeg_entropy.hip also compiles with a host compiler into tools/jpeg_host_check.cpp's sanitizer
// build.  The C ABI over it (hpe_jpeg_info, hpe_jpeg_decode) and the two launches live in jpeg_decode.hip.
#pragma once

#include <string>

#include "../../include/hpe.h"

namespace jpeg {

constexpr int IDCT_BLOCKS_PER_GROUP = 32;  // launch one: 8 threads per 8x8 block, 256 threads
constexpr int STORE_BYTES_PER_GROUP = 1024;  // launch two: 4 output bytes per thread, 256 threads

// Header of one stream -> info (status HPE_OK) or a refusal (status HPE_ERR_INVALID, every other field 0, the clause in *why).
void stream_info(const unsigned char* data, long long len, HpeJpegInfo* info, std::string* why);

// Both return HPE_OK or HPE_ERR_INVALID with the message in *why ("image <b>: <clause>" for a refused stream); the arguments are
// those of hpe_jpeg_info / hpe_jpeg_decode (include/hpe.h).
int info_batch(int B, const unsigned char* const* streams, const long long* lengths, HpeJpegInfo* info_out, std::string* why);
int decode_batch(int B, const unsigned char* const* streams, const long long* lengths, const int* channels, int threads, short* coef_out,
                 long long coef_capacity, HpeJpegImage* table_out, int* status_out, long long* totals_out, std::string* why);

// The block grid the layout gives a frame: what hpe_jpeg_backend holds every table entry against.
inline int blocks_for(int side, int smax, int s) { return (side + 8 * smax - 1) / (8 * smax) * s; }

}  // namespace jpeg
