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

// The host half of the encoder (jpeg_huffman_enc.hip), also plain C++17 (tools/jpeg_enc_host_check.cpp is its sanitizer build): the
// arguments are those of hpe_jpeg_encode_layout / hpe_jpeg_entropy_encode; HPE_OK, or HPE_ERR_INVALID with the message in *why.
int encode_layout(int B, const int* shapes, const long long* frame_offsets, int hmax, int vmax, int quality, HpeJpegEncImage* table_out,
                  long long* totals_out, std::string* why);
int entropy_encode(const HpeJpegEncImage* table, int B, const short* coef, long long coef_count, int units, int xdensity, int ydensity,
                   int threads, unsigned char* out, long long out_capacity, long long* offsets_out, long long* lengths_out, std::string* why);
// What hpe_jpeg_forward and entropy_encode hold a table entry against ("" = fine), but for the buffer sizes and the workgroup base.
const char* enc_entry_fault(const HpeJpegEncImage& e);
inline long long enc_blocks(const HpeJpegEncImage& e) {
    long long n = 0;
    for (int c = 0; c < e.C; ++c) n += (long long)e.blocks_w[c] * e.blocks_h[c];
    return n;
}
inline long long enc_stream_bound(const HpeJpegEncImage& e) { return HPE_JPEG_ENC_HEADER_BYTES + HPE_JPEG_ENC_BLOCK_BYTES * enc_blocks(e); }

// The block grid the layout gives a frame: what hpe_jpeg_backend holds every table entry against.
inline int blocks_for(int side, int smax, int s) { return (side + 8 * smax - 1) / (8 * smax) * s; }

}  // namespace jpeg
