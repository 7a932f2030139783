// jpeg.h -- the host half of the JPEG decoder (jpeg_entropy.hip): marker parser, Huffman decoder and the packed layout of a batch.
// Plain C++17 with nothing of HIP, so jpeg_entropy.hip also compiles with a host compiler into tools/jpeg_host_check.cpp's sanitizer
// build.  The C ABI over it (hpe_jpeg_info, hpe_jpeg_decode) and the two launches live in jpeg_decode.hip.
#pragma once

#include <atomic>
#include <string>
#include <thread>
#include <vector>

#include "../../include/hpe.h"

namespace jpeg {

// zigzag position -> natural order, shared by the entropy decoder and the entropy coder
inline constexpr unsigned char ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                             41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                             30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// a refusal: the clause into *why, false back
inline bool refuse(std::string* why, const std::string& clause) {
    if (why) *why = clause;
    return false;
}
inline std::string at_image(int b, const std::string& clause) { return "image " + std::to_string(b) + ": " + clause; }

// work(b) for every image of the batch on min(threads, B) threads; an atomic counter hands the images out
template <class Work>
void for_each_image(int B, int threads, Work work) {
    std::atomic<int> next(0);
    auto run = [&]() {
        for (int b = next.fetch_add(1); b < B; b = next.fetch_add(1)) work(b);
    };
    const int workers = threads < B ? threads : B;
    if (workers <= 1) return run();
    std::vector<std::thread> pool;
    for (int i = 0; i < workers; ++i) pool.emplace_back(run);
    for (auto& th : pool) th.join();
}

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
