// jpeg_huffman_enc.hip -- the serial half of the JPEG encoder (DESIGN.md "Dataset writers and JPEG encode"): the layout of a batch, the
// marker segments and the Huffman coder, on the host, where a bit stream belongs.  Plain C++17: nothing of HIP is included, so this file
// also builds with a host compiler (tools/jpeg_enc_host_check.cpp runs it under the address and undefined-behaviour sanitizers).
//
// Scope: what libjpeg's default baseline compressor writes -- JFIF 1.01, 8-bit tables scaled from Annex K by `quality`, SOF0 with
// component ids 1, 2, 3, the Annex K.3-K.6 Huffman tables, one interleaved scan, no restart markers.  Every write goes through Out,
// which holds it against the end of the image's own region; every coefficient read lies in a plane that the entry check held against
// coef_count.
#include <climits>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "jpeg.h"

namespace {

using jpeg::at_image;
using jpeg::refuse;
using jpeg::ZIGZAG;

// Annex K.1, K.2 in natural order
const unsigned char BASE_Q[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

// Annex K.3 - K.6: counts of the codes of length 1..16, then the symbols in code order
const unsigned char DC_COUNTS[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
const unsigned char DC_VALS[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const unsigned char AC_COUNTS[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
const unsigned char AC_VALS[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
     0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
     0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
     0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
     0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
     0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
     0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
     0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
     0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
     0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
     0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
     0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
     0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa}};

// symbol -> code and length (0: the table has no code for it)
struct Codes {
    unsigned short code[256];
    unsigned char len[256];
};

struct Tables {
    Codes dc[2], ac[2];
    Tables() {
        for (int t = 0; t < 2; ++t) {
            fill(&dc[t], DC_COUNTS[t], DC_VALS);
            fill(&ac[t], AC_COUNTS[t], AC_VALS[t]);
        }
    }
    static void fill(Codes* c, const unsigned char* counts, const unsigned char* vals) {
        std::memset(c, 0, sizeof(*c));
        unsigned code = 0;
        int k = 0;
        for (int l = 1; l <= 16; ++l) {
            for (int i = 0; i < counts[l - 1]; ++i, ++k, ++code) {
                c->code[vals[k]] = (unsigned short)code;
                c->len[vals[k]] = (unsigned char)l;
            }
            code <<= 1;
        }
    }
};

const Tables& tables() {
    static const Tables t;
    return t;
}

// the image's own region of the caller's buffer: a write past its end is dropped and remembered
struct Out {
    unsigned char* p;
    long long pos, end;
    bool ok = true;
    void u8(int b) {
        if (pos < end)
            p[pos++] = (unsigned char)b;
        else
            ok = false;
    }
    void u16(int v) {
        u8(v >> 8);
        u8(v & 0xFF);
    }
    void bytes(const unsigned char* s, int n) {
        for (int i = 0; i < n; ++i) u8(s[i]);
    }
    void segment(int marker, int body) {  // the marker and the length of a segment whose body follows
        u8(0xFF);
        u8(marker);
        u16(body + 2);
    }
};

struct BitOut {
    Out* o;
    uint64_t acc = 0;  // the low n bits wait for their byte
    int n = 0;
    void put(unsigned code, int len) {  // len in [0, 16]
        acc = (acc << len) | code;
        n += len;
        while (n >= 8) {
            const int b = (int)((acc >> (n - 8)) & 0xFF);
            o->u8(b);
            if (b == 0xFF) o->u8(0);
            n -= 8;
        }
    }
    void flush() {
        if (n) put((1u << (8 - n)) - 1u, 8 - n);
    }
};

inline int category(int v) {
    unsigned a = (unsigned)(v < 0 ? -v : v);
    int s = 0;
    while (a) {
        ++s;
        a >>= 1;
    }
    return s;
}

void write_header(Out* o, const HpeJpegEncImage& e, int units, int xd, int yd) {
    o->u8(0xFF);
    o->u8(0xD8);
    o->segment(0xE0, 14);
    o->bytes(reinterpret_cast<const unsigned char*>("JFIF"), 5);
    o->u8(1);
    o->u8(1);
    o->u8(units);
    o->u16(xd);
    o->u16(yd);
    o->u8(0);
    o->u8(0);
    const int ntab = e.C == 3 ? 2 : 1;
    for (int t = 0; t < ntab; ++t) {
        o->segment(0xDB, 65);
        o->u8(t);
        for (int i = 0; i < 64; ++i) o->u8(e.quant[t][ZIGZAG[i]]);
    }
    o->segment(0xC0, 6 + 3 * e.C);
    o->u8(8);
    o->u16(e.H);
    o->u16(e.W);
    o->u8(e.C);
    for (int c = 0; c < e.C; ++c) {
        o->u8(c + 1);
        o->u8(c ? 0x11 : (e.hmax << 4 | e.vmax));
        o->u8(c ? 1 : 0);
    }
    for (int t = 0; t < ntab; ++t) {
        o->segment(0xC4, 17 + 12);
        o->u8(t);
        o->bytes(DC_COUNTS[t], 16);
        o->bytes(DC_VALS, 12);
        o->segment(0xC4, 17 + 162);
        o->u8(0x10 | t);
        o->bytes(AC_COUNTS[t], 16);
        o->bytes(AC_VALS[t], 162);
    }
    o->segment(0xDA, 4 + 2 * e.C);
    o->u8(e.C);
    for (int c = 0; c < e.C; ++c) {
        o->u8(c + 1);
        o->u8(c ? 0x11 : 0x00);
    }
    o->u8(0);
    o->u8(63);
    o->u8(0);
}

// One block.  false: a value the standard tables have no code for.
bool encode_block(BitOut* bo, const Codes& dc, const Codes& ac, const short* blk, int* pred) {
    const int diff = (int)blk[0] - *pred;
    *pred = blk[0];
    int s = category(diff);
    if (s > 11) return false;
    bo->put(dc.code[s], dc.len[s]);
    if (s) bo->put((unsigned)(diff < 0 ? diff + (1 << s) - 1 : diff), s);
    int run = 0;
    for (int k = 1; k < 64; ++k) {
        const int v = blk[ZIGZAG[k]];
        if (v == 0) {
            ++run;
            continue;
        }
        for (; run > 15; run -= 16) bo->put(ac.code[0xF0], ac.len[0xF0]);
        s = category(v);
        if (s > 10) return false;
        bo->put(ac.code[run << 4 | s], ac.len[run << 4 | s]);
        bo->put((unsigned)(v < 0 ? v + (1 << s) - 1 : v), s);
        run = 0;
    }
    if (run) bo->put(ac.code[0], ac.len[0]);
    return true;
}

bool encode_image(const HpeJpegEncImage& e, const short* coef, int units, int xd, int yd, Out* o, std::string* why) {
    write_header(o, e, units, xd, yd);
    const Tables& T = tables();
    BitOut bo{o};
    const int mcus_x = e.blocks_w[0] / e.hmax, mcus_y = e.blocks_h[0] / e.vmax;
    int pred[3] = {0, 0, 0};
    for (int my = 0; my < mcus_y; ++my)
        for (int mx = 0; mx < mcus_x; ++mx)
            for (int c = 0; c < e.C; ++c) {
                const int h = c ? 1 : e.hmax, v = c ? 1 : e.vmax, t = c ? 1 : 0;
                for (int dy = 0; dy < v; ++dy)
                    for (int dx = 0; dx < h; ++dx) {
                        const long long blk = (long long)(my * v + dy) * e.blocks_w[c] + mx * h + dx;
                        if (!encode_block(&bo, T.dc[t], T.ac[t], coef + e.coef_offset[c] + 64 * blk, &pred[c]))
                            return refuse(why, "a coefficient the standard Huffman tables cannot code (|AC| > 1023 or |DC difference| > 2047)");
                    }
            }
    bo.flush();
    o->u8(0xFF);
    o->u8(0xD9);
    if (!o->ok) return refuse(why, "the stream does not fit its bound");  // cannot happen with a table that passed the entry check
    return true;
}

}  // namespace

namespace jpeg {

const char* enc_entry_fault(const HpeJpegEncImage& e) {
    if (e.C != 1 && e.C != 3) return "C must be 1 or 3";
    if (e.H < 1 || e.W < 1 || e.H > HPE_JPEG_MAX_SIDE || e.W > HPE_JPEG_MAX_SIDE) return "H and W must be in [1, 16384]";
    const bool samp_ok = (e.hmax == 1 || e.hmax == 2) && (e.vmax == 1 || e.vmax == 2) && e.vmax <= e.hmax && (e.C == 3 || e.hmax == 1);
    if (!samp_ok) return "sampling must be 1x1, 2x1 or 2x2, and 1x1 for a grey frame";
    for (int c = 0; c < e.C; ++c) {
        const int h = c ? 1 : e.hmax, v = c ? 1 : e.vmax;
        if (e.blocks_w[c] != blocks_for(e.W, e.hmax, h) || e.blocks_h[c] != blocks_for(e.H, e.vmax, v))
            return "the block grid is not that of H, W and the sampling";
        const int rw = ((e.W * h + e.hmax - 1) / e.hmax + 7) / 8, rh = ((e.H * v + e.vmax - 1) / e.vmax + 7) / 8;
        if (e.real_w[c] != rw || e.real_h[c] != rh) return "the real block grid is not that of H, W and the sampling";
        if (e.coef_offset[c] < 0 || (e.coef_offset[c] & 7)) return "a coefficient plane off an 8-element boundary";
    }
    for (int t = 0; t < 2; ++t)
        for (int i = 0; i < 64; ++i)
            if (e.quant[t][i] == 0) return "a quantisation table entry of 0";
    return "";
}

int encode_layout(int B, const int* shapes, const long long* frame_offsets, int hmax, int vmax, int quality, HpeJpegEncImage* table_out,
                  long long* totals_out, std::string* why) {
    if (!shapes || !frame_offsets || !table_out || !totals_out) return refuse(why, "null argument"), HPE_ERR_INVALID;
    if (B < 1) return refuse(why, "B must be >= 1"), HPE_ERR_INVALID;
    if (quality < 1 || quality > 100) return refuse(why, "quality must be in [1, 100]"), HPE_ERR_INVALID;
    if (!((hmax == 1 && vmax == 1) || (hmax == 2 && vmax == 1) || (hmax == 2 && vmax == 2)))
        return refuse(why, "sampling must be 1x1 (4:4:4), 2x1 (4:2:2) or 2x2 (4:2:0)"), HPE_ERR_INVALID;
    unsigned char quant[2][64];
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int t = 0; t < 2; ++t)
        for (int i = 0; i < 64; ++i) {
            const int q = (BASE_Q[t][i] * scale + 50) / 100;
            quant[t][i] = (unsigned char)(q < 1 ? 1 : q > 255 ? 255 : q);
        }
    long long coefs = 0, groups = 0, bound = 0;
    for (int b = 0; b < B; ++b) {
        const int H = shapes[3 * b], W = shapes[3 * b + 1], C = shapes[3 * b + 2];
        if (C != 1 && C != 3) return refuse(why, at_image(b, std::to_string(C) + " channels: the channel count must be 1 or 3")), HPE_ERR_INVALID;
        if (H < 1 || W < 1) return refuse(why, at_image(b, "an empty side: " + std::to_string(H) + " x " + std::to_string(W) + " (H x W)")), HPE_ERR_INVALID;
        if (H > HPE_JPEG_MAX_SIDE || W > HPE_JPEG_MAX_SIDE)
            return refuse(why, at_image(b, "a side of " + std::to_string(H) + " x " + std::to_string(W) + " (H x W) is above 16384")), HPE_ERR_INVALID;
        if (frame_offsets[b] < 0) return refuse(why, at_image(b, "a negative frame offset")), HPE_ERR_INVALID;
        HpeJpegEncImage& e = table_out[b];
        std::memset(&e, 0, sizeof(e));
        e.frame_offset = frame_offsets[b];
        e.H = H;
        e.W = W;
        e.C = C;
        e.hmax = C == 3 ? hmax : 1;
        e.vmax = C == 3 ? vmax : 1;
        for (int c = 0; c < C; ++c) {
            const int h = c ? 1 : e.hmax, v = c ? 1 : e.vmax;
            e.blocks_w[c] = blocks_for(W, e.hmax, h);
            e.blocks_h[c] = blocks_for(H, e.vmax, v);
            e.real_w[c] = ((W * h + e.hmax - 1) / e.hmax + 7) / 8;
            e.real_h[c] = ((H * v + e.vmax - 1) / e.vmax + 7) / 8;
            e.coef_offset[c] = coefs;
            coefs += 64LL * e.blocks_w[c] * e.blocks_h[c];
        }
        std::memcpy(e.quant, quant, sizeof(quant));
        if (groups > INT_MAX) return refuse(why, "the batch needs more than 2^31 workgroups"), HPE_ERR_INVALID;
        e.group0 = (int)groups;
        groups += (enc_blocks(e) + IDCT_BLOCKS_PER_GROUP - 1) / IDCT_BLOCKS_PER_GROUP;
        bound += enc_stream_bound(e);
    }
    if (groups > INT_MAX) return refuse(why, "the batch needs more than 2^31 workgroups"), HPE_ERR_INVALID;
    totals_out[0] = coefs;
    totals_out[1] = groups;
    totals_out[2] = bound;
    return HPE_OK;
}

int entropy_encode(const HpeJpegEncImage* table, int B, const short* coef, long long coef_count, int units, int xdensity, int ydensity,
                   int threads, unsigned char* out, long long out_capacity, long long* offsets_out, long long* lengths_out, std::string* why) {
    if (!table || !coef || !out || !offsets_out || !lengths_out) return refuse(why, "null argument"), HPE_ERR_INVALID;
    if (B < 1) return refuse(why, "B must be >= 1"), HPE_ERR_INVALID;
    if (threads < 1 || threads > 16) return refuse(why, "threads must be in [1, 16]"), HPE_ERR_INVALID;
    if (units < 0 || units > 2 || xdensity < 1 || xdensity > 65535 || ydensity < 1 || ydensity > 65535)
        return refuse(why, "units must be 0, 1 or 2 and the densities in [1, 65535]"), HPE_ERR_INVALID;
    if (coef_count < 0 || out_capacity < 0) return refuse(why, "negative buffer size"), HPE_ERR_INVALID;
    long long bound = 0;
    for (int b = 0; b < B; ++b) {
        const HpeJpegEncImage& e = table[b];
        const char* fault = enc_entry_fault(e);
        if (fault[0]) return refuse(why, "table entry " + std::to_string(b) + ": " + fault), HPE_ERR_INVALID;
        for (int c = 0; c < e.C; ++c)
            if (e.coef_offset[c] > coef_count - 64LL * e.blocks_w[c] * e.blocks_h[c])
                return refuse(why, "table entry " + std::to_string(b) + ": coefficients outside the coefficient buffer"), HPE_ERR_INVALID;
        offsets_out[b] = bound;
        bound += enc_stream_bound(e);
    }
    if (bound > out_capacity)
        return refuse(why, "out_capacity " + std::to_string(out_capacity) + " is below the batch's bound " + std::to_string(bound)), HPE_ERR_INVALID;
    std::vector<std::string> whys((size_t)B);
    std::vector<char> bad((size_t)B, 0);
    for_each_image(B, threads, [&](int b) {
        Out o{out, offsets_out[b], offsets_out[b] + enc_stream_bound(table[b])};
        if (!encode_image(table[b], coef, units, xdensity, ydensity, &o, &whys[(size_t)b])) bad[(size_t)b] = 1;
        lengths_out[b] = bad[(size_t)b] ? 0 : o.pos - offsets_out[b];
    });
    for (int b = 0; b < B; ++b)
        if (bad[(size_t)b]) return refuse(why, at_image(b, whys[(size_t)b])), HPE_ERR_INVALID;
    return HPE_OK;
}

}  // namespace jpeg
