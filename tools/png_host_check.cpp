// png_host_check.cpp -- stand-alone sanitizer run of the table check hpe_png_backend makes before it launches (csrc/png.h: plain C++17,
// no HIP).
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/png_host_check.cpp -o /tmp/png_host_check
//   /tmp/png_host_check
//
// Builds valid tables over every accepted colour type, depth and channel count at sides 1 .. 16384, each in an exactly sized heap block,
// which must pass; then damages every field of every entry with a set of values (offsets off their boundary and outside the buffers,
// sizes and kinds outside what is accepted, the extremes of the field's type), which must return HPE_OK or HPE_ERR_INVALID -- and
// HPE_ERR_INVALID with a message for every change that moves an extent outside its buffer; then shortens each buffer.  The sanitizers are
// the check: a read past the table or a signed overflow in the bounds arithmetic ends the program.  A CPU program, run by hand.
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../human-pose-estimation_amd/csrc/png.h"

namespace {

long long up16(long long n) { return (n + 15) / 16 * 16; }

struct Batch {
    std::vector<HpePngImage> table;
    long long raw = 0, work = 0, frames = 0, groups = 0;
};

// the layout hpe_amd/png.py writes: scanlines, then palettes; rows in the workspace; frames packed in order
Batch layout(const std::vector<HpePngImage>& shapes) {
    Batch b;
    for (HpePngImage e : shapes) {
        const int samples = png::samples_of(e.color_type);
        e.rowbytes = (int)(((long long)e.W * samples * e.depth + 7) / 8);
        e.bpp = samples * e.depth / 8 < 1 ? 1 : samples * e.depth / 8;
        e.raw_offset = b.raw;
        b.raw += up16((long long)e.H * (e.rowbytes + 1LL));
        e.out_offset = b.frames;
        b.frames += up16((long long)e.H * e.W * e.channels);
        e.store_group0 = (int)b.groups;
        e.pal_offset = -1;
        if (png::is_direct(e.color_type, e.depth, e.channels)) {
            e.work_offset = -1;
        } else {
            e.work_offset = b.work;
            b.work += up16((long long)e.H * e.rowbytes);
            b.groups += png::store_groups(e);
        }
        b.table.push_back(e);
    }
    for (HpePngImage& e : b.table)
        if (e.color_type == 3) {
            e.pal_offset = b.raw;
            b.raw += png::PALETTE_BYTES;
        }
    return b;
}

// the table in an exactly sized heap block, so a read past its end is seen
int check(const Batch& b, const std::vector<HpePngImage>& table, long long raw, long long work, long long frames, std::string* why) {
    HpePngImage* copy = new HpePngImage[table.size()];
    std::memcpy(copy, table.data(), table.size() * sizeof(HpePngImage));
    long long groups = -1;
    int lds = -1;
    why->clear();
    const int rc = png::check_table(copy, (int)table.size(), raw, work, frames, &groups, &lds, why);
    delete[] copy;
    if (rc != HPE_OK && rc != HPE_ERR_INVALID) std::exit(2);
    if (rc == HPE_ERR_INVALID && why->empty()) {
        std::fprintf(stderr, "a refusal without a message\n");
        std::exit(2);
    }
    if (rc == HPE_OK && ((&table == &b.table && groups != b.groups) || groups < 0 || lds < 0 || lds > 65536 || lds % 16)) {
        std::fprintf(stderr, "accepted, but groups %lld (want %lld) or lds %d is off\n", groups, b.groups, lds);
        std::exit(2);
    }
    return rc;
}

}  // namespace

int main() {
    const int kinds[][2] = {{0, 1}, {0, 2}, {0, 4}, {0, 8}, {2, 8}, {3, 1}, {3, 2}, {3, 4}, {3, 8}, {4, 8}, {6, 8}};
    const int sides[] = {1, 2, 3, 5, 9, 63, 64, 65, 67, 130, 1280, 16384};
    std::vector<HpePngImage> shapes;
    int k = 0;
    for (const auto& kd : kinds)
        for (int ch = 1; ch <= 3; ch += 2, ++k) {
            HpePngImage e{};
            e.color_type = kd[0], e.depth = kd[1], e.channels = ch;
            e.H = sides[k % 12], e.W = sides[(k * 5 + 3) % 12];
            shapes.push_back(e);
        }
    HpePngImage big{};  // the size cap: a 64 KB row, the whole LDS row buffer
    big.color_type = 6, big.depth = 8, big.channels = 3, big.H = 16384, big.W = 16384;
    shapes.push_back(big);
    const Batch b = layout(shapes);
    std::string why;
    if (check(b, b.table, b.raw, b.work, b.frames, &why) != HPE_OK) {
        std::fprintf(stderr, "the valid table was refused: %s\n", why.c_str());
        return 2;
    }
    const long long ll[] = {LLONG_MIN, LLONG_MIN + 1, -17, -16, -1, 0, 1, 4, 8, 15, 16, b.raw, b.work, b.frames, b.raw - 16, b.frames - 16,
                            (1LL << 31), (1LL << 40), LLONG_MAX - 15, LLONG_MAX};
    const int in[] = {INT_MIN, -1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 16, 63, 64, 65, 255, 256, 16384, 16385, 65536, 65537, INT_MAX - 1, INT_MAX};
    long long tried = 0, refused = 0;
    for (size_t i = 0; i < b.table.size(); ++i) {
        for (int f = 0; f < 4; ++f)
            for (long long v : ll) {
                std::vector<HpePngImage> t = b.table;
                long long* field = f == 0 ? &t[i].raw_offset : f == 1 ? &t[i].pal_offset : f == 2 ? &t[i].work_offset : &t[i].out_offset;
                if (*field == v) continue;
                const long long extent = f == 0 ? (long long)t[i].H * (t[i].rowbytes + 1LL) : f == 1 ? png::PALETTE_BYTES
                                         : f == 2 ? (long long)t[i].H * t[i].rowbytes : (long long)t[i].H * t[i].W * t[i].channels;
                const long long size = f < 2 ? b.raw : f == 2 ? b.work : b.frames;
                *field = v;
                const int rc = check(b, t, b.raw, b.work, b.frames, &why);
                ++tried, refused += rc != HPE_OK;
                const bool used = f == 0 || f == 3 || (f == 1 && t[i].color_type == 3) || (f == 2 && b.table[i].work_offset >= 0);
                if (rc == HPE_OK && (!used || v < 0 || (v & 15) || v > size - extent)) {
                    std::fprintf(stderr, "entry %zu: offset field %d = %lld was accepted\n", i, f, v);
                    return 2;
                }
            }
        for (int f = 0; f < 8; ++f)
            for (int v : in) {
                std::vector<HpePngImage> t = b.table;
                int* field = f == 0 ? &t[i].H : f == 1 ? &t[i].W : f == 2 ? &t[i].color_type : f == 3 ? &t[i].depth : f == 4 ? &t[i].channels
                             : f == 5 ? &t[i].rowbytes : f == 6 ? &t[i].bpp : &t[i].store_group0;
                if (*field == v) continue;
                *field = v;
                const int rc = check(b, t, b.raw, b.work, b.frames, &why);
                ++tried, refused += rc != HPE_OK;
                if (rc == HPE_OK && f >= 5) {  // rowbytes, bpp and the prefix sums are implied by the rest: any other value must go
                    std::fprintf(stderr, "entry %zu: int field %d = %d was accepted\n", i, f, v);
                    return 2;
                }
            }
    }
    // short buffers: each one byte, 16 bytes and wholly too small
    for (int which = 0; which < 3; ++which)
        for (long long cut : {1LL, 16LL, 1LL << 62}) {
            long long raw = b.raw, work = b.work, frames = b.frames;
            long long& s = which == 0 ? raw : which == 1 ? work : frames;
            s = cut > s ? 0 : s - cut;
            const int rc = check(b, b.table, raw, work, frames, &why);
            ++tried, refused += rc != HPE_OK;
            if (rc == HPE_OK && (which == 0 || cut >= 16)) {  // work and frames end in up to 15 bytes of padding
                std::fprintf(stderr, "buffer %d shortened by %lld was accepted\n", which, cut);
                return 2;
            }
        }
    if (check(b, b.table, -1, b.work, b.frames, &why) == HPE_OK) return 2;
    std::printf("%zu entries valid; %lld damaged tables and short buffers, %lld refused, the rest still in bounds: clean\n", b.table.size(), tried, refused);
    return 0;
}
