// jpeg_host_check.cpp -- stand-alone sanitizer run of the JPEG decoder's host half (csrc/jpeg_entropy.hip: plain C++17, no HIP).
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -pthread \
//       -x c++ human-pose-estimation_amd/csrc/jpeg_entropy.hip tools/jpeg_host_check.cpp -o /tmp/jpeg_host_check
//   /tmp/jpeg_host_check tests/golden/jpeg/*.jpg
//
// Over every file given: the info pass and the decode pass (3 channels and 1) into a heap buffer of exactly the reported size; every
// prefix of the stream, which must be refused; every single-byte change to 0x00 and to 0xFF in the first 700 bytes, which must return
// success or an error status; then all files as one batch with 1 and with 4 threads, whose coefficient and table bytes must agree.
// The sanitizers are the check: a read past a stream or a write past a buffer ends the program.  A CPU program, run by hand.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "../human-pose-estimation_amd/csrc/jpeg.h"

namespace {

typedef std::vector<unsigned char> Bytes;

// decode one stream into an exactly sized buffer; -> status
int decode_one(const Bytes& s, int channels, std::vector<short>* coef_out = nullptr) {
    // the stream itself in an exactly sized heap block, so a read past its end is seen
    unsigned char* copy = new unsigned char[s.size() ? s.size() : 1];
    if (!s.empty()) std::memcpy(copy, s.data(), s.size());
    const unsigned char* ptr = copy;
    const long long len = (long long)s.size();
    HpeJpegImage entry;
    int status = -1;
    long long totals[5];
    std::string why;
    int rc = jpeg::decode_batch(1, &ptr, &len, &channels, 1, nullptr, 0, &entry, &status, totals, &why);
    if (rc == HPE_OK) {
        std::vector<short> coef((size_t)totals[0]);
        rc = jpeg::decode_batch(1, &ptr, &len, &channels, 1, coef.data(), (long long)coef.size(), &entry, &status, totals, &why);
        if (rc == HPE_OK && coef_out) *coef_out = coef;
    }
    if ((rc == HPE_OK) != (status == HPE_OK) || (rc != HPE_OK && why.empty())) {
        std::fprintf(stderr, "status and return code disagree, or a refusal without a message\n");
        std::exit(2);
    }
    delete[] copy;
    return rc;
}

}  // namespace

int main(int argc, char** argv) {
    std::vector<Bytes> files;
    long long prefixes = 0, mutations = 0, mutated_ok = 0;
    for (int i = 1; i < argc; ++i) {
        std::ifstream f(argv[i], std::ios::binary);
        Bytes s((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        if (s.empty()) {
            std::fprintf(stderr, "%s: cannot read\n", argv[i]);
            return 2;
        }
        HpeJpegInfo info;
        std::string why;
        jpeg::stream_info(s.data(), (long long)s.size(), &info, &why);
        const int rc3 = decode_one(s, 3), rc1 = decode_one(s, 1);
        std::printf("%-40s %5zu bytes  info %d  decode %d %d  %s\n", argv[i], s.size(), info.status, rc3, rc1, why.c_str());
        if ((info.status == HPE_OK) != (rc3 == HPE_OK) || rc3 != rc1) {
            std::fprintf(stderr, "info and decode disagree\n");
            return 2;
        }
        for (size_t n = 0; n < s.size(); ++n, ++prefixes)
            if (decode_one(Bytes(s.begin(), s.begin() + (long)n), 3) == HPE_OK) {
                std::fprintf(stderr, "%s: the prefix of %zu bytes was accepted\n", argv[i], n);
                return 2;
            }
        for (size_t p = 0; p < s.size() && p < 700; ++p)
            for (int v = 0; v < 2; ++v, ++mutations) {
                Bytes m = s;
                m[p] = v ? 0xFF : 0x00;
                mutated_ok += decode_one(m, 3) == HPE_OK;
                decode_one(m, 1);
            }
        if (rc3 == HPE_OK) files.push_back(s);
    }
    if (!files.empty()) {
        const int B = (int)files.size();
        std::vector<const unsigned char*> ptrs;
        std::vector<long long> lens;
        std::vector<int> ch;
        for (int b = 0; b < B; ++b) {
            ptrs.push_back(files[b].data());
            lens.push_back((long long)files[b].size());
            ch.push_back(b % 2 ? 1 : 3);
        }
        std::vector<short> coef[2];
        std::vector<HpeJpegImage> table[2];
        for (int t = 0; t < 2; ++t) {
            std::vector<int> status((size_t)B);
            long long totals[5];
            std::string why;
            table[t].resize((size_t)B);
            if (jpeg::decode_batch(B, ptrs.data(), lens.data(), ch.data(), t ? 4 : 1, nullptr, 0, table[t].data(), status.data(), totals, &why) != HPE_OK) return 2;
            coef[t].assign((size_t)totals[0], (short)0x5A5A);
            if (jpeg::decode_batch(B, ptrs.data(), lens.data(), ch.data(), t ? 4 : 1, coef[t].data(), totals[0], table[t].data(), status.data(), totals, &why) != HPE_OK) return 2;
        }
        if (coef[0] != coef[1] || std::memcmp(table[0].data(), table[1].data(), sizeof(HpeJpegImage) * (size_t)B) != 0) {
            std::fprintf(stderr, "1 thread and 4 threads disagree\n");
            return 2;
        }
    }
    std::printf("%zu decodable files, %lld prefixes all refused, %lld single-byte changes (%lld still decodable), threads 1 == 4: clean\n", files.size(),
                prefixes, mutations, mutated_ok);
    return 0;
}
