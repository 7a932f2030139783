// jpeg_entropy.hip -- the serial half of the JPEG decoder (DESIGN.md "Training records and JPEG decode"): marker parser, Huffman
// decoder and the packed layout of a batch, on the host, where a bit stream belongs.  Plain C++17: nothing of HIP is included, so this
// file also builds with a host compiler (tools/jpeg_host_check.cpp runs it under the address and undefined-behaviour sanitizers).
//
// Scope: baseline sequential DCT (SOF0), 8-bit samples and quantisation tables, 1 or 3 components, luma 1x1 / 2x1 / 2x2 with 1x1
// chroma, one interleaved scan, DRI / RST0-7, any DHT.  Everything else is refused with a clause; nothing is decoded "as far as it goes".
// Every read is checked against the stream length (Reader, Bits), every coefficient index against 63, and every write lands in the
// image's own region of the coefficient buffer, whose end decode_batch holds against the caller's capacity before anything is written.
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

struct Huff {
    bool defined = false;
    int nvals = 0;
    unsigned char vals[256];
    int maxcode[17];           // largest code of length l, -1 if there is none
    int valoff[17];            // vals index of a code of length l = code + valoff[l]
    unsigned short look[256];  // first 8 bits -> (length << 8) | symbol for codes of at most 8 bits, 0 otherwise
};

struct Header {
    int H = 0, W = 0, ncomp = 0;
    int id[3], hs[3], vs[3], tq[3], td[3], ta[3];
    unsigned char quant[4][64];  // natural order
    bool qdef[4] = {false, false, false, false};
    Huff dc[4], ac[4];
    int restart = 0;
    long long scan_pos = 0;  // first byte of the entropy-coded data
};

// bounds-checked big-endian reads of the marker segments
struct Reader {
    const unsigned char* p;
    long long len, pos;
    bool u8(int* v) {
        if (pos >= len) return false;
        *v = p[pos++];
        return true;
    }
    bool u16(int* v) {
        if (len - pos < 2) return false;
        *v = (p[pos] << 8) | p[pos + 1];
        pos += 2;
        return true;
    }
};

bool build_huff(Huff* h, const unsigned char* counts /* [16] */, const unsigned char* vals, int nvals) {
    h->nvals = nvals;
    std::memcpy(h->vals, vals, (size_t)nvals);
    std::memset(h->look, 0, sizeof(h->look));
    int code = 0, k = 0;
    h->maxcode[0] = -1;
    h->valoff[0] = 0;
    for (int l = 1; l <= 16; ++l) {
        const int n = counts[l - 1];
        h->valoff[l] = k - code;
        if (l <= 8)
            for (int i = 0; i < n; ++i) {
                const int first = (code + i) << (8 - l);
                if (first + (1 << (8 - l)) > 256) return false;
                for (int j = 0; j < (1 << (8 - l)); ++j) h->look[first + j] = (unsigned short)((l << 8) | vals[k + i]);
            }
        k += n;
        code += n;
        if (code >= (1 << l) && n > 0) return false;  // libjpeg's rule: the codes of one length must leave the all-ones code free
        if (code > (1 << l)) return false;
        h->maxcode[l] = n ? code - 1 : -1;
        code <<= 1;
    }
    h->defined = true;
    return true;
}

// Markers up to and including SOS.  false = refused, the clause in *why.
bool parse_header(const unsigned char* data, long long len, Header* hd, std::string* why) {
    if (!data || len < 2 || data[0] != 0xFF || data[1] != 0xD8) return refuse(why, "no SOI marker: not a JPEG stream");
    Reader r{data, len, 2};
    bool have_sof = false, jfif = false, adobe = false;
    int adobe_transform = -1;
    for (;;) {
        int b;
        if (!r.u8(&b)) return refuse(why, "the stream ends before the scan");
        if (b != 0xFF) return refuse(why, "a marker was expected");
        do {  // 0xFF fill bytes
            if (!r.u8(&b)) return refuse(why, "the stream ends before the scan");
        } while (b == 0xFF);
        const int m = b;
        if (m == 0xD8) return refuse(why, "a second SOI marker");
        if (m == 0xD9) return refuse(why, "EOI before any scan");
        if (m == 0x00 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) return refuse(why, "a marker that cannot stand before the scan");
        int L;
        if (!r.u16(&L) || L < 2 || len - r.pos < L - 2) return refuse(why, "a marker segment runs past the end of the stream");
        const long long seg_end = r.pos + (L - 2);
        Reader s{data, seg_end, r.pos};
        if (m == 0xC0) {
            if (have_sof) return refuse(why, "a second frame header");
            int prec, nc;
            if (!s.u8(&prec) || !s.u16(&hd->H) || !s.u16(&hd->W) || !s.u8(&nc)) return refuse(why, "SOF0 is too short");
            if (prec != 8) return refuse(why, "only 8-bit samples are decoded");
            if (hd->H == 0) return refuse(why, "zero height (DNL streams are not decoded)");
            if (hd->W == 0) return refuse(why, "zero width");
            if (hd->H > HPE_JPEG_MAX_SIDE || hd->W > HPE_JPEG_MAX_SIDE) return refuse(why, "a side above 16384 pixels");
            if (nc != 1 && nc != 3) return refuse(why, "only 1 or 3 components are decoded");
            hd->ncomp = nc;
            for (int c = 0; c < nc; ++c) {
                int hv;
                if (!s.u8(&hd->id[c]) || !s.u8(&hv) || !s.u8(&hd->tq[c])) return refuse(why, "SOF0 is too short");
                hd->hs[c] = hv >> 4;
                hd->vs[c] = hv & 15;
                if (hd->tq[c] > 3) return refuse(why, "a quantisation table index above 3");
                for (int o = 0; o < c; ++o)
                    if (hd->id[o] == hd->id[c]) return refuse(why, "two components share an id");
            }
            if (s.pos != seg_end) return refuse(why, "SOF0 has a wrong length");
            if (nc == 1) {
                if (hd->hs[0] < 1 || hd->hs[0] > 4 || hd->vs[0] < 1 || hd->vs[0] > 4) return refuse(why, "sampling factors outside 1..4");
                hd->hs[0] = hd->vs[0] = 1;  // a single-component scan is not interleaved: its MCU is one block whatever the factors say
            } else {
                const bool luma_ok = (hd->hs[0] == 1 && hd->vs[0] == 1) || (hd->hs[0] == 2 && hd->vs[0] == 1) || (hd->hs[0] == 2 && hd->vs[0] == 2);
                if (!luma_ok || hd->hs[1] != 1 || hd->vs[1] != 1 || hd->hs[2] != 1 || hd->vs[2] != 1)
                    return refuse(why, "sampling other than luma 1x1, 2x1 or 2x2 with 1x1 chroma");
            }
            have_sof = true;
        } else if (m == 0xC4) {
            while (s.pos < seg_end) {
                int tc_th;
                if (!s.u8(&tc_th)) return refuse(why, "DHT is too short");
                const int tc = tc_th >> 4, th = tc_th & 15;
                if (tc > 1 || th > 3) return refuse(why, "a Huffman table class above 1 or index above 3");
                if (seg_end - s.pos < 16) return refuse(why, "DHT is too short");
                const unsigned char* counts = data + s.pos;
                s.pos += 16;
                int n = 0;
                for (int i = 0; i < 16; ++i) n += counts[i];
                if (n > 256 || seg_end - s.pos < n) return refuse(why, "DHT declares more symbols than it holds");
                Huff* h = tc ? &hd->ac[th] : &hd->dc[th];
                if (!build_huff(h, counts, data + s.pos, n)) return refuse(why, "DHT code lengths do not form a prefix code");
                s.pos += n;
            }
        } else if (m == 0xDB) {
            while (s.pos < seg_end) {
                int pq_tq;
                if (!s.u8(&pq_tq)) return refuse(why, "DQT is too short");
                if (pq_tq >> 4) return refuse(why, "16-bit quantisation tables are not decoded");
                const int t = pq_tq & 15;
                if (t > 3) return refuse(why, "a quantisation table index above 3");
                if (seg_end - s.pos < 64) return refuse(why, "DQT is too short");
                for (int i = 0; i < 64; ++i) hd->quant[t][ZIGZAG[i]] = data[s.pos + i];
                s.pos += 64;
                hd->qdef[t] = true;
            }
        } else if (m == 0xDD) {
            if (L != 4 || !s.u16(&hd->restart)) return refuse(why, "DRI has a wrong length");
        } else if (m == 0xDA) {
            if (!have_sof) return refuse(why, "SOS before the frame header");
            int ns;
            if (!s.u8(&ns)) return refuse(why, "SOS is too short");
            if (ns != hd->ncomp) return refuse(why, "several scans: only one interleaved scan is decoded");
            for (int c = 0; c < ns; ++c) {
                int cs, tt;
                if (!s.u8(&cs) || !s.u8(&tt)) return refuse(why, "SOS is too short");
                if (cs != hd->id[c]) return refuse(why, "the scan's components are not the frame's, in its order");
                hd->td[c] = tt >> 4;
                hd->ta[c] = tt & 15;
                if (hd->td[c] > 3 || hd->ta[c] > 3) return refuse(why, "a Huffman table index above 3");
                if (!hd->dc[hd->td[c]].defined || !hd->ac[hd->ta[c]].defined) return refuse(why, "the scan uses a Huffman table that was not defined");
                if (!hd->qdef[hd->tq[c]]) return refuse(why, "the frame uses a quantisation table that was not defined");
                const Huff& d = hd->dc[hd->td[c]];
                for (int i = 0; i < d.nvals; ++i)
                    if (d.vals[i] > 15) return refuse(why, "a DC Huffman table holds a category above 15");
            }
            int ss, se, ahl;
            if (!s.u8(&ss) || !s.u8(&se) || !s.u8(&ahl) || s.pos != seg_end) return refuse(why, "SOS has a wrong length");
            if (ss != 0 || se != 63 || ahl != 0) return refuse(why, "spectral selection or successive approximation: not a baseline scan");
            if (hd->ncomp == 3) {
                if (adobe && adobe_transform == 0) return refuse(why, "Adobe transform 0 (RGB or CMYK data) is not decoded");
                if (!jfif && !adobe && hd->id[0] == 'R' && hd->id[1] == 'G' && hd->id[2] == 'B') return refuse(why, "RGB component ids: not YCbCr data");
            }
            hd->scan_pos = seg_end;
            return true;
        } else if (m == 0xC8 || m == 0xCC) {
            return refuse(why, "arithmetic coding is not decoded");
        } else if (m == 0xC2) {
            return refuse(why, "progressive streams are not decoded (SOF2)");
        } else if (m >= 0xC1 && m <= 0xCF) {
            return refuse(why, "only baseline sequential DCT (SOF0) is decoded");
        } else if (m == 0xDC) {
            return refuse(why, "DNL is not decoded");
        } else if (m == 0xE0) {
            if (L >= 7 && std::memcmp(data + r.pos, "JFIF", 5) == 0) jfif = true;
        } else if (m == 0xEE) {
            if (L >= 14 && std::memcmp(data + r.pos, "Adobe", 5) == 0) {
                adobe = true;
                adobe_transform = data[r.pos + 11];
            }
        } else if ((m >= 0xE1 && m <= 0xEF) || m == 0xFE || (m >= 0xF0 && m <= 0xFD)) {
            // APPn, COM, JPGn: skipped
        } else {
            return refuse(why, "an unknown marker");
        }
        r.pos = seg_end;
    }
}

void fill_info(const Header& hd, HpeJpegInfo* info) {
    std::memset(info, 0, sizeof(*info));
    info->status = HPE_OK;
    info->H = hd.H;
    info->W = hd.W;
    info->ncomp = hd.ncomp;
    for (int c = 0; c < hd.ncomp; ++c) {
        info->hs[c] = hd.hs[c];
        info->vs[c] = hd.vs[c];
        info->blocks_w[c] = jpeg::blocks_for(hd.W, hd.hs[0], hd.hs[c]);
        info->blocks_h[c] = jpeg::blocks_for(hd.H, hd.vs[0], hd.vs[c]);
        info->coefs += 64LL * info->blocks_w[c] * info->blocks_h[c];
    }
}

// the entropy-coded segment as a bit stream: 0xFF00 is a data byte 0xFF, any other 0xFFxx ends the data (marker = xx)
struct Bits {
    const unsigned char* p;
    long long pos, end;
    uint64_t acc = 0;  // the low n bits are valid
    int n = 0;
    int marker = 0;
    bool eof = false;
    void fill() {
        while (n <= 56 && !marker && !eof) {
            if (pos >= end) {
                eof = true;
                break;
            }
            const int b = p[pos++];
            if (b == 0xFF) {
                while (pos < end && p[pos] == 0xFF) ++pos;
                if (pos >= end) {
                    eof = true;
                    break;
                }
                const int b2 = p[pos++];
                if (b2 != 0) {
                    marker = b2;
                    break;
                }
            }
            acc = (acc << 8) | (uint64_t)b;
            n += 8;
        }
    }
    // s in [1, 16]
    bool get(int s, int* v) {
        if (n < s) fill();
        if (n < s) return false;
        *v = (int)((acc >> (n - s)) & ((1u << s) - 1u));
        n -= s;
        return true;
    }
    // -1: the code is not in the table, or the data ends inside it
    int decode(const Huff& h) {
        if (n < 16) fill();
        const int first = n >= 8 ? (int)((acc >> (n - 8)) & 0xFF) : (int)((acc << (8 - n)) & 0xFF);
        const int e = h.look[first];
        if (e) {
            const int l = e >> 8;
            if (l > n) return -1;
            n -= l;
            return e & 0xFF;
        }
        for (int l = 9; l <= 16; ++l) {
            if (n < l) return -1;
            const int code = (int)((acc >> (n - l)) & ((1u << l) - 1u));
            if (h.maxcode[l] >= 0 && code <= h.maxcode[l]) {
                const int idx = code + h.valoff[l];
                if (idx < 0 || idx >= h.nvals) return -1;
                n -= l;
                return h.vals[idx];
            }
        }
        return -1;
    }
};

inline int extend(int v, int s) { return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

// One block into out[64] (natural order; zero on entry).  pred is the component's DC predictor.
bool decode_block(Bits* bs, const Huff& dc, const Huff& ac, int* pred, short* out, std::string* why) {
    const int s = bs->decode(dc);
    if (s < 0) return refuse(why, "a Huffman code that is not in the DC table, or the data ends early");
    int diff = 0;
    if (s) {
        if (s > 15) return refuse(why, "a DC category above 15");
        int v;
        if (!bs->get(s, &v)) return refuse(why, "the entropy-coded data ends early");
        diff = extend(v, s);
    }
    *pred = (int)((unsigned)*pred + (unsigned)diff);  // a corrupt stream wraps
    out[0] = (short)(unsigned short)((unsigned)*pred & 0xFFFFu);
    for (int k = 1; k < 64;) {
        const int rs = bs->decode(ac);
        if (rs < 0) return refuse(why, "a Huffman code that is not in the AC table, or the data ends early");
        const int run = rs >> 4, size = rs & 15;
        if (size == 0) {
            if (run != 15) break;  // EOB
            k += 16;
            continue;
        }
        k += run;
        if (k > 63) return refuse(why, "a coefficient index above 63");
        int v;
        if (!bs->get(size, &v)) return refuse(why, "the entropy-coded data ends early");
        out[ZIGZAG[k]] = (short)extend(v, size);
        ++k;
    }
    return true;
}

// The scan of one stream into its coefficient planes (zeroed here).  stored = 1 keeps Y alone.
bool decode_scan(const unsigned char* data, long long len, const Header& hd, const HpeJpegImage& e, short* coef, std::string* why) {
    for (int c = 0; c < e.ncomp; ++c)
        std::memset(coef + e.coef_offset[c], 0, sizeof(short) * 64 * (size_t)e.blocks_w[c] * (size_t)e.blocks_h[c]);
    Bits bs{data, hd.scan_pos, len};
    const int mcus_x = jpeg::blocks_for(hd.W, hd.hs[0], 1), mcus_y = jpeg::blocks_for(hd.H, hd.vs[0], 1);
    int pred[3] = {0, 0, 0};
    int next_rst = 0;
    long long mcu = 0;
    short dropped[64];
    for (int my = 0; my < mcus_y; ++my)
        for (int mx = 0; mx < mcus_x; ++mx, ++mcu) {
            if (hd.restart && mcu > 0 && mcu % hd.restart == 0) {
                bs.n = 0;  // the padding bits of the interval
                bs.acc = 0;
                if (!bs.marker) {
                    bs.fill();
                    if (bs.n > 0 || !bs.marker) return refuse(why, "a restart marker is missing");
                }
                if (bs.marker != 0xD0 + (next_rst & 7)) return refuse(why, "a wrong restart marker");
                bs.marker = 0;
                ++next_rst;
                pred[0] = pred[1] = pred[2] = 0;
            }
            for (int c = 0; c < hd.ncomp; ++c)
                for (int v = 0; v < hd.vs[c]; ++v)
                    for (int h = 0; h < hd.hs[c]; ++h) {
                        short* out = dropped;
                        if (c < e.ncomp) {
                            const long long by = (long long)my * hd.vs[c] + v, bx = (long long)mx * hd.hs[c] + h;
                            if (by >= e.blocks_h[c] || bx >= e.blocks_w[c]) return refuse(why, "a block outside the component's grid");
                            out = coef + e.coef_offset[c] + 64 * (by * e.blocks_w[c] + bx);
                        } else {
                            std::memset(dropped, 0, sizeof(dropped));
                        }
                        if (!decode_block(&bs, hd.dc[hd.td[c]], hd.ac[hd.ta[c]], &pred[c], out, why)) return false;
                    }
        }
    bs.n = 0;
    bs.acc = 0;
    if (!bs.marker) {
        bs.fill();
        if (bs.n > 0) return refuse(why, "data after the last MCU");
        if (!bs.marker) return refuse(why, "the stream ends without EOI");
    }
    if (bs.marker == 0xDA) return refuse(why, "several scans: only one interleaved scan is decoded");
    if (bs.marker == 0xDC) return refuse(why, "DNL is not decoded");
    if (bs.marker != 0xD9) return refuse(why, "a marker other than EOI after the scan");
    return true;
}

struct Totals {
    long long coef = 0, workspace = 0, frames = 0, idct_groups = 0, store_groups = 0;
};

// the table entry of one accepted stream, packed after what `t` already holds
bool layout_one(const HpeJpegInfo& in, int channels, Totals* t, HpeJpegImage* e) {
    std::memset(e, 0, sizeof(*e));
    e->H = in.H;
    e->W = in.W;
    e->channels = channels;
    e->ncomp = (in.ncomp == 3 && channels == 3) ? 3 : 1;
    e->hmax = in.hs[0];  // also when Y alone is stored: its plane keeps the stream's MCU grid
    e->vmax = in.vs[0];
    long long blocks = 0;
    for (int c = 0; c < e->ncomp; ++c) {
        e->blocks_w[c] = in.blocks_w[c];
        e->blocks_h[c] = in.blocks_h[c];
        const long long n = (long long)in.blocks_w[c] * in.blocks_h[c];
        e->coef_offset[c] = t->coef;
        e->plane_offset[c] = t->workspace;
        t->coef += 64 * n;
        t->workspace += 64 * n;
        blocks += n;
    }
    const long long bytes = (long long)in.H * in.W * channels;
    e->out_offset = t->frames;
    t->frames += (bytes + 15) / 16 * 16;
    if (t->idct_groups > INT_MAX || t->store_groups > INT_MAX) return false;
    e->idct_group0 = (int)t->idct_groups;
    e->store_group0 = (int)t->store_groups;
    t->idct_groups += (blocks + jpeg::IDCT_BLOCKS_PER_GROUP - 1) / jpeg::IDCT_BLOCKS_PER_GROUP;
    t->store_groups += (bytes + jpeg::STORE_BYTES_PER_GROUP - 1) / jpeg::STORE_BYTES_PER_GROUP;
    return t->idct_groups <= INT_MAX && t->store_groups <= INT_MAX;
}

}  // namespace

namespace jpeg {

void stream_info(const unsigned char* data, long long len, HpeJpegInfo* info, std::string* why) {
    Header hd;
    if (parse_header(data, len, &hd, why)) {
        fill_info(hd, info);
    } else {
        std::memset(info, 0, sizeof(*info));
        info->status = HPE_ERR_INVALID;
    }
}

int info_batch(int B, const unsigned char* const* streams, const long long* lengths, HpeJpegInfo* info_out, std::string* why) {
    if (!streams || !lengths || !info_out) return refuse(why, "null argument"), HPE_ERR_INVALID;
    if (B < 1) return refuse(why, "B must be >= 1"), HPE_ERR_INVALID;
    int first = -1;
    for (int b = 0; b < B; ++b) {
        std::string w;
        if (!streams[b] || lengths[b] < 0) {
            std::memset(&info_out[b], 0, sizeof(HpeJpegInfo));
            info_out[b].status = HPE_ERR_INVALID;
            w = "a null stream or a negative length";
        } else {
            stream_info(streams[b], lengths[b], &info_out[b], &w);
        }
        if (info_out[b].status != HPE_OK && first < 0) {
            first = b;
            if (why) *why = at_image(b, w);
        }
    }
    return first < 0 ? HPE_OK : HPE_ERR_INVALID;
}

int decode_batch(int B, const unsigned char* const* streams, const long long* lengths, const int* channels, int threads, short* coef_out,
                 long long coef_capacity, HpeJpegImage* table_out, int* status_out, long long* totals_out, std::string* why) {
    if (!streams || !lengths || !channels || !table_out || !status_out || !totals_out) return refuse(why, "null argument"), HPE_ERR_INVALID;
    if (B < 1) return refuse(why, "B must be >= 1"), HPE_ERR_INVALID;
    if (threads < 1 || threads > 16) return refuse(why, "threads must be in [1, 16]"), HPE_ERR_INVALID;
    if (coef_out && coef_capacity < 0) return refuse(why, "negative coef_capacity"), HPE_ERR_INVALID;
    for (int b = 0; b < B; ++b)
        if (channels[b] != 1 && channels[b] != 3) {
            if (why) *why = at_image(b, "channels must be 1 or 3");
            return HPE_ERR_INVALID;
        }
    std::vector<Header> headers((size_t)B);
    std::vector<std::string> whys((size_t)B);
    Totals t;
    for (int b = 0; b < B; ++b) {
        std::memset(&table_out[b], 0, sizeof(HpeJpegImage));
        status_out[b] = HPE_ERR_INVALID;
        if (!streams[b] || lengths[b] < 0) {
            whys[b] = "a null stream or a negative length";
            continue;
        }
        if (!parse_header(streams[b], lengths[b], &headers[b], &whys[b])) continue;
        HpeJpegInfo info;
        fill_info(headers[b], &info);
        if (!layout_one(info, channels[b], &t, &table_out[b])) return refuse(why, "the batch needs more than 2^31 workgroups"), HPE_ERR_INVALID;
        status_out[b] = HPE_OK;
    }
    totals_out[0] = t.coef;
    totals_out[1] = t.workspace;
    totals_out[2] = t.frames;
    totals_out[3] = t.idct_groups;
    totals_out[4] = t.store_groups;
    if (coef_out) {
        if (t.coef > coef_capacity)
            return refuse(why, "coef_capacity is below the batch's coefficient count"), HPE_ERR_INVALID;
        for_each_image(B, threads, [&](int b) {
            if (status_out[b] != HPE_OK) return;
            HpeJpegImage& e = table_out[b];
            const Header& hd = headers[b];
            for (int c = 0; c < e.ncomp; ++c) std::memcpy(e.quant[c], hd.quant[hd.tq[c]], 64);
            if (!decode_scan(streams[b], lengths[b], hd, e, coef_out, &whys[b])) {
                for (int c = 0; c < e.ncomp; ++c)  // no partial decode stays behind
                    std::memset(coef_out + e.coef_offset[c], 0, sizeof(short) * 64 * (size_t)e.blocks_w[c] * (size_t)e.blocks_h[c]);
                std::memset(&e, 0, sizeof(e));
                status_out[b] = HPE_ERR_INVALID;
            }
        });
    }
    for (int b = 0; b < B; ++b)
        if (status_out[b] != HPE_OK) {
            if (why) *why = at_image(b, whys[b]);
            return HPE_ERR_INVALID;
        }
    return HPE_OK;
}

}  // namespace jpeg
