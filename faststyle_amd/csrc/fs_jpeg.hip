// Baseline JPEG decoding, split where the hardware splits it (include/faststyle_io.h):
//   host   -- fs_jpeg_parse / fs_jpeg_decode: marker parsing and Huffman decoding, plain C++ with no global state (decode threads call
//             it concurrently, the interpreter lock released); writes quantised int16 coefficients, de-zigzagged, one plane per component;
//   device -- jpeg_idct_kernel (dequantise + 8x8 inverse DCT, in place: a block's 128 coefficient bytes become its 64 samples) and
//             jpeg_color_kernel (chroma upsampling + YCbCr -> RGB, written as the u8 pixels fs_resize_bicubic_u8x_many reads).
// The arithmetic is the integer arithmetic of the IJG library as libjpeg-turbo ships it (ITU-T T.81; jidctint.c "islow", jdsample.c "fancy"
// upsampling, jdcolor.c), restated from its published description: the result equals PIL's decode of the same bytes bit for bit
// (tests/test_jpeg.py).  Whatever this decoder does not take answers 1 and goes to PIL; whatever is malformed answers a negative code.
#include "../../include/faststyle_io.h"

#include <cstring>

#include "fs_jpeg.h"

namespace fs {

// 0, or the error code of fs_jpeg_reconstruct_many for this descriptor; the kernels skip a descriptor that fails it
__host__ __device__ int jpeg_item_check(const fs_jpeg_item& it, unsigned long long coef_bytes, unsigned long long rgb_bytes) {
    if (it.pixel_bytes != 3 && it.pixel_bytes != 4) return -2;
    if (it.width < 1 || it.height < 1 || it.width > 65535 || it.height > 65535) return -1;
    if (it.ncomp != 1 && it.ncomp != 3) return -1;
    if (it.hs < 1 || it.hs > 2 || it.vs < 1 || it.vs > it.hs) return -1;
    if (it.ncomp == 1 && (it.hs != 1 || it.vs != 1)) return -1;
    if ((it.coef_offset & 15) || (it.qt_offset & 15) || (it.pixel_bytes == 4 && (it.dst_offset & 3))) return -5;
    JpegGeom g;
    jpeg_geom(it.width, it.height, it.ncomp, it.hs, it.vs, g);
    if (it.coef_offset > coef_bytes || g.coef_count * 2 > coef_bytes - it.coef_offset) return -1;
    if (it.qt_offset > coef_bytes || 384 > coef_bytes - it.qt_offset) return -1;
    const unsigned long long out = (unsigned long long)it.width * it.height * it.pixel_bytes;
    if (it.dst_offset > rgb_bytes || out > rgb_bytes - it.dst_offset) return -1;
    return 0;
}

namespace {

// ---------------------------------------------------------------- host: markers and Huffman decoding
constexpr int kLookBits = 9;

struct Huff {
    bool set = false;
    unsigned char vals[256];
    int maxcode[18];                    // largest code of each length, -1: none
    int valoff[17];                     // vals index of the first code of a length, minus that code
    unsigned short look[1 << kLookBits];  // (length << 8) | symbol for codes of up to kLookBits bits; 0: longer
};

struct Header {
    fs_jpeg_info info;
    unsigned short qt[4][64];           // natural order
    bool qt_set[4] = {false, false, false, false};
    Huff dc[4], ac[4];
    int td[3], ta[3];
    int comp_id[3];
    bool sof = false, jfif = false, adobe = false;
};

inline unsigned be16(const unsigned char* p) { return ((unsigned)p[0] << 8) | p[1]; }

// A DHT table: counts[16] then the symbols.  Every code must fit its length (a full code space is allowed, an overfull one is not).
int build_huff(Huff& h, const unsigned char* counts, const unsigned char* syms, bool dc) {
    memset(h.look, 0, sizeof(h.look));
    int code = 0, k = 0;
    for (int l = 1; l <= 16; ++l) {
        h.valoff[l] = k - code;
        for (int i = 0; i < counts[l - 1]; ++i, ++k, ++code) {
            if (code >= (1 << l)) return -2;
            const unsigned char s = syms[k];
            if (dc && s > 15) return -2;
            h.vals[k] = s;
            if (l <= kLookBits) {
                const int first = code << (kLookBits - l);
                for (int j = 0; j < (1 << (kLookBits - l)); ++j) h.look[first + j] = (unsigned short)((l << 8) | s);
            }
        }
        h.maxcode[l] = counts[l - 1] ? code - 1 : -1;
        code <<= 1;
    }
    h.maxcode[17] = 0x7fffffff;
    h.set = true;
    return 0;
}

// Markers up to and including SOS.  0: handled (h.info filled, the tables of the scan present), 1: a JPEG for PIL, < 0: malformed.
int parse_headers(const unsigned char* p, size_t n, Header& h, const char* who) {
    if (n < 4 || p[0] != 0xFF || p[1] != 0xD8) return set_error(-1, "%s: no SOI marker (not a JPEG)", who);
    memset(&h.info, 0, sizeof(h.info));
    size_t pos = 2;
    for (;;) {
        if (pos >= n || n - pos < 2) return set_error(-1, "%s: truncated before the scan (byte %zu)", who, pos);
        if (p[pos] != 0xFF) return set_error(-2, "%s: byte %zu is not a marker", who, pos);
        while (pos < n && p[pos] == 0xFF) ++pos;
        if (pos >= n) return set_error(-1, "%s: truncated inside a marker", who);
        const unsigned m = p[pos++];
        if (m == 0xD8 || m == 0xD9 || m == 0x01 || m == 0x00 || (m >= 0xD0 && m <= 0xD7))
            return set_error(-2, "%s: marker 0x%02x before the scan", who, m);
        if (n - pos < 2) return set_error(-1, "%s: truncated segment header at byte %zu", who, pos);
        const size_t L = be16(p + pos);
        if (L < 2 || L > n - pos) return set_error(-1, "%s: segment 0x%02x at byte %zu runs past the end", who, m, pos);
        const unsigned char* seg = p + pos + 2;
        size_t len = L - 2;
        pos += L;
        switch (m) {
        case 0xC0:
        case 0xC1: {
            if (h.sof) return set_error(-2, "%s: two frame headers", who);
            if (len < 6 || len != 6 + 3 * (size_t)seg[5]) return set_error(-2, "%s: bad frame header length", who);
            const int P = seg[0], H = (int)be16(seg + 1), W = (int)be16(seg + 3), nf = seg[5];
            if (W == 0) return set_error(-2, "%s: zero width", who);
            if (P != 8 || H == 0 || (nf != 1 && nf != 3)) return 1;
            h.info.width = W;
            h.info.height = H;
            h.info.ncomp = nf;
            for (int c = 0; c < nf; ++c) {
                const unsigned char* q = seg + 6 + 3 * c;
                h.comp_id[c] = q[0];
                h.info.hs[c] = q[1] >> 4;
                h.info.vs[c] = q[1] & 15;
                h.info.tq[c] = q[2];
                if (h.info.hs[c] < 1 || h.info.hs[c] > 4 || h.info.vs[c] < 1 || h.info.vs[c] > 4 || q[2] > 3)
                    return set_error(-2, "%s: bad component %d in the frame header", who, c);
            }
            const int hs = h.info.hs[0], vs = h.info.vs[0];
            if (nf == 1) {
                if (hs != 1 || vs != 1) return 1;
            } else {
                if (h.info.hs[1] != 1 || h.info.vs[1] != 1 || h.info.hs[2] != 1 || h.info.vs[2] != 1) return 1;
                if (!((hs == 1 && vs == 1) || (hs == 2 && vs == 1) || (hs == 2 && vs == 2))) return 1;      // (1x2, 4:4:0, among the rest)
            }
            h.sof = true;
            break;
        }
        case 0xC4:
            while (len > 0) {
                if (len < 17) return set_error(-2, "%s: truncated Huffman table", who);
                const int tc = seg[0] >> 4, th = seg[0] & 15;
                int total = 0;
                for (int i = 0; i < 16; ++i) total += seg[1 + i];
                if (tc > 1 || th > 3 || total > 256 || (size_t)total > len - 17) return set_error(-2, "%s: bad Huffman table header", who);
                if (build_huff(tc ? h.ac[th] : h.dc[th], seg + 1, seg + 17, tc == 0)) return set_error(-2, "%s: Huffman table with an impossible code", who);
                seg += 17 + total;
                len -= 17 + (size_t)total;
            }
            break;
        case 0xDB:
            while (len > 0) {
                const int pq = seg[0] >> 4, tq = seg[0] & 15;
                if (pq > 1 || tq > 3) return set_error(-2, "%s: bad quantisation table header", who);
                if (pq == 1) return 1;         // 16-bit tables: PIL's
                if (len < 65) return set_error(-2, "%s: truncated quantisation table", who);
                for (int i = 0; i < 64; ++i) h.qt[tq][kJpegZigzag[i]] = seg[1 + i];
                h.qt_set[tq] = true;
                seg += 65;
                len -= 65;
            }
            break;
        case 0xDD:
            if (len != 2) return set_error(-2, "%s: bad restart interval segment", who);
            h.info.restart_interval = (int)be16(seg);
            break;
        case 0xE0:
            if (len >= 14 && !memcmp(seg, "JFIF\0", 5)) h.jfif = true;
            break;
        case 0xEE:
            if (len >= 12 && !memcmp(seg, "Adobe", 5)) h.adobe = true;
            break;
        case 0xDA: {
            if (!h.sof) return set_error(-2, "%s: scan before the frame header", who);
            const int nf = h.info.ncomp;
            if (len < 1) return set_error(-2, "%s: bad scan header", who);
            const int ns = seg[0];
            if (ns < 1 || ns > 4 || len != 4 + 2 * (size_t)ns) return set_error(-2, "%s: bad scan header", who);
            if (ns != nf) return 1;            // several scans
            for (int c = 0; c < ns; ++c) {
                if (seg[1 + 2 * c] != h.comp_id[c]) return 1;
                h.td[c] = seg[2 + 2 * c] >> 4;
                h.ta[c] = seg[2 + 2 * c] & 15;
                if (h.td[c] > 3 || h.ta[c] > 3) return set_error(-2, "%s: bad table selector in the scan header", who);
                if (!h.dc[h.td[c]].set || !h.ac[h.ta[c]].set || !h.qt_set[h.info.tq[c]]) return 1;      // (tables a decoder may supply itself)
            }
            const unsigned char* t = seg + 1 + 2 * ns;
            if (t[0] != 0 || t[1] != 63 || t[2] != 0) return 1;
            if (nf == 3) {
                if (h.adobe) return 1;
                if (!h.jfif && !(h.comp_id[0] == 1 && h.comp_id[1] == 2 && h.comp_id[2] == 3)) return 1;
            }
            jpeg_fill_info(h.info);
            if (h.info.coef_count > (1ull << 28)) return 1;
            h.info.scan_offset = pos;
            return 0;
        }
        case 0xC2: case 0xC3: case 0xC5: case 0xC6: case 0xC7: case 0xC8: case 0xC9: case 0xCA: case 0xCB: case 0xCC: case 0xCD: case 0xCE:
        case 0xCF: case 0xDC: case 0xDE: case 0xDF:
            return 1;                          // progressive, lossless, arithmetic, hierarchical, DNL
        default:
            break;                             // APPn, COM and reserved segments: skipped
        }
    }
}

// MSB-first bit reader over the entropy-coded segment.  It never reads at or beyond `end`; once the data or the segment (a marker) ends it
// supplies zero bits and counts them, and a decoder that consumed one of those has run out of data.
struct Bits {
    const unsigned char* p;
    size_t pos, end;
    unsigned long long acc = 0;
    int nbits = 0, fake = 0;

    void fill() {
        while (nbits <= 56) {
            unsigned b = 0;
            if (fake == 0 && pos < end && (p[pos] != 0xFF || (pos + 1 < end && p[pos + 1] == 0x00))) {
                b = p[pos];
                pos += b == 0xFF ? 2 : 1;
            } else {
                fake += 8;
            }
            acc = (acc << 8) | b;
            nbits += 8;
        }
    }
    unsigned peek(int k) const { return (unsigned)(acc >> (nbits - k)) & ((1u << k) - 1); }
    bool overrun() const { return nbits < fake; }
};

inline int decode_symbol(Bits& b, const Huff& h) {
    b.fill();
    const unsigned look = h.look[b.peek(kLookBits)];
    if (look) {
        b.nbits -= (int)(look >> 8);
        return (int)(look & 255);
    }
    const int code16 = (int)b.peek(16);
    for (int l = kLookBits + 1; l <= 16; ++l) {
        const int code = code16 >> (16 - l);
        if (code <= h.maxcode[l]) {
            b.nbits -= l;
            return h.vals[h.valoff[l] + code];
        }
    }
    return -1;
}

inline int receive_extend(Bits& b, int s) {
    b.fill();
    const int v = (int)b.peek(s);
    b.nbits -= s;
    return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

}  // namespace
}  // namespace fs

extern "C" {

int fs_jpeg_parse(const void* jpeg, size_t n, fs_jpeg_info* info) {
    if (!jpeg || !info) return fs::set_error(-1, "fs_jpeg_parse: null argument");
    fs::Header h;
    const int rc = fs::parse_headers(static_cast<const unsigned char*>(jpeg), n, h, "fs_jpeg_parse");
    if (rc == 0) *info = h.info;
    return rc;
}

int fs_jpeg_decode(const void* jpeg, size_t n, const fs_jpeg_info* info, void* out, size_t out_bytes) {
    using namespace fs;
    if (!jpeg || !info || !out) return set_error(-1, "fs_jpeg_decode: null argument");
    if ((uintptr_t)out & 1) return set_error(-5, "fs_jpeg_decode: out must be 2-byte aligned");
    const unsigned char* p = static_cast<const unsigned char*>(jpeg);
    Header h;
    const int rc = parse_headers(p, n, h, "fs_jpeg_decode");
    if (rc) return rc;
    if (memcmp(&h.info, info, sizeof(h.info))) return set_error(-1, "fs_jpeg_decode: info was not filled by fs_jpeg_parse from these bytes");
    const fs_jpeg_info& in = h.info;
    if (out_bytes < in.coef_bytes) return set_error(-1, "fs_jpeg_decode: out holds %zu bytes, the image needs %llu", out_bytes, (unsigned long long)in.coef_bytes);
    unsigned char* o = static_cast<unsigned char*>(out);
    memset(o, 0, (size_t)in.coef_bytes);
    for (int c = 0; c < in.ncomp; ++c) memcpy(o + in.qt_offset + 128 * c, h.qt[in.tq[c]], 128);

    Bits b;
    b.p = p;
    b.pos = (size_t)in.scan_offset;
    b.end = n;
    int pred[3] = {0, 0, 0};
    int left = in.restart_interval, next_rst = 0;
    for (int my = 0; my < in.mcu_y; ++my)
        for (int mx = 0; mx < in.mcu_x; ++mx) {
            if (in.restart_interval && left == 0) {
                // the bits left are the padding of the last byte; then RSTm, m counting modulo 8
                if (b.nbits - b.fake >= 8) return set_error(-4, "fs_jpeg_decode: data left over before a restart marker");
                size_t q = b.pos;
                while (q + 1 < n && p[q] == 0xFF && p[q + 1] == 0xFF) ++q;
                if (q + 1 >= n || p[q] != 0xFF || p[q + 1] != 0xD0 + next_rst) return set_error(-4, "fs_jpeg_decode: restart marker %d missing at byte %zu", next_rst, q);
                b.pos = q + 2;
                b.acc = 0;
                b.nbits = b.fake = 0;
                next_rst = (next_rst + 1) & 7;
                left = in.restart_interval;
                pred[0] = pred[1] = pred[2] = 0;
            }
            --left;
            for (int c = 0; c < in.ncomp; ++c) {
                const Huff& dc = h.dc[h.td[c]];
                const Huff& ac = h.ac[h.ta[c]];
                for (int v = 0; v < in.vs[c]; ++v)
                    for (int u = 0; u < in.hs[c]; ++u) {
                        const size_t blk = (size_t)(my * in.vs[c] + v) * in.blocks_x[c] + (size_t)(mx * in.hs[c] + u);
                        int16_t* dst = reinterpret_cast<int16_t*>(o + in.plane_offset[c]) + blk * 64;
                        int s = decode_symbol(b, dc);
                        if (s < 0 || s > 11) return set_error(-4, "fs_jpeg_decode: bad DC code in MCU (%d, %d)", mx, my);
                        if (s) pred[c] += receive_extend(b, s);
                        if (pred[c] < -32768 || pred[c] > 32767) return set_error(-4, "fs_jpeg_decode: DC value out of range in MCU (%d, %d)", mx, my);
                        dst[0] = (int16_t)pred[c];
                        for (int k = 1; k < 64;) {
                            const int rs = decode_symbol(b, ac);
                            if (rs < 0) return set_error(-4, "fs_jpeg_decode: bad AC code in MCU (%d, %d)", mx, my);
                            const int r = rs >> 4;
                            s = rs & 15;
                            if (s == 0) {
                                if (r == 0) break;                              // end of block
                                if (r != 15 || k + 16 > 63) return set_error(-4, "fs_jpeg_decode: bad zero run in MCU (%d, %d)", mx, my);
                                k += 16;
                                continue;
                            }
                            k += r;
                            if (k > 63 || s > 10) return set_error(-4, "fs_jpeg_decode: coefficient outside the block in MCU (%d, %d)", mx, my);
                            dst[kJpegZigzag[k]] = (int16_t)receive_extend(b, s);
                            ++k;
                        }
                        if (b.overrun()) return set_error(-4, "fs_jpeg_decode: scan data ends in MCU (%d, %d)", mx, my);
                    }
            }
        }
    // what a complete file has next: the padding bits, then EOI
    if (b.nbits - b.fake >= 8) return set_error(-4, "fs_jpeg_decode: data left over after the last MCU");
    size_t q = b.pos;
    while (q + 1 < n && p[q] == 0xFF && p[q + 1] == 0xFF) ++q;
    if (q + 1 >= n || p[q] != 0xFF || p[q + 1] != 0xD9) return set_error(-4, "fs_jpeg_decode: no EOI marker after the scan (byte %zu)", q);
    return 0;
}

}  // extern "C"

namespace fs {
namespace {

// ---------------------------------------------------------------- device: inverse DCT
// jidctint.c's "islow": 13-bit constants, two extra bits after the column pass.  Written in wrapping (unsigned) arithmetic: the coefficients of a
// corrupt file that still parsed are arbitrary int16 values, and they must not make the arithmetic undefined -- the result is then garbage
// pixels, nothing else.  For the coefficients of an encoder no sum leaves 32 bits and this is the signed arithmetic of the library.
typedef unsigned u32;
constexpr u32 F0_298 = 2446, F0_390 = 3196, F0_541 = 4433, F0_765 = 6270, F0_899 = 7373, F1_175 = 9633, F1_501 = 12299, F1_847 = 15137,
              F1_961 = 16069, F2_053 = 16819, F2_562 = 20995, F3_072 = 25172;

__device__ __forceinline__ int descale(u32 x, int n) { return (int)(x + (1u << (n - 1))) >> n; }

// one 8-point pass: in[0..8) -> out[0..8), descaled by `shift`
__device__ __forceinline__ void idct8(const u32 in[8], int out[8], int shift) {
    u32 z2 = in[2], z3 = in[6];
    u32 z1 = (z2 + z3) * F0_541;
    const u32 tmp2 = z1 - z3 * F1_847, tmp3 = z1 + z2 * F0_765;
    const u32 e0 = (in[0] + in[4]) << 13, e1 = (in[0] - in[4]) << 13;
    const u32 tmp10 = e0 + tmp3, tmp13 = e0 - tmp3, tmp11 = e1 + tmp2, tmp12 = e1 - tmp2;
    u32 t0 = in[7], t1 = in[5], t2 = in[3], t3 = in[1];
    z1 = t0 + t3;
    z2 = t1 + t2;
    z3 = t0 + t2;
    u32 z4 = t1 + t3;
    const u32 z5 = (z3 + z4) * F1_175;
    t0 *= F0_298;
    t1 *= F2_053;
    t2 *= F3_072;
    t3 *= F1_501;
    z1 = 0u - z1 * F0_899;
    z2 = 0u - z2 * F2_562;
    z3 = z5 - z3 * F1_961;
    z4 = z5 - z4 * F0_390;
    t0 += z1 + z3;
    t1 += z2 + z4;
    t2 += z2 + z3;
    t3 += z1 + z4;
    out[0] = descale(tmp10 + t3, shift);
    out[7] = descale(tmp10 - t3, shift);
    out[1] = descale(tmp11 + t2, shift);
    out[6] = descale(tmp11 - t2, shift);
    out[2] = descale(tmp12 + t1, shift);
    out[5] = descale(tmp12 - t1, shift);
    out[3] = descale(tmp13 + t0, shift);
    out[4] = descale(tmp13 - t0, shift);
}

__device__ __forceinline__ int half_of(const uint4& v, int e) {      // int16 element e (0..7) of a 16-byte word, sign extended
    const u32 w = e < 2 ? v.x : e < 4 ? v.y : e < 6 ? v.z : v.w;
    return (int)(short)(unsigned short)(w >> ((e & 1) * 16));
}
__device__ __forceinline__ u32 uhalf_of(const uint4& v, int e) {
    const u32 w = e < 2 ? v.x : e < 4 ? v.y : e < 6 ? v.z : v.w;
    return (w >> ((e & 1) * 16)) & 0xffffu;
}
__device__ __forceinline__ u32 clamp_u8(int v) { return (u32)(v < 0 ? 0 : v > 255 ? 255 : v); }

// One lane per 8x8 block, grid.y = image.  The block's 128 bytes are read whole before its first 64 bytes are rewritten with the samples
// (row-major 8x8 u8): no other lane touches them, so the pass needs no second buffer.
__global__ __launch_bounds__(64) void jpeg_idct_kernel(unsigned char* coef_base, unsigned long long coef_bytes, const fs_jpeg_item* __restrict__ items,
                                                       unsigned char* rgb_base, unsigned long long rgb_bytes) {
    (void)rgb_base;
    const fs_jpeg_item it = items[blockIdx.y];
    if (jpeg_item_check(it, coef_bytes, rgb_bytes)) return;
    JpegGeom g;
    jpeg_geom(it.width, it.height, it.ncomp, it.hs, it.vs, g);
    long long blk = (long long)blockIdx.x * 64 + threadIdx.x;
    int c = 0;
    while (c < 3 && blk >= (long long)g.bw[c] * g.bh[c]) {
        blk -= (long long)g.bw[c] * g.bh[c];
        ++c;
    }
    if (c >= it.ncomp) return;
    uint4* block = reinterpret_cast<uint4*>(coef_base + it.coef_offset + g.plane[c] + (unsigned long long)blk * 128);
    const uint4* qt = reinterpret_cast<const uint4*>(coef_base + it.qt_offset + 128 * c);
    uint4 cf[8], q[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        cf[r] = block[r];
        q[r] = qt[r];
    }
    int ws[8][8];
#pragma unroll
    for (int x = 0; x < 8; ++x) {                 // columns: dequantise, descale by CONST_BITS - PASS1_BITS
        u32 in[8];
        int col[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) in[r] = (u32)half_of(cf[r], x) * uhalf_of(q[r], x);
        idct8(in, col, 11);
#pragma unroll
        for (int r = 0; r < 8; ++r) ws[r][x] = col[r];
    }
    u32 px[16];
#pragma unroll
    for (int r = 0; r < 8; ++r) {                 // rows: descale by CONST_BITS + PASS1_BITS + 3, level shift, clamp
        u32 in[8];
        int row[8];
#pragma unroll
        for (int x = 0; x < 8; ++x) in[x] = (u32)ws[r][x];
        idct8(in, row, 18);
        px[2 * r] = clamp_u8(row[0] + 128) | clamp_u8(row[1] + 128) << 8 | clamp_u8(row[2] + 128) << 16 | clamp_u8(row[3] + 128) << 24;
        px[2 * r + 1] = clamp_u8(row[4] + 128) | clamp_u8(row[5] + 128) << 8 | clamp_u8(row[6] + 128) << 16 | clamp_u8(row[7] + 128) << 24;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) block[i] = make_uint4(px[4 * i], px[4 * i + 1], px[4 * i + 2], px[4 * i + 3]);
}

// ---------------------------------------------------------------- device: chroma upsampling and colour
// address of sample (x, y) of a plane of bw blocks per row, as jpeg_idct_kernel left it
__device__ __forceinline__ const unsigned char* sample_at(const unsigned char* plane, int bw, int x, int y) {
    return plane + ((size_t)(y >> 3) * bw + (x >> 3)) * 128 + (y & 7) * 8 + (x & 7);
}

// samples cx0 - 1 .. cx0 + 4 of chroma row y (cx0 a multiple of 4), an index outside [0, cw) clamped to the edge sample: with the edge
// repeated, the triangle filter's general form gives exactly the library's edge values ((3 s + s + 1) >> 2 = s; (3 t + t + 8) >> 4 = (4 t + 8) >> 4)
__device__ __forceinline__ void chroma_row(const unsigned char* plane, int bw, int cw, int cx0, int y, int a[6]) {
    const u32 w = *reinterpret_cast<const u32*>(sample_at(plane, bw, cx0, y));
    a[0] = *sample_at(plane, bw, cx0 > 0 ? cx0 - 1 : 0, y);
    a[1] = (int)(w & 255);
    a[2] = (int)((w >> 8) & 255);
    a[3] = (int)((w >> 16) & 255);
    a[4] = (int)(w >> 24);
    a[5] = *sample_at(plane, bw, cx0 + 4 < cw ? cx0 + 4 : cw - 1, y);
    const int last = cw - 1 - cx0;              // position of the last true sample among a[1..4] (>= 4: beyond them)
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (j >= last) a[j + 2] = a[j + 1];
}

// One lane per 8 output pixels of a row, grid.y = image.
__global__ __launch_bounds__(256) void jpeg_color_kernel(const unsigned char* __restrict__ coef_base, unsigned long long coef_bytes,
                                                         const fs_jpeg_item* __restrict__ items, unsigned char* __restrict__ rgb_base,
                                                         unsigned long long rgb_bytes) {
    const fs_jpeg_item it = items[blockIdx.y];
    if (jpeg_item_check(it, coef_bytes, rgb_bytes)) return;
    JpegGeom g;
    jpeg_geom(it.width, it.height, it.ncomp, it.hs, it.vs, g);
    const int W = it.width, H = it.height, gx = (W + 7) >> 3;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)gx * H) return;
    const int y = (int)(t / gx), x0 = (int)(t - (long long)y * gx) * 8;
    const unsigned char* img = coef_base + it.coef_offset;
    const uint2 yw = *reinterpret_cast<const uint2*>(sample_at(img + g.plane[0], g.bw[0], x0, y));
    int Y[8], cb[8], cr[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) Y[j] = (int)(((j < 4 ? yw.x : yw.y) >> ((j & 3) * 8)) & 255);
    if (it.ncomp == 1) {
#pragma unroll
        for (int j = 0; j < 8; ++j) cb[j] = cr[j] = 128;
    } else if (it.hs == 1) {
        const uint2 bw_ = *reinterpret_cast<const uint2*>(sample_at(img + g.plane[1], g.bw[1], x0, y));
        const uint2 rw_ = *reinterpret_cast<const uint2*>(sample_at(img + g.plane[2], g.bw[2], x0, y));
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            cb[j] = (int)(((j < 4 ? bw_.x : bw_.y) >> ((j & 3) * 8)) & 255);
            cr[j] = (int)(((j < 4 ? rw_.x : rw_.y) >> ((j & 3) * 8)) & 255);
        }
    } else {
        const int cx0 = x0 >> 1, cy = it.vs == 2 ? y >> 1 : y;
        const bool fancy = g.cw > 2;             // the library replicates when the chroma row has one or two samples
#pragma unroll
        for (int c = 1; c < 3; ++c) {
            int* dst = c == 1 ? cb : cr;
            const unsigned char* plane = img + g.plane[c];
            int a[6];
            chroma_row(plane, g.bw[c], g.cw, cx0, cy, a);
            if (!fancy) {
#pragma unroll
                for (int j = 0; j < 8; ++j) dst[j] = a[1 + (j >> 1)];
            } else if (it.vs == 1) {
#pragma unroll
                for (int j = 0; j < 8; ++j) dst[j] = (3 * a[1 + (j >> 1)] + ((j & 1) ? a[2 + (j >> 1)] + 2 : a[j >> 1] + 1)) >> 2;
            } else {
                const int far_y = (y & 1) ? (cy + 1 < g.ch ? cy + 1 : cy) : (cy > 0 ? cy - 1 : 0);
                int f[6];
                chroma_row(plane, g.bw[c], g.cw, cx0, far_y, f);
#pragma unroll
                for (int j = 0; j < 6; ++j) a[j] = 3 * a[j] + f[j];
#pragma unroll
                for (int j = 0; j < 8; ++j) dst[j] = (3 * a[1 + (j >> 1)] + ((j & 1) ? a[2 + (j >> 1)] + 7 : a[j >> 1] + 8)) >> 4;
            }
        }
    }
    u32 px[8];
    unsigned char rgb[8][3];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int b_ = cb[j] - 128, r_ = cr[j] - 128;
        const u32 R = clamp_u8(Y[j] + ((91881 * r_ + 32768) >> 16));
        const u32 G = clamp_u8(Y[j] + ((-22554 * b_ - 46802 * r_ + 32768) >> 16));
        const u32 B = clamp_u8(Y[j] + ((116130 * b_ + 32768) >> 16));
        px[j] = R | G << 8 | B << 16 | 0xff000000u;
        rgb[j][0] = (unsigned char)R;
        rgb[j][1] = (unsigned char)G;
        rgb[j][2] = (unsigned char)B;
    }
    const int nvalid = W - x0 < 8 ? W - x0 : 8;
    unsigned char* out = rgb_base + it.dst_offset + ((size_t)y * W + x0) * it.pixel_bytes;
    if (it.pixel_bytes == 4) {
        if (nvalid == 8 && ((uintptr_t)out & 15) == 0) {
            reinterpret_cast<uint4*>(out)[0] = make_uint4(px[0], px[1], px[2], px[3]);
            reinterpret_cast<uint4*>(out)[1] = make_uint4(px[4], px[5], px[6], px[7]);
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (j < nvalid) reinterpret_cast<u32*>(out)[j] = px[j];
        }
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (j < nvalid) {
                out[3 * j] = rgb[j][0];
                out[3 * j + 1] = rgb[j][1];
                out[3 * j + 2] = rgb[j][2];
            }
    }
}

}  // namespace

// max_blocks / max_groups: the largest block count (all components) and 8-pixel group count of one image, from the host's copy of the table
int jpeg_reconstruct_many(unsigned char* coef_base, size_t coef_bytes, const fs_jpeg_item* items_dev, int K, unsigned long long max_blocks,
                          unsigned long long max_groups, unsigned char* rgb_base, size_t rgb_bytes, hipStream_t s) {
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)((max_blocks + 63) / 64), (unsigned)K), dim3(64), 0, s, coef_base,
                       (unsigned long long)coef_bytes, items_dev, rgb_base, (unsigned long long)rgb_bytes);
    if (hipGetLastError() != hipSuccess) return -3;
    hipLaunchKernelGGL(jpeg_color_kernel, dim3((unsigned)((max_groups + 255) / 256), (unsigned)K), dim3(256), 0, s,
                       (const unsigned char*)coef_base, (unsigned long long)coef_bytes, items_dev, rgb_base, (unsigned long long)rgb_bytes);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

void jpeg_item_extent(const fs_jpeg_item& it, unsigned long long* blocks, unsigned long long* groups) {
    JpegGeom g;
    jpeg_geom(it.width, it.height, it.ncomp, it.hs, it.vs, g);
    *blocks = g.coef_count / 64;
    *groups = (unsigned long long)((it.width + 7) >> 3) * it.height;
}

}  // namespace fs
