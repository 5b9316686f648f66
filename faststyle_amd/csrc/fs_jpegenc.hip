// Baseline JPEG encoding, the decoder's split (fs_jpeg.hip) the other way round (include/faststyle_io.h):
//   device -- jpegenc_sample_kernel (RGB -> YCbCr, chroma box downsampling, edge replication: the u8 samples of every block, written into the
//             block's first 64 bytes) and jpegenc_fdct_kernel (level shift, 8x8 forward DCT, quantisation, in place: a block's 64 samples
//             become its 64 int16 coefficients; the quantisation tables of the quality are written behind the planes);
//   host   -- fs_jpeg_encode_plan / fs_jpeg_write_bound / fs_jpeg_write: markers and Huffman coding with the Annex K tables, plain C++ with no
//             global state and no allocation (encode threads call it concurrently, the interpreter lock released).
// The arithmetic is the integer arithmetic of the IJG library's default compressor as libjpeg-turbo ships it (ITU-T T.81; jccolor.c, jcsample.c,
// jfdctint.c "islow", jcdctmgr.c, the single-pass coefficient controller of jccoefct.c, jchuff.c, jcmarker.c), restated from its published
// description: the file equals PIL's for the same pixels and options byte for byte (tests/test_jpeg_encode.py).
#include "../../include/faststyle_io.h"

#include <cstring>

#include "fs_jpeg.h"

namespace fs {

// 0, or the error code of fs_jpeg_forward_many for this descriptor; the kernels skip a descriptor that fails it
__host__ __device__ int jpegenc_item_check(const fs_jpegenc_item& it, unsigned long long src_bytes, unsigned long long coef_bytes) {
    if (it.width < 1 || it.height < 1 || it.width > 65535 || it.height > 65535) return -1;
    if (it.ncomp != 1 && it.ncomp != 3) return -1;
    if (it.hs < 1 || it.hs > 2 || it.vs < 1 || it.vs > it.hs) return -1;
    if (it.ncomp == 1 && (it.hs != 1 || it.vs != 1)) return -1;
    if (it.ncomp == 1 ? it.pixel_bytes != 1 : (it.pixel_bytes != 3 && it.pixel_bytes != 4)) return -2;
    if (it.quality < 1 || it.quality > 100) return -2;
    if ((it.coef_offset & 15) || (it.qt_offset & 15) || (it.pixel_bytes == 4 && (it.src_offset & 3))) return -5;
    JpegGeom g;
    jpeg_geom(it.width, it.height, it.ncomp, it.hs, it.vs, g);
    if (it.coef_offset > coef_bytes || g.coef_count * 2 > coef_bytes - it.coef_offset) return -1;
    if (it.qt_offset > coef_bytes || 384 > coef_bytes - it.qt_offset) return -1;
    const unsigned long long in = (unsigned long long)it.width * it.height * it.pixel_bytes;
    if (it.src_offset > src_bytes || in > src_bytes - it.src_offset) return -1;
    return 0;
}

namespace {

// ---------------------------------------------------------------- device: quantisation tables of a quality
// Annex K tables K.1 (c == 0) and K.2, natural order, scaled the IJG way: the quantisation value of entry i
__host__ __device__ inline int jpegenc_quant(int c, int i, int quality) {
    constexpr unsigned char kStd[2][64] = {
        {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
         18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,  49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
        {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
         99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    const int v = ((int)kStd[c ? 1 : 0][i] * scale + 50) / 100;
    return v < 1 ? 1 : v > 255 ? 255 : v;
}

// ---------------------------------------------------------------- device: colour conversion and downsampling
// jccolor.c: 16-bit fixed point, FIX(x) = (int)(x * 65536 + 0.5); the chroma offset carries ONE_HALF - 1
__device__ __forceinline__ int ycc_y(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }
__device__ __forceinline__ int ycc_cb(int r, int g, int b) { return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16; }
__device__ __forceinline__ int ycc_cr(int r, int g, int b) { return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16; }

// component c (0 Y, 1 Cb, 2 Cr) of source pixel (x, y), both inside the image
__device__ __forceinline__ int comp_at(const unsigned char* __restrict__ src, int W, int pixel_bytes, int c, int x, int y) {
    const unsigned char* p = src + ((size_t)y * W + x) * pixel_bytes;
    if (pixel_bytes == 1) return p[0];
    int r, g, b;
    if (pixel_bytes == 4) {
        const unsigned w = *reinterpret_cast<const unsigned*>(p);
        r = (int)(w & 255);
        g = (int)((w >> 8) & 255);
        b = (int)((w >> 16) & 255);
    } else {
        r = p[0];
        g = p[1];
        b = p[2];
    }
    return c == 0 ? ycc_y(r, g, b) : c == 1 ? ycc_cb(r, g, b) : ycc_cr(r, g, b);
}

// One lane per row of 8 samples of a block, grid.y = image; within a component, consecutive lanes take consecutive blocks of a block row (their
// source pixels are consecutive).  What the library's edge expansion amounts to: a source column beyond the image is its last column, a source
// row beyond it its last row, and a downsampled row beyond the true chroma height the last true one.  A dummy block (one that only pads the last
// MCU column or row; luma only) receives the samples of the block whose DC it takes: its own lane of jpegenc_fdct_kernel then finds that DC
// without reading another lane's block.
__global__ __launch_bounds__(256) void jpegenc_sample_kernel(const unsigned char* __restrict__ src_base, unsigned long long src_bytes,
                                                             const fs_jpegenc_item* __restrict__ items, unsigned char* __restrict__ coef_base,
                                                             unsigned long long coef_bytes) {
    const fs_jpegenc_item it = items[blockIdx.y];
    if (jpegenc_item_check(it, src_bytes, coef_bytes)) return;
    JpegGeom g;
    jpeg_geom(it.width, it.height, it.ncomp, it.hs, it.vs, g);
    long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    int c = 0;
    while (c < 3 && t >= (long long)g.bw[c] * g.bh[c] * 8) {
        t -= (long long)g.bw[c] * g.bh[c] * 8;
        ++c;
    }
    if (c >= it.ncomp) return;
    const int W = it.width, H = it.height;
    const int rows = (int)(t / g.bw[c]), bx = (int)(t - (long long)rows * g.bw[c]), by = rows >> 3, r = rows & 7;
    int sbx = bx, sby = by;
    if (c == 0) {
        const int wib = (W + 7) >> 3, hib = (H + 7) >> 3;        // the luma blocks that hold pixels
        if (sby >= hib) {                                        // a dummy row: the last block of the MCU's row above
            sby -= 1;
            sbx |= it.hs - 1;
        }
        if (sbx >= wib) sbx -= 1;                                // a dummy column: the block to its left
    }
    const unsigned char* src = src_base + it.src_offset;
    const int y = sby * 8 + r;
    unsigned s[8];
    if (c == 0 || it.hs == 1) {
        const int yc = y < H ? y : H - 1;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int x = sbx * 8 + j;
            s[j] = (unsigned)comp_at(src, W, it.pixel_bytes, c, x < W ? x : W - 1, yc);
        }
    } else if (it.vs == 1) {                                     // h2v1: bias 0, 1, 0, 1, ...
        const int yc = y < H ? y : H - 1;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int x = (sbx * 8 + j) * 2;
            const int a = comp_at(src, W, it.pixel_bytes, c, x < W ? x : W - 1, yc);
            const int b = comp_at(src, W, it.pixel_bytes, c, x + 1 < W ? x + 1 : W - 1, yc);
            s[j] = (unsigned)((a + b + (j & 1)) >> 1);
        }
    } else {                                                     // h2v2: bias 1, 2, 1, 2, ...
        const int cy = y < g.ch ? y : g.ch - 1;
        const int y0 = 2 * cy < H ? 2 * cy : H - 1, y1 = 2 * cy + 1 < H ? 2 * cy + 1 : H - 1;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int x = (sbx * 8 + j) * 2;
            const int x0 = x < W ? x : W - 1, x1 = x + 1 < W ? x + 1 : W - 1;
            const int sum = comp_at(src, W, it.pixel_bytes, c, x0, y0) + comp_at(src, W, it.pixel_bytes, c, x1, y0) +
                            comp_at(src, W, it.pixel_bytes, c, x0, y1) + comp_at(src, W, it.pixel_bytes, c, x1, y1);
            s[j] = (unsigned)((sum + 1 + (j & 1)) >> 2);
        }
    }
    unsigned char* block = coef_base + it.coef_offset + g.plane[c] + ((unsigned long long)by * g.bw[c] + bx) * 128;
    *reinterpret_cast<uint2*>(block + r * 8) =
        make_uint2(s[0] | s[1] << 8 | s[2] << 16 | s[3] << 24, s[4] | s[5] << 8 | s[6] << 16 | s[7] << 24);
}

// ---------------------------------------------------------------- device: forward DCT and quantisation
// jfdctint.c's "islow": 13-bit constants, two extra bits kept after the row pass; the result is the DCT scaled by 8.  Samples are 8-bit, so
// no sum leaves 32 bits.
constexpr int E0_298 = 2446, E0_390 = 3196, E0_541 = 4433, E0_765 = 6270, E0_899 = 7373, E1_175 = 9633, E1_501 = 12299, E1_847 = 15137,
              E1_961 = 16069, E2_053 = 16819, E2_562 = 20995, E3_072 = 25172;

__device__ __forceinline__ int fdescale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// one 8-point pass, in place.  Row pass: the even-even outputs are scaled up by 2 bits and the rest descaled by 11; column pass: 2 and 15.
template <bool kRows>
__device__ __forceinline__ void fdct8(int d[8]) {
    const int tmp0 = d[0] + d[7], tmp7 = d[0] - d[7], tmp1 = d[1] + d[6], tmp6 = d[1] - d[6];
    const int tmp2 = d[2] + d[5], tmp5 = d[2] - d[5], tmp3 = d[3] + d[4], tmp4 = d[3] - d[4];
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    constexpr int sh = kRows ? 11 : 15;
    d[0] = kRows ? (tmp10 + tmp11) * 4 : fdescale(tmp10 + tmp11, 2);
    d[4] = kRows ? (tmp10 - tmp11) * 4 : fdescale(tmp10 - tmp11, 2);
    int z1 = (tmp12 + tmp13) * E0_541;
    d[2] = fdescale(z1 + tmp13 * E0_765, sh);
    d[6] = fdescale(z1 - tmp12 * E1_847, sh);
    z1 = tmp4 + tmp7;
    int z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
    const int z5 = (z3 + z4) * E1_175;
    const int t4 = tmp4 * E0_298, t5 = tmp5 * E2_053, t6 = tmp6 * E3_072, t7 = tmp7 * E1_501;
    z1 *= -E0_899;
    z2 *= -E2_562;
    z3 = z3 * -E1_961 + z5;
    z4 = z4 * -E0_390 + z5;
    d[7] = fdescale(t4 + z1 + z3, sh);
    d[5] = fdescale(t5 + z2 + z4, sh);
    d[3] = fdescale(t6 + z2 + z3, sh);
    d[1] = fdescale(t7 + z1 + z4, sh);
}

// One lane per 8x8 block, grid.y = image (the geometry is the same in every lane of a workgroup).  The block's 64 sample bytes are read whole
// before its 128 bytes are rewritten with the coefficients: no other lane touches them.  The workgroup first derives the two quantisation
// tables of the image's quality into LDS; workgroup 0 of an image also writes them out behind the planes.
__global__ __launch_bounds__(64) void jpegenc_fdct_kernel(const unsigned char* src_base, unsigned long long src_bytes,
                                                          const fs_jpegenc_item* __restrict__ items, unsigned char* coef_base,
                                                          unsigned long long coef_bytes) {
    (void)src_base;
    __shared__ unsigned short qt[2][64];
    const fs_jpegenc_item it = items[blockIdx.y];
    if (jpegenc_item_check(it, src_bytes, coef_bytes)) return;
    JpegGeom g;
    jpeg_geom(it.width, it.height, it.ncomp, it.hs, it.vs, g);
    const int lane = threadIdx.x;
    qt[0][lane] = (unsigned short)jpegenc_quant(0, lane, it.quality);
    qt[1][lane] = (unsigned short)jpegenc_quant(1, lane, it.quality);
    if (blockIdx.x == 0) {
        unsigned short* out = reinterpret_cast<unsigned short*>(coef_base + it.qt_offset);
        out[lane] = qt[0][lane];
        out[64 + lane] = it.ncomp == 3 ? qt[1][lane] : (unsigned short)0;
        out[128 + lane] = it.ncomp == 3 ? qt[1][lane] : (unsigned short)0;
    }
    __syncthreads();
    long long blk = (long long)blockIdx.x * 64 + lane;
    int c = 0;
    while (c < 3 && blk >= (long long)g.bw[c] * g.bh[c]) {
        blk -= (long long)g.bw[c] * g.bh[c];
        ++c;
    }
    if (c >= it.ncomp) return;
    const int by = (int)(blk / g.bw[c]), bx = (int)(blk - (long long)by * g.bw[c]);
    const bool dummy = c == 0 && (bx >= ((it.width + 7) >> 3) || by >= ((it.height + 7) >> 3));
    uint4* block = reinterpret_cast<uint4*>(coef_base + it.coef_offset + g.plane[c] + (unsigned long long)blk * 128);
    uint4 sm[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) sm[i] = block[i];
    int ws[8][8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {                 // rows: level shift, first pass
        const unsigned lo = (r & 1) ? sm[r >> 1].z : sm[r >> 1].x, hi = (r & 1) ? sm[r >> 1].w : sm[r >> 1].y;
        int d[8];
#pragma unroll
        for (int x = 0; x < 8; ++x) d[x] = (int)(((x < 4 ? lo : hi) >> ((x & 3) * 8)) & 255) - 128;
        fdct8<true>(d);
#pragma unroll
        for (int x = 0; x < 8; ++x) ws[r][x] = d[x];
    }
    const unsigned short* q = qt[c ? 1 : 0];
    unsigned cf[8][8];
#pragma unroll
    for (int x = 0; x < 8; ++x) {                 // columns: second pass, then quantisation: divisor 8 q, half away from zero
        int d[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) d[r] = ws[r][x];
        fdct8<false>(d);
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const unsigned div = 8u * q[r * 8 + x];
            const int v = d[r];
            const unsigned m = ((unsigned)(v < 0 ? -v : v) + (div >> 1)) / div;
            const int qv = dummy && (r | x) ? 0 : (v < 0 ? -(int)m : (int)m);
            cf[r][x] = (unsigned)qv & 0xffffu;
        }
    }
#pragma unroll
    for (int r = 0; r < 8; ++r)
        block[r] = make_uint4(cf[r][0] | cf[r][1] << 16, cf[r][2] | cf[r][3] << 16, cf[r][4] | cf[r][5] << 16, cf[r][6] | cf[r][7] << 16);
}

}  // namespace

// max_blocks: the largest block count (all components) of one image, from the host's copy of the table
int jpeg_forward_many(const unsigned char* src_base, size_t src_bytes, const fs_jpegenc_item* items_dev, int K, unsigned long long max_blocks,
                      unsigned char* coef_base, size_t coef_bytes, hipStream_t s) {
    hipLaunchKernelGGL(jpegenc_sample_kernel, dim3((unsigned)((max_blocks * 8 + 255) / 256), (unsigned)K), dim3(256), 0, s, src_base,
                       (unsigned long long)src_bytes, items_dev, coef_base, (unsigned long long)coef_bytes);
    if (hipGetLastError() != hipSuccess) return -3;
    hipLaunchKernelGGL(jpegenc_fdct_kernel, dim3((unsigned)((max_blocks + 63) / 64), (unsigned)K), dim3(64), 0, s, src_base,
                       (unsigned long long)src_bytes, items_dev, coef_base, (unsigned long long)coef_bytes);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

unsigned long long jpegenc_item_blocks(const fs_jpegenc_item& it) {
    JpegGeom g;
    jpeg_geom(it.width, it.height, it.ncomp, it.hs, it.vs, g);
    return g.coef_count / 64;
}

namespace {

// ---------------------------------------------------------------- host: markers and Huffman coding
// Annex K tables K.3 - K.6: the number of codes of each length 1..16, then the symbols in code order
const unsigned char kDcBits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
const unsigned char kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const unsigned char kAcBits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
const unsigned char kAcVals[2][162] = {
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

// the headers of a file: at most SOI 2 + APP0 18 + 2 DQT of 69 + SOF0 19 + DHT 33 + 183 + 33 + 183 + SOS 14
constexpr size_t kHeaderBound = 640;
// a block at its longest: a DC code of 11 bits + 11 bits, 63 AC codes of 16 bits + 10 bits = 1660 bits, every byte stuffed; rounded up
constexpr size_t kBlockBound = 432;

struct Code {
    unsigned short code[256];
    unsigned char len[256];             // 0: the table has no such symbol
};

void build_code(Code& h, const unsigned char* bits, const unsigned char* vals) {
    memset(&h, 0, sizeof(h));
    unsigned code = 0;
    int k = 0;
    for (int l = 1; l <= 16; ++l) {
        for (int i = 0; i < bits[l - 1]; ++i, ++k, ++code) {
            h.code[vals[k]] = (unsigned short)code;
            h.len[vals[k]] = (unsigned char)l;
        }
        code <<= 1;
    }
}

// Bounded output: a byte at or beyond cap is dropped and remembered.
struct Sink {
    unsigned char* p;
    size_t cap, pos = 0;
    bool full = false;
    unsigned long long acc = 0;         // the low nbits bits are pending, MSB first
    int nbits = 0;

    void byte(unsigned b) {
        if (pos < cap)
            p[pos++] = (unsigned char)b;
        else
            full = true;
    }
    void be16(unsigned v) {
        byte(v >> 8);
        byte(v & 255);
    }
    void bytes(const unsigned char* s, size_t n) {
        for (size_t i = 0; i < n; ++i) byte(s[i]);
    }
    void bits(unsigned v, int n) {      // n <= 27; bytes leave four at a time, without a look at each unless one of them is 0xFF or the end is near
        acc = (acc << n) | (v & ((1u << n) - 1));
        nbits += n;
        if (nbits < 32) return;
        nbits -= 32;
        const unsigned w = (unsigned)(acc >> nbits);
        const unsigned inv = ~w;
        if (pos + 4 <= cap && !((inv - 0x01010101u) & ~inv & 0x80808080u)) {
            p[pos] = (unsigned char)(w >> 24);
            p[pos + 1] = (unsigned char)(w >> 16);
            p[pos + 2] = (unsigned char)(w >> 8);
            p[pos + 3] = (unsigned char)w;
            pos += 4;
            return;
        }
        for (int sh = 24; sh >= 0; sh -= 8) {
            const unsigned b = (w >> sh) & 255;
            byte(b);
            if (b == 0xFF) byte(0);
        }
    }
    void flush() {                      // pad the last byte with 1-bits
        if (nbits & 7) {
            const int pad = 8 - (nbits & 7);
            acc = (acc << pad) | ((1u << pad) - 1);
            nbits += pad;
        }
        for (; nbits; nbits -= 8) {
            const unsigned b = (unsigned)(acc >> (nbits - 8)) & 255;
            byte(b);
            if (b == 0xFF) byte(0);
        }
    }
};

inline int category(int v) {            // number of bits of |v|
    const unsigned a = (unsigned)(v < 0 ? -v : v);
    return a ? 32 - __builtin_clz(a) : 0;
}

// whether info is what fs_jpeg_encode_plan fills (scan_offset aside)
bool plan_matches(const fs_jpeg_info& in) {
    fs_jpeg_info want;
    if (fs_jpeg_encode_plan(in.width, in.height, in.ncomp, in.hs[0], in.vs[0], &want)) return false;
    want.scan_offset = in.scan_offset;
    return !memcmp(&want, &in, sizeof(want));
}

}  // namespace
}  // namespace fs

extern "C" {

int fs_jpeg_encode_plan(int width, int height, int ncomp, int hs, int vs, fs_jpeg_info* info) {
    using namespace fs;
    if (!info) return set_error(-1, "fs_jpeg_encode_plan: null argument");
    if (width < 1 || height < 1 || width > 65535 || height > 65535)
        return set_error(-1, "fs_jpeg_encode_plan: dimensions %dx%d outside [1, 65535]", width, height);
    const bool sampling = (hs == 1 && vs == 1) || (ncomp == 3 && hs == 2 && (vs == 1 || vs == 2));
    if ((ncomp != 1 && ncomp != 3) || !sampling)
        return set_error(-1, "fs_jpeg_encode_plan: %d components sampled %dx%d are not in the handled set", ncomp, hs, vs);
    memset(info, 0, sizeof(*info));
    info->width = width;
    info->height = height;
    info->ncomp = ncomp;
    for (int c = 0; c < ncomp; ++c) {
        info->hs[c] = c ? 1 : hs;
        info->vs[c] = c ? 1 : vs;
        info->tq[c] = c ? 1 : 0;
    }
    jpeg_fill_info(*info);
    return 0;
}

size_t fs_jpeg_write_bound(const fs_jpeg_info* info) {
    using namespace fs;
    if (!info || !plan_matches(*info)) return 0;
    return kHeaderBound + (size_t)(info->coef_count / 64) * kBlockBound + 16;
}

int fs_jpeg_write(const fs_jpeg_info* info, const void* coef, size_t coef_bytes, void* out, size_t cap, size_t* n) {
    using namespace fs;
    if (!info || !coef || !out || !n) return set_error(-1, "fs_jpeg_write: null argument");
    if ((uintptr_t)coef & 1) return set_error(-5, "fs_jpeg_write: coef must be 2-byte aligned");
    if (!plan_matches(*info)) return set_error(-1, "fs_jpeg_write: info was not filled by fs_jpeg_encode_plan");
    const fs_jpeg_info& in = *info;
    if (coef_bytes < in.coef_bytes)
        return set_error(-1, "fs_jpeg_write: coef holds %zu bytes, the image needs %llu", coef_bytes, (unsigned long long)in.coef_bytes);
    const unsigned char* cb = static_cast<const unsigned char*>(coef);
    const int ntab = in.ncomp == 3 ? 2 : 1;
    const unsigned short* qt = reinterpret_cast<const unsigned short*>(cb + in.qt_offset);
    for (int t = 0; t < ntab; ++t)
        for (int i = 0; i < 64; ++i)
            if (qt[64 * t + i] < 1 || qt[64 * t + i] > 255)
                return set_error(-1, "fs_jpeg_write: quantisation table %d, entry %d is %d: a baseline table holds 1..255", t, i, (int)qt[64 * t + i]);

    Sink o;
    o.p = static_cast<unsigned char*>(out);
    o.cap = cap;
    o.be16(0xFFD8);
    static const unsigned char kJfif[16] = {0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1};
    o.bytes(kJfif, 16);
    o.be16(0);                                   // no thumbnail
    for (int t = 0; t < ntab; ++t) {
        o.be16(0xFFDB);
        o.be16(67);
        o.byte((unsigned)t);
        for (int k = 0; k < 64; ++k) o.byte(qt[64 * t + kJpegZigzag[k]]);
    }
    o.be16(0xFFC0);
    o.be16(8 + 3 * (unsigned)in.ncomp);
    o.byte(8);
    o.be16((unsigned)in.height);
    o.be16((unsigned)in.width);
    o.byte((unsigned)in.ncomp);
    for (int c = 0; c < in.ncomp; ++c) {
        o.byte((unsigned)c + 1);
        o.byte((unsigned)(in.hs[c] << 4 | in.vs[c]));
        o.byte((unsigned)in.tq[c]);
    }
    Code dc[2], ac[2];
    for (int t = 0; t < ntab; ++t) {
        build_code(dc[t], kDcBits[t], kDcVals);
        build_code(ac[t], kAcBits[t], kAcVals[t]);
        o.be16(0xFFC4);
        o.be16(2 + 1 + 16 + 12);
        o.byte((unsigned)t);
        o.bytes(kDcBits[t], 16);
        o.bytes(kDcVals, 12);
        o.be16(0xFFC4);
        o.be16(2 + 1 + 16 + 162);
        o.byte(0x10 | (unsigned)t);
        o.bytes(kAcBits[t], 16);
        o.bytes(kAcVals[t], 162);
    }
    o.be16(0xFFDA);
    o.be16(6 + 2 * (unsigned)in.ncomp);
    o.byte((unsigned)in.ncomp);
    for (int c = 0; c < in.ncomp; ++c) {
        o.byte((unsigned)c + 1);
        o.byte(c ? 0x11 : 0x00);
    }
    o.byte(0);
    o.byte(63);
    o.byte(0);
    if (o.full) return set_error(-3, "fs_jpeg_write: out holds %zu bytes, less than the headers", cap);

    int pred[3] = {0, 0, 0};
    for (int my = 0; my < in.mcu_y; ++my) {
        for (int mx = 0; mx < in.mcu_x; ++mx)
            for (int c = 0; c < in.ncomp; ++c) {
                const Code& hd = dc[c ? 1 : 0];
                const Code& ha = ac[c ? 1 : 0];
                for (int v = 0; v < in.vs[c]; ++v)
                    for (int u = 0; u < in.hs[c]; ++u) {
                        const size_t blk = (size_t)(my * in.vs[c] + v) * in.blocks_x[c] + (size_t)(mx * in.hs[c] + u);
                        const int16_t* src = reinterpret_cast<const int16_t*>(cb + in.plane_offset[c]) + blk * 64;
                        const int diff = (int)src[0] - pred[c];
                        pred[c] = src[0];
                        int s = category(diff);
                        if (s > 11) return set_error(-4, "fs_jpeg_write: DC difference %d in MCU (%d, %d) is beyond category 11", diff, mx, my);
                        o.bits((unsigned)hd.code[s] << s | ((unsigned)(diff < 0 ? diff - 1 : diff) & ((1u << s) - 1)), hd.len[s] + s);
                        int run = 0;
                        for (int k = 1; k < 64; ++k) {
                            const int a = src[kJpegZigzag[k]];
                            if (a == 0) {
                                ++run;
                                continue;
                            }
                            for (; run > 15; run -= 16) o.bits(ha.code[0xF0], ha.len[0xF0]);
                            s = category(a);
                            if (s > 10) return set_error(-4, "fs_jpeg_write: AC coefficient %d in MCU (%d, %d) is beyond category 10", a, mx, my);
                            const int sym = run << 4 | s;
                            o.bits((unsigned)ha.code[sym] << s | ((unsigned)(a < 0 ? a - 1 : a) & ((1u << s) - 1)), ha.len[sym] + s);
                            run = 0;
                        }
                        if (run) o.bits(ha.code[0], ha.len[0]);
                    }
            }
        if (o.full) return set_error(-3, "fs_jpeg_write: out holds %zu bytes, too few for the scan (see fs_jpeg_write_bound)", cap);
    }
    o.flush();
    o.be16(0xFFD9);
    if (o.full) return set_error(-3, "fs_jpeg_write: out holds %zu bytes, too few for the scan (see fs_jpeg_write_bound)", cap);
    *n = o.pos;
    return 0;
}

}  // extern "C"
