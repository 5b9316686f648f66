// What the baseline JPEG decoder (fs_jpeg.hip) and encoder (fs_jpegenc.hip) share: the geometry of a coefficient buffer
// (include/faststyle_io.h: fs_jpeg_info) and the zigzag order.
#pragma once
#include "../../include/faststyle_io.h"

#include "fs_kernels.h"

namespace fs {

struct JpegGeom {
    int bw[3], bh[3];                 // blocks per row / column of each component plane (whole MCUs)
    unsigned long long plane[3];      // byte offset of each plane from the image's coefficient offset
    unsigned long long coef_count;    // int16 coefficients of all planes
    int cw, ch;                       // true chroma extent: ceil(W / hs), ceil(H / vs)
};

__host__ __device__ inline void jpeg_geom(int W, int H, int ncomp, int hs, int vs, JpegGeom& g) {
    const int mx = (W + 8 * hs - 1) / (8 * hs), my = (H + 8 * vs - 1) / (8 * vs);
    unsigned long long off = 0;
    for (int c = 0; c < 3; ++c) {
        g.bw[c] = c < ncomp ? mx * (c ? 1 : hs) : 0;
        g.bh[c] = c < ncomp ? my * (c ? 1 : vs) : 0;
        g.plane[c] = off;
        off += (unsigned long long)g.bw[c] * g.bh[c] * 128;
    }
    g.coef_count = off / 2;
    g.cw = (W + hs - 1) / hs;
    g.ch = (H + vs - 1) / vs;
}

// the derived fields of an fs_jpeg_info whose width, height, ncomp, hs[0] and vs[0] are set
inline void jpeg_fill_info(fs_jpeg_info& in) {
    JpegGeom g;
    jpeg_geom(in.width, in.height, in.ncomp, in.hs[0], in.vs[0], g);
    in.mcu_x = g.bw[0] / in.hs[0];
    in.mcu_y = g.bh[0] / in.vs[0];
    for (int c = 0; c < 3; ++c) {
        in.blocks_x[c] = g.bw[c];
        in.blocks_y[c] = g.bh[c];
        in.plane_offset[c] = g.plane[c];
    }
    in.coef_count = g.coef_count;
    in.qt_offset = (g.coef_count * 2 + 15) & ~15ull;
    in.coef_bytes = in.qt_offset + 384;
    in.rgb_bytes = (uint64_t)in.width * in.height * 3;
}

// natural (row-major) position of the k-th coefficient in zigzag order
constexpr unsigned char kJpegZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                           41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                           30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

}  // namespace fs
