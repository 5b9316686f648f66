// Planar 8-bit YCbCr frames <-> packed RGB (include/faststyle_io.h, whose comment is the arithmetic contract): the colour conversion of raw
// video streams, inside the lane's captured graph (faststyle_amd/stream.py, source yuv= / yuv_out=).
//   host   -- fs_yuv_plan: the plane geometry of one frame; plain C++ with no global state and no allocation.  The 16-bit fixed-point
//             coefficients are formed per call from the matrix and the range: there are no tables.
//   device -- one kernel per direction, instantiated per sampling and pixel size, grid.y = image.  A thread takes four pixels of a row (and, going
//             to YCbCr, the vs rows of their chroma cell).  Bandwidth-trivial: no LDS; the Y samples and packed pixels move as dwords where the
//             width is a multiple of 4 and the buffers are 4-byte aligned (`vec`, uniform per launch), as bytes otherwise; the chroma taps of
//             neighbouring lanes share cache lines.  Every neighbour index is clamped, and no sample value reaches an address.
// Upsampling and downsampling are written with common denominators: a pixel's chroma is (sum wx * wy * C + 8) >> 4 with wx, wy in quarters
// ((3, 1) centre, (4, 0) own sample, (2, 2) between two co-sited samples), a chroma sample is (sum over the cell's rows and the columns
// 2c - 1, 2c, 2c + 1 + 4) >> 3 with column weights (0, 2, 2) centre, (1, 2, 1) co-sited, (0, 4, 0) not subsampled, and row weight 1 (two rows)
// or 2 (one row): the same integers as the per-case forms of the header, which are these with the common factor divided out.
#include "../../include/faststyle_io.h"

#include <cmath>
#include <cstring>

#include "fs_kernels.h"

namespace fs {
namespace {

constexpr int kYuvMaxSide = 32767;

struct YuvToRgbCoef {
    int cy, oy;            // luma scale, luma offset
    int r_cr, b_cb;        // R from Cr - 128, B from Cb - 128
    int g_cb, g_cr;        // (negative)
};

struct RgbToYuvCoef {
    int y[3], cb[3], cr[3];   // by R, G, B
    int oy;
};

inline int fix16(double c) { return (int)floor(c * 65536.0 + 0.5); }

void matrix_constants(const fs_yuv_desc& D, double& Kr, double& Kb, double& Kg, double& sy, double& sc, int& oy) {
#pragma clang fp contract(off)
    Kr = D.matrix ? 0.2126 : 0.299;
    Kb = D.matrix ? 0.0722 : 0.114;
    Kg = 1.0 - Kr - Kb;
    sy = D.full_range ? 1.0 : 255.0 / 219.0;
    sc = D.full_range ? 1.0 : 255.0 / 224.0;
    oy = D.full_range ? 0 : 16;
}

YuvToRgbCoef yuv_to_rgb_coef(const fs_yuv_desc& D) {
#pragma clang fp contract(off)
    double Kr, Kb, Kg, sy, sc;
    YuvToRgbCoef c;
    matrix_constants(D, Kr, Kb, Kg, sy, sc, c.oy);
    c.cy = fix16(sy);
    c.r_cr = fix16(2.0 * (1.0 - Kr) * sc);
    c.b_cb = fix16(2.0 * (1.0 - Kb) * sc);
    c.g_cb = fix16(-(2.0 * (1.0 - Kb) * Kb / Kg * sc));
    c.g_cr = fix16(-(2.0 * (1.0 - Kr) * Kr / Kg * sc));
    return c;
}

RgbToYuvCoef rgb_to_yuv_coef(const fs_yuv_desc& D) {
#pragma clang fp contract(off)
    double Kr, Kb, Kg, sy, sc;
    RgbToYuvCoef c;
    matrix_constants(D, Kr, Kb, Kg, sy, sc, c.oy);
    const double ry[3] = {Kr, Kg, Kb}, rb[3] = {-Kr, -Kg, 1.0 - Kb}, rr[3] = {1.0 - Kr, -Kg, -Kb};
    for (int k = 0; k < 3; ++k) {
        c.y[k] = fix16(ry[k] / sy);
        c.cb[k] = fix16(rb[k] / (2.0 * (1.0 - Kb)) / sc);
        c.cr[k] = fix16(rr[k] / (2.0 * (1.0 - Kr)) / sc);
    }
    return c;
}

__device__ __forceinline__ int yuv_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ int yuv_u8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// ---------------------------------------------------------------- YCbCr -> RGB
// Thread i: row y = i / groups, pixels x0 = 4 * (i % groups) ... x0 + 3 (groups = ceil(width / 4)).  Their chroma cells are columns c0 and
// c0 + 1 (HS 2) and the taps reach c0 - 1 ... c0 + 2: four clamped columns of the near and the far chroma row, combined vertically first.
template <int PB, int HS, int VS>
__global__ __launch_bounds__(256) void yuv_to_rgb_kernel(const fs_yuv_desc D, const YuvToRgbCoef K, const unsigned char* __restrict__ yuv, int swap_rb,
                                                         int vec, unsigned char* __restrict__ rgb) {
    const int groups = (D.width + 3) >> 2;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= groups * D.height) return;
    const int y = i / groups, x0 = (i - y * groups) * 4;
    const int n = D.width - x0 < 4 ? D.width - x0 : 4;
    const unsigned char* __restrict__ frame = yuv + (size_t)blockIdx.y * D.frame_bytes;
    const unsigned char* __restrict__ yp = frame + D.plane_offset[0] + (size_t)y * D.width + x0;
    int Y[4] = {0, 0, 0, 0};
    if (vec) {                                             // (width a multiple of 4: n is 4)
        const unsigned w = *reinterpret_cast<const unsigned*>(yp);
#pragma unroll
        for (int k = 0; k < 4; ++k) Y[k] = (int)((w >> (8 * k)) & 255);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < n) Y[k] = yp[k];
    }
    int cb[4] = {128, 128, 128, 128}, cr[4] = {128, 128, 128, 128};
    if (D.ncomp == 3) {
        const int cw = D.chroma_w, ch = D.chroma_h;
        int near_r = y, far_r = y, wn = 4, wf = 0;
        if (VS == 2) {
            near_r = y >> 1;
            far_r = yuv_clampi((y & 1) ? near_r + 1 : near_r - 1, 0, ch - 1);
            wn = 3;
            wf = 1;
        }
        const unsigned char* __restrict__ pb = frame + D.plane_offset[1];
        const unsigned char* __restrict__ pr = frame + D.plane_offset[2];
        const size_t rn = (size_t)near_r * cw, rf = (size_t)far_r * cw;
        if (HS == 2) {
            const int c0 = x0 >> 1;
            int vb[4], vr[4];                              // columns c0 - 1 ... c0 + 2, in sixteenths after the horizontal weights below
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = yuv_clampi(c0 - 1 + j, 0, cw - 1);
                vb[j] = wn * (int)pb[rn + c] + wf * (int)pb[rf + c];
                vr[j] = wn * (int)pr[rn + c] + wf * (int)pr[rf + c];
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int own = 1 + (k >> 1);
                int sb, sr;
                if (D.siting == 0) {                       // centre: three quarters of the own sample, one of the neighbour on the pixel's side
                    const int far = (k & 1) ? own + 1 : own - 1;
                    sb = 3 * vb[own] + vb[far];
                    sr = 3 * vr[own] + vr[far];
                } else if (k & 1) {                        // co-sited, odd column: half way between two samples
                    sb = 2 * vb[own] + 2 * vb[own + 1];
                    sr = 2 * vr[own] + 2 * vr[own + 1];
                } else {                                   // co-sited, even column: the sample's own position
                    sb = 4 * vb[own];
                    sr = 4 * vr[own];
                }
                cb[k] = (sb + 8) >> 4;
                cr[k] = (sr + 8) >> 4;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int c = yuv_clampi(x0 + k, 0, cw - 1);
                cb[k] = (4 * (wn * (int)pb[rn + c] + wf * (int)pb[rf + c]) + 8) >> 4;
                cr[k] = (4 * (wn * (int)pr[rn + c] + wf * (int)pr[rf + c]) + 8) >> 4;
            }
        }
    }
    unsigned px[4];                                        // byte 0, 1, 2 as stored, byte 3 = 255
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int l = K.cy * (Y[k] - K.oy) + 32768;
        const int u = cb[k] - 128, v = cr[k] - 128;
        const int r = yuv_u8((l + K.r_cr * v) >> 16);
        const int g = yuv_u8((l + K.g_cb * u + K.g_cr * v) >> 16);
        const int b = yuv_u8((l + K.b_cb * u) >> 16);
        px[k] = (unsigned)(swap_rb ? b : r) | ((unsigned)g << 8) | ((unsigned)(swap_rb ? r : b) << 16) | 0xFF000000u;
    }
    const size_t pixel = ((size_t)blockIdx.y * D.height + y) * D.width + x0;
    if (PB == 4) {                                         // (rgb is 4-byte aligned: checked by the caller)
        unsigned* __restrict__ o = reinterpret_cast<unsigned*>(rgb) + pixel;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < n) o[k] = px[k];
    } else if (vec) {                                      // 12 bytes at a multiple of 12
        unsigned* __restrict__ o = reinterpret_cast<unsigned*>(rgb + pixel * 3);
        o[0] = (px[0] & 0xFFFFFFu) | (px[1] << 24);
        o[1] = ((px[1] >> 8) & 0xFFFFu) | (px[2] << 16);
        o[2] = ((px[2] >> 16) & 0xFFu) | (px[3] << 8);
    } else {
        unsigned char* __restrict__ o = rgb + pixel * 3;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < n) {
                o[3 * k] = (unsigned char)(px[k] & 255);
                o[3 * k + 1] = (unsigned char)((px[k] >> 8) & 255);
                o[3 * k + 2] = (unsigned char)((px[k] >> 16) & 255);
            }
    }
}

// ---------------------------------------------------------------- RGB -> YCbCr
// Thread i: cell row gy = i / groups (luma rows VS * gy ... ), pixels x0 = 4 * (i % groups) ... x0 + 3.  Per row it reads the columns x0 - 1 ...
// x0 + 4 (clamped to the image; the outer two only feed the [1 2 1] taps of co-sited chroma and are read for that layout alone), writes the four
// Y samples, and accumulates the chroma of its cells: two per plane (HS 2) or four (HS 1); a mono frame skips the chroma arithmetic.
template <int PB, int HS, int VS>
__global__ __launch_bounds__(256) void rgb_to_yuv_kernel(const fs_yuv_desc D, const RgbToYuvCoef K, const unsigned char* __restrict__ rgb, int swap_rb,
                                                         int vec, unsigned char* __restrict__ yuv) {
    const int groups = (D.width + 3) >> 2;
    const int rows = (D.height + VS - 1) / VS;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= groups * rows) return;
    const int gy = i / groups, x0 = (i - gy * groups) * 4;
    const int n = D.width - x0 < 4 ? D.width - x0 : 4;
    const unsigned char* __restrict__ img = rgb + (size_t)blockIdx.y * D.height * D.width * PB;
    unsigned char* __restrict__ frame = yuv + (size_t)blockIdx.y * D.frame_bytes;
    const bool chroma = D.ncomp == 3;
    constexpr int NC = HS == 2 ? 2 : 4;                    // chroma cells of this thread
    int sb[NC], sr[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) sb[j] = sr[j] = 0;
    const int wl = D.siting ? 1 : 0, wr = D.siting ? 1 : 2;       // column weights about 2c (HS 2): (0, 2, 2) centre, (1, 2, 1) co-sited
    const bool outer = chroma && HS == 2 && D.siting;             // only the [1 2 1] taps reach the columns x0 - 1 and x0 + 4
#pragma unroll
    for (int r = 0; r < VS; ++r) {
        const int yy = VS * gy + r;
        const int ys = yy < D.height ? yy : D.height - 1;         // (an odd height: the last row twice)
        const unsigned char* __restrict__ row = img + (size_t)ys * D.width * PB;
        unsigned p[6];                                           // columns x0 - 1 ... x0 + 4 as R | G << 8 | B << 16 (| anything << 24)
        if (PB == 4) {
#pragma unroll
            for (int j = 0; j < 6; ++j)
                p[j] = (outer || (j >= 1 && j <= 4)) ? reinterpret_cast<const unsigned*>(row)[yuv_clampi(x0 - 1 + j, 0, D.width - 1)] : 0u;
        } else {
            if (vec) {
                const unsigned* __restrict__ w = reinterpret_cast<const unsigned*>(row + (size_t)x0 * 3);
                const unsigned a = w[0], b = w[1], c = w[2];
                p[1] = a;
                p[2] = (a >> 24) | (b << 8);
                p[3] = (b >> 16) | (c << 16);
                p[4] = c >> 8;
            } else {
#pragma unroll
                for (int j = 1; j < 5; ++j) {
                    const unsigned char* __restrict__ q = row + (size_t)yuv_clampi(x0 - 1 + j, 0, D.width - 1) * 3;
                    p[j] = (unsigned)q[0] | ((unsigned)q[1] << 8) | ((unsigned)q[2] << 16);
                }
            }
            p[0] = p[5] = 0;
            if (outer) {
#pragma unroll
                for (int j = 0; j < 6; j += 5) {
                    const unsigned char* __restrict__ q = row + (size_t)yuv_clampi(x0 - 1 + j, 0, D.width - 1) * 3;
                    p[j] = (unsigned)q[0] | ((unsigned)q[1] << 8) | ((unsigned)q[2] << 16);
                }
            }
        }
        int cbv[6], crv[6];
        unsigned yw = 0;
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            const int c0 = (int)(p[j] & 255), G = (int)((p[j] >> 8) & 255), c2 = (int)((p[j] >> 16) & 255);
            const int R = swap_rb ? c2 : c0, B = swap_rb ? c0 : c2;
            if (j >= 1 && j <= 4) yw |= (unsigned)yuv_u8((K.y[0] * R + K.y[1] * G + K.y[2] * B + (K.oy << 16) + 32768) >> 16) << (8 * (j - 1));
            cbv[j] = crv[j] = 0;
            if (chroma && (outer || (j >= 1 && j <= 4))) {       // (mono has no chroma; the outer columns carry weight 0 unless co-sited)
                cbv[j] = yuv_u8((K.cb[0] * R + K.cb[1] * G + K.cb[2] * B + (128 << 16) + 32768) >> 16);
                crv[j] = yuv_u8((K.cr[0] * R + K.cr[1] * G + K.cr[2] * B + (128 << 16) + 32768) >> 16);
            }
        }
        if (yy < D.height) {
            unsigned char* __restrict__ yp = frame + D.plane_offset[0] + (size_t)yy * D.width + x0;
            if (vec) {
                *reinterpret_cast<unsigned*>(yp) = yw;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (k < n) yp[k] = (unsigned char)((yw >> (8 * k)) & 255);
            }
        }
        const int wy = VS == 2 ? 1 : 2;
#pragma unroll
        for (int j = 0; chroma && j < NC; ++j) {
            if (HS == 2) {
                const int m = 1 + 2 * j;                         // column 2c of cell c0 + j; its right neighbour is clamped by the load
                sb[j] += wy * (wl * cbv[m - 1] + 2 * cbv[m] + wr * cbv[m + 1]);
                sr[j] += wy * (wl * crv[m - 1] + 2 * crv[m] + wr * crv[m + 1]);
            } else {
                sb[j] += wy * 4 * cbv[1 + j];
                sr[j] += wy * 4 * crv[1 + j];
            }
        }
    }
    if (!chroma) return;
    const int cw = D.chroma_w;
    const int c0 = x0 / HS;
    unsigned char* __restrict__ ob = frame + D.plane_offset[1] + (size_t)gy * cw + c0;
    unsigned char* __restrict__ orr = frame + D.plane_offset[2] + (size_t)gy * cw + c0;
#pragma unroll
    for (int j = 0; j < NC; ++j)
        if (c0 + j < cw) {
            ob[j] = (unsigned char)((sb[j] + 4) >> 3);
            orr[j] = (unsigned char)((sr[j] + 4) >> 3);
        }
}

template <int PB>
int launch_to_rgb(const fs_yuv_desc& D, const unsigned char* yuv, int N, int swap_rb, int vec, unsigned char* rgb, hipStream_t s) {
    const YuvToRgbCoef K = yuv_to_rgb_coef(D);
    const dim3 grid((unsigned)((((long long)(D.width + 3) >> 2) * D.height + 255) / 256), (unsigned)N), block(256);
    if (D.hs == 2 && D.vs == 2) hipLaunchKernelGGL((yuv_to_rgb_kernel<PB, 2, 2>), grid, block, 0, s, D, K, yuv, swap_rb, vec, rgb);
    else if (D.hs == 2) hipLaunchKernelGGL((yuv_to_rgb_kernel<PB, 2, 1>), grid, block, 0, s, D, K, yuv, swap_rb, vec, rgb);
    else hipLaunchKernelGGL((yuv_to_rgb_kernel<PB, 1, 1>), grid, block, 0, s, D, K, yuv, swap_rb, vec, rgb);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

template <int PB>
int launch_to_yuv(const fs_yuv_desc& D, const unsigned char* rgb, int N, int swap_rb, int vec, unsigned char* yuv, hipStream_t s) {
    const RgbToYuvCoef K = rgb_to_yuv_coef(D);
    const long long rows = (D.height + D.vs - 1) / D.vs;
    const dim3 grid((unsigned)((((long long)(D.width + 3) >> 2) * rows + 255) / 256), (unsigned)N), block(256);
    if (D.hs == 2 && D.vs == 2) hipLaunchKernelGGL((rgb_to_yuv_kernel<PB, 2, 2>), grid, block, 0, s, D, K, rgb, swap_rb, vec, yuv);
    else if (D.hs == 2) hipLaunchKernelGGL((rgb_to_yuv_kernel<PB, 2, 1>), grid, block, 0, s, D, K, rgb, swap_rb, vec, yuv);
    else hipLaunchKernelGGL((rgb_to_yuv_kernel<PB, 1, 1>), grid, block, 0, s, D, K, rgb, swap_rb, vec, yuv);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

// the dword path: a width that is a multiple of 4 (then every plane, row and frame starts at a multiple of 4) and 4-byte aligned buffers
inline int dword_path(const fs_yuv_desc& D, const void* yuv, const void* rgb) {
    return (D.width & 3) == 0 && (D.frame_bytes & 3) == 0 && (((uintptr_t)yuv | (uintptr_t)rgb) & 3) == 0;
}

}  // namespace

bool yuv_desc_ok(const fs_yuv_desc& d) {
    fs_yuv_desc want;
    if (fs_yuv_plan(d.width, d.height, d.hs, d.vs, d.ncomp, d.siting, d.matrix, d.full_range, &want)) return false;
    return !memcmp(&want, &d, sizeof(want));
}

// desc: checked by the caller (fs_api.hip: yuv_desc_ok); pixel_bytes 3 or 4
int yuv_to_rgb_u8(const fs_yuv_desc& D, const unsigned char* yuv, int N, int pixel_bytes, int swap_rb, unsigned char* rgb, hipStream_t s) {
    const int vec = dword_path(D, yuv, rgb);
    return pixel_bytes == 4 ? launch_to_rgb<4>(D, yuv, N, swap_rb, vec, rgb, s) : launch_to_rgb<3>(D, yuv, N, swap_rb, vec, rgb, s);
}

int rgb_to_yuv_u8(const fs_yuv_desc& D, const unsigned char* rgb, int pixel_bytes, int swap_rb, int N, unsigned char* yuv, hipStream_t s) {
    const int vec = dword_path(D, yuv, rgb);
    return pixel_bytes == 4 ? launch_to_yuv<4>(D, rgb, N, swap_rb, vec, yuv, s) : launch_to_yuv<3>(D, rgb, N, swap_rb, vec, yuv, s);
}

}  // namespace fs

extern "C" {

int fs_yuv_plan(int width, int height, int hs, int vs, int ncomp, int siting, int matrix, int full_range, fs_yuv_desc* desc) {
    using namespace fs;
    if (!desc) return set_error(-1, "fs_yuv_plan: null argument");
    if (width < 1 || height < 1 || width > kYuvMaxSide || height > kYuvMaxSide)
        return set_error(-1, "fs_yuv_plan: frame %dx%d outside [1, %d]", width, height, kYuvMaxSide);
    if (!((hs == 1 && vs == 1) || (hs == 2 && vs == 1) || (hs == 2 && vs == 2)))
        return set_error(-2, "fs_yuv_plan: sampling %dx%d is none of 1x1 (4:4:4), 2x1 (4:2:2), 2x2 (4:2:0)", hs, vs);
    if (ncomp != 3 && ncomp != 1) return set_error(-2, "fs_yuv_plan: %d components: 3, or 1 for mono", ncomp);
    if (ncomp == 1 && hs != 1) return set_error(-2, "fs_yuv_plan: a mono frame has sampling 1x1, got %dx%d", hs, vs);
    if ((siting | 1) != 1) return set_error(-2, "fs_yuv_plan: siting %d is neither 0 (centre) nor 1 (co-sited)", siting);
    if ((matrix | 1) != 1) return set_error(-2, "fs_yuv_plan: matrix %d is neither 0 (BT.601) nor 1 (BT.709)", matrix);
    if ((full_range | 1) != 1) return set_error(-2, "fs_yuv_plan: full_range %d is neither 0 nor 1", full_range);
    memset(desc, 0, sizeof(*desc));
    desc->width = width;
    desc->height = height;
    desc->hs = hs;
    desc->vs = vs;
    desc->ncomp = ncomp;
    desc->siting = siting;
    desc->matrix = matrix;
    desc->full_range = full_range;
    desc->plane_bytes[0] = (uint64_t)width * height;
    if (ncomp == 3) {
        desc->chroma_w = (width + hs - 1) / hs;
        desc->chroma_h = (height + vs - 1) / vs;
        desc->plane_bytes[1] = desc->plane_bytes[2] = (uint64_t)desc->chroma_w * desc->chroma_h;
        desc->plane_offset[1] = desc->plane_bytes[0];
        desc->plane_offset[2] = desc->plane_offset[1] + desc->plane_bytes[1];
    }
    desc->frame_bytes = desc->plane_bytes[0] + desc->plane_bytes[1] + desc->plane_bytes[2];
    return 0;
}

}  // extern "C"
