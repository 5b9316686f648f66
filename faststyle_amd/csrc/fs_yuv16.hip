// Planar YCbCr frames of 9 to 16 bits per sample <-> the net's fp32 NHWC tensors (include/faststyle_io.h, whose comment is the arithmetic
// contract): the deep video path of faststyle_amd/stream.py (source yuv= / yuv_out= with bits=), with no u8 stage on either side.
//   host   -- fs_yuv_plan_deep: fs_yuv_plan's geometry at two bytes per sample, reserved[0] = bits.  The 2^24 fixed-point coefficients are
//             formed per call from the matrix, the range and the depth: there are no tables.
//   device -- one kernel per direction, instantiated per sampling, grid.y = image, the thread layout of fs_yuv.hip: four pixels of a row (and,
//             going to YCbCr, the vs rows of their chroma cell).  No LDS.  Where the width is a multiple of 4, a frame a multiple of 8 bytes, the
//             planes 8-byte and the tensor 16-byte aligned (`vec`, uniform per launch) the four Y samples move as one 8-byte access, the twelve
//             floats as three 16-byte accesses and the thread's chroma samples as one 4- or 8-byte store; as single samples and floats
//             otherwise, with the same values.  Every neighbour index is clamped, a stored sample above 2^bits - 1 reads as that, and no sample
//             value reaches an address.
// Chroma resampling is the common-denominator form of fs_yuv.hip on the d-bit values (16 * 65535 + 8 fits int32); the matrix sums are int64.
#include "../../include/faststyle_io.h"

#include <cmath>
#include <cstring>

#include "fs_kernels.h"

namespace fs {
namespace {

struct DeepToRgbCoef {
    long long cy, r_cr, b_cb, g_cb, g_cr;   // by 2^24: luma scale, R from Cr, B from Cb, G from Cb and Cr (negative)
    int oy, coff, m;                        // luma offset, chroma offset 2^(d-1), 2^d - 1
};

struct DeepToYuvCoef {
    long long y[3], cb[3], cr[3];           // by 2^24, by R, G, B
    long long oy, coff;                     // (offset << 24) + 2^23
    int m;
};

inline long long fix24(double c) { return (long long)floor(c * 16777216.0 + 0.5); }

void deep_constants(const fs_yuv_desc& D, double& Kr, double& Kb, double& Kg, double& sy, double& sc, int& oy, int& coff, int& m) {
#pragma clang fp contract(off)
    const int d = D.reserved[0], k = d - 8;
    m = (1 << d) - 1;
    coff = 1 << (d - 1);
    Kr = D.matrix ? 0.2126 : 0.299;
    Kb = D.matrix ? 0.0722 : 0.114;
    Kg = 1.0 - Kr - Kb;
    sy = D.full_range ? 65280.0 / (double)m : 65280.0 / (219.0 * (double)(1 << k));
    sc = D.full_range ? 65280.0 / (double)m : 65280.0 / (224.0 * (double)(1 << k));
    oy = D.full_range ? 0 : 16 << k;
}

DeepToRgbCoef deep_to_rgb_coef(const fs_yuv_desc& D) {
#pragma clang fp contract(off)
    double Kr, Kb, Kg, sy, sc;
    DeepToRgbCoef c;
    deep_constants(D, Kr, Kb, Kg, sy, sc, c.oy, c.coff, c.m);
    c.cy = fix24(sy);
    c.r_cr = fix24(2.0 * (1.0 - Kr) * sc);
    c.b_cb = fix24(2.0 * (1.0 - Kb) * sc);
    c.g_cb = fix24(-(2.0 * (1.0 - Kb) * Kb / Kg * sc));
    c.g_cr = fix24(-(2.0 * (1.0 - Kr) * Kr / Kg * sc));
    return c;
}

DeepToYuvCoef deep_to_yuv_coef(const fs_yuv_desc& D) {
#pragma clang fp contract(off)
    double Kr, Kb, Kg, sy, sc;
    int oy, coff;
    DeepToYuvCoef c;
    deep_constants(D, Kr, Kb, Kg, sy, sc, oy, coff, c.m);
    const double ry[3] = {Kr, Kg, Kb}, rb[3] = {-Kr, -Kg, 1.0 - Kb}, rr[3] = {1.0 - Kr, -Kg, -Kb};
    for (int k = 0; k < 3; ++k) {
        c.y[k] = fix24(ry[k] / sy);
        c.cb[k] = fix24(rb[k] / (2.0 * (1.0 - Kb)) / sc);
        c.cr[k] = fix24(rr[k] / (2.0 * (1.0 - Kr)) / sc);
    }
    c.oy = ((long long)oy << 24) + (1LL << 23);
    c.coff = ((long long)coff << 24) + (1LL << 23);
    return c;
}

__device__ __forceinline__ int deep_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ int deep_clampl(long long v, int hi) { return v < 0 ? 0 : (v > hi ? hi : (int)v); }
__device__ __forceinline__ int deep_sample(const unsigned short* __restrict__ p, size_t i, int m) {
    const int v = (int)p[i];
    return v > m ? m : v;
}
// the net's float on the 8.8 scale: clamped to [0, 255] (NaN: 0), times 256 (exact), truncated
__device__ __forceinline__ int deep_f88(float v) { return (int)(fminf(fmaxf(v, 0.f), 255.f) * 256.0f); }

// ---------------------------------------------------------------- planes -> fp32 RGB
// Thread i: row y = i / groups, pixels x0 = 4 * (i % groups) ... x0 + 3 (groups = ceil(width / 4)); the chroma taps as in fs_yuv.hip.
template <int HS, int VS>
__global__ __launch_bounds__(256) void yuv_deep_to_f32_kernel(const fs_yuv_desc D, const DeepToRgbCoef K, const unsigned char* __restrict__ yuv,
                                                              int swap_rb, int vec, float* __restrict__ dst) {
    const int groups = (D.width + 3) >> 2;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= groups * D.height) return;
    const int y = i / groups, x0 = (i - y * groups) * 4;
    const int n = D.width - x0 < 4 ? D.width - x0 : 4;
    const int m = K.m;
    const unsigned short* __restrict__ frame = reinterpret_cast<const unsigned short*>(yuv + (size_t)blockIdx.y * D.frame_bytes);
    const unsigned short* __restrict__ yp = frame + (size_t)y * D.width + x0;                     // (plane_offset[0] is 0)
    int Y[4] = {0, 0, 0, 0};
    if (vec) {                                             // (width a multiple of 4: n is 4)
        const uint2 w = *reinterpret_cast<const uint2*>(yp);
        Y[0] = (int)(w.x & 0xFFFFu);
        Y[1] = (int)(w.x >> 16);
        Y[2] = (int)(w.y & 0xFFFFu);
        Y[3] = (int)(w.y >> 16);
#pragma unroll
        for (int k = 0; k < 4; ++k) Y[k] = Y[k] > m ? m : Y[k];
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < n) Y[k] = deep_sample(yp, k, m);
    }
    int cb[4], cr[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) cb[k] = cr[k] = K.coff;
    if (D.ncomp == 3) {
        const int cw = D.chroma_w, ch = D.chroma_h;
        int near_r = y, far_r = y, wn = 4, wf = 0;
        if (VS == 2) {
            near_r = y >> 1;
            far_r = deep_clampi((y & 1) ? near_r + 1 : near_r - 1, 0, ch - 1);
            wn = 3;
            wf = 1;
        }
        const unsigned short* __restrict__ pb = frame + (D.plane_offset[1] >> 1);
        const unsigned short* __restrict__ pr = frame + (D.plane_offset[2] >> 1);
        const size_t rn = (size_t)near_r * cw, rf = (size_t)far_r * cw;
        if (HS == 2) {
            const int c0 = x0 >> 1;
            int vb[4], vr[4];                              // columns c0 - 1 ... c0 + 2, in sixteenths after the horizontal weights below
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = deep_clampi(c0 - 1 + j, 0, cw - 1);
                vb[j] = wn * deep_sample(pb, rn + c, m) + wf * deep_sample(pb, rf + c, m);
                vr[j] = wn * deep_sample(pr, rn + c, m) + wf * deep_sample(pr, rf + c, m);
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
                const int c = deep_clampi(x0 + k, 0, cw - 1);
                cb[k] = deep_sample(pb, rn + c, m);        // (not subsampled: the sample itself)
                cr[k] = deep_sample(pr, rn + c, m);
            }
        }
    }
    float o[12];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const long long l = K.cy * (long long)(Y[k] - K.oy) + (1LL << 23);
        const long long u = cb[k] - K.coff, v = cr[k] - K.coff;
        const float r = (float)deep_clampl((l + K.r_cr * v) >> 24, 65280) * 0.00390625f;
        const float g = (float)deep_clampl((l + K.g_cb * u + K.g_cr * v) >> 24, 65280) * 0.00390625f;
        const float b = (float)deep_clampl((l + K.b_cb * u) >> 24, 65280) * 0.00390625f;
        o[3 * k] = swap_rb ? b : r;
        o[3 * k + 1] = g;
        o[3 * k + 2] = swap_rb ? r : b;
    }
    float* __restrict__ op = dst + (((size_t)blockIdx.y * D.height + y) * D.width + x0) * 3;
    if (vec) {                                             // 48 bytes at a multiple of 48 of a 16-byte aligned tensor
        float4* __restrict__ o4 = reinterpret_cast<float4*>(op);
        o4[0] = make_float4(o[0], o[1], o[2], o[3]);
        o4[1] = make_float4(o[4], o[5], o[6], o[7]);
        o4[2] = make_float4(o[8], o[9], o[10], o[11]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < n) {
                op[3 * k] = o[3 * k];
                op[3 * k + 1] = o[3 * k + 1];
                op[3 * k + 2] = o[3 * k + 2];
            }
    }
}

// ---------------------------------------------------------------- fp32 RGB -> planes
// Thread i: cell row gy = i / groups (luma rows VS * gy ... ), pixels x0 = 4 * (i % groups) ... x0 + 3.  Per row it reads the columns x0 - 1 ...
// x0 + 4 (clamped to the image; the outer two only feed the [1 2 1] taps of co-sited chroma and are read for that layout alone), writes the four
// Y samples, and accumulates the chroma of its cells: two per plane (HS 2) or four (HS 1); a mono frame skips the chroma arithmetic.
template <int HS, int VS>
__global__ __launch_bounds__(256) void f32_to_yuv_deep_kernel(const fs_yuv_desc D, const DeepToYuvCoef K, const float* __restrict__ src, int swap_rb,
                                                              int vec, unsigned char* __restrict__ yuv) {
    const int groups = (D.width + 3) >> 2;
    const int rows = (D.height + VS - 1) / VS;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= groups * rows) return;
    const int gy = i / groups, x0 = (i - gy * groups) * 4;
    const int n = D.width - x0 < 4 ? D.width - x0 : 4;
    const int m = K.m;
    const float* __restrict__ img = src + (size_t)blockIdx.y * D.height * D.width * 3;
    unsigned short* __restrict__ frame = reinterpret_cast<unsigned short*>(yuv + (size_t)blockIdx.y * D.frame_bytes);
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
        const float* __restrict__ row = img + (size_t)ys * D.width * 3;
        float p[6][3];                                           // columns x0 - 1 ... x0 + 4, channels as stored
        if (vec) {
            const float4* __restrict__ w = reinterpret_cast<const float4*>(row + (size_t)x0 * 3);
            const float4 a = w[0], b = w[1], c = w[2];
            p[1][0] = a.x; p[1][1] = a.y; p[1][2] = a.z;
            p[2][0] = a.w; p[2][1] = b.x; p[2][2] = b.y;
            p[3][0] = b.z; p[3][1] = b.w; p[3][2] = c.x;
            p[4][0] = c.y; p[4][1] = c.z; p[4][2] = c.w;
        } else {
#pragma unroll
            for (int j = 1; j < 5; ++j) {
                const float* __restrict__ q = row + (size_t)deep_clampi(x0 - 1 + j, 0, D.width - 1) * 3;
                p[j][0] = q[0]; p[j][1] = q[1]; p[j][2] = q[2];
            }
        }
#pragma unroll
        for (int j = 0; j < 6; j += 5) {
            p[j][0] = p[j][1] = p[j][2] = 0.f;
            if (outer) {
                const float* __restrict__ q = row + (size_t)deep_clampi(x0 - 1 + j, 0, D.width - 1) * 3;
                p[j][0] = q[0]; p[j][1] = q[1]; p[j][2] = q[2];
            }
        }
        int cbv[6], crv[6], yv[4];
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            const long long c0 = deep_f88(p[j][0]), G = deep_f88(p[j][1]), c2 = deep_f88(p[j][2]);
            const long long R = swap_rb ? c2 : c0, B = swap_rb ? c0 : c2;
            if (j >= 1 && j <= 4) yv[j - 1] = deep_clampl((K.y[0] * R + K.y[1] * G + K.y[2] * B + K.oy) >> 24, m);
            cbv[j] = crv[j] = 0;
            if (chroma && (outer || (j >= 1 && j <= 4))) {       // (mono has no chroma; the outer columns carry weight 0 unless co-sited)
                cbv[j] = deep_clampl((K.cb[0] * R + K.cb[1] * G + K.cb[2] * B + K.coff) >> 24, m);
                crv[j] = deep_clampl((K.cr[0] * R + K.cr[1] * G + K.cr[2] * B + K.coff) >> 24, m);
            }
        }
        if (yy < D.height) {
            unsigned short* __restrict__ yp = frame + (size_t)yy * D.width + x0;
            if (vec) {
                *reinterpret_cast<uint2*>(yp) = make_uint2((unsigned)yv[0] | ((unsigned)yv[1] << 16), (unsigned)yv[2] | ((unsigned)yv[3] << 16));
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (k < n) yp[k] = (unsigned short)yv[k];
            }
        }
        const int wy = VS == 2 ? 1 : 2;
#pragma unroll
        for (int j = 0; chroma && j < NC; ++j) {
            if (HS == 2) {
                const int c = 1 + 2 * j;                         // column 2c of cell c0 + j; its right neighbour is clamped by the load
                sb[j] += wy * (wl * cbv[c - 1] + 2 * cbv[c] + wr * cbv[c + 1]);
                sr[j] += wy * (wl * crv[c - 1] + 2 * crv[c] + wr * crv[c + 1]);
            } else {
                sb[j] += wy * 4 * cbv[1 + j];
                sr[j] += wy * 4 * crv[1 + j];
            }
        }
    }
    if (!chroma) return;
    const int cw = D.chroma_w;
    const int c0 = x0 / HS;
    unsigned short* __restrict__ ob = frame + (D.plane_offset[1] >> 1) + (size_t)gy * cw + c0;
    unsigned short* __restrict__ orr = frame + (D.plane_offset[2] >> 1) + (size_t)gy * cw + c0;
    unsigned vb[NC], vr[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        vb[j] = (unsigned)((sb[j] + 4) >> 3);
        vr[j] = (unsigned)((sr[j] + 4) >> 3);
    }
    if (vec) {                                                   // (width a multiple of 4: every cell of the thread is inside the plane)
        if (HS == 2) {
            *reinterpret_cast<unsigned*>(ob) = vb[0] | (vb[1] << 16);
            *reinterpret_cast<unsigned*>(orr) = vr[0] | (vr[1] << 16);
        } else {
            *reinterpret_cast<uint2*>(ob) = make_uint2(vb[0] | (vb[1] << 16), vb[NC - 2] | (vb[NC - 1] << 16));
            *reinterpret_cast<uint2*>(orr) = make_uint2(vr[0] | (vr[1] << 16), vr[NC - 2] | (vr[NC - 1] << 16));
        }
    } else {
#pragma unroll
        for (int j = 0; j < NC; ++j)
            if (c0 + j < cw) {
                ob[j] = (unsigned short)vb[j];
                orr[j] = (unsigned short)vr[j];
            }
    }
}

// the wide path: a width that is a multiple of 4 and frames of a multiple of 8 bytes (then every Y row starts at a multiple of 8 bytes, every
// chroma plane and row at a multiple of 4, and of 8 where chroma is not subsampled), planes 8-byte and tensor 16-byte aligned
inline int wide_path(const fs_yuv_desc& D, const void* yuv, const void* f32) {
    return (D.width & 3) == 0 && (D.frame_bytes & 7) == 0 && ((uintptr_t)yuv & 7) == 0 && ((uintptr_t)f32 & 15) == 0;
}

}  // namespace

bool yuv_deep_desc_ok(const fs_yuv_desc& d) {
    fs_yuv_desc want;
    if (fs_yuv_plan_deep(d.width, d.height, d.hs, d.vs, d.ncomp, d.siting, d.matrix, d.full_range, d.reserved[0], &want)) return false;
    return !memcmp(&want, &d, sizeof(want));
}

// desc: checked by the caller (fs_api.hip: yuv_deep_desc_ok)
int yuv_deep_to_f32(const fs_yuv_desc& D, const unsigned char* yuv, int N, int swap_rb, float* dst, hipStream_t s) {
    const DeepToRgbCoef K = deep_to_rgb_coef(D);
    const int vec = wide_path(D, yuv, dst);
    const dim3 grid((unsigned)((((long long)(D.width + 3) >> 2) * D.height + 255) / 256), (unsigned)N), block(256);
    if (D.hs == 2 && D.vs == 2) hipLaunchKernelGGL((yuv_deep_to_f32_kernel<2, 2>), grid, block, 0, s, D, K, yuv, swap_rb, vec, dst);
    else if (D.hs == 2) hipLaunchKernelGGL((yuv_deep_to_f32_kernel<2, 1>), grid, block, 0, s, D, K, yuv, swap_rb, vec, dst);
    else hipLaunchKernelGGL((yuv_deep_to_f32_kernel<1, 1>), grid, block, 0, s, D, K, yuv, swap_rb, vec, dst);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

int f32_to_yuv_deep(const fs_yuv_desc& D, const float* src, int swap_rb, int N, unsigned char* yuv, hipStream_t s) {
    const DeepToYuvCoef K = deep_to_yuv_coef(D);
    const int vec = wide_path(D, yuv, src);
    const long long rows = (D.height + D.vs - 1) / D.vs;
    const dim3 grid((unsigned)((((long long)(D.width + 3) >> 2) * rows + 255) / 256), (unsigned)N), block(256);
    if (D.hs == 2 && D.vs == 2) hipLaunchKernelGGL((f32_to_yuv_deep_kernel<2, 2>), grid, block, 0, s, D, K, src, swap_rb, vec, yuv);
    else if (D.hs == 2) hipLaunchKernelGGL((f32_to_yuv_deep_kernel<2, 1>), grid, block, 0, s, D, K, src, swap_rb, vec, yuv);
    else hipLaunchKernelGGL((f32_to_yuv_deep_kernel<1, 1>), grid, block, 0, s, D, K, src, swap_rb, vec, yuv);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace fs

extern "C" {

int fs_yuv_plan_deep(int width, int height, int hs, int vs, int ncomp, int siting, int matrix, int full_range, int bits, fs_yuv_desc* desc) {
    using namespace fs;
    if (!desc) return set_error(-1, "fs_yuv_plan_deep: null argument");
    fs_yuv_desc d;
    const int rc = fs_yuv_plan(width, height, hs, vs, ncomp, siting, matrix, full_range, &d);
    if (rc) return rc;                                          // (the message is fs_yuv_plan's)
    if (bits < 9 || bits > 16)
        return set_error(-2, "fs_yuv_plan_deep: %d bits per sample is outside [9, 16] (8-bit frames: fs_yuv_plan)", bits);
    d.reserved[0] = bits;
    for (int k = 0; k < 3; ++k) {
        d.plane_offset[k] *= 2;
        d.plane_bytes[k] *= 2;
    }
    d.frame_bytes *= 2;
    *desc = d;
    return 0;
}

}  // extern "C"
