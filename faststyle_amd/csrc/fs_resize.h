// TF1 bicubic resize arithmetic shared by the single-image kernel (fs_io.hip) and the many-image kernel of the device-fed
// input path (fs_feed.hip): both call resize_bicubic_pixel, so their results are the same bits by construction.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>

namespace fs {

// ---------------------------------------------------------------- TF1 bicubic resize
// One thread per output pixel (3 channels).  Every product and sum is rounded separately, in TF's order
// (`#pragma clang fp contract(off)`: hipcc's default would fuse a*b+c into FMAs), so the result is bit-identical
// to the float32 restatement in oracle/datapipe.py.
__device__ __forceinline__ float bicubic_near(float x) {
#pragma clang fp contract(off)
    // TF's coefficient table entry 2i, x = i/1024:  ((a+2)x - (a+3)) x x + 1, a = -0.75
    float t = 1.25f * x;
    t = t - 2.25f;
    t = t * x;
    t = t * x;
    return t + 1.0f;
}
__device__ __forceinline__ float bicubic_far(float x) {
#pragma clang fp contract(off)
    // entry 2i+1 (x += 1):  ((a x - 5a) x + 8a) x - 4a
    x = x + 1.0f;
    float t = -0.75f * x;
    t = t - (-3.75f);
    t = t * x;
    t = t + (-6.0f);
    t = t * x;
    return t - (-3.0f);
}
__device__ __forceinline__ void bicubic_weights(float scale, int out_loc, int limit, float w[4], int idx[4]) {
#pragma clang fp contract(off)
    const float in_f = scale * (float)out_loc;
    const int in_loc = (int)in_f;  // in_loc >= 0: truncation == floor
    const float delta = in_f - (float)in_loc;
    const int offset = (int)lrintf(delta * 1024.0f);
    const float x0 = (float)offset * (1.0f / 1024.0f), x1 = (float)(1024 - offset) * (1.0f / 1024.0f);  // exact
    w[0] = bicubic_far(x0);
    w[1] = bicubic_near(x0);
    w[2] = bicubic_near(x1);
    w[3] = bicubic_far(x1);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        int i = in_loc - 1 + k;
        idx[k] = i < 0 ? 0 : (i > limit - 1 ? limit - 1 : i);
    }
}
__device__ __forceinline__ float interp1d(const float w[4], float v0, float v1, float v2, float v3) {
#pragma clang fp contract(off)
    const float p0 = v0 * w[0], p1 = v1 * w[1], p2 = v2 * w[2], p3 = v3 * w[3];
    float acc = p0 + p1;
    acc = acc + p2;
    return acc + p3;
}

// One output pixel (3 channels) of the resize.  PB = bytes per source pixel: 3 (packed RGB) or 4 (RGBX -- PIL's own storage of an RGB image,
// which the host hands over as it is: no repack under the interpreter lock; the fourth byte is never read).  i = oy * Wo + ox; dst = the
// [Ho,Wo,3] image.
template <int PB>
__device__ __forceinline__ void resize_bicubic_pixel(const unsigned char* __restrict__ src, int H, int W, float* __restrict__ dst, int Wo,
                                                     float hs, float ws, int i) {
    const int oy = i / Wo, ox = i - oy * Wo;
    float wy[4], wx[4];
    int iy[4], ix[4];
    bicubic_weights(hs, oy, H, wy, iy);
    bicubic_weights(ws, ox, W, wx, ix);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float col[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const unsigned char* row = src + ((size_t)iy[r] * W) * PB + c;
            col[r] = interp1d(wx, (float)row[ix[0] * PB], (float)row[ix[1] * PB], (float)row[ix[2] * PB], (float)row[ix[3] * PB]);
        }
        dst[(size_t)i * 3 + c] = interp1d(wy, col[0], col[1], col[2], col[3]);
    }
}

}  // namespace fs
