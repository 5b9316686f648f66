// Two styles per stream (include/faststyle_io.h, whose comment is the arithmetic contract): the fp32 outputs of two nets merged on the unsigned
// 8.8 scale of compose, by one weight per image and an optional region mask, ahead of fs_compose_f32 and every output conversion of
// faststyle_amd/stream.py (mix=).
//   device -- one kernel, grid.y = image, the thread layout of fs_compose.hip: four pixels of an output row.  No LDS, no tables.  The weight of
//             an image is a kernel argument or, with weight_dev, one int32 read from device memory and clamped to [0, 256] (uniform per block:
//             one captured graph serves every frame of a fade).  Both tensors have the output's size; the mask has the net's input size, up
//             to 3 rows and columns less, and is read at (min(y, H - 1), min(x, W - 1)).  Where the width is a multiple of 4 and the three
//             tensors are 16-byte aligned (`wide`, uniform per launch) the twelve floats of a thread move as three 16-byte accesses per tensor,
//             and the four mask bytes as one dword where W == Wo and the mask is 4-byte aligned; as single floats and bytes otherwise, with the
//             same values.  No value read from a tensor, the mask or the weight buffer reaches an address.
// The arithmetic is integer throughout; the blend product is int64 (65536 * 65280 does not fit int32).
#include "../../include/faststyle_io.h"

#include "fs_kernels.h"

namespace fs {
namespace {

struct MixArgs {
    int H, W, Ho, Wo;
    int weight_q8;
    int wide, mask_wide;
};

// the float on the 8.8 scale, as fs_compose.hip's compose_f88: clamped to [0, 255] (NaN: 0), times 256 (exact), truncated
__device__ __forceinline__ int mix_f88(float v) { return (int)(fminf(fmaxf(v, 0.f), 255.f) * 256.0f); }

// Thread i: row y = i / groups, pixels x0 = 4 * (i % groups) ... x0 + 3 (groups = ceil(Wo / 4)).  dst may be a or b, and a may be b: a thread
// reads its pixels before it writes them, and no other thread reads them (hence no __restrict__ on the tensors).
__global__ __launch_bounds__(256) void mix_kernel(const MixArgs A, const float* a, const float* b, const int* __restrict__ weight_dev,
                                                  const unsigned char* __restrict__ mask, float* dst) {
    const int groups = (A.Wo + 3) >> 2;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)groups * A.Ho) return;
    const int y = (int)(i / groups), x0 = (int)(i - (long long)y * groups) * 4;
    const int n = A.Wo - x0 < 4 ? A.Wo - x0 : 4;
    const size_t at = (((size_t)blockIdx.y * A.Ho + y) * A.Wo + x0) * 3;
    int t = A.weight_q8;
    if (weight_dev) {                                      // one weight per image, clamped: whatever the buffer holds, w stays in [0, 65536]
        t = weight_dev[blockIdx.y];
        t = t < 0 ? 0 : (t > 256 ? 256 : t);
    }
    float p[12], q[12];
    int m[4] = {255, 255, 255, 255};
    if (A.wide) {                                          // (Wo a multiple of 4: n is 4)
        const float4* a4 = reinterpret_cast<const float4*>(a + at);
        const float4* b4 = reinterpret_cast<const float4*>(b + at);
        const float4 a0 = a4[0], a1 = a4[1], a2 = a4[2], b0 = b4[0], b1 = b4[1], b2 = b4[2];
        p[0] = a0.x; p[1] = a0.y; p[2] = a0.z; p[3] = a0.w; p[4] = a1.x; p[5] = a1.y; p[6] = a1.z; p[7] = a1.w;
        p[8] = a2.x; p[9] = a2.y; p[10] = a2.z; p[11] = a2.w;
        q[0] = b0.x; q[1] = b0.y; q[2] = b0.z; q[3] = b0.w; q[4] = b1.x; q[5] = b1.y; q[6] = b1.z; q[7] = b1.w;
        q[8] = b2.x; q[9] = b2.y; q[10] = b2.z; q[11] = b2.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int xn = k < n ? k : n - 1;               // (beyond the row's end: the last pixel again, never stored)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                p[3 * k + c] = a[at + 3 * xn + c];
                q[3 * k + c] = b[at + 3 * xn + c];
            }
        }
    }
    if (mask) {
        const unsigned char* mrow = mask + (size_t)(y < A.H ? y : A.H - 1) * A.W;
        if (A.mask_wide) {                                 // (wide, W == Wo and the mask 4-byte aligned: row and x0 are multiples of 4)
            const unsigned v = *reinterpret_cast<const unsigned*>(mrow + x0);
            m[0] = (int)(v & 0xFFu);
            m[1] = (int)((v >> 8) & 0xFFu);
            m[2] = (int)((v >> 16) & 0xFFu);
            m[3] = (int)(v >> 24);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) m[k] = (int)mrow[x0 + k < A.W ? x0 + k : A.W - 1];
        }
    }
    float o[12];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const long long w = (long long)t * (m[k] + (m[k] >> 7));                    // 0 ... 65536
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int P = mix_f88(p[3 * k + c]), Q = mix_f88(q[3 * k + c]);
            // a convex combination of two values in [0, 65280]: the rounding cannot pass either end, no clamp (faststyle_io.h)
            o[3 * k + c] = (float)(P + (int)(((long long)(Q - P) * w + 32768) >> 16)) * 0.00390625f;
        }
    }
    float* op = dst + at;
    if (A.wide) {                                          // 48 bytes at a multiple of 48 of a 16-byte aligned tensor
        float4* o4 = reinterpret_cast<float4*>(op);
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

}  // namespace

// arguments: checked by the caller (fs_api.hip: fs_mix_f32)
int mix_f32(const float* a, const float* b, int H, int W, int Ho, int Wo, int N, int weight_q8, const int* weight_dev, const unsigned char* mask,
            float* dst, hipStream_t s) {
    MixArgs A;
    A.H = H; A.W = W; A.Ho = Ho; A.Wo = Wo;
    A.weight_q8 = weight_q8;
    A.wide = (Wo & 3) == 0 && (((uintptr_t)a | (uintptr_t)b | (uintptr_t)dst) & 15) == 0;
    A.mask_wide = A.wide && W == Wo && mask && ((uintptr_t)mask & 3) == 0;
    const long long threads = ((long long)(Wo + 3) >> 2) * Ho;
    const dim3 grid((unsigned)((threads + 255) / 256), (unsigned)N), block(256);
    hipLaunchKernelGGL(mix_kernel, grid, block, 0, s, A, a, b, weight_dev, mask, dst);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace fs
