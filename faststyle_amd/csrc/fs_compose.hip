// Style strength, colour preservation and a region mask between the net's forward pass and the output conversions (include/faststyle_io.h,
// whose comment is the arithmetic contract): the net's fp32 output is blended back towards the net's fp32 input on the unsigned 8.8 scale of
// the deep video path, and every output conversion of faststyle_amd/stream.py (compose=) reads the composed tensor instead of the net's.
//   device -- one kernel, grid.y = image, the thread layout of fs_yuv16.hip: four pixels of an output row.  No LDS, no tables: the luma
//             weights travel in the kernel arguments.  The output is up to 3 rows and columns larger than the input (fs_tnet_out_shape) and
//             aligned top-left: source and mask are read at (min(y, H - 1), min(x, W - 1)).  Where the two sizes have one width, that width is a
//             multiple of 4 and the three tensors are 16-byte aligned (`wide`, uniform per launch) the twelve floats of a thread move as three
//             16-byte accesses per tensor, and the four mask bytes as one dword where the mask is 4-byte aligned; as single floats and bytes
//             otherwise, with the same values.  No value read from a tensor or the mask reaches an address.
// The arithmetic is integer throughout; the luma sums and the blend product are int64 (65536 * 65280 does not fit int32).
#include "../../include/faststyle_io.h"

#include "fs_kernels.h"

namespace fs {
namespace {

struct ComposeArgs {
    int H, W, Ho, Wo;
    int k0, k1, k2;                         // luma weights by 2^16 of the channels as stored (k0 is kb when channel 0 is blue)
    int strength_q8, keep_color;
    int src_swap;                           // the source holds R and B the other way round than the net's output: read exchanged
    int wide, mask_wide;
};

// the float on the 8.8 scale, as fs_yuv16.hip's deep_f88: clamped to [0, 255] (NaN: 0), times 256 (exact), truncated
__device__ __forceinline__ int compose_f88(float v) { return (int)(fminf(fmaxf(v, 0.f), 255.f) * 256.0f); }

// Thread i: row y = i / groups, pixels x0 = 4 * (i % groups) ... x0 + 3 (groups = ceil(Wo / 4)).  dst may be net: a thread reads its pixels
// before it writes them, and no other thread reads them (hence no __restrict__ on the tensors).
__global__ __launch_bounds__(256) void compose_kernel(const ComposeArgs A, const float* src, const float* net, const unsigned char* __restrict__ mask,
                                                      float* dst) {
    const int groups = (A.Wo + 3) >> 2;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)groups * A.Ho) return;
    const int y = (int)(i / groups), x0 = (int)(i - (long long)y * groups) * 4;
    const int n = A.Wo - x0 < 4 ? A.Wo - x0 : 4;
    const int ys = y < A.H ? y : A.H - 1;
    const float* srow = src + ((size_t)blockIdx.y * A.H + ys) * A.W * 3;
    const size_t at = (((size_t)blockIdx.y * A.Ho + y) * A.Wo + x0) * 3;
    float a[12], b[12];
    int m[4] = {255, 255, 255, 255};
    if (A.wide) {                                          // (W == Wo, a multiple of 4: n is 4 and x0 + 3 < W)
        const float4* s4 = reinterpret_cast<const float4*>(srow + (size_t)x0 * 3);
        const float4* n4 = reinterpret_cast<const float4*>(net + at);
        const float4 s0 = s4[0], s1 = s4[1], s2 = s4[2], n0 = n4[0], n1 = n4[1], n2 = n4[2];
        a[0] = s0.x; a[1] = s0.y; a[2] = s0.z; a[3] = s0.w; a[4] = s1.x; a[5] = s1.y; a[6] = s1.z; a[7] = s1.w;
        a[8] = s2.x; a[9] = s2.y; a[10] = s2.z; a[11] = s2.w;
        b[0] = n0.x; b[1] = n0.y; b[2] = n0.z; b[3] = n0.w; b[4] = n1.x; b[5] = n1.y; b[6] = n1.z; b[7] = n1.w;
        b[8] = n2.x; b[9] = n2.y; b[10] = n2.z; b[11] = n2.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int xs = x0 + k < A.W ? x0 + k : A.W - 1;
            const int xn = k < n ? k : n - 1;               // (beyond the row's end: the last pixel again, never stored)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                a[3 * k + c] = srow[(size_t)xs * 3 + c];
                b[3 * k + c] = net[at + 3 * xn + c];
            }
        }
    }
    if (A.src_swap) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float t = a[3 * k];
            a[3 * k] = a[3 * k + 2];
            a[3 * k + 2] = t;
        }
    }
    if (mask) {
        const unsigned char* mrow = mask + (size_t)ys * A.W;
        if (A.mask_wide) {                                 // (wide, and the mask 4-byte aligned: row and x0 are multiples of 4)
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
        const int A0 = compose_f88(a[3 * k]), A1 = compose_f88(a[3 * k + 1]), A2 = compose_f88(a[3 * k + 2]);
        const int B0 = compose_f88(b[3 * k]), B1 = compose_f88(b[3 * k + 1]), B2 = compose_f88(b[3 * k + 2]);
        int D0 = B0 - A0, D1 = B1 - A1, D2 = B2 - A2;
        if (A.keep_color) {                                // one delta for the three channels: luma moves, the colour differences stay
            const long long la = ((long long)A.k0 * A0 + (long long)A.k1 * A1 + (long long)A.k2 * A2 + 32768) >> 16;
            const long long lb = ((long long)A.k0 * B0 + (long long)A.k1 * B1 + (long long)A.k2 * B2 + 32768) >> 16;
            D0 = D1 = D2 = (int)(lb - la);
        }
        const long long w = (long long)A.strength_q8 * (m[k] + (m[k] >> 7));        // 0 ... 65536
        const long long f0 = A0 + (((long long)D0 * w + 32768) >> 16);
        const long long f1 = A1 + (((long long)D1 * w + 32768) >> 16);
        const long long f2 = A2 + (((long long)D2 * w + 32768) >> 16);
        o[3 * k] = (float)(int)(f0 < 0 ? 0 : (f0 > 65280 ? 65280 : f0)) * 0.00390625f;
        o[3 * k + 1] = (float)(int)(f1 < 0 ? 0 : (f1 > 65280 ? 65280 : f1)) * 0.00390625f;
        o[3 * k + 2] = (float)(int)(f2 < 0 ? 0 : (f2 > 65280 ? 65280 : f2)) * 0.00390625f;
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

// arguments: checked by the caller (fs_api.hip: fs_compose_f32)
int compose_f32(const float* src, int H, int W, const float* net, int Ho, int Wo, int N, int strength_q8, int keep_color, int matrix, int bgr,
                int src_swap, const unsigned char* mask, float* dst, hipStream_t s) {
    const int kr = matrix ? 13933 : 19595, kg = matrix ? 46871 : 38470, kb = matrix ? 4732 : 7471;      // each triple sums to 65536
    ComposeArgs A;
    A.H = H; A.W = W; A.Ho = Ho; A.Wo = Wo;
    A.k0 = bgr ? kb : kr; A.k1 = kg; A.k2 = bgr ? kr : kb;
    A.strength_q8 = strength_q8;
    A.keep_color = keep_color;
    A.src_swap = src_swap;
    A.wide = W == Wo && (W & 3) == 0 && (((uintptr_t)src | (uintptr_t)net | (uintptr_t)dst) & 15) == 0;
    A.mask_wide = A.wide && mask && ((uintptr_t)mask & 3) == 0;
    const long long threads = ((long long)(Wo + 3) >> 2) * Ho;
    const dim3 grid((unsigned)((threads + 255) / 256), (unsigned)N), block(256);
    hipLaunchKernelGGL(compose_kernel, grid, block, 0, s, A, src, net, mask, dst);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace fs
