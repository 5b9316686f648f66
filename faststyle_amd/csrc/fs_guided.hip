// Guided delivery (include/faststyle_io.h, whose comment is the arithmetic contract): the fast guided filter of He & Sun between the net's
// grid and the delivery grid.  On the net's grid a local linear model output ~ a * luma(source) + b is fitted per channel over a (2r + 1)^2
// window (coef), a and b are box-averaged over the same window (mean), and at the delivery size the four neighbouring (a, b) are interpolated
// bilinearly and applied to the luma of the full-size source (apply).  Three launches, grid.z / grid.y = image.
//   coef   -- one 256-thread workgroup per 32 x 16 tile of the net's grid.  The tile plus an r halo of I and of the three P_c is staged as u16
//             with the clamped coordinates applied; the eight kinds of window sums (S_I, S_c u32; S_II, S_Ic u64: a product of two 8.8 values
//             fits u32, 17 of them do not) are formed separably, rows into LDS, then columns, 2 (2r + 1) taps a pixel instead of (2r + 1)^2.
//             Static LDS at the largest radius: 4 x 32 x 48 u16 + 32 x 32 x (4 x 4 + 4 x 8) = 61440 bytes, two workgroups a CU.  Every array is
//             read and written with consecutive lanes on consecutive elements (u16: two lanes a dword, the same dword broadcasts; u32: the 32
//             lanes of a half on 32 banks; u64: 256 contiguous bytes a half, the 64-bank row of ds_read_b64), so no access conflicts.
//   mean   -- the same scheme on the six int32 planes, 16 x 16 tiles: 6 x 32 x 32 int32 + 32 x 16 x (3 x 4 + 3 x 8) = 43008 bytes (17 values
//             below 2^27 do not fit int32: the partial sums of b are int64, those of a int32).
//   apply  -- the thread layout of fs_compose.hip: four pixels of a delivery row.  The vertical axis triple is the thread's, the horizontal one
//             the pixel's, both int32.  Bilinear weights distribute over integer sums exactly, so the four taps are combined as two vertical
//             blends and one horizontal one.  Where the delivery width is a multiple of 4 and source and destination are 16-byte aligned
//             (`wide`, uniform per launch) the source pixels move as one 16-byte (kind 1), three 4-byte (kind 0) or three 16-byte (kind 2)
//             accesses and the twelve floats of the result as three 16-byte stores; as single bytes and floats otherwise, with the same values.
//             The 24 bytes of a `mean` pixel are 8-byte aligned and move as three 8-byte loads.
// The arithmetic is integer throughout (int64 wherever the contract says so); every coordinate that reaches an address is computed from the
// launch geometry and clamped, no value read from a tensor does.
#include "../../include/faststyle_io.h"

#include "fs_kernels.h"

namespace fs {
namespace {

constexpr int GR_MAX = 8;                                   // the largest radius
constexpr int GC_TW = 32, GC_TH = 16;                       // coef: the tile
constexpr int GC_HW = GC_TW + 2 * GR_MAX, GC_HH = GC_TH + 2 * GR_MAX;
constexpr int GM_TW = 16, GM_TH = 16;                       // mean: the tile
constexpr int GM_HW = GM_TW + 2 * GR_MAX, GM_HH = GM_TH + 2 * GR_MAX;

struct GuidedArgs {
    int H, W, Ho, Wo, Hd, Wd;
    int r;
    int l0, l1, l2;                         // luma weights by 2^16 of lo_src's channels as stored
    int h0, h1, h2;                         // ... of hi_src's
    long long n, eps;                       // (2r + 1)^2; n^2 E^2 65536
    int wide;
};

// compose's to88: clamped to [0, 255] (NaN: 0), times 256 (exact), truncated
__device__ __forceinline__ int guided_f88(float v) { return (int)(fminf(fmaxf(v, 0.f), 255.f) * 256.0f); }

__device__ __forceinline__ int guided_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// grid (ceil(W / 32), ceil(H / 16), N)
__global__ __launch_bounds__(256) void guided_coef_kernel(const GuidedArgs A, const float* __restrict__ lo_src, const float* __restrict__ lo_out,
                                                          int* __restrict__ coef) {
    __shared__ unsigned short sI[GC_HH * GC_HW], sP[3][GC_HH * GC_HW];
    __shared__ unsigned rI[GC_HH * GC_TW], rP[3][GC_HH * GC_TW];
    __shared__ unsigned long long rII[GC_HH * GC_TW], rIP[3][GC_HH * GC_TW];
    const int r = A.r, hw = GC_TW + 2 * r, hh = GC_TH + 2 * r, taps = 2 * r + 1;
    const int tx0 = (int)blockIdx.x * GC_TW, ty0 = (int)blockIdx.y * GC_TH;
    const float* src = lo_src + (size_t)blockIdx.z * A.H * A.W * 3;
    const float* out = lo_out + (size_t)blockIdx.z * A.Ho * A.Wo * 3;
    for (int i = (int)threadIdx.x; i < hh * hw; i += 256) {                       // stage: hw <= 48, hh <= 32
        const int hy = i / hw, hx = i - hy * hw;
        const int y = guided_clamp(ty0 + hy - r, A.H - 1), x = guided_clamp(tx0 + hx - r, A.W - 1);
        const float* sp = src + ((size_t)y * A.W + x) * 3;
        const float* op = out + ((size_t)y * A.Wo + x) * 3;
        const float s0 = sp[0], s1 = sp[1], s2 = sp[2], o0 = op[0], o1 = op[1], o2 = op[2];
        const long long I = ((long long)A.l0 * guided_f88(s0) + (long long)A.l1 * guided_f88(s1) + (long long)A.l2 * guided_f88(s2) + 32768) >> 16;
        sI[i] = (unsigned short)I;
        sP[0][i] = (unsigned short)guided_f88(o0);
        sP[1][i] = (unsigned short)guided_f88(o1);
        sP[2][i] = (unsigned short)guided_f88(o2);
    }
    __syncthreads();
    for (int i = (int)threadIdx.x; i < hh * GC_TW; i += 256) {                    // rows: the sums over hx = x .. x + 2r of halo row hy
        const int hy = i / GC_TW, x = i - hy * GC_TW;
        const int at = hy * hw + x;
        unsigned si = 0, sp0 = 0, sp1 = 0, sp2 = 0;
        unsigned long long sii = 0, sip0 = 0, sip1 = 0, sip2 = 0;
        for (int k = 0; k < taps; ++k) {
            const unsigned I = sI[at + k], p0 = sP[0][at + k], p1 = sP[1][at + k], p2 = sP[2][at + k];
            si += I; sp0 += p0; sp1 += p1; sp2 += p2;
            sii += I * I; sip0 += I * p0; sip1 += I * p1; sip2 += I * p2;        // (65280^2 < 2^32: each product fits u32)
        }
        rI[i] = si; rP[0][i] = sp0; rP[1][i] = sp1; rP[2][i] = sp2;
        rII[i] = sii; rIP[0][i] = sip0; rIP[1][i] = sip1; rIP[2][i] = sip2;
    }
    __syncthreads();
    for (int p = (int)threadIdx.x; p < GC_TW * GC_TH; p += 256) {                 // columns, the two divisions, the store
        const int ty = p / GC_TW, tx = p - ty * GC_TW;
        const int y = ty0 + ty, x = tx0 + tx;
        if (y >= A.H || x >= A.W) continue;
        unsigned si = 0, sp[3] = {0, 0, 0};
        unsigned long long sii = 0, sip[3] = {0, 0, 0};
        for (int j = 0; j < taps; ++j) {
            const int at = (ty + j) * GC_TW + tx;
            si += rI[at]; sp[0] += rP[0][at]; sp[1] += rP[1][at]; sp[2] += rP[2][at];
            sii += rII[at]; sip[0] += rIP[0][at]; sip[1] += rIP[1][at]; sip[2] += rIP[2][at];
        }
        const long long SI = (long long)si, n = A.n;
        const long long D = n * (long long)sii - SI * SI + A.eps;
        int* cp = coef + (((size_t)blockIdx.z * A.H + y) * A.W + x) * 6;
        int av[3], bv[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const long long SP = (long long)sp[c];
            const long long C = n * (long long)sip[c] - SI * SP;
            const long long a = (C * 4096) / D;
            const long long b = (SP * 4096 - a * SI) / (256 * n);
            av[c] = (int)a;
            bv[c] = (int)b;
        }
        cp[0] = av[0]; cp[1] = av[1]; cp[2] = av[2];
        cp[3] = bv[0]; cp[4] = bv[1]; cp[5] = bv[2];
    }
}

// grid (ceil(W / 16), ceil(H / 16), N)
__global__ __launch_bounds__(256) void guided_mean_kernel(const GuidedArgs A, const int* __restrict__ coef, int* __restrict__ mean) {
    __shared__ int sC[6][GM_HH * GM_HW];
    __shared__ int rA[3][GM_HH * GM_TW];
    __shared__ long long rB[3][GM_HH * GM_TW];
    const int r = A.r, hw = GM_TW + 2 * r, hh = GM_TH + 2 * r, taps = 2 * r + 1;
    const int tx0 = (int)blockIdx.x * GM_TW, ty0 = (int)blockIdx.y * GM_TH;
    const int* cimg = coef + (size_t)blockIdx.z * A.H * A.W * 6;
    for (int i = (int)threadIdx.x; i < hh * hw; i += 256) {
        const int hy = i / hw, hx = i - hy * hw;
        const int y = guided_clamp(ty0 + hy - r, A.H - 1), x = guided_clamp(tx0 + hx - r, A.W - 1);
        const int2* cp = reinterpret_cast<const int2*>(cimg + ((size_t)y * A.W + x) * 6);      // 24 bytes at a multiple of 24 of a 16-byte aligned part
        const int2 c0 = cp[0], c1 = cp[1], c2 = cp[2];
        sC[0][i] = c0.x; sC[1][i] = c0.y; sC[2][i] = c1.x;
        sC[3][i] = c1.y; sC[4][i] = c2.x; sC[5][i] = c2.y;
    }
    __syncthreads();
    for (int i = (int)threadIdx.x; i < hh * GM_TW; i += 256) {
        const int hy = i / GM_TW, x = i - hy * GM_TW;
        const int at = hy * hw + x;
        int a0 = 0, a1 = 0, a2 = 0;                                               // (|a| < 2^18: 17 of them fit int32)
        long long b0 = 0, b1 = 0, b2 = 0;
        for (int k = 0; k < taps; ++k) {
            a0 += sC[0][at + k]; a1 += sC[1][at + k]; a2 += sC[2][at + k];
            b0 += sC[3][at + k]; b1 += sC[4][at + k]; b2 += sC[5][at + k];
        }
        rA[0][i] = a0; rA[1][i] = a1; rA[2][i] = a2;
        rB[0][i] = b0; rB[1][i] = b1; rB[2][i] = b2;
    }
    __syncthreads();
    const int ty = (int)threadIdx.x / GM_TW, tx = (int)threadIdx.x - ty * GM_TW;
    const int y = ty0 + ty, x = tx0 + tx;
    if (y >= A.H || x >= A.W) return;
    long long a0 = 0, a1 = 0, a2 = 0, b0 = 0, b1 = 0, b2 = 0;
    for (int j = 0; j < taps; ++j) {
        const int at = (ty + j) * GM_TW + tx;
        a0 += rA[0][at]; a1 += rA[1][at]; a2 += rA[2][at];
        b0 += rB[0][at]; b1 += rB[1][at]; b2 += rB[2][at];
    }
    const long long n = A.n;
    int* mp = mean + (((size_t)blockIdx.z * A.H + y) * A.W + x) * 6;
    mp[0] = (int)(a0 / n); mp[1] = (int)(a1 / n); mp[2] = (int)(a2 / n);
    mp[3] = (int)(b0 / n); mp[4] = (int)(b1 / n); mp[5] = (int)(b2 / n);
}

// One axis of the contract: for the delivery index d of nd, over a source axis of ns: the two clamped taps and the fraction in [0, 255].  All
// int32 for sides up to 32767; nd >= ns, so num > -2 nd and the floor is -1 for every negative num.
__device__ __forceinline__ void guided_axis(int d, int ns, int nd, int& t0, int& t1, int& f) {
    const int num = (2 * d + 1) * ns - nd, den = 2 * nd;
    const int q = num < 0 ? -1 : num / den;
    f = ((num - q * den) * 256) / den;
    t0 = guided_clamp(q, ns - 1);
    t1 = guided_clamp(q + 1, ns - 1);
}

// Thread i: row Y = i / groups, pixels X0 = 4 * (i % groups) ... X0 + 3 (groups = ceil(Wd / 4)); grid.y = image
template <int KIND>
__global__ __launch_bounds__(256) void guided_apply_kernel(const GuidedArgs A, const int* __restrict__ mean, const void* __restrict__ hi_src,
                                                           float* __restrict__ dst) {
    const int groups = (A.Wd + 3) >> 2;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)groups * A.Hd) return;
    const int Y = (int)(i / groups), X0 = (int)(i - (long long)Y * groups) * 4;
    const int nv = A.Wd - X0 < 4 ? A.Wd - X0 : 4;
    int ya, yb, fy;
    guided_axis(Y, A.H, A.Hd, ya, yb, fy);
    const int* ma = mean + ((size_t)blockIdx.y * A.H + ya) * A.W * 6;
    const int* mb = mean + ((size_t)blockIdx.y * A.H + yb) * A.W * 6;
    const size_t at = ((size_t)blockIdx.y * A.Hd + Y) * A.Wd + X0;                // the first pixel, in pixels
    int h[12];                                                                    // the source on the 8.8 scale
    if (KIND == 2) {
        const float* sp = static_cast<const float*>(hi_src) + at * 3;
        float v[12];
        if (A.wide) {
            const float4* s4 = reinterpret_cast<const float4*>(sp);
            const float4 s0 = s4[0], s1 = s4[1], s2 = s4[2];
            v[0] = s0.x; v[1] = s0.y; v[2] = s0.z; v[3] = s0.w; v[4] = s1.x; v[5] = s1.y; v[6] = s1.z; v[7] = s1.w;
            v[8] = s2.x; v[9] = s2.y; v[10] = s2.z; v[11] = s2.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int xk = k < nv ? k : nv - 1;                               // (beyond the row's end: the last pixel again, never stored)
                v[3 * k] = sp[3 * xk]; v[3 * k + 1] = sp[3 * xk + 1]; v[3 * k + 2] = sp[3 * xk + 2];
            }
        }
#pragma unroll
        for (int e = 0; e < 12; ++e) h[e] = guided_f88(v[e]);
    } else if (KIND == 1) {
        const unsigned char* sp = static_cast<const unsigned char*>(hi_src) + at * 4;
        unsigned w[4];
        if (A.wide) {
            const uint4 q = *reinterpret_cast<const uint4*>(sp);
            w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int xk = k < nv ? k : nv - 1;
                w[k] = (unsigned)sp[4 * xk] | ((unsigned)sp[4 * xk + 1] << 8) | ((unsigned)sp[4 * xk + 2] << 16);
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            h[3 * k] = (int)(w[k] & 0xFFu) << 8;
            h[3 * k + 1] = (int)((w[k] >> 8) & 0xFFu) << 8;
            h[3 * k + 2] = (int)((w[k] >> 16) & 0xFFu) << 8;
        }
    } else {
        const unsigned char* sp = static_cast<const unsigned char*>(hi_src) + at * 3;
        if (A.wide) {                                                             // 12 bytes at a multiple of 12 of a 16-byte aligned tensor
            const unsigned* s1 = reinterpret_cast<const unsigned*>(sp);
            const unsigned w0 = s1[0], w1 = s1[1], w2 = s1[2];
            h[0] = (int)(w0 & 0xFFu) << 8; h[1] = (int)((w0 >> 8) & 0xFFu) << 8; h[2] = (int)((w0 >> 16) & 0xFFu) << 8;
            h[3] = (int)(w0 >> 24) << 8; h[4] = (int)(w1 & 0xFFu) << 8; h[5] = (int)((w1 >> 8) & 0xFFu) << 8;
            h[6] = (int)((w1 >> 16) & 0xFFu) << 8; h[7] = (int)(w1 >> 24) << 8; h[8] = (int)(w2 & 0xFFu) << 8;
            h[9] = (int)((w2 >> 8) & 0xFFu) << 8; h[10] = (int)((w2 >> 16) & 0xFFu) << 8; h[11] = (int)(w2 >> 24) << 8;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int xk = k < nv ? k : nv - 1;
                h[3 * k] = (int)sp[3 * xk] << 8; h[3 * k + 1] = (int)sp[3 * xk + 1] << 8; h[3 * k + 2] = (int)sp[3 * xk + 2] << 8;
            }
        }
    }
    float o[12];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        int xa, xb, fx;
        guided_axis(X0 + k < A.Wd ? X0 + k : A.Wd - 1, A.W, A.Wd, xa, xb, fx);
        const int2* paa = reinterpret_cast<const int2*>(ma + (size_t)xa * 6);     // 24 bytes at a multiple of 24 of a 16-byte aligned part
        const int2* pab = reinterpret_cast<const int2*>(ma + (size_t)xb * 6);
        const int2* pba = reinterpret_cast<const int2*>(mb + (size_t)xa * 6);
        const int2* pbb = reinterpret_cast<const int2*>(mb + (size_t)xb * 6);
        const int2 aa0 = paa[0], aa1 = paa[1], aa2 = paa[2], ab0 = pab[0], ab1 = pab[1], ab2 = pab[2];
        const int2 ba0 = pba[0], ba1 = pba[1], ba2 = pba[2], bb0 = pbb[0], bb1 = pbb[1], bb2 = pbb[2];
        const int maa[6] = {aa0.x, aa0.y, aa1.x, aa1.y, aa2.x, aa2.y}, mab[6] = {ab0.x, ab0.y, ab1.x, ab1.y, ab2.x, ab2.y};
        const int mba[6] = {ba0.x, ba0.y, ba1.x, ba1.y, ba2.x, ba2.y}, mbb[6] = {bb0.x, bb0.y, bb1.x, bb1.y, bb2.x, bb2.y};
        const long long G = ((long long)A.h0 * h[3 * k] + (long long)A.h1 * h[3 * k + 1] + (long long)A.h2 * h[3 * k + 2] + 32768) >> 16;
        const long long wy0 = 256 - fy, wy1 = fy, wx0 = 256 - fx, wx1 = fx;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const long long Ah = wx0 * (wy0 * maa[c] + wy1 * mba[c]) + wx1 * (wy0 * mab[c] + wy1 * mbb[c]);
            const long long Bh = wx0 * (wy0 * maa[3 + c] + wy1 * mba[3 + c]) + wx1 * (wy0 * mab[3 + c] + wy1 * mbb[3 + c]);
            const long long F = (Ah * G + Bh * 256 + (1ll << 27)) >> 28;
            o[3 * k + c] = (float)(int)(F < 0 ? 0 : (F > 65280 ? 65280 : F)) * 0.00390625f;
        }
    }
    float* op = dst + at * 3;
    if (A.wide) {                                                                 // 48 bytes at a multiple of 48 of a 16-byte aligned tensor
        float4* o4 = reinterpret_cast<float4*>(op);
        o4[0] = make_float4(o[0], o[1], o[2], o[3]);
        o4[1] = make_float4(o[4], o[5], o[6], o[7]);
        o4[2] = make_float4(o[8], o[9], o[10], o[11]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < nv) {
                op[3 * k] = o[3 * k];
                op[3 * k + 1] = o[3 * k + 1];
                op[3 * k + 2] = o[3 * k + 2];
            }
    }
}

}  // namespace

// the bytes of one part (coef or mean) of the workspace, a multiple of 16
size_t guided_part_bytes(int H, int W, int N) { return ((size_t)N * H * W * 6 * sizeof(int) + 15) & ~(size_t)15; }

// arguments: checked by the caller (fs_api.hip: fs_guided_f32)
int guided_f32(const float* lo_src, int H, int W, const float* lo_out, int Ho, int Wo, const void* hi_src, int hi_kind, int Hd, int Wd, int N, int radius,
               int smoothness, int matrix, int lo_bgr, int hi_bgr, void* work, float* dst, hipStream_t s) {
    const int kr = matrix ? 13933 : 19595, kg = matrix ? 46871 : 38470, kb = matrix ? 4732 : 7471;      // compose's triples
    GuidedArgs A;
    A.H = H; A.W = W; A.Ho = Ho; A.Wo = Wo; A.Hd = Hd; A.Wd = Wd;
    A.r = radius;
    A.l0 = lo_bgr ? kb : kr; A.l1 = kg; A.l2 = lo_bgr ? kr : kb;
    A.h0 = hi_bgr ? kb : kr; A.h1 = kg; A.h2 = hi_bgr ? kr : kb;
    A.n = (long long)(2 * radius + 1) * (2 * radius + 1);
    A.eps = A.n * A.n * smoothness * smoothness * 65536;
    A.wide = (Wd & 3) == 0 && (((uintptr_t)hi_src | (uintptr_t)dst) & 15) == 0;
    int* coef = static_cast<int*>(work);
    int* mean = reinterpret_cast<int*>(static_cast<unsigned char*>(work) + guided_part_bytes(H, W, N));
    const dim3 block(256);
    hipLaunchKernelGGL(guided_coef_kernel, dim3((unsigned)((W + GC_TW - 1) / GC_TW), (unsigned)((H + GC_TH - 1) / GC_TH), (unsigned)N), block, 0, s, A,
                       lo_src, lo_out, coef);
    hipLaunchKernelGGL(guided_mean_kernel, dim3((unsigned)((W + GM_TW - 1) / GM_TW), (unsigned)((H + GM_TH - 1) / GM_TH), (unsigned)N), block, 0, s, A,
                       (const int*)coef, mean);
    const long long threads = ((long long)(Wd + 3) >> 2) * Hd;
    const dim3 grid((unsigned)((threads + 255) / 256), (unsigned)N);
    if (hi_kind == 0) hipLaunchKernelGGL(guided_apply_kernel<0>, grid, block, 0, s, A, (const int*)mean, hi_src, dst);
    else if (hi_kind == 1) hipLaunchKernelGGL(guided_apply_kernel<1>, grid, block, 0, s, A, (const int*)mean, hi_src, dst);
    else hipLaunchKernelGGL(guided_apply_kernel<2>, grid, block, 0, s, A, (const int*)mean, hi_src, dst);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace fs
