// cv2.resize of OpenCV 3.1.0 on u8 images (include/faststyle_io.h), the resampling of the reference's utils.imresize (utils.py:25-40) and of the
// frame loop's --frame_size: INTER_CUBIC and INTER_AREA, bit-identical to the host restatement faststyle_amd/cvresize.py, whose docstring is the
// arithmetic contract (restated from the published algorithm of imgproc/src/imgwarp.cpp: resizeGeneric_ with the 8-bit fixed-point cubic path,
// resizeAreaFast_, resizeArea_ with computeResizeAreaTab).
//   host   -- fs_cvresize_plan / fs_cvresize_tables: the destination size, the path, and the per-axis tables in the double -> float32 arithmetic
//             of cvresize._cubic_axis / _area_tab; plain C++ with no global state and no allocation;
//   device -- one thread per output pixel (3 channels), one kernel per path, grid.y = image.  Bandwidth-trivial: the taps of neighbouring
//             lanes share cache lines, the tables are a few KB read through the cache.  No value read from an image or a table reaches an
//             address unclamped.
// Every float32 product and sum is rounded separately (`#pragma clang fp contract(off)`, as in fs_resize.h): a fused multiply-add would change bits.
#include "../../include/faststyle_io.h"

#include <cmath>
#include <cstring>

#include "fs_kernels.h"

namespace fs {
namespace {

constexpr int kCvMaxSide = 32767;
constexpr int kCoefBits = 11;

inline size_t align_up(size_t n, size_t a) { return (n + a - 1) / a * a; }

// ---------------------------------------------------------------- host: tables
// interpolateCubic in float32, A = -0.75, the four weights rounded to 11-bit fixed point (cvRound: ties to even); per output index the four
// source indices clamped to the edge pixel, then the four weights
void cubic_axis(int n_src, int n_dst, double scale, int32_t* tab) {
#pragma clang fp contract(off)
    for (int d = 0; d < n_dst; ++d) {
        const double fd = ((double)d + 0.5) * scale;
        const float f = (float)(fd - 0.5);
        const float fl = floorf(f);
        const int s = (int)fl;
        const float x = f - fl;
        const float x1 = x + 1.0f;
        float c0 = -0.75f * x1;
        c0 = c0 - (-3.75f);
        c0 = c0 * x1;
        c0 = c0 + (-6.0f);
        c0 = c0 * x1;
        c0 = c0 - (-3.0f);
        float c1 = 1.25f * x;
        c1 = c1 - 2.25f;
        c1 = c1 * x;
        c1 = c1 * x;
        c1 = c1 + 1.0f;
        const float xm = 1.0f - x;
        float c2 = 1.25f * xm;
        c2 = c2 - 2.25f;
        c2 = c2 * xm;
        c2 = c2 * xm;
        c2 = c2 + 1.0f;
        float c3 = 1.0f - c0;
        c3 = c3 - c1;
        c3 = c3 - c2;
        const float c[4] = {c0, c1, c2, c3};
        for (int k = 0; k < 4; ++k) {
            const int i = s - 1 + k;
            tab[d * 8 + k] = i < 0 ? 0 : (i > n_src - 1 ? n_src - 1 : i);
            tab[d * 8 + 4 + k] = (int32_t)lrintf(c[k] * (float)(1 << kCoefBits));
        }
    }
}

struct AreaTap {
    int32_t si;
    float alpha;
};

// computeResizeAreaTab: the leading partial pixel, the whole pixels at 1 / cellWidth, the trailing partial pixel of every output index.
// Returns the number of entries; ofs (n_dst + 1 entries) and taps are written where given.
int area_tab(int n_src, int n_dst, double scale, int32_t* ofs, AreaTap* taps) {
#pragma clang fp contract(off)
    int k = 0;
    for (int d = 0; d < n_dst; ++d) {
        if (ofs) ofs[d] = k;
        const double fs1 = (double)d * scale;
        const double fs2 = fs1 + scale;
        const double rest = (double)n_src - fs1;
        const double cell = scale < rest ? scale : rest;
        int s1 = (int)ceil(fs1), s2 = (int)floor(fs2);
        s2 = s2 < n_src - 1 ? s2 : n_src - 1;
        s1 = s1 < s2 ? s1 : s2;
        if ((double)s1 - fs1 > 1e-3) {
            if (taps) taps[k] = AreaTap{s1 - 1, (float)(((double)s1 - fs1) / cell)};
            ++k;
        }
        for (int s = s1; s < s2; ++s) {
            if (taps) taps[k] = AreaTap{s, (float)(1.0 / cell)};
            ++k;
        }
        if (fs2 - (double)s2 > 1e-3) {
            double a = fs2 - (double)s2;
            a = a < 1.0 ? a : 1.0;
            a = a < cell ? a : cell;
            if (taps) taps[k] = AreaTap{s2, (float)(a / cell)};
            ++k;
        }
    }
    if (ofs) ofs[n_dst] = k;
    return k;
}

inline size_t area_axis_bytes(int n_dst, int taps) { return align_up(((size_t)n_dst + 1) * 4, 8) + (size_t)taps * sizeof(AreaTap); }

// whether p is what fs_cvresize_plan fills
bool plan_matches(const fs_cvresize_info& p) {
    fs_cvresize_info want;
    if (fs_cvresize_plan(p.src_h, p.src_w, p.fx, p.fy, p.interpolation, &want)) return false;
    return !memcmp(&want, &p, sizeof(want));
}

// ---------------------------------------------------------------- device
template <int PB>
__device__ __forceinline__ void load_rgb(const unsigned char* __restrict__ p, int& r, int& g, int& b) {
    if (PB == 4) {
        const unsigned w = *reinterpret_cast<const unsigned*>(p);
        r = (int)(w & 255);
        g = (int)((w >> 8) & 255);
        b = (int)((w >> 16) & 255);
    } else {
        r = p[0];
        g = p[1];
        b = p[2];
    }
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ void store_rgb(unsigned char* __restrict__ dst, size_t pixel, int swap_rb, int r, int g, int b) {
    unsigned char* o = dst + pixel * 3;
    o[0] = (unsigned char)(swap_rb ? b : r);
    o[1] = (unsigned char)g;
    o[2] = (unsigned char)(swap_rb ? r : b);
}

// cvRound of a float32, saturated to a u8 (saturate_cast<uchar>)
__device__ __forceinline__ int round_u8(float v) {
    const float r = rintf(v);              // ties to even
    return r < 0.f ? 0 : (r > 255.f ? 255 : (int)r);
}

// INTER_CUBIC, uchar: horizontal pass and vertical pass in int32 with the 11-bit weights of the tables, (v + 2^21) >> 22 saturated.
template <int PB>
__global__ __launch_bounds__(256) void cvresize_cubic_kernel(const fs_cvresize_info P, const unsigned char* __restrict__ tables,
                                                             const unsigned char* __restrict__ src, int swap_rb, unsigned char* __restrict__ dst) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P.dst_h * P.dst_w) return;
    const int oy = i / P.dst_w, ox = i - oy * P.dst_w;
    const int* __restrict__ xt = reinterpret_cast<const int*>(tables + P.x_offset) + (size_t)ox * 8;
    const int* __restrict__ yt = reinterpret_cast<const int*>(tables + P.y_offset) + (size_t)oy * 8;
    int xi[4], xw[4], yi[4], yw[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        xi[k] = clampi(xt[k], 0, P.src_w - 1);
        xw[k] = xt[4 + k];
        yi[k] = clampi(yt[k], 0, P.src_h - 1);
        yw[k] = yt[4 + k];
    }
    const unsigned char* __restrict__ img = src + (size_t)blockIdx.y * P.src_h * P.src_w * PB;
    int acc[3] = {0, 0, 0};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const unsigned char* __restrict__ row = img + (size_t)yi[r] * P.src_w * PB;
        int h[3] = {0, 0, 0};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            int pr, pg, pb;
            load_rgb<PB>(row + (size_t)xi[k] * PB, pr, pg, pb);
            h[0] += pr * xw[k];
            h[1] += pg * xw[k];
            h[2] += pb * xw[k];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] += h[c] * yw[r];
    }
    int o[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = clampi((acc[c] + (1 << (2 * kCoefBits - 1))) >> (2 * kCoefBits), 0, 255);
    store_rgb(dst, (size_t)blockIdx.y * P.dst_h * P.dst_w + i, swap_rb, o[0], o[1], o[2]);
}

// INTER_AREA with integer factors: the box mean.  A whole 2x2 cell is (a + b + c + d + 2) >> 2, another whole cell cvRound(float32(sum) *
// float32(1 / area)); a cell the image cuts takes the mean of the pixels that exist, cvRound(float32(sum) / float32(n)); 0 where none exists.
template <int PB>
__global__ __launch_bounds__(256) void cvresize_area_fast_kernel(const fs_cvresize_info P, float inv_area, const unsigned char* __restrict__ src,
                                                                 int swap_rb, unsigned char* __restrict__ dst) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P.dst_h * P.dst_w) return;
    const int oy = i / P.dst_w, ox = i - oy * P.dst_w;
    const int isx = P.factor_x, isy = P.factor_y;
    const int wfast = P.src_w / isx < P.dst_w ? P.src_w / isx : P.dst_w, hfast = P.src_h / isy < P.dst_h ? P.src_h / isy : P.dst_h;
    const long long y0 = (long long)oy * isy, x0 = (long long)ox * isx;
    const int y1 = y0 + isy < P.src_h ? (int)(y0 + isy) : P.src_h, x1 = x0 + isx < P.src_w ? (int)(x0 + isx) : P.src_w;
    int o[3] = {0, 0, 0};
    if (y0 < P.src_h && x0 < P.src_w) {
        const unsigned char* __restrict__ img = src + (size_t)blockIdx.y * P.src_h * P.src_w * PB;
        unsigned long long sum[3] = {0, 0, 0};
        for (int y = (int)y0; y < y1; ++y) {
            const unsigned char* __restrict__ row = img + (size_t)y * P.src_w * PB;
            unsigned rs[3] = {0, 0, 0};
            for (int x = (int)x0; x < x1; ++x) {
                int pr, pg, pb;
                load_rgb<PB>(row + (size_t)x * PB, pr, pg, pb);
                rs[0] += (unsigned)pr;
                rs[1] += (unsigned)pg;
                rs[2] += (unsigned)pb;
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) sum[c] += rs[c];
        }
        const bool whole = oy < hfast && ox < wfast;
        const float n = (float)((y1 - (int)y0) * (x1 - (int)x0));
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (whole && isx == 2 && isy == 2)
                o[c] = (int)((sum[c] + 2) >> 2);
            else if (whole)
                o[c] = round_u8((float)sum[c] * inv_area);
            else
                o[c] = round_u8((float)sum[c] / n);
        }
    }
    store_rgb(dst, (size_t)blockIdx.y * P.dst_h * P.dst_w + i, swap_rb, o[0], o[1], o[2]);
}

// INTER_AREA with fractional factors: per source row of the cell the horizontal weighted sum in float32, in the tap order of the x table; the
// rows combined in the order of the y table (the first tap assigns, the others add); cvRound, saturated.  An output index without taps is 0.
template <int PB>
__global__ __launch_bounds__(256) void cvresize_area_kernel(const fs_cvresize_info P, const unsigned char* __restrict__ tables,
                                                            const unsigned char* __restrict__ src, int swap_rb, unsigned char* __restrict__ dst) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P.dst_h * P.dst_w) return;
    const int oy = i / P.dst_w, ox = i - oy * P.dst_w;
    const int* __restrict__ xo = reinterpret_cast<const int*>(tables + P.x_offset);
    const int* __restrict__ yo = reinterpret_cast<const int*>(tables + P.y_offset);
    const AreaTap* __restrict__ xt = reinterpret_cast<const AreaTap*>(tables + P.x_offset + (((size_t)P.dst_w + 1) * 4 + 7) / 8 * 8);
    const AreaTap* __restrict__ yt = reinterpret_cast<const AreaTap*>(tables + P.y_offset + (((size_t)P.dst_h + 1) * 4 + 7) / 8 * 8);
    const int xb = clampi(xo[ox], 0, P.x_taps), xe = clampi(xo[ox + 1], xb, P.x_taps);
    const int yb = clampi(yo[oy], 0, P.y_taps), ye = clampi(yo[oy + 1], yb, P.y_taps);
    const unsigned char* __restrict__ img = src + (size_t)blockIdx.y * P.src_h * P.src_w * PB;
    float acc[3] = {0.f, 0.f, 0.f};
    for (int ky = yb; ky < ye; ++ky) {
        const AreaTap ty = yt[ky];
        const unsigned char* __restrict__ row = img + (size_t)clampi(ty.si, 0, P.src_h - 1) * P.src_w * PB;
        float h[3] = {0.f, 0.f, 0.f};
        for (int kx = xb; kx < xe; ++kx) {
            const AreaTap tx = xt[kx];
            int pr, pg, pb;
            load_rgb<PB>(row + (size_t)clampi(tx.si, 0, P.src_w - 1) * PB, pr, pg, pb);
            const float tr = (float)pr * tx.alpha, tg = (float)pg * tx.alpha, tb = (float)pb * tx.alpha;
            h[0] = h[0] + tr;
            h[1] = h[1] + tg;
            h[2] = h[2] + tb;
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float term = h[c] * ty.alpha;
            acc[c] = ky == yb ? term : acc[c] + term;
        }
    }
    store_rgb(dst, (size_t)blockIdx.y * P.dst_h * P.dst_w + i, swap_rb, round_u8(acc[0]), round_u8(acc[1]), round_u8(acc[2]));
}

}  // namespace

// plan: checked by the caller (fs_api.hip: cvresize_plan_ok); pixel_bytes 3 or 4
int cvresize_u8(const fs_cvresize_info& P, const unsigned char* tables, const unsigned char* src, int pixel_bytes, int N, int swap_rb,
                unsigned char* dst, hipStream_t s) {
    const dim3 grid((unsigned)(((long long)P.dst_h * P.dst_w + 255) / 256), (unsigned)N), block(256);
    if (P.path == FS_CVRESIZE_PATH_CUBIC) {
        if (pixel_bytes == 4) hipLaunchKernelGGL(cvresize_cubic_kernel<4>, grid, block, 0, s, P, tables, src, swap_rb, dst);
        else hipLaunchKernelGGL(cvresize_cubic_kernel<3>, grid, block, 0, s, P, tables, src, swap_rb, dst);
    } else if (P.path == FS_CVRESIZE_PATH_AREA_FAST) {
        const float inv_area = (float)(1.0 / (double)((long long)P.factor_x * P.factor_y));
        if (pixel_bytes == 4) hipLaunchKernelGGL(cvresize_area_fast_kernel<4>, grid, block, 0, s, P, inv_area, src, swap_rb, dst);
        else hipLaunchKernelGGL(cvresize_area_fast_kernel<3>, grid, block, 0, s, P, inv_area, src, swap_rb, dst);
    } else {
        if (pixel_bytes == 4) hipLaunchKernelGGL(cvresize_area_kernel<4>, grid, block, 0, s, P, tables, src, swap_rb, dst);
        else hipLaunchKernelGGL(cvresize_area_kernel<3>, grid, block, 0, s, P, tables, src, swap_rb, dst);
    }
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

bool cvresize_plan_ok(const fs_cvresize_info& p) { return plan_matches(p); }

}  // namespace fs

extern "C" {

int fs_cvresize_plan(int H, int W, double fx, double fy, int interpolation, fs_cvresize_info* plan) {
    using namespace fs;
    if (!plan) return set_error(-1, "fs_cvresize_plan: null argument");
    if (H < 1 || W < 1 || H > kCvMaxSide || W > kCvMaxSide) return set_error(-1, "fs_cvresize_plan: source %dx%d outside [1, %d]", H, W, kCvMaxSide);
    if (!(fx > 0.0) || !(fy > 0.0) || !std::isfinite(fx) || !std::isfinite(fy))
        return set_error(-1, "fs_cvresize_plan: fx %g, fy %g must be finite and positive", fx, fy);
    if (interpolation != FS_CV_INTER_CUBIC && interpolation != FS_CV_INTER_AREA)
        return set_error(-2, "fs_cvresize_plan: interpolation %d is neither INTER_CUBIC (%d) nor INTER_AREA (%d)", interpolation, FS_CV_INTER_CUBIC,
                         FS_CV_INTER_AREA);
    if (interpolation == FS_CV_INTER_AREA && (fx > 1.0 || fy > 1.0))
        return set_error(-2, "fs_cvresize_plan: INTER_AREA with fx %g, fy %g would enlarge: only shrinking is defined", fx, fy);
    const double dw = nearbyint((double)W * fx), dh = nearbyint((double)H * fy);          // cvRound: ties to even
    if (!(dw >= 1.0) || !(dh >= 1.0) || dw > (double)kCvMaxSide || dh > (double)kCvMaxSide)
        return set_error(-1, "fs_cvresize_plan: destination %gx%g outside [1, %d]", dh, dw, kCvMaxSide);
    memset(plan, 0, sizeof(*plan));
    plan->src_h = H;
    plan->src_w = W;
    plan->dst_h = (int)dh;
    plan->dst_w = (int)dw;
    plan->interpolation = interpolation;
    plan->fx = fx;
    plan->fy = fy;
    const double sx = 1.0 / fx, sy = 1.0 / fy;
    if (interpolation == FS_CV_INTER_CUBIC) {
        plan->path = FS_CVRESIZE_PATH_CUBIC;
        plan->x_offset = 0;
        plan->y_offset = (uint64_t)plan->dst_w * 32;
        plan->table_bytes = plan->y_offset + (uint64_t)plan->dst_h * 32;
        return 0;
    }
    const double isx = nearbyint(sx), isy = nearbyint(sy);
    if (fabs(sx - isx) < 2.220446049250313e-16 && fabs(sy - isy) < 2.220446049250313e-16) {       // is_area_fast
        plan->path = FS_CVRESIZE_PATH_AREA_FAST;
        plan->factor_x = (int)isx;
        plan->factor_y = (int)isy;
        return 0;
    }
    plan->path = FS_CVRESIZE_PATH_AREA;
    plan->x_taps = area_tab(W, plan->dst_w, sx, nullptr, nullptr);
    plan->y_taps = area_tab(H, plan->dst_h, sy, nullptr, nullptr);
    plan->x_offset = 0;
    plan->y_offset = align_up(area_axis_bytes(plan->dst_w, plan->x_taps), 16);
    plan->table_bytes = plan->y_offset + align_up(area_axis_bytes(plan->dst_h, plan->y_taps), 16);
    return 0;
}

int fs_cvresize_tables(const fs_cvresize_info* plan, void* tables, size_t cap) {
    using namespace fs;
    if (!plan) return set_error(-1, "fs_cvresize_tables: null argument");
    if (!plan_matches(*plan)) return set_error(-1, "fs_cvresize_tables: the plan was not filled by fs_cvresize_plan");
    if (plan->table_bytes == 0) return 0;
    if (!tables) return set_error(-1, "fs_cvresize_tables: null argument");
    if ((uintptr_t)tables & 3) return set_error(-5, "fs_cvresize_tables: tables must be 4-byte aligned");
    if (cap < plan->table_bytes) return set_error(-1, "fs_cvresize_tables: tables holds %zu bytes, the plan needs %llu", cap, (unsigned long long)plan->table_bytes);
    unsigned char* t = static_cast<unsigned char*>(tables);
    memset(t, 0, (size_t)plan->table_bytes);
    const double sx = 1.0 / plan->fx, sy = 1.0 / plan->fy;
    if (plan->path == FS_CVRESIZE_PATH_CUBIC) {
        cubic_axis(plan->src_w, plan->dst_w, sx, reinterpret_cast<int32_t*>(t + plan->x_offset));
        cubic_axis(plan->src_h, plan->dst_h, sy, reinterpret_cast<int32_t*>(t + plan->y_offset));
    } else {
        unsigned char* x = t + plan->x_offset;
        unsigned char* y = t + plan->y_offset;
        area_tab(plan->src_w, plan->dst_w, sx, reinterpret_cast<int32_t*>(x),
                 reinterpret_cast<AreaTap*>(x + align_up(((size_t)plan->dst_w + 1) * 4, 8)));
        area_tab(plan->src_h, plan->dst_h, sy, reinterpret_cast<int32_t*>(y),
                 reinterpret_cast<AreaTap*>(y + align_up(((size_t)plan->dst_h + 1) * 4, 8)));
    }
    return 0;
}

}  // extern "C"
