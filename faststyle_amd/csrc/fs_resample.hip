// Resampling between fp32 tensors (include/faststyle_io.h states the arithmetic: Pillow's Image.resize on mode-F images -- double coefficients,
// double accumulation in tap order, a float32 result per pass, horizontal pass first, a pass of an unchanged axis skipped, nothing clamped).
//   host   -- fs_resample_plan / fs_resample_tables: sizes, tap capacities, table offsets, the tile geometry, and the per-axis tables; plain C++
//             with no global state and no allocation;
//   device -- one launch, one 256-thread workgroup per tile of 64 destination columns by tile_h destination rows of one image.  Phase 1 runs
//             the horizontal pass for exactly the source rows the tile's vertical taps span and leaves float32 results in LDS, phase 2 runs
//             the vertical pass out of LDS: the src_h x dst_w intermediate never reaches memory.  Both phases give a wave one row at a time
//             and a lane three floats of it, 64 apart (192 floats, channel-interleaved, per row), so a wave's LDS stores and loads are consecutive dwords
//             (conflict-free for any row pitch: a wave never spans two rows) and its global stores are consecutive floats.  No value read from
//             a tensor reaches an address, and every table entry is clamped into the source and every LDS row index into the array.
// Every product and sum is rounded on its own (`#pragma clang fp contract(off)`): a fused multiply-add would change bits.
#include "../../include/faststyle_io.h"

#include <cmath>
#include <cstring>

#include "fs_kernels.h"

namespace fs {
namespace {

constexpr int kMaxSide = 32767;
constexpr int kTileW = FS_RESAMPLE_TILE_W;
constexpr int kRowFloats = kTileW * 3;                 // one LDS row: 64 pixels, channel-interleaved
constexpr int kLdsRows = FS_RESAMPLE_LDS_ROWS;         // 85 * 192 * 4 = 65280 bytes
constexpr int kLdsSmall = 16, kLdsMid = 40;            // the smaller instances: 12 KB and 30 KB, for the occupancy of enlargements and mild shrinks
constexpr double kPi = 3.14159265358979323846;

inline size_t align_up(size_t n, size_t a) { return (n + a - 1) / a * a; }

// ---------------------------------------------------------------- host: filters and tables
double filter_support(int filter) {
    return filter == FS_RESAMPLE_BOX ? 0.5 : filter == FS_RESAMPLE_BILINEAR ? 1.0 : filter == FS_RESAMPLE_BICUBIC ? 2.0 : 3.0;
}

double sinc(double x) {
#pragma clang fp contract(off)
    if (x == 0.0) return 1.0;
    x = x * kPi;
    return sin(x) / x;
}

double filter_value(int filter, double x) {
#pragma clang fp contract(off)
    if (filter == FS_RESAMPLE_BOX) return (x > -0.5 && x <= 0.5) ? 1.0 : 0.0;
    if (filter == FS_RESAMPLE_LANCZOS) return (-3.0 <= x && x < 3.0) ? sinc(x) * sinc(x / 3.0) : 0.0;
    if (x < 0.0) x = -x;
    if (filter == FS_RESAMPLE_BILINEAR) return x < 1.0 ? 1.0 - x : 0.0;
    const double a = -0.5;
    if (x < 1.0) {
        double t = (a + 2.0) * x;
        t = t - (a + 3.0);
        t = t * x;
        t = t * x;
        return t + 1.0;
    }
    if (x < 2.0) {
        double t = x - 5.0;
        t = t * x;
        t = t + 8.0;
        t = t * x;
        t = t - 4.0;
        return t * a;
    }
    return 0.0;
}

struct Axis {
    double scale, support, inv;
    int ksize;
};

Axis axis_of(int n_in, int n_out, int filter) {
#pragma clang fp contract(off)
    Axis a;
    a.scale = (double)n_in / (double)n_out;
    const double fscale = a.scale < 1.0 ? 1.0 : a.scale;
    a.support = filter_support(filter) * fscale;
    a.inv = 1.0 / fscale;
    a.ksize = (int)ceil(a.support) * 2 + 1;
    return a;
}

// xmin and cnt of output index d; center where asked
inline void axis_bounds(const Axis& a, int n_in, int d, int* xmin, int* cnt, double* center_out) {
#pragma clang fp contract(off)
    const double center = ((double)d + 0.5) * a.scale;
    int lo = (int)(center - a.support + 0.5);
    if (lo < 0) lo = 0;
    int hi = (int)(center + a.support + 0.5);
    if (hi > n_in) hi = n_in;
    *xmin = lo;
    *cnt = hi - lo;
    if (center_out) *center_out = center;
}

inline size_t axis_stride(int ksize) { return 8 + (size_t)ksize * 8; }

void axis_table(int n_in, int n_out, int filter, unsigned char* t) {
#pragma clang fp contract(off)
    const Axis a = axis_of(n_in, n_out, filter);
    for (int d = 0; d < n_out; ++d) {
        int xmin, cnt;
        double center;
        axis_bounds(a, n_in, d, &xmin, &cnt, &center);
        unsigned char* e = t + (size_t)d * axis_stride(a.ksize);
        int32_t head[2] = {xmin, cnt};
        memcpy(e, head, 8);
        double* w = reinterpret_cast<double*>(e + 8);
        double ww = 0.0;
        for (int k = 0; k < cnt; ++k) {
            double x = (double)(k + xmin) - center;
            x = x + 0.5;
            w[k] = filter_value(filter, x * a.inv);
            ww = ww + w[k];
        }
        if (ww != 0.0)
            for (int k = 0; k < cnt; ++k) w[k] = w[k] / ww;
        for (int k = cnt < 0 ? 0 : cnt; k < a.ksize; ++k) w[k] = 0.0;
    }
}

// the most source rows the vertical taps of one tile of th destination rows span
int tile_span(const Axis& a, int n_in, int n_out, int th) {
    int most = 0;
    for (int d0 = 0; d0 < n_out; d0 += th) {
        int lo, c, hi = 0;
        axis_bounds(a, n_in, d0, &lo, &c, nullptr);
        const int d1 = d0 + th < n_out ? d0 + th : n_out;
        for (int d = d0; d < d1; ++d) {
            int m, n;
            axis_bounds(a, n_in, d, &m, &n, nullptr);
            hi = m + n > hi ? m + n : hi;
        }
        most = hi - lo > most ? hi - lo : most;
    }
    return most;
}

bool plan_matches(const fs_resample_info& p) {
    fs_resample_info want;
    if (fs_resample_plan(p.src_h, p.src_w, p.dst_h, p.dst_w, p.filter, &want)) return false;
    return !memcmp(&want, &p, sizeof(want));
}

// ---------------------------------------------------------------- device
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// one table entry, held to the source: first in [0, n_in - 1], cnt in [0, min(ksize, n_in - first)]
__device__ __forceinline__ const double* entry(const unsigned char* axis, int ksize, int d, int n_in, int& first, int& cnt) {
    const unsigned char* e = axis + (size_t)d * (8 + (size_t)ksize * 8);
    const int* head = reinterpret_cast<const int*>(e);
    first = clampi(head[0], 0, n_in - 1);
    const int room = n_in - first < ksize ? n_in - first : ksize;
    cnt = clampi(head[1], 0, room);
    return reinterpret_cast<const double*>(e + 8);
}

// The table entries a tile needs, staged in LDS where they fit (all but the 85-row instance, whose LDS the rows fill): 64 columns of the x
// axis in kStageX bytes, tile_h rows of the y axis in kStageY bytes.  Entries that do not fit are read from memory through the same pointer.
constexpr int kStageX = 8192, kStageY = 4096;

template <int ROWS>
__global__ __launch_bounds__(256) void resample_kernel(const fs_resample_info P, const unsigned char* __restrict__ tables,
                                                       const float* __restrict__ src, int src_rows, int src_pitch, float* __restrict__ dst) {
#pragma clang fp contract(off)
    constexpr bool kStage = ROWS < kLdsRows;
    __shared__ float lds[ROWS * kRowFloats];
    __shared__ unsigned long long xstage[kStage ? kStageX / 8 : 1];
    __shared__ unsigned long long ystage[kStage ? kStageY / 8 : 1];
    const int tiles_x = (P.dst_w + kTileW - 1) / kTileW;
    const int tyi = (int)blockIdx.x / tiles_x, txi = (int)blockIdx.x - tyi * tiles_x;
    const int x0 = txi * kTileW, y0 = tyi * P.tile_h;
    if (y0 >= P.dst_h) return;                                                   // (whole workgroup: no barrier is skipped by a part of it)
    const int cols = P.dst_w - x0 < kTileW ? P.dst_w - x0 : kTileW;
    const int rows = P.dst_h - y0 < P.tile_h ? P.dst_h - y0 : P.tile_h;
    const int floats = cols * 3;
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    // xt / yt: entry 0 is the tile's first column / row
    const int xstride = 8 + 8 * P.x_ksize, ystride = 8 + 8 * P.y_ksize;
    const unsigned char* xt = tables + P.x_offset + (size_t)x0 * xstride;
    const unsigned char* yt = tables + P.y_offset + (size_t)y0 * ystride;
    if (kStage) {
        const bool sx = P.x_ksize && kTileW * xstride <= kStageX, sy = P.y_ksize && P.tile_h * ystride <= kStageY;
        if (sx) {
            const unsigned long long* g = reinterpret_cast<const unsigned long long*>(xt);
            for (int i = (int)threadIdx.x; i < cols * xstride / 8; i += 256) xstage[i] = g[i];
            xt = reinterpret_cast<const unsigned char*>(xstage);
        }
        if (sy) {
            const unsigned long long* g = reinterpret_cast<const unsigned long long*>(yt);
            for (int i = (int)threadIdx.x; i < rows * ystride / 8; i += 256) ystage[i] = g[i];
            yt = reinterpret_cast<const unsigned char*>(ystage);
        }
        __syncthreads();
    }

    // the source rows this tile's vertical taps span: [s0, s0 + nrows)
    int s0 = y0, s1 = y0 + rows;
    if (P.y_ksize) {
        int m, c;
        entry(yt, P.y_ksize, 0, P.src_h, m, c);
        s0 = m;
        s1 = m;
        for (int r = 0; r < rows; ++r) {
            entry(yt, P.y_ksize, r, P.src_h, m, c);
            s1 = m + c > s1 ? m + c : s1;
        }
    }
    const int nrows = s1 - s0 < ROWS ? s1 - s0 : ROWS;                           // (s1 <= src_h by the clamps)

    // phase 1: the horizontal pass of those rows into LDS, float32.  A lane owns floats lane, lane + 64, lane + 128 of a row: three
    // independent sums, each in its own tap order.
    const float* __restrict__ img = src + (size_t)blockIdx.y * (size_t)src_rows * (size_t)src_pitch * 3;
    if (P.x_ksize) {
        int xm[3], xn[3], nmax = 0;
        const double* xw[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int e = lane + 64 * j, col = e / 3;
            xm[j] = 0;
            xn[j] = 0;
            xw[j] = nullptr;
            if (e < floats) {
                xw[j] = entry(xt, P.x_ksize, col, P.src_w, xm[j], xn[j]);
                xm[j] = xm[j] * 3 + (e - col * 3);
            }
            nmax = xn[j] > nmax ? xn[j] : nmax;
        }
        for (int r = wave; r < nrows; r += 4) {
            const float* __restrict__ row = img + (size_t)(s0 + r) * (size_t)src_pitch * 3;
            double ss[3] = {0.0, 0.0, 0.0};
            for (int k = 0; k < nmax; ++k) {
#pragma unroll
                for (int j = 0; j < 3; ++j)
                    if (k < xn[j]) {
                        const double t = (double)row[xm[j] + k * 3] * xw[j][k];
                        ss[j] = ss[j] + t;
                    }
            }
#pragma unroll
            for (int j = 0; j < 3; ++j)
                if (lane + 64 * j < floats) lds[r * kRowFloats + lane + 64 * j] = (float)ss[j];
        }
    } else {
        for (int r = wave; r < nrows; r += 4) {
            const float* __restrict__ row = img + ((size_t)(s0 + r) * (size_t)src_pitch + (size_t)x0) * 3;
            for (int e = lane; e < floats; e += 64) lds[r * kRowFloats + e] = row[e];
        }
    }
    __syncthreads();

    // phase 2: the vertical pass out of LDS, consecutive floats of a destination row per wave, the lane's three sums side by side
    for (int r = wave; r < rows; r += 4) {
        float* __restrict__ out = dst + (((size_t)blockIdx.y * P.dst_h + (size_t)(y0 + r)) * P.dst_w + (size_t)x0) * 3;
        if (P.y_ksize) {
            int m, n;
            const double* w = entry(yt, P.y_ksize, r, P.src_h, m, n);
            const int base = m - s0;
            double ss[3] = {0.0, 0.0, 0.0};
            for (int k = 0; k < n; ++k) {
                const float* __restrict__ line = lds + clampi(base + k, 0, ROWS - 1) * kRowFloats;
                const double wk = w[k];
#pragma unroll
                for (int j = 0; j < 3; ++j)
                    if (lane + 64 * j < floats) {
                        const double t = (double)line[lane + 64 * j] * wk;
                        ss[j] = ss[j] + t;
                    }
            }
#pragma unroll
            for (int j = 0; j < 3; ++j)
                if (lane + 64 * j < floats) out[lane + 64 * j] = (float)ss[j];
        } else {
            const int i = clampi(r, 0, ROWS - 1);
            for (int e = lane; e < floats; e += 64) out[e] = lds[i * kRowFloats + e];
        }
    }
}

}  // namespace

bool resample_plan_ok(const fs_resample_info& p) { return plan_matches(p); }

// plan: checked by the caller (fs_api.hip: resample_plan_ok)
int resample_f32(const fs_resample_info& P, const unsigned char* tables, const float* src, int src_rows, int src_pitch, int N, float* dst,
                 hipStream_t s) {
    const long long tiles = (long long)((P.dst_w + kTileW - 1) / kTileW) * ((P.dst_h + P.tile_h - 1) / P.tile_h);
    const dim3 grid((unsigned)tiles, (unsigned)N), block(256);
    if (P.lds_rows == kLdsSmall) hipLaunchKernelGGL(resample_kernel<kLdsSmall>, grid, block, 0, s, P, tables, src, src_rows, src_pitch, dst);
    else if (P.lds_rows == kLdsMid) hipLaunchKernelGGL(resample_kernel<kLdsMid>, grid, block, 0, s, P, tables, src, src_rows, src_pitch, dst);
    else hipLaunchKernelGGL(resample_kernel<kLdsRows>, grid, block, 0, s, P, tables, src, src_rows, src_pitch, dst);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace fs

extern "C" {

int fs_resample_plan(int src_h, int src_w, int dst_h, int dst_w, int filter, fs_resample_info* plan) {
    using namespace fs;
    if (!plan) return set_error(-1, "fs_resample_plan: null argument");
    if (src_h < 1 || src_w < 1 || src_h > kMaxSide || src_w > kMaxSide || dst_h < 1 || dst_w < 1 || dst_h > kMaxSide || dst_w > kMaxSide)
        return set_error(-1, "fs_resample_plan: %dx%d -> %dx%d has a side outside [1, %d]", src_h, src_w, dst_h, dst_w, kMaxSide);
    if (filter < FS_RESAMPLE_BOX || filter > FS_RESAMPLE_LANCZOS)
        return set_error(-2, "fs_resample_plan: filter %d is none of box (0), bilinear (1), bicubic (2), lanczos (3)", filter);
    fs_resample_info p;
    memset(&p, 0, sizeof(p));
    p.src_h = src_h;
    p.src_w = src_w;
    p.dst_h = dst_h;
    p.dst_w = dst_w;
    p.filter = filter;
    p.tile_w = kTileW;
    p.x_ksize = src_w == dst_w ? 0 : axis_of(src_w, dst_w, filter).ksize;
    p.tile_h = 16;
    p.tile_rows = 16;
    if (src_h != dst_h) {
        const Axis a = axis_of(src_h, dst_h, filter);
        p.y_ksize = a.ksize;
        for (p.tile_h = 16; p.tile_h >= 1; p.tile_h >>= 1) {
            p.tile_rows = tile_span(a, src_h, dst_h, p.tile_h);
            if (p.tile_rows <= kLdsRows) break;
        }
        if (p.tile_h < 1)
            return set_error(-2, "fs_resample_plan: %d -> %d rows: one output row takes %d source rows, a tile's LDS holds %d", src_h, dst_h, p.tile_rows,
                             kLdsRows);
    }
    p.lds_rows = p.tile_rows <= kLdsSmall ? kLdsSmall : (p.tile_rows <= kLdsMid ? kLdsMid : kLdsRows);
    p.x_offset = 0;
    p.y_offset = p.x_ksize ? align_up((size_t)dst_w * axis_stride(p.x_ksize), 16) : 0;
    p.table_bytes = p.y_offset + (p.y_ksize ? align_up((size_t)dst_h * axis_stride(p.y_ksize), 16) : 0);
    *plan = p;
    return 0;
}

int fs_resample_tables(const fs_resample_info* plan, void* tables, size_t cap) {
    using namespace fs;
    if (!plan) return set_error(-1, "fs_resample_tables: null argument");
    if (!plan_matches(*plan)) return set_error(-1, "fs_resample_tables: the plan was not filled by fs_resample_plan");
    if (plan->table_bytes == 0) return 0;
    if (!tables) return set_error(-1, "fs_resample_tables: null argument");
    if ((uintptr_t)tables & 7) return set_error(-5, "fs_resample_tables: tables must be 8-byte aligned");
    if (cap < plan->table_bytes)
        return set_error(-1, "fs_resample_tables: tables holds %zu bytes, the plan needs %llu", cap, (unsigned long long)plan->table_bytes);
    unsigned char* t = static_cast<unsigned char*>(tables);
    memset(t, 0, (size_t)plan->table_bytes);
    if (plan->x_ksize) axis_table(plan->src_w, plan->dst_w, plan->filter, t + plan->x_offset);
    if (plan->y_ksize) axis_table(plan->src_h, plan->dst_h, plan->filter, t + plan->y_offset);
    return 0;
}

}  // extern "C"
