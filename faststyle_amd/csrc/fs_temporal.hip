// Temporal stabilisation between the forward pass (or compose) and the output conversions (include/faststyle_io.h, whose comments are the
// arithmetic contract): a byte luma of the net's input on the output grid, a block-matching motion search between this luma and the previous
// frame's, and a per-pixel blend of the new output towards the previous stabilised output fetched along the block vectors, weighted by how
// well the source matched there.  faststyle_amd/stream.py (temporal=) keeps the two state slots and runs the launches behind compose.
// One pipeline with options (TemporalCall, fs_kernels.h), launched by temporal_run for every entry point of the header:
//   luma    -- elementwise, the thread layout of compose_kernel: four pixels of an output row.
//   pyramid -- levels > 1: halves the luma once or twice (elementwise, one launch).
//   search  -- one launch per level, coarsest first, each on a window displaced by twice the coarser level's vector (held to its bound before
//              it reaches an address).  One workgroup of 256 threads per 16x16 block, one thread per candidate (dy, dx) in [-R, R]^2 (225 at
//              R = 7).  The block's luma (16 rows of 16 bytes, zero outside the frame) and the previous luma's (16 + 2R)^2 window go to LDS
//              with the clamped coordinates applied, so the inner loop has no bounds logic; a ragged block runs `rows` rows (uniform) and
//              masks the window's dwords beyond `cols` (uniform), where the block's own bytes are zero already.  A candidate reads, per row,
//              the five aligned dwords that hold its sixteen bytes, shifts them into place and adds four packed-byte SADs against the block's
//              dwords (the same address in every lane: a broadcast).  Window pitch 32 bytes = 8 banks: the lanes of a 32-lane group are
//              candidates of at most 4 consecutive dy (15 apart is one row down) and of dword columns 0 ... 3 + k, so they touch 4 rows x 8
//              banks, each bank once per distinct address -- conflict-free by the rule that ds_read_b32 banks are (a / 4) mod 32 per 32-lane
//              half.  The 256 keys are reduced by an LDS min tree.
//   subpel  -- subpel > 0: a fraction per block in quarter pixels from five SADs around the whole-pixel winner (described at the kernel).
//   blend   -- one launch per frame, elementwise, four pixels of an output row.  One body in three instantiations: along the block's whole-pixel
//              vector, along vector plus fraction with a bilinear fetch (subpel > 0), or along the vectors of the four blocks whose centres
//              surround the pixel (overlap 1).
// Frames: a call covers `frames` consecutive frames.  Only the blend is recursive, so the launches before it run once over all frames with the
// frame index f as one more grid dimension (blockIdx.y of the luma's 1-D grid, blockIdx.z of the others).  A buffer of frame f lies in the work
// buffer's slot f, except the last frame's, which is the state's (pointer selection, no copy launch); frame f's "previous" is slot f - 1, for
// f = 0 the state the previous call wrote (null: no previous frame).  f is uniform per workgroup and held below `frames`, so the selection
// stays in scalar registers.  The selection costs a call of one frame 0.2 to 0.3 us per launch, so luma, pyramid, search and
// refinement are a body with two entries: *_kernel takes one frame's pointers (frames == 1: no work buffer), *_batch_kernel selects them.
// Streams: a call covers `streams` independent streams, one frame of each (fs_temporal_streams_f32).  Nothing is recursive inside such a pass,
// so every launch, the blend included, runs once over all streams with the stream index s as one more grid dimension (blockIdx.y of the 1-D
// grids, blockIdx.z of the others), held below `streams`: the third set of entries, *_streams_kernel, of the same bodies.  The state of all
// streams is one buffer, per stream two slots of [luma | out88 | pyr | mv | mvf] (fs_temporal_streams_layout).  What differs per stream --
// whether it has a previous frame, which slot it writes, whether it takes part -- is the device word ctl[s] (FS_TS_PREV, FS_TS_SLOT,
// FS_TS_SKIP), read once per workgroup: s is uniform, so the read and the pointer selection stay in scalar registers, as the frame selection
// does.  A skipped stream's workgroups return before their first access and before any barrier.
// No value read from a tensor reaches an address except through mv and mvf, which the search and the refinement bound and every reader holds
// to those bounds again together with the displaced coordinates, and through the slot index (ctl[s] >> 1) & 1 of a streams call, which the
// mask bounds.  The arithmetic is integer throughout.
#include <cstring>

#include "../../include/faststyle_io.h"

#include "fs_kernels.h"

namespace fs {
namespace {

constexpr int TB = 16;                      // block edge
constexpr int TRMAX = 7;                    // largest search radius
constexpr int TPITCH = 32;                  // bytes per LDS window row: 16 + 2 * 7 = 30 used, the five-dword read of column 14 ends at byte 31
constexpr int TWROWS = TB + 2 * TRMAX;      // 30
constexpr int SPITCH = 12;                  // dwords per LDS window row of the refinement: 5 used (18 bytes, the read of dword 4 ends at byte 19)
constexpr int SWROWS = TB + 2;              // 18

// the float on the 8.8 scale, as compose_kernel's: clamped to [0, 255] (NaN: 0), times 256 (exact), truncated
__device__ __forceinline__ int temporal_f88(float v) { return (int)(fminf(fmaxf(v, 0.f), 255.f) * 256.0f); }

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// v held to [-bound, bound]
__device__ __forceinline__ int hold_to(int v, int bound) { return v < -bound ? -bound : (v > bound ? bound : v); }

// acc + the four absolute byte differences of a and b
__device__ __forceinline__ unsigned sad4(unsigned a, unsigned b, unsigned acc) {
#ifndef FS_EMULATOR
    return __builtin_amdgcn_sad_u8(a, b, acc);
#else
    for (int k = 0; k < 4; ++k) {
        const int x = (int)((a >> (8 * k)) & 0xFFu), y = (int)((b >> (8 * k)) & 0xFFu);
        acc += (unsigned)(x > y ? x - y : y - x);
    }
    return acc;
#endif
}

struct FrameSel {
    unsigned char* work;                    // slot f at work + f * slot, f < frames - 1
    unsigned long long slot;
    int frames;
};

// one buffer of every frame: the last frame's (in the state written), frame 0's predecessor (in the state read, or null), the offset in a slot
struct FrameBuf {
    unsigned char* last;
    const unsigned char* before;
    unsigned long long off;
};

__device__ __forceinline__ unsigned char* frame_at(const FrameSel& S, const FrameBuf& B, int f) {
    if (f == S.frames - 1) return B.last;
    return S.work + (size_t)f * S.slot + B.off;
}

__device__ __forceinline__ const unsigned char* frame_before(const FrameSel& S, const FrameBuf& B, int f) {
    if (f == 0) return B.before;
    return S.work + (size_t)(f - 1) * S.slot + B.off;
}

// the streams of a call: the control words, the state of all streams, the strides of a slot and of a stream (two slots)
struct StreamSel {
    const int* ctl;
    unsigned char* state;
    unsigned long long slot, stream;
    int streams;
};

// the two slots of stream s: wr the one this pass writes, rd the one it reads (null: a first frame).  False: nothing of s is touched.
struct StreamAt {
    unsigned char* wr;
    const unsigned char* rd;
};

__device__ __forceinline__ bool stream_at(const StreamSel& T, int s, StreamAt& at) {
    if (s >= T.streams) return false;
    const int c = T.ctl[s] & 7;                             // (uniform per workgroup)
    if (c & FS_TS_SKIP) return false;
    const int w = (c >> 1) & 1;                             // the only value from the control buffer that reaches an address: 0 or 1
    unsigned char* base = T.state + (size_t)s * T.stream;
    at.wr = base + (size_t)w * T.slot;
    at.rd = (c & FS_TS_PREV) ? base + (size_t)(w ^ 1) * T.slot : nullptr;
    return true;
}

struct LumaArgs {
    int H, W, Ho, Wo;
    int k0, k1, k2;                         // luma weights by 2^16 of the channels as stored (k0 is kb when channel 0 is blue)
};

// Thread i: row y = i / groups, pixels x0 = 4 * (i % groups) ... x0 + 3 (groups = ceil(Wo / 4)); the source is read at (min(y, H - 1), min(x, W - 1)).
__device__ __forceinline__ void temporal_luma_body(const LumaArgs& A, const float* __restrict__ src, unsigned char* __restrict__ luma) {
    const int groups = (A.Wo + 3) >> 2;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)groups * A.Ho) return;
    const int y = (int)(i / groups), x0 = (int)(i - (long long)y * groups) * 4;
    const int ys = y < A.H ? y : A.H - 1;
    const float* srow = src + (size_t)ys * A.W * 3;
    unsigned char* lrow = luma + (size_t)y * A.Wo;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int x = x0 + k;
        if (x >= A.Wo) break;
        const int xs = x < A.W ? x : A.W - 1;
        const int A0 = temporal_f88(srow[(size_t)xs * 3]), A1 = temporal_f88(srow[(size_t)xs * 3 + 1]), A2 = temporal_f88(srow[(size_t)xs * 3 + 2]);
        const long long Y = ((long long)A.k0 * A0 + (long long)A.k1 * A1 + (long long)A.k2 * A2 + 32768) >> 16;       // 0 ... 65280
        lrow[x] = (unsigned char)(Y >> 8);
    }
}

__global__ __launch_bounds__(256) void temporal_luma_kernel(const LumaArgs A, const float* __restrict__ src, unsigned char* __restrict__ luma) {
    temporal_luma_body(A, src, luma);
}

__global__ __launch_bounds__(256) void temporal_luma_batch_kernel(const LumaArgs A, const FrameSel S, const FrameBuf L, const float* __restrict__ src) {
    const int f = (int)blockIdx.y;
    if (f >= S.frames) return;
    temporal_luma_body(A, src + (size_t)f * A.H * A.W * 3, frame_at(S, L, f));
}

// (loff: the luma's offset in a slot, here and below)
__global__ __launch_bounds__(256) void temporal_luma_streams_kernel(const LumaArgs A, const StreamSel T, unsigned long long loff,
                                                                    const float* __restrict__ src) {
    const int s = (int)blockIdx.y;
    StreamAt at;
    if (!stream_at(T, s, at)) return;
    temporal_luma_body(A, src + (size_t)s * A.H * A.W * 3, at.wr + loff);
}

struct PyrArgs {
    int H0, W0, H1, W1;
    int H2, W2;                             // 0, 0 with two levels
};

// the byte of level 1 at (y, x) from level 0: the rounded mean of its 2 x 2 bytes, the odd edge clamped
__device__ __forceinline__ int pyr_level1(const unsigned char* __restrict__ l0, int H0, int W0, int y, int x) {
    const int ya = 2 * y < H0 - 1 ? 2 * y : H0 - 1, yb = 2 * y + 1 < H0 - 1 ? 2 * y + 1 : H0 - 1;
    const int xa = 2 * x < W0 - 1 ? 2 * x : W0 - 1, xb = 2 * x + 1 < W0 - 1 ? 2 * x + 1 : W0 - 1;
    const unsigned char* ra = l0 + (size_t)ya * W0;
    const unsigned char* rb = l0 + (size_t)yb * W0;
    return ((int)ra[xa] + (int)ra[xb] + (int)rb[xa] + (int)rb[xb] + 2) >> 2;
}

// Levels 1 and 2 in one launch: workgroup row blockIdx.x < H1 is row y of level 1, row H1 + y is row y of level 2; thread
// blockIdx.y * 256 + t writes the four bytes x0 = 4 (...) ... x0 + 3 of that row.  A byte of level 2 comes from its four level-1 bytes
// recomputed from level 0 with the nested rounding and clamps, so level 2 does not wait for level 1.  Bytes throughout: the buffers are held
// to no alignment.
__device__ __forceinline__ void temporal_pyramid_body(const PyrArgs& A, const unsigned char* __restrict__ l0, unsigned char* __restrict__ l1,
                                                      unsigned char* __restrict__ l2) {
    const int x0 = ((int)blockIdx.y * 256 + (int)threadIdx.x) * 4;
    int y = (int)blockIdx.x;
    if (y < A.H1) {                                         // (uniform per workgroup)
        unsigned char* row = l1 + (size_t)y * A.W1;
        for (int x = x0; x < x0 + 4 && x < A.W1; ++x) row[x] = (unsigned char)pyr_level1(l0, A.H0, A.W0, y, x);
        return;
    }
    y -= A.H1;                                              // below H2: the grid has H1 + H2 rows
    const int ya = 2 * y < A.H1 - 1 ? 2 * y : A.H1 - 1, yb = 2 * y + 1 < A.H1 - 1 ? 2 * y + 1 : A.H1 - 1;
    unsigned char* row = l2 + (size_t)y * A.W2;
    for (int x = x0; x < x0 + 4 && x < A.W2; ++x) {
        const int xa = 2 * x < A.W1 - 1 ? 2 * x : A.W1 - 1, xb = 2 * x + 1 < A.W1 - 1 ? 2 * x + 1 : A.W1 - 1;
        row[x] = (unsigned char)((pyr_level1(l0, A.H0, A.W0, ya, xa) + pyr_level1(l0, A.H0, A.W0, ya, xb) + pyr_level1(l0, A.H0, A.W0, yb, xa) +
                                  pyr_level1(l0, A.H0, A.W0, yb, xb) + 2) >> 2);
    }
}

__global__ __launch_bounds__(256) void temporal_pyramid_kernel(const PyrArgs A, const unsigned char* __restrict__ l0, unsigned char* __restrict__ l1,
                                                               unsigned char* __restrict__ l2) {
    temporal_pyramid_body(A, l0, l1, l2);
}

__global__ __launch_bounds__(256) void temporal_pyramid_batch_kernel(const PyrArgs A, const FrameSel S, const FrameBuf L0, const FrameBuf L1,
                                                                     const FrameBuf L2) {
    const int f = (int)blockIdx.z;
    if (f >= S.frames) return;
    temporal_pyramid_body(A, frame_at(S, L0, f), frame_at(S, L1, f), A.H2 > 0 ? frame_at(S, L2, f) : nullptr);
}

__global__ __launch_bounds__(256) void temporal_pyramid_streams_kernel(const PyrArgs A, const StreamSel T, unsigned long long l0off,
                                                                       unsigned long long l1off, unsigned long long l2off) {
    StreamAt at;
    if (!stream_at(T, (int)blockIdx.z, at)) return;
    temporal_pyramid_body(A, at.wr + l0off, at.wr + l1off, A.H2 > 0 ? at.wr + l2off : nullptr);
}

// One level (cur8 / prev8 [H, W]), one workgroup per block (blockIdx.y, blockIdx.x).  prev8 == nullptr (no previous frame): every vector is
// (0, 0).  The window's origin is displaced by the block's predictor, twice the vector of block (by >> 1, bx >> 1) of the coarser level
// (parent [.., pnbx, 2]; nullptr at the coarsest level: (0, 0)), held to `hold` per component before it reaches an address: the window is
// (y0 + py - R, x0 + px - R) ..., each byte clamped into the level.  The winner is the predictor plus the refinement.
__device__ __forceinline__ void temporal_search_body(const unsigned char* __restrict__ cur8, const unsigned char* __restrict__ prev8, int H, int W, int R,
                                                     const signed char* __restrict__ parent, int pnbx, int hold, signed char* __restrict__ v) {
    __shared__ unsigned win[TWROWS * (TPITCH / 4)];         // the previous luma's window, row pitch 8 dwords
    __shared__ unsigned blk[TB * (TB / 4)];                 // the block's luma, 4 dwords per row, zero outside the frame
    __shared__ unsigned keys[256];
    const int t = (int)threadIdx.x;
    const int bx = (int)blockIdx.x, by = (int)blockIdx.y;
    signed char* out = v + ((size_t)by * gridDim.x + bx) * 2;
    if (prev8 == nullptr) {                                 // (uniform per workgroup)
        if (t == 0) { out[0] = 0; out[1] = 0; }
        return;
    }
    int py = 0, px = 0;
    if (parent != nullptr) {                                // (uniform per launch)
        const signed char* p = parent + ((size_t)(by >> 1) * pnbx + (bx >> 1)) * 2;
        py = hold_to(2 * (int)p[0], hold);                  // (the coarser search wrote them within it; held to it again)
        px = hold_to(2 * (int)p[1], hold);
    }
    const int y0 = by * TB, x0 = bx * TB;
    const int rows = H - y0 < TB ? H - y0 : TB, cols = W - x0 < TB ? W - x0 : TB;            // at least 1 each
    const int n = 2 * R + 1;
    if (t < (TB + 2 * R) * (TPITCH / 4)) {                  // window row t / 8, dword t % 8: level rows y0 + py - R ..., columns x0 + px - R ...
        const int wr = t >> 3, wc = (t & 7) * 4;
        const unsigned char* prow = prev8 + (size_t)clampi(y0 + py - R + wr, H - 1) * W;
        unsigned u = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) u |= (unsigned)prow[clampi(x0 + px - R + wc + b, W - 1)] << (8 * b);
        win[t] = u;
    }
    if (t < TB * (TB / 4)) {                                // block row t / 4, dword t % 4
        const int r = t >> 2, c = (t & 3) * 4;
        unsigned u = 0;
        if (r < rows) {
            const unsigned char* crow = cur8 + (size_t)(y0 + r) * W + x0;
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (c + b < cols) u |= (unsigned)crow[c + b] << (8 * b);
        }
        blk[t] = u;
    }
    __syncthreads();
    unsigned key = 0xFFFFFFFFu;
    if (t < n * n) {
        const int ryi = t / n, rxi = t - ryi * n;           // ry + R, rx + R: the window's row and column of the candidate's first pixel
        const int ry = ryi - R, rx = rxi - R;
        unsigned m[4];                                      // the bytes of dword k that lie inside the block
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int inside = cols - 4 * k;
            m[k] = inside >= 4 ? 0xFFFFFFFFu : (inside <= 0 ? 0u : (1u << (8 * inside)) - 1u);
        }
        const int sh = (rxi & 3) * 8;
        const unsigned* wp = win + ryi * (TPITCH / 4) + (rxi >> 2);          // (rxi >> 2) + 4 <= 7: inside the row
        unsigned sad = 0;
        for (int r = 0; r < rows; ++r) {
            const unsigned* w = wp + r * (TPITCH / 4);
            const unsigned* c = blk + r * 4;
            unsigned lo = w[0];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const unsigned hi = w[k + 1];
                const unsigned a = (unsigned)((((unsigned long long)hi << 32) | lo) >> sh);
                sad = sad4(a & m[k], c[k], sad);
                lo = hi;
            }
        }
        const int mag = (ry < 0 ? -ry : ry) + (rx < 0 ? -rx : rx);
        const unsigned cost = sad + (unsigned)(((rows * cols) >> 5) * mag);              // below 2^17
        key = (cost << 12) | ((unsigned)mag << 8) | ((unsigned)(ry + 7) << 4) | (unsigned)(rx + 7);
    }
    keys[t] = key;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) {
            const unsigned a = keys[t], b = keys[t + s];
            keys[t] = a < b ? a : b;
        }
        __syncthreads();
    }
    if (t == 0) {
        const unsigned k = keys[0];
        out[0] = (signed char)(py + (int)((k >> 4) & 15u) - 7);                          // |.| <= hold + R <= 49
        out[1] = (signed char)(px + (int)(k & 15u) - 7);
    }
}

__global__ __launch_bounds__(256) void temporal_search_kernel(const unsigned char* __restrict__ cur8, const unsigned char* __restrict__ prev8, int H, int W,
                                                              int R, const signed char* __restrict__ parent, int pnbx, int hold,
                                                              signed char* __restrict__ v) {
    temporal_search_body(cur8, prev8, H, W, R, parent, pnbx, hold, v);
}

// C: the level's luma (its predecessor: the previous luma), P: the coarser level's vectors (has_parent 0: none), V: the vectors written
__global__ __launch_bounds__(256) void temporal_search_batch_kernel(const FrameSel S, const FrameBuf C, int H, int W, int R, const FrameBuf P, int has_parent,
                                                                    int pnbx, int hold, const FrameBuf V) {
    const int f = (int)blockIdx.z;
    if (f >= S.frames) return;
    temporal_search_body(frame_at(S, C, f), frame_before(S, C, f), H, W, R, has_parent ? (const signed char*)frame_at(S, P, f) : nullptr, pnbx, hold,
                         (signed char*)frame_at(S, V, f));
}

// coff: the level's luma in a slot (its predecessor: the same place in the slot read), poff: the coarser level's vectors, voff: those written
__global__ __launch_bounds__(256) void temporal_search_streams_kernel(const StreamSel T, unsigned long long coff, int H, int W, int R,
                                                                      unsigned long long poff, int has_parent, int pnbx, int hold,
                                                                      unsigned long long voff) {
    StreamAt at;
    if (!stream_at(T, (int)blockIdx.z, at)) return;         // (before the body's first barrier, the whole workgroup alike)
    temporal_search_body(at.wr + coff, at.rd ? at.rd + coff : nullptr, H, W, R, has_parent ? (const signed char*)(at.wr + poff) : nullptr, pnbx, hold,
                         (signed char*)(at.wr + voff));
}

// the contract's fit: m, p the SADs one pixel before / after the winner's s0 along one axis -> the fraction in quarter pixels
__device__ __forceinline__ int subpel_fit(int s0, int m, int p, int S) {
    const int E = (m > p ? m : p) - s0;
    if (E <= 0) return 0;
    const int num = (m - p) * (1 << S) + E, den = 2 * E;    // |num| < 2^20
    int g = num / den;
    if (num < 0 && g * den != num) --g;                     // a true floor
    const int half = 1 << (S - 1);
    g = g < -half ? -half : (g > half ? half : g);
    return g * (1 << (2 - S));
}

// The refinement: one workgroup of 256 threads per 16x16 block (blockIdx.y, blockIdx.x) of level 0.  prev8 == nullptr (no previous frame) or
// R == 0: every fraction is (0, 0).  The previous luma's 18 x 18 window around the block displaced by its
// vector (one pixel more on every side, every coordinate clamped) and the block's bytes go to LDS as in the search.  Thread t has block row
// (t >> 2) & 15 and dword t & 3 of that row; the wave t >> 6 says which sums it forms: 0 the row above, 1 the row below, 2 the columns left and
// right, 3 the winner itself.  A thread reads the two window dwords that hold its four bytes, shifts them into place and adds one packed-byte
// SAD per sum.  Window pitch 12 dwords: the lanes of a 32-lane half are 8 consecutive rows x 4 dwords at dword address 12 row + k (+ a
// constant per wave), and 12 row mod 32 over 8 consecutive rows is a permutation of {0, 4, ..., 28} -- 32 lanes on 32 banks, conflict-free by
// the rule that ds_read_b32 (and ds_read2_b32) banks are (a / 4) mod 32 per 32-lane half; the block's dwords are at 4 row + k, the lane's own
// index.  The five sums of 64 partial sums each are reduced by an LDS tree; thread 0 fits and writes the fraction.  mv is held to `hold` per
// component before it reaches an address; nothing else read from a buffer does.
__device__ __forceinline__ void temporal_subpel_body(const unsigned char* __restrict__ cur8, const unsigned char* __restrict__ prev8, int Ho, int Wo,
                                                     int R, int hold, int Sp, const signed char* __restrict__ mv, signed char* __restrict__ mvf) {
    __shared__ unsigned win[SWROWS * SPITCH];
    __shared__ unsigned blk[TB * (TB / 4)];
    __shared__ unsigned part[5 * 64];                       // S0, Sym, Syp, Sxm, Sxp: 64 partial sums each
    const int t = (int)threadIdx.x;
    const int bx = (int)blockIdx.x, by = (int)blockIdx.y;
    const size_t b = (size_t)by * gridDim.x + bx;
    signed char* out = mvf + b * 2;
    if (prev8 == nullptr || R == 0) {                       // (uniform per workgroup)
        if (t == 0) { out[0] = 0; out[1] = 0; }
        return;
    }
    const int dy = hold_to((int)mv[b * 2], hold), dx = hold_to((int)mv[b * 2 + 1], hold);   // (the search wrote them within it; held to it again)
    const int y0 = by * TB, x0 = bx * TB;
    const int rows = Ho - y0 < TB ? Ho - y0 : TB, cols = Wo - x0 < TB ? Wo - x0 : TB;        // at least 1 each
    if (t < SWROWS * 5) {                                   // window row t / 5, dword t % 5: frame rows y0 + dy - 1 ..., columns x0 + dx - 1 ...
        const int wr = t / 5, wd = t - wr * 5;
        const unsigned char* prow = prev8 + (size_t)clampi(y0 + dy - 1 + wr, Ho - 1) * Wo;
        unsigned v = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) v |= (unsigned)prow[clampi(x0 + dx - 1 + wd * 4 + k, Wo - 1)] << (8 * k);
        win[wr * SPITCH + wd] = v;
    }
    if (t < TB * (TB / 4)) {                                // block row t / 4, dword t % 4
        const int r = t >> 2, c = (t & 3) * 4;
        unsigned v = 0;
        if (r < rows) {
            const unsigned char* crow = cur8 + (size_t)(y0 + r) * Wo + x0;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (c + k < cols) v |= (unsigned)crow[c + k] << (8 * k);
        }
        blk[t] = v;
    }
    __syncthreads();
    {
        const int r = (t >> 2) & 15, k = t & 3, which = t >> 6;                 // (which: uniform per wave)
        const int inside = cols - 4 * k;
        const unsigned m = r >= rows || inside <= 0 ? 0u : (inside >= 4 ? 0xFFFFFFFFu : (1u << (8 * inside)) - 1u);
        const unsigned c = blk[r * 4 + k];                  // (zero outside the frame, as the masked window bytes are)
        const int wr = r + (which == 0 ? 0 : (which == 1 ? 2 : 1));             // the window's row of the block's row r: r + 1 + u
        const unsigned long long w = ((unsigned long long)win[wr * SPITCH + k + 1] << 32) | win[wr * SPITCH + k];
        const unsigned mid = sad4((unsigned)(w >> 8) & m, c, 0u);              // the window's column of the block's column x: x + 1 + v
        const int i = t & 63;
        if (which == 0) part[64 + i] = mid;
        else if (which == 1) part[128 + i] = mid;
        else if (which == 3) part[i] = mid;
        else {
            part[192 + i] = sad4((unsigned)w & m, c, 0u);
            part[256 + i] = sad4((unsigned)(w >> 16) & m, c, 0u);
        }
    }
    __syncthreads();
    for (int s = 32; s > 0; s >>= 1) {                      // thread t: sum t >> 5 (below 5), entry t & 31
        if (t < 160 && (t & 31) < s) part[(t >> 5) * 64 + (t & 31)] += part[(t >> 5) * 64 + (t & 31) + s];
        __syncthreads();
    }
    if (t == 0) {
        const int s0 = (int)part[0];
        out[0] = (signed char)subpel_fit(s0, (int)part[64], (int)part[128], Sp);
        out[1] = (signed char)subpel_fit(s0, (int)part[192], (int)part[256], Sp);
    }
}

__global__ __launch_bounds__(256) void temporal_subpel_kernel(const unsigned char* __restrict__ cur8, const unsigned char* __restrict__ prev8, int Ho,
                                                              int Wo, int R, int hold, int Sp, const signed char* __restrict__ mv,
                                                              signed char* __restrict__ mvf) {
    temporal_subpel_body(cur8, prev8, Ho, Wo, R, hold, Sp, mv, mvf);
}

__global__ __launch_bounds__(256) void temporal_subpel_batch_kernel(const FrameSel S, const FrameBuf C, int Ho, int Wo, int R, int hold, int Sp,
                                                                    const FrameBuf MV, const FrameBuf MVF) {
    const int f = (int)blockIdx.z;
    if (f >= S.frames) return;
    temporal_subpel_body(frame_at(S, C, f), frame_before(S, C, f), Ho, Wo, R, hold, Sp, (const signed char*)frame_at(S, MV, f),
                         (signed char*)frame_at(S, MVF, f));
}

__global__ __launch_bounds__(256) void temporal_subpel_streams_kernel(const StreamSel T, unsigned long long coff, int Ho, int Wo, int R, int hold,
                                                                      int Sp, unsigned long long mvoff, unsigned long long mvfoff) {
    StreamAt at;
    if (!stream_at(T, (int)blockIdx.z, at)) return;         // (before the body's first barrier, the whole workgroup alike)
    temporal_subpel_body(at.wr + coff, at.rd ? at.rd + coff : nullptr, Ho, Wo, R, hold, Sp, (const signed char*)(at.wr + mvoff),
                         (signed char*)(at.wr + mvfoff));
}

struct BlendArgs {
    int Ho, Wo, nby, nbx;
    int strength_q8, sensitivity, R;
};

// the rows, columns and weights of the fetch for a thread's four pixels (y, x0 ... x0 + 3) displaced by (qy, qx) quarter pixels: two rows by
// five columns, every one clamped into the frame; ay and ax are the same for the four pixels (4 x is a multiple of 4)
struct Tap {
    size_t r0, r1;
    int col[5];
    int ay, ax;
};

__device__ __forceinline__ Tap make_tap(const BlendArgs& A, int y, int x0, int qy, int qx) {
    Tap t;
    const int Y4 = 4 * y + qy, X4 = 4 * x0 + qx;
    t.ay = Y4 & 3; t.ax = X4 & 3;
    t.r0 = (size_t)clampi(Y4 >> 2, A.Ho - 1) * A.Wo;
    t.r1 = (size_t)clampi((Y4 >> 2) + 1, A.Ho - 1) * A.Wo;
#pragma unroll
    for (int j = 0; j < 5; ++j) t.col[j] = clampi((X4 >> 2) + j, A.Wo - 1);
    return t;
}

// pixel k of the thread: the previous luma and output at the tap, bilinear; a weight of zero stands before whatever is not fetched.  FRAC
// false: the caller's vectors are whole pixels (ay = ax = 0), nothing but the first position is fetched and no branch stands for it.
template <bool FRAC>
__device__ __forceinline__ void tap_fetch(const Tap& t, int k, const unsigned char* __restrict__ prev8, const unsigned short* __restrict__ prev88, int& pq,
                                          int P[3]) {
    const size_t q00 = t.r0 + t.col[k], q01 = t.r0 + t.col[k + 1], q10 = t.r1 + t.col[k], q11 = t.r1 + t.col[k + 1];
    pq = (int)prev8[q00];
#pragma unroll
    for (int c = 0; c < 3; ++c) P[c] = prev88[q00 * 3 + c];
    if (FRAC && (t.ay | t.ax)) {
        const int wy0 = 4 - t.ay, wx0 = 4 - t.ax;
        int l01 = 0, l10 = 0, l11 = 0, p01[3] = {0, 0, 0}, p10[3] = {0, 0, 0}, p11[3] = {0, 0, 0};
        if (t.ax) {
            l01 = prev8[q01];
#pragma unroll
            for (int c = 0; c < 3; ++c) p01[c] = prev88[q01 * 3 + c];
        }
        if (t.ay) {
            l10 = prev8[q10];
#pragma unroll
            for (int c = 0; c < 3; ++c) p10[c] = prev88[q10 * 3 + c];
            if (t.ax) {
                l11 = prev8[q11];
#pragma unroll
                for (int c = 0; c < 3; ++c) p11[c] = prev88[q11 * 3 + c];
            }
        }
        pq = (wy0 * (wx0 * pq + t.ax * l01) + t.ay * (wx0 * l10 + t.ax * l11) + 8) >> 4;
#pragma unroll
        for (int c = 0; c < 3; ++c) P[c] = (wy0 * (wx0 * P[c] + t.ax * p01[c]) + t.ay * (wx0 * p10[c] + t.ax * p11[c]) + 8) >> 4;   // at most 16 x 65280 + 8
    }
}

// how well the source matched: 256 where the current luma c8 equals the fetched previous luma pq, less `sensitivity` per step apart, at least 0
__device__ __forceinline__ int confidence(int c8, int pq, const BlendArgs& A) {
    const int d = c8 - pq;
    const int conf = 256 - (d < 0 ? -d : d) * A.sensitivity;
    return conf > 0 ? conf : 0;
}

// F += (P - F) w / 2^16, rounded; w = strength_q8 x confidence, 0 ... 65536
__device__ __forceinline__ void step_towards(int F[3], const int P[3], long long w) {
#pragma unroll
    for (int c = 0; c < 3; ++c) F[c] += (int)(((long long)(P[c] - F[c]) * w + 32768) >> 16);
}

__device__ __forceinline__ void blend_towards(int F[3], const int P[3], int c8, int pq, const BlendArgs& A) {
    step_towards(F, P, (long long)A.strength_q8 * confidence(c8, pq, A));
}

// floor(num / den) for num < 2^36 and 0 < den <= 2^19 with a quotient below 2^16: a float estimate (off by less than one) and an exact
// integer fix-up, which is right whatever the estimate was
__device__ __forceinline__ int floor_div(unsigned long long num, unsigned den) {
    long long q = (long long)((float)num / (float)den);
    long long r = (long long)num - q * (long long)den;
    while (r < 0) { --q; r += den; }
    while (r >= (long long)den) { ++q; r -= den; }
    return (int)q;
}

enum BlendMode { BLEND_WHOLE, BLEND_SUB, BLEND_OBMC };

// The blends.  Thread i: row y, pixels x0 ... x0 + 3 as in the luma kernel (they lie in one block).  prev8 == nullptr (no previous frame,
// uniform per launch): F = to88(cur).  dst may be cur: a thread reads its own pixels before it writes them, and no other thread reads them
// (hence no __restrict__ on the two).  prev8 / prev88 are read at displaced positions: they are not cur8 / out88.  mv and mvf are held to
// their bounds and the block indices clamped before any of them reaches an address; nothing else read from a buffer does.
//   BLEND_WHOLE -- along the block's vector mv (mvf is not read); the tap's fractions are zero.
//   BLEND_SUB   -- along 4 mv + mvf quarter pixels, fetched bilinearly: the second row / column only where the fraction along it is not zero.
//   BLEND_OBMC  -- every pixel weighs the vectors of the four blocks whose centres surround it (mvf == nullptr: every fraction is zero).  The
//                  thread's four pixels share their four blocks (the block row changes between rows y = 16 b + 7 and 16 b + 8, the block
//                  column between x = 16 b + 7 and 16 b + 8, a multiple of 4), so the four vectors are read once per thread and only the
//                  column window weight differs per pixel.  A thread whose four held quarter-pixel vectors are equal blends as BLEND_SUB
//                  along that vector: one fetch per pixel, no division (Pbar = P and cbar = conf there).  The others fetch along the four
//                  vectors, sum in 64 bits and divide once per channel.  Waves diverge only along motion edges.
template <BlendMode MODE>
__device__ __forceinline__ void temporal_blend_body(const BlendArgs& A, const float* cur, const unsigned char* __restrict__ cur8,
                                                    const unsigned char* __restrict__ prev8, const unsigned short* __restrict__ prev88,
                                                    const signed char* __restrict__ mv, const signed char* __restrict__ mvf, float* dst,
                                                    unsigned short* __restrict__ out88) {
    const int groups = (A.Wo + 3) >> 2;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)groups * A.Ho) return;
    const int y = (int)(i / groups), x0 = (int)(i - (long long)y * groups) * 4;
    const size_t row = (size_t)y * A.Wo;
    int qy[4] = {0, 0, 0, 0}, qx[4] = {0, 0, 0, 0};         // the held vectors in quarter pixels; BLEND_OBMC: of the candidates (row, column) (0, 0) (0, 1) (1, 0) (1, 1)
    const int ty = 2 * y - 15, tx = 2 * x0 - 15;            // BLEND_OBMC (tx + 2 k for pixel k: the same tx >> 5 for the four)
    const int wy1 = ty & 31;                                // the window weight of the second block row; 32 - wy1 of the first
    bool same = true;
    if (prev8 != nullptr) {
        if (MODE == BLEND_OBMC) {
            const int j0 = ty >> 5, i0 = tx >> 5;
            const int bj[2] = {clampi(j0, A.nby - 1), clampi(j0 + 1, A.nby - 1)}, bi[2] = {clampi(i0, A.nbx - 1), clampi(i0 + 1, A.nbx - 1)};
            const signed char* __restrict__ fr = mvf != nullptr ? mvf : mv;                  // (no fractions: bytes that can be read, masked away below)
            const int fmask = mvf != nullptr ? -1 : 0;      // (uniform per launch)
            int raw[16];                                    // the sixteen loads ahead of their first use, with no branch between them: one wait
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const size_t b = ((size_t)bj[c >> 1] * A.nbx + bi[c & 1]) * 2;
                raw[4 * c] = (int)mv[b]; raw[4 * c + 1] = (int)mv[b + 1]; raw[4 * c + 2] = (int)fr[b]; raw[4 * c + 3] = (int)fr[b + 1];
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) {                   // (written within these bounds; held to them again)
                qy[c] = 4 * hold_to(raw[4 * c], A.R) + (hold_to(raw[4 * c + 2], 2) & fmask);
                qx[c] = 4 * hold_to(raw[4 * c + 1], A.R) + (hold_to(raw[4 * c + 3], 2) & fmask);
                same = same && qy[c] == qy[0] && qx[c] == qx[0];
            }
        } else {
            const size_t b = ((size_t)(y >> 4) * A.nbx + (x0 >> 4)) * 2;
            qy[0] = 4 * hold_to((int)mv[b], A.R);           // (written within these bounds; held to them again)
            qx[0] = 4 * hold_to((int)mv[b + 1], A.R);
            if (MODE == BLEND_SUB) {
                qy[0] += hold_to((int)mvf[b], 2);
                qx[0] += hold_to((int)mvf[b + 1], 2);
            }
        }
    }
    const int n = A.Wo - x0 < 4 ? A.Wo - x0 : 4;
    const size_t at0 = (row + x0) * 3;
    float b[12];                                            // every read of cur before the first write of dst: the two may be one tensor
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int xn = k < n ? k : n - 1;                   // (beyond the row's end: the last pixel again, never stored)
#pragma unroll
        for (int c = 0; c < 3; ++c) b[3 * k + c] = cur[at0 + 3 * xn + c];
    }
    int F[12], c8[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int c = 0; c < 3; ++c) F[3 * k + c] = temporal_f88(b[3 * k + c]);
        c8[k] = prev8 != nullptr ? (int)cur8[row + x0 + (k < n ? k : n - 1)] : 0;
    }
    if (prev8 != nullptr && same) {                         // one vector for the four pixels
        const Tap t = make_tap(A, y, x0, qy[0], qx[0]);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            int pq, P[3];
            tap_fetch<MODE != BLEND_WHOLE>(t, k, prev8, prev88, pq, P);        // (beyond the row's end: whatever lies there, clamped; never stored)
            blend_towards(F + 3 * k, P, c8[k], pq, A);
        }
    } else if (MODE == BLEND_OBMC && prev8 != nullptr) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {                       // pixel by pixel: the sums of one pixel are live at a time
            unsigned D = 0;                                 // at most 2^18
            unsigned long long N[3] = {0, 0, 0};            // below 2^34
            int cmax = 0;
            const int wx1 = (tx + 2 * k) & 31;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const Tap t = make_tap(A, y, x0 + k, qy[c], qx[c]);
                int pq, P[3];
                tap_fetch<true>(t, 0, prev8, prev88, pq, P);                   // (beyond the row's end: whatever lies there, clamped; never stored)
                const int conf = confidence(c8[k], pq, A);
                const unsigned wc = (unsigned)(((c >> 1) ? wy1 : 32 - wy1) * ((c & 1) ? wx1 : 32 - wx1) * conf);
                D += wc;
                cmax = conf > cmax ? conf : cmax;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) N[ch] += (unsigned long long)wc * (unsigned)P[ch];
            }
            if (D == 0) continue;                           // F = B
            const int cbar = cmax < (int)(D >> 8) ? cmax : (int)(D >> 8);
            int Pbar[3];
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) Pbar[ch] = floor_div(2 * N[ch] + D, 2 * D);   // the rounded weighted mean, 0 ... 65280
            step_towards(F + 3 * k, Pbar, (long long)A.strength_q8 * cbar);
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (k < n) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                dst[at0 + 3 * k + c] = (float)F[3 * k + c] * 0.00390625f;
                out88[at0 + 3 * k + c] = (unsigned short)F[3 * k + c];
            }
        }
}

__global__ __launch_bounds__(256) void temporal_blend_kernel(const BlendArgs A, const float* cur, const unsigned char* __restrict__ cur8,
                                                             const unsigned char* __restrict__ prev8, const unsigned short* __restrict__ prev88,
                                                             const signed char* __restrict__ mv, float* dst, unsigned short* __restrict__ out88) {
    temporal_blend_body<BLEND_WHOLE>(A, cur, cur8, prev8, prev88, mv, nullptr, dst, out88);
}

__global__ __launch_bounds__(256) void temporal_blend_sub_kernel(const BlendArgs A, const float* cur, const unsigned char* __restrict__ cur8,
                                                                 const unsigned char* __restrict__ prev8, const unsigned short* __restrict__ prev88,
                                                                 const signed char* __restrict__ mv, const signed char* __restrict__ mvf, float* dst,
                                                                 unsigned short* __restrict__ out88) {
    temporal_blend_body<BLEND_SUB>(A, cur, cur8, prev8, prev88, mv, mvf, dst, out88);
}

__global__ __launch_bounds__(256) void temporal_blend_obmc_kernel(const BlendArgs A, const float* cur, const unsigned char* __restrict__ cur8,
                                                                  const unsigned char* __restrict__ prev8, const unsigned short* __restrict__ prev88,
                                                                  const signed char* __restrict__ mv, const signed char* __restrict__ mvf, float* dst,
                                                                  unsigned short* __restrict__ out88) {
    temporal_blend_body<BLEND_OBMC>(A, cur, cur8, prev8, prev88, mv, mvf, dst, out88);
}

// where the blend's buffers lie in a slot (mvf: ignored where has_mvf is 0)
struct StreamBlend {
    unsigned long long luma, out88, mv, mvf;
    int has_mvf;
};

// stream s blends image s of cur into image s of dst: "no previous frame" is uniform per workgroup here, not per launch
template <BlendMode MODE>
__device__ __forceinline__ void temporal_blend_streams(const BlendArgs& A, const StreamSel& T, const StreamBlend& O, const float* cur, float* dst) {
    const int s = (int)blockIdx.y;
    StreamAt at;
    if (!stream_at(T, s, at)) return;
    const size_t image = (size_t)s * A.Ho * A.Wo * 3;
    temporal_blend_body<MODE>(A, cur + image, at.wr + O.luma, at.rd ? at.rd + O.luma : nullptr,
                              at.rd ? (const unsigned short*)(at.rd + O.out88) : nullptr, (const signed char*)(at.wr + O.mv),
                              O.has_mvf ? (const signed char*)(at.wr + O.mvf) : nullptr, dst + image, (unsigned short*)(at.wr + O.out88));
}

__global__ __launch_bounds__(256) void temporal_blend_streams_kernel(const BlendArgs A, const StreamSel T, const StreamBlend O, const float* cur,
                                                                     float* dst) {
    temporal_blend_streams<BLEND_WHOLE>(A, T, O, cur, dst);
}

__global__ __launch_bounds__(256) void temporal_blend_sub_streams_kernel(const BlendArgs A, const StreamSel T, const StreamBlend O, const float* cur,
                                                                         float* dst) {
    temporal_blend_streams<BLEND_SUB>(A, T, O, cur, dst);
}

__global__ __launch_bounds__(256) void temporal_blend_obmc_streams_kernel(const BlendArgs A, const StreamSel T, const StreamBlend O, const float* cur,
                                                                          float* dst) {
    temporal_blend_streams<BLEND_OBMC>(A, T, O, cur, dst);
}

inline uint64_t up16(uint64_t v) { return (v + 15) & ~(uint64_t)15; }

// the work buffer: frames - 1 slots of [luma | pyr | mv | mvf], then min(frames - 1, 2) out88 frames (a blend reads its predecessor's only)
struct BatchLay {
    uint64_t luma_off, pyr_off, mv_off, mvf_off, slot, o88_off, o88_size, bytes;
};

BatchLay batch_lay(const fs_temporal_pyr_info& lay, int subpel, int frames) {
    BatchLay b;
    const uint64_t blocks = up16((uint64_t)lay.nby[0] * (uint64_t)lay.nbx[0] * 2);
    b.luma_off = 0;
    b.pyr_off = up16((uint64_t)lay.h[0] * (uint64_t)lay.w[0]);
    b.mv_off = b.pyr_off + lay.pyr_bytes;   // (a multiple of 16 already)
    b.mvf_off = b.mv_off + blocks;
    b.slot = b.mvf_off + (subpel > 0 ? blocks : 0);
    b.o88_off = b.slot * (uint64_t)(frames - 1);
    b.o88_size = up16((uint64_t)lay.h[0] * (uint64_t)lay.w[0] * 6);
    b.bytes = b.o88_off + b.o88_size * (uint64_t)(frames - 1 < 2 ? frames - 1 : 2);
    return b;
}

// a slot of a streams call: [luma | out88 | pyr | mv | mvf], every part at a multiple of 16
struct StreamLay {
    uint64_t luma_off, o88_off, pyr_off, mv_off, mvf_off, slot;
};

StreamLay stream_lay(const fs_temporal_pyr_info& lay, int subpel) {
    StreamLay t;
    const uint64_t blocks = up16((uint64_t)lay.nby[0] * (uint64_t)lay.nbx[0] * 2);
    t.luma_off = 0;
    t.o88_off = up16((uint64_t)lay.h[0] * (uint64_t)lay.w[0]);
    t.pyr_off = t.o88_off + up16((uint64_t)lay.h[0] * (uint64_t)lay.w[0] * 6);
    t.mv_off = t.pyr_off + lay.pyr_bytes;   // (a multiple of 16 already)
    t.mvf_off = t.mv_off + blocks;
    t.slot = t.mvf_off + (subpel > 0 ? blocks : 0);
    return t;
}

}  // namespace

// arguments: checked by the caller (fs_api.hip)
int temporal_run(const TemporalCall& c, hipStream_t s) {
    fs_temporal_pyr_info lay;
    if (fs_temporal_pyr_layout(c.Ho, c.Wo, c.levels, &lay)) return -1;                   // (cannot happen: the caller checked all three)
    const int L = c.levels, Ho = c.Ho, Wo = c.Wo, N = c.frames, St = c.streams;         // (St > 0: one frame of each of St streams, N is 1)
    BatchLay B = batch_lay(lay, c.subpel, N);
    const StreamLay TL = stream_lay(lay, c.subpel);
    StreamSel T;
    T.ctl = c.ctl; T.state = c.state; T.slot = TL.slot; T.stream = 2 * TL.slot; T.streams = St;
    if (St > 0) {                                           // (the offsets below are then those in a stream's slot; the pointers beside them are null)
        B.luma_off = TL.luma_off; B.pyr_off = TL.pyr_off; B.mv_off = TL.mv_off; B.mvf_off = TL.mvf_off;
    }
    FrameSel S;
    S.work = c.work; S.slot = B.slot; S.frames = N;
    const FrameBuf FMV = {(unsigned char*)c.mv, nullptr, B.mv_off}, FMVF = {(unsigned char*)c.mvf, nullptr, B.mvf_off};
    FrameBuf FPL[FS_TEMPORAL_MAX_LEVELS], FPV[FS_TEMPORAL_MAX_LEVELS];                    // the levels' lumas and vectors
    FPL[0] = {c.luma, c.prev_luma, B.luma_off}; FPV[0] = FMV;
    for (int l = 1; l < L; ++l) {
        FPL[l] = {St > 0 ? nullptr : c.pyr + lay.luma_offset[l], c.prev_luma == nullptr ? nullptr : c.prev_pyr + lay.luma_offset[l],
                  B.pyr_off + lay.luma_offset[l]};
        FPV[l] = {St > 0 ? nullptr : c.pyr + lay.mv_offset[l], nullptr, B.pyr_off + lay.mv_offset[l]};
    }
    const int kr = c.matrix ? 13933 : 19595, kg = c.matrix ? 46871 : 38470, kb = c.matrix ? 4732 : 7471;  // each triple sums to 65536
    LumaArgs LA;
    LA.H = c.H; LA.W = c.W; LA.Ho = Ho; LA.Wo = Wo;
    LA.k0 = c.src_bgr ? kb : kr; LA.k1 = kg; LA.k2 = c.src_bgr ? kr : kb;
    const long long threads = ((long long)(Wo + 3) >> 2) * Ho;
    const dim3 egrid((unsigned)((threads + 255) / 256)), block(256);
    if (St > 0)                                             // (streams: the entries that select by ctl[s], here and below)
        hipLaunchKernelGGL(temporal_luma_streams_kernel, dim3(egrid.x, (unsigned)St), block, 0, s, LA, T, FPL[0].off, c.src);
    else if (N == 1)                                        // (one frame: the entries without a frame index, here and below)
        hipLaunchKernelGGL(temporal_luma_kernel, egrid, block, 0, s, LA, c.src, c.luma);
    else
        hipLaunchKernelGGL(temporal_luma_batch_kernel, dim3(egrid.x, (unsigned)N), block, 0, s, LA, S, FPL[0], c.src);
    if (L > 1) {
        PyrArgs PA;
        PA.H0 = Ho; PA.W0 = Wo; PA.H1 = lay.h[1]; PA.W1 = lay.w[1];
        PA.H2 = L > 2 ? lay.h[2] : 0; PA.W2 = L > 2 ? lay.w[2] : 0;
        const unsigned chunks = (unsigned)((((PA.W1 + 3) >> 2) + 255) / 256);            // (W1 >= W2; at most 2^21 columns: within grid.y)
        if (St > 0)
            hipLaunchKernelGGL(temporal_pyramid_streams_kernel, dim3((unsigned)(PA.H1 + PA.H2), chunks, (unsigned)St), block, 0, s, PA, T, FPL[0].off,
                               FPL[1].off, L > 2 ? FPL[2].off : FPL[1].off);
        else if (N == 1)
            hipLaunchKernelGGL(temporal_pyramid_kernel, dim3((unsigned)(PA.H1 + PA.H2), chunks), block, 0, s, PA, (const unsigned char*)c.luma, FPL[1].last,
                               L > 2 ? FPL[2].last : nullptr);
        else
            hipLaunchKernelGGL(temporal_pyramid_batch_kernel, dim3((unsigned)(PA.H1 + PA.H2), chunks, (unsigned)N), block, 0, s, PA, S, FPL[0], FPL[1],
                               L > 2 ? FPL[2] : FPL[1]);
    }
    for (int l = L - 1; l >= 0; --l) {                      // coarsest first: level l reads the vectors level l + 1 wrote
        const bool top = l == L - 1;
        const int pnbx = top ? 0 : lay.nbx[l + 1], lhold = 2 * c.radius * ((1 << (L - 1 - l)) - 1);
        if (St > 0)
            hipLaunchKernelGGL(temporal_search_streams_kernel, dim3((unsigned)lay.nbx[l], (unsigned)lay.nby[l], (unsigned)St), block, 0, s, T, FPL[l].off,
                               lay.h[l], lay.w[l], c.radius, top ? FPV[l].off : FPV[l + 1].off, top ? 0 : 1, pnbx, lhold, FPV[l].off);
        else if (N == 1)
            hipLaunchKernelGGL(temporal_search_kernel, dim3((unsigned)lay.nbx[l], (unsigned)lay.nby[l]), block, 0, s, (const unsigned char*)FPL[l].last,
                               FPL[l].before, lay.h[l], lay.w[l], c.radius, top ? nullptr : (const signed char*)FPV[l + 1].last, pnbx, lhold,
                               (signed char*)FPV[l].last);
        else
            hipLaunchKernelGGL(temporal_search_batch_kernel, dim3((unsigned)lay.nbx[l], (unsigned)lay.nby[l], (unsigned)N), block, 0, s, S, FPL[l], lay.h[l],
                               lay.w[l], c.radius, top ? FPV[l] : FPV[l + 1], top ? 0 : 1, pnbx, lhold, FPV[l]);
    }
    const int hold = c.radius * ((1 << L) - 1);
    if (c.subpel > 0 && St > 0)
        hipLaunchKernelGGL(temporal_subpel_streams_kernel, dim3((unsigned)lay.nbx[0], (unsigned)lay.nby[0], (unsigned)St), block, 0, s, T, FPL[0].off, Ho,
                           Wo, c.radius, hold, c.subpel, FMV.off, FMVF.off);
    else if (c.subpel > 0 && N == 1)
        hipLaunchKernelGGL(temporal_subpel_kernel, dim3((unsigned)lay.nbx[0], (unsigned)lay.nby[0]), block, 0, s, (const unsigned char*)c.luma, c.prev_luma,
                           Ho, Wo, c.radius, hold, c.subpel, (const signed char*)c.mv, c.mvf);
    else if (c.subpel > 0)
        hipLaunchKernelGGL(temporal_subpel_batch_kernel, dim3((unsigned)lay.nbx[0], (unsigned)lay.nby[0], (unsigned)N), block, 0, s, S, FPL[0], Ho, Wo,
                           c.radius, hold, c.subpel, FMV, FMVF);
    BlendArgs BA;
    BA.Ho = Ho; BA.Wo = Wo; BA.nby = lay.nby[0]; BA.nbx = lay.nbx[0];
    BA.strength_q8 = c.strength_q8; BA.sensitivity = c.sensitivity; BA.R = hold;
    const size_t image = (size_t)Ho * Wo * 3;
    if (St > 0) {                                           // nothing recursive inside the pass: one blend over all streams
        const StreamBlend O = {TL.luma_off, TL.o88_off, TL.mv_off, TL.mvf_off, c.subpel > 0 ? 1 : 0};
        const dim3 sgrid(egrid.x, (unsigned)St);
        if (c.overlap)
            hipLaunchKernelGGL(temporal_blend_obmc_streams_kernel, sgrid, block, 0, s, BA, T, O, c.cur, c.dst);
        else if (c.subpel > 0)
            hipLaunchKernelGGL(temporal_blend_sub_streams_kernel, sgrid, block, 0, s, BA, T, O, c.cur, c.dst);
        else
            hipLaunchKernelGGL(temporal_blend_streams_kernel, sgrid, block, 0, s, BA, T, O, c.cur, c.dst);
    }
    for (int i = 0; St == 0 && i < N; ++i) {                // in order: frame i reads the out88 frame i - 1 wrote (the two in `work` alternate)
        const bool last = i == N - 1;                       // (i == 0 and the last frame take state pointers only: `work` may be null with one frame)
        const unsigned char* c8 = last ? c.luma : c.work + (size_t)i * B.slot + B.luma_off;
        const unsigned char* p8 = i == 0 ? c.prev_luma : c.work + (size_t)(i - 1) * B.slot + B.luma_off;
        const unsigned short* p88 = i == 0 ? c.prev_out88 : (const unsigned short*)(c.work + B.o88_off + (size_t)((i - 1) & 1) * B.o88_size);
        unsigned short* o88 = last ? c.out88 : (unsigned short*)(c.work + B.o88_off + (size_t)(i & 1) * B.o88_size);
        const signed char* v = (const signed char*)(last ? (unsigned char*)c.mv : c.work + (size_t)i * B.slot + B.mv_off);
        const signed char* vf = c.subpel > 0 ? (const signed char*)(last ? (unsigned char*)c.mvf : c.work + (size_t)i * B.slot + B.mvf_off) : nullptr;
        if (c.overlap)
            hipLaunchKernelGGL(temporal_blend_obmc_kernel, egrid, block, 0, s, BA, c.cur + i * image, c8, p8, p88, v, vf, c.dst + i * image, o88);
        else if (c.subpel > 0)
            hipLaunchKernelGGL(temporal_blend_sub_kernel, egrid, block, 0, s, BA, c.cur + i * image, c8, p8, p88, v, vf, c.dst + i * image, o88);
        else
            hipLaunchKernelGGL(temporal_blend_kernel, egrid, block, 0, s, BA, c.cur + i * image, c8, p8, p88, v, c.dst + i * image, o88);
    }
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace fs

extern "C" {

int fs_temporal_batch_layout(int Ho, int Wo, int levels, int subpel, int frames, fs_temporal_batch_info* info) {
    using namespace fs;
    if (!info) return set_error(-1, "fs_temporal_batch_layout: null argument");
    if (Ho < 1 || Wo < 1) return set_error(-1, "fs_temporal_batch_layout: a %dx%d output has a side below 1", Ho, Wo);
    if (frames < 1 || frames > 64) return set_error(-1, "fs_temporal_batch_layout: frames must be in [1, 64], got %d", frames);
    if (levels < 1 || levels > FS_TEMPORAL_MAX_LEVELS)
        return set_error(-2, "fs_temporal_batch_layout: levels must be in [1, %d], got %d", FS_TEMPORAL_MAX_LEVELS, levels);
    if (subpel < 0 || subpel > 2) return set_error(-2, "fs_temporal_batch_layout: subpel must be 0 (whole), 1 (half) or 2 (quarter pixels), got %d", subpel);
    fs_temporal_pyr_info lay;
    if (fs_temporal_pyr_layout(Ho, Wo, levels, &lay)) return -1;                    // (cannot happen: checked above)
    const BatchLay B = batch_lay(lay, subpel, frames);
    fs_temporal_batch_info b;
    memset(&b, 0, sizeof(b));
    b.frames = frames; b.levels = levels; b.subpel = subpel;
    if (frames > 1) {
        b.mv_offset = B.mv_off; b.mv_stride = B.slot;
        if (subpel > 0) { b.mvf_offset = B.mvf_off; b.mvf_stride = B.slot; }
        b.work_bytes = B.bytes;
    }
    *info = b;
    return 0;
}

int fs_temporal_streams_layout(int Ho, int Wo, int levels, int subpel, int streams, fs_temporal_streams_info* info) {
    using namespace fs;
    if (!info) return set_error(-1, "fs_temporal_streams_layout: null argument");
    if (Ho < 1 || Wo < 1) return set_error(-1, "fs_temporal_streams_layout: a %dx%d output has a side below 1", Ho, Wo);
    if (streams < 1 || streams > 64) return set_error(-1, "fs_temporal_streams_layout: streams must be in [1, 64], got %d", streams);
    if (levels < 1 || levels > FS_TEMPORAL_MAX_LEVELS)
        return set_error(-2, "fs_temporal_streams_layout: levels must be in [1, %d], got %d", FS_TEMPORAL_MAX_LEVELS, levels);
    if (subpel < 0 || subpel > 2) return set_error(-2, "fs_temporal_streams_layout: subpel must be 0 (whole), 1 (half) or 2 (quarter pixels), got %d", subpel);
    fs_temporal_pyr_info lay;
    if (fs_temporal_pyr_layout(Ho, Wo, levels, &lay)) return -1;                    // (cannot happen: checked above)
    const StreamLay TL = stream_lay(lay, subpel);
    fs_temporal_streams_info t;
    memset(&t, 0, sizeof(t));
    t.streams = streams; t.levels = levels; t.subpel = subpel;
    t.luma_offset = TL.luma_off; t.out88_offset = TL.o88_off; t.pyr_offset = TL.pyr_off; t.mv_offset = TL.mv_off; t.mvf_offset = TL.mvf_off;
    t.slot_stride = TL.slot; t.stream_stride = 2 * TL.slot;
    t.state_bytes = (uint64_t)streams * t.stream_stride;
    *info = t;
    return 0;
}

int fs_temporal_pyr_layout(int Ho, int Wo, int levels, fs_temporal_pyr_info* info) {
    using namespace fs;
    if (!info) return set_error(-1, "fs_temporal_pyr_layout: null argument");
    if (Ho < 1 || Wo < 1) return set_error(-1, "fs_temporal_pyr_layout: a %dx%d output has a side below 1", Ho, Wo);
    if (levels < 1 || levels > FS_TEMPORAL_MAX_LEVELS)
        return set_error(-2, "fs_temporal_pyr_layout: levels must be in [1, %d], got %d", FS_TEMPORAL_MAX_LEVELS, levels);
    fs_temporal_pyr_info p;
    memset(&p, 0, sizeof(p));
    p.levels = levels;
    for (int l = 0; l < levels; ++l) {
        p.h[l] = l ? (p.h[l - 1] + 1) / 2 : Ho;
        p.w[l] = l ? (p.w[l - 1] + 1) / 2 : Wo;
        p.nby[l] = (p.h[l] + TB - 1) / TB;
        p.nbx[l] = (p.w[l] + TB - 1) / TB;
    }
    uint64_t at = 0;
    for (int l = 1; l < levels; ++l) {
        p.luma_offset[l] = at;
        at += ((uint64_t)p.h[l] * (uint64_t)p.w[l] + 15) & ~(uint64_t)15;
    }
    for (int l = 1; l < levels; ++l) {
        p.mv_offset[l] = at;
        at += ((uint64_t)p.nby[l] * (uint64_t)p.nbx[l] * 2 + 15) & ~(uint64_t)15;
    }
    p.pyr_bytes = at;
    *info = p;
    return 0;
}

}  // extern "C"
