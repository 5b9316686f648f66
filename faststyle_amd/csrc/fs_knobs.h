// The tuning / debugging knobs of the library: ONE row per knob -- X(id, default, meaning); the environment variable is FS_<id>.
// None is needed in production.  DESIGN.md 10a lists the same rows (tests/test_knobs.py holds the two together through
// fs_debug_knob); a default is written here and nowhere else.
//
// fs::knob(K_<id>) reads a knob: its slot is filled from the environment (strtol, base 0; absent: the default) at the first
// lookup after start or after fs_debug_reload_env(), so no launch or planning path reads the environment afterwards and a value only
// changes together with tune_epoch().  (fs_api.hip holds the slots and the only environment read of the library.)
#pragma once

namespace fs {

#define FS_KNOBS(X)                                                                                                                      \
    /* Winograd generations, the F(2x2) kernels */                                                                                       \
    X(CONV_WINO, 1, "0: every 3x3 conv through the direct kernels (no Winograd family is planned)")                                      \
    X(WINO_V, 6, "newest Winograd generation in use: 1 fs_wino, 2 + fs_wino2 / fs_wino2h, 4 + fs_wino4, 5 + fs_wino4t, 6 + fs_wino6")    \
    X(WINO2_MAXCIN, 128, "largest Cin the second-generation F(2x2) kernel takes (the first-generation one beyond)")                      \
    X(WINO2_WGS, 256, "persistent grid of the second-generation F(2x2) kernels (full and half items)")                                   \
    X(WINO2_REM, 1, "0: no remainder split in the transform net's F(2x2) launches")                                                      \
    X(WINO_KSPLIT, 4, "cap of the split-K factor of every Winograd kernel")                                                              \
    X(TNET_WINO, 1, "transform-net residual convs through a Winograd kernel: 0 never, 1 where the items fill the chip (>= 200), 2 always") \
    X(TNET_WINO_HALF, 1, "0: no half-item F(2x2) kernel (fs_wino2h) for the residual convs on small grids")                              \
    X(WINO2H_MIN_ITEMS, 96, "smallest launch (half items) that takes the half-item kernel")                                              \
    X(WINO2H_SHAPE, -1, "0..3 pins the half-item block shape (4x8, 5x6, 6x5, 8x4 tiles); -1: the planner's pick")                        \
    X(VGG_WINO_MASK, -1, "per VGG16 layer: bit l the forward, bit 16+l the input gradient through a Winograd kernel")                    \
    X(VGG_PREPARE_ALL, 0, "1: fs_vgg_prepare builds the filter layouts of every generation, not only those FS_WINO_V selects")           \
    /* fp32 F(4x4): fs_wino4t (filter in registers), fs_wino4 (filter through LDS) */                                                    \
    X(TNET_WINO4, 1, "residual convs through the 16-tile F(4x4) kernel: 0 never, 1 from FS_WINO4T_MIN_ITEMS items, 2 always")            \
    X(WINO4T_MIN_ITEMS, 64, "smallest residual launch (items of 16x16 pixels) that takes the 16-tile F(4x4) kernel")                     \
    X(WINO4T_WGS, 256, "persistent grid of fs_wino4t")                                                                                   \
    X(WINO4T_TB, 0, "1 / 2 pins the tile blocks per item of fs_wino4t; 0: the planner's pick")                                           \
    X(WINO4T_CB, 2, "1: no 128-channel item form in fs_wino4t")                                                                          \
    X(WINO4T_FLAT, 1, "flattened 16-tile items in the transform net's plans: 0 never, 1 when a round of the grid is saved, 2 always")    \
    X(WINO4_WGS, 256, "persistent grid of fs_wino4")                                                                                     \
    X(WINO4_STAGGER, 0, "start stagger of fs_wino4's workgroups (DESIGN.md 10)")                                                         \
    X(WINO4_KSPLIT_MINSTEPS, 16, "fewest channel chunks a split-K part of an F(4x4) launch may get")                                     \
    /* split-bf16 F(4x4) pipeline: fs_wino6 */                                                                                           \
    X(WINO6_MINCC, 512 * 256, "smallest Cin * Cout the split-bf16 Winograd pipeline takes")                                              \
    X(WINO6_MINTILES, 256, "smallest launch (tiles of 4x4 outputs) it takes")                                                            \
    X(WINO6_CHAIN_MINTILES, 1024, "smallest half batch (tiles) that runs as one of two overlapped chains")                               \
    X(WINO6_OVERLAP, 1, "VGG16 under fs_wino6: 0 one chain, 1 two half-batch chains on two streams, 2 two chunks per launch")            \
    X(WINO6_PIPE, 1, "0: no software pipeline of a launch's two chunks over the side stream")                                            \
    X(WINO6_CHUNK, 0, "tiles per pass (multiples of 128); 0: what the workspace holds")                                                  \
    X(WINO6_WS_MB, 2048, "cap of the pipeline's scratch in MiB")                                                                         \
    X(WINO6_WAVES, 4, "waves per workgroup of its GEMM kernel: 4 or 8")                                                                  \
    /* split-bf16 direct kernels */                                                                                                      \
    X(S16_SPLIT, 1, "0: the 16-channel layers on fp32 matrix instructions instead of six exact bf16-piece products")                     \
    X(CSTREAM_SPLIT, 1, "0: the narrow-layer instances of conv_stream_kernel likewise on fp32 matrix instructions")                      \
    X(GRAM_SPLIT, 1, "0: the 128-channel Gram tiles likewise on fp32 matrix instructions")                                               \
    X(TNET_RES_X6, 1, "forward residual convs through the direct split-bf16 kernel: 0 never, 1 below FS_TNET_RES_X6_MAX_ITEMS, 2 wherever eligible") \
    X(TNET_RES_X6_MAX_ITEMS, 129, "Winograd items (16x16 pixels) below which the forward residual convs take that kernel")               \
    X(R64X_PIPE, 1, "0: the residual split-bf16 kernel without the next tile's staging threaded into its sweep")                         \
    X(CSTREAM_R64X_ALL, 0, "1: fs_conv2d_fwd may reach the residual split-bf16 kernel (micro-benchmarks)")                               \
    /* streams */                                                                                                                        \
    X(NO_SIDE_STREAM, 0, "1: a context creates no second stream (no filter-gradient branch, no overlapped chains)")                      \
    X(SIDE_MIN_PIXELS, 1000000, "smallest N * H * W whose fs_tnet_backward forks the filter gradients onto the second stream")           \
    X(FEED_DEPTH, 2, "train.py: device batches the input path keeps in its ring, produced ahead of the step on a stream of its own; 0: the synchronous path") \
    X(FEED_JPEG, 0, "train.py: 1: baseline JPEGs are decoded by the library on the device-fed path (fs_jpeg.hip: Huffman pass on the decode threads, reconstruction on the GPU); 0: PIL") \
    /* instance norm */                                                                                                                  \
    X(INBWD_REC, 1, "0: instance-norm backward in its three-launch form everywhere")                                                     \
    X(INBWD_FUSED, 1, "0: no partial-sum records from the residual input-gradient epilogues (a pass of its own instead)")                \
    X(INBWD_REC_MAXT, 192, "records per sample of that partial-sum pass")                                                                \
    X(INBWD_APPLY_WGS, 1024, "persistent grid of the instance-norm-backward apply kernel")                                               \
    X(INBWD_PUNR, 8, "its 16-byte loads in flight per thread (8: sixteen, less: eight)")                                                 \
    X(INBWD_CHUNK, 0, "pixels per partial-sum block of the three-launch form (multiples of 64); 0: planned")                             \
    X(FUSED_FINALIZE, 0, "1: instance-norm finalize inside the producing conv kernel (measured slower, DESIGN.md 10)")                   \
    X(FUSED_FINALIZE_MAX, 24576, "largest N * C * tiles * groups record count that the fused finalize takes")                            \
    X(FINALIZE_MIN_T, 16 * kFinalizeSplit, "tile records per sample above which in_finalize pre-reduces in a launch of its own")         \
    /* launch collapses of round 5 */                                                                                                    \
    X(GRAM_FINISH_BATCH, 1, "0: a reduce + squared-difference launch per style layer")                                                   \
    X(GRAM_FINISH_KEEP_G, 0, "1: the training step also writes the Gram matrices")                                                       \
    X(WGRAD_DEFER, 1, "0: a slab reduction per filter-gradient launch")                                                                  \
    X(TNET_BWD_FILTERS_IN_FWD, 1, "0: the backward's filter re-layouts in launches of its own")                                          \
    /* filter gradients */                                                                                                               \
    X(WGW, 1, "0: residual filter gradients through wgrad2_kernel instead of the Winograd kernel (fs_wgw)")                              \
    X(WGW_WGS, 256, "persistent grid of fs_wgw")                                                                                         \
    X(WGW_MIN_STEPS, 64, "smallest problem (16-tile steps) that takes fs_wgw")                                                           \
    X(WGRAD2, 1, "0: filter gradients through the round-1 kernel")                                                                       \
    X(WGRAD2_WGS, 256, "persistent grid of wgrad2_kernel, also its planner's tile-size target")                                          \
    X(WGRAD2_STATIC, 1, "0: any-geometry instances of wgrad2_kernel only")                                                               \
    X(WGRAD2_COMBINE, 1, "0: one partial slab per pixel-row group")                                                                      \
    X(WGRAD2_DEBUG, 0, "timing ablations, results wrong: 1 no sweeps, 2 only the first tile is staged")                                  \
    X(TNET_WGRAD_BATCH, 1, "0: one launch per residual filter gradient")                                                                 \
    X(WGRAD_WGS, 512, "round-1 filter-gradient kernel: workgroups aimed at")                                                             \
    X(WGRAD_MAXPX, 256, "... largest pixel tile its planner starts from")                                                                \
    X(WGRAD_BALANCE, 1, "... 0: no smaller tile to balance the grid")                                                                    \
    /* narrow layers */                                                                                                                  \
    X(S16, 1, "0: 16-output-channel layers and VGG conv1_1 through conv_igemm_kernel")                                                   \
    X(S16_VGG, 1, "0: only VGG conv1_1 back to conv_igemm_kernel")                                                                       \
    X(S16_MIN_TILES, 64, "smallest launch that takes conv_s16_kernel")                                                                   \
    X(S16_WGS, 512, "persistent grid of conv_s16_kernel")                                                                                \
    X(CSTREAM, 1, "0: narrow layers through conv_igemm_kernel")                                                                          \
    X(CSTREAM_MASK, 15, "conv_stream_kernel instances in use (bit i = instance i+1; bit 4, the 64->64 3x3 one, is off)")                 \
    X(CSTREAM_MIN_TILES, 64, "smallest launch that takes conv_stream_kernel")                                                            \
    X(CSTREAM_WGS, 256, "persistent grid of conv_stream_kernel")                                                                         \
    /* VGG16 and Gram fusions */                                                                                                         \
    X(VGG_POOL_FUSED, 1, "0: max-pool as a pass of its own")                                                                             \
    X(VGG_SKIP_CONTENT_Y, 1, "0: the content half's full-resolution conv1_2 / conv2_2 outputs are stored")                               \
    X(VGG_ROUTE_FUSED, 0, "1: pool-gradient routing inside the Gram-gradient conv")                                                      \
    X(GRAM_SAME, 1, "0: two-operand Gram staging")                                                                                       \
    X(C3_VALU, 1, "0: conv1_1 input gradient on the matrix cores")                                                                       \
    X(GRAM2, 1, "0: Gram matrices through the round-1 kernel")                                                                           \
    X(GRAM2_ITEMS, 768, "workgroups a Gram launch aims at")                                                                              \
    X(GRAM2_MIN_TILES, 4, "fewest pixel tiles a range of a Gram launch keeps")                                                           \
    X(GRAM_BWD2, 1, "0: Gram gradient through the round-1 kernel")                                                                       \
    X(GRAM_BWD2_WGS, 256, "persistent grid of the Gram-gradient kernel")                                                                 \
    X(GRAM_ROUTE_FUSED, 1, "0: the three-launch form of the pooled style layers' gradient")                                              \
    X(GRAM_CONTENT_FUSED, 1, "0: the content term from the squared-difference pass")                                                     \
    /* bf16 inference */                                                                                                                 \
    X(BSTREAM, 1, "0: bf16 inference through the round-2 kernels of fs_bf16.hip")                                                        \
    X(BSTREAM_MASK, 127, "bstream instances in use (bit i = instance i+1: initconv_1 .. image layer)")                                   \
    X(BSTREAM_WGS, 512, "persistent grid of the 32-wide bstream instances")                                                              \
    X(BSTREAM_WGS64, 256, "persistent grid of the 64-wide ones")                                                                         \
    X(BF16_WM, 0, "1: caps the pixel tile of the round-2 bf16 kernels at 128")                                                           \
    X(BF16_GRID, 2048, "their persistent grid")                                                                                          \
    /* direct-conv plan overrides */                                                                                                     \
    X(CONV_VARIANT, -1, "pins the tile variant; -1: planned")                                                                            \
    X(CONV_MIN_WGS, 512, "grid size below which a smaller tile or split-K is tried")                                                     \
    X(CONV_KSPLIT, 4, "cap of the split-K factor")                                                                                       \
    X(CONV_FORCE_KSPLIT, 0, "test hook: this split-K factor whatever the grid size")                                                     \
    X(CONV_KSPLIT_FILL, 4, "no split-K once the plain grid exceeds FS_CONV_MIN_WGS / this")                                              \
    X(CONV_CC, 0, "pins the channel chunk; 0: planned")                                                                                  \
    X(CONV_LDS_KB, 36, "LDS budget per pipeline stage, KiB")                                                                             \
    X(CONV_XCD, 1, "0: no XCD-aware workgroup map")                                                                                      \
    X(CONV_SKEW, 0, "launch stagger")                                                                                                    \
    X(CONV_DEBUG, 0, "1: one stderr line per conv launch with the chosen plan")

enum Knob : int {
#define FS_KNOB_ENUM(id, dflt, doc) K_##id,
    FS_KNOBS(FS_KNOB_ENUM)
#undef FS_KNOB_ENUM
    K_COUNT
};
#define FS_KNOB_NAME(id) "FS_" #id

int knob(Knob k);
void tune_reload();      // fs_debug_reload_env: drops every slot
unsigned tune_epoch();   // bumped by tune_reload: cached plans made under older knob values are stale

}  // namespace fs
