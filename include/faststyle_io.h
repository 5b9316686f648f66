/* faststyle_io.h -- C ABI of the training-data input path and of the frame tools' image input / output.
 *
 * Replaces, for the reference's train.py input pipeline:
 *   datapipe.py:38-49   tf.TFRecordReader().read + tf.parse_single_example   -> fs_tfrecord_scan, fs_example_bytes/_int64
 *   datapipe.py:24      tf.image.resize_images(image, size, method=2)          -> fs_resize_bicubic_u8 (device kernel)
 *   tfrecords_writer.py:217-239  tf.python_io.TFRecordWriter.write             -> fs_tfrecord_frame
 * JPEG decoding: by default libjpeg through PIL on several host threads, the decoded u8 pixels uploaded (a quarter of the fp32
 * bytes over PCIe) and resized by the TF1 bicubic kernel straight into the HBM-resident shuffle buffer.  On the device-fed path the
 * library can decode baseline JPEGs itself (FS_FEED_JPEG=1, the fs_jpeg_* calls below): only the serial part, marker parsing and Huffman
 * decoding, stays on the host threads (fs_jpeg_parse / fs_jpeg_decode, no Python work around it); the int16 coefficients cross PCIe and
 * dequantisation, inverse DCT, chroma upsampling and colour conversion run on the GPU (fs_jpeg_reconstruct_many), bit-identical to PIL's
 * decode of the same bytes.  A JPEG outside the handled set is PIL's, as before.
 * The way out mirrors it (the fs_jpeg_forward_many / fs_jpeg_write calls at the end): a u8 frame on the device becomes quantised coefficients
 * there, and host threads Huffman-code them into the baseline file PIL would write for the same pixels.
 *
 * The host-side functions are pure C (no HIP calls) and work without a GPU.  All return 0 / a
 * non-negative count on success and a negative code on error (fs_last_error() has the text).
 */
#ifndef FASTSTYLE_IO_H
#define FASTSTYLE_IO_H
#include <stddef.h>
#include <stdint.h>

#include "faststyle_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* CRC-32C (Castagnoli) and TensorFlow's masked form ((crc >> 15 | crc << 17) + 0xa282ead8), the
 * checksum of TFRecord framing (tensorflow/core/lib/io/record_writer.cc) and of bundle checkpoints. */
uint32_t fs_crc32c(const void* data, size_t n);
uint32_t fs_crc32c_masked(const void* data, size_t n);

/* Walks the records of one TFRecord file image held in memory: each record is
 * {uint64 length, uint32 masked_crc(length), payload, uint32 masked_crc(payload)} (little endian).
 * Writes the payload offsets/lengths of the first `cap` records and returns the TOTAL number of
 * records (call with cap = 0 to count).  verify_crc != 0 checks both checksums of every record.
 * Errors: -1 truncated file, -2 length checksum mismatch, -3 payload checksum mismatch. */
long long fs_tfrecord_scan(const void* buf, size_t n, int verify_crc, uint64_t* payload_off, uint64_t* payload_len,
                           size_t cap);

/* Frames one payload for writing: out must hold n + 16 bytes; returns n + 16. */
size_t fs_tfrecord_frame(const void* payload, size_t n, void* out);

/* tf.parse_single_example restricted to what datapipe.py:40-46 asks for: looks `key` up in a
 * serialized tf.train.Example.  _bytes: offset/length (within ex) of bytes_list.value[0];
 * _int64: int64_list.value[0] (packed or unpacked encoding).
 * Errors: -1 malformed proto, -2 key absent, -3 feature has another kind / is empty. */
int fs_example_bytes(const void* ex, size_t n, const char* key, uint64_t* off, uint64_t* len);
int fs_example_int64(const void* ex, size_t n, const char* key, long long* value);

/* tf.image.resize_images(method=2) of TF 1.0 = ResizeBicubic, align_corners=False, legacy (no
 * half-pixel) coordinates, Keys a = -0.75 through TF's 1024-entry coefficient table, borders clamped,
 * result NOT clipped to [0,255] (tensorflow/core/kernels/resize_bicubic_op.cc @ r1.0).
 * src: device u8 [H,W,3]; dst: device f32 [Ho,Wo,3].  Asynchronous on the ctx stream. */
int fs_resize_bicubic_u8(fs_ctx* ctx, const unsigned char* src, int H, int W, float* dst, int Ho, int Wo);
/* The same with pixel_bytes bytes per source pixel: 3 = packed RGB (what fs_resize_bicubic_u8 takes), 4 = RGBX -- the storage a JPEG decoder
 * such as PIL's keeps an RGB image in, handed over without a host-side repack (faststyle_amd/datapipe.py exports it zero-copy through the Arrow C
 * data interface; the repack was the largest interpreter-locked piece of a decode thread's work).  The fourth byte is never read; the result is
 * bit-identical to the packed form's.  Error -2: another pixel size. */
int fs_resize_bicubic_u8x(fs_ctx* ctx, const unsigned char* src, int H, int W, int pixel_bytes, float* dst, int Ho, int Wo);

/* Frame streaming (stylize_webcam.py:88-95): u8 frame -> float net input (channel order untouched), and
 * net output -> u8 by truncation (numpy .astype(np.uint8)) with an optional R<->B swap
 * (cv2.cvtColor(..., COLOR_BGR2RGB)).  src of _u8_to_f32: 4-byte aligned; dst: 16-byte aligned. */
int fs_u8_to_f32(fs_ctx* ctx, const unsigned char* src, size_t n, float* dst);
int fs_f32_to_u8(fs_ctx* ctx, const float* src, size_t npix, int swap_rb, unsigned char* dst);

/* ---- Device-fed training input path (csrc/fs_feed.hip; faststyle_amd/datapipe.py runs these on a side stream, ahead of the step).
 * All three are asynchronous on the ctx stream, allocate nothing and can be captured into a hipGraph. */

/* One image of fs_resize_bicubic_u8x_many: H x W pixels of pixel_bytes (3 = RGB, 4 = RGBX) bytes each, starting src_offset bytes into the
 * staged buffer, resized into row dst_row of the destination store.  24 bytes, 8-byte aligned. */
typedef struct fs_resize_item {
    uint64_t src_offset;
    int32_t H, W;
    int32_t pixel_bytes;
    int32_t dst_row;
} fs_resize_item;

/* K fs_resize_bicubic_u8x calls in ONE launch: image k of the staged device buffer `base` (base_bytes long) goes to store[dst_row[k]] of the
 * device store [capacity,Ho,Wo,3] float32, bit-identical to the single-image call.  The descriptor table is passed twice: items_host is read
 * by this call (checks, nothing else -- it may be freed on return), items_dev is the copy the kernel reads (the same pointer where host memory
 * is device-visible).  Errors: -1 null argument / K <= 0 / bad shape / an image outside base_bytes, -2 a pixel_bytes other than 3 or 4,
 * -4 a dst_row outside [0, capacity), -5 items_dev not 8-byte aligned. */
int fs_resize_bicubic_u8x_many(fs_ctx* ctx, const unsigned char* base, size_t base_bytes, const fs_resize_item* items_host,
                               const fs_resize_item* items_dev, int K, float* store, int capacity, int Ho, int Wo);

/* tf.RandomShuffleQueue.dequeue_many on the device store [capacity, row_floats] in ONE launch:
 *   batch_out[i] = store[take_idx[i]]  (i < B)   and   store[move_dst[j]] = store[move_src[j]]  (j < M, 0 <= M <= B).
 * take_idx, move_src, move_dst: device int32 tables.  The caller resolves the swap-remove: the move_dst rows are the holes (taken rows) below
 * the new size, every move_src row lies at or above it, is not taken and is nobody's destination.  A hole is gathered before it is
 * back-filled (by the same workgroup); an index outside [0, capacity) moves nothing.  row_floats: a multiple of 4; store and batch_out
 * 16-byte aligned.  Errors: -1 null argument / B < 1 / M outside [0, B] / capacity < 1, -2 row_floats not a positive multiple of 4,
 * -5 a misaligned pointer. */
int fs_queue_take(fs_ctx* ctx, float* store, int capacity, size_t row_floats, const int32_t* take_idx, int B, const int32_t* move_src,
                  const int32_t* move_dst, int M, float* batch_out);

/* Uniform [0, 255) float32 images on the device: element e of out[0, n) is word (e & 3) of the Philox4x32-10 block with counter
 * (e >> 2, batch_index low, batch_index high, rank) and key (seed low, seed high), mapped by float(word >> 8) * 2^-24 * 255.0f (both products
 * rounded separately; the largest value is 254.99998).  A pure function of its arguments: independent of the launch geometry, so a resumed
 * run asks for batch `global_step` and continues the stream.  out: 16-byte aligned.  Errors: -1 null argument / n == 0 / n > 2^34,
 * -5 misaligned out. */
int fs_synth_uniform(fs_ctx* ctx, float* out, size_t n, uint64_t seed, uint32_t rank, uint64_t batch_index);

/* ---- Baseline JPEG decoding (csrc/fs_jpeg.hip): the host half works without a GPU, keeps no global state (any number of threads may
 * decode at once) and allocates nothing. */

/* What fs_jpeg_parse found in a handled JPEG, and where fs_jpeg_decode puts it.  The coefficient buffer of an image is coef_bytes long:
 * component c's plane starts at plane_offset[c] and holds blocks_y[c] rows of blocks_x[c] blocks (the component padded to whole MCUs), a block
 * being 64 int16 quantised coefficients in natural (de-zigzagged, row-major) order; coef_count int16 in all.  At qt_offset (a multiple of 16)
 * follow three tables of 64 uint16, natural order: the quantisation table of component 0, 1, 2 (zeros beyond ncomp).  All sizes in bytes
 * unless named otherwise.  No implicit padding: 22 int32, then uint64. */
typedef struct fs_jpeg_info {
    int32_t width, height;
    int32_t ncomp;                     /* 1 (grayscale) or 3 (YCbCr) */
    int32_t hs[3], vs[3];              /* sampling factors: component 0 is 1x1, 2x1 or 2x2, the chroma components 1x1 */
    int32_t tq[3];                     /* quantisation table each component names */
    int32_t mcu_x, mcu_y;              /* MCU grid */
    int32_t restart_interval;          /* MCUs between RSTn markers; 0: none */
    int32_t blocks_x[3], blocks_y[3];
    int32_t reserved;
    uint64_t scan_offset;              /* first byte of the entropy-coded data within the file */
    uint64_t plane_offset[3];
    uint64_t qt_offset;
    uint64_t coef_count;
    uint64_t coef_bytes;               /* what fs_jpeg_decode writes: qt_offset + 384 */
    uint64_t rgb_bytes;                /* width * height * 3 */
} fs_jpeg_info;

/* Reads the markers of a JPEG file image up to its scan.  Returns
 *    0  handled: *info is filled;
 *    1  a JPEG this decoder does not take (not an error: the caller decodes it with PIL);
 *  < 0  malformed (-1 not a JPEG / truncated / null argument, -2 a bad segment).
 * Handled: SOF0, or SOF1 with 8-bit samples; Huffman coded; ONE scan with all components (interleaved, or the single component of a grayscale
 * file); luma sampled 1x1, 2x1 or 2x2 against 1x1 chroma; YCbCr by the JFIF rule (a JFIF marker, or component ids 1, 2, 3) and no Adobe marker;
 * restart intervals; any Huffman tables (up to four per class, several per segment); 8-bit quantisation tables.  Everything else answers 1:
 * progressive, arithmetic, lossless, 12-bit, 16-bit quantisation tables, CMYK / Adobe files, 4:4:0 and other sampling factors, several scans,
 * a height given by DNL, tables left for the decoder to supply. */
int fs_jpeg_parse(const void* jpeg, size_t n, fs_jpeg_info* info);

/* Huffman-decodes the scan of a handled JPEG (info: what fs_jpeg_parse filled from the same bytes) into out[0, info->coef_bytes), laid out as
 * described at fs_jpeg_info.  Every read is checked against n, every code against its table; the call writes only inside out[0, coef_bytes).
 * Stricter than a viewer: whatever is not a complete, well-formed scan followed by EOI is an error, and the caller decodes that file the way it
 * did before.  Returns 0, 1 (as fs_jpeg_parse), or < 0: -1 / -2 as fs_jpeg_parse or an info / out_bytes that does not fit, -4 corrupt or
 * truncated scan data, -5 out not 2-byte aligned. */
int fs_jpeg_decode(const void* jpeg, size_t n, const fs_jpeg_info* info, void* out, size_t out_bytes);

/* One image of fs_jpeg_reconstruct_many: its coefficient planes start coef_offset bytes into coef_base (laid out as fs_jpeg_decode writes them
 * for this geometry) and its three quantisation tables qt_offset bytes into coef_base (for a buffer written by fs_jpeg_decode at byte o:
 * coef_offset = o, qt_offset = o + info.qt_offset); both multiples of 16.  hs, vs: the luma sampling factors (info.hs[0], info.vs[0]).  The
 * pixels go to rgb_base + dst_offset, height rows of width pixels of pixel_bytes bytes (3 = RGB, 4 = RGBX with dst_offset a multiple of 4), no
 * row padding: what an fs_resize_item with the same offset, shape and pixel_bytes describes.  48 bytes, 8-byte aligned. */
typedef struct fs_jpeg_item {
    uint64_t coef_offset;
    uint64_t qt_offset;
    uint64_t dst_offset;
    int32_t width, height;
    int32_t ncomp;
    int32_t hs, vs;
    int32_t pixel_bytes;
} fs_jpeg_item;

/* Dequantisation, inverse DCT, chroma upsampling and colour conversion of K images in one launch sequence (two kernels), in the integer
 * arithmetic of the IJG library's default decoder (accurate integer DCT, "fancy" triangle upsampling, 16-bit fixed-point YCbCr -> RGB): the
 * pixels PIL gives for the same file, bit for bit.  coef_base is WORKING memory: each block's coefficients are replaced by its samples, so a
 * region is reconstructed once.  The descriptor table is passed twice, as for fs_resize_bicubic_u8x_many (items_host is only checked).
 * Asynchronous on the ctx stream, allocates nothing, can be captured into a hipGraph.  No value of the coefficient data reaches an address: a
 * corrupt file that still decoded gives wrong pixels, nothing else; a descriptor the check refuses is skipped by the kernels too.
 * Errors: -1 null argument / K outside [1, 65535] / a bad geometry / an image outside coef_bytes or rgb_bytes, -2 a pixel_bytes other than 3
 * or 4, -5 items_dev not 8-byte aligned, coef_base or an image's coef_offset / qt_offset not 16-byte aligned, rgb_base or (4-byte pixels) a
 * dst_offset not 4-byte aligned. */
int fs_jpeg_reconstruct_many(fs_ctx* ctx, void* coef_base, size_t coef_bytes, const fs_jpeg_item* items_host, const fs_jpeg_item* items_dev,
                             int K, void* rgb_base, size_t rgb_bytes);

/* ---- Baseline JPEG encoding (csrc/fs_jpegenc.hip): the decoder's split, the other way round.  The data-parallel part -- colour conversion,
 * chroma downsampling, forward DCT, quantisation -- runs on the GPU (fs_jpeg_forward_many) and leaves, per image, exactly the coefficient buffer
 * fs_jpeg_decode would write for the file; the int16 coefficients cross PCIe and the serial part, Huffman coding and the markers, runs on host
 * threads (fs_jpeg_write: pure C, no HIP calls, no global state, no allocation; any number of threads at once).  The arithmetic is the integer
 * arithmetic of the IJG library's default compressor (16-bit fixed-point RGB -> YCbCr, box downsampling with the alternating bias, the accurate
 * integer DCT, the Annex K tables scaled by the quality), and the file is laid out as that library lays it out: the bytes PIL writes for the same
 * pixels, quality and subsampling (tests/test_jpeg_encode.py).  Not written: optimised Huffman tables, restart markers, progressive or arithmetic
 * coding, metadata beyond the JFIF header. */

/* One image of fs_jpeg_forward_many: height rows of width pixels of pixel_bytes bytes (3 = RGB, 4 = RGBX with src_offset a multiple of 4 and the
 * fourth byte never read, 1 = the samples of a grayscale image: ncomp 1), no row padding, src_offset bytes into src_base -- what fs_f32_to_u8 and
 * fs_jpeg_reconstruct_many produce.  The coefficient planes go to coef_base + coef_offset and the three quantisation tables to coef_base +
 * qt_offset (both multiples of 16; for a buffer fs_jpeg_write is to read at byte o: coef_offset = o, qt_offset = o + info.qt_offset).
 * hs, vs: the luma sampling factors, 1x1, 2x1 or 2x2 (4:4:4, 4:2:2, 4:2:0); quality: 1..100, the IJG scale.  56 bytes, 8-byte aligned. */
typedef struct fs_jpegenc_item {
    uint64_t src_offset;
    uint64_t coef_offset;
    uint64_t qt_offset;
    int32_t width, height;
    int32_t ncomp;
    int32_t hs, vs;
    int32_t pixel_bytes;
    int32_t quality;
    int32_t reserved;
} fs_jpegenc_item;

/* The mirror of fs_jpeg_reconstruct_many: K images in one launch sequence (two kernels).  Each image's region of coef_base first holds its
 * component samples (a block's first 64 bytes), then, in place, the quantised coefficients: 64 int16 per block in natural order, planes and
 * padding to whole MCUs as described at fs_jpeg_info, the tables (64 uint16 each, natural order, zeros beyond ncomp) derived from `quality`:
 * entry = (Annex K entry * scale + 50) / 100 clamped to [1, 255], scale = 5000 / quality below 50, else 200 - 2 * quality.  A block that only
 * pads the last MCU column or row is not transformed: its AC coefficients are 0 and its DC is that of the preceding block of its MCU.  The
 * source pixels are only read.  The descriptor table is passed twice, as for fs_resize_bicubic_u8x_many (items_host is only checked).
 * Asynchronous on the ctx stream, allocates nothing, can be captured into a hipGraph.  No value of the pixel data reaches an address; a
 * descriptor the check refuses is skipped by the kernels too.
 * Errors: -1 null argument / K outside [1, 65535] / a bad geometry / an image outside src_bytes or coef_bytes, -2 a pixel_bytes other than 3 or
 * 4 (other than 1 with ncomp 1) or a quality outside [1, 100], -5 items_dev not 8-byte aligned, coef_base or an image's coef_offset / qt_offset
 * not 16-byte aligned, the source of an image of 4-byte pixels not 4-byte aligned. */
int fs_jpeg_forward_many(fs_ctx* ctx, const void* src_base, size_t src_bytes, const fs_jpegenc_item* items_host, const fs_jpegenc_item* items_dev,
                         int K, void* coef_base, size_t coef_bytes);

/* The fs_jpeg_info that fs_jpeg_parse would report for the file fs_jpeg_write writes of a width x height image of ncomp components with luma
 * sampling hs x vs: tables 0 / 1 / 1, no restart interval, scan_offset 0.  Returns -1 for a geometry outside the handled set (dimensions
 * 1..65535; ncomp 1 with 1x1, or ncomp 3 with 1x1, 2x1 or 2x2) or a null info. */
int fs_jpeg_encode_plan(int width, int height, int ncomp, int hs, int vs, fs_jpeg_info* info);

/* A size that surely holds the file fs_jpeg_write writes for this info, whatever the coefficients (0: a null or inconsistent info). */
size_t fs_jpeg_write_bound(const fs_jpeg_info* info);

/* Writes the complete baseline file of the coefficient buffer `coef` (coef_bytes >= info->coef_bytes, laid out as fs_jpeg_decode /
 * fs_jpeg_forward_many leave it, the quantisation tables read at info->qt_offset) into out[0, cap) and its length into *n: SOI, the JFIF header
 * (1.01, no units, density 1x1), one DQT segment per table, SOF0, one DHT segment per Annex K Huffman table (DC 0, AC 0, DC 1, AC 1; the first
 * two for grayscale), SOS, the scan (zigzag order, DC prediction per component, ZRL / EOB, 0xFF bytes stuffed, the last byte padded with 1-bits),
 * EOI.  Every write is checked against cap.  Returns 0, or -1 null argument / an info that fs_jpeg_encode_plan did not fill / coef_bytes too
 * small / a quantisation entry outside [1, 255], -3 cap too small (nothing is written at or beyond out + cap), -4 a coefficient outside the
 * baseline range (a DC difference beyond category 11, an AC value beyond category 10), -5 coef not 2-byte aligned. */
int fs_jpeg_write(const fs_jpeg_info* info, const void* coef, size_t coef_bytes, void* out, size_t cap, size_t* n);

/* ---- cv2.resize of OpenCV 3.1.0 on u8 images (csrc/fs_cvresize.hip): the resampling of the reference's utils.imresize and of the frame loop's
 * --frame_size, bit-identical to faststyle_amd/cvresize.py (resize_cubic_u8 / resize_area_u8), whose docstring is the arithmetic contract.  The
 * encoder's split: a host-only plan, host-only per-axis tables, and one asynchronous device call. */

#define FS_CV_INTER_CUBIC 2           /* cv2.INTER_CUBIC */
#define FS_CV_INTER_AREA 3            /* cv2.INTER_AREA */
#define FS_CVRESIZE_PATH_CUBIC 0      /* 11-bit fixed-point Keys taps, int32 passes */
#define FS_CVRESIZE_PATH_AREA_FAST 1  /* integer factors on both axes: box means, no tables */
#define FS_CVRESIZE_PATH_AREA 2       /* fractional factors: coverage-weighted float32 sums in computeResizeAreaTab's order */

/* What fs_cvresize_plan reports.  The tables of the two axes share one buffer of table_bytes bytes: the x axis at x_offset, the y axis at
 * y_offset (multiples of 16).
 *   cubic      per output index 8 int32: the four source indices (clamped to the edge pixel), then their four 11-bit weights;
 *   area       n_dst + 1 int32 (entry d: the first tap of output index d; entry n_dst: x_taps / y_taps), padded to a multiple of 8 bytes, then per
 *              tap {int32 source index, float32 weight}, in computeResizeAreaTab's order;
 *   area fast  no tables (table_bytes 0): factor_x x factor_y boxes.
 * No implicit padding: 12 int32, then double and uint64. */
typedef struct fs_cvresize_info {
    int32_t src_h, src_w;
    int32_t dst_h, dst_w;              /* cvRound(src_h * fy), cvRound(src_w * fx), ties to even */
    int32_t interpolation;             /* FS_CV_INTER_CUBIC or FS_CV_INTER_AREA, as asked */
    int32_t path;                      /* FS_CVRESIZE_PATH_* */
    int32_t factor_x, factor_y;        /* area fast: cvRound(1 / fx), cvRound(1 / fy); else 0 */
    int32_t x_taps, y_taps;            /* area: entries of each axis table; else 0 */
    int32_t reserved[2];
    double fx, fy;
    uint64_t x_offset, y_offset;
    uint64_t table_bytes;
} fs_cvresize_info;

/* Plans cv2.resize(src [H,W,3] u8, dsize=None, fx, fy, interpolation).  Host only: no HIP call, no global state, no allocation.
 * Errors: -1 null plan / H or W outside [1, 32767] / fx or fy not finite and positive / a destination side outside [1, 32767],
 * -2 an interpolation other than the two above, or FS_CV_INTER_AREA with fx > 1 or fy > 1 (enlarging by area is not defined here). */
int fs_cvresize_plan(int H, int W, double fx, double fy, int interpolation, fs_cvresize_info* plan);

/* Writes the plan's tables into tables[0, plan->table_bytes): the double -> float32 arithmetic of cvresize._cubic_axis / _area_tab.  Host
 * only, as fs_cvresize_plan.  Errors: -1 null argument (tables may be null when table_bytes is 0) / a plan fs_cvresize_plan did not fill /
 * cap < table_bytes, -5 tables not 4-byte aligned. */
int fs_cvresize_tables(const fs_cvresize_info* plan, void* tables, size_t cap);

/* Resizes N images: src holds N images of src_h x src_w pixels of src_pixel_bytes bytes each (3 = RGB, 4 = RGBX as fs_jpeg_reconstruct_many
 * writes it, the fourth byte never read), back to back without padding; dst receives N packed-RGB images of dst_h x dst_w pixels; with
 * swap_rb != 0 R and B are exchanged on the way out (the BGR order of a cv2 capture).  tables_dev: the device copy of what fs_cvresize_tables
 * wrote (ignored for the area fast path).  Asynchronous on the ctx stream, allocates nothing, can be captured into a hipGraph.  No pixel value
 * reaches an address, and the kernels clamp every table entry into the source themselves: a stale or wrong table gives wrong pixels, nothing
 * else.  A refused call launches nothing.
 * Errors: -1 null argument / N outside [1, 65535] / a plan fs_cvresize_plan did not fill, -2 src_pixel_bytes other than 3 or 4,
 * -5 tables_dev not 16-byte aligned, or a source of 4-byte pixels not 4-byte aligned. */
int fs_cvresize_u8(fs_ctx* ctx, const fs_cvresize_info* plan, const void* tables_dev, const unsigned char* src, int src_pixel_bytes, int N,
                   int swap_rb, unsigned char* dst);

/* ---- Planar 8-bit YCbCr frames <-> packed RGB (csrc/fs_yuv.hip): the colour conversion of raw video streams (YUV4MPEG2, faststyle_amd/y4m.py),
 * so that a frame crosses PCIe as its planes (1.5 B/px for 4:2:0) and needs no entropy coder on the host.  A host-only plan and two asynchronous
 * device calls.  The arithmetic below is the contract (tests/test_yuv.py restates it in numpy and compares exactly); it is integer throughout.
 *
 * Layout: the Y plane (height rows of width samples), then Cb, then Cr (chroma_h rows of chroma_w samples each, chroma_w = ceil(width / hs),
 * chroma_h = ceil(height / vs)), back to back without padding, as YUV4MPEG2 stores a frame; a mono frame (ncomp 1) is its Y plane alone.
 *
 * Chroma upsampling to one u8 value per pixel: bilinear interpolation at the sited positions, edge samples replicated (neighbour indices
 * clamped), rounded half up once.  Every weight is dyadic, so each value is exact.  With C the chroma sample of the pixel's own cell
 * (column x / hs, row y / vs):
 *   centre siting (siting 0), a subsampled axis       near = C, far = the neighbour on the pixel's side of the cell (x or y even: the previous
 *                                                     sample, odd: the next); one axis (3 near + far + 2) >> 2, both axes
 *                                                     (9 a + 3 b + 3 c + d + 8) >> 4 with a near on both axes, d far on both;
 *   co-sited horizontally (siting 1, hs 2)            even column: the sample itself; odd column: (l + r + 1) >> 1 of C and its right neighbour;
 *   vertically (vs 2)                                 as centre siting, for either value of siting; with siting 1 the odd column of 4:2:0 is
 *                                                     (3 ln + 3 rn + lf + rf + 4) >> 3 (n the near row, f the far row).
 * (Not the IJG library's alternating-bias variant of fs_jpeg_reconstruct_many.)
 *
 * YCbCr -> RGB: with (Kr, Kb) = (0.299, 0.114) for BT.601 or (0.2126, 0.0722) for BT.709, Kg = 1 - Kr - Kb, and (sy, sc, oy) =
 * (255/219, 255/224, 16) for limited range or (1, 1, 0) for full range, the real formulas
 *   R = sy (Y - oy) + 2 (1 - Kr) sc (Cr - 128)
 *   B = sy (Y - oy) + 2 (1 - Kb) sc (Cb - 128)
 *   G = sy (Y - oy) - 2 (1 - Kb) Kb / Kg sc (Cb - 128) - 2 (1 - Kr) Kr / Kg sc (Cr - 128)
 * are evaluated with each coefficient c replaced by floor(c * 65536 + 0.5) (BT.601 limited range: 76309 for sy), the sum in int32, plus 32768,
 * arithmetic shift right by 16, clamped to [0, 255].  A mono frame reads as Cb = Cr = 128.
 *
 * RGB -> YCbCr, per pixel, to u8: the rows (Kr, Kg, Kb) / sy, (-Kr, -Kg, 1 - Kb) / (2 (1 - Kb)) / sc and (1 - Kr, -Kg, -Kb) / (2 (1 - Kr)) / sc,
 * each coefficient rounded the same way, the offset (oy, 128, 128) added as offset << 16, plus 32768, shift right by 16, clamped to [0, 255]
 * (full range reaches 256).
 *
 * Chroma downsampling of those u8 values, neighbour indices clamped to the image:
 *   centre siting     2x2: (a + b + c + d + 2) >> 2 of the cell's four pixels; 2x1: (a + b + 1) >> 1;
 *   co-sited          [1 2 1] / 4 about the even column m = 2 * column: (l + 2 m + r + 2) >> 2 for 2x1; for 2x2 that sum of the cell's two rows,
 *                     plus 4, >> 3;
 *   1x1               the value itself.  A mono frame gets its Y plane only. */

/* One frame geometry, filled by fs_yuv_plan.  No implicit padding: 12 int32, then 7 uint64 (104 bytes). */
typedef struct fs_yuv_desc {
    int32_t width, height;
    int32_t hs, vs;                    /* luma samples per chroma sample: 1x1 (4:4:4), 2x1 (4:2:2), 2x2 (4:2:0) */
    int32_t ncomp;                     /* 3, or 1: mono */
    int32_t siting;                    /* 0 centre (JPEG / MPEG-1), 1 horizontally co-sited with the even luma column (MPEG-2, 4:2:2) */
    int32_t matrix;                    /* 0 BT.601, 1 BT.709 */
    int32_t full_range;                /* 0: Y 16..235, chroma 16..240; 1: 0..255 */
    int32_t chroma_w, chroma_h;        /* ceil(width / hs), ceil(height / vs); 0 for mono */
    int32_t reserved[2];               /* 0, 0; fs_yuv_plan_deep: reserved[0] = bits per sample */
    uint64_t plane_offset[3];          /* within a frame, bytes */
    uint64_t plane_bytes[3];
    uint64_t frame_bytes;
} fs_yuv_desc;

/* Fills *desc.  Host only: no HIP call, no global state, no allocation.  Errors: -1 null desc / width or height outside [1, 32767],
 * -2 a sampling other than 1x1, 2x1, 2x2, ncomp other than 3 or 1 (1 with 1x1 only), siting, matrix or full_range other than 0 or 1. */
int fs_yuv_plan(int width, int height, int hs, int vs, int ncomp, int siting, int matrix, int full_range, fs_yuv_desc* desc);

/* N frames at yuv, desc->frame_bytes apart -> N images of height x width pixels of pixel_bytes bytes at rgb, back to back: 3 = packed R,G,B,
 * 4 = R,G,B,X with X written as 255 (what fs_cvresize_u8 reads); swap_rb != 0: the pixels are written B,G,R.  Asynchronous on the ctx stream,
 * allocates nothing, can be captured into a hipGraph; grid.y is the image.  No value read from a frame reaches an address.  A refused call
 * launches nothing.  Errors: -1 null argument / N outside [1, 65535] / a desc fs_yuv_plan did not fill, -2 pixel_bytes other than 3 or 4,
 * -5 rgb of 4-byte pixels not 4-byte aligned (yuv and packed rgb may have any alignment: 4-byte aligned buffers of a width that is a multiple
 * of 4 take the dword path, the others the byte path, with the same values). */
int fs_yuv_to_rgb_u8(fs_ctx* ctx, const fs_yuv_desc* desc, const void* yuv, int N, int pixel_bytes, int swap_rb, unsigned char* rgb);

/* The reverse: N images of pixel_bytes bytes per pixel at rgb (the fourth byte never read; swap_rb != 0: the source pixels are B,G,R) -> N
 * frames at yuv.  As fs_yuv_to_rgb_u8 in every other respect, error codes included. */
int fs_rgb_to_yuv_u8(fs_ctx* ctx, const fs_yuv_desc* desc, const unsigned char* rgb, int pixel_bytes, int swap_rb, int N, void* yuv);

/* ---- Planar YCbCr frames of 9 to 16 bits per sample <-> the net's fp32 tensors (csrc/fs_yuv16.hip): deep video (C420p10, C422p10, C444p12,
 * C420p16, Cmono16 ... of YUV4MPEG2) goes straight to the transformation net's [N, H, W, 3] fp32 input, and the net's fp32 output straight to
 * such planes, one kernel each way and no u8 stage on either side.  A host-only plan and two asynchronous device calls.  The arithmetic below
 * is the contract (tests/test_yuv_deep.py restates it in numpy and compares exactly); it is integer throughout.
 *
 * Samples: d = bits per sample, 9 <= d <= 16; k = d - 8, m = 2^d - 1.  A sample is an unsigned little-endian 16-bit word; a stored value above
 * m is read as m.  No sample value reaches an address.
 *
 * Layout: that of the 8-bit frames above with two bytes per sample: Y, Cb, Cr back to back, chroma ceil(width / hs) x ceil(height / vs), a mono
 * frame its Y plane alone.
 *
 * RGB scale: RGB lives on the net's 0..255 scale in unsigned 8.8 fixed point: an integer F in [0, 65280], value F / 256.
 *
 * Chroma resampling: exactly the integer formulas stated above for the 8-bit frames -- the same taps, clamping, rounding and siting rules --
 * applied to the d-bit values.  Every sum fits int32.
 *
 * Scale factors and offsets: (Kr, Kb) as above, Kg = 1 - Kr - Kb.  Limited range: sy = 65280 / (219 * 2^k), sc = 65280 / (224 * 2^k),
 * oy = 16 * 2^k.  Full range: sy = sc = 65280 / m, oy = 0.  The chroma offset is 2^(d-1) in both.  A mono frame reads as Cb = Cr = 2^(d-1).
 *
 * Planes -> RGB: the real formulas of the 8-bit contract,
 *   R = sy (Y - oy) + 2 (1 - Kr) sc (Cr - 2^(d-1))
 *   B = sy (Y - oy) + 2 (1 - Kb) sc (Cb - 2^(d-1))
 *   G = sy (Y - oy) - 2 (1 - Kb) Kb / Kg sc (Cb - 2^(d-1)) - 2 (1 - Kr) Kr / Kg sc (Cr - 2^(d-1))
 * with these sy, sc, oy, each coefficient c replaced by floor(c * 2^24 + 0.5) (d = 10, limited range: 1250247329 for sy), the sum in int64, plus
 * 2^23, arithmetic shift right by 24, clamped to [0, 65280]: that is F.  The net's input is (float)F * 0.00390625f, which is exact (a power of
 * two, F < 2^24).  Channel order R,G,B, or B,G,R with swap_rb.
 *
 * Net output -> planes: for each channel q = the float clamped to [0, 255], NaN -> 0; F = (int)(q * 256.0f) -- the product is exact, the
 * conversion truncates: numpy's astype carried to 8.8, so that F >> 8 is what fs_f32_to_u8 writes.  Y, Cb, Cr per pixel come from the rows
 * (Kr, Kg, Kb) / sy, (-Kr, -Kg, 1 - Kb) / (2 (1 - Kb)) / sc and (1 - Kr, -Kg, -Kb) / (2 (1 - Kr)) / sc applied to (F_R, F_G, F_B) with the
 * sy, sc above: coefficients floor(c * 2^24 + 0.5), int64 sums, the offset (oy, 2^(d-1), 2^(d-1)) added as offset << 24, plus 2^23, shift
 * right by 24, clamped to [0, m].  The per-pixel d-bit chroma is downsampled with the integer formulas above.
 *
 * Both directions are within 1 unit of floor(exact + 0.5) of the float64 formulas and equal to it in over 99.8 % of random samples; every
 * intermediate sum stays below 2^42. */

/* Fills *desc as fs_yuv_plan does, with every byte size and offset doubled and reserved[0] = bits.  Host only: no HIP call, no global state,
 * no allocation.  Errors: those of fs_yuv_plan, and -2 for bits outside [9, 16] (8 is not deep: fs_yuv_plan).  fs_yuv_to_rgb_u8 and
 * fs_rgb_to_yuv_u8 refuse such a desc with -1, as the two calls below refuse one of fs_yuv_plan. */
int fs_yuv_plan_deep(int width, int height, int hs, int vs, int ncomp, int siting, int matrix, int full_range, int bits, fs_yuv_desc* desc);

/* N frames at yuv, desc->frame_bytes apart -> [N, height, width, 3] fp32 at dst on the net's 0..255 scale (swap_rb != 0: written B,G,R).
 * Asynchronous on the ctx stream, allocates nothing, can be captured into a hipGraph; grid.y is the image.  A refused call launches nothing.
 * Errors: -1 null argument / N outside [1, 65535] / a desc that fs_yuv_plan_deep does not reproduce byte for byte, -5 yuv not 2-byte aligned
 * (a width that is a multiple of 4 with frames of a multiple of 8 bytes, yuv 8-byte and dst 16-byte aligned takes 8- and 16-byte accesses,
 * anything else single samples and floats, with the same values). */
int fs_yuv_deep_to_f32(fs_ctx* ctx, const fs_yuv_desc* desc, const void* yuv, int N, int swap_rb, float* dst);

/* The reverse: [N, height, width, 3] fp32 at src (swap_rb != 0: the source channels are B,G,R) -> N frames at yuv.  As fs_yuv_deep_to_f32 in
 * every other respect, error codes included. */
int fs_f32_to_yuv_deep(fs_ctx* ctx, const fs_yuv_desc* desc, const float* src, int swap_rb, int N, void* yuv);

/* ---- Style strength, colour preservation and a region mask (csrc/fs_compose.hip): the net's fp32 output blended back towards the net's fp32
 * input, one elementwise launch between the forward pass and whichever output conversion follows (fs_f32_to_u8, fs_jpeg_forward_many,
 * fs_rgb_to_yuv_u8, fs_f32_to_yuv_deep: each consumes the composed tensor unchanged).  The arithmetic below is the contract
 * (tests/test_compose.py restates it in numpy and compares exactly); it is integer throughout, on the unsigned 8.8 scale of the deep video
 * block above, so no float tolerance and no contraction question arises.
 *
 * Inputs per image: src [H, W, 3] fp32, the net's input; net [Ho, Wo, 3] fp32, the net's output, H <= Ho <= H + 3 and W <= Wo <= W + 3
 * (fs_tnet_out_shape gives Ho = 4 ceil(ceil(H / 2) / 2): the output is up to 3 rows and columns larger and aligned top-left); optionally mask
 * [H, W] u8, shared by the N images.  Source and mask are read at (min(y, H - 1), min(x, W - 1)).  No value read from a tensor or the mask
 * reaches an address.
 *
 * For output pixel (y, x) and channel c:
 *   to 8.8     to88(v): q = v clamped to [0, 255], NaN -> 0; (int)(q * 256.0f) -- exactly fs_f32_to_yuv_deep's conversion.
 *              A_c = to88(src), B_c = to88(net).
 *   luma       (kr, kg, kb) = (19595, 38470, 7471) for BT.601, (13933, 46871, 4732) for BT.709; each triple sums to 65536.
 *              L(X) = (kr X_R + kg X_G + kb X_B + 32768) >> 16, in int64.  bgr 1: channel 0 is blue (the meaning of swap_rb in
 *              fs_f32_to_yuv_deep: "the source channels are B,G,R").
 *   orders     bgr 0 and 1 take src and net in one channel order.  The frame tools keep the reference's channel handling -- the net is FED
 *              B,G,R and its output is SHOWN as R,G,B -- so there the source must be read the other way round to show through in its own
 *              colours: bgr + 2 (2: net R,G,B and src B,G,R; 3: net B,G,R and src R,G,B) reads src with channels 0 and 2 exchanged, A_c =
 *              to88(src channel 2 - c), and is bgr in every other respect.
 *   delta      plain: D_c = B_c - A_c.  keep_color: D_c = L(B) - L(A) for the three channels -- one delta added to R, G and B moves Y by
 *              that delta and leaves Cb and Cr where they were, so no YCbCr round trip is needed and the result holds for every output kind.
 *   weight     m = the mask byte, 255 without a mask; m' = m + (m >> 7), in 0..256 with 255 -> 256; w = strength_q8 * m', in [0, 65536].
 *   result     F_c = clamp(A_c + (((int64)D_c * w + 32768) >> 16), 0, 65280), the shift arithmetic (a floor); the output is
 *              (float)F_c * 0.00390625f, which is exact.
 * Hence: strength_q8 256 without a mask in plain mode gives F = B, and a u8 / JPEG / 8-bit YCbCr conversion behind it writes byte for byte
 * what it writes for the net's tensor (F >> 8 is what fs_f32_to_u8 writes); strength_q8 0 or a mask byte 0 gives F = A; net == src (bgr 0 or 1) gives
 * F = A in every mode; under keep_color, where no clamp acts, F_c - F_c' = A_c - A_c' for every channel pair. */

/* N images: src [N, H, W, 3], net [N, Ho, Wo, 3], mask [H, W] or null, dst [N, Ho, Wo, 3]; dst may be net (a thread reads its pixels before it
 * writes them).  matrix: 0 BT.601, 1 BT.709, as in fs_yuv_plan.  Asynchronous on the ctx stream, allocates nothing, can be captured into a
 * hipGraph; grid.y is the image.  A refused call launches nothing.  Errors: -1 null src / net / dst, N outside [1, 65535], H or W below 1, Ho
 * outside [H, H + 3] or Wo outside [W, W + 3]; -2 strength_q8 outside [0, 256], a matrix other than 0 or 1, bgr outside [0, 3]; -5 src, net or dst not 4-byte
 * aligned (W == Wo a multiple of 4 with the three tensors 16-byte aligned takes 16-byte accesses, and a 4-byte aligned mask dwords; anything
 * else single floats and bytes, with the same values). */
int fs_compose_f32(fs_ctx* ctx, const float* src, int H, int W, const float* net, int Ho, int Wo, int N, int strength_q8, int keep_color,
                   int matrix, int bgr, const unsigned char* mask, float* dst);

/* ---- Two styles per stream (csrc/fs_mix.hip): the fp32 outputs of two nets merged by a weight per image and an optional region mask, one
 * elementwise launch between the two forward passes and fs_compose_f32 (or whichever stage or output conversion follows: each consumes the
 * mixed tensor unchanged).  The arithmetic below is the contract (tests/test_mix.py restates it in numpy and compares exactly); it is
 * integer throughout, on compose's unsigned 8.8 scale.
 *
 * Inputs per image: a and b [Ho, Wo, 3] fp32, the two nets' outputs; optionally mask [H, W] u8 at the net's INPUT size, H <= Ho <= H + 3 and
 * W <= Wo <= W + 3 as in compose, read at (min(y, H - 1), min(x, W - 1)) and shared by the N images; a weight t in [0, 256], one for all
 * images (weight_q8) or one int32 per image in device memory (weight_dev; weight_q8 is then ignored and every value read is clamped to
 * [0, 256]).  No value read from a tensor, the mask or the weight buffer reaches an address.
 *
 * For output pixel (y, x) and channel c, to88 being compose's:
 *   A_c = to88(a), B_c = to88(b).
 *   weight     m = the mask byte, 255 without a mask; m' = m + (m >> 7); w = t * m', in [0, 65536].
 *   result     F_c = A_c + (((int64)(B_c - A_c) * w + 32768) >> 16), the shift arithmetic (a floor); the output is (float)F_c * 0.00390625f,
 *              which is exact.  No clamp: F is a convex combination of two values in [0, 65280] and the rounding cannot pass either end
 *              (with D = B - A >= 0 the rounded term lies in [0, D], with D < 0 in [D, 0]) -- the argument DESIGN.md section 7h gives.
 * Hence: t 0 or a mask byte 0 gives F = A = to88(a); t 256 without a mask or with mask byte 255 gives F = B = to88(b); t 128 between 0 and 255
 * gives 32640; a == b gives to88 of it; and F >> 8 is the byte fs_f32_to_u8 writes, so a u8 / JPEG / 8-bit YCbCr conversion behind weight 0
 * writes byte for byte what it writes for a, behind weight 256 what it writes for b. */

/* N images: a, b, dst [N, Ho, Wo, 3]; mask [H, W] or null; weight_dev N int32 in device memory or null.  dst may be a or b and a may be b (a
 * thread reads its pixels before it writes them).  Asynchronous on the ctx stream, allocates nothing, can be captured into a hipGraph -- with
 * weight_dev one captured graph serves every weight; grid.y is the image.  A refused call launches nothing.  Errors: -1 null a / b / dst, N
 * outside [1, 65535], H or W below 1, Ho outside [H, H + 3] or Wo outside [W, W + 3]; -2 weight_q8 outside [0, 256] when weight_dev is null;
 * -5 a, b, dst or weight_dev not 4-byte aligned (Wo a multiple of 4 with the three tensors 16-byte aligned takes 16-byte accesses, and with
 * W == Wo and a 4-byte aligned mask dwords; anything else single floats and bytes, with the same values). */
int fs_mix_f32(fs_ctx* ctx, const float* a, const float* b, int H, int W, int Ho, int Wo, int N, int weight_q8, const int* weight_dev,
               const unsigned char* mask, float* dst);

/* ---- Temporal stabilisation (csrc/fs_temporal.hip): a recursive, motion-compensated blend of the tensor the output conversions would read
 * towards the previous frame's stabilised output, three launches behind the forward pass (or fs_compose_f32).  The arithmetic below is the
 * contract (tests/test_temporal.py restates it in numpy and compares for equality); it is integer throughout, on compose's unsigned 8.8 scale.
 *
 * Inputs, one image per call (N consecutive frames per call: fs_temporal_batch_f32 below): src [H, W, 3] fp32, the net's input; cur [Ho, Wo, 3] fp32, the net's output or the composed tensor, H <= Ho <=
 * H + 3 and W <= Wo <= W + 3, aligned top-left.  to88 is compose's.  clampy(v) = min(max(v, 0), Ho - 1), clampx likewise with Wo.
 *
 *   luma       cur8 [Ho, Wo] u8: A_c = to88(src[min(y, H - 1)][min(x, W - 1)][c]); Y = (k0 A_0 + k1 A_1 + k2 A_2 + 32768) >> 16 in int64 with
 *              compose's weight triples (matrix 0 BT.601, 1 BT.709), k0 the blue weight when src_bgr says channel 0 of src is blue;
 *              cur8 = Y >> 8.
 *   blocks     16 x 16, anchored top-left: nby = ceil(Ho / 16), nbx = ceil(Wo / 16); a ragged block holds only its pixels inside the frame,
 *              npix of them.
 *   search     needs the previous frame's luma prev8; radius R in [0, 7].  For every (dy, dx) in [-R, R]^2:
 *                SAD  = sum over the block's pixels (y, x) of |cur8[y][x] - prev8[clampy(y + dy)][clampx(x + dx)]|
 *                cost = SAD + (npix >> 5) (|dy| + |dx|)                                  (below 2^17)
 *                key  = cost << 12 | (|dy| + |dx|) << 8 | (dy + 7) << 4 | (dx + 7)       (29 bits)
 *              and the smallest key wins: mv[by][bx] = (dy, dx), two signed char.  The motion penalty keeps flat and noisy blocks at rest;
 *              the key orders every tie: smaller motion first, then smaller dy, then smaller dx.  Without a previous frame, or with R = 0,
 *              every vector is (0, 0).
 *   blend      pixel p = (y, x) of block b, (dy, dx) = mv[b], q = (clampy(y + dy), clampx(x + dx)):
 *                e    = |cur8[p] - prev8[q]|
 *                conf = max(0, 256 - e K), the sensitivity K in [1, 256]
 *                w    = strength_q8 conf, in [0, 65536]
 *                B_c  = to88(cur[p][c]);  P_c = prev88[q][c], the previous frame's stabilised output as u16 on the 8.8 scale
 *                F_c  = B_c + (((int64)(P_c - B_c) w + 32768) >> 16), the shift arithmetic (a floor)
 *                dst[p][c] = (float)F_c * 2^-8 (exact);  out88[p][c] = F_c
 *              Without a previous frame F_c = B_c.  F_c is a convex combination of B_c and P_c, both in [0, 65280] (w / 65536 lies in
 *              [0, 1], and the rounding cannot pass either end), so no clamp is needed.
 * Hence: strength_q8 0, the first frame, or e K >= 256 everywhere give F = to88(cur), and a u8 / JPEG / 8-bit or deep YCbCr conversion behind
 * the stage writes byte for byte what it writes without it; strength_q8 256 with e = 0 gives F = P exactly.
 *
 * prev_luma / prev_out88: the luma / out88 a previous call wrote, both null for "no previous frame"; luma [Ho, Wo] u8, out88 [Ho, Wo, 3] u16 and
 * mv [nby, nbx, 2] signed char are written for the next call.  dst may be cur (a thread reads its own pixels before it writes them); prev_luma
 * and prev_out88 are read at displaced positions and may not be luma / out88.  No value read from a tensor reaches an address except through
 * mv, which the search bounds by R and the blend holds to R again before it clamps q.  Asynchronous on the ctx stream, allocates nothing, can
 * be captured into a hipGraph.  A refused call launches nothing.  Errors: -1 null src / cur / luma / out88 / mv / dst, exactly one of the two
 * prev pointers null, prev_luma == luma or prev_out88 == out88, H or W below 1, Ho outside [H, H + 3] or Wo outside [W, W + 3]; -2 strength_q8
 * outside [0, 256], sensitivity outside [1, 256], radius outside [0, 7], matrix or src_bgr other than 0 or 1; -5 src, cur or dst not 4-byte
 * aligned, prev_out88 or out88 not 2-byte aligned. */
int fs_temporal_f32(fs_ctx* ctx, const float* src, int H, int W, const float* cur, int Ho, int Wo, int strength_q8, int sensitivity, int radius,
                    int matrix, int src_bgr, const unsigned char* prev_luma, const unsigned short* prev_out88, unsigned char* luma,
                    unsigned short* out88, signed char* mv, float* dst);

/* ---- Coarse-to-fine block search for the temporal stage (csrc/fs_temporal.hip): the search above reaches R <= 7 pixels; this one runs it on
 * a pyramid of `levels` L in {1, 2, 3} halved lumas, each level's window displaced by twice the vector of the level above.  Luma and blend
 * are those of fs_temporal_f32; the arithmetic below is the contract (tests/test_temporal_pyr.py restates it), integer throughout.
 *
 *   pyramid    level 0 is cur8: H_0 = Ho, W_0 = Wo.  For l >= 1: H_l = ceil(H_{l-1} / 2), W_l = ceil(W_{l-1} / 2) and
 *                L_l[y][x] = (a + b + c + d + 2) >> 2, a .. d = L_{l-1}[min(2y + i, H_{l-1} - 1)][min(2x + j, W_{l-1} - 1)] for i, j in {0, 1}.
 *              The levels 1 .. L-1 of the current frame are written into the state (pyr), where the next call reads them as the previous
 *              frame's (prev_pyr).
 *   search     from level L-1 down to level 0.  Each level has its own 16 x 16 block grid anchored top-left, nby_l = ceil(H_l / 16), nbx_l =
 *              ceil(W_l / 16), npix per ragged block as above.  The predictor p = (py, px) of block (by, bx) is (0, 0) at level L-1 and
 *              2 v_{l+1}[by >> 1][bx >> 1] below it (that parent block always exists).  For every (ry, rx) in [-R, R]^2:
 *                SAD  = sum over the block's pixels (y, x) of |cur_l[y][x] - prev_l[clampy_l(y + py + ry)][clampx_l(x + px + rx)]|
 *                cost = SAD + (npix >> 5) (|ry| + |rx|)
 *                key  = cost << 12 | (|ry| + |rx|) << 8 | (ry + 7) << 4 | (rx + 7)
 *              and the smallest key wins: v_l[b] = p + (ry, rx).  The penalty and the tie order apply to the refinement, not to the whole
 *              vector.  mv = v_0, two signed char per block, |component| <= R (2^L - 1) <= 49.  Without a previous frame, or with R = 0,
 *              every vector of every level is (0, 0).  With L = 1 this is the search of fs_temporal_f32, term for term.
 *   blend      as above, with the vectors held to R (2^L - 1) instead of R before q is clamped.
 * Reach: a vector can be as long as R (2^L - 1), but motion is reliably found only where the coarsest level sees it, about R 2^(L-1) pixels:
 * 14 at L = 2, 28 at L = 3 (at L = 3 a move by (20, -33) is mostly lost, since -33 / 4 lies outside 7).  Not provided: L above 3 (the coarsest
 * level of a small frame becomes one ragged block), a second zero-vector predictor per level, smoothing of the vector field
 * (sub-pixel vectors and batches, which stood in this list: fs_temporal_sub_f32 and fs_temporal_batch_f32 below). */

#define FS_TEMPORAL_MAX_LEVELS 3

/* What fs_temporal_pyr_layout reports: the sizes and block counts of the levels 0 .. levels - 1 (zero beyond), and where the parts of the one
 * extra state buffer `pyr` lie: the luma of level l >= 1 (h[l] w[l] bytes) at luma_offset[l], then the vectors v_l of level l >= 1 (2 nby[l]
 * nbx[l] signed char) at mv_offset[l], each a multiple of 16; entry 0 of both is 0 and unused (level 0 lives in luma and mv).  pyr_bytes is
 * the buffer's size, 0 for levels = 1.  No implicit padding: 14 int32, then uint64. */
typedef struct fs_temporal_pyr_info {
    int32_t levels, reserved;
    int32_t h[FS_TEMPORAL_MAX_LEVELS], w[FS_TEMPORAL_MAX_LEVELS];
    int32_t nby[FS_TEMPORAL_MAX_LEVELS], nbx[FS_TEMPORAL_MAX_LEVELS];
    uint64_t luma_offset[FS_TEMPORAL_MAX_LEVELS], mv_offset[FS_TEMPORAL_MAX_LEVELS];
    uint64_t pyr_bytes;
} fs_temporal_pyr_info;

/* Host only: no HIP call, no global state, no allocation.  Errors: -1 null info, Ho or Wo below 1; -2 levels outside [1, 3]. */
int fs_temporal_pyr_layout(int Ho, int Wo, int levels, fs_temporal_pyr_info* info);

/* fs_temporal_f32 with the coarse-to-fine search: 2 + levels launches, and one more for the pyramid when levels > 1.  pyr / prev_pyr: the
 * extra state buffer written / the one the previous call wrote (fs_temporal_pyr_layout; bytes, no alignment asked); both are ignored and may
 * be null with levels = 1.  A predictor is held to 2 R (2^(L-1-l) - 1) per component before it reaches an address and every window byte is
 * clamped into its level, so a stale prev_pyr gives wrong vectors and nothing else.  Asynchronous on the ctx stream, allocates nothing, can be
 * captured into a hipGraph.  A refused call launches nothing.  Errors: those of fs_temporal_f32, and -2 levels outside [1, 3]; with levels >
 * 1: -1 null pyr, prev_pyr null while prev_luma and prev_out88 are given or the reverse, prev_pyr == pyr. */
int fs_temporal_pyr_f32(fs_ctx* ctx, const float* src, int H, int W, const float* cur, int Ho, int Wo, int strength_q8, int sensitivity,
                        int radius, int levels, int matrix, int src_bgr, const unsigned char* prev_luma, const unsigned short* prev_out88,
                        const unsigned char* prev_pyr, unsigned char* luma, unsigned short* out88, unsigned char* pyr, signed char* mv,
                        float* dst);

/* ---- Quarter-pixel block vectors for the temporal stage (csrc/fs_temporal.hip): `subpel` S in {0, 1, 2} gives vectors in whole, half or
 * quarter pixels, so that the stage follows a slow pan instead of switching itself off on moving texture.  Luma, pyramid and the `levels`
 * searches are those of fs_temporal_pyr_f32 and yield mv; the arithmetic below, at level 0 only, is the contract (tests/test_temporal_sub.py
 * restates it), integer throughout.
 *
 *   refinement for block b with (dy, dx) = mv[b]:
 *                SAD(u, v) = sum over the block's pixels (y, x) of |cur8[y][x] - prev8[clampy(y + u)][clampx(x + v)]| (a ragged block: its
 *                pixels inside the frame), raw sums without the search's motion penalty.
 *                S0 = SAD(dy, dx), Sym = SAD(dy - 1, dx), Syp = SAD(dy + 1, dx), Sxm = SAD(dy, dx - 1), Sxp = SAD(dy, dx + 1)
 *                fit(m, p): E = max(m, p) - S0; 0 if E <= 0; otherwise g = floor((2^S (m - p) + E) / (2 E)) (a true floor, also of a
 *                negative numerator), held to [-2^(S-1), 2^(S-1)]; the result is g 2^(2-S), in quarter pixels.
 *                mvf[b] = (fit(Sym, Syp), fit(Sxm, Sxp)), two signed char in [-2, 2]; at S = 1 each is in {-2, 0, 2}.
 *              It is the equiangular line fit through the winner and its two neighbours per axis.  Without a previous frame, with R = 0 or
 *              with S = 0 every mvf is (0, 0); with S = 0 mvf is not written and may be null.  mv keeps its meaning: the block's vector in
 *              quarter pixels is 4 mv + mvf.  A flat block has E = 0 and stays whole.  A neighbour one pixel beyond the search bound is a
 *              clamped read like any other, and nothing is stored from it.
 *   blend      pixel p = (y, x) of block b; dy, dx held to R (2^L - 1) and fy, fx to [-2, 2]:
 *                Y4 = 4 (y + dy) + fy; y0 = Y4 >> 2 (arithmetic); ay = Y4 & 3; r0 = clampy(y0), r1 = clampy(y0 + 1)
 *                X4 = 4 (x + dx) + fx; x0 = X4 >> 2; ax = X4 & 3; c0 = clampx(x0), c1 = clampx(x0 + 1)
 *                bil(a, b, c, d) = ((4 - ay) ((4 - ax) a + ax b) + ay ((4 - ax) c + ax d) + 8) >> 4
 *                pq  = bil(prev8[r0][c0], prev8[r0][c1], prev8[r1][c0], prev8[r1][c1])
 *                P_c = bil of the four u16 prev88[..][..][c]
 *              and then as fs_temporal_f32's blend: e = |cur8[p] - pq|, conf, w, F_c = B_c + (((int64)(P_c - B_c) w + 32768) >> 16), dst,
 *              out88.  bil of values in [0, 65280] lies in [0, 65280]: still no clamp.
 * Hence: where mvf[b] = (0, 0), bil returns its first argument and the block's pixels are those of fs_temporal_pyr_f32, bit for bit; S = 0
 * is fs_temporal_pyr_f32 term for term; strength_q8 0, a first frame, or e K >= 256 everywhere still give F = to88(cur); strength_q8 256 on a
 * still picture still returns the first frame in every block whose fraction is (0, 0).  A still block has S0 = 0 and E = max(m, p), so the
 * fit leaves it whole exactly while the smaller neighbour sum along each axis stays above (1 - 2^-S) of the larger; an edge that lies on the
 * block's first or last row or column, or a ragged block of few rows or columns, whose clamped neighbour repeats pixels, can fall below that
 * and is then fetched a fraction away (a ragged block of one row takes (2, 0) and fetches the same row twice: no change).  Known property:
 * under steady fractional motion the state is resampled bilinearly on every frame, so at strength 1 and full confidence the stabilised
 * picture softens over time; below 1 the current frame re-injects its detail.
 * Not provided: smoothing of the vectors, a sharper (bicubic) fetch, fractions at coarse levels (overlapped blocks, the smoothed confidence
 * and batches, which stood in this list: fs_temporal_obmc_f32 and fs_temporal_batch_f32 below).
 *
 * mvf [nby, nbx, 2] signed char is written for inspection (the next call does not read it).  With S > 0: fs_temporal_pyr_f32's launches, one
 * more for the refinement, and the bilinear blend in place of the whole-pixel one: 4 launches at L = 1, 6 at L = 2, 7 at L = 3.  mv is held to
 * R (2^L - 1) and mvf to [-2, 2] before either reaches an address.  Asynchronous on the ctx stream, allocates nothing, can be captured into a
 * hipGraph.  A refused call launches nothing.  Errors: those of fs_temporal_pyr_f32, -2 subpel outside [0, 2], -1 null mvf with subpel > 0. */
int fs_temporal_sub_f32(fs_ctx* ctx, const float* src, int H, int W, const float* cur, int Ho, int Wo, int strength_q8, int sensitivity,
                        int radius, int levels, int subpel, int matrix, int src_bgr, const unsigned char* prev_luma,
                        const unsigned short* prev_out88, const unsigned char* prev_pyr, unsigned char* luma, unsigned short* out88,
                        unsigned char* pyr, signed char* mv, signed char* mvf, float* dst);

/* ---- Overlapped block vectors for the temporal stage (csrc/fs_temporal.hip): with `overlap` 1 every pixel considers the vectors of the four
 * blocks whose centres surround it, weighs them by a bilinear window and by how well the source matched along each, and blends towards the
 * confidence-weighted prediction, so that the pixels of a block that straddles a motion edge keep their weight on either side of it.  Luma,
 * pyramid, the `levels` searches and (with subpel > 0) the refinement are those of fs_temporal_sub_f32 and yield mv and mvf; without subpel
 * read mvf as 0.  The state gains no buffer.  Only the blend differs; its arithmetic below is the contract (tests/test_temporal_obmc.py
 * restates it), integer throughout.
 *
 *   window     pixel (y, x): ty = 2 y - 15; j0 = ty >> 5 (arithmetic); ay = ty & 31.  The two block rows are clamp(j0, 0, nby - 1) and
 *              clamp(j0 + 1, 0, nby - 1) with the weights 32 - ay and ay; the columns likewise from tx = 2 x - 15 with ax and nbx.  The four
 *              candidates k have the window weight w_k = wy wx; the four sum to 1024.  Block centres sit at 16 b + 7.5 and the window is
 *              symmetric about them.  A clamped index repeats the border block: a frame of one block has four equal candidates.
 *   candidate  k with block b_k: mv[b_k] held to R (2^L - 1) and mvf[b_k] to [-2, 2]; pq_k and P_k,c are fetched exactly as the blend of
 *              fs_temporal_sub_f32 fetches them for that vector -- bil of prev8 and prev88 at 4 (p + mv) + mvf quarter pixels, every
 *              coordinate clamped; with subpel 0 the plain fetch of fs_temporal_f32 at the clamped q.
 *                e_k = |cur8[p] - pq_k|;  conf_k = max(0, 256 - e_k K)
 *   blend      D = sum w_k conf_k (at most 2^18);  N_c = sum w_k conf_k P_k,c (below 2^34);  cmax = max conf_k.
 *              D = 0: F_c = B_c.  Otherwise
 *                Pbar_c = (2 N_c + D) / (2 D), a floor of non-negative integers: the rounded weighted mean, between the smallest and the
 *                         largest P_k,c and so in [0, 65280]
 *                cbar   = min(cmax, D >> 8)
 *                w      = strength_q8 cbar, in [0, 65536]
 *                F_c    = B_c + (((int64)(Pbar_c - B_c) w + 32768) >> 16)
 *              dst and out88 as fs_temporal_f32's; still no clamp.  Without a previous frame F = B.
 * D >> 8 lets a candidate count four times its window share; a pixel's own block has w_k >= 17 x 17 = 289 > 256, so whenever its own vector
 * matches the pixel keeps everything the whole-block blend gave it.  Hence:
 *   1. where the four candidates' held quarter-pixel vectors 4 mv + mvf are equal, the pixel is that of fs_temporal_sub_f32 (of
 *      fs_temporal_f32 without fractions), bit for bit: Pbar = P and cbar = conf.  Uniform motion, the inside of a moving region and a frame
 *      of one block are such.
 *   2. the same holds where every candidate other than the pixel's own block has conf_k = 0.
 *   3. cbar is never below the conf of the whole-block blend for the same mv and mvf.
 *   4. strength_q8 0, a first frame, or e_k K >= 256 for every candidate give F = to88(cur), and a conversion behind the stage writes byte
 *      for byte what it writes without it.
 *   5. strength_q8 256 on a still picture returns the first frame wherever the four candidates' vectors are (0, 0).
 * Not provided: a vector median or other smoothing of mv itself, windows wider than the four nearest blocks, overlap at coarse levels or in
 * the search, a bicubic fetch (batches, which stood in this list: fs_temporal_batch_f32 below).
 *
 * overlap 0 is fs_temporal_sub_f32 term for term (subpel 0 with a null mvf included).  overlap 1 runs the same launches with the blend
 * replaced: 3 at L = 1, S = 0; 7 at L = 3, S = 2.  mv, mvf and the block indices are held to their bounds before any reaches an address.
 * Asynchronous on the ctx stream, allocates nothing, can be captured into a hipGraph.  A refused call launches nothing.  Errors: those of
 * fs_temporal_sub_f32, and -2 overlap outside [0, 1]. */
int fs_temporal_obmc_f32(fs_ctx* ctx, const float* src, int H, int W, const float* cur, int Ho, int Wo, int strength_q8, int sensitivity,
                         int radius, int levels, int subpel, int overlap, int matrix, int src_bgr, const unsigned char* prev_luma,
                         const unsigned short* prev_out88, const unsigned char* prev_pyr, unsigned char* luma, unsigned short* out88,
                         unsigned char* pyr, signed char* mv, signed char* mvf, float* dst);

/* ---- Batches of consecutive frames for the temporal stage (csrc/fs_temporal.hip): `frames` N in [1, 64] successive frames of one stream in
 * one call, oldest first.  The arithmetic is that of the four blocks above and is not restated: the call writes bit for bit what N successive
 * calls of fs_temporal_obmc_f32 with the same parameters write, frame 0 reading the prev_* state (all null: no previous frame -- zero vectors
 * and F = B for frame 0 only), frame i > 0 the state frame i - 1 wrote.  luma / out88 / pyr / mv / mvf receive frame N - 1's state, which the
 * next call reads as its prev_*; dst[i] is frame i's stabilised tensor; dst may be cur.  Only the blend is recursive, so luma, pyramid, every
 * search level and the refinement run once over all frames (the frame is one more grid dimension) and the N blends follow in order: 2 + N
 * launches at L = 1, S = 0; 6 + N at L = 3, S = 2.
 *
 * The state of the frames 0 .. N - 2 lives in `work` (device memory, 16-byte aligned, fs_temporal_batch_layout's work_bytes; nothing is kept
 * in it between calls).  Its layout is private but for the vectors: frame i < N - 1 has mv [nby, nbx, 2] signed char at work + mv_offset +
 * i mv_stride and, with subpel > 0, mvf at work + mvf_offset + i mvf_stride (frame N - 1's are in mv / mvf).  It holds two out88 frames
 * whatever N is: a blend reads its predecessor's only.  With frames = 1 the call is fs_temporal_obmc_f32 term for term, work_bytes is 0 and
 * work may be null.  No implicit padding: 4 int32, then uint64. */
typedef struct fs_temporal_batch_info {
    int32_t frames, levels, subpel, reserved;
    uint64_t mv_offset, mv_stride, mvf_offset, mvf_stride, work_bytes;
} fs_temporal_batch_info;

/* Host only: no HIP call, no global state, no allocation.  Errors: -1 null info, Ho or Wo below 1, frames outside [1, 64]; -2 levels outside
 * [1, 3], subpel outside [0, 2]. */
int fs_temporal_batch_layout(int Ho, int Wo, int levels, int subpel, int frames, fs_temporal_batch_info* info);

/* src [frames, H, W, 3], cur and dst [frames, Ho, Wo, 3] fp32.  The frame index comes from the grid and is bounded by `frames`; no value
 * read from a tensor reaches an address except through the held vectors, as in the single-frame calls.  Asynchronous on the ctx stream,
 * allocates nothing, can be captured into a hipGraph.  A refused call launches nothing.  Errors: those of fs_temporal_obmc_f32; -1 frames
 * outside [1, 64]; with frames > 1: -1 null work or work_bytes below the layout's, -5 work not 16-byte aligned. */
int fs_temporal_batch_f32(fs_ctx* ctx, const float* src, int H, int W, const float* cur, int Ho, int Wo, int frames, int strength_q8,
                          int sensitivity, int radius, int levels, int subpel, int overlap, int matrix, int src_bgr,
                          const unsigned char* prev_luma, const unsigned short* prev_out88, const unsigned char* prev_pyr, unsigned char* luma,
                          unsigned short* out88, unsigned char* pyr, signed char* mv, signed char* mvf, void* work, size_t work_bytes,
                          float* dst);

/* ---- Batches of independent streams for the temporal stage (csrc/fs_temporal.hip): `streams` S in [1, 64] streams, one frame of each, in
 * one call.  The arithmetic is that of the blocks above and is not restated: for every stream s without FS_TS_SKIP the call writes bit for
 * bit what fs_temporal_obmc_f32 writes for image s of src and cur with the same parameters, its prev_* being the slot of stream s that this
 * pass does not write where FS_TS_PREV is set and all null where it is clear (no previous frame: zero vectors and F = B), its luma / out88 /
 * pyr / mv / mvf the slot written, its dst image s of dst; dst may be cur.  For a stream with FS_TS_SKIP nothing is read or written: neither
 * of its slots nor image s of dst.  Nothing is recursive inside such a pass, so luma, pyramid, every search level, the refinement and the
 * blend each run once over all streams (the stream is one more grid dimension): the launches are those of one single-frame call whatever S
 * is, 3 at L = 1, S = 0 and 7 at L = 3, S = 2.
 *
 * What differs per stream is a device word: ctl is int32 [S] in device memory, read by every launch of the call (so it is written ahead of
 * the call on the same stream, or otherwise ordered before it, and left alone until the call has completed); bits above 2 are ignored.
 * The state of all streams is one device buffer, 16-byte aligned: stream s has its two slots at s stream_stride and s stream_stride +
 * slot_stride, each [luma | out88 | pyr | mv | mvf] at the reported offsets, laid out inside as the single-frame buffers are (pyr as
 * fs_temporal_pyr_layout says; pyr_bytes is 0 at one level and mvf has no bytes at subpel 0).  A stream alternates FS_TS_SLOT from one of
 * its passes to the next; a skipped pass does not count. */
#define FS_TS_PREV 1 /* the stream has a previous frame, in the slot not written; clear: a first frame */
#define FS_TS_SLOT 2 /* the slot this pass writes is the second one; it reads the other */
#define FS_TS_SKIP 4 /* the stream does not take part: its workgroups return before their first access and before any barrier */

/* What fs_temporal_streams_layout reports; every offset and stride is a multiple of 16, stream_stride = 2 slot_stride, state_bytes = streams
 * stream_stride.  No implicit padding: 4 int32, then uint64. */
typedef struct fs_temporal_streams_info {
    int32_t streams, levels, subpel, reserved;
    uint64_t luma_offset, out88_offset, pyr_offset, mv_offset, mvf_offset;
    uint64_t slot_stride, stream_stride, state_bytes;
} fs_temporal_streams_info;

/* Host only: no HIP call, no global state, no allocation.  Errors: -1 null info, Ho or Wo below 1, streams outside [1, 64]; -2 levels outside
 * [1, 3], subpel outside [0, 2]. */
int fs_temporal_streams_layout(int Ho, int Wo, int levels, int subpel, int streams, fs_temporal_streams_info* info);

/* src [streams, H, W, 3], cur and dst [streams, Ho, Wo, 3] fp32.  The stream index comes from the grid and is bounded by `streams`.  No value
 * read from a tensor reaches an address except through the held vectors, as in the single-frame calls, and through the slot index
 * (ctl[s] >> 1) & 1, the only value from the control buffer that does, which the mask bounds: whatever ctl holds, every access lies inside
 * stream s's two slots.  Asynchronous on the ctx stream, allocates nothing, can be captured into a hipGraph (one graph serves every control
 * pattern: first frames, parities and skips are data).  A refused call launches nothing.  Errors: those of fs_temporal_obmc_f32 that do not
 * concern its state pointers; -1 streams outside [1, 64], null ctl or state, state_bytes below the layout's; -5 state not 16-byte aligned,
 * ctl not 4-byte aligned. */
int fs_temporal_streams_f32(fs_ctx* ctx, const float* src, int H, int W, const float* cur, int Ho, int Wo, int streams, int strength_q8,
                            int sensitivity, int radius, int levels, int subpel, int overlap, int matrix, int src_bgr, const int* ctl,
                            void* state, size_t state_bytes, float* dst);

/* ---- Resampling between fp32 tensors (csrc/fs_resample.hip): the net's (or composed, or stabilised) output at a delivery size, a deep
 * source's fp32 planes at the net's size; no u8 stage on either path.  The arithmetic below is the contract: it is Pillow's Image.resize on
 * mode-F images (double coefficients, double accumulation, a float32 result), and tests/test_resample.py restates it in numpy, holds the
 * restatement to Pillow and the kernel to the restatement, for equality.  A host-only plan, host-only tables, one asynchronous device call.
 *
 * Per axis, for the source length n_in, the destination length n_out and a filter f of support s:
 *   box       s = 0.5   f(x) = 1 for -0.5 < x <= 0.5
 *   bilinear  s = 1     f(x) = 1 - |x| for |x| < 1
 *   bicubic   s = 2     a = -0.5; |x| < 1: ((a + 2)|x| - (a + 3)) |x| |x| + 1; |x| < 2: (((|x| - 5)|x| + 8)|x| - 4) a
 *   lanczos   s = 3     sinc(x) sinc(x / 3) for -3 <= x < 3; sinc(0) = 1, otherwise sin(pi x) / (pi x) with pi x rounded first
 *   and f = 0 elsewhere.
 * Tables, all in double, every operation rounded on its own (no fused multiply-add):
 *   scale = n_in / n_out;  fscale = max(scale, 1);  support = s * fscale;  inv = 1 / fscale;  ksize = 2 * (int)ceil(support) + 1
 *   for the output index d:  center = (d + 0.5) * scale
 *     xmin = max(0, (int)(center - support + 0.5));  xmax = min(n_in, (int)(center + support + 0.5));  cnt = xmax - xmin
 *     w_k = f((k + xmin - center + 0.5) * inv) for k in [0, cnt);  ww = the sum of the w_k in order of k, from 0.0;  w_k = w_k / ww when ww != 0
 * A pass: out = (float)(sum over k of (double)in[xmin + k] * w_k), the sum from 0.0 in order of k, the product and the sum rounded separately.
 * The horizontal pass runs first and its result is rounded to float32; the vertical pass runs on those float32 values.  A pass whose axis
 * does not change length is skipped (not run with unit weights: NaN and infinities pass through it untouched).  Channels are independent.
 * Nothing is clamped: a bicubic overshoots a 0 | 255 step to about -19 and 274, and the output conversions clamp. */

#define FS_RESAMPLE_BOX 0
#define FS_RESAMPLE_BILINEAR 1
#define FS_RESAMPLE_BICUBIC 2
#define FS_RESAMPLE_LANCZOS 3
#define FS_RESAMPLE_TILE_W 64         /* destination columns of a workgroup's tile */
#define FS_RESAMPLE_LDS_ROWS 85       /* most source rows a tile keeps in LDS: 85 rows of 64 pixels of 3 float32 are 65280 bytes */

/* What fs_resample_plan reports.  The tables of the two axes share one buffer of table_bytes bytes, the x axis at x_offset and the y axis at
 * y_offset (multiples of 16): per output index 8 + 8 ksize bytes, {int32 xmin, int32 cnt} and then ksize doubles, w_k for k < cnt and 0.0 behind
 * them.  An axis that keeps its length has ksize 0 and no table; with both kept table_bytes is 0 and the call copies.
 * The kernel's geometry: one 256-thread workgroup per tile of FS_RESAMPLE_TILE_W destination columns by tile_h destination rows of one image;
 * tile_rows is the largest number of source rows the vertical taps of one tile span (tile_h when the y axis is kept), and tile_h is the largest
 * of 16, 8, 4, 2, 1 with tile_rows <= FS_RESAMPLE_LDS_ROWS; lds_rows (16, 40 or 85) is the row capacity of the kernel instance launched, the
 * smallest that holds tile_rows.  No implicit padding: 12 int32, then uint64. */
typedef struct fs_resample_info {
    int32_t src_h, src_w;
    int32_t dst_h, dst_w;
    int32_t filter;                    /* FS_RESAMPLE_* */
    int32_t x_ksize, y_ksize;          /* tap capacity per output index: 2 ceil(support) + 1; 0 for an axis that keeps its length */
    int32_t tile_w, tile_h;
    int32_t tile_rows, lds_rows;
    int32_t reserved;
    uint64_t x_offset, y_offset;
    uint64_t table_bytes;
} fs_resample_info;

/* Plans the resampling of src_h x src_w images to dst_h x dst_w.  Host only: no HIP call, no global state, no allocation.  Equal sizes are
 * taken and give a copy.  Errors: -1 null plan / a side outside [1, 32767]; -2 a filter other than the four above, or a vertical shrink one of
 * whose output rows takes more than FS_RESAMPLE_LDS_ROWS source rows (cnt > 85 on the y axis).  cnt is at most 2 s scale + 2, so a vertical
 * shrink by up to 83 (box), 41 (bilinear), 20 (bicubic) and 13 (lanczos) is always taken; the horizontal factor and any enlargement are
 * free. */
int fs_resample_plan(int src_h, int src_w, int dst_h, int dst_w, int filter, fs_resample_info* plan);

/* Writes the plan's tables into tables[0, plan->table_bytes), in the arithmetic above.  Host only.  Errors: -1 null argument (tables may be
 * null when table_bytes is 0) / a plan fs_resample_plan did not fill / cap < table_bytes, -5 tables not 8-byte aligned. */
int fs_resample_tables(const fs_resample_info* plan, void* tables, size_t cap);

/* Resamples N images of 3-channel fp32.  Image n starts at src + n * src_rows * src_pitch * 3 and its row y at + y * src_pitch * 3, with
 * src_rows >= src_h and src_pitch >= src_w: the top-left src_h x src_w of larger images is read and the margin never is.  dst is packed
 * [N, dst_h, dst_w, 3] and must not overlap src.  tables_dev: the device copy of what fs_resample_tables wrote (may be null when table_bytes is
 * 0).  Asynchronous on the ctx stream, allocates nothing, can be captured into a hipGraph.  The kernel clamps every table entry into the source
 * itself (xmin into [0, n_in - 1], cnt into [0, min(ksize, n_in - xmin)]) and every LDS row index into its array: a stale or wrong table gives
 * wrong pixels, nothing else.  A refused call launches nothing.
 * Errors: -1 null ctx / plan / src / dst, null tables_dev with table_bytes > 0, N outside [1, 65535], src_rows < src_h or src_pitch < src_w or
 * either above 32767, a plan fs_resample_plan did not fill, dst == src; -5 src or dst not 4-byte aligned, tables_dev not 16-byte aligned. */
int fs_resample_f32(fs_ctx* ctx, const fs_resample_info* plan, const void* tables_dev, const float* src, int src_rows, int src_pitch, int N,
                    float* dst);

/* ---- Guided delivery (csrc/fs_guided.hip): the net's (or composed, or stabilised) output at a larger delivery size with the edges of the
 * full-size source, by the fast guided filter (He & Sun): a local linear model output ~ a * luma(source) + b per channel on the net's grid,
 * a and b smoothed there, interpolated to the delivery grid and applied to the luma of the full-size source.  Three launches.  The arithmetic
 * below is the contract (tests/test_guided.py restates it in numpy and compares for equality); it is integer throughout, on compose's
 * unsigned 8.8 scale: to88, the luma weight triples, L(X) and the meaning of "bgr" are those of the fs_compose_f32 block above.  Every sum is
 * an integer sum, so the order of addition is free.
 *
 * Inputs per image: lo_src [H, W, 3] fp32, the net's input; lo_out [Ho, Wo, 3] fp32, the net's, composed or stabilised output, H <= Ho <= H + 3
 * and W <= Wo <= W + 3, of which only the top-left H x W is read; hi_src, the source at the delivery size Hd x Wd (Hd >= H, Wd >= W), of kind
 * 0: u8, 3 bytes per pixel; 1: u8, 4 bytes per pixel, the fourth ignored; 2: fp32, 3 floats per pixel.  Parameters: the radius r in [1, 8], n =
 * (2r + 1)^2; the smoothness E in [1, 64], in 8-bit levels; matrix 0 | 1; lo_bgr, hi_bgr 0 | 1: whether channel 0 of lo_src, respectively of
 * hi_src, is blue.  The channels of lo_out are treated alike, so its order does not matter.
 *
 * clampy(v) = min(max(v, 0), H - 1), clampx likewise with W.  The window of pixel (y, x) is {(clampy(y + j), clampx(x + i)) : |i|, |j| <= r},
 * with multiplicity, so always n terms.
 *
 *   coef       on the net's grid.  I = L(to88(lo_src)) under lo_bgr, in [0, 65280]; P_c = to88(lo_out[..c]).  Window sums in int64: S_I, S_II of
 *              I I, S_c of P_c, S_Ic of I P_c.
 *                V = n S_II - S_I^2 (never negative);  C_c = n S_Ic - S_I S_c;  D = V + n^2 E^2 65536
 *                a_c = (C_c 4096) / D;  b_c = (S_c 4096 - a_c S_I) / (256 n)
 *              both int64 divisions that truncate towards zero, as C++'s do.  |a_c| < 2^18 (|cov| <= sqrt(var_I var_P) and the
 *              arithmetic-geometric mean) and |b_c| < 2^27 (S_c 4096 / (256 n) <= 2^20, |a_c| S_I / (256 n) < 2^26), stored as int32:
 *              coef[H][W][6] = a_0 a_1 a_2 b_0 b_1 b_2.  a is Q12; b is 8.8 with four more fraction bits.
 *   mean       on the net's grid.  abar_c = (sum over the window of a_c) / n, bbar_c likewise, the sums in int64, the division truncating;
 *              mean[H][W][6] int32.
 *   apply      at output pixel (Y, X) of the delivery grid.  Vertical axis: ny = (2Y + 1) H - Hd;  y0 = floor(ny / (2 Hd)), which is -1 for the
 *              first rows of an enlargement;  fy = ((ny - y0 2 Hd) 256) / (2 Hd), in [0, 255]; the rows read are clampy(y0) and clampy(y0 + 1).
 *              ny, 2 Hd and the remainder times 256 fit int32 for every side up to 32767.  Horizontal axis: the same with X, W, Wd.  Weights
 *              (256 - fy)(256 - fx), (256 - fy) fx, fy (256 - fx), fy fx, which sum to 65536.  Ahat_c, Bhat_c: the weighted sums of the four
 *              abar_c, respectively bbar_c, in int64.  G = L(hi88) under hi_bgr, hi88 = to88(v) for kind 2 and v << 8 for the u8 kinds.
 *                F_c = clamp((Ahat_c G + (Bhat_c << 8) + 2^27) >> 28, 0, 65280), the shift arithmetic; the sum stays below 2^52
 *                dst = (float)F_c * 2^-8 (exact)
 * Hence: a constant lo_out of value v gives F = to88(v) everywhere, for every source, radius and smoothness (a = 0 and b = 16 to88(v)
 * exactly); a flat lo_src gives a = 0, so F is the bilinear interpolation of the window means of P; with Hd = H and Wd = W, fy = fx = 0 and
 * y0 = Y, so no interpolation takes place; a source that is NaN, below 0 or above 255 behaves as to88 says.  No value read from a tensor
 * reaches an address.
 * Not provided: a colour (three-channel) guide, coefficients on a grid coarser than the net's, delivery below the net's size. */

/* The workspace of fs_guided_f32 for N images on an H x W grid: coef [N, H, W, 6] int32 at offset 0, then mean [N, H, W, 6] int32 at offset
 * *bytes / 2; each part is N H W 24 bytes rounded up to a multiple of 16.  Host only.  Errors: -1 null bytes, N outside [1, 65535], H or W
 * outside [1, 32767]. */
int fs_guided_workspace(int H, int W, int N, size_t* bytes);

/* N images: lo_src [N, H, W, 3], lo_out [N, Ho, Wo, 3], hi_src [N, Hd, Wd, 3 | 4] of hi_kind, dst [N, Hd, Wd, 3] fp32; work: work_bytes >=
 * fs_guided_workspace's, both parts are written (and may be read back: the layout above).  Asynchronous on the ctx stream, allocates nothing,
 * can be captured into a hipGraph; grid.z (coef, mean) and grid.y (apply) are the image.  A refused call launches nothing.
 * Errors: -1 null argument, N outside [1, 65535], H or W below 1, Ho outside [H, H + 3] or Wo outside [W, W + 3], Hd or Wd above 32767, Hd < H or
 * Wd < W, work_bytes short, dst equal to lo_out, lo_src or hi_src; -2 radius outside [1, 8], smoothness outside [1, 64], hi_kind outside [0, 2],
 * matrix, lo_bgr or hi_bgr other than 0 or 1; -5 lo_src, lo_out, dst or an fp32 hi_src not 4-byte aligned, work not 16-byte aligned (Wd a
 * multiple of 4 with hi_src and dst 16-byte aligned takes 16-byte accesses, anything else single bytes and floats, with the same values). */
int fs_guided_f32(fs_ctx* ctx, const float* lo_src, int H, int W, const float* lo_out, int Ho, int Wo, const void* hi_src, int hi_kind, int Hd,
                  int Wd, int N, int radius, int smoothness, int matrix, int lo_bgr, int hi_bgr, void* work, size_t work_bytes, float* dst);

#ifdef __cplusplus
}
#endif
#endif
