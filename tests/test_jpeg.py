"""The library's baseline JPEG decoder (csrc/fs_jpeg.hip: host Huffman pass, device reconstruction) against PIL's decode of the same bytes --
equality, not a tolerance: the IJG arithmetic both implement is integer -- and against known answers that pin the coefficient layout; what it
does not take answers 1 and what is malformed answers a negative code without writing outside its buffer; the batcher's native path yields the
batches of the PIL path.  The same bodies run on the CPU emulator and, under -m gpu, on the MI355X."""
import ctypes
import io
import os

import numpy as np
import pytest
from PIL import Image, ImageFile

from faststyle_amd import _lib, datapipe, tfrecord
from tests.backends import engine_params, get_engine, on_emulator
from tests.test_datapipe import make_shards

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHICAGO = os.path.join(ROOT, "tests", "golden", "ref_assets", "chicago.jpg")
STARRY = os.path.join(ROOT, "style_images", "starry_night_crop.jpg")


@pytest.fixture(params=engine_params())
def eng(request):
    return get_engine(request.param)


def encode(arr, **kw):
    """PIL sizes the encoder's output buffer from width x height when optimize is set, which noise at 4:4:4 outgrows ("Suspension not allowed
    here"); a block that surely holds the file avoids it and leaves the bytes as they are."""
    buf = io.BytesIO()
    block = ImageFile.MAXBLOCK
    ImageFile.MAXBLOCK = max(block, 4 * arr.size + 65536)
    try:
        Image.fromarray(arr).save(buf, "JPEG", **kw)
    finally:
        ImageFile.MAXBLOCK = block
    return buf.getvalue()


def picture(kind, h, w, gray, seed):
    rng = np.random.default_rng(seed)
    c = () if gray else (3,)
    if kind == "random":
        return rng.integers(0, 256, (h, w) + c, dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    ramp = (yy[..., None] * rng.uniform(0.5, 3, 3) + xx[..., None] * rng.uniform(0.5, 3, 3) + rng.uniform(0, 120, 3)) % 256
    return (ramp[..., 0] if gray else ramp).astype(np.uint8)


def pil_decode(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def host_decode(eng, data):
    """(info, coefficient buffer) of a JPEG that must be in the handled set."""
    rc, info = eng.jpeg_parse(data)
    assert rc == 0, (rc, eng.lib.fs_last_error())
    coef = np.zeros(int(info.coef_bytes), dtype=np.uint8)
    rc = eng.jpeg_decode(data, info, coef.ctypes.data, coef.nbytes)
    assert rc == 0, (rc, eng.lib.fs_last_error())
    return info, coef


def reconstruct(eng, decoded, pixel_bytes):
    """[(info, coef)] through ONE fs_jpeg_reconstruct_many: the images [H,W,pixel_bytes] and whatever lies behind the last of them."""
    items = np.zeros(len(decoded), dtype=eng.JPEG_ITEM)
    coef_off = dst_off = 0
    for k, (info, coef) in enumerate(decoded):
        items[k] = eng.jpeg_item(info, coef_off, dst_off, pixel_bytes)
        coef_off += (coef.nbytes + 15) & ~15
        dst_off += (info.width * info.height * pixel_bytes + 15) & ~15
    staged = np.zeros(coef_off, dtype=np.uint8)
    for it, (info, coef) in zip(items, decoded):
        staged[int(it["coef_offset"]):int(it["coef_offset"]) + coef.nbytes] = coef
    rgb = eng.mem.upload_u8(np.full(dst_off + 32, 0xAB, dtype=np.uint8))
    eng.jpeg_reconstruct_many(eng.mem.upload_u8(staged), items, rgb)
    flat = np.asarray(eng.mem.to_numpy(rgb))
    out = []
    for it, (info, _) in zip(items, decoded):
        n = info.width * info.height * pixel_bytes
        out.append(flat[int(it["dst_offset"]):int(it["dst_offset"]) + n].reshape(info.height, info.width, pixel_bytes))
        pad = flat[int(it["dst_offset"]) + n:int(it["dst_offset"]) + ((n + 15) & ~15)]
        assert (pad == 0xAB).all()                       # nothing behind an image's last pixel is written
    assert (flat[dst_off:] == 0xAB).all()
    return out


def native_decode(eng, data, pixel_bytes=3):
    return reconstruct(eng, [host_decode(eng, data)], pixel_bytes)[0][:, :, :3]


# ------------------------------------------------------------------ 1. exactness against PIL
SIZES = [(8, 8), (16, 16), (1, 1), (17, 9), (37, 53), (64, 48)]
OPTIONS = [dict(), dict(optimize=True), dict(restart_marker_blocks=3), dict(optimize=True, restart_marker_blocks=3)]


@pytest.mark.parametrize("quality", [30, 75, 95, 100])
@pytest.mark.parametrize("sub", [0, 1, 2, "gray"])
def test_native_decode_equals_pil(eng, sub, quality):
    """Every image must be HANDLED (answer 0: host_decode asserts it), so equality cannot be met by handing files to PIL."""
    gray = sub == "gray"
    sizes = SIZES if on_emulator(eng) else SIZES + [(480, 640), (474, 712)]
    want_sampling = {0: (1, 1), 1: (2, 1), 2: (2, 2), "gray": (1, 1)}[sub]
    n = 0
    for h, w in sizes:
        for kind in ("random", "smooth"):
            for opt in (OPTIONS if h * w <= 64 * 64 else OPTIONS[:1] + OPTIONS[3:]):
                arr = picture(kind, h, w, gray, seed=1000 * h + w + quality)
                data = encode(arr, quality=quality, **(opt if gray else dict(opt, subsampling=sub)))
                info, coef = host_decode(eng, data)
                assert (info.width, info.height, info.ncomp) == (w, h, 1 if gray else 3) and (info.hs[0], info.vs[0]) == want_sampling
                assert (info.restart_interval > 0) == ("restart_marker_blocks" in opt)
                want = pil_decode(data)
                for pixel_bytes in ((3, 4) if n % 4 == 0 else (4,)):
                    got = reconstruct(eng, [(info, coef)], pixel_bytes)[0]
                    diff = int(np.abs(got[:, :, :3].astype(int) - want).max())
                    print("%dx%d %s sub=%s q=%d %s stride %d: max |native - PIL| = %d" % (h, w, kind, sub, quality, opt, pixel_bytes, diff))
                    assert np.array_equal(got[:, :, :3], want), (h, w, kind, sub, quality, opt, pixel_bytes, diff)
                n += 1
    assert n >= 48


def test_shipped_photograph_equals_pil(eng):
    data = open(CHICAGO, "rb").read()
    info, coef = host_decode(eng, data)
    assert (info.hs[0], info.vs[0], info.ncomp) == (2, 2, 3)
    got = reconstruct(eng, [(info, coef)], 4)[0]
    assert np.array_equal(got[:, :, :3], pil_decode(data))


# ------------------------------------------------------------------ 2. what the decoder does not take
def write_shard(path, jpegs):
    with tfrecord.RecordWriter(path) as w:
        for k, data in enumerate(jpegs):
            im = Image.open(io.BytesIO(data))
            w.write(tfrecord.encode_example({"image/encoded": data, "image/height": im.height, "image/width": im.width, "image/channels": 3,
                                             "image/colorspace": b"RGB", "image/format": b"JPEG", "image/filename": b"%d.jpg" % k}))
    return path


def not_handled():
    rng = np.random.default_rng(3)
    arr = picture("smooth", 40, 56, False, 5)
    cmyk = io.BytesIO()
    Image.frombytes("CMYK", (32, 24), rng.integers(0, 256, (24, 32, 4), dtype=np.uint8).tobytes()).save(cmyk, "JPEG", quality=90)
    return [encode(arr, quality=85, progressive=True), open(STARRY, "rb").read(), cmyk.getvalue()]


def test_unsupported_files_answer_one(eng):
    for data in not_handled():
        info = _lib.fs_jpeg_info()
        assert eng.lib.fs_jpeg_parse(data, len(data), ctypes.byref(info)) == 1
        guard = np.full(64, 0x5A, dtype=np.uint8)
        assert eng.lib.fs_jpeg_decode(data, len(data), ctypes.byref(info), ctypes.c_void_p(guard.ctypes.data + 16), 0) == 1
        assert (guard == 0x5A).all()


def collect(eng, files, **kw):
    it = datapipe.batcher(files, engine=eng, **kw)
    return [eng.mem.to_numpy(b).copy() for b in it], it


def test_unsupported_files_take_the_pil_path_through_the_batcher(eng, tmp_path):
    good = [encode(picture("smooth", 30 + 3 * k, 41 - 2 * k, False, k), quality=90, subsampling=k % 3) for k in range(5)]
    bad = not_handled()
    files = [write_shard(str(tmp_path / "train-00000-of-00002"), good[:2] + bad[:2] + good[2:3]),
             write_shard(str(tmp_path / "train-00001-of-00002"), bad[2:] + good[3:])]
    kw = dict(batch_size=2, resize_shape=(16, 20), num_epochs=2, min_after_dequeue=3, seed=4, num_threads=2)
    want, plain = collect(eng, files, prefetch=2, **kw)
    got, native = collect(eng, files, prefetch=2, jpeg="device", **kw)
    assert len(want) == 8 and len(got) == 8 and all(np.array_equal(a, b) for a, b in zip(got, want))
    assert (native.jpeg_handled, native.jpeg_fallback) == (10, 6) and (plain.jpeg_handled, plain.jpeg_fallback) == (0, 0)


# ------------------------------------------------------------------ 3. malformed input (host code only)
def decode_guarded(lib, data, guard=4096, emu=None):
    """fs_jpeg_parse + fs_jpeg_decode of arbitrary bytes with guard bytes around the output buffer: (parse answer, decode answer or None).
    emu: an EMULATOR engine -- a damaged file that still decodes is then reconstructed too (arbitrary coefficients through the kernels'
    arithmetic, for the sanitisers to watch); nothing damaged is ever sent to a GPU by these tests."""
    info = _lib.fs_jpeg_info()
    src = np.frombuffer(bytes(data), dtype=np.uint8).copy()         # an exact-size heap block: a read past n is the sanitiser's to see
    rc = lib.fs_jpeg_parse(ctypes.c_void_p(src.ctypes.data), src.size, ctypes.byref(info))
    if rc != 0:
        return rc, None
    assert 0 < info.coef_bytes < (1 << 26)
    buf = np.full(int(info.coef_bytes) + 2 * guard, 0xC3, dtype=np.uint8)
    rc2 = lib.fs_jpeg_decode(ctypes.c_void_p(src.ctypes.data), src.size, ctypes.byref(info), ctypes.c_void_p(buf.ctypes.data + guard), int(info.coef_bytes))
    assert (buf[:guard] == 0xC3).all() and (buf[guard + int(info.coef_bytes):] == 0xC3).all()
    if rc2 == 0 and emu is not None:
        coef = buf[guard:guard + int(info.coef_bytes)].copy()
        in_range = within_coding_range(info, coef)
        got = reconstruct(emu, [(info, coef)], 4)[0][:, :, :3]
        try:
            want = pil_decode(bytes(data))
        except OSError:                  # PIL does not open it (its test of the first marker is stricter than the format's)
            want = None
        if in_range and want is not None:
            assert np.array_equal(got, want)
    return rc, rc2


def within_coding_range(info, coef):
    """Whether every dequantised coefficient is one that the DCT of 8-bit samples can give: at most 8 x 128 = 1024 in magnitude, and half a
    quantisation step (<= 128) of rounding -- 2048 bounds it with room.  A file within that range that decodes is, to any decoder, a
    well-formed JPEG, and PIL's pixels are the reference for it as for an intended file.  Beyond it the values are no image's: libjpeg-turbo's
    vector inverse DCT keeps 16-bit lanes and wraps where the C arithmetic does not, so there is no one answer to be equal to, and what is
    checked is memory safety alone."""
    qt = coef[int(info.qt_offset):int(info.qt_offset) + 384].view(np.uint16).reshape(3, 64).astype(np.int64)
    for c in range(info.ncomp):
        n = info.blocks_x[c] * info.blocks_y[c] * 64
        plane = coef[int(info.plane_offset[c]):int(info.plane_offset[c]) + 2 * n].view(np.int16).reshape(-1, 64).astype(np.int64)
        if np.abs(plane * qt[c]).max() > 2048:
            return False
    return True


def scan_start(data):
    i = data.index(b"\xff\xda")
    return i + 2 + int.from_bytes(data[i + 2:i + 4], "big")


def malformed_cases(lib, emu=None):
    """Runs every damaged file; returns the number of cases.  Damage of three kinds:
      * truncation at seeded lengths: the scan of a complete file is followed by EOI, so every proper prefix is malformed;
      * structural damage at seeded places: a field set to a value the format does not allow or this decoder does not take, or a marker
        written into the scan (the scan then ends early).  Each is malformed or unsupported BY CONSTRUCTION, so the answer must be negative
        or 1;
      * seeded random byte changes in headers and scan.  A changed byte may leave a well-formed JPEG (a quantisation value, the magnitude
        bits of a coefficient): no decoder can tell that file from an intended one, so here answer 0 is legitimate too.  What is
        checked is that nothing is written outside the buffer, that the process survives and, on the emulator, that a file answering 0 whose
        coefficients are within what an encoder can produce (within_coding_range) decodes to PIL's pixels for the same bytes."""
    rng = np.random.default_rng(2024)
    files = [encode(picture("random", 37, 53, False, 1), quality=75, subsampling=2),
             encode(picture("smooth", 24, 40, False, 2), quality=95, subsampling=1, optimize=True, restart_marker_blocks=3),
             encode(picture("random", 16, 16, True, 3), quality=30)]
    n = 0
    for data in files:
        assert decode_guarded(lib, data) == (0, 0)
        s0 = scan_start(data)
        for cut in sorted(set(int(v) for v in rng.integers(0, len(data), 60)) | {0, 1, 2, 3, s0 - 1, s0, s0 + 1, len(data) - 2, len(data) - 1}):
            rc, rc2 = decode_guarded(lib, data[:cut])
            assert rc < 0 or rc == 1 or (rc == 0 and rc2 < 0), (cut, rc, rc2)
            n += 1
        sof = data.index(b"\xff\xc0")
        dht = data.index(b"\xff\xc4")
        dqt = data.index(b"\xff\xdb")
        sos = data.index(b"\xff\xda")
        structural = [(1, 0xD9), (sof + 1, 0xC2), (sof + 1, 0xC9), (sof + 2, 0xFF), (sof + 3, 0x02), (sof + 4, 12), (sof + 9, 2), (sof + 9, 4),
                      (sof + 11, 0x00), (sof + 11, 0x41), (sof + 12, 7), (dht + 2, 0xFF), (dht + 3, 0x01), (dht + 4, 0x25), (dht + 5, 0xFF),
                      (dqt + 3, 0x01), (dqt + 4, 0x35), (dqt + 4, 0x10), (sos + 4, 0), (sos + 4, 9), (sos + 6, 0x44)]
        for pos, val in structural:
            bad = bytearray(data)
            bad[pos] = val
            rc, rc2 = decode_guarded(lib, bad)
            assert rc < 0 or rc == 1 or (rc == 0 and (rc2 < 0 or rc2 == 1)), (pos, val, rc, rc2)
            n += 1
        for pos in rng.integers(s0, len(data) - 3, 40):
            for marker in (0xD9, 0xD8, 0xD3, 0xC4):
                bad = bytearray(data)
                bad[pos], bad[pos + 1] = 0xFF, marker
                if bad[pos:pos + 2] == data[pos:pos + 2]:
                    continue                                         # (the file's own restart marker)
                rc, rc2 = decode_guarded(lib, bad)
                assert rc == 0 and rc2 < 0, (int(pos), marker, rc, rc2)
                n += 1
        for _ in range(300):
            bad = bytearray(data)
            for pos in rng.integers(2, len(data), int(rng.integers(1, 4))):
                bad[pos] = int(rng.integers(0, 256))
            rc, rc2 = decode_guarded(lib, bad, emu=emu)
            assert rc <= 1 and (rc2 is None or rc2 <= 1)
            n += 1
    for junk in (b"", b"\xff", b"\xff\xd8", b"\xff\xd8\xff", b"\xff\xd8\xff\xd9", b"GIF89a" + bytes(40), bytes(rng.integers(0, 256, 500, dtype=np.uint8))):
        rc, _ = decode_guarded(lib, junk)
        assert rc < 0
        n += 1
    return n


def test_malformed_input_is_refused_without_touching_memory_outside_the_buffer(eng):
    """Host code: the same source in the emulator build and in the product library (whichever `eng` carries).  tests/test_jpeg_train.py runs the
    same cases against the emulator build under the address and undefined-behaviour sanitisers."""
    assert malformed_cases(eng.lib, eng if on_emulator(eng) else None) > 1200
    info = _lib.fs_jpeg_info()
    assert eng.lib.fs_jpeg_parse(None, 10, ctypes.byref(info)) == -1 and b"fs_jpeg_parse" in eng.lib.fs_last_error()
    data = encode(picture("smooth", 8, 8, False, 0), quality=75)
    _, coef = host_decode(eng, data)
    rc, info = eng.jpeg_parse(data)
    assert eng.jpeg_decode(data, info, coef.ctypes.data, coef.nbytes - 1) == -1                      # a buffer too small
    assert eng.jpeg_decode(data, info, coef.ctypes.data + 1, coef.nbytes) == -5
    other = encode(picture("smooth", 8, 16, False, 0), quality=75)
    assert eng.jpeg_decode(other, info, coef.ctypes.data, coef.nbytes) == -1                         # an info of another file


# ------------------------------------------------------------------ 4. known answer: the coefficient layout
@pytest.mark.parametrize("sub", [0, 1, 2])
def test_constant_colour_decodes_to_dc_only_blocks(eng, sub):
    """A constant image has no AC energy: every block is its DC term alone, quantised: round(8 (v - 128) / q) with q the table's first entry,
    v the component's constant value -- (Y, Cb, Cr) of the colour, which at 100 % quality (q = 1) is read back exactly.  24 x 40 pixels with
    2 x 2 sampling: 3 x 5 luma blocks padded to 4 x 6 (whole MCUs), 2 x 3 chroma blocks."""
    colour = np.array([200, 90, 40], dtype=np.uint8)
    data = encode(np.broadcast_to(colour, (24, 40, 3)).copy(), quality=100, subsampling=sub)
    info, coef = host_decode(eng, data)
    hs, vs = {0: (1, 1), 1: (2, 1), 2: (2, 2)}[sub]
    assert list(info.blocks_x) == [5 if hs == 1 else 6, 5 // hs + (1 if hs == 2 else 0), 5 // hs + (1 if hs == 2 else 0)]
    assert list(info.blocks_y) == [3 if vs == 1 else 4, 3 // vs + (1 if vs == 2 else 0), 3 // vs + (1 if vs == 2 else 0)]
    assert info.coef_count == 64 * sum(info.blocks_x[c] * info.blocks_y[c] for c in range(3))
    assert info.qt_offset == (2 * info.coef_count + 15) // 16 * 16 and info.coef_bytes == info.qt_offset + 384 and info.rgb_bytes == 24 * 40 * 3
    qt = coef[int(info.qt_offset):].view(np.uint16).reshape(3, 64)
    assert (qt == 1).all()                                                               # quality 100
    r, g, b = (float(v) for v in colour)
    ycc = [0.299 * r + 0.587 * g + 0.114 * b, -0.168736 * r - 0.331264 * g + 0.5 * b + 128, 0.5 * r - 0.418688 * g - 0.081312 * b + 128]
    for c in range(3):
        n = info.blocks_x[c] * info.blocks_y[c]
        assert info.plane_offset[c] == 128 * sum(info.blocks_x[k] * info.blocks_y[k] for k in range(c))
        blocks = coef[int(info.plane_offset[c]):int(info.plane_offset[c]) + 128 * n].view(np.int16).reshape(info.blocks_y[c], info.blocks_x[c], 64)
        assert not blocks[:, :, 1:].any()
        assert (blocks[:, :, 0] == 8 * (round(ycc[c]) - 128)).all(), (c, blocks[:, :, 0])
    got = native_decode(eng, data)
    assert np.array_equal(got, pil_decode(data)) and (np.abs(got.astype(int) - colour).max() <= 2) and (got == got[0, 0]).all()


def test_zigzag_order_is_undone(eng):
    """One cosine half-wave across an 8 x 8 grayscale block is one DCT basis function: varying along x it is coefficient (row 0, column 1) =
    natural index 1; varying along y it is (row 1, column 0) = natural index 8, which the zigzag scan visits third (a block left in scan order
    would hold it at index 2)."""
    x = np.arange(8)
    wave = (128 + 100 * np.cos((2 * x + 1) * np.pi / 16)).astype(np.uint8)
    for arr, where in ((np.tile(wave, (8, 1)), 1), (np.tile(wave[:, None], (1, 8)), 8)):
        data = encode(arr, quality=100)
        info, coef = host_decode(eng, data)
        blk = coef[:128].view(np.int16)
        assert abs(int(blk[where])) > 300 and abs(int(blk[9 - where])) <= 8 and abs(int(blk[2])) <= 8
        assert np.array_equal(native_decode(eng, data), pil_decode(data))


# ------------------------------------------------------------------ 5. reconstruct-many
def test_reconstruct_many_equals_the_single_image_calls(eng):
    specs = [(37, 53, 2, 75, dict(optimize=True)), (16, 24, "gray", 90, dict()), (9, 17, 1, 60, dict(restart_marker_blocks=3)), (64, 48, 0, 95, dict()),
             (1, 1, 2, 80, dict()), (3, 4, 1, 80, dict())]
    decoded, want = [], []
    for h, w, sub, q, opt in specs:
        gray = sub == "gray"
        data = encode(picture("random", h, w, gray, h + w), quality=q, **(opt if gray else dict(opt, subsampling=sub)))
        decoded.append(host_decode(eng, data))
        want.append(pil_decode(data))
    for pixel_bytes in (3, 4):
        singles = [reconstruct(eng, [d], pixel_bytes)[0] for d in decoded]
        many = reconstruct(eng, decoded, pixel_bytes)
        for k in range(len(specs)):
            assert np.array_equal(many[k], singles[k]) and np.array_equal(many[k][:, :, :3], want[k]), (k, pixel_bytes)


def test_reconstruct_many_refuses_bad_descriptors(eng):
    lib, ctx, mem = eng.lib, eng.ctx, eng.mem
    data = encode(picture("smooth", 16, 24, False, 1), quality=80, subsampling=2)
    info, coef_h = host_decode(eng, data)
    items = np.array([eng.jpeg_item(info, 0, 0, 4)], dtype=eng.JPEG_ITEM)
    coef = mem.upload_u8(np.concatenate([coef_h, np.zeros(16, np.uint8)]))
    rgb = mem.upload_u8(np.full(16 * 24 * 4 + 16, 0xAB, np.uint8))
    table = mem.upload_u8(np.concatenate([items.view(np.uint8), np.zeros(8, np.uint8)]))

    def run(it, K=1, dev=None, cb=coef_h.size, rb=16 * 24 * 4, c=None, r=None):
        return lib.fs_jpeg_reconstruct_many(ctx, mem.ptr_u8(coef) if c is None else c, cb, it.ctypes.data, mem.ptr_u8(table) if dev is None else dev, K,
                                            mem.ptr_u8(rgb) if r is None else r, rb)
    assert run(items, K=0) == -1 and b"fs_jpeg_reconstruct_many" in lib.fs_last_error()
    assert run(items, c=0) == -1 and run(items, r=0) == -1
    for field, value, code in [("pixel_bytes", 5, -2), ("pixel_bytes", 1, -2), ("coef_offset", 400, -1), ("coef_offset", 1 << 40, -1), ("qt_offset", coef_h.size, -1),
                               ("dst_offset", 16, -1), ("dst_offset", 1 << 40, -1), ("width", 0, -1), ("height", 70000, -1), ("width", 25, -1), ("ncomp", 2, -1),
                               ("hs", 3, -1), ("vs", 0, -1), ("coef_offset", 8, -5), ("qt_offset", int(info.qt_offset) + 2, -5), ("dst_offset", 2, -5)]:
        bad = items.copy()
        bad[field] = value
        assert run(bad) == code, (field, value)
        assert b"image 0" in lib.fs_last_error()
    assert run(items, dev=mem.ptr_u8(table) + 4) == -5 and run(items, c=mem.ptr_u8(coef) + 8) == -5 and run(items, r=mem.ptr_u8(rgb) + 2) == -5
    assert run(items, cb=coef_h.size - 1) == -1 and run(items, rb=16 * 24 * 4 - 1) == -1
    assert (np.asarray(mem.to_numpy(rgb)) == 0xAB).all()                                   # no refused call launched anything
    assert run(items) == 0
    got = np.asarray(mem.to_numpy(rgb))
    assert np.array_equal(got[:16 * 24 * 4].reshape(16, 24, 4)[:, :, :3], pil_decode(data)) and (got[16 * 24 * 4:] == 0xAB).all()


# ------------------------------------------------------------------ 6. the batcher
@pytest.mark.parametrize("depth", [1, 2])
def test_native_batcher_yields_the_batches_of_the_pil_batcher(eng, tmp_path, depth):
    files, _ = make_shards(tmp_path, [5, 4, 6])
    for cut in (None, 4):
        kw = dict(batch_size=3, resize_shape=(16, 20), num_epochs=2, min_after_dequeue=4, seed=5, num_threads=2, max_batches=cut, prefetch=depth)
        want, _ = collect(eng, files, **kw)
        got, it = collect(eng, files, jpeg="device", **kw)
        assert len(want) == (10 if cut is None else cut) and len(got) == len(want)
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
        assert it.jpeg_fallback == 0 and (it.jpeg_handled == 30 if cut is None else 0 < it.jpeg_handled <= 30)


def test_native_batcher_through_small_arena_chunks_and_staging_pieces(eng, tmp_path, monkeypatch):
    """Chunks of a few images (an _issue's images straddle chunks, chunks are recycled) and a staging cap that flushes the fill phase."""
    files, _ = make_shards(tmp_path, [9, 8])
    kw = dict(batch_size=2, resize_shape=(16, 20), num_epochs=3, min_after_dequeue=6, seed=9, num_threads=2, prefetch=2)
    want, _ = collect(eng, files, **kw)
    monkeypatch.setattr(datapipe.CoefArena, "CHUNK_BYTES", 20000)            # an image here: 2.7 - 6.5 KB of coefficients
    monkeypatch.setattr(datapipe.FedQueue, "STAGE_CAP_BYTES", 15000)
    got, it = collect(eng, files, jpeg="device", **kw)
    assert len(got) == len(want) == 25 and all(np.array_equal(a, b) for a, b in zip(got, want))
    assert (it.jpeg_handled, it.jpeg_fallback) == (51, 0)


def test_native_path_needs_the_fed_path(eng, tmp_path):
    files, _ = make_shards(tmp_path, [3])
    with pytest.raises(_lib.FaststyleError, match="prefetch > 0"):
        next(datapipe.batcher(files, 1, (16, 20), engine=eng, jpeg="device"))
    with pytest.raises(_lib.FaststyleError, match="jpeg must be"):
        next(datapipe.batcher(files, 1, (16, 20), engine=eng, prefetch=2, jpeg="gpu"))
