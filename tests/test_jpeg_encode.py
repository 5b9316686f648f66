"""The library's baseline JPEG encoder (csrc/fs_jpegenc.hip: device colour conversion / downsampling / forward DCT / quantisation, host Huffman
pass) against PIL's encoding of the same pixels -- equality of the file bytes, not a tolerance: the IJG arithmetic both implement is integer --
and against the library's own decoder, which pins the coefficient layout and the tables independently of PIL; what the calls refuse answers the
documented code without writing outside its buffer; the stylizers' jpeg= option and stylize_webcam.py --output_format jpg give PIL's bytes of
the frames they give without it.  The same bodies run on the CPU emulator and, under -m gpu, on the MI355X."""
import ctypes
import io
import os

import numpy as np
import pytest
from PIL import Image

from faststyle_amd import _lib, ckpt, stream
from oracle import tnet
from tests.backends import engine_params, get_engine, on_emulator
from tests.test_aux_scripts import f64
from tests.test_jpeg import encode, host_decode, picture, pil_decode, reconstruct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHICAGO = os.path.join(ROOT, "tests", "golden", "ref_assets", "chicago.jpg")
SAMPLING = {0: (1, 1), 1: (2, 1), 2: (2, 2), "gray": (1, 1)}
GUARD = 64


@pytest.fixture(params=engine_params())
def eng(request):
    return get_engine(request.param)


def pil_encode(arr, quality, sub):
    return encode(arr, quality=quality) if sub in ("gray", None) else encode(arr, quality=quality, subsampling=sub)


def make_picture(kind, h, w, gray, seed):
    """random / smooth as in tests/test_jpeg.py; extreme1 / extreme8: a 0 / 255 checkerboard of period 1 / 8 (the largest coefficients)."""
    if kind.startswith("extreme"):
        p = int(kind[7:])
        yy, xx = np.mgrid[0:h, 0:w]
        board = ((((yy // p) + (xx // p)) & 1) * 255).astype(np.uint8)
        return board if gray else np.repeat(board[:, :, None], 3, axis=2).copy()
    return picture(kind, h, w, gray, seed)



def forward(eng, jobs):
    """jobs [(pixels [H,W] or [H,W,3], quality, sub, pixel_bytes)] through ONE fs_jpeg_forward_many, the coefficient regions separated (and
    followed) by 0xAB guard bytes: [(info, coefficient buffer)].  Checks the guards and that the source buffer is unchanged."""
    plans, srcs, items = [], [], np.zeros(len(jobs), dtype=eng.JPEGENC_ITEM)
    src_off = coef_off = 0
    for k, (arr, quality, sub, pixel_bytes) in enumerate(jobs):
        h, w = arr.shape[:2]
        rc, info = eng.jpeg_encode_plan(w, h, 1 if arr.ndim == 2 else 3, *SAMPLING[sub])
        assert rc == 0, (rc, eng.lib.fs_last_error())
        if pixel_bytes == 4:                                     # RGBX with a fourth byte that must not matter
            arr = np.concatenate([arr, np.full((h, w, 1), 0x5A + k, np.uint8)], axis=2)
        assert arr.shape[2:] == ((pixel_bytes,) if pixel_bytes > 1 else ())
        items[k] = eng.jpegenc_item(info, src_off, coef_off + GUARD, pixel_bytes, quality)
        plans.append(info)
        srcs.append((src_off, arr.reshape(-1)))
        src_off += (arr.size + 15) & ~15
        coef_off += GUARD + int(info.coef_bytes)
    staged = np.zeros(src_off, dtype=np.uint8)
    for off, flat in srcs:
        staged[off:off + flat.size] = flat
    src = eng.mem.upload_u8(staged)
    coef = eng.mem.upload_u8(np.full(coef_off + GUARD, 0xAB, dtype=np.uint8))
    eng.jpeg_forward_many(src, items, coef)
    flat = np.array(eng.mem.to_numpy(coef), copy=True)
    assert np.array_equal(np.asarray(eng.mem.to_numpy(src)), staged)                  # the source pixels are never written
    out, end = [], 0
    for it, info in zip(items, plans):
        o = int(it["coef_offset"])
        assert (flat[end:o] == 0xAB).all()
        end = o + int(info.coef_bytes)
        out.append((info, flat[o:end].copy()))
    assert (flat[end:] == 0xAB).all() and flat.size - end == GUARD
    return out


def write(eng, info, coef):
    data = eng.jpeg_write_bytes(info, coef)
    assert eng.jpeg_write_bound(info) >= len(data)
    return data


def native_encode(eng, arr, quality, sub, pixel_bytes=None):
    (info, coef), = forward(eng, [(arr, quality, sub, pixel_bytes or (1 if arr.ndim == 2 else 3))])
    return write(eng, info, coef)


# ------------------------------------------------------------------ 1. the bytes PIL writes
SIZES = [(8, 8), (16, 16), (1, 1), (17, 9), (37, 53), (64, 48)]
QUALITIES = [5, 30, 75, 95, 100]
KINDS = ["random", "smooth", "extreme1", "extreme8"]


@pytest.mark.parametrize("sub", [0, 1, 2, "gray"])
def test_native_encode_equals_pil(eng, sub):
    gray = sub == "gray"
    sizes = SIZES if on_emulator(eng) else SIZES + [(480, 640), (474, 712)]
    n = 0
    worst = 0.0
    for h, w in sizes:
        for quality in QUALITIES:
            for kind in KINDS:
                arr = make_picture(kind, h, w, gray, seed=1000 * h + w + quality)
                want = pil_encode(arr, quality, sub)
                for pixel_bytes in ((1,) if gray else (3, 4) if n % 3 == 0 else (3,) if n % 3 == 1 else (4,)):
                    (info, coef), = forward(eng, [(arr, quality, sub, pixel_bytes)])
                    got = write(eng, info, coef)
                    worst = max(worst, len(got) / eng.jpeg_write_bound(info))
                    assert got == want, (h, w, kind, sub, quality, pixel_bytes, len(got), len(want))
                n += 1
    print("sub=%s: %d files equal PIL's; the largest fills %.3f of fs_jpeg_write_bound" % (sub, n, worst))
    assert n >= 100


def test_pil_default_subsampling_is_420(eng):
    """Image.save(..., quality=95) with no subsampling argument: what utils.imwrite writes."""
    arr = picture("smooth", 37, 53, False, seed=5)
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, "JPEG", quality=95)
    assert native_encode(eng, arr, 95, 2) == buf.getvalue()


def test_write_bound_holds_noise_at_full_quality(eng):
    """Random noise at q = 100, 4:4:4 is the longest file of a size."""
    arr = picture("random", 64, 48, False, seed=9)
    (info, coef), = forward(eng, [(arr, 100, 0, 3)])
    data = write(eng, info, coef)
    assert data == pil_encode(arr, 100, 0) and len(data) <= eng.jpeg_write_bound(info)


# ------------------------------------------------------------------ 2. the layout is the decoder's
@pytest.mark.parametrize("sub", [0, 1, 2, "gray"])
def test_written_file_decodes_to_the_same_buffer(eng, sub):
    gray = sub == "gray"
    for h, w in [(1, 1), (17, 9), (37, 53)]:
        arr = picture("smooth", h, w, gray, seed=h + w)
        (plan, coef), = forward(eng, [(arr, 75, sub, 1 if gray else 3)])
        data = write(eng, plan, coef)
        info, decoded = host_decode(eng, data)                   # (asserts answer 0 of fs_jpeg_parse and fs_jpeg_decode)
        for name, _ in _lib.fs_jpeg_info._fields_:
            if name == "scan_offset":
                continue
            a, b = getattr(info, name), getattr(plan, name)
            assert (list(a), name) == (list(b), name) if hasattr(a, "__len__") else (a, name) == (b, name)
        assert plan.scan_offset == 0 and plan.restart_interval == 0
        assert np.array_equal(decoded, coef)
        got = reconstruct(eng, [(info, decoded)], 4)[0]
        assert np.array_equal(got[:, :, :3], pil_decode(data))


# ------------------------------------------------------------------ 3. several images in one launch
def test_many_images_in_one_launch(eng):
    jobs = [(picture("random", 17, 9, False, seed=1), 95, 2, 3),
            (picture("smooth", 37, 53, False, seed=2), 30, 1, 4),
            (picture("random", 8, 24, True, seed=3), 75, "gray", 1),
            (picture("smooth", 64, 48, False, seed=4), 100, 0, 4),
            (picture("random", 1, 1, False, seed=5), 5, 2, 3),
            (picture("random", 33, 16, False, seed=6), 60, 2, 4)]
    many = forward(eng, jobs)                                    # (guards and source checked inside)
    for job, (info, coef) in zip(jobs, many):
        (info1, coef1), = forward(eng, [job])
        assert np.array_equal(coef, coef1)
        assert write(eng, info, coef) == write(eng, info1, coef1) == pil_encode(job[0], job[1], job[2])


# ------------------------------------------------------------------ 4. the shipped photograph
def test_shipped_photograph_equals_pil(eng):
    arr = np.asarray(Image.open(CHICAGO).convert("RGB"))
    assert native_encode(eng, arr, 95, 2) == pil_encode(arr, 95, 2)


# ------------------------------------------------------------------ 5. refusals
def test_forward_refusals(eng):
    lib, ctx, mem = eng.lib, eng.ctx, eng.mem
    arr = picture("random", 17, 9, False, seed=1)
    rc, info = eng.jpeg_encode_plan(9, 17, 3, 2, 2)
    assert rc == 0
    src = mem.upload_u8(np.concatenate([arr, np.zeros((17, 9, 1), np.uint8)], axis=2).reshape(-1))       # 612 bytes: fits 3- and 4-byte pixels
    nsrc = 17 * 9 * 4
    coef = mem.upload_u8(np.full(int(info.coef_bytes) + 32, 0xAB, dtype=np.uint8))
    ncoef = int(info.coef_bytes)
    good = np.array([eng.jpegenc_item(info, 0, 0, 3, 95)], dtype=eng.JPEGENC_ITEM)
    table = mem.upload_u8(np.concatenate([good.view(np.uint8).reshape(-1), np.zeros(8, np.uint8)]))
    assert eng.JPEGENC_ITEM.itemsize == 56

    def run(it=good, K=1, s=None, sb=nsrc, c=None, cb=ncoef, dev=None, host=True):
        return lib.fs_jpeg_forward_many(ctx, mem.ptr_u8(src) if s is None else s, sb, it.ctypes.data if host else None,
                                        mem.ptr_u8(table) if dev is None else dev, K, mem.ptr_u8(coef) if c is None else c, cb)

    def changed(**kw):
        it = good.copy()
        for k, v in kw.items():
            it[0][k] = v
        return it

    assert run(K=0) == -1 and b"fs_jpeg_forward_many" in lib.fs_last_error()
    assert run(K=65536) == -1
    assert run(host=False) == -1 and run(s=0) == -1 and run(c=0) == -1 and run(dev=0) == -1
    assert lib.fs_jpeg_forward_many(None, mem.ptr_u8(src), nsrc, good.ctypes.data, mem.ptr_u8(table), 1, mem.ptr_u8(coef), ncoef) == -1
    for kw in (dict(width=0), dict(height=0), dict(width=65536), dict(ncomp=2), dict(hs=3), dict(hs=1, vs=2), dict(vs=0)):
        assert run(changed(**kw)) == -1, kw
    assert run(changed(ncomp=1, pixel_bytes=1)) == -1            # one component sampled 2x2
    assert run(sb=17 * 9 * 3 - 1) == -1 and run(cb=ncoef - 1) == -1
    assert run(changed(src_offset=nsrc - 17 * 9 * 3 + 1)) == -1
    assert run(changed(coef_offset=400)) == -1 and run(changed(qt_offset=ncoef - 384 + 16)) == -1
    for kw in (dict(pixel_bytes=2), dict(pixel_bytes=1), dict(pixel_bytes=5), dict(quality=0), dict(quality=101)):
        assert run(changed(**kw)) == -2, kw
    assert run(changed(ncomp=1, hs=1, vs=1, pixel_bytes=3)) == -2
    assert run(dev=mem.ptr_u8(table) + 4) == -5
    assert run(c=mem.ptr_u8(coef) + 8) == -5
    assert run(changed(coef_offset=8)) == -5 and run(changed(qt_offset=int(info.qt_offset) + 8)) == -5
    assert run(changed(pixel_bytes=4, src_offset=2)) == -5
    assert (np.asarray(mem.to_numpy(coef)) == 0xAB).all()        # argument checks: nothing was launched
    assert run() == 0 and run(changed(pixel_bytes=4)) == 0
    flat = np.asarray(mem.to_numpy(coef))
    assert (flat[ncoef:] == 0xAB).all() and not (flat[:ncoef] == 0xAB).all()


def test_forward_refuses_a_misaligned_rgbx_source(eng):
    lib, ctx, mem = eng.lib, eng.ctx, eng.mem
    rc, info = eng.jpeg_encode_plan(8, 8, 3, 1, 1)
    src = mem.upload_u8(np.zeros(8 * 8 * 4 + 16, np.uint8))
    coef = mem.upload_u8(np.full(int(info.coef_bytes), 0xAB, dtype=np.uint8))
    it = np.array([eng.jpegenc_item(info, 0, 0, 4, 95)], dtype=eng.JPEGENC_ITEM)
    table = mem.upload_u8(it.view(np.uint8).reshape(-1))
    assert lib.fs_jpeg_forward_many(ctx, mem.ptr_u8(src) + 2, 8 * 8 * 4, it.ctypes.data, mem.ptr_u8(table), 1, mem.ptr_u8(coef), int(info.coef_bytes)) == -5
    assert (np.asarray(mem.to_numpy(coef)) == 0xAB).all()


def test_host_refusals(eng):
    lib = eng.lib
    info = _lib.fs_jpeg_info()
    for args in ((0, 8, 3, 2, 2), (8, 0, 3, 2, 2), (65536, 8, 3, 1, 1), (8, 65536, 3, 1, 1), (8, 8, 2, 1, 1), (8, 8, 4, 1, 1), (8, 8, 3, 1, 2),
                 (8, 8, 3, 3, 1), (8, 8, 3, 2, 3), (8, 8, 1, 2, 2), (8, 8, 1, 2, 1)):
        assert lib.fs_jpeg_encode_plan(*args, ctypes.byref(info)) == -1, args
    assert lib.fs_jpeg_encode_plan(8, 8, 3, 2, 2, None) == -1 and b"fs_jpeg_encode_plan" in lib.fs_last_error()
    assert lib.fs_jpeg_encode_plan(65535, 65535, 3, 2, 2, ctypes.byref(info)) == 0 and lib.fs_jpeg_write_bound(ctypes.byref(info)) > 0
    assert lib.fs_jpeg_write_bound(None) == 0

    arr = picture("random", 17, 9, False, seed=3)
    (info, coef), = forward(eng, [(arr, 95, 2, 3)])
    data = write(eng, info, coef)
    assert data == pil_encode(arr, 95, 2)
    n = ctypes.c_size_t(0)
    aligned = np.zeros(coef.size + 16, dtype=np.uint8)           # a 2-byte aligned home for the coefficients, and an odd one
    base = aligned.ctypes.data + (aligned.ctypes.data & 1)
    ctypes.memmove(base, coef.ctypes.data, coef.size)

    def run(cap, info_=info, addr=base, nbytes=coef.size, out=True, count=True):
        buf = np.full(len(data) + 2 * GUARD, 0xAB, dtype=np.uint8)
        rc = lib.fs_jpeg_write(ctypes.byref(info_) if info_ is not None else None, ctypes.c_void_p(addr), nbytes,
                               ctypes.c_void_p(buf.ctypes.data + GUARD) if out else None, cap, ctypes.byref(n) if count else None)
        assert (buf[:GUARD] == 0xAB).all() and (buf[GUARD + min(cap, len(data)):] == 0xAB).all(), cap
        return rc, buf[GUARD:GUARD + len(data)].tobytes()

    header = data.index(b"\xff\xda") + 14                        # SOS segment of three components: marker + 12
    for cap in (0, 1, header - 1, header, len(data) - 1):
        rc, _ = run(cap)
        assert rc == -3 and b"fs_jpeg_write" in lib.fs_last_error(), cap
    rc, got = run(len(data))
    assert rc == 0 and got == data and n.value == len(data)
    assert run(len(data), info_=None)[0] == -1 and run(len(data), addr=0)[0] == -1 and run(len(data), out=False)[0] == -1
    assert run(len(data), count=False)[0] == -1
    assert run(len(data), nbytes=coef.size - 1)[0] == -1
    assert run(len(data), addr=base + 1)[0] == -5
    other = _lib.fs_jpeg_info()
    ctypes.memmove(ctypes.byref(other), ctypes.byref(info), ctypes.sizeof(other))
    other.mcu_x += 1
    assert run(len(data), info_=other)[0] == -1                  # an info fs_jpeg_encode_plan did not fill

    # hand-made coefficients outside the baseline range
    def with_coef(index, value):
        c = coef.copy()
        c[:int(info.coef_count) * 2].view("<i2")[:] = 0
        c[:int(info.coef_count) * 2].view("<i2")[index] = value
        ctypes.memmove(base, c.ctypes.data, c.size)
        return run(len(data) + GUARD)[0]

    assert with_coef(0, 2047) == 0 and with_coef(0, 2048) == -4 and with_coef(0, -2048) == -4          # a DC step of 2048: category 12
    assert with_coef(64, 2047) == 0                              # (the second block's step is -2047)
    assert with_coef(5, 1023) == 0 and with_coef(5, 1024) == -4 and with_coef(63, -1024) == -4          # an AC value of 1024: category 11
    c = coef.copy()
    c[int(info.qt_offset):int(info.qt_offset) + 2] = 0           # a quantisation entry of 0
    ctypes.memmove(base, c.ctypes.data, c.size)
    assert run(len(data) + GUARD)[0] == -1


# ------------------------------------------------------------------ 6. the stylizers
def starry(eng):
    P = tnet.strip_scope(ckpt.load_checkpoint(os.path.join(ROOT, "models", "starry_final.ckpt")))
    return P, eng.mem.from_numpy(eng.flatten_params(P, scope=""))


def check_against_oracle(frame, P, out):
    """tests/test_aux_scripts.py::test_frame_stylizer_matches_reference_loop_body: the jpeg=None path is the parent's."""
    want = tnet.create_net(frame[np.newaxis].astype(np.float64), f64(P))[0].astype(np.uint8)[:, :, ::-1]
    diff = np.abs(out.astype(int) - want.astype(int))
    assert out.shape == want.shape and diff.max() <= 1 and (diff > 0).mean() < 2e-3


def test_frame_stylizer_returns_pil_bytes(eng):
    """Eager on the emulator (48 x 56: not a multiple of 16 either way), the captured graph at 96 x 136 on the GPU."""
    H, W = (48, 56) if on_emulator(eng) else (96, 136)
    P, variables = starry(eng)
    rng = np.random.default_rng(2)
    frames = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(1 if on_emulator(eng) else 2)]
    plain = stream.FrameStylizer(eng, variables, H, W, use_graph=not on_emulator(eng))
    again = stream.FrameStylizer(eng, variables, H, W, use_graph=not on_emulator(eng), jpeg=None)
    st = stream.FrameStylizer(eng, variables, H, W, use_graph=not on_emulator(eng), jpeg=dict(quality=90, subsampling=1))
    for k, frame in enumerate(frames):
        want = plain(frame)
        assert want.dtype == np.uint8 and np.array_equal(want, again(frame))
        if k == 0:
            check_against_oracle(frame, P, want)
        got = st(frame)                                          # (the second frame replays the captured graph on the GPU)
        assert isinstance(got, bytes) and got == pil_encode(want, 90, 1)
    assert st.jpeg == dict(quality=90, subsampling=1) and plain.jpeg is None
    with pytest.raises(_lib.FaststyleError):
        stream.FrameStylizer(eng, variables, H, W, jpeg=dict(quality=0))
    for s in (plain, again, st):
        s.release()


@pytest.mark.gpu
def test_frame_stylizer_batch_returns_a_list():
    eng = get_engine("hip")
    H, W = 48, 56
    _, variables = starry(eng)
    frames = np.random.default_rng(3).integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    plain = stream.FrameStylizer(eng, variables, H, W, batch=2, swap_rb=False, use_graph=False)
    st = stream.FrameStylizer(eng, variables, H, W, batch=2, swap_rb=False, use_graph=False, jpeg=dict(), jpeg_threads=2)
    want, got = plain(frames), st(frames)
    assert isinstance(got, list) and got == [pil_encode(want[b], 95, 2) for b in range(2)]
    for s in (plain, st):
        s.release()


@pytest.mark.gpu
def test_pipelined_stylizer_returns_pil_bytes_in_order():
    eng = get_engine("hip")
    H, W = 96, 136
    _, variables = starry(eng)
    rng = np.random.default_rng(4)
    frames = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(5)]
    plain = stream.PipelinedStylizer(eng, variables, H, W, depth=2)
    single = stream.FrameStylizer(eng, variables, H, W)
    ps = stream.PipelinedStylizer(eng, variables, H, W, depth=2, jpeg=dict(quality=95, subsampling=2), jpeg_threads=2)
    want = list(plain.run(frames))
    assert all(np.array_equal(w, single(f)) for w, f in zip(want, frames))            # jpeg=None: the frames of the existing path
    got = list(ps.run(frames))
    assert len(got) == 5 and all(isinstance(g, bytes) for g in got)
    assert got == [pil_encode(w, 95, 2) for w in want]
    assert len({g for g in got}) == 5                            # five distinct frames: an order mix-up cannot pass
    for s in (plain, single, ps):
        s.release()


# ------------------------------------------------------------------ 7. command line
@pytest.mark.gpu
def test_frames_dir_writes_jpg(tmp_path):
    import stylize_webcam
    fd = tmp_path / "frames"
    fd.mkdir()
    for k in range(3):
        Image.fromarray(picture("smooth", 56, 72, False, seed=20 + k)).save(str(fd / ("f%02d.png" % k)))
    common = ["--model_path", os.path.join(ROOT, "models", "starry_final.ckpt"), "--frames_dir", str(fd)]
    parser = stylize_webcam.setup_parser()
    default = parser.parse_args(common + ["--output_dir", str(tmp_path / "png")])
    assert (default.output_format, default.output_quality) == ("png", 95)
    stylize_webcam.run_frames_dir(default)
    stylize_webcam.run_frames_dir(parser.parse_args(common + ["--output_dir", str(tmp_path / "jpg"), "--output_format", "jpg", "--output_quality", "90"]))
    assert sorted(os.listdir(str(tmp_path / "png"))) == ["f00.png", "f01.png", "f02.png"]               # the default run writes only .png
    assert sorted(os.listdir(str(tmp_path / "jpg"))) == ["f00.jpg", "f01.jpg", "f02.jpg"]
    for k in range(3):
        pixels = np.asarray(Image.open(str(tmp_path / "png" / ("f%02d.png" % k))))
        assert pixels.shape == (56, 72, 3)
        assert open(str(tmp_path / "jpg" / ("f%02d.jpg" % k)), "rb").read() == pil_encode(pixels, 90, 2)
