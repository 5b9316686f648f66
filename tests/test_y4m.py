"""The YUV4MPEG2 container (faststyle_amd/y4m.py): header variants, every refused tag, frames through a pipe, clean and unclean ends of a
stream.  Host code only."""
import io
import os
import threading

import numpy as np
import pytest

from faststyle_amd import y4m


class Desc(object):
    """What y4m.Writer reads of a frame descriptor (the fields of fs_yuv_desc)"""

    def __init__(self, width, height, hs=2, vs=2, ncomp=3, siting=0, full_range=0):
        self.width, self.height, self.hs, self.vs, self.ncomp, self.siting, self.full_range = width, height, hs, vs, ncomp, siting, full_range


def test_a_hand_written_stream_is_read_sample_for_sample():
    # 4 x 2, 4:2:0: 8 luma samples, two Cb, two Cr per frame; the second frame line carries parameters
    data = b"YUV4MPEG2 W4 H2 F30000:1001 Ip A1:1 C420jpeg XYSCSS=420JPEG\n" \
           b"FRAME\n" + bytes([10, 11, 12, 13, 20, 21, 22, 23, 99, 100, 200, 201]) + \
           b"FRAME Ip Xwhatever\n" + bytes([0, 255, 0, 255, 10, 10, 10, 10, 128, 10, 128, 10])        # (a sample that is 10 = '\n' is data, not a line end)
    r = y4m.Reader(io.BytesIO(data))
    f = r.format
    assert (f.width, f.height, f.sampling, f.siting, f.components, f.full_range) == (4, 2, (2, 2), 0, 3, False)
    assert (f.rate, f.aspect, f.colourspace, f.frame_bytes) == ((30000, 1001), (1, 1), "420jpeg", 12)
    buf = np.zeros(12, np.uint8)
    assert r.read_frame_into(buf) is True and buf.tolist() == [10, 11, 12, 13, 20, 21, 22, 23, 99, 100, 200, 201]
    assert r.read_frame_into(buf) is True and buf.tolist() == [0, 255, 0, 255, 10, 10, 10, 10, 128, 10, 128, 10]
    assert r.read_frame_into(buf) is False and r.frames == 2
    assert buf.tolist() == [0, 255, 0, 255, 10, 10, 10, 10, 128, 10, 128, 10]                          # the end of the stream writes nothing


@pytest.mark.parametrize("header,want", [
    (b"YUV4MPEG2 W6 H4", ((2, 2), 0, 3, False, None, None, None, 36)),                       # no C tag: 4:2:0, centre
    (b"YUV4MPEG2 H4 C420 W6", ((2, 2), 0, 3, False, None, None, "420", 36)),                 # tag order, a bare C420
    (b"YUV4MPEG2 W5 H3 C420mpeg2 F25:1", ((2, 2), 1, 3, False, (25, 1), None, "420mpeg2", 15 + 2 * 3 * 2)),
    (b"YUV4MPEG2 W5 H3 C420paldv I?", ((2, 2), 1, 3, False, None, None, "420paldv", 27)),
    (b"YUV4MPEG2 XCOLORRANGE=FULL W5 H3 C422 A128:117", ((2, 1), 1, 3, True, None, (128, 117), "422", 15 + 2 * 3 * 3)),
    (b"YUV4MPEG2 W5 H3 C444 XCOLORRANGE=LIMITED XOTHER=1", ((1, 1), 0, 3, False, None, None, "444", 45)),
    (b"YUV4MPEG2 W5 H3 Cmono Ip F0:0", ((1, 1), 0, 1, False, (0, 0), None, "mono", 15)),
])
def test_header_variants(header, want):
    for line in (header, header + b"\n"):
        f = y4m.parse_header(line)
        assert (f.sampling, f.siting, f.components, f.full_range, f.rate, f.aspect, f.colourspace, f.frame_bytes) == want


@pytest.mark.parametrize("tag", ["C420p10", "C422p10", "C444p12", "C420p16", "Cmono16", "C411", "C444alpha", "It", "Ib", "Im"])
def test_refused_tags_are_named(tag):
    with pytest.raises(y4m.Y4MError) as e:
        y4m.Reader(io.BytesIO(("YUV4MPEG2 W8 H8 F25:1 %s\nFRAME\n" % tag).encode() + bytes(96)))
    assert tag in str(e.value)


@pytest.mark.parametrize("data", [b"", b"RIFF....AVI LIST", b"YUV4MPEG2 W8\n", b"YUV4MPEG2 W8 H0\n", b"YUV4MPEG2 W8 Hx\n", b"YUV4MPEG2 W8 H8 F25\n",
                                  b"YUV4MPEG2 W8 H8 XCOLORRANGE=WIDE\n", b"YUV4MPEG2 W8 H8 Q1\n", b"YUV4MPEG2 W8 H8", b"YUV4MPEG2 " + b"X" * 5000 + b"\n",
                                  b"YUV4MPEG\xff W8 H8\n"])
def test_what_is_not_a_header_raises(data):
    with pytest.raises(y4m.Y4MError):
        y4m.Reader(io.BytesIO(data))


def test_truncated_frames_and_bad_magic_raise_a_clean_end_does_not():
    head = b"YUV4MPEG2 W4 H2 Cmono\n"
    frame = b"FRAME\n" + bytes(range(8))
    buf = bytearray(8)
    for tail in (b"FRAME\n" + bytes(5), b"FRAME\n", b"FRA", b"FRAMES\n" + bytes(8), b"frame\n" + bytes(8), b"\n", bytes(8)):
        r = y4m.Reader(io.BytesIO(head + frame + tail))
        assert r.read_frame_into(buf) is True and bytes(buf) == bytes(range(8))
        with pytest.raises(y4m.Y4MError):
            r.read_frame_into(buf)
    r = y4m.Reader(io.BytesIO(head + frame))
    assert r.read_frame_into(buf) is True and r.read_frame_into(buf) is False and r.read_frame_into(buf) is False
    r = y4m.Reader(io.BytesIO(head))                                                           # a stream without frames is a stream
    assert r.read_frame_into(buf) is False
    with pytest.raises(y4m.Y4MError):
        y4m.Reader(io.BytesIO(head + frame)).read_frame_into(bytearray(9))                     # a buffer of another size


@pytest.mark.parametrize("buffered", [True, False])
def test_writer_to_reader_through_a_pipe(buffered):
    """A non-seekable stream, frames larger than the pipe's capacity, so that reads and writes come back short"""
    W, H = 640, 360
    desc = Desc(W, H, 2, 2, 3, siting=1, full_range=1)
    n = y4m.frame_bytes(W, H, (2, 2), 3)
    frames = [np.random.RandomState(k).randint(0, 256, n).astype(np.uint8) for k in range(3)]
    rfd, wfd = os.pipe()

    def produce():
        with os.fdopen(wfd, "wb", -1 if buffered else 0) as f:
            w = y4m.Writer(f, desc, rate=(24000, 1001), aspect=(4, 3))
            for fr in frames:
                w.write_frame(fr)
            w.flush()
            assert w.frames == 3

    t = threading.Thread(target=produce)
    t.start()
    got = []
    with os.fdopen(rfd, "rb", -1 if buffered else 0) as f:
        assert not f.seekable()
        r = y4m.Reader(f)
        buf = np.zeros((1, n), np.uint8)                                                       # (a lane's staging is [1, frame_bytes])
        while r.read_frame_into(buf):
            got.append(buf[0].copy())
    t.join()
    fm = r.format
    assert (fm.width, fm.height, fm.sampling, fm.siting, fm.components, fm.full_range, fm.rate, fm.aspect) == (W, H, (2, 2), 1, 3, True, (24000, 1001), (4, 3))
    assert len(got) == 3 and all(np.array_equal(g, f) for g, f in zip(got, frames))


def test_writer_headers():
    def head(desc, **kw):
        b = io.BytesIO()
        y4m.Writer(b, desc, **kw)
        return b.getvalue()

    assert head(Desc(8, 6)) == b"YUV4MPEG2 W8 H6 Ip C420jpeg XCOLORRANGE=LIMITED\n"
    assert head(Desc(8, 6, siting=1, full_range=1), rate=(25, 1), aspect=(1, 1)) == b"YUV4MPEG2 W8 H6 F25:1 Ip A1:1 C420mpeg2 XCOLORRANGE=FULL\n"
    assert b" C422 " in head(Desc(8, 6, 2, 1, siting=1)) and b" C444 " in head(Desc(8, 6, 1, 1)) and b" Cmono " in head(Desc(8, 6, 1, 1, ncomp=1))
    for desc in (Desc(8, 6, 2, 1, siting=0), Desc(8, 6, 4, 1), Desc(8, 6, 2, 2, ncomp=2)):     # no tag says centre-sited 4:2:2, 4:1:1 is not written
        with pytest.raises(y4m.Y4MError):
            head(desc)
    b = io.BytesIO()
    w = y4m.Writer(b, Desc(4, 2, 1, 1, ncomp=1))
    with pytest.raises(y4m.Y4MError):
        w.write_frame(bytes(7))
    for desc in (Desc(7, 5), Desc(7, 5, 2, 1, siting=1), Desc(7, 5, 1, 1), Desc(7, 5, 1, 1, ncomp=1)):     # every header the writer writes reads back
        f = y4m.parse_header(head(desc, rate=(30, 1)))
        assert (f.width, f.height, f.sampling, f.components, f.siting, f.rate) == (7, 5, (desc.hs, desc.vs), desc.ncomp, desc.siting, (30, 1))
