"""Deep YUV4MPEG2 streams (faststyle_amd/y4m.py with deep=True): the tags of 9 to 16 bits per sample, their refusal by name without the
option, frames of 16-bit words through a pipe, and the writer's deep headers.  Host code only."""
import io
import os
import threading

import numpy as np
import pytest

from faststyle_amd import y4m
from tests.test_yuv import host_lib

HEAD = "YUV4MPEG2 W7 H5 F30:1 Ip A1:1 %s\n"
# prefix -> (sampling, siting, components, samples of a 7 x 5 frame)
FAMILIES = {"C420p": ((2, 2), 0, 3, 35 + 2 * 4 * 3), "C422p": ((2, 1), 1, 3, 35 + 2 * 4 * 5), "C444p": ((1, 1), 0, 3, 3 * 35), "Cmono": ((1, 1), 0, 1, 35)}
DEEP_TAGS = ["%s%d" % (p, n) for p in FAMILIES for n in range(9, 17)]


@pytest.mark.parametrize("tag", DEEP_TAGS)
def test_every_deep_tag_is_taken_when_asked_for(tag):
    prefix, bits = tag[:5], int(tag[5:])
    sampling, siting, components, samples = FAMILIES[prefix]
    f = y4m.parse_header((HEAD % tag).encode(), deep=True)
    assert (f.width, f.height, f.sampling, f.siting, f.components, f.bits, f.frame_bytes) == (7, 5, sampling, siting, components, bits, 2 * samples)
    assert f.colourspace == tag[1:] and f.rate == (30, 1) and f.aspect == (1, 1) and f.full_range is False and f[-1] == bits
    assert y4m.parse_header((HEAD % (tag + " XCOLORRANGE=FULL")).encode(), deep=True).full_range is True
    assert y4m.Reader(io.BytesIO((HEAD % tag).encode()), deep=True).format == f


@pytest.mark.parametrize("tag", DEEP_TAGS)
def test_every_deep_tag_is_refused_by_name_without_the_option(tag):
    for call in (lambda: y4m.parse_header((HEAD % tag).encode()), lambda: y4m.parse_header((HEAD % tag).encode(), deep=False),
                 lambda: y4m.Reader(io.BytesIO((HEAD % tag).encode()))):
        with pytest.raises(y4m.Y4MError) as e:
            call()
        assert tag in str(e.value) and "deep=True" in str(e.value) and "--video_depth stream" in str(e.value)


@pytest.mark.parametrize("tag", ["C420p8", "C420p17", "C444p8", "Cmono8", "Cmono17", "C422p100", "C420p010", "C420p", "C411p10", "C444alpha", "C444alpha10",
                                 "C420jpeg10", "C420mpeg2p10"])
@pytest.mark.parametrize("deep", [False, True])
def test_tags_that_are_refused_either_way(tag, deep):
    with pytest.raises(y4m.Y4MError) as e:
        y4m.parse_header((HEAD % tag).encode(), deep=deep)
    assert tag in str(e.value) and "deep=True" not in str(e.value)


def test_eight_bit_streams_read_the_same_with_the_option():
    for tag in ("C420jpeg", "C420", "C420mpeg2", "C420paldv", "C422", "C444", "Cmono", ""):
        a, b = y4m.parse_header((HEAD % tag).encode()), y4m.parse_header((HEAD % tag).encode(), deep=True)
        assert a == b and a.bits == 8 and a.frame_bytes == y4m.frame_bytes(7, 5, a.sampling, a.components)
    assert y4m.Format._fields[-1] == "bits" and y4m.Format._fields[-2] == "frame_bytes"


@pytest.mark.parametrize("buffered", [True, False])
def test_deep_writer_to_reader_through_a_pipe(buffered):
    """A non-seekable stream and frames larger than the pipe's capacity; the writer's header comes from a descriptor of fs_yuv_plan_deep."""
    W, H = 320, 180
    desc = host_lib().yuv_plan(W, H, sampling=(2, 2), siting=0, full_range=True, bits=10)
    n = int(desc.frame_bytes)
    assert n == y4m.frame_bytes(W, H, (2, 2), 3, 10) == 2 * y4m.frame_bytes(W, H, (2, 2), 3)
    frames = [np.random.RandomState(k).randint(0, 1024, n // 2).astype("<u2") for k in range(3)]
    rfd, wfd = os.pipe()

    def produce():
        with os.fdopen(wfd, "wb", -1 if buffered else 0) as f:
            w = y4m.Writer(f, desc, rate=(24000, 1001), aspect=(4, 3))
            assert w.bits == 10 and w.frame_bytes == n
            for fr in frames:
                w.write_frame(fr.view(np.uint8))
            w.flush()

    t = threading.Thread(target=produce)
    t.start()
    got = []
    with os.fdopen(rfd, "rb", -1 if buffered else 0) as f:
        r = y4m.Reader(f, deep=True)
        buf = np.zeros((1, n), np.uint8)
        while r.read_frame_into(buf):
            got.append(buf[0].copy().view("<u2"))
    t.join()
    fm = r.format
    assert (fm.width, fm.height, fm.sampling, fm.siting, fm.components, fm.full_range, fm.rate, fm.aspect, fm.bits, fm.colourspace) == \
        (W, H, (2, 2), 0, 3, True, (24000, 1001), (4, 3), 10, "420p10")
    assert len(got) == 3 and all(np.array_equal(g, f) for g, f in zip(got, frames))


def test_truncation_inside_a_deep_frame():
    head = (HEAD % "Cmono12").encode()
    frame = b"FRAME\n" + bytes(70)
    r = y4m.Reader(io.BytesIO(head + frame + frame[:-1]), deep=True)
    buf = bytearray(70)
    assert r.read_frame_into(buf) is True
    with pytest.raises(y4m.Y4MError) as e:
        r.read_frame_into(buf)
    assert "ends after 69 of 70" in str(e.value)
    r = y4m.Reader(io.BytesIO(head + frame), deep=True)
    with pytest.raises(y4m.Y4MError):
        r.read_frame_into(bytearray(35))                                                       # the 8-bit size of such a frame
    assert r.read_frame_into(buf) is True and r.read_frame_into(buf) is False


def test_deep_headers_of_the_writer():
    h = host_lib()

    def head(**kw):
        b = io.BytesIO()
        y4m.Writer(b, h.yuv_plan(8, 6, **kw), rate=(25, 1))
        return b.getvalue()

    assert head(bits=10) == b"YUV4MPEG2 W8 H6 F25:1 Ip C420p10 XCOLORRANGE=LIMITED\n"
    assert head(bits=8) == head() == b"YUV4MPEG2 W8 H6 F25:1 Ip C420jpeg XCOLORRANGE=LIMITED\n"
    assert b" C422p12 " in head(sampling=(2, 1), siting=1, bits=12) and b" C444p16 " in head(sampling=(1, 1), bits=16)
    assert b" Cmono9 " in head(sampling=(1, 1), components=1, bits=9) and b"XCOLORRANGE=FULL" in head(bits=14, full_range=True)
    for kw in (dict(siting=1, bits=10), dict(sampling=(2, 1), siting=0, bits=10)):            # no deep tag says co-sited 4:2:0 or centre-sited 4:2:2
        with pytest.raises(y4m.Y4MError):
            head(**kw)
    for bits in (7, 17, 0):
        with pytest.raises(y4m.Y4MError):
            y4m.header(8, 6, bits=bits)
    for kw in (dict(bits=10), dict(sampling=(2, 1), siting=1, bits=12), dict(sampling=(1, 1), bits=16), dict(sampling=(1, 1), components=1, bits=9)):
        d = h.yuv_plan(7, 5, **kw)                                                             # every header the writer writes reads back
        b = io.BytesIO()
        w = y4m.Writer(b, d)
        f = y4m.parse_header(b.getvalue(), deep=True)
        assert (f.width, f.height, f.sampling, f.components, f.siting, f.bits, f.frame_bytes) == \
            (7, 5, (d.hs, d.vs), d.ncomp, d.siting, kw["bits"], d.frame_bytes) and w.frame_bytes == d.frame_bytes
