"""YUV4MPEG2 ("Y4M") streams: the raw video container that ``ffmpeg -f yuv4mpegpipe``, x264, mpv and others read and write on pipes.

A stream is one text header line

    YUV4MPEG2 W<width> H<height> F<num>:<den> I<interlacing> A<num>:<den> C<colour space> X<extension> ...\\n

(tags in any order, only W and H required) and then, per frame, the line ``FRAME`` (optionally followed by parameters, which are ignored) and
the frame's planes: Y, then Cb, then Cr, 8 bits per sample, no padding -- exactly the layout of include/faststyle_io.h's fs_yuv_desc, so a
frame goes from the stream into a lane's pinned staging buffer with one ``readinto`` and from there to the device as it is.

Taken: ``C420jpeg``, a bare ``C420`` and a missing C tag (4:2:0, chroma sited at the centre of its 2x2 cell), ``C420mpeg2`` and ``C420paldv``
(4:2:0, chroma horizontally co-sited with the even luma column; paldv's vertical chroma offset of half a line is ignored: its chroma rows are
treated as mpeg2's), ``C422`` (co-sited), ``C444``, ``Cmono``; ``XCOLORRANGE=FULL`` / ``=LIMITED`` (default limited); progressive streams
(``Ip``, ``I?`` or no I tag).  Refused, with a message that names the tag: bit depths above 8 (``C420p10`` ...), ``C411``, ``C444alpha``,
interlaced streams (``It``, ``Ib``, ``Im``).  Host code only; it needs neither the library nor a device."""
import collections

MAGIC = b"YUV4MPEG2"
FRAME = b"FRAME"
MAX_LINE = 4096          # a header or frame line longer than this is not a Y4M stream

# C tag -> (sampling (hs, vs), siting, components)
COLOURSPACES = {
    "420jpeg": ((2, 2), 0, 3), "420": ((2, 2), 0, 3), "420mpeg2": ((2, 2), 1, 3), "420paldv": ((2, 2), 1, 3),
    "422": ((2, 1), 1, 3), "444": ((1, 1), 0, 3), "mono": ((1, 1), 0, 1),
}


class Y4MError(ValueError):
    pass


Format = collections.namedtuple("Format", "width height sampling siting components full_range rate aspect colourspace frame_bytes")
Format.__doc__ = """What a stream's header says: sampling (hs, vs), siting 0 centre / 1 co-sited, components 3 / 1, rate and aspect as (num, den)
(None where the header has no such tag), the C tag as written (None: absent), and the bytes of one frame's planes."""


def frame_bytes(width, height, sampling, components):
    hs, vs = sampling
    if components == 1:
        return width * height
    return width * height + 2 * ((width + hs - 1) // hs) * ((height + vs - 1) // vs)


def _ratio(tag, text):
    try:
        num, den = text.split(":")
        return int(num), int(den)
    except ValueError:
        raise Y4MError("Y4M header: tag %s%s is not <num>:<den>" % (tag, text))


def parse_header(line):
    """The Format of a header line (bytes, with or without the newline)."""
    try:
        fields = line.decode("ascii").split()
    except UnicodeDecodeError:
        raise Y4MError("not a YUV4MPEG2 stream: the header is not ASCII")
    if not fields or fields[0] != MAGIC.decode():
        raise Y4MError("not a YUV4MPEG2 stream: the header begins %r" % line[:16])
    width = height = rate = aspect = cs = None
    full = False
    for f in fields[1:]:
        tag, text = f[0], f[1:]
        if tag in "WH":
            try:
                v = int(text)
            except ValueError:
                v = 0
            if v < 1:
                raise Y4MError("Y4M header: tag %s is not a positive size" % f)
            if tag == "W":
                width = v
            else:
                height = v
        elif tag == "F":
            rate = _ratio(tag, text)
        elif tag == "A":
            aspect = _ratio(tag, text)
        elif tag == "I":
            if text not in ("p", "?"):
                raise Y4MError("Y4M header: tag %s: interlaced streams are not taken (progressive only)" % f)
        elif tag == "C":
            if text not in COLOURSPACES:
                why = "alpha planes are not taken" if "alpha" in text else "4:1:1 is not taken" if text == "411" else \
                    "bit depths above 8 are not taken" if text[:4] == "mono" or (text[:3] in ("420", "422", "444") and text[3:4] == "p") else \
                    "unknown colour space"
                raise Y4MError("Y4M header: tag %s: %s" % (f, why))
            cs = text
        elif tag == "X":
            if text.startswith("COLORRANGE="):
                value = text[len("COLORRANGE="):]
                if value not in ("FULL", "LIMITED"):
                    raise Y4MError("Y4M header: tag %s: the range is FULL or LIMITED" % f)
                full = value == "FULL"
        else:
            raise Y4MError("Y4M header: unknown tag %s" % f)
    if width is None or height is None:
        raise Y4MError("Y4M header: no W or no H tag in %r" % line[:80])
    sampling, siting, components = COLOURSPACES[cs or "420jpeg"]
    return Format(width, height, sampling, siting, components, full, rate, aspect, cs, frame_bytes(width, height, sampling, components))


def _read_line(f, what):
    """One line of ``f`` without its newline (readline: a buffered object keeps what it read ahead for the readinto calls that follow, a raw one
    reads byte by byte); None at the end of the stream."""
    line = f.readline(MAX_LINE + 1)
    if line and not line.endswith(b"\n"):
        if len(line) > MAX_LINE:
            raise Y4MError("%s: no newline within %d bytes" % (what, MAX_LINE))
        raise Y4MError("%s: the stream ends inside the line %r" % (what, line[:32]))
    return line[:-1] if line else None


def _write_all(f, view):
    """f.write of the whole view: a raw (unbuffered) object may take less than it is given."""
    while len(view):
        k = f.write(view)
        if k is None or k >= len(view):
            return
        view = view[k:]


class Reader(object):
    """Frames of a YUV4MPEG2 stream from any binary file object -- a pipe or ``sys.stdin.buffer`` as well: nothing seeks.

        r = Reader(f)                        # reads the header: r.format
        while r.read_frame_into(buf): ...    # buf: a writable buffer of r.format.frame_bytes bytes (a lane's pinned staging)
    """

    def __init__(self, f):
        self.f = f
        line = _read_line(f, "Y4M header")
        if line is None:
            raise Y4MError("not a YUV4MPEG2 stream: it is empty")
        self.format = parse_header(line)
        self.frames = 0

    def read_frame_into(self, buffer):
        """Fills ``buffer`` with the next frame's planes; False on a clean end of stream (at a frame boundary).  Raises Y4MError for a bad
        frame line or a stream that ends inside a frame."""
        view = memoryview(buffer).cast("B")
        n = self.format.frame_bytes
        if len(view) != n:
            raise Y4MError("a frame of this stream is %d bytes, the buffer holds %d" % (n, len(view)))
        line = _read_line(self.f, "Y4M frame %d" % self.frames)
        if line is None:
            return False
        if line[:len(FRAME)] != FRAME or line[len(FRAME):len(FRAME) + 1] not in (b"", b" "):
            raise Y4MError("Y4M frame %d: expected FRAME, found %r" % (self.frames, line[:16]))
        got = 0
        while got < n:
            k = self.f.readinto(view[got:])
            if not k:
                raise Y4MError("Y4M frame %d: the stream ends after %d of %d bytes" % (self.frames, got, n))
            got += k
        self.frames += 1
        return True


def header(width, height, sampling=(2, 2), siting=0, components=3, full_range=False, rate=None, aspect=None):
    """The header line of a stream of such frames (bytes, with the newline): progressive; the C tag by sampling and siting (420jpeg, 420mpeg2,
    422, 444, mono; the format has no tag for centre-sited 4:2:2, which is refused); XCOLORRANGE always written, so that a reader need not know
    the default."""
    sampling = tuple(int(v) for v in sampling)
    if components == 1:
        cs = "mono"
    else:
        cs = {((2, 2), 0): "420jpeg", ((2, 2), 1): "420mpeg2", ((2, 1), 1): "422", ((1, 1), 0): "444", ((1, 1), 1): "444"}.get(
            (sampling, int(siting)))
        if cs is None or components != 3:
            raise Y4MError("no Y4M colour space for sampling %r, siting %r, %r components" % (sampling, siting, components))
    fields = ["YUV4MPEG2", "W%d" % width, "H%d" % height]
    if rate is not None:
        fields.append("F%d:%d" % tuple(rate))
    fields.append("Ip")
    if aspect is not None:
        fields.append("A%d:%d" % tuple(aspect))
    fields += ["C" + cs, "XCOLORRANGE=" + ("FULL" if full_range else "LIMITED")]
    return (" ".join(fields) + "\n").encode("ascii")


class Writer(object):
    """Writes a stream: the header from a frame descriptor (an fs_yuv_desc, or anything with width, height, hs, vs, ncomp, siting, full_range)
    plus frame rate and aspect, then frames from buffers of frame_bytes bytes."""

    def __init__(self, f, desc, rate=None, aspect=None):
        self.f = f
        self.frame_bytes = frame_bytes(int(desc.width), int(desc.height), (int(desc.hs), int(desc.vs)), int(desc.ncomp))
        f.write(header(int(desc.width), int(desc.height), (int(desc.hs), int(desc.vs)), int(desc.siting), int(desc.ncomp), bool(desc.full_range),
                       rate, aspect))
        self.frames = 0

    def write_frame(self, buffer):
        view = memoryview(buffer).cast("B")
        if len(view) != self.frame_bytes:
            raise Y4MError("a frame of this stream is %d bytes, the buffer holds %d" % (self.frame_bytes, len(view)))
        _write_all(self.f, memoryview(b"FRAME\n"))
        _write_all(self.f, view)
        self.frames += 1

    def flush(self):
        self.f.flush()
