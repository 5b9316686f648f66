"""Device-fed input path (csrc/fs_feed.hip, datapipe.DeviceRing / FedQueue): the three kernels against restatements that do not share their
code (a numpy Philox4x32-10 checked against the published Random123 vectors, oracle.datapipe.resize_bicubic_tf1, ShuffleQueue.dequeue_many),
and the fed batcher against datapipe.batcher -- same batches, bit for bit, in the same order.  The same bodies run on the CPU emulator and, under
-m gpu, on the MI355X."""
import ctypes

import numpy as np
import pytest

from faststyle_amd import _lib, datapipe
from oracle import datapipe as odp
from tests.backends import engine_params, get_engine, on_emulator
from tests.test_datapipe import make_shards

M32 = np.uint64(0xFFFFFFFF)


@pytest.fixture(params=engine_params())
def eng(request):
    return get_engine(request.param)


# ------------------------------------------------------------------ fs_synth_uniform
def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 of Salmon et al. (SC'11) restated on uint64 arrays: counters c0..c3 (arrays or ints), key k0, k1 (ints)."""
    c0, c1, c2, c3 = (np.atleast_1d(np.asarray(c, dtype=np.uint64)) for c in (c0, c1, c2, c3))
    k0, k1 = int(k0), int(k1)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0, c1, c2, c3


def synth_restated(n, seed, rank, batch_index):
    blocks = (n + 3) // 4
    t = np.arange(blocks, dtype=np.uint64)
    one = np.ones(blocks, dtype=np.uint64)
    w = np.stack(philox4x32_10(t, one * np.uint64(batch_index & 0xFFFFFFFF), one * np.uint64(batch_index >> 32), one * np.uint64(rank),
                               seed & 0xFFFFFFFF, seed >> 32), axis=1).reshape(-1)[:n]
    u = (w >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return u * np.float32(255.0)


def test_philox_restatement_gives_the_published_answers():
    """Random123's kat_vectors for philox4x32 with 10 rounds."""
    f = 0xFFFFFFFF
    for ctr, key, want in [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
                           ((f, f, f, f), (f, f), "408f276d 41c83b0e a20bc7c6 6d5451fd"),
                           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")]:
        got = philox4x32_10(*ctr, *key)
        assert " ".join("%08x" % int(v[0]) for v in got) == want


def test_synth_known_answer_blocks_through_the_kernel(eng):
    """The kernel's block with counter (0,0,0,0), key (0,0) holds the first published vector under the value mapping (which keeps the top 24
    bits of each word); element block 2^32 - 1 is out of reach of a small call, so the all-ones vector is approached through rank, batch
    index and seed all-ones at block 0 against the restatement, which holds the published answers."""
    out = eng.mem.empty((4,))
    eng.synth_uniform(out, 0, 0, 0)
    words = np.array([0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8], dtype=np.uint64)
    want = (words >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24) * np.float32(255.0)
    assert np.array_equal(eng.mem.to_numpy(out), want)
    eng.synth_uniform(out, 2 ** 64 - 1, 2 ** 32 - 1, 2 ** 64 - 1)
    assert np.array_equal(eng.mem.to_numpy(out), synth_restated(4, 2 ** 64 - 1, 2 ** 32 - 1, 2 ** 64 - 1))


@pytest.mark.parametrize("seed", [1234, 0xDEADBEEF12345678])
@pytest.mark.parametrize("rank", [0, 3])
def test_synth_batch_equals_the_restatement(eng, seed, rank):
    shape = (2, 16, 20, 3) if on_emulator(eng) else (4, 64, 64, 3)
    n = int(np.prod(shape))
    seen = []
    for bi in (0, 1, 2 ** 32 + 5):
        out = eng.mem.empty(shape)
        eng.synth_uniform(out, seed, rank, bi)
        got = eng.mem.to_numpy(out).reshape(-1).copy()
        assert np.array_equal(got, synth_restated(n, seed, rank, bi)), bi
        seen.append(got)
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])


def test_synth_tail_and_range(eng):
    for n in (1, 5, 1023):                                   # n % 4 != 0: the last block stores element by element
        out = eng.mem.zeros((n + 3,))
        view = eng.mem.view(out, 0, (n,))
        eng.synth_uniform(view, 7, 1, 9)
        got = eng.mem.to_numpy(out)
        assert np.array_equal(got[:n], synth_restated(n, 7, 1, 9)) and not got[n:].any()      # nothing behind the end is written
    n = 100000 if on_emulator(eng) else 1000000
    out = eng.mem.empty((n,))
    eng.synth_uniform(out, 1234, 0, 3)
    v = eng.mem.to_numpy(out)
    assert v.min() >= 0.0 and v.max() < 255.0 and abs(float(v.astype(np.float64).mean()) - 127.5) < 0.5
    # the largest value the mapping can give
    assert np.float32(0xFFFFFF) * np.float32(2.0 ** -24) * np.float32(255.0) < np.float32(255.0)


# ------------------------------------------------------------------ fs_resize_bicubic_u8x_many
def stage(images):
    """(staged bytes, RESIZE_ITEM rows without dst_row): the images back to back, 16-byte aligned."""
    from faststyle_amd.engine import Engine
    items = np.zeros(len(images), dtype=Engine.RESIZE_ITEM)
    off, parts = 0, []
    for k, im in enumerate(images):
        items[k] = (off, im.shape[0], im.shape[1], im.shape[2], 0)
        pad = (-im.nbytes) % 16
        parts.append(np.concatenate([im.reshape(-1), np.full(pad, 0xAB, np.uint8)]))
        off += im.nbytes + pad
    return np.concatenate(parts), items


def test_resize_many_is_bit_exact_per_row(eng):
    rng = np.random.default_rng(11)
    Ho, Wo = 9, 1
    shapes = [(37, 53, 3), (19, 23, 4), (9, 1, 3), (5, 4, 3), (64, 48, 4)]           # packed and RGBX mixed; an identity resize; 5x4 -> 9x1
    images = [rng.integers(0, 256, s, dtype=np.uint8) for s in shapes]               # (garbage in the fourth byte of the RGBX ones)
    rows = [6, 0, 3, 7, 2]
    staged, items = stage(images)
    items["dst_row"] = rows
    store = eng.mem.from_numpy(np.full((8, Ho, Wo, 3), np.nan, np.float32))            # poisoned
    eng.resize_bicubic_u8_many(eng.mem.upload_u8(staged), items, store)
    got = eng.mem.to_numpy(store)
    for im, r in zip(images, rows):
        assert np.array_equal(got[r], odp.resize_bicubic_tf1(im[:, :, :3], Ho, Wo)), r
    assert np.array_equal(got[3], images[2][:, :, :3].astype(np.float32))            # the identity
    for r in (1, 4, 5):
        assert np.isnan(got[r]).all()                                                # untouched rows keep their poison


def test_resize_many_equals_the_single_image_calls(eng):
    rng = np.random.default_rng(12)
    Ho, Wo = 16, 20
    images = [rng.integers(0, 256, (int(rng.integers(5, 60)), int(rng.integers(5, 60)), int(rng.choice([3, 4]))), dtype=np.uint8) for _ in range(5)]
    staged, items = stage(images)
    items["dst_row"] = [4, 2, 0, 1, 3]
    store = eng.mem.empty((5, Ho, Wo, 3))
    eng.resize_bicubic_u8_many(eng.mem.upload_u8(staged), items, store)
    got = eng.mem.to_numpy(store)
    for im, r in zip(images, items["dst_row"]):
        one = eng.mem.empty((Ho, Wo, 3))
        eng.resize_bicubic_u8(im, one)
        assert np.array_equal(got[r], eng.mem.to_numpy(one))
        assert np.array_equal(got[r], odp.resize_bicubic_tf1(im[:, :, :3], Ho, Wo))


# ------------------------------------------------------------------ fs_queue_take
class FixedRng(object):
    """rng.choice returns what the case says (the draw itself is numpy's; the queue logic is what is compared)."""

    def __init__(self, idx):
        self.idx = np.asarray(idx, dtype=np.int64)

    def choice(self, n, size, replace):
        assert not replace and size == len(self.idx) and self.idx.max() < n
        return self.idx.copy()


def take_both_ways(eng, shape, size, capacity, rng_a, rng_b, n):
    """The same queue state through ShuffleQueue.dequeue_many and through FedQueue.take: (batch, store[:new size]) of each."""
    content = np.random.default_rng(size * 131 + n).standard_normal((capacity,) + shape).astype(np.float32)
    old = datapipe.ShuffleQueue(eng, capacity, shape, rng_a)
    old.store = eng.mem.from_numpy(content)
    old.size = size
    want = eng.mem.to_numpy(old.dequeue_many(n)).copy()
    ring = datapipe.DeviceRing(eng, (n,) + shape, 1)
    new = datapipe.FedQueue(eng, capacity, shape, rng_b, ring)
    new.store = eng.mem.from_numpy(content)
    new.size = size
    s = ring.produce(new.take(n))
    got = eng.mem.to_numpy(ring.hand_over(s)).copy()
    ring.close()
    assert new.size == old.size == size - n
    return (want, eng.mem.to_numpy(old.store)[:old.size].copy()), (got, eng.mem.to_numpy(new.store)[:new.size].copy())


@pytest.mark.parametrize("size,idx", [(6, [5, 4]),            # no moves: the taken rows are the tail
                                      (10, [1, 0, 2]),        # all moves: every hole lies below the new size
                                      (5, [2, 3]),            # the chain: row 4 -> 3 -> 2
                                      (5, [3, 2]),
                                      (4, [2, 0, 3, 1]),      # B equal to size: the queue is empty afterwards
                                      (9, [8, 0, 7, 3])],
                         ids=["no_moves", "all_moves", "chain", "chain_rev", "whole_queue", "mixed"])
def test_queue_take_cases_equal_dequeue_many(eng, size, idx):
    (want_b, want_s), (got_b, got_s) = take_both_ways(eng, (3, 4), size, 12, FixedRng(idx), FixedRng(idx), len(idx))
    assert np.array_equal(got_b, want_b) and np.array_equal(got_s, want_s)


def test_queue_take_random_draws_equal_dequeue_many(eng):
    for seed in range(6):
        size, n = 7 + 3 * seed, 2 + seed
        (want_b, want_s), (got_b, got_s) = take_both_ways(eng, (2, 5, 3, 4), size, 40, np.random.default_rng(seed), np.random.default_rng(seed), n)
        assert np.array_equal(got_b, want_b) and np.array_equal(got_s, want_s), seed


def test_queue_take_rows_longer_than_a_chunk(eng):
    """Rows of several workgroup chunks with a ragged end (a chunk is 2048 float4); on the GPU the training row, 256 x 256 x 3 floats."""
    shape = (3, 2100, 4) if on_emulator(eng) else (256, 256, 3)
    (want_b, want_s), (got_b, got_s) = take_both_ways(eng, shape, 9, 10, np.random.default_rng(3), np.random.default_rng(3), 4)
    assert np.array_equal(got_b, want_b) and np.array_equal(got_s, want_s)


# ------------------------------------------------------------------ the fed batcher
def collect(eng, files, **kw):
    return [eng.mem.to_numpy(b).copy() for b in datapipe.batcher(files, engine=eng, **kw)]


@pytest.mark.parametrize("depth", [1, 2, 3])
def test_fed_batcher_yields_the_batches_of_batcher(eng, tmp_path, depth):
    files, _ = make_shards(tmp_path, [5, 4, 6])
    for cut in (None, 5, 1):
        kw = dict(batch_size=3, resize_shape=(16, 20), num_epochs=2, min_after_dequeue=4, seed=5, num_threads=2, max_batches=cut)
        want = collect(eng, files, **kw)
        got = collect(eng, files, prefetch=depth, **kw)
        assert len(want) == (10 if cut is None else cut) and len(got) == len(want)
        for a, b in zip(got, want):
            assert np.array_equal(a, b)


def test_fed_batcher_stages_in_pieces_beyond_the_cap(eng, tmp_path, monkeypatch):
    files, _ = make_shards(tmp_path, [6, 5])
    kw = dict(batch_size=2, resize_shape=(16, 20), num_epochs=1, min_after_dequeue=6, seed=9, num_threads=2)
    want = collect(eng, files, **kw)
    monkeypatch.setattr(datapipe.FedQueue, "STAGE_CAP_BYTES", 5000)        # an image is 1.2 - 6 KB: the fill phase is flushed several times
    got = collect(eng, files, prefetch=2, **kw)
    assert len(got) == len(want) == 5 and all(np.array_equal(a, b) for a, b in zip(got, want))


def test_fed_batcher_ranks_and_early_close(eng, tmp_path):
    files, _ = make_shards(tmp_path, [4, 3])
    kw = dict(batch_size=1, resize_shape=(16, 20), num_epochs=1, min_after_dequeue=1, num_threads=1, world=2)
    for rank in (0, 1):
        want, got = collect(eng, files, rank=rank, **kw), collect(eng, files, rank=rank, prefetch=2, **kw)
        assert len(got) == len(want) and all(np.array_equal(a, b) for a, b in zip(got, want))
    gen = datapipe.batcher(files, 1, (16, 20), num_epochs=None, min_after_dequeue=2, engine=eng, num_threads=1, prefetch=3)
    first = eng.mem.to_numpy(next(gen)).copy()
    gen.close()                                                             # drains; nothing left running
    assert first.shape == (1, 16, 20, 3) and np.isfinite(first).all()


def test_fed_batcher_issues_no_row_copies_and_one_copy_per_batch(eng, tmp_path, monkeypatch):
    files, _ = make_shards(tmp_path, [8, 7])
    calls = {"copy_row": 0, "gather_rows": 0, "upload": 0}

    def counted(name, key):
        real = getattr(eng.mem, name)

        def f(*a, **k):
            calls[key] += 1
            return real(*a, **k)
        monkeypatch.setattr(eng.mem, name, f, raising=True)
    counted("copy_row", "copy_row")
    counted("gather_rows", "gather_rows")
    counted("upload_u8", "upload")
    if getattr(eng.mem, "upload_u8_pinned", None) is not None:
        counted("upload_u8_pinned", "upload")
    got = collect(eng, files, batch_size=4, resize_shape=(16, 20), num_epochs=2, min_after_dequeue=6, seed=1, num_threads=2, prefetch=2)
    assert len(got) == 7                                                    # 30 images, batch 4
    assert calls["copy_row"] == 0 and calls["gather_rows"] == 0
    assert calls["upload"] <= len(got) + 1                                  # one staging copy per batch (+ none extra here), not one per image (30)
    before = dict(calls)
    collect(eng, files, batch_size=4, resize_shape=(16, 20), num_epochs=2, min_after_dequeue=6, seed=1, num_threads=2)
    assert calls["gather_rows"] - before["gather_rows"] == 7 and calls["upload"] - before["upload"] >= 30      # what the counters see of the old path


# ------------------------------------------------------------------ error paths
def test_feed_entry_points_refuse_bad_arguments(eng):
    lib, ctx, mem = eng.lib, eng.ctx, eng.mem
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (6, 7, 3), dtype=np.uint8)
    staged_h, items = stage([img])
    staged = mem.upload_u8(staged_h)
    store = mem.from_numpy(np.full((4, 5, 5, 3), np.nan, np.float32))
    table = mem.upload_u8(np.concatenate([items.view(np.uint8), np.zeros(8, np.uint8)]))

    def resize(it, K=1, dev=None):
        return lib.fs_resize_bicubic_u8x_many(ctx, mem.ptr_u8(staged), staged_h.size, it.ctypes.data, mem.ptr_u8(table) if dev is None else dev,
                                              K, mem.ptr(store), 4, 5, 5)
    assert resize(items) == 0
    assert resize(items, K=0) == -1 and b"fs_resize_bicubic_u8x_many" in lib.fs_last_error()
    for field, value, code in [("dst_row", 4, -4), ("dst_row", -1, -4), ("pixel_bytes", 5, -2), ("pixel_bytes", 1, -2), ("H", 0, -1),
                               ("src_offset", staged_h.size, -1), ("H", 7, -1)]:           # (7 x 7 x 3 bytes do not fit the staged 126 + pad)
        bad = items.copy()
        bad[field] = value
        assert resize(bad) == code, (field, value)
        assert b"image 0" in lib.fs_last_error()
    assert resize(items, dev=mem.ptr_u8(table) + 4) == -5
    assert np.array_equal(mem.to_numpy(store)[0], odp.resize_bicubic_tf1(img, 5, 5)) and np.isnan(mem.to_numpy(store)[1:]).all()

    qs, out = mem.zeros((6, 8)), mem.empty((2, 8))
    idx = mem.upload_u8(np.array([0, 1, 5, 0], dtype=np.int32).view(np.uint8))
    ip = mem.ptr_u8(idx)

    def take(B=2, M=1, row=8, o=None, cap=6, src=ip + 8, dst=ip + 12):
        return lib.fs_queue_take(ctx, mem.ptr(qs), cap, row, ip, B, src, dst, M, mem.ptr(out) if o is None else o)
    assert take() == 0
    assert take(M=3) == -1 and b"fs_queue_take" in lib.fs_last_error()
    assert take(B=0, M=0) == -1 and take(M=-1) == -1 and take(cap=0) == -1 and take(src=None) == -1
    assert take(row=6) == -2 and take(row=0) == -2
    assert take(o=mem.ptr(out) + 4) == -5 and take(src=ip + 9) == -5

    buf = mem.zeros((8,))
    assert lib.fs_synth_uniform(ctx, mem.ptr(buf), 8, 1, 0, 0) == 0
    assert lib.fs_synth_uniform(ctx, mem.ptr(buf), 0, 1, 0, 0) == -1 and b"fs_synth_uniform" in lib.fs_last_error()
    assert lib.fs_synth_uniform(ctx, None, 8, 1, 0, 0) == -1
    assert lib.fs_synth_uniform(ctx, mem.ptr(buf) + 4, 4, 1, 0, 0) == -5
    assert lib.fs_synth_uniform(ctx, mem.ptr(buf), 2 ** 34 + 1, 1, 0, 0) == -1


def test_feed_depth_knob_is_a_table_row():
    lib = _lib.load()
    assert _lib.knob(lib, "FS_FEED_DEPTH") == 2
    with pytest.raises(_lib.FaststyleError):
        _lib.knob(lib, "NO_SUCH_ROW")
