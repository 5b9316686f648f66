"""The library's FS_* knobs are the rows of one table (csrc/fs_knobs.h), reported by fs_debug_knob: the documentation lists exactly
those rows, tests and tools only set names that exist, a knob is read from the environment once per fs_debug_reload_env -- the last
row included -- and the default knobs still select the kernels (hence the workspace sizes) they selected before the table existed.
Host-side only: the product library, no GPU."""
import ctypes
import glob
import os
import re

import pytest

from faststyle_amd import _lib, build as fsbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "faststyle_amd", "csrc")
# read by Python (the paragraph under the table), not by the library
PYTHON_SIDE = {"FS_DIST_BACKEND", "FS_DIST_SHARE_GPU", "FS_DATAPIPE_RGBX", "FS_BUILD_SLP_ALLOWLIST", "FASTSTYLE_HIP_LIB",
               "FS_EMU_SANITIZE", "FS_TEST_WORKERS", "FS_BENCH_FRAMES_IN_FLIGHT", "FS_TRACE_MARK"}


@pytest.fixture(scope="module")
def lib():
    fsbuild.build()
    return _lib.load()


def knob_rows(lib):
    rows = []
    while True:
        name, dflt, value = ctypes.c_char_p(), ctypes.c_int(), ctypes.c_int()
        if lib.fs_debug_knob(len(rows), ctypes.byref(name), ctypes.byref(dflt), ctypes.byref(value)) != 0:
            return rows
        rows.append((name.value.decode(), dflt.value, value.value))


def design_rows():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = text[text.index("## 10a."):text.index("## 10b.")]
    return sec, re.findall(r"^\| `(FS_[A-Z0-9_]+)` \| (-?\d+)[^|]*\|", sec, flags=re.M)


def test_design_lists_every_knob_with_its_default(lib):
    rows = knob_rows(lib)
    assert len(rows) > 64 and len({r[0] for r in rows}) == len(rows)
    assert lib.fs_debug_knob(-1, None, None, None) == -1 and lib.fs_debug_knob(len(rows), None, None, None) == -1
    sec, doc = design_rows()
    assert [(n, int(d)) for n, d in doc] == [(n, d) for n, d, _ in rows]      # same rows, same order, same defaults
    for name in PYTHON_SIDE:
        assert name in sec, name


def test_names_set_by_tests_and_tools_exist(lib):
    known = {r[0] for r in knob_rows(lib)} | PYTHON_SIDE
    files = glob.glob(os.path.join(ROOT, "tests", "*.py")) + glob.glob(os.path.join(ROOT, "tools", "*.py")) + \
        [os.path.join(ROOT, "bench.py"), os.path.join(ROOT, "train.py")]
    unknown = []
    for f in sorted(files):
        text = open(f).read()
        # a quoted name (os.environ[...], setenv, a dict of knobs) or a keyword of dict(...); constants of the C header are attributes of _lib
        for name in set(re.findall(r"[\"'](FS_[A-Z0-9_]+)[\"']", text)) | set(re.findall(r"\b(FS_[A-Z0-9_]+)=(?!=)", text)):
            if name not in known and not hasattr(_lib, name):
                unknown.append((os.path.relpath(f, ROOT), name))
    assert not unknown, unknown


def test_last_row_is_read_once_per_reload(lib, monkeypatch):
    name, dflt, _ = knob_rows(lib)[-1]          # the 64-entry cache this table replaced could not hold it
    last = len(knob_rows(lib)) - 1

    def value():
        v = ctypes.c_int()
        assert lib.fs_debug_knob(last, None, None, ctypes.byref(v)) == 0
        return v.value
    try:
        monkeypatch.setenv(name, "0x11")       # strtol, base 0
        lib.fs_debug_reload_env()
        assert value() == 17
        monkeypatch.setenv(name, "23")
        assert value() == 17                    # not re-read without a reload
        lib.fs_debug_reload_env()
        assert value() == 23
        monkeypatch.delenv(name)
        assert value() == 23
        lib.fs_debug_reload_env()
        assert value() == dflt
    finally:
        monkeypatch.undo()
        lib.fs_debug_reload_env()


def test_one_getenv_and_no_knob_name_outside_the_table():
    getenvs, stray = [], []
    for f in sorted(os.listdir(CSRC)):
        text = open(os.path.join(CSRC, f)).read()
        getenvs += [f] * len(re.findall(r"\bgetenv\s*\(", text))
        assert "tune_int(" not in text and "env_int(" not in text and "env_int2(" not in text, f
        if f != "fs_knobs.h":
            stray += [(f, s) for s in re.findall(r"\"FS_[A-Z0-9_]+\"", text)]
    assert getenvs == ["fs_api.hip"] and not stray, (getenvs, stray)


# fs_tnet_workspace_bytes under default knobs, recorded from the library BEFORE the residual-conv choice moved into one function: the size depends on
# the kernel of every residual unit (16 or 36 filter planes, records per tile), so it fingerprints the choice
PINNED_WS = {(32, 256, 256): (3234142720, 761272320), (4, 256, 256): (550272768, 95957248), (1, 256, 256): (222041344, 24676352),
             (1, 720, 1280): (1206602240, 271219968)}


def test_default_knobs_select_the_same_kernels(lib, monkeypatch):
    for k in [k for k in os.environ if k.startswith("FS_")]:
        monkeypatch.delenv(k)
    lib.fs_debug_reload_env()
    try:
        for (n, h, w), (train, bf16) in PINNED_WS.items():
            assert lib.fs_tnet_workspace_bytes(n, h, w, _lib.FS_FLAG_SAVE_FOR_BWD) == train, (n, h, w)
            assert lib.fs_tnet_workspace_bytes(n, h, w, _lib.FS_FLAG_BF16) == bf16, (n, h, w)
    finally:
        monkeypatch.undo()
        lib.fs_debug_reload_env()
