"""The native JPEG path at script level: train.py over TFRecord shards writes the same checkpoint, byte for byte, with FS_FEED_JPEG=1 and
without it (GPU), the knob is a row of the library's table and off by default, and the decoder's malformed-input cases pass under the
emulator build's address and undefined-behaviour sanitisers."""
import glob
import os
import subprocess
import sys

import pytest

from tests.test_datapipe import make_shards
from tests.test_feed_train import _train, _work

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_feed_jpeg_knob_is_off_by_default(monkeypatch):
    from faststyle_amd import _lib, build as fsbuild
    fsbuild.build()
    lib = _lib.load()
    monkeypatch.delenv("FS_FEED_JPEG", raising=False)
    lib.fs_debug_reload_env()
    try:
        assert _lib.knob(lib, "FS_FEED_JPEG") == 0
        monkeypatch.setenv("FS_FEED_JPEG", "1")
        lib.fs_debug_reload_env()
        assert _lib.knob(lib, "FS_FEED_JPEG") == 1
    finally:
        monkeypatch.undo()
        lib.fs_debug_reload_env()


@pytest.mark.gpu
def test_train_writes_the_same_checkpoint_with_native_jpeg_decode(tmp_path, monkeypatch):
    from faststyle_amd import _lib
    lib = _lib.load()
    make_shards(tmp_path, [9, 8, 7])
    files = {}
    try:
        for native in (None, "1"):
            if native is None:
                monkeypatch.delenv("FS_FEED_JPEG", raising=False)
            else:
                monkeypatch.setenv("FS_FEED_JPEG", native)
            monkeypatch.delenv("FS_FEED_DEPTH", raising=False)
            lib.fs_debug_reload_env()
            assert _lib.knob(lib, "FS_FEED_JPEG") == (1 if native else 0)
            work = _work(tmp_path, monkeypatch, "w%s" % native)
            tr = _train(["--train_dir", str(tmp_path), "--model_name", "j", "--n_epochs", "2", "--num_pipe_buffer", "5", "--num_steps_ckpt", "10"])
            assert tr.global_step == 24                                      # 48 images / 2
            files[native] = {os.path.relpath(f, str(work)): open(f, "rb").read()
                             for f in sorted(glob.glob(str(work / "training" / "j.ckpt-*")) + glob.glob(str(work / "models" / "j_final.ckpt*")))}
            assert open(str(work / "summaries" / "train" / "j0" / "scalars.jsonl")).read().count("\n") == 3
        # the native path is refused, not silently replaced, without the ring
        monkeypatch.setenv("FS_FEED_JPEG", "1")
        monkeypatch.setenv("FS_FEED_DEPTH", "0")
        lib.fs_debug_reload_env()
        _work(tmp_path, monkeypatch, "wsync")
        with pytest.raises(_lib.FaststyleError, match="prefetch > 0"):
            _train(["--train_dir", str(tmp_path), "--model_name", "j", "--n_epochs", "1", "--num_pipe_buffer", "5"])
    finally:
        monkeypatch.undo()
        lib.fs_debug_reload_env()
    assert len(files[None]) >= 4 and sorted(files[None]) == sorted(files["1"])
    for name in files[None]:
        assert files[None][name] == files["1"][name], name


SANITIZED_BODY = """
import sys
sys.path.insert(0, %r)
from tests import emu_lib, test_jpeg
eng = emu_lib.emu_engine()
print("jpeg malformed: %%d cases ok" %% test_jpeg.malformed_cases(eng.lib, eng))
"""


def test_malformed_input_under_address_and_undefined_behaviour_sanitizers():
    from tests import emu_lib
    emu_lib.build_emu_sanitized()
    env = dict(os.environ, FS_EMU_SANITIZE="1", LD_PRELOAD=emu_lib.ASAN_RT,
               ASAN_OPTIONS="detect_leaks=0:detect_stack_use_after_return=0:halt_on_error=1:verify_asan_link_order=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    out = subprocess.run([sys.executable, "-c", SANITIZED_BODY % ROOT], cwd=ROOT, capture_output=True, text=True, timeout=2400, env=env)
    assert out.returncode == 0 and "jpeg malformed:" in out.stdout and "cases ok" in out.stdout, (out.stdout[-1500:], out.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error:" not in out.stderr, out.stderr[-3000:]
