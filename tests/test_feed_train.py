"""The device-fed input path under the training loop, on the GPU: a ring slot is never overwritten while a step still reads it, a
``synthetic:device`` run continues bit for bit through --resume_from, and train.py logs the same losses with the ring and without it."""
import json
import os
import sys

import numpy as np
import pytest

from tests.test_datapipe import make_shards

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STYLE = os.path.join(ROOT, "style_images", "starry_night_crop.jpg")


@pytest.mark.gpu
@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
def test_steps_fed_from_the_ring_equal_steps_fed_from_clones(use_graph):
    """Thirty steps from a depth-2 ring (batch k + 2 is generated into the slot of batch k while step k + 1 runs) against the same thirty steps
    from up-front clones of the same batches: an early overwrite of a slot changes the parameters."""
    import torch
    from faststyle_amd import datapipe, engine, im_transf_net, trainer, vgg16
    e = engine.Engine()
    style = np.random.default_rng(0).uniform(0, 255, (1, 64, 80, 3)).astype(np.float32)
    p0 = e.flatten_params(im_transf_net.initial_variables(0), scope="")
    vw = vgg16.synthetic_weights(3)
    clones = [b.clone() for b in datapipe.synthetic_device_batches(e, 2, (64, 64), 77, 0, 0, 30, 2)]
    torch.cuda.synchronize()
    assert len(clones) == 30 and not torch.equal(clones[0], clones[2])
    a = trainer.Trainer(e, p0, vw, style, use_graph=use_graph)
    for b in clones:
        a.step(b)
    b_tr = trainer.Trainer(e, p0, None, style, use_graph=use_graph)
    fed = datapipe.synthetic_device_batches(e, 2, (64, 64), 77, 0, 0, 30, 2)
    for b in fed:
        b_tr.step(b)
    fed.close()
    torch.cuda.synchronize()
    assert a.global_step == b_tr.global_step == 30 and (a.graph is not None) == use_graph
    assert torch.equal(a.params, b_tr.params) and torch.equal(a.m, b_tr.m) and torch.equal(a.v, b_tr.v)
    assert not torch.equal(a.params, e.mem.from_numpy(p0))


def _work(tmp_path, monkeypatch, name):
    from faststyle_amd import vgg16
    work = tmp_path / name
    (work / "libs").mkdir(parents=True)
    np.savez(str(work / "libs" / "vgg16_weights.npz"), **vgg16.synthetic_weights(3))
    monkeypatch.chdir(work)
    return work


def _train(argv):
    sys.path.insert(0, ROOT)
    import train
    return train.main(train.setup_parser().parse_args(
        argv + ["--style_img_path", STYLE, "--style_target_resize", "0.25", "--preprocess_size", "64", "64", "--batch_size", "2"]))


@pytest.mark.gpu
def test_synthetic_device_run_resumes_bit_for_bit(tmp_path, monkeypatch, capsys):
    from faststyle_amd import ckpt
    wa = _work(tmp_path, monkeypatch, "a")
    tr = _train(["--train_dir", "synthetic:device", "--model_name", "m", "--num_steps_break", "20", "--num_steps_ckpt", "10"])
    assert tr.global_step == 21
    out = [l for l in capsys.readouterr().out.splitlines() if l and "amdgpu" not in l]
    assert out[-1] == "Done training."
    wb = _work(tmp_path, monkeypatch, "b")
    tr = _train(["--train_dir", "synthetic:device", "--model_name", "m", "--num_steps_break", "10", "--num_steps_ckpt", "10"])
    assert tr.global_step == 11
    tr = _train(["--train_dir", "synthetic:device", "--model_name", "m", "--run_name", "m0", "--num_steps_break", "20", "--num_steps_ckpt", "10",
                 "--resume_from", str(wb / "training" / "m.ckpt-10")])
    assert tr.global_step == 21
    out = [l for l in capsys.readouterr().out.splitlines() if l and "amdgpu" not in l]
    assert out[-1] == "Done training." and any(l.startswith("Resumed from") and l.endswith("at step 10.") for l in out)
    fa, fb = (ckpt.load_checkpoint(str(w / "models" / "m_final.ckpt")) for w in (wa, wb))
    assert sorted(fa) == sorted(fb) and len(fa) == 48
    for k in fa:
        assert np.array_equal(fa[k], fb[k]), k
    la, lb = ([json.loads(l) for l in open(str(w / "summaries" / "train" / "m0" / "scalars.jsonl"))] for w in (wa, wb))
    assert [d["step"] for d in la] == [0, 10, 20] and la[2] == lb[-1] and la[1] == [d for d in lb if d["step"] == 10][-1]


@pytest.mark.gpu
def test_train_logs_the_same_losses_with_the_ring_and_without(tmp_path, monkeypatch):
    from faststyle_amd import _lib
    lib = _lib.load()
    make_shards(tmp_path, [9, 8, 7])
    logs = {}
    try:
        for depth in ("0", None, "3"):
            if depth is None:
                monkeypatch.delenv("FS_FEED_DEPTH", raising=False)
            else:
                monkeypatch.setenv("FS_FEED_DEPTH", depth)
            lib.fs_debug_reload_env()
            assert _lib.knob(lib, "FS_FEED_DEPTH") == (2 if depth is None else int(depth))
            work = _work(tmp_path, monkeypatch, "w%s" % depth)
            _train(["--train_dir", str(tmp_path), "--model_name", "r", "--n_epochs", "2", "--num_pipe_buffer", "5", "--num_steps_ckpt", "100"])
            logs[depth] = [json.loads(l) for l in open(str(work / "summaries" / "train" / "r0" / "scalars.jsonl"))]
    finally:
        monkeypatch.undo()
        lib.fs_debug_reload_env()
    assert [d["step"] for d in logs["0"]] == [0, 10, 20] and all(np.isfinite(d["loss"]) for d in logs["0"])      # 48 images / 2 = 24 steps
    assert logs[None] == logs["0"] and logs["3"] == logs["0"]
