"""CPU: tools/sample.py --regenerate-boxes --composite end to end with a stub pipeline (this file, loaded through the driver's
--pipe-factory hook), as tests/test_sample_regions.py tests the flag it builds on.

The stub samples nothing: a view's generated picture is one value (tests/sample_stub.py).  With pipe.composite_images set, this file's
subclass paints that value over the run's (224, 400) picture and composites it with the recorded picture it was handed, the matte being
magicdrive_amd.dataset.edit_matte of the keep mask it was handed — the torch statement of what the device op computes.
  the flags' refusals    --composite without --regenerate-boxes, --feather / --save-matte without --composite, a feather outside [0, 16];
  without --composite    files and index.json are byte-identical to the plain run's (which tests/test_sample_regions.py rebuilds from
                         first principles), and the pipeline's composite attributes are never touched;
  with --composite       index.json gains "composite": {"feather": N} and kept_fraction per generation and view, nothing else changes in
                         it; a written PNG holds the recorded picture's bytes wherever the matte is 1 and the generated value wherever
                         it is 0; --save-matte writes round(255 w) next to each view.
"""
import importlib.util
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import sample_stub

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH, TIMES, SEED, FEATHER = 2, 2, 7, 3


class _Vae:
    dtype = torch.float32
    config = SimpleNamespace(scaling_factor=0.5)

    def encode(self, x):
        mean = x.mean(dim=(1, 2, 3)).view(-1, 1, 1, 1).expand(-1, 4, 28, 50) * 2.0
        return SimpleNamespace(latent_dist=SimpleNamespace(mean=mean))


class CompositeStub(sample_stub.StubPipe):
    _execution_device = torch.device("cpu")

    def __init__(self, given_view):
        self.vae = _Vae()
        self.keep_masks = None
        self.given_view = bool(given_view)

    def __call__(self, conditional_latents=None, **kw):
        from magicdrive_amd.dataset import edit_matte
        pics, feather = getattr(self, "composite_images", None), getattr(self, "composite_feather", None)
        rec = dict(given_view=self.given_view, has_attr=hasattr(self, "composite_images") or hasattr(self, "composite_feather"), feather=feather,
                   pics=None if pics is None else [[[list(p.shape), str(p.dtype), float(p.min()), float(p.max())] for p in r] for r in pics])
        with open(os.environ["COMPOSITE_STUB_LOG"], "a") as f:
            f.write(json.dumps(rec) + "\n")
        out = super().__call__(**kw)
        if pics is None:
            return out
        H, W = kw["height"], kw["width"]
        images, mattes = [], []
        for bi, views in enumerate(out.images):
            row, mrow = [], []
            for vi, small in enumerate(views):
                g = np.float32(small.flat[0]) / np.float32(255)
                w = edit_matte(self.keep_masks[bi][vi], 8, feather).numpy()[..., None]
                o = pics[bi][vi].numpy()
                x = np.where(w == 0, g, np.where(w == 1, o, w * o + (1 - w) * g)).astype(np.float32)
                row.append((x * 255).round().astype("uint8"))
                mrow.append(w[..., 0])
                assert x.shape == (H, W, 3)
            images.append(row); mattes.append(np.stack(mrow))
        out.images, out.matte = images, np.stack(mattes)
        return out


def make(ckpt, sd15, scheduler, device, given_view):
    return CompositeStub(given_view)


def run_driver(tmp_path, out_name, extra=()):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), os.environ.get("PYTHONPATH", "")]),
               CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="", OMP_NUM_THREADS="2", COMPOSITE_STUB_LOG=str(tmp_path / f"{out_name}.jsonl"))
    cmd = [sys.executable, os.path.join(ROOT, "tools", "sample.py"), "--ckpt", str(tmp_path / "ckpt"), "--sd15", str(tmp_path / "sd15"), "--data", str(tmp_path / "data"),
           "--out", str(tmp_path / out_name), "--prompt-embeds", "--pipe-factory", "test_sample_composite:make", "--dist-backend", "gloo", "--device", "cpu",
           "--batch-size", str(BATCH), f"runner.validation_times={TIMES}", *extra]
    return subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("sample_composite")
    gold = torch.load(os.path.join(ROOT, "tests", "golden", "sample_preprocess.pt"), weights_only=False)
    os.makedirs(tmp / "data"); os.makedirs(tmp / "ckpt" / "hydra"); os.makedirs(tmp / "sd15")
    for i, case in enumerate(gold["cases"]):                     # the golden samples carry thumbnails: give each one pictures at the run's size
        smp = dict(case["sample"])
        smp["img"] = torch.rand(6, 3, 224, 400, generator=torch.Generator().manual_seed(40 + i)) * 2 - 1
        torch.save(smp, tmp / "data" / f"tok{i}.pth")
    with open(tmp / "ckpt" / "hydra" / "overrides.yaml", "w") as f:
        f.write(f"- +exp=224x400\n- seed={SEED}\n")
    res = {"plain": run_driver(tmp, "plain"), "regen": run_driver(tmp, "regen", ["--regenerate-boxes"]),
           "comp": run_driver(tmp, "comp", ["--regenerate-boxes", "--composite", "--feather", str(FEATHER), "--save-matte"]),
           "comp4": run_driver(tmp, "comp4", ["--regenerate-boxes", "--composite"])}
    return tmp, res, len(gold["cases"])


def files(tmp, d, suffix=".png"):
    return sorted(x for x in os.listdir(tmp / d) if x.endswith(suffix))


def read(tmp, d, n):
    with open(tmp / d / n, "rb") as f:
        return f.read()


def log(tmp, d):
    with open(tmp / f"{d}.jsonl") as f:
        return [json.loads(ln) for ln in f]


@pytest.mark.parametrize("extra,what", [(["--composite"], "--regenerate-boxes only"), (["--composite", "--cond-on-view"], "--regenerate-boxes only"),
                                        (["--regenerate-boxes", "--feather", "3"], "belong to --composite"), (["--regenerate-boxes", "--save-matte"], "belong to --composite"),
                                        (["--regenerate-boxes", "--composite", "--feather", "17"], r"\[0, 16\]"), (["--regenerate-boxes", "--composite", "--feather", "-1"], r"\[0, 16\]")])
def test_the_flags_refusals(tmp_path, extra, what):
    """Refused while the command line is read, as --resample is: before a pipeline is built (the factory named here does not exist)."""
    sp = importlib.util.spec_from_file_location("mdx_tools_sample_cp", os.path.join(ROOT, "tools", "sample.py"))
    sample = importlib.util.module_from_spec(sp); sp.loader.exec_module(sample)
    os.makedirs(tmp_path / "ckpt")
    with pytest.raises(SystemExit, match=what):
        sample.main(["--ckpt", str(tmp_path / "ckpt"), "--sd15", str(tmp_path), "--data", str(tmp_path), "--out", str(tmp_path / "out"), "--device", "cpu",
                     "--pipe-factory", "no_such_module:make", *extra])
    assert not os.path.exists(tmp_path / "out")


def test_without_the_flag_nothing_changes(runs):
    tmp, res, n = runs
    for d in ("plain", "regen"):
        assert res[d].returncode == 0, res[d].stderr[-2000:]
    assert files(tmp, "regen") == files(tmp, "plain") and len(files(tmp, "regen")) == n * TIMES * 6
    for name in files(tmp, "regen") + ["index.json"]:
        assert read(tmp, "regen", name) == read(tmp, "plain", name), name
    index = json.loads(read(tmp, "regen", "index.json"))
    assert set(index) == {"world", "seed", "gather_images", "generations"} and all(set(g) == {"scene", "gen", "rank", "seed", "files"} for g in index["generations"])
    calls = log(tmp, "regen")
    assert len(calls) == 3 * TIMES and all(c["given_view"] and c["pics"] is None and c["feather"] is None and not c["has_attr"] for c in calls)
    assert not files(tmp, "regen", "_matte.png")


@pytest.mark.parametrize("d,feather", [("comp", FEATHER), ("comp4", 4)])
def test_with_the_flag_the_index_gains_its_fields(runs, d, feather):
    from magicdrive_amd import dataset as DS
    tmp, res, n = runs
    assert res[d].returncode == 0, res[d].stderr[-2000:]
    index = json.loads(read(tmp, d, "index.json"))
    base = json.loads(read(tmp, "regen", "index.json"))
    assert list(index) == ["world", "seed", "gather_images", "composite", "generations"] and index["composite"] == {"feather": feather}
    assert [{k: v for k, v in g.items() if k != "kept_fraction"} for g in index["generations"]] == base["generations"]
    data = DS.FolderSet(str(tmp / "data"))
    for g in index["generations"]:
        ex = data[g["scene"]]
        corners, kept = DS.project_box_corners(ex["gt_bboxes_3d"], ex["lidar2image"], ex["img_aug_matrix"])
        w = DS.edit_matte(DS.box_keep_mask(corners, kept, (224, 400), (28, 50)), 8, feather)
        assert len(g["kept_fraction"]) == 6 and g["kept_fraction"] == pytest.approx([float(w[v].mean()) for v in range(6)], abs=1e-6)
    calls = log(tmp, d)
    assert len(calls) == 3 * TIMES and all(c["feather"] == feather for c in calls)
    for c in calls:                                              # the recorded pictures: fp32 (224, 400, 3) in [0, 1], one per scene and view
        assert all(len(r) == 6 for r in c["pics"])
        assert all(p[0] == [224, 400, 3] and p[1] == "torch.float32" and 0.0 <= p[2] <= p[3] <= 1.0 for r in c["pics"] for p in r)
    assert len(files(tmp, d, "_matte.png")) == (n * TIMES * 6 if d == "comp" else 0)
    assert sorted(set(files(tmp, d)) - set(files(tmp, d, "_matte.png"))) == files(tmp, "regen")


def test_kept_pixels_are_the_recorded_bytes(runs):
    """Every written view against the sample's own picture: where the matte is 1 the PNG holds the recorded bytes, where it is 0 the
    generated value (the one the run without --composite wrote), and both regimes occur; the matte file is round(255 w)."""
    from PIL import Image
    from magicdrive_amd import dataset as DS
    tmp, res, n = runs
    assert res["comp"].returncode == 0, res["comp"].stderr[-2000:]
    data = DS.FolderSet(str(tmp / "data"))
    kept_px = regen_px = 0
    for s in range(n):
        ex = data[s]
        px = DS.preprocess_fn(ex)["pixel_values"][0]                                         # (6, 3, 224, 400) in [-1, 1]
        rec = ((px.float() / 2 + 0.5).clamp(0, 1).permute(0, 2, 3, 1).numpy() * 255).round().astype("uint8")
        corners, kept = DS.project_box_corners(ex["gt_bboxes_3d"], ex["lidar2image"], ex["img_aug_matrix"])
        w = DS.edit_matte(DS.box_keep_mask(corners, kept, (224, 400), (28, 50)), 8, FEATHER).numpy()
        for ti in range(TIMES):
            for v in range(6):
                name = f"{s}_gen{ti}_view{v}.png"
                got = np.asarray(Image.open(tmp / "comp" / name))
                gen_value = np.asarray(Image.open(tmp / "regen" / name))[0, 0, 0]
                assert got.shape == (224, 400, 3)
                one, zero = w[v] == 1, w[v] == 0
                assert np.array_equal(got[one], rec[v][one]), name
                assert (got[zero] == gen_value).all(), name
                kept_px += int(one.sum()); regen_px += int(zero.sum())
                m = np.asarray(Image.open(tmp / "comp" / f"{s}_gen{ti}_view{v}_matte.png"))
                assert m.dtype == np.uint8 and np.array_equal(m, (w[v] * 255).round().astype("uint8")), name
    assert kept_px > 0 and regen_px > 0
