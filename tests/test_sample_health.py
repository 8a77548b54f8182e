"""CPU: tools/sample.py --health {off,flag,skip} with a stub pipeline (this file, loaded through the driver's --pipe-factory hook).

Five scenes in batches of two, two generations each; the stub reports scene 1 as dead from step 2 on, in both generations.
  off   the run is what it is without the option: same files, same bytes, same index.json (no health field anywhere), exit status 0;
  flag  every picture is written, index.json gains ok / first_bad_step / nonfinite / absmax per scene and generation, exit status 3;
  skip  as flag, and exactly the bad scene's twelve files are missing; its batchmate's files are byte-identical to the clean run's.
The stub samples nothing: a view is a 4 x 6 uint8 picture whose value says which seed / camera / scene produced it.
"""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH, TIMES, BAD_SCENE, BAD_STEP, N_STEPS = 2, 2, 1, 2, 4


class _Out:
    def __init__(self, images, health):
        self.images, self.health = images, health


class _Health:
    def __init__(self, ok, first_bad_step, final, image_nonfinite=None):
        self.ok, self.first_bad_step, self.final, self.image_nonfinite = ok, first_bad_step, final, image_nonfinite


class _Unet:
    cfg = {"cross_attention_dim": 8}


class StubPipe:
    text_encoder = None
    unet = _Unet()

    def __init__(self):
        self.health = None
        self.calls = 0

    def __call__(self, generator=None, image=None, camera_param=None, prompt_embeds=None, **kw):
        g = generator[0] if isinstance(generator, (list, tuple)) else generator
        seed = 0 if g is None else int(g.initial_seed())
        draw = int(torch.randint(0, 97, [1], generator=g)) if g is not None else 0
        scene0 = (self.calls // TIMES) * BATCH                 # the driver makes TIMES calls per batch of BATCH scenes, in order
        self.calls += 1
        bs, n_cam = image.shape[0], camera_param.shape[1]
        images = []
        for bi in range(bs):
            tag = int(image[bi].float().abs().sum().item() * 1000) % 251
            images.append([np.full((4, 6, 3), (seed * 7 + cam * 13 + tag + draw) % 256, dtype=np.uint8) for cam in range(n_cam)])
        health = None
        if self.health is not None:
            assert self.health == "trace" and self.health_action == "flag", "the driver asks for the per-step records and decides itself"
            bad = [scene0 + bi == BAD_SCENE for bi in range(bs)]
            final = np.zeros((bs, n_cam, 4), dtype=np.float32)
            final[..., 1] = 4.5
            for bi in range(bs):
                if bad[bi]:
                    final[bi, :, 0] = 5600.0
                    final[bi, :, 1] = 0.0
            health = _Health([not b for b in bad], [BAD_STEP if b else -1 for b in bad], final)
        return _Out(images, health)


def make(ckpt, sd15, scheduler, device, given_view):
    return StubPipe()


def run_driver(tmp_path, out_name, extra=(), world=1):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), os.environ.get("PYTHONPATH", "")]),
               CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="", OMP_NUM_THREADS="2")
    argv = [os.path.join(ROOT, "tools", "sample.py"), "--ckpt", str(tmp_path / "ckpt"), "--sd15", str(tmp_path / "sd15"), "--data", str(tmp_path / "data"),
            "--out", str(tmp_path / out_name), "--prompt-embeds", "--pipe-factory", "test_sample_health:make", "--dist-backend", "gloo", "--device", "cpu",
            "--batch-size", str(BATCH), f"runner.validation_times={TIMES}", *extra]
    if world == 1:
        cmd = [sys.executable] + argv
    else:
        with socket.socket() as so:
            so.bind(("127.0.0.1", 0))
            port = so.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
               "--master-port", str(port)] + argv
    return subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("sample_health")
    gold = torch.load(os.path.join(ROOT, "tests", "golden", "sample_preprocess.pt"), weights_only=False)
    os.makedirs(tmp / "data"); os.makedirs(tmp / "ckpt" / "hydra"); os.makedirs(tmp / "sd15")
    for i, case in enumerate(gold["cases"]):
        torch.save(case["sample"], tmp / "data" / f"tok{i}.pth")
    with open(tmp / "ckpt" / "hydra" / "overrides.yaml", "w") as f:
        f.write("- +exp=224x400\n- seed=7\n")
    res = {"plain": run_driver(tmp, "plain"), "off": run_driver(tmp, "off", ["--health", "off"]),
           "flag": run_driver(tmp, "flag", ["--health", "flag"]), "skip": run_driver(tmp, "skip", ["--health", "skip"]),
           "skip_gathered": run_driver(tmp, "skip_gathered", ["--health", "skip", "--gather-images"])}
    return tmp, res


def pngs(tmp, d):
    return sorted(x for x in os.listdir(tmp / d) if x.endswith(".png"))


def read(tmp, d, n):
    with open(tmp / d / n, "rb") as f:
        return f.read()


def test_off_is_the_run_without_the_option(runs):
    tmp, res = runs
    assert res["plain"].returncode == 0 and res["off"].returncode == 0, res["off"].stderr[-2000:]
    assert len(pngs(tmp, "plain")) == 5 * TIMES * 6 and pngs(tmp, "off") == pngs(tmp, "plain")
    for n in pngs(tmp, "plain") + ["index.json"]:
        assert read(tmp, "off", n) == read(tmp, "plain", n), n
    assert res["off"].stdout.replace("/off", "/plain") == res["plain"].stdout and "health:" not in res["off"].stdout
    for g in json.loads(read(tmp, "off", "index.json"))["generations"]:
        assert set(g) == {"scene", "gen", "rank", "seed", "files"}, g


def test_flag_records_and_keeps_every_picture(runs):
    tmp, res = runs
    assert res["flag"].returncode == 3, (res["flag"].returncode, res["flag"].stderr[-2000:])
    assert pngs(tmp, "flag") == pngs(tmp, "plain")
    for n in pngs(tmp, "plain"):
        assert read(tmp, "flag", n) == read(tmp, "plain", n), n
    gens = json.loads(read(tmp, "flag", "index.json"))["generations"]
    assert [(g["scene"], g["gen"]) for g in gens] == [(s, t) for s in range(5) for t in range(TIMES)]
    for g in gens:
        if g["scene"] == BAD_SCENE:
            assert (g["ok"], g["first_bad_step"], g["nonfinite"], g["absmax"]) == (False, BAD_STEP, 6 * 5600, 0.0) and len(g["files"]) == 6, g
        else:
            assert (g["ok"], g["first_bad_step"], g["nonfinite"], g["absmax"]) == (True, -1, 0, 4.5) and len(g["files"]) == 6, g
    last = res["flag"].stdout.strip().splitlines()[-1]
    assert last == f"health: {TIMES} of {5 * TIMES} generations bad (scenes [{BAD_SCENE}])", last


@pytest.mark.parametrize("d", ["skip", "skip_gathered"])
def test_skip_leaves_out_exactly_the_bad_scenes_files(runs, d):
    tmp, res = runs
    assert res[d].returncode == 3, (res[d].returncode, res[d].stderr[-2000:])
    missing = sorted(set(pngs(tmp, "plain")) - set(pngs(tmp, d)))
    assert missing == sorted(f"{BAD_SCENE}_gen{t}_view{v}.png" for t in range(TIMES) for v in range(6))
    assert set(pngs(tmp, d)) <= set(pngs(tmp, "plain"))
    for n in pngs(tmp, d):                                   # the batchmate (scene 0) and everyone else: the clean run's bytes
        assert read(tmp, d, n) == read(tmp, "plain", n), n
    gens = json.loads(read(tmp, d, "index.json"))["generations"]
    assert len(gens) == 5 * TIMES
    for g in gens:
        if g["scene"] == BAD_SCENE:
            assert g["ok"] is False and g["first_bad_step"] == BAD_STEP and g["files"] == [], g
        else:
            assert g["ok"] is True and len(g["files"]) == 6 and all(os.path.exists(tmp / d / f) for f in g["files"]), g
    last = res[d].stdout.strip().splitlines()[-1]
    assert last == f"health: {TIMES} of {5 * TIMES} generations bad (scenes [{BAD_SCENE}], pictures not written)", last
