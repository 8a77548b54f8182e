"""tools/sample.py --resample JL,JN: on the CPU with a stub pipeline (this file, loaded through the driver's --pipe-factory hook), and
-m gpu end to end on a tiny checkpoint.

  with the flag       pipe.resample reaches the pipeline as a pair of ints next to the masks of --regenerate-boxes, index.json carries
                      "resample": [JL, JN] and nothing else changes (the stub ignores the switch: same pictures, same records);
  refusals            without --regenerate-boxes, with --scheduler unipc (the driver's default) and for a malformed pair the driver stops
                      before it builds a pipeline;
  without the flag    byte for byte today's output: tests/test_sample_regions.py rebuilds those bytes from first principles, and the
                      --regenerate-boxes run of this file equals it file by file;
  on the GPU          --regenerate-boxes --resample 2,2 on the real pipeline: the files are written, index.json carries the pair, and
                      generation 0 is bit-identical to setting pipe.resample by hand.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import test_sample_regions as SR

ROOT = SR.ROOT


class ResampleStub(SR.RegionStub):
    def __init__(self, given_view):
        super().__init__(given_view)
        self.resample = None

    def __call__(self, **kw):
        with open(os.environ["REGION_STUB_LOG"] + ".resample", "a") as f:
            f.write(json.dumps(dict(resample=self.resample, kind=type(self.resample).__name__)) + "\n")
        return super().__call__(**kw)


def make(ckpt, sd15, scheduler, device, given_view):
    return ResampleStub(given_view)


def run_driver(tmp_path, out_name, extra=()):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), os.environ.get("PYTHONPATH", "")]),
               CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="", OMP_NUM_THREADS="2", REGION_STUB_LOG=str(tmp_path / f"{out_name}.jsonl"))
    cmd = [sys.executable, os.path.join(ROOT, "tools", "sample.py"), "--ckpt", str(tmp_path / "ckpt"), "--sd15", str(tmp_path / "sd15"), "--data", str(tmp_path / "data"),
           "--out", str(tmp_path / out_name), "--prompt-embeds", "--pipe-factory", "test_sample_resample:make", "--dist-backend", "gloo", "--device", "cpu",
           "--batch-size", str(SR.BATCH), f"runner.validation_times={SR.TIMES}", *extra]
    return subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("sample_resample")
    gold = torch.load(os.path.join(ROOT, "tests", "golden", "sample_preprocess.pt"), weights_only=False)
    os.makedirs(tmp / "data"); os.makedirs(tmp / "ckpt" / "hydra"); os.makedirs(tmp / "sd15")
    for i, case in enumerate(gold["cases"]):
        torch.save(case["sample"], tmp / "data" / f"tok{i}.pth")
    with open(tmp / "ckpt" / "hydra" / "overrides.yaml", "w") as f:
        f.write(f"- +exp=224x400\n- seed={SR.SEED}\n")
    res = {"regen": run_driver(tmp, "regen", ["--regenerate-boxes", "--scheduler", "ddim"]),
           "on": run_driver(tmp, "on", ["--regenerate-boxes", "--scheduler", "ddim", "--resample", "5,2"]),
           "plain": run_driver(tmp, "plain", ["--resample", "5,2", "--scheduler", "ddim"]),
           "unipc": run_driver(tmp, "unipc", ["--regenerate-boxes", "--resample", "5,2"]),
           "bad": run_driver(tmp, "bad", ["--regenerate-boxes", "--scheduler", "ddim", "--resample", "5,0"]),
           "bad2": run_driver(tmp, "bad2", ["--regenerate-boxes", "--scheduler", "ddim", "--resample", "5"])}
    return tmp, res


def test_the_pair_reaches_the_pipeline_and_the_index(runs):
    tmp, res = runs
    assert res["on"].returncode == 0, res["on"].stderr[-2000:]
    assert res["regen"].returncode == 0, res["regen"].stderr[-2000:]
    with open(tmp / "on.jsonl.resample") as f:
        seen = [json.loads(ln) for ln in f]
    assert seen and all(r["resample"] == [5, 2] and r["kind"] == "tuple" for r in seen)
    with open(tmp / "regen.jsonl.resample") as f:
        assert all(json.loads(ln)["resample"] is None for ln in f)
    on, off = json.load(open(tmp / "on" / "index.json")), json.load(open(tmp / "regen" / "index.json"))
    assert on["resample"] == [5, 2] and "resample" not in off
    assert {k: v for k, v in on.items() if k != "resample"} == off
    assert list(on) == ["world", "seed", "gather_images", "resample", "generations"]
    # the stub ignores the switch: the same calls (masks, latents, seeds) and the same pictures
    assert SR.log(tmp, "on") == [dict(r, gen_id=o["gen_id"]) for r, o in zip(SR.log(tmp, "regen"), SR.log(tmp, "on"))]
    assert SR.pngs(tmp, "on") == SR.pngs(tmp, "regen") and all(SR.read(tmp, "on", n) == SR.read(tmp, "regen", n) for n in SR.pngs(tmp, "on"))


def test_the_flag_is_refused_where_it_has_no_meaning(runs):
    tmp, res = runs
    for name, what in (("plain", "--regenerate-boxes only"), ("unipc", "--scheduler ddim"), ("bad", "two integers >= 1"), ("bad2", "two integers >= 1")):
        assert res[name].returncode != 0 and what in res[name].stderr, (name, res[name].stderr[-500:])
        assert not os.path.exists(tmp / name / "index.json") and not os.path.exists(tmp / f"{name}.jsonl")


@pytest.mark.gpu
def test_resample_on_the_real_pipeline(dev, tmp_path):
    """A tiny checkpoint in the reference layout, DDIM, the ground-truth views encoded by the HIP VAE encoder, masks from the samples' own
    boxes, --resample 2,2 at 4 steps (6 step launches, one jump)."""
    import importlib.util
    import yaml
    from PIL import Image
    from magicdrive_amd import dataset as DS
    from magicdrive_amd.networks import spec
    from magicdrive_amd.networks.autoencoder_kl import AutoencoderKL
    from magicdrive_amd.networks.unet_2d_condition_multiview import UNet2DConditionModelMultiview
    from magicdrive_amd.networks.unet_addon_rawbox import BEVControlNetModel
    from magicdrive_amd.schedulers import resample_actions
    sp = importlib.util.spec_from_file_location("mdx_tools_sample_rs", os.path.join(ROOT, "tools", "sample.py"))
    sample = importlib.util.module_from_spec(sp); sp.loader.exec_module(sample)
    cfg = spec.TINY_CONFIG
    ckpt, sd15, data, out = tmp_path / "ckpt", tmp_path / "sd15", tmp_path / "data", tmp_path / "out"
    UNet2DConditionModelMultiview.from_config(cfg, seed=0).save_pretrained(str(ckpt / "unet"))
    BEVControlNetModel.from_config(cfg, seed=1).save_pretrained(str(ckpt / "controlnet"))
    os.makedirs(ckpt / "hydra"); os.makedirs(sd15 / "scheduler"); os.makedirs(data)
    with open(ckpt / "hydra" / "overrides.yaml", "w") as f:
        yaml.safe_dump(["+exp=224x400", "runner.validation_times=2", "seed=7"], f)
    with open(sd15 / "scheduler" / "scheduler_config.json", "w") as f:
        f.write('{"_class_name": "PNDMScheduler", "beta_end": 0.012, "beta_schedule": "scaled_linear", "beta_start": 0.00085, '
                '"num_train_timesteps": 1000, "set_alpha_to_one": false, "skip_prk_steps": true, "steps_offset": 1, "clip_sample": false}')
    AutoencoderKL.from_config(spec.VAE_TINY_CONFIG, 5, with_encoder=True).save_pretrained(str(sd15 / "vae"))
    G = torch.load(os.path.join(ROOT, "tests", "golden", "sample_preprocess.pt"), weights_only=False)
    for i, case in enumerate(G["cases"][:2]):
        smp = dict(case["sample"])
        m = smp["gt_masks_bev"]
        smp["gt_masks_bev"] = m.repeat_interleave(10, 1).repeat_interleave(10, 2) if isinstance(m, torch.Tensor) else np.repeat(np.repeat(m, 10, 1), 10, 2)
        smp["img"] = torch.rand(6, 3, 224, 400, generator=torch.Generator().manual_seed(40 + i)) * 2 - 1
        torch.save(smp, data / f"tok{i}.pth")
    steps = "runner.pipeline_param.num_inference_steps=4"
    assert resample_actions(4, 2, 2).count("step") == 6
    sample.main(["--ckpt", str(ckpt), "--sd15", str(sd15), "--data", str(data), "--out", str(out), "--scheduler", "ddim", "--batch-size", "2",
                 "--prompt-embeds", "--device", str(dev), "--regenerate-boxes", "--resample", "2,2", steps])
    files = sorted(f_ for f_ in os.listdir(out) if f_.endswith(".png"))
    assert len(files) == 2 * 2 * 6, files[:8]
    idx = json.load(open(out / "index.json"))
    assert idx["resample"] == [2, 2]
    assert [(g["scene"], g["gen"]) for g in idx["generations"]] == [(0, 0), (0, 1), (1, 0), (1, 1)]
    pipe = sample.build_pipe(str(ckpt), str(sd15), "ddim", dev, given_view=True)
    run = sample.resolve_run_config(str(ckpt), [steps])
    fs = DS.FolderSet(str(data))
    (kw, px, meta), = list(sample.iter_pipe_kwargs(fs, run, 2, with_meta=True))
    lat = sample.encode_given_views(pipe, px)
    masks = []
    for i in range(2):
        corners, kept = DS.project_box_corners(fs[i]["gt_bboxes_3d"], fs[i]["lidar2image"], fs[i]["img_aug_matrix"])
        masks.append(list(DS.box_keep_mask(corners, kept, (224, 400), (28, 50))))
    D = cfg["cross_attention_dim"]
    kw.update(prompt=None, prompt_embeds=torch.zeros(2, 77, D), negative_prompt_embeds=torch.zeros(2, 77, D))
    pipe.keep_masks, pipe.resample = masks, (2, 2)
    cl = [[lat[b, v] for v in range(6)] for b in range(2)]
    direct = pipe(conditional_latents=cl, generator=torch.Generator().manual_seed(7), **kw).images
    for b in range(2):
        for v in range(6):
            assert (np.asarray(direct[b][v]) == np.asarray(Image.open(out / f"{b}_gen0_view{v}.png"))).all(), (b, v)
    # the jumps matter: the same call without them gives other pictures
    pipe.resample = None
    plain = pipe(conditional_latents=cl, generator=torch.Generator().manual_seed(7), **kw).images
    assert any((np.asarray(plain[b][v]) != np.asarray(direct[b][v])).any() for b in range(2) for v in range(6))
