"""CPU: tools/sample.py --regenerate-boxes end to end with a stub pipeline (this file, loaded through the driver's --pipe-factory hook).

Five scenes in batches of two, three generations each.  The stub samples nothing: a view is a 4 x 6 uint8 picture whose value says which
seed / camera / scene / generator draw produced it (tests/sample_stub.py); this file's subclass adds a stand-in VAE encoder and writes what
every pipe() call received to a JSON-lines log.
  without the flag   the files and index.json are, byte for byte, what the driver has always written: the expected bytes are rebuilt
                     here from the stub's formula and the driver's documented seeding, not from a second run of the driver;
  with the flag      the given-view pipeline class is asked for, every view of every scene is given (the encoded ground truth), pipe.keep_masks
                     holds one (28, 50) mask in [0, 1] per scene and view built from the sample's own boxes, there is one call per generation,
                     seeded as the plain loop is — so the stub's pictures, the file names and index.json equal the plain run's.
One case is marked gpu: the flag with the real pipeline on a tiny checkpoint, generation 0 against the same call composed by hand.
"""
import io
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
BATCH, TIMES, SEED = 2, 3, 7


class _Vae:
    dtype = torch.float32
    config = SimpleNamespace(scaling_factor=0.5)

    def encode(self, x):                                           # (b n, 3, H, W) -> a recognisable (b n, 4, 28, 50)
        mean = x.mean(dim=(1, 2, 3)).view(-1, 1, 1, 1).expand(-1, 4, 28, 50) * 2.0
        return SimpleNamespace(latent_dist=SimpleNamespace(mean=mean))


class RegionStub(sample_stub.StubPipe):
    _execution_device = torch.device("cpu")

    def __init__(self, given_view):
        self.vae = _Vae()
        self.keep_masks = None
        self.given_view = bool(given_view)

    def __call__(self, conditional_latents=None, **kw):
        km = self.keep_masks
        rec = dict(given_view=self.given_view, bs=int(kw["image"].shape[0]), height=kw["height"], width=kw["width"],
                   seed=int(kw["generator"].initial_seed()), gen_id=id(kw["generator"]),
                   cond=None if conditional_latents is None else [[None if v is None else [list(v.shape), float(v.flatten()[0])] for v in r] for r in conditional_latents],
                   masks=None if km is None else [[[list(m.shape), str(m.dtype), float(m.min()), float(m.max()), float(m.mean())] for m in r] for r in km])
        with open(os.environ["REGION_STUB_LOG"], "a") as f:
            f.write(json.dumps(rec) + "\n")
        return super().__call__(**kw)


def make(ckpt, sd15, scheduler, device, given_view):
    return RegionStub(given_view)


def run_driver(tmp_path, out_name, extra=()):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), os.environ.get("PYTHONPATH", "")]),
               CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="", OMP_NUM_THREADS="2", REGION_STUB_LOG=str(tmp_path / f"{out_name}.jsonl"))
    cmd = [sys.executable, os.path.join(ROOT, "tools", "sample.py"), "--ckpt", str(tmp_path / "ckpt"), "--sd15", str(tmp_path / "sd15"), "--data", str(tmp_path / "data"),
           "--out", str(tmp_path / out_name), "--prompt-embeds", "--pipe-factory", "test_sample_regions:make", "--dist-backend", "gloo", "--device", "cpu",
           "--batch-size", str(BATCH), f"runner.validation_times={TIMES}", *extra]
    return subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("sample_regions")
    gold = torch.load(os.path.join(ROOT, "tests", "golden", "sample_preprocess.pt"), weights_only=False)
    os.makedirs(tmp / "data"); os.makedirs(tmp / "ckpt" / "hydra"); os.makedirs(tmp / "sd15")
    for i, case in enumerate(gold["cases"]):
        torch.save(case["sample"], tmp / "data" / f"tok{i}.pth")
    with open(tmp / "ckpt" / "hydra" / "overrides.yaml", "w") as f:
        f.write(f"- +exp=224x400\n- seed={SEED}\n")
    res = {"plain": run_driver(tmp, "plain"), "regen": run_driver(tmp, "regen", ["--regenerate-boxes"]),
           "regen3": run_driver(tmp, "regen3", ["--regenerate-boxes", "--region-dilate", "3"]),
           "both": run_driver(tmp, "both", ["--regenerate-boxes", "--cond-on-view"])}
    return tmp, res, gold


def pngs(tmp, d):
    return sorted(x for x in os.listdir(tmp / d) if x.endswith(".png"))


def read(tmp, d, n):
    with open(tmp / d / n, "rb") as f:
        return f.read()


def log(tmp, d):
    with open(tmp / f"{d}.jsonl") as f:
        return [json.loads(ln) for ln in f]


def test_without_the_flag_the_output_is_what_it_always_was(runs):
    """Expected bytes from first principles: batches of two scenes in order, ONE generator per batch seeded with the run's seed whose state
    carries over the validation_times calls (the stub draws once per call), view value = (seed * 7 + cam * 13 + tag + draw) % 256 with the
    tag a function of the scene's BEV map; PNG files <scene>_gen<gen>_view<v>.png; index.json = {world, seed, gather_images, generations}."""
    from PIL import Image
    from magicdrive_amd import dataset as DS
    tmp, res, gold = runs
    assert res["plain"].returncode == 0, res["plain"].stderr[-2000:]
    data = DS.FolderSet(str(tmp / "data"))
    expect, index = {}, []
    for s0 in range(0, 5, BATCH):
        g = torch.Generator().manual_seed(SEED)
        scenes = list(range(s0, min(s0 + BATCH, 5)))
        bev = [DS.preprocess_fn(data[s])["bev_map_with_aux"][0] for s in scenes]
        for ti in range(TIMES):
            draw = int(torch.randint(0, 97, [1], generator=g))
            for s, b in zip(scenes, bev):
                tag = int(b.float().abs().sum().item() * 1000) % 251
                names = []
                for cam in range(6):
                    buf = io.BytesIO()
                    Image.fromarray(np.full((4, 6, 3), (SEED * 7 + cam * 13 + tag + draw) % 256, dtype=np.uint8)).save(buf, format="PNG")
                    names.append(f"{s}_gen{ti}_view{cam}.png")
                    expect[names[-1]] = buf.getvalue()
                index.append(dict(scene=s, gen=ti, rank=0, seed=SEED, files=names))
    assert pngs(tmp, "plain") == sorted(expect)
    for n, want in expect.items():
        assert read(tmp, "plain", n) == want, n
    index.sort(key=lambda r: (r["scene"], r["gen"]))
    assert read(tmp, "plain", "index.json").decode() == json.dumps(dict(world=1, seed=SEED, gather_images=False, generations=index), indent=1)
    assert res["plain"].stdout.strip().splitlines()[-1] == f"sampled 5 scenes x {TIMES} on 1 rank(s) -> {tmp / 'plain'}"
    calls = log(tmp, "plain")
    assert len(calls) == 3 * TIMES and all(c["given_view"] is False and c["cond"] is None and c["masks"] is None for c in calls)


@pytest.mark.parametrize("d", ["regen", "regen3"])
def test_regenerate_boxes_reaches_the_pipeline(runs, d):
    from magicdrive_amd import dataset as DS
    tmp, res, gold = runs
    assert res[d].returncode == 0, res[d].stderr[-2000:]
    dilate = 3 if d == "regen3" else 1
    calls = log(tmp, d)
    assert len(calls) == 3 * TIMES and [c["bs"] for c in calls] == [2] * TIMES + [2] * TIMES + [1] * TIMES
    data = DS.FolderSet(str(tmp / "data"))
    for k, c in enumerate(calls):
        s0 = (k // TIMES) * BATCH
        assert c["given_view"] is True and (c["height"], c["width"], c["seed"]) == (224, 400, SEED)
        assert c["gen_id"] == calls[(k // TIMES) * TIMES]["gen_id"]                    # one generator per batch, carried over the generations
        assert len(c["cond"]) == c["bs"] == len(c["masks"])
        for bi in range(c["bs"]):
            ex = data[s0 + bi]
            px = DS.preprocess_fn(ex)["pixel_values"][0]
            corners, kept = DS.project_box_corners(ex["gt_bboxes_3d"], ex["lidar2image"], ex["img_aug_matrix"])
            want = DS.box_keep_mask(corners, kept, (224, 400), (28, 50), dilate=dilate)
            assert len(c["cond"][bi]) == 6 and len(c["masks"][bi]) == 6
            for v in range(6):
                shape, first = c["cond"][bi][v]                                         # every view given: the encoded ground truth
                assert shape == [4, 28, 50] and first == pytest.approx(float(px[v].mean()) * 2.0 * 0.5, abs=1e-6)
                mshape, mdtype, lo, hi, mean = c["masks"][bi][v]
                assert mshape == [28, 50] and mdtype == "torch.float32" and 0.0 <= lo <= hi <= 1.0
                assert (lo, hi, mean) == (float(want[v].min()), float(want[v].max()), pytest.approx(float(want[v].mean()), abs=1e-7))
    means = [m[4] for c in calls for r in c["masks"] for m in r]
    assert min(means) < 0.9 and max(means) == 1.0                                       # boxes cover something; the scene without boxes keeps everything
    # seeded as the plain loop: the stub's pictures, the file names and the index are the plain run's
    assert pngs(tmp, d) == pngs(tmp, "plain") and len(pngs(tmp, d)) == 5 * TIMES * 6
    for n in pngs(tmp, d) + ["index.json"]:
        assert read(tmp, d, n) == read(tmp, "plain", n), n
    assert res[d].stdout.strip().splitlines()[-1] == f"sampled 5 scenes x {TIMES} on 1 rank(s) -> {tmp / d}"


def test_dilation_grows_the_regenerated_region(runs):
    tmp, res, gold = runs
    m1 = [m[4] for c in log(tmp, "regen") for r in c["masks"] for m in r]
    m3 = [m[4] for c in log(tmp, "regen3") for r in c["masks"] for m in r]
    assert all(b <= a for a, b in zip(m1, m3)) and sum(m3) < sum(m1)


def test_the_two_given_view_modes_exclude_each_other(runs):
    tmp, res, gold = runs
    assert res["both"].returncode != 0 and "pass one of the two" in res["both"].stderr
    assert not os.path.exists(tmp / "both.jsonl")


@pytest.mark.gpu
def test_regenerate_boxes_on_the_real_pipeline(dev, tmp_path):
    """The flag on the GPU: a tiny checkpoint in the reference layout, UniPC (what build_pipe installs), the ground-truth views encoded by the
    HIP VAE encoder, masks from the samples' own boxes.  validation_times x 6 files per scene, and the driver's generation 0 is bit-identical
    to encoding, building the masks and calling the given-view pipeline by hand."""
    import importlib.util
    import yaml
    from PIL import Image
    from magicdrive_amd import dataset as DS
    from magicdrive_amd.networks import spec
    from magicdrive_amd.networks.autoencoder_kl import AutoencoderKL
    from magicdrive_amd.networks.unet_2d_condition_multiview import UNet2DConditionModelMultiview
    from magicdrive_amd.networks.unet_addon_rawbox import BEVControlNetModel
    sp = importlib.util.spec_from_file_location("mdx_tools_sample_rg", os.path.join(ROOT, "tools", "sample.py"))
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
    steps = "runner.pipeline_param.num_inference_steps=3"
    sample.main(["--ckpt", str(ckpt), "--sd15", str(sd15), "--data", str(data), "--out", str(out), "--scheduler", "unipc", "--batch-size", "2",
                 "--prompt-embeds", "--device", str(dev), "--regenerate-boxes", steps])
    files = sorted(f_ for f_ in os.listdir(out) if f_.endswith(".png"))
    assert len(files) == 2 * 2 * 6, files[:8]
    index = json.load(open(out / "index.json"))["generations"]
    assert [(g["scene"], g["gen"]) for g in index] == [(0, 0), (0, 1), (1, 0), (1, 1)] and all(set(g) == {"scene", "gen", "rank", "seed", "files"} for g in index)
    pipe = sample.build_pipe(str(ckpt), str(sd15), "unipc", dev, given_view=True)
    run = sample.resolve_run_config(str(ckpt), [steps])
    fs = DS.FolderSet(str(data))
    (kw, px, meta), = list(sample.iter_pipe_kwargs(fs, run, 2, with_meta=True))
    lat = sample.encode_given_views(pipe, px)
    assert tuple(lat.shape) == (2, 6, 4, 28, 50)
    masks = []
    for i in range(2):
        corners, kept = DS.project_box_corners(fs[i]["gt_bboxes_3d"], fs[i]["lidar2image"], fs[i]["img_aug_matrix"])
        masks.append(list(DS.box_keep_mask(corners, kept, (224, 400), (28, 50))))
    assert any(float(m.min()) < 1.0 for r in masks for m in r)
    D = cfg["cross_attention_dim"]
    kw.update(prompt=None, prompt_embeds=torch.zeros(2, 77, D), negative_prompt_embeds=torch.zeros(2, 77, D))
    pipe.keep_masks = masks
    direct = pipe(conditional_latents=[[lat[b, v] for v in range(6)] for b in range(2)], generator=torch.Generator().manual_seed(7), **kw).images
    for b in range(2):
        for v in range(6):
            assert (np.asarray(direct[b][v]) == np.asarray(Image.open(out / f"{b}_gen0_view{v}.png"))).all(), (b, v)
    # the masks matter: the same call with every view kept whole gives other pictures where a box was regenerated
    pipe.keep_masks = None
    whole = pipe(conditional_latents=[[lat[b, v] for v in range(6)] for b in range(2)], generator=torch.Generator().manual_seed(7), **kw).images
    assert any((np.asarray(whole[b][v]) != np.asarray(direct[b][v])).any() for b in range(2) for v in range(6))
