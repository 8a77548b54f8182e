"""-m gpu: pipe.health — per-scene sample health from device-side records (ops.GroupStats inside the captured step graphs), on the tiny nets.

Scenes without boxes are independent of each other (the text context is per scene, cross-view attention couples the cameras of one scene
only), so a NaN planted in ONE scene's prompt embedding must cost that scene and nothing else: its batchmates keep the bits of the clean
run, the bad scene is named with the step it died at, and with the switch off nothing at all changes.  Planting a NaN in an input provokes
no fault: it is data.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import scene  # noqa: E402
from magicdrive_amd import schedulers  # noqa: E402
from magicdrive_amd.networks import spec  # noqa: E402

STEPS = 4
NAN = float("nan")


def make_pipe(dev, scheduler=None, torch_dtype=None, vae=None):
    from magicdrive_amd.networks.unet_2d_condition_multiview import UNet2DConditionModelMultiview
    from magicdrive_amd.networks.unet_addon_rawbox import BEVControlNetModel
    from magicdrive_amd.pipeline.pipeline_bev_controlnet import StableDiffusionBEVControlNetPipeline
    cfg = spec.TINY_CONFIG
    kw = {} if torch_dtype is None else {"torch_dtype": torch_dtype}
    pipe = StableDiffusionBEVControlNetPipeline(vae=vae, unet=UNet2DConditionModelMultiview.from_config(cfg, 0, **kw),
                                                controlnet=BEVControlNetModel.from_config(cfg, 1, **kw)).to(dev)
    if scheduler is not None:
        pipe.scheduler = scheduler.from_config(pipe.scheduler.config)
    return pipe


def inputs(n, poison=None):
    sc = scene(spec.TINY_CONFIG, n, None)
    if poison is not None:
        sc["prompt_embeds"][poison, 0, 0] = NAN
    return sc


def call(pipe, sc, output_type="latent", **kw):
    return pipe(prompt=None, image=sc["bev_map"], camera_param=sc["camera_param"], height=224, width=400, num_inference_steps=STEPS,
                guidance_scale=2.0, latents=sc["latents"], prompt_embeds=sc["prompt_embeds"], negative_prompt_embeds=sc["negative_prompt_embeds"],
                output_type=output_type, bev_controlnet_kwargs={"bboxes_3d_data": None}, **kw)


@pytest.fixture(scope="module")
def pipe(dev):
    return make_pipe(dev)


@pytest.fixture(scope="module")
def clean(pipe):
    """The clean 3-scene call with the switch off: the latents every other test compares with.  Computed once, never modified."""
    assert pipe.health is None
    out = call(pipe, inputs(3))
    assert out.health is None
    return out.images.clone()


def test_clean_run_is_ok_and_changes_no_bit(pipe, clean):
    pipe.health = "trace"
    try:
        out = call(pipe, inputs(3))
    finally:
        pipe.health = None
    h = out.health
    assert h.ok == [True, True, True] and h.first_bad_step == [-1, -1, -1] and h.bad_scenes == [] and h.image_nonfinite is None
    assert torch.equal(out.images, clean), "health='trace' changed the latents"
    assert h.trace.shape == (STEPS, 3, 6, 4) and h.final.shape == (3, 6, 4) and np.array_equal(h.final, h.trace[-1])
    assert (h.trace[..., 0] == 0).all()
    # the last row describes the latents that were returned: absmax bit-exact, the moments within fp32 summation error of float64
    lat = clean.double().cpu()                                                   # [3, 6, 4, 28, 50]
    assert np.array_equal(h.final[..., 1], lat.abs().amax(dim=(2, 3, 4)).float().numpy())
    assert np.allclose(h.final[..., 2], lat.sum(dim=(2, 3, 4)).numpy(), rtol=0, atol=17 * 2.0 ** -24 * float(lat.abs().sum(dim=(2, 3, 4)).max()))
    assert np.allclose(h.final[..., 3], (lat * lat).sum(dim=(2, 3, 4)).numpy(), rtol=17 * 2.0 ** -24, atol=0)
    assert (h.trace[:, :, :, 1] > 0).all(), "a step's row was not written"
    # without return_dict the tuple is what it was
    pipe.health = "trace"
    try:
        tup = call(pipe, inputs(3), return_dict=False)
    finally:
        pipe.health = None
    assert isinstance(tup, tuple) and len(tup) == 2 and tup[1] is None and torch.equal(tup[0], clean)


def test_poisoned_scene_costs_that_scene_only(pipe, clean):
    from magicdrive_amd.pipeline.pipeline_bev_controlnet import SampleHealthError
    sc = inputs(3, poison=1)
    outs = {}
    for mode in ("trace", "final"):
        pipe.health = mode
        try:
            outs[mode] = call(pipe, sc)
        finally:
            pipe.health = None
    tr, fi = outs["trace"].health, outs["final"].health
    assert tr.ok == [True, False, True] and fi.ok == [True, False, True]
    assert tr.first_bad_step == [-1, 0, -1] and fi.first_bad_step is None and fi.trace is None
    assert tr.bad_scenes == [1]
    for out in outs.values():
        assert torch.equal(out.images[0], clean[0]) and torch.equal(out.images[2], clean[2]), "a batchmate of the poisoned scene changed"
        assert not torch.isfinite(out.images[1]).all()
    assert (tr.trace[:, 1, :, 0] > 0).all() and (tr.trace[:, 0, :, 0] == 0).all() and (tr.trace[:, 2, :, 0] == 0).all()
    # the final record counts exactly what the returned latents hold
    want = (~torch.isfinite(outs["final"].images)).sum(dim=(2, 3, 4)).cpu().numpy()
    assert np.array_equal(fi.final[..., 0], want) and np.array_equal(tr.final[..., 0], want)
    # "raise": the same call raises, naming the scene; the records and the output ride on the exception
    pipe.health, pipe.health_action = "final", "raise"
    try:
        with pytest.raises(SampleHealthError) as ei:
            call(pipe, sc)
        assert ei.value.bad_scenes == [1] and "[1]" in str(ei.value) and ei.value.health.ok == [True, False, True]
        assert torch.equal(ei.value.output.images[0], clean[0])
        assert call(pipe, inputs(3)).health.ok == [True, True, True]            # a clean call does not raise
    finally:
        pipe.health, pipe.health_action = None, "flag"


def test_eager_steps_and_callback_give_the_same_records(pipe, clean):
    sc = inputs(3, poison=1)
    pipe.health = "trace"
    try:
        graph = call(pipe, sc).health
        pipe.use_graph = False
        seen = []
        eager = call(pipe, sc, callback=lambda i, t, lat: seen.append(i)).health
    finally:
        pipe.health, pipe.use_graph = None, True
    assert seen == list(range(STEPS))
    assert eager.ok == graph.ok == [True, False, True] and eager.first_bad_step == graph.first_bad_step
    assert np.array_equal(eager.trace.view(np.int32), graph.trace.view(np.int32))


def test_scene_index_is_global_over_chunks(dev):
    """Two scene chunks on two streams, 4 scenes, scene 2 poisoned: it is local scene 0 of chunk 1 and must be reported as 2."""
    pipe = make_pipe(dev)
    pipe.streams, pipe.min_scenes_per_stream = 2, 1
    ref = call(pipe, inputs(4)).images.clone()
    pipe.health = "trace"
    out = call(pipe, inputs(4, poison=2))
    assert len(pipe._plans) == 4, "expected two chunk plans per switch position"
    assert out.health.ok == [True, True, False, True] and out.health.first_bad_step == [-1, -1, 0, -1] and out.health.bad_scenes == [2]
    assert out.health.trace.shape == (STEPS, 4, 6, 4)
    for i in (0, 1, 3):
        assert torch.equal(out.images[i], ref[i]), i
    pipe.health = "final"
    assert call(pipe, inputs(4, poison=2)).health.ok == [True, True, False, True]


@pytest.mark.parametrize("case", ["unipc", "fp16"])
def test_other_scheduler_and_other_build(dev, case):
    pipe = make_pipe(dev, schedulers.UniPCMultistepScheduler if case == "unipc" else None, torch.float16 if case == "fp16" else None)
    ref = call(pipe, inputs(3)).images.clone()
    pipe.health = "trace"
    good, out = call(pipe, inputs(3)), call(pipe, inputs(3, poison=1))
    assert good.health.ok == [True, True, True] and torch.equal(good.images, ref)
    assert out.health.ok == [True, False, True] and out.health.first_bad_step == [-1, 0, -1]
    assert torch.equal(out.images[0], ref[0]) and torch.equal(out.images[2], ref[2])


def test_absmax_threshold_flags_a_finite_blow_up(pipe, clean):
    """No default threshold: a finite 1e30 in the initial latents of scene 1 goes unflagged unless it turns non-finite on its way; with a
    threshold the scene is bad either way.  On the clean run the threshold alone decides: below the latent range every scene is bad at step 0
    with a non-finite count of zero, far above it none is."""
    sc = inputs(3)
    sc["latents"][1, 0, 0, 0] = 1e30
    pipe.health, pipe.health_absmax = "trace", 1e6
    try:
        h = call(pipe, sc).health
        assert h.ok == [True, False, True] and h.first_bad_step == [-1, 0, -1]
        pipe.health_absmax = 1e-3
        low = call(pipe, inputs(3)).health
        assert low.ok == [False, False, False] and low.first_bad_step == [0, 0, 0] and (low.trace[..., 0] == 0).all()
        pipe.health_absmax = 1e6
        assert call(pipe, inputs(3)).health.ok == [True, True, True]
    finally:
        pipe.health, pipe.health_absmax = None, None


def test_sample_driver_skips_a_poisoned_scene(dev, tmp_path):
    """tools/sample.py --health skip on the GPU, batches of two: scene 1's BEV map carries one NaN.  Its six PNGs are not written, index.json
    names it with the step it died at, and every other file — its batchmate's included — has the bytes of the clean run without the option."""
    import importlib.util
    import json
    import os
    import yaml
    from magicdrive_amd.networks.autoencoder_kl import AutoencoderKL
    from magicdrive_amd.networks.unet_2d_condition_multiview import UNet2DConditionModelMultiview
    from magicdrive_amd.networks.unet_addon_rawbox import BEVControlNetModel
    here = os.path.dirname(os.path.abspath(__file__))
    sp = importlib.util.spec_from_file_location("mdx_tools_sample", os.path.join(os.path.dirname(here), "tools", "sample.py"))
    sample = importlib.util.module_from_spec(sp); sp.loader.exec_module(sample)
    cfg = spec.TINY_CONFIG
    ckpt = tmp_path / "ckpt"
    UNet2DConditionModelMultiview.from_config(cfg, seed=0).save_pretrained(str(ckpt / "unet"))
    BEVControlNetModel.from_config(cfg, seed=1).save_pretrained(str(ckpt / "controlnet"))
    os.makedirs(ckpt / "hydra")
    with open(ckpt / "hydra" / "overrides.yaml", "w") as f:
        yaml.safe_dump(["+exp=224x400", "runner.validation_times=1", "seed=7"], f)
    sd15 = tmp_path / "sd15"
    os.makedirs(sd15 / "scheduler")
    with open(sd15 / "scheduler" / "scheduler_config.json", "w") as f:
        f.write('{"_class_name": "PNDMScheduler", "beta_end": 0.012, "beta_schedule": "scaled_linear", "beta_start": 0.00085, '
                '"num_train_timesteps": 1000, "set_alpha_to_one": false, "skip_prk_steps": true, "steps_offset": 1, "clip_sample": false}')
    AutoencoderKL.from_config(spec.VAE_TINY_CONFIG, 5).save_pretrained(str(sd15 / "vae"))
    G = torch.load(os.path.join(here, "golden", "sample_preprocess.pt"), weights_only=False)
    for name, poison in (("clean", None), ("poisoned", 1)):
        os.makedirs(tmp_path / name)
        for i, case in enumerate(G["cases"][:3]):
            smp = dict(case["sample"])
            m = torch.as_tensor(np.asarray(smp["gt_masks_bev"])).float().repeat_interleave(10, 1).repeat_interleave(10, 2)   # 8 x 20 x 20 -> 8 x 200 x 200
            if i == poison:
                m[0, 100, 100] = NAN
            smp["gt_masks_bev"] = m
            torch.save(smp, tmp_path / name / f"tok{i}.pth")
    argv = lambda data, out: ["--ckpt", str(ckpt), "--sd15", str(sd15), "--data", str(tmp_path / data), "--out", str(tmp_path / out), "--scheduler", "unipc",
                              "--batch-size", "2", "--prompt-embeds", "--device", str(dev), "runner.pipeline_param.num_inference_steps=3", "fix_seed_within_batch=true"]
    sample.main(argv("clean", "out_clean"))
    with pytest.raises(SystemExit) as ei:
        sample.main(argv("poisoned", "out_skip") + ["--health", "skip"])
    assert ei.value.code == 3
    png = lambda d: sorted(f_ for f_ in os.listdir(tmp_path / d) if f_.endswith(".png"))
    assert len(png("out_clean")) == 3 * 6
    assert sorted(set(png("out_clean")) - set(png("out_skip"))) == [f"1_gen0_view{v}.png" for v in range(6)] and set(png("out_skip")) < set(png("out_clean"))
    for n in png("out_skip"):
        with open(tmp_path / "out_skip" / n, "rb") as fa, open(tmp_path / "out_clean" / n, "rb") as fb:
            assert fa.read() == fb.read(), n
    gens = json.load(open(tmp_path / "out_skip" / "index.json"))["generations"]
    assert [(g["scene"], g["ok"], g["first_bad_step"], len(g["files"])) for g in gens] == [(0, True, -1, 6), (1, False, 0, 0), (2, True, -1, 6)]
    assert gens[1]["nonfinite"] > 0 and gens[0]["nonfinite"] == 0 and gens[0]["absmax"] > 0
    assert "ok" not in json.load(open(tmp_path / "out_clean" / "index.json"))["generations"][0]


class OneNaNVAE:
    """The tiny HIP VAE with ONE NaN planted in the input of one view: the latents the sampler returns are clean, the decoded view is not."""

    def __init__(self, vae, view):
        self.vae, self.view, self.config = vae, view, vae.config

    def to(self, device):
        self.vae.to(device)
        return self

    def parameters(self):
        return self.vae.parameters()

    def decode(self, x):
        x = x.clone()
        x[self.view, 0, 0, 0] = NAN
        return self.vae.decode(x)


def test_decoded_images_are_checked_too(dev):
    from magicdrive_amd.networks.autoencoder_kl import AutoencoderKL
    pipe = make_pipe(dev, vae=OneNaNVAE(AutoencoderKL.from_config(spec.VAE_TINY_CONFIG, 5), view=7))
    pipe.health = "final"
    out = call(pipe, inputs(2), output_type="np")
    h = out.health
    assert h.image_nonfinite.shape == (2, 6) and h.image_nonfinite[1, 1] > 0
    assert h.image_nonfinite.sum() == h.image_nonfinite[1, 1], "a NaN in one view's input reached another view"
    assert (h.final[..., 0] == 0).all() and h.ok == [True, False]
    assert out.images.shape == (2, 6, 224, 400, 3)                              # the pictures of the bad scene are still returned
    assert np.isfinite(out.images[0]).all()
    pipe.health = None
    off = call(pipe, inputs(2), output_type="np")
    assert off.health is None and np.array_equal(off.images[0], out.images[0])
