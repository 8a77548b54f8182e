#!/usr/bin/env python3
"""What pipe.composite_images costs per pipe() call, on one GPU: `python tools/composite_cost.py --scenes 64 --out profiles/composite_cost.jsonl`.

The region call of tools/region_keep_cost.py — SD-1.5-sized nets with seeded random weights, CFG, no boxes, --steps DDIM steps, the
given-view pipeline with the first three views of every scene given and masked — but with output_type="np": the SD-1.5-sized HIP VAE
decodes every view and the pictures reach the host.  Two modes, one pipeline each, built and warmed, then --repeats timed calls per
mode, interleaved in ONE process (the order alternates from repeat to repeat):
  off  composite_images = None: the region call as it is without the switch (clamp / permute / float by torch, one copy to the host);
  on   composite_images set (uint8 pictures for the three given views, composite_feather = --feather): one ops.ImageComposite launch
       behind the decoder, the pictures and the matte copied to the host.
A call is timed with the host clock around work that ends in a device synchronise.  Every line of the output is one JSON record, appended to
--out; nothing is asserted.

The "off" mode only uses what the pipeline had before the switch existed, so a copy of this script placed in the tools/ directory of a
checkout of the PARENT commit measures that commit (`--modes off --label parent`): alternate the two processes to compare "off" with the
parent.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from magicdrive_amd import _lib as L, schedulers, synthetic  # noqa: E402
from magicdrive_amd.networks import spec  # noqa: E402
from magicdrive_amd.networks.autoencoder_kl import AutoencoderKL  # noqa: E402
from magicdrive_amd.networks.unet_2d_condition_multiview import UNet2DConditionModelMultiview  # noqa: E402
from magicdrive_amd.networks.unet_addon_rawbox import BEVControlNetModel  # noqa: E402
from magicdrive_amd.pipeline.pipeline_bev_controlnet_given_view import StableDiffusionBEVControlNetGivenViewPipeline  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "composite_cost.jsonl"))
    ap.add_argument("--scenes", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--feather", type=int, default=4)
    ap.add_argument("--modes", default="off,on")
    ap.add_argument("--label", default="this", help="which checkout this process measures (free text, recorded)")
    ap.add_argument("--dtype", choices=["bf16", "fp16"], default="bf16")
    a = ap.parse_args()
    modes = a.modes.split(",")
    dev = torch.device("cuda:0")
    tdt = torch.float16 if a.dtype == "fp16" else torch.bfloat16
    cfg = spec.SD15_CONFIG
    unet = UNet2DConditionModelMultiview.from_config(cfg, seed=0, torch_dtype=tdt)
    cn = BEVControlNetModel.from_config(cfg, seed=1, torch_dtype=tdt)
    vae = AutoencoderKL.from_config(spec.VAE_SD15_CONFIG, 7, torch_dtype=tdt)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    f = open(a.out, "a")

    def emit(**rec):
        f.write(json.dumps(rec) + "\n"); f.flush()
        print(json.dumps(rec), flush=True)

    sc = synthetic.make_scene_batch(a.scenes, seed=1234, ctx_dim=cfg["cross_attention_dim"], max_len=None)
    g = lambda k: sc[k].to(dev)
    gen = torch.Generator().manual_seed(77)
    n_cam, given = 6, 3
    cl = [[(torch.randn(4, 28, 50, generator=gen) * 0.8).to(dev) if v < given else None for v in range(n_cam)] for _ in range(a.scenes)]
    masks, pics = [], []
    for _ in range(a.scenes):
        row, prow = [], []
        for v in range(n_cam):
            if v >= given:
                row.append(None); prow.append(None)
                continue
            m = torch.rand(28, 50, generator=gen)
            m[:9, :20] = 1.0
            m[12:20, 25:] = 0.0
            row.append(m)
            prow.append(torch.randint(0, 256, (224, 400, 3), generator=gen, dtype=torch.uint8))
        masks.append(row); pics.append(prow)
    kw = dict(prompt=None, image=g("bev_map"), camera_param=g("camera_param"), height=224, width=400, conditional_latents=cl, num_inference_steps=a.steps,
              guidance_scale=2.0, latents=g("latents"), prompt_embeds=g("prompt_embeds"), negative_prompt_embeds=g("negative_prompt_embeds"),
              output_type="np", bev_controlnet_kwargs={"bboxes_3d_data": None})

    def timed(pipe):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = pipe(**kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    pipes = {}
    for m in modes:
        pipes[m] = StableDiffusionBEVControlNetGivenViewPipeline(vae=vae, unet=unet, controlnet=cn, scheduler=schedulers.DDIMScheduler()).to(dev)
        pipes[m].keep_masks = masks
        if m == "on":
            pipes[m].composite_images, pipes[m].composite_feather = pics, a.feather
        timed(pipes[m]); timed(pipes[m])                      # build + capture, then one warm replay
    times = {m: [] for m in modes}
    finite, kept = {}, {}
    for rep in range(a.repeats):
        for m in (modes if rep % 2 == 0 else modes[::-1]):
            dt, out = timed(pipes[m])
            times[m].append(dt)
            finite[m] = bool((out.images == out.images).all())
            kept[m] = None if getattr(out, "matte", None) is None else round(float(out.matte.mean()), 4)
    for m in modes:
        t = sorted(times[m])
        emit(record="composite_cost", label=a.label, mode=m, build_id=L.build_id(), scenes=a.scenes, steps=a.steps, dtype=a.dtype, given_views=given,
             feather=a.feather if m == "on" else None, seconds=[round(x, 4) for x in times[m]], min_s=round(t[0], 4), median_s=round(t[len(t) // 2], 4),
             spread_s=round(t[-1] - t[0], 4), finite=finite[m], kept_fraction=kept[m], device=torch.cuda.get_device_name(0))
    f.close()


if __name__ == "__main__":
    main()
