#!/usr/bin/env python3
"""What pipe(..., eta > 0) costs per call, on one GPU: `python tools/eta_cost.py --scenes 64 --out profiles/eta_cost.jsonl`.

SD-1.5-sized nets with seeded random weights, CFG, no boxes, --steps DDIM steps, output_type="latent", the plain pipeline.  Two modes on ONE
pipeline (they differ in the call's eta only, so each has its own cached plan), built and warmed, then --repeats timed calls per mode,
interleaved in ONE process (the order alternates from repeat to repeat):
  eta0   eta = 0: the deterministic call, whose plan is today's (ops.DdimStep);
  eta1   eta = --eta (default 1): the stochastic plan — ops.DdimEtaStep in the scheduler op's place, one Philox block per four latents.
A call is timed with the host clock around work that ends in a device synchronise.  Every line of the output is one JSON record, appended to
--out; nothing is asserted and no threshold is fixed in advance.  The expectation to check in the records: "eta0" equals the parent commit's
call within the spread of the repeats, and "eta1" costs the same per step (the scheduler op is one small launch behind ~600 others).

The "eta0" mode only uses what the pipeline had before eta > 0 existed, so a copy of this script placed in the tools/ directory of a
checkout of the PARENT commit measures that commit (`--modes eta0 --label parent`): alternate the two processes.
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
from magicdrive_amd.networks.unet_2d_condition_multiview import UNet2DConditionModelMultiview  # noqa: E402
from magicdrive_amd.networks.unet_addon_rawbox import BEVControlNetModel  # noqa: E402
from magicdrive_amd.pipeline.pipeline_bev_controlnet import StableDiffusionBEVControlNetPipeline  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eta_cost.jsonl"))
    ap.add_argument("--scenes", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--modes", default="eta0,eta1")
    ap.add_argument("--eta", type=float, default=1.0, help="eta of the eta1 mode")
    ap.add_argument("--label", default="this", help="which checkout this process measures (free text, recorded)")
    ap.add_argument("--dtype", choices=["bf16", "fp16"], default="bf16")
    a = ap.parse_args()
    modes = a.modes.split(",")
    dev = torch.device("cuda:0")
    tdt = torch.float16 if a.dtype == "fp16" else torch.bfloat16
    cfg = spec.SD15_CONFIG
    unet = UNet2DConditionModelMultiview.from_config(cfg, seed=0, torch_dtype=tdt)
    cn = BEVControlNetModel.from_config(cfg, seed=1, torch_dtype=tdt)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    f = open(a.out, "a")

    def emit(**rec):
        f.write(json.dumps(rec) + "\n"); f.flush()
        print(json.dumps(rec), flush=True)

    sc = synthetic.make_scene_batch(a.scenes, seed=1234, ctx_dim=cfg["cross_attention_dim"], max_len=None)
    g = lambda k: sc[k].to(dev)
    kw = dict(prompt=None, image=g("bev_map"), camera_param=g("camera_param"), height=224, width=400, num_inference_steps=a.steps,
              guidance_scale=2.0, latents=g("latents"), prompt_embeds=g("prompt_embeds"), negative_prompt_embeds=g("negative_prompt_embeds"),
              output_type="latent", bev_controlnet_kwargs={"bboxes_3d_data": None})
    pipe = StableDiffusionBEVControlNetPipeline(unet=unet, controlnet=cn, scheduler=schedulers.DDIMScheduler()).to(dev)
    eta_of = {"eta0": 0.0, "eta1": a.eta}

    def timed(m):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = pipe(generator=torch.Generator().manual_seed(5), eta=eta_of[m], **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    for m in modes:
        timed(m); timed(m)                                    # build + capture, then one warm replay
    times = {m: [] for m in modes}
    finite = {}
    for rep in range(a.repeats):
        for m in (modes if rep % 2 == 0 else modes[::-1]):
            dt, out = timed(m)
            times[m].append(dt)
            finite[m] = bool(torch.isfinite(out.images).all())
    for m in modes:
        t = sorted(times[m])
        emit(record="eta_cost", label=a.label, mode=m, eta=eta_of[m], build_id=L.build_id(), scenes=a.scenes, steps=a.steps, dtype=a.dtype,
             seconds=[round(x, 4) for x in times[m]], min_s=round(t[0], 4), median_s=round(t[len(t) // 2], 4), spread_s=round(t[-1] - t[0], 4),
             s_per_step=round(t[len(t) // 2] / a.steps, 5), finite=finite[m], device=torch.cuda.get_device_name(0))
    f.close()


if __name__ == "__main__":
    main()
