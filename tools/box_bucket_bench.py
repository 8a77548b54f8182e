#!/usr/bin/env python3
"""What pipe.box_bucket buys in a validation-like run, on one GPU: `python tools/box_bucket_bench.py --out profiles/box_bucket_bench.jsonl`.

1. A sequence of 24 pipe() calls at SD-1.5 size (2 scenes, CFG, 20 DDIM steps, random weights) whose padded box count L is drawn from a
   fixed seeded list in 1..64 — the reference's validation flow pads the boxes of every batch to that batch's maximum — run with
   box_bucket=None and with box_bucket=16, interleaved call by call in one process.  Per call: wall time and whether a plan was built.
2. Steady state of a call at L = 32 on an exact plan, a capacity-32 and a capacity-48 dynamic plan: --repeats (default 3) repeats each,
   interleaved, and the summed time of the step's text-context attention launches (the 23 launches the new kernel takes over), timed op by op.
   --scene-boxes adds the same two capacities with pipe.scene_boxes = True (one key count per view: workgroups of one launch walk different
   tile counts); the exact form is what the pipeline computes with both switches off.  --steady-only skips part 1.
Every line of the output file is one JSON record; nothing is asserted."""
import argparse
import json
import os
import random
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from magicdrive_amd import _lib as L, ops as O, schedulers, synthetic  # noqa: E402
from magicdrive_amd.networks import spec  # noqa: E402
from magicdrive_amd.networks.unet_2d_condition_multiview import UNet2DConditionModelMultiview  # noqa: E402
from magicdrive_amd.networks.unet_addon_rawbox import BEVControlNetModel  # noqa: E402
from magicdrive_amd.pipeline.pipeline_bev_controlnet import StableDiffusionBEVControlNetPipeline  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "box_bucket_bench.jsonl"))
    ap.add_argument("--calls", type=int, default=24)
    ap.add_argument("--scenes", type=int, default=2)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--bucket", type=int, default=16)
    ap.add_argument("--dtype", choices=["bf16", "fp16"], default="bf16")
    ap.add_argument("--scene-boxes", action="store_true", help="steady state: also time pipe.scene_boxes = True at both capacities")
    ap.add_argument("--repeats", type=int, default=3, help="steady state: timed calls per form (interleaved); min and median are reported")
    ap.add_argument("--steady-only", action="store_true", help="skip the validation-like sequence")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    tdt = torch.float16 if a.dtype == "fp16" else torch.bfloat16
    cfg = spec.SD15_CONFIG
    unet = UNet2DConditionModelMultiview.from_config(cfg, seed=0, torch_dtype=tdt)
    cn = BEVControlNetModel.from_config(cfg, seed=1, torch_dtype=tdt)
    mk = lambda: StableDiffusionBEVControlNetPipeline(unet=unet, controlnet=cn, scheduler=schedulers.DDIMScheduler()).to(dev)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    f = open(a.out, "w")

    def emit(**rec):
        f.write(json.dumps(rec) + "\n"); f.flush()
        print(json.dumps(rec), flush=True)

    emit(record="config", build_id=L.build_id(), scenes=a.scenes, steps=a.steps, bucket=a.bucket, dtype=a.dtype, calls=a.calls, repeats=a.repeats,
         plan_cache=int(L.get_option("PLAN_CACHE")), device=torch.cuda.get_device_name(0))

    def kwargs(Lb, seed=0):
        sc = synthetic.make_scene_batch(a.scenes, seed=1234 + seed, ctx_dim=cfg["cross_attention_dim"], max_len=Lb)
        g = lambda k: sc[k].to(dev)
        return dict(prompt=None, image=g("bev_map"), camera_param=g("camera_param"), height=224, width=400, num_inference_steps=a.steps,
                    guidance_scale=2.0, latents=g("latents"), prompt_embeds=g("prompt_embeds"), negative_prompt_embeds=g("negative_prompt_embeds"),
                    output_type="latent", bev_controlnet_kwargs={"bboxes_3d_data": {k: v.to(dev) for k, v in sc["bboxes_3d_data"].items()}})

    from magicdrive_amd import denoiser as DN
    built_total = [0]
    compile_plan = DN.SamplerPlan.compile

    def counted_compile(self):          # every plan the pipeline builds goes through compile() once
        built_total[0] += 1
        return compile_plan(self)
    DN.SamplerPlan.compile = counted_compile

    def timed(pipe, kw):
        have = built_total[0]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = pipe(**kw).images
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert torch.isfinite(out).all()
        return dt, built_total[0] - have

    # warm the process (allocator, weight packing, kernel load) on a call neither sequence repeats: no boxes share a plan with L > 0
    warm = mk(); timed(warm, kwargs(64, seed=99)); warm._plans.clear(); del warm

    # ---- 1. the validation-like sequence ----
    if not a.steady_only:
        rng = random.Random(20240)
        Ls = [rng.randint(1, 64) for _ in range(a.calls)]
        pipes = {"exact": mk(), "bucket": mk()}
        pipes["bucket"].box_bucket = a.bucket
        tot = {"exact": [0.0, 0], "bucket": [0.0, 0]}
        for i, Lb in enumerate(Ls):
            kw = kwargs(Lb, seed=i)
            for mode in (("exact", "bucket") if i % 2 == 0 else ("bucket", "exact")):
                dt, built = timed(pipes[mode], kw)
                tot[mode][0] += dt; tot[mode][1] += built
                emit(record="call", i=i, L=Lb, mode=mode, box_bucket=pipes[mode].box_bucket, seconds=round(dt, 4), plans_built=built,
                     plans_cached=len(pipes[mode]._plans))
        for mode in tot:
            emit(record="sequence", mode=mode, seconds=round(tot[mode][0], 3), plans_built=tot[mode][1], distinct_L=len(set(Ls)),
                 distinct_buckets=len({-(-x // a.bucket) for x in Ls}))
        for p in pipes.values():
            p._plans.clear()
        del pipes

    # ---- 2. steady state at L = 32: exact plan vs capacity 32 vs capacity 48 ----
    forms = {"exact": (None, False), "capacity32": (32, False), "capacity48": (48, False)}
    if a.scene_boxes:
        forms.update({"scene_capacity32": (32, True), "scene_capacity48": (48, True)})
    pipes = {}
    kw = kwargs(32, seed=7)
    for name, (bucket, per_scene) in forms.items():
        pipes[name] = mk(); pipes[name].box_bucket = bucket; pipes[name].scene_boxes = per_scene
        timed(pipes[name], kw); timed(pipes[name], kw)                  # build + one warm replay
    times = {name: [] for name in forms}
    for rep in range(a.repeats):
        for name in (list(forms) if rep % 2 == 0 else list(forms)[::-1]):
            dt, built = timed(pipes[name], kw)
            assert built == 0
            times[name].append(dt)
    for name in forms:
        (plan,) = pipes[name]._plans.values()
        ops = [op for op in plan.step_ops if isinstance(op, O.Attn) and op.name.endswith(".attn2")]
        kernels, total_us = {}, 0.0
        for op in ops:
            for _ in range(3):
                O.run_ops([op])
            kern = (L.lib().mdx_last_kernel() or b"").decode()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                O.run_ops([op])
            e1.record(); torch.cuda.synchronize()
            us = e0.elapsed_time(e1) * 1000 / 20
            total_us += us
            k = f"{kern} Tq={op.Q.shape[1]}"
            kernels.setdefault(k, [0, 0.0]); kernels[k][0] += 1; kernels[k][1] += us
        t = times[name]
        emit(record="steady_state_L32", form=name, seconds=[round(x, 4) for x in t], min_s=round(min(t), 4), median_s=round(sorted(t)[len(t) // 2], 4), spread_s=round(max(t) - min(t), 4),
             per_step_ms=round(min(t) / a.steps * 1e3, 3), ctx_attention_launches=len(ops), ctx_attention_us_per_step=round(total_us, 1),
             ctx_attention_kernels={k: {"launches": v[0], "us": round(v[1], 1)} for k, v in kernels.items()},
             ctx_keys_capacity=plan.cond.S, ctx_keys_live=sorted(set(plan.cond.live.tolist())), scene_boxes=bool(pipes[name].scene_boxes), prologue_rows=plan.cond.S * plan.B)
    f.close()


if __name__ == "__main__":
    main()
