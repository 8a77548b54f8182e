#!/usr/bin/env python
"""Which op moved?  Walks an SD-1.5-size sampler plan op by op (prologue + two steps) and judges every op alone against fp64 on the inputs it
actually received (tests/op_parity.py: values at kernel-level tolerance, finite, borders, inputs).  One line per op: name, kernel, rel L2,
worst err / tol; then the worst ten.  Exits non-zero at the first failing condition; launches nothing after a HIP error.
Usage: python tools/op_parity.py --scenes 1 [--cfg] [--dtype bf16|fp16] [--scheduler ddim|unipc] [--boxes 32] [--fork 1]"""
import argparse, os, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import op_parity as P  # noqa: E402
from helpers import cfg_inputs, scene, state_dicts  # noqa: E402
from magicdrive_amd import _lib as L, ops as O, schedulers  # noqa: E402
from magicdrive_amd.denoiser import SamplerPlan  # noqa: E402
from magicdrive_amd.engine import PackedNet  # noqa: E402
from magicdrive_amd.networks import spec  # noqa: E402
from oracle import denoiser as D  # noqa: E402
ap = argparse.ArgumentParser()
ap.add_argument("--scenes", type=int, default=1); ap.add_argument("--cfg", action="store_true"); ap.add_argument("--dtype", choices=("bf16", "fp16"), default="bf16")
ap.add_argument("--scheduler", choices=("ddim", "unipc"), default="ddim"); ap.add_argument("--boxes", type=int, default=32); ap.add_argument("--fork", type=int, default=1)
ap.add_argument("--tiny", action="store_true", help="TINY_CONFIG instead of SD15_CONFIG")
a = ap.parse_args()
dev = torch.device("cuda:0")
dtype = torch.bfloat16 if a.dtype == "bf16" else torch.float16
cfg = spec.TINY_CONFIG if a.tiny else spec.SD15_CONFIG
usd, csd = state_dicts(cfg)
un, cn = PackedNet(usd, dev, dtype), PackedNet(csd, dev, dtype)
sc = scene(cfg, a.scenes, a.boxes or None, (28, 50))
sch = schedulers.DDIMScheduler() if a.scheduler == "ddim" else schedulers.UniPCMultistepScheduler()
ts = sch.set_timesteps(2)
if a.cfg:
    cam, text, bev, boxes = cfg_inputs(D, csd, sc)
else:
    cam, text, bev, boxes = sc["camera_param"], sc["prompt_embeds"], sc["bev_map"], sc["bboxes_3d_data"]
plan = SamplerPlan(cfg, un, cn, dev, a.scenes, a.cfg, a.boxes, (28, 50), num_steps=2, guidance_scale=2.0, scheduler_kind=a.scheduler, fork=bool(a.fork))
plan.load_inputs(torch.stack([sc["latents"]] * 6, 1), cam, text, bev, boxes, ts, sch.coefficient_table())
kernel = lambda: (L.lib().mdx_last_kernel() or b"").decode()
records = []


def execute(op):
    O.run_ops([op])


def show(tag, recs):
    for r in recs:
        print(f"{tag}[{r.index}] {r.cls} {r.name} {r.kernel} rel_l2 {r.rel_l2:.3e} worst err/tol {r.worst:.3f}" + ("" if r.rule == "close" else f" ({r.rule}: {r.emu_rel_l2:.3e})"), flush=True)
        records.append((tag, r))


try:
    for tag, ops in (("prologue", plan.prologue_ops), ("step0", plan.step_ops), ("step1", plan.step_ops)):
        for i in range(len(ops)):                      # one op per walk: its line is printed before the next op is launched
            recs = P.walk(ops[i:i + 1], execute, kernel=kernel, plan="tool")
            recs[0].index = i
            show(tag, recs)
except P.OpParityError as e:
    print(f"FAILED in {tag}[{i}]: {e}")
    sys.exit(1)
print("worst ten by err / tol:")
for tag, r in sorted(records, key=lambda x: -x[1].worst)[:10]:
    print(f"  {tag}[{r.index}] {r.name} {r.kernel}: worst err/tol {r.worst:.3f}, rel_l2 {r.rel_l2:.3e}")
print(f"{len(records)} ops judged, all conditions met")
