#!/usr/bin/env python
"""tools/sample.py — the mm-free equivalent of the reference's sampling entry points (tools/test.py:38-72, demo/run.py:33-90):
load a checkpoint in the reference layout, read the training run's hydra overrides, feed preprocessed `.pth` samples
(demo/readme.md:3-22) through StableDiffusionBEVControlNetPipeline on the MI355X path and save the six views per scene.

  python tools/sample.py --ckpt <ckpt dir with unet/ controlnet/ hydra/overrides.yaml> --sd15 <stable-diffusion-v1-5 dir> \
         --data <folder of *.pth> --out <dir> [key=value overrides as for tools/test.py] [--scheduler unipc|ddim] [--eta X] [--prompt-embeds]
         [--cond-on-view] [--regenerate-boxes [--region-dilate N] [--resample JL,JN] [--composite [--feather N] [--save-matte]]]

--cond-on-view is demo/run_cond_on_view.py:34-120: the pipe class becomes StableDiffusionBEVControlNetGivenViewPipeline, the ground-truth
views of every sample (`img` of the `.pth`) are encoded with the pipeline's VAE (`vae.encode(x).latent_dist.mean * scaling_factor`, on
the HIP kernels), and generation `ti` of the `validation_times - 1` generations is sampled with view `ti` given.

--regenerate-boxes is box editing on recorded scenes (the use demo/interactive_gui.py and demo/run_cond_on_view.py serve): the inputs of
--cond-on-view, but ALL ground-truth views are encoded and given, and `pipe.keep_masks` — one (h, w) mask per view from the sample's own
boxes (magicdrive_amd.dataset.box_keep_mask: 1 - coverage of each latent pixel by the projected boxes, grown by --region-dilate latent
pixels, default 1) — lets the sampler regenerate the boxes and keep everything else.  `validation_times` generations, one pipe() call each,
seeded as the plain loop is (there is no "view ti given" rule), the same files and index.json.  The kept background is the model's own
last-step output given the known latents, not the encoded input; --composite puts the recorded pixels back.
--composite [--feather N] [--save-matte] (with --regenerate-boxes only) sets pipe.composite_images to the samples' own `img`, mapped from
[-1, 1] to [0, 1], and pipe.composite_feather = N (image pixels, 0 to 16, default 4): behind the VAE decoder every view becomes
w * recorded + (1 - w) * generated on the device (ops.ImageComposite; w = dataset.edit_matte of the view's keep mask), so a pixel the
matte keeps whole is written as the recorded byte.  index.json gains "composite": {"feather": N} and, per generation, `kept_fraction`:
the mean of the matte per view.  --save-matte writes <scene>_gen<gen>_view<v>_matte.png (8-bit, round(255 w)) next to each view, from
the rank that sampled the scene.  Without the flag the output is byte for byte what it was.
--resample JL,JN (with --regenerate-boxes and --scheduler ddim only) sets pipe.resample = (jump_length, jump_n_sample): RePaint resampling,
which gives the model time to harmonise the regenerated boxes with what is kept at the price of more UNet evaluations per call
(INTEGRATION.md §1); index.json then carries "resample": [JL, JN].  Without the flag the output is byte for byte what it was.
--eta X (with --scheduler ddim only) is runner.pipeline_param.eta=X: stochastic DDIM with variance noise made on the device from one seed
per scene; index.json then carries "eta": X.  Without the flag the output is byte for byte what it was.

No hydra / omegaconf / mmdet3d: the config tree of the reference is not rebuilt (SURVEY.md §8 out of scope) — only the handful of
keys the sampling loop reads are resolved, in the reference's order (checkpoint overrides first, command line last, tools/test.py:46-54):
  seed, runner.validation_times, runner.pipeline_param.{guidance_scale,num_inference_steps,...}, dataset.image_size / +exp=HxW,
  fix_seed_within_batch, runner.bbox_max_length.
Without a text encoder in --sd15 the prompts cannot be embedded; pass --prompt-embeds to sample with zero embeddings (plumbing /
throughput runs) instead of failing.

Multi-GPU = the reference's FID generator flow (perception/data_prepare/val_set_gen.py:71-161), one process per GPU under torchrun:

  python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 --master-port 29511 tools/sample.py --ckpt ... --out ...

batch j of the data goes to rank j mod N (what `accelerator.prepare(dataloader)` does, :79), every rank drives GPU LOCAL_RANK; seeding follows
the reference's two branches — default: `manual_seed(cfg.seed)` per batch on every rank (test_utils.py:233-238: a scene's latents do not depend on N);
runner.validation_seed_global=true: one generator per rank seeded `seed + rank` (:83-87), a local seed drawn per batch, nothing is exchanged inside the sampling loop, and
per batch the ranks either write their own scenes' files and gather the labels on rank 0 (the reference's single-node branch, :147-150) or —
`--gather-images`, its multi-node branch :141-146 — gather the uint8 images on rank 0, which writes everything.  File names carry the GLOBAL
scene index, so a file is written exactly once whatever N is; rank 0 writes `index.json` (scene -> files, rank, seed) at the end
(perception/common/ddp_utils.py:5-16: one all_gather_object per batch).
"""
import argparse
import os
import sys
from typing import Dict, Iterator, List, Sequence

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DEFAULTS = dict(seed=42, validation_times=4, guidance_scale=2.0, num_inference_steps=20, image_size=(224, 400), fix_seed_within_batch=False,
                bbox_max_length=None, validation_seed_global=False)          # configs/test_config.yaml + configs/runner/default.yaml:54-61


def _parse(v: str):
    lo = v.strip().lower()
    if lo in ("null", "none", "~"):
        return None
    if lo in ("true", "false"):
        return lo == "true"
    try:
        return int(v)
    except ValueError:
        try:
            return float(v)
        except ValueError:
            return v


def resolve_run_config(ckpt_dir: str, cli_overrides: Sequence[str]) -> Dict:
    """Checkpoint overrides, then the command line's (tools/test.py:46-54), reduced to the keys the sampling loop reads."""
    from magicdrive_amd.dataset import load_overrides
    ov = load_overrides(ckpt_dir)
    for it in cli_overrides:
        k, _, v = it.partition("=")
        ov[k.lstrip("+")] = v
    run = dict(DEFAULTS)
    for k, v in ov.items():
        if k == "exp" and "x" in v:                                  # +exp=224x400 / 272x736 / 424x800abox0.1_nockpt (configs/exp/*.yaml)
            h, w = v.split("x")[:2]
            w = "".join(ch for ch in w if ch.isdigit() or ch == "_").split("_")[0]
            digits = "".join(c for c in w if c.isdigit())
            run["image_size"] = (int(h), int(digits))
        elif k == "dataset.image_size":
            run["image_size"] = tuple(int(x) for x in v.strip("[]() ").split(","))
        elif k == "seed":
            run["seed"] = _parse(v)
        elif k == "fix_seed_within_batch":
            run["fix_seed_within_batch"] = bool(_parse(v))
        elif k == "runner.validation_seed_global":
            run["validation_seed_global"] = bool(_parse(v))
        elif k == "runner.validation_times":
            run["validation_times"] = int(v)
        elif k == "runner.bbox_max_length":
            run["bbox_max_length"] = _parse(v)
        elif k.startswith("runner.pipeline_param."):
            run[k[len("runner.pipeline_param."):]] = _parse(v)
    return run


def iter_batches_index(n: int, batch_size: int) -> Iterator[List[int]]:
    """Sample indices of batch 0, 1, ... (the order of the reference's sequential val dataloader)."""
    for i0 in range(0, n, batch_size):
        yield list(range(i0, min(i0 + batch_size, n)))


def iter_pipe_kwargs(dataset, run: Dict, batch_size: int = 1, with_pixels: bool = False, only=None, with_meta: bool = False) -> Iterator[Dict]:
    """Batches of samples -> keyword arguments of StableDiffusionBEVControlNetPipeline.__call__, as run_one_batch /
    run_one_batch_pipe assemble them (magicdrive/misc/test_utils.py:191-255, :258-330).  with_pixels: (kwargs, pixel_values) pairs;
    with_meta: (kwargs, pixel_values, meta_data) triples (the samples' boxes and camera matrices, one list entry per scene).
    only: the batch indices to produce (a rank's share: rank_batches)."""
    from magicdrive_amd.dataset import collate_samples, preprocess_fn
    extra = {k: v for k, v in run.items() if k not in DEFAULTS or k in ("guidance_scale", "num_inference_steps")}
    for j, i0 in enumerate(range(0, len(dataset), batch_size)):
        if only is not None and j not in only:                       # another rank's batch: not even loaded
            continue
        batch = collate_samples([preprocess_fn(dataset[i]) for i in range(i0, min(i0 + batch_size, len(dataset)))])
        kw = dict(prompt=batch["captions"], image=batch["bev_map_with_aux"], camera_param=batch["camera_param"],
                  height=run["image_size"][0], width=run["image_size"][1], bev_controlnet_kwargs=batch["kwargs"],
                  bbox_max_length=run["bbox_max_length"], **extra)
        if with_meta:
            yield kw, batch["pixel_values"], batch["meta_data"]
        elif with_pixels:
            yield kw, batch["pixel_values"]
        else:
            yield kw


def encode_given_views(pipe, pixel_values: torch.Tensor) -> torch.Tensor:
    """pixel_values (b, n, 3, H, W) in [-1, 1] -> scaled latents (b, n, 4, H / 8, W / 8): demo/run_cond_on_view.py:77-86."""
    b, n = pixel_values.shape[:2]
    x = pixel_values.reshape(b * n, *pixel_values.shape[2:]).to(device=pipe._execution_device, dtype=pipe.vae.dtype)
    lat = pipe.vae.encode(x).latent_dist.mean * pipe.vae.config.scaling_factor
    return lat.reshape(b, n, *lat.shape[1:])


def cond_on_view_runs(pipe, kw: Dict, pixel_values: torch.Tensor, run: Dict, generator=None, fix_seed_for_every_generation: bool = False,
                      full_output: bool = False):
    """run_one_batch_pipe_given_view (demo/run_cond_on_view.py:34-120): `validation_times - 1` generations, generation `ti` with the
    encoded ground-truth view `ti` of every scene given and the other views sampled.  Yields (ti, images: List[List[PIL]]);
    full_output: (ti, the pipeline's output object) instead (--health reads its .health)."""
    if pixel_values is None:
        raise ValueError("--cond-on-view needs the ground-truth views (`img`) in the samples")
    latents = encode_given_views(pipe, pixel_values)
    bs, n_cam = latents.shape[:2]
    for ti in range(run["validation_times"] - 1):
        conditional_latents = [[None] * n_cam for _ in range(bs)]
        for b in range(bs):
            conditional_latents[b][ti] = latents[b, ti]
        if run["seed"] is not None and fix_seed_for_every_generation:
            generator = torch.Generator().manual_seed(run["seed"])         # :97-99
        out = pipe(conditional_latents=conditional_latents, generator=generator, **kw)
        yield ti, (out if full_output else out.images)


def recorded_pictures(pixel_values: torch.Tensor) -> List[List[torch.Tensor]]:
    """pixel_values (b, n, 3, H, W) in [-1, 1] -> the B x N_cam list of fp32 (H, W, 3) pictures in [0, 1] that pipe.composite_images takes."""
    o = (pixel_values.detach().to("cpu", torch.float32) / 2 + 0.5).clamp(0, 1).permute(0, 1, 3, 4, 2).contiguous()
    return [[o[b, v] for v in range(o.shape[1])] for b in range(o.shape[0])]


def save_mattes(out_dir: str, scene: int, gen: int, matte) -> List[str]:
    """--save-matte: one scene's mattes [n_cam, H, W] in [0, 1] -> <scene>_gen<gen>_view<v>_matte.png, 8-bit grey.  Returns the file names."""
    import numpy as np
    from PIL import Image
    names = []
    for vi, m in enumerate(np.asarray(matte)):
        name = f"{scene}_gen{gen}_view{vi}_matte.png"
        Image.fromarray((np.asarray(m, dtype=np.float32) * 255).round().astype("uint8")).save(os.path.join(out_dir, name))
        names.append(name)
    return names


def regenerate_boxes_inputs(pipe, pixel_values: torch.Tensor, meta: Dict, run: Dict, dilate: int = 1, composite=None) -> Dict:
    """--regenerate-boxes, per batch: every ground-truth view encoded (encode_given_views) and given, and pipe.keep_masks set from each
    sample's own boxes — project_box_corners with the sample's lidar2image / img_aug_matrix, box_keep_mask at the run's image size and the
    latents' (h, w).  composite (--composite: the feather, or None): pipe.composite_images = the same views as pictures in [0, 1] and
    pipe.composite_feather.  Returns the extra keyword arguments of the batch's pipe() calls: {conditional_latents}."""
    from magicdrive_amd.dataset import box_keep_mask, project_box_corners
    if pixel_values is None:
        raise ValueError("--regenerate-boxes needs the ground-truth views (`img`) in the samples")
    latents = encode_given_views(pipe, pixel_values)
    bs, n_cam = latents.shape[:2]
    masks = []
    for boxes, l2i, aug in zip(meta["gt_bboxes_3d"], meta["lidar2image"], meta["img_aug_matrix"]):
        corners, kept = project_box_corners(boxes, l2i, aug)
        masks.append(list(box_keep_mask(corners, kept, tuple(run["image_size"]), tuple(latents.shape[-2:]), dilate=dilate)))
    assert len(masks) == bs and all(len(m) == n_cam for m in masks)
    pipe.keep_masks = masks
    if composite is not None:
        pipe.composite_images, pipe.composite_feather = recorded_pictures(pixel_values), int(composite)
    return dict(conditional_latents=[[latents[b, v] for v in range(n_cam)] for b in range(bs)])


def build_pipe(ckpt: str, sd15: str, scheduler: str, device, given_view: bool = False, hip_text_encoder: bool = False):
    """The reference's build_pipe sequence (magicdrive/misc/test_utils.py:94-138) with the magicdrive_amd config strings."""
    from magicdrive_amd import schedulers
    from magicdrive_amd.misc.common import load_module
    model_cls = load_module("magicdrive_amd.networks.unet_addon_rawbox.BEVControlNetModel")
    unet_cls = load_module("magicdrive_amd.networks.unet_2d_condition_multiview.UNet2DConditionModelMultiview")
    pipe_cls = load_module("magicdrive_amd.pipeline.pipeline_bev_controlnet.StableDiffusionBEVControlNetPipeline")
    if given_view:                                                         # the swap demo/run_cond_on_view.py:138-140 makes
        pipe_cls = load_module("magicdrive_amd.pipeline.pipeline_bev_controlnet_given_view.StableDiffusionBEVControlNetGivenViewPipeline")
    ckpt = ckpt[:-1] if ckpt.endswith("/") else ckpt
    controlnet = model_cls.from_pretrained(os.path.join(ckpt, "controlnet"), torch_dtype=torch.float16).eval()
    unet = unet_cls.from_pretrained(os.path.join(ckpt, "unet"), torch_dtype=torch.float16).eval()
    pipe = pipe_cls.from_pretrained(sd15, controlnet=controlnet, unet=unet, safety_checker=None, feature_extractor=None, torch_dtype=torch.float16,
                                    hip_text_encoder=hip_text_encoder)
    if scheduler == "unipc":
        pipe.scheduler = schedulers.UniPCMultistepScheduler.from_config(pipe.scheduler.config)
    pipe.enable_xformers_memory_efficient_attention()
    return pipe.to(device)


def rank_batches(n_batches: int, rank: int, world: int) -> List[int]:
    """Batch indices of this rank: j -> rank j mod world (accelerate's dataloader sharding, val_set_gen.py:79)."""
    return list(range(rank, n_batches, world))


def rank_seed(seed, rank: int, world: int, seed_global: bool = False):
    """The seed a rank's generator starts from.  Default (runner.validation_seed_global false, configs/runner/default.yaml): run_one_batch_pipe
    seeds `torch.manual_seed(cfg.seed)` per batch on EVERY rank, no rank offset (magicdrive/misc/test_utils.py:233-238) — a scene's initial
    latents do not depend on the world size or on the rank its batch lands on.  validation_seed_global: ONE generator per rank, seeded
    `cfg.seed + accelerator.process_index` before the loop (perception/data_prepare/val_set_gen.py:83-87)."""
    if seed is None:
        return None
    return int(seed) + rank if seed_global else int(seed)


def new_local_seed(global_generator) -> int:
    """magicdrive/misc/test_utils.py:184-188."""
    return int(torch.randint(0x7ffffffffffffff0, [1], generator=global_generator).item())


def batch_generator(seed, bs: int, fix_seed_within_batch: bool, global_generator=None):
    """The `generator` argument of one batch's pipe() calls, as run_one_batch_pipe builds it (test_utils.py:221-238).  The reference's
    `torch.manual_seed(s)` re-seeds and returns THE default generator, so its per-scene list holds one object `bs` times — seeded with the
    last local seed drawn when a global generator is given — and its state carries over the validation_times loop; reproduced with one
    private generator."""
    if seed is None:
        return None
    if global_generator is not None:
        local = [new_local_seed(global_generator) for _ in range(bs if fix_seed_within_batch else 1)][-1]
        g = torch.Generator().manual_seed(local)
    else:
        g = torch.Generator().manual_seed(int(seed))
    return [g] * bs if fix_seed_within_batch else g


def save_views(out_dir: str, scene: int, gen: int, views) -> List[str]:
    """One scene's views of one generation -> <scene>_gen<gen>_view<v>.png; `views`: PIL images or uint8 HxWx3 arrays.  Returns the file names."""
    names = []
    for vi, im in enumerate(views):
        if not hasattr(im, "save"):
            from PIL import Image
            import numpy as np
            im = Image.fromarray(np.asarray(im, dtype="uint8"))
        name = f"{scene}_gen{gen}_view{vi}.png"
        im.save(os.path.join(out_dir, name))
        names.append(name)
    return names


def health_fields(health, bi: int) -> Dict:
    """The index.json entries of scene `bi` of one pipeline call from its output.health (pipeline_bev_controlnet.SampleHealth): ok, the step
    the scene died at (-1: never), the non-finite values of its final latents plus decoded pixels, the largest finite |latent|."""
    nonfinite = int(health.final[bi, :, 0].sum())
    if health.image_nonfinite is not None:
        nonfinite += int(health.image_nonfinite[bi].sum())
    first = -1 if health.first_bad_step is None else int(health.first_bad_step[bi])
    return dict(ok=bool(health.ok[bi]), first_bad_step=first, nonfinite=nonfinite, absmax=float(health.final[bi, :, 1].max()))


def exchange_batch(records: List[Dict], images, rank: int, world: int, gather_images: bool, out_dir: str, skip_bad: bool = False) -> List[Dict]:
    """End of a batch on every rank (val_set_gen.py:137-151).  records: this rank's [{scene, gen, rank, seed}], images: the matching
    [views] lists.  Single-node branch: the rank writes its own files, then the labels are gathered; multi-node branch (gather_images): labels
    AND uint8 images are gathered and rank 0 writes.  Returns the records with their file names — on rank 0 those of every rank, elsewhere []
    (ddp_utils.concat_from_everyone).  One all_gather_object per batch; ranks whose shard ran out contribute an empty list.
    skip_bad (--health skip): a record with ok == False keeps its place in the index with files = [], and none of its views is written or sent;
    the health fields are part of the records, so they ride on the same exchange."""
    import numpy as np
    import torch.distributed as dist
    if skip_bad:
        images = [[] if r_.get("ok") is False else views for r_, views in zip(records, images)]
    if not gather_images:
        for r_, views in zip(records, images):
            r_["files"] = save_views(out_dir, r_["scene"], r_["gen"], views)
        payload = records
    else:
        payload = [dict(r_, pixels=[np.asarray(v, dtype="uint8") for v in views]) for r_, views in zip(records, images)]
    if world == 1:
        gathered = [payload]
    else:
        gathered = [None] * world
        dist.all_gather_object(gathered, payload)
    if rank != 0:
        return []
    out = []
    for part in gathered:
        for r_ in part:
            if gather_images:
                r_["files"] = save_views(out_dir, r_["scene"], r_["gen"], r_.pop("pixels"))
            out.append(r_)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ckpt", required=True); ap.add_argument("--sd15", required=True)
    ap.add_argument("--data", required=True); ap.add_argument("--out", required=True)
    ap.add_argument("--scheduler", choices=["unipc", "ddim"], default="unipc")
    ap.add_argument("--batch-size", type=int, default=1)
    ap.add_argument("--prompt-embeds", action="store_true", help="no text encoder available: sample with zero prompt embeddings")
    ap.add_argument("--hip-text-encoder", action="store_true", help="encode the prompts on the HIP kernels (magicdrive_amd.networks.clip_text) instead of transformers' CLIPTextModel")
    ap.add_argument("--device", default=None, help="default: cuda:<LOCAL_RANK>")
    ap.add_argument("--gather-images", action="store_true", help="multi-rank: rank 0 writes every file from gathered uint8 images (the reference's multi-node branch); "
                                                                 "default: each rank writes its own scenes, labels are gathered (its single-node branch)")
    ap.add_argument("--pipe-factory", default="", help="TESTS: module:function(ckpt, sd15, scheduler, device, given_view) returning the pipeline instead of build_pipe")
    ap.add_argument("--dist-backend", default=None, help="torch.distributed backend under torchrun (default: nccl = RCCL with a GPU, else gloo)")
    ap.add_argument("--reseed-per-run", action="store_true", help="deviation from the reference: an independent seed per (batch, validation run)")
    ap.add_argument("--cond-on-view", action="store_true", help="demo/run_cond_on_view.py: generation ti is sampled with the encoded ground-truth view ti given")
    ap.add_argument("--regenerate-boxes", action="store_true", help="box editing: all ground-truth views are encoded and given, pipe.keep_masks keeps every latent "
                    "pixel outside the sample's projected boxes (INTEGRATION.md §1); validation_times generations, seeded as the plain loop")
    ap.add_argument("--region-dilate", type=int, default=1, help="--regenerate-boxes: grow the regenerated region by N latent pixels (default 1)")
    ap.add_argument("--resample", default=None, metavar="JL,JN", help="--regenerate-boxes with --scheduler ddim: RePaint resampling, pipe.resample = (jump_length, "
                    "jump_n_sample), two integers >= 1 (INTEGRATION.md §1); recorded in index.json")
    ap.add_argument("--eta", type=float, default=None, metavar="X", help="--scheduler ddim: stochastic DDIM, the same as runner.pipeline_param.eta=X (variance noise made "
                    "on the device from one seed per scene, INTEGRATION.md §1); finite and >= 0; recorded in index.json")
    ap.add_argument("--composite", action="store_true", help="--regenerate-boxes: composite every view with the sample's recorded picture on the device "
                    "(pipe.composite_images, INTEGRATION.md §1): pixels the matte keeps whole are the recorded bytes; index.json gains composite / kept_fraction")
    ap.add_argument("--feather", type=int, default=None, metavar="N", help="--composite: pipe.composite_feather, the matte's erosion and blur radius in image pixels, 0 to 16 (default 4)")
    ap.add_argument("--save-matte", action="store_true", help="--composite: write <scene>_gen<gen>_view<v>_matte.png (8-bit) next to each view")
    ap.add_argument("--box-bucket", type=int, default=None, help="one sampler plan per bucket of N padded box counts (pipe.box_bucket, INTEGRATION.md §1): the "
                    "padded box count changes with almost every batch of a validation run; default: an exact plan per count")
    ap.add_argument("--scene-boxes", action="store_true", help="every scene of a batch attends to its own boxes only (pipe.scene_boxes, INTEGRATION.md §1): "
                    "with fix_seed_within_batch=true a scene's pictures are those of the reference's batch-1 run at any --batch-size; default: the "
                    "reference's padded-batch semantics")
    ap.add_argument("--health", choices=["off", "flag", "skip"], default="off", help="per-scene sample health from the device-side records (pipe.health = 'trace', "
                    "INTEGRATION.md §1).  flag: index.json gains ok / first_bad_step / nonfinite / absmax per scene and generation; skip: also, the PNGs of "
                    "a bad scene are not written.  Either ends with a one-line summary and exit status 3 if any scene was bad.  off (default): nothing changes")
    ap.add_argument("overrides", nargs="*")
    a = ap.parse_args(argv)
    from magicdrive_amd.dataset import FolderSet
    from magicdrive_amd import distributed as DD
    import json
    rank, world, local = DD.init_from_env(backend=a.dist_backend)
    device = a.device or (f"cuda:{local}" if torch.cuda.is_available() else "cpu")
    run = resolve_run_config(a.ckpt, a.overrides)
    if a.regenerate_boxes and a.cond_on_view:
        raise SystemExit("--regenerate-boxes gives every view with a mask; --cond-on-view gives view ti whole: pass one of the two")
    if a.region_dilate < 0:
        raise SystemExit("--region-dilate must be >= 0")
    resample = None
    if a.resample is not None:
        if not a.regenerate_boxes:
            raise SystemExit("--resample harmonises a kept-region edit: it is valid with --regenerate-boxes only")
        if a.scheduler != "ddim":
            raise SystemExit("--resample needs --scheduler ddim: a jump would invalidate UniPC's multistep history")
        parts = a.resample.split(",")
        if len(parts) != 2 or not all(p_.strip().isdigit() and int(p_) >= 1 for p_ in parts):
            raise SystemExit(f"--resample {a.resample!r}: JL,JN, two integers >= 1")
        resample = (int(parts[0]), int(parts[1]))
    if a.eta is not None:
        if a.scheduler != "ddim":
            raise SystemExit("--eta needs --scheduler ddim: eta is DDIM's parameter, the fused UniPC sampler is deterministic")
        if not (a.eta == a.eta and 0.0 <= a.eta < float("inf")):
            raise SystemExit(f"--eta {a.eta!r}: a finite number >= 0")
        run["eta"] = float(a.eta)
    if a.composite and not a.regenerate_boxes:
        raise SystemExit("--composite puts the recorded pictures back around a kept-region edit: it is valid with --regenerate-boxes only")
    if (a.feather is not None or a.save_matte) and not a.composite:
        raise SystemExit("--feather and --save-matte belong to --composite")
    feather = None
    if a.composite:
        feather = 4 if a.feather is None else a.feather
        if not 0 <= feather <= 16:
            raise SystemExit(f"--feather {feather}: an integer number of image pixels in [0, 16]")
    given_view = a.cond_on_view or a.regenerate_boxes
    if a.pipe_factory:
        import importlib
        mod, fn = a.pipe_factory.split(":")
        pipe = getattr(importlib.import_module(mod), fn)(a.ckpt, a.sd15, a.scheduler, device, given_view)
    else:
        pipe = build_pipe(a.ckpt, a.sd15, a.scheduler, device, given_view=given_view, hip_text_encoder=a.hip_text_encoder)
    if a.box_bucket is not None:
        if a.box_bucket < 1:
            raise SystemExit("--box-bucket must be >= 1")
        pipe.box_bucket = a.box_bucket
    if a.scene_boxes:
        pipe.scene_boxes = True
    if resample is not None:
        pipe.resample = resample
    health_on = a.health != "off"
    if health_on:
        pipe.health, pipe.health_action = "trace", "flag"
    data = FolderSet(a.data)
    if rank == 0:
        os.makedirs(a.out, exist_ok=True)
    DD.barrier()
    seed = rank_seed(run["seed"], rank, world, run["validation_seed_global"])
    global_gen = torch.Generator().manual_seed(seed) if (run["validation_seed_global"] and seed is not None) else None   # carried across batches
    batches = list(iter_batches_index(len(data), a.batch_size))
    mine = set(rank_batches(len(batches), rank, world))
    n_rounds = (len(batches) + world - 1) // world                  # every rank takes part in every per-batch exchange (a collective)
    index: List[Dict] = []
    n_local = 0
    n_bad_local = 0
    it = iter_pipe_kwargs(data, run, a.batch_size, with_pixels=a.cond_on_view, only=mine, with_meta=a.regenerate_boxes)
    for rnd in range(n_rounds):
        j = rnd * world + rank
        records, images_out = [], []
        if j < len(batches):
            item = next(it)
            kw, pixel_values, meta = item if a.regenerate_boxes else ((*item, None) if a.cond_on_view else (item, None, None))
            bs = kw["image"].shape[0]
            scene0 = batches[j][0]
            if getattr(pipe, "text_encoder", None) is None:
                if not a.prompt_embeds:
                    raise SystemExit(f"{a.sd15} has no text_encoder/: pass --prompt-embeds to sample with zero embeddings")
                D = pipe.unet.cfg["cross_attention_dim"]
                kw.update(prompt=None, prompt_embeds=torch.zeros(bs, 77, D), negative_prompt_embeds=torch.zeros(bs, 77, D))
            # Seeding as run_one_batch_pipe does it (magicdrive/misc/test_utils.py:221-238): the generator is built ONCE per batch, before the
            # validation_times loop (its state carries across the iterations).  Default: manual_seed(cfg.seed) on every rank; with
            # runner.validation_seed_global=true the rank's global generator (seed + rank, val_set_gen.py:83-87) hands out a local seed per batch.
            # --reseed-per-run (a deviation) draws a fresh seed per (batch, run).
            gen = batch_generator(seed, bs, run["fix_seed_within_batch"], global_gen)
            base_gen = gen[0] if isinstance(gen, list) else gen
            if a.cond_on_view:
                for ti, out in cond_on_view_runs(pipe, kw, pixel_values, run, generator=base_gen, full_output=health_on):
                    for bi, views in enumerate(out.images if health_on else out):
                        records.append(dict(scene=scene0 + bi, gen=ti, rank=rank, seed=seed, **(health_fields(out.health, bi) if health_on else {})))
                        images_out.append(views)
            else:
                if a.regenerate_boxes:                  # every view given, masked by the sample's boxes; the loop below is the plain one
                    kw = dict(kw, **regenerate_boxes_inputs(pipe, pixel_values, meta, run, a.region_dilate, composite=feather))
                for ti in range(run["validation_times"]):
                    g = gen
                    if a.reseed_per_run and base_gen is not None:
                        g1 = torch.Generator().manual_seed(new_local_seed(base_gen))
                        g = [g1] * bs if run["fix_seed_within_batch"] else g1
                    out = pipe(generator=g, **kw)
                    for bi, views in enumerate(out.images):                       # List[List[PIL]]: scene x view
                        records.append(dict(scene=scene0 + bi, gen=ti, rank=rank, seed=seed, **(health_fields(out.health, bi) if health_on else {})))
                        images_out.append(views)
                        if feather is not None:
                            records[-1]["kept_fraction"] = [float(m.mean()) for m in out.matte[bi]]
                            if a.save_matte and not (a.health == "skip" and records[-1].get("ok") is False):
                                save_mattes(a.out, scene0 + bi, ti, out.matte[bi])
            n_local += bs
        n_bad_local += sum(1 for r_ in records if r_.get("ok") is False)
        index += exchange_batch(records, images_out, rank, world, a.gather_images, a.out, skip_bad=a.health == "skip")
    if rank == 0:
        index.sort(key=lambda r_: (r_["scene"], r_["gen"]))
        with open(os.path.join(a.out, "index.json"), "w") as f:
            json.dump(dict(world=world, seed=run["seed"], gather_images=bool(a.gather_images), **({} if resample is None else {"resample": list(resample)}),
                           **({} if a.eta is None else {"eta": float(a.eta)}),
                           **({} if feather is None else {"composite": {"feather": feather}}),
                           generations=index), f, indent=1)
        print(f"sampled {len(data)} scenes x {run['validation_times'] - (1 if a.cond_on_view else 0)} on {world} rank(s) -> {a.out}")
    n_bad = n_bad_local
    if health_on and rank == 0:
        bad = [r_ for r_ in index if r_.get("ok") is False]
        n_bad = len(bad)
        print(f"health: {n_bad} of {len(index)} generations bad" + (f" (scenes {sorted({r_['scene'] for r_ in bad})}"
              + (", pictures not written" if a.health == "skip" else "") + ")" if bad else ""))
    DD.shutdown()
    if health_on and n_bad:
        sys.exit(3)


if __name__ == "__main__":
    main()
