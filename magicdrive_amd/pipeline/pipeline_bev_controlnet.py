"""StableDiffusionBEVControlNetPipeline — drop-in for magicdrive/pipeline/pipeline_bev_controlnet.py.

`__call__` keeps the reference signature (:115-141) and return contract (:466-498: `.images` is
List[List[PIL]] (B x N_cam) for output_type="pil", ndarray (B,N,H,W,3) for "np", latents (B,N,4,h,w) for
"latent").  The 50-step loop (:349-451) — BEV-ControlNet, multi-view UNet, CFG combine, scheduler step — is
one libmdx op program per step (magicdrive_amd.denoiser.SamplerPlan), replayed as a hipGraph; everything
timestep-independent runs once in a prologue program.

Scope notes: CLIP text encoding is outside the built hot path (an ordinary torch module when the caller supplies
it; `prompt_embeds=` bypasses it).  The VAE decode runs on the HIP kernels: `from_pretrained` attaches
`magicdrive_amd.networks.autoencoder_kl.AutoencoderKL` from `<sd15>/vae` exactly where the reference's `from_pretrained` attaches
diffusers' (misc/test_utils.py:118-126); a caller-supplied torch VAE is still accepted.
Fused schedulers: DDIM (eta = 0, the north-star config, and eta > 0 with device-side variance noise) and UniPC (what tools/test.py installs); others raise.
"""
from __future__ import annotations

import inspect
import json
import os
from dataclasses import dataclass
from typing import Any, Callable, Dict, List, Optional, Tuple, Union

import numpy as np
import torch

from .. import _lib
from ..denoiser import PlanCache, SamplerPlan, device_stream
from ..schedulers import DDIMScheduler, UniPCMultistepScheduler, resample_actions


@dataclass
class SampleHealth:
    """Per-scene health of one pipeline call (`pipe.health`), from the device-side records of ops.GroupStats (csrc/stats.hip).
    A record is fp32 {nonfinite, absmax, sum, sumsq} of one view's latents.  Scene indices are those of the call (global over its chunks)."""
    ok: List[bool]                                  # [B]: no bad record (and no non-finite decoded pixel)
    first_bad_step: Optional[List[int]]             # [B], "trace" only: first step whose record is bad, -1 if none (a scene bad only in its pixels keeps -1)
    final: np.ndarray                               # [B, n_cam, 4]: records of the final latents
    trace: Optional[np.ndarray] = None              # [n_steps, B, n_cam, 4], "trace" only
    image_nonfinite: Optional[np.ndarray] = None    # [B, n_cam]: non-finite values of each decoded view; None for output_type="latent"

    @property
    def bad_scenes(self) -> List[int]:
        return [i for i, ok in enumerate(self.ok) if not ok]


class SampleHealthError(RuntimeError):
    """pipe.health_action = "raise": some scenes of the call are bad.  `.bad_scenes` names them, `.health` holds the records and `.output`
    what the call would have returned."""

    def __init__(self, bad_scenes, health=None, output=None):
        self.bad_scenes = list(bad_scenes)
        self.health = health
        self.output = output
        super().__init__(f"bad samples: scenes {self.bad_scenes} (non-finite or out-of-range latents / pixels)")


@dataclass
class BEVStableDiffusionPipelineOutput:
    images: Union[List[List[Any]], np.ndarray, torch.Tensor]
    nsfw_content_detected: Optional[List[bool]]
    health: Optional[SampleHealth] = None           # pipe.health is None: None
    matte: Optional[np.ndarray] = None              # pipe.composite_images is None: None; else [B, n_cam, H, W], the weight of the recorded picture


class _NullBar:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False

    def update(self, n=1):
        pass


class StableDiffusionBEVControlNetPipeline:
    def __init__(self, vae=None, text_encoder=None, unet=None, controlnet=None, scheduler=None, tokenizer=None,
                 safety_checker=None, feature_extractor=None, requires_safety_checker: bool = False):
        assert safety_checker is None, "Please do not use safety_checker."          # pipeline_bev_controlnet.py:63
        self.vae, self.text_encoder, self.unet, self.controlnet = vae, text_encoder, unet, controlnet
        self.scheduler = scheduler if scheduler is not None else DDIMScheduler()
        self.tokenizer = tokenizer
        self.vae_scale_factor = 8
        self._progress_bar_config: Dict[str, Any] = {}
        self._device = torch.device("cpu")
        # Plans (op programs + activation pool + captured hipGraph) are cached per batch geometry.  The reference's eval flow pads
        # boxes to the per-batch maximum (configs/runner/default.yaml:61 bbox_max_length null), so L_box changes from batch to batch:
        # the cache is a small LRU and an evicted plan releases its graph and buffers.
        self._plans = PlanCache()
        self.use_graph = True
        # Scene chunks replayed concurrently on separate HIP streams (see __call__): the library option STREAMS (csrc/options.h; `pipe.streams = n`
        # overrides per pipeline); chunks hold at least `min_scenes_per_stream` scenes (below that a launch has too few tiles to fill the chip
        # even alone).  Measured on one box (profiles/r04_streams_ab.log, configs[1]): 128 scenes 7.02 -> 7.21 scenes/s, 192 scenes 7.14 -> 7.23.
        self.streams = None                                   # None: follow the option
        self.min_scenes_per_stream = 16
        # The small-batch operating point (the reference's own flows run bs = 1...4): up to this many scenes per call the ControlNet and the UNet
        # encoder of every step — independent until the zero-convs — replay side by side on two streams (SamplerPlan.launch_step).  Measured
        # (profiles/r05_fork_ab.log, 50-step DDIM, s per call without / with): 1 scene 0.656 / 0.559 (-15 %), 2: 0.849 / 0.747, 4: 1.196 / 1.071,
        # 8: 1.810 / 1.661, 16: 2.749 / 2.582 (-6 %).  From 32 scenes a call is split into scene chunks on two streams instead (above).
        self.fork_max_scenes = 31
        self.fork_chunks = False                              # also fork inside every scene chunk of a multi-stream call (A/B switch: tools/streams_ab.py)
        self._side: Dict[Any, List[Any]] = {}
        # One plan for a bucket of box counts.  The reference's validation flow pads the boxes of every batch to that batch's maximum, so the
        # padded count L_box — part of the plan key — changes almost every call, and each new value builds a plan and captures its graphs.
        # None (default): exact plans, keyed by L_box.  An integer n >= 1: a call with L_box > 0 uses the plan of capacity ceil(L_box / n) * n,
        # built with SamplerPlan(dynamic_boxes=True) — the context attention reads the live key count from device memory, positions < L_box
        # are computed as on the exact plan and the padded slots up to the capacity are never attended to.  Calls without boxes keep their plan.
        self.box_bucket: Optional[int] = None
        # Every scene of a batched call attends to its OWN boxes.  The reference pads the boxes of a batch to the batch maximum and its text-context
        # attention sees the padded slots as null-embedded tokens, so a scene's pictures depend on which scenes share its call; the reference's own
        # default is one scene per call (validation_batch_size: 1).  False (default): that padded semantics, behaviour and plan key unchanged.
        # True: a call with boxes uses a plan built with SamplerPlan(dynamic_boxes="scene") at the capacity L_box (ceil(L_box / n) * n under
        # box_bucket = n); each scene's context length 1 + 77 + L_scene is read per view from device memory, L_scene being the length a call of
        # that scene alone pads to — its latents then equal the batch-1 call's up to rounding, at any batch size, on one captured plan.
        self.scene_boxes: bool = False
        # Per-scene sample health.  The library reports what it cannot report without a host sync by writing NaN into the result, and this
        # pipeline hands latents to the VAE and pixels to a uint8 cast: a scene whose latents went non-finite (or blew up) becomes pictures
        # with no error anywhere.  None (default): nothing is emitted or copied, plan keys unchanged.  "final": one record launch per chunk
        # over the final latents.  "trace": one record per step and view from inside the captured step graphs (first_bad_step).  Either way
        # the records reach the host in ONE copy at the end of the call (no sync inside the loop) as output.health (SampleHealth).
        self.health: Optional[str] = None
        self.health_action: str = "flag"                      # "flag": report in output.health; "raise": SampleHealthError after the call
        # None: only non-finite values make a scene bad.  A float: a finite |latent| above it does too.  There is NO default threshold:
        # nobody has measured the latent range of trained weights on this path.
        self.health_absmax: Optional[float] = None
        # Keep known REGIONS of given views (StableDiffusionBEVControlNetGivenViewPipeline only; an attribute because __call__ keeps the
        # reference's signature).  None (default): today's path, plan key included.  Set: a B x N_cam list, each entry None or an (h, w)
        # tensor in [0, 1] at latent resolution — 1 keeps the view's conditional latent at that latent pixel, 0 regenerates it, a fraction
        # mixes (a box edge inside the 8x8 image pixels of a latent pixel).  None on a view WITH a conditional latent keeps the whole view;
        # a view without one is regenerated and takes no mask.  After every step but the last the sample becomes
        # m * add_noise(cond, noise, t_next) + (1 - m) * sample (ops.LatentBlend behind the scheduler op): the kept background of the
        # result is the model's own last-step output given that context, NOT the encoded input; pipe.composite_images (below) puts the
        # recorded pixels back outside the edited regions.  magicdrive_amd.dataset.regions.box_keep_mask builds the masks from projected boxes.
        self.keep_masks: Optional[List[List[Optional[torch.Tensor]]]] = None
        # Composite a kept-region edit with the RECORDED pictures, on the device (with keep_masks only; attributes like keep_masks).
        # None (default): today's path, decode_latents byte for byte what it is.  Set: a B x N_cam list, each entry None or an (H, W, 3)
        # picture — a uint8 array / tensor is taken as k / 255, a floating one must be finite and in [0, 1].  Behind the VAE decoder (and
        # behind the health image records, which still see the raw decoded tensor) ONE ops.ImageComposite launch on the decode's stream
        # turns each view into w * recorded + (1 - w) * generated, w = dataset.edit_matte(keep mask, 8, composite_feather): the keep mask
        # upsampled to the image, eroded by composite_feather image pixels and box-filtered by the same radius.  w == 1 returns the
        # recorded pixel bit for bit (numpy_to_pil_double then gives back the recorded byte), w == 0 the bits of the plain path; the
        # transition band of width 2 * composite_feather lies INSIDE the kept region, and next to the image border w = 0 may reach a few
        # pixels past the regenerated region.  A None entry leaves its view as the plain path gives it.  output.matte holds w.
        # output_type="latent", a picture on a view without a conditional latent, a wrong shape or range: ValueError before any device work.
        # Nobody has looked at composited pictures from trained weights: the feature is the mechanism and its exactness guarantees.
        self.composite_images: Optional[List[List[Any]]] = None
        self.composite_feather: int = 4
        # RePaint resampling of a kept-region edit (Lugmayr et al. 2022; with keep_masks only, DDIM only; an attribute like keep_masks).
        # None (default): today's path, plan key included.  (jump_length, jump_n_sample), integers >= 1: the loop follows
        # schedulers.resample_actions(num_steps, jump_length, jump_n_sample) — after the step at every jump_length-th index the sample is
        # diffused forward again by jump_length steps with fresh Gaussian noise made on the device (ops.LatentRenoise, the plan's own
        # captured graph; no host copy, no sync) and those steps are taken once more, jump_n_sample times in all: the model gets time to
        # harmonise regenerated content with kept content.  A call costs actions.count("step") UNet evaluations instead of num_steps;
        # callbacks and the progress bar count step launches.  One int64 seed per scene is drawn from the call's generator (from each
        # scene's own in list form) AFTER the initial latents and shared by the scene's views; the noise of a jump depends on that seed,
        # the number of jumps taken so far and the element's place in its view only, so a scene has the same jump noise alone and in a
        # batch, on one stream or two.  health="trace" rows are indexed by step, so a revisited step overwrites its row; the final step
        # is not blended on any visit.  UniPC is refused (NotImplementedError): a jump would invalidate its multistep history.
        # Nobody has measured picture quality with trained weights on this path: the feature is the mechanism.
        self.resample: Optional[Tuple[int, int]] = None

    # ---- construction / housekeeping the reference's callers use (misc/test_utils.py:94-138) ----
    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path: str, controlnet=None, unet=None, safety_checker=None,
                        feature_extractor=None, torch_dtype=torch.bfloat16, vae=None, text_encoder=None, tokenizer=None,
                        hip_text_encoder: bool = False, **kw):
        """`pipe_cls.from_pretrained(<sd15 dir>, controlnet=, unet=, safety_checker=None, feature_extractor=None, torch_dtype=)` —
        the call `build_pipe` makes (magicdrive/misc/test_utils.py:118-126).  Reads the SD-1.5 directory layout: `scheduler/
        scheduler_config.json`, `vae/` (decoded on the HIP kernels), `text_encoder/` + `tokenizer/` (transformers; optional).  hip_text_encoder=True loads
        `text_encoder/` with magicdrive_amd.networks.clip_text.CLIPTextModel (the library's kernels, no transformers import) instead; an
        instance of that class can also be passed as text_encoder=."""
        root = pretrained_model_name_or_path
        sch = DDIMScheduler()
        p = os.path.join(root, "scheduler", "scheduler_config.json")
        if os.path.exists(p):
            with open(p) as f:
                sch = DDIMScheduler.from_config(json.load(f))
        if vae is None and os.path.exists(os.path.join(root, "vae", "config.json")):
            from ..networks.autoencoder_kl import AutoencoderKL
            vae = AutoencoderKL.from_pretrained(os.path.join(root, "vae"), torch_dtype=torch_dtype)
        if text_encoder is None and hip_text_encoder:
            from ..networks.clip_text import CLIPTextModel
            text_encoder = CLIPTextModel.from_pretrained(os.path.join(root, "text_encoder"), torch_dtype=torch_dtype or torch.bfloat16)
        if text_encoder is None and os.path.isdir(os.path.join(root, "text_encoder")):
            import transformers
            text_encoder = transformers.CLIPTextModel.from_pretrained(os.path.join(root, "text_encoder")).eval()
            if torch_dtype is not None:
                text_encoder = text_encoder.to(dtype=torch_dtype)
        if tokenizer is None and os.path.isdir(os.path.join(root, "tokenizer")):
            import transformers
            tokenizer = transformers.CLIPTokenizer.from_pretrained(os.path.join(root, "tokenizer"))
        for m in (unet, controlnet):
            if m is not None and torch_dtype is not None:
                m.to(torch_dtype)
        return cls(vae=vae, text_encoder=text_encoder, unet=unet, controlnet=controlnet, scheduler=sch, tokenizer=tokenizer)

    def to(self, device):
        self._device = torch.device(device)
        for m in (self.unet, self.controlnet):
            if m is not None:
                m.to(self._device)
        for m in (self.vae, self.text_encoder):
            if m is not None and hasattr(m, "to"):
                m.to(self._device)
        self._plans.clear()
        return self

    def _side_streams(self, device, n: int):
        """`n` extra HIP streams on `device`, created once per pipeline."""
        have = self._side.setdefault(str(device), [])
        while len(have) < n:
            have.append(torch.cuda.Stream(device=device))
        return have[:n]

    @property
    def device(self):
        return self._device

    @property
    def _execution_device(self):
        return self._device

    def enable_xformers_memory_efficient_attention(self, *a, **k):
        """Accepted for call-site compatibility (misc/test_utils.py:131-132); attention is always the fused HIP kernel."""

    def enable_vae_slicing(self):
        if self.vae is not None and hasattr(self.vae, "enable_slicing"):
            self.vae.enable_slicing()

    def set_progress_bar_config(self, **kwargs):
        self._progress_bar_config = kwargs

    def progress_bar(self, iterable=None, total=None):
        if self._progress_bar_config.get("disable", True):
            return _NullBar() if iterable is None else iterable
        from tqdm.auto import tqdm
        return tqdm(iterable, **self._progress_bar_config) if iterable is not None else tqdm(total=total, **self._progress_bar_config)

    # ---- helpers with the behaviour of pipeline_controlnet.py:285-437, 634-680 ----
    def _encode_prompt(self, prompt, device, num_images_per_prompt, do_cfg, negative_prompt=None, prompt_embeds=None, negative_prompt_embeds=None):
        if prompt_embeds is None:
            if self.text_encoder is None or self.tokenizer is None:
                raise ValueError("pass prompt_embeds= (and negative_prompt_embeds=) or construct the pipeline with text_encoder + tokenizer")
            prompts = [prompt] if isinstance(prompt, str) else list(prompt)
            tok = self.tokenizer(prompts, padding="max_length", max_length=self.tokenizer.model_max_length, truncation=True, return_tensors="pt")
            prompt_embeds = self.text_encoder(tok.input_ids.to(device))[0]
        bs = prompt_embeds.shape[0]
        prompt_embeds = prompt_embeds.repeat_interleave(num_images_per_prompt, dim=0)
        if do_cfg:
            if negative_prompt_embeds is None:
                if self.text_encoder is None or self.tokenizer is None:
                    raise ValueError("classifier-free guidance needs negative_prompt_embeds= when no text encoder is attached")
                neg = [""] * bs if negative_prompt is None else ([negative_prompt] * bs if isinstance(negative_prompt, str) else list(negative_prompt))
                tok = self.tokenizer(neg, padding="max_length", max_length=prompt_embeds.shape[1], truncation=True, return_tensors="pt")
                negative_prompt_embeds = self.text_encoder(tok.input_ids.to(device))[0]
            negative_prompt_embeds = negative_prompt_embeds.repeat_interleave(num_images_per_prompt, dim=0)
        return prompt_embeds, negative_prompt_embeds

    def prepare_latents(self, batch_size, num_channels_latents, height, width, dtype, device, generator, latents=None):
        """pipeline_controlnet.py:665-680 + utils/torch_utils.py:36-77: drawn on the generator's device (CPU by
        default, so seeds are device independent), then moved."""
        shape = (batch_size, num_channels_latents, height // self.vae_scale_factor, width // self.vae_scale_factor)
        if isinstance(generator, (list, tuple)) and len(generator) != batch_size:
            raise ValueError(f"You have passed a list of generators of length {len(generator)}, but requested an effective batch"
                             f" size of {batch_size}. Make sure the batch size matches the length of the generators.")
        if latents is None:
            if isinstance(generator, (list, tuple)):      # one generator per scene (`fix_seed_within_batch`, misc/test_utils.py:224-237):
                gdev = generator[0].device                 # randn_tensor draws (1, ...) from each in turn (torch_utils.py:64-71)
                latents = torch.cat([torch.randn((1,) + shape[1:], generator=g, device=gdev, dtype=dtype) for g in generator], dim=0)
            else:
                gdev = generator.device if isinstance(generator, torch.Generator) else torch.device("cpu")
                latents = torch.randn(shape, generator=generator, device=gdev, dtype=dtype)
        else:
            assert tuple(latents.shape) == shape, f"latents {tuple(latents.shape)} != {shape}"
        return latents.to(device) * self.scheduler.init_noise_sigma

    def prepare_extra_step_kwargs(self, generator, eta):
        """Same guard as the reference (:82-98): a scheduler whose step() takes `generator` is refused."""
        params = set(inspect.signature(self.scheduler.step).parameters.keys())
        if "generator" in params:
            raise RuntimeError("If you fixed the logic for generator, please remove this. Otherwise, please use other sampler.")
        return {"eta": eta} if "eta" in params else {}

    def decode_latents(self, latents, _records=None, _composite=None):
        """pipeline_bev_controlnet.py:100-112 (5-D latents); VAE is a caller-supplied torch module.
        _records: a list that receives the device-side health records [views, 4] of the decoded tensor (before the clamp, which would
        turn +-Inf into valid pixels); not part of the reference signature.
        _composite: (orig fp32 [views, H, W, 3], has uint8 [views], keep fp32 [views, h, w], feather, sink) from _checked_composite, host
        tensors: the decoded tensor goes through ops.ImageComposite instead of the clamp / permute / float below, and sink (a list)
        receives the matte [B, n_cam, H, W], still on the device; likewise not part of the reference signature."""
        if self.vae is None:
            raise ValueError("no VAE attached: use output_type='latent' or pass vae= to the pipeline")
        sf = getattr(getattr(self.vae, "config", None), "scaling_factor", 0.18215)
        bs = latents.shape[0]
        x = (latents / sf).reshape(-1, *latents.shape[2:])
        vdt = next(self.vae.parameters()).dtype
        image = self.vae.decode(x.to(vdt)).sample
        if _records is not None:
            _records.append(self._image_records(image))
        if _composite is not None:
            from .. import ops as O
            orig, has, keep, feather, sink = _composite
            if image.dtype not in (torch.float32, torch.bfloat16, torch.float16):
                raise TypeError(f"composite of a {image.dtype} image: the kernel reads fp32, bf16 or fp16")
            if not image.is_cuda:
                raise RuntimeError("the composite is computed on the MI355X only: the decoded image is not a device tensor")
            if image.stride(-1) != 1 or image.stride(-2) < image.shape[-1]:
                image = image.contiguous()
            dev = image.device
            with torch.cuda.device(dev):
                out, matte = O.image_composite(image, orig.to(dev), keep.to(dev), feather, has=has.to(dev), return_matte=True)
            sink.append(matte.reshape(bs, -1, *matte.shape[1:]))
            return out.reshape(bs, -1, *out.shape[1:]).cpu().numpy()
        image = image.reshape(bs, -1, *image.shape[1:])
        image = (image / 2 + 0.5).clamp(0, 1)
        return image.cpu().permute(0, 1, 3, 4, 2).float().numpy()

    @staticmethod
    def _image_records(image: torch.Tensor) -> torch.Tensor:
        """fp32 [views, 4] health records of a decoded image tensor [views, 3, H, W] (ops.GroupStats, one group per view), on its device.
        16-bit and fp32 tensors go through the kernel as they are; the launch is on the current stream, behind the decode."""
        from .. import ops as O
        if image.dtype not in (torch.float32, torch.bfloat16, torch.float16):
            raise TypeError(f"health records of a {image.dtype} image: the kernel reads fp32, bf16 or fp16")
        if not image.is_cuda:
            raise RuntimeError("health records are computed on the MI355X only: the decoded image is not a device tensor")
        image = image.contiguous()
        rec = torch.zeros(image.shape[0], 4, dtype=torch.float32, device=image.device)
        O.run_ops([O.GroupStats(image, rec, name="health.image")])
        return rec

    def _sample_health(self, mode: str, table: np.ndarray, b: int, n_cam: int, image_rec: Optional[np.ndarray]) -> SampleHealth:
        """Host side of pipe.health: table [rows, b * n_cam, 4] (rows = n_steps for "trace", 1 for "final"), image_rec [b * n_cam, 4] or None."""
        table = table.reshape(table.shape[0], b, n_cam, 4)
        bad = table[..., 0] > 0                                                 # [rows, b, n_cam]
        if self.health_absmax is not None:
            bad = bad | (table[..., 1] > float(self.health_absmax))
        bad_scene_step = bad.any(axis=2)                                        # [rows, b]
        ok = ~bad_scene_step.any(axis=0)
        first = None
        if mode == "trace":
            first = [int(np.argmax(bad_scene_step[:, i])) if bad_scene_step[:, i].any() else -1 for i in range(b)]
        img_nf = None
        if image_rec is not None:
            img_nf = image_rec.reshape(b, n_cam, 4)[..., 0].astype(np.int64)
            ok = ok & ~(img_nf > 0).any(axis=1)
        return SampleHealth(ok=[bool(v) for v in ok], first_bad_step=first, final=table[-1].copy(), trace=table.copy() if mode == "trace" else None,
                            image_nonfinite=img_nf)

    @staticmethod
    def numpy_to_pil_double(images):
        from PIL import Image
        out = []
        for imgs in images:
            arr = (imgs * 255).round().astype("uint8")
            out.append([Image.fromarray(a) for a in arr])
        return out

    # ---- the sampler ----
    def _box_plan_geometry(self, L_box: int):
        """(box count the plan is built for, dynamic_boxes, the plan key's box entry) of a call whose boxes are padded to L_box, under
        self.box_bucket and self.scene_boxes.  The key entry is L_box itself — today's key — unless the plan is dynamic; then
        (capacity, "dynamic"), or (capacity, "scene") for per-scene counts."""
        n = self.box_bucket
        scene = bool(getattr(self, "scene_boxes", False))
        if L_box <= 0 or (n is None and not scene):
            return int(L_box), False, int(L_box)
        cap = int(L_box)
        if n is not None:
            if isinstance(n, bool) or int(n) != n or int(n) < 1:
                raise ValueError(f"box_bucket={n!r}: None or an integer >= 1")
            n = int(n)
            cap = -(-int(L_box) // n) * n
        return (cap, "scene", (cap, "scene")) if scene else (cap, True, (cap, "dynamic"))

    def _plan_key(self, n_scene, chunk, do_cfg, box_key, h, w, n_steps, guidance_scale, conditioning_scale, n_text, sched_kind, gv_mode, pdt, fork,
                  health=None, regions=False, resample=None, stochastic=False):
        """Cache key of one scene chunk's SamplerPlan.  `health` enters as a trailing entry only when it is on: with the switch off the key is,
        entry for entry, what it was before the switch existed.  Likewise `regions` (pipe.keep_masks set): a trailing ("regions",), and
        `resample` (pipe.resample set; the jump length: jump_n_sample only shapes the loop): a trailing ("resample", jump_length), and
        `stochastic` (a call with eta > 0; eta's value is data of the plan, not part of its key): a trailing ("eta",)."""
        key = (n_scene, chunk, do_cfg, box_key, h, w, n_steps, float(guidance_scale), float(conditioning_scale), n_text, sched_kind,
               gv_mode, pdt, id(self.unet.packed()), id(self.controlnet.packed()), fork)
        if health is not None:
            key = key + (("health", health),)
        if regions:
            key = key + (("regions",),)
        if resample is not None:
            key = key + (("resample", int(resample)),)
        if stochastic:
            key = key + (("eta",),)
        return key

    def _checked_resample(self) -> Tuple[int, int]:
        """pipe.resample as (jump_length, jump_n_sample).  Every refusal is raised here, on the host, before any device work of the call."""
        rs = self.resample
        ok = isinstance(rs, (tuple, list)) and len(rs) == 2 and all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) and v >= 1 for v in rs)
        if not ok:
            raise ValueError(f"resample={rs!r}: None or (jump_length, jump_n_sample), two integers >= 1")
        if getattr(self, "keep_masks", None) is None:
            raise ValueError("resample is set without keep_masks: resampling harmonises regenerated content with KEPT content "
                             "(set pipe.keep_masks, or pipe.resample = None)")
        if isinstance(self.scheduler, UniPCMultistepScheduler):
            raise NotImplementedError("resample under UniPC: a jump moves the sample to another noise level, which invalidates UniPC's multistep history "
                                      "(last sample, two model outputs); resampling is built for DDIMScheduler, whose step is stateless")
        return int(rs[0]), int(rs[1])

    def _checked_keep_masks(self, given_view, height: int, width: int) -> torch.Tensor:
        """pipe.keep_masks as one (B, N_cam, h, w) fp32 tensor on the host: None on a view with a conditional latent -> ones, a view without
        one -> zeros.  Every refusal is a ValueError raised here, before any device work of the call."""
        masks = self.keep_masks
        if given_view is None:
            raise ValueError("keep_masks is set, but this pipeline has no given views: masks belong to the conditional_latents of "
                             "StableDiffusionBEVControlNetGivenViewPipeline (set pipe.keep_masks = None for a plain call)")
        cond_lat, every_input = given_view
        if not every_input:
            raise ValueError("keep_masks needs conditional_latents_change_every_input=True: a kept region is the known latent re-noised to "
                             "every step's level; the False branch (noise-prediction override) has no per-pixel form")
        h, w = height // self.vae_scale_factor, width // self.vae_scale_factor
        if len(masks) != len(cond_lat) or any(len(mr) != len(cr) for mr, cr in zip(masks, cond_lat)):
            raise ValueError(f"keep_masks must be a B x N_cam list like conditional_latents: got {[len(r) for r in masks]} rows for "
                             f"{[len(r) for r in cond_lat]}")
        out = torch.zeros(len(cond_lat), max((len(r) for r in cond_lat), default=0), h, w, dtype=torch.float32)
        for i, (mr, cr) in enumerate(zip(masks, cond_lat)):
            for j, (m, v) in enumerate(zip(mr, cr)):
                if m is None:
                    if v is not None:
                        out[i, j] = 1.0
                    continue
                if v is None:
                    raise ValueError(f"keep_masks[{i}][{j}]: a mask on a view without a conditional latent (nothing is known there to keep)")
                m = torch.as_tensor(m)
                if tuple(m.shape) != (h, w):
                    raise ValueError(f"keep_masks[{i}][{j}]: shape {tuple(m.shape)}, expected the latent size ({h}, {w})")
                mf = m.detach().to("cpu", torch.float32)
                if not bool(torch.isfinite(mf).all()) or float(mf.min()) < 0.0 or float(mf.max()) > 1.0:
                    raise ValueError(f"keep_masks[{i}][{j}]: values must be finite and in [0, 1] (1 keeps, 0 regenerates)")
                out[i, j] = mf
        return out

    def _checked_composite(self, given_view, height: int, width: int, output_type) -> Tuple[torch.Tensor, torch.Tensor, int]:
        """pipe.composite_images as (orig fp32 [B * N_cam, H, W, 3] in [0, 1], has uint8 [B * N_cam], feather), host tensors; a None entry
        -> has 0 and a zero picture the kernel never reads.  Every refusal is a ValueError raised here, before any device work of the call."""
        pics, r = self.composite_images, self.composite_feather
        if getattr(self, "keep_masks", None) is None:
            raise ValueError("composite_images is set without keep_masks: the composite puts the recorded pictures back where the latents were "
                             "KEPT (set pipe.keep_masks, or pipe.composite_images = None)")
        if output_type == "latent":
            raise ValueError("composite_images with output_type='latent': the composite is an op on decoded pictures (ask for 'pil' or 'np', or "
                             "set pipe.composite_images = None)")
        if not (isinstance(r, (int, np.integer)) and not isinstance(r, bool) and 0 <= r <= 16):
            raise ValueError(f"composite_feather={r!r}: an integer number of image pixels in [0, 16]")
        cond_lat = given_view[0]                               # keep_masks passed its checks: given views exist
        if not isinstance(pics, (list, tuple)) or len(pics) != len(cond_lat) or any(not isinstance(pr, (list, tuple)) or len(pr) != len(cr) for pr, cr in zip(pics, cond_lat)):
            got = [len(pr) if isinstance(pr, (list, tuple)) else "?" for pr in pics] if isinstance(pics, (list, tuple)) else type(pics).__name__
            raise ValueError(f"composite_images must be a B x N_cam list like conditional_latents: got {got} rows for {[len(cr) for cr in cond_lat]}")
        n_cam = max((len(cr) for cr in cond_lat), default=0)
        orig = torch.zeros(len(cond_lat) * n_cam, height, width, 3, dtype=torch.float32)
        has = torch.zeros(len(cond_lat) * n_cam, dtype=torch.uint8)
        for i, (pr, cr) in enumerate(zip(pics, cond_lat)):
            for j, (pic, v) in enumerate(zip(pr, cr)):
                if pic is None:
                    continue
                if v is None:
                    raise ValueError(f"composite_images[{i}][{j}]: a picture on a view without a conditional latent (nothing is kept there)")
                t = pic.detach().cpu() if isinstance(pic, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(pic)))
                if tuple(t.shape) != (height, width, 3):
                    raise ValueError(f"composite_images[{i}][{j}]: shape {tuple(t.shape)}, expected the picture size ({height}, {width}, 3)")
                if t.dtype == torch.uint8:
                    o = t.to(torch.float32) / 255.0
                elif t.dtype.is_floating_point:
                    o = t.to(torch.float32)
                    if not bool(torch.isfinite(o).all()) or float(o.min()) < 0.0 or float(o.max()) > 1.0:
                        raise ValueError(f"composite_images[{i}][{j}]: floating values must be finite and in [0, 1]")
                else:
                    raise ValueError(f"composite_images[{i}][{j}]: dtype {t.dtype}: uint8 (taken as k / 255) or floating in [0, 1]")
                orig[i * n_cam + j] = o
                has[i * n_cam + j] = 1
        return orig, has, int(r)

    def _plan_config(self) -> Dict[str, Any]:
        """Architecture config of the sampler plan: the UNet's, with the conditioning encoders' geometry taken from the ControlNet."""
        cfg = dict(self.unet.cfg)
        cfg["controlnet"] = self.controlnet.cfg["controlnet"]
        return cfg

    @torch.no_grad()
    def __call__(self, prompt: Union[str, List[str], None], image: torch.Tensor, camera_param: Optional[torch.Tensor],
                 height: int, width: int, num_inference_steps: int = 50, guidance_scale: float = 7.5,
                 negative_prompt: Optional[Union[str, List[str]]] = None, num_images_per_prompt: Optional[int] = 1,
                 eta: float = 0.0, generator: Optional[torch.Generator] = None, latents: Optional[torch.Tensor] = None,
                 prompt_embeds: Optional[torch.Tensor] = None, negative_prompt_embeds: Optional[torch.Tensor] = None,
                 output_type: Optional[str] = "pil", return_dict: bool = True,
                 callback: Optional[Callable[[int, int, torch.Tensor], None]] = None, callback_steps: int = 1,
                 cross_attention_kwargs: Optional[Dict[str, Any]] = None, controlnet_conditioning_scale: float = 1,
                 guess_mode: bool = False, use_zero_map_as_unconditional: bool = False, bev_controlnet_kwargs={},
                 bbox_max_length=None, _given_view=None):
        """`_given_view` = (conditional_latents, change_every_input) is how StableDiffusionBEVControlNetGivenViewPipeline reuses
        this body; not part of the reference signature."""
        keep = None
        resample = None
        if getattr(self, "resample", None) is not None:        # likewise, and before the masks are looked at
            resample = self._checked_resample()
        if getattr(self, "keep_masks", None) is not None:      # refused or accepted on the host, before anything else of the call
            keep = self._checked_keep_masks(_given_view, height, width)
        composite = None
        if getattr(self, "composite_images", None) is not None:   # likewise; its own refusals need the masks to have passed theirs
            composite = self._checked_composite(_given_view, height, width, output_type)
        if guess_mode:
            # the reference's own guess path cannot run either: under CFG it feeds the ControlNet 5-D `latents` with a 2x-batched camera_param
            # and the un-repeated prompt (pipeline_bev_controlnet.py:366-373) — refused rather than guessed at
            raise NotImplementedError("guess_mode is outside the built hot path")
        if cross_attention_kwargs:
            # the reference forwards these to the UNet's attention processors (:420); the fused attention has no such hooks — refuse,
            # like attention_mask, instead of silently ignoring them
            raise NotImplementedError(f"cross_attention_kwargs={cross_attention_kwargs!r}: the fused attention kernels take no processor kwargs")
        eta = DDIMScheduler.checked_eta(eta)                   # ValueError for a negative or non-finite eta, before anything else of the call
        if self.scene_boxes and bbox_max_length is not None:
            raise ValueError(f"bbox_max_length={bbox_max_length!r} with scene_boxes=True: bbox_max_length asks for the padded slots as tokens every "
                             "scene attends to, scene_boxes for every scene attending to its own boxes only — pass one of the two")
        if isinstance(self.scheduler, DDIMScheduler):
            sched_kind = "ddim"
        elif isinstance(self.scheduler, UniPCMultistepScheduler):
            sched_kind = "unipc"
        else:
            raise NotImplementedError(f"{type(self.scheduler).__name__}: fused steps exist for magicdrive_amd.schedulers.DDIMScheduler and UniPCMultistepScheduler")
        # eta > 0 (DDIM only): the stochastic plan — ops.DdimEtaStep in the scheduler op's place, its variance noise made on the device from
        # one int64 seed per scene (the draw of pipe.resample: AFTER the initial latents, from each scene's own generator in list form; with
        # both switches on it is ONE draw).  eta's value is data of the plan (SamplerPlan.var): every eta > 0 shares one captured plan.
        # The last step adds noise too (std about 0.02 eta at SD-1.5's schedule), as diffusers does; the noise is not torch's.
        stochastic = eta > 0.0
        if stochastic and sched_kind != "ddim":
            raise NotImplementedError("the fused UniPC sampler is deterministic: eta > 0 is built for magicdrive_amd.schedulers.DDIMScheduler (eta is DDIM's parameter)")
        if self._device.type != "cuda":
            raise RuntimeError("pipeline.to('cuda') first: the sampler has no CPU path")
        health = getattr(self, "health", None)
        if health not in (None, "final", "trace"):
            raise ValueError(f"health={health!r}: None, 'final' or 'trace'")
        if health is not None and self.health_action not in ("flag", "raise"):
            raise ValueError(f"health_action={self.health_action!r}: 'flag' or 'raise'")
        if output_type != "latent" and self.vae is None:      # fail BEFORE the sampling loop, not after it
            raise ValueError("no VAE attached: use output_type='latent', pass vae= to the pipeline, or build it with from_pretrained(<sd15 dir>)")
        device = self._device
        if prompt is not None and isinstance(prompt, str):
            batch_size = 1
        elif prompt is not None and isinstance(prompt, list):
            batch_size = len(prompt)
        else:
            batch_size = prompt_embeds.shape[0]
        do_cfg = guidance_scale > 1.0
        n_cam = len(self.unet.cfg["neighboring_view_pair"])
        if camera_param is None:                                       # :260-264
            camera_param = self.controlnet.uncond_cam_param((batch_size, n_cam))
            do_cfg = False
        prompt_embeds, negative_prompt_embeds = self._encode_prompt(prompt, device, num_images_per_prompt, do_cfg, negative_prompt,
                                                                    prompt_embeds=prompt_embeds, negative_prompt_embeds=negative_prompt_embeds)
        b = batch_size * num_images_per_prompt
        image = image.to(device, torch.float32)
        if image.shape[0] == 1 and b > 1:
            image = image.expand(b, *image.shape[1:])
        assert image.shape[0] == b, f"image batch {image.shape[0]} != {b}"
        self.scheduler.set_timesteps(num_inference_steps, device=device)
        timesteps = self.scheduler.timesteps
        num_channels_latents = self.unet.config.in_channels
        latents = self.prepare_latents(b, num_channels_latents, height, width, prompt_embeds.dtype, device, generator, latents)
        jump_seeds = None
        if resample is not None or stochastic:      # one int64 seed per scene, drawn AFTER the initial latents from the same generator(s), on the host
            if isinstance(generator, (list, tuple)):
                jump_seeds = torch.cat([torch.empty(1, dtype=torch.int64, device=g.device).random_(generator=g).cpu() for g in generator])
            else:
                gdev = generator.device if isinstance(generator, torch.Generator) else torch.device("cpu")
                jump_seeds = torch.empty(b, dtype=torch.int64, device=gdev).random_(generator=generator).cpu()
        self.prepare_extra_step_kwargs(generator, eta)
        assert camera_param.shape[0] == batch_size, f"Except {batch_size} camera params, but you have bs={len(camera_param)}"
        n_cam = camera_param.shape[1]
        latents = torch.stack([latents] * n_cam, dim=1)                 # the SAME noise for every view (:326)
        camera_param = camera_param.to(device)
        boxes = dict(bev_controlnet_kwargs).get("bboxes_3d_data", None)
        text = prompt_embeds
        if do_cfg:
            kw = self.controlnet.add_uncond_to_kwargs(camera_param=camera_param, image=image, max_len=bbox_max_length,
                                                      bboxes_3d_data=boxes)
            camera_param, boxes = kw["camera_param"], kw["bboxes_3d_data"]
            uncond_image = torch.zeros_like(image) if use_zero_map_as_unconditional else kw["image"]
            image = torch.cat([uncond_image, image])
            text = torch.cat([negative_prompt_embeds.to(device), prompt_embeds.to(device)])
        # without CFG the reference never looks at bbox_max_length: the padding lives inside add_uncond_to_kwargs, which only the CFG branch
        # calls (pipeline_bev_controlnet.py:330-343) — ignored here too
        L_box = 0 if boxes is None else int(boxes["bboxes"].shape[2])
        h, w = latents.shape[-2:]
        n_steps = len(timesteps)
        gv_mode, gv_mask, gv_lat = 0, None, None
        if _given_view is not None:
            cond_lat, every_input = _given_view
            assert len(cond_lat) == b and all(len(r) == n_cam for r in cond_lat), "conditional_latents must be a B x N_cam list"
            gv_mode = 1 if every_input else 2
            gv_mask = torch.tensor([[v is not None for v in r] for r in cond_lat], dtype=torch.bool)
            gv_lat = torch.zeros(b, n_cam, *latents.shape[2:], dtype=torch.float32, device=device)
            for i, r in enumerate(cond_lat):
                for j, v in enumerate(r):
                    if v is not None:
                        gv_lat[i, j] = v.to(device, torch.float32)
        # ---- scene chunks: `self.streams` HIP streams, each replaying its own plan over a contiguous share of the scenes -------------
        # Scenes are independent (cross-view attention couples only the cameras of one scene, the CFG halves of a scene stay together),
        # and every kernel of a step owns whole CUs: on ONE stream the tail of each launch (the last partial round of tiles) and the
        # boundary between two launches leave CUs idle ~620 times per step.  Two half-batch graph replays in flight on two streams
        # fill those gaps with the other half's kernels (profiles/r04_streams_ab.log).  Callbacks need the whole
        # batch at a step boundary, so they keep the single-stream path.
        n_chunk = 1
        n_streams = max(1, int(self.streams if self.streams is not None else _lib.get_option("STREAMS")))
        if n_streams > 1 and callback is None and b >= 2 * self.min_scenes_per_stream:
            # every chunk's plan must stay cached for the whole call: the LRU evicts (and RELEASES) the oldest plan when it overflows, which
            # with a cache smaller than the chunk count would be chunk 0's, still held in `plans` below
            n_chunk = min(n_streams, b // self.min_scenes_per_stream, self._plans.maxsize)
        bounds = [(b * i) // n_chunk for i in range(n_chunk + 1)]
        c_halves = 2 if do_cfg else 1

        def rows(t, s0, s1):      # rows of scenes [s0, s1) of a tensor that holds the [uncond | cond] halves when CFG is on
            if t is None or n_chunk == 1:
                return t
            return torch.cat([t[hf * b + s0:hf * b + s1] for hf in range(c_halves)]) if c_halves == 2 else t[s0:s1]

        pdt = self.unet.packed().dtype
        fork = (n_chunk == 1 and 0 < b <= int(self.fork_max_scenes)) or (n_chunk > 1 and bool(self.fork_chunks))
        L_plan, dyn_boxes, box_key = self._box_plan_geometry(L_box)
        plans = []
        for ci in range(n_chunk):
            s0, s1 = bounds[ci], bounds[ci + 1]
            # the packed nets' identity and 16-bit type are part of the key: `pipe.unet.to(torch.float16)` re-packs the weights, and a plan
            # built on the old PackedNet would keep running (and keep alive) the old ones
            # box_bucket: the key carries (capacity, "dynamic") in the place of L_box, scene_boxes (capacity, "scene"); neither / no boxes: today's key
            key = self._plan_key(s1 - s0, ci, do_cfg, box_key, h, w, n_steps, guidance_scale, controlnet_conditioning_scale, text.shape[1], sched_kind,
                                 gv_mode, pdt, fork, health, regions=keep is not None, resample=None if resample is None else resample[0],
                                 **({"stochastic": True} if stochastic else {}))
            plan = self._plans.get(key)
            if plan is None:
                with torch.cuda.device(device):
                    # the UNet's config.json knows nothing about the conditioning encoders: their geometry (box MLP widths, map embedder
                    # class / size, camera frequencies) is the ControlNet checkpoint's (a tiny or a 272x736 `...Plus` checkpoint loaded with
                    # from_pretrained would otherwise be planned with the SD-1.5 defaults)
                    plan_cfg = self._plan_config()
                    plan = SamplerPlan(plan_cfg, self.unet.packed(), self.controlnet.packed(), device, s1 - s0, do_cfg, L_plan, (h, w),
                                       num_steps=n_steps, guidance_scale=guidance_scale,
                                       conditioning_scale=float(controlnet_conditioning_scale), n_text=text.shape[1], scheduler_kind=sched_kind,
                                       given_view_mode=gv_mode, fork=fork, dynamic_boxes=dyn_boxes, **({} if health is None else {"health": health}),
                                       **({} if keep is None else {"keep_regions": True}),
                                       **({} if resample is None else {"resample": resample[0]}), **({"stochastic": True} if stochastic else {}))
                    plan.compile()
                self._plans.put(key, plan)
            plan.load_inputs(latents[s0:s1], rows(camera_param, s0, s1), rows(text, s0, s1), rows(image, s0, s1),
                             None if boxes is None else {k: rows(v, s0, s1) for k, v in boxes.items()}, timesteps,
                             self.scheduler.coefficient_table(), given_mask=None if gv_mask is None else gv_mask[s0:s1],
                             given_latents=None if gv_lat is None else gv_lat[s0:s1], **({} if keep is None else {"keep_mask": keep[s0:s1]}),
                             **({} if jump_seeds is None else {"seeds": jump_seeds[s0:s1]}),
                             **({"var": self.scheduler.variance_table(eta)} if stochastic else {}))
            plans.append(plan)
        with torch.cuda.device(device):                       # launches, graph replays and torch copies all target the pipeline's device
            main = torch.cuda.current_stream(device)
            side_all = self._side_streams(device, (n_chunk - 1) + (n_chunk if fork else 0))
            side, fside = side_all[:n_chunk - 1], side_all[n_chunk - 1:]      # chunk streams beside the caller's; one fork stream per chunk
            if side:
                ready = torch.cuda.Event()
                ready.record(main)                            # the inputs were loaded on the caller's stream
                for s_ in side:
                    s_.wait_event(ready)
            sts = [main.cuda_stream] + [s_.cuda_stream for s_ in side]
            for plan, st in zip(plans, sts):
                plan.prologue.run(st)
            # resample: the loop is an action list; a "step" entry is the launch below, unchanged, and a jump runs each chunk's own
            # jump program on that chunk's stream.  Which step a launch takes is the device-side counter's business: i counts launches.
            actions = ["step"] * n_steps if resample is None else resample_actions(n_steps, *resample)
            n_launch = actions.count("step")
            with self.progress_bar(total=num_inference_steps if resample is None else n_launch) as bar:
                i, step_of = -1, 0      # launches so far - 1; the step the next launch takes (host mirror of step_ctr, for the callback's t)
                for act in actions:
                    if act != "step":
                        for plan, st in zip(plans, sts):
                            plan.launch_jump(st, self.use_graph)
                        step_of -= act[1]
                        continue
                    i += 1
                    t = timesteps[step_of]
                    step_of += 1
                    if fork:                                  # two branches per step and chunk (ControlNet on the chunk's fork stream)
                        for plan, cst, fst in zip(plans, [main] + list(side), fside):
                            plan.launch_step(cst, fst, self.use_graph)
                    else:
                        for plan, st in zip(plans, sts):
                            if self.use_graph:
                                plan.step.launch(st)
                            else:
                                plan.step.run(st)
                    bar.update()
                    if callback is not None and i % callback_steps == 0:
                        callback(i, t, plans[0].latents().to(prompt_embeds.dtype))
            if health == "final":                             # one record launch per chunk, on the chunk's stream, behind its last step
                for plan, st in zip(plans, sts):
                    plan.run_health(st)
            for s_ in side_all:                               # the caller's stream owns the result: join the side streams into it
                done = torch.cuda.Event()
                done.record(s_)
                main.wait_event(done)
            latents = (plans[0].latents() if n_chunk == 1 else torch.cat([pl.latents_on(main) for pl in plans])).to(prompt_embeds.dtype)
            health_dev = None
            if health is not None:                            # still on the device: the chunks' tables side by side, scenes in call order
                with torch.cuda.stream(main):
                    health_dev = torch.cat([pl.health_table() for pl in plans], dim=1).reshape(-1)
        image_rec = [] if (health is not None and output_type != "latent") else None
        matte_dev, matte = [], None
        if output_type == "latent":
            out, nsfw = latents, None
        else:
            extra = {} if image_rec is None else {"_records": image_rec}
            if composite is not None:
                matte_dev = []
                extra["_composite"] = (composite[0], composite[1], keep.reshape(-1, *keep.shape[2:]), composite[2], matte_dev)
            out = self.decode_latents(latents, **extra)
            nsfw = None
            if output_type == "pil":
                out = self.numpy_to_pil_double(out)
        report = None
        if health is not None:
            # ONE device-to-host copy for everything: [latent records | image records]
            with torch.cuda.device(device):
                packed = (torch.cat([health_dev] + [r.reshape(-1) for r in image_rec]) if image_rec else health_dev).cpu().numpy()
            n_lat = health_dev.numel()
            report = self._sample_health(health, packed[:n_lat].reshape(-1, b * n_cam, 4), b, n_cam,
                                         packed[n_lat:].reshape(b * n_cam, 4) if image_rec else None)
        if matte_dev:
            with torch.cuda.device(device):
                matte = matte_dev[0].cpu().numpy()
        result = (out, nsfw) if not return_dict else BEVStableDiffusionPipelineOutput(images=out, nsfw_content_detected=nsfw, health=report, **({} if matte is None else {"matte": matte}))
        if report is not None and self.health_action == "raise" and report.bad_scenes:
            raise SampleHealthError(report.bad_scenes, health=report, output=result)
        return result
