"""Plans: the op programs of the hot path at a fixed batch geometry.

  SamplerPlan   — what StableDiffusionBEVControlNetPipeline.__call__ runs: one prologue program and one
                  per-step program (ControlNet -> UNet -> CFG + DDIM), replayed num_inference_steps times
                  (eager, or as a captured hipGraph).
  ControlNetPlan / UNetPlan — the module-level forwards behind BEVControlNetModel.forward /
                  UNet2DConditionModelMultiview.forward (reference signatures).

View ordering everywhere: view index = (cfg_half * b + scene) * n_cam + cam, "uncond first, cond second"
(pipeline_bev_controlnet.py:330-343, 352-354).
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _lib as L
from . import ops as O
from . import packing as PK
from .networks import spec
from .engine import Act, Builder, PackedNet, Pool, TembTable, build_context_kv, level_sizes, skip_geometry

BF16, F32 = torch.bfloat16, torch.float32
CIN_PAD = 8      # latent channels (4) zero-padded so conv_in meets the MFMA path's Cin % 8 == 0


def _rows_as_pixels(t2d: torch.Tensor) -> torch.Tensor:
    """[M, C] view with row stride ld -> [M, 1, 1, C] 'image' of M one-pixel samples (for linear layers run
    through the direct-conv kernel, which may write into a column/row slice of a wider buffer)."""
    M, C = t2d.shape
    ld = t2d.stride(0)
    assert t2d.stride(1) == 1
    return torch.as_strided(t2d, (M, 1, 1, C), (ld, ld, ld, 1), t2d.storage_offset())


def device_stream(device=None) -> int:
    """Raw hipStream_t of torch's current stream ON `device` (not on whatever device happens to be current)."""
    if not torch.cuda.is_available():
        return 0
    return torch.cuda.current_stream(device).cuda_stream


def _stream(device=None) -> int:
    return device_stream(device)


class PlanCache:
    """Small LRU of plans keyed by batch geometry.  A plan owns a 64 MB workspace, its activation pool, K/V and temb tables and a
    captured hipGraph; the reference's validation flow changes the padded box count (and with it the plan key) almost every batch,
    so an unbounded dict would accumulate ~100 plans per batch size.  Evicted plans release their graph and device buffers.
    Size: the library option PLAN_CACHE (csrc/options.h, default 6: a multi-stream call holds one plan per scene chunk)."""

    def __init__(self, maxsize: Optional[int] = None):
        from collections import OrderedDict
        from . import _lib
        self.maxsize = maxsize if maxsize is not None else max(1, int(_lib.get_option("PLAN_CACHE")))
        self._d = OrderedDict()

    def get(self, key):
        p = self._d.get(key)
        if p is not None:
            self._d.move_to_end(key)
        return p

    def put(self, key, plan):
        self._d[key] = plan
        self._d.move_to_end(key)
        while len(self._d) > self.maxsize:
            _, old = self._d.popitem(last=False)
            rel = getattr(old, "release", None)
            if rel is not None:
                rel()

    def clear(self):
        for old in self._d.values():
            rel = getattr(old, "release", None)
            if rel is not None:
                rel()
        self._d.clear()

    def values(self):
        return self._d.values()

    def __len__(self):
        return len(self._d)

    def __contains__(self, key):
        return key in self._d


class ConditioningBuffers:
    """Input-side device buffers of the conditioning prologue + the ops that turn them into the context tokens
    ehs_with_cam [B, 1+77+L, D] and the per-view map feature (BEVControlNetModel.forward :743-793, 842-850)."""

    def __init__(self, bld: Builder, cn: PackedNet, cfg, n_scene: int, n_cam: int, L_box: int, latent_hw, n_text: int = 77, dynamic=False,
                 cfg_halves: int = 1):
        """dynamic: L_box is a box CAPACITY.  load() then takes boxes padded to any L <= L_box, fills the first L slots of every view (the
        rest stay masked out: null embeddings, finite) and writes the live context length 1 + n_text + L to `self.live` (int32 [1]), which the
        context attention reads on the device (ops.Attn.tk_dev).
        dynamic="scene": one count per view, `self.live` is int32 [B] (ops.Attn.tk_rows): load() writes 1 + n_text + L_scene for every view
        of a scene, L_scene = the scene's own padded length (1 + the index of its last kept box over its cameras; 0 without one) — what a
        call of that scene alone would have padded to, so the scene attends to exactly the tokens of its batch-1 call.  cfg_halves = 2: the
        scenes are [uncond | cond] halves; a scene's count is its cond row's and holds for both halves (the reference pads the uncond boxes
        to the cond length, add_uncond_to_kwargs)."""
        dev = bld.device
        assert dynamic in (False, True, "scene"), f"dynamic={dynamic!r}: False, True or 'scene'"
        assert not dynamic or L_box > 0, "a dynamic plan needs a box capacity >= 1"
        assert cfg_halves in (1, 2) and n_scene % cfg_halves == 0
        self.dynamic = bool(dynamic)
        self.per_scene = dynamic == "scene"
        self.cfg_halves = cfg_halves
        H16 = bld.dtype                     # the plan's 16-bit activation type (bf16 or fp16)
        self.dtype = H16
        cc = cfg["controlnet"]; bb = cc["bbox"]
        self.minmax_normalize = bool(bb.get("minmax_normalize", False))
        self.n_scene, self.n_cam, self.L = n_scene, n_cam, L_box
        B = n_scene * n_cam
        D = cfg["cross_attention_dim"]
        self.S = 1 + n_text + L_box
        self.n_text = n_text
        S = self.S
        self.ctx = torch.zeros(B, S, D, dtype=H16, device=dev)
        # keys the context attention sees; < S only on a dynamic plan.  One entry, or one per view through the nets (dynamic="scene")
        self.live = torch.full((B if self.per_scene else 1,), S, dtype=torch.int32, device=dev)
        # camera: [B, 7, 3] fp32 (columns of the (3,7) matrix) -> Fourier 189 -> cam2token -> ctx[:, 0]
        ncol = cc["uncond_cam_in_dim"][1]
        F_cam = cc["cam_embedder_num_freqs"]
        self.cam_in = torch.zeros(B, ncol, 3, dtype=F32, device=dev)
        cam_emb = torch.empty(B, ncol * (3 + 6 * F_cam), dtype=H16, device=dev)
        bld.emit(O.Fourier(self.cam_in, cam_emb, F_cam, name="cam.fourier"))
        wc = cn.lin("cam2token.weight")
        bld.emit(O.Conv(cam_emb.view(B, 1, 1, -1), wc.view(wc.shape[0], 1, 1, wc.shape[1]), _rows_as_pixels(self.ctx[:, 0, :]),
                        bias=cn.vec("cam2token.bias"), pad=(0, 0), direct=True, name="cam2token"))
        # boxes
        if L_box > 0:
            P, Fq = bb["n_corners"], bb["embedder_num_freq"]
            fdim = P * (3 + 6 * Fq)
            pd = bb["proj_dims"]; ctd = bb["class_token_dim"]
            n = B * L_box
            self.box_in = torch.zeros(n, P, 3, dtype=F32, device=dev)
            self.box_mask = torch.zeros(n, dtype=torch.uint8, device=dev)
            self.box_cls = torch.zeros(n, dtype=torch.int64, device=dev)
            pos = torch.empty(n, fdim, dtype=H16, device=dev)
            bld.emit(O.Fourier(self.box_in, pos, Fq, mask=self.box_mask, null_feat=cn.vec("bbox_embedder.null_pos_feature"), name="box.fourier"))
            e1 = torch.empty(n, pd[0] + ctd, dtype=H16, device=dev)       # [silu(bbox_proj) | class token]
            wp = cn.lin("bbox_embedder.bbox_proj.weight")
            bld.emit(O.Conv(pos.view(n, 1, 1, fdim), wp.view(pd[0], 1, 1, fdim), _rows_as_pixels(e1[:, :pd[0]]),
                            bias=cn.vec("bbox_embedder.bbox_proj.bias"), pad=(0, 0), epilogue=L.EPI_SILU, direct=True, name="box.bbox_proj"))
            bld.emit(O.Gather(cn.table("bbox_embedder._class_tokens"), e1[:, pd[0]:], self.box_cls, mask=self.box_mask,
                              null_row=cn.vec_bf16("bbox_embedder.null_class_feature"), name="box.class_token"))
            e2 = torch.empty(n, pd[1], dtype=H16, device=dev)
            bld.emit(O.Gemm(e1, cn.lin("bbox_embedder.second_linear.0.weight"), e2, bias=cn.vec("bbox_embedder.second_linear.0.bias"), epilogue=L.EPI_SILU, name="box.mlp0"))
            e3 = torch.empty(n, pd[2], dtype=H16, device=dev)
            bld.emit(O.Gemm(e2, cn.lin("bbox_embedder.second_linear.2.weight"), e3, bias=cn.vec("bbox_embedder.second_linear.2.bias"), epilogue=L.EPI_SILU, name="box.mlp2"))
            # last layer writes straight into the box rows of every view's context (batched over views)
            bld.emit(O.Gemm(e3.view(B, L_box, pd[2]), cn.lin("bbox_embedder.second_linear.4.weight"), self.ctx[:, 1 + n_text:, :],
                            bias=cn.vec("bbox_embedder.second_linear.4.bias"), name="box.mlp4"))
            self._keep = (pos, e1, e2, e3)
        self._keep_cam = cam_emb
        # BEV map encoder: once per scene (the reference convolves 6 identical copies every step)
        h, w = latent_hw
        msz = cc["map_size"]
        ch = cc["conditioning_embedding_out_channels"]
        self.map_in = torch.zeros(n_scene, msz[0], msz[1], msz[2], dtype=F32, device=dev)
        x = torch.empty(n_scene, msz[1], msz[2], msz[0], dtype=H16, device=dev)
        bld.emit(O.Layout(self.map_in, x, True, name="map.nhwc"))
        pre = "controlnet_cond_embedding."
        layers = [(pre + "conv_in.", (1, 1), (1, 1), True)]
        nblk = 0
        while cn.has(f"{pre}blocks.{nblk}.weight"):
            nblk += 1
        plus = spec.map_embedder_plus_size(cfg)
        for i in range(nblk):
            if plus is None:                                # BEVControlNetConditioningEmbedding, map_embedder.py:36-56
                if i < nblk - 2:
                    layers.append((f"{pre}blocks.{i}.", (1, 1), (1, 1), True) if i % 2 == 0 else (f"{pre}blocks.{i}.", (2, 2), (2, 1), True))
                elif i == nblk - 2:
                    layers.append((f"{pre}blocks.{i}.", (1, 1), (2, 1), True))
                else:
                    layers.append((f"{pre}blocks.{i}.", (2, 1), (2, 1), True))
            else:                                           # ...Plus, map_embedder.py:94-117: pad 1 everywhere; strides 1,1 | 1,2 | 1,(2,1)
                stride = (1, 1) if i % 2 == 0 else ((2, 1) if i == nblk - 1 else ((1, 1) if i == 1 else (2, 2)))
                layers.append((f"{pre}blocks.{i}.", stride, (1, 1), True))
        layers.append((pre + "conv_out.", (1, 1), (1, 1), False))
        keep = [x]
        for key, stride, pad, act in layers:
            if plus is not None and key == pre + "conv_out.":
                x = self._adaptive_avg_pool_silu(bld, x, plus, keep)      # blocks[-1] = AdaptiveAvgPool2d, then SiLU (map_embedder.py:117, :71-73)
            wt = cn.conv(key + "weight")
            Hi, Wi = x.shape[1], x.shape[2]
            Ho = (Hi + 2 * pad[0] - 3) // stride[0] + 1
            Wo = (Wi + 2 * pad[1] - 3) // stride[1] + 1
            y = torch.empty(n_scene, Ho, Wo, wt.shape[0], dtype=H16, device=dev)
            bld.emit(O.Conv(x, wt, y, bias=cn.vec(key + "bias"), stride=stride, pad=pad, epilogue=L.EPI_SILU if act else L.EPI_NONE,
                            direct=(wt.shape[3] % 8 != 0 or wt.shape[0] % 4 != 0), ws=bld.ws, name="map." + key))
            keep.append(y)
            x = y
        if (x.shape[1], x.shape[2]) != (h, w):
            raise ValueError(f"map encoder output {tuple(x.shape[1:3])} != latent size {(h, w)}: select BEVControlNetConditioningEmbeddingPlus with "
                             f"conditioning_embedding_size={[h, w]} (configs/exp/272x736.yaml:15-22; spec.with_plus_map_embedder)")
        C0 = x.shape[3]
        self.map_rep = torch.empty(B, h, w, C0, dtype=H16, device=dev)
        for s in range(n_scene):
            for c in range(n_cam):
                bld.emit(O.Ew(L.EW_COPY, x[s].view(h * w, C0), self.map_rep[s * n_cam + c].view(h * w, C0), name="map.repeat"))
        self._keep_map = keep

    @staticmethod
    def _adaptive_avg_pool_silu(bld, x, out_hw, keep):
        """SiLU(AdaptiveAvgPool2d(out_hw)(x)) for channels-last x [n, Hi, Wi, C] on the existing kernels (runs once per scene, in the
        prologue): the pooling is a fixed linear map over pixels, so it is ONE batched GEMM  out[n] = P @ x[n]  with the
        [Ho*Wo, Hi*Wi] matrix of window weights (torch's windows: start = floor(o*I/O), end = ceil((o+1)*I/O)) and the SiLU epilogue;
        the GEMM wants its second operand K-contiguous, i.e. x as [C, Hi*Wi] = NCHW, hence the layout op.  Weights 1/count are bf16:
        exact for counts 1, 2, 4 (every window of the 432x768 case), 2^-9 relative otherwise."""
        n, Hi, Wi, C = x.shape
        Ho, Wo = out_hw
        dev = x.device
        H16 = x.dtype

        def windows(I, Oo):
            m = torch.zeros(Oo, I, dtype=torch.float64)
            for o in range(Oo):
                a, b = (o * I) // Oo, -((-(o + 1) * I) // Oo)
                m[o, a:b] = 1.0 / (b - a)
            return m
        P = torch.kron(windows(Hi, Ho), windows(Wi, Wo)).to(H16).to(dev)              # [(oy,ox), (iy,ix)]
        xn = torch.empty(n, C, Hi, Wi, dtype=H16, device=dev)
        bld.emit(O.Layout(x, xn, False, name="map.pool.nchw"))
        y = torch.empty(n, Ho, Wo, C, dtype=H16, device=dev)
        bld.emit(O.Gemm(P, xn.view(n, C, Hi * Wi), y.view(n, Ho * Wo, C), epilogue=L.EPI_SILU, ws=bld.ws, name="map.pool"))
        keep += [P, xn, y]
        return y

    # ---- input marshalling (torch: dtype / layout of user tensors only) ----
    def load(self, camera_param: torch.Tensor, text: torch.Tensor, bev_map: torch.Tensor, boxes: Optional[Dict[str, torch.Tensor]]):
        """camera_param (n_scene, n_cam, 3, 7); text (n_scene, n_text, D); bev_map (n_scene, C, H, W);
        boxes {bboxes (n_scene, n_cam | 1, L, 8, 3), classes, masks} or None."""
        ns, nc = self.n_scene, self.n_cam
        assert camera_param.shape[:2] == (ns, nc), f"camera_param {tuple(camera_param.shape)} vs scenes {ns} cams {nc}"
        self.cam_in.copy_(camera_param.to(self.cam_in.device, F32).permute(0, 1, 3, 2).reshape(ns * nc, -1, 3))
        assert text.shape[0] == ns and text.shape[1] == self.n_text
        self.ctx.view(ns, nc, self.S, -1)[:, :, 1:1 + self.n_text, :] = text.to(self.ctx.device, self.ctx.dtype).unsqueeze(1)
        self.map_in.copy_(bev_map.to(self.map_in.device, F32))
        if self.L > 0:
            assert boxes is not None
            bb, cl, mk = boxes["bboxes"], boxes["classes"], boxes["masks"]
            if bb.shape[1] != nc:                               # view-shared boxes (unet_addon_rawbox.py:785-787)
                assert bb.shape[1] == 1
                bb = bb.expand(ns, nc, *bb.shape[2:]); cl = cl.expand(ns, nc, -1); mk = mk.expand(ns, nc, -1)
            Lb = int(bb.shape[2])
            dynamic = getattr(self, "dynamic", False)   # load() is also called unbound on bare stand-ins (tests/test_host.py), which predate the field
            if dynamic:
                assert 1 <= Lb <= self.L, f"boxes padded to {Lb} but the plan's box capacity is {self.L}"
            else:
                assert Lb == self.L, f"boxes padded to {Lb} but plan built for L={self.L}"
            bb = bb.to(self.box_in.device, F32)
            if self.minmax_normalize:          # normalizer('all-xyz'): (xyz - XYZ_MIN) / XYZ_RANGE (bbox_embedder.py:10-25, :175-176)
                bb = (bb - bb.new_tensor([-200.0, -300.0, -20.0])) / bb.new_tensor([350.0, 650.0, 80.0])
            if Lb == self.L:
                self.box_in.copy_(bb.reshape(-1, *bb.shape[3:]))
                self.box_cls.copy_(cl.to(self.box_cls.device, torch.int64).reshape(-1))
                self.box_mask.copy_(mk.to(self.box_mask.device).reshape(-1).to(torch.uint8))
            else:                              # slots Lb .. capacity of every view: mask 0 -> null embeddings (finite), never attended to
                B = ns * nc
                self.box_in.zero_(); self.box_cls.zero_(); self.box_mask.zero_()
                self.box_in.view(B, self.L, *bb.shape[3:])[:, :Lb].copy_(bb.reshape(B, Lb, *bb.shape[3:]))
                self.box_cls.view(B, self.L)[:, :Lb].copy_(cl.to(self.box_cls.device, torch.int64).reshape(B, Lb))
                self.box_mask.view(B, self.L)[:, :Lb].copy_(mk.to(self.box_mask.device).reshape(B, Lb).to(torch.uint8))
            if dynamic and getattr(self, "per_scene", False):
                # the scene's own padded length, from the masks, with device ops only (no host sync): for the prefix-form masks of
                # _preprocess_bbox / collate_samples this is the length a call of the scene alone pads to
                m = mk.to(self.live.device).reshape(ns, nc * Lb).to(torch.int32)
                pos = torch.arange(1, Lb + 1, dtype=torch.int32, device=m.device).repeat(nc)
                Ls = (m * pos).amax(dim=1)                                               # [ns]; 0: no kept box
                if self.cfg_halves == 2:
                    Ls = Ls[ns // 2:].repeat(2)
                self.live.copy_((1 + self.n_text + Ls).view(ns, 1).expand(ns, nc).reshape(-1))
            elif dynamic:                      # an ordinary stream-ordered device write: no host sync, seen by the next replay
                self.live.fill_(1 + self.n_text + Lb)


def _emit_controlnet(bld: Builder, cn: PackedNet, x_in: torch.Tensor, cond: ConditioningBuffers, temb: TembTable, ctx_kv, h, w):
    """conv_in + map feature, then the encoder copy (unet_addon_rawbox.py:846-880).
    x_in: bf16 [B,h,w,CIN_PAD] — latent channels zero-padded to 8 so conv_in runs on the MFMA implicit-GEMM path."""
    c0 = bld.cfg["block_out_channels"][0]
    x0 = bld.new(bld.B, h, w, c0)
    bld.emit(O.Conv(x_in, cn.conv_cin_padded("conv_in.weight", x_in.shape[3]), x0.bhwc, bias=cn.vec("conv_in.bias"), R=cond.map_rep, ws=bld.ws, name="cn.conv_in+map"))
    return bld.encoder(cn, x0, temb, ctx_kv, "cn")


def _zero_conv_keys(n_skips: int):
    return [f"controlnet_down_blocks.{k}." for k in range(n_skips)]


class SamplerPlan:
    """Everything the DDIM loop needs for `b` scenes (x `n_cam` views, x2 with CFG) on one GPU."""

    def __init__(self, cfg, unet: PackedNet, cn: PackedNet, device, b: int, do_cfg: bool, L_box: int, latent_hw=(28, 50),
                 num_steps: int = 50, guidance_scale: float = 2.0, conditioning_scale: float = 1.0, n_text: int = 77,
                 scheduler_kind: str = "ddim", given_view_mode: int = 0, fork: bool = False, dynamic_boxes=False, health=None, keep_regions: bool = False,
                 resample: Optional[int] = None, stochastic: bool = False):
        """dynamic_boxes: L_box is a box CAPACITY; one plan (and one captured graph) then serves every call whose boxes are padded to
        1 .. L_box: the prologue (box MLP, attn2 to_k / to_v) runs at capacity, and every text-context attention reads its key count
        from cond.live on the device.  Self and cross-view attention are untouched.
        dynamic_boxes="scene": the same with one count per view (cond.live is int32 [B], ops.Attn.tk_rows): every scene of a batched call
        attends to its own boxes only, so its latents equal those of a call of that scene alone up to rounding.
        health: per-view sample-health records of the latents (ops.GroupStats over self.x: one group per view; health_table()).
          None (default): nothing is emitted — prologue and step programs are op for op those of a plan built without the argument.
          "trace": ONE op appended to the step program, behind the scheduler step, row-selected by step_ctr: one record per step and view,
                   written inside the captured step graph (at which step did a view die?).
          "final": no per-step op; run_health() launches one op over the final latents behind the loop.
        keep_regions (with given_view_mode 1): the known views carry a per-pixel keep mask (self.keep, fp32 [b * n_cam, h, w] in [0, 1]: 1 keeps
          the known latent, 0 regenerates, a fraction mixes).  The scheduler op is emitted with its given-view fields OFF and one
          ops.LatentBlend follows it (in front of the health trace op, whose records then see the blended latents): after every step but
          the last, x <- m * add_noise(cond, noise, t_next) + (1 - m) * x.  UniPC's history keeps the values computed from the un-blended
          samples, as under gv_mode 1 (include/mdx.h).  False (default): prologue and step programs are op for op those of today.
        resample (a jump length >= 1; with keep_regions and scheduler_kind "ddim" only): RePaint resampling.  The plan owns visit_ctr (int32 [1],
          jumps taken in this call), seeds (int64 [b * n_cam], one per view) and ONE more program, self.jump = [ops.LatentRenoise]: x is
          diffused forward again by `resample` steps with noise made on the device, step_ctr moves back by as many (time embeddings,
          scheduler row, blend and health trace all select by it), visit_ctr moves on.  The caller launches it between steps
          (schedulers.resample_actions; launch_jump).  The step program is unchanged, op for op.  UniPC is refused: its multistep history
          (x_last, m1, m2) belongs to the trajectory a jump abandons.  None (default): nothing is allocated or built.
        stochastic (scheduler_kind "ddim" only): DDIM with eta > 0.  ops.DdimEtaStep stands in the scheduler op's place (same fields, same
          given views); every other op of the step program, the prologue and the jump program are unchanged: blend, jump and health
          trace read the unchanged 4-column table.  The plan owns var (fp32 [num_steps, 2] = (dir, std) per step, written by load_inputs:
          eta's VALUE is data, one captured plan serves every eta > 0), draw_ctr (int32 [1], zeroed by load_inputs; a jump moves
          step_ctr back and leaves it alone, so a revisited step draws fresh noise) and seeds (int64 [b * n_cam], one per view) — the
          tensor a resample plan already owns: with both switches on there is ONE, and the noise domain separates the two streams.
          False (default): nothing is allocated or built."""
        self.cfg, self.device = cfg, device
        assert health in (None, "final", "trace"), f"health={health!r}: None, 'final' or 'trace'"
        self.health = health
        assert dynamic_boxes in (False, True, "scene"), f"dynamic_boxes={dynamic_boxes!r}: False, True or 'scene'"
        self.dynamic_boxes = bool(dynamic_boxes)
        self.scene_boxes = dynamic_boxes == "scene"
        assert not dynamic_boxes or L_box > 0, "dynamic_boxes needs a box capacity >= 1 (calls without boxes keep their exact plan)"
        assert scheduler_kind in ("ddim", "unipc")
        assert given_view_mode in (0, 1, 2)
        assert not keep_regions or given_view_mode == 1, "keep_regions is the per-pixel form of given_view_mode 1 (re-noised known latents)"
        self.keep_regions = bool(keep_regions)
        assert resample is None or (isinstance(resample, int) and not isinstance(resample, bool) and resample >= 1), f"resample={resample!r}: None or a jump length >= 1"
        assert resample is None or keep_regions, "resample harmonises a kept-region edit: it needs keep_regions"
        assert resample is None or scheduler_kind == "ddim", "resample is DDIM-only: UniPC's multistep history does not survive a jump"
        self.resample = resample
        assert not stochastic or scheduler_kind == "ddim", "stochastic is DDIM with eta > 0: UniPC has no variance noise"
        self.stochastic = bool(stochastic)
        self.scheduler_kind = scheduler_kind
        self.given_view_mode = given_view_mode
        n_cam = len(cfg["neighboring_view_pair"])
        self.b, self.n_cam, self.c = b, n_cam, (2 if do_cfg else 1)
        self.do_cfg = do_cfg
        self.num_steps = num_steps
        h, w = latent_hw
        self.h, self.w = h, w
        B = self.c * b * n_cam
        self.B = B
        Cl = cfg["in_channels"]
        assert unet.dtype == cn.dtype, "UNet and ControlNet must be packed in the same 16-bit type"
        self.dtype = unet.dtype
        bld = Builder(cfg, device, B, n_cam, dtype=self.dtype)
        self.bld = bld
        # state
        self.x = torch.zeros(b * n_cam, h, w, Cl, dtype=F32, device=device)            # latents, NHWC
        self.x_in = torch.zeros(B, h, w, CIN_PAD, dtype=self.dtype, device=device)      # model input ([uncond|cond] copies), channels padded
        self.eps = torch.zeros(B, h, w, cfg["out_channels"], dtype=F32, device=device)
        self.coef = torch.zeros(num_steps, 4 if scheduler_kind == "ddim" else 12, dtype=F32, device=device)
        if scheduler_kind == "unipc":       # multistep history of the fused UniPC update (scheduling_unipc_multistep.py:518-600)
            self.x_last = torch.zeros_like(self.x); self.m1 = torch.zeros_like(self.x); self.m2 = torch.zeros_like(self.x)
        self.step_ctr = torch.zeros(1, dtype=torch.int32, device=device)
        if given_view_mode:       # pipeline_bev_controlnet_given_view.py: known clean latents of some views + every view's initial noise
            self.gv_mask = torch.zeros(b * n_cam, dtype=torch.uint8, device=device)
            self.gv_cond = torch.zeros_like(self.x)
            self.gv_noise = torch.zeros_like(self.x)
        if self.keep_regions:
            self.keep = torch.zeros(b * n_cam, h, w, dtype=F32, device=device)         # one value per latent pixel (mask_elems = Cl)
        if resample is not None or self.stochastic:                                    # one seed per view, for the jumps and the step noise alike
            self.seeds = torch.zeros(b * n_cam, dtype=torch.int64, device=device)
        if self.stochastic:
            self.var = torch.zeros(num_steps, 2, dtype=F32, device=device)
            self.draw_ctr = torch.zeros(1, dtype=torch.int32, device=device)
        # ---------------- prologue ----------------
        self.cond = ConditioningBuffers(bld, cn, cfg, self.c * b, n_cam, L_box, latent_hw, n_text, dynamic=dynamic_boxes, cfg_halves=self.c)
        if self.dynamic_boxes:
            bld.ctx_tk_dev = self.cond.live
            bld.ctx_tk_per_view = self.scene_boxes
        self.temb_cn = TembTable(cn, num_steps, device, per_sample=False)
        self.temb_un = TembTable(unet, num_steps, device, per_sample=False)
        self.temb_cn.sel = self.step_ctr
        self.temb_un.sel = self.step_ctr
        self.temb_cn.emit_fill(bld, cn, cfg)
        self.temb_un.emit_fill(bld, unet, cfg)
        self.kv_cn = build_context_kv(bld, cn, self.cond.ctx, B, self.cond.S)
        self.kv_un = build_context_kv(bld, unet, self.cond.ctx, B, self.cond.S)
        self.prologue_ops = bld.ops
        bld.ops = []
        # ---------------- one denoising step ----------------
        # The ControlNet and the UNet encoder of a step are INDEPENDENT until the zero-convs add the one into the other's skips (both read x_in;
        # unet_addon_rawbox.py:882-910 / unet_2d_condition_multiview.py:464-488).  fork: the two are emitted with SEPARATE buffer pools and workspaces
        # (the pool's aliasing of freed buffers is only safe for ops that execute in order), so that the pipeline may replay them side by side on
        # two streams and join before the zero-convs (round 5: the small-batch operating point, where a launch fills a fraction of the chip and
        # every kernel boundary is a dependency bubble).  The linear program (self.step) stays valid: same ops, same buffers.
        cn_mid, cn_skips = _emit_controlnet(bld, cn, self.x_in, self.cond, self.temb_cn, self.kv_cn, h, w)
        n_cn = len(bld.ops)
        if fork:
            pool_cn = bld.pool
            bld.pool = Pool(device, self.dtype)
            bld.ws = torch.empty_like(bld.ws)
        c0 = cfg["block_out_channels"][0]
        # The decoder's concat buffers [x | skip] exist before the UNet encoder runs: the mid block writes its output into the first one's x half,
        # and each zero-conv below writes `skip + ControlNet residual` straight into its concat's skip half — no concat copy is left in the step
        # (round 5: 13 per step).  The reference adds the residuals out of place (unet_2d_condition_multiview.py:464-488) and
        # concatenates in every up-block layer (unet_2d_blocks.py:1948-1951): same values, one pass instead of three.
        cats = bld.decoder_concats(unet, B, cfg["block_out_channels"][-1], skip_geometry(cfg, h, w))
        u0 = bld.new(B, h, w, c0)
        bld.emit(O.Conv(self.x_in, unet.conv_cin_padded("conv_in.weight", CIN_PAD), u0.bhwc, bias=unet.vec("conv_in.bias"), ws=bld.ws, name="unet.conv_in"))
        u_mid, u_skips = bld.encoder(unet, u0, self.temb_un, self.kv_un, "unet", mid_out=cats[0].channels(0, cfg["block_out_channels"][-1]))
        self.fork_at = (n_cn, len(bld.ops)) if fork else None   # step_ops[:a] ControlNet | [a:b] UNet conv_in + encoder | [b:] zero-convs, decoder, scheduler
        if fork:                                                # behind the join the tail may reuse what either branch has freed
            for k_, v_ in pool_cn.free_list.items():
                bld.pool.free_list.setdefault(k_, []).extend(v_)
            bld.pool.total_bytes += pool_cn.total_bytes
        # zero-convs (unet_addon_rawbox.py:882-910 + unet_2d_condition_multiview.py:464-488): after the UNet encoder + mid consumed the un-added
        # tensors, exactly like the reference's out-of-place `sample + residual`; skip k (encoder order) is popped by decoder layer n - 1 - k
        assert len(cn_skips) == len(u_skips) == len(cats)
        for k, (cs, us) in enumerate(zip(cn_skips, u_skips)):
            key = f"controlnet_down_blocks.{k}."
            cat = cats[len(cats) - 1 - k]
            assert (cat.H, cat.W) == (us.H, us.W)
            dst = cat.channels(cat.C - us.C, cat.C)
            bld.emit(O.Gemm(cs.tok, cn.lin(key + "weight", conditioning_scale), dst.tok, bias=cn.vec(key + "bias", conditioning_scale), R=us.tok, name=f"zero_conv.{k}"))
            bld.free(cs)
            bld.free(us)
        bld.emit(O.Gemm(cn_mid.tok, cn.lin("controlnet_mid_block.weight", conditioning_scale), u_mid.tok,
                        bias=cn.vec("controlnet_mid_block.bias", conditioning_scale), R=u_mid.tok, name="zero_conv.mid"))
        bld.free(cn_mid)
        y = bld.decoder(unet, u_mid, u_skips, self.temb_un, self.kv_un, "unet", cats=cats)
        bld.emit(O.Conv(y.bhwc, unet.conv("conv_out.weight"), self.eps, bias=unet.vec("conv_out.bias"), direct=True, name="unet.conv_out"))
        bld.free(y)
        if scheduler_kind == "ddim":
            gv = {}
            if given_view_mode and not self.keep_regions:
                gv = dict(gv_mask=self.gv_mask, gv_cond=self.gv_cond.view(-1), gv_noise=self.gv_noise.view(-1), gv_mode=given_view_mode,
                          gv_last_step=num_steps - 1)
            if self.stochastic:
                bld.emit(O.DdimEtaStep(self.x.view(-1), self.eps.view(-1), self.coef, self.var, self.step_ctr, self.draw_ctr, seeds=self.seeds,
                                       x_in=self.x_in.view(-1, CIN_PAD), cfg=do_cfg, guidance=guidance_scale, xin_c=Cl, name="cfg+ddim_eta", **gv))
            else:
                bld.emit(O.DdimStep(self.x.view(-1), self.eps.view(-1), self.coef, self.step_ctr, x_in=self.x_in.view(-1, CIN_PAD), cfg=do_cfg,
                                    guidance=guidance_scale, xin_c=Cl, name="cfg+ddim", **gv))
        else:
            gv = {}
            if given_view_mode and not self.keep_regions:
                gv = dict(gv_mask=self.gv_mask, gv_cond=self.gv_cond.view(-1), gv_noise=self.gv_noise.view(-1), gv_mode=given_view_mode,
                          gv_last_step=num_steps - 1)
            bld.emit(O.UniPCStep(self.x.view(-1), self.eps.view(-1), self.coef, self.step_ctr, self.x_last.view(-1), self.m1.view(-1),
                                 self.m2.view(-1), x_in=self.x_in.view(-1, CIN_PAD), cfg=do_cfg, guidance=guidance_scale, xin_c=Cl, name="cfg+unipc", **gv))
        if self.keep_regions:       # behind the scheduler op (which has advanced step_ctr), in front of the health trace op
            bld.emit(O.LatentBlend(self.x.view(-1), self.gv_cond.view(-1), self.gv_noise.view(-1), self.keep.view(-1), self.coef, self.step_ctr,
                                   last_step=num_steps - 1, x_in=self.x_in.view(-1, CIN_PAD), cfg=do_cfg, xin_c=Cl, name="keep_regions"))
        self._health = None
        self.health_ops: List = []
        if health == "trace":
            # the scheduler op has already advanced step_ctr when this op runs: step s selects row s + 1 of the storage.  Row 0 is a pad no
            # step selects, and a replay past the last step selects a row outside the storage (nothing is written).
            self._health = torch.zeros(num_steps + 1, b * n_cam, 4, dtype=F32, device=device)
            bld.emit(O.GroupStats(self.x.view(b * n_cam, -1), self._health, row=self.step_ctr, name="health.trace"))
        elif health == "final":
            self._health = torch.zeros(1, b * n_cam, 4, dtype=F32, device=device)
            self.health_ops = [O.GroupStats(self.x.view(b * n_cam, -1), self._health, name="health.final")]
        self.step_ops = bld.ops
        bld.ops = []
        self.jump_ops: List = []
        self.jump: Optional[L.Program] = None
        if resample is not None:    # a program of its own, launched between steps: one group (one seed) per view
            self.visit_ctr = torch.zeros(1, dtype=torch.int32, device=device)
            self.jump_ops = [O.LatentRenoise(self.x.view(-1), self.coef, self.step_ctr, self.visit_ctr, self.seeds, jump=resample,
                                             x_in=self.x_in.view(-1, CIN_PAD), cfg=do_cfg, xin_c=Cl, name="resample.jump")]
        self.health_prog: Optional[L.Program] = None
        self.prologue: Optional[L.Program] = None
        self.step: Optional[L.Program] = None
        self.step_cn = self.step_enc = self.step_tail = None    # fork: the three parts of the step as programs of their own
        self._ev = None                                         # fork: (ready, done) events of launch_step

    def compile(self):
        self.prologue = O.build_program(self.prologue_ops)
        if self.health_ops:
            self.health_prog = O.build_program(self.health_ops)
        if self.jump_ops:
            self.jump = O.build_program(self.jump_ops)
        if self.fork_at is None:
            self.step = O.build_program(self.step_ops)
        else:
            # a forked plan replays its three parts; the linear program (and its hipGraph) is only built if launch_step ever falls back to it
            a, b_ = self.fork_at
            self.step_cn = O.build_program(self.step_ops[:a])
            self.step_enc = O.build_program(self.step_ops[a:b_])
            self.step_tail = O.build_program(self.step_ops[b_:])

    def launch_step(self, main, side, use_graph: bool = True):
        """One denoising step.  Without fork (or without a side stream): the linear program on `main`.  With fork: the ControlNet on `side`, the UNet
        encoder on `main`, joined before the zero-convs — `main` / `side` are torch streams; everything else the caller does stays on `main`."""
        go = (lambda prog, st: prog.launch(st.cuda_stream)) if use_graph else (lambda prog, st: prog.run(st.cuda_stream))
        if self.fork_at is None or side is None:
            if self.step is None:
                self.step = O.build_program(self.step_ops)
            go(self.step, main)
            return
        if self._ev is None:                                    # two events per plan, re-recorded every step (not two new ones per step)
            self._ev = (torch.cuda.Event(), torch.cuda.Event())
        ready, done = self._ev
        ready.record(main)                                      # x_in of this step: written by the previous step's scheduler kernel on main
        side.wait_event(ready)
        go(self.step_cn, side)
        done.record(side)
        go(self.step_enc, main)
        main.wait_event(done)
        go(self.step_tail, main)

    def launch_jump(self, stream: int, use_graph: bool = True) -> None:
        """One forward jump of a resample plan on `stream` (raw hipStream_t), between two steps: its own captured graph, or eagerly."""
        assert self.jump_ops, "this plan was built without resample"
        if self.jump is None:
            self.jump = O.build_program(self.jump_ops)
        if use_graph:
            self.jump.launch(stream)
        else:
            self.jump.run(stream)

    def health_table(self) -> Optional[torch.Tensor]:
        """The plan's health records on the device, fp32 {nonfinite, absmax, sum, sumsq} per view (view = scene * n_cam + cam):
        "trace": [num_steps, b * n_cam, 4], row s written by step s (rows of steps that have not run yet are zero);
        "final": [1, b * n_cam, 4], written by run_health().  None with health off.  Zeroed by load_inputs."""
        if self._health is None:
            return None
        return self._health[1:] if self.health == "trace" else self._health

    def run_health(self, stream: int) -> None:
        """health="final": the one record launch over the final latents, on `stream` (raw hipStream_t), behind the last step.  Else nothing."""
        if self.health_ops:
            if self.health_prog is None:
                self.health_prog = O.build_program(self.health_ops)
            self.health_prog.run(stream)

    def release(self):
        """Drop the captured graph and every device buffer this plan owns (called on LRU eviction).  The plan's last replay may still
        be in flight (an output_type='latent' caller that has not synchronised): destroying a hipGraphExec / freeing its buffers under
        a running graph is not safe, so the device is drained first (evictions are rare: once per new batch geometry)."""
        if self.device is not None and torch.device(self.device).type == "cuda":
            torch.cuda.synchronize(self.device)
        for prog in (self.prologue, self.step, self.step_cn, self.step_enc, self.step_tail, self.jump):
            if prog is not None:
                prog.destroy()
        self.prologue = self.step = self.step_cn = self.step_enc = self.step_tail = self.jump = None
        self.prologue_ops = self.step_ops = []
        self.jump_ops = []
        self.health_ops, self.health_prog = [], None
        self.bld = None
        self.cond = self.temb_cn = self.temb_un = self.kv_cn = self.kv_un = None

    # ---- per-call inputs ----
    def load_inputs(self, latents: torch.Tensor, camera_param, text, bev_map, boxes, timesteps: torch.Tensor, coef: torch.Tensor,
                    given_mask: Optional[torch.Tensor] = None, given_latents: Optional[torch.Tensor] = None,
                    keep_mask: Optional[torch.Tensor] = None, seeds: Optional[torch.Tensor] = None, var: Optional[torch.Tensor] = None):
        """latents (b, n_cam, C, h, w) any float dtype; camera/text/map/boxes already hold the [uncond | cond] halves.
        given_mask (b, n_cam) bool + given_latents (b, n_cam, C, h, w): the known views of a given-view plan.
        keep_mask (b, n_cam, h, w) in [0, 1], a keep_regions plan only (validated by the caller; zero on views that are not given): the
        first sample is m * add_noise(cond, noise, t_0) + (1 - m) * noise, with exact m == 1 / m == 0 taking the term itself.
        seeds (b,) int64, a resample plan only: one seed per scene, replicated over its views (the jump noise is shared across the views
        of a scene like the initial noise); visit_ctr restarts at zero.
        var (num_steps, 2) fp32, a stochastic plan only (DDIMScheduler.variance_table(eta)), with the same seeds: draw_ctr restarts at zero."""
        b, nc = self.b, self.n_cam
        assert latents.shape[:2] == (b, nc)
        xl = latents.to(self.device, F32).reshape(b * nc, *latents.shape[2:]).permute(0, 2, 3, 1).contiguous()
        if self.given_view_mode:
            assert given_mask is not None and given_latents is not None and tuple(given_mask.shape) == (b, nc)
            gm = given_mask.to(self.device).reshape(-1).bool()
            self.gv_mask.copy_(gm.to(torch.uint8))
            self.gv_noise.copy_(xl)                                                  # original_noise (:263)
            self.gv_cond.copy_(given_latents.to(self.device, F32).reshape(b * nc, *latents.shape[2:]).permute(0, 2, 3, 1))
            c0 = coef[0].to(self.device, F32)                                        # add_noise at the first timestep (:265-275, :284-291)
            if self.scheduler_kind == "ddim":
                a0, s0 = c0[0], c0[1]                                                # DDIM row: sqrt(acp_t), sqrt(1 - acp_t), ...
            else:
                a0, s0 = 1.0 / c0[0], -c0[1] / c0[0]                                 # UniPC row: a = 1 / alpha_t, b = -sigma_t / alpha_t
            t0 = a0 * self.gv_cond + s0 * self.gv_noise
            if self.keep_regions:
                assert keep_mask is not None and tuple(keep_mask.shape) == (b, nc, self.h, self.w), "keep_mask must be (b, n_cam, h, w)"
                self.keep.copy_(keep_mask.to(self.device, F32).reshape(b * nc, self.h, self.w))
                m = self.keep.unsqueeze(-1)
                xl = torch.where(m == 1, t0, torch.where(m == 0, xl, m * t0 + (1 - m) * xl))
            else:
                assert keep_mask is None, "this plan was built without keep_regions"
                xl = torch.where(gm.view(-1, 1, 1, 1), t0, xl)
        else:
            assert given_mask is None, "this plan was built without given views"
            assert keep_mask is None, "this plan was built without keep_regions"
        self.x.copy_(xl)
        self.x_in.view(self.c, b * nc, self.h, self.w, CIN_PAD)[..., :xl.shape[-1]].copy_(self.x.unsqueeze(0).expand(self.c, *self.x.shape))
        self.cond.load(camera_param, text, bev_map, boxes)
        t = timesteps.to(self.device, F32)
        assert t.numel() == self.num_steps
        self.temb_cn.t.copy_(t); self.temb_un.t.copy_(t)
        self.coef.copy_(coef.to(self.device, F32))
        self.step_ctr.zero_()
        if self.resample is not None or self.stochastic:
            assert seeds is not None and tuple(seeds.shape) == (b,) and seeds.dtype == torch.int64, "seeds must be (b,) int64"
            self.seeds.copy_(seeds.to(self.device).repeat_interleave(nc))
        else:
            assert seeds is None, "this plan was built without resample"
        if self.resample is not None:
            self.visit_ctr.zero_()
        if self.stochastic:
            assert var is not None and tuple(var.shape) == (self.num_steps, 2), "var must be (num_steps, 2): DDIMScheduler.variance_table(eta)"
            self.var.copy_(var.to(self.device, F32))
            self.draw_ctr.zero_()
        else:
            assert var is None, "this plan was built without stochastic"
        if self._health is not None:
            self._health.zero_()
        if self.scheduler_kind == "unipc":
            self.x_last.zero_(); self.m1.zero_(); self.m2.zero_()

    def run(self, use_graph: bool = True) -> torch.Tensor:
        """prologue + num_steps denoising steps on the current stream; returns latents (b, n_cam, C, h, w) fp32."""
        if self.prologue is None:
            self.compile()
        if self.step is None:
            self.step = O.build_program(self.step_ops)
        st = _stream(self.device)
        self.prologue.run(st)
        for _ in range(self.num_steps):
            if use_graph:
                self.step.launch(st)
            else:
                self.step.run(st)
        self.run_health(st)
        return self.latents()

    def latents(self) -> torch.Tensor:
        return self.x.view(self.b, self.n_cam, self.h, self.w, -1).permute(0, 1, 4, 2, 3).contiguous()

    def latents_on(self, stream) -> torch.Tensor:
        """latents() as a copy made on `stream` (a torch stream that already waits for this plan's last replay)."""
        with torch.cuda.stream(stream):
            return self.latents()


class ControlNetPlan:
    """BEVControlNetModel.forward at a fixed geometry: returns 12 down residuals + mid (NCHW) + ehs_with_cam."""

    def __init__(self, cfg, cn: PackedNet, device, n_scene: int, L_box: int, latent_hw, conditioning_scale: float = 1.0, n_text: int = 77):
        n_cam = len(cfg["neighboring_view_pair"])
        B = n_scene * n_cam
        h, w = latent_hw
        self.cfg, self.device, self.B, self.n_scene, self.n_cam, self.h, self.w = cfg, device, B, n_scene, n_cam, h, w
        self.dtype = cn.dtype
        bld = Builder(cfg, device, B, n_cam, dtype=self.dtype)
        self.bld = bld
        self.sample_nchw = torch.zeros(B, cfg["in_channels"], h, w, dtype=F32, device=device)
        self.x_in = torch.zeros(B, h, w, CIN_PAD, dtype=self.dtype, device=device)
        bld.emit(O.Layout(self.sample_nchw, self.x_in[..., :cfg["in_channels"]], True, name="cn.sample.nhwc"))
        self.cond = ConditioningBuffers(bld, cn, cfg, n_scene, n_cam, L_box, latent_hw, n_text)
        self.temb = TembTable(cn, B, device, per_sample=True)        # one timestep per view row
        self.temb.emit_fill(bld, cn, cfg)
        self.kv = build_context_kv(bld, cn, self.cond.ctx, B, self.cond.S)
        mid, skips = _emit_controlnet(bld, cn, self.x_in, self.cond, self.temb, self.kv, h, w)
        self.down_out: List[torch.Tensor] = []
        for k, s in enumerate(skips):
            key = f"controlnet_down_blocks.{k}."
            r = bld.new(s.B, s.H, s.W, s.C)
            bld.emit(O.Gemm(s.tok, cn.lin(key + "weight", conditioning_scale), r.tok, bias=cn.vec(key + "bias", conditioning_scale), name=f"zero_conv.{k}"))
            o = torch.zeros(s.B, s.C, s.H, s.W, dtype=self.dtype, device=device)
            bld.emit(O.Layout(r.bhwc, o, False, name=f"res{k}.nchw"))
            self.down_out.append(o)
        r = bld.new(mid.B, mid.H, mid.W, mid.C)
        bld.emit(O.Gemm(mid.tok, cn.lin("controlnet_mid_block.weight", conditioning_scale), r.tok, bias=cn.vec("controlnet_mid_block.bias", conditioning_scale), name="zero_conv.mid"))
        self.mid_out = torch.zeros(mid.B, mid.C, mid.H, mid.W, dtype=self.dtype, device=device)
        bld.emit(O.Layout(r.bhwc, self.mid_out, False, name="mid.nchw"))
        self.ops = bld.ops
        self.program: Optional[L.Program] = None

    def run(self, sample, timestep, camera_param, boxes, text, bev_map):
        if self.program is None:
            self.program = O.build_program(self.ops)
        self.sample_nchw.copy_(sample.to(self.device, F32).reshape(self.B, *sample.shape[-3:]))
        t = torch.as_tensor(timestep).to(self.device, F32).reshape(-1)
        if t.numel() == 1:
            t = t.expand(self.n_scene)
        if t.numel() == self.n_scene:
            t = t.repeat_interleave(self.n_cam)                      # unet_addon_rawbox.py:840-841
        self.temb.t.copy_(t)
        self.cond.load(camera_param, text, bev_map, boxes)
        with torch.cuda.device(self.device):
            self.program.run(_stream(self.device))
        return self.down_out, self.mid_out, self.cond.ctx


class UNetPlan:
    """UNet2DConditionModelMultiview.forward at a fixed geometry (sample (B,4,h,w), ehs (B,S,D), residuals)."""

    def __init__(self, cfg, unet: PackedNet, device, B: int, S: int, latent_hw, with_residuals: bool = True):
        n_cam = len(cfg["neighboring_view_pair"])
        assert B % n_cam == 0, "batch must hold whole scenes: (b n) views (blocks.py:196-197)"
        h, w = latent_hw
        self.cfg, self.device, self.B, self.S, self.h, self.w = cfg, device, B, S, h, w
        self.dtype = unet.dtype
        bld = Builder(cfg, device, B, n_cam, dtype=self.dtype)
        self.bld = bld
        D = cfg["cross_attention_dim"]
        self.sample_nchw = torch.zeros(B, cfg["in_channels"], h, w, dtype=F32, device=device)
        self.x_in = torch.zeros(B, h, w, CIN_PAD, dtype=self.dtype, device=device)
        self.ctx = torch.zeros(B, S, D, dtype=self.dtype, device=device)
        bld.emit(O.Layout(self.sample_nchw, self.x_in[..., :cfg["in_channels"]], True, name="unet.sample.nhwc"))
        self.temb = TembTable(unet, B, device, per_sample=True)
        self.temb.emit_fill(bld, unet, cfg)
        self.kv = build_context_kv(bld, unet, self.ctx, B, S)
        c0 = cfg["block_out_channels"][0]
        u0 = bld.new(B, h, w, c0)
        bld.emit(O.Conv(self.x_in, unet.conv_cin_padded("conv_in.weight", CIN_PAD), u0.bhwc, bias=unet.vec("conv_in.bias"), ws=bld.ws, name="unet.conv_in"))
        mid, skips = bld.encoder(unet, u0, self.temb, self.kv, "unet")
        self.res_in: List[torch.Tensor] = []
        self.mid_in = None
        if with_residuals:
            for k, s in enumerate(skips):
                rin = torch.zeros(s.B, s.C, s.H, s.W, dtype=self.dtype, device=device)
                rn = bld.new(s.B, s.H, s.W, s.C)
                bld.emit(O.Layout(rin, rn.bhwc, True, name=f"res{k}.nhwc"))
                bld.emit(O.Ew(L.EW_ADD, rn.tok, s.tok, name=f"skip{k}+=res"))
                bld.free(rn)
                self.res_in.append(rin)
            self.mid_in = torch.zeros(mid.B, mid.C, mid.H, mid.W, dtype=self.dtype, device=device)
            rn = bld.new(mid.B, mid.H, mid.W, mid.C)
            bld.emit(O.Layout(self.mid_in, rn.bhwc, True, name="midres.nhwc"))
            bld.emit(O.Ew(L.EW_ADD, rn.tok, mid.tok, name="mid+=res"))
            bld.free(rn)
        y = bld.decoder(unet, mid, skips, self.temb, self.kv, "unet")
        self.eps_nhwc = torch.zeros(B, h, w, cfg["out_channels"], dtype=F32, device=device)
        bld.emit(O.Conv(y.bhwc, unet.conv("conv_out.weight"), self.eps_nhwc, bias=unet.vec("conv_out.bias"), direct=True, name="unet.conv_out"))
        self.out_nchw = torch.zeros(B, cfg["out_channels"], h, w, dtype=F32, device=device)
        bld.emit(O.Layout(self.eps_nhwc, self.out_nchw, False, name="eps.nchw"))
        self.ops = bld.ops
        self.program: Optional[L.Program] = None

    def run(self, sample, timestep, ehs, down_res=None, mid_res=None):
        if self.program is None:
            self.program = O.build_program(self.ops)
        self.sample_nchw.copy_(sample.to(self.device, F32))
        t = torch.as_tensor(timestep).to(self.device, F32).reshape(-1)
        self.temb.t.copy_(t.expand(self.B) if t.numel() == 1 else t)
        self.ctx.copy_(ehs.to(self.device, self.dtype))
        if self.res_in:
            assert down_res is not None and len(down_res) == len(self.res_in)
            for dst, src in zip(self.res_in, down_res):
                dst.copy_(src.to(self.device, self.dtype))
            self.mid_in.copy_(mid_res.to(self.device, self.dtype))
        with torch.cuda.device(self.device):
            self.program.run(_stream(self.device))
        return self.out_nchw
