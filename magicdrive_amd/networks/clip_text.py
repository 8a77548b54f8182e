"""CLIPTextModel — drop-in for the `text_encoder` the reference pipeline encodes prompts with (pipeline_bev_controlnet.py:148-165 ->
transformers CLIPTextModel, models/clip/modeling_clip.py: CLIPTextEmbeddings, CLIPEncoderLayer x N under a causal mask, final_layer_norm).

Only what that caller touches is built: `text_encoder(input_ids)[0]` / `.last_hidden_state` ([B, T, hidden] in the model dtype), `.to()`,
`.eval()`, `.dtype`, `.device`, `.parameters()`, `.config`, `from_pretrained` on the SD-1.5 layout `<sd15>/text_encoder/{config.json,
model.safetensors | pytorch_model.bin}` — read without importing transformers.  `pooler_output` is not produced (the pipeline reads `[0]`
only), `hidden_act="gelu"` (OpenCLIP) is refused, a tokenizer is the caller's.  The arithmetic is one op program on libmdx
(magicdrive_amd/text_encoder.py); there is no CPU path.
"""
from __future__ import annotations

import json
import os
from collections import OrderedDict
from types import SimpleNamespace
from typing import Dict, Optional

import torch

from ..engine import PackedNet
from ..denoiser import PlanCache

CONFIG_NAME = "config.json"
WEIGHT_FILES = ("model.safetensors", "pytorch_model.bin")
PREFIX = "text_model."

# openai/clip-vit-large-patch14's text tower: what SD-1.5 ships under text_encoder/
CLIP_SD15_CONFIG = dict(vocab_size=49408, hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12,
                        max_position_embeddings=77, hidden_act="quick_gelu", layer_norm_eps=1e-5)


def clip_text_param_shapes(cfg: Dict) -> "OrderedDict[str, tuple]":
    """Tensor names (without the `text_model.` prefix) and shapes of transformers' CLIPTextModel for `cfg`."""
    C, I = cfg["hidden_size"], cfg["intermediate_size"]
    s: "OrderedDict[str, tuple]" = OrderedDict()
    s["embeddings.token_embedding.weight"] = (cfg["vocab_size"], C)
    s["embeddings.position_embedding.weight"] = (cfg["max_position_embeddings"], C)
    for i in range(cfg["num_hidden_layers"]):
        p = f"encoder.layers.{i}."
        for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
            s[p + f"self_attn.{n}.weight"] = (C, C)
            s[p + f"self_attn.{n}.bias"] = (C,)
        for n in ("layer_norm1", "layer_norm2"):
            s[p + n + ".weight"] = (C,)
            s[p + n + ".bias"] = (C,)
        s[p + "mlp.fc1.weight"] = (I, C); s[p + "mlp.fc1.bias"] = (I,)
        s[p + "mlp.fc2.weight"] = (C, I); s[p + "mlp.fc2.bias"] = (C,)
    s["final_layer_norm.weight"] = (C,)
    s["final_layer_norm.bias"] = (C,)
    return s


def random_clip_state_dict(cfg: Dict, seed: int) -> "OrderedDict[str, torch.Tensor]":
    """Seeded init for parity tests: linear weights U(+-1/sqrt(fan_in)) (q / k twice that, so the attention maps are not flat), norm gains
    1 + 0.1 N, biases 0.05 N, embeddings N(0, 0.02^2) / N(0, 0.01^2) as CLIP initialises them.  The q / k gain decides how much a 16-bit store
    ahead of the softmax moves the output: at 2x the 12-layer SD-1.5 geometry loses 7.8e-3 (bf16) / 9.8e-4 (fp16) rel L2 to its 16-bit
    stores (tests/clip_text_ref.py with `cast`); at 4x it would be 4.3e-2, too wide a band for a parity test to mean much."""
    g = torch.Generator().manual_seed(seed)
    sd: "OrderedDict[str, torch.Tensor]" = OrderedDict()
    for name, shape in clip_text_param_shapes(cfg).items():
        if "layer_norm" in name:
            t = 1.0 + 0.1 * torch.randn(shape, generator=g) if name.endswith("weight") else 0.05 * torch.randn(shape, generator=g)
        elif name.endswith("bias"):
            t = 0.05 * torch.randn(shape, generator=g)
        elif "embedding" in name:
            t = torch.randn(shape, generator=g) * (0.02 if "token" in name else 0.01)
        else:
            t = (torch.rand(shape, generator=g) * 2 - 1) * shape[1] ** -0.5 * (2.0 if ("q_proj" in name or "k_proj" in name) else 1.0)
        sd[name] = t
    return sd


def _check_config(cfg: Dict) -> None:
    act = cfg.get("hidden_act", "quick_gelu")
    if act != "quick_gelu":
        raise NotImplementedError(f"CLIPTextModel hidden_act={act!r}: only quick_gelu (SD-1.5's CLIP ViT-L/14) is built; it rides on the GEMM's SiLU epilogue")
    C, H = cfg["hidden_size"], cfg["num_attention_heads"]
    if C % H or C // H not in (32, 64):
        raise NotImplementedError(f"CLIPTextModel head dim {C}/{H}: the short-sequence attention kernel serves 32 and 64")
    if C % 8 or C > 2048 or cfg["intermediate_size"] % 8:
        raise NotImplementedError(f"CLIPTextModel hidden_size={C}, intermediate_size={cfg['intermediate_size']}: need multiples of 8, hidden <= 2048 (LayerNorm kernel)")
    if cfg["max_position_embeddings"] > 128:
        raise NotImplementedError(f"CLIPTextModel max_position_embeddings={cfg['max_position_embeddings']}: the short-sequence attention kernel serves T <= 128")


class CLIPTextModelOutput:
    """`out[0]` / `out.last_hidden_state` (transformers' BaseModelOutputWithPooling without the pooled vector)."""

    def __init__(self, last_hidden_state: torch.Tensor):
        self.last_hidden_state = last_hidden_state

    def __getitem__(self, i):
        return (self.last_hidden_state,)[i]


class CLIPTextModel:
    def __init__(self, cfg: Dict, state_dict: Dict[str, torch.Tensor], torch_dtype=torch.bfloat16):
        self.cfg = dict(CLIP_SD15_CONFIG)
        self.cfg.update({k: v for k, v in cfg.items() if v is not None})
        _check_config(self.cfg)
        shapes = clip_text_param_shapes(self.cfg)
        # SD-1.5 checkpoints name the tensors text_model.<...>; newer transformers save them without the prefix
        sd = {(k[len(PREFIX):] if k.startswith(PREFIX) else k): v for k, v in state_dict.items()}
        sd.pop("embeddings.position_ids", None)
        missing = [k for k in shapes if k not in sd]
        if missing:
            raise KeyError(f"CLIPTextModel: state dict lacks {len(missing)} tensors, e.g. {missing[:4]}")
        for k, shp in shapes.items():
            if tuple(sd[k].shape) != tuple(shp):
                raise ValueError(f"CLIPTextModel: {k} has shape {tuple(sd[k].shape)}, config implies {tuple(shp)}")
        self._sd = OrderedDict((k, sd[k].detach()) for k in shapes)
        self._dtype = torch_dtype
        self._device = torch.device("cpu")
        self._packed: Optional[PackedNet] = None
        self._plans = PlanCache()
        self.config = SimpleNamespace(**self.cfg)
        self.use_graph = True

    @classmethod
    def from_config(cls, cfg: Dict, seed: int = 0, torch_dtype=torch.bfloat16):
        full = dict(CLIP_SD15_CONFIG)
        full.update(cfg)
        _check_config(full)
        return cls(full, random_clip_state_dict(full, seed), torch_dtype)

    @classmethod
    def from_pretrained(cls, path: str, torch_dtype=torch.bfloat16, subfolder: Optional[str] = None, **unused):
        d = os.path.join(path, subfolder) if subfolder else path
        with open(os.path.join(d, CONFIG_NAME)) as f:
            js = json.load(f)
        js = js.get("text_config", js) if "hidden_size" not in js else js
        cfg = {k: js[k] for k in CLIP_SD15_CONFIG if k in js}
        _check_config({**CLIP_SD15_CONFIG, **cfg})
        for name in WEIGHT_FILES:
            fp = os.path.join(d, name)
            if os.path.exists(fp):
                if name.endswith(".safetensors"):
                    from safetensors.torch import load_file
                    sd = load_file(fp)
                else:
                    sd = torch.load(fp, map_location="cpu")
                return cls(cfg, sd, torch_dtype)
        raise FileNotFoundError(f"no {' / '.join(WEIGHT_FILES)} under {d}")

    # ---- torch-module-like surface ----
    def state_dict(self):
        return self._sd

    def parameters(self):
        return iter(self._sd.values())

    def eval(self):
        return self

    def to(self, *args, **kw):
        """.to(device) / .to(dtype) / .to(device, dtype) / .to(dtype=...) like a torch module (dtype = the type of last_hidden_state)."""
        for a in list(args) + list(kw.values()):
            if isinstance(a, torch.dtype):
                if (a == torch.float16) != (self._dtype == torch.float16):
                    self._packed = None
                    self._plans.clear()
                self._dtype = a
            elif isinstance(a, (str, torch.device)):
                dev = torch.device(a)
                if dev != self._device:
                    self._device, self._packed = dev, None
                    self._plans.clear()
        return self

    @property
    def dtype(self):
        return self._dtype

    @property
    def device(self):
        return self._device

    def packed(self) -> PackedNet:
        if self._packed is None:
            # arithmetic type: fp16 when the model was asked for in fp16, bf16 otherwise (operands are 16-bit on the MFMA path either way)
            self._packed = PackedNet(self._sd, self._device, torch.float16 if self._dtype == torch.float16 else torch.bfloat16)
        return self._packed

    @torch.no_grad()
    def __call__(self, input_ids: torch.Tensor, attention_mask=None, **unused):
        """input_ids int [B, T], T <= max_position_embeddings -> CLIPTextModelOutput(last_hidden_state [B, T, hidden])."""
        from ..text_encoder import TextEncoderPlan
        if attention_mask is not None:
            raise NotImplementedError("CLIPTextModel: a padding mask is not built (the reference pipeline passes input_ids only)")
        if self._device.type != "cuda":
            raise RuntimeError("CLIPTextModel.to('cuda') first: the text encoder has no CPU path")
        if input_ids.dim() != 2 or input_ids.shape[1] > self.cfg["max_position_embeddings"] or input_ids.shape[1] < 1:
            raise ValueError(f"input_ids {tuple(input_ids.shape)}: need [B, T] with 1 <= T <= {self.cfg['max_position_embeddings']}")
        B, T = input_ids.shape
        if B == 0:
            return CLIPTextModelOutput(torch.empty(0, T, self.cfg["hidden_size"], dtype=self._dtype, device=self._device))
        key = (B, T)
        plan = self._plans.get(key)
        if plan is None:
            with torch.cuda.device(self._device):
                plan = TextEncoderPlan(self.cfg, self.packed(), self._device, B, T)
                plan.compile()
            self._plans.put(key, plan)
        return CLIPTextModelOutput(plan.run(input_ids, graph=self.use_graph).to(self._dtype))
