"""CLIP text encoder (transformers models/clip/modeling_clip.py: CLIPTextTransformer) as one op program on the library's kernels.

Per prompt batch [B, T]:
    x = token_embedding[ids] + position_embedding[:T]                one gather with an added row (MdxGatherDesc.add)
    per layer:  n = LayerNorm1(x)
                qkv = n [Wq; Wk; Wv]^T + [bq; bk; bv]                one GEMM, N = 3 C
                o = causal attention(q, k, v, scale = d^-0.5)        the three column blocks of qkv, V row-major (csrc/attention_short.hip)
                x = o Wo^T + bo + x                                  residual in the GEMM epilogue
                n = LayerNorm2(x)
                f = quick_gelu(n W1^T + b1);  x = f W2^T + b2 + x
    last_hidden_state = final_layer_norm(x)
quick_gelu(u) = u sigmoid(1.702 u) = silu(1.702 u) / 1.702, so fc1 is packed as 1.702 (W1, b1) under the GEMM's SiLU epilogue and fc2 as
W2 / 1.702: no new epilogue.  The program is captured once per (B, T) and replayed as a hipGraph; the ids are its only input.
"""
from __future__ import annotations

from typing import List

import torch

from . import _lib as L
from . import ops as O
from .engine import PackedNet, Pool

F32 = torch.float32
QUICK_GELU = 1.702


class TextEncoderPlan:
    def __init__(self, cfg, net: PackedNet, device, B: int, T: int):
        self.cfg, self.device, self.B, self.T = cfg, device, B, T
        C, I, H = cfg["hidden_size"], cfg["intermediate_size"], cfg["num_attention_heads"]
        eps = float(cfg.get("layer_norm_eps", 1e-5))
        M = B * T
        self.ops: List[object] = []
        self.keep: List[torch.Tensor] = []
        self.ws = torch.empty(16 * 1024 * 1024 // 4, dtype=F32, device=device)
        emit = self.ops.append
        H16 = net.dtype

        def buf(*shape, dtype=H16):
            n_ = 1
            for d_ in shape:
                n_ *= int(d_)
            t = Pool.alloc(n_, dtype, device).view(*shape)
            self.keep.append(t)
            return t

        def ln(x, y, pre):
            emit(O.LayerNorm(x, y, net.vec(pre + "weight"), net.vec(pre + "bias"), eps, name="clip." + pre))
            return y

        # one set of activation buffers for all layers: the program runs in order on one stream, and a layer reads nothing of the previous
        # one but its output x (two buffers: out_proj writes xb = .. + xa, fc2 writes xa = .. + xb)
        self.ids = torch.zeros(M, dtype=torch.int64, device=device)
        xa, xb, n, o = buf(M, C), buf(M, C), buf(M, C), buf(B, T, C)
        qkv, f = buf(M, 3 * C), buf(M, I)
        q3 = qkv.view(B, T, 3 * C)
        emit(O.Gather(net.table("embeddings.token_embedding.weight"), xa, self.ids, add=net.table("embeddings.position_embedding.weight")[:T],
                      name="clip.embeddings"))
        for i in range(cfg["num_hidden_layers"]):
            p = f"encoder.layers.{i}."
            a = p + "self_attn."
            ln(xa, n, p + "layer_norm1.")
            emit(O.Gemm(n, net.cat_lin([a + "q_proj.weight", a + "k_proj.weight", a + "v_proj.weight"]), qkv,
                        bias=net.cat_vec([a + "q_proj.bias", a + "k_proj.bias", a + "v_proj.bias"]), ws=self.ws, name="clip." + a + "qkv"))
            emit(O.Attn(q3[:, :, :C], q3[:, :, C:2 * C], q3[:, :, 2 * C:], o, heads=H, Tk=T, scale=float(C // H) ** -0.5, causal=True, v_rowmajor=True,
                        name="clip." + a + "attn"))
            emit(O.Gemm(o.view(M, C), net.lin(a + "out_proj.weight"), xb, bias=net.vec(a + "out_proj.bias"), R=xa, ws=self.ws, name="clip." + a + "out"))
            ln(xb, n, p + "layer_norm2.")
            emit(O.Gemm(n, net.lin(p + "mlp.fc1.weight", QUICK_GELU), f, bias=net.vec(p + "mlp.fc1.bias", QUICK_GELU), epilogue=L.EPI_SILU,
                        ws=self.ws, name="clip." + p + "fc1"))
            emit(O.Gemm(f, net.lin(p + "mlp.fc2.weight", 1.0 / QUICK_GELU), xa, bias=net.vec(p + "mlp.fc2.bias"), R=xb, ws=self.ws, name="clip." + p + "fc2"))
        self.out = ln(xa, buf(M, C), "final_layer_norm.").view(B, T, C)
        self.program = None

    def compile(self):
        self.program = O.build_program(self.ops)

    def run(self, input_ids: torch.Tensor, graph: bool = True) -> torch.Tensor:
        """input_ids [B, T] -> last_hidden_state [B, T, hidden] in the plan's 16-bit type (a fresh tensor)."""
        if self.program is None:
            self.compile()
        with torch.cuda.device(self.device):
            self.ids.copy_(input_ids.reshape(-1).to(self.device, torch.int64))
            stream = torch.cuda.current_stream(self.device).cuda_stream
            if graph:
                self.program.launch(stream)
            else:
                self.program.run(stream)
            return self.out.clone()

    def release(self):
        if self.program is not None:
            self.program.destroy()
        self.program = None
        self.ops, self.keep = [], []
