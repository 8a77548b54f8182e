"""Plain-torch fp32 restatement of transformers' CLIPTextModel forward (models/clip/modeling_clip.py: CLIPTextEmbeddings, CLIPEncoderLayer
under the causal mask, final_layer_norm) — the reference of tests/test_clip_text*.py.  `cast`, when given, is applied wherever the HIP
program (magicdrive_amd/text_encoder.py) stores an activation in its 16-bit type: the embedding sum, every LayerNorm output, the attention
output, the two residual sums and the fc1 activation.  (The HIP path rounds at two more points, the fused q/k/v store and P before PV.)"""
import torch
import torch.nn.functional as F

PREFIX = "text_model."


def strip(sd):
    return {(k[len(PREFIX):] if k.startswith(PREFIX) else k): v.float() for k, v in sd.items() if not k.endswith("position_ids")}


def quick_gelu(x):
    return x * torch.sigmoid(1.702 * x)


def clip_text_forward(cfg, sd, ids, cast=None):
    """ids int64 [B, T] -> last_hidden_state fp32 [B, T, hidden]."""
    c = cast or (lambda t: t)
    sd = strip(sd)
    C, H, eps = cfg["hidden_size"], cfg["num_attention_heads"], cfg.get("layer_norm_eps", 1e-5)
    B, T = ids.shape
    d = C // H
    x = c(sd["embeddings.token_embedding.weight"][ids] + sd["embeddings.position_embedding.weight"][:T][None])
    mask = torch.full((T, T), float("-inf")).triu(1)
    for i in range(cfg["num_hidden_layers"]):
        p = f"encoder.layers.{i}."
        n = c(F.layer_norm(x, (C,), sd[p + "layer_norm1.weight"], sd[p + "layer_norm1.bias"], eps))
        q, k, v = (F.linear(n, sd[p + f"self_attn.{w}_proj.weight"], sd[p + f"self_attn.{w}_proj.bias"]).view(B, T, H, d).transpose(1, 2) for w in "qkv")
        o = c((torch.softmax(q @ k.transpose(-1, -2) * d ** -0.5 + mask, -1) @ v).transpose(1, 2).reshape(B, T, C))
        x = c(F.linear(o, sd[p + "self_attn.out_proj.weight"], sd[p + "self_attn.out_proj.bias"]) + x)
        n = c(F.layer_norm(x, (C,), sd[p + "layer_norm2.weight"], sd[p + "layer_norm2.bias"], eps))
        f = c(quick_gelu(F.linear(n, sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"])))
        x = c(F.linear(f, sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"]) + x)
    return c(F.layer_norm(x, (C,), sd["final_layer_norm.weight"], sd["final_layer_norm.bias"], eps))


def caster(dtype):
    return lambda t: t.to(dtype).float()
