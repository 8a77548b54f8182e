"""-m gpu: the short-sequence attention kernel (csrc/attention_short.hip: V row-major, causal), the gather with an added row, the CLIP text
encoder built on them (magicdrive_amd/networks/clip_text.py) and its place in the pipeline — bf16 and fp16.

Measured on MI355X (profiles/clip_text_parity_measured.jsonl): see the docstrings of the network tests."""
import ctypes
import os
from types import SimpleNamespace

import pytest
import torch

import clip_text_ref as R
from helpers import check, close, parity_log, rel_l2
from magicdrive_amd import _lib as L
from magicdrive_amd import ops as O
from magicdrive_amd.networks.clip_text import CLIPTextModel

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [pytest.param(torch.bfloat16, id="bf16"), pytest.param(torch.float16, id="f16")]
KIND = {torch.bfloat16: "bf16", torch.float16: "f16"}


def attn_ref(q, k, v, H, scale, causal):
    """fp32 softmax(q k^T scale [+ causal mask]) v on the 16-bit inputs; q [B,Tq,C], k / v [B,Tk,C]."""
    B, Tq, C = q.shape
    Tk = k.shape[1]
    d = C // H
    qf, kf, vf = (t.float().view(B, -1, H, d).transpose(1, 2) for t in (q, k, v))
    s = qf @ kf.transpose(-1, -2) * scale
    if causal:
        s = s + torch.full((Tq, Tk), float("-inf"), device=q.device).triu(1)
    return (torch.softmax(s, -1) @ vf).transpose(1, 2).reshape(B, Tq, C)


def run_attn(q, k, v, o, H, causal):
    d = q.shape[2] // H
    O.run_ops([O.Attn(q, k, v, o, heads=H, Tk=k.shape[1], scale=d ** -0.5, causal=causal, v_rowmajor=True)])
    tag = (L.lib().mdx_last_kernel() or b"").decode()
    assert tag == f"attn_short_kernel<{d},{'causal' if causal else 'full'}>", tag
    torch.cuda.synchronize()
    return tag


def rand16(shape, dtype, dev, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g).to(dtype).to(dev)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("B,H", [(1, 1), (3, 12)])
@pytest.mark.parametrize("d", [32, 64])
@pytest.mark.parametrize("T", [1, 16, 17, 33, 64, 65, 77, 128])
def test_short_attention_vs_torch(dev, T, d, B, H, causal, dtype):
    C = H * d
    q, k, v = (rand16((B, T, C), dtype, dev, 100 * T + d + i) for i in range(3))
    o = torch.full((B, T, C), float("nan"), dtype=dtype, device=dev)
    tag = run_attn(q, k, v, o, H, causal)
    parity_log("clip_text:kernel", kernel=tag, T=T, d=d, B=B, H=H, dtype=KIND[dtype])
    close(o, attn_ref(q, k, v, H, d ** -0.5, causal), name=f"attn_short T={T} d={d} B={B} H={H} causal={causal}", kind=KIND[dtype])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [32, 64])
@pytest.mark.parametrize("Tq,Tk", [(77, 40), (5, 128)])
def test_short_attention_full_rectangular(dev, Tq, Tk, d, dtype):
    B, H = 3, 12
    q = rand16((B, Tq, H * d), dtype, dev, 1)
    k, v = rand16((B, Tk, H * d), dtype, dev, 2), rand16((B, Tk, H * d), dtype, dev, 3)
    o = torch.full_like(q, float("nan"))
    run_attn(q, k, v, o, H, False)
    close(o, attn_ref(q, k, v, H, d ** -0.5, False), name=f"attn_short Tq={Tq} Tk={Tk} d={d}", kind=KIND[dtype])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("d,T", [(64, 77), (32, 17), (64, 128)])
def test_qkv_as_column_blocks_with_nan_gap_rows(dev, d, T, causal, dtype):
    """Q, K, V = the three column blocks of ONE [B][T + 3][3C] buffer whose 3 rows behind every batch's T are NaN: nothing past a batch's T
    rows may be read into the result."""
    B, H = 3, 2
    C = H * d
    buf = rand16((B, T + 3, 3 * C), dtype, dev, 7)
    buf[:, T:] = float("nan")
    q, k, v = buf[:, :T, :C], buf[:, :T, C:2 * C], buf[:, :T, 2 * C:]
    assert q.stride(0) == k.stride(0) == v.stride(0) == (T + 3) * 3 * C
    o = torch.full((B, T, C), float("nan"), dtype=dtype, device=dev)
    run_attn(q, k, v, o, H, causal)
    assert torch.isfinite(o).all()
    close(o, attn_ref(q, k, v, H, d ** -0.5, causal), name=f"attn_short fused-buffer T={T} d={d} causal={causal}", kind=KIND[dtype])


def bits(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [32, 64])
def test_causal_is_exact(dev, d, dtype):
    """No tolerance: row 0 sees key 0 only, so O[:, 0] is V[:, 0] bit for bit; and rows <= t do not depend on K / V rows > t at all."""
    B, H, T = 2, 3, 77
    C = H * d
    q, k, v = (rand16((B, T, C), dtype, dev, 40 + i) for i in range(3))
    o = torch.empty_like(q)
    run_attn(q, k, v, o, H, True)
    assert torch.equal(bits(o[:, 0]), bits(v[:, 0]))
    for t in (0, 15, 16, 40):
        k2, v2 = k.clone(), v.clone()
        k2[:, t + 1:] = rand16((B, T - t - 1, C), dtype, dev, 50 + t) * 3
        v2[:, t + 1:] = rand16((B, T - t - 1, C), dtype, dev, 60 + t) * 3
        o2 = torch.empty_like(q)
        run_attn(q, k2, v2, o2, H, True)
        assert torch.equal(bits(o2[:, :t + 1]), bits(o[:, :t + 1])), t
        assert not torch.equal(bits(o2[:, t + 1:]), bits(o[:, t + 1:])), t        # the overwritten keys are seen by the later rows


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,period,C", [(231, 77, 128), (10, 3, 24), (5, 5, 8), (300, 1, 40)])
def test_gather_with_added_row_vs_torch(dev, n, period, C, dtype):
    rows = 64
    T = rand16((rows, C), dtype, dev, 1)
    add = rand16((period, C), dtype, dev, 2)
    idx = torch.randint(-rows, rows, (n,), generator=torch.Generator().manual_seed(3)).to(dev)
    mask = (torch.arange(n) % 4 != 1).to(torch.uint8).to(dev)
    null = rand16((C,), dtype, dev, 4)
    y = torch.full((n, C), float("nan"), dtype=dtype, device=dev)
    O.run_ops([O.Gather(T, y, idx, mask=mask, null_row=null, add=add)])
    assert (L.lib().mdx_last_kernel() or b"").decode() == "gather_add_kernel"
    torch.cuda.synchronize()
    base = torch.where(mask.bool()[:, None], T[idx % rows].float(), null.float()[None])
    ref = (base + add.float()[torch.arange(n, device=dev) % period]).to(dtype)          # fp32 sum, one rounding
    assert torch.equal(bits(y), bits(ref))


class OldGatherDesc(ctypes.Structure):      # MdxGatherDesc as ABI 11 declared it
    _fields_ = [(n, ctypes.c_void_p) for n in "T Y idx mask null_row reserved_p".split()] + [(n, ctypes.c_int64) for n in "n C ldt ldy n_rows reserved0".split()]


@pytest.mark.parametrize("dtype", DTYPES)
def test_gather_without_add_is_the_old_gather(dev, dtype):
    n, C, rows = 50, 24, 16
    T = rand16((rows, C), dtype, dev, 1)
    idx = torch.randint(0, rows, (n,), generator=torch.Generator().manual_seed(3)).to(dev)
    y_new = torch.zeros(n, C, dtype=dtype, device=dev)
    y_old = torch.zeros_like(y_new)
    O.run_ops([O.Gather(T, y_new, idx)])
    assert (L.lib().mdx_last_kernel() or b"").decode() == "gather_kernel"
    d = OldGatherDesc(T=T.data_ptr(), Y=y_old.data_ptr(), idx=idx.data_ptr(), n=n, C=C, ldt=C, ldy=C, n_rows=rows)
    assert ctypes.sizeof(d) == ctypes.sizeof(L.MdxGatherDesc)
    fn = getattr(L.lib(), L.entry_name(L.OP_GATHER, L.DTYPE_F16 if dtype == torch.float16 else L.DTYPE_BF16))
    L.check(fn(ctypes.byref(d), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "old-layout gather")
    torch.cuda.synchronize()
    assert torch.equal(bits(y_new), bits(y_old)) and torch.equal(bits(y_new), bits(T[idx]))


# ---- the network ------------------------------------------------------------------------------------------------------------------------
def network_parity(name, cfg, sd32, ids, dtype, dev):
    """HIP vs the fp32 mirror on the SAME (16-bit-rounded) weights.  Yardstick: what the mirror itself loses when it stores 16-bit at the
    points the HIP program does; limit = 2 x that (the HIP path also rounds the fused q/k/v store and P before PV).
    Measured on MI355X, rel L2 HIP / yardstick: tiny golden bf16 5.66e-3 / 4.64e-3, fp16 6.71e-4 / 5.28e-4; SD-1.5 geometry (12 layers, seeded
    random weights, 2x q / k gain) bf16 8.78e-3 / 7.82e-3, fp16 1.10e-3 / 9.79e-4."""
    sd = {k: v.to(dtype).float() for k, v in sd32.items()}
    ref = R.clip_text_forward(cfg, sd, ids)
    yard = rel_l2(R.clip_text_forward(cfg, sd, ids, R.caster(dtype)), ref)
    model = CLIPTextModel(cfg, sd, dtype).to(dev)
    out = model(ids.to(dev))
    assert out[0] is out.last_hidden_state and out[0].dtype == dtype and out[0].shape == ref.shape and torch.isfinite(out[0]).all()
    err = rel_l2(out[0], ref)
    eager = CLIPTextModel(cfg, sd, dtype).to(dev)
    eager.use_graph = False
    assert torch.equal(bits(eager(ids.to(dev))[0]), bits(out[0])), "graph replay and eager run of the same program differ"
    assert torch.equal(bits(model(ids.to(dev))[0]), bits(out[0])), "second replay differs"
    parity_log("clip_text:" + name, kind=KIND[dtype], rel_l2=err, yardstick=yard, limit=2 * yard)
    print(f"[{name} {KIND[dtype]}] rel_l2 {err:.3e}  cast-mirror yardstick {yard:.3e}")
    check(f"{name} {KIND[dtype]}: HIP vs fp32 mirror", err, 2 * yard)


@pytest.mark.parametrize("dtype", DTYPES)
def test_tiny_golden_network(dev, dtype):
    g = torch.load(os.path.join(ROOT, "tests", "golden", "clip_text_tiny.pt"))
    network_parity("tiny golden", g["config"], {k: v.float() for k, v in g["state_dict"].items()}, g["input_ids"], dtype, dev)


@pytest.mark.parametrize("dtype", DTYPES)
def test_sd15_geometry_network(dev, dtype):
    """12 layers, 768 wide, 12 heads of 64, intermediate 3072, vocabulary 49408: SD-1.5's text tower with seeded random weights."""
    from magicdrive_amd.networks.clip_text import CLIP_SD15_CONFIG
    m = CLIPTextModel.from_config({}, seed=3)
    assert m.config.hidden_size == 768 and m.config.num_hidden_layers == 12
    ids = torch.randint(0, 49408, (2, 77), generator=torch.Generator().manual_seed(5))
    network_parity("sd15 geometry", dict(CLIP_SD15_CONFIG), m.state_dict(), ids, dtype, dev)


# ---- the pipeline -------------------------------------------------------------------------------------------------------------------------
class StubTokenizer:
    """Fixed ids per string: BOS, one id per character, EOS, EOS padding — the call signature of transformers' CLIPTokenizer."""
    model_max_length = 77

    def __call__(self, prompts, padding="max_length", max_length=77, truncation=True, return_tensors="pt"):
        ids = torch.full((len(prompts), max_length), 63, dtype=torch.int64)
        for i, s in enumerate(prompts):
            body = [ord(c) % 62 for c in s][:max_length - 2]
            ids[i, 0] = 62
            ids[i, 1:1 + len(body)] = torch.tensor(body, dtype=torch.int64)
        return SimpleNamespace(input_ids=ids)


def test_pipeline_prompt_path_runs_on_the_hip_text_encoder(dev):
    from helpers import scene
    from magicdrive_amd.networks import spec
    from magicdrive_amd.networks.unet_2d_condition_multiview import UNet2DConditionModelMultiview
    from magicdrive_amd.networks.unet_addon_rawbox import BEVControlNetModel
    from magicdrive_amd.pipeline.pipeline_bev_controlnet import StableDiffusionBEVControlNetPipeline
    cfg = spec.TINY_CONFIG
    tcfg = dict(vocab_size=64, hidden_size=cfg["cross_attention_dim"], intermediate_size=64, num_hidden_layers=1, num_attention_heads=2, max_position_embeddings=77)
    te = CLIPTextModel.from_config(tcfg, seed=9)
    pipe = StableDiffusionBEVControlNetPipeline(unet=UNet2DConditionModelMultiview.from_config(cfg, 0), controlnet=BEVControlNetModel.from_config(cfg, 1),
                                                text_encoder=te, tokenizer=StubTokenizer()).to(dev)
    assert te.device.type == "cuda"
    prompts = ["a driving scene in boston, rainy", "night, a bus ahead"]
    pe, ne = pipe._encode_prompt(prompts, dev, 1, True)
    tok = StubTokenizer()
    assert torch.equal(bits(pe), bits(te(tok(prompts).input_ids.to(dev))[0])) and torch.equal(bits(ne), bits(te(tok(["", ""]).input_ids.to(dev))[0]))
    assert pe.shape == (2, 77, cfg["cross_attention_dim"]) and not torch.equal(bits(pe[0]), bits(pe[1]))
    sc = scene(cfg, 2, 5)
    kw = dict(image=sc["bev_map"], camera_param=sc["camera_param"], height=224, width=400, num_inference_steps=2, guidance_scale=2.0, latents=sc["latents"],
              output_type="latent", bev_controlnet_kwargs={"bboxes_3d_data": sc["bboxes_3d_data"]})
    a = pipe(prompt=prompts, **kw).images
    b = pipe(prompt=None, prompt_embeds=pe, negative_prompt_embeds=ne, **kw).images
    torch.cuda.synchronize()
    assert a.shape == (2, 6, 4, 28, 50) and torch.isfinite(a).all()
    assert torch.equal(a, b)
