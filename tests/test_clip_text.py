"""CPU: the CLIP text encoder's reference (tests/clip_text_ref.py) against transformers, the loader of magicdrive_amd.networks.clip_text,
the quick_gelu fold, the op program's lowering, and the host-side contract of the ABI-12 descriptor fields (MdxAttnDesc.causal / v_rowmajor,
MdxGatherDesc.add / add_period)."""
import ctypes
import json
import os

import pytest
import torch

import clip_text_ref as R
from helpers import rel_l2
from magicdrive_amd import _lib as L
from magicdrive_amd import ops as O
from magicdrive_amd.networks.clip_text import CLIPTextModel, clip_text_param_shapes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "clip_text_tiny.pt")


@pytest.fixture(scope="module")
def golden():
    g = torch.load(GOLDEN)
    g["sd"] = {k: v.float() for k, v in g["state_dict"].items()}
    g["ref"] = R.clip_text_forward(g["config"], g["sd"], g["input_ids"])
    return g


def test_mirror_matches_the_recorded_transformers_output(golden):
    # same fp32 arithmetic up to summation order (K <= 128, 2 layers): a few fp32 ulps per element, measured 3.3e-7
    assert golden["ref"].shape == (3, 77, 128)
    assert rel_l2(golden["ref"], golden["last_hidden_state"]) < 2e-6


def test_mirror_matches_live_transformers(golden):
    transformers = pytest.importorskip("transformers")
    cfg = transformers.CLIPTextConfig(**golden["config"], bos_token_id=62, eos_token_id=63, pad_token_id=63)
    model = transformers.CLIPTextModel(cfg).eval().float()
    missing = model.load_state_dict(golden["sd"], strict=False)
    assert not [k for k in missing.missing_keys if not k.endswith("position_ids")] and not missing.unexpected_keys
    with torch.no_grad():
        out = model(input_ids=golden["input_ids"]).last_hidden_state
    assert rel_l2(golden["ref"], out) < 2e-6


def test_cast_mirror_is_a_yardstick_not_a_copy(golden):
    """The 16-bit mirrors differ from the fp32 one by the rounding noise of their type and by no more (bf16: 8 mantissa bits, fp16: 11)."""
    e_bf = rel_l2(R.clip_text_forward(golden["config"], golden["sd"], golden["input_ids"], R.caster(torch.bfloat16)), golden["ref"])
    e_h = rel_l2(R.clip_text_forward(golden["config"], golden["sd"], golden["input_ids"], R.caster(torch.float16)), golden["ref"])
    assert 2.0 ** -10 < e_bf < 2.0 ** -6 and 2.0 ** -13 < e_h < 2.0 ** -9 and e_h < e_bf / 4


def _save(tmp_path, cfg, sd, name="model.safetensors"):
    from safetensors.torch import save_file
    with open(tmp_path / "config.json", "w") as f:
        json.dump(cfg, f)
    if name.endswith(".safetensors"):
        save_file({k: v.contiguous() for k, v in sd.items()}, str(tmp_path / name))
    else:
        torch.save(sd, str(tmp_path / name))


@pytest.mark.parametrize("prefix,fname", [("", "model.safetensors"), ("text_model.", "model.safetensors"), ("text_model.", "pytorch_model.bin")])
def test_from_pretrained_reads_both_key_layouts(golden, tmp_path, prefix, fname):
    sd = {prefix + k: v for k, v in golden["sd"].items()}
    if prefix:
        sd[prefix + "embeddings.position_ids"] = torch.arange(77)[None]          # SD-1.5 checkpoints carry it
    _save(tmp_path, dict(golden["config"], architectures=["CLIPTextModel"]), sd, fname)
    m = CLIPTextModel.from_pretrained(str(tmp_path), torch_dtype=torch.float16)
    assert list(m.state_dict()) == list(clip_text_param_shapes(golden["config"]))
    assert all(torch.equal(m.state_dict()[k], golden["sd"][k]) for k in m.state_dict())
    assert m.dtype == torch.float16 and m.device.type == "cpu" and m.config.hidden_size == 128 and m.eval() is m
    assert sum(p.numel() for p in m.parameters()) == sum(v.numel() for v in golden["sd"].values())
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(golden["input_ids"])


def test_missing_tensor_and_wrong_shape_are_refused(golden):
    sd = dict(golden["sd"]); sd.pop("final_layer_norm.bias")
    with pytest.raises(KeyError):
        CLIPTextModel(golden["config"], sd)
    sd = dict(golden["sd"]); sd["final_layer_norm.bias"] = torch.zeros(64)
    with pytest.raises(ValueError):
        CLIPTextModel(golden["config"], sd)


def test_gelu_is_refused(golden, tmp_path):
    with pytest.raises(NotImplementedError, match="gelu"):
        CLIPTextModel.from_config(dict(golden["config"], hidden_act="gelu"))
    _save(tmp_path, dict(golden["config"], hidden_act="gelu"), golden["sd"])
    with pytest.raises(NotImplementedError, match="gelu"):
        CLIPTextModel.from_pretrained(str(tmp_path))


def test_quick_gelu_fold_is_exact_in_fp32(golden):
    """x sigmoid(1.702 x) == silu(1.702 x) / 1.702: with fc1 packed as 1.702 (W, b) under SiLU and fc2 as W / 1.702 the fp32 forward moves by
    fp32 rounding only (two extra roundings per fc1 / fc2 weight, ~6e-8 each)."""
    x = torch.linspace(-12, 12, 4001)
    a, b = R.quick_gelu(x), torch.nn.functional.silu(1.702 * x) / 1.702
    assert (a - b).abs().max() <= 4 * torch.finfo(torch.float32).eps * a.abs().max()
    sd = dict(golden["sd"])
    for i in range(golden["config"]["num_hidden_layers"]):
        p = f"encoder.layers.{i}.mlp."
        sd[p + "fc1.weight"] = sd[p + "fc1.weight"] * 1.702; sd[p + "fc1.bias"] = sd[p + "fc1.bias"] * 1.702
        sd[p + "fc2.weight"] = sd[p + "fc2.weight"] / 1.702
    orig = R.quick_gelu
    try:
        R.quick_gelu = torch.nn.functional.silu
        out = R.clip_text_forward(golden["config"], sd, golden["input_ids"])
    finally:
        R.quick_gelu = orig
    assert rel_l2(out, golden["ref"]) < 1e-6


def test_plan_lowers_to_the_expected_program(golden):
    """The op program of TextEncoderPlan, built on the CPU (descriptors only, nothing runs): gather(+add), 7 ops per layer, final LayerNorm;
    attention reads the three column blocks of the fused projection, causal, V row-major."""
    from magicdrive_amd.engine import PackedNet
    from magicdrive_amd.text_encoder import TextEncoderPlan
    cfg = golden["config"]
    plan = TextEncoderPlan(cfg, PackedNet(golden["sd"], torch.device("cpu"), torch.bfloat16), torch.device("cpu"), 3, 77)
    kinds = [type(op).__name__ for op in plan.ops]
    assert kinds == ["Gather"] + ["LayerNorm", "Gemm", "Attn", "Gemm", "LayerNorm", "Gemm", "Gemm"] * cfg["num_hidden_layers"] + ["LayerNorm"]
    low = [op.lower() for op in plan.ops]
    g = low[0][1]
    assert g.add and g.add_period == 77 and g.n == 3 * 77 and g.C == 128
    a = low[3][1]
    assert (a.causal, a.v_rowmajor, a.nsrc, a.joint, a.q_prescaled) == (1, 1, 1, 0, 0)
    assert (a.B, a.H, a.Tq, a.Tk, a.d) == (3, 2, 77, 77, 64) and a.ldq == a.ldk == a.ldv == 384 and a.sQ == a.sK == a.sV == 77 * 384
    assert a.K - a.Q == 256 and a.Vt - a.K == 256 and abs(a.scale - 0.125) < 1e-12
    fc1 = plan.ops[6]
    assert fc1.epilogue == L.EPI_SILU and torch.equal(fc1.W, (golden["sd"]["encoder.layers.0.mlp.fc1.weight"] * 1.702).to(torch.bfloat16))
    plan.compile()
    assert plan.program.n == len(plan.ops)


def test_ops_reject_causal_without_rowmajor_v():
    q = torch.zeros(1, 8, 64, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="causal"):
        O.Attn(q, q, torch.zeros(1, 64, 8, dtype=torch.bfloat16), torch.zeros_like(q), heads=1, Tk=8, scale=1.0, causal=True).lower()
    with pytest.raises(ValueError, match="add"):
        O.Gather(torch.zeros(4, 8, dtype=torch.bfloat16), torch.zeros(2, 8, dtype=torch.bfloat16), torch.zeros(2, dtype=torch.int64),
                 add=torch.zeros(2, 16, dtype=torch.bfloat16)[:, :8]).lower()


# ---- descriptor contract (as tests/test_contract.py: fake pointers, rejected on the host before any launch) ---------------------------------
EINVAL, EUNSUPPORTED = -1, -3
P = lambda k: 0x10000000 * k


def attn(**kw):
    d = dict(Q=P(1), K=P(2), Vt=P(3), O=P(4), B=1, H=1, Tq=8, Tk=8, d=64, nsrc=1, ldq=64, sQ=512, ldk=64, sK=512, ldv=64, sV=512, ldo=64, sO=512,
             scale=0.125, v_rowmajor=1)
    d.update(kw); return d


def gather(**kw):
    d = dict(T=P(1), Y=P(2), idx=P(3), n=2, C=8, ldt=8, ldy=8, n_rows=4, add=P(4), add_period=2)
    d.update(kw); return d


TABLE = [
    (L.OP_ATTN, "causal needs Tq == Tk", attn(causal=1, Tq=8, Tk=16), EINVAL, "Tq"),
    (L.OP_ATTN, "causal needs v_rowmajor == 1", attn(causal=1, v_rowmajor=0, Vt=P(3), d=8, ldq=8, ldk=8, ldv=8, ldo=8), EINVAL, "v_rowmajor"),
    (L.OP_ATTN, "causal must be 0 or 1", attn(causal=2), EINVAL, "causal=2"),
    (L.OP_ATTN, "v_rowmajor must be 0 or 1", attn(v_rowmajor=3), EINVAL, "v_rowmajor=3"),
    (L.OP_ATTN, "nsrc must be 1", attn(nsrc=2, kvmap=P(5)), EINVAL, "nsrc"),
    (L.OP_ATTN, "joint 0", attn(joint=1), EINVAL, "joint"),
    (L.OP_ATTN, "q_prescaled 0", attn(q_prescaled=1), EINVAL, "q_prescaled"),
    (L.OP_ATTN, "a larger Tq / Tk returns MDX_EUNSUPPORTED", attn(Tq=129, Tk=129, sQ=129 * 64, sK=129 * 64, sV=129 * 64, sO=129 * 64), EUNSUPPORTED, "Tq=129"),
    (L.OP_ATTN, "a larger Tq / Tk returns MDX_EUNSUPPORTED", attn(causal=1, Tq=129, Tk=129), EUNSUPPORTED, "Tk=129"),
    (L.OP_ATTN, "any other d returns MDX_EUNSUPPORTED", attn(d=40, ldq=40, ldk=40, ldv=40, ldo=40), EUNSUPPORTED, "d=40"),
    (L.OP_ATTN, "any other d returns MDX_EUNSUPPORTED", attn(d=128, ldq=128, ldk=128, ldv=128, ldo=128), EUNSUPPORTED, "d=128"),
    (L.OP_ATTN, "ldv >= H*d", attn(H=2, ldv=64), EINVAL, "ldv=64"),
    (L.OP_ATTN, "ldv multiple of 8", attn(ldv=68), EINVAL, "ldv=68"),
    (L.OP_ATTN, "Vt 16-byte aligned", attn(Vt=P(3) + 8), EINVAL, "Vt must be 16-byte"),
    (L.OP_ATTN, "null operand", attn(Vt=0), EINVAL, "null operand"),
    (L.OP_GATHER, "add 2-byte aligned", gather(add=P(4) + 1), EINVAL, "add must be 2-byte"),
    (L.OP_GATHER, "add_period positive", gather(add_period=0), EINVAL, "add_period=0"),
]


def _desc(opcode, fields):
    d = L.DESC_OF_OP[opcode]()
    names = {f[0] for f in d._fields_}
    for k, v in fields.items():
        assert k in names, (opcode, k)
        setattr(d, k, v)
    return d


@pytest.mark.skipif(torch.cuda.is_available(), reason="fake device pointers: the rejection table must not run where a launch could succeed")
@pytest.mark.parametrize("path", ["bf16", "f16", "program"])
@pytest.mark.parametrize("opcode,clause,fields,code,names", TABLE, ids=[f"{i}-{n}" for i, (_, _, _, _, n) in enumerate(TABLE)])
def test_new_fields_are_checked_on_the_host(opcode, clause, fields, code, names, path):
    lib = L.lib()
    d = _desc(opcode, fields)
    if path == "program":
        prog = L.Program([(opcode, d, L.DTYPE_BF16)])
        rc = lib.mdx_program_run(ctypes.byref(prog.buf), 1, None)
    else:
        rc = getattr(lib, L.entry_name(opcode, L.DTYPE_F16 if path == "f16" else L.DTYPE_BF16))(ctypes.byref(d), None)
    msg = (lib.mdx_last_error() or b"").decode()
    assert rc == code, f"[{clause}] via {path}: rc={rc} (want {code}): {msg!r}"
    assert names in msg, f"[{clause}] via {path}: {msg!r} does not name {names!r}"


def test_header_documents_the_new_fields():
    hdr = open(os.path.join(ROOT, "include", "mdx.h")).read()
    assert "#define MDX_ABI_VERSION 12" in hdr and L.ABI_VERSION == 12
    for word in ("int64_t causal;", "int64_t v_rowmajor;", "const void* add;", "add_period;", "attention_short.hip"):
        assert word in hdr, word
    assert [f[0] for f in L.MdxAttnDesc._fields_][-2:] == ["causal", "v_rowmajor"]
    assert ctypes.sizeof(L.MdxGatherDesc) == 12 * 8            # the renamed fields did not move anything
