"""-m gpu: a dirty call, then another call, on the same objects (tests/call_state.py).  Every comparison is torch.equal / array_equal.

The predecessor is a real call A that leaves the worst state a call can leave: NaN latents in every scene, boxes at the bucket's
capacity, every view given under fractional keep masks, its own seeds and eta, another text and other cameras.  Then call B — fewer boxes,
fewer given views, other masks, seeds and eta — must give the bits of B on freshly built objects.  Only floating-point state is ever
made bad, and only through the product API: NaN never becomes an address, and integer state ends where a finished call leaves it.

  plans      every plan of call_state.PLANS in both 16-bit types, 3 steps, the step program replayed as its captured graph: the latents,
             x_in, the health table, UniPC's history and the counters behind every step and jump.
  pipelines  (a) DDIM under box_bucket  (b) scene_boxes, two scenes  (c) UniPC with given views  (d) keep_masks + resample + eta + health
             (e) two chunks on two streams  (f) pictures through the tiny VAE with composite_images  (g) the HIP text encoder.
  seeded     with the UniPC history zeroing left out (floating-point state only), plan and pipeline (c) both differ: the instrument sees."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import call_state as CS  # noqa: E402
from helpers import given_view_inputs, scene, state_dicts  # noqa: E402
from magicdrive_amd import schedulers  # noqa: E402
from magicdrive_amd.engine import PackedNet  # noqa: E402
from magicdrive_amd.networks import spec  # noqa: E402

DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
STEPS = 3
NAN = float("nan")


# ---- SamplerPlan level ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nets(dev):
    cfg = spec.TINY_CONFIG
    usd, csd = state_dicts(cfg)
    packed = {}

    def get(dt):
        if dt not in packed:
            packed[dt] = (cfg, csd, PackedNet(usd, dev, DTYPES[dt]), PackedNet(csd, dev, DTYPES[dt]))
        return packed[dt]
    return get


def call_on(plan, four, which, variant):
    args, kw = CS.inputs(four, which, variant, steps=STEPS)
    plan.load_inputs(*args, **kw)
    return CS.run_on_device(plan, CS.actions(which, steps=STEPS))


def fresh_b(four, which, dev):
    plan = CS.build_plan(four, which, dev, steps=STEPS)
    want = call_on(plan, four, which, "B")
    plan.release()
    return want


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("which", list(CS.PLANS))
def test_plan_after_a_dirty_call_gives_the_bits_of_a_fresh_plan(dev, nets, which, dt):
    four = nets(dt)
    used = CS.build_plan(four, which, dev, steps=STEPS)
    left = call_on(used, four, which, "A")
    assert torch.isnan(left[-1]["latents"]).all(), "call A must leave NaN in every latent"
    if "m1" in left[-1]:
        assert torch.isnan(left[-1]["m1"]).all() and torch.isnan(left[-1]["x_last"]).all()
    got = call_on(used, four, which, "B")
    used.release()
    want = fresh_b(four, which, dev)
    assert torch.isfinite(want[-1]["latents"]).all()
    assert CS.differences(got, want) == [], f"{which} {dt}: call B on a used plan differs from call B on a fresh one"


def test_plan_without_the_history_reset_differs(dev, nets, monkeypatch):
    which, four = "unipc_given1", nets("bf16")
    used = CS.build_plan(four, which, dev, steps=STEPS)
    call_on(used, four, which, "A")
    with monkeypatch.context() as mp:
        for name in ("x_last", "m1", "m2"):
            mp.setattr(used, name, CS.NoReset(getattr(used, name)))
        got = call_on(used, four, which, "B")
    used.release()
    diff = CS.differences(got, fresh_b(four, which, dev))
    assert (0, "latents") in diff and (STEPS, "latents") in diff, diff


# ---- pipeline level ---------------------------------------------------------------------------------------------------------------------------
def make_pipe(dev, dt="bf16", given_view=False, unipc=False, vae=False, text=False):
    from magicdrive_amd.networks.unet_2d_condition_multiview import UNet2DConditionModelMultiview
    from magicdrive_amd.networks.unet_addon_rawbox import BEVControlNetModel
    from magicdrive_amd.pipeline.pipeline_bev_controlnet import StableDiffusionBEVControlNetPipeline
    from magicdrive_amd.pipeline.pipeline_bev_controlnet_given_view import StableDiffusionBEVControlNetGivenViewPipeline
    cfg = spec.TINY_CONFIG
    kw = {"torch_dtype": torch.float16} if dt == "f16" else {}
    parts = {}
    if vae:
        from magicdrive_amd.networks.autoencoder_kl import AutoencoderKL
        parts["vae"] = AutoencoderKL.from_config(spec.VAE_TINY_CONFIG, 5)
    if text:
        from magicdrive_amd.networks.clip_text import CLIPTextModel
        from test_clip_text_gpu import StubTokenizer
        tcfg = dict(vocab_size=64, hidden_size=cfg["cross_attention_dim"], intermediate_size=64, num_hidden_layers=1, num_attention_heads=2, max_position_embeddings=77)
        parts.update(text_encoder=CLIPTextModel.from_config(tcfg, seed=9), tokenizer=StubTokenizer())
    cls = StableDiffusionBEVControlNetGivenViewPipeline if given_view else StableDiffusionBEVControlNetPipeline
    pipe = cls(unet=UNet2DConditionModelMultiview.from_config(cfg, 0, **kw), controlnet=BEVControlNetModel.from_config(cfg, 1, **kw), **parts).to(dev)
    if unipc:
        pipe.scheduler = schedulers.UniPCMultistepScheduler.from_config(pipe.scheduler.config)
    return pipe


def scenes(variant, L, dt="bf16", n=2):
    """Call A: another seed (text, cameras, map, boxes), boxes padded to L, NaN latents in every scene.  Call B: the suite's usual scenes."""
    sc = scene(spec.TINY_CONFIG, n, L, seed=4321 if variant == "A" else 1234)
    if variant == "A":
        sc["latents"] = torch.full_like(sc["latents"], NAN)
    if dt == "f16":
        sc["prompt_embeds"], sc["negative_prompt_embeds"] = sc["prompt_embeds"].half(), sc["negative_prompt_embeds"].half()
    return sc


def given(variant):
    """(conditional latents, fractional keep masks): call A gives every view, call B the three views of helpers.given_view_inputs."""
    if variant == "A":
        g = torch.Generator().manual_seed(31)
        cl = [[torch.randn(4, 28, 50, generator=g) * 0.8 for _ in range(6)] for _ in range(2)]
    else:
        cl = given_view_inputs()
    gm = torch.tensor([[v is not None for v in r] for r in cl])
    m = CS._masks(gm, 7 if variant == "A" else 5)
    return cl, [[m[i, j] if gm[i, j] else None for j in range(6)] for i in range(2)]


def gens(base, n=2):
    return [torch.Generator().manual_seed(base + i) for i in range(n)]


def call(pipe, sc, output_type="latent", embeds=True, **kw):
    text = dict(prompt=None, prompt_embeds=sc["prompt_embeds"], negative_prompt_embeds=sc["negative_prompt_embeds"]) if embeds else {}
    out = pipe(image=sc["bev_map"], camera_param=sc["camera_param"], height=224, width=400, num_inference_steps=STEPS, guidance_scale=2.0,
               latents=sc["latents"], output_type=output_type, bev_controlnet_kwargs={"bboxes_3d_data": sc["bboxes_3d_data"]}, **text, **kw)
    torch.cuda.synchronize()
    return out


def same(got, want, what):
    """The returned latents or pictures, the matte and every health record, bit for bit."""
    eq = lambda a, b: torch.equal(a, b) if isinstance(a, torch.Tensor) else np.array_equal(np.asarray(a), np.asarray(b))
    assert eq(got.images, want.images), f"{what}: the result of call B on used objects differs from call B on fresh ones"
    finite = torch.isfinite(want.images).all() if isinstance(want.images, torch.Tensor) else np.isfinite(want.images).all()
    assert bool(finite), f"{what}: call B itself is not finite"
    assert (got.matte is None) == (want.matte is None) and (want.matte is None or np.array_equal(got.matte, want.matte)), f"{what}: matte"
    assert (got.health is None) == (want.health is None)
    if want.health is not None:
        assert all(want.health.ok), what
        for k in ("ok", "first_bad_step", "final", "trace", "image_nonfinite"):
            a, b = getattr(got.health, k), getattr(want.health, k)
            assert (a is None) == (b is None) and (b is None or np.array_equal(np.asarray(a), np.asarray(b))), f"{what}: health.{k}"


def dirty_then_b(make, setup, call_a, call_b, what, n_keys=1, sabotage=None):
    """A then B on one pipeline; B alone on a fresh one.  The plan cache must hold after B exactly the keys it held after A (n_keys of
    them): no plan was rebuilt behind the test's back, which would make the comparison trivial.  Returns (got, want)."""
    used = make(); setup(used)
    bad = call_a(used)
    if isinstance(bad.images, torch.Tensor):
        assert bool(torch.isnan(bad.images).flatten(1).any(1).all()), f"{what}: call A must leave NaN latents in every scene"
    keys = list(used._plans._d)
    assert n_keys is None or len(keys) == n_keys, keys
    if sabotage is not None:
        sabotage(used)
    got = call_b(used)
    assert list(used._plans._d) == keys, "call B must be served by the plans call A used"
    used._plans.clear()
    fresh = make(); setup(fresh)
    want = call_b(fresh)
    fresh._plans.clear()
    return got, want


@pytest.mark.parametrize("dt", list(DTYPES))
def test_a_ddim_under_box_bucket(dev, dt):
    def setup(p):
        p.box_bucket = 8
    got, want = dirty_then_b(lambda: make_pipe(dev, dt), setup, lambda p: call(p, scenes("A", 8, dt)), lambda p: call(p, scenes("B", 3, dt)), "(a)")
    same(got, want, f"(a) box_bucket {dt}")


@pytest.mark.parametrize("dt", list(DTYPES))
def test_b_scene_boxes_two_scenes(dev, dt):
    def setup(p):
        p.box_bucket, p.scene_boxes = 8, True
    got, want = dirty_then_b(lambda: make_pipe(dev, dt), setup, lambda p: call(p, scenes("A", 8, dt)), lambda p: call(p, scenes("B", 5, dt)), "(b)")
    same(got, want, f"(b) scene_boxes {dt}")


def unipc_given_views(dev, dt, sabotage=None):
    return dirty_then_b(lambda: make_pipe(dev, dt, given_view=True, unipc=True), lambda p: None,
                        lambda p: call(p, scenes("A", 5, dt), conditional_latents=given("A")[0]),
                        lambda p: call(p, scenes("B", 5, dt), conditional_latents=given("B")[0]), "(c)", sabotage=sabotage)


@pytest.mark.parametrize("dt", list(DTYPES))
def test_c_unipc_given_views(dev, dt):
    same(*unipc_given_views(dev, dt), f"(c) unipc given views {dt}")


def test_c_without_the_history_reset_differs(dev, monkeypatch):
    """The seeded carry-over: call A leaves NaN in x_last, m1 and m2 (floating-point state); with their zeroing left out of the plan's
    load_inputs, call B is no longer the fresh call."""
    def sabotage(pipe):
        plan, = pipe._plans._d.values()
        assert torch.isnan(plan.m1).all()
        for name in ("x_last", "m1", "m2"):
            monkeypatch.setattr(plan, name, CS.NoReset(getattr(plan, name)))
    got, want = unipc_given_views(dev, "bf16", sabotage)
    assert torch.isfinite(want.images).all() and not torch.equal(got.images, want.images)


@pytest.mark.parametrize("dt", list(DTYPES))
def test_d_keep_masks_resample_eta_and_health_at_once(dev, dt):
    def setup(p):
        p.health, p.resample = "trace", CS.RESAMPLE

    def run(variant, eta, seed):
        def go(p):
            cl, masks = given(variant)
            p.keep_masks = masks
            return call(p, scenes(variant, 5, dt), conditional_latents=cl, eta=eta, generator=gens(seed))
        return go
    got, want = dirty_then_b(lambda: make_pipe(dev, dt, given_view=True), setup, run("A", 1.0, 71), run("B", 0.5, 41), "(d)")
    same(got, want, f"(d) everything on {dt}")
    assert got.health.trace.shape == (STEPS, 2, 6, 4)


def test_e_two_chunks_on_two_streams(dev):
    def setup(p):
        p.streams, p.min_scenes_per_stream = 2, 1
    got, want = dirty_then_b(lambda: make_pipe(dev), setup, lambda p: call(p, scenes("A", 5)), lambda p: call(p, scenes("B", 5)), "(e)", n_keys=None)
    same(got, want, "(e) two chunks")


def test_f_pictures_through_the_vae_with_composite_images(dev):
    """The decode plan and the composite program are reused after a call whose latents were NaN."""
    g = torch.Generator().manual_seed(9)
    pics = {v: [[torch.randint(0, 256, (224, 400, 3), generator=g, dtype=torch.uint8) for _ in range(6)] for _ in range(2)] for v in "AB"}

    def run(variant):
        def go(p):
            cl, masks = given(variant)
            p.keep_masks, p.composite_feather = masks, 3
            p.composite_images = [[pics[variant][i][j] if cl[i][j] is not None else None for j in range(6)] for i in range(2)]
            return call(p, scenes(variant, 5), output_type="np", conditional_latents=cl)
        return go
    got, want = dirty_then_b(lambda: make_pipe(dev, given_view=True, vae=True), lambda p: None, run("A"), run("B"), "(f)")
    same(got, want, "(f) pictures")
    assert want.matte is not None and 0 < float(want.matte.mean()) < 1


def test_g_hip_text_encoder_with_another_prompt(dev):
    run = lambda prompts: (lambda p: call(p, scenes("A" if prompts[0].startswith("fog") else "B", 5), embeds=False, prompt=prompts))
    got, want = dirty_then_b(lambda: make_pipe(dev, text=True), lambda p: None, run(["fog, a truck crossing, night in singapore", "fog"]),
                             run(["a driving scene in boston, rainy", "night, a bus ahead"]), "(g)")
    same(got, want, "(g) text encoder")
