"""-m gpu: the model-input refresh store_xin (csrc/latent.h) through each of the four kernels that call it — ddim_kernel, unipc_kernel
(csrc/elementwise.hip), blend_kernel (csrc/blend.hip), renoise_kernel (csrc/noise.hip) — in both builds, both x_in layouts and both CFG
settings.  The refresh has ONE rule whatever op wrote x: after a launch every x_in pixel, in both CFG halves, holds x.to(x_in's type) of
the x read back, bit for bit; the pad channels of a padded pixel stride and the rows behind the last pixel are never written.

n = 257 pixels x 4 channels = 1028: one full 256-thread block plus a tail for the one-element-per-thread kernels, 257 groups of four
(a block and one thread) for the 16-byte instances of blend and renoise.  What each op computes is judged elsewhere
(tests/test_kernels_gpu.py, test_tails_gpu.py, test_latent_blend_gpu.py, test_latent_renoise_gpu.py); here x must only have changed.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from magicdrive_amd import _lib as L  # noqa: E402
from magicdrive_amd import ops as O  # noqa: E402

SENT = -12288.0            # exact in fp32, bf16 and fp16
PIX, C = 257, 4
N = PIX * C
ROWS = 6                   # coefficient rows
BUILDS = {"bf16": (L.DTYPE_BF16, torch.bfloat16), "f16": (L.DTYPE_F16, torch.float16)}
LAYOUTS = {"fp32": 0, "ld4": 4, "ld8": 8}
KERNEL = {"ddim": "ddim_kernel", "unipc": "unipc_kernel", "blend": "blend_kernel", "renoise": "renoise_kernel"}


def _record(op, x, x_in, cfg, xin_c, gen):
    rnd = lambda *s: torch.randn(*s, generator=gen, device="cuda")
    table = lambda ld: torch.rand(ROWS, ld, generator=gen, device="cuda") * 0.65 + 0.3        # every coefficient in [0.3, 0.95]
    step = lambda v: torch.full((1,), v, dtype=torch.int32, device="cuda")
    kw = dict(x_in=x_in, cfg=cfg, xin_c=xin_c)
    if op == "ddim":
        return O.DdimStep(x, rnd((2 if cfg else 1) * N), table(4), step(2), guidance=2.0, **kw)
    if op == "unipc":
        return O.UniPCStep(x, rnd((2 if cfg else 1) * N), table(12), step(2), rnd(N), rnd(N), rnd(N), guidance=2.0, **kw)
    if op == "blend":                      # mask of ones, counter inside [0, last_step): every element is written
        return O.LatentBlend(x, rnd(N), rnd(N), torch.ones(PIX, device="cuda"), table(4), step(2), last_step=5, **kw)
    seeds = torch.tensor([0x1234_5678_9ABC_DEF0], dtype=torch.int64, device="cuda")
    return O.LatentRenoise(x, table(4), step(3), step(0), seeds, jump=2, **kw)


@pytest.mark.parametrize("cfg", [0, 1])
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("op", list(KERNEL))
def test_x_in_holds_the_new_latents(op, build, layout, cfg):
    code_dtype, dtype16 = BUILDS[build]
    ld = LAYOUTS[layout]
    gen = torch.Generator(device="cuda").manual_seed(4100)
    x = torch.randn(N, generator=gen, device="cuda") * 2.0
    x0 = x.clone()
    halves = 2 if cfg else 1
    if ld:                                 # [halves * PIX (+ 2 rows behind), ld] in the build's 16-bit type
        buf = torch.full(((halves * PIX + 2) * ld,), SENT, dtype=dtype16, device="cuda")
        x_in = buf[:halves * PIX * ld].view(halves * PIX, ld)
    else:                                  # fp32 flat (+ 2 pixels behind)
        buf = torch.full((halves * N + 2 * C,), SENT, device="cuda")
        x_in = buf[:halves * N]
    rec = _record(op, x, x_in, bool(cfg), C if ld else 0, gen)
    code, d = rec.lower()
    assert (d.n, d.cfg, d.xin_c, d.xin_ld) == (N, cfg, C if ld else 0, ld)
    L.call_op(code, d, torch.cuda.current_stream().cuda_stream, code_dtype)
    torch.cuda.synchronize()
    assert (L.lib().mdx_last_kernel() or b"").decode() == KERNEL[op]
    assert bool(torch.isfinite(x).all()) and int((x != x0).sum()) > N // 2, "the op did not update x"
    bits = lambda t: t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)
    if ld:
        rows = buf.view(halves * PIX + 2, ld)
        want = bits(x.view(PIX, C).to(dtype16))
        for h in range(halves):
            assert torch.equal(bits(rows[h * PIX:(h + 1) * PIX, :C]), want), f"half {h}"
        assert bool((rows[:, C:] == SENT).all()) and bool((rows[halves * PIX:] == SENT).all()), "pad channels or the rows behind x_in were written"
    else:
        for h in range(halves):
            assert torch.equal(bits(buf[h * N:(h + 1) * N]), bits(x)), f"half {h}"
        assert bool((buf[halves * N:] == SENT).all()), "the elements behind x_in were written"
