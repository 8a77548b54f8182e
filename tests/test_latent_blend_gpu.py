"""-m gpu: blend_kernel (csrc/blend.hip, mdx_latent_blend_*, ops.LatentBlend) against a float64 restatement, in both builds.

Behind the scheduler op of step s (the counter already reads s + 1), element i with m = mask[i // mask_elems] becomes
    m == 0: untouched,  m == 1: t = a cond + sg noise,  else: fma(m, t - x, x),     (a, sg) = coef[s, col_a], coef[s, col_s]
and every written element refreshes x_in.  Checked here, on 2 views of 3x5x4 (n = 120), 7x9x4 and 263 pixels x 4 (n = 1052: past one
workgroup of the 16-byte path, five of the scalar path with a ragged tail), x_in fp32 flat / 16-bit with pixel stride 8, cfg 0 / 1, the
DDIM and UniPC column sets, mask_elems 4 / 1, masks mixing exact 0, exact 1 and fractions:
  - m == 0 elements and their x_in copies keep their bits (x_in is pre-filled with a sentinel: nothing else is written, pad channels included);
  - m == 1 elements are bit-equal to what mdx_cfg_ddim_step / mdx_cfg_unipc_step write for a given view on the same operands;
  - fractional m within 4 * 2^-24 * (|a cond| + |sg noise| + |x|) of float64: three roundings in t (two products, one sum), one in
    t - x, one in the fma, each of relative error 2^-24 on a term bounded by that sum, m <= 1 — and a contraction either way stays inside
    (a derived bound; the test prints the worst error / bound ratio it meets: 0.36 on the MI355X);
  - x_in is the 16-bit rounding of the written fp32 value, bit for bit, in both CFG halves;
  - a step counter of 0 writes nothing, and so does last_step + 1;
  - operands offset by 4 bytes (the scalar path) give the bits of the aligned run;
  - every buffer ends where a NaN / sentinel guard begins: an over-read would reach the output, an over-write the guard;
  - a captured graph replayed over the steps walks the coefficient rows.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from magicdrive_amd import _lib as L  # noqa: E402
from magicdrive_amd import ops as O  # noqa: E402

U = 2.0 ** -24
NAN = float("nan")
SENT = -12288.0            # exact in fp32, bf16 and fp16
GUARD = 64
STEPS, LAST = 4, 3
SHAPES = {"2x3x5x4": (2 * 3 * 5, 4), "7x9x4": (7 * 9, 4), "263x4": (263, 4)}      # name -> (latent pixels, channels)
BUILDS = {"bf16": (L.DTYPE_BF16, torch.bfloat16), "f16": (L.DTYPE_F16, torch.float16)}
COLS = {"ddim": (4, 2, 3), "unipc": (12, 10, 11)}


def last_kernel():
    return (L.lib().mdx_last_kernel() or b"").decode()


def guarded(vals, off=0, fill=NAN):
    """A 1-D tensor as a view that ENDS where a guard of `fill` begins (and starts behind one): [64 | off | vals | 64].  off = 1 moves
    the start 4 bytes past a 16-byte boundary.  Returns (buffer, view)."""
    n = vals.numel()
    buf = torch.full((GUARD + off + n + GUARD,), fill, dtype=vals.dtype, device="cuda")
    view = buf[GUARD + off:GUARD + off + n]
    view.copy_(vals)
    return buf, view


def guards_intact(buf, view_start, n, fill):
    g = torch.cat([buf[:view_start], buf[view_start + n:]])
    return bool((g == fill).all()) if fill == fill else bool(torch.isnan(g).all())


def make_mask(entries, gen):
    """fp32 [entries]: exact 0, exact 1 and fractions, all three present."""
    kind = torch.randint(0, 3, (entries,), generator=gen, device="cuda")
    kind[:3] = torch.tensor([0, 1, 2], device="cuda")
    frac = torch.rand(entries, generator=gen, device="cuda") * 0.98 + 0.01
    return torch.where(kind == 0, torch.zeros_like(frac), torch.where(kind == 1, torch.ones_like(frac), frac))


class Case:
    """Operands of one launch, each in a guarded allocation."""

    def __init__(self, pixels, C, mask_elems, xin_ld, cfg, sched, dtype16, off=0, seed=0):
        gen = torch.Generator(device="cuda").manual_seed(1000 + seed)
        n = pixels * C
        self.n, self.C, self.cfg, self.xin_ld, self.mask_elems, self.sched, self.off = n, C, cfg, xin_ld, mask_elems, sched, off
        rnd = lambda k, s=1.0: torch.randn(k, generator=gen, device="cuda") * s
        self.x0 = rnd(n, 2.0)
        self.xb, self.x = guarded(self.x0, off)
        self.cb, self.cond = guarded(rnd(n, 0.8), off)
        self.nb, self.noise = guarded(rnd(n), off)
        self.mb, self.mask = guarded(make_mask(n // mask_elems, gen))
        ld = COLS[sched][0]
        self.coefb, coef = guarded(torch.rand(STEPS * ld, generator=gen, device="cuda") * 0.9 + 0.05)
        self.coef = coef.view(STEPS, ld)
        self.step = torch.zeros(1, dtype=torch.int32, device="cuda")
        c = 2 if cfg else 1
        if xin_ld:
            rows = c * pixels
            self.xinb = torch.full(((rows + 2) * xin_ld,), SENT, dtype=dtype16, device="cuda")
            self.x_in = self.xinb[:rows * xin_ld].view(rows, xin_ld)
        else:
            self.xinb, flat = guarded(torch.full((c * n,), SENT, device="cuda"), fill=SENT)
            self.x_in = flat
        self.m_el = self.mask.repeat_interleave(mask_elems)

    def op(self):
        return O.LatentBlend(self.x, self.cond, self.noise, self.mask, self.coef, self.step, last_step=LAST, x_in=self.x_in, cfg=bool(self.cfg), xin_c=self.C)

    def run(self, counter, build):
        self.step.fill_(counter)
        code, d = self.op().lower()
        L.call_op(code, d, torch.cuda.current_stream().cuda_stream, build)
        torch.cuda.synchronize()
        return last_kernel()

    def xin_halves(self):
        """x_in as [halves, n] values (the channels of x only) and the pad channels, if any."""
        c = 2 if self.cfg else 1
        if self.xin_ld:
            v = self.x_in.view(c, self.n // self.C, self.xin_ld)
            return v[..., :self.C].reshape(c, self.n), v[..., self.C:]
        return self.x_in.view(c, self.n), None

    def scheduler_given_view(self, s, build):
        """What mdx_cfg_ddim_step / mdx_cfg_unipc_step write at step s for a GIVEN view (gv_mode 1, mask of ones) on the same cond / noise
        / coefficient row: (x, x_in) of that launch."""
        gen = torch.Generator(device="cuda").manual_seed(5)
        n, c = self.n, (2 if self.cfg else 1)
        x = self.x0.clone()
        eps = torch.randn(c * n, generator=gen, device="cuda")
        step = torch.full((1,), s, dtype=torch.int32, device="cuda")
        x_in = torch.full_like(self.x_in, SENT).contiguous()
        gv = dict(gv_mask=torch.ones(1, dtype=torch.uint8, device="cuda"), gv_cond=self.cond.clone(), gv_noise=self.noise.clone(), gv_mode=1, gv_last_step=LAST)
        if self.sched == "ddim":
            op = O.DdimStep(x, eps, self.coef.clone(), step, x_in=x_in, cfg=bool(self.cfg), guidance=2.0, xin_c=self.C, **gv)
        else:
            z = lambda: torch.zeros(n, device="cuda")
            op = O.UniPCStep(x, eps, self.coef.clone(), step, z(), z(), z(), x_in=x_in, cfg=bool(self.cfg), guidance=2.0, xin_c=self.C, **gv)
        code, d = op.lower()
        L.call_op(code, d, torch.cuda.current_stream().cuda_stream, build)
        torch.cuda.synchronize()
        return x, x_in

    def assert_guards(self):
        o, n = self.off, self.n
        assert guards_intact(self.xb, GUARD + o, n, NAN), "x: a guard element was written"
        assert guards_intact(self.cb, GUARD + o, n, NAN) and guards_intact(self.nb, GUARD + o, n, NAN)
        if self.xin_ld:
            assert bool((self.xinb[self.x_in.numel():] == SENT).all()), "x_in: a row behind the last pixel was written"
        else:
            assert guards_intact(self.xinb, GUARD, self.x_in.numel(), SENT), "x_in: a guard element was written"


@pytest.mark.parametrize("sched", ["ddim", "unipc"])
@pytest.mark.parametrize("build", ["bf16", "f16"])
def test_blend_against_float64_and_the_schedulers(dev, build, sched):
    code, dtype16 = BUILDS[build]
    ld, ca, cs = COLS[sched]
    worst = 0.0
    seed = 0
    for sname, (pixels, C) in SHAPES.items():
        for mask_elems in (4, 1):
            for xin_ld in (0, 8):
                for cfg in (0, 1):
                    seed += 1
                    s = seed % LAST                                        # steps 0, 1, 2 in turn
                    K = Case(pixels, C, mask_elems, xin_ld, cfg, sched, dtype16, seed=seed)
                    name = f"{build} {sched} {sname} mask_elems={mask_elems} xin_ld={xin_ld} cfg={cfg} s={s}"
                    kern = K.run(s + 1, code)
                    assert kern == ("blend_kernel" if mask_elems == 4 else "blend_kernel_scalar"), (name, kern)
                    K.assert_guards()
                    x, m, x0 = K.x, K.m_el, K.x0
                    assert torch.isfinite(x).all(), name + ": a guard value reached x"
                    keep0, keep1, fr = m == 0, m == 1, (m != 0) & (m != 1)
                    assert keep0.any() and keep1.any() and fr.any()
                    # m == 0: x and x_in untouched
                    assert torch.equal(x[keep0], x0[keep0]), name
                    halves, pad = K.xin_halves()
                    assert bool((halves[:, keep0] == SENT).all()), name + ": x_in of an m == 0 element was written"
                    if pad is not None:
                        assert bool((pad == SENT).all()), name + ": a pad channel of x_in was written"
                    # m == 1: the scheduler kernels' own given-view bits
                    xs, xs_in = K.scheduler_given_view(s, code)
                    assert torch.equal(x[keep1], xs[keep1]), name + ": m == 1 differs from the scheduler's given-view path"
                    # fractions: float64 restatement
                    a, sg = K.coef[s, ca].double(), K.coef[s, cs].double()
                    ac, sn = a * K.cond.double(), sg * K.noise.double()
                    y64 = x0.double() + m.double() * (ac + sn - x0.double())
                    bound = 4 * U * (ac.abs() + sn.abs() + x0.double().abs())
                    err = (x.double() - y64).abs()
                    print(f"[{name}] max err / bound over fractional m: {(err[fr] / bound[fr]).max().item():.3f}")
                    worst = max(worst, (err[fr] / bound[fr]).max().item())
                    assert bool((err[fr] <= bound[fr]).all()), name
                    assert bool((err[keep1] <= bound[keep1]).all()), name
                    # x_in: the rounding of the written value, both halves
                    wr = ~keep0
                    want = x.to(K.x_in.dtype)
                    for hf in range(halves.shape[0]):
                        assert torch.equal(halves[hf][wr].view(torch.int16 if xin_ld else torch.int32), want[wr].view(torch.int16 if xin_ld else torch.int32)), f"{name}: x_in half {hf}"
                    if xin_ld:                                             # and the scheduler's own x_in at the m == 1 elements
                        sh = xs_in.view(halves.shape[0], K.n // C, xin_ld)[..., :C].reshape(halves.shape[0], K.n)
                        assert torch.equal(halves[:, keep1].view(torch.int16), sh[:, keep1].view(torch.int16)), name
    print(f"[{build} {sched}] worst err / bound = {worst:.3f}")


@pytest.mark.parametrize("build", ["bf16", "f16"])
def test_counter_outside_the_steps_writes_nothing(dev, build):
    code, dtype16 = BUILDS[build]
    for sched in COLS:
        for mask_elems, xin_ld in ((4, 8), (1, 0)):
            K = Case(263, 4, mask_elems, xin_ld, 1, sched, dtype16, seed=77)
            for counter in (0, LAST + 1, -5, STEPS + 3):
                K.run(counter, code)
                assert torch.equal(K.x, K.x0), (sched, counter)
                assert bool((K.xin_halves()[0] == SENT).all()), (sched, counter)
                K.assert_guards()
            K.run(LAST, code)                                              # the last step that blends: s = LAST - 1
            assert not torch.equal(K.x, K.x0)


@pytest.mark.parametrize("build", ["bf16", "f16"])
def test_operands_offset_by_4_bytes_give_the_same_bits(dev, build):
    code, dtype16 = BUILDS[build]
    for sched in COLS:
        for sname, (pixels, C) in SHAPES.items():
            for xin_ld, cfg in ((0, 0), (8, 1)):
                A = Case(pixels, C, 4, xin_ld, cfg, sched, dtype16, off=0, seed=9)
                B = Case(pixels, C, 4, xin_ld, cfg, sched, dtype16, off=1, seed=9)
                assert A.x.data_ptr() % 16 == 0 and B.x.data_ptr() % 16 == 4 and torch.equal(A.x0, B.x0) and torch.equal(A.mask, B.mask)
                ka, kb = A.run(2, code), B.run(2, code)
                assert (ka, kb) == ("blend_kernel", "blend_kernel_scalar")
                assert torch.equal(A.x.view(torch.int32), B.x.view(torch.int32)), (sched, sname)
                assert torch.equal(A.x_in.view(torch.int16 if xin_ld else torch.int32), B.x_in.view(torch.int16 if xin_ld else torch.int32))
                A.assert_guards(); B.assert_guards()
                assert not torch.equal(A.x, A.x0)


@pytest.mark.parametrize("sched", ["ddim", "unipc"])
@pytest.mark.parametrize("build", ["bf16", "f16"])
def test_captured_graph_walks_the_coefficient_rows(dev, build, sched):
    """[scheduler op, blend op] captured once and replayed STEPS times against the same two ops launched eagerly: same bits after every
    step; after steps 0 .. LAST - 1 the m == 1 elements hold coef[s] applied to (cond, noise) — two rounded products and their rounded
    sum, which is what torch's fp32 `a * cond + sg * noise` computes; after step LAST the output is the scheduler's."""
    _, dtype16 = BUILDS[build]
    ld, ca, cs = COLS[sched]
    pixels, C, n = 263, 4, 263 * 4
    gen = torch.Generator(device="cuda").manual_seed(3)
    cond, noise = torch.randn(n, generator=gen, device="cuda"), torch.randn(n, generator=gen, device="cuda")
    mask = make_mask(pixels, gen)
    coef = torch.rand(STEPS, ld, generator=gen, device="cuda") * 0.5 + 0.25
    eps = torch.randn(2 * n, generator=gen, device="cuda") * 0.1
    x_start = torch.randn(n, generator=gen, device="cuda")

    def state():
        st = dict(x=x_start.clone(), step=torch.zeros(1, dtype=torch.int32, device="cuda"), x_in=torch.full((2 * pixels, 8), SENT, dtype=dtype16, device="cuda"))
        if sched == "ddim":
            sch = O.DdimStep(st["x"], eps, coef, st["step"], x_in=st["x_in"], cfg=True, guidance=2.0, xin_c=C)
        else:
            z = lambda: torch.zeros(n, device="cuda")
            sch = O.UniPCStep(st["x"], eps, coef, st["step"], z(), z(), z(), x_in=st["x_in"], cfg=True, guidance=2.0, xin_c=C)
        st["ops"] = [sch, O.LatentBlend(st["x"], cond, noise, mask, coef, st["step"], last_step=LAST, x_in=st["x_in"], cfg=True, xin_c=C)]
        return st

    G, E = state(), state()
    prog = O.build_program(G["ops"])
    stream = torch.cuda.current_stream().cuda_stream
    m = mask.repeat_interleave(C)
    for s in range(STEPS):
        prog.launch(stream)
        O.run_ops([E["ops"][0]]); unblended = E["x"].clone(); O.run_ops([E["ops"][1]])
        torch.cuda.synchronize()
        assert int(G["step"].item()) == s + 1
        assert torch.equal(G["x"].view(torch.int32), E["x"].view(torch.int32)) and torch.equal(G["x_in"].view(torch.int16), E["x_in"].view(torch.int16)), s
        if s < LAST:
            t = coef[s, ca] * cond + coef[s, cs] * noise
            assert torch.equal(G["x"][m == 1], t[m == 1]), f"step {s}: row {s} of the table was not the one applied"
            assert torch.equal(G["x"][m == 0], unblended[m == 0])
            assert not torch.equal(G["x"], unblended)
        else:
            assert torch.equal(G["x"], unblended), "the last step's output must stay the scheduler's"
    prog.destroy()
