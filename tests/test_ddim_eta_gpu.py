"""-m gpu: ddim_eta_kernel (csrc/noise.hip, mdx_cfg_ddim_eta_step_*, ops.DdimEtaStep) — stochastic DDIM, eta > 0 — and the path from it up
to pipe(..., eta=), both builds.

With s = *step_ptr, v = *draw_ptr, c = coef[s], (dir, std) = var[s]:
    e = eps_u + g (eps_c - eps_u) | eps;  x0 = (x - c1 e) / c0;  det = c2 x0 + dir e;  x <- std != 0 ? det + (std z) : det
(a given element under gv_mode 2: e = gv_noise, dir = c3, std = 0; under gv_mode 1 and s < last: x <- c2 cond + c3 noise); z = noise[i], or
Philox4x32-10 + Box-Muller of (seeds[g], v, e) with counter word 3 = 1; then step <- s + 1, draw <- v + 1.

  1. given noise      against the float64 evaluation of the contract.  The bound counts the fp32 roundings of the kernel's expression
                      tree, each u = 2^-24 of the magnitude it rounds (IEEE add, multiply, fma and the correctly rounded division):
                        e    : 3 under CFG (the difference, the product, the sum)      de   = u (2 g |ec - eu| + |e|)        (0 without)
                        num  : 2 (c1 e, the difference)                                dnum = u (|c1 e| + |num|) + c1 de
                        x0   : 1                                                       dx0  = u |x0| + dnum / c0
                        det  : 3 (two products, the sum)                               ddet = u (|c2 x0| + |dir e| + |det|) + c2 dx0 + dir de
                        xn   : 2 (std z, the sum)                                      dxn  = u (|std z| + |xn|) + ddet
                      a contracted multiply-add only removes a rounding.  A gv_mode 1 element is two products and a sum:
                      u (|c2 cond| + |c3 noise| + |x|).  The test allows 2x this bound and prints the worst error / bound.
                      4, 5, 7, 1027 groups of 1, 4, 20 elements and one group of 4, 5, 7, 1027; x aligned and 4 bytes off; CFG on and
                      off, both x_in layouts and none, given-view modes 0, 1, 2, both builds; pad channels and guards untouched.
  2. generated noise  crafted rows c = (1, 0, 0, .), dir = 0, std = 1: x becomes z.  |x - z64| <= 1e-5 (the bound
                      tests/test_latent_renoise_gpu.py derives for this evaluation); the aligned and the scalar instance give equal bits.
  3. std == 0 row     with dir = c3: the bits of ops.DdimStep on the same operands, x and x_in.
  4. counters         step and draw advance by one per launch; the SAME captured graph replayed gives the noise of draw + 1; each
                      out-of-range step fills x with NaN and leaves x_in and both counters alone.
  5. independence     permuting groups with their seeds permutes the result bit for bit; with equal seed and draw = visit the stream
                      shares no 4-word block with renoise's over 2^16 elements; mean and variance of 2^20 values within 5 standard errors.
  6. scheduler        DDIMScheduler.step(..., eta, variance_noise=) against the reference scheduler's recorded outputs.
  7. pipeline         TINY_CONFIG with conv_out zeroed: eps is exactly 0 and every step is x <- (c2 / c0) x + std z, so the final latents
                      have a closed form in float64 from the call's initial latents, the plan's seeds and draw = 0 .. n - 1.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import given_view_inputs, scene  # noqa: E402
from magicdrive_amd import _lib as L  # noqa: E402
from magicdrive_amd import ops as O  # noqa: E402
from magicdrive_amd import schedulers  # noqa: E402
from magicdrive_amd.networks import spec  # noqa: E402
from philox_ref import eta_noise_ref, eta_noise_words, noise_ref, noise_words, shared_blocks  # noqa: E402
from test_ddim_eta_contract import ULP, _golden, table_bounds  # noqa: E402

U = 2.0 ** -24
NAN = float("nan")
SENT = -12288.0            # exact in fp32, bf16 and fp16
GUARD = 64
ROWS = 6
SEED_FILL = 0x5A5A5A5A5A5A5A5A
BUILDS = {"bf16": (L.DTYPE_BF16, torch.bfloat16), "f16": (L.DTYPE_F16, torch.float16)}
NOISE_LIMIT = 1e-5
SHAPES = [(m, g) for g in ("1", "4", "20", "whole") for m in (4, 5, 7, 1024 + 3)]


def last_kernel():
    return (L.lib().mdx_last_kernel() or b"").decode()


def guarded(vals, off=0, fill=NAN):
    """A 1-D tensor as a view that ENDS where a guard of `fill` begins (and starts behind one): [64 | off | vals | 64]; off = 1 moves the
    start 4 bytes past a 16-byte boundary.  Returns (buffer, view)."""
    n = vals.numel()
    buf = torch.full((GUARD + off + n + GUARD,), fill, dtype=vals.dtype, device="cuda")
    view = buf[GUARD + off:GUARD + off + n]
    view.copy_(vals)
    return buf, view


def guards_intact(buf, start, n, fill):
    g = torch.cat([buf[:start], buf[start + n:]])
    return bool((g == fill).all()) if fill == fill else bool(torch.isnan(g).all())


def seeds_for(groups, salt=0):
    g = torch.Generator().manual_seed(99 + salt)
    return torch.empty(groups, dtype=torch.int64).random_(generator=g) * torch.where(torch.arange(groups) % 2 == 0, 1, -1)   # both signs: all 64 bits


def z64(seeds, draw, group_elems):
    return np.concatenate([eta_noise_ref(int(s), draw, group_elems) for s in seeds.tolist()])


def geometry(m, group):
    return (m, m) if group == "whole" else (m * int(group), int(group))


class Case:
    """Operands of one launch, each in a guarded allocation.  The tables are random (their rows need not be a schedule): every coefficient
    in [0.3, 0.95], dir in [0.2, 0.9], std in [0.1, 0.8], so every term of the update matters.  crafted: c = (1, 0, 0, .), dir 0, std 1."""

    def __init__(self, n, ge, xin="none", cfg=0, dtype16=torch.bfloat16, off=0, C=1, xin_ld=0, seed=0, gv_mode=0, view=None, noise=False, crafted=False,
                 guidance=2.5):
        gen = torch.Generator(device="cuda").manual_seed(3000 + seed)
        rnd = lambda k, s=1.0: torch.randn(k, generator=gen, device="cuda") * s
        self.n, self.ge, self.cfg, self.off, self.C, self.xin_ld, self.g = n, ge, cfg, off, C, xin_ld, guidance
        self.x0 = rnd(n, 2.0)
        self.xb, self.x = guarded(self.x0, off)
        self.epsb, self.eps = guarded(rnd((2 if cfg else 1) * n))
        self.coefb, coef = guarded(torch.rand(ROWS * 4, generator=gen, device="cuda") * 0.65 + 0.3)
        self.coef = coef.view(ROWS, 4)
        self.varb, var = guarded(torch.rand(ROWS * 2, generator=gen, device="cuda"))
        self.var = var.view(ROWS, 2)
        self.var[:, 0] = 0.2 + 0.7 * self.var[:, 0]
        self.var[:, 1] = 0.1 + 0.7 * self.var[:, 1]
        if crafted:
            self.coef[:, 0], self.coef[:, 1], self.coef[:, 2] = 1.0, 0.0, 0.0
            self.var[:, 0], self.var[:, 1] = 0.0, 1.0
        self.step = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.draw = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.seeds_host = seeds_for(n // ge, seed)
        self.sb, self.seeds = guarded(self.seeds_host.cuda(), fill=SEED_FILL)
        self.noise = self.nb = None
        if noise:
            self.nb, self.noise = guarded(rnd(n))
        self.gv_mode, self.view = gv_mode, view or ge
        self.mask = self.gcond = self.gnoise = None
        if gv_mode:
            self.mb, self.mask = guarded((torch.arange(n // self.view, device="cuda") % 3 != 1).to(torch.uint8), fill=7)
            self.gcb, self.gcond = guarded(rnd(n, 0.8))
            self.gnb, self.gnoise = guarded(rnd(n))
        c = 2 if cfg else 1
        self.x_in, self.xinb = None, None
        if xin == "h16":
            rows = c * (n // C)
            self.xinb = torch.full(((rows + 2) * xin_ld,), SENT, dtype=dtype16, device="cuda")
            self.x_in = self.xinb[:rows * xin_ld].view(rows, xin_ld)
        elif xin == "f32":
            self.xinb, self.x_in = guarded(torch.full((c * n,), SENT, device="cuda"), fill=SENT)

    def gv(self):
        return {} if not self.gv_mode else dict(gv_mask=self.mask, gv_cond=self.gcond, gv_noise=self.gnoise, gv_mode=self.gv_mode, gv_last_step=ROWS - 1)

    def op(self):
        return O.DdimEtaStep(self.x, self.eps, self.coef, self.var, self.step, self.draw, seeds=self.seeds, noise=self.noise, x_in=self.x_in,
                             cfg=bool(self.cfg), guidance=self.g, xin_c=self.C if self.xin_ld else 0, **self.gv())

    def plain_op(self, x, x_in, step):
        return O.DdimStep(x, self.eps, self.coef, step, x_in=x_in, cfg=bool(self.cfg), guidance=self.g, xin_c=self.C if self.xin_ld else 0, **self.gv())

    def run(self, s, v, build=L.DTYPE_BF16):
        self.step.fill_(s); self.draw.fill_(v)
        code, d = self.op().lower()
        L.call_op(code, d, torch.cuda.current_stream().cuda_stream, build)
        torch.cuda.synchronize()
        return last_kernel()

    def reference(self, s, z):
        """(float64 result of the contract, the derived bound) for row s and noise z (float64 [n])."""
        f = lambda t: t.cpu().numpy().astype(np.float64)
        n, g = self.n, float(np.float32(self.g))
        c0, c1, c2, c3 = f(self.coef)[s]
        d, sd = f(self.var)[s]
        x, eps = f(self.x0), f(self.eps)
        if self.cfg:
            eu, ec = eps[:n], eps[n:]
            e = eu + g * (ec - eu)
            de = U * (2 * g * np.abs(ec - eu) + np.abs(e))
        else:
            e, de = eps, np.zeros(n)
        dirs, sds = np.full(n, d), np.full(n, sd)
        given = np.zeros(n, bool)
        if self.gv_mode:
            given = np.repeat(self.mask.cpu().numpy() != 0, self.view)
        if self.gv_mode == 2:
            e, de = np.where(given, f(self.gnoise), e), np.where(given, 0.0, de)
            dirs, sds = np.where(given, c3, dirs), np.where(given, 0.0, sds)
        num = x - c1 * e
        dnum = U * (np.abs(c1 * e) + np.abs(num)) + c1 * de
        x0 = num / c0
        dx0 = U * np.abs(x0) + dnum / c0
        det = c2 * x0 + dirs * e
        ddet = U * (np.abs(c2 * x0) + np.abs(dirs * e) + np.abs(det)) + c2 * dx0 + dirs * de
        xn = det + sds * z
        dxn = U * (np.abs(sds * z) + np.abs(xn)) + ddet
        if self.gv_mode == 1 and s < ROWS - 1:
            t = c2 * f(self.gcond) + c3 * f(self.gnoise)
            xn = np.where(given, t, xn)
            dxn = np.where(given, U * (np.abs(c2 * f(self.gcond)) + np.abs(c3 * f(self.gnoise)) + np.abs(t)), dxn)
        return xn, dxn

    def assert_guards(self):
        assert guards_intact(self.xb, GUARD + self.off, self.n, NAN), "x: a guard element was written"
        assert guards_intact(self.sb, GUARD, self.seeds.numel(), SEED_FILL) and guards_intact(self.coefb, GUARD, ROWS * 4, NAN)
        assert guards_intact(self.varb, GUARD, ROWS * 2, NAN) and guards_intact(self.epsb, GUARD, self.eps.numel(), NAN)
        if self.noise is not None:
            assert guards_intact(self.nb, GUARD, self.n, NAN)
        if self.gv_mode:
            assert guards_intact(self.mb, GUARD, self.mask.numel(), 7) and guards_intact(self.gcb, GUARD, self.n, NAN) and guards_intact(self.gnb, GUARD, self.n, NAN)
        if self.x_in is not None and self.xin_ld:
            assert bool((self.xinb[self.x_in.numel():] == SENT).all()), "x_in: a row behind the last pixel was written"
        elif self.x_in is not None:
            assert guards_intact(self.xinb, GUARD, self.x_in.numel(), SENT), "x_in: a guard element was written"

    def assert_xin(self, dt16):
        if self.x_in is None:
            return
        halves = 2 if self.cfg else 1
        if self.xin_ld:
            xi = self.x_in.view(halves, self.n // self.C, self.xin_ld)
            assert bool((xi[..., self.C:] == SENT).all()), "pad channels were written"
            for hf in range(halves):
                assert torch.equal(xi[hf, :, :self.C].reshape(-1), self.x.to(dt16)), f"x_in half {hf} is not the 16-bit rounding of x"
        else:
            for hf in range(halves):
                assert torch.equal(self.x_in.view(halves, self.n)[hf], self.x)


COMBOS = [(cfg, xin, build) for cfg in (0, 1) for xin in ("none", "f32", "h16") for build in ("bf16", "f16")]


@pytest.mark.parametrize("gv_mode", [0, 1, 2])
@pytest.mark.parametrize("m,group", SHAPES, ids=[f"{m}x{g}" for m, g in SHAPES])
def test_given_noise_against_float64(dev, m, group, gv_mode):
    """Every (CFG, x_in layout, build) combination at this shape, x aligned and 4 bytes off.  Under a given-view mode the mask has one byte
    per group (per element when there is one group), so given and free elements sit side by side."""
    n, ge = geometry(m, group)
    C = 4 if n % 4 == 0 else 1
    worst = 0.0
    for k, (cfg, xin, build) in enumerate(COMBOS):
        code, dt16 = BUILDS[build]
        for off in (0, 1):
            cs = Case(n, ge, xin=xin, cfg=cfg, dtype16=dt16, off=off, C=C, xin_ld=8 if xin == "h16" else 0, seed=k + 13 * off, gv_mode=gv_mode,
                      view=1 if group == "whole" else ge, noise=True)
            s = (k + off) % ROWS                              # every row, the last one included (gv_mode 1 keeps its output)
            kern = cs.run(s, 3, code)
            assert kern == ("ddim_eta_kernel" if off == 0 and ge % 4 == 0 else "ddim_eta_kernel_scalar"), kern
            ref, bound = cs.reference(s, cs.noise.cpu().numpy().astype(np.float64))
            got = cs.x.cpu().numpy().astype(np.float64)
            assert np.isfinite(got).all()
            ratio = float((np.abs(got - ref) / bound).max())
            worst = max(worst, ratio)
            assert ratio <= 2.0, f"n={n} group_elems={ge} gv={gv_mode} cfg={cfg} {xin} {build} off={off} row {s}: error / derived bound = {ratio:.3f} > 2"
            if gv_mode == 2:                                  # a given element: c3 and no noise, exactly the deterministic update
                given = np.repeat(cs.mask.cpu().numpy() != 0, cs.view)
                quiet, _ = Case.reference(cs, s, np.zeros(n))
                assert given.any() and np.abs(got - quiet)[given].max() <= 2.0 * bound[given].max()
            assert int(cs.step) == s + 1 and int(cs.draw) == 4
            cs.assert_guards()
            cs.assert_xin(dt16)
    print(f"[ddim_eta given noise n={n} group_elems={ge} gv_mode={gv_mode}] worst error / derived bound = {worst:.3f} (allowed 2)")


@pytest.mark.parametrize("m,group", SHAPES, ids=[f"{m}x{g}" for m, g in SHAPES])
def test_generated_noise_is_the_documented_mapping(dev, m, group):
    n, ge = geometry(m, group)
    worst, outs = 0.0, []
    for off in (0, 1):
        cs = Case(n, ge, off=off, seed=n % 13, crafted=True, cfg=off)
        k = cs.run(2, 5)
        assert k == ("ddim_eta_kernel" if off == 0 and ge % 4 == 0 else "ddim_eta_kernel_scalar"), k
        got = cs.x.cpu().numpy().astype(np.float64)
        want = z64(cs.seeds_host, 5, ge)
        err = float(np.abs(got - want).max())
        worst = max(worst, err)
        assert np.isfinite(got).all() and err <= NOISE_LIMIT, f"n={n} group_elems={ge} off={off}: |x - z| max {err:.3e} > {NOISE_LIMIT}"
        assert np.abs(got - np.concatenate([noise_ref(int(s), 5, ge) for s in cs.seeds_host.tolist()])).max() > 0.1, "this is renoise's stream"
        cs.assert_guards()
        assert int(cs.step) == 3 and int(cs.draw) == 6
        outs.append(cs.x.clone())
    print(f"[ddim_eta noise n={n} group_elems={ge}] max |z_gpu - z_fp64| = {worst:.3e} (limit {NOISE_LIMIT})")
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), "the scalar instance must give the 16-byte instance's bits"


@pytest.mark.parametrize("build", ["bf16", "f16"])
@pytest.mark.parametrize("gv_mode", [0, 1, 2])
@pytest.mark.parametrize("m,group,off", [(7, "20", 0), (7, "20", 1), (1027, "whole", 0), (1027, "4", 0), (5, "1", 1)])
def test_zero_std_row_is_the_deterministic_step(dev, m, group, off, gv_mode, build):
    """var row = (c3, 0): no noise is made, and x, x_in carry ops.DdimStep's bits on the same operands."""
    code, dt16 = BUILDS[build]
    n, ge = geometry(m, group)
    C = 4 if n % 4 == 0 else 1
    for cfg, xin in ((1, "h16"), (0, "f32"), (1, "none")):
        cs = Case(n, ge, xin=xin, cfg=cfg, dtype16=dt16, off=off, C=C, xin_ld=8 if xin == "h16" else 0, seed=m + gv_mode, gv_mode=gv_mode,
                  view=1 if group == "whole" else ge)
        s = 2 + cfg
        cs.var[:, 0], cs.var[:, 1] = cs.coef[:, 3], 0.0
        xb2, x2 = guarded(cs.x0, off)
        xin2 = None if cs.x_in is None else torch.full_like(cs.x_in, SENT)
        step2 = torch.full((1,), s, dtype=torch.int32, device="cuda")
        c2, d2 = cs.plain_op(x2, xin2, step2).lower()
        L.call_op(c2, d2, torch.cuda.current_stream().cuda_stream, code)
        cs.run(s, 9, code)
        assert torch.equal(cs.x.view(torch.int32), x2.view(torch.int32)), f"gv={gv_mode} cfg={cfg} {xin}: std == 0 with dir = c3 differs from ddim_kernel"
        if xin2 is not None:
            assert torch.equal(cs.x_in.view(torch.int16) if xin == "h16" else cs.x_in.view(torch.int32), xin2.view(torch.int16) if xin == "h16" else xin2.view(torch.int32))
        assert int(cs.step) == int(step2) == s + 1 and int(cs.draw) == 10
        cs.assert_guards()


@pytest.mark.parametrize("build", ["bf16", "f16"])
def test_counters_and_graph_replay(dev, build):
    code, dt16 = BUILDS[build]
    n, ge = 2 * 7 * 9 * 4, 7 * 9 * 4
    cs = Case(n, ge, xin="h16", cfg=1, dtype16=dt16, C=4, xin_ld=8, seed=9, crafted=True)
    lowered = cs.op().lower()
    prog = L.Program([(lowered[0], lowered[1], code)])
    st = torch.cuda.current_stream().cuda_stream
    cs.step.fill_(2); cs.draw.fill_(4)
    seen = []
    for k in range(3):                               # the same captured graph: the counters it reads are the ones it wrote
        prog.launch(st)
        torch.cuda.synchronize()
        assert int(cs.step) == 3 + k and int(cs.draw) == 5 + k
        got = cs.x.cpu().numpy().astype(np.float64)
        assert np.abs(got - z64(cs.seeds_host, 4 + k, ge)).max() <= NOISE_LIMIT, f"replay {k}: not the noise of draw {4 + k}"
        seen.append(cs.x.clone())
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])
    prog.destroy()
    cs.assert_guards()
    cs.assert_xin(dt16)
    # out of range, discovered on the device: NaN in x, x_in and both counters untouched
    for s, why in ((-1, "step < 0"), (-7, "step < 0"), (ROWS, "step >= n_rows"), (ROWS + 5, "step >= n_rows")):
        for noise in (False, True):
            cs = Case(n, ge, xin="h16", cfg=1, dtype16=dt16, C=4, xin_ld=8, seed=9, noise=noise, off=int(noise))
            cs.run(s, 11, code)
            assert bool(torch.isnan(cs.x).all()), why
            assert int(cs.step) == s and int(cs.draw) == 11, f"{why}: a counter moved"
            assert bool((cs.xinb == SENT).all()), f"{why}: x_in was written"
            cs.assert_guards()
    # the first and the last row are in range
    for s in (0, ROWS - 1):
        cs = Case(n, ge, seed=9)
        cs.run(s, 0)
        assert bool(torch.isfinite(cs.x).all()) and int(cs.step) == s + 1 and int(cs.draw) == 1


def test_groups_are_independent_of_position_and_size(dev):
    ge, groups = 20, 8
    n = ge * groups
    cs = Case(n, ge, seed=4, cfg=1)
    cs.run(4, 1)
    base = cs.x.view(groups, ge).clone()
    perm = torch.tensor([5, 2, 7, 0, 3, 6, 1, 4]).cuda()
    cp = Case(n, ge, seed=4, cfg=1)
    cp.x.copy_(cs.x0.view(groups, ge)[perm].reshape(-1))
    cp.eps.copy_(cs.eps.view(2, groups, ge)[:, perm].reshape(-1))
    cp.seeds.copy_(cs.seeds[perm])
    cp.run(4, 1)
    assert torch.equal(cp.x.view(groups, ge).view(torch.int32), base[perm].view(torch.int32)), "permuting groups with their seeds must permute the result"
    for g in (0, 5):                                  # a group alone (another launch geometry, scalar or 16-byte instance) has its bits in the batch
        one = Case(ge, ge, seed=4, cfg=1, off=1 if g == 5 else 0)
        one.x.copy_(cs.x0.view(groups, ge)[g]); one.eps.copy_(cs.eps.view(2, groups, ge)[:, g].reshape(-1)); one.seeds.copy_(cs.seeds[g:g + 1])
        one.coef.copy_(cs.coef); one.var.copy_(cs.var)
        one.run(4, 1)
        assert torch.equal(one.x.view(torch.int32), base[g].view(torch.int32)), f"group {g} alone differs from itself in the batch"


def test_step_noise_shares_no_block_with_jump_noise(dev):
    """Equal seed, draw = visit, 2^16 elements: the 4-value blocks of the step's stream and of renoise's are all different (compared as
    the fp32 bits of z, and the reference's words likewise); so are two draws."""
    from test_latent_renoise_gpu import Case as JumpCase
    n = 1 << 16
    outs = {}
    for name, seed, v in (("a", 1, 0), ("draw", 1, 1), ("b", -77, 3)):
        cs = Case(n, n, crafted=True)
        cs.seeds.fill_(seed)
        cs.run(1, v)
        outs[name] = cs.x.view(-1, 4).cpu().numpy().view(np.uint32)
        jc = JumpCase(n, n, target_zero=True)
        jc.seeds.fill_(seed)
        jc.run(c=2, v=v, jump=1)
        outs["jump-" + name] = jc.x.view(-1, 4).cpu().numpy().view(np.uint32)
    for name in ("a", "draw", "b"):
        assert shared_blocks(outs[name], outs["jump-" + name]) == 0, f"{name}: a block is shared with the jump of the same seed and counter"
    assert shared_blocks(outs["a"], outs["draw"]) == 0
    assert shared_blocks(eta_noise_words(1, 0, n), noise_words(1, 0, n)) == 0 and shared_blocks(eta_noise_words(-77, 3, n), noise_words(-77, 3, n)) == 0


def test_moments_over_many_values(dev):
    n = 1 << 20
    cs = Case(n, n, seed=3, crafted=True)
    cs.run(0, 0)
    got = cs.x.cpu().numpy().astype(np.float64)
    err = np.abs(got - z64(cs.seeds_host, 0, n))
    print(f"[ddim_eta noise 2^20] max |z_gpu - z_fp64| = {err.max():.3e}; mean {got.mean():.3e}, var {got.var():.6f}")
    assert err.max() <= NOISE_LIMIT
    assert abs(got.mean()) < 5 / np.sqrt(n) and abs(got.var() - 1) < 5 * np.sqrt(2 / n), (got.mean(), got.var())


def test_scheduler_step_with_variance_noise_against_the_reference(dev):
    """DDIMScheduler.step(..., eta, variance_noise=) on the kernel against the reference scheduler's recorded prev_sample: the bound of
    tests/test_ddim_eta_contract.py (the reference's own 9 fp32 operations and the tables' bounds) plus the kernel's 9."""
    worst = 0.0
    for c in _golden():
        sch = schedulers.DDIMScheduler(); sch.set_timesteps(c["n_steps"])
        t32 = lambda a: torch.tensor(a, dtype=torch.float32, device=dev).view(1, 4, 2, 2)
        kw = dict(variance_noise=t32(c["z"])) if c["eta"] > 0 else {}
        out = sch.step(t32(c["eps"]), c["timestep"], t32(c["sample"]), eta=c["eta"], use_clipped_model_output=bool(c["index"] % 2), **kw)
        got = out.prev_sample.cpu().double().numpy().reshape(-1)
        tup = sch.step(t32(c["eps"]), torch.tensor(c["timestep"], device=dev), t32(c["sample"]), eta=c["eta"], return_dict=False, **kw)
        assert isinstance(tup, tuple) and torch.equal(tup[0], out.prev_sample), "a device timestep must give the host timestep's bits"
        i = c["index"]
        c0, c1, c2, _ = sch.coefficient_table()[i].double().tolist()
        d, s = sch.variance_table(c["eta"])[i].double().tolist()
        tol_dir, tol_std = table_bounds(c["a_t"], c["a_prev"], c["eta"])
        S = c2 * (np.abs(c["sample"]) + c1 * np.abs(c["eps"])) / c0 + d * np.abs(c["eps"]) + s * np.abs(c["z"])
        bound = 2 * 9 * ULP * S + tol_dir * np.abs(c["eps"]) + tol_std * np.abs(c["z"])
        ratio = float((np.abs(got - c["prev"]) / bound).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, f"{c['n_steps']} steps eta={c['eta']} row {i}: |step - reference| / bound = {ratio:.3f}"
    print(f"[ddim_eta scheduler.step] worst |step - reference scheduler| / bound = {worst:.3f}")
    with pytest.raises(ValueError, match="variance_noise"):
        sch.step(t32(c["eps"]), c["timestep"], t32(c["sample"]), eta=0.5)


# ---- the pipeline ----------------------------------------------------------------------------------------------------------------
_PIPES = {}
H, W, CL = 28, 50, 4


def zero_eps_pipe(dev, dt="bf16", given_view=False):
    """A TINY_CONFIG pipeline whose UNet ends in a zeroed conv_out: the noise prediction is exactly 0 whatever the conditions are."""
    if (dt, given_view) not in _PIPES:
        from magicdrive_amd.networks.unet_2d_condition_multiview import UNet2DConditionModelMultiview
        from magicdrive_amd.networks.unet_addon_rawbox import BEVControlNetModel
        from magicdrive_amd.pipeline.pipeline_bev_controlnet import StableDiffusionBEVControlNetPipeline
        from magicdrive_amd.pipeline.pipeline_bev_controlnet_given_view import StableDiffusionBEVControlNetGivenViewPipeline
        cfg = spec.TINY_CONFIG
        kw = {"torch_dtype": torch.float16} if dt == "f16" else {}
        sd = spec.random_state_dict(spec.unet_param_shapes(cfg), 0)
        sd["conv_out.weight"].zero_(); sd["conv_out.bias"].zero_()
        cls = StableDiffusionBEVControlNetGivenViewPipeline if given_view else StableDiffusionBEVControlNetPipeline
        _PIPES[(dt, given_view)] = cls(unet=UNet2DConditionModelMultiview(cfg, sd, **kw), controlnet=BEVControlNetModel.from_config(cfg, 1, **kw)).to(dev)
    return _PIPES[(dt, given_view)]


def scene_inputs(dt="bf16", n=2):
    sc = scene(spec.TINY_CONFIG, n, 5)
    if dt == "f16":
        sc["prompt_embeds"], sc["negative_prompt_embeds"] = sc["prompt_embeds"].half(), sc["negative_prompt_embeds"].half()
    return sc


def one_scene(sc, i):
    out = {k: (v[i:i + 1] if isinstance(v, torch.Tensor) else v) for k, v in sc.items()}
    out["bboxes_3d_data"] = {k: v[i:i + 1] for k, v in sc["bboxes_3d_data"].items()}
    return out


def call(pipe, sc, steps, **kw):
    out = pipe(prompt=None, image=sc["bev_map"], camera_param=sc["camera_param"], height=224, width=400, num_inference_steps=steps, guidance_scale=2.0,
               latents=sc["latents"], prompt_embeds=sc["prompt_embeds"], negative_prompt_embeds=sc["negative_prompt_embeds"], output_type="latent",
               bev_controlnet_kwargs={"bboxes_3d_data": sc["bboxes_3d_data"]}, **kw)
    torch.cuda.synchronize()
    return out


def gens(base, n=2):
    """One generator per scene (the list form): the latents are passed in, so each generator's first draw is its scene's seed."""
    return [torch.Generator().manual_seed(base + i) for i in range(n)]


def first_draws(base, n=2):
    return [int(torch.empty(1, dtype=torch.int64).random_(generator=g)) for g in gens(base, n)]


def eta_plans(pipe):
    return [p for k, p in pipe._plans._d.items() if ("eta",) in k]


def closed_form(lat, seed, coef, var, actions=None, draws=None):
    """float64 (x, bound) of one view, NHWC order, for eps == 0: every step x <- (c2 / c0) x + std z(seed, draw); every ("jump", j) entry
    x <- r x + sg z_jump(seed, visit) with the contract's fp32 r and sg.  The kernel rounds the quotient x / c0, the product with c2, the
    product std z and the sum (the terms with e = 0 are exact): a step adds u (2 |a x| + |std z| + |x'|) + 1e-5 std to a times the
    bound so far; a jump u (|r x| + |sg z| + |x'|) + 1e-5 sg to r times it (tests/test_latent_renoise_gpu.py).  draws: the draw counter
    of each step launch (default 0, 1, 2, ...)."""
    coef, var = coef.double().numpy(), var.double().numpy()
    x = lat.permute(1, 2, 0).reshape(-1).double().numpy()
    bound = np.zeros_like(x)
    actions = actions or ["step"] * len(coef)
    c = launch = visit = 0
    for act in actions:
        if act == "step":
            a, s = coef[c, 2] / coef[c, 0], var[c, 1]
            z = eta_noise_ref(seed, launch if draws is None else draws[launch], x.size)
            new = a * x + s * z
            bound = a * bound + U * (2 * np.abs(a * x) + np.abs(s * z) + np.abs(new)) + NOISE_LIMIT * s
            x, c, launch = new, c + 1, launch + 1
        else:
            j = act[1]
            r = float(np.float32(coef[c - j, 0]) / np.float32(coef[c - 1, 2]))
            sg = float(np.sqrt(np.maximum(np.float32(0), np.float32(1.0 - r * r)), dtype=np.float32))
            z = noise_ref(seed, visit, x.size)
            new = r * x + sg * z
            bound = r * bound + U * (np.abs(r * x) + np.abs(sg * z) + np.abs(new)) + NOISE_LIMIT * sg
            x, c, visit = new, c - j, visit + 1
    return x, bound


@pytest.mark.parametrize("dt,steps,eta", [("bf16", 4, 1.0), ("f16", 6, 0.3)])
def test_pipeline_latents_have_their_closed_form(dev, dt, steps, eta):
    pipe = zero_eps_pipe(dev, dt)
    sc = scene_inputs(dt)
    pipe._plans.clear()
    seen = []
    first = call(pipe, sc, steps, eta=eta, generator=gens(41), callback=lambda i, t, lat: seen.append((i, int(t)))).images.clone()
    plan, = eta_plans(pipe)
    assert int(plan.step_ctr) == steps and int(plan.draw_ctr) == steps
    assert [i for i, _ in seen] == list(range(steps)) and [t for _, t in seen] == pipe.scheduler.timesteps.tolist()
    want = first_draws(41)
    assert plan.seeds.tolist() == [want[0]] * 6 + [want[1]] * 6, "one seed per scene: its generator's first draw, shared by its views"
    sch = schedulers.DDIMScheduler(); sch.set_timesteps(steps)
    assert torch.equal(plan.coef.cpu(), sch.coefficient_table()) and torch.equal(plan.var.cpu(), sch.variance_table(eta))
    got = plan.x.view(2, 6, -1).cpu().double().numpy()
    worst = 0.0
    for i in range(2):
        ref, bound = closed_form(sc["latents"][i], want[i], sch.coefficient_table(), sch.variance_table(eta))
        for v in range(6):
            worst = max(worst, float((np.abs(got[i, v] - ref) / bound).max()))
    print(f"[ddim_eta pipeline {dt} {steps} steps eta={eta}] worst |latents - closed form| / derived bound = {worst:.3f}")
    assert worst <= 1.0
    assert torch.equal(first.float().cpu(), plan.latents().to(first.dtype).float().cpu())
    # the same seed, the same bits; the eager loop, the graph's bits; another seed, another sample
    assert torch.equal(call(pipe, sc, steps, eta=eta, generator=gens(41)).images, first)
    pipe.use_graph = False
    try:
        assert torch.equal(call(pipe, sc, steps, eta=eta, generator=gens(41)).images, first), "use_graph=False must give the captured graph's bits"
    finally:
        pipe.use_graph = True
    assert not torch.equal(call(pipe, sc, steps, eta=eta, generator=gens(42)).images, first)


def test_eta_is_data_of_one_plan_and_zero_is_the_plain_call(dev):
    pipe = zero_eps_pipe(dev)
    sc = scene_inputs()
    pipe._plans.clear()
    plain = call(pipe, sc, 4).images.clone()
    key0, = list(pipe._plans._d)
    zero = call(pipe, sc, 4, eta=0.0, generator=gens(5)).images
    assert list(pipe._plans._d) == [key0] and torch.equal(zero, plain), "eta = 0 is today's call: the same plan key, the same bits"
    assert sum(isinstance(o, O.DdimStep) for o in pipe._plans._d[key0].step_ops) == 1 and not any(isinstance(o, O.DdimEtaStep) for o in pipe._plans._d[key0].step_ops)
    a = call(pipe, sc, 4, eta=1.0, generator=gens(5)).images.clone()
    keys = list(pipe._plans._d)
    assert len(keys) == 2 and keys[1] == key0 + (("eta",),), "exactly one trailing key entry"
    b = call(pipe, sc, 4, eta=0.25, generator=gens(5)).images.clone()
    assert list(pipe._plans._d) == keys, "a second eta value reuses the plan: eta is data"
    plan, = eta_plans(pipe)
    sch = schedulers.DDIMScheduler(); sch.set_timesteps(4)
    assert torch.equal(plan.var.cpu(), sch.variance_table(0.25)) and sum(isinstance(o, O.DdimEtaStep) for o in plan.step_ops) == 1
    assert not torch.equal(a, b) and not torch.equal(a, plain) and torch.isfinite(a).all() and torch.isfinite(b).all()
    # the deterministic closed form of the plain call: the eta plan's table at eta = 0 is the same update (dir = c3, std = 0)
    ref, _ = closed_form(sc["latents"][0], 0, sch.coefficient_table(), sch.variance_table(0.0))
    got = pipe._plans._d[key0].x.view(2, 6, -1)[0, 0].cpu().double().numpy()
    assert (np.abs(got - ref) <= 8 * U * np.abs(ref) * (1 + 1e-6)).all(), "4 steps of two roundings each (x / c0, the product with c2)"
    # UniPC keeps refusing, before any device work
    keep = pipe.scheduler
    pipe.scheduler = schedulers.UniPCMultistepScheduler.from_config(keep.config)
    try:
        with pytest.raises(NotImplementedError, match="UniPC"):
            call(pipe, sc, 4, eta=0.5)
        with pytest.raises(ValueError, match="eta="):
            call(pipe, sc, 4, eta=-1.0)
    finally:
        pipe.scheduler = keep
    assert list(pipe._plans._d) == keys


def test_a_scene_alone_in_a_batch_in_chunks_and_with_health(dev):
    """A scene's seed — hence its step noise — is the same in a call of its own (the forked one-scene plan) and inside a batch; with eps = 0
    the update is elementwise, so the scene's latents are the same BITS alone, in the batch and as a chunk on its own stream; the health
    trace changes no bit; box_bucket and scene_boxes run on the stochastic plan."""
    pipe = zero_eps_pipe(dev)
    sc = scene_inputs()
    pipe._plans.clear()
    try:
        single = call(pipe, sc, 4, eta=0.8, generator=gens(31)).images.clone()
        batch_plan, = eta_plans(pipe)
        batch_seeds = batch_plan.seeds.clone()
        assert batch_plan.fork_at is not None
        pipe.health = "trace"
        traced = call(pipe, sc, 4, eta=0.8, generator=gens(31))
        pipe.health = None
        alone = []
        for i in range(2):
            alone.append(call(pipe, one_scene(sc, i), 4, eta=0.8, generator=[gens(31)[i]]).images.clone())
            p1, = [p for p in eta_plans(pipe) if p.b == 1 and p.health is None]
            assert p1.seeds.tolist() == [first_draws(31)[i]] * 6 == batch_seeds[6 * i:6 * i + 6].tolist()
        pipe.streams, pipe.min_scenes_per_stream = 2, 1
        chunked = call(pipe, sc, 4, eta=0.8, generator=gens(31)).images.clone()
        pipe.streams, pipe.min_scenes_per_stream = None, 16
        pipe.box_bucket, pipe.scene_boxes = 4, True
        bucket = call(pipe, sc, 4, eta=0.8, generator=gens(31)).images.clone()
    finally:
        pipe.streams, pipe.min_scenes_per_stream, pipe.health, pipe.box_bucket, pipe.scene_boxes = None, 16, None, None, False
    assert batch_seeds[0] != batch_seeds[6]
    assert torch.equal(traced.images, single) and traced.health.ok == [True, True] and traced.health.trace.shape == (4, 2, 6, 4)
    assert torch.equal(torch.cat(alone), single), "a scene alone differs from itself in the batch"
    assert torch.equal(chunked, single), "two chunks on two streams differ from the one-chunk call"
    assert torch.equal(bucket, single), "box_bucket / scene_boxes changed the stochastic sample (eps is 0: they must not)"


def test_a_revisited_step_draws_fresh_noise(dev):
    """keep_masks + resample = (2, 2) at 6 steps + eta: 10 step launches and 2 jumps on ONE seed per scene.  A view without a conditional
    latent is regenerated whole (its mask is 0: the blend leaves it alone), so it follows the closed form with draw = 0 .. 9 and
    visit = 0, 1 — and NOT the one in which a revisited step reuses the draw of its first visit."""
    from magicdrive_amd.schedulers import resample_actions
    pipe = zero_eps_pipe(dev, given_view=True)
    sc, cl = scene_inputs(), given_view_inputs()
    pipe._plans.clear()
    try:
        pipe.keep_masks = [[None if v is None else torch.full((H, W), 0.5) for v in r] for r in cl]
        pipe.resample = (2, 2)
        out = call(pipe, sc, 6, eta=1.0, generator=gens(61), conditional_latents=cl).images.clone()
        again = call(pipe, sc, 6, eta=1.0, generator=gens(61), conditional_latents=cl).images
        keys = list(pipe._plans._d)
    finally:
        pipe.keep_masks, pipe.resample = None, None
    assert len(keys) == 1 and keys[0][-3:] == (("regions",), ("resample", 2), ("eta",))
    plan = pipe._plans._d[keys[0]]
    assert (int(plan.step_ctr), int(plan.draw_ctr), int(plan.visit_ctr)) == (6, 10, 2), "the jump moves step_ctr back and leaves draw_ctr alone"
    want = first_draws(61)
    assert plan.seeds.tolist() == [want[0]] * 6 + [want[1]] * 6 and plan.jump_ops[0].seeds is plan.seeds, "one draw, one tensor for both streams"
    assert torch.equal(again, out) and torch.isfinite(out).all()
    acts = resample_actions(6, 2, 2)
    assert acts.count("step") == 10
    sch = schedulers.DDIMScheduler(); sch.set_timesteps(6)
    got = plan.x.view(2, 6, -1).cpu().double().numpy()
    steps_taken, c = [], 0
    for a in acts:
        if a == "step":
            steps_taken.append(c); c += 1
        else:
            c -= a[1]
    assert steps_taken == [0, 1, 2, 3, 2, 3, 4, 5, 4, 5]
    for i, v in ((0, 1), (1, 0), (1, 4)):                      # views without a conditional latent
        assert cl[i][v] is None
        ref, bound = closed_form(sc["latents"][i], want[i], sch.coefficient_table(), sch.variance_table(1.0), actions=acts)
        ratio = float((np.abs(got[i, v] - ref) / bound).max())
        print(f"[ddim_eta resample scene {i} view {v}] |latents - closed form| / derived bound = {ratio:.3f}")
        assert ratio <= 1.0
        stale, _ = closed_form(sc["latents"][i], want[i], sch.coefficient_table(), sch.variance_table(1.0), actions=acts, draws=steps_taken)
        assert (np.abs(got[i, v] - stale) / bound).max() > 1e3, "the result matches the closed form in which a revisited step REUSES its noise"
