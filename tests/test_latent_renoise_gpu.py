"""-m gpu: renoise_kernel (csrc/noise.hip, mdx_latent_renoise_*, ops.LatentRenoise) against the float64 evaluation of the documented
mapping (tests/test_latent_renoise_contract.py: numpy Philox4x32-10 with the Random123 known answers, Box-Muller in float64), both builds.

With c = *step_ptr, v = *visit_ptr: r = coef[c - jump, col_t] / coef[c - 1, col_p], sg = sqrtf(max(0, fma(-r, r, 1))), x <- fma(r, x, sg z),
z = z(seeds[g], v, e); then step <- c - jump, visit <- v + 1.

  1. noise values   a crafted table with target 0 gives r = 0, sg = 1: x becomes z itself.  |x - z64| <= 1e-5: |z| <= sqrt(48 ln 2) = 5.77,
                    u1, u2 and the Philox words are exact, what is left is the rounding of the angle (<= 3.7e-7), a few ulp each in log,
                    sqrt, cos, sin and one product: ~4.3e-6 at the largest radius, taken with a 2x margin.  4, 5, 7, 1027 groups of
                    1, 4, 20 elements and one group of 4, 5, 7, 1027; x aligned (16-byte instance where group_elems % 4 == 0) and 4 bytes
                    off (scalar): equal bits.
                    The measured maximum is printed (DESIGN.md quotes it).
  2. general update against float64 r x + sg z with r, sg the contract's fp32 values: |err| <= 1e-5 sg + 4 * 2^-24 |ref| (the noise's
                    1e-5 scaled by sg, plus the roundings of the product and of the fma on terms bounded by |ref| + sg |z|); both x_in
                    layouts, both CFG halves, pad channels and guard bands untouched.
  3. counters       step and visit after a launch; the SAME captured graph replayed gives the noise of v + 1; each out-of-range case
                    fills x with NaN and leaves x_in and both counters alone.
  4. independence   permuting groups with their seeds permutes the result bit for bit; equal seeds, equal bits; different seeds or
                    visits share no 4-word block over 2^16 elements; mean and variance of 2^20 values within 5 standard errors.
  5. 64-bit         one x that crosses the 4 GiB mark, sampled positions against the reference.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from magicdrive_amd import _lib as L  # noqa: E402
from magicdrive_amd import ops as O  # noqa: E402
from philox_ref import noise_ref, noise_words, shared_blocks  # noqa: E402

U = 2.0 ** -24
NAN = float("nan")
SENT = -12288.0            # exact in fp32, bf16 and fp16
GUARD = 64
ROWS, LD = 6, 4
BUILDS = {"bf16": (L.DTYPE_BF16, torch.bfloat16), "f16": (L.DTYPE_F16, torch.float16)}
NOISE_LIMIT = 1e-5


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
    g = torch.Generator().manual_seed(77 + salt)
    return torch.empty(groups, dtype=torch.int64).random_(generator=g) * torch.where(torch.arange(groups) % 2 == 0, 1, -1)   # both signs: all 64 bits


def z64(seeds, visit, group_elems):
    """float64 [groups * group_elems]: the reference noise of every group."""
    return np.concatenate([noise_ref(int(s), visit, group_elems) for s in seeds.tolist()])


class Case:
    """Operands of one launch, each in a guarded allocation.  The table is random (its rows need not be a schedule): the target column in
    [0.2, 0.6], the current column in [0.62, 0.95], so r is in (0.2, 0.97) and both terms of the update matter."""

    def __init__(self, n, group_elems, xin="none", cfg=0, dtype16=torch.bfloat16, off=0, C=1, xin_ld=0, seed=0, target_zero=False):
        gen = torch.Generator(device="cuda").manual_seed(2000 + seed)
        self.n, self.ge, self.cfg, self.off, self.C, self.xin_ld = n, group_elems, cfg, off, C, xin_ld
        self.x0 = torch.randn(n, generator=gen, device="cuda") * 2.0
        self.xb, self.x = guarded(self.x0, off)
        tab = torch.rand(ROWS * LD, generator=gen, device="cuda") * 0.65 + 0.3
        self.coefb, coef = guarded(tab)
        self.coef = coef.view(ROWS, LD)
        self.coef[:, 0] = 0.2 + 0.4 * torch.rand(ROWS, generator=gen, device="cuda")
        self.coef[:, 2] = 0.62 + 0.33 * torch.rand(ROWS, generator=gen, device="cuda")
        if target_zero:
            self.coef[:, 0] = 0.0
        self.step = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.visit = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.seeds_host = seeds_for(n // group_elems, seed)
        self.sb, self.seeds = guarded(self.seeds_host.cuda(), fill=0x5A5A5A5A5A5A5A5A)
        c = 2 if cfg else 1
        self.x_in, self.xinb = None, None
        if xin == "h16":
            rows = c * (n // C)
            self.xinb = torch.full(((rows + 2) * xin_ld,), SENT, dtype=dtype16, device="cuda")
            self.x_in = self.xinb[:rows * xin_ld].view(rows, xin_ld)
        elif xin == "f32":
            self.xinb, self.x_in = guarded(torch.full((c * n,), SENT, device="cuda"), fill=SENT)

    def op(self, jump):
        return O.LatentRenoise(self.x, self.coef, self.step, self.visit, self.seeds, jump=jump, x_in=self.x_in, cfg=bool(self.cfg), xin_c=self.C if self.xin_ld else 0)

    def run(self, c, v, jump, build=L.DTYPE_BF16):
        self.step.fill_(c); self.visit.fill_(v)
        code, d = self.op(jump).lower()
        L.call_op(code, d, torch.cuda.current_stream().cuda_stream, build)
        torch.cuda.synchronize()
        return last_kernel()

    def r_sg(self, c, jump):
        """The contract's fp32 r and sg as float64 numbers (division and sqrt correctly rounded, 1 - r r with one rounding)."""
        t = self.coef.cpu().numpy()
        r = np.float32(t[c - jump, 0]) / np.float32(t[c - 1, 2])
        one_m = np.float32(1.0 - float(r) * float(r))
        return float(r), float(np.sqrt(np.maximum(np.float32(0), one_m), dtype=np.float32))

    def assert_guards(self):
        assert guards_intact(self.xb, GUARD + self.off, self.n, NAN), "x: a guard element was written"
        assert guards_intact(self.sb, GUARD, self.seeds.numel(), 0x5A5A5A5A5A5A5A5A) and guards_intact(self.coefb, GUARD, ROWS * LD, NAN)
        if self.x_in is not None and self.xin_ld:
            assert bool((self.xinb[self.x_in.numel():] == SENT).all()), "x_in: a row behind the last pixel was written"
        elif self.x_in is not None:
            assert guards_intact(self.xinb, GUARD, self.x_in.numel(), SENT), "x_in: a guard element was written"


@pytest.mark.parametrize("group", ["1", "4", "20", "whole"])
@pytest.mark.parametrize("m", [4, 5, 7, 1024 + 3])
def test_noise_values_are_the_documented_mapping(dev, m, group):
    """group_elems divides n, so m counts GROUPS of 1, 4 or 20 elements (group_elems 1: n = m itself), and "whole" is one group of m
    elements: n = 5, 7, 1027 with a partial last block."""
    n, ge = (m, m) if group == "whole" else (m * int(group), int(group))
    worst = 0.0
    outs = []
    for off in (0, 1):
        cs = Case(n, ge, off=off, seed=n % 13, target_zero=True)
        k = cs.run(c=3, v=2, jump=2)
        assert k == ("renoise_kernel" if off == 0 and ge % 4 == 0 else "renoise_kernel_scalar"), k
        got = cs.x.cpu().numpy().astype(np.float64)
        want = z64(cs.seeds_host, 2, ge)
        err = float(np.abs(got - want).max())
        worst = max(worst, err)
        assert np.isfinite(got).all() and err <= NOISE_LIMIT, f"n={n} group_elems={ge} off={off}: |x - z| max {err:.3e} > {NOISE_LIMIT}"
        cs.assert_guards()
        assert int(cs.step) == 1 and int(cs.visit) == 3
        outs.append(cs.x.clone())
    print(f"[renoise noise n={n} group_elems={ge}] max |z_gpu - z_fp64| = {worst:.3e} (limit {NOISE_LIMIT})")
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), "the scalar instance must give the 16-byte instance's bits"


def test_noise_accuracy_over_many_values(dev):
    """2^20 values of one group and 2^20 / 20 groups of 20: the maximum error where the largest radii live, and the moments."""
    n = 1 << 20
    cs = Case(n, n, seed=3, target_zero=True)
    cs.run(c=ROWS, v=0, jump=1)
    got = cs.x.cpu().numpy().astype(np.float64)
    want = z64(cs.seeds_host, 0, n)
    err = np.abs(got - want)
    i = int(err.argmax())
    print(f"[renoise noise 2^20] max |z_gpu - z_fp64| = {err.max():.3e} at |z| = {abs(want[i]):.3f}; max |z| = {np.abs(want).max():.3f} (limit {NOISE_LIMIT})")
    assert err.max() <= NOISE_LIMIT
    assert abs(got.mean()) < 5 / np.sqrt(n) and abs(got.var() - 1) < 5 * np.sqrt(2 / n), (got.mean(), got.var())


@pytest.mark.parametrize("build", ["bf16", "f16"])
@pytest.mark.parametrize("xin,cfg", [("f32", 0), ("f32", 1), ("h16", 0), ("h16", 1), ("none", 0)])
@pytest.mark.parametrize("shape", ["2x3x5x4", "263x4", "7x9x3"])
def test_general_update_against_float64(dev, shape, xin, cfg, build):
    code, dt16 = BUILDS[build]
    dims = [int(v) for v in shape.split("x")]
    C, pixels = dims[-1], int(np.prod(dims[:-1]))
    n = pixels * C
    ge = n // 2 if shape == "2x3x5x4" else (n if shape == "263x4" else 9 * 3)     # 60 (16-byte), 1052 (16-byte, > 1 workgroup), 27 (scalar, partial blocks)
    cs = Case(n, ge, xin=xin, cfg=cfg, dtype16=dt16, C=C, xin_ld=8 if xin == "h16" else 0, seed=len(shape) + cfg)
    c, v, jump = 5, 7, 3
    k = cs.run(c, v, jump, code)
    assert k == ("renoise_kernel" if ge % 4 == 0 else "renoise_kernel_scalar"), k
    r, sg = cs.r_sg(c, jump)
    assert 0.2 < r < 0.97 and sg > 0.24
    z = z64(cs.seeds_host, v, ge)
    ref = r * cs.x0.cpu().numpy().astype(np.float64) + sg * z
    got = cs.x.cpu().numpy().astype(np.float64)
    bound = 1e-5 * sg + 4 * U * np.abs(ref)
    ratio = float((np.abs(got - ref) / bound).max())
    print(f"[renoise update {shape} {xin} cfg={cfg} {build}] r={r:.4f} sg={sg:.4f} worst error / bound = {ratio:.3f}")
    assert ratio <= 1.0
    assert int(cs.step) == c - jump and int(cs.visit) == v + 1
    cs.assert_guards()
    if xin == "none":
        return
    halves = 2 if cfg else 1
    if xin == "h16":
        xi = cs.x_in.view(halves, pixels, 8)
        assert bool((xi[..., C:] == SENT).all()), "pad channels were written"
        for hf in range(halves):
            assert torch.equal(xi[hf, :, :C].reshape(-1), cs.x.to(dt16)), f"x_in half {hf} is not the 16-bit rounding of x"
    else:
        for hf in range(halves):
            assert torch.equal(cs.x_in.view(halves, n)[hf], cs.x)


def test_r_above_one_clamps_sigma(dev):
    """target > current (not a schedule, but a table may hold it): sg = sqrt(max(0, .)) = 0, x <- r x, never NaN."""
    cs = Case(64, 16, seed=1)
    cs.coef[2, 0], cs.coef[4, 2] = 0.9, 0.45
    cs.run(c=5, v=0, jump=3)
    assert torch.equal(cs.x, torch.full_like(cs.x0, 2.0) * cs.x0)


@pytest.mark.parametrize("build", ["bf16", "f16"])
def test_counters_and_graph_replay(dev, build):
    code, dt16 = BUILDS[build]
    n, ge = 2 * 7 * 9 * 4, 7 * 9 * 4
    cs = Case(n, ge, xin="h16", cfg=1, dtype16=dt16, C=4, xin_ld=8, seed=9, target_zero=True)
    lowered = cs.op(1).lower()
    prog = L.Program([(lowered[0], lowered[1], code)])
    st = torch.cuda.current_stream().cuda_stream
    cs.step.fill_(ROWS); cs.visit.fill_(4)
    seen = []
    for k in range(3):                               # the same captured graph: the counters it reads are the ones it wrote
        prog.launch(st)
        torch.cuda.synchronize()
        assert int(cs.step) == ROWS - 1 - k and int(cs.visit) == 5 + k
        got = cs.x.cpu().numpy().astype(np.float64)
        assert np.abs(got - z64(cs.seeds_host, 4 + k, ge)).max() <= NOISE_LIMIT, f"replay {k}: not the noise of visit {4 + k}"
        seen.append(cs.x.clone())
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])
    prog.destroy()
    cs.assert_guards()
    # out of range, discovered on the device: NaN in x, x_in and both counters untouched
    for c, jump, why in ((0, 1, "c < 1"), (-1, 1, "c < 1"), (ROWS + 1, 1, "c > n_rows"), (2, 3, "c - jump < 0")):
        cs = Case(n, ge, xin="h16", cfg=1, dtype16=dt16, C=4, xin_ld=8, seed=9)
        cs.run(c, 11, jump, code)
        assert bool(torch.isnan(cs.x).all()), why
        assert int(cs.step) == c and int(cs.visit) == 11, f"{why}: a counter moved"
        assert bool((cs.xinb == SENT).all()), f"{why}: x_in was written"
        cs.assert_guards()
    # the last row and a jump to row 0 are in range
    cs = Case(n, ge, seed=9)
    cs.run(ROWS, 0, ROWS)
    assert bool(torch.isfinite(cs.x).all()) and int(cs.step) == 0 and int(cs.visit) == 1


def test_groups_are_independent_of_position_and_size(dev):
    ge, groups = 20, 8
    n = ge * groups
    cs = Case(n, ge, seed=4)
    cs.run(4, 1, 2)
    base = cs.x.view(groups, ge).clone()
    perm = torch.tensor([5, 2, 7, 0, 3, 6, 1, 4])
    cp = Case(n, ge, seed=4)
    cp.x.copy_(cs.x0.view(groups, ge)[perm.cuda()].reshape(-1))
    cp.seeds.copy_(cs.seeds[perm.cuda()])
    cp.run(4, 1, 2)
    assert torch.equal(cp.x.view(groups, ge).view(torch.int32), base[perm.cuda()].view(torch.int32)), "permuting groups with their seeds must permute the result"
    # a group alone (n = group_elems, scalar or 16-byte instance, another launch geometry) has its bits in the batch
    for g in (0, 5):
        one = Case(ge, ge, seed=4, off=1 if g == 5 else 0)
        one.x.copy_(cs.x0.view(groups, ge)[g]); one.seeds.copy_(cs.seeds[g:g + 1]); one.coef.copy_(cs.coef)
        one.run(4, 1, 2)
        assert torch.equal(one.x.view(torch.int32), base[g].view(torch.int32)), f"group {g} alone differs from itself in the batch"
    # equal seeds: equal noise (r = 0 shows z itself)
    eq = Case(n, ge, seed=4, target_zero=True)
    eq.seeds.fill_(123456789)
    eq.run(3, 0, 1)
    assert bool((eq.x.view(groups, ge) == eq.x.view(groups, ge)[0]).all())


def test_seeds_and_visits_share_no_block(dev):
    """Over 2^16 elements: the 4-value blocks of another seed or another visit are all different (compared as the fp32 bits of z, and the
    reference's words likewise)."""
    n = 1 << 16
    outs = {}
    for name, seed, v in (("a", 1, 0), ("seed", 2, 0), ("visit", 1, 1), ("hi", 1 + (1 << 32), 0)):
        cs = Case(n, n, seed=0, target_zero=True)
        cs.seeds.fill_(seed)
        cs.run(2, v, 1)
        outs[name] = cs.x.view(-1, 4).cpu().numpy().view(np.uint32)
    for other in ("seed", "visit", "hi"):
        assert shared_blocks(outs["a"], outs[other]) == 0, f"a block is shared with another {other}"
    assert shared_blocks(noise_words(1, 0, n), noise_words(2, 0, n)) == 0 and shared_blocks(noise_words(1, 0, n), noise_words(1, 1, n)) == 0


def test_x_across_the_4gib_mark(dev):
    """n = 2^30 + 2^16 fp32 elements in two groups: element indices and byte offsets past 2^32, block counters past 2^27.  Sampled
    positions (the first and last blocks of both groups and the blocks around the 4 GiB mark) against the reference."""
    n = (1 << 30) + (1 << 16)
    ge = n // 2
    free, _ = torch.cuda.mem_get_info()
    assert free > 6 * (1 << 30), "the device has less than 6 GiB free"
    x = torch.ones(n, device="cuda")
    coef = torch.tensor([[0.0, 0.5, 0.5, 0.5], [0.0, 0.5, 0.5, 0.5]], device="cuda")
    step = torch.full((1,), 2, dtype=torch.int32, device="cuda")
    visit = torch.full((1,), 6, dtype=torch.int32, device="cuda")
    seeds = torch.tensor([-3, 1 << 40], dtype=torch.int64, device="cuda")
    O.run_ops([O.LatentRenoise(x, coef, step, visit, seeds, jump=1)])
    torch.cuda.synchronize()
    assert last_kernel() == "renoise_kernel" and int(step) == 1 and int(visit) == 7
    mark = 1 << 30                                   # the element at byte 2^32
    for g, seed in ((0, -3), (1, 1 << 40)):
        for e0 in (0, ge - 64, (mark - 32 - g * ge) if g == 1 else 4096):
            e0 -= e0 % 4
            i0 = g * ge + e0
            got = x[i0:i0 + 64].cpu().numpy().astype(np.float64)
            want = noise_ref(seed, 6, 64, first_block=e0 // 4)
            assert np.abs(got - want).max() <= NOISE_LIMIT, f"group {g} element {e0} (index {i0})"
    # nothing was left out: a value of exactly 1.0 (the fill) has probability ~2e-8, a skipped workgroup leaves 1024 of them
    assert int((x == 1.0).sum()) < 1000 and bool(torch.isfinite(x[mark - 1024:]).all())
    del x
