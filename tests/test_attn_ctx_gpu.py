"""-m gpu: attn_ctx_kernel (csrc/attention_ctx.hip) — context attention whose key count is read from device memory (MdxAttnDesc.tk_dev).

Reference: fp32 torch attention over the first n keys.  Every case also runs the existing kernels (tk_dev = NULL, Tk = n, tight buffers) on
the same inputs.  The inputs are built so that a kernel that ignores tk_dev is wrong by O(1): keys >= n are scaled x8 in K and carry O(1)
values in V^T.

Accuracy bound (no number fixed in advance): for each (d, dtype) the existing kernel's rel-L2 against the fp32 reference is measured over all
cases of this file — pooled, sqrt(sum |o - ref|^2 / sum |ref|^2), ONE value — and the new kernel, pooled the same way over the same inputs, gets
2x that value: both kernels round P and O once to 16 bits, only tile size and summation order differ (the margin of the CLIP change).  The
measured pairs go to the parity log (helpers.parity_log, records named box_bucket:*)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import parity_log  # noqa: E402
from magicdrive_amd import _lib as L  # noqa: E402
from magicdrive_amd import ops as O  # noqa: E402

B, H = 3, 2
DIMS = (16, 32, 40, 80, 160)
TQS = (28, 91, 130)            # a partial wave, a partial workgroup, two workgroups
CAPS = (96, 200)
DTYPES = (torch.bfloat16, torch.float16)
NAN = float("nan")
PAD = 8                        # V^T pitch beyond roundup8(capacity): real pad columns, NaN-filled
LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453


def counts(Tk):
    return [n for n in (1, 31, 32, 33, 63, 64, 65, 78, Tk - 1, Tk) if n <= Tk]


def rup8(x):
    return (x + 7) // 8 * 8


def make(d, Tq, Tk, n, pre, dtype, seed=0):
    """q [B,Tq,C], k [B,Tk,C] (rows >= n scaled x8), vt [B,C,ldv] with ldv = roundup8(Tk) + 8 (columns Tk..ldv NaN); plus the fp32 reference over the first n keys.
    Drawn at the largest capacity and cut to Tk: the same (d, Tq, n, pre) has the same Q and the same first Tk keys at every capacity."""
    g = torch.Generator(device="cuda").manual_seed(seed + 1000 * d + 10 * Tq + n)
    C = H * d
    q = torch.randn(B, Tq, C, generator=g, device="cuda")
    k = torch.randn(B, max(CAPS), C, generator=g, device="cuda")[:, :Tk].contiguous()
    v = torch.randn(B, max(CAPS), C, generator=g, device="cuda")[:, :Tk].contiguous()
    k[:, n:] *= 8.0
    scale = d ** -0.5
    if pre:                         # the caller folded scale * log2(e) into Q: scores are base-2 exponents
        q = q * (scale * LOG2E)
    q, k, v = q.to(dtype), k.to(dtype), v.to(dtype)
    vt = torch.full((B, C, rup8(Tk) + PAD), NAN, dtype=dtype, device="cuda")      # ldv > Tk: the pad columns Tk .. ldv hold NaN in EVERY run
    vt[:, :, :Tk] = v.transpose(1, 2)
    return q, k, vt, reference(q, k[:, :n], v[:, :n], d, LN2 if pre else scale)


def reference(q, k, v, d, factor):
    Bq, Tq, C = q.shape
    qh = q.float().view(Bq, Tq, H, d).transpose(1, 2)
    kh = k.float().view(Bq, -1, H, d).transpose(1, 2)
    vh = v.float().view(Bq, -1, H, d).transpose(1, 2)
    att = torch.softmax(qh @ kh.transpose(-1, -2) * factor, -1)
    return (att @ vh).transpose(1, 2).reshape(Bq, Tq, C)


def live_of(n):
    return torch.tensor([n], dtype=torch.int32, device="cuda")


def run_ctx(q, k, vt, Tk, live, d, pre, o=None):
    o = torch.full_like(q, NAN) if o is None else o
    O.run_ops([O.Attn(q, k, vt, o, heads=H, Tk=Tk, scale=d ** -0.5, q_prescaled=pre, tk_dev=live)])
    kern = (L.lib().mdx_last_kernel() or b"").decode()
    assert kern == f"attn_ctx_kernel<{d},{'pre' if pre else 'scaled'}>", kern
    return o


def run_exact(q, k, vt, n, d, pre):
    """The existing kernels: tk_dev = NULL, Tk = n, tight buffers."""
    kt = k[:, :n].contiguous()
    vtt = torch.zeros(vt.shape[0], vt.shape[1], rup8(n), dtype=vt.dtype, device="cuda")
    vtt[:, :, :n] = vt[:, :, :n]
    o = torch.full_like(q, NAN)
    O.run_ops([O.Attn(q, kt, vtt, o, heads=H, Tk=n, scale=d ** -0.5, q_prescaled=pre)])
    kern = (L.lib().mdx_last_kernel() or b"").decode()
    assert not kern.startswith("attn_ctx_kernel"), kern
    return o


def poisoned(k, vt, Tk, n):
    kp, vp = k.clone(), vt.clone()
    kp[:, n:] = NAN
    vp[:, :, n:] = NAN             # columns n .. Tk and the pad columns Tk .. ldv
    return kp, vp


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("d", DIMS)
def test_live_key_count_every_edge(dev, d, dtype):
    """Every (Tq, capacity, n, q_prescaled): wrong by O(1) without tk_dev, finite and bit-identical under NaN poison, bit-identical across the
    two capacities, and within 2x the existing kernel's pooled rel-L2 (measured here, on the same inputs)."""
    kind = "bf16" if dtype == torch.bfloat16 else "fp16"
    e_new = e_old = r2 = 0.0
    worst = (0.0, None)
    for pre in (False, True):
        for Tq in TQS:
            by_n = {}
            for Tk in CAPS:
                for n in counts(Tk):
                    q, k, vt, ref = make(d, Tq, Tk, n, pre, dtype)
                    o = run_ctx(q, k, vt, Tk, live_of(n), d, pre)
                    assert torch.isfinite(o).all(), (Tq, Tk, n, pre)
                    # poison: what lies at or past n, pad columns included, never reaches O
                    kp, vp = poisoned(k, vt, Tk, n)
                    op = run_ctx(q, kp, vp, Tk, live_of(n), d, pre)
                    assert torch.equal(op, o), f"poison leaks: Tq={Tq} Tk={Tk} n={n} pre={pre}"
                    # the existing kernel at Tk = n on the same inputs
                    ox = run_exact(q, k, vt, n, d, pre)
                    dn, dx = (o.float() - ref).pow(2).sum().item(), (ox.float() - ref).pow(2).sum().item()
                    rr = ref.pow(2).sum().item()
                    e_new += dn; e_old += dx; r2 += rr
                    if (dn / rr) ** 0.5 > worst[0]:
                        worst = ((dn / rr) ** 0.5, (Tq, Tk, n, pre, (dx / rr) ** 0.5))
                    if n < Tk:      # must fail without the feature: ignoring tk_dev (all Tk keys, the x8 rows included) is far off
                        full = reference(q, k, vt[:, :, :Tk].transpose(1, 2), d, LN2 if pre else d ** -0.5)
                        assert ((full - ref).norm() / ref.norm()).item() > 0.3
                        assert ((o.float() - ref).norm() / ref.norm()).item() < 0.05, (Tq, Tk, n, pre)
                    # capacity independence: the same Q and first n keys (make) at the other capacity, other strides and pitch
                    if n in by_n:
                        assert torch.equal(o, by_n[n]), f"capacity dependence: Tq={Tq} n={n} pre={pre}"
                    elif Tk == CAPS[0]:
                        by_n[n] = o
    new, old = (e_new / r2) ** 0.5, (e_old / r2) ** 0.5
    print(f"[attn_ctx d={d} {kind}] pooled rel-L2 new {new:.3e} existing {old:.3e}; worst case new {worst[0]:.3e} at (Tq,Tk,n,pre,existing) {worst[1]}")
    parity_log(f"box_bucket:attn_ctx:d{d}:{kind}", new=new, existing=old, limit=2 * old, worst_case_new=worst[0], worst_case=str(worst[1]))
    assert new <= 2 * old, f"d={d} {kind}: pooled rel-L2 {new:.3e} > 2 x existing {old:.3e}"


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_graph_replay_reads_the_current_count(dev, dtype):
    """One captured launch, replayed with live = 40, 78, 40: each replay equals the eager run for that n; first and third are bit-identical."""
    d, Tq, Tk = 40, 130, 96
    q, k, vt, _ = make(d, Tq, Tk, 40, True, dtype)
    eager = {n: run_ctx(q, k, vt, Tk, live_of(n), d, True) for n in (40, 78)}
    assert not torch.equal(eager[40], eager[78])
    live = live_of(40)
    o = torch.full_like(q, NAN)
    prog = O.build_program([O.Attn(q, k, vt, o, heads=H, Tk=Tk, scale=d ** -0.5, q_prescaled=True, tk_dev=live)])
    torch.cuda.synchronize()
    st = torch.cuda.current_stream().cuda_stream
    outs = []
    for n in (40, 78, 40):
        live.fill_(n)                      # an ordinary stream-ordered write between replays
        o.fill_(NAN)
        prog.launch(st)
        outs.append(o.clone())
    torch.cuda.synchronize()
    prog.destroy()
    assert torch.equal(outs[0], eager[40]) and torch.equal(outs[1], eager[78]) and torch.equal(outs[2], outs[0])


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("d", (40, 160))
def test_count_out_of_range_is_loud(dev, d, dtype):
    """n = 0 and n = Tk + 1 cannot raise without a sync: every O row is NaN, and the kernel addresses as for a clamped n (the buffers are
    sized exactly: K has Tk rows, V^T rows end at ldv = roundup8(Tk))."""
    Tq, Tk = 91, 96
    q, k, vt, _ = make(d, Tq, Tk, Tk, False, dtype)
    for n in (0, Tk + 1, -5):
        o = run_ctx(q, k, vt, Tk, live_of(n), d, False, o=torch.zeros_like(q))
        assert torch.isnan(o).all(), n
    o = run_ctx(q, k, vt, Tk, live_of(Tk), d, False)
    assert torch.isfinite(o).all()


def test_last_batch_past_4g(dev):
    """Q and O batch strides that put the last batch item past 4 GiB (64-bit batch offsets); the small shape is checked there."""
    d, Tq, Tk, n, dtype = 40, 130, 96, 78, torch.bfloat16
    free = torch.cuda.mem_get_info()[0]
    if free < 10e9:
        pytest.skip(f"needs 10 GB of free device memory, {free / 1e9:.1f} GB free")
    C = H * d
    q, k, vt, ref = make(d, Tq, Tk, n, True, dtype)
    sB = 2 ** 30 + 8                                       # elements: batch 2 starts at 2 * sB * 2 bytes > 4 GiB
    qbuf = torch.empty(2 * sB + Tq * C, dtype=dtype, device="cuda")
    obuf = torch.empty(2 * sB + Tq * C, dtype=dtype, device="cuda")
    assert 2 * sB * 2 > 2 ** 32
    qs = torch.as_strided(qbuf, (B, Tq, C), (sB, C, 1))
    os_ = torch.as_strided(obuf, (B, Tq, C), (sB, C, 1))
    qs.copy_(q); os_.fill_(NAN)
    run_ctx(qs, k, vt, Tk, live_of(n), d, True, o=os_)
    small = run_ctx(q, k, vt, Tk, live_of(n), d, True)
    assert torch.equal(os_, small)
    assert ((os_[2].float() - ref[2]).norm() / ref[2].norm()).item() < 0.02
    del qbuf, obuf
    torch.cuda.empty_cache()
