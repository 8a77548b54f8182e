"""-m gpu: attn_vrow_kernel (csrc/attention_vrow.hip, mdx_sdpa_*, ops.Sdpa / ops.sdpa) — flash attention on a row-major V at any length,
causal mask, key count per batch from device memory.  Both builds (bf16, fp16).

Reference: torch attention in float64 on the 16-bit-rounded inputs, compared with helpers.close at its own settings for the storage type
(the xformers table the flash-attention tests of tests/test_kernels_gpu.py use); test_kernels_gpu.ref_attention is the fp32 cross-check of
the unmasked cases.  No limit of this file is new.  K and V are always views of buffers whose remaining rows are NaN, O a view of a larger
NaN-filled buffer: every case also checks that nothing past Tk reaches O and that nothing outside O's view is written."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import close  # noqa: E402
from magicdrive_amd import _lib as L  # noqa: E402
from magicdrive_amd import ops as O  # noqa: E402
from test_kernels_gpu import ref_attention  # noqa: E402

DTYPES = (torch.bfloat16, torch.float16)
KIND = {torch.bfloat16: "bf16", torch.float16: "f16"}
IDS = ["bf16", "fp16"]
NAN = float("nan")
GUARD = 64                     # NaN rows behind the last key of every batch of K and V


def inputs(B, Tq, Tk, H, d, dtype, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed + 7919 * d + 31 * Tq + Tk + 1000003 * H + B)
    C = H * d
    return tuple(torch.randn(B, T, C, generator=g, device="cuda").to(dtype) for T in (Tq, Tk, Tk))


def guarded_kv(x):
    """x [B, Tk, C] as the view [:, :Tk] of a [B, Tk + 64, C] buffer whose other rows are NaN."""
    B, Tk, C = x.shape
    buf = torch.full((B, Tk + GUARD, C), NAN, dtype=x.dtype, device=x.device)
    buf[:, :Tk] = x
    return buf[:, :Tk]


class GuardedO:
    """A [B, Tq, C] view of a NaN-filled [B, Tq + 3, C + 8] buffer: guard rows behind every batch and guard columns behind every row."""

    def __init__(self, B, Tq, C, dtype):
        self.buf = torch.full((B, Tq + 3, C + 8), NAN, dtype=dtype, device="cuda")
        self.view = self.buf[:, :Tq, :C]

    def intact(self):
        rest = self.buf.clone()
        rest[:, :self.view.shape[1], :self.view.shape[2]] = NAN
        return bool(torch.isnan(rest).all())


def ref64(q, k, v, H, scale, causal=False, klen=None):
    """float64 attention on the given (16-bit) values; klen: list of key counts per batch."""
    B, Tq, C = q.shape
    Tk, d = k.shape[1], C // H
    qh = q.double().reshape(B, Tq, H, d).transpose(1, 2)
    kh = k.double().reshape(B, Tk, H, d).transpose(1, 2)
    vh = v.double().reshape(B, Tk, H, d).transpose(1, 2)
    s = qh @ kh.transpose(-1, -2) * scale
    j = torch.arange(Tk, device=q.device)
    if causal:
        s = s.masked_fill(j[None, :] > torch.arange(Tq, device=q.device)[:, None], float("-inf"))
    if klen is not None:
        n = torch.tensor(klen, device=q.device)
        s = s.masked_fill((j[None, :] >= n[:, None])[:, None, None, :], float("-inf"))
    return (s.softmax(-1) @ vh).transpose(1, 2).reshape(B, Tq, C)


def last_kernel():
    return (L.lib().mdx_last_kernel() or b"").decode()


def run(q, k, v, H, scale=None, causal=False, klen=None, o=None):
    """One launch through ops.run_ops on guarded operands; returns O's view.  Asserts the route and that O's guards are untouched."""
    B, Tq, C = q.shape
    scale = (C // H) ** -0.5 if scale is None else scale
    own = o is None
    if own:
        G = GuardedO(B, Tq, C, q.dtype)
        o = G.view
    O.run_ops([O.Sdpa(q, k, v, o, heads=H, scale=scale, causal=causal, klen=klen)])
    kern = last_kernel()
    assert kern.startswith("attn_vrow_kernel<"), kern
    torch.cuda.synchronize()
    if own:
        assert G.intact(), "a guard row or column of O was written"
    return o


def counts(vals):
    return torch.tensor(vals, dtype=torch.int32, device="cuda")


# (Tq, Tk, H, B): every listed Tk, Tq, H and B appears, Tq != Tk among them; run with every d
TAILS = [(1, 1, 1, 1), (31, 7, 3, 3), (32, 63, 1, 3), (33, 64, 3, 1), (129, 65, 1, 3), (1, 130, 3, 1), (129, 130, 3, 3), (33, 1, 3, 3)]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("d", (8, 40, 64, 80, 128, 160))
def test_tile_tails_and_guard_rows(dev, d, dtype):
    """Lengths around the 64-kv tile and the 32-query wave, with NaN behind the last key and around O.  Tk = 1: O = V[b, 0] bit for bit."""
    for Tq, Tk, H, B in TAILS:
        q, k, v = inputs(B, Tq, Tk, H, d, dtype)
        o = run(q, guarded_kv(k), guarded_kv(v), H)
        name = f"sdpa tails d={d} Tq={Tq} Tk={Tk} H={H} B={B}"
        assert torch.isfinite(o).all(), name
        close(o, ref64(q, k, v, H, d ** -0.5), name=name, kind=KIND[dtype])
        close(o, ref_attention(q.float(), k.float(), v.float(), H, d ** -0.5), name=name + " fp32", kind=KIND[dtype])
        if Tk == 1:
            assert torch.equal(o, v[:, :1].expand(B, Tq, H * d)), name


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("d", (40, 64, 160))
def test_fused_operand_has_the_bits_of_separate_copies(dev, d, dtype):
    """Q, K and V as the column blocks of one [B, T, 3C] tensor: nothing is copied and the bits equal the run on three contiguous copies."""
    B, T, H = 2, 130, 2
    C = H * d
    g = torch.Generator(device="cuda").manual_seed(d)
    qkv = torch.randn(B, T, 3 * C, generator=g, device="cuda").to(dtype)
    qs, ks, vs = qkv[:, :, :C], qkv[:, :, C:2 * C], qkv[:, :, 2 * C:]
    o = run(qs, ks, vs, H)
    o2 = run(qs.contiguous(), guarded_kv(ks), guarded_kv(vs), H)
    assert torch.equal(o, o2)
    close(o, ref64(qs, ks, vs, H, d ** -0.5), name=f"sdpa fused d={d}", kind=KIND[dtype])
    o3 = O.sdpa(qs, ks, vs, H)                         # the functional form: current stream, default scale, a new tensor
    torch.cuda.synchronize()
    assert o3.is_contiguous() and torch.equal(o3, o) and last_kernel().startswith("attn_vrow_kernel<")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("d", (16, 32, 40, 64, 160))
def test_causal(dev, d, dtype):
    """Row 0 = V[0] bit for bit; the masked reference; for T <= 128 and d in {32, 64} agreement with mdx_attention_* (v_rowmajor = causal = 1)."""
    B, H = 2, 3
    for T in (1, 33, 64, 65, 130):
        q, k, v = inputs(B, T, T, H, d, dtype, seed=1)
        o = run(q, guarded_kv(k), guarded_kv(v), H, causal=True)
        assert last_kernel().endswith(",causal>")
        name = f"sdpa causal d={d} T={T}"
        assert torch.equal(o[:, 0], v[:, 0]), name
        close(o, ref64(q, k, v, H, d ** -0.5, causal=True), name=name, kind=KIND[dtype])
        if T <= 128 and d in (32, 64):
            os_ = torch.full_like(q, NAN)
            O.run_ops([O.Attn(q, k, v, os_, heads=H, Tk=T, scale=d ** -0.5, causal=True, v_rowmajor=True)])
            assert last_kernel().startswith("attn_short_kernel<"), last_kernel()
            torch.cuda.synchronize()
            close(o, os_, name=name + " vs short", kind=KIND[dtype])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("d,Tq,Tk", [(40, 129, 130), (64, 33, 65), (160, 31, 63)])
def test_key_count_per_batch(dev, d, Tq, Tk, dtype):
    """klen_dev = [1, Tk, Tk // 2]: the reference on the truncated keys; what lies at or past a batch's count never reaches O (NaN there);
    the full-count batch has the bits of the klen_dev = NULL run; counts 0 and Tk + 1 give NaN in exactly that batch's rows."""
    B, H = 3, 2
    q, k, v = inputs(B, Tq, Tk, H, d, dtype, seed=2)
    lens = [1, Tk, Tk // 2]
    kg, vg = guarded_kv(k), guarded_kv(v)
    o = run(q, kg, vg, H, klen=counts(lens))
    name = f"sdpa klen d={d} Tq={Tq} Tk={Tk}"
    close(o, ref64(q, k, v, H, d ** -0.5, klen=lens), name=name, kind=KIND[dtype])
    assert torch.equal(o[0], v[0, :1].expand(Tq, H * d))                       # one key: V[0, 0] bit for bit
    assert torch.equal(o[1], run(q, kg, vg, H)[1]), "full count != klen_dev = NULL"
    kp, vp = k.clone(), v.clone()
    for b, n in enumerate(lens):
        kp[b, n:] = NAN; vp[b, n:] = NAN
    assert torch.equal(run(q, guarded_kv(kp), guarded_kv(vp), H, klen=counts(lens)), o), "keys at or past the count reach O"
    for b, bad in ((0, 0), (1, Tk + 1), (2, -7)):
        lb = list(lens); lb[b] = bad
        ob = run(q, kg, vg, H, klen=counts(lb))
        for bb in range(B):
            if bb == b:
                assert torch.isnan(ob[bb]).all(), (b, bad)
            else:
                assert torch.equal(ob[bb], o[bb]), (b, bad, bb)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_causal_with_key_count(dev, dtype):
    """Key j is visible to query i iff j <= i and j < klen[b]."""
    B, H, d, T = 3, 2, 40, 130
    q, k, v = inputs(B, T, T, H, d, dtype, seed=3)
    lens = [T, 70, 5]
    o = run(q, guarded_kv(k), guarded_kv(v), H, causal=True, klen=counts(lens))
    close(o, ref64(q, k, v, H, d ** -0.5, causal=True, klen=lens), name="sdpa causal + klen", kind=KIND[dtype])
    assert torch.equal(o[:, 0], v[:, 0])
    assert torch.equal(o[0], run(q, guarded_kv(k), guarded_kv(v), H, causal=True)[0])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_graph_replay_reads_the_current_counts(dev, dtype):
    """One captured program, replayed after the counts were rewritten on the device: each replay equals the eager run for those counts."""
    B, H, d, Tq, Tk = 3, 2, 40, 129, 130
    q, k, v = inputs(B, Tq, Tk, H, d, dtype, seed=4)
    kg, vg = guarded_kv(k), guarded_kv(v)
    sets = ([40, 130, 7], [130, 65, 64], [40, 130, 7])
    eager = [run(q, kg, vg, H, klen=counts(s)).clone() for s in sets[:2]]
    assert not torch.equal(eager[0], eager[1])
    kl = counts(sets[0])
    G = GuardedO(B, Tq, H * d, dtype)
    prog = O.build_program([O.Sdpa(q, kg, vg, G.view, heads=H, scale=d ** -0.5, klen=kl)])
    torch.cuda.synchronize()
    st = torch.cuda.current_stream().cuda_stream
    outs = []
    for s in sets:
        kl.copy_(counts(s))                # an ordinary stream-ordered write between replays
        G.view.fill_(NAN)
        prog.launch(st)
        outs.append(G.view.clone())
    torch.cuda.synchronize()
    prog.destroy()
    assert torch.equal(outs[0], eager[0]) and torch.equal(outs[1], eager[1]) and torch.equal(outs[2], outs[0])
    assert G.intact()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("causal", (False, True), ids=["full", "causal"])
def test_batch_independence_across_workgroup_widths(dev, causal, dtype):
    """The rows of batch b from a B = 3 launch equal the bits of a B = 1 launch on that batch alone — at a shape where the launcher picks
    4 waves per workgroup for B = 3 (ceil(256 / 128) * 64 * 3 = 384 >= 256 blocks) and 2 for B = 1 (128 blocks, T >= 64)."""
    B, H, d, T = 3, 64, 8, 256
    q, k, v = inputs(B, T, T, H, d, dtype, seed=5)
    o = run(q, k, v, H, causal=causal)
    assert last_kernel().startswith("attn_vrow_kernel<1,4,"), last_kernel()
    for b in range(B):
        ob = run(q[b:b + 1], k[b:b + 1], v[b:b + 1], H, causal=causal)
        assert last_kernel().startswith("attn_vrow_kernel<1,2,"), last_kernel()
        assert torch.equal(ob[0], o[b]), b
    close(o, ref64(q, k, v, H, d ** -0.5, causal=causal), name=f"sdpa batch independence causal={causal}", kind=KIND[dtype])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("d", (24, 96, 160))
def test_waves_per_workgroup_change_no_bit(dev, d, dtype):
    """1, 2, 4 and 8 waves per workgroup (option ATTN_NW) on one problem, with and without the causal mask: the same bits."""
    B, H, T = 2, 2, 300
    q, k, v = inputs(B, T, T, H, d, dtype, seed=6)
    for causal in (False, True):
        outs = []
        for nw in (1, 2, 4, 8):
            with L.options(ATTN_NW=nw):
                outs.append(run(q, guarded_kv(k), guarded_kv(v), H, causal=causal))
                assert f",{nw}," in last_kernel(), last_kernel()
        assert all(torch.equal(outs[0], x) for x in outs[1:]), (d, causal)
        close(outs[0], ref64(q, k, v, H, d ** -0.5, causal=causal), name=f"sdpa nw d={d} causal={causal}", kind=KIND[dtype])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("d", (40, 64))
def test_value_ranges(dev, d, dtype):
    """Logits with max |scale q.k| about 80; keys that are all equal (uniform probabilities); one head whose V sits near the top of the
    16-bit range.  The PV accumulator is fp32 and un-normalised (sum_j p_j v_j with p_j <= 1, up to Tk terms), so the largest |V| that
    cannot overflow an intermediate is fp32_max / Tk: fp16's maximum qualifies as it is, for bf16 (whose maximum is fp32's) the head
    holds +-max / (2 Tk), i.e. 2^-9 of the range below the top.  Finite and within helpers.close in every case."""
    B, H, Tq, Tk = 2, 2, 129, 130
    C = H * d
    scale = d ** -0.5
    kind = KIND[dtype]
    q, k, v = inputs(B, Tq, Tk, H, d, dtype, seed=7)
    # (1) large logits
    s = torch.einsum("bqhd,bkhd->bhqk", q.double().view(B, Tq, H, d), k.double().view(B, Tk, H, d)) * scale
    qs = (q.double() * (80.0 / s.abs().max().item())).to(dtype)
    s2 = torch.einsum("bqhd,bkhd->bhqk", qs.double().view(B, Tq, H, d), k.double().view(B, Tk, H, d)) * scale
    assert 70 < s2.abs().max().item() < 90
    o = run(qs, guarded_kv(k), guarded_kv(v), H)
    close(o, ref64(qs, k, v, H, scale), name=f"sdpa values logits80 d={d}", kind=kind)
    # (2) all keys of batch 0 equal: every probability is 1 / Tk
    ke = k.clone(); ke[0] = k[0, :1]
    o = run(q, guarded_kv(ke), guarded_kv(v), H)
    close(o, ref64(q, ke, v, H, scale), name=f"sdpa values equal keys d={d}", kind=kind)
    # (3) head 0 of V near the 16-bit maximum (see the docstring); the heads are judged separately, each at its own magnitude
    top = torch.finfo(dtype).max if dtype == torch.float16 else torch.finfo(dtype).max / (2 * Tk)
    vb = v.clone()
    vb[:, :, :d] = (torch.sign(v[:, :, :d].float()) * top * 0.99).to(dtype)
    o = run(q, guarded_kv(k), guarded_kv(vb), H)
    assert torch.isfinite(o).all()
    ref = ref64(q, k, vb, H, scale)
    unit = 2.0 ** torch.tensor(float(top)).log2().floor().item()               # a power of two: the division is exact
    close((o[:, :, :d].double() / unit).float(), ref[:, :, :d] / unit, name=f"sdpa values big V head d={d}", kind=kind)
    close(o[:, :, d:], ref[:, :, d:], name=f"sdpa values other heads d={d}", kind=kind)


def test_batch_stride_past_4g(dev):
    """ONE allocation past 4 GiB, uninitialised except for the rows used; the batch stride puts batch 1 of Q, K, V and O beyond the 4 GiB
    mark (64-bit batch offsets).  Bits of the small-tensor run, and batch 1 against the reference."""
    B, H, d, T, dtype = 2, 2, 40, 130, torch.bfloat16
    C = H * d
    sB = 2 ** 31 + 64                                  # elements: batch 1 starts 4 GiB + 128 bytes after batch 0
    region = 16384                                     # >= T * C elements, a multiple of 8
    n = sB + 4 * region
    free = torch.cuda.mem_get_info()[0]
    if free < n * 2 + 2e9:
        pytest.skip(f"needs {(n * 2 + 2e9) / 1e9:.1f} GB of free device memory, {free / 1e9:.1f} GB free")
    assert T * C <= region and sB * 2 > 2 ** 32
    q, k, v = inputs(B, T, T, H, d, dtype, seed=8)
    buf = torch.empty(n, dtype=dtype, device="cuda")
    qs, ks, vs, os_ = (torch.as_strided(buf, (B, T, C), (sB, C, 1), i * region) for i in range(4))
    assert all(t[1].data_ptr() - buf.data_ptr() > 2 ** 32 for t in (qs, ks, vs, os_))
    qs.copy_(q); ks.copy_(k); vs.copy_(v); os_.fill_(NAN)
    run(qs, ks, vs, H, causal=True, o=os_)
    small = run(q, k, v, H, causal=True)
    assert torch.equal(os_, small)
    close(os_[1], ref64(q, k, v, H, d ** -0.5, causal=True)[1], name="sdpa past 4 GiB, batch 1", kind="bf16")
    del buf, qs, ks, vs, os_
    torch.cuda.empty_cache()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_program_executor(dev, dtype):
    """One MDX_OP_SDPA op through ops.run_ops and through mdx_program_run (a built program): same bits, right answer, in both builds."""
    B, H, d, Tq, Tk = 2, 3, 80, 33, 65
    q, k, v = inputs(B, Tq, Tk, H, d, dtype, seed=9)
    o = run(q, k, v, H)
    o2 = torch.full_like(q, NAN)
    op = O.Sdpa(q, k, v, o2, heads=H, scale=d ** -0.5)
    assert op.lower()[0] == L.OP_SDPA == 17 and O.dtype_code(op) == (L.DTYPE_F16 if dtype == torch.float16 else L.DTYPE_BF16)
    prog = O.build_program([op])
    prog.run(torch.cuda.current_stream().cuda_stream)
    assert last_kernel().startswith("attn_vrow_kernel<")
    torch.cuda.synchronize()
    assert torch.equal(o, o2)
    close(o2, ref64(q, k, v, H, d ** -0.5), name="sdpa program", kind=KIND[dtype])
