"""-m gpu: group_stats_kernel (csrc/stats.hip, mdx_group_stats_*, ops.GroupStats) against torch in float64.

Per group the kernel writes {nonfinite, absmax, sum, sumsq} of n contiguous elements.  Checked here:
  - nonfinite exact, absmax bit-exact, sum / sumsq within k(n) * 2^-24 * sum|x| (sum x^2) of the float64 value, k(n) = the longest addition
    chain the kernel states in its head comment (ops.GroupStats.chain_length): each input passes through at most k(n) - 1 rounded fp32
    additions (the first one, onto a zero accumulator, is exact), each of relative error <= 2^-24 — a derived bound, nothing measured;
  - NaN / +Inf / -Inf at element 0, at element n - 1, in the scalar tail, at one element of every thread's share;
  - dense groups (sG == n), padded groups, and a group start that has only the element's own alignment (the scalar path);
  - two launches give the same bits, a group alone gives the bits it has among seven, nothing behind the last group is read
    (it is NaN: a read would show in the count) and nothing around the records is written (sentinels);
  - the row select: the row index is read from device memory when a captured graph replays.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from magicdrive_amd import _lib as L  # noqa: E402
from magicdrive_amd import ops as O  # noqa: E402

NS = (1, 3, 4, 5, 7, 8, 9, 255, 256, 257, 1023, 1025, 5600)
GS = (1, 7)
T = 256
U = 2.0 ** -24
NAN, INF = float("nan"), float("inf")
SENT = -12345.5
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


def layout(G, n, mode, dtype, gen):
    """(buffer, X view [G, n]) of a mode: dense (sG = n, aligned base), padded (sG a multiple of 16 bytes past n), offset (base one element
    past an aligned address, sG = n).  Everything of the buffer outside the groups is NaN."""
    sG = n if mode != "padded" else (n + 15) // 16 * 16 + 16
    off = 1 if mode == "offset" else 0
    buf = torch.full((off + G * sG + 64,), NAN, dtype=dtype, device="cuda")
    X = torch.as_strided(buf, (G, n), (sG, 1), off)
    X.copy_((torch.randn(G, n, generator=gen, device="cuda") * 3.0).to(dtype))
    return buf, X


def placements(n, V):
    """name -> [(element index, value)] to plant in every group."""
    P = n // V
    vals = (NAN, INF, -INF)
    out = {"clean": [], "first": [(0, NAN)], "last": [(n - 1, INF)], "first+last": [(0, -INF), (n - 1, NAN)]}
    if n % V:
        out["tail"] = [(P * V + r, vals[r % 3]) for r in range(n % V)]
    if P:
        # one element of every thread's share: thread t owns pieces t, t + T, ...: take its LAST piece and element t % V of it
        share = []
        for t in range(min(P, T)):
            last = t + (P - 1 - t) // T * T
            share.append((last * V + t % V, vals[t % 3]))
        out["every_thread"] = share
    return out


def reference(X):
    """float64 {nonfinite, absmax, sum, sumsq, sum|x|} per group of X [G, n]."""
    x = X.double()
    fin = torch.isfinite(x)
    xz = torch.where(fin, x, torch.zeros_like(x))
    return (~fin).sum(1), xz.abs().amax(1), xz.sum(1), (xz * xz).sum(1), xz.abs().sum(1)


def run(X, out=None, row=None):
    if out is None:
        out = torch.full((X.shape[0], 4), SENT, dtype=torch.float32, device="cuda")
    O.run_ops([O.GroupStats(X, out, row=row)])
    return out


@pytest.mark.parametrize("mode", ["dense", "padded", "offset"])
@pytest.mark.parametrize("kind", ["fp32", "bf16", "fp16"])
def test_records_against_float64(dev, kind, mode):
    dtype = DTYPES[kind]
    f32 = dtype == torch.float32
    V = 4 if f32 else 8
    gen = torch.Generator(device="cuda").manual_seed(17)
    worst = 0.0
    kernels = set()
    for n in NS:
        k = O.GroupStats.chain_length(n, f32)
        for G in GS:
            for pname, plant in placements(n, V).items():
                buf, X = layout(G, n, mode, dtype, gen)
                if plant:
                    X[:, torch.tensor([i for i, _ in plant], device="cuda")] = torch.tensor([v for _, v in plant], device="cuda").to(dtype)
                guard = buf.clone()
                sent = torch.full((G + 2, 4), SENT, dtype=torch.float32, device="cuda")
                rec = sent[1:G + 1]
                run(X, rec)
                kernels.add((L.lib().mdx_last_kernel() or b"").decode())
                tag = f"{kind} {mode} n={n} G={G} {pname}"
                assert torch.equal(buf.view(torch.int16 if not f32 else torch.int32), guard.view(torch.int16 if not f32 else torch.int32)), tag
                assert (sent[0] == SENT).all() and (sent[-1] == SENT).all(), f"{tag}: a record was written outside [0, G)"
                bad, amax, s, q, sabs = reference(X)
                assert torch.equal(rec[:, 0].double(), bad.double()), f"{tag}: nonfinite {rec[:, 0].tolist()} != {bad.tolist()}"
                assert torch.equal(rec[:, 1].view(torch.int32), amax.float().view(torch.int32)), f"{tag}: absmax"
                es, eq = (rec[:, 2].double() - s).abs(), (rec[:, 3].double() - q).abs()
                assert (es <= k * U * sabs).all(), f"{tag}: sum off by {es.tolist()}, bound {(k * U * sabs).tolist()}"
                assert (eq <= k * U * q).all(), f"{tag}: sumsq off by {eq.tolist()}, bound {(k * U * q).tolist()}"
                worst = max(worst, float((es / (k * U * sabs).clamp_min(1e-300)).max()), float((eq / (k * U * q).clamp_min(1e-300)).max()))
                # the same launch again: same bits
                again = run(X)
                assert torch.equal(again.view(torch.int32), rec.view(torch.int32)), f"{tag}: two launches differ"
                # every group alone: the bits it has among G (whatever path its own alignment selects)
                if G > 1:
                    for g in range(G):
                        alone = run(X[g:g + 1])
                        assert torch.equal(alone.view(torch.int32), rec[g:g + 1].view(torch.int32)), f"{tag}: group {g} alone differs"
    print(f"group_stats {kind} {mode}: worst error / bound = {worst:.3f}, kernels {sorted(kernels)}")
    assert worst <= 1.0
    if mode == "offset":
        assert kernels == {"group_stats_kernel_scalar"}, kernels
    elif mode == "padded":
        assert kernels == {"group_stats_kernel"}, kernels


def test_all_nonfinite_and_zero_sizes(dev):
    """A group without a finite element: absmax, sum, sumsq are 0.  G == 0 / n == 0: nothing is launched, nothing written."""
    X = torch.full((2, 37), NAN, device="cuda")
    X[1, ::2] = -INF
    rec = run(X)
    assert rec.tolist() == [[37.0, 0.0, 0.0, 0.0], [37.0, 0.0, 0.0, 0.0]]
    out = torch.full((1, 4), SENT, device="cuda")
    d = L.MdxStatsDesc()
    d.X, d.out, d.G, d.n, d.sG, d.f32 = X.data_ptr(), out.data_ptr(), 0, 37, 37, 1
    L.call_op(L.OP_GROUP_STATS, d, torch.cuda.current_stream().cuda_stream)
    d.G, d.n = 1, 0
    L.call_op(L.OP_GROUP_STATS, d, torch.cuda.current_stream().cuda_stream)
    assert (out == SENT).all()


@pytest.mark.parametrize("kind", ["bf16", "fp16"])
def test_decoded_image_size(dev, kind):
    """One view of a decoded picture per group (224 * 400 * 3 16-bit elements: a thread walks 132 pieces), with one NaN in the last view."""
    dtype = DTYPES[kind]
    X = (torch.randn(6, 3, 224, 400, generator=torch.Generator(device="cuda").manual_seed(3), device="cuda") * 0.5).to(dtype)
    X[5, 2, 223, 399] = NAN
    rec = run(X)
    bad, amax, s, q, sabs = reference(X.reshape(6, -1))
    k = O.GroupStats.chain_length(3 * 224 * 400, False)
    assert rec[:, 0].tolist() == [0, 0, 0, 0, 0, 1]
    assert torch.equal(rec[:, 1].view(torch.int32), amax.float().view(torch.int32))
    assert ((rec[:, 2].double() - s).abs() <= k * U * sabs).all() and ((rec[:, 3].double() - q).abs() <= k * U * q).all()


def test_row_select_in_a_replayed_graph(dev):
    """[counter increment, GroupStats] captured once and replayed n_rows + 2 times: rows 0 .. n_rows - 1 are filled in order, the two extra replays
    (rows n_rows and n_rows + 1) write nothing.  The increment is the library's own: the scheduler op advances its step counter behind its update
    (a counter of -1 is its documented "no such step" input: it poisons its 8 dummy latents and still advances)."""
    n_rows, G, n = 5, 3, 100
    ctr = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    x = torch.zeros(8, device="cuda"); eps = torch.zeros(8, device="cuda")
    coef = torch.ones(n_rows + 2, 4, device="cuda")
    src = torch.zeros(G, n, device="cuda")
    store = torch.full((n_rows + 2, G, 4), SENT, device="cuda")        # the table is rows 1 .. n_rows of this; a sentinel row on either side
    table = store[1:n_rows + 1]
    prog = O.build_program([O.DdimStep(x, eps, coef, ctr), O.GroupStats(src, table, row=ctr)])
    prog.capture()
    st = torch.cuda.current_stream().cuda_stream
    snaps = []
    for r in range(n_rows + 2):
        src.fill_(float(r + 1)); src[:, 0] = -float(10 * (r + 1))        # stream-ordered with the replays: replay r sees the value r + 1
        prog.launch(st)
        snaps.append(store.clone())
    torch.cuda.synchronize()
    prog.destroy()
    assert ctr.item() == n_rows + 1
    for r in range(n_rows + 2):
        for row in range(n_rows):
            if row <= r:
                v = float(row + 1)
                want = [0.0, 10 * v, (n - 1) * v - 10 * v, (n - 1) * v * v + 100 * v * v]
                assert snaps[r][1 + row].tolist() == [want] * G, (r, row)
            else:
                assert (snaps[r][1 + row] == SENT).all(), (r, row)
        assert (snaps[r][0] == SENT).all() and (snaps[r][-1] == SENT).all(), r
    assert torch.equal(snaps[-1], snaps[n_rows - 1]) and torch.equal(snaps[-2], snaps[n_rows - 1])
