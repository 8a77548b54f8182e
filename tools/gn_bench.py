#!/usr/bin/env python
"""Per-site A/B of the register-resident GroupNorm (ops.GroupNormResident, gn_resident_kernel) against the default op (two streaming
stages) on ONE library in ONE process, repetitions interleaved.

Sites = every distinct GroupNorm of the SD-1.5 224x400 step program (shapes, strides and SiLU flag read from a shape-only plan built on
the CPU, with how often each occurs per step), at 576 views (one stream, 96 scenes) and 192 views (what bench.py runs: two streams x 32
scenes).  Before every timed launch a copy writes the input tensor in ascending order, as the producing conv does, so both variants meet
the cache state they meet in the step program.  The resident op is timed at the k of csrc/gn_route.h and, with --sweep-k, at every narrower
k the kernel can run.  Prints a table; --out writes it as JSON (per site: median / min / max us of each variant; the sums over the sites the
rule routes to the resident op, weighted by their count per step).

Usage: python tools/gn_bench.py [--views 576 192] [--reps 7] [--sweep-k] [--out profiles/gn_resident_ab.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from magicdrive_amd import _lib as L, denoiser as DN, gn_route as GR, ops as O  # noqa: E402
from magicdrive_amd.engine import PackedNet  # noqa: E402
from magicdrive_amd.networks import spec  # noqa: E402

BF = torch.bfloat16


class ShapeNet(PackedNet):
    def _get(self, tag, keys, fn):
        ck = (tag,) + tuple(keys)
        if ck not in self.cache:
            self.cache[ck] = fn(*[torch.zeros(self.sd[k].shape) for k in keys])
        return self.cache[ck]


def sites():
    """[(HW, C, G, ldx, ldy, silu, eps, count per step)] of the 224x400 step program."""
    cfg = spec.SD15_CONFIG
    cpu = torch.device("cpu")
    z = lambda shapes: {k: torch.zeros(1).expand(s) for k, s in shapes.items()}
    sp = DN.SamplerPlan(cfg, ShapeNet(z(spec.unet_param_shapes(cfg)), cpu), ShapeNet(z(spec.controlnet_param_shapes(cfg)), cpu), cpu, 1, False, 32, (28, 50), num_steps=50)
    out = {}
    for op in sp.step_ops:
        if isinstance(op, O.GroupNorm):
            key = (op.X.shape[1], op.X.shape[2], op.groups, op.X.stride(1), op.Y.stride(1), bool(op.silu), float(op.eps))
            out[key] = out.get(key, 0) + 1
    return [k + (n,) for k, n in sorted(out.items(), key=lambda kv: (-kv[0][0], kv[0][1], kv[0][3]))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, nargs="+", default=[576, 192])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sweep-k", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda")
    ws = torch.empty(64 * 1024 * 1024 // 4, dtype=torch.float32, device=dev)
    floor = L.get_option("GN_ONE_KERNEL_ELEMS")
    rows = []
    for B in a.views:
        for (HW, C, G, ldx, ldy, silu, eps, count) in sites():
            g = torch.Generator().manual_seed(HW + C)
            src = (torch.randn(HW, ldx, generator=g) * 2 + 0.7).to(BF).to(dev).expand(B, HW, ldx)
            xbuf = torch.empty(B, HW, ldx, dtype=BF, device=dev)
            ybuf = torch.empty(B, HW, ldy, dtype=BF, device=dev)
            x, y = xbuf[:, :, ldx - C:], ybuf[:, :, :C]
            gam = torch.randn(C, generator=g).to(dev); bet = torch.randn(C, generator=g).to(dev)
            k_rule = GR.gn_resident_plan(B, HW, C, G, ldx, ldy, 16, floor)
            k_any = GR.gn_resident_plan(B, HW, C, G, ldx, ldy, 16, 0)
            variants = [("two_stage", O.GroupNorm(x, y, gam, bet, G, eps, silu, ws=ws), {})]
            ks = [k_any] if k_any else []
            if a.sweep_k and k_any:
                ks += [k for k in range(k_any - 1, 0, -1) if GR.gn_resident_nv(HW, C, G, k)][:2]
            for k in ks:
                variants.append((f"resident_k{k}", O.GroupNormResident(x, y, gam, bet, G, eps, silu), {"GN_RESIDENT": 2, "GN_RESIDENT_K": k}))
            times = {n: [] for n, _, _ in variants}
            tags = {}
            for rep in range(a.reps + 1):                      # repetition 0 warms up
                for name, op, opts in variants:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    xbuf.copy_(src)                            # the producer: writes the tensor front to back
                    with L.options(**opts):
                        e0.record(); O.run_ops([op]); e1.record()
                        tags[name] = (L.lib().mdx_last_kernel() or b"").decode()
                    torch.cuda.synchronize()
                    if rep:
                        times[name].append(e0.elapsed_time(e1) * 1e3)
            row = {"views": B, "HW": HW, "C": C, "ldx": ldx, "ldy": ldy, "silu": silu, "count": count, "k_rule": k_rule, "k_widest": k_any,
                   "bytes": 2 * B * HW * C * 2, "variants": {}}
            for name, _, _ in variants:
                t = times[name]
                row["variants"][name] = {"kernel": tags[name], "median_us": round(statistics.median(t), 1), "min_us": round(min(t), 1), "max_us": round(max(t), 1)}
            rows.append(row)
            line = "  ".join(f"{n} {v['median_us']:8.1f} [{v['min_us']:.1f}, {v['max_us']:.1f}]" for n, v in row["variants"].items())
            print(f"views {B:4d}  {HW:5d} px  C {C:5d} (ld {ldx}/{ldy}) x{count:2d}  rule k={k_rule:2d}  {line}", flush=True)
            del src, xbuf, ybuf, x, y
    summary = {}
    for B in a.views:
        two = res = two_lo = two_hi = res_lo = res_hi = 0.0
        n = 0
        for r in rows:
            if r["views"] != B or not r["k_rule"]:
                continue
            v2, vr = r["variants"]["two_stage"], r["variants"][f"resident_k{r['k_widest']}"]
            two += r["count"] * v2["median_us"]; res += r["count"] * vr["median_us"]
            two_lo += r["count"] * v2["min_us"]; two_hi += r["count"] * v2["max_us"]
            res_lo += r["count"] * vr["min_us"]; res_hi += r["count"] * vr["max_us"]
            n += r["count"]
        summary[str(B)] = {"routed_ops_per_step": n, "two_stage_us": round(two, 1), "two_stage_range_us": [round(two_lo, 1), round(two_hi, 1)],
                           "resident_us": round(res, 1), "resident_range_us": [round(res_lo, 1), round(res_hi, 1)]}
        print(f"views {B}: {n} routed ops per step: two-stage {two:.1f} us [{two_lo:.1f}, {two_hi:.1f}]  resident {res:.1f} us [{res_lo:.1f}, {res_hi:.1f}]")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"build_id": L.build_id(), "reps": a.reps, "sites": rows, "summary": summary}, f, indent=1)


if __name__ == "__main__":
    main()
