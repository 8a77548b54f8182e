#!/usr/bin/env python
"""Folded upsample conv (MdxConvDesc.upsample2x) against the pair it replaces (nearest resize + 3x3 conv): per-op medians at the headline's
576 views (UNet decoder stages) and at 48 images (VAE upsamplers), with the library's own tile width and both forced ones.
Usage: python tools/upfold_bench.py [out.json]   (profiles/r07_upsample_fold_ops.json was written by it)"""
import os, sys, json, statistics
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from magicdrive_amd import _lib as L, ops as O, packing as PK
BF = torch.bfloat16
dev = torch.device("cuda")
ws = torch.empty(64 * 1024 * 1024 // 4, dtype=torch.float32, device=dev)
st = torch.cuda.current_stream().cuda_stream

def timeit(ops, reps=15):
    low = [op.lower() for op in ops]
    for _ in range(3):
        for c, d in low: L.call_op(c, d, st)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a = torch.cuda.Event(enable_timing=True); b = torch.cuda.Event(enable_timing=True)
        a.record()
        for c, d in low: L.call_op(c, d, st)
        b.record(); b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)

out = {}
for name, B, lo, hi, C in [("u0", 576, (4, 7), (7, 13), 1280), ("u1", 576, (7, 13), (14, 25), 1280), ("u2", 576, (14, 25), (28, 50), 640),
                           ("vae.up0", 48, (28, 50), (56, 100), 512), ("vae.up1", 48, (56, 100), (112, 200), 512), ("vae.up2", 48, (112, 200), (224, 400), 256)]:
    x = (torch.randn(B, *lo, C, device=dev) * 0.5).to(BF)
    w = torch.randn(C, C, 3, 3) * (9 * C) ** -0.5
    bias = torch.randn(C, device=dev)
    up = torch.empty(B, *hi, C, dtype=BF, device=dev)
    y = torch.empty(B, *hi, C, dtype=BF, device=dev)
    pair = [O.Upsample(x, up, PK.nearest_index(lo[0], hi[0]).to(dev), PK.nearest_index(lo[1], hi[1]).to(dev)),
            O.Conv(up, PK.pack_conv_weight(w, BF).to(dev), y, bias=bias, ws=ws)]
    t_pair = timeit(pair); t_conv = timeit(pair[1:])
    k_pair = (L.lib().mdx_last_kernel() or b"").decode()
    fold = O.Conv(x, PK.fold_upsample_conv(w, hi[0] != 2 * lo[0], hi[1] != 2 * lo[1], BF).to(dev), y, bias=bias, ws=ws, upsample2x=True)
    r = {"pair_ms": t_pair, "conv_only_ms": t_conv, "pair_kernel": k_pair}
    for bn in (0, 256, 320):
        with L.options(XL_BN=bn):
            r[f"fold_bn{bn}_ms"] = timeit([fold])
            if bn == 0: r["fold_kernel"] = (L.lib().mdx_last_kernel() or b"").decode()
    r["speedup_default"] = t_pair / r["fold_bn0_ms"]
    gf = 2.0 * B * hi[0] * hi[1] * C * C
    r["fold_exec_tflops"] = gf * 4 / r["fold_bn0_ms"] / 1e9
    r["pair_tflops"] = gf * 9 / t_conv / 1e9
    out[name] = r
    print(name, json.dumps(r), flush=True)
    del x, up, y
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
