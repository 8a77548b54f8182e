"""q/k/v projection + self-attention of one transformer block, two lowerings, timed per part on one GPU in one process.

  (a) today's lowering, as engine.Builder.self_like_attention emits it:
        levels 1-3: `.qk` GEMM [M, C] -> [M, 2C]  +  batched `.vT` GEMM (W_v as the A operand) -> V^T [B, C, roundup8(T)]  +  ops.Attn
        level 0   : the fused q/k/v launch of gemm_ws.hip with the V columns stored transposed  +  ops.Attn (attention2.hip at d = 40)
      Q carries scale * log2(e) (q_prescaled), as in the engine.
  (b) one plain [M, 3C] projection  +  ops.Sdpa on its three column blocks (csrc/attention_vrow.hip reads V row-major, in place).

Report only: nothing is gated on the numbers.  Every part is a program of its own; a timed sample is `--inner` back-to-back runs of one
part between two device events (the kernels are 10 us .. 10 ms: one sample is long enough to time), the parts of both lowerings are
interleaved in every round, and the median, minimum and maximum of the rounds are reported per part together with the kernel that ran.
The outputs of the two lowerings are compared once per shape (rel-L2), so a fast wrong answer cannot go unnoticed.

    python tools/sdpa_bench.py [--views 576] [--rounds 9] [--inner 10] [--dtype bf16|f16] [--out profiles/sdpa_bench.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(1400, 320, 8), (350, 640, 8), (91, 1280, 8), (28, 1280, 8)]      # (T, C, heads): the four levels of the denoiser
LOG2E = 1.4426950408889634


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=576)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--dtype", choices=["bf16", "f16"], default="bf16")
    ap.add_argument("--out", default=None, help="append one JSON line per shape to this file (also printed)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sdpa_bench: no GPU visible; this tool measures on the MI355X only")
    from magicdrive_amd import _lib as L
    from magicdrive_amd import flops as FL
    from magicdrive_amd import ops as O
    from magicdrive_amd import packing as PK
    from magicdrive_amd.engine import Builder

    dev = torch.device("cuda:0")
    dtype = torch.bfloat16 if a.dtype == "bf16" else torch.float16
    ws = torch.empty(64 * 1024 * 1024 // 4, dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    B = a.views
    lines = []
    for T, C, heads in SHAPES:
        d = C // heads
        M = B * T
        g = torch.Generator(device=dev).manual_seed(T)
        x = torch.randn(M, C, generator=g, device=dev).to(dtype)
        w = (torch.randn(3 * C, C, generator=g, device=dev) * C ** -0.5)
        w_pre = w.clone(); w_pre[:C] *= d ** -0.5 * LOG2E                        # (a): to_q carries scale * log2(e)
        w, w_pre = w.to(dtype), w_pre.to(dtype)
        fused = Builder.fuses_qkv(B, T, C)
        # ---- (a) ----
        qk = torch.empty(M, 2 * C, dtype=dtype, device=dev)
        vt = torch.zeros(B, C, PK.round_up(T, 8), dtype=dtype, device=dev)
        oa = torch.empty(B, T, C, dtype=dtype, device=dev)
        if fused:
            gemm_a = [O.Gemm(x, w_pre, qk, Vt=vt, vt_from=2 * C, vt_T=T, ws=ws, name="qkv")]
        else:
            gemm_a = [O.Gemm(x, w_pre[:2 * C], qk, ws=ws, name="qk"), O.Gemm(w_pre[2 * C:], x.view(B, T, C), vt[:, :, :T], name="vT")]
        qk3 = qk.view(B, T, 2 * C)
        attn_a = [O.Attn(qk3[:, :, :C], qk3[:, :, C:], vt, oa, heads=heads, Tk=T, scale=d ** -0.5, q_prescaled=True, name="attn")]
        # ---- (b) ----
        qkv = torch.empty(M, 3 * C, dtype=dtype, device=dev)
        ob = torch.empty(B, T, C, dtype=dtype, device=dev)
        gemm_b = [O.Gemm(x, w, qkv, ws=ws, name="qkv_plain")]
        q3 = qkv.view(B, T, 3 * C)
        attn_b = [O.Sdpa(q3[:, :, :C], q3[:, :, C:2 * C], q3[:, :, 2 * C:], ob, heads=heads, scale=d ** -0.5, name="sdpa")]
        parts = {"a_gemm": gemm_a, "a_attn": attn_a, "b_gemm": gemm_b, "b_attn": attn_b}
        progs = {k: O.build_program(v) for k, v in parts.items()}
        kernels = {}
        for k, ops_ in parts.items():                       # warm-up, one op at a time: code objects, and the kernel each op reaches
            names = []
            for op in ops_:
                O.run_ops([op])
                names.append((L.lib().mdx_last_kernel() or b"").decode())
            kernels[k] = names
        for k in progs:
            for _ in range(3):
                progs[k].run(stream)
        torch.cuda.synchronize()
        rel = ((ob.float() - oa.float()).norm() / oa.float().norm()).item()
        times = {k: [] for k in progs}
        for _ in range(a.rounds):
            for k, p in progs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _i in range(a.inner):
                    p.run(stream)
                e1.record(); torch.cuda.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3 / a.inner)
        stat = lambda v: {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}
        rec = {"bench": "sdpa", "views": B, "T": T, "C": C, "heads": heads, "d": d, "dtype": a.dtype, "rounds": a.rounds, "inner": a.inner,
               "build": L.build_id(), "a_form": "fused qkv + transposed V store" if fused else "qk GEMM + vT GEMM",
               "rel_l2_b_vs_a": round(rel, 6), "attn_gflop": round(FL.op_flops(attn_b[0]) / 1e9, 3)}
        for k in progs:
            rec[k] = dict(stat(times[k]), kernels=kernels[k])
        tot = {s: [times[s + "_gemm"][i] + times[s + "_attn"][i] for i in range(a.rounds)] for s in "ab"}
        rec["a_total"], rec["b_total"] = stat(tot["a"]), stat(tot["b"])
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
        del x, qk, vt, oa, qkv, ob, progs, parts
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
