"""Time of the SD-1.5-size CLIP text encoder on the library (magicdrive_amd.networks.clip_text, one captured graph) and — where transformers
is importable — of transformers' CLIPTextModel on torch's kernels with the same weights, interleaved in one process (rounds of both, median
and min reported).  Report only; prints one JSON line.

    python tools/clip_text_bench.py [--prompts 384] [--rounds 7] [--dtype bf16|f16]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prompts", type=int, default=384)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--dtype", choices=["bf16", "f16"], default="bf16")
    a = ap.parse_args()
    from magicdrive_amd import _lib as L
    from magicdrive_amd.networks.clip_text import CLIP_SD15_CONFIG, CLIPTextModel
    dev = torch.device("cuda:0")
    dtype = torch.bfloat16 if a.dtype == "bf16" else torch.float16
    hip = CLIPTextModel.from_config({}, seed=3, torch_dtype=dtype).to(dev)
    ids = torch.randint(0, 49408, (a.prompts, 77), generator=torch.Generator().manual_seed(5)).to(dev)
    arms = {"hip_graph": lambda: hip(ids)[0]}
    try:
        import transformers
        cfg = transformers.CLIPTextConfig(**{k: v for k, v in CLIP_SD15_CONFIG.items()})
        ref = transformers.CLIPTextModel(cfg).eval()
        ref.load_state_dict(hip.state_dict(), strict=False)
        ref = ref.to(dev, dtype)
        arms["transformers_torch"] = lambda: ref(input_ids=ids)[0]
    except ImportError:
        pass
    times = {k: [] for k in arms}
    with torch.no_grad():
        for fn in arms.values():           # warm-up: plan + graph capture, torch's kernel selection
            fn(); fn()
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for k, fn in arms.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); fn(); e1.record(); torch.cuda.synchronize()
                times[k].append(e0.elapsed_time(e1))
        out = {k: arms[k]().float() for k in arms}
    res = {"bench": "clip_text", "prompts": a.prompts, "tokens": 77, "dtype": a.dtype, "rounds": a.rounds, "build": L.build_id(),
           **{k + "_ms_median": round(statistics.median(v), 3) for k, v in times.items()}, **{k + "_ms_min": round(min(v), 3) for k, v in times.items()}}
    if "transformers_torch" in out:
        res["rel_l2_hip_vs_torch"] = round(((out["hip_graph"] - out["transformers_torch"]).norm() / out["transformers_torch"].norm()).item(), 5)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
