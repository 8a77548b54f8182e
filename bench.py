#!/usr/bin/env python
"""bench.py — headline benchmark of the MI355X-native MagicDrive sampler hot path.

Metric (BASELINE.json): 6-view scenes/sec at 224x400, 50-step DDIM, on 1/2/4/8 MI355X.
Workload at every N: BASELINE.json configs[1] — "6-view 224x400, text-only conditioning, 50-step DDIM, bf16":
the reference's own degenerate mode `camera_param=None` (learned unconditional camera for all six views,
CFG forced off: pipeline_bev_controlnet.py:260-264), no boxes, zero BEV map; SD-1.5-sized multi-view UNet +
BEV-ControlNet with seeded random weights (no checkpoints exist offline), synthetic prompt embeddings.
One bench "step" = one complete `pipe(...)` call: conditioning prologue + 50 denoising steps for
`--scenes-per-gpu` scenes per rank, inputs resident in HBM, output_type="latent" (VAE decode and CLIP are
outside the built hot path).  Weak scaling: every rank samples its own scenes; the only
collective is the final all_gather of the result latents (RCCL), inside the timed region.

Launch: `python bench.py` (1 GPU), `python bench.py --gpus N` (re-executes itself under torch.distributed.run with N ranks), or
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...
A plain run sets up, warms up, times --steps calls and prints one JSON line (metric, value, unit, ms_per_step, ...).  `--full` adds
what is measured beside the headline after the timed region (batch consistency, 1-scene latency, configs[2] / configs[3], VAE decode,
per-op profile + roofline, CPU baseline); `--dump-outputs DIR` writes the last timed call's latents for output-by-output comparison.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

MFMA_BF16_PEAK_TFLOPS = 2500.0     # dense bf16 MFMA peak, /opt/skills/guides/MI355X_MICROARCH.md "Peak BF16/FP16 MFMA"


def build_pipeline(cfg, device, scheduler="ddim", torch_dtype=torch.bfloat16):
    from magicdrive_amd import schedulers
    from magicdrive_amd.networks.unet_2d_condition_multiview import UNet2DConditionModelMultiview
    from magicdrive_amd.networks.unet_addon_rawbox import BEVControlNetModel
    from magicdrive_amd.pipeline.pipeline_bev_controlnet import StableDiffusionBEVControlNetPipeline
    unet = UNet2DConditionModelMultiview.from_config(cfg, seed=0, torch_dtype=torch_dtype)
    cn = BEVControlNetModel.from_config(cfg, seed=1, torch_dtype=torch_dtype)
    pipe = StableDiffusionBEVControlNetPipeline(unet=unet, controlnet=cn, scheduler=schedulers.DDIMScheduler() if scheduler == "ddim" else schedulers.UniPCMultistepScheduler())
    return pipe.to(device), unet, cn


def pmc_traffic(kernel_name, avg_us=None):
    """Counter-derived numbers of ONE launch of `kernel_name` from the committed rocprofv3 --pmc passes (profiles/r03_pmc_summary.json,
    collected at the bench batch of 768 views by tools/pmc_collect.sh: HBM-side bytes = FETCH_SIZE x 2 per the gfx950 correction of
    MI355X_MICROARCH.md + WRITE_SIZE, hbm_gbps = those bytes / the profiled duration, mfma_util = SQ_VALU_MFMA_BUSY_CYCLES /
    (GRBM_GUI_ACTIVE x 1024 SIMDs); separate passes).  Counters cannot be collected inside a timed run; the summary records the shape
    it was measured on next to the algorithmic bytes of that launch."""
    summ = pmc_summary()
    if summ is None:
        return None
    rows = summ.get("kernels", {})
    for k, v in rows.items():
        if kernel_name.startswith(k):
            cases = v.get("cases") or [v]
            if "views" in _PMC:                 # nor counters of another batch: only cases profiled at the views of the plan timed here
                cases = [c for c in cases if c.get("views") == _PMC["views"]]
                if not cases:
                    return None
            if avg_us is not None:      # several shapes of this kernel were profiled: report the one closest to the timed run's average launch
                cases = sorted(cases, key=lambda c: abs((c.get("avg_us_profiled") or 0.0) - avg_us))
            best = dict(cases[0])
            best["profiled_cases"] = [c.get("case") for c in (v.get("cases") or [v])]
            return best
    return None


_PMC = {}


def pmc_summary():
    """The newest committed counter summary whose `build_id` equals the loaded library's (mdx_build_id: a hash of the kernel sources).
    Counters of another build are NOT reported next to this run's timings: `pmc_status` in the JSON line says which
    file was used or why none was."""
    if "summ" in _PMC:
        return _PMC["summ"]
    from magicdrive_amd import _lib as L
    bid = L.build_id()
    _PMC["summ"], _PMC["status"] = None, f"no profiles/r*_pmc_summary.json for build {bid}"
    import glob
    for p in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_summary.json")), reverse=True):
        try:
            with open(p) as f:
                d = json.load(f)
        except Exception:
            continue
        if d.get("build_id") == bid:
            _PMC["summ"], _PMC["status"] = d, f"{os.path.basename(p)} (build {bid})"
            break
        _PMC["status"] = f"{os.path.basename(p)} is of build {d.get('build_id')}, library is {bid}: counters dropped"
    return _PMC["summ"]


def per_op_profile(plan, reps=5):
    """HIP-event timing of every launch of the step program on the stream it is launched on."""
    from magicdrive_amd import _lib as L, flops as FL
    st = torch.cuda.current_stream().cuda_stream
    from magicdrive_amd import ops as O_
    lowered = [O_.lower_with_dtype(op) for op in plan.step_ops]
    n = len(lowered)
    best = [float("inf")] * n
    samples = [[] for _ in range(n)]
    kname = [""] * n
    last_kernel = L.lib().mdx_last_kernel
    for _ in range(reps):
        plan.step_ctr.zero_()
        evs = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
        evs[0].record()
        for i, (code, desc, dt) in enumerate(lowered):
            L.call_op(code, desc, st, dt)
            kname[i] = (last_kernel() or b"").decode()          # which kernel the library routed this op to
            evs[i + 1].record()
        torch.cuda.synchronize()
        for i in range(n):
            ms = evs[i].elapsed_time(evs[i + 1])
            best[i] = min(best[i], ms)
            samples[i].append(ms)
    med = [sorted(v)[len(v) // 2] for v in samples]
    fam, kern = {}, {}
    rows = []
    # `ms` = the MEDIAN of `reps` repetitions (what the per-kernel / per-family rates are computed from); `ms_best` = the fastest one
    for op, ms, mb, kn in zip(plan.step_ops, med, best, kname):
        k = FL.kernel_family(op)
        for d, key in ((fam, k), (kern, kn)):
            f = d.setdefault(key, {"ms": 0.0, "ms_best": 0.0, "flops": 0.0, "bytes": 0.0, "launches": 0, "mfma": k.startswith(("gemm_conv", "attn"))})
            f["ms"] += ms; f["ms_best"] += mb; f["flops"] += FL.op_flops(op); f["bytes"] += FL.op_bytes(op); f["launches"] += 1
        rows.append({"name": getattr(op, "name", ""), "family": k, "kernel": kn, "ms": ms, "ms_best": mb, "gflop": FL.op_flops(op) / 1e9})
    return fam, kern, rows


def cpu_cfg1(cfg, cores, steps=20):
    """BASELINE.json configs[0] in full: ONE 224x400 view through the vanilla SD-1.5 UNet (no ControlNet, no cross-view attention:
    the multi-view state dict minus its attn4 / norm4 / connector tensors), 20-step DDIM, on the CPU oracle."""
    from magicdrive_amd.networks import spec
    from oracle import denoiser as D
    usd = {k: v for k, v in spec.random_state_dict(spec.unet_param_shapes(cfg), 0).items()
           if ".attn4." not in k and ".norm4." not in k and ".connector." not in k}
    g = torch.Generator().manual_seed(1234)
    x = torch.randn(1, 4, 28, 50, generator=g)
    ehs = torch.randn(1, 77, cfg["cross_attention_dim"], generator=g)
    sch = D.DDIM()
    t0 = time.perf_counter()
    with torch.no_grad():
        for t in sch.set_timesteps(steps).tolist():
            x = sch.step(D.unet_forward(usd, cfg, x, t, ehs), t, x)
    dt = time.perf_counter() - t0
    assert torch.isfinite(x).all()
    return {"seconds": round(dt, 2), "views_per_s": round(1.0 / dt, 4), "steps": steps, "cores": cores,
            "what": "configs[0]: single 224x400 view, vanilla SD-1.5 UNet, 20-step DDIM, CPU oracle fp32, run in full"}


def cpu_baseline(cfg, n_steps_timed=3):
    """The CPU oracle (restatement of the reference's diffusers path, fp32) on this host's cores: one warm-up
    denoise step + `n_steps_timed` timed steps of ONE scene of the same workload, extrapolated to 50 steps."""
    from magicdrive_amd import synthetic
    from magicdrive_amd.networks import spec
    from oracle import denoiser as D
    usd = spec.random_state_dict(spec.unet_param_shapes(cfg), 0)
    csd = spec.random_state_dict(spec.controlnet_param_shapes(cfg), 1)
    sc = synthetic.make_scene_batch(1, ctx_dim=cfg["cross_attention_dim"], max_len=None, zero_map=True)
    n_cam = len(cfg["neighboring_view_pair"])
    lat = torch.stack([sc["latents"]] * n_cam, 1)
    cam = D.uncond_cam_param(csd, 1, n_cam)
    # Thread count: measured on the GPU box's host (2 x EPYC 9575F, container-limited): 16 threads 3.7 s per UNet pass,
    # 32 -> 5.5 s, 64 -> 10 s, 128 -> 20 s (oversubscription) — so the baseline uses the fastest setting, 16.
    prev_threads = torch.get_num_threads()
    cores = min(16, prev_threads)
    torch.set_num_threads(cores)

    def one_step(t):
        with torch.no_grad():
            d, m, ctx = D.controlnet_forward(csd, cfg, lat, torch.tensor([t]), cam, None, sc["prompt_embeds"], sc["bev_map"])
            return D.unet_forward(usd, cfg, lat.reshape(-1, *lat.shape[2:]), t, ctx, d, m)
    one_step(981)
    t0 = time.perf_counter()
    for i in range(n_steps_timed):
        one_step(961 - 20 * i)
    dt = (time.perf_counter() - t0) / n_steps_timed
    cfg1 = cpu_cfg1(cfg, cores)
    # The REAL reference (BEVControlNetModel.forward + UNet2DConditionModelMultiview.forward through the vendored diffusers, fp32) on THIS
    # host's cores, same scene / weights / threads / step count — when /root/reference is importable here (oracle/refshim.py).  It is not on
    # the GPU box: there the number beside the GPU line stays the port's, and `reference_on_this_host` says so.
    ref_dt = None
    try:
        if os.path.isdir("/root/reference"):
            from oracle import ref_models
            _, r_unet, r_cnet = ref_models.build_reference(cfg, usd, csd)

            def ref_step(t):
                tt = torch.tensor([t])
                with torch.no_grad():
                    d, m, ctx = r_cnet(lat, tt, cam, None, sc["prompt_embeds"], sc["bev_map"], return_dict=False)
                    return r_unet(lat.reshape(-1, *lat.shape[2:]), tt.repeat_interleave(n_cam), encoder_hidden_states=ctx,
                                  down_block_additional_residuals=d, mid_block_additional_residual=m).sample
            ref_step(981)
            t0 = time.perf_counter()
            for i in range(n_steps_timed):
                ref_step(961 - 20 * i)
            ref_dt = (time.perf_counter() - t0) / n_steps_timed
    except Exception as e:                                       # an unimportable reference is not a bench failure
        ref_dt = None
        sys.stderr.write(f"cpu_baseline: reference not timed ({type(e).__name__}: {e})\n")
    torch.set_num_threads(prev_threads)
    use = ref_dt if ref_dt is not None else dt
    out = {"value": 1.0 / (50 * use), "unit": "scenes/s", "cores": cores, "kind": "reference" if ref_dt is not None else "port",
           "reference_on_this_host": ref_dt is not None,
           "sample": f"1 scene, text-only config, {n_steps_timed} timed denoise steps after 1 warm-up ({use:.2f} s/step, torch {torch.__version__} fp32), extrapolated x50",
           "port_s_per_step": round(dt, 3), "reference_s_per_step": None if ref_dt is None else round(ref_dt, 3),
           "cfg1_single_view_20step": cfg1}
    # The REAL reference (diffusers path imported from /root/reference, which does not exist on the GPU box) is timed beside this port in
    # the authoring container by `tools/make_golden.py cpuref`, same threads, same scene; the committed log is quoted verbatim (a fixed
    # external measurement, NOT a number of this run: no scenes/s is derived from it here).
    rp = os.path.join(ROOT, "profiles", "r04_cpu_reference_vs_port.json")
    if os.path.exists(rp):
        with open(rp) as f:
            rvp = json.load(f)
        out["reference_vs_port_authoring_container"] = dict(rvp, source="profiles/r04_cpu_reference_vs_port.json")
        ratio = rvp.get("reference_over_port") or (rvp["port_s_per_step"] / rvp["reference_s_per_step"] if rvp.get("reference_s_per_step") else None)
        if ratio and ref_dt is None:
            # DERIVED, not measured here: this host's port rate x the reference / port speed ratio measured once in the authoring container
            # (same threads, scene and weights) — what the real reference would do on these cores if the ratio carries over
            out["reference_estimate_scenes_per_s"] = {"value": round(out["value"] * ratio, 6), "derived": True,
                                                      "how": f"port value x {ratio:.3f} (reference / port speed ratio of profiles/r04_cpu_reference_vs_port.json, authoring container)"}
    return out


DUMP_BUDGET_BYTES = 60_000_000       # the dump stays under 64 MB (10^6 bytes), .npy header included


def dump_latents(out_dir, latents):
    """--dump-outputs: the [scenes, ...] result as `out_dir/latents.npy` in float32.  Past DUMP_BUDGET_BYTES a fixed seeded sample of
    scenes (in scene order), so that two runs with the same arguments dump the same rows."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    n, per_scene = latents.shape[0], latents[0].numel() * 4
    if n * per_scene > DUMP_BUDGET_BYTES:
        keep = torch.randperm(n, generator=torch.Generator().manual_seed(0))[:max(1, DUMP_BUDGET_BYTES // per_scene)].sort().values
        latents = latents[keep.to(latents.device)]
    np.save(os.path.join(out_dir, "latents.npy"), latents.detach().float().cpu().numpy())


def launcher_command(gpus, argv, port):
    """`python bench.py --gpus N` without a launcher becomes this command: one rank per GPU under torch.distributed.run, same flags."""
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={gpus}", "--master-addr", "127.0.0.1",
            "--master-port", str(port), os.path.abspath(__file__)] + list(argv)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--scenes-per-gpu", type=int, default=64,
                    help="scenes sampled per rank per pipe() call = one timed step (throughput grows with the batch — fewer partial rounds of tiles: "
                         "5.41 / 6.94 / 7.46 / 7.49 / 7.70 scenes/s at 8 / 32 / 64 / 96 / 192, profiles/r07_bench_batch_sizes.log).  64 keeps a step at "
                         "8.6 s, 3.1 %% below the 192-scene rate, so that a run of 25 steps takes 4 minutes, not 10.5; 192 is the batch of the round 1-6 "
                         "records (tools/gpu_evidence.sh passes it)")
    ap.add_argument("--streams", type=int, default=0,
                    help="HIP streams a pipe() call spreads its scenes over (pipeline.streams: contiguous scene chunks, one plan + hipGraph each, "
                         "replayed concurrently; fills the tail / boundary gaps of whole-CU kernels); 0 = the library option STREAMS (csrc/options.h: 2)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed region also run everything beside the headline figure: the batch-consistency check, the 1-scene latency, "
                         "configs[2] / configs[3] / VAE decode side measurements, the per-op profile + roofline and the CPU baseline (the --no-* / "
                         "--*-scenes / --side-runs / --ops-json options below tune these).  Off: set up, warm up, time --steps calls, print the line")
    ap.add_argument("--dump-outputs", type=str, default="", metavar="DIR",
                    help="after the timed region write what the last timed call returned as DIR/latents.npy (float32, [scenes, 6, 4, 28, 50] in "
                         "global scene order; above 64 MiB a fixed seeded sample of scenes, kept in scene order).  Inputs and weights are seeded: "
                         "two builds run with the same arguments can be compared output for output")
    ap.add_argument("--side-runs", action="store_true",
                    help="with --full and --gpus > 1: also run the side measurements (configs[2], configs[3], VAE decode); by default a multi-GPU run "
                         "does the timed region only, so that N = 1, 2, 4, 8 back to back stay inside a time limit")
    ap.add_argument("--pipe-factory", type=str, default="",
                    help="TEST HOOK (tests/test_distributed.py): 'module:function' returning (pipe, unet, cn) instead of the HIP pipeline, so that the "
                         "multi-rank control flow of this script (sharding, gather, timing, teardown, ONE JSON line) runs on a box without GPUs")
    ap.add_argument("--ddim-steps", type=int, default=50)
    ap.add_argument("--scheduler", choices=["ddim", "unipc"], default="ddim",
                    help="ddim = the headline metric's sampler; unipc (with --ddim-steps 20) = what the reference's tools/test.py runs")
    ap.add_argument("--dtype", choices=["bf16", "fp16"], default="bf16",
                    help="16-bit arithmetic type of the sampler (fp32 accumulate either way): bf16 = what BASELINE.json's configs[1] names; "
                         "fp16 = what the reference samples in (magicdrive/misc/test_utils.py:95)")
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-op-profile", action="store_true")
    ap.add_argument("--ops-json", type=str, default="")
    ap.add_argument("--full-cond", action="store_true", help="run configs[2] (camera + 32 boxes + map + CFG 2.0) AS the timed workload instead of configs[1]")
    ap.add_argument("--full-cond-scenes", type=int, default=32,
                    help="after the headline measurement also time ONE configs[2] call of this many scenes per GPU (CFG doubles the views: 32 scenes = "
                         "the headline's 384 views) and report it as config.full_cond_scenes_per_s; 0 skips it")
    ap.add_argument("--no-consistency-check", action="store_true")
    ap.add_argument("--hires-scenes", type=int, default=4,
                    help="outside the timed region: also sample this many scenes per GPU of BASELINE configs[3] (6-view 432x768, camera + 32 boxes + BEV map "
                         "through the ...Plus map encoder, CFG 2.0, same sampler) and report config.hires (~1 minute at 4 scenes incl. building the "
                         "second model); 0 skips it")
    ap.add_argument("--vae-scenes", type=int, default=8,
                    help="outside the timed region: decode this many scenes' latents with the HIP AutoencoderKL (VAE_SD15_CONFIG, random weights) — what output_type='np' "
                         "adds per scene (config.vae_decode_ms_per_scene, config.scenes_per_s_incl_vae_decode); 0 skips it")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be >= 1")
    if args.ops_json and not args.full:
        ap.error("--ops-json needs --full (the per-op profile runs only there)")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` without a launcher: become the launcher (one rank per GPU over RCCL), same flags.  What the reference
        # does with `accelerate launch` (perception/data_prepare/val_set_gen.py:71-87).
        import socket
        import subprocess
        with socket.socket() as so:
            so.bind(("127.0.0.1", 0))
            port = so.getsockname()[1]
        env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        sys.exit(subprocess.call(launcher_command(args.gpus, sys.argv[1:], port), env=env))

    from magicdrive_amd import distributed as DD
    from magicdrive_amd import synthetic, flops as FL
    from magicdrive_amd.networks import spec
    rank, world, local = DD.init_from_env()
    assert world == args.gpus, f"WORLD_SIZE={world} but --gpus {args.gpus}: a line measured on fewer GPUs than it claims is worthless"
    stub = bool(args.pipe_factory)
    if not stub:
        assert torch.cuda.is_available(), "bench.py measures the HIP path: no GPU visible (there is no CPU fallback to time)"
        assert torch.cuda.device_count() > local, f"rank {rank}: local rank {local} but only {torch.cuda.device_count()} GPUs visible"
        dev = torch.device("cuda", local)
        torch.cuda.set_device(dev)
        n_devices = DD.assert_distinct_devices(dev, rank, world)    # N ranks on N different GPUs (PCI id / uuid gathered over the process group)
        sync = torch.cuda.synchronize
    else:
        dev, n_devices, sync = torch.device("cpu"), world, (lambda: None)
        args.no_op_profile = args.no_cpu_baseline = True
        args.full_cond_scenes = args.hires_scenes = args.vae_scenes = 0
    if world > 1:                                               # N ranks generate 1.3 G random weights each on the host: share the cores
        torch.set_num_threads(max(4, (os.cpu_count() or 8) // world))
    cfg = spec.SD15_CONFIG
    tdt = torch.float16 if args.dtype == "fp16" else torch.bfloat16
    if stub:
        import importlib
        mod, fn = args.pipe_factory.split(":")
        pipe, unet, cn = getattr(importlib.import_module(mod), fn)(cfg, dev)
    else:
        pipe, unet, cn = build_pipeline(cfg, dev, args.scheduler, tdt)
    pipe.use_graph = not args.no_graph
    from magicdrive_amd import _lib as _L
    pipe.streams = max(1, args.streams if args.streams > 0 else int(_L.get_option("STREAMS")) if hasattr(_L, "get_option") else 2)
    b = args.scenes_per_gpu
    n_total = b * world
    mine = DD.shard_scenes(n_total, rank, world)
    scenes = [synthetic.make_scene_batch(1, seed=1234 + i, max_len=(32 if args.full_cond else None), zero_map=not args.full_cond) for i in mine]
    cat = lambda k: torch.cat([s[k] for s in scenes]).to(dev)
    prompt, neg, bev, lat = cat("prompt_embeds"), cat("negative_prompt_embeds"), cat("bev_map"), cat("latents")
    cam = cat("camera_param") if args.full_cond else None
    boxes = {k: torch.cat([s["bboxes_3d_data"][k] for s in scenes]).to(dev) for k in ("bboxes", "classes", "masks")} if args.full_cond else None
    gs = 2.0 if args.full_cond else 1.0

    def one_call():
        out = pipe(prompt=None, image=bev, camera_param=cam, height=224, width=400, num_inference_steps=args.ddim_steps,
                   guidance_scale=gs, latents=lat, prompt_embeds=prompt, negative_prompt_embeds=neg, output_type="latent",
                   bev_controlnet_kwargs={"bboxes_3d_data": boxes} if boxes is not None else {}).images
        return DD.gather_scene_results(out, n_total, rank, world)

    for _ in range(args.warmup):
        res = one_call()
    DD.barrier(); sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        res = one_call()
    sync(); DD.barrier()
    dt = DD.max_over_ranks(time.perf_counter() - t0, dev)
    assert torch.isfinite(res).all(), "non-finite latents"
    scenes_per_s = n_total * args.steps / dt
    if args.dump_outputs and rank == 0:
        dump_latents(args.dump_outputs, res)

    # ---- outside the timed region, --full only: is the measured configuration computing the same thing as the oracle-verified one? ----
    # Scenes are independent, so scene 0 of this rank's batch must reproduce a ONE-scene call on the same inputs (the configuration
    # tests/test_e2e_gpu.py::test_real_size_ddim_loop_sd15 checks against the CPU oracle) — whatever main loops the big batch routes to.
    side = args.full and (world == 1 or args.side_runs)
    consistency = None
    if not args.no_consistency_check and b > 1 and side:
        # first, middle and LAST scene of this rank's batch (the last one sits at the highest row indices: index arithmetic, 2 GiB windows)
        consistency = 0.0
        for si in sorted({0, b // 2, b - 1}):
            sl = slice(si, si + 1)
            one = pipe(prompt=None, image=bev[sl], camera_param=None if cam is None else cam[sl], height=224, width=400, num_inference_steps=args.ddim_steps,
                       guidance_scale=gs, latents=lat[sl], prompt_embeds=prompt[sl], negative_prompt_embeds=neg[sl], output_type="latent",
                       bev_controlnet_kwargs={"bboxes_3d_data": {k: v[sl] for k, v in boxes.items()}} if boxes is not None else {}).images.float()
            row = (mine[si] if res.shape[0] == n_total else si)
            got = res[row:row + 1].float().to(one.device)
            c_ = max(((got[:, v] - one[:, v]).norm() / (one[:, v].norm() + 1e-20)).item() for v in range(one.shape[1]))
            # measured 1.6e-3 after 50 steps (bf16; BENCH_r05 batch_consistency_rel): the limit leaves room for box-to-box route changes, not for a bug
            assert c_ < 1e-2, f"scene {si} of the {b}-scene batch differs from the 1-scene call by {c_:.3e} (per-view rel L2)"
            consistency = max(consistency, c_)
    latency_1 = None
    if not args.no_consistency_check and side:
        # the other operating point: ONE scene per call (the reference's own flows run bs = 1...4) — weight-bound, one stream, plan cached above
        kw1 = dict(prompt=None, image=bev[:1], camera_param=None if cam is None else cam[:1], height=224, width=400, num_inference_steps=args.ddim_steps,
                   guidance_scale=gs, latents=lat[:1], prompt_embeds=prompt[:1], negative_prompt_embeds=neg[:1], output_type="latent",
                   bev_controlnet_kwargs={"bboxes_3d_data": {k: v[:1] for k, v in boxes.items()}} if boxes is not None else {})
        pipe(**kw1); sync()
        ts1 = []
        for _ in range(3):
            t5 = time.perf_counter(); pipe(**kw1); sync(); ts1.append(time.perf_counter() - t5)
        latency_1 = min(ts1)
    full_cond = None
    if args.full_cond_scenes > 0 and not args.full_cond and side:
        nb = args.full_cond_scenes
        fsc = [synthetic.make_scene_batch(1, seed=1234 + i, max_len=32) for i in DD.shard_scenes(nb * world, rank, world)]
        fcat = lambda k: torch.cat([s_[k] for s_ in fsc]).to(dev)
        fbox = {k: torch.cat([s_["bboxes_3d_data"][k] for s_ in fsc]).to(dev) for k in ("bboxes", "classes", "masks")}
        fkw = dict(prompt=None, image=fcat("bev_map"), camera_param=fcat("camera_param"), height=224, width=400, num_inference_steps=args.ddim_steps,
                   guidance_scale=2.0, latents=fcat("latents"), prompt_embeds=fcat("prompt_embeds"), negative_prompt_embeds=fcat("negative_prompt_embeds"),
                   output_type="latent", bev_controlnet_kwargs={"bboxes_3d_data": fbox})
        pipe(**fkw)                                              # builds + captures the plan, warms up
        DD.barrier(); torch.cuda.synchronize()
        t1 = time.perf_counter()
        fout = pipe(**fkw).images
        torch.cuda.synchronize(); DD.barrier()
        fdt = DD.max_over_ranks(time.perf_counter() - t1, dev)
        assert torch.isfinite(fout).all()
        full_cond = {"scenes_per_s": nb * world / fdt, "scenes_per_gpu": nb, "seconds_per_call": fdt}
        # ... and the reference's own call (tools/test.py, validation_batch_size 1): ONE scene with camera + boxes + map and CFG = 12 views per pass
        fkw1 = dict(fkw, image=fkw["image"][:1], camera_param=fkw["camera_param"][:1], latents=fkw["latents"][:1], prompt_embeds=fkw["prompt_embeds"][:1],
                    negative_prompt_embeds=fkw["negative_prompt_embeds"][:1], bev_controlnet_kwargs={"bboxes_3d_data": {k: v[:1] for k, v in fbox.items()}})
        pipe(**fkw1); torch.cuda.synchronize()
        ts2 = []
        for _ in range(3):
            t6 = time.perf_counter(); pipe(**fkw1); torch.cuda.synchronize(); ts2.append(time.perf_counter() - t6)
        full_cond["latency_1scene_s"] = min(ts2)

    hires = None
    if args.hires_scenes > 0 and side:
        hh, hw_ = 432 // 8, 768 // 8
        hcfg = spec.with_plus_map_embedder(cfg, (hh, hw_))
        hpipe, _, _ = build_pipeline(hcfg, dev, args.scheduler, tdt)
        hpipe.use_graph = pipe.use_graph
        hpipe.streams = pipe.streams
        nh = args.hires_scenes
        hsc = [synthetic.make_scene_batch(1, seed=4321 + i, max_len=32, latent_hw=(hh, hw_)) for i in DD.shard_scenes(nh * world, rank, world)]
        hcat = lambda k: torch.cat([s_[k] for s_ in hsc]).to(dev)
        hbox = {k: torch.cat([s_["bboxes_3d_data"][k] for s_ in hsc]).to(dev) for k in ("bboxes", "classes", "masks")}
        hkw = dict(prompt=None, image=hcat("bev_map"), camera_param=hcat("camera_param"), height=432, width=768, num_inference_steps=args.ddim_steps,
                   guidance_scale=2.0, latents=hcat("latents"), prompt_embeds=hcat("prompt_embeds"), negative_prompt_embeds=hcat("negative_prompt_embeds"),
                   output_type="latent", bev_controlnet_kwargs={"bboxes_3d_data": hbox})
        hpipe(**hkw)
        DD.barrier(); torch.cuda.synchronize()
        t3 = time.perf_counter()
        hout = hpipe(**hkw).images
        torch.cuda.synchronize(); DD.barrier()
        hdt = DD.max_over_ranks(time.perf_counter() - t3, dev)
        assert torch.isfinite(hout).all()
        hplan = next(iter(hpipe._plans.values()))
        hf = FL.program_flops(hplan.step_ops)["total"] * args.ddim_steps / nh
        hires = {"workload": "configs[3]: 6-view 432x768 (54x96 latents), camera + 32 boxes + BEV map (...Plus map encoder), CFG 2.0, same sampler",
                 "scenes_per_gpu": nh, "scenes_per_s": round(nh * world / hdt, 4), "seconds_per_call": round(hdt, 3), "tflop_per_scene": round(hf / 1e12, 1),
                 "mfma_frac_end_to_end": round(hf * nh / hdt / 1e12 / MFMA_BF16_PEAK_TFLOPS, 4)}
        del hpipe
    vae_ms = None
    if args.vae_scenes > 0 and side:
        from magicdrive_amd.networks.autoencoder_kl import AutoencoderKL
        vae = AutoencoderKL.from_config(spec.VAE_SD15_CONFIG, 7).to(dev)
        nv = min(args.vae_scenes, b)
        zl = (res[:nv].to(dev).float() / 0.18215).reshape(-1, 4, 28, 50)            # decode_latents, pipeline_bev_controlnet.py:100-112
        img = vae.decode(zl).sample                                                  # plan build + warm-up
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        img = vae.decode(zl).sample
        img = (img / 2 + 0.5).clamp(0, 1).permute(0, 2, 3, 1).float().cpu()          # the pipeline's "np" output incl. the device -> host copy
        vae_ms = 1e3 * (time.perf_counter() - t2) / nv
        assert img.shape == (6 * nv, 224, 400, 3) and torch.isfinite(img).all()
        vplan = next(iter(vae._plans.values()))
        vae_tf = FL.program_flops(vplan.ops)["total"] / max(vplan.n // 6, 1) / 1e12   # per 6-view scene (algorithmic, 2 FLOPs per MAC); the plan decodes vplan.n images per run
        torch.cuda.synchronize()
        t4 = time.perf_counter()
        vae.decode(zl)
        torch.cuda.synchronize()
        vae_dev_ms = 1e3 * (time.perf_counter() - t4) / nv                              # device part only (no clamp / permute / host copy)
        del vae, img, zl
    # Every rank leaves the process group TOGETHER before rank 0 goes on alone (per-op profile, CPU baseline: minutes): ranks that return
    # while rank 0 still holds the group make torchrun's teardown / the RCCL watchdog kill the job before the JSON line is printed.
    DD.shutdown()
    if rank != 0:
        return
    if stub:
        plan, f_scene = None, 0.0
    else:
        plan = max((pl for pl in pipe._plans.values() if pl.do_cfg == (gs > 1.0 and cam is not None) and pl.h == 28), key=lambda pl: pl.b)
        f_step = FL.program_flops(plan.step_ops)
        f_pro = FL.program_flops(plan.prologue_ops)
        f_scene = (args.ddim_steps * f_step["total"] + f_pro["total"]) / plan.b     # per scene, incl. CFG duplication if any
    out = {
        "metric": "6-view scenes/sec at 224x400, 50-step DDIM" if (args.scheduler, args.ddim_steps) == ("ddim", 50) else f"6-view scenes/sec at 224x400, {args.ddim_steps}-step {args.scheduler}", "value": scenes_per_s, "unit": "scenes/s",
        "n_gpus": n_devices, "steps": args.steps, "warmup": args.warmup, "ms_per_step": 1e3 * dt / args.steps,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
        "config": {"workload": ("configs[2]: 6-view 224x400, camera+32 boxes+BEV map, CFG 2.0" if args.full_cond else
                                f"configs[1]: 6-view 224x400, text-only conditioning (camera_param=None -> CFG off), {args.ddim_steps}-step {args.scheduler.upper() if args.scheduler == 'ddim' else 'UniPC'}, {args.dtype}"),
                   "scenes_per_gpu": b, "ddim_steps": args.ddim_steps, "scheduler": args.scheduler, "unet_params_M": round(unet.num_parameters() / 1e6, 1),
                   "controlnet_params_M": round(cn.num_parameters() / 1e6, 1), "parallelism": f"scene-sharded x{world}",
                   "hipgraph": pipe.use_graph, "streams": pipe.streams, "output_type": "latent",
                   "tflop_per_scene": round(f_scene / 1e12, 3),
                   "mfma_frac_end_to_end": round(f_scene * scenes_per_s / world / 1e12 / MFMA_BF16_PEAK_TFLOPS, 4),
                   "batch_consistency_rel": None if consistency is None else round(consistency, 5),
                   "latency_1scene_s": None if latency_1 is None else round(latency_1, 4),
                   "hires": hires,
                   "vae_decode_ms_per_scene": None if vae_ms is None else round(vae_ms, 2),
                   "vae": None if vae_ms is None else {"tflop_per_scene": round(vae_tf, 3), "decode_ms_per_scene_device": round(vae_dev_ms, 2),
                                                       "mfma_frac": round(vae_tf / (vae_dev_ms * 1e-3) / MFMA_BF16_PEAK_TFLOPS, 4),
                                                       "what": "AutoencoderKL.decode of one 6-view scene (SD-1.5 VAE, 224x400): op program on the sampler's kernels"},
                   "scenes_per_s_incl_vae_decode": None if vae_ms is None else round(1.0 / (world / scenes_per_s + vae_ms * 1e-3) * world, 4),
                   "latency_1scene_full_cond_cfg_s": None if full_cond is None else round(full_cond["latency_1scene_s"], 4),
                   "full_cond_scenes_per_s": None if full_cond is None else round(full_cond["scenes_per_s"], 4),
                   "full_cond": None if full_cond is None else
                   {"workload": "configs[2]: 6-view 224x400, camera + 32 boxes + BEV map, CFG 2.0, same sampler", "scenes_per_gpu": full_cond["scenes_per_gpu"],
                    "seconds_per_call": round(full_cond["seconds_per_call"], 3)}},
    }
    if args.full and not args.no_op_profile:
        fam, kern, rows = per_op_profile(plan)
        _PMC["views"] = plan.B
        summ = pmc_summary()
        pviews = sorted({c.get("views") for v in (summ or {}).get("kernels", {}).values() for c in (v.get("cases") or [v])}, key=str)
        if summ is not None and plan.B not in pviews:
            _PMC["status"] += f"; its counters were collected at {pviews} views, the profiled plan has {plan.B}: counters dropped"
        out["config"]["per_op_profile"] = {"scenes": plan.b, "views": plan.B, "reps": 5, "statistic": "median (ms_best beside it in --ops-json)",
                                           "note": "one plan's step program launched op by op on ONE stream with HIP events between the launches"
                                                   + (f"; the timed region replays {pipe.streams} such plans concurrently" if pipe.streams > 1 and plan.b < b else "")}
        # dominant KERNEL (the name rocprofv3 --kernel-trace --stats reports, template arguments abbreviated) by time in a step
        name, d = max(kern.items(), key=lambda kv: kv[1]["ms"])
        compute = {k: v for k, v in fam.items() if v["flops"] > 0 and k.startswith(("gemm_conv", "attn"))}
        if d["mfma"] and d["flops"] > 0:
            ach = d["flops"] / (d["ms"] * 1e-3) / 1e12
            out["roofline"] = {"bound": "mfma", "kernel": name, "achieved": ach, "peak": MFMA_BF16_PEAK_TFLOPS, "unit": "TFLOP/s",
                               "frac": ach / MFMA_BF16_PEAK_TFLOPS, "traffic": pmc_traffic(name, 1e3 * d["ms"] / d["launches"]),
                               "launches_per_step": d["launches"], "avg_launch_us": 1e3 * d["ms"] / d["launches"]}
        else:
            ach = d["bytes"] / (d["ms"] * 1e-3) / 1e9
            out["roofline"] = {"bound": "hbm", "kernel": name, "achieved": ach, "peak": 8000.0, "unit": "GB/s", "frac": ach / 8000.0,
                               "traffic": None, "launches_per_step": d["launches"], "avg_launch_us": 1e3 * d["ms"] / d["launches"]}
        top = sorted(kern.items(), key=lambda kv: -kv[1]["ms"])[:10]
        def pk(k, v):
            row = {"ms_per_step": round(v["ms"], 3), "ms_per_step_best": round(v["ms_best"], 3), "launches": v["launches"], "avg_launch_us": round(1e3 * v["ms"] / v["launches"], 1),
                   "tflops": round(v["flops"] / (v["ms"] * 1e-3) / 1e12, 1) if v["mfma"] and v["flops"] else None,
                   "alg_gbps": round(v["bytes"] / (v["ms"] * 1e-3) / 1e9, 1)}
            c = pmc_traffic(k, 1e3 * v["ms"] / v["launches"])   # counters of a representative launch of this kernel (committed PMC passes)
            if c:
                row.update(mfma_util=c.get("mfma_util"), hbm_gbps=c.get("hbm_gbps"), l2_hit_rate=c.get("l2_hit_rate"),
                           traffic_over_algorithmic=c.get("traffic_over_algorithmic"), pmc_case=c.get("case"),
                           pmc_build=(pmc_summary() or {}).get("build_id"))      # == library_build_id below, or the counters were dropped
            return row
        out["roofline"]["per_kernel"] = {k: pk(k, v) for k, v in top}
        # the north-star's own counter: rocprof MfmaUtil (SQ_VALU_MFMA_BUSY_CYCLES / (cycles x SIMDs)) of the committed counter passes, weighted by the
        # time each kernel takes in THIS run's step program — over the attention + conv kernels, and over attention + conv + GEMM
        def weighted_util(pred):
            num = den = 0.0
            for k, v in kern.items():
                if not (v["mfma"] and pred(k)):
                    continue
                c = pmc_traffic(k, 1e3 * v["ms"] / v["launches"])
                if c and c.get("mfma_util") is not None:
                    num += v["ms"] * c["mfma_util"]; den += v["ms"]
            tot = sum(v["ms"] for k, v in kern.items() if v["mfma"] and pred(k))
            return None if den == 0 else {"mfma_util": round(num / den, 4), "ms_covered": round(den, 2), "ms_total": round(tot, 2)}
        is_attn_conv = lambda k: k.startswith("attn") or "conv" in k
        out["roofline"]["mfma_util_time_weighted"] = {"attn_conv": weighted_util(is_attn_conv), "attn_conv_gemm": weighted_util(lambda k: True),
                                                      "source": _PMC.get("status")}
        out["roofline"]["pmc_status"] = _PMC.get("status")
        out["roofline"]["library_build_id"] = __import__("magicdrive_amd._lib", fromlist=["x"]).build_id()
        out["roofline"]["per_family"] = {k: {"ms_per_step": round(v["ms"], 4), "launches": v["launches"],
                                              "tflops": round(v["flops"] / (v["ms"] * 1e-3) / 1e12, 2) if v["flops"] else None}
                                         for k, v in fam.items()}
        tot_ms = sum(v["ms"] for v in compute.values()); tot_fl = sum(v["flops"] for v in compute.values())
        out["roofline"]["attn_conv_gemm_tflops"] = round(tot_fl / (tot_ms * 1e-3) / 1e12, 2)
        # FLOP-based ("useful") fraction of the dense peak over the attention + 3x3-conv launches: algorithmic FLOPs (no padded MFMA rows: the
        # d = 40 attention multiplies 48 / 64-row tiles, which the MfmaUtil COUNTER above books as busy) / their time — the north-star's ">= 60 % on
        # the attention + conv blocks" read against work done, beside the counter figure
        ac = {k: v for k, v in fam.items() if v["flops"] > 0 and (k.startswith("attn") or k == "gemm_conv_kernel<conv>")}
        ac_ms = sum(v["ms"] for v in ac.values()); ac_fl = sum(v["flops"] for v in ac.values())
        out["roofline"]["useful_frac_attn_conv"] = round(ac_fl / (ac_ms * 1e-3) / 1e12 / MFMA_BF16_PEAK_TFLOPS, 4) if ac_ms > 0 else None
        out["roofline"]["useful_frac_attn_conv_gemm"] = round(tot_fl / (tot_ms * 1e-3) / 1e12 / MFMA_BF16_PEAK_TFLOPS, 4) if tot_ms > 0 else None
        if args.ops_json:
            os.makedirs(os.path.dirname(args.ops_json) or ".", exist_ok=True)
            with open(args.ops_json, "w") as f:
                json.dump(rows, f)
    if args.full and world == 1 and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(cfg)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
