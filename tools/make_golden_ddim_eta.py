#!/usr/bin/env python
"""Generate tests/golden/ddim_eta_steps.pt by running the REAL reference DDIMScheduler (diffusers' scheduling_ddim.py, imported through
oracle.refshim like tools/make_golden.py does; authoring container only): what tests/test_ddim_eta_contract.py and
tests/test_ddim_eta_gpu.py compare DDIMScheduler.variance_table and DDIMScheduler.step(..., variance_noise=) against.

SD-1.5 betas (scaled_linear 0.00085 .. 0.012, 1000 train steps, steps_offset 1, set_alpha_to_one False, no clipping); 20 and 50 inference
steps; eta in {0, 0.3, 1}; the first, the middle and the last timestep.  Per case, all fp32 as the reference computes them
(stored as four stacked tensors, see `layout` in the file):
  index, timestep     row of the timestep list and its value
  a_t, a_prev         the two alphas_cumprod entries the reference's step reads
  variance            scheduler._get_variance(timestep, prev_timestep)
  std                 the reference step's output for sample = model_output = 0 and variance_noise = 1: std_dev_t itself
  sample, model_output, variance_noise, prev_sample     16 random elements each and the reference step's result
A few kB of data, no program text.

  python tools/make_golden_ddim_eta.py
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import refshim  # noqa: E402

N_ELEM = 16


def main():
    ns = refshim.load()
    gen = torch.Generator().manual_seed(20)
    cases = []
    for n_steps in (20, 50):
        sch = ns.DDIMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", num_train_timesteps=1000,
                               clip_sample=False, set_alpha_to_one=False, steps_offset=1)
        sch.set_timesteps(n_steps)
        ts = sch.timesteps.tolist()
        for eta in (0.0, 0.3, 1.0):
            for index in (0, n_steps // 2, n_steps - 1):
                t = int(ts[index])
                prev_t = t - sch.config.num_train_timesteps // sch.num_inference_steps
                a_t = sch.alphas_cumprod[t]
                a_prev = sch.alphas_cumprod[prev_t] if prev_t >= 0 else sch.final_alpha_cumprod
                sample = torch.randn(N_ELEM, generator=gen) * 2.0
                eps = torch.randn(N_ELEM, generator=gen)
                z = torch.randn(N_ELEM, generator=gen)
                kw = dict(eta=eta, variance_noise=z) if eta > 0 else dict(eta=eta)
                prev = sch.step(eps, t, sample, **kw).prev_sample
                zero = torch.zeros(N_ELEM)
                std = sch.step(zero, t, zero, eta=eta, variance_noise=torch.ones(N_ELEM)).prev_sample[0] if eta > 0 else torch.tensor(0.0)
                cases.append(((n_steps, index, t), eta, torch.stack([a_t, a_prev, sch._get_variance(t, prev_t), std]).float(),
                              torch.stack([sample, eps, z, prev])))
    out = os.path.join(ROOT, "tests", "golden", "ddim_eta_steps.pt")
    # four stacked tensors (one zip entry each: a tensor per field and case would cost ten times the bytes in container overhead)
    torch.save(dict(case=torch.tensor([c[0] for c in cases], dtype=torch.int64), eta=torch.tensor([c[1] for c in cases], dtype=torch.float64),
                    scalars=torch.stack([c[2] for c in cases]), tensors=torch.stack([c[3] for c in cases]),
                    layout="case [n, 3] = (n_steps, index, timestep); scalars [n, 4] = (a_t, a_prev, variance, std); "
                           "tensors [n, 4, 16] = (sample, model_output, variance_noise, prev_sample)"), out)
    print(out, os.path.getsize(out), "bytes,", len(cases), "cases")


if __name__ == "__main__":
    main()
