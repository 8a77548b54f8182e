"""tools/sample.py --eta X on the CPU with a stub pipeline (this file, loaded through the driver's --pipe-factory hook).

  with the flag       eta reaches the pipeline call as a float — the same call runner.pipeline_param.eta=X makes — index.json carries
                      "eta": X and nothing else changes (the stub ignores the value: same pictures, same records);
  refusals            with --scheduler unipc (the driver's default) and for a negative or non-finite value the driver stops before it
                      builds a pipeline;
  without the flag    byte for byte today's output: tests/test_sample_regions.py rebuilds those bytes from first principles, and the
                      plain run of this file equals a run without the flag file by file.
"""
import json
import os
import subprocess
import sys

import pytest
import torch

import sample_stub
import test_sample_regions as SR

ROOT = SR.ROOT


class EtaStub(sample_stub.StubPipe):
    def __call__(self, **kw):
        with open(os.environ["ETA_STUB_LOG"], "a") as f:
            f.write(json.dumps(dict(has="eta" in kw, eta=kw.get("eta"), kind=type(kw.get("eta")).__name__, seed=int(kw["generator"].initial_seed()))) + "\n")
        kw.pop("eta", None)
        return super().__call__(**kw)


def make(ckpt, sd15, scheduler, device, given_view):
    return EtaStub()


def run_driver(tmp_path, out_name, extra=(), overrides=()):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), os.environ.get("PYTHONPATH", "")]),
               CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="", OMP_NUM_THREADS="2", ETA_STUB_LOG=str(tmp_path / f"{out_name}.jsonl"))
    cmd = [sys.executable, os.path.join(ROOT, "tools", "sample.py"), "--ckpt", str(tmp_path / "ckpt"), "--sd15", str(tmp_path / "sd15"), "--data", str(tmp_path / "data"),
           "--out", str(tmp_path / out_name), "--prompt-embeds", "--pipe-factory", "test_sample_eta:make", "--dist-backend", "gloo", "--device", "cpu",
           "--batch-size", str(SR.BATCH), *extra, f"runner.validation_times={SR.TIMES}", *overrides]
    return subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("sample_eta")
    gold = torch.load(os.path.join(ROOT, "tests", "golden", "sample_preprocess.pt"), weights_only=False)
    os.makedirs(tmp / "data"); os.makedirs(tmp / "ckpt" / "hydra"); os.makedirs(tmp / "sd15")
    for i, case in enumerate(gold["cases"]):
        torch.save(case["sample"], tmp / "data" / f"tok{i}.pth")
    with open(tmp / "ckpt" / "hydra" / "overrides.yaml", "w") as f:
        f.write(f"- +exp=224x400\n- seed={SR.SEED}\n")
    res = {"plain": run_driver(tmp, "plain", ["--scheduler", "ddim"]),
           "on": run_driver(tmp, "on", ["--scheduler", "ddim", "--eta", "0.5"]),
           "override": run_driver(tmp, "override", ["--scheduler", "ddim"], ["runner.pipeline_param.eta=0.5"]),
           "zero": run_driver(tmp, "zero", ["--scheduler", "ddim", "--eta", "0"]),
           "unipc": run_driver(tmp, "unipc", ["--eta", "0.5"]),
           "unipc2": run_driver(tmp, "unipc2", ["--scheduler", "unipc", "--eta", "1"]),
           "neg": run_driver(tmp, "neg", ["--scheduler", "ddim", "--eta", "-0.5"]),
           "nan": run_driver(tmp, "nan", ["--scheduler", "ddim", "--eta", "nan"]),
           "inf": run_driver(tmp, "inf", ["--scheduler", "ddim", "--eta", "inf"])}
    return tmp, res


def _log(tmp, name):
    with open(tmp / f"{name}.jsonl") as f:
        return [json.loads(ln) for ln in f]


def test_eta_reaches_the_call_and_the_index(runs):
    tmp, res = runs
    for name in ("plain", "on", "override", "zero"):
        assert res[name].returncode == 0, res[name].stderr[-2000:]
    on, override, plain, zero = (_log(tmp, n) for n in ("on", "override", "plain", "zero"))
    assert on and all(r["has"] and r["eta"] == 0.5 and r["kind"] == "float" for r in on)
    assert on == override, "--eta X is runner.pipeline_param.eta=X: the same calls"
    assert all(not r["has"] for r in plain) and [r["seed"] for r in plain] == [r["seed"] for r in on]
    assert all(r["has"] and r["eta"] == 0.0 for r in zero)
    idx = {n: json.load(open(tmp / n / "index.json")) for n in ("plain", "on", "override", "zero")}
    assert idx["on"]["eta"] == 0.5 and idx["zero"]["eta"] == 0.0 and "eta" not in idx["plain"] and "eta" not in idx["override"]
    assert {k: v for k, v in idx["on"].items() if k != "eta"} == idx["plain"] == idx["override"]
    assert list(idx["on"]) == ["world", "seed", "gather_images", "eta", "generations"]
    # the stub ignores the value: the same pictures
    assert SR.pngs(tmp, "on") == SR.pngs(tmp, "plain") and all(SR.read(tmp, "on", n) == SR.read(tmp, "plain", n) for n in SR.pngs(tmp, "on"))


def test_without_the_flag_the_output_is_what_it_was(runs):
    """index.json of the plain run, byte for byte, is the dump tests/test_sample_regions.py spells out: no key was added, none moved."""
    tmp, res = runs
    idx = json.load(open(tmp / "plain" / "index.json"))
    assert list(idx) == ["world", "seed", "gather_images", "generations"]
    assert SR.read(tmp, "plain", "index.json").decode() == json.dumps(dict(world=1, seed=SR.SEED, gather_images=False, generations=idx["generations"]), indent=1)
    assert SR.read(tmp, "override", "index.json") == SR.read(tmp, "plain", "index.json")
    assert res["plain"].stdout.strip().splitlines()[-1] == f"sampled 5 scenes x {SR.TIMES} on 1 rank(s) -> {tmp / 'plain'}"
    assert len(SR.pngs(tmp, "plain")) == 5 * SR.TIMES * 6


def test_the_flag_is_refused_where_it_has_no_meaning(runs):
    tmp, res = runs
    for name, what in (("unipc", "--scheduler ddim"), ("unipc2", "--scheduler ddim"), ("neg", "finite number >= 0"), ("nan", "finite number >= 0"),
                       ("inf", "finite number >= 0")):
        assert res[name].returncode != 0 and what in res[name].stderr, (name, res[name].stderr[-500:])
        assert not os.path.exists(tmp / name / "index.json") and not os.path.exists(tmp / f"{name}.jsonl")
