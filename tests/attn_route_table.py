"""The attention route table (tests/golden/attn_routes.json): loading it, turning a case into the inputs of attn_route
(tests/attn_route_check.cpp) and issuing it to the built library.  tools/attn_route_table.py defines the cases and records the table."""
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "attn_routes.json")

# Tk: None = Tq.  kmult: K rows are a column block of a fused projection `kmult` heads-times-d wide (self / cross-view: q|k, CLIP: q|k|v).
# ctx: "dev" = MdxAttnDesc.tk_dev (one live key count), "rows" = mdx_attention_ctx_rows_* (one per query batch); live = that count.
DEFAULTS = dict(H=8, Tk=None, nsrc=1, joint=False, pre=True, causal=False, rowmajor=False, ctx=None, live=None, kmult=2, ldv_extra=0, opts={}, f16=False)


def load():
    with open(GOLDEN) as f:
        return [dict(DEFAULTS, **c) for c in json.load(f)["cases"]]


def layout(c):
    """(Tk, ldk, sK, ldv, sV) of the dense tensors run_case builds."""
    Tk = c["Tk"] or c["Tq"]
    C = c["H"] * c["d"]
    ldk = c["kmult"] * C
    if c["rowmajor"]:
        return Tk, ldk, Tk * ldk, ldk, Tk * ldk
    ldv = (Tk + 7) // 8 * 8 + c["ldv_extra"]
    return Tk, ldk, Tk * ldk, ldv, C * ldv


def route_line(c):
    """'key=value ...': the AttnIn / AttnOpts of a case."""
    Tk, ldk, sK, ldv, sV = layout(c)
    f = dict(B=c["B"], H=c["H"], Tq=c["Tq"], Tk=Tk, d=c["d"], nsrc=c["nsrc"], joint=int(c["joint"]), q_prescaled=int(c["pre"]), causal=int(c["causal"]),
             v_rowmajor=int(c["rowmajor"]), has_tk_dev=int(c["ctx"] is not None), rows=int(c["ctx"] == "rows"), ldk=ldk, ldv=ldv, sK=sK, sV=sV)
    return " ".join(f"{k}={v}" for k, v in {**f, **c["opts"]}.items())


def evaluate(lines, workdir):
    """Build tests/attn_route_check.cpp with g++ into `workdir`, feed it `lines` ('name key=value ...') and return {name: {field: value}} of what
    it prints.  None when there is no g++."""
    import shutil
    import subprocess
    gxx = shutil.which("g++")
    if gxx is None:
        return None
    exe = os.path.join(str(workdir), "attn_route_check")
    subprocess.run([gxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(HERE, "attn_route_check.cpp")], check=True)
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    out = {}
    for line in r.stdout.splitlines():
        name, rest = line.split(" ", 1)
        out[name] = dict(kv.split("=", 1) for kv in rest.split())
    return out


def run_case(c, values=False):
    """Issue the case to the built library once and return mdx_last_kernel(); with values=True, (tag, O, fp32 reference) on seeded inputs."""
    import torch
    from magicdrive_amd import _lib as L
    from magicdrive_amd import ops as O

    dt = torch.float16 if c["f16"] else torch.bfloat16
    g = torch.Generator(device="cuda").manual_seed(1234)
    B, H, Tq, d = c["B"], c["H"], c["Tq"], c["d"]
    Tk, ldk, _, ldv, _ = layout(c)
    C = H * d

    def rnd(*shape):
        return torch.randn(*shape, generator=g, device="cuda").to(dt) if values else torch.zeros(*shape, dtype=dt, device="cuda")

    qscale = d ** -0.5 * 1.4426950408889634 if c["pre"] else 1.0
    if c["kmult"] > 1:                    # Q | K (| V) column blocks of one fused projection (self attention: Tk == Tq)
        fused = rnd(B, Tq, c["kmult"] * C)
        q, k = fused[:, :, :C], fused[:, :, C:2 * C]
        v = fused[:, :, 2 * C:] if c["rowmajor"] else rnd(B, Tk, C)
        if c["pre"]:
            fused[:, :, :C] = (fused[:, :, :C].float() * qscale).to(dt)
    else:
        q, k, v = (rnd(B, Tq, C).float() * qscale).to(dt), rnd(B, Tk, C), rnd(B, Tk, C)
    if c["rowmajor"]:
        vt = v
    else:
        vt = torch.full((B, C, ldv), float("nan") if values else 0.0, dtype=dt, device="cuda")
        vt[:, :, :Tk] = v.transpose(1, 2)
    o = torch.full((B, Tq, C), float("nan"), dtype=dt, device="cuda")
    kw = {}
    srcs = lambda i: [(i + s) % B for s in range(c["nsrc"])]
    if c["nsrc"] > 1:
        kw.update(kvmap=torch.tensor([j for i in range(B) for j in srcs(i)], dtype=torch.int32, device="cuda"), nsrc=c["nsrc"], joint=c["joint"])
    live = c["live"] or Tk
    if c["ctx"] == "dev":
        kw["tk_dev"] = torch.tensor([live], dtype=torch.int32, device="cuda")
    elif c["ctx"] == "rows":
        kw["tk_rows"] = torch.full((B,), live, dtype=torch.int32, device="cuda")
    with L.options(**c["opts"]):
        O.run_ops([O.Attn(q, k, vt, o, heads=H, Tk=Tk, scale=d ** -0.5, q_prescaled=c["pre"], causal=c["causal"], v_rowmajor=c["rowmajor"], **kw)])
        tag = (L.lib().mdx_last_kernel() or b"").decode()
        torch.cuda.synchronize()
    if not values:
        return tag
    # fp32 reference on the rounded inputs: per source softmax(Q K^T scale) V, summed; joint: one softmax over the concatenated sources
    qf = (q.float() / qscale).view(B, Tq, H, d).transpose(1, 2)
    kf, vf = (t.float()[:, :live].reshape(B, live, H, d).transpose(1, 2) for t in (k, v))
    ref = torch.zeros(B, H, Tq, d, device="cuda")
    for i in range(B):
        js = srcs(i)
        groups = [js] if c["joint"] or len(js) == 1 else [[j] for j in js]
        for grp in groups:
            s = qf[i] @ torch.cat([kf[j] for j in grp], 1).transpose(1, 2) * d ** -0.5
            if c["causal"]:
                s = s.masked_fill(torch.ones(Tq, live, dtype=torch.bool, device="cuda").triu(1), float("-inf"))
            ref[i] += torch.softmax(s, -1) @ torch.cat([vf[j] for j in grp], 1)
    return tag, o, ref.transpose(1, 2).reshape(B, Tq, C)
