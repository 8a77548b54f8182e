"""The GEMM / conv route table (tests/golden/gemm_routes.json): loading it, turning a case into the inputs of gemm_route
(tests/gemm_route_check.cpp) and issuing it to the built library.  tools/route_table.py defines the cases and records the table."""
import hashlib
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "gemm_routes.json")

DEFAULTS = dict(kind="gemm", bias=True, res=False, temb=False, epi=0, splitk=0, ws_mb=64, ln=False, ln_scratch=True, ln_stats=0, rowstat=0, lda=0,
                k=3, stride=1, opts={}, gpu=True)


def load():
    with open(GOLDEN) as f:
        return [dict(DEFAULTS, **c) for c in json.load(f)["cases"]]


def _common(c, M, N, K, nout):
    ws = c["ws_mb"] << 20
    return dict(M=M, N=N, K=K, epi=c["epi"], splitk=c["splitk"], ldw=K, ldc=nout, ldr=nout if c["res"] else 0, wide=int(nout % 8 == 0),
                has_ws=int(ws > 0 and not c.get("ws_null")), ws_bytes=ws, bias=int(c["bias"]), R=int(c["res"]), temb=int(c["temb"]))


def route_lines(c):
    """[(label, 'key=value ...')]: the RouteIn / RouteOpts of a case as tests use dense, 16-byte aligned tensors for it.  A flat case gives
    two lines: the flattened form and the per-batch launches it falls back to when the flattened form declines."""
    kind = c["kind"]
    if kind == "gemm":
        M, N, K = c["M"], c["N"], c["K"]
        f = _common(c, M, N, K, N // 2 if c["epi"] == 1 else N)
        f.update(lda=c["lda"] or K, ln=int(c["ln"]), ln_csum=int(c["ln"]), ln_scratch=int(c["ln"] and c["ln_scratch"]),
                 ln_stats=int(c["ln_stats"] > 0), ln_stats_parts=c["ln_stats"], rowstat=int(c["rowstat"] > 0), rowstat_parts=c["rowstat"])
        sets = [("", f)]
    elif kind == "conv":
        k, s = c["k"], c["stride"]
        pad = k // 2
        Ho, Wo = (c["H"] + 2 * pad - k) // s + 1, (c["W"] + 2 * pad - k) // s + 1
        f = _common(c, c["B"] * Ho * Wo, c["Cout"], k * k * c["Cin"], c["Cout"])
        f.update(conv=1, lda=c["Cin"], rows_per_b=Ho * Wo, Hi=c["H"], Wi=c["W"], Cin=c["Cin"], Ho=Ho, Wo=Wo, kh=k, kw=k, sh=s, sw=s, ph=pad, pw=pad,
                 cimajor=int(k > 1 and c["Cin"] % 64 == 0), ln=int(c["ln"]))
        sets = [("", f)]
    elif kind == "up2":
        f = _common(c, c["B"] * c["Ho"] * c["Wo"], c["Cout"], 4 * c["Cin"], c["Cout"])
        f.update(conv=int(c.get("conv", 1)), lda=c["Cin"], rows_per_b=c["Ho"] * c["Wo"], Hi=c["H"], Wi=c["W"], Cin=c["Cin"], Ho=c["Ho"], Wo=c["Wo"],
                 kh=2, kw=2, sh=1, sw=1, up2=1, upB=c["B"], splitk=1)
        sets = [("", f)]
    else:   # flat: Gemm(Wv [Cc, Cc], X [Bt, T, Cc], Vt [Bt, Cc, ldv][:, :, :T])
        Bt, T, Cc = c["Bt"], c["T"], c["Cc"]
        ldv = (T + 7) // 8 * 8
        base = dict(M=Cc, K=Cc, lda=Cc, ldw=Cc, ldc=ldv, sC=Cc * ldv, has_ws=0)
        sets = [("#flat", dict(base, N=Bt * T, col_split=T, wide=0, flat=1)), ("#batch", dict(base, N=T, batch=Bt, wide=int(T % 8 == 0)))]
    return [(c["name"] + tag, " ".join(f"{k}={v}" for k, v in {**f, **c["opts"]}.items())) for tag, f in sets]


def evaluate(lines, workdir):
    """Build tests/gemm_route_check.cpp with g++ into `workdir`, feed it `lines` ('name key=value ...') and return {name: {field: value}} of what
    it prints (an error's text under "msg").  None when there is no g++."""
    import shutil
    import subprocess
    gxx = shutil.which("g++")
    if gxx is None:
        return None
    exe = os.path.join(str(workdir), "gemm_route_check")
    subprocess.run([gxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(HERE, "gemm_route_check.cpp")], check=True)
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    out = {}
    for line in r.stdout.splitlines():
        name, rest = line.split(" ", 1)
        if " msg=" in rest:
            head, msg = rest.split(" msg=", 1)
            out[name] = dict(kv.split("=", 1) for kv in head.split()); out[name]["msg"] = msg
        else:
            out[name] = dict(kv.split("=", 1) for kv in rest.split())
    return out


def run_case(c):
    """Issue the case to the built library once: (mdx_last_kernel(), SHA-256 of everything it wrote).  Inputs are seeded; the kernels are
    deterministic (split-K slabs, not atomics)."""
    import torch
    from magicdrive_amd import _lib as L
    from magicdrive_amd import ops as O

    BF = torch.bfloat16
    g = torch.Generator(device="cuda").manual_seed(1234)

    def rnd(*shape, scale=1.0, dtype=BF):
        return (torch.randn(*shape, generator=g, device="cuda") * scale).to(dtype)

    ws = torch.empty((c["ws_mb"] << 20) // 4, dtype=torch.float32, device="cuda") if c["ws_mb"] else None
    outs = []
    kind = c["kind"]
    if kind == "gemm":
        M, N, K = c["M"], c["N"], c["K"]
        nout = N // 2 if c["epi"] == 1 else N
        A, W = rnd(M, K), rnd(N, K, scale=K ** -0.5)
        C = torch.zeros(M, nout, dtype=BF, device="cuda")
        kw = dict(bias=rnd(N, dtype=torch.float32) if c["bias"] else None, R=rnd(M, nout) if c["res"] else None, epilogue=c["epi"], splitk=c["splitk"], ws=ws)
        if c["ln"]:
            kw.update(ln_eps=1e-5, ln_csum=W.float().sum(1).contiguous(), ln_scratch=torch.zeros(M, K, dtype=BF, device="cuda") if c["ln_scratch"] else None)
            if c["ln_stats"]:
                st = torch.zeros(c["ln_stats"], M, 2, dtype=torch.float32, device="cuda")
                st[0, :, 0] = A.float().sum(1); st[0, :, 1] = (A.float() ** 2).sum(1)
                kw["ln_stats"] = st
        if c["rowstat"]:
            kw["rowstat"] = torch.zeros(c["rowstat"], M, 2, dtype=torch.float32, device="cuda")
            outs.append(kw["rowstat"])
        op = O.Gemm(A, W, C, **kw)
        outs.append(C)
    elif kind == "conv":
        k, s = c["k"], c["stride"]
        pad = k // 2
        B, H, Wd, Cin, Cout = c["B"], c["H"], c["W"], c["Cin"], c["Cout"]
        Ho, Wo = (H + 2 * pad - k) // s + 1, (Wd + 2 * pad - k) // s + 1
        x, w = rnd(B, H, Wd, Cin), rnd(Cout, k, k, Cin, scale=(Cin * k * k) ** -0.5)
        y = torch.zeros(B, Ho, Wo, Cout, dtype=BF, device="cuda")
        op = O.Conv(x, w, y, bias=rnd(Cout, dtype=torch.float32) if c["bias"] else None, R=rnd(B, Ho, Wo, Cout) if c["res"] else None,
                    temb=rnd(B, Cout, dtype=torch.float32) if c["temb"] else None, temb_b_stride=Cout if c["temb"] else 0, stride=(s, s), pad=(pad, pad),
                    epilogue=c["epi"], splitk=c["splitk"], ws=ws)
        outs.append(y)
    elif kind == "up2":
        B, H, Wd, Cin, Cout, Ho, Wo = c["B"], c["H"], c["W"], c["Cin"], c["Cout"], c["Ho"], c["Wo"]
        nph = (2 + (Ho != 2 * H)) * (2 + (Wo != 2 * Wd))
        x, w = rnd(B, H, Wd, Cin), rnd(nph, Cout, 2, 2, Cin, scale=(Cin * 4) ** -0.5)
        y = torch.zeros(B, Ho, Wo, Cout, dtype=BF, device="cuda")
        op = O.Conv(x, w, y, bias=rnd(Cout, dtype=torch.float32) if c["bias"] else None, upsample2x=True, ws=ws)
        outs.append(y)
    else:
        Bt, T, Cc = c["Bt"], c["T"], c["Cc"]
        X, Wv = rnd(Bt, T, Cc), rnd(Cc, Cc, scale=Cc ** -0.5)
        Vt = torch.zeros(Bt, Cc, (T + 7) // 8 * 8, dtype=BF, device="cuda")
        op = O.Gemm(Wv, X, Vt[:, :, :T])
        outs.append(Vt)
    with L.options(**c["opts"]):
        O.run_ops([op])
        tag = (L.lib().mdx_last_kernel() or b"").decode()
        torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in outs:
        h.update(t.contiguous().view(torch.uint8).cpu().numpy().tobytes())
    return tag, h.hexdigest()
