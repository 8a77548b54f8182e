#!/usr/bin/env python3
"""ISA identity of the kernels of two source trees: `tools/isa_compare.py <parent tree> [<this tree>] > profiles/<name>_isa.log`.

Every kernel source of csrc/Makefile's KSRCS is compiled to gfx950 assembly (the Makefile's CXXFLAGS + --cuda-device-only -S), once plain
(bf16) and once with -DMDX_F16=1 -Dmdx=mdx_f16, in both trees.  Compared per kernel symbol: the instruction text from the symbol's label to
its s_endpgm-terminated end (local label numbers normalised), every .amdhsa_ directive except .amdhsa_kernarg_size, and the metadata fields
vgpr / agpr / sgpr counts, spill counts, LDS and scratch size.  Needs hipcc; no GPU."""
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

FLAGS = "-O3 -std=c++17 --offload-arch=gfx950 -fPIC -ffp-contract=fast -mllvm -amdgpu-mfma-vgpr-form -Wall -Wno-unused-function".split()
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def ksrcs(tree):
    mk = open(os.path.join(tree, "magicdrive_amd", "csrc", "Makefile")).read()
    return re.search(r"^KSRCS = (.*)$", mk, re.M).group(1).split()


def compile_s(tree, src, f16, out):
    extra = ["-DMDX_F16=1", "-Dmdx=mdx_f16"] if f16 else []
    r = subprocess.run([HIPCC] + FLAGS + extra + ["--cuda-device-only", "-S", os.path.join(tree, "magicdrive_amd", "csrc", src), "-o", out], capture_output=True, text=True)
    if r.returncode:                 # keep the compiler's diagnostic (its warnings on success are dropped)
        sys.stderr.write(r.stderr)
        raise RuntimeError(f"hipcc failed on {src}{' (f16)' if f16 else ''}")


def kernels(path):
    """{symbol: (normalised text, directives, metadata dict)}"""
    txt = open(path).read()
    out = {}
    meta = {}
    for m in re.finditer(r"  - \.agpr_count:.*?(?=\n  - \.agpr_count:|\namdhsa\.target|\Z)", txt, re.S):
        blk = m.group(0)
        sym = re.search(r"\.symbol:\s+(\S+)\.kd", blk).group(1)
        g = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1))
        meta[sym] = dict(vgpr=g("vgpr_count"), agpr=g("agpr_count"), sgpr=g("sgpr_count"), spill_s=g("sgpr_spill_count"), spill_v=g("vgpr_spill_count"),
                         lds=g("group_segment_fixed_size"), scratch=g("private_segment_fixed_size"))
    for sym in meta:
        m = re.search(r"^%s:.*?\n(.*?)^\s*\.amdhsa_kernel %s\n(.*?)\.end_amdhsa_kernel" % (re.escape(sym), re.escape(sym)), txt, re.S | re.M)
        body, dirs = m.group(1), m.group(2)
        lines = [l.split(";")[0].rstrip() for l in body.splitlines()]
        lines = [l for l in lines if l.strip() and not l.strip().startswith((".p2align", ".section", ".size", ".type", ".rodata", ".Lfunc_end", ".set", ".text", ".protected", ".globl", ".weak"))]
        norm = re.sub(r"\.LBB\d+_", ".LBB_", "\n".join(lines))
        dirs = "\n".join(l.strip() for l in dirs.splitlines() if ".amdhsa_kernarg_size" not in l)
        n_instr = sum(1 for l in lines if not l.strip().endswith(":"))
        out[sym] = (norm, dirs, meta[sym], n_instr)
    return out


def demangle(sym):
    for tool in ("/opt/rocm/llvm/bin/llvm-cxxfilt", "/opt/rocm/lib/llvm/bin/llvm-cxxfilt", "llvm-cxxfilt", "c++filt"):
        try:
            return subprocess.run([tool, sym], capture_output=True, text=True, check=True).stdout.strip()
        except Exception:
            continue
    return sym


def main():
    parent = os.path.abspath(sys.argv[1])
    new = os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tmp = tempfile.mkdtemp(prefix="isa_")
    try:
        return compare(parent, new, tmp)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def compare(parent, new, tmp):
    jobs = []
    for tag, tree in (("parent", parent), ("new", new)):
        for src in ksrcs(tree):
            for f16 in (False, True):
                jobs.append((tree, src, f16, os.path.join(tmp, f"{tag}_{src[:-4]}{'_f16' if f16 else ''}.s")))
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:
        list(ex.map(lambda j: compile_s(*j), jobs))
    names = sorted({os.path.basename(j[3]).split("_", 1)[1] for j in jobs})
    tot_p = tot_n = n_diff = n_new = n_gone = 0
    body = []
    for nm in names:
        pp, pn = os.path.join(tmp, "parent_" + nm), os.path.join(tmp, "new_" + nm)
        kp = kernels(pp) if os.path.exists(pp) else {}
        kn = kernels(pn) if os.path.exists(pn) else {}
        tot_p += len(kp); tot_n += len(kn)
        body.append(f"== {nm}: parent {len(kp)} kernel symbols, new {len(kn)}")
        for sym, (text, dirs, md, ni) in kn.items():
            if sym not in kp:
                verdict = "NEW      "; n_new += 1
            elif kp[sym][:3] == (text, dirs, md):
                verdict = "identical"
            else:
                verdict = "DIFFERS  "; n_diff += 1
            body.append(f"  {verdict} {ni:6d} instr  vgpr {md['vgpr']} agpr {md['agpr']} sgpr {md['sgpr']} spill {md['spill_s']}/{md['spill_v']} lds {md['lds']} "
                        f"scratch {md['scratch']}  {demangle(sym)}")
        for sym in kp:
            if sym not in kn:
                body.append(f"  REMOVED   {demangle(sym)}"); n_gone += 1
    print("# ISA identity of the kernels: parent tree vs this tree (tools/isa_compare.py).  Every KSRCS source compiled with the Makefile CXXFLAGS +")
    print("# --cuda-device-only -S, once plain (bf16) and once with -DMDX_F16=1 -Dmdx=mdx_f16; compared per kernel symbol (instruction text, .amdhsa_")
    print("# directives except .amdhsa_kernarg_size, register / spill / LDS / scratch metadata).")
    print(f"# kernel symbols: parent {tot_p}, new {tot_n}; existing symbols that differ: {n_diff}; symbols without a parent: {n_new}; parent symbols removed: {n_gone}")
    print("#")
    print("\n".join(body))
    return 1 if n_diff or n_gone else 0


if __name__ == "__main__":
    sys.exit(main())
