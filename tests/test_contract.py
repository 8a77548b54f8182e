"""CPU: the host-side contract of every C-ABI entry point (include/mdx.h, the "Requirements" of each descriptor).

One valid descriptor per entry point and, per contract clause, ONE mutation of it that violates only that clause.  Every mutated descriptor
must come back with the documented code (MDX_EINVAL, or MDX_EUNSUPPORTED where the header says so) and a message that names the field —
through the bf16 symbol, the _f16 symbol and a one-op mdx_program_run.  Pointers are plain integers with the wanted alignment: a check
that is missing shows up here as a launch attempt (MDX_ELAUNCH on a machine without a device), never as a memory access.  For that reason
the module refuses to run where a device is visible, and the unmutated descriptors are never called (tests/test_edges_gpu.py runs the
least-aligned ACCEPTED descriptors on the device).
"""
import ctypes

import pytest
import torch

from magicdrive_amd import _lib as L

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="fake device pointers: the rejection table must not run where a launch could succeed")

EINVAL, EUNSUPPORTED = -1, -3
BIG = 1 << 31                       # first value that does not fit a 32-bit int
P = lambda k: 0x10000000 * k        # fake, 256 MiB apart, aligned to everything


def gemm(**kw):
    d = dict(A=P(1), W=P(2), C=P(3), M=64, N=64, K=64, lda=64, ldw=64, ldc=64)
    d.update(kw); return d


def conv(**kw):
    d = dict(X=P(1), Wt=P(2), Y=P(3), B=1, Hi=8, Wi=8, Cin=8, Ho=8, Wo=8, Cout=8, kh=3, kw=3, sh=1, sw=1, ph=1, pw=1, ldx=8, ldy=8)
    d.update(kw); return d


def convd(**kw):
    d = dict(X=P(1), Wt=P(2), Y=P(3), B=1, Hi=8, Wi=8, Cin=4, Ho=8, Wo=8, Cout=4, kh=3, kw=3, sh=1, sw=1, ph=1, pw=1, ldx=4, ldy=4)
    d.update(kw); return d


def attn(**kw):
    d = dict(Q=P(1), K=P(2), Vt=P(3), O=P(4), B=1, H=1, Tq=8, Tk=8, d=8, nsrc=1, ldq=8, sQ=64, ldk=8, sK=64, ldv=8, sV=64, ldo=8, sO=64, scale=1.0)
    d.update(kw); return d


def gn(**kw):
    d = dict(X=P(1), Y=P(2), gamma=P(3), beta=P(4), B=1, HW=4, C=8, G=2, ldx=8, ldy=8, eps=1e-5)
    d.update(kw); return d


def ln(**kw):
    d = dict(X=P(1), Y=P(2), gamma=P(3), beta=P(4), M=4, C=8, ldx=8, ldy=8, eps=1e-5)
    d.update(kw); return d


def sm(**kw):
    d = dict(X=P(1), Y=P(2), rows=4, T=8, ldx=8, ldy=8, scale=1.0)
    d.update(kw); return d


def ew(**kw):
    d = dict(X=P(1), Y=P(2), kind=L.EW_COPY, M=4, C=8, ldx=8, ldy=8)
    d.update(kw); return d


def fourier(**kw):
    d = dict(X=P(1), Y=P(2), n=2, P=1, F=2, ldy=16)
    d.update(kw); return d


def gather(**kw):
    d = dict(T=P(1), Y=P(2), idx=P(3), n=2, C=8, ldt=8, ldy=8, n_rows=4)
    d.update(kw); return d


def timeemb(**kw):
    d = dict(t=P(1), Y=P(2), n=2, dim=8, ldy=8, max_period=10000.0)
    d.update(kw); return d


def ddim(**kw):
    d = dict(x=P(1), eps=P(2), coef=P(3), step_ptr=P(4), n=64)
    d.update(kw); return d


def unipc(**kw):
    d = dict(x=P(1), eps=P(2), coef=P(3), step_ptr=P(4), x_last=P(5), m1=P(6), m2=P(7), n=64)
    d.update(kw); return d


# (opcode, clause of include/mdx.h, descriptor, expected code, what mdx_last_error() must name)
TABLE = [
    # ---- mdx_gemm_bf16 ---------------------------------------------------------------------------------------------------------------
    (L.OP_GEMM, "null operand", gemm(A=0), EINVAL, "null operand"),
    (L.OP_GEMM, "null operand", gemm(W=0), EINVAL, "null operand"),
    (L.OP_GEMM, "null operand", gemm(C=0), EINVAL, "null operand"),
    (L.OP_GEMM, "M, N, K, batch, rows_per_b, splitk fit a 32-bit int", gemm(M=BIG), EINVAL, "M="),
    (L.OP_GEMM, "M, N, K, batch, rows_per_b, splitk fit a 32-bit int", gemm(N=BIG), EINVAL, "N="),
    (L.OP_GEMM, "M, N, K, batch, rows_per_b, splitk fit a 32-bit int", gemm(K=BIG), EINVAL, "K="),
    (L.OP_GEMM, "M, N, K, batch, rows_per_b, splitk fit a 32-bit int", gemm(batch=BIG), EINVAL, "batch="),
    (L.OP_GEMM, "M, N, K, batch, rows_per_b, splitk fit a 32-bit int", gemm(rows_per_b=BIG), EINVAL, "rows_per_b="),
    (L.OP_GEMM, "M, N, K, batch, rows_per_b, splitk fit a 32-bit int", gemm(splitk=BIG), EINVAL, "splitk="),
    (L.OP_GEMM, "K % 8 == 0", gemm(K=68), EINVAL, "K=68"),
    (L.OP_GEMM, "lda % 8 == 0", gemm(lda=68), EINVAL, "lda="),
    (L.OP_GEMM, "ldw % 8 == 0", gemm(ldw=68), EINVAL, "ldw="),
    (L.OP_GEMM, "A and W 16-byte aligned", gemm(A=P(1) + 8), EINVAL, "A must be 16-byte"),
    (L.OP_GEMM, "A and W 16-byte aligned", gemm(W=P(2) + 8), EINVAL, "W must be 16-byte"),
    (L.OP_GEMM, "ldc % 4 == 0", gemm(ldc=66), EINVAL, "ldc="),
    (L.OP_GEMM, "ldr % 4 == 0", gemm(R=P(4), ldr=66), EINVAL, "ldr="),
    (L.OP_GEMM, "C and R 8-byte aligned", gemm(C=P(3) + 4), EINVAL, "C must be 8-byte"),
    (L.OP_GEMM, "C and R 8-byte aligned", gemm(R=P(4) + 4, ldr=64), EINVAL, "R must be 8-byte"),
    (L.OP_GEMM, "c_is_f32: C and R must be 16-byte aligned", gemm(c_is_f32=1, C=P(3) + 8), EINVAL, "C (fp32) must be 16-byte"),
    (L.OP_GEMM, "c_is_f32: C and R must be 16-byte aligned", gemm(c_is_f32=1, R=P(4) + 8, ldr=64), EINVAL, "R (fp32) must be 16-byte"),
    (L.OP_GEMM, "c_is_f32: C and R must be 16-byte aligned (under split-K too)", gemm(c_is_f32=1, R=P(4) + 8, ldr=64, K=2048, lda=2048, ldw=2048, splitk=4, ws=P(5), ws_bytes=1 << 20),
     EINVAL, "R (fp32) must be 16-byte"),
    (L.OP_GEMM, "bias and temb must be 16-byte aligned", gemm(bias=P(5) + 8), EINVAL, "bias must be 16-byte"),
    (L.OP_GEMM, "bias and temb must be 16-byte aligned", gemm(bias=P(5) + 4), EINVAL, "bias must be 16-byte"),
    (L.OP_GEMM, "bias and temb must be 16-byte aligned", gemm(temb=P(5) + 8, temb_b_stride=64), EINVAL, "temb must be 16-byte"),
    (L.OP_GEMM, "temb_sel_stride % 4 == 0", gemm(temb=P(5), temb_sel_stride=130, temb_b_stride=64), EINVAL, "temb_sel_stride="),
    (L.OP_GEMM, "temb_b_stride % 4 == 0", gemm(temb=P(5), temb_sel_stride=128, temb_b_stride=66), EINVAL, "temb_b_stride="),
    (L.OP_GEMM, "sel_ptr 4-byte aligned", gemm(temb=P(5), temb_b_stride=64, sel_ptr=P(6) + 2), EINVAL, "sel_ptr must be 4-byte"),
    (L.OP_GEMM, "ws must be 16-byte aligned", gemm(ws=P(5) + 8, ws_bytes=1 << 20), EINVAL, "ws must be 16-byte"),
    (L.OP_GEMM, "a split with ws_bytes > 0 and ws == NULL is refused", gemm(K=2048, lda=2048, ldw=2048, splitk=4, ws_bytes=1 << 20), EINVAL, "split-K needs a workspace"),
    (L.OP_GEMM, "batch > 1: sA % 8 == 0", gemm(batch=2, sA=4100, sW=4096, sC=4096), EINVAL, "sA="),
    (L.OP_GEMM, "batch > 1: sW % 8 == 0", gemm(batch=2, sA=4096, sW=4100, sC=4096), EINVAL, "sW="),
    (L.OP_GEMM, "batch > 1: sC % 4 == 0", gemm(batch=2, sA=4096, sW=4096, sC=4098), EINVAL, "sC="),
    (L.OP_GEMM, "batch > 1: sR % 4 == 0", gemm(batch=2, sA=4096, sW=4096, sC=4096, R=P(4), ldr=64, sR=4098), EINVAL, "sR="),
    (L.OP_GEMM, "N % 4 != 0 needs a plain epilogue and ldc >= roundup4(N)", gemm(N=62, bias=P(5)), EINVAL, "N=62"),
    (L.OP_GEMM, "N % 4 != 0 needs a plain epilogue and ldc >= roundup4(N)", gemm(N=62, ldc=60), EINVAL, "N=62"),
    (L.OP_GEMM, "MDX_EPI_GEGLU needs N % 64 == 0", gemm(N=96, epilogue=L.EPI_GEGLU), EINVAL, "N=96"),
    (L.OP_GEMM, "Vt: needs K == 320, vt_from % 128 == 0, ...", gemm(Vt=P(5), vt_from=32, vt_T=8, vt_ld=8, vt_stride=64), EINVAL, "transposed V"),
    (L.OP_GEMM, "Vt: 16-byte aligned Vt rows", gemm(M=64, N=256, K=320, lda=320, ldw=320, ldc=128, Vt=P(5) + 8, vt_from=128, vt_T=8, vt_ld=8, vt_stride=1024), EINVAL, "aligned Vt"),
    (L.OP_GEMM, "ln_eps: needs ln_csum", gemm(ln_eps=1e-5), EINVAL, "ln_csum"),
    (L.OP_GEMM, "ln_eps: 16-byte aligned ln_scratch", gemm(ln_eps=1e-5, ln_csum=P(5), ln_scratch=P(6) + 8), EINVAL, "ln_scratch"),
    (L.OP_GEMM, "ln_stats without ln_eps", gemm(ln_stats=P(5), ln_stats_parts=1), EINVAL, "ln_stats"),
    (L.OP_GEMM, "ln_stats: parts >= 1, 8-byte aligned", gemm(ln_eps=1e-5, ln_csum=P(5), ln_stats=P(6) + 4, ln_stats_parts=1), EINVAL, "ln_stats"),
    (L.OP_GEMM, "rowstat_out: rowstat_parts >= 1", gemm(rowstat_out=P(5), rowstat_parts=0), EINVAL, "rowstat_out"),
    (L.OP_GEMM, "rowstat_out: 8-byte aligned", gemm(rowstat_out=P(5) + 4, rowstat_parts=1), EINVAL, "rowstat_out"),
    (L.OP_GEMM, "rowstat_out: 16-bit C", gemm(rowstat_out=P(5), rowstat_parts=1, c_is_f32=1), EINVAL, "rowstat_out"),
    (L.OP_GEMM, "Wq must be 16-byte aligned", gemm(Wq=P(5) + 8), EINVAL, "Wq"),
    # ---- mdx_conv2d_bf16 -------------------------------------------------------------------------------------------------------------
    (L.OP_CONV, "null operand", conv(X=0), EINVAL, "null operand"),
    (L.OP_CONV, "Cin % 8 == 0", conv(Cin=4), EINVAL, "Cin=4"),
    (L.OP_CONV, "Cout % 4 == 0", conv(Cout=6), EINVAL, "Cout=6"),
    (L.OP_CONV, "no GEGLU epilogue", conv(epilogue=L.EPI_GEGLU), EINVAL, "GEGLU"),
    (L.OP_CONV, "every size field fits a 32-bit int", conv(B=BIG), EINVAL, "B="),
    (L.OP_CONV, "every size field fits a 32-bit int", conv(Cout=BIG), EINVAL, "Cout="),
    (L.OP_CONV, "Ho * Wo fits a 32-bit int", conv(Ho=1 << 16, Wo=1 << 16), EINVAL, "Ho * Wo="),
    (L.OP_CONV, "B * Ho * Wo fits a 32-bit int", conv(B=1 << 26), EINVAL, "B * Ho * Wo="),
    (L.OP_CONV, "kh * kw * Cin fits a 32-bit int", conv(Cin=1 << 29), EINVAL, "kh * kw * Cin="),
    (L.OP_CONV, "ldx % 8 == 0", conv(ldx=12), EINVAL, "ldx="),
    (L.OP_CONV, "ldy % 4 == 0", conv(ldy=10), EINVAL, "ldy="),
    (L.OP_CONV, "ldr % 4 == 0", conv(R=P(4), ldr=10), EINVAL, "ldr="),
    (L.OP_CONV, "X and Wt 16-byte aligned", conv(X=P(1) + 8), EINVAL, "X must be 16-byte"),
    (L.OP_CONV, "X and Wt 16-byte aligned", conv(Wt=P(2) + 8), EINVAL, "Wt must be 16-byte"),
    (L.OP_CONV, "Y and R 8-byte aligned", conv(Y=P(3) + 4), EINVAL, "Y must be 8-byte"),
    (L.OP_CONV, "Y and R 8-byte aligned", conv(R=P(4) + 4, ldr=8), EINVAL, "R must be 8-byte"),
    (L.OP_CONV, "bias and temb must be 16-byte aligned", conv(bias=P(5) + 8), EINVAL, "bias must be 16-byte"),
    (L.OP_CONV, "bias and temb must be 16-byte aligned", conv(temb=P(5) + 8, temb_b_stride=8), EINVAL, "temb must be 16-byte"),
    (L.OP_CONV, "temb_sel_stride % 4 == 0", conv(temb=P(5), temb_sel_stride=18, temb_b_stride=8), EINVAL, "temb_sel_stride="),
    (L.OP_CONV, "temb_b_stride % 4 == 0", conv(temb=P(5), temb_sel_stride=16, temb_b_stride=10), EINVAL, "temb_b_stride="),
    (L.OP_CONV, "sel_ptr 4-byte aligned", conv(temb=P(5), temb_b_stride=8, sel_ptr=P(6) + 2), EINVAL, "sel_ptr must be 4-byte"),
    (L.OP_CONV, "ws 16-byte aligned", conv(ws=P(5) + 8, ws_bytes=1 << 20), EINVAL, "ws must be 16-byte"),
    # ---- mdx_conv2d_direct -----------------------------------------------------------------------------------------------------------
    (L.OP_CONV_DIRECT, "null operand", convd(Wt=0), EINVAL, "null operand"),
    (L.OP_CONV_DIRECT, "no GEGLU epilogue", convd(epilogue=L.EPI_GEGLU), EINVAL, "GEGLU"),
    (L.OP_CONV_DIRECT, "natural alignment", convd(X=P(1) + 1), EINVAL, "X must be 2-byte"),
    (L.OP_CONV_DIRECT, "natural alignment", convd(x_is_f32=1, X=P(1) + 2), EINVAL, "X must be 4-byte"),
    (L.OP_CONV_DIRECT, "natural alignment", convd(Wt=P(2) + 1), EINVAL, "Wt must be 2-byte"),
    (L.OP_CONV_DIRECT, "natural alignment", convd(y_is_f32=1, Y=P(3) + 2), EINVAL, "Y must be 4-byte"),
    (L.OP_CONV_DIRECT, "natural alignment", convd(R=P(4) + 1, ldr=4), EINVAL, "R must be 2-byte"),
    (L.OP_CONV_DIRECT, "natural alignment", convd(bias=P(4) + 2), EINVAL, "bias must be 4-byte"),
    (L.OP_CONV_DIRECT, "natural alignment", convd(temb=P(4) + 2), EINVAL, "temb must be 4-byte"),
    (L.OP_CONV_DIRECT, "natural alignment", convd(temb=P(4), sel_ptr=P(5) + 2), EINVAL, "sel_ptr must be 4-byte"),
    (L.OP_CONV_DIRECT, "every size field fits a 32-bit int", convd(Hi=BIG), EINVAL, "Hi="),
    (L.OP_CONV_DIRECT, "B * Ho * Wo fits a 32-bit int", convd(B=1 << 26), EINVAL, "B * Ho * Wo="),
    (L.OP_CONV_DIRECT, "kh * kw * Cin fits a 32-bit int", convd(Cin=1 << 29), EINVAL, "kh * kw * Cin="),
    # ---- mdx_attention_bf16 ----------------------------------------------------------------------------------------------------------
    (L.OP_ATTN, "null operand", attn(O=0), EINVAL, "null operand"),
    (L.OP_ATTN, "d % 8 == 0", attn(d=12), EINVAL, "d=12"),
    (L.OP_ATTN, "0 < d <= 160", attn(d=168), EINVAL, "d=168"),
    (L.OP_ATTN, "0 < d <= 160", attn(d=0), EINVAL, "d=0"),
    (L.OP_ATTN, "d = 104, 112, 136, 144 return MDX_EUNSUPPORTED", attn(d=104), EUNSUPPORTED, "d=104"),
    (L.OP_ATTN, "d = 104, 112, 136, 144 return MDX_EUNSUPPORTED", attn(d=112), EUNSUPPORTED, "d=112"),
    (L.OP_ATTN, "d = 104, 112, 136, 144 return MDX_EUNSUPPORTED", attn(d=136), EUNSUPPORTED, "d=136"),
    (L.OP_ATTN, "d = 104, 112, 136, 144 return MDX_EUNSUPPORTED", attn(d=144), EUNSUPPORTED, "d=144"),
    (L.OP_ATTN, "ldq, ldk, ldv, sQ, sK, sV multiples of 8", attn(ldq=12), EINVAL, "ldq="),
    (L.OP_ATTN, "ldq, ldk, ldv, sQ, sK, sV multiples of 8", attn(ldk=12), EINVAL, "ldk="),
    (L.OP_ATTN, "ldq, ldk, ldv, sQ, sK, sV multiples of 8", attn(ldv=12), EINVAL, "ldv="),
    (L.OP_ATTN, "ldq, ldk, ldv, sQ, sK, sV multiples of 8", attn(sQ=68), EINVAL, "sQ="),
    (L.OP_ATTN, "ldq, ldk, ldv, sQ, sK, sV multiples of 8", attn(sK=68), EINVAL, "sK="),
    (L.OP_ATTN, "ldq, ldk, ldv, sQ, sK, sV multiples of 8", attn(sV=68), EINVAL, "sV="),
    (L.OP_ATTN, "Q, K, Vt 16-byte aligned", attn(Q=P(1) + 8), EINVAL, "Q must be 16-byte"),
    (L.OP_ATTN, "Q, K, Vt 16-byte aligned", attn(K=P(2) + 8), EINVAL, "K must be 16-byte"),
    (L.OP_ATTN, "Q, K, Vt 16-byte aligned", attn(Vt=P(3) + 8), EINVAL, "Vt must be 16-byte"),
    (L.OP_ATTN, "ldv >= Tk", attn(Tk=16), EINVAL, "ldv < Tk"),
    (L.OP_ATTN, "ldo % 4 == 0", attn(ldo=10), EINVAL, "ldo="),
    (L.OP_ATTN, "sO % 4 == 0", attn(sO=66), EINVAL, "sO="),
    (L.OP_ATTN, "O must be 8-byte aligned", attn(O=P(4) + 4), EINVAL, "O must be 8-byte"),
    (L.OP_ATTN, "B, H, Tq, Tk fit a 32-bit int", attn(Tq=BIG), EINVAL, "Tq="),
    (L.OP_ATTN, "B, H, Tq, Tk fit a 32-bit int", attn(B=BIG), EINVAL, "B="),
    (L.OP_ATTN, "joint must be 0 or 1", attn(joint=2), EINVAL, "joint"),
    (L.OP_ATTN, "nsrc must be 1..2 (joint: 1..8)", attn(nsrc=3, kvmap=P(5)), EINVAL, "nsrc"),
    (L.OP_ATTN, "nsrc must be 1..2 (joint: 1..8)", attn(nsrc=9, joint=1, kvmap=P(5)), EINVAL, "nsrc"),
    (L.OP_ATTN, "nsrc > 1 needs a kvmap", attn(nsrc=2), EINVAL, "kvmap"),
    (L.OP_ATTN, "kvmap 4-byte aligned", attn(nsrc=2, kvmap=P(5) + 2), EINVAL, "kvmap must be 4-byte"),
    (L.OP_ATTN, "q_prescaled must be 0 or 1", attn(q_prescaled=2), EINVAL, "q_prescaled"),
    # ---- mdx_groupnorm_bf16 ----------------------------------------------------------------------------------------------------------
    (L.OP_GROUPNORM, "null operand", gn(gamma=0), EINVAL, "null operand"),
    (L.OP_GROUPNORM, "G > 0 and C % G == 0", gn(G=3), EINVAL, "G=3"),
    (L.OP_GROUPNORM, "G > 0 and C % G == 0", gn(G=0), EINVAL, "G=0"),
    (L.OP_GROUPNORM, "0 < C <= ldx, ldy", gn(ldx=4), EINVAL, "ldx"),
    (L.OP_GROUPNORM, "0 < C <= ldx, ldy", gn(ldy=4), EINVAL, "ldy"),
    (L.OP_GROUPNORM, "B, HW, C, G fit a 32-bit int", gn(HW=BIG), EINVAL, "HW="),
    (L.OP_GROUPNORM, "B, HW, C, G fit a 32-bit int", gn(C=BIG, G=2, ldx=BIG, ldy=BIG), EINVAL, "C="),
    (L.OP_GROUPNORM, "gamma, beta must be 16-byte aligned", gn(gamma=P(3) + 8), EINVAL, "gamma must be 16-byte"),
    (L.OP_GROUPNORM, "gamma, beta must be 16-byte aligned", gn(beta=P(4) + 4), EINVAL, "beta must be 16-byte"),
    (L.OP_GROUPNORM, "ws must be 16-byte aligned", gn(ws=P(5) + 8, ws_bytes=1 << 20), EINVAL, "ws must be 16-byte"),
    (L.OP_GROUPNORM, "X / Y at any 2-byte alignment", gn(X=P(1) + 1), EINVAL, "X must be 2-byte"),
    (L.OP_GROUPNORM, "X / Y at any 2-byte alignment", gn(Y=P(2) + 1), EINVAL, "Y must be 2-byte"),
    (L.OP_GROUPNORM, "MDX_EUNSUPPORTED: more than 2560 channels per group on the one-launch kernel", gn(C=4096, G=1, ldx=4096, ldy=4096), EUNSUPPORTED, "channels per group"),
    (L.OP_GROUPNORM, "MDX_EUNSUPPORTED: ... (a workspace does not help a small tensor)", gn(C=4096, G=1, ldx=4096, ldy=4096, ws=P(5), ws_bytes=1 << 20), EUNSUPPORTED, "channels per group"),
    # ---- mdx_layernorm_bf16 ----------------------------------------------------------------------------------------------------------
    (L.OP_LAYERNORM, "null operand", ln(beta=0), EINVAL, "null operand"),
    (L.OP_LAYERNORM, "C, ldx, ldy must be multiples of 8", ln(C=4), EINVAL, "C=4"),
    (L.OP_LAYERNORM, "C, ldx, ldy must be multiples of 8", ln(ldx=12), EINVAL, "ldx="),
    (L.OP_LAYERNORM, "C, ldx, ldy must be multiples of 8", ln(ldy=12), EINVAL, "ldy="),
    (L.OP_LAYERNORM, "0 < C <= ldx, ldy", ln(C=16), EINVAL, "ldx"),
    (L.OP_LAYERNORM, "X, Y, gamma, beta must be 16-byte aligned", ln(X=P(1) + 8), EINVAL, "X must be 16-byte"),
    (L.OP_LAYERNORM, "X, Y, gamma, beta must be 16-byte aligned", ln(Y=P(2) + 8), EINVAL, "Y must be 16-byte"),
    (L.OP_LAYERNORM, "X, Y, gamma, beta must be 16-byte aligned", ln(gamma=P(3) + 8), EINVAL, "gamma must be 16-byte"),
    (L.OP_LAYERNORM, "X, Y, gamma, beta must be 16-byte aligned", ln(beta=P(4) + 8), EINVAL, "beta must be 16-byte"),
    (L.OP_LAYERNORM, "M fits a 32-bit int", ln(M=BIG), EINVAL, "M="),
    (L.OP_LAYERNORM, "C > 2048 returns MDX_EUNSUPPORTED", ln(C=4096, ldx=4096, ldy=4096), EUNSUPPORTED, "C=4096"),
    # ---- mdx_softmax_rows ------------------------------------------------------------------------------------------------------------
    (L.OP_SOFTMAX, "null operand", sm(X=0), EINVAL, "null operand"),
    (L.OP_SOFTMAX, "0 < T <= ldx, ldy", sm(T=0), EINVAL, "T"),
    (L.OP_SOFTMAX, "0 < T <= ldx, ldy", sm(ldx=4), EINVAL, "ldx"),
    (L.OP_SOFTMAX, "0 < T <= ldx, ldy", sm(ldy=4), EINVAL, "ldy"),
    (L.OP_SOFTMAX, "rows, T, ldy fit a 32-bit int", sm(rows=BIG), EINVAL, "rows="),
    (L.OP_SOFTMAX, "rows, T, ldy fit a 32-bit int", sm(ldy=BIG), EINVAL, "ldy="),
    (L.OP_SOFTMAX, "X 4-byte, Y 2-byte aligned", sm(X=P(1) + 2), EINVAL, "X must be 4-byte"),
    (L.OP_SOFTMAX, "X 4-byte, Y 2-byte aligned", sm(Y=P(2) + 1), EINVAL, "Y must be 2-byte"),
    # ---- mdx_elementwise -------------------------------------------------------------------------------------------------------------
    (L.OP_EW, "null operand", ew(Y=0), EINVAL, "null operand"),
    (L.OP_EW, "a known kind", ew(kind=99), EINVAL, "kind 99"),
    (L.OP_EW, "natural alignment", ew(X=P(1) + 1), EINVAL, "X must be 2-byte"),
    (L.OP_EW, "natural alignment", ew(x_is_f32=1, X=P(1) + 2), EINVAL, "X must be 4-byte"),
    (L.OP_EW, "natural alignment", ew(y_is_f32=1, Y=P(2) + 2), EINVAL, "Y must be 4-byte"),
    (L.OP_EW, "C, B, Hi, Wi, Ho, Wo fit a 32-bit int", ew(C=BIG), EINVAL, "C="),
    (L.OP_EW, "C, B, Hi, Wi, Ho, Wo fit a 32-bit int", ew(kind=L.EW_NCHW_TO_NHWC, B=1, Hi=BIG, Wi=2), EINVAL, "Hi="),
    (L.OP_EW, "MDX_EW_UPSAMPLE needs ymap / xmap", ew(kind=L.EW_UPSAMPLE, B=1, Hi=2, Wi=2, Ho=4, Wo=4), EINVAL, "ymap"),
    (L.OP_EW, "natural alignment", ew(kind=L.EW_UPSAMPLE, B=1, Hi=2, Wi=2, Ho=4, Wo=4, ymap=P(3) + 2, xmap=P(4)), EINVAL, "ymap must be 4-byte"),
    # ---- mdx_fourier_embed / mdx_gather_rows / mdx_timestep_embedding ------------------------------------------------------------------
    (L.OP_FOURIER, "null operand", fourier(X=0), EINVAL, "null operand"),
    (L.OP_FOURIER, "0 <= F <= 16", fourier(F=17), EINVAL, "F out of range"),
    (L.OP_FOURIER, "P fits a 32-bit int", fourier(P=BIG), EINVAL, "P="),
    (L.OP_FOURIER, "natural alignment", fourier(X=P(1) + 2), EINVAL, "X must be 4-byte"),
    (L.OP_FOURIER, "natural alignment", fourier(Y=P(2) + 1), EINVAL, "Y must be 2-byte"),
    (L.OP_FOURIER, "natural alignment", fourier(null_feat=P(3) + 2), EINVAL, "null_feat must be 4-byte"),
    (L.OP_GATHER, "null operand", gather(idx=0), EINVAL, "null operand"),
    (L.OP_GATHER, "C and n_rows fit a 32-bit int", gather(C=BIG), EINVAL, "C="),
    (L.OP_GATHER, "C and n_rows fit a 32-bit int", gather(n_rows=BIG), EINVAL, "n_rows="),
    (L.OP_GATHER, "n_rows must be positive", gather(n_rows=0), EINVAL, "n_rows"),
    (L.OP_GATHER, "idx 8-byte aligned", gather(idx=P(3) + 4), EINVAL, "idx must be 8-byte"),
    (L.OP_GATHER, "T / Y / null_row 2-byte aligned", gather(T=P(1) + 1), EINVAL, "T must be 2-byte"),
    (L.OP_GATHER, "T / Y / null_row 2-byte aligned", gather(null_row=P(4) + 1), EINVAL, "null_row must be 2-byte"),
    (L.OP_TIMEEMB, "null operand", timeemb(t=0), EINVAL, "null operand"),
    (L.OP_TIMEEMB, "dim fits a 32-bit int", timeemb(dim=BIG, ldy=BIG), EINVAL, "dim="),
    (L.OP_TIMEEMB, "ldy >= dim", timeemb(ldy=4), EINVAL, "ldy < dim"),
    (L.OP_TIMEEMB, "t and Y 4-byte aligned", timeemb(t=P(1) + 2), EINVAL, "t must be 4-byte"),
    (L.OP_TIMEEMB, "t and Y 4-byte aligned", timeemb(Y=P(2) + 2), EINVAL, "Y must be 4-byte"),
    # ---- mdx_cfg_ddim_step / mdx_cfg_unipc_step ----------------------------------------------------------------------------------------
    (L.OP_DDIM, "null operand", ddim(step_ptr=0), EINVAL, "null operand"),
    (L.OP_DDIM, "x, eps, coef, step_ptr 4-byte aligned", ddim(x=P(1) + 2), EINVAL, "x must be 4-byte"),
    (L.OP_DDIM, "x, eps, coef, step_ptr 4-byte aligned", ddim(coef=P(3) + 2), EINVAL, "coef must be 4-byte"),
    (L.OP_DDIM, "xin_c, xin_ld, gv_last_step fit a 32-bit int", ddim(xin_ld=BIG, xin_c=4, x_in=P(5)), EINVAL, "xin_ld="),
    (L.OP_DDIM, "xin_ld > 0 needs 0 < xin_c <= xin_ld and xin_c dividing n", ddim(x_in=P(5), xin_ld=4, xin_c=8), EINVAL, "x_in"),
    (L.OP_DDIM, "xin_ld > 0 needs 0 < xin_c <= xin_ld and xin_c dividing n", ddim(x_in=P(5), xin_ld=8, xin_c=5), EINVAL, "x_in"),
    (L.OP_DDIM, "a given-view mode needs gv_noise", ddim(gv_mask=P(5), gv_mode=2, gv_view_elems=8), EINVAL, "gv_noise"),
    (L.OP_DDIM, "mode 1: also gv_cond", ddim(gv_mask=P(5), gv_noise=P(6), gv_mode=1, gv_view_elems=8), EINVAL, "gv_cond"),
    (L.OP_DDIM, "gv_view_elems dividing n", ddim(gv_mask=P(5), gv_noise=P(6), gv_mode=2, gv_view_elems=7), EINVAL, "gv_view_elems"),
    (L.OP_UNIPC, "null operand", unipc(m2=0), EINVAL, "null operand"),
    (L.OP_UNIPC, "x, eps, coef, step_ptr 4-byte aligned", unipc(eps=P(2) + 2), EINVAL, "eps must be 4-byte"),
    (L.OP_UNIPC, "x, eps, coef, step_ptr 4-byte aligned", unipc(step_ptr=P(4) + 2), EINVAL, "step_ptr must be 4-byte"),
    (L.OP_UNIPC, "xin_ld > 0 needs 0 < xin_c <= xin_ld and xin_c dividing n", unipc(x_in=P(8), xin_ld=4, xin_c=8), EINVAL, "x_in"),
    (L.OP_UNIPC, "a given-view mode needs gv_noise", unipc(gv_mask=P(8), gv_mode=2, gv_view_elems=8), EINVAL, "gv_noise"),
    (L.OP_UNIPC, "gv_view_elems dividing n", unipc(gv_mask=P(8), gv_noise=P(9), gv_mode=2, gv_view_elems=7), EINVAL, "gv_view_elems"),
]

# the remaining single-field clauses, one row per field
_INT = "fits a 32-bit int"
for _f in ("Hi", "Wi", "Ho", "Wo", "kh", "kw", "sh", "sw", "ph", "pw", "splitk"):
    TABLE.append((L.OP_CONV, f"every size field {_INT}", conv(**{_f: BIG}), EINVAL, _f + "="))
for _f in ("B", "Wi", "Cin", "Ho", "Wo", "Cout", "kh", "kw", "sh", "sw", "ph", "pw"):
    TABLE.append((L.OP_CONV_DIRECT, f"every size field {_INT}", convd(**{_f: BIG}), EINVAL, _f + "="))
for _f in ("B", "Wi", "Ho", "Wo"):
    TABLE.append((L.OP_EW, f"C, B, Hi, Wi, Ho, Wo {_INT}", ew(**{_f: BIG}), EINVAL, _f + "="))
TABLE += [
    (L.OP_CONV, f"kh * kw {_INT}", conv(kh=1 << 16, kw=1 << 16), EINVAL, "kh * kw="),
    (L.OP_CONV, "sizes are not negative", conv(B=-1), EINVAL, "negative size"),
    (L.OP_CONV_DIRECT, f"Ho * Wo {_INT}", convd(Ho=1 << 16, Wo=1 << 16), EINVAL, "Ho * Wo="),
    (L.OP_CONV_DIRECT, f"kh * kw {_INT}", convd(kh=1 << 16, kw=1 << 16), EINVAL, "kh * kw="),
    (L.OP_CONV_DIRECT, "sizes are not negative", convd(Ho=-1), EINVAL, "negative size"),
    (L.OP_EW, "natural alignment", ew(kind=L.EW_UPSAMPLE, B=1, Hi=2, Wi=2, Ho=4, Wo=4, ymap=P(3), xmap=P(4) + 2), EINVAL, "xmap must be 4-byte"),
    (L.OP_ATTN, f"B, H, Tq, Tk {_INT}", attn(H=BIG), EINVAL, "H="),
    (L.OP_ATTN, f"B, H, Tq, Tk {_INT}", attn(Tk=BIG), EINVAL, "Tk="),
    (L.OP_GROUPNORM, f"B, HW, C, G {_INT}", gn(B=BIG), EINVAL, "B="),
    (L.OP_LAYERNORM, "0 < C <= ldx, ldy", ln(C=16, ldx=16), EINVAL, "ldy"),
    (L.OP_SOFTMAX, f"rows, T, ldy {_INT}", sm(T=BIG, ldx=BIG, ldy=BIG), EINVAL, "T="),
    (L.OP_GATHER, "T / Y / null_row 2-byte aligned", gather(Y=P(2) + 1), EINVAL, "Y must be 2-byte"),
    (L.OP_DDIM, "x, eps, coef, step_ptr 4-byte aligned", ddim(eps=P(2) + 2), EINVAL, "eps must be 4-byte"),
    (L.OP_DDIM, "x, eps, coef, step_ptr 4-byte aligned", ddim(step_ptr=P(4) + 2), EINVAL, "step_ptr must be 4-byte"),
    (L.OP_DDIM, f"xin_c, xin_ld, gv_last_step {_INT}", ddim(xin_c=BIG), EINVAL, "xin_c="),
    (L.OP_DDIM, f"xin_c, xin_ld, gv_last_step {_INT}", ddim(gv_last_step=BIG), EINVAL, "gv_last_step="),
    (L.OP_UNIPC, "x, eps, coef, step_ptr 4-byte aligned", unipc(x=P(1) + 2), EINVAL, "x must be 4-byte"),
    (L.OP_UNIPC, "x, eps, coef, step_ptr 4-byte aligned", unipc(coef=P(3) + 2), EINVAL, "coef must be 4-byte"),
    (L.OP_UNIPC, f"xin_c, xin_ld, gv_last_step {_INT}", unipc(xin_c=BIG), EINVAL, "xin_c="),
    (L.OP_UNIPC, f"xin_c, xin_ld, gv_last_step {_INT}", unipc(xin_ld=BIG, xin_c=4, x_in=P(8)), EINVAL, "xin_ld="),
    (L.OP_UNIPC, f"xin_c, xin_ld, gv_last_step {_INT}", unipc(gv_last_step=BIG), EINVAL, "gv_last_step="),
]
# rows added later go HERE, at the end: the test ids carry the row's index in TABLE
TABLE += [
    (L.OP_GEMM, "Vt: A (M * lda * 2 bytes) below 0x7FFF0000", gemm(M=3355520, N=256, K=320, lda=320, ldw=320, ldc=128, Vt=P(5), vt_from=128, vt_T=8, vt_ld=8, vt_stride=1024),
     EINVAL, "2 GiB buffer window"),
    # the x_in clauses every latent op shares (csrc/latent.h: need_xin; tests/test_xin_contract.py has the whole table for all four ops)
    (L.OP_DDIM, "xin_ld is not negative", ddim(x_in=P(5), xin_ld=-8, xin_c=4), EINVAL, "xin_ld=-8"),
    (L.OP_DDIM, "x_in at its element's alignment (4 / 2 bytes)", ddim(x_in=P(5) + 1, xin_ld=8, xin_c=4), EINVAL, "x_in must be 2-byte"),
    (L.OP_DDIM, "x_in at its element's alignment (4 / 2 bytes)", ddim(x_in=P(5) + 2), EINVAL, "x_in must be 4-byte"),
    (L.OP_UNIPC, "xin_ld is not negative", unipc(x_in=P(8), xin_ld=-8, xin_c=4), EINVAL, "xin_ld=-8"),
    (L.OP_UNIPC, "x_in at its element's alignment (4 / 2 bytes)", unipc(x_in=P(8) + 1, xin_ld=8, xin_c=4), EINVAL, "x_in must be 2-byte"),
    (L.OP_UNIPC, "x_in at its element's alignment (4 / 2 bytes)", unipc(x_in=P(8) + 2), EINVAL, "x_in must be 4-byte"),
    # the checks of the context (tk_dev) and the short-sequence (v_rowmajor) route of mdx_attention_* (tests/test_attn_contract.py has their whole tables)
    (L.OP_ATTN, "tk_dev 4-byte aligned", attn(tk_dev=P(6) + 2, d=16), EINVAL, "tk_dev must be 4-byte"),
    (L.OP_ATTN, "tk_dev: B * H * ceil(Tq / 128) fits a 32-bit int", attn(tk_dev=P(6), d=16, B=1 << 16, H=1 << 16), EINVAL, "B * H * ceil(Tq / 128)=4294967296"),
    (L.OP_ATTN, "v_rowmajor: B * H fits a 32-bit int", attn(v_rowmajor=1, d=32, B=1 << 16, H=1 << 16, ldv=1 << 21), EINVAL, "B * H=4294967296"),
]


def _desc(opcode, fields):
    d = L.DESC_OF_OP[opcode]()
    names = {f[0] for f in d._fields_}
    for k, v in fields.items():
        assert k in names, (opcode, k)
        setattr(d, k, v)
    return d


def _call(path, opcode, d):
    lib = L.lib()
    if path == "program":
        prog = L.Program([(opcode, d, L.DTYPE_BF16)])
        rc = lib.mdx_program_run(ctypes.byref(prog.buf), 1, None)
    else:
        fn = getattr(lib, L.entry_name(opcode, L.DTYPE_F16 if path == "f16" else L.DTYPE_BF16))
        rc = fn(ctypes.byref(d), None)
    return rc, (lib.mdx_last_error() or b"").decode()


_IDS = [f"{L.ENTRY_OF_OP[op]}-{i}-{names}" for i, (op, _, _, _, names) in enumerate(TABLE)]


@pytest.mark.parametrize("path", ["bf16", "f16", "program"])
@pytest.mark.parametrize("opcode,clause,fields,code,names", TABLE, ids=_IDS)
def test_violation_is_rejected_on_the_host(opcode, clause, fields, code, names, path):
    rc, msg = _call(path, opcode, _desc(opcode, fields))
    assert rc == code, f"{L.ENTRY_OF_OP[opcode]} [{clause}] via {path}: rc={rc} (want {code}): {msg!r}"
    assert names in msg, f"{L.ENTRY_OF_OP[opcode]} [{clause}] via {path}: message {msg!r} does not name {names!r}"
    if path == "program":
        assert msg.startswith("op 0 (opcode %d)" % opcode), msg


def test_every_entry_point_has_rows():
    assert {op for op, *_ in TABLE} == set(L.DESC_OF_OP)


def latent_helper_bodies():
    """{name: body} of the host checks csrc/latent.h shares among the latent ops' entry points (need_xin, need_given_views)."""
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "magicdrive_amd", "csrc", "latent.h")).read()
    bodies = dict(re.findall(r"template <class D> int (need_\w+)\(const char\* op, const D\* d\) \{\n(.*?)\n\}", hdr, re.S))
    assert set(bodies) == {"need_xin", "need_given_views"}, sorted(bodies)
    return bodies


def with_latent_helpers(body):
    """An entry point's body plus the body of each shared helper of csrc/latent.h that it calls."""
    return body + "".join("\n" + hb for name, hb in latent_helper_bodies().items() if name + "(" in body)


def attn_helper_bodies():
    """{name: body} of what mdx_attention_* calls for its checks: the layout checks every attention route shares (csrc/attn.h:
    need_attn_layout) and the routes that run their own checks (attn_short, attn_ctx)."""
    import os
    import re
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "magicdrive_amd", "csrc")
    src = lambda f: open(os.path.join(csrc, f)).read()
    bodies = dict(re.findall(r"inline int (need_attn_layout)\(const char\* op, const MdxAttnDesc\* a\) \{\n(.*?)\n\}", src("attn.h"), re.S))
    for f in ("attention_short.hip", "attention_ctx.hip"):
        bodies.update(re.findall(r"\nint (attn_\w+)\(const MdxAttnDesc\* a, hipStream_t st, const char\* op[^)]*\) \{\n(.*?)\n\}", src(f), re.S))
    assert set(bodies) == {"need_attn_layout", "attn_short", "attn_ctx"}, sorted(bodies)
    return bodies


def with_attn_helpers(body):
    """An entry point's body plus the body of everything of attn_helper_bodies that it calls, followed to the end (a route calls the
    shared layout checks itself)."""
    helpers, seen = attn_helper_bodies(), set()
    while True:
        more = [n for n in helpers if n not in seen and n + "(" in body]
        if not more:
            return body
        seen |= set(more)
        body += "".join("\n" + helpers[n] for n in more)


def _host_checks():
    """(entry point, field) of every need_int / need_multiple / need_aligned call with a literal field name in the entry points' sources."""
    import os
    import re
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "magicdrive_amd", "csrc")
    found = set()
    for fn in ("gemm_conv.hip", "attention.hip", "norm.hip", "elementwise.hip"):
        parts = re.split(r'extern "C" int (mdx_\w+)\(', open(os.path.join(csrc, fn)).read())
        shared = re.findall(r'need_\w+\(op, "([^"]+)"', parts[0])          # helpers ahead of the first entry point (check_epilogue_operands)
        for name, body in zip(parts[1::2], parts[2::2]):
            body = with_attn_helpers(with_latent_helpers(body.split("\nnamespace mdx {")[0]))
            fields = re.findall(r'need_\w+\((?:op|"mdx_\w+"), "([^"]+)"', body)
            if "check_epilogue_operands(" in body:
                fields += shared
            found |= {(name, f) for f in fields}
    assert {(e, f) for e in ("mdx_cfg_ddim_step", "mdx_cfg_unipc_step") for f in ("x_in", "xin_c", "xin_ld")} <= found
    assert {("mdx_attention_bf16", f) for f in ("ldq", "Vt", "tk_dev", "B * H", "B * H * ceil(Tq / 128)")} <= found
    return found


def test_every_host_check_has_a_row():
    """One mutation per clause, mechanically: every field a need_* call of an entry point names must be named by a row of that entry point
    ("<field>=..." for a range / multiple check, "<field> must be N-byte aligned" for a pointer), so a check cannot be added without a row
    and a row cannot be dropped while its check stays."""
    rows = {}
    for op, _, _, _, names in TABLE:
        rows.setdefault(L.ENTRY_OF_OP[op], []).append(names)
    # the conv entry point passes K = ldw = kh * kw * Cin to the shared checks: with Cin % 8 == 0 (checked first) neither can fail
    checks = _host_checks() - {("mdx_conv2d_bf16", "K"), ("mdx_conv2d_bf16", "ldw")}
    assert len(checks) >= 140, len(checks)
    missing = sorted((e, f) for e, f in checks if not any(n.startswith(f + "=") or n.startswith(f + " must be") for n in rows.get(e, [])))
    assert not missing, missing


def test_header_requirement_blocks_have_rows():
    """Every clause text of TABLE that quotes the header must really be in include/mdx.h, and every 'Requirements' block belongs to an entry
    point with rows."""
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mdx.h")).read()
    # gemm, conv, conv_direct, attention, groupnorm, layernorm, softmax, elementwise, fourier, gather, timeemb, ddim (shared with unipc)
    assert len(re.findall(r"Requirements \(", hdr)) == 12
    flat = re.sub(r"[\s*]+", " ", hdr)
    quoted = [c for _, c, *_ in TABLE if c in flat]
    assert len(quoted) >= 60, len(quoted)
