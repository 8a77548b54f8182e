"""Op IR of the MI355X denoiser: one Python record per kernel launch, holding torch tensor
*views* (device memory owned by the engine).  `lower()` turns a record into the C descriptor of
include/mdx.h; `magicdrive_amd._lib.Program` packs the descriptors into the array libmdx executes.

The records carry no arithmetic: the only implementation of each op is the HIP kernel behind its
C entry point.  (tests/plan_interp.py holds an independent torch restatement of the records'
semantics, used only to check the op graph on CPU.)
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Optional

import torch

from . import _lib as L

BF16 = torch.bfloat16
F16 = torch.float16
H16 = (BF16, F16)          # the two 16-bit storage types: every 16-bit operand of ONE op must use the same one (dtype_code)
F32 = torch.float32


def _p(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _chk(cond: bool, msg: str):
    if not cond:
        raise ValueError(msg)


def _rows2d(t: torch.Tensor):
    """[M, C] view with unit inner stride -> (M, C, ld)."""
    _chk(t.dim() == 2 and (t.shape[1] == 1 or t.stride(1) == 1), f"need [M,C] view with unit inner stride, got {tuple(t.shape)} {t.stride()}")
    return t.shape[0], t.shape[1], t.stride(0)


def _nhwc(t: torch.Tensor):
    """[B,H,W,C] channels-last view, pixels dense -> (B,H,W,C,ld)."""
    _chk(t.dim() == 4 and t.stride(3) == 1, f"need [B,H,W,C] view, got {tuple(t.shape)} {t.stride()}")
    B, H, W, Cc = t.shape
    ld = t.stride(2)
    _chk((W == 1 or True) and (H == 1 or t.stride(1) == W * ld) and (B == 1 or t.stride(0) == H * W * ld),
         f"pixels must be dense: shape {tuple(t.shape)} stride {t.stride()}")
    return B, H, W, Cc, ld


def _lower_xin(d, what: str, x_in: Optional[torch.Tensor], n: int, cfg: bool, xin_c: int):
    """x_in / n / cfg / xin_c / xin_ld of a latent op's descriptor (csrc/latent.h: XinDst).  x_in holds the n latents once, twice under
    CFG: fp32 flat, or 16-bit channels-last [pixels, ld] with xin_c channels per pixel and ld >= xin_c (padded); an fp32 or absent x_in
    leaves xin_c = xin_ld = 0."""
    c = 2 if cfg else 1
    d.x_in, d.n, d.cfg = _p(x_in), n, int(cfg)
    if x_in is None:
        return
    if x_in.dtype == F32:
        _chk(x_in.is_contiguous() and x_in.numel() == c * n, f"{what}: fp32 x_in must hold {c} x n elements")
    else:
        _chk(x_in.dtype in H16 and x_in.dim() == 2 and x_in.is_contiguous() and xin_c > 0, f"{what}: 16-bit x_in must be [pixels, ld]")
        _chk(x_in.shape[0] * xin_c == c * n and x_in.shape[1] >= xin_c, f"{what}: 16-bit x_in shape")
        d.xin_c, d.xin_ld = xin_c, x_in.shape[1]


def _lower_given_views(d, what: str, n: int, mode: int, mask, cond, noise, last_step: int):
    """gv_* of a scheduler op's descriptor (MdxDdimDesc.gv_*): mask uint8 [views], cond / noise fp32 [n] in x's layout, mode 1 | 2."""
    if not mode:
        return
    _chk(mode in (1, 2) and mask is not None and mask.dtype == torch.uint8 and mask.is_contiguous() and n % mask.numel() == 0, f"{what}: given-view mask")
    _chk(noise is not None and noise.dtype == F32 and noise.is_contiguous() and noise.numel() == n, f"{what}: gv_noise")
    _chk(mode == 2 or (cond is not None and cond.dtype == F32 and cond.is_contiguous() and cond.numel() == n), f"{what}: gv_cond")
    d.gv_mask, d.gv_noise, d.gv_cond = _p(mask), _p(noise), _p(cond)
    d.gv_mode, d.gv_view_elems, d.gv_last_step = mode, n // mask.numel(), last_step


def _columns(what: str, table: dict, ld: int, cols, names: str):
    """The two coefficient columns of a latent op: as given, or (either negative) by the table's width."""
    if min(cols) < 0:
        _chk(ld in table, f"{what}: a coefficient table of width {ld} needs {names}")
        cols = table[ld]
    _chk(all(0 <= c < ld for c in cols), f"{what}: columns {cols[0]}, {cols[1]} of a table of width {ld}")
    return cols


@dataclass
class Gemm:
    """C = epi(A @ W^T + bias + temb[row]) + R.  A [M,K] or [Bt,M,K]; W [N,K] or [Bt,N,K]; C [M,No] or [Bt,M,No]."""
    A: torch.Tensor
    W: torch.Tensor
    C: torch.Tensor
    bias: Optional[torch.Tensor] = None      # fp32 [N]
    R: Optional[torch.Tensor] = None         # same shape/dtype as C
    temb: Optional[torch.Tensor] = None      # fp32 table
    sel: Optional[torch.Tensor] = None       # int32 [1]
    epilogue: int = L.EPI_NONE
    temb_sel_stride: int = 0
    temb_b_stride: int = 0
    rows_per_b: int = 1
    splitk: int = 0
    ws: Optional[torch.Tensor] = None
    name: str = ""
    # fused q/k/v projection: raw columns >= vt_from go, transposed, to Vt [Bv, N - vt_from, >= vt_T] (token m -> view m // vt_T,
    # position m % vt_T); C then has vt_from columns (include/mdx.h: MdxGemmDesc.Vt)
    Vt: Optional[torch.Tensor] = None
    vt_from: int = 0
    vt_T: int = 0
    # LayerNorm of the A rows fused in (include/mdx.h: MdxGemmDesc.ln_eps): A = raw rows, W / bias carry gamma / beta (engine.PackedNet.ln_lin),
    # ln_csum fp32 [N] = row sums of W, ln_scratch [M, K] = where routes that cannot fuse put the normalised rows
    ln_eps: float = 0.0
    ln_csum: Optional[torch.Tensor] = None
    ln_scratch: Optional[torch.Tensor] = None
    # row statistics (include/mdx.h: MdxGemmDesc.rowstat_out / ln_stats): fp32 [parts, M, 2] = (sum, sum of squares) of the stored C rows per column part,
    # written by the producer of a LayerNorm's input and read by the GEMM that carries that LayerNorm (ln_eps > 0)
    rowstat: Optional[torch.Tensor] = None
    ln_stats: Optional[torch.Tensor] = None
    # W once more in MFMA-fragment order (packing.pack_wq; include/mdx.h: MdxGemmDesc.Wq): the W-direct persistent kernel reads this copy
    Wq: Optional[torch.Tensor] = None
    opcode = L.OP_GEMM

    def lower(self):
        A, W, Cm = self.A, self.W, self.C
        batch = 1
        sA = sW = sC = sR = 0
        if Cm.dim() == 3:
            batch = Cm.shape[0]
            sC = Cm.stride(0)
            if A.dim() == 3:
                sA = A.stride(0); A = A[0]
            if W.dim() == 3:
                sW = W.stride(0); W = W[0]
            C2 = Cm[0]
        else:
            C2 = Cm
        M, K, lda = _rows2d(A)
        N, K2, ldw = _rows2d(W)
        Mc, No, ldc = _rows2d(C2)
        _chk(K == K2 and M == Mc, f"gemm {self.name}: shape mismatch A{tuple(A.shape)} W{tuple(W.shape)} C{tuple(C2.shape)}")
        if self.Vt is not None:
            _chk(self.epilogue == L.EPI_NONE and batch == 1 and No == self.vt_from and 0 < self.vt_from < N and self.vt_T > 0,
                 f"gemm {self.name}: fused V^T output needs a plain epilogue and C with vt_from columns")
            _chk(self.Vt.dim() == 3 and self.Vt.dtype == A.dtype and self.Vt.stride(2) == 1 and self.Vt.shape[1] == N - self.vt_from
                 and self.Vt.shape[0] * self.vt_T == M and self.Vt.shape[2] >= self.vt_T, f"gemm {self.name}: Vt shape {tuple(self.Vt.shape)}")
        else:
            _chk(No == (N // 2 if self.epilogue == L.EPI_GEGLU else N), f"gemm {self.name}: C has {No} cols for N={N}")
        _chk(A.dtype in H16 and W.dtype == A.dtype and Cm.dtype in (A.dtype, F32), f"gemm {self.name}: dtypes")
        d = L.MdxGemmDesc()
        d.A, d.W, d.C = _p(A), _p(W), _p(C2)
        ldr = 0
        if self.R is not None:
            R2 = self.R
            if R2.dim() == 3:
                sR = R2.stride(0); R2 = R2[0]
            _chk(R2.dtype == Cm.dtype and tuple(R2.shape) == tuple(C2.shape), f"gemm {self.name}: residual shape/dtype")
            ldr = R2.stride(0)
            d.R = _p(R2)
        if self.bias is not None:
            _chk(self.bias.dtype == F32 and self.bias.numel() == N, f"gemm {self.name}: bias")
            d.bias = _p(self.bias)
        if self.temb is not None:
            _chk(self.temb.dtype == F32, "temb must be fp32")
            d.temb = _p(self.temb)
        if self.sel is not None:
            _chk(self.sel.dtype == torch.int32, "sel must be int32")
            d.sel_ptr = _p(self.sel)
        if self.ws is not None:
            d.ws = _p(self.ws); d.ws_bytes = self.ws.numel() * self.ws.element_size()
        d.M, d.N, d.K = M, N, K
        d.lda, d.ldw, d.ldc, d.ldr = lda, ldw, ldc, ldr
        d.batch, d.sA, d.sW, d.sC, d.sR = batch, sA, sW, sC, sR
        d.temb_sel_stride, d.temb_b_stride, d.rows_per_b = self.temb_sel_stride, self.temb_b_stride, self.rows_per_b
        d.epilogue, d.splitk, d.c_is_f32 = self.epilogue, self.splitk, int(Cm.dtype == F32)
        if self.Vt is not None:
            d.Vt = _p(self.Vt)
            d.vt_from, d.vt_T, d.vt_ld, d.vt_stride = self.vt_from, self.vt_T, self.Vt.stride(1), self.Vt.stride(0)
        if self.ln_eps > 0:
            _chk(batch == 1 and self.ln_csum is not None and self.ln_csum.dtype == F32 and self.ln_csum.numel() == N, f"gemm {self.name}: ln_csum")
            _chk(self.ln_scratch is None or (self.ln_scratch.dtype == A.dtype and self.ln_scratch.is_contiguous() and self.ln_scratch.numel() >= M * lda),
                 f"gemm {self.name}: ln_scratch must be a contiguous [M, lda] buffer of the operand type")
            d.ln_eps, d.ln_csum, d.ln_scratch = float(self.ln_eps), _p(self.ln_csum), _p(self.ln_scratch)
            if self.ln_stats is not None:
                st = self.ln_stats
                _chk(st.dtype == F32 and st.dim() == 3 and st.is_contiguous() and st.shape[1] == M and st.shape[2] == 2, f"gemm {self.name}: ln_stats must be fp32 [parts, M, 2]")
                d.ln_stats, d.ln_stats_parts = _p(st), st.shape[0]
        else:
            _chk(self.ln_stats is None, f"gemm {self.name}: ln_stats without ln_eps")
        if self.rowstat is not None:
            rs = self.rowstat
            _chk(rs.dtype == F32 and rs.dim() == 3 and rs.is_contiguous() and rs.shape[1] == M and rs.shape[2] == 2 and rs.shape[0] >= 1,
                 f"gemm {self.name}: rowstat must be fp32 [parts, M, 2]")
            _chk(batch == 1 and self.epilogue == L.EPI_NONE and self.Vt is None and Cm.dtype in H16, f"gemm {self.name}: rowstat needs a plain 2-D GEMM with 16-bit C")
            d.rowstat_out, d.rowstat_parts = _p(rs), rs.shape[0]
        if self.Wq is not None:
            _chk(batch == 1 and self.Wq.dtype == W.dtype and self.Wq.is_contiguous() and self.Wq.numel() == (N + 255) // 256 * 256 * K and K % 32 == 0,
                 f"gemm {self.name}: Wq must be packing.pack_wq(W)")
            d.Wq = _p(self.Wq)
        return self.opcode, d


@dataclass
class Conv:
    """Channels-last conv: X [B,Hi,Wi,Cin], Wt [Cout,kh,kw,Cin] packed bf16, Y [B,Ho,Wo,Cout].
    upsample2x: Y = conv3x3(pad 1)(nearest resize of X to Ho x Wo) from the low-res X; Wt = packing.fold_upsample_conv's
    [phases,Cout,2,2,Cin] (MdxConvDesc.upsample2x)."""
    X: torch.Tensor
    Wt: torch.Tensor
    Y: torch.Tensor
    bias: Optional[torch.Tensor] = None
    R: Optional[torch.Tensor] = None
    temb: Optional[torch.Tensor] = None
    sel: Optional[torch.Tensor] = None
    stride: tuple = (1, 1)
    pad: tuple = (1, 1)
    pad_end: Optional[tuple] = None          # zero padding at the bottom / right when it differs from `pad` (Downsample2D with padding=0:
                                             # F.pad(x, (0, 1, 0, 1)), resnet.py:215-217) — the kernels zero-fill every tap outside the image,
                                             # so only the output size depends on it
    epilogue: int = L.EPI_NONE
    temb_sel_stride: int = 0
    temb_b_stride: int = 0
    direct: bool = False                     # vector-ALU path (tiny Cin / Cout, fp32 I/O allowed)
    splitk: int = 0
    ws: Optional[torch.Tensor] = None
    name: str = ""
    upsample2x: bool = False

    @property
    def opcode(self):
        return L.OP_CONV_DIRECT if self.direct else L.OP_CONV

    def _lower_upsample2x(self):
        B, Hi, Wi, Cin, ldx = _nhwc(self.X)
        B2, Ho, Wo, Cout, ldy = _nhwc(self.Y)
        _chk(self.Wt.dim() == 5 and self.Wt.is_contiguous() and self.Wt.dtype in H16, f"conv {self.name}: upsample2x takes packed phase weights")
        nph, Co2, kh, kw, Ci2 = self.Wt.shape
        _chk(B == B2 and Cout == Co2 and Cin == Ci2 and (kh, kw) == (2, 2), f"conv {self.name}: shape mismatch")
        _chk(Ho in (2 * Hi, 2 * Hi - 1) and Wo in (2 * Wi, 2 * Wi - 1) and nph == (2 + (Ho != 2 * Hi)) * (2 + (Wo != 2 * Wi)), f"conv {self.name}: upsample2x sizes")
        _chk(not self.direct and self.R is None and self.temb is None and self.epilogue == L.EPI_NONE and tuple(self.stride) == (1, 1),
             f"conv {self.name}: upsample2x has a bias-only epilogue")
        _chk(self.X.dtype == self.Wt.dtype and self.Y.dtype == self.Wt.dtype, f"conv {self.name}: the MFMA path takes one 16-bit type")
        d = L.MdxConvDesc()
        d.X, d.Wt, d.Y = _p(self.X), _p(self.Wt), _p(self.Y)
        if self.bias is not None:
            _chk(self.bias.dtype == F32 and self.bias.numel() == Cout, f"conv {self.name}: bias")
            d.bias = _p(self.bias)
        d.B, d.Hi, d.Wi, d.Cin, d.Ho, d.Wo, d.Cout = B, Hi, Wi, Cin, Ho, Wo, Cout
        d.kh, d.kw, d.sh, d.sw, d.ph, d.pw = 2, 2, 1, 1, 0, 0
        d.ldx, d.ldy = ldx, ldy
        d.upsample2x = 1
        if self.ws is not None:
            d.ws = _p(self.ws); d.ws_bytes = self.ws.numel() * self.ws.element_size()
        return self.opcode, d

    def lower(self):
        if self.upsample2x:
            return self._lower_upsample2x()
        B, Hi, Wi, Cin, ldx = _nhwc(self.X)
        B2, Ho, Wo, Cout, ldy = _nhwc(self.Y)
        Co2, kh, kw, Ci2 = self.Wt.shape
        _chk(self.Wt.is_contiguous() and self.Wt.dtype in H16, f"conv {self.name}: weights must be packed bf16 / fp16")
        _chk(B == B2 and Cout == Co2 and Cin == Ci2, f"conv {self.name}: shape mismatch")
        sh, sw = self.stride
        ph, pw = self.pad
        phe, pwe = self.pad_end if self.pad_end is not None else self.pad
        _chk(Ho == (Hi + ph + phe - kh) // sh + 1 and Wo == (Wi + pw + pwe - kw) // sw + 1, f"conv {self.name}: output size")
        d = L.MdxConvDirectDesc() if self.direct else L.MdxConvDesc()
        d.X, d.Wt, d.Y = _p(self.X), _p(self.Wt), _p(self.Y)
        if self.R is not None:
            rB, rH, rW, rC, ldr = _nhwc(self.R)
            _chk((rB, rH, rW, rC) == (B, Ho, Wo, Cout) and self.R.dtype == self.Y.dtype, f"conv {self.name}: residual")
            d.R, d.ldr = _p(self.R), ldr
        if self.bias is not None:
            _chk(self.bias.dtype == F32 and self.bias.numel() == Cout, f"conv {self.name}: bias")
            d.bias = _p(self.bias)
        if self.temb is not None:
            d.temb = _p(self.temb)
        if self.sel is not None:
            d.sel_ptr = _p(self.sel)
        d.B, d.Hi, d.Wi, d.Cin, d.Ho, d.Wo, d.Cout = B, Hi, Wi, Cin, Ho, Wo, Cout
        d.kh, d.kw, d.sh, d.sw, d.ph, d.pw = kh, kw, sh, sw, ph, pw
        d.ldx, d.ldy = ldx, ldy
        d.temb_sel_stride, d.temb_b_stride = self.temb_sel_stride, self.temb_b_stride
        d.epilogue = self.epilogue
        if self.direct:
            d.x_is_f32 = int(self.X.dtype == F32)
            d.y_is_f32 = int(self.Y.dtype == F32)
        else:
            _chk(self.X.dtype == self.Wt.dtype and self.Y.dtype == self.Wt.dtype, f"conv {self.name}: the MFMA path takes one 16-bit type")
            d.splitk = self.splitk
            if self.ws is not None:
                d.ws = _p(self.ws); d.ws_bytes = self.ws.numel() * self.ws.element_size()
        return self.opcode, d


@dataclass
class Attn:
    """O = sum_s softmax(Q K_s^T * scale) V_s.  Q [B,Tq,C]; K [Bkv,Tk,C]; Vt [Bkv,C,ldv] (V transposed); O [B,Tq,C].
    v_rowmajor: Vt is V itself, [B,Tk,C] (short sequences only: MdxAttnDesc.v_rowmajor); causal: query t sees keys 0..t.
    tk_dev: int32 [1] on the device — Tk is then the CAPACITY of K / Vt and the kernel attends to the first tk_dev[0] keys, read when
    it runs (MdxAttnDesc.tk_dev: the context attention of a sampler plan built for a bucket of box counts).
    tk_rows: int32 [B] on the device — the same with one count per query batch: batch b attends to the first tk_rows[b] keys of its own
    K / Vt (OP_ATTN_ROWS, mdx_attention_ctx_rows_*: the scenes of a batched call attend to their own boxes only)."""
    Q: torch.Tensor
    K: torch.Tensor
    Vt: torch.Tensor
    O: torch.Tensor
    heads: int
    Tk: int
    scale: float
    kvmap: Optional[torch.Tensor] = None     # int32 [B*nsrc]
    nsrc: int = 1
    name: str = ""
    joint: bool = False                      # one softmax over the concatenated sources (neighboring_attn_type concat / self) instead of a sum of per-source attentions
    q_prescaled: bool = False                # Q already carries scale * log2(e) (folded into to_q at pack time): probabilities are exp2(Q K^T - max)
    causal: bool = False
    v_rowmajor: bool = False
    tk_dev: Optional[torch.Tensor] = None    # int32 [1], same device as Q: the live key count (<= Tk)
    tk_rows: Optional[torch.Tensor] = None   # int32 [B], same device as Q: the live key count of every query batch; not together with tk_dev
    opcode = L.OP_ATTN

    def lower(self):
        Q, K, Vt, O = self.Q, self.K, self.Vt, self.O
        B, Tq, Cc = Q.shape
        _chk(Q.stride(2) == 1 and K.stride(2) == 1 and O.stride(2) == 1 and Vt.stride(2) == 1, f"attn {self.name}: inner strides")
        if self.v_rowmajor:
            _chk(Cc % self.heads == 0 and K.shape[2] == Cc and Vt.shape[2] == Cc and O.shape == Q.shape, f"attn {self.name}: shapes")
            _chk(K.shape[1] == self.Tk and Vt.shape[1] == self.Tk and Vt.shape[0] == K.shape[0], f"attn {self.name}: kv shapes")
        else:
            _chk(not self.causal, f"attn {self.name}: causal needs v_rowmajor")
            _chk(Cc % self.heads == 0 and K.shape[2] == Cc and Vt.shape[1] == Cc and O.shape == Q.shape, f"attn {self.name}: shapes")
            _chk(K.shape[1] == self.Tk and Vt.shape[2] >= self.Tk and Vt.shape[0] == K.shape[0], f"attn {self.name}: kv shapes")
        d = L.MdxAttnDesc()
        d.Q, d.K, d.Vt, d.O = _p(Q), _p(K), _p(Vt), _p(O)
        if self.kvmap is not None:
            _chk(self.kvmap.dtype == torch.int32 and self.kvmap.numel() == B * self.nsrc, f"attn {self.name}: kvmap")
            d.kvmap = _p(self.kvmap)
        else:
            _chk(self.nsrc == 1 and K.shape[0] == B, f"attn {self.name}: identity kv map needs Bkv == B")
        d.B, d.H, d.Tq, d.Tk, d.d, d.nsrc = B, self.heads, Tq, self.Tk, Cc // self.heads, self.nsrc
        d.ldq, d.sQ = Q.stride(1), Q.stride(0)
        d.ldk, d.sK = K.stride(1), K.stride(0)
        d.ldv, d.sV = Vt.stride(1), Vt.stride(0)
        d.ldo, d.sO = O.stride(1), O.stride(0)
        d.scale = float(self.scale)
        d.joint = int(self.joint)
        d.q_prescaled = int(self.q_prescaled)
        d.causal, d.v_rowmajor = int(self.causal), int(self.v_rowmajor)
        if self.tk_dev is not None:
            _chk(self.tk_dev.dtype == torch.int32 and self.tk_dev.numel() == 1 and self.tk_dev.device == Q.device,
                 f"attn {self.name}: tk_dev must be one int32 on the device of Q")
            _chk(self.nsrc == 1 and self.kvmap is None and not self.joint and not self.causal and not self.v_rowmajor,
                 f"attn {self.name}: tk_dev serves one source, no joint softmax, no causal mask, the V^T operand")
            d.tk_dev = _p(self.tk_dev)
        opcode = self.opcode
        if self.tk_rows is not None:
            _chk(self.tk_dev is None, f"attn {self.name}: tk_rows and tk_dev are mutually exclusive")
            _chk(self.tk_rows.dtype == torch.int32 and self.tk_rows.dim() == 1 and self.tk_rows.numel() == B and self.tk_rows.is_contiguous()
                 and self.tk_rows.device == Q.device, f"attn {self.name}: tk_rows must be int32 [B={B}], contiguous, on the device of Q")
            _chk(self.nsrc == 1 and self.kvmap is None and not self.joint and not self.causal and not self.v_rowmajor,
                 f"attn {self.name}: tk_rows serves one source, no joint softmax, no causal mask, the V^T operand")
            d.tk_dev = _p(self.tk_rows)
            opcode = L.OP_ATTN_ROWS
        _chk(self.nsrc >= 1 and (self.nsrc <= 8 if self.joint else self.nsrc <= 2), f"attn {self.name}: nsrc={self.nsrc} (joint={self.joint})")
        return opcode, d


@dataclass
class GroupNorm:
    X: torch.Tensor      # [B, HW, C] view
    Y: torch.Tensor
    gamma: torch.Tensor  # fp32 [C]
    beta: torch.Tensor
    groups: int
    eps: float
    silu: bool = False
    ws: Optional[torch.Tensor] = None
    name: str = ""
    opcode = L.OP_GROUPNORM

    def lower(self):
        B, HW, Cc = self.X.shape
        _chk(self.X.stride(2) == 1 and self.Y.stride(2) == 1 and self.Y.shape == self.X.shape, f"gn {self.name}: layout")
        _chk(B == 1 or (self.X.stride(0) == HW * self.X.stride(1) and self.Y.stride(0) == HW * self.Y.stride(1)), f"gn {self.name}: batch stride")
        _chk(self.gamma.dtype == F32 and self.beta.dtype == F32 and self.gamma.numel() == Cc, f"gn {self.name}: affine")
        d = L.MdxGroupNormDesc()
        d.X, d.Y, d.gamma, d.beta = _p(self.X), _p(self.Y), _p(self.gamma), _p(self.beta)
        d.B, d.HW, d.C, d.G, d.ldx, d.ldy = B, HW, Cc, self.groups, self.X.stride(1), self.Y.stride(1)
        d.eps, d.silu = float(self.eps), int(self.silu)
        if self.ws is not None:
            d.ws = _p(self.ws); d.ws_bytes = self.ws.numel() * self.ws.element_size()
        return self.opcode, d


@dataclass
class GroupNormResident(GroupNorm):
    """The same operation through mdx_groupnorm_resident_*: ONE kernel that reads the tensor once (csrc/gn_route.h says which shapes it
    takes; the library returns MDX_EUNSUPPORTED for the others and never falls back).  Same fields, same descriptor."""
    opcode = L.OP_GROUPNORM_RESIDENT


@dataclass
class LayerNorm:
    X: torch.Tensor      # [M, C]
    Y: torch.Tensor
    gamma: torch.Tensor
    beta: torch.Tensor
    eps: float = 1e-5
    name: str = ""
    opcode = L.OP_LAYERNORM

    def lower(self):
        M, Cc, ldx = _rows2d(self.X)
        M2, C2, ldy = _rows2d(self.Y)
        _chk(M == M2 and Cc == C2, f"ln {self.name}: shapes")
        d = L.MdxLayerNormDesc()
        d.X, d.Y, d.gamma, d.beta = _p(self.X), _p(self.Y), _p(self.gamma), _p(self.beta)
        d.M, d.C, d.ldx, d.ldy, d.eps = M, Cc, ldx, ldy, float(self.eps)
        return self.opcode, d


@dataclass
class Softmax:
    """Y[r, :T] = softmax(scale * X[r, :T]) (fp32 scores -> bf16 probabilities); Y's columns T.. are zero-filled."""
    X: torch.Tensor      # fp32 [rows, >=T] (row stride = X.stride(0))
    Y: torch.Tensor      # bf16 [rows, ldy >= T] contiguous rows
    T: int
    scale: float = 1.0
    name: str = ""
    opcode = L.OP_SOFTMAX

    def lower(self):
        _chk(self.X.dtype == F32 and self.Y.dtype in H16 and self.X.dim() == 2 and self.Y.dim() == 2, "softmax: dtypes / rank")
        _chk(self.X.stride(1) == 1 and self.Y.stride(1) == 1 and self.X.shape[0] == self.Y.shape[0], "softmax: layout")
        _chk(0 < self.T <= self.X.shape[1] and self.T <= self.Y.shape[1], "softmax: T")
        d = L.MdxSoftmaxDesc()
        d.X, d.Y, d.rows, d.T, d.ldx, d.ldy, d.scale = _p(self.X), _p(self.Y), self.X.shape[0], self.T, self.X.stride(0), self.Y.stride(0), float(self.scale)
        # the kernel zero-fills Y[:, T:ldy]: Y must own its whole row pitch
        _chk(self.Y.shape[1] == self.Y.stride(0), "softmax: Y rows must be dense (the pad columns are written)")
        return self.opcode, d


@dataclass
class Ew:
    """kind in {ADD (Y += X), COPY, SILU, SCALE} on [M,C] views."""
    kind: int
    X: torch.Tensor
    Y: torch.Tensor
    alpha: float = 1.0
    name: str = ""
    opcode = L.OP_EW

    def lower(self):
        M, Cc, ldx = _rows2d(self.X)
        M2, C2, ldy = _rows2d(self.Y)
        _chk(M == M2 and Cc == C2, f"ew {self.name}: shapes {tuple(self.X.shape)} vs {tuple(self.Y.shape)}")
        d = L.MdxEwDesc()
        d.X, d.Y, d.kind, d.M, d.C, d.ldx, d.ldy = _p(self.X), _p(self.Y), self.kind, M, Cc, ldx, ldy
        d.x_is_f32, d.y_is_f32, d.alpha = int(self.X.dtype == F32), int(self.Y.dtype == F32), float(self.alpha)
        return self.opcode, d


@dataclass
class Upsample:
    """Nearest resize X [B,Hi,Wi,C] -> Y [B,Ho,Wo,C]; ymap/xmap int32 source indices (host-computed, torch's rule)."""
    X: torch.Tensor
    Y: torch.Tensor
    ymap: torch.Tensor
    xmap: torch.Tensor
    name: str = ""
    opcode = L.OP_EW

    def lower(self):
        B, Hi, Wi, Cc, ldx = _nhwc(self.X)
        B2, Ho, Wo, C2, ldy = _nhwc(self.Y)
        _chk(B == B2 and Cc == C2 and self.ymap.numel() == Ho and self.xmap.numel() == Wo, f"upsample {self.name}")
        d = L.MdxEwDesc()
        d.X, d.Y, d.ymap, d.xmap = _p(self.X), _p(self.Y), _p(self.ymap), _p(self.xmap)
        d.kind, d.C, d.ldx, d.ldy = L.EW_UPSAMPLE, Cc, ldx, ldy
        d.B, d.Hi, d.Wi, d.Ho, d.Wo = B, Hi, Wi, Ho, Wo
        d.x_is_f32, d.y_is_f32 = int(self.X.dtype == F32), int(self.Y.dtype == F32)
        return self.opcode, d


@dataclass
class Layout:
    """to_nhwc: X contiguous [B,C,H,W] -> Y [B,H,W,C] view ; else the reverse (X nhwc view, Y contiguous nchw)."""
    X: torch.Tensor
    Y: torch.Tensor
    to_nhwc: bool
    name: str = ""
    opcode = L.OP_EW

    def lower(self):
        d = L.MdxEwDesc()
        if self.to_nhwc:
            _chk(self.X.is_contiguous() and self.X.dim() == 4, "layout: X must be contiguous NCHW")
            B, Cc, H, W = self.X.shape
            B2, H2, W2, C2, ldy = _nhwc(self.Y)
            _chk((B, H, W, Cc) == (B2, H2, W2, C2), "layout: shapes")
            d.kind, d.ldy = L.EW_NCHW_TO_NHWC, ldy
        else:
            _chk(self.Y.is_contiguous() and self.Y.dim() == 4, "layout: Y must be contiguous NCHW")
            B, Cc, H, W = self.Y.shape
            B2, H2, W2, C2, ldx = _nhwc(self.X)
            _chk((B, H, W, Cc) == (B2, H2, W2, C2), "layout: shapes")
            d.kind, d.ldx = L.EW_NHWC_TO_NCHW, ldx
        d.X, d.Y, d.B, d.C, d.Hi, d.Wi = _p(self.X), _p(self.Y), B, Cc, H, W
        d.x_is_f32, d.y_is_f32 = int(self.X.dtype == F32), int(self.Y.dtype == F32)
        return self.opcode, d


@dataclass
class Fourier:
    X: torch.Tensor                      # fp32 [n, P, 3] contiguous
    Y: torch.Tensor                      # bf16 [n, P*(3+6F)] view
    F: int
    mask: Optional[torch.Tensor] = None  # uint8 [n]
    null_feat: Optional[torch.Tensor] = None  # fp32 [P*(3+6F)]
    name: str = ""
    opcode = L.OP_FOURIER

    def lower(self):
        n, Pn, three = self.X.shape
        _chk(three == 3 and self.X.is_contiguous() and self.X.dtype == F32, "fourier: X fp32 [n,P,3]")
        n2, width, ldy = _rows2d(self.Y)
        _chk(n2 == n and width == Pn * (3 + 6 * self.F) and self.Y.dtype in H16, "fourier: Y")
        d = L.MdxFourierDesc()
        d.X, d.Y, d.mask, d.null_feat = _p(self.X), _p(self.Y), _p(self.mask), _p(self.null_feat)
        if self.mask is not None:
            _chk(self.mask.dtype == torch.uint8 and self.mask.numel() == n, "fourier: mask")
        if self.null_feat is not None:
            _chk(self.null_feat.dtype == F32 and self.null_feat.numel() == width, "fourier: null")
        d.n, d.P, d.F, d.ldy = n, Pn, self.F, ldy
        return self.opcode, d


@dataclass
class Gather:
    T: torch.Tensor                      # bf16 [rows, C]
    Y: torch.Tensor                      # bf16 [n, C] view
    idx: torch.Tensor                    # int64 [n]
    mask: Optional[torch.Tensor] = None  # uint8 [n]
    null_row: Optional[torch.Tensor] = None  # bf16 [C]
    name: str = ""
    add: Optional[torch.Tensor] = None       # bf16 [period, C], same row stride as T: Y[i] += add[i % period] (fp32 sum, one rounding)
    opcode = L.OP_GATHER

    def lower(self):
        rows, Cc, ldt = _rows2d(self.T)
        n, C2, ldy = _rows2d(self.Y)
        _chk(Cc == C2 and self.idx.dtype == torch.int64 and self.idx.numel() == n, "gather: shapes")
        d = L.MdxGatherDesc()
        d.T, d.Y, d.idx, d.mask, d.null_row = _p(self.T), _p(self.Y), _p(self.idx), _p(self.mask), _p(self.null_row)
        d.n, d.C, d.ldt, d.ldy, d.n_rows = n, Cc, ldt, ldy, rows
        if self.add is not None:
            period, C3, lda = _rows2d(self.add)
            _chk(C3 == Cc and lda == ldt and period > 0 and self.add.dtype == self.T.dtype, "gather: add must be [period, C] with T's row stride and dtype")
            d.add, d.add_period = _p(self.add), period
        return self.opcode, d


@dataclass
class TimeEmb:
    t: torch.Tensor                      # fp32 [n]
    Y: torch.Tensor                      # fp32 [n, dim]
    flip_sin_to_cos: bool = True
    freq_shift: float = 0.0
    max_period: float = 10000.0
    name: str = ""
    opcode = L.OP_TIMEEMB

    def lower(self):
        n, dim, ldy = _rows2d(self.Y)
        _chk(self.t.dtype == F32 and self.t.numel() == n and self.Y.dtype == F32, "timeemb: dtypes")
        d = L.MdxTimeEmbDesc()
        d.t, d.Y, d.n, d.dim, d.flip_sin_to_cos, d.ldy = _p(self.t), _p(self.Y), n, dim, int(self.flip_sin_to_cos), ldy
        d.freq_shift, d.max_period = float(self.freq_shift), float(self.max_period)
        return self.opcode, d


@dataclass
class DdimStep:
    x: torch.Tensor                      # fp32 [n] latents (any layout), updated in place
    eps: torch.Tensor                    # fp32 [c*n], same layout ([uncond | cond] when cfg)
    coef: torch.Tensor                   # fp32 [steps, 4]
    step: torch.Tensor                   # int32 [1]
    x_in: Optional[torch.Tensor] = None  # fp32 flat [c*n]  or  bf16 [c*pixels, ld] channels-last with ld >= C (padded)
    cfg: bool = False
    guidance: float = 1.0
    xin_c: int = 0                        # channels per pixel of x (for the bf16 padded x_in)
    name: str = ""
    # given views (MdxDdimDesc.gv_*): mask uint8 [views], cond / noise fp32 [n] in x's layout, mode 1 | 2, last step index
    gv_mask: Optional[torch.Tensor] = None
    gv_cond: Optional[torch.Tensor] = None
    gv_noise: Optional[torch.Tensor] = None
    gv_mode: int = 0
    gv_last_step: int = 0
    opcode = L.OP_DDIM

    def lower(self):
        n = self.x.numel()
        _chk(self.x.is_contiguous() and self.eps.is_contiguous() and self.eps.numel() == n * (2 if self.cfg else 1), "ddim: sizes")
        _chk(self.x.dtype == F32 and self.eps.dtype == F32 and self.coef.dtype == F32 and self.step.dtype == torch.int32, "ddim: dtypes")
        d = L.MdxDdimDesc()
        d.x, d.eps, d.coef, d.step_ptr, d.guidance = _p(self.x), _p(self.eps), _p(self.coef), _p(self.step), float(self.guidance)
        _lower_xin(d, "ddim", self.x_in, n, self.cfg, self.xin_c)
        _lower_given_views(d, "ddim", n, self.gv_mode, self.gv_mask, self.gv_cond, self.gv_noise, self.gv_last_step)
        return self.opcode, d


@dataclass
class UniPCStep:
    """Fused CFG + UniPC (order <= 2) predictor-corrector step; state buffers x_last / m1 / m2 are fp32 [n]."""
    x: torch.Tensor
    eps: torch.Tensor
    coef: torch.Tensor                   # fp32 [steps, 12]
    step: torch.Tensor
    x_last: torch.Tensor
    m1: torch.Tensor
    m2: torch.Tensor
    x_in: Optional[torch.Tensor] = None
    cfg: bool = False
    guidance: float = 1.0
    xin_c: int = 0
    name: str = ""
    # given views (MdxUniPCDesc.gv_*): as in DdimStep
    gv_mask: Optional[torch.Tensor] = None
    gv_cond: Optional[torch.Tensor] = None
    gv_noise: Optional[torch.Tensor] = None
    gv_mode: int = 0
    gv_last_step: int = 0
    opcode = L.OP_UNIPC

    def lower(self):
        n = self.x.numel()
        _chk(self.eps.numel() == n * (2 if self.cfg else 1) and all(t.numel() == n and t.dtype == F32 and t.is_contiguous() for t in (self.x, self.x_last, self.m1, self.m2)), "unipc: sizes")
        _chk(self.coef.dtype == F32 and self.coef.shape[1] == 12 and self.step.dtype == torch.int32, "unipc: coef/step")
        d = L.MdxUniPCDesc()
        d.x, d.eps, d.coef, d.step_ptr, d.guidance = _p(self.x), _p(self.eps), _p(self.coef), _p(self.step), float(self.guidance)
        d.x_last, d.m1, d.m2 = _p(self.x_last), _p(self.m1), _p(self.m2)
        _lower_xin(d, "unipc", self.x_in, n, self.cfg, self.xin_c)
        _lower_given_views(d, "unipc", n, self.gv_mode, self.gv_mask, self.gv_cond, self.gv_noise, self.gv_last_step)
        return self.opcode, d


@dataclass
class GroupStats:
    """Sample-health records (MdxStatsDesc, csrc/stats.hip): out[row, g] = {nonfinite, absmax, sum, sumsq} of X[g], fp32.
    X [G, ...]: fp32 or 16-bit, every X[g] dense (group stride X.stride(0)); out fp32 [G, 4], or [n_rows, G, 4] with `row`
    (int32 [1] on the device, read when the kernel runs: a plan's step counter); a row outside the table writes nothing."""
    X: torch.Tensor
    out: torch.Tensor
    row: Optional[torch.Tensor] = None
    name: str = ""
    opcode = L.OP_GROUP_STATS

    @staticmethod
    def chain_length(n: int, f32: bool) -> int:
        """k(n) of csrc/stats.hip's head comment: the longest chain of fp32 additions between an element and the stored sum / sumsq —
        a thread's own pieces, the tree over its V accumulators, the tail element, 6 butterfly levels, 2 levels over the 4 waves."""
        V = 4 if f32 else 8
        return -(-(-(-n // V)) // 256) + (2 if f32 else 3) + 1 + 6 + 2

    def lower(self):
        X, out = self.X, self.out
        _chk(X.dim() >= 1 and X.dtype in (F32,) + H16, f"stats {self.name}: X must be fp32 or 16-bit [G, ...]")
        G = X.shape[0]
        n = X.numel() // G if G else 0
        _chk(G == 0 or X[0].is_contiguous(), f"stats {self.name}: every group must be dense, got shape {tuple(X.shape)} stride {X.stride()}")
        _chk(out.dtype == F32 and out.is_contiguous() and out.dim() in (2, 3) and tuple(out.shape[-2:]) == (G, 4), f"stats {self.name}: out must be fp32 [rows, G={G}, 4]")
        d = L.MdxStatsDesc()
        d.X, d.out = _p(X), _p(out)
        d.G, d.n, d.sG, d.f32 = G, n, (X.stride(0) if G > 1 else n), int(X.dtype == F32)
        d.n_rows = out.shape[0] if out.dim() == 3 else 1
        if self.row is not None:
            _chk(self.row.dtype == torch.int32 and self.row.numel() == 1 and self.row.device == X.device, f"stats {self.name}: row must be one int32 on the device of X")
            d.row_dev = _p(self.row)
        else:
            _chk(out.dim() == 2 or out.shape[0] == 1, f"stats {self.name}: a table of rows needs `row`")
        return self.opcode, d


@dataclass
class Sdpa:
    """O = softmax(scale * Q K^T + mask) V on Q, K and V as a projection writes them (MdxSdpaDesc, csrc/attention_vrow.hip): Q, O
    [B,Tq,H*d], K, V [B,Tk,H*d], 16-bit views with unit inner stride — e.g. the three column blocks of one [B,T,3C] buffer.  V is read
    row-major, in place, at any length.  causal: key j is visible to query i iff j <= i (needs Tq == Tk).  klen: int32 [B] on the device,
    read when the kernel runs — batch b attends to its first klen[b] keys; a count outside [1, Tk] writes NaN to that batch's rows."""
    Q: torch.Tensor
    K: torch.Tensor
    V: torch.Tensor
    O: torch.Tensor
    heads: int
    scale: float
    causal: bool = False
    klen: Optional[torch.Tensor] = None      # int32 [B], same device as Q
    name: str = ""
    opcode = L.OP_SDPA

    def lower(self):
        Q, K, V, O = self.Q, self.K, self.V, self.O
        _chk(all(t.dim() == 3 for t in (Q, K, V, O)), f"sdpa {self.name}: Q, K, V, O must be [B, T, H*d]")
        B, Tq, Cc = Q.shape
        Tk = K.shape[1]
        _chk(Q.dtype in H16 and K.dtype == Q.dtype and V.dtype == Q.dtype and O.dtype == Q.dtype, f"sdpa {self.name}: one 16-bit type for Q, K, V, O")
        _chk(all(t.shape[2] == 1 or t.stride(2) == 1 for t in (Q, K, V, O)), f"sdpa {self.name}: inner strides")
        _chk(self.heads > 0 and Cc % self.heads == 0, f"sdpa {self.name}: C={Cc} is not a multiple of heads={self.heads}")
        _chk(tuple(K.shape) == (B, Tk, Cc) and tuple(V.shape) == (B, Tk, Cc) and O.shape == Q.shape,
             f"sdpa {self.name}: shapes Q{tuple(Q.shape)} K{tuple(K.shape)} V{tuple(V.shape)} O{tuple(O.shape)}")
        _chk(not self.causal or Tq == Tk, f"sdpa {self.name}: causal needs Tq == Tk (Tq={Tq}, Tk={Tk})")
        d = L.MdxSdpaDesc()
        d.Q, d.K, d.V, d.O = _p(Q), _p(K), _p(V), _p(O)
        d.B, d.H, d.Tq, d.Tk, d.d = B, self.heads, Tq, Tk, Cc // self.heads
        d.ldq, d.sQ = Q.stride(1), Q.stride(0)
        d.ldk, d.sK = K.stride(1), K.stride(0)
        d.ldv, d.sV = V.stride(1), V.stride(0)
        d.ldo, d.sO = O.stride(1), O.stride(0)
        d.scale, d.causal = float(self.scale), int(self.causal)
        if self.klen is not None:
            _chk(self.klen.dtype == torch.int32 and self.klen.dim() == 1 and self.klen.numel() == B and self.klen.is_contiguous()
                 and self.klen.device == Q.device, f"sdpa {self.name}: klen must be int32 [B={B}], contiguous, on the device of Q")
            d.klen_dev = _p(self.klen)
        return self.opcode, d


@dataclass
class LatentBlend:
    """Keep known regions of the latents (MdxBlendDesc, csrc/blend.hip), placed BEHIND the scheduler op of a step: with s = step - 1 (the
    scheduler op has advanced the counter) and s in [0, last_step), element i with m = mask[i // (n / mask.numel())] becomes
    m == 0: untouched; m == 1: t = coef[s, col_a] * cond + coef[s, col_s] * noise; else fma(m, t - x, x) — and x_in is refreshed as the
    scheduler ops do.  x, cond, noise fp32 [n] in one layout; mask fp32, one value per n / mask.numel() consecutive elements (per latent
    pixel of an NHWC latent); coef / step / x_in / cfg / xin_c: the scheduler op's.  col_a / col_s: 2, 3 of a DDIM table, 10, 11 of UniPC's.
    The build follows x_in's 16-bit type (dtype_code); with an fp32 x_in or none the two builds are the same kernel."""
    x: torch.Tensor
    cond: torch.Tensor
    noise: torch.Tensor
    mask: torch.Tensor
    coef: torch.Tensor                   # fp32 [steps, 4 | 12]
    step: torch.Tensor                   # int32 [1]
    last_step: int
    col_a: int = -1                      # -1: by the table's width (4 -> 2, 3; 12 -> 10, 11)
    col_s: int = -1
    x_in: Optional[torch.Tensor] = None
    cfg: bool = False
    xin_c: int = 0
    name: str = ""
    opcode = L.OP_LATENT_BLEND

    COLUMNS = {4: (2, 3), 12: (10, 11)}  # (alpha, sigma) of the next timestep in a DDIM / UniPC coefficient row

    def lower(self):
        n = self.x.numel()
        _chk(all(t.dtype == F32 and t.is_contiguous() and t.numel() == n for t in (self.x, self.cond, self.noise)), f"blend {self.name}: x, cond, noise must be fp32, dense, of one size")
        _chk(self.mask.dtype == F32 and self.mask.is_contiguous() and self.mask.numel() > 0 and n % self.mask.numel() == 0,
             f"blend {self.name}: mask must be fp32, dense, with a size dividing n={n}")
        _chk(self.coef.dtype == F32 and self.coef.dim() == 2 and self.coef.is_contiguous() and self.step.dtype == torch.int32 and self.step.numel() == 1,
             f"blend {self.name}: coef fp32 [steps, ld], step int32 [1]")
        ld = self.coef.shape[1]
        col_a, col_s = _columns(f"blend {self.name}", self.COLUMNS, ld, (self.col_a, self.col_s), "col_a / col_s")
        d = L.MdxBlendDesc()
        d.x, d.cond, d.noise, d.mask, d.coef, d.step_ptr = _p(self.x), _p(self.cond), _p(self.noise), _p(self.mask), _p(self.coef), _p(self.step)
        _lower_xin(d, f"blend {self.name}", self.x_in, n, self.cfg, self.xin_c)
        d.mask_elems, d.coef_ld, d.col_a, d.col_s, d.last_step = n // self.mask.numel(), ld, col_a, col_s, int(self.last_step)
        return self.opcode, d


@dataclass
class LatentRenoise:
    """One forward jump of the sampler with device-side Gaussian noise (MdxRenoiseDesc, csrc/noise.hip), launched BETWEEN steps: with
    c = step, v = visit (read on the device), r = coef[c - jump, col_t] / coef[c - 1, col_p] and sg = sqrt(max(0, 1 - r^2)),
    x <- fma(r, x, sg * z), x_in refreshed as the scheduler ops do, then step <- c - jump and visit <- v + 1.  z is Philox4x32-10 +
    Box-Muller of (seeds[g], v, e) for element e of group g (include/mdx.h has the mapping to the bit).  x fp32 [n]; seeds int64 / uint64
    [groups], one per n / groups consecutive elements (a view); coef / step / x_in / cfg / xin_c: the scheduler op's; visit int32 [1].
    col_t / col_p: 0, 2 of a DDIM table (the only one a jump is defined for: UniPC's multistep history does not survive it).
    The build follows x_in's 16-bit type (dtype_code); with an fp32 x_in or none the two builds are the same kernel."""
    x: torch.Tensor
    coef: torch.Tensor                   # fp32 [steps, 4]
    step: torch.Tensor                   # int32 [1], read and written
    visit: torch.Tensor                  # int32 [1], read and written
    seeds: torch.Tensor                  # int64 [groups]
    jump: int
    col_t: int = -1                      # -1: by the table's width (4 -> 0, 2)
    col_p: int = -1
    x_in: Optional[torch.Tensor] = None
    cfg: bool = False
    xin_c: int = 0
    name: str = ""
    opcode = L.OP_LATENT_RENOISE

    COLUMNS = {4: (0, 2)}                # sqrt(abar) of a step's own timestep / of the next one in a DDIM coefficient row

    def lower(self):
        n = self.x.numel()
        _chk(self.x.dtype == F32 and self.x.is_contiguous(), f"renoise {self.name}: x must be fp32, dense")
        _chk(self.seeds.dtype in (torch.int64, torch.uint64) and self.seeds.is_contiguous() and self.seeds.numel() > 0 and n % self.seeds.numel() == 0,
             f"renoise {self.name}: seeds must be int64, dense, with a size dividing n={n}")
        _chk(self.coef.dtype == F32 and self.coef.dim() == 2 and self.coef.is_contiguous() and self.coef.shape[0] >= 1,
             f"renoise {self.name}: coef fp32 [steps, ld]")
        _chk(all(t.dtype == torch.int32 and t.numel() == 1 for t in (self.step, self.visit)), f"renoise {self.name}: step and visit int32 [1]")
        _chk(isinstance(self.jump, int) and not isinstance(self.jump, bool) and self.jump >= 1, f"renoise {self.name}: jump={self.jump!r} must be an integer >= 1")
        ld = self.coef.shape[1]
        col_t, col_p = _columns(f"renoise {self.name}", self.COLUMNS, ld, (self.col_t, self.col_p), "col_t / col_p")
        d = L.MdxRenoiseDesc()
        d.x, d.coef, d.step_ptr, d.visit_ptr, d.seeds = _p(self.x), _p(self.coef), _p(self.step), _p(self.visit), _p(self.seeds)
        _lower_xin(d, f"renoise {self.name}", self.x_in, n, self.cfg, self.xin_c)
        d.group_elems, d.jump, d.n_rows, d.coef_ld, d.col_t, d.col_p = n // self.seeds.numel(), self.jump, self.coef.shape[0], ld, col_t, col_p
        return self.opcode, d


@dataclass
class DdimEtaStep:
    """The DDIM step with eta > 0 (MdxDdimEtaDesc, csrc/noise.hip), in the scheduler op's place: DdimStep's fields and update, plus
    var fp32 [steps, 2] = (dir, std) per step (DDIMScheduler.variance_table), draw int32 [1] (steps of this op taken so far, read and
    written like step) and the source of z: seeds int64 / uint64 [groups], one per n / groups consecutive elements (a view) — Philox4x32-10
    + Box-Muller of (seeds[g], draw, e) in the step's own domain (include/mdx.h has the mapping to the bit) — or noise fp32 [n], the
    caller's own (it wins; groups is then 1 unless seeds is given too).  x <- c2 x0 + dir e + std z; a row with std == 0 and dir = c3
    gives DdimStep's bits.  n_rows: rows of coef and var (by default coef's).  The build follows x_in's 16-bit type (dtype_code)."""
    x: torch.Tensor                      # fp32 [n] latents, updated in place
    eps: torch.Tensor                    # fp32 [c*n] ([uncond | cond] when cfg)
    coef: torch.Tensor                   # fp32 [steps, 4]: DdimStep's table, unchanged
    var: torch.Tensor                    # fp32 [steps, 2]
    step: torch.Tensor                   # int32 [1], read and written
    draw: torch.Tensor                   # int32 [1], read and written
    seeds: Optional[torch.Tensor] = None
    noise: Optional[torch.Tensor] = None
    n_rows: int = -1                     # -1: coef.shape[0]
    x_in: Optional[torch.Tensor] = None
    cfg: bool = False
    guidance: float = 1.0
    xin_c: int = 0
    name: str = ""
    gv_mask: Optional[torch.Tensor] = None
    gv_cond: Optional[torch.Tensor] = None
    gv_noise: Optional[torch.Tensor] = None
    gv_mode: int = 0
    gv_last_step: int = 0
    opcode = L.OP_DDIM_ETA

    def lower(self):
        n = self.x.numel()
        what = f"ddim_eta {self.name}"
        _chk(self.x.dtype == F32 and self.x.is_contiguous(), f"{what}: x must be fp32, dense")
        _chk(self.eps.dtype == F32 and self.eps.is_contiguous() and self.eps.numel() == n * (2 if self.cfg else 1), f"{what}: eps must be fp32, dense, {2 if self.cfg else 1} x n")
        _chk(self.coef.dtype == F32 and self.coef.dim() == 2 and self.coef.is_contiguous() and self.coef.shape[1] == 4 and self.coef.shape[0] >= 1,
             f"{what}: coef fp32 [steps, 4]")
        rows = self.coef.shape[0] if self.n_rows < 0 else self.n_rows
        _chk(isinstance(rows, int) and not isinstance(rows, bool) and 1 <= rows <= self.coef.shape[0], f"{what}: n_rows={self.n_rows!r} must be in [1, {self.coef.shape[0]}]")
        _chk(self.var.dtype == F32 and self.var.is_contiguous() and tuple(self.var.shape) == (self.coef.shape[0], 2), f"{what}: var fp32 [steps={self.coef.shape[0]}, 2]")
        _chk(all(t.dtype == torch.int32 and t.numel() == 1 for t in (self.step, self.draw)), f"{what}: step and draw int32 [1]")
        _chk(self.seeds is not None or self.noise is not None, f"{what}: seeds or noise must be given")
        groups = 1
        if self.seeds is not None:
            _chk(self.seeds.dtype in (torch.int64, torch.uint64) and self.seeds.is_contiguous() and self.seeds.numel() > 0 and n % self.seeds.numel() == 0,
                 f"{what}: seeds must be int64, dense, with a size dividing n={n}")
            groups = self.seeds.numel()
        if self.noise is not None:
            _chk(self.noise.dtype == F32 and self.noise.is_contiguous() and self.noise.numel() == n, f"{what}: noise must be fp32, dense, of x's size")
        d = L.MdxDdimEtaDesc()
        d.x, d.eps, d.coef, d.var, d.step_ptr, d.draw_ptr = _p(self.x), _p(self.eps), _p(self.coef), _p(self.var), _p(self.step), _p(self.draw)
        d.seeds, d.noise, d.guidance = _p(self.seeds), _p(self.noise), float(self.guidance)
        _lower_xin(d, what, self.x_in, n, self.cfg, self.xin_c)
        _lower_given_views(d, what, n, self.gv_mode, self.gv_mask, self.gv_cond, self.gv_noise, self.gv_last_step)
        d.group_elems, d.n_rows = max(n // groups, 1), rows
        return self.opcode, d


@dataclass
class ImageComposite:
    """Composite a kept-region edit with the recorded pictures (MdxCompositeDesc, csrc/composite.hip), on the VAE decoder's output.
    gen [V, C, H, W] in [-1, 1]: bf16, fp16 or fp32, a view with unit inner stride (a channel slice or a wider row pitch is taken as it
    is); orig fp32 [V, H, W, C] in [0, 1]; keep fp32 [V, H / f, W / f]; out fp32 [V, H, W, C]; matte None or fp32 [V, H, W]; has None or
    uint8 [V] (0: no picture for this view — out is the plain picture, the matte 0).  With w the matte of magicdrive_amd.dataset.edit_matte
    (keep, f, feather) and g = (gen / 2 + 0.5).clamp(0, 1).float(): out = g where w == 0, orig where w == 1, fma(w, orig - g, g) between."""
    gen: torch.Tensor
    orig: torch.Tensor
    keep: torch.Tensor
    out: torch.Tensor
    feather: int
    matte: Optional[torch.Tensor] = None
    has: Optional[torch.Tensor] = None
    name: str = ""
    opcode = L.OP_IMAGE_COMPOSITE

    def lower(self):
        gen, orig, keep, out = self.gen, self.orig, self.keep, self.out
        what = f"composite {self.name}"
        _chk(gen.dim() == 4 and gen.dtype in (F32,) + H16, f"{what}: gen must be [V, C, H, W], fp32 or 16-bit, got {tuple(gen.shape)} {gen.dtype}")
        V, Cc, H, W = gen.shape
        _chk(1 <= Cc <= 4 and H >= 1 and W >= 1, f"{what}: gen {tuple(gen.shape)}: 1 to 4 channels, H, W >= 1")
        _chk((W == 1 or gen.stride(3) == 1) and (H == 1 or gen.stride(2) >= W) and all(s >= 0 for s in gen.stride()), f"{what}: gen needs a unit inner stride and a row stride >= W, got {gen.stride()}")
        _chk(orig.dtype == F32 and tuple(orig.shape) == (V, H, W, Cc) and orig.is_contiguous(), f"{what}: orig must be fp32 [V, H, W, C] = {(V, H, W, Cc)}, dense")
        _chk(out.dtype == F32 and tuple(out.shape) == (V, H, W, Cc) and out.is_contiguous(), f"{what}: out must be fp32 [V, H, W, C] = {(V, H, W, Cc)}, dense")
        _chk(keep.dtype == F32 and keep.dim() == 3 and keep.shape[0] == V and keep.is_contiguous() and keep.shape[1] >= 1 and keep.shape[2] >= 1,
             f"{what}: keep must be fp32 [V, h, w], dense")
        f = H // keep.shape[1]
        _chk(f >= 1 and keep.shape[1] * f == H and keep.shape[2] * f == W, f"{what}: keep {tuple(keep.shape[1:])} is not the image {(H, W)} divided by one whole factor")
        _chk(isinstance(self.feather, int) and not isinstance(self.feather, bool) and 0 <= self.feather <= 16, f"{what}: feather={self.feather!r} must be an integer in [0, 16]")
        if self.matte is not None:
            _chk(self.matte.dtype == F32 and tuple(self.matte.shape) == (V, H, W) and self.matte.is_contiguous(), f"{what}: matte must be fp32 [V, H, W], dense")
        if self.has is not None:
            _chk(self.has.dtype == torch.uint8 and tuple(self.has.shape) == (V,) and self.has.is_contiguous(), f"{what}: has must be uint8 [V]")
        others = [t for t in (orig, keep, out, self.matte, self.has) if t is not None]
        _chk(all(t.device == gen.device for t in others), f"{what}: every operand must be on the device of gen")
        d = L.MdxCompositeDesc()
        d.gen, d.orig, d.keep, d.out, d.matte, d.has = _p(gen), _p(orig), _p(keep), _p(out), _p(self.matte), _p(self.has)
        d.V, d.C, d.H, d.W, d.f, d.feather, d.gen_f32 = V, Cc, H, W, f, self.feather, int(gen.dtype == F32)
        d.g_sv, d.g_sc, d.g_ld = (gen.stride(0) if V > 1 else Cc * H * gen.stride(2)), (gen.stride(1) if Cc > 1 else 0), (gen.stride(2) if H > 1 else W)
        return self.opcode, d


def sdpa(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int, *, scale: Optional[float] = None, causal: bool = False,
         key_lengths: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """softmax(scale * q k^T + mask) v per head on the GPU kernel behind mdx_sdpa_* (ops.Sdpa), on torch's current stream.
    q [B,Tq,H*d], k, v [B,Tk,H*d]: bf16 or fp16 tensors or strided views with unit inner stride (the column blocks of a fused projection
    buffer are passed as they are: nothing is copied).  scale defaults to d ** -0.5; key_lengths is int32 [B] on the device.  Returns
    `out`, or a new [B,Tq,H*d] tensor."""
    for t in (q, k, v):
        if t.dtype not in H16:
            raise TypeError(f"ops.sdpa takes bfloat16 or float16 tensors, got {t.dtype}")
    for t in (q, k, v):
        if not t.is_cuda:
            raise RuntimeError("magicdrive_amd: ops.sdpa runs on the MI355X only (no CPU fallback)")
    _chk(q.dim() == 3 and heads > 0 and q.shape[2] % heads == 0, f"sdpa: q must be [B, Tq, H*d] with H={heads}, got {tuple(q.shape)}")
    if scale is None:
        scale = (q.shape[2] // heads) ** -0.5
    if out is None:
        out = torch.empty(q.shape, dtype=q.dtype, device=q.device)
    run_ops([Sdpa(q, k, v, out, heads=heads, scale=scale, causal=causal, klen=key_lengths)])
    return out


def image_composite(gen: torch.Tensor, orig: torch.Tensor, keep: torch.Tensor, feather: int, *, has: Optional[torch.Tensor] = None,
                    return_matte: bool = False):
    """Composite decoded views with their recorded pictures on the GPU kernel behind mdx_image_composite_* (ops.ImageComposite), on
    torch's current stream.  gen [V, C, H, W] (bf16, fp16 or fp32, in [-1, 1]), orig fp32 [V, H, W, C] in [0, 1], keep fp32
    [V, H / f, W / f], feather in image pixels (0 to 16), has uint8 [V] or None.  Returns out fp32 [V, H, W, C], or (out, matte [V, H, W])."""
    for t in (gen, orig, keep):
        if not t.is_cuda:
            raise RuntimeError("magicdrive_amd: ops.image_composite runs on the MI355X only (no CPU fallback; dataset.edit_matte states the matte in torch)")
    _chk(gen.dim() == 4, f"image_composite: gen must be [V, C, H, W], got {tuple(gen.shape)}")
    V, Cc, H, W = gen.shape
    out = torch.empty(V, H, W, Cc, dtype=F32, device=gen.device)
    matte = torch.empty(V, H, W, dtype=F32, device=gen.device) if return_matte else None
    run_ops([ImageComposite(gen, orig, keep, out, feather, matte=matte, has=has)])
    return (out, matte) if return_matte else out


def dtype_code(op) -> int:
    """MdxOp.dtype of an IR op: fp16 when its 16-bit tensors are torch.float16, else bf16 (ops without 16-bit tensors run either build)."""
    for v in vars(op).values():
        if isinstance(v, torch.Tensor):
            if v.dtype == F16:
                return L.DTYPE_F16
            if v.dtype == BF16:
                return L.DTYPE_BF16
    return L.DTYPE_BF16


def lower_with_dtype(op):
    code, desc = op.lower()
    return code, desc, dtype_code(op)


def build_program(ops) -> L.Program:
    return L.Program([lower_with_dtype(op) for op in ops])


def run_ops(ops, stream: Optional[int] = None) -> None:
    """Eagerly launch a list of IR ops on `stream` (default: torch's current stream)."""
    if stream is None:
        dev = None
        for op in ops:                       # launch on the device that owns the operands, not on whatever device is current
            for v in vars(op).values():
                if isinstance(v, torch.Tensor) and v.is_cuda:
                    dev = v.device
                    break
            if dev is not None:
                break
        if dev is None:
            raise RuntimeError("magicdrive_amd: ops run on the MI355X only (no CPU fallback): none of the operands is a CUDA / HIP tensor")
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            for op in ops:
                L.call_op(*op.lower(), stream, dtype_code(op))
        return
    for op in ops:
        L.call_op(*op.lower(), stream, dtype_code(op))
