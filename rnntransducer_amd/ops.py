"""torch.autograd wrappers over the C ABI (include/rnnt_hip.h).  PyTorch here is plumbing only: it owns
device memory and the stream and records the graph; every FLOP below runs in librnnt_hip.so.

All internal activations are TIME-MAJOR (T,B,F): one LSTM step touches one contiguous (B,F) slab.
"""
from __future__ import annotations

import ctypes as C
import math
import os
import re
from typing import List, NamedTuple, Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import (GEMM_ACCUM, GEMM_GELU_A, GEMM_GELU_B, GEMM_HP_F16, GEMM_MUL_DGELU, PRECISION_F16, PRECISION_FP32, GemmDesc, LstmBwdDesc,
                   LstmDesc, RnntHipError, check)

BIG = 1 << 40  # "no second level" divisor for the GEMM row maps


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _need_gpu(*tensors: torch.Tensor) -> None:
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RnntHipError("rnntransducer_amd runs on the MI355X only: got a CPU tensor. There is no CPU or "
                               "eager fallback; move the module and the batch to cuda:<n>.")


def _f32c(t: torch.Tensor, name: str) -> torch.Tensor:
    if t.dtype != torch.float32:
        raise ValueError(f"{name} must be float32, got {t.dtype}")
    return t if t.is_contiguous() else t.contiguous()


def _addr(t: Optional[torch.Tensor], elem_off: int = 0) -> Optional[int]:
    if t is None:
        return None
    return t.data_ptr() + elem_off * t.element_size()


# --------------------------------------------------------------------------------------------------
# flat-gradient targets (optim.FlatAdamW(direct_grads=True) tags its parameters): backward kernels then ADD their weight
# gradients straight into the parameter's `.grad` view of the flat buffer and hand autograd `None`, instead of returning
# a fresh tensor that autograd would `+=` into the view with one extra kernel per parameter.
# --------------------------------------------------------------------------------------------------
def _direct_grad(param: torch.Tensor) -> Optional[torch.Tensor]:
    g = param.grad if getattr(param, "_rnnt_direct_grad", False) else None
    if g is None or not g.is_contiguous() or g.dtype != torch.float32 or g.shape != param.shape:
        return None
    return g


# --------------------------------------------------------------------------------------------------
# sticky status word of the persistent recurrences (include/rnnt_hip.h: rnnt_lstm_desc.status), one per device.
# Kernels raise it when an inter-workgroup wait is abandoned; nothing in the library clears it.  FlatAdamW hands it to
# the update kernel as a guard and reads it back asynchronously once per step; `lstm_status_check` is the explicit read.
# --------------------------------------------------------------------------------------------------
_STATUS = {}


def lstm_status_word(device) -> torch.Tensor:
    dev = torch.device(device)
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    w = _STATUS.get(idx)
    if w is None:
        w = torch.zeros(4, dtype=torch.int32, device=torch.device("cuda", idx))
        _STATUS[idx] = w
    return w


def lstm_status_check(device=None) -> None:
    """Synchronous read of the device's sticky status word; raises RnntHipError if a persistent LSTM kernel gave up on an
    inter-workgroup wait (its outputs, and every later LSTM launch on this device, are invalid).  Clears the word so a
    caller that handles the exception can go on."""
    for idx, w in list(_STATUS.items()):
        if device is not None and torch.device(device).index not in (None, idx):
            continue
        if int(w[0].item()) != 0:
            w.zero_()
            raise RnntHipError("a persistent LSTM kernel abandoned an inter-workgroup wait (its workgroups were not "
                               "co-resident for 4 s — is another kernel holding the CUs?): activations and gradients "
                               "of that step are invalid; the guarded AdamW update was skipped")


# --------------------------------------------------------------------------------------------------
# raw GEMM
# --------------------------------------------------------------------------------------------------
def _gemm_desc(M: int, N: int, K: int, A: torch.Tensor, B: torch.Tensor, Cout: torch.Tensor, *, a_off=0, a_div=BIG, a_so=0,
               a_si=None, a_sk=1, a_mc=False, a_rowidx=None, b_off=0, b_sn=None, b_sk=1, c_off=0, c_div=BIG, c_so=0, c_si=None,
               bias=None, aux=None, flags=0, split_k=None, need_ws=True):
    """The descriptor of one gemm() call and the tensor that owns its split-K workspace (None without one).  need_ws=False: only
    the workspace's size is entered (rnnt_hip_gemm_plan reads the size and whether the pointer is null, never the memory)."""
    d = GemmDesc()
    ws = None
    if split_k is None:
        split_k = M * N <= (1 << 21)
    if split_k:
        nws = _lib.lib().rnnt_hip_gemm_workspace_bytes(M, N, K)
        if nws:
            ws = torch.empty(nws if need_ws else 16, device=Cout.device, dtype=torch.uint8)
            d.workspace, d.workspace_bytes = _addr(ws), nws
    d.M, d.N, d.K = M, N, K
    d.A = _addr(A, a_off)
    d.a_div, d.a_so, d.a_si, d.a_sk = a_div, a_so, (K if a_si is None else a_si), a_sk
    d.a_mc = 1 if a_mc else 0
    d.a_rowidx = _addr(a_rowidx)
    d.B = _addr(B, b_off)
    d.b_sn, d.b_sk = (K if b_sn is None else b_sn), b_sk
    d.C = _addr(Cout, c_off)
    d.c_div, d.c_so, d.c_si = c_div, c_so, (N if c_si is None else c_si)
    d.bias = _addr(bias)
    d.aux = _addr(aux, c_off)   # aux is laid out like C: element (m, n) of both sits at the same mapped offset behind c_off
    d.flags = flags
    return d, ws


def gemm(M: int, N: int, K: int, A: torch.Tensor, B: torch.Tensor, Cout: torch.Tensor, **kw) -> None:
    """C(m,n) = sum_k A(m,k) B(k,n) (+bias) — see include/rnnt_hip.h for the operand maps.  Keywords: a_off=0, a_div=BIG, a_so=0,
    a_si=K, a_sk=1, a_mc=False, a_rowidx=None, b_off=0, b_sn=K, b_sk=1, c_off=0, c_div=BIG, c_so=0, c_si=N, bias=None, aux=None,
    flags=0, split_k=None.
    split_k=True hands the kernel a slab workspace so small-output / deep-K products (weight gradients) fill the chip;
    None (default): do so when the output is small (<= 2^21 elements: the prediction net's and the joint's products)."""
    _need_gpu(A, B, Cout)
    d, ws = _gemm_desc(M, N, K, A, B, Cout, **kw)
    check(_lib.lib().rnnt_hip_gemm_f32(C.byref(d), _stream()), "rnnt_hip_gemm_f32")


class GemmPlan(NamedTuple):
    """What one gemm() call launches (rnnt_hip_gemm_plan): arithmetic mode (6 / 3 / 0), tile (rows, columns), operand layouts,
    vector or scalar operand loads, workgroups per K slab, split-K slab count (1 = no split) and depth."""
    mode: int
    tile: Tuple[int, int]
    a_kc: bool
    b_kc: bool
    vec: bool
    tiles: int
    splits: int
    kchunk: int


def gemm_plan(M: int, N: int, K: int, A: torch.Tensor, B: torch.Tensor, Cout: torch.Tensor, **kw) -> GemmPlan:
    """The plan of the gemm() call with these arguments, from the function that call takes its decisions from; launches nothing
    (the tensors are looked at for their addresses only, so any device serves)."""
    d, ws = _gemm_desc(M, N, K, A, B, Cout, need_ws=False, **kw)
    p = _lib.GemmPlan()
    check(_lib.lib().rnnt_hip_gemm_plan(C.byref(d), C.byref(p)), "rnnt_hip_gemm_plan")
    return GemmPlan(p.mode, (p.tile_m, p.tile_n), bool(p.a_kc), bool(p.b_kc), bool(p.vec), p.tiles, p.splits, p.kchunk)


# --------------------------------------------------------------------------------------------------
# half-pair (hp) operands + the f16-MFMA GEMM on them (include/rnnt_hip.h).  The LSTM entry points use these internally for
# their big products; exposed here for tests and tools.
# --------------------------------------------------------------------------------------------------
class HpTensor:
    """hp planes of an fp32 matrix (rows x K): device byte buffer + the per-row amax words the row scales derive from."""

    def __init__(self, rows: int, K: int, device):
        self.rows, self.K = int(rows), int(K)
        n = _lib.lib().rnnt_hip_hp_bytes(self.rows, self.K)
        self.planes = torch.empty(max(n, 128), device=device, dtype=torch.uint8)
        self.amax = torch.empty(max(self.rows, 1), device=device, dtype=torch.int32)   # per-row maxima (fp32 bit patterns), written by the split


def hp_split(x: torch.Tensor, transpose: bool = False, shift: int = 0, K: Optional[int] = None) -> HpTensor:
    """x (rows, K) fp32 -> HpTensor(rows, K).  transpose=True: x is (src_rows, rows); plane row r, index k = x[k + shift, r]
    (zero outside the source), contraction length K (default src_rows)."""
    _need_gpu(x)
    x = _f32c(x, "x")
    if x.dim() != 2:
        raise ValueError("hp_split takes a 2-D tensor")
    if not transpose:
        rows, kk = x.shape
        t = HpTensor(rows, kk, x.device)
        check(_lib.lib().rnnt_hip_hp_split(_addr(x), rows, kk, kk, 0, 0, 0, _addr(t.planes), _addr(t.amax), 0, _stream()), "hp_split")
        return t
    src_rows, rows = x.shape
    kk = src_rows if K is None else int(K)
    t = HpTensor(rows, kk, x.device)
    check(_lib.lib().rnnt_hip_hp_split(_addr(x), rows, kk, rows, 1, src_rows, int(shift), _addr(t.planes), _addr(t.amax), 0, _stream()),
          "hp_split")
    return t


def gemm_hp(a: HpTensor, b: HpTensor, out: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None,
            accumulate: bool = False, split_k: bool = True, f16: bool = False) -> torch.Tensor:
    """C (M, N) [+]= A (M, K) . B (N, K)^T + bias on hp operands.  f16=True: the one-product form (RNNT_GEMM_HP_F16) — only the hi
    halves are multiplied (f16 operand rounding, fp32 accumulation)."""
    if a.K != b.K:
        raise ValueError(f"contraction lengths differ: {a.K} vs {b.K}")
    M, N, K = a.rows, b.rows, a.K
    if out is None:
        out = torch.empty(M, N, device=a.planes.device, dtype=torch.float32)
    if tuple(out.shape) != (M, N) or not out.is_contiguous() or out.dtype != torch.float32:
        raise ValueError(f"out must be a contiguous float32 ({M}, {N}) tensor")
    if bias is not None and tuple(bias.shape) != (N,):
        raise ValueError(f"bias must be ({N},)")
    nws = _lib.lib().rnnt_hip_gemm_hp_workspace_bytes(M, N, K) if split_k else 0
    ws = torch.empty(nws, device=out.device, dtype=torch.uint8) if nws else None
    check(_lib.lib().rnnt_hip_gemm_hp(_addr(a.planes), _addr(a.amax), _addr(b.planes), _addr(b.amax), M, N, K, _addr(out), N, _addr(bias),
                                      (GEMM_ACCUM if accumulate else 0) | (GEMM_HP_F16 if f16 else 0), _addr(ws), nws, _stream()),
          "rnnt_hip_gemm_hp")
    return out


def gemm_hp_grouped(pairs, outs=None, accumulate=False, xcd_skip: int = 0, check: bool = False, f16: bool = False,
                    workspace_bytes: Optional[int] = None):
    """[C_i (M_i, N_i) [+]= A_i . B_i^T] for up to 4 (A, B) pairs of hp operands in ONE queue-driven launch; `xcd_skip`: bit mask of
    XCDs whose workgroups leave at once (the launch then runs on the other XCDs only).  `check`: read back (synchronising) the
    launch's self-check — word 9 of the workspace is 1 when units were left undone because the mask named XCDs the device does not
    expose (include/rnnt_hip.h) — and raise RnntHipError in that case.  f16=True: every product in the one-product form (as gemm_hp).
    outs[i] may be a column block of a wider matrix (unit column stride, row stride ldc >= N_i); `accumulate` may be one flag per
    problem; `workspace_bytes`: hand the launch this much instead of what rnnt_hip_gemm_hp_grouped_workspace_bytes asks for (>= 256:
    the split-K slabs shrink to fit)."""
    n = len(pairs)
    if not 1 <= n <= 4:
        raise ValueError("1..4 products per grouped launch")
    acc = list(accumulate) if isinstance(accumulate, (list, tuple)) else [bool(accumulate)] * n
    if len(acc) != n:
        raise ValueError("one accumulate flag per problem")
    pr = (_lib.HpProblem * n)()
    res = []
    for i, (a, b) in enumerate(pairs):
        if a.K != b.K:
            raise ValueError(f"contraction lengths differ: {a.K} vs {b.K}")
        out = outs[i] if outs is not None else torch.empty(a.rows, b.rows, device=a.planes.device, dtype=torch.float32)
        if tuple(out.shape) != (a.rows, b.rows) or out.dtype != torch.float32 or (b.rows > 1 and out.stride(1) != 1) \
                or (a.rows > 1 and out.stride(0) < b.rows):
            raise ValueError(f"out[{i}] must be a float32 ({a.rows}, {b.rows}) tensor with unit column stride and row stride >= {b.rows}")
        pr[i].A, pr[i].a_amax, pr[i].B, pr[i].b_amax = _addr(a.planes), _addr(a.amax), _addr(b.planes), _addr(b.amax)
        pr[i].M, pr[i].N, pr[i].K, pr[i].C, pr[i].ldc = a.rows, b.rows, a.K, _addr(out), max(out.stride(0), b.rows)
        pr[i].flags = (GEMM_ACCUM if acc[i] else 0) | (GEMM_HP_F16 if f16 else 0)
        res.append(out)
    nws = _lib.lib().rnnt_hip_gemm_hp_grouped_workspace_bytes(pr, n) if workspace_bytes is None else int(workspace_bytes)
    ws = torch.empty(max(nws, 256), device=res[0].device, dtype=torch.uint8)
    _lib.check(_lib.lib().rnnt_hip_gemm_hp_grouped(pr, n, int(xcd_skip), _addr(ws), nws, _stream()), "rnnt_hip_gemm_hp_grouped")
    if check:
        words = ws[:64].view(torch.int32).tolist()
        if words[9] != 0:
            raise RnntHipError(f"grouped half-pair GEMM left units undone ({words[8]} drawn): xcd_skip = {xcd_skip:#x} names XCDs this "
                               "device does not expose")
    return res


# The index tables and the C map the ragged batches of the LSTM layers run these kernels with (rnnt_hip_*_ex, include/rnnt_hip.h), on
# caller-owned buffers: for the tests that poison everything a call does not own.  `off`: element offset of the view into `x` / `out`.
def hp_split_ex(x: torch.Tensor, rows: int, K: int, ld: int, planes: torch.Tensor, amax: torch.Tensor, *, off: int = 0,
                transpose: bool = False, src_rows: int = 0, shift: int = 0, idx: Optional[torch.Tensor] = None,
                amax_given: bool = False) -> None:
    """rnnt_hip_hp_split_ex: idx (int32, device) = rowidx of the row-major form (length rows) / kidx of the transposed form (length K)."""
    _need_gpu(x, planes, amax, idx)
    if idx is not None and (idx.dtype != torch.int32 or idx.numel() != (K if transpose else rows)):
        raise ValueError("idx must be int32 with one entry per listed row")
    check(_lib.lib().rnnt_hip_hp_split_ex(_addr(x, off), rows, K, ld, 1 if transpose else 0, src_rows, int(shift), _addr(planes),
                                          _addr(amax), 1 if amax_given else 0, _addr(idx), _stream()), "rnnt_hip_hp_split_ex")


def hp_split_both_ex(x: torch.Tensor, M: int, Cc: int, ld: int, rowmax: torch.Tensor, colmax: torch.Tensor, planes_rm: torch.Tensor,
                     planes_t: torch.Tensor, *, off: int = 0, rowidx: Optional[torch.Tensor] = None) -> None:
    _need_gpu(x, rowmax, colmax, planes_rm, planes_t, rowidx)
    if rowidx is not None and (rowidx.dtype != torch.int32 or rowidx.numel() != M):
        raise ValueError("rowidx must be int32 with M entries")
    check(_lib.lib().rnnt_hip_hp_split_both_ex(_addr(x, off), M, Cc, ld, _addr(rowmax), _addr(colmax), _addr(planes_rm), _addr(planes_t),
                                               _addr(rowidx), _stream()), "rnnt_hip_hp_split_both_ex")


def hp_colmax(x: torch.Tensor, rows: int, Cc: int, ld: int, amax: torch.Tensor, *, off: int = 0) -> None:
    """amax[c] (int32 words: fp32 bit patterns) = max_r |x[off + r * ld + c]|."""
    _need_gpu(x, amax)
    check(_lib.lib().rnnt_hip_hp_colmax(_addr(x, off), rows, Cc, ld, _addr(amax), _stream()), "rnnt_hip_hp_colmax")


class HpGemmPlan(NamedTuple):
    """What one gemm_hp / gemm_hp_ex call launches (rnnt_hip_gemm_hp_plan): 256 x 256 tiles, band height of the tile walk, split-K
    slabs (1 = one pass), K-tiles of 32 per slab, and the workspace the launch would like."""
    tiles_m: int
    tiles_n: int
    group_m: int
    splits: int
    kt_per_split: int
    workspace_bytes_wanted: int


def gemm_hp_plan(M: int, N: int, K: int, workspace_bytes: Optional[int] = None) -> HpGemmPlan:
    """workspace_bytes=None: a workspace of the size the query asks for (what gemm_hp(split_k=True) hands over); 0: none."""
    if workspace_bytes is None:
        workspace_bytes = _lib.lib().rnnt_hip_gemm_hp_workspace_bytes(M, N, K)
    p = _lib.HpGemmPlan()
    check(_lib.lib().rnnt_hip_gemm_hp_plan(M, N, K, int(workspace_bytes), C.byref(p)), "rnnt_hip_gemm_hp_plan")
    return HpGemmPlan(p.tiles_m, p.tiles_n, p.group_m, p.splits, p.kt_per_split, p.workspace_bytes_wanted)


def gemm_hp_ex(a_planes: torch.Tensor, a_amax: torch.Tensor, b_planes: torch.Tensor, b_amax: torch.Tensor, M: int, N: int, K: int,
               out: torch.Tensor, *, c_off: int = 0, c_div: int = 1, c_so: Optional[int] = None, c_si: int = 0,
               bias: Optional[torch.Tensor] = None, flags: int = 0, a_rowidx: Optional[torch.Tensor] = None, a_plane_rows: int = 0,
               c_rowidx: Optional[torch.Tensor] = None, workspace_bytes: Optional[int] = None) -> None:
    """rnnt_hip_gemm_hp_ex on caller-owned buffers.  workspace_bytes as in gemm_hp_plan."""
    _need_gpu(a_planes, a_amax, b_planes, b_amax, out, bias, a_rowidx, c_rowidx)
    for t in (a_rowidx, c_rowidx):
        if t is not None and (t.dtype != torch.int32 or t.numel() != M):
            raise ValueError("row index tables must be int32 with M entries")
    if workspace_bytes is None:
        workspace_bytes = _lib.lib().rnnt_hip_gemm_hp_workspace_bytes(M, N, K)
    ws = torch.empty(workspace_bytes, device=out.device, dtype=torch.uint8) if workspace_bytes else None
    d = _lib.HpGemmDesc()
    d.A, d.a_amax, d.B, d.b_amax = _addr(a_planes), _addr(a_amax), _addr(b_planes), _addr(b_amax)
    d.M, d.N, d.K, d.C = M, N, K, _addr(out, c_off)
    d.c_div, d.c_so, d.c_si = c_div, (N if c_so is None else c_so), c_si
    d.bias, d.flags = _addr(bias), flags
    d.workspace, d.workspace_bytes = _addr(ws), int(workspace_bytes)
    d.a_rowidx, d.a_plane_rows, d.c_rowidx = _addr(a_rowidx), a_plane_rows, _addr(c_rowidx)
    check(_lib.lib().rnnt_hip_gemm_hp_ex(C.byref(d), _stream()), "rnnt_hip_gemm_hp_ex")


def colsum(X: torch.Tensor, M: int, N: int, ld: Optional[int] = None, into: Optional[torch.Tensor] = None):
    """Column sums of X (M,N).  `into`: add them to this (N,) tensor (a flat-gradient view) and return None."""
    out = torch.empty(N, device=X.device, dtype=torch.float32) if into is None else into
    nws = _lib.lib().rnnt_hip_colsum_workspace_bytes(M, N)
    ws = torch.empty(max(nws, 16), device=X.device, dtype=torch.uint8)
    fn = _lib.lib().rnnt_hip_colsum_f32 if into is None else _lib.lib().rnnt_hip_colsum_f32_acc
    check(fn(_addr(X), M, N, N if ld is None else ld, _addr(out), _addr(ws), nws, _stream()), "colsum")
    return out if into is None else None


# --------------------------------------------------------------------------------------------------
# Linear: y = x W^T + b on rows of a 2-D view (replaces nn.Linear: encoder.py:76,103; decoder.py:80,124)
# --------------------------------------------------------------------------------------------------
class LinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, W, bias):
        _need_gpu(x, W, bias)
        x = _f32c(x, "x")
        W0 = _f32c(W, "weight")
        lead, K = x.shape[:-1], x.shape[-1]
        N = W.shape[0]
        if W.dim() != 2 or W.shape[1] != K or (bias is not None and tuple(bias.shape) != (N,)):
            raise ValueError(f"linear: x (..., {K}) needs weight (N, {K}) and bias (N,); got weight {tuple(W.shape)}, "
                             f"bias {None if bias is None else tuple(bias.shape)}")
        M = x.numel() // K
        y = torch.empty(*lead, N, device=x.device, dtype=torch.float32)
        # big products (the encoder's out_proj: 32000 x 512 x 1024 at config 2) take the half-pair f16 path of the LSTM layers'
        # products (include/rnnt_hip.h: same fp32-grade arithmetic, 440 instead of 140-150 TFLOP/s); its operand splits only pay
        # for themselves on deep, wide shapes
        # (an operand whose planes reach 4 GB is beyond gemm_hp.hip's 32-bit buffer offsets: such a product stays on gemm.hip)
        hpb = _lib.lib().rnnt_hip_hp_bytes
        ctx.hp = (M >= 1024 and N >= 256 and K >= 1024 and not os.environ.get("RNNT_GEMM_NO_HP")
                  and max(hpb(M, K), hpb(K, M), hpb(M, N), hpb(N, M)) < (1 << 32))
        if ctx.hp:
            gemm_hp(hp_split(x.view(M, K)), hp_split(W0), out=y.view(M, N), bias=bias)
        else:
            gemm(M, N, K, x, W0, y, bias=bias)
        ctx.save_for_backward(x, W0)
        ctx.has_bias = bias is not None
        ctx.w_param, ctx.b_param = W, bias  # the Parameter objects themselves (for their flat .grad views)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, W = ctx.saved_tensors
        dy = _f32c(dy, "dy")
        N, K = W.shape
        M = x.numel() // K
        dx = dW = db = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            if ctx.hp:
                gemm_hp(hp_split(dy.view(M, N)), hp_split(W, transpose=True), out=dx.view(M, K))   # dx = dy . W
            else:
                gemm(M, K, N, dy, W, dx, b_sn=1, b_sk=K)          # dx = dy . W
        if ctx.needs_input_grad[1]:
            tgt = _direct_grad(ctx.w_param)
            dW = torch.empty_like(W) if tgt is None else None
            if ctx.hp:   # dW = dy^T . x: both operands row-major over the contraction index M (transposed splits), split-K slabs
                gemm_hp(hp_split(dy.view(M, N), transpose=True), hp_split(x.view(M, K), transpose=True),
                        out=dW if tgt is None else tgt, accumulate=tgt is not None)
            else:
                gemm(N, K, M, dy, x, dW if tgt is None else tgt, a_mc=True, a_sk=N, b_sn=1, b_sk=K, split_k=True,
                     flags=0 if tgt is None else GEMM_ACCUM)  # dW = dy^T . x
        if ctx.has_bias and ctx.needs_input_grad[2]:
            db = colsum(dy, M, N, into=_direct_grad(ctx.b_param))
        return dx, dW, db


# --------------------------------------------------------------------------------------------------
# Embedding (networks/decoder.py:69,102)
# --------------------------------------------------------------------------------------------------
class EmbeddingFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, W, idx, padding_idx):
        _need_gpu(W, idx)
        W_param = W
        W = _f32c(W, "embedding.weight")
        if idx.dtype != torch.int64:
            raise ValueError(f"token ids must be int64 (dataloader.py:28-36), got {idx.dtype}")
        idx = idx.contiguous()
        V, H = W.shape
        out = torch.empty(*idx.shape, H, device=W.device, dtype=torch.float32)
        check(_lib.lib().rnnt_hip_embedding_fwd(_addr(W), _addr(idx), idx.numel(), H, V, _addr(out), _stream()), "embedding_fwd")
        ctx.save_for_backward(idx)
        ctx.shape = (V, H)
        ctx.padding_idx = -1 if padding_idx is None else int(padding_idx)
        ctx.w_param = W_param
        return out

    @staticmethod
    def backward(ctx, dE):
        (idx,) = ctx.saved_tensors
        V, H = ctx.shape
        dE = _f32c(dE, "dE")
        tgt = _direct_grad(ctx.w_param)
        if tgt is not None:
            check(_lib.lib().rnnt_hip_embedding_bwd_acc(_addr(dE), _addr(idx), idx.numel(), H, V, ctx.padding_idx, _addr(tgt),
                                                        _stream()), "embedding_bwd_acc")
            return None, None, None
        dW = torch.zeros(V, H, device=dE.device, dtype=torch.float32)
        check(_lib.lib().rnnt_hip_embedding_bwd(_addr(dE), _addr(idx), idx.numel(), H, V, ctx.padding_idx, _addr(dW),
                                                _stream()), "embedding_bwd")
        return dW, None, None


# --------------------------------------------------------------------------------------------------
# LSTM stack (replaces nn.LSTM over a PackedSequence: encoder.py:67-75,93-102; decoder.py:71-79,105-120)
# --------------------------------------------------------------------------------------------------
class RaggedPlan:
    """Valid-frame table of a padded time-major batch (rnnt_lstm_desc.row_idx): what pack_padded_sequence buys the reference
    (networks/encoder.py:93-96,99-101) without a packed copy.  Built on the HOST from the python list of lengths the reference's
    collate hands over (dataloader.py:20) — no device synchronisation — and uploaded once per batch: `row_idx` lists the rows
    t*B + b with t < lens[b] in ascending order, `n_rows` = sum(lens).  Pass it to HipLSTM / LstmStackFn in place of `lens`."""

    def __init__(self, lens_host: Sequence[int], T: int, device):
        import numpy as np
        lens_np = np.asarray(list(lens_host), dtype=np.int64)
        if lens_np.ndim != 1 or lens_np.size < 1 or lens_np.min() < 1 or lens_np.max() > T:
            raise ValueError(f"lengths must lie in [1, {T}]")
        self.T, self.B = int(T), int(lens_np.size)
        idx = np.flatnonzero((np.arange(T, dtype=np.int64)[:, None] < lens_np[None, :]).reshape(-1)).astype(np.int32)
        self.n_rows = int(idx.size)
        self.dense = self.n_rows == self.T * self.B
        self.lens = torch.from_numpy(lens_np.astype(np.int32)).to(device, non_blocking=True)
        self.row_idx = None if self.dense else torch.from_numpy(idx).to(device, non_blocking=True)


def lstm_workspace(T: int, B: int, I: int, H: int, D: int, device) -> torch.Tensor:
    n = _lib.lib().rnnt_hip_lstm_workspace_bytes(T, B, I, H, D)
    if n == 0:
        raise RnntHipError(f"LSTM configuration not supported by the HIP kernels: T={T} B={B} I={I} H={H} D={D} "
                           "(need H % 4 == 0, 1 <= B <= 64, D in {1,2})")
    return torch.empty(n, device=device, dtype=torch.uint8)


def _fill_lstm_desc(d: LstmDesc, T, B, I, H, D, lens, x, weights, y, y_drop, p, seed, gates, cst, ws, cell=0, aux=None, plan=None) -> None:
    d.T, d.B, d.I, d.H, d.D = T, B, I, H, D
    if plan is not None and plan.row_idx is not None:
        d.row_idx, d.n_rows = _addr(plan.row_idx), plan.n_rows
    d.cell = cell
    d.aux = _addr(aux)
    d.lens = _addr(lens)
    d.x = _addr(x)
    d.x_st, d.x_sb = B * I, I
    for k in range(D):
        w_ih, w_hh, b_ih, b_hh = weights[4 * k:4 * k + 4]
        d.w_ih[k], d.w_hh[k], d.b_ih[k], d.b_hh[k] = _addr(w_ih), _addr(w_hh), _addr(b_ih), _addr(b_hh)
    d.y = _addr(y)
    d.y_drop = _addr(y_drop)
    d.dropout_p = float(p)
    d.dropout_seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    d.gates = _addr(gates)
    d.cst = _addr(cst)
    d.workspace = _addr(ws)
    d.workspace_bytes = ws.numel()
    d.status = _addr(lstm_status_word(ws.device))


COMPUTE_PRECISIONS = {"fp32": PRECISION_FP32, "fp16": PRECISION_F16}


def check_compute_precision(p) -> str:
    if not isinstance(p, str) or p not in COMPUTE_PRECISIONS:
        raise ValueError(f"compute_precision must be one of {sorted(COMPUTE_PRECISIONS)}, got {p!r}")
    return p


class LstmStackFn(torch.autograd.Function):
    """x (T,B,I) time-major, lens (B) int32 on device -> y (T,B,D*H); zero rows for t >= lens[b].
    `cell`: 0 LSTM, 1 GRU, 2 tanh-RNN, 3 ReLU-RNN (the reference's supported_rnns, encoder.py:48-52).
    `want_final`: also return (h_n, c_n) — (L*D, B, H) states after each sequence's own last step, what torch's RNN modules
    return next to the output (decoder.py:115); not differentiable here (the reference never differentiates through them).
    Compute precision: an optional string "fp32" (default) | "fp16" in front of the weight tensors (autograd.Function.apply takes
    no keywords) selects rnnt_hip_lstm_fwd_ex / _bwd_ex's mode; the backward uses the mode its forward ran."""

    @staticmethod
    def forward(ctx, x, lens, hidden, num_layers, bidirectional, dropout_p, seed, cell, want_final, *weights):
        precision = "fp32"
        ctx.has_precision_arg = bool(weights) and isinstance(weights[0], str)
        if ctx.has_precision_arg:
            precision, weights = check_compute_precision(weights[0]), weights[1:]
        prec = COMPUTE_PRECISIONS[precision]
        plan = None
        if isinstance(lens, RaggedPlan):   # ragged batch with its valid-frame table: the big products and the recurrences skip padding
            plan, lens = lens, lens.lens
            if (plan.T, plan.B) != tuple(x.shape[:2]):
                raise ValueError(f"RaggedPlan was built for (T,B) = ({plan.T},{plan.B}), x is {tuple(x.shape)}")
            if plan.dense:
                plan = None
        _need_gpu(x, lens, *weights)
        if lens.dtype != torch.int32:
            raise ValueError(f"lengths must be int32 (dataloader.py:23-24), got {lens.dtype}")
        x = _f32c(x, "x")
        if x.dim() != 3 or lens.shape != (x.shape[1],):
            raise ValueError(f"x must be (T,B,I) with lens (B,): got {tuple(x.shape)} and {tuple(lens.shape)}")
        T, B, I0 = x.shape
        D = 2 if bidirectional else 1
        H = hidden
        # the kernels index raw pointers: every weight's shape is checked here, on the host, before anything is launched
        ngate = {0: 4, 1: 3, 2: 1, 3: 1}.get(cell)
        if ngate is None or not isinstance(want_final, bool):
            raise ValueError(f"cell must be 0..3 and want_final a bool (got cell={cell!r}, want_final={type(want_final).__name__})")
        if len(weights) != 4 * D * num_layers:
            raise ValueError(f"expected {4 * D * num_layers} weight tensors (w_ih, w_hh, b_ih, b_hh per layer and direction), got {len(weights)}")
        for i, w in enumerate(weights):
            layer, kind = i // (4 * D), i % 4
            I_l = I0 if layer == 0 else D * H
            want = [(ngate * H, I_l), (ngate * H, H), (ngate * H,), (ngate * H,)][kind]
            if not isinstance(w, torch.Tensor) or tuple(w.shape) != want:
                raise ValueError(f"lstm weight #{i} (layer {layer}, {['w_ih', 'w_hh', 'b_ih', 'b_hh'][kind]}): expected shape {want}, "
                                 f"got {tuple(w.shape) if isinstance(w, torch.Tensor) else type(w).__name__}")
        params = weights
        weights = [_f32c(w, "lstm weight") for w in weights]
        dev = x.device
        # one workspace for all layers: the larger of what the first (input width I0) and the inner layers (D*H) ask for
        ws = lstm_workspace(T, B, I0, H, D, dev)
        if num_layers > 1 and _lib.lib().rnnt_hip_lstm_workspace_bytes(T, B, D * H, H, D) > ws.numel():
            ws = lstm_workspace(T, B, D * H, H, D, dev)
        saved = []
        cur = x
        for layer in range(num_layers):
            I = cur.shape[-1]
            wl = weights[4 * D * layer:4 * D * (layer + 1)]
            gates = torch.empty(T, B, D * 4 * H, device=dev, dtype=torch.float32)
            cst = torch.empty(D * T * B * H, device=dev, dtype=torch.float32) if cell == 0 else None
            # (with a valid-frame table the recurrence leaves frames beyond a sync group's longest row untouched: they must read 0)
            y = (torch.zeros if plan is not None else torch.empty)(T, B, D * H, device=dev, dtype=torch.float32)
            p = dropout_p if layer < num_layers - 1 else 0.0
            y_drop = torch.empty_like(y) if p > 0 else None
            d = LstmDesc()
            _fill_lstm_desc(d, T, B, I, H, D, lens, cur, wl, y, y_drop, p, seed + layer, gates, cst, ws, cell, plan=plan)
            check(_lib.lib().rnnt_hip_lstm_fwd_ex(C.byref(d), prec, _stream()), "rnnt_hip_lstm_fwd_ex")
            saved.append((cur, y, gates, cst, p))
            cur = y_drop if p > 0 else y
        ctx.meta = (T, B, H, D, num_layers, seed, cell)
        ctx.prec = prec
        ctx.lens = lens
        ctx.plan = plan
        ctx.ws = ws
        ctx.saved = saved
        ctx.weights = weights
        ctx.params = params
        ctx.x_needs_grad = x.requires_grad
        if not want_final:
            return cur
        # final states: plumbing gathers from the stash (forward direction: frame lens-1, reverse direction: frame 0)
        last = (lens.long() - 1).clamp_(min=0)
        rows = torch.arange(B, device=dev)
        hs, cs = [], []
        for (_, y, _, cst, _) in saved:
            yv = y.view(T, B, D, H)
            cv = cst.view(D, T, H // 4, B, 4) if cst is not None else None
            for dd in range(D):
                tsel = last if dd == 0 else torch.zeros_like(last)
                hs.append(yv[tsel, rows, dd])
                if cv is not None:
                    cs.append(cv[dd, tsel, :, rows, :].reshape(B, H))
        h_n = torch.stack(hs)
        c_n = torch.stack(cs) if cs else torch.empty(0, device=dev)
        ctx.mark_non_differentiable(h_n, c_n)
        return cur, h_n, c_n

    @staticmethod
    def backward(ctx, dy, *_unused):
        T, B, H, D, L, seed, cell = ctx.meta
        prec = ctx.prec   # the forward's mode
        dy = _f32c(dy, "dy")
        weights = ctx.weights
        grads: List[Optional[torch.Tensor]] = [None] * len(weights)
        targets = [_direct_grad(p) for p in ctx.params]
        direct = all(t is not None for t in targets)  # all-or-nothing per stack: one accumulate flag per launch
        # Only dx is on the chain to the layer below: the weight / bias gradients of layer l (phase 2 of rnnt_hip_lstm_bwd) go to a
        # second stream and run beside the reverse-time recurrence of layer l-1 (phase 1), which leaves most of the chip idle.
        # Two workspaces alternate by layer parity so that phase 1 of layer l-1 never touches what phase 2 of layer l still reads.
        # Worth it only where the recurrence leaves XCDs free (c3: 4 of 8, +3.9 %): when its groups fill the chip (c2: 8 groups x 32
        # workgroups) the second stream's kernels merely queue behind it (+0.1..0.7 %, and every per-kernel timing turns into a
        # shared-device duration).  RNNT_LSTM_OVERLAP=1 forces it (tests), RNNT_LSTM_NO_OVERLAP=1 forbids it.
        overlap = L >= 2 and not os.environ.get("RNNT_LSTM_NO_OVERLAP") and (
            bool(os.environ.get("RNNT_LSTM_OVERLAP")) or _lib.lib().rnnt_hip_lstm_free_xcds(T, B, H, D, cell) >= 4)
        main = torch.cuda.current_stream()
        side = _side_stream(dy.device) if overlap else None
        wss = [ctx.ws, torch.empty_like(ctx.ws)] if overlap else [ctx.ws, ctx.ws]
        side_done: dict = {}
        keep = []   # tensors phase 2 reads or writes on the side stream: held until the streams have joined
        dx = None
        for layer in range(L - 1, -1, -1):
            x_l, y_l, gates, cst, p = ctx.saved[layer]
            I = x_l.shape[-1]
            wl = weights[4 * D * layer:4 * D * (layer + 1)]
            bd = LstmBwdDesc()
            aux = torch.empty_like(gates) if cell == 1 else None
            _fill_lstm_desc(bd.f, T, B, I, H, D, ctx.lens, x_l, wl, y_l, y_l if p > 0 else None, p, seed + layer, gates,
                            cst, wss[layer % 2], cell, aux, plan=ctx.plan)
            if layer > 0 and cell != 3:   # x of this layer is the (dropped) output of a bounded cell: |x| <= 1 / (1 - p) of the layer below
                bd.f.x_abs_bound = 1.0 / (1.0 - ctx.saved[layer - 1][4])
            bd.dy = _addr(dy)
            need_dx = layer > 0 or ctx.x_needs_grad
            dx = torch.empty(T, B, I, device=dy.device, dtype=torch.float32) if need_dx else None
            bd.dx = _addr(dx)
            bd.accumulate = 1 if direct else 0
            for k in range(D):
                base = 4 * D * layer + 4 * k
                if direct:  # += straight into the flat-gradient views; b_hh's view is the second destination of db
                    bd.dw_ih[k], bd.dw_hh[k] = _addr(targets[base]), _addr(targets[base + 1])
                    bd.db[k], bd.db_hh[k] = _addr(targets[base + 2]), _addr(targets[base + 3])
                    continue
                dw_ih = torch.empty_like(wl[4 * k])
                dw_hh = torch.empty_like(wl[4 * k + 1])
                db = torch.empty_like(wl[4 * k + 2])
                db_hh = torch.empty_like(db) if cell == 1 else db  # GRU: b_hn sits inside r * (.), its gradient differs
                bd.dw_ih[k], bd.dw_hh[k], bd.db[k] = _addr(dw_ih), _addr(dw_hh), _addr(db)
                bd.db_hh[k] = _addr(db_hh) if cell == 1 else None
                grads[base], grads[base + 1], grads[base + 2], grads[base + 3] = dw_ih, dw_hh, db, db_hh
            if not overlap:
                check(_lib.lib().rnnt_hip_lstm_bwd_ex(C.byref(bd), prec, main.cuda_stream), "rnnt_hip_lstm_bwd_ex")
                dy = dx
                continue
            if layer + 2 in side_done:   # this layer's workspace was last read by phase 2 of layer + 2
                main.wait_event(side_done[layer + 2])
            bd.phase = 1
            check(_lib.lib().rnnt_hip_lstm_bwd_ex(C.byref(bd), prec, main.cuda_stream), "rnnt_hip_lstm_bwd_ex (recurrence + dx)")
            side.wait_event(main.record_event())
            bd.phase, bd.beside_recurrence = 2, 1 if layer > 0 else 0
            check(_lib.lib().rnnt_hip_lstm_bwd_ex(C.byref(bd), prec, side.cuda_stream), "rnnt_hip_lstm_bwd_ex (weight gradients)")
            side_done[layer] = side.record_event()
            keep.append((aux, dy, dx))
            dy = dx
        if overlap:
            main.wait_stream(side)   # everything below (autograd's accumulation, the optimizer, frees) is ordered after phase 2
        del keep
        ctx.saved = None  # release the stash
        return (dx if ctx.x_needs_grad else None, None, None, None, None, None, None, None, None,
                *((None,) if ctx.has_precision_arg else ()), *grads)


_SIDE_STREAMS: dict = {}


def _side_stream(device) -> "torch.cuda.Stream":
    """One extra stream per device for work that overlaps the persistent recurrences (created once, reused)."""
    key = torch.device(device).index if torch.device(device).index is not None else torch.cuda.current_device()
    if key not in _SIDE_STREAMS:
        _SIDE_STREAMS[key] = torch.cuda.Stream(device=key)
    return _SIDE_STREAMS[key]


def lstm_check(ws: torch.Tensor) -> None:
    """C-ABI diagnostic for callers that pass status = NULL (the workspace's own per-launch word); the package itself uses
    the sticky device word: see lstm_status_check()."""
    check(_lib.lib().rnnt_hip_lstm_check(_addr(ws), _stream()), "rnnt_hip_lstm_check")


_MANGLED_INSTANCE = re.compile(r"\d(lstm_\w+?)_kernelI((?:L[bi]n?\d+E)+)E")
_PLAIN_INSTANCE = re.compile(r"\b(lstm_\w+?)_kernel<([^<>]*)>")


def recurrence_instance(symbol: str) -> str:
    """The instance a recurrence kernel's device symbol names, mangled or demangled, as 'lstm_fwd5<3,0,8,5,0>' (kernel name without
    '_kernel', template arguments in order, bools as 0 / 1)."""
    m = _MANGLED_INSTANCE.search(symbol)
    if m:
        args = [("-" if neg else "") + v for _, neg, v in re.findall(r"L([bi])(n?)(\d+)E", m.group(2))]
    else:
        m = _PLAIN_INSTANCE.search(symbol)
        if not m:
            raise ValueError(f"not a recurrence kernel symbol: {symbol!r}")
        args = [{"true": "1", "false": "0"}.get(a.strip(), a.strip()) for a in m.group(2).split(",")]
    return f"{m.group(1)}<{','.join(args)}>"


class lstm_launch_record:
    """Records the recurrence kernels launched inside the `with` block (rnnt_hip_lstm_launch_log_enable): afterwards `symbols` holds
    their device symbols and `instances` the instances they name (recurrence_instance), in launch order."""

    def __enter__(self):
        check(_lib.lib().rnnt_hip_lstm_launch_log_enable(1), "rnnt_hip_lstm_launch_log_enable")
        self.symbols: List[str] = []
        self.instances: List[str] = []
        return self

    def __exit__(self, *exc):
        L = _lib.lib()
        check(L.rnnt_hip_lstm_launch_log_enable(0), "rnnt_hip_lstm_launch_log_enable")
        n = L.rnnt_hip_lstm_launch_log(None, 0)
        buf = C.create_string_buffer(n + 1)
        L.rnnt_hip_lstm_launch_log(buf, n + 1)
        self.symbols = buf.value.decode().splitlines()
        self.instances = [recurrence_instance(s) for s in self.symbols]
        return False


# --------------------------------------------------------------------------------------------------
# fused joint + RNN-T loss  (replaces transducer.py:54-69 + model.py:39,57)
# --------------------------------------------------------------------------------------------------
def _joint_ac(enc, dec, W, Oe, Od, V):
    """A (T,B,V) = gelu(enc) W[:, :Oe]^T ; C (U1,Bd,V) = gelu(dec) W[:, Oe:]^T  (two small GEMMs, GELU on load)."""
    T, B = enc.shape[:2]
    U1, Bd = dec.shape[:2]   # Bd = B, or B * group label rows (JointLossGroupedFn)
    A = torch.empty(T, B, V, device=enc.device, dtype=torch.float32)
    Cm = torch.empty(U1, Bd, V, device=enc.device, dtype=torch.float32)
    gemm(T * B, V, Oe, enc, W, A, b_sn=Oe + Od, b_sk=1, flags=GEMM_GELU_A)
    gemm(U1 * Bd, V, Od, dec, W, Cm, b_off=Oe, b_sn=Oe + Od, b_sk=1, flags=GEMM_GELU_A)
    return A, Cm


def _joint_backward(enc, dec, W, dA, dC, needs, w_tgt=None, b_tgt=None, db_from_c=False):
    """d_enc, d_dec, dW, db from dA (T,B,V), dC (U1,B,V).  w_tgt / b_tgt: flat-gradient views to add into (then None is
    returned for that gradient).  dec and dC may hold more rows than enc (JointLossGroupedFn: a group of label rows per
    encoder row, dA already summed over the group).
    db_from_c: db = the column sums of dC instead of dA's.  z = A + C + bias, so the lattice's dA and dC have the same column sums;
    a dC that also carries the internal-LM term (whose logits are C + bias) therefore holds the whole bias gradient.
    enc = dA = None (IlmLossFn, with db_from_c): the decoder half alone; a fresh dW then has exact zeros in its encoder columns."""
    U1, Bd, Od = dec.shape
    V, O = W.shape
    Oe = O - Od
    d_enc = d_dec = dW = db = None
    if needs[0]:
        T, B = enc.shape[:2]
        d_enc = torch.empty_like(enc)
        gemm(T * B, Oe, V, dA, W, d_enc, b_sn=1, b_sk=O, aux=enc, flags=GEMM_MUL_DGELU)
    if needs[1]:
        d_dec = torch.empty_like(dec)
        gemm(U1 * Bd, Od, V, dC, W, d_dec, b_off=Oe, b_sn=1, b_sk=O, aux=dec, flags=GEMM_MUL_DGELU)
    if needs[2]:
        dW = (torch.empty_like(W) if enc is not None else torch.zeros_like(W)) if w_tgt is None else None
        out = dW if w_tgt is None else w_tgt
        fl = GEMM_GELU_B | (0 if w_tgt is None else GEMM_ACCUM)
        if enc is not None:
            T, B = enc.shape[:2]
            gemm(V, Oe, T * B, dA, enc, out, a_mc=True, a_sk=V, b_sn=1, b_sk=Oe, c_div=1, c_so=O, c_si=0, flags=fl, split_k=True)
        gemm(V, Od, U1 * Bd, dC, dec, out, a_mc=True, a_sk=V, b_sn=1, b_sk=Od, c_off=Oe, c_div=1, c_so=O, c_si=0, flags=fl,
             split_k=True)
    if needs[3]:
        db = colsum(dC, U1 * Bd, V, into=b_tgt) if db_from_c else colsum(dA, enc.shape[0] * enc.shape[1], V, into=b_tgt)
    return d_enc, d_dec, dW, db


def check_fastemit_lambda(fastemit_lambda) -> float:
    """FastEmit's weight (include/rnnt_hip.h): a finite number >= 0, as the library itself requires."""
    lam = float(fastemit_lambda)
    if not (math.isfinite(lam) and lam >= 0.0):
        raise ValueError(f"fastemit_lambda must be finite and >= 0, got {fastemit_lambda!r}")
    return lam


def check_ilmt_weight(ilmt_weight) -> float:
    """The weight of the internal-LM training term (ILMT; include/rnnt_hip.h): a finite number >= 0."""
    if isinstance(ilmt_weight, bool) or not isinstance(ilmt_weight, (int, float)):
        raise ValueError(f"ilmt_weight must be a number, finite and >= 0, got {ilmt_weight!r}")
    w = float(ilmt_weight)
    if not (math.isfinite(w) and w >= 0.0):
        raise ValueError(f"ilmt_weight must be finite and >= 0, got {ilmt_weight!r}")
    return w


def check_kd_weight(kd_weight) -> float:
    """The weight of the lattice distillation term (KD; include/rnnt_hip.h): a finite number >= 0."""
    if isinstance(kd_weight, bool) or not isinstance(kd_weight, (int, float)):
        raise ValueError(f"kd_weight must be a number, finite and >= 0, got {kd_weight!r}")
    w = float(kd_weight)
    if not (math.isfinite(w) and w >= 0.0):
        raise ValueError(f"kd_weight must be finite and >= 0, got {kd_weight!r}")
    return w


class CellLogProbs(NamedTuple):
    """A model's collapsed per-cell log-probabilities over a batch's lattices (include/rnnt_hip.h, lattice distillation): three
    (B, U+1, T) fp32 planes, plane[b, u, t] -- log p(blank), log p(y_u), and log of everything else (every non-blank entry where the
    row has no label left).  What a teacher hands to a student's loss (`kd_teacher=`)."""
    blk: torch.Tensor
    emit: torch.Tensor
    rest: torch.Tensor


def check_kd_teacher(kd_teacher, B: int, U1: int, T: int, V: int, device, emit_windows=None):
    """The `kd_teacher` argument of the losses: None, or a CellLogProbs of three (B, U1, T) float32 tensors on `device` (made
    contiguous here).  ValueError for anything else, for V < 3 (the third class would be empty) and for emission windows next to a
    teacher, before anything runs."""
    if kd_teacher is None:
        return None
    if not isinstance(kd_teacher, (tuple, list)) or len(kd_teacher) != 3:
        raise ValueError(f"kd_teacher must be None or a CellLogProbs (blk, emit, rest), got {type(kd_teacher).__name__}")
    if emit_windows is not None:
        raise ValueError("kd_teacher does not combine with emit_windows: the distillation term has no windowed form")
    if V < 3:
        raise ValueError(f"kd_teacher needs a vocabulary of at least 3 entries (blank, label, rest), got V = {V}")
    out = []
    for name, t in zip(("kd_teacher.blk", "kd_teacher.emit", "kd_teacher.rest"), kd_teacher):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a tensor, got {type(t).__name__}")
        if t.dtype != torch.float32:
            raise ValueError(f"{name} must be float32, got {t.dtype}")
        if tuple(t.shape) != (B, U1, T):
            raise ValueError(f"{name} must be (B, U+1, T) = ({B}, {U1}, {T}), got {tuple(t.shape)}")
        if t.device != torch.device(device):
            raise ValueError(f"{name} must be on {device}, got {t.device}")
        out.append(t.detach().contiguous())
    return CellLogProbs(*out)


def _ilm_forward(Cm, bias, labels, u_lens, blank: int, keep_lse: bool):
    """The internal LM's per-utterance NLL (B,) on Cm (U1,B,V) time-major, and the rows' lse (U1*B) for the backward (or None).
    (B, 0) labels have no storage to point at: u_lens stands in for them, and is never read as labels (every length clamps to 0)."""
    U1, B, V = Cm.shape
    labels = labels if labels.numel() else u_lens
    ilm = torch.empty(B, device=Cm.device, dtype=torch.float32)
    lse = torch.empty(U1 * B, device=Cm.device, dtype=torch.float32) if keep_lse else None
    check(_lib.lib().rnnt_hip_ilm_loss_fwd(_addr(Cm), V, B * V, _addr(bias), _addr(labels), _addr(u_lens), B, U1, V, int(blank),
                                           _addr(ilm), _addr(lse), _stream()), "rnnt_hip_ilm_loss_fwd")
    return ilm, lse


def _ilm_backward(Cm, bias, labels, u_lens, lse, blank: int, g, red_scale, accumulate: bool, dC) -> None:
    """dC (+)= the internal-LM term's gradient under the upstream gradient g ((B,), or 0-d with the reduction's red_scale)."""
    U1, B, V = Cm.shape
    labels = labels if labels.numel() else u_lens
    gvec = _f32c(g.to(torch.float32), "grad of the internal-LM loss")
    scalar = red_scale is not None
    check(_lib.lib().rnnt_hip_ilm_loss_bwd(_addr(Cm), V, B * V, _addr(bias), _addr(labels), _addr(u_lens), _addr(lse), B, U1, V,
                                           int(blank), red_scale if scalar else 1.0, _addr(gvec), 0 if scalar else 1,
                                           1 if accumulate else 0, _addr(dC), _stream()), "rnnt_hip_ilm_loss_bwd")


def _reduce_loss(nll, red_scale):
    """The (B,) losses themselves (red_scale None) or red_scale * their sum, 0-d, inside the library."""
    if red_scale is None:
        return nll
    out = torch.empty((), device=nll.device, dtype=torch.float32)
    check(_lib.lib().rnnt_hip_scaled_sum_f32(_addr(nll), nll.numel(), red_scale, _addr(out), _stream()), "rnnt_hip_scaled_sum_f32")
    return out


def check_emit_windows(emit_windows, B: int, U: int, device):
    """Emission windows of the alignment-restricted loss (include/rnnt_hip.h): None, or a pair (lo, hi) of (B, U) int32 tensors on
    `device`.  -> None, or (lo, hi, row stride) as the library takes them (contiguous; one column of padding when U = 0, so that the
    pointers are not null).  ValueError for anything else, before anything runs."""
    if emit_windows is None:
        return None
    if not isinstance(emit_windows, (tuple, list)) or len(emit_windows) != 2:
        raise ValueError(f"emit_windows must be None or a pair (lo, hi) of (B, U) int32 tensors, got {type(emit_windows).__name__}")
    out = []
    for name, t in zip(("emit_windows lo", "emit_windows hi"), emit_windows):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a tensor, got {type(t).__name__}")
        if t.dtype != torch.int32:
            raise ValueError(f"{name} must be int32, got {t.dtype}")
        if tuple(t.shape) != (B, U):
            raise ValueError(f"{name} must be (B, U) = ({B}, {U}), got {tuple(t.shape)}")
        if t.device != torch.device(device):
            raise ValueError(f"{name} must be on {device}, got {t.device}")
        out.append(t.contiguous() if U > 0 else torch.zeros(B, 1, dtype=torch.int32, device=t.device))
    return out[0], out[1], max(U, 1)


def emit_windows(frames, t_lens, u_lens, left: int, right: int):
    """(lo, hi) = (frames - left, frames + right), int32, for the `emit_windows` argument of the losses: label u of row b may be
    emitted at most `left` frames before and `right` frames after its reference frame frames[b, u].  `frames`: a (B, U) integer table
    such as align().frames (entries past u_lens[b] are not read by the loss; -1 there is fine).  The loss itself clamps the windows to
    [0, t_lens[b] - 1]; t_lens / u_lens are only checked against the table's batch size here.  Plain torch ops: not a hot path."""
    for name, v in (("left", left), ("right", right)):
        if isinstance(v, bool) or not isinstance(v, int) or v < 0:
            raise ValueError(f"emit_windows: {name} must be an integer >= 0, got {v!r}")
    if not isinstance(frames, torch.Tensor) or frames.dim() != 2 or frames.is_floating_point() or frames.dtype == torch.bool:
        raise ValueError("emit_windows: frames must be a (B, U) integer tensor")
    for name, t in (("t_lens", t_lens), ("u_lens", u_lens)):
        n = len(t) if isinstance(t, (list, tuple)) else (t.numel() if isinstance(t, torch.Tensor) else None)
        if n != frames.shape[0]:
            raise ValueError(f"emit_windows: {name} must hold one length per row of frames ({frames.shape[0]})")
    fr = frames.to(torch.int32)
    return fr - left, fr + right


_LOGITS_DTYPE_CODE = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}   # RNNT_DTYPE_* of include/rnnt_hip.h


def _logits_dtype_code(logits: torch.Tensor) -> int:
    if logits.dtype not in _LOGITS_DTYPE_CODE:
        raise ValueError(f"logits must be float32, float16 or bfloat16, got {logits.dtype}")
    return _LOGITS_DTYPE_CODE[logits.dtype]


def _i32(named, note: str = "") -> None:
    """ValueError unless every tensor of the (name, tensor) pairs is int32."""
    for name, t in named:
        if t.dtype != torch.int32:
            raise ValueError(f"{name} must be int32{note}, got {t.dtype}")


def _loss_forward(entry: str, operands, B: int, T: int, U1: int, V: int, blank: int, win, lam: float, grads, device):
    """One call of the library's loss with its workspace: the query, the allocation, the call.  entry + operands: the separable
    "rnnt_hip_joint_loss_fwd_bwd" with _sep_operands(...), or the dense "rnnt_hip_loss_from_logits_fwd_bwd" with (logits, dtype
    code, labels, t_lens, u_lens) -- its _fastemit form, or with win (check_emit_windows' triple, not None) its _window form and
    the larger workspace.  grads: the entry's gradient pointers -- (None, None) for the separable forward, whose backward is
    _sep_loss_backward on the workspace; (d/d logits or None,) for the dense one.  -> (nll (B,), workspace)."""
    L = _lib.lib()
    name = entry + ("_fastemit" if win is None else "_window")
    nws = (L.rnnt_hip_joint_loss_workspace_bytes if win is None else L.rnnt_hip_joint_loss_window_workspace_bytes)(B, T, U1, V)
    ws = torch.empty(nws, device=device, dtype=torch.uint8)
    nll = torch.empty(B, device=device, dtype=torch.float32)
    windows = () if win is None else (_addr(win[0]), _addr(win[1]), win[2])
    check(getattr(L, name)(*operands, B, T, U1, V, int(blank), 1.0, lam, *windows, _addr(nll), *grads, _addr(ws), nws, _stream()), name)
    return nll, ws


def _sep_loss_forward(A, Cm, bias, labels, t_lens, u_lens, blank: int, win, lam: float):
    """Forward of the separable loss on A (T,B,V), Cm (U1,B,V) time-major, without gradients -> (nll (B,), workspace)."""
    (T, B, V), U1 = A.shape, Cm.shape[0]
    return _loss_forward("rnnt_hip_joint_loss_fwd_bwd", _sep_operands(A, Cm, bias, labels, t_lens, u_lens), B, T, U1, V, blank, win, lam,
                         (None, None), A.device)


def _sep_operands(A, Cm, bias, labels, t_lens, u_lens):
    """The separable operand block of the library's loss entries for A (T,B,V), Cm (U1,B,V) time-major."""
    B, V = A.shape[1:]
    return (_addr(A), V, B * V, _addr(Cm), V, B * V, _addr(bias), _addr(labels), _addr(t_lens), _addr(u_lens))


def _sep_loss_backward(A, Cm, bias, labels, t_lens, u_lens, blank: int, windowed: bool, lam: float, gscale: float, gvec, gvec_stride: int,
                       ws):
    """dA, dC of the loss whose forward (_loss_forward on the same operands) left `ws`, under the upstream gradient gvec."""
    (T, B, V), U1 = A.shape, Cm.shape[0]
    dA, dC = torch.empty_like(A), torch.empty_like(Cm)
    name = "rnnt_hip_joint_loss_bwd_window" if windowed else "rnnt_hip_joint_loss_bwd_fastemit"
    check(getattr(_lib.lib(), name)(*_sep_operands(A, Cm, bias, labels, t_lens, u_lens), B, T, U1, V, blank, gscale, lam, _addr(gvec),
                                    gvec_stride, _addr(dA), _addr(dC), _addr(ws), ws.numel(), _stream()), name)
    return dA, dC


def _sep_loss_forward_kd(A, Cm, bias, labels, t_lens, u_lens, blank: int, lam: float, teacher):
    """_sep_loss_forward with a teacher's planes: -> (nll (B,), kd (B,), workspace), the workspace with the student's third plane."""
    (T, B, V), U1 = A.shape, Cm.shape[0]
    L = _lib.lib()
    nws = L.rnnt_hip_joint_loss_kd_workspace_bytes(B, T, U1, V)
    ws = torch.empty(nws, device=A.device, dtype=torch.uint8)
    nll, kd = torch.empty(B, device=A.device, dtype=torch.float32), torch.empty(B, device=A.device, dtype=torch.float32)
    check(L.rnnt_hip_joint_loss_fwd_bwd_kd(*_sep_operands(A, Cm, bias, labels, t_lens, u_lens), B, T, U1, V, int(blank), 1.0, lam,
                                           _addr(teacher.blk), _addr(teacher.emit), _addr(teacher.rest), 1.0, _addr(nll), _addr(kd), None,
                                           None, _addr(ws), nws, _stream()), "rnnt_hip_joint_loss_fwd_bwd_kd")
    return nll, kd, ws


def _sep_loss_backward_kd(A, Cm, bias, labels, t_lens, u_lens, blank: int, lam: float, gscale: float, gvec, kvec, stride: int, teacher, ws):
    """dA, dC of nll and kd together (_sep_loss_forward_kd left `ws`) under their upstream gradients gvec and kvec."""
    (T, B, V), U1 = A.shape, Cm.shape[0]
    dA, dC = torch.empty_like(A), torch.empty_like(Cm)
    check(_lib.lib().rnnt_hip_joint_loss_bwd_kd(*_sep_operands(A, Cm, bias, labels, t_lens, u_lens), B, T, U1, V, blank, gscale, lam,
                                                _addr(gvec), stride, _addr(teacher.blk), _addr(teacher.emit), _addr(teacher.rest), gscale,
                                                _addr(kvec), stride, _addr(dA), _addr(dC), _addr(ws), ws.numel(), _stream()),
          "rnnt_hip_joint_loss_bwd_kd")
    return dA, dC


def joint_cell_logprobs(enc, dec, W, bias, labels, t_lens, u_lens, blank: int) -> CellLogProbs:
    """The teacher's side of lattice distillation: enc (T,B,Oe), dec (U1,B,Od) time-major, fc.weight, fc.bias, labels (B,U) int32 and
    the int32 lengths, as JointLossFn takes them -> CellLogProbs of three (B, U1, T) fp32 planes.  The joint's two pre-GEMMs and one
    launch; no lattice sweep, no graph (the result never requires grad)."""
    _need_gpu(enc, dec, W, bias, labels, t_lens, u_lens)
    with torch.no_grad():
        enc, dec, W, bias = _f32c(enc, "enc"), _f32c(dec, "dec"), _f32c(W, "fc.weight"), _f32c(bias, "fc.bias")
        _i32((("targets", labels), ("frame lengths", t_lens), ("target lengths", u_lens)), " (dataloader.py:21-24)")
        labels = labels.contiguous()
        T, B, Oe = enc.shape
        U1, B2, Od = dec.shape
        V = W.shape[0]
        if B2 != B or W.shape[1] != Oe + Od or labels.shape != (B, U1 - 1):
            raise ValueError(f"shape mismatch: enc {tuple(enc.shape)} dec {tuple(dec.shape)} fc {tuple(W.shape)} "
                             f"targets {tuple(labels.shape)}")
        if V < 3:
            raise ValueError(f"joint_cell_logprobs needs a vocabulary of at least 3 entries (blank, label, rest), got V = {V}")
        A, Cm = _joint_ac(enc, dec, W, Oe, Od, V)
        out = CellLogProbs(*(torch.empty(B, U1, T, device=enc.device, dtype=torch.float32) for _ in range(3)))
        check(_lib.lib().rnnt_hip_joint_cell_logprobs(*_sep_operands(A, Cm, bias, labels, t_lens, u_lens), B, T, U1, V, int(blank),
                                                      _addr(out.blk), _addr(out.emit), _addr(out.rest), _stream()),
              "rnnt_hip_joint_cell_logprobs")
    return out


class JointLossFn(torch.autograd.Function):
    """enc (T,B,Oe), dec (U1,B,Od) time-major -> per-utterance NLL (B,).  Never builds (B,T,U1,V).
    forward: A/C pre-GEMMs + log-softmax terms + alpha/beta (kept in a workspace); backward: the lattice gradient kernel with
    the upstream per-utterance gradient folded in (1/B under reduction="mean", model.py:39), then the joint's own backward.
    Under torch.no_grad() (validation_step) no gradient kernel runs and nothing is kept.
    fastemit_lambda > 0: FastEmit regularisation of the GRADIENT (label log-probability gradients scaled by 1 + lambda, through the
    log-softmax exactly; include/rnnt_hip.h).  The returned loss stays the unregularised NLL, bit for bit that of lambda = 0.
    emit_windows = (lo, hi), two (B,U) int32 tensors: the alignment-restricted loss (label u only at frames lo[b,u] .. hi[b,u]; an
    infeasible row has NLL +inf and a zero gradient; include/rnnt_hip.h).  None: the unrestricted loss, the entries without windows.
    ilmt_weight > 0 (internal-LM training; csrc/ilm_loss.hip): the function returns (nll, ilm_nll), the second the internal LM's NLL
    of the labels under the same reduction, from one more launch on the C tensor the loss already holds.  The weight itself is the
    caller's to apply: the upstream gradient of ilm_nll reaches the gradient kernel, which adds the term into the lattice's dC (one
    launch); fc.bias's gradient is then the column sums of that dC.  At 0: one output, the launches and bits of a call without it.
    (Lattice distillation is JointLossKdFn below: this function's arguments plus a teacher's planes.  Both run _joint_loss_forward /
    _joint_loss_backward.)"""

    @staticmethod
    def forward(ctx, enc, dec, W, bias, labels, t_lens, u_lens, blank, want_grad=True, reduction="none", fastemit_lambda=0.0,
                emit_windows=None, ilmt_weight=0.0):
        return _joint_loss_forward(ctx, enc, dec, W, bias, labels, t_lens, u_lens, blank, want_grad, reduction, fastemit_lambda,
                                   emit_windows, ilmt_weight, None, 0.0)

    @staticmethod
    def backward(ctx, g, *g_more):
        return _joint_loss_backward(ctx, g, *g_more) + (None,) * 9


class JointLossKdFn(torch.autograd.Function):
    """JointLossFn with lattice knowledge distillation: the same arguments, then kd_teacher (a CellLogProbs from a
    teacher on the same batch, or None) and kd_weight.  With a teacher and kd_weight > 0 the function returns one more value, LAST:
    kd, the collapsed KL between the teacher's and the student's cells per utterance, under the same reduction.  The weight is the
    caller's to apply; the upstream gradients of nll and kd both reach the KD instances of the lattice gradient kernels (either may be
    0).  Not with emit_windows.  Without a teacher or at weight 0 nothing of it runs: the outputs, launches and bits of JointLossFn."""

    @staticmethod
    def forward(ctx, enc, dec, W, bias, labels, t_lens, u_lens, blank, want_grad=True, reduction="none", fastemit_lambda=0.0,
                emit_windows=None, ilmt_weight=0.0, kd_teacher=None, kd_weight=0.0):
        return _joint_loss_forward(ctx, enc, dec, W, bias, labels, t_lens, u_lens, blank, want_grad, reduction, fastemit_lambda,
                                   emit_windows, ilmt_weight, kd_teacher, kd_weight)

    @staticmethod
    def backward(ctx, g, *g_more):
        return _joint_loss_backward(ctx, g, *g_more) + (None,) * 11


# the shared body of the two functions above
def _joint_loss_forward(ctx, enc, dec, W, bias, labels, t_lens, u_lens, blank, want_grad, reduction, fastemit_lambda, emit_windows,
                        ilmt_weight, kd_teacher, kd_weight):
    _need_gpu(enc, dec, W, bias, labels, t_lens, u_lens)
    ctx.fastemit_lambda = check_fastemit_lambda(fastemit_lambda)
    ctx.ilmt = check_ilmt_weight(ilmt_weight) > 0.0
    teacher = check_kd_teacher(kd_teacher, enc.shape[1], dec.shape[0], enc.shape[0], W.shape[0], enc.device, emit_windows)
    ctx.kd = check_kd_weight(kd_weight) > 0.0 and teacher is not None
    win = check_emit_windows(emit_windows, enc.shape[1], dec.shape[0] - 1, enc.device)
    w_param, b_param = W, bias
    enc, dec, W, bias = _f32c(enc, "enc"), _f32c(dec, "dec"), _f32c(W, "fc.weight"), _f32c(bias, "fc.bias")
    _i32((("targets", labels), ("frame lengths", t_lens), ("target lengths", u_lens)), " (dataloader.py:21-24)")
    labels = labels.contiguous()
    T, B, Oe = enc.shape
    U1, B2, Od = dec.shape
    V = W.shape[0]
    if B2 != B or W.shape[1] != Oe + Od or labels.shape != (B, U1 - 1):
        raise ValueError(f"shape mismatch: enc {tuple(enc.shape)} dec {tuple(dec.shape)} fc {tuple(W.shape)} "
                         f"targets {tuple(labels.shape)}")
    A, Cm = _joint_ac(enc, dec, W, Oe, Od, V)
    kd = None
    if ctx.kd:
        nll, kd, ws = _sep_loss_forward_kd(A, Cm, bias, labels, t_lens, u_lens, blank, ctx.fastemit_lambda, teacher)
    else:
        nll, ws = _sep_loss_forward(A, Cm, bias, labels, t_lens, u_lens, blank, win, ctx.fastemit_lambda)
    ctx.windowed = win is not None   # the backward reads the band tables the forward left in the workspace
    keep = want_grad and any(ctx.needs_input_grad[:4])  # want_grad: the caller's torch.is_grad_enabled() (always off in here)
    ilm, lse = _ilm_forward(Cm, bias, labels, u_lens, blank, keep) if ctx.ilmt else (None, None)
    if keep:
        ctx.save_for_backward(enc, dec, W, bias, labels, t_lens, u_lens, A, Cm, ws, *((lse,) if ctx.ilmt else ()),
                              *(teacher if ctx.kd else ()))
        ctx.blank = int(blank)
        ctx.w_param, ctx.b_param = w_param, b_param
    ctx.red_scale = {"none": None, "sum": 1.0, "mean": 1.0 / B}[reduction]
    if ctx.ilmt or ctx.kd:
        return tuple(_reduce_loss(x, ctx.red_scale) for x in (nll, ilm, kd) if x is not None)
    return _reduce_loss(nll, ctx.red_scale)   # reduction inside the library: no torch arithmetic on the path

def _joint_loss_backward(ctx, g, *g_more):
    """-> (d_enc, d_dec, dW, db)"""
    enc, dec, W, bias, labels, t_lens, u_lens, A, Cm, ws = ctx.saved_tensors[:10]
    gvec = _f32c(g.to(torch.float32), "grad of the loss")
    scalar = ctx.red_scale is not None   # reduced loss: ONE upstream scalar, the 1/B of "mean" rides in gscale
    if ctx.kd:   # both upstream gradients, of nll and of kd (the last output), in one pass of the KD gradient instances
        kvec = _f32c(g_more[-1].to(torch.float32), "grad of the distillation term")
        dA, dC = _sep_loss_backward_kd(A, Cm, bias, labels, t_lens, u_lens, ctx.blank, ctx.fastemit_lambda,
                                       ctx.red_scale if scalar else 1.0, gvec, kvec, 0 if scalar else 1,
                                       CellLogProbs(*ctx.saved_tensors[-3:]), ws)
    else:
        dA, dC = _sep_loss_backward(A, Cm, bias, labels, t_lens, u_lens, ctx.blank, ctx.windowed, ctx.fastemit_lambda,
                                    ctx.red_scale if scalar else 1.0, gvec, 0 if scalar else 1, ws)
    if ctx.ilmt:   # the internal-LM term's gradient lands in the dC the lattice kernel has just written; db then comes from dC
        _ilm_backward(Cm, bias, labels, u_lens, ctx.saved_tensors[10], ctx.blank, g_more[0], ctx.red_scale, True, dC)
    d_enc, d_dec, dW, db = _joint_backward(enc, dec, W, dA, dC, ctx.needs_input_grad[:4],
                                           _direct_grad(ctx.w_param), _direct_grad(ctx.b_param), db_from_c=ctx.ilmt)
    return d_enc, d_dec, dW, db


class JointLossGroupedFn(torch.autograd.Function):
    """JointLossFn for B*group label rows over B encoder rows (MWER training: the `group` hypotheses of utterance b, rows
    b*group .. b*group + group - 1 of dec / labels / t_lens / u_lens, share encoder row b): enc (T,B,Oe), dec (U1,B*group,Od) ->
    per-row NLL (B*group,), the bits JointLossFn gives on enc.repeat_interleave(group, dim=1).
    A = gelu(enc) W_e^T is computed ONCE as (T,B,V) and expanded to (T,B*group,V) by a gather for the unchanged loss kernels; the
    backward adds dA over the group in rank order (a fixed order: bitwise reproducible) before the joint's own backward, so the
    encoder-side GEMMs run once per step, not `group` times.  reduction "none" only, and no FastEmit: the rows are hypotheses.
    No emission windows either (JointLossFn's emit_windows): a hypothesis has no reference alignment to build them from."""

    @staticmethod
    def forward(ctx, enc, dec, W, bias, labels, t_lens, u_lens, blank, group, want_grad=True):
        if isinstance(group, bool) or not isinstance(group, int) or group < 1:
            raise ValueError(f"group must be a positive integer, got {group!r}")
        _need_gpu(enc, dec, W, bias, labels, t_lens, u_lens)
        w_param, b_param = W, bias
        enc, dec, W, bias = _f32c(enc, "enc"), _f32c(dec, "dec"), _f32c(W, "fc.weight"), _f32c(bias, "fc.bias")
        _i32((("targets", labels), ("frame lengths", t_lens), ("target lengths", u_lens)), " (dataloader.py:21-24)")
        labels = labels.contiguous()
        T, B, Oe = enc.shape
        U1, R, Od = dec.shape
        V = W.shape[0]
        if R != B * group or W.shape[1] != Oe + Od or labels.shape != (R, U1 - 1) or t_lens.shape != (R,) or u_lens.shape != (R,):
            raise ValueError(f"shape mismatch: enc {tuple(enc.shape)} dec {tuple(dec.shape)} fc {tuple(W.shape)} targets "
                             f"{tuple(labels.shape)} lengths {tuple(t_lens.shape)} / {tuple(u_lens.shape)} for group = {group}")
        A, Cm = _joint_ac(enc, dec, W, Oe, Od, V)
        rows = torch.arange(R, device=enc.device, dtype=torch.int64) // group
        Ax = A.index_select(1, rows)   # (T, B*group, V): the gather
        del A
        nll, ws = _sep_loss_forward(Ax, Cm, bias, labels, t_lens, u_lens, blank, None, 0.0)
        if want_grad and any(ctx.needs_input_grad[:4]):
            ctx.save_for_backward(enc, dec, W, bias, labels, t_lens, u_lens, Ax, Cm, ws)
            ctx.blank, ctx.group = int(blank), group
            ctx.w_param, ctx.b_param = w_param, b_param
        return nll

    @staticmethod
    def backward(ctx, g):
        enc, dec, W, bias, labels, t_lens, u_lens, Ax, Cm, ws = ctx.saved_tensors
        T, B, _ = enc.shape
        V, G = W.shape[0], ctx.group
        gvec = _f32c(g.to(torch.float32), "grad of the loss")
        dAx, dC = _sep_loss_backward(Ax, Cm, bias, labels, t_lens, u_lens, ctx.blank, False, 0.0, 1.0, gvec, 1, ws)
        dAg = dAx.view(T, B, G, V)
        dA = dAg[:, :, 0].contiguous()
        for n in range(1, G):   # rank order, one addition per rank: the same bits on every run
            dA.add_(dAg[:, :, n])
        d_enc, d_dec, dW, db = _joint_backward(enc, dec, W, dA, dC, ctx.needs_input_grad[:4],
                                               _direct_grad(ctx.w_param), _direct_grad(ctx.b_param))
        return d_enc, d_dec, dW, db, None, None, None, None, None, None


class IlmLossFn(torch.autograd.Function):
    """The internal-LM loss alone, on text (text-only internal-LM adaptation; include/rnnt_hip.h, csrc/ilm_loss.hip): dec (U1,B,Od)
    time-major, fc.weight (V, Oe + Od), fc.bias -> per-utterance NLL (B,) of the internal LM on labels (B,U) int32, or its "sum" /
    "mean" over the batch (0-d).  No encoder operand: the decoder half of the joint's pre-GEMM alone, the forward kernel, and in the
    backward the gradient kernel (accumulate = 0) and the decoder half of the joint's own backward.  fc.weight's encoder columns get
    exact zeros (nothing is added to them in a flat-gradient view).  Under torch.no_grad() nothing is kept."""

    @staticmethod
    def forward(ctx, dec, W, bias, labels, u_lens, blank, want_grad=True, reduction="none"):
        _need_gpu(dec, W, bias, labels, u_lens)
        w_param, b_param = W, bias
        dec, W, bias = _f32c(dec, "dec"), _f32c(W, "fc.weight"), _f32c(bias, "fc.bias")
        _i32((("targets", labels), ("target lengths", u_lens)), " (dataloader.py:21-24)")
        if reduction not in ("none", "sum", "mean"):
            raise ValueError(f"reduction must be mean|sum|none, got {reduction!r}")
        labels, u_lens = labels.contiguous(), u_lens.contiguous()
        U1, B, Od = dec.shape
        V, O = W.shape
        Oe = O - Od
        if Oe < 0 or tuple(bias.shape) != (V,) or tuple(labels.shape) != (B, U1 - 1) or tuple(u_lens.shape) != (B,):
            raise ValueError(f"shape mismatch: dec {tuple(dec.shape)} fc {tuple(W.shape)} bias {tuple(bias.shape)} targets "
                             f"{tuple(labels.shape)} lengths {tuple(u_lens.shape)}")
        Cm = torch.empty(U1, B, V, device=dec.device, dtype=torch.float32)
        gemm(U1 * B, V, Od, dec, W, Cm, b_off=Oe, b_sn=O, b_sk=1, flags=GEMM_GELU_A)
        keep = want_grad and any(ctx.needs_input_grad[:3])
        ilm, lse = _ilm_forward(Cm, bias, labels, u_lens, blank, keep)
        if keep:
            ctx.save_for_backward(dec, W, bias, labels, u_lens, Cm, lse)
            ctx.blank = int(blank)
            ctx.w_param, ctx.b_param = w_param, b_param
        ctx.red_scale = {"none": None, "sum": 1.0, "mean": 1.0 / B}[reduction]
        return _reduce_loss(ilm, ctx.red_scale)

    @staticmethod
    def backward(ctx, g):
        dec, W, bias, labels, u_lens, Cm, lse = ctx.saved_tensors
        dC = torch.empty_like(Cm)
        _ilm_backward(Cm, bias, labels, u_lens, lse, ctx.blank, g, ctx.red_scale, False, dC)
        _, d_dec, dW, db = _joint_backward(None, dec, W, None, dC, (False,) + tuple(ctx.needs_input_grad[:3]),
                                           _direct_grad(ctx.w_param), _direct_grad(ctx.b_param), db_from_c=True)
        return d_dec, dW, db, None, None, None, None, None


class JointLogitsFn(torch.autograd.Function):
    """Materialising joint for RNNTransducer.forward() (model.py:47-50): logits (B,T,U1,V)."""

    @staticmethod
    def forward(ctx, enc, dec, W, bias):
        _need_gpu(enc, dec, W, bias)
        enc, dec, W, bias = _f32c(enc, "enc"), _f32c(dec, "dec"), _f32c(W, "fc.weight"), _f32c(bias, "fc.bias")
        T, B, Oe = enc.shape
        U1, _, Od = dec.shape
        V = W.shape[0]
        A, Cm = _joint_ac(enc, dec, W, Oe, Od, V)
        logits = torch.empty(B, T, U1, V, device=enc.device, dtype=torch.float32)
        check(_lib.lib().rnnt_hip_joint_logits_fwd(_addr(A), V, B * V, _addr(Cm), V, B * V, _addr(bias), B, T, U1, V,
                                                   _addr(logits), _stream()), "rnnt_hip_joint_logits_fwd")
        ctx.save_for_backward(enc, dec, W)
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        enc, dec, W = ctx.saved_tensors
        # compatibility path only (the fused training_step never comes here): two axis sums by torch
        dA = dlogits.sum(dim=2).transpose(0, 1).contiguous()   # (T,B,V)
        dC = dlogits.sum(dim=1).transpose(0, 1).contiguous()   # (U1,B,V)
        return _joint_backward(enc, dec, W, dA, dC, ctx.needs_input_grad[:4])


class RnntLossFromLogitsFn(torch.autograd.Function):
    """warp-transducer-shaped loss on dense logits (model.py:39,57) -> per-utterance NLL (B,).
    fastemit_lambda > 0: FastEmit regularisation of the gradient only (see JointLossFn); the NLL is that of lambda = 0.
    emit_windows = (lo, hi), (B,U) int32: the alignment-restricted loss (see JointLossFn); None: the unrestricted one."""

    @staticmethod
    def forward(ctx, logits, targets, t_lens, u_lens, blank, fastemit_lambda=0.0, emit_windows=None):
        _need_gpu(logits, targets, t_lens, u_lens)
        lam = check_fastemit_lambda(fastemit_lambda)
        if logits.dim() != 4:
            raise ValueError("logits must be (B, T, U+1, V)")
        win = check_emit_windows(emit_windows, logits.shape[0], logits.shape[2] - 1, logits.device)
        code = _logits_dtype_code(logits)
        logits = logits if logits.is_contiguous() else logits.contiguous()
        _i32((("targets", targets), ("logit lengths", t_lens), ("target lengths", u_lens)))
        B, T, U1, V = logits.shape
        if targets.shape != (B, U1 - 1):
            raise ValueError(f"targets must be (B, U) = ({B}, {U1 - 1}), got {tuple(targets.shape)}")
        targets = targets.contiguous()
        grad = torch.empty_like(logits) if logits.requires_grad else None
        nll, _ = _loss_forward("rnnt_hip_loss_from_logits_fwd_bwd", (_addr(logits), code, _addr(targets), _addr(t_lens), _addr(u_lens)),
                               B, T, U1, V, blank, win, lam, (_addr(grad),), logits.device)
        ctx.grad = grad
        return nll

    @staticmethod
    def backward(ctx, g):
        grad = ctx.grad
        ctx.grad = None
        return (grad.float() * g.to(torch.float32).view(-1, 1, 1, 1)).to(grad.dtype), None, None, None, None, None, None


# --------------------------------------------------------------------------------------------------
# CTC loss on per-frame logits and the greedy CTC decode (include/rnnt_hip.h: rnnt_hip_ctc_*, csrc/ctc.hip)
# --------------------------------------------------------------------------------------------------
def _ctc_strides(logits: torch.Tensor, time_major: bool):
    """(B, T, V) and the element strides over b and t of a contiguous (B,T,V) or, time_major, (T,B,V) tensor."""
    if logits.dim() != 3:
        raise ValueError("logits must be (B, T, V), or (T, B, V) with time_major=True")
    if time_major:
        T, B, V = logits.shape
        return B, T, V, V, B * V
    B, T, V = logits.shape
    return B, T, V, T * V, V


def _ctc_operands(logits, time_major: bool, t_lens, labels=None, u_lens=None):
    """The checked operands of a CTC entry: fp32 contiguous logits, int32 contiguous lengths (B,) and, for the entries that take a
    transcript, labels (B, U) and u_lens (B,) (None, None otherwise).
    -> (logits, labels, t_lens, u_lens, B, T, V, z_sb, z_st)."""
    _need_gpu(logits, labels, t_lens, u_lens)
    logits = _f32c(logits, "logits")
    if labels is None:
        _i32((("logit lengths", t_lens),))
    else:
        _i32((("targets", labels), ("logit lengths", t_lens), ("target lengths", u_lens)))
    B, T, V, z_sb, z_st = _ctc_strides(logits, time_major)
    if labels is None:
        if t_lens.shape != (B,):
            raise ValueError(f"logit lengths must be (B,) = ({B},), got {tuple(t_lens.shape)}")
    elif labels.dim() != 2 or labels.shape[0] != B or t_lens.shape != (B,) or u_lens.shape != (B,):
        raise ValueError(f"targets must be (B, U) with B = {B} and both lengths (B,), got {tuple(labels.shape)}, "
                         f"{tuple(t_lens.shape)}, {tuple(u_lens.shape)}")
    else:
        labels, u_lens = labels.contiguous(), u_lens.contiguous()
    return logits, labels, t_lens.contiguous(), u_lens, B, T, V, z_sb, z_st


class CtcLossFn(torch.autograd.Function):
    """logits (B,T,V) (time_major: (T,B,V)) fp32 -> per-utterance CTC NLL (B,), or its "sum" / "mean" over the batch (0-d).
    forward: per-frame terms + alpha/beta (kept in a workspace); backward: the gradient kernel with the upstream gradient folded
    in (1/B under "mean").  Under torch.no_grad() nothing is kept.  A row without any path has NLL +inf (0 with zero_infinity)
    and an exactly zero gradient."""

    @staticmethod
    def forward(ctx, logits, labels, t_lens, u_lens, blank, want_grad=True, reduction="none", time_major=False, zero_infinity=False):
        logits, labels, t_lens, u_lens, B, T, V, z_sb, z_st = _ctc_operands(logits, time_major, t_lens, labels, u_lens)
        if reduction not in ("none", "sum", "mean"):
            raise ValueError(f"reduction must be mean|sum|none, got {reduction!r}")
        U, L = labels.shape[1], _lib.lib()
        nll = torch.empty(B, device=logits.device, dtype=torch.float32)
        nws = L.rnnt_hip_ctc_loss_workspace_bytes(B, T, U, V)
        ws = torch.empty(max(nws, 16), device=logits.device, dtype=torch.uint8)
        check(L.rnnt_hip_ctc_loss_fwd(_addr(logits), z_sb, z_st, _addr(labels) if U else None, _addr(t_lens), _addr(u_lens), B, T, U, V,
                                      int(blank), _addr(nll), _addr(ws), nws, _stream()), "rnnt_hip_ctc_loss_fwd")
        if want_grad and ctx.needs_input_grad[0]:   # want_grad: the caller's torch.is_grad_enabled() (always off in here)
            ctx.save_for_backward(logits, labels, t_lens, u_lens, ws)
            ctx.dims = (B, T, U, V, z_sb, z_st, int(blank), nws)
        if zero_infinity:   # (the row's gradient is zero either way)
            nll = torch.where(torch.isinf(nll), torch.zeros_like(nll), nll)
        ctx.red_scale = {"none": None, "sum": 1.0, "mean": 1.0 / B}[reduction]
        if ctx.red_scale is None:
            return nll
        out = torch.empty((), device=logits.device, dtype=torch.float32)
        check(L.rnnt_hip_scaled_sum_f32(_addr(nll), B, ctx.red_scale, _addr(out), _stream()), "rnnt_hip_scaled_sum_f32")
        return out

    @staticmethod
    def backward(ctx, g):
        logits, labels, t_lens, u_lens, ws = ctx.saved_tensors
        B, T, U, V, z_sb, z_st, blank, nws = ctx.dims
        gvec = _f32c(g.to(torch.float32), "grad of the loss")
        scalar = ctx.red_scale is not None   # reduced loss: ONE upstream scalar, the 1/B of "mean" rides in gscale
        dlogits = torch.empty_like(logits)
        check(_lib.lib().rnnt_hip_ctc_loss_bwd(_addr(logits), z_sb, z_st, _addr(labels) if U else None, _addr(t_lens), _addr(u_lens),
                                               B, T, U, V, blank, ctx.red_scale if scalar else 1.0, _addr(gvec), 0 if scalar else 1,
                                               _addr(dlogits), _addr(ws), nws, _stream()), "rnnt_hip_ctc_loss_bwd")
        return dlogits, None, None, None, None, None, None, None, None


@torch.no_grad()
def ctc_greedy(logits: torch.Tensor, t_lens: torch.Tensor, blank: int, *, time_major: bool = False, return_frames: bool = False):
    """Greedy CTC decode of logits (B,T,V) (time_major: (T,B,V)) fp32, t_lens (B,) int32: per frame the argmax (ties to the
    lowest index), repeats collapsed, blanks dropped.  One launch, then one host copy (the counts).  Returns a list of B 1-D
    LongTensors; with return_frames a list of (tokens, frames) pairs, frames int32: the first frame of each token's run."""
    logits, _, t_lens, _, B, T, V, z_sb, z_st = _ctc_operands(logits, time_major, t_lens)
    tokens = torch.empty(B, T, device=logits.device, dtype=torch.int32)
    counts = torch.empty(B, device=logits.device, dtype=torch.int32)
    frames = torch.empty(B, T, device=logits.device, dtype=torch.int32) if return_frames else None
    check(_lib.lib().rnnt_hip_ctc_greedy(_addr(logits), z_sb, z_st, _addr(t_lens), B, T, V, int(blank), _addr(tokens), _addr(counts),
                                         _addr(frames), _stream()), "rnnt_hip_ctc_greedy")
    n = counts.tolist()   # the only host sync of the decode
    if return_frames:
        return [(tokens[b, :n[b]].long(), frames[b, :n[b]]) for b in range(B)]
    return [tokens[b, :n[b]].long() for b in range(B)]


class CtcAlignment(NamedTuple):
    """Result of ctc_align, on the device (nothing here has synchronised with the host): `first`, `last` (B,U) int32 — the first and
    last frame the best CTC path spends in label u's state, -1 for u >= target_lengths[b] and in a row without any path —, `score`
    (B,) float64 — the log-probability of that path, -inf without one —, `path` (B,T) int32 or None — the token of the path's state
    per frame, the blank id in blank states, -1 past the row's frames —, `token_logp` (B,U) float64 or None — per label the sum of
    its log-probabilities over its span."""
    first: torch.Tensor
    last: torch.Tensor
    score: torch.Tensor
    path: Optional[torch.Tensor]
    token_logp: Optional[torch.Tensor]


class CtcEmitWindows(NamedTuple):
    """`emit_windows=` of JointNet.loss from the model's own CTC head instead of a (lo, hi) pair: the head's best path of the
    transcript gives every label a span [first, last], and label u may be emitted at frames first - left .. last + right."""
    left: int
    right: int


def check_ctc_emit_windows(w: "CtcEmitWindows") -> "CtcEmitWindows":
    for name, v in (("left", w.left), ("right", w.right)):
        if isinstance(v, bool) or not isinstance(v, int) or v < 0:
            raise ValueError(f"CtcEmitWindows: {name} must be an integer >= 0, got {v!r}")
    return w


def ctc_align_workspace_bytes(B: int, T: int, U: int, V: int) -> int:
    n = _lib.lib().rnnt_hip_ctc_align_workspace_bytes(B, T, U, V)
    if n == 0:
        raise ValueError(f"ctc_align: B, T, V must be positive and U >= 0 (B={B} T={T} U={U} V={V})")
    return n


@torch.no_grad()
def ctc_align(logits: torch.Tensor, labels: torch.Tensor, t_lens: torch.Tensor, u_lens: torch.Tensor, blank: int, *,
              time_major: bool = False, return_path: bool = False, return_token_logp: bool = False,
              workspace: Optional[torch.Tensor] = None) -> CtcAlignment:
    """Best CTC path of the known transcripts `labels` (B,U) int32 on logits (B,T,V) (time_major: (T,B,V)) fp32, t_lens / u_lens
    (B,) int32 (include/rnnt_hip.h: rnnt_hip_ctc_align, csrc/ctc.hip): the CTC loss's per-frame terms, its sweep in the (max, +)
    semiring, a back-trace.  `workspace` (uint8, >= ctc_align_workspace_bytes): the caller's buffer, allocated here when None; it
    holds the emission rows afterwards (layout in the header).  -> CtcAlignment; absent outputs are None.  No host sync."""
    _need_gpu(workspace)
    logits, labels, t_lens, u_lens, B, T, V, z_sb, z_st = _ctc_operands(logits, time_major, t_lens, labels, u_lens)
    U, dev, L = labels.shape[1], logits.device, _lib.lib()
    first = torch.empty(B, U, device=dev, dtype=torch.int32)
    last = torch.empty(B, U, device=dev, dtype=torch.int32)
    score = torch.empty(B, device=dev, dtype=torch.float64)
    path = torch.empty(B, T, device=dev, dtype=torch.int32) if return_path else None
    token_logp = torch.empty(B, U, device=dev, dtype=torch.float64) if return_token_logp else None
    nws = ctc_align_workspace_bytes(B, T, U, V)
    ws = torch.empty(nws, device=dev, dtype=torch.uint8) if workspace is None else workspace
    if not isinstance(ws, torch.Tensor) or ws.dtype != torch.uint8 or ws.device != dev or not ws.is_contiguous():
        raise ValueError(f"workspace: expected a contiguous uint8 tensor on {dev}")
    check(L.rnnt_hip_ctc_align(_addr(logits), z_sb, z_st, _addr(labels) if U else None, _addr(t_lens), _addr(u_lens), B, T, U, V,
                               int(blank), _addr(first) if U else None, _addr(last) if U else None, _addr(path),
                               _addr(token_logp) if U else None, _addr(score), _addr(ws), ws.numel() * ws.element_size(), _stream()),
          "rnnt_hip_ctc_align")
    return CtcAlignment(first, last, score, path, token_logp)


def ctc_emit_windows(logits_tm: torch.Tensor, labels: torch.Tensor, t_lens: torch.Tensor, u_lens: torch.Tensor, blank: int,
                     w: "CtcEmitWindows"):
    """(lo, hi) int32 (B, U) for the alignment-restricted loss from the CTC head's logits (T,B,V): lo = first - left, hi = last +
    right around the head's best path (ctc_align on the detached values); a row without a CTC path gets the full window
    [0, T-1].  Entries past u_lens[b] are not read by the loss.  No host sync."""
    al = ctc_align(logits_tm.detach(), labels, t_lens, u_lens, blank, time_major=True)
    nopath = torch.isinf(al.score).unsqueeze(1)
    lo = torch.where(nopath, torch.zeros_like(al.first), al.first - w.left)
    hi = torch.where(nopath, torch.full_like(al.last, logits_tm.shape[0] - 1), al.last + w.right)
    return lo, hi


# --------------------------------------------------------------------------------------------------
# CTC-guided blank-frame skipping in front of the transducer searches (include/rnnt_hip.h: rnnt_hip_ctc_frame_skip, csrc/ctc_skip.hip)
# --------------------------------------------------------------------------------------------------
class FrameSkip(NamedTuple):
    """Result of ctc_frame_skip, on the device (nothing here has synchronised with the host): `enc` (T, B, O) fp32 — per utterance its
    kept frames' rows of the input, in order, in rows 0 .. t_lens[b]-1 (the rows behind them are not written) —, `t_lens` (B,)
    int32 — the number of kept frames —, `frame_map` (B, T) int32 — the original frame of kept frame j, -1 for j >= t_lens[b] —,
    `blank_logp` (B, T) fp32 or None — the head's log-softmax at the blank per valid frame (frames past the input's t_lens[b] are
    not written)."""
    enc: torch.Tensor
    t_lens: torch.Tensor
    frame_map: torch.Tensor
    blank_logp: Optional[torch.Tensor] = None


def check_ctc_skip(threshold, what: str) -> float:
    """ValueError unless threshold is a probability in (0, 1]; -> float32(log threshold), the entry's log_threshold."""
    if isinstance(threshold, bool) or not isinstance(threshold, (int, float)) or math.isnan(threshold) or not 0.0 < threshold <= 1.0:
        raise ValueError(f"{what}: the blank-posterior threshold must be a probability in (0, 1], got {threshold!r}")
    return torch.tensor(math.log(threshold), dtype=torch.float32).item()


@torch.no_grad()
def ctc_frame_skip(logits: torch.Tensor, t_lens: torch.Tensor, blank: int, threshold: float, enc_tm: torch.Tensor, *,
                   time_major: bool = True, return_blank_logp: bool = False) -> FrameSkip:
    """Drops the frames the CTC head calls blank (include/rnnt_hip.h: rnnt_hip_ctc_frame_skip, csrc/ctc_skip.hip):
    logits (T,B,V) (time_major=False: (B,T,V)) fp32 are the head's, t_lens (B,) int32, enc_tm (T,B,O) fp32 the rows to compact
    (the encoder's output).  Frame t < t_lens[b] is skipped exactly when the head's fp32 log-softmax at `blank` exceeds
    float32(log threshold); threshold is a probability in (0, 1], and 1.0 skips nothing.  -> FrameSkip(enc, t_lens, frame_map[,
    blank_logp]): a new (T,B,O) tensor holding the kept rows, the new lengths and the original frame of every kept frame, for the
    searches that take (enc_tm, t_lens).  Two launches, no host sync.  ValueError for bad arguments before anything runs."""
    what = "ctc_frame_skip"
    log_thr = check_ctc_skip(threshold, what)
    for name, t, dt in (("logits", logits, torch.float32), ("enc_tm", enc_tm, torch.float32), ("t_lens", t_lens, torch.int32)):
        if not isinstance(t, torch.Tensor) or t.dtype != dt:
            raise ValueError(f"{what}: {name} must be a {dt} tensor, got {getattr(t, 'dtype', type(t))}")
    if enc_tm.dim() != 3:
        raise ValueError(f"{what}: enc_tm must be (T, B, O), got {tuple(enc_tm.shape)}")
    B, T, V, z_sb, z_st = _ctc_strides(logits, time_major)
    if tuple(enc_tm.shape[:2]) != (T, B) or tuple(t_lens.shape) != (B,):
        raise ValueError(f"{what}: logits give T = {T}, B = {B}; enc_tm must be (T, B, O) and t_lens (B,), got {tuple(enc_tm.shape)}, "
                         f"{tuple(t_lens.shape)}")
    if V < 2 or isinstance(blank, bool) or not 0 <= int(blank) < V:
        raise ValueError(f"{what}: V = {V} < 2 or blank {blank!r} outside [0, {V})")
    if T < 1 or B < 1 or enc_tm.shape[2] < 1:
        raise ValueError(f"{what}: T, B and O must be positive, got logits {tuple(logits.shape)} and enc_tm {tuple(enc_tm.shape)}")
    for name, t in (("logits", logits), ("enc_tm", enc_tm), ("t_lens", t_lens)):
        if not t.is_cuda:
            raise ValueError(f"{what}: {name} is a CPU tensor; there is no CPU path")
    if not (logits.device == enc_tm.device == t_lens.device):
        raise ValueError(f"{what}: logits, enc_tm and t_lens must be on one device")
    logits, enc_tm, t_lens = logits.contiguous(), enc_tm.contiguous(), t_lens.contiguous()
    O, dev, L = enc_tm.shape[2], enc_tm.device, _lib.lib()
    out = torch.empty_like(enc_tm)
    small = torch.empty(B + B * T, device=dev, dtype=torch.int32)   # new lengths | frame map
    lp = torch.empty(B, T, device=dev, dtype=torch.float32) if return_blank_logp else None
    nws = L.rnnt_hip_ctc_frame_skip_workspace_bytes(B, T)
    ws = torch.empty(nws, device=dev, dtype=torch.uint8)
    check(L.rnnt_hip_ctc_frame_skip(_addr(logits), z_sb, z_st, _addr(t_lens), B, T, V, int(blank), log_thr, _addr(enc_tm), O, B * O, O,
                                    _addr(out), O, B * O, _addr(small), _addr(small, B), _addr(lp), _addr(ws), nws, _stream()),
          "rnnt_hip_ctc_frame_skip")
    return FrameSkip(out, small[:B], small[B:].view(B, T), lp)


def map_frames(frames: torch.Tensor, frame_map: torch.Tensor) -> torch.Tensor:
    """frames (B, ...) integer frame numbers of a compacted encoder output -> the original frames through frame_map (B, T) of
    ctc_frame_skip, on the tensors' device; -1 stays -1."""
    flat = frames.reshape(frames.shape[0], -1).long()
    orig = frame_map.gather(1, flat.clamp(min=0)).to(frames.dtype)
    return torch.where(flat < 0, flat.to(frames.dtype), orig).view(frames.shape)


CTC_BEAM_MAX_WIDTH = 128


def _check_search_args(what: str, token_min_logp, **ranges) -> None:
    """ValueError unless every name=(value, max) of `ranges` is an integer in [1, max] and token_min_logp is a number below
    +inf: the argument checks of the frame-synchronous searches."""
    for name, (value, top) in ranges.items():
        if isinstance(value, bool) or not isinstance(value, int) or not 1 <= value <= top:
            raise ValueError(f"{what}: {name} must be an integer in [1, {top}], got {value!r}")
    if isinstance(token_min_logp, bool) or not isinstance(token_min_logp, (int, float)) or math.isnan(token_min_logp) \
            or token_min_logp == math.inf:
        raise ValueError(f"{what}: token_min_logp must be a number below +inf (-inf: no pruning), got {token_min_logp!r}")


def check_ctc_beam_args(beam_width, token_min_logp, what: str) -> None:
    """ValueError unless 1 <= beam_width <= 128 and token_min_logp is a number below +inf: before anything is launched."""
    _check_search_args(what, token_min_logp, **{"beam width": (beam_width, CTC_BEAM_MAX_WIDTH)})


def _hyps_to_host(count, lens_h, tokens, scores, fused=None, frames=None):
    """The searches' result lists from their device outputs: count (B) and lens_h (B, W) are already on the host (the one
    copy of counts and lengths), tokens / frames (B, W, max_len), scores / fused (B, W).  One host copy per array, tokens and
    frames cut to the longest returned hypothesis first.  -> per utterance [(tokens, score[, fused][, frames]), ...]."""
    B = len(count)
    longest = max([1] + [lens_h[b][r] for b in range(B) for r in range(count[b])])
    tok_h, scores_h = tokens[:, :, :longest].cpu(), scores.cpu().tolist()
    out = [[(tok_h[b, r, :lens_h[b][r]].tolist(), scores_h[b][r]) for r in range(count[b])] for b in range(B)]
    if fused is not None:
        fused_h = fused.cpu().tolist()
        out = [[(y, s, fused_h[b][r]) for r, (y, s) in enumerate(hyps)] for b, hyps in enumerate(out)]
    if frames is not None:
        fr_h = frames[:, :, :longest].cpu()
        out = [[(*e, fr_h[b, r, :len(e[0])].tolist()) for r, e in enumerate(hyps)] for b, hyps in enumerate(out)]
    return out


@torch.no_grad()
def ctc_beam_search(logits: torch.Tensor, t_lens: torch.Tensor, blank: int, beam_width: int, *, token_min_logp: float = -math.inf,
                    time_major: bool = False, fusion=None, return_frames: bool = False):
    """CTC prefix beam search (include/rnnt_hip.h: rnnt_hip_ctc_beam_search, csrc/ctc_beam.hip) on logits (B,T,V) (time_major:
    (T,B,V)) fp32, t_lens (B,) int32: per utterance up to `beam_width` (<= 128) hypotheses, best first, as a list of
    (tokens, score) — tokens a list without blanks, score the fp64 CTC log-probability mass the search kept for that labelling, no
    length normalisation.  token_min_logp: per frame only tokens with log-softmax >= it extend a prefix (-inf: all).
    fusion (a fusion.TokenFusion or fusion.NgramFusion over the same V on the logits' device): the search ranks by score + the automaton's total of
    the prefix, the output by score + total + final; every entry is then (tokens, score, fused_score).  return_frames appends
    `frames`: per token the frame at which its prefix first entered the beam.  One launch, then one host copy of the counts and
    lengths (and one per returned array).  Argument errors raise ValueError before anything is launched."""
    check_ctc_beam_args(beam_width, token_min_logp, "ctc_beam_search")
    V = _ctc_strides(logits, time_major)[2]   # the search's own arguments are checked first, before the operands and the GPU
    if V < 2 or not 0 <= int(blank) < V:
        raise ValueError(f"ctc_beam_search: V = {V} < 2 or blank {blank} outside [0, {V})")
    if beam_width * (V + 1) > 1 << 24:
        raise ValueError(f"ctc_beam_search: beam_width * (V + 1) = {beam_width * (V + 1)} exceeds 2^24 candidates per frame")
    check_fusion(fusion, V, logits.device, "ctc_beam_search", ngram=True)
    logits, _, t_lens, _, B, T, V, z_sb, z_st = _ctc_operands(logits, time_major, t_lens)
    dev, W, L = logits.device, beam_width, _lib.lib()
    tokens = torch.empty(B, W, T, device=dev, dtype=torch.int32)
    small = torch.empty(B + B * W, device=dev, dtype=torch.int32)   # counts | lens: one transfer
    scores = torch.empty(B, W, device=dev, dtype=torch.float64)
    frames = torch.empty(B, W, T, device=dev, dtype=torch.int32) if return_frames else None
    fused = torch.empty(B, W, device=dev, dtype=torch.float64) if fusion is not None else None
    fs = fusion_struct(fusion, fused) if fusion is not None else None
    nws = L.rnnt_hip_ctc_beam_workspace_bytes(B, T, V, W)
    if nws == 0:
        raise ValueError(f"ctc_beam_search: sizes outside the kernel's limits (B={B} T={T} V={V} W={W})")
    ws = torch.empty(nws, device=dev, dtype=torch.uint8)
    entry = "rnnt_hip_ctc_beam_search_ngram" if isinstance(fs, _lib.BeamNgram) else "rnnt_hip_ctc_beam_search"
    check(getattr(L, entry)(_addr(logits), z_sb, z_st, _addr(t_lens), B, T, V, int(blank), W, float(token_min_logp),
                            C.byref(fs) if fs is not None else None, _addr(tokens), _addr(small, B), _addr(scores),
                            _addr(frames), _addr(small), _addr(ws), nws, _stream()), entry)
    host = small.cpu()   # the only host sync of the search
    return _hyps_to_host(host[:B].tolist(), host[B:].reshape(B, W).tolist(), tokens, scores, fused, frames)


# --------------------------------------------------------------------------------------------------
# forced alignment (include/rnnt_hip.h: rnnt_hip_joint_align / rnnt_hip_align_from_logits_ex): best path of a known transcript
# --------------------------------------------------------------------------------------------------
class Alignment:
    """Result of an alignment call, on the device: `frames` (B,U) int32 — frames[b, u] = the frame at which label u of
    utterance b is emitted on the best path, -1 for u >= target_lengths[b] — and `score` (B,) float64, the log-probability of
    that path (-inf, frames -1, for an utterance without frames).  Nothing here has synchronised with the host yet;
    `token_frames(b)` does, once, for the whole batch."""

    def __init__(self, frames: torch.Tensor, score: torch.Tensor, u_lens: torch.Tensor):
        self.frames, self.score, self.target_lengths = frames, score, u_lens
        self._host = None

    def token_frames(self, b: int) -> List[int]:
        """The un-padded list of emission frames of utterance b (one host copy of the batch on first use)."""
        if self._host is None:
            self._host = (self.frames.tolist(), self.target_lengths.tolist())
        rows, n = self._host
        return rows[b][:n[b]]


def _align_buffers(B, U1, device, frames, score):
    frames = torch.empty(B, U1 - 1, device=device, dtype=torch.int32) if frames is None else frames
    score = torch.empty(B, device=device, dtype=torch.float64) if score is None else score
    _check_buffer("frames", frames, (B, U1 - 1), torch.int32, device)
    _check_buffer("score", score, (B,), torch.float64, device)
    return frames, score


def _align_lengths(labels, t_lens, u_lens, B, U1):
    _i32((("targets", labels), ("frame lengths", t_lens), ("target lengths", u_lens)))
    if labels.shape != (B, U1 - 1) or t_lens.shape != (B,) or u_lens.shape != (B,):
        raise ValueError(f"targets must be (B, U) = ({B}, {U1 - 1}) and both lengths (B,), got {tuple(labels.shape)}, "
                         f"{tuple(t_lens.shape)}, {tuple(u_lens.shape)}")
    return labels.contiguous(), t_lens.contiguous(), u_lens.contiguous()


def align_workspace_bytes(B: int, T: int, U1: int, V: int) -> int:
    n = _lib.lib().rnnt_hip_joint_align_workspace_bytes(B, T, U1, V)
    if n == 0:
        raise ValueError(f"alignment: dims must be positive (B={B} T={T} U1={U1} V={V})")
    return n


def joint_align(A: torch.Tensor, Cm: torch.Tensor, bias: torch.Tensor, labels: torch.Tensor, t_lens: torch.Tensor,
                u_lens: torch.Tensor, blank: int, *, batch_first: bool = False, workspace: Optional[torch.Tensor] = None,
                frames: Optional[torch.Tensor] = None, score: Optional[torch.Tensor] = None) -> Alignment:
    """Best RNN-T path per utterance for logits[b,t,u,:] = A[b,t,:] + C[b,u,:] + bias, never built.  A (T,B,V) and Cm (U1,B,V)
    time-major as the joint's pre-GEMMs leave them (batch_first=True: (B,T,V) and (B,U1,V)), fp32 contiguous; labels (B,U),
    t_lens, u_lens int32.  `workspace` (uint8, >= align_workspace_bytes), `frames`, `score`: the caller's buffers, allocated
    here when None.  No host synchronisation."""
    _need_gpu(A, Cm, bias, labels, t_lens, u_lens, workspace, frames, score)
    A, Cm, bias = _f32c(A, "A"), _f32c(Cm, "C"), _f32c(bias, "bias")
    if A.dim() != 3 or Cm.dim() != 3:
        raise ValueError("joint_align takes A (T,B,V) and C (U1,B,V) (or batch-first with batch_first=True)")
    (B, T, V), U1 = (A.shape, Cm.shape[1]) if batch_first else ((A.shape[1], A.shape[0], A.shape[2]), Cm.shape[0])
    if Cm.shape != ((B, U1, V) if batch_first else (U1, B, V)) or bias.shape != (V,):
        raise ValueError(f"shape mismatch: A {tuple(A.shape)} C {tuple(Cm.shape)} bias {tuple(bias.shape)}")
    labels, t_lens, u_lens = _align_lengths(labels, t_lens, u_lens, B, U1)
    frames, score = _align_buffers(B, U1, A.device, frames, score)
    nws = align_workspace_bytes(B, T, U1, V)
    ws = torch.empty(nws, device=A.device, dtype=torch.uint8) if workspace is None else workspace
    a_sb, a_st, c_sb, c_su = (T * V, V, U1 * V, V) if batch_first else (V, B * V, V, B * V)
    check(_lib.lib().rnnt_hip_joint_align(_addr(A), a_sb, a_st, _addr(Cm), c_sb, c_su, _addr(bias), _addr(labels), _addr(t_lens),
                                          _addr(u_lens), B, T, U1, V, int(blank), _addr(frames), _addr(score), _addr(ws),
                                          ws.numel() * ws.element_size(), _stream()), "rnnt_hip_joint_align")
    return Alignment(frames, score, u_lens)


def align_from_logits(logits: torch.Tensor, labels: torch.Tensor, t_lens: torch.Tensor, u_lens: torch.Tensor, blank: int, *,
                      workspace: Optional[torch.Tensor] = None, frames: Optional[torch.Tensor] = None,
                      score: Optional[torch.Tensor] = None) -> Alignment:
    """joint_align for dense logits (B,T,U1,V) in float32, float16 or bfloat16 (arithmetic fp32 / fp64 whatever the storage)."""
    _need_gpu(logits, labels, t_lens, u_lens, workspace, frames, score)
    code = _logits_dtype_code(logits)
    if logits.dim() != 4:
        raise ValueError("logits must be (B, T, U+1, V)")
    logits = logits if logits.is_contiguous() else logits.contiguous()
    B, T, U1, V = logits.shape
    labels, t_lens, u_lens = _align_lengths(labels, t_lens, u_lens, B, U1)
    frames, score = _align_buffers(B, U1, logits.device, frames, score)
    nws = align_workspace_bytes(B, T, U1, V)
    ws = torch.empty(nws, device=logits.device, dtype=torch.uint8) if workspace is None else workspace
    check(_lib.lib().rnnt_hip_align_from_logits_ex(_addr(logits), code, _addr(labels), _addr(t_lens), _addr(u_lens),
                                                   B, T, U1, V, int(blank), _addr(frames), _addr(score), _addr(ws),
                                                   ws.numel() * ws.element_size(), _stream()), "rnnt_hip_align_from_logits_ex")
    return Alignment(frames, score, u_lens)


# --------------------------------------------------------------------------------------------------
# greedy decoding (replaces the host loop of transducer.py:95-145)
# --------------------------------------------------------------------------------------------------
class TimedTokens(NamedTuple):
    """One utterance's greedy result with timing: three 1-D tensors of equal length."""
    tokens: torch.Tensor   # int64
    frames: torch.Tensor   # int32: the encoder frame each token was chosen at (streaming: counted from the stream's last reset)
    logp: torch.Tensor     # float32: log-softmax of the joint at that evaluation, at the chosen token


def _check_rnn_weights(rnn_weights, cell: int, I0: int, H: int, what: str) -> None:
    """Shapes of a uni-directional stack's [w_ih, w_hh, b_ih, b_hh] per layer (layer 0 reads I0 inputs, the others H)."""
    ngate = {0: 4, 1: 3, 2: 1, 3: 1}.get(cell)
    if ngate is None or not rnn_weights or len(rnn_weights) % 4 != 0:
        raise ValueError(f"{what}: cell {cell!r} / {len(rnn_weights)} weight tensors")
    for i, w in enumerate(rnn_weights):
        want = [(ngate * H, I0 if i < 4 else H), (ngate * H, H), (ngate * H,), (ngate * H,)][i % 4]
        if not isinstance(w, torch.Tensor) or tuple(w.shape) != want:
            raise ValueError(f"{what} weight #{i}: expected shape {want}, "
                             f"got {tuple(w.shape) if isinstance(w, torch.Tensor) else type(w).__name__}")


def _fill_prednet_weights(d, emb_w, rnn_weights, cell: int, what: str) -> list:
    """The prediction net of a search or step descriptor: checks the layer limit and every weight shape against the embedding
    width (the kernels index raw pointers), fills d.Hp, d.L, d.cell, d.emb and the per-layer weights.  -> tensors to keep alive."""
    Hp, L = emb_w.shape[1], len(rnn_weights) // 4
    if L > _lib.DECODE_MAX_LAYERS:
        raise ValueError(f"{what}: {L} prediction-net layers (RNNT_DECODE_MAX_LAYERS = {_lib.DECODE_MAX_LAYERS})")
    _check_rnn_weights(rnn_weights, cell, Hp, Hp, "prediction net")
    keep = [_f32c(t, "prediction-net weight") for t in rnn_weights] + [_f32c(emb_w, "embedding")]
    d.Hp, d.L, d.cell, d.emb = Hp, L, cell, _addr(keep[-1])
    for l in range(L):
        d.w_ih[l], d.w_hh[l], d.b_ih[l], d.b_hh[l] = (_addr(t) for t in keep[4 * l:4 * l + 4])
    return keep


def _fill_prednet(d, fc_w, emb_w, rnn_weights, cell: int, out_w, out_b, blank: int, what: str) -> list:
    """The prediction net and its half of the joint of a search descriptor (greedy or beam, offline or streaming): fc, out_proj
    and embedding checked against each other (a row of the embedding per fc output: the kernels read emb[tok] for any tok < V),
    0 <= blank < V, then _fill_prednet_weights; fills d.V, d.O, d.blank, d.w_o, d.b_o and the fc slice d.w_d / d.ld_d, whose
    offset Oe = Ocat - Od is the encoder's share of the joint input.  -> tensors to keep alive."""
    V, Ocat = fc_w.shape
    Od, Hp = out_w.shape[0], emb_w.shape[1]
    if not 1 <= Od < Ocat or tuple(out_w.shape) != (Od, Hp) or tuple(out_b.shape) != (Od,) or emb_w.shape[0] < V:
        raise ValueError(f"{what}: fc {tuple(fc_w.shape)} / out_proj {tuple(out_w.shape)} / embedding {tuple(emb_w.shape)} "
                         "do not fit together (the embedding needs a row per fc output)")
    if not 0 <= blank < V:
        raise ValueError(f"{what}: blank {blank} outside [0,{V})")
    keep = _fill_prednet_weights(d, emb_w, rnn_weights, cell, what)
    keep += [_f32c(out_w, "out_proj weight"), _f32c(out_b, "out_proj bias"), _f32c(fc_w, "fc weight")]
    d.V, d.O, d.blank = V, Od, blank
    d.w_o, d.b_o = _addr(keep[-3]), _addr(keep[-2])
    d.w_d, d.ld_d = _addr(keep[-1], Ocat - Od), Ocat
    return keep


def _search_fit(d, enc_tm, fc_w, fc_b, emb_w, rnn_weights, cell: int, out_w, out_b, blank: int, what: str):
    """The host half of the opening of the three offline searches on enc_tm (T,B,Oe): _fill_prednet on the search's descriptor
    d, then the joint's weights against the encoder's width.  Nothing here touches a device, so each search keeps its own
    argument checks where they were, around this call.  -> (keep, T, B, V)"""
    T, B, Oe = enc_tm.shape
    V, Ocat = fc_w.shape
    keep = _fill_prednet(d, fc_w, emb_w, rnn_weights, cell, out_w, out_b, blank, what)
    if Ocat - d.O != Oe or tuple(fc_b.shape) != (V,):
        raise ValueError(f"{what}: fc {tuple(fc_w.shape)} / {tuple(fc_b.shape)} / out_proj {tuple(out_w.shape)} do not fit "
                         f"encoder width {Oe}")
    return keep, T, B, V


def _joint_half(enc_tm: torch.Tensor, fc_w: torch.Tensor, fc_b: torch.Tensor) -> torch.Tensor:
    """The device half of that opening: A (T,B,V) = gelu(enc_tm) W_e^T + fc_b, the encoder half of the joint, in one product
    (fc_w: the float32 contiguous (V, Oe + Od) weight _search_fit kept, its encoder columns first)."""
    T, B, Oe = enc_tm.shape
    V, Ocat = fc_w.shape
    A = torch.empty(T, B, V, device=enc_tm.device, dtype=torch.float32)
    gemm(T * B, V, Oe, enc_tm, fc_w, A, b_sn=Ocat, b_sk=1, bias=fc_b, flags=GEMM_GELU_A)
    return A


def _aligned_workspace(nbytes: int, device):
    """A search's workspace of nbytes at a 256-byte boundary: nbytes + 256 are allocated and the address is rounded up.
    -> (the tensor that owns it, the aligned address)"""
    ws = torch.empty(nbytes + 256, device=device, dtype=torch.uint8)
    return ws, (_addr(ws) + 255) // 256 * 256


def _check_step_group(step_group, what: str) -> None:
    if isinstance(step_group, bool) or not isinstance(step_group, int) or step_group < 0:
        raise ValueError(f"{what}: step_group must be an integer >= 0, got {step_group!r}")


def greedy_decode(enc_tm: torch.Tensor, fc_w: torch.Tensor, fc_b: torch.Tensor, emb_w: torch.Tensor, rnn_weights,
                  cell: int, out_w: torch.Tensor, out_b: torch.Tensor, blank: int, max_iters: int,
                  t_lens: Optional[torch.Tensor] = None, timing: bool = False, max_out: Optional[int] = None):
    """enc_tm (T,B,Oe) encoder outputs (time-major) -> (tokens (B, T*max_iters) int64, ntok (B,) int32), all on device.
    rnn_weights: [w_ih, w_hh, b_ih, b_hh] per prediction-net layer; t_lens (B) int32 on device = frames visited per
    utterance (None: all T).  timing=True (rnnt_hip_greedy_decode_timed, the same kernel) -> (tokens, ntok, frames (B,
    max_out) int32, logp (B, max_out) float32): per appended token the frame it was chosen at and the log-softmax of the
    joint there.  max_out (default T*max_iters, which never truncates) caps the stored entries per utterance."""
    _need_gpu(enc_tm, fc_w, emb_w)
    enc_tm = _f32c(enc_tm, "encoder outputs")
    d, dev = _lib.DecodeDesc(), enc_tm.device
    keep, T, B, V = _search_fit(d, enc_tm, fc_w, fc_b, emb_w, rnn_weights, cell, out_w, out_b, blank, "greedy decode")
    if max_iters < 1:
        raise ValueError(f"greedy decode: max_iters {max_iters} < 1")
    A = _joint_half(enc_tm, keep[-1], fc_b)
    max_out = T * max_iters if max_out is None else int(max_out)
    if max_out < 1:
        raise ValueError(f"greedy decode: max_out {max_out} < 1")
    tokens = torch.full((B, max_out), blank, device=dev, dtype=torch.int64)
    ntok = torch.zeros(B, device=dev, dtype=torch.int32)
    d.T, d.B, d.max_iters, d.max_out = T, B, max_iters, max_out
    d.A, d.t_lens = _addr(A), _addr(t_lens)
    d.tokens, d.ntok = _addr(tokens), _addr(ntok)
    if timing:
        frames = torch.full((B, max_out), -1, device=dev, dtype=torch.int32)
        logp = torch.zeros(B, max_out, device=dev, dtype=torch.float32)
        tm = _lib.GreedyTiming(_addr(frames), _addr(logp), None)
        check(_lib.lib().rnnt_hip_greedy_decode_timed(C.byref(d), C.byref(tm), _stream()), "rnnt_hip_greedy_decode_timed")
        return tokens, ntok, frames, logp
    check(_lib.lib().rnnt_hip_greedy_decode(C.byref(d), _stream()), "rnnt_hip_greedy_decode")
    return tokens, ntok


def prednet_step(tokens: torch.Tensor, emb_w: torch.Tensor, rnn_weights, cell: int, h_in=None, c_in=None):
    """One prediction-net step for a batch with carried state (decoder.py:121-123).  tokens (B,) int64; h_in / c_in (L,B,H)
    or None (zeros) -> (h_out, c_out) with c_out None unless LSTM; the layer output is h_out[-1]."""
    _need_gpu(tokens, emb_w)
    L = len(rnn_weights) // 4
    B, H = tokens.numel(), emb_w.shape[1]
    d = _lib.PrednetStepDesc()
    keep = _fill_prednet_weights(d, emb_w, rnn_weights, cell, "prediction-net step")
    for name, t in (("h_in", h_in), ("c_in", c_in)):
        if t is not None and tuple(t.shape) != (L, B, H):
            raise ValueError(f"{name} must be (L,B,H) = ({L},{B},{H}), got {tuple(t.shape)}")
    tokens = tokens.reshape(-1).to(torch.int64).contiguous()
    h_out = torch.empty(L, B, H, device=emb_w.device, dtype=torch.float32)
    c_out = torch.empty_like(h_out) if cell == _lib.CELL_LSTM else None
    d.B, d.tokens = B, _addr(tokens)
    h_in = None if h_in is None else _f32c(h_in, "h_in")
    c_in = None if c_in is None else _f32c(c_in, "c_in")
    d.h_in, d.c_in, d.h_out, d.c_out = _addr(h_in), _addr(c_in), _addr(h_out), _addr(c_out)
    check(_lib.lib().rnnt_hip_prednet_step(C.byref(d), _stream()), "rnnt_hip_prednet_step")
    return h_out, c_out


# --------------------------------------------------------------------------------------------------
# beam search (replaces the host loop of transducer.py:215-361 with lm=None, hotwords=None; with fusion=, the lm_score branch
# over a token automaton: fusion.py)
# --------------------------------------------------------------------------------------------------
NGRAM_SEARCHES = "recognize_beams_sync, init_beam_sync_stream / recognize_beams_sync_stream and recognize_ctc_beams"


def check_fusion(fusion, V: int, device, what: str, ngram: bool = False) -> None:
    """ValueError unless `fusion` is None or a TokenFusion over V tokens on `device`, or, where the search walks backoff tables
    (ngram=True), an NgramFusion: before anything is launched."""
    if fusion is None:
        return
    from .fusion import NgramFusion, TokenFusion
    if isinstance(fusion, NgramFusion):
        if not ngram:
            raise ValueError(f"{what}: an NgramFusion is taken by the searches whose cost per frame is bounded ({NGRAM_SEARCHES}); "
                             "this search takes a TokenFusion (NgramFusion.to_dense() where it fits)")
    elif not isinstance(fusion, TokenFusion):
        raise ValueError(f"{what}: fusion must be a rnntransducer_amd.TokenFusion{' or NgramFusion' if ngram else ''}, got "
                         f"{type(fusion).__name__}")
    if fusion.vocab_size != V:
        raise ValueError(f"{what}: the fusion automaton is over {fusion.vocab_size} tokens, the model's joint over {V}")
    if fusion.device != device:
        raise ValueError(f"{what}: the fusion tables are on {fusion.device}, the search runs on {device}; use fusion.to(device)")


ILM_SEARCHES = "recognize_beams_sync and init_beam_sync_stream / recognize_beams_sync_stream"


def check_ilm_weight(ilm_weight, what: str) -> float:
    """ValueError unless ilm_weight is a finite number >= 0 (0: no internal-LM subtraction): before anything runs.  -> float"""
    if isinstance(ilm_weight, bool) or not isinstance(ilm_weight, (int, float)) or not math.isfinite(ilm_weight) or ilm_weight < 0:
        raise ValueError(f"{what}: ilm_weight must be a finite number >= 0 (0: off), got {ilm_weight!r}")
    return float(ilm_weight)


def refuse_ilm_weight(ilm_weight, what: str, why: str) -> None:
    """The searches that cannot subtract the internal LM: ValueError naming the two that can, unless ilm_weight is None or 0."""
    if ilm_weight is not None and not (isinstance(ilm_weight, (int, float)) and ilm_weight == 0):
        raise ValueError(f"{what}: ilm_weight is not taken here ({why}); internal-LM subtraction is taken by {ILM_SEARCHES}")


def ilm_fusion(fusion, V: int, device):
    """The automaton an internal-LM call runs with: `fusion`, or without one the all-zero one-state TokenFusion (subtraction
    alone)."""
    if fusion is not None:
        return fusion
    from .fusion import TokenFusion
    return TokenFusion(torch.zeros(1, V, dtype=torch.int32), torch.zeros(1, V), torch.zeros(1)).to(device)


def fusion_struct(fusion, fused_scores: torch.Tensor):
    """rnnt_beam_fusion of a checked TokenFusion, or rnnt_beam_ngram of a checked NgramFusion (raw pointers: the caller keeps
    `fusion` and `fused_scores` alive)."""
    from .fusion import NgramFusion
    if isinstance(fusion, NgramFusion):
        return _lib.BeamNgram(_addr(fusion.row_ptr), _addr(fusion.tok), _addr(fusion.arc), _addr(fusion.next), _addr(fusion.bow),
                              _addr(fusion.backoff), _addr(fusion.final), fusion.root, fusion.order, fusion.n_states, fusion.n_arcs,
                              _addr(fused_scores))
    return _lib.BeamFusion(_addr(fusion.next), _addr(fusion.arc), _addr(fusion.final), fusion.n_states, _addr(fused_scores))


def ilm_struct(bias: torch.Tensor, weight: float):
    """rnnt_beam_ilm over the joint's bias (a raw pointer: the caller keeps the tensor alive)."""
    if bias.dtype != torch.float32 or not bias.is_contiguous():
        raise ValueError("internal-LM subtraction: fc.bias must be a contiguous float32 tensor")
    return _lib.BeamIlm(_addr(bias), weight)


def beam_search(enc_tm: torch.Tensor, fc_w: torch.Tensor, fc_b: torch.Tensor, emb_w: torch.Tensor, rnn_weights,
                cell: int, out_w: torch.Tensor, out_b: torch.Tensor, blank: int, beam: int, improved: bool = False,
                state_beam: float = 4.6, expand_beam: float = 2.3, t_lens: Optional[torch.Tensor] = None, *,
                max_pops: int = 1024, max_candidates: Optional[int] = None, max_states: Optional[int] = None,
                max_nodes: int = 1 << 18, max_len: Optional[int] = None, stats: bool = False, frames: bool = False,
                fusion=None):
    """enc_tm (T,B,Oe) encoder outputs (time-major) -> per utterance the n-best list [(y_star, asr_score), ...] of
    transducer.py:215-361 (lm=None), one kernel launch for the batch (csrc/beam.hip) and one host sync.
    t_lens (B) int32 on device = frames visited per utterance (None: all T).  Caps (each raises RnntHipError naming it):
    max_pops = pops per frame, max_candidates = A entries per frame (default max_pops * V), max_states = live prediction-net
    states (default 3 * max_pops: a frame carries at most 2 per B entry and adds 1 per pop), max_nodes = y_star prefix nodes
    per utterance, max_len = tokens of a returned y_star (default 4 T + 64).  stats=True also returns a (B, 6) int tensor:
    pops, prediction-net steps run, max pops in a frame, max A entries in a frame, max live states, prefix nodes.
    frames=True (rnnt_hip_beam_search_timed, the same kernel): every entry is (y_star, asr_score, frames) with frames aligned
    with y_star: the frame at which each token was appended, -1 for the leading blank.
    fusion (a fusion.TokenFusion on enc_tm's device; rnnt_hip_beam_search_fused, the FUSED instance of the same kernel): the
    search ranks by asr_score + the automaton's total, and every entry is (y_star, asr_score, fused_score[, frames]) with
    fused_score = asr_score + total + final, fp64.  Positive arcs can make a frame's pop loop run away: max_pops bounds it."""
    _need_gpu(enc_tm, fc_w, emb_w)
    enc_tm = _f32c(enc_tm, "encoder outputs")
    d, dev = _lib.BeamDesc(), enc_tm.device
    keep, T, B, V = _search_fit(d, enc_tm, fc_w, fc_b, emb_w, rnn_weights, cell, out_w, out_b, blank, "beam search")
    if V < 2 or beam < 1:
        raise ValueError(f"beam search: V {V} < 2 or beam {beam} < 1")
    check_fusion(fusion, V, dev, "beam search")
    max_candidates = max_pops * V if max_candidates is None else max_candidates
    max_states = 3 * max_pops if max_states is None else max_states
    max_len = 4 * T + 64 if max_len is None else max_len
    A = _joint_half(enc_tm, keep[-1], fc_b)
    tokens = torch.empty(B, beam, max_len, device=dev, dtype=torch.int32)
    lens = torch.empty(B, beam, device=dev, dtype=torch.int32)
    scores = torch.empty(B, beam, device=dev, dtype=torch.float64)
    small = torch.empty(B, 2 + _lib.BEAM_NSTATS, device=dev, dtype=torch.int32)   # count | status | stats: one transfer
    d.T, d.B = T, B
    d.beam, d.improved, d.state_beam, d.expand_beam = beam, int(bool(improved)), float(state_beam), float(expand_beam)
    d.max_candidates, d.max_pops, d.max_states, d.max_nodes, d.max_len = max_candidates, max_pops, max_states, max_nodes, max_len
    ws_query = _lib.lib().rnnt_hip_beam_workspace_bytes if fusion is None else _lib.lib().rnnt_hip_beam_fused_workspace_bytes
    ws_bytes = ws_query(C.byref(d))
    if ws_bytes == 0:
        raise ValueError("beam search: invalid sizes or caps (all caps must be >= 1)")
    ws, d.workspace = _aligned_workspace(ws_bytes, dev)
    d.workspace_bytes = ws_bytes
    d.A, d.t_lens = _addr(A), _addr(t_lens)
    d.tokens, d.lens, d.scores = _addr(tokens), _addr(lens), _addr(scores)
    d.count, d.status, d.stats = _addr(small), _addr(small, B), _addr(small, 2 * B)
    tm = fr = fused = None
    if frames:
        fr = torch.empty(B, beam, max_len, device=dev, dtype=torch.int32)
        tm = _lib.BeamTiming(_addr(fr), None)
    if fusion is not None:
        fused = torch.empty(B, beam, device=dev, dtype=torch.float64)
        fs = fusion_struct(fusion, fused)
        check(_lib.lib().rnnt_hip_beam_search_fused(C.byref(d), C.byref(fs), C.byref(tm) if frames else None, _stream()),
              "rnnt_hip_beam_search_fused")
    elif frames:
        check(_lib.lib().rnnt_hip_beam_search_timed(C.byref(d), C.byref(tm), _stream()), "rnnt_hip_beam_search_timed")
    else:
        check(_lib.lib().rnnt_hip_beam_search(C.byref(d), _stream()), "rnnt_hip_beam_search")
    host = small.cpu()   # the only host sync of the search
    count, status = host.reshape(-1)[:B].tolist(), host.reshape(-1)[B:2 * B].tolist()
    for b, st in enumerate(status):
        if st != 0:
            what, kw = _lib.BEAM_STATUS.get(st, ("unknown", "?"))
            cap = {"max_candidates": max_candidates, "max_pops": max_pops, "max_states": max_states, "max_nodes": max_nodes,
                   "max_len": max_len}.get(kw)
            raise RnntHipError(f"beam search: utterance {b} exceeded the cap on {what} ({kw}={cap}); raise it with the {kw}= "
                               "keyword (the reference's search is unbounded here)")
    out = _hyps_to_host(count, lens.cpu().tolist(), tokens, scores, fused, fr)
    if stats:
        return out, host.reshape(-1)[2 * B:].reshape(B, _lib.BEAM_NSTATS)
    return out


# --------------------------------------------------------------------------------------------------
# frame-synchronous beam search with batched hypothesis steps (include/rnnt_hip.h: rnnt_hip_beam_sync_search, csrc/beam_sync.hip)
# --------------------------------------------------------------------------------------------------
def check_beam_sync_args(beam_width, max_symbols, token_min_logp, what: str) -> None:
    """ValueError unless 1 <= beam_width <= 64, 1 <= max_symbols <= 4 and token_min_logp is a number below +inf."""
    _check_search_args(what, token_min_logp, **{"beam width": (beam_width, _lib.BEAM_SYNC_MAX_WIDTH),
                                                "max_symbols": (max_symbols, _lib.BEAM_SYNC_MAX_SYMBOLS)})


@torch.no_grad()
def beam_search_sync(enc_tm: torch.Tensor, fc_w: torch.Tensor, fc_b: torch.Tensor, emb_w: torch.Tensor, rnn_weights,
                     cell: int, out_w: torch.Tensor, out_b: torch.Tensor, blank: int, beam_width: int, max_symbols: int = 1,
                     t_lens: Optional[torch.Tensor] = None, *, token_min_logp: float = -math.inf, frames: bool = False,
                     fusion=None, step_group: int = 0, ilm_weight: float = 0.0):
    """Frame-synchronous transducer beam search (include/rnnt_hip.h: rnnt_hip_beam_sync_search, csrc/beam_sync.hip, DESIGN.md
    §20) on enc_tm (T,B,Oe) encoder outputs (time-major): per frame the whole beam (beam_width <= 64) expands at once, at most
    max_symbols (<= 4) tokens are emitted, hypotheses with the same token sequence merge by logaddexp, and the prediction net
    advances once for all new hypotheses together.  -> per utterance up to beam_width entries (y, score), best first by score
    (fp64: the log-probability mass the search kept for y; no length normalisation), y with the leading blank as beam_search
    returns y_star.  t_lens (B) int32 on device = frames visited per utterance (None: all T).  token_min_logp: per frame only
    tokens whose log-softmax reaches it extend a hypothesis (-inf: all; the blank is never pruned).
    fusion (a fusion.TokenFusion or fusion.NgramFusion on enc_tm's device): ranked by score + the automaton's total, the output by
    score + total + final; every entry is then (y, score, fused_score).  frames=True appends `frames`: per token the frame at which its prefix's
    node was created (-1 for the leading blank).  step_group: 0, or a smaller number of hypotheses per step group than the
    kernel would take (results do not depend on it).
    ilm_weight = mu > 0 (rnnt_hip_beam_sync_search_ilm): internal-LM subtraction.  Every emitted token v also adds
    -mu * ilm_h[v] to the total, ilm_h = the fp32 log-softmax over the non-blank tokens of Cv_h + fc_b (the joint with the
    encoder zeroed); fused_score carries it.  Without fusion the all-zero automaton is used: subtraction alone, entries still
    (y, score, fused_score).  0: the entries above, untouched.
    The cost per frame is bounded by beam_width, V and max_symbols: no cap can overflow.  One search launch, then one host copy
    of the counts and lengths (and one per returned array).  Argument errors raise ValueError before anything runs."""
    tokens, lens, counts, scores, host, fused, fr = _beam_search_sync_run(
        enc_tm, fc_w, fc_b, emb_w, rnn_weights, cell, out_w, out_b, blank, beam_width, max_symbols, t_lens, token_min_logp, frames,
        fusion, step_group, ilm_weight)
    B, W = lens.shape
    return _hyps_to_host(host[:B].tolist(), host[B:].reshape(B, W).tolist(), tokens, scores, fused, fr)


@torch.no_grad()
def beam_search_sync_device(enc_tm: torch.Tensor, fc_w: torch.Tensor, fc_b: torch.Tensor, emb_w: torch.Tensor, rnn_weights,
                            cell: int, out_w: torch.Tensor, out_b: torch.Tensor, blank: int, beam_width: int, max_symbols: int = 1,
                            t_lens: Optional[torch.Tensor] = None, *, token_min_logp: float = -math.inf, fusion=None,
                            ilm_weight: float = 0.0):
    """beam_search_sync with its results left on the device (MWER training packs them into loss inputs there):
    -> (tokens (B, W, 1 + max_symbols*T) int32 with the leading blank, lens (B, W) int32, counts (B,) int32, scores (B, W) fp64,
    host): `host` is the search's one host copy, a CPU int32 tensor counts | lens.  Entries of rank >= counts[b] are unwritten.
    fusion (a TokenFusion or NgramFusion): the search ranks with it as beam_search_sync does, and the tuple gains a sixth entry,
    fused (B, W) fp64.  ilm_weight > 0: internal-LM subtraction as in beam_search_sync; the sixth entry is then always there."""
    out = _beam_search_sync_run(enc_tm, fc_w, fc_b, emb_w, rnn_weights, cell, out_w, out_b, blank, beam_width, max_symbols, t_lens,
                                token_min_logp, False, fusion, 0, ilm_weight)
    return out[:5] if out[5] is None else out[:6]


def _beam_search_sync_run(enc_tm, fc_w, fc_b, emb_w, rnn_weights, cell, out_w, out_b, blank, beam_width, max_symbols, t_lens,
                          token_min_logp, frames, fusion, step_group, ilm_weight=0.0):
    """The launch behind beam_search_sync and beam_search_sync_device -> (tokens, lens, counts, scores, host, fused, frames)."""
    check_beam_sync_args(beam_width, max_symbols, token_min_logp, "beam_search_sync")
    mu = check_ilm_weight(ilm_weight, "beam_search_sync")
    _check_step_group(step_group, "beam_search_sync")
    if enc_tm.dim() != 3 or fc_w.dim() != 2:
        raise ValueError(f"beam_search_sync: encoder outputs must be (T,B,Oe) and fc (V,Oe+Od), got {tuple(enc_tm.shape)} / "
                         f"{tuple(fc_w.shape)}")
    (T, B, _), V = enc_tm.shape, fc_w.shape[0]
    if V < 2:
        raise ValueError(f"beam_search_sync: V = {V} < 2 (a blank and at least one token)")
    if beam_width * V > 1 << 24:
        raise ValueError(f"beam_search_sync: beam_width * V = {beam_width * V} exceeds 2^24 candidates per round")
    if T < 1 or B < 1:
        raise ValueError(f"beam_search_sync: T and B must be positive, got T={T} B={B}")
    d = _lib.BeamSyncDesc()
    keep = _search_fit(d, enc_tm, fc_w, fc_b, emb_w, rnn_weights, cell, out_w, out_b, int(blank), "beam_search_sync")[0]
    check_fusion(fusion, V, enc_tm.device, "beam_search_sync", ngram=True)
    if t_lens is not None and (t_lens.dtype != torch.int32 or tuple(t_lens.shape) != (B,)):
        raise ValueError(f"beam_search_sync: t_lens must be (B,) = ({B},) int32, got {tuple(t_lens.shape)} {t_lens.dtype}")
    _need_gpu(enc_tm, fc_w, emb_w)   # every argument check above runs without a device
    enc_tm = _f32c(enc_tm, "encoder outputs")
    dev, W, S, L = enc_tm.device, beam_width, max_symbols, _lib.lib()
    if mu > 0.0:
        fusion, fc_b = ilm_fusion(fusion, V, dev), _f32c(fc_b, "fc bias")
    A = _joint_half(enc_tm, keep[-1], fc_b)
    max_len = 1 + S * T
    tokens = torch.empty(B, W, max_len, device=dev, dtype=torch.int32)
    small = torch.empty(B + B * W, device=dev, dtype=torch.int32)   # counts | lens: one transfer
    scores = torch.empty(B, W, device=dev, dtype=torch.float64)
    d.T, d.B, d.beam, d.max_symbols, d.step_group, d.token_min_logp = T, B, W, S, step_group, float(token_min_logp)
    d.A, d.a_st, d.a_sb = _addr(A), B * V, V
    d.t_lens = _addr(t_lens.contiguous()) if t_lens is not None else None
    nws = (L.rnnt_hip_beam_sync_ilm_workspace_bytes if mu > 0.0 else L.rnnt_hip_beam_sync_workspace_bytes)(C.byref(d))
    if nws == 0:
        raise ValueError("beam_search_sync: " + L.rnnt_hip_last_error().decode("utf-8", "replace"))
    ws, d.workspace = _aligned_workspace(nws, dev)
    d.workspace_bytes = nws
    d.tokens, d.lens, d.scores, d.count = _addr(tokens), _addr(small, B), _addr(scores), _addr(small)
    fr = torch.empty(B, W, max_len, device=dev, dtype=torch.int32) if frames else None
    tm = _lib.BeamTiming(_addr(fr), None) if frames else None
    fused = torch.empty(B, W, device=dev, dtype=torch.float64) if fusion is not None else None
    fs = fusion_struct(fusion, fused) if fusion is not None else None
    if mu > 0.0:
        entry, ngram = "rnnt_hip_beam_sync_search_ilm", isinstance(fs, _lib.BeamNgram)
        ilm = ilm_struct(fc_b, mu)
        check(L.rnnt_hip_beam_sync_search_ilm(C.byref(d), None if ngram else C.byref(fs), C.byref(fs) if ngram else None, C.byref(ilm),
                                              C.byref(tm) if tm is not None else None, _stream()), entry)
    else:
        entry = "rnnt_hip_beam_sync_search_ngram" if isinstance(fs, _lib.BeamNgram) else "rnnt_hip_beam_sync_search"
        check(getattr(L, entry)(C.byref(d), C.byref(fs) if fs is not None else None, C.byref(tm) if tm is not None else None,
                                _stream()), entry)
    host = small.cpu()   # the only host sync of the search
    return tokens, small[B:].view(B, W), small[:B], scores, host, fused, fr


# --------------------------------------------------------------------------------------------------
# MWER training (include/rnnt_hip.h: rnnt_hip_edit_distance / rnnt_hip_nbest_pack / rnnt_hip_mwer_risk, csrc/mwer.hip)
# --------------------------------------------------------------------------------------------------
MWER_MAX_LEN = 511     # tokens per sequence of the edit distance and per packed hypothesis: the loss's U + 1 <= 512
MWER_MAX_NBEST = 64    # = the search's beam width limit


def _i32c(t: torch.Tensor, name: str, shape=None) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or (shape is not None and tuple(t.shape) != tuple(shape)):
        got = (tuple(t.shape), t.dtype) if isinstance(t, torch.Tensor) else type(t).__name__
        raise ValueError(f"{name} must be int32{'' if shape is None else ' of shape ' + str(tuple(shape))}, got {got}")
    return t if t.is_contiguous() else t.contiguous()


@torch.no_grad()
def edit_distance(hyp: torch.Tensor, hyp_lens: torch.Tensor, ref: torch.Tensor, ref_lens: torch.Tensor,
                  ref_div: int = 1) -> torch.Tensor:
    """Levenshtein distances on the device (rnnt_hip_edit_distance): hyp (P, Lh) and ref (Q, Lr) int32 token rows with int32
    lengths (P,) / (Q,); pair p compares hyp[p, :hyp_lens[p]] with ref[p // ref_div, :ref_lens[p // ref_div]], so ref_div
    hypotheses share one reference (P = Q * ref_div).  -> (P,) int32, exact; what metrics.edit_distance gives on the host.
    Rows of up to 511 tokens; what lies behind a row's length is not read."""
    if isinstance(ref_div, bool) or not isinstance(ref_div, int) or ref_div < 1:
        raise ValueError(f"edit_distance: ref_div must be a positive integer, got {ref_div!r}")
    if not isinstance(hyp, torch.Tensor) or not isinstance(ref, torch.Tensor) or hyp.dim() != 2 or ref.dim() != 2:
        raise ValueError("edit_distance: hyp and ref must be 2-D int32 tensors")
    P, Q = hyp.shape[0], ref.shape[0]
    if P < 1 or P != Q * ref_div:
        raise ValueError(f"edit_distance: {P} hypothesis rows do not match {Q} reference rows x ref_div = {ref_div}")
    if hyp.shape[1] > MWER_MAX_LEN or ref.shape[1] > MWER_MAX_LEN:
        raise ValueError(f"edit_distance: rows of up to {MWER_MAX_LEN} tokens, got {hyp.shape[1]} / {ref.shape[1]}")
    hyp, ref = _i32c(hyp, "edit_distance: hyp"), _i32c(ref, "edit_distance: ref")
    hyp_lens, ref_lens = _i32c(hyp_lens, "edit_distance: hyp_lens", (P,)), _i32c(ref_lens, "edit_distance: ref_lens", (Q,))
    _need_gpu(hyp, hyp_lens, ref, ref_lens)
    Lh, Lr = hyp.shape[1], ref.shape[1]
    if Lh == 0:   # an empty row still needs an address
        hyp = torch.zeros(P, 1, device=hyp.device, dtype=torch.int32)
    if Lr == 0:
        ref = torch.zeros(Q, 1, device=ref.device, dtype=torch.int32)
    dist = torch.empty(P, device=hyp.device, dtype=torch.int32)
    check(_lib.lib().rnnt_hip_edit_distance(_addr(hyp), Lh, _addr(hyp_lens), _addr(ref), Lr, _addr(ref_lens), ref_div, P, _addr(dist),
                                            _stream()), "rnnt_hip_edit_distance")
    return dist


def nbest_umax(host: torch.Tensor, B: int, N: int, max_hyp_len: int = MWER_MAX_LEN) -> int:
    """The longest valid hypothesis (tokens behind the leading blank, at most max_hyp_len) in the search's host copy counts | lens;
    at least 1.  Host arithmetic on what the search has already copied: no device sync."""
    counts, lens = host[:B].tolist(), host[B:].reshape(B, N).tolist()
    return max([1] + [lens[b][n] - 1 for b in range(B) for n in range(min(counts[b], N)) if lens[b][n] - 1 <= max_hyp_len])


@torch.no_grad()
def nbest_pack(tokens: torch.Tensor, lens: torch.Tensor, counts: torch.Tensor, frame_lens: torch.Tensor, Umax: int, blank: int,
               max_hyp_len: int = MWER_MAX_LEN):
    """The device results of beam_search_sync_device -> the loss's inputs for rows r = b*N + n (rnnt_hip_nbest_pack): tokens
    (B, N, max_len) int32 with the leading blank, lens (B, N), counts (B,), frame_lens (B,) int32, Umax from nbest_umax.
    -> texts (B*N, Umax+1) int64 (blank, hypothesis, blank padding), labels (B*N, Umax) int32, u_lens (B*N,), t_lens (B*N,)
    (the utterance's frame count; 0 for an invalid row, which the loss answers with +inf and exact-zero gradients), valid (B*N,)
    int32.  A row is invalid when its rank is >= counts[b] or its hypothesis is longer than max_hyp_len tokens."""
    if not isinstance(tokens, torch.Tensor) or tokens.dim() != 3:
        raise ValueError("nbest_pack: tokens must be (B, N, max_len) int32")
    B, N, max_len = tokens.shape
    for name, v, top in (("N", N, MWER_MAX_NBEST), ("Umax", Umax, MWER_MAX_LEN), ("max_hyp_len", max_hyp_len, MWER_MAX_LEN)):
        if isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= top:
            raise ValueError(f"nbest_pack: {name} must be an integer in [1, {top}], got {v!r}")
    if B < 1 or max_len < 1:
        raise ValueError(f"nbest_pack: tokens {tuple(tokens.shape)} has an empty dimension")
    tokens = _i32c(tokens, "nbest_pack: tokens")
    lens, counts = _i32c(lens, "nbest_pack: lens", (B, N)), _i32c(counts, "nbest_pack: counts", (B,))
    frame_lens = _i32c(frame_lens, "nbest_pack: frame_lens", (B,))
    _need_gpu(tokens, lens, counts, frame_lens)
    dev, R = tokens.device, B * N
    texts = torch.empty(R, Umax + 1, device=dev, dtype=torch.int64)
    labels = torch.empty(R, Umax, device=dev, dtype=torch.int32)
    u_lens, t_lens, valid = (torch.empty(R, device=dev, dtype=torch.int32) for _ in range(3))
    check(_lib.lib().rnnt_hip_nbest_pack(_addr(tokens), max_len, _addr(counts), _addr(lens), _addr(frame_lens), B, N, Umax, max_hyp_len,
                                         int(blank), _addr(texts), _addr(labels), _addr(u_lens), _addr(t_lens), _addr(valid),
                                         _stream()), "rnnt_hip_nbest_pack")
    return texts, labels, u_lens, t_lens, valid


class MwerRiskFn(torch.autograd.Function):
    """Expected number of token errors over an n-best list, relative to the list's mean (rnnt_hip_mwer_risk, fp64 inside): nll
    (B*N,) fp32 per-hypothesis losses, dist (B*N,) int32 edit distances, valid (B*N,) int32 -> risk (B,) fp32 (reduction "none"),
    or its 0-d "mean" / "sum" over B.  The forward also stores d risk_b / d nll_j (B*N, exactly 0 for invalid rows); the backward
    is those weights times the upstream gradient."""

    @staticmethod
    def forward(ctx, nll, dist, valid, N, reduction="none"):
        if isinstance(N, bool) or not isinstance(N, int) or not 1 <= N <= MWER_MAX_NBEST:
            raise ValueError(f"mwer risk: N must be an integer in [1, {MWER_MAX_NBEST}], got {N!r}")
        if reduction not in ("none", "mean", "sum"):
            raise ValueError(f"mwer risk: reduction must be 'none', 'mean' or 'sum', got {reduction!r}")
        if nll.dim() != 1 or nll.numel() < N or nll.numel() % N:
            raise ValueError(f"mwer risk: nll must be (B*N,) with N = {N}, got {tuple(nll.shape)}")
        R = nll.numel()
        B = R // N
        nll = _f32c(nll.detach(), "mwer risk: nll")
        dist, valid = _i32c(dist, "mwer risk: dist", (R,)), _i32c(valid, "mwer risk: valid", (R,))
        _need_gpu(nll, dist, valid)
        risk = torch.empty(B, device=nll.device, dtype=torch.float32)
        weights = torch.empty(R, device=nll.device, dtype=torch.float32)
        check(_lib.lib().rnnt_hip_mwer_risk(_addr(nll), _addr(dist), _addr(valid), B, N, 1.0, _addr(risk), _addr(weights), _stream()),
              "rnnt_hip_mwer_risk")
        ctx.save_for_backward(weights)
        ctx.red_scale = {"none": None, "sum": 1.0, "mean": 1.0 / B}[reduction]
        ctx.N = N
        if ctx.red_scale is None:
            return risk
        out = torch.empty((), device=nll.device, dtype=torch.float32)
        check(_lib.lib().rnnt_hip_scaled_sum_f32(_addr(risk), B, ctx.red_scale, _addr(out), _stream()), "rnnt_hip_scaled_sum_f32")
        return out

    @staticmethod
    def backward(ctx, g):
        (weights,) = ctx.saved_tensors
        g = g.to(torch.float32)
        if ctx.red_scale is not None:
            return weights * (g * ctx.red_scale), None, None, None, None
        return (weights.view(-1, ctx.N) * g.unsqueeze(1)).reshape(-1), None, None, None, None


# --------------------------------------------------------------------------------------------------
# streaming greedy recognition (include/rnnt_hip.h: rnnt_hip_stream_rnn_chunk / rnnt_hip_stream_greedy[_reset]); the state
# tensors belong to streaming.GreedyStreamState
# --------------------------------------------------------------------------------------------------
def _check_buffer(name: str, t: Optional[torch.Tensor], shape, dtype, device) -> None:
    """A caller-owned buffer the streaming kernels index as a dense array of `shape`."""
    if not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(shape) or t.dtype != dtype or t.device != device \
            or not t.is_contiguous():
        got = (tuple(t.shape), t.dtype, str(t.device), "contiguous" if t.is_contiguous() else "strided") \
            if isinstance(t, torch.Tensor) else type(t).__name__
        raise ValueError(f"{name}: expected a contiguous {dtype} tensor of shape {tuple(shape)} on {device}, got {got}")


def stream_rnn_chunk(chunk: torch.Tensor, lens: torch.Tensor, rnn_weights, cell: int, h: torch.Tensor, c: Optional[torch.Tensor],
                     out_w: torch.Tensor, out_b: torch.Tensor, out: torch.Tensor, out_strides: Tuple[int, int],
                     fc_w: Optional[torch.Tensor] = None, fc_b: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
    """Unidirectional encoder over one chunk with carried state.  chunk (B,T,F) fp32 (any strides with unit feature stride),
    lens (B) int32 on device (frames per stream; the kernels never read past T whatever they hold), h / c (L,B,H) updated in
    place (c: LSTM only, else None); frame t of stream b of out_proj(h_top) goes to out + b * out_strides[0] + t * out_strides[1]
    (zeros past lens).  With fc_w / fc_b: returns A (T,B,V) = gelu(out) W_e^T + b (the encoder half of the joint).
    The kernels index raw pointers: every shape is checked here, on the host, before anything is launched."""
    _need_gpu(chunk, lens, h, c, out_w, out_b, out, fc_w, fc_b, *rnn_weights)
    if chunk.dim() != 3 or chunk.dtype != torch.float32:
        raise ValueError(f"chunk must be (B,T,F) float32, got {tuple(chunk.shape)} {chunk.dtype}")
    B, T, F = chunk.shape
    dev = chunk.device
    if not isinstance(h, torch.Tensor) or h.dim() != 3:
        raise ValueError("h must be an (L,B,H) tensor")
    L, H = h.shape[0], h.shape[2]
    _check_rnn_weights(rnn_weights, cell, F, H, "encoder")
    if len(rnn_weights) != 4 * L:
        raise ValueError(f"encoder: {len(rnn_weights) // 4} layers of weights for an ({L},B,H) state")
    _check_buffer("encoder h", h, (L, B, H), torch.float32, dev)
    if cell == _lib.CELL_LSTM:
        _check_buffer("encoder c", c, (L, B, H), torch.float32, dev)
    _check_buffer("lengths", lens, (B,), torch.int32, dev)
    O = out_w.shape[0]
    if tuple(out_w.shape) != (O, H) or tuple(out_b.shape) != (O,):
        raise ValueError(f"out_proj {tuple(out_w.shape)} / {tuple(out_b.shape)} does not fit hidden size {H}")
    sb, st = out_strides
    if out.dtype != torch.float32 or not out.is_contiguous() or sb < 0 or st < 0 or \
            (B - 1) * sb + (T - 1) * st + O > out.numel():
        raise ValueError(f"out: a contiguous float32 buffer holding (B,T,O) = ({B},{T},{O}) at strides {out_strides}")
    if chunk.stride(2) != 1:
        chunk = chunk.contiguous()
    d = _lib.StreamRnnDesc()
    d.T, d.B, d.F, d.H, d.L, d.cell, d.O = T, B, F, H, L, cell, O
    d.x, d.x_sb, d.x_st, d.lens = _addr(chunk), chunk.stride(0), chunk.stride(1), _addr(lens)
    keep = [_f32c(t, "encoder weight") for t in rnn_weights]
    for l in range(min(L, _lib.STREAM_MAX_LAYERS)):   # more layers: the entry refuses and names the limit
        d.w_ih[l], d.w_hh[l], d.b_ih[l], d.b_hh[l] = (_addr(t) for t in keep[4 * l:4 * l + 4])
    out_w, out_b = _f32c(out_w, "out_proj weight"), _f32c(out_b, "out_proj bias")
    d.h, d.c, d.w_o, d.b_o = _addr(h), _addr(c), _addr(out_w), _addr(out_b)
    d.out = _addr(out)
    d.out_sb, d.out_st = sb, st
    A = None
    if fc_w is not None:
        V = fc_w.shape[0]
        if fc_w.dim() != 2 or fc_w.shape[1] < O or tuple(fc_b.shape) != (V,):
            raise ValueError(f"fc {tuple(fc_w.shape)} / {tuple(fc_b.shape)} does not fit encoder width {O}")
        fc_w, fc_b = _f32c(fc_w, "fc weight"), _f32c(fc_b, "fc bias")
        A = torch.empty(T, B, V, device=dev, dtype=torch.float32)
        d.V, d.fc_w, d.ld_fc, d.fc_b, d.A = V, _addr(fc_w), fc_w.shape[1], _addr(fc_b), _addr(A)
    nbytes = _lib.lib().rnnt_hip_stream_rnn_workspace_bytes(C.byref(d))
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    d.workspace, d.workspace_bytes = _addr(ws), nbytes
    check(_lib.lib().rnnt_hip_stream_rnn_chunk(C.byref(d), _stream()), "rnnt_hip_stream_rnn_chunk")
    return A


def _stream_greedy_desc(T: int, B: int, fc_w, emb_w, rnn_weights, cell: int, out_w, out_b, blank: int, h, c, Cs, last):
    """Descriptor of the streaming search; every weight and state shape checked against the others (raw pointers)."""
    d = _lib.StreamGreedyDesc()
    keep = _fill_prednet(d, fc_w, emb_w, rnn_weights, cell, out_w, out_b, blank, "streaming greedy search")
    V, Hp, L, dev = d.V, d.Hp, d.L, fc_w.device
    _check_buffer("prediction-net h", h, (L, B, Hp), torch.float32, dev)
    if cell == _lib.CELL_LSTM:
        _check_buffer("prediction-net c", c, (L, B, Hp), torch.float32, dev)
    _check_buffer("prediction-net joint half", Cs, (B, V), torch.float32, dev)
    _check_buffer("last token", last, (B,), torch.int64, dev)
    d.T, d.B = T, B
    d.h, d.c, d.C, d.last = _addr(h), _addr(c), _addr(Cs), _addr(last)
    return d, keep


def stream_greedy_reset(rows: torch.Tensor, fc_w, emb_w, rnn_weights, cell: int, out_w, out_b, blank: int, h, c, Cs, last) -> None:
    """Prime rows (int32 on device) of the prediction-net state as transducer.py:116-119: zero state, one blank step."""
    _need_gpu(rows, fc_w, emb_w, h, Cs, last)
    d, keep = _stream_greedy_desc(1, h.shape[1], fc_w, emb_w, rnn_weights, cell, out_w, out_b, blank, h, c, Cs, last)
    _check_buffer("rows", rows, (rows.numel(),), torch.int32, fc_w.device)
    if rows.numel() and not bool(((rows >= 0) & (rows < h.shape[1])).all()):
        raise ValueError(f"rows must lie in [0, {h.shape[1]})")
    check(_lib.lib().rnnt_hip_stream_greedy_reset(C.byref(d), _addr(rows), rows.numel(), _stream()), "rnnt_hip_stream_greedy_reset")


def stream_greedy(A: torch.Tensor, lens: torch.Tensor, fc_w, emb_w, rnn_weights, cell: int, out_w, out_b, blank: int, max_iters: int,
                  h, c, Cs, last, frame_base: Optional[torch.Tensor] = None):
    """Greedy search over one chunk from carried state.  A (T,B,V) from stream_rnn_chunk, lens (B) int32 on device; h / c / Cs /
    last updated in place -> (tokens (B, T*max_iters) int64, ntok (B,) int32) appended in this chunk.  With frame_base ((B,)
    int64 on device: the frames every stream consumed before this chunk; rnnt_hip_stream_greedy_timed, the same kernel) ->
    (tokens, ntok, frames (B, T*max_iters) int32 absolute, logp float32)."""
    _need_gpu(A, lens, fc_w, emb_w, h, Cs, last)
    T, B = A.shape[0], A.shape[1]
    d, keep = _stream_greedy_desc(T, B, fc_w, emb_w, rnn_weights, cell, out_w, out_b, blank, h, c, Cs, last)
    _check_buffer("A", A, (T, B, fc_w.shape[0]), torch.float32, fc_w.device)
    _check_buffer("lengths", lens, (B,), torch.int32, fc_w.device)
    if max_iters < 1:
        raise ValueError(f"max_iters must be >= 1, got {max_iters}")
    max_out = T * max_iters
    tokens = torch.full((B, max_out), blank, device=A.device, dtype=torch.int64)
    ntok = torch.zeros(B, device=A.device, dtype=torch.int32)
    d.max_iters, d.max_out = max_iters, max_out
    d.A, d.lens, d.tokens, d.ntok = _addr(A), _addr(lens), _addr(tokens), _addr(ntok)
    if frame_base is not None:
        _check_buffer("frame_base", frame_base, (B,), torch.int64, fc_w.device)
        frames = torch.full((B, max_out), -1, device=A.device, dtype=torch.int32)
        logp = torch.zeros(B, max_out, device=A.device, dtype=torch.float32)
        tm = _lib.GreedyTiming(_addr(frames), _addr(logp), _addr(frame_base))
        check(_lib.lib().rnnt_hip_stream_greedy_timed(C.byref(d), C.byref(tm), _stream()), "rnnt_hip_stream_greedy_timed")
        return tokens, ntok, frames, logp
    check(_lib.lib().rnnt_hip_stream_greedy(C.byref(d), _stream()), "rnnt_hip_stream_greedy")
    return tokens, ntok


# --------------------------------------------------------------------------------------------------
# streaming beam search (include/rnnt_hip.h: rnnt_hip_beam_stream_*); the workspace and the output buffers belong to
# streaming.BeamStreamState
# --------------------------------------------------------------------------------------------------
BEAM_STREAM_CAPS = ("max_pops", "max_candidates", "max_states", "max_nodes", "max_len")


def beam_stream_caps(V: int, beam: int, *, max_pops: Optional[int] = None, max_candidates: Optional[int] = None,
                     max_states: Optional[int] = None, max_nodes: int = 8192, max_len: int = 256) -> dict:
    """The streaming defaults of the caps of `beam_search`: max_pops = max(128, 4 * beam) pops per frame, max_candidates =
    max_pops * V, max_states = 3 * max_pops, max_nodes = 8192 LIVE prefix nodes (the tree is collected after every chunk, so
    this must hold the carried tree plus one chunk's growth of at most one node per pop), max_len = 256 tokens of a y_star
    not yet committed.  The offline defaults size for a whole utterance without collection (max_pops 1024, 2^18 nodes)."""
    max_pops = max(128, 4 * beam) if max_pops is None else max_pops
    caps = dict(max_pops=max_pops, max_candidates=max_pops * V if max_candidates is None else max_candidates,
                max_states=3 * max_pops if max_states is None else max_states, max_nodes=max_nodes, max_len=max_len)
    for k, v in caps.items():
        if not isinstance(v, int) or v < 1:
            raise ValueError(f"streaming beam search: {k} must be an integer >= 1, got {v!r}")
    return caps


def beam_stream_desc(B: int, fc_w, emb_w, rnn_weights, cell: int, out_w, out_b, blank: int, beam: int, improved: bool,
                     state_beam: float, expand_beam: float, caps: dict):
    """Descriptor of the streaming beam search with every weight shape checked against the others (raw pointers); the
    workspace, A, lens and the outputs are the caller's to fill.  -> (descriptor, tensors to keep alive)."""
    _need_gpu(fc_w, emb_w)
    d = _lib.BeamStreamDesc()
    keep = _fill_prednet(d, fc_w, emb_w, rnn_weights, cell, out_w, out_b, blank, "streaming beam search")
    if d.V < 2 or beam < 1 or B < 1:
        raise ValueError(f"streaming beam search: V {d.V} < 2, beam {beam} < 1 or {B} streams")
    d.T, d.B = 0, B
    d.beam, d.improved, d.state_beam, d.expand_beam = beam, int(bool(improved)), float(state_beam), float(expand_beam)
    d.max_candidates, d.max_pops, d.max_states, d.max_nodes, d.max_len = (caps[k] for k in ("max_candidates", "max_pops",
                                                                                           "max_states", "max_nodes", "max_len"))
    return d, keep


def beam_stream_workspace_bytes(d, fused: bool = False) -> int:
    """Bytes of the carried workspace; fused=True: the layout of the *_fused entries (side arrays for the fusion fields)."""
    L = _lib.lib()
    n = (L.rnnt_hip_beam_stream_fused_workspace_bytes if fused else L.rnnt_hip_beam_stream_workspace_bytes)(C.byref(d))
    if n == 0:
        raise ValueError("streaming beam search: invalid sizes or caps (all caps must be >= 1)")
    return n


def beam_stream_reset(d, rows: torch.Tensor, build_table: bool, fusion=None) -> None:
    """rows (int32 on device, each in [0, B): the caller checks) start a new utterance in the workspace d points to.
    fusion: the rnnt_beam_fusion struct of a stream opened with one (fusion_struct): the fused layout, automaton state 0."""
    _need_gpu(rows)
    _check_buffer("rows", rows, (rows.numel(),), torch.int32, rows.device)
    if fusion is not None:
        check(_lib.lib().rnnt_hip_beam_stream_reset_fused(C.byref(d), C.byref(fusion), _addr(rows), rows.numel(), int(build_table),
                                                          _stream()), "rnnt_hip_beam_stream_reset_fused")
        return
    check(_lib.lib().rnnt_hip_beam_stream_reset(C.byref(d), _addr(rows), rows.numel(), int(build_table), _stream()),
          "rnnt_hip_beam_stream_reset")


def beam_stream_chunk(d, A: torch.Tensor, lens: torch.Tensor, frames: Optional[torch.Tensor] = None,
                      commit_frames: Optional[torch.Tensor] = None, fusion=None) -> None:
    """One chunk: A (T,B,V) from stream_rnn_chunk, lens (B) int32 on device; the outputs d points to are written.  With
    frames (B, beam, max_len) and commit_frames (B, max_nodes), int32 on device: rnnt_hip_beam_stream_chunk_timed, the same
    kernel, which also writes the tail's and the committed tokens' absolute frames.  fusion: the rnnt_beam_fusion struct the
    stream was reset with (rnnt_hip_beam_stream_chunk_fused, with or without frames)."""
    _need_gpu(A, lens)
    _check_buffer("A", A, (A.shape[0], d.B, d.V), torch.float32, A.device)
    _check_buffer("lengths", lens, (d.B,), torch.int32, A.device)
    d.T, d.A, d.lens = A.shape[0], _addr(A), _addr(lens)
    try:
        tm = None
        if frames is not None:
            _check_buffer("frames", frames, (d.B, d.beam, d.max_len), torch.int32, A.device)
            _check_buffer("commit_frames", commit_frames, (d.B, d.max_nodes), torch.int32, A.device)
            tm = _lib.BeamTiming(_addr(frames), _addr(commit_frames))
        if fusion is not None:
            check(_lib.lib().rnnt_hip_beam_stream_chunk_fused(C.byref(d), C.byref(fusion), C.byref(tm) if tm is not None else None,
                                                              _stream()), "rnnt_hip_beam_stream_chunk_fused")
        elif frames is not None:
            check(_lib.lib().rnnt_hip_beam_stream_chunk_timed(C.byref(d), C.byref(tm), _stream()), "rnnt_hip_beam_stream_chunk_timed")
        else:
            check(_lib.lib().rnnt_hip_beam_stream_chunk(C.byref(d), _stream()), "rnnt_hip_beam_stream_chunk")
    finally:
        d.T, d.A, d.lens = 0, None, None


# --------------------------------------------------------------------------------------------------
# streaming frame-synchronous beam search (include/rnnt_hip.h: rnnt_hip_beam_sync_stream_*, csrc/beam_sync_stream.hip); the
# workspace and the output buffers belong to streaming.BeamSyncStreamState
# --------------------------------------------------------------------------------------------------
BEAM_SYNC_STREAM_CAPS = ("max_nodes", "max_len")


def beam_sync_stream_caps(beam: int, max_symbols: int, *, max_nodes: int = 8192, max_len: int = 256) -> dict:
    """The two caps of the streaming frame-synchronous search, checked: max_nodes = live prefix-tree nodes (the tree is
    collected at every chunk's end and inside a chunk whenever a frame would not find beam * max_symbols free slots; at least
    1 + 4 * beam * max_symbols), max_len = tokens of a returned sequence that are not yet committed."""
    caps = dict(max_nodes=max_nodes, max_len=max_len)
    for k, v in caps.items():
        if isinstance(v, bool) or not isinstance(v, int) or v < 1:
            raise ValueError(f"streaming frame-synchronous beam search: {k} must be an integer >= 1, got {v!r}")
    need = 1 + 4 * beam * max_symbols
    if max_nodes < need or max_nodes >= (1 << 31) // 5:
        raise ValueError(f"streaming frame-synchronous beam search: max_nodes = {max_nodes} outside [1 + 4 * beam_widths * "
                         f"max_symbols = {need}, 2^31 / 5)")
    return caps


def beam_sync_stream_desc(B: int, fc_w, emb_w, rnn_weights, cell: int, out_w, out_b, blank: int, beam: int, max_symbols: int,
                          token_min_logp: float, caps: dict, step_group: int = 0):
    """Descriptor of the streaming frame-synchronous beam search with every weight shape checked against the others (raw
    pointers) and the search options checked as beam_search_sync checks them; the workspace, A, lens and the outputs are the
    caller's to fill.  -> (descriptor, tensors to keep alive)."""
    what = "streaming frame-synchronous beam search"
    check_beam_sync_args(beam, max_symbols, token_min_logp, what)
    _check_step_group(step_group, what)
    if B < 1:
        raise ValueError(f"{what}: {B} streams")
    _need_gpu(fc_w, emb_w)
    d = _lib.BeamSyncStreamDesc()
    keep = _fill_prednet(d, fc_w, emb_w, rnn_weights, cell, out_w, out_b, int(blank), what)
    if d.V < 2 or beam * d.V > 1 << 24:
        raise ValueError(f"{what}: V = {d.V} < 2, or beam_widths * V = {beam * d.V} exceeds 2^24 candidates per round")
    d.T, d.B = 0, B
    d.beam, d.max_symbols, d.step_group, d.token_min_logp = beam, max_symbols, step_group, float(token_min_logp)
    d.max_nodes, d.max_len = caps["max_nodes"], caps["max_len"]
    return d, keep


def beam_sync_stream_workspace_bytes(d, ilm: bool = False) -> int:
    """Bytes of the carried workspace (ValueError with the library's message for sizes outside its limits).  ilm: of a stream
    opened with internal-LM subtraction, which also carries the (m, lse) pair of every state slot."""
    L = _lib.lib()
    n = (L.rnnt_hip_beam_sync_stream_ilm_workspace_bytes if ilm else L.rnnt_hip_beam_sync_stream_workspace_bytes)(C.byref(d))
    if n == 0:
        raise ValueError("streaming frame-synchronous beam search: " + L.rnnt_hip_last_error().decode("utf-8", "replace"))
    return n


def beam_sync_stream_reset(d, rows: torch.Tensor, build_table: bool, ilm: bool = False) -> None:
    """rows (int32 on device, each in [0, B): the caller checks) start a new utterance in the workspace d points to (ilm: a
    workspace of the internal-LM layout)."""
    _need_gpu(rows)
    _check_buffer("rows", rows, (rows.numel(),), torch.int32, rows.device)
    entry = "rnnt_hip_beam_sync_stream_reset_ilm" if ilm else "rnnt_hip_beam_sync_stream_reset"
    check(getattr(_lib.lib(), entry)(C.byref(d), _addr(rows), rows.numel(), int(build_table), _stream()), entry)


def beam_sync_stream_chunk(d, A: torch.Tensor, lens_dev: torch.Tensor, commit: torch.Tensor, frames: Optional[torch.Tensor] = None,
                           commit_frames: Optional[torch.Tensor] = None, fusion=None, ilm=None) -> None:
    """One chunk: A (T,B,V) float32 (from stream_rnn_chunk; any positive frame and stream strides with contiguous rows), lens_dev
    (B) int32 on device, commit (B, max_nodes + max_symbols * T) int32; the outputs d points to are written.  frames
    (B, beam, max_len) and commit_frames (shaped as commit), int32 on device: the tails' and the committed tokens' absolute
    frames are written too.  fusion: the rnnt_beam_fusion or rnnt_beam_ngram struct of the stream's automaton (fusion_struct), the
    same for every chunk.  ilm: the rnnt_beam_ilm struct of a stream opened with internal-LM subtraction (fusion is then required;
    d.workspace has the internal-LM layout)."""
    _need_gpu(A, lens_dev, commit)
    dev = A.device
    if A.dim() != 3 or tuple(A.shape[1:]) != (d.B, d.V) or A.dtype != torch.float32 or A.shape[0] < 1 or A.stride(2) != 1 \
            or A.stride(0) < 1 or A.stride(1) < 1:
        raise ValueError(f"A: expected float32 (T >= 1, {d.B}, {d.V}) with contiguous rows, got {tuple(A.shape)} {A.dtype} "
                         f"strides {A.stride()}")
    T = A.shape[0]
    _check_buffer("lengths", lens_dev, (d.B,), torch.int32, dev)
    ncom = d.max_nodes + d.max_symbols * T
    _check_buffer("commit", commit, (d.B, ncom), torch.int32, dev)
    tm = None
    if frames is not None or commit_frames is not None:
        _check_buffer("frames", frames, (d.B, d.beam, d.max_len), torch.int32, dev)
        _check_buffer("commit_frames", commit_frames, (d.B, ncom), torch.int32, dev)
        tm = _lib.BeamTiming(_addr(frames), _addr(commit_frames))
    d.T, d.A, d.a_st, d.a_sb, d.lens, d.commit = T, _addr(A), A.stride(0), A.stride(1), _addr(lens_dev), _addr(commit)
    try:
        ngram = isinstance(fusion, _lib.BeamNgram)
        if ilm is not None:
            entry = "rnnt_hip_beam_sync_stream_chunk_ilm"
            check(_lib.lib().rnnt_hip_beam_sync_stream_chunk_ilm(
                C.byref(d), C.byref(fusion) if fusion is not None and not ngram else None, C.byref(fusion) if ngram else None,
                C.byref(ilm), C.byref(tm) if tm is not None else None, _stream()), entry)
        else:
            entry = "rnnt_hip_beam_sync_stream_chunk_ngram" if ngram else "rnnt_hip_beam_sync_stream_chunk"
            check(getattr(_lib.lib(), entry)(C.byref(d), C.byref(fusion) if fusion is not None else None,
                                             C.byref(tm) if tm is not None else None, _stream()), entry)
    finally:
        d.T, d.A, d.lens, d.commit = 0, None, None, None
