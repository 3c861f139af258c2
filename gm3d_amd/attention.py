"""Which kernel runs attention, and the one place that launches it.

Four launches compute softmax(Q K^T * scale [masked]) V on a (B*T, 3*H*hd) qkv (timm layout (B,T,3,H,hd)), and `route` names the one a
length takes:

    head     gm3d_attention_fwd / _bwd          csrc/attention.hip         one workgroup per (cloud, head), the whole head in LDS: T <= 128,
                                                                           head_dim 64, no mask
    flash    gm3d_attention_masked_fwd / _bwd   csrc/attention_masked.hip  a head's K, V (backward: Q, K, V, dO) resident in LDS: T <= 512
    stream   gm3d_attention_long_fwd / _bwd     csrc/attention_long.hip    K, V streamed through: 513 <= T <= 2048
    stream at PAD_T = 513 rows                                             the lengths the flash kernels' LDS does not hold in bf16

and a fifth, gm3d_attention_qkv_fwd, forms q|k|v from the block's LayerNorm output inside the head kernel (`route_qkv`, `qkv_fwd`).

The padded form: in bf16 at head_dim 64 the flash kernels' LDS holds 480 tokens forward and 256 backward, and the streaming kernels start
at 513.  The lengths in between (a GeoMask3D model of 257..512 groups: its teacher and its decoders see every token) run on the streaming
kernels at PAD_T rows, the rows past T zero and blocked as keys by a constant mask bitset.  A padded query row attends to the real keys
and is dropped; in the backward its dO is zero, so it adds exact zeros to dK and dV.  A forward of up to 480 tokens keeps its (B,H,T)
lse, and the backward pads it with zeros (p = exp(0 - 0) of a padded row stays finite, and meets dO = 0); a padded forward hands its
(B,H,PAD_T) lse to the backward as it is.

A caller states `head` (may the whole-head kernel run) and `pad` (may the padded form) and holds no predicate of its own.  What the C
entry points refuse is not refused here: the launch is made and the guard answers.
"""
import torch

from ._capi import lib
from .ops import _DT, _launch, _ptr, _require, _stream, pack_mask      # ops imports this module at its end

PAD_T = 513
_pad_bits = {}


def route(T, hd, dtype, masked, backward, head=True, pad=False):
    """-> (family, rows of the launch): ("head", T), ("flash", T), ("stream", T), or ("stream", PAD_T) for the padded form"""
    if head and not masked and hd == 64 and T <= 128:
        return "head", T
    if pad and not masked and hd == 64 and dtype is torch.bfloat16 and (256 if backward else 480) < T < PAD_T:
        return "stream", PAD_T
    return ("stream" if T > 512 else "flash"), T


def _key_bits(B, T, device):
    """(B,PAD_T,ceil(PAD_T/32)) int32: keys >= T blocked for every query (ops.pack_mask layout); cached per shape, outside capture only
    (a tensor first made inside a capture lives in the graph's pool and holds nothing until the first replay)"""
    key = (B, T, device.type, device.index)
    bits = _pad_bits.get(key)
    if bits is None:
        blocked = (torch.arange(PAD_T, device=device) >= T).view(1, 1, PAD_T).expand(1, PAD_T, PAD_T)
        bits = pack_mask(blocked).expand(B, -1, -1).contiguous()
        if not (device.type == "cuda" and torch.cuda.is_current_stream_capturing()):
            _pad_bits[key] = bits
    return bits


def _pad(x, B, T):
    """(B*T, C) rows or a (B,H,T) lse -> the same with T padded to PAD_T by zeros"""
    if x.dim() == 3:
        p = torch.zeros(B, x.shape[1], PAD_T, dtype=x.dtype, device=x.device)
        p[:, :, :T] = x
        return p
    p = torch.zeros(B, PAD_T, x.shape[-1], dtype=x.dtype, device=x.device)
    p[:, :T] = x.view(B, T, -1)
    return p


def _run(family, backward, qkv, bits, rest, B, T, H, hd, scale):
    """the one launch: `rest` = the tensors between the mask and the sizes (out, lse | out, dout, lse, dqkv)"""
    way = "bwd" if backward else "fwd"
    if family == "head":
        name = "gm3d_attention_" + way
        _launch(name, {"B": B, "T": T, "H": H, "dtype": str(qkv.dtype)}, getattr(lib, name), _ptr(qkv), *[_ptr(t) for t in rest],
                B, T, H, float(scale), _DT[qkv.dtype], _stream())
    else:
        name = "gm3d_attention_%s_%s" % ("long" if family == "stream" else "masked", way)
        _launch(name, {"B": B, "T": T, "H": H, "HD": hd, "dtype": str(qkv.dtype)}, getattr(lib, name), _ptr(qkv), _ptr(bits),
                *[_ptr(t) for t in rest], B, T, H, hd, float(scale), _DT[qkv.dtype], _stream())


def fwd(qkv, bits, B, T, H, hd, scale, out=None, head=True, pad=False):
    """qkv (B*T, 3*H*hd), bits (ops.pack_mask) | None -> (out (B*T, H*hd), lse (B,H,T) f32 -- (B,H,PAD_T) from the padded form)"""
    if out is None:
        out = torch.empty(B * T, H * hd, dtype=qkv.dtype, device=qkv.device)
    family, rows = route(T, hd, qkv.dtype, bits is not None, False, head, pad)
    if rows == T:
        lse = torch.empty(B, H, T, dtype=torch.float32, device=qkv.device)
        _run(family, False, qkv, bits, (out, lse), B, T, H, hd, scale)
        return out, lse
    qp, kb = _pad(qkv, B, T), _key_bits(B, T, qkv.device)       # named: each lives until the launch is queued
    op = torch.zeros(B, PAD_T, H * hd, dtype=qkv.dtype, device=qkv.device)
    lp = torch.zeros(B, H, PAD_T, dtype=torch.float32, device=qkv.device)
    _run(family, False, qp, kb, (op, lp), B, PAD_T, H, hd, scale)
    out.view(B, T, H * hd).copy_(op[:, :T])
    return out, lp


def bwd(qkv, bits, out, dout, lse, B, T, H, hd, scale, dqkv=None, head=True, pad=False):
    """-> dqkv (B*T, 3*H*hd); lse as fwd returned it"""
    if dqkv is None:
        dqkv = torch.empty_like(qkv)
    family, rows = route(T, hd, qkv.dtype, bits is not None, True, head, pad)
    if rows == T:
        _run(family, True, qkv, bits, (out, dout, lse, dqkv), B, T, H, hd, scale)
        return dqkv
    lp = lse if lse.shape[-1] == PAD_T else _pad(lse, B, T)
    qp, op, dop, kb = _pad(qkv, B, T), _pad(out, B, T), _pad(dout, B, T), _key_bits(B, T, qkv.device)
    dq = torch.zeros(B, PAD_T, qkv.shape[-1], dtype=qkv.dtype, device=qkv.device)
    _run(family, True, qp, kb, (op, dop, lp, dq), B, PAD_T, H, hd, scale)
    dqkv.view(B, T, -1).copy_(dq[:, :T])
    return dqkv


# ----------------------------------------------------------------------------- qkv projection + attention in one launch
def qkv_supported(h, wqkv, T, H):
    """what gm3d_attention_qkv_fwd takes: bf16, T <= 64, C = 384 = H * 64, dense 16-byte aligned operands"""
    return (h.is_cuda and h.dtype == torch.bfloat16 and wqkv.dtype == torch.bfloat16 and T <= 64 and h.shape[1] == 384 == H * 64
            and h.is_contiguous() and wqkv.is_contiguous() and tuple(wqkv.shape) == (1152, 384)
            and h.data_ptr() % 16 == 0 and wqkv.data_ptr() % 16 == 0)


def route_qkv(h, wqkv, T, H, fuse):
    """does the qkv-fused launch run this block: where the kernel takes it, above 32 tokens.  fuse: the caller's switch
    (fused.FUSE_QKV_ATTENTION)"""
    return fuse and T > 32 and qkv_supported(h, wqkv, T, H)


def qkv_fwd(h, wqkv, B, T, H, scale, out=None, want_qkv=False, want_lse=False):
    """qkv projection + attention in one launch (csrc/attention.hip attn_qkv_fwd_bf16_kernel); returns (out, lse|None, qkv|None)."""
    C = h.shape[1]
    if out is None:
        out = torch.empty(B * T, C, dtype=h.dtype, device=h.device)
    lse = torch.empty(B, H, T, dtype=torch.float32, device=h.device) if want_lse else None
    qkv = torch.empty(B * T, 3 * C, dtype=h.dtype, device=h.device) if want_qkv else None
    _launch("gm3d_attention_qkv_fwd", {"B": B, "T": T, "H": H, "C": C, "dtype": str(h.dtype)}, lib.gm3d_attention_qkv_fwd, _ptr(h),
            _ptr(wqkv), _ptr(out), _ptr(lse) if want_lse else None, _ptr(qkv) if want_qkv else None, B, T, H, C, float(scale),
            _DT[h.dtype], _stream())
    return out, lse, qkv


# ----------------------------------------------------------------------------- the autograd node under ops.attention / attention_masked
class AttentionFn(torch.autograd.Function):
    """args: qkv (B,T,3*H*hd), bits | None, num_heads, scale, head, hd64.  hd64: ops.attention's contract -- head_dim 64, which it
    has only ever checked where the whole-head kernel runs."""

    @staticmethod
    def forward(ctx, qkv, bits, num_heads, scale, head, hd64):
        qkv = qkv.contiguous()
        if qkv.dtype not in _DT:
            raise RuntimeError("attention supports float32 and bfloat16, got %s" % qkv.dtype)
        _require(qkv, None, "qkv")
        B, T, C3 = qkv.shape
        if hd64 and route(T, 64, qkv.dtype, bits is not None, False, head)[0] == "head":
            hd = 64
            if C3 != 3 * num_heads * 64:
                raise RuntimeError("qkv last dim must be 3*num_heads*64")
        else:
            hd = C3 // (3 * num_heads)
            if C3 != 3 * num_heads * hd or hd not in (16, 32, 64):
                raise RuntimeError("qkv last dim must be 3*num_heads*head_dim with head_dim 16, 32 or 64")
            if bits is not None and (bits.dtype != torch.int32 or tuple(bits.shape) != (B, T, (T + 31) // 32)
                                     or not bits.is_contiguous() or not bits.is_cuda):
                raise RuntimeError("mask bitset must be a contiguous int32 (B,T,ceil(T/32)) GPU tensor (ops.pack_mask)")
        qkv = qkv.view(B * T, C3)
        out, lse = fwd(qkv, bits, B, T, num_heads, hd, scale, head=head)
        ctx.save_for_backward(qkv, out, lse, bits)
        ctx.dims = (B, T, num_heads, hd, float(scale), head)
        return out.view(B, T, num_heads * hd)

    @staticmethod
    def backward(ctx, dout):
        qkv, out, lse, bits = ctx.saved_tensors
        B, T, H, hd, scale, head = ctx.dims
        dout = dout.contiguous().to(qkv.dtype)
        return bwd(qkv, bits, out, dout, lse, B, T, H, hd, scale, head=head).view(B, T, -1), None, None, None, None, None
