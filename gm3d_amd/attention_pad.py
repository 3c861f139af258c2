"""Attention of the block stacks (fused.py) above 128 tokens per cloud at head_dim 64: the flash-style kernels of csrc/attention_masked.hip
with no mask, the streaming kernels of csrc/attention_long.hip from 513 tokens -- and the lengths neither takes in bf16.

bf16, head_dim 64: the flash-style kernels keep a head's K and V (backward: Q, K, V, dO) in LDS, which holds 480 tokens forward and 256
backward; the streaming kernels start at 513.  The lengths in between (a GeoMask3D model of 257..512 groups: its teacher and its decoders
see every token) run on the streaming kernels at PAD_T = 513 rows, the rows past T zero and blocked as keys by a constant mask bitset.
A padded query row attends to the real keys and is dropped; in the backward its dO is zero, so it adds exact zeros to dK and dV.
Every length the flash-style kernels take stays on them, with the bits it had: a forward of up to 480 tokens keeps its (B,H,T) lse, and
the backward pads it with zeros (p = exp(0 - 0) of a padded row stays finite, and meets dO = 0).
The C entry points and ops.attention_masked are untouched: they refuse what they refused."""
import torch

from .ops import _DT, _ptr, _stream, launch_masked_attention, pack_mask

PAD_T = 513
_pad_bits = {}


def lds_fits(T, dtype, backward):
    """does a kernel take (T, head_dim 64, dtype) as it is: the LDS-resident form, or the streaming form from PAD_T on"""
    return dtype != torch.bfloat16 or T <= (256 if backward else 480) or T >= PAD_T


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


def _dims(qkv, B, T, H):
    return {"B": B, "T": T, "H": H, "HD": 64, "dtype": str(qkv.dtype)}


def forward(qkv, out, lse, B, T, H, scale):
    """qkv (B*T, 3*H*64) -> out (B*T, H*64), filled; returns (out, lse): the given (B,H,T) lse, or a (B,H,PAD_T) one on the padded route"""
    if lds_fits(T, qkv.dtype, False):
        launch_masked_attention(False, _dims(qkv, B, T, H), _ptr(qkv), None, _ptr(out), _ptr(lse), B, T, H, 64, float(scale),
                                _DT[qkv.dtype], _stream())
        return out, lse
    qp, bits = _pad(qkv, B, T), _key_bits(B, T, qkv.device)       # named: each lives until the launch is queued
    op = torch.zeros(B, PAD_T, H * 64, dtype=qkv.dtype, device=qkv.device)
    lp = torch.zeros(B, H, PAD_T, dtype=torch.float32, device=qkv.device)
    launch_masked_attention(False, _dims(qkv, B, PAD_T, H), _ptr(qp), _ptr(bits), _ptr(op), _ptr(lp), B, PAD_T, H, 64, float(scale),
                            _DT[qkv.dtype], _stream())
    out.view(B, T, H * 64).copy_(op[:, :T])
    return out, lp


def backward(qkv, out, dout, lse, dqkv, B, T, H, scale):
    """-> dqkv (B*T, 3*H*64), filled; lse as forward() returned it"""
    if lds_fits(T, qkv.dtype, True):
        launch_masked_attention(True, _dims(qkv, B, T, H), _ptr(qkv), None, _ptr(out), _ptr(dout), _ptr(lse), _ptr(dqkv), B, T, H, 64,
                                float(scale), _DT[qkv.dtype], _stream())
        return dqkv
    lp = lse if lse.shape[-1] == PAD_T else _pad(lse, B, T)
    qp, op, dop, bits = _pad(qkv, B, T), _pad(out, B, T), _pad(dout, B, T), _key_bits(B, T, qkv.device)
    dq = torch.zeros(B, PAD_T, qkv.shape[-1], dtype=qkv.dtype, device=qkv.device)
    launch_masked_attention(True, _dims(qkv, B, PAD_T, H), _ptr(qp), _ptr(bits), _ptr(op), _ptr(dop), _ptr(lp), _ptr(dq), B, PAD_T, H, 64,
                            float(scale), _DT[qkv.dtype], _stream())
    dqkv.view(B, T, -1).copy_(dq[:, :T])
    return dqkv
