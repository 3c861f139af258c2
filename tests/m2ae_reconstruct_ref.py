"""Not a test: gm3d_reconstruct_partition restated in aten (pure torch, CPU or GPU) -- a stable argsort of the mask, gathers along it,
torch.where on the gathered mask, one fp32 add.  The launch must equal it bit for bit."""
import torch


def _take(x, order):
    """x (B,G,...) gathered along dim 1 by order (B,G) int64"""
    tail = x.shape[2:]
    return torch.gather(x, 1, order.reshape(order.shape + (1,) * len(tail)).expand(order.shape + tail))


def partition(pred, neighborhood, center, masked):
    """pred (B,G,3k) f32 / bf16 or None, neighborhood (B,G,k,3) f32, center (B,G,3) f32, masked (B,G) bool / uint8 (non-zero = masked)
    -> (dense (B,G*k,3) f32, full_center (B,G,3) f32, order (B,G) int32, n_visible (B,) int32)."""
    B, G, k, _ = neighborhood.shape
    m = masked != 0
    order = torch.argsort(m.to(torch.uint8), dim=1, stable=True)           # visible tokens first, each part in ascending token index
    src = _take(neighborhood, order)
    if pred is not None:
        src = torch.where(_take(m, order).view(B, G, 1, 1), _take(pred.float().reshape(B, G, k, 3), order), src)
    c = _take(center, order)
    dense = src + c.unsqueeze(2)                                           # the one fp32 add
    return dense.reshape(B, G * k, 3), c, order.to(torch.int32), (~m).sum(1).to(torch.int32)
