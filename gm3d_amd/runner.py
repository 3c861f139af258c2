"""The reference's tester (Point-MAE_SA3D/tools/runner.py:34-113): run a pre-trained Point-MAE with vis=True over a test loader and
write, per kept cloud, the input (gt.txt), its visible patches (vis.txt) and the visible + rebuilt cloud (dense_points.txt).

Same category filter, folder name `{taxonomy_id}_{idx}` and np.savetxt(..., delimiter=';') files.  Differences: batches of any size
are accepted -- the model's flat vis=True layout is split per cloud, one folder each, `idx` the running cloud index over the loader
(the reference's batch index at its batch size 1), the filter applied per batch entry --, and the rendered plot.jpg (matplotlib +
OpenCV) is not produced: the reference's view angles of each category come back in the per-cloud record for whoever renders.

test_m2ae is the same tester for Point-M2AE + GeoMask3D (reconstruct.reconstruct_m2ae): vis.txt holds the cloud's visible level-0
points -- the raw input points the encoder saw, a different number of rows per cloud -- and dense_points.txt its dense level-1 cloud.
"""
import os

import numpy as np
import torch

USEFUL_CATE = (
    "02691156",  # plane
    "04379243",  # table
    "03790512",  # motorbike
    "03948459",  # pistol
    "03642806",  # laptop
    "03467517",  # guitar
    "03261776",  # earphone
    "03001627",  # chair
    "02958343",  # car
    "04090263",  # rifle
    "03759954",  # microphone
)
# the (a, b) the reference passes to misc.get_ptcloud_img; every other category is drawn at (0, 0)
VIEW_ANGLES = {"02691156": (90, 135), "04379243": (30, 30), "03642806": (30, -45), "03467517": (0, 90), "03261776": (0, 75),
               "03001627": (30, -45)}


def split_flat(ret1, ret2, B):
    """The vis=True pair of a batch of B clouds -- ret1 (1,B*G*k,3) = [all visible patches | all rebuilt patches], ret2 (1,B*V*k,3) its
    head -- -> (dense (B,G*k,3) with cloud b = [its visible | its rebuilt], vis (B,V*k,3))."""
    nv, nd = ret2.shape[1], ret1.shape[1]
    if nv % B or (nd - nv) % B:
        raise ValueError("a vis=True pair of %d and %d rows does not split over %d clouds" % (nd, nv, B))
    vis = ret2.reshape(B, nv // B, 3)
    rebuilt = ret1[:, nv:].reshape(B, (nd - nv) // B, 3)
    return torch.cat([vis, rebuilt], dim=1), vis


def _device_of(model):
    try:
        return next(model.parameters()).device
    except (AttributeError, StopIteration, TypeError):
        return None


@torch.no_grad()
def test(base_model, test_dataloader, out_dir="./vis", useful_cate=USEFUL_CATE, max_idx=1500, bf16=False):
    """The loader yields (taxonomy_ids, model_ids, points (B,N,3)) like the reference's ShapeNet test loader.  The points are moved to
    the model's device.  -> one record per written cloud: {"idx", "taxonomy_id", "model_id", "path", "view": (a, b)}.  Stops after
    the first written cloud whose idx exceeds max_idx (P/tools/runner.py:110)."""
    base_model.eval()
    dev = _device_of(base_model)
    records, idx = [], 0
    for taxonomy_ids, model_ids, data in test_dataloader:
        B = data.shape[0]
        keep = [b for b in range(B) if taxonomy_ids[b] in useful_cate]
        first, idx = idx, idx + B
        if not keep:
            continue
        points = data if dev is None else data.to(dev)
        with torch.autocast(points.device.type, dtype=torch.bfloat16, enabled=bf16):
            dense_points, vis_points, _ = base_model(points, vis=True)
        dense, vis = split_flat(dense_points.detach().float(), vis_points.detach().float(), B)
        gt, dense, vis = points.detach().cpu().numpy(), dense.cpu().numpy(), vis.cpu().numpy()
        for b in keep:
            data_path = os.path.join(out_dir, "%s_%d" % (taxonomy_ids[b], first + b))
            os.makedirs(data_path, exist_ok=True)
            np.savetxt(os.path.join(data_path, "gt.txt"), gt[b], delimiter=";")
            np.savetxt(os.path.join(data_path, "vis.txt"), vis[b], delimiter=";")
            np.savetxt(os.path.join(data_path, "dense_points.txt"), dense[b], delimiter=";")
            records.append({"idx": first + b, "taxonomy_id": taxonomy_ids[b], "model_id": model_ids[b], "path": data_path,
                            "view": VIEW_ANGLES.get(taxonomy_ids[b], (0, 0))})
            if first + b > max_idx:
                return records
    return records


@torch.no_grad()
def test_m2ae(model, teacher, test_dataloader, out_dir, epoch, total_epoch, useful_cate=USEFUL_CATE, max_idx=1500, bf16=False):
    """`test` for the hierarchical model: the student `model` and its EMA `teacher` (module or ModelEma; None is refused by
    reconstruct_m2ae, which then needs a mask) through reconstruct.reconstruct_m2ae(model, points, teacher, epoch, total_epoch) per
    kept batch.  Same loader triple, category filter per batch entry, running idx, folder names, files and records as `test`."""
    from . import reconstruct
    dev = _device_of(model)
    records, idx = [], 0
    for taxonomy_ids, model_ids, data in test_dataloader:
        B = data.shape[0]
        keep = [b for b in range(B) if taxonomy_ids[b] in useful_cate]
        first, idx = idx, idx + B
        if not keep:
            continue
        points = data if dev is None else data.to(dev)
        r = reconstruct.reconstruct_m2ae(model, points, teacher, epoch, total_epoch, bf16=bf16)
        k0 = r.points0.shape[1] // r.masks[0].shape[1]
        rows0 = (r.n_visible0.cpu().numpy().astype(np.int64) * k0).tolist()       # the one read of the ragged counts, outside the pass
        gt, dense, points0 = points.detach().cpu().numpy(), r.dense.float().cpu().numpy(), r.points0.float().cpu().numpy()
        for b in keep:
            data_path = os.path.join(out_dir, "%s_%d" % (taxonomy_ids[b], first + b))
            os.makedirs(data_path, exist_ok=True)
            np.savetxt(os.path.join(data_path, "gt.txt"), gt[b], delimiter=";")
            np.savetxt(os.path.join(data_path, "vis.txt"), points0[b, :rows0[b]], delimiter=";")
            np.savetxt(os.path.join(data_path, "dense_points.txt"), dense[b], delimiter=";")
            records.append({"idx": first + b, "taxonomy_id": taxonomy_ids[b], "model_id": model_ids[b], "path": data_path,
                            "view": VIEW_ANGLES.get(taxonomy_ids[b], (0, 0))})
            if first + b > max_idx:
                return records
    return records
