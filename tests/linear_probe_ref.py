"""Restatement of the linear probe (Point-MAE_SA3D/main_linprob.py:219-263) with torch modules on the CPU, float64 by default:
BatchNorm1d(affine=False, eps=1e-6) -> Linear, cross_entropy, SGD(momentum, weight decay 0), the rate of util/lr_sched.
adjust_learning_rate at epoch + it / iterations_per_epoch, consecutive batches of the given orders with drop_last=True, evaluation
over ALL test rows with the classes ranked by (logit descending, class ascending).  dtype=torch.float32 runs the same in fp32 (the
rates are rounded to fp32 in both, as the GPU path holds them)."""
import math

import numpy as np
import torch


def learning_rates(epochs, ipe, lr, min_lr, warmup_epochs, adjust=None):
    """The rate of every iteration, rounded to fp32.  adjust: the reference's own adjust_learning_rate(optimizer, epoch, args)."""
    out = []
    for e in range(epochs):
        for it in range(ipe):
            x = e + it / ipe
            if adjust is not None:
                class A:
                    pass
                a = A()
                a.lr, a.min_lr, a.warmup_epochs, a.epochs = lr, min_lr, warmup_epochs, epochs
                group = {"lr": None}
                opt = A()
                opt.param_groups = [group]
                v = adjust(opt, x, a)
                assert group["lr"] == v
            elif x < warmup_epochs:
                v = lr * x / warmup_epochs
            else:
                v = min_lr + (lr - min_lr) * 0.5 * (1.0 + math.cos(math.pi * (x - warmup_epochs) / (epochs - warmup_epochs)))
            out.append(v)
    return np.asarray(out, np.float64).astype(np.float32)


def default_orders(n, epochs, seed):
    """DistributedSampler(range(n), 1, 0, shuffle=True, seed) after set_epoch(e): randperm on a CPU generator seeded seed + e."""
    return [torch.randperm(n, generator=torch.Generator().manual_seed(seed + e)).tolist() for e in range(epochs)]


def evaluate(Q, yq, W, b, running_mean, running_var, eps=1e-6):
    """-> (top-1 hits, top-min(5, C) hits, gap12 (m), gap56 (m)): the logit gaps at ranks 1|2 and 5|6 (inf without such a boundary)."""
    z = ((Q - running_mean) / torch.sqrt(running_var + eps)) @ W.T + b
    z = z.double().numpy() + 0.0
    m, C = z.shape
    ranking = np.argsort(-z, axis=1, kind="stable")                # stable: equal logits stay in ascending class order
    ranked = np.take_along_axis(z, ranking, 1)
    hit = ranking == np.asarray(yq).reshape(-1, 1)
    lim = min(5, C)
    gap12 = ranked[:, 0] - ranked[:, 1]
    gap56 = ranked[:, 4] - ranked[:, 5] if C > 5 else np.full(m, np.inf)
    return int(hit[:, :1].sum()), int(hit[:, :lim].sum()), gap12, gap56


def fit(X, y, Q, yq, num_classes, weight, orders, batch, epochs, warmup_epochs, lr, min_lr=0.0, momentum=0.9, eval_every=1,
        dtype=torch.float64, rates=None):
    """X (n,d), Q (m,d) float arrays, y, yq int arrays, weight (C,d) the initial weights, orders: `epochs` lists of row indices.
    -> dict: weight, bias, running_mean, running_var, losses (numpy, float64), eval_epochs, hits [(top-1, top-5)], min_gap [(1|2, 5|6)]
    and row_gaps [(m) the smaller of the two gaps per test row] per evaluated epoch."""
    X, Q = torch.as_tensor(np.asarray(X)).to(dtype), torch.as_tensor(np.asarray(Q)).to(dtype)
    y = torch.as_tensor(np.asarray(y)).long()
    n, d = X.shape
    ipe = n // batch
    if rates is None:
        rates = learning_rates(epochs, ipe, lr, min_lr, warmup_epochs)
    bn = torch.nn.BatchNorm1d(d, affine=False, eps=1e-6).to(dtype)
    lin = torch.nn.Linear(d, num_classes).to(dtype)
    with torch.no_grad():
        lin.weight.copy_(torch.as_tensor(np.asarray(weight)).to(dtype))
        lin.bias.zero_()
    head = torch.nn.Sequential(bn, lin)
    opt = torch.optim.SGD(lin.parameters(), lr=float(rates[0]), momentum=momentum, weight_decay=0)
    losses, hits, gaps, row_gaps, evals = [], [], [], [], []
    t = 0
    for e in range(epochs):
        head.train()
        rows = torch.as_tensor(list(orders[e])[:ipe * batch]).long()
        for it in range(ipe):
            for g in opt.param_groups:
                g["lr"] = float(rates[t])
            b = rows[it * batch:(it + 1) * batch]
            loss = torch.nn.functional.cross_entropy(head(X[b]), y[b])
            opt.zero_grad()
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
            t += 1
        if Q is not None and Q.shape[0] and ((e + 1) % eval_every == 0 or e + 1 == epochs):
            with torch.no_grad():
                h1, h5, g12, g56 = evaluate(Q, yq, lin.weight, lin.bias, bn.running_mean, bn.running_var)
            evals.append(e + 1)
            hits.append((h1, h5))
            gaps.append((float(g12.min()), float(g56.min())))
            row_gaps.append(np.minimum(g12, g56))
    return {"weight": lin.weight.detach().double().numpy(), "bias": lin.bias.detach().double().numpy(),
            "running_mean": bn.running_mean.double().numpy(), "running_var": bn.running_var.double().numpy(),
            "losses": np.asarray(losses, np.float64), "eval_epochs": evals, "hits": hits, "min_gap": gaps, "row_gaps": row_gaps}


def rel_err(a, ref):
    """max |a - ref| / max |ref|, the project's parity measure (README "Parity")."""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-300))


def features(n, m, d, num_classes, seed, offset=3.0, pool=None):
    """Seeded, weakly clustered features: per-column scales 0.5 .. 2, an offset, one all-zero column (column 1).
    -> X (n,d) f32, y (n), Q (pool or m, d) f32, yq."""
    g = torch.Generator().manual_seed(seed)
    centres = torch.randn(num_classes, d, generator=g)
    scale = 0.5 + 1.5 * torch.rand(d, generator=g)

    def rows(cnt):
        lab = torch.arange(cnt) % num_classes
        x = (0.25 * centres[lab] + torch.randn(cnt, d, generator=g)) * scale + offset
        x[:, 1] = 0.0
        return x.float().numpy(), lab.numpy().astype(np.int64)
    X, y = rows(n)
    Q, yq = rows(pool or m)
    return X, y, Q, yq


MIN_GAP = 1e-3


def initial_weight(num_classes, d, seed):
    """main_linprob.py:219: trunc_normal_(std=0.01), on a CPU generator seeded with `seed` (what LinearProbe.fit draws)."""
    w = torch.empty(num_classes, d, dtype=torch.float32)
    torch.nn.init.trunc_normal_(w, std=0.01, generator=torch.Generator().manual_seed(seed))
    return w.numpy()


def peak_lr(batch, blr=0.1):
    return blr * batch / 256


def select_rows(X, y, Qpool, ypool, m, num_classes, weight, orders, batch, epochs, warmup_epochs, lr, rates=None):
    """The first m rows of the pool whose float64 logits keep a gap above MIN_GAP at ranks 1|2 and 5|6 at every evaluated epoch
    from the second on (the only epoch, when there is one)."""
    res = fit(X, y, Qpool, ypool, num_classes, weight, orders, batch, epochs, warmup_epochs, lr, rates=rates)
    keep = np.ones(Qpool.shape[0], bool)
    for e, g in zip(res["eval_epochs"], res["row_gaps"]):
        if e >= min(2, epochs):
            keep &= g > MIN_GAP
    rows = np.nonzero(keep)[0][:m]
    assert rows.size == m, "only %d of %d pool rows are unambiguous" % (rows.size, Qpool.shape[0])
    return rows


_CASES = {}


def case(n, m, d, num_classes, batch, epochs, offset=3.0, seed=0, warmup_epochs=1):
    """Inputs of one GPU case and their float64 / float32 restatements, computed once per process:
    -> dict X, y, Q, yq, weight, orders, lr, ref (float64 fit), ref32 (float32 fit)."""
    key = (n, m, d, num_classes, batch, epochs, offset, seed, warmup_epochs)
    if key not in _CASES:
        X, y, Qpool, ypool = features(n, m, d, num_classes, seed + 17 * n + d, offset, pool=4 * m)
        weight, orders, lr = initial_weight(num_classes, d, seed), default_orders(n, epochs, seed), peak_lr(batch)
        rows = select_rows(X, y, Qpool, ypool, m, num_classes, weight, orders, batch, epochs, warmup_epochs, lr)
        Q, yq = np.ascontiguousarray(Qpool[rows]), np.ascontiguousarray(ypool[rows])
        args = (X, y, Q, yq, num_classes, weight, orders, batch, epochs, warmup_epochs, lr)
        _CASES[key] = {"X": X, "y": y, "Q": Q, "yq": yq, "weight": weight, "orders": orders, "lr": lr, "warmup_epochs": warmup_epochs,
                       "ref": fit(*args), "ref32": fit(*args, dtype=torch.float32)}
    return _CASES[key]


# n, m, d, C, batch, epochs, offset: the GPU cases (tests/test_gpu_linear_probe.py) and the fp32 headroom check on their inputs
GPU_CASES = [(200, 96, 72, 40, 48, 3, 3.0), (200, 96, 72, 40, 48, 3, 50.0), (130, 64, 8, 2, 33, 4, 3.0), (1100, 300, 384, 40, 512, 2, 3.0),
             (2048, 64, 1024, 64, 1024, 1, 3.0)]
TENSORS = ("weight", "bias", "running_mean", "running_var", "losses")
BAR = 1e-5                                                         # README "Parity"

# the committed fixture (tests/golden/make_golden_linear_probe.py)
FIXTURE = {"n": 640, "m": 256, "d": 384, "num_classes": 40, "batch": 100, "epochs": 6, "warmup_epochs": 2, "seed": 0, "pool": 1024,
           "feature_seed": 20240}


def fixture_inputs():
    f = FIXTURE
    X, y, Qpool, ypool = features(f["n"], f["m"], f["d"], f["num_classes"], f["feature_seed"], 3.0, pool=f["pool"])
    return X, y, Qpool, ypool, initial_weight(f["num_classes"], f["d"], f["seed"]), default_orders(f["n"], f["epochs"], f["seed"])
