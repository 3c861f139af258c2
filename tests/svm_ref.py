"""Float64 numpy restatement of the device SVM (gm3d_amd/csrc/svm.hip): libsvm's C-SVC one-vs-one without shrinking.

Test infrastructure only.  The SMO below performs the same floating-point operations in the same order as the kernel, so given the
same Gram matrix it follows the same path: the same working sets, the same iteration counts and the same alpha.
"""
import numpy as np

TAU = 1e-12


def pairs(ncls):
    return [(s, t) for s in range(ncls) for t in range(s + 1, ncls)]


def smo_pair(Kp, ns, C=0.01, tol=1e-3, max_iter=0):
    """Kp (m,m) Gram of one pair (rows of s with y=+1, then rows of t with y=-1) -> (alpha, rho, iterations, capped)."""
    m = Kp.shape[0]
    y = np.where(np.arange(m) < ns, 1.0, -1.0)
    pos = y > 0
    alpha = np.zeros(m)
    G = -np.ones(m)
    Kd = np.diag(Kp).copy()
    cap = max_iter if max_iter > 0 else max(10_000_000, 100 * m)
    it, capped = 0, False
    while True:
        if it >= cap:
            capped = True
            break
        yg = y * G
        up = np.where(pos, alpha < C, alpha > 0)
        low = np.where(pos, alpha > 0, alpha < C)
        if not up.any() or not low.any():
            break
        cand = np.where(up, -yg, -np.inf)
        i = int(np.argmax(cand))                       # first maximum: ties to the lowest row
        Gmax = cand[i]
        Gmax2 = yg[low].max()
        if not (Gmax + Gmax2 >= tol):
            break
        Ki = Kp[i]
        b = Gmax + yg
        ok = low & (b > 0)
        if not ok.any():
            break
        quad = Kd[i] + Kd - 2.0 * Ki
        quad = np.where(quad <= 0, TAU, quad)
        obj = np.where(ok, -(b * b) / quad, np.inf)
        j = int(np.argmin(obj))
        yi, yj = y[i], y[j]
        Kii, Kjj = Kd[i], Kd[j]
        Qij = yi * yj * Kp[i, j]
        aio, ajo, Gi, Gj = alpha[i], alpha[j], G[i], G[j]
        ai, aj = aio, ajo
        if yi != yj:
            q = Kii + Kjj + 2.0 * Qij
            if q <= 0:
                q = TAU
            delta = (-Gi - Gj) / q
            diff = ai - aj
            ai += delta
            aj += delta
            if diff > 0:
                if aj < 0:
                    aj, ai = 0.0, diff
            elif ai < 0:
                ai, aj = 0.0, -diff
            if diff > 0:
                if ai > C:
                    ai, aj = C, C - diff
            elif aj > C:
                aj, ai = C, C + diff
        else:
            q = Kii + Kjj - 2.0 * Qij
            if q <= 0:
                q = TAU
            delta = (Gi - Gj) / q
            s = ai + aj
            ai -= delta
            aj += delta
            if s > C:
                if ai > C:
                    ai, aj = C, s - C
            elif aj < 0:
                aj, ai = 0.0, s
            if s > C:
                if aj > C:
                    aj, ai = C, s - C
            elif ai < 0:
                ai, aj = 0.0, s
        dai, daj = ai - aio, aj - ajo
        qi = (yi * y) * Ki
        qj = (yj * y) * Kp[j]
        G = G + (qi * dai + qj * daj)
        alpha[i], alpha[j] = ai, aj
        it += 1
    yg = y * G
    at_c, at_0 = alpha >= C, alpha <= 0
    free = ~at_c & ~at_0
    if free.any():
        rho = yg[free].sum() / free.sum()
    else:
        ub = np.concatenate([yg[at_c & ~pos], yg[at_0 & pos], [np.inf]]).min()
        lb = np.concatenate([yg[at_c & pos], yg[at_0 & ~pos], [-np.inf]]).max()
        rho = (ub + lb) / 2
    return alpha, rho, it, capped


def kkt_gap(Kp, ns, alpha, C=0.01):
    """Gmax + Gmax2 of libsvm's stopping rule, from alpha alone (the gradient recomputed as Q alpha - 1)."""
    m = Kp.shape[0]
    y = np.where(np.arange(m) < ns, 1.0, -1.0)
    G = y * (Kp @ (y * alpha)) - 1.0
    yg = y * G
    pos = y > 0
    up = np.where(pos, alpha < C, alpha > 0)
    low = np.where(pos, alpha > 0, alpha < C)
    return (-yg[up]).max() + yg[low].max()


class OvO:
    """One-vs-one fit on float64 features; `gram` may be given (class-grouped rows) to share the device's Gram matrix."""

    def __init__(self, C=0.01, tol=1e-3):
        self.C, self.tol = C, tol

    def fit(self, X, labels, gram=None):
        labels = np.asarray(labels)
        self.classes_, inv = np.unique(labels, return_inverse=True)
        order = np.argsort(inv, kind="stable")
        Xg = np.asarray(X, dtype=np.float64)[order]
        counts = np.bincount(inv, minlength=len(self.classes_))
        self.class_start_ = np.concatenate([[0], np.cumsum(counts)])
        K = Xg @ Xg.T if gram is None else gram
        cs = self.class_start_
        self.alpha_, self.rho_, self.n_iter_, self.coef_ = [], [], [], []
        for s, t in pairs(len(self.classes_)):
            rows = np.concatenate([np.arange(cs[s], cs[s + 1]), np.arange(cs[t], cs[t + 1])])
            ns = cs[s + 1] - cs[s]
            a, rho, it, capped = smo_pair(K[np.ix_(rows, rows)], ns, self.C, self.tol)
            assert not capped
            y = np.where(np.arange(len(rows)) < ns, 1.0, -1.0)
            self.alpha_.append(a)
            self.rho_.append(rho)
            self.n_iter_.append(it)
            self.coef_.append((y * a) @ Xg[rows])
        self.coef_ = np.stack(self.coef_)
        self.rho_ = np.array(self.rho_)
        return self

    def predict(self, X):
        dec = np.asarray(X, dtype=np.float64) @ self.coef_.T - self.rho_
        votes = np.zeros((dec.shape[0], len(self.classes_)), dtype=np.int64)
        for p, (s, t) in enumerate(pairs(len(self.classes_))):
            win = np.where(dec[:, p] > 0, s, t)
            np.add.at(votes, (np.arange(dec.shape[0]), win), 1)
        return self.classes_[np.argmax(votes, axis=1)]


def sklearn_coef(clf):
    """sklearn's coef_ / intercept_ in the multi-class sign convention (undoes its flip of the binary problem)."""
    sign = -1.0 if len(clf.classes_) == 2 else 1.0
    return clf.coef_ * sign, clf.intercept_ * sign


# ModelNet40's per-class cloud counts (train 9,843 / test 2,468), the shape of the validation problem
MODELNET40_TRAIN = [626, 106, 515, 173, 572, 335, 64, 197, 889, 167, 79, 138, 200, 109, 200, 149, 171, 155, 145, 124, 149, 284, 465,
                    200, 88, 231, 240, 104, 115, 128, 680, 124, 90, 392, 163, 344, 267, 475, 87, 103]
MODELNET40_TEST = [100, 50, 100, 20, 100, 100, 20, 100, 100, 20, 20, 20, 86, 20, 86, 20, 100, 100, 20, 20, 20, 100, 100, 86, 20, 100,
                   100, 20, 100, 20, 100, 20, 20, 100, 20, 100, 100, 100, 20, 20]


def modelnet40_like(d=384, seed=0, sep=1.0):
    """Synthetic features with ModelNet40's class counts: (Xtr f32, ytr, Xte f32, yte), rows shuffled."""
    rng = np.random.RandomState(seed)
    ncls = len(MODELNET40_TRAIN)
    centres = rng.randn(ncls, d) * sep / np.sqrt(d) * 4.0

    def draw(counts):
        y = rng.permutation(np.repeat(np.arange(ncls), counts))
        return (centres[y] + rng.randn(len(y), d)).astype(np.float32), y.astype(np.int64)

    Xtr, ytr = draw(MODELNET40_TRAIN)
    Xte, yte = draw(MODELNET40_TEST)
    return Xtr, ytr, Xte, yte


def synthetic(n_train, n_test, ncls, d, seed=0, sep=1.0, sizes=None):
    """Labelled Gaussian clusters with uneven class sizes: (Xtr f32, ytr, Xte f32, yte)."""
    rng = np.random.RandomState(seed)
    centres = rng.randn(ncls, d) * sep / np.sqrt(d) * 4.0
    if sizes is None:
        w = rng.gamma(2.0, 1.0, ncls)
        p = w / w.sum()
    else:
        p = np.asarray(sizes, dtype=np.float64) / np.sum(sizes)

    def draw(count):
        y = rng.choice(ncls, count, p=p)
        y[:ncls] = np.arange(ncls)[: min(ncls, count)]
        x = centres[y] + rng.randn(count, d)
        return x.astype(np.float32), y.astype(np.int64)

    Xtr, ytr = draw(n_train)
    Xte, yte = draw(n_test)
    return Xtr, ytr, Xte, yte
