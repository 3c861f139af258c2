"""float64 numpy restatement of the weighted k-NN probe (main_knn.py::knn_classifier) with the project's tie rules:
neighbours by (similarity descending, training row ascending), classes by (score descending, class ascending).
Beside the result it reports, per test row, how far the row is from an ambiguity: the similarity gap at the k | k+1 boundary and
the relative score margins at ranks 1|2 and 5|6 (inf where there is no such boundary)."""
import numpy as np


def neighbours(train, test, k):
    """-> idx (m,k) int64, sim (m,k) f64, gap (m) f64 = sim[k-1] - sim[k] of the full ranking (inf when k == n)."""
    S = np.asarray(test, np.float64) @ np.asarray(train, np.float64).T
    S = S + 0.0                                                    # -0 -> +0
    order = np.argsort(-S, axis=1, kind="stable")                  # stable: equal similarities stay in ascending row order
    ranked = np.take_along_axis(S, order, 1)
    n = S.shape[1]
    gap = ranked[:, k - 1] - ranked[:, k] if k < n else np.full(S.shape[0], np.inf)
    return order[:, :k], ranked[:, :k], gap


def _margin(s, a):
    """relative margin between ranks a and a+1 (0-based a-1 | a) of the descending scores s (m,C)."""
    if s.shape[1] <= a:
        return np.full(s.shape[0], np.inf)
    hi, lo = s[:, a - 1], s[:, a]
    return np.where(hi > 0, (hi - lo) / np.where(hi > 0, hi, 1.0), np.inf)    # two unvoted classes: an exact tie, decided by the rule


def knn_classifier(train, train_labels, test, test_labels, k, T, num_classes):
    """-> dict: top1, top5 (percent), idx, sim, gap, probs (m,C) f64, ranking (m,C) class ids, voted (m) classes with a neighbour,
    margin12, margin56 (m)."""
    train_labels = np.asarray(train_labels).reshape(-1)
    test_labels = np.asarray(test_labels).reshape(-1)
    idx, sim, gap = neighbours(train, test, k)
    m = idx.shape[0]
    w = np.exp(sim / T)
    lab = train_labels[idx]
    probs = np.zeros((m, num_classes))
    for j in range(k):                                             # neighbour-rank order
        np.add.at(probs, (np.arange(m), lab[:, j]), w[:, j])
    ranking = np.argsort(-probs, axis=1, kind="stable")            # stable: equal scores stay in ascending class order
    ranked = np.take_along_axis(probs, ranking, 1)
    hit = ranking == test_labels[:, None]
    lim = min(5, k, num_classes)
    return {
        "top1": hit[:, :1].sum() * 100.0 / max(m, 1),
        "top5": hit[:, :lim].sum() * 100.0 / max(m, 1),
        "idx": idx, "sim": sim, "gap": gap, "probs": probs, "ranking": ranking,
        "voted": (probs > 0).sum(1),
        "margin12": _margin(ranked, 1), "margin56": _margin(ranked, 5),
    }
