"""numpy restatement of the boosted-tree classifier behind DCI (csrc/gbt.hip, encdiff_amd/metrics.py
dci_score): sklearn's GradientBoostingClassifier with its defaults (log loss, friedman_mse, best
splitter, max_depth 3, subsample 1) as evaluation/metrics/dci.py fits it, with the two decisions of
DESIGN §1 "DCI" that make a run repeatable:

  * trees are grown on Gq = rint(G * 2^32) as int64, so the split statistics are integers, prefix sums
    are exact in any order and the proxy is one fp64 formula of (nL, sL, n, s);
  * features whose best cuts tie are ranked by splitmix64(tie_seed, stage, tree, node, feature), the
    highest priority winning (sklearn visits the features in a random order and keeps the first).

Nodes carry heap ids: the root is 1, the children of i are 2 i and 2 i + 1, depth 3 ends at 8..15;
tables are indexed by id - 1.  feature is -1 at a leaf and -2 where there is no node.

Sums of fp64 values (the sum of squares behind the impurity, the leaf numerators and denominators)
are taken in the kernel's order, block_sum below: thread t of 256 adds the rows t, t + 256, ... and
the 256 partials are folded 128, 64, ..., 1.  The impurity decides whether a node is a leaf, so this
keeps the node tables of the kernel and of this file identical, not merely close.
"""
import numpy as np

EPS32 = float(np.finfo(np.float32).eps)
DBL_EPS = float(np.finfo(np.float64).eps)
CUT = np.float32(1e-7)          # sklearn's FEATURE_THRESHOLD, a float32 added to a float32
SCALE = 4294967296.0            # 2^32
NODES = 15
BLOCK = 256
_M64 = (1 << 64) - 1


def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def tie_priority(tie_seed, stage, tree, node, feature):
    h = splitmix64(int(tie_seed) & _M64)
    for v in (stage, tree, node, feature):
        h = splitmix64(h ^ int(v))
    return h


def block_sum(v):
    """Sums along the last axis in the kernel's order (see the module docstring)."""
    v = np.asarray(v, np.float64)
    n = v.shape[-1]
    rows = -(-n // BLOCK)
    a = np.zeros(v.shape[:-1] + (rows * BLOCK,))
    a[..., :n] = v
    a = a.reshape(v.shape[:-1] + (rows, BLOCK))
    acc = np.zeros(v.shape[:-1] + (BLOCK,))
    for r in range(rows):
        acc = acc + a[..., r, :]
    o = BLOCK // 2
    while o:
        acc = acc[..., :o] + acc[..., o:2 * o]
        o //= 2
    return acc[..., 0]


def init_raw(y, classes):
    """The initial raw predictions of the prior: (1,) for two classes, (C,) otherwise."""
    prior = np.clip(np.bincount(y, minlength=classes) / float(len(y)), EPS32, 1 - EPS32)
    if classes == 2:
        return np.array([np.log(prior[1] / (1 - prior[1]))])
    lp = np.log(prior)
    return lp - np.mean(lp)


def gradients(raw, y, classes):
    """G (T, N) = onehot - P and P (T, N), T = 1 for two classes (the column of class 1)."""
    if classes == 2:
        p = 1.0 / (1.0 + np.exp(-raw[:, 0]))
        return ((y == 1) - p)[None], p[None]
    e = np.exp(raw - raw.max(1, keepdims=True))
    p = e / e.sum(1, keepdims=True)
    onehot = (y[:, None] == np.arange(classes)[None]).astype(np.float64)
    return np.ascontiguousarray((onehot - p).T), np.ascontiguousarray(p.T)


def best_cut(xs, gqs, n, s):
    """The best cut of one feature inside one node: xs, gqs the members in the feature's sorted
    order.  None, or (proxy, x_lo, x_hi, nL, sL); the lowest position wins a tie."""
    ok = xs[1:] > xs[:-1] + CUT
    if not ok.any():
        return None
    nl = np.arange(1, n, dtype=np.int64)
    sl = np.cumsum(gqs)[:-1]
    diff = (n * sl - nl * s).astype(np.float64)
    proxy = diff * diff / (nl.astype(np.float64) * (n - nl).astype(np.float64))
    proxy[~ok] = -np.inf
    j = int(np.argmax(proxy))
    return float(proxy[j]), xs[j], xs[j + 1], int(nl[j]), int(sl[j])


def threshold(x_lo, x_hi):
    thr = np.float32(np.float64(x_lo) / 2.0 + np.float64(x_hi) / 2.0)
    return x_lo if thr == x_hi else thr


def fit_tree(x, xs, order, g, onehot, classes, stage, tree, tie_seed):
    """One depth-3 tree on the gradient column g (fp64) of one class; onehot: 1.0 where the row is of
    that class.  x (N, D) float32; xs, order (D, N): every column sorted (stable) and its
    permutation.  Returns the node tables, the node id of every row and the tree's unnormalised
    importances.  The leaf denominators take p = onehot - g, as sklearn does."""
    n_rows, dims = x.shape
    gq = np.rint(g * SCALE).astype(np.int64)
    gd = gq.astype(np.float64) / SCALE
    p = onehot - g
    pq = p * (1.0 - p)
    node = np.ones(n_rows, np.int64)
    feature = np.full(NODES + 1, -2, np.int32)
    thr = np.zeros(NODES + 1, np.float32)
    count = np.zeros(NODES + 1, np.int32)
    value = np.zeros(NODES + 1, np.float64)
    imp = np.zeros(NODES + 1, np.float64)
    for level in range(4):
        ids = np.arange(2 ** level, 2 ** (level + 1))
        member = node[None, :] == ids[:, None]
        cnt = member.sum(1)
        ssq = block_sum(np.where(member, gd * gd, 0.0))
        sg = block_sum(np.where(member, g, 0.0))
        sp = block_sum(np.where(member, pq, 0.0))
        for j, nd in enumerate(ids):
            n = int(cnt[j])
            if n == 0:
                continue
            m = member[j]
            s = int(gq[m].sum())
            mean = (float(s) / SCALE) / float(n)
            imp[nd] = ssq[j] / float(n) - mean * mean
            count[nd] = n
            best = None
            if level < 3 and n >= 2 and not imp[nd] <= DBL_EPS:
                for f in range(dims):
                    mm = m[order[f]]
                    c = best_cut(xs[f][mm], gq[order[f]][mm], n, s)
                    if c is None:
                        continue
                    prio = tie_priority(tie_seed, stage, tree, nd, f)
                    if best is None or c[0] > best[0][0] or (c[0] == best[0][0] and prio > best[1]):
                        best = (c, prio, f)
            if best is None:
                feature[nd] = -1
                num, den = sg[j] / float(n), sp[j] / float(n)
                if classes > 2:
                    num = num * ((classes - 1.0) / classes)
                value[nd] = 0.0 if abs(den) < 1e-150 else num / den
                continue
            (_, x_lo, x_hi, _, _), _, f = best
            feature[nd], thr[nd] = f, threshold(x_lo, x_hi)
            node[m] = 2 * nd + (x[m, f] > thr[nd])
    importance = np.zeros(dims)
    for nd in range(1, 8):
        if feature[nd] >= 0:
            a, b = 2 * nd, 2 * nd + 1
            importance[feature[nd]] += (float(count[nd]) * imp[nd] - float(count[a]) * imp[a]
                                        - float(count[b]) * imp[b]) / float(n_rows)
    return feature[1:], thr[1:], count[1:], value[1:], node, importance


def apply_tree(feature, thr, value, x):
    """The leaf value of every row of x (tables indexed by id - 1)."""
    node = np.ones(x.shape[0], np.int64)
    for _ in range(3):
        f = feature[node - 1]
        inner = f >= 0
        right = x[np.arange(x.shape[0]), np.where(inner, f, 0)] > thr[node - 1]
        node = np.where(inner, 2 * node + right, node)
    return value[node - 1]


def predict(raw, classes):
    return (raw[:, 0] >= 0).astype(np.int64) if classes == 2 else np.argmax(raw, axis=1)


def fit(x_train, y_train, x_test, y_test, classes, n_estimators=100, learning_rate=0.1, tie_seed=0):
    """The classifier of one factor.  y_train in 0..classes-1; y_test likewise, -1 for a label the
    training sample does not hold (counted wrong).  Returns a dict: raw_train, raw_test (rows, Kc),
    pred_train, pred_test, acc_train, acc_test, importance (D,), trees (number of trees with a
    split) and the node tables feature, threshold, count, value (stages, T, 15)."""
    x_train = np.ascontiguousarray(x_train, np.float32)
    x_test = np.ascontiguousarray(x_test, np.float32)
    y_train, y_test = np.asarray(y_train, np.int64), np.asarray(y_test, np.int64)
    n, dims = x_train.shape
    trees = 1 if classes == 2 else classes
    order = np.stack([np.argsort(x_train[:, f], kind="stable") for f in range(dims)])
    xs = np.stack([x_train[order[f], f] for f in range(dims)])
    r0 = init_raw(y_train, classes)
    raw, raw_t = np.tile(r0, (n, 1)), np.tile(r0, (x_test.shape[0], 1))
    tabs = [np.zeros((n_estimators, trees, NODES), dt) for dt in (np.int32, np.float32, np.int32, np.float64)]
    acc, used = np.zeros(dims), 0
    for stage in range(n_estimators):
        g, p = gradients(raw, y_train, classes)
        for t in range(trees):
            onehot = (y_train == (1 if classes == 2 else t)).astype(np.float64)
            feat, thr, cnt, val, node, imp = fit_tree(x_train, xs, order, g[t], onehot, classes, stage, t, tie_seed)
            for tab, v in zip(tabs, (feat, thr, cnt, val)):
                tab[stage, t] = v
            raw[:, t] += learning_rate * val[node - 1]
            raw_t[:, t] += learning_rate * apply_tree(feat, thr, val, x_test)
            if feat[0] >= 0:
                acc, used = acc + imp, used + 1
    importance = np.zeros(dims)
    if used:
        avg = acc / float(used)
        with np.errstate(invalid="ignore", divide="ignore"):
            importance = avg / np.sum(avg)
    pred, pred_t = predict(raw, classes), predict(raw_t, classes)
    return {"raw_train": raw, "raw_test": raw_t, "pred_train": pred, "pred_test": pred_t,
            "acc_train": float(np.mean(pred == y_train)), "acc_test": float(np.mean(pred_t == y_test)),
            "importance": importance, "trees": used,
            "feature": tabs[0], "threshold": tabs[1], "count": tabs[2], "value": tabs[3]}


def encode_labels(y_train, y_test):
    """(classes, y_train in 0..C-1, y_test in 0..C-1 or -1): the classes are the distinct training
    values, as sklearn's LabelEncoder takes them."""
    values = np.unique(y_train)
    yt = np.searchsorted(values, y_test)
    yt = np.where((yt < len(values)) & (values[np.minimum(yt, len(values) - 1)] == y_test), yt, -1)
    return len(values), np.searchsorted(values, y_train), yt


def entropy(pk, base):
    """scipy.stats.entropy along axis 0: normalise the columns, then -sum p log p / log base."""
    pk = np.asarray(pk, np.float64)
    pk = pk / np.sum(pk, axis=0, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        h = -np.sum(np.where(pk > 0, pk * np.log(pk), 0.0), axis=0)
    return h / np.log(base)


def scores_from_importance(im):
    """(disentanglement, completeness) of a (D, K) importance matrix, dci.py:105-135."""
    im = np.asarray(im, np.float64)
    total = im.sum()
    w = np.ones_like(im) if total == 0. else im
    dis = np.sum((1. - entropy(im.T + 1e-11, im.shape[1])) * (w.sum(axis=1) / w.sum()))
    com = np.sum((1. - entropy(im + 1e-11, im.shape[0])) * (w.sum(axis=0) / w.sum()))
    return float(dis), float(com)


def dci(mus_train, ys_train, mus_test, ys_test, n_estimators=100, learning_rate=0.1, tie_seed=0):
    """_compute_dci on (rows, D) codes and (K, rows) factor tables.  Returns the four scores, the
    importance matrix and the per-factor fits."""
    dims, k = mus_train.shape[1], ys_train.shape[0]
    im, fits = np.zeros((dims, k)), []
    for i in range(k):
        classes, yt, ye = encode_labels(ys_train[i], ys_test[i])
        if classes < 2:
            raise ValueError(f"factor {i} takes one value in the training sample")
        r = fit(mus_train, yt, mus_test, ye, classes, n_estimators, learning_rate, tie_seed)
        im[:, i] = np.abs(r["importance"])
        fits.append(r)
    dis, com = scores_from_importance(im)
    return {"informativeness_train": float(np.mean([r["acc_train"] for r in fits])),
            "informativeness_test": float(np.mean([r["acc_test"] for r in fits])),
            "disentanglement": dis, "completeness": com, "importance_matrix": im, "fits": fits}
