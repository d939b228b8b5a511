"""Vectorised numpy restatement of the reference's TAD metric, written from the reference's text
(ae_utils_exp.py: LatentClass, calculate_auroc, aurocs, aurocs_search; celeba_tad.py:47-120), not
from csrc/tad.hip or encdiff_amd/metrics.py.  Steps 1-5 (the areas) are float32 as the reference
computes them, step 6 (the script's arithmetic) float64.  tests/test_tad_host.py checks it against
the reference's own output (tests/golden/tad_small.npz, tools/gen_golden_tad.py); the GPU tests
compare the kernels with it where the reference recorded nothing.
"""
import numpy as np

F32 = np.float32
GATE = F32(0.2)


def column_range(z):
    """aurocs_search:224-225, out.max(dim=0)[0] and out.min(dim=0)[0]."""
    z = np.asarray(z, F32)
    return z.max(axis=0), z.min(axis=0)


def thresholds(t, ma, mi):
    """LatentClass.__call__:169-170, thr = t * (ma - mi) + mi: (L, 11) float32, the difference, the
    product and the sum rounded one by one (numpy float32 arithmetic does not fuse)."""
    t, ma, mi = np.asarray(t, F32), np.asarray(ma, F32), np.asarray(mi, F32)
    d = (ma - mi).astype(F32)
    return ((t[None, :] * d[:, None]).astype(F32) + mi[:, None]).astype(F32)


def counts(z, targ, thr):
    """calculate_auroc:183-186.  pred is 1 where z[:, l] >= thr (LatentClass:171), so
    logical_and(pred == targ, pred) counts the rows with pred and label set (p_tp) and
    logical_and(pred != targ, pred) those with pred set and the label not (p_fp = total - p_tp).
    Returns int64 (L, 11, A + 1): [..., a] = p_tp of attribute a, [..., A] = #{z >= thr}."""
    z, targ = np.asarray(z, F32), np.asarray(targ)
    N, L = z.shape
    A = targ.shape[1]
    lab = np.concatenate([targ != 0, np.ones((N, 1), bool)], 1).astype(np.float64)  # exact below 2^53
    out = np.empty((L, thr.shape[1], A + 1), np.int64)
    for k in range(thr.shape[1]):
        pred = (z >= thr[None, :, k]).astype(np.float64)  # (N, L)
        out[:, k, :] = np.rint(pred.T @ lab).astype(np.int64)
    return out


def joint_counts(targ):
    """TT[i][j] = rows with labels i and j set (j_prob of celeba_tad.py:74,101 times N)."""
    b = (np.asarray(targ) != 0).astype(np.int64)
    return b.T @ b


def aurocs_from_counts(cnt, pos, n, ma, mi):
    """calculate_auroc:177-203 and aurocs:207-212 from the counts: (A, L) float32."""
    cnt = np.asarray(cnt, np.int64)
    L, T, A1 = cnt.shape
    A = A1 - 1
    pos = np.asarray(pos, np.int64)                      # :178 pos_total
    neg = n - pos                                        # :179 neg_total
    posf, negf = pos.astype(F32)[None, None, :], neg.astype(F32)[None, None, :]
    tp = cnt[:, :, :A]                                   # :185 p_tp
    fp = cnt[:, :, A:] - tp                              # :186 p_fp
    with np.errstate(divide="ignore", invalid="ignore"):
        p_fpr = fp.astype(F32) / negf                    # :187
        p_tpr = tp.astype(F32) / posf                    # :188
        n_fpr = (neg[None, None, :] - fp).astype(F32) / negf   # :191-193, pred = z < thr
        n_tpr = (pos[None, None, :] - tp).astype(F32) / posf   # :194

    def area(fpr, tpr):
        fpr, tpr = np.sort(fpr, axis=1), np.sort(tpr, axis=1)  # :197-198 sort(dim=0), each column alone
        dist = (fpr[:, 1:] - fpr[:, :-1]).astype(F32)          # :199
        prod = (tpr[:, 1:] * dist).astype(F32)                 # :200
        acc = np.zeros((L, A), F32)
        for i in range(T - 1):                                 # :200 .sum(), in index order
            acc = (acc + prod[:, i]).astype(F32)
        return acc

    pa, na = area(p_fpr, p_tpr), area(n_fpr, n_tpr)
    m = np.where(na > pa, na, pa)                        # aurocs:211, Python's max(p_auroc, n_auroc)
    gate = (np.asarray(ma, F32) - np.asarray(mi, F32)).astype(F32) > GATE   # aurocs:209
    return np.where(gate[:, None], m, F32(0.5)).astype(F32).T   # aurocs:207, 0.5 where not searched


def aurocs(z, targ, t):
    """Steps 1-5: what aurocs_search returns as aurocs_all, for every attribute of targ."""
    ma, mi = column_range(z)
    thr = thresholds(t, ma, mi)
    cnt = counts(z, targ, thr)
    pos = (np.asarray(targ) != 0).sum(axis=0)
    return aurocs_from_counts(cnt, pos, z.shape[0], ma, mi)


def base_rates(targ):
    """aurocs_search:221-222, targ.sum(dim=0) / N in float32."""
    targ = np.asarray(targ)
    return (targ != 0).sum(axis=0).astype(F32) / F32(targ.shape[0])


def label_mi(targ):
    """celeba_tad.py:72-104 in float64: the mutual information of every pair of labels."""
    t = (np.asarray(targ) != 0)
    n = t.shape[0]
    A = t.shape[1]
    nt = ~t
    mi = np.zeros((A, A))
    for i in range(A):
        i_mp = t[:, i].sum() / n                                     # :81
        for j in range(A):
            j_mp = t[:, j].sum() / n                                 # :83
            for x, y, pi, pj in ((nt[:, i], nt[:, j], 1. - i_mp, 1. - j_mp),   # :86-89 FF
                                 (nt[:, i], t[:, j], 1. - i_mp, j_mp),         # :91-94 FT
                                 (t[:, i], nt[:, j], i_mp, 1. - j_mp),         # :96-99 TF
                                 (t[:, i], t[:, j], i_mp, j_mp)):              # :101-104 TT
                jp = np.logical_and(x, y).sum() / n                  # :74 j_prob
                if not (jp == 0. or pi == 0. or pj == 0.):           # :75 mi
                    mi[i, j] += jp * np.log(jp / (pi * pj))
    return mi


def tad(au, targ, thresh=0.75, ent_red_thresh=0.2):
    """celeba_tad.py:51-120 in float64 from the (A, L) areas and the labels."""
    au = np.asarray(au, np.float64)
    A = au.shape[0]
    max_aur, argmax_aur = au.max(axis=1), au.argmax(axis=1)          # :51
    norm_diffs, aurs_diffs = np.zeros(A), np.zeros(A)                # :52-53
    for ind in range(A):                                             # :54
        aurs, argmax_a = au[ind], argmax_aur[ind]
        with np.errstate(divide="ignore", invalid="ignore"):
            norm_aurs = (aurs - 0.5) / (aurs[argmax_a] - 0.5)        # :55
        aurs_next = aurs.copy()                                      # :56
        aurs_next[argmax_a] = 0.0                                    # :57
        aurs_diffs[ind] = max_aur[ind] - aurs_next.max()             # :58-59
        norm_aurs[argmax_a] = 0.0                                    # :60
        norm_diffs[ind] = 1. - norm_aurs.max()                       # :61-62
    mi_mat = label_mi(targ)
    mi_maxes = (mi_mat * (1 - np.eye(A))).max(axis=1)                # :106
    with np.errstate(divide="ignore", invalid="ignore"):
        ent_red_prop = 1. - (np.diag(mi_mat) - mi_maxes) / np.diag(mi_mat)   # :107
    filt = np.logical_and(max_aur >= thresh, ent_red_prop <= ent_red_thresh)  # :114
    return {"tad_score": float(aurs_diffs[filt].sum()), "attributes_captured": int(filt.sum()),   # :116-120
            "max_auroc": max_aur, "argmax_latent": argmax_aur, "auroc_diff": aurs_diffs, "norm_diff": norm_diffs,
            "ent_red_prop": ent_red_prop, "captured": filt}
