"""numpy restatement of the beta-VAE score's device path (csrc/beta_vae.hip) and of the token PCA
(csrc/token_pca.hip): the feature table, sklearn's default multinomial LogisticRegression as
scipy's L-BFGS-B runs it on an unconstrained problem, the prediction, and PCA(n_components=1).

The fit is a plain two-loop L-BFGS (memory 10, initial scaling y.s / y.y of the newest pair) under
MINPACK-2's dcsrch / dcstep line search with L-BFGS-B's constants (ftol 1e-3, gtol 0.9, xtol 0.1,
stpmin 0, stpmax 1e10; first trial step 1 / |d| in iteration 0, 1 afterwards; at most `maxls`
evaluations per search) and L-BFGS-B's stopping tests.  dcsrch and dcstep are restated here, so
nothing below needs scipy.  Differences from L-BFGS-B, both deliberate: a line search that ends on
anything but its convergence test ends the fit (status 3; L-BFGS-B would accept a "warning" step, or
drop its history and restart), and the direction comes from the two-loop recursion, not from the
compact representation (equal in exact arithmetic).
"""
import numpy as np

EPS = float(np.finfo(np.float64).eps)
M_PAIRS = 10
LS_FTOL, LS_GTOL, LS_XTOL, STPMAX = 1e-3, 0.9, 0.1, 1e10
MAXLS = 50
FACTR = 64.0    # sklearn: ftol = 64 * eps
CONVERGED_GRAD, CONVERGED_F, MAX_ITER, LINE_SEARCH = 0, 1, 2, 3


# ------------------------------------------------------------------ sampler and features
def sample_beta_vae(factor_sizes, random_state, batch_size, num_points):
    """(idx1, idx2 int32 (P, B), labels int32 (P,)) of beta_vae.py _generate_training_sample on a
    full grid in which every factor is latent (row-major mixed radix)."""
    sizes = [int(v) for v in factor_sizes]
    bases = int(np.prod(sizes)) // np.cumprod(sizes)
    idx1 = np.empty((num_points, batch_size), np.int32)
    idx2 = np.empty((num_points, batch_size), np.int32)
    labels = np.empty(num_points, np.int32)

    def factors():
        return np.stack([random_state.randint(s, size=batch_size) for s in sizes], 1)
    for p in range(num_points):
        k = random_state.randint(len(sizes))
        f1 = factors()
        f2 = factors()
        f2[:, k] = f1[:, k]
        idx1[p], idx2[p], labels[p] = f1 @ bases, f2 @ bases, k
    return idx1, idx2, labels


def features(codes, idx1, idx2):
    """fp64 (P, D): np.mean(np.abs(codes[idx1[p]] - codes[idx2[p]]), axis=0) as numpy evaluates it on
    float32 rows: a float32 sum in the order b = 0..B-1, one float32 division by B, then widened."""
    codes = np.asarray(codes, np.float32)
    P, B = idx1.shape
    acc = np.zeros((P, codes.shape[1]), np.float32)
    for b in range(B):
        acc += np.abs(codes[idx1[:, b]] - codes[idx2[:, b]])
    return (acc / np.float32(B)).astype(np.float64)


# ------------------------------------------------------------------ loss
def loss_grad(w, X, y, l2):
    """sklearn's LinearModelLoss(HalfMultinomialLoss, fit_intercept=True).loss_gradient with unit
    sample weights: w (K, D + 1), the intercepts in the last column.  Returns (loss, grad (K, D + 1))."""
    n, D = X.shape
    z = X @ w[:, :D].T + w[:, D]
    zmax = z.max(axis=1, keepdims=True)
    e = np.exp(z - zmax)
    se = e.sum(axis=1, keepdims=True)
    lse = zmax[:, 0] + np.log(se[:, 0])
    loss = np.sum(lse - z[np.arange(n), y]) / n + 0.5 * l2 * np.sum(w[:, :D] * w[:, :D])
    r = e / se
    r[np.arange(n), y] -= 1.0
    r /= n
    g = np.empty_like(w)
    g[:, :D] = r.T @ X + l2 * w[:, :D]
    g[:, D] = r.sum(axis=0)
    return float(loss), g


# ------------------------------------------------------------------ MINPACK-2 line search
def dcstep(stx, fx, dx, sty, fy, dy, stp, fp, dp, brackt, stpmin, stpmax):
    sgnd = dp * (dx / abs(dx))
    if fp > fx:
        theta = 3.0 * (fx - fp) / (stp - stx) + dx + dp
        s = max(abs(theta), abs(dx), abs(dp))
        gamma = s * np.sqrt((theta / s) ** 2 - (dx / s) * (dp / s))
        if stp < stx:
            gamma = -gamma
        p = (gamma - dx) + theta
        q = ((gamma - dx) + gamma) + dp
        r = p / q
        stpc = stx + r * (stp - stx)
        stpq = stx + ((dx / ((fx - fp) / (stp - stx) + dx)) / 2.0) * (stp - stx)
        stpf = stpc if abs(stpc - stx) < abs(stpq - stx) else stpc + (stpq - stpc) / 2.0
        brackt = True
    elif sgnd < 0.0:
        theta = 3.0 * (fx - fp) / (stp - stx) + dx + dp
        s = max(abs(theta), abs(dx), abs(dp))
        gamma = s * np.sqrt((theta / s) ** 2 - (dx / s) * (dp / s))
        if stp > stx:
            gamma = -gamma
        p = (gamma - dp) + theta
        q = ((gamma - dp) + gamma) + dx
        r = p / q
        stpc = stp + r * (stx - stp)
        stpq = stp + (dp / (dp - dx)) * (stx - stp)
        stpf = stpc if abs(stpc - stp) > abs(stpq - stp) else stpq
        brackt = True
    elif abs(dp) < abs(dx):
        theta = 3.0 * (fx - fp) / (stp - stx) + dx + dp
        s = max(abs(theta), abs(dx), abs(dp))
        gamma = s * np.sqrt(max(0.0, (theta / s) ** 2 - (dx / s) * (dp / s)))
        if stp > stx:
            gamma = -gamma
        p = (gamma - dp) + theta
        q = (gamma + (dx - dp)) + gamma
        r = p / q
        if r < 0.0 and gamma != 0.0:
            stpc = stp + r * (stx - stp)
        elif stp > stx:
            stpc = stpmax
        else:
            stpc = stpmin
        stpq = stp + (dp / (dp - dx)) * (stx - stp)
        if brackt:
            stpf = stpc if abs(stpc - stp) < abs(stpq - stp) else stpq
            if stp > stx:
                stpf = min(stp + 0.66 * (sty - stp), stpf)
            else:
                stpf = max(stp + 0.66 * (sty - stp), stpf)
        else:
            stpf = stpc if abs(stpc - stp) > abs(stpq - stp) else stpq
            stpf = min(stpmax, stpf)
            stpf = max(stpmin, stpf)
    else:
        if brackt:
            theta = 3.0 * (fp - fy) / (sty - stp) + dy + dp
            s = max(abs(theta), abs(dy), abs(dp))
            gamma = s * np.sqrt((theta / s) ** 2 - (dy / s) * (dp / s))
            if stp > sty:
                gamma = -gamma
            p = (gamma - dp) + theta
            q = ((gamma - dp) + gamma) + dy
            r = p / q
            stpf = stp + r * (sty - stp)
        elif stp > stx:
            stpf = stpmax
        else:
            stpf = stpmin
    if fp > fx:
        sty, fy, dy = stp, fp, dp
    else:
        if sgnd < 0.0:
            sty, fy, dy = stx, fx, dx
        stx, fx, dx = stp, fp, dp
    return stx, fx, dx, sty, fy, dy, stpf, brackt


class Dcsrch:
    """dcsrch with stpmin = 0: start(f0, g0, stp) opens a search, step(f, g) takes the values at the
    current trial step and returns 'FG' (evaluate self.stp next), 'CONV' or 'WARN'."""

    def start(self, f, g, stp):
        self.brackt, self.stage = False, 1
        self.finit, self.ginit, self.gtest = f, g, LS_FTOL * g
        self.width = STPMAX
        self.width1 = 2.0 * self.width
        self.stx, self.fx, self.gx = 0.0, f, g
        self.sty, self.fy, self.gy = 0.0, f, g
        self.stmin, self.stmax = 0.0, stp + 4.0 * stp
        self.stp = stp

    def step(self, f, g):
        stp = self.stp
        ftest = self.finit + stp * self.gtest
        if self.stage == 1 and f <= ftest and g >= 0.0:
            self.stage = 2
        warn = (self.brackt and (stp <= self.stmin or stp >= self.stmax)) or \
            (self.brackt and self.stmax - self.stmin <= LS_XTOL * self.stmax) or \
            (stp == STPMAX and f <= ftest and g <= self.gtest) or \
            (stp == 0.0 and (f > ftest or g >= self.gtest))
        if f <= ftest and abs(g) <= LS_GTOL * (-self.ginit):
            return 'CONV'
        if warn:
            return 'WARN'
        if self.stage == 1 and f <= self.fx and f > ftest:
            gt = self.gtest
            fm, fxm, fym = f - stp * gt, self.fx - self.stx * gt, self.fy - self.sty * gt
            gm, gxm, gym = g - gt, self.gx - gt, self.gy - gt
            self.stx, fxm, gxm, self.sty, fym, gym, stp, self.brackt = dcstep(
                self.stx, fxm, gxm, self.sty, fym, gym, stp, fm, gm, self.brackt, self.stmin, self.stmax)
            self.fx, self.fy = fxm + self.stx * gt, fym + self.sty * gt
            self.gx, self.gy = gxm + gt, gym + gt
        else:
            self.stx, self.fx, self.gx, self.sty, self.fy, self.gy, stp, self.brackt = dcstep(
                self.stx, self.fx, self.gx, self.sty, self.fy, self.gy, stp, f, g, self.brackt, self.stmin,
                self.stmax)
        if self.brackt:
            if abs(self.sty - self.stx) >= 0.66 * self.width1:
                stp = self.stx + 0.5 * (self.sty - self.stx)
            self.width1 = self.width
            self.width = abs(self.sty - self.stx)
            self.stmin, self.stmax = min(self.stx, self.sty), max(self.stx, self.sty)
        else:
            self.stmin = stp + 1.1 * (stp - self.stx)
            self.stmax = stp + 4.0 * (stp - self.stx)
        stp = min(max(stp, 0.0), STPMAX)
        if (self.brackt and (stp <= self.stmin or stp >= self.stmax)) or \
                (self.brackt and self.stmax - self.stmin <= LS_XTOL * self.stmax):
            stp = self.stx
        self.stp = stp
        return 'FG'


# ------------------------------------------------------------------ the fit
def fit(X, y, classes, C=1.0, max_iter=100, tol=1e-4):
    """X fp64 (n, D), y int (n,) in 0..classes-1.  Returns dict(coef (K, D), intercept (K,), n_iter,
    n_fev, status, loss, max_ls_evals)."""
    X = np.ascontiguousarray(X, np.float64)
    n, D = X.shape
    l2 = 1.0 / (C * n)
    w = np.zeros((classes, D + 1))
    f, g = loss_grad(w, X, y, l2)
    nfev, it, status, max_ls = 1, 0, None, 0
    S, Y, YS = [], [], []
    theta = 1.0
    if np.abs(g).max() <= tol:
        status = CONVERGED_GRAD
    ls = Dcsrch()
    while status is None:
        # two-loop recursion
        q = g.copy()
        alpha = []
        for s_, y_, ys in zip(reversed(S), reversed(Y), reversed(YS)):
            a = np.sum(s_ * q) / ys
            alpha.append(a)
            q -= a * y_
        q /= theta
        for (s_, y_, ys), a in zip(zip(S, Y, YS), reversed(alpha)):
            b = np.sum(y_ * q) / ys
            q += s_ * (a - b)
        d = -q
        dnorm = np.sqrt(np.sum(d * d))
        stp = min(1.0 / dnorm, STPMAX) if it == 0 else 1.0
        w_old, g_old, f_old = w, g, f
        gd = gd_old = np.sum(g * d)
        if gd >= 0.0:
            status = LINE_SEARCH
            break
        ls.start(f, gd, stp)
        evals = 0
        while True:
            if evals >= MAXLS:
                status = LINE_SEARCH
                break
            stp = ls.stp
            w = w_old + stp * d
            f, g = loss_grad(w, X, y, l2)
            nfev += 1
            evals += 1
            gd = np.sum(g * d)
            task = ls.step(f, gd)
            if task == 'CONV':
                break
            if task == 'WARN':
                status = LINE_SEARCH
                break
        max_ls = max(max_ls, evals)
        if status is not None:
            break
        it += 1
        if np.abs(g).max() <= tol:
            status = CONVERGED_GRAD
            break
        if f_old - f <= FACTR * EPS * max(abs(f_old), abs(f), 1.0):
            status = CONVERGED_F
            break
        yv = g - g_old
        rr = np.sum(yv * yv)
        dr = (gd - gd_old) * stp
        if dr > EPS * (-gd_old * stp):
            if len(S) == M_PAIRS:
                S.pop(0), Y.pop(0), YS.pop(0)
            S.append(stp * d), Y.append(yv), YS.append(dr)
            theta = rr / dr
        if it >= max_iter:
            status = MAX_ITER
    return dict(coef=w[:, :D].copy(), intercept=w[:, D].copy(), n_iter=it, n_fev=nfev, status=status, loss=f,
                max_ls_evals=max_ls)


def decisions(X, coef, intercept):
    return np.asarray(X, np.float64) @ coef.T + intercept


def predict(X, coef, intercept):
    """(decisions (P, K), predictions (P,)): first-maximum argmax."""
    z = decisions(X, coef, intercept)
    return z, np.argmax(z, axis=1)


def centred(z):
    return z - z.mean(axis=1, keepdims=True)


# ------------------------------------------------------------------ token PCA
def token_moments(tokens):
    """float64 (mean (U, d), covariance (U, d, d), ddof = 1) of tokens (N, U, d)."""
    t = np.asarray(tokens, np.float64)
    mean = t.mean(axis=0)
    c = t - mean
    cov = np.einsum('nui,nuj->uij', c, c) / (t.shape[0] - 1)
    return mean, cov


def flip_sign(v):
    """sklearn >= 1.5's svd_flip(u_based_decision=False) on one component: the entry of largest
    magnitude (the first of equals) becomes positive."""
    s = np.sign(v[np.argmax(np.abs(v))])
    return v * (s if s != 0 else 1.0)


def top_components(cov):
    """(components (U, d), explained_variance (U,)): the eigenvector of the largest eigenvalue of
    every unit's covariance, signed by flip_sign."""
    comps, ev = [], []
    for c in cov:
        w, v = np.linalg.eigh(c)
        comps.append(flip_sign(v[:, -1]))
        ev.append(w[-1])
    return np.stack(comps), np.array(ev)


def token_pca(tokens):
    """float64 PCA(n_components=1).fit_transform of every unit: (codes (N, U), components, mean,
    explained_variance)."""
    mean, cov = token_moments(tokens)
    comps, ev = top_components(cov)
    codes = np.einsum('nud,ud->nu', np.asarray(tokens, np.float64) - mean, comps)
    return codes, comps, mean, ev


# ------------------------------------------------------------------ shared test inputs
TOKEN_SHAPES = ((2, 1, 1), (257, 3, 16), (4099, 20, 16), (513, 64, 64))


def make_tokens(shape, seed=0):
    """float32 (N, U, d) tokens whose units each have one clearly dominant direction (standard
    deviation 3 along it, 0.3 across it) around a non-zero mean; the legacy RandomState stream is
    the same in every numpy, and the fixture records the sum of the table as a guard."""
    n, u, d = shape
    rs = np.random.RandomState(100 + seed)
    direction = rs.randn(u, d)
    direction /= np.linalg.norm(direction, axis=1, keepdims=True)
    a = rs.randn(n, u)
    t = 3.0 * a[:, :, None] * direction + 0.3 * rs.randn(n, u, d) + rs.uniform(-2, 2, size=(u, d))
    return t.astype(np.float32)
