"""genphi_result_eigen's iteration (include/genphi.h) restated in numpy on a host matrix, with the same start stream: Lanczos with
full reorthogonalisation (classical Gram-Schmidt twice), the convergence test beta_m |s_(m,i)| <= tol theta_1, the breakdown rule and the
sign rule.  Not the library's code: numpy's products, sums and eigh, so values agree to rounding, not to the bit.  Beside the pairs,
lanczos() reports the step at which its estimate passes 4 tol, tol and tol / 4 -- the window that the device's step count must fall into."""
import numpy as np

GAMMA = np.uint64(0x9E3779B97F4A7C15)
BREAKDOWN = 2.0 ** -40
MASK = (1 << 64) - 1


def draws(seed, first, n):
    """Draws first .. first + n - 1 of the splitmix64 stream on seed, as float64 in [-1, 1)."""
    with np.errstate(over="ignore"):
        z = np.uint64(seed & MASK) + GAMMA * np.arange(first + 1, first + n + 1, dtype=np.uint64)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return 2.0 * ((z >> np.uint64(11)).astype(np.float64) * 2.0 ** -53) - 1.0


def sign_rule(v):
    big = np.argmax(np.abs(v), axis=0)
    return v * np.where(v[big, np.arange(v.shape[1])] < 0.0, -1.0, 1.0)


def centred(a):
    a = np.asarray(a, dtype=np.float64)
    a = a - a.mean(axis=0)[None, :]
    return a - a.mean(axis=1)[:, None]


def lanczos(a, k, center=False, tol=1e-8, maxiter=300, seed=0):
    """dict: values, vectors, residual, converged, products (all at the stop for `tol`), and steps = {4 tol: m, tol: m, tol / 4: m}, the
    first step at which the k largest pairs meet that tolerance (None if min(maxiter, N) steps do not get there)."""
    a = np.asarray(a, dtype=np.float64)
    n = len(a)
    c = (lambda x: x - x.sum() / n) if center else (lambda x: x)
    op = lambda x: c(a @ c(x))
    taken = 0

    def fresh():
        nonlocal taken
        x = c(draws(seed, taken, n))
        taken += n
        return x / np.sqrt(x @ x)

    tols = {4 * tol: None, tol: None, tol / 4: None}
    V = np.zeros((min(maxiter, n) + 1, n))
    V[0] = fresh()
    alpha, beta = [], []
    scale, m, at_tol = 0.0, 0, None

    def ortho(w, m):
        h = V[:m] @ w
        w = w - h @ V[:m]
        h2 = V[:m] @ w
        return w - h2 @ V[:m], h[m - 1] + h2[m - 1]

    def snapshot(flags):
        T = np.diag(alpha) + np.diag(beta[:m - 1], 1) + np.diag(beta[:m - 1], -1)
        lam, s = np.linalg.eigh(T)
        order = np.argsort(-lam, kind="stable")[:k]
        vec = sign_rule((V[:m].T @ s[:, order]))
        if center:
            vec = vec - vec.mean(axis=0)[None, :]
        val = lam[order]
        res = np.sqrt(((np.apply_along_axis(op, 0, vec) - vec * val) ** 2).sum(axis=0))
        return dict(values=val, vectors=vec, residual=res, converged=np.array(flags, dtype=bool), products=m)

    while m < min(maxiter, n):
        w = op(V[m])
        m += 1
        w, al = ortho(w, m)
        b = np.sqrt(w @ w)
        alpha.append(al)
        scale = max(scale, abs(al) + b)
        if b <= BREAKDOWN * scale:
            beta.append(0.0)
            if m >= k:
                for t in tols:
                    tols[t] = tols[t] or m
                at_tol = at_tol or snapshot([True] * k)
                break
            x, _ = ortho(fresh(), m)
            left = np.sqrt(x @ x)
            if left <= BREAKDOWN:
                break
            V[m] = x / left
            continue
        beta.append(b)
        V[m] = w / b
        if m < k:
            continue
        T = np.diag(alpha) + np.diag(beta[:m - 1], 1) + np.diag(beta[:m - 1], -1)
        lam, s = np.linalg.eigh(T)
        order = np.argsort(-lam, kind="stable")[:k]
        est = b * np.abs(s[m - 1, order])
        for t in tols:
            if tols[t] is None and np.all(est <= t * lam[order[0]]):
                tols[t] = m
        if at_tol is None and tols[tol] is not None:
            at_tol = snapshot(est <= tol * lam[order[0]])
        if tols[tol / 4] is not None:
            break
    if at_tol is None:
        T = np.diag(alpha) + np.diag(beta[:m - 1], 1) + np.diag(beta[:m - 1], -1)
        lam, s = np.linalg.eigh(T)
        order = np.argsort(-lam, kind="stable")[:k]
        at_tol = snapshot(beta[m - 1] * np.abs(s[m - 1, order]) <= tol * lam[order[0]])
    at_tol["steps"] = tols
    return at_tol
