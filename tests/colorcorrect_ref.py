"""Numpy float64 restatement of the colour fit (adgs.colorcorrect, include/adgs_colorcorrect.h): the clipping in float32, then in double
the iterated, masked, ridge-regularised least-squares fit of a per-image colour transform and its application.  Beside the results it
reports how well-posed the case was: `cond`, the largest condition number of any system solved, and `margin`, how close any COMPUTED
value came to one of the two thresholds of the `unclipped` predicate (a value within the summation-order noise of a threshold could
fall on either side of it in another implementation, and change a mask bit)."""
import numpy as np

FEATURES = 10
LINEAR = (0, 1, 2, 9)            # the features of the affine model


def features(x, model):
    """x: [3, N] float64 -> [10, N]: [r, g, b, r^2, rg, rb, g^2, gb, b^2, 1]; affine: the six quadratic rows are zero"""
    r, g, b = x
    one = np.ones_like(r)
    if model == "affine":
        z = np.zeros_like(r)
        return np.stack([r, g, b, z, z, z, z, z, z, one])
    return np.stack([r, g, b, r * r, r * g, r * b, g * g, g * b, b * b, one])


def identity(c):
    e = np.zeros(FEATURES)
    e[c] = 1.0
    return e


def solve(G, h, c, model, ridge):
    """W of (G + ridge I) W = h + ridge e_c over the model's features -> (W [10], condition number)"""
    idx = list(LINEAR) if model == "affine" else list(range(FEATURES))
    A = G[np.ix_(idx, idx)] + ridge * np.eye(len(idx))
    b = (h + ridge * identity(c))[idx]
    W = np.zeros(FEATURES)
    W[idx] = np.linalg.solve(A, b)
    return W, float(np.linalg.cond(A))


def color_correct(image, gt, weight=None, model="quadratic", iters=5, eps=0.5 / 255, ridge=1e-6):
    """image, gt: [3, H, W] float32 arrays, unclipped; weight: [H, W] in [0, 1] or None.  Returns a dict: "image64" the corrected image
    in double, "image" the same rounded to float32, "warps" [iters, 3, 10], "support" [iters, 3], "cond", "margin"."""
    image, gt = np.asarray(image), np.asarray(gt)
    assert image.dtype == np.float32 and gt.dtype == np.float32 and image.shape == gt.shape and image.shape[0] == 3
    _, H, W = image.shape
    x0 = np.clip(image, np.float32(0), np.float32(1)).astype(np.float64).reshape(3, -1)
    y = np.clip(gt, np.float32(0), np.float32(1)).astype(np.float64).reshape(3, -1)
    w = np.ones(H * W) if weight is None else np.asarray(weight, dtype=np.float64).reshape(-1)
    eps = float(np.float32(eps))
    unclipped = lambda z: (z >= eps) & (z <= 1.0 - eps)
    x = x0
    warps, support = np.zeros((iters, 3, FEATURES)), np.zeros((iters, 3))
    cond, margin = 1.0, np.inf
    for k in range(iters):
        phi = features(x, model)
        for c in range(3):
            m = w * (unclipped(x0[c]) & unclipped(x[c]) & unclipped(y[c]))
            support[k, c] = m.sum()
            if support[k, c] == 0:
                warps[k, c] = identity(c)
                continue
            G = (m * phi) @ phi.T
            h = (m * phi) @ y[c]
            warps[k, c], cnd = solve(G, h, c, model, ridge)
            cond = max(cond, cnd)
        x = np.clip(warps[k] @ phi, 0.0, 1.0)       # a computed value: x0 and y are compared exactly on both sides, this is not
        margin = min(margin, float(np.minimum(np.abs(x - eps), np.abs(x - (1.0 - eps))).min()))
    out = x.reshape(3, H, W)
    return {"image64": out, "image": out.astype(np.float32), "warps": warps, "support": support, "cond": cond, "margin": margin}
