"""Reference for nr_fit_*: a helper, not a test.

The numpy restatement of the arithmetic contract in include/neural_render.h (steps 1-7), on
grad_ref's exact f32 fmaf: the forward pass with its activations, the clamped or plain residual, the
backward chains seeded with it, the partial sums in point order (tile t of 16 points in partial
t mod S, a ragged last tile completed with points x = 0 whose e and g are +0), the two-level totals,
the scaling and Adam.  tests/test_fit_cpu.py pins the forward against grad_ref.forward_masks (and so
against the oracle) and the gradient against an f64 backpropagation on a designed network.
"""
import numpy as np

from grad_ref import F, _chain, fmaf, forward_masks  # noqa: F401  (forward_masks: re-exported for the tests)

CHUNKS = 16
DEFAULT_PARTIALS = 1024


def flatten(K, B):
    """K_0, B_0, K_1, B_1, ..., K_last, B_last, each kernel (in, out) row-major."""
    return np.concatenate([np.concatenate([np.asarray(k, F).ravel(), np.asarray(b, F).ravel()]) for k, b in zip(K, B)])


def unflatten(dims, flat):
    K, B, q = [], [], 0
    for i, o in zip(dims[:-1], dims[1:]):
        K.append(np.array(flat[q:q + i * o], F).reshape(i, o)); q += i * o
        B.append(np.array(flat[q:q + o], F)); q += o
    assert q == len(flat)
    return K, B


def forward_acts(K, B, X):
    """(value [n], acts a_0..a_nh [n, 32], masks z_l > 0): step 1."""
    a = np.ascontiguousarray(X, F)
    acts, masks = [], []
    for l, (W, b) in enumerate(zip(K, B)):
        z = (_chain(np.asarray(W, F), a) + np.asarray(b, F)[None, :]).astype(F)
        if l == len(K) - 1:
            return z[:, 0], acts, masks
        masks.append(z > 0)
        a = np.maximum(z, F(0))
        acts.append(a)


def per_point(K, B, X, Y, clamp):
    """Steps 1-3 on the points completed to whole tiles: value, e, g, acts, deltas d_0..d_nh."""
    X, Y = np.ascontiguousarray(X, F).reshape(-1, 3), np.ascontiguousarray(Y, F).reshape(-1)
    n = len(X)
    npad = -(-n // 16) * 16
    Xp, Yp = np.zeros((npad, 3), F), np.zeros(npad, F)
    Xp[:n], Yp[:n] = X, Y
    live = np.arange(npad) < n
    v, acts, masks = forward_acts(K, B, Xp)
    c = F(clamp)
    if c > 0:
        vc = np.minimum(np.maximum(v, -c), c)
        inside = (v > -c) & (v < c)
    else:
        vc, inside = v, np.ones(npad, bool)
    e = np.where(live, (vc - Yp).astype(F), F(0)).astype(F)
    g = np.where(inside, e, F(0)).astype(F)
    nh = len(K) - 2
    kl = np.asarray(K[-1], F)[:, 0]
    d = [None] * (nh + 1)
    d[nh] = np.where(masks[nh], (kl[None, :] * g[:, None]).astype(F), F(0)).astype(F)
    for l in range(nh, 0, -1):
        acc = _chain(np.asarray(K[l], F).T, d[l])  # acc[i] = chain over j of K_l[i][j] d_l[j]
        d[l - 1] = np.where(masks[l - 1], acc, F(0)).astype(F)
    return {"n": n, "X": Xp, "value": v, "e": e, "g": g, "acts": acts, "d": d}


def partial_sums(K, pp, S):
    """Step 4: (GK [S, in, out] per layer, GB [S, out] per layer, SS [S])."""
    nl = len(K)
    ntiles = len(pp["X"]) // 16
    shapes = [np.asarray(k).shape for k in K]
    GK = [np.zeros((S,) + s, F) for s in shapes]
    GB = [np.zeros((S, s[1]), F) for s in shapes]
    SS = np.zeros(S, F)
    ins = [pp["X"]] + pp["acts"]
    outs = pp["d"] + [pp["g"][:, None]]
    for r in range(-(-ntiles // S)):
        cnt = min(S, ntiles - r * S)
        for i in range(16):
            idx = (r * S + np.arange(cnt)) * 16 + i
            for l in range(nl):
                a, dl = ins[l][idx], outs[l][idx]
                GK[l][:cnt] = fmaf(a[:, :, None], dl[:, None, :], GK[l][:cnt])
                GB[l][:cnt] = (GB[l][:cnt] + dl).astype(F)
            SS[:cnt] = fmaf(pp["e"][idx], pp["e"][idx], SS[:cnt])
    return GK, GB, SS


def totals(Pm):
    """Step 5 over axis 0 of Pm [S, ...]."""
    S = Pm.shape[0]
    C = -(-S // CHUNKS)
    T = np.zeros(Pm.shape[1:], F)
    for k in range(CHUNKS):
        U = np.zeros(Pm.shape[1:], F)
        for s in range(k * C, min((k + 1) * C, S)):
            U = (U + Pm[s]).astype(F)
        T = (T + U).astype(F)
    return T


def gradient(K, B, X, Y, clamp=0.0, partials=0):
    """nr_fit_gradient: {loss (f32), grad (flat [P]), value [n]}."""
    S = partials if partials > 0 else DEFAULT_PARTIALS
    pp = per_point(K, B, X, Y, clamp)
    GK, GB, SS = partial_sums(K, pp, S)
    inv_n = F(1.0) / F(pp["n"])
    flat = np.concatenate([np.concatenate([totals(gk).ravel(), totals(gb).ravel()]) for gk, gb in zip(GK, GB)])
    return {"loss": F(totals(SS) * inv_n), "grad": (flat * inv_n).astype(F), "value": pp["value"][:pp["n"]]}


def adam_consts(lr, beta1, beta2, t):
    """(a_t, omb1, omb2): formed in double from the f32 options, rounded to f32."""
    lr, b1, b2 = float(F(lr)), float(F(beta1)), float(F(beta2))
    return F(lr * np.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)), F(1.0 - b1), F(1.0 - b2)


class Fit:
    """nr_fit's state and calls."""

    def __init__(self, dims, K, B, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, clamp=0.0, partials=0):
        self.dims = list(dims)
        self.theta = flatten(K, B)
        self.m = np.zeros_like(self.theta)
        self.v = np.zeros_like(self.theta)
        self.step = 0
        self.lr, self.beta1, self.beta2, self.eps = F(lr), F(beta1), F(beta2), F(eps)
        self.clamp, self.partials = clamp, partials

    def weights(self):
        return unflatten(self.dims, self.theta)

    def gradient(self, X, Y):
        K, B = self.weights()
        return gradient(K, B, X, Y, self.clamp, self.partials)

    def run(self, X, Y, batch):
        X, Y = np.ascontiguousarray(X, F).reshape(-1, 3), np.ascontiguousarray(Y, F).reshape(-1)
        assert len(X) % batch == 0
        losses = []
        for k in range(len(X) // batch):
            out = self.gradient(X[k * batch:(k + 1) * batch], Y[k * batch:(k + 1) * batch])
            losses.append(out["loss"])
            self.step += 1
            a_t, omb1, omb2 = adam_consts(self.lr, self.beta1, self.beta2, self.step)
            G = out["grad"]
            self.m = ((self.beta1 * self.m).astype(F) + (omb1 * G).astype(F)).astype(F)
            self.v = ((self.beta2 * self.v).astype(F) + (omb2 * (G * G).astype(F)).astype(F)).astype(F)
            upd = ((a_t * self.m).astype(F) / (np.sqrt(self.v).astype(F) + self.eps).astype(F)).astype(F)
            self.theta = (self.theta - upd).astype(F)
        return np.array(losses, F)
