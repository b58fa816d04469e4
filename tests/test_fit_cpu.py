"""The numpy restatement of nr_fit_* (tests/fit_ref.py) against independent arithmetic: no GPU.

The GPU tests (tests/test_gpu_fit.py) compare the library bit for bit with fit_ref; these tests pin
that fit_ref computes what the contract means: the oracle's forward bits, the true gradient, the
clamp's semantics, Adam's step numbering, and a loss that falls.
"""

import numpy as np
import pytest

import fit_ref
import grad_ref

F = np.float32


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def seeded_net(dims, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    K = [(rng.normal(0, scale / np.sqrt(i), (i, o))).astype(F) for i, o in zip(dims[:-1], dims[1:])]
    B = [rng.normal(0, 0.1, o).astype(F) for o in dims[1:]]
    return K, B


@pytest.mark.parametrize("dims", [[3, 32, 1], [3, 32, 32, 1], [3] + [32] * 8 + [1]])
def test_forward_bits_are_grad_refs(dims):
    K, B = seeded_net(dims, 3)
    X = np.random.default_rng(4).uniform(-1.2, 1.2, (77, 3)).astype(F)
    v, acts, masks = fit_ref.forward_acts(K, B, X)
    rv, rmasks = grad_ref.forward_masks(K, B, X)
    assert np.array_equal(bits(v), bits(rv))
    assert len(masks) == len(rmasks) == len(dims) - 2
    for m, rm, a in zip(masks, rmasks, acts):
        assert np.array_equal(m, rm) and np.array_equal(a > 0, m)
    # and the value the fit's own calls return (points completed to whole tiles, then cut back)
    assert np.array_equal(bits(fit_ref.gradient(K, B, X, np.zeros(77, F), 0.0, 4)["value"]), bits(rv))


def designed_net():
    """[3, 32, 32, 1], weights in {-1, 0, 1} (three non-zeros per hidden unit, eight in the last
    kernel), biases multiples of 1/4."""
    rng = np.random.default_rng(11)
    K0 = rng.integers(-1, 2, (3, 32)).astype(F)
    K1 = np.zeros((32, 32), F)
    for j in range(32):
        K1[rng.choice(32, 3, replace=False), j] = rng.choice([-1.0, 1.0], 3)
    K2 = np.zeros((32, 1), F)
    K2[rng.choice(32, 8, replace=False), 0] = rng.choice([-1.0, 1.0], 8)
    B = [(rng.integers(-2, 3, o) / 4).astype(F) for o in (32, 32, 1)]
    return [K0, K1, K2], B


def test_exact_gradient_on_designed_network():
    K, B = designed_net()
    n, S = 128, 4
    rng = np.random.default_rng(12)
    X = (rng.integers(-4, 5, (n, 3)) / 4).astype(F)
    Y = (rng.integers(-8, 9, n) / 4).astype(F)
    # f64 backpropagation, every intermediate checked to be an f32 (then no rounding happens in any
    # order of any sum, and the f32 chains are exact)
    exact = lambda a: np.array_equal(np.asarray(a, np.float64), np.asarray(a, np.float64).astype(F).astype(np.float64))
    a = X.astype(np.float64)
    acts = [a]
    for l in range(3):
        z = a @ K[l].astype(np.float64) + B[l].astype(np.float64)
        assert exact(z)
        if l < 2:
            a = np.maximum(z, 0)
            acts.append(a)
    e = z[:, 0] - Y
    assert exact(e) and exact(np.cumsum(e * e))
    assert (e != 0).sum() > n // 2
    d = e[:, None]
    G = []
    for l in (2, 1, 0):
        per_point = acts[l][:, :, None] * d[:, None, :]
        assert exact(per_point) and exact(np.cumsum(per_point, axis=0)) and exact(np.cumsum(d, axis=0))
        # (bound on every partial sum in any order: the sum of magnitudes is an exact f32 integer multiple of 1/16)
        assert np.abs(per_point).sum(axis=0).max() < 2 ** 20 and np.abs(d).sum(axis=0).max() < 2 ** 20
        G.append((per_point.sum(axis=0) / n, d.sum(axis=0) / n))
        if l > 0:
            d = (d @ K[l].astype(np.float64).T) * (acts[l] > 0)
            assert exact(d)
    G = G[::-1]
    assert all((gk != 0).any() for gk, _ in G)
    want = np.concatenate([np.concatenate([gk.ravel(), gb.ravel()]) for gk, gb in G])
    got = fit_ref.gradient(K, B, X, Y, 0.0, S)
    assert np.array_equal(got["grad"].astype(np.float64), want)
    assert float(got["loss"]) == (e * e).sum() / n


def test_clamp_semantics():
    dims = [3, 32, 32, 1]
    K, B = seeded_net(dims, 5)
    rng = np.random.default_rng(6)
    X = rng.uniform(-1, 1, (100, 3)).astype(F)
    v = grad_ref.forward_masks(K, B, X)[0]
    Y = (v + rng.normal(0, 0.05, 100)).astype(F)
    c = F(np.median(np.abs(v)))
    pp = fit_ref.per_point(K, B, X, Y, c)
    out = (v >= c) | (v <= -c)
    assert 20 < out.sum() < 80
    vn = pp["value"][:100]
    assert np.array_equal(bits(vn), bits(v))
    want_e = (np.clip(v, -c, c) - Y).astype(F)
    assert np.array_equal(bits(pp["e"][:100]), bits(want_e))
    assert np.all(bits(pp["g"][:100][out]) == 0) and np.array_equal(bits(pp["g"][:100][~out]), bits(want_e[~out]))
    assert np.all(pp["e"][100:] == 0) and np.all(bits(pp["g"][100:]) == 0)
    for dl in pp["d"]:
        assert not dl[:100][out].any()
    # only clamped points: the loss is the chain of e * e, every gradient entry +0
    Xo, Yo = X[out], Y[out]
    g = fit_ref.gradient(K, B, Xo, Yo, c, 1)
    assert np.all(bits(g["grad"]) == 0)
    ss = F(0)
    for ei in want_e[out]:
        ss = grad_ref.fmaf(ei, ei, ss)
    assert bits(g["loss"]) == bits(F(ss * (F(1) / F(out.sum()))))
    # clamp = 0: the plain residual
    p0 = fit_ref.per_point(K, B, X, Y, 0.0)
    assert np.array_equal(bits(p0["e"][:100]), bits((v - Y).astype(F))) and np.array_equal(bits(p0["g"]), bits(p0["e"]))


def test_step_numbering_carries_across_calls():
    dims = [3, 32, 32, 1]
    K, B = seeded_net(dims, 8)
    rng = np.random.default_rng(9)
    X = rng.uniform(-1, 1, (20 * 32, 3)).astype(F)
    Y = (np.linalg.norm(X, axis=1) - 0.5).astype(F)
    one = fit_ref.Fit(dims, K, B, lr=1e-2, partials=4)
    l1 = one.run(X, Y, 32)
    four = fit_ref.Fit(dims, K, B, lr=1e-2, partials=4)
    l4 = np.concatenate([four.run(X[q * 160:(q + 1) * 160], Y[q * 160:(q + 1) * 160], 32) for q in range(4)])
    assert one.step == four.step == 20
    assert np.array_equal(bits(l1), bits(l4))
    assert np.array_equal(bits(one.theta), bits(four.theta)) and np.array_equal(bits(one.m), bits(four.m))
    assert not np.array_equal(bits(one.theta), bits(fit_ref.flatten(K, B)))
    # a_t really depends on t: the first step's differs from the twentieth's
    assert fit_ref.adam_consts(1e-2, 0.9, 0.999, 1)[0] != fit_ref.adam_consts(1e-2, 0.9, 0.999, 20)[0]


def test_loss_falls_on_a_sphere():
    """y = |x| - 0.5 on 1024 points, [3, 32, 32, 1], seeded init, lr = 1e-3, 50 full-batch steps.
    Measured: loss 0.89389 at step 0, 0.03401 after 50 steps, ratio 0.038."""
    dims = [3, 32, 32, 1]
    K, B = seeded_net(dims, 21)
    rng = np.random.default_rng(22)
    X = rng.uniform(-1, 1, (1024, 3)).astype(F)
    Y = (np.linalg.norm(X, axis=1) - 0.5).astype(F)
    f = fit_ref.Fit(dims, K, B, lr=1e-3, partials=16)
    losses = f.run(np.tile(X, (51, 1)), np.tile(Y, 51), 1024)
    print("sphere losses", losses[0], losses[50], losses[50] / losses[0])
    assert f.step == 51 and losses[50] < losses[0]
