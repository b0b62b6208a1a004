"""Numpy restatement of the batched ADVI entry points (csrc/gsmvi_advi_batched.hip): init, step, cov and the fit loop, in the
packed layout (scales = the entries of L in np.tril_indices order) and with the draws of the batched fits (draw c of a key is
B x (D + D % 2) normals of philox_randn, column D dropped for odd D).  Test-only; it is pinned to torch autograd + torch.optim.Adam
through ``torch_advi_run`` (tests/test_advi_batched_cpu.py), which drives the package's single-problem ``ADVI.neg_elbo`` with the
same normals."""
import math
from unittest import mock

import numpy as np

from oracle import gsm_oracle as orc

LOG_2PI = math.log(2.0 * math.pi)


def tri(D):
    return D * (D + 1) // 2


def draw(seed, call, B, D):
    """z (B, D) of draw ``call`` of key ``seed`` in the fits' layout"""
    Dz = D + (D & 1)
    return orc.philox_randn(int(seed), int(call), B * Dz).reshape(B, Dz)[:, :D].copy()


def unpack(scales, D):
    L = np.zeros((D, D))
    L[np.tril_indices(D)] = scales
    return L


def cov_of(scales, D):
    """(K, P) packed factors -> (K, D, D) covariances L L^T"""
    scales = np.asarray(scales)
    out = np.empty((scales.shape[0], D, D))
    for k in range(scales.shape[0]):
        L = unpack(scales[k], D)
        out[k] = L @ L.T
    return out


def sample(loc, scales, Z):
    """one problem: x_b = loc + L z_b and sum_b log q(x_b)"""
    B, D = Z.shape
    L = unpack(scales, D)
    X = Z @ L.T + loc[None, :]
    logq = -0.5 * np.sum(Z * Z) - B * np.sum(np.log(np.abs(np.diag(L)))) - 0.5 * B * D * LOG_2PI
    return X, logq


def init(mean, cov, Z=None):
    """(K, D), (K, D, D) -> scales (K, P); with Z (K, B, D) also X and logq"""
    K, D = mean.shape
    scales = np.stack([np.linalg.cholesky(cov[k])[np.tril_indices(D)] for k in range(K)])
    if Z is None:
        return scales
    out = [sample(mean[k], scales[k], Z[k]) for k in range(K)]
    return scales, np.stack([o[0] for o in out]), np.array([o[1] for o in out])


def gradient(G, Z, scales):
    """one problem: the gradient of -(sum_b lp(x_b) - sum_b log q(x_b)) with respect to (loc, scales), g_b = grad lp(x_b)"""
    B, D = Z.shape
    L = unpack(scales, D)
    gL = -(G.T @ Z)
    gL[np.diag_indices(D)] -= B / np.diag(L)
    return -G.sum(axis=0), gL[np.tril_indices(D)]


def adam(p, g, m, v, t, lr, b1, b2, eps):
    """torch.optim.Adam at its defaults / optax.adam: returns the new (p, m, v)"""
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * (g * g)
    step = lr / (1.0 - b1 ** t)
    return p - step * (m / (np.sqrt(v) / math.sqrt(1.0 - b2 ** t) + eps)), m, v


def step(G, Z, loc, scales, moments, t, lr, b1=0.9, b2=0.999, eps=1e-8, Znext=None):
    """K problems, nothing in place: returns (loc, scales, moments[, X, logq of Znext from the updated state]); lr a float or K"""
    K, B, D = G.shape
    lrs = np.broadcast_to(np.asarray(lr, dtype=np.float64), (K,))
    loc, scales = np.array(loc, copy=True), np.array(scales, copy=True)
    m_loc, v_loc, m_s, v_s = (np.array(a, copy=True) for a in moments)
    for k in range(K):
        with np.errstate(all="ignore"):
            gl, gs = gradient(G[k], Z[k], scales[k])
            loc[k], m_loc[k], v_loc[k] = adam(loc[k], gl, m_loc[k], v_loc[k], t, lrs[k], b1, b2, eps)
            scales[k], m_s[k], v_s[k] = adam(scales[k], gs, m_s[k], v_s[k], t, lrs[k], b1, b2, eps)
    out = (loc, scales, (m_loc, v_loc, m_s, v_s))
    if Znext is None:
        return out
    with np.errstate(all="ignore"):
        nx = [sample(loc[k], scales[k], Znext[k]) for k in range(K)]
    return out + (np.stack([o[0] for o in nx]), np.array([o[1] for o in nx]))


def fit(keys, lp, lp_g, lr, mean, cov, B, niter, b1=0.9, b2=0.999, eps=1e-8, forced_z=None):
    """the loop of ADVIBatch.fit for K problems: lp (K, B, D) -> (K,) sums (or None), lp_g (K, B, D) -> (K, B, D); lr a float, K
    values or a callable of the iteration; returns (loc, cov, losses (niter + 1, K))"""
    K, D = mean.shape
    z = (lambda i: np.stack([draw(keys[k], i, B, D) for k in range(K)])) if forced_z is None else (lambda i: forced_z[i])
    Z = z(0)
    scales, X, logq = init(mean, cov, Z)
    loc = np.array(mean, copy=True)
    moments = (np.zeros((K, D)), np.zeros((K, D)), np.zeros((K, tri(D))), np.zeros((K, tri(D))))
    losses = np.zeros((niter + 1, K))
    for i in range(niter + 1):
        G = lp_g(X)
        if lp is not None:
            losses[i] = logq - lp(X)
        Zn = z(i + 1) if i < niter else None
        out = step(G, Z, loc, scales, moments, i + 1, lr(i) if callable(lr) else lr, b1, b2, eps, Znext=Zn)
        loc, scales, moments = out[:3]
        if Zn is not None:
            X, logq, Z = out[3], out[4], Zn
    return loc, cov_of(scales, D), losses


def gaussian_targets(K, D, seed=0):
    ms, Ps = [], []
    for k in range(K):
        m, _, P = orc.make_gaussian_target(D, 100 * seed + k)
        ms.append(m)
        Ps.append(0.5 * (P + P.T))
    return np.array(ms), np.array(Ps)


def gaussian_lp(ms, Ps):
    """(K, rows, D) -> (K,) sums of -1/2 (x - m_k)^T P_k (x - m_k), the density of BatchedGaussianTarget.lp"""
    def lp(X):
        r = ms[:, None, :] - np.asarray(X)
        return -0.5 * np.einsum("kbi,kij,kbj->k", r, Ps, r)
    return lp


def gaussian_score(ms, Ps):
    def lp_g(X):
        return np.stack([orc.gaussian_score(X[k], ms[k], Ps[k]) for k in range(X.shape[0])])
    return lp_g


def torch_advi_run(m, P, seed, lr, B, nsteps, mean0=None, cov0=None):
    """The package's single-problem ``ADVI.neg_elbo`` (torch autograd) + ``torch.optim.Adam`` on the CPU for one Gaussian target
    N(m, P^-1), fed the draws ``draw(seed, i, B, D)`` in place of ``torch.randn``: returns (loc, scales, losses) after
    ``nsteps`` steps and the gradient of the first step."""
    import torch
    from gsmvi_amd.advi import ADVI
    D = m.shape[0]
    mt, Pt = torch.tensor(m), torch.tensor(P)

    def lp(x):
        r = x - mt[None, :]
        return -0.5 * torch.einsum("bi,ij,bj->b", r, Pt, r)

    advi = ADVI(D, lp, device="cpu")
    mean0 = np.zeros(D) if mean0 is None else mean0
    cov0 = np.eye(D) if cov0 is None else cov0
    loc = torch.tensor(mean0, dtype=torch.float64, requires_grad=True)
    scales = torch.tensor(np.linalg.cholesky(cov0)[np.tril_indices(D)], dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([loc, scales], lr=lr)
    losses, g0 = [], None
    for i in range(nsteps):
        z = torch.tensor(draw(seed, i, B, D))
        opt.zero_grad(set_to_none=True)
        with mock.patch.object(torch, "randn", lambda *a, **kw: z):
            loss = advi.neg_elbo([loc, scales], None, B)
        loss.backward()
        if g0 is None:
            g0 = (loc.grad.numpy().copy(), scales.grad.numpy().copy())
        opt.step()
        losses.append(float(loss.detach()))
    return loc.detach().numpy().copy(), scales.detach().numpy().copy(), np.array(losses), g0
