"""UMAP projection of the latent means (the reference's project_latent, vae_reg_GP.py:542-583: n_components 2, n_neighbors 20,
min_dist 0.1, Euclidean, random_state 42), computed on the MI355X without umap-learn.

The three O(N^2 D) / O(epochs * edges) phases are HIP kernels (include/vaegam.h):
  vg_knn               exact k nearest neighbours;
  vg_umap_fuzzy        rho, sigma and the membership strengths of every neighbour row;
  vg_umap_layout_epoch one synchronous negative-sampling SGD epoch of the 2-D layout.
The rest is plumbing: the union of the fuzzy sets and the CSR graph (torch on the device, once), the a/b curve fit and the spectral
initialisation (scipy on the host, float64, once).  Deliberate differences to umap-learn: the epoch is a Jacobi
update (every contribution of epoch n reads Y_n), and every due edge draws exactly `negative_sample_rate` negatives.
"""
import ctypes
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from .ops import _call, _p


def default_n_epochs(n):
    """umap-learn's rule: 500 epochs up to 10,000 points, 200 above."""
    return 500 if n <= 10000 else 200


KnnPlan = namedtuple('KnnPlan', _lib.KNN_PLAN_FIELDS)


def knn_plan(N, D, k) -> KnnPlan:
    """What knn launches for N points of D dimensions and k neighbours, from vg_knn's own planner (vg_knn_plan): nothing is launched.
    KB: places of the register list of the kernel instance (0: k = 1, no partial launch), S splits of `chunk` candidates, `last` of them
    in the last split, Dp the padded D, qblocks blocks of 256 queries, lds_bytes of the partial kernel.  A bad shape raises VgError."""
    rec = (ctypes.c_int32 * len(KnnPlan._fields))()
    _lib.get_lib().call('vg_knn_plan', int(N), int(D), int(k), rec, len(rec))
    return KnnPlan(*rec)


def knn(latent, k):
    """latent (N, D) -> (idx (N, k) int32, dist (N, k) fp32): exact Euclidean neighbours, self at position 0, the rest sorted by
    (distance, index)."""
    x = latent.to(torch.float32).contiguous()
    N, D = x.shape
    k = int(k)
    ws_bytes = _lib.get_lib().size('vg_knn_ws_bytes', N, D, k)
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=x.device)
    idx = torch.empty(N, k, dtype=torch.int32, device=x.device)
    dist = torch.empty(N, k, dtype=torch.float32, device=x.device)
    _call(x, 'vg_knn', _p(x), N, D, k, _p(ws), _p(idx), _p(dist))
    return idx, dist


def smooth_knn(idx, dist):
    """-> (rho (N,), sigma (N,), w (N, k)) fp32: the fuzzy simplicial set of every neighbour row (local_connectivity 1)."""
    idx = idx.to(torch.int32).contiguous(); dist = dist.to(torch.float32).contiguous()
    N, k = dist.shape
    ws = torch.empty(256, dtype=torch.float64, device=dist.device)
    rho = torch.empty(N, dtype=torch.float32, device=dist.device)
    sigma = torch.empty_like(rho)
    w = torch.empty_like(dist)
    _call(dist, 'vg_umap_fuzzy', _p(dist), _p(idx), N, k, _p(ws), _p(rho), _p(sigma), _p(w))
    return rho, sigma, w


def fuzzy_simplicial_set(idx, dist):
    """-> the symmetric W = P + P^T - P o P^T as a COO (rows int64, cols int64, vals fp32), sorted by (row, col), zeros dropped.
    P[i, idx[i, j]] = w[i, j] from smooth_knn."""
    _, _, w = smooth_knn(idx, dist)
    N, k = w.shape
    dev = w.device
    r = torch.arange(N, device=dev, dtype=torch.int64).repeat_interleave(k)
    c = idx.reshape(-1).to(torch.int64)
    v = w.reshape(-1)
    keys = torch.cat([r * N + c, c * N + r])                     # P, then P^T
    vals = torch.cat([v, v])
    keys, order = torch.sort(keys, stable=True)
    vals = vals[order]
    uniq, counts = torch.unique_consecutive(keys, return_counts=True)
    start = torch.cumsum(counts, 0) - counts
    a = vals[start]
    pair = counts == 2                                          # (i, j) in both P and P^T (each neighbour list holds j once)
    b = torch.where(pair, vals[torch.clamp(start + 1, max=vals.numel() - 1)], torch.zeros_like(a))
    W = torch.where(pair, (a + b) - a * b, a)
    keep = W > 0
    uniq, W = uniq[keep], W[keep]
    return uniq // N, uniq % N, W


def prune_graph(rows, cols, vals, n_epochs):
    """Drop the edges below max(W) / n_epochs (they would never be sampled)."""
    if vals.numel() == 0:
        return rows, cols, vals
    keep = vals >= vals.max() / float(n_epochs)
    return rows[keep], cols[keep], vals[keep]


def to_csr(rows, cols, vals, N):
    """Sorted COO -> (rowptr (N+1,) int32, col (nnz,) int32, epochs_per_sample (nnz,) fp32 = max(W) / w)."""
    rowptr = torch.searchsorted(rows, torch.arange(N + 1, device=rows.device, dtype=torch.int64)).to(torch.int32)
    eps = (vals.max().double() / vals.double()).float() if vals.numel() else vals.clone()
    return rowptr.contiguous(), cols.to(torch.int32).contiguous(), eps.contiguous()


def find_ab_params(spread=1.0, min_dist=0.1):
    """Least-squares fit of 1 / (1 + a x^(2b)) to 1 below min_dist and exp(-(x - min_dist) / spread) above it (umap-learn)."""
    from scipy.optimize import curve_fit

    def curve(x, a, b):
        return 1.0 / (1.0 + a * x ** (2 * b))

    xv = np.linspace(0, spread * 3, 300)
    yv = np.zeros(xv.shape)
    yv[xv < min_dist] = 1.0
    yv[xv >= min_dist] = np.exp(-(xv[xv >= min_dist] - min_dist) / spread)
    params, _ = curve_fit(curve, xv, yv)
    return float(params[0]), float(params[1])


def spectral_init(rows, cols, vals, N, random_state):
    """-> ((N, 2) float32 initial layout, name of the initialisation that ran).  Eigenvectors 2..3 of the normalised Laplacian
    I - D^-1/2 W D^-1/2, scaled to max |Y| = 10 plus N(0, 1e-4) noise; uniform(-10, 10) when the graph has more than one connected
    component, N <= 4, or the eigensolver does not converge."""
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components
    from scipy.sparse.linalg import ArpackError, ArpackNoConvergence, eigsh
    rng = np.random.RandomState(random_state)
    W = sp.coo_matrix((vals.double().cpu().numpy(), (rows.cpu().numpy(), cols.cpu().numpy())), shape=(N, N)).tocsr()
    how = 'random'
    if N > 4 and connected_components(W, directed=False)[0] == 1:
        deg = np.asarray(W.sum(axis=0)).ravel()
        Dm = sp.diags(1.0 / np.sqrt(deg))
        L = sp.identity(N, dtype=np.float64) - Dm @ W @ Dm
        k = 3
        try:
            ev, vec = eigsh(L, k, which='SM', ncv=min(N, max(2 * k + 1, int(np.sqrt(N)))), tol=1e-4, v0=rng.normal(size=N),
                            maxiter=N * 5)
            Y = vec[:, np.argsort(ev)[1:k]]
            Y = (Y * (10.0 / np.abs(Y).max())).astype(np.float32) + rng.normal(scale=0.0001, size=(N, 2)).astype(np.float32)
            how = 'spectral'
        except (ArpackNoConvergence, ArpackError):
            pass
    if how == 'random':
        Y = rng.uniform(low=-10.0, high=10.0, size=(N, 2)).astype(np.float32)
    return Y, how


def normalise_layout(Y):
    """Min-max each coordinate to [0, 10] (umap-learn does this before the layout); a constant coordinate becomes 0."""
    lo, hi = Y.min(0), Y.max(0)
    rng = np.where(hi > lo, hi - lo, 1.0)
    return (10.0 * (Y - lo) / rng).astype(np.float32)


def layout(y0, rowptr, col, eps, n_epochs, a, b, negative_sample_rate=5, seed=0):
    """n_epochs launches of vg_umap_layout_epoch on the current stream, ping-ponging two buffers; no host synchronisation."""
    y = y0.to(torch.float32).contiguous().clone()
    y_next = torch.empty_like(y)
    N, nnz = y.shape[0], int(col.numel())
    for n in range(int(n_epochs)):
        _call(y, 'vg_umap_layout_epoch', _p(rowptr), _p(col), _p(eps), _p(y), N, nnz, n, int(n_epochs), float(a), float(b),
              int(negative_sample_rate), int(seed) & 0xFFFFFFFFFFFFFFFF, _p(y_next))
        y, y_next = y_next, y
    return y


def build_graph(latent, n_neighbors=20, n_epochs=None):
    """kNN -> fuzzy set -> pruned symmetric CSR.  -> (rows, cols, vals, rowptr, col, eps, n_epochs)."""
    N = latent.shape[0]
    k = min(int(n_neighbors), N)
    n_epochs = default_n_epochs(N) if n_epochs is None else int(n_epochs)
    idx, dist = knn(latent, k)
    rows, cols, vals = prune_graph(*fuzzy_simplicial_set(idx, dist), n_epochs)
    rowptr, col, eps = to_csr(rows, cols, vals, N)
    return rows, cols, vals, rowptr, col, eps, n_epochs


def umap_project(latent, n_neighbors=20, min_dist=0.1, spread=1.0, n_epochs=None, negative_sample_rate=5, random_state=42,
                 init='spectral'):
    """latent (N, D) device tensor -> (N, 2) fp32 device tensor: the UMAP embedding with the reference's settings.
    init: 'spectral' (falls back to 'random' where umap-learn would) or 'random'."""
    if init not in ('spectral', 'random'):
        raise ValueError("init must be 'spectral' or 'random', got %r" % (init,))
    if latent.dim() != 2 or latent.shape[0] < 1:
        raise ValueError('latent must be (N, D) with N >= 1, got %s' % (tuple(latent.shape),))
    N = latent.shape[0]
    seed = int(np.random.randint(2 ** 31)) if random_state is None else int(random_state)
    rows, cols, vals, rowptr, col, eps, n_epochs = build_graph(latent, n_neighbors, n_epochs)
    a, b = find_ab_params(spread, min_dist)
    if init == 'spectral':
        Y, how = spectral_init(rows, cols, vals, N, seed)
    else:
        Y, how = np.random.RandomState(seed).uniform(low=-10.0, high=10.0, size=(N, 2)).astype(np.float32), 'random'
    print('[latent_projection] N %d, k %d, %d edges, %d epochs, %s initialisation' % (N, min(int(n_neighbors), N), col.numel(),
                                                                                       n_epochs, how))
    y0 = torch.from_numpy(normalise_layout(Y)).to(latent.device)
    return layout(y0, rowptr, col, eps, n_epochs, a, b, negative_sample_rate, seed)
