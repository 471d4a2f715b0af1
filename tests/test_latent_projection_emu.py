"""The latent projection (VAE.project_latent; vae_gam_amd.latent_projection) on the host build of its HIP kernels (tests/emu): kNN,
fuzzy set and layout epochs against numpy restatements of include/vaegam.h, the host-side graph logic, and project_latent at the
21x21x21 toy geometry.  No GPU needed; tests/test_latent_projection_gpu.py repeats the kernels at size on the real library."""
import os

import numpy as np
import pandas as pd
import pytest
import torch

import toy_case as T
from vae_gam_amd import _lib
from vae_gam_amd import latent_projection as LP


@pytest.fixture(scope='module', autouse=True)
def emu():
    prev = _lib._LIB
    T.load_emu_library()
    yield
    _lib._LIB = prev


# ----------------------------------------------------------------------------------------------------------- numpy restatements
def ref_knn(x, k):
    x = x.astype(np.float64)
    d = np.sqrt(((x[:, None, :] - x[None, :, :]) ** 2).sum(-1))
    N = len(x)
    idx = np.zeros((N, k), np.int64); dist = np.zeros((N, k))
    for i in range(N):
        o = [j for j in np.lexsort((np.arange(N), d[i])) if j != i][:k - 1]
        idx[i] = [i] + o; dist[i] = [0.0] + list(d[i, o])
    return idx, dist


def ref_fuzzy(idx, dist):
    dist = dist.astype(np.float64)
    N, k = dist.shape
    mean_all = dist.mean()
    target = np.log2(k)
    rho = np.zeros(N); sigma = np.zeros(N); w = np.zeros((N, k))
    for i in range(N):
        nz = dist[i][dist[i] > 0]
        r = nz.min() if len(nz) else 0.0
        lo, hi, mid = 0.0, np.inf, 1.0
        for _ in range(64):
            t = dist[i, 1:] - r
            psum = np.where(t > 0, np.exp(-(np.maximum(t, 0) / mid)), 1.0).sum()
            if abs(psum - target) < 1e-5:
                break
            if psum > target:
                hi = mid; mid = (lo + hi) / 2.0
            else:
                lo = mid; mid = mid * 2.0 if hi == np.inf else (lo + hi) / 2.0
        mid = max(mid, 1e-3 * (dist[i].mean() if r > 0 else mean_all))
        rho[i], sigma[i] = r, mid
        for j in range(k):
            t = dist[i, j] - r
            w[i, j] = 0.0 if idx[i, j] == i else (1.0 if (t <= 0 or mid == 0) else np.exp(-t / mid))
    return rho, sigma, w


M64 = (1 << 64) - 1


def splitmix64(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def ref_epoch(y, rowptr, col, eps, n, n_epochs, a, b, neg, seed):
    f = np.float32
    N = len(y)
    a, b = f(a), f(b)
    alpha = f(1) - f(n) / f(n_epochs)
    out = y.copy()
    two_ab, bm1, two_b = f(-2) * a * b, b - f(1), f(2) * b
    sk = (seed * 0x9E3779B97F4A7C15) & M64

    def clip(v):
        return min(max(v, f(-4)), f(4))

    for i in range(N):
        ox, oy = y[i, 0], y[i, 1]
        if n >= 1:
            for e in range(rowptr[i], rowptr[i + 1]):
                ep = float(eps[e])
                if not (np.floor(n / ep) > np.floor((n - 1) / ep)):
                    continue
                j = col[e]
                dx, dy = y[i, 0] - y[j, 0], y[i, 1] - y[j, 1]
                d2 = dx * dx + dy * dy
                if d2 > 0:
                    coef = (two_ab * np.power(d2, bm1)) / (a * np.power(d2, b) + f(1))
                    gx, gy = alpha * clip(coef * dx), alpha * clip(coef * dy)
                    ox = ox + gx; oy = oy + gy
                    ox = ox + gx; oy = oy + gy
                for s in range(neg):
                    kk = splitmix64(((((n << 44) | (e << 5)) | s) + sk) & M64) % N
                    if kk == i:
                        continue
                    dx, dy = y[i, 0] - y[kk, 0], y[i, 1] - y[kk, 1]
                    d2 = dx * dx + dy * dy
                    if not d2 > 0:
                        continue
                    coef = two_b / ((f(0.001) + d2) * (a * np.power(d2, b) + f(1)))
                    ox = ox + alpha * clip(coef * dx); oy = oy + alpha * clip(coef * dy)
        out[i, 0], out[i, 1] = ox, oy
    return out


def check_knn(x, k, idx, dist):
    ri, rd = ref_knn(x, k)
    n_out = ref_knn(x, min(k + 1, len(x)))[1]                       # the first point outside the list bounds the last position
    np.testing.assert_allclose(dist, rd, rtol=1e-5, atol=1e-5)
    assert (idx[:, 0] == np.arange(len(x))).all() and (dist[:, 0] == 0).all()
    # indices must agree wherever the neighbouring reference distances are separated by more than 1e-5 relative
    for i in range(len(x)):
        for j in range(1, k):
            lo = rd[i, j - 1] if j > 1 else -np.inf
            hi = rd[i, j + 1] if j + 1 < k else (n_out[i, k] if k < len(x) else np.inf)
            sep = 1e-5 * max(rd[i, j], 1e-30)
            if rd[i, j] - lo > sep and hi - rd[i, j] > sep:
                assert idx[i, j] == ri[i, j], (i, j, idx[i], ri[i])


# ----------------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize('D,k', [(32, 20), (7, 5)])
def test_knn_matches_numpy_brute_force(D, k):
    rng = np.random.default_rng(D * 100 + k)
    x = rng.normal(size=(300, D)).astype(np.float32)
    idx, dist = LP.knn(torch.from_numpy(x), k)
    assert idx.dtype == torch.int32 and dist.dtype == torch.float32 and idx.shape == (300, k)
    check_knn(x, k, idx.numpy(), dist.numpy())


def test_knn_duplicates_self_first_and_ties_to_lower_index():
    rng = np.random.default_rng(3)
    base = rng.normal(size=(40, 6)).astype(np.float32)
    x = np.concatenate([base, base[:10], base[:10]])               # points 0..9 appear three times each
    N, k = len(x), 8
    idx, dist = LP.knn(torch.from_numpy(x), k)
    idx, dist = idx.numpy(), dist.numpy()
    assert (idx[:, 0] == np.arange(N)).all() and (dist[:, 0] == 0).all()
    for i in range(10):
        copies = [i, 40 + i, 50 + i]
        for c in copies:                                            # the two other copies next, at distance 0, lower index first
            assert list(idx[c, 1:3]) == [o for o in copies if o != c] and (dist[c, 1:3] == 0).all()
    check_knn(x, k, idx, dist)


def test_knn_k_equal_n_and_k_one():
    x = np.random.default_rng(4).normal(size=(12, 3)).astype(np.float32)
    idx, dist = LP.knn(torch.from_numpy(x), 12)
    check_knn(x, 12, idx.numpy(), dist.numpy())
    idx, dist = LP.knn(torch.from_numpy(x), 1)
    assert (idx.numpy()[:, 0] == np.arange(12)).all() and (dist.numpy() == 0).all()


def test_fuzzy_rho_sigma_w_match_restatement():
    rng = np.random.default_rng(5)
    x = rng.normal(size=(120, 9)).astype(np.float32)
    x[100:110] = x[:10]                                             # duplicates: rho from the first NON-zero distance
    idx, dist = LP.knn(torch.from_numpy(x), 15)
    rho, sigma, w = LP.smooth_knn(idx, dist)
    rr, rs, rw = ref_fuzzy(idx.numpy(), dist.numpy())
    np.testing.assert_allclose(rho.numpy(), rr, rtol=1e-6)
    np.testing.assert_allclose(sigma.numpy(), rs, rtol=1e-6)
    np.testing.assert_allclose(w.numpy(), rw, atol=1e-6)
    assert (w.numpy()[:, 0] == 0).all()


def test_fuzzy_all_zero_rows_use_the_global_floor():
    x = np.zeros((6, 4), np.float32); x[5] = 1.0                    # rows 0..4: every neighbour at distance 0 except one
    idx, dist = LP.knn(torch.from_numpy(x), 4)
    rho, sigma, w = LP.smooth_knn(idx, dist)
    rr, rs, rw = ref_fuzzy(idx.numpy(), dist.numpy())
    np.testing.assert_allclose(rho.numpy(), rr, rtol=1e-6)
    np.testing.assert_allclose(sigma.numpy(), rs, rtol=1e-6)
    np.testing.assert_allclose(w.numpy(), rw, atol=1e-6)


def test_three_layout_epochs_match_restatement():
    rng = np.random.default_rng(6)
    x = np.concatenate([rng.normal(size=(30, 5)), rng.normal(size=(30, 5)) + 4]).astype(np.float32)
    N, n_epochs, seed = len(x), 50, 1234
    rows, cols, vals, rowptr, col, eps, n_epochs = LP.build_graph(torch.from_numpy(x), 10, n_epochs)
    a, b = LP.find_ab_params(1.0, 0.1)
    y = LP.normalise_layout(np.random.RandomState(0).uniform(-10, 10, size=(N, 2)).astype(np.float32))
    got = LP.layout(torch.from_numpy(y), rowptr, col, eps, 3, a, b, 5, seed).numpy()
    # the kernel was launched with n_epochs = 3 here: restate the same three epochs
    ref = y.copy()
    for n in range(3):
        ref = ref_epoch(ref, rowptr.numpy(), col.numpy(), eps.numpy(), n, 3, a, b, 5, seed)
    assert not np.array_equal(ref, y)
    np.testing.assert_allclose(got, ref, atol=1e-5)
    # and the first three of a longer schedule (alpha and the due edges depend on n_epochs)
    got = y.copy(); ref = y.copy()
    yt, yn = torch.from_numpy(y.copy()), torch.empty(N, 2)
    for n in range(3):
        _lib.get_lib().call('vg_umap_layout_epoch', LP._p(rowptr), LP._p(col), LP._p(eps), LP._p(yt), N, int(col.numel()), n,
                            n_epochs, a, b, 5, seed, LP._p(yn), None)
        yt, yn = yn, yt
        ref = ref_epoch(ref, rowptr.numpy(), col.numpy(), eps.numpy(), n, n_epochs, a, b, 5, seed)
    np.testing.assert_allclose(yt.numpy(), ref, atol=1e-5)


# ----------------------------------------------------------------------------------------------------------- host logic
def test_find_ab_params_reference_settings():
    a, b = LP.find_ab_params(1.0, 0.1)
    assert abs(a - 1.5769) < 1e-3 and abs(b - 0.8951) < 1e-3


def test_default_n_epochs_rule():
    assert LP.default_n_epochs(12) == 500 and LP.default_n_epochs(10000) == 500
    assert LP.default_n_epochs(10001) == 200 and LP.default_n_epochs(50000) == 200


def test_graph_is_symmetric_union_and_pruned():
    rng = np.random.default_rng(7)
    x = rng.normal(size=(80, 6)).astype(np.float32)
    idx, dist = LP.knn(torch.from_numpy(x), 10)
    _, _, w = LP.smooth_knn(idx, dist)
    rows, cols, vals = LP.fuzzy_simplicial_set(idx, dist)
    N = 80
    P = np.zeros((N, N), np.float32)
    for i in range(N):
        P[i, idx.numpy()[i]] = w.numpy()[i]
    Wr = (P + P.T) - P * P.T
    W = np.zeros((N, N), np.float32); W[rows.numpy(), cols.numpy()] = vals.numpy()
    np.testing.assert_allclose(W, Wr, atol=1e-7)
    np.testing.assert_array_equal(W, W.T)
    assert (vals.numpy() > 0).all()
    key = rows.numpy() * N + cols.numpy()
    assert (np.diff(key) > 0).all()                                 # sorted by (row, col), no duplicates
    n_epochs = 3
    pr, pc, pv = LP.prune_graph(rows, cols, vals, n_epochs)
    thr = vals.max().item() / n_epochs
    assert (pv.numpy() >= thr).all() and int((vals.numpy() < thr).sum()) == len(vals) - len(pv) > 0
    rowptr, col, eps = LP.to_csr(pr, pc, pv, N)
    assert rowptr[0] == 0 and rowptr[-1] == len(pv) and (np.diff(rowptr.numpy()) >= 0).all()
    np.testing.assert_allclose(eps.numpy(), (pv.max().double() / pv.double()).numpy(), rtol=1e-7)


def test_k_eff_for_fewer_points_than_neighbours():
    x = torch.from_numpy(np.random.default_rng(8).normal(size=(12, 5)).astype(np.float32))
    rows, cols, vals, rowptr, col, eps, n_epochs = LP.build_graph(x, 20)
    assert n_epochs == 500 and rowptr.numel() == 13
    y = LP.umap_project(x, n_epochs=5)
    assert y.shape == (12, 2) and y.dtype == torch.float32 and torch.isfinite(y).all()


# ----------------------------------------------------------------------------------------------------------- VAE.project_latent
def test_project_latent_toy_geometry(tmp_path):
    B, C = 4, 3
    _, cov, xu, glm = T.make_inputs(B, C, seed=11)
    model = T.make_model(C, xu, glm)
    model.epoch = 7
    batches = []
    for s in range(3):
        x, _, _, _ = T.make_inputs(B, C, seed=20 + s)
        batches.append({'volume': x, 'covariates': cov, 'subjid': torch.full((B,), s // 2, dtype=torch.int64),
                        'vol_num': torch.arange(B, dtype=torch.float64) + 4 * s})
    latent, proj = model.project_latent({'UnShuffled_train': batches}, str(tmp_path), title='Latent Space plot', split=5)
    L = model.num_latents
    assert latent.shape == (3 * B, L) and proj.shape == (3 * B, 2)
    with torch.no_grad():
        mu = torch.cat([model.encode(b['volume'])[0] for b in batches]).numpy()
    np.testing.assert_array_equal(latent, mu)
    df = pd.read_csv(os.path.join(str(tmp_path), '007_latent_projection.csv'))
    assert df.shape == (3 * B, L + 4)
    assert list(df.columns) == ['subjid', 'vol_num'] + ['mu_%d' % j for j in range(L)] + ['umap_0', 'umap_1']
    np.testing.assert_array_equal(df[['mu_%d' % j for j in range(L)]].to_numpy(np.float32), mu)
    np.testing.assert_array_equal(df[['umap_0', 'umap_1']].to_numpy(np.float32), proj)
    assert df['subjid'].tolist() == [0] * 8 + [1] * 4 and df['vol_num'].tolist() == list(range(12))
    try:
        import matplotlib  # noqa: F401
        assert os.path.getsize(os.path.join(str(tmp_path), '007_temp.pdf')) > 0
    except ImportError:
        pass
