"""The latent projection on the MI355X: kNN at size against float64 brute force, embedding quality and determinism of
latent_projection.umap_project, VAE.project_latent at 41x49x35, and the CLI's --recons_only export with the projection."""
import os

import numpy as np
import pytest
import torch

import vae_gam_amd  # noqa: F401
from vae_gam_amd import _lib
from vae_gam_amd import latent_projection as LP

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def hip_lib():
    assert torch.cuda.is_available()
    import emu_inject; emu_inject.use_product_library()
    _lib.get_lib()
    yield


def test_knn_20000_points_matches_float64_brute_force():
    N, D, k = 20000, 32, 20
    x = np.random.default_rng(0).normal(size=(N, D)).astype(np.float32)
    idx, dist = LP.knn(torch.from_numpy(x).cuda(), k)
    torch.cuda.synchronize()
    idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
    assert (idx[:, 0] == np.arange(N)).all() and (dist[:, 0] == 0).all()
    xt = torch.from_numpy(x).double()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    for q0 in range(0, N, 2000):
        d = torch.cdist(xt[q0:q0 + 2000], xt)
        d[torch.arange(d.shape[0]), torch.arange(q0, q0 + d.shape[0])] = -1.0          # self first, as the kernel puts it
        rd1, ri1 = torch.topk(d, k + 1, largest=False, sorted=True)          # one more: the first point OUTSIDE the list
        rd1, ri1 = rd1.numpy(), ri1.numpy(); rd1[:, 0] = 0.0
        rd, ri = rd1[:, :k], ri1[:, :k]
        g_d, g_i = dist[q0:q0 + 2000], idx[q0:q0 + 2000]
        np.testing.assert_allclose(g_d, rd, rtol=1e-5, atol=1e-5)
        # indices must agree wherever the neighbouring reference distances (the next point outside the list included) differ by
        # more than 1e-5 relative
        lo = np.concatenate([np.full((rd.shape[0], 1), -np.inf), rd[:, :-1]], 1)
        hi = rd1[:, 1:]
        sep = 1e-5 * np.maximum(rd, 1e-30)
        sel = (rd - lo > sep) & (hi - rd > sep)
        assert sel[:, 1:].mean() > 0.99
        np.testing.assert_array_equal(g_i[sel], ri[sel])


def blobs(n=5000, d=32, c=10, seed=0):
    rng = np.random.default_rng(seed)
    centers = rng.normal(scale=10.0, size=(c, d))
    labels = np.arange(n) % c
    return (centers[labels] + rng.normal(size=(n, d))).astype(np.float32), labels


def test_umap_quality_on_separated_blobs():
    from sklearn.manifold import trustworthiness
    from sklearn.neighbors import NearestNeighbors
    x, labels = blobs()
    proj = LP.umap_project(torch.from_numpy(x).cuda()).cpu().numpy()
    assert proj.shape == (5000, 2) and np.isfinite(proj).all()
    t = trustworthiness(x, proj, n_neighbors=20)
    nb = NearestNeighbors(n_neighbors=6).fit(proj).kneighbors(proj, return_distance=False)[:, 1:]
    votes = labels[nb]
    pred = np.array([np.bincount(v, minlength=10).argmax() for v in votes])
    acc = (pred == labels).mean()
    assert t >= 0.90 and acc >= 0.98, (t, acc)


def test_umap_is_deterministic_and_seeded():
    x, _ = blobs(n=3000, seed=1)
    xt = torch.from_numpy(x).cuda()
    a = LP.umap_project(xt, random_state=7).cpu().numpy()
    b = LP.umap_project(xt, random_state=7).cpu().numpy()
    c = LP.umap_project(xt, random_state=8).cpu().numpy()
    np.testing.assert_array_equal(a, b)
    assert not np.array_equal(a, c)


def test_project_latent_writes_pdf_and_csv(tmp_path):
    import pandas as pd
    from vae_gam_amd import DataClass_GP, synthetic
    from vae_gam_amd.vae_reg_GP import VAE
    ds = synthetic.make_dataset(num_subjects=2, vols_per_subject=15, num_covariates=8, seed=3)
    csv, _ = synthetic.write_csvs(ds, str(tmp_path))
    torch.manual_seed(1)
    m = VAE(num_covariates=8, glm_maps=ds['glm'], xu_ranges=ds['xu_ranges'], device_name='cuda', save_dir=str(tmp_path))
    loaders = DataClass_GP.setup_data_loaders(batch_size=8, train_csv=csv, test_csv=csv)
    latent, proj = m.project_latent(loaders, str(tmp_path), title='Latent Space plot', split=15)
    assert latent.shape == (30, m.num_latents) and proj.shape == (30, 2) and np.isfinite(proj).all()
    with torch.no_grad():
        mu = torch.cat([m.encode(b['volume'].cuda())[0] for b in loaders['UnShuffled_train']]).cpu().numpy()
    np.testing.assert_array_equal(latent, mu)
    assert os.path.getsize(str(tmp_path / '000_temp.pdf')) > 0
    df = pd.read_csv(str(tmp_path / '000_latent_projection.csv'))
    assert df.shape == (30, m.num_latents + 4) and sorted(set(df['subjid'])) == [0, 1]


def test_cli_recons_only_writes_the_latent_projection(tmp_path):
    import pandas as pd
    from vae_gam_amd import multsubj_reg_run_GP as cli, synthetic
    ds = synthetic.make_dataset(num_subjects=2, vols_per_subject=6, num_covariates=8, seed=3)
    csv, glm_csv = synthetic.write_csvs(ds, str(tmp_path / 'data'))
    out1, out2 = str(tmp_path / 'run1'), str(tmp_path / 'run2')
    cli.main(['--train_csv', csv, '--test_csv', csv, '--glm_maps', glm_csv, '--save_dir', out1, '--batch-size', '4',
              '--epochs', '2', '--save_freq', '1', '--test_freq', '1'])
    assert os.path.exists(os.path.join(out1, '002_temp.pdf'))
    m2 = cli.main(['--train_csv', csv, '--test_csv', csv, '--glm_maps', glm_csv, '--save_dir', out2, '--batch-size', '4',
                   '--from_ckpt', 'True', '--ckpt_path', os.path.join(out1, 'checkpoint_001.tar'), '--recons_only', 'True'])
    assert m2.epoch == 2
    assert os.path.getsize(os.path.join(out2, '002_temp.pdf')) > 0
    df = pd.read_csv(os.path.join(out2, '002_latent_projection.csv'))
    assert len(df) == 12 and df.shape[1] == m2.num_latents + 4
