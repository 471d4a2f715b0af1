"""Voxel-wise statistics of the effect maps and of the fit (an extension; the reference has first moments only, from re-read files).

`VAE.map_statistics` accumulates, per subject and voxel, the running sums that `ops.gam_stats_accumulate` forms on the device straight
from the decoder's logits (slot table: include/vaegam.h); a `MapStatistics` holds them and derives from them, in float64 on the device,
  - how stable a map is over the volumes of a subject (`subject_std`),
  - whether it is consistent across subjects (`group_t`: a one-sample t map over the subject means, df = S - 1),
  - where the model explains the data (`r2`, and `partial_r2`: what the fit loses when covariate i's contribution is taken out).
Every undefined value (too few volumes or subjects, no variance, a voxel outside the mask) is written as 0, never nan or inf.
"""
import torch


class MapStatistics:
    """acc: float64 [S, 3C+8, V] (vg_gam_stats_accumulate's layout), counts: float64 [S] volumes per subject, keys: the C+2 map names
    ['base', <img_key of covariate 1..C>, 'full_rec'] in slot order."""

    def __init__(self, acc, counts, keys, img_shape=None):
        keys = list(keys)
        C = len(keys) - 2
        assert C >= 0 and acc.dim() == 3 and acc.shape[1] == 3 * C + 8 and acc.dtype == torch.float64
        assert counts.shape == (acc.shape[0],) and counts.dtype == torch.float64
        self.acc, self.counts, self.keys, self.img_shape = acc, counts, keys, img_shape
        self.num_covariates = C

    # ------------------------------------------------------------------ raw sums, (S, V) each
    @property
    def num_subjects(self):
        return int(self.acc.shape[0])

    def _slot(self, key):
        if key not in self.keys:
            raise KeyError('no map %r (have %s)' % (key, ', '.join(self.keys)))
        return self.keys.index(key)

    def _cov(self, key):
        j = self._slot(key)
        if not 1 <= j <= self.num_covariates:
            raise KeyError('%r is not a covariate map (have %s)' % (key, ', '.join(self.keys[1:-1])))
        return j - 1

    def sum(self, key):
        return self.acc[:, self._slot(key)]

    def sum_sq(self, key):
        return self.acc[:, self.num_covariates + 2 + self._slot(key)]

    def _fit(self, k):                                   # 0 sum x, 1 sum x^2, 2 sum r, 3 sum r^2
        return self.acc[:, 2 * self.num_covariates + 4 + k]

    def _n(self):
        return self.counts.clamp_min(1.0).unsqueeze(1)   # (a subject without volumes has sums of 0: its means are 0)

    # ------------------------------------------------------------------ per subject, (S, V) each
    def subject_mean(self, key):
        return self.sum(key) / self._n()

    def subject_std(self, key):
        """sqrt(max(0, sum m^2 - (sum m)^2 / n) / (n - 1)); 0 for a subject with fewer than 2 volumes"""
        n = self.counts.unsqueeze(1)
        ss = (self.sum_sq(key) - self.sum(key) ** 2 / self._n()).clamp_min(0.0)
        sd = (ss / (n - 1.0).clamp_min(1.0)).sqrt()
        return torch.where(n >= 2.0, sd, torch.zeros_like(sd))

    def residual_mean(self):
        return self._fit(2) / self._n()

    def _sst(self):
        """sum x^2 - (sum x)^2 / n, with what is within the rounding of that one-pass form (8 n 2^-52 sum x^2: data that never varies)
        set to exactly 0"""
        sxx = self._fit(1)
        sst = sxx - self._fit(0) ** 2 / self._n()
        return torch.where(sst > 8.0 * 2.0 ** -52 * self._n() * sxx, sst, torch.zeros_like(sst))

    @staticmethod
    def _over_sst(num, sst):
        ok = sst > 0
        return torch.where(ok, num / torch.where(ok, sst, torch.ones_like(sst)), torch.zeros_like(sst))

    def r2(self):
        """1 - sum r^2 / SST with SST = sum x^2 - (sum x)^2 / n; 0 where SST <= 0"""
        sst = self._sst()
        return self._over_sst(sst - self._fit(3), sst)

    def partial_r2(self, key):
        """(sum (r + cons_i)^2 - sum r^2) / SST: the share of the data's variance the fit loses without covariate i; 0 where SST <= 0"""
        i = self._cov(key)
        return self._over_sst(self.acc[:, 2 * self.num_covariates + 8 + i] - self._fit(3), self._sst())

    # ------------------------------------------------------------------ across subjects, (V,) each
    def group_mean(self, key):
        """mean of the subject means, as build_model_recons.mk_avg_maps"""
        return self.subject_mean(key).mean(0)

    def group_r2(self):
        return self.r2().mean(0)

    def group_t(self, key):
        """one-sample t over the subject means: mean / (sd / sqrt(S)), sd with S - 1 degrees of freedom; 0 for S < 2 or sd = 0"""
        m = self.subject_mean(key)
        S = m.shape[0]
        mean = m.mean(0)
        if S < 2:
            return torch.zeros_like(mean)
        ss = ((m - mean) ** 2).sum(0)
        sd = ss.div(S - 1).sqrt()
        ok = ss > (2.0 ** -50) ** 2 * (m ** 2).sum(0)            # (subject means that agree to the rounding of their own mean: sd = 0)
        return torch.where(ok, mean / (torch.where(ok, sd, torch.ones_like(sd)) / S ** 0.5), torch.zeros_like(mean))
