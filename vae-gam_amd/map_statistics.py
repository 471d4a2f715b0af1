"""Voxel-wise statistics of the effect maps and of the fit (an extension; the reference has first moments only, from re-read files).

`VAE.map_statistics` accumulates, per subject and voxel, the running sums that `ops.gam_stats_accumulate` forms on the device straight
from the decoder's logits (slot table: include/vaegam.h); a `MapStatistics` holds them and derives from them, in float64 on the device,
  - how stable a map is over the volumes of a subject (`subject_std`),
  - whether it is consistent across subjects (`group_t`: a one-sample t map over the subject means, df = S - 1),
  - where the model explains the data (`r2`, and `partial_r2`: what the fit loses when covariate i's contribution is taken out).
Every undefined value (too few volumes or subjects, no variance, a voxel outside the mask) is written as 0, never nan or inf.
"""
import torch


class NoVoxelError(ValueError):
    """group_permutation: the group statistic of the map is defined at no voxel"""


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

    @staticmethod
    def _group_spread(m):
        """-> (mean, ss, sum m^2, ok) of subject means m (S, V), S >= 2: ss the sum of squared deviations from the mean, ok where the
        group statistics are defined (the subject means do not agree to the rounding of their own mean)"""
        mean = m.mean(0)
        ss = ((m - mean) ** 2).sum(0)
        sq = (m ** 2).sum(0)
        return mean, ss, sq, ss > (2.0 ** -50) ** 2 * sq

    def group_t(self, key):
        """one-sample t over the subject means: mean / (sd / sqrt(S)), sd with S - 1 degrees of freedom; 0 for S < 2 or sd = 0"""
        m = self.subject_mean(key)
        S = m.shape[0]
        if S < 2:
            return torch.zeros_like(m.mean(0))
        mean, ss, _, ok = self._group_spread(m)
        sd = ss.div(S - 1).sqrt()
        return torch.where(ok, mean / (torch.where(ok, sd, torch.ones_like(sd)) / S ** 0.5), torch.zeros_like(mean))

    def group_permutation(self, key, n_perm=10000, seed=0, tail='two'):
        """Sign-flip permutation test of the group map with the max-statistic (as FSL randomise / SnPM; ops.signflip_maxstat): under the
        null the sign of each subject's mean map is exchangeable; every permutation flips a set of subjects and records the largest
        statistic over the voxels, and a voxel's family-wise-error corrected p is the share of those maxima that reach its own
        statistic.  Statistic: u = sum_s m / sqrt(S sum_s m^2), strictly increasing in the one-sample t (t = u sqrt((S-1) / (1-u^2))),
        so every rank and p-value is that of t; tail 'two' tests |t|, 'pos' t, 'neg' -t.  A voxel where group_t is undefined takes no
        part: its p-values are 1 and its statistic is 0.
        2^S <= n_perm: every one of the 2^S sign patterns, once (exhaustive).  Otherwise n_perm patterns: the identity and n_perm - 1
        drawn from torch's CPU generator seeded with `seed` (the same patterns on every device).  -> GroupPermutation."""
        from . import _lib, ops
        if tail not in _lib.SIGNFLIP_TAILS:
            raise ValueError('group_permutation: tail must be one of %s, not %r' % (', '.join(_lib.SIGNFLIP_TAILS), tail))
        m = self.subject_mean(key).contiguous()
        S = int(m.shape[0])
        n_perm = int(n_perm)
        if S < 2 or S > 64:
            raise ValueError('group_permutation: needs 2 to 64 subjects, not %d' % S)
        if n_perm < 1 or n_perm > 2 ** 20:
            raise ValueError('group_permutation: n_perm must be 1 to 2^20, not %d' % n_perm)
        _, _, sq, ok = self._group_spread(m)
        if not bool(ok.any()):
            raise NoVoxelError('group_permutation: the group statistic of %r is defined at no voxel' % (key,))
        scale = torch.where(ok, 1.0 / torch.where(ok, sq * S, torch.ones_like(sq)).sqrt(), torch.zeros_like(sq))
        exhaustive = 2 ** S <= n_perm
        if exhaustive:
            signs = torch.arange(2 ** S, dtype=torch.int64)
        else:
            bits = torch.randint(0, 2, (n_perm - 1, S), generator=torch.Generator('cpu').manual_seed(int(seed)))
            words = (bits << torch.arange(S, dtype=torch.int64)).sum(1)              # (distinct bits: the sum is their union, also at bit 63)
            signs = torch.cat([torch.zeros(1, dtype=torch.int64), words])
        signs = signs.to(m.device)
        stat, max_stat, cnt = ops.signflip_maxstat(m, scale, signs, tail)
        P = int(signs.shape[0])
        n = torch.full((), float(P), dtype=torch.float64, device=m.device)              # (a tensor: a true division on every device; by a
        p_unc = cnt.to(torch.float64) / n                                                #  Python number the GPU multiplies by 1 / P)
        below = torch.searchsorted(max_stat.sort().values, stat, right=False)        # maxima strictly below the voxel's statistic
        p_fwe = torch.where(ok, (P - below).to(torch.float64) / n, torch.ones_like(stat))
        return GroupPermutation(t=self.group_t(key), scale=scale, stat=stat, max_stat=max_stat, signs=signs, p_unc=p_unc, p_fwe=p_fwe, n_perm=P,
                                exhaustive=exhaustive, tail=tail, num_subjects=S)


class GroupPermutation:
    """What MapStatistics.group_permutation found.  t (V,): group_t of the map; scale (V,): 1 / sqrt(S sum_s m^2) as handed to the kernel,
    0 at a voxel that took no part; stat (V,): the statistic compared, g(u) with g = |.|
    ('two'), as it is ('pos') or negated ('neg'); max_stat (n_perm,): its maximum over the voxels under each sign pattern; signs
    (n_perm,) int64: the patterns as bit sets (bit s flips subject s; word 0 is the identity); p_unc, p_fwe (V,): uncorrected and
    family-wise-error corrected p, both in [1 / n_perm, 1]; n_perm: patterns actually used (2^S when exhaustive)."""

    def __init__(self, **fields):
        self.__dict__.update(fields)

    def threshold(self, alpha=0.05):
        """The critical value at family-wise level alpha on the scale of t: the ceil((1 - alpha) n_perm)-th smallest max_stat mapped
        through u -> t = u sqrt((S-1) / (1-u^2)).  'two': |t| has to exceed it; 'pos': t; 'neg': the value is negative and t has to lie
        below it.  A critical u of 1 (some pattern makes every subject agree exactly at a voxel) maps to inf."""
        import math
        P, S = self.n_perm, self.num_subjects
        k = min(P, max(1, int(math.ceil((1.0 - float(alpha)) * P))))
        u = float(self.max_stat.sort().values[k - 1])
        t = math.copysign(math.inf, u) if abs(u) >= 1.0 else u * math.sqrt((S - 1) / (1.0 - u * u))
        return -t if self.tail == 'neg' else t
