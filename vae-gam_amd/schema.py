"""Covariate schema and network geometry of the VAE-GAM (host-side description only).

The reference hard-codes eight covariates, six inducing points and one image shape
(vae_reg_GP.py:32,68,308,352,377).  This module states the same rules as data so
that the 3-, 8- and 12-covariate configurations and the 82x98x70 geometry share one code path,
and reduces exactly to the reference for num_covariates <= 8 at 41x49x35.  Any other volume grid gets a
network derived from its shape (`net_geometry`: the family rule, and embedding for grids outside the family).
"""
from dataclasses import dataclass
from typing import List, Sequence, Tuple

import numpy as np

from .ops import ConvSpec

REF_NAMES = ['task', 'x', 'y', 'z', 'xrot', 'yrot', 'zrot', 'sex']                      # vae_reg_GP.py:68
REF_IMG_KEYS = ['base', 'task', 'x_mot', 'y_mot', 'z_mot', 'pitch_mot', 'roll_mot', 'yaw_mot', 'sex',
                'full_rec']                                                              # vae_reg_GP.py:308-309
REF_CSV_COLS = ['x', 'y', 'z', 'rot_x', 'rot_y', 'rot_z']                                # utils.py:50


@dataclass(frozen=True)
class Covariate:
    name: str
    gp: bool       # continuous: linear gain + sparse-GP gain (vae_reg_GP.py:352)
    hrf: bool      # gain convolved with the HRF along the batch axis (vae_reg_GP.py:377)
    img_key: str   # key in the dict returned with return_latent_rec=True


def covariate_schema(num_covariates: int, neural_covariates: bool = True) -> List[Covariate]:
    """Roles the reference assigns by position: GP iff 1 < i < 8, HRF iff neural and i < C-6.
    Beyond eight covariates (no reference counterpart) extra continuous covariates c1.. follow
    `task`, every covariate but the first and last gets a GP term, the HRF rule stays positional."""
    C = int(num_covariates)
    if C < 1:
        raise ValueError('num_covariates must be >= 1')
    if C <= 8:
        names, keys = REF_NAMES[:C], REF_IMG_KEYS[1:C + 1]
        gp = [1 < i < 8 for i in range(1, C + 1)]
    else:
        extra = ['c%d' % k for k in range(1, C - 8 + 1)]
        names = ['task'] + extra + REF_NAMES[1:]
        keys = ['task'] + extra + REF_IMG_KEYS[2:9]
        gp = [1 < i < C for i in range(1, C + 1)]
    hrf = [bool(neural_covariates) and i < (C - 6) for i in range(1, C + 1)]
    return [Covariate(n, g, h, k) for n, g, h, k in zip(names, gp, hrf, keys)]


def parameter_sets(num_covariates: int, neural_covariates: bool = True) -> List[Covariate]:
    """Gain-parameter sets that are INSTANTIATED: the reference always creates all eight
    (vae_reg_GP.py:68-172) even when fewer covariates are used."""
    return covariate_schema(max(8, num_covariates), neural_covariates)


@dataclass(frozen=True)
class NetGeometry:
    img: Tuple[int, int, int]
    nf: int
    enc: Tuple[ConvSpec, ...]          # conv1..conv5
    dec: Tuple[ConvSpec, ...]          # convt1..convt5
    dec_seed: Tuple[int, int, int]     # spatial size fc8's output is viewed as
    native: Tuple[int, int, int] = None   # the data's own grid; img = native + pad is the grid the layers run on
    pad: Tuple[int, int, int] = (0, 0, 0)  # zero voxels appended at the high end of each axis (embedding)

    def __post_init__(self):
        if self.native is None:
            object.__setattr__(self, 'native', self.img)

    def enc_sizes(self):
        s = [self.img]
        for sp in self.enc:
            s.append(sp.out_size(s[-1]))
        return s

    def dec_sizes(self):
        s = [self.dec_seed]
        for sp in self.dec:
            s.append(sp.out_size(s[-1]))
        return s

    @property
    def enc_flat(self):
        return 2 * self.nf * int(np.prod(self.enc_sizes()[-1]))

    @property
    def dec_flat(self):
        return 2 * self.nf * int(np.prod(self.dec_seed))


MIN_NATIVE_AXIS = 19       # an axis is padded by at most 3 voxels: the smallest family member is 22
MAX_LAST_AXIS = 130        # the weight-gradient kernel walks rows of at most 128 positions (the first layer's output row: last axis - 2)


def in_family(img: Sequence[int]) -> bool:
    """Grids the family rule covers: every axis = 2 (mod 4) and >= 22."""
    return all(int(n) % 4 == 2 and int(n) >= 22 for n in img)


def grid_for(native: Sequence[int]) -> Tuple[int, int, int]:
    """Per axis the smallest family member >= the native size (0..3 voxels more)."""
    native = tuple(int(v) for v in native)
    if len(native) != 3 or min(native) < MIN_NATIVE_AXIS:
        raise ValueError('image shape %r: every axis must have at least %d voxels (an axis is embedded into the next size = 2 (mod 4) '
                         'from 22 on, by at most 3 voxels of zero padding)' % (native, MIN_NATIVE_AXIS))
    return tuple(max(22, n + (2 - n) % 4) for n in native)


def family_decoder(grid: Sequence[int], enc, nf: int = 8):
    """(decoder layers, seed) the family rule gives a grid with in_family(grid): the mirror of the encoder `enc`."""
    assert in_family(grid), grid
    k3 = (3, 3, 3)
    dec = (ConvSpec('convt', 2 * nf, 2 * nf, k3, 1), ConvSpec('convt', 2 * nf, 2 * nf, k3, 2),
           ConvSpec('convt', 2 * nf, nf, k3, 1), ConvSpec('convt', nf, nf, (4, 4, 4), 2),
           ConvSpec('convt', nf, 1, k3, 1))
    seed = tuple(int(v) for v in grid)
    for sp in enc:
        seed = sp.out_size(seed)
    return dec, seed


def net_geometry(img: Sequence[int], nf: int = 8) -> NetGeometry:
    """The network of a volume grid.  41x49x35 (the reference's), 82x98x70 and the 21^3 test toy have explicit entries.
    Family rule: on a grid whose axes are all = 2 (mod 4) and >= 22 the encoder sizes are exact (n-2, (n-2)/2-1, -2, (.-1)/2, -2:
    no floor ever drops a voxel) and the decoder is their mirror: seed = the last encoder size, convt1 3^3 s1, convt2 3^3 s2 without
    padding, convt3 3^3 s1, convt4 4^3 s2, convt5 3^3 s1 -- the layer kinds of the 82x98x70 network, which is the rule's output.
    Any other grid with axes >= 19 is EMBEDDED: the layers run on grid_for(img), the volumes are zero-padded at the high end of each
    axis (NetGeometry.pad), and everything that is scored or exported stays on the native grid (NetGeometry.native)."""
    img = tuple(int(v) for v in img)
    k3 = (3, 3, 3)
    enc = (ConvSpec('conv', 1, nf, k3, 1), ConvSpec('conv', nf, nf, k3, 2), ConvSpec('conv', nf, 2 * nf, k3, 1),
           ConvSpec('conv', 2 * nf, 2 * nf, k3, 2), ConvSpec('conv', 2 * nf, 2 * nf, k3, 1))      # :189-193
    native = img
    if img == (41, 49, 35):
        dec = (ConvSpec('convt', 2 * nf, 2 * nf, k3, 1),
               ConvSpec('convt', 2 * nf, 2 * nf, k3, 2, (1, 0, 1), (1, 0, 1)),
               ConvSpec('convt', 2 * nf, nf, k3, 1),
               ConvSpec('convt', nf, nf, (5, 3, 3), 2),
               ConvSpec('convt', nf, 1, k3, 1))                                                   # :211-215
        seed = (6, 8, 5)                                                                          # :259
    elif img == (82, 98, 70):
        # 16x20x13 -> 18x22x15 -> 37x45x31 -> 39x47x33 -> (k4,s2) 80x96x68 -> 82x98x70
        dec = (ConvSpec('convt', 2 * nf, 2 * nf, k3, 1), ConvSpec('convt', 2 * nf, 2 * nf, k3, 2),
               ConvSpec('convt', 2 * nf, nf, k3, 1), ConvSpec('convt', nf, nf, (4, 4, 4), 2),
               ConvSpec('convt', nf, 1, k3, 1))
        seed = (16, 20, 13)
    elif img == (21, 21, 21):
        # smallest volume the encoder admits; used by the CPU tests (host build of the kernels) only
        dec = (ConvSpec('convt', 2 * nf, 2 * nf, k3, 1), ConvSpec('convt', 2 * nf, 2 * nf, k3, 2),
               ConvSpec('convt', 2 * nf, nf, k3, 1), ConvSpec('convt', nf, nf, k3, 2), ConvSpec('convt', nf, 1, k3, 1))
        seed = (1, 1, 1)
    else:
        if len(img) != 3:
            raise ValueError('no network geometry defined for image shape %r' % (img,))
        img = native if in_family(native) else grid_for(native)
        if img[2] > MAX_LAST_AXIS:
            raise ValueError('image shape %r (network grid %r): the last axis of the grid must be <= %d' % (native, img, MAX_LAST_AXIS))
        dec, seed = family_decoder(img, enc, nf)
    from dataclasses import replace
    enc = tuple(replace(sp, name='conv%d' % (i + 1)) for i, sp in enumerate(enc))
    dec = tuple(replace(sp, name='convt%d' % (i + 1)) for i, sp in enumerate(dec))
    g = NetGeometry(img, nf, enc, dec, seed, native, tuple(a - b for a, b in zip(img, native)))
    assert g.dec_sizes()[-1] == img, (g.dec_sizes(), img)
    return g
