"""Shapes and shared references of the NF class x fixed-block layout tests
(tests/test_gpu_nf_matrix.py, tests/test_gpu_bdraw_persist.py, tests/test_nf_matrix_ref.py).

``dispatch_nf`` (csrc/gibbs_bdraw.h) stamps every b-draw, sweep, likelihood and hyper-MH kernel
out in eight NF classes -- the fixed NFC = 20 / 40 / 60 and, with NF at run time, NTC = NF/16 + 1 =
1..5 tile rows -- and the fixed-prior block is read in tiles (NMX <= 16), row-major (17..64) or by
the wide kernel (> 64).  NF_LIST has every class at its smallest, an interior and its largest NF,
the last-tile edges CP = NF mod 16 = 0 (16, 32, 48, 64) included.

The pulsars are synthetic.single_pulsar_pta(n_f, tm_cols=nm) as tests/test_gpu_nf.py builds them;
each one and its long-double (TNT, d) is computed once per session and never modified."""
from functools import lru_cache

import numpy as np

from oracle import gibbs_oracle as O
from tests.parity_data import exact_tnt

#           NTC=1  NTC=1 NTC=2 NFC=20 NTC=2 NTC=3 NFC=40 NTC=3 NTC=4 NFC=60 NTC=4 NTC=5
NF_LIST = (2, 14, 16, 20, 30, 32, 40, 46, 48, 60, 62, 64)
CORNERS = ((2, 0), (2, 64), (16, 17), (64, 64))


def nf_class(NF):
    """The dispatch_nf class of NF as the kernels' template arguments (NFC, NTC)."""
    return (NF, 0) if NF in (20, 40, 60) else (0, NF // 16 + 1)


@lru_cache(maxsize=None)
def pulsar(NF, nm):
    """(T, N, r) of the J1713 pulsar with NF / 2 free-spectrum bins and nm timing-model columns."""
    from pulsar_timing_gibbsspec_amd import synthetic
    pta = synthetic.single_pulsar_pta("J1713+0747", n_f=NF // 2, tm_cols=nm, seed=2)
    out = pta.get_basis()[0], pta.get_ndiag({})[0], pta.get_residuals()[0]
    for a in out:
        a.setflags(write=False)
    return out


@lru_cache(maxsize=None)
def exact(NF, nm):
    """(long-double (TNT, d), Cholesky column order) of pulsar(NF, nm)."""
    T, N, r = pulsar(NF, nm)
    return exact_tnt(T, N, r), O.chol_order(T.shape[1], np.arange(NF))


@lru_cache(maxsize=None)
def tnt64(NF, nm):
    return O.tnt(*pulsar(NF, nm))


def phiinv_rows(rng, C, NF):
    """C rows of phiinv_F = 1 / repeat(rho, 2) with log10 rho uniform in (-8.5, -5)."""
    logrho = rng.uniform(-8.5, -5.0, (C, NF // 2))
    return 1.0 / np.repeat(10 ** (2 * logrho), 2, axis=1)
