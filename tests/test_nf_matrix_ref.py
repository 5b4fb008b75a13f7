"""The references of the NF class tests, checked without a GPU: the long-double draw against the
oracle's Cholesky draw at the corner shapes, the numpy hyper-MH block (tests/hyper_ref.py) against the
reference's own captured run, and the committed hyper-MH cases free of undecidable steps."""
import numpy as np
import pytest

from oracle import gibbs_oracle as O
from tests import hyper_ref as H
from tests import nf_cases as K
from tests.conftest import golden
from tests.parity_data import exact_chol_draw_pre, normwise_rel


@pytest.mark.parametrize("NF,nm", K.CORNERS)
def test_exact_draw_agrees_with_oracle_chol_at_corners(NF, nm):
    """exact_chol_draw_pre (x87 long double) == oracle.bdraw_chol (fp64) to 1e-9 normwise at the
    smallest and largest NF with no and with 64 fixed columns and at the CP = 0, nm = 17 edge: the
    long-double reference of the device tests is the oracle's draw at these sizes too."""
    T, N, r = K.pulsar(NF, nm)
    m = T.shape[1]
    assert m == NF + nm
    TNT, d = K.tnt64(NF, nm)
    tl, order = K.exact(NF, nm)
    rng = np.random.default_rng(NF + 100 * nm)
    ph = K.phiinv_rows(rng, 4, NF)
    z = rng.standard_normal((4, m))
    for c in range(4):
        phi = np.concatenate([ph[c], np.full(nm, 1e-40)])
        want = O.bdraw_chol(TNT, d, phi, z[c], order)
        got = exact_chol_draw_pre(tl, phi, z[c], order)
        assert normwise_rel(got, want) < 1e-9, (NF, nm, c, normwise_rel(got, want))


def test_hyper_ref_reproduces_reference_run():
    """HyperRef fed the captured draws of the reference's PTABlockGibbs(redsample='mh') run (45
    pulsars, power-law red noise) from the reference's x at each block's start ends on the reference's
    x exactly, block by block, walking the draw log as tests/test_gpu_pta_mh.py does."""
    from pulsar_timing_gibbsspec_amd import synthetic
    from tests.test_gpu_pta_mh import DrawLog
    g = golden("pta_plred_mh.npz")
    pta = synthetic.array_pta(kind="curn_plred", seed=0)
    ref = H.HyperRef(pta, hind=g["hind"])
    assert np.array_equal(ref.hind, H.hyper_indices(pta.param_names))
    log = DrawLog(g)
    P = int(g["n_psr"])
    n_acc = n_steps = 0
    for ii in range(g["chain"].shape[0]):
        if ii == 0:
            for _ in range(P):
                log.take("randn")
        n = int(g["warm"]) if ii == 0 else int(g["aclength"])
        got, acc, _ = ref.block(g["hyper_in"][ii], log.mh(n))
        assert np.array_equal(got, g["hyper_out"][ii]), (ii, np.nonzero(got != g["hyper_out"][ii]))
        n_acc += acc
        n_steps += n
        log.take("uniform")
        if log.peek() == "randn":
            for _ in range(P):
                log.take("randn")
    assert log.k == len(log.kinds)
    assert 0 < n_acc < n_steps


@pytest.mark.parametrize("n_f,seed", H.MH_CASES)
def test_committed_hyper_cases_have_no_near_tie(n_f, seed):
    """No step of a committed case has |diff - log u| below 1e-9 |lnL_p|, so an fp64 kernel decides
    every one as the reference does; every chain sees both outcomes."""
    _, x0, rows, x_out, n_acc, n_tie = H.mh_case(n_f, seed)
    assert rows.shape == (H.MH_STEPS, H.MH_CHAINS, 4) and H.MH_STEPS > 64
    assert not n_tie.any(), n_tie
    assert np.all((0 < n_acc) & (n_acc < H.MH_STEPS)), n_acc
    assert not np.array_equal(x_out, x0)
