"""CPU self-tests of tests/white_ref.py, the long-double references of the white-noise kernel
tests (tests/test_gpu_white_shapes.py).

* white_mh_ref reproduces the reference's own first Metropolis block (white_mh_j1713.npz) and
  oracle.white_mh on it; exact_white_tnt / exact_N agree with the fp64 oracle within the bounds
  the GPU tests use.
* white_mh_philox (whole likelihood per step) and white_mh_ref (touched backend only) agree on
  the Philox-generated steps.
* No committed seed or shape of the GPU tests has an accept/reject near-tie (margin <= B): the
  GPU tests may skip a system only on a near-tie, and their cap is zero skipped systems.  If a
  new seed produces one, change the seed; the cap stays.
"""
import numpy as np
import pytest

from oracle import gibbs_oracle as O
from tests import white_ref as W
from tests.conftest import golden
from tests.parity_data import white_params


@pytest.fixture(scope="module")
def j1713():
    from tests.parity_data import white_replay
    g = golden("white_mh_j1713.npz")
    return g, white_replay(g)


def test_white_mh_ref_reproduces_reference_block(j1713):
    g, rp = j1713
    wl = white_params(g)
    wind = [int(j) for j in g["wind"]]
    bk = np.asarray(g["backends"])
    perm = np.argsort(bk, kind="stable")
    bk_off = np.concatenate([[0], np.cumsum(np.bincount(bk))])
    y = (g["r"] - g["T"] @ rp["b_first"])[perm]
    steps = rp["mh"][0]
    x, n_acc, q_rec, margin, B = W.white_mh_ref(g["x0"], wl, g["sigma"][perm] ** 2, bk_off, y, steps, len(steps))
    assert np.array_equal(x[wind], g["white_out"][0][wind])
    names = list(g["param_names"])
    ef_i = [names.index(f"J1713+0747_b{i}_efac") for i in range(3)]
    eq_i = [names.index(f"J1713+0747_b{i}_log10_tnequad") for i in range(3)]
    xo = O.white_mh(g["x0"], wind, [(s[0], wind[int(s[1])], s[2], s[3]) for s in steps],
                    lambda q: O.lnlike_white(g["r"], g["T"], rp["b_first"],
                                             O.ndiag_white(g["sigma"], g["backends"], q[ef_i], q[eq_i])),
                    lambda q: 0.0 if np.all((q >= g["pmin"]) & (q <= g["pmax"])) else -np.inf)
    assert np.array_equal(x, xo)
    assert 0 < n_acc < len(steps) and q_rec.shape == (len(steps), len(wl))
    assert np.all(margin > B)
    # a shorter block stops early
    x7 = W.white_mh_ref(g["x0"], wl, g["sigma"][perm] ** 2, bk_off, y, steps, 7)
    assert x7[2].shape[0] == 7 and np.array_equal(x7[2], q_rec[:7])
    assert np.array_equal(W.white_mh_ref(g["x0"], wl, g["sigma"][perm] ** 2, bk_off, y, steps, 0)[0], g["x0"])


def test_exact_tnt_agrees_with_oracle(j1713):
    g, _ = j1713
    wl = white_params(g)
    N = W.exact_N(g["sigma"] ** 2, g["backends"], W.params_of(wl, g["x0"]))
    ef = g["x0"][[c for c, kind, *_ in wl if kind == W.EFAC]]
    eq = g["x0"][[c for c, kind, *_ in wl if kind == W.TNEQUAD]]
    N64 = O.ndiag_white(g["sigma"], g["backends"], ef, eq)
    assert np.max(np.abs(N64 - N) / N) <= 4 * W.U
    TNT, d = O.tnt(g["T"], N64, g["r"])
    W.check_tnt(TNT, d, g["T"], N, g["r"], symmetric=False)    # numpy's dgemm is not a SYRK
    # absent parameters: efac 1, equad 0
    s2 = np.array([1e-14, 4e-14])
    assert np.array_equal(W.exact_N(s2, [0, 1], []), s2.astype(W.L))
    n = W.exact_N(s2, [0, 1], [(W.T2EQUAD, 1, -7.0), (W.EFAC, 1, 2.0), (W.TNEQUAD, 0, -7.0)])
    assert np.allclose(np.asarray(n, float), [1e-14 + 1e-14, 4 * (4e-14 + 1e-14)], rtol=1e-15)


def test_check_tnt_catches_a_wrong_small_tile():
    """The entrywise bound sees what max|dTNT| <= 1e-12 max|TNT| cannot: a zeroed 16 x 16 tile in
    the small-magnitude block, a one-sided entry, a 1e-13 relative error."""
    psr, vals = W.syrk_case(70, 47)
    d = psr[0]
    N = W.exact_N(d["sigma"] ** 2, d["backends"], W.params_of(W.SYRK_WHITE[0], W.layout_x(
        vals, W.SYRK_WHITE, W.SYRK_C, W.SYRK_LDX, False)[0]))
    TNT, dd, _ = W.exact_white_tnt(d["T"], N, d["r"])
    TNT, dd = np.asarray(TNT, float), np.asarray(dd, float)
    TNT = np.tril(TNT) + np.tril(TNT, -1).T
    W.check_tnt(TNT, dd, d["T"], N, d["r"])
    small = np.argsort(np.diag(TNT))[:16]
    for kind in ("tile", "asym", "rel", "d"):
        A, v = TNT.copy(), dd.copy()
        if kind == "tile":
            A[np.ix_(small, small)] = 0.0
            assert np.max(np.abs(A - TNT)) <= 1e-12 * np.max(np.abs(TNT))   # the old assertion passes
        elif kind == "asym":
            A[5, 3] = np.nextafter(A[5, 3], np.inf)
        elif kind == "rel":
            A[7, 2] *= 1 + 1e-13
            A[2, 7] = A[7, 2]
        else:
            v[small[0]] *= 1 + 1e-12
        with pytest.raises(AssertionError):
            W.check_tnt(A, v, d["T"], N, d["r"])


@pytest.mark.parametrize("per_sys", [False, True])
def test_philox_block_equals_ref_on_its_own_steps(per_sys):
    _, refs = W.mh_philox_refs(per_sys)
    assert len(refs) == 3 * W.MH_C
    for (p, c), (ph, ref) in refs.items():
        assert np.array_equal(ph[0], ref[0]), (p, c)
        assert ph[1] == ref[1], (p, c)
        assert ph[2].shape == (W.MH_STEPS, 4) and np.all((ph[3] >= 0) & (ph[3] < len(W.MH_WHITE[p])))


def test_philox_steps_are_the_device_stream():
    """Counter words: slot 3 s + j, sweep, global chain, (global pulsar << 8) | GS_EV_WHITE."""
    key = np.array([3, 4], np.uint32)
    st = W.philox_steps(5, 2, key, 9, 21, 6)
    u1, u2 = O.philox_uniform_pair(np.array([3, 9, 21, (6 << 8) | 7], np.uint32), key)
    v1, v2 = O.philox_uniform_pair(np.array([4, 9, 21, (6 << 8) | 7], np.uint32), key)
    u, _ = O.philox_uniform_pair(np.array([5, 9, 21, (6 << 8) | 7], np.uint32), key)
    assert st[1, 0] == W.mh_scale(float(u1)) and st[1, 1] == min(int(float(u2) * 5), 4)
    assert st[1, 2] == O.box_muller(v1, v2)[0] and st[1, 3] == float(u)
    assert [W.mh_scale(v) for v in (0.0, 0.0999, 0.1, 0.2499, 0.25, 0.7499, 0.75, 0.8999, 0.9, 0.9999)] == \
        [0.1, 0.1, 0.5, 0.5, 1.0, 1.0, 3.0, 3.0, 10.0, 10.0]


def _no_near_tie(refs):
    for sys, r in enumerate(refs):
        margin, B = r[3], r[4]
        assert np.all(margin > B), (sys, np.nonzero(margin <= B)[0], margin.min())


@pytest.mark.parametrize("per_sys", [False, True])
def test_committed_seeds_have_no_near_tie(per_sys):
    """Every Metropolis case of the GPU tests: zero near-tie steps, so zero skipped systems."""
    _, refs = W.mh_refs(per_sys)
    _no_near_tie(refs)
    for p in range(3):   # the block both accepts and rejects, inside and outside the prior
        acc = sum(r[1] for r in refs[p * W.MH_C:(p + 1) * W.MH_C])
        out = sum(int(np.isinf(r[3]).sum()) for r in refs[p * W.MH_C:(p + 1) * W.MH_C])
        assert 0.05 * W.MH_C * W.MH_STEPS < acc < 0.95 * W.MH_C * W.MH_STEPS, (p, acc)
        assert p == 0 or out > 0, p
    ns = W.mh_nsteps(per_sys)
    assert ns.min() == 0 and ns.max() == W.MH_STEPS
    _no_near_tie(W.mh_refs(per_sys, nsteps=ns)[1])
    inj, wmax = W.mh_edge_case()
    _, edge = W.mh_refs(per_sys, inj=inj, wmax=wmax)
    _no_near_tie(edge)
    a, b = edge[0 * W.MH_C + 2], edge[2 * W.MH_C + 4]
    assert a[1] == 1 and a[2][0, 0] == wmax[(0, 0)] and np.isfinite(a[3][0])     # on the edge: evaluated, accepted
    assert b[1] == 0 and b[2][0, 0] == np.nextafter(wmax[(2, 0)], np.inf) and np.isinf(b[3][0])
    _no_near_tie([r[1] for r in W.mh_philox_refs(per_sys)[1].values()])


def test_case_builders_reach_the_intended_paths():
    assert sorted({(m + 16) // 16 for nb in range(1, 17) for m in W.syrk_ms(nb)}) == list(range(1, 17))
    assert all((m + 16) // 16 == nb for nb in range(1, 17) for m in W.syrk_ms(nb))
    assert [len(w) for w in W.MH_WHITE] == [1, 32, 4] and len(W.MH_BK15) == 15
    cols = [c for w in W.MH_WHITE for c, *_ in w]
    assert len(set(cols)) == len(cols) and max(cols) < W.MH_LDX
    for first_big in (True, False):
        e = W.epoch_case(48, 1, 40, first_big)
        tot = [int(np.sum(e["sizes"][i:i + 16])) for i in range(0, 40, 16)]
        assert [t > 256 for t in tot] == [first_big, not first_big, first_big]
    assert W.epoch_case(48, 1, 1, True)["sizes"][0] > 256
