"""The long-double ECORR references (tests/ecorr_ref.py) on the CPU: against the float64 oracle within the
tolerances tests/test_gpu_ecorr_shapes.py applies to the device (so the reference alone sits inside
them), the three routes to the likelihood inside the reference against each other, and the Metropolis
cases' decision margins above the floor below which the device's 1e-9 likelihood could flip a decision."""
import numpy as np
import pytest

from oracle import gibbs_oracle as O
from tests import ecorr_ref as E
from tests.parity_data import normwise_rel

L_ = np.longdouble
MODELS = E.FUSED + E.UNFUSED
N_X = 3   # chains' states per case


def _f64(a):
    return np.asarray(a, dtype=np.float64)


@pytest.mark.parametrize("name", MODELS)
def test_lnlike_ref_matches_oracle(name):
    """lnlike_ref against oracle.lnlike_fullmarg and lnlike_ecorr_marg, 1e-7 max(1, |ref|); its second
    value is the first without the white-noise and the timing-model prior constants."""
    c = E.case(name)
    TNT, d = E.tnt64(name)
    for x in E.draws(c, N_X):
        phiinv, ld = E.phiinv_full(c, x)
        full, red = E.lnlike_ref(c["T"], c["N"], c["r"], phiinv, ld, fixed=c["fixed"])
        for ref in (O.lnlike_fullmarg(c["r"], c["N"], TNT, d, phiinv, ld),
                    O.lnlike_ecorr_marg(c["r"], c["N"], TNT, d, c["ecid"], phiinv, ld)):
            assert abs(float(full) - ref) < 1e-7 * max(1.0, abs(ref)), (name, float(full), ref)
        const = E.white_const(c["N"], c["r"]) + c["nm"] * np.log(L_(1e-40)) / 2
        assert abs(red + const - full) < 1e-15 * abs(full)
    if c["pta"] is not None:   # phiinv_full is the model's own get_phiinv
        x = E.draws(c, 1)[0]
        want, wld = c["pta"].get_phiinv(c["pta"].map_params(x), logdet=True)[0]
        got, gld = E.phiinv_full(c, x)
        assert np.array_equal(got, want) and abs(gld - wld) < 1e-12 * abs(wld)


@pytest.mark.parametrize("name", MODELS)
def test_reference_routes_agree(name):
    """Dense from (T, N, r); the epochs eliminated first; and (fused cases) the reordered [M | F | d]
    operands through prefix_ref -- all in long double from the long-double TNT: 1e-15 relative."""
    c = E.case(name)
    op = E.host_operands(name, exact=True)
    for x in E.draws(c, N_X):
        # phi_E as prefix_ref forms it from x (long-double pow), so that the routes see one model
        phiinv = np.asarray(E.phiinv_full(c, x)[0], dtype=L_)
        phiinv[c["ecid"]] = 1 / E._phi_E(x, c["eind"], c["ebk"])
        ld = -np.sum(np.log(phiinv))
        full, red = E.lnlike_ref(c["T"], c["N"], c["r"], phiinv, ld, fixed=c["fixed"])
        elim = E.lnlike_ecorr_ref(c["T"], c["N"], c["r"], c["ecid"], phiinv, ld)
        print(name, "dense vs eliminated", float(abs(elim - full) / abs(full)))
        assert abs(elim - full) < 1e-15 * abs(full)
        if "Bp" in op:
            p = E.prefix_ref(op["Bp"], op["Dg"], c["ebk"], op["Ap"], x, c["eind"], E.phiinv_F(c, x)[0], c["NF"],
                             c["nm"], c["nm"])
            a = p["aux_lnl"]
            got = p["lnl"] + (a[1] - a[0] - a[2]) / 2
            print(name, "dense vs reordered", float(abs(got - red) / abs(full)))
            assert abs(got - red) < 1e-15 * abs(full)
            # the block mode's factors give the same value: log det Sigma = 2 am0 + log det(S0 + D_F), d^T
            # Sigma^-1 d = P_dd + am1 + dF^T (S0 + D_F)^-1 dF
            phF = np.asarray(E.phiinv_F(c, x)[0], dtype=L_)
            LS = E.chol(p["S0"][:, :c["NF"]] + np.diag(phF))
            y = E.solve_lower(LS, p["dF"])
            blk = (p["aux_block"][1] + p["am"][1] + y @ y - 2 * p["am"][0] - 2 * np.sum(np.log(np.diag(LS)))
                   + np.sum(np.log(phF)) - p["aux_block"][0] - p["aux_block"][2]) / 2
            assert abs(blk - red) < 1e-12 * abs(full)


@pytest.mark.parametrize("name", E.FUSED)
def test_prefix_ref_matches_oracle(name):
    """prefix_ref on the float64 operands: the likelihood against oracle.lnlike_ecorr_marg (1e-9 max(1,
    |ref|), the device's tolerance on lnl) and every section of the model block against oracle.ecorr_schur
    + prefix_factor (1e-9 normwise); NMX > nM only strides the fixed-block sections."""
    c = E.case(name)
    op = E.host_operands(name)
    TNT, d = E.tnt64(name)
    NF, nm = c["NF"], c["nm"]
    const = float(E.white_const(c["N"], c["r"])) + 0.5 * nm * np.log(1e-40)
    for x in E.draws(c, N_X):
        phiinv, ld = E.phiinv_full(c, x)
        p = E.prefix_ref(op["Bp"], op["Dg"], c["ebk"], op["Ap"], x, c["eind"], E.phiinv_F(c, x)[0], NF, nm, nm)
        a = p["aux_lnl"]
        got = float(p["lnl"] + (a[1] - a[0] - a[2]) / 2) + const
        fast = E._prefix_lnl(op, c["ebk"], x, c["eind"], E.phiinv_F(c, x)[0], NF)   # mh_case's likelihood
        assert abs(fast - (p["lnl"] + (a[1] - a[0] - a[2]) / 2)) < 1e-17 * abs(got)
        ref = O.lnlike_ecorr_marg(c["r"], c["N"], TNT, d, c["ecid"], phiinv, ld)
        assert abs(got - ref) < 1e-9 * max(1.0, abs(ref)), (name, got, ref)
        rc, S, dR, sla, sdw = O.ecorr_schur(TNT, d, c["ecid"], 1.0 / phiinv[c["ecid"]])
        pos = {col: i for i, col in enumerate(rc)}
        pf = O.prefix_factor(S, dR, np.array([pos[g] for g in c["gwid"]]), np.full(nm, 1e-40))
        np.testing.assert_allclose(_f64(p["aux_block"]), [sla, sdw, -np.sum(np.log(phiinv[c["ecid"]])), 0.0],
                                   rtol=1e-11)
        assert normwise_rel(_f64(p["S0"][:, :NF]), pf["S0"]) < 1e-9
        assert normwise_rel(_f64(p["dF"]), pf["dF"]) < 1e-9 and np.array_equal(p["S0"][:, NF], p["dF"])
        assert normwise_rel(_f64(p["Gm"][:, :NF]), pf["G"]) < 1e-9 and not p["Gm"][:, NF].any()
        assert normwise_rel(_f64(p["hm"]), pf["h"]) < 1e-9
        assert normwise_rel(_f64(p["Rm"]).ravel(), pf["R"].ravel()) < 1e-9
        assert p["block"].size == sum(E.section_sizes(NF, nm))
        wide = E.prefix_ref(op["Bp"], op["Dg"], c["ebk"], op["Ap"], x, c["eind"], E.phiinv_F(c, x)[0], NF, nm,
                            nm + 3)
        assert np.array_equal(wide["Rm"][:nm, :nm], p["Rm"]) and not wide["Rm"][nm:].any()
        assert np.array_equal(wide["Gm"][:nm], p["Gm"]) and not wide["Gm"][nm:].any()
        assert wide["block"].size == sum(E.section_sizes(NF, nm + 3))


@pytest.mark.parametrize("name", MODELS)
def test_schur_and_bdraw_ref_match_oracle(name):
    """schur_ref against oracle.ecorr_schur (the direct Schur test's 1e-12 entrywise) and bdraw_ref's mean
    against oracle.bdraw_ecorr at zero normals (1e-8 normwise, the device's tolerance)."""
    c = E.case(name)
    op = E.host_operands(name)
    TNT, d = E.tnt64(name)
    x = E.draws(c, 1)[0]
    phiinv, _ = E.phiinv_full(c, x)
    S, dv, aux = E.schur_ref(op["Bx"], op["Dg"], c["ebk"], x, c["eind"], op["A"], op["dR"], op["mR"])
    rc, So, dRo, sla, sdw = O.ecorr_schur(TNT, d, c["ecid"], 1.0 / phiinv[c["ecid"]])
    assert np.max(np.abs(_f64(S) - So)) <= 1e-12 * np.max(np.abs(So))
    assert normwise_rel(_f64(dv), dRo) < 1e-12
    np.testing.assert_allclose(_f64(aux[:2]), [sla, sdw], rtol=1e-12)
    mean, Sig = E.bdraw_ref(c["T"], c["N"], c["r"], phiinv)
    ref = O.bdraw_ecorr(TNT, d, c["ecid"], phiinv, np.zeros(rc.size), np.zeros(c["ne"]))
    assert normwise_rel(ref, _f64(mean)) < 1e-8
    assert np.max(np.abs(_f64(Sig) - (TNT + np.diag(phiinv)))) <= 1e-12 * np.max(np.abs(TNT))


@pytest.mark.parametrize("name", E.MH_CASES)
def test_mh_ref_margins_above_floor(name):
    """No injected step of the Metropolis cases is a near-tie: the smallest |delta - log u| over all
    chains and steps exceeds 4e-9 max |lnL|, and every chain accepts at least once -- so the GPU test
    compares every step's decision."""
    c = E.case(name)
    X0, inj, Xo, acc, marg, lmax = E.mh_case(name)
    print(name, "min margin", marg.min(), "max |lnL|", lmax, "accepted", int(acc.sum()), "of", marg.size)
    assert marg.shape == (E.MH_CHAINS, E.MH_STEPS)
    assert marg.min() > E.MH_MARGIN_REL * lmax, (marg.min(), lmax)
    assert acc.min() >= 1
    assert np.all((Xo[:, c["eind"]] >= c["emin"]) & (Xo[:, c["eind"]] <= c["emax"]))
    other = np.setdiff1d(np.arange(c["n_param"]), c["eind"])
    assert np.array_equal(Xo[:, other], X0[:, other])
    if name == "EMPTY":
        k = np.searchsorted(c["ebk"], [1, 2])
        assert k[0] == k[1]           # backend 1 owns no epoch


def test_mh_ref_is_white_mh_with_a_box_prior():
    """mh_ref against oracle.white_mh (the same block with an explicit prior) on a cheap likelihood."""
    rng = np.random.default_rng(3)
    ecol, lo, hi = np.array([0, 2]), np.array([-1.0, -1.0]), np.array([1.0, 1.0])
    steps = np.stack([rng.choice(O.MH_SIZES, 60, p=O.MH_PROBS), rng.integers(0, 2, 60), rng.standard_normal(60),
                      rng.uniform(0, 1, 60)], axis=1)
    lnl = lambda x: -4.0 * float(np.sum(np.asarray(x, float)[ecol] ** 2))                     # noqa: E731
    lnp = lambda x: 0.0 if np.all((x[ecol] >= lo) & (x[ecol] <= hi)) else -np.inf              # noqa: E731
    x0 = np.array([0.2, 7.0, -0.3])
    got, n_acc, marg, lmax = E.mh_ref(lnl, x0, ecol, lo, hi, steps)
    want = O.white_mh(x0, ecol, [(s, ecol[int(p)], z, u) for s, p, z, u in steps], lnl, lnp)
    assert np.array_equal(got, want) and 0 < n_acc < 60 and marg.shape == (60,)
