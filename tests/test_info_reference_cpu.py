"""The oracle's information estimators (oracle/info.c: the literal restatement of the reference's text)
against tests/info_reference.py (an independent float64 restatement from the calculus) on explicit pair
sets, over rotations that real registrations produce, both branches of Eigen's eulerAngles(0, 1, 2),
the gimbal, roll near pi, translations up to 50 m and a 1e4-m offset.  No GPU.

Tolerances come from the reference's float sub-products (2 * Z3 * Z4 and the like, rounded to float
before they meet a double): 1e-7 of the largest entry of d2J/dX2 and of `middle` (measured: <= 2e-9 near
the origin, <= 4e-8 at the offset), and on the information matrix the perturbation bound of
info_reference.info_tolerance, which carries the measured conditions of H and M."""
import math

import numpy as np
import pytest

import info_reference as IR
from libwave_amd import synth

REL = 1e-7
OFFSET = np.array([12345.0, -54321.0, 250.0], np.float32)
POSES = {
    "identity": (0.0, 0.0, 0.0),
    "roll+0.05": (0.05, 0.0, 0.0),
    "roll-0.05": (-0.05, 0.0, 0.0),
    "pitch+0.05": (0.0, 0.05, 0.0),
    "pitch-0.05": (0.0, -0.05, 0.0),
    "yaw+0.05": (0.0, 0.0, 0.05),
    "yaw-0.05": (0.0, 0.0, -0.05),
    "rpy+": (0.4, -0.3, 0.7),
    "rpy-": (-0.4, 0.3, -0.7),
    "yaw2.5": (0.0, 0.0, 2.5),
    "roll~+pi": (math.pi - 1e-3, 0.1, 0.2),
    "roll~-pi": (-math.pi + 1e-3, 0.1, 0.2),
    "pitch~+pi/2": (0.1, math.pi / 2 - 1e-6, 0.2),
    "pitch~-pi/2": (0.1, -math.pi / 2 + 1e-6, 0.2),
}
# Eigen's flip branch is taken when the inverse rotation's first angle is positive, atan2(R12, R22) > 0:
# roll < 0 for a pure roll; for the composite poses as that sign comes out (both gimbal sides differ)
FLIPS = {"roll-0.05", "rpy-", "pitch~+pi/2"}
TRANSLATIONS = [(0.0, 0.0, 0.0), (3.0, -2.0, 1.0), (50.0, -20.0, 5.0)]


def _pairs(T, n=3000, seed=3, offset=False):
    """Source points b on the synthetic scene; matched target points a ~ T b (+ 2 cm noise), as a
    registration at T leaves them.  offset: the same pairs moved by OFFSET."""
    b = synth.scene(n, seed=seed)
    rng = np.random.default_rng(seed)
    a = (synth.transform_points(b, T) + rng.normal(0, 0.02, b.shape)).astype(np.float32)
    if offset:
        a, b = (a + OFFSET).astype(np.float32), (b + OFFSET).astype(np.float32)
    return b, a


def _close(got, want, rel, what):
    scale = np.abs(want).max()
    err = np.abs(got - want).max()
    assert err <= rel * scale, "%s: max |diff| %.3e > %.1e x %.3e" % (what, err, rel, scale)


def _check_censi(oracle, b, a, T):
    o = oracle.censi_from_pairs(b, a, T)
    r = IR.censi(b, a, T)
    _close(o["d2J_dX2"], r["H"], REL, "d2J/dX2")
    _close(o["middle"], r["M"], REL, "middle")
    err = np.abs(o["info"] - r["info"]).max()
    tol = IR.info_tolerance(r["H"], r["M"], REL)
    assert err <= tol, (err, tol, np.linalg.cond(r["H"]), np.linalg.cond(r["M"]))
    return o, r


@pytest.mark.parametrize("pose", list(POSES))
def test_euler_012_branch_and_value(oracle, pose):
    R = synth.make_T(rpy=POSES[pose])[:3, :3]
    e = IR.euler_012(R)
    np.testing.assert_allclose(oracle.euler_012(R), e, rtol=0, atol=1e-12)
    assert IR.euler_flipped(R) == (pose in FLIPS)
    # Rx(e0) Ry(e1) Rz(e2) reproduces R on either branch, e0 in [0, pi]
    np.testing.assert_allclose(IR.elem(0, e[0]) @ IR.elem(1, e[1]) @ IR.elem(2, e[2]), R, atol=1e-12)
    assert 0.0 <= e[0] <= math.pi
    if pose == "roll-0.05":   # the flip branch on a pure roll: (pi + roll, pi, +-pi)
        assert abs(e[0] - (math.pi - 0.05)) < 1e-12 and abs(e[1] - math.pi) < 1e-12
        assert abs(abs(e[2]) - math.pi) < 1e-12


@pytest.mark.parametrize("t", TRANSLATIONS, ids=["t0", "t3m", "t50m"])
@pytest.mark.parametrize("pose", list(POSES))
def test_censi_matches_the_calculus(oracle, pose, t):
    T = synth.make_T(t=t, rpy=POSES[pose])
    b, a = _pairs(T)
    _, r = _check_censi(oracle, b, a, T)
    assert np.linalg.cond(r["H"]) < 1e5   # near the origin the information is well determined


@pytest.mark.parametrize("pose", ["identity", "roll-0.05", "rpy+", "yaw2.5", "pitch~+pi/2"])
def test_censi_matches_the_calculus_far_from_the_origin(oracle, pose):
    """The same pairs 5.6e4 m out: H's condition reaches 1e10 ... 1e14 and M's 1e7 ... 1e12, so the
    information matrix the reference forms as (H^-1 M H^-1)^-1 is dominated by its own rounding (the
    bound's u cond(H)^2 cond(M) term exceeds |info|): H and M are held to 1e-7, info only to that bound."""
    T = synth.make_T(t=(3.0, -2.0, 1.0), rpy=POSES[pose])
    b, a = _pairs(T, offset=True)
    _, r = _check_censi(oracle, b, a, T)
    assert np.linalg.cond(r["H"]) > 1e9


@pytest.mark.parametrize("pose", ["roll+0.05", "roll-0.05", "rpy+", "rpy-", "yaw2.5", "roll~-pi"])
def test_censi_composed_rx_ry_rz_is_not_the_reference(oracle, pose):
    """Convention (a) has teeth: composing the restatement's rotation as Rx Ry Rz (the order eulerAngles
    decomposes in) moves the Hessian's coupling entries by far more than the tolerance."""
    T = synth.make_T(t=(3.0, -2.0, 1.0), rpy=POSES[pose])
    b, a = _pairs(T)
    o = oracle.censi_from_pairs(b, a, T)
    wrong = IR.censi(b, a, T, order=(0, 1, 2))
    assert np.abs(o["d2J_dX2"] - wrong["H"]).max() > 1e3 * REL * np.abs(o["d2J_dX2"]).max()


def test_censi_hessian_is_the_cost_hessian_by_autograd(oracle):
    """Convention (a) is a property of the cost, not of the restatement: torch's f64 autograd Hessian of
    J(t, theta) = sum |Rz Ry Rx(theta) a + t - b|^2 at theta = eulerAngles(0, 1, 2) equals the oracle's
    d2J/dX2, and the mixed derivative d2J/dz dx of one pair equals the restatement's D (rows z)."""
    torch = pytest.importorskip("torch")
    T = synth.make_T(t=(0.5, -1.0, 2.0), rpy=(0.4, -0.3, 0.7))
    b, a = _pairs(T, n=400)
    theta0 = IR.euler_012(T[:3, :3])

    def rot(th):
        c, s = torch.cos(th), torch.sin(th)
        o, z = torch.ones((), dtype=th.dtype), torch.zeros((), dtype=th.dtype)
        Rx = torch.stack([torch.stack([o, z, z]), torch.stack([z, c[0], -s[0]]), torch.stack([z, s[0], c[0]])])
        Ry = torch.stack([torch.stack([c[1], z, s[1]]), torch.stack([z, o, z]), torch.stack([-s[1], z, c[1]])])
        Rz = torch.stack([torch.stack([c[2], -s[2], z]), torch.stack([s[2], c[2], z]), torch.stack([z, z, o])])
        return Rz @ Ry @ Rx

    A = torch.tensor(a.astype(np.float64))
    B = torch.tensor(b.astype(np.float64))

    def J(x, A=A, B=B):
        e = A @ rot(x[3:]).T + x[:3] - B
        return (e * e).sum()

    x0 = torch.tensor(np.concatenate([T[:3, 3], theta0]))
    Hs = torch.autograd.functional.hessian(J, x0).numpy()
    o = oracle.censi_from_pairs(b, a, T)
    _close(o["d2J_dX2"], Hs, REL, "autograd d2J/dX2 vs oracle")

    # the mixed term of pair 0: d/dz (dJ/dx), z = (a, b)
    def grad_x(z):
        x = x0.clone().requires_grad_(True)
        g, = torch.autograd.grad(J(x, z[:3][None], z[3:][None]), x, create_graph=True)
        return g
    z0 = torch.cat([A[0], B[0]])
    Dt = torch.autograd.functional.jacobian(grad_x, z0).numpy()     # [x, z]
    R, dR, _ = IR.rotation_and_derivatives(theta0)
    e = R @ a[0].astype(np.float64) + T[:3, 3] - b[0].astype(np.float64)
    D = np.zeros((6, 6))
    D[:3, :3], D[3:, :3] = 2.0 * R.T, -2.0 * np.eye(3)
    for k in range(3):
        Ra = dR[k] @ a[0].astype(np.float64)
        D[:3, 3 + k], D[3:, 3 + k] = 2.0 * (R.T @ Ra + dR[k].T @ e), -2.0 * Ra
    np.testing.assert_allclose(Dt.T, D, rtol=1e-12, atol=1e-12 * np.abs(D).max())
    # and the Hessian of the Rx Ry Rz cost is not the reference's (O(1) apart in the coupling entries)
    wrong = IR.censi(b, a, T, order=(0, 1, 2))
    assert np.abs(wrong["H"][3:, 3:] - Hs[3:, 3:]).max() > 1e-3 * np.abs(Hs[3:, 3:]).max()


@pytest.mark.parametrize("edge", ["origin", "z_axis", "branch_cut"])
def test_censi_singular_spherical_jacobian(oracle, edge):
    """Points where the reference's spherical Jacobian is singular: (0, 0, 0) -> atan(0 / 0) = NaN, which
    poisons the whole information matrix; (0, 0, z) -> atan(+-inf) = +-pi / 2 (finite); (x < 0, 0, z) ->
    atan2's branch cut (+pi for +0, -pi for -0)."""
    T = synth.make_T(t=(0.2, -0.1, 0.05), rpy=(0.05, -0.03, 0.1))
    b, a = _pairs(T, n=1000)
    pts = {"origin": [[0.0, 0.0, 0.0]], "z_axis": [[0.0, 0.0, 4.0], [0.0, 0.0, -2.0]],
           "branch_cut": [[-5.0, 0.0, 1.0], [-3.0, -0.0, 2.0]]}[edge]
    e = np.array(pts, np.float32)
    b, a = np.vstack([b, e]), np.vstack([a, e])
    o = oracle.censi_from_pairs(b, a, T)
    r = IR.censi(b, a, T) if edge != "origin" else None
    if edge == "origin":
        assert np.isnan(o["info"]).all() and np.isnan(o["middle"]).all()
        with np.errstate(invalid="ignore"):
            J = IR.spherical_jacobian(e, [1.0, 1.0, 1.0])
        assert np.isnan(J).any()
        return
    assert np.isfinite(o["info"]).all()
    _close(o["d2J_dX2"], r["H"], REL, "d2J/dX2")
    _close(o["middle"], r["M"], REL, "middle")
    assert np.abs(o["info"] - r["info"]).max() <= IR.info_tolerance(r["H"], r["M"], REL)


@pytest.mark.parametrize("pose", ["identity", "roll-0.05", "rpy+", "yaw2.5", "roll~+pi"])
@pytest.mark.parametrize("offset", [False, True], ids=["near", "offset"])
def test_lum_matches_the_normal_equations(oracle, pose, offset):
    """estimateLUM on explicit pairs: p = the aligned source (PCL's float transform), q = its match."""
    T = synth.make_T(t=(3.0, -2.0, 1.0), rpy=POSES[pose])
    b, a = _pairs(T, offset=offset)
    Tf = T.copy()
    if offset:   # the pose that maps the moved source onto the moved target
        Tf[:3, 3] = T[:3, 3] + OFFSET - T[:3, :3] @ OFFSET
    p = oracle.transform_cloud_f(b, Tf)
    o = oracle.lum_from_pairs(p, a)
    r = IR.lum(p, a, pairs=(np.arange(len(p)), np.arange(len(p))))
    assert o["rc"] == 0
    # M'M: the same float products summed in double (summation order only)
    np.testing.assert_allclose(o["MM"], r["MM"], rtol=1e-12, atol=1e-12 * np.abs(r["MM"]).max())
    # s^2: both sum the same float terms sequentially in float; D differs by the solve only
    assert abs(o["ss"] - r["ss"]) <= 1e-6 * r["ss"]
    np.testing.assert_allclose(o["info"], r["info"], rtol=2e-6, atol=1e-9 * np.abs(r["info"]).max())


@pytest.mark.parametrize("rpy", [(0.05, 0.0, 0.0), (-0.05, 0.02, -0.03)], ids=["roll+", "roll-"])
def test_icp_match_estimators_against_the_restatement(oracle, rpy):
    """The oracle's whole match() + estimateInfo() at a rotated pose that an align from identity reaches;
    a third of the source has no match within max_corr; LUMold searched with max_corr 0.5 / 3 / 10."""
    T = synth.make_T(t=(0.3, -0.2, 0.1), rpy=rpy)
    ref, tgt, _ = synth.pair(6000, seed=11, T=T)
    far = np.arange(len(ref)) % 3 == 0
    ref = ref.copy()
    ref[far, 2] += 40.0                       # 40 m above the scene: nothing within 3 m
    m = oracle.IcpMatch(ref, tgt, max_corr=3.0, incremental_float=0)
    assert m.ok
    r_ref, r_tgt, fin, corr = m.clouds()
    assert (corr[far] < 0).all() and (corr[~far] >= 0).mean() > 0.99
    ok = corr >= 0
    i, j = np.flatnonzero(ok), corr[ok]
    lum, rc = m.lum()
    want = IR.lum(fin, r_tgt, pairs=(i, j))
    assert rc == 0
    np.testing.assert_allclose(lum, want["info"], rtol=2e-6, atol=1e-9 * np.abs(want["info"]).max())
    for mc in (0.5, 3.0, 10.0):
        lumold, _ = m.lumold(mc)
        want = IR.lum(fin, r_tgt, max_corr=mc)
        np.testing.assert_allclose(lumold, want["info"], rtol=2e-6, atol=1e-9 * np.abs(want["info"]).max())
    censi, _ = m.censi()
    r = IR.censi(r_ref[i], r_tgt[j], m.T)
    assert IR.euler_flipped(m.T[:3, :3]) == (rpy[0] < 0)
    assert np.abs(censi - r["info"]).max() <= IR.info_tolerance(r["H"], r["M"], REL)
