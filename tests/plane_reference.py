"""Point-to-plane ICP restated in float64 numpy: the checker of WM_ICP_PLANE (libwave_amd/csrc/wm_plane.hip), in the
manner of info_reference.py / ground_reference.py.

  knn / normals   the k nearest points of a cloud's own points (the point itself included; float32 squared distances
                  formed operation by operation as the device forms them, ties by index), the covariance of the
                  neighbourhood in float64 about its mean, the eigenvector of the smallest eigenvalue turned towards
                  the origin (n . p <= 0), the curvature lambda0 / (lambda0 + lambda1 + lambda2)
  plane_sums      the 29 sums of the public GN layout: n, sum d2, upper triangle of J^T J, J^T r with J = [n, p x n],
                  r = n . (p - q)
  step            (J^T J) delta = -J^T r, T_k = [exp(d omega) | d t]; `degenerate` = a Cholesky pivot not above
                  PIVOT_TOL x the largest diagonal entry
  align           the loop: search under the float32 pose (the oracle's kd-tree: exact nearest neighbours, PCL's
                  distance gate), sums, step, pcl::registration::DefaultConvergenceCriteria as icp_apply_stats states it
                  (libwave_amd/csrc/wm_icp_step.hpp); the criteria's MSE is the mean point-to-point d2
  match           ICPMatcher::match()'s three branches around align (wave_matching/src/icp.cpp:75-133)
"""
import numpy as np

DEFAULT_K = 20
PIVOT_TOL = 1e-12  # kPlanePivotTol (wm_plane.hip)
CONV_NOT, CONV_ITERATIONS, CONV_TRANSFORM, CONV_ABS_MSE, CONV_REL_MSE, CONV_NO_CORR, CONV_FORCED, CONV_DEGENERATE = range(8)
STATE_NAMES = ["NOT_CONVERGED", "ITERATIONS", "TRANSFORM", "ABS_MSE", "REL_MSE", "NO_CORRESPONDENCES", "FORCED", "DEGENERATE"]


# ------------------------------------------------------------------ neighbourhoods and normals
def knn(xyz, k, chunk=256):
    """-> (idx [n, k + 1], d2 [n, k + 1]): the k + 1 nearest points of every point among the cloud's finite points,
    ascending by (float32 d2, index).  Rows of non-finite points are -1 / inf."""
    xyz = np.ascontiguousarray(xyz, np.float32)
    n = len(xyz)
    finite = np.isfinite(xyz).all(1)
    cand = np.nonzero(finite)[0]
    c = xyz[cand]
    m = min(k + 1, len(cand))
    idx = np.full((n, k + 1), -1, np.int64)
    d2o = np.full((n, k + 1), np.inf, np.float32)
    for s in range(0, len(cand), chunk):
        q = c[s:s + chunk]
        dx = q[:, None, 0] - c[None, :, 0]
        dy = q[:, None, 1] - c[None, :, 1]
        dz = q[:, None, 2] - c[None, :, 2]
        d2 = (dx * dx + dy * dy) + dz * dz  # float32, every operation rounded: g_d2 (wm_gicp_dev.hpp)
        key = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | cand[None, :].astype(np.uint64)
        part = np.partition(key, m - 1, axis=1)[:, :m]
        part.sort(axis=1)
        rows = cand[s:s + chunk]
        idx[rows, :m] = (part & np.uint64(0xFFFFFFFF)).astype(np.int64)
        d2o[rows, :m] = (part >> np.uint64(32)).astype(np.uint32).view(np.float32)
    return idx, d2o


def normals(xyz, k=DEFAULT_K, nbrs=None, origin=None):
    """-> dict(normal [n, 3], curvature [n], eig [n, 3] ascending, gap [n] = (l1 - l0) / l2, tie [n] = the k-th and
    (k + 1)-th neighbour distances tie in float, valid [n]).  nbrs: (idx, d2) of k + 1 neighbours per point from elsewhere
    (-1: none).  origin: subtracted from the coordinates, in float64, before the covariance is formed -- for a cloud far
    from zero, whose covariance about raw coordinates loses (offset^2 x 2^-52) / spread^2 to cancellation; exact when the
    origin is a whole number.  The flip still looks at the true coordinates."""
    xyz = np.ascontiguousarray(xyz, np.float32)
    n = len(xyz)
    idx, d2 = nbrs if nbrs is not None else knn(xyz, k)
    valid = idx[:, k - 1] >= 0
    P = xyz.astype(np.float64)
    Q = P if origin is None else P - np.asarray(origin, np.float64)
    nb = Q[np.where(idx[:, :k] >= 0, idx[:, :k], 0)]  # [n, k, 3]
    mean = nb.mean(1, keepdims=True)
    d = nb - mean
    cov = np.einsum("nka,nkb->nab", d, d) / k
    cov[~valid] = np.eye(3)
    w, v = np.linalg.eigh(cov)  # ascending
    nrm = v[:, :, 0].copy()
    flip = np.einsum("na,na->n", nrm, P) > 0
    nrm[flip] *= -1
    tot = w.sum(1)
    ok = valid & (w[:, 2] > 0)
    curv = np.where(ok, w[:, 0] / np.where(tot > 0, tot, 1.0), 0.0)
    nrm[~ok] = 0.0
    gap = np.where(ok, (w[:, 1] - w[:, 0]) / np.where(w[:, 2] > 0, w[:, 2], 1.0), 0.0)
    tie = (idx.shape[1] > k) & (idx[:, k] >= 0) & (d2[:, k - 1] == d2[:, k])
    return dict(normal=nrm, curvature=curv, eig=w, gap=gap, tie=tie, valid=ok)


def angle(a, b):
    """angle between the LINES of two unit vectors (sign aside), well conditioned near 0"""
    return np.arcsin(np.minimum(1.0, np.linalg.norm(np.cross(a, b), axis=1)))


def check_normals(got, cloud, k, what, ref=None, cap=0.03):
    """The device's (nx, ny, nz, curvature) rows against the reference's (`ref`: normals(cloud, k) unless given): unit
    length, 1e-6 rad, 1e-6 in curvature, turned towards the origin -- on every point but those whose normal the data
    does not determine (eigen-gap < 1e-3, or a float tie at the k-th neighbour), which may be `cap` of the cloud at
    the most.  -> (largest angle, largest curvature difference)."""
    if ref is None:
        ref = normals(cloud, k)
    out = (ref["gap"] < 1e-3) | ref["tie"]
    share = out.mean()
    print("%s: left out %.3f %%" % (what, 100 * share))
    assert share <= cap, (what, share)
    use = ~out & ref["valid"]
    g = got[use, :3].astype(np.float64)
    assert np.abs(np.linalg.norm(g, axis=1) - 1.0).max() < 1e-6
    ang = angle(g, ref["normal"][use])
    curv = np.abs(got[use, 3] - ref["curvature"][use])
    print("%s: max angle %.3e rad, max curvature diff %.3e" % (what, ang.max(), curv.max()))
    assert ang.max() <= 1e-6, (what, ang.max())
    assert curv.max() <= 1e-6, (what, curv.max())
    p = cloud[use].astype(np.float64)
    ndotp = np.einsum("na,na->n", g, p)
    rounding = 1e-6 * np.linalg.norm(p, axis=1)
    assert (ndotp <= rounding).all(), what                      # n . p <= 0: towards the origin
    same = np.einsum("na,na->n", g, ref["normal"][use]) > 0
    assert (same | (np.abs(ndotp) <= rounding)).all(), what
    return ang.max(), curv.max()


# ------------------------------------------------------------------ sums and step
def transform_f32(xyz, T):
    """The source under the pose as the search kernels form it: float32 rows of T, products and sums rounded one by one."""
    Tf = np.asarray(T, np.float64).astype(np.float32)
    x, y, z = (np.ascontiguousarray(xyz[:, a], np.float32) for a in range(3))
    out = np.empty((len(xyz), 3), np.float32)
    for r in range(3):
        out[:, r] = ((Tf[r, 0] * x + Tf[r, 1] * y) + Tf[r, 2] * z) + Tf[r, 3]
    return out


def plane_sums(p, q, nq, d2):
    """p: matched source points under the pose, q: their matches, nq: the matches' normals (zero rows: no normal),
    d2: the search's float32 squared distances -> the 32-slot block (GN layout)."""
    p = np.asarray(p, np.float64)
    q = np.asarray(q, np.float64)
    nq = np.asarray(nq, np.float64)
    st = np.zeros(32)
    st[0] = len(p)
    st[1] = np.asarray(d2, np.float64).sum()
    has = (nq != 0).any(1)
    p, q, nq = p[has], q[has], nq[has]
    J = np.concatenate([nq, np.cross(p, nq)], axis=1)
    r = np.einsum("na,na->n", nq, p - q)
    H = J.T @ J
    st[2:23] = H[np.triu_indices(6)]
    st[23:29] = J.T @ r
    return st


def unpack(st):
    H = np.zeros((6, 6))
    H[np.triu_indices(6)] = st[2:23]
    H = H + H.T - np.diag(np.diag(H))
    return H, st[23:29].copy()


def degenerate(st):
    H, _ = unpack(st)
    dmax = np.diag(H).max()
    if not dmax > 0:
        return True
    L = np.zeros((6, 6))
    for i in range(6):
        for j in range(i + 1):
            s = H[i, j] - L[i, :j] @ L[j, :j]
            if i == j:
                if not s > PIVOT_TOL * dmax:
                    return True
                L[i, i] = np.sqrt(s)
            else:
                L[i, j] = s / L[j, j]
    return False


def rodrigues(w):
    th = np.linalg.norm(w)
    a, b = (1.0, 0.5) if th < 1e-12 else (np.sin(th) / th, (1.0 - np.cos(th)) / (th * th))
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return np.eye(3) + a * K + b * (K @ K)


def step(st):
    """-> T_k (4x4) of one Gauss-Newton step from the sums (gn6_from_stats)."""
    H, g = unpack(st)
    delta = np.linalg.solve(H, -g)
    Tk = np.eye(4)
    Tk[:3, :3] = rodrigues(delta[3:])
    Tk[:3, 3] = delta[:3]
    return Tk


# ------------------------------------------------------------------ the loop
def correspondences(tree, tgt, src_f, max_corr):
    """PCL's gate on the exact nearest neighbour: accepted unless (double) d2 > max_corr^2."""
    idx, d2 = tree.nn(src_f)
    keep = d2.astype(np.float64) <= float(max_corr) ** 2
    return np.nonzero(keep)[0], idx[keep], d2[keep]


def align(oracle, src, tgt, max_corr=3.0, max_iter=100, t_eps=1e-8, fit_eps=1e-2, k=DEFAULT_K, tgt_normals=None,
          prev_mse=None, trace=None):
    """-> dict(T, converged, iterations, state, n_corr, mse, margin): `margin` = the smallest relative distance of a
    stop decision's quantity from its threshold over the run (how close the run came to deciding otherwise)."""
    src = np.ascontiguousarray(src, np.float32)
    tgt = np.ascontiguousarray(tgt, np.float32)
    fin_s = np.isfinite(src).all(1)
    src = src[fin_s]
    if tgt_normals is None:
        tgt_normals = normals(tgt, k)["normal"]
    fin_t = np.isfinite(tgt).all(1)
    tmap = np.nonzero(fin_t)[0]
    tree = oracle.KdTree(tgt[fin_t])
    T = np.eye(4)
    prev = np.finfo(np.float64).max if prev_mse is None else prev_mse
    out = dict(T=None, converged=False, iterations=0, state=CONV_NOT, n_corr=0, mse=0.0, margin=np.inf)
    it = 0
    while True:
        pf = transform_f32(src, T)
        si, ti, d2 = correspondences(tree, tgt, pf, max_corr)
        ti = tmap[ti]
        n = len(si)
        out["n_corr"] = n
        out["mse"] = mse = float(d2.astype(np.float64).sum() / n) if n else 0.0
        if n < 3:
            out["state"] = CONV_NO_CORR
            break
        st = plane_sums(pf[si], tgt[ti], tgt_normals[ti], d2)
        if degenerate(st):
            out["state"] = CONV_DEGENERATE
            break
        Tk = step(st)
        T = Tk @ T
        it += 1
        out["iterations"] = it
        if trace is not None:
            trace.append(dict(T=T.copy(), mse=mse, n=n))
        if it >= max_iter:
            out["state"], out["converged"] = CONV_ITERATIONS, True
            break
        cos_angle = 0.5 * (Tk[0, 0] + Tk[1, 1] + Tk[2, 2] - 1.0)
        tsq = float(Tk[:3, 3] @ Tk[:3, 3])
        rel = abs(mse - prev) / prev
        out["margin"] = min(out["margin"], abs(rel - fit_eps) / fit_eps, abs(tsq - t_eps) / t_eps)
        state = CONV_NOT
        if cos_angle >= 1.0 - t_eps and tsq <= t_eps:
            state = CONV_TRANSFORM
        elif abs(mse - prev) < 1e-12:
            state = CONV_ABS_MSE
        elif rel < fit_eps:
            state = CONV_REL_MSE
        if state != CONV_NOT:
            out["state"], out["converged"] = state, True
            break
        prev = mse
    out["prev_mse"] = prev
    if out["converged"]:
        out["T"] = T
    return out


def match(oracle, ref, tgt, res=-1.0, multiscale_steps=0, max_corr=3.0, **kw):
    """ICPMatcher::match() (icp.cpp:75-133) with the plane metric: per scale the normals of the FILTERED target.
    -> (T or None, [align results per scale])."""
    runs = []
    if not res > 0:
        r = align(oracle, ref, tgt, max_corr=max_corr, **kw)
        return r["T"], [r]
    steps = max(int(multiscale_steps), 0)
    running = np.eye(4)
    prev = None
    for i in range(steps, -1, -1):
        leaf = np.float32(2.0 ** i * res)
        fr, ft = oracle.voxel_grid(ref, leaf), oracle.voxel_grid(tgt, leaf)
        mc = max_corr
        if steps > 0:
            fr = oracle.transform_cloud_d(fr, running)
            mc = 2.0 ** i * max_corr
        r = align(oracle, fr, ft, max_corr=mc, prev_mse=prev, **kw)
        runs.append(r)
        prev = r["prev_mse"]  # one matcher object: the criteria keep their previous MSE across aligns
        if not r["converged"]:
            return None, runs
        running = r["T"] @ running
    return running, runs


# ------------------------------------------------------------------ the issue's pairs
def split_pair(oracle, scan, t, yaw_deg=0.0, pitch_deg=0.0):
    """testscan voxelled at 0.1 m: the even-index points as source, the odd-index points moved by the perturbation
    as target (the reference's fixture: target = perturb * ref, result compared with perturb)."""
    from libwave_amd import synth
    pts = oracle.voxel_grid(scan, 0.1)
    P = synth.make_T(t, (0.0, np.deg2rad(pitch_deg), np.deg2rad(yaw_deg)))
    return pts[0::2].copy(), synth.transform_points(pts[1::2], P), P


SPLIT_PERTURBATIONS = [((0.2, 0.0, 0.0), 0.0, 0.0), ((0.5, 0.1, 0.0), 3.0, 0.0), ((1.0, 0.5, 0.05), 5.0, 1.0)]
