"""wm_cluster_extract (libwave_amd/csrc/wm_cluster.hip) restated in float32 numpy + scipy: the checker of
tests/test_cluster_gpu.py, in the manner of outlier_reference.py.

  edges     r2 = (float32) (tolerance * tolerance), the product in double; two different finite points are joined iff
            d2 < r2 (strict), d2 = (dx * dx + dy * dy) + dz * dz in float32, every operation rounded, none fused (as
            outlier_reference.radius_counts forms it).
  clusters  the connected components of that graph (scipy.sparse.csgraph.connected_components); kept iff
            max(min_cluster_size, 1) <= size <= max_cluster_size; largest first, equal sizes by their smallest member
            index; the members of a cluster ascending.  labels: the cluster's rank, REJECTED for a point of a component
            the size rule drops, NONE for a non-finite point (which is nobody's neighbour).
  two forms components_brute: every pair, in chunks.  components: candidate pairs from a float64 kd-tree at
            tolerance * 1.001 + 1e-6 (at the utm shapes' scale this covers the float rounding of the differences), the
            float32 d2 re-formed on them, the same strict test.  tests/test_cluster_reference_cpu.py holds the two to
            each other on every (shape, tolerance) the device is compared on."""
import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

import knn_reference as KR

NONE, REJECTED = -1, -2
INT_MAX = 2 ** 31 - 1


def _r2(tolerance):
    return np.float32(float(tolerance) * float(tolerance))


def _finish(n, cand, rows, cols, min_cluster_size, max_cluster_size, extra):
    """cand: the finite points' caller indices, ascending; rows / cols: edges between positions in cand."""
    m = len(cand)
    n_comp, lab = connected_components(coo_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(m, m)).tocsr(),
                                       directed=False) if m else (0, np.zeros(0, np.int64))
    sizes = np.bincount(lab, minlength=n_comp).astype(np.int64)
    first = np.unique(lab, return_index=True)[1] if m else np.zeros(0, np.int64)
    min_idx = cand[first].astype(np.int64)  # (cand ascends: a component's first member is its smallest index)
    kept = np.nonzero((sizes >= max(int(min_cluster_size), 1)) & (sizes <= int(max_cluster_size)))[0]
    order = kept[np.lexsort((min_idx[kept], -sizes[kept]))]
    rank = np.full(n_comp, REJECTED, np.int64)
    rank[order] = np.arange(len(order))
    labels = np.full(n, NONE, np.int32)
    labels[cand] = rank[lab]
    members = np.nonzero(labels >= 0)[0]
    indices = members[np.argsort(labels[members], kind="stable")].astype(np.int32)
    offsets = np.r_[0, np.cumsum(sizes[order])].astype(np.uint32)
    out = dict(labels=labels, indices=indices, offsets=offsets, n_clusters=len(order), n_out=len(indices), n_finite=m,
               n_components=int(n_comp), n_clustered=len(indices), largest=int(sizes[order[0]]) if len(order) else 0,
               component_sizes=np.sort(sizes)[::-1], n_edges=len(rows))
    out.update(extra)
    return out


def components_brute(cloud, tolerance, min_cluster_size=1, max_cluster_size=INT_MAX, chunk=256):
    """Every pair of finite points.  Also n_edges (unordered pairs with d2 < r2) and n_at_r2 (... with d2 == r2)."""
    cloud = np.ascontiguousarray(cloud, np.float32)
    finite = np.isfinite(cloud).all(1)
    cand = np.nonzero(finite)[0]
    c = cloud[cand]
    r2 = _r2(tolerance)
    rows, cols, at = [], [], 0
    for s in range(0, len(cand), chunk):
        q = c[s:s + chunk]
        dx = q[:, None, 0] - c[None, :, 0]
        dy = q[:, None, 1] - c[None, :, 1]
        dz = q[:, None, 2] - c[None, :, 2]
        d2 = (dx * dx + dy * dy) + dz * dz  # float32 arrays: every operation rounded, none fused (as KR._top)
        assert d2.dtype == np.float32
        upper = np.arange(len(cand))[None, :] > np.arange(s, s + len(q))[:, None]  # each unordered pair once
        a, b = np.nonzero((d2 < r2) & upper)
        rows.append(a + s)
        cols.append(b)
        at += int(((d2 == r2) & upper).sum())
    rows = np.concatenate(rows) if rows else np.zeros(0, np.int64)
    cols = np.concatenate(cols) if cols else np.zeros(0, np.int64)
    return _finish(len(cloud), cand, rows, cols, min_cluster_size, max_cluster_size, dict(n_at_r2=at))


def components(cloud, tolerance, min_cluster_size=1, max_cluster_size=INT_MAX):
    """Candidate pairs from a float64 kd-tree, the float32 test on them."""
    from scipy.spatial import cKDTree
    cloud = np.ascontiguousarray(cloud, np.float32)
    finite = np.isfinite(cloud).all(1)
    cand = np.nonzero(finite)[0]
    c = cloud[cand]
    r2 = _r2(tolerance)
    rows = cols = np.zeros(0, np.int64)
    if len(cand) > 1:
        pairs = cKDTree(c.astype(np.float64)).query_pairs(float(tolerance) * 1.001 + 1e-6, output_type="ndarray")
        a, b = c[pairs[:, 0]], c[pairs[:, 1]]
        dx, dy, dz = a[:, 0] - b[:, 0], a[:, 1] - b[:, 1], a[:, 2] - b[:, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        assert d2.dtype == np.float32
        ok = d2 < r2
        rows, cols = pairs[ok, 0], pairs[ok, 1]
    return _finish(len(cloud), cand, rows, cols, min_cluster_size, max_cluster_size, {})


def with_size_rule(ref, min_cluster_size, max_cluster_size):
    """The outputs of `ref` (computed with the default size rule: every component kept) under another size rule."""
    n = len(ref["labels"])
    cand = np.nonzero(ref["labels"] != NONE)[0]
    lab = ref["labels"][cand].astype(np.int64)
    # a star per component: the same components, nothing searched again
    first = np.unique(lab, return_index=True)[1]
    return _finish(n, cand, np.arange(len(cand)), first[lab], min_cluster_size, max_cluster_size, {})


# ------------------------------------------------------------------ the shapes of this checker's own
def _build_shapes():
    rng = np.random.default_rng(201)
    s = np.arange(4096) * 0.09
    helix = np.c_[3 * np.cos(s / 3), 3 * np.sin(s / 3), 0.02 * s].astype(np.float32)
    helix = helix[rng.permutation(len(helix))]  # a 4096-point path, indices unrelated to position
    x = np.float32(np.arange(1024) * 0.125)
    z = np.zeros(1024, np.float32)
    rails = np.r_[np.c_[x, z, z], np.c_[x, z + np.float32(0.25), z]].astype(np.float32)
    rails = rails[rng.permutation(len(rails))]  # every coordinate and distance exactly representable
    out = dict(helix=np.ascontiguousarray(helix), rails=np.ascontiguousarray(rails))
    for c in out.values():
        c.setflags(write=False)
    return out


_SHAPES = None


def shapes():
    """name -> float32 [n, 3]: knn_reference's twelve and the two above (read-only, built once)."""
    global _SHAPES
    if _SHAPES is None:
        _SHAPES = dict(KR.shapes(), **_build_shapes())
    return _SHAPES


# what tests/test_cluster_gpu.py runs, and tests/test_cluster_reference_cpu.py holds the two forms to each other on
TOLERANCES = [0.05, 0.5, 0.5000001, 2.0]
OWN = {"helix": [0.1, 0.08], "rails": [0.25, 0.2500001, 0.125, 0.1250001]}
CASES = [(name, t) for name in KR.NAMES for t in TOLERANCES] + [(name, t) for name in OWN for t in OWN[name]]
BIG_N, BIG_SEED, BIG_TOLERANCES = 270000, 5, [0.1, 0.3]  # one size above the 256k sort switch (synth.scene)

_BRUTE = {}
_BIG = {}


def brute_case(name, tolerance):
    """components_brute of a named shape with the default size rule, computed once."""
    key = (name, float(tolerance))
    if key not in _BRUTE:
        _BRUTE[key] = components_brute(shapes()[name], tolerance)
    return _BRUTE[key]


def big_cloud():
    from libwave_amd import synth
    if "cloud" not in _BIG:
        _BIG["cloud"] = synth.scene(BIG_N, seed=BIG_SEED)
    return _BIG["cloud"]


def big_case(tolerance):
    """components of the large scene (a brute force over 270 000 points is out of reach), computed once."""
    if tolerance not in _BIG:
        _BIG[tolerance] = components(big_cloud(), tolerance)
    return _BIG[tolerance]
