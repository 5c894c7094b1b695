"""Every output array and statistic of wm_sac_segment and wm_sac_segment_batch over a fixed set of runs, saved as one
.npz -- to compare two builds of the library byte for byte:

    python scripts/dev/dev_sac_dump.py --lib A/libwavematch_hip.so --out a.npz      (a fresh process per library)
    python scripts/dev/dev_sac_dump.py --lib B/libwavematch_hip.so --out b.npz
    python scripts/dev/dev_sac_dump.py --compare a.npz b.npz                        (exit status 1 if an array differs)

The runs: the twenty cases of tests/sac_reference.py with the refit on and off, each as a single call, in the groups of
tests/test_sac_batch_gpu.py and as a batch of one; option sac_round 1, 7, 256 and 1024; clouds in host and in device
memory; `negative` with points_out; a short capacity; one scene of 300 000 points.  kernel_ms is left out: it is a time."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

GROUP_A = ("exact_plane", "line", "point", "scene", "holes", "clumps_outliers", "noisy_plane", "utm_plane")
GROUP_B = ("line", "point", "lattice", "dups", "shell")
A = dict(distance_threshold=0.05, max_iterations=50)
B = dict(distance_threshold=0.5, max_iterations=1000)
PERP = dict(model=1, axis=(0, 0, 1), eps_angle=0.1)
PAR = dict(model=2, axis=(0, 0, 1), eps_angle=0.1)
GROUPS = {"A": (GROUP_A, A), "B": (GROUP_B, B), "decks": (("decks",), dict(distance_threshold=0.25, max_iterations=50)),
          "decks+slab": (("decks", "slab"), dict(distance_threshold=0.25, max_iterations=50)),
          "perp": (("noisy_plane", "scene", "shell"), dict(A, **PERP)), "par50": (("noisy_plane", "scene", "shell"), dict(A, **PAR)),
          "par200": (("noisy_plane", "scene", "shell"), dict(A, max_iterations=200, **PAR))}


def _np(a):
    return a if isinstance(a, np.ndarray) else a.cpu().numpy()


def put(store, key, got):
    """one dict of sac_segment, or one scan's of sac_segment_batch"""
    for f, v in got.items():
        if f == "kernel_ms":
            continue
        if v is None:
            v = np.zeros(0, np.uint8)
        store["%s/%s" % (key, f)] = np.asarray(_np(v) if hasattr(v, "shape") else v)


def put_batch(store, key, out):
    if isinstance(out, tuple):
        out, kept, offs = out
        store[key + "/kept"] = _np(kept)
        store[key + "/offsets"] = np.asarray(offs)
    for k, g in enumerate(out):
        put(store, "%s/%d" % (key, k), g)


def run(ctx):
    import torch
    import sac_reference as SR
    from libwave_amd import synth
    shapes = SR.shapes()
    dev = {n: torch.from_numpy(c.copy()).cuda() for n, c in shapes.items() if n in GROUP_A + GROUP_B + ("decks", "slab")}
    store = {}
    for opt in (0, 1):
        for i, (name, thr, max_it, extra) in enumerate(SR.CASES):
            kw = dict(distance_threshold=thr, max_iterations=max_it, optimize_coefficients=opt, **extra)
            key = "opt%d/%s" % (opt, SR.case_id(i))
            put(store, key + "/single", ctx.sac_segment(shapes[name], **kw))
            put(store, key + "/single-dev", ctx.sac_segment(dev[name], **kw))
            put_batch(store, key + "/batch1", ctx.sac_segment_batch([shapes[name]], **kw))
            put_batch(store, key + "/batch1-dev-neg", ctx.sac_segment_batch([dev[name]], points=True, negative=True, **kw))
        for g, (names, kw) in GROUPS.items():
            kw = dict(kw, optimize_coefficients=opt)
            key = "opt%d/group-%s" % (opt, g)
            put_batch(store, key + "/host", ctx.sac_segment_batch([shapes[n] for n in names], **kw))
            put_batch(store, key + "/dev", ctx.sac_segment_batch([dev[n] for n in names], **kw))
            put_batch(store, key + "/neg", ctx.sac_segment_batch([shapes[n] for n in names], points=True, negative=True, **kw))
            put_batch(store, key + "/neg-dev", ctx.sac_segment_batch([dev[n] for n in names], points=True, negative=True, **kw))
            put_batch(store, key + "/host-out", ctx.sac_segment_batch([dev[n] for n in names], out_mem=0, labels=False, **kw))
    for R in (1, 7, 256, 1024):
        ctx.set_option("sac_round", R)
        for name in ("lattice", "dups"):
            put(store, "round%d/%s" % (R, name), ctx.sac_segment(shapes[name], **B))
        for n in GROUP_A:
            put(store, "round%d/A/%s" % (R, n), ctx.sac_segment(shapes[n], **A))
        put_batch(store, "round%d/A/batch" % R, ctx.sac_segment_batch([shapes[n] for n in GROUP_A], **A))
        put_batch(store, "round%d/B/batch" % R, ctx.sac_segment_batch([shapes[n] for n in ("lattice", "dups", "shell")], **B))
    ctx.set_option("sac_round", 256)
    # short capacities, tiny scans, nothing finite
    scene = shapes["scene"]
    for cap in (0, 10, 1500):
        put(store, "cap%d/single" % cap, ctx.sac_segment(scene, cap=cap, **A))
        put_batch(store, "cap%d/batch" % cap, ctx.sac_segment_batch([scene, shapes["holes"]], cap=cap, points=True, **A))
        put_batch(store, "cap%d/batch1" % cap, ctx.sac_segment_batch([dev["scene"]], cap=cap, points=True, **A))
    nans = np.full((300, 3), np.nan, np.float32)
    tiny = [np.ascontiguousarray(scene[a:a + n]) for a, n in ((0, 0), (10, 1), (20, 2), (30, 3), (40, 4), (50, 65), (60, 257))]
    for k, c in enumerate(tiny + [nans]):
        put(store, "tiny/single/%d" % k, ctx.sac_segment(c, **A))
        put_batch(store, "tiny/batch1/%d" % k, ctx.sac_segment_batch([c], **A))
    put_batch(store, "tiny/batch", ctx.sac_segment_batch(tiny + [nans, scene], points=True, negative=True, **A))
    put_batch(store, "tiny/only", ctx.sac_segment_batch(tiny[:3], **A))
    rng = np.random.default_rng(17)
    big = np.ascontiguousarray(np.tile(scene, (7, 1)) + rng.uniform(-1e-3, 1e-3, (7 * len(scene), 3)), np.float32)
    put(store, "wrap/single", ctx.sac_segment(big, **A))
    put_batch(store, "wrap/batch", ctx.sac_segment_batch([np.ascontiguousarray(scene[:1000]), big, np.ascontiguousarray(scene[2000:2300])], **A))
    # one large scene
    P = synth.scene(300000, seed=9)
    Pd = torch.from_numpy(P).cuda()
    for opt in (0, 1):
        kw = dict(distance_threshold=0.05, optimize_coefficients=opt)
        put(store, "scene300k/opt%d/single" % opt, ctx.sac_segment(P, **kw))
        put(store, "scene300k/opt%d/single-dev" % opt, ctx.sac_segment(Pd, **kw))
        put(store, "scene300k/opt%d/it1000" % opt, ctx.sac_segment(Pd, max_iterations=1000, distance_threshold=0.2, optimize_coefficients=opt))
        put_batch(store, "scene300k/opt%d/batch1" % opt, ctx.sac_segment_batch([Pd], points=True, negative=True, **kw))
        put_batch(store, "scene300k/opt%d/batch" % opt, ctx.sac_segment_batch([scene, P, shapes["holes"]], **kw))
    return store


def compare(a, b):
    x, y = np.load(a), np.load(b)
    bad = [k for k in sorted(set(x.files) | set(y.files))
           if k not in x.files or k not in y.files or x[k].dtype != y[k].dtype or x[k].shape != y[k].shape or
           x[k].tobytes() != y[k].tobytes()]
    for k in bad[:40]:
        print("differs:", k)
    print("%d arrays compared, %d differ" % (len(set(x.files) | set(y.files)), len(bad)))
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default="")
    ap.add_argument("--out", default="")
    ap.add_argument("--compare", nargs=2, metavar="FILE")
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(*a.compare))
    from libwave_amd import capi
    if a.lib:
        capi.LIB_PATH = os.path.abspath(a.lib)  # (before the first Context: capi.lib() loads it once)
    ctx = capi.Context(0)
    store = run(ctx)
    ctx.close()
    np.savez_compressed(a.out, **store)
    print("%d arrays -> %s" % (len(store), a.out))


if __name__ == "__main__":
    main()
