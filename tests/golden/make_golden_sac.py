#!/usr/bin/env python3
"""Record tests/golden/sac_refit_bits.json -- what wm_sac_segment returns WITH THE REFIT, bit for bit, on the library as
it stands (needs the GPU).  tests/test_sac_gpu.py holds the refit to bounds against a float64 eigh and
tests/test_sac_batch_gpu.py holds a batch to the single call; neither pins the returned coefficients' bits, which depend
on which wave feeds which bin of the refit's sums and on the order the bins are added in.  tests/test_sac_pinned_gpu.py
holds the single call and the batch to this record.

The inputs: the twenty cases of tests/sac_reference.py with optimize_coefficients = 1; the "scene x 7" cloud of
test_sac_batch_gpu.py (more than 16 384 points: the 256 bins wrap) and the 4- and 65-point slices of its
test_scan_boundaries, at distance_threshold 0.05, max_iterations 50.  Per input: rc, the words of the returned and of
the model's coefficients, refined, the loop's counters, n_out, and the SHA-256 of the indices, of the labels and of the
input itself -- the last tells a drift of the generators from a change of the library.

    python tests/golden/make_golden_sac.py [--lib PATH] [--out FILE]     # rewrites sac_refit_bits.json
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import sac_reference as SR  # noqa: E402

PATH = os.path.join(HERE, "sac_refit_bits.json")
COUNTERS = ("iterations", "skipped", "hypotheses", "best_hypothesis", "n_inliers_model", "n_inliers", "n_finite", "rounds")
A = dict(distance_threshold=0.05, max_iterations=50)


def _sha(a):
    return None if a is None else hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _words(a):
    return None if a is None else [int(v) for v in np.asarray(a, np.float32).view(np.uint32)]


def inputs():
    """-> [(id, cloud float32 [n, 3], keywords of sac_segment)], the order of the record"""
    from libwave_amd import synth
    shapes = SR.shapes()
    out = []
    for i, (name, thr, max_it, extra) in enumerate(SR.CASES):
        kw = dict(distance_threshold=thr, max_iterations=max_it)
        for k, v in extra.items():
            kw[{"prob": "probability"}.get(k, k)] = v
        out.append((SR.case_id(i), shapes[name], kw))
    scene = shapes["scene"]
    rng = np.random.default_rng(17)
    out.append(("scene-x-7", np.ascontiguousarray(np.tile(scene, (7, 1)) + rng.uniform(-1e-3, 1e-3, (7 * len(scene), 3)),
                                                   np.float32), dict(A)))
    big = synth.scene(5000, seed=4)
    out.append(("scene5000[524:+4]", np.ascontiguousarray(big[524:528]), dict(A)))
    out.append(("scene5000[217:+65]", np.ascontiguousarray(big[217:282]), dict(A)))
    return [(what, P, dict(kw, optimize_coefficients=1)) for what, P, kw in out]


def digest(got):
    """what the record keeps of a dict of Context.sac_segment (or of one scan of sac_segment_batch), host arrays"""
    rec = dict(rc=int(got["rc"]), coefficients=_words(got["coefficients"]), model_coefficients=_words(got["model_coefficients"]),
               refined=int(got["refined"]), n_out=int(got["n_out"]), indices_sha256=_sha(got["indices"]),
               labels_sha256=_sha(got["labels"]))
    rec.update({k: int(got[k]) for k in COUNTERS})
    return rec


def load():
    with open(PATH) as f:
        return json.load(f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default="", help="the library to record (default: the tree's)")
    ap.add_argument("--out", default=PATH)
    a = ap.parse_args()
    from libwave_amd import capi
    if a.lib:
        capi.LIB_PATH = os.path.abspath(a.lib)
    ctx = capi.Context(0)
    rec = {}
    for what, P, kw in inputs():
        rec[what] = dict(digest(ctx.sac_segment(P, **kw)), input_sha256=_sha(P), n=len(P))
        print(what, rec[what]["rc"], rec[what]["refined"], rec[what]["coefficients"])
    ctx.close()
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
