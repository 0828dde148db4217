#!/usr/bin/env python3
"""Write tests/golden/tsne_quality.json: what the NumPy statement of the map (tests/tsne_cases.py) reaches on the two quality
fixtures, in float64 and in plain float32 - 10-NN label purity, the share of preserved neighbours and the divergence.  The
float64 run of 1025 rows takes most of a minute, which is why it is recorded and not recomputed by the tests.

    python tools/make_tsne_golden.py

The lists are those of the host restatement of the neighbour search (tests/propagate_cases.planted_lists), which the device
lists equal in every bit; everything after them is NumPy."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import propagate_cases, tsne_cases as C  # noqa: E402

K = 48
PERPLEXITY = 16.0
FIXTURES = ((513, 32, 100, 150), (1025, 32, 250, 250))          # rows, planted clusters, exaggerated iterations, the rest


def run(w, clusters, early, rest):
    e, truth, ids, sims = propagate_cases.planted_lists(w, clusters, K)
    plane = C.pca_plane(e)
    start = C.start_of(plane)
    out = {"rows": w, "clusters": clusters, "k": K, "perplexity": PERPLEXITY, "exaggeration_iter": early, "n_iter": early + rest,
           "pca": {"purity10": C.purity10(plane, truth), "preservation": C.preservation(plane, ids)}}
    for name, dt in (("float64", np.float64), ("float32", np.float32)):
        p, _ = C.affinities(ids, sims, PERPLEXITY, dt)
        row_start, nbr, big = C.joint(ids, p)
        y, kl = C.fit(row_start, nbr, big, start, dt, n_iter=early + rest, exaggeration_iter=early)
        out[name] = {"purity10": C.purity10(y, truth), "preservation": C.preservation(y, ids), "kl": float(kl)}
        print(w, name, out[name], flush=True)
    return out


if __name__ == "__main__":
    found = {f"{w}x{c}": run(w, c, early, rest) for w, c, early, rest in FIXTURES}
    path = os.path.join(ROOT, "tests", "golden", "tsne_quality.json")
    with open(path, "w") as f:
        json.dump(found, f, indent=1, sort_keys=True)
        f.write("\n")
    print(path)
