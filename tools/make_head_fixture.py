"""Record what the reader sees in the reference's ``models/model_general_v3`` as a test fixture.

    python tools/make_head_fixture.py /path/to/reference [tests/golden/head_graph_model_general_v3.json]

Run where a reference checkout exists.  The fixture holds recorded results only - for every node of ``saved_model.pb`` its
function, name, op, inputs and decoded scalar attributes, and for every entry of ``variables.index`` its name, dtype and
shape - no graph bytes and no weights.  ``tests/test_head_loader.py`` feeds it to ``weights.dense_chain`` and
``weights.bundle_layer_entries``.
"""
from __future__ import annotations

import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from buzzdetect_amd import artifacts  # noqa: E402

SKIP_ATTRS = ("config_proto", "value")      # a serialized ConfigProto / a Const payload: not part of the structure


def record(model_dir: str) -> dict:
    nodes = artifacts.saved_model_nodes(os.path.join(model_dir, "saved_model.pb"))
    index = artifacts.read_bundle_index(artifacts.bundle_paths(model_dir)[0])
    return {
        "source": "models/model_general_v3 (saved_model.pb, variables/variables.index)",
        "nodes": [{"function": n.function, "name": n.name, "op": n.op, "inputs": list(n.inputs),
                   "attrs": {k: v for k, v in sorted(n.attrs.items()) if k not in SKIP_ATTRS}} for n in nodes],
        "index": [{"name": e.name, "dtype": e.dtype, "shape": list(e.shape)} for e in index.values()],
    }


def load(path: str):
    """(nodes as ``artifacts.GraphNode``, index as ``{name: artifacts.BundleEntry}``) from a recorded fixture."""
    with open(path) as f:
        rec = json.load(f)
    nodes = [artifacts.GraphNode(n["function"], n["name"], n["op"], tuple(n["inputs"]), n["attrs"], None) for n in rec["nodes"]]
    index = {e["name"]: artifacts.BundleEntry(e["name"], e["dtype"], tuple(e["shape"]), 0, 0, 0, 0) for e in rec["index"]}
    return nodes, index


if __name__ == "__main__":
    ref = sys.argv[1]
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                             "tests", "golden", "head_graph_model_general_v3.json")
    with open(out, "w") as f:
        json.dump(record(os.path.join(ref, "models", "model_general_v3")), f, indent=1)
        f.write("\n")
    print(out)
