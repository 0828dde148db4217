"""Write a trained-model directory in the reference's layout from Python, without TensorFlow.

    python tools/modelgen.py OUT_DIR --widths 256 13 --activations relu linear [--seed 1] [--name model_mine]

The writer lives in the package (``buzzdetect_amd/modeldir.py``; ``buzzdetect_amd.train.save_model`` writes fitted heads
through it); its functions are importable from here under the names they always had.  ``write_model_dir`` lays down what ``buzzdetect_amd.weights.read_model_dir`` reads - and what a Keras ``model.save()`` of
a Sequential of Dense layers leaves behind, as far as that reader looks:

    config_model.json                        classes, embeddername, digits_results
    saved_model.pb                           SavedModel{MetaGraphDef{GraphDef{nodes, FunctionDefLibrary}}}: the variables and
                                             the serving call in the main graph; in the library the signature wrapper and
                                             ``__inference__wrapped_model_N`` with the inlined body under the node names Keras
                                             gives them (``<model>/dense_1/MatMul/ReadVariableOp``, ``.../MatMul``,
                                             ``.../BiasAdd``, ``.../Relu``, ``Identity``, ``NoOp``)
    variables/variables.index                TensorBundle index: a LevelDB table (one data block, block trailers with masked
                                             CRC-32C, 48-byte footer) of BundleEntryProto values
    variables/variables.data-00000-of-00001  the tensors: ``layer_with_weights-k/{kernel,bias}`` and, as a real bundle has
                                             them, optimizer slots of the same shapes (decoys: filled with other values)
    tests/metrics.csv                        threshold / precision / sensitivity / fpr rows

Written from the formats (protobuf wire format, the TensorBundle and LevelDB table layouts as ``buzzdetect_amd/artifacts.py``
restates them), not from any existing file.  ``faults`` plants what the reader must refuse (tests/test_head_loader.py).
"""
from __future__ import annotations

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from buzzdetect_amd.modeldir import (  # noqa: E402,F401  (re-exported)
    ACTIVATION_OPS, DT_DOUBLE, DT_FLOAT, DT_INT64, DT_RESOURCE, DT_STRING, EXAMPLE_STACKS, MODEL_PY, attr_bool, attr_func,
    attr_shape, attr_type, bundle_bytes, crc32c, default_metrics, f_bytes, f_str, f_varint, function, glorot_layers,
    layer_scope, masked_crc, node, saved_model_bytes, shape_proto, table_block, varint, write_model_dir, write_model_py)


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("out_dir", help="the models directory; the model lands in OUT_DIR/NAME")
    ap.add_argument("--name", default="model_mine")
    ap.add_argument("--widths", type=int, nargs="+", default=[256, 13])
    ap.add_argument("--activations", nargs="+", default=None, help="one per layer: linear relu sigmoid tanh softmax")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--digits-results", type=int, default=2)
    a = ap.parse_args()
    acts = a.activations or ["relu"] * (len(a.widths) - 1) + ["linear"]
    path = write_model_dir(os.path.join(a.out_dir, a.name), glorot_layers(a.widths, acts, a.seed), seed=a.seed,
                           digits_results=a.digits_results)
    write_model_py(path, a.name, digits_results=a.digits_results)
    print(path)


if __name__ == "__main__":
    main()
