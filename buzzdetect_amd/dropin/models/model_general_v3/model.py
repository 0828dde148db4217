"""`model_general_v3` on the MI355X engine (reference: models/model_general_v3/model.py:6-31).

The reference chains ``embedder.embed`` and a Dense(1024 -> 13) SavedModel; the engine runs the
same chain in one enqueue (src/inference/hip_model.py) and returns raw logits.
"""
from src.inference import hip_model


class ModelGeneralV3(hip_model.HipModel):
    modelname = "model_general_v3"
    embeddername = 'yamnet_k2'
    digits_results = 2
