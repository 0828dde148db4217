"""A model plugin on the MI355X engine (reference contract: src/inference/models.py:12-37).

The reference's ``models/<name>/model.py`` chains ``embedder.embed`` and the model's own SavedModel; the engine runs the
same chain in one enqueue (front end, 14 conv layers, pooling, the model's dense stack) and returns what the stack's last
layer gives.  A trained model's plugin is a subclass with three class attributes beside its ``config_model.json``,
``saved_model.pb`` and ``variables/``:

    from src.inference import hip_model

    class ModelMine(hip_model.HipModel):
        modelname = "model_mine"
        embeddername = "yamnet_k2"
        digits_results = 2

(The module is imported, not the class: the loader takes the first BaseModel subclass it finds among the plugin module's
names, and an imported ``HipModel`` would be one.)
"""
import os

from src import config as cfg
from src.inference.models import BaseModel


class HipModel(BaseModel):
    def initialize(self):
        from buzzdetect_amd.engine import HipEngine
        engine_embedder = getattr(self.embedder, "engine_embedder", None)
        if engine_embedder is None:
            raise RuntimeError(f"embedder plugin '{self.embeddername}' is not backed by the HIP engine")
        # the embedder's weights come from beside the EMBEDDER plugin, where the reference's embedder.initialize() loads them;
        # the classifier from beside THIS plugin when its SavedModel is there (cfg.DIR_MODELS/<modelname>/variables), else by
        # buzzdetect_amd.weights.load_head's own lookup (the packaged model_general_v3 ships without a variables/ directory)
        beside = os.path.exists(os.path.join(cfg.DIR_MODELS, self.modelname, "variables", "variables.index"))
        self.model = HipEngine(embeddername=engine_embedder, modelname=self.modelname,
                               models_dir=os.path.abspath(cfg.DIR_MODELS) if beside else None,
                               variables_candidates=self.embedder.variables_candidates())
        self.embedder.attach(self.model)   # one set of weights serves embed() and predict()

    def predict(self, audiosamples):
        """1-D float32 audio at 16 kHz -> [n_windows, n_classes] (device-resident, has .numpy())."""
        return self.model.predict(audiosamples, self.embedder.framehop_s)
