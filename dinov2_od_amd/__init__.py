"""MI355X-native forward path of dino_detector (DINOv2 ViT backbone + DETR-style head).

`from dinov2_od_amd import DINOv2ObjectDetector` mirrors `from dino_detector import DINOv2ObjectDetector`
(dino_detector/__init__.py:2).  Importing the package does not load the HIP library; the first
forward does, and fails loudly if it is missing.
"""
__version__ = "0.1.0"


def __getattr__(name):
    if name in ("DINOv2ObjectDetector", "DINOv2Backbone", "DETRDecoder"):
        from . import models
        return getattr(models, name)
    if name == "optim":      # dinov2_od_amd.optim.Adam / AdamW / ModelEMA / clip_grad_norm_: the optimizer step on the HIP kernels
        import importlib
        return importlib.import_module(".optim", __name__)
    if name in ("draw_detections", "log_images", "save_images"):      # dinov2_od_amd.visualize: boxes drawn into the batch on the GPU
        import importlib
        return getattr(importlib.import_module(".visualize", __name__), name)
    if name in ("Tracker", "TrackedDetections"):      # dinov2_od_amd.tracking: ByteTrack association on the GPU behind detect
        import importlib
        return getattr(importlib.import_module(".tracking", __name__), name)
    raise AttributeError(name)
