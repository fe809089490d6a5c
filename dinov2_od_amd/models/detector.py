"""DINOv2ObjectDetector: host-side mirror of dino_detector/models/detector.py:8-69."""
import torch
import torch.nn as nn

from ..config import REF_DEFAULTS
from ..engine import check_train_precision, default_precision, split_detections
from .dinov2_backbone import DINOv2Backbone, _EngineMixin
from .detr_decoder import DETRDecoder


class DINOv2ObjectDetector(_EngineMixin, nn.Module):   # state-dict keys already carry "backbone." / "decoder."
    """Same constructor defaults as the reference (config.py:21-35 via detector.py:9-21).
    Extra keyword arguments: `pretrained`, `precision`, `backbone_config` (micro test models), `aux_loss` (train() outputs
    gain "aux_outputs": DETRDecoder), `train_precision` ("fp32" | "bf16x3": the linears of the native train() steps as bf16 split
    products on their fp32 operands; it acts on the native steps only -- the autograd composite stays fp32 -- and `precision` keeps
    governing eval() and the frozen prefix.  set_train_precision() changes it later)."""

    def __init__(self,
                 num_classes=REF_DEFAULTS["num_classes"],
                 dino_model_name=REF_DEFAULTS["dino_model_name"],
                 lora_r=REF_DEFAULTS["lora_r"],
                 lora_alpha=REF_DEFAULTS["lora_alpha"],
                 hidden_dim=REF_DEFAULTS["hidden_dim"],
                 num_queries=REF_DEFAULTS["num_queries"],
                 nheads=REF_DEFAULTS["nheads"],
                 num_decoder_layers=REF_DEFAULTS["num_decoder_layers"],
                 dim_feedforward=REF_DEFAULTS["dim_feedforward"],
                 dropout=REF_DEFAULTS["dropout"],
                 n_points=REF_DEFAULTS["n_points"],
                 use_deformable=REF_DEFAULTS["use_deformable"],
                 pretrained=True, precision=None, backbone_config=None, train_precision="fp32", aux_loss=False):
        super().__init__()
        self.train_precision = check_train_precision(train_precision)
        if hidden_dim is None:                                  # detector.py:25-35
            hidden_dim = 768
            for key, dim in (("small", 384), ("base", 768), ("large", 1024), ("giant", 1536)):
                if key in dino_model_name:
                    hidden_dim = dim
                    break
        precision = precision or default_precision()
        self.backbone = DINOv2Backbone(model_name=dino_model_name, lora_r=lora_r, lora_alpha=lora_alpha,
                                       target_dim=hidden_dim, pretrained=pretrained, precision=precision,
                                       config=backbone_config, train_precision=train_precision)
        self.decoder = DETRDecoder(num_queries=num_queries, hidden_dim=hidden_dim, nheads=nheads,
                                   num_decoder_layers=num_decoder_layers, num_classes=num_classes,
                                   dim_feedforward=dim_feedforward, dropout=dropout, n_points=n_points,
                                   use_deformable=use_deformable, precision=precision, aux_loss=aux_loss,
                                   train_precision=train_precision)
        self.precision = precision
        self._dropout_p = float(dropout)
        self._bb_cfg = self.backbone._bb_cfg
        self._dc_cfg = self.decoder._dc_cfg

    def enable_hipgraph(self, on=True):
        """eval-mode forwards replay one captured hipGraph per input shape (the returned tensors are the graph's static output
        buffer: consume or clone them before the next forward of the same shape)"""
        self._get_engine().use_graph = bool(on)
        return self

    def forward_packed(self, pixel_values):
        """[B,3,H,W] -> packed detections [B, Q, C+4] (logits | boxes): the buffer the multi-GPU
        all-gather moves (dinov2_od_amd.dist.gather_detections)."""
        if self._use_autograd(pixel_values):
            o = self.forward(pixel_values)
            return torch.cat([o["pred_logits"], o["pred_boxes"]], dim=-1)
        return self._get_engine().forward(pixel_values, self._engine_named())

    def forward_packed_u8(self, pixels_hwc):
        """eval-mode forward straight from the device input pipeline's bytes: uint8 [B, H, W, 3] as
        `preprocess_batch(images, size, as_uint8=True)` returns them (Resize done, ToTensor not yet: train.py:584-587) -> packed
        detections.  Identical, bit for bit, to forward_packed(preprocess_batch(images, size)); bf16 / bf16x3 / fp8 precision."""
        if self.training:
            raise RuntimeError("forward_packed_u8 is an eval-mode entry (train() takes the fp32 batch)")
        return self._get_engine().forward_u8(pixels_hwc, self._engine_named())

    def detect(self, pixel_values, sizes=None, **kw):
        """[B,3,H,W] -> postprocess.Detections: the top_k detections of every image as pixel xyxy boxes with score and label
        (postprocess.detect_packed takes **kw: top_k, threshold, nms_iou, class_agnostic, clamp, skip_background).  sizes: the
        (height, width) the boxes are scaled to -- None = the input's own (H, W).  Runs the eval-mode forward under no_grad and
        puts the model back into the mode it was in; no host sync."""
        from ..postprocess import detect_packed
        was_training = self.training
        self.eval()
        try:
            with torch.no_grad():
                det = self.forward_packed(pixel_values)
                if sizes is None:
                    sizes = (pixel_values.shape[-2], pixel_values.shape[-1])
                return detect_packed(det, self._dc_cfg.num_classes, sizes, **kw)
        finally:
            self.train(was_training)

    def _token_grid(self, pixel_values):
        p = self._bb_cfg.patch
        return pixel_values.shape[-2] // p, pixel_values.shape[-1] // p

    def detect_embed(self, pixel_values, sizes=None, grid=4, **kw):
        """`detect` plus one appearance vector per detection: (postprocess.Detections, embeddings [B, K, D] fp32).  One forward
        (Engine.forward_mem: the same detections, and the backbone tokens it computed anyway), postprocess.detect_packed with **kw, then
        reid.roi_embed pools the tokens under the detections' own boxes, in the detections' own pixel frame, from grid x grid samples:
        unit vectors, zeros for padding rows.  No host sync."""
        from ..postprocess import detect_packed
        from ..reid import roi_embed
        was_training = self.training
        self.eval()
        try:
            with torch.no_grad():
                det, mem = self._get_engine().forward_mem(pixel_values, self._engine_named())
                if sizes is None:
                    sizes = (pixel_values.shape[-2], pixel_values.shape[-1])
                out = detect_packed(det, self._dc_cfg.num_classes, sizes, **kw)
                return out, roi_embed(mem, out.boxes, out.counts, sizes, grid, 1, self._token_grid(pixel_values))
        finally:
            self.train(was_training)

    def embed(self, pixel_values, boxes, counts=None, sizes=None, grid=4):
        """[B,3,H,W] and caller-supplied boxes [B, K, 4] fp32 xyxy (pixels of `sizes`: (height, width), None = the input's own; counts
        [B] int32 or None = every row) -> [B, K, D] fp32 unit vectors pooled from the backbone tokens (reid.roi_embed): the building
        block for retrieval and few-shot labelling on this backbone.  Eval-mode forward under no_grad; no host sync."""
        from ..reid import roi_embed
        was_training = self.training
        self.eval()
        try:
            with torch.no_grad():
                _, mem = self._get_engine().forward_mem(pixel_values, self._engine_named())
                if sizes is None:
                    sizes = (pixel_values.shape[-2], pixel_values.shape[-1])
                return roi_embed(mem, boxes, counts, sizes, grid, 1, self._token_grid(pixel_values))
        finally:
            self.train(was_training)

    def track(self, pixel_values, tracker, sizes=None, grid=4, **kw):
        """`detect(pixel_values, sizes, **kw)` followed by `tracker.update`: image b of the batch is the next frame of the tracker's
        stream b (tracking.Tracker with num_streams = the batch size).  Returns tracking.TrackedDetections: the Detections plus the track
        id and the filtered box of every row.  With a Tracker(appearance=True) it is `detect_embed(pixel_values, sizes, grid, **kw)`
        followed by `tracker.update(detections, embeddings)`.  No host sync."""
        if getattr(tracker, "appearance", False):
            return tracker.update(*self.detect_embed(pixel_values, sizes, grid, **kw))
        return tracker.update(self.detect(pixel_values, sizes, **kw))

    def detect_sliced(self, images, size=None, tile=None, overlap=0.2, full_view=True, flip=False, max_batch=64, **kw):
        """raw uint8 RGB images [H_i, W_i, 3] (as `preprocess_batch` takes them) -> slicing.SlicedDetections in each image's own
        pixels: the model runs on the whole image (full_view), on overlapping tiles of `tile` source pixels a side (slicing.plan_views;
        None = `size`) and with `flip` on their mirrored copies, every view resized to `size` (None = 224 x 224), and the answers are
        merged by one dod_detect_views launch (slicing.detect_views_packed takes **kw: top_k, threshold, nms_iou, nms_metric,
        class_agnostic, clamp, edge_margin, skip_background, and merge="fuse" with fuse_conf for weighted boxes fusion by one
        dod_fuse_views launch instead, which returns slicing.FusedDetections).  The views go through forward_packed_u8 in chunks of at most max_batch.
        Runs the eval-mode forward under no_grad and puts the model back into the mode it was in; no host sync after staging."""
        from ..slicing import detect_sliced
        was_training = self.training
        self.eval()
        try:
            with torch.no_grad():
                return detect_sliced(self, images, size, tile, overlap, full_view, flip, max_batch, **kw)
        finally:
            self.train(was_training)

    def forward(self, pixel_values):
        """pixel_values [batch, 3, H, W] -> {"pred_logits", "pred_boxes"} (detector.py:58-69)."""
        if self._use_autograd(pixel_values):            # train(): autograd composite of the same math (detector.py:58-69)
            return self.decoder(self.backbone(pixel_values))
        return split_detections(self.forward_packed(pixel_values), self._dc_cfg.num_classes)
