"""Multi-object tracking on the GPU: the host side of `dod_track_update` (include/dinodet.h).

`model.detect` answers every frame in isolation; a caller with a camera wants the same object to keep the same number from frame to
frame.  `Tracker` is ByteTrack's association (Kalman prediction, a high-score pass, a low-score rescue pass, tentative tracks, lost
tracks with a time-out) behind `detect`, for any number of independent streams, in one launch per frame and without a host sync: the
track table stays on the device.

    tracker = Tracker(num_streams=B, max_tracks=128)
    for frames in video:                                        # [B, 3, H, W]
        t = model.track(frames, tracker, top_k=100, threshold=0.1)      # detect + tracker.update -> TrackedDetections
        canvas = draw_detections(frames_u8, t.by_id())          # coloured and captioned by track id

Geometry alone swaps ids when two objects cross or one stops while another passes.  `Tracker(appearance=True)` also keeps a smoothed
embedding per track on the device and fuses appearance into the first and the tentative association the way BoT-SORT does
(dod_track_update_app): the embeddings are `model.detect_embed`'s, pooled from the backbone tokens the forward computed anyway
(reid.roi_embed), and `model.track` passes them on by itself.  Still no host sync.

The header states the semantics and tests/track_cases.py restates them in numpy + scipy; the kernel's result equals that restatement
bit for bit.  No CPU fallback: without the HIP library and a GPU this module raises.
"""
import ctypes as C
import math

import torch

from . import _native as nat
from .postprocess import Detections, MAX_TOP_K

MAX_TRACKS = 512                       # include/dinodet.h dod_track_update: slots per stream
MAX_STREAMS = 65535
MAX_EMBED_DIM = 2048                   # dod_track_embed_dots: channels of an embedding (a multiple of 4)
FREE, TENTATIVE, TRACKED, LOST = 0, 1, 2, 3       # slot states, as `tracks()["state"]` holds them
_THRESHOLDS = ("track_thresh", "low_thresh", "new_thresh", "match_thresh", "second_thresh", "tentative_thresh")


class TrackedDetections(Detections):
    """postprocess.Detections (scores, labels, boxes, queries, counts: the tensors `update` was given, not copies) with two more
    tensors: `ids` [S, K] int32, the track id of every row (-1 where the row is untracked or padding), and `track_boxes` [S, K, 4] fp32,
    the track's filtered box as pixel xyxy (0 where the id is -1).  It is a Detections: detections_to_list and draw_detections take it."""

    def __new__(cls, scores, labels, boxes, queries, counts, ids, track_boxes):
        self = super().__new__(cls, scores, labels, boxes, queries, counts)
        self.ids = ids
        self.track_boxes = track_boxes
        return self

    def by_id(self):
        """a plain Detections whose labels are the track ids and whose rows with id -1 are blanked as padding rows are (score 0, label
        -1, query -1, box 0): draw_detections(images, t.by_id()) colours and captions by track.  No host sync."""
        on = self.ids >= 0
        zero = torch.zeros((), dtype=self.scores.dtype, device=self.scores.device)
        return Detections(torch.where(on, self.scores, zero), self.ids, torch.where(on[..., None], self.boxes, zero),
                          torch.where(on, self.queries, self.ids), self.counts)      # where not `on` the id is the -1 a padding row's query holds


class Tracker:
    """ByteTrack association for `num_streams` independent streams of at most `max_tracks` (1..512) simultaneous tracks each.  The
    defaults are ByteTrack's.  `update` takes the Detections of one frame of every stream (row s = stream s) and returns them with track
    ids; `reset` forgets the tracks of all or some streams; `tracks` returns the table; `check` is the one call that syncs.
    fuse_score: the first and the tentative pass use 1 - iou * score as cost instead of 1 - iou.  class_aware: a track is only matched
    to rows of its own label.  device: where the table lives (None: the device of the first update's detections).
    appearance: `update` also takes one unit vector per row (reid.roi_embed) and the first and the tentative pass use
    min(that cost, d_app) with d_app = 0.5 * (1 - <track embedding, row embedding>), counted as 1 where it exceeds appearance_thresh or
    where 1 - iou exceeds proximity_thresh (BoT-SORT's gates and defaults); a track's embedding is the one it was born with, blended
    with every first- or tentative-pass hit as E = normalise(momentum * E + (1 - momentum) * e).  Without it nothing new is allocated."""

    def __init__(self, num_streams=1, max_tracks=128, track_thresh=0.5, low_thresh=0.1, new_thresh=0.6, match_thresh=0.8,
                 second_thresh=0.5, tentative_thresh=0.7, max_age=30, fuse_score=True, class_aware=False, device=None,
                 appearance=False, appearance_thresh=0.25, proximity_thresh=0.5, momentum=0.9):
        S, T = int(num_streams), int(max_tracks)
        if not 1 <= S <= MAX_STREAMS:
            raise ValueError(f"num_streams must be in 1..{MAX_STREAMS}, got {num_streams}")
        if not 1 <= T <= MAX_TRACKS:
            raise ValueError(f"max_tracks must be in 1..{MAX_TRACKS}, got {max_tracks}")
        p = nat.DodTrackParams()
        for name, v in zip(_THRESHOLDS, (track_thresh, low_thresh, new_thresh, match_thresh, second_thresh, tentative_thresh)):
            v = float(v)
            if math.isnan(v):
                raise ValueError(f"{name} must be a number, got NaN")
            setattr(p, name, v)
        if float(low_thresh) > float(track_thresh):
            raise ValueError(f"low_thresh must not exceed track_thresh, got {low_thresh} > {track_thresh}")
        if int(max_age) != max_age or int(max_age) < 0:
            raise ValueError(f"max_age must be a non-negative integer, got {max_age}")
        p.max_age, p.fuse_score, p.class_aware = int(max_age), int(bool(fuse_score)), int(bool(class_aware))
        self.num_streams, self.max_tracks, self.params = S, T, p
        self.appearance = bool(appearance)
        self.app_params = None
        if self.appearance:
            q = nat.DodTrackAppParams()
            for name, v in (("appearance_thresh", appearance_thresh), ("proximity_thresh", proximity_thresh), ("momentum", momentum)):
                v = float(v)
                if math.isnan(v):
                    raise ValueError(f"{name} must be a number, got NaN")
                setattr(q, name, v)
            if not 0.0 <= float(momentum) <= 1.0:
                raise ValueError(f"momentum must lie in [0, 1], got {momentum}")
            self.app_params = q
        self._emb = None                                         # slot_emb [S, T, D], allocated by the first update of an appearance tracker
        self.device = None if device is None else torch.device(device)
        self._state = self._ws = None

    # ---- device side -----------------------------------------------------------------------------------------------------------
    def _ensure(self, device):
        if self._state is None:
            dev = self.device or device
            if dev is None or torch.device(dev).type != "cuda":
                raise ValueError("the tracker lives on the GPU (there is no CPU fallback)")
            self.device = torch.device(dev)
            L = nat.lib()
            self._state = torch.empty(L.dod_track_state_bytes(self.num_streams, self.max_tracks), dtype=torch.uint8, device=self.device)
            nat.check(L.dod_track_reset(nat.ptr(self._state), self.num_streams, self.max_tracks, None, nat.stream_ptr()))
        return self._state

    def _check_streams(self, streams):
        if streams is None:
            return None
        idx = [int(s) for s in streams]
        if any(not 0 <= s < self.num_streams for s in idx):
            raise ValueError(f"streams must lie in 0..{self.num_streams - 1}, got {list(streams)}")
        return idx

    def reset(self, streams=None):
        """forget every track of the given streams (None: all): their slots are FREE, the next id is 1 and the frame count 0 again"""
        idx = self._check_streams(streams)
        if self._state is None and self.device is None:
            return                                               # nothing on a device yet: the first update starts from a reset table
        state = self._ensure(None)
        mask = None
        if idx is not None:
            m = torch.zeros(self.num_streams, dtype=torch.int32)
            m[idx] = 1
            mask = m.to(self.device)
        with torch.cuda.device(self.device):
            nat.check(nat.lib().dod_track_reset(nat.ptr(state), self.num_streams, self.max_tracks, nat.ptr(mask), nat.stream_ptr()))
            if self._emb is not None:
                if idx is None:
                    self._emb.zero_()
                else:
                    self._emb[torch.tensor(idx, dtype=torch.int64).to(self.device)] = 0.0

    def embeddings(self):
        """slot_emb [S, T, D] fp32: the smoothed unit embedding of every slot (the tensor itself; a FREE slot's row is stale), or None
        before the first update of an appearance tracker"""
        if not self.appearance:
            raise ValueError("this tracker keeps no embeddings (appearance=False)")
        return self._emb

    def update(self, detections, embeddings=None):
        """detections: a postprocess.Detections (or SlicedDetections / FusedDetections) of one frame per stream: scores [S, K] fp32,
        labels [S, K] int32, boxes [S, K, 4] fp32 pixel xyxy, counts [S] int32, K <= 1024.  Returns TrackedDetections on the same
        tensors plus ids and track_boxes.  One launch on the current stream, no host sync.  An appearance tracker takes
        embeddings [S, K, D] fp32 (one unit vector per row, D a multiple of 4 up to 2048: reid.roi_embed) as well -- three launches:
        similarities, association, the tracks' embeddings -- and a tracker without appearance takes none."""
        S, T = self.num_streams, self.max_tracks
        try:
            scores, labels, boxes, queries, counts = (detections.scores, detections.labels, detections.boxes, detections.queries,
                                                      detections.counts)
        except AttributeError:
            raise ValueError("update takes a postprocess.Detections (scores, labels, boxes, queries, counts)") from None
        for name, t, dt in (("scores", scores, torch.float32), ("labels", labels, torch.int32), ("boxes", boxes, torch.float32),
                            ("counts", counts, torch.int32)):
            if not (isinstance(t, torch.Tensor) and t.dtype == dt):
                raise ValueError(f"detections.{name} must be a {dt} tensor")
        if scores.dim() != 2 or scores.shape[0] != S:
            raise ValueError(f"detections must hold one row block per stream ({S}), got scores {tuple(scores.shape)}")
        K = int(scores.shape[1])
        if not 1 <= K <= MAX_TOP_K:
            raise ValueError(f"detections must hold 1..{MAX_TOP_K} rows per stream, got {K}")
        if tuple(labels.shape) != (S, K) or tuple(boxes.shape) != (S, K, 4) or tuple(counts.shape) != (S,):
            raise ValueError(f"detections must hold labels [{S}, {K}], boxes [{S}, {K}, 4] and counts [{S}], got {tuple(labels.shape)}, "
                             f"{tuple(boxes.shape)} and {tuple(counts.shape)}")
        if self.appearance != (embeddings is not None):
            raise ValueError("update takes embeddings exactly when the tracker was made with appearance=True")
        if self.appearance:
            e = embeddings
            if not (isinstance(e, torch.Tensor) and e.dtype == torch.float32 and e.dim() == 3 and tuple(e.shape[:2]) == (S, K)):
                raise ValueError(f"embeddings must be a fp32 tensor [{S}, {K}, D]")
            D = int(e.shape[2])
            if not 4 <= D <= MAX_EMBED_DIM or D % 4:
                raise ValueError(f"embeddings must hold 4..{MAX_EMBED_DIM} channels, a multiple of 4, got {D}")
            if self._emb is not None and self._emb.shape[2] != D:
                raise ValueError(f"embeddings have {D} channels, the tracks' {self._emb.shape[2]}")
            if not e.is_cuda:
                raise ValueError("embeddings must be on the GPU (there is no CPU fallback)")
        if not (scores.is_cuda and labels.is_cuda and boxes.is_cuda and counts.is_cuda):      # last: every argument is checked whether or not a GPU is present
            raise ValueError("detections must be on the GPU (there is no CPU fallback)")
        state = self._ensure(scores.device)
        if scores.device != self.device:
            raise ValueError(f"the tracker lives on {self.device}, the detections on {scores.device}")
        L = nat.lib()
        sc, lb, bx, ct = scores.contiguous(), labels.contiguous(), boxes.contiguous(), counts.contiguous()
        with torch.cuda.device(self.device):
            if self._ws is None or self._ws[0] != K:
                self._ws = (K, torch.empty(L.dod_track_workspace_bytes(S, T, K), dtype=torch.uint8, device=self.device))
            ws = self._ws[1]
            ids = torch.empty(S, K, dtype=torch.int32, device=self.device)
            tb = torch.empty(S, K, 4, dtype=torch.float32, device=self.device)
            if self.appearance:
                if embeddings.device != self.device:
                    raise ValueError(f"the tracker lives on {self.device}, the embeddings on {embeddings.device}")
                em = embeddings.contiguous()
                if self._emb is None:
                    self._emb = torch.zeros(S, T, D, dtype=torch.float32, device=self.device)
                dots = torch.empty(S, T, K, dtype=torch.float32, device=self.device)
                assoc = torch.empty(S, K, dtype=torch.int32, device=self.device)
                nat.check(L.dod_track_embed_dots(nat.ptr(self._emb), nat.ptr(em), S, T, K, D, nat.ptr(dots), nat.stream_ptr()))
                nat.check(L.dod_track_update_app(nat.ptr(state), S, T, nat.ptr(sc), nat.ptr(lb), nat.ptr(bx), nat.ptr(ct), K, C.byref(self.params),
                                                 C.byref(self.app_params), nat.ptr(dots), nat.ptr(ids), nat.ptr(tb), nat.ptr(assoc), nat.ptr(ws),
                                                 ws.numel(), nat.stream_ptr()))
                nat.check(L.dod_track_embed_commit(nat.ptr(self._emb), nat.ptr(em), nat.ptr(assoc), S, T, K, D, self.app_params.momentum,
                                                   nat.stream_ptr()))
                return TrackedDetections(scores, labels, boxes, queries, counts, ids, tb)
            nat.check(L.dod_track_update(nat.ptr(state), S, T, nat.ptr(sc), nat.ptr(lb), nat.ptr(bx), nat.ptr(ct), K, C.byref(self.params),
                                         nat.ptr(ids), nat.ptr(tb), nat.ptr(ws), ws.numel(), nat.stream_ptr()))
        return TrackedDetections(scores, labels, boxes, queries, counts, ids, tb)

    def tracks(self):
        """the table as CUDA tensors (dod_track_export): mean fp64 [S, T, 8] (cx, cy, aspect, height and their velocities), cov fp64
        [S, T, 12] ((variance, covariance, velocity variance) of each of the four), state / id / label / last_frame int32 [S, T], score
        fp32 [S, T], frame / next_id / overflow int32 [S].  A FREE slot's other fields are stale.  No host sync."""
        state = self._ensure(None)
        S, T, dev = self.num_streams, self.max_tracks, self.device
        out = dict(mean=torch.empty(S, T, 8, dtype=torch.float64, device=dev), cov=torch.empty(S, T, 12, dtype=torch.float64, device=dev))
        for k in ("state", "id", "label", "last_frame"):
            out[k] = torch.empty(S, T, dtype=torch.int32, device=dev)
        out["score"] = torch.empty(S, T, dtype=torch.float32, device=dev)
        for k in ("frame", "next_id", "overflow"):
            out[k] = torch.empty(S, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            nat.check(nat.lib().dod_track_export(nat.ptr(state), S, T, *(nat.ptr(out[k]) for k in (
                "mean", "cov", "state", "id", "label", "last_frame", "score", "frame", "next_id", "overflow")), nat.stream_ptr()))
        return out

    def check(self, strict=False):
        """the one sync: returns how many births every stream has dropped for want of a free slot since its last reset (a list of
        num_streams ints); with strict raises RuntimeError when any were dropped"""
        if self._state is None:
            return [0] * self.num_streams
        over = self.tracks()["overflow"].tolist()
        if strict and any(over):
            raise RuntimeError(f"tracker overflow: births dropped per stream {over} (max_tracks = {self.max_tracks})")
        return over
