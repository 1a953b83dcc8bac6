"""Edge-module configuration = IoT Edge module twin desired properties (SURVEY.md §5.6 layer 4).

The reference's config layers are Helm values -> cloud-init -> config.toml; the module
layer (IoT Hub deployment manifest + twin) is where the reference's demo module
(SimulatedTemperatureSensor) takes its settings.  kvedge keeps that shape: the twin's
desired properties below drive the GPU inference module, and the same keys exist as
CLI flags for bare-metal runs (kvedge_amd.module.__main__).
"""
from __future__ import annotations

import json
from dataclasses import asdict, dataclass, fields, replace
from typing import Any, Dict, Tuple

MODELS = ("resnet50", "yolov8n", "detect-classify", "simulated-temperature")
SOURCES = ("synthetic", "camera", "camera-nv12")
DTYPES = ("bf16",)
ZONE_ANCHORS = ("bottom", "centre")
MAX_REGIONS = 8  # lines, and zones, per camera (csrc/kernels/zones.hip)
SNAPSHOT_SUBSAMPLINGS = ("420", "444")
SNAPSHOT_LABELS = ("none", "class", "id", "both")
MAX_PRIVACY = 8  # privacy classes, and privacy zones, per camera (csrc/kernels/annotate.hip)


def _point(p, what: str):
    if not isinstance(p, (list, tuple)) or len(p) != 2:
        raise ValueError(f"{what} must be [x, y], got {p!r}")
    return [float(p[0]), float(p[1])]


def _regions(v, kind: str) -> Tuple[Dict[str, Any], ...]:
    """The ``lines`` / ``zones`` twin key (a list of objects, or the same as a JSON string) in
    normal form: name, class (-1 = any), cameras (None = all) and the geometry as floats."""
    if isinstance(v, str):
        v = json.loads(v) if v.strip() else []
    if v is None:
        v = []
    if not isinstance(v, (list, tuple)):
        raise ValueError(f"{kind} must be a list, got {type(v).__name__}")
    out = []
    for i, r in enumerate(v):
        if not isinstance(r, dict):
            raise ValueError(f"{kind}[{i}] must be an object, got {r!r}")
        unknown = set(r) - ({"name", "class", "cameras"} |
                            ({"a", "b"} if kind == "lines" else {"polygon"}))
        if unknown:
            raise ValueError(f"{kind}[{i}]: unknown keys {sorted(unknown)}")
        name = str(r.get("name", ""))
        if not name:
            raise ValueError(f"{kind}[{i}] needs a name")
        cams = r.get("cameras")
        if cams is not None:
            if not isinstance(cams, (list, tuple)):
                raise ValueError(f"{kind}[{i}].cameras must be a list of camera indices")
            cams = [int(c) for c in cams]
        n = {"name": name, "class": int(r.get("class", -1)), "cameras": cams}
        if kind == "lines":
            n["a"] = _point(r.get("a"), f"{kind}[{i}].a")
            n["b"] = _point(r.get("b"), f"{kind}[{i}].b")
        else:
            poly = r.get("polygon")
            if not isinstance(poly, (list, tuple)):
                raise ValueError(f"{kind}[{i}].polygon must be a list of [x, y]")
            n["polygon"] = [_point(p, f"{kind}[{i}].polygon[{j}]") for j, p in enumerate(poly)]
        out.append(n)
    return tuple(out)


def _privacy_zones(v) -> Tuple[Dict[str, Any], ...]:
    """The ``snapshot_privacy_zones`` twin key, shaped like ``zones`` without a class: name,
    polygon, cameras (None = all), in normal form."""
    if isinstance(v, str):
        v = json.loads(v) if v.strip() else []
    if isinstance(v, (list, tuple)):
        for i, r in enumerate(v):
            if isinstance(r, dict) and "class" in r:
                raise ValueError(f"snapshot_privacy_zones[{i}]: unknown keys ['class']")
    return tuple({k: r[k] for k in ("name", "cameras", "polygon")}
                 for r in _regions(v, "snapshot_privacy_zones"))


def _int_tuple(v, what: str) -> Tuple[int, ...]:
    """A list of integers, or the same as "0,2" / JSON text."""
    if isinstance(v, str):
        v = [p for p in v.replace("[", " ").replace("]", " ").replace(",", " ").split()]
    if v is None:
        v = []
    if isinstance(v, bool) or not isinstance(v, (list, tuple)):
        raise ValueError(f"{what} must be a list of integers, got {v!r}")
    try:
        out = tuple(int(c) for c in v)
    except (TypeError, ValueError):
        raise ValueError(f"{what} must be a list of integers, got {v!r}") from None
    if any(isinstance(c, (bool, float)) and int(c) != c for c in v):
        raise ValueError(f"{what} must be a list of integers, got {v!r}")
    return out


@dataclass(frozen=True)
class ModuleConfig:
    model: str = "resnet50"
    batch: int = 64
    dtype: str = "bf16"
    seed: int = 0
    report_interval_s: float = 10.0
    world_size: int = 1
    image_size: int = 0          # 0 = model default (224 / 640)
    conf: float = 0.25           # YOLO score threshold
    iou: float = 0.7             # YOLO NMS IoU threshold
    max_det: int = 300
    fps: float = 0.0             # 0 = run flat out; > 0 throttles batches/s*batch
    use_graph: bool = True
    # frame source: "synthetic" = on-device generator inside the graph; "camera" = a host
    # producer thread feeding a pinned FrameRing that the native serve loop DMAs from;
    # "camera-nv12" = the same with NV12 frames [Hs * 3 / 2, Ws] as capture devices and video
    # decoders deliver them (1.5 bytes per pixel through the ring and over PCIe instead of 3;
    # the colour conversion happens inside the on-device resample).  It needs frame_height /
    # frame_width (for model-size frames, set them to the model size)
    source: str = "synthetic"
    # native resolution of the incoming frames (e.g. 1080 x 1920); the engine resamples them
    # to the model size on the device (YOLO: letterbox, ResNet: resize + centre-crop) and
    # YOLO boxes are reported in frame pixels.  0 / 0 = frames arrive at model size
    frame_height: int = 0
    frame_width: int = 0
    # model "detect-classify": the top crops_per_image boxes of every frame are cut out on the
    # device and classified (ResNet-50 at 224); the classifier runs batch * crops_per_image
    # images per step whatever the detection counts are
    crops_per_image: int = 4
    # multi-object tracking (models "yolov8n" / "detect-classify"): ONE BATCH ROW = ONE CAMERA
    # -- row n of every batch is the next frame of camera n, so the module serves `batch`
    # cameras, one frame each per step -- and every detection gets the id of the track it
    # continues (on-device IoU tracker, ops.track_update).  track_iou: association gate;
    # track_max_age: frames a lost track coasts before it is dropped; track_min_hits:
    # consecutive matches before a track gets its id; track_max_tracks: slots per camera
    track: bool = False
    track_iou: float = 0.3
    track_max_age: int = 30
    track_min_hits: int = 3
    track_max_tracks: int = 64
    # virtual lines and polygon zones on the tracked boxes (they need `track`), counted on the
    # device (ops.zone_update): up to 8 of each per camera, in the pixel frame the boxes are
    # reported in.  lines: [{name, a: [x, y], b: [x, y], class?, cameras?}]; zones: [{name,
    # polygon: [[x, y], ...] (3..8 vertices), class?, cameras?}]; class: only that class counts
    # (default -1, any); cameras: batch rows the region applies to (default all).
    # zone_anchor: the point of a box that is tested, "bottom" (bottom-centre) or "centre"
    lines: Tuple[Dict[str, Any], ...] = ()
    zones: Tuple[Dict[str, Any], ...] = ()
    zone_anchor: str = "bottom"
    # per-camera frame watch (ops.frame_watch): one more streaming pass over the incoming
    # frames, one batch row = one camera.  A motion grid of watch_cell-pixel cells against a
    # running background (background = mean of about 2^watch_bg_shift frames; every
    # watch_row_step-th row is read) and five conditions -- motion / scene (watch_motion_share /
    # watch_scene_share of the cells moved by more than watch_motion_level luma levels), dark
    # (mean luma below watch_dark_level), flat (mean neighbour difference below
    # watch_flat_level: covered, defocused, fogged), frozen (the frame repeats) -- each an
    # alarm once it has held for watch_hold frames
    watch: bool = False
    watch_cell: int = 16
    watch_row_step: int = 1
    watch_bg_shift: int = 4
    watch_motion_level: float = 10.0
    watch_motion_share: float = 0.01
    watch_scene_share: float = 0.5
    watch_dark_level: float = 24.0
    watch_flat_level: float = 1.5
    watch_hold: int = 8
    # camera snapshots (ops.jpeg_encode): every step each camera's current frame is resized on
    # the device to snapshot_width pixels wide (the height follows the frame's shape) and
    # encoded as a baseline JPEG of snapshot_subsampling ("420" / "444") at snapshot_quality.
    # A picture leaves on output `snapshots` when one of the camera's watch alarms is raised
    # and, with snapshot_every_s > 0, every snapshot_every_s seconds; one above
    # snapshot_max_bytes is counted as oversize and not sent.  Direct method `snapshot`
    # returns a camera's last picture
    snapshots: bool = False
    snapshot_width: int = 320
    snapshot_subsampling: str = "420"
    snapshot_quality: int = 75
    snapshot_every_s: float = 0.0
    snapshot_max_bytes: int = 131072
    # snapshot_annotate: what the device knows is drawn into each picture before it is encoded
    # (ops.annotate) -- with a detector the boxes (snapshot_boxes, outlines of
    # snapshot_box_thickness 1..4 pixels) and their labels (snapshot_labels "class" / "id" /
    # "both" = cls:id / "none", glyphs at snapshot_label_scale 1..2); boxes of
    # snapshot_privacy_classes (at most 8 class ids) and the polygons snapshot_privacy_zones
    # ([{name, polygon: [[x, y], ...] (3..8 vertices), cameras?}], at most 8, in the pixel frame
    # the boxes are reported in) are hidden under a mosaic of snapshot_privacy_block (4 / 8 /
    # 16) thumbnail pixels.  Only snapshot_annotate needs a rebuild: the others are read on
    # the device at every step
    snapshot_annotate: bool = False
    snapshot_boxes: bool = True
    snapshot_labels: str = "both"
    snapshot_box_thickness: int = 1
    snapshot_label_scale: int = 1
    snapshot_privacy_classes: Tuple[int, ...] = ()
    snapshot_privacy_block: int = 8
    snapshot_privacy_zones: Tuple[Dict[str, Any], ...] = ()
    native_loop: bool = True    # GPU: replay the graph from the C++ serve loop
    steps_per_poll: int = 1      # graph replays per module step (native loop)
    # seconds of in-graph tile refinement when the engine is built (engine.prepare refine_s;
    # 0 = off, the default).  It times runner-up tiles inside the captured step; on the
    # driver's fresh boxes it returned -0.5 .. +0.1 % (BENCH_r05 / r6 builder boxes) for
    # 3.1 s of a 6.6 s cold start, so it is opt-in
    refine_s: float = 0.0
    # multi-replica lockstep: module steps between control boundaries (0 = auto: every
    # step at world 1, 16 otherwise).  Twin patches, collective direct methods, report
    # decisions and stop requests are exchanged ONLY at these boundaries, so every rank
    # issues the same collectives in the same order.  Rank 0's value wins fleet-wide.
    sync_every: int = 0
    # SimulatedTemperatureSensor compatibility (BASELINE config 1, CPU-only plumbing)
    send_interval_s: float = 5.0
    max_messages: int = 500

    # keys that force an engine rebuild when they change
    REBUILD = ("model", "batch", "dtype", "seed", "image_size", "conf", "iou", "max_det",
               "use_graph", "source", "frame_height", "frame_width", "crops_per_image",
               "track", "track_iou", "track_max_age", "track_min_hits", "track_max_tracks",
               "lines", "zones", "zone_anchor", "watch", "watch_cell", "watch_row_step",
               "watch_bg_shift", "snapshots", "snapshot_width", "snapshot_subsampling",
               "snapshot_annotate")

    def __post_init__(self):
        for kind in ("lines", "zones"):  # lists as given (or JSON text) -> normal form
            object.__setattr__(self, kind, _regions(getattr(self, kind), kind))
        object.__setattr__(self, "snapshot_privacy_zones",
                           _privacy_zones(self.snapshot_privacy_zones))
        object.__setattr__(self, "snapshot_privacy_classes",
                           _int_tuple(self.snapshot_privacy_classes, "snapshot_privacy_classes"))

    def validate(self) -> "ModuleConfig":
        if self.model not in MODELS:
            raise ValueError(f"model must be one of {MODELS}, got {self.model!r}")
        if self.dtype not in DTYPES:
            raise ValueError(f"dtype must be one of {DTYPES} (bf16 compute), got {self.dtype!r}")
        if not 1 <= self.batch <= 4096:
            raise ValueError(f"batch out of range: {self.batch}")
        if self.report_interval_s <= 0:
            raise ValueError("report_interval_s must be > 0")
        if not 1 <= self.world_size <= 64:
            raise ValueError("world_size must be 1..64")
        if self.image_size and self.image_size % 32:
            raise ValueError("image_size must be a multiple of 32")
        if not 0.0 <= self.conf <= 1.0 or not 0.0 <= self.iou <= 1.0:
            raise ValueError("conf/iou must be in [0, 1]")
        if not 1 <= self.max_det <= 300:
            raise ValueError("max_det must be 1..300")
        if self.source not in SOURCES:
            raise ValueError(f"source must be one of {SOURCES}, got {self.source!r}")
        if bool(self.frame_height) != bool(self.frame_width):
            raise ValueError("frame_height and frame_width must be set together (0/0 = model size)")
        if self.frame_height:
            if not (16 <= self.frame_height <= 4096 and 16 <= self.frame_width <= 4096):
                raise ValueError("frame_height / frame_width must be 16..4096")
            if self.frame_width % 8:
                raise ValueError("frame_width must be a multiple of 8")
        if self.source == "camera-nv12":
            if not self.frame_height:
                raise ValueError("source camera-nv12 needs frame_height and frame_width (for "
                                 "frames at model size, set them to the model size)")
            if self.frame_height % 2:
                raise ValueError("source camera-nv12 needs an even frame_height")
        if not 1 <= self.crops_per_image <= 16:
            raise ValueError("crops_per_image must be 1..16")
        if self.model == "detect-classify":  # cross-key limits bind the cascade only
            if self.crops_per_image > self.max_det:
                raise ValueError("crops_per_image must be <= max_det")
            if self.batch * self.crops_per_image > 4096:
                raise ValueError("batch * crops_per_image must be <= 4096")
        # the tracker launcher's ranges (csrc/kernels/track.hip); the gate is kept in 1/1024
        if not 1 <= int(self.track_iou * 1024 + 0.5) <= 1024:
            raise ValueError("track_iou must be in (0, 1] (at least 1/2048)")
        if not 0 <= self.track_max_age <= 255:
            raise ValueError("track_max_age must be 0..255")
        if not 1 <= self.track_min_hits <= 255:
            raise ValueError("track_min_hits must be 1..255")
        if self.track_max_tracks not in (64, 128, 192, 256):
            raise ValueError("track_max_tracks must be 64, 128, 192 or 256")
        if self.track and self.model not in ("yolov8n", "detect-classify"):  # binds only when on
            raise ValueError("track needs a detector: model yolov8n or detect-classify")
        if self.zone_anchor not in ZONE_ANCHORS:
            raise ValueError(f"zone_anchor must be one of {ZONE_ANCHORS}, got {self.zone_anchor!r}")
        for kind in ("lines", "zones"):
            regions = getattr(self, kind)
            if len(regions) > MAX_REGIONS:
                raise ValueError(f"at most {MAX_REGIONS} {kind}, got {len(regions)}")
            names = [r["name"] for r in regions]
            if len(set(names)) != len(names):
                raise ValueError(f"{kind} names must be unique, got {names}")
            for r in regions:
                if not -1 <= r["class"] <= 65535:
                    raise ValueError(f"{kind} {r['name']!r}: class must be -1..65535")
                if r["cameras"] is not None and not all(0 <= c < self.batch for c in r["cameras"]):
                    raise ValueError(f"{kind} {r['name']!r}: cameras must be 0..batch - 1")
                if kind == "zones" and not 3 <= len(r["polygon"]) <= 8:
                    raise ValueError(f"zone {r['name']!r} needs 3..8 vertices, got "
                                     f"{len(r['polygon'])}")
        if (self.lines or self.zones) and not self.track:
            raise ValueError("lines / zones count tracked objects: they need track true")
        # the frame-watch launcher's ranges (csrc/kernels/frame_watch.hip)
        if self.watch_cell not in (8, 16, 32):
            raise ValueError("watch_cell must be 8, 16 or 32")
        if self.watch_row_step not in (1, 2, 4):
            raise ValueError("watch_row_step must be 1, 2 or 4")
        if not 0 <= self.watch_bg_shift <= 8:
            raise ValueError("watch_bg_shift must be 0..8")
        if not 0.0 <= self.watch_motion_level <= 255.0:
            raise ValueError("watch_motion_level must be 0..255 luma levels")
        if not (0.0 <= self.watch_motion_share <= 1.0 and 0.0 <= self.watch_scene_share <= 1.0):
            raise ValueError("watch_motion_share / watch_scene_share must be in [0, 1]")
        if not (0.0 <= self.watch_dark_level <= 256.0 and 0.0 <= self.watch_flat_level <= 256.0):
            raise ValueError("watch_dark_level / watch_flat_level must be 0..256")
        if not 1 <= self.watch_hold <= 255:
            raise ValueError("watch_hold must be 1..255")
        if self.watch and self.model == "simulated-temperature":
            raise ValueError("watch needs frames: a vision model")
        if not 16 <= self.snapshot_width <= 1920:
            raise ValueError("snapshot_width must be 16..1920")
        if self.snapshot_subsampling not in SNAPSHOT_SUBSAMPLINGS:
            raise ValueError(f"snapshot_subsampling must be one of {SNAPSHOT_SUBSAMPLINGS}, got "
                             f"{self.snapshot_subsampling!r}")
        if not 1 <= self.snapshot_quality <= 100:
            raise ValueError("snapshot_quality must be 1..100")
        if self.snapshot_every_s < 0:
            raise ValueError("snapshot_every_s must be >= 0 (0 = never periodic)")
        if self.snapshot_max_bytes < 1:
            raise ValueError("snapshot_max_bytes must be >= 1")
        if self.snapshots and self.model == "simulated-temperature":
            raise ValueError("snapshots need frames: a vision model")
        # the annotate style's ranges (ops.AnnotateStyle, csrc/kernels/annotate.hip)
        if self.snapshot_labels not in SNAPSHOT_LABELS:
            raise ValueError(f"snapshot_labels must be one of {SNAPSHOT_LABELS}, got "
                             f"{self.snapshot_labels!r}")
        if not 1 <= self.snapshot_box_thickness <= 4:
            raise ValueError("snapshot_box_thickness must be 1..4")
        if not 1 <= self.snapshot_label_scale <= 2:
            raise ValueError("snapshot_label_scale must be 1..2")
        if self.snapshot_privacy_block not in (4, 8, 16):
            raise ValueError("snapshot_privacy_block must be 4, 8 or 16")
        if len(self.snapshot_privacy_classes) > MAX_PRIVACY:
            raise ValueError(f"at most {MAX_PRIVACY} snapshot_privacy_classes, got "
                             f"{len(self.snapshot_privacy_classes)}")
        if not all(0 <= c <= 65535 for c in self.snapshot_privacy_classes):
            raise ValueError("snapshot_privacy_classes must be class ids 0..65535")
        pz = self.snapshot_privacy_zones
        if len(pz) > MAX_PRIVACY:
            raise ValueError(f"at most {MAX_PRIVACY} snapshot_privacy_zones, got {len(pz)}")
        if len({r["name"] for r in pz}) != len(pz):
            raise ValueError("snapshot_privacy_zones names must be unique, got "
                             f"{[r['name'] for r in pz]}")
        for r in pz:
            if r["cameras"] is not None and not all(0 <= c < self.batch for c in r["cameras"]):
                raise ValueError(f"privacy zone {r['name']!r}: cameras must be 0..batch - 1")
            if not 3 <= len(r["polygon"]) <= 8:
                raise ValueError(f"privacy zone {r['name']!r} needs 3..8 vertices, got "
                                 f"{len(r['polygon'])}")
        if self.snapshot_annotate:  # cross-key limits bind only when the stage is on
            if not self.snapshots:
                raise ValueError("snapshot_annotate draws into the snapshots: it needs "
                                 "snapshots true")
            base = ModuleConfig.__dataclass_fields__
            if self.model not in ("yolov8n", "detect-classify"):
                for k in self.ANNOTATE_BOX_KEYS:
                    if getattr(self, k) != base[k].default:
                        raise ValueError(f"{k} needs a detector: model {self.model} has no "
                                         f"boxes (snapshot_privacy_zones work with any model)")
        if not 1 <= self.steps_per_poll <= 1000:
            raise ValueError("steps_per_poll must be 1..1000")
        if not 0.0 <= self.refine_s <= 600.0:
            raise ValueError("refine_s must be 0..600")
        if not 0 <= self.sync_every <= 10000:
            raise ValueError("sync_every must be 0..10000")
        return self

    def apply_patch(self, patch: Dict[str, Any]) -> "ModuleConfig":
        """Apply a (partial) twin desired-properties patch; unknown keys and the
        IoT Hub '$version' bookkeeping are ignored; types are coerced."""
        kw = {}
        by_name = {f.name: f for f in fields(self)}
        for k, v in (patch or {}).items():
            if k.startswith("$") or k not in by_name:
                continue
            cur = getattr(self, k)
            if isinstance(cur, bool):
                v = v if isinstance(v, bool) else str(v).lower() in ("1", "true", "yes")
            elif isinstance(cur, int):
                v = int(v)
            elif isinstance(cur, float):
                v = float(v)
            elif k == "snapshot_privacy_zones":
                v = _privacy_zones(v)
            elif k == "snapshot_privacy_classes":
                v = _int_tuple(v, k)
            elif isinstance(cur, tuple):
                v = _regions(v, k)
            else:
                v = str(v)
            kw[k] = v
        return replace(self, **kw).validate()

    def needs_rebuild(self, other: "ModuleConfig") -> bool:
        return any(getattr(self, k) != getattr(other, k) for k in self.REBUILD)

    def resolved_image_size(self) -> int:
        if self.image_size:
            return self.image_size
        return 640 if self.model in ("yolov8n", "detect-classify") else 224

    def frame_hw(self):
        """(frame_height, frame_width), or None when frames arrive at model size."""
        return (self.frame_height, self.frame_width) if self.frame_height else None

    def is_camera(self) -> bool:
        """A host producer feeds the ring (any frame format)."""
        return self.source in ("camera", "camera-nv12")

    def frame_format(self) -> str:
        """Format of the incoming frames (InferenceEngine frame_format)."""
        return "nv12" if self.source == "camera-nv12" else "rgb"

    TRACK_KEYS = ("track", "track_iou", "track_max_age", "track_min_hits", "track_max_tracks")
    ZONE_KEYS = ("lines", "zones", "zone_anchor")
    WATCH_KEYS = ("watch", "watch_cell", "watch_row_step", "watch_bg_shift",
                  "watch_motion_level", "watch_motion_share", "watch_scene_share",
                  "watch_dark_level", "watch_flat_level", "watch_hold")

    SNAPSHOT_KEYS = ("snapshots", "snapshot_width", "snapshot_subsampling", "snapshot_quality",
                     "snapshot_every_s", "snapshot_max_bytes")

    # the annotate stage: what needs boxes, and what the device reads live
    ANNOTATE_BOX_KEYS = ("snapshot_boxes", "snapshot_labels", "snapshot_box_thickness",
                         "snapshot_label_scale", "snapshot_privacy_classes")
    ANNOTATE_LIVE_KEYS = ANNOTATE_BOX_KEYS + ("snapshot_privacy_block", "snapshot_privacy_zones")
    ANNOTATE_KEYS = ("snapshot_annotate",) + ANNOTATE_LIVE_KEYS

    def watch_params(self) -> Dict[str, int]:
        """The threshold words of ops.WatchState.set_params: levels in 1/16 luma
        (floor(level * 16 + 0.5)), shares in 1/1024 of the cells."""
        import math

        def q(v, scale):
            return int(math.floor(float(v) * scale + 0.5))

        return {"motion_thr16": q(self.watch_motion_level, 16),
                "motion_share_q": q(self.watch_motion_share, 1024),
                "scene_share_q": q(self.watch_scene_share, 1024),
                "dark16": q(self.watch_dark_level, 16), "flat16": q(self.watch_flat_level, 16),
                "hold": int(self.watch_hold)}

    def to_dict(self) -> Dict[str, Any]:
        """The reported / saved config.  The tracking keys are listed once any of them has
        left its default: a module that was never asked to track reports exactly the config
        it reported before tracking existed."""
        d = asdict(self)
        base = ModuleConfig()
        if all(getattr(self, k) == getattr(base, k) for k in self.TRACK_KEYS):
            for k in self.TRACK_KEYS:
                d.pop(k)
        # likewise the line / zone keys
        if all(getattr(self, k) == getattr(base, k) for k in self.ZONE_KEYS):
            for k in self.ZONE_KEYS:
                d.pop(k)
        else:
            d["lines"], d["zones"] = list(d["lines"]), list(d["zones"])
        # and the frame-watch keys
        if all(getattr(self, k) == getattr(base, k) for k in self.WATCH_KEYS):
            for k in self.WATCH_KEYS:
                d.pop(k)
        # and the snapshot keys
        if all(getattr(self, k) == getattr(base, k) for k in self.SNAPSHOT_KEYS):
            for k in self.SNAPSHOT_KEYS:
                d.pop(k)
        # and the annotate keys
        if all(getattr(self, k) == getattr(base, k) for k in self.ANNOTATE_KEYS):
            for k in self.ANNOTATE_KEYS:
                d.pop(k)
        else:
            d["snapshot_privacy_classes"] = list(d["snapshot_privacy_classes"])
            d["snapshot_privacy_zones"] = list(d["snapshot_privacy_zones"])
        return d
