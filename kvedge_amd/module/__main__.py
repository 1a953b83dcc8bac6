"""`python -m kvedge_amd.module` -- the IoT Edge module entry point (also bare-metal).

Inside IoT Edge: --transport azure (twin/methods/outputs via edgeHub).  Outside:
--transport stdout prints telemetry as JSON lines; CLI flags mirror the twin keys
 and are overridden by the twin's desired properties.
"""
from __future__ import annotations

import argparse
import os
import signal
import sys
import time

from .. import parallel
from .app import GpuUnavailableError, ModuleApp
from .config import ModuleConfig
from .transport import make_transport

_T_IMPORTED = time.time()  # torch, the op library bindings and the module are imported


def _process_start_epoch():
    """Epoch at which the kernel started this process (/proc: boot time + start ticks)."""
    try:
        with open("/proc/self/stat") as f:
            start_ticks = int(f.read().rsplit(")", 1)[1].split()[19])
        with open("/proc/stat") as f:
            btime = next(int(ln.split()[1]) for ln in f if ln.startswith("btime"))
        return btime + start_ticks / os.sysconf("SC_CLK_TCK")
    except (OSError, ValueError, StopIteration, IndexError):
        return None


def _topology_from_env() -> int:
    """Map the chart's per-VM env (KVEDGE_NODE_RANK / KVEDGE_NNODES /
    KVEDGE_RANKS_PER_NODE, deploy/helm/templates/kvedge-module-deployment.yaml) to
    torch.distributed's.  Returns the number of local ranks this process must launch
    (0 = run in-process)."""
    if "WORLD_SIZE" in os.environ:  # already a launched rank (torchrun / our launcher)
        return 0
    nnodes = int(os.environ.get("KVEDGE_NNODES", "1"))
    rpn = int(os.environ.get("KVEDGE_RANKS_PER_NODE", "1"))
    node = int(os.environ.get("KVEDGE_NODE_RANK", "0"))
    if rpn > 1:
        return rpn
    if nnodes > 1:  # one GPU per VM: this process IS the rank
        os.environ.update(RANK=str(node), LOCAL_RANK="0", WORLD_SIZE=str(nnodes))
    return 0


def main(argv=None):
    local = _topology_from_env()
    if local:
        # topology (a): one VM owns several GPUs -> one child rank per GPU (the parent
        # never touches the GPU); topology (a)+(b) mixes work the same way per VM
        pkg_root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        env = dict(os.environ, PYTHONPATH=os.pathsep.join(
            p for p in (pkg_root, os.environ.get("PYTHONPATH", "")) if p))
        return parallel.launch_local(
            local, ["-m", "kvedge_amd.module", *(sys.argv[1:] if argv is None else argv)],
            env=env,
            node_rank=int(os.environ.get("KVEDGE_NODE_RANK", "0")),
            nnodes=int(os.environ.get("KVEDGE_NNODES", "1")),
            master_addr=os.environ.get("MASTER_ADDR"),
            master_port=int(os.environ["MASTER_PORT"]) if "MASTER_PORT" in os.environ else None)
    d = ModuleConfig()
    ap = argparse.ArgumentParser(prog="kvedge-module")
    ap.add_argument("--transport", default=os.environ.get("KVEDGE_TRANSPORT", "stdout"),
                    choices=["stdout", "fake", "azure"])
    ap.add_argument("--model", default=os.environ.get("KVEDGE_MODEL", d.model))
    ap.add_argument("--batch", type=int, default=int(os.environ.get("KVEDGE_BATCH", d.batch)))
    ap.add_argument("--dtype", default=os.environ.get("KVEDGE_DTYPE", d.dtype))
    ap.add_argument("--seed", type=int, default=d.seed)
    ap.add_argument("--report-interval-s", type=float, default=d.report_interval_s)
    ap.add_argument("--image-size", type=int, default=d.image_size)
    ap.add_argument("--frame-height", type=int, default=d.frame_height,
                    help="native frame height, resampled to the model size on the device "
                         "(0 with --frame-width 0 = frames arrive at model size)")
    ap.add_argument("--frame-width", type=int, default=d.frame_width,
                    help="native frame width (a multiple of 8)")
    ap.add_argument("--crops-per-image", type=int, default=d.crops_per_image,
                    help="--model detect-classify: boxes per frame cut out and classified "
                         "(1..16, <= max_det)")
    ap.add_argument("--track", action="store_true",
                    help="--model yolov8n / detect-classify: track objects across frames "
                         "(one batch row = one camera; telemetry gains `tracks`)")
    ap.add_argument("--track-iou", type=float, default=d.track_iou,
                    help="tracker association gate, IoU in (0, 1]")
    ap.add_argument("--track-max-age", type=int, default=d.track_max_age,
                    help="frames a lost track coasts before it is dropped (0..255)")
    ap.add_argument("--track-min-hits", type=int, default=d.track_min_hits,
                    help="consecutive matches before a track gets its id (1..255)")
    ap.add_argument("--track-max-tracks", type=int, default=d.track_max_tracks,
                    help="track slots per camera (64, 128, 192 or 256)")
    ap.add_argument("--lines-json", default="",
                    help="--track: virtual lines counted on the device, inline JSON "
                         "'[{\"name\": ..., \"a\": [x, y], \"b\": [x, y], \"class\"?, "
                         "\"cameras\"?}]' (at most 8; telemetry gains `lines`)")
    ap.add_argument("--zones-json", default="",
                    help="--track: polygon zones, inline JSON '[{\"name\": ..., \"polygon\": "
                         "[[x, y], ...], \"class\"?, \"cameras\"?}]' (at most 8, 3..8 vertices; "
                         "telemetry gains `zones`)")
    ap.add_argument("--zone-anchor", default=d.zone_anchor, choices=["bottom", "centre"],
                    help="the point of a box tested against lines and zones")
    ap.add_argument("--watch", action="store_true",
                    help="watch every camera's frames on the device (one batch row = one "
                         "camera): motion grid, dark / flat / frozen / scene alarms; telemetry "
                         "gains `cameras` and `camera_alarms`")
    ap.add_argument("--watch-cell", type=int, default=d.watch_cell, choices=[8, 16, 32],
                    help="motion grid cell, pixels")
    ap.add_argument("--watch-row-step", type=int, default=d.watch_row_step, choices=[1, 2, 4],
                    help="read every n-th frame row")
    ap.add_argument("--watch-bg-shift", type=int, default=d.watch_bg_shift,
                    help="background = mean of about 2^k frames (0..8; 0 = frame differencing)")
    ap.add_argument("--watch-motion-level", type=float, default=d.watch_motion_level,
                    help="luma levels a cell must differ from the background to move")
    ap.add_argument("--watch-motion-share", type=float, default=d.watch_motion_share,
                    help="share of moving cells for `motion`")
    ap.add_argument("--watch-scene-share", type=float, default=d.watch_scene_share,
                    help="share of moving cells for `scene` (camera moved or covered)")
    ap.add_argument("--watch-dark-level", type=float, default=d.watch_dark_level,
                    help="mean luma below which the scene is `dark`")
    ap.add_argument("--watch-flat-level", type=float, default=d.watch_flat_level,
                    help="mean neighbour difference below which the picture is `flat`")
    ap.add_argument("--watch-hold", type=int, default=d.watch_hold,
                    help="frames a condition must hold before its alarm (1..255)")
    ap.add_argument("--snapshots", action="store_true",
                    help="encode every camera's frame as a JPEG thumbnail on the device; "
                         "pictures leave on output `snapshots` with watch alarms and "
                         "periodically, and through direct method `snapshot`")
    ap.add_argument("--snapshot-width", type=int, default=d.snapshot_width,
                    help="thumbnail width, pixels (16..1920; the height follows the frame)")
    ap.add_argument("--snapshot-subsampling", default=d.snapshot_subsampling,
                    choices=["420", "444"], help="chroma subsampling of the JPEG")
    ap.add_argument("--snapshot-quality", type=int, default=d.snapshot_quality,
                    help="JPEG quality 1..100 (changes without a rebuild)")
    ap.add_argument("--snapshot-every-s", type=float, default=d.snapshot_every_s,
                    help="seconds between periodic pictures per camera (0 = never)")
    ap.add_argument("--snapshot-max-bytes", type=int, default=d.snapshot_max_bytes,
                    help="a larger picture is counted as oversize, not sent")
    ap.add_argument("--snapshot-annotate", action="store_true",
                    help="--snapshots: draw boxes, cls:id labels and the privacy mosaic into "
                         "the pictures on the device (messages gain `annotated`)")
    ap.add_argument("--snapshot-labels", default=d.snapshot_labels,
                    choices=["none", "class", "id", "both"],
                    help="label parts of an annotated box (changes without a rebuild)")
    ap.add_argument("--privacy-classes", default="",
                    help="class ids whose boxes are hidden under a mosaic, e.g. 0,2 (at most 8)")
    ap.add_argument("--privacy-zones-json", default="",
                    help="polygons hidden under a mosaic, inline JSON '[{\"name\": ..., "
                         "\"polygon\": [[x, y], ...], \"cameras\"?}]' (at most 8, 3..8 vertices)")
    ap.add_argument("--fps", type=float, default=d.fps)
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--source", default=d.source,
                    choices=["synthetic", "camera", "camera-nv12"],
                    help="camera-nv12: NV12 frames through the ring (needs --frame-height / "
                         "--frame-width)")
    ap.add_argument("--no-native-loop", action="store_true")
    ap.add_argument("--steps-per-poll", type=int, default=d.steps_per_poll)
    ap.add_argument("--refine-s", type=float, default=d.refine_s,
                    help="seconds of in-graph tile refinement at engine build (0 = off)")
    ap.add_argument("--steps", type=int, default=None, help="stop after N steps")
    ap.add_argument("--duration-s", type=float, default=None)
    ap.add_argument("--sync-every", type=int, default=d.sync_every,
                    help="module steps between lockstep control boundaries (0 = auto)")
    ap.add_argument("--state", default=os.environ.get("KVEDGE_STATE", "/var/lib/kvedge/module-state.json"))
    ap.add_argument("--heartbeat", default=os.environ.get("KVEDGE_HEARTBEAT", ""),
                    help="heartbeat file rewritten at every report (VMI health probes)")
    ap.add_argument("--stamps", default=os.environ.get("KVEDGE_STAMPS", "/var/lib/kvedge/boot-timing"),
                    help="guest boot-timing stamp file (module_first_inference is appended)")
    ap.add_argument("--tune-cache", default=os.environ.get("KVEDGE_TUNE_CACHE",
                                                           "/var/lib/kvedge/tune-cache.json"),
                    help="autotuner picks on the persistent disk ('' = always re-tune)")
    ap.add_argument("--require-gpu", type=int, default=int(os.environ.get("KVEDGE_REQUIRE_GPU", "0") or 0),
                    help="exit non-zero unless at least this many GPUs are visible (the chart "
                         "sets KVEDGE_REQUIRE_GPU from gpu.count; 0 = allow the CPU)")
    a = ap.parse_args(argv)
    di = parallel.init_from_env(prefer_gpu=True)
    cfg = ModuleConfig(model=a.model, batch=a.batch, dtype=a.dtype, seed=a.seed,
                       report_interval_s=a.report_interval_s, image_size=a.image_size,
                       fps=a.fps, use_graph=not a.no_graph, world_size=di.world_size,
                       source=a.source, native_loop=not a.no_native_loop,
                       steps_per_poll=a.steps_per_poll, sync_every=a.sync_every,
                       refine_s=a.refine_s, frame_height=a.frame_height,
                       frame_width=a.frame_width,
                       crops_per_image=a.crops_per_image, track=a.track,
                       track_iou=a.track_iou, track_max_age=a.track_max_age,
                       track_min_hits=a.track_min_hits,
                       track_max_tracks=a.track_max_tracks, lines=a.lines_json,
                       zones=a.zones_json, zone_anchor=a.zone_anchor, watch=a.watch,
                       watch_cell=a.watch_cell, watch_row_step=a.watch_row_step,
                       watch_bg_shift=a.watch_bg_shift,
                       watch_motion_level=a.watch_motion_level,
                       watch_motion_share=a.watch_motion_share,
                       watch_scene_share=a.watch_scene_share,
                       watch_dark_level=a.watch_dark_level,
                       watch_flat_level=a.watch_flat_level, watch_hold=a.watch_hold,
                       snapshots=a.snapshots, snapshot_width=a.snapshot_width,
                       snapshot_subsampling=a.snapshot_subsampling,
                       snapshot_quality=a.snapshot_quality,
                       snapshot_every_s=a.snapshot_every_s,
                       snapshot_max_bytes=a.snapshot_max_bytes,
                       snapshot_annotate=a.snapshot_annotate,
                       snapshot_labels=a.snapshot_labels,
                       snapshot_privacy_classes=a.privacy_classes,
                       snapshot_privacy_zones=a.privacy_zones_json).validate()
    # one IoT Edge identity per VM: only local rank 0 talks to edgeHub
    kind = a.transport if di.local_rank == 0 or a.transport != "azure" else "null"
    try:
        app = ModuleApp(make_transport(kind), cfg, state_path=a.state,
                        stamp_path=a.stamps or None, heartbeat_path=a.heartbeat or None,
                        tune_cache=a.tune_cache or None, require_gpus=a.require_gpu)
    except GpuUnavailableError as e:
        print(str(e), file=sys.stderr, flush=True)
        parallel.shutdown()
        return 3
    # cold-start legs: this process's start (kernel start time) and the end of imports; no
    # process-start stamp when /proc cannot say (a stamp at "now" would corrupt the legs)
    t_start = _process_start_epoch()
    if t_start is not None:
        app._stamp("module_process_start", t_start)
    app._stamp("module_imported", _T_IMPORTED)
    # SIGTERM (edgeAgent stop, VM shutdown) only votes to stop: the replicas leave the
    # loop together at the next control boundary, so the final report's collectives match
    signal.signal(signal.SIGTERM, lambda *_: app.request_stop())
    app.start()
    try:
        app.run(max_steps=a.steps, duration_s=a.duration_s)
        if app.engine is not None:
            app.report()
    finally:
        app.stop()
        parallel.shutdown()
    return 0


if __name__ == "__main__":
    sys.exit(main())
