"""Scene-level driver of the hot path: what MVSDet.extract_feat does between the 2-D neck and the 3-D neck
(mvsdet.py:404-515 of Pixie8888/MVSDet), on the HIP operators.

    features (N,C,Hf,Wf) + img_meta  ->  volume_mean (C,X,Y,Z), valid count (1,X,Y,Z)
                                         (+ prob_volume, depth_coding, est_depth, est_densities for the NVS branch)

Per scene the host does only the camera algebra on N 4x4 matrices (`prepare_scene`, ATen-CPU like the
reference); everything proportional to pixels or voxels runs in five kernel launches:
pack -> plane-sweep variance -> [cost regularisation network, not ours] -> depth_prob_topk -> backproject mean.
"""
from __future__ import annotations

from collections.abc import Mapping
from dataclasses import dataclass
from typing import Callable, Optional, Sequence

import numpy as np
import torch
from torch import Tensor

from . import functional as F_
from . import ops


@dataclass
class SceneGeometry:
    """Device-resident camera data of one scene (all tiny)."""
    neighbor_ids: Tensor   # (N,k) int64   mvsdet.py:434
    proj_rel: Tensor       # (N,k,4,4)     nei_proj @ inverse(ref_proj), module.py:116
    depth_values: Tensor   # (N,D)         mvsdet.py:450
    projection: Tensor     # (N,3,4)       mvsdet.py:407
    points: Tensor         # (3,X,Y,Z)     mvsdet.py:409
    height: int            # un-padded feature rows (img_shape[0] // stride)
    width: int


def _tensors_of(v):
    if isinstance(v, Tensor):
        yield v
    elif isinstance(v, (list, tuple)):
        for x in v:
            yield from _tensors_of(x)


class SceneOutputs(Mapping):
    """What `forward_scene` returns: a read-only mapping.  With `overlap_detector` everything but `variance` was produced on a
    side stream and is only valid behind the event `ready`: this holder makes the stream that READS a value wait for that event
    (once the event has completed the check is one query) and tells the caching allocator that the stream uses the value's
    memory, so a consumer on any stream -- the caller's, a third one -- gets correct data without knowing about the side stream.
    It is a `collections.abc.Mapping`, not a `dict` subclass: `dict(out)`, `{**out}`, iteration over `items()` / `values()` and
    `get` all go through `__getitem__` and therefore through the wait (CPython copies a dict SUBCLASS with its fast path,
    past any override); there is no `pop` / `setdefault` / item assignment to get around it.
    `ready`, `detector_ready`, `geometry` and `variance` (produced on the caller's own stream) are handed out as they are;
    `out.raw(key)` bypasses the wait for callers that order the streams themselves."""

    _PLAIN = ("ready", "detector_ready", "geometry", "variance")
    __slots__ = ("_d",)

    def __init__(self, **values):
        self._d = dict(values)

    def raw(self, key):
        return self._d[key]

    def _put(self, key, value):
        """The producer's own write (this module only; the side stream is current or ordered by the caller)."""
        self._d[key] = value

    def __getitem__(self, key):
        value = self._d[key]
        ev = self._d.get("ready")
        if ev is None or key in self._PLAIN:
            return value
        cur = None
        for t in _tensors_of(value):
            if t.is_cuda:
                if cur is None:
                    cur = torch.cuda.current_stream(t.device)
                    if not ev.query():
                        cur.wait_event(ev)
                t.record_stream(cur)
        return value

    def __iter__(self):
        return iter(self._d)

    def __len__(self):
        return len(self._d)

    def __contains__(self, key):
        return key in self._d

    def copy(self) -> dict:
        return dict(self)          # through __getitem__: the copy's values are safe on the current stream

    def __repr__(self):
        return f"SceneOutputs({list(self._d)})"


class _GeometryWorker:
    """One daemon thread per MVSDetHotPath: evaluates `_host_geometry` (ATen-CPU, one intra-op thread -- set ONCE, in this
    thread; note that torch.set_num_threads also sets MKL's process-wide thread count), packs the results into a pinned
    staging buffer and uploads them with a single asynchronous copy on its own stream.  What hides the camera algebra in a
    real pipeline is `prefetch_scene`: the data loader knows the next scene while the current one runs.  Entries are also
    kept by the CONTENT of the camera data (a 16-byte digest of extrinsics, intrinsics, origin and image shapes), which
    only pays when the very same cameras AND origin come again (loss + predict on one batch, repeated evaluation): the
    reference's training pipeline re-samples the views and shifts the origin per item (multiview_pipeline.py:141,
    RandomShiftOrigin), so there every scene is a miss.  `stats` counts the three cases."""

    _ALIGN = 16

    def __init__(self, owner, max_entries: int = 32):
        import queue
        import threading
        self.owner = owner
        self.max_entries = max_entries
        self.entries: dict = {}        # id(img_meta) -> [img_meta, device, threading.Event, SceneGeometry | Exception, cuda Event]
        self.lock = threading.Lock()
        self.todo: "queue.Queue" = queue.Queue()
        self.thread = None
        self.streams: dict = {}
        # prefetch_joins: prepare_scene found the entry its own prefetch_scene made (same dict object);
        # content_hits: an entry made for ANOTHER dict with the same camera bytes; misses: algebra + upload ran
        self.stats = {"misses": 0, "prefetch_joins": 0, "content_hits": 0}

    def _start(self):
        import threading
        if self.thread is None or not self.thread.is_alive():
            self.thread = threading.Thread(target=self._run, name="mvsdet-geometry", daemon=True)
            self.thread.start()

    @staticmethod
    def _content_key(img_meta: dict, device):
        """The camera data the geometry depends on, as bytes (`origin` included: the voxel points hang on it)."""
        import hashlib
        l2i = img_meta["lidar2img"]
        h = hashlib.blake2b(digest_size=16)
        h.update(np.ascontiguousarray(np.asarray(l2i["extrinsic"], dtype=np.float32)).tobytes())
        h.update(np.ascontiguousarray(np.asarray(l2i["intrinsic"], dtype=np.float32)).tobytes())
        h.update(np.asarray(l2i["origin"], dtype=np.float32).tobytes())
        h.update(repr((tuple(img_meta["img_shape"][:2]), tuple(img_meta["ori_shape"][:2]), isinstance(l2i["intrinsic"], list))).encode())
        return (h.digest(), str(device))

    def submit(self, img_meta: dict, device, count: bool = False):
        import threading
        key = self._content_key(img_meta, device)
        with self.lock:
            ent = self.entries.get(key)
            if ent is not None:
                if count:
                    self.stats["prefetch_joins" if ent[0] is img_meta else "content_hits"] += 1
                self.entries[key] = self.entries.pop(key)   # most recently used last
                return ent
            while len(self.entries) >= self.max_entries:    # least recently used finished entry first
                old = next((k for k, e in self.entries.items() if e[2].is_set()), None)
                if old is None:
                    break
                del self.entries[old]
            ent = [img_meta, device, threading.Event(), None, None]
            self.entries[key] = ent
            self.stats["misses"] += 1
        self._start()
        self.todo.put(ent)
        return ent

    def get(self, img_meta: dict, device) -> "SceneGeometry":
        ent = self.submit(img_meta, device, count=True)
        ent[2].wait()
        if isinstance(ent[3], BaseException):
            with self.lock:
                self.entries.pop(self._content_key(img_meta, device), None)
            raise ent[3]
        if ent[4] is not None:   # the caller's stream waits for the upload; the host does not
            cur = torch.cuda.current_stream(device)
            cur.wait_event(ent[4])
            ent[3].neighbor_ids.record_stream(cur)   # all four views share the one uploaded buffer
            ent[3].points.record_stream(cur)         # allocated under the worker's stream too (its own block)
        return ent[3]

    def _run(self):
        torch.set_num_threads(1)   # once, in this thread: N 4x4 matrices do not want an OpenMP team
        while True:
            ent = self.todo.get()
            try:
                ent[3], ent[4] = self._build(ent[0], ent[1])
            except BaseException as exc:  # noqa: BLE001 -- handed to the waiting caller
                ent[3] = exc
            ent[2].set()

    def _build(self, img_meta: dict, device):
        hp = self.owner
        nbr, proj_rel, depth_values, projection, origin, height, width = hp._host_geometry(img_meta)
        parts = [nbr.contiguous(), proj_rel.contiguous(), depth_values.contiguous(), projection.contiguous()]
        if device.type != "cuda":
            points = hp._voxel_points(origin, device)
            return SceneGeometry(parts[0], parts[1], parts[2], parts[3], points, height, width), None
        offs, total = [], 0
        for t in parts:
            offs.append(total)
            total += (t.numel() * t.element_size() + self._ALIGN - 1) // self._ALIGN * self._ALIGN
        stage = torch.empty(max(total, self._ALIGN), dtype=torch.uint8, pin_memory=True)
        for t, o in zip(parts, offs):
            nb = t.numel() * t.element_size()
            if nb:
                stage[o:o + nb].copy_(t.reshape(-1).view(torch.uint8))
        stream = self.streams.get(str(device))
        if stream is None:
            stream = self.streams[str(device)] = torch.cuda.Stream(device=device)
        with torch.cuda.stream(stream):
            dev = stage.to(device, non_blocking=True)        # ONE host-to-device copy per scene
            points = hp._voxel_points(origin, device)
            done = torch.cuda.Event()
            done.record(stream)
        views = []
        for t, o in zip(parts, offs):
            nb = t.numel() * t.element_size()
            views.append(dev[o:o + nb].view(t.dtype).view(t.shape))
        geo = SceneGeometry(views[0], views[1], views[2], views[3], points, height, width)
        geo._staging = stage   # keeps the pinned buffer alive until the geometry is dropped
        return geo, done


class MVSDetHotPath:
    """Holds the hyper-parameters MVSDet.__init__ keeps for this path (mvsdet.py:165-230)."""

    def __init__(self, n_voxels: Sequence[int], voxel_size: Sequence[float], near_far_range: Sequence[float],
                 num_monocular_samples: int, topk: int = 3,
                 cost_regularization: Optional[Callable[[Tensor], Tensor]] = None, stride: int = 4,
                 neck_3d: Optional[Callable[[Tensor], list]] = None,
                 bbox_head: Optional[Callable[[list], tuple]] = None, test_cfg=None):
        self.n_voxels = [int(v) for v in n_voxels]
        self.voxel_size = [float(v) for v in voxel_size]      # python floats -> torch.tensor(...) is fp32, as in the reference
        self.near_far_range = [float(v) for v in near_far_range]
        self.num_depth = int(num_monocular_samples)
        self.topk = int(topk)
        self.stride = int(stride)
        # mvsdet.py:221-225
        self.depth_interval = (self.near_far_range[1] - self.near_far_range[0]) / self.num_depth
        self.depth_values = np.arange(self.near_far_range[0], self.near_far_range[1], self.depth_interval,
                                      dtype=np.float32)
        assert len(self.depth_values) == self.num_depth
        self.cost_regularization = cost_regularization
        self.neck_3d = neck_3d   # mvsdet.py:681-698: x = self.neck_3d(torch.stack(volumes)); SURVEY 8 f-3 (mvsdet_amd.neck)
        self.bbox_head = bbox_head   # nerfdet_head.py:116-118: the head's convolutions on the neck's levels (mvsdet_amd.head)
        # opt-in: an `mvsdet_amd.fpn.FPNLevel0` (mvsdet.py:374-376, `self.neck(x)[0]`) for `forward_scene_from_stages`; every other
        # entry starts from the feature map and never looks at it
        self.fpn = None
        # opt-in: an `mvsdet_amd.resnet.ResNetStages` (the 2-D backbone's C2..C5) for `forward_scene_from_images`
        self.backbone = None
        # opt-in: with a test_cfg (nms_pre, score_thr, iou_thr), out["detections"] = the padded boxes of predict_by_feat
        # (ops.HeadPrediction; 7-wide and class-major for a head with `arkit_head`) made from out["head"] and out["valid"] on the
        # stream the head ran on
        self.test_cfg = test_cfg
        self._points_cache: dict = {}
        self._geo_streams: dict = {}
        self._geometry = _GeometryWorker(self)
        # "auto": the tabled sweep of forward_scene writes a ROW-PITCHED volume (rows on 128-byte lines, handed out as the
        # (N,C,D,H,W) view of an (N,C,D,H,pitch) buffer: same values, `stride(3)` = pitch) where that pays -- maps whose
        # width is a multiple of 16 but not of 32 swept with the 32x4 tiles (48 planes or more): 6.1 against 6.5 ms at 50 views x
        # 96 planes x 60x80.  The cost network and the depth distribution read such views in place.  False: always contiguous.
        self.pitched_variance = "auto"
        # True: what follows the cost network (depth distribution, lifting, neck_3d / bbox_head) runs on a side stream; forward_scene
        # returns out["ready"] (= out["detector_ready"]), a CUDA event the consumer's stream waits for
        # "auto": the route is MEASURED per scene shape -- the first scenes of a shape run each route of `OVERLAP_ROUTES` for a few
        # scenes (period between consecutive scenes' cost networks finishing on the caller's stream, HIP events, no host wait) and the
        # fastest is kept (a side route only if it beats the one-stream route by 1 %): what the side stream buys depends on the view
        # count, on how many hardware queues the process's streams share and on the box (profiles/r06_overlap_routes.txt: +10 % at
        # 40 views, -1.7 % .. +5 % at 80, +2 % at 100 for the same code), so no fixed rule is right everywhere.
        self.overlap_detector = False
        # view streams of the cost network while the detector tail of the previous scene runs beside it (overlap_detector = True)
        self.overlap_network_streams = 1
        self._overlap_tuning: dict = {}
        self._detector_streams: dict = {}

    # ---- reference-named methods (mvsdet.py:249, 266, 298) -------------------------------------------
    def collect_proj(self, w2c, intr, neighbor_ids):
        return F_.collect_proj(w2c, intr, neighbor_ids)

    def sample_depth_prob(self, prob_volume: Tensor, off_pred: Tensor, topk: int = 3):
        """mvsdet.py:266-283 -> (est_depth (N,k,H,W), est_density (N,k,H,W))."""
        est_depth, est_dens, _, _ = ops.sample_depth_prob(prob_volume, off_pred, float(self.near_far_range[0]),
                                                          float(self.depth_interval), int(topk))
        return est_depth, est_dens

    def compute_avg_depth(self, prob_volume: Tensor, off_pred: Tensor):
        """mvsdet.py:298-317 -> depth expectation (N,H,W)."""
        return ops.sample_depth_prob(prob_volume, off_pred, float(self.near_far_range[0]),
                                     float(self.depth_interval), min(self.topk, prob_volume.shape[1]))[3]

    # ---- host-side camera algebra -----------------------------------------------------------------------
    def prepare_scene(self, img_meta: dict, device) -> SceneGeometry:
        """mvsdet.py:407-450 for one scene, evaluated with ATen-CPU exactly as the reference does, then uploaded.
        The algebra runs on this object's geometry worker thread (single-threaded ATen: on a 256-core host the OpenMP
        fork/join of the default pool costs ~10 ms per scene for N 4x4 matrices), is packed into ONE pinned staging
        buffer and reaches the device as ONE asynchronous copy on a side stream; the caller's stream waits for it with
        an event, never the host.  Results are kept by the content of the camera data, so a scene seen again (or
        announced with `prefetch_scene` while the previous scene was running) costs a digest and a dictionary lookup."""
        return self._geometry.get(img_meta, torch.device(device))

    def prefetch_scene(self, img_meta: dict, device) -> None:
        """Start the camera algebra and the upload of a coming scene on the worker thread; returns at once."""
        self._geometry.submit(img_meta, torch.device(device))

    def ray_depth(self, img_meta: dict, est_depth: Tensor):
        """NVS-branch input (mvsdet.py:487-494): `cur_depth_scale` (N, h*w, 1) of compute_depth_scale[_MultiIntrin]
        (:1158-1216) and `est_ray_depth` (N, h*w, 1, J) = est_depth / (scale + 1e-8) from the padded (N,J,Hf,Wf) candidates.
        est_ray_depth carries the reference's gradient back to est_depth (ops.ray_depth); depth_scale carries none."""
        stride = self.stride
        h, w = img_meta["img_shape"][0] // stride, img_meta["img_shape"][1] // stride
        K = torch.tensor(np.array(img_meta["lidar2img"]["intrinsic"])).clone()
        ratio = img_meta["ori_shape"][0] / (img_meta["img_shape"][0] / stride)
        if K.dim() == 2:
            K[:2] /= ratio
            K = K.unsqueeze(0).repeat(est_depth.shape[0], 1, 1)      # one intrinsic matrix for all views (ScanNet)
        else:
            K[:, :2] /= ratio                                         # per-view intrinsics (ARKitScenes)
        intr = torch.stack([K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2], K[:, 0, 1]], dim=1).float()
        return ops.ray_depth(intr.to(est_depth.device), est_depth, int(h), int(w))

    def _feature_cameras(self, img_meta: dict):
        """World-to-camera matrices (N,4,4) and the intrinsics at feature level, (4,4) or per view (N,4,4) (mvsdet.py:419-431), on
        the host."""
        stride = self.stride
        w2c = torch.tensor(np.array(img_meta["lidar2img"]["extrinsic"]))
        K = torch.tensor(np.array(img_meta["lidar2img"]["intrinsic"]))
        ratio = img_meta["ori_shape"][0] / (img_meta["img_shape"][0] / stride)
        K_feat = K.clone()
        if K_feat.dim() == 2:
            K_feat[:2] /= ratio
        else:
            K_feat[:, :2] /= ratio
        return w2c, K_feat

    def _host_geometry(self, img_meta: dict):
        """The reference's ATen-CPU operator sequence (mvsdet.py:407-450) -> host tensors."""
        stride = self.stride
        projection = F_.compute_projection(img_meta, stride)
        height = img_meta["img_shape"][0] // stride
        width = img_meta["img_shape"][1] // stride
        w2c, K_feat = self._feature_cameras(img_meta)
        n = w2c.shape[0]
        k = min(2, n - 1)  # mvsdet.py:432
        c2w = w2c.inverse()
        nbr = F_.get_nearest_pose_ids(c2w, c2w, k, maskself=True)
        ops.validate_neighbors(nbr, n)  # the reference's index gather raises on an id outside [0, N)
        ref_proj, nei_projs = F_.collect_proj(w2c, K_feat, nbr)
        inv_ref = torch.inverse(ref_proj)
        if k > 0:
            proj_rel = torch.stack([torch.matmul(p, inv_ref) for p in nei_projs], dim=1)
        else:
            proj_rel = torch.zeros((n, 0, 4, 4))
        depth_values = torch.tensor(self.depth_values).unsqueeze(0).repeat(n, 1)
        origin = torch.tensor(img_meta["lidar2img"]["origin"])
        return nbr, proj_rel, depth_values, projection, origin, int(height), int(width)

    def _voxel_points(self, origin: Tensor, device) -> Tensor:
        """get_points (mvsdet.py:1316) depends on the grid and the scene origin only: kept on the device per origin."""
        key = (tuple(float(v) for v in origin.tolist()), str(device))
        pts = self._points_cache.get(key)
        if pts is None:
            pts = F_.get_points(n_voxels=torch.tensor(self.n_voxels), voxel_size=torch.tensor(self.voxel_size),
                                origin=origin).to(device)
            while len(self._points_cache) >= 64:          # least recently used first; a dropped tensor that is still being
                self._points_cache.pop(next(iter(self._points_cache)))   # read is protected by record_stream (worker.get)
        else:
            self._points_cache.pop(key)
        self._points_cache[key] = pts
        return pts

    # ---- the hot path -------------------------------------------------------------------------------------
    def sweep_geometry_async(self, geo: SceneGeometry, H: int, W: int, events: bool = False):
        """The sweep geometry (footprint boxes and runs: plane_sweep_coords_kernel, VALU-bound) enqueued on a side stream,
        so that it runs beside the feature packing (memory-bound) instead of in front of the sweep.  Returns
        (table, event[, start, end timing events]); `cost_volume_tabled` waits for the event on the current stream."""
        dev = geo.proj_rel.device
        cur = torch.cuda.current_stream(dev)
        side = self._geo_streams.get(str(dev))
        if side is None:
            side = self._geo_streams[str(dev)] = torch.cuda.Stream(device=dev)
        side.wait_stream(cur)   # proj_rel / depth_values may have been produced on the current stream
        with torch.cuda.stream(side):
            t0 = t1 = None
            if events:   # bench.py: timing events on the stream the kernel launches on
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record(side)
            pitch = self.variance_row_pitch(W)
            # forward only: the pooled geometry (a footprint box may take the other neighbour's idle LDS slot)
            table = ops.plane_sweep_table_pooled(geo.proj_rel, geo.depth_values, H, W, pitch if pitch != W else 0)
            if events:
                t1.record(side)
            done = torch.cuda.Event()
            done.record(side)
        table.record_stream(cur)   # allocated under the side stream, consumed on the current one
        return (table, done, t0, t1) if events else (table, done)

    def _consumer_reads_strided(self) -> bool:
        """A pitched volume is a non-contiguous view: a consumer that calls `.view` on it raises, one that calls `.reshape` /
        `.contiguous` silently copies gigabytes.  Only None (the caller gets `variance` back and the stand-in logits are used)
        and this package's cost network, which reads pitched rows in place, are known to be safe."""
        from .costreg import CostRegNet3DGS
        return self.cost_regularization is None or isinstance(self.cost_regularization, CostRegNet3DGS)

    def variance_row_pitch(self, W: int) -> int:
        """Row pitch (elements) of the variance volume `forward_scene` produces for maps of width W (W itself: contiguous)."""
        if (self.pitched_variance == "auto" and W % 32 != 0 and W % 16 == 0 and self.num_depth >= 48
                and self._consumer_reads_strided()):
            return ops.sweep_row_pitch(W)
        return int(W)

    def cost_volume_tabled(self, packed: Tensor, geo: SceneGeometry, table_and_event, C: int, H: int, W: int) -> Tensor:
        """a3+a4 from the packed maps and a geometry built by `sweep_geometry_async` (forward only)."""
        table, done = table_and_event
        torch.cuda.current_stream(packed.device).wait_event(done)
        pitch = self.variance_row_pitch(W)
        if pitch != W:   # the geometry was built for this pitch (sweep_geometry_async)
            return ops.plane_sweep_variance_tabled_pitched(packed, geo.neighbor_ids, table, C, self.num_depth, H, W, pitch)
        return ops.plane_sweep_variance_tabled(packed, geo.neighbor_ids, table, C, self.num_depth, H, W)

    def cost_volume(self, feature: Tensor, geo: SceneGeometry, packed: Optional[Tensor] = None,
                    depth: Optional[Tensor] = None) -> Tensor:
        """a3+a4, mvsdet.py:439-467 -> variance (N,C,D,Hf,Wf).  `depth` (N,D,Hf,Wf): per-pixel depth hypotheses instead of the
        scene's planes (homo_warping's 4-D depth_values, module.py:130-133: the sweep of a refinement stage)."""
        if depth is not None:
            if packed is not None and not (feature.requires_grad and torch.is_grad_enabled()):
                return ops.plane_sweep_variance_pixel_packed(packed, geo.neighbor_ids, geo.proj_rel, depth, feature.shape[1])
            return ops.plane_sweep_variance_pixel(feature, geo.neighbor_ids, geo.proj_rel, depth)
        if packed is not None and not (feature.requires_grad and torch.is_grad_enabled()):
            n, c, h, w = feature.shape
            return ops.plane_sweep_variance_packed(packed, geo.neighbor_ids, geo.proj_rel, geo.depth_values, c, h, w)
        return ops.plane_sweep_variance(feature, geo.neighbor_ids, geo.proj_rel, geo.depth_values)

    def cost_volume_chunks(self, packed: Tensor, geo: SceneGeometry, C: int, H: int, W: int, views_per_chunk: int,
                           half_out: bool = False, events: Optional[list] = None):
        """a3+a4 for cost volumes that do not fit HBM whole (BASELINE configs[4]: 503 GB in fp16): yields
        `(first_view, variance rows (M,C,D,H,W))` chunk by chunk; the consumer (the cost regularisation network)
        finishes with a chunk and drops it before the next one is produced.  Rows are those of `cost_volume`
        (bit-identical in fp32; the same values rounded to float16 with `half_out`).  Forward only.
        `events`: optional list receiving a (start, end) HIP-event pair per launch (bench.py)."""
        n_src = geo.neighbor_ids.shape[0]
        if views_per_chunk < 1:
            raise ValueError("views_per_chunk must be >= 1")
        for first in range(0, n_src, views_per_chunk):
            sl = slice(first, min(n_src, first + views_per_chunk))
            if events is not None:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
            var = ops.plane_sweep_variance_shard(packed, geo.neighbor_ids[sl], geo.proj_rel[sl], geo.depth_values[sl],
                                                 n_src, first, C, H, W, half_out)
            if events is not None:
                e1.record()
                events.append((e0, e1))
            yield first, var
            del var

    def depth_distribution(self, cost_logits: Tensor):
        """a5-a7 on the (N,2,D,H,W) output of the cost regularisation network (mvsdet.py:470-482)."""
        cost_reg, off_logit = cost_logits[:, 0], cost_logits[:, 1]
        return ops.depth_prob_topk(cost_reg, off_logit, float(self.near_far_range[0]), float(self.depth_interval),
                                   self.topk)

    def lift(self, feature: Tensor, packed: Tensor, geo: SceneGeometry, est_depth: Tensor, est_dens: Tensor):
        """a9+a10, mvsdet.py:499-515 -> volume_mean (C,X,Y,Z), valid count (1,X,Y,Z) int64."""
        n, c, hf, wf = feature.shape
        h, w = geo.height, geo.width
        mean, count = ops.backproject_weigh_mean(feature[:, :, :h, :w], packed, geo.points, geo.projection,
                                                 est_depth[:, :, :h, :w], est_dens[:, :, :h, :w], hf, wf,
                                                 float(self.voxel_size[-1]))
        nx, ny, nz = self.n_voxels
        return mean.view(c, nx, ny, nz), count.view(1, nx, ny, nz).long()

    def lift_packed(self, packed: Tensor, geo: SceneGeometry, est_depth: Tensor, est_dens: Tensor, C: int, Hf: int,
                    Wf: int):
        """a9+a10 from the packed maps alone (fp16 feature maps have no fp32 NCHW form to hand to `lift`):
        un-normalised sum over all views + count, then the mvsdet.py:511-515 division.  Forward only."""
        n_src = geo.neighbor_ids.shape[0]
        h, w = geo.height, geo.width
        total, count = ops.backproject_weigh_sum_shard(packed, geo.points, geo.projection, est_depth[:, :, :h, :w],
                                                       est_dens[:, :, :h, :w], n_src, 0, C, Hf, Wf,
                                                       float(self.voxel_size[-1]))
        mean = torch.where(count > 0, total / (count.to(total.dtype) + 1e-8), torch.zeros((), device=total.device))
        nx, ny, nz = self.n_voxels
        return mean.view(C, nx, ny, nz), count.view(1, nx, ny, nz).long()

    def _front(self, feature: Tensor, img_meta: dict, cost_logits: Optional[Tensor], geo: Optional[SceneGeometry],
               net_streams: Optional[int] = None, packed: Optional[Tensor] = None):
        """a1..a4 and the cost network of one scene on the caller's stream -> (geo, packed, variance, cost_logits).
        net_streams: CostRegNet3DGS.view_streams for this call (None: the module's own setting).
        packed: the packed maps of `feature` where the caller has them already (`forward_scene_from_stages`: the pyramid's 3x3
        kernel wrote them); used by the inference branch only, in place of its packing launch."""
        if geo is None:
            geo = self.prepare_scene(img_meta, feature.device)
        if feature.is_cuda and not (feature.requires_grad and torch.is_grad_enabled()) and geo.neighbor_ids.shape[1] > 0:
            n, c, h_, w_ = feature.shape
            tab = self.sweep_geometry_async(geo, h_, w_)     # side stream: beside the packing
            if packed is None:
                packed = ops.pack_features(feature.detach())
            variance = self.cost_volume_tabled(packed, geo, tab, c, h_, w_)
        elif feature.is_cuda and feature.requires_grad and torch.is_grad_enabled() and geo.neighbor_ids.shape[1] > 0:
            # training: ONE packing pass and ONE geometry for the forward sweep, the lifting and the backward sweep
            variance, packed, _ = ops.plane_sweep_variance_keep(feature, geo.neighbor_ids, geo.proj_rel, geo.depth_values)
        else:
            packed = ops.pack_features(feature.detach())
            variance = self.cost_volume(feature, geo, packed)
        if self.cost_regularization is not None:
            net = self.cost_regularization
            halves = getattr(net, "view_streams", 1)
            keep = halves if net_streams is None or torch.is_grad_enabled() else int(net_streams)
            if keep != halves:
                # the previous scene's neck and head are running beside this network on their own stream: a second stream
                # INSIDE the network (CostRegNet3DGS.view_streams: 89.5 -> 90.4 scenes/s alone) then takes from them what it
                # gives (pipelined 97 against 99-103 scenes/s on one box at 40 views)
                net.view_streams = keep
                try:
                    cost_logits = net(variance)
                finally:
                    net.view_streams = halves
            else:
                cost_logits = net(variance)
        elif cost_logits is None:
            raise ValueError("forward_scene needs `cost_logits` when no cost_regularization module is set")
        return geo, packed, variance, cost_logits

    def _lift_tail(self, feature, geo, packed, variance, cost_logits, gt_depth: Optional[Tensor] = None) -> "SceneOutputs":
        """a5..a10 of one scene (mvsdet.py:470-515) on the current stream; with `gt_depth` the depth diagnostics of the lifting
        block (the gt_depth branch of backproject_Weigh, :1435-1484) behind them, on the same stream."""
        prob, off, est_depth, est_dens, est_idx, avg_depth = self.depth_distribution(cost_logits)
        volume_mean, valid = self.lift(feature, packed, geo, est_depth, est_dens)
        h, w = geo.height, geo.width
        out = SceneOutputs(volume=volume_mean, valid=valid, variance=variance, prob_volume=prob, off_pred=off,
                         est_depth=est_depth[:, :, :h, :w], est_densities=est_dens[:, :, :h, :w],
                         depth_coding=avg_depth[:, :h, :w].unsqueeze(1), geometry=geo,
                         # mvsdet.py:582 `opacity = torch.max(prob_volume, dim=1)[0]`: the first of the sorted top-k values IS
                         # that maximum (the depth-distribution kernel has it in registers); uncropped like prob_volume
                         opacity=est_dens[:, 0])
        if gt_depth is not None:
            gap, rmse, per_view, gt_resized = F_.depth_diagnostics(geo.points, geo.projection, est_depth[:, :, :h, :w],
                                                                   est_dens[:, :, :h, :w], avg_depth[:, :h, :w], gt_depth,
                                                                   float(self.voxel_size[-1]))
            out._put("weight_gap", gap)                 # predictions[i].weight_gap / .src_rmse of MVSDet.predict (:1054-1058)
            out._put("src_rmse", rmse)
            out._put("depth_diagnostics", per_view)     # (N,4) {gap_i, orig_gap, new_gap, n_reduce} (:1473-1479)
            out._put("gt_depth_resized", gt_resized)
        return out

    def depth_loss(self, outputs, gt_depth) -> dict:
        """`loss_depth` of MVSDet.loss (mvsdet.py:771-843, depth_loss_func_new :893-915) for one `SceneOutputs` and its ground
        truth (N,Hg,Wg), or a sequence of them and the matching depths -> dict(loss_depth=...).  The estimate is
        outputs["depth_coding"] (N,1,h,w) -- what the reference meant to collect in `est_depth_crop` -- so the gradient reaches
        the cost network through depth_prob_topk's backward (its g_avg)."""
        if isinstance(outputs, Mapping):
            outputs, gt_depth = [outputs], [gt_depth]
        return F_.depth_loss_func_new([o["depth_coding"] for o in outputs], list(gt_depth))

    def photometric_loss(self, outputs, images, img_meta, ref_id=None) -> dict:
        """`loss_pc`, the self-supervised photometric consistency term the reference ships commented out (mvsdet.py:687-692, 838-839;
        warp_img :701-768, photometric_loss :845-874), for one `SceneOutputs` with its images (N,3,Hi,Wi) in [0,1] and its img_meta,
        or sequences of them -> dict(loss_pc=...).  The depth is outputs["depth_coding"] (N,1,h,w), so the gradient reaches the cost
        network through depth_prob_topk's backward (its g_avg) -- through the sample position, no ground-truth depth involved.
        Neighbours come from the scene's geometry, world-to-camera matrices and feature-level intrinsics from img_meta as
        `forward_scene` derives them.  `ref_id` fixes the chosen views (None: torch.randperm on the CPU, at most 10, as the reference)."""
        if isinstance(outputs, Mapping):
            outputs, images, img_meta, ref_id = [outputs], [images], [img_meta], [ref_id]
        elif ref_id is None:
            ref_id = [None] * len(outputs)
        if not (len(outputs) == len(images) == len(img_meta) == len(ref_id)):
            raise ValueError(f"photometric_loss: {len(outputs)} scenes, {len(images)} image stacks, {len(img_meta)} metas, {len(ref_id)} selections")
        warped, masks, refs = [], [], []
        for out, img, meta, rid in zip(outputs, images, img_meta, ref_id):
            depth = out["depth_coding"]
            w2c, K_feat = self._feature_cameras(meta)
            w2c, K_feat = w2c.float(), K_feat.float()
            if depth.is_cuda:
                w2c, K_feat = (ops._common.to_device(t, depth.device) for t in (w2c, K_feat))
            wv, mv, rv = F_.warp_img(img, out["geometry"].neighbor_ids, w2c, K_feat, depth, ref_id=rid)
            warped.append(wv)
            masks.append(mv)
            refs.append(rv)
        return F_.photometric_loss(warped, masks, refs)

    # ---- the NVS branch (mvsdet.py:518-677, 878-890) -------------------------------------------------
    def render_source_ids(self, img_meta: dict, tgt_c2w, num_select: int = 3) -> Tensor:
        """mvsdet.py:532-535: the `num_select` nearest source views of every target view, unique and ascending -> (n_src) int64 on
        the host.  tgt_c2w (n_tgt,4,4) camera-to-world, array or tensor.  The poses are host data (img_meta), so the `unique` here
        costs no device synchronisation."""
        w2c, _ = self._feature_cameras(img_meta)
        src_c2w = w2c.inverse()
        tgt = torch.as_tensor(np.asarray(tgt_c2w.detach().cpu() if isinstance(tgt_c2w, Tensor) else tgt_c2w)).to(src_c2w.dtype)
        ids = F_.get_nearest_pose_ids(tgt, src_c2w, num_select=num_select, maskself=False)
        return torch.unique(ids.reshape(-1))

    def novel_views(self, outputs, feature: Tensor, img_meta: dict, to_gaussians, tgt_c2w, tgt_intrinsic, tgt_shape, rgb_raw=None, *,
                    num_surfaces: int = 1, gaussian_scale_min: float = 0.5, gaussian_scale_max: float = 15.0, sh_degree: int = 4,
                    num_select: int = 3, sh_rotation=None, background_color=None, max_keys=None, depth_mode=None,
                    gaussian_head: str = "torch", denorm_images=None):
        """The novel-view branch of extract_feat for one scene (mvsdet.py:519-677) -> colour (1,n_tgt,3,H,W), what
        `self.decoder.forward(...)` returns as `.color`.  outputs: the scene's `SceneOutputs`; feature (N,C,Hf,Wf); to_gaussians:
        the caller's nn.Sequential(ReLU, Linear) with num_surfaces * (2 + 7 + 3 d_sh) outputs, run by torch; tgt_c2w (n_tgt,4,4),
        tgt_intrinsic (4,4) or (n_tgt,4,4) in pixels of the target image, tgt_shape (H, W, ...); rgb_raw (n_src,R,3) or (1,n_src,R,3):
        what process_rgb_raw returns for `use_rgb_gaussian` (the resize stays with the caller).  Source views by `render_source_ids`;
        feature rows, depth_coding and rgb_raw are concatenated as :561-569; opacity is the largest probability (:581-582); the depth
        along the ray is depth_coding / (depth_scale + 1e-8) (:583); then `functional.pixel_gaussians` and
        `functional.decode_splatting` with near / far = near_far_range.  Gradients reach feature, to_gaussians' parameters, depth_coding
        and the opacity.  The scale / degree defaults are those of the shipped configs.  depth_mode: one of
        `functional.render_depth_cuda`'s modes -> (colour, depth (1,n_tgt,H,W)), the decoder's `.depth`, from the same fused
        rasteriser call; the depth carries gradients to the same places.
        gaussian_head "torch" (default): the rows are concatenated and to_gaussians is run by torch, as above.  "hip": to_gaussians must
        be nn.Sequential(ReLU, Linear); its weight and bias go to `functional.gaussian_head`, which reads feature, depth_coding and the
        rgb in place (one kernel, no row matrix).  denorm_images (N,3,Hi,Wi): the denormalised images instead of rgb_raw
        (never both) -- "hip" reduces them inside the kernel, "torch" through `functional.process_rgb_raw` (ratio 4 only)."""
        if gaussian_head not in ("torch", "hip"):
            raise ValueError(f"novel_views: gaussian_head = {gaussian_head!r} (\"torch\" or \"hip\")")
        if rgb_raw is not None and denorm_images is not None:
            raise ValueError("novel_views: rgb comes as rgb_raw or as denorm_images, not both")
        geo = outputs["geometry"]
        h, w = geo.height, geo.width
        dev = feature.device
        src_id = self.render_source_ids(img_meta, tgt_c2w, num_select)
        n_src, R = int(src_id.numel()), h * w
        w2c, K_feat = self._feature_cameras(img_meta)
        K = K_feat.clone().float()
        if K.dim() == 2:                                   # one intrinsic matrix for all views (ScanNet), :546-548
            K[0] /= w
            K[1] /= h
            K = K[None, :3, :3].repeat(n_src, 1, 1)
        else:                                              # per view (ARKitScenes), :551-553
            K[:, 0] /= w
            K[:, 1] /= h
            K = K[src_id, :3, :3]
        c2w = w2c.inverse().float()[src_id]
        ids, K, c2w = (ops._common.to_device(t, dev) for t in (src_id, K.contiguous(), c2w.contiguous()))
        depth_coding = outputs["depth_coding"]
        if gaussian_head == "hip":
            raw = self._gaussian_head_hip(to_gaussians, feature, depth_coding, ids, h, w, int(num_surfaces), rgb_raw, denorm_images)
        else:
            if denorm_images is not None:
                rgb_raw = F_.process_rgb_raw(denorm_images, 4, h, w, ids)
            rows = [feature[ids][:, :, :h, :w].reshape(n_src, feature.shape[1], R).transpose(1, 2), depth_coding[ids].reshape(n_src, R, 1)]
            if rgb_raw is not None:
                rows.append(rgb_raw.reshape(n_src, R, 3).to(rows[0].dtype))
            raw = to_gaussians(torch.cat(rows, dim=-1))
            raw = raw.reshape(n_src, R, int(num_surfaces), raw.shape[-1] // int(num_surfaces))
        opacity = outputs["opacity"][ids][:, :h, :w].reshape(n_src, R)
        # compute_depth_scale[_MultiIntrin] (:1158-1216) through the kernel of `ray_depth`, without candidates
        Kp = torch.tensor(np.array(img_meta["lidar2img"]["intrinsic"])).clone()
        ratio = img_meta["ori_shape"][0] / (img_meta["img_shape"][0] / self.stride)
        if Kp.dim() == 2:
            Kp[:2] /= ratio
            Kp = Kp.unsqueeze(0).repeat(feature.shape[0], 1, 1)
        else:
            Kp[:, :2] /= ratio
        intr = torch.stack([Kp[:, 0, 0], Kp[:, 1, 1], Kp[:, 0, 2], Kp[:, 1, 2], Kp[:, 0, 1]], dim=1).float()
        scale, _ = ops.ray_depth(ops._common.to_device(intr, dev), None, int(h), int(w))
        ray = (depth_coding.reshape(feature.shape[0], R, 1) / (scale + 1e-8))[ids].reshape(n_src, R)
        gaussians = F_.pixel_gaussians(c2w, K, raw, ray, opacity, (h, w), gaussian_scale_min, gaussian_scale_max, sh_degree,
                                       sh_rotation=sh_rotation)
        # the target cameras (:645-662)
        H, W = int(tgt_shape[0]), int(tgt_shape[1])
        tgt = torch.as_tensor(np.asarray(tgt_c2w.detach().cpu() if isinstance(tgt_c2w, Tensor) else tgt_c2w)).float()
        Kt = torch.as_tensor(np.asarray(tgt_intrinsic.detach().cpu() if isinstance(tgt_intrinsic, Tensor) else tgt_intrinsic)).float().clone()
        n_tgt = tgt.shape[0]
        if Kt.dim() == 2:
            Kt = Kt[None].repeat(n_tgt, 1, 1)
        Kt[:, 0] /= W
        Kt[:, 1] /= H
        near = torch.full((1, n_tgt), self.near_far_range[0])
        far = torch.full((1, n_tgt), self.near_far_range[1])
        tgt, Kt, near, far = (ops._common.to_device(t, dev) for t in (tgt[None].contiguous(), Kt[None, :, :3, :3].contiguous(), near, far))
        return F_.decode_splatting(gaussians, tgt, Kt, near, far, (H, W), background_color, max_keys=max_keys, depth_mode=depth_mode)

    @staticmethod
    def _gaussian_head_hip(to_gaussians, feature, depth_coding, ids, h, w, num_surfaces, rgb_raw, denorm_images):
        """`to_gaussians` on the kernel of `functional.gaussian_head`; TypeError unless it is ReLU followed by a Linear of the rows' width."""
        layers = list(to_gaussians) if isinstance(to_gaussians, torch.nn.Sequential) else []
        want = feature.shape[1] + (1 if rgb_raw is None and denorm_images is None else 4)
        if len(layers) != 2 or not isinstance(layers[0], torch.nn.ReLU) or not isinstance(layers[1], torch.nn.Linear):
            raise TypeError(f"novel_views(gaussian_head=\"hip\"): to_gaussians must be nn.Sequential(nn.ReLU(), nn.Linear(...)), got {to_gaussians!r}")
        linear = layers[1]
        if linear.in_features != want or linear.bias is None:
            raise TypeError(f"novel_views(gaussian_head=\"hip\"): the rows have {want} entries ({feature.shape[1]} feature channels, depth_coding"
                            f"{'' if want == feature.shape[1] + 1 else ', rgb'}); to_gaussians[1] is {linear!r} and must have a bias")
        return F_.gaussian_head(feature, depth_coding, linear.weight, linear.bias, ids, h, w, num_surfaces, rgb_raw, denorm_images)

    def nvs_loss(self, rgb_preds, gt_rgb) -> dict:
        """`loss_nvs` of MVSDet.loss (nvs_loss_func, mvsdet.py:878-890, without use_nerf_mask): rgb_preds, one colour (1,n_tgt,3,H,W)
        per scene as `novel_views` returns it (or one tensor), gt_rgb the matching (n_tgt,3,H,W) in [0,1] -> dict(loss_nvs=...)."""
        if isinstance(rgb_preds, Tensor):
            rgb_preds, gt_rgb = [rgb_preds], [gt_rgb]
        return F_.nvs_loss_func(list(rgb_preds), list(gt_rgb))

    def nvs_scores(self, rgb_preds, gt_rgb, evaluator=None, depth_preds=None, gt_depth=None) -> dict:
        """What the reference's test loop stores for a scene (mvsdet.py:1017-1040: save_rendered_img_Image, and save_rendered_depth
        where a rendered depth exists): rgb_preds, the scene's colour (1,n_tgt,3,H,W) as `novel_views` returns it (or (n_tgt,3,H,W)),
        gt_rgb the matching (n_tgt,3,H,W) in [0,1] -> dict(psnr=, ssim=, rmse=) as 0-dim float64 device tensors, the means over the
        target views.  depth_preds (1,n_tgt,H,W) as `novel_views(depth_mode=...)` returns it (or (n_tgt,H,W)) with gt_depth
        (n_tgt,H,W): rmse is then what `functional.save_rendered_depth` gives for the pair; without the pair it is 0 (the shipped
        configs render no depth).  evaluator: an `evaluation.NVSEvaluator` that is fed the scene (it then scores it; no second
        launch).  No host synchronisation."""
        if not isinstance(rgb_preds, Tensor):
            if len(rgb_preds) != 1:
                raise ValueError(f"nvs_scores: one scene at a time (got {len(rgb_preds)}); NVSEvaluator.update takes lists")
            rgb_preds, gt_rgb = rgb_preds[0], gt_rgb if isinstance(gt_rgb, Tensor) else gt_rgb[0]
        rgb = rgb_preds[0] if rgb_preds.dim() == 5 else rgb_preds
        if (depth_preds is None) != (gt_depth is None):
            raise ValueError("nvs_scores: depth_preds and gt_depth come as a pair")
        if depth_preds is not None:
            if not isinstance(depth_preds, Tensor):
                depth_preds, gt_depth = depth_preds[0], gt_depth if isinstance(gt_depth, Tensor) else gt_depth[0]
            depth_preds = depth_preds[0] if depth_preds.dim() == 4 else depth_preds
        if evaluator is not None:
            evaluator.update(rgb, gt_rgb, depth_preds, gt_depth)
            scene = evaluator.last_scene
        else:
            scene = ops.nvsmetric.nvs_score(None, rgb, gt_rgb, depth_preds, gt_depth)[1]
        return dict(psnr=scene[0], ssim=scene[1], rmse=scene[2])

    # name -> (detector tail on the side stream, view streams of the cost network beside it; None = the module's own setting)
    OVERLAP_ROUTES = {"one": (False, None), "side1": (True, 1), "side2": (True, 2)}
    _TUNE_WARM, _TUNE_SPAN = 2, 4    # scenes of a route left out (the previous route drains), scenes measured

    def _route(self, feature: Tensor, cost_logits: Optional[Tensor]):
        """(route name, side stream?, network streams, tuning state or None) for this call."""
        mode = self.overlap_detector
        grad = torch.is_grad_enabled() and (feature.requires_grad or (cost_logits is not None and cost_logits.requires_grad)
                                            or any(p.requires_grad for p in getattr(self.cost_regularization, "parameters", lambda: ())()))
        if not mode or not feature.is_cuda or grad:
            return "one", False, None, None          # autograd: the backward's stream order is left to the ops' own streams
        if mode != "auto":
            return "side", True, int(self.overlap_network_streams), None
        key = (tuple(feature.shape), self.num_depth, str(feature.device))
        st = self._overlap_tuning.get(key)
        if st is None:
            st = self._overlap_tuning[key] = {"cand": 0, "marks": [], "side_marks": [], "spans": {}, "choice": None, "periods_ms": None}
        names = list(self.OVERLAP_ROUTES)
        if st["choice"] is None and len(st["spans"]) == len(names) and all(e.query() for sp in st["spans"].values() for e in sp[1::2]):
            # a route's period: the slower of its two streams (the tails must keep up with the fronts)
            per = {k: max(sp[i].elapsed_time(sp[i + 1]) for i in range(0, len(sp), 2)) / self._TUNE_SPAN for k, sp in st["spans"].items()}
            best_side = min((k for k in names if k != "one"), key=lambda k: per[k])
            st["choice"] = best_side if per[best_side] < 0.99 * per["one"] else "one"
            st["periods_ms"] = {k: round(v, 4) for k, v in per.items()}
        name = st["choice"] or names[min(st["cand"], len(names) - 1)]
        side, streams = self.OVERLAP_ROUTES[name]
        return name, side, streams, (st if st["choice"] is None or st["choice"] != "one" else None)

    _WATCH_SPAN = 8      # scenes per check of a kept side route

    def _watch(self, st: dict, device, side_done=None) -> None:
        """A kept side route stays under watch: its period over every `_WATCH_SPAN` scenes (the slower of the two streams, from
        events, no host wait) against the period `one` was measured at.  Two windows in a row more than 3 % behind it and the
        shape goes back to `one` for good (`overlap_choice` then says so): the routes were compared over a few scenes, and what
        shares the device's hardware queues with them can change afterwards."""
        w = st.setdefault("watch", {"main": [], "side": [], "strikes": 0})
        if side_done is not None:
            w["side"].append(side_done)
            return
        ev = torch.cuda.Event(enable_timing=True)
        ev.record(torch.cuda.current_stream(device))
        w["main"].append(ev)
        n = self._WATCH_SPAN + 1
        if len(w["main"]) >= 2 * n and len(w["side"]) >= 2 * n - 1:
            # the OLDER window: its events have long completed (query() guards it; a window still in flight is looked at later)
            m, sd = w["main"][:n], w["side"][:n]
            if m[-1].query() and sd[-1].query():
                period = max(m[0].elapsed_time(m[-1]), sd[0].elapsed_time(sd[-1])) / self._WATCH_SPAN
                w["strikes"] = w["strikes"] + 1 if period > 1.03 * st["periods_ms"]["one"] else 0
                st["watched_period_ms"] = round(period, 4)
                if w["strikes"] >= 2:
                    st["demoted_from"] = st["choice"]
                    st["choice"] = "one"
                del w["main"][:n - 1], w["side"][:n - 1]

    def _tune_mark(self, st: dict, name: str, device, side_done=None) -> None:
        """Timing events of a tuning scene: one behind its cost network on the caller's stream (side_done is None), one behind
        its tail on the side stream."""
        if name in st["spans"]:
            return                                   # every route has been run; waiting for the events to complete
        if side_done is not None:
            st["side_marks"].append(side_done)
        else:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record(torch.cuda.current_stream(device))
            st["marks"].append(ev)
        full = self._TUNE_WARM + self._TUNE_SPAN + 1
        if len(st["marks"]) == full and len(st["side_marks"]) in (0, full):
            span = (st["marks"][self._TUNE_WARM], st["marks"][-1])
            if st["side_marks"]:
                span += (st["side_marks"][self._TUNE_WARM], st["side_marks"][-1])
            st["spans"][name] = span
            st["marks"], st["side_marks"] = [], []
            st["cand"] += 1

    def overlap_choice(self, feature_shape, device="cuda:0"):
        """What `overlap_detector = "auto"` decided for scenes of this feature shape: (route name or None while it is still
        measuring, {route: ms per scene} or None)."""
        st = self._overlap_tuning.get((tuple(feature_shape), self.num_depth, str(torch.device(device))))
        return (None, None) if st is None else (st["choice"], st["periods_ms"])

    def _side_stream(self, dev):
        side = self._detector_streams.get(str(dev))
        if side is None:
            side = self._detector_streams[str(dev)] = torch.cuda.Stream(device=dev)
        return side

    @staticmethod
    def _keep_for(side, *values):
        """Inputs of a side-stream tail that live in another stream's pool must not be recycled while the side stream reads them."""
        for t in values:
            if isinstance(t, Tensor) and t.is_cuda:
                t.record_stream(side)

    def _detections(self, head_out, valid: Tensor, img_metas):
        """predict_by_feat's padded device result (head.predict_head_maps) of the head's maps; the ARKit head's through its
        rotated NMS (7-wide boxes, class-major)."""
        from .head import predict_head_maps
        return predict_head_maps(*head_out, valid, img_metas, self.test_cfg, rotated=bool(getattr(self.bbox_head, "arkit_head", False)))

    def forward_scene(self, feature: Tensor, img_meta: dict, cost_logits: Optional[Tensor] = None,
                      geo: Optional[SceneGeometry] = None, gt_depth: Optional[Tensor] = None) -> dict:
        """One scene through a1..a10.  `cost_logits` (N,2,D,Hf,Wf) stands in for the cost regularisation
        network's output when `self.cost_regularization` is None (benchmarks / parity tests).
        With `pitched_variance = "auto"` (default) `out["variance"]` may be a NON-CONTIGUOUS (N,C,D,H,W) view of a buffer whose
        rows are `variance_row_pitch(W)` elements apart (same values; only for widths 16 mod 32 with 48+ planes, and only when
        the consumer is None or `CostRegNet3DGS`): `.view()` on it raises; set `pitched_variance = False` for a contiguous one.
        The result is a `SceneOutputs`: with `overlap_detector` a value read from it makes the reading stream wait for the side
        stream's event first.
        `gt_depth` (N,Hg,Wg), any size: the result gains `weight_gap` and `src_rmse` (0-dim device tensors: what the reference's
        backproject_Weigh returns with gt_depth), `depth_diagnostics` (N,4) {gap_i, orig_gap, new_gap, n_reduce} per view and
        `gt_depth_resized` (N,h,w); they are made in the tail, on the stream the lifting runs on.  None: no such key."""
        return self._scene(feature, img_meta, cost_logits, geo, gt_depth)

    def forward_scene_from_stages(self, stages: Sequence[Tensor], img_meta: dict, **kw) -> dict:
        """`forward_scene` from the four backbone maps instead of the pyramid's output: `self.fpn` (an `mvsdet_amd.fpn.FPNLevel0`)
        makes the feature map AND its packed form -- on its HIP route the 3x3 kernel's epilogue writes both -- and the scene path
        sweeps that packed tensor instead of launching `ops.pack_features`.  Keyword arguments as `forward_scene`'s.  The result
        gains `feature`, the (N,256,H0,W0) map."""
        if self.fpn is None:
            raise ValueError("forward_scene_from_stages needs `fpn` (MVSDetHotPath.fpn = FPNLevel0.from_module(model.neck))")
        feature, packed = self.fpn(stages, packed=True)
        out = self._scene(feature, img_meta, kw.pop("cost_logits", None), kw.pop("geo", None), kw.pop("gt_depth", None), packed, **kw)
        out._put("feature", feature)
        return out

    def forward_scene_from_images(self, img: Tensor, img_meta: dict, **kw) -> dict:
        """`forward_scene_from_stages` from the images (N,3,H,W): `self.backbone` (an `mvsdet_amd.resnet.ResNetStages`) makes the four
        maps C2..C5 that `self.fpn` takes.  Keyword arguments as `forward_scene`'s.  The result gains `stages`, the tuple of maps."""
        if self.backbone is None or self.fpn is None:
            raise ValueError("forward_scene_from_images needs `backbone` and `fpn` (MVSDetHotPath.backbone = "
                             "ResNetStages.from_module(model.backbone), MVSDetHotPath.fpn = FPNLevel0.from_module(model.neck))")
        stages = self.backbone(img)
        out = self.forward_scene_from_stages(stages, img_meta, **kw)
        out._put("stages", stages)
        return out

    def _scene(self, feature: Tensor, img_meta: dict, cost_logits: Optional[Tensor], geo: Optional[SceneGeometry],
               gt_depth: Optional[Tensor], packed: Optional[Tensor] = None) -> dict:
        """`forward_scene`; packed: `_front`'s."""
        route, on_side, net_streams, tuning = self._route(feature, cost_logits)
        watching = tuning is not None and tuning["choice"] is not None   # a kept side route: `_watch`
        geo, packed, variance, cost_logits = self._front(feature, img_meta, cost_logits, geo, net_streams, packed)
        if watching:
            self._watch(tuning, variance.device)
        elif tuning is not None:
            self._tune_mark(tuning, route, variance.device)

        def tail():
            out = self._lift_tail(feature, geo, packed, variance, cost_logits, gt_depth)
            if self.neck_3d is not None:   # the reference stacks the scenes of a batch first (batch_size = 1 per GPU): forward_scenes
                out._put("neck", self.neck_3d(out.raw("volume").unsqueeze(0)))
                if self.bbox_head is not None:
                    out._put("head", self.bbox_head(out.raw("neck")))   # (centerness, bbox, cls) lists over the levels
                    if self.test_cfg is not None:
                        out._put("detections", self._detections(out.raw("head"), out.raw("valid").unsqueeze(0), [img_meta]))
            return out

        if not on_side or (torch.is_grad_enabled() and cost_logits.requires_grad):
            return tail()
        # Everything behind the cost network -- depth distribution, lifting, and the neck and head when they are attached -- on a
        # stream of its own: small kernels that do not fill the chip (one thread per pixel; ONE 40 x 40 x 16 volume: 200 blocks for
        # 256 CUs at the neck's largest level) run beside the NEXT scene's packing, sweep and first convolution instead of in
        # front of them.  Reading a value from the returned SceneOutputs makes the reading stream wait for out["ready"].
        dev = variance.device
        cur = torch.cuda.current_stream(dev)
        side = self._side_stream(dev)
        ready = torch.cuda.Event()
        ready.record(cur)
        with torch.cuda.stream(side):
            side.wait_event(ready)
            out = tail()
            done = torch.cuda.Event(enable_timing=tuning is not None)
            done.record(side)
        if watching:
            self._watch(tuning, dev, side_done=done)
        elif tuning is not None:
            self._tune_mark(tuning, route, dev, side_done=done)
        # (`lift` reads geo.projection -- a view of the ONE uploaded staging buffer, which neighbor_ids, proj_rel and depth_values
        # share: recording any view records the whole block -- and geo.points, a block of its own)
        self._keep_for(side, cost_logits, packed, feature, geo.projection, geo.points, gt_depth)
        out._put("ready", done)
        out._put("detector_ready", done)
        return out

    def forward_scenes(self, features: Sequence[Tensor], img_metas: Sequence[dict],
                       cost_logits: Optional[Sequence[Tensor]] = None, keep_variance: bool = False,
                       gt_depths: Optional[Sequence[Tensor]] = None) -> dict:
        """A BATCH of scenes the way mvsdet.py:681-698 runs it: every scene through a1..a10 on its own, then `neck_3d` (and
        `bbox_head`) ONCE on the stacked (B,C,X,Y,Z) volume -- one 40 x 40 x 16 volume is 200 blocks for 256 CUs at the neck's
        largest level and a few dozen at the others; a batch fills the chip (throughput runs, `samples_per_gpu` > 1).
        Returns {"scenes": [SceneOutputs per scene, each with its own rows of the batched neck / head results as views],
        "volume": (B,C,X,Y,Z), "valid": (B,1,X,Y,Z), "neck": levels of (B,...), "head": the head's lists, "ready": event}.
        With `overlap_detector` the tails and the batched detector run on the side stream beside the following scenes' sweeps
        and cost networks; values read through the returned holders wait for it.  ONE decision for the whole batch: if any
        scene has to keep its tail on the caller's stream (autograd), every tail and the detector stay there -- a detector on
        the side stream would stack volumes the caller's stream is still writing.
        A scene's `variance` (2.4 GB at the reference-true shape) is dropped as soon as its cost network has read it unless
        `keep_variance`: B of them alive until the batch returns is what would bound B.
        `gt_depths`: one (N,Hg,Wg) ground-truth depth per scene; every scene's holder then carries the keys `forward_scene`
        adds with `gt_depth`."""
        B = len(features)
        if B == 0 or len(img_metas) != B or (cost_logits is not None and len(cost_logits) != B) \
                or (gt_depths is not None and len(gt_depths) != B):
            raise ValueError("forward_scenes: one img_meta (and one cost_logits / gt_depth, if given) per feature tensor")
        dev = features[0].device
        for i in range(B):                      # the camera algebra of every scene of the batch starts now, on the worker thread
            self.prefetch_scene(img_metas[i], dev)
        grad = torch.is_grad_enabled()
        one_stream = (not (self.overlap_detector and dev.type == "cuda")
                      or (grad and (any(f.requires_grad for f in features)
                                    or (cost_logits is not None and any(c.requires_grad for c in cost_logits))
                                    or any(p.requires_grad for p in getattr(self.cost_regularization, "parameters", lambda: ())()))))
        net_streams = None if one_stream else (1 if self.overlap_detector == "auto" else int(self.overlap_network_streams))
        outs, side, cur = [], None, None
        for i in range(B):
            logits_i = None if cost_logits is None else cost_logits[i]
            gt_i = None if gt_depths is None else gt_depths[i]
            geo, packed, variance, logits_i = self._front(features[i], img_metas[i], logits_i, None, net_streams)
            if not keep_variance and not (grad and variance.requires_grad):
                variance = variance.new_empty(0)   # the holder's slot; the volume itself goes back to the allocator
            if one_stream:
                outs.append(self._lift_tail(features[i], geo, packed, variance, logits_i, gt_i))
                continue
            cur = torch.cuda.current_stream(dev)
            side = self._side_stream(dev)
            ready = torch.cuda.Event()
            ready.record(cur)
            with torch.cuda.stream(side):
                side.wait_event(ready)
                outs.append(self._lift_tail(features[i], geo, packed, variance, logits_i, gt_i))
            self._keep_for(side, logits_i, packed, features[i], geo.projection, geo.points, gt_i)

        def detector():
            res = SceneOutputs(scenes=outs)
            res._put("volume", torch.stack([o.raw("volume") for o in outs]))
            res._put("valid", torch.stack([o.raw("valid") for o in outs]))
            if self.neck_3d is not None:
                res._put("neck", self.neck_3d(res.raw("volume")))
                for i, o in enumerate(outs):
                    o._put("neck", [lvl[i:i + 1] for lvl in res.raw("neck")])
                if self.bbox_head is not None:
                    res._put("head", self.bbox_head(res.raw("neck")))
                    for i, o in enumerate(outs):
                        o._put("head", tuple([lvl[i:i + 1] for lvl in part] for part in res.raw("head")))
                    if self.test_cfg is not None:
                        res._put("detections", self._detections(res.raw("head"), res.raw("valid"), img_metas))
            return res

        if side is None:
            return detector()
        with torch.cuda.stream(side):
            res = detector()
            done = torch.cuda.Event()
            done.record(side)
        for o in outs + [res]:
            o._put("ready", done)
            o._put("detector_ready", done)
        return res
