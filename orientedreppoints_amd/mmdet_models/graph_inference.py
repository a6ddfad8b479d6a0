"""Inference of a detector as ONE hipGraph replay per call (MI355X deployment path; no counterpart in the reference,
whose test loop launches ~2000 framework kernels per image from Python).

The whole device part of `simple_test_batch` -- backbone, FPN, dense head, decode, multiclass rotated NMS, packing --
is fixed-shape and free of host synchronisation (`get_bboxes(..., static=True)`, mmdet_models/core.py), so it is
captured once for a given input shape and replayed: ~240 kernel launches become one graph launch, and the step no
longer depends on how fast the host can issue them.  Per call: one device copy of the image into the captured input
buffer, the replay, one D2H copy of the packed detections per image (`rbbox2result_packed`, what the reference's
`rbbox2result` also pays).  Results are those of `simple_test_batch`.
"""
import torch

from .. import _lib
from .core import is_scalar_scale, rbbox2result_packed


def _param_fingerprint(tensors):
    """(storage address, version) of every parameter and buffer: changes when load_state_dict / an optimizer step /
    .to() replaced or rewrote them (writes through `.data` bypass the version counter: call `recapture()` after those)."""
    fp = 0
    for t in tensors:
        fp = (fp * 1000003 + t.data_ptr() + 7919 * t._version) & 0xFFFFFFFFFFFF
    return fp


class GraphedInference(object):
    """Owns everything its graph touches: the input buffer, the packed output, the scratch (allocated from the graph's
    private memory pool while capturing: `_lib.workspace`), and references to the cached packed DeformConv / 3x3 weights
    and folded BatchNorm affines the captured kernels read (`_lib.keep_for_graph`) -- so no later eager call (a large
    merge NMS growing the shared scratch, the capacity-overflow fallback, a training step, a cache eviction) can free
    or move memory a replay uses.  If the model's parameters change, the next call re-captures."""

    def __init__(self, model, img, img_metas, warmup=3, rescale=False):
        """model: an eval-mode OrientedRepPointsDetector on a GPU; img [B,3,H,W] (its shape / dtype are captured);
        img_metas: the B meta dicts used for every later call; rescale: as in `simple_test_batch(img, img_metas, rescale)` --
        boxes and rep-points divided by each meta's `scale_factor` before the NMS, inside the graph.  Raises if the path is
        not capturable (with rescale: a per-axis `scale_factor`, i.e. `keep_ratio=False`)."""
        self.model, self.metas, self.rescale = model, list(img_metas), bool(rescale)
        if self.rescale and not all(is_scalar_scale(m['scale_factor']) for m in self.metas):
            raise ValueError("GraphedInference: rescale=True needs one scale factor per image (keep_ratio=True); a per-axis "
                             "scale_factor is left to simple_test_batch")
        if model.training or not img.is_cuda:
            raise ValueError("GraphedInference needs an eval-mode model and a CUDA image")
        if model.test_cfg.nms.get('type', 'rnms') != 'rnms' or not model.test_cfg.get('static_postprocess', True):
            raise ValueError("GraphedInference needs the static rnms post-processing")
        self.num_classes = model.bbox_head.num_classes
        self.static_img = img.clone()
        self.warmup = max(1, warmup)
        self.captures = 0
        self._capture()

    def _device_part(self):
        model, head = self.model, self.model.bbox_head
        outs = head(model.extract_feat(self.static_img))
        return head.get_bboxes(*(tuple(outs) + (self.metas, model.test_cfg, self.rescale)), static=True)

    @property
    def inputs(self):
        """What a device-side producer fills before a replay (`PipelinedInference.submit_device`)."""
        return self.static_img

    @property
    def device(self):
        return self.static_img.device

    def load(self, img):
        self.static_img.copy_(img, non_blocking=True)

    def decode(self, packed):
        """The packed results (device or pinned host) -> per-image result lists; an entry is None where the capacity overflowed."""
        return [rbbox2result_packed(p, self.num_classes) for p in packed]

    def fallback(self, img):
        """The reference-shaped route for a call whose static capacity overflowed."""
        with torch.no_grad():
            return self.model.simple_test_batch(img, self.metas, self.rescale)

    def _capture(self):
        dev = self.device
        self.graph = None                                     # release the previous graph (and its pool) first
        self.packed = None
        self._refs = []
        prev, _lib._keepalive = _lib._keepalive, self._refs
        try:
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side), torch.no_grad():
                for _ in range(self.warmup):                  # library algorithm selection, weight packing, BN folding
                    self._device_part()
            torch.cuda.current_stream(dev).wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            # thread_local: only this thread's calls are checked during capture (a process-group watchdog thread polling
            # its events must not abort it)
            with torch.no_grad(), torch.cuda.graph(graph, capture_error_mode="thread_local"):
                self.packed = self._device_part()
            self.graph = graph
        finally:
            _lib._keepalive = prev
        self._tensors = list(self.model.parameters()) + list(self.model.buffers())
        self._fingerprint = _param_fingerprint(self._tensors)
        self.captures += 1

    def recapture(self):
        """Force a new capture (after parameter writes the version counters do not see, e.g. through `.data`)."""
        self._capture()

    def __call__(self, img):
        """The per-image result lists of `simple_test_batch(img, img_metas, rescale)`."""
        self.load(img)
        self.graph.replay()
        # checked while the replay runs (keeps ~50 us of host work off the critical path): if the weights changed, the
        # packs / folded affines baked into the graph are stale -> capture again and redo this call
        if _param_fingerprint(self._tensors) != self._fingerprint:
            self._capture()
            self.graph.replay()
        results = self.decode(self.packed)
        if any(r is None for r in results):               # more pairs above score_thr than the static capacity holds
            return self.fallback(img)
        return results


class GraphedAugInference(GraphedInference):
    """`GraphedInference` for test-time augmentation: `model.aug_test(imgs, img_metas, rescale)` as one graph.  imgs: one
    [B, 3, H_v, W_v] tensor per view (every view has its own static input buffer; B tiles of a view share it), img_metas: per
    view the B meta dicts.  All views' forwards and, per image, one merged post-processing (`fused_postprocess_views`) are
    captured together.  `__call__(imgs)` returns, per image, `aug_test`'s per-class [k, 9] lists.  Ownership, keep-alive,
    fingerprint / recapture are `GraphedInference`'s; on overflow the call goes to `model.aug_test`."""

    def __init__(self, model, imgs, img_metas, warmup=3, rescale=True):
        self.model, self.metas, self.rescale = model, [list(m) for m in img_metas], bool(rescale)
        imgs = list(imgs)
        if len(imgs) == 0 or len(imgs) != len(self.metas) or any(len(m) != img.size(0) for img, m in zip(imgs, self.metas)):
            raise ValueError("GraphedAugInference: one image tensor and one list of metas per view, one meta per image")
        if len(set(int(img.size(0)) for img in imgs)) != 1:
            raise ValueError("GraphedAugInference: every view holds the same number of images")
        if model.training or not all(img.is_cuda for img in imgs):
            raise ValueError("GraphedAugInference needs an eval-mode model and CUDA images")
        with torch.no_grad():
            if not model.aug_static_ok(imgs[0], self.metas):
                raise ValueError("GraphedAugInference needs the fused static rnms post-processing and one scale factor per view "
                                 "(keep_ratio=True)")
        self.num_classes = model.bbox_head.num_classes
        self.static_imgs = [img.clone() for img in imgs]
        self.warmup = max(1, warmup)
        self.captures = 0
        self._capture()

    @property
    def inputs(self):
        return self.static_imgs

    @property
    def device(self):
        return self.static_imgs[0].device

    def load(self, imgs):
        for buf, img in zip(self.static_imgs, imgs):
            buf.copy_(img, non_blocking=True)

    def _device_part(self):
        model = self.model
        outs = [model.bbox_head(model.extract_feat(buf)) for buf in self.static_imgs]
        return [model.aug_postprocess_static(outs, self.metas, self.rescale, b) for b in range(self.static_imgs[0].size(0))]

    def decode(self, packed):
        return [self.model.aug_result_packed(p) for p in packed]

    def fallback(self, imgs):
        with torch.no_grad():
            return [self.model.aug_test([img[b:b + 1] for img in imgs], [[m[b]] for m in self.metas], self.rescale)
                    for b in range(imgs[0].size(0))]


class PipelinedInference(object):
    """Throughput mode of `GraphedInference`: `depth` (default 2) captured graphs, each with its own input / output /
    scratch, replayed on their own streams with the results fetched asynchronously into pinned host buffers.  `submit(img)`
    queues an image and returns the results of the image submitted `depth` calls earlier (None while the pipe fills);
    `flush()` returns what is still in flight, oldest first.  The tail of one image (decode, NMS: many small kernels
    that leave most CUs idle) then overlaps the backbone of the next one, and the host never waits on the image it has
    just queued.  Every image still runs the complete step and produces the same detections as `GraphedInference`;
    `rescale` is passed on to it."""

    def __init__(self, model, img, img_metas, depth=2, warmup=3, _allow_half=False, rescale=False):
        dev = img[0].device if isinstance(img, (list, tuple)) else img.device
        if (depth > 2 and not _allow_half and torch.backends.cudnn.deterministic
                and any(p.dtype != torch.float32 for p in model.parameters())):
            # measured (round 6, tests/checks/half_pipeline_probe.py): with the library restricted to its reproducible solvers
            # (torch.backends.cudnn.deterministic = True) a model.half() detector replays correctly from one or two captured graphs, but
            # with FOUR in flight the device stops making progress (a replay's completion event never signals; either half-precision
            # DeformConv kernel).  In the default library mode the same model runs four deep at the fp32 model's rate (338 images/s).
            # Refused here rather than hung there.
            raise ValueError("PipelinedInference: with torch.backends.cudnn.deterministic = True a half / bfloat16 model supports at most "
                             "two graphs in flight (depth <= 2); switch the flag off or lower the depth")
        self.model, self.metas, self.depth, self.rescale = model, list(img_metas), depth, bool(rescale)
        self.num_classes = model.bbox_head.num_classes
        # with several images in flight the two towers of ONE image need no second stream (measured: 225 vs 218 img/s)
        head = model.bbox_head
        prev = getattr(head, 'tower_streams', None)
        head.tower_streams = False
        try:
            self.slots = [self._make_slot(model, img, img_metas, warmup, rescale) for _ in range(depth)]
        finally:
            head.tower_streams = prev
        self.streams = [torch.cuda.Stream(device=dev) for _ in range(depth)]
        self.events = [torch.cuda.Event() for _ in range(depth)]
        self.host = [[torch.empty(p.shape, dtype=p.dtype, pin_memory=True) for p in s.packed] for s in self.slots]
        self.pending = [None] * depth
        self.count = 0

    _make_slot = staticmethod(GraphedInference)

    def _collect(self, k):
        img = self.pending[k]
        self.pending[k] = None
        self.events[k].synchronize()
        results = self.slots[k].decode(self.host[k])
        if any(r is None for r in results):               # static capacity overflow: the reference-shaped path, synchronously
            return self.slots[k].fallback(img)
        return results

    def _fresh_slot(self, k):
        """Slot k, captured again first if the model's parameters changed since its capture."""
        slot = self.slots[k]
        if _param_fingerprint(slot._tensors) != slot._fingerprint:
            head = self.model.bbox_head
            prev, head.tower_streams = getattr(head, 'tower_streams', None), False
            try:
                slot._capture()
            finally:
                head.tower_streams = prev
            self.host[k] = [torch.empty(p.shape, dtype=p.dtype, pin_memory=True) for p in slot.packed]
        return slot

    def submit_device(self, fill, sink):
        """`submit` for a producer and a consumer that live on the device (`SceneInference`): `fill(static_img)` writes the
        next slot's input (`fill(list of view buffers)` for `PipelinedAugInference`) and `sink(packed)` reads its packed results, both on the slot's stream around the replay.  No
        host copy and nothing pending: stream order alone keeps a slot's replays apart, the host never waits, and the
        caller makes its own stream wait on `streams` before it uses what `sink` wrote.  Not to be mixed with `submit`
        while results of that are in flight."""
        k = self.count % self.depth
        if self.pending[k] is not None:
            raise RuntimeError("PipelinedInference.submit_device: results of submit() are still in flight; flush() first")
        slot, s = self._fresh_slot(k), self.streams[k]
        s.wait_stream(torch.cuda.current_stream(slot.device))
        with torch.cuda.stream(s):
            fill(slot.inputs)
            slot.graph.replay()
            sink(slot.packed)
        self.count += 1

    def submit(self, img):
        k = self.count % self.depth
        out = self._collect(k) if self.pending[k] is not None else None
        slot, s = self._fresh_slot(k), self.streams[k]
        s.wait_stream(torch.cuda.current_stream(slot.device))    # the image may have been produced on the caller's stream
        with torch.cuda.stream(s):
            slot.load(img)
            slot.graph.replay()
            for h, p in zip(self.host[k], slot.packed):
                h.copy_(p, non_blocking=True)
            self.events[k].record(s)
        self.pending[k] = img
        self.count += 1
        return out

    def flush(self):
        outs = []
        for j in range(self.depth):
            k = (self.count + j) % self.depth
            if self.pending[k] is not None:
                outs.append(self._collect(k))
        return outs


class PipelinedAugInference(PipelinedInference):
    """`PipelinedInference` over `GraphedAugInference` slots: `img` is the list of view tensors, `img_metas` the per-view meta
    lists, `submit(imgs)` / `flush()` return `aug_test`'s results per image, and `submit_device(fill, sink)` hands `fill` the
    slot's list of view buffers.  `rescale` defaults to what a scene's patches need (rows in original-image coordinates)."""

    def __init__(self, model, imgs, img_metas, depth=2, warmup=3, _allow_half=False, rescale=True):
        super(PipelinedAugInference, self).__init__(model, list(imgs), img_metas, depth, warmup, _allow_half, rescale)

    _make_slot = staticmethod(GraphedAugInference)
