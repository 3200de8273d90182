"""The three-model surface: ``MaskRCNN``, ``Classifier``, ``Mask``.

Mirrors the classes Xcode generates from the reference's three ``.mlmodel`` artefacts
(``Example/iOS Example.xcodeproj/project.pbxproj:25-28``; specs emitted by
``Sources/maskrcnn/Python/Conversion/task.py:69-116``): ``MaskRCNN().prediction(image:)`` →
``detections`` (100,6) + ``mask`` (100,28,28); ``Classifier.prediction(feature_map:)`` →
``probabilities``, ``bounding_boxes``; ``Mask.prediction(feature_map:)`` → ``masks``.
``MaskRCNN.predict`` is the batched extension used by the bench / multi-GPU driver.
Nothing here computes: all work is ``mrcnn_*`` calls into libmaskrcnn_hip.so.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, Optional

import numpy as np

from . import _lib
from ._marshal import image_table
from .config import MaskRCNNConfig

# f32s / f32x3: fp32 tensors, 2- / 3-part split-fp16 MFMA.  "default" = MRCNN_DEFAULT (include/maskrcnn_hip.h): what the artefact is prepared
# for — f32x3 with the stored exponents when `convert --calibrate` wrote them into MaskRCNN.mrcw, f32 otherwise — the mode a host that names no
# precision gets (`MaskRCNN()` of ViewController.swift:37).
DTYPES = {"default": _lib.DEFAULT, "f32": _lib.F32, "f16": _lib.F16, "f32s": _lib.F32S, "f32x3": _lib.F32X3}
DTYPE_NAMES = {v: k for k, v in DTYPES.items() if k != "default"}
STAGES = ["Trunk", "Proposal-Eval", "PyramidROIAlign-Eval", "TimeDistributedClassifierLayer-Eval", "Detection-Eval",
          "PyramidROIAlign-Eval-Mask", "TimeDistributedMask-Eval"]


class _Model:
    KIND = -1

    def __init__(self, path: str, max_batch: int, compute_dtype: int = _lib.DEFAULT):
        self._h = C.c_void_p()
        _lib.check(_lib.lib().mrcnn_model_load(self.KIND, os.fspath(path).encode(), int(max_batch), compute_dtype,
                                               C.byref(self._h)))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            try:
                _lib.lib().mrcnn_model_destroy(h)
            except Exception:
                pass
            self._h = None

    def get_int(self, key: str) -> int:
        v = C.c_int64(0)
        _lib.check(_lib.lib().mrcnn_model_get_int(self._h, key.encode(), C.byref(v)))
        return int(v.value)

    def enable_graph(self, on: bool = True):
        """hipGraph replay of predict's launch sequence (default off; see mrcnn_model_enable_graph)."""
        _lib.check(_lib.lib().mrcnn_model_enable_graph(self._h, int(on)))

    def set_stream(self, hip_stream: int):
        _lib.check(_lib.lib().mrcnn_model_set_stream(self._h, C.c_void_p(hip_stream)))


class MaskRCNN(_Model):
    """``MaskRCNN(path)``: loads MaskRCNN.mrcw; anchors / Classifier / Mask come from
    ``MaskRCNNConfig.defaultConfig()`` which must be set first (AppDelegate.swift:18-20)."""
    KIND = _lib.MODEL_MASKRCNN

    def __init__(self, path: str, max_batch: int = 1, compute_dtype: str = "default"):
        cfg = MaskRCNNConfig.defaultConfig()
        for name in ("anchorsURL", "compiledClassifierModelURL", "compiledMaskModelURL"):
            if getattr(cfg, name) is None:
                # the reference force-unwraps and crashes (ProposalLayer.swift:68); we raise
                raise _lib.MrcnnError(6, f"MaskRCNNConfig.defaultConfig().{name} must be set before loading MaskRCNN")
        super().__init__(path, max_batch, DTYPES[compute_dtype])
        self.compute_dtype = DTYPE_NAMES[self.get_int("compute_dtype")]      # the RESOLVED mode ("default" never stays)
        self.compute_dtype_defaulted = bool(self.get_int("compute_dtype_defaulted"))
        self.max_batch = max_batch
        self.image_height = self.get_int("image_height")
        self.image_width = self.get_int("image_width")
        self.max_detections = self.get_int("max_detections")
        self.max_proposals = self.get_int("max_proposals")
        self.num_classes = self.get_int("num_classes")
        self.mask_size = self.get_int("mask_size")

    # -- reference-shaped single-image call ---------------------------------------------------------
    def prediction(self, image: np.ndarray) -> Dict[str, np.ndarray]:
        """image (H,W,3) uint8 RGB → {"detections": (maxDet,6), "mask": (maxDet,28,28)}."""
        det, mask = self.predict(image[None])
        return {"detections": det[0], "mask": mask[0]}

    # -- batched extension --------------------------------------------------------------------------
    def predict(self, images):
        """images (B,H,W,3) uint8 — numpy (host) or torch CUDA tensor (device, results stay on the GPU)."""
        if isinstance(images, np.ndarray):
            imgs = np.ascontiguousarray(images, dtype=np.uint8)
            B, H, W, _ = imgs.shape
            det = np.empty((B, self.max_detections, 6), dtype=np.float32)
            mask = np.empty((B, self.max_detections, self.mask_size, self.mask_size), dtype=np.float32)
            _lib.check(_lib.lib().mrcnn_maskrcnn_predict(self._h, imgs.ctypes.data, B, H, W, _lib.HOST, det.ctypes.data,
                                                         mask.ctypes.data))
            return det, mask
        import torch
        assert images.is_cuda and images.dtype == torch.uint8 and images.is_contiguous()
        B, H, W, _ = images.shape
        det = torch.empty((B, self.max_detections, 6), dtype=torch.float32, device=images.device)
        mask = torch.empty((B, self.max_detections, self.mask_size, self.mask_size), dtype=torch.float32, device=images.device)
        _lib.check(_lib.lib().mrcnn_maskrcnn_predict(self._h, images.data_ptr(), B, H, W, _lib.DEVICE, det.data_ptr(),
                                                     mask.data_ptr()))
        return det, mask

    def predict_scalefit(self, images: np.ndarray):
        """images (B,h,w,3) uint8 of ANY size: `.scaleFit` letterbox fused into the pre-processing kernel, then predict.
        Boxes are normalized in the letterboxed frame (evaluate.unletterbox_boxes / mrcnn_unletterbox_boxes map them back)."""
        imgs = np.ascontiguousarray(images, dtype=np.uint8)
        B, h, w, _ = imgs.shape
        det = np.empty((B, self.max_detections, 6), dtype=np.float32)
        mask = np.empty((B, self.max_detections, self.mask_size, self.mask_size), dtype=np.float32)
        _lib.check(_lib.lib().mrcnn_maskrcnn_predict_scalefit(self._h, imgs.ctypes.data, B, h, w, _lib.HOST, det.ctypes.data, mask.ctypes.data))
        return det, mask

    def predict_images(self, images):
        """One predict over images of DIFFERENT sizes (mrcnn_maskrcnn_predict_images): a list of (h_i, w_i, 3) uint8 numpy arrays —
        or of uint8 CUDA tensors, in which case the results stay on the device.  Every image is letterboxed with its own geometry
        inside the one pre-processing launch; row b equals predict_scalefit(images[b][None]).  Returns (det, mask) like
        predict_scalefit: boxes normalized in the letterboxed frame (detection.paste_masks_source maps them back)."""
        table, space, keep, _, _ = image_table(images)
        B = len(keep)
        det = space.new((B, self.max_detections, 6), np.float32)
        mask = space.new((B, self.max_detections, self.mask_size, self.mask_size), np.float32)
        _lib.check(_lib.lib().mrcnn_maskrcnn_predict_images(self._h, table, B, space.code, space.ptr(det), space.ptr(mask)))
        return det, mask

    def predict_tiles(self, images, tiles):
        """One predict per WINDOW of the images (mrcnn_maskrcnn_predict_tiles): images as predict_images takes them, tiles an (n, 5)
        int32 table of (image, y0, x0, height, width) (detection.tile_plan).  Record t equals predict_images on a contiguous copy
        of window t; every image crosses to the device once.  Any number of tiles: the call runs them max_batch at a time."""
        from .detection import _tile_table
        tab = _tile_table(tiles)
        table, space, keep, _, _ = image_table(images)
        B, T = len(keep), int(tab.shape[0])
        det = space.new((T, self.max_detections, 6), np.float32)
        mask = space.new((T, self.max_detections, self.mask_size, self.mask_size), np.float32)
        _lib.check(_lib.lib().mrcnn_maskrcnn_predict_tiles(self._h, table, B, tab.ctypes.data_as(C.POINTER(_lib.Tile)), T, space.code, space.ptr(det), space.ptr(mask)))
        return det, mask

    def predict_tiled(self, images, tile=None, overlap=(64, 64), metric="ios", match_threshold=0.5, max_out=None, threshold=0.5,
                      unite=False, link_threshold=0.5, polygons=False, tolerance=None, nest=False, close=0,
                      min_component_area=0, fill_holes=False, disjoint=False, props=False):
        """Large images as overlapping windows at native resolution: detection.tile_plan per image (tile = None: the model's input
        size), predict_tiles, detection.merge_tiles.  Returns (det_src, source, n_kept, rles) in the frame of the images, in the
        form coco_results.coco_results and coco_eval.score_batch take.  By default an object is found whole only if some window
        holds it whole: choose the overlap at least as large as the largest object of interest.  unite=True replaces the third step
        by detection.unite_tiles(metric, link_threshold): the cut parts of an object larger than the overlap, and its duplicates,
        become one mask (match_threshold is not used then).  polygons=True adds a fifth result, (rings, areas) as
        detection.rle_to_polygons returns them: the boundaries of the masks, traced from the runs where the merge or the union left
        them — on the device when the images are CUDA tensors.  tolerance (pixels) simplifies those rings there too
        (detection.simplify_polygons); the areas stay the pixel areas.  nest=True makes that result (rings, areas, nesting): the rings
        nested into outlines and their holes (detection.nest_polygons), in the same place, on the traced rings.  close=r (pixels; 0: the
        masks as they are) closes the kept masks first — detection.rle_close on the runs where they lie: pinholes and gaps up to 2r
        wide are filled — and both the returned rles and the polygons are those of the closed masks.  fill_holes (True: every hole;
        an integer: holes of up to that many pixels, 0 like False) and min_component_area=a (specks of fewer than a pixels are cleared) filter the
        kept masks by their connected components after the closing, holes first, in the same place (detection.rle_fill_holes,
        detection.rle_remove_small).  disjoint=True then takes from every kept mask the pixels of the kept masks before it in its image
        (detection.rle_disjoint, in the same place): no pixel belongs to two masks, as detection.instance_map_rle decides it.
        props=True appends one more result, the last: the dictionary of detection.rle_region_props — centroid, orientation, perimeter,
        hull, solidity, oriented box — of the final masks (after close, fill_holes, min_component_area and disjoint), measured from the
        runs where they lie, entry b * max_out + i for row i of image b.  The defaults change nothing."""
        from .detection import (_merge_tiles, rle_close, rle_disjoint, rle_fill_holes, rle_region_props, rle_remove_small, rle_rows_of, rle_to_polygons,
                                tile_plan)
        images = list(images)
        H, W = self.image_height, self.image_width
        tile = (H, W) if tile is None else tile
        sizes = [(int(im.shape[0]), int(im.shape[1])) for im in images]
        tiles = np.concatenate([tile_plan(h, w, tile, overlap, b) for b, (h, w) in enumerate(sizes)])
        det, mask = self.predict_tiles(images, tiles)
        resident = []
        out = _merge_tiles(False, det, mask, tiles, sizes, H, W, threshold, metric, link_threshold if unite else match_threshold, max_out, unite=unite,
                           resident=resident)[:4]
        if close:
            resident[0] = rle_close(resident[0], sizes, int(close))
        fill = fill_holes is True or (fill_holes is not False and fill_holes is not None and int(fill_holes) > 0)      # (0 fills nothing: like False)
        if fill:
            resident[0] = rle_fill_holes(resident[0], sizes, max_area=None if fill_holes is True else int(fill_holes))
        if min_component_area:
            resident[0] = rle_remove_small(resident[0], sizes, int(min_component_area))
        if disjoint:
            resident[0] = rle_disjoint(out[0], resident[0], sizes)[0]
        if close or min_component_area or fill or disjoint:
            out = (*out[:3], rle_rows_of(resident[0], sizes))
        if polygons:
            out = (*out, rle_to_polygons(resident[0], sizes, tolerance=tolerance, nest=nest))
        if props:
            out = (*out, rle_region_props(resident[0], sizes))
        return out

    def predict_jpegs(self, files, entropy="host"):
        """predict_images straight from JPEG files (mrcnn_maskrcnn_predict_jpegs_on): a list of bytes.  The entropy decoders run on the
        host, everything after them on the GPU, and the decoded images stay in staging the handle owns; the results equal
        ``predict_images([jpeg.decode_host(f) for f in files])`` bit for bit.  Returns (det, mask, [(h_b, w_b)]) with det and mask
        CUDA tensors, like predict_images on CUDA tensors.  entropy="device" (opt-in) decodes the Huffman streams on the GPU as well
        (jpeg.decode_batch explains it); the results are the same."""
        import torch
        from .jpeg import entropy_code, file_table
        files = list(files)
        B = len(files)
        table, keep = file_table(files)
        hs, ws = np.zeros(max(1, B), np.int32), np.zeros(max(1, B), np.int32)
        det = torch.empty((B, self.max_detections, 6), dtype=torch.float32, device="cuda")
        mask = torch.empty((B, self.max_detections, self.mask_size, self.mask_size), dtype=torch.float32, device="cuda")
        _lib.check(_lib.lib().mrcnn_maskrcnn_predict_jpegs_on(self._h, table, B, _lib.DEVICE, entropy_code(entropy), det.data_ptr(), mask.data_ptr(),
                                                              hs.ctypes.data, ws.ctypes.data))
        del keep
        return det, mask, [(int(hs[b]), int(ws[b])) for b in range(B)]

    def render_images(self, images, **kw):
        """predict_images followed by detection.render_detections_source at this handle's model size: the images with their
        detections drawn on them (DetectionRenderer.swift:26-88).  Keyword arguments go to the render (threshold, min_score, alpha,
        stroke).  A convenience: no device work of its own."""
        from .detection import render_detections_source
        images = list(images)
        det, mask = self.predict_images(images)
        return render_detections_source(images, det, mask, self.image_height, self.image_width, **kw)

    def render_jpegs(self, images, quality: int = 90, sampling="420", **kw):
        """render_images followed by jpeg.encode_batch on the device result: the overlays as JPEG files, a list of bytes.  For CUDA
        images the rendered pixels never exist in host memory — only the files cross back.  A convenience: no device work of its own."""
        from .jpeg import encode_batch
        return encode_batch(self.render_images(images, **kw), quality=quality, sampling=sampling)

    def instance_pngs(self, images, **kw):
        """predict_images followed by detection.instance_map_source at this handle's model size and png.encode_batch on the device
        result: which detection owns each pixel, as PNG files (index = row + 1, 0 and transparent where there is none; coloured
        like render_images), a list of bytes.  Keyword arguments go to the map (threshold, min_score).  For CUDA images the maps
        never exist in host memory — only the files cross back.  A convenience: no device work of its own."""
        from .detection import instance_map_source
        from .png import encode_batch
        images = list(images)
        det, mask = self.predict_images(images)
        _, maps, _ = instance_map_source(det, mask, [(int(im.shape[0]), int(im.shape[1])) for im in images], self.image_height, self.image_width, **kw)
        return encode_batch(maps, rows=self.max_detections)

    def _tiled_draw_args(self, kw):
        """Splits the keywords of the tiled renderers: predict_tiled's own (tile, overlap, unite, ...) and the rest for the draw."""
        names = ("tile", "overlap", "metric", "match_threshold", "max_out", "threshold", "unite", "link_threshold")
        return {k: kw.pop(k) for k in names if k in kw}, kw

    def render_tiled(self, images, **kw):
        """predict_tiled followed by detection.render_detections_rle: large images with the detections of their windows drawn on
        them, the masks taken from the run lengths — united ones (unite=True) included, which no 28x28 mask reproduces.  predict_tiled's
        keywords (tile, overlap, unite, metric, ...) pass through, the others go to the render (min_score, alpha, stroke).  A
        convenience: no device work of its own."""
        from .detection import render_detections_rle
        images = list(images)
        tiled, draw = self._tiled_draw_args(dict(kw))
        det_src, _source, _n_kept, rles = self.predict_tiled(images, **tiled)
        return render_detections_rle(images, det_src, rles, **draw)

    def render_tiled_jpegs(self, images, quality: int = 90, sampling="420", **kw):
        """render_tiled followed by jpeg.encode_batch on the device result: the overlays as JPEG files, a list of bytes.  A
        convenience: no device work of its own."""
        from .jpeg import encode_batch
        return encode_batch(self.render_tiled(images, **kw), quality=quality, sampling=sampling)

    def instance_pngs_tiled(self, images, **kw):
        """predict_tiled followed by detection.instance_map_rle and png.encode_batch on the device result: which detection owns each
        pixel of a large image, as PNG files (index = row + 1, 0 and transparent where there is none), a list of bytes.  The PNG
        palette holds 255 rows: max_out (default: the model's rows per window) above 255 raises ValueError.  predict_tiled's keywords
        pass through, min_score goes to the map.  A convenience: no device work of its own."""
        from .detection import instance_map_rle
        from .png import encode_batch
        images = list(images)
        tiled, draw = self._tiled_draw_args(dict(kw))
        max_out = self.max_detections if tiled.get("max_out") is None else int(tiled["max_out"])
        if not 1 <= max_out <= 255:
            raise ValueError(f"instance_pngs_tiled: max_out = {max_out} rows do not fit the PNG palette (1..255): pass max_out <= 255")
        det_src, _source, _n_kept, rles = self.predict_tiled(images, **tiled)
        maps, _visible = instance_map_rle(det_src, rles, [(int(im.shape[0]), int(im.shape[1])) for im in images], **draw)
        return encode_batch(maps, rows=max_out)

    def predict_into(self, images, det, mask, sync: bool = True):
        """Device tensors in, pre-allocated device tensors out (bench loop: no allocation, optional no sync)."""
        B, H, W, _ = images.shape
        fn = _lib.lib().mrcnn_maskrcnn_predict if sync else None
        if sync:
            _lib.check(fn(self._h, images.data_ptr(), B, H, W, _lib.DEVICE, det.data_ptr(), mask.data_ptr()))
        else:
            _lib.check(_lib.lib().mrcnn_maskrcnn_predict_async(self._h, images.data_ptr(), B, H, W, det.data_ptr(), mask.data_ptr()))

    def predict_host_into(self, images: np.ndarray, det: np.ndarray, mask: np.ndarray):
        """Host buffers in and out without allocation (pinned memory gives asynchronous PCIe copies): the H2D of the batch
        and the D2H of the records are part of the call — bench.py's h2d_included leg."""
        B, H, W, _ = images.shape
        _lib.check(_lib.lib().mrcnn_maskrcnn_predict(self._h, images.ctypes.data, B, H, W, _lib.HOST, det.ctypes.data, mask.ctypes.data))

    def submit(self, images: np.ndarray):
        """Pipelined host entry (mrcnn_maskrcnn_submit): the H2D copy of this batch overlaps the predict of the previous one.
        `images` must stay alive (and unchanged) until the matching collect()."""
        B, H, W, _ = images.shape
        _lib.check(_lib.lib().mrcnn_maskrcnn_submit(self._h, images.ctypes.data, B, H, W))

    def collect(self, det: np.ndarray, mask: np.ndarray) -> int:
        """Results of the OLDEST submission into the given host buffers; returns its batch size."""
        n = C.c_int(0)
        _lib.check(_lib.lib().mrcnn_maskrcnn_collect(self._h, det.ctypes.data, mask.ctypes.data, C.byref(n)))
        return int(n.value)

    def check_range(self) -> bool:
        """After predict_into(sync=False): synchronises the model's stream and reports whether the last predict left
        the fp16 range (its results are then not valid) — the async counterpart of the error predict() raises."""
        t = C.c_int(0)
        _lib.check(_lib.lib().mrcnn_model_check_range(self._h, C.byref(t)))
        return bool(t.value)

    # -- scale-aware split (include/maskrcnn_hip.h: mrcnn_model_calibrate_split) ----------------------
    def calibrate_split(self, images, apply: bool = True) -> Dict[str, int]:
        """One calibration predict on `images` (numpy (B,H,W,3) uint8 or a CUDA tensor): a power-of-two pre-scale per tensor
        group so that the split modes carry every activation like fp32 whatever the checkpoint's scale.  apply=False only
        diagnoses.  Returns the totals of the pass (see split_report for the per-group view)."""
        if isinstance(images, np.ndarray):
            imgs = np.ascontiguousarray(images, dtype=np.uint8)
            B, H, W, _ = imgs.shape
            _lib.check(_lib.lib().mrcnn_model_calibrate_split(self._h, imgs.ctypes.data, B, H, W, _lib.HOST, int(apply)))
        else:
            B, H, W, _ = images.shape
            _lib.check(_lib.lib().mrcnn_model_calibrate_split(self._h, images.data_ptr(), B, H, W, _lib.DEVICE, int(apply)))
        return {k: self.get_int(k) for k in ("split_small_inputs", "split_inexact_inputs", "split_inputs_counted", "split_min_exponent",
                                             "split_max_exponent", "split_calibrated")}

    def split_report(self):
        """[{name, exponent, fixed, absmax, small_inputs, inexact_inputs, inputs_counted}] per tensor group."""
        out = []
        st = _lib.SplitGroupStat()
        for i in range(self.get_int("split_groups")):
            _lib.check(_lib.lib().mrcnn_model_split_group_stat(self._h, i, C.byref(st)))
            out.append({"name": st.name.decode(), "exponent": int(st.exponent), "fixed": bool(st.fixed), "absmax": float(st.absmax),
                        "small_inputs": int(st.small_inputs), "inexact_inputs": int(st.inexact_inputs), "inputs_counted": int(st.inputs_counted)})
        return out

    @property
    def split_exponents(self) -> np.ndarray:
        n = C.c_int(0)
        _lib.check(_lib.lib().mrcnn_model_get_split_exponents(self._h, None, 0, C.byref(n)))
        e = np.zeros(n.value, np.int32)
        _lib.check(_lib.lib().mrcnn_model_get_split_exponents(self._h, e.ctypes.data, e.size, C.byref(n)))
        return e

    @split_exponents.setter
    def split_exponents(self, exps):
        e = np.ascontiguousarray(exps, dtype=np.int32)
        _lib.check(_lib.lib().mrcnn_model_set_split_exponents(self._h, e.ctypes.data, e.size))

    # -- parity / profiling hooks -------------------------------------------------------------------
    def read_tensor(self, name: str, image_index: int = 0) -> np.ndarray:
        """A named intermediate of the last predict for one image, flat fp32 (include/maskrcnn_hip.h: mrcnn_model_read_tensor).
        Trunk: "C1" (the pooled stem output, NHWC 64 channels), "C2".."C5" (the backbone stages), "P2".."P5" (NHWC 256 channels),
        "rpn_probs", "rpn_deltas"; then "topk_idx", "boxes_sorted", "keep_count", "rois", "pooled", "cls_probs", "cls_bbox", "cls6",
        "detections", "pooled_mask", "mask_row_flags", "mask".  Split-mode tensors come back without their stored exponent."""
        cnt = C.c_int64(0)
        L = _lib.lib()
        st = L.mrcnn_model_read_tensor(self._h, name.encode(), image_index, None, 0, C.byref(cnt))
        if cnt.value <= 0:
            _lib.check(st)
        buf = np.empty(cnt.value, dtype=np.float32)
        _lib.check(L.mrcnn_model_read_tensor(self._h, name.encode(), image_index, buf.ctypes.data, buf.size, C.byref(cnt)))
        return buf

    def conv_profile_enable(self, on: bool = True):
        _lib.check(_lib.lib().mrcnn_model_conv_profile_enable(self._h, int(on)))

    def conv_profile(self):
        """{tile: (launches, total_ms, total_algorithmic_flops)} since conv_profile_enable()."""
        out = {}
        for tile, name in enumerate(("128x128", "128x64", "128x32", "128x128w4", "256x256pp", "128xNhalo", "128x256tail", "bneck", "c3h")):
            n, ms, fl = C.c_int64(0), C.c_double(0), C.c_double(0)
            _lib.check(_lib.lib().mrcnn_model_conv_profile_get(self._h, tile, C.byref(n), C.byref(ms), C.byref(fl)))
            out[name] = (int(n.value), float(ms.value), float(fl.value))
        return out

    def conv_profile_bytes(self):
        """{tile: total ALGORITHMIC bytes} of the launches conv_profile() counts (every operand across HBM once)."""
        out = {}
        for tile, name in enumerate(("128x128", "128x64", "128x32", "128x128w4", "256x256pp", "128xNhalo", "128x256tail", "bneck", "c3h")):
            b = C.c_double(0)
            _lib.check(_lib.lib().mrcnn_model_conv_profile_bytes(self._h, tile, C.byref(b)))
            out[name] = float(b.value)
        return out

    def conv_profile_groups(self):
        """{"backbone" | "other": (launches, total_ms, total_algorithmic_flops)} — conv1 + res2..res5 against everything else."""
        out = {}
        for grp, name in ((1, "backbone"), (0, "other")):
            n, ms, fl = C.c_int64(0), C.c_double(0), C.c_double(0)
            _lib.check(_lib.lib().mrcnn_model_conv_profile_group(self._h, grp, C.byref(n), C.byref(ms), C.byref(fl)))
            out[name] = (int(n.value), float(ms.value), float(fl.value))
        return out

    def conv_profile_shapes(self):
        """[(M, N, K, tile, launches, total_ms, total_algorithmic_flops, total_algorithmic_bytes)] per distinct GEMM shape."""
        L = _lib.lib()
        n = C.c_int(0)
        _lib.check(L.mrcnn_model_conv_profile_shapes(self._h, None, 0, C.byref(n)))
        buf = (_lib.ConvShapeStat * max(n.value, 1))()
        _lib.check(L.mrcnn_model_conv_profile_shapes(self._h, buf, n.value, C.byref(n)))
        return [(r.M, r.N, r.K, r.tile, r.launches, r.total_ms, r.total_flops, r.total_bytes) for r in buf[:n.value]]

    def enable_timing(self, on: bool = True):
        _lib.check(_lib.lib().mrcnn_model_enable_timing(self._h, int(on)))

    def stage_ms(self) -> Dict[str, float]:
        out = {}
        for s in STAGES:
            v = C.c_float(0)
            _lib.check(_lib.lib().mrcnn_model_stage_ms(self._h, s.encode(), C.byref(v)))
            out[s] = float(v.value)
        return out


class Classifier(_Model):
    KIND = _lib.MODEL_CLASSIFIER

    def __init__(self, path: str, max_rows: int = 1000, compute_dtype: str = "default"):
        super().__init__(path, max_rows, DTYPES[compute_dtype])
        self.num_classes = self.get_int("num_classes")

    def prediction(self, feature_map: np.ndarray) -> Dict[str, np.ndarray]:
        """feature_map (256,7,7) or (n,256,7,7) float32 CHW → probabilities (n,nc), bounding_boxes (n,nc*4)."""
        fm = np.ascontiguousarray(feature_map, dtype=np.float32)
        single = fm.ndim == 3
        if single:
            fm = fm[None]
        n = fm.shape[0]
        probs = np.empty((n, self.num_classes), dtype=np.float32)
        bbox = np.empty((n, self.num_classes * 4), dtype=np.float32)
        _lib.check(_lib.lib().mrcnn_classifier_predict(self._h, fm.ctypes.data, n, _lib.HOST, probs.ctypes.data, bbox.ctypes.data))
        if single:
            return {"probabilities": probs[0], "bounding_boxes": bbox[0]}
        return {"probabilities": probs, "bounding_boxes": bbox}


class Mask(_Model):
    KIND = _lib.MODEL_MASK

    def __init__(self, path: str, max_rows: int = 100, compute_dtype: str = "default"):
        super().__init__(path, max_rows, DTYPES[compute_dtype])
        self.num_classes = self.get_int("num_classes")

    def prediction(self, feature_map: np.ndarray) -> Dict[str, np.ndarray]:
        """feature_map (256,14,14) or (n,256,14,14) float32 CHW → masks (n,nc,28,28)."""
        fm = np.ascontiguousarray(feature_map, dtype=np.float32)
        single = fm.ndim == 3
        if single:
            fm = fm[None]
        n = fm.shape[0]
        masks = np.empty((n, self.num_classes, 2 * fm.shape[2], 2 * fm.shape[3]), dtype=np.float32)
        _lib.check(_lib.lib().mrcnn_mask_predict(self._h, fm.ctypes.data, n, _lib.HOST, masks.ctypes.data))
        return {"masks": masks[0] if single else masks}


def load_maskrcnn(model_dir: str, max_batch: int = 1, compute_dtype: str = "default") -> MaskRCNN:
    """Sets MaskRCNNConfig from a directory holding MaskRCNN.mrcw / Classifier.mrcw / Mask.mrcw /
    anchors.bin (the four artefacts of DownloadCommand.swift:10-32) and loads the main model —
    the sequence of EvaluateCommand.swift:144-153."""
    cfg = MaskRCNNConfig.defaultConfig()
    cfg.anchorsURL = os.path.join(model_dir, "anchors.bin")
    cfg.compiledClassifierModelURL = os.path.join(model_dir, "Classifier.mrcw")
    cfg.compiledMaskModelURL = os.path.join(model_dir, "Mask.mrcw")
    return MaskRCNN(os.path.join(model_dir, "MaskRCNN.mrcw"), max_batch=max_batch, compute_dtype=compute_dtype)
