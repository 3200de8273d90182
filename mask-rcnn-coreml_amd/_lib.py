"""ctypes binding of libmaskrcnn_hip.so (C ABI: include/maskrcnn_hip.h).

The library is the product; there is no CPU fallback.  ``lib()`` raises ``NativeLibraryMissing`` when
the shared object has not been built (``python __graft_entry__.py`` / ``make -C csrc``), and every
compute entry point returns ``MRCNN_ERR_HIP`` when no gfx950 device is present.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.environ.get("MRCNN_HIP_LIB") or os.path.join(_HERE, "libmaskrcnn_hip.so")   # override: A/B builds

MRCNN_OK = 0
F32, F64, F16, U8, I32, F32S, F32X3 = 0, 1, 2, 3, 4, 5, 6
DEFAULT = -1          # MRCNN_DEFAULT of mrcnn_model_load: the mode the artefact is prepared for (stored split exponents -> F32X3, else F32)
HOST, DEVICE = 0, 1
MORPH_ERODE, MORPH_DILATE, MORPH_BOUNDARY, MORPH_MAX_RADIUS = 0, 1, 2, 1024
COMPONENTS_OF_ZEROS, COMPONENTS_OF_ONES, COMPONENTS_MERGE, COMPONENTS_SPLIT = 0, 1, 0, 1
RLE_OR, RLE_AND, RLE_XOR, RLE_DIFF = 0, 1, 2, 3
XF_TRANSPOSE, XF_MAX_BOX_WORDS = 1, 1 << 30
PARAM_INT, PARAM_DOUBLE, PARAM_STRING = 0, 1, 2
MODEL_MASKRCNN, MODEL_CLASSIFIER, MODEL_MASK = 0, 1, 2

# declared in include/maskrcnn_hip.h (the drop-in surface)
EXPORTED_SYMBOLS = [
    "mrcnn_last_error", "mrcnn_version", "mrcnn_device_count", "mrcnn_config_set_anchors_path",
    "mrcnn_config_set_classifier_path", "mrcnn_config_set_mask_path", "mrcnn_config_get_anchors_path",
    "mrcnn_config_get_classifier_path", "mrcnn_config_get_mask_path", "mrcnn_layer_create",
    "mrcnn_layer_set_weight_data", "mrcnn_layer_output_shapes", "mrcnn_layer_evaluate", "mrcnn_layer_destroy",
    "mrcnn_iou", "mrcnn_model_load", "mrcnn_model_destroy", "mrcnn_model_set_stream", "mrcnn_maskrcnn_predict",
    "mrcnn_maskrcnn_predict_async", "mrcnn_maskrcnn_submit", "mrcnn_maskrcnn_collect", "mrcnn_classifier_predict", "mrcnn_mask_predict", "mrcnn_model_get_int",
    "mrcnn_model_read_tensor", "mrcnn_model_enable_timing", "mrcnn_model_stage_ms", "mrcnn_model_enable_graph",
    "mrcnn_detections_decode", "mrcnn_mask_to_u8", "mrcnn_paste_masks", "mrcnn_generate_anchors",
    "mrcnn_letterbox_geometry", "mrcnn_letterbox_rgb", "mrcnn_model_check_range", "mrcnn_model_calibrate_split", "mrcnn_model_split_group_stat",
    "mrcnn_model_get_split_exponents", "mrcnn_model_set_split_exponents", "mrcnn_roi_align_nhwc",
    "mrcnn_dist_unique_id", "mrcnn_dist_init", "mrcnn_dist_destroy", "mrcnn_dist_shard", "mrcnn_dist_record_floats",
    "mrcnn_dist_all_gather_records", "mrcnn_maskrcnn_predict_sharded", "mrcnn_mask_to_u8_f64",
    "mrcnn_dist_all_gather_records_async", "mrcnn_dist_wait", "mrcnn_dist_recovered", "mrcnn_dist_rccl_shared", "mrcnn_dist_plan", "mrcnn_dist_simulate_host",
    "mrcnn_maskrcnn_predict_scalefit", "mrcnn_unletterbox_boxes",
    "mrcnn_maskrcnn_predict_images", "mrcnn_paste_masks_source",
    "mrcnn_masks_rle_source", "mrcnn_rle_to_string", "mrcnn_rle_from_string",
    "mrcnn_instance_map_source", "mrcnn_render_detections_source",
    "mrcnn_rle_iou", "mrcnn_box_iou_xywh", "mrcnn_coco_match", "mrcnn_rle_from_polygons",
    "mrcnn_rle_from_polygons_batch", "mrcnn_coco_accumulate",
    "mrcnn_jpeg_info", "mrcnn_jpeg_decode_host", "mrcnn_jpeg_decode_batch", "mrcnn_maskrcnn_predict_jpegs",
    "mrcnn_jpeg_decode_batch_on", "mrcnn_maskrcnn_predict_jpegs_on",
    "mrcnn_jpeg_encode_host", "mrcnn_jpeg_encode_batch",
    "mrcnn_png_encode_host", "mrcnn_png_encode_batch",
    "mrcnn_tile_plan", "mrcnn_maskrcnn_predict_tiles", "mrcnn_merge_tiles", "mrcnn_merge_tiles_host",
    "mrcnn_unite_tiles", "mrcnn_unite_tiles_host",
    "mrcnn_rle_decode", "mrcnn_rle_decode_host", "mrcnn_instance_map_rle", "mrcnn_instance_map_rle_host",
    "mrcnn_render_detections_rle", "mrcnn_render_detections_rle_host",
    "mrcnn_rle_to_polygons", "mrcnn_rle_to_polygons_host",
    "mrcnn_polygons_simplify", "mrcnn_polygons_simplify_host",
    "mrcnn_polygons_nest", "mrcnn_polygons_nest_host",
    "mrcnn_rle_morph", "mrcnn_rle_morph_host", "mrcnn_boundary_radius",
    "mrcnn_rle_components", "mrcnn_rle_components_host", "mrcnn_rle_components_select", "mrcnn_rle_components_select_host",
    "mrcnn_rle_combine", "mrcnn_rle_combine_host",
    "mrcnn_rle_transform", "mrcnn_rle_transform_host",
    "mrcnn_rle_measure", "mrcnn_rle_measure_host", "mrcnn_rle_convex_hull", "mrcnn_rle_convex_hull_host",
]
# declared in include/maskrcnn_hip_test.h (test / measurement entry points of the same library)
TEST_SYMBOLS = [
    "mrcnn_bench_conv", "mrcnn_bench_conv_dtype", "mrcnn_model_conv_profile_enable", "mrcnn_model_conv_profile_get",
    "mrcnn_model_conv_profile_shapes", "mrcnn_conv2d_nhwc", "mrcnn_debug_set", "mrcnn_bottleneck_nhwc", "mrcnn_bench_mfma_probe", "mrcnn_model_conv_profile_group", "mrcnn_bottleneck_first_nhwc", "mrcnn_bottleneck_stage_nhwc", "mrcnn_model_conv_profile_bytes",
    "mrcnn_jpeg_last_stage_ms", "mrcnn_jpeg_coefficients", "mrcnn_test_last_range_flag", "mrcnn_classifier_rows", "mrcnn_test_roi_align_nhwc_batch", "mrcnn_conv_chain_nhwc",
    "mrcnn_test_conv_form_nhwc", "mrcnn_test_chain_stream_image", "mrcnn_test_proposals_batch", "mrcnn_test_detections_batch",
    "mrcnn_test_mask_select_batch", "mrcnn_test_xf_preimage",
]


class NativeLibraryMissing(RuntimeError):
    pass


class MrcnnError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"[mrcnn status {code}] {msg}")
        self.code = code


class Tensor(C.Structure):          # mrcnn_tensor
    _fields_ = [("data", C.c_void_p), ("dtype", C.c_int32), ("memspace", C.c_int32),
                ("shape", C.c_int64 * 5), ("strides", C.c_int64 * 5)]


class Param(C.Structure):           # mrcnn_param
    _fields_ = [("key", C.c_char_p), ("type", C.c_int32), ("i", C.c_int64), ("d", C.c_double), ("s", C.c_char_p)]


class SplitGroupStat(C.Structure):   # mrcnn_split_group_stat
    _fields_ = [("name", C.c_char * 48), ("exponent", C.c_int32), ("fixed", C.c_int32), ("absmax", C.c_float),
                ("small_inputs", C.c_int64), ("inexact_inputs", C.c_int64), ("inputs_counted", C.c_int64)]


class DetectionRecord(C.Structure):  # mrcnn_detection
    _fields_ = [("index", C.c_int64), ("x", C.c_double), ("y", C.c_double), ("w", C.c_double), ("h", C.c_double),
                ("class_id", C.c_int64), ("score", C.c_double)]


class IouGroup(C.Structure):        # mrcnn_iou_group
    _fields_ = [("d0", C.c_int64), ("d1", C.c_int64), ("g0", C.c_int64), ("g1", C.c_int64), ("out_offset", C.c_int64)]


class MatchGroup(C.Structure):      # mrcnn_match_group
    _fields_ = [("iou_offset", C.c_int64), ("iou_stride", C.c_int32), ("dt0", C.c_int32), ("dt1", C.c_int32), ("gt0", C.c_int32),
                ("gt1", C.c_int32), ("reserved", C.c_int32)]


class Jpeg(C.Structure):            # mrcnn_jpeg
    _fields_ = [("data", C.c_void_p), ("length", C.c_int64)]


class Image(C.Structure):           # mrcnn_image
    _fields_ = [("rgb", C.c_void_p), ("height", C.c_int32), ("width", C.c_int32)]


class Tile(C.Structure):            # mrcnn_tile
    _fields_ = [("image", C.c_int32), ("y0", C.c_int32), ("x0", C.c_int32), ("height", C.c_int32), ("width", C.c_int32)]


MATCH_IOU, MATCH_IOS = 0, 1
TILES_MAX_CANDIDATES = 8192
POLYGON_LDS_CORNERS = 1024      # MRCNN_POLYGON_LDS_CORNERS
SIMPLIFY_LDS_VERTICES = 1024    # MRCNN_SIMPLIFY_LDS_VERTICES
MEASURE_WORDS = 7               # MRCNN_MEASURE_WORDS
HULL_LDS_COLUMNS = 4096         # MRCNN_HULL_LDS_COLUMNS


class PngSource(C.Structure):       # mrcnn_png_source
    _fields_ = [("pixels", C.c_void_p), ("height", C.c_int32), ("width", C.c_int32)]


_lib = None


class ConvFormOutput(C.Structure):   # mrcnn_test_conv_output
    _fields_ = [("data", C.c_void_p), ("len", C.c_int64), ("offset", C.c_int64), ("batch_stride", C.c_int64), ("pitch", C.c_int64),
                ("row_pitch", C.c_int64)]


class ConvForm(C.Structure):     # mrcnn_test_conv_form
    _fields_ = [(k, C.c_int32) for k in ("dtype", "batch", "h", "w", "cin", "cout", "ksize", "stride", "act", "in_step", "res_shift", "n_split",
                                         "deconv2", "out_f32", "nc", "reserved")] + \
               [("sentinel", C.c_float), ("reserved2", C.c_int32)] + \
               [(k, C.c_void_p) for k in ("in_", "filters", "scale", "shift", "residual", "sel_w", "sel_cid")] + \
               [("out", ConvFormOutput), ("out2", ConvFormOutput), ("sel_partial", C.c_void_p), ("sel_parts", C.c_void_p)]


class MaskSelect(C.Structure):   # mrcnn_test_mask_select
    _fields_ = [(k, C.c_int32) for k in ("form", "dtype", "batch", "d", "det_rows", "hw", "c", "nc", "parts", "reserved")] + \
               [(k, C.c_int64) for k in ("row_len", "row_stride", "pooled_batch_stride", "det_stride", "out_stride")] + \
               [(k, C.c_void_p) for k in ("flags", "pooled", "det", "feat", "w", "bias", "partial", "masks", "out", "row_flags", "mapping", "kept",
                                          "sel_cid")]


class ConvShapeStat(C.Structure):    # mrcnn_conv_shape_stat
    _fields_ = [("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32), ("tile", C.c_int32),
                ("launches", C.c_int64), ("total_ms", C.c_double), ("total_flops", C.c_double), ("total_bytes", C.c_double)]


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO_PATH):
        raise NativeLibraryMissing(
            f"{SO_PATH} not built. Run `python __graft_entry__.py` (or `make -C mask-rcnn-coreml_amd/csrc`). "
            "There is no CPU fallback: the HIP library is the product.")
    # torch ships its own copy of the HIP runtime (torch/lib/libamdhip64.so, soname libamdhip64.so.7).
    # Two HIP runtimes in one process cannot both own the GPU, so when torch is importable it is
    # imported FIRST: the loader then resolves this library's DT_NEEDED libamdhip64.so.7 to the copy
    # torch already mapped, and torch tensors / streams and this library share one runtime.  A host
    # without torch (the Swift host) simply gets /opt/rocm's runtime.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(SO_PATH)
    vp, cp, i64p, f32p = C.c_void_p, C.c_char_p, C.POINTER(C.c_int64), C.POINTER(C.c_float)
    L.mrcnn_last_error.restype = cp
    L.mrcnn_version.restype = cp
    L.mrcnn_device_count.restype = C.c_int
    for n in ("anchors", "classifier", "mask"):
        getattr(L, f"mrcnn_config_set_{n}_path").argtypes = [cp]
        getattr(L, f"mrcnn_config_get_{n}_path").restype = cp
    L.mrcnn_layer_create.argtypes = [cp, C.POINTER(Param), C.c_int, C.POINTER(vp)]
    L.mrcnn_layer_set_weight_data.argtypes = [vp, vp, vp, C.c_int]
    L.mrcnn_layer_output_shapes.argtypes = [vp, vp, C.c_int, vp, C.POINTER(C.c_int)]
    L.mrcnn_layer_evaluate.argtypes = [vp, C.POINTER(Tensor), C.c_int, C.POINTER(Tensor), C.c_int]
    L.mrcnn_layer_destroy.argtypes = [vp]
    L.mrcnn_layer_destroy.restype = None
    L.mrcnn_iou.argtypes = [f32p, f32p]
    L.mrcnn_iou.restype = C.c_float
    L.mrcnn_model_load.argtypes = [C.c_int, cp, C.c_int, C.c_int, C.POINTER(vp)]
    L.mrcnn_model_destroy.argtypes = [vp]
    L.mrcnn_model_destroy.restype = None
    L.mrcnn_model_set_stream.argtypes = [vp, vp]
    L.mrcnn_maskrcnn_predict.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]
    L.mrcnn_maskrcnn_predict_scalefit.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]
    L.mrcnn_unletterbox_boxes.argtypes = [vp, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int]
    L.mrcnn_maskrcnn_predict_images.argtypes = [vp, C.POINTER(Image), C.c_int, C.c_int, vp, vp]
    L.mrcnn_paste_masks_source.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, C.c_float, C.c_int, vp, vp, vp]
    L.mrcnn_masks_rle_source.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, C.c_float, C.c_int, vp, vp, C.c_int64, vp, vp, vp]
    L.mrcnn_instance_map_source.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, vp, vp, vp, vp]
    L.mrcnn_render_detections_source.argtypes = [C.POINTER(Image), vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int,
                                                 C.c_int, vp, vp, vp]
    L.mrcnn_tile_plan.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(Tile), C.c_int, C.POINTER(C.c_int)]
    L.mrcnn_maskrcnn_predict_tiles.argtypes = [vp, C.POINTER(Image), C.c_int, C.POINTER(Tile), C.c_int, C.c_int, vp, vp]
    _merge = [vp, vp, C.POINTER(Tile), C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_double, C.c_int]
    L.mrcnn_merge_tiles.argtypes = _merge + [C.c_int, vp, vp, vp, vp, C.c_int64, vp, vp, vp]
    L.mrcnn_merge_tiles_host.argtypes = _merge + [vp, vp, vp, vp, C.c_int64, vp, vp, vp]
    L.mrcnn_unite_tiles.argtypes = _merge + [C.c_int, vp, vp, vp, vp, vp, vp, C.c_int64, vp, vp, vp]
    L.mrcnn_unite_tiles_host.argtypes = _merge + [vp, vp, vp, vp, vp, vp, C.c_int64, vp, vp, vp]
    _rles = [vp, vp, C.c_int, C.c_int]                          # counts, run_offsets, n_images, slots
    L.mrcnn_rle_decode.argtypes = _rles + [vp, vp, C.c_int, vp, vp]
    L.mrcnn_rle_decode_host.argtypes = _rles + [vp, vp, vp, vp]
    L.mrcnn_instance_map_rle.argtypes = [vp] + _rles + [vp, vp, C.c_float, C.c_int, vp, vp, vp]
    L.mrcnn_instance_map_rle_host.argtypes = [vp] + _rles + [vp, vp, C.c_float, vp, vp, vp]
    L.mrcnn_render_detections_rle.argtypes = [C.POINTER(Image), vp] + _rles + [C.c_float, C.c_int, C.c_int, C.c_int, vp, vp]
    L.mrcnn_render_detections_rle_host.argtypes = [C.POINTER(Image), vp] + _rles + [C.c_float, C.c_int, C.c_int, vp, vp]
    _rings = [vp, i64p, i64p, vp, vp, C.c_int64, vp, C.c_int64]    # rle_rings, n_rings, n_vertices, ring_offsets, ring_areas, capacity, xy, capacity
    L.mrcnn_rle_to_polygons.argtypes = _rles + [vp, vp, C.c_int] + _rings
    L.mrcnn_rle_to_polygons_host.argtypes = _rles + [vp, vp] + _rings
    _simple = [vp, vp, vp, vp, i64p, C.c_int64]                   # out_ring_offsets, out_areas2, out_xy, out_src_index, n_vertices_out, capacity
    L.mrcnn_polygons_simplify.argtypes = [vp, vp, C.c_int64, C.c_double, C.c_int] + _simple
    L.mrcnn_polygons_simplify_host.argtypes = [vp, vp, C.c_int64, C.c_double] + _simple
    _nest = [vp, vp, vp, vp, vp, i64p]                            # parent, depth, rle_polys, poly_rings, ring_order, n_polys
    L.mrcnn_polygons_nest.argtypes = [vp, C.c_int64, vp, vp, C.c_int64, C.c_int] + _nest
    L.mrcnn_polygons_nest_host.argtypes = [vp, C.c_int64, vp, vp, C.c_int64] + _nest
    _morph = [vp, C.c_int64, vp, vp, vp]                          # out_counts, capacity, out_run_offsets, areas, bboxes_xywh
    L.mrcnn_rle_morph.argtypes = [vp, vp, C.c_int64, vp, vp, vp, C.c_int, C.c_int] + _morph
    L.mrcnn_rle_morph_host.argtypes = [vp, vp, C.c_int64, vp, vp, vp, C.c_int] + _morph
    L.mrcnn_boundary_radius.argtypes = [C.c_int, C.c_int, C.c_double, vp]
    _cset = [vp, vp, C.c_int64, vp, vp, C.c_int, C.c_int]         # counts, run_offsets, n, heights, widths, connectivity, of
    _comps = [vp, vp, vp, vp, C.c_int64]                          # comp_offsets, comp_areas, comp_bboxes_xywh, comp_flags, comp_capacity
    L.mrcnn_rle_components.argtypes = _cset + [C.c_int] + _comps
    L.mrcnn_rle_components_host.argtypes = _cset + _comps
    _csel = _morph + [vp, i64p]                                   # ... out_parent, out_n
    L.mrcnn_rle_components_select.argtypes = _cset + [vp, C.c_int64, C.c_int, C.c_int] + _csel
    L.mrcnn_rle_components_select_host.argtypes = _cset + [vp, C.c_int64, C.c_int] + _csel
    _groups = [vp, vp, C.c_int64, C.c_int]                        # group_offsets, members, n_groups, op
    L.mrcnn_rle_combine.argtypes = [vp, vp, C.c_int64, vp, vp] + _groups + [C.c_int] + _morph
    L.mrcnn_rle_combine_host.argtypes = [vp, vp, C.c_int64, vp, vp] + _groups + _morph
    _xf = [vp, vp, vp]                                            # out_heights, out_widths, xf
    L.mrcnn_rle_transform.argtypes = [vp, vp, C.c_int64, vp, vp] + _xf + [C.c_int] + _morph
    L.mrcnn_rle_transform_host.argtypes = [vp, vp, C.c_int64, vp, vp] + _xf + _morph
    _hull = [vp, vp, vp, vp, i64p, C.c_int64]                     # hull_offsets, hull_areas2, obb, xy, n_vertices, vertex_capacity
    L.mrcnn_rle_measure.argtypes = [vp, vp, C.c_int64, vp, vp, C.c_int, vp]
    L.mrcnn_rle_measure_host.argtypes = [vp, vp, C.c_int64, vp, vp, vp]
    L.mrcnn_rle_convex_hull.argtypes = [vp, vp, C.c_int64, vp, vp, C.c_int] + _hull
    L.mrcnn_rle_convex_hull_host.argtypes = [vp, vp, C.c_int64, vp, vp] + _hull
    L.mrcnn_rle_to_string.argtypes = [vp, C.c_int64, vp, C.c_int64, i64p]
    L.mrcnn_rle_from_string.argtypes = [vp, C.c_int64, vp, C.c_int64, i64p]
    L.mrcnn_rle_iou.argtypes = [vp, vp, C.c_int64, vp, vp, C.c_int64, vp, vp, C.c_int, C.c_int, vp, vp, C.c_int64]
    L.mrcnn_box_iou_xywh.argtypes = [vp, C.c_int64, vp, C.c_int64, vp, vp, C.c_int, C.c_int, vp, C.c_int64]
    L.mrcnn_coco_match.argtypes = [vp, C.c_int64, C.c_int, vp, C.c_int, vp, vp, C.c_int64, vp, vp, vp, C.c_int64, vp, C.c_int, vp, C.c_int, vp, vp, vp]
    L.mrcnn_rle_from_polygons.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp, C.c_int64, i64p]
    L.mrcnn_rle_from_polygons_batch.argtypes = [vp, vp, vp, C.c_int64, vp, vp, C.c_int, vp, C.c_int64, vp, vp, vp]
    L.mrcnn_coco_accumulate.argtypes = [vp, vp, vp, vp, C.c_int64, vp, C.c_int, vp, C.c_int, C.c_int, vp, C.c_int, vp, C.c_int, C.c_int, vp, vp]
    i32p = C.POINTER(C.c_int32)
    L.mrcnn_jpeg_info.argtypes = [vp, C.c_int64, i32p, i32p, i32p, i32p, i32p]
    L.mrcnn_jpeg_decode_host.argtypes = [vp, C.c_int64, vp, C.c_int64]
    L.mrcnn_jpeg_decode_batch.argtypes = [C.POINTER(Jpeg), C.c_int, C.c_int, vp, vp, vp, vp]
    L.mrcnn_maskrcnn_predict_jpegs.argtypes = [vp, C.POINTER(Jpeg), C.c_int, C.c_int, vp, vp, vp, vp]
    L.mrcnn_jpeg_encode_host.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int64, C.POINTER(C.c_int64)]
    L.mrcnn_jpeg_encode_batch.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int64, vp]
    L.mrcnn_png_encode_host.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int64, C.POINTER(C.c_int64)]
    L.mrcnn_png_encode_batch.argtypes = [C.POINTER(PngSource), C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int64, vp]
    L.mrcnn_jpeg_last_stage_ms.argtypes = [f32p, f32p]
    L.mrcnn_jpeg_decode_batch_on.argtypes = [C.POINTER(Jpeg), C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]
    L.mrcnn_maskrcnn_predict_jpegs_on.argtypes = [vp, C.POINTER(Jpeg), C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]
    L.mrcnn_jpeg_coefficients.argtypes = [C.POINTER(Jpeg), C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int64, vp, vp]
    L.mrcnn_maskrcnn_predict_async.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp, vp]
    L.mrcnn_maskrcnn_submit.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int]
    L.mrcnn_maskrcnn_collect.argtypes = [vp, vp, vp, C.POINTER(C.c_int)]
    L.mrcnn_classifier_predict.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp]
    L.mrcnn_mask_predict.argtypes = [vp, vp, C.c_int, C.c_int, vp]
    L.mrcnn_model_get_int.argtypes = [vp, cp, i64p]
    L.mrcnn_model_read_tensor.argtypes = [vp, cp, C.c_int, vp, C.c_int64, i64p]
    L.mrcnn_model_enable_timing.argtypes = [vp, C.c_int]
    L.mrcnn_model_stage_ms.argtypes = [vp, cp, f32p]
    L.mrcnn_model_conv_profile_enable.argtypes = [vp, C.c_int]
    L.mrcnn_model_conv_profile_get.argtypes = [vp, C.c_int, i64p, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.mrcnn_model_conv_profile_group.argtypes = [vp, C.c_int, i64p, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.mrcnn_model_enable_graph.argtypes = [vp, C.c_int]
    L.mrcnn_model_conv_profile_bytes.argtypes = [vp, C.c_int, C.POINTER(C.c_double)]
    L.mrcnn_model_conv_profile_shapes.argtypes = [vp, C.POINTER(ConvShapeStat), C.c_int, C.POINTER(C.c_int)]
    L.mrcnn_bench_conv.argtypes = [C.c_int] * 8 + [f32p, C.POINTER(C.c_double)]
    L.mrcnn_bench_conv_dtype.argtypes = [C.c_int] * 9 + [f32p, C.POINTER(C.c_double)]
    L.mrcnn_detections_decode.argtypes = [vp, C.c_int64, C.c_int64, C.POINTER(DetectionRecord), C.c_int64, i64p]
    L.mrcnn_mask_to_u8.argtypes = [vp, C.c_int64, vp]
    L.mrcnn_mask_to_u8_f64.argtypes = [vp, C.c_int64, vp]
    ip = C.POINTER(C.c_int)
    L.mrcnn_letterbox_geometry.argtypes = [C.c_int] * 4 + [ip] * 4
    L.mrcnn_letterbox_rgb.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int]
    L.mrcnn_generate_anchors.argtypes = [C.c_int, C.c_int, vp, C.c_int64, i64p]
    L.mrcnn_paste_masks.argtypes = [vp, C.c_int64, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, vp]
    L.mrcnn_conv2d_nhwc.argtypes = [vp] + [C.c_int] * 4 + [vp] + [C.c_int] * 3 + [vp, vp, vp, C.c_int, C.c_int, vp]
    L.mrcnn_debug_set.argtypes = [cp, C.c_int]
    L.mrcnn_bench_mfma_probe.argtypes = [C.c_double, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.mrcnn_bottleneck_first_nhwc.argtypes = [vp] + [C.c_int] * 4 + [vp] * 5 + [C.c_int, C.c_int, vp, vp]
    L.mrcnn_bottleneck_stage_nhwc.argtypes = [vp] + [C.c_int] * 4 + [vp] * 4 + [C.c_int, C.c_int, vp, vp, vp]
    L.mrcnn_bottleneck_nhwc.argtypes = [vp] + [C.c_int] * 4 + [vp] * 9 + [C.c_int, C.c_int, vp, vp]
    L.mrcnn_test_last_range_flag.argtypes = [ip]
    L.mrcnn_conv_chain_nhwc.argtypes = [vp] + [C.c_int] * 4 + [vp] * 5 + [C.c_int, C.c_int] + [vp] * 6 + [C.c_int] * 3 + [vp, vp]
    L.mrcnn_test_chain_stream_image.argtypes = [vp, C.c_int, C.c_int, vp]
    L.mrcnn_classifier_rows.argtypes = [vp, C.c_int64, vp, C.c_int, C.c_int64, vp, vp]
    L.mrcnn_model_check_range.argtypes = [vp, ip]
    L.mrcnn_model_calibrate_split.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    L.mrcnn_model_split_group_stat.argtypes = [vp, C.c_int, C.POINTER(SplitGroupStat)]
    L.mrcnn_model_get_split_exponents.argtypes = [vp, vp, C.c_int, ip]
    L.mrcnn_model_set_split_exponents.argtypes = [vp, vp, C.c_int]
    L.mrcnn_dist_rccl_shared.argtypes = []
    L.mrcnn_dist_rccl_shared.restype = C.c_int
    L.mrcnn_dist_unique_id.argtypes = [vp]
    L.mrcnn_dist_init.argtypes = [C.c_int, C.c_int, vp, C.POINTER(vp)]
    L.mrcnn_dist_destroy.argtypes = [vp]
    L.mrcnn_dist_destroy.restype = None
    L.mrcnn_dist_shard.argtypes = [C.c_int, C.c_int, C.c_int, ip, ip]
    L.mrcnn_dist_record_floats.argtypes = [C.c_int, C.c_int]
    L.mrcnn_dist_record_floats.restype = C.c_int64
    L.mrcnn_dist_all_gather_records.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, vp, vp]
    L.mrcnn_maskrcnn_predict_sharded.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]
    L.mrcnn_dist_all_gather_records_async.argtypes = [vp, vp, vp, vp, C.c_int, vp, vp]
    L.mrcnn_dist_wait.argtypes = [vp]
    L.mrcnn_dist_recovered.argtypes = [vp, vp, C.POINTER(C.c_int)]
    L.mrcnn_dist_plan.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, i64p, i64p]
    L.mrcnn_dist_simulate_host.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(vp), C.POINTER(vp), vp, vp, vp, vp]
    L.mrcnn_roi_align_nhwc.argtypes = [C.POINTER(vp), ip, ip, C.c_int, C.c_int, vp, C.c_int64, C.c_int, C.c_int, C.c_double, C.c_double,
                                       C.c_int, vp, vp]
    L.mrcnn_test_roi_align_nhwc_batch.argtypes = [C.POINTER(vp), ip, ip, C.c_int, C.c_int, f32p, vp, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_double,
                                                  C.c_double, vp, vp]
    L.mrcnn_test_conv_form_nhwc.argtypes = [C.POINTER(ConvForm)]
    L.mrcnn_test_proposals_batch.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_float, vp, C.c_int64, vp]
    L.mrcnn_test_detections_batch.argtypes = [vp, vp, C.c_int, C.c_int, vp, C.c_int, C.c_float, C.c_float, vp, C.c_int64]
    L.mrcnn_test_mask_select_batch.argtypes = [C.POINTER(MaskSelect)]
    L.mrcnn_test_xf_preimage.argtypes = [C.c_int64] * 5 + [i64p, i64p]
    _lib = L
    return L


def check(status: int):
    if status != MRCNN_OK:
        raise MrcnnError(status, lib().mrcnn_last_error().decode(errors="replace"))


def make_params(d: dict):
    """dict → (Param array, n).  int → intValue, float → doubleValue, like task.py:25-67."""
    arr = (Param * max(1, len(d)))()
    keep = []
    for i, (k, v) in enumerate(d.items()):
        kb = str(k).encode()
        keep.append(kb)
        arr[i].key = kb
        if isinstance(v, bool) or isinstance(v, int):
            arr[i].type, arr[i].i = PARAM_INT, int(v)
        elif isinstance(v, float):
            arr[i].type, arr[i].d = PARAM_DOUBLE, float(v)
        else:
            sb = str(v).encode()
            keep.append(sb)
            arr[i].type, arr[i].s = PARAM_STRING, sb
    arr._keepalive = keep
    return arr, len(d)
