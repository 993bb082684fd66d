"""ctypes binding of include/arucohip.h (libarucohip.so). Fails loudly when the HIP library is missing —
there is no CPU fallback on the product path.

Import torch BEFORE this module when both are used in one process: torch bundles its own libamdhip64.so.7 and the
dynamic loader then resolves libarucohip's dependency to that already-loaded runtime (same SONAME), so device
pointers and streams can be shared between torch and the library.
"""
import ctypes as C
import os
import sys

import numpy as np

from .build import library_path

OK, E_INVALID, E_CAPACITY, E_UNSUPPORTED, E_HIP, E_OVERFLOW, E_BOARD_CONFIG = range(7)
THRES_FIXED, THRES_ADPT, THRES_CANNY = 0, 1, 2
CORNER_NONE, CORNER_HARRIS, CORNER_SUBPIX, CORNER_LINES = 0, 1, 2, 3
BOARD_NONE, BOARD_PIX, BOARD_METERS = -1, 0, 1
# arucohip_calibrate_*: the values of cv::CALIB_*
CALIB_USE_INTRINSIC_GUESS, CALIB_FIX_ASPECT_RATIO, CALIB_FIX_PRINCIPAL_POINT, CALIB_ZERO_TANGENT_DIST = 1, 2, 4, 8
CALIB_FIX_FOCAL_LENGTH, CALIB_FIX_K1, CALIB_FIX_K2, CALIB_FIX_K3 = 16, 32, 64, 128
CALIB_MAX_VIEW_POINTS = 512
# arucohip_fisheye_calibrate*
FISHEYE_USE_INTRINSIC_GUESS, FISHEYE_FIX_ASPECT_RATIO, FISHEYE_FIX_PRINCIPAL_POINT = 1, 2, 4
FISHEYE_FIX_K1, FISHEYE_FIX_K2, FISHEYE_FIX_K3, FISHEYE_FIX_K4 = 8, 16, 32, 64
# arucohip_board_map*: listed markers, listed markers used per frame
MAP_MAX_MARKERS, MAP_MAX_FRAME_MARKERS = 64, 16
# arucohip_rig_*: cameras of a rig, markers of its board
RIG_MAX_CAMERAS, RIG_MAX_BOARD = 16, 128

_ERR_NAMES = {1: "ARUCOHIP_E_INVALID", 2: "ARUCOHIP_E_CAPACITY", 3: "ARUCOHIP_E_UNSUPPORTED", 4: "ARUCOHIP_E_HIP",
              5: "ARUCOHIP_E_OVERFLOW", 6: "ARUCOHIP_E_BOARD_CONFIG"}


class ArucoHipError(RuntimeError):
    def __init__(self, code, msg=""):
        super().__init__("%s (%d): %s" % (_ERR_NAMES.get(code, "error"), code, msg))
        self.code = code


class Params(C.Structure):
    _fields_ = [("thres_method", C.c_int32), ("thres_param1_range", C.c_int32), ("thres_param1", C.c_double),
                ("thres_param2", C.c_double), ("corner_method", C.c_int32), ("warp_size", C.c_int32),
                ("min_size", C.c_float), ("max_size", C.c_float), ("border_dist", C.c_float),
                ("use_locked_corners", C.c_int32), ("decoder_kind", C.c_int32), ("erode", C.c_int32)]


class Marker(C.Structure):
    _fields_ = [("id", C.c_int32), ("corners", C.c_float * 8), ("ssize", C.c_float), ("has_pose", C.c_int32),
                ("pad_", C.c_int32), ("rvec", C.c_double * 3), ("tvec", C.c_double * 3)]


class BoardOut(C.Structure):
    _fields_ = [("n_markers", C.c_int32), ("has_pose", C.c_int32), ("rvec", C.c_double * 3), ("tvec", C.c_double * 3)]


class RigCamera(C.Structure):
    """arucohip_rig_camera_t: fixed intrinsics (in), calibrated and the transform rig -> camera (out of rig_calibrate, in of rig_pose)."""
    _fields_ = [("K", C.c_float * 9), ("dist", C.c_float * 5), ("ndist", C.c_int32), ("calibrated", C.c_int32), ("rvec", C.c_double * 3),
                ("tvec", C.c_double * 3)]


class PlanarPoses(C.Structure):
    """arucohip_planar_poses_t: both pose solutions of one marker, rms[0] <= rms[1]; n_solutions is 0 or 2."""
    _fields_ = [("rvec", (C.c_double * 3) * 2), ("tvec", (C.c_double * 3) * 2), ("rms", C.c_double * 2), ("n_solutions", C.c_int32),
                ("pad_", C.c_int32)]


class Overlay(C.Structure):
    """arucohip_overlay_t: what arucohip_draw_markers_batch draws (DRAW_* flags), the outline's width and its colour (B, G, R)."""
    _fields_ = [("flags", C.c_int32), ("line_width", C.c_int32), ("color", C.c_uint8 * 4)]


class Recover(C.Structure):
    """arucohip_recover_t: what board_recover_batch accepts (corner distance in pixels, differing cells of the 7 x 7 grid, board members a
    frame must already hold) and whether the recovered markers get their own pose."""
    _fields_ = [("max_corner_dist", C.c_float), ("max_cell_errors", C.c_int32), ("min_markers", C.c_int32), ("pose_markers", C.c_int32)]


DRAW_OUTLINE, DRAW_IDS, DRAW_AXIS, DRAW_CUBE, DRAW_Y_PERPENDICULAR = 1, 2, 4, 8, 16
class Charuco(C.Structure):
    """arucohip_charuco_t: the layout of a chessboard-corner board"""
    _fields_ = [("squares_x", C.c_int32), ("squares_y", C.c_int32), ("square_px", C.c_int32), ("marker_px", C.c_int32)]


class CharucoOpt(C.Structure):
    _fields_ = [("min_markers", C.c_int32), ("max_win", C.c_int32)]


class Fisheye(C.Structure):
    """arucohip_fisheye_t: the equidistant fisheye model, K row-major and D = k1..k4."""
    _fields_ = [("K", C.c_double * 9), ("D", C.c_double * 4)]


def fisheye_models(models):
    """A ctypes array of Fisheye from one (K, D) pair or a list of them; K is 3x3 or 9 values."""
    if len(models) == 2 and len(models[1]) == 4:   # one (K, D): D has four entries, a second model two
        models = [models]
    arr = (Fisheye * len(models))()
    for m, (K, D) in zip(arr, models):
        m.K[:] = [float(v) for v in np.asarray(K, np.float64).reshape(9)]
        m.D[:] = [float(v) for v in np.asarray(D, np.float64).reshape(4)]
    return arr


CHARUCO_CORNER_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("start_x", "<f4"), ("start_y", "<f4"), ("found", "<i4"), ("win", "<i4"),
                                 ("markers", "<i4"), ("pad_", "<i4")])
assert CHARUCO_CORNER_DTYPE.itemsize == 32

BOARD_DTYPE = np.dtype([("n_markers", "<i4"), ("has_pose", "<i4"), ("rvec", "<f8", (3,)), ("tvec", "<f8", (3,))])
assert C.sizeof(Overlay) == 12 and BOARD_DTYPE.itemsize == 56


class Rectify(C.Structure):
    """arucohip_rectify_t: a window of the board plane. Output pixel (u, v) shows the plane point (x0 + u ux + v vx, y0 + u uy + v vy)."""
    _fields_ = [("out_width", C.c_int32), ("out_height", C.c_int32), ("x0", C.c_float), ("y0", C.c_float), ("ux", C.c_float),
                ("uy", C.c_float), ("vx", C.c_float), ("vy", C.c_float)]


assert C.sizeof(Rectify) == 32


class Texture(C.Structure):
    """arucohip_texture_t: what arucohip_composite_plane_batch / arucohip_board_composite_batch lay on the plane. texture() fills one."""
    _fields_ = [("data", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32), ("channels", C.c_int32), ("on_device", C.c_int32),
                ("row_stride", C.c_size_t), ("frame_stride", C.c_size_t), ("opacity", C.c_int32), ("pad_", C.c_int32)]


assert C.sizeof(Texture) == 48


def texture(tex, opacity=255, per_frame=False):
    """The Texture of a contiguous uint8 numpy array or torch tensor: [H][W] or [H][W][C], or with per_frame [N][H][W] / [N][H][W][C] (frame
    f takes tex[f]). C is the frames' channels, or one more with straight alpha last. The record keeps a reference to the array."""
    shape = tuple(int(v) for v in (tex.shape[1:] if per_frame else tex.shape))
    assert len(shape) in (2, 3) and str(tex.dtype).endswith("uint8")
    ch = shape[2] if len(shape) == 3 else 1
    ptr, dev = Handle._buf(tex)
    t = Texture(ptr.value, shape[1], shape[0], ch, dev, shape[1] * ch, shape[0] * shape[1] * ch if per_frame else 0, int(opacity), 0)
    t.keep = tex
    return t


class Mesh(C.Structure):
    """arucohip_mesh_t: what arucohip_render_markers_batch / arucohip_render_boards_batch draw. mesh() fills one."""
    _fields_ = [("vertices", C.c_void_p), ("triangles", C.c_void_p), ("colors", C.c_void_p), ("nverts", C.c_int32), ("ntris", C.c_int32),
                ("on_device", C.c_int32), ("pad_", C.c_int32)]


class Render(C.Structure):
    """arucohip_render_t: RENDER_* flags, opacity and ambient 0..255, the scale, the direction towards the light (camera frame) and the
    colour (B, G, R) of a mesh without colours of its own. render_style() fills one."""
    _fields_ = [("flags", C.c_int32), ("opacity", C.c_int32), ("ambient", C.c_int32), ("scale", C.c_float), ("light", C.c_float * 3),
                ("color", C.c_uint8 * 4)]


assert C.sizeof(Mesh) == 40 and C.sizeof(Render) == 32
RENDER_CULL_BACK, RENDER_UNLIT, RENDER_EDGES_INT64 = 1, 2, 4


def mesh(vertices, triangles, colors=None):
    """The Mesh of float32 [nverts][3] vertices, int32 [ntris][3] indices and optional uint8 [ntris][3] B G R colours: numpy arrays
    (converted where needed) or contiguous torch tensors on the device, all of one kind. The record keeps references to the arrays."""
    if isinstance(vertices, (np.ndarray, list, tuple)):
        vertices = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
        triangles = np.ascontiguousarray(triangles, dtype=np.int32).reshape(-1, 3)
        colors = None if colors is None else np.ascontiguousarray(colors, dtype=np.uint8).reshape(-1, 3)
    assert colors is None or len(colors) == len(triangles)
    (vp, vd), (tp, td) = Handle._buf(vertices), Handle._buf(triangles)
    cp, cd = (None, vd) if colors is None else Handle._buf(colors)
    assert vd == td == cd
    m = Mesh(vp.value, tp.value, cp.value if cp is not None else None, len(vertices), len(triangles), vd, 0)
    m._keep = (vertices, triangles, colors)
    return m


def render_style(flags=RENDER_CULL_BACK, opacity=255, ambient=64, scale=1.0, light=(0.0, 0.0, -1.0), color=(0, 200, 0)):
    return Render(int(flags), int(opacity), int(ambient), float(scale), (C.c_float * 3)(*[float(v) for v in light]),
                  (C.c_uint8 * 4)(*[int(c) for c in color][:3], 0))


def cube_mesh():
    """The unit cube on the pose's plane: [-0.5, 0.5]^2 x [0, 1], 8 vertices, 12 outward (counter-clockwise) triangles."""
    v = np.array([[x, y, z] for z in (0.0, 1.0) for y in (-0.5, 0.5) for x in (-0.5, 0.5)], np.float32)
    quads = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]
    t = np.array([tri for a, b, c, d in quads for tri in ((a, b, c), (a, c, d))], np.int32)
    return v, t


def uv_sphere_mesh(stacks, slices, radius=0.5, center=(0.0, 0.0, 0.5)):
    """A latitude / longitude sphere: 2 + (stacks - 1) * slices vertices, 2 * slices * (stacks - 1) outward triangles."""
    assert stacks >= 2 and slices >= 3
    v = [(0.0, 0.0, 1.0)]
    for i in range(1, stacks):
        th = np.pi * i / stacks
        for j in range(slices):
            ph = 2.0 * np.pi * j / slices
            v.append((np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)))
    v.append((0.0, 0.0, -1.0))
    ring = lambda i, j: 1 + (i - 1) * slices + j % slices   # noqa: E731
    south = len(v) - 1
    t = []
    for j in range(slices):
        t.append((0, ring(1, j), ring(1, j + 1)))
        for i in range(1, stacks - 1):
            t.append((ring(i, j), ring(i + 1, j), ring(i + 1, j + 1)))
            t.append((ring(i, j), ring(i + 1, j + 1), ring(i, j + 1)))
        t.append((south, ring(stacks - 1, j + 1), ring(stacks - 1, j)))
    return (np.asarray(v, np.float64) * radius + np.asarray(center, np.float64)).astype(np.float32), np.asarray(t, np.int32)


class FrameFormat(C.Structure):
    """arucohip_frame_format_t: how a caller's frames are stored (camera-native input). bits belongs to GRAY16, chroma_offset to NV12."""
    _fields_ = [("format", C.c_int32), ("bits", C.c_int32), ("chroma_offset", C.c_uint64)]

    def min_row_stride(self, width):
        """Bytes of a row that are read (0: invalid format, bits or width)."""
        return int(load().arucohip_frame_min_row_stride(C.byref(self), int(width)))

    def min_stride(self, width, height, row_stride=None):
        """Bytes of one frame from its first to its last byte read (0: invalid)."""
        rs = self.min_row_stride(width) if row_stride is None else row_stride
        return int(load().arucohip_frame_min_stride(C.byref(self), int(width), int(height), rs))


# arucohip_pixel_format
(PIX_GRAY8, PIX_BGR8, PIX_RGB8, PIX_BGRA8, PIX_RGBA8, PIX_GRAY16, PIX_YUYV, PIX_UYVY, PIX_NV12, PIX_BAYER_RGGB, PIX_BAYER_BGGR, PIX_BAYER_GRBG,
 PIX_BAYER_GBRG) = range(13)
EXPORT_GREY_IS_LUMA = 1   # arucohip_export_batch: a grey source is the Y of a YUV destination as it lies
PIX_NAMES = ("GRAY8", "BGR8", "RGB8", "BGRA8", "RGBA8", "GRAY16", "YUYV", "UYVY", "NV12", "BAYER_RGGB", "BAYER_BGGR", "BAYER_GRBG", "BAYER_GBRG")


def frame_format(fmt, bits=0, chroma_offset=0):
    """A FrameFormat from a PIX_* value or its name ("NV12", "BAYER_RGGB", ...)."""
    return FrameFormat(PIX_NAMES.index(fmt.upper()) if isinstance(fmt, str) else int(fmt), int(bits), int(chroma_offset))


def gray16(bits=16):
    return FrameFormat(PIX_GRAY16, int(bits), 0)


def nv12(chroma_offset=0):
    return FrameFormat(PIX_NV12, 0, int(chroma_offset))


def bayer(pattern):
    """pattern: the top-left 2 x 2 block row by row, "RGGB", "BGGR", "GRBG" or "GBRG"."""
    return frame_format("BAYER_" + pattern)


class Limits(C.Structure):
    _fields_ = [("max_width", C.c_int32), ("max_height", C.c_int32), ("max_batch", C.c_int32),
                ("max_thres_planes", C.c_int32), ("triggers_per_frame", C.c_int32), ("contours_per_frame", C.c_int32),
                ("points_per_frame", C.c_int32), ("candidates_per_frame", C.c_int32), ("markers_per_frame", C.c_int32),
                ("long_walks_per_plane", C.c_int32)]


# arucohip_debug_plane_counters: words of a plane's line; [PC_SEGMENTS] = 1 on a handle of the waypoint-segment pipeline
PLANE_COUNTER_WORDS, PC_SEGMENTS = 36, 35

MARKER_DTYPE = np.dtype([("id", "<i4"), ("corners", "<f4", (8,)), ("ssize", "<f4"), ("has_pose", "<i4"),
                         ("pad_", "<i4"), ("rvec", "<f8", (3,)), ("tvec", "<f8", (3,))])
assert MARKER_DTYPE.itemsize == 96 and C.sizeof(Marker) == 96
# numpy view of a PlanarPoses array: np.frombuffer(array, PLANAR_DTYPE)
PLANAR_DTYPE = np.dtype([("rvec", "<f8", (2, 3)), ("tvec", "<f8", (2, 3)), ("rms", "<f8", (2,)), ("n_solutions", "<i4"), ("pad_", "<i4")])
assert PLANAR_DTYPE.itemsize == 120 and C.sizeof(PlanarPoses) == 120

# every symbol include/arucohip.h declares
SYMBOLS = [
    "arucohip_version", "arucohip_default_params", "arucohip_default_limits", "arucohip_create", "arucohip_create_ex",
    "arucohip_destroy", "arucohip_set_params", "arucohip_get_params", "arucohip_last_error_string", "arucohip_set_stream",
    "arucohip_get_stream", "arucohip_synchronize", "arucohip_detect", "arucohip_detect_batch", "arucohip_batch_status", "arucohip_batch_chunks",
    "arucohip_get_thresholded", "arucohip_get_candidates", "arucohip_threshold", "arucohip_detect_rectangles",
    "arucohip_warp", "arucohip_debug_num_contours", "arucohip_debug_contour", "arucohip_debug_candidates", "arucohip_debug_otsu",
    "arucohip_debug_cells", "arucohip_debug_start_candidates",
    "arucohip_debug_threshold_batch", "arucohip_debug_threshold_plan", "arucohip_debug_threshold_plane",
    "arucohip_board_detect", "arucohip_calculate_extrinsics", "arucohip_stage_times", "arucohip_stage_name",
    "arucohip_enable_timing", "arucohip_kernel_times", "arucohip_threshold_exec_ms", "arucohip_kernel_name",
    "arucohip_debug_counters", "arucohip_debug_plane_counters", "arucohip_board_detect_batch",
    "arucohip_gl_modelview", "arucohip_ogre_pose", "arucohip_gl_projection", "arucohip_ogre_projection",
    "arucohip_detect_bgr", "arucohip_detect_batch_bgr", "arucohip_bgr_to_gray", "arucohip_set_dictionary",
    "arucohip_set_decoder_callback",
    "arucohip_undistort", "arucohip_gl_modelview_n", "arucohip_gl_modelview_batch",
    "arucohip_set_pipeline_depth", "arucohip_detect_batch_submit", "arucohip_detect_batch_wait",
    "arucohip_mgpu_device_count", "arucohip_mgpu_create", "arucohip_mgpu_destroy", "arucohip_mgpu_size", "arucohip_mgpu_handle",
    "arucohip_mgpu_set_params", "arucohip_mgpu_last_error_string", "arucohip_mgpu_detect_batch", "arucohip_mgpu_detect_streams",
    "arucohip_mgpu_set_depth", "arucohip_mgpu_submit_batch", "arucohip_mgpu_submit_streams", "arucohip_mgpu_wait",
    "arucohip_compact_bytes", "arucohip_compact_markers", "arucohip_wait_event", "arucohip_detect_batch_retry_overflowed",
    "arucohip_refine_candidate_lines", "arucohip_debug_refine_pixels", "arucohip_debug_decode_quads", "arucohip_debug_marker_tail", "arucohip_mgpu_gather_mode", "arucohip_build_info",
    "arucohip_calibrate_camera", "arucohip_calibrate_board_batch", "arucohip_debug_calib_start", "arucohip_board_map", "arucohip_board_map_batch",
    "arucohip_rig_calibrate", "arucohip_rig_calibrate_batch", "arucohip_rig_pose", "arucohip_rig_pose_batch",
    "arucohip_planar_poses", "arucohip_planar_poses_batch",
    "arucohip_chromatic_board_corners", "arucohip_chromatic_create", "arucohip_chromatic_destroy", "arucohip_chromatic_train",
    "arucohip_chromatic_classify", "arucohip_chromatic_update", "arucohip_chromatic_get_mask", "arucohip_chromatic_get_cell_map",
    "arucohip_chromatic_is_valid", "arucohip_chromatic_get_model", "arucohip_chromatic_set_model", "arucohip_em_fit",
    "arucohip_chromatic_debug_geometry", "arucohip_chromatic_debug_hist", "arucohip_chromatic_classify_batch", "arucohip_chromatic_grid",
    "arucohip_chromatic_reset_mask",
    "arucohip_hrm_create_dictionary", "arucohip_hrm_board_size", "arucohip_hrm_board_image", "arucohip_debug_hrm_stream",
    "arucohip_debug_hrm_counters",
    "arucohip_fiducial_marker_images", "arucohip_fiducial_marker_side", "arucohip_fiducial_marker_mat", "arucohip_fiducial_shuffle_ids",
    "arucohip_fiducial_board_size", "arucohip_fiducial_board_image", "arucohip_board_pix_to_meters", "arucohip_fiducial_distances",
    "arucohip_fiducial_select", "arucohip_board_place",
    "arucohip_draw_markers_batch", "arucohip_draw_boards_batch",
    "arucohip_set_pyr_down", "arucohip_get_pyr_down", "arucohip_pyr_down",
    "arucohip_default_recover", "arucohip_board_recover_batch",
    "arucohip_default_charuco", "arucohip_charuco_board_size", "arucohip_charuco_board_image", "arucohip_charuco_corners_batch",
    "arucohip_charuco_calibrate_batch", "arucohip_charuco_pose_batch",
    "arucohip_fisheye_undistort_points", "arucohip_fisheye_distort_points", "arucohip_fisheye_undistort",
    "arucohip_fisheye_undistort_markers_batch", "arucohip_fisheye_calibrate", "arucohip_fisheye_calibrate_board_batch",
    "arucohip_warp_plane_batch", "arucohip_rectify_board_window", "arucohip_board_rectify_batch",
    "arucohip_composite_plane_batch", "arucohip_board_composite_batch",
    "arucohip_default_render", "arucohip_render_markers_batch", "arucohip_render_boards_batch", "arucohip_render_times",
    "arucohip_frame_min_row_stride", "arucohip_frame_min_stride", "arucohip_convert_batch", "arucohip_export_batch",
]

_lib = None


def load():
    """dlopen libarucohip.so; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    # ARUCOHIP_LIB: an experiment's variant build (tools/ab_variants.sh, tools/stage_cost.sh) is loaded from its own path; the product
    # library in the tree is never overwritten
    path = os.environ.get("ARUCOHIP_LIB") or library_path()
    if "torch" not in sys.modules:
        # One HIP runtime per process: torch ships its own libamdhip64.so.7; when torch is importable load it first so
        # that libarucohip binds to the same runtime (two runtimes in one process cannot both own the GPU).
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    if not os.path.exists(path):
        raise ArucoHipError(E_HIP, "libarucohip.so is not built (%s); run aruco_amd.build_library()" % path)
    L = C.CDLL(path, mode=C.RTLD_GLOBAL)
    L.arucohip_last_error_string.restype = C.c_char_p
    L.arucohip_build_info.restype = C.c_char_p
    L.arucohip_stage_name.restype = C.c_char_p
    L.arucohip_kernel_name.restype = C.c_char_p
    L.arucohip_get_stream.restype = C.c_void_p
    vp, i, f, sz = C.c_void_p, C.c_int, C.c_float, C.c_size_t
    L.arucohip_create.argtypes = [vp, i, i, i, i, vp]
    L.arucohip_create_ex.argtypes = [vp, i, vp, vp]
    L.arucohip_destroy.argtypes = [vp]
    L.arucohip_set_params.argtypes = [vp, vp]
    L.arucohip_get_params.argtypes = [vp, vp]
    L.arucohip_last_error_string.argtypes = [vp]
    L.arucohip_set_stream.argtypes = [vp, vp]
    L.arucohip_get_stream.argtypes = [vp]
    L.arucohip_synchronize.argtypes = [vp]
    L.arucohip_detect.argtypes = [vp, vp, i, i, sz, vp, vp, i, f, i, vp, i, vp]
    L.arucohip_detect_batch.argtypes = [vp, vp, i, i, i, sz, sz, i, vp, vp, i, f, i, vp, i, vp, i]
    L.arucohip_batch_status.argtypes = [vp]
    L.arucohip_batch_chunks.argtypes = [vp, C.POINTER(C.c_int)]
    L.arucohip_get_thresholded.argtypes = [vp, i, vp]
    L.arucohip_get_candidates.argtypes = [vp, i, vp, i, vp]
    L.arucohip_threshold.argtypes = [vp, i, vp, i, i, sz, C.c_double, C.c_double, vp]
    L.arucohip_detect_rectangles.argtypes = [vp, vp, i, i, sz, vp, i, vp]
    L.arucohip_warp.argtypes = [vp, vp, i, i, sz, vp, i, vp]
    L.arucohip_debug_num_contours.argtypes = [vp, i, vp]
    L.arucohip_debug_contour.argtypes = [vp, i, i, vp, vp, vp, vp, i, vp]
    L.arucohip_debug_candidates.argtypes = [vp, i, vp, vp, vp, i, vp]
    L.arucohip_board_detect.argtypes = [vp, vp, i, vp, vp, i, i, vp, vp, i, f, f, i, vp, vp, vp]
    L.arucohip_calculate_extrinsics.argtypes = [vp, vp, i, vp, vp, i, f, i]
    L.arucohip_stage_times.argtypes = [vp, vp, i]
    L.arucohip_stage_name.argtypes = [i]
    L.arucohip_enable_timing.argtypes = [vp, i]
    L.arucohip_kernel_times.argtypes = [vp, vp, i]
    L.arucohip_threshold_exec_ms.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_int)]
    L.arucohip_kernel_name.argtypes = [i]
    L.arucohip_debug_counters.argtypes = [vp, vp]
    L.arucohip_debug_plane_counters.argtypes = [vp, C.c_int, vp, C.c_int]
    L.arucohip_debug_start_candidates.argtypes = [vp, i, i, vp, i, vp]
    L.arucohip_debug_threshold_batch.argtypes = [vp, vp, i, i, i, C.c_size_t, C.c_size_t, i, i]
    L.arucohip_debug_threshold_plan.argtypes = [vp, vp, i, vp]
    L.arucohip_debug_threshold_plane.argtypes = [vp, i, i, vp, vp, vp]
    L.arucohip_board_detect_batch.argtypes = [vp, i, vp, vp, i, i, vp, vp, i, f, f, i, vp, vp]
    L.arucohip_default_recover.argtypes = [vp]
    L.arucohip_default_recover.restype = None
    L.arucohip_board_recover_batch.argtypes = [vp, i, vp, vp, i, i, vp, vp, i, f, f, i, vp, vp, i, vp, i, vp, vp, vp]
    L.arucohip_calibrate_camera.argtypes = [vp, vp, vp, vp, i, i, i, i, i, vp, vp, vp, vp, vp, vp]
    L.arucohip_debug_calib_start.argtypes = [vp, vp, vp, vp, i, i, i, i, i, i, vp, vp, vp, vp, vp, vp]
    L.arucohip_calibrate_board_batch.argtypes = [vp, i, vp, vp, i, i, f, i, i, i, i, vp, vp, vp, vp, vp, vp]
    L.arucohip_board_map.argtypes = [vp, vp, vp, vp, i, i, i, vp, i, vp, vp, i, f] + [vp] * 10
    L.arucohip_board_map_batch.argtypes = [vp, i, vp, i, vp, vp, i, f, i] + [vp] * 10
    L.arucohip_rig_calibrate.argtypes = [vp, vp, vp, vp, i, i, i, vp, i, vp, vp, i, i, f, i] + [vp] * 6
    L.arucohip_rig_calibrate_batch.argtypes = [vp, i, vp, i, vp, vp, i, i, f, i] + [vp] * 6
    L.arucohip_rig_pose.argtypes = [vp, vp, vp, vp, i, i, i, vp, i, vp, vp, i, i, f, i, vp, vp]
    L.arucohip_rig_pose_batch.argtypes = [vp, i, vp, i, vp, vp, i, i, f, i, vp, vp]
    L.arucohip_planar_poses.argtypes = [vp, vp, i, i, vp, vp, i, f, i, i, vp]
    L.arucohip_planar_poses_batch.argtypes = [vp, i, vp, vp, i, f, i, i, vp, i, i]
    L.arucohip_draw_markers_batch.argtypes = [vp, vp, i, i, i, i, sz, sz, i, vp, i, vp, i, vp, vp, i, vp]
    L.arucohip_draw_boards_batch.argtypes = [vp, vp, i, i, i, i, sz, sz, i, vp, i, f, vp, vp, i, i]
    d = C.c_double
    L.arucohip_chromatic_board_corners.argtypes = [vp, i, i, f, vp]
    L.arucohip_chromatic_create.argtypes = [vp, i, i, d, vp, vp, i, i, i, vp, vp]
    L.arucohip_chromatic_destroy.argtypes = [vp]
    L.arucohip_chromatic_train.argtypes = [vp, vp, i, sz, vp, vp]
    L.arucohip_chromatic_classify.argtypes = [vp, vp, i, sz, vp, vp, i]
    L.arucohip_chromatic_update.argtypes = [vp, vp, i, sz]
    L.arucohip_chromatic_grid.argtypes = [vp, vp, vp]
    L.arucohip_chromatic_reset_mask.argtypes = [vp]
    L.arucohip_chromatic_get_mask.argtypes = [vp, vp, i]
    L.arucohip_chromatic_get_cell_map.argtypes = [vp, vp, i]
    L.arucohip_chromatic_is_valid.argtypes = [vp]
    L.arucohip_chromatic_get_model.argtypes = [vp, vp, vp]
    L.arucohip_chromatic_set_model.argtypes = [vp, vp, vp]
    L.arucohip_em_fit.argtypes = [vp, vp, d, vp, vp, vp]
    L.arucohip_hrm_create_dictionary.argtypes = [vp, i, i, C.c_uint32, vp, vp, vp]
    L.arucohip_hrm_board_size.argtypes = [i, i, i, i, vp, vp, vp]
    L.arucohip_hrm_board_image.argtypes = [vp, i, i, vp, i, i, i, vp, sz, i, vp, vp]
    L.arucohip_debug_hrm_stream.argtypes = [vp, C.c_uint32, C.c_uint64, i, vp]
    L.arucohip_debug_hrm_counters.argtypes = [vp, vp]
    L.arucohip_fiducial_marker_images.argtypes = [vp, vp, i, i, i, vp, sz, sz, i]
    L.arucohip_fiducial_marker_side.argtypes = [i, i]
    L.arucohip_fiducial_marker_mat.argtypes = [i, vp]
    L.arucohip_fiducial_shuffle_ids.argtypes = [vp, i, vp, i, vp]
    L.arucohip_fiducial_board_size.argtypes = [i, i, i, i, i, vp, vp, vp, vp]
    L.arucohip_fiducial_board_image.argtypes = [vp, i, i, i, i, i, i, vp, i, vp, sz, i, vp]
    L.arucohip_board_pix_to_meters.argtypes = [vp, i, f, vp]
    L.arucohip_board_place.argtypes = [vp, i, vp, vp, vp]
    L.arucohip_fiducial_distances.argtypes = [vp, vp, i]
    L.arucohip_fiducial_select.argtypes = [vp, i, i, vp, vp, vp]
    L.arucohip_chromatic_debug_geometry.argtypes = [vp, i, vp, vp, vp]
    L.arucohip_chromatic_debug_hist.argtypes = [vp, vp, vp, vp]
    L.arucohip_chromatic_classify_batch.argtypes = [vp, vp, vp, i, i, i, sz, sz, i, i, f, vp, i, vp]
    L.arucohip_detect_bgr.argtypes = [vp, vp, i, i, sz, vp, vp, i, f, i, vp, i, vp]
    L.arucohip_detect_batch_bgr.argtypes = [vp, vp, i, i, i, sz, sz, i, vp, vp, i, f, i, vp, i, vp, i]
    L.arucohip_bgr_to_gray.argtypes = [vp, vp, i, i, sz, vp]
    L.arucohip_set_dictionary.argtypes = [vp, i, i, vp, i, f]
    L.arucohip_undistort.argtypes = [vp, vp, i, i, i, sz, sz, i, i, vp, vp, i, vp, i]
    L.arucohip_set_pyr_down.argtypes = [vp, i]
    L.arucohip_get_pyr_down.argtypes = [vp]
    L.arucohip_pyr_down.argtypes = [vp, vp, i, i, i, sz, sz, i, i, vp, i]
    L.arucohip_gl_modelview.argtypes = [vp, vp, vp]
    L.arucohip_gl_modelview_n.argtypes = [vp, i, vp]
    L.arucohip_gl_modelview_batch.argtypes = [vp, i, i, vp, vp]
    L.arucohip_ogre_pose.argtypes = [vp, vp, vp, vp]
    L.arucohip_gl_projection.argtypes = [vp, i, i, i, i, C.c_double, C.c_double, i, vp]
    L.arucohip_ogre_projection.argtypes = [vp, i, i, i, i, C.c_double, C.c_double, i, vp]
    L.arucohip_set_decoder_callback.argtypes = [vp, vp, vp]
    L.arucohip_set_pipeline_depth.argtypes = [vp, i]
    L.arucohip_detect_batch_submit.argtypes = [vp, vp, i, i, i, sz, sz, i, vp, vp, i, f, i, vp, i, vp, i, vp]
    L.arucohip_detect_batch_wait.argtypes = [vp, i]
    L.arucohip_mgpu_create.argtypes = [vp, vp, i, i, i, i, i, i, vp]
    L.arucohip_mgpu_destroy.argtypes = [vp]
    L.arucohip_mgpu_destroy.restype = None
    L.arucohip_mgpu_size.argtypes = [vp]
    L.arucohip_mgpu_handle.argtypes = [vp, i]
    L.arucohip_mgpu_handle.restype = vp
    L.arucohip_mgpu_set_params.argtypes = [vp, vp]
    L.arucohip_mgpu_last_error_string.argtypes = [vp]
    L.arucohip_mgpu_last_error_string.restype = C.c_char_p
    L.arucohip_mgpu_detect_batch.argtypes = [vp, vp, i, i, i, sz, sz, vp, vp, i, f, i, vp, i, vp]
    L.arucohip_mgpu_detect_streams.argtypes = [vp, vp, vp, i, i, sz, sz, vp, vp, i, f, i, vp, i, vp]
    L.arucohip_mgpu_set_depth.argtypes = [vp, i]
    L.arucohip_mgpu_submit_batch.argtypes = [vp, vp, i, i, i, sz, sz, vp, vp, i, f, i, vp, i, vp, vp]
    L.arucohip_mgpu_submit_streams.argtypes = [vp, vp, vp, i, i, sz, sz, vp, vp, i, f, i, vp, i, vp, vp]
    L.arucohip_mgpu_wait.argtypes = [vp, i]
    L.arucohip_mgpu_gather_mode.argtypes = [vp]
    L.arucohip_compact_bytes.argtypes = [i, i]
    L.arucohip_compact_bytes.restype = sz
    L.arucohip_compact_markers.argtypes = [vp, vp, i, i, vp, i, vp]
    L.arucohip_wait_event.argtypes = [vp, vp]
    L.arucohip_detect_batch_retry_overflowed.argtypes = [vp, vp, i, i, i, sz, sz, i, vp, vp, i, f, i, vp, i, vp, i, vp]
    L.arucohip_refine_candidate_lines.argtypes = [vp, vp, i, vp, vp, vp, i]
    L.arucohip_debug_refine_pixels.argtypes = [vp, vp, i, i, C.c_size_t, vp, i, i, i, i]
    L.arucohip_debug_decode_quads.argtypes = [vp, vp, i, i, i, C.c_size_t, vp, vp, i, vp, vp, vp, vp, vp, vp, vp, vp]
    L.arucohip_debug_marker_tail.argtypes = [vp, i, i, i, vp, vp, vp, i, vp, vp, vp, i, f, i, vp, i, vp, vp, vp, vp, vp, vp, vp]
    L.arucohip_default_charuco.argtypes = [vp]
    L.arucohip_default_charuco.restype = None
    L.arucohip_charuco_board_size.argtypes = [vp, vp, vp, vp, vp]
    L.arucohip_charuco_board_image.argtypes = [vp, vp, i, vp, i, vp, sz, i, vp, vp]
    L.arucohip_charuco_corners_batch.argtypes = [vp, vp, vp, i, vp, i, i, i, sz, sz, i, vp, vp, vp, i]
    L.arucohip_charuco_calibrate_batch.argtypes = [vp, f, i, i, i, i, vp, vp, vp, vp, vp, vp]
    L.arucohip_charuco_pose_batch.argtypes = [vp, i, vp, vp, i, f, i, i, vp]
    L.arucohip_fisheye_undistort_points.argtypes = [vp, vp, vp, f, vp, i, i, vp, vp]
    L.arucohip_fisheye_distort_points.argtypes = [vp, vp, vp, vp, i, i, vp]
    L.arucohip_fisheye_undistort.argtypes = [vp, vp, i, i, i, sz, sz, i, i, vp, vp, f, vp, i]
    L.arucohip_fisheye_undistort_markers_batch.argtypes = [vp, i, vp, i, vp, f, vp, i, vp, i, vp]
    L.arucohip_fisheye_calibrate.argtypes = [vp, vp, vp, vp, i, i, i, i, i, vp, vp, vp, vp, vp]
    L.arucohip_fisheye_calibrate_board_batch.argtypes = [vp, i, vp, vp, i, i, f, i, i, i, i, vp, vp, vp, vp, vp]
    L.arucohip_warp_plane_batch.argtypes = [vp, vp, i, i, i, i, sz, sz, i, vp, vp, i, vp, vp, i, vp, i, i, sz, sz, i]
    L.arucohip_rectify_board_window.argtypes = [vp, i, i, f, f, f, i, vp]
    L.arucohip_board_rectify_batch.argtypes = [vp, vp, i, i, i, i, sz, sz, i, vp, i, vp, vp, i, vp, vp, sz, sz, i, vp, vp]
    L.arucohip_composite_plane_batch.argtypes = [vp, vp, i, i, i, i, sz, sz, i, vp, vp, vp, i, vp, vp, i, vp, i]
    L.arucohip_board_composite_batch.argtypes = [vp, vp, i, i, i, i, sz, sz, i, vp, i, vp, vp, i, vp, vp, vp, i, vp, vp]
    L.arucohip_default_render.argtypes = [vp]
    L.arucohip_default_render.restype = None
    L.arucohip_render_markers_batch.argtypes = [vp, vp, i, i, i, i, sz, sz, i, vp, i, vp, i, vp, vp, i, vp, vp, vp, i]
    L.arucohip_render_boards_batch.argtypes = [vp, vp, i, i, i, i, sz, sz, i, vp, i, vp, vp, i, vp, vp, vp, i]
    L.arucohip_render_times.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.arucohip_frame_min_row_stride.argtypes = [vp, i]
    L.arucohip_frame_min_row_stride.restype = sz
    L.arucohip_frame_min_stride.argtypes = [vp, i, i, sz]
    L.arucohip_frame_min_stride.restype = sz
    L.arucohip_convert_batch.argtypes = [vp, vp, vp, i, i, i, sz, sz, i, i, vp, sz, sz, i]
    L.arucohip_export_batch.argtypes = [vp, vp, i, i, i, i, sz, sz, i, vp, i, vp, sz, sz, i]
    L.arucohip_default_params.argtypes = [vp]
    L.arucohip_default_limits.argtypes = [vp, i, i, i]
    _lib = L
    return L


def build_info():
    """arucohip_build_info(): 'src=<digest> flags=[...]' of the loaded library."""
    return (load().arucohip_build_info() or b"").decode()


def compact_bytes(nframes, cap_total):
    """Size of the packed gather block of arucohip_compact_markers."""
    return int(load().arucohip_compact_bytes(int(nframes), int(cap_total)))


def compact_markers(blocks_ptr, counts_ptr, nframes, cap, dst_ptr, cap_total, stream_ptr=0):
    """arucohip_compact_markers on device pointers (plain integers) and a HIP stream pointer."""
    rc = load().arucohip_compact_markers(C.c_void_p(blocks_ptr), C.c_void_p(counts_ptr), int(nframes), int(cap), C.c_void_p(dst_ptr), int(cap_total),
                                          C.c_void_p(stream_ptr))
    if rc != OK:
        raise ArucoHipError(rc, "arucohip_compact_markers")


def default_params():
    p = Params()
    load().arucohip_default_params(C.byref(p))
    return p


def default_recover():
    o = Recover()
    load().arucohip_default_recover(C.byref(o))
    return o


def default_charuco():
    o = CharucoOpt()
    load().arucohip_default_charuco(C.byref(o))
    return o


def charuco_layout(squares, square_px, marker_px):
    return Charuco(int(squares[0]), int(squares[1]), int(square_px), int(marker_px))


def charuco_board_size(layout):
    """(width, height, markers, inner corners) of a chessboard-corner layout (host arithmetic, no handle)."""
    w, hh, nm, nc = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    rc = load().arucohip_charuco_board_size(C.byref(layout), C.byref(w), C.byref(hh), C.byref(nm), C.byref(nc))
    if rc != OK:
        raise ArucoHipError(rc, "arucohip_charuco_board_size")
    return w.value, hh.value, nm.value, nc.value


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


FIDUCIAL_PANEL, FIDUCIAL_CHESSBOARD, FIDUCIAL_FRAME = 0, 1, 2


def fiducial_marker_mat(marker_id):
    """FiducidalMarkers::getMarkerMat: the 5 x 5 cells of a marker as uint8 0 / 1 (host arithmetic, no handle)."""
    out = np.zeros((5, 5), np.uint8)
    rc = load().arucohip_fiducial_marker_mat(int(marker_id), _ptr(out))
    if rc != OK:
        raise ArucoHipError(rc, "arucohip_fiducial_marker_mat")
    return out


def fiducial_marker_side(size, locked=False):
    """Side of createMarkerImage(id, size, ., locked); 0 for a size the library refuses."""
    return int(load().arucohip_fiducial_marker_side(int(size), int(bool(locked))))


def fiducial_shuffle_ids(rng_state, n, excluded=()):
    """getListOfValidMarkersIds_random on cv::theRNG() with state rng_state: (ids int32 [n], the state afterwards)."""
    st = C.c_uint64(int(rng_state) & 0xFFFFFFFFFFFFFFFF)
    ex = np.ascontiguousarray(excluded, dtype=np.int32).reshape(-1)
    out = np.zeros(max(int(n), 1), np.int32)
    rc = load().arucohip_fiducial_shuffle_ids(C.byref(st), int(n), _ptr(ex) if ex.size else None, ex.size, _ptr(out))
    if rc != OK:
        raise ArucoHipError(rc, "arucohip_fiducial_shuffle_ids")
    return out[:max(int(n), 0)], int(st.value)


def fiducial_board_size(board_type, grid, marker_size, marker_distance=0):
    """(width, height, ids the reference draws from the shuffle, markers placed) of a board layout (FIDUCIAL_*)."""
    w, hh, drawn, nm = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    rc = load().arucohip_fiducial_board_size(int(board_type), int(grid[0]), int(grid[1]), int(marker_size), int(marker_distance), C.byref(w),
                                             C.byref(hh), C.byref(drawn), C.byref(nm))
    if rc != OK:
        raise ArucoHipError(rc, "arucohip_fiducial_board_size")
    return w.value, hh.value, drawn.value, nm.value


def board_pix_to_meters(obj, marker_size_m):
    """aruco_board_pix2meters: objPoints in pixels [n][4][3] -> metres, float32 arithmetic (host, no handle)."""
    o = np.ascontiguousarray(obj, dtype=np.float32).reshape(-1, 4, 3)
    out = np.zeros_like(o)
    rc = load().arucohip_board_pix_to_meters(_ptr(o), o.shape[0], float(marker_size_m), _ptr(out))
    if rc != OK:
        raise ArucoHipError(rc, "arucohip_board_pix_to_meters")
    return out


def rectify_board_window(obj, info_type, marker_size, px_per_unit, margin=0.0, flip_y=False):
    """arucohip_rectify_board_window: the Rectify window that shows the bounding box of obj[N][4][3] plus `margin` (plane units: metres
    for a PIX board with a marker size) at px_per_unit output pixels per unit; flip_y for boards whose y points up."""
    oa = _f32(obj)
    win = Rectify()
    rc = load().arucohip_rectify_board_window(_ptr(oa), oa.size // 12, int(info_type), float(marker_size), float(px_per_unit), float(margin),
                                              int(bool(flip_y)), C.byref(win))
    if rc != OK:
        raise ArucoHipError(rc, "arucohip_rectify_board_window")
    return win


def board_place(obj, rvec, tvec):
    """A board's corners [n][4][3] moved by a rigid transform: R(rvec) p + tvec in double, rounded once to float32 (host, no handle). A cube
    or a folded board is np.concatenate of placed panels."""
    o = np.ascontiguousarray(obj, dtype=np.float32).reshape(-1, 4, 3)
    r, t = np.ascontiguousarray(rvec, dtype=np.float64).reshape(3), np.ascontiguousarray(tvec, dtype=np.float64).reshape(3)
    out = np.zeros_like(o)
    rc = load().arucohip_board_place(_ptr(o), o.shape[0], _ptr(r), _ptr(t), _ptr(out))
    if rc != OK:
        raise ArucoHipError(rc, "arucohip_board_place")
    return out


def _f32(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float32)


class Handle:
    """Owns one arucohip_handle (one HIP stream + device buffers)."""

    def __init__(self, max_width, max_height, max_batch=1, device=0, params=None, limits=None):
        self.L = load()
        self.h = C.c_void_p()
        p = params if params is not None else default_params()
        if limits is None:
            rc = self.L.arucohip_create(C.byref(p), device, max_width, max_height, max_batch, C.byref(self.h))
            lim = Limits()
            self.L.arucohip_default_limits(C.byref(lim), max_width, max_height, max_batch)
            self._markers_per_frame = lim.markers_per_frame
        else:
            rc = self.L.arucohip_create_ex(C.byref(p), device, C.byref(limits), C.byref(self.h))
            self._markers_per_frame = limits.markers_per_frame
        if rc != OK:
            raise ArucoHipError(rc, "arucohip_create")
        self.max_batch = max_batch
        self.device = device

    def close(self):
        if self.h:
            self.L.arucohip_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, allow=()):
        if rc != OK and rc not in allow:
            raise ArucoHipError(rc, (self.L.arucohip_last_error_string(self.h) or b"").decode())
        return rc

    def get_params(self):
        p = Params()
        self._chk(self.L.arucohip_get_params(self.h, C.byref(p)))
        return p

    def set_params(self, p):
        self._chk(self.L.arucohip_set_params(self.h, C.byref(p)))

    def set_stream(self, stream_ptr):
        self._chk(self.L.arucohip_set_stream(self.h, C.c_void_p(stream_ptr)))

    def get_stream(self):
        return self.L.arucohip_get_stream(self.h)

    def synchronize(self):
        self._chk(self.L.arucohip_synchronize(self.h))

    def wait_event(self, event_ptr):
        """The handle's next work waits for a hipEvent_t (plain integer) recorded behind the producer of the frames."""
        self._chk(self.L.arucohip_wait_event(self.h, C.c_void_p(event_ptr)))

    # ---- host-buffer API
    def detect(self, gray, K=None, dist=None, marker_size=-1.0, y_perp=False, cap=128):
        g = np.ascontiguousarray(gray, dtype=np.uint8)
        h, w = g.shape
        Ka, da = _f32(K), _f32(dist)
        out = np.zeros(cap, MARKER_DTYPE)
        n = C.c_int(0)
        self._chk(self.L.arucohip_detect(self.h, _ptr(g), w, h, w, _ptr(Ka), _ptr(da), 0 if da is None else da.size,
                                         float(marker_size), int(bool(y_perp)), _ptr(out), cap, C.byref(n)))
        return out[:n.value].copy()

    def set_dictionary(self, markers, tau0, rate=1.0):
        """HighlyReliableMarkers::loadDictionary: markers = bit strings of n*n characters; selects the HRM decoder
        (None / empty list: back to the 5x5 fiducial decoder)."""
        p = self.get_params()
        if not markers:
            p.decoder_kind = 0
            self.set_params(p)
            self._chk(self.L.arucohip_set_dictionary(self.h, 0, 0, None, 0, 1.0))
            return
        n = int(round(len(markers[0]) ** 0.5))
        codes = np.array([sum(1 << i for i, ch in enumerate(m) if ch == "1") for m in markers], np.uint64)
        self._chk(self.L.arucohip_set_dictionary(self.h, n, len(codes), _ptr(codes), int(tau0), float(rate)))
        p.decoder_kind = 1
        self.set_params(p)

    def detect_bgr(self, bgr, K=None, dist=None, marker_size=-1.0, y_perp=False, cap=128):
        """One host frame [H][W][3] in B,G,R order: converted to gray on the device, then detect()."""
        b = np.ascontiguousarray(bgr, dtype=np.uint8)
        h, w, c = b.shape
        assert c == 3
        Ka, da = _f32(K), _f32(dist)
        out = np.zeros(cap, MARKER_DTYPE)
        n = C.c_int(0)
        self._chk(self.L.arucohip_detect_bgr(self.h, _ptr(b), w, h, 3 * w, _ptr(Ka), _ptr(da), 0 if da is None else da.size,
                                             float(marker_size), int(bool(y_perp)), _ptr(out), cap, C.byref(n)))
        return out[:n.value].copy()

    def detect_batch_bgr_host(self, frames, K=None, dist=None, marker_size=-1.0, y_perp=False, cap=128):
        fr = np.ascontiguousarray(frames, dtype=np.uint8)
        nf, h, w, c = fr.shape
        assert c == 3
        Ka, da = _f32(K), _f32(dist)
        out = np.zeros((nf, cap), MARKER_DTYPE)
        n = np.zeros(nf, np.int32)
        self._chk(self.L.arucohip_detect_batch_bgr(self.h, _ptr(fr), nf, w, h, 3 * w, 3 * w * h, 0, _ptr(Ka), _ptr(da),
                                                   0 if da is None else da.size, float(marker_size), int(bool(y_perp)), _ptr(out), cap, _ptr(n), 0))
        return [out[f, :n[f]].copy() for f in range(nf)]

    # ---- camera-native input: fmt is a FrameFormat; host arrays are uint8 [n][rows][row bytes] exactly as the producer stores them
    # (NV12: rows = height * 3 / 2 with the U,V plane behind the Y plane; GRAY16: a uint16 array [n][H][W] is taken as its bytes)
    @staticmethod
    def _raw_frames(frames, fmt, width, height):
        a = np.ascontiguousarray(frames)
        if a.dtype == np.uint16:
            a = a.view(np.uint8)
        assert a.dtype == np.uint8 and a.ndim == 3
        n, rows, row_bytes = a.shape
        w = width if width is not None else row_bytes // max(fmt.min_row_stride(2) // 2, 1)   # tight rows: bytes per pixel from a 2-pixel row
        h = height if height is not None else (rows * 2 // 3 if fmt.format == PIX_NV12 else rows)
        return a, n, w, h, row_bytes, rows * row_bytes

    def convert(self, frames, fmt, channels, width=None, height=None):
        """arucohip_convert_batch of host frames: -> uint8 [n][H][W] (channels = 1) or [n][H][W][3] (B,G,R)."""
        a, n, w, h, rs, fs = self._raw_frames(frames, fmt, width, height)
        out = np.empty((n, h, w) if channels == 1 else (n, h, w, channels), np.uint8)
        self._chk(self.L.arucohip_convert_batch(self.h, _ptr(a), C.byref(fmt), n, w, h, rs, fs, 0, int(channels), _ptr(out), w * channels,
                                                w * h * channels, 0))
        return out

    def convert_device(self, src_ptr, fmt, nframes, width, height, row_stride, frame_stride, channels, dst_ptr, dst_row_stride=None,
                       dst_frame_stride=None, src_on_device=True, dst_on_device=True):
        """arucohip_convert_batch on pointers (plain integers); with dst_on_device asynchronous on the handle's stream."""
        drs = width * channels if dst_row_stride is None else dst_row_stride
        dfs = drs * height if dst_frame_stride is None else dst_frame_stride
        self._chk(self.L.arucohip_convert_batch(self.h, C.c_void_p(src_ptr), C.byref(fmt), nframes, width, height, row_stride, frame_stride,
                                                int(bool(src_on_device)), int(channels), C.c_void_p(dst_ptr), drs, dfs, int(bool(dst_on_device))))

    # ---- frames out: the library's grey [n][H][W] or B,G,R [n][H][W][3] frames in the layout fmt describes
    def export_frames(self, frames, fmt, row_stride=None, chroma_offset=0, flags=0):
        """arucohip_export_batch of host frames: -> uint8 [n][frame bytes], every frame as fmt.min_stride(W, H, row_stride) bytes (NV12: the
        U,V plane at chroma_offset, 0: behind the Y plane). fmt: a FrameFormat, a PIX_* value or a name. Bytes the call does not write are 0."""
        a = np.ascontiguousarray(frames, dtype=np.uint8)
        assert a.ndim in (3, 4)
        n, h, w = a.shape[:3]
        c = 1 if a.ndim == 3 else a.shape[3]
        fmt = frame_format(fmt.format if isinstance(fmt, FrameFormat) else fmt, chroma_offset=chroma_offset)
        rs = fmt.min_row_stride(w) if row_stride is None else int(row_stride)
        fs = fmt.min_stride(w, h, rs)
        out = np.zeros((n, max(fs, 1)), np.uint8)
        self._chk(self.L.arucohip_export_batch(self.h, _ptr(a), c, n, w, h, w * c, w * h * c, 0, C.byref(fmt), int(flags), _ptr(out), rs, fs, 0))
        return out

    def export_batch_ptr(self, src_ptr, channels, nframes, width, height, fmt, dst_ptr, dst_row_stride=None, dst_frame_stride=None,
                         src_row_stride=None, src_frame_stride=None, flags=0, src_on_device=True, dst_on_device=True):
        """arucohip_export_batch on pointers (plain integers); with dst_on_device asynchronous on the handle's stream."""
        srs = width * channels if src_row_stride is None else src_row_stride
        sfs = srs * height if src_frame_stride is None else src_frame_stride
        drs = fmt.min_row_stride(width) if dst_row_stride is None else dst_row_stride
        dfs = fmt.min_stride(width, height, drs) if dst_frame_stride is None else dst_frame_stride
        self._chk(self.L.arucohip_export_batch(self.h, C.c_void_p(src_ptr), int(channels), nframes, width, height, srs, sfs, int(bool(src_on_device)),
                                               C.byref(fmt), int(flags), C.c_void_p(dst_ptr), drs, dfs, int(bool(dst_on_device))))

    def undistort(self, img, K, dist):
        """cv::undistort of host frames: [H][W], [H][W][3], [N][H][W] (gray batch) -> same shape."""
        a = np.ascontiguousarray(img, dtype=np.uint8)
        if a.ndim == 2:
            n, (hgt, wid), cn = 1, a.shape, 1
        elif a.ndim == 3 and a.shape[2] == 3:
            n, (hgt, wid), cn = 1, a.shape[:2], 3
        else:
            n, hgt, wid = a.shape
            cn = 1
        Ka, da = _f32(K), _f32(dist)
        out = np.empty_like(a)
        self._chk(self.L.arucohip_undistort(self.h, _ptr(a), n, wid, hgt, wid * cn, wid * hgt * cn, cn, 0, _ptr(Ka), _ptr(da),
                                            0 if da is None else da.size, _ptr(out), 0))
        return out

    # ---- fisheye lenses: model = (K, D) with D = k1..k4; Knew = the ideal pinhole camera (None: K); max_angle <= 0: the default 1.4 rad
    def fisheye_undistort_points(self, pts, model, Knew=None, max_angle=0.0):
        """Fisheye pixels [n][2] -> (ideal pixels under Knew as float32 [n][2], valid [n] bool); invalid points are (0, 0)."""
        p = np.ascontiguousarray(pts, dtype=np.float32).reshape(-1, 2)
        m, Kn = fisheye_models((model[0], model[1])), _f32(Knew)
        out = np.zeros_like(p)
        valid = np.zeros(len(p), np.uint8)
        self._chk(self.L.arucohip_fisheye_undistort_points(self.h, m, _ptr(Kn), float(max_angle), _ptr(p), len(p), 0, _ptr(out), _ptr(valid)))
        return out, valid.astype(bool)

    def fisheye_distort_points(self, pts, model, Knew=None):
        """Ideal pixels under Knew [n][2] -> fisheye pixels float32 [n][2]."""
        p = np.ascontiguousarray(pts, dtype=np.float32).reshape(-1, 2)
        m, Kn = fisheye_models((model[0], model[1])), _f32(Knew)
        out = np.zeros_like(p)
        self._chk(self.L.arucohip_fisheye_distort_points(self.h, m, _ptr(Kn), _ptr(p), len(p), 0, _ptr(out)))
        return out

    def fisheye_points_device(self, src_ptr, n, dst_ptr, model, Knew=None, max_angle=0.0, valid_ptr=None):
        """Either direction on device arrays (plain integers), asynchronous on the handle's stream: with valid_ptr fisheye -> ideal pixels,
        without it ideal -> fisheye pixels."""
        m, Kn = fisheye_models((model[0], model[1])), _f32(Knew)
        if valid_ptr is None:
            rc = self.L.arucohip_fisheye_distort_points(self.h, m, _ptr(Kn), C.c_void_p(src_ptr), int(n), 1, C.c_void_p(dst_ptr))
        else:
            rc = self.L.arucohip_fisheye_undistort_points(self.h, m, _ptr(Kn), float(max_angle), C.c_void_p(src_ptr), int(n), 1, C.c_void_p(dst_ptr),
                                                          C.c_void_p(valid_ptr))
        self._chk(rc)

    def fisheye_undistort(self, img, model, Knew=None, max_angle=0.0):
        """Host frames seen through a fisheye lens -> the frames of the ideal camera Knew: [H][W], [H][W][3], [N][H][W] -> same shape."""
        a = np.ascontiguousarray(img, dtype=np.uint8)
        if a.ndim == 2:
            n, (hgt, wid), cn = 1, a.shape, 1
        elif a.ndim == 3 and a.shape[2] == 3:
            n, (hgt, wid), cn = 1, a.shape[:2], 3
        else:
            n, hgt, wid = a.shape
            cn = 1
        m, Kn = fisheye_models((model[0], model[1])), _f32(Knew)
        out = np.empty_like(a)
        self._chk(self.L.arucohip_fisheye_undistort(self.h, _ptr(a), n, wid, hgt, wid * cn, wid * hgt * cn, cn, 0, m, _ptr(Kn), float(max_angle),
                                                    _ptr(out), 0))
        return out

    def fisheye_undistort_device(self, src_ptr, nframes, width, height, channels, dst_ptr, model, Knew=None, max_angle=0.0, row_stride=None,
                                 frame_stride=None):
        """The same between device arrays (plain integers): asynchronous on the handle's stream, dst tightly packed."""
        m, Kn = fisheye_models((model[0], model[1])), _f32(Knew)
        rs = width * channels if row_stride is None else row_stride
        self._chk(self.L.arucohip_fisheye_undistort(self.h, C.c_void_p(src_ptr), int(nframes), int(width), int(height), rs,
                                                    rs * height if frame_stride is None else frame_stride, int(channels), 1, m, _ptr(Kn),
                                                    float(max_angle), C.c_void_p(dst_ptr), 1))

    def fisheye_undistort_markers_batch(self, nframes, models, Knew=None, max_angle=0.0, cap=64, allow=()):
        """arucohip_fisheye_undistort_markers_batch on the last batch, in place: models = one (K, D) or a list of them (frame f uses
        models[f % len]), Knew = None, one 3x3 or one per model. Returns (markers per frame, counts, dropped per frame); cap = 0: the
        lists are not fetched (empty lists, counts None)."""
        m = fisheye_models(models)
        Kn = None if Knew is None else np.ascontiguousarray(np.broadcast_to(np.asarray(Knew, np.float32).reshape(-1, 9), (len(m), 9)))
        out = np.zeros((nframes, cap), MARKER_DTYPE)
        n = np.zeros(nframes, np.int32)
        dropped = np.zeros(nframes, np.int32)
        self._chk(self.L.arucohip_fisheye_undistort_markers_batch(self.h, int(nframes), m, len(m), _ptr(Kn), float(max_angle), _ptr(out) if cap else None,
                                                                  int(cap), _ptr(n) if cap else None, 0, _ptr(dropped)), allow=allow)
        return [out[f, :max(min(int(n[f]), cap), 0)].copy() for f in range(nframes)], n if cap else None, dropped

    def fisheye_undistort_markers_batch_device(self, nframes, models, out_ptr, cap, n_out_ptr, Knew=None, max_angle=0.0):
        """The same with the lists written to device arrays (pointers as plain integers): asynchronous on the handle's stream."""
        m = fisheye_models(models)
        Kn = None if Knew is None else np.ascontiguousarray(np.broadcast_to(np.asarray(Knew, np.float32).reshape(-1, 9), (len(m), 9)))
        self._chk(self.L.arucohip_fisheye_undistort_markers_batch(self.h, int(nframes), m, len(m), _ptr(Kn), float(max_angle), C.c_void_p(out_ptr), int(cap),
                                                                  C.c_void_p(n_out_ptr), 1, None))

    def set_pyr_down(self, level):
        """MarkerDetector::pyrDown(level): threshold, contours and quads on the frame reduced `level` times (0..3), the rest on the frame."""
        self._chk(self.L.arucohip_set_pyr_down(self.h, int(level)))

    @property
    def pyr_down(self):
        return self.L.arucohip_get_pyr_down(self.h)

    def pyr_down_image(self, frames, levels=1):
        """cv::pyrDown, `levels` times, of host frames [H][W] or [N][H][W] -> [Ho][Wo] or [N][Ho][Wo]."""
        a = np.ascontiguousarray(frames, dtype=np.uint8)
        one = a.ndim == 2
        if one:
            a = a[None]
        n, hgt, wid = a.shape
        wo, ho = wid, hgt
        for _ in range(int(levels)):
            wo, ho = (wo + 1) // 2, (ho + 1) // 2
        out = np.empty((n, ho, wo), np.uint8)
        self._chk(self.L.arucohip_pyr_down(self.h, _ptr(a), n, wid, hgt, wid, wid * hgt, 0, int(levels), _ptr(out), 0))
        return out[0] if one else out

    def pyr_down_device(self, src_ptr, nframes, width, height, levels, dst_ptr, row_stride=None, frame_stride=None):
        """arucohip_pyr_down on device frames (plain integer pointers), the result left on the device, tightly packed."""
        rs = width if row_stride is None else row_stride
        fs = rs * height if frame_stride is None else frame_stride
        self._chk(self.L.arucohip_pyr_down(self.h, C.c_void_p(src_ptr), nframes, width, height, rs, fs, 1, int(levels), C.c_void_p(dst_ptr), 1))

    def refine_candidate_lines(self, contour, corners, K=None, dist=None):
        """MarkerDetector::refineCandidateLines: contour = n x 2 integer points, corners = 4 x 2; returns the refined corners (4 x 2)."""
        xy = np.ascontiguousarray(contour, dtype=np.int32).reshape(-1, 2)
        c = np.ascontiguousarray(corners, dtype=np.float32).reshape(8).copy()
        Ka, da = _f32(K), _f32(dist)
        self._chk(self.L.arucohip_refine_candidate_lines(self.h, _ptr(xy), len(xy), _ptr(c), _ptr(Ka), _ptr(da), 0 if da is None else da.size))
        return c.reshape(4, 2)

    def debug_refine_pixels(self, gray, corners, method, win=0, locked_wsize=0, width=None):
        """The locked-corner pre-pass (locked_wsize > 0) and the SUBPIX / HARRIS refinement (method CORNER_SUBPIX with `win`, CORNER_HARRIS;
        CORNER_NONE: the pre-pass alone) on `corners` (n x 2) of one gray frame [H][stride]; `width` < stride gives a padded frame, whose row
        stride is kept on the device. Returns the refined corners (n x 2, float32)."""
        g = np.ascontiguousarray(gray, dtype=np.uint8)
        hgt, stride = g.shape
        c = np.ascontiguousarray(corners, dtype=np.float32).reshape(-1, 2).copy()
        self._chk(self.L.arucohip_debug_refine_pixels(self.h, _ptr(g), stride if width is None else int(width), hgt, stride, _ptr(c), len(c), int(method),
                                                      int(win), int(locked_wsize)))
        return c

    def debug_decode_quads(self, frames, quads, frame_of=None, width=None):
        """The decode stage on integer quads (n x 4 x 2, what an int16 holds) of gray frames [nframes][H][stride] (one frame: [H][stride]); `width` <
        stride gives padded frames whose row stride is kept on the device; frame_of: the frame of each quad (default 0). The handle's warp size,
        decoder and dictionary and the frame count choose the kernels as they do for a batch. Returns a dict: iM (n x 9 float64), hist (n x 256
        uint16), thr, ids, nrot (n, int32) and, as the path that ran left them, cells (n x 49 cell medians) or patches (n x ws x ws), else None."""
        g = np.ascontiguousarray(frames, dtype=np.uint8)
        if g.ndim == 2:
            g = g[None]
        nf, hgt, stride = g.shape
        q = np.ascontiguousarray(quads, dtype=np.int16).reshape(-1, 8)
        n = len(q)
        fo = np.zeros(n, np.int32) if frame_of is None else np.ascontiguousarray(frame_of, dtype=np.int32).reshape(-1)
        assert len(fo) == n
        ws = self.get_params().warp_size
        out = {"iM": np.zeros((n, 9), np.float64), "hist": np.zeros((n, 256), np.uint16), "thr": np.zeros(n, np.int32),
               "cells": np.zeros((n, 49), np.uint8), "patches": np.zeros((n, ws, ws), np.uint8), "ids": np.zeros(n, np.int32),
               "nrot": np.zeros(n, np.int32)}
        paths = C.c_int32(0)
        self._chk(self.L.arucohip_debug_decode_quads(self.h, _ptr(g), nf, stride if width is None else int(width), hgt, stride, _ptr(q), _ptr(fo), n,
                                                     _ptr(out["iM"]), _ptr(out["hist"]), _ptr(out["thr"]), _ptr(out["cells"]), _ptr(out["patches"]),
                                                     _ptr(out["ids"]), _ptr(out["nrot"]), C.byref(paths)))
        if not paths.value & 1:
            out["cells"] = None
        if not paths.value & 2:
            out["patches"] = None
        return out

    def debug_marker_tail(self, nframes, width, height, ids, corners, frame_of=None, plane_status=None, K=None, dist=None, marker_size=-1.0,
                          y_perp=False, out_dev=None, out_cap=0, n_out_dev=None):
        """The marker-list tail (sort by id, same-id dedupe, border filter, capacities and statuses, poses with K and marker_size) on decoded
        candidates: ids (n, -1 = not a marker), corners (n x 4 x 2 float32), frame_of (n, default 0). plane_status: [nframes][planes] status words
        of the threshold planes. out_dev / n_out_dev: device pointers (integers) of [nframes][out_cap] markers and [nframes] counts for the
        write-through path. Returns a dict: rows ([nframes][markers_per_frame] MARKER_DTYPE, 0xA5 bytes where nothing was written), n (true
        counts, -1 = given up), status, nmark, list (the flat marker list's nmark entries), raw_list (all of it) and hdr (the two words behind
        the rows). The frames stay the handle's last batch."""
        ia = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
        n = len(ia)
        ca = np.ascontiguousarray(corners, dtype=np.float32).reshape(n, 8)
        fo = np.zeros(n, np.int32) if frame_of is None else np.ascontiguousarray(frame_of, dtype=np.int32).reshape(-1)
        assert len(fo) == n
        ps = None if plane_status is None else np.ascontiguousarray(plane_status, dtype=np.uint32).reshape(nframes, -1)
        assert ps is None or ps.shape[1] == 2 * self.get_params().thres_param1_range + 1
        Ka, da = _f32(K), _f32(dist)
        capm = self.markers_per_frame()
        out = {"rows": np.zeros((nframes, capm), MARKER_DTYPE), "n": np.zeros(nframes, np.int32), "raw_list": np.zeros(nframes * capm, np.uint32),
               "hdr": np.zeros(2, np.int32)}
        status, nmark = C.c_uint32(0), C.c_uint32(0)
        self._chk(self.L.arucohip_debug_marker_tail(self.h, int(nframes), int(width), int(height), _ptr(ia) if n else None, _ptr(ca) if n else None,
                                                    _ptr(fo) if n else None, n, None if ps is None else _ptr(ps), _ptr(Ka), _ptr(da),
                                                    0 if da is None else da.size, float(marker_size), int(bool(y_perp)),
                                                    None if out_dev is None else C.c_void_p(out_dev), int(out_cap),
                                                    None if n_out_dev is None else C.c_void_p(n_out_dev), _ptr(out["rows"]), _ptr(out["n"]),
                                                    C.byref(status), C.byref(nmark), _ptr(out["raw_list"]), _ptr(out["hdr"])))
        out["status"], out["nmark"] = status.value, nmark.value
        out["list"] = out["raw_list"][:nmark.value].copy()
        return out

    def markers_per_frame(self):
        """The handle's markers_per_frame limit (rows of a frame in the device marker array)."""
        return int(self._markers_per_frame)

    def bgr_to_gray(self, bgr):
        b = np.ascontiguousarray(bgr, dtype=np.uint8)
        h, w, c = b.shape
        assert c == 3
        g = np.empty((h, w), np.uint8)
        self._chk(self.L.arucohip_bgr_to_gray(self.h, _ptr(b), w, h, 3 * w, _ptr(g)))
        return g

    def detect_batch_host(self, frames, K=None, dist=None, marker_size=-1.0, y_perp=False, cap=128):
        fr = np.ascontiguousarray(frames, dtype=np.uint8)
        nf, h, w = fr.shape
        Ka, da = _f32(K), _f32(dist)
        out = np.zeros((nf, cap), MARKER_DTYPE)
        n = np.zeros(nf, np.int32)
        self._chk(self.L.arucohip_detect_batch(self.h, _ptr(fr), nf, w, h, w, w * h, 0, _ptr(Ka), _ptr(da),
                                               0 if da is None else da.size, float(marker_size), int(bool(y_perp)), _ptr(out),
                                               cap, _ptr(n), 0))
        return [out[f, :n[f]].copy() for f in range(nf)]

    # ---- device-pointer API (frames resident in HBM, results left in HBM): pointers are plain integers
    def detect_batch_device(self, frames_ptr, nframes, width, height, out_ptr, cap, n_out_ptr, K=None, dist=None,
                            marker_size=-1.0, y_perp=False, row_stride=None, frame_stride=None):
        Ka, da = _f32(K), _f32(dist)
        rs = width if row_stride is None else row_stride
        fs = rs * height if frame_stride is None else frame_stride
        self._chk(self.L.arucohip_detect_batch(self.h, C.c_void_p(frames_ptr), nframes, width, height, rs, fs, 1, _ptr(Ka),
                                               _ptr(da), 0 if da is None else da.size, float(marker_size), int(bool(y_perp)),
                                               C.c_void_p(out_ptr), cap, C.c_void_p(n_out_ptr), 1))

    def retry_overflowed_device(self, frames_ptr, nframes, width, height, out_ptr, cap, n_out_ptr, K=None, dist=None, marker_size=-1.0, y_perp=False):
        """arucohip_detect_batch_retry_overflowed on device frames / device results (after batch_status or wait returned E_OVERFLOW):
        returns the number of frames that were run again."""
        Ka, da = _f32(K), _f32(dist)
        k = C.c_int(0)
        self._chk(self.L.arucohip_detect_batch_retry_overflowed(self.h, C.c_void_p(frames_ptr), nframes, width, height, width, width * height, 1, _ptr(Ka),
                                                                _ptr(da), 0 if da is None else da.size, float(marker_size), int(bool(y_perp)),
                                                                C.c_void_p(out_ptr), cap, C.c_void_p(n_out_ptr), 1, C.byref(k)))
        return k.value

    def detect_batch_host_tolerant(self, frames, K=None, dist=None, marker_size=-1.0, y_perp=False, cap=128, retry=True):
        """detect_batch_host that survives list overflows: returns (per-frame arrays or None for a frame still given up, frames retried)."""
        fr = np.ascontiguousarray(frames, dtype=np.uint8)
        nf, h, w = fr.shape
        Ka, da = _f32(K), _f32(dist)
        out = np.zeros((nf, cap), MARKER_DTYPE)
        n = np.zeros(nf, np.int32)
        nd = 0 if da is None else da.size
        rc = self._chk(self.L.arucohip_detect_batch(self.h, _ptr(fr), nf, w, h, w, w * h, 0, _ptr(Ka), _ptr(da), nd, float(marker_size), int(bool(y_perp)),
                                                    _ptr(out), cap, _ptr(n), 0), allow=(E_OVERFLOW,))
        k = C.c_int(0)
        first = n.copy()
        if rc == E_OVERFLOW and retry:
            self._chk(self.L.arucohip_detect_batch_retry_overflowed(self.h, _ptr(fr), nf, w, h, w, w * h, 0, _ptr(Ka), _ptr(da), nd, float(marker_size),
                                                                    int(bool(y_perp)), _ptr(out), cap, _ptr(n), 0, C.byref(k)))
        return [out[f, :n[f]].copy() if n[f] >= 0 else None for f in range(nf)], k.value, first

    def detect_batch_mixed(self, frames_host_ptr, nframes, width, height, out_ptr, cap, n_out_ptr, K=None, dist=None,
                           marker_size=-1.0, y_perp=False):
        """Frames in (pinned) host memory, results left on the device: the PCIe-inclusive path."""
        Ka, da = _f32(K), _f32(dist)
        self._chk(self.L.arucohip_detect_batch(self.h, C.c_void_p(frames_host_ptr), nframes, width, height, width, width * height, 0,
                                               _ptr(Ka), _ptr(da), 0 if da is None else da.size, float(marker_size), int(bool(y_perp)),
                                               C.c_void_p(out_ptr), cap, C.c_void_p(n_out_ptr), 1))

    # ---- batches in flight
    def set_pipeline_depth(self, depth):
        self._chk(self.L.arucohip_set_pipeline_depth(self.h, int(depth)))

    def submit_device(self, frames_ptr, nframes, width, height, out_ptr, cap, n_out_ptr, K=None, dist=None, marker_size=-1.0, y_perp=False,
                      frames_on_device=True):
        """arucohip_detect_batch_submit with results left on the device (frames device-resident, or in pinned host memory with
        frames_on_device=False); returns the ticket."""
        Ka, da = _f32(K), _f32(dist)
        t = C.c_int(-1)
        self._chk(self.L.arucohip_detect_batch_submit(self.h, C.c_void_p(frames_ptr), nframes, width, height, width, width * height,
                                                      int(bool(frames_on_device)), _ptr(Ka),
                                                      _ptr(da), 0 if da is None else da.size, float(marker_size), int(bool(y_perp)),
                                                      C.c_void_p(out_ptr), cap, C.c_void_p(n_out_ptr), 1, C.byref(t)))
        return t.value

    def submit_host(self, frames, out, n, K=None, dist=None, marker_size=-1.0, y_perp=False):
        """Host frames [n][H][W] and host result arrays (out: [n][cap] MARKER_DTYPE, n: int32[n]) that must stay alive
        until wait(ticket)."""
        nf, h, w = frames.shape
        Ka, da = _f32(K), _f32(dist)
        t = C.c_int(-1)
        self._chk(self.L.arucohip_detect_batch_submit(self.h, _ptr(frames), nf, w, h, w, w * h, 0, _ptr(Ka), _ptr(da), 0 if da is None else da.size,
                                                      float(marker_size), int(bool(y_perp)), _ptr(out), out.shape[1], _ptr(n), 0, C.byref(t)))
        return t.value

    def wait(self, ticket, allow=()):
        return self._chk(self.L.arucohip_detect_batch_wait(self.h, int(ticket)), allow)

    def batch_status(self):
        return self._chk(self.L.arucohip_batch_status(self.h))

    def batch_chunks(self):
        """(chunks, frames per chunk) of the last batch: every kernel launch covers one chunk."""
        per = C.c_int(0)
        n = self.L.arucohip_batch_chunks(self.h, C.byref(per))
        return n, per.value

    def thresholded(self, frame=0, shape=None):
        out = np.empty(shape, np.uint8)
        self._chk(self.L.arucohip_get_thresholded(self.h, frame, _ptr(out)))
        return out

    def debug_threshold_batch(self, frames, nframes=None, width=None, height=None, row_stride=None, frame_stride=None, want_bytes=False):
        """arucohip_debug_threshold_batch: the threshold stage alone, with the handle's parameters. frames: a device address (an int; nframes,
        width and height are then required) or a host array [nframes][height][width]."""
        if isinstance(frames, int):
            ptr, on_dev = C.c_void_p(frames), 1
        else:
            fr = np.ascontiguousarray(frames, np.uint8)
            nframes, height, width = fr.shape
            ptr, on_dev = _ptr(fr), 0
        rs = width if row_stride is None else row_stride
        fs = rs * height if frame_stride is None else frame_stride
        self._chk(self.L.arucohip_debug_threshold_batch(self.h, ptr, int(nframes), int(width), int(height), rs, fs, on_dev, int(bool(want_bytes))))

    THR_FAMILIES = ("strip", "wide", "eo")

    def debug_threshold_plan(self):
        """arucohip_debug_threshold_plan: {"planes": [{"family", "R", "p16", "fast", "seg"}, ...], "strips", "no_bytes", "bitmap_pass"} of the last
        threshold launch."""
        out = np.zeros(5 * 16 + 3, np.int32)
        n = C.c_int(0)
        self._chk(self.L.arucohip_debug_threshold_plan(self.h, _ptr(out), out.size, C.byref(n)))
        k = n.value
        planes = [{"family": self.THR_FAMILIES[out[5 * t]], "R": int(out[5 * t + 1]), "p16": bool(out[5 * t + 2]), "fast": bool(out[5 * t + 3]),
                   "seg": int(out[5 * t + 4])} for t in range(k)]
        return {"planes": planes, "strips": int(out[5 * k]), "no_bytes": bool(out[5 * k + 1]), "bitmap_pass": bool(out[5 * k + 2])}

    def debug_threshold_plane(self, frame, t, width, height):
        """arucohip_debug_threshold_plane: (bytes [height][width], tiles [tiles_y][tiles_x], tile_bits [tiles_y][2 * strips]) of plane t of a frame
        of the last batch."""
        tnx, tny, ns = max(4, (width + 7) // 8 + 1), max(4, (height + 7) // 8 + 1), (width + 1023) // 1024
        b = np.empty((height, width), np.uint8)
        tl = np.empty((tny, tnx), np.uint64)
        tb = np.empty((tny, 2 * ns), np.uint64)
        self._chk(self.L.arucohip_debug_threshold_plane(self.h, int(frame), int(t), _ptr(b), _ptr(tl), _ptr(tb)))
        return b, tl, tb

    def candidates(self, frame=0, cap=512):
        q = np.zeros((cap, 4, 2), np.float32)
        n = C.c_int(0)
        self._chk(self.L.arucohip_get_candidates(self.h, frame, _ptr(q), cap, C.byref(n)))
        return q[:n.value].copy()

    def debug_candidates(self, frame=0, cap=512):
        q = np.zeros((cap, 4, 2), np.float32)
        ids = np.zeros(cap, np.int32)
        nrot = np.zeros(cap, np.int32)
        n = C.c_int(0)
        self._chk(self.L.arucohip_debug_candidates(self.h, frame, _ptr(q), _ptr(ids), _ptr(nrot), cap, C.byref(n)))
        k = n.value
        return q[:k].copy(), ids[:k].copy(), nrot[:k].copy()

    def debug_otsu(self, frame=0, cap=512):
        """Otsu threshold of every candidate's patch (candidate order of debug_candidates)."""
        t = np.zeros(cap, np.int32)
        n = C.c_int(0)
        self._chk(self.L.arucohip_debug_otsu(self.h, frame, _ptr(t), cap, C.byref(n)))
        return t[:n.value].copy()

    def debug_cells(self, frame=0, cap=512):
        """Cell medians (7 x 7, the 33rd-largest of each cell's 64 pixels) of every candidate's 56x56 patch, candidate order of debug_candidates."""
        c = np.zeros((cap, 7, 7), np.uint8)
        n = C.c_int(0)
        self._chk(self.L.arucohip_debug_cells(self.h, frame, _ptr(c), cap, C.byref(n)))
        return c[:n.value].copy()

    def debug_start_candidates(self, frame=0, kind=0):
        """Border-start candidates of a frame after the run rule, walker mode only: the transition pixels y << 16 | x of the outer (kind 0)
        or hole (kind 1) list, in the order the device appended them."""
        n = C.c_int(0)
        self._chk(self.L.arucohip_debug_start_candidates(self.h, int(frame), int(kind), None, 0, C.byref(n)), allow=(E_CAPACITY,))
        out = np.zeros(max(n.value, 1), np.uint32)
        self._chk(self.L.arucohip_debug_start_candidates(self.h, int(frame), int(kind), _ptr(out), n.value, C.byref(n)))
        return out[:n.value].copy()

    def debug_contours(self, frame=0):
        n = C.c_int(0)
        self._chk(self.L.arucohip_debug_num_contours(self.h, frame, C.byref(n)))
        res = []
        for i in range(n.value):
            hole, sx, sy, npts = C.c_int(), C.c_int(), C.c_int(), C.c_int()
            self._chk(self.L.arucohip_debug_contour(self.h, frame, i, C.byref(hole), C.byref(sx), C.byref(sy), None, 0, C.byref(npts)))
            pts = np.zeros((npts.value, 2), np.int16)
            self._chk(self.L.arucohip_debug_contour(self.h, frame, i, C.byref(hole), C.byref(sx), C.byref(sy), _ptr(pts),
                                                    npts.value, C.byref(npts)))
            res.append({"hole": hole.value, "start": (sx.value, sy.value), "pts": pts.astype(np.int32)})
        return res

    def threshold(self, gray, method=THRES_ADPT, param1=-1.0, param2=-1.0):
        g = np.ascontiguousarray(gray, dtype=np.uint8)
        h, w = g.shape
        out = np.empty((h, w), np.uint8)
        self._chk(self.L.arucohip_threshold(self.h, method, _ptr(g), w, h, w, float(param1), float(param2), _ptr(out)))
        return out

    def detect_rectangles(self, thres, cap=512):
        t = np.ascontiguousarray(thres, dtype=np.uint8)
        h, w = t.shape
        q = np.zeros((cap, 4, 2), np.float32)
        n = C.c_int(0)
        self._chk(self.L.arucohip_detect_rectangles(self.h, _ptr(t), w, h, w, _ptr(q), cap, C.byref(n)))
        return q[:n.value].copy()

    def warp(self, gray, quad, size=56):
        g = np.ascontiguousarray(gray, dtype=np.uint8)
        h, w = g.shape
        q = _f32(quad).reshape(8)
        out = np.empty((size, size), np.uint8)
        self._chk(self.L.arucohip_warp(self.h, _ptr(g), w, h, w, _ptr(q), size, _ptr(out)))
        return out

    def calculate_extrinsics(self, markers, K, dist, marker_size, y_perp=False):
        m = np.ascontiguousarray(markers, dtype=MARKER_DTYPE).copy()
        Ka, da = _f32(K), _f32(dist)
        self._chk(self.L.arucohip_calculate_extrinsics(self.h, _ptr(m), len(m), _ptr(Ka), _ptr(da), 0 if da is None else da.size,
                                                       float(marker_size), int(bool(y_perp))))
        return m

    def planar_poses(self, markers, K, dist, marker_size, refine=True, y_perp=False):
        """Both planar pose solutions of every marker (only the corners are read), each refined by the library's Levenberg-Marquardt
        unless refine is False: a PlanarPoses array, one entry per marker, the solution with the smaller reprojection error first."""
        m = np.ascontiguousarray(markers, dtype=MARKER_DTYPE)
        Ka, da = _f32(K), _f32(dist)
        out = (PlanarPoses * len(m))()
        self._chk(self.L.arucohip_planar_poses(self.h, _ptr(m) if len(m) else None, len(m), 0, _ptr(Ka), _ptr(da), 0 if da is None else da.size,
                                               float(marker_size), int(bool(refine)), int(bool(y_perp)), out))
        return out

    def planar_poses_device(self, markers_ptr, n, out_ptr, K, dist, marker_size, refine=True, y_perp=False):
        """planar_poses on device arrays (arucohip_marker_t [n] in, arucohip_planar_poses_t [n] out, given as pointers)."""
        Ka, da = _f32(K), _f32(dist)
        self._chk(self.L.arucohip_planar_poses(self.h, markers_ptr, int(n), 1, _ptr(Ka), _ptr(da), 0 if da is None else da.size,
                                               float(marker_size), int(bool(refine)), int(bool(y_perp)), out_ptr))

    def planar_poses_batch(self, nframes, K, dist, marker_size, refine=True, y_perp=False, cap=64, fill=0):
        """planar_poses on the device-resident markers of the last detect_batch call: a PlanarPoses array of nframes * cap entries,
        entry f * cap + i for marker i of frame f; the entries beyond a frame's markers keep the byte `fill`."""
        Ka, da = _f32(K), _f32(dist)
        out = (PlanarPoses * (nframes * cap))()
        C.memset(out, int(fill), C.sizeof(out))
        self._chk(self.L.arucohip_planar_poses_batch(self.h, int(nframes), _ptr(Ka), _ptr(da), 0 if da is None else da.size, float(marker_size),
                                                     int(bool(refine)), int(bool(y_perp)), out, int(cap), 0))
        return out

    def planar_poses_batch_device(self, nframes, out_ptr, cap, K, dist, marker_size, refine=True, y_perp=False):
        """planar_poses_batch into a device array of nframes * cap arucohip_planar_poses_t, given as a pointer."""
        Ka, da = _f32(K), _f32(dist)
        self._chk(self.L.arucohip_planar_poses_batch(self.h, int(nframes), _ptr(Ka), _ptr(da), 0 if da is None else da.size, float(marker_size),
                                                     int(bool(refine)), int(bool(y_perp)), out_ptr, int(cap), 1))

    # ---- overlays: frames and markers are numpy arrays (host) or torch tensors on the handle's device, painted in place
    @staticmethod
    def _buf(a):
        """(pointer, on_device) of a numpy array or a torch tensor; both must be contiguous."""
        if isinstance(a, np.ndarray):
            assert a.flags.c_contiguous
            return a.ctypes.data_as(C.c_void_p), 0
        assert a.is_contiguous()
        return C.c_void_p(a.data_ptr()), int(a.is_cuda)

    @classmethod
    def _frames(cls, frames, width, channels):
        """Frame arguments of the draw calls. frames: uint8 [N][H][W] (gray) or [N][H][W][3] (B G R); with `width` (and `channels`) given
        instead [N][H][row_stride bytes], rows padded."""
        assert str(frames.dtype).endswith("uint8")
        if width is None:
            assert frames.ndim in (3, 4)
            ch = 1 if frames.ndim == 3 else int(frames.shape[3])
            n, hgt, wid = (int(v) for v in frames.shape[:3])
            rs = wid * ch
        else:
            assert frames.ndim == 3
            n, hgt, rs = (int(v) for v in frames.shape)
            wid, ch = int(width), int(channels)
        ptr, dev = cls._buf(frames)
        return ptr, n, wid, hgt, ch, rs, rs * hgt, dev

    def draw_markers(self, frames, markers, counts, K=None, dist=None, flags=DRAW_OUTLINE | DRAW_IDS, line_width=1, color=(0, 0, 255), width=None,
                     channels=1):
        """arucohip_draw_markers_batch, in place. markers: [N][cap] MARKER_DTYPE (numpy) or the device array detect_batch_device filled
        (any tensor of N * cap * 96 bytes), counts: N int32 of the same kind. Device frames with device markers: asynchronous."""
        ptr, n, wid, hgt, ch, rs, fs, dev = self._frames(frames, width, channels)
        if isinstance(markers, np.ndarray):
            assert markers.dtype == MARKER_DTYPE and counts.dtype == np.int32
            total = markers.size
        else:
            total = markers.numel() * markers.element_size() // MARKER_DTYPE.itemsize
        assert total % n == 0 and total >= n and len(counts) == n
        mptr, mdev = self._buf(markers)
        cptr, cdev = self._buf(counts)
        assert mdev == cdev
        Ka, da = _f32(K), _f32(dist)
        st = Overlay(int(flags), int(line_width), (C.c_uint8 * 4)(*[int(c) for c in color][:3], 0))
        self._chk(self.L.arucohip_draw_markers_batch(self.h, ptr, n, wid, hgt, ch, rs, fs, dev, mptr, total // n, cptr, mdev, _ptr(Ka), _ptr(da),
                                                     0 if da is None else da.size, C.byref(st)))
        return frames

    def draw_boards(self, frames, boards, marker_size, K, dist=None, flags=DRAW_AXIS | DRAW_CUBE, width=None, channels=1):
        """arucohip_draw_boards_batch, in place. boards: N BOARD_DTYPE entries (numpy; board_detect_batch's first result converts with
        np.frombuffer) or a device tensor of N * 56 bytes."""
        ptr, n, wid, hgt, ch, rs, fs, dev = self._frames(frames, width, channels)
        if isinstance(boards, np.ndarray):
            assert boards.dtype == BOARD_DTYPE and boards.size == n
        bptr, bdev = self._buf(boards)
        Ka, da = _f32(K), _f32(dist)
        self._chk(self.L.arucohip_draw_boards_batch(self.h, ptr, n, wid, hgt, ch, rs, fs, dev, bptr, bdev, float(marker_size), _ptr(Ka), _ptr(da),
                                                    0 if da is None else da.size, int(flags)))
        return frames

    @staticmethod
    def _board_records(boards):
        """N BOARD_DTYPE entries of the list of dicts board_detect_batch returns; an array passes through."""
        if isinstance(boards, np.ndarray):
            return boards
        b = np.zeros(len(boards), BOARD_DTYPE)
        for k, d in enumerate(boards):
            b[k] = (d.get("n_markers", 0), d["has_pose"], d["rvec"], d["tvec"])
        return b

    # ---- plane rectification: the fronto-parallel view of a board's plane, one map per frame
    def warp_plane_device(self, src_ptr, nframes, width, height, channels, maps_ptr, dst_ptr, out_width, out_height, K=None, dist=None,
                          valid_ptr=None, row_stride=None, frame_stride=None, dst_row_stride=None, dst_frame_stride=None, src_on_device=1,
                          maps_on_device=1, dst_on_device=1):
        """arucohip_warp_plane_batch on plain addresses: dst pixel (u, v) of frame f = src frame f sampled at cam(maps[f] (u, v, 1)). Strides
        default to tightly packed. With everything on the device the call is asynchronous on the handle's stream."""
        rs = width * channels if row_stride is None else row_stride
        drs = out_width * channels if dst_row_stride is None else dst_row_stride
        Ka, da = _f32(K), _f32(dist)
        self._chk(self.L.arucohip_warp_plane_batch(self.h, src_ptr, int(nframes), int(width), int(height), int(channels), rs,
                                                   rs * height if frame_stride is None else frame_stride, int(src_on_device), maps_ptr, valid_ptr,
                                                   int(maps_on_device), _ptr(Ka), _ptr(da), 0 if da is None else da.size, dst_ptr, int(out_width),
                                                   int(out_height), drs, drs * out_height if dst_frame_stride is None else dst_frame_stride,
                                                   int(dst_on_device)))

    def warp_plane(self, frames, maps, out_size, K=None, dist=None, valid=None, width=None, channels=1):
        """Host frames uint8 [N][H][W] or [N][H][W][3] (see _frames for padded rows), maps float64 [N][3][3] or [N][9], out_size =
        (out_width, out_height), valid: N flags or None. Returns uint8 [N][out_height][out_width] (x 3)."""
        assert isinstance(frames, np.ndarray)
        ptr, n, wid, hgt, ch, rs, fs, _ = self._frames(frames, width, channels)
        m = np.ascontiguousarray(maps, dtype=np.float64).reshape(n, 9)
        va = None if valid is None else np.ascontiguousarray(valid, dtype=np.int32).reshape(n)
        ow, oh = int(out_size[0]), int(out_size[1])
        out = np.zeros((n, oh, ow) if ch == 1 else (n, oh, ow, ch), np.uint8)
        self.warp_plane_device(ptr, n, wid, hgt, ch, _ptr(m), _ptr(out), ow, oh, K, dist, _ptr(va), rs, fs, src_on_device=0, maps_on_device=0,
                               dst_on_device=0)
        return out

    def board_rectify_device(self, frames_ptr, nframes, width, height, channels, boards, K, win, dst_ptr, dist=None, row_stride=None,
                             frame_stride=None, dst_row_stride=None, dst_frame_stride=None, frames_on_device=1, dst_on_device=1, report=False):
        """arucohip_board_rectify_batch on plain addresses. boards: N BOARD_DTYPE entries (numpy) or a device tensor of N * 56 bytes. With
        report: returns (status int32 [N], maps float64 [N][9]) and is synchronous; without it device frames, boards and dst make the
        call asynchronous on the handle's stream."""
        if isinstance(boards, np.ndarray):
            assert boards.dtype == BOARD_DTYPE and boards.size == nframes
        bptr, bdev = self._buf(boards)
        rs = width * channels if row_stride is None else row_stride
        drs = win.out_width * channels if dst_row_stride is None else dst_row_stride
        Ka, da = _f32(K), _f32(dist)
        status = np.zeros(nframes, np.int32) if report else None
        maps = np.zeros((nframes, 9), np.float64) if report else None
        self._chk(self.L.arucohip_board_rectify_batch(self.h, frames_ptr, int(nframes), int(width), int(height), int(channels), rs,
                                                      rs * height if frame_stride is None else frame_stride, int(frames_on_device), bptr, bdev,
                                                      _ptr(Ka), _ptr(da), 0 if da is None else da.size, C.byref(win), dst_ptr, drs,
                                                      drs * win.out_height if dst_frame_stride is None else dst_frame_stride, int(dst_on_device),
                                                      _ptr(status), _ptr(maps)))
        return (status, maps) if report else None

    def board_rectify(self, frames, boards, K, win, dist=None, width=None, channels=1):
        """Host frames (as warp_plane) resampled on the plane of boards[f]: N BOARD_DTYPE entries, or the list of dicts board_detect_batch
        returns. Returns (images uint8 [N][win.out_height][win.out_width] (x 3), status int32 [N], maps float64 [N][9])."""
        assert isinstance(frames, np.ndarray)
        ptr, n, wid, hgt, ch, rs, fs, _ = self._frames(frames, width, channels)
        boards = self._board_records(boards)
        out = np.zeros((n, win.out_height, win.out_width) if ch == 1 else (n, win.out_height, win.out_width, ch), np.uint8)
        status, maps = self.board_rectify_device(ptr, n, wid, hgt, ch, boards, K, win, _ptr(out), dist, rs, fs, frames_on_device=0, dst_on_device=0,
                                                 report=True)
        return out, status, maps

    # ---- plane compositing: a texture blended onto the plane of every frame, in place
    def composite_plane_device(self, frames_ptr, nframes, width, height, channels, tex, maps_ptr, K=None, dist=None, valid_ptr=None, masks_ptr=None,
                               row_stride=None, frame_stride=None, frames_on_device=1, maps_on_device=1, masks_on_device=1):
        """arucohip_composite_plane_batch on plain addresses: frame pixel (u, v) of frame f is blended with the Texture `tex` sampled at
        maps[f] ray(u, v). Strides default to tightly packed. With everything on the device the call is asynchronous on the handle's stream."""
        rs = width * channels if row_stride is None else row_stride
        Ka, da = _f32(K), _f32(dist)
        self._chk(self.L.arucohip_composite_plane_batch(self.h, frames_ptr, int(nframes), int(width), int(height), int(channels), rs,
                                                        rs * height if frame_stride is None else frame_stride, int(frames_on_device), C.byref(tex),
                                                        maps_ptr, valid_ptr, int(maps_on_device), _ptr(Ka), _ptr(da), 0 if da is None else da.size,
                                                        masks_ptr, int(masks_on_device)))

    def composite_plane(self, frames, tex, maps, K=None, dist=None, valid=None, opacity=255, masks=None, per_frame=False, width=None, channels=1):
        """Host frames uint8 [N][H][W] or [N][H][W][3] (see _frames for padded rows), tex: a uint8 array as texture() takes it (with
        per_frame one texture per frame) or a Texture, maps float64 [N][3][3] or [N][9], valid: N flags or None, masks: uint8 [N][H][W] or
        None. Returns the painted frames (a copy)."""
        assert isinstance(frames, np.ndarray)
        out = np.ascontiguousarray(frames).copy()
        ptr, n, wid, hgt, ch, rs, fs, _ = self._frames(out, width, channels)
        t = tex if isinstance(tex, Texture) else texture(np.ascontiguousarray(tex), opacity, per_frame)
        m = np.ascontiguousarray(maps, dtype=np.float64).reshape(n, 9)
        va = None if valid is None else np.ascontiguousarray(valid, dtype=np.int32).reshape(n)
        ma = None if masks is None else np.ascontiguousarray(masks, dtype=np.uint8).reshape(n, hgt, wid)
        self.composite_plane_device(ptr, n, wid, hgt, ch, t, _ptr(m), K, dist, _ptr(va), _ptr(ma), rs, fs, frames_on_device=0, maps_on_device=0,
                                    masks_on_device=0)
        return out

    def board_composite_device(self, frames_ptr, nframes, width, height, channels, boards, K, win, tex, dist=None, masks_ptr=None, row_stride=None,
                               frame_stride=None, frames_on_device=1, masks_on_device=1, report=False):
        """arucohip_board_composite_batch on plain addresses. boards: N BOARD_DTYPE entries (numpy) or a device tensor of N * 56 bytes; tex: a
        Texture of win's size. With report: returns (status int32 [N], maps float64 [N][9]) and is synchronous; without it device frames,
        boards, texture and masks make the call asynchronous on the handle's stream."""
        if isinstance(boards, np.ndarray):
            assert boards.dtype == BOARD_DTYPE and boards.size == nframes
        bptr, bdev = self._buf(boards)
        rs = width * channels if row_stride is None else row_stride
        Ka, da = _f32(K), _f32(dist)
        status = np.zeros(nframes, np.int32) if report else None
        maps = np.zeros((nframes, 9), np.float64) if report else None
        self._chk(self.L.arucohip_board_composite_batch(self.h, frames_ptr, int(nframes), int(width), int(height), int(channels), rs,
                                                        rs * height if frame_stride is None else frame_stride, int(frames_on_device), bptr, bdev,
                                                        _ptr(Ka), _ptr(da), 0 if da is None else da.size, C.byref(win), C.byref(tex), masks_ptr,
                                                        int(masks_on_device), _ptr(status), _ptr(maps)))
        return (status, maps) if report else None

    def board_composite(self, frames, boards, K, win, tex, dist=None, opacity=255, masks=None, per_frame=False, width=None, channels=1):
        """Host frames (as composite_plane) painted with tex on the plane of boards[f]: N BOARD_DTYPE entries, or the list of dicts
        board_detect_batch returns. Returns (the painted frames, status int32 [N], maps float64 [N][9])."""
        assert isinstance(frames, np.ndarray)
        out = np.ascontiguousarray(frames).copy()
        ptr, n, wid, hgt, ch, rs, fs, _ = self._frames(out, width, channels)
        boards = self._board_records(boards)
        t = tex if isinstance(tex, Texture) else texture(np.ascontiguousarray(tex), opacity, per_frame)
        ma = None if masks is None else np.ascontiguousarray(masks, dtype=np.uint8).reshape(n, hgt, wid)
        status, maps = self.board_composite_device(ptr, n, wid, hgt, ch, boards, K, win, t, dist, _ptr(ma), rs, fs, frames_on_device=0,
                                                   masks_on_device=0, report=True)
        return out, status, maps

    # ---- mesh rendering: shaded triangle meshes at marker and board poses, in place
    def render_markers_device(self, frames_ptr, nframes, width, height, channels, markers_ptr, cap, counts_ptr, K, msh, style=None, dist=None,
                              masks_ptr=None, row_stride=None, frame_stride=None, frames_on_device=1, markers_on_device=1, masks_on_device=1):
        """arucohip_render_markers_batch on plain addresses. msh: a Mesh (mesh()), style: a Render (render_style()) or None for the
        defaults. Strides default to tightly packed. With everything on the device the call is asynchronous on the handle's stream."""
        rs = width * channels if row_stride is None else row_stride
        Ka, da = _f32(K), _f32(dist)
        self._chk(self.L.arucohip_render_markers_batch(self.h, frames_ptr, int(nframes), int(width), int(height), int(channels), rs,
                                                       rs * height if frame_stride is None else frame_stride, int(frames_on_device), markers_ptr,
                                                       int(cap), counts_ptr, int(markers_on_device), _ptr(Ka), _ptr(da),
                                                       0 if da is None else da.size, C.byref(msh) if msh is not None else None,
                                                       C.byref(style) if style is not None else None, masks_ptr, int(masks_on_device)))

    def render_markers(self, frames, markers, counts, K, msh, style=None, dist=None, masks=None, width=None, channels=1):
        """arucohip_render_markers_batch, in place. frames, markers and counts as draw_markers takes them (numpy, or torch tensors on the
        device); masks: uint8 [N][H][W] of the same kind as the frames, or None."""
        ptr, n, wid, hgt, ch, rs, fs, dev = self._frames(frames, width, channels)
        if isinstance(markers, np.ndarray):
            assert markers.dtype == MARKER_DTYPE and counts.dtype == np.int32
            total = markers.size
        else:
            total = markers.numel() * markers.element_size() // MARKER_DTYPE.itemsize
        assert total % n == 0 and total >= n and len(counts) == n
        (mptr, mdev), (cptr, cdev) = self._buf(markers), self._buf(counts)
        assert mdev == cdev
        kptr, kdev = (None, 1) if masks is None else self._buf(masks)
        self.render_markers_device(ptr, n, wid, hgt, ch, mptr, total // n, cptr, K, msh, style, dist, kptr, rs, fs, dev, mdev, kdev)
        return frames

    def render_boards_device(self, frames_ptr, nframes, width, height, channels, boards, K, msh, style=None, dist=None, masks_ptr=None,
                             row_stride=None, frame_stride=None, frames_on_device=1, masks_on_device=1):
        """arucohip_render_boards_batch on plain addresses. boards: N BOARD_DTYPE entries (numpy) or a device tensor of N * 56 bytes."""
        if isinstance(boards, np.ndarray):
            assert boards.dtype == BOARD_DTYPE and boards.size == nframes
        bptr, bdev = self._buf(boards)
        rs = width * channels if row_stride is None else row_stride
        Ka, da = _f32(K), _f32(dist)
        self._chk(self.L.arucohip_render_boards_batch(self.h, frames_ptr, int(nframes), int(width), int(height), int(channels), rs,
                                                      rs * height if frame_stride is None else frame_stride, int(frames_on_device), bptr, bdev,
                                                      _ptr(Ka), _ptr(da), 0 if da is None else da.size, C.byref(msh) if msh is not None else None,
                                                      C.byref(style) if style is not None else None, masks_ptr, int(masks_on_device)))

    def render_boards(self, frames, boards, K, msh, style=None, dist=None, masks=None, width=None, channels=1):
        """arucohip_render_boards_batch, in place. boards: N BOARD_DTYPE entries, the list of dicts board_detect_batch returns, or a
        device tensor of N * 56 bytes."""
        ptr, n, wid, hgt, ch, rs, fs, dev = self._frames(frames, width, channels)
        if isinstance(boards, (list, tuple)):
            boards = self._board_records(boards)
        kptr, kdev = (None, 1) if masks is None else self._buf(masks)
        self.render_boards_device(ptr, n, wid, hgt, ch, boards, K, msh, style, dist, kptr, rs, fs, dev, kdev)
        return frames

    def render_times(self):
        """(calls, build ms, raster ms): the render calls since enable_timing(True) and their kernels' average times per call."""
        b, r = C.c_float(0), C.c_float(0)
        n = self.L.arucohip_render_times(self.h, C.byref(b), C.byref(r))
        return n, b.value, r.value

    def board_detect(self, markers, ids, obj, info_type, K=None, dist=None, marker_size=-1.0, repj_err_thres=-1.0, y_perp=False):
        m = np.ascontiguousarray(markers, dtype=MARKER_DTYPE)
        ida = np.ascontiguousarray(ids, dtype=np.int32)
        oa = _f32(obj)
        Ka, da = _f32(K), _f32(dist)
        outm = np.zeros(max(len(m), 1), MARKER_DTYPE)
        bo = BoardOut()
        prob = C.c_float(0)
        self._chk(self.L.arucohip_board_detect(self.h, _ptr(m) if len(m) else None, len(m), _ptr(ida), _ptr(oa), len(ida), info_type,
                                               _ptr(Ka), _ptr(da), 0 if da is None else da.size, float(marker_size),
                                               float(repj_err_thres), int(bool(y_perp)), _ptr(outm), C.byref(bo), C.byref(prob)))
        return {"prob": prob.value, "markers": outm[:bo.n_markers].copy(), "has_pose": bo.has_pose,
                "rvec": np.array(bo.rvec), "tvec": np.array(bo.tvec)}

    def enable_timing(self, on=True):
        self.L.arucohip_enable_timing(self.h, int(on))

    def stage_times(self):
        ms = (C.c_float * 8)()
        n = self.L.arucohip_stage_times(self.h, ms, 8)
        return {self.L.arucohip_stage_name(i).decode(): ms[i] for i in range(n)}

    def kernel_times(self):
        ms = (C.c_float * 16)()
        n = self.L.arucohip_kernel_times(self.h, ms, 16)
        return {self.L.arucohip_kernel_name(i).decode(): ms[i] for i in range(n)}

    def threshold_exec_ms(self):
        """(total ms, launches) of the wide threshold kernel since enable_timing(True), from the device clock stamps of its waves."""
        ms, n = C.c_double(0), C.c_int(0)
        self._chk(self.L.arucohip_threshold_exec_ms(self.h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def debug_counters(self):
        c = np.zeros(8, np.uint32)
        self._chk(self.L.arucohip_debug_counters(self.h, _ptr(c)))
        seg = bool(c[5])   # [4] counts what the batch's contour pipeline keeps: waypoint records (segments) or long walks; the other key is None
        return {"raw": int(c[4]) if seg else None, "triggers": int(c[0]), "contours": int(c[1]), "points": int(c[2]), "status": int(c[3]),
                "long_walks": None if seg else int(c[4]),   # walker mode: [4] = long walks (checkpoint rings handed out)
                "late_walks": int(c[6]),   # of them: walks that reached the late generations (borders above 960 points)
                "side_streams": int(c[7])}   # workers of the batch that own a side stream for those generations (a pipeline lane: 0)

    def debug_plane_counters(self, plane):
        """arucohip_debug_plane_counters: fill levels and overflow bits of one threshold plane (frame * planes per frame + t) of the last
        batch, as the kernels left them. The counters keep counting past the capacities: they are the plane's demand."""
        line = np.zeros(PLANE_COUNTER_WORDS, np.uint32)
        self._chk(self.L.arucohip_debug_plane_counters(self.h, int(plane), _ptr(line), line.size))
        seg = bool(line[PC_SEGMENTS])
        return {"starts": (int(line[0]), int(line[1])), "contours": int(line[2]), "points": int(line[3]), "status": int(line[5]),
                "late_contours": int(line[6]), "rings": None if seg else (int(line[32]), int(line[33])), "raw": int(line[34]) if seg else None,
                "segments": seg}

    def gl_modelview_batch(self, nframes, cap=64):
        """Marker::glGetModelViewMatrix for every marker of the last batch (device kernel): list per frame of [n][16]."""
        mv = np.zeros((nframes, cap, 16), np.float64)
        n = np.zeros(nframes, np.int32)
        self._chk(self.L.arucohip_gl_modelview_batch(self.h, nframes, cap, _ptr(mv), _ptr(n)))
        return [mv[f, :max(int(n[f]), 0)].copy() for f in range(nframes)]   # n = -1: a frame the batch gave up

    def board_detect_batch(self, nframes, ids, obj, info_type, K=None, dist=None, marker_size=-1.0, repj_err_thres=-1.0, y_perp=False):
        """BoardDetector::detect on the device-resident markers of the last detect_batch call, all frames at once."""
        ida = np.ascontiguousarray(ids, dtype=np.int32)
        oa = _f32(obj)
        Ka, da = _f32(K), _f32(dist)
        out = (BoardOut * nframes)()
        prob = np.zeros(nframes, np.float32)
        self._chk(self.L.arucohip_board_detect_batch(self.h, nframes, _ptr(ida), _ptr(oa), len(ida), info_type, _ptr(Ka), _ptr(da),
                                                     0 if da is None else da.size, float(marker_size), float(repj_err_thres),
                                                     int(bool(y_perp)), out, _ptr(prob)))
        return [{"n_markers": out[f].n_markers, "has_pose": out[f].has_pose, "rvec": np.array(out[f].rvec), "tvec": np.array(out[f].tvec),
                 "prob": float(prob[f])} for f in range(nframes)]

    def board_recover_batch(self, nframes, ids, obj, info_type, K, dist=None, marker_size=-1.0, repj_err_thres=-1.0, y_perp=False, opt=None,
                            cap=64, allow=()):
        """arucohip_board_recover_batch on the last batch: the board's markers that the decoder rejected are taken back from the frames'
        rejected candidates, in place. opt: a Recover (None: the defaults). Returns (markers per frame, counts, recovered per frame,
        boards as board_detect_batch returns them); counts[f] = -1 for a frame the batch gave up. cap = 0: the marker lists are not
        fetched (empty lists, counts None)."""
        ida = np.ascontiguousarray(ids, dtype=np.int32)
        oa = _f32(obj)
        Ka, da = _f32(K), _f32(dist)
        out = np.zeros((nframes, cap), MARKER_DTYPE)
        n = np.zeros(nframes, np.int32)
        rec = np.zeros(nframes, np.int32)
        boards = (BoardOut * nframes)()
        prob = np.zeros(nframes, np.float32)
        self._chk(self.L.arucohip_board_recover_batch(self.h, int(nframes), _ptr(ida), _ptr(oa), len(ida), int(info_type), _ptr(Ka), _ptr(da),
                                                      0 if da is None else da.size, float(marker_size), float(repj_err_thres), int(bool(y_perp)),
                                                      None if opt is None else C.cast(C.byref(opt), C.c_void_p), _ptr(out) if cap else None, int(cap),
                                                      _ptr(n) if cap else None, 0, _ptr(rec), boards, _ptr(prob)), allow=allow)
        bl = [{"n_markers": boards[f].n_markers, "has_pose": boards[f].has_pose, "rvec": np.array(boards[f].rvec), "tvec": np.array(boards[f].tvec),
               "prob": float(prob[f])} for f in range(nframes)]
        return [out[f, :max(min(int(n[f]), cap), 0)].copy() for f in range(nframes)], n if cap else None, rec, bl

    def board_recover_batch_device(self, nframes, ids, obj, info_type, out_ptr, cap, n_out_ptr, K, dist=None, marker_size=-1.0, repj_err_thres=-1.0,
                                   y_perp=False, opt=None):
        """board_recover_batch with the marker lists written to device arrays (arucohip_marker_t [nframes][cap], int32 [nframes], given as
        pointers): asynchronous on the handle's stream, for a detect -> recover -> draw chain."""
        ida = np.ascontiguousarray(ids, dtype=np.int32)
        oa = _f32(obj)
        Ka, da = _f32(K), _f32(dist)
        self._chk(self.L.arucohip_board_recover_batch(self.h, int(nframes), _ptr(ida), _ptr(oa), len(ida), int(info_type), _ptr(Ka), _ptr(da),
                                                      0 if da is None else da.size, float(marker_size), float(repj_err_thres), int(bool(y_perp)),
                                                      None if opt is None else C.cast(C.byref(opt), C.c_void_p), C.c_void_p(out_ptr), int(cap),
                                                      C.c_void_p(n_out_ptr), 1, None, None, None))

    @staticmethod
    def _calib_start(K, dist):
        Ka = np.zeros(9) if K is None else np.array(K, dtype=np.float64).reshape(9)
        da = np.zeros(5) if dist is None else np.array(dist, dtype=np.float64).reshape(-1)
        if da.size != 5:
            raise ValueError("dist must hold 5 coefficients (k1, k2, p1, p2, k3)")
        return Ka, da

    def calibrate_camera(self, obj_list, img_list, image_size, flags=0, K=None, dist=None):
        """cv::calibrateCamera on planar views: obj_list[v] (n, 3), img_list[v] (n, 2); image_size = (width, height). K / dist: the
        start with CALIB_USE_INTRINSIC_GUESS, K's fx / fy ratio with CALIB_FIX_ASPECT_RATIO."""
        if len(obj_list) != len(img_list):
            raise ValueError("obj_list and img_list differ in length")
        objs = [np.asarray(o, np.float32).reshape(-1, 3) for o in obj_list]
        imgs = [np.asarray(m, np.float32).reshape(-1, 2) for m in img_list]
        if any(len(o) != len(m) for o, m in zip(objs, imgs)):
            raise ValueError("a view has different numbers of object and image points")
        npts = np.array([len(o) for o in objs], np.int32)
        oa = np.ascontiguousarray(np.concatenate(objs) if objs else np.zeros((0, 3), np.float32))
        ia = np.ascontiguousarray(np.concatenate(imgs) if imgs else np.zeros((0, 2), np.float32))
        Ka, da = self._calib_start(K, dist)
        V = len(objs)
        rv, tv, pv, rms = np.zeros((V, 3)), np.zeros((V, 3)), np.zeros(V), C.c_double()
        self._chk(self.L.arucohip_calibrate_camera(self.h, _ptr(oa), _ptr(ia), _ptr(npts), V, 0, int(image_size[0]), int(image_size[1]),
                                                   int(flags), _ptr(Ka), _ptr(da), _ptr(rv), _ptr(tv), _ptr(pv), C.byref(rms)))
        return {"rms": rms.value, "K": Ka.reshape(3, 3), "dist": da, "rvecs": rv, "tvecs": tv, "per_view_rms": pv}

    def calibrate_camera_device(self, obj_ptr, img_ptr, npoints_ptr, nviews, image_size, flags=0, K=None, dist=None):
        """calibrate_camera on device arrays (obj float32 [N,3], img float32 [N,2], npoints int32 [nviews], given as pointers)."""
        Ka, da = self._calib_start(K, dist)
        rv, tv, pv, rms = np.zeros((nviews, 3)), np.zeros((nviews, 3)), np.zeros(nviews), C.c_double()
        self._chk(self.L.arucohip_calibrate_camera(self.h, obj_ptr, img_ptr, npoints_ptr, nviews, 1, int(image_size[0]), int(image_size[1]),
                                                   int(flags), _ptr(Ka), _ptr(da), _ptr(rv), _ptr(tv), _ptr(pv), C.byref(rms)))
        return {"rms": rms.value, "K": Ka.reshape(3, 3), "dist": da, "rvecs": rv, "tvecs": tv, "per_view_rms": pv}

    def debug_calib_start(self, obj_list, img_list, image_size, flags=0, K=None, dist=None, fisheye=False):
        """arucohip_debug_calib_start: the start values of calibrate_camera (or, with fisheye, of fisheye_calibrate: K and dist = D are its
        model, flags its FISHEYE_*) on the same views: intr [9], poses [V, 6] (rvec, tvec), cost and the start kernels' err bits."""
        objs = [np.asarray(o, np.float32).reshape(-1, 3) for o in obj_list]
        imgs = [np.asarray(m, np.float32).reshape(-1, 2) for m in img_list]
        if len(objs) != len(imgs) or any(len(o) != len(m) for o, m in zip(objs, imgs)):
            raise ValueError("the views' object and image points differ in number")
        npts = np.array([len(o) for o in objs], np.int32)
        oa, ia = np.ascontiguousarray(np.concatenate(objs)), np.ascontiguousarray(np.concatenate(imgs))
        Ka = np.zeros(9) if K is None else np.array(K, dtype=np.float64).reshape(9)
        da = np.zeros(5)
        if dist is not None:
            dd = np.asarray(dist, np.float64).reshape(-1)
            da[:dd.size] = dd
        V = len(objs)
        intr, poses, cost, err = np.zeros(9), np.zeros((V, 6)), C.c_double(), C.c_int32()
        self._chk(self.L.arucohip_debug_calib_start(self.h, _ptr(oa), _ptr(ia), _ptr(npts), V, 0, int(image_size[0]), int(image_size[1]), int(flags),
                                                    int(bool(fisheye)), _ptr(Ka), _ptr(da), _ptr(intr), _ptr(poses), C.byref(cost), C.byref(err)))
        return {"intr": intr, "poses": poses, "cost": cost.value, "err": err.value}

    def calibrate_board_batch(self, nframes, ids, obj, info_type, image_size, marker_size=-1.0, min_markers=4, flags=0, K=None, dist=None):
        """calibrate_camera on the board detections of the last detect_batch call, left on the device: frames with at least
        min_markers board markers are the views. rvecs / tvecs have one row per used frame; used[f] marks them."""
        ida = np.ascontiguousarray(ids, dtype=np.int32)
        oa = _f32(obj)
        Ka, da = self._calib_start(K, dist)
        used = np.zeros(nframes, np.int32)
        rv, tv, rms = np.zeros((nframes, 3)), np.zeros((nframes, 3)), C.c_double()
        self._chk(self.L.arucohip_calibrate_board_batch(self.h, nframes, _ptr(ida), _ptr(oa), len(ida), info_type, float(marker_size),
                                                        int(min_markers), int(image_size[0]), int(image_size[1]), int(flags), _ptr(Ka),
                                                        _ptr(da), _ptr(used), _ptr(rv), _ptr(tv), C.byref(rms)))
        nv = int(used.sum())
        return {"rms": rms.value, "K": Ka.reshape(3, 3), "dist": da, "rvecs": rv[:nv], "tvecs": tv[:nv], "used": used.astype(bool)}

    # ---- fisheye calibration: model = (K, D) is the start with FISHEYE_USE_INTRINSIC_GUESS, K's fx / fy ratio with FISHEYE_FIX_ASPECT_RATIO
    @staticmethod
    def _fisheye_start(model):
        m = Fisheye()
        if model is not None:
            m = fisheye_models((model[0], model[1]))[0]
        return m

    @staticmethod
    def _fisheye_result(m, rms, **more):
        return dict({"rms": rms.value, "K": np.array(list(m.K)).reshape(3, 3), "D": np.array(list(m.D))}, **more)

    def fisheye_calibrate(self, obj_list, img_list, image_size, flags=0, model=None):
        """arucohip_fisheye_calibrate on planar views: obj_list[v] (n, 3), img_list[v] (n, 2); image_size = (width, height)."""
        if len(obj_list) != len(img_list):
            raise ValueError("obj_list and img_list differ in length")
        objs = [np.asarray(o, np.float32).reshape(-1, 3) for o in obj_list]
        imgs = [np.asarray(p, np.float32).reshape(-1, 2) for p in img_list]
        if any(len(o) != len(p) for o, p in zip(objs, imgs)):
            raise ValueError("a view has different numbers of object and image points")
        npts = np.array([len(o) for o in objs], np.int32)
        oa = np.ascontiguousarray(np.concatenate(objs) if objs else np.zeros((0, 3), np.float32))
        ia = np.ascontiguousarray(np.concatenate(imgs) if imgs else np.zeros((0, 2), np.float32))
        m = self._fisheye_start(model)
        V = len(objs)
        rv, tv, pv, rms = np.zeros((V, 3)), np.zeros((V, 3)), np.zeros(V), C.c_double()
        self._chk(self.L.arucohip_fisheye_calibrate(self.h, _ptr(oa), _ptr(ia), _ptr(npts), V, 0, int(image_size[0]), int(image_size[1]), int(flags),
                                                    C.byref(m), _ptr(rv), _ptr(tv), _ptr(pv), C.byref(rms)))
        return self._fisheye_result(m, rms, rvecs=rv, tvecs=tv, per_view_rms=pv)

    def fisheye_calibrate_device(self, obj_ptr, img_ptr, npoints_ptr, nviews, image_size, flags=0, model=None):
        """fisheye_calibrate on device arrays (obj float32 [N,3], img float32 [N,2], npoints int32 [nviews], given as pointers)."""
        m = self._fisheye_start(model)
        rv, tv, pv, rms = np.zeros((nviews, 3)), np.zeros((nviews, 3)), np.zeros(nviews), C.c_double()
        self._chk(self.L.arucohip_fisheye_calibrate(self.h, obj_ptr, img_ptr, npoints_ptr, nviews, 1, int(image_size[0]), int(image_size[1]), int(flags),
                                                    C.byref(m), _ptr(rv), _ptr(tv), _ptr(pv), C.byref(rms)))
        return self._fisheye_result(m, rms, rvecs=rv, tvecs=tv, per_view_rms=pv)

    def fisheye_calibrate_board_batch(self, nframes, ids, obj, info_type, image_size, marker_size=-1.0, min_markers=4, flags=0, model=None):
        """fisheye_calibrate on the board detections of the last detect_batch call, left on the device: frames with at least min_markers
        board markers are the views. rvecs / tvecs have one row per used frame; used[f] marks them."""
        ida = np.ascontiguousarray(ids, dtype=np.int32)
        oa = _f32(obj)
        m = self._fisheye_start(model)
        used = np.zeros(nframes, np.int32)
        rv, tv, rms = np.zeros((nframes, 3)), np.zeros((nframes, 3)), C.c_double()
        self._chk(self.L.arucohip_fisheye_calibrate_board_batch(self.h, nframes, _ptr(ida), _ptr(oa), len(ida), info_type, float(marker_size),
                                                                int(min_markers), int(image_size[0]), int(image_size[1]), int(flags), C.byref(m),
                                                                _ptr(used), _ptr(rv), _ptr(tv), C.byref(rms)))
        nv = int(used.sum())
        return self._fisheye_result(m, rms, rvecs=rv[:nv], tvecs=tv[:nv], used=used.astype(bool))

    # ---- marker mapping: the 3-D layout of a rigid marker set
    def _map_call(self, fn, head, nframes, board_ids, K, dist, marker_size, tail=()):
        ida = np.ascontiguousarray(board_ids, dtype=np.int32).reshape(-1)
        nb = len(ida)
        Ka, da = _f32(K), _f32(dist)
        obj, rv, tv = np.zeros((max(nb, 1), 4, 3), np.float32), np.zeros((max(nb, 1), 3)), np.zeros((max(nb, 1), 3))
        mapped, used = np.zeros(max(nb, 1), np.int32), np.zeros(max(nframes, 1), np.int32)
        frv, ftv, mrms = np.zeros((max(nframes, 1), 3)), np.zeros((max(nframes, 1), 3)), np.zeros(max(nb, 1))
        rms, it = C.c_double(), C.c_int32()
        self._chk(fn(self.h, *head, int(nframes), _ptr(ida), nb, _ptr(Ka), _ptr(da), 0 if da is None else da.size, float(marker_size), *tail,
                     _ptr(obj), _ptr(rv), _ptr(tv), _ptr(mapped), _ptr(used), _ptr(frv), _ptr(ftv), _ptr(mrms), C.byref(rms), C.byref(it)))
        return {"obj": obj[:nb], "marker_rvecs": rv[:nb], "marker_tvecs": tv[:nb], "mapped": mapped[:nb].astype(bool),
                "used": used[:nframes].astype(bool), "frame_rvecs": frv[:nframes], "frame_tvecs": ftv[:nframes], "marker_rms": mrms[:nb],
                "rms": rms.value, "iterations": it.value}

    def board_map(self, frames, ids, corners, nframes, board_ids, K, dist, marker_size):
        """arucohip_board_map: the placement of every marker of board_ids in the frame of the first one, from observations given as
        parallel arrays (frame index, id, 4 corners). Returns obj float32 [n][4][3] in metres (board_detect's obj with BOARD_METERS),
        marker_rvecs / marker_tvecs [n][3], mapped [n], used [nframes], frame_rvecs / frame_tvecs [nframes][3] (zeros where not used),
        marker_rms [n], rms, iterations."""
        fa = np.ascontiguousarray(frames, dtype=np.int32).reshape(-1)
        ia = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
        ca = np.ascontiguousarray(corners, dtype=np.float32).reshape(-1, 8)
        if not len(fa) == len(ia) == len(ca):
            raise ValueError("frames, ids and corners differ in length")
        head = (_ptr(fa) if len(fa) else None, _ptr(ia) if len(fa) else None, _ptr(ca) if len(fa) else None, len(fa), 0)
        return self._map_call(self.L.arucohip_board_map, head, nframes, board_ids, K, dist, marker_size)

    def board_map_device(self, frames_ptr, ids_ptr, corners_ptr, nobs, nframes, board_ids, K, dist, marker_size):
        """board_map on device arrays (int32 [nobs], int32 [nobs], float32 [nobs][8], given as pointers)."""
        head = (C.c_void_p(frames_ptr), C.c_void_p(ids_ptr), C.c_void_p(corners_ptr), int(nobs), 1)
        return self._map_call(self.L.arucohip_board_map, head, nframes, board_ids, K, dist, marker_size)

    def board_map_batch(self, nframes, board_ids, K, dist, marker_size, min_markers=2):
        """board_map on the device-resident markers of the first nframes frames of the last detect_batch call."""
        return self._map_call(self.L.arucohip_board_map_batch, (), nframes, board_ids, K, dist, marker_size, tail=(int(min_markers),))

    # ---- camera rigs: extrinsics between cameras, one board pose from all of them
    @staticmethod
    def rig_cameras(cams):
        """A RigCamera array from a list of dicts: K, dist (None, 4 or 5 coefficients) and, for rig_pose, calibrated / rvec / tvec (as
        rig_calibrate returns them). A RigCamera array passes through."""
        if isinstance(cams, C.Array):
            return cams
        arr = (RigCamera * max(len(cams), 1))()
        for rc, cam in zip(arr, cams):
            rc.K[:] = [float(v) for v in np.asarray(cam["K"], np.float32).reshape(9)]
            dist = cam.get("dist")
            da = np.zeros(0, np.float32) if dist is None else np.asarray(dist, np.float32).reshape(-1)
            rc.ndist = int(cam.get("ndist", da.size))
            for k in range(min(da.size, 5)):
                rc.dist[k] = float(da[k])
            rc.calibrated = int(bool(cam.get("calibrated", False)))
            rc.rvec[:] = [float(v) for v in np.asarray(cam.get("rvec", np.zeros(3)), np.float64).reshape(3)]
            rc.tvec[:] = [float(v) for v in np.asarray(cam.get("tvec", np.zeros(3)), np.float64).reshape(3)]
        return arr

    @staticmethod
    def _rig_obs(views, ids, corners):
        va = np.ascontiguousarray(views, dtype=np.int32).reshape(-1)
        ia = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
        ca = np.ascontiguousarray(corners, dtype=np.float32).reshape(-1, 8)
        if not len(va) == len(ia) == len(ca):
            raise ValueError("views, ids and corners differ in length")
        n = len(va)
        return (va, ia, ca), (_ptr(va) if n else None, _ptr(ia) if n else None, _ptr(ca) if n else None, n, 0)

    def _rig_calibrate_call(self, fn, head, ninstants, cams, ncams, board_ids, obj, info_type, marker_size, min_markers):
        arr = self.rig_cameras(cams)
        ncams = len(cams) if ncams is None else int(ncams)
        ida = np.ascontiguousarray(board_ids, dtype=np.int32).reshape(-1)
        oa = _f32(obj)
        T = max(int(ninstants), 1)
        used, brv, btv, crms = np.zeros(T, np.int32), np.zeros((T, 3)), np.zeros((T, 3)), np.zeros(max(ncams, 1))
        rms, it = C.c_double(), C.c_int32()
        self._chk(fn(self.h, *head, C.cast(arr, C.c_void_p), ncams, _ptr(ida), _ptr(oa), len(ida), int(info_type), float(marker_size), int(min_markers),
                     _ptr(used), _ptr(brv), _ptr(btv), _ptr(crms), C.byref(rms), C.byref(it)))
        n = min(ncams, len(arr))
        return {"cams": arr, "calibrated": np.array([bool(arr[c].calibrated) for c in range(n)]),
                "rvecs": np.array([list(arr[c].rvec) for c in range(n)]), "tvecs": np.array([list(arr[c].tvec) for c in range(n)]),
                "used": used[:ninstants].astype(bool), "board_rvecs": brv[:ninstants], "board_tvecs": btv[:ninstants], "camera_rms": crms[:ncams],
                "rms": rms.value, "iterations": it.value}

    def rig_calibrate(self, views, ids, corners, ninstants, cams, board_ids, obj, info_type, marker_size=-1.0, min_markers=1, ncams=None):
        """arucohip_rig_calibrate: the transforms rig -> camera of cams (a list of dicts K / dist, or a RigCamera array; camera 0 is the rig
        frame) from observations given as parallel arrays (view index = instant * ncams + camera, id, 4 corners). Returns cams (the RigCamera
        array, as rig_pose takes it), calibrated [ncams], rvecs / tvecs [ncams][3], used [ninstants], board_rvecs / board_tvecs
        [ninstants][3] (zeros where not used), camera_rms [ncams], rms, iterations."""
        keep, head = self._rig_obs(views, ids, corners)
        return self._rig_calibrate_call(self.L.arucohip_rig_calibrate, head + (int(ninstants),), ninstants, cams, ncams, board_ids, obj, info_type,
                                        marker_size, min_markers)

    def rig_calibrate_device(self, views_ptr, ids_ptr, corners_ptr, nobs, ninstants, cams, board_ids, obj, info_type, marker_size=-1.0, min_markers=1):
        """rig_calibrate on device arrays (int32 [nobs], int32 [nobs], float32 [nobs][8], given as pointers)."""
        head = (C.c_void_p(views_ptr), C.c_void_p(ids_ptr), C.c_void_p(corners_ptr), int(nobs), 1, int(ninstants))
        return self._rig_calibrate_call(self.L.arucohip_rig_calibrate, head, ninstants, cams, None, board_ids, obj, info_type, marker_size, min_markers)

    def rig_calibrate_batch(self, nframes, cams, board_ids, obj, info_type, marker_size=-1.0, min_markers=1):
        """rig_calibrate on the device-resident markers of the first nframes frames of the last detect_batch call: frame f is view f."""
        ninstants = int(nframes) // max(len(cams), 1)
        return self._rig_calibrate_call(self.L.arucohip_rig_calibrate_batch, (int(nframes),), ninstants, cams, None, board_ids, obj, info_type,
                                        marker_size, min_markers)

    def _rig_pose_call(self, fn, head, ninstants, cams, ncams, board_ids, obj, info_type, marker_size, min_markers):
        arr = self.rig_cameras(cams)
        ncams = len(cams) if ncams is None else int(ncams)
        ida = np.ascontiguousarray(board_ids, dtype=np.int32).reshape(-1)
        oa = _f32(obj)
        T = max(int(ninstants), 1)
        out = (BoardOut * T)()
        vu = np.zeros(T, np.int32)
        self._chk(fn(self.h, *head, C.cast(arr, C.c_void_p), ncams, _ptr(ida), _ptr(oa), len(ida), int(info_type), float(marker_size), int(min_markers),
                     C.cast(out, C.c_void_p), _ptr(vu)))
        return [{"n_markers": out[t].n_markers, "has_pose": out[t].has_pose, "rvec": np.array(out[t].rvec), "tvec": np.array(out[t].tvec),
                 "views_used": int(vu[t])} for t in range(ninstants)]

    def rig_pose(self, views, ids, corners, ninstants, cams, board_ids, obj, info_type, marker_size=-1.0, min_markers=1, ncams=None):
        """arucohip_rig_pose: the board's pose in the rig frame at every instant, from every calibrated camera whose view counts. cams: the
        `cams` of rig_calibrate, or dicts with K, dist, calibrated, rvec, tvec. Returns a list of dicts n_markers, has_pose, rvec, tvec,
        views_used."""
        keep, head = self._rig_obs(views, ids, corners)
        return self._rig_pose_call(self.L.arucohip_rig_pose, head + (int(ninstants),), ninstants, cams, ncams, board_ids, obj, info_type, marker_size,
                                   min_markers)

    def rig_pose_batch(self, nframes, cams, board_ids, obj, info_type, marker_size=-1.0, min_markers=1):
        """rig_pose on the device-resident markers of the first nframes frames of the last detect_batch call: frame f is view f."""
        ninstants = int(nframes) // max(len(cams), 1)
        return self._rig_pose_call(self.L.arucohip_rig_pose_batch, (int(nframes),), ninstants, cams, None, board_ids, obj, info_type, marker_size,
                                   min_markers)

    # ---- chessboard-corner (ChArUco) boards
    def charuco_board_image(self, layout, ids, centered=False):
        """The board image of a layout with the caller's marker ids: (image uint8 [H][W], objPoints of the markers float32 [markers][4][3],
        object points of the inner corners float32 [corners][3]), in pixels."""
        a = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
        try:
            w, hh, nm, nc = charuco_board_size(layout)
        except ArucoHipError:
            w, hh, nm, nc = 1, 1, 1, 1   # the call below reports the error with its message
        img = np.zeros((hh, w), np.uint8)
        obj, cobj = np.zeros((nm, 4, 3), np.float32), np.zeros((nc, 3), np.float32)
        self._chk(self.L.arucohip_charuco_board_image(self.h, C.byref(layout), int(bool(centered)), _ptr(a), a.size, _ptr(img), w, 0, _ptr(obj),
                                                      _ptr(cobj)))
        return img, obj, cobj

    def charuco_corners_batch(self, layout, ids, frames, opt=None, width=None):
        """The chessboard's inner corners in the frames of the last batch, from its device-resident markers. frames: the gray planes that
        batch saw, uint8 [N][H][W] (numpy, or a torch tensor on the handle's device), or [N][H][row_stride] with `width` given. Returns
        (records CHARUCO_CORNER_DTYPE [N][corners], found corners per frame int32 [N]); the records also stay on the device for
        charuco_calibrate_batch and charuco_pose_batch."""
        a = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
        ptr, n, wid, hgt, _, rs, fs, dev = self._frames(frames, width, 1)
        try:
            nc = charuco_board_size(layout)[3]
        except ArucoHipError:
            nc = 1
        out = np.zeros((n, nc), CHARUCO_CORNER_DTYPE)
        nf = np.zeros(n, np.int32)
        self._chk(self.L.arucohip_charuco_corners_batch(self.h, C.byref(layout), _ptr(a), a.size, ptr, n, wid, hgt, rs, fs, dev,
                                                        None if opt is None else C.cast(C.pointer(opt), C.c_void_p), _ptr(out), _ptr(nf), 0))
        self._charuco_frames = n
        return out, nf

    def charuco_corners_batch_device(self, layout, ids, frames_ptr, nframes, width, height, out_ptr, opt=None, row_stride=None, frame_stride=None):
        """charuco_corners_batch on device frames into a device array of nframes * corners records, both given as pointers; returns the found
        corners per frame."""
        a = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
        rs = int(width) if row_stride is None else int(row_stride)
        fs = rs * int(height) if frame_stride is None else int(frame_stride)
        nf = np.zeros(nframes, np.int32)
        self._chk(self.L.arucohip_charuco_corners_batch(self.h, C.byref(layout), _ptr(a), a.size, C.c_void_p(frames_ptr), int(nframes), int(width),
                                                        int(height), rs, fs, 1, None if opt is None else C.cast(C.pointer(opt), C.c_void_p),
                                                        C.c_void_p(out_ptr), _ptr(nf), 1))
        self._charuco_frames = int(nframes)
        return nf

    def charuco_calibrate_batch(self, image_size, square_size=-1.0, min_corners=4, flags=0, K=None, dist=None):
        """calibrate_camera on the corners the last charuco_corners_batch left on the device: frames with at least min_corners found corners are
        the views. rvecs / tvecs have one row per used frame; used[f] marks them."""
        Ka, da = self._calib_start(K, dist)
        nframes = max(getattr(self, "_charuco_frames", 0), 1)   # without resident corners the library reports the error
        used = np.zeros(nframes, np.int32)
        rv, tv, rms = np.zeros((nframes, 3)), np.zeros((nframes, 3)), C.c_double()
        self._chk(self.L.arucohip_charuco_calibrate_batch(self.h, float(square_size), int(min_corners), int(image_size[0]), int(image_size[1]),
                                                          int(flags), _ptr(Ka), _ptr(da), _ptr(used), _ptr(rv), _ptr(tv), C.byref(rms)))
        nv = int(used.sum())
        return {"rms": rms.value, "K": Ka.reshape(3, 3), "dist": da, "rvecs": rv[:nv], "tvecs": tv[:nv], "used": used.astype(bool)}

    def charuco_pose_batch(self, nframes, K, dist=None, square_size=-1.0, min_corners=4, y_perp=False):
        """The board pose of every frame from the resident corners: a BOARD_DTYPE array, n_markers = the corners used."""
        Ka, da = _f32(K), _f32(dist)
        out = np.zeros(max(int(nframes), 1), BOARD_DTYPE)
        self._chk(self.L.arucohip_charuco_pose_batch(self.h, int(nframes), _ptr(Ka), _ptr(da), 0 if da is None else da.size, float(square_size),
                                                     int(min_corners), int(bool(y_perp)), _ptr(out)))
        return out[:max(int(nframes), 0)]

    def chromatic(self, mc, nc, thresh_prob, K, dist, width, height, corners):
        """ChromaticMask::setParams(mc, nc, threshProb, CP, BC, corners) on this handle's device and stream: see Chromatic."""
        return Chromatic(self, mc, nc, thresh_prob, K, dist, width, height, corners)

    def em_fit(self, samples_hist, thresh_prob, prob=None):
        """EMClassifier::train on one cell's raw-sample histogram (256 counts): (prob[256], inside[256], trained). prob starts at 0.5
        (a fresh classifier) unless given; it is returned unchanged when fewer than 10 discretised samples remain."""
        hist = np.ascontiguousarray(samples_hist, dtype=np.uint32).reshape(256)
        p = np.full(256, 0.5) if prob is None else np.array(prob, dtype=np.float64).reshape(256)
        inside = (p > thresh_prob).astype(np.uint8)
        t = C.c_int()
        self._chk(self.L.arucohip_em_fit(self.h, _ptr(hist), float(thresh_prob), _ptr(p), _ptr(inside), C.byref(t)))
        return p, inside.astype(bool), bool(t.value)

    def hrm_create_dictionary(self, n, size, seed):
        """HighlyReliableMarkers::createDicitionary(size, n) right after srand(seed), on the device: (codes uint64 [size] in
        arucohip_set_dictionary's bit layout, tau0, candidates examined)."""
        codes = np.zeros(max(int(size), 1), np.uint64)
        tau0, ex = C.c_int(), C.c_int64()
        self._chk(self.L.arucohip_hrm_create_dictionary(self.h, int(n), int(size), int(seed) & 0xFFFFFFFF, _ptr(codes), C.byref(tau0),
                                                        C.byref(ex)))
        return codes, tau0.value, ex.value

    def hrm_board_image(self, codes, n, grid, chromatic=False, ids=True):
        """HighlyReliableMarkers::createBoardImage(Size(grid[0], grid[1]), D, BC, chromatic) on the device: (image [H][W] or
        [H][W][3] BGR uint8, ids int32 (None for n >= 6 or ids=False), obj float32 [gw * gh][4][3])."""
        gw, gh = int(grid[0]), int(grid[1])
        c = np.ascontiguousarray(codes, dtype=np.uint64)
        w, hh, ch = C.c_int(), C.c_int(), C.c_int()
        rc = self.L.arucohip_hrm_board_size(int(n), gw, gh, int(bool(chromatic)), C.byref(w), C.byref(hh), C.byref(ch))
        if rc != OK:
            raise ArucoHipError(rc, "arucohip_hrm_board_size")
        img = np.zeros((hh.value, w.value, ch.value), np.uint8)
        want_ids = ids and int(n) <= 5
        ida = np.zeros(gw * gh, np.int32) if want_ids else None
        obj = np.zeros((gw * gh, 4, 3), np.float32)
        self._chk(self.L.arucohip_hrm_board_image(self.h, int(n), c.size, _ptr(c), gw, gh, int(bool(chromatic)), _ptr(img), w.value * ch.value,
                                                  0, _ptr(ida), _ptr(obj)))
        return (img if chromatic else img[:, :, 0]), ida, obj

    def fiducial_marker_images(self, ids, size, locked=False):
        """FiducidalMarkers::createMarkerImage(id, size, false, locked) for every id, one launch: uint8 [len(ids)][side][side]."""
        a = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
        side = max(fiducial_marker_side(size, locked), 1)
        out = np.zeros((max(a.size, 1), side, side), np.uint8)
        self._chk(self.L.arucohip_fiducial_marker_images(self.h, _ptr(a), a.size, int(size), int(bool(locked)), _ptr(out), side, side * side, 0))
        return out[:a.size]

    def fiducial_board_image(self, board_type, grid, marker_size, marker_distance, ids, centered=True):
        """createBoardImage / _ChessBoard / _Frame (board_type FIDUCIAL_*) with the caller's ids: (image uint8 [H][W], the ids the
        layout used int32 [markers], objPoints float32 [markers][4][3] in pixels)."""
        a = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
        try:
            w, hh, _, nm = fiducial_board_size(board_type, grid, marker_size, marker_distance)
        except ArucoHipError:
            w, hh, nm = 1, 1, 1   # the call below reports the error with its message
        img = np.zeros((hh, w), np.uint8)
        obj = np.zeros((nm, 4, 3), np.float32)
        self._chk(self.L.arucohip_fiducial_board_image(self.h, int(board_type), int(grid[0]), int(grid[1]), int(marker_size), int(marker_distance),
                                                       int(bool(centered)), _ptr(a), a.size, _ptr(img), w, 0, _ptr(obj)))
        return img, a[:nm].copy(), obj

    def fiducial_distances(self):
        """the 1024 x 1024 int32 matrix of aruco_selectoptimalmarkers: rotation-minimal Hamming distance of every pair of markers"""
        out = np.zeros((1024, 1024), np.int32)
        self._chk(self.L.arucohip_fiducial_distances(self.h, _ptr(out), 0))
        return out

    def fiducial_select(self, n_markers, min_entropy=0):
        """aruco_selectoptimalmarkers: (ids int32 ascending, smallest pairwise distance). Raises ArucoHipError (E_INVALID) where the
        reference gives up; the exception's `partial` holds the ids found until then."""
        out = np.zeros(max(int(n_markers), 1), np.int32)
        n, md = C.c_int(), C.c_int()
        rc = self.L.arucohip_fiducial_select(self.h, int(n_markers), int(min_entropy), _ptr(out), C.byref(n), C.byref(md))
        if rc != OK:
            e = ArucoHipError(rc, (self.L.arucohip_last_error_string(self.h) or b"").decode())
            e.partial = out[:n.value].copy()
            raise e
        return out[:n.value].copy(), md.value

    def debug_hrm_stream(self, seed, offset, count):
        """glibc rand() outputs [offset, offset + count) after srand(seed), made on the device"""
        out = np.zeros(max(int(count), 1), np.uint32)
        self._chk(self.L.arucohip_debug_hrm_stream(self.h, int(seed) & 0xFFFFFFFF, int(offset), int(count), _ptr(out)))
        return out[:int(count)]

    def debug_hrm_counters(self):
        """the last hrm_create_dictionary: dict(windows, syncs, accepted, decrements)"""
        out = np.zeros(4, np.int32)
        self._chk(self.L.arucohip_debug_hrm_counters(self.h, _ptr(out)))
        return dict(zip(("windows", "syncs", "accepted", "decrements"), (int(x) for x in out)))


def chromatic_board_corners(obj, info_type, marker_size=-1.0):
    """ChromaticMask::setParams(.., BC, markersize)'s board corners (4 x 3 float32) from obj[N][4][3]."""
    oa = _f32(obj)
    out = np.zeros(12, np.float32)
    rc = load().arucohip_chromatic_board_corners(_ptr(oa), oa.size // 12, int(info_type), float(marker_size), _ptr(out))
    if rc != OK:
        raise ArucoHipError(rc, "arucohip_chromatic_board_corners")
    return out.reshape(4, 3)


class Chromatic:
    """arucohip_chromatic: the reference's ChromaticMask (board occlusion mask) on the device. Planes are uint8 numpy arrays of the
    create-time size, or device pointers (the *_device forms); poses are rvec / tvec in the corners' units."""

    def __init__(self, handle, mc, nc, thresh_prob, K, dist, width, height, corners):
        self.handle, self.L = handle, handle.L
        self.mc, self.nc, self.width, self.height, self.thresh = mc, nc, width, height, thresh_prob
        self.m = C.c_void_p()
        Ka = _f32(np.asarray(K).reshape(9))
        da = None if dist is None else _f32(np.asarray(dist).reshape(-1))
        ca = _f32(np.asarray(corners).reshape(12))
        handle._chk(self.L.arucohip_chromatic_create(handle.h, mc, nc, float(thresh_prob), _ptr(Ka), _ptr(da), 0 if da is None else da.size,
                                                     width, height, _ptr(ca), C.byref(self.m)))

    def close(self):
        if self.m:
            self.L.arucohip_chromatic_destroy(self.m)
            self.m = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        return self.handle._chk(rc)

    def _plane(self, img):
        a = np.ascontiguousarray(img, dtype=np.uint8)
        if a.shape != (self.height, self.width):
            raise ValueError("plane must be %dx%d" % (self.height, self.width))
        return a

    @staticmethod
    def _pose(rvec, tvec):
        return np.array(rvec, np.float64).reshape(3), np.array(tvec, np.float64).reshape(3)

    def train(self, img, rvec, tvec):
        a, (r, t) = self._plane(img), self._pose(rvec, tvec)
        self._chk(self.L.arucohip_chromatic_train(self.m, _ptr(a), 0, self.width, _ptr(r), _ptr(t)))

    def classify(self, img, rvec, tvec, method=2):
        """method 1: classify, 2: classify2. Returns the mask (0 / 1)."""
        a, (r, t) = self._plane(img), self._pose(rvec, tvec)
        self._chk(self.L.arucohip_chromatic_classify(self.m, _ptr(a), 0, self.width, _ptr(r), _ptr(t), int(method)))
        return self.mask()

    def calculate_grid_image(self, rvec, tvec):
        r, t = self._pose(rvec, tvec)
        self._chk(self.L.arucohip_chromatic_grid(self.m, _ptr(r), _ptr(t)))

    def reset_mask(self):
        self._chk(self.L.arucohip_chromatic_reset_mask(self.m))

    def update(self, img):
        a = self._plane(img)
        self._chk(self.L.arucohip_chromatic_update(self.m, _ptr(a), 0, self.width))

    def train_device(self, ptr, row_stride, rvec, tvec):
        r, t = self._pose(rvec, tvec)
        self._chk(self.L.arucohip_chromatic_train(self.m, ptr, 1, row_stride, _ptr(r), _ptr(t)))

    def classify_device(self, ptr, row_stride, rvec, tvec, method=2):
        r, t = self._pose(rvec, tvec)
        self._chk(self.L.arucohip_chromatic_classify(self.m, ptr, 1, row_stride, _ptr(r), _ptr(t), int(method)))

    def update_device(self, ptr, row_stride):
        self._chk(self.L.arucohip_chromatic_update(self.m, ptr, 1, row_stride))

    def mask(self):
        out = np.zeros((self.height, self.width), np.uint8)
        self._chk(self.L.arucohip_chromatic_get_mask(self.m, _ptr(out), 0))
        return out

    def cell_map(self):
        out = np.zeros((self.height, self.width), np.uint8)
        self._chk(self.L.arucohip_chromatic_get_cell_map(self.m, _ptr(out), 0))
        return out

    def is_valid(self):
        return bool(self.L.arucohip_chromatic_is_valid(self.m))

    def get_model(self):
        """(prob[mc*nc][256] float64, trained[mc*nc] bool)"""
        n = self.mc * self.nc
        p, t = np.zeros((n, 256)), np.zeros(n, np.int32)
        self._chk(self.L.arucohip_chromatic_get_model(self.m, _ptr(p), _ptr(t)))
        return p, t.astype(bool)

    def set_model(self, prob, trained):
        p = np.ascontiguousarray(prob, dtype=np.float64).reshape(self.mc * self.nc, 256)
        t = np.ascontiguousarray(trained, dtype=np.int32).reshape(self.mc * self.nc)
        self._chk(self.L.arucohip_chromatic_set_model(self.m, _ptr(p), _ptr(t)))

    def debug_geometry(self, frame=-1):
        """(corners2d[4][2] float32, H_train[3][3], H_classify[3][3]) of the last single-frame call (frame < 0) or a batch frame"""
        c, ht, hc = np.zeros(8, np.float32), np.zeros(9), np.zeros(9)
        self._chk(self.L.arucohip_chromatic_debug_geometry(self.m, int(frame), _ptr(c), _ptr(ht), _ptr(hc)))
        return c.reshape(4, 2), ht.reshape(3, 3), hc.reshape(3, 3)

    def debug_hist(self):
        """(raw[mc*nc][256], hist_count[mc*nc][256], fitted[mc*nc]) of the last train / update"""
        n = self.mc * self.nc
        raw, hc, fit = np.zeros((n, 256), np.uint32), np.zeros((n, 256), np.uint32), np.zeros(n, np.int32)
        self._chk(self.L.arucohip_chromatic_debug_hist(self.m, _ptr(raw), _ptr(hc), _ptr(fit)))
        return raw, hc, fit

    def classify_batch(self, handle, frames, method=2, min_prob=0.0, npix=True):
        """classify every frame of handle's last detect_batch at its last board_detect_batch poses: frames uint8 [N, H, W] on the host.
        Returns (masks [N, H, W], npix [N] or None)."""
        fa = np.ascontiguousarray(frames, dtype=np.uint8)
        if fa.ndim != 3 or fa.shape[1:] != (self.height, self.width):
            raise ValueError("frames must be [N, %d, %d]" % (self.height, self.width))
        n = fa.shape[0]
        masks = np.zeros((n, self.height, self.width), np.uint8)
        cnt = np.zeros(n, np.int32) if npix else None
        self._chk(self.L.arucohip_chromatic_classify_batch(self.m, handle.h, _ptr(fa), n, self.width, self.height, self.width,
                                                           self.width * self.height, 0, int(method), float(min_prob), _ptr(masks), 0, _ptr(cnt)))
        return masks, cnt

    def classify_batch_device(self, handle, frames_ptr, nframes, row_stride, frame_stride, masks_ptr, method=2, min_prob=0.0, npix=None):
        """device frames and masks (pointers); npix: a host int32 array of nframes, or None"""
        self._chk(self.L.arucohip_chromatic_classify_batch(self.m, handle.h, frames_ptr, nframes, self.width, self.height, row_stride, frame_stride,
                                                           1, int(method), float(min_prob), masks_ptr, 1, _ptr(npix)))


class MultiGpu:
    """arucohip_mgpu_*: frames sharded round-robin over device slots, marker blocks gathered (host or peer/xGMI)."""

    GATHER_HOST, GATHER_PEER = 0, 1

    def __init__(self, devices, max_width, max_height, frames_per_device, cap=64, flags=0, params=None):
        self.L = load()
        self.m = C.c_void_p()
        p = params if params is not None else default_params()
        dv = np.ascontiguousarray(devices, dtype=np.int32)
        rc = self.L.arucohip_mgpu_create(C.byref(p), _ptr(dv), len(dv), max_width, max_height, frames_per_device, cap, flags, C.byref(self.m))
        if rc != OK:
            raise ArucoHipError(rc, "arucohip_mgpu_create")
        self.cap, self.per, self.G = cap, frames_per_device, len(dv)

    def close(self):
        if self.m:
            self.L.arucohip_mgpu_destroy(self.m)
            self.m = C.c_void_p()

    def _chk(self, rc):
        if rc != OK:
            raise ArucoHipError(rc, (self.L.arucohip_mgpu_last_error_string(self.m) or b"").decode())

    def detect_batch_host(self, frames, K=None, dist=None, marker_size=-1.0, y_perp=False):
        fr = np.ascontiguousarray(frames, dtype=np.uint8)
        nf, h, w = fr.shape
        Ka, da = _f32(K), _f32(dist)
        out = np.zeros((nf, self.cap), MARKER_DTYPE)
        n = np.zeros(nf, np.int32)
        self._chk(self.L.arucohip_mgpu_detect_batch(self.m, _ptr(fr), nf, w, h, w, w * h, _ptr(Ka), _ptr(da), 0 if da is None else da.size,
                                                    float(marker_size), int(bool(y_perp)), _ptr(out), self.cap, _ptr(n)))
        return [out[f, :n[f]].copy() for f in range(nf)]

    def set_depth(self, depth):
        self._chk(self.L.arucohip_mgpu_set_depth(self.m, int(depth)))

    def gather_mode(self):
        """GATHER_PEER only if it was asked for and every device reaches the first one; else GATHER_HOST."""
        return int(self.L.arucohip_mgpu_gather_mode(self.m))

    def submit_batch_host(self, frames, K=None, dist=None, marker_size=-1.0, y_perp=False):
        """arucohip_mgpu_submit_batch; returns a job whose arrays stay alive until wait(job)."""
        fr = np.ascontiguousarray(frames, dtype=np.uint8)
        nf, h, w = fr.shape
        Ka, da = _f32(K), _f32(dist)
        out = np.zeros((nf, self.cap), MARKER_DTYPE)
        n = np.zeros(nf, np.int32)
        t = C.c_int(-1)
        self._chk(self.L.arucohip_mgpu_submit_batch(self.m, _ptr(fr), nf, w, h, w, w * h, _ptr(Ka), _ptr(da), 0 if da is None else da.size,
                                                    float(marker_size), int(bool(y_perp)), _ptr(out), self.cap, _ptr(n), C.byref(t)))
        return {"ticket": t.value, "frames": fr, "out": out, "n": n, "K": Ka, "dist": da, "kind": "batch"}

    def submit_streams(self, ptrs, counts, width, height, K=None, dist=None, marker_size=-1.0, y_perp=False):
        pa = (C.c_void_p * self.G)(*[C.c_void_p(int(x)) for x in ptrs])
        ca = np.ascontiguousarray(counts, dtype=np.int32)
        Ka, da = _f32(K), _f32(dist)
        out = np.zeros((self.G * self.per, self.cap), MARKER_DTYPE)
        n = np.zeros(self.G * self.per, np.int32)
        t = C.c_int(-1)
        self._chk(self.L.arucohip_mgpu_submit_streams(self.m, pa, _ptr(ca), width, height, width, width * height, _ptr(Ka), _ptr(da),
                                                      0 if da is None else da.size, float(marker_size), int(bool(y_perp)), _ptr(out), self.cap, _ptr(n), C.byref(t)))
        return {"ticket": t.value, "ptrs": pa, "counts": ca, "out": out, "n": n, "K": Ka, "dist": da, "kind": "streams"}

    def wait(self, job):
        """arucohip_mgpu_wait: per-frame marker arrays of the job (frame order for a batch, [slot][frame] for streams)."""
        self._chk(self.L.arucohip_mgpu_wait(self.m, int(job["ticket"])))
        out, n = job["out"], job["n"]
        if job["kind"] == "batch":
            return [out[f, :n[f]].copy() for f in range(len(n))]
        ca = job["counts"]
        return [[out[g * self.per + j, :n[g * self.per + j]].copy() for j in range(int(ca[g]))] for g in range(self.G)]

    def detect_streams(self, ptrs, counts, width, height, K=None, dist=None, marker_size=-1.0, y_perp=False):
        """ptrs[g] = device pointer of slot g's frames (resident on its device), counts[g] frames each."""
        pa = (C.c_void_p * self.G)(*[C.c_void_p(int(x)) for x in ptrs])
        ca = np.ascontiguousarray(counts, dtype=np.int32)
        Ka, da = _f32(K), _f32(dist)
        out = np.zeros((self.G * self.per, self.cap), MARKER_DTYPE)
        n = np.zeros(self.G * self.per, np.int32)
        self._chk(self.L.arucohip_mgpu_detect_streams(self.m, pa, _ptr(ca), width, height, width, width * height, _ptr(Ka), _ptr(da),
                                                      0 if da is None else da.size, float(marker_size), int(bool(y_perp)), _ptr(out), self.cap, _ptr(n)))
        return [[out[g * self.per + j, :n[g * self.per + j]].copy() for j in range(int(ca[g]))] for g in range(self.G)]


# ---- OpenGL / Ogre conversions (host arithmetic)
def gl_modelview(rvec, tvec):
    """GetGLModelViewMatrix (src/utils.cpp:32-69): 16 doubles, column-major."""
    L = load()
    r, t, m = np.ascontiguousarray(rvec, np.float64), np.ascontiguousarray(tvec, np.float64), np.zeros(16, np.float64)
    rc = L.arucohip_gl_modelview(_ptr(r), _ptr(t), _ptr(m))
    if rc:
        raise ArucoHipError(rc, "gl_modelview")
    return m


def ogre_pose(rvec, tvec):
    """GetOgrePoseParameters (src/utils.cpp:71-147): (position[3], quaternion w,x,y,z)."""
    L = load()
    r, t = np.ascontiguousarray(rvec, np.float64), np.ascontiguousarray(tvec, np.float64)
    pos, q = np.zeros(3, np.float64), np.zeros(4, np.float64)
    rc = L.arucohip_ogre_pose(_ptr(r), _ptr(t), _ptr(pos), _ptr(q))
    if rc:
        raise ArucoHipError(rc, "ogre_pose")
    return pos, q


def gl_projection(K, cam_size, size, gnear, gfar, invert=False, ogre=False):
    """CameraParameters::glGetProjectionMatrix / OgreGetProjectionMatrix (src/cameraparameters.cpp:226-295)."""
    L = load()
    Ka, m = np.ascontiguousarray(K, np.float32).reshape(-1), np.zeros(16, np.float64)
    fn = L.arucohip_ogre_projection if ogre else L.arucohip_gl_projection
    rc = fn(_ptr(Ka), int(cam_size[0]), int(cam_size[1]), int(size[0]), int(size[1]), float(gnear), float(gfar), int(bool(invert)), _ptr(m))
    if rc:
        raise ArucoHipError(rc, "gl_projection")
    return m
