"""Drop-in for the reference's ``fused_depth_map.py`` stereo path.

``create_depth_map_stereo_scaled(left_img, right_img, min_disp, num_disp, window_size)``
keeps the reference's name, arguments and return tuple (fused_depth_map.py:934-1041):

    (disparity_normalized float32, disparity float32, depth_colormap uint8 HxWx3,
     confidence float32)

with the print-traceback-zeros error convention (:1031-1041).  The numeric body runs in
one pass of the gfx950 kernels (``sv_stereo_scaled``).  The scaled-parameter rules of the
caller (fused_depth_map.py:2258-2266) are exposed as :func:`scaled_stereo_params`.

``fuse_depth_maps(...)`` (fused_depth_map.py:1560-1718) keeps its name, arguments, module
settings (``FUSION_*``, ``fusion_params``, read at call time) and return value as well; its
blend, Gaussian fill weight, bilateral filter, quantisation and colormap run on the GPU
(``fusion.fuse_maps``).

``process_frame(frame_left, frame_right, stereo_calib, midas)`` runs the whole frame body
(fused_depth_map.py:2483-2842) through ``frame.FusionFramePipeline``, the maps staying on the
device between the stages.

``OpticalFlowDepthEstimator`` (fused_depth_map.py:1263-1501), the producer of
``flow_depth_normalized``, is ``flow.OpticalFlowDepthEstimator``: Farneback flow, residual depth
and the bilateral filter on the GPU, the RANSAC homography on the host.

The reference calls the stereo function from a ThreadPoolExecutor worker and waits at most
0.5 s (fused_depth_map.py:2591-2598, :2671); :func:`warmup` builds the engine and runs
the scaled path once at the processing size, so the first real frame does not pay HIP
initialisation, context creation, code-object loading and staging allocation inside that
budget.  It runs at import on a background thread (``warmup_done`` is set when it has
finished); ``SV_WARMUP_AT_IMPORT=0`` disables it.
"""
from __future__ import annotations

import os
import traceback

import numpy as np

from . import colormap
from . import flow as _flow
from . import fusion as _fusion
from . import rectify as _rectify
from .fusion import (calibrate_midas_to_stereo, detect_camera_occlusion,  # noqa: F401
                     normalize_to_stereo_range)
from .engine import POST_SCALED, get_engine, start_warmup
from .flow import OpticalFlowDepthEstimator  # noqa: F401
from .preamble import ensure_same_size, to_engine_image

STEREO_CALIBRATION_FILE = "output/stereo_calibration_data.pkl"   # fused_depth_map.py:61

PROCESSING_SCALE = 0.33
MIN_DISP_BASE = 0
NUM_DISP_BASE = 16 * 20
WINDOW_SIZE_BASE = 7
COST = "sad"
# engine.RefineParams: run the refinement stage (left-right check, curvature test, sub-pixel step,
# speckle filter) between the match and the median, so that occluded and flat
# regions reach fuse_depth_maps as invalid pixels of confidence 0.  None: the plain path.
REFINE = None

# fuse_depth_maps' settings (fused_depth_map.py:81-116), read at call time
FUSION_WEIGHTS = {"stereo_base": 0.8, "midas_max_fill": 0.9, "flow_max_fill": 0.5}
FUSION_THRESHOLDS = {"stereo_low_conf": 0.5, "midas_fill_start": 0.3, "flow_hole_threshold": 15,
                     "flow_min_inliers": 15}
FUSION_SMOOTHING = {"midas_blend_radius": 15, "fusion_bilateral_d": 9, "fusion_bilateral_sigma": 75}
FUSION_METHODS = {"use_stereo": True, "use_midas_fill": True, "use_flow_fill": True}
fusion_params = {
    "stereo_weight": FUSION_WEIGHTS["stereo_base"],
    "midas_fill_weight": FUSION_WEIGHTS["midas_max_fill"],
    "flow_fill_weight": FUSION_WEIGHTS["flow_max_fill"],
    "stereo_conf_threshold": FUSION_THRESHOLDS["stereo_low_conf"],
    "flow_hole_threshold": FUSION_THRESHOLDS["flow_hole_threshold"],
}


def scaled_stereo_params(processing_scale: float = None, num_disp_base: int = None,
                         window_size_base: int = None) -> tuple[int, int]:
    """fused_depth_map.py:2258-2266: (num_disp_scaled, window_size_scaled)."""
    s = PROCESSING_SCALE if processing_scale is None else processing_scale
    nb = NUM_DISP_BASE if num_disp_base is None else num_disp_base
    wb = WINDOW_SIZE_BASE if window_size_base is None else window_size_base
    num_disp_scaled = max(16, int(nb * s) // 16 * 16)
    window_size_scaled = max(5, int(wb * s))
    if window_size_scaled % 2 == 0:
        window_size_scaled += 1
    return num_disp_scaled, window_size_scaled


def load_stereo_calibration_with_scaling(scale_factor=1.0, path=None):
    """fused_depth_map.py:307-441: camera matrices scaled by ``scale_factor``,
    stereoRectify(alpha=0, CALIB_ZERO_DISPARITY) at int(w*s) x int(h*s), maps on the GPU."""
    return _rectify.load_stereo_calibration_with_scaling(scale_factor,
                                                         path or STEREO_CALIBRATION_FILE)


def apply_stereo_rectification(left_img, right_img, stereo_calib):
    """fused_depth_map.py:444-500: resize to img_size_proc, both INTER_LINEAR remaps."""
    return _rectify.apply_stereo_rectification(left_img, right_img, stereo_calib)


def create_depth_map_stereo_scaled(left_img, right_img, min_disp, num_disp, window_size):
    """fused_depth_map.py:934-1041 on the MI355X engine."""
    left_img, right_img = ensure_same_size(left_img, right_img)
    engine = get_engine()          # raises loudly when the HIP path is unavailable
    gl = to_engine_image(left_img)
    gr = to_engine_image(right_img)
    if gl.ndim != gr.ndim:
        gl = engine.gray(gl) if gl.ndim == 3 else gl
        gr = engine.gray(gr) if gr.ndim == 3 else gr
    try:
        if REFINE is not None:   # match, refine, median, post (+ the colormap) on the device
            dn, disparity, _, confidence, depth_colormap = engine.refined_frame(
                gl, gr, int(min_disp), int(num_disp), int(window_size), REFINE, POST_SCALED, cost=COST,
                cmap_bgr=colormap.table("jet"))
            colormap.put_text(depth_colormap, f"Scale:{PROCESSING_SCALE:.2f}x Disp:{num_disp}px")
            return dn, disparity, depth_colormap, confidence
        # applyColorMap(disparity_normalized u8, JET) (:1013) runs in the same GPU epilogue
        dn, disparity, depth_colormap, confidence = engine.stereo_scaled_color(
            gl, gr, int(min_disp), int(num_disp), int(window_size), colormap.table("jet"), cost=COST)
        colormap.put_text(depth_colormap, f"Scale:{PROCESSING_SCALE:.2f}x Disp:{num_disp}px")
        return dn, disparity, depth_colormap, confidence
    except Exception as e:  # the reference's per-frame error convention (:1031-1041)
        print(f"Stereo error: {e}")
        traceback.print_exc()
        h, w = gl.shape[:2]
        empty = np.zeros((h, w), dtype=np.float32)
        empty_colormap = colormap.apply(np.zeros((h, w), dtype=np.uint8), "jet")
        return empty, empty.copy(), empty_colormap, empty.copy()


last_fuse_info = None   # fusion.fuse_maps' info of the last fuse_depth_maps call + mode_parts, mode_text


def _valid(use, m) -> bool:
    return bool(use) and m is not None and np.size(m) > 0


def fuse_settings() -> dict:
    """fusion.fuse_maps' parameters from this module's settings, read at call time."""
    fp = fusion_params
    return dict(
        stereo_weight=fp["stereo_weight"], midas_fill_weight=fp["midas_fill_weight"],
        flow_fill_weight=fp["flow_fill_weight"], stereo_conf_threshold=fp["stereo_conf_threshold"],
        flow_hole_threshold=fp["flow_hole_threshold"], use_midas_fill=FUSION_METHODS["use_midas_fill"],
        use_flow_fill=FUSION_METHODS["use_flow_fill"], midas_blend_radius=FUSION_SMOOTHING["midas_blend_radius"],
        bilateral_d=FUSION_SMOOTHING["fusion_bilateral_d"],
        bilateral_sigma=FUSION_SMOOTHING["fusion_bilateral_sigma"])


def fuse_mode(info: dict) -> dict:
    """fuse_maps' info with the mode parts (:1629, :1650, :1662, :1668, :1678, :1684) and the mode
    text: a fill is named when it changed a pixel."""
    fp = fusion_params
    mode_parts = []
    if info["base"] == _fusion.BASE_STEREO:
        mode_parts.append(f"Stereo\u00d7{fp['stereo_weight']:.1f}")
        if info["n_midas"] > 0:
            mode_parts.append(f"MiDaS_fill\u00d7{fp['midas_fill_weight']:.1f}")
    elif info["base"] == _fusion.BASE_MIDAS:
        mode_parts.append("MiDaS_base")
    else:
        mode_parts.append("Flow_base")
    if info["n_hole"] > 0:
        mode_parts.append(f"Flow_fill\u00d7{fp['flow_fill_weight']:.1f}")
    mode_text = " + ".join(mode_parts) if mode_parts else "NO DATA"
    return dict(info, mode_parts=mode_parts, mode_text=mode_text)


def annotate_fused(fused_colormap, info: dict, valid_flow: bool, camera_moving) -> None:
    """The overlays of fuse_depth_maps (:1702-1716) on the host colormap."""
    min_val, max_val = info["range"]
    w = fused_colormap.shape[1]
    colormap.put_text(fused_colormap, f"FUSED: {info['mode_text']}", (10, 30), scale=0.65)
    colormap.put_text(fused_colormap, f"Range: {min_val:.0f}-{max_val:.0f}", (10, 55), scale=0.5,
                      color=(0, 255, 255), thickness=1)
    if valid_flow:     # (camera_moving holds whenever the flow map is valid)
        motion_text = "CAM MOVING" if camera_moving else "STATIC"
        colormap.put_text(fused_colormap, motion_text, (w - 150, 30), scale=0.5,
                          color=(0, 255, 0) if camera_moving else (0, 0, 255), thickness=1)


def fuse_depth_maps(stereo_depth, stereo_conf, midas_depth_calibrated, midas_conf,
                    flow_depth_normalized, camera_moving, use_stereo=True, use_midas=True,
                    use_flow=True):
    """fused_depth_map.py:1560-1718 on the MI355X engine: (fused_uint8, fused_colormap), or
    None when no method is valid.  The blend, the Gaussian fill weight, the bilateral filter,
    the quantisation and the colormap run in two kernel launches (fusion.fuse_maps);
    ``last_fuse_info`` keeps the mode parts and the range of the last call."""
    global last_fuse_info
    valid_stereo = _valid(use_stereo, stereo_depth)
    valid_midas = _valid(use_midas, midas_depth_calibrated)
    valid_flow = _valid(use_flow, flow_depth_normalized) and bool(camera_moving)
    if not (valid_stereo or valid_midas or valid_flow):
        return None
    res = _fusion.fuse_maps(
        stereo_depth if valid_stereo else None,
        stereo_conf if valid_stereo else None,
        midas_depth_calibrated if valid_midas else None,
        flow_depth_normalized if valid_flow else None,
        cmap=colormap.table("jet"), engine=get_engine(), **fuse_settings())
    fused_uint8, fused_colormap, info = res
    info = fuse_mode(info)
    last_fuse_info = info
    annotate_fused(fused_colormap, info, valid_flow, camera_moving)
    return fused_uint8, fused_colormap


_frame_pipelines: dict = {}      # id(calibration) -> (calibration, FusionFramePipeline)


def process_frame(frame_left, frame_right, stereo_calib=None, midas=None, **pipeline_args):
    """One iteration of the frame loop (fused_depth_map.py:2483-2842) with every map resident on
    the device: ``frame.FusionFramePipeline.step`` on a pipeline kept per calibration object
    (``pipeline_args`` configure it when it is first made).  Returns the step's FrameResult."""
    from .frame import FusionFramePipeline
    entry = _frame_pipelines.get(id(stereo_calib))
    if entry is None or entry[0] is not stereo_calib:
        if entry is not None:
            entry[1].close()
        entry = (stereo_calib, FusionFramePipeline(stereo_calib, **pipeline_args))
        _frame_pipelines[id(stereo_calib)] = entry
    return entry[1].step(frame_left, frame_right, midas)


def frame_pipeline(stereo_calib=None):
    """The pipeline process_frame keeps for ``stereo_calib`` (None before its first frame): its
    ``use_stereo`` / ``use_midas`` / ``use_flow`` / ``show_fused`` switches are the loop's USE_*."""
    entry = _frame_pipelines.get(id(stereo_calib))
    return entry[1] if entry is not None and entry[0] is stereo_calib else None


def warmup(height: int = 356, width: int = 633, processing_scale: float = None) -> None:
    """Create the engine and run the scaled path once at the processing size
    (default: 1920x1080 at PROCESSING_SCALE 0.33 -> 633x356, D=96, window 5), BGR frames as
    the camera delivers them."""
    nd, ws = scaled_stereo_params(processing_scale)
    z = np.zeros((height, width, 3), np.uint8)
    eng = get_engine()
    eng.stereo_scaled_color(z, z, MIN_DISP_BASE, nd, ws, colormap.table("jet"), cost=COST)
    # one optical-flow step, so the estimator's first pair does not load the flow kernels' code
    # objects and allocate their scratch inside the caller's budget
    if height >= 16 and width >= 16:
        _flow.farneback_flow(z[..., 0], z[..., 0], *_flow.OpticalFlowDepthEstimator.FLOW_ARGS, engine=eng)


warmup_done = None
if os.environ.get("SV_WARMUP_AT_IMPORT", "1") != "0":
    warmup_done = start_warmup(warmup, "sv-warmup-fused")
