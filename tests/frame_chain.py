"""The frame body of the reference's loop (fused_depth_map.py:2483-2842) as the chain of the
host-array drop-ins, each of which is oracle-tested on its own: what FusionFramePipeline is held
equal to (test_frame_gpu.py) and measured against (tools/frame_rate.py).  Also the literal
transcription of the loop's hysteresis (:2515-2571) and moving stereo scenes for both."""
import numpy as np

import flow_scenes as S
from stereovision_amd import fused_depth_map as FDM
from stereovision_amd import fusion, preamble
from stereovision_amd.flow import OpticalFlowDepthEstimator


class LoopTranscription:
    """fused_depth_map.py:2325-2359 and :2515-2571, statement by statement (the prints left out).
    frame_counter is tested before its increment, so the first frame is checked."""

    def __init__(self):
        self.occlusion_state = 'none'
        self.occlusion_hysteresis_counter = 0
        self.OCCLUSION_HYSTERESIS_FRAMES = 5
        self.OCCLUSION_CHECK_INTERVAL = 2
        self.frame_counter = 0
        self.USE_STEREO = True
        self.checked = 0

    def check_due(self):
        return self.frame_counter % self.OCCLUSION_CHECK_INTERVAL == 0

    def check(self, new_occlusion_state):
        self.checked += 1
        if new_occlusion_state == self.occlusion_state:
            self.occlusion_hysteresis_counter = 0
        else:
            self.occlusion_hysteresis_counter += 1
            if self.occlusion_hysteresis_counter >= self.OCCLUSION_HYSTERESIS_FRAMES:
                self.occlusion_state = new_occlusion_state
                self.occlusion_hysteresis_counter = 0
                if self.occlusion_state in ['left', 'right']:
                    if self.USE_STEREO:
                        self.USE_STEREO = False
                elif self.occlusion_state in ['none', 'both']:
                    if not self.USE_STEREO:
                        self.USE_STEREO = True

    def frame(self, detected):
        if self.check_due():
            self.check(detected)
        self.frame_counter += 1


class HostChain:
    """One loop iteration per step() on host arrays, through the drop-ins of
    stereovision_amd.fused_depth_map, with the reference's statements around them."""

    def __init__(self, stereo_calib=None, use_rectify=True, min_disp=0, num_disp=32, window_size=5):
        self.stereo_calib, self.use_rectify = stereo_calib, use_rectify
        self.min_disp, self.num_disp, self.window_size = min_disp, num_disp, window_size
        self.loop = LoopTranscription()
        self.USE_MIDAS = self.USE_OPTICAL_FLOW = self.show_fused_depth = True
        self.left_score = self.right_score = 0.0
        self.flow_estimator = OpticalFlowDepthEstimator(min_inliers=15, motion_timeout=1.5)

    def step(self, frame_left, frame_right, midas=None):
        L, stereo_calib = self.loop, self.stereo_calib
        if self.use_rectify and stereo_calib is not None:                       # :2483-2507
            processed_left, processed_right = FDM.apply_stereo_rectification(frame_left, frame_right, stereo_calib)
        else:
            proc_w, proc_h = stereo_calib['img_size_proc'] if stereo_calib else (640, 480)
            processed_left = preamble.resize_linear(frame_left, proc_w, proc_h)
            processed_right = preamble.resize_linear(frame_right, proc_w, proc_h)
        if L.check_due():                                                       # :2515-2571
            new_state, self.left_score, self.right_score = FDM.detect_camera_occlusion(
                processed_left, processed_right, occlusion_threshold=0.45)
            L.check(new_state)
        USE_STEREO = L.USE_STEREO
        source = 'right' if L.occlusion_state == 'left' else 'left'            # :2614-2642
        source_frame = processed_right if source == 'right' else processed_left
        flow_depth_raw, camera_moving = None, False
        if self.USE_OPTICAL_FLOW:                                               # :2637-2648
            flow_depth_raw = self.flow_estimator(source_frame)
            camera_moving = self.flow_estimator.camera_moving
        h, w = processed_left.shape[:2]
        if USE_STEREO:                                                          # :2667-2708
            stereo_depth, stereo_disparity_raw, stereo_colormap, stereo_conf = FDM.create_depth_map_stereo_scaled(
                processed_left.copy(), processed_right.copy(), self.min_disp, self.num_disp, self.window_size)
        else:
            stereo_depth = np.zeros((h, w), dtype=np.float32)
            stereo_disparity_raw = np.zeros((h, w), dtype=np.float32)
            stereo_colormap = FDM.colormap.apply(np.zeros((h, w), dtype=np.uint8), "jet")
            stereo_conf = np.zeros((h, w), dtype=np.float32)
        midas_depth_calibrated = midas_conf = None                              # :2719-2774
        if midas is not None and self.USE_MIDAS:
            midas_raw, midas_conf = midas if isinstance(midas, tuple) else (midas, None)
            if midas_raw is not None:
                if USE_STEREO and stereo_depth is not None and stereo_conf is not None:
                    midas_depth_calibrated = FDM.calibrate_midas_to_stereo(midas_raw, stereo_depth, stereo_conf)
                else:
                    min_val = np.min(midas_raw)
                    max_val = np.max(midas_raw)
                    if max_val > min_val + 1e-6:
                        midas_normalized = (midas_raw - min_val) / (max_val - min_val + 1e-8)
                    else:
                        midas_normalized = np.zeros_like(midas_raw)
                    midas_depth_calibrated = np.clip(midas_normalized * 255.0, 0, 255).astype(np.float32)
                if midas_depth_calibrated is not None and np.max(midas_depth_calibrated) > 10.0:
                    midas_depth_calibrated = fusion.bilateral_filter(midas_depth_calibrated.astype(np.float32),
                                                                     5, 50, 50)
        flow_depth_normalized = None                                            # :2793-2811
        if flow_depth_raw is not None:
            if USE_STEREO and stereo_disparity_raw is not None:
                flow_depth_normalized = FDM.normalize_to_stereo_range(flow_depth_raw, stereo_disparity_raw)
                if flow_depth_normalized is not None:
                    flow_depth_normalized = 255.0 - flow_depth_normalized
            else:
                flow_depth_normalized = np.clip(flow_depth_raw * 255.0, 0, 255).astype(np.float32)
                flow_depth_normalized = 255.0 - flow_depth_normalized
        fused_u8 = fused_colormap = mode_text = rng = None                      # :2822-2842
        if self.show_fused_depth:
            fused_result = FDM.fuse_depth_maps(stereo_depth, stereo_conf, midas_depth_calibrated, midas_conf,
                                               flow_depth_normalized, camera_moving, use_stereo=USE_STEREO,
                                               use_midas=self.USE_MIDAS, use_flow=self.USE_OPTICAL_FLOW)
            if fused_result is not None:
                fused_u8, fused_colormap = fused_result
                mode_text, rng = FDM.last_fuse_info["mode_text"], FDM.last_fuse_info["range"]
        L.frame_counter += 1
        return {"occlusion_state": L.occlusion_state, "left_score": self.left_score, "right_score": self.right_score,
                "camera_moving": camera_moving, "use_stereo": USE_STEREO, "mode_text": mode_text, "range": rng,
                "source": source, "fused_u8": fused_u8, "fused_colormap": fused_colormap,
                "stereo_depth": stereo_depth, "stereo_disparity": stereo_disparity_raw, "stereo_conf": stereo_conf,
                "stereo_colormap": stereo_colormap, "flow_depth_raw": flow_depth_raw,
                "flow_depth_normalized": flow_depth_normalized, "midas_calibrated": midas_depth_calibrated,
                "processed_left": processed_left, "processed_right": processed_right}


SCALARS = ("occlusion_state", "left_score", "right_score", "camera_moving", "use_stereo", "mode_text", "range",
           "source")


def moving_stereo_sequence(H, W, frames, disparity=8, step=(1.5, 0.75), seed=7):
    """[(left BGR, right BGR)] of a camera that translates by `step` pixels per frame over a
    smooth texture; right(x, y) = left(x + disparity, y).  NumPy only."""
    pad = int(np.ceil(max(abs(step[0]), abs(step[1])) * frames)) + disparity + 4
    t = S.smooth_texture(H, W, seed, pad)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    out = []
    for k in range(frames):
        left = S._u8(S._sample(t, ys + pad - k * step[1], xs + pad - k * step[0]))
        right = S._u8(S._sample(t, ys + pad - k * step[1], xs + pad - k * step[0] + disparity))
        out.append((S.to_bgr(left), S.to_bgr(right)))
    return out
