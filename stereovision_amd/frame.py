"""The frame body of the reference's ``fused_depth_map.py`` loop (:2483-2842) with every map
resident in device memory: one upload per camera frame, downloads only of what the caller asks for.

``FusionFramePipeline.step(frame_left, frame_right, midas=None)`` restates one iteration, in the
reference's order and with its decisions:

  processing frames (:2483-2507)   resize + both remaps, or the plain resize; BGR and gray stay in HBM
  occlusion + hysteresis (:2515-2571)   ``k_frame_stats`` on the processed pair, :class:`OcclusionSwitch`
  source frame (:2614-2642)        the right camera while the left one is covered
  stereo (:2587-2598, :2667-2708)  the scaled path on the device gray pair
  flow (:2637-2648)                ``OpticalFlowDepthEstimator.step_dev`` on the device gray frame
  MiDaS branch (:2719-2774)        the caller's map, calibrated to the stereo maps or min-max normalised
  flow normalisation (:2793-2811)  one elementwise pass (``k_affine_f32`` modes 3 and 4)
  fuse (:2822-2842)                ``fusion.fuse_maps_dev`` under fuse_depth_maps' validity rules
  cloud (not in the reference)     opt-in: ``cloud.point_cloud_dev`` on the stereo disparity and the left frame

UI, capture, frame skipping, the keyboard handlers and the legends are not part of it, and MiDaS
is a map the caller supplies: the process stays torch-free.  Everything is enqueued on the
engine's context stream.  What still crosses to the host per frame is listed in DESIGN.md §5h.
"""
from __future__ import annotations

import dataclasses
import traceback

import numpy as np

from . import cloud as _cloud
from . import colormap
from . import flow as _flow
from . import fusion as _fusion
from . import rectify as _rectify
from .engine import POST_SCALED, STAGE_ALL, EngineUnavailable, get_engine, map_out

OUTPUT_NAMES = ("fused_u8", "fused_colormap", "stereo_depth", "stereo_disparity", "stereo_conf",
                "stereo_colormap", "flow_depth_raw", "flow_depth_normalized", "midas_calibrated",
                "processed_left", "processed_right")
DEFAULT_PROC_SIZE = (640, 480)      # fused_depth_map.py:2495 without a calibration


class OcclusionSwitch:
    """The hysteresis and the automatic stereo switch of fused_depth_map.py:2515-2571 in plain
    Python: ``state`` changes only after ``hysteresis_frames`` consecutive checks that disagree
    with it; 'left' / 'right' switch ``use_stereo`` off, 'none' / 'both' switch it back on.  The
    check is due when ``frame_counter % check_interval == 0``; ``tick`` ends a frame."""

    def __init__(self, check_interval: int = 2, hysteresis_frames: int = 5, use_stereo: bool = True):
        self.check_interval = int(check_interval)
        self.hysteresis_frames = int(hysteresis_frames)
        self.use_stereo = bool(use_stereo)
        self.state = "none"
        self.counter = 0
        self.frame_counter = 0

    def due(self) -> bool:
        return self.frame_counter % self.check_interval == 0

    def update(self, new_state: str) -> bool:
        """One check's result; True when the state changed."""
        if new_state == self.state:
            self.counter = 0
            return False
        self.counter += 1
        if self.counter < self.hysteresis_frames:
            return False
        self.state = new_state
        self.counter = 0
        if self.state in ("left", "right"):
            if self.use_stereo:
                print(f"\n[WARNING] {self.state.upper()} camera covered: stereo switched off, "
                      f"{'right' if self.state == 'left' else 'left'} camera + MiDaS + optical flow")
                self.use_stereo = False
        elif self.state in ("none", "both"):
            if not self.use_stereo:
                print("\n[INFO] view restored: stereo switched on" if self.state == "none" else
                      "\n[INFO] both cameras covered: stereo switched on all the same")
                self.use_stereo = True
        return True

    def tick(self) -> None:
        self.frame_counter += 1


class FrameResult:
    """One step's scalars, the host arrays of the requested outputs (attributes named as in
    OUTPUT_NAMES; None when the map does not exist this frame) and the device maps.  ``cloud``:
    the frame's point cloud, (xyz, bgr[, index]) as cloud.point_cloud returns it, for a pipeline
    built with ``cloud=``; None when stereo did not run this frame or the calibration has no Q."""

    def __init__(self):
        self.occlusion_state = "none"
        self.left_score = 0.0
        self.right_score = 0.0
        self.camera_moving = False
        self.use_stereo = True
        self.mode_text = None
        self.range = None
        self.source = "left"
        self.cloud = None
        self._dev = {}
        for name in OUTPUT_NAMES:
            setattr(self, name, None)

    def device(self, name: str):
        """(device pointer, shape, dtype) of the map ``name``, valid until the pipeline's next
        step; None when the map does not exist this frame.  The zero stereo maps of a frame
        without stereo exist on the device only when they were requested as outputs, and the
        colormaps carry no text."""
        if name not in OUTPUT_NAMES:
            raise ValueError(f"unknown map {name!r}; expected one of {OUTPUT_NAMES}")
        return self._dev.get(name)


def calib_q(calib):
    """The calibration's disparity-to-3D matrix, or None when it has none."""
    if calib is None or "Q" not in calib or calib["Q"] is None:
        return None
    return calib["Q"]


def _log(stage: str, e: Exception) -> None:
    print(f"[{stage} error] {e}")
    traceback.print_exc()


class FusionFramePipeline:
    """fused_depth_map.py:2483-2842 on the MI355X engine (see the module text)."""

    def __init__(self, stereo_calib=None, *, use_rectify=True, min_disp=None, num_disp=None,
                 window_size=None, cost=None, engine=None, outputs=("fused_u8", "fused_colormap"),
                 occlusion_check_interval=2, occlusion_hysteresis_frames=5, occlusion_threshold=0.45,
                 min_inliers=15, motion_timeout=1.5, refine=None, cloud=None):
        outputs = tuple(outputs)
        unknown = [n for n in outputs if n not in OUTPUT_NAMES]
        if unknown:
            raise ValueError(f"unknown outputs {unknown}; expected names from {OUTPUT_NAMES}")
        if int(occlusion_check_interval) < 1 or int(occlusion_hysteresis_frames) < 1:
            raise ValueError("occlusion_check_interval and occlusion_hysteresis_frames must be >= 1")
        self.stereo_calib = stereo_calib
        self.use_rectify = bool(use_rectify)
        self.min_disp, self.num_disp, self.window_size, self.cost = min_disp, num_disp, window_size, cost
        self.refine = refine        # engine.RefineParams; None: fused_depth_map.REFINE at each step
        if cloud is not None:
            if not isinstance(cloud, _cloud.CloudParams):
                raise TypeError(f"cloud: CloudParams expected, got {type(cloud).__name__}")
            cloud.check()
        self.cloud = cloud          # cloud.CloudParams; None: no point cloud (min_disp: the stereo step's)
        self.outputs = outputs
        self.occlusion_threshold = occlusion_threshold
        self.use_midas = True
        self.use_flow = True
        self.show_fused = True
        self.left_score = 0.0
        self.right_score = 0.0
        self._switch = OcclusionSwitch(occlusion_check_interval, occlusion_hysteresis_frames)
        self._eng = engine
        self._est_args = (min_inliers, motion_timeout)
        self._est = None
        self._bufs = {}
        self._rect = None           # (calibration maps' ids, StereoRectifier) on another engine than the default
        self._parity = 0

    # -- the reference's loop variables ---------------------------------------------------
    @property
    def use_stereo(self) -> bool:
        return self._switch.use_stereo

    @use_stereo.setter
    def use_stereo(self, value):
        self._switch.use_stereo = bool(value)

    @property
    def occlusion_state(self) -> str:
        return self._switch.state

    @property
    def frame_counter(self) -> int:
        return self._switch.frame_counter

    @property
    def camera_moving(self) -> bool:
        return bool(self._est.camera_moving) if self._est is not None else False

    # -- buffers ----------------------------------------------------------------------------
    def _buf(self, name: str, nbytes: int) -> int:
        p, cap = self._bufs.get(name, (0, 0))
        if cap < nbytes:
            if p:
                self._eng.dev_free(p)
                self._bufs.pop(name)
            p = self._eng.dev_alloc(max(int(nbytes), 256))
            self._bufs[name] = (p, max(int(nbytes), 256))
        return p

    def close(self):
        eng, bufs = self._eng, self._bufs
        self._bufs = {}
        for p, _ in bufs.values():
            try:
                eng.dev_free(p)
            except Exception:
                pass
        if self._est is not None:
            self._est._free()
            self._est = None
        if self._rect is not None:
            self._rect[1].close()
            self._rect = None

    def __del__(self):  # pragma: no cover - best effort
        try:
            if getattr(self._eng, "handle", None):
                self.close()
        except Exception:
            pass

    # -- inputs -------------------------------------------------------------------------------
    @staticmethod
    def check_inputs(frame_left, frame_right, midas=None):
        """The step's arguments as contiguous arrays: (left, right, midas_raw or None).  Camera
        frames: uint8 (TypeError) H x W x 3 of one shape (ValueError).  midas: a float32 H x W
        map or (map, confidence), either None; its size is free (the calibration resizes it,
        :1215)."""
        frames = []
        for name, f in (("frame_left", frame_left), ("frame_right", frame_right)):
            if not isinstance(f, np.ndarray):
                raise TypeError(f"{name}: a NumPy array expected, got {type(f).__name__}")
            if f.dtype != np.uint8:
                raise TypeError(f"{name}: uint8 expected, got {f.dtype}")
            if f.ndim != 3 or f.shape[2] != 3 or f.shape[0] == 0 or f.shape[1] == 0:
                raise ValueError(f"{name}: a BGR H x W x 3 frame expected, got shape {f.shape}")
            frames.append(np.ascontiguousarray(f))
        if frames[0].shape != frames[1].shape:
            raise ValueError(f"camera frames differ in shape: {frames[0].shape} and {frames[1].shape}")
        raw = None
        if midas is not None:
            raw, conf = midas if isinstance(midas, (tuple, list)) else (midas, None)
            if isinstance(midas, (tuple, list)) and len(midas) != 2:
                raise ValueError("midas: (midas_raw, midas_conf) expected")
            for name, m in (("midas_raw", raw), ("midas_conf", conf)):
                if m is None:
                    continue
                if not isinstance(m, np.ndarray) or m.dtype != np.float32:
                    raise TypeError(f"{name}: a float32 array expected")
                if m.ndim != 2 or m.size == 0:
                    raise ValueError(f"{name}: an H x W map expected, got shape {m.shape}")
            if raw is not None:
                raw = np.ascontiguousarray(raw)
        return frames[0], frames[1], raw

    def _stereo_settings(self):
        from . import fused_depth_map as FDM
        nd, ws = FDM.scaled_stereo_params()
        return (int(FDM.MIN_DISP_BASE if self.min_disp is None else self.min_disp),
                int(nd if self.num_disp is None else self.num_disp),
                int(ws if self.window_size is None else self.window_size),
                FDM.COST if self.cost is None else self.cost, FDM.PROCESSING_SCALE)

    # -- stages -------------------------------------------------------------------------------
    def _rectifier(self, calib):
        rect = _rectify._rectifier_for(calib)
        if rect.engine is self._eng:
            return rect
        keys = ("left_map1", "left_map2", "right_map1", "right_map2")
        ids = tuple(id(calib[k]) for k in keys)
        if self._rect is None or self._rect[0] != ids:
            if self._rect is not None:
                self._rect[1].close()
            self._rect = (ids, _rectify.StereoRectifier.from_maps(*(calib[k] for k in keys), engine=self._eng))
        return self._rect[1]

    def _upload(self, name, frame):
        d = self._buf(name, frame.nbytes)
        self._eng.to_device(d, frame)
        return d

    def _process(self, fl, fr):
        """:2483-2507 -> (d_left, d_right, H, W): the processed BGR pair in device memory."""
        eng, calib = self._eng, self.stereo_calib
        sH, sW = fl.shape[:2]
        cur = [self._upload("cam_l", fl), self._upload("cam_r", fr)]       # each camera frame once
        if self.use_rectify and calib is not None:
            try:                                                            # apply_stereo_rectification
                tw, th = calib["img_size_proc"] if "img_size_proc" in calib else calib["img_size"]
                tw, th = int(tw), int(th)
                rect = self._rectifier(calib)
                m1l, m2l, m1r, m2r, H, W = rect.device_maps
                src, (rH, rW) = list(cur), (sH, sW)
                if (sW, sH) != (tw, th):
                    for k, name in enumerate(("rs_l", "rs_r")):
                        d = self._buf(name, th * tw * 3)
                        eng.resize_dev(src[k], sH, sW, 3, sW * 3, d, th, tw, tw * 3)
                        src[k] = d
                    rH, rW = th, tw
                out = [self._buf("proc_l", H * W * 3), self._buf("proc_r", H * W * 3)]
                eng.remap_dev(src[0], rH, rW, 3, rW * 3, m1l, m2l, H, W, out[0], W * 3)
                eng.remap_dev(src[1], rH, rW, 3, rW * 3, m1r, m2r, H, W, out[1], W * 3)
                return out[0], out[1], H, W
            except EngineUnavailable:
                raise
            except Exception as e:                                          # :496-500: the frames as they came
                _log("Stereo rectification", e)
                return cur[0], cur[1], sH, sW
        if calib is not None:
            pw, ph = calib["img_size_proc"] if "img_size_proc" in calib else calib["img_size"]
        else:
            pw, ph = DEFAULT_PROC_SIZE
        pw, ph = int(pw), int(ph)
        if (sW, sH) != (pw, ph):
            for k, name in enumerate(("proc_l", "proc_r")):
                d = self._buf(name, ph * pw * 3)
                eng.resize_dev(cur[k], sH, sW, 3, sW * 3, d, ph, pw, pw * 3)
                cur[k] = d
        return cur[0], cur[1], ph, pw

    def _check_occlusion(self, d_l, d_r, H, W):
        """detect_camera_occlusion (:2518-2522) on the processed device pair + the hysteresis."""
        eng = self._eng
        bh, bw = max(1, H // 48), max(1, W // 48)
        nb = bh * bw
        d = self._buf("stats", (4 * nb + 512) * 4)
        eng.frame_stats_dev(d_l, d_r, H, W, 3, W * 3, d, d + 2 * nb * 4, d + 4 * nb * 4)
        st = eng.to_host(d, (4 * nb + 512,), np.uint32)
        bs, bq, hist = st[:2 * nb].reshape(2, bh, bw), st[2 * nb:4 * nb].reshape(2, bh, bw), st[4 * nb:].reshape(2, 256)
        mets = [_fusion.occlusion_metrics(bs[k], bq[k], hist[k], H, W) for k in range(2)]
        new_state, self.left_score, self.right_score = _fusion.occlusion_decision(mets[0], mets[1],
                                                                                   self.occlusion_threshold)
        self._switch.update(new_state)

    def _minmax(self, d_x, n):
        """(np.min, np.max) of a float32 device map from order statistics 0 and n - 1."""
        sel, nans = self._eng.select_count(d_x, n)
        if nans or sel == 0:
            return np.float32(np.nan), np.float32(np.nan)
        mn, mx = self._eng.select_ranks(d_x, n, [0, n - 1])
        return np.float32(mn), np.float32(mx)

    def _midas(self, raw, stereo, H, W):
        """:2730-2774 -> (device pointer, (h, w)) of midas_depth_calibrated."""
        eng = self._eng
        mH, mW = raw.shape
        d_raw = self._upload("midas_raw", raw)
        if stereo is not None:                                   # calibrate_midas_to_stereo
            oh, ow = H, W
            d_cal = self._buf("midas_cal", 4 * H * W)
            _fusion.calibrate_midas_to_stereo_dev(eng, d_raw, mH, mW, stereo["stereo_depth"], stereo["stereo_conf"],
                                                  H, W, d_cal, self._buf("midas_rs", 4 * H * W))
            mn, mx = self._minmax(d_cal, oh * ow)
        else:                                                    # :2749-2759, at the map's own size
            oh, ow = mH, mW
            d_cal = self._buf("midas_cal", 4 * mH * mW)
            _fusion.minmax_normalize_dev(eng, d_raw, mH * mW, d_cal)
            # the normalised map lies in [0, 255]: the clipped range of a radius-0 pass is its range
            mn, mx = eng.bilateral_f32_dev(d_cal, oh, ow, 0, None, None, 0.0, minmax=True)
        if mx > 10.0:                                            # :2766-2774 (a NaN maximum: no filter)
            d_out = self._buf("midas_smooth", 4 * oh * ow)
            _fusion.bilateral_filter_dev(eng, d_cal, oh, ow, mn, mx, 5, 50, 50, d_out)
            d_cal = d_out
        return d_cal, (oh, ow)

    def _stereo(self, d_gl, d_gr, H, W, want_colormap, settings):
        """create_depth_map_stereo_scaled's numeric body on the device gray pair."""
        eng, n = self._eng, H * W
        min_disp, num_disp, win, cost, _ = settings
        m = {"stereo_depth": self._buf("st_depth", 4 * n), "stereo_disparity": self._buf("st_disp", 4 * n),
             "stereo_conf": self._buf("st_conf", 4 * n)}
        d_u8 = self._buf("st_u8", n)
        d_bgr = self._buf("st_bgr", 3 * n) if want_colormap else 0
        try:
            out = map_out(POST_SCALED, m["stereo_disparity"], m["stereo_depth"], d_u8, m["stereo_conf"], bgr=d_bgr,
                          cmap=colormap.table("jet") if d_bgr else None)
            from . import fused_depth_map as FDM
            refine = FDM.REFINE if self.refine is None else self.refine
            if refine is not None:   # match, refine, then the median over the checked, full table
                d16 = self._buf("st_d16", 2 * n)
                eng.disparity_refined_dev(d_gl, d_gr, H, W, W, min_disp, num_disp, win, cost, refine, d16, W)
                eng.median_rows_dev(d16, H, W, 0, H, out, min_disp, num_disp, "sgbm")
            else:
                eng.depth_map_batch_ex(d_gl, d_gr, 1, H, W, W, H * W, min_disp, num_disp, win, cost, STAGE_ALL, 0,
                                       out)
            ok = True
        except EngineUnavailable:
            raise
        except Exception as e:                                   # :2678-2695: zero maps
            _log("Stereo", e)
            self._zero_stereo(m, d_bgr, H, W)
            ok = False
        if d_bgr:
            m["stereo_colormap"] = d_bgr
        return m, ok

    def _zero_stereo(self, m, d_bgr, H, W):
        for k in ("stereo_depth", "stereo_disparity", "stereo_conf"):
            self._eng.affine_f32_dev(m[k], H * W, _fusion.AFF_FILL, m[k], fc=0.0)
        if d_bgr:
            self._eng.to_device(d_bgr, colormap.apply(np.zeros((H, W), np.uint8), "jet"))

    # -- the step -------------------------------------------------------------------------------
    def step(self, frame_left, frame_right, midas=None) -> FrameResult:
        fl, fr, midas_raw = self.check_inputs(frame_left, frame_right, midas)
        if self._eng is None:
            self._eng = get_engine()          # EngineUnavailable when the HIP path cannot run
        eng, sw, want = self._eng, self._switch, set(self.outputs)
        res = FrameResult()
        dev, shapes = res._dev, {}

        d_l, d_r, H, W = self._process(fl, fr)                                        # 1
        n = H * W
        if sw.due():                                                                    # 2
            try:
                self._check_occlusion(d_l, d_r, H, W)
            except EngineUnavailable:
                raise
            except Exception as e:
                _log("Occlusion check", e)
        use_stereo = sw.use_stereo
        source = "right" if sw.state == "left" else "left"                            # 3
        settings = self._stereo_settings()

        # the gray frames.  The flow's source frame goes into one of two buffers that only the
        # frames given to the estimator take turns in: its previous frame stays as it was, however
        # many frames pass with the flow switched off
        d_gl = d_gr = 0
        if self.use_flow:
            self._parity ^= 1
            d_src = self._buf(f"flow_gray{self._parity}", n)
            eng.gray_dev(d_r if source == "right" else d_l, H, W, W * 3, d_src)
            if source == "right":
                d_gr = d_src
            else:
                d_gl = d_src
        if use_stereo:
            if not d_gl:
                d_gl = self._buf("gray_l", n)
                eng.gray_dev(d_l, H, W, W * 3, d_gl)
            if not d_gr:
                d_gr = self._buf("gray_r", n)
                eng.gray_dev(d_r, H, W, W * 3, d_gr)

        stereo, stereo_ok = None, False                                                # 4
        if use_stereo:
            stereo, stereo_ok = self._stereo(d_gl, d_gr, H, W, "stereo_colormap" in want, settings)
        else:   # the reference's zero maps (:2697-2708), on the device only when asked for
            asked = want & {"stereo_depth", "stereo_disparity", "stereo_conf", "stereo_colormap"}
            if asked:
                z = {k: self._buf(b, 4 * n) for k, b in (("stereo_depth", "st_depth"), ("stereo_disparity", "st_disp"),
                                                         ("stereo_conf", "st_conf"))}
                d_bgr = self._buf("st_bgr", 3 * n) if "stereo_colormap" in asked else 0
                self._zero_stereo(z, d_bgr, H, W)
                if d_bgr:
                    z["stereo_colormap"] = d_bgr
                for k in asked:
                    dev[k] = z[k]
        if stereo is not None:
            dev.update(stereo)

        d_flow = None                                                                  # 5
        camera_moving = False
        if self.use_flow:
            if self._est is None:
                self._est = _flow.OpticalFlowDepthEstimator(*self._est_args, engine=eng)
            d_flow = self._est.step_dev(d_gl if source == "left" else d_gr, H, W)
            camera_moving = self._est.camera_moving
            if d_flow is not None:
                dev["flow_depth_raw"] = d_flow

        d_midas, midas_shape = None, None                                              # 6
        if midas_raw is not None and self.use_midas:
            try:
                d_midas, midas_shape = self._midas(midas_raw, stereo, H, W)
                dev["midas_calibrated"] = d_midas
                shapes["midas_calibrated"] = midas_shape
            except EngineUnavailable:
                raise
            except Exception as e:                                                     # :2776-2783: no MiDaS map
                _log("MiDaS", e)
                d_midas = None

        d_fnorm = None                                                                 # 7
        if d_flow is not None:
            try:
                d_fnorm = self._buf("flow_norm", 4 * n)
                _fusion.flow_normalize_dev(eng, d_flow, n, stereo["stereo_disparity"] if stereo is not None else 0,
                                           d_fnorm)
                dev["flow_depth_normalized"] = d_fnorm
            except EngineUnavailable:
                raise
            except Exception as e:
                _log("Flow normalisation", e)
                d_fnorm = None

        info, valid_flow = None, False                                                 # 8
        if self.show_fused:
            valid_midas = d_midas is not None
            valid_flow = self.use_flow and d_fnorm is not None and bool(camera_moving)
            if stereo is not None or valid_midas or valid_flow:
                try:
                    info = self._fuse(stereo, d_midas if valid_midas else 0, midas_shape,
                                      d_fnorm if valid_flow else 0, H, W, "fused_colormap" in want, dev)
                except EngineUnavailable:
                    raise
                except Exception as e:
                    _log("Fusion", e)
                    info = None
                    dev.pop("fused_u8", None)
                    dev.pop("fused_colormap", None)

        if self.cloud is not None and stereo_ok and calib_q(self.stereo_calib) is not None:   # 9
            try:
                res.cloud = _cloud.point_cloud_dev(
                    eng, stereo["stereo_disparity"], "f32", H, W, calib_q(self.stereo_calib), d_l,
                    dataclasses.replace(self.cloud, min_disp=settings[0]),
                    bufs=lambda name, nbytes: self._buf("cloud_" + name, nbytes))
            except EngineUnavailable:
                raise
            except Exception as e:
                _log("Point cloud", e)
                res.cloud = None

        # the scalars, then the requested maps
        res.occlusion_state, res.left_score, res.right_score = sw.state, self.left_score, self.right_score
        res.camera_moving, res.use_stereo, res.source = bool(camera_moving), use_stereo, source
        if info is not None:
            res.mode_text, res.range = info["mode_text"], info["range"]
        dev["processed_left"], dev["processed_right"] = d_l, d_r
        dtypes = {"fused_u8": np.uint8}
        for name in list(dev):
            if name in ("processed_left", "processed_right", "stereo_colormap", "fused_colormap"):
                shape, dt = (H, W, 3), np.uint8
            else:
                shape, dt = shapes.get(name, (H, W)), dtypes.get(name, np.float32)
            dev[name] = (dev[name], shape, dt)
        for name in self.outputs:
            if name in dev:
                setattr(res, name, eng.to_host(*dev[name]))
        if res.stereo_colormap is not None and stereo_ok:       # create_depth_map_stereo_scaled's overlay
            colormap.put_text(res.stereo_colormap, f"Scale:{settings[4]:.2f}x Disp:{settings[1]}px")
        if res.fused_colormap is not None:
            from . import fused_depth_map as FDM
            FDM.annotate_fused(res.fused_colormap, info, valid_flow, camera_moving)
        sw.tick()
        return res

    def _fuse(self, stereo, d_midas, midas_shape, d_fnorm, H, W, want_colormap, dev):
        """fuse_depth_maps' numeric body (:1603-1700) on the device maps, its module settings."""
        from . import fused_depth_map as FDM
        if d_midas and midas_shape != (H, W):
            raise ValueError(f"fuse_maps: midas has shape {midas_shape}, expected {(H, W)}")
        n = H * W
        d_u8 = self._buf("fused_u8", n)
        d_bgr = self._buf("fused_bgr", 3 * n) if want_colormap else 0
        info = _fusion.fuse_maps_dev(
            self._eng, H, W, stereo["stereo_depth"] if stereo is not None else 0,
            stereo["stereo_conf"] if stereo is not None else 0, d_midas, d_fnorm, self._buf("fused_f32", 4 * n),
            d_u8, d_bgr, colormap.table("jet") if d_bgr else None, **FDM.fuse_settings())
        info = FDM.fuse_mode(info)
        dev["fused_u8"] = d_u8
        if d_bgr:
            dev["fused_colormap"] = d_bgr
        return info
