"""Metric XYZ from a disparity map on the MI355X engine: the dense map of
``cv2.reprojectImageTo3D`` and the ordered, coloured point cloud of its valid pixels.

  reproject_image_to_3d(disparity, Q)            H x W int16 x16 or float32 -> H x W x 3 float32
  point_cloud(disparity, Q, colors, min_disp=…)  -> (xyz N x 3 float32, bgr N x 3 uint8 or None[, index])
  point_cloud_dev(engine, d_disp, …)             the same on device maps, downloaded by its N
  write_ply(path, xyz, bgr)                      binary little-endian PLY (a host step)

The points keep the pixels' row-major order.  Semantics: tests/sv_cloud_oracle.py.  Argument
errors are raised before an engine is needed.
"""
from __future__ import annotations

import dataclasses

import numpy as np

from .engine import cloud_params, get_engine


@dataclasses.dataclass
class CloudParams:
    """The keyword arguments of :func:`point_cloud`: ``min_disp`` (pixels with a smaller
    disparity are left out: the ``min_disp - 1`` marker of SGBM and of the refinement stage),
    ``z_range`` (z_min, z_max; both ends kept), ``roi`` (x, y, w, h; the calibration's ``roi1``),
    ``handle_missing_values`` (the map's minimum is left out as well), ``capacity`` (points the
    outputs hold at most; None: every pixel) and ``with_index`` (also y * W + x of every point)."""
    min_disp: float = 0
    z_range: tuple | None = None
    roi: tuple | None = None
    handle_missing_values: bool = False
    capacity: int | None = None
    with_index: bool = False

    def check(self, H: int | None = None, W: int | None = None) -> "CloudParams":
        """ValueError / TypeError for what no map could be cut with (and, given a size, for a
        region outside it)."""
        md = float(self.min_disp)
        if np.isnan(md):
            raise ValueError("min_disp is NaN")
        if self.z_range is not None:
            if len(self.z_range) != 2:
                raise ValueError(f"z_range: (z_min, z_max) expected, got {self.z_range!r}")
            z0, z1 = (float(v) for v in self.z_range)
            if np.isnan(z0) or np.isnan(z1) or z0 > z1:
                raise ValueError(f"z_range: z_min <= z_max expected, got {self.z_range!r}")
        if self.roi is not None:
            if len(self.roi) != 4:
                raise ValueError(f"roi: (x, y, w, h) expected, got {self.roi!r}")
            x, y, w, h = (int(v) for v in self.roi)
            if x < 0 or y < 0 or w <= 0 or h <= 0:
                raise ValueError(f"roi {self.roi!r}: a region with a positive size at x, y >= 0 expected")
            if H is not None and (x + w > W or y + h > H):
                raise ValueError(f"roi {self.roi!r} is not inside the {W} x {H} map")
        if self.capacity is not None and int(self.capacity) < 0:
            raise ValueError(f"capacity must be >= 0, got {self.capacity}")
        return self

    def c_struct(self):
        return cloud_params(self.min_disp, self.z_range, self.roi, self.handle_missing_values)


def _check_map(disparity) -> np.ndarray:
    if not isinstance(disparity, np.ndarray):
        raise TypeError(f"disparity: a NumPy array expected, got {type(disparity).__name__}")
    if disparity.dtype not in (np.int16, np.float32):
        raise TypeError(f"disparity: int16 (x16) or float32 expected, got {disparity.dtype}")
    if disparity.ndim != 2 or disparity.size == 0:
        raise ValueError(f"disparity: an H x W map expected, got shape {disparity.shape}")
    if disparity.size >= 2 ** 31:
        raise ValueError("disparity: H * W must stay below 2^31")
    return np.ascontiguousarray(disparity)


def _check_q(Q) -> np.ndarray:
    q = np.asarray(Q)
    if q.shape != (4, 4):
        raise ValueError(f"Q: a 4 x 4 matrix expected, got shape {q.shape}")
    if not np.issubdtype(q.dtype, np.number) or np.issubdtype(q.dtype, np.complexfloating):
        raise TypeError(f"Q: a real matrix expected, got {q.dtype}")
    q = np.ascontiguousarray(q, np.float64)
    if not np.isfinite(q).all():
        raise ValueError("Q holds a non-finite entry")
    return q


def _check_colors(colors, H: int, W: int):
    if colors is None:
        return None
    if not isinstance(colors, np.ndarray) or colors.dtype != np.uint8:
        raise TypeError("colors: a uint8 array expected")
    if colors.shape != (H, W, 3):
        raise ValueError(f"colors: shape {(H, W, 3)} expected to match the map, got {colors.shape}")
    return np.ascontiguousarray(colors)


def reproject_image_to_3d(disparity, Q, handle_missing_values: bool = False, engine=None) -> np.ndarray:
    """``cv2.reprojectImageTo3D(disparity, Q, handleMissingValues, ddepth=CV_32F)`` for an int16
    x16 map (d = m / 16: what it gives on the float disparity ``create_depth_map`` returns) or a
    float32 map."""
    d, q = _check_map(disparity), _check_q(Q)
    eng = engine if engine is not None else get_engine()
    return eng.reproject_3d(d, q, bool(handle_missing_values))


def point_cloud(disparity, Q, colors=None, *, min_disp=0, z_range=None, roi=None, handle_missing_values=False,
                capacity=None, with_index=False, engine=None):
    """(xyz, bgr or None[, index]): the pixels with ``disparity >= min_disp``, finite coordinates,
    Z inside ``z_range`` and a place inside ``roi``, in row-major order; ``colors`` is the H x W x 3
    image the points take their BGR from.  With ``capacity`` below the cloud's size the first
    ``capacity`` points are returned."""
    d, q = _check_map(disparity), _check_q(Q)
    H, W = d.shape
    bgr = _check_colors(colors, H, W)
    p = CloudParams(min_disp, z_range, roi, handle_missing_values, capacity, with_index).check(H, W)
    eng = engine if engine is not None else get_engine()
    xyz, out_bgr, idx, _ = eng.point_cloud(d, q, bgr, p.c_struct(), p.capacity, p.with_index)
    return (xyz, out_bgr, idx) if with_index else (xyz, out_bgr)


def point_cloud_dev(engine, d_disp: int, fmt, H: int, W: int, Q, d_colors: int = 0, params: CloudParams | None = None,
                    *, pitch: int | None = None, colors_pitch: int | None = None, bufs=None):
    """:func:`point_cloud` on a device map (``fmt`` "i16x16" or "f32") and a device H x W x 3
    image: three launches, one 4-byte read of the cloud's size N, then the downloads of
    min(N, capacity) points.  ``bufs(name, nbytes)`` supplies the device outputs (default: the
    engine's scratch)."""
    p = (params if params is not None else CloudParams()).check(H, W)
    q = _check_q(Q)
    cap = H * W if p.capacity is None else min(int(p.capacity), H * W)
    buf = bufs if bufs is not None else (lambda name, n: engine.scratch("cloud_" + name, n))
    d_xyz = buf("xyz", 12 * cap)
    d_bgr = buf("bgr", 3 * cap) if d_colors else 0
    d_idx = buf("idx", 4 * cap) if p.with_index else 0
    n = engine.point_cloud_dev(d_disp, fmt, H, W, W if pitch is None else pitch, q, p.c_struct(), cap, d_xyz,
                               d_colors, (3 * W if colors_pitch is None else colors_pitch) if d_colors else 0,
                               d_bgr, d_idx)
    m = min(n, cap)

    def down(ptr, shape, dt):
        return engine.to_host(ptr, shape, dt) if m else np.empty(shape, dt)

    xyz = down(d_xyz, (m, 3), np.float32)
    bgr = down(d_bgr, (m, 3), np.uint8) if d_colors else None
    return (xyz, bgr, down(d_idx, (m,), np.uint32)) if p.with_index else (xyz, bgr)


def write_ply(path, xyz, bgr=None) -> None:
    """A binary little-endian PLY of the points: ``float x y z`` and, with ``bgr``, ``uchar red
    green blue``."""
    xyz = np.asarray(xyz)
    if xyz.ndim != 2 or xyz.shape[1] != 3:
        raise ValueError(f"xyz: N x 3 expected, got shape {xyz.shape}")
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    if bgr is not None:
        bgr = np.asarray(bgr)
        if bgr.shape != xyz.shape:
            raise ValueError(f"bgr: shape {xyz.shape} expected, got {bgr.shape}")
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    rec = np.empty(len(xyz), np.dtype(fields))
    for k, name in enumerate("xyz"):
        rec[name] = xyz[:, k]
    if bgr is not None:
        for k, name in enumerate(("blue", "green", "red")):
            rec[name] = bgr[:, k]
    names = {"<f4": "float", "u1": "uchar"}
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {len(xyz)}"]
    header += [f"property {names[t]} {n}" for n, t in fields] + ["end_header"]
    with open(path, "wb") as f:
        f.write(("\n".join(header) + "\n").encode("ascii"))
        f.write(rec.tobytes())
