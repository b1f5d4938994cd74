"""stereovision_amd — MI355X-native (gfx950) stereo-disparity engine.

A drop-in for the disparity hot path of AlexGr5/StereoVision's ``depth_map.py`` and
``fused_depth_map.py``: the same Python entry points, computed by hand-written HIP kernels
through a C ABI (``include/stereovision_amd.h``, ``lib/libsvhip.so``).  See DESIGN.md.
"""
from .engine import (COSTS, Engine, EngineUnavailable, SVError, device_count, get_engine,
                     load_library, plan)
from .fusion import (bilateral_filter, bilateral_filter_dev, bilateral_tables, fuse_maps,
                     fuse_maps_dev, gaussian_blur, gaussian_kernel)

__all__ = ["COSTS", "Engine", "EngineUnavailable", "SVError", "device_count", "get_engine",
           "load_library", "plan", "bilateral_filter", "bilateral_filter_dev", "bilateral_tables",
           "fuse_maps", "fuse_maps_dev", "gaussian_blur", "gaussian_kernel", "fuse_depth_maps",
           "farneback_flow", "farneback_flow_dev", "OpticalFlowDepthEstimator"]


def __getattr__(name):
    # fused_depth_map starts the engine warm-up when it is imported: only on first use
    if name == "fuse_depth_maps":
        from .fused_depth_map import fuse_depth_maps
        return fuse_depth_maps
    if name in ("farneback_flow", "farneback_flow_dev", "OpticalFlowDepthEstimator"):
        from . import flow
        return getattr(flow, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
