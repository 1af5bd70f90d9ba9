"""`from src.dust3r.post_process import estimate_focal_knowing_depth` (/root/reference/hislam2/track_frontend.py:10, commented out there):
the signature and return value of /root/reference/src/dust3r/post_process.py:12-64 -- `estimate_focal_knowing_depth(pts3d, pp,
focal_mode="median", min_focal=0.0, max_focal=np.inf) -> focal [B]` -- plus an optional confidence gate, on the HIP kernels."""
from . import _root  # noqa: F401
from cut3r_slam_amd.self_calib import estimate_focal_knowing_depth  # noqa: E402,F401

__all__ = ["estimate_focal_knowing_depth"]
