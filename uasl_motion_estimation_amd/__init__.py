"""uasl_motion_estimation_amd — MI355X-native stereo-VO hot path.

A from-scratch HIP/CDNA4 implementation of the inner loop of
abeauvisage/uasl_motion_estimation: mutual-information patch scores and the
MI stereo-scale optimiser, KLT track updates, the corner detector that seeds
them, scanline NMS and the windowed stereo bundle adjuster (residual/Jacobian
kernels + on-device Schur on FP64 MFMA), behind the C ABI of include/me_hip.h
(libme_hip.so).
"""
from ._lib import Context, MEError, default_context, device_count, load_library  # noqa: F401
from .corners import (corner_params, corner_response, corner_response_ref, new_corners,  # noqa: F401
                      new_corners_ref)
from .equalise import Clahe, clahe, clahe_ref  # noqa: F401
from .frame_pose import (FramePose, frame_pose_device, frame_pose_ref,  # noqa: F401  (frame_pose.frame_pose: the device call)
                         info_words as frame_pose_info_words, parse_info as frame_pose_parse_info)
from .tonemap import ToneMap, ToneMapState, tonemap_ref  # noqa: F401  (tonemap.tonemap: the device call)
from .rectify import (CameraModel, RectifiedModel, StereoRectifier, rectify_map, rectify_map_ref,  # noqa: F401
                      remap, remap_ref)

__all__ = ["Context", "MEError", "default_context", "device_count", "load_library", "corner_params",
           "corner_response", "corner_response_ref", "new_corners", "new_corners_ref", "Clahe", "clahe",
           "clahe_ref", "FramePose", "frame_pose_device", "frame_pose_ref", "frame_pose_info_words",
           "frame_pose_parse_info", "ToneMap", "ToneMapState", "tonemap_ref", "CameraModel",
           "RectifiedModel", "StereoRectifier", "rectify_map", "rectify_map_ref", "remap", "remap_ref"]
