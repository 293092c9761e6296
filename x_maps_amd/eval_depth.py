"""The reference's offline-evaluation caller of the hot path (python/eval/compute_depth_x_maps.py:81-114) on the GPU.

That script turns one camera time surface (a float image, 0 = no event) into "events" in raster order with a
normalised float timestamp, then calls the same per-event functions as the live pipe -- rectify, compute_event_disparity,
compute_disp_map_camera_view, disparity_to_depth_rectified -- and, for the point cloud, rectify_cam_coords_f32 +
construct_point_cloud.  Raster order means the timestamps are NOT sorted: this goes through the general
(min/max-reduction) path of the engine, never the time-sorted one.

Two routes: compute_depth_from_time_surface, the reference's stage sequence (or the live path's fused kernels) for one
surface, with the front half -- normalising, argwhere, the x / y / t columns -- on the host; and
compute_depths_from_time_surfaces, a GROUP of surfaces in one device call (XMapsEngine.process_time_surfaces: surfaces in,
depth maps and point clouds out, nothing on the host in between, no atomics; camera view).  Both widen the surface to float64
before normalising it (the reference normalises a float32 file in float32: the last bit of t can differ; golden G7 pins
this build's choice), and both give the same depth maps and clouds bit for bit.

The baseline of the same evaluation, ESL-init (compute_depth_esl.py up to depth_init), takes the same surfaces: esl_init.py; so does the
MC3D baseline (mc3d_baseline.py): mc3d.py.  ESL's depth optimisation behind ESL-init (depth_optimization): esl_optim.py.

The other direction -- a frame of events -> its camera time surface, the `scans_np` image these routes start from -- is
XMapsEngine.frames_to_time_surfaces (a group of frames in one device call), DeviceIngest.set_surface_output / surface (every cut
frame of a live stream or a replay) and RuntimeParams.surface_callback; tools/run_esl_on_arrival.py --scans-from-raw writes the
files.  Those surfaces are this build's definition (include/xmaps.h): the ESL dataset's own events-to-scan converter is not part
of the reference, so they are not pinned against its scans_np files.  The filters behind ESL's optimisation, which
turn its maps into the table's ground truth: esl_filter.py.

Out of scope: a projector-view surface path; device-resident surfaces in the Python interface.  (The metrics of
eval/ are in eval_metrics.py.)
"""
from __future__ import annotations

import numpy as np

from .cam_proj_calibration import CamProjMaps
from .disp_to_depth import disparity_to_depth_rectified
from .x_maps_disparity import XMapsDisparity


def time_surface_to_events(cam_image):
    """eval/compute_depth_x_maps.py:83-97: normalise the non-zero times to [0, 1], clip negatives, list the pixels that
    stay > 0 in raster order.  (The earliest event lands on exactly 0 and is dropped -- as in the reference.)"""
    cam_image = np.array(cam_image, dtype=np.float64, copy=True)
    nz = cam_image != 0
    if not nz.any():
        return None
    lo, hi = cam_image[nz].min(), cam_image[nz].max()
    cam_image = (cam_image - lo) / (hi - lo)
    cam_image[cam_image < 0] = 0
    yx = np.argwhere(cam_image > 0)
    return {"x": yx[:, 1], "y": yx[:, 0], "t": cam_image[cam_image > 0]}


def compute_depth_from_time_surface(cam_proj_maps: CamProjMaps, x_maps_disp: XMapsDisparity, cam_image,
                                    want_point_cloud: bool = False, fused: bool = False):
    """-> (depth [cam_h][cam_w] float32, point_cloud [k][3] float32 or None); None, None for an empty surface.
    eval/compute_depth_x_maps.py:99-120.  fused=True runs the three fused kernels of the live path instead of the
    reference's stage sequence (needs cam_proj_maps built with camera_perspective=True); the depth map is identical."""
    if fused and want_point_cloud:  # depth AND cloud on the device: the group entry with a group of one
        if not cam_proj_maps.camera_perspective:
            raise ValueError("fused evaluation needs CamProjMaps(camera_perspective=True)")
        if not np.any(np.asarray(cam_image) != 0):
            return None, None
        depth, cloud, _ = cam_proj_maps.engine.process_time_surfaces([cam_image], want_cloud=True)[0]
        return depth, cloud
    events = time_surface_to_events(cam_image)
    if events is None:
        return None, None
    if fused and not want_point_cloud:
        if not cam_proj_maps.camera_perspective:
            raise ValueError("fused evaluation needs CamProjMaps(camera_perspective=True)")
        depth, _, _ = cam_proj_maps.engine.process_frame(events["x"], events["y"], events["t"], want_depth=True,
                                                         want_bgr=False)
        return depth, None
    xr, yr = cam_proj_maps.rectify_cam_coords_i16(events)
    disp, mask = x_maps_disp.compute_event_disparity(events=events, ev_x_rect_i16=xr, ev_y_rect_i16=yr)
    disparity = cam_proj_maps.compute_disp_map_camera_view(events=events, inlier_mask=mask, ev_disparity_f32=disp)
    depth = disparity_to_depth_rectified(disparity, cam_proj_maps.P2, engine=cam_proj_maps.engine)
    cloud = None
    if want_point_cloud:
        xr_f, yr_f = cam_proj_maps.rectify_cam_coords_f32(events)
        cloud = cam_proj_maps.construct_point_cloud(xr_f[mask], yr_f[mask], disp)
    return depth, cloud


def compute_depths_from_time_surfaces(cam_proj_maps: CamProjMaps, cam_images, want_point_cloud: bool = False):
    """A group of time surfaces (list of [cam_h][cam_w] arrays or a 3-D array) in one device call ->
    [(depth, point_cloud or None)] per surface, each as compute_depth_from_time_surface returns it: (None, None) for an
    all-zero surface.  Needs cam_proj_maps built with camera_perspective=True (and, for clouds, tables with cam_mapx_f32,
    cam_mapy_f32 and Q)."""
    if not cam_proj_maps.camera_perspective:
        raise ValueError("the time-surface entry needs CamProjMaps(camera_perspective=True)")
    res = cam_proj_maps.engine.process_time_surfaces(cam_images, want_cloud=want_point_cloud)
    return [(None, None) if st.n_nonzero == 0 else (depth, cloud) for depth, cloud, st in res]
