"""GPU: RuntimeParams.tables_on_device -- a pipe on a calibration YAML builds the same tables with the switch as without it."""
import numpy as np
import pytest

import rig_maps_cases as RC
from x_maps_amd.depth_reprojection_pipe import DepthReprojectionPipe
from x_maps_amd.depth_reprojection_processor import RuntimeParams
from x_maps_amd.stats import StatsPrinter

pytestmark = pytest.mark.gpu


def _write_reference_yaml(path):
    """the reference's calibration file layout (python/cam_proj_calibration.py:10-28,77-108) from the fixture's arrays, at rig L's
    scale: from_yaml zeroes the projector's distortion and takes rect = round(2.75 x camera), which is rig L"""
    import yaml
    cp = RC.params("L")
    g = RC.g6()

    def node(a):
        a = np.asarray(a, dtype=float)
        a = a.reshape(a.shape[0], -1)
        return {"type-id": "opencv_matrix", "rows": int(a.shape[0]), "cols": int(a.shape[1]), "dt": "d", "data": a.ravel().tolist()}

    doc = {"camera_intrinsic_matrix": node(cp.camera_K), "camera_distortion_coefficients": node(np.asarray(cp.camera_D).reshape(1, 5)),
           "projector_intrinsic_matrix": node(cp.projector_K), "projector_distortion_coefficients": node(g["projector_D"]),
           "relative_rotation": node(g["R"]), "relative_translation": node(g["T"]), "F": node(np.eye(3))}
    path.write_text(yaml.safe_dump(doc))
    return cp


def test_pipe_builds_the_same_tables_on_the_device(tmp_path):
    path = tmp_path / "calib.yaml"
    cp = _write_reference_yaml(path)
    tables = []
    for on_device in (False, True):
        params = RuntimeParams(camera_width=cp.camera_width, camera_height=cp.camera_height, projector_width=cp.projector_width,
                               projector_height=cp.projector_height, projector_fps=60, z_near=0.1, z_far=1.2, calib=str(path),
                               tables_on_device=on_device)
        assert RuntimeParams.__dataclass_fields__["tables_on_device"].default is False
        pipe = DepthReprojectionPipe(params, StatsPrinter(), lambda frame: None)
        try:
            tables.append(dict(pipe.calib_maps.tables))
        finally:
            pipe.close()
    want, got = tables
    assert set(got) == set(want)
    assert (want["rect_w"], want["rect_h"]) == (220, 165)
    n_arrays = 0
    for k, w in want.items():
        if isinstance(w, np.ndarray):
            n_arrays += 1
            g = got[k]
            assert g.dtype == w.dtype and g.shape == w.shape, k
            assert RC.bits_equal(g, w) if w.dtype == np.float32 else np.array_equal(g, w), k
        else:
            assert got[k] == w, k
    assert n_arrays >= 8 and int((np.asarray(got["proj_x_map"]) != 0).sum()) > 0
