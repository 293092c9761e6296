"""-m gpu: the patch loaders of the tiled frame kernel K2 (frame_proj_tiled_body, xmaps_k2.hpp) that the shapes of
tests/test_gpu_a4_bruteforce.py do not reach, against the 49-tap definition of A4 (k2_frame_cases.shifted_dilate_remap, pinned to
the loops by tests/test_k2_frame_cases_cpu.py) and the oracle's A5 - A7:

* interior patches of more than 64 rows: the u16 loader's divide by the octet count, the 64-bit loader's 8-load variant;
* a patch that does not fit in LDS: the per-pixel reads of the frame, in both formats;
* interior patches of 2, 3 and 4 sixteen-byte loads per thread: the 64-bit loader's smaller unroll variants;
* interior tiles of a frame whose height is 4 mod 8: the u16 loader's 8-byte loads;

each at one pixel per thread (what a lone frame of these projectors takes) and at two (XM_K2_PPT=2), through xm_shard_finish on a
hand-built 64-bit key frame with stale cells and through xm_shard_finish_u16 on the plain disparities.  Which loader a tile takes is
worked out on the CPU (k2_frame_cases.classify_tiles) and asserted before anything is launched."""
import functools

import numpy as np
import pytest

from conftest import xm_option
from x_maps_amd import XMapsEngine
import k2_frame_cases as K

pytestmark = pytest.mark.gpu

KEY_IDX_SHIFT, KEY_TAG_SHIFT, TAG = 16, 44, 7


@functools.lru_cache(maxsize=None)
def _case(shape):
    """(tables, keys u64 [rect_w][rect_h], disparities u16 [rect_w][rect_h], depth, bgr): computed once per shape, never written to"""
    rect_w, rect_h = shape[:2]
    tb, rng = K.border_tables(*shape, seed=rect_w)
    rect = K.sparse_frame(rng, rect_w, rect_h, 0.2)
    idx = rng.integers(0, 1 << 20, rect.shape).astype(np.uint64)
    keys = (np.uint64(TAG) << np.uint64(KEY_TAG_SHIFT)) | (idx << np.uint64(KEY_IDX_SHIFT)) | rect.astype(np.uint64)
    keys[rect == 0] = 0
    stale = (rect == 0) & (rng.random(rect.shape) < 0.3)  # cells of an older frame (smaller tag) read as empty
    keys[stale] = (np.uint64(TAG - 1) << np.uint64(KEY_TAG_SHIFT)) | np.uint64(777)
    depth, bgr = K.expected(tb, rect)
    out = (np.ascontiguousarray(keys.T).view(np.int64), np.ascontiguousarray(rect.T).astype(np.uint16).view(np.int16), depth, bgr)
    for a in out:
        a.setflags(write=False)
    return (tb,) + out


def _run(eng, fmt, frame, want_depth=True, want_bgr=True):
    """the lone-frame tiled K2 on a device copy of `frame` (column-major [col][row]) -> (depth or None, bgr or None)"""
    d0 = np.full((eng.out_h, eng.out_w), -1.0, np.float32) if want_depth else None  # (what the outputs hold before: no right value)
    b0 = np.full((eng.out_h, eng.out_w, 3), 7, np.uint8) if want_bgr else None
    dev = eng.to_device(frame)
    depth = eng.to_device(d0) if want_depth else None
    bgr = eng.to_device(b0) if want_bgr else None
    try:
        if fmt == "key64":
            eng.shard_finish(dev, TAG, depth, bgr)
        else:
            eng.shard_finish_u16(dev, depth, bgr)
        eng.sync()
        if want_depth:
            eng.dev_download(d0, depth)
        if want_bgr:
            eng.dev_download(b0, bgr)
    finally:
        for p in (dev, depth, bgr):
            if p is not None:
                eng.dev_free(p)
    return d0, b0


def test_the_shapes_reach_every_loader_named_above():
    for ppt, wanted in K.TILED_PATHS_WANTED.items():
        reached = set()
        for shape in K.TILED_PATH_CASES:
            reached |= K.tiled_loader_paths(_case(shape)[0], ppt)
        assert wanted <= reached, (ppt, wanted - reached)


@pytest.mark.parametrize("ppt", [1, 2])
@pytest.mark.parametrize("shape", K.TILED_PATH_CASES, ids=lambda s: "x".join(str(v) for v in s))
def test_tiled_k2_equals_the_49_tap_definition_on_both_formats(shape, ppt):
    tb, keys, d16, want_depth, want_bgr = _case(shape)
    assert K.tiled_loader_paths(tb, ppt)  # (classified before the launch: the reach test above says what the shapes cover)
    if ppt == 2:
        xm_option("XM_K2_PPT", "2")  # (read when the handle is created; one pixel per thread is these grids' default)
    with XMapsEngine(tb) as eng:
        for fmt, frame in (("key64", keys), ("u16", d16)):
            depth, bgr = _run(eng, fmt, frame)
            assert np.array_equal(depth, want_depth), fmt
            assert np.array_equal(bgr, want_bgr), fmt


@pytest.mark.parametrize("fmt", ["key64", "u16"])
def test_either_output_may_be_null(fmt):
    """depth null on the shape with the large interior patches, bgr null on the one whose patch does not fit in LDS"""
    for shape, null in ((K.TILED_PATH_CASES[0], "depth"), (K.TILED_PATH_CASES[1], "bgr")):
        tb, keys, d16, want_depth, want_bgr = _case(shape)
        with XMapsEngine(tb) as eng:
            depth, bgr = _run(eng, fmt, keys if fmt == "key64" else d16, want_depth=null != "depth", want_bgr=null != "bgr")
        if null == "depth":
            assert depth is None and np.array_equal(bgr, want_bgr)
        else:
            assert bgr is None and np.array_equal(depth, want_depth)
