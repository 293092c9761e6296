"""CPU: the NumPy restatement of the frame event filters (tests/frame_filter_ref.py) reproduces the outputs of the reference's own
classes (golden G5) for all four; its `intended` form keeps the first event per cell."""
import os

import numpy as np
import pytest

import frame_filter_ref as R
from x_maps_amd import synthetic as S


def _golden_events(golden_dir):
    g = np.load(os.path.join(golden_dir, "g5_filters.npz"))
    ev = np.zeros(len(g["t"]), S.EVENT_CD_DTYPE)
    ev["x"], ev["y"], ev["t"], ev["p"] = g["x"], g["y"], g["t"], g["p"]
    return g, ev


@pytest.mark.parametrize("cls", sorted(R.BY_CLASS))
def test_restatement_matches_the_references_outputs(golden_dir, cls):
    g, ev = _golden_events(golden_dir)
    out = R.filter_events(ev, g["xp"], R.BY_CLASS[cls])
    assert out.dtype == S.EVENT_CD_DTYPE and len(out) == len(g[f"{cls}_t"])
    for fld in ("x", "y", "t", "p"):
        assert np.array_equal(out[fld], g[f"{cls}_{fld}"]), (cls, fld)


def test_intended_semantics_keep_the_first_event_and_int32_wraps(golden_dir):
    g, ev = _golden_events(golden_dir)
    pos = ev[ev["p"] == 1]
    first = {}
    for i in range(len(pos)):
        first.setdefault((int(pos["y"][i]), int(pos["x"][i])), i)
    want = np.array([first[k] for k in sorted(first)])
    out = R.filter_events(ev, None, R.FIRST_PER_XY, intended=True)
    assert np.array_equal(out["t"], pos["t"][want]) and np.array_equal(out["x"], pos["x"][want])
    assert not np.array_equal(out["t"], R.filter_events(ev, None, R.FIRST_PER_XY)["t"])
    big = ev.copy()
    big["t"] += (1 << 31) + 12345
    out = R.filter_events(big, None, R.LAST_PER_XY)
    assert (out["t"] < 0).all() and np.array_equal(out["t"], R.filter_events(ev, None, R.LAST_PER_XY)["t"] + 12345 - (1 << 31))
    # a negative column wraps at the frame's own width; one that is still out of range raises, as in the reference
    xp = g["xp"].astype(np.int16) - 12
    assert xp.min() < 0
    last, _ = R.survivor_maps(ev, xp, R.FIRST_PER_YT)
    assert last.shape[1] == int(xp.max()) + 1 and (last[:, xp.min():] >= 0).any()
    with pytest.raises(IndexError):
        R.survivor_maps(ev, np.where(xp < 0, -1000, xp), R.FIRST_PER_YT)
