#!/usr/bin/env python3
"""Generate tests/golden/g11_esl_init.npz by RUNNING THE REFERENCE'S OWN FUNCTIONS of python/eval/compute_depth_esl.py:
disparity_init (:72-85), get_projector_time_surface (:94-101) and disparity_to_depth_rectified (:88-91).

Run only in the build container (needs /root/reference, which does not exist on the GPU box):
    python tests/golden/make_golden_esl_init.py
The module imports cv2 and esl_utilities at its top; neither is installed offline and the three functions touch neither, so both
are replaced by empty in-process stubs before the import (scipy.optimize is present).  Nothing from /root/reference is copied: the
.npz holds inputs and the outputs the reference produced for them -- data, not source.  The one third-party call between the
captured functions, cv2.remap(INTER_NEAREST, BORDER_CONSTANT) of the disparity back to the camera (:219), is a plain NumPy gather
through an int16 map here (stored beside its result).

Inputs: float64 camera rows against float32 projector rows, 12 x 1100 (frame "a": hand-built rows for every edge, then random
rows) and 3 x 2300 (frame "b").  The script ASSERTS that the inputs hold every case it exists for -- see check_cases().

One case of the issue's list cannot exist: "two candidates whose squared differences both underflow to 0".  A candidate p is a
non-zero float32 (|p| >= 2^-149), e a float64: p - e is exact-or-rounded to a multiple of the smaller operand's ulp, so it is
either 0 or at least 2^-201 in magnitude, and its square at least 2^-402 -- far above float64's underflow threshold (2^-1074).
Only d == 0 gives cost 0.  What the case is after -- several candidates share the minimal cost 0 and the first must win -- is
covered by two SEPARATE exact matches with a worse candidate between them (row 6); the same at the other end of the range, every
square overflowing to +inf, is row 7."""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF_EVAL = "/root/reference/python/eval"
MIN_D, MAX_D = 5, 900


def import_reference():
    for name, kw in (("cv2", {}), ("esl_utilities", {"utils": object})):
        m = types.ModuleType(name)
        m.__dict__.update(kw)
        sys.modules[name] = m
    sys.path.insert(0, REF_EVAL)
    import compute_depth_esl
    return compute_depth_esl


def remap_like_rows(rng, h, w, density, run):
    """projector rows as a nearest remap of a rising surface makes them: runs of equal values, holes of zeros"""
    base = np.sort(rng.random((h, (w + run - 1) // run)).astype(np.float32), axis=1)
    rows = np.repeat(base, run, axis=1)[:, :w].copy()
    rows[rng.random((h, w)) >= density] = 0
    return rows


def frame_a(rng):
    h, w = 12, 1100
    cam = np.zeros((h, w), np.float64)
    proj = np.zeros((h, w), np.float32)
    # row 0: dense random -- full (c <= 200), clipped and empty (c >= 1095) windows, runs of equal values, values <= 0
    proj[0] = remap_like_rows(rng, 1, w, 0.8, 3)[0]
    cam[0] = rng.random(w)
    cam[0, rng.random(w) < 0.4] = 0
    cam[0, rng.random(w) < 0.1] = -0.25
    cam[0, 1095:] = [0.5, 0.25, 0.75, 0.1, 0.9]  # empty windows: c + 5 >= w
    # row 1: no candidate at all
    cam[1, [0, 100, 200, 640, 1094, 1099]] = 0.5
    # row 2: c = 100 sees exactly one candidate (-> 0), c = 200 exactly two
    proj[2, 300], proj[2, 1050] = 0.4, 0.6
    cam[2, 100], cam[2, 200] = 0.41, 0.41
    # row 3: an exact match at disparity 5; a winner at disparity 899
    proj[3, 15], proj[3, 400], proj[3, 919] = 0.5, 0.3, 0.78125
    cam[3, 10], cam[3, 20] = 0.5, 0.78125
    # row 4: strictly closer values just outside the window, at c + 4 and at c + 900: neither may win
    c = 50
    proj[4, c + 4], proj[4, c + 5], proj[4, 500], proj[4, c + 899], proj[4, c + 900] = 0.6, 0.61, 0.7, 0.62, 0.6
    cam[4, c] = 0.6
    # row 5: e + delta in front of e - delta, equal cost: the first wins (not the smaller value)
    proj[5, 120], proj[5, 130], proj[5, 700] = 0.5 + 2.0 ** -10, 0.5 - 2.0 ** -10, 0.9
    cam[5, 100] = 0.5
    # row 6: two separate exact matches (cost 0 twice) around a worse candidate: the first wins
    proj[6, 210], proj[6, 220], proj[6, 230] = 0.375, 0.5, 0.375
    cam[6, 200] = 0.375
    # row 7: every square overflows to +inf: the first candidate wins; values <= 0 beside good candidates are skipped
    proj[7, 310], proj[7, 320] = 0.25, 0.75
    cam[7, 300], cam[7, 301], cam[7, 302] = 1e200, 0.0, -0.75
    # rows 8-11: random, sparse to dense projector rows
    for r, (density, run) in zip(range(8, 12), ((0.01, 1), (0.3, 2), (0.7, 5), (1.0, 4))):
        proj[r] = remap_like_rows(rng, 1, w, density, run)[0]
        cam[r] = rng.random(w)
        cam[r, rng.random(w) < 0.5] = 0
    return cam, proj


def frame_b(rng):
    h, w = 3, 2300
    proj = remap_like_rows(rng, h, w, 0.9, 3)
    proj[:, :150] = 0
    proj[:, -260:] = 0
    cam = rng.random((h, w))
    cam[rng.random((h, w)) < 0.5] = 0
    return cam, proj


def windows(cam, proj):
    """per pixel > 0: (r, c, columns of the window's candidates, their costs)"""
    w = cam.shape[1]
    for r, c in zip(*np.nonzero(cam > 0)):
        cols = np.arange(c + MIN_D, min(c + MAX_D, w))
        cols = cols[proj[r, cols] != 0] if len(cols) else cols
        with np.errstate(over="ignore"):
            yield r, c, cols, (proj[r, cols].astype(np.float64) - cam[r, c]) ** 2


def check_cases(cam, proj, disp):
    """every case the fixture exists for, found in frame a's inputs and the reference's output"""
    w = cam.shape[1]
    seen = set()
    for r, c, cols, cost in windows(cam, proj):
        d = int(disp[r, c])
        seen.add("full" if c + MAX_D <= w else "empty" if c + MIN_D >= w else "clipped")
        seen.add("cand0" if len(cols) == 0 else "cand1" if len(cols) == 1 else "cand2" if len(cols) == 2 else "many")
        if len(cols) <= 1:
            assert d == 0
            continue
        assert d == cols[np.argmin(cost)] - c and MIN_D <= d < MAX_D
        best = cost.min()
        if d == MIN_D:
            seen.add("win5")
        if d == MAX_D - 1:
            seen.add("win899")
        e = cam[r, c]
        for off, tag in ((MIN_D - 1, "closer_c+4"), (MAX_D, "closer_c+900")):
            if c + off < w and proj[r, c + off] != 0 and (np.float64(proj[r, c + off]) - e) ** 2 < best:
                seen.add(tag)
        ties = cols[cost == best]
        if len(ties) > 1:
            assert d == ties[0] - c
            pv = proj[r, ties]
            if np.all(pv == pv[0]) and np.all(np.diff(ties) == 1):
                seen.add("run_tie")
            if len(ties) == 2 and best > 0 and np.isfinite(best) and pv[0] - e == e - pv[1]:
                seen.add("plus_minus_delta_tie")
            if best == 0 and np.any(np.diff(ties) > 1):
                seen.add("cost0_twice")
            if np.isinf(best):
                seen.add("all_inf")
        if best == 0:
            seen.add("exact")
    if np.any((cam <= 0) & (disp == 0)) and np.any(cam < 0):
        seen.add("skipped")
    assert not np.any(disp[cam <= 0])
    need = {"full", "clipped", "empty", "cand0", "cand1", "cand2", "win5", "win899", "closer_c+4", "closer_c+900", "run_tie",
            "plus_minus_delta_tie", "exact", "cost0_twice", "all_inf", "skipped"}
    assert need <= seen, sorted(need - seen)
    return sorted(seen)


def main():
    assert os.path.isdir(REF_EVAL), "needs /root/reference (build container only)"
    ref = import_reference()
    rng = np.random.default_rng(11)
    out = {}
    for tag, (cam, proj) in (("a", frame_a(rng)), ("b", frame_b(rng))):
        disp = ref.disparity_init(cam, proj)
        assert disp.dtype == np.float64 and np.array_equal(disp, np.rint(disp)) and disp.max() < MAX_D
        out[f"{tag}_cam_rect"], out[f"{tag}_proj_rect"], out[f"{tag}_disparity"] = cam, proj, disp.astype(np.uint16)
    print("frame a cases:", check_cases(out["a_cam_rect"], out["a_proj_rect"], out["a_disparity"]))
    assert any(c + MAX_D <= 2300 for _, c, _, _ in windows(out["b_cam_rect"], out["b_proj_rect"]))
    out["proj_7x11"] = ref.get_projector_time_surface((7, 11))
    assert out["proj_7x11"].shape == (11, 7) and out["proj_7x11"].dtype == np.float32 and out["proj_7x11"][0, 0] == 0
    # the disparity back in a 14 x 9 camera (nearest, border 0; entries outside the frame included), then the reference's depth
    back = np.stack((rng.integers(-3, 1103, (9, 14)), rng.integers(-2, 14, (9, 14))), -1).astype(np.int16)
    back[0, :4] = [[10, 3], [20, 3], [100, 5], [200, 2]]  # (known non-zero disparities of the hand-built rows)
    mx, my = back[..., 0].astype(np.int64), back[..., 1].astype(np.int64)
    ok = (mx >= 0) & (mx < 1100) & (my >= 0) & (my < 12)
    disp_cam = np.zeros((9, 14), np.float64)
    disp_cam[ok] = ref.disparity_init(out["a_cam_rect"], out["a_proj_rect"])[my[ok], mx[ok]]
    disp_cam = disp_cam.astype(np.float32)  # (:219-221)
    assert np.count_nonzero(disp_cam) >= 4 and np.count_nonzero(disp_cam == 0) >= 4 and not ok.all()
    out["back_map"], out["disp_cam"] = back, disp_cam
    for tag, p03 in (("pos", 5821.0837), ("neg", -5821.0837)):
        P1 = np.zeros((3, 4))
        P1[0, 3] = p03
        with np.errstate(divide="ignore"):
            depth = ref.disparity_to_depth_rectified(disp_cam.copy(), P1, None, None)
        assert np.all(np.isfinite(depth)) and np.all((depth == 0) == (disp_cam == 0))
        out[f"depth_{tag}"], out[f"p1_03_{tag}"] = depth, np.float64(p03)
    path = os.path.join(HERE, "g11_esl_init.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(path, size, "bytes")
    assert size < 300 * 1024


if __name__ == "__main__":
    main()
