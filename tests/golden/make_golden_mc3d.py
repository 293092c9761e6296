#!/usr/bin/env python3
"""Generate tests/golden/g12_mc3d.npz by RUNNING THE REFERENCE'S OWN FUNCTIONS of python/eval/mc3d_baseline.py:
compute_disparity (:40-78) and disparity_to_depth (:15-18).

Run only in the build container (needs /root/reference, which does not exist on the GPU box):
    python tests/golden/make_golden_mc3d.py
The module imports cv2 and esl_utilities at its top; neither is installed offline and the two functions touch neither, so both are
replaced by empty in-process stubs before the import (as make_golden_esl_init.py does).  Nothing from /root/reference is copied:
the .npz holds inputs and the outputs the reference produced for them -- data, not source.  cv2.medianBlur (:130) sits in front
of the captured function and is not part of the fixture: the surfaces go to compute_disparity as stored.

Three rigs (projector W x H, camera w x h; no camera is a multiple of 64 x 4):
    a   5 x 100,  37 x 13   nc 6,   window 12: narrower than a wave; hand-built scenarios, one per projector column stretch
    b   6 x 990,  70 x 9    nc 66,  window 132: the third trip of 64 is partial
    c   7 x 1920, 45 x 6    nc 128, the reference's window
Each rig has a float32 surface and a float64 one (the float32 values widened, plus pixels whose float32 rounding names another
projector pixel than the float64 value does).  The script ASSERTS that inputs and outputs hold every case it exists for -- see
check_cases(), which re-derives each pixel's window in plain Python integers."""
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF_EVAL = "/root/reference/python/eval"
FAR = 500.25  # a projector row this far from every admissible yc (< 3 * W <= 21) costs more than 50


def import_reference():
    for name, kw in (("cv2", {}), ("esl_utilities", {"utils": object})):
        m = types.ModuleType(name)
        m.__dict__.update(kw)
        sys.modules[name] = m
    sys.path.insert(0, REF_EVAL)
    import mc3d_baseline
    return mc3d_baseline


def v_of(idx, wh):
    """a float32 surface value whose id is idx (half an id of margin on either side)"""
    v = np.float32((idx + 0.5) / wh)
    assert int(np.float32(wh) * v) == idx
    return v


class Rig:
    def __init__(self, W, H, cw, ch, rng):
        self.W, self.H, self.cw, self.ch, self.rng = W, H, cw, ch, rng
        self.nc = int(H / 15)
        self.x_lim, self.y_lim = 3 * H, 3 * W  # (swapped, as the reference tests them)
        self.pmx = np.full((H, W), 3.5, np.float32)
        self.pmy = np.full((H, W), FAR, np.float32)
        self.cmx = np.full((ch, cw), 10.5, np.float32)
        self.cmy = np.full((ch, cw), 7.5, np.float32)
        self.surf = np.zeros((ch, cw), np.float32)
        self.free = [(i, j) for i in range(ch) for j in range(cw)]
        rng.shuffle(self.free)
        self.tags = {}  # scenario name -> camera pixel

    def pixel(self, tag, v, xc=10.5, yc=7.5):
        i, j = self.free.pop()
        self.surf[i, j], self.cmx[i, j], self.cmy[i, j] = v, xc, yc
        if tag:
            self.tags[tag] = (i, j)
        return i, j

    def at(self, tag, col, row, xc=10.5, yc=7.5):
        return self.pixel(tag, v_of(col * self.H + row, self.W * self.H), xc, yc)

    def random_columns(self, cols, density, nan_rate=0.0):
        rng, H = self.rng, self.H
        for c, dens in zip(cols, density):
            on = rng.random(H) < dens
            self.pmy[on, c] = rng.uniform(-45, 65, on.sum()).astype(np.float32)
            self.pmx[:, c] = rng.uniform(-20, self.x_lim + 40, H).astype(np.float32)
            frac = rng.random(H) < 0.05  # entries in (-1, 0): truncate to 0
            self.pmy[on & frac, c] = -rng.uniform(0.05, 0.95, (on & frac).sum()).astype(np.float32)
            if nan_rate:
                self.pmy[rng.random(H) < nan_rate, c] = np.nan
                self.pmx[rng.random(H) < nan_rate, c] = np.inf

    def random_pixels(self, n, cols):
        rng = self.rng
        for _ in range(n):
            col, row = int(rng.choice(cols)), int(rng.integers(0, self.H))
            xc = rng.uniform(-2, self.x_lim + 2) if rng.random() < 0.15 else rng.uniform(1, 60)
            yc = rng.uniform(-1.5, self.y_lim + 1.5)
            self.at(None, col, row, np.float32(xc), np.float32(yc))

    def specials(self):
        """surface values that name no projector pixel, and the two ends of the range"""
        self.pixel("v_one", np.float32(1.0))
        self.pixel("v_above_one", np.float32(1.5))
        self.pixel("v_inf", np.float32(np.inf))
        self.pixel("v_last", np.float32(1.0) - np.float32(2.0 ** -24))
        self.pixel("v_id0", np.float32(1e-6))
        self.pixel("v_negative", np.float32(-0.25))
        self.pixel("cam_nan", v_of(3, self.W * self.H), np.nan, 7.5)
        self.pixel("cam_inf", v_of(3, self.W * self.H), 10.5, -np.inf)

    def surf64(self):
        """the float32 surface widened; three pixels get float64 values just below an id boundary that float32 rounds across"""
        s = self.surf.astype(np.float64)
        wh = self.W * self.H
        n = 0
        for k in range(1, wh):
            v = k / wh - 1e-13
            if int(wh * v) == k - 1 and int(np.float32(wh) * np.float32(v)) == k:
                i, j = self.free.pop()
                s[i, j] = v
                self.surf[i, j] = np.float32(v)
                self.tags[f"f64_{n}"] = (i, j)
                n += 1
                if n == 3:
                    break
        assert n == 3
        return s


def rig_a(rng):
    r = Rig(5, 100, 37, 13, rng)
    r.random_columns([0, 1], [0.9, 0.3], nan_rate=0.02)
    xc, yc = 10.5, 7.5  # -> 10, 7
    # column 2: ties, the acceptance bound, poison inside / outside a window
    r.pmy[12, 2], r.pmx[12, 2], r.pmy[18, 2], r.pmx[18, 2] = 4.2, 17.0, 10.9, 19.0  # |7 - 4| == |7 - 10|: row 12 wins
    r.at("tie_minus_first", 2, 16)
    r.pmy[33, 2], r.pmx[33, 2] = 57.3, 14.0  # cost exactly 50: accepted
    r.at("cost_50", 2, 36)
    r.pmy[55, 2], r.pmx[55, 2] = 58.0, 14.0  # cost 51: refused
    r.at("cost_51", 2, 56)
    r.pmy[70, 2] = np.nan
    r.pmy[76, 2], r.pmx[76, 2] = 7.0, 15.9
    r.at("nan_inside", 2, 75)   # window [69, 81)
    r.at("nan_outside", 2, 77)  # window [71, 83)
    r.pmx[90, 2] = np.nan  # (a poisoned x beside a good y poisons the window as well)
    r.pmy[92, 2], r.pmx[92, 2] = 7.0, 15.9
    r.at("nan_x_inside", 2, 93)
    # column 3: the winner's disparity 1, 0, negative beside a losing candidate with a positive one; truncation
    for tag, row, xw in (("disp_1", 14, 11.2), ("disp_0", 34, 10.9), ("disp_neg", 54, 2.0)):
        r.pmy[row, 3], r.pmx[row, 3] = 7.9, xw          # cost 0
        r.pmy[row + 2, 3], r.pmx[row + 2, 3] = 9.0, 40.0  # cost 2, disparity 30
        r.at(tag, 3, row + 1)
    r.pmy[72, 3], r.pmx[72, 3], r.pmy[78, 3], r.pmx[78, 3] = -0.5, 21.0, 10.25, 23.0  # yc 5: |5 - 0| == |5 - 10|, floor would say 6
    r.at("trunc_not_floor", 3, 75, 10.5, 5.5)
    r.pmy[86, 3], r.pmx[86, 3], r.pmy[94, 3], r.pmx[94, 3] = -3.7, 25.0, 13.0, 27.0   # yc 5: |5 + 3| == |5 - 13|, floor would say 9
    r.at("trunc_negative", 3, 90, 10.5, 5.5)
    # column 4: every row admissible for every yc, x far to the right: the rect limits decide alone
    r.pmy[:, 4], r.pmx[:, 4] = 7.0, 400.0
    for k, row in zip((0, 1, r.x_lim - 1, r.x_lim), (10, 20, 30, 40)):
        r.at(f"xc_{k}", 4, row, np.float32(k + 0.25), 7.5)
    for k, row in zip((0, 1, r.y_lim - 1, r.y_lim), (50, 60, 70, 80)):
        r.at(f"yc_{k}", 4, row, 10.5, np.float32(k + 0.25))
    r.at("xc_frac_0", 4, 45, np.float32(-0.5), 7.5)  # truncates to 0: dropped like 0, not like -1 (both drop; the map case)
    r.at("win_clip_0", 4, 2)
    r.at("win_clip_H", 4, 97)
    r.at("win_full", 4, 50)
    r.specials()
    r.random_pixels(150, [0, 1])
    return r


def rig_big(rng, W, H, cw, ch, n):
    r = Rig(W, H, cw, ch, rng)
    r.random_columns(range(W - 1), [1.0, 0.5, 0.1, 0.02, 0.004, 0.3][:W - 1], nan_rate=0.002)
    r.pmy[:, W - 1], r.pmx[:, W - 1] = 7.0, 400.0
    head_y, head_x = r.pmy[:r.nc, 0], r.pmx[:r.nc, 0]  # (id 0's window stays searchable)
    head_y[~np.isfinite(head_y)], head_x[~np.isfinite(head_x)] = 3.0, 30.0
    r.at("win_clip_0", W - 1, 5)
    r.at("win_clip_H", W - 1, H - 3)
    r.at("win_full", W - 1, H // 2)
    r.specials()
    r.random_pixels(n, range(W - 1))
    return r


def analyse(r, surf, floor=False):
    """per lit pixel, in plain integers: status and, when searched, (lo, hi, costs, disparities of the window)"""
    to_int = (lambda f: int(np.floor(f))) if floor else int
    out = {}
    for i, j in zip(*np.nonzero(surf > 0)):
        v = surf[i, j]
        try:
            xc, yc = to_int(r.cmx[i, j]), to_int(r.cmy[i, j])
        except (ValueError, OverflowError):
            out[i, j] = ("cam_poison",)
            continue
        if not (0 < xc < r.x_lim and 0 < yc < r.y_lim):
            out[i, j] = ("outside_rect", xc, yc)
            continue
        p = r.W * r.H * v
        if not p < r.W * r.H:
            out[i, j] = ("out_of_range",)
            continue
        idx = int(p)
        col, row = idx // r.H, idx % r.H
        lo, hi = max(row - r.nc, 0), min(row + r.nc, r.H)
        try:
            cand = [(abs(yc - to_int(r.pmy[y, col])), to_int(r.pmx[y, col]) - xc) for y in range(lo, hi)]
        except (ValueError, OverflowError):
            out[i, j] = ("poisoned", lo, hi, col)
            continue
        out[i, j] = ("searched", lo, hi, col, cand, xc, yc, idx)
    return out


def expected(rec):
    if rec[0] != "searched":
        return 0
    cost = [c for c, _ in rec[4]]
    k = cost.index(min(cost))
    return rec[4][k][1] if cost[k] <= 50 and rec[4][k][1] > 0 else 0


def check_cases(r, surf, disp, name):
    """every case the fixture exists for, found in the inputs and the reference's output"""
    seen = set()
    an = analyse(r, surf)
    for (i, j), rec in an.items():
        d = int(disp[i, j])
        assert d == expected(rec), (name, i, j, rec[0], d)
        seen.add(rec[0])
        if rec[0] == "outside_rect":
            for nm, val, lim in (("xc", rec[1], r.x_lim), ("yc", rec[2], r.y_lim)):
                if val in (0, lim):
                    seen.add(f"{nm}_at_{'0' if val == 0 else 'limit'}_dropped")
        if rec[0] != "searched":
            continue
        _, lo, hi, col, cand, xc, yc, idx = rec
        seen.add("clip_0" if lo == 0 and hi - lo < 2 * r.nc else "clip_H" if hi == r.H and hi - lo < 2 * r.nc else "full")
        if idx == 0:
            seen.add("id_0")
        for nm, val, lim in (("xc", xc, r.x_lim), ("yc", yc, r.y_lim)):
            if val in (1, lim - 1):
                seen.add(f"{nm}_at_{'1' if val == 1 else 'limit-1'}_kept")
        cost = [c for c, _ in cand]
        best = min(cost)
        k = cost.index(best)
        ties = [q for q, c in enumerate(cost) if c == best]
        if len(ties) > 1 and best <= 50:
            yps = [int(r.pmy[lo + q, col]) for q in ties]
            if yps[0] == yc - best and yc + best in yps[1:] and best > 0 and cand[ties[0]][1] != cand[ties[1]][1]:
                seen.add("minus_before_plus_tie")
        if best == 50:
            seen.add("cost_50_accepted")
            assert d == cand[k][1] > 0
        if best == 51:
            seen.add("cost_51_refused")
            assert d == 0
        if best <= 50 and any(dd > 0 for q, (_, dd) in enumerate(cand) if q != k):
            if cand[k][1] == 1:
                seen.add("winner_disp_1")
            if cand[k][1] == 0:
                seen.add("winner_disp_0_loser_positive")
            if cand[k][1] < 0:
                seen.add("winner_disp_negative_loser_positive")
        win_y = r.pmy[lo:hi, col]
        if np.any((win_y > -1) & (win_y < 0)):
            seen.add("entry_in_(-1,0)")
        col_bad = ~np.isfinite(r.pmy[:, col]) | ~np.isfinite(r.pmx[:, col])
        if col_bad.any() and not col_bad[lo:hi].any():
            seen.add("poison_outside_window")
    if np.any((r.cmx > -1) & (r.cmx < 0) & (surf > 0)):
        seen.add("cam_entry_in_(-1,0)")
    fl = analyse(r, surf, floor=True)
    if any(expected(fl[k]) != expected(an[k]) for k in an):
        seen.add("floor_would_differ")
    for tag, (i, j) in r.tags.items():
        if tag in ("v_one", "v_above_one", "v_inf"):
            assert an[i, j][0] == "out_of_range" and disp[i, j] == 0
            seen.add(tag)
        if tag == "v_last":
            assert surf[i, j] < 1 and an[i, j][0] in ("searched", "out_of_range")
            seen.add("v_last_" + an[i, j][0])
    return seen


NEED_ALL = {"searched", "outside_rect", "out_of_range", "poisoned", "cam_poison", "clip_0", "clip_H", "full", "id_0", "entry_in_(-1,0)",
            "poison_outside_window", "v_one", "v_above_one", "v_inf"}
NEED_A = NEED_ALL | {"minus_before_plus_tie", "cost_50_accepted", "cost_51_refused", "winner_disp_1", "winner_disp_0_loser_positive",
                     "winner_disp_negative_loser_positive", "xc_at_0_dropped", "xc_at_limit_dropped", "yc_at_0_dropped",
                     "yc_at_limit_dropped", "xc_at_1_kept", "xc_at_limit-1_kept", "yc_at_1_kept", "yc_at_limit-1_kept",
                     "cam_entry_in_(-1,0)", "floor_would_differ"}


def main():
    assert os.path.isdir(REF_EVAL), "needs /root/reference (build container only)"
    ref = import_reference()
    rng = np.random.default_rng(12)
    out = {}
    rigs = (("a", rig_a(rng)), ("b", rig_big(rng, 6, 990, 70, 9, 300)), ("c", rig_big(rng, 7, 1920, 45, 6, 160)))
    for name, r in rigs:
        assert (r.cw % 64 or r.ch % 4) and r.W != r.H
        s64 = r.surf64()
        s32 = r.surf
        for tag, s in (("f32", s32), ("f64", s64)):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                disp = ref.compute_disparity(s, r.cmx, r.cmy, r.pmx, r.pmy, (r.W, r.H), (3 * r.W, 3 * r.H))
            assert disp.dtype == np.float32 and np.array_equal(disp, np.rint(disp)) and 0 <= disp.min() and disp.max() <= 65535
            seen = check_cases(r, s, disp, name + tag)
            need = NEED_A if name == "a" else NEED_ALL
            assert need <= seen, (name, tag, sorted(need - seen))
            assert any(t.startswith("v_last_") for t in seen)
            out[f"{name}_surf_{tag}"], out[f"{name}_disp_{tag}"] = s, disp.astype(np.uint16)
            print(name, tag, "lit", int((s > 0).sum()), "matched", int((disp > 0).sum()), sorted(seen - NEED_ALL))
        # the float64 pixels: their float32 rounding names the next projector pixel
        wh = r.W * r.H
        for k in range(3):
            i, j = r.tags[f"f64_{k}"]
            assert int(wh * s64[i, j]) + 1 == int(np.float32(wh) * s32[i, j])
        a32, a64 = analyse(r, s32), analyse(r, s64)
        assert any(a32[r.tags[f"f64_{k}"]] != a64[r.tags[f"f64_{k}"]] for k in range(3))
        if name == "a":
            t, d = r.tags, out["a_disp_f32"]
            assert d[t["tie_minus_first"]] == 7 and d[t["cost_50"]] == 4 and d[t["cost_51"]] == 0
            assert d[t["nan_inside"]] == 0 and d[t["nan_outside"]] == 5 and d[t["nan_x_inside"]] == 0
            assert d[t["disp_1"]] == 1 and d[t["disp_0"]] == 0 and d[t["disp_neg"]] == 0
            assert d[t["trunc_not_floor"]] == 11 and d[t["trunc_negative"]] == 15
            assert d[t["xc_0"]] == 0 and d[t["xc_1"]] == 399 and d[t[f"xc_{r.x_lim - 1}"]] == 400 - (r.x_lim - 1) and d[t[f"xc_{r.x_lim}"]] == 0
            assert d[t["yc_0"]] == 0 and d[t["yc_1"]] == 390 and d[t[f"yc_{r.y_lim - 1}"]] == 390 and d[t[f"yc_{r.y_lim}"]] == 0
            assert d[t["v_last"]] == 390 and d[t["v_id0"]] == expected(analyse(r, s32)[t["v_id0"]])
            out["a_tags"] = np.array([f"{k}:{i}:{j}" for k, (i, j) in sorted(t.items())])
        out[f"{name}_cam_mapx"], out[f"{name}_cam_mapy"] = r.cmx, r.cmy
        out[f"{name}_proj_mapx"], out[f"{name}_proj_mapy"] = r.pmx, r.pmy
        out[f"{name}_proj_shape"] = np.array([r.W, r.H], np.int32)
        for tag, p03 in (("pos", 5821.0837), ("neg", -5821.0837)):
            with np.errstate(divide="ignore"):
                depth = ref.disparity_to_depth(out[f"{name}_disp_f32"].astype(np.float32), np.float64(p03))
            assert depth.dtype == np.float64 and np.all(np.isfinite(depth)) and np.all((depth == 0) == (out[f"{name}_disp_f32"] == 0))
            out[f"{name}_depth_{tag}"] = depth
            out[f"p1_03_{tag}"] = np.float64(p03)
    path = os.path.join(HERE, "g12_mc3d.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(path, size, "bytes")
    assert size < 300 * 1024


if __name__ == "__main__":
    main()
