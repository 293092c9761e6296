"""The pipelined K2's live-slot masks (x_maps_amd/csrc/host/xm_k2_live.hpp: which 16-byte quads of the column tiles' disparity
frame can ever be written; the kernel does not load the others).  Host code only, no GPU:

* tests/c_host/k2_live_host.cpp, a stand-alone program, compares the masks with a brute-force enumeration over cells on
  hand-built rigs (single live cells at an octet's first / last row, dead and full tiles, patches that stick out of the frame
  on every side, xr_min on a reachable column, sheared frames, NumPy's negative wrap, odd widths); built here with
  AddressSanitizer and UBSan and run as it is.
* the same rule restated in NumPy on the C-1M tables: the live fractions the profiles quote, and the mask's cells as a
  superset of what the oracle's disparity frame holds for dense frames."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import xmaps_oracle as O
from x_maps_amd import synthetic as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def _gxx_with_asan(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    r = subprocess.run([gxx] + FLAGS + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if r.returncode != 0 or subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("g++ without -fsanitize=address,undefined")
    return gxx


def test_masks_against_brute_force_under_address_and_ub_sanitizers(tmp_path):
    gxx = _gxx_with_asan(tmp_path)
    exe = tmp_path / "k2_live_host"
    subprocess.run([gxx] + FLAGS + [os.path.join(ROOT, "tests", "c_host", "k2_live_host.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.strip() == "ok"


def _live_cells(tb):
    """[rect_w][rect_h] bool: the cells some (row r < xmap_h - 1, time column) pair stores into (the flush of the column tiles:
    live = xp - x_offset >= the LUT's smallest rectified x; the frame column as int16 with NumPy's one negative wrap)"""
    xm = tb["proj_x_map"].astype(np.int64)
    rh, rw = tb["rect_h"], tb["rect_w"]
    xr_min = int(tb["cam_mapx_i16"].min())
    fu = xm - tb["x_offset"]
    rows = np.broadcast_to(np.arange(xm.shape[0])[:, None], xm.shape)
    ok = (fu >= xr_min) & (rows < xm.shape[0] - 1) & (rows < rh)
    fc = fu.astype(np.int16).astype(np.int64)
    fc = np.where(fc < 0, fc + rw, fc)
    ok &= (fc >= 0) & (fc < rw)
    cells = np.zeros((rw, rh), bool)
    cells[fc[ok], rows[ok]] = True
    return cells


@pytest.fixture(scope="module")
def c1m():
    tb = S.make_tables(S.C_1M)
    return tb, _live_cells(tb)


def test_live_fractions_of_the_c1m_frame(c1m):
    """profiles/r06_k1_chain.md section 4: 36 % of the cells, 41 % of the 16-byte quads, 77 % of the 128-byte lines"""
    tb, cells = c1m
    rw, rh = cells.shape
    assert (rw, rh) == (1760, 1320) and rh % 8 == 0
    quads = cells.reshape(rw, rh // 8, 8).any(axis=2).reshape(-1)
    lines = quads.reshape(-1, 8).any(axis=1)
    assert int(cells.sum()) == 833_195 and cells.size == 2_323_200, cells.sum()  # 35.86 %
    assert int(quads.sum()) == 120_112 and quads.size == 290_400, quads.sum()  # 41.36 %
    assert abs(quads.mean() - 0.41) < 0.01
    assert abs(lines.mean() - 0.7718) < 0.0005, lines.mean()  # 77.18 %


@pytest.mark.parametrize("frame", [3, 4, 11])
def test_the_live_cells_hold_every_cell_the_oracle_writes(c1m, frame):
    tb, cells = c1m
    x, y, t, _ = S.to_soa(S.make_events(S.C_1M, frame=frame))
    ref = O.process_ev_frame(tb, x.astype(np.int64), y.astype(np.int64), t, want_bgr=False)
    dm = ref["disp_map"]  # [rect_h][rect_w]
    assert dm.shape == cells.T.shape and np.count_nonzero(dm) > 250_000
    assert not np.any((dm != 0) & ~cells.T)
