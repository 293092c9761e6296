"""-m gpu: ONE object of each group kind (ESL-init, MC3D, ESL depth optimisation, ESL filters; the shared host skeleton is
csrc/host/xm_group.hpp) through growth, both memory kinds and a refused call, in this order:

  1. a group of 1 from host memory, every optional output given;
  2. a group of 3 from host memory: every scratch and staging buffer grows;
  3. a refused call (n = 0): XM_ERR_INVALID, and the object stays good;
  4. the group of 1 again through XM_MEM_DEVICE pointers (torch tensors), every optional output given;
  5. the same with every optional output NULL (the statistics are one of them: 5b gives them alone).

Main outputs and statistics of 1, 4 and 5 are bit-equal, 2's first map is bit-equal to 1, and every map is held against the
object's *_ref.py restatement by the comparison its own test file uses: equality of bits for the three integer / float32 objects,
max(1000 x the CPU's numpy-vs-fsum difference, 1e-12) for the filter's float64 stage.  Outputs are pre-filled with 0xFF bytes (NaN
in a float, 0xFFFF in a u16), so an unwritten element shows.

The gap this closes: the objects' own test files cover each of these separately -- groups of several sizes on fresh objects, the
device path, the refused calls -- but never growth and then a smaller group, nor both memory kinds, on ONE object, which is where
a staging pointer left over from an earlier call would show.

Shapes are the smallest the *_cases.py files have: MC3D's rig "a" (37 x 13 camera), the 37 x 13 ESL-init rig, the seeded 20 x 15
ESL-optim rig; the filter takes scenes one pixel wider and taller than its bilateral tile (33 x 9) with 2 x 2 iterations: 60
launches."""
import ctypes as C
import os
import re

import numpy as np
import pytest

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Out:
    def __init__(self, name, dtype, shape=None, optional=False):
        self.name, self.dtype, self.shape, self.optional = name, np.dtype(dtype), shape, optional


class EslInitCase:
    entry, stats_t = "xm_esl_init_time_surfaces", "xm_esl_init_stats"
    outs = (Out("depth", np.float32), Out("disp", np.uint16, optional=True))

    def __init__(self, golden_dir):
        import esl_init_cases as K
        import esl_init_ref as R
        self.rig, self.p1_03 = K.make_rig(), 812.25
        self.surfaces = K.make_surfaces(self.rig, 3, np.float32)
        self.want = [R.depth_init_fused(s, self.rig["cam_to_rect"], self.rig["rect_to_cam"], self.rig["proj_rect"], self.p1_03)
                     for s in self.surfaces]

    def open(self):
        from x_maps_amd.esl_init import EslInit
        r = self.rig
        return EslInit({"cam_w": r["cam_w"], "cam_h": r["cam_h"], "rect_w": r["rect_w"], "rect_h": r["rect_h"], "cam_to_rect_map": r["cam_to_rect"],
                        "rect_to_cam_map": r["rect_to_cam"], "proj_rect": r["proj_rect"], "p1_03": self.p1_03})

    def inputs(self, n):
        return [self.surfaces[:n]]

    def args(self, N, ins, n, mem, outs, stats):
        return (ins[0], N.XM_T_FLOAT32, n, mem, outs["depth"], outs["disp"], stats)

    def check(self, i, got, st):
        w_depth, w_disp, w_st = self.want[i]
        assert np.array_equal(got["depth"].view(np.uint32), w_depth.view(np.uint32)), i
        if got["disp"] is not None:
            assert np.array_equal(got["disp"], w_disp), i
        if st is not None:
            assert {k: getattr(st, k) for k in w_st} == w_st, (i, w_st)


class Mc3dCase:
    entry, stats_t = "xm_mc3d_time_surfaces", "xm_mc3d_stats"
    outs = (Out("depth", np.float32), Out("disp", np.uint16, optional=True))

    def __init__(self, golden_dir):
        import mc3d_cases as K
        import mc3d_ref as R
        from x_maps_amd.mc3d import mc3d_int_maps
        self.K, self.R = K, R
        self.rig = K.load_rigs(golden_dir, mc3d_int_maps)["a"]
        self.surfaces = K.group(self.rig, np.float32, 3)
        self.want = [R.mc3d(s, self.rig["cam_map"], self.rig["proj_map"], K.P1_03[0]) for s in self.surfaces]

    def open(self):
        from x_maps_amd.mc3d import Mc3d
        return Mc3d(self.K.tables(self.rig, self.K.P1_03[0]))

    def inputs(self, n):
        return [self.surfaces[:n]]

    def args(self, N, ins, n, mem, outs, stats):
        return (ins[0], N.XM_T_FLOAT32, n, mem, 0, outs["depth"], outs["disp"], stats)

    def check(self, i, got, st):
        w_depth, w_disp, w_st = self.want[i]
        depth = got["depth"]
        assert np.array_equal(depth.view(np.uint32), w_depth.view(np.uint32)) and np.all(np.isfinite(depth)), i
        if got["disp"] is not None:
            assert np.array_equal(got["disp"], w_disp) and np.all((depth == 0) == (got["disp"] == 0)), i
        if st is not None:
            assert {k: getattr(st, k) for k in self.R.STAT_KEYS} == w_st, (i, w_st)


class EslOptimCase:
    entry, stats_t = "xm_esl_optim_time_surfaces", "xm_esl_optim_stats"
    outs = (Out("depth", np.float32), Out("nfev", np.uint16, optional=True))

    def __init__(self, golden_dir):
        import esl_optim_cases as K
        import esl_optim_ref as R
        self.K, self.R = K, R
        self.rig = K.make_rig(20, 15, 40, 64, 41)
        self.surfaces = K.group(self.rig, np.float32, 3)
        self.d0 = np.ascontiguousarray(np.broadcast_to(self.rig["depth_init"], self.surfaces.shape), dtype=np.float32)
        rr = K.ref_rig(self.rig)
        self.want = [R.depth_optim(rr, s, self.rig["depth_init"]) for s in self.surfaces]

    def open(self):
        from x_maps_amd.esl_optim import EslOptim
        return EslOptim(self.K.tables(self.rig))

    def inputs(self, n):
        return [self.surfaces[:n], self.d0[:n]]

    def args(self, N, ins, n, mem, outs, stats):
        return (ins[0], N.XM_T_FLOAT32, n, mem, ins[1], outs["depth"], outs["nfev"], stats)

    def check(self, i, got, st):
        w_depth, w_nfev, w_st = self.want[i]
        assert not np.isnan(got["depth"]).any() and np.array_equal(got["depth"].view(np.uint32), w_depth.view(np.uint32)), i
        if got["nfev"] is not None:
            assert np.array_equal(got["nfev"], w_nfev), i
        if st is not None:
            assert {k: getattr(st, k) for k in self.R.STAT_KEYS} == w_st, (i, w_st)


class EslFilterCase:
    entry, stats_t = "xm_esl_filter_maps", "xm_esl_filter_stats"
    PARAMS = dict(niter_outer=2, niter_inner=2)
    outs = (Out("filtered", np.float64), Out("bilateral", np.float32, optional=True), Out("trips", np.uint8, (4,), optional=True))

    def __init__(self, golden_dir):
        import esl_filter_cases as K
        import esl_filter_ref as R
        geo = open(os.path.join(ROOT, "x_maps_amd", "csrc", "xmaps_geometry.hpp")).read()
        m = re.search(r"constexpr int BLOCK = (\d+);", geo), re.search(r"constexpr int ESLF_BW = (\d+), ESLF_BH = BLOCK / ESLF_BW,", geo)
        bw = int(m[1][1])
        self.W, self.H = bw + 1, int(m[0][1]) // bw + 1  # one pixel wider and taller than a bilateral tile
        self.maps = np.ascontiguousarray(np.stack([K.scene(self.H, self.W, 190), K.zero_map(self.H, self.W), K.scene(self.H, self.W, 191)]))
        self.want = []
        for img in self.maps:  # the restatement and the CPU's own summation-order difference: the bound of tests/test_gpu_esl_filter.py
            out, bil, info = R.esl_filter(img, **self.PARAMS)
            out_fsum, _, info_fsum = R.esl_filter(img, norm=R.norm_fsum, **self.PARAMS)
            assert np.array_equal(info["trips"], info_fsum["trips"])
            self.want.append((out, bil, info, max(1000.0 * float(np.abs(out - out_fsum).max()), 1e-12)))

    def open(self):
        from x_maps_amd.esl_filter import EslFilter
        return EslFilter(self.W, self.H, **self.PARAMS)

    def inputs(self, n):
        return [self.maps[:n]]

    def args(self, N, ins, n, mem, outs, stats):
        return (ins[0], n, mem, outs["filtered"], outs["bilateral"], outs["trips"], stats)

    def check(self, i, got, st):
        w_out, w_bil, info, bound = self.want[i]
        diff = float(np.abs(got["filtered"] - w_out).max())
        print(f"filter map {i}: max |gpu - ref| = {diff:.3e}, bound = {bound:.3e}")
        assert not np.isnan(got["filtered"]).any() and diff <= bound, (i, diff, bound)
        if got["bilateral"] is not None:
            assert np.array_equal(got["bilateral"].view(np.uint32), w_bil.view(np.uint32)), i
        if got["trips"] is not None:
            assert np.array_equal(got["trips"], info["trips"]), i
        if st is not None:
            img = self.maps[i]
            assert (st.n_outer, st.n_lsqr, st.sum_itn) == (info["n_outer"], info["n_lsqr"], info["sum_itn"])
            assert list(st.istop_count) == list(info["istop_count"]) and st.lo == float(img.min()) and st.hi == float(img.max())
            assert abs(st.final_norm - info["final_norm"]) <= 2.0 * np.sqrt(img.size) * bound + 1e-12 * info["final_norm"]


CASES = {"esl_init": EslInitCase, "mc3d": Mc3dCase, "esl_optim": EslOptimCase, "esl_filter": EslFilterCase}


def call(case, obj, n, mem, optional=True, stats=True):
    """one raw call of the C entry on pre-filled outputs -> (return code, {name: array | None}, [stats struct] | None)"""
    import torch
    from x_maps_amd import _native as N
    stats_t = getattr(N, case.stats_t)
    device = mem == N.XM_MEM_DEVICE
    keep, ptrs = [], []

    def place(a):  # -> the pointer the call gets; keep[] holds what owns the memory
        a = np.ascontiguousarray(a)
        keep.append(torch.from_numpy(a.view(np.uint8).reshape(-1)).cuda() if device else a)
        return keep[-1].data_ptr() if device else a.ctypes.data

    ins = [place(a) for a in case.inputs(max(n, 1))]
    rows = max(n, 1)
    shapes = {o.name: (rows,) + (o.shape or case.inputs(1)[0].shape[1:]) for o in case.outs}
    outs = {}
    for o in case.outs:
        given = optional or not o.optional
        outs[o.name] = place(np.full(int(np.prod(shapes[o.name])) * o.dtype.itemsize, 0xFF, np.uint8)) if given else None
        ptrs.append(len(keep) - 1 if given else None)
    st_ptr = place(np.full(rows * C.sizeof(stats_t), 0xFF, np.uint8)) if stats else None
    st_at = len(keep) - 1
    if device:
        torch.cuda.synchronize()
    rc = getattr(obj._lib, case.entry)(obj._h, *case.args(N, ins, n, mem, outs, st_ptr))
    raw = lambda k: keep[k].cpu().numpy() if device else keep[k].view(np.uint8).reshape(-1)
    got = {o.name: None if k is None else raw(k).view(o.dtype).reshape(shapes[o.name]) for o, k in zip(case.outs, ptrs)}
    st = [stats_t.from_buffer_copy(raw(st_at)[i * C.sizeof(stats_t):(i + 1) * C.sizeof(stats_t)].tobytes()) for i in range(rows)] if stats else None
    return rc, got, st


def bits(a):
    return None if a is None else np.ascontiguousarray(a).view(np.uint8).tobytes()


@gpu
@pytest.mark.parametrize("kind", list(CASES))
def test_one_object_through_growth_both_memory_kinds_and_a_refused_call(kind, golden_dir):
    from x_maps_amd import _native as N
    case = CASES[kind](golden_dir)
    main = case.outs[0].name
    with case.open() as obj:
        rc1, got1, st1 = call(case, obj, 1, N.XM_MEM_HOST)
        rc2, got2, st2 = call(case, obj, 3, N.XM_MEM_HOST)
        rc3, _, _ = call(case, obj, 0, N.XM_MEM_HOST)
        assert rc3 == N.XM_ERR_INVALID and "must be positive" in N.last_error()
        rc4, got4, st4 = call(case, obj, 1, N.XM_MEM_DEVICE)
        rc5, got5, st5 = call(case, obj, 1, N.XM_MEM_DEVICE, optional=False, stats=False)
        rc5b, got5b, st5b = call(case, obj, 1, N.XM_MEM_DEVICE, optional=False)
    assert (rc1, rc2, rc4, rc5, rc5b) == (N.XM_OK,) * 5
    assert st5 is None and all(got5[o.name] is None for o in case.outs if o.optional)
    for i in range(3):
        case.check(i, {k: v[i] for k, v in got2.items()}, st2[i])
    for got, st in ((got1, st1), (got4, st4), (got5, None), (got5b, st5b)):
        case.check(0, {k: None if v is None else v[0] for k, v in got.items()}, None if st is None else st[0])
        assert bits(got[main]) == bits(got1[main]) == bits(got2[main][:1])
        if st is not None:
            assert bytes(st[0]) == bytes(st1[0]) == bytes(st2[0])
    for o in case.outs[1:]:  # the optional maps: host, group and device agree wherever they were asked for
        assert bits(got1[o.name]) == bits(got4[o.name]) == bits(got2[o.name][:1])
