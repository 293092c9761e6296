// xmaps_rigmaps.hpp -- a rig's rectification maps at setup time: x_maps_amd/calibration.py's init_undistort_rectify_map,
// init_undistort_rectify_map_inverse, mapf_to_i16 and remap_nearest (with esl_init._pair_i16 and the linear projector time map
// of proj_time_map.py / esl_init.get_projector_time_surface), one thread per pixel.  (gfx950 / MI355X)
//
// PINNED to the project's NumPy, bit for bit -- not to OpenCV ("map rounding unpinned against cv2" stands).
// The arithmetic is float64 and every expression is evaluated as NumPy evaluates it: operators associate left to right, a product
// of scalars is formed first (2 * p1 * x * y is ((2 p1) x) y), the radial polynomial is 1 + r2 (k1 + r2 (k2 + r2 k3)), every
// quotient is one IEEE division (the only reciprocal is icdist = 1.0 / (...), where NumPy takes one), the rotation is the three
// sums R[i,0] x + R[i,1] y + R[i,2], and nothing is fused: the library is built with -ffp-contract=off and there is no fma here.
// rintf is round-half-to-even (v_rndne_f32), np.rint's rule; the float32 cast rounds to nearest even like .astype(np.float32).
//
// No atomics, no block that waits for another; every output is one store per pixel, consecutive threads to consecutive addresses.
//
// Map values far outside every image are ordinary (a 1/8-scale rig with strong distortion reaches 1.6e9, rims fold over into
// inf / NaN): an index is only formed from a value that has been compared, as a float, against the image first.
//   constant border : an entry is inside iff 0 <= rint(v) <= size - 1 in float32; NaN, +-inf and anything beyond int32 fail that
//                     comparison and take the border value -- what NumPy's int64 comparison gives for every finite value.
//   replicate border: rint(v) is clamped to [0, size - 1] by sign; NaN goes to the first row / column.  NumPy's own result for
//                     NaN, +-inf and values beyond int64 is UNDEFINED there (a float -> int64 cast out of range); finite values
//                     within int64 agree.
//
// Needs xmaps_common.hpp (BLOCK and the integer typedefs only).
#pragma once
#include "xmaps_common.hpp"

namespace xm {

constexpr int RIG_SRC_NONE = 0, RIG_SRC_IMAGE = 1, RIG_SRC_LINEAR_TIME = 2;  // = XM_RIG_SRC_* of include/xmaps.h

struct RigCam {  // K's four scalars, the Brown model's five
  double fx, fy, cx, cy, k1, k2, p1, p2, k3;
};

struct RigFwdArgs {
  int w, h;       // the target frame
  double ir[9];   // inv(P[:3,:3] @ R), from the host
  RigCam c;
  const float* mapx_in;  // both given: the map is read, not computed (calibration.remap_nearest on a caller's map)
  const float* mapy_in;
  float* mapx;    // every output is nullable
  float* mapy;
  u32* pair;      // interleaved int16 (x, y), saturated like esl_init._pair_i16
  float* remap;   // the nearest-neighbour sample of the source through the map
  const float* src;  // RIG_SRC_IMAGE: [src_h][src_w]
  int src_kind, src_w, src_h, replicate, scan_upwards;
  float border_value;
};

struct RigInvArgs {
  int w, h;  // the source frame
  RigCam c;
  int iterate;  // any distortion coefficient != 0: the five fixed-point rounds (without them the same bits, NumPy skips them too)
  double R[9];
  double p00, p11, p02, p12;
  float* mapx;  // every output is nullable
  float* mapy;
  int16_t* mapx_i16;  // mapf_to_i16
  int16_t* mapy_i16;
  u32* pair;          // interleaved int16 (x, y): the layout of disp_proj_mapxy_i16
  u32* flags;         // [2]: an x / a y entry outside int16 (mapf_to_i16's assertion); every offender stores the same 1
};

// esl_init._pair_i16's saturation: NaN -> -32768, +-inf and everything out of range clipped, then rint
__device__ __forceinline__ u32 rig_sat_i16(float m) {
  float s = m != m ? -32768.0f : m;
  s = s < -32768.0f ? -32768.0f : s;
  s = s > 32767.0f ? 32767.0f : s;
  return (u32)(uint16_t)(int16_t)(int)rintf(s);
}

// the gathered index along one axis of `size` cells (size <= 2^24: size - 1 is a float32); false = outside (constant border only)
__device__ __forceinline__ bool rig_index(float m, int size, bool replicate, int& idx) {
  const float r = rintf(m), last = (float)(size - 1);
  if (replicate) {
    idx = !(r > 0.0f) ? 0 : (r >= last ? size - 1 : (int)r);  // (NaN fails r > 0: the first cell)
    return true;
  }
  const bool ok = r >= 0.0f && r <= last;
  idx = ok ? (int)r : 0;
  return ok;
}

__global__ __launch_bounds__(BLOCK) void k_rig_forward_map(const RigFwdArgs a) {
  const u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= (u64)a.w * (u64)a.h) return;
  float mx, my;
  if (a.mapx_in) {
    mx = a.mapx_in[i];
    my = a.mapy_in[i];
  } else {
    const u32 vi = (u32)(i / (u32)a.w), ui = (u32)(i - (u64)vi * (u32)a.w);
    const double u = (double)ui, v = (double)vi;
    double x = a.ir[0] * u + a.ir[1] * v + a.ir[2];
    double y = a.ir[3] * u + a.ir[4] * v + a.ir[5];
    const double wz = a.ir[6] * u + a.ir[7] * v + a.ir[8];
    x = x / wz;
    y = y / wz;
    // distort_normalized
    const double r2 = x * x + y * y;
    const double radial = 1.0 + r2 * (a.c.k1 + r2 * (a.c.k2 + r2 * a.c.k3));
    const double xd = x * radial + 2.0 * a.c.p1 * x * y + a.c.p2 * (r2 + 2.0 * x * x);
    const double yd = y * radial + a.c.p1 * (r2 + 2.0 * y * y) + 2.0 * a.c.p2 * x * y;
    mx = (float)(a.c.fx * xd + a.c.cx);
    my = (float)(a.c.fy * yd + a.c.cy);
  }
  if (a.mapx) a.mapx[i] = mx;
  if (a.mapy) a.mapy[i] = my;
  if (a.pair) a.pair[i] = rig_sat_i16(mx) | (rig_sat_i16(my) << 16);
  if (a.remap) {
    int ix, iy;
    const bool okx = rig_index(mx, a.src_w, a.replicate != 0, ix), oky = rig_index(my, a.src_h, a.replicate != 0, iy);
    float val = a.border_value;
    if (okx && oky) {
      if (a.src_kind == RIG_SRC_LINEAR_TIME) {  // generate_linear_projector_time_map at the gathered pixel: no table
        const int row = a.scan_upwards ? a.src_h - 1 - iy : iy;
        val = (float)((double)((long long)ix * a.src_h + row) / (double)((long long)a.src_w * a.src_h));
      } else {
        val = a.src[(size_t)iy * (size_t)a.src_w + (size_t)ix];
      }
    }
    a.remap[i] = val;
  }
}

__global__ __launch_bounds__(BLOCK) void k_rig_inverse_map(const RigInvArgs a) {
  const u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= (u64)a.w * (u64)a.h) return;
  const u32 vi = (u32)(i / (u32)a.w), ui = (u32)(i - (u64)vi * (u32)a.w);
  // undistort_points on the float32 pixel coordinate
  const double px = (double)(float)ui, py = (double)(float)vi;
  const double x0 = (px - a.c.cx) / a.c.fx;
  const double y0 = (py - a.c.cy) / a.c.fy;
  double x = x0, y = y0;
  if (a.iterate) {
    for (int it = 0; it < 5; ++it) {
      const double r2 = x * x + y * y;
      const double icdist = 1.0 / (1.0 + r2 * (a.c.k1 + r2 * (a.c.k2 + r2 * a.c.k3)));
      const double dx = 2.0 * a.c.p1 * x * y + a.c.p2 * (r2 + 2.0 * x * x);
      const double dy = a.c.p1 * (r2 + 2.0 * y * y) + 2.0 * a.c.p2 * x * y;
      x = (x0 - dx) * icdist;
      y = (y0 - dy) * icdist;
    }
  }
  const double xr = a.R[0] * x + a.R[1] * y + a.R[2];
  const double yr = a.R[3] * x + a.R[4] * y + a.R[5];
  const double wr = a.R[6] * x + a.R[7] * y + a.R[8];
  x = xr / wr;
  y = yr / wr;
  const float mx = (float)(a.p00 * x + a.p02);
  const float my = (float)(a.p11 * y + a.p12);
  if (a.mapx) a.mapx[i] = mx;
  if (a.mapy) a.mapy[i] = my;
  if (a.mapx_i16 || a.mapy_i16 || a.pair) {
    const float rx = rintf(mx), ry = rintf(my);
    const bool okx = rx >= -32768.0f && rx <= 32767.0f, oky = ry >= -32768.0f && ry <= 32767.0f;  // (a NaN fails, as in mapf_to_i16)
    if (!okx) a.flags[0] = 1u;
    if (!oky) a.flags[1] = 1u;
    const int16_t sx = okx ? (int16_t)(int)rx : (int16_t)0, sy = oky ? (int16_t)(int)ry : (int16_t)0;
    if (a.mapx_i16) a.mapx_i16[i] = sx;
    if (a.mapy_i16) a.mapy_i16[i] = sy;
    if (a.pair) a.pair[i] = (u32)(uint16_t)sx | ((u32)(uint16_t)sy << 16);
  }
}

}  // namespace xm
