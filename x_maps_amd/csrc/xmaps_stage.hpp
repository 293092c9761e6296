// xmaps_stage.hpp -- the reference's stages one at a time (rectify, event disparity, disparity maps, point cloud:
// cam_proj_calibration.py:277-317, x_maps_disparity.py:12-29, disp_to_depth.py) and the debug outputs per event.  Not on the
// fused path.  (gfx950 / MI355X)
//
// Needs xmaps_common.hpp.
#pragma once
#include "xmaps_common.hpp"

namespace xm {

// =====================================================================================================
// stage / debug kernels (reference stage signatures; not on the fused path)
// =====================================================================================================
__global__ __launch_bounds__(BLOCK) void k_stage_rectify(const uint16_t* __restrict__ xs, const uint16_t* __restrict__ ys,
                                                         u64 n, DevTables tb, int16_t* __restrict__ xr,
                                                         int16_t* __restrict__ yr, u32* __restrict__ oob_count) {
  const u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  const u32 x = xs[i], y = ys[i];
  if (x >= (u32)tb.cam_w || y >= (u32)tb.cam_h) {
    atomicAdd(oob_count, 1u);
    xr[i] = 0;
    yr[i] = 0;
    return;
  }
  const u32 l = tb.lut[x * (u32)tb.cam_h + y];
  xr[i] = (int16_t)(l & 0xffff);
  yr[i] = (int16_t)(l >> 16);
}

// CamProjMaps.rectify_cam_coords_f32 (cam_proj_calibration.py:272-275): gather from the caller's float rectify maps
// (row-major [cam_h][cam_w]); used by the offline evaluation caller (eval/compute_depth_x_maps.py:99) for the point cloud.
__global__ __launch_bounds__(BLOCK) void k_stage_rectify_f32(const uint16_t* __restrict__ xs, const uint16_t* __restrict__ ys,
                                                             u64 n, int cam_w, int cam_h, const float* __restrict__ mapx,
                                                             const float* __restrict__ mapy, float* __restrict__ xr,
                                                             float* __restrict__ yr, u32* __restrict__ oob_count) {
  const u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  const u32 x = xs[i], y = ys[i];
  if (x >= (u32)cam_w || y >= (u32)cam_h) {
    atomicAdd(oob_count, 1u);
    xr[i] = 0.f;
    yr[i] = 0.f;
    return;
  }
  const u32 o = y * (u32)cam_w + x;
  xr[i] = mapx[o];
  yr[i] = mapy[o];
}

// CamProjMaps.construct_point_cloud (cam_proj_calibration.py:319-331): [x+d, y, -d, 1] through Q in float32,
// perspective divide, y and z negated.  d == 0 gives the same inf/nan the NumPy code produces.
struct Mat4f {
  float m[16];
};
// one point (shared with the time-surface path, xmaps_surface.hpp: the same float32 operations in the same order)
__device__ inline void point_from_disparity(const Mat4f& Q, float xpr, float ypr, float d, float (&out)[3]) {
  const float p0 = xpr + d, p1 = ypr, p2 = -d;
  float r[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    float acc = Q.m[4 * k] * p0;
    acc = fmaf(Q.m[4 * k + 1], p1, acc);
    acc = fmaf(Q.m[4 * k + 2], p2, acc);
    acc = acc + Q.m[4 * k + 3];
    r[k] = acc;
  }
  out[0] = r[0] / r[3];
  out[1] = -(r[1] / r[3]);
  out[2] = -(r[2] / r[3]);
}
__global__ __launch_bounds__(BLOCK) void k_point_cloud(const float* __restrict__ xpr, const float* __restrict__ ypr,
                                                       const float* __restrict__ disp, u64 n, Mat4f Q,
                                                       float* __restrict__ cloud) {
  const u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  float p[3];
  point_from_disparity(Q, xpr[i], ypr[i], disp[i], p);
  cloud[3 * i + 0] = p[0];
  cloud[3 * i + 1] = p[1];
  cloud[3 * i + 2] = p[2];
}

// A2 on caller-supplied rectified coordinates
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_stage_event_disparity(const int16_t* __restrict__ xr,
                                                                 const int16_t* __restrict__ yr, const T* __restrict__ ts,
                                                                 u64 n, DevTables tb, const SlotState* st, u32 tag,
                                                                 int16_t* __restrict__ disp, uint8_t* __restrict__ mask) {
  u64 lo, hi;
  load_frame_minmax(st, tag & 1, lo, hi);
  const TimeNorm<T> tn(TimeCodec<T>::dec(lo), TimeCodec<T>::dec(hi), tb.t_px_scale);
  const u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  const int x = xr[i], y = yr[i];
  int d = 0;
  bool ok = y >= 0 && y < tb.xmap_h - 1;
  if (ok) {
    const int col = tn.column(ts[i]);
    const int xp = (int)tb.xmap[col * tb.xmap_h + y];
    d = (int)(short)(xp - x - tb.x_offset);
    ok = d >= 0;
  }
  disp[i] = (int16_t)(ok ? d : 0);
  mask[i] = ok ? 1 : 0;
}

// A3 / A3' on caller-supplied per-event arrays (full length + mask)
template <int VIEW>
__global__ __launch_bounds__(BLOCK) void k_stage_scatter(const int16_t* __restrict__ xr, const int16_t* __restrict__ yr,
                                                         const uint16_t* __restrict__ xs, const uint16_t* __restrict__ ys,
                                                         const int16_t* __restrict__ disp, const uint8_t* __restrict__ mask,
                                                         u64 n, DevTables tb, u32 tag, u64* __restrict__ frame,
                                                         u32* __restrict__ oob_count) {
  const u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n || !mask[i]) return;
  u32 cell;
  const int d = disp[i];
  if constexpr (VIEW == 0) {
    int col = (int)(short)(xr[i] + d);
    const int row = yr[i];
    if (col < 0) col += tb.rect_w;
    int r = row;
    if (r < 0) r += tb.rect_h;  // stage API: arbitrary caller arrays, NumPy index rules
    if (col < 0 || col >= tb.rect_w || r < 0 || r >= tb.rect_h) {
      atomicAdd(oob_count, 1u);
      return;
    }
    cell = (u32)r * (u32)tb.rect_w + (u32)col;
  } else {
    const u32 x = xs[i], y = ys[i];
    if (x >= (u32)tb.cam_w || y >= (u32)tb.cam_h) {
      atomicAdd(oob_count, 1u);
      return;
    }
    cell = y * (u32)tb.cam_w + x;
  }
  // the stage frame stores the f32 value of the int16 disparity; negative values never pass the mask
  // in the reference's pipeline, but keep the low 16 bits faithfully and sign-extend on decode
  const u64 key = ((u64)tag << KEY_TAG_SHIFT) | (i << KEY_IDX_SHIFT) | (u64)(u32)(uint16_t)d;
  __hip_atomic_fetch_max(&frame[cell], key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(BLOCK) void k_decode_keys_signed(const u64* __restrict__ f, u64 n_cells, u32 tag,
                                                              float* __restrict__ out) {
  const u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x;
  if (i < n_cells) {
    const u64 k = f[i];
    out[i] = (u32)(k >> KEY_TAG_SHIFT) == tag ? (float)(int)(short)(k & 0xffff) : 0.0f;
  }
}

// every intermediate of A1/A2 per event (tests)
template <typename T, bool HAS_P>
__global__ __launch_bounds__(BLOCK) void k_debug_events(const uint16_t* __restrict__ xs, const uint16_t* __restrict__ ys,
                                                        const T* __restrict__ ts, const int16_t* __restrict__ ps, u64 n,
                                                        DevTables tb, const SlotState* st, u32 tag,
                                                        int16_t* __restrict__ xr, int16_t* __restrict__ yr,
                                                        int16_t* __restrict__ tcol, int16_t* __restrict__ disp,
                                                        uint8_t* __restrict__ mask) {
  u64 lo, hi;
  load_frame_minmax(st, tag & 1, lo, hi);
  const TimeNorm<T> tn(TimeCodec<T>::dec(lo), TimeCodec<T>::dec(hi), tb.t_px_scale);
  const u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  bool oob;
  const bool used = !HAS_P || ps[i] == 1;
  const EventResult r = event_disparity<T>(tb, tn, xs[i], ys[i], ts[i], used, oob);
  if (xr) xr[i] = (int16_t)r.xr;
  if (yr) yr[i] = (int16_t)r.yr;
  if (tcol) tcol[i] = (int16_t)r.ts;
  if (disp) disp[i] = (int16_t)r.disp;
  if (mask) mask[i] = r.inlier ? 1 : 0;
}

}  // namespace xm
