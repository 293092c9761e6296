// xm_api_rigmaps.hpp -- C-ABI: a rig's rectification maps, time map and X-map on the device (calibration.py's NumPy, bit for bit)
// (part of libxmaps_hip.so's host side: included by ../xmaps_hip.hip, one translation unit; see that file for the order)
// The kernels and the arithmetic: ../xmaps_rigmaps.hpp.  No xm_handle: device-ordinal entries like xm_build_x_map, synchronous,
// on the null stream; every buffer lives for one call.
#pragma once

namespace {

// one output of a call: the caller's device pointer, or a device buffer of the call's own that goes back to the caller's host pointer
struct RigOut {
  DevMem<unsigned char> own;
  void* dev = nullptr;
  void* host = nullptr;
  size_t bytes = 0;
  hipError_t open(void* user, size_t n, bool host_mem) {
    bytes = n;
    if (!user) return hipSuccess;
    if (!host_mem) return dev = user, hipSuccess;
    host = user;
    const hipError_t e = own.alloc(n);
    dev = own.p;
    return e;
  }
  hipError_t back() const { return host ? hipMemcpy(host, dev, bytes, hipMemcpyDeviceToHost) : hipSuccess; }
  template <typename T>
  T* as() const { return static_cast<T*>(dev); }
};

// an input: the caller's device pointer, or an upload of the caller's host array
struct RigIn {
  DevMem<unsigned char> own;
  const void* dev = nullptr;
  hipError_t open(const void* user, size_t n, bool host_mem) {
    if (!user) return hipSuccess;
    if (!host_mem) return dev = user, hipSuccess;
    hipError_t e = own.alloc(n);
    if (e == hipSuccess) e = hipMemcpy(own.p, user, n, hipMemcpyHostToDevice);
    dev = own.p;
    return e;
  }
};

// the kernel's time between two events on the null stream
struct RigTimer {
  Event a, b;
  hipError_t start() {
    hipError_t e;
    if ((e = a.create(hipEventDefault)) != hipSuccess || (e = b.create(hipEventDefault)) != hipSuccess) return e;
    return hipEventRecord(a, 0);
  }
  hipError_t stop() { return hipEventRecord(b, 0); }
  float ms() const {  // after the device has been synchronised
    float t = 0.0f;
    return a && b && hipEventElapsedTime(&t, a, b) == hipSuccess ? t : 0.0f;
  }
};

int rig_open_device(int device) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(XM_ERR_HIP, "no HIP device visible");
  HIP_TRY(hipSetDevice(device));
  return XM_OK;
}

RigCam rig_cam(const double* K, const double* D) { return RigCam{K[0], K[1], K[2], K[3], D[0], D[1], D[2], D[3], D[4]}; }

bool rig_frame_ok(int w, int h) { return w > 0 && h > 0 && (u64)w * (u64)h < (1ull << 31); }

void rig_launch_forward(const RigFwdArgs& a) {
  hipLaunchKernelGGL(k_rig_forward_map, dim3(grid_for((u64)a.w * (u64)a.h, BLOCK)), dim3(BLOCK), 0, 0, a);
}

RigInvArgs rig_inv_args(int w, int h, const double* K, const double* D, const double* R, const double* P, u32* flags) {
  RigInvArgs a{};
  a.w = w, a.h = h;
  a.c = rig_cam(K, D);
  for (int i = 0; i < 5; ++i) a.iterate |= D[i] != 0.0;
  for (int i = 0; i < 9; ++i) a.R[i] = R[i];
  a.p00 = P[0], a.p11 = P[1], a.p02 = P[2], a.p12 = P[3];
  a.flags = flags;
  return a;
}

void rig_launch_inverse(const RigInvArgs& a) {
  hipLaunchKernelGGL(k_rig_inverse_map, dim3(grid_for((u64)a.w * (u64)a.h, BLOCK)), dim3(BLOCK), 0, 0, a);
}

// mapf_to_i16's assertion, from the kernel's flag words
int rig_i16_verdict(const char* entry, const char* whose, const u32* flags) {
  if (!flags[0] && !flags[1]) return XM_OK;
  return fail(XM_ERR_INVALID, "%s: %s inverse %s has entries outside int16 (mapf_to_i16)", entry, whose,
              flags[0] && flags[1] ? "mapx and mapy" : flags[0] ? "mapx" : "mapy");
}

}  // namespace

extern "C" {

int xm_rig_forward_map(int device, const xm_rig_forward_config* cfg, xm_rig_forward_outputs* out, int mem) {
  if (!cfg || !out) return fail(XM_ERR_INVALID, "NULL argument");
  if (cfg->struct_size != sizeof(xm_rig_forward_config)) return fail(XM_ERR_INVALID, "xm_rig_forward_config: struct_size mismatch");
  if (mem != XM_MEM_HOST && mem != XM_MEM_DEVICE) return fail(XM_ERR_INVALID, "mem must be XM_MEM_HOST or XM_MEM_DEVICE");
  if (!rig_frame_ok(cfg->width, cfg->height)) return fail(XM_ERR_INVALID, "the frame must be positive and hold fewer than 2^31 pixels");
  if (!out->mapx && !out->mapy && !out->pair_i16 && !out->remap) return fail(XM_ERR_INVALID, "no output asked for");
  if (!cfg->mapx_in != !cfg->mapy_in) return fail(XM_ERR_INVALID, "mapx_in and mapy_in come together");
  if (cfg->border != XM_RIG_BORDER_CONSTANT && cfg->border != XM_RIG_BORDER_REPLICATE) return fail(XM_ERR_INVALID, "unknown border");
  if (out->remap) {
    if (cfg->src_kind != XM_RIG_SRC_IMAGE && cfg->src_kind != XM_RIG_SRC_LINEAR_TIME) return fail(XM_ERR_INVALID, "remap needs a source");
    if (cfg->src_width <= 0 || cfg->src_height <= 0 || cfg->src_width > (1 << 24) || cfg->src_height > (1 << 24))
      return fail(XM_ERR_INVALID, "the source's sides must lie in 1 .. 2^24");
    if (cfg->src_kind == XM_RIG_SRC_IMAGE && !cfg->src) return fail(XM_ERR_INVALID, "NULL source image");
  }
  const bool host = mem == XM_MEM_HOST;
  if (!host && out->pair_i16 && !aligned(out->pair_i16, 4)) return fail(XM_ERR_INVALID, "pair_i16 must be 4-byte aligned");
  if (int rc = rig_open_device(device)) return rc;
  const size_t px = (size_t)cfg->width * (size_t)cfg->height;
  const bool image = out->remap && cfg->src_kind == XM_RIG_SRC_IMAGE;
  RigOut o_mx, o_my, o_pair, o_remap;
  RigIn i_src, i_mx, i_my;
  hipError_t e;
  if ((e = o_mx.open(out->mapx, px * 4, host)) != hipSuccess || (e = o_my.open(out->mapy, px * 4, host)) != hipSuccess ||
      (e = o_pair.open(out->pair_i16, px * 4, host)) != hipSuccess || (e = o_remap.open(out->remap, px * 4, host)) != hipSuccess ||
      (e = i_src.open(image ? cfg->src : nullptr, (size_t)cfg->src_width * (size_t)cfg->src_height * 4, host)) != hipSuccess ||
      (e = i_mx.open(cfg->mapx_in, px * 4, host)) != hipSuccess || (e = i_my.open(cfg->mapy_in, px * 4, host)) != hipSuccess) {
    return fail(XM_ERR_HIP, "xm_rig_forward_map: %s", hipGetErrorString(e));
  }
  RigFwdArgs a{};
  a.w = cfg->width, a.h = cfg->height;
  for (int i = 0; i < 9; ++i) a.ir[i] = cfg->ir[i];
  a.c = rig_cam(cfg->K, cfg->D);
  a.mapx_in = (const float*)i_mx.dev, a.mapy_in = (const float*)i_my.dev;
  a.mapx = o_mx.as<float>(), a.mapy = o_my.as<float>(), a.pair = o_pair.as<u32>(), a.remap = o_remap.as<float>();
  a.src = (const float*)i_src.dev;
  a.src_kind = out->remap ? cfg->src_kind : RIG_SRC_NONE;
  a.src_w = cfg->src_width, a.src_h = cfg->src_height;
  a.replicate = cfg->border == XM_RIG_BORDER_REPLICATE, a.scan_upwards = cfg->scan_upwards != 0;
  a.border_value = cfg->border_value;
  RigTimer tm;
  if ((e = tm.start()) != hipSuccess) return fail(XM_ERR_HIP, "xm_rig_forward_map: %s", hipGetErrorString(e));
  rig_launch_forward(a);
  if ((e = hipGetLastError()) != hipSuccess || (e = tm.stop()) != hipSuccess || (e = hipDeviceSynchronize()) != hipSuccess ||
      (e = o_mx.back()) != hipSuccess || (e = o_my.back()) != hipSuccess || (e = o_pair.back()) != hipSuccess ||
      (e = o_remap.back()) != hipSuccess) {
    return fail(XM_ERR_HIP, "xm_rig_forward_map: %s", hipGetErrorString(e));
  }
  out->kernel_ms = tm.ms();
  return XM_OK;
}

int xm_rig_inverse_map(int device, const xm_rig_inverse_config* cfg, xm_rig_inverse_outputs* out, int mem) {
  if (!cfg || !out) return fail(XM_ERR_INVALID, "NULL argument");
  if (cfg->struct_size != sizeof(xm_rig_inverse_config)) return fail(XM_ERR_INVALID, "xm_rig_inverse_config: struct_size mismatch");
  if (mem != XM_MEM_HOST && mem != XM_MEM_DEVICE) return fail(XM_ERR_INVALID, "mem must be XM_MEM_HOST or XM_MEM_DEVICE");
  if (!rig_frame_ok(cfg->width, cfg->height)) return fail(XM_ERR_INVALID, "the frame must be positive and hold fewer than 2^31 pixels");
  if (!out->mapx && !out->mapy && !out->mapx_i16 && !out->mapy_i16 && !out->pair_i16) return fail(XM_ERR_INVALID, "no output asked for");
  const bool host = mem == XM_MEM_HOST;
  if (!host && out->pair_i16 && !aligned(out->pair_i16, 4)) return fail(XM_ERR_INVALID, "pair_i16 must be 4-byte aligned");
  if (int rc = rig_open_device(device)) return rc;
  const size_t px = (size_t)cfg->width * (size_t)cfg->height;
  RigOut o_mx, o_my, o_ix, o_iy, o_pair;
  DevMem<u32> d_flags;
  u32 flags[2] = {0, 0};
  hipError_t e;
  if ((e = o_mx.open(out->mapx, px * 4, host)) != hipSuccess || (e = o_my.open(out->mapy, px * 4, host)) != hipSuccess ||
      (e = o_ix.open(out->mapx_i16, px * 2, host)) != hipSuccess || (e = o_iy.open(out->mapy_i16, px * 2, host)) != hipSuccess ||
      (e = o_pair.open(out->pair_i16, px * 4, host)) != hipSuccess || (e = d_flags.alloc(2)) != hipSuccess ||
      (e = hipMemset(d_flags, 0, sizeof flags)) != hipSuccess) {
    return fail(XM_ERR_HIP, "xm_rig_inverse_map: %s", hipGetErrorString(e));
  }
  RigInvArgs a = rig_inv_args(cfg->width, cfg->height, cfg->K, cfg->D, cfg->R, cfg->P, d_flags);
  a.mapx = o_mx.as<float>(), a.mapy = o_my.as<float>();
  a.mapx_i16 = o_ix.as<int16_t>(), a.mapy_i16 = o_iy.as<int16_t>(), a.pair = o_pair.as<u32>();
  RigTimer tm;
  if ((e = tm.start()) != hipSuccess) return fail(XM_ERR_HIP, "xm_rig_inverse_map: %s", hipGetErrorString(e));
  rig_launch_inverse(a);
  if ((e = hipGetLastError()) != hipSuccess || (e = tm.stop()) != hipSuccess || (e = hipDeviceSynchronize()) != hipSuccess ||
      (e = hipMemcpy(flags, d_flags, sizeof flags, hipMemcpyDeviceToHost)) != hipSuccess) {
    return fail(XM_ERR_HIP, "xm_rig_inverse_map: %s", hipGetErrorString(e));
  }
  out->kernel_ms = tm.ms();
  if (int rc = rig_i16_verdict("xm_rig_inverse_map", "the", flags)) return rc;
  if ((e = o_mx.back()) != hipSuccess || (e = o_my.back()) != hipSuccess || (e = o_ix.back()) != hipSuccess ||
      (e = o_iy.back()) != hipSuccess || (e = o_pair.back()) != hipSuccess) {
    return fail(XM_ERR_HIP, "xm_rig_inverse_map: %s", hipGetErrorString(e));
  }
  return XM_OK;
}

int xm_rig_build_xmaps_tables(int device, const xm_rig_tables_config* cfg, xm_rig_tables_outputs* out) {
  if (!cfg || !out) return fail(XM_ERR_INVALID, "NULL argument");
  if (cfg->struct_size != sizeof(xm_rig_tables_config)) return fail(XM_ERR_INVALID, "xm_rig_tables_config: struct_size mismatch");
  if (!out->time_map_rect || !out->x_map || !out->cam_mapx_f32 || !out->cam_mapy_f32 || !out->cam_mapx_i16 || !out->cam_mapy_i16 ||
      !out->proj_mapxy_i16)
    return fail(XM_ERR_INVALID, "NULL output");
  if (!rig_frame_ok(cfg->cam_width, cfg->cam_height) || !rig_frame_ok(cfg->proj_width, cfg->proj_height) ||
      !rig_frame_ok(cfg->rect_width, cfg->rect_height))
    return fail(XM_ERR_INVALID, "every frame must be positive and hold fewer than 2^31 pixels");
  if (cfg->proj_width > (1 << 24) || cfg->proj_height > (1 << 24)) return fail(XM_ERR_INVALID, "the projector's sides must lie in 1 .. 2^24");
  if (cfg->border != XM_RIG_BORDER_CONSTANT && cfg->border != XM_RIG_BORDER_REPLICATE) return fail(XM_ERR_INVALID, "unknown border");
  if (int rc = x_map_check(true, cfg->rect_height, cfg->rect_width, cfg->x_map_width, cfg->t_px_scale, cfg->x_offset, cfg->num_scanlines))
    return rc;
  if (int rc = rig_open_device(device)) return rc;
  const size_t n_rect = (size_t)cfg->rect_width * (size_t)cfg->rect_height, n_x = (size_t)cfg->rect_height * (size_t)cfg->x_map_width;
  const size_t n_cam = (size_t)cfg->cam_width * (size_t)cfg->cam_height, n_proj = (size_t)cfg->proj_width * (size_t)cfg->proj_height;
  DevMem<float> d_tm, d_cx, d_cy;
  DevMem<int16_t> d_x, d_cix, d_ciy;
  DevMem<u32> d_pp, d_flags;  // (flags: [0..1] the camera's, [2..3] the projector's)
  u32 flags[4] = {0, 0, 0, 0};
  hipError_t e;
  if ((e = d_tm.alloc(n_rect)) != hipSuccess || (e = d_x.alloc(n_x)) != hipSuccess || (e = d_cx.alloc(n_cam)) != hipSuccess ||
      (e = d_cy.alloc(n_cam)) != hipSuccess || (e = d_cix.alloc(n_cam)) != hipSuccess || (e = d_ciy.alloc(n_cam)) != hipSuccess ||
      (e = d_pp.alloc(n_proj)) != hipSuccess || (e = d_flags.alloc(4)) != hipSuccess ||
      (e = hipMemset(d_flags, 0, sizeof flags)) != hipSuccess) {
    return fail(XM_ERR_HIP, "xm_rig_build_xmaps_tables: %s", hipGetErrorString(e));
  }
  RigTimer t_fwd, t_x, t_cam, t_proj;
  if (cfg->time_map_rect_in) {  // ProjectorTimeMap.from_file: uploaded as xm_build_x_map uploads it
    if ((e = hipMemcpy(d_tm, cfg->time_map_rect_in, n_rect * 4, hipMemcpyHostToDevice)) != hipSuccess)
      return fail(XM_ERR_HIP, "xm_rig_build_xmaps_tables: %s", hipGetErrorString(e));
  } else {  // ProjectorTimeMap.from_calib: the projector's forward map, the linear time map sampled through it; neither is stored
    RigFwdArgs a{};
    a.w = cfg->rect_width, a.h = cfg->rect_height;
    for (int i = 0; i < 9; ++i) a.ir[i] = cfg->proj_ir[i];
    a.c = rig_cam(cfg->proj_K, cfg->proj_fwd_D);
    a.remap = d_tm;
    a.src_kind = RIG_SRC_LINEAR_TIME, a.src_w = cfg->proj_width, a.src_h = cfg->proj_height;
    a.replicate = cfg->border == XM_RIG_BORDER_REPLICATE, a.scan_upwards = cfg->scan_upwards != 0;
    a.border_value = 0.0f;
    if ((e = t_fwd.start()) != hipSuccess) return fail(XM_ERR_HIP, "xm_rig_build_xmaps_tables: %s", hipGetErrorString(e));
    rig_launch_forward(a);
    if ((e = t_fwd.stop()) != hipSuccess) return fail(XM_ERR_HIP, "xm_rig_build_xmaps_tables: %s", hipGetErrorString(e));
  }
  if ((e = t_x.start()) != hipSuccess) return fail(XM_ERR_HIP, "xm_rig_build_xmaps_tables: %s", hipGetErrorString(e));
  if (int rc = x_map_launch(d_tm, cfg->rect_height, cfg->rect_width, cfg->x_map_width, cfg->t_px_scale, cfg->x_offset, cfg->num_scanlines,
                            d_x, nullptr))
    return rc;
  RigInvArgs ca = rig_inv_args(cfg->cam_width, cfg->cam_height, cfg->cam_K, cfg->cam_D, cfg->cam_R, cfg->cam_P, d_flags.p);
  ca.mapx = d_cx, ca.mapy = d_cy, ca.mapx_i16 = d_cix, ca.mapy_i16 = d_ciy;
  RigInvArgs pa = rig_inv_args(cfg->proj_width, cfg->proj_height, cfg->proj_K, cfg->proj_D, cfg->proj_R, cfg->proj_P, d_flags.p + 2);
  pa.pair = d_pp;
  if ((e = t_x.stop()) != hipSuccess || (e = t_cam.start()) != hipSuccess) return fail(XM_ERR_HIP, "xm_rig_build_xmaps_tables: %s", hipGetErrorString(e));
  rig_launch_inverse(ca);
  if ((e = t_cam.stop()) != hipSuccess || (e = t_proj.start()) != hipSuccess) return fail(XM_ERR_HIP, "xm_rig_build_xmaps_tables: %s", hipGetErrorString(e));
  rig_launch_inverse(pa);
  if ((e = t_proj.stop()) != hipSuccess || (e = hipGetLastError()) != hipSuccess || (e = hipDeviceSynchronize()) != hipSuccess ||
      (e = hipMemcpy(flags, d_flags, sizeof flags, hipMemcpyDeviceToHost)) != hipSuccess) {
    return fail(XM_ERR_HIP, "xm_rig_build_xmaps_tables: %s", hipGetErrorString(e));
  }
  out->kernel_ms[0] = t_fwd.ms(), out->kernel_ms[1] = t_x.ms(), out->kernel_ms[2] = t_cam.ms(), out->kernel_ms[3] = t_proj.ms();
  if (int rc = rig_i16_verdict("xm_rig_build_xmaps_tables", "the camera's", flags)) return rc;
  if (int rc = rig_i16_verdict("xm_rig_build_xmaps_tables", "the projector's", flags + 2)) return rc;
  if ((e = hipMemcpy(out->time_map_rect, d_tm, n_rect * 4, hipMemcpyDeviceToHost)) != hipSuccess ||
      (e = hipMemcpy(out->x_map, d_x, n_x * 2, hipMemcpyDeviceToHost)) != hipSuccess ||
      (e = hipMemcpy(out->cam_mapx_f32, d_cx, n_cam * 4, hipMemcpyDeviceToHost)) != hipSuccess ||
      (e = hipMemcpy(out->cam_mapy_f32, d_cy, n_cam * 4, hipMemcpyDeviceToHost)) != hipSuccess ||
      (e = hipMemcpy(out->cam_mapx_i16, d_cix, n_cam * 2, hipMemcpyDeviceToHost)) != hipSuccess ||
      (e = hipMemcpy(out->cam_mapy_i16, d_ciy, n_cam * 2, hipMemcpyDeviceToHost)) != hipSuccess ||
      (e = hipMemcpy(out->proj_mapxy_i16, d_pp, n_proj * 4, hipMemcpyDeviceToHost)) != hipSuccess) {
    return fail(XM_ERR_HIP, "xm_rig_build_xmaps_tables: %s", hipGetErrorString(e));
  }
  return XM_OK;
}

}  // extern "C"
