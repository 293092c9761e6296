// xm_api_timecal.hpp -- C-ABI: the projector time-map calibration (camera time surfaces of a white frame -> the projector-space time map)
// (part of libxmaps_hip.so's host side: included by ../xmaps_hip.hip, one translation unit; see that file for the order)
// The kernels and the arithmetic (this build's definition): ../xmaps_timecal.hpp.  A group object (xm_group.hpp) whose accumulators
// live in device memory between calls.  The corner verdict is host code on four integer points.
#pragma once

struct xm_timecal : GroupObj {
  Event ev[8];             // HIP events around the launches of a call (xm_res.hpp's rule: declared before the buffers)
  float kernel_ms[6] = {0, 0, 0, 0, 0, 0};  // T0 .. T5 of the last call that ran them: xm_timecal_kernel_ms
  int w = 0, h = 0;
  bool has_mean = false;
  xm_timecal_stats last{};  // counters as of the last add, the mean's part as of the last mean
  DevMem<double> d_sum, d_mean;
  DevMem<u32> d_cnt;
  DevMem<uint8_t> d_valid;
  DevMem<TcalCounts> d_counts;
  DevMem<TcalAcc> d_acc;
  DevBuf part1, value, next_r;  // device-side intermediates
  DevBuf in, map, present;      // staging of XM_MEM_HOST calls
};

namespace {

// the time between events a and a + 1 into kernel_ms[k], after the stream has been synchronised
void timecal_elapsed(xm_timecal* tc, int a, int k) {
  float t = 0.0f;
  tc->kernel_ms[k] = hipEventElapsedTime(&t, tc->ev[a], tc->ev[a + 1]) == hipSuccess ? t : 0.0f;
}

int timecal_clear(xm_timecal* tc) {
  HIP_TRY(hipMemsetAsync(tc->d_sum, 0, tc->px * sizeof(double), tc->stream));
  HIP_TRY(hipMemsetAsync(tc->d_cnt, 0, tc->px * sizeof(u32), tc->stream));
  HIP_TRY(hipMemsetAsync(tc->d_counts, 0, sizeof(TcalCounts), tc->stream));
  HIP_TRY(hipStreamSynchronize(tc->stream));
  tc->has_mean = false;
  tc->last = xm_timecal_stats{};
  return XM_OK;
}

// TL -> TR -> BR -> BL: distinct and strictly convex (integer cross products of consecutive edges, all of one sign)
int timecal_corner_verdict(const xm_timecal_stats& st) {
  if (st.n_core == 0) return fail(XM_ERR_INVALID, "xm_timecal_mean: no core pixel (no valid pixel has a valid 3 x 3 neighbourhood)");
  for (int a = 0; a < 4; ++a)
    for (int b = a + 1; b < 4; ++b)
      if (st.corners[a][0] == st.corners[b][0] && st.corners[a][1] == st.corners[b][1])
        return fail(XM_ERR_INVALID, "xm_timecal_mean: two corners coincide at (%d, %d)", st.corners[a][0], st.corners[a][1]);
  int n_pos = 0, n_neg = 0;
  for (int k = 0; k < 4; ++k) {
    const int32_t* p = st.corners[k];
    const int32_t* q = st.corners[(k + 1) & 3];
    const int32_t* r = st.corners[(k + 2) & 3];
    const long long cross = (long long)(q[0] - p[0]) * (r[1] - q[1]) - (long long)(q[1] - p[1]) * (r[0] - q[0]);
    n_pos += cross > 0, n_neg += cross < 0;
  }
  if (n_pos != 4 && n_neg != 4) return fail(XM_ERR_INVALID, "xm_timecal_mean: the corner quadrilateral is not strictly convex");
  return XM_OK;
}

// T3 on the object's mask, the stats' mean part, the outputs back, then the verdict
int timecal_corners(xm_timecal* tc, GroupCall& c, double* mean_out, uint8_t* valid_out, xm_timecal_stats* stats) {
  hipStream_t stream = tc->stream;
  HIP_TRY(hipMemsetAsync(tc->d_acc, 0xff, sizeof(u64) * 4, stream));
  HIP_TRY(hipMemsetAsync((char*)tc->d_acc.get() + sizeof(u64) * 4, 0, sizeof(TcalAcc) - sizeof(u64) * 4, stream));
  HIP_TRY(hipEventRecord(tc->ev[2], stream));
  hipLaunchKernelGGL(k_tcal_corners, dim3(grid_for(tc->px, BLOCK)), dim3(BLOCK), 0, stream, (const uint8_t*)tc->d_valid, tc->w, tc->h,
                     tc->d_acc.get());
  HIP_TRY(hipEventRecord(tc->ev[3], stream));
  HIP_TRY(hipGetLastError());
  TcalAcc acc{};
  c.back_host(&acc, tc->d_acc, sizeof acc);
  c.back(mean_out, tc->d_mean, tc->px * sizeof(double));
  c.back(valid_out, tc->d_valid, tc->px);
  if (int rc = c.finish()) return rc;
  timecal_elapsed(tc, 2, 3);
  tc->has_mean = true;
  xm_timecal_stats& st = tc->last;
  st.n_valid = acc.n_valid, st.n_core = acc.n_core, st.n_missing = st.n_unfilled = 0;
  for (int k = 0; k < 4; ++k) {
    const bool any = acc.key[k] != TCAL_NO_KEY;
    const u32 i = (u32)acc.key[k];
    st.corners[k][0] = any ? (int32_t)(i % (u32)tc->w) : -1;
    st.corners[k][1] = any ? (int32_t)(i / (u32)tc->w) : -1;
  }
  if (stats) *stats = st;
  return timecal_corner_verdict(st);
}

}  // namespace

extern "C" {

void xm_timecal_destroy(xm_timecal* tc) { group_destroy(tc); }

int xm_timecal_create(int device, int cam_width, int cam_height, xm_timecal** out) {
  if (!out) return fail(XM_ERR_INVALID, "NULL argument");
  *out = nullptr;
  if (cam_width <= 0 || cam_height <= 0) return fail(XM_ERR_INVALID, "dimensions must be positive");
  if ((u64)cam_width * (u64)cam_height >= (1ull << 31)) return fail(XM_ERR_INVALID, "camera frame too large");
  Owned<xm_timecal, xm_timecal_destroy> tc;
  if (int rc = group_open(device, tc)) return rc;
  tc->w = cam_width, tc->h = cam_height;
  tc->px = (size_t)cam_width * (size_t)cam_height;
  HIP_TRY(tc->d_sum.alloc(tc->px));
  HIP_TRY(tc->d_mean.alloc(tc->px));
  HIP_TRY(tc->d_cnt.alloc(tc->px));
  HIP_TRY(tc->d_valid.alloc(tc->px));
  HIP_TRY(tc->d_counts.alloc(1));
  HIP_TRY(tc->d_acc.alloc(1));
  for (Event& e : tc->ev) HIP_TRY(e.create(hipEventDefault));
  if (int rc = timecal_clear(tc.get())) return rc;
  *out = tc.release();
  return XM_OK;
}

int xm_timecal_reset(xm_timecal* tc) {
  if (int rc = group_enter(tc, 1, XM_MEM_HOST)) return rc;
  return timecal_clear(tc);
}

int xm_timecal_counts(xm_timecal* tc, uint64_t* n_added, uint64_t* n_skipped) {
  if (!tc) return fail(XM_ERR_INVALID, "NULL object");
  if (n_added) *n_added = tc->last.n_added;
  if (n_skipped) *n_skipped = tc->last.n_skipped;
  return XM_OK;
}

int xm_timecal_kernel_ms(xm_timecal* tc, float ms[6]) {
  if (!tc || !ms) return fail(XM_ERR_INVALID, "NULL argument");
  for (int k = 0; k < 6; ++k) ms[k] = tc->kernel_ms[k];
  return XM_OK;
}

int xm_timecal_add_surfaces(xm_timecal* tc, const void* surfaces, int dtype, int n, int mem) {
  if (int rc = group_enter(tc, n, mem, &dtype)) return rc;
  if (!surfaces) return fail(XM_ERR_INVALID, "NULL argument");
  const size_t ns = (size_t)n, px = tc->px;
  const u32 nb = grid_for(px, SURF_RED_CHUNK);
  hipStream_t stream = tc->stream;
  GroupCall c{stream, mem == XM_MEM_HOST};
  const void* d_in = c.in(tc->in, surfaces, ns * px * t_size(dtype));
  if (int rc = c.start({{tc->part1, ns * nb * sizeof(SurfPart1)}})) return rc;
  SurfPart1* p1 = (SurfPart1*)tc->part1.p;
  HIP_TRY(hipEventRecord(tc->ev[0], stream));
  by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((k_surf_extrema<T>), dim3(nb, (unsigned)ns), dim3(BLOCK), 0, stream, (const T*)d_in, (u32)px, p1);
    (void)hipEventRecord(tc->ev[1], stream);
    hipLaunchKernelGGL((k_tcal_accumulate<T>), dim3(nb), dim3(BLOCK), 0, stream, (const T*)d_in, (u32)px, (u32)ns, (const SurfPart1*)p1,
                       tc->d_sum.get(), tc->d_cnt.get(), tc->d_counts.get());
  });
  HIP_TRY(hipEventRecord(tc->ev[2], stream));
  HIP_TRY(hipGetLastError());
  TcalCounts counts{};
  c.back_host(&counts, tc->d_counts, sizeof counts);
  if (int rc = c.finish()) return rc;
  timecal_elapsed(tc, 0, 0), timecal_elapsed(tc, 1, 1);
  tc->last.n_added = counts.n_added, tc->last.n_skipped = counts.n_skipped;
  return XM_OK;
}

int xm_timecal_mean(xm_timecal* tc, uint32_t min_count, double* mean_out, uint8_t* valid_out, int mem, xm_timecal_stats* stats) {
  if (int rc = group_enter(tc, 1, mem)) return rc;
  if (min_count == 0) return fail(XM_ERR_INVALID, "min_count must be at least 1");
  GroupCall c{tc->stream, mem == XM_MEM_HOST};
  tc->has_mean = false;
  HIP_TRY(hipEventRecord(tc->ev[0], tc->stream));
  hipLaunchKernelGGL(k_tcal_mean, dim3(grid_for(tc->px, BLOCK)), dim3(BLOCK), 0, tc->stream, (const double*)tc->d_sum, (const u32*)tc->d_cnt,
                     (u32)tc->px, (u32)min_count, tc->d_mean.get(), tc->d_valid.get());
  HIP_TRY(hipEventRecord(tc->ev[1], tc->stream));
  HIP_TRY(hipGetLastError());
  const int rc = timecal_corners(tc, c, mean_out, valid_out, stats);
  if (tc->has_mean) timecal_elapsed(tc, 0, 2);
  return rc;
}

int xm_timecal_set_mean(xm_timecal* tc, const double* mean, const uint8_t* valid, int mem, xm_timecal_stats* stats) {
  if (int rc = group_enter(tc, 1, mem)) return rc;
  if (!mean || !valid) return fail(XM_ERR_INVALID, "NULL argument");
  GroupCall c{tc->stream, mem == XM_MEM_HOST};
  tc->has_mean = false;
  const hipMemcpyKind kind = c.host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
  if (int rc = c.copy(tc->d_mean, mean, tc->px * sizeof(double), kind)) return rc;
  if (int rc = c.copy(tc->d_valid, valid, tc->px, kind)) return (void)hipStreamSynchronize(tc->stream), rc;
  return timecal_corners(tc, c, nullptr, nullptr, stats);
}

int xm_timecal_warp(xm_timecal* tc, const double h[9], int proj_width, int proj_height, float* time_map_out, uint8_t* present_out,
                    int mem, xm_timecal_stats* stats) {
  if (int rc = group_enter(tc, 1, mem)) return rc;
  if (!h || !time_map_out) return fail(XM_ERR_INVALID, "NULL argument");
  if (!tc->has_mean) return fail(XM_ERR_INVALID, "xm_timecal_warp: no mean yet (xm_timecal_mean comes first)");
  if (proj_width <= 0 || proj_height <= 0 || proj_width > (1 << 24) || proj_height > (1 << 24))
    return fail(XM_ERR_INVALID, "the projector's sides must lie in 1 .. 2^24");
  const size_t n = (size_t)proj_width * (size_t)proj_height;
  if (n >= (1ull << 31)) return fail(XM_ERR_INVALID, "the projector frame must hold fewer than 2^31 pixels");
  hipStream_t stream = tc->stream;
  GroupCall c{stream, mem == XM_MEM_HOST};
  float* d_map = c.out(tc->map, time_map_out, n * 4);
  uint8_t* d_present = c.out(tc->present, present_out, n, true);
  if (int rc = c.start({{tc->value, n * sizeof(double)}, {tc->next_r, n * sizeof(int)}})) return rc;
  TcalAcc* acc = tc->d_acc;
  HIP_TRY(hipMemsetAsync(&acc->n_missing, 0, 2 * sizeof(u32), stream));
  TcalWarpArgs a{};
  for (int i = 0; i < 9; ++i) a.h[i] = h[i];
  a.cam_w = tc->w, a.cam_h = tc->h, a.proj_w = proj_width, a.proj_h = proj_height;
  a.mean = tc->d_mean, a.valid = tc->d_valid;
  a.value = (double*)tc->value.p, a.present = d_present, a.acc = acc;
  HIP_TRY(hipEventRecord(tc->ev[4], stream));
  hipLaunchKernelGGL(k_tcal_warp, dim3(grid_for(n, BLOCK)), dim3(BLOCK), 0, stream, a);
  HIP_TRY(hipEventRecord(tc->ev[5], stream));
  hipLaunchKernelGGL(k_tcal_fill, dim3((unsigned)proj_height), dim3(BLOCK), 0, stream, (const double*)a.value, (const uint8_t*)d_present,
                     proj_width, (int*)tc->next_r.p, d_map, acc);
  HIP_TRY(hipEventRecord(tc->ev[6], stream));
  HIP_TRY(hipGetLastError());
  TcalAcc got{};
  c.back_host(&got, acc, sizeof got);
  if (int rc = c.finish()) return rc;
  timecal_elapsed(tc, 4, 4), timecal_elapsed(tc, 5, 5);
  tc->last.n_missing = got.n_missing, tc->last.n_unfilled = got.n_unfilled;
  if (stats) *stats = tc->last;
  return XM_OK;
}

}  // extern "C"
