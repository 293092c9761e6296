// xm_api_evaltable.hpp -- C-ABI: the evaluation table's scorer (the ground truth and every method's depth maps of a sequence ->
// the cells of the reference's Table 1: python/eval/create_evaluation_table.py:121-163 around esl_utilities.py:153-175)
// (part of libxmaps_hip.so's host side: included by ../xmaps_hip.hip, one translation unit; see that file for the order)
// The kernels and the arithmetic: ../xmaps_evaltable.hpp.  No xm_handle: the object owns its device, stream, staging and scratch.
#pragma once

static_assert(sizeof(xm_eval_sums) == sizeof(EvalAcc) && offsetof(xm_eval_sums, n10) == offsetof(EvalAcc, n10),
              "xm_eval_sums is what k_evt_fold writes");

struct xm_eval_table : GroupObj {
  int W = 0, H = 0;
  float min_d = 0, max_d = 0;
  u32 n_tiles = 0, tiles_x = 0, tiles_y = 0;  // flat tiles of EVT_TILE pixels; the median's EVT_MW x EVT_MH blocks
  DevBuf mean, one_sec;                       // [stacks][px] before the median; the 1-sec maps behind it
  DevBuf msum, mcnt, avg;                     // the median's partials; avg_depth per stack
  DevBuf p1_sum, p1_cnt, p2_sum, p2_cnt, sums;
  DevBuf in_gt, in_est[EVT_MAX_METHODS], mask;  // staging of XM_MEM_HOST calls (mask: also the scratch of a call that does not ask for it)
  std::vector<EvalAcc> h_sums;
};

namespace {

// 16-byte loads: the maps of a stack follow each other px pixels apart
bool evt_vec(const xm_eval_table* e, std::initializer_list<const void*> ptrs) {
  if (e->px % 4) return false;
  for (const void* p : ptrs)
    if (p && !aligned(p, 16)) return false;
  return true;
}

// combine + median of `n_stacks` stacks of n_maps maps each -> comb0 (stack 0), e->one_sec (the others), e->avg
void evt_launch_combine(xm_eval_table* e, bool vec, const EvtStacks& st, u32 n_stacks, u32 n_maps, float* d_mean, float* comb0) {
  hipStream_t stream = e->stream;
  const dim3 g_flat(e->n_tiles, n_stacks);
  if (vec) hipLaunchKernelGGL((k_evt_combine<true>), g_flat, dim3(BLOCK), 0, stream, st, n_maps, e->px, e->min_d, e->max_d, d_mean);
  else hipLaunchKernelGGL((k_evt_combine<false>), g_flat, dim3(BLOCK), 0, stream, st, n_maps, e->px, e->min_d, e->max_d, d_mean);
  hipLaunchKernelGGL(k_evt_median, dim3(e->tiles_x, e->tiles_y, n_stacks), dim3(BLOCK), 0, stream, (const float*)d_mean, e->W, e->H, comb0,
                     (float*)e->one_sec.p, (double*)e->msum.p, (u32*)e->mcnt.p);
  hipLaunchKernelGGL(k_evt_avg, dim3(n_stacks), dim3(BLOCK), 0, stream, (const double*)e->msum.p, (const u32*)e->mcnt.p,
                     (int)(e->tiles_x * e->tiles_y), (double*)e->avg.p);
}

}  // namespace

extern "C" {

void xm_eval_table_destroy(xm_eval_table* e) { group_destroy(e); }

int xm_eval_table_create(int device, const xm_eval_table_config* cfg, xm_eval_table** out) {
  if (int rc = group_create_args(cfg, out, "xm_eval_table_config")) return rc;
  if (cfg->height <= 0 || cfg->width <= 0) return fail(XM_ERR_INVALID, "dimensions must be positive");
  const u32 tiles_x = grid_for((u64)cfg->width, EVT_MW), tiles_y = grid_for((u64)cfg->height, EVT_MH);
  if (tiles_y > 65535) return fail(XM_ERR_INVALID, "maps too tall (at most %d rows)", 65535 * EVT_MH);
  Owned<xm_eval_table, xm_eval_table_destroy> e;
  if (int rc = group_open(device, e)) return rc;
  e->W = cfg->width, e->H = cfg->height;
  e->min_d = cfg->min_depth, e->max_d = cfg->max_depth;
  e->px = (size_t)cfg->width * (size_t)cfg->height;
  e->noun = "maps";
  e->n_tiles = grid_for(e->px, EVT_TILE), e->tiles_x = tiles_x, e->tiles_y = tiles_y;
  *out = e.release();
  return XM_OK;
}

int xm_eval_table_combine(xm_eval_table* e, const float* maps, int n_maps, int mem, float* combined_out, float* mean_out,
                          double* avg_depth_out) {
  if (int rc = group_enter(e, n_maps, mem)) return rc;
  if (!maps) return fail(XM_ERR_INVALID, "NULL argument");
  const size_t px = e->px, n_mt = (size_t)e->tiles_x * e->tiles_y;
  GroupCall c{e->stream, mem == XM_MEM_HOST};
  EvtStacks st{};
  st.p[0] = c.in(e->in_gt, maps, (size_t)n_maps * px * 4);
  float* d_mean = c.out(e->mean, mean_out, px * 4, true);
  float* d_comb = c.out(e->mask, combined_out, px * 4, true);
  if (int rc = c.start({{e->msum, n_mt * 8}, {e->mcnt, n_mt * 4}, {e->avg, 8}})) return rc;
  evt_launch_combine(e, evt_vec(e, {st.p[0], d_mean, d_comb}), st, 1, (u32)n_maps, d_mean, d_comb);
  HIP_TRY(hipGetLastError());
  c.back_host(avg_depth_out, e->avg.p, 8);
  return c.finish();
}

int xm_eval_table_score(xm_eval_table* e, const float* gt, const float* const* est, int n_methods, uint32_t one_sec_mask, int n_scans,
                        int mem, xm_eval_result* results_out, xm_eval_sums* sums_out, float* mask_out, double* avg_depth_out) {
  if (int rc = group_enter(e, n_scans, mem)) return rc;
  if (!gt || !est) return fail(XM_ERR_INVALID, "NULL argument");
  if (n_methods < 1 || n_methods > EVT_MAX_METHODS) return fail(XM_ERR_INVALID, "n_methods must lie in 1 .. %d", EVT_MAX_METHODS);
  if (one_sec_mask >> n_methods) return fail(XM_ERR_INVALID, "one_sec_mask names a method beyond n_methods");
  for (int m = 0; m < n_methods; ++m)
    if (!est[m]) return fail(XM_ERR_INVALID, "NULL estimate stack");
  const size_t px = e->px, S = (size_t)n_scans, n_tiles = e->n_tiles, n_mt = (size_t)e->tiles_x * e->tiles_y;
  u32 n_one = 0;
  for (int m = 0; m < n_methods; ++m) n_one += (one_sec_mask >> m) & 1u;
  const size_t R = (size_t)n_methods + n_one, G = 1 + (size_t)n_one;
  try {
    e->h_sums.resize(R * S);
  } catch (const std::bad_alloc&) {
    return fail(XM_ERR_NOMEM, "out of host memory");
  }
  hipStream_t stream = e->stream;
  GroupCall c{stream, mem == XM_MEM_HOST};
  const float* d_gt = c.in(e->in_gt, gt, S * px * 4);
  const float* d_est[EVT_MAX_METHODS] = {};
  for (int m = 0; m < n_methods; ++m) d_est[m] = c.in(e->in_est[m], est[m], S * px * 4);
  float* d_mask = c.out(e->mask, mask_out, px * 4, true);
  if (int rc = c.start({{e->mean, G * px * 4}, {e->one_sec, n_one * px * 4}, {e->msum, G * n_mt * 8}, {e->mcnt, G * n_mt * 4}, {e->avg, G * 8},
                        {e->p1_sum, S * n_tiles * 8}, {e->p1_cnt, S * EVT_P1_CNT * n_tiles * 4}, {e->p2_sum, R * S * n_tiles * 8},
                        {e->p2_cnt, R * S * EVT_P2_CNT * n_tiles * 4}, {e->sums, R * S * sizeof(EvalAcc)}}))
    return rc;
  // the stacks to combine: the ground truth, then the methods with a 1-sec row; the rows: methods 0 .. M-1, then the 1-sec rows by ascending m
  EvtStacks st{};
  EvtRows rows{};
  st.p[0] = d_gt;
  rows.n_rows = (u32)R;
  u32 k = 0;
  for (int m = 0; m < n_methods; ++m) {
    rows.est[m] = d_est[m];
    if ((one_sec_mask >> m) & 1u) {
      st.p[1 + k] = d_est[m];
      rows.est[n_methods + k] = (const float*)e->one_sec.p + (size_t)k * px;
      rows.one_sec |= 1u << (n_methods + k);
      ++k;
    }
  }
  bool vec = evt_vec(e, {d_gt, d_mask});
  for (int m = 0; m < n_methods; ++m) vec = vec && evt_vec(e, {d_est[m]});
  evt_launch_combine(e, vec, st, (u32)G, (u32)S, (float*)e->mean.p, d_mask);
  double* p1_sum = (double*)e->p1_sum.p;
  double* p2_sum = (double*)e->p2_sum.p;
  u32* p1_cnt = (u32*)e->p1_cnt.p;
  u32* p2_cnt = (u32*)e->p2_cnt.p;
  const dim3 g_flat((unsigned)n_tiles, (unsigned)S);
  if (vec) {
    hipLaunchKernelGGL((k_evt_pass1<true>), g_flat, dim3(BLOCK), 0, stream, d_gt, (const float*)d_mask, px, e->min_d, e->max_d, p1_sum, p1_cnt);
    hipLaunchKernelGGL((k_evt_pass2<true>), g_flat, dim3(BLOCK), 0, stream, d_gt, (const float*)d_mask, rows, px, e->min_d, e->max_d,
                       (const double*)p1_sum, (const u32*)p1_cnt, p2_sum, p2_cnt);
  } else {
    hipLaunchKernelGGL((k_evt_pass1<false>), g_flat, dim3(BLOCK), 0, stream, d_gt, (const float*)d_mask, px, e->min_d, e->max_d, p1_sum, p1_cnt);
    hipLaunchKernelGGL((k_evt_pass2<false>), g_flat, dim3(BLOCK), 0, stream, d_gt, (const float*)d_mask, rows, px, e->min_d, e->max_d,
                       (const double*)p1_sum, (const u32*)p1_cnt, p2_sum, p2_cnt);
  }
  hipLaunchKernelGGL(k_evt_fold, dim3((unsigned)(R * S)), dim3(BLOCK), 0, stream, (const double*)p1_sum, (const u32*)p1_cnt,
                     (const double*)p2_sum, (const u32*)p2_cnt, (u32)S, (int)n_tiles, (EvalAcc*)e->sums.p);
  HIP_TRY(hipGetLastError());
  c.back_host(e->h_sums.data(), e->sums.p, R * S * sizeof(EvalAcc));
  c.back_host(avg_depth_out, e->avg.p, 8);
  if (int rc = c.finish()) return rc;
  for (size_t i = 0; i < R * S; ++i) {
    if (results_out) eval_result_from_sums(e->h_sums[i], (double)px, &results_out[i]);
    if (sums_out) memcpy(&sums_out[i], &e->h_sums[i], sizeof(EvalAcc));
  }
  return XM_OK;
}

}  // extern "C"
