// xm_api_sharded.hpp -- C-ABI: one frame sharded by event index over several GPUs of ONE process (last row:
// xm_create_sharded owning the RCCL communicators; 8(e): the partitioning and the exchange)
// (part of libxmaps_hip.so's host side: included by ../xmaps_hip.hip, one translation unit; see that file for the order)
//
//   device g owns events [g N / W, (g + 1) N / W) of the frame; tables are replicated (one xm_handle per device).
//   per frame, one host thread per device, everything on that device's stream, in three steps (sharded_frame_on):
//     1. the shard's way to the device and the buffers of the exchange;
//     2. the exchange (xm_shard_peers.hpp: shard_exchange_keys, or shard_exchange_columns for time-sorted int64 frames on rigs
//        whose X-map is injective; a frame one of whose pieces objects is redone with the keys: xm_sharded_stats);
//     3. device 0, the only one to ask for the frame: depth / BGR and the extrema back to the host; the columns' verdict.
//   (x_maps_amd/sharded.py is the same exchange for multi-process hosts on torch.distributed.)
// How a device thread reaches its peers -- RCCL, the agreement in front of every collective, the tests' virtual ranks
// (XM_SHARD_FAKE_RANKS) and fault injection (XM_SHARD_FAIL_AT) -- is xm_shard_peers.hpp; this file owns the devices, their
// threads and the frame's start / done hand-shake.  The rule that goes with it: everything that can fail on the host happens in
// front of an agreement (the exchanges hand their return codes to ShardPeers::enter), and a thread that leaves the frame with an
// error anywhere else poisons the agreement on its way out (sharded_thread_main), so that no peer waits for it.
#pragma once

struct xm_sharded {
  explicit xm_sharded(int world) : team(world) {}
  struct Dev {
    int id = 0;
    xm_handle* h = nullptr;
    ShardPeers peers;
    Event ev[4];                   // device 0: around the two collectives
    DevBuf x, y, t, p, depth, bgr;
    DevBuf send, gathered;         // columns exchange: this device's header + last events, every device's
    DevMem<uint16_t> frame16;      // columns exchange: the plain u16 disparity frame (+ the boundary pass' scratch)
    int flagged = 0;               // columns exchange: this device's piece could not be handled
    DevMem<uint64_t> key;
    DevMem<long long> mm;          // {tmin, -tmax} of the shard, then of the frame (16 bytes, int64 or float64)
    long long mm_back[2] = {0, 0}; // device 0: the frame's {tmin, -tmax} copied back (the copy outlives an early return: not on the stack)
    std::thread th;
    int rc = XM_OK;
    std::string err;
  };
  std::vector<std::unique_ptr<Dev>> devs;
  RcclApi rccl;
  bool use_rccl = false;
  ShardTeam team;                  // the device threads' agreement; the tests' virtual ranks and fault injection
  // the frame in flight (set by xm_sharded_process_frame, read by the device threads)
  const uint16_t *x = nullptr, *y = nullptr;
  const void* t = nullptr;
  const int16_t* p = nullptr;
  size_t n = 0;
  int t_dtype = XM_T_INT64;
  float* depth_out = nullptr;
  uint8_t* bgr_out = nullptr;
  u32 tag = 0;
  // the exchange of the frame in flight: every time column on one device + SUM of u16 frames (xm_shard_cols_*), or packed keys
  bool cols_now = false;
  size_t cols_frame_bytes = 0;
  ShardColsBufs cols;              // (the sizes; every device fills in its own buffers)
  unsigned long long frames_columns = 0, frames_keys = 0, frames_redone = 0;
  double mm_host[2] = {0, 0};
  float coll_ms[2] = {0, 0};
  // start / done hand-shake
  std::mutex mu;
  std::condition_variable cv;
  unsigned long long gen = 0;
  int done = 0;
  bool stop = false;
};

namespace {

int sharded_frame_on(xm_sharded* s, int g) {
  xm_sharded::Dev& d = *s->devs[g];
  const int W = (int)s->devs.size();
  const bool cols = s->cols_now;
  HIP_TRY(hipSetDevice(d.id));
  hipStream_t st = (hipStream_t)xm_stream(d.h, 0);
  const size_t a = (size_t)(((unsigned __int128)g * s->n) / (unsigned)W), b = (size_t)(((unsigned __int128)(g + 1) * s->n) / (unsigned)W);
  const size_t m = b - a, tsz = t_size(s->t_dtype), px = (size_t)d.h->plan().dims.out_w * d.h->plan().dims.out_h;
  // 1. the shard and what the exchange needs.  The columns exchange wants cap + 8 events of headroom in front of the shard (the
  // predecessor's last column is copied there on the device) and 8 behind it.
  const size_t head = cols ? s->cols.cap + 8 : 0, tail = cols ? 8 : 0;
  ShardColsBufs bufs = s->cols;
  const auto stage = [&]() -> int {
    int rc;
    if ((rc = stage_in(d.x, s->x + a, m * 2, st, head * 2, tail * 2))) return rc;
    if ((rc = stage_in(d.y, s->y + a, m * 2, st, head * 2, tail * 2))) return rc;
    if ((rc = stage_in(d.t, (const char*)s->t + a * tsz, m * tsz, st, head * tsz, tail * tsz))) return rc;
    if (s->p && (rc = stage_in(d.p, s->p + a, m * 2, st))) return rc;
    if (g == 0 && s->depth_out && (rc = d.depth.reserve(px * 4))) return rc;
    if (g == 0 && s->bgr_out && (rc = d.bgr.reserve(px * 3))) return rc;
    if (!cols) return XM_OK;
    if ((rc = d.send.reserve(bufs.send_bytes)) || (rc = d.gathered.reserve(bufs.send_bytes * (size_t)W))) return rc;
    if (!d.frame16) {
      HIP_TRY(d.frame16.alloc((s->cols_frame_bytes + 1) / sizeof(uint16_t)));
      HIP_TRY(hipMemsetAsync(d.frame16, 0, s->cols_frame_bytes, st));
    }
    bufs.send = d.send.p, bufs.gathered = d.gathered.p, bufs.frame16 = d.frame16;
    return XM_OK;
  };
  // 2. the exchange; what the staging returned reaches its first agreement
  int rc = stage();
  uint16_t *dx = rc ? nullptr : (uint16_t*)d.x.p + head, *dy = rc ? nullptr : (uint16_t*)d.y.p + head;
  char* dt = rc ? nullptr : (char*)d.t.p + head * tsz;
  float* dd = g == 0 && s->depth_out ? (float*)d.depth.p : nullptr;  // (device 0 alone asks for the frame)
  uint8_t* db = g == 0 && s->bgr_out ? (uint8_t*)d.bgr.p : nullptr;
  if (cols) rc = shard_exchange_columns(d.peers, d.h, dx, dy, (int64_t*)dt, m, s->n, W, bufs, dd, db, rc);
  else rc = shard_exchange_keys(d.peers, d.h, dx, dy, dt, s->p ? (const int16_t*)d.p.p : nullptr, m, s->t_dtype, (uint64_t)a, d.mm, d.key, s->tag, dd, db, rc);
  if (rc) return rc;
  // 3. device 0: the outputs and the frame's {tmin, -tmax} (columns: prepare left them in the handle); the columns' verdict
  if (g == 0) {
    if (dd) HIP_TRY(hipMemcpyAsync(s->depth_out, dd, px * 4, hipMemcpyDeviceToHost, st));
    if (db) HIP_TRY(hipMemcpyAsync(s->bgr_out, db, px * 3, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(d.mm_back, cols ? (const void*)d.h->d_shard_n.get() : (const void*)d.mm.get(), 16, hipMemcpyDeviceToHost, st));
  }
  if (!cols) HIP_TRY(hipStreamSynchronize(st));
  else if ((rc = xm_shard_cols_failed(d.h, &d.flagged))) {  // (synchronises the stream)
    (void)hipStreamSynchronize(st);
    return rc;
  }
  if (g == 0) {
    double v[2] = {(double)d.mm_back[0], (double)d.mm_back[1]};
    if (s->t_dtype != XM_T_INT64) memcpy(v, d.mm_back, 16);
    s->mm_host[0] = v[0];
    s->mm_host[1] = -v[1];
    HIP_TRY(hipEventElapsedTime(&s->coll_ms[0], d.ev[0], d.ev[1]));
    HIP_TRY(hipEventElapsedTime(&s->coll_ms[1], d.ev[2], d.ev[3]));
  }
  return XM_OK;
}

void sharded_thread_main(xm_sharded* s, int g) {
  xm_sharded::Dev& d = *s->devs[g];
  unsigned long long seen = 0;
  for (;;) {
    {
      std::unique_lock<std::mutex> lk(s->mu);
      s->cv.wait(lk, [&] { return s->stop || s->gen != seen; });
      if (s->stop) return;
      seen = s->gen;
    }
    d.peers.peer_only = false;
    d.flagged = 0;
    d.rc = sharded_frame_on(s, g);
    if (d.rc) d.err = g_err;
    s->team.agreement.leave(d.rc);  // (an error return outside an agreement point must not leave the peers waiting at the next one)
    {
      std::lock_guard<std::mutex> lk(s->mu);
      s->done += 1;
    }
    s->cv.notify_all();
  }
}

}  // namespace

extern "C" {

void xm_sharded_destroy(xm_sharded* s) {
  if (!s) return;
  {
    std::lock_guard<std::mutex> lk(s->mu);
    s->stop = true;
  }
  s->cv.notify_all();
  for (auto& d : s->devs)
    if (d->th.joinable()) d->th.join();
  for (auto& d : s->devs) {
    (void)hipSetDevice(d->id);
    if (d->h) (void)xm_sync(d->h);  // (the device thread launched on the handle's streams only)
    if (d->peers.comm && s->rccl.CommDestroy) (void)s->rccl.CommDestroy(d->peers.comm);
    if (d->h) xm_destroy(d->h);
    d.reset();  // the device's own buffers and events, while it is the current device
  }
  delete s;
}

int xm_create_sharded(const int* dev_ids, int n_dev, const xm_config* cfg, xm_sharded** out) {
  if (!dev_ids || n_dev <= 0 || !cfg || !out) return fail(XM_ERR_INVALID, "bad argument");
  *out = nullptr;
  int have = 0;
  if (hipGetDeviceCount(&have) != hipSuccess || have <= 0) return fail(XM_ERR_HIP, "no AMD GPU visible");
  for (int i = 0; i < n_dev; ++i) {
    if (dev_ids[i] < 0 || dev_ids[i] >= have) return fail(XM_ERR_INVALID, "device %d is not one of the %d visible", dev_ids[i], have);
    for (int j = 0; j < i; ++j)
      if (dev_ids[j] == dev_ids[i]) return fail(XM_ERR_INVALID, "device %d is listed twice", dev_ids[i]);
  }
  std::vector<int> ids(dev_ids, dev_ids + n_dev);
  const char* fr = dbg_opt("XM_SHARD_FAKE_RANKS");  // tests: W virtual ranks on the one device (xm_shard_peers.hpp)
  if (fr) {
    const int W = atoi(fr);
    if (n_dev != 1 || W < 1 || W > 64) return fail(XM_ERR_INVALID, "XM_SHARD_FAKE_RANKS = %s needs n_dev == 1 and 1 <= W <= 64", fr);
    ids.assign(W, dev_ids[0]);
    n_dev = W;
  }
  dev_ids = ids.data();
  Owned<xm_sharded, xm_sharded_destroy> s(new (std::nothrow) xm_sharded(n_dev));
  if (!s) return fail(XM_ERR_NOMEM, "out of host memory");
  s->team.fake = fr && n_dev > 1;
  if (const char* fa = dbg_opt("XM_SHARD_FAIL_AT")) {
    if (sscanf(fa, "%d:%d", &s->team.fail_rank, &s->team.fail_point) != 2) s->team.fail_rank = -1;
  }
  s->rccl = load_rccl();
  s->use_rccl = !s->team.fake && s->rccl.ok();
  if (n_dev > 1 && !s->use_rccl && !s->team.fake)
    return fail(XM_ERR_INVALID, "librccl was not found: a sharded handle over %d devices needs it", n_dev);
  int rc = XM_OK;
  for (int i = 0; i < n_dev && !rc; ++i) {
    s->devs.emplace_back(new xm_sharded::Dev());
    xm_sharded::Dev& d = *s->devs.back();
    d.id = dev_ids[i];
    d.peers.rccl = &s->rccl;
    d.peers.rank = i;
    d.peers.team = &s->team;
    if (i == 0) d.peers.ev = d.ev;
    xm_config c = *cfg;
    c.device = d.id;
    if ((rc = xm_create(&c, &d.h))) break;
    hipError_t e = hipSetDevice(d.id);
    if (e == hipSuccess) e = d.key.alloc(d.h->plan().dims.key_cells);
    if (e == hipSuccess) e = d.mm.alloc(2);
    for (Event& ev : d.ev)
      if (e == hipSuccess) e = ev.create(hipEventDefault);
    if (e == hipSuccess && s->team.fake) e = d.peers.fake_ptrs.alloc(64);
    if (e != hipSuccess) rc = fail(XM_ERR_HIP, "device %d: %s", d.id, hipGetErrorString(e));
  }
  if (!rc && s->use_rccl) {  // one communicator per device, all in this process
    std::vector<void*> comms(n_dev, nullptr);
    const int e = s->rccl.CommInitAll(comms.data(), n_dev, dev_ids);
    if (e) rc = fail(XM_ERR_HIP, "ncclCommInitAll failed: %s", s->rccl.err(e));
    else
      for (int i = 0; i < n_dev; ++i) s->devs[i]->peers.comm = comms[i];
  }
  if (rc) {
    const std::string keep = g_err;  // (the destroy function's own calls may overwrite it)
    s.reset();
    return fail(rc, "%s", keep.c_str());
  }
  for (int i = 0; i < n_dev; ++i) s->devs[i]->th = std::thread(sharded_thread_main, s.get(), i);
  *out = s.release();
  return XM_OK;
}

int xm_sharded_process_frame(xm_sharded* s, const uint16_t* x, const uint16_t* y, const void* t, const int16_t* p, size_t n, int t_dtype,
                             float* depth_out, uint8_t* bgr_out, xm_frame_stats* stats) {
  if (!s || (n && (!x || !y || !t))) return fail(XM_ERR_INVALID, "NULL argument");
  if (t_dtype != XM_T_INT64 && t_dtype != XM_T_FLOAT32 && t_dtype != XM_T_FLOAT64) return fail(XM_ERR_INVALID, "unknown t_dtype");
  if (n >= XM_KEY_MAX_EVENTS) return fail(XM_ERR_TOO_MANY, "a frame of %zu events exceeds the packed keys' 2^%d", n, XM_KEY_IDX_BITS);
  s->x = x; s->y = y; s->t = t; s->p = p; s->n = n; s->t_dtype = t_dtype;
  s->depth_out = depth_out;
  s->bgr_out = bgr_out;
  s->tag = s->tag >= 1000 ? 1 : s->tag + 1;  // (the key frames are cleared every frame: any tag in [1, 2^19) would do)
  const auto run_frame = [&]() -> int {
    s->team.agreement.reset();  // (the device threads are idle: the frame starts clean, whatever the last frame left)
    {
      std::lock_guard<std::mutex> lk(s->mu);
      s->done = 0;
      s->gen += 1;
    }
    s->cv.notify_all();
    {
      std::unique_lock<std::mutex> lk(s->mu);
      s->cv.wait(lk, [&] { return s->done == (int)s->devs.size(); });
    }
    for (int pass = 0; pass < 2; ++pass)  // (the device that failed first, not the ones that stopped because of it)
      for (size_t i = 0; i < s->devs.size(); ++i) {
        auto& d = s->devs[i];
        if (d->rc && (pass == 1 || !d->peers.peer_only)) return fail(d->rc, "device %d (index %zu): %s", d->id, i, d->err.c_str());
      }
    return XM_OK;
  };
  // Time-sorted int64 frames on rigs whose X-map is injective take the columns exchange (2-byte cells on the wire, no atomics,
  // no extrema pass); a frame one of whose pieces objects (a shard inside one column, events out of order ...) is redone with
  // the packed keys -- as is everything else.
  const char* force = dbg_opt("XM_SHARDED_KEYS");
  s->cols_now = t_dtype == XM_T_INT64 && !p && n >= 64 * s->devs.size() && !(force && force[0] == '1') &&
                (!s->use_rccl || s->rccl.AllGather) &&
                xm_shard_cols_info(s->devs[0]->h, n, &s->cols_frame_bytes, &s->cols.reduce_u32, &s->cols.send_bytes, &s->cols.cap) == XM_OK;
  int rc = run_frame();
  if (rc) return rc;
  if (s->cols_now) {
    bool flagged = false;
    for (auto& d : s->devs) flagged = flagged || d->flagged;
    s->frames_columns += 1;
    if (flagged) {
      s->frames_redone += 1;
      s->cols_now = false;
      if ((rc = run_frame())) return rc;
    }
  } else {
    s->frames_keys += 1;
  }
  if (stats) {
    memset(stats, 0, sizeof *stats);
    stats->n_events = n;
    stats->n_used = n;
    stats->t_min = n ? s->mm_host[0] : 0.0;
    stats->t_max = n ? s->mm_host[1] : 0.0;
    stats->gpu_ms[0] = s->coll_ms[0];  // the two collectives on device 0's stream (HIP events around them)
    stats->gpu_ms[1] = s->coll_ms[1];
  }
  return XM_OK;
}

int xm_sharded_stats(xm_sharded* s, uint64_t* frames_columns, uint64_t* frames_keys, uint64_t* frames_redone) {
  if (!s) return fail(XM_ERR_INVALID, "NULL argument");
  if (frames_columns) *frames_columns = s->frames_columns;
  if (frames_keys) *frames_keys = s->frames_keys;
  if (frames_redone) *frames_redone = s->frames_redone;
  return XM_OK;
}

int xm_sharded_info(xm_sharded* s, int* n_dev, int* uses_rccl, uint64_t* key_frame_bytes) {
  if (!s) return fail(XM_ERR_INVALID, "NULL argument");
  if (n_dev) *n_dev = (int)s->devs.size();
  if (uses_rccl) *uses_rccl = s->use_rccl ? 1 : 0;
  if (key_frame_bytes) *key_frame_bytes = (uint64_t)s->devs[0]->h->plan().dims.key_cells * 8;
  return XM_OK;
}

}  // extern "C"
