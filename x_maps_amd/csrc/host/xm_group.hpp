// xm_group.hpp -- the host skeleton of the group objects: ESL-init, MC3D, ESL depth optimisation, ESL filters, evaluation table
// (part of libxmaps_hip.so's host side: included by ../xmaps_hip.hip, one translation unit; see that file for the order)
//
// A group object is create(device, cfg) -> object, ONE synchronous call per group of maps on XM_MEM_HOST or XM_MEM_DEVICE
// pointers, and destroy.  What all of them do the same way is written here once; an xm_api_*.hpp keeps what is its own:
// config validation and defaults, table building, grid shapes and the launches.  A call reads
//
//   if (int rc = group_enter(e, n, mem, &dtype)) return rc;      the argument check; the object's device is current afterwards
//   GroupCall c{e->stream, mem == XM_MEM_HOST};
//   d_in = c.in(e->in, user_in, bytes);                          device pointers to launch on (staging when the caller's are host)
//   d_out = c.out(e->out, user_out, bytes);
//   if (int rc = c.start({{e->scratch, bytes}, ...})) return rc; scratch grows; the first failure so far comes out here
//   by_dtype(dtype, [&](auto t) { using T = decltype(t); hipLaunchKernelGGL((k<T>), ...); });
//   HIP_TRY(hipGetLastError());
//   c.back(stats_out, d_stats, bytes);
//   return c.finish();                                           the copies back, then the stream is synchronised
//
// Every call is synchronous, so nothing in flight can still use a buffer that grows, and a call that fails on memory waits for
// the copies in it has already enqueued: nothing that reads the caller's memory is left behind on the stream.
//
// LAUNCHES: the group objects launch with plain hipLaunchKernelGGL, not XM_LAUNCH.  XM_LAUNCH stamps the events of
// xm_profile_frame (g_prof, per thread) on a dispatch; that is a mode of the handle, which a group object does not have, and a
// group call made on a thread while a handle's frame is being profiled there must not write into that frame's events.
// xm_process_time_surfaces is a call on the handle and keeps XM_LAUNCH.
#pragma once

namespace {

struct GroupObj {  // the base of a group object: declared before any buffer of the object (xm_res.hpp's rule: released after them)
  int device = 0;
  Stream stream;
  // what group_enter holds a call's n against: set by the object's create
  const char* noun = "surfaces";  // "n_surfaces" / "n_maps" in the messages
  size_t px = 0;                  // pixels of one map
  size_t max_n = 65535;           // maps per call: a grid's y / z dimension ends there (0: the object splits a larger group itself)
  int total_log2 = 40;            // n * px stays below 2^this
};

// ---- create / destroy ----

template <typename Cfg, typename T>
int group_create_args(const Cfg* cfg, T** out, const char* cfg_name) {
  if (!cfg || !out) return fail(XM_ERR_INVALID, "NULL argument");
  *out = nullptr;
  if (cfg->struct_size != sizeof(Cfg)) return fail(XM_ERR_INVALID, "%s.struct_size mismatch", cfg_name);
  return XM_OK;
}

// the device is checked and made current, then the object exists with its stream; on failure `o` destroys what there is of it
template <typename T, void (*Destroy)(T*)>
int group_open(int device, Owned<T, Destroy>& o) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(XM_ERR_HIP, "no HIP device visible");
  if (device < 0 || device >= ndev) return fail(XM_ERR_INVALID, "no device %d", device);
  HIP_TRY(hipSetDevice(device));
  o.reset(new (std::nothrow) T);
  if (!o) return fail(XM_ERR_NOMEM, "out of host memory");
  o->device = device;
  HIP_TRY(o->stream.create());
  return XM_OK;
}

template <typename T>
void group_destroy(T* o) {  // (tolerates a half-built object)
  if (!o) return;
  (void)hipSetDevice(o->device);
  if (o->stream) (void)hipStreamSynchronize(o->stream);
  delete o;
}

// ---- the arguments of a group call ----

int group_args(int n, int mem, const int* dtype, const char* noun) {  // (what xm_process_time_surfaces shares with the objects)
  if (dtype && *dtype != XM_T_FLOAT32 && *dtype != XM_T_FLOAT64) return fail(XM_ERR_INVALID, "a time surface is XM_T_FLOAT32 or XM_T_FLOAT64");
  if (n <= 0) return fail(XM_ERR_INVALID, "n_%s must be positive", noun);
  if (mem != XM_MEM_HOST && mem != XM_MEM_DEVICE) return fail(XM_ERR_INVALID, "mem must be XM_MEM_HOST or XM_MEM_DEVICE");
  return XM_OK;
}

int group_enter(const GroupObj* o, int n, int mem, const int* dtype = nullptr) {
  if (!o) return fail(XM_ERR_INVALID, "NULL object");
  if (int rc = group_args(n, mem, dtype, o->noun)) return rc;
  if (o->max_n && (size_t)n > o->max_n) return fail(XM_ERR_TOO_MANY, "group too large (at most %zu %s per call)", o->max_n, o->noun);
  if ((u64)n * o->px >= (1ull << o->total_log2)) return fail(XM_ERR_TOO_MANY, "group too large");
  HIP_TRY(hipSetDevice(o->device));
  return XM_OK;
}

template <typename F>
void by_dtype(int dtype, F&& f) {  // f(float{}) or f(double{}): `using T = decltype(t);` names the surfaces' type in the lambda
  if (dtype == XM_T_FLOAT32) f(float{}); else f(double{});
}

// ---- buffers ----

struct BufNeed {
  DevBuf& buf;
  size_t bytes;  // (0: not needed by this call, left as it is)
};

bool any_grows(std::initializer_list<BufNeed> needs) {
  for (const BufNeed& b : needs)
    if (b.bytes > b.buf.cap) return true;
  return false;
}

int reserve_all(std::initializer_list<BufNeed> needs) {
  for (const BufNeed& b : needs)
    if (b.bytes)
      if (int rc = b.buf.reserve(b.bytes)) return rc;
  return XM_OK;
}

// ---- staging of one synchronous call ----

struct GroupCall {
  hipStream_t stream;
  bool host;  // the caller's pointers are host memory: everything goes through the object's staging buffers
  struct Copy {
    void* dst;
    const void* src;
    size_t bytes;
    bool to_host;  // dst is host memory whatever the call's `mem` says
  };
  static constexpr int MAX_BACK = 6;  // (the filter's four copies back are the most there are)
  Copy backs[MAX_BACK];
  int n_back = 0, rc = XM_OK;  // rc: the first failure of in() / out() / back(); start() and finish() return it

  int copy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, kind, stream));
    return XM_OK;
  }
  // an input: the pointer the kernels read.  Host memory is copied into `buf` here.
  template <typename T>
  const T* in(DevBuf& buf, const T* user, size_t bytes) {
    if (!host) return user;
    if (!rc) rc = buf.reserve(bytes);
    if (!rc) rc = copy(buf.p, user, bytes, hipMemcpyHostToDevice);
    return static_cast<const T*>(buf.p);
  }
  // an output: the pointer the kernels write.  `user` may be NULL when the output is optional: then there is none (nullptr), unless
  // `needed` says that a later launch reads it, and it goes to `buf`.  Host memory gets `buf`'s content from finish().
  template <typename T>
  T* out(DevBuf& buf, T* user, size_t bytes, bool needed = false) {
    if (user && !host) return user;
    if (!user && !needed) return nullptr;
    if (!rc) rc = buf.reserve(bytes);
    back(user, buf.p, bytes);
    return static_cast<T*>(buf.p);
  }
  // device memory of the object's that the caller may have asked for (stats, counters): copied to `user` by finish(), host or device
  void back(void* user, const void* dev, size_t bytes, bool to_host = false) {
    if (!user || rc) return;
    if (n_back == MAX_BACK) rc = fail(XM_ERR_INVALID, "GroupCall: more than %d copies back", MAX_BACK);
    else backs[n_back++] = Copy{user, dev, bytes, to_host};
  }
  // device memory of the object's that the HOST goes on to use, also in a call on device pointers (the sums a result is made of)
  void back_host(void* host_dst, const void* dev, size_t bytes) { back(host_dst, dev, bytes, true); }
  // the scratch grows; a call that stops here (or in in() / out()) waits for the copies in it has enqueued, which read the caller's memory
  int start(std::initializer_list<BufNeed> scratch) {
    if (!rc) rc = reserve_all(scratch);
    if (rc) (void)hipStreamSynchronize(stream);
    return rc;
  }
  int finish() {
    for (int i = 0; i < n_back && !rc; ++i)
      rc = copy(backs[i].dst, backs[i].src, backs[i].bytes, host || backs[i].to_host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice);
    HIP_TRY(hipStreamSynchronize(stream));
    return rc;
  }
};

}  // namespace
