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
//
// Also here: the prologue of the two frame entries on the handle (xm_frames_to_time_surfaces, xm_frames_to_point_clouds), which
// take a group of frames as offsets into one record array: frame_spans, frame_records, frame_seq_fill.
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

// ---- the frame entries' prologue: a group of frames in ONE array of EventCD records (xm_frames_to_time_surfaces / _point_clouds) ----

struct FrameSpans {
  u64 ev0 = 0, n_total = 0, n_max = 0;  // the group's first record, its records, the records of its longest frame
};

// offsets_host[0 .. n_frames] (not NULL) against the record array.  A frame holds at most 2^32 - 2 events, the group fewer than
// total_limit (0: no limit of its own); `too_many` is the entry's own text for either.
int frame_spans(const void* eventcd16, const uint64_t* offsets_host, int n_frames, int mem, u64 total_limit, const char* too_many,
                FrameSpans* out) {
  FrameSpans sp;
  for (int f = 0; f < n_frames; ++f) {
    if (offsets_host[f + 1] < offsets_host[f]) return fail(XM_ERR_INVALID, "offsets must not decrease (frame %d)", f);
    sp.n_max = std::max<u64>(sp.n_max, offsets_host[f + 1] - offsets_host[f]);
  }
  sp.ev0 = offsets_host[0], sp.n_total = offsets_host[n_frames] - sp.ev0;
  if (sp.n_max >= 0xffffffffull || (total_limit && sp.n_total >= total_limit)) return fail(XM_ERR_TOO_MANY, "%s", too_many);
  if (sp.n_total && !eventcd16) return fail(XM_ERR_INVALID, "NULL argument");
  if (mem != XM_MEM_HOST && ((uintptr_t)eventcd16 & 15)) return fail(XM_ERR_INVALID, "the record array must be 16-byte aligned");
  *out = sp;
  return XM_OK;
}

// the records the kernels read: the caller's from ev0 on, or their copy in `in` (host memory; enqueued on `stream`)
int frame_records(const void* eventcd16, const FrameSpans& sp, bool host, DevBuf& in, hipStream_t stream, const uint4** d_ev) {
  *d_ev = (const uint4*)eventcd16 + sp.ev0;
  if (!host) return XM_OK;
  if (sp.n_total) HIP_TRY(hipMemcpyAsync(in.p, *d_ev, (size_t)sp.n_total * 16, hipMemcpyHostToDevice, stream));
  *d_ev = (const uint4*)in.p;
  return XM_OK;
}

// frames [f0, f0 + nf) as one launch sequence: first[] relative to ev0 and n[]; returns the longest frame's count
u64 frame_seq_fill(const uint64_t* offsets_host, u64 ev0, size_t f0, unsigned nf, u64* first, u32* n) {
  u64 seq_max = 0;
  for (unsigned k = 0; k < nf; ++k) {
    first[k] = offsets_host[f0 + k] - ev0;
    n[k] = (u32)(offsets_host[f0 + k + 1] - offsets_host[f0 + k]);
    seq_max = std::max<u64>(seq_max, n[k]);
  }
  return seq_max;
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
