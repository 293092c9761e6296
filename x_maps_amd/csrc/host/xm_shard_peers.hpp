// xm_shard_peers.hpp -- how one rank of a sharded frame reaches its peers: RCCL looked up at run time (RcclApi), the virtual
// ranks' collectives on one device, and ShardPeers; the two exchanges that merge a frame's shards, written once against it for
// the device threads of an in-process handle (xm_api_sharded.hpp) and for one rank per process (xm_api_shardcomm.hpp) alike
// (part of libxmaps_hip.so's host side: included by ../xmaps_hip.hip, one translation unit; see that file for the order)
//
// RCCL is not linked: librccl is looked up at run time (the copy a host process has loaded already -- PyTorch ships its own --
// else ROCm's), so that the library keeps loading on hosts without it; the create functions report its absence.
// Failure, in-process: everything that can fail on the host (allocations, launches that report at once) happens in front of an
// AGREEMENT among the device threads (xm_agree.hpp) placed before every collective -- ShardPeers::enter: either every thread
// enters the collective or none does -- no thread is left waiting in RCCL for a peer that has returned.
// Virtual ranks (xm_debug_option("XM_SHARD_FAKE_RANKS", "W"), tests): W ranks on the one device, the collectives emulated by
// agreements + a copy or a reduction kernel over the ranks' buffers (RCCL refuses two ranks on one device).
#pragma once

#include <dlfcn.h>

namespace {

// the few RCCL entry points and enum values used here (rccl.h: ncclDataType_t / ncclRedOp_t)
struct RcclApi {
  void* lib = nullptr;
  struct UniqueId { char bytes[128]; };  // ncclUniqueId: 128 opaque bytes, passed by value
  int (*CommInitAll)(void** comms, int ndev, const int* devlist) = nullptr;
  int (*GetUniqueId)(UniqueId* id) = nullptr;
  int (*CommInitRank)(void** comm, int nranks, UniqueId id, int rank) = nullptr;
  int (*CommDestroy)(void* comm) = nullptr;
  int (*AllReduce)(const void* send, void* recv, size_t count, int dtype, int op, void* comm, hipStream_t stream) = nullptr;
  int (*AllGather)(const void* send, void* recv, size_t sendcount, int dtype, void* comm, hipStream_t stream) = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
  static constexpr int Uint8 = 1, Int32 = 2, Int64 = 4, Uint64 = 5, Float64 = 8, Sum = 0, Max = 2, Min = 3;
  bool ok() const { return CommInitAll && CommDestroy && AllReduce; }
  bool ok_ranks() const { return ok() && GetUniqueId && CommInitRank && AllGather; }
  const char* err(int e) const { return GetErrorString ? GetErrorString(e) : "?"; }
};

RcclApi load_rccl() {
  RcclApi r;
  const char* loaded[] = {"librccl.so.1", "librccl.so"};
  for (const char* n : loaded)
    if (!r.lib) r.lib = dlopen(n, RTLD_NOW | RTLD_NOLOAD);  // a copy the process has already (PyTorch's)
  const char* fresh[] = {"/opt/rocm/lib/librccl.so.1", "librccl.so.1", "librccl.so"};
  for (const char* n : fresh)
    if (!r.lib) r.lib = dlopen(n, RTLD_NOW | RTLD_LOCAL);
  if (!r.lib) return r;
  r.CommInitAll = reinterpret_cast<decltype(r.CommInitAll)>(dlsym(r.lib, "ncclCommInitAll"));
  r.GetUniqueId = reinterpret_cast<decltype(r.GetUniqueId)>(dlsym(r.lib, "ncclGetUniqueId"));
  r.CommInitRank = reinterpret_cast<decltype(r.CommInitRank)>(dlsym(r.lib, "ncclCommInitRank"));
  r.AllGather = reinterpret_cast<decltype(r.AllGather)>(dlsym(r.lib, "ncclAllGather"));
  r.CommDestroy = reinterpret_cast<decltype(r.CommDestroy)>(dlsym(r.lib, "ncclCommDestroy"));
  r.AllReduce = reinterpret_cast<decltype(r.AllReduce)>(dlsym(r.lib, "ncclAllReduce"));
  r.GetErrorString = reinterpret_cast<decltype(r.GetErrorString)>(dlsym(r.lib, "ncclGetErrorString"));
  return r;
}

}  // namespace

namespace xm {
// out[i] = op over r of bufs[r][i]  (virtual ranks: every buffer lives on the one device)
template <typename T, int OP>  // OP: 0 sum, 1 max, 2 min
__global__ __launch_bounds__(256) void k_fake_reduce(const T* const* __restrict__ bufs, int W, size_t n, T* __restrict__ out) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    T v = bufs[0][i];
    for (int r = 1; r < W; ++r) {
      const T u = bufs[r][i];
      v = OP == 0 ? (T)(v + u) : OP == 1 ? (u > v ? u : v) : (u < v ? u : v);
    }
    out[i] = v;
  }
}
}  // namespace xm

namespace {

// what the device threads of one in-process handle share
struct ShardTeam {
  explicit ShardTeam(int world) : agreement(world), cur(world, nullptr) {}
  Agreement agreement;
  bool fake = false;                  // XM_SHARD_FAKE_RANKS: virtual ranks on one device, collectives emulated
  int fail_rank = -1, fail_point = 0; // XM_SHARD_FAIL_AT (tests)
  std::vector<const void*> cur;       // virtual ranks: the buffer each rank brings to the collective in flight
};

template <typename T, int OP>
void launch_fake_reduce(const void* bufs, int W, size_t n, void* out, hipStream_t st) {
  const unsigned gx = (unsigned)std::min<size_t>(4096, (n + 255) / 256);
  hipLaunchKernelGGL((k_fake_reduce<T, OP>), dim3(gx ? gx : 1), dim3(256), 0, st, (const T* const*)bufs, W, n, (T*)out);
}

// One rank's way to its peers.  Per process: rccl + comm, nothing else.  In-process: team as well (and comm == nullptr for the
// virtual ranks, or for a world of one on a host without RCCL, whose collectives are no-ops).
struct ShardPeers {
  const RcclApi* rccl = nullptr;
  void* comm = nullptr;
  int rank = 0;
  ShardTeam* team = nullptr;
  bool peer_only = false;           // this frame: the rank itself was fine, it stopped because a peer had failed
  Event* ev = nullptr;              // rank 0 of an in-process handle: the four events around the two collectives (mark)
  DevBuf fake_tmp;                  // virtual ranks: the reduction's result before it replaces the rank's own buffer
  DevMem<const void*> fake_ptrs;    // virtual ranks: device array of the ranks' buffers

  // (a peer failed: this thread has nothing to report itself -- xm_sharded_process_frame reports the peer's error, not this one)
  int agree(int rc) {
    const int agreed = team->agreement.agree(rc);
    if (!agreed || rc) return rc;
    peer_only = true;
    return fail(agreed, "another device of the sharded handle failed in front of a collective");
  }

  // What precedes collective `point` (1, 2) of a frame, rc being what the host work in front of it returned: 0 lets the rank
  // enter the collective.  Fault injection for the tests: xm_debug_option("XM_SHARD_FAIL_AT", "<device index>:<point>") makes
  // that device thread fail in front of collective <point> (1: the first of the frame, 2: the second; 3: BEHIND the first
  // agreement, i.e. outside any agreement point -- its peers are then on their way into the collective and must be woken by the
  // poisoned agreement) -- read when the handle is created.
  int enter(int point, int rc) {
    if (!team) return rc;
    const auto injected = [&](int pt) { return team->fail_rank == rank && team->fail_point == pt; };
    if (!rc && injected(point)) rc = fail(XM_ERR_HIP, "injected failure (XM_SHARD_FAIL_AT) on device index %d in front of collective %d", rank, point);
    if ((rc = agree(rc))) return rc;
    if (point == 1 && injected(3))
      return fail(XM_ERR_HIP, "injected failure (XM_SHARD_FAIL_AT) on device index %d BEHIND the agreement, outside any agreement point", rank);
    return XM_OK;
  }

  int mark(int i, hipStream_t st) {
    if (ev) HIP_TRY(hipEventRecord(ev[i], st));
    return XM_OK;
  }

  // virtual ranks, either side of a collective: what this rank enqueued is complete (the stream synchronised), everybody agrees
  int fake_meet(int rc, hipStream_t st) {
    if (!rc && hipStreamSynchronize(st) != hipSuccess) rc = fail(XM_ERR_HIP, "hipStreamSynchronize failed");
    return agree(rc);
  }

  // *gathered: where the ranks' `bytes` each stand in rank order -- recv, or send itself where there is nobody to gather from
  int all_gather(const void* send, void* recv, size_t bytes, hipStream_t st, const void** gathered) {
    *gathered = recv;
    if (comm) {
      const int e = rccl->AllGather(send, recv, bytes, RcclApi::Uint8, comm, st);
      return e ? fail(XM_ERR_HIP, "ncclAllGather(%zu bytes) failed: %s", bytes, rccl->err(e)) : XM_OK;
    }
    if (!team || !team->fake) return *gathered = send, XM_OK;
    // virtual ranks: meet, read everybody's buffer on the own stream, meet (nobody overwrites a buffer a peer is still reading)
    team->cur[rank] = send;
    int rc = fake_meet(XM_OK, st);
    if (rc) return rc;
    for (size_t r = 0; r < team->cur.size() && !rc; ++r)
      if (hipMemcpyAsync((char*)recv + r * bytes, team->cur[r], bytes, hipMemcpyDeviceToDevice, st) != hipSuccess)
        rc = fail(XM_ERR_HIP, "hipMemcpyAsync (virtual all-gather) failed");
    return fake_meet(rc, st);
  }

  // in place; dtype / op: RcclApi's
  int all_reduce(void* buf, size_t count, int dtype, int op, hipStream_t st) {
    if (comm) {
      const int e = rccl->AllReduce(buf, buf, count, dtype, op, comm, st);
      return e ? fail(XM_ERR_HIP, "ncclAllReduce(op %d, %zu of type %d) failed: %s", op, count, dtype, rccl->err(e)) : XM_OK;
    }
    if (!team || !team->fake) return XM_OK;
    // virtual ranks: as above, the result into fake_tmp first, into the rank's own buffer once everybody has read everybody's
    const int W = (int)team->cur.size();
    const size_t bytes = count * (dtype == RcclApi::Int32 ? 4 : 8);
    team->cur[rank] = buf;
    int rc = fake_meet(fake_tmp.reserve(bytes), st);
    if (rc) return rc;
    if (hipMemcpyAsync(fake_ptrs, team->cur.data(), sizeof(void*) * W, hipMemcpyHostToDevice, st) != hipSuccess) rc = fail(XM_ERR_HIP, "hipMemcpyAsync failed");
    else if (dtype == RcclApi::Int32 && op == RcclApi::Sum) launch_fake_reduce<u32, 0>(fake_ptrs, W, count, fake_tmp.p, st);
    else if (dtype == RcclApi::Int64 && op == RcclApi::Min) launch_fake_reduce<long long, 2>(fake_ptrs, W, count, fake_tmp.p, st);
    else if (dtype == RcclApi::Float64 && op == RcclApi::Min) launch_fake_reduce<double, 2>(fake_ptrs, W, count, fake_tmp.p, st);
    else if (dtype == RcclApi::Uint64 && op == RcclApi::Max) launch_fake_reduce<unsigned long long, 1>(fake_ptrs, W, count, fake_tmp.p, st);
    else rc = fail(XM_ERR_INVALID, "the virtual ranks have no all-reduce of type %d with op %d", dtype, op);
    if (!rc && hipGetLastError() != hipSuccess) rc = fail(XM_ERR_HIP, "virtual all-reduce kernel failed");
    if ((rc = fake_meet(rc, st))) return rc;
    if (hipMemcpyAsync(buf, fake_tmp.p, bytes, hipMemcpyDeviceToDevice, st) != hipSuccess) return fail(XM_ERR_HIP, "hipMemcpyAsync failed");
    return XM_OK;
  }
};

}  // namespace

// ---- the two exchanges that merge a frame's shards, once for every caller -----------------------------------------------------
// Everything goes onto the handle's stream (the calls between the collectives: xm_api_shard.hpp).  `staged` is what the caller's
// own work in front returned (its allocations, the shard's way to the device): it reaches the first agreement like every other
// failure on the host.  Only a caller that wants the frame passes depth_out / bgr_out (device): the frame kernel runs for it alone.
namespace {

struct ShardColsBufs {  // xm_shard_cols_info's sizes and the buffers that have them
  size_t cap = 0, send_bytes = 0, reduce_u32 = 0;
  void *send = nullptr, *gathered = nullptr;
  uint16_t* frame16 = nullptr;
};

// columns: pack -> all-gather (headers + last events) -> prepare + boundary pass + column-tile K1 -> all-reduce SUM of the u16
// frame (as int32 pairs) -> frame kernel
int shard_exchange_columns(ShardPeers& P, xm_handle* h, uint16_t* x, uint16_t* y, int64_t* t, size_t n_own, uint64_t n_frame, int world,
                           const ShardColsBufs& b, float* depth_out, uint8_t* bgr_out, int staged) {
  hipStream_t st = h->slots[0].stream;
  int rc = staged;
  if (!rc) rc = xm_shard_cols_pack(h, x, y, t, n_own, b.send, b.cap);
  if (!rc) rc = P.mark(0, st);
  if ((rc = P.enter(1, rc))) return rc;
  const void* gathered = nullptr;
  if ((rc = P.all_gather(b.send, b.gathered, b.send_bytes, st, &gathered))) return rc;
  rc = P.mark(1, st);
  if (!rc) rc = xm_shard_cols_scatter(h, x, y, t, n_own, n_frame, gathered, b.send_bytes, P.rank, world, b.cap, b.frame16);
  if (!rc) rc = P.mark(2, st);
  if ((rc = P.enter(2, rc))) return rc;
  if ((rc = P.all_reduce(b.frame16, b.reduce_u32, RcclApi::Int32, RcclApi::Sum, st))) return rc;
  if ((rc = P.mark(3, st))) return rc;
  return depth_out || bgr_out ? xm_shard_finish_u16(h, b.frame16, depth_out, bgr_out) : XM_OK;
}

// keys: extrema -> all-reduce MIN of {tmin, -tmax} -> clear + scatter with global indices -> all-reduce MAX of the packed keys
// -> frame kernel.  MAX over packed keys = the event with the largest GLOBAL index wins = NumPy's last-writer-wins across
// shards, bit for bit.
int shard_exchange_keys(ShardPeers& P, xm_handle* h, const uint16_t* x, const uint16_t* y, const void* t, const int16_t* p, size_t n_own,
                        int t_dtype, uint64_t first_index, void* mm, uint64_t* key, uint32_t tag, float* depth_out, uint8_t* bgr_out,
                        int staged) {
  hipStream_t st = h->slots[0].stream;
  int rc = staged;
  if (!rc) rc = xm_shard_minmax_device(h, t, p, n_own, t_dtype, mm);
  if (!rc) rc = P.mark(0, st);
  if ((rc = P.enter(1, rc))) return rc;
  if ((rc = P.all_reduce(mm, 2, t_dtype == XM_T_INT64 ? RcclApi::Int64 : RcclApi::Float64, RcclApi::Min, st))) return rc;
  rc = P.mark(1, st);
  if (!rc) rc = xm_shard_clear(h, key);
  if (!rc) rc = xm_shard_scatter_device(h, x, y, t, p, n_own, t_dtype, first_index, mm, tag, key);
  if (!rc) rc = P.mark(2, st);
  if ((rc = P.enter(2, rc))) return rc;
  if ((rc = P.all_reduce(key, h->plan().dims.key_cells, RcclApi::Uint64, RcclApi::Max, st))) return rc;
  if ((rc = P.mark(3, st))) return rc;
  return depth_out || bgr_out ? xm_shard_finish(h, key, tag, depth_out, bgr_out) : XM_OK;
}

}  // namespace
