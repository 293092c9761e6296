// xm_res.hpp -- owners of device memory, pinned memory, streams and events
// (part of libxmaps_hip.so's host side: included by ../xmaps_hip.hip, one translation unit; see that file for the order)
//
// THE RULE: nothing is released until every stream that may touch it has been synchronised; the destroy function of the object
// that holds it (xm_destroy, xm_ingest_destroy, ...) does that before `delete`.  The holders never synchronise and never set
// the device: they only release what they own when they go out of scope.  Structs declare their streams and events BEFORE their
// buffers, so that the buffers are released first (members are destroyed in reverse order of declaration).
//
// All four are move-only and convert to the raw handle they own, so launches and HIP calls read as they would with a raw field.
// Structs that kernels take by value or that live in device memory (DevTables, FrameDesc, SlotState, IngestDev, ActDev,
// K2PipeArgs) stay plain: their pointers are views, filled from get().
#pragma once

namespace {

template <typename T>
struct DevMem {  // hipMalloc / hipFree
  T* p = nullptr;
  DevMem() = default;
  DevMem(DevMem&& o) noexcept : p(o.p) { o.p = nullptr; }
  DevMem& operator=(DevMem&& o) noexcept { return std::swap(p, o.p), *this; }
  ~DevMem() { reset(); }
  hipError_t alloc(size_t count, size_t slack_bytes = 0) {  // (whatever it held is released first)
    reset();
    return hipMalloc((void**)&p, count * sizeof(T) + slack_bytes);
  }
  void reset() { if (p) (void)hipFree(p), p = nullptr; }
  T* get() const { return p; }
  operator T*() const { return p; }
  explicit operator bool() const { return p != nullptr; }
};

template <typename T>
struct PinnedMem {  // hipHostMalloc / hipHostFree
  T* p = nullptr;
  PinnedMem() = default;
  PinnedMem(PinnedMem&& o) noexcept : p(o.p) { o.p = nullptr; }
  PinnedMem& operator=(PinnedMem&& o) noexcept { return std::swap(p, o.p), *this; }
  ~PinnedMem() { reset(); }
  hipError_t alloc(size_t count, unsigned flags = hipHostMallocDefault) {
    reset();
    return hipHostMalloc((void**)&p, count * sizeof(T), flags);
  }
  void reset() { if (p) (void)hipHostFree(p), p = nullptr; }
  T* get() const { return p; }
  T* device_ptr() const {  // mapped memory (hipHostMallocMapped): the address kernels use; nullptr on failure
    T* d = nullptr;
    return p && hipHostGetDevicePointer((void**)&d, p, 0) == hipSuccess ? d : nullptr;
  }
  operator T*() const { return p; }
  T* operator->() const { return p; }
  explicit operator bool() const { return p != nullptr; }
};

struct Stream {  // owning (create / create_with_priority) or borrowed (borrow): destroys only what it owns
  hipStream_t s = nullptr;
  bool owned = false;
  Stream() = default;
  Stream(Stream&& o) noexcept : s(o.s), owned(o.owned) { o.s = nullptr, o.owned = false; }
  Stream& operator=(Stream&& o) noexcept { return std::swap(s, o.s), std::swap(owned, o.owned), *this; }
  ~Stream() { reset(); }
  hipError_t create(unsigned flags = hipStreamNonBlocking) {
    reset();
    owned = true;
    return hipStreamCreateWithFlags(&s, flags);
  }
  hipError_t create_with_priority(unsigned flags, int priority) {
    reset();
    owned = true;
    return hipStreamCreateWithPriority(&s, flags, priority);
  }
  void borrow(hipStream_t other) {
    reset();
    s = other;
  }
  void reset() {
    if (s && owned) (void)hipStreamDestroy(s);
    s = nullptr;
    owned = false;
  }
  hipStream_t get() const { return s; }
  operator hipStream_t() const { return s; }
  explicit operator bool() const { return s != nullptr; }
};

struct Event {  // hipEventCreateWithFlags / hipEventDestroy; may be created late
  hipEvent_t e = nullptr;
  Event() = default;
  Event(Event&& o) noexcept : e(o.e) { o.e = nullptr; }
  Event& operator=(Event&& o) noexcept { return std::swap(e, o.e), *this; }
  ~Event() { reset(); }
  hipError_t create(unsigned flags = hipEventDisableTiming) {
    reset();
    return hipEventCreateWithFlags(&e, flags);
  }
  void reset() { if (e) (void)hipEventDestroy(e), e = nullptr; }
  hipEvent_t get() const { return e; }
  operator hipEvent_t() const { return e; }
  explicit operator bool() const { return e != nullptr; }
};

// Create functions hold the new object in one of these and release() it into *out on success: every early `return rc` then
// runs the object's destroy function (which tolerates a half-built object).
template <typename T, void (*Destroy)(T*)>
struct DestroyWith {
  void operator()(T* p) const { Destroy(p); }
};
template <typename T, void (*Destroy)(T*)>
using Owned = std::unique_ptr<T, DestroyWith<T, Destroy>>;

}  // namespace
